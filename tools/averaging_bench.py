#!/usr/bin/env python3
"""What the optimizer's options cost per training step (BASELINE config 2: 6+6 layers, d_model 256, V 4337, the seed-0 batch of
32 utterances of 500..1000 frames, graph mode) - same box, same process, ALTERNATELY: --repeats rounds of --steps timed steps
each of
  plain       ScheduledOptim as it always was (st_grad_norm, st_adam_clip),
  guard       enable_nonfinite_guard() (st_grad_norm with a guard, st_adam_clip with found_inf),
  guard_avg   guard + enable_averaging() (the same two launches; the update also reads and writes the averaged copy).
The three steps share the model; each has its own optimizer (the options are per optimizer) and its own captured graph.  As in
bench.py the update runs at a learning rate of zero, so every timed step computes from the same weights - the kernels move the
same bytes either way.  Prints one JSON line and writes it to --out (default profiles/averaging_bench.json): ms per step of
every round, the medians, the spread of the repeats and the differences to plain.  --only plain: that variant alone (it needs
nothing this tool's commit added, so the same file times the parent commit's step from a checkout of it)."""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "speech-tranformer-pytorch_amd")):
    if p not in sys.path:
        sys.path.insert(0, p)
import torch  # noqa: E402

CFG = dict(feature_dim=80, max_inputs_length=1000, max_target_length=50, num_enc_layer=6, num_dec_layer=6, n_heads=4,
           d_k=64, d_v=64, d_model=256, d_inner_hid=1024, dropout=0.1, vocab_size=4337)
VARIANTS = ("plain", "guard", "guard_avg")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=30)
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--only", choices=VARIANTS, default=None)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "averaging_bench.json"))
    args = ap.parse_args()

    import transformer.Models as M
    import transformer.Utils as U
    from st_amd import native as nv
    from st_amd import synthetic
    from st_amd.arena import arena_of
    from st_amd.trainer import TrainStep
    from transformer.Optim import ScheduledOptim

    nv.load(build_if_missing=False)
    torch.manual_seed(0)
    model = M.Transformer(U.AttrDict(CFG))
    U.init_parameters(model)
    model = model.eval().cuda()
    x, tokens, in_len, tgt_len, gt = synthetic.make_batch(32, 1000, 50, CFG["feature_dim"], CFG["vocab_size"], seed=0, t_min=500, l_min=25)
    xg, tg, gg = x.cuda(), tokens.cuda(), gt.cuda()

    variants = [args.only] if args.only else list(VARIANTS)
    steps, optims = {}, {}
    for v in variants:
        optim = ScheduledOptim(model, CFG["d_model"], U.AttrDict(n_warmup_steps=12000))
        optim.update_learning_rate = (lambda o: lambda global_step: o.lr_tensor.fill_(0.0))(optim)
        if v != "plain":
            optim.enable_nonfinite_guard()
        if v == "guard_avg":
            optim.enable_averaging(decay=0.999, warmup=True)
        optims[v] = optim
        steps[v] = TrainStep(model, optim, CFG["vocab_size"], max_grad_norm=5.0, use_graph=True)
    last = {}
    for v in variants:                                     # eager warm-ups, capture, first replays
        for _ in range(5):
            last[v] = steps[v](xg, in_len, tg, tgt_len, gg)
    torch.cuda.synchronize()
    rounds = {v: [] for v in variants}
    for _ in range(args.repeats):
        for v in variants:
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(args.steps):
                last[v] = steps[v](xg, in_len, tg, tgt_len, gg)
            torch.cuda.synchronize()
            rounds[v].append((time.perf_counter() - t0) / args.steps * 1e3)

    out = {"shape": "config 2: B 32, T 500..1000, L 25..50, 6+6 layers, d_model 256, V 4337", "device": torch.cuda.get_device_name(),
           "steps_per_round": args.steps, "graph": True, "arena_mb": round(arena_of(model).total * 4 / 1e6, 2)}
    for v in variants:
        r = sorted(rounds[v])
        out[v] = {"ms_per_step_rounds": [round(t, 4) for t in rounds[v]], "ms_per_step_median": round(r[len(r) // 2], 4),
                  "spread_ms": round(r[-1] - r[0], 4), "graphs": len(steps[v]._graphs),
                  "loss": round(float(last[v][0]), 4), "grad_norm": round(float(last[v][1]), 4)}
        skipped = getattr(optims[v], "skipped", None)
        if skipped is not None:
            out[v]["skipped"] = float(skipped)
    for v in variants:
        if v != "plain" and "plain" in out:
            out[v + "_minus_plain_us"] = round((out[v]["ms_per_step_median"] - out["plain"]["ms_per_step_median"]) * 1e3, 2)
    line = json.dumps(out)
    print(line)
    if args.out and args.out != os.devnull:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
