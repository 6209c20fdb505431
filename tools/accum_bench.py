#!/usr/bin/env python3
"""What gradient accumulation costs, and what it saves (BASELINE config 2: 6+6 layers, d_model 256, V 4337, the seed-0 batch of
32 utterances of 500..1000 frames, graph mode) - same box, same process, ALTERNATELY: --repeats rounds of --windows timed windows
each of
  plain   K non-accumulating steps (TrainStep as it always was: zero_grad, forward, backward, norm, clip + Adam - K times),
  accum   K micro-batches + ONE update (TrainStep(accumulate=K): no zero_grad launch, st_accum_note per micro-batch;
          st_grad_norm, st_adam_clip with the window, st_window_close once).
Both share the model; each has its own optimizer and its own captured graphs.  As in bench.py the update runs at a learning
rate of zero, so every timed step computes from the same weights.  Prints one JSON line and writes it to --out: ms per window of
every round, the medians, the spread of the repeats and accum minus plain.

--only plain: that variant alone - it needs nothing this tool's commit added, so the same file times the PARENT commit's step
from a checkout of it.  The "nothing enabled" gate is a comparison between processes: run this commit and the parent alternately
(one process each, several times, in one session on one box), then --merge the JSON lines into --out: the medians per commit, the
process-to-process spread of each, and their difference."""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "speech-tranformer-pytorch_amd")):
    if p not in sys.path:
        sys.path.insert(0, p)

CFG = dict(feature_dim=80, max_inputs_length=1000, max_target_length=50, num_enc_layer=6, num_dec_layer=6, n_heads=4,
           d_k=64, d_v=64, d_model=256, d_inner_hid=1024, dropout=0.1, vocab_size=4337)
VARIANTS = ("plain", "accum")


def _median(xs):
    xs = sorted(xs)
    return xs[len(xs) // 2]


def merge(paths, out_path):
    """JSON lines of several processes (each tagged with --label) -> one document: per label the plain medians of its processes,
    their spread, and the differences between the labels' medians."""
    runs = []
    for path in paths:
        with open(path) as f:
            runs += [json.loads(line) for line in f if line.strip().startswith("{")]
    labels = sorted({r["label"] for r in runs})
    out = {"shape": runs[0]["shape"], "device": runs[0]["device"], "K": runs[0]["K"], "processes": len(runs), "labels": {}}
    for lab in labels:
        mine = [r for r in runs if r["label"] == lab]
        doc = {}
        for v in VARIANTS:
            meds = [r[v]["ms_per_window_median"] for r in mine if v in r]
            if meds:
                doc[v] = {"ms_per_window_by_process": meds, "median": round(_median(meds), 4),
                          "process_spread_ms": round(max(meds) - min(meds), 4)}
        diffs = [r["accum_minus_plain_us"] for r in mine if "accum_minus_plain_us" in r]
        if diffs:
            doc["accum_minus_plain_us_by_process"] = diffs
            doc["accum_minus_plain_us_median"] = _median(diffs)
        out["labels"][lab] = doc
    if len(labels) == 2:
        a, b = labels
        out["plain_%s_minus_%s_us" % (a, b)] = round((out["labels"][a]["plain"]["median"] - out["labels"][b]["plain"]["median"]) * 1e3, 2)
    line = json.dumps(out)
    print(line)
    with open(out_path, "w") as f:
        f.write(line + "\n")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--windows", type=int, default=8)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("-K", type=int, default=4)
    ap.add_argument("--only", choices=VARIANTS, default=None)
    ap.add_argument("--label", default="this")
    ap.add_argument("--merge", nargs="+", default=None, help="JSON-line files of earlier processes to combine into --out")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "accum_bench.json"))
    args = ap.parse_args()
    if args.merge:
        return merge(args.merge, args.out)

    import torch
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
    K = args.K

    variants = [args.only] if args.only else list(VARIANTS)
    steps = {}
    for v in variants:
        optim = ScheduledOptim(model, CFG["d_model"], U.AttrDict(n_warmup_steps=12000))
        optim.update_learning_rate = (lambda o: lambda global_step: o.lr_tensor.fill_(0.0))(optim)
        kw = dict(accumulate=K) if v == "accum" else {}
        steps[v] = TrainStep(model, optim, CFG["vocab_size"], max_grad_norm=5.0, use_graph=True, **kw)
    last = {}
    for v in variants:                                     # eager warm-ups, capture, first replays: whole windows
        for _ in range(2 * K):
            last[v] = steps[v](xg, in_len, tg, tgt_len, gg)
    torch.cuda.synchronize()
    rounds = {v: [] for v in variants}
    for _ in range(args.repeats):
        for v in variants:
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(args.windows * K):
                last[v] = steps[v](xg, in_len, tg, tgt_len, gg)
            torch.cuda.synchronize()
            rounds[v].append((time.perf_counter() - t0) / args.windows * 1e3)

    out = {"label": args.label, "shape": "config 2: B 32, T 500..1000, L 25..50, 6+6 layers, d_model 256, V 4337",
           "device": torch.cuda.get_device_name(), "K": K, "windows_per_round": args.windows, "graph": True,
           "arena_mb": round(arena_of(model).total * 4 / 1e6, 2)}
    for v in variants:
        r = sorted(rounds[v])
        out[v] = {"ms_per_window_rounds": [round(t, 4) for t in rounds[v]], "ms_per_window_median": round(r[len(r) // 2], 4),
                  "spread_ms": round(r[-1] - r[0], 4), "graphs": len(steps[v]._graphs), "loss": round(float(last[v][0]), 4),
                  "grad_norm": round(float(last[v][1]), 4), "updates": steps[v].global_step}
    if len(variants) == 2:
        out["accum_minus_plain_us"] = round((out["accum"]["ms_per_window_median"] - out["plain"]["ms_per_window_median"]) * 1e3, 2)
    line = json.dumps(out)
    print(line)
    if args.out and args.out != os.devnull:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "a" if os.path.basename(args.out).endswith(".jsonl") else "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
