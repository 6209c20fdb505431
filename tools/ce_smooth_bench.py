#!/usr/bin/env python3
"""The label-smoothed cross-entropy against the plain one, same box, same process, ALTERNATELY.

(1) Kernels at BASELINE config 2's decoder shape (the seed-0 batch's target rows x V 4337, logits [R, v_pad] fp32 with the
    padding columns at -1e30): ``st_ce_fwd + st_ce_bwd`` against ``st_ce_smooth_fwd + st_ce_smooth_bwd`` (the reference's
    LabelSmoothingLoss spec, with its denominator), device events around each pair, --repeats rounds of --iters pairs each.
    Both move the same bytes (forward reads R x V x 4; backward reads that again and writes R x v_pad x 2), so the expectation
    is a ratio inside the spread of the rounds.
(2) TrainStep graph replay on config 2 (6+6 layers, d_model 256, B 32, T 500..1000): ``criterion=None`` against
    ``criterion=LabelSmoothingLoss(0.1, V, ignore_index=0)``, --repeats rounds of --steps steps each; as in bench.py the update
    runs at a learning rate of zero.  Informational.
Prints one JSON line and writes it to --out (default profiles/ce_smooth_bench.json).  --no-step: part (1) only."""
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


def _stats(rounds):
    r = sorted(rounds)
    return {"rounds": [round(v, 5) for v in rounds], "median": round(r[len(r) // 2], 5), "spread": round(r[-1] - r[0], 5)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--no-step", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "ce_smooth_bench.json"))
    args = ap.parse_args()

    import transformer.Models as M
    import transformer.Utils as U
    from st_amd import functional as F_
    from st_amd import native as nv
    from st_amd import synthetic
    from st_amd.trainer import TrainStep
    from transformer.Loss import LabelSmoothingLoss
    from transformer.Optim import ScheduledOptim

    nv.load(build_if_missing=False)
    V = CFG["vocab_size"]
    vp = (V + 7) // 8 * 8
    x, tokens, in_len, tgt_len, gt = synthetic.make_batch(32, 1000, 50, CFG["feature_dim"], V, seed=0, t_min=500, l_min=25)
    R = int(tgt_len.sum())
    spec = F_.ce_spec(LabelSmoothingLoss(0.1, V, ignore_index=0), V)

    # ---- (1) the kernel pairs ------------------------------------------------------------------------------------------
    gen = torch.Generator().manual_seed(0)
    logits = torch.full((R, vp), -1e30)
    logits[:, :V] = torch.randn(R, V, generator=gen) * 3
    target = torch.randint(1, V, (R,), generator=gen)
    target[::20] = 0
    lg, tg = logits.cuda(), target.cuda()
    lse, sums3, sums4 = torch.empty(R, device="cuda"), torch.empty(3, device="cuda"), torch.empty(4, device="cuda")
    dl = torch.empty(R, vp, dtype=torch.bfloat16, device="cuda")
    go = torch.ones(1, device="cuda")
    denom = torch.tensor([float(32 * int(tgt_len.max()))], device="cuda")

    def plain():
        nv.ce_fwd(lg, tg, 0, lse, sums3)
        nv.ce_bwd(lg, tg, 0, lse, sums3, go, dl)

    def smooth():
        nv.ce_smooth_fwd(lg, tg, 0, spec.confidence, spec.smooth, spec.zero_col, lse, sums4, V=V, denom=denom)
        nv.ce_smooth_bwd(lg, tg, 0, spec.confidence, spec.smooth, spec.zero_col, lse, sums4, go, dl, V=V, denom=denom)

    pairs = {"st_ce": plain, "st_ce_smooth": smooth}
    for fn in pairs.values():
        for _ in range(20):
            fn()
    torch.cuda.synchronize()
    rounds = {k: [] for k in pairs}
    for _ in range(args.repeats):
        for k, fn in pairs.items():
            s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            s.record()
            for _ in range(args.iters):
                fn()
            e.record()
            torch.cuda.synchronize()
            rounds[k].append(s.elapsed_time(e) / args.iters * 1e3)
    out = {"shape": "config 2 decoder: R %d rows, V %d (v_pad %d), fp32 logits, bf16 gradient" % (R, V, vp),
           "device": torch.cuda.get_device_name(), "iters_per_round": args.iters,
           "kernels_us_per_fwd_bwd_pair": {k: _stats(v) for k, v in rounds.items()}}
    a, b = out["kernels_us_per_fwd_bwd_pair"]["st_ce"], out["kernels_us_per_fwd_bwd_pair"]["st_ce_smooth"]
    out["smooth_over_plain_ratio"] = round(b["median"] / a["median"], 4)
    out["spread_over_median"] = round(max(a["spread"] / a["median"], b["spread"] / b["median"]), 4)
    out["ratio_inside_the_spread"] = bool(abs(out["smooth_over_plain_ratio"] - 1.0) <= out["spread_over_median"])

    # ---- (2) the captured step -----------------------------------------------------------------------------------------
    if not args.no_step:
        torch.manual_seed(0)
        model = M.Transformer(U.AttrDict(CFG))
        U.init_parameters(model)
        model = model.eval().cuda()
        optim = ScheduledOptim(model, CFG["d_model"], U.AttrDict(n_warmup_steps=12000))
        optim.update_learning_rate = lambda global_step: optim.lr_tensor.fill_(0.0)
        xg, tkg, gg = x.cuda(), tokens.cuda(), gt.cuda()
        steps = {"plain": TrainStep(model, optim, V, max_grad_norm=5.0, use_graph=True),
                 "label_smoothing": TrainStep(model, optim, V, max_grad_norm=5.0, use_graph=True,
                                              criterion=LabelSmoothingLoss(0.1, V, ignore_index=0))}
        last = {}
        for k, st in steps.items():
            for _ in range(5):                      # eager warm-up, capture, first replays
                last[k] = st(xg, in_len, tkg, tgt_len, gg)
        torch.cuda.synchronize()
        srounds = {k: [] for k in steps}
        for _ in range(args.repeats):
            for k, st in steps.items():
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                for _ in range(args.steps):
                    last[k] = st(xg, in_len, tkg, tgt_len, gg)
                torch.cuda.synchronize()
                srounds[k].append((time.perf_counter() - t0) / args.steps * 1e3)
        out["step_ms_per_replay"] = {k: dict(_stats(v), loss=round(float(last[k][0]), 4), nll=round(float(steps[k].nll), 4),
                                             graphs=len(steps[k]._graphs)) for k, v in srounds.items()}
        out["step_smooth_minus_plain_ms"] = round(out["step_ms_per_replay"]["label_smoothing"]["median"]
                                                  - out["step_ms_per_replay"]["plain"]["median"], 4)
    line = json.dumps(out)
    print(line)
    if args.out and args.out != os.devnull:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
