#!/usr/bin/env python3
"""What SpecAugment's time warp costs (BASELINE config 2's seed-0 batch: B 32, 24,060 frames of 500..1000 per utterance), on
one box, in one process.

Per launch (eager, inside native.timing_start/stop; median, p10, p90 of --launches): st_pack_rows, st_pack_rows_aug, the
warping pack st_pack_rows_warp, and the two plan launches st_specaug_plan / st_specaug_plan_warp - at F = 320 (80 bins x 4
context slots, interval 3: the reference's geometry) and at F = 80 (plain frames).  The yardstick of the warping pack is
st_pack_rows_aug on the same input: it writes the same bytes and reads up to two source chunks per output chunk.

Whole step (config 2: 6+6 layers, d_model 256, V 4337; training mode, graph replay, learning rate zero as in bench.py),
ALTERNATELY --repeats rounds of --steps steps each of: no policy, SpecAugment(80), SpecAugment(80, time_warp=80).

Prints one JSON line and writes it to --out (default profiles/timewarp_bench.json)."""
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
VARIANTS = ("none", "masks", "masks_warp")
WARP = 80


def _stats(ms):
    us = sorted(1e3 * t for t in ms)
    return {"median_us": round(us[len(us) // 2], 2), "p10_us": round(us[len(us) // 10], 2), "p90_us": round(us[len(us) * 9 // 10], 2)}


def launches(in_len, n, geometry):
    """One geometry (mel_bins, left, frame_rate) -> {launch: {median_us, p10_us, p90_us}} over n launches each."""
    from st_amd import native as nv
    from st_amd.augment import SpecAugment
    from st_amd.functional import Rows
    bins, left, rate = geometry
    Fd = bins * (1 + left)
    rows = Rows.packed(in_len, "cuda")
    x = torch.randn(in_len.numel(), int(in_len.max()), Fd, device="cuda")
    out = torch.empty(rows.total, Fd, dtype=torch.bfloat16, device="cuda")
    plain = SpecAugment(bins, left=left, frame_rate=rate)
    warp = SpecAugment(bins, left=left, frame_rate=rate, time_warp=WARP)

    def plan(aug):
        aug.plan(rows.len, stacked=True)

    plan(plain), plan(warp)
    calls = {
        "st_pack_rows": lambda: nv.pack_rows(x, rows.off, rows.len, out),
        "st_pack_rows_aug": lambda: nv.pack_rows_aug(x, rows.off, rows.len, out, plain.last_masks, plain.n_time_masks, plain.n_freq_masks,
                                                     bins, left, 0, plain.interval),
        "st_pack_rows_warp": lambda: nv.pack_rows_warp(x, rows.off, rows.len, out, warp.last_masks, warp.last_warp, warp.n_time_masks,
                                                       warp.n_freq_masks, bins, left, 0, warp.interval),
        "st_specaug_plan": lambda: plan(plain),
        "st_specaug_plan_warp": lambda: plan(warp),
    }
    res = {}
    for name, call in calls.items():
        for _ in range(20):
            call()
        torch.cuda.synchronize()
        nv.timing_start()
        for _ in range(n):
            call()
        ms = [t for who, _, t, _ in nv.timing_stop() if who == name]
        assert len(ms) == n, (name, len(ms))
        res[name] = _stats(ms)
    res["warp_over_aug"] = round(res["st_pack_rows_warp"]["median_us"] / res["st_pack_rows_aug"]["median_us"], 3)
    res["warped_utterances"] = int((warp.last_warp[:, 0] > 0).sum())
    res["rows"], res["F"] = rows.total, Fd
    return res


def whole_step(args, batch):
    import transformer.Models as M
    import transformer.Utils as U
    from st_amd.augment import SpecAugment
    from st_amd.trainer import TrainStep
    from transformer.Optim import ScheduledOptim
    x, tokens, in_len, tgt_len, gt = batch
    torch.manual_seed(0)
    model = M.Transformer(U.AttrDict(CFG))
    U.init_parameters(model)
    model = model.train().cuda()
    xg, tg, gg = x.cuda(), tokens.cuda(), gt.cuda()
    policy = {"none": None, "masks": SpecAugment(80), "masks_warp": SpecAugment(80, time_warp=WARP)}
    steps = {}
    for v in VARIANTS:
        optim = ScheduledOptim(model, CFG["d_model"], U.AttrDict(n_warmup_steps=12000))
        optim.update_learning_rate = (lambda o: lambda global_step: o.lr_tensor.fill_(0.0))(optim)
        steps[v] = TrainStep(model, optim, CFG["vocab_size"], max_grad_norm=5.0, use_graph=True)

    def run(v, n):
        model.encoder.spec_augment = policy[v]            # (read when the step is captured; a replay launches what was captured)
        for _ in range(n):
            last = steps[v](xg, in_len, tg, tgt_len, gg)
        return last

    for v in VARIANTS:                                     # eager warm-ups, capture, first replays
        run(v, 5)
    torch.cuda.synchronize()
    rounds = {v: [] for v in VARIANTS}
    last = {}
    for _ in range(args.repeats):
        for v in VARIANTS:
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            last[v] = run(v, args.steps)
            torch.cuda.synchronize()
            rounds[v].append((time.perf_counter() - t0) / args.steps * 1e3)
    out = {"steps_per_round": args.steps, "graph": True, "mode": "train"}
    for v in VARIANTS:
        r = sorted(rounds[v])
        out[v] = {"ms_per_step_rounds": [round(t, 4) for t in rounds[v]], "ms_per_step_median": round(r[len(r) // 2], 4),
                  "spread_ms": round(r[-1] - r[0], 4), "graphs": len(steps[v]._graphs), "loss": round(float(last[v][0]), 4)}
    for v in VARIANTS[1:]:
        out[v + "_minus_none_us"] = round((out[v]["ms_per_step_median"] - out["none"]["ms_per_step_median"]) * 1e3, 2)
    assert policy["masks_warp"].last_warp is not None and policy["masks"].last_warp is None
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--launches", type=int, default=200)
    ap.add_argument("--steps", type=int, default=30)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--skip-step", action="store_true", help="the per-launch table alone")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "timewarp_bench.json"))
    args = ap.parse_args()

    from st_amd import native as nv
    from st_amd import synthetic
    nv.load(build_if_missing=False)
    batch = synthetic.make_batch(32, 1000, 50, CFG["feature_dim"], CFG["vocab_size"], seed=0, t_min=500, l_min=25)
    in_len = batch[2]
    out = {"shape": "config 2 batch: B 32, %d frames (500..1000 per utterance)" % int(in_len.sum()), "device": torch.cuda.get_device_name(),
           "time_warp": WARP, "launches": args.launches,
           "F320": launches(in_len, args.launches, (80, 3, 30)), "F80": launches(in_len, args.launches, (80, 0, 10))}
    if not args.skip_step:
        out["step"] = whole_step(args, batch)
    line = json.dumps(out)
    print(line)
    if args.out and args.out != os.devnull:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
