#!/usr/bin/env python3
"""Contextual biasing at BASELINE config 5's decode batch (6+6 layers, d_model 256, V 4337, the seed-0 batch of st_amd.synthetic:
32 utterances of 500..1000 frames, beam 10, ctc_weight 0.3, pre-beam 15, 50 decoder steps - random weights never emit EOS), with
phrase lists of 2-8 tokens: half cut from the batch's targets, half random.

Every figure comes from a process of its own (``--worker``), the kinds alternating: the unbiased joint search on the PARENT tree
(``--parent DIR``: a checkout of the parent commit with its library built; left out when not given), the same search on this
tree, and the search with 100 and with 5,000 phrases (bias_weight 1).  A worker times whole ``decode_batch`` calls (median of
--calls after a warm-up call): ms per call, ms per captured joint step (= call / steps, the figure of
profiles/joint_decode_bench.json) and utterances/s; a bias worker also times the two launches the bias adds to a step
(st_bias_score + st_bias_advance at the search's shape, device events around windows of launches) and the host-side table build.

Writes profiles/bias_bench.json: the per-process figures, each kind's median and min .. max, and whether this tree's unbiased
median lies inside the parent's process-to-process spread."""
import argparse
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CFG = dict(feature_dim=80, max_inputs_length=1000, max_target_length=50, num_enc_layer=6, num_dec_layer=6, n_heads=4,
           d_k=64, d_v=64, d_model=256, d_inner_hid=1024, dropout=0.1, vocab_size=4337)
B, BEAM, W, BW = 32, 10, 0.3, 1.0
PHRASES = {"bias100": 100, "bias5000": 5000}


def median(v):
    return sorted(v)[len(v) // 2]


def phrase_list(count, tokens, tgt_len, V):
    """``count`` phrases of 2-8 tokens: alternately a window of a target of the batch and a random list."""
    import numpy as np
    rng = np.random.default_rng(count)
    out = []
    for i in range(count):
        k = int(rng.integers(2, 9))
        if i % 2 == 0:
            b = int(rng.integers(tokens.shape[0]))
            at = int(rng.integers(0, max(1, int(tgt_len[b]) - k + 1)))
            out.append(tokens[b, at:at + k].tolist())
        else:
            out.append([int(x) for x in rng.integers(4, V, k)])
    return out


def worker(args):
    tree = os.path.abspath(args.tree)
    for p in (tree, os.path.join(tree, "speech-tranformer-pytorch_amd")):
        sys.path.insert(0, p)
    import torch
    import transformer.Models as M
    import transformer.Utils as U
    from st_amd import native as nv
    from st_amd import synthetic
    from transformer.Decode import Decode
    from transformer.Loss import CTCAttentionLoss

    if not torch.cuda.is_available():
        raise SystemExit("bias_bench: needs a GPU (a CPU run measures nothing)")
    nv.load(build_if_missing=False)
    torch.manual_seed(0)
    model = M.Transformer(U.AttrDict(CFG))
    U.init_parameters(model)
    model = model.eval().cuda()
    torch.manual_seed(1)
    head = CTCAttentionLoss(CFG["d_model"], CFG["vocab_size"]).cuda()
    x, tokens, in_len, tgt_len, _ = synthetic.make_batch(B, 1000, 50, CFG["feature_dim"], CFG["vocab_size"], seed=0, t_min=500, l_min=25)
    src = (x.cuda(), in_len)
    opt = dict(beam_size=BEAM, n_best=1, max_steps=args.steps, ctc_weight=W)
    out = {"kind": args.worker, "tree": "parent" if args.worker == "parent" else "this"}
    bias = None
    if args.worker in PHRASES:
        from st_amd.biasing import ContextBias
        t0 = time.perf_counter()
        bias = ContextBias.from_phrases(phrase_list(PHRASES[args.worker], tokens, tgt_len, CFG["vocab_size"]), weight=0.5).to("cuda")
        out.update(phrases=len(bias.phrases), states=bias.tables.S, bias_weight=BW, build_s=round(time.perf_counter() - t0, 3))
        dec = Decode(U.AttrDict(dict(opt, bias_weight=BW)), "cuda", model=model, ctc_head=head, bias=bias)
    else:
        dec = Decode(U.AttrDict(opt), "cuda", model=model, ctc_head=head)
    dec.decode_batch(src)                                   # warm-up at the measured shape (eager first step, capture, allocator)
    times = []
    for _ in range(args.calls):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        hyps, scores = dec.decode_batch(src)
        torch.cuda.synchronize()
        times.append(time.perf_counter() - t0)
    dt, steps = median(times), len(hyps[0][0])
    out.update(ms_per_call=round(dt * 1e3, 3), ms_per_step=round(dt / steps * 1e3, 4), utterances_per_s=round(B / dt, 1), steps=steps,
               calls=args.calls, ms_per_call_all=[round(t * 1e3, 3) for t in times],
               all_scores_finite=bool(all(torch.isfinite(s).all() for s in scores)))
    if bias is not None:                                    # the two launches the bias adds to a step, alone
        out["rewarded_best_hypotheses"] = sum(bias.reward(h[0]) > 0 for h in hyps)
        n, K, t = B * BEAM, dec.ctc_pre_beam, bias.tables
        g = torch.Generator().manual_seed(0)
        state = torch.randint(0, t.S, (n,), generator=g).int().cuda()
        ids = torch.randint(4, CFG["vocab_size"], (n, K), generator=g).int().cuda()
        lp = torch.zeros(n, K, device="cuda")
        order = torch.arange(n, device="cuda")
        toks = torch.randint(4, CFG["vocab_size"], (n,), generator=g).cuda()
        done = torch.zeros(B, dtype=torch.bool, device="cuda")
        keep = state.clone()

        def window(launches=50):
            s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            s.record()
            for _ in range(launches):
                state.copy_(keep)                           # (deep states every time: the advance would drain them to the root)
                nv.bias_score(t, state, ids, done, 3, 1.0, lp=lp)
                nv.bias_advance(t, state, order, toks, done, 3, BEAM)
            e.record()
            torch.cuda.synchronize()
            return s.elapsed_time(e) * 1e3 / launches

        def copies(launches=50):
            s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            s.record()
            for _ in range(launches):
                state.copy_(keep)
            e.record()
            torch.cuda.synchronize()
            return s.elapsed_time(e) * 1e3 / launches
        window(), copies()
        us = [window() - copies() for _ in range(7)]
        out.update(bias_launch_pair_us=round(median(us), 2), bias_launch_pair_us_rounds=[round(v, 2) for v in us])
    print("BIAS_BENCH " + json.dumps(out))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--worker", choices=("parent", "nobias") + tuple(PHRASES), default=None, help="internal: one measuring process")
    ap.add_argument("--tree", default=ROOT)
    ap.add_argument("--parent", default=None, help="a checkout of the parent commit with its library built")
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--calls", type=int, default=7)
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--timeout", type=int, default=150, help="seconds per worker process")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "bias_bench.json"))
    args = ap.parse_args()
    if args.worker:
        return worker(args)
    kinds = ([("parent", os.path.abspath(args.parent))] if args.parent else []) + [("nobias", ROOT)] + [(k, ROOT) for k in PHRASES]
    runs = {k: [] for k, _ in kinds}
    for _ in range(args.rounds):
        for kind, tree in kinds:
            r = subprocess.run([sys.executable, os.path.abspath(__file__), "--worker", kind, "--tree", tree, "--calls", str(args.calls),
                                "--steps", str(args.steps)], capture_output=True, text=True, timeout=args.timeout, cwd=tree)
            line = [l for l in r.stdout.splitlines() if l.startswith("BIAS_BENCH ")]
            if r.returncode != 0 or not line:
                raise SystemExit("bias_bench: the %s worker failed (exit %d): %s" % (kind, r.returncode, r.stderr[-2000:]))
            runs[kind].append(json.loads(line[0][len("BIAS_BENCH "):]))
    out = {"shape": "config 5: B 32, T 500..1000, 6+6 layers, d_model 256, V 4337, beam 10, ctc_weight 0.3, pre_beam 15, %d steps; "
                    "phrases of 2-8 tokens, half from the batch's targets, per-token weight 0.5, bias_weight %.1f" % (args.steps, BW),
           "order": [k for k, _ in kinds] * args.rounds, "processes": runs}
    for kind, _ in kinds:
        for key in ("ms_per_step", "ms_per_call", "utterances_per_s"):
            v = [r[key] for r in runs[kind]]
            out["%s_%s" % (kind, key)] = {"median": median(v), "min": min(v), "max": max(v)}
    for kind in PHRASES:
        out["%s_step_cost_ms" % kind] = round(out["%s_ms_per_step" % kind]["median"] - out["nobias_ms_per_step"]["median"], 4)
        out["%s_launch_pair_us" % kind] = median([r["bias_launch_pair_us"] for r in runs[kind]])
        out["%s_states" % kind] = runs[kind][0]["states"]
        out["%s_build_s" % kind] = median([r["build_s"] for r in runs[kind]])
    if args.parent:
        p, t = out["parent_ms_per_step"], out["nobias_ms_per_step"]
        out["nobias_median_inside_parent_spread"] = bool(p["min"] <= t["median"] <= p["max"])
        out["nobias_median_minus_parent_median_ms"] = round(t["median"] - p["median"], 4)
    with open(args.out, "w") as f:
        f.write(json.dumps(out, indent=1) + "\n")
    print(json.dumps(out))


if __name__ == "__main__":
    main()
