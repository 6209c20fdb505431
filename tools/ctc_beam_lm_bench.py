#!/usr/bin/env python3
"""The n-gram model inside the CTC prefix beam search (st_ctc_beam_search_lm) at BASELINE config 5's decode batch - 6+6 layers,
d_model 256, V 4337, 32 utterances of 500..1000 frames, beam 10, pre-beam 10, as tools/ctc_beam_bench.py - with a model estimated
from the batch's targets, as tools/ngram_bench.py.

Every figure comes from a process of its own (``--worker``), the kinds alternating, medians over --rounds processes:

* ``parent`` (``--parent DIR``: a checkout of the parent commit with its library built; left out when not given) and ``nolm``
  (this tree): the LM-less ``st_ctc_beam_search`` on the batch's pre-beam output, device events around windows of --launches
  launches.  The kernel body became a template: (a) is whether that cost the LM-less instantiation anything beyond the
  process-to-process spread the same run shows.
* ``lm`` (this tree): (b) the fused launch, per frame (launch time / T_max: one wave per utterance, the longest is the launch),
  at orders 2 and 4, lambda 0.5, beta 0.5, on three inputs of the same shape: the batch's own head posteriors, synthetic STICKY
  rows (the same K classes for 16 frames, a label on top once in 16: prefixes and their caches live long) and synthetic rows
  whose K classes CHANGE EVERY FRAME with a label on top of every 4th (the worst case: every extension of every frame is a miss,
  a quarter of the frames replace the beam) - each next to the LM-less launch on the same input; (c) end to end, wall clock around synchronised
  calls, the routes alternating: ``Decode.ctc_beam`` and ``Decode.decode_two_pass`` with and without the first-pass weight, and
  the common objective log p_ctc + lambda log p_lm(h . EOS) + beta (|h| + 1) of the best hypothesis of 'fused search' against
  'LM-less search, then rescoring of its n-best'.

Writes profiles/ctc_beam_lm_bench.json (and prints it)."""
import argparse
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CFG = dict(feature_dim=80, max_inputs_length=1000, max_target_length=50, num_enc_layer=6, num_dec_layer=6, n_heads=4,
           d_k=64, d_v=64, d_model=256, d_inner_hid=1024, dropout=0.1, vocab_size=4337)
B, BEAM, K, LAM, BETA, L_CAP = 32, 10, 10, 0.5, 0.5, 255


def median(v):
    return sorted(v)[len(v) // 2]


def synthetic_rows(torch, off, length, pool, period, spike_every, seed):
    """ids i32 / lp f32 [R, K], lpb f32 [R] of the batch's row layout: the blank and K - 1 labels of ``pool`` per row; the label
    set is redrawn every ``period`` frames; every ``spike_every``-th frame a label is on top (0.6, blank 0.2), elsewhere the blank
    (0.8); the other classes share 0.1 in falling shares.  (A label every 4th frame keeps the longest prefix below the 255 the
    kernel holds - past them nothing is extended and nothing looked up.)"""
    g = torch.Generator().manual_seed(seed)
    R = int((off + length).max())
    ids = torch.zeros(R, K, dtype=torch.int32)
    lp = torch.zeros(R, K)
    lpb = torch.zeros(R)
    share = torch.tensor([0.5 ** (j + 1) for j in range(K - 2)])
    share = 0.1 * share / share.sum()
    for b in range(off.numel()):
        o, n = int(off[b]), int(length[b])
        t = 0
        while t < n:
            labels = pool[torch.randperm(pool.numel(), generator=g)[:K - 1]].int()
            for u in range(t, min(t + period, n)):
                spike = u % spike_every == 0
                ids[o + u, 0], ids[o + u, 1] = (labels[0], 0) if spike else (0, labels[0])
                ids[o + u, 2:] = labels[1:]
                p = torch.cat([torch.tensor([0.6, 0.2] if spike else [0.8, 0.1]), share if spike else share * 0.999])
                lp[o + u] = p.log()
                lpb[o + u] = float(p[1] if spike else p[0])
            t += period
    return ids, lp, lpb.log()


def worker(args):
    tree = os.path.abspath(args.tree)
    for p in (tree, os.path.join(tree, "speech-tranformer-pytorch_amd")):
        sys.path.insert(0, p)
    import torch
    import transformer.Models as M
    import transformer.Utils as U
    from st_amd import ctc_decode, synthetic
    from st_amd import native as nv
    from st_amd.arena import arena_of
    from transformer.Decode import Decode
    from transformer.Loss import CTCAttentionLoss

    if not torch.cuda.is_available():
        raise SystemExit("ctc_beam_lm_bench: needs a GPU (a CPU run measures nothing)")
    nv.load(build_if_missing=False)
    torch.manual_seed(0)
    model = M.Transformer(U.AttrDict(CFG))
    U.init_parameters(model)
    model = model.eval().cuda()
    torch.manual_seed(2)
    head = CTCAttentionLoss(CFG["d_model"], CFG["vocab_size"])
    with torch.no_grad():                       # mostly blank frames, peaky label frames (as tools/ctc_beam_bench.py)
        head.ctc_proj.weight.mul_(4.0)
        head.ctc_proj.bias.zero_()
        head.ctc_proj.bias[int(head.blank)] = 2.0
    head = head.cuda()
    x, tokens, in_len, tgt_len, _ = synthetic.make_batch(B, 1000, 50, CFG["feature_dim"], CFG["vocab_size"], seed=0, t_min=500, l_min=25)
    src = (x.cuda(), in_len)
    T_max, V, blank = int(in_len.max()), CFG["vocab_size"], int(head.blank)
    opt = dict(beam_size=BEAM, n_best=1, max_steps=50, ctc_beam_pre_beam=K, ctc_weight=0.3)
    plain = Decode(U.AttrDict(opt), "cuda", model=model, ctc_head=head)
    with torch.no_grad(), arena_of(model).scope():
        enc, in_rows = plain._encode(src)
        logits = ctc_decode.head_logits(head, enc)
        ids = torch.empty(logits.shape[0], K, dtype=torch.int32, device="cuda")
        lp = torch.empty(logits.shape[0], K, dtype=torch.float32, device="cuda")
        nv.beam_pre_beam(logits, V, ids, lp)
        lpb = (logits[:, blank] - (logits.gather(1, ids[:, :1].long()).squeeze(1) - lp[:, 0])).contiguous()
        off, length = in_rows.off.clone(), in_rows.len.clone()
    bufs = (torch.empty(B, BEAM, L_CAP, dtype=torch.int32, device="cuda"), torch.empty(B, BEAM, dtype=torch.int32, device="cuda"),
            torch.empty(B, BEAM, dtype=torch.float32, device="cuda"))
    fused = torch.empty(B, BEAM, dtype=torch.float32, device="cuda")

    def windows(launch):
        def window():
            s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            s.record()
            for _ in range(args.launches):
                launch()
            e.record()
            torch.cuda.synchronize()
            return s.elapsed_time(e) * 1e3 / args.launches  # us per launch
        window()
        return round(median([window() for _ in range(args.windows)]), 1)

    out = {"kind": args.worker, "T_max": T_max}
    out["search_us"] = windows(lambda: nv.ctc_beam_search(ids, lp, lpb, off, length, blank, *bufs))
    out["search_us_per_frame"] = round(out["search_us"] / T_max, 3)
    if args.worker != "lm":
        print("CTC_BEAM_LM_BENCH " + json.dumps(out))
        return

    from st_amd import ngram
    lists = [tokens[b, :int(tgt_len[b])].tolist() for b in range(B)]
    pool = torch.tensor(sorted(set(k for row in lists for k in row)))
    inputs = {"head": (ids, lp, lpb), "sticky16": tuple(t.cuda() for t in synthetic_rows(torch, off.cpu(), length.cpu(), pool, 16, 16, 1)),
              "change_every_frame": tuple(t.cuda() for t in synthetic_rows(torch, off.cpu(), length.cpu(), pool, 1, 4, 2))}
    lms = {order: ngram.NGramLM.estimate(lists, order, V).to("cuda") for order in (2, 4)}
    out["lm_trie_nodes"] = {str(o): lm.trie.nodes for o, lm in lms.items()}
    out["lm_weight"], out["lm_length_bonus"] = LAM, BETA
    launch_us = {}
    for name, (i_, l_, b_) in inputs.items():
        row = {"lm_less": windows(lambda: nv.ctc_beam_search(i_, l_, b_, off, length, blank, *bufs))}
        row["best_labels_mean_lm_less"] = round(float(bufs[1][:, 0].float().mean()), 1)
        for order, lm in lms.items():
            row["order%d" % order] = windows(lambda: nv.ctc_beam_search_lm(i_, l_, b_, off, length, blank, *bufs, lm.trie, 2, 3, LAM, BETA,
                                                                          fused))
            row["order%d_zero_weights" % order] = windows(lambda: nv.ctc_beam_search_lm(i_, l_, b_, off, length, blank, *bufs, lm.trie, 2,
                                                                                       3, 0.0, 0.0, fused))
            row["best_labels_mean_order%d" % order] = round(float(bufs[1][:, 0].float().mean()), 1)
        for k in list(row):
            if not k.startswith("best_"):
                row[k + "_per_frame"] = round(row[k] / T_max, 3)
        launch_us[name] = row
    out["launch_us"] = launch_us

    # ---- end to end -------------------------------------------------------------------------------------------------------------
    lm = lms[4]
    dec = Decode(U.AttrDict(dict(opt, lm_weight=LAM, lm_length_bonus=BETA)), "cuda", model=model, ctc_head=head, lm=lm)
    routes = [("ctc_beam", lambda: dec.ctc_beam(src)), ("ctc_beam_fused", lambda: dec.ctc_beam(src, lm_weight=LAM, lm_length_bonus=BETA)),
              ("decode_two_pass", lambda: dec.decode_two_pass(src)),
              ("decode_two_pass_fused_first_pass", lambda: dec.decode_two_pass(src, first_pass_lm_weight=LAM, first_pass_lm_length_bonus=BETA))]

    def timed(fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        return time.perf_counter() - t0

    for _ in range(2):
        for _, fn in routes:
            fn()
    times = {name: [] for name, _ in routes}
    for _ in range(args.calls):
        for name, fn in routes:
            times[name].append(timed(fn))
    for name, _ in routes:
        ms = median(times[name]) * 1e3
        out[name + "_ms"] = round(ms, 3)
        out[name + "_utt_per_s"] = round(B / (ms * 1e-3), 1)
    # the common objective of both routes' best hypothesis
    hyps, scores, fu = dec.ctc_beam(src, n_best=BEAM, lm_weight=LAM, lm_length_bonus=BETA)
    fused_obj = [float(scores[b][0] + fu[b][0]) for b in range(B)]
    hyps0, scores0 = dec.ctc_beam(src, n_best=BEAM)
    lm0 = dec.lm_score(hyps0).double().cpu()
    resc_obj, same = [], 0
    for b in range(B):
        cand = [(float(scores0[b][j]) + LAM * float(lm0[b, j]) + BETA * (len(h) + 1), h) for j, h in enumerate(hyps0[b])
                if float(scores0[b][j]) > float("-inf")]
        best = max(cand, key=lambda c: c[0])
        resc_obj.append(best[0])
        same += int(best[1] == hyps[b][0])
    diff = [a - b for a, b in zip(fused_obj, resc_obj)]
    out["objective"] = {"fused_mean": round(sum(fused_obj) / B, 3), "rescored_mean": round(sum(resc_obj) / B, 3),
                        "fused_minus_rescored_mean": round(sum(diff) / B, 3), "fused_minus_rescored_min": round(min(diff), 3),
                        "fused_minus_rescored_max": round(max(diff), 3), "fused_better": sum(d > 1e-4 for d in diff),
                        "fused_worse": sum(d < -1e-4 for d in diff), "same_best_hypothesis": same, "utterances": B}
    print("CTC_BEAM_LM_BENCH " + json.dumps(out))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--worker", choices=("parent", "nolm", "lm"), default=None, help="internal: one measuring process")
    ap.add_argument("--tree", default=ROOT)
    ap.add_argument("--parent", default=None, help="a checkout of the parent commit with its library built")
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--lm-rounds", type=int, default=3, help="processes of the lm kind (the long one)")
    ap.add_argument("--launches", type=int, default=20)
    ap.add_argument("--windows", type=int, default=5)
    ap.add_argument("--calls", type=int, default=7)
    ap.add_argument("--timeout", type=int, default=240, help="seconds per worker process")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "ctc_beam_lm_bench.json"))
    args = ap.parse_args()
    if args.worker:
        return worker(args)
    kinds = ([("parent", os.path.abspath(args.parent))] if args.parent else []) + [("nolm", ROOT), ("lm", ROOT)]
    runs = {k: [] for k, _ in kinds}
    for r_ in range(args.rounds):
        for kind, tree in kinds:
            if kind == "lm" and r_ >= args.lm_rounds:
                continue
            r = subprocess.run([sys.executable, os.path.abspath(__file__), "--worker", kind, "--tree", tree, "--calls", str(args.calls),
                                "--launches", str(args.launches), "--windows", str(args.windows)], capture_output=True, text=True,
                               timeout=args.timeout, cwd=tree)
            line = [l for l in r.stdout.splitlines() if l.startswith("CTC_BEAM_LM_BENCH ")]
            if r.returncode != 0 or not line:
                raise SystemExit("ctc_beam_lm_bench: the %s worker failed (exit %d): %s" % (kind, r.returncode, r.stderr[-2000:]))
            runs[kind].append(json.loads(line[0][len("CTC_BEAM_LM_BENCH "):]))
            print("round %d %s: st_ctc_beam_search %.1f us" % (r_, kind, runs[kind][-1]["search_us"]), flush=True)
    out = {"shape": "config 5: B 32, T 500..1000, 6+6 layers, d_model 256, V 4337, beam 10, pre_beam 10; models estimated from the "
                    "batch's targets, lambda %.1f, beta %.1f" % (LAM, BETA), "processes": runs}
    for kind, _ in kinds:
        v = [r["search_us"] for r in runs[kind]]
        out["%s_search_us" % kind] = {"median": median(v), "min": min(v), "max": max(v)}
    if args.parent:
        p, t = out["parent_search_us"], out["nolm_search_us"]
        out["nolm_median_inside_parent_spread"] = bool(p["min"] <= t["median"] <= p["max"])
        out["nolm_median_minus_parent_median_us"] = round(t["median"] - p["median"], 1)
    lm_runs = runs["lm"]
    out["fused_launch_us"] = {name: {k: median([r["launch_us"][name][k] for r in lm_runs]) for k in lm_runs[0]["launch_us"][name]}
                              for name in lm_runs[0]["launch_us"]}
    for key in ("ctc_beam_ms", "ctc_beam_fused_ms", "decode_two_pass_ms", "decode_two_pass_fused_first_pass_ms"):
        out[key] = median([r[key] for r in lm_runs])
    out["objective"] = lm_runs[0]["objective"]
    with open(args.out, "w") as f:
        f.write(json.dumps(out, indent=1) + "\n")
    print(json.dumps({k: v for k, v in out.items() if k != "processes"}))


if __name__ == "__main__":
    main()
