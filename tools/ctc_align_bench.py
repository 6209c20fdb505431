#!/usr/bin/env python3
"""CTC forced alignment at BASELINE config 4's batch (B 32, 500..1000 frames, 25..50 labels; 6+6 layers, d_model 256, V 4337),
same box, same process:

* ``st_ctc_align`` beside ``st_ctc_loss_fwd`` on the SAME lp / classes / lengths - existing code with the same dependent sweep
  over the frames and heavier arithmetic per frame (exp / log instead of compare / select, two directions on two CUs), no
  backtrace: the fair yardstick.  Device events around windows of --launches launches, the two kernels alternating, median of
  --rounds windows.
* ``Decode.align`` end to end (encoder pass, head projection, gather, alignment, one host read) beside the host alternative:
  the same device work up to lp, then lp copied out and the fp64 reference Viterbi (tests/_ctc_align_ref.py) on the CPU.

Writes one JSON line to profiles/ctc_align_bench.json (and prints it)."""
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


def median(v):
    return sorted(v)[len(v) // 2]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--launches", type=int, default=200)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--calls", type=int, default=7)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "ctc_align_bench.json"))
    args = ap.parse_args()

    import numpy as np
    import transformer.Models as M
    import transformer.Utils as U
    from st_amd import synthetic
    from st_amd import native as nv
    from st_amd.arena import arena_of
    from tests import _ctc_align_ref as ref
    from transformer.Decode import Decode
    from transformer.Loss import CTCAttentionLoss

    if not torch.cuda.is_available():
        raise SystemExit("ctc_align_bench: needs a GPU (a CPU run measures nothing)")
    nv.load(build_if_missing=False)
    torch.manual_seed(0)
    model = M.Transformer(U.AttrDict(CFG))
    U.init_parameters(model)
    model = model.eval().cuda()
    torch.manual_seed(1)
    head = CTCAttentionLoss(CFG["d_model"], CFG["vocab_size"]).cuda()
    B = 32
    x, tokens, in_len, tgt_len, _ = synthetic.make_batch(B, 1000, 50, CFG["feature_dim"], CFG["vocab_size"], seed=0, t_min=500, l_min=25)
    xg = x.cuda()
    hyps = [tokens[b, :int(tgt_len[b])].tolist() for b in range(B)]
    dec = Decode(U.AttrDict(beam_size=1, n_best=1, max_steps=50, use_graph=False), "cuda", model=model, ctc_head=head)

    # ---- the two kernels on the same lp ------------------------------------------------------------------------------------
    out_e2e = dec.align((xg, in_len), hyps)                 # (warm-up of every launch below, and the plan)
    al = dec.alignment
    plan = al.plan
    T, L = plan.T, plan.L
    ws_a, ws_l = plan.align_workspace(), torch.empty(nv.ctc_loss_ws_bytes(B, T, L), dtype=torch.uint8, device="cuda")
    path, spans, score = torch.empty_like(al.path), torch.empty_like(al.spans), torch.empty_like(al.score)
    nll = torch.empty(B, dtype=torch.float32, device="cuda")

    def k_align():
        nv.ctc_align(plan.lp, plan.classes, plan.in_len_dev, plan.tgt_len_dev, ws_a, path, spans, score)

    def k_loss():
        nv.ctc_loss_fwd(plan.lp, plan.classes, plan.in_len_dev, plan.tgt_len_dev, ws_l, nll)

    def window(fn):
        s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        s.record()
        for _ in range(args.launches):
            fn()
        e.record()
        torch.cuda.synchronize()
        return s.elapsed_time(e) * 1e3 / args.launches      # us per launch

    for fn in (k_align, k_loss):
        window(fn)
    t_align, t_loss = [], []
    for _ in range(args.rounds):                            # alternating: the box's clock and neighbours hit both alike
        t_align.append(window(k_align))
        t_loss.append(window(k_loss))
    assert torch.equal(path, al.path) and torch.equal(score, al.score)
    assert bool((score <= -nll + 1e-3 * nll.abs()).all()), "the best path beats the sum over all paths"

    # ---- end to end: Decode.align beside lp copied out + the fp64 reference on the CPU -------------------------------------
    def e2e_device():
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = dec.align((xg, in_len), hyps)
        torch.cuda.synchronize()
        return time.perf_counter() - t0, out

    def e2e_host():
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        with torch.no_grad(), arena_of(model).scope():
            enc, in_rows = model.encoder.forward_rows(xg[:, :int(in_len.max())], in_len)
            from st_amd import ctc_decode
            from st_amd import functional as F_
            logits = ctc_decode.head_logits(head, enc)
            labels = torch.zeros(B, L, dtype=torch.long)
            for b, h in enumerate(hyps):
                labels[b, :len(h)] = torch.tensor(h)
            pl = F_.CtcPlan(labels.cuda(), tgt_len, in_len, in_rows, int(head.blank), logits.shape[1])
            nv.ctc_gather(logits, pl.rowmap, pl.T, pl.cols, torch.empty(logits.shape[0], dtype=torch.float32, device="cuda"), pl.lp)
            lp_h, cls_h = pl.lp.cpu().numpy(), pl.classes.cpu().numpy()
        t1 = time.perf_counter()
        res = ref.align_batch(lp_h, cls_h, in_len.tolist(), tgt_len.tolist())
        return time.perf_counter() - t0, time.perf_counter() - t1, res

    dev = [e2e_device()[0] for _ in range(args.calls)]
    host = [e2e_host() for _ in range(max(1, args.calls // 2))]
    same = int(sum(np.array_equal(host[0][2][0][b], al.path[b].cpu().numpy()) for b in range(B)))
    assert len(out_e2e) == B

    out = {"shape": "config 4: B 32, T 500..1000 (lp [32, %d, %d]), L 25..50, 6+6 layers, d_model 256, V 4337" % (T, L + 1),
           "device": torch.cuda.get_device_name(), "launches_per_window": args.launches,
           "st_ctc_align_us": round(median(t_align), 2), "st_ctc_align_us_rounds": [round(v, 2) for v in t_align],
           "st_ctc_loss_fwd_us": round(median(t_loss), 2), "st_ctc_loss_fwd_us_rounds": [round(v, 2) for v in t_loss],
           "align_over_loss_fwd": round(median(t_align) / median(t_loss), 3),
           "decode_align_ms": round(median(dev) * 1e3, 3), "decode_align_ms_calls": [round(v * 1e3, 3) for v in dev],
           "host_alternative_ms": round(median([h[0] for h in host]) * 1e3, 3),
           "host_alternative_cpu_viterbi_ms": round(median([h[1] for h in host]) * 1e3, 3),
           "host_over_device": round(median([h[0] for h in host]) / median(dev), 2),
           "paths_equal_to_fp64_reference": "%d of %d" % (same, B)}
    line = json.dumps(out)
    with open(args.out, "w") as f:
        f.write(line + "\n")
    print(line)


if __name__ == "__main__":
    main()
