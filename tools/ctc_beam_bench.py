#!/usr/bin/env python3
"""CTC prefix beam search and two-pass decoding at BASELINE config 5's decode batch (6+6 layers, d_model 256, V 4337, 32
utterances of 500..1000 frames, beam 10, pre-beam 10), same box, same process:

* ``st_ctc_beam_search`` alone on the batch's pre-beam output: device events around windows of --launches launches, median of
  --rounds windows; per frame = launch time / T_max (one wave per utterance: the longest utterance is the launch).
* end to end, wall clock around a synchronised call, the routes alternating inside every round so the box's clock and its
  neighbours hit all alike: ``Decode.ctc_beam``, ``Decode.decode_two_pass``, ``Decode.decode_batch`` attention-only and joint
  (ctc_weight 0.3), ``Decode.ctc_greedy``; utterances/s = 32 / median.

Writes one JSON line to profiles/ctc_beam_bench.json (and prints it)."""
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
    ap.add_argument("--launches", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--calls", type=int, default=7)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "ctc_beam_bench.json"))
    args = ap.parse_args()

    import transformer.Models as M
    import transformer.Utils as U
    from st_amd import ctc_decode, synthetic
    from st_amd import native as nv
    from st_amd.arena import arena_of
    from transformer.Decode import Decode
    from transformer.Loss import CTCAttentionLoss

    if not torch.cuda.is_available():
        raise SystemExit("ctc_beam_bench: needs a GPU (a CPU run measures nothing)")
    nv.load(build_if_missing=False)
    torch.manual_seed(0)
    model = M.Transformer(U.AttrDict(CFG))
    U.init_parameters(model)
    model = model.eval().cuda()
    torch.manual_seed(2)
    head = CTCAttentionLoss(CFG["d_model"], CFG["vocab_size"])
    with torch.no_grad():                       # mostly blank frames, peaky label frames (as tests/test_joint_decode_gpu.py)
        head.ctc_proj.weight.mul_(4.0)
        head.ctc_proj.bias.zero_()
        head.ctc_proj.bias[int(head.blank)] = 2.0
    head = head.cuda()
    B, beam, K = 32, 10, 10
    x, _, in_len, _, _ = synthetic.make_batch(B, 1000, 50, CFG["feature_dim"], CFG["vocab_size"], seed=0, t_min=500, l_min=25)
    src = (x.cuda(), in_len)
    T_max, V = int(in_len.max()), CFG["vocab_size"]

    def decoder(**opt):
        return Decode(U.AttrDict(dict(dict(beam_size=beam, n_best=1, max_steps=50, ctc_beam_pre_beam=K), **opt)), "cuda", model=model,
                      ctc_head=head)

    two = decoder(ctc_weight=0.3)
    att_only = decoder()
    joint = decoder(ctc_weight=0.3, ctc_pre_beam=15)

    # ---- the search launch alone ------------------------------------------------------------------------------------------------
    with torch.no_grad(), arena_of(model).scope():
        enc, in_rows = two._encode(src)
        logits = ctc_decode.head_logits(head, enc)
        ids = torch.empty(logits.shape[0], K, dtype=torch.int32, device="cuda")
        lp = torch.empty(logits.shape[0], K, dtype=torch.float32, device="cuda")
        nv.beam_pre_beam(logits, V, ids, lp)
        lpb = (logits[:, int(head.blank)] - (logits.gather(1, ids[:, :1].long()).squeeze(1) - lp[:, 0])).contiguous()
        off, length = in_rows.off.clone(), in_rows.len.clone()
    L_cap = 255
    tokens = torch.empty(B, beam, L_cap, dtype=torch.int32, device="cuda")
    lens = torch.empty(B, beam, dtype=torch.int32, device="cuda")
    score = torch.empty(B, beam, dtype=torch.float32, device="cuda")

    def window():
        s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        s.record()
        for _ in range(args.launches):
            nv.ctc_beam_search(ids, lp, lpb, off, length, int(head.blank), tokens, lens, score)
        e.record()
        torch.cuda.synchronize()
        return s.elapsed_time(e) * 1e3 / args.launches      # us per launch

    window()
    t_search = [window() for _ in range(args.rounds)]
    best_len = lens[:, 0].float()

    # ---- end to end -------------------------------------------------------------------------------------------------------------
    routes = [("ctc_beam", lambda: two.ctc_beam(src)), ("decode_two_pass", lambda: two.decode_two_pass(src)),
              ("decode_batch_attention", lambda: att_only.decode_batch(src)), ("decode_batch_joint", lambda: joint.decode_batch(src)),
              ("ctc_greedy", lambda: two.ctc_greedy(src))]

    def timed(fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        return time.perf_counter() - t0

    for _ in range(2):                                      # warm-up: kernel modules, allocator, graph capture of the searches
        for _, fn in routes:
            fn()
    times = {name: [] for name, _ in routes}
    for _ in range(args.calls):
        for name, fn in routes:
            times[name].append(timed(fn))

    out = {"shape": "config 5: B 32, T 500..1000 (T_max %d), 6+6 layers, d_model 256, V 4337, beam 10, pre_beam 10, max_steps 50" % T_max,
           "device": torch.cuda.get_device_name(), "launches_per_window": args.launches,
           "st_ctc_beam_search_us": round(median(t_search), 1), "st_ctc_beam_search_us_rounds": [round(v, 1) for v in t_search],
           "st_ctc_beam_search_us_per_frame": round(median(t_search) / T_max, 3),
           "best_hypothesis_labels_mean": round(float(best_len.mean()), 1), "best_hypothesis_labels_max": int(best_len.max())}
    for name, _ in routes:
        ms = median(times[name]) * 1e3
        out[name + "_ms"] = round(ms, 3)
        out[name + "_ms_calls"] = [round(v * 1e3, 3) for v in times[name]]
        out[name + "_utt_per_s"] = round(B / (ms * 1e-3), 1)
    line = json.dumps(out)
    with open(args.out, "w") as f:
        f.write(line + "\n")
    print(line)


if __name__ == "__main__":
    main()
