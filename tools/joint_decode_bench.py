#!/usr/bin/env python3
"""Joint CTC / attention decode against attention-only decode, same box, same process: the decode block of bench.py
(BASELINE config 5 shape: 6+6 layers, d_model 256, V 4337, the seed-0 batch of 32 utterances of 500..1000 frames, beam 10,
50 decoder steps - random weights never emit EOS) timed as whole decode_batch calls (median of --calls after one warm-up
call), once without the CTC head and once with a random head at ctc_weight 0.3 (pre-beam ceil(1.5 beam) = 15).  Prints one
JSON line: utterances/s and ms per step of both, and their ratio.  --joint-only: only the joint calls (for a kernel trace:
rocprofv3 --kernel-trace --stats -- python tools/joint_decode_bench.py --joint-only --calls 1)."""
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=5)
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--weight", type=float, default=0.3)
    ap.add_argument("--joint-only", action="store_true")
    args = ap.parse_args()

    import transformer.Models as M
    import transformer.Utils as U
    from st_amd import native as nv
    from st_amd import synthetic
    from transformer.Decode import Decode
    from transformer.Loss import CTCAttentionLoss

    nv.load(build_if_missing=False)
    torch.manual_seed(0)
    model = M.Transformer(U.AttrDict(CFG))
    U.init_parameters(model)
    model = model.eval().cuda()
    torch.manual_seed(1)
    head = CTCAttentionLoss(CFG["d_model"], CFG["vocab_size"]).cuda()
    B = 32
    x, _, in_len, _, _ = synthetic.make_batch(B, 1000, 50, CFG["feature_dim"], CFG["vocab_size"], seed=0, t_min=500, l_min=25)
    xg = x.cuda()

    def timed(dec):
        dec.decode_batch((xg, in_len))                    # warm-up at the measured shape (eager first step, capture, allocator)
        times = []
        for _ in range(args.calls):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            hyps, scores = dec.decode_batch((xg, in_len))
            torch.cuda.synchronize()
            times.append(time.perf_counter() - t0)
        dt = sorted(times)[len(times) // 2]
        steps = len(hyps[0][0])
        return {"utterances_per_s": round(B / dt, 1), "ms_per_call": round(dt * 1e3, 3), "ms_per_step": round(dt / steps * 1e3, 4),
                "steps": steps, "calls": args.calls, "all_scores_finite": bool(all(torch.isfinite(s).all() for s in scores))}

    out = {"shape": "B 32, T 500..1000, 6+6 layers, d_model 256, V 4337, beam 10", "device": torch.cuda.get_device_name()}
    if not args.joint_only:
        out["attention_only"] = timed(Decode(U.AttrDict(beam_size=10, n_best=1, max_steps=args.steps), "cuda", model=model))
    out["joint"] = timed(Decode(U.AttrDict(beam_size=10, n_best=1, max_steps=args.steps, ctc_weight=args.weight), "cuda", model=model,
                                ctc_head=head))
    out["joint"]["ctc_weight"] = args.weight
    if "attention_only" in out:
        out["joint_over_attention_only_utterances_per_s"] = round(out["joint"]["utterances_per_s"]
                                                                  / out["attention_only"]["utterances_per_s"], 3)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
