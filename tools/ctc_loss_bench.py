#!/usr/bin/env python3
"""The joint CTC + attention training step (BASELINE config 4: 6+6 layers, d_model 256, V 4337, the seed-0 batch of 32
utterances of 500..1000 frames) with the CTC loss from PyTorch-ROCm (``ctc="torch"``: three graphs around an eager side stream)
against the HIP kernels (``ctc="hip"``: one graph) - same box, same process, ALTERNATELY: --repeats rounds of --steps timed
steps each, torch then hip.  Both steps share the model, the head and their optimisers; as in bench.py the update runs at a
learning rate of zero, so every timed step computes from the same weights.  Prints one JSON line and writes it to --out
(default profiles/ctc_loss_bench.json): ms per step of every round, the medians, the spread of the repeats and the difference.
--only hip|torch: that path alone (for a kernel trace: rocprofv3 --kernel-trace --stats -- python tools/ctc_loss_bench.py
--only hip --repeats 1 --steps 1 --out /dev/null)."""
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
    ap.add_argument("--steps", type=int, default=30)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--only", choices=("torch", "hip"), default=None)
    ap.add_argument("--no-graph", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "ctc_loss_bench.json"))
    args = ap.parse_args()

    import transformer.Models as M
    import transformer.Utils as U
    from st_amd import native as nv
    from st_amd import synthetic
    from st_amd.trainer import JointTrainStep
    from transformer.Loss import CTCAttentionLoss
    from transformer.Optim import ScheduledOptim

    nv.load(build_if_missing=False)
    torch.manual_seed(0)
    model = M.Transformer(U.AttrDict(CFG))
    U.init_parameters(model)
    model = model.eval().cuda()
    optim = ScheduledOptim(model, CFG["d_model"], U.AttrDict(n_warmup_steps=12000))
    optim.update_learning_rate = lambda global_step: optim.lr_tensor.fill_(0.0)
    torch.manual_seed(0)
    head = CTCAttentionLoss(CFG["d_model"], CFG["vocab_size"], ctc_weight=0.3).cuda()
    head._st_prepare("cuda")
    head_opt = torch.optim.Adam(head.parameters(), lr=0.0, betas=(0.9, 0.98), eps=1e-9, capturable=True, fused=True)
    x, tokens, in_len, tgt_len, gt = synthetic.make_batch(32, 1000, 50, CFG["feature_dim"], CFG["vocab_size"], seed=0, t_min=500, l_min=25)
    xg, tg, gg = x.cuda(), tokens.cuda(), gt.cuda()

    impls = [args.only] if args.only else ["torch", "hip"]
    steps = {i: JointTrainStep(model, optim, head, max_grad_norm=5.0, head_optimizer=head_opt, use_graph=not args.no_graph, ctc=i)
             for i in impls}
    last = {}
    for i in impls:                                        # eager warm-up, capture, first replays
        for _ in range(4):
            last[i] = steps[i](xg, in_len, tg, tgt_len, gg)
    torch.cuda.synchronize()
    rounds = {i: [] for i in impls}
    for _ in range(args.repeats):
        for i in impls:
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(args.steps):
                last[i] = steps[i](xg, in_len, tg, tgt_len, gg)
            torch.cuda.synchronize()
            rounds[i].append((time.perf_counter() - t0) / args.steps * 1e3)

    out = {"shape": "config 4: B 32, T 500..1000, L 25..50, 6+6 layers, d_model 256, V 4337, ctc_weight 0.3",
           "device": torch.cuda.get_device_name(), "steps_per_round": args.steps, "graph": not args.no_graph}
    for i in impls:
        r = sorted(rounds[i])
        out[i] = {"ms_per_step_rounds": [round(v, 4) for v in rounds[i]], "ms_per_step_median": round(r[len(r) // 2], 4),
                  "spread_ms": round(r[-1] - r[0], 4), "graphs": len(steps[i].graphs),
                  "loss": round(float(last[i][0]), 4), "att": round(float(last[i][1]), 4), "ctc": round(float(last[i][2]), 4)}
    if len(impls) == 2:
        t, h = out["torch"], out["hip"]
        out["hip_minus_torch_ms"] = round(h["ms_per_step_median"] - t["ms_per_step_median"], 4)
        out["hip_faster_by_more_than_the_spread"] = bool(max(rounds["hip"]) < min(rounds["torch"]))
    line = json.dumps(out)
    print(line)
    if args.out and args.out != os.devnull:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
