#!/usr/bin/env python3
"""What a validation batch costs (BASELINE config 2: 6+6 layers, d_model 256, V 4337, the seed-0 batch of 32 utterances of
500..1000 frames - the bench.py batch - in eval mode), and that the training step did not move.  One process times, ALTERNATELY
over --repeats rounds of --batches timed calls each, the variants asked for with --only (default: all):
  eval_eager  EvalStep(use_graph=False): forward_packed + st_ce_eval_fwd + st_eval_note, launched from the host
  eval_graph  EvalStep(use_graph=True, bucket=(1000, 50)): the same as one replayed bucket graph over the PADDED layouts
              (32 x 1000 frame rows where the batch has 24,060)
  eval_graph_packed  ... with bucket_rows=(24576, 1440), the packed capacities bench.py gives TrainStep for this loader
  torch       the only route without EvalStep: model(...) scatters the logits to [B, L, V], then nn.functional.cross_entropy
              (sum) and an arg-max in torch, accumulated in device tensors (no host read per batch either)
  train       TrainStep(use_graph=True) ms per step, as tools/accum_bench.py times its plain variant
Prints one JSON line and writes it to --out.

`torch` and `train` need nothing this tool's commit added (st_amd.evaluate is imported only for the eval_* variants), so the
same file times the PARENT commit from a checkout of it: run this commit and the parent alternately, one fresh process each,
several times, in one session on one box, with --label this / parent and --out some.jsonl; then --merge the lines into
--out: per label and variant the medians by process, their process-to-process spread, and the differences between the labels."""
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
VARIANTS = ("eval_eager", "eval_graph", "eval_graph_packed", "torch", "train")


def _median(xs):
    xs = sorted(xs)
    return xs[len(xs) // 2]


def merge(paths, out_path):
    runs = []
    for path in paths:
        with open(path) as f:
            runs += [json.loads(line) for line in f if line.strip().startswith("{")]
    labels = sorted({r["label"] for r in runs})
    out = {"shape": runs[0]["shape"], "device": runs[0]["device"], "processes": len(runs), "labels": {}}
    for lab in labels:
        mine = [r for r in runs if r["label"] == lab]
        doc = {}
        for v in VARIANTS:
            meds = [r[v]["ms_median"] for r in mine if v in r]
            if meds:
                doc[v] = {"ms_by_process": meds, "median": round(_median(meds), 4), "process_spread_ms": round(max(meds) - min(meds), 4)}
                res = [r[v]["result"] for r in mine if v in r and "result" in r[v]]
                if res:
                    doc[v]["result"] = res[-1]
        out["labels"][lab] = doc
    if len(labels) == 2:
        a, b = labels
        for v in VARIANTS:
            if v in out["labels"][a] and v in out["labels"][b]:
                out["%s_%s_minus_%s_us" % (v, a, b)] = round((out["labels"][a][v]["median"] - out["labels"][b][v]["median"]) * 1e3, 2)
    line = json.dumps(out)
    print(line)
    with open(out_path, "w") as f:
        f.write(line + "\n")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batches", type=int, default=200)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--only", nargs="+", choices=VARIANTS, default=None)
    ap.add_argument("--label", default="this")
    ap.add_argument("--merge", nargs="+", default=None, help="JSON-line files of earlier processes to combine into --out")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "eval_bench.json"))
    args = ap.parse_args()
    if args.merge:
        return merge(args.merge, args.out)

    import torch
    import transformer.Models as M
    import transformer.Utils as U
    from st_amd import native as nv
    from st_amd import synthetic
    from st_amd.trainer import TrainStep
    from transformer.Optim import ScheduledOptim

    nv.load(build_if_missing=False)
    torch.manual_seed(0)
    model = M.Transformer(U.AttrDict(CFG))
    U.init_parameters(model)
    model = model.eval().cuda()
    V = CFG["vocab_size"]
    x, tokens, in_len, tgt_len, gt = synthetic.make_batch(32, 1000, 50, CFG["feature_dim"], V, seed=0, t_min=500, l_min=25)
    xg, tg, gg = x.cuda(), tokens.cuda(), gt.cuda()
    variants = list(args.only) if args.only else list(VARIANTS)
    calls, results = {}, {}

    for v in variants:
        if v.startswith("eval_"):
            from st_amd.evaluate import EvalStep
            kw = dict(use_graph=False) if v == "eval_eager" else dict(use_graph=True, bucket=(1000, 50))
            if v == "eval_graph_packed":
                kw["bucket_rows"] = (256 * 96, 1440)
            ev = EvalStep(model, V, **kw)
            calls[v] = (lambda e: lambda: e(xg, in_len, tg, tgt_len, gg))(ev)
            results[v] = (lambda e: lambda: {k: (round(val, 6) if isinstance(val, float) else val) for k, val in e.result().items()})(ev)
        elif v == "torch":
            acc = torch.zeros(3, dtype=torch.float64, device="cuda")

            def torch_route(acc=acc):
                with torch.no_grad():
                    logits, _ = model(xg, in_len, tg, tgt_len)
                    flat, t = logits.view(-1, V), gg.view(-1)
                    keep = t != 0
                    acc[0] += torch.nn.functional.cross_entropy(flat, t, ignore_index=0, reduction="sum")
                    acc[1] += keep.sum()
                    acc[2] += ((flat.argmax(-1) == t) & keep).sum()
            calls[v] = torch_route
            results[v] = (lambda a: lambda: dict(nll=round(float(a[0] / a[1]), 6), accuracy=round(float(a[2] / a[1]), 6),
                                                 tokens=int(a[1])))(acc)
        else:
            optim = ScheduledOptim(model, CFG["d_model"], U.AttrDict(n_warmup_steps=12000))
            optim.update_learning_rate = (lambda o: lambda global_step: o.lr_tensor.fill_(0.0))(optim)      # (as bench.py: the weights stay put)
            step = TrainStep(model, optim, V, max_grad_norm=5.0, use_graph=True)
            calls[v] = (lambda s: lambda: s(xg, in_len, tg, tgt_len, gg))(step)      # (eval mode: no dropout, as tools/accum_bench.py)
    for v in variants:                                     # eager warm-ups, captures, first replays
        for _ in range(4):
            calls[v]()
    torch.cuda.synchronize()
    rounds = {v: [] for v in variants}
    for _ in range(args.repeats):
        for v in variants:
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(args.batches):
                calls[v]()
            torch.cuda.synchronize()
            rounds[v].append((time.perf_counter() - t0) / args.batches * 1e3)

    out = {"label": args.label, "shape": "config 2: B 32, T 500..1000, L 25..50, 6+6 layers, d_model 256, V 4337",
           "device": torch.cuda.get_device_name(), "batches_per_round": args.batches}
    for v in variants:
        r = sorted(rounds[v])
        out[v] = {"ms_rounds": [round(t, 4) for t in rounds[v]], "ms_median": round(r[len(r) // 2], 4), "spread_ms": round(r[-1] - r[0], 4)}
        if v in results:
            out[v]["result"] = results[v]()
    line = json.dumps(out)
    print(line)
    if args.out and args.out != os.devnull:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "a" if os.path.basename(args.out).endswith(".jsonl") else "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
