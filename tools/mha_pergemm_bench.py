"""One encoder-sized self-attention sublayer on the per-GEMM path (the stand-alone MultiHeadAttention module at d_model 256,
4 heads of 64: st_amd.functional.MhaFn), forward + backward, timed with device events.  st_attn_bwd serves pre-scaled keys
with the backward streams and plain keys with the general kernels; at these row counts the weight-stationary GEMM
(native.ws_ok) would serve the q | k | v projection, but it leaves the keys plain, so MhaFn takes st_gemm_kscale instead when a
backward follows.  What either choice costs:

    python tools/mha_pergemm_bench.py                # as shipped: st_gemm_kscale projection, pre-scaled keys, the streams
    python tools/mha_pergemm_bench.py --plain-keys   # st_gemm_ws projection, plain keys, the general backward kernels
    ST_HIP_LIB=<another build's libst_hip.so> python tools/mha_pergemm_bench.py --plain-keys    # the same step on that library

One process per variant; alternate the processes on one box (LABNOTES.md).  Prints one JSON line: ms per forward + backward
(median and range over the windows) and the attention backward call alone.
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "speech-tranformer-pytorch_amd")):
    if p not in sys.path:
        sys.path.insert(0, p)

import torch          # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--plain-keys", action="store_true", help="no pre-scaled keys: the q | k | v projection through st_gemm_ws")
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--frames", type=int, default=752)          # 32 x 752 = 24,064 rows: config 2's encoder
    ap.add_argument("--windows", type=int, default=7)
    ap.add_argument("--iters", type=int, default=1000)          # ~0.3 s per window
    a = ap.parse_args()
    assert torch.cuda.is_available(), "needs a GPU"
    from st_amd import native as nv
    import transformer.Attention as A
    if a.plain_keys:
        from st_amd import functional as F_
        F_.MhaFn.PRESCALE_KEYS = False
    calls = {"n": 0, "kpre": None}
    bwd = nv.attn_bwd

    def spy(*args, **kw):
        calls["n"] += 1
        calls["kpre"] = bool(kw.get("k_prescaled", False))
        return bwd(*args, **kw)

    nv.attn_bwd = spy
    torch.manual_seed(0)
    mha = A.MultiHeadAttention(4, 256, 64, 64, dropout=0.0).cuda().eval()
    x = (torch.randn(a.batch, a.frames, 256, device="cuda") * 1.0).requires_grad_(True)
    dy = torch.randn(a.batch, a.frames, 256, device="cuda")

    def step():
        out, _ = mha(x, x, x)
        out.backward(dy)
        x.grad = None

    for _ in range(5):
        step()
    torch.cuda.synchronize()
    ms = []
    for _ in range(a.windows):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(a.iters):
            step()
        e1.record()
        torch.cuda.synchronize()
        ms.append(e0.elapsed_time(e1) / a.iters)
    ms.sort()
    # the attention backward call alone, on operands of the same shape and key form
    H, dk, d, M = 4, 64, 256, a.batch * a.frames
    kpre = bool(calls["kpre"])
    off = torch.arange(a.batch, dtype=torch.int32, device="cuda") * a.frames
    ln = torch.full((a.batch,), a.frames, dtype=torch.int32, device="cuda")
    qkv = (torch.randn(M, 3 * d, device="cuda") * 0.7).to(torch.bfloat16)
    Q, K, V = qkv[:, :d], qkv[:, d:2 * d], qkv[:, 2 * d:]
    if kpre:
        K = (K.float() * (nv.K_LOG2_SCALE / 8)).to(torch.bfloat16)
    dO = (torch.randn(M, d, device="cuda") * 0.5).to(torch.bfloat16)
    O, lse = torch.empty(M, d, dtype=torch.bfloat16, device="cuda"), torch.empty(H * M, dtype=torch.float32, device="cuda")
    nv.attn_fwd(Q, K, V, O, lse, off, ln, off, ln, H, a.frames, False, 0.125, max_k=a.frames, k_prescaled=kpre)
    delta = (dO.float() * O.float()).view(M, H, dk).sum(-1).t().contiguous().view(-1)
    outs = [torch.empty(M, d, dtype=torch.bfloat16, device="cuda") for _ in range(3)]
    call = lambda: bwd(Q, K, V, None, dO, lse, delta, *outs, off, ln, off, ln, H, a.frames, a.frames, False, 0.125, k_prescaled=kpre)
    for _ in range(5):
        call()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(100):
        call()
    e1.record()
    torch.cuda.synchronize()
    print(json.dumps(dict(variant="plain-keys" if a.plain_keys else "default", lib=os.environ.get("ST_HIP_LIB", "tree"), rows=M, keys_prescaled=kpre,
                          ms_fwd_bwd_median=round(ms[len(ms) // 2], 4), ms_fwd_bwd_min=round(ms[0], 4), ms_fwd_bwd_max=round(ms[-1], 4),
                          us_attn_bwd_call=round(e0.elapsed_time(e1) * 10, 1))))


if __name__ == "__main__":
    main()
