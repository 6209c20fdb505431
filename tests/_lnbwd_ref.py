"""A plain fp64 reference of the LayerNorm-backward family: st_ln_bwd, st_gemm_lnbwd and the HEAD, FFN and TAIL stages of
st_row_chain_bwd.  Everything in float64; the only rounded values are the operands as they are handed to the kernel and the rounding
points include/st_hip.h states as contract - dy = bf16(dY W (+ aux)) inside st_gemm_lnbwd and the chain stages, dH = bf16(bf16(acc *
mask_scale) * bit).  No output is rounded.  With g = dy * gamma over the N columns of a row:
    dx = rstd * (g - mean(g) - xhat * mean(g * xhat)),  dgamma = sum_rows dy * xhat,  dbeta = sum_rows dy,  dbias = sum_rows dx
dy is masked and rescaled first where the forward dropped the LayerNorm output (``keep``: the bool mask of tests/_emul.keep_rc);
``mask``: dx is zero where mask <= 0 and scaled by mask_scale elsewhere."""
import torch

BF16, F64 = torch.bfloat16, torch.float64


def keep_of(drop, M, N):
    """(bool [M, N] or None, scale): the kept elements of an [M, N] row matrix under the emulation's Drop."""
    from tests import _emul as em
    if drop is None or drop.thresh <= 0:
        return None, 1.0
    return em.keep_rc(drop, torch.arange(M), torch.arange(N), N), float(drop.scale)


def ln_bwd(dy, xhat, rstd, gamma, keep=None, drop_scale=1.0, mask=None, mask_scale=1.0):
    """-> dict(dx, dgamma, dbeta, dbias), fp64, nothing rounded."""
    d, xh = dy.to(F64), xhat.to(F64)[:dy.shape[0]]
    if keep is not None:
        d = d * keep * drop_scale
    g = d * gamma.to(F64)
    n = g.shape[1]
    v = rstd.to(F64)[:dy.shape[0]].unsqueeze(1) * (g - g.sum(1, keepdim=True) / n - xh * ((g * xh).sum(1, keepdim=True) / n))
    if mask is not None:
        v = torch.where(mask.to(F64) > 0, v * mask_scale, torch.zeros_like(v))
    return dict(dx=v, dgamma=(d * xh).sum(0), dbeta=d.sum(0), dbias=v.sum(0))


def dgrad(dY, W, aux=None):
    """dY W (+ aux), unrounded; W [Kc, N] as the nn.Linear weight is stored."""
    acc = dY.to(F64) @ W.to(F64)
    return acc if aux is None else acc + aux.to(F64)


def gemm_lnbwd(dY, W, aux, xhat, rstd, gamma, keep=None, drop_scale=1.0):
    """Dgrad followed by LayerNorm backward; dy passes the contract's one rounding point.  -> ln_bwd's dict + dy (the bf16 values)."""
    dy = dgrad(dY, W, aux).to(BF16)
    out = ln_bwd(dy, xhat, rstd, gamma, keep, drop_scale)
    out["dy"] = dy
    return out


def masked_dgrad(ds, W2, bits, mask_scale=1.0):
    """dH = (ds W2) * mask_scale where the hidden value was kept (bits: bool [M, d_ff]), zero elsewhere; W2 [256, d_ff].  Unrounded
    (bf16(bf16(x) * bit) = bf16(x * bit): the contract's two roundings are one)."""
    return ds.to(F64) @ W2.to(F64) * mask_scale * bits.to(F64)


def colsum(x):
    """Column sum of a tensor AS STORED (the kernel's own bf16 dx): what st_gemm_lnbwd and the chains add up for dbias."""
    return x.to(F64).sum(0)


def delta_of(dctx, O, Ores, heads=4):
    """delta [heads, M] flattened: the sum over each head's columns of dctx AS STORED times O + Ores as handed."""
    o = O.to(F64)[:dctx.shape[0]] + (0.0 if Ores is None else Ores.to(F64)[:dctx.shape[0]])
    M = dctx.shape[0]
    return (dctx.to(F64) * o).reshape(M, heads, -1).sum(-1).t().reshape(-1)
