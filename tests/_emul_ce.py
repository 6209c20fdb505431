"""Test-only torch emulations of native.ce_smooth_fwd / ce_smooth_bwd (st_ce_smooth_fwd / _bwd, csrc/st_loss.hip): the
closed form of the header, evaluated in the logits' own precision (fp64 logits -> an fp64 statement about the formula; the
-m gpu tests hold the kernels to the same form).  Used inside ``tests._emul.emulated_kernels()`` for everything else."""
import contextlib

import torch

from st_amd import native as nv


def _rows(logits, target, V, index, zero_col):
    V = logits.shape[1] if V is None else V
    x = logits[:, :V] if logits.dtype == torch.float64 else logits[:, :V].float()
    t = (target if index is None else target.reshape(-1)[index]).reshape(-1)
    tc = t.clamp(0, V - 1).view(-1, 1)
    hasz = ((t != zero_col).to(x.dtype) if zero_col >= 0 else torch.zeros_like(t, dtype=x.dtype))
    return V, x, t, tc, hasz


def smoothed_sum(x, smooth, zero_col, hasz):
    """-> (smooth x sum_v x[v], smooth x x[zero_col] hasz): what the row loss subtracts and adds back, as the kernels form the two when
    a logit is -inf (a column of probability zero): a masked zero column carries no target mass and stays out of both, and smooth == 0
    gives no column any (0 x -inf is 0, not NaN)."""
    zero = torch.zeros_like(x[:, 0])
    if smooth == 0:
        return zero, zero
    if zero_col < 0:
        return smooth * x.sum(-1), zero
    z = x[:, zero_col]
    skip = (hasz != 0) & torch.isinf(z) & (z < 0)
    if not bool(skip.any()):
        return smooth * x.sum(-1), smooth * z * hasz
    zs = torch.where(skip, zero, z)
    return smooth * torch.cat([x[:, :zero_col], zs.view(-1, 1), x[:, zero_col + 1:]], 1).sum(-1), smooth * zs * hasz


def ce_smooth_fwd(logits, target, ignore_index, confidence, smooth, zero_col, lse, sums, V=None, index=None, denom=None):
    V, x, t, tc, hasz = _rows(logits, target, V, index, zero_col)
    valid = (t != ignore_index).to(x.dtype)
    l = torch.logsumexp(x, -1)
    lse.copy_(l)
    xt = x.gather(1, tc).squeeze(1)
    Q = confidence + smooth * (V - 1 - hasz)
    sub, add = smoothed_sum(x, smooth, zero_col, hasz)
    row = Q * l - (confidence - smooth) * xt - sub
    if zero_col >= 0:
        row = row + add
    sums[0] = (row * valid).sum()
    sums[1] = valid.sum()
    sums[2] = sums[0] / (sums[1] if denom is None else denom.reshape(-1)[0].to(sums.dtype))
    sums[3] = ((l - xt) * valid).sum() / sums[1]


def ce_smooth_bwd(logits, target, ignore_index, confidence, smooth, zero_col, lse, sums, grad_out, dlogits, V=None, index=None,
                  denom=None):
    V, x, t, tc, hasz = _rows(logits, target, V, index, zero_col)
    valid = (t != ignore_index).to(x.dtype).view(-1, 1)
    q = torch.full_like(x, smooth)
    if zero_col >= 0:
        q[:, zero_col] = 0
    q.scatter_(1, tc, confidence)
    Q = (confidence + smooth * (V - 1 - hasz)).view(-1, 1)
    D = sums[1] if denom is None else denom.reshape(-1)[0].to(sums.dtype)
    g = (Q * torch.exp(x - lse.to(x.dtype).view(-1, 1)) - q) * valid * (grad_out.to(x.dtype).reshape(-1)[0] / D.to(x.dtype))
    if float(sums[1]) == 0:
        g = torch.zeros_like(g)
    dlogits.zero_()
    dlogits[:, :V] = g.to(dlogits.dtype)


@contextlib.contextmanager
def emulated_ce_smooth():
    saved = nv.ce_smooth_fwd, nv.ce_smooth_bwd
    try:
        nv.ce_smooth_fwd, nv.ce_smooth_bwd = torch.no_grad()(ce_smooth_fwd), torch.no_grad()(ce_smooth_bwd)
        yield
    finally:
        nv.ce_smooth_fwd, nv.ce_smooth_bwd = saved
