"""Test-only torch emulations of native.ce_eval_fwd / eval_note (st_ce_eval_fwd / st_eval_note, csrc/st_eval.hip), in the
conventions of tests/_emul_ce.py: the closed form of the header evaluated in the logits' own precision (fp64 logits -> an
fp64 statement about the formula; the -m gpu tests hold the kernels to the same form on fp32 logits taken to fp64)."""
import contextlib

import torch

from st_amd import native as nv
from tests._emul_ce import smoothed_sum


def ce_eval_fwd(logits, target, ignore_index, confidence, smooth, zero_col, rows, V=None, index=None):
    """rows [R, 4] = {criterion numerator, lse - x[t], arg-max == t (lowest column among equal maxima), state}; state 0 =
    ignored, 1 = counted, 2 = a target outside [0, V) that is not ignore_index (contributes nothing else)."""
    V = logits.shape[1] if V is None else V
    x = logits[:, :V] if logits.dtype == torch.float64 else logits[:, :V].float()
    t = (target if index is None else target.reshape(-1)[index]).reshape(-1)
    bad = (t != ignore_index) & ((t < 0) | (t >= V))
    ok = (t != ignore_index) & ~bad
    tc = t.clamp(0, V - 1).view(-1, 1)
    hasz = (t != zero_col).to(x.dtype) if zero_col >= 0 else torch.zeros_like(t, dtype=x.dtype)
    l = torch.logsumexp(x, -1)
    xt = x.gather(1, tc).squeeze(1)
    Q = confidence + smooth * (V - 1 - hasz)
    sub, add = smoothed_sum(x, smooth, zero_col, hasz)
    loss = Q * l - (confidence - smooth) * xt - sub
    if zero_col >= 0:
        loss = loss + add
    # the FIRST column holding the row's maximum (torch.argmax documents no tie rule)
    cols = torch.arange(V, device=x.device).expand_as(x)
    first = torch.where(x == x.max(-1, keepdim=True).values, cols, torch.full_like(cols, V)).min(-1).values
    okf = ok.to(x.dtype)
    out = torch.stack([torch.where(ok, loss, torch.zeros_like(loss)), torch.where(ok, l - xt, torch.zeros_like(l)),
                       (first == t).to(x.dtype) * okf, okf + 2 * bad.to(x.dtype)], 1)
    rows.copy_(out.to(rows.dtype))
    return rows


def eval_note(rows, acc, last, denom=None):
    """acc (f64 [8]) += {loss, denominator, NLL, tokens, hits, 1, stray labels, 0}; last = this batch's (loss, nll, accuracy,
    tokens) - 0 / 0 = nan."""
    r = rows.double()
    tok, bad = (r[:, 3] == 1).double().sum(), (r[:, 3] == 2).double().sum()
    den = tok if denom is None else denom.reshape(-1)[0].double()
    s = r[:, :3].sum(0)
    acc += torch.stack([s[0], den, s[1], tok, s[2], torch.ones_like(tok), bad, torch.zeros_like(tok)]).to(acc.dtype)
    last.copy_(torch.stack([s[0] / den, s[1] / tok, s[2] / tok, tok]).to(last.dtype))
    return last


@contextlib.contextmanager
def emulated_eval():
    saved = nv.ce_eval_fwd, nv.eval_note
    try:
        nv.ce_eval_fwd, nv.eval_note = torch.no_grad()(ce_eval_fwd), torch.no_grad()(eval_note)
        yield
    finally:
        nv.ce_eval_fwd, nv.eval_note = saved
