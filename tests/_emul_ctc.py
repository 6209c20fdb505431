"""Torch emulation of the two launches of csrc/st_ctc_loss.hip (native.ctc_loss_fwd / ctc_loss_grad) on CPU tensors - test
infrastructure only, beside tests/_emul.py.  The values come from autograd through the forward restatement of
tests/_ctc_loss_ref.py in float64, rounded to the kernels' float32 outputs; what the composition tests pin with it is the
wiring around the launches (classes, device lengths, coef, who fills g_lp / roww), not the kernels' arithmetic."""
import contextlib

import torch

from st_amd import native as nv
from tests._ctc_loss_ref import is_inf, nll_torch


def ctc_loss_ws_bytes(B, T, L):
    if L > nv.CTC_LOSS_MAX_L:
        raise ValueError("ctc_loss: at most %d labels per utterance are supported (got L = %d)" % (nv.CTC_LOSS_MAX_L, L))
    return 8


def ctc_loss_fwd(lp, classes, in_len, tgt_len, ws, nll):
    assert in_len.dtype == torch.int32 and tgt_len.dtype == torch.int32 and classes.dtype == torch.int64
    out = nll_torch(lp.detach().double(), classes, in_len, tgt_len)
    nll.copy_(torch.where(is_inf(out), torch.full_like(out, float("inf")), out).float())
    return nll


def ctc_loss_grad(lp, classes, in_len, tgt_len, coef, ws, nll, g, roww, softmax_term=True):
    with torch.enable_grad():
        leaf = lp.detach().double().requires_grad_(True)
        out = nll_torch(leaf, classes, in_len, tgt_len)
        fin = ~is_inf(out)
        (d,) = torch.autograd.grad(torch.where(fin, out, torch.zeros_like(out)).sum(), leaf)          # = -occ
    frames = torch.arange(lp.shape[1]).view(1, -1) < in_len.view(-1, 1)
    keep = (frames & fin.view(-1, 1)).unsqueeze(2)
    soft = torch.exp(torch.where(keep, lp.double(), torch.zeros((), dtype=torch.float64))) if softmax_term else 0.0
    g.copy_((coef.double().view(-1, 1, 1) * torch.where(keep, soft + d, torch.zeros((), dtype=torch.float64))).float())
    roww.copy_(torch.where(fin, coef.double(), torch.zeros((), dtype=torch.float64)).float())
    return g


_NAMES = ["ctc_loss_ws_bytes", "ctc_loss_fwd", "ctc_loss_grad"]


@contextlib.contextmanager
def emulated_ctc_loss():
    """Swap the three entry points (use inside ``tests._emul.emulated_kernels()`` for everything else)."""
    saved = {n: getattr(nv, n) for n in _NAMES}
    try:
        for n in _NAMES:
            setattr(nv, n, torch.no_grad()(globals()[n]))
        yield
    finally:
        for n, f in saved.items():
            setattr(nv, n, f)
