"""Torch emulation of st_ctc_align (native.ctc_align / ctc_align_ws_bytes) on CPU tensors - test infrastructure only, beside
tests/_emul_ctc.py.  The values come from the fp64 restatement tests/_ctc_align_ref.py; what the composition tests pin with it
is the wiring around the launch (classes, device lengths, who fills path / spans / score), not the kernel's arithmetic."""
import contextlib

import torch

from st_amd import native as nv
from tests import _ctc_align_ref as ref


def ctc_align_ws_bytes(B, T, L):
    if L > nv.CTC_LOSS_MAX_L:
        raise ValueError("ctc_align: at most %d labels per utterance are supported (got L = %d)" % (nv.CTC_LOSS_MAX_L, L))
    return 0


def ctc_align(lp, classes, in_len, tgt_len, ws, path, spans, score):
    assert in_len.dtype == torch.int32 and tgt_len.dtype == torch.int32 and classes.dtype == torch.int64
    assert path.dtype == torch.int32 and spans.dtype == torch.int32 and score.dtype == torch.float32
    p, sp, sc, _ = ref.align_batch(lp.detach().numpy(), classes.numpy(), in_len.tolist(), tgt_len.tolist())
    path.copy_(torch.from_numpy(p))
    spans.copy_(torch.from_numpy(sp))
    score.copy_(torch.from_numpy(sc))
    return path, spans, score


_NAMES = ["ctc_align_ws_bytes", "ctc_align"]


@contextlib.contextmanager
def emulated_ctc_align():
    """Swap the two entry points (use inside ``tests._emul.emulated_kernels()`` for everything else)."""
    saved = {n: getattr(nv, n) for n in _NAMES}
    try:
        for n in _NAMES:
            setattr(nv, n, torch.no_grad()(globals()[n]))
        yield
    finally:
        for n, f in saved.items():
            setattr(nv, n, f)
