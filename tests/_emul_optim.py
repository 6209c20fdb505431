"""Test-only torch emulations of the optimizer wrappers of st_amd.native (grad_norm_guard, adam_clip_avg,
swap_), like tests/_emul_ce.py: the host logic of ScheduledOptim / TrainStep runs on CPU tensors against them.  The
arithmetic follows include/st_hip.h; it is NOT the kernels' rounding (the -m gpu tests pin that on hardware)."""
import contextlib

import numpy as np
import torch

from st_amd import native as nv
from tests import _emul


def grad_norm_guard(g, scratch, out, step, guard, grad_scale=1.0):
    if step is None or guard is None:
        raise ValueError("grad_norm_guard: step and guard are required")
    out.copy_((torch.linalg.vector_norm(g.double()) * float(grad_scale)).float())
    if bool(torch.isfinite(out)):
        step.add_(1)
        guard[0] = 0.0
    else:
        guard[0] = 1.0
        guard[1] += 1.0
    return out


def averaging_weight(decay, warmup, step):
    """w of st_adam_clip's avg, formed in fp32 as the header spells it."""
    d = np.float32(decay)
    if warmup:
        t = np.float32(step)
        d = min(d, (np.float32(1.0) + t) / (np.float32(10.0) + t))
    return np.float32(1.0) - np.float32(d)


def adam_clip_avg(p, g, m, v, lr, step, gnorm, max_norm, beta1, beta2, eps, grad_scale=1.0, found_inf=None, avg=None,
                  decay=0.999, decay_warmup=True):
    if avg is not None and not 0.0 <= float(decay) <= 1.0:
        raise ValueError("adam_clip_avg: decay must lie in [0, 1]")
    if found_inf is not None and float(found_inf) != 0.0:
        return
    _emul.adam_clip(p, g, m, v, lr, step, gnorm, max_norm, beta1, beta2, eps, grad_scale=grad_scale)
    if avg is not None:
        w = float(averaging_weight(decay, decay_warmup, float(step)))
        if w != 0.0:
            avg.add_(w * (p - avg))


def swap_(a, b):
    if a.numel() != b.numel() or a.numel() % 4:
        raise ValueError("swap_: the buffers must hold the same multiple of 4 elements")
    tmp = a.clone()
    a.copy_(b)
    b.copy_(tmp)


_NAMES = ["grad_norm_guard", "adam_clip_avg", "swap_"]


@contextlib.contextmanager
def emulated_optim():
    """Inside tests._emul.emulated_kernels(): the three wrappers as well."""
    saved = {n: getattr(nv, n) for n in _NAMES}
    try:
        for n in _NAMES:
            setattr(nv, n, torch.no_grad()(globals()[n]))
        yield
    finally:
        for n, f in saved.items():
            setattr(nv, n, f)
