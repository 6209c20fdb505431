"""Test-only torch emulations of the gradient-accumulation wrappers of st_amd.native (accum_note, window_close,
grad_norm_win, adam_clip_win), like tests/_emul_optim.py: the host logic of TrainStep(accumulate=K) / ScheduledOptim runs on CPU
tensors against them.  The arithmetic follows include/st_hip.h; it is NOT the kernels' rounding (the -m gpu tests pin that on
hardware)."""
import contextlib

import torch

from st_amd import native as nv


def accum_note(sums, d, win, out):
    if sums.numel() != 4 or win.numel() != 4:
        raise ValueError("accum_note: sums and win hold 4 elements")
    s, n = sums[0].clone(), float(sums[1])
    win[1] += s
    if n > 0:
        win[2] += sums[3] * sums[1]
    win[3] += 1.0
    if d is None:
        win[0] = 1.0
        out[0] = s
    else:
        dd = d.reshape(-1)[0].clone()
        win[0] += dd
        out[0] = s / dd
    return out


def window_close(win, out):
    d = win[0].clone()
    out[0] = win[1] / d
    out[1] = win[2] / d
    out[2] = d
    out[3] = win[3]
    win.zero_()
    return out


def grad_norm_win(g, scratch, out, step, guard, win, grad_scale=1.0):
    if step is None or win is None:
        raise ValueError("grad_norm_win: step and win are required")
    out.copy_((torch.linalg.vector_norm(g.double()) * float(grad_scale) / win[0].double()).float())
    if guard is None:
        step.add_(1)
    elif bool(torch.isfinite(out)) and float(win[0]) > 0:
        step.add_(1)
        guard[0] = 0.0
    else:
        guard[0] = 1.0
        guard[1] += 1.0
    return out


def adam_clip_win(p, g, m, v, lr, step, gnorm, max_norm, beta1, beta2, eps, win, grad_scale=1.0, found_inf=None, avg=None,
                  decay=0.999, decay_warmup=True):
    if win is None:
        raise ValueError("adam_clip_win: win is required")
    if avg is not None and not 0.0 <= float(decay) <= 1.0:
        raise ValueError("adam_clip_win: decay must lie in [0, 1]")
    if found_inf is None or float(found_inf) == 0.0:
        from tests._emul_optim import adam_clip_avg
        adam_clip_avg(p, g, m, v, lr, step, gnorm, max_norm, beta1, beta2, eps, grad_scale=float(grad_scale) / float(win[0]),
                      found_inf=None, avg=avg, decay=decay, decay_warmup=decay_warmup)
    g.zero_()


_NAMES = ["accum_note", "window_close", "grad_norm_win", "adam_clip_win"]


@contextlib.contextmanager
def emulated_accum():
    """Inside tests._emul.emulated_kernels(): the four wrappers as well."""
    saved = {n: getattr(nv, n) for n in _NAMES}
    try:
        for n in _NAMES:
            setattr(nv, n, torch.no_grad()(globals()[n]))
        yield
    finally:
        for n, f in saved.items():
            setattr(nv, n, f)
