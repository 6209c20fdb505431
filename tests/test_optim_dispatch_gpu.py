"""-m gpu: the dispatch of the two optimizer entry points.  st_grad_norm and st_adam_clip choose an instantiation of their one
kernel body by which optional pointers are non-NULL; this calls them through native.load() directly, once per combination, and
holds every result to the test-only emulations (tests/_emul.py, _emul_optim.py, _emul_accum.py) evaluated in fp64 on the same
inputs.  The bitwise relations between the forms are held by tests/test_averaging_gpu.py and tests/test_accum_gpu.py.

Sizes.  st_adam_clip's grid is min(4096, ceil(n4 / 256)) workgroups of 256 over n4 = n / 4 16-byte elements: n = 4 is one active
thread; 4 * 257 two workgroups, the second with one; 4 * (1,048,576 + 7) seven elements past a full pass of the 4,096 x 256
grid, so the grid-stride loop takes a second trip.  st_grad_norm's is min(256, ceil(n4 / 1024)) of 1024: n = 4; 4 * (2 * 1024 + 1)
three workgroups with a ragged tail; 4 * (262,144 + 5) five elements past a full pass of 256 x 1024.

Bounds are the ones those two files derive and use: tests.test_accum_gpu.BOUND for p, m, v per element against fp64 Adam (its
docstring's rounding count, with its inputs, step count and constants - which is why they are taken from there; g, where the
clipped gradient is left, carries the coefficient's 3 roundings and one product: 4 of its 16 units), tests.test_averaging_gpu's
AVG_BOUND for the average, and 1e-5 relative for the norm."""
import numpy as np
import pytest
import torch

from tests import _emul, _emul_accum, _emul_optim
from tests._local import Guarded
from tests.test_accum_gpu import BOUND, HYPER, _inputs
from tests.test_averaging_gpu import AVG_BOUND

pytestmark = pytest.mark.gpu

ADAM_SIZES = [4, 4 * 257, 4 * (1048576 + 7)]
NORM_SIZES = [4, 4 * (2 * 1024 + 1), 4 * (262144 + 5)]
DENOM, SCALE, LR, STEP, DECAY = 37.0, 0.5, 1e-2, 3.0, 0.9


def _f32(x):
    return float(np.float32(x))          # a constant as the kernel holds it


def _scalar(v):
    return torch.tensor(float(v), dtype=torch.float32, device="cuda")


def _guarded(src):
    gd = Guarded.vec(src.numel(), torch.float32, "cuda")
    gd.view.copy_(src)
    return gd


def _stream():
    from st_amd import native as nv
    return nv._stream()


def _within(x, want, bound, scale, what):
    err, lim = (x.double() - want).abs(), bound * scale
    worst = int((err - lim).argmax())
    print("%s: worst error / scale = %.3e (bound %.3e)" % (what, float((err / scale.clamp_min(1e-300)).max()), bound))
    assert bool((err <= lim).all()), "%s: element %d: got %.9g, want %.9g" % (what, worst, float(x[worst]), float(want[worst]))


# ---- st_adam_clip: eight (found_inf, avg, win) combinations ------------------------------------------------------------------------
@pytest.mark.parametrize("n", ADAM_SIZES)
@pytest.mark.parametrize("has_inf,has_avg,has_win", [(i, a, w) for i in (False, True) for a in (False, True) for w in (False, True)])
def test_adam_clip_every_pointer_combination_against_the_emulation(n, has_inf, has_avg, has_win):
    from st_amd import native as nv
    lib = nv.load()
    p0, g0, m0, v0, a0 = _inputs(n)
    gnorm = _scalar(float(torch.linalg.vector_norm(g0.double())) * SCALE / (DENOM if has_win else 1.0))      # > 1: the clip is active
    lr, step, win = _scalar(LR), _scalar(STEP), torch.tensor([DENOM, 0.0, 0.0, 0.0], device="cuda")
    for verdict in ((0.0, 1.0) if has_inf else (None,)):
        found = None if verdict is None else _scalar(verdict)
        bufs = [_guarded(t) for t in (p0, g0, m0, v0, a0)]
        p, g, m, v, a = (b.view for b in bufs)
        rc = lib.st_adam_clip(_stream(), n, p.data_ptr(), g.data_ptr(), m.data_ptr(), v.data_ptr(), lr.data_ptr(), step.data_ptr(),
                              gnorm.data_ptr(), HYPER["max_norm"], HYPER["beta1"], HYPER["beta2"], HYPER["eps"], SCALE,
                              nv._p(found), a.data_ptr() if has_avg else None, DECAY, 0, win.data_ptr() if has_win else None)
        assert rc == 0
        torch.cuda.synchronize()
        for name, b in zip(("p", "g", "m", "v", "avg"), bufs):
            b.assert_intact("%s, n = %d" % (name, n))
        # the emulation in fp64, the constants as the kernel holds them in fp32
        wp, wg, wm, wv, wa = (t.double().clone() for t in (p0, g0, m0, v0, a0))
        hyper = (_f32(LR), STEP, float(gnorm), _f32(HYPER["max_norm"]), _f32(HYPER["beta1"]), _f32(HYPER["beta2"]), _f32(HYPER["eps"]))
        kw = dict(grad_scale=SCALE, found_inf=found, avg=wa if has_avg else None, decay=DECAY, decay_warmup=False)
        if has_win:
            _emul_accum.adam_clip_win(wp, wg, wm, wv, *hyper, win=win.double(), **kw)
        else:
            _emul_optim.adam_clip_avg(wp, wg, wm, wv, *hyper, **kw)
        what = "n %d found_inf %s avg %s win %s" % (n, verdict, has_avg, has_win)
        if verdict == 1.0:               # a skipped update: nothing is written - under a window, only the zeros into g
            for name, x, src in (("p", p, p0), ("m", m, m0), ("v", v, v0), ("avg", a, a0)):
                assert torch.equal(x.view(torch.int32), src.view(torch.int32)), "%s: %s was written" % (what, name)
            assert torch.equal(g, torch.zeros_like(g) if has_win else g0) and torch.equal(wg.float(), g)
            continue
        for name, x, want in (("p", p, wp), ("m", m, wm), ("v", v, wv), ("g", g, wg)):
            _within(x, want, BOUND, torch.maximum(x.double().abs(), want.abs()), "%s: %s" % (what, name))
        assert not torch.equal(p, p0) and (float(g.abs().max()) == 0.0) == has_win
        if has_avg:
            _within(a, wa, AVG_BOUND, torch.maximum(a.abs(), p.abs()).double(), "%s: avg" % what)
            assert not torch.equal(a, a0)
        else:
            assert torch.equal(a.view(torch.int32), a0.view(torch.int32))


# ---- st_grad_norm: the five legal (step, guard, win) combinations ------------------------------------------------------------------
@pytest.mark.parametrize("n", NORM_SIZES)
@pytest.mark.parametrize("has_step,has_guard,has_win", [(False, False, False), (True, False, False), (True, True, False),
                                                        (True, False, True), (True, True, True)])
def test_grad_norm_every_legal_pointer_combination_against_the_emulation(n, has_step, has_guard, has_win):
    from st_amd import native as nv
    lib = nv.load()
    g0 = _inputs(ADAM_SIZES[-1])[1][:n]
    bad = g0.clone()
    bad[n - 1] = float("nan")
    scratch = nv.grad_norm_scratch("cuda")
    step, guard, out = _scalar(4), torch.zeros(2, device="cuda"), _guarded(torch.zeros(1))
    wstep, wguard, wout = step.clone(), guard.clone(), torch.zeros((), device="cuda")
    # a finite gradient, then (with a guard) a NaN element, then a window without a denominator - on one scratch, one step count
    cases = [(g0, DENOM)] + ([(bad, DENOM)] if has_guard else []) + ([(g0, 0.0)] if has_guard and has_win else [])
    for g, denom in cases:
        gg = _guarded(g)
        win = torch.tensor([denom, 0.0, 0.0, 0.0], device="cuda")
        rc = lib.st_grad_norm(_stream(), gg.view.data_ptr(), n, scratch.data_ptr(), out.view.data_ptr(), step.data_ptr() if has_step else None,
                              SCALE, guard.data_ptr() if has_guard else None, win.data_ptr() if has_win else None)
        assert rc == 0
        torch.cuda.synchronize()
        gg.assert_intact("g, n = %d" % n), out.assert_intact("gnorm")
        assert torch.equal(gg.view.view(torch.int32), g.view(torch.int32))
        if has_win:
            _emul_accum.grad_norm_win(g, None, wout, wstep, wguard if has_guard else None, win, grad_scale=SCALE)
        elif has_guard:
            _emul_optim.grad_norm_guard(g, None, wout, wstep, wguard, grad_scale=SCALE)
        else:
            _emul.grad_norm(g, None, wout, step=wstep if has_step else None, grad_scale=SCALE)
        got, want = float(out.view[0]), float(wout)
        if np.isfinite(want):
            assert abs(got - want) <= 1e-5 * want, (n, denom, got, want)
        else:
            assert not np.isfinite(got), (n, denom, got, want)
        assert float(step) == (float(wstep) if has_step else 4.0) and guard.tolist() == (wguard.tolist() if has_guard else [0.0, 0.0])
    assert int(scratch[-1].view(torch.int32)) == 0          # the ticket is back at zero


# ---- arguments the entry points refuse: -1, nothing launched -----------------------------------------------------------------------
def test_refused_arguments_return_minus_one_and_launch_nothing():
    from st_amd import native as nv
    lib = nv.load()
    bufs = [_guarded(torch.ones(8)) for _ in range(4)]
    scratch, out, step = nv.grad_norm_scratch("cuda"), _guarded(torch.zeros(1)), _scalar(4)
    guard, win, lr = torch.zeros(2, device="cuda"), torch.tensor([1.0, 0.0, 0.0, 0.0], device="cuda"), _scalar(LR)
    before = [b.buf.clone() for b in bufs] + [scratch.clone(), out.buf.clone()]
    g = bufs[1].view.data_ptr()
    norm = lambda n, s, gd, w: lib.st_grad_norm(_stream(), g, n, scratch.data_ptr(), out.view.data_ptr(), s, 1.0, gd, w)      # noqa: E731
    assert norm(8, None, guard.data_ptr(), None) == -1               # a verdict needs the step count it holds back
    assert norm(8, None, None, win.data_ptr()) == -1                 # ... and so does a window
    assert norm(8, None, guard.data_ptr(), win.data_ptr()) == -1
    for gd, w in ((None, None), (guard.data_ptr(), None), (None, win.data_ptr()), (guard.data_ptr(), win.data_ptr())):
        assert norm(6, step.data_ptr(), gd, w) == -1                 # n & 3
        assert norm(0, step.data_ptr(), gd, w) == -1
    for found, avg, w in ((None, None, None), (guard.data_ptr(), bufs[0].view.data_ptr(), win.data_ptr())):
        rc = lib.st_adam_clip(_stream(), 6, *(b.view.data_ptr() for b in bufs), lr.data_ptr(), step.data_ptr(), None, 1.0, 0.9, 0.98,
                              1e-9, 1.0, found, avg, DECAY, 0, w)
        assert rc == -1                                              # n & 3
    torch.cuda.synchronize()
    after = [b.buf for b in bufs] + [scratch, out.buf]
    assert all(torch.equal(x.view(torch.int32), y.view(torch.int32)) for x, y in zip(before, after))
    assert float(step) == 4.0 and guard.tolist() == [0.0, 0.0]
