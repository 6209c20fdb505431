"""-m gpu: gradient accumulation on the hardware - st_grad_norm / st_adam_clip with a window against the forms without
one (bit for bit at a denominator of 1) and against an fp64 evaluation of Adam per element, st_accum_note /
st_window_close on exact values, then TrainStep(accumulate=K) against the fp64 oracle's full-batch gradient (the bodies of
tests/test_accum_cpu.py), through bucket captures, and two consecutive windows through captured graphs.

Sizes (tests/test_averaging_gpu.py): n = 4 is one 16-byte element; 1,028 one element past a workgroup; 4,194,308 one element
past a full pass of the update's 4,096 x 256 grid, so exactly one thread takes a second trip.

The fp64 bound of the update, per element: |x - want| <= 2^-20 max(|x|, |want|) for x in p, m, v.  The body is pinned bit for bit
at a denominator of 1; a denominator of 37 changes ONE fp32 scalar, the coefficient c every gradient element is multiplied by.
``want`` is Adam in fp64 from the fp32 inputs, with the constants the kernel holds in fp32 (beta1, beta2, eps, the rate) taken
as those fp32 values and c formed in fp64 from the fp32 norm the norm kernel returned; the kernel's c carries 3 roundings (the sum
and the quotient of the clip, the division by the denominator): 3 * 2^-24 relative.  In units of 2^-24:
  m = m0 + (1 - beta1) (c g - m0): c (3), c g, the difference, the product, the sum - at most 0.8 max(|c g|, |m0|) + |m|;
  v = beta2 v0 + (1 - beta2) (c g)^2: c twice (6), c g twice (2), four more - at most 12 |v|;
  p = p0 - u, u = lr / bc1 * m / (sqrt(v) / sqrt(bc2) + eps): m (9), half of v's (6), powf twice, sqrtf twice, two quotients, a
      sum, a product - below 30 |u|, plus 1 |p| for the difference.
For these to be fractions of the RESULTS the inputs avoid cancellation and keep u small: m0 has the sign of g (|m| >= 0.1
max(|c g|, |m0|), so m is within 9 |m|), v0 >= 0.025 (|u| <= 0.0369 * 0.245 * |m| / 0.156 < 0.1 for |m| < 1.7), |p0| >= 0.5
(30 * 0.1 + 0.6 < 16 * 0.4).  All three stay below 16 = 2^-20.  A denominator not applied, applied twice, or applied to the norm
only is off by a factor of 37 in c: orders of magnitude beyond the bound in m and v."""
import functools

import numpy as np
import pytest
import torch

from tests._local import Guarded
from tests.test_accum_cpu import SPLITS, micro, rel, run_accum_bucket_mode, run_window_vs_oracle, watch_g_eff
from tests.test_composition_cpu import _build, _load_c1

pytestmark = pytest.mark.gpu

SIZES = [4, 1028, 4194308]
HYPER = dict(max_norm=1.0, beta1=0.9, beta2=0.98, eps=1e-9)
BOUND = 2.0 ** -20


def _scalar(v):
    return torch.tensor(float(v), dtype=torch.float32, device="cuda")


def _win(d, device="cuda"):
    return torch.tensor([float(d), 0.0, 0.0, 0.0], dtype=torch.float32, device=device)


def _bits(*ts):
    return [t.detach().clone().view(torch.int32) for t in ts]


def _guarded(src):
    gd = Guarded.vec(src.numel(), torch.float32, "cuda")
    gd.view.copy_(src)
    return gd


@functools.lru_cache(maxsize=None)
def _inputs(n):
    """(p0, g, m0, v0, avg0) on the GPU; see the module docstring for the shape of p0 and m0."""
    gen = torch.Generator().manual_seed(n)
    g = torch.randn(n, generator=gen)
    p0 = torch.randn(n, generator=gen)
    p0 = torch.where(p0 >= 0, p0 + 0.5, p0 - 0.5)
    m0 = torch.sign(g) * torch.randn(n, generator=gen).abs() * 0.3
    v0 = (torch.randn(n, generator=gen).abs() + 0.5).pow(2) * 0.1
    a0 = torch.randn(n, generator=gen) * 0.1
    return tuple(t.cuda() for t in (p0, g, m0, v0, a0))


def _run(n, update, win=None, guarded=False, step0=2.0):
    """One norm + update over guarded copies of _inputs(n) (rank scale 0.5, the clip active, averaging on; guarded: the norm's
    verdict is the update's found_inf) -> (the guarded buffers p, g, m, v, avg, the norm)."""
    from st_amd import native as nv
    bufs = [_guarded(t) for t in _inputs(n)]
    p, g, m, v, a = bufs
    scratch, lr, step = nv.grad_norm_scratch("cuda"), _scalar(1e-2), _scalar(step0)
    guard = torch.zeros(2, device="cuda")
    out = torch.empty((), device="cuda")
    if win is None:
        gnorm = nv.grad_norm_guard(g.view, scratch, out, step, guard, grad_scale=0.5)
    else:
        gnorm = nv.grad_norm_win(g.view, scratch, out, step, guard, win, grad_scale=0.5)
    assert float(step) == step0 + 1 and guard.tolist() == [0.0, 0.0]
    update(p.view, g.view, m.view, v.view, lr, step, gnorm, a.view, guard[:1] if guarded else None)
    torch.cuda.synchronize()
    for name, gd in zip(("p", "g", "m", "v", "avg"), bufs):
        gd.assert_intact("%s, n = %d" % (name, n))
    return bufs, gnorm


def _avg_update(p, g, m, v, lr, step, gnorm, a, found_inf):
    from st_amd import native as nv
    nv.adam_clip_avg(p, g, m, v, lr, step, gnorm, grad_scale=0.5, found_inf=found_inf, avg=a, decay=0.9, decay_warmup=False, **HYPER)


def _win_update(win):
    def update(p, g, m, v, lr, step, gnorm, a, found_inf):
        from st_amd import native as nv
        nv.adam_clip_win(p, g, m, v, lr, step, gnorm, win=win, grad_scale=0.5, found_inf=found_inf, avg=a, decay=0.9,
                         decay_warmup=False, **HYPER)
    return update


# ---- 1. the two extended kernels ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("guarded", [False, True])
@pytest.mark.parametrize("n", SIZES)
def test_adam_clip_win_at_denominator_one_is_adam_clip_avg_and_leaves_zeros(n, guarded):
    want, gn_want = _run(n, _avg_update, guarded=guarded)
    got, gn_got = _run(n, _win_update(_win(1)), win=_win(1), guarded=guarded)
    assert torch.equal(*_bits(gn_got, gn_want))
    for name, a, b in zip(("p", "g", "m", "v", "avg"), got, want):
        if name == "g":
            assert float(a.view.abs().max()) == 0.0 and float(b.view.abs().max()) > 0       # zeros, where the plain kernel clips
            continue
        x, y = _bits(a.view, b.view)
        assert torch.equal(x, y), "%s differs in %d elements" % (name, int((x != y).sum()))
    assert not torch.equal(got[0].view, _inputs(n)[0])


@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("denom", [37.0, 32.0])
def test_adam_clip_win_against_fp64_adam(n, denom):
    win = _win(denom)
    got, gnorm = _run(n, _win_update(win), win=win)
    p0, g, m0, v0, _ = (t.double() for t in _inputs(n))
    f32 = lambda x: float(np.float32(x))          # noqa: E731 - the constants as the kernel holds them
    b1, b2, eps, lr, step = f32(0.9), f32(0.98), f32(1e-9), f32(1e-2), 3.0
    norm64 = float(torch.linalg.vector_norm(g)) * 0.5 / denom
    assert abs(float(gnorm) - norm64) <= 1e-5 * norm64, (float(gnorm), norm64)
    coef = min(1.0 / (float(gnorm) + f32(1e-6)), 1.0) * 0.5 / denom
    ge = g * coef
    m = m0 + (1.0 - b1) * (ge - m0)
    v = b2 * v0 + (1.0 - b2) * ge * ge
    bc1, bc2 = 1.0 - b1 ** step, 1.0 - b2 ** step
    p = p0 - (lr / bc1) * m / (v.sqrt() / bc2 ** 0.5 + eps)
    for name, gd, want in (("p", got[0], p), ("m", got[2], m), ("v", got[3], v)):
        x = gd.view.double()
        err, bound = (x - want).abs(), BOUND * torch.maximum(x.abs(), want.abs())
        worst = int((err - bound).argmax())
        print("n %d denominator %g %s: worst |x - want| / max(|x|, |want|) = %.3e (bound %.3e)"
              % (n, denom, name, float((err / torch.maximum(x.abs(), want.abs()).clamp_min(1e-300)).max()), BOUND))
        assert bool((err <= bound).all()), "%s: element %d: got %.9g, want %.9g" % (name, worst, float(x[worst]), float(want[worst]))
    assert float(got[1].view.abs().max()) == 0.0


@pytest.mark.parametrize("n", SIZES)
def test_found_inf_writes_only_the_zeros(n):
    from st_amd import native as nv
    p0, g0, m0, v0, a0 = _inputs(n)
    bad = g0.clone()
    bad[0], bad[n // 2], bad[-1] = float("nan"), float("inf"), float("-inf")
    bufs = [_guarded(t) for t in (p0, bad, m0, v0, a0)]
    before = _bits(*(b.view for b in bufs))
    nv.adam_clip_win(*(b.view for b in bufs[:4]), _scalar(1e-2), _scalar(3), _scalar(float("nan")), win=_win(37), grad_scale=0.5,
                     found_inf=_scalar(1), avg=bufs[4].view, decay=0.9, decay_warmup=True, **HYPER)
    torch.cuda.synchronize()
    for name, b, x in zip(("p", "g", "m", "v", "avg"), bufs, before):
        b.assert_intact(name)
        if name == "g":
            assert torch.equal(b.view.view(torch.int32), torch.zeros_like(x)), "g must hold zeros (+0.0)"
        else:
            assert torch.equal(b.view.view(torch.int32), x), name


@pytest.mark.parametrize("n", SIZES)
def test_grad_norm_win_is_grad_norm_guard_over_a_denominator(n):
    from st_amd import native as nv
    g = _inputs(n)[1]
    scratch, scratch2 = nv.grad_norm_scratch("cuda"), nv.grad_norm_scratch("cuda")
    step, step2, guard, guard2 = _scalar(4), _scalar(4), torch.zeros(2, device="cuda"), torch.zeros(2, device="cuda")
    one = _win(1)
    for scale in (1.0, 0.25):
        want = nv.grad_norm_guard(g, scratch2, torch.empty((), device="cuda"), step2, guard2, grad_scale=scale)
        got = nv.grad_norm_win(g, scratch, torch.empty((), device="cuda"), step, guard, one, grad_scale=scale)
        assert torch.equal(got.view(torch.int32), want.view(torch.int32)), (float(got), float(want))
        free = nv.grad_norm_win(g, scratch, torch.empty((), device="cuda"), step, None, one, grad_scale=scale)      # no guard
        assert torch.equal(free.view(torch.int32), want.view(torch.int32))
    assert float(step) == 8.0 and float(step2) == 6.0 and guard.tolist() == [0.0, 0.0]
    got = nv.grad_norm_win(g, scratch, torch.empty((), device="cuda"), step, guard, _win(37), grad_scale=0.25)
    ref = float(torch.linalg.vector_norm(g.double())) * 0.25 / 37.0
    assert abs(float(got) - ref) <= 1e-5 * ref, (float(got), ref)
    assert float(step) == 9.0 and guard.tolist() == [0.0, 0.0]
    # a window without a denominator is a bad verdict: the step count stays, the ticket is back at zero
    for k, d in enumerate((0.0, -3.0), start=1):
        nv.grad_norm_win(g, scratch, torch.empty((), device="cuda"), step, guard, _win(d))
        assert float(step) == 9.0 and guard.tolist() == [1.0, float(k)], (d, guard.tolist())
    bad = g.clone()
    bad[n - 1] = float("nan")
    got = nv.grad_norm_win(bad, scratch, torch.empty((), device="cuda"), step, guard, _win(37))
    assert not bool(torch.isfinite(got)) and float(step) == 9.0 and guard.tolist() == [1.0, 3.0]
    assert int(scratch[-1].view(torch.int32)) == 0
    got = nv.grad_norm_win(g, scratch, torch.empty((), device="cuda"), step, guard, one, grad_scale=0.25)      # a finite launch works
    assert torch.equal(got.view(torch.int32), want.view(torch.int32)) and float(step) == 10.0 and guard.tolist() == [0.0, 3.0]


# ---- 2. the window's two small launches -----------------------------------------------------------------------------------------
def test_accum_note_and_window_close_on_exact_values():
    from st_amd import native as nv
    win, out4 = _guarded(torch.zeros(4)), _guarded(torch.full((4,), 7.0))
    one = _guarded(torch.zeros(1))
    notes = [([12.0, 8.0, 0.0, 1.25], 1.5), ([6.0, 8.0, 0.0, 0.75], 0.75), ([0.0, 0.0, 0.0, float("nan")], float("nan"))]
    for vals, want in notes:                                      # "tokens": the denominator is sums[1] itself
        sums = torch.tensor(vals, device="cuda")
        nv.accum_note(sums, sums[1:2], win.view, one.view)
        got = float(one.view[0])
        assert got == want or (want != want and got != got), (vals, got)
    assert win.view.tolist() == [16.0, 18.0, 16.0, 3.0]           # (the empty micro-batch adds no NLL: 0 tokens, 0 / 0 mean)
    nv.window_close(win.view, out4.view)
    assert out4.view.tolist() == [1.125, 1.0, 16.0, 3.0] and win.view.tolist() == [0.0] * 4
    rows = torch.tensor([16.0], device="cuda")                    # "rows": a staged denominator
    nv.accum_note(torch.tensor([12.0, 8.0, 0.0, 1.25], device="cuda"), rows, win.view, one.view)
    assert float(one.view[0]) == 0.75 and win.view.tolist() == [16.0, 12.0, 10.0, 1.0]
    nv.accum_note(torch.tensor([4.0, 4.0, 0.0, 0.5], device="cuda"), rows, win.view, one.view)
    nv.window_close(win.view, out4.view)
    assert out4.view.tolist() == [0.5, 0.375, 32.0, 2.0] and win.view.tolist() == [0.0] * 4
    for _ in range(2):                                            # "sum": no division, the denominator stays 1
        nv.accum_note(torch.tensor([12.0, 8.0, 0.0, 1.25], device="cuda"), None, win.view, one.view)
        assert float(one.view[0]) == 12.0
    assert win.view.tolist() == [1.0, 24.0, 20.0, 2.0]
    nv.window_close(win.view, out4.view)
    assert out4.view.tolist() == [24.0, 20.0, 1.0, 2.0]
    torch.cuda.synchronize()
    for name, gd in (("win", win), ("out", out4), ("loss", one)):
        gd.assert_intact(name)


# ---- 3. a window against the fp64 full-batch truth -----------------------------------------------------------------------------
@pytest.mark.parametrize("use_graph", [False, True])
@pytest.mark.parametrize("split", SPLITS)
def test_window_vs_oracle_on_the_gpu(golden_dir, split, use_graph):
    step, _ = run_window_vs_oracle(golden_dir, "cuda", split, "plain", use_graph)
    if use_graph:
        assert len(step._graphs) == len(split) and step._g_opt is not None


@pytest.mark.parametrize("kind", ["ce", "ls"])
def test_smoothed_window_vs_oracle_on_the_gpu(golden_dir, kind):
    run_window_vs_oracle(golden_dir, "cuda", SPLITS[0], kind, use_graph=True)


# ---- 4. bucket modes through captures ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("bucket_rows", [None, (340, 48)])
def test_accum_bucket_mode_on_the_gpu(bucket_rows):
    run_accum_bucket_mode("cuda", use_graph=True, bucket_rows=bucket_rows)


# ---- 5. the fused zeroing ------------------------------------------------------------------------------------------------------
def test_two_consecutive_windows_through_captured_graphs_consume_the_same_gradient(golden_dir):
    """The same two micro-batches twice, near-zero learning rate: the second window's g_eff is the first's up to the order of
    the fp32 atomics (1e-5).  A gradient buffer the update did not clear doubles it; a window state that was not reset halves it."""
    from st_amd.trainer import TrainStep
    from transformer.Optim import ScheduledOptim
    from tests.test_accum_cpu import _cfg
    _, w, batch = _load_c1(golden_dir)
    m = _build(w, device="cuda")
    opt = ScheduledOptim(m, 128, _cfg())
    step = TrainStep(m, opt, 30, 1e9, use_graph=True, graph_warmup=1, accumulate=2)
    box = watch_g_eff(step)
    parts = [micro(batch, part, "cuda") for part in SPLITS[0]]
    losses = []
    for _ in range(3):                    # window 1: eager warm-ups; windows 2 and 3: replays of the two captures
        for part in parts:
            loss, gnorm = step(*part)
            losses.append(float(loss))
    assert len(box) == 3 and len(step._graphs) == 2 and step._last_cap is not None
    (g1, w1), (g2, w2) = box[1], box[2]
    assert w1.tolist()[0] == w2.tolist()[0] == 32.0 and w1.tolist()[3] == w2.tolist()[3] == 2.0
    assert rel(g2, g1) <= 1e-5, rel(g2, g1)
    assert rel(g1, box[0][0]) <= 1e-5                                  # ... and the eager window's
    assert losses[2:4] == pytest.approx(losses[4:6], rel=1e-6)
    assert float(opt.arena.grad.abs().max()) == 0.0 and step._win.tolist() == [0.0] * 4
    assert float(opt._flat_state()[1]["step"]) == 3.0 and step.global_step == 3 and bool(torch.isfinite(gnorm))
