"""-m gpu: the optimizer update that skips non-finite gradients and keeps averaged weights - st_grad_norm with a guard,
st_adam_clip with found_inf / avg, st_swap_f32 against the plain st_grad_norm / st_adam_clip (bit for bit) and an fp64 evaluation of the averaging
recursion, then the same through TrainStep (graph mode), optimizer.averaged() and JointTrainStep(ctc="hip").

Sizes: n = 4 is one 16-byte element; 1,028 one element past a 256-thread workgroup (and past a 1,024-thread one of the norm);
4,194,308 one element past a full pass of st_adam_clip's 4,096 x 256 grid, so exactly one thread takes a second trip.

The averaging bound, per element: |avg - want| <= 2^-20 max(|avg|, |p|), want = the recursion in fp64 from the previous average
as stored, the kernel's own new p and w formed in fp32 on the host.  Three fp32 roundings (p - avg, the product, the sum) give
at most 3.5 * 2^-23 of that maximum, one ulp of d another 2^-23; a wrong w (another step count, decay for 1 - decay) is off by
1e-3 and more."""
import functools

import pytest
import torch

from tests._emul_optim import averaging_weight
from tests._local import Guarded

pytestmark = pytest.mark.gpu

SIZES = [4, 1028, 4194308]
BIG = SIZES[-1]
HYPER = dict(max_norm=1.0, beta1=0.9, beta2=0.98, eps=1e-9)
AVG_BOUND = 2.0 ** -20


def _scalar(v):
    return torch.tensor(float(v), dtype=torch.float32, device="cuda")


def _bits(*ts):
    return [t.detach().clone().view(torch.int32) for t in ts]


def _guarded(src):
    gd = Guarded.vec(src.numel(), torch.float32, "cuda")
    gd.view.copy_(src)
    return gd


@functools.lru_cache(maxsize=None)
def _inputs(n):
    g = torch.Generator().manual_seed(n)
    return (torch.randn(n, generator=g).cuda(), [torch.randn(n, generator=g).cuda() for _ in range(3)],
            (torch.randn(n, generator=g) * 0.1).cuda())


def _three_steps(n, update, avg=False):
    """p, m, v (and avg) in guarded buffers through 3 consecutive updates, the gradient norm from st_grad_norm with a rank
    scale of 0.5, the clip active; -> the int32 views of (p, g, m, v[, avg]) after every step."""
    from st_amd import native as nv
    p0, grads, a0 = _inputs(n)
    gp, gm, gv = _guarded(p0), _guarded(torch.zeros(n)), _guarded(torch.zeros(n))
    ga = _guarded(a0) if avg else None
    scratch, lr, step = nv.grad_norm_scratch("cuda"), _scalar(1e-2), _scalar(0)
    out = []
    for g in grads:
        gg = _guarded(g)
        gnorm = nv.grad_norm(gg.view, scratch, torch.empty((), device="cuda"), step=step, grad_scale=0.5)
        update(gp.view, gg.view, gm.view, gv.view, lr, step, gnorm, ga.view if avg else None)
        for gd in (gp, gg, gm, gv) + ((ga,) if avg else ()):
            gd.assert_intact("n = %d" % n)
        out.append(_bits(gp.view, gg.view, gm.view, gv.view, *((ga.view,) if avg else ())))
    assert float(step) == 3.0
    return out


@functools.lru_cache(maxsize=None)
def _reference(n):
    from st_amd import native as nv
    return _three_steps(n, lambda p, g, m, v, lr, step, gnorm, avg: nv.adam_clip(p, g, m, v, lr, step, gnorm, grad_scale=0.5, **HYPER))


# ---- 1. one kernel body: the new entry point with nothing switched on is st_adam_clip ------------------------------------------
@pytest.mark.parametrize("n", SIZES)
def test_adam_clip_avg_without_options_equals_adam_clip_bit_for_bit(n):
    from st_amd import native as nv
    got = _three_steps(n, lambda p, g, m, v, lr, step, gnorm, avg: nv.adam_clip_avg(p, g, m, v, lr, step, gnorm, grad_scale=0.5,
                                                                                  found_inf=None, avg=None, **HYPER))
    for it, (a, b) in enumerate(zip(got, _reference(n))):
        for name, x, y in zip("pgmv", a, b):
            assert torch.equal(x, y), "step %d: %s differs in %d elements" % (it + 1, name, int((x != y).sum()))


# ---- 2. the guard ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", SIZES)
def test_found_inf_freezes_all_five_buffers_and_zero_changes_nothing(n):
    from st_amd import native as nv
    # found_inf = 0 (and an average kept beside): p, g, m, v are st_adam_clip's
    zero = _scalar(0)
    got = _three_steps(n, lambda p, g, m, v, lr, step, gnorm, avg: nv.adam_clip_avg(
        p, g, m, v, lr, step, gnorm, grad_scale=0.5, found_inf=zero, avg=avg, decay=0.9, decay_warmup=False, **HYPER), avg=True)
    for it, (a, b) in enumerate(zip(got, _reference(n))):
        for name, x, y in zip("pgmv", a, b):
            assert torch.equal(x, y), "step %d: %s differs" % (it + 1, name)
    assert not torch.equal(got[0][4], got[1][4])                 # (the average moved)
    # found_inf = 1: nothing is written, whatever the gradient holds
    p0, grads, a0 = _inputs(n)
    bad = grads[0].clone()
    bad[0], bad[n // 2], bad[-1] = float("nan"), float("inf"), float("-inf")
    bufs = [_guarded(t) for t in (p0, bad, grads[1].abs(), grads[2].abs(), a0)]
    before = _bits(*(b.view for b in bufs))
    nv.adam_clip_avg(*(b.view for b in bufs[:4]), _scalar(1e-2), _scalar(3), _scalar(float("nan")), grad_scale=0.5,
                     found_inf=_scalar(1), avg=bufs[4].view, decay=0.9, decay_warmup=True, **HYPER)
    torch.cuda.synchronize()
    for name, b, x in zip(("p", "g", "m", "v", "avg"), bufs, before):
        assert torch.equal(b.view.view(torch.int32), x), name
        b.assert_intact(name)


@pytest.mark.parametrize("n", SIZES)
def test_grad_norm_guard_is_grad_norm_with_a_verdict(n):
    from st_amd import native as nv
    g = _inputs(n)[1][0].clone()
    scratch, scratch2 = nv.grad_norm_scratch("cuda"), nv.grad_norm_scratch("cuda")
    step, step2, guard = _scalar(4), _scalar(4), torch.zeros(2, device="cuda")
    for scale in (1.0, 0.25):
        want = nv.grad_norm(g, scratch2, torch.empty((), device="cuda"), step=step2, grad_scale=scale)
        got = nv.grad_norm_guard(g, scratch, torch.empty((), device="cuda"), step, guard, grad_scale=scale)
        assert torch.equal(got.view(torch.int32), want.view(torch.int32)), (float(got), float(want))
    assert float(step) == float(step2) == 6.0 and guard.tolist() == [0.0, 0.0]
    ref = float(torch.linalg.vector_norm(g.double())) * 0.25
    assert abs(float(got) - ref) <= 1e-5 * ref
    # non-finite elements at either end; finite values whose squares, or whose sum of squares, overflow fp32
    cases = [(i, v) for v in (float("nan"), float("inf"), float("-inf")) for i in (0, n - 1)]
    cases += [(n - 1, 1e20), (0, -3e19), (None, 1e19)]
    skipped = 0
    for idx, val in cases:
        bad = g.clone()
        if idx is None:
            bad.fill_(val)             # every square is 1e38: the sum of four overflows
        else:
            bad[idx] = val
        got = nv.grad_norm_guard(bad, scratch, torch.empty((), device="cuda"), step, guard)
        skipped += 1
        assert not bool(torch.isfinite(got)), (idx, val, float(got))
        assert float(step) == 6.0 and guard.tolist() == [1.0, float(skipped)], (idx, val, guard.tolist())
        # a finite launch on the same scratch clears the verdict, keeps the count and has the ticket back at zero
        got = nv.grad_norm_guard(g, scratch, torch.empty((), device="cuda"), step, guard, grad_scale=0.25)
        assert torch.equal(got.view(torch.int32), want.view(torch.int32))
        assert guard.tolist() == [0.0, float(skipped)]
        step.fill_(6.0)
    assert int(scratch[-1].view(torch.int32)) == 0


# ---- 3. the average -------------------------------------------------------------------------------------------------------------
def _assert_recursion(avg, prev, p, w, what):
    want = prev.double() + float(w) * (p.double() - prev.double())
    err = (avg.double() - want).abs()
    bound = AVG_BOUND * torch.maximum(avg.abs(), p.abs()).double()
    worst = int((err - bound).argmax())
    print("%s: w %.6f, worst |avg - want| / max(|avg|, |p|) = %.3e (bound %.3e)"
          % (what, float(w), float((err / torch.maximum(avg.abs(), p.abs()).double().clamp_min(1e-300)).max()), AVG_BOUND))
    assert bool((err <= bound).all()), "%s: element %d: avg %.9g, want %.9g" % (what, worst, float(avg[worst]), float(want[worst]))


@pytest.mark.parametrize("warmup", [False, True])
def test_average_follows_the_fp64_recursion_over_20_updates(warmup):
    from st_amd import native as nv
    n = 1028
    gen = torch.Generator().manual_seed(5)
    p, m, v = _guarded(torch.randn(n, generator=gen)), _guarded(torch.zeros(n)), _guarded(torch.zeros(n))
    avg = _guarded(p.view)
    frozen = _guarded(torch.randn(n, generator=gen))
    frozen_bits = _bits(frozen.view)[0]
    lr, step = _scalar(3e-2), _scalar(0)
    ws = []
    for it in range(1, 21):
        g = torch.randn(n, generator=gen).cuda()
        step.add_(1)
        prev = avg.view.clone()
        nv.adam_clip_avg(p.view, g, m.view, v.view, lr, step, None, 0.0, 0.9, 0.98, 1e-9, avg=avg.view, decay=0.99,
                         decay_warmup=warmup)
        w = averaging_weight(0.99, warmup, it)
        ws.append(float(w))
        _assert_recursion(avg.view, prev, p.view, w, "update %d" % it)
        # decay 1.0: the average keeps its bits while the parameters move
        nv.adam_clip_avg(p.view.clone(), g.clone(), m.view.clone(), v.view.clone(), lr, step, None, 0.0, 0.9, 0.98, 1e-9,
                         avg=frozen.view, decay=1.0, decay_warmup=False)
        assert torch.equal(frozen.view.view(torch.int32), frozen_bits)
    for gd in (p, m, v, avg, frozen):
        gd.assert_intact("average")
    assert abs(ws[0] - (1.0 - (2.0 / 11.0 if warmup else 0.99))) < 1e-6 and abs(ws[-1] - (1.0 - (21.0 / 30.0 if warmup else 0.99))) < 1e-6
    assert float((avg.view - p.view).abs().max()) > 1e-3          # (the average is not the parameters)


@pytest.mark.parametrize("n", SIZES)
def test_swap_exchanges_two_buffers_in_place(n):
    from st_amd import native as nv
    a0, grads, _ = _inputs(n)
    a, b = _guarded(a0), _guarded(grads[0])
    nv.swap_(a.view, b.view)
    assert torch.equal(a.view, grads[0]) and torch.equal(b.view, a0)
    a.assert_intact("a"), b.assert_intact("b")
    with pytest.raises(ValueError):
        nv.swap_(a.view, a.view)
    with pytest.raises(ValueError):
        nv.swap_(a.buf.view(-1)[:8], a.buf.view(-1)[4:12])


# ---- 4. - 6. through the step drivers --------------------------------------------------------------------------------------------
def _small(warmup_steps=100):
    from st_amd import synthetic
    from transformer.Models import Transformer
    from transformer.Optim import ScheduledOptim
    from transformer.Utils import AttrDict, init_parameters
    cfg = AttrDict(dict(feature_dim=80, max_inputs_length=200, max_target_length=32, num_enc_layer=2, num_dec_layer=2, n_heads=4,
                        d_k=32, d_v=32, d_model=128, d_inner_hid=256, dropout=0.0, vocab_size=30))
    torch.manual_seed(0)
    model = Transformer(cfg).cuda()
    init_parameters(model)
    model.eval()
    opt = ScheduledOptim(model, 128, AttrDict(n_warmup_steps=warmup_steps))
    inputs, targets, in_len, tgt_len, truth = synthetic.make_batch(2, 160, 20, 80, 30, seed=1, t_min=60, l_min=6)
    return cfg, model, opt, (inputs.cuda(), in_len, targets.cuda(), tgt_len, truth.cuda())


def test_trainstep_graph_mode_averages_and_skips_a_poisoned_batch():
    from st_amd.trainer import TrainStep
    cfg, model, opt, batch = _small()
    opt.enable_nonfinite_guard()
    opt.enable_averaging(decay=0.99, warmup=True)
    arena = opt.arena
    step = TrainStep(model, opt, 30, 5.0, use_graph=True, graph_warmup=2)
    for it in range(1, 6):                                     # two eager warm-ups, the capture + replay, two more replays
        prev = arena.avg.clone()
        loss, gnorm = step(*batch)
        assert bool(torch.isfinite(loss)) and bool(torch.isfinite(gnorm))
        assert float(opt._flat_state()[1]["step"]) == float(it) and float(opt.found_inf) == 0.0
        _assert_recursion(arena.avg, prev, arena.flat, averaging_weight(0.99, True, it), "call %d" % it)
    assert step._g_fb is not None and len(step._graphs) == 1
    assert float((arena.avg - arena.flat).abs().max()) > 0
    st = opt._flat_state()[1]
    watched = (arena.flat, st["exp_avg"], st["exp_avg_sq"], arena.avg, st["step"])
    before = _bits(*watched)
    x = batch[0]
    keep = x[0, 3, 5].clone()
    x[0, 3, 5] = float("inf")                                  # one element of the static input buffer
    loss, gnorm = step(*batch)
    assert not (bool(torch.isfinite(loss)) and bool(torch.isfinite(gnorm))), (float(loss), float(gnorm))
    assert float(opt.found_inf) == 1.0 and float(opt.skipped) == 1.0
    for name, a, b in zip(("parameters", "exp_avg", "exp_avg_sq", "average", "step count"), before, _bits(*watched)):
        assert torch.equal(a, b), name
    x[0, 3, 5] = keep
    prev = arena.avg.clone()
    loss, gnorm = step(*batch)
    assert bool(torch.isfinite(loss)) and bool(torch.isfinite(gnorm))
    assert float(st["step"]) == 6.0 and float(opt.found_inf) == 0.0 and float(opt.skipped) == 1.0 and step.global_step == 7
    assert not torch.equal(arena.flat.view(torch.int32), before[0]) and bool(torch.isfinite(arena.flat).all())
    _assert_recursion(arena.avg, prev, arena.flat, averaging_weight(0.99, True, 6), "after the skip")
    assert len(step._graphs) == 1                               # all of it through the one captured graph
    # the captured graph holds the options it was captured with; inside averaged() the step refuses
    with opt.averaged():
        with pytest.raises(RuntimeError, match="averaged"):
            step(*batch)
    opt._avg_opts = (0.5, True)
    with pytest.raises(RuntimeError, match="options changed"):
        step(*batch)


def test_averaged_puts_the_average_under_the_model_for_eval_and_decode():
    from st_amd.trainer import TrainStep
    from transformer.Decode import Decode
    from transformer.Models import Transformer
    from transformer.Utils import AttrDict
    cfg, model, opt, batch = _small(warmup_steps=20)            # a rate at which three steps move the hypotheses' scores
    opt.enable_averaging(decay=0.5, warmup=False)
    arena = opt.arena
    step = TrainStep(model, opt, 30, 5.0, use_graph=False)
    for _ in range(3):
        step(*batch)
    flat0, avg0 = _bits(arena.flat, arena.avg)
    assert not torch.equal(flat0, avg0)
    # a fresh model loaded from the averaged tensors
    sd = {k: v.detach().clone() for k, v in model.state_dict().items()}
    for name, p in model.named_parameters():
        sd[name] = arena.avg_view(p).detach().clone()
    fresh = Transformer(cfg).cuda()
    fresh.load_state_dict(sd)
    fresh.eval()
    src = (batch[0], batch[1])
    dopt = AttrDict(dict(beam_size=4, n_best=2, max_steps=16))
    want_h, want_s = Decode(dopt, "cuda", model=fresh).decode_batch(src)
    own_h, own_s = Decode(dopt, "cuda", model=model).decode_batch(src)
    with opt.averaged():
        assert torch.equal(arena.flat.view(torch.int32), avg0) and torch.equal(arena.avg.view(torch.int32), flat0)
        with torch.no_grad():
            model(batch[0], batch[1], batch[2], batch[3])
        assert torch.equal(arena.shadow, arena.flat.to(torch.bfloat16))
        got_h, got_s = Decode(dopt, "cuda", model=model).decode_batch(src)
        with pytest.raises(RuntimeError, match="already inside"):
            with opt.averaged():
                pass
    assert got_h == want_h and all(torch.equal(a, b) for a, b in zip(got_s, want_s))
    assert not all(torch.equal(a, b) for a, b in zip(own_s, want_s)), "the averaged weights must decode differently"
    assert torch.equal(arena.flat.view(torch.int32), flat0) and torch.equal(arena.avg.view(torch.int32), avg0)
    with torch.no_grad():
        model(batch[0], batch[1], batch[2], batch[3])
    assert torch.equal(arena.shadow, arena.flat.to(torch.bfloat16))          # and the next forward reads the trained weights again


def test_joint_trainstep_hip_skips_and_averages_the_head_too():
    from st_amd.trainer import JointTrainStep
    from transformer.Loss import CTCAttentionLoss
    cfg, model, opt, batch = _small()
    head = CTCAttentionLoss(128, 30, ctc_weight=0.3).cuda()
    head._st_prepare("cuda")
    opt.enable_nonfinite_guard()
    opt.enable_averaging(decay=0.9, warmup=False)
    with pytest.raises(ValueError, match="fused capturable"):
        JointTrainStep(model, opt, head, max_grad_norm=5.0, ctc="hip",
                       head_optimizer=torch.optim.Adam(head.parameters(), lr=1e-3, betas=(0.9, 0.98), eps=1e-9, capturable=True))
    hopt = torch.optim.Adam(head.parameters(), lr=1e-3, betas=(0.9, 0.98), eps=1e-9, fused=True, capturable=True)
    step = JointTrainStep(model, opt, head, max_grad_norm=5.0, head_optimizer=hopt, use_graph=True, graph_warmup=1, ctc="hip")
    assert hopt.found_inf.data_ptr() == opt.found_inf.data_ptr()
    params, avgs = step._head_avg
    assert len(params) == len(avgs) == len(list(head.parameters())) and all(torch.equal(q, a) for q, a in zip(params, avgs))
    arena = opt.arena
    w = averaging_weight(0.9, False, 0)
    for it in range(1, 4):                                      # eager, capture + replay, replay
        prev, prev_model = [a.clone() for a in avgs], arena.avg.clone()
        out = step(*batch)
        assert all(bool(torch.isfinite(o)) for o in out) and float(opt._flat_state()[1]["step"]) == float(it)
        for q, a, b in zip(params, avgs, prev):
            _assert_recursion(a.reshape(-1), b.reshape(-1), q.detach().reshape(-1), w, "head, call %d" % it)
        _assert_recursion(arena.avg, prev_model, arena.flat, w, "model, call %d" % it)
    assert len(step.graphs) == 1
    assert all(float((q.detach() - a).abs().max()) > 0 for q, a in zip(params, avgs))
    st = opt._flat_state()[1]
    hstate = [hopt.state[q][k] for q in params for k in ("exp_avg", "exp_avg_sq", "step")]
    watched = [arena.flat, st["exp_avg"], st["exp_avg_sq"], arena.avg, st["step"]] + [q.detach() for q in params] + avgs + hstate
    before = _bits(*watched)
    x = batch[0]
    keep = x[1, 2, 7].clone()
    x[1, 2, 7] = float("inf")
    out = step(*batch)
    assert not bool(torch.isfinite(out[3])) and float(opt.found_inf) == 1.0 and float(opt.skipped) == 1.0
    for i, (a, b) in enumerate(zip(before, _bits(*watched))):
        assert torch.equal(a, b), "buffer %d of the model / the head changed on the skipped step" % i
    x[1, 2, 7] = keep
    prev = [a.clone() for a in avgs]
    out = step(*batch)
    assert all(bool(torch.isfinite(o)) for o in out) and float(st["step"]) == 4.0 and float(opt.skipped) == 1.0
    assert all(float(hopt.state[q]["step"]) == 4.0 for q in params)
    for q, a, b in zip(params, avgs, prev):
        assert not torch.equal(a, b)
        _assert_recursion(a.reshape(-1), b.reshape(-1), q.detach().reshape(-1), w, "head, after the skip")
    # averaged() swaps the head's tensors with the arena
    q_bits, a_bits = _bits(*params), _bits(*avgs)
    with opt.averaged():
        assert all(torch.equal(q.detach().view(torch.int32), a) for q, a in zip(params, a_bits))
        with pytest.raises(RuntimeError, match="averaged"):
            step(*batch)
    assert all(torch.equal(q.detach().view(torch.int32), b) for q, b in zip(params, q_bits))
    assert all(torch.equal(a.view(torch.int32), b) for a, b in zip(avgs, a_bits))
