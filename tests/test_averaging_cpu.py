"""-m "not gpu": the host side of the optimizer options - ScheduledOptim.enable_nonfinite_guard / enable_averaging / averaged(),
their checkpoint key, and the step drivers' refusals - on the arena path with emulated kernels (tests/_emul.py,
tests/_emul_optim.py).  Kernel arithmetic is pinned on hardware by tests/test_averaging_gpu.py."""
import copy

import pytest
import torch

from st_amd import native as nv
from tests._emul import emulated_kernels
from tests._emul_optim import averaging_weight, emulated_optim
from tests.test_composition_cpu import _build, _load_c1


def _cfg(**kw):
    import transformer.Utils as U
    return U.AttrDict(dict(n_warmup_steps=100, **kw))


def _fill_grad(opt, seed, poison=None):
    flat = opt._flat_state()[0]
    flat.grad.copy_(torch.randn(flat.shape, generator=torch.Generator().manual_seed(seed)))
    if poison is not None:
        flat.grad[7] = poison
    return flat


def _bits(*tensors):
    return [t.detach().clone().view(torch.int32) for t in tensors]


def _same(a, b):
    return all(torch.equal(x, y) for x, y in zip(a, b))


@pytest.fixture()
def c1(golden_dir):
    return _load_c1(golden_dir)


def test_nothing_enabled_calls_the_old_wrappers_only(c1, monkeypatch):
    from transformer.Optim import ScheduledOptim
    _, w, _ = c1
    with emulated_kernels(), emulated_optim(), monkeypatch.context() as mp:      # (undone before the emulations are)
        calls = []
        for name in ("grad_norm", "adam_clip", "grad_norm_guard", "adam_clip_avg", "swap_"):
            def rec(*a, _f=getattr(nv, name), _n=name, **k):
                calls.append(_n)
                return _f(*a, **k)
            mp.setattr(nv, name, rec)
        opt = ScheduledOptim(_build(w), 128, _cfg())
        assert opt.found_inf is None and opt.skipped is None and opt.arena.avg is None
        opt.update_learning_rate(1)
        _fill_grad(opt, 1)
        opt.step_captured(grad_norm=True, max_norm=5.0)
        assert calls == ["grad_norm", "adam_clip"]
        _fill_grad(opt, 2)
        opt.step_captured(grad_norm=torch.tensor(3.0), max_norm=5.0)
        assert calls == ["grad_norm", "adam_clip", "adam_clip"]
        assert float(opt._flat_state()[1]["step"]) == 2.0
        assert set(opt.state_dict()) == {"state", "param_groups"}
        # a config that carries the keys builds the options
        opt2 = ScheduledOptim(_build(w), 128, _cfg(skip_nonfinite=True, ema_decay=0.9, ema_warmup=False))
        assert opt2.found_inf is not None and opt2._avg_opts == (0.9, False) and opt2.arena.avg is not None
        del calls[:]
        opt2.update_learning_rate(1)
        _fill_grad(opt2, 1)
        opt2.step_captured(grad_norm=True, max_norm=5.0)
        assert calls == ["grad_norm_guard", "adam_clip_avg"]


@pytest.mark.parametrize("norm_given", [False, True])
@pytest.mark.parametrize("poison", [float("nan"), float("inf"), float("-inf")])
def test_a_non_finite_gradient_skips_the_step_and_the_next_clean_one_applies(c1, poison, norm_given):
    from transformer.Optim import ScheduledOptim
    _, w, _ = c1
    with emulated_kernels(), emulated_optim():
        opt = ScheduledOptim(_build(w), 128, _cfg())
        opt.enable_nonfinite_guard()
        opt.enable_averaging(decay=0.9, warmup=True)
        opt.update_learning_rate(1)

        def step(flat):
            gn = torch.linalg.vector_norm(flat.grad) if norm_given else True
            return opt.step_captured(grad_norm=gn, max_norm=5.0)

        step(_fill_grad(opt, 1))
        flat, st = opt._flat_state()
        assert float(st["step"]) == 1.0 and float(opt.found_inf) == 0.0 and float(opt.skipped) == 0.0
        assert not torch.equal(opt.arena.avg, flat.detach()) and float((opt.arena.avg - flat.detach()).abs().max()) > 0
        _fill_grad(opt, 2, poison=poison)
        watched = (flat, st["exp_avg"], st["exp_avg_sq"], opt.arena.avg, st["step"], flat.grad)
        before = _bits(*watched)
        gn = step(flat)
        assert not bool(torch.isfinite(gn))
        assert _same(before, _bits(*watched))
        assert float(opt.found_inf) == 1.0 and float(opt.skipped) == 1.0
        step(_fill_grad(opt, 3))
        assert float(st["step"]) == 2.0 and float(opt.found_inf) == 0.0 and float(opt.skipped) == 1.0
        assert not torch.equal(before[0], flat.detach().view(torch.int32))
        assert bool(torch.isfinite(flat).all()) and bool(torch.isfinite(opt.arena.avg).all())


def test_the_average_follows_the_recursion_and_step_routes_through_it(c1):
    from transformer.Optim import ScheduledOptim
    _, w, _ = c1
    with emulated_kernels(), emulated_optim():
        m = _build(w)
        opt = ScheduledOptim(m, 128, _cfg())
        opt.enable_averaging(decay=0.99, warmup=True)
        want = opt.arena.flat.detach().clone().double()
        assert torch.equal(opt.arena.avg, opt.arena.flat) and opt.arena.avg.data_ptr() != opt.arena.flat.data_ptr()
        for s in (1, 2, 3):
            _fill_grad(opt, s)
            opt.step(s)                                        # train.py:46's entry point keeps the average too
            wgt = float(averaging_weight(0.99, True, s))
            assert abs(wgt - (1.0 - min(0.99, (1.0 + s) / (10.0 + s)))) < 1e-6
            want += wgt * (opt.arena.flat.detach().double() - want)
            assert float((opt.arena.avg.double() - want).abs().max()) < 1e-6
        assert float(opt._flat_state()[1]["step"]) == 3.0


def test_averaged_swaps_and_restores_and_refuses_nesting_and_training(c1):
    from st_amd.trainer import TrainStep
    from transformer.Optim import ScheduledOptim
    _, w, batch = c1
    with emulated_kernels(), emulated_optim():
        m = _build(w)
        opt = ScheduledOptim(m, 128, _cfg())
        with pytest.raises(RuntimeError, match="not enabled"):
            with opt.averaged():
                pass
        opt.enable_averaging(decay=0.5, warmup=False)
        opt.update_learning_rate(1)
        _fill_grad(opt, 1)
        opt.step_captured(grad_norm=True, max_norm=5.0)
        arena = opt.arena
        flat0, avg0 = _bits(arena.flat)[0], _bits(arena.avg)[0]
        assert not torch.equal(flat0, avg0)
        p0 = next(m.parameters())
        step = TrainStep(m, opt, 30, 5.0, use_graph=False)
        with opt.averaged():
            assert torch.equal(arena.flat.view(torch.int32), avg0) and torch.equal(arena.avg.view(torch.int32), flat0)
            assert torch.equal(p0.detach().view(torch.int32).reshape(-1), avg0[:p0.numel()])      # the model's views see it
            with pytest.raises(RuntimeError, match="already inside"):
                with opt.averaged():
                    pass
            with pytest.raises(RuntimeError, match="averaged"):
                step(batch["x"], batch["in_len"], batch["tokens"], batch["tgt_len"], batch["gt"])
            with pytest.raises(RuntimeError, match="averaged"):
                opt.step_captured(grad_norm=True, max_norm=5.0)
            assert step.global_step == 0
        assert torch.equal(arena.flat.view(torch.int32), flat0) and torch.equal(arena.avg.view(torch.int32), avg0)
        # an exception inside still restores
        with pytest.raises(KeyError):
            with opt.averaged():
                raise KeyError("x")
        assert torch.equal(arena.flat.view(torch.int32), flat0) and not opt._in_averaged
        # and outside the context the step trains
        loss, gnorm = step(batch["x"], batch["in_len"], batch["tokens"], batch["tgt_len"], batch["gt"])
        assert bool(torch.isfinite(loss)) and bool(torch.isfinite(gnorm)) and float(opt._flat_state()[1]["step"]) == 2.0


def test_state_dict_round_trips_with_and_without_the_extra_key(c1):
    from transformer.Optim import ScheduledOptim
    _, w, _ = c1
    with emulated_kernels(), emulated_optim():
        m, m_ref = _build(w), _build(w)
        opt, ref = ScheduledOptim(m, 128, _cfg()), ScheduledOptim(m_ref, 128, _cfg())
        opt.enable_nonfinite_guard()
        opt.enable_averaging(decay=0.9, warmup=False)
        for o in (opt, ref):
            o.update_learning_rate(1)
        for s in (1, 2):
            for o in (opt, ref):
                _fill_grad(o, s)
                o.step_captured(grad_norm=True, max_norm=5.0)
        _fill_grad(opt, 3, poison=float("nan"))
        opt.step_captured(grad_norm=True, max_norm=5.0)
        sd, sd_ref = opt.state_dict(), ref.state_dict()
        # the reference-format entries are those of the optimizer with nothing enabled
        assert set(sd) == {"state", "param_groups", "averaging"} and set(sd_ref) == {"state", "param_groups"}
        assert sd["param_groups"] == sd_ref["param_groups"] and sd["state"].keys() == sd_ref["state"].keys()
        for i in sd["state"]:
            for k in ("step", "exp_avg", "exp_avg_sq"):
                assert torch.equal(sd["state"][i][k], sd_ref["state"][i][k]), (i, k)
        extra, params = sd["averaging"], list(m.parameters())
        assert extra["decay"] == 0.9 and extra["warmup"] is False and extra["skipped"] == 1.0
        assert len(extra["avg"]) == len(params) and all(a.shape == p.shape for a, p in zip(extra["avg"], params))
        assert torch.equal(extra["avg"][3], opt.arena.avg_view(params[3]))
        # with the key
        m2 = _build({k: v.detach().clone() for k, v in m.state_dict().items()})
        opt2 = ScheduledOptim(m2, 128, _cfg(skip_nonfinite=True, ema_decay=0.9, ema_warmup=False))
        opt2.load_state_dict(copy.deepcopy(sd))
        # (per parameter: _fill_grad also moved the alignment gaps between the slots, which no checkpoint carries)
        assert all(torch.equal(opt2.arena.avg_view(q), opt.arena.avg_view(p)) for q, p in zip(m2.parameters(), params))
        assert float(opt2.skipped) == 1.0 and float(opt2.found_inf) == 0.0
        assert float(opt2._flat_state()[1]["step"]) == 2.0
        # without it: the average is re-seeded from the parameters
        opt3 = ScheduledOptim(_build({k: v.detach().clone() for k, v in m.state_dict().items()}), 128, _cfg(ema_decay=0.9))
        opt3.arena.avg.zero_()
        opt3.load_state_dict(copy.deepcopy(sd_ref))
        assert torch.equal(opt3.arena.avg, opt3.arena.flat)
        # a checkpoint WITH the key loads into an optimizer with nothing enabled, and a plain per-parameter Adam takes its entries
        plain = ScheduledOptim(_build(w), 128, _cfg())
        plain.load_state_dict(copy.deepcopy(sd))
        assert set(plain.state_dict()) == {"state", "param_groups"}
        adam = torch.optim.Adam([torch.nn.Parameter(p.detach().clone()) for p in params], lr=0.0, betas=(0.9, 0.98), eps=1e-9)
        adam.load_state_dict({k: copy.deepcopy(sd[k]) for k in ("state", "param_groups")})
        with pytest.raises(ValueError, match="averaged tensors"):
            bad = copy.deepcopy(sd)
            bad["averaging"]["avg"] = bad["averaging"]["avg"][:-1]
            opt2.load_state_dict(bad)


def test_every_listed_error_is_raised(c1):
    from st_amd.trainer import JointTrainStep, TrainStep, _Captured
    from transformer.Loss import CTCAttentionLoss
    from transformer.Optim import ScheduledOptim
    _, w, batch = c1
    off_arena = ScheduledOptim(_build(w), 128, _cfg())            # CPU tensors, no emulation: the per-tensor path
    assert off_arena.arena is None
    with pytest.raises(ValueError, match="flat-arena"):
        off_arena.enable_nonfinite_guard()
    with pytest.raises(ValueError, match="flat-arena"):
        off_arena.enable_averaging()
    with pytest.raises(ValueError, match="flat-arena"):
        ScheduledOptim(_build(w), 128, _cfg(skip_nonfinite=True))
    with emulated_kernels(), emulated_optim():
        for key in ("weight_decay", "amsgrad", "maximize"):
            opt = ScheduledOptim(_build(w), 128, _cfg())
            opt.optimizer.param_groups[0][key] = 1e-2 if key == "weight_decay" else True
            with pytest.raises(ValueError, match="weight decay"):
                opt.enable_nonfinite_guard()
            with pytest.raises(ValueError, match="weight decay"):
                opt.enable_averaging()
        m = _build(w)
        opt = ScheduledOptim(m, 128, _cfg())
        for decay in (-0.1, 1.5, float("nan")):
            with pytest.raises(ValueError, match="decay"):
                opt.enable_averaging(decay=decay)
        assert opt.arena.avg is None and opt._avg_opts is None
        with pytest.raises(ValueError, match="not enabled"):
            opt.register_averaged([])
        opt.enable_nonfinite_guard()
        opt.update_learning_rate(1)
        _fill_grad(opt, 1)
        with pytest.raises(ValueError, match="needs a norm"):
            opt.step_captured()
        with pytest.raises(ValueError, match="needs a norm"):
            opt.step_captured(grad_norm=None, max_norm=5.0)
        opt.optimizer.param_groups[0]["weight_decay"] = 1e-2        # switched on behind the guard's back
        with pytest.raises(ValueError, match="HIP update only"):
            opt.step_captured(grad_norm=True, max_norm=5.0)
        opt.optimizer.param_groups[0]["weight_decay"] = 0

        # a captured step holds the options it was captured with
        opt = ScheduledOptim(m, 128, _cfg())
        step = TrainStep(m, opt, 30, 5.0, use_graph=True)
        cap = _Captured()
        cap.options = step._options()
        opt.enable_nonfinite_guard()
        with pytest.raises(RuntimeError, match="options changed"):
            step._replay(cap)
        cap.options = step._options()
        opt.enable_averaging()
        with pytest.raises(RuntimeError, match="options changed"):
            step._replay(cap)

        # the joint step: the head's optimizer must be able to skip on a device scalar
        head = CTCAttentionLoss(128, 30, ctc_weight=0.3)
        for kw in (dict(), dict(capturable=True), dict(foreach=True)):
            hopt = torch.optim.Adam(head.parameters(), lr=1e-3, **kw)
            with pytest.raises(ValueError, match="fused capturable"):
                JointTrainStep(m, opt, head, max_grad_norm=5.0, head_optimizer=hopt, use_graph=False, ctc="hip")
        plain = ScheduledOptim(_build(w), 128, _cfg())
        hopt = torch.optim.Adam(head.parameters(), lr=1e-3)
        joint = JointTrainStep(plain.arena.root, plain, head, max_grad_norm=5.0, head_optimizer=hopt, use_graph=False, ctc="hip")
        assert not hasattr(hopt, "found_inf") and joint._head_avg is None      # nothing enabled: nothing touched
        plain.enable_nonfinite_guard()
        with pytest.raises(ValueError, match="fused capturable"):
            joint(batch["x"], batch["in_len"], batch["tokens"], batch["tgt_len"], batch["gt"])


def test_wrappers_check_their_arguments_before_any_launch():
    f = torch.zeros(8)
    with pytest.raises(RuntimeError, match="GPU"):
        nv.grad_norm_guard(f, f, f[0], f[0], f[:2])
    with pytest.raises(RuntimeError, match="GPU"):
        nv.adam_clip_avg(f, f, f, f, f[0], f[0], None, 1.0, 0.9, 0.98, 1e-9)
    with pytest.raises(RuntimeError, match="GPU"):
        nv.swap_(f, f.clone())
