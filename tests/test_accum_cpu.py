"""-m "not gpu": gradient accumulation - TrainStep(accumulate=K) - on the arena path with emulated kernels (tests/_emul.py,
tests/_emul_ce.py, tests/_emul_optim.py, tests/_emul_accum.py): its entry points in the ABI, the window's gradient against
the fp64 oracle's FULL-batch gradient, the window's bookkeeping, the guard, the untouched defaults, bucket modes and two ranks
over gloo.  The ``run_*`` bodies take a device: tests/test_accum_gpu.py calls them on the hardware.

What "the truth" of a window is.  S = the SUM of the criterion's row losses over all utterances of the window and N = the sum of
their plain NLL (fp64, oracle.transformer on the whole batch at once; rows of padding contribute 0, so neither depends on how
the batch is padded).  The window's loss is S / D, its gradient dS / D, its nll N / D with D = the non-ignored tokens
(nn.CrossEntropyLoss, with or without smoothing) - then S / D is exactly CrossEntropyLoss on the 4 utterances - or, for
transformer.Loss.LabelSmoothingLoss, which divides by EVERY row of the padded, trimmed batch, the rows the micro-batches were
padded to: sum of B_k * l_max_k.  (LabelSmoothingLoss on the 4 utterances as ONE padded batch would divide by 4 * 10 = 40 rows,
the splits below by 3 * 10 + 9 = 39 and 10 + 3 * 9 = 37: its denominator counts padding, so it is a property of how the tokens
were batched.  The window keeps each micro-batch's own padding, as the step's docstring says.)"""
import contextlib
import ctypes
import os
import re
import socket
import subprocess

import pytest
import torch
import torch.nn as nn
import torch.nn.functional as func

import oracle as orc
from st_amd import build, native
from st_amd import native as nv
from tests._emul import emulated_kernels
from tests._emul_accum import emulated_accum
from tests._emul_ce import emulated_ce_smooth
from tests._emul_optim import emulated_optim
from tests.test_composition_cpu import GRAD_TOL_GLOBAL, GRAD_TOL_MEDIAN, GRAD_TOL_TENSOR, _build, _load_c1, rel
from tests.test_label_smoothing_cpu import EPS, make_criterion

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("st_accum_note", "st_grad_norm", "st_adam_clip", "st_window_close")
SPLITS = [[[0, 1, 2], [3]], [[0], [1, 2, 3]]]
KINDS = ["plain", "ce", "ls"]


@contextlib.contextmanager
def emulated():
    with emulated_kernels(), emulated_ce_smooth(), emulated_optim(), emulated_accum():
        yield


def criterion(kind):
    return None if kind == "plain" else make_criterion(kind)


def _cfg(n_warmup_steps=10 ** 9):          # (the default: ~zero learning rate, the weights stay put)
    import transformer.Utils as U
    return U.AttrDict(dict(n_warmup_steps=n_warmup_steps))


def micro(batch, idx, device="cpu"):
    """Utterances ``idx`` of the fixture as a batch of their own (padded to the fixture's width: the step trims)."""
    i = torch.as_tensor(idx)
    return (batch["x"][i].contiguous().to(device), batch["in_len"][i], batch["tokens"][i].contiguous().to(device),
            batch["tgt_len"][i], batch["gt"][i].contiguous().to(device))


# ---- the fp64 truth ------------------------------------------------------------------------------------------------------------
def _sums64(w, batch, kind, idx):
    """fp64, utterances idx as one batch -> (S, N, tokens, rows of the trimmed batch, dS per parameter)."""
    p = {k: v.double() for k, v in w.items()}
    names = [n for n in p if not n.endswith(".pe")]
    leaves = {n: (p[n].clone().requires_grad_(True) if n in names else p[n]) for n in p}
    i = torch.as_tensor(idx)
    in_len, tgt_len = batch["in_len"][i], batch["tgt_len"][i]
    ti, tl = int(in_len.max()), int(tgt_len.max())
    logits, _ = orc.transformer(leaves, batch["x"][i][:, :ti].double(), in_len, batch["tokens"][i][:, :tl], tgt_len, 4)
    gt = batch["gt"][i][:, :tl]
    flat, t = logits.reshape(-1, 30), gt.reshape(-1)
    n_rows, n_tok = t.numel(), int((t != 0).sum())
    if kind == "ls":
        S = orc.label_smoothing_loss(flat, t, EPS, 0) * n_rows
    elif kind == "ce":
        S = func.cross_entropy(flat, t, label_smoothing=EPS, ignore_index=0) * n_tok
    else:
        S = func.cross_entropy(flat, t, ignore_index=0) * n_tok
    N = func.cross_entropy(flat, t, ignore_index=0, reduction="sum")
    grads = torch.autograd.grad(S, [leaves[n] for n in names], allow_unused=True)
    grads = {n: (g if g is not None else torch.zeros_like(p[n])) for n, g in zip(names, grads)}
    return float(S.detach()), float(N.detach()), n_tok, n_rows, grads


def truth_window(w, batch, kind, split):
    """-> the window's truth (module docstring) and the WRONG convention: the mean over micro-batches of each one's own mean."""
    everyone = sorted(u for part in split for u in part)
    S, N, n_tok, _, dS = _sums64(w, batch, kind, everyone)
    parts = [_sums64(w, batch, kind, part) for part in split]
    D = float(sum(q[3] for q in parts)) if kind == "ls" else float(n_tok)
    assert abs(sum(q[0] for q in parts) - S) <= 1e-9 * abs(S) and sum(q[2] for q in parts) == n_tok
    grads = {n: g / D for n, g in dS.items()}
    wrong = {n: sum(q[4][n] / (q[3] if kind == "ls" else q[2]) for q in parts) / len(parts) for n in dS}
    gnorm = float(torch.sqrt(sum((g ** 2).sum() for g in grads.values())))
    return dict(loss=S / D, nll=N / D, denom=D, grads=grads, wrong=wrong, gnorm=gnorm)


def watch_g_eff(step):
    """Record, before every update, the gradient that update consumes: the flat buffer (after the ranks' exchange) over win[0]."""
    from st_amd.arena import arena_of
    box, apply = [], step._apply_window

    def spy():
        box.append((arena_of(step.model).grad.detach().double().cpu() / float(step._win[0]), step._win.detach().cpu().clone()))
        return apply()
    step._apply_window = spy
    return box


def compare_grads(model, g_eff, truth_grads):
    """The three gradient bounds of tests/test_composition_cpu.py; -> the flat (got, truth) pair."""
    from st_amd.arena import arena_of
    arena = arena_of(model)
    bad, rels, flat_g, flat_t = [], [], [], []
    for n, p in model.named_parameters():
        off = arena.offset[id(p)]
        g, t = g_eff[off:off + p.numel()].view(p.shape), truth_grads[n]
        assert torch.isfinite(g).all(), n
        if "linear_k.bias" in n:          # analytically zero (tests/test_label_smoothing_cpu.py)
            assert g.abs().max().item() < 2.5e-1 * truth_grads[n.replace("linear_k", "linear_q")].abs().max().item() + 1e-6
            continue
        rels.append(rel(g, t))
        flat_g.append(g.double().reshape(-1))
        flat_t.append(t.double().reshape(-1))
        if rels[-1] > GRAD_TOL_TENSOR:
            bad.append((n, rels[-1]))
    assert not bad, bad
    assert sorted(rels)[len(rels) // 2] < GRAD_TOL_MEDIAN, sorted(rels)[len(rels) // 2]
    got, want = torch.cat(flat_g), torch.cat(flat_t)
    assert rel(got, want) < GRAD_TOL_GLOBAL, rel(got, want)
    return got, want


def flat_of(model, grads):
    return torch.cat([grads[n].double().reshape(-1) for n, _ in model.named_parameters() if "linear_k.bias" not in n])


# ---- 1. the ABI -----------------------------------------------------------------------------------------------------------------
def test_the_entry_points_are_declared_bound_and_defined():
    """(header == binding == library == sources for EVERY entry point: tests/test_abi_cpu.py.)  The window's norm and update are
    st_grad_norm / st_adam_clip with their last pointer: pinned by position, a window is the LAST argument of both."""
    S = native.SIGNATURES
    assert set(NEW) <= set(S)
    src = open(os.path.join(build.CSRC, "st_optim.hip")).read()
    assert set(NEW) <= set(re.findall(r'extern\s+"C"\s+int\s+(st\w+)\s*\(', src))
    assert len(S["st_adam_clip"]) == 19 and S["st_adam_clip"][1] is ctypes.c_longlong
    assert S["st_adam_clip"][-5:] == [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_float, ctypes.c_int, ctypes.c_void_p]
    assert len(S["st_grad_norm"]) == 9 and S["st_grad_norm"][-2:] == [ctypes.c_void_p, ctypes.c_void_p]


def test_wrappers_check_their_arguments_before_any_launch():
    f, w = torch.zeros(8), torch.zeros(4)
    with pytest.raises(RuntimeError, match="GPU"):
        nv.accum_note(w, None, w.clone(), f[:1])
    with pytest.raises(RuntimeError, match="GPU"):
        nv.window_close(w, w.clone())
    with pytest.raises(RuntimeError, match="GPU"):
        nv.grad_norm_win(f, f, f[0], f[0], None, w)
    with pytest.raises(RuntimeError, match="GPU"):
        nv.adam_clip_win(f, f, f, f, f[0], f[0], None, 1.0, 0.9, 0.98, 1e-9, w)
    with pytest.raises(ValueError, match="win"):
        nv.adam_clip_win(f, f, f, f, f[0], f[0], None, 1.0, 0.9, 0.98, 1e-9, None)
    with pytest.raises(ValueError, match="required"):
        nv.grad_norm_win(f, f, f[0], None, None, w)
    # the backward row chain exists at width 256 only: a 512-wide operand is refused by name, before the chain is looked at
    with pytest.raises(ValueError, match="width 256 only"):
        nv.row_chain_bwd(None, 8, head=(0, None, torch.zeros(8, 512, dtype=torch.bfloat16)) + (None,) * 8)


# ---- 2. a window against the fp64 full-batch truth --------------------------------------------------------------------------
def run_window_vs_oracle(golden_dir, device, split, kind, use_graph):
    from st_amd.trainer import TrainStep
    from transformer.Optim import ScheduledOptim
    _, w, batch = _load_c1(golden_dir)
    truth = truth_window(w, batch, kind, split)
    m = _build(w, device=device)
    opt = ScheduledOptim(m, 128, _cfg())
    step = TrainStep(m, opt, 30, 1e9, use_graph=use_graph, graph_warmup=0, criterion=criterion(kind), accumulate=len(split))
    box = watch_g_eff(step)
    parts = [micro(batch, part, device) for part in split]
    if use_graph:     # lazy set-up (arena, ragged layouts, work lists) must not happen inside the capture
        with torch.no_grad():
            for x, in_len, tok, tgt_len, gt in parts:
                m.forward_packed(x[:, :int(in_len.max())], in_len, tok[:, :int(tgt_len.max())], tgt_len)
    for k, part in enumerate(parts):
        loss, gnorm = step(*part)
        assert step.updated == (k == len(parts) - 1)
        own = _sums64(w, batch, kind, split[k])
        own = own[0] / (own[3] if kind == "ls" else own[2])
        assert abs(float(loss) - own) <= 2e-2 * own, (k, float(loss), own)       # the micro-batch's loss in its own normalisation
    assert len(box) == 1 and step.global_step == 1
    g_eff, win = box[0]
    wl, wn, gn = float(step.window_loss), float(step.window_nll), float(gnorm)
    got, want = compare_grads(m, g_eff, truth["grads"])
    away = rel(got, flat_of(m, truth["wrong"]))
    print("window %s %s graph=%s: loss %.6f (fp64 %.6f) nll %.6f (%.6f) norm %.5f (%.5f) denominator %g; g_eff vs truth %.3e, vs "
          "mean of means %.3e" % (split, kind, use_graph, wl, truth["loss"], wn, truth["nll"], gn, truth["gnorm"], float(win[0]),
                                  rel(got, want), away))
    assert float(win[0]) == truth["denom"] and float(win[3]) == len(split)
    assert abs(wl - truth["loss"]) <= 2e-2 * truth["loss"], (wl, truth["loss"])
    assert abs(wn - truth["nll"]) <= 2e-2 * truth["nll"], (wn, truth["nll"])
    assert abs(gn - truth["gnorm"]) <= 2e-2 * truth["gnorm"], (gn, truth["gnorm"])
    # the wrong convention cannot pass: the fp64 mean of the micro-batches' means lies 0.24 and more from the truth
    assert away >= 5 * GRAD_TOL_GLOBAL, away
    # closed: the buffer is the next window's zero_grad, and the window's state is back at zero
    from st_amd.arena import arena_of
    assert float(arena_of(m).grad.abs().max()) == 0.0 and step._win.tolist() == [0.0] * 4
    return step, parts


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("split", SPLITS)
def test_window_vs_oracle_composition(golden_dir, split, kind):
    with emulated():
        run_window_vs_oracle(golden_dir, "cpu", split, kind, use_graph=False)


def test_the_oracle_alone_tells_the_conventions_apart(golden_dir):
    _, w, batch = _load_c1(golden_dir)
    m = _build(w)
    for split, least in zip(SPLITS, (0.3, 0.2)):
        t = truth_window(w, batch, "plain", split)
        assert rel(flat_of(m, t["wrong"]), flat_of(m, t["grads"])) > least
        # ... and the token-exact window IS the full batch: the micro-batches' sum-loss gradients add up to it
        parts = [_sums64(w, batch, "plain", part)[4] for part in split]
        window = {n: sum(q[n] for q in parts) / t["denom"] for n in t["grads"]}
        exact = rel(flat_of(m, window), flat_of(m, t["grads"]))
        print("split %s: window vs full batch %.1e, mean of means vs full batch %.3f" % (split, exact, rel(flat_of(m, t["wrong"]), flat_of(m, t["grads"]))))
        assert exact < 1e-12


# ---- 3. the window's bookkeeping ---------------------------------------------------------------------------------------------
def test_window_bookkeeping_and_flush(golden_dir):
    from st_amd.trainer import TrainStep
    from transformer.Optim import ScheduledOptim
    _, w, batch = _load_c1(golden_dir)
    with emulated():
        m = _build(w)
        opt = ScheduledOptim(m, 128, _cfg())
        step = TrainStep(m, opt, 30, 1e9, accumulate=3)
        box = watch_g_eff(step)
        assert step.flush() is None and step.global_step == 0 and not box          # nothing accumulated: a no-op
        adam_step = opt._flat_state()[1]["step"]
        seen = []
        for call in range(1, 7):
            step(*micro(batch, [call % 4]))
            seen.append(step.updated)
            assert step.global_step == call // 3 and float(adam_step) == call // 3
            closed = call % 3 == 0
            assert (float(opt.arena.grad.abs().max()) == 0.0) == closed and (step._win.tolist() == [0.0] * 4) == closed
        assert seen == [False, False, True, False, False, True] and len(box) == 2
        assert float(step._win_out[3]) == 3.0
        # a partly filled window: its update consumes that micro-batch's own token-mean gradient (the micro-batch is the whole
        # fixture batch: the three gradient bounds were set for the bf16 noise of exactly that batch)
        step(*micro(batch, [0, 1, 2, 3]))
        assert not step.updated and step._n_acc == 1
        out = step.flush()
        assert out is not None and step.updated and step.global_step == 3 and float(adam_step) == 3.0 and len(box) == 3
        t = truth_window(w, batch, "plain", [[0, 1, 2, 3]])
        compare_grads(m, box[2][0], t["grads"])
        assert float(box[2][1][0]) == t["denom"] == 32.0 and float(step._win_out[3]) == 1.0
        assert abs(float(out[0]) - t["loss"]) <= 2e-2 * t["loss"]
        assert step.flush() is None and step.global_step == 3 and len(box) == 3       # a second flush does nothing
        # after optimizer.load_state_dict a fresh window starts: what was accumulated is dropped
        step(*micro(batch, [1]))
        opt.load_state_dict(opt.state_dict())
        step(*micro(batch, [2]))
        assert step._n_acc == 1 and float(step._win[3]) == 1.0 and float(step._win[0]) == 7.0


# ---- 4. the guard ---------------------------------------------------------------------------------------------------------------
def test_a_poisoned_micro_batch_or_a_window_without_tokens_skips_the_whole_window(golden_dir):
    from st_amd.trainer import TrainStep
    from transformer.Optim import ScheduledOptim
    _, w, batch = _load_c1(golden_dir)
    with emulated():
        m = _build(w)
        opt = ScheduledOptim(m, 128, _cfg(n_warmup_steps=100))
        opt.enable_nonfinite_guard()
        opt.enable_averaging(decay=0.9, warmup=False)
        step = TrainStep(m, opt, 30, 5.0, accumulate=2)
        step(*micro(batch, [0, 1]))
        step(*micro(batch, [2, 3]))
        flat, st = opt._flat_state()
        assert step.updated and float(st["step"]) == 1.0 and float(opt.skipped) == 0.0
        watched = (flat, st["exp_avg"], st["exp_avg_sq"], st["step"], opt.arena.avg)

        def bits():
            return [t.detach().clone().view(torch.int32) for t in watched]

        def no_tokens(part):
            x, in_len, tok, tgt_len, gt = part
            return x, in_len, tok, tgt_len, torch.zeros_like(gt)

        poisoned = list(micro(batch, [2, 3]))
        poisoned[0] = poisoned[0].clone()
        poisoned[0][0, 3, 5] = float("nan")
        windows = [(micro(batch, [0, 1]), tuple(poisoned)), (no_tokens(micro(batch, [0, 1])), no_tokens(micro(batch, [2, 3])))]
        for skipped, (a, b) in enumerate(windows, start=1):
            before = bits()
            step(*a)
            step(*b)
            assert step.updated and step.global_step == 1 + skipped
            assert all(torch.equal(x, y) for x, y in zip(before, bits())), "window %d moved the state" % skipped
            assert float(opt.found_inf) == 1.0 and float(opt.skipped) == float(skipped)
            assert float(opt.arena.grad.abs().max()) == 0.0 and step._win.tolist() == [0.0] * 4       # cleared for the next window
        before = bits()
        step(*micro(batch, [0, 1]))
        _, gnorm = step(*micro(batch, [2, 3]))
        assert bool(torch.isfinite(gnorm)) and float(opt.found_inf) == 0.0 and float(opt.skipped) == 2.0
        assert float(st["step"]) == 2.0 and not torch.equal(before[0], bits()[0]) and not torch.equal(before[4], bits()[4])
        assert bool(torch.isfinite(flat).all()) and bool(torch.isfinite(opt.arena.avg).all())


# ---- 5. the defaults are untouched --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("accumulate", [None, 1])
def test_without_accumulation_the_new_wrappers_are_never_called(golden_dir, monkeypatch, accumulate):
    from st_amd.trainer import TrainStep
    from transformer.Optim import ScheduledOptim
    _, w, batch = _load_c1(golden_dir)
    with emulated(), monkeypatch.context() as mp:
        calls = []
        for name in ("grad_norm", "adam_clip", "ce_fwd", "ce_smooth_fwd", "accum_note", "window_close", "grad_norm_win", "adam_clip_win"):
            def rec(*a, _f=getattr(nv, name), _n=name, **k):
                calls.append(_n)
                return _f(*a, **k)
            mp.setattr(nv, name, rec)
        m = _build(w)
        opt = ScheduledOptim(m, 128, _cfg())
        step = TrainStep(m, opt, 30, 5.0, accumulate=accumulate)
        assert step.accumulate is None
        for _ in range(2):
            step(*micro(batch, [0, 1, 2, 3]))
        assert calls == ["ce_fwd", "grad_norm", "adam_clip"] * 2 and step.global_step == 2 and step.flush() is None
        assert float(opt.arena.grad.abs().max()) > 0          # (the clipped gradient stays in the buffer, as before)


def test_refusals(golden_dir):
    from st_amd.trainer import JointTrainStep, TrainStep
    from transformer.Optim import ScheduledOptim
    _, w, _ = _load_c1(golden_dir)

    class Padded(nn.Module):          # a model without forward_packed
        def __init__(self):
            super().__init__()
            self.lin = nn.Linear(4, 4)

    plain = Padded()
    with pytest.raises(ValueError, match="forward_packed"):
        TrainStep(plain, ScheduledOptim(plain, 4, _cfg()), 30, 5.0, accumulate=2)
    off_arena = _build(w)
    with pytest.raises(ValueError, match="flat arena"):
        TrainStep(off_arena, ScheduledOptim(off_arena, 128, _cfg()), 30, 5.0, accumulate=2)
    with emulated():
        m = _build(w)
        opt = ScheduledOptim(m, 128, _cfg())
        for bad in (0, -2, 2.5, True):
            with pytest.raises(ValueError, match="accumulate"):
                TrainStep(m, opt, 30, 5.0, accumulate=bad)
        with pytest.raises(TypeError):
            JointTrainStep(m, opt, None, max_grad_norm=5.0, accumulate=2)
        with pytest.raises(ValueError, match="window"):
            opt.step_captured(grad_norm=torch.tensor(1.0), max_norm=5.0, window=torch.zeros(4))
        # the options token still guards a captured step
        from st_amd.trainer import _Captured
        step = TrainStep(m, opt, 30, 5.0, use_graph=True, accumulate=2)
        cap = _Captured()
        cap.options = step._options()
        opt.enable_nonfinite_guard()
        with pytest.raises(RuntimeError, match="options changed"):
            step._replay(cap)


# ---- 6. bucket modes ----------------------------------------------------------------------------------------------------------
def run_accum_bucket_mode(device, use_graph, bucket_rows=None, T_cap=96, L_cap=12):
    """Two windows of two micro-batches whose lengths differ, through ONE bucket (one micro-batch capture in graph mode), against
    the eager accumulating step on a twin with the same weights: loss, nll, the window's results and g_eff within 2e-3."""
    import copy
    import transformer.Models as M
    import transformer.Utils as U
    from st_amd.trainer import TrainStep
    from transformer.Optim import ScheduledOptim
    torch.manual_seed(5)
    cfg = U.AttrDict(dict(feature_dim=80, max_inputs_length=T_cap, max_target_length=L_cap, num_enc_layer=2, num_dec_layer=2,
                          n_heads=4, d_k=64, d_v=64, d_model=256, d_inner_hid=512, dropout=0.0, vocab_size=30))
    ma = M.Transformer(cfg)
    U.init_parameters(ma)
    mb = copy.deepcopy(ma)
    ma, mb = ma.eval().to(device), mb.eval().to(device)
    oa, ob = ScheduledOptim(ma, 256, _cfg()), ScheduledOptim(mb, 256, _cfg())
    sa = TrainStep(ma, oa, 30, 1e9, use_graph=use_graph, graph_warmup=1, bucket=(T_cap, L_cap), bucket_rows=bucket_rows, accumulate=2)
    sb = TrainStep(mb, ob, 30, 1e9, use_graph=False, accumulate=2)
    ba, bb = watch_g_eff(sa), watch_g_eff(sb)
    caps = []
    for i, l_max in enumerate((L_cap, L_cap - 3, L_cap - 5, L_cap - 2)):      # (the first call is the eager warm-up)
        b = orc.synthetic_batch(4, 80, l_max, 80, 30, seed=60 + i, t_min=40, l_min=4)
        T, L = int(b["in_len"].max()), int(b["tgt_len"].max())
        x, tok, gt = b["x"][:, :T].to(device), b["tokens"][:, :L].to(device), b["gt"][:, :L].to(device)
        la, _ = sa(x, b["in_len"], tok, b["tgt_len"], gt)
        lb, _ = sb(x, b["in_len"], tok, b["tgt_len"], gt)
        la, lb, na, nb = float(la), float(lb), float(sa.nll), float(sb.nll)
        print("accumulating bucket %s graph=%s micro-batch %d: loss %.6f (eager %.6f) nll %.6f (%.6f)" % (bucket_rows, use_graph, i, la, lb, na, nb))
        assert abs(la - lb) <= 2e-3 * abs(lb), (i, la, lb)
        assert abs(na - nb) <= 2e-3 * abs(nb), (i, na, nb)
        assert sa.updated == sb.updated == (i % 2 == 1)
        caps.append(sa._g_fb if use_graph and i else None)
        if sa.updated:
            (ga, wa), (gb, wb) = ba[-1], bb[-1]
            assert float(wa[0]) == float(wb[0]) > 0 and float(wa[3]) == 2.0
            assert rel(ga, gb) <= 2e-3, (i, rel(ga, gb))
            for got, want in ((sa.window_loss, sb.window_loss), (sa.window_nll, sb.window_nll)):
                assert abs(float(got) - float(want)) <= 2e-3 * abs(float(want)), (i, float(got), float(want))
            assert float(oa.arena.grad.abs().max()) == 0.0
    assert len(ba) == len(bb) == 2 and len(sa._buckets) == 1
    if use_graph:
        assert caps[1] is not None and caps[1] is caps[2] is caps[3], "one capture serves every micro-batch"


@pytest.mark.parametrize("bucket_rows", [None, (340, 48)])
def test_accum_bucket_mode_composition(bucket_rows):
    with emulated():
        run_accum_bucket_mode("cpu", use_graph=False, bucket_rows=bucket_rows)


# ---- 7. two ranks over gloo ----------------------------------------------------------------------------------------------------
def _free_port():
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


def _dp_worker(rank, world, port, out_q):
    import sys
    import torch.distributed as dist
    here = ROOT
    for p in (here, os.path.join(here, "speech-tranformer-pytorch_amd")):
        if p not in sys.path:
            sys.path.insert(0, p)
    from st_amd import dp
    from st_amd.arena import arena_of
    from st_amd.trainer import TrainStep
    from transformer.Optim import ScheduledOptim
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), LOCAL_RANK=str(rank), WORLD_SIZE=str(world))
    dp.init_from_env(backend="gloo")
    _, w, batch = _load_c1(os.path.join(here, "tests", "golden"))
    if rank != 0:
        w = {k: (v if k.endswith(".pe") else torch.randn_like(v)) for k, v in w.items()}
    with emulated():
        m = _build(w)
        arena = arena_of(m)
        dp.broadcast_parameters(arena)
        red = dp.GradReducer(arena, bucket_bytes=64 << 10)
        fired = []
        fire = red._fire
        red._fire = lambda i: (fired.append(i), fire(i))[1]
        import transformer.Utils as U
        opt = ScheduledOptim(m, 128, U.AttrDict(n_warmup_steps=100))
        step = TrainStep(m, opt, 30, 1e9, reducer=red, accumulate=2)
        box = watch_g_eff(step)
        step(*micro(batch, [2 * rank]))
        before_update = len(fired)                      # no collective on a non-final micro-batch
        step(*micro(batch, [2 * rank + 1]))
        g_eff, win = box[0]
        flat = arena.flat.detach().clone()
    gathered = [torch.zeros_like(flat) for _ in range(world)]
    dist.all_gather(gathered, flat)
    same = all(torch.equal(gathered[0], g) for g in gathered)
    if rank == 0:
        out_q.put((g_eff.numpy().copy(), win.numpy().copy(), before_update, len(fired), len(red.buckets), same,
                   float(step.window_loss), float(step._gnorm)))
    dist.barrier()
    dist.destroy_process_group()


def test_two_ranks_accumulate_the_token_mean_over_all_ranks(golden_dir):
    import torch.multiprocessing as mp
    world, port = 2, _free_port()
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    procs = [ctx.Process(target=_dp_worker, args=(r, world, port, q)) for r in range(world)]
    for p in procs:
        p.start()
    g_eff, win, before_update, fired, n_buckets, same, wloss, gnorm = q.get(timeout=300)
    for p in procs:
        p.join(timeout=60)
        assert p.exitcode == 0
    assert same, "the ranks hold different parameters after the update"
    assert before_update == 0 and fired == n_buckets
    _, w, batch = _load_c1(golden_dir)
    truth = truth_window(w, batch, "plain", [[0], [1], [2], [3]])
    assert float(win[0]) == truth["denom"] == 32.0 and float(win[3]) == 2.0       # (micro-batches are counted per rank)
    with emulated_kernels():          # (the arena's layout of the parameters: offsets only)
        compare_grads(_build(w), torch.from_numpy(g_eff), truth["grads"])
    assert abs(wloss - truth["loss"]) <= 2e-2 * truth["loss"] and abs(gnorm - truth["gnorm"]) <= 2e-2 * truth["gnorm"]


# ---- 8. the garbage collector stays out of a capture ------------------------------------------------------------------------------
def test_no_garbage_collection_inside_a_capture():
    """trainer.no_gc_inside_capture (around every capture of TrainStep / JointTrainStep): dead cycles are collected BEFORE the
    capture begins, no generational pass can fire inside it, and the collector's state is what it was afterwards - also when
    the capture raises, and also when it was off to begin with."""
    import gc
    import weakref
    from st_amd.trainer import no_gc_inside_capture

    class Node:
        pass

    a, b = Node(), Node()
    a.other, b.other = b, a                       # a dead cycle, as a discarded step object leaves behind
    alive = weakref.ref(a)
    del a, b
    assert gc.isenabled()
    with no_gc_inside_capture():
        assert alive() is None and not gc.isenabled()
    assert gc.isenabled()
    with pytest.raises(RuntimeError):
        with no_gc_inside_capture():
            raise RuntimeError("the capture failed")
    assert gc.isenabled()
    gc.disable()
    try:
        with no_gc_inside_capture():
            assert not gc.isenabled()
        assert not gc.isenabled()
    finally:
        gc.enable()
