"""-m "not gpu": the definition the HIP CTC loss (csrc/st_ctc_loss.hip) is held to, and the host side around it.

The fp64 truth of tests/_ctc_loss_ref.py is checked against ``torch.nn.functional.ctc_loss`` where the two definitions coincide
(labels >= 1) and against autograd of an independent forward-only restatement everywhere (labels equal to the blank id
included: there torch's CPU gradient is NOT the derivative of its own value at the last frame - see
test_truth_value_with_blank_id_labels); then the exports, the binding's argument checks and, under the kernel emulations, the
wiring of CTCAttentionLoss.ctc_rows(impl="hip") and JointTrainStep(ctc="hip")."""
import os
import re
import subprocess

import numpy as np
import pytest
import torch
import torch.nn.functional as func

from st_amd import native
from tests import _ctc_loss_ref as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _case(rng, lo, B=4, allow_tl0=True, feasible=False):
    """A random ragged batch: log-probabilities [B, T, C] (fp64), classes in [lo, C) with forced repeats, lengths."""
    T, L, C = int(rng.integers(1, 15)), int(rng.integers(1, 7)), int(rng.integers(3, 7))
    g = torch.Generator().manual_seed(int(rng.integers(1 << 30)))
    lp = torch.log_softmax(torch.randn(B, T, C, dtype=torch.float64, generator=g) * 2, -1)
    cls = torch.randint(lo, C, (B, L), generator=g)
    if L > 1:
        cls[0, 1] = cls[0, 0]                                   # an adjacent repeat in every case
    il = torch.randint(1, T + 1, (B,), generator=g)
    tl = torch.randint(0 if allow_tl0 else 1, L + 1, (B,), generator=g)
    if feasible:
        rep = torch.tensor([sum(int(cls[b, j] == cls[b, j - 1]) for j in range(1, int(tl[b]))) for b in range(B)])
        tl = torch.where(tl + rep <= T, tl, torch.zeros_like(tl))
        rep = torch.where(tl > 0, rep, torch.zeros_like(rep))
        il = torch.maximum(il, tl + rep)
    return lp, cls, il, tl


def _torch_ctc(lp, cls, il, tl):
    leaf = lp.clone().requires_grad_(True)
    nll = func.ctc_loss(leaf.transpose(0, 1), cls, il, tl, blank=0, reduction="none", zero_infinity=True)
    (g,) = torch.autograd.grad(nll.sum(), leaf)
    return nll.detach().numpy(), g.numpy()


def test_truth_matches_torch_ctc_loss_where_the_definitions_coincide():
    """Labels >= 1 (tl = 0 and repeated labels included): value and gradient of torch's fp64 CPU ctc_loss.  torch's gradient with
    respect to its log_probs argument is exp(lp) - occ: the convention of ``g`` with coef = 1."""
    rng = np.random.default_rng(0)
    worst_n = worst_g = 0.0
    seen_tl0 = seen_inf = False
    for _ in range(60):
        lp, cls, il, tl = _case(rng, lo=1)
        out = ref.alpha_beta(lp.numpy(), cls.numpy(), il.numpy(), tl.numpy())
        nll_t, g_t = _torch_ctc(lp, cls, il, tl)
        seen_tl0 |= bool((tl == 0).any())
        for b in range(lp.shape[0]):
            if not np.isfinite(out["nll"][b]):
                seen_inf = True
                assert nll_t[b] == 0.0 and np.abs(g_t[b]).max() == 0.0 and np.abs(out["g"][b]).max() == 0.0
                continue
            worst_n = max(worst_n, abs(out["nll"][b] - nll_t[b]))
            worst_g = max(worst_g, np.abs(out["g"][b] - g_t[b]).max())
    assert seen_tl0 and seen_inf
    assert worst_n < 1e-12 and worst_g < 1e-12, (worst_n, worst_g)


def test_truth_value_with_blank_id_labels():
    """Labels may equal the blank id: the VALUE still agrees with torch (an ordinary label state that emits column 0).  torch's
    CPU gradient is not compared: at the last frame of an utterance whose last label is the blank id it assigns the two
    final-state terms instead of accumulating them, and its row there no longer sums to zero."""
    rng = np.random.default_rng(1)
    worst, n_blank = 0.0, 0
    for _ in range(60):
        lp, cls, il, tl = _case(rng, lo=0)
        cls[1, :] = 0                                          # one utterance of blank-id labels only
        out = ref.alpha_beta(lp.numpy(), cls.numpy(), il.numpy(), tl.numpy())
        nll_t, _ = _torch_ctc(lp, cls, il, tl)
        for b in range(lp.shape[0]):
            if np.isfinite(out["nll"][b]):
                worst = max(worst, abs(out["nll"][b] - nll_t[b]))
                n_blank += int((cls[b, :int(tl[b])] == 0).any())
            else:
                assert nll_t[b] == 0.0
    assert n_blank > 20 and worst < 1e-12, (n_blank, worst)


def test_truth_gradient_is_the_derivative_of_the_forward_and_occupancies_are_distributions():
    """alpha-beta against autograd through the forward-only restatement (d nll / d lp = -occ), blank-id labels, tl = 0 and
    infeasible utterances included; every live frame's occupancies sum to 1; a row of g sums to sum_k exp(lp) - 1 = 0."""
    rng = np.random.default_rng(2)
    worst = worst_n = worst_row = 0.0
    for i in range(40):
        lp, cls, il, tl = _case(rng, lo=0, feasible=(i % 2 == 0))
        out = ref.alpha_beta(lp.numpy(), cls.numpy(), il.numpy(), tl.numpy())
        leaf = lp.clone().requires_grad_(True)
        n = ref.nll_torch(leaf, cls, il, tl)
        inf = ref.is_inf(n)
        (d,) = torch.autograd.grad(torch.where(inf, torch.zeros_like(n), n).sum(), leaf)
        assert np.array_equal(inf.numpy(), ~np.isfinite(out["nll"]))
        fin = ~inf.numpy()
        worst_n = max(worst_n, np.abs(out["nll"][fin] - n.detach().numpy()[fin]).max() if fin.any() else 0.0)
        worst = max(worst, np.abs(-out["occ"] - d.numpy()).max())
        for b in range(lp.shape[0]):
            T = int(il[b])
            rows = out["occ"][b].sum(1)
            if fin[b]:
                worst_row = max(worst_row, np.abs(rows[:T] - 1.0).max(), np.abs(out["g"][b, :T].sum(1)).max())
            else:
                assert np.abs(out["occ"][b]).max() == 0.0
            assert np.abs(out["occ"][b, T:]).max(initial=0.0) == 0.0 and np.abs(out["g"][b, T:]).max(initial=0.0) == 0.0
    assert worst < 1e-12 and worst_n < 1e-12 and worst_row < 1e-12, (worst, worst_n, worst_row)
    # no label slots at all (L = 0): the single blank state - nll = -sum of the blank column
    lp = torch.log_softmax(torch.randn(3, 5, 2, dtype=torch.float64), -1)
    il, tl, cls = torch.tensor([5, 3, 1]), torch.zeros(3, dtype=torch.int64), torch.zeros(3, 0, dtype=torch.int64)
    out = ref.alpha_beta(lp.numpy(), cls.numpy(), il.numpy(), tl.numpy())
    want = np.array([-lp[b, :int(il[b]), 0].sum().item() for b in range(3)])
    assert np.abs(out["nll"] - want).max() < 1e-12 and np.abs(ref.nll_torch(lp, cls, il, tl).numpy() - want).max() < 1e-12
    assert np.abs(out["occ"][0, :, 0] - 1.0).max() < 1e-12 and np.abs(out["occ"][:, :, 1]).max() == 0.0


def test_infeasible_utterances_agree_with_the_plan():
    """in_len < tl + repeats: nll = inf, zero gradient, roww = 0 - and exactly the utterances CtcPlan.finite marks."""
    from st_amd import functional as F_
    torch.manual_seed(3)
    tgt = torch.tensor([[3, 3, 3, 3, 0, 0], [1, 2, 3, 4, 5, 6], [2, 2, 5, 5, 0, 0], [7, 0, 0, 0, 0, 0], [4, 4, 0, 0, 0, 0]])
    tgt_len = torch.tensor([4, 6, 4, 1, 2])
    in_len = torch.tensor([6, 6, 6, 1, 2])          # 4 equal labels need 7 frames; 6 on 6 fine; 2 + 2 equal need 6; 1 on 1; 2 equal need 3
    rows = F_.Rows.packed(in_len, "cpu")
    plan = F_.CtcPlan(tgt, tgt_len, in_len, rows, 0, 16)
    lp = torch.log_softmax(torch.randn(5, 6, 7, dtype=torch.float64), -1)
    out = ref.alpha_beta(lp.numpy(), plan.classes.numpy(), in_len.numpy(), tgt_len.numpy(), coef=np.full(5, 0.25))
    assert plan.finite.tolist() == [False, True, True, True, False]
    assert np.array_equal(np.isfinite(out["nll"]), plan.finite.numpy())
    for b in (0, 4):
        assert out["nll"][b] == np.inf and np.abs(out["g"][b]).max() == 0.0 and out["roww"][b] == 0.0
    assert (out["roww"][[1, 2, 3]] == 0.25).all()
    assert plan.in_len_dev.dtype == torch.int32 and plan.in_len_dev.tolist() == in_len.tolist()
    assert plan.tgt_len_dev.dtype == torch.int32 and plan.tgt_len_dev.tolist() == tgt_len.tolist()
    assert torch.allclose(plan.inv_btl, 1.0 / (5 * tgt_len.clamp_min(1).float()))


def test_new_exports_in_header_binding_and_library():
    names = ["st_ctc_loss_ws_kib", "st_ctc_loss_fwd", "st_ctc_loss_grad"]
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "st_hip.h")).read(), flags=re.S)
    assert native.ABI_VERSION == int(re.search(r"#define\s+ST_ABI_VERSION\s+(\d+)", text).group(1)) == native.abi_fingerprint(text)
    decl = dict(re.findall(r"\bint\s+(st_[a-z0-9_]+)\s*\(([^;]*?)\)\s*;", text, flags=re.S))
    lib = native.load()
    assert lib.st_version() == native.ABI_VERSION
    syms = subprocess.run(["nm", "-D", "--defined-only", native.lib_path()], check=True, capture_output=True, text=True).stdout
    exported = set(re.findall(r"\bT\s+(st_[a-z0-9_]+)", syms))
    for n in names:
        assert n in decl and n in native.SIGNATURES and n in exported, n
        assert decl[n].count(",") + 1 == len(native.SIGNATURES[n]), n
    assert "st_ctc_loss.hip" in __import__("st_amd.build", fromlist=["SOURCES"]).SOURCES
    # the host-only workspace query: alpha + beta f32 [B, T, 2 L + 2] + f64 offsets [B, 2, T / 8 + 2], in KiB
    raw = lib._cdll.st_ctc_loss_ws_kib
    assert raw(32, 1000, 50) == (2 * 32 * 1000 * 102 * 4 + 16 * 32 * 127 + 1023) // 1024
    assert raw(1, 1, 0) == 1 and raw(32, 1000, 255) > 0 and raw(32, 1000, 256) == -1 and raw(-1, 10, 3) == -1
    assert native.ctc_loss_ws_bytes(32, 1000, 50) == raw(32, 1000, 50) * 1024
    with pytest.raises(ValueError):
        native.ctc_loss_ws_bytes(4, 100, 256)


def test_binding_argument_checks_raise_before_any_launch():
    B, T, C, L = 3, 9, 5, 4
    ok = dict(lp=torch.zeros(B, T, C), classes=torch.zeros(B, L, dtype=torch.int64), in_len=torch.full((B,), T, dtype=torch.int32),
              tgt_len=torch.full((B,), L, dtype=torch.int32), ws=torch.zeros(1 << 16, dtype=torch.uint8), nll=torch.zeros(B))
    bad = [dict(lp=torch.zeros(B, T, C, dtype=torch.float64)), dict(lp=torch.zeros(B, T, 2 * C)[:, :, ::2]), dict(lp=torch.zeros(B, T, 1)),
           dict(lp=torch.zeros(B * T, C)), dict(classes=torch.zeros(B, L, dtype=torch.int32)), dict(classes=torch.zeros(B, 256, dtype=torch.int64)),
           dict(classes=torch.zeros(B + 1, L, dtype=torch.int64)), dict(in_len=torch.full((B,), T, dtype=torch.int64)),
           dict(tgt_len=torch.full((B + 1,), L, dtype=torch.int32)), dict(nll=torch.zeros(B, dtype=torch.float64)),
           dict(ws=torch.zeros(16, dtype=torch.float32))]
    for change in bad:
        with pytest.raises(ValueError):
            native.ctc_loss_fwd(**{**ok, **change})
    okg = dict(ok, coef=torch.ones(B), g=torch.zeros(B, T, C), roww=torch.zeros(B))
    for change in bad + [dict(coef=torch.ones(B + 1)), dict(g=torch.zeros(B, T, C + 1)), dict(roww=torch.zeros(B, dtype=torch.float64))]:
        with pytest.raises(ValueError):
            native.ctc_loss_grad(**{**okg, **change})
    # well-formed arguments that are not on the GPU: refused as everywhere in the binding (no CPU fallback)
    with pytest.raises(RuntimeError):
        native.ctc_loss_fwd(**ok)
    with pytest.raises(RuntimeError):
        native.ctc_loss_grad(**okg)
    from st_amd import functional as F_
    with pytest.raises(ValueError):
        F_.ctc_loss(ok["lp"], ok["classes"], ok["in_len"], ok["tgt_len"], reduction="sum")
    with pytest.raises(ValueError):
        F_.ctc_loss(ok["lp"], ok["classes"], ok["in_len"], ok["tgt_len"], zero_infinity=False)


def _recording_dlogits(log):
    from tests import _emul
    inner = torch.no_grad()(_emul.ctc_dlogits)

    def ctc_dlogits(logits, lse, rowmap, T, roww, scat, gsmall, grad_out, dlogits, V=None):
        log.append((roww.clone(), gsmall.clone()))
        return inner(logits, lse, rowmap, T, roww, scat, gsmall, grad_out, dlogits, V=V)
    return ctc_dlogits


def _truth_for_plan(plan, w):
    coef = w / (plan.B * plan.tl.double().numpy())
    out = ref.alpha_beta(plan.lp.double().numpy(), plan.classes.numpy(), plan.in_len_dev.numpy(), plan.tgt_len_dev.numpy(), coef=coef)
    fin = np.isfinite(out["nll"])
    loss = float((np.where(fin, out["nll"], 0.0) / plan.tl.double().numpy()).mean())
    return out, loss


def test_ctc_rows_hip_feeds_dlogits_what_the_truth_says(monkeypatch):
    """CTCAttentionLoss.ctc_rows(impl="hip") under the emulations: the loss, the returned gradient, and - with fill_weight - the
    tensors st_ctc_dlogits receives (plan.g_lp, plan.roww, written by the gradient launch itself) against the fp64 truth on the
    batch of test_loss_heads_cpu (repeats, a blank-id label inside a target, padding, an infeasible utterance)."""
    from st_amd import functional as F_
    from tests._emul import emulated_kernels
    from tests._emul_ctc import emulated_ctc_loss
    from transformer.Loss import CTCAttentionLoss
    torch.manual_seed(0)
    d, V = 32, 23
    in_len = torch.tensor([30, 8, 25, 6, 22])
    tgt_len = torch.tensor([7, 5, 9, 6, 4])
    tgt = torch.tensor([[3, 5, 5, 9, 3, 0, 11, 0, 0], [8, 8, 8, 8, 8, 0, 0, 0, 0], [4, 7, 4, 7, 4, 7, 22, 1, 1],
                        [1, 2, 3, 4, 5, 6, 0, 0, 0], [9, 9, 9, 0, 0, 0, 0, 0, 0]])     # utterance 1: 5 equal labels on 8 frames
    enc0 = (torch.randn(int(in_len.sum()), d) * 0.7).to(torch.bfloat16)
    log = []
    with emulated_kernels(), emulated_ctc_loss(), monkeypatch.context() as mp:      # (undone before the emulations are)
        mp.setattr(native, "ctc_dlogits", _recording_dlogits(log))
        head = CTCAttentionLoss(d, V, ctc_weight=0.3)
        plan = head.plan(tgt, tgt_len, in_len, F_.Rows.packed(in_len, "cpu"))
        head.zero_grad_buffers()
        enc = enc0.clone().requires_grad_(True)
        lp = head.project_rows(enc, plan)
        loss1, g1 = head.ctc_rows(lp, plan, impl="hip")
        assert g1.data_ptr() != plan.g_lp.data_ptr() and float(plan.g_lp.abs().max()) == 0.0
        loss_t, g_t = head.ctc_rows(lp, plan, impl="torch")
        loss2, g2 = head.ctc_rows(lp, plan, impl="hip", fill_weight=0.3)
        assert g2 is plan.g_lp
        torch.autograd.backward([lp], [plan.g_lp])
    (roww, gsmall), = log
    out1, want_loss = _truth_for_plan(plan, 1.0)
    out3, _ = _truth_for_plan(plan, 0.3)
    assert not np.isfinite(out1["nll"][1]) and float(roww[1]) == 0.0 and float(gsmall[1].abs().max()) == 0.0
    assert abs(float(loss1) - want_loss) < 1e-5 * abs(want_loss) and abs(float(loss2) - want_loss) < 1e-5 * abs(want_loss)
    assert abs(float(loss_t) - want_loss) < 1e-4 * abs(want_loss)
    assert np.abs(g1.double().numpy() - out1["g"]).max() < 1e-6 * np.abs(out1["g"]).max()
    assert np.abs(gsmall.double().numpy() - out3["g"]).max() < 1e-6 * np.abs(out3["g"]).max()
    assert np.abs(roww.double().numpy() - out3["roww"]).max() < 1e-7
    assert enc.grad is not None and float(enc.grad.float().abs().sum()) > 0
    # (torch's float32 gradient is not compared: utterance 4 ends in a blank-id label, where it is not the derivative)
    assert g_t.shape == g1.shape


def test_joint_trainstep_hip_eager_feeds_dlogits_what_the_truth_says(monkeypatch):
    """JointTrainStep(ctc="hip", use_graph=False) on CPU tensors under the emulations: one step; the (roww, g_lp) that reach
    st_ctc_dlogits equal the fp64 truth evaluated on the step's own log-probabilities, the reported CTC loss is the truth's, and
    no CUDA stream is touched (there is no side stream on this path)."""
    import oracle as orc
    import transformer.Models as M
    import transformer.Utils as U
    from st_amd.trainer import JointTrainStep
    from tests._emul import emulated_kernels
    from tests._emul_ctc import emulated_ctc_loss
    from transformer.Loss import CTCAttentionLoss
    from transformer.Optim import ScheduledOptim
    cfg = U.AttrDict(dict(feature_dim=80, max_inputs_length=100, max_target_length=20, num_enc_layer=1, num_dec_layer=1, n_heads=4,
                          d_k=32, d_v=32, d_model=128, d_inner_hid=256, dropout=0.0, vocab_size=30))
    batch = orc.synthetic_batch(3, 60, 9, 80, 30, seed=6, t_min=30, l_min=4)
    x, in_len, tokens, tgt_len, gt = (batch[k] for k in ("x", "in_len", "tokens", "tgt_len", "gt"))
    monkeypatch.setattr(torch.cuda, "current_stream", lambda *a, **k: pytest.fail("the HIP path must not touch streams"))
    for impl in ("hip",):
        log = []
        with emulated_kernels(), emulated_ctc_loss(), monkeypatch.context() as mp:      # (undone before the emulations are)
            mp.setattr(native, "ctc_dlogits", _recording_dlogits(log))
            torch.manual_seed(0)
            model = M.Transformer(cfg).eval()
            U.init_parameters(model)
            head = CTCAttentionLoss(128, 30, ctc_weight=0.3)
            opt = ScheduledOptim(model, 128, U.AttrDict(n_warmup_steps=10 ** 9))
            step = JointTrainStep(model, opt, head, max_grad_norm=1e9, use_graph=False, ctc=impl)
            loss, att, ctc, gnorm = step(x, in_len, tokens, tgt_len, gt)
            plan = step._plan
        (roww, gsmall), = log
        out, want = _truth_for_plan(plan, 0.3)
        assert plan.ws is not None and step.graphs == []
        assert abs(float(ctc) - want) < 1e-5 * abs(want), (float(ctc), want)
        assert abs(float(loss) - (0.3 * want + 0.7 * float(att))) < 1e-5 * abs(float(loss))
        assert np.abs(gsmall.double().numpy() - out["g"]).max() < 1e-6 * np.abs(out["g"]).max()
        assert np.abs(roww.double().numpy() - out["roww"]).max() < 1e-7 and float(roww.min()) > 0
        assert float(head.ctc_proj.weight.grad.abs().sum()) > 0 and torch.isfinite(gnorm)
    with pytest.raises(ValueError):
        JointTrainStep(model, opt, head, max_grad_norm=1.0, ctc="cuda")
    monkeypatch.setenv("ST_CTC_LOSS", "hip")
    assert JointTrainStep(model, opt, head, max_grad_norm=1.0).ctc == "hip"
    monkeypatch.delenv("ST_CTC_LOSS")
    assert JointTrainStep(model, opt, head, max_grad_norm=1.0).ctc == "torch"
