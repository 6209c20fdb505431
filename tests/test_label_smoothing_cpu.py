"""-m "not gpu": label-smoothed cross-entropy on the HIP loss path - the closed form the kernels implement (held to three fp64
references through the test-only emulation tests/_emul_ce.py), the criterion -> kernel mapping (functional.ce_spec), the two
entry points in the ABI, and the wiring through TrainStep(criterion=...) / JointTrainStep against the fp64 oracle.

The ``run_*`` bodies take a device: tests/test_label_smoothing_gpu.py calls the same bodies on the hardware."""
import copy
import ctypes
import os
import re
import subprocess

import pytest
import torch
import torch.nn as nn
import torch.nn.functional as func

import oracle as orc
from st_amd import build, native
from st_amd import functional as F_
from tests import _emul_ce
from tests._emul import emulated_kernels
from tests._emul_ce import emulated_ce_smooth
from tests.test_composition_cpu import GRAD_TOL_GLOBAL, GRAD_TOL_MEDIAN, GRAD_TOL_TENSOR, _build, _load_c1, rel
from transformer.Loss import CTCAttentionLoss, LabelSmoothingLoss

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EPS = 0.1


def make_criterion(kind, V=30):
    return LabelSmoothingLoss(EPS, V, ignore_index=0) if kind == "ls" else nn.CrossEntropyLoss(ignore_index=0, label_smoothing=EPS)


# ---- 1. the emulation is the truth (fp64) ----------------------------------------------------------------------------------
def _case64(V, R=45, seed=0):
    gen = torch.Generator().manual_seed(seed)
    x = torch.randn(R, V, generator=gen, dtype=torch.float64) * 3
    t = torch.randint(1, V, (R,), generator=gen)
    t[::4] = 0
    t[1] = V - 1
    return x, t


def _emul64(x, t, spec, denom):
    R, V = x.shape
    lse, sums, dl = torch.empty(R, dtype=torch.float64), torch.empty(4, dtype=torch.float64), torch.empty(R, V, dtype=torch.float64)
    d = None if denom is None else torch.tensor([denom], dtype=torch.float64)
    _emul_ce.ce_smooth_fwd(x, t, 0, spec[0], spec[1], spec[2], lse, sums, denom=d)
    _emul_ce.ce_smooth_bwd(x, t, 0, spec[0], spec[1], spec[2], lse, sums, torch.tensor([0.7], dtype=torch.float64), dl, denom=d)
    return sums, dl


@pytest.mark.parametrize("V", [30, 257])
def test_emulation_is_the_closed_form_in_fp64(V):
    x, t = _case64(V)
    R = x.shape[0]
    # (a) the reference's LabelSmoothingLoss (oracle restatement), divided by all R rows
    leaf = x.clone().requires_grad_(True)
    ref = orc.label_smoothing_loss(leaf, t, EPS, 0)
    (g_ref,) = torch.autograd.grad(ref * 0.7, leaf)
    sums, dl = _emul64(x, t, F_.ce_spec(LabelSmoothingLoss(EPS, V, ignore_index=0), V), float(R))
    assert abs(float(sums[2]) - float(ref.detach())) <= 1e-12 * abs(float(ref.detach())), float(sums[2])
    assert float((dl - g_ref).abs().max()) <= 1e-12 * float(g_ref.abs().max())
    # (b) torch's label smoothing, mean over the non-ignored tokens
    leaf = x.clone().requires_grad_(True)
    ref = func.cross_entropy(leaf, t, label_smoothing=EPS, ignore_index=0)
    (g_ref,) = torch.autograd.grad(ref * 0.7, leaf)
    sums, dl = _emul64(x, t, F_.ce_spec(nn.CrossEntropyLoss(ignore_index=0, label_smoothing=EPS), V), None)
    assert abs(float(sums[2]) - float(ref.detach())) <= 1e-12 * abs(float(ref.detach())), float(sums[2])
    assert float((dl - g_ref).abs().max()) <= 1e-12 * float(g_ref.abs().max())
    plain = func.cross_entropy(x, t, ignore_index=0)
    assert abs(float(sums[3]) - float(plain)) <= 1e-12 * float(plain) and float(sums[1]) == float((t != 0).sum())
    # (c) the plain loss at (1, 0, -1): the smoothed kernels' degenerate case
    leaf = x.clone().requires_grad_(True)
    ref = func.cross_entropy(leaf, t, ignore_index=0)
    (g_ref,) = torch.autograd.grad(ref * 0.7, leaf)
    sums, dl = _emul64(x, t, (1.0, 0.0, -1), None)
    assert abs(float(sums[2]) - float(ref.detach())) <= 1e-12 * abs(float(ref.detach())) and float(sums[3]) == float(sums[2])
    assert float((dl - g_ref).abs().max()) <= 1e-12 * float(g_ref.abs().max())
    assert float(dl[::4].abs().max()) == 0.0


# ---- 2. criterion -> kernels -----------------------------------------------------------------------------------------------
def test_ce_spec_table():
    V, e = 30, 0.1
    assert F_.ce_spec(None, V) is None
    assert F_.ce_spec(nn.CrossEntropyLoss(ignore_index=0), V) is None
    assert F_.ce_spec(nn.CrossEntropyLoss(ignore_index=0, label_smoothing=e), V) == F_.CeSpec(1 - e + e / V, e / V, -1, "tokens")
    assert F_.ce_spec(LabelSmoothingLoss(e, V, ignore_index=0), V) == F_.CeSpec(1 - e, e / (V - 1), 0, "rows")
    assert F_.ce_spec(LabelSmoothingLoss(e, V, size_average=False, ignore_index=0), V) == F_.CeSpec(1 - e, e / (V - 1), 0, "sum")
    spec = F_.ce_spec(LabelSmoothingLoss(e, V, ignore_index=0), V)
    assert tuple(spec) == (spec.confidence, spec.smooth, spec.zero_col, spec.norm)
    bad = [nn.CrossEntropyLoss(weight=torch.ones(V), ignore_index=0), nn.CrossEntropyLoss(ignore_index=0, reduction="sum"),
           nn.CrossEntropyLoss(ignore_index=0, reduction="none", label_smoothing=e), nn.CrossEntropyLoss(),
           nn.CrossEntropyLoss(ignore_index=-1, label_smoothing=e), LabelSmoothingLoss(e, V), LabelSmoothingLoss(e, V, ignore_index=3),
           LabelSmoothingLoss(e, V, weight=torch.ones(V), ignore_index=0), LabelSmoothingLoss(e, V + 1, ignore_index=0),
           nn.NLLLoss(ignore_index=0), nn.MSELoss()]
    for crit in bad:
        with pytest.raises(ValueError, match="not supported|vocabulary"):
            F_.ce_spec(crit, V)


# ---- 3. the two entry points in the ABI (header == binding == library == sources: tests/test_abi_cpu.py, for every entry point) ---
def test_smoothed_entry_points_of_the_abi():
    assert {"st_ce_smooth_fwd", "st_ce_smooth_bwd"} <= set(native.SIGNATURES)
    fwd, bwd = native.SIGNATURES["st_ce_smooth_fwd"], native.SIGNATURES["st_ce_smooth_bwd"]
    assert fwd[8] is ctypes.c_float and fwd[9] is ctypes.c_float and fwd[10] is ctypes.c_int and fwd[11] is ctypes.c_void_p
    assert bwd[8] is ctypes.c_float and bwd[9] is ctypes.c_float and bwd[10] is ctypes.c_int and bwd[11] is ctypes.c_void_p
    assert fwd[0] is ctypes.c_void_p and fwd[7] is ctypes.c_int and len(fwd) == 15 and len(bwd) == 17 and bwd[-1] is ctypes.c_int
    assert "st_loss.hip" in build.SOURCES
    src = open(os.path.join(build.CSRC, "st_loss.hip")).read()
    assert re.search(r'^\s*#\s*include\s+"st_hip.h"', src, flags=re.M)
    assert set(re.findall(r'extern\s+"C"\s+int\s+(st\w+)\s*\(', src)) == {"st_ce_smooth_fwd", "st_ce_smooth_bwd"}


def test_binding_argument_checks_raise_before_any_launch():
    R, V, vp = 5, 30, 32
    ok = dict(logits=torch.zeros(R, vp), target=torch.ones(R, dtype=torch.int64), ignore_index=0, confidence=0.9, smooth=0.1 / 29,
              zero_col=0, lse=torch.zeros(R), sums=torch.zeros(4), V=V)
    okb = dict(ok, grad_out=torch.ones(1), dlogits=torch.zeros(R, vp, dtype=torch.bfloat16))
    for change in (dict(V=vp + 1), dict(V=0), dict(zero_col=V), dict(V=None, zero_col=vp)):      # (plain numbers: refused on any device)
        with pytest.raises(ValueError, match="TRUE vocabulary"):
            native.ce_smooth_fwd(**{**ok, **change})
        with pytest.raises(ValueError, match="TRUE vocabulary"):
            native.ce_smooth_bwd(**{**okb, **change})
    with pytest.raises(RuntimeError):          # well-formed, but not on the GPU: no CPU fallback
        native.ce_smooth_fwd(**ok)
    with pytest.raises(RuntimeError):
        native.ce_smooth_bwd(**okb)
    spec = F_.CeSpec(0.9, 0.1 / 29, 0, "rows")
    with emulated_kernels(), emulated_ce_smooth():
        with pytest.raises(ValueError, match="denominator"):
            F_.cross_entropy_rows(torch.zeros(R, V), torch.ones(R, dtype=torch.int64), 0, spec=spec)


# ---- 4. TrainStep(criterion=...) against the fp64 oracle -------------------------------------------------------------------
def _truth_c1(w, batch, kind):
    """fp64: oracle.transformer + the smoothed loss on logits.view(-1, 30) / gt.view(-1), autograd gradients, global norm - the
    rest of oracle.train_step."""
    p = {k: v.double() for k, v in w.items()}
    names = [n for n in p if not n.endswith(".pe")]
    leaves = {n: (p[n].clone().requires_grad_(True) if n in names else p[n]) for n in p}
    ti, tl = int(batch["in_len"].max()), int(batch["tgt_len"].max())
    logits, _ = orc.transformer(leaves, batch["x"][:, :ti].double(), batch["in_len"], batch["tokens"][:, :tl], batch["tgt_len"], 4)
    gt = batch["gt"][:, :tl]
    flat, t = logits.reshape(-1, 30), gt.reshape(-1)
    n_rows, n_tok = t.numel(), int((t != 0).sum())
    if kind == "ls":
        loss = orc.label_smoothing_loss(flat, t, EPS, 0)
        wrong = loss * n_rows / n_tok              # the same sum over the token count: what a "tokens" denominator would give
    else:
        loss = func.cross_entropy(flat, t, label_smoothing=EPS, ignore_index=0)
        wrong = loss * n_tok / n_rows
    grads = torch.autograd.grad(loss, [leaves[n] for n in names], allow_unused=True)
    grads = {n: (g if g is not None else torch.zeros_like(p[n])) for n, g in zip(names, grads)}
    total = torch.sqrt(sum((g ** 2).sum() for g in grads.values()))
    return dict(loss=float(loss.detach()), wrong=float(wrong.detach()), nll=float(orc.cross_entropy(logits, gt).detach()), grads=grads, gnorm=float(total))


def run_smooth_trainstep_vs_oracle(golden_dir, device, kind, use_graph=False):
    import transformer.Utils as U
    from st_amd.arena import arena_of
    from st_amd.trainer import TrainStep
    from transformer.Optim import ScheduledOptim
    fx, w, batch = _load_c1(golden_dir)
    truth = _truth_c1(w, batch, kind)
    m = _build(w, device=device)
    opt = ScheduledOptim(m, 128, U.AttrDict(n_warmup_steps=10 ** 9))          # ~zero learning rate: the weights stay put
    step = TrainStep(m, opt, 30, 1e9, use_graph=use_graph, graph_warmup=0, criterion=make_criterion(kind))
    assert step.ce_spec is not None and step.ce_spec.norm == ("rows" if kind == "ls" else "tokens")
    x, tok, gt = batch["x"].to(device), batch["tokens"].to(device), batch["gt"].to(device)
    if use_graph:     # lazy set-up (arena, ragged layouts, work lists) must not happen inside the capture
        with torch.no_grad():
            m.forward_packed(x, batch["in_len"], tok[:, :10], batch["tgt_len"])
    loss, gnorm = step(x, batch["in_len"], tok, batch["tgt_len"], gt)
    loss, gnorm, nll = float(loss), float(gnorm), float(step.nll)
    print("smoothed C1 step (%s, graph=%s): loss %.6f (fp64 %.6f), norm %.5f (%.5f), nll %.6f (%.6f)"
          % (kind, use_graph, loss, truth["loss"], gnorm, truth["gnorm"], nll, truth["nll"]))
    assert abs(loss - truth["loss"]) <= 2e-2 * truth["loss"], (loss, truth["loss"])
    assert abs(gnorm - truth["gnorm"]) <= 2e-2 * truth["gnorm"], (gnorm, truth["gnorm"])
    assert abs(nll - truth["nll"]) <= 2e-2 * truth["nll"], (nll, truth["nll"])
    # a wrong denominator cannot pass: the same sum over the other count (the fixture has 32 tokens in 40 rows: a factor 0.8 or
    # 1.25) lies five times the loss bound away or more
    assert abs(loss - truth["wrong"]) > 5 * 2e-2 * truth["wrong"], (loss, truth["wrong"])
    if kind == "ls":          # ... and nll is not the loss under another name (with the token mean and a near-uniform model the
        assert abs(truth["nll"] - truth["loss"]) > 4e-2 * truth["nll"]      # two lie within the bound of each other: no statement)
    arena = arena_of(m)
    bad, rels, flat_g, flat_t = [], [], [], []
    for n, p in m.named_parameters():
        g, t = arena.grad_view(p).detach().cpu(), truth["grads"][n]          # (max_grad_norm 1e9: nothing was clipped)
        assert torch.isfinite(g).all(), n
        if "linear_k.bias" in n:
            # analytically zero; bf16 rounding of dK leaves noise well below the q-bias gradient scale
            assert g.abs().max().item() < 2.5e-1 * truth["grads"][n.replace("linear_k", "linear_q")].abs().max().item() + 1e-6
            continue
        rels.append(rel(g, t))
        flat_g.append(g.double().reshape(-1))
        flat_t.append(t.double().reshape(-1))
        if rels[-1] > GRAD_TOL_TENSOR:
            bad.append((n, rels[-1]))
    assert not bad, bad
    assert sorted(rels)[len(rels) // 2] < GRAD_TOL_MEDIAN, sorted(rels)[len(rels) // 2]
    assert rel(torch.cat(flat_g), torch.cat(flat_t)) < GRAD_TOL_GLOBAL
    if not use_graph:
        return
    # a second, different batch of the same length signature through the captured step (the loader refills its buffers in
    # place): the loss and the nll must follow it - against the eager step on the same (unmoved) weights
    assert len(step._graphs) == 1
    valid = gt > 0
    gt.copy_(torch.where(valid, (gt + 7) % 26 + 4, gt))
    x.mul_(0.5)
    loss2, _ = step(x, batch["in_len"], tok, batch["tgt_len"], gt)
    loss2, nll2 = float(loss2), float(step.nll)
    assert len(step._graphs) == 1 and step._g_fb is not None
    eager = TrainStep(m, opt, 30, 1e9, use_graph=False, criterion=make_criterion(kind))
    want, _ = eager(x, batch["in_len"], tok, batch["tgt_len"], gt)
    want, want_nll = float(want), float(eager.nll)
    assert abs(want - loss) > 1e-2 * abs(loss), "the two batches must differ in their loss"
    assert abs(loss2 - want) <= 2e-3 * abs(want), (loss2, want)
    assert abs(nll2 - want_nll) <= 2e-3 * abs(want_nll), (nll2, want_nll)


@pytest.mark.parametrize("kind", ["ls", "ce"])
def test_smooth_trainstep_vs_oracle_composition(golden_dir, kind):
    with emulated_kernels(), emulated_ce_smooth():
        run_smooth_trainstep_vs_oracle(golden_dir, "cpu", kind)


def test_trainstep_refuses_a_criterion_the_fast_path_cannot_honour(golden_dir):
    import transformer.Utils as U
    from st_amd.trainer import TrainStep
    from transformer.Optim import ScheduledOptim
    _, w, _ = _load_c1(golden_dir)
    with emulated_kernels():
        m = _build(w)
        opt = ScheduledOptim(m, 128, U.AttrDict(n_warmup_steps=100))
        for crit in (nn.CrossEntropyLoss(weight=torch.ones(30), ignore_index=0), LabelSmoothingLoss(EPS, 31, ignore_index=0),
                     nn.CrossEntropyLoss(label_smoothing=EPS)):
            with pytest.raises(ValueError):
                TrainStep(m, opt, 30, 5.0, criterion=crit)
        assert TrainStep(m, opt, 30, 5.0).ce_spec is None
        assert TrainStep(m, opt, 30, 5.0, criterion=nn.CrossEntropyLoss(ignore_index=0)).ce_spec is None


# ---- 5. the joint CTC + attention step honours head.att_criterion -------------------------------------------------------
def run_joint_smooth_step(device, use_graph=False, d_model=128, layers=1):
    """JointTrainStep(ctc="hip") with att_criterion=LabelSmoothingLoss: the attention loss it returns is the torch module's on the
    padded logits; in graph mode one graph, whose attention loss equals the eager step's."""
    import transformer.Models as M
    import transformer.Utils as U
    from st_amd.trainer import JointTrainStep
    from transformer.Optim import ScheduledOptim
    cfg = U.AttrDict(dict(feature_dim=80, max_inputs_length=100, max_target_length=20, num_enc_layer=layers, num_dec_layer=layers,
                          n_heads=4, d_k=d_model // 4, d_v=d_model // 4, d_model=d_model, d_inner_hid=2 * d_model, dropout=0.0,
                          vocab_size=30))
    batch = orc.synthetic_batch(3, 60, 9, 80, 30, seed=6, t_min=30, l_min=4)
    x, in_len, tokens, tgt_len, gt = (batch[k] for k in ("x", "in_len", "tokens", "tgt_len", "gt"))
    x, tokens, gt = x.to(device), tokens.to(device), gt.to(device)
    torch.manual_seed(0)
    model = M.Transformer(cfg)
    U.init_parameters(model)
    model = model.eval().to(device)
    crit = LabelSmoothingLoss(EPS, 30, ignore_index=0)
    opt = ScheduledOptim(model, d_model, U.AttrDict(n_warmup_steps=10 ** 9))       # ~zero learning rate: the weights stay put

    def make(graph):
        torch.manual_seed(1)
        head = CTCAttentionLoss(d_model, 30, ctc_weight=0.3, att_criterion=crit).to(device)
        return JointTrainStep(model, opt, head, max_grad_norm=1e9, use_graph=graph, graph_warmup=1, ctc="hip")

    step = make(False)
    assert step.ce_spec == F_.CeSpec(1 - EPS, EPS / 29, 0, "rows")
    loss, att, ctc, gnorm = step(x, in_len, tokens, tgt_len, gt)
    att, nll = float(att), float(step.nll)
    L = int(tgt_len.max())
    with torch.no_grad():
        logits, _ = model(x, in_len, tokens[:, :L], tgt_len)
        flat, t = logits.reshape(-1, 30).float(), gt[:, :L].reshape(-1)
        want = float(crit.to(device)(flat, t))
        want_nll = float(func.cross_entropy(flat, t, ignore_index=0))
    assert abs(att - want) <= 2e-2 * abs(want), (att, want)
    assert abs(nll - want_nll) <= 2e-2 * abs(want_nll) and abs(want - want_nll) > 4e-2 * want_nll
    assert abs(float(loss) - (0.3 * float(ctc) + 0.7 * att)) <= 1e-5 * abs(float(loss)) and torch.isfinite(gnorm)
    # a head whose criterion the fast path cannot honour raises (it used to train with the plain loss, silently)
    weighted = CTCAttentionLoss(d_model, 30, att_criterion=nn.CrossEntropyLoss(weight=torch.ones(30), ignore_index=0)).to(device)
    with pytest.raises(ValueError, match="class weights"):
        JointTrainStep(model, opt, weighted, max_grad_norm=1.0, ctc="hip")
    assert JointTrainStep(model, opt, CTCAttentionLoss(d_model, 30).to(device), max_grad_norm=1.0, ctc="hip").ce_spec is None
    if use_graph:
        gstep = make(True)
        for _ in range(3):
            out = [float(v) for v in gstep(x, in_len, tokens, tgt_len, gt)]
        assert len(gstep.graphs) == 1
        assert abs(out[1] - att) <= 2e-3 * abs(att), (out[1], att)
        assert abs(float(gstep.nll) - nll) <= 2e-3 * abs(nll)


def test_joint_smooth_step_composition():
    from tests._emul_ctc import emulated_ctc_loss
    with emulated_kernels(), emulated_ctc_loss(), emulated_ce_smooth():
        run_joint_smooth_step("cpu")


# ---- 9 (body; runs on the GPU only: a capture is what it is about) -------------------------------------------------------
def run_smooth_bucket_mode(device, use_graph, bucket_rows=None, T_cap=96, L_cap=12):
    """TrainStep(bucket=..., criterion=LabelSmoothingLoss) - norm "rows", D = B * l_max: batches whose l_max differ, served by ONE
    bucket (one capture in graph mode); every loss equals the eager un-bucketed step's on the same batch and weights.  A
    denominator baked into the capture would be off by l_max' / l_max."""
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
    oa = ScheduledOptim(ma, 256, U.AttrDict(n_warmup_steps=10 ** 9))          # ~zero learning rate: both twins stay put
    ob = ScheduledOptim(mb, 256, U.AttrDict(n_warmup_steps=10 ** 9))
    crit = LabelSmoothingLoss(EPS, 30, ignore_index=0)
    sa = TrainStep(ma, oa, 30, 5.0, use_graph=use_graph, graph_warmup=1, bucket=(T_cap, L_cap), bucket_rows=bucket_rows, criterion=crit)
    sb = TrainStep(mb, ob, 30, 5.0, use_graph=False, criterion=crit)
    denoms, caps = [], []
    for i, l_max in enumerate((L_cap, L_cap, L_cap - 3, L_cap - 5)):      # (the first call is the eager warm-up)
        b = orc.synthetic_batch(4, 80, l_max, 80, 30, seed=40 + i, t_min=40, l_min=4)
        T, L = int(b["in_len"].max()), int(b["tgt_len"].max())
        assert L == l_max
        x, tok, gt = b["x"][:, :T].to(device), b["tokens"][:, :L].to(device), b["gt"][:, :L].to(device)
        la, _ = sa(x, b["in_len"], tok, b["tgt_len"], gt)
        lb, _ = sb(x, b["in_len"], tok, b["tgt_len"], gt)
        la, lb, na, nb = float(la), float(lb), float(sa.nll), float(sb.nll)
        print("bucket %s graph=%s batch %d: l_max %d loss %.6f (eager %.6f) nll %.6f (%.6f)" % (bucket_rows, use_graph, i, L, la, lb, na, nb))
        assert abs(la - lb) <= 2e-3 * abs(lb), (i, la, lb)
        assert abs(na - nb) <= 2e-3 * abs(nb), (i, na, nb)
        denoms.append(float(sa._ce_denom))
        caps.append(sa._g_fb if use_graph and i else None)
    assert denoms == [4.0 * L_cap, 4.0 * L_cap, 4.0 * (L_cap - 3), 4.0 * (L_cap - 5)]
    assert len(sa._buckets) == 1
    if use_graph:
        assert caps[1] is not None and caps[1] is caps[2] is caps[3], "one capture serves every l_max"


@pytest.mark.parametrize("bucket_rows", [None, (340, 48)])
def test_smooth_bucket_mode_composition(bucket_rows):
    with emulated_kernels(), emulated_ce_smooth():
        run_smooth_bucket_mode("cpu", use_graph=False, bucket_rows=bucket_rows)
