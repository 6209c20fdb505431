"""-m "not gpu": forward-only validation (st_amd/evaluate.py:EvalStep over st_ce_eval_fwd / st_eval_note, csrc/st_eval.hip) -
its entry points in the ABI, the wrappers' argument checks, the closed form of the two kernels (tests/_emul_eval.py) against
torch in fp64 on the committed loss fixture, the constructor's refusals, and the driver itself on the emulated kernels.
The ``run_*`` bodies take a device: tests/test_eval_gpu.py calls them on the hardware."""
import contextlib
import os
import re
import subprocess

import numpy as np
import pytest
import torch
import torch.nn as nn
import torch.nn.functional as func

import oracle as orc
from st_amd import build, native
from st_amd import functional as F_
from st_amd import native as nv
from tests import _emul_eval
from tests._emul import emulated_kernels
from tests._emul_eval import emulated_eval
from tests.test_composition_cpu import _build, _load_c1
from transformer.Loss import LabelSmoothingLoss

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "st_hip.h")
EPS = 0.1
# NLL of a whole step against the fp64 oracle: bf16 activations against fp64 truth - the bound tests/test_composition_cpu.py's
# run_c1_step holds the full step's loss to (`abs(loss - truth) < 2e-2 * truth`; tests/test_modules_gpu.py::test_c1_full_step_gpu
# runs that body on the GPU) and the driver smoke's `rel < 2e-2`
STEP_LOSS_TOL = 2e-2


@contextlib.contextmanager
def emulated():
    with emulated_kernels(), emulated_eval():
        yield


# ---- 1. the two entry points in the ABI (header == binding == library == sources: tests/test_abi_cpu.py, for every entry point) ---
def test_eval_entry_points_are_declared_bound_and_defined():
    assert {"st_ce_eval_fwd", "st_eval_note"} <= set(native.SIGNATURES)
    assert "st_eval.hip" in build.SOURCES
    src = open(os.path.join(build.CSRC, "st_eval.hip")).read()
    assert set(re.findall(r'extern\s+"C"\s+int\s+(st\w+)\s*\(', src)) == {"st_ce_eval_fwd", "st_eval_note"}
    # no other source defines them
    for other in build.SOURCES:
        if other != "st_eval.hip":
            assert not re.findall(r'extern\s+"C"\s+int\s+(st_ce_eval_fwd|st_eval_note)\s*\(', open(os.path.join(build.CSRC, other)).read()), other


def test_versions():
    """One version, and it is the header's fingerprint - whatever its value (tests/test_abi_cpu.py holds the fingerprint itself)."""
    text = open(HEADER).read()
    assert native.load().st_version() == native.ABI_VERSION == native.abi_fingerprint(text)
    assert not [n for n in native.SIGNATURES if n.endswith("_version") and n != "st_version"]


# ---- 2. the wrappers refuse before any launch --------------------------------------------------------------------------------
def test_wrappers_check_their_arguments_before_any_launch():
    R, V, vp = 5, 30, 32
    ok = dict(logits=torch.zeros(R, vp), target=torch.ones(R, dtype=torch.int64), ignore_index=0, confidence=1.0, smooth=0.0,
              zero_col=-1, rows=torch.zeros(R, 4), V=V)
    for change, name in ((dict(V=vp + 1), "ldl >= V"), (dict(V=0), "ldl >= V"), (dict(zero_col=V), "zero_col"),
                         (dict(V=None, zero_col=vp), "zero_col"), (dict(logits=torch.zeros(R, vp, dtype=torch.float64)), "logits"),
                         (dict(logits=torch.zeros(vp, R).t()), "logits"), (dict(target=torch.ones(R, dtype=torch.int32)), "target"),
                         (dict(target=torch.ones(R - 1, dtype=torch.int64)), "target"), (dict(rows=torch.zeros(R, 3)), "rows"),
                         (dict(rows=torch.zeros(R, 4, dtype=torch.float64)), "rows"), (dict(rows=torch.zeros(4, R).t()), "rows"),
                         (dict(index=torch.zeros(R, dtype=torch.int32)), "index"), (dict(index=torch.zeros(R + 1, dtype=torch.int64)), "index")):
        with pytest.raises(ValueError, match=name):
            nv.ce_eval_fwd(**{**ok, **change})
    with pytest.raises(RuntimeError, match="GPU"):          # well-formed, but not on the GPU: no CPU fallback
        nv.ce_eval_fwd(**ok)
    okn = dict(rows=torch.zeros(R, 4), acc=torch.zeros(8, dtype=torch.float64), last=torch.zeros(4))
    for change, name in ((dict(acc=torch.zeros(8)), "acc"), (dict(acc=torch.zeros(7, dtype=torch.float64)), "acc"),
                         (dict(acc=torch.zeros(16, dtype=torch.float64)[::2]), "acc"), (dict(acc=None), "acc"),
                         (dict(last=torch.zeros(3)), "last"), (dict(last=torch.zeros(4, dtype=torch.float64)), "last"),
                         (dict(rows=torch.zeros(R, 5)), "rows"), (dict(denom=torch.ones(2)), "denom"),
                         (dict(denom=torch.ones(1, dtype=torch.float64)), "denom")):
        with pytest.raises(ValueError, match=name):
            nv.eval_note(**{**okn, **change})
    with pytest.raises(RuntimeError, match="GPU"):
        nv.eval_note(**okn)


# ---- 3. the closed form, in fp64, on the committed loss fixture --------------------------------------------------------------
def _fixture64(golden_dir):
    fx = dict(np.load(os.path.join(golden_dir, "loss_optim.npz")))
    return torch.from_numpy(fx["logits"]).double(), torch.from_numpy(fx["target"])


def _emul64(x, t, triple, denom=None):
    R = x.shape[0]
    rows, acc, last = torch.empty(R, 4, dtype=torch.float64), torch.zeros(8, dtype=torch.float64), torch.empty(4, dtype=torch.float64)
    _emul_eval.ce_eval_fwd(x, t, 0, triple[0], triple[1], triple[2], rows)
    _emul_eval.eval_note(rows, acc, last, denom=None if denom is None else torch.tensor([denom], dtype=torch.float64))
    return rows, acc, last


def test_emulation_is_torch_in_fp64_on_the_loss_fixture(golden_dir):
    x, t = _fixture64(golden_dir)
    R, V = x.shape
    n_tok = float((t != 0).sum())
    assert 0 < n_tok < R, "the fixture has both ignored and counted rows"
    close = lambda a, b: abs(float(a) - float(b)) <= 1e-12 * abs(float(b))      # noqa: E731
    plain = func.cross_entropy(x, t, ignore_index=0)
    hits = float(((torch.argmax(x, -1) == t) & (t != 0)).sum())
    # nn.CrossEntropyLoss(ignore_index=0)
    rows, acc, last = _emul64(x, t, (1.0, 0.0, -1))
    assert close(acc[0] / acc[1], nn.CrossEntropyLoss(ignore_index=0)(x, t)) and close(last[0], plain) and close(last[1], plain)
    assert acc.tolist()[3:] == [n_tok, hits, 1.0, 0.0, 0.0] and float(acc[1]) == n_tok
    assert float(last[2]) == hits / n_tok and float(last[3]) == n_tok
    assert torch.equal(rows[:, 2], ((torch.argmax(x, -1) == t) & (t != 0)).double())
    assert float(rows[t == 0].abs().max()) == 0.0
    # nn.CrossEntropyLoss(ignore_index=0, label_smoothing=0.1)
    crit = nn.CrossEntropyLoss(ignore_index=0, label_smoothing=EPS)
    spec = F_.ce_spec(crit, V)
    _, acc, last = _emul64(x, t, spec[:3])
    assert close(acc[0] / acc[1], crit(x, t)) and close(acc[2] / acc[3], plain) and float(acc[4]) == hits
    # transformer.Loss.LabelSmoothingLoss: divided by every row
    crit = LabelSmoothingLoss(EPS, V, ignore_index=0)
    spec = F_.ce_spec(crit, V)
    _, acc, last = _emul64(x, t, spec[:3], denom=float(R))
    ref = orc.label_smoothing_loss(x, t, EPS, 0)
    assert close(acc[0] / acc[1], ref) and close(last[0], ref) and float(acc[1]) == R and close(acc[2] / acc[3], plain)
    # ... and the module itself, which builds its smoothed target in fp32 (eps / (V - 1) rounded once: ~6e-8 relative)
    assert abs(float(acc[0] / acc[1]) - float(crit(x, t))) <= 1e-6 * float(ref)


def test_emulation_ties_strays_accumulation_and_empty_batches():
    V = 9
    x = torch.zeros(6, V, dtype=torch.float64)
    x[1, 3] = x[1, 7] = 2.0                 # a tie: the lower column is the arg-max
    x[2, V - 1] = 1.0
    t = torch.tensor([0, 3, V - 1, 7, V, -5])
    x[3] = x[1]
    rows = torch.empty(6, 4, dtype=torch.float64)
    _emul_eval.ce_eval_fwd(x, t, -1, 1.0, 0.0, -1, rows)
    assert rows[:, 2].tolist() == [1.0, 1.0, 1.0, 0.0, 0.0, 0.0] and rows[:, 3].tolist() == [1.0, 1.0, 1.0, 1.0, 2.0, 2.0]
    assert float(rows[4:, :3].abs().max()) == 0.0
    acc, last = torch.zeros(8, dtype=torch.float64), torch.empty(4)
    for k in range(3):
        _emul_eval.eval_note(rows, acc, last, denom=torch.tensor([5.0]))
    assert acc.tolist() == [3 * float(rows[:, 0].sum()), 15.0, 3 * float(rows[:, 1].sum()), 12.0, 9.0, 3.0, 6.0, 0.0]
    before = acc.clone()
    _emul_eval.ce_eval_fwd(x, torch.full((6,), -1), -1, 1.0, 0.0, -1, rows)      # all ignored
    _emul_eval.eval_note(rows, acc, last)
    assert torch.equal(acc[:5], before[:5]) and float(acc[5]) == 4.0 and bool(torch.isnan(last[:3]).all()) and float(last[3]) == 0.0


# ---- 4. the constructor ----------------------------------------------------------------------------------------------------------
def test_constructor_refusals(golden_dir):
    from st_amd.evaluate import EvalStep
    _, w, _ = _load_c1(golden_dir)
    m = _build(w)
    with pytest.raises(ValueError, match="bucket"):
        EvalStep(m, 30)                                        # use_graph defaults to True
    with pytest.raises(ValueError, match="bucket"):
        EvalStep(m, 30, use_graph=True, bucket=None)
    with pytest.raises(ValueError, match="bucket_rows needs"):
        EvalStep(m, 30, use_graph=False, bucket_rows=(100, 20))
    for crit in (nn.CrossEntropyLoss(), nn.CrossEntropyLoss(ignore_index=0, reduction="sum"), nn.NLLLoss(ignore_index=0),
                 nn.CrossEntropyLoss(weight=torch.ones(30), ignore_index=0), LabelSmoothingLoss(EPS, 31, ignore_index=0)):
        with pytest.raises(ValueError, match="not supported|vocabulary"):
            EvalStep(m, 30, criterion=crit, use_graph=False)
    with pytest.raises(ValueError, match="forward_packed"):
        EvalStep(nn.Linear(2, 2), 30, use_graph=False)
    ev = EvalStep(m, 30, use_graph=True, bucket=(100, 20), bucket_rows=(300, 40))
    assert ev.bucket == (100, 20) and ev.bucket_rows == [(300, 40)] and ev.norm == "tokens"
    assert EvalStep(m, 30, criterion=LabelSmoothingLoss(EPS, 30, ignore_index=0), use_graph=False).norm == "rows"
    r = EvalStep(m, 30, use_graph=False).result()             # nothing evaluated yet: no device, no numbers
    assert r["tokens"] == 0 and r["batches"] == 0 and r["loss"] != r["loss"]


# ---- 5. the driver (bodies shared with the GPU tests) --------------------------------------------------------------------------
def c1_case(golden_dir, device):
    """BASELINE config 1 (d_model 128) on its committed step fixture -> (model, batch on the device, fp64 oracle loss)."""
    _, w, batch = _load_c1(golden_dir)
    truth = orc.train_step({k: v.double() for k, v in w.items()},
                           {k: (v.double() if v.is_floating_point() else v) for k, v in batch.items()}, 4, 128, 100, 1, 5.0)
    m = _build(w, device=device)
    return m, _to(batch, device), 30, float(truth["loss"])


def d256_case(device):
    """The d_model-256 row-chain model and batch of the driver smoke."""
    import transformer.Models as M
    import transformer.Utils as U
    p = orc.xavier_init_(orc.make_params(80, 30, 256, 512, 1, 2, 100, 20, dtype=torch.float64), seed=3)
    b = orc.synthetic_batch(3, 70, 9, 80, 30, seed=4, t_min=30, l_min=4)
    truth = orc.train_step(p, {k: (v.double() if v.is_floating_point() else v) for k, v in b.items()}, 4, 256, 100, 1, 5.0)
    cfg = U.AttrDict(dict(feature_dim=80, max_inputs_length=100, max_target_length=20, num_enc_layer=1, num_dec_layer=2,
                          n_heads=4, d_k=64, d_v=64, d_model=256, d_inner_hid=512, dropout=0.0, vocab_size=30))
    m = M.Transformer(cfg)
    m.load_state_dict({k: v.float() for k, v in p.items()})
    return m.eval().to(device), _to(b, device), 30, float(truth["loss"])


def _to(batch, device):
    return (batch["x"].to(device), batch["in_len"], batch["tokens"].to(device), batch["tgt_len"], batch["gt"].to(device))


def run_step_consistency_and_oracle(model, batch, V, oracle_loss, row_tol=1e-5):
    """EvalStep (eager, packed layouts) on one batch: hits and tokens EQUAL torch's arg-max and count on the logits
    forward_packed returns for that batch; NLL within ``row_tol`` of torch's fp64 cross-entropy over those logits, and within
    STEP_LOSS_TOL of the fp64 oracle.  Accuracy is not compared with the oracle: at random initialisation the margins between
    the best two columns are below bf16 noise."""
    from st_amd.evaluate import EvalStep
    x, in_len, tok, tgt_len, gt = batch
    l_max = int(tgt_len.max())
    with torch.no_grad():
        logits, t_rows = model.forward_packed(x[:, :int(in_len.max())], in_len, tok[:, :l_max], tgt_len)
    t = gt[:, :l_max].contiguous().view(-1)[t_rows.scatter_index(l_max)]
    lg = logits.double()
    n_tok = int((t != 0).sum())
    hits = int(((torch.argmax(lg, -1) == t) & (t != 0)).sum())
    nll64 = float(func.cross_entropy(lg, t, ignore_index=0))
    ev = EvalStep(model, V, use_graph=False)
    last = ev(*batch)
    r = ev.result()
    print("EvalStep: nll %.6f (fp64 over the same logits %.6f, oracle %.6f), hits %d / %d" % (r["nll"], nll64, oracle_loss, hits, n_tok))
    assert r["tokens"] == n_tok and 0 < n_tok <= int(tgt_len.sum()) and r["batches"] == 1 and r["bad_targets"] == 0
    assert r["accuracy"] * n_tok == hits
    assert abs(r["nll"] - nll64) <= row_tol * abs(nll64) and r["loss"] == r["nll"]
    assert abs(r["ppl"] - float(np.exp(r["nll"]))) <= 1e-12 * r["ppl"]
    assert abs(r["nll"] - oracle_loss) < STEP_LOSS_TOL * oracle_loss
    assert abs(float(last[1]) - r["nll"]) <= 1e-6 * r["nll"] and float(last[3]) == n_tok
    # a second batch accumulates; reset() starts over
    ev(*batch)
    r2 = ev.result()
    assert r2["tokens"] == 2 * n_tok and r2["batches"] == 2 and abs(r2["nll"] - r["nll"]) <= 1e-12 * r["nll"]
    ev.reset()
    ev(*batch)
    assert ev.result() == r
    return ev


def run_model_mode(model, batch, V):
    from st_amd.evaluate import EvalStep
    ev = EvalStep(model, V, use_graph=False)
    model.train()
    try:
        with pytest.raises(RuntimeError, match="training mode"):
            ev(*batch)
        model.eval()
        model.decoder.train()                  # one module left in training mode is refused as well
        with pytest.raises(RuntimeError, match="training mode"):
            ev(*batch)
    finally:
        model.eval()
    ev(*batch)
    assert ev.result()["batches"] == 1


def test_step_c1_on_emulated_kernels(golden_dir):
    with emulated():
        m, batch, V, truth = c1_case(golden_dir, "cpu")
        run_step_consistency_and_oracle(m, batch, V, truth)
        run_model_mode(m, batch, V)


def test_step_criteria_on_emulated_kernels(golden_dir):
    """The three criteria through the driver: loss = the criterion on the padded logits ``model(...)`` returns, nll and accuracy
    the same for all three; the "rows" denominator follows B * l_max of the trimmed batch."""
    from st_amd.evaluate import EvalStep
    with emulated():
        m, batch, V, _ = c1_case(golden_dir, "cpu")
        x, in_len, tok, tgt_len, gt = batch
        with torch.no_grad():
            logits, _ = m(x, in_len, tok, tgt_len)
        flat, t = logits.double().view(-1, V), gt.view(-1)
        seen = []
        for crit, ref in ((nn.CrossEntropyLoss(ignore_index=0, label_smoothing=EPS), None),
                          (LabelSmoothingLoss(EPS, V, ignore_index=0), orc.label_smoothing_loss(flat, t, EPS, 0)),
                          (LabelSmoothingLoss(EPS, V, size_average=False, ignore_index=0), orc.label_smoothing_loss(flat, t, EPS, 0) * t.numel())):
            ref = float(crit(flat, t)) if ref is None else float(ref)
            ev = EvalStep(m, V, criterion=crit, use_graph=False)
            ev(*batch)
            r = ev.result()
            assert abs(r["loss"] - ref) <= 1e-5 * abs(ref), (type(crit).__name__, r["loss"], ref)
            seen.append((r["nll"], r["accuracy"], r["tokens"]))
        assert seen[0] == seen[1] == seen[2]
