"""The checks of tests/test_lse_fp64_gpu.py on the CPU: the emulations (tests/_emul.py, _emul_ce.py, _emul_eval.py; plain fp32 torch
restatements where there is none) pass every family at every V unmodified, and every defect of the table in tests/LOCAL_BOUNDS.md,
injected into an emulation's computation or output, is reported by the check named there.  Also held here: the two conditions on
the measured bounds (L_LSE <= log(5120 / 5119) / 4, P_REL <= 2^-10, both equal to what tools/local_bounds.py measures) and that the
reference alone shows no near tie on the families that may not use the exemption."""
import numpy as np
import pytest
import torch

from tests import _emul_ce as emc
from tests import _lse_cases as lc
from tests import _lse_ref as ref

F32, F64, BF16 = torch.float32, torch.float64, torch.bfloat16
CASES = lc.cases()
BIG = tuple(V for V in lc.VS if V >= 257)


@pytest.fixture(scope="module")
def be():
    return lc.cpu_backend()


@pytest.mark.parametrize("kernel,family", [kw for _, kw in CASES], ids=[i for i, _ in CASES])
def test_the_emulation_passes_every_family(kernel, family, be):
    lc.run(kernel, family, be)


def test_the_bounds_are_the_measured_ones_and_meet_their_conditions():
    l_lse, p_rel, _ = lc.measure_bounds()
    assert l_lse <= lc.L_LSE <= 1.05 * l_lse and lc.L_LSE <= lc.L_LSE_MAX, (l_lse, lc.L_LSE, lc.L_LSE_MAX)
    assert p_rel <= lc.P_REL <= 1.05 * p_rel and lc.P_REL <= lc.P_REL_MAX, (p_rel, lc.P_REL, lc.P_REL_MAX)


def test_the_reference_shows_no_near_tie_where_no_exemption_is_allowed():
    for family in lc.NO_EXEMPTION:
        for V in lc.VS:
            assert not lc.reference_near_ties(lc.build(family, V)), (family, V)


# ---- defects in the sum: which rows does check_lse's bound report? -----------------------------------------------------------------
def off_bound(c, got):
    """Per row: is got (numpy f32 [R]) NaN or outside L_LSE + ulp32(|ref|)?  (what check_lse asserts, row by row)"""
    got = torch.from_numpy(np.asarray(got, dtype=np.float32)).to(F64)
    bad = ~((got - c.lse).abs() <= lc.L_LSE + ref.ulp32(c.lse))
    if bool(bad.any()):
        with pytest.raises(AssertionError):
            lc.check_lse(None, "defect", c, got.to(F32))
    else:
        lc.check_lse(None, "restatement", c, got.to(F32))
    return bad


@pytest.mark.parametrize("V", lc.VS)
def test_the_restatements_pass_unmodified(V):
    for family in lc.FAMILIES:
        if V in lc.family_vs(family):
            c = lc.build(family, V)
            for fn in (lc.lse32_batched, lc.lse32_serial, lambda x: lc.lse32_gather_today(x, guarded=True)):
                assert not bool(off_bound(c, fn(c.x.numpy())).any()), (family, V)


@pytest.mark.parametrize("V", lc.VS)
def test_a_dropped_last_column_is_reported(V):
    c = lc.build("uniform", V)
    assert bool(off_bound(c, lc.lse32_batched(c.x.numpy(), defect="drop_last")).all())
    c = lc.build("one-hot", V)
    bad = off_bound(c, lc.lse32_batched(c.x.numpy(), defect="drop_last"))
    assert bool(bad[torch.tensor(c.onehot) == V - 1].all()) and bool((torch.tensor(c.onehot) == V - 1).any())


@pytest.mark.parametrize("V", [V for V in lc.VS if V >= 2049])
def test_a_column_read_twice_is_reported(V):
    c = lc.build("uniform", V)
    assert bool(off_bound(c, lc.lse32_batched(c.x.numpy(), defect="double_2048")).all())


@pytest.mark.parametrize("V", BIG)
@pytest.mark.parametrize("beyond", [float("nan"), 50.0])
def test_a_column_past_v_read_is_reported(V, beyond):
    c = lc.build("legacy", V)
    x = np.concatenate([c.x.numpy(), np.full((c.R, 1), beyond, dtype=np.float32)], 1)
    got = lc.lse32_batched(x, V=V, defect="read_V")
    assert bool(np.isnan(got).all()) if beyond != beyond else True
    assert bool(off_bound(c, got).all())


@pytest.mark.parametrize("V", lc.VS)
def test_no_max_subtraction_is_reported(V):
    c = lc.build("offset", V)
    got = lc.lse32_batched(c.x.numpy(), defect="no_max")
    rows100 = slice(4, 8)                                  # the rows offset by 100
    assert not bool(np.isfinite(got[rows100]).any()) and bool(off_bound(c, got)[rows100].all())


@pytest.mark.parametrize("V", [V for V in lc.VS if V > 2048])
def test_a_running_max_without_rescaling_is_reported(V):
    c = lc.build("ramp-up", V)                             # (more than one pass: below 2,049 columns there is nothing to rescale)
    assert bool(off_bound(c, lc.lse32_batched(c.x.numpy(), defect="no_rescale")).all())


@pytest.mark.parametrize("V", [V for V in lc.VS if V >= 513])
def test_the_gather_update_without_its_guard_is_reported(V):
    """st_ctc_gather's update as it stood: a thread whose first logit is -inf and a later one finite keeps exp(-inf + inf) = NaN.
    (From 513 columns: at 257 thread 0 owns columns 0 and 256 = V - 1, both masked, and a thread that saw nothing but -inf was
    rescued already.)"""
    c = lc.build("masked", V)
    got = lc.lse32_gather_today(c.x.numpy())
    assert bool(np.isnan(got).any()) and bool(off_bound(c, got).any())
    assert not bool(np.isnan(lc.lse32_gather_today(c.x.numpy(), guarded=True)).any())


@pytest.mark.parametrize("V", lc.VS)
def test_a_neighbours_lse_is_reported(V):
    c = lc.build("peaked", V)
    assert bool(off_bound(c, np.roll(lc.lse32_batched(c.x.numpy()), 1)).all())


# ---- defects in the gradient -------------------------------------------------------------------------------------------------------
GO, DENOM = 32.0, 12.0


def smoothed_gradient(c, conf, sm, zc, target=None, go=GO):
    """The smoothed loss's emulated bf16 gradient in probability units (divided by the NOMINAL scale GO / DENOM), and the reference."""
    R, V = c.R, c.V
    t = c.target if target is None else target
    lse, sums, dl = torch.zeros(R), torch.zeros(4), torch.zeros(R, V, dtype=BF16)
    denom = torch.tensor([DENOM])
    emc.ce_smooth_fwd(c.x, t, lc.IGNORE, conf, sm, zc, lse, sums, denom=denom)
    emc.ce_smooth_bwd(c.x, t, lc.IGNORE, conf, sm, zc, lse, sums, torch.tensor([go]), dl, denom=denom)
    conf0, sm0, zc0 = lc.smooth_cfg(V)
    want = ref.grad_ce(c.x, c.tclamp, conf0, sm0, zc0) * c.valid.to(F64).view(-1, 1)
    q_sum = ref.smoothed_target(R, V, c.tclamp, conf0, sm0, zc0).sum(-1, keepdim=True)
    return dl.to(F64) / (GO / DENOM), want, c.p * q_sum * c.valid.to(F64).view(-1, 1)


GRAD_DEFECTS = {
    "the one-hot subtracted one column off": lambda c, conf, sm, zc: dict(conf=conf, sm=sm, zc=zc, target=torch.where(c.valid, (c.target + 1) % c.V, c.target)),
    "the smoothing mass left on zero_col": lambda c, conf, sm, zc: dict(conf=conf, sm=sm, zc=-1),
    "confidence and smooth swapped": lambda c, conf, sm, zc: dict(conf=sm, sm=conf, zc=zc),
    "the gradient's scale missing": lambda c, conf, sm, zc: dict(conf=conf, sm=sm, zc=zc, go=DENOM),
}


@pytest.mark.parametrize("family", ["legacy", "peaked", "one-hot"])
@pytest.mark.parametrize("V", [5, 257, 4337, 5120])
def test_gradient_defects_are_reported(family, V):
    c = lc.build(family, V)
    conf, sm, zc = lc.smooth_cfg(V)
    lc.check_grad(None, "emulation", c, "dlogits", *smoothed_gradient(c, conf, sm, zc))
    for name, kw in GRAD_DEFECTS.items():
        with pytest.raises(AssertionError, match="off bound"):
            lc.check_grad(None, name, c, "dlogits", *smoothed_gradient(c, **kw(c, conf, sm, zc)))


@pytest.mark.parametrize("V", lc.VS)
def test_a_peaked_targets_gradient_forced_to_fp64_passes(V):
    """At the target of a peaked row p - 1 cancels: fp32 legitimately has 0 (or a few ulp of 1) where fp64 has -V e^-60.  Forcing the fp64
    value in must pass like the fp32 one does: the P_REL p term, not the relative one, carries that element."""
    c = lc.build("peaked", V)
    got, want, p = smoothed_gradient(c, 1.0, 0.0, -1)
    want = ref.grad_ce(c.x, c.tclamp) * c.valid.to(F64).view(-1, 1)
    lc.check_grad(None, "emulation", c, "dlogits", got, want, c.p)
    rows = torch.nonzero(c.x.argmax(-1) == c.target).flatten()
    assert rows.numel() >= 4
    forced = got.clone()
    forced[rows, c.target[rows]] = want[rows, c.target[rows]]
    lc.check_grad(None, "forced", c, "dlogits", forced, want, c.p)
    if V > 5:                                              # (the element is carried by P_REL p alone: the relative term is far too small)
        assert bool((forced[rows[4:], c.target[rows[4:]]].abs() * 2.0 ** -8 < 1e-20).all())


# ---- ties ----------------------------------------------------------------------------------------------------------------------------
def _higher_id_pre_beam(logits, V, ids, lp):
    x = logits[:, :V].float()
    v, i = torch.sort(x.flip(-1), dim=-1, descending=True, stable=True)
    K = ids.shape[1]
    ids.copy_((V - 1 - i[:, :K]).to(torch.int32))
    lp.copy_(v[:, :K] - torch.logsumexp(x, -1, keepdim=True))


@pytest.mark.parametrize("V", lc.VS)
def test_ties_broken_towards_the_higher_id_are_reported(V, be):
    bad = lc.Backend("cpu", "cpu", **{k: v for k, v in be.__dict__.items() if k not in ("name", "dev")})
    bad.beam_pre_beam = _higher_id_pre_beam
    with pytest.raises(AssertionError, match="all candidates tie"):
        lc.run("beam_pre_beam", "uniform", bad, vs=(V,))
    lc.run("beam_pre_beam", "legacy", bad, vs=(V,))        # (without ties the defect is invisible, as it must be)
