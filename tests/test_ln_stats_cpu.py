"""The checks of tests/test_ln_stats_gpu.py, run here on the emulation (tests/_ln_stats.py with a CPU backend): the unmodified
emulation in fp32 passes every family through every implementation's shape - the inputs keep a correct fp32 LayerNorm inside the
bounds - and each defect the checks are there for is reported when it is injected through a backend: a one-pass fp32 variance off
centre, an eps that does not arrive or is another one, the divisor N - 1, xhat without the mean subtracted, a row's rstd taken from its
neighbour, a constant row whose xhat is not zero."""
import pytest
import torch

from tests import _emul as em
from tests import _ln_ref as ref
from tests import _ln_stats as ls

BF16, F32, F64 = torch.bfloat16, torch.float32, torch.float64
CASES = ls.cases()
BY_ID = dict(CASES)


@pytest.mark.parametrize("kw", [kw for _, kw in CASES], ids=[i for i, _ in CASES])
def test_the_emulation_alone_passes(kw):
    report = []
    c = ls.run(kw, ls.CPU, report=report)
    assert len(report) == (2 if c.kind == "chain" else 1)
    # the reference's own figure: far inside the bound (the room the kernels have is L_RSTD itself)
    assert all(r[2] <= 1e-5 for r in report), report


def test_case_list_reaches_every_implementation_and_family():
    by_impl = {}
    for _, kw in CASES:
        by_impl.setdefault(kw["impl"], set()).add(kw["family"])
    assert set(by_impl) == set(ls.IMPLS)
    for iid, fams in by_impl.items():
        impl = ls.IMPLS[iid]
        want = set(ls.F1_FAMILIES) if impl["kind"] == "f1" else set(ls.FAMILIES) - ({"res64"} if impl.get("relu_pe") else set())
        assert fams == want, iid
    assert {i for i, v in ls.IMPLS.items() if v.get("one_pass")} == {"chain-pipe64", "chain-pipe96", "chain512"}
    shapes = {(v["M"], v["N"], v["K"]) for v in ls.IMPLS.values() if v["kind"] == "gemm_ln"}
    # the shapes the issue lists, and the two that reach the 128-row 8-wave kernels of csrc/st_gemm_ln.hip (N = 256: K >= 512 and
    # 16,384 < M <= 32,768; N = 512: M > 8,192 and K >= 1,024)
    assert shapes == {(70, 128, 128), (70, 256, 256), (70, 512, 512), (130, 256, 512), (8250, 256, 80), (8250, 512, 512),
                      (16400, 256, 512), (8250, 512, 1024)}
    assert {(v["d"], v["M"]) for v in ls.IMPLS.values() if v["kind"] == "chain"} == {(256, 70), (256, 8200), (256, 16400), (512, 70)}
    # the split kernel needs two hidden chunks (st_row_chain: split_parts_for): the issue's d_ff 256 case stays, d_ff 512 reaches it
    assert {v.get("d_ff", ls.D_FF) for v in ls.IMPLS.values() if v.get("split")} == {256, 512}


def test_the_families_are_what_their_names_say():
    """|row mean| / row std of the offset families is rho, the spread families' variance is comparable to eps / far below it, the
    64.0 of the residual family survives the rounding, a constant row's every value is 3.0."""
    iid = "gemm_ln-res-n256"
    stat = lambda c: ref.gemm_ln(c.X, c.W, c.bias, c.res, c.gamma, c.beta, c.eps)
    for rho in (8, 32, 128, 512):
        r = stat(ls.build(iid, "offset%d" % rho))
        ratio = (r["mean"].abs() / r["var"].sqrt()).median()
        assert abs(float(ratio) / rho - 1) < 0.05, (rho, float(ratio))
    r = stat(ls.build(iid, "res64"))
    assert 30 < float((r["mean"].abs() / r["var"].sqrt()).median()) < 45
    assert 1e-6 < float(stat(ls.build(iid, "spread1e-3"))["var"].median()) < 1e-5
    assert 1e-10 < float(stat(ls.build(iid, "spread1e-5"))["var"].median()) < 1e-9
    c = ls.build(iid, "offset32-spread1e-3")
    r = stat(c)
    assert abs(float((r["mean"].abs() / r["var"].sqrt()).median()) / 32 - 1) < 0.05 and float(r["var"].median()) < 1e-5
    c = ls.build(iid, "constant")
    r = stat(c)
    assert int(c.const.sum()) == 10 and bool((r["pre"][c.const] == 3.0).all()) and bool((r["var"][c.const] == 0).all())
    assert bool((r["rstd"][c.const] == 1e-6 ** -0.5).all()) and bool((r["var"][~c.const] > 1).all())
    assert ls.build(iid, "spread1e-3-eps1e-5").eps == 1e-5
    # a chain: the offset reaches both LayerNorms, the spread the first only
    c = ls.build("chain-32row", "offset32-spread1e-3")
    s1, s2 = ls.sigmas("chain-32row")
    base = ls._centred_operands("chain-32row")
    assert abs(float((c.b2 - base.b2).mean()) / (32 * s2) - 1) < 1e-3 and abs(float((c.bo - 1e-3 * base.bo).mean()) / (32e-3 * s1) - 1) < 1e-3


# ---- defects, injected through a backend -----------------------------------------------------------------------------------------------
def _defective(kind):
    """tests._emul.gemm_ln with one defect."""

    def gemm_ln(X, W, bias, res, gamma, beta, out, xhat, rstd, eps=1e-6, relu=False, pe=None, pos=None, pre=None, drop=None,
                drop_where=0, dtype=F32):
        v = X.to(dtype) @ W.to(dtype).t() + bias.to(dtype)
        if relu:
            v = torch.relu(v)
        if res is not None:
            v = v + res.to(dtype)
        n = v.shape[1]
        mu = v.mean(-1, keepdim=True)
        if kind == "one-pass":                 # var = max(sum v^2 / N - mean^2, 0) in fp32, 8 partial sums of N / 8 columns
            q = (v * v).view(v.shape[0], 8, -1).sum(-1).sum(-1, keepdim=True)
            var = (q / n - mu * mu).clamp_min(0)
        elif kind == "n-1":
            var = ((v - mu) ** 2).sum(-1, keepdim=True) / (n - 1)
        else:
            var = ((v - mu) ** 2).mean(-1, keepdim=True)
        if kind == "no-eps":
            rs = torch.rsqrt(var)
        elif kind == "eps-1e-5":               # a kernel with its own eps
            rs = torch.rsqrt(var + 1e-5)
        else:
            rs = torch.rsqrt(var + eps)
        if kind == "neighbour":
            rs = rs.clone()
            rs[-1] = rs[-2]
        h = (v if kind == "mean-kept" else v - mu) * rs
        if kind == "constant-not-zero":       # what cancellation leaves of a constant row: one part in 2^20 of the value
            h = h + (var == 0) * v * 2.0 ** -20 * rs
        y = h * gamma.to(dtype) + beta.to(dtype)
        if pe is not None:
            y = y + pe[pos.long()].to(dtype)
        out.copy_(y.to(BF16))
        xhat.copy_(h.to(BF16))
        rstd.copy_(rs.squeeze(-1))
        if pre is not None:
            pre.copy_(v.to(BF16))
        return out
    return gemm_ln


def _reported(cid, kind, match="bound violated"):
    with pytest.raises(AssertionError, match=match):
        ls.run(BY_ID[cid], ls.cpu_backend(_defective(kind)))


def _figures(cid, kind):
    report = []
    ls.run(BY_ID[cid], ls.cpu_backend(_defective(kind)), report=report, asserted=False)
    return [r[2] for r in report]


@pytest.mark.parametrize("cid", [i for i, kw in CASES if kw["impl"] in ("gemm_ln-res-n256", "chain-32row", "chain512", "gemm_ln-relu_pe")])
def test_the_harness_of_the_injections_without_a_defect_passes(cid):
    ls.run(BY_ID[cid], ls.cpu_backend(_defective(None)))


@pytest.mark.parametrize("impl", ["chain-32row", "chain-split-dff512", "chain512", "attn_f1-short-keys"])
def test_a_defect_injected_through_a_backend_reaches_the_emulated_chains(impl):
    """The backend swaps tests._emul.gemm_ln while the emulated chain runs: the divisor N - 1 must move rstd of EVERY LayerNorm
    stage of a chain by 1 / (2 N) - were the swap ever to miss the chains, the figures would stay at 1e-7."""
    clean, moved = [], []
    ls.run(BY_ID["%s-centred" % impl], ls.CPU, report=clean)
    ls.run(BY_ID["%s-centred" % impl], ls.cpu_backend(_defective("n-1")), report=moved, asserted=False)
    n = ls.IMPLS[impl].get("d", 256)
    assert len(clean) == len(moved) == (1 if impl.startswith("attn_f1") else 2)
    for c, m in zip(clean, moved):
        assert c[2] < 1e-6 and 0.45 / n < m[2] < 0.55 / n, (c, m)


@pytest.mark.parametrize("impl,family", [(i, f) for i in ("gemm_ln-res-n128", "gemm_ln-res-n256", "gemm_ln-res-n512", "chain-32row", "chain512")
                                         for f in ("offset32", "offset128", "offset512", "res64")]
                         + [(i, "offset32-spread1e-3") for i in ("gemm_ln-tiles-n256", "gemm_ln-tiles-n512", "chain-pipe64")])
def test_reports_an_fp32_one_pass_variance_off_centre(impl, family):
    """2.4e-4 at rho = 32, 4.7e-3 at 128 over thousands of rows; the worst of 70 rows at rho = 32 still stands at 1.3e-4 or more.  (With
    a variance of 3 eps, eps damps the loss: that family is held to the shapes with thousands of rows.)"""
    _reported("%s-%s" % (impl, family), "one-pass", "rstd bound violated")


@pytest.mark.parametrize("impl", ["gemm_ln-res-n128", "gemm_ln-res-n256", "gemm_ln-res-n512", "chain-32row", "chain512"])
def test_an_fp32_one_pass_variance_hides_near_the_centre(impl):
    """... and at rho = 0 and 8 it passes (at rho = 8: 1.0e-5 over these 70 rows, 1.6e-5 over the cases of 8,200 rows, 1.8e-5 in the
    restatement of tests/LOCAL_BOUNDS.md over 4,096 - the 2^-24 rho^2 law) - why the families at rho >= 32 exist; the
    tiny-spread rows at rho = 0 and the constant rows (whose sums are exact) pass too."""
    for family in ("centred", "offset8", "spread1e-3", "spread1e-5", "constant"):
        ls.run(BY_ID["%s-%s" % (impl, family)], ls.cpu_backend(_defective("one-pass")))
    assert max(_figures("%s-offset8" % impl, "one-pass")) < ls.L_RSTD / 2
    f32, f128 = max(_figures("%s-offset32" % impl, "one-pass")), max(_figures("%s-offset128" % impl, "one-pass"))
    assert ls.L_RSTD < f32 < f128, (f32, f128)


@pytest.mark.parametrize("impl,family", [(i, f) for i in ("gemm_ln-res-n256", "gemm_ln-tiles-n512", "chain-32row", "chain512")
                                         for f in ("spread1e-3", "spread1e-5")] + [("attn_f1-short-keys", "spread1e-3")])
@pytest.mark.parametrize("kind", ["no-eps", "eps-1e-5"])
def test_reports_an_eps_that_does_not_arrive_or_is_another_one(impl, family, kind):
    _reported("%s-%s" % (impl, family), kind)


def test_reports_an_eps_of_1e_6_where_1e_5_is_asked_for():
    def gemm_ln(*a, **kw):
        return em.gemm_ln(*a, **dict(kw, eps=1e-6))
    with pytest.raises(AssertionError, match="rstd bound violated"):
        ls.run(BY_ID["gemm_ln-res-n256-spread1e-3-eps1e-5"], ls.cpu_backend(gemm_ln))


def test_a_wrong_eps_is_invisible_on_centred_rows():
    """... at a variance of 3 neither shows: 1.7e-7 (no eps) and 1.5e-6 (1e-5 for 1e-6) of rstd."""
    for kind in ("no-eps", "eps-1e-5"):
        assert max(_figures("gemm_ln-res-n256-centred", kind)) < 1e-5


@pytest.mark.parametrize("impl,low", [("gemm_ln-res-n128", 3.8e-3), ("gemm_ln-res-n256", 1.9e-3), ("gemm_ln-res-n512", 9.6e-4), ("chain-32row", 1.9e-3),
                                      ("chain512", 9.6e-4), ("gemm_ln-tiles-n256", 1.9e-3)])
def test_reports_the_divisor_n_minus_1(impl, low):
    """rstd moves by 1 / (2 N): 3.9e-3 / 2.0e-3 / 9.8e-4 at N = 128 / 256 / 512 - at or under the 2e-3 rstd is held to elsewhere."""
    _reported("%s-centred" % impl, "n-1", "rstd bound violated")
    assert low < max(_figures("%s-centred" % impl, "n-1")) < low * 1.1


@pytest.mark.parametrize("cid", ["gemm_ln-res-n256-centred", "gemm_ln-res-n256-offset8", "chain-32row-offset512", "gemm_ln-relu_pe-centred"])
def test_reports_xhat_without_the_mean_subtracted(cid):
    _reported(cid, "mean-kept", "rel-L2|local bound")


@pytest.mark.parametrize("cid", ["gemm_ln-res-n256-centred", "gemm_ln-tiles-n256-offset128", "chain-32row-spread1e-3", "chain512-centred"])
def test_reports_one_rows_rstd_taken_from_its_neighbour(cid):
    _reported(cid, "neighbour", "rstd bound violated: 1 of")


@pytest.mark.parametrize("impl", ["gemm_ln-res-n128", "gemm_ln-res-n512", "gemm_ln-relu_pe", "chain-32row", "chain512"])
def test_reports_a_constant_row_whose_xhat_is_not_zero(impl):
    _reported("%s-constant" % impl, "constant-not-zero", "xhat of a constant row is not zero")


def test_reports_a_write_outside_the_window_and_a_row_never_written():
    def stray(*a, **kw):
        em.gemm_ln(*a, **kw)
        a[8]._base[0, 0] = 0.0                  # rstd's guard in front of the window
    with pytest.raises(AssertionError, match="written outside"):
        ls.run(BY_ID["gemm_ln-res-n256-centred"], ls.cpu_backend(stray))

    def skip_row(*a, **kw):
        keep = a[7][5].clone()
        em.gemm_ln(*a, **kw)
        a[7][5] = keep
    with pytest.raises(AssertionError, match="non-finite"):
        ls.run(BY_ID["gemm_ln-res-n256-centred"], ls.cpu_backend(skip_row))
