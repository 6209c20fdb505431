"""The checks of tests/test_lnbwd_fp64_gpu.py, run here on the emulation (tests/_lnbwd_cases.py with a CPU backend): the unmodified
emulation in fp32 passes every family through every kernel's shape - under two summation orders, whose figures times three are the
bounds in force - and each defect the checks are there for is reported when it is injected: Ores left out of delta, delta summed from
the unrounded dctx, a chain's dbias summed before the rounding, the xhat mean(g xhat) term missing, gamma applied after the means, the
divisor N - 1, a row's rstd taken from its neighbour (reported row by row against the row's own norm, and NOT under the floor the other
kernel tests use: the pair is why the rstd-wide family exists), a small-rstd row left unwritten, mask_scale dropped, -0.0 or a
subnormal mask value treated the other way, a dead row that contributes to a column sum."""
import contextlib
import io

import pytest
import torch

from tests import _emul as em
from tests import _lnbwd_cases as lc
from tests import _lnbwd_ref as ref
from tests._local import local_figures

BF16, F32, F64 = torch.bfloat16, torch.float32, torch.float64
# (the deferred fold is the GPU wrapper's business: on the emulation those cases repeat chain-pipe64 / chain-pipe96)
CASES = [(i, kw) for i, kw in lc.cases() if not lc.IMPLS[kw["impl"]].get("deferred")]
COLS = {"dga": "dgamma", "dgb": "dgamma", "dba": "dbeta", "dbb": "dbeta", "dbia": "dbias", "dbib": "dbias"}


@pytest.mark.parametrize("be", [lc.CPU, lc.SERIAL], ids=["emulation", "serial"])
@pytest.mark.parametrize("kw", [kw for _, kw in CASES], ids=[i for i, _ in CASES])
def test_the_emulation_alone_passes(kw, be):
    """... and stays a factor three inside every bound that is 3 x its figure (a bound capped by the one already in force: inside it);
    the fused kernels' common-mode rows below a third of the row bound - the rule CM_FUSED was chosen by."""
    report = []
    c = lc.run(kw, be, report=report)
    kind = c.kind
    for _, nm, f, bound in report:
        if "element" in f:
            q = COLS.get(nm, nm)
            capped = nm != "delta" and bound == lc.IN_FORCE[kind][q]
            assert f["element"] <= (bound if capped else bound / 3 * 1.02), (nm, f, bound)
        elif c.family == "common-mode" and kind != "ln_bwd":
            assert f["row"] <= lc.L_BF16 / 3, (nm, f)


def test_no_bound_is_above_the_ones_in_force():
    for kind, b in lc.L_COL.items():
        for q, v in b.items():
            assert v <= lc.IN_FORCE[kind][q], (kind, q)
    assert lc.L_DELTA <= 2e-3 and lc.L_BF16 == 1e-2


def test_case_list_reaches_every_kernel_and_family():
    by_impl = {}
    for _, kw in lc.cases():
        by_impl.setdefault(kw["impl"], set()).add(kw["family"])
    assert set(by_impl) == set(lc.IMPLS)
    for iid, fams in by_impl.items():
        assert fams == set(lc.FAMILIES) | ({"mask-edge"} if lc.IMPLS[iid].get("mask") else set()), iid
    shapes = lambda kind, *keys: {tuple(v.get(k) for k in keys) for v in lc.IMPLS.values() if v["kind"] == kind}
    # st_ln_bwd: 256 workgroups x 16 rows = 4,096 rows per trip at N = 256
    assert shapes("ln_bwd", "M", "N") == {(70, 128), (70, 256), (70, 512), (4100, 256)}
    # st_gemm_lnbwd's dispatch: N = 256, Kc >= 512, 16,384 < M <= 32,768; N = 512, M > 8,192, Kc < 1,024 / >= 1,024
    assert shapes("gemm_lnbwd", "M", "N", "K") == {(70, 128, 128), (70, 256, 256), (70, 512, 512), (16400, 256, 512), (8200, 512, 512),
                                                   (8200, 512, 1024)}
    assert shapes("chain", "M", "parts") == {(70, "head3+ffn+tail"), (8200, "head3+ffn+tail"), (16400, "head3+ffn+tail"),
                                             (70, "head0+ffn+tail"), (70, "ffn+tail"), (70, "tail")}
    assert lc.D_FF // 256 == 2                                      # the smallest d_ff with more than one hidden chunk: the split kernel runs


def test_the_families_are_what_their_names_say():
    c = lc.build("ln_bwd-stride-n256-mask", "rstd-wide")
    x = c.xhat.double()
    assert float(x.mean(1).abs().max()) < 2e-3 and float((x.pow(2).mean(1) - 1).abs().max()) < 5e-3          # normalised, then rounded
    assert float(c.rstd.min()) == pytest.approx(1e-3, rel=1e-5) and float(c.rstd.max()) == pytest.approx(1e3, rel=1e-5)
    lg = c.rstd.double().log10()
    assert float(lg[:64].max() - lg[:64].min()) > 5                               # the first 64 rows alone span more than five of the six decades
    # rows the floor of check_local cannot see: their norm is below 0.25 % of the typical one (a wrong row stays under 1e-2 x 0.25)
    r = ref.ln_bwd(c.dy, c.xhat, c.rstd, c.gamma, mask=c.mask, mask_scale=c.mask_scale)["dx"].norm(dim=1)
    frac = float((r < 0.0025 * r.pow(2).mean().sqrt()).double().mean())
    assert 0.3 < frac < 0.6, frac                                                   # (45 %: every row whose rstd is below ~0.7)
    leg = lc.build("ln_bwd-stride-n256", "legacy")
    r = ref.ln_bwd(leg.dy, leg.xhat, leg.rstd, leg.gamma)["dx"].norm(dim=1)
    assert float(r.min() / r.pow(2).mean().sqrt()) > 0.25                          # ... and today's inputs have no small row at all
    # common mode: dy gamma is a + b xhat + noise, for the operand and for the fused kernels' internal dy
    c = lc.build("ln_bwd-n256", "common-mode")
    t = c.dy.double() * c.gamma.double()
    a, b, sigma = lc.CM_OPERAND
    assert abs(float(t.mean()) / a - 1) < 0.01 and abs(float((t * c.xhat.double()).mean()) / b - 1) < 0.02
    assert float((t - a - b * c.xhat.double()).std()) < 4 * sigma                  # sigma and the bf16 rounding of an operand near 64
    c = lc.build("gemm_lnbwd-n256", "common-mode")
    t = ref.dgrad(c.dY, c.W, c.aux) * c.gamma.double()
    a, b, sigma = lc.CM_FUSED
    assert abs(float(t.mean()) / a - 1) < 0.02 and abs(float((t * c.xhat.double()).mean()) / b - 1) < 0.05
    assert lc.CM_FUSED in lc.CM_CANDIDATES
    c = lc.build("gemm_lnbwd-n256", "gamma-hard")
    gm = c.gamma
    assert int((gm == 0).sum()) == 3 and 0.15 < float((gm < 0).float().mean()) < 0.45
    assert float(gm.abs().max()) > 8 and float(gm[gm != 0].abs().min()) < 0.125
    c = lc.build("chain-32row", "dead-rows")
    assert int(c.dead.sum()) == 10 and all(float(t[c.dead].float().abs().max()) == 0 for t in (c.dP, c.G, c.DS))
    c = lc.build("ln_bwd-n256-mask", "mask-edge")
    bits = c.mask.view(torch.int16)
    for v in (0, -32768, 1, -32767):
        assert int((bits == v).sum()) == c.M * c.N // 8 or abs(int((bits == v).sum()) - c.M * c.N // 8) < c.N
    assert float(c.mask.double()[bits == 1].min()) > 0 and float(c.mask.double()[bits == -32767].max()) < 0


def test_delta_bound_sits_below_what_leaving_ores_out_moves():
    """Ores is 2^-9 of O: left out, the worst element of delta moves by 1.2e-2 or more of max(|delta|, 0.25 x typical) in every case -
    600 times L_DELTA."""
    for _, kw in CASES:
        c = lc.build(**kw)
        if c.kind != "chain" or not c.has_tail or c.M > 100:
            continue
        dctx = lc.launch(c, lc.CPU)["dctx"].view
        ratio = local_figures(ref.delta_of(dctx, c.O, None), ref.delta_of(dctx, c.O, c.Ores))[0][1]
        assert float(ratio.max()) > 1e-2 > 100 * lc.L_DELTA, (c.id, float(ratio.max()))


# ---- defects ----------------------------------------------------------------------------------------------------------------------------
def _defective(kind, row=None):
    """tests._emul.ln_bwd with one defect."""

    def ln_bwd(dy, xhat, rstd, gamma, dx, dgamma=None, dbeta=None, dbias=None, mask=None, drop=None, mask_scale=1.0, dtype=F32,
               dbias_rounded=False):
        d, xh = dy.to(dtype), xhat.to(dtype)
        if em._on(drop):
            d = d * em.keep_rc(drop, torch.arange(d.shape[0]), torch.arange(d.shape[1]), d.shape[1]) * drop.scale
        n = d.shape[1]
        div = n - 1 if kind == "n-1" else n
        rs = rstd.to(dtype).clone()
        if kind == "neighbour":
            rs[row] = rs[row + 1]
        if kind == "gamma-late":              # gamma after the means instead of before
            v = rs.unsqueeze(-1) * gamma.to(dtype) * (d - d.sum(-1, keepdim=True) / div - xh * ((d * xh).sum(-1, keepdim=True) / div))
        else:
            g = d * gamma.to(dtype)
            m2 = 0.0 if kind == "no-xhat-term" else (g * xh).sum(-1, keepdim=True) / div
            v = rs.unsqueeze(-1) * (g - g.sum(-1, keepdim=True) / div - xh * m2)
        if mask is not None:
            mk = mask.to(dtype)
            if kind == "zero-kept":           # -0.0 and +0.0 treated as positive
                keep = mk >= 0
            elif kind == "subnormal-flushed":   # a subnormal treated as zero
                keep = mk >= 2.0 ** -126
            else:
                keep = mk > 0
            v = v * keep * (1.0 if kind == "no-mask-scale" else mask_scale)
        dx.copy_(v.to(BF16))
        if kind == "unwritten":
            dx[row] = 0
        if dgamma is not None:
            dgamma += (d * xh).sum(0)
        if dbeta is not None:
            dbeta += d.sum(0)
        if dbias is not None:
            dbias += dx.to(dtype).sum(0) if dbias_rounded else v.sum(0)
        return dx
    return ln_bwd


def _run(impl, family, ln_bwd=None, tamper=None, own_rows=True):
    with contextlib.redirect_stdout(io.StringIO()):
        lc.run(dict(impl=impl, family=family), lc.cpu_backend(ln_bwd, tamper), own_rows=own_rows)


def _reported(impl, family, match, ln_bwd=None, tamper=None, own_rows=True):
    _run(impl, family, own_rows=own_rows)             # (the case passes without the defect)
    with pytest.raises(AssertionError, match=match):
        _run(impl, family, ln_bwd, tamper, own_rows)


CHAINS = ["chain-32row", "chain-split", "chain-ffn+tail", "chain-tail", "chain-pipe64"]


@pytest.mark.parametrize("impl", CHAINS)
@pytest.mark.parametrize("family", ["legacy", "rstd-wide"])
def test_ores_left_out_of_delta_is_reported(impl, family):
    def tamper(c, gd):
        gd["delta"].view.copy_(ref.delta_of(gd["dctx"].view, c.O, None))
    _reported(impl, family, "delta: local bound violated", tamper=tamper)


@pytest.mark.parametrize("impl", CHAINS)
def test_delta_from_the_unrounded_dctx_is_reported(impl):
    def tamper(c, gd):
        ds = gd["ds_b"].view if c.has_ffn else c.DS
        gd["delta"].view.copy_(ref.delta_of(ds.float() @ c.wo.float(), c.O, c.Ores))
    _reported(impl, "legacy", "delta: local bound violated", tamper=tamper)


@pytest.mark.parametrize("impl,stage", [("chain-32row", "a"), ("chain-32row", "b"), ("chain-pipe64", "a"), ("chain-pipe64", "b"),
                                        ("gemm_lnbwd-n256", "x")])
def test_dbias_summed_before_the_rounding_is_reported(impl, stage):
    """The fused kernels sum dx AS STORED: the fp32 values before their rounding give another sum - by 1.5e-2 to 2.2e-2 of the worst
    entry, hundreds of times the bound against the own-output sum."""
    def tamper(c, gd):
        if stage == "x":
            r = ref.gemm_lnbwd(c.dY, c.W, c.aux, c.xhat, c.rstd, c.gamma)
            gd["dbias"].view.copy_(r["dbias"] + 1.0)
        elif stage == "a":
            r = ref.gemm_lnbwd(c.dP, c.wp, c.G, c.xa, c.ra, c.ga)
            gd["dbia"].view.copy_(r["dbias"] + lc.CHAIN_INIT["dbia"])
        else:
            r = ref.gemm_lnbwd(gd["dH"].view, c.w1, gd["ds_a"].view, c.xb, c.rb, c.gb)
            gd["dbib"].view.copy_(r["dbias"] + lc.CHAIN_INIT["dbib"])
    _reported(impl, "legacy", "%s: local bound violated" % {"x": "dbias", "a": "dbia", "b": "dbib"}[stage], tamper=tamper)


@pytest.mark.parametrize("impl,out", [("ln_bwd-n128", "dx"), ("ln_bwd-n512", "dx"), ("gemm_lnbwd-n256", "dx"), ("chain-32row", "ds_a")])
@pytest.mark.parametrize("family", ["rstd-wide", "common-mode", "gamma-hard"])
def test_missing_xhat_term_is_reported(impl, out, family):
    _reported(impl, family, out, ln_bwd=_defective("no-xhat-term"))


@pytest.mark.parametrize("impl,out", [("ln_bwd-n256", "dx"), ("gemm_lnbwd-n512", "dx"), ("chain-ffn+tail", "ds_b")])
def test_gamma_after_the_means_is_reported_on_the_hard_gamma(impl, out):
    _reported(impl, "gamma-hard", out, ln_bwd=_defective("gamma-late"))


def test_gamma_after_the_means_on_todays_inputs():
    """Today's inputs see it too: gamma = 1 +- 0.2 puts the worst row 0.14 - 0.15 of its norm off at N = 128, 256 and 512 (xhat is not
    normalised there: the two means are large); the hard gamma stands at 0.3 - 0.6 of a row, the common mode at hundreds."""
    for n in (128, 256, 512):
        with pytest.raises(AssertionError, match="dx"):
            _run("ln_bwd-n%d" % n, "legacy", ln_bwd=_defective("gamma-late"))


@pytest.mark.parametrize("impl,out", [("ln_bwd-n128", "dx"), ("ln_bwd-n256", "dx"), ("ln_bwd-n512", "dx"), ("gemm_lnbwd-n256", "dx"),
                                      ("chain-head0", "ds_a")])
def test_divisor_n_minus_one_is_reported_on_the_common_mode(impl, out):
    _reported(impl, "common-mode", out, ln_bwd=_defective("n-1"))
    # the common mode puts the worst row 1.2 - 4.2 of its norm off; on today's inputs the means are 1 / sqrt(N) of a row and 1 / N of
    # that is invisible in dx (3e-3 of the worst row: the rounding) - only st_ln_bwd's dbias at N = 128 shows it (6.7e-3 against 5e-3)
    if impl != "ln_bwd-n128":
        _run(impl, "legacy", ln_bwd=_defective("n-1"))


def _small_pair(c):
    """A row whose rstd and whose neighbour's are both below 0.3 and a factor two or more apart."""
    rs = (c.rstd if c.kind != "chain" else c.ra).double()
    ok = (rs[:-1] < 0.3) & (rs[1:] < 0.3) & ((rs[:-1] / rs[1:]).log2().abs() > 1)
    return int(torch.nonzero(ok)[0])


@pytest.mark.parametrize("impl,out", [("ln_bwd-n256", "dx"), ("ln_bwd-stride-n256", "dx"), ("gemm_lnbwd-n256", "dx"),
                                      ("gemm_lnbwd-tiles-n512", "dx"), ("chain-32row", "ds_a")])
def test_neighbour_rstd_is_reported_row_by_row_and_missed_by_the_floor(impl, out):
    row = _small_pair(lc.build(impl, "rstd-wide"))
    _reported(impl, "rstd-wide", "%s: local bound violated: 1 of \\d+ rows fail, worst row %d:" % (out, row), ln_bwd=_defective("neighbour", row))
    _run(impl, "rstd-wide", ln_bwd=_defective("neighbour", row), own_rows=False)          # today's floor: the wrong row passes


@pytest.mark.parametrize("impl,out", [("ln_bwd-n256", "dx"), ("gemm_lnbwd-tall-n256", "dx"), ("chain-split", "ds_a")])
def test_small_rstd_row_left_unwritten_is_reported(impl, out):
    """(into a buffer that held zeros: in the guards' NaN it would be a non-finite output)"""
    c = lc.build(impl, "rstd-wide")
    row = int((c.rstd if c.kind != "chain" else c.ra).argmin())
    _reported(impl, "rstd-wide", "%s: local bound violated: 1 of \\d+ rows fail, worst row %d:" % (out, row), ln_bwd=_defective("unwritten", row))
    _run(impl, "rstd-wide", ln_bwd=_defective("unwritten", row), own_rows=False)


def test_mask_scale_dropped_is_reported():
    _reported("ln_bwd-n256-mask", "legacy", "dx", ln_bwd=_defective("no-mask-scale"))

    def tamper(c, gd):                      # the chain's masked dgrad without its 1 / (1 - p)
        gd["dH"].view.copy_((gd["dH"].view.float() / c.mask_scale).to(BF16))
    _reported("chain-32row", "legacy", "dH", tamper=tamper)


@pytest.mark.parametrize("n", [128, 256, 512])
def test_mask_edge_values_treated_the_other_way_are_reported(n):
    impl = "ln_bwd-n%d-mask" % n
    _reported(impl, "mask-edge", "not zero where mask <= 0", ln_bwd=_defective("zero-kept"))
    _reported(impl, "mask-edge", "dx: (rel-L2|local bound violated)", ln_bwd=_defective("subnormal-flushed"))
    _run(impl, "legacy", ln_bwd=_defective("zero-kept"))           # ordinary mask values: neither shows
    _run(impl, "legacy", ln_bwd=_defective("subnormal-flushed"))


@pytest.mark.parametrize("impl", ["ln_bwd-n256", "ln_bwd-stride-n256", "gemm_lnbwd-n256", "chain-32row", "chain-pipe64"])
def test_dead_row_that_contributes_to_a_column_sum_is_reported(impl):
    """A dead row handled with the row above's dy still in the registers: one row's worth added to dgamma and dbeta."""
    def tamper(c, gd):
        r = int(torch.nonzero(c.dead)[0])
        if c.kind == "ln_bwd":
            dy, xh, names = c.dy[r - 1].float(), c.xhat[r].float(), ("dgamma", "dbeta")
        elif c.kind == "gemm_lnbwd":
            dy, xh, names = ref.dgrad(c.dY, c.W, c.aux)[r - 1].float(), c.xhat[r].float(), ("dgamma", "dbeta")
        else:
            dy, xh, names = ref.dgrad(c.dP, c.wp, c.G)[r - 1].float(), c.xa[r].float(), ("dga", "dba")
        gd[names[0]].view.add_(dy * xh)
        gd[names[1]].view.add_(dy)
    _reported(impl, "dead-rows", "(dgamma|dga): local bound violated", tamper=tamper)


def test_dead_row_that_is_not_zero_is_reported():
    def tamper(c, gd):
        gd["dctx"].view[int(torch.nonzero(c.dead)[0]), 7] = 2.0 ** -100
    _reported("chain-32row", "dead-rows", "a dead row is not zero", tamper=tamper)

    def tamper_delta(c, gd):
        gd["delta"].view[c.M + int(torch.nonzero(c.dead)[0])] = 1e-30
    _reported("chain-32row", "dead-rows", "a dead row's delta is not zero", tamper=tamper_delta)
