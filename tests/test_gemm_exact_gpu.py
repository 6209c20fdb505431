"""-m gpu: the GEMM family bit for bit.  Operands are small integers (tests/_exact.py: the recipe), so every product and every
partial sum is exact in fp32 in any order; the fp32 outputs must EQUAL the fp64 reference and the bf16 outputs its one
round-to-nearest-even, whatever the tiling, the wave-group split, the split-K merge or the order of the atomics.  One case per
dispatch variant at its smallest shape; every output inside guards, every operand inside NaN; every comparison is
assert_same_bits.  tests/test_gemm_exact_cpu.py holds the recipe's premise and shows what these cases see that the bounds of
tests/test_kernels_gpu.py do not."""
import pytest
import torch

from st_amd import native as nv
from tests import _exact as ex
from tests._local import Guarded, guarded_input

pytestmark = pytest.mark.gpu
BF16, F32, F64, I32 = torch.bfloat16, torch.float32, torch.float64, torch.int32


def GO(rows, cols, dtype=BF16, contiguous=False):
    lo_hi = (0, 0) if contiguous else (64, 64)
    pad_rows = 3 if (3 * (sum(lo_hi) + cols)) % 8 == 0 else 4          # (N = 132: Guarded wants the window to start on 8 elements)
    return Guarded(rows, cols, dtype, "cuda", pad_rows=pad_rows, pad_cols=lo_hi)


def GV(n, dtype=F32):
    return Guarded.vec(n, dtype, "cuda")


def GI(t, **kw):
    return None if t is None else guarded_input(t, "cuda", **kw)


def cu(t):
    return None if t is None else t.cuda()


def drop_site(salt):
    return nv.Drop(torch.tensor([ex.DROP_SEED], dtype=I32, device="cuda"), salt, ex.DROP_P)


def holding(t, dtype=F32):
    """A guarded accumulator that already holds ``t``."""
    gd = GV(t.numel(), dtype) if t.dim() == 1 else GO(t.shape[0], t.shape[1], dtype)
    gd.view.copy_(t)
    return gd


# ---- a. the premise: the bf16 MFMA keeps integer sums exact (first in the file: everything below rests on it) ----------------
@pytest.mark.parametrize("lo,hi", [(-4, 4), (-128, 127)])
def test_mfma_keeps_integer_sums_exact(lo, hi):
    A, Bt = ex.mfma_operands(lo, hi)
    ex.assert_exact_fp32(A.to(F64).abs() @ Bt.to(F64).abs().t(), "mfma probe")
    gd = GO(32, 32, F32, contiguous=True)
    nv.probe_mfma(GI(A, pad_cols=(0, 0)), GI(Bt, pad_cols=(0, 0)), gd.view)
    torch.cuda.synchronize()
    ex.assert_same_bits(gd.view, A.to(F64) @ Bt.to(F64).t(), "mfma 32x32x16 [%d, %d]" % (lo, hi), tile=(32, 32))
    gd.assert_intact("mfma probe")


# ---- b. st_gemm forward (0, 0) ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", ex.FWD_CASES, ids=ex.fwd_id)
def test_gemm_forward_exact(case):
    what = "gemm fwd " + ex.fwd_id(case)
    bt = ex.build_fwd(case)
    ex.check_conds(bt, what)
    M, N, K = case["shape"]
    gd = GO(M, N, F32 if case["epi"] == ex.EPI_F32 else BF16)
    nv.gemm(GI(bt.ops["X"]), GI(bt.ops["W"]), gd.view, bias=GI(bt.ops["bias"]), epi=case["epi"], drop=drop_site(11) if case["drop"] else None)
    ex.assert_same_bits(gd.view, bt.refs["D"], what)
    gd.assert_intact(what)


# ---- c. st_gemm dgrad (0, 1) --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", ex.DGRAD_CASES, ids=ex.dgrad_id)
def test_gemm_dgrad_exact(case):
    what = "gemm dgrad " + ex.dgrad_id(case)
    bt = ex.build_dgrad(case)
    ex.check_conds(bt, what)
    M, C, N = case["shape"]
    epi, o = case["epi"], bt.ops
    gd, gdd, kw = GO(M, N), None, {}
    if epi == ex.EPI_BF16_MASK:
        kw = dict(aux=GI(o["aux"]), drop=drop_site(11) if case["scale"] == 2.0 else None)
    elif epi == ex.EPI_BF16_ADD:
        if case["alias"]:          # in place, as functional.py accumulates the cross-attention K/V input gradient: aux IS the output
            gd.view.copy_(o["aux"])
            kw = dict(aux=gd.view)
        else:
            kw = dict(aux=GI(o["aux"]))
    elif epi == ex.EPI_BF16_DELTA:
        gdd = GV((N // case["hd"]) * M)
        kw = dict(aux=GI(o["aux"]), aux2=GI(o["aux2"]), delta=gdd.view, head_dim=case["hd"])
    nv.gemm(GI(o["dy"]), GI(o["W"]), gd.view, bias=GI(o["bias"]), epi=epi, y_cmajor=True, **kw)
    ex.assert_same_bits(gd.view, bt.refs["D"], what, alternatives=bt.alts.get("D"))
    gd.assert_intact(what)
    if gdd is not None:
        ex.assert_same_bits(gdd.view, bt.refs["delta"], what + ": delta", tile=(1, M), alternatives=bt.alts["delta"])
        gdd.assert_intact(what + ": delta")


# ---- d. st_gemm wgrad (1, 1) --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", ex.WGRAD_CASES, ids=ex.wgrad_id)
def test_gemm_wgrad_exact(case):
    """dW += dy^T x on top of an existing gradient: split-K with fp32 atomics (in any order: exact), the transposed coalesced
    store, and the fused bias gradient."""
    what = "gemm wgrad " + ex.wgrad_id(case)
    bt = ex.build_wgrad(case)
    ex.check_conds(bt, what)
    o, N, sp = bt.ops, case["out"][0], case["splits"]
    gd = holding(o["init"])
    nv.gemm(GI(o["dy"]), GI(o["x"]), gd.view, epi=nv.EPI_F32_ATOMIC, x_cmajor=True, y_cmajor=True, splits=sp, m=N)
    ex.assert_same_bits(gd.view, bt.refs["dW"], what + " ATOMIC")
    gd.assert_intact(what + " ATOMIC")
    gd = holding(o["init"])
    nv.gemm(GI(o["x"]), GI(o["dy"]), gd.view, epi=nv.EPI_F32_ATOMIC_T, x_cmajor=True, y_cmajor=True, splits=sp, n=N)
    ex.assert_same_bits(gd.view, bt.refs["dW"], what + " ATOMIC_T")
    gd.assert_intact(what + " ATOMIC_T")
    gd, gb = holding(o["init"]), holding(o["b0"])
    nv.gemm(GI(o["x"]), GI(o["dy"]), gd.view, bias=gb.view, epi=nv.EPI_F32_ATOMIC_T, x_cmajor=True, y_cmajor=True, splits=sp, n=N)
    ex.assert_same_bits(gd.view, bt.refs["dW"], what + " ATOMIC_T + bias gradient")
    ex.assert_same_bits(gb.view, bt.refs["db"], what + ": bias gradient", tile=(1, 128))
    gd.assert_intact(what + " ATOMIC_T + bias gradient"), gb.assert_intact(what + ": bias gradient")


# ---- e. st_gemm_splitk --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", ex.SPLITK_CASES, ids=ex.splitk_id)
def test_gemm_splitk_exact(case):
    what = "gemm_splitk " + ex.splitk_id(case)
    bt = ex.build_splitk(case)
    ex.check_conds(bt, what)
    M, N, K = case["shape"]
    X, Y = GI(bt.ops["X"]), GI(bt.ops["Y"])
    for run in ("first", "second"):          # twice in a row on the same work buffer
        gd = GO(M, N)
        nv.gemm_splitk(X, Y, gd.view, case["splits"], y_cmajor=case["ycm"])
        ex.assert_same_bits(gd.view, bt.refs["D"], "%s, %s call" % (what, run))
        gd.assert_intact(what)
        for wk in nv._splitk_work.values():
            assert int(wk[:1024].abs().sum()) == 0, "%s: split-K tickets not left zero after the %s call" % (what, run)


# ---- f. st_gemm_kscale --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", ex.KSCALE_CASES, ids=ex.kscale_id)
def test_gemm_kscale_exact(case):
    """Equality says both: the columns [lo, hi) are scaled BEFORE their one rounding, the others are not scaled."""
    what = "gemm_kscale " + ex.kscale_id(case)
    bt = ex.build_kscale(case)
    ex.check_conds(bt, what)
    M, N, K = case["shape"]
    gd = GO(M, N)
    nv.gemm_kscale(GI(bt.ops["X"]), GI(bt.ops["W"]), gd.view, GI(bt.ops["bias"]), *case["cols"], case["scale"])
    ex.assert_same_bits(gd.view, bt.refs["D"], what)
    gd.assert_intact(what)


# ---- g. st_gemm_stacked -------------------------------------------------------------------------------------------------------
def _stack_views(o, rows, K):
    aw, ab = o["arena_w"].cuda(), o["arena_b"].cuda()
    return torch.as_strided(aw, (rows, K), (K, 1), o["w_off"]), ab[o["b_off"]:o["b_off"] + rows]


@pytest.mark.parametrize("case", ex.STACKED_CASES, ids=ex.stacked_id)
def test_gemm_stacked_exact(case):
    """The blocks lie further apart than rows * ld, NaN between them (and between the bias blocks)."""
    what = "gemm_stacked " + ex.stacked_id(case)
    bt = ex.build_stacked(case)
    ex.check_conds(bt, what)
    o, M, blocks, rows, K = bt.ops, case["M"], case["blocks"], case["rows"], case["K"]
    assert o["w_stride"] > rows * K and o["b_stride"] > rows and bool(torch.isnan(o["arena_w"].float()).any())
    W0, b0 = _stack_views(o, rows, K)
    if case["kind"] == "fwd":
        gd = GO(M, blocks * rows)
        nv.gemm(GI(o["X"]), W0, gd.view, bias=b0, stack=(blocks, o["w_stride"], o["b_stride"]))
    else:
        gd = GO(M, K)
        nv.gemm(GI(o["dy"]), W0, gd.view, bias=GI(o["bias"]), y_cmajor=True, stack=(blocks, o["w_stride"], 0), epi=case["epi"], aux=GI(o.get("aux")))
    ex.assert_same_bits(gd.view, bt.refs["D"], what, alternatives=bt.alts.get("D"))
    gd.assert_intact(what)


# ---- h. st_gemm_ws ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", ex.WS_CASES, ids=ex.ws_id)
def test_gemm_ws_exact(case):
    what = "gemm_ws " + ex.ws_id(case)
    bt = ex.build_ws(case)
    ex.check_conds(bt, what)
    o, (M, N) = bt.ops, case["shape"]
    gd = GO(M, N)
    drop = drop_site(11) if case["drop"] else None
    if case["stack"]:
        blocks, rows = case["stack"]
        W0, b0 = _stack_views(o, rows, 256)
        nv.gemm_ws(GI(o["X"]), W0, gd.view, bias=b0, relu=case["relu"], drop=drop, stack=(blocks, o["w_stride"], o["b_stride"]))
    else:
        nv.gemm_ws(GI(o["X"]), GI(o["W"]), gd.view, bias=GI(o["bias"]), relu=case["relu"], drop=drop)
    ex.assert_same_bits(gd.view, bt.refs["D"], what, tile=(32, 256))
    gd.assert_intact(what)


# ---- i. st_wgrad_group / st_wgrad_wide ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", ex.GROUP_CASES, ids=ex.group_id)
def test_wgrad_group_and_wide_exact(case):
    """One launch of several problems (49 of them: more than one launch's worth of descriptors), against fp64 - not against
    each other - on top of existing gradients."""
    what = "wgrad " + ex.group_id(case)
    built = ex.build_group(case)
    probs, gds = [], []
    for q, (bt, (t, n, k, sp)) in enumerate(zip(built, case["problems"])):
        ex.check_conds(bt, "%s problem %d" % (what, q))
        gw, gb = holding(bt.ops["init"]), (holding(bt.ops["b0"]) if case["bias"] else None)
        gds.append((gw, gb))
        probs.append((GI(bt.ops["x"]), GI(bt.ops["dy"]), gw.view, gb.view if gb is not None else None, sp, n))
    nv.wgrad_group(probs, wide=case["wide"])
    tile = (256, 256) if case["wide"] else (128, 128)
    for q, (bt, (gw, gb)) in enumerate(zip(built, gds)):
        ex.assert_same_bits(gw.view, bt.refs["dW"], "%s problem %d dW" % (what, q), tile=tile)
        gw.assert_intact("%s problem %d dW" % (what, q))
        if gb is not None:
            ex.assert_same_bits(gb.view, bt.refs["db"], "%s problem %d db" % (what, q), tile=(1, tile[1]))
            gb.assert_intact("%s problem %d db" % (what, q))


# ---- j. st_gemm_ln: the `pre` output --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", ex.LN_CASES, ids=ex.ln_id)
def test_gemm_ln_pre_exact(case):
    """pre = bf16(act(X W^T + bias) + res), rounded once; the normalised outputs keep their own tests (tests/test_kernels_gpu.py,
    tests/test_ln_stats_gpu.py) and are only held inside their guards here."""
    what = "gemm_ln " + ex.ln_id(case)
    bt = ex.build_ln(case)
    ex.check_conds(bt, what)
    o, (M, N, K) = bt.ops, case["shape"]
    out, xhat, rstd, pre = GO(M, N), GO(M, N, contiguous=True), GV(M), GO(M, N, contiguous=True)
    nv.gemm_ln(GI(o["X"]), cu(o["W"]), cu(o["bias"]), GI(o["res"]), cu(o["gamma"]), cu(o["beta"]), out.view, xhat.view, rstd.view,
               eps=1e-6, relu=case["relu"], pre=pre.view, drop=drop_site(6) if case["drop"] else None, drop_where=1 if case["drop"] else 0)
    ex.assert_same_bits(pre.view, bt.refs["pre"], what, tile=(32, 128))
    for gd, nm in ((out, "out"), (xhat, "xhat"), (rstd, "rstd"), (pre, "pre")):
        gd.assert_intact("%s: %s" % (what, nm))
    assert bool(torch.isfinite(out.view.float()).all()) and bool(torch.isfinite(rstd.view).all())


# ---- k. st_row_chain with only the POST stage -----------------------------------------------------------------------------------
@pytest.mark.parametrize("case", ex.CHAIN_CASES, ids=ex.chain_id)
def test_row_chain_post_stage_exact(case):
    """Three 256-row blocks, the chain the encoder's layer-0 q | k | v projection runs as: P = A Wp^T + bp, the key block times
    post_kscale in fp32 before its one rounding.  (`split`: the chain carries a split-work scratch, as the encoder's chains do;
    a chain without a feed-forward stage must not touch it.)"""
    from st_amd import chains
    what = "row_chain " + ex.chain_id(case)
    bt = ex.build_chain(case)
    ex.check_conds(bt, what)
    M = case["M"]
    cs = chains.ChainSet("cuda")
    cid = cs.add(chains.blocks_of(bt.ops["W"].cuda()))
    cs.finalize().rebuild()
    ch = cs.chain(cid)
    work = None
    if case["split"]:
        work = ch.split_work = torch.zeros(nv.split_work_words(), dtype=I32, device="cuda")
    gd = GO(M, 768)
    nv.row_chain(GI(bt.ops["X"], pad_cols=(32, 32)), ch, post=(3, cu(bt.ops["bias"]), gd.view),
                 **({} if case["scale"] is None else {"post_kscale": case["scale"]}))
    ex.assert_same_bits(gd.view, bt.refs["D"], what, tile=(32, 256))
    gd.assert_intact(what)
    if work is not None:
        assert int(work.abs().sum()) == 0, what + ": the split-work scratch was written"
