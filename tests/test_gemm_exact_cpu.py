"""The exact cases of the GEMM family (tests/_exact.py) on the CPU: the recipe keeps its premise for every case, its references
hold enough ties and truncation-sensitive values to tell the rounding modes apart, the emulation agrees with the new fp64
reference bit for bit, and - in the style of tests/test_local_check_cpu.py - every planted defect below PASSES the bounds the
Gaussian kernel tests hold the family to (relative L2 1e-2 / 2e-3 with the per-row, per-column L_BF16 / L_F32) and FAILS the bit
comparator.  That gap is what tests/test_gemm_exact_gpu.py closes; it is kept here as assertions.  No kernel runs."""
import pytest
import torch

from st_amd import native as nv
from tests import _emul as em
from tests import _exact as ex
from tests._local import check

BF16, F32, F64 = torch.bfloat16, torch.float32, torch.float64
L_BF16, L_F32 = 1e-2, 2e-3          # tests/test_kernels_gpu.py's bounds of the family
CASES = ex.all_cases()
IDS = ["%s-%s" % (f, i) for f, i, _, _ in CASES]


def _fails(fn, *needles):
    with pytest.raises(AssertionError) as e:
        fn()
    for n in needles:
        assert n in str(e.value), "%r not in: %s" % (n, e.value)
    return str(e.value)


def test_case_ids_are_unique_and_the_epilogue_numbers_are_the_headers():
    assert len(set(IDS)) == len(IDS)
    assert (ex.EPI_BF16, ex.EPI_BF16_RELU, ex.EPI_F32, ex.EPI_BF16_MASK, ex.EPI_BF16_ADD, ex.EPI_F32_ATOMIC, ex.EPI_F32_ATOMIC_T,
            ex.EPI_BF16_DELTA) == (nv.EPI_BF16, nv.EPI_BF16_RELU, nv.EPI_F32, nv.EPI_BF16_MASK, nv.EPI_BF16_ADD, nv.EPI_F32_ATOMIC,
                                   nv.EPI_F32_ATOMIC_T, nv.EPI_BF16_DELTA)
    d = em.Drop(torch.tensor([ex.DROP_SEED], dtype=torch.int32), 11, ex.DROP_P)
    assert d.scale == 2.0 and nv.Drop.__init__ is not None


# ---- the rounder ----------------------------------------------------------------------------------------------------------
def test_integer_rounder_equals_torchs_conversion():
    """(bits + 0x7FFF + ((bits >> 16) & 1)) >> 16 on the fp32 pattern == torch's fp32 -> bf16, on every kind of value the cases
    hold (ties to even and to odd neighbours, both signs, zeros, eighths, five-bit scales) and on random fp32 patterns."""
    gen = torch.Generator().manual_seed(1)
    vals = [torch.arange(-4200, 4201, dtype=F64) / 8, torch.arange(-70000, 70001, 7, dtype=F64) * 1.4375 / 8,
            torch.tensor([0.0, -0.0, 257.0, 258.0, 259.0, 385.0, 387.0, -257.0, -259.0, 1.0 + 2.0 ** -8, 1.0 + 3 * 2.0 ** -8], dtype=F64),
            torch.randn(200000, generator=gen, dtype=F32).to(F64) * 1000]
    for v in vals:
        want = v.to(F32).to(BF16).view(torch.int16).to(torch.int64) & 0xFFFF
        assert torch.equal(ex.bf16_rne_bits(v), want)
        assert torch.equal(ex.rne64(v), v.to(F32).to(BF16).to(F64))
    t = torch.tensor([257.0, 259.0, 256.5, 3.0], dtype=F64)          # 257 -> 256 (even), 259 -> 260; 256.5 is no tie of bf16
    assert ex.is_tie(t).tolist() == [True, True, False, False]
    assert ex.rne64(t).tolist() == [256.0, 260.0, 256.0, 3.0]
    assert ex.bits_to_f64(ex.bf16_trunc_bits(t)).tolist() == [256.0, 258.0, 256.0, 3.0]
    assert ex.bits_to_f64(ex.bf16_half_away_bits(t)).tolist() == [258.0, 260.0, 256.0, 3.0]


def test_assert_exact_fp32_refuses_what_is_not_exact():
    ex.assert_exact_fp32(torch.tensor([3.0, -7.0, 16777215.0], dtype=F64), "fine")
    ex.assert_exact_fp32(torch.tensor([3.0, -0.125, 2.0 ** 21 - 0.125], dtype=F64), "fine, in eighths")
    _fails(lambda: ex.assert_exact_fp32(torch.tensor([16777216.0, 1.0], dtype=F64), "2^24"), "not below 2^24")
    _fails(lambda: ex.assert_exact_fp32(torch.tensor([2.0 ** 21, 0.125], dtype=F64), "2^24 eighths"), "not below 2^24")
    _fails(lambda: ex.assert_exact_fp32(torch.tensor([0.1], dtype=F64), "0.1"), "does not survive")
    _fails(lambda: ex.assert_exact_fp32(torch.tensor([float("nan")], dtype=F64), "nan"), "non-finite")


# ---- the recipe -----------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def built():
    """Every single-output case built once: id -> (family, case, Built)."""
    return {i: (f, c, b(c)) for (f, _, c, b), i in zip(CASES, IDS)}


def test_recipe_conditions_hold_for_every_case(built):
    for i, (f, c, bt) in built.items():
        ex.check_conds(bt, i)
        for name, ref in bt.refs.items():
            ex.assert_exact_fp32(ref, "%s: the exact %s" % (i, name))
    for c in ex.GROUP_CASES:
        for q, bt in enumerate(ex.build_group(c)):
            ex.check_conds(bt, "%s problem %d" % (ex.group_id(c), q))
    for lo, hi in ((-4, 4), (-128, 127)):
        A, Bt = ex.mfma_operands(lo, hi)
        assert A.to(F64).abs().max() <= 128 and torch.equal(A.to(F64), A.to(F64).round())
        ex.assert_exact_fp32(A.to(F64).abs() @ Bt.to(F64).abs().t(), "mfma probe [%d, %d]" % (lo, hi))


# bf16 cases whose references cannot hold the shares below, by name.  Integer sums have no ties below 256 (every integer there
# is a bf16 value) and few below 512: without a bias - and the DELTA epilogue and st_gemm_splitk take none - a contraction of 72 or
# 520 terms stays there; K = 8 stays below 40 with one.
EXEMPT = {"fwd-bf16-1x8x8-bias", "fwd-bf16-1x8x8-nobias", "fwd-relu-1x8x8-bias", "fwd-relu-1x8x8-nobias",
          "fwd-bf16-127x136x72-nobias", "fwd-relu-127x136x72-nobias", "fwd-bf16-129x264x64-nobias", "fwd-relu-129x264x64-nobias",
          "fwd-bf16-257x136x200-nobias", "fwd-relu-257x136x200-nobias",
          "dgrad-delta-hd32-127x72x128", "dgrad-delta-hd32-aux2-127x72x128", "dgrad-delta-hd64-127x72x128",
          "dgrad-delta-hd64-aux2-127x72x128", "dgrad-delta-hd128-127x72x128", "dgrad-delta-hd128-aux2-127x72x128",
          "dgrad-delta-hd32-129x520x256", "dgrad-delta-hd32-aux2-129x520x256", "dgrad-delta-hd64-129x520x256",
          "dgrad-delta-hd64-aux2-129x520x256", "dgrad-delta-hd128-129x520x256", "dgrad-delta-hd128-aux2-129x520x256",
          "splitk-5x136x520-splits9-natural", "splitk-5x136x520-splits9-ycm"}


def _contraction(f, c):
    if f in ("fwd", "splitk", "kscale", "ln"):
        return c["shape"][2]
    if f == "dgrad":
        return c["shape"][1]
    if f == "stacked":
        return c["K"] if c["kind"] == "fwd" else c["blocks"] * c["rows"]
    return 256          # ws, chain


def test_tie_and_truncation_shares(built):
    """Every bf16 reference with K >= 40 holds >= 5 % ties and >= 10 % values that truncation rounds differently (among the values
    the epilogue does not zero: a ReLU / mask / dropout zero is exact under every rounding; ST_EPI_BF16_ADD: among the values of
    its first rounding); the exempt are named, at most a quarter of the bf16 cases."""
    n_bf16, seen = 0, set()
    for i, (f, c, bt) in built.items():
        if not ex.bf16_output(f, c):
            continue
        n_bf16 += 1
        ref = bt.first if bt.first is not None else bt.refs["pre" if f == "ln" else "D"]
        res = bt.ops.get("res") if f == "ln" else None          # (a zero of st_gemm_ln's activation leaves as the residual alone)
        live = ref[(ref if res is None else ref - res.to(F64)) != 0]
        ties = float(ex.is_tie(live).double().mean()) if live.numel() else 0.0
        trunc = float((ex.bf16_trunc_bits(live) != ex.bf16_rne_bits(live)).double().mean()) if live.numel() else 0.0
        if i in EXEMPT:
            seen.add(i)
            continue
        assert _contraction(f, c) >= 40, "%s: K < 40 and not named exempt" % i
        assert ties >= 0.05 and trunc >= 0.10, "%s: %.1f %% ties, %.1f %% truncation-sensitive" % (i, 100 * ties, 100 * trunc)
    assert seen == EXEMPT and len(EXEMPT) <= n_bf16 / 4


def test_recipe_figures_of_the_record():
    """The table of tests/LOCAL_BOUNDS.md ("Exact cases"): largest value, tie share, truncation share at four shapes."""
    for (M, N, K), top_max, tie_min, trunc_min in (((129, 136, 40), 260, 0.15, 0.10), ((257, 264, 256), 640, 0.15, 0.20),
                                                   ((129, 136, 2072), 1800, 0.10, 0.30), ((1206, 256, 4344), 2900, 0.08, 0.35)):
        gen = torch.Generator().manual_seed(K)
        X, W, b = ex.ints(gen, (M, K)), ex.ints(gen, (N, K)), ex.eighths(gen, (N,), 8)
        v = X.to(F64) @ W.to(F64).t() + b.to(F64)
        ex.assert_exact_fp32(X.to(F64).abs() @ W.to(F64).abs().t() + b.to(F64).abs(), "record %s" % ((M, N, K),))
        ties, trunc = float(ex.is_tie(v).double().mean()), float((ex.bf16_trunc_bits(v) != ex.bf16_rne_bits(v)).double().mean())
        print("%s: max |v| %.1f, ties %.1f %%, truncation differs %.1f %%" % ((M, N, K), float(v.abs().max()), 100 * ties, 100 * trunc))
        assert float(v.abs().max()) <= top_max and ties >= tie_min and trunc >= trunc_min
        assert torch.equal(v.to(F32).to(F64), v)


# ---- agreement with the emulation -------------------------------------------------------------------------------------------
def _emulate(f, c, bt):
    """The emulation (tests/_emul.py) in fp64 on the case's operands -> {output name: tensor}."""
    o = bt.ops
    if f == "fwd":
        M, N, K = c["shape"]
        out = torch.zeros(M, N, dtype=F32 if c["epi"] == ex.EPI_F32 else BF16)
        em.gemm(o["X"], o["W"], out, bias=o["bias"], epi=c["epi"], drop=ex.drops(11) if c["drop"] else None, dtype=F64)
        return dict(D=out)
    if f == "dgrad":
        M, C, N = c["shape"]
        out, delta = torch.zeros(M, N, dtype=BF16), torch.zeros((N // c["hd"]) * M if "hd" in c else 0, dtype=F32)
        drop = ex.drops(11) if c.get("scale", 1.0) == 2.0 else None
        em.gemm(o["dy"], o["W"], out, bias=o["bias"], aux=o.get("aux"), aux2=o.get("aux2"), epi=c["epi"], y_cmajor=True, drop=drop, delta=delta,
                head_dim=c.get("hd", 0), dtype=F64)
        return dict(D=out, delta=delta) if "hd" in c else dict(D=out)
    if f == "wgrad":
        dW, db = o["init"].clone(), o["b0"].clone()
        em.gemm(o["x"], o["dy"], dW, bias=db, epi=nv.EPI_F32_ATOMIC_T, x_cmajor=True, y_cmajor=True, splits=c["splits"], n=c["out"][0], dtype=F64)
        return dict(dW=dW, db=db)
    if f == "splitk":
        M, N, K = c["shape"]
        return dict(D=em.gemm_splitk(o["X"], o["Y"], torch.zeros(M, N, dtype=BF16), c["splits"], y_cmajor=c["ycm"], dtype=F64))
    if f == "kscale":
        M, N, K = c["shape"]
        return dict(D=em.gemm_kscale(o["X"], o["W"], torch.zeros(M, N, dtype=BF16), o["bias"], *c["cols"], c["scale"], dtype=F64))
    if f == "ws":
        M, N = c["shape"]
        return dict(D=em.gemm_ws(o["X"], o["W"], torch.zeros(M, N, dtype=BF16), bias=o["bias"], relu=c["relu"],
                                 drop=ex.drops(11) if c["drop"] else None, dtype=F64))
    if f == "ln":
        M, N, K = c["shape"]
        out, xhat, pre = (torch.zeros(M, N, dtype=BF16) for _ in range(3))
        em.gemm_ln(o["X"], o["W"], o["bias"], o["res"], o["gamma"], o["beta"], out, xhat, torch.zeros(M, dtype=F32), relu=c["relu"], pre=pre,
                   drop=ex.drops(6) if c["drop"] else None, drop_where=1 if c["drop"] else 0, dtype=F64)
        return dict(pre=pre)
    return None


def test_emulation_agrees_with_the_exact_reference(built):
    """em.gemm (every epilogue, ST_EPI_BF16_ADD in its two-rounding form), em.gemm_kscale, em.gemm_ws and em.gemm_ln's pre, in
    fp64, give the new reference's bits on every case (the encoder-sized st_gemm_ln shapes run the same emulation code as the
    small ones and are left out)."""
    n = 0
    for i, (f, c, bt) in built.items():
        if f == "ln" and c["shape"][0] > 1000:
            continue
        got = _emulate(f, c, bt)
        if got is None:
            continue
        for name, t in got.items():
            ex.assert_same_bits(t, bt.refs[name], "emulation %s %s" % (i, name))
            n += 1
    assert n > 150


def test_emulated_add_rounds_twice_and_the_fused_lnbwd_once():
    """The contract of ST_EPI_BF16_ADD (include/st_hip.h): D = bf16(bf16(acc) + aux).  The case set tells it from the single
    rounding of acc + aux, which is what the emulated st_gemm_lnbwd keeps (as the fused kernel does)."""
    c = dict(shape=(129, 520, 264), epi=ex.EPI_BF16_ADD, alias=False, bias=False)
    bt = ex.build_dgrad(c)
    once = bt.alts["D"]["one rounding of acc + aux"]
    differ = ex.bf16_rne_bits(once) != ex.bf16_rne_bits(bt.refs["D"])
    assert float(differ.double().mean()) > 0.02, "the two contracts coincide on this case"
    one = torch.zeros(129, 264, dtype=BF16)
    em.gemm(bt.ops["dy"], bt.ops["W"], one, epi=nv.EPI_BF16, y_cmajor=True, dtype=F64)
    ex.assert_same_bits((one.to(F64) + bt.ops["aux"].to(F64)).to(BF16), bt.refs["D"], "two roundings")
    # in place, as functional.py accumulates the cross-attention K/V input gradient: aux IS the output
    buf = bt.ops["aux"].clone()
    em.gemm(bt.ops["dy"], bt.ops["W"], buf, aux=buf, epi=nv.EPI_BF16_ADD, y_cmajor=True, dtype=F64)
    ex.assert_same_bits(buf, bt.refs["D"], "emulated ADD in place")


# ---- planted defects: the old bounds pass, the comparator fails ---------------------------------------------------------------
def _old_bf16(got, ref64, what):
    check(got, ref64, 1e-2, what, tol_local=L_BF16)


def _old_f32(got, ref64, what):
    check(got, ref64, 2e-3, what, tol_local=L_F32)


@pytest.fixture(scope="module")
def fwd():
    """A bf16 forward case with long K (exact fp64 result, its correct bf16 output) - (130, 136, 2104) with bias."""
    bt = ex.build_fwd(dict(shape=ex.FWD_8WAVE, epi=ex.EPI_BF16, bias=True, drop=False))
    good = bt.refs["D"].to(F32).to(BF16)
    ex.assert_same_bits(good, bt.refs["D"], "undamaged")
    _old_bf16(good, bt.refs["D"], "undamaged")
    return bt, good


def test_planted_one_element_one_ulp_off(fwd):
    bt, good = fwd
    got = good.clone()
    r, c = 77, 101
    got.view(torch.int16)[r, c] += 1
    _old_bf16(got, bt.refs["D"], "one ulp")
    msg = _fails(lambda: ex.assert_same_bits(got, bt.refs["D"], "one ulp"), "1 of %d elements differ" % got.numel(), "row 77 column 101",
                 "row % 32 / 64 / 96 / 128 = 13 / 13 / 77 / 77", "column % 32 / 128 = 5 / 101", "tile (0, 0)")
    assert "got - exact" in msg


def test_planted_truncating_rounding(fwd):
    bt, _ = fwd
    exact = bt.refs["D"]
    got = ex.bits_to_f64(ex.bf16_trunc_bits(exact)).to(BF16)
    n = int((ex.bf16_trunc_bits(exact) != ex.bf16_rne_bits(exact)).sum())
    assert n > 0.3 * exact.numel()
    _old_bf16(got, exact, "truncation")
    _fails(lambda: ex.assert_same_bits(got, exact, "truncation"), "%d of %d elements differ" % (n, exact.numel()),
           "truncation: %d of %d" % (n, n), "round half away: 0 of %d" % n)


def test_planted_round_half_away(fwd):
    bt, _ = fwd
    exact = bt.refs["D"]
    got = ex.bits_to_f64(ex.bf16_half_away_bits(exact)).to(BF16)
    n = int((ex.bf16_half_away_bits(exact) != ex.bf16_rne_bits(exact)).sum())
    assert n > 0.03 * exact.numel()          # half of the ties: those whose even neighbour lies towards zero
    _old_bf16(got, exact, "round half away")
    _fails(lambda: ex.assert_same_bits(got, exact, "half away"), "%d of %d elements differ" % (n, exact.numel()),
           "round half away: %d of %d" % (n, n), "truncation: 0 of %d" % n)


def test_planted_one_k_term_dropped(fwd):
    bt, good = fwd
    X, W, exact = bt.ops["X"].to(F64), bt.ops["W"].to(F64), bt.refs["D"]
    r, c = 129, 135          # the last row and column
    prod = X[r] * W[c]
    k = int(torch.where(prod != 0, prod.abs(), torch.full_like(prod, 99.0)).argmin())
    assert 1 <= abs(float(prod[k])) <= 4
    short = exact.clone()
    short[r, c] -= prod[k]
    got = short.to(F32)          # an fp32 output shows the missing product itself
    _old_f32(got, exact, "one k term")
    _fails(lambda: ex.assert_same_bits(got, exact, "one k term"), "1 of %d elements differ" % got.numel(), "row 129 column 135",
           "got - exact = %r" % float(-prod[k]))
    # a bf16 output shows it wherever it crosses a rounding step - always below 256, where every integer is a bf16 value
    r, c = [int(v) for v in torch.nonzero((exact.abs() < 200) & (exact.abs() > 8))[0]]
    k = int(torch.nonzero(X[r] * W[c])[0])
    short = exact.clone()
    short[r, c] -= X[r, k] * W[c, k]
    got = short.to(F32).to(BF16)
    _old_bf16(got, exact, "one k term, bf16")
    _fails(lambda: ex.assert_same_bits(got, exact, "one k term, bf16"), "1 of %d elements differ" % got.numel(), "row %d column %d" % (r, c))


@pytest.fixture(scope="module")
def wg():
    """A weight gradient over 32,769 tokens in 64-token splits (the 513th holds ONE token), on top of existing gradients.  Only
    at such a share can a whole partial pass the old bounds: a split that holds a third of 1,000 tokens moves the rows of its
    128 x 128 tile by 0.29 of their norm, and 2e-3 sees that."""
    bt = ex.build_wgrad(dict(tokens=32769, splits=513, out=(264, 520)))
    ex.check_conds(bt, "planted weight gradient")
    for n in ("dW", "db"):
        ex.assert_same_bits(bt.refs[n].to(F32), bt.refs[n], "undamaged " + n)
        _old_f32(bt.refs[n].to(F32), bt.refs[n], "undamaged " + n)
    return bt


def test_planted_one_splits_partial_tile_lost(wg):
    """The last split's partial never reaches one 128 x 128 tile of dW - the ragged corner tile (rows 256 .., columns 512 ..)."""
    dy, x, exact = wg.ops["dy"].to(F64), wg.ops["x"].to(F64), wg.refs["dW"]
    got = exact.clone()
    lost = dy[32768:, 256:].t() @ x[32768:, 512:]
    n = int((lost != 0).sum())
    assert n > 16
    got[256:, 512:] -= lost
    got = got.to(F32)
    _old_f32(got, exact, "one split's partial tile")
    _fails(lambda: ex.assert_same_bits(got, exact, "partial tile"), "%d of %d elements differ" % (n, exact.numel()), "tile (2, 4)", "row 25")
    # one lost ATOMIC (a single element of a partial) anywhere, and a third of 1,000 tokens - which the old bounds do see
    got = exact.clone()
    got[200, 400] -= 3.0
    _old_f32(got.to(F32), exact, "one lost atomic")
    _fails(lambda: ex.assert_same_bits(got.to(F32), exact, "one lost atomic"), "1 of %d elements differ" % exact.numel(),
           "row 200 column 400", "got - exact = -3.0", "tile (1, 3)")
    small = ex.build_wgrad(dict(tokens=1000, splits=3, out=(264, 520)))
    dy, x, got = small.ops["dy"].to(F64), small.ops["x"].to(F64), small.refs["dW"].clone()
    got[128:256, 384:512] -= dy[334:668, 128:256].t() @ x[334:668, 384:512]
    _fails(lambda: _old_f32(got.to(F32), small.refs["dW"], "a third of the tokens"), "rel-L2")


def test_planted_one_bias_gradient_element_doubled(wg):
    """One split's contribution to one bias-gradient element added twice (its last token's dy: +-1 on top of a sum of hundreds)."""
    dy, ref = wg.ops["dy"].to(F64), wg.refs["db"]
    last = dy[32768]
    j = int(torch.where(last.abs() == 1, ref.abs(), torch.zeros_like(ref)).argmax())
    add = float(last[j])
    assert abs(add) == 1 and abs(float(ref[j])) >= 500
    got = ref.clone()
    got[j] += add
    got = got.to(F32)
    _old_f32(got, ref, "doubled bias gradient")
    _fails(lambda: ex.assert_same_bits(got, ref, "doubled bias gradient"), "1 of %d elements differ" % got.numel(), "column %d" % j,
           "got - exact = %r" % add)


def test_planted_two_roundings_on_the_add_epilogue():
    """If the contract were ONE rounding of acc + aux, a kernel that rounds twice passes the old bounds and fails here - and the
    comparator says which of the two it saw.  (The header now states two; the GPU test holds that.)"""
    bt = ex.build_dgrad(dict(shape=(129, 520, 264), epi=ex.EPI_BF16_ADD, alias=False, bias=True))
    one = bt.alts["D"]["one rounding of acc + aux"]
    twice = bt.refs["D"].to(F32).to(BF16)
    _old_bf16(twice, one, "two roundings")
    n = int((ex.bf16_rne_bits(one) != ex.bf16_rne_bits(bt.refs["D"])).sum())
    _fails(lambda: ex.assert_same_bits(twice, one, "two roundings", alternatives={"two roundings": bt.refs["D"]}),
           "%d of %d elements differ" % (n, one.numel()), "two roundings: %d of %d" % (n, n))
    once = one.to(F32).to(BF16)
    _old_bf16(once, bt.refs["D"], "one rounding")
    _fails(lambda: ex.assert_same_bits(once, bt.refs["D"], "one rounding", alternatives=bt.alts["D"]),
           "one rounding of acc + aux: %d of %d" % (n, n))


def test_negative_zero_equals_positive_zero_and_nan_equals_nothing():
    exact = torch.tensor([[0.0, -0.0, 1.0, -3.0]], dtype=F64)
    ex.assert_same_bits(torch.tensor([[-0.0, 0.0, 1.0, -3.0]], dtype=BF16), exact, "zeros bf16")
    ex.assert_same_bits(torch.tensor([[-0.0, 0.0, 1.0, -3.0]], dtype=F32), exact, "zeros f32")
    _fails(lambda: ex.assert_same_bits(torch.tensor([[0.0, 0.0, float("nan"), -3.0]], dtype=BF16), exact, "nan"), "1 of 4 elements differ",
           "row 0 column 2")
    want = ex.bf16_rne_bits(exact)
    ex.assert_same_bits(torch.tensor([[0.0, -0.0, 1.0, -3.0]], dtype=BF16), want, "bit patterns as the reference")
