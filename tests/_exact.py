"""Exact cases of the GEMM family: integer operands on which fp32 accumulation is EXACT, an fp64 reference, a bit comparator.

The recipe (tests/LOCAL_BOUNDS.md, "Exact cases"): bf16 matrices hold integers in [-4, 4], the fp32 bias multiples of 2^-3 in
[-8, 8], an addend / mask source integers in [-4, 4], aux2 multiples of 2^-3 in [-1, 1], an existing gradient integers in
[-64, 64]; scales are 2^-3 and 1.4375, dropout runs at p = 0.5 (survivors x 2).  Every product and every partial sum is then a
multiple of a fixed power of two below 2^24 of it IN ANY ORDER - inside the MFMA, across k-tiles, wave groups, split-K partials
and atomics - so the fp32 result must equal the fp64 one bit for bit and a bf16 result must be the ONE round-to-nearest-even
of the exact value.  ``assert_exact_fp32`` checks that premise on the inputs of every case; ``assert_same_bits`` compares.

Plain torch; st_amd.native is not imported here (the dropout masks come from tests/_emul.py, imported where a case needs one).
"""
import collections
import functools
import zlib

import torch

BF16, F32, F64 = torch.bfloat16, torch.float32, torch.float64
# include/st_hip.h's ST_EPI_* (tests/test_gemm_exact_cpu.py asserts they are the header's)
EPI_BF16, EPI_BF16_RELU, EPI_F32, EPI_BF16_MASK, EPI_BF16_ADD, EPI_F32_ATOMIC, EPI_F32_ATOMIC_T, EPI_BF16_DELTA = range(8)
SCALES = (0.125, 1.4375)          # 2^-3 and 23 / 16: five significant bits
DROP_P, DROP_SEED = 0.5, 1234567  # drop_scale is exactly 2


# ---- the rounder and the premise ------------------------------------------------------------------------------------------
def _f32_bits(x64):
    """The fp32 bit patterns (int64, 0 .. 2^32 - 1) of an fp64 tensor whose values are fp32 values."""
    return x64.to(F32).contiguous().view(torch.int32).to(torch.int64) & 0xFFFFFFFF


def bf16_rne_bits(x64):
    """The bf16 bit pattern (int64, 0 .. 65535) of round-to-nearest-even of every value, in integer arithmetic on its fp32
    bit pattern: (bits + 0x7FFF + ((bits >> 16) & 1)) >> 16.  The values must be fp32 values (assert_exact_fp32)."""
    bits = _f32_bits(x64)
    return ((bits + 0x7FFF + ((bits >> 16) & 1)) >> 16) & 0xFFFF


def bf16_trunc_bits(x64):
    return _f32_bits(x64) >> 16


def bf16_half_away_bits(x64):
    return ((_f32_bits(x64) + 0x8000) >> 16) & 0xFFFF


def _f32_of_bits(bits):
    """fp32 bit patterns (int64, 0 .. 2^32 - 1) -> the fp32 values."""
    return torch.where(bits >= 2 ** 31, bits - 2 ** 32, bits).to(torch.int32).view(F32)


def bits_to_f64(bits):
    """bf16 bit patterns (int64) -> their values in fp64."""
    return _f32_of_bits(bits << 16).to(F64)


def rne64(x64):
    """round-to-nearest-even to bf16, value in fp64."""
    return bits_to_f64(bf16_rne_bits(x64))


def is_tie(x64):
    """Exactly halfway between two bf16 values: the low 16 bits of the fp32 pattern are 0x8000."""
    return (_f32_bits(x64) & 0xFFFF) == 0x8000


def assert_exact_fp32(x64, what):
    """The premise, a condition on the INPUTS: every value of ``x64`` (a quantity the kernel forms in fp32, or the sum of
    absolute products that bounds every partial sum it can form, in any order) is an fp32 value and stays below 2^24 of its
    own unit - the largest power of two (down to 2^-20) that divides all of them."""
    x = x64.detach().to(F64).reshape(-1)
    if not x.numel():
        return
    assert bool(torch.isfinite(x).all()), "%s: non-finite value in the recipe" % what
    assert bool((x.to(F32).to(F64) == x).all()), "%s: a value does not survive fp64 -> fp32 -> fp64" % what
    for k in range(0, 21):
        if bool(((x * 2.0 ** k) == (x * 2.0 ** k).round()).all()):
            break
    else:
        raise AssertionError("%s: values are not multiples of 2^-20" % what)
    top = float(x.abs().max()) * 2.0 ** k
    assert top < 2.0 ** 24, "%s: %.0f units of 2^-%d is not below 2^24 - fp32 sums are not exact in every order" % (what, top, k)


# ---- the comparator -------------------------------------------------------------------------------------------------------
def _expected_bits(exact64, dtype):
    if dtype == BF16:
        b = bf16_rne_bits(exact64)
        return torch.where(b == 0x8000, torch.zeros_like(b), b)
    b = _f32_bits(exact64)
    return torch.where(b == 0x80000000, torch.zeros_like(b), b)


def _got_bits(got):
    if got.dtype == BF16:
        b = got.contiguous().view(torch.int16).to(torch.int64) & 0xFFFF
        return torch.where(b == 0x8000, torch.zeros_like(b), b)
    assert got.dtype == F32, "bf16 or fp32 outputs"
    b = got.contiguous().view(torch.int32).to(torch.int64) & 0xFFFFFFFF
    return torch.where(b == 0x80000000, torch.zeros_like(b), b)


def assert_same_bits(got, ref_bits_or_f32, what, tile=(128, 128), alternatives=None):
    """``got`` (bf16 or fp32, any device) equals the reference bit for bit.  The reference is the EXACT result in fp64 (a bf16
    output must be its one round-to-nearest-even, an fp32 output the value itself) or, as an integer tensor, the expected bit
    patterns themselves.  -0.0 and +0.0 count as EQUAL: no epilogue of include/st_hip.h promises a sign of zero (a masked
    or dropped element is +0 in the kernels and acc * 0 = -0 for a negative acc in the reference), so both sides are compared
    after mapping -0 to +0.  A NaN in ``got`` never equals anything.
    On failure: how many elements differ, the first and the worst with row, column, row % 32 / 64 / 96 / 128, column % 32 / 128
    and the ``tile`` they lie in, the difference got - exact (integer data: it reads directly as a missing or doubled
    contribution), and which alternative explains the kernel's value at the differing elements: "truncation", "round half
    away", "exact value not rounded", and whatever fp64 tensors ``alternatives`` names (each rounded once like the reference,
    e.g. "two roundings").  Prints one summary line either way (pytest -s) and returns (elements, ties, mismatches)."""
    g = got.detach().cpu()
    g = g.reshape(1, -1) if g.dim() <= 1 else g.reshape(-1, g.shape[-1])
    ref = ref_bits_or_f32.detach().cpu()
    ref = ref.reshape(1, -1) if ref.dim() <= 1 else ref.reshape(-1, ref.shape[-1])
    assert g.shape == ref.shape, "%s: shapes differ: got %s, reference %s" % (what, tuple(g.shape), tuple(ref.shape))
    exact = ref.to(F64) if ref.dtype.is_floating_point else None
    want = _expected_bits(exact, g.dtype) if exact is not None else ref.to(torch.int64)
    want = torch.where(want == (0x8000 if g.dtype == BF16 else 0x80000000), torch.zeros_like(want), want)
    gb = _got_bits(g)
    ties = int(is_tie(exact).sum()) if (exact is not None and g.dtype == BF16) else 0
    bad = gb != want
    n_bad = int(bad.sum())
    print("exact %s: %d elements compared, %d ties, %d mismatches" % (what, g.numel(), ties, n_bad))
    if n_bad == 0:
        return g.numel(), ties, 0
    idx = torch.nonzero(bad)
    gv = g.to(F64)
    wv = exact if exact is not None else (bits_to_f64(want) if g.dtype == BF16 else _f32_of_bits(want).to(F64))
    diff = torch.nan_to_num(gv - wv, nan=float("inf"), posinf=float("inf"), neginf=float("-inf"))
    worst = idx[int(diff[bad].abs().argmax())].tolist()

    def where(rc):
        r, c = rc
        return ("row %d column %d (row %% 32 / 64 / 96 / 128 = %d / %d / %d / %d, column %% 32 / 128 = %d / %d, tile (%d, %d)): got %r, "
                "exact %r, got - exact = %r" % (r, c, r % 32, r % 64, r % 96, r % 128, c % 32, c % 128, r // tile[0], c // tile[1],
                                                float(gv[r, c]), float(wv[r, c]), float(diff[r, c])))

    msg = "%s: %d of %d elements differ from the exact result; first at %s; worst at %s" % (
        what, n_bad, g.numel(), where(idx[0].tolist()), where(worst))
    if exact is not None:
        alts = collections.OrderedDict()
        if g.dtype == BF16:
            alts["truncation"] = bf16_trunc_bits(exact)
            alts["round half away"] = bf16_half_away_bits(exact)
        alts["exact value not rounded"] = None
        for name, t in (alternatives or {}).items():
            t = t.detach().cpu().to(F64)
            alts[name] = _expected_bits(t.reshape(1, -1) if t.dim() <= 1 else t.reshape(-1, t.shape[-1]), g.dtype)
        said = []
        for name, b in alts.items():
            if b is None:
                hit = int((gv[bad] == exact[bad]).sum())
            else:
                b = torch.where(b == (0x8000 if g.dtype == BF16 else 0x80000000), torch.zeros_like(b), b)
                hit = int((gb[bad] == b[bad]).sum())
            said.append("%s: %d of %d" % (name, hit, n_bad))
        msg += "; the kernel's value at the differing elements is reproduced by - " + ", ".join(said)
    raise AssertionError(msg)


# ---- operands -------------------------------------------------------------------------------------------------------------
def _gen(*key):
    return torch.Generator().manual_seed(zlib.crc32(repr(key).encode()))


def ints(gen, shape, lo=-4, hi=4, dtype=BF16):
    return torch.randint(lo, hi + 1, tuple(shape), generator=gen).to(dtype)


def eighths(gen, shape, bound, dtype=F32):
    """Multiples of 2^-3 within [-bound, bound]."""
    return (torch.randint(-8 * bound, 8 * bound + 1, tuple(shape), generator=gen).to(F64) / 8).to(dtype)


def drops(salt):
    """The emulation's dropout call site at p = 0.5 (st_amd.native.Drop takes the same seed, salt and p on the device)."""
    from tests import _emul as em
    return em.Drop(torch.tensor([DROP_SEED], dtype=torch.int32), salt, DROP_P)


def keep(salt, M, N):
    from tests import _emul as em
    return em.keep_rc(drops(salt), torch.arange(M), torch.arange(N), N).to(F64)


@functools.lru_cache(maxsize=4)
def _xw(key, M, N, K):
    """X [M, K], W [N, K], their fp64 product and the sum of absolute products (shared by the cases of one shape)."""
    gen = _gen(key, M, N, K)
    X, W = ints(gen, (M, K)), ints(gen, (N, K))
    x, w = X.to(F64), W.to(F64)
    return X, W, x @ w.t(), x.abs() @ w.abs().t()


Built = collections.namedtuple("Built", "ops refs alts conds first", defaults=(None,))
# ops: name -> CPU tensor (the kernel's operands);  refs: output name -> exact fp64 result;  alts: output name -> {diagnostic
# alternative -> fp64};  conds: [(what, fp64)] - every quantity assert_exact_fp32 must accept;  first: ST_EPI_BF16_ADD only - the
# value of the FIRST of its two roundings (acc + bias), where the ties of such a case lie


def check_conds(built, what):
    for name, x in built.conds:
        assert_exact_fp32(x, "%s: %s" % (what, name))


# ---- the cases (shared by tests/test_gemm_exact_cpu.py and tests/test_gemm_exact_gpu.py) -------------------------------------
FWD_SHAPES = [(1, 8, 8), (127, 136, 72), (129, 264, 64), (257, 136, 200)]
FWD_8WAVE = (130, 136, 2104)          # 8-wave K split: epi == BF16, tiles <= 128, K >= 2048; K is no multiple of 64
FWD_CASES = ([dict(shape=s, epi=e, bias=b, drop=False) for s in FWD_SHAPES for e in (EPI_BF16, EPI_BF16_RELU) for b in (True, False)]
             + [dict(shape=FWD_8WAVE, epi=EPI_BF16, bias=b, drop=False) for b in (True, False)]
             + [dict(shape=s, epi=EPI_F32, bias=True, drop=False) for s in FWD_SHAPES + [FWD_8WAVE, (33, 132, 40)]]
             + [dict(shape=(33, 132, 40), epi=EPI_F32, bias=False, drop=False)]
             + [dict(shape=(129, 264, 72), epi=EPI_BF16_RELU, bias=True, drop=True)])


def fwd_id(c):
    return "%s-%dx%dx%d-%s%s%s" % (("bf16", "relu", "f32")[c["epi"]], *c["shape"], "bias" if c["bias"] else "nobias",
                                   "-drop" if c["drop"] else "", "-8wave" if c["shape"] == FWD_8WAVE and c["epi"] == EPI_BF16 else "")


def build_fwd(c, salt=11):
    """st_gemm forward (0, 0): D = epilogue(X W^T + bias)."""
    M, N, K = c["shape"]
    X, W, acc, bound = _xw("fwd", M, N, K)
    b = eighths(_gen("fwd-bias", M, N, K), (N,), 8) if c["bias"] else None
    v = acc + (b.to(F64) if b is not None else 0.0)
    bound = bound + (b.to(F64).abs() if b is not None else 0.0)
    conds = [("sum |x||w| + |bias|", bound)]
    if c["epi"] == EPI_BF16_RELU:
        v = torch.relu(v)
        if c["drop"]:
            v = v * keep(salt, M, N) * 2.0
            conds.append(("survivors x 2", bound * 2.0))
    return Built(dict(X=X, W=W, bias=b), dict(D=v), {}, conds)


# dgrad (0, 1): dx [M, out] = dy [M, C] W [C, out]
DGRAD_SHAPES = [(127, 72, 136), (129, 520, 264), (64, 4344, 256)]
# the head widths 32 / 64 / 128 must divide the output width: 136 and 264 take none of them, so the DELTA epilogue runs at
# the same row counts and contractions with the next width that does (128, 256)
DELTA_SHAPES = [(127, 72, 128), (129, 520, 256), (64, 4344, 256)]
# BF16 / MASK / ADD carry a bias (the header's D = epilogue(acc + bias); it puts ties below 256, where integer sums have none);
# the form production calls - no bias - runs at the long contraction, whose sums pass 256 by themselves
_DG = [(s, True) for s in DGRAD_SHAPES] + [(DGRAD_SHAPES[2], False)]
DGRAD_CASES = ([dict(shape=s, epi=EPI_BF16, bias=b) for s, b in _DG]
               + [dict(shape=s, epi=EPI_BF16_MASK, scale=sc, bias=b) for s, b in _DG for sc in (1.0, 2.0)]
               + [dict(shape=s, epi=EPI_BF16_ADD, alias=al, bias=b) for s, b in _DG for al in (False, True)]
               + [dict(shape=s, epi=EPI_BF16_DELTA, hd=hd, aux2=a2) for s in DELTA_SHAPES for hd in (32, 64, 128) for a2 in (False, True)])


def dgrad_id(c):
    tag = {EPI_BF16: "bf16", EPI_BF16_MASK: "mask-x%g" % c.get("scale", 1), EPI_BF16_ADD: "add-%s" % ("inplace" if c.get("alias") else "separate"),
           EPI_BF16_DELTA: "delta-hd%d%s" % (c.get("hd", 0), "-aux2" if c.get("aux2") else "")}[c["epi"]]
    return "%s-%dx%dx%d%s" % (tag, *c["shape"], "" if c["epi"] == EPI_BF16_DELTA else "-bias" if c["bias"] else "-nobias")


def build_dgrad(c):
    M, C, N = c["shape"]
    W, X, acct, boundt = _xw("dgrad", N, M, C)          # W^T [N, C] and dy [M, C] of the cached pair: acc = dy W
    acc, bound = acct.t().contiguous(), boundt.t().contiguous()
    ops = dict(dy=X, W=W.t().contiguous(), bias=None)
    epi = c["epi"]
    gen = _gen("dgrad-aux", M, C, N, epi)
    if c.get("bias"):
        ops["bias"] = eighths(gen, (N,), 8)
        acc, bound = acc + ops["bias"].to(F64), bound + ops["bias"].to(F64).abs()
    conds, alts = [("sum |dy||w| + |bias|", bound)], {}
    if epi == EPI_BF16:
        refs = dict(D=acc)
    elif epi == EPI_BF16_MASK:
        ops["aux"] = ints(gen, (M, N))                  # zeros, negatives and positives
        refs = dict(D=acc * c["scale"] * (ops["aux"].to(F64) > 0))
        conds.append(("survivors x drop_scale", bound * c["scale"]))
    elif epi == EPI_BF16_ADD:
        ops["aux"] = ints(gen, (M, N))
        once = rne64(acc)                               # the header's contract: D = bf16(bf16(acc + bias) + aux)
        refs = dict(D=once + ops["aux"].to(F64))
        alts["D"] = {"one rounding of acc + aux": acc + ops["aux"].to(F64)}
        conds.append(("bf16(acc + bias) + aux", once.abs() + ops["aux"].to(F64).abs()))
    else:
        hd = c["hd"]
        ops["aux"] = ints(gen, (M, N))
        ops["aux2"] = eighths(gen, (M, N), 1, BF16) if c["aux2"] else None
        o = ops["aux"].to(F64) + (ops["aux2"].to(F64) if c["aux2"] else 0.0)
        d = rne64(acc)                                  # delta is computed from the ROUNDED D
        refs = dict(D=acc, delta=(d * o).view(M, N // hd, hd).sum(-1).t().contiguous().view(-1))
        alts["delta"] = {"delta from the unrounded D": (acc * o).view(M, N // hd, hd).sum(-1).t().contiguous().view(-1)}
        conds += [("aux + aux2", o), ("sum |D||aux + aux2| per head", (d.abs() * o.abs()).view(M, N // hd, hd).sum(-1))]
    return Built(ops, refs, alts, conds, acc if epi == EPI_BF16_ADD else None)


# wgrad (1, 1): dW [N_out, K_in] += dy^T x over `tokens` rows
WGRAD_CASES = [dict(tokens=t, splits=s, out=o) for t in (1, 63, 65, 1000) for s in (1, 3, 40) for o in ((136, 72), (264, 520))]


def wgrad_id(c):
    return "tokens%d-splits%d-%dx%d" % (c["tokens"], c["splits"], *c["out"])


def build_wgrad(c, key="wgrad"):
    T, (N, K) = c["tokens"], c["out"]
    gen = _gen(key, T, N, K)
    dy, x = ints(gen, (T, N)), ints(gen, (T, K))
    init, b0 = ints(gen, (N, K), -64, 64, F32), ints(gen, (N,), -64, 64, F32)
    refs = dict(dW=init.to(F64) + dy.to(F64).t() @ x.to(F64), db=b0.to(F64) + dy.to(F64).sum(0))
    conds = [("|existing| + sum |dy||x|", init.to(F64).abs() + dy.to(F64).abs().t() @ x.to(F64).abs()),
             ("|existing| + sum |dy|", b0.to(F64).abs() + dy.to(F64).abs().sum(0))]
    return Built(dict(dy=dy, x=x, init=init, b0=b0), refs, {}, conds)


SPLITK_CASES = [dict(shape=s, splits=sp, ycm=y) for (s, sp) in (((130, 264, 2104), 3), ((5, 136, 520), 9)) for y in (False, True)]


def splitk_id(c):
    return "%dx%dx%d-splits%d-%s" % (*c["shape"], c["splits"], "ycm" if c["ycm"] else "natural")


def build_splitk(c):
    M, N, K = c["shape"]
    X, W, acc, bound = _xw("splitk", M, N, K)
    return Built(dict(X=X, Y=W.t().contiguous() if c["ycm"] else W), dict(D=acc), {}, [("sum |x||y|", bound)])


KSCALE_CASES = [dict(shape=(129, 768, 256), cols=cols, scale=s) for cols in ((256, 512), (32, 160)) for s in SCALES]


def kscale_id(c):
    return "cols%d-%d-x%g" % (*c["cols"], c["scale"])


def build_kscale(c, key="kscale"):
    """(X W^T + bias), columns [lo, hi) times scale, rounded once (st_gemm_kscale; st_row_chain's POST stage with post_kscale)."""
    M, N, K = c["shape"]
    X, W, acc, bound = _xw(key, M, N, K)
    b = eighths(_gen(key + "-bias", M, N, K), (N,), 8)
    v, bound = acc + b.to(F64), bound + b.to(F64).abs()
    conds = [("sum |x||w| + |bias|", bound)]
    if c["cols"] is not None:
        lo, hi = c["cols"]
        v = v.clone()
        v[:, lo:hi] *= c["scale"]
        conds.append(("(acc + bias) x scale", bound[:, lo:hi] * c["scale"]))
    return Built(dict(X=X, W=W, bias=b), dict(D=v), {}, conds)


# st_gemm_stacked: forward 3 blocks of 128 rows, K = 72, M = 129; dgrad 2 blocks of 128 (plain and with the addend)
STACKED_CASES = [dict(kind="fwd", M=129, blocks=3, rows=128, K=72), dict(kind="dgrad", M=129, blocks=2, rows=128, K=72, epi=EPI_BF16),
                 dict(kind="dgrad", M=129, blocks=2, rows=128, K=72, epi=EPI_BF16_ADD)]


def stacked_id(c):
    return "%s-%dblocks%s" % (c["kind"], c["blocks"], "-add" if c.get("epi") == EPI_BF16_ADD else "")


def stack_arena(gen, blocks, rows, K, lead=64, gap=4096 + 64, bias_lead=32, bias_gap=192):
    """`blocks` weight blocks [rows, K] (and their bias blocks) lying further apart than rows * ld, NaN between them.
    -> (arena_w, w_offset, w_stride, arena_b, b_offset, b_stride, the gathered stack [blocks rows, K], the gathered bias)."""
    w_stride, b_stride = rows * K + gap, rows + bias_gap
    aw = torch.full((lead + blocks * w_stride + 128,), float("nan"), dtype=BF16)
    ab = torch.full((bias_lead + blocks * b_stride + 64,), float("nan"), dtype=F32)
    ws, bs = [], []
    for l in range(blocks):
        w, b = ints(gen, (rows, K)), eighths(gen, (rows,), 8)
        aw[lead + l * w_stride:lead + l * w_stride + rows * K] = w.reshape(-1)
        ab[bias_lead + l * b_stride:bias_lead + l * b_stride + rows] = b
        ws.append(w), bs.append(b)
    return aw, lead, w_stride, ab, bias_lead, b_stride, torch.cat(ws), torch.cat(bs)


def build_stacked(c):
    M, blocks, rows, K = c["M"], c["blocks"], c["rows"], c["K"]
    gen = _gen("stacked", c["kind"], c.get("epi"), M, blocks, rows, K)
    aw, w_off, w_stride, ab, b_off, b_stride, Wcat, bcat = stack_arena(gen, blocks, rows, K)
    ops = dict(arena_w=aw, w_off=w_off, w_stride=w_stride, arena_b=ab, b_off=b_off, b_stride=b_stride)
    w = Wcat.to(F64)
    if c["kind"] == "fwd":          # more output columns
        X = ints(gen, (M, K))
        ops["X"] = X
        bound = X.to(F64).abs() @ w.abs().t() + bcat.to(F64).abs()
        return Built(ops, dict(D=X.to(F64) @ w.t() + bcat.to(F64)), {}, [("sum |x||w| + |bias|", bound)])
    dy = ints(gen, (M, blocks * rows))          # a longer contraction
    ops["dy"] = dy
    ops["bias"] = eighths(gen, (K,), 8)          # (a dgrad's bias is one plain [K] vector: only a forward's is stacked)
    acc, bound = dy.to(F64) @ w + ops["bias"].to(F64), dy.to(F64).abs() @ w.abs() + ops["bias"].to(F64).abs()
    if c["epi"] == EPI_BF16:
        return Built(ops, dict(D=acc), {}, [("sum |dy||w| + |bias|", bound)])
    ops["aux"] = ints(gen, (M, K))
    once = rne64(acc)
    return Built(ops, dict(D=once + ops["aux"].to(F64)), {"D": {"one rounding of acc + aux": acc + ops["aux"].to(F64)}},
                 [("sum |dy||w| + |bias|", bound), ("bf16(acc + bias) + aux", once.abs() + ops["aux"].to(F64).abs())], acc)


# st_gemm_ws: K = 256, chunks of 32 rows, ranks = min(512 / (N / 256), chunks); (4101, 1024): 128 ranks, 129 chunks
WS_SHAPES = [(m, n) for m in (1, 31, 33) for n in (256, 768)] + [(4101, 1024)]
WS_CASES = ([dict(shape=s, relu=r, drop=False, stack=None) for s in WS_SHAPES for r in (False, True)]
            + [dict(shape=(33, 768), relu=True, drop=True, stack=None), dict(shape=(33, 512), relu=False, drop=False, stack=(2, 256))])


def ws_id(c):
    return "%dx%d-%s%s%s" % (*c["shape"], "relu" if c["relu"] else "identity", "-drop" if c["drop"] else "", "-stacked" if c["stack"] else "")


def build_ws(c, salt=11):
    M, N = c["shape"]
    K = 256
    if c["stack"]:
        blocks, rows = c["stack"]
        gen = _gen("ws-stacked", M, N)
        aw, w_off, w_stride, ab, b_off, b_stride, W, b = stack_arena(gen, blocks, rows, K)
        X = ints(gen, (M, K))
        ops = dict(X=X, arena_w=aw, w_off=w_off, w_stride=w_stride, arena_b=ab, b_off=b_off, b_stride=b_stride, W=W, bias=b)
        acc, bound = X.to(F64) @ W.to(F64).t(), X.to(F64).abs() @ W.to(F64).abs().t()
    else:
        X, W, acc, bound = _xw("ws", M, N, K)
        b = eighths(_gen("ws-bias", M, N), (N,), 8)
        ops = dict(X=X, W=W, bias=b)
    v, bound = acc + b.to(F64), bound + b.to(F64).abs()
    conds = [("sum |x||w| + |bias|", bound)]
    if c["relu"]:
        v = torch.relu(v)
        if c["drop"]:
            v = v * keep(salt, M, N) * 2.0
            conds.append(("survivors x 2", bound * 2.0))
    return Built(ops, dict(D=v), {}, conds)


# st_wgrad_group / st_wgrad_wide: (tokens, N_out, K_in, splits)
GROUP_PROBLEMS = [(1, 8, 8, 1), (33, 264, 72, 3), (300, 520, 256, 5), (1000, 296, 200, 7)]
GROUP_CASES = [dict(wide=w, problems=GROUP_PROBLEMS, bias=b) for w in (False, True) for b in (True, False)] + \
              [dict(wide=w, problems=[(33, 264, 72, 3)] * 49, bias=True) for w in (False, True)]          # 49 > GROUP_MAX / WIDE_MAX


def group_id(c):
    return "%s-%dproblems-%s" % ("wide" if c["wide"] else "group", len(c["problems"]), "bias" if c["bias"] else "nobias")


def build_group(c):
    """One Built per problem; every copy of a repeated problem has operands of its own."""
    return [build_wgrad(dict(tokens=t, out=(n, k)), key=("group", q)) for q, (t, n, k, sp) in enumerate(c["problems"])]


# st_gemm_ln, the `pre` output: one shape per kernel variant (csrc/st_gemm_ln.hip, st_gemm_ln's dispatch)
LN_SHAPES = [((33, 128, 72), "n128"), ((130, 128, 520), "n128-ksplit"), ((33, 256, 72), "n256"), ((130, 256, 520), "n256-ksplit"),
             ((16500, 256, 520), "n256-tall"), ((33, 512, 72), "n512"), ((8250, 512, 520), "n512-tall64"),
             ((8230, 512, 1032), "n512-tall128")]
LN_CASES = ([dict(shape=s, variant=v, res=r, relu=a, drop=False) for s, v in LN_SHAPES for r in (True, False) for a in (False, True)]
            + [dict(shape=(130, 256, 520), variant="n256-ksplit", res=True, relu=True, drop=True)])


def ln_id(c):
    return "%s-%dx%dx%d-%s-%s%s" % (c["variant"], *c["shape"], "res" if c["res"] else "nores", "relu" if c["relu"] else "id",
                                    "-drop1" if c["drop"] else "")


def build_ln(c, salt=6):
    """pre = bf16(act(X W^T + bias) + res), with drop_where = 1 the dropout between the activation and the residual."""
    M, N, K = c["shape"]
    X, W, acc, bound = _xw("ln", M, N, K)
    gen = _gen("ln-vec", M, N, K)
    b = eighths(gen, (N,), 8)
    gamma, beta = 1 + eighths(gen, (N,), 1) / 4, eighths(gen, (N,), 1)
    res = ints(_gen("ln-res", M, N, K), (M, N)) if c["res"] else None
    v, bound = acc + b.to(F64), bound + b.to(F64).abs()
    conds = [("sum |x||w| + |bias|", bound)]
    if c["relu"]:
        v = torch.relu(v)
    if c["drop"]:
        v, bound = v * keep(salt, M, N) * 2.0, bound * 2.0
        conds.append(("survivors x 2", bound))
    if res is not None:
        v = v + res.to(F64)
        conds.append(("act(acc + bias) + res", bound + res.to(F64).abs()))
    return Built(dict(X=X, W=W, bias=b, res=res, gamma=gamma, beta=beta), dict(pre=v), {}, conds)


# st_row_chain with only the POST stage, three 256-row blocks (the encoder's layer-0 q | k | v projection): P = A Wp^T + bp, the key
# block [256, 512) times post_kscale before its one rounding.  The row counts at which the chain kernels change.
CHAIN_CASES = [dict(M=m, split=sp, scale=s) for (m, sp) in ((5, False), (320, False), (3120, False), (9000, False), (3120, True))
               for s in (None,) + SCALES]


def chain_id(c):
    return "post3-M%d%s-%s" % (c["M"], "-split" if c["split"] else "", "plain" if c["scale"] is None else "ks%g" % c["scale"])


def build_chain(c):
    return build_kscale(dict(shape=(c["M"], 768, 256), cols=None if c["scale"] is None else (256, 512), scale=c["scale"]), key="chain")


def mfma_operands(lo, hi):
    """st_probe_mfma's operands A [32, 16], Bt [32, 16] with integers in [lo, hi] (every one a bf16 value: |v| <= 256)."""
    gen = _gen("mfma", lo, hi)
    return ints(gen, (32, 16), lo, hi), ints(gen, (32, 16), lo, hi)


# every case that yields ONE Built, with the id the tests show: (family, id, case, builder)
def all_cases():
    fams = (("fwd", FWD_CASES, fwd_id, build_fwd), ("dgrad", DGRAD_CASES, dgrad_id, build_dgrad), ("wgrad", WGRAD_CASES, wgrad_id, build_wgrad),
            ("splitk", SPLITK_CASES, splitk_id, build_splitk), ("kscale", KSCALE_CASES, kscale_id, build_kscale),
            ("stacked", STACKED_CASES, stacked_id, build_stacked), ("ws", WS_CASES, ws_id, build_ws), ("ln", LN_CASES, ln_id, build_ln),
            ("chain", CHAIN_CASES, chain_id, build_chain))
    return [(f, idf(c), c, b) for f, cases, idf, b in fams for c in cases]


def bf16_output(family, case):
    """The case's main output is bf16 (rounded once): wgrad accumulators and EPI_F32 are fp32."""
    return family != "wgrad" and case.get("epi") != EPI_F32
