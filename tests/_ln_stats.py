"""Row families and checks of the LayerNorm-statistic tests: every kernel that forms a LayerNorm behind a GEMM - st_gemm_ln, the
LayerNorm stages of st_row_chain (32-row, split, pipelined 64- / 96-row kernels) and st_row_chain512, the PRE stage of st_attn_f1_fwd -
against the plain fp64 reference tests/_ln_ref.py on rows that are NOT N(0, 1): off-centre (|row mean| = rho row std), of tiny spread
(variance comparable to eps and far below it) and constant.  Shared by tests/test_ln_stats_gpu.py (the kernels),
tests/test_ln_stats_cpu.py (the emulation, with defects injected, so that the checks are known to see them) and tools/local_bounds.py
(family "ln_stats").  A ``Backend`` says whose gemm_ln / row_chain / attn_f1_fwd run and where; operands, guards, references and
assertions are the same code for all of them.

A chain is referenced stage by stage FROM THE TENSORS THE KERNEL ITSELF WROTE for the stage before (the second LayerNorm from the
kernel's H and out0, as tests/test_kernels_gpu.py::_delta_of takes the O the kernel read): an upstream bf16 rounding is not charged to
the statistic.

Bounds - none is tuned against a kernel (tests/LOCAL_BOUNDS.md, "The LayerNorm statistic off centre and at tiny spread"):
  rstd            |got / ref - 1| <= L_RSTD = 1e-4, element by element.  An fp32 sum of N <= 512 squares in any order is within
                  N 2^-24 = 3.1e-5 of the variance = 1.5e-5 of rstd, the reciprocal square root adds an ulp, the fp32 accumulation of v at
                  the offset's magnitude adds what the fp32 emulation shows against fp64 (at most 2.8e-6 over all families).  The defects
                  the bound is there for stand at 1.3e-4 (one-pass variance at rho = 32, the worst of 70 rows; 2.4e-4 over thousands
                  of rows) and above.
  out, xhat, pre  L_BF16 = 1e-2, whole tensor and row by row / column by column, against the UNROUNDED reference: single-rounding
                  outputs (the rounding alone takes ~2e-3 of a row).
  constant rows   xhat +0 or -0 in every element, out = bf16(beta) bit for bit, rstd = eps^-1/2 within L_RSTD.
  exact           guards intact, everything finite."""
import contextlib
import functools
import types

import torch

from tests import _emul as em
from tests import _ln_ref as ref
from tests._local import Guarded, check, guarded_input, local_figures

BF16, F32, F64, I32 = torch.bfloat16, torch.float32, torch.float64, torch.int32

L_RSTD = 1e-4
L_BF16 = 1e-2

# ---- the row families --------------------------------------------------------------------------------------------------------------------
# rho: the constant rho sigma is added to the fp32 bias (exact: no operand is quantised by it), sigma = the median row std of the
#      centred case; res_add: a constant added to the residual BEFORE its rounding to bf16 (64.0 is representable; the rest of the
#      residual is then quantised to the bf16 step at 64 - an input property, the reference reads the same operand);
# tau: X, res and the bias scaled by it (variance ~3e-6 at 1e-3: comparable to eps; ~3e-10 at 1e-5: eps rules);
# const: bias = 3.0 in every column and a band of rows with X = 0 and res = 0 - rows whose every value is 3.0 exactly.
FAMILIES = {
    "centred": {},
    "offset8": dict(rho=8.0),
    "offset32": dict(rho=32.0),
    "offset128": dict(rho=128.0),
    "offset512": dict(rho=512.0),
    "res64": dict(res_add=64.0),
    "spread1e-3": dict(tau=1e-3),
    "spread1e-3-eps1e-5": dict(tau=1e-3, eps=1e-5),
    "spread1e-5": dict(tau=1e-5),
    "offset32-spread1e-3": dict(rho=32.0, tau=1e-3),
    "constant": dict(const=True),
}
F1_FAMILIES = ("centred", "offset128", "spread1e-3")

# ---- the implementations, each at the smallest shape that selects it -----------------------------------------------------------------------
# one_pass: the statistic comes from one pass over the row (csrc/st_rowchain_pipe.cuh, st_rowchain_pipe512.cuh); all others take the
# mean first and the squared deviations then.
IMPLS = {
    "gemm_ln-res-n128": dict(kind="gemm_ln", M=70, N=128, K=128),
    "gemm_ln-res-n256": dict(kind="gemm_ln", M=70, N=256, K=256),
    "gemm_ln-res-n512": dict(kind="gemm_ln", M=70, N=512, K=512),
    "gemm_ln-ksplit": dict(kind="gemm_ln", M=130, N=256, K=512),                  # K >= 512, M <= 8,192: the 8-wave K split
    "gemm_ln-tiles-n256": dict(kind="gemm_ln", M=8250, N=256, K=80),              # (N = 256, short contraction: the plain 4-wave kernel over many row tiles)
    "gemm_ln-tiles-n512": dict(kind="gemm_ln", M=8250, N=512, K=512),             # N = 512, M > 8,192, K < 1,024: 64-row tiles on 8 waves
    "gemm_ln-tall-n256": dict(kind="gemm_ln", M=16400, N=256, K=512),             # N = 256, K >= 512, 16,384 < M <= 32,768: 128-row tiles on 8 waves
    "gemm_ln-tall-n512": dict(kind="gemm_ln", M=8250, N=512, K=1024),             # N = 512, M > 8,192, K >= 1,024: 128-row tiles on 8 waves
    "gemm_ln-relu_pe": dict(kind="gemm_ln", M=70, N=256, K=256, relu_pe=True),
    "chain-32row": dict(kind="chain", d=256, M=70),
    "chain-split": dict(kind="chain", d=256, M=70, split=True),                    # (d_ff 256 is ONE hidden chunk: the scratch is ignored, the 32-row kernel runs)
    "chain-split-dff512": dict(kind="chain", d=256, M=70, d_ff=512, split=True),   # two hidden chunks: row_chain_split_kernel, 3 row blocks x 2 workgroups
    "chain-pipe64": dict(kind="chain", d=256, M=8200, one_pass=True),             # 8,192 < M <= 16,384: 64-row workgroups
    "chain-pipe96": dict(kind="chain", d=256, M=16400, one_pass=True),            # M > 16,384: 96-row workgroups
    "chain512": dict(kind="chain", d=512, M=70, one_pass=True),
    "attn_f1-short-keys": dict(kind="f1", case="short-keys"),                     # (too few keys for the fused kernel: the two launches)
    "attn_f1-train": dict(kind="f1", case="train"),                               # ... and the fused launch of csrc/st_attn_xs.hip
}
D_FF = 256            # of every chain but the one whose impl names its own


def cases():
    """[(id, dict(impl=, family=))]: every family through every implementation (relu_pe has no residual; st_attn_f1_fwd: three)."""
    out = []
    for iid, impl in IMPLS.items():
        for fam in (F1_FAMILIES if impl["kind"] == "f1" else FAMILIES):
            if fam == "res64" and impl.get("relu_pe"):
                continue
            out.append(("%s-%s" % (iid, fam), dict(impl=iid, family=fam)))
    return out


def g(*shape, seed=0, scale=1.0, dtype=BF16):
    """The seeded operands of tests/test_kernels_gpu.py."""
    gen = torch.Generator().manual_seed(seed)
    return (torch.randn(*shape, generator=gen) * scale).to(dtype)


def band(M):
    """The constant rows: a band across the first 32-row tile boundary and the last two rows (a ragged last tile)."""
    rows = torch.zeros(M, dtype=torch.bool)
    rows[30:38] = True
    rows[M - 2:] = True
    return rows


def _f1_lengths(case):
    gen = torch.Generator().manual_seed(11)
    if case == "short-keys":
        return torch.randint(3, 50, (5,), generator=gen), torch.randint(40, 200, (5,), generator=gen)
    q_len, k_len = torch.randint(1, 64, (9,), generator=gen), torch.randint(260, 1000, (9,), generator=gen)
    q_len[0], q_len[1], k_len[0] = 64, 33, 999
    return q_len, k_len


def _centred_operands(iid):
    """The centred case's operands (float32 where a family still has to scale or shift them before the one rounding to bf16)."""
    impl = IMPLS[iid]
    o = types.SimpleNamespace(impl=impl, id=iid, kind=impl["kind"])
    if o.kind == "gemm_ln":
        M, N, K = impl["M"], impl["N"], impl["K"]
        o.M, o.N = M, N
        o.X, o.W = g(M, K, seed=1, dtype=F32), g(N, K, seed=2, scale=K ** -0.5)
        o.bias, o.gamma, o.beta = g(N, seed=3, dtype=F32), 1 + 0.2 * g(N, seed=4, dtype=F32), 0.2 * g(N, seed=5, dtype=F32)
        o.relu = bool(impl.get("relu_pe"))
        o.res = None if o.relu else g(M, N, seed=6, dtype=F32)
        o.pe = g(64, N, seed=7, dtype=F32) if o.relu else None
        o.pos = (torch.arange(M) % 64).to(I32) if o.relu else None
        return o
    d = impl.get("d", 256)
    if o.kind == "f1":
        o.q_len, o.k_len = _f1_lengths(impl["case"])
        M = int(o.q_len.sum())
        o.H = 4
        o.wo, o.wq = g(d, d, seed=1, scale=d ** -0.5), g(d, d, seed=2, scale=d ** -0.5)
        o.bo, o.bq = g(d, seed=3, dtype=F32), g(d, seed=4, dtype=F32)
        o.g0, o.be0 = g(d, seed=5, dtype=F32) * 0.2 + 1, g(d, seed=6, dtype=F32) * 0.1
        o.A, o.R, o.kv = g(M, d, seed=7, dtype=F32), g(M, d, seed=8, dtype=F32), g(int(o.k_len.sum()), 2 * d, seed=9)
    else:
        M = impl["M"]
        o.d_ff = dff = impl.get("d_ff", D_FF)
        o.wo, o.w1, o.w2 = g(d, d, seed=1, scale=d ** -0.5), g(dff, d, seed=2, scale=d ** -0.5), g(d, dff, seed=3, scale=dff ** -0.5)
        o.bo, o.b1, o.b2 = g(d, seed=5, dtype=F32), g(dff, seed=6, dtype=F32), g(d, seed=7, dtype=F32)
        o.g0, o.be0 = g(d, seed=9, dtype=F32) * 0.2 + 1, g(d, seed=10, dtype=F32) * 0.1
        o.g1, o.be1 = g(d, seed=11, dtype=F32) * 0.2 + 1, g(d, seed=12, dtype=F32) * 0.1
        o.A, o.R = g(M, d, seed=13, dtype=F32), g(M, d, seed=14, dtype=F32)
    o.M, o.N = M, d
    return o


@functools.lru_cache(maxsize=None)
def sigmas(iid):
    """(sigma of the first LayerNorm, of the second): the median row std of the centred case, in fp64."""
    o = _centred_operands(iid)
    if o.kind == "gemm_ln":
        r = ref.gemm_ln(o.X.to(BF16), o.W, o.bias, None if o.res is None else o.res.to(BF16), o.gamma, o.beta, 1e-6, relu=o.relu)
        return float(r["var"].sqrt().median()), None
    r = ref.gemm_ln(o.A.to(BF16), o.wo, o.bo, o.R.to(BF16), o.g0, o.be0, 1e-6)
    s1 = float(r["var"].sqrt().median())
    if o.kind == "f1":
        return s1, None
    out0 = r["out"].to(BF16)
    r2 = ref.gemm_ln(ref.hidden(out0, o.w1, o.b1).to(BF16), o.w2, o.b2, out0, o.g1, o.be1, 1e-6)
    return s1, float(r2["var"].sqrt().median())


def _apply(fam, X, bias, res, sigma, M):
    """One LayerNorm's operands under a family: -> X bf16, bias fp32, res bf16 (or None), the constant rows (or None)."""
    tau, rho = fam.get("tau", 1.0), fam.get("rho", 0.0)
    X, bias = X.clone(), bias.clone()
    res = None if res is None else res.clone()
    rows = None
    if fam.get("const"):
        rows = band(M)
        bias.fill_(3.0)
        X[rows] = 0
        if res is not None:
            res[rows] = 0
    if res is not None:
        res = ((res + fam.get("res_add", 0.0)) * tau).to(BF16)
    bias = ((bias.double() + rho * sigma) * tau).to(F32)
    return (X * tau).to(BF16), bias, res, rows


def build(impl, family):
    """One case: the operands as the kernel gets them.  (The spread families apply to the first LayerNorm of a chain only - its
    residual carries an O(1) out0 into the second; the offsets apply to both.)"""
    fam = FAMILIES[family]
    c = _centred_operands(impl)
    c.family, c.id, c.eps = family, "%s-%s" % (impl, family), fam.get("eps", 1e-6)
    c.one_pass = bool(c.impl.get("one_pass"))
    s1, s2 = sigmas(impl)
    if c.kind == "gemm_ln":
        c.X, c.bias, c.res, c.const = _apply(fam, c.X, c.bias, c.res, s1, c.M)
        return c
    c.A, c.bo, c.R, c.const = _apply(fam, c.A, c.bo, c.R, s1, c.M)
    if c.kind == "chain":
        c.b2 = (c.b2.double() + fam.get("rho", 0.0) * s2).to(F32)
    return c


# ---- backends ---------------------------------------------------------------------------------------------------------------------------
class Backend:
    """Whose kernels run, on which device.  gemm_ln: a function with tests._emul.gemm_ln's signature (the emulation, or one with a
    defect); the emulated chains are composed of it.  gpu: st_amd.native."""

    def __init__(self, device, gemm_ln=None, dtype=None, gpu=False):
        self.device, self.dtype, self.gpu = device, dtype, gpu
        self._gemm_ln = gemm_ln

    def _kw(self, kw):
        return kw if self.dtype is None else dict(kw, dtype=self.dtype)

    @contextlib.contextmanager
    def _swapped(self):
        saved = em.gemm_ln
        try:
            em.gemm_ln = self._gemm_ln
            yield
        finally:
            em.gemm_ln = saved

    def gemm_ln(self, *a, **kw):
        if self.gpu:
            from st_amd import native as nv
            return nv.gemm_ln(*a, **kw)
        return self._gemm_ln(*a, **self._kw(kw))

    def row_chain(self, *a, **kw):
        if self.gpu:
            from st_amd import native as nv
            return nv.row_chain(*a, **kw)
        with self._swapped():
            return em.row_chain(*a, **self._kw(kw))

    def attn_f1_fwd(self, *a, **kw):
        if self.gpu:
            from st_amd import native as nv
            return nv.attn_f1_fwd(*a, **kw)
        with self._swapped():
            return em.attn_f1_fwd(*a, **kw)

    def chain(self, blocks, split=False):
        from st_amd import chains
        blocks = blocks(self.device)
        if not self.gpu:
            return chains.Chain(None, len(blocks), blocks)
        from st_amd import native as nv
        cs = chains.ChainSet(self.device)
        cid = cs.add(blocks)
        cs.finalize().rebuild()
        ch = cs.chain(cid)
        if split:          # the scratch of the split kernel: with it, a chain of two or more hidden chunks runs one workgroup per chunk and row block
            ch.split_work = torch.zeros(nv.split_work_words(), dtype=I32, device=self.device)
        return ch

    def mask_words(self, M, d, d_ff):
        if self.gpu:
            from st_amd import native as nv
            return nv.chain_mask_words(M, d_ff, d)
        return em.chain_mask_words(M, d_ff, d)


CPU = Backend("cpu", gemm_ln=em.gemm_ln, dtype=F32)            # the emulation as the other kernel tests use it


def cpu_backend(gemm_ln):
    return Backend("cpu", gemm_ln=gemm_ln, dtype=F32)


def gpu_backend():
    return Backend("cuda", gpu=True)


# ---- running a case -------------------------------------------------------------------------------------------------------------------
def _go(rows, cols, dev, contiguous=False):
    return Guarded(rows, cols, BF16, dev, pad_cols=(0, 0) if contiguous else (64, 64))


def launch(c, be, split=None):
    """The case by the backend's kernels: outputs in guards, bf16 operands in NaN surroundings.  -> {output name: Guarded}
    split: hand the chain the split kernel's scratch or not (None: as the implementation says)."""
    dev = be.device
    mv = lambda t: None if t is None else t.to(dev)
    GI = lambda t, **kw: None if t is None else guarded_input(t, dev, **kw)
    M, N = c.M, c.N
    if c.kind == "gemm_ln":      # out takes any leading dimension; xhat / pre are [M, N] exactly (row guards)
        gd = dict(out=_go(M, N, dev), xhat=_go(M, N, dev, True), rstd=Guarded.vec(M, F32, dev), pre=_go(M, N, dev, True))
        be.gemm_ln(GI(c.X), mv(c.W), mv(c.bias), GI(c.res), mv(c.gamma), mv(c.beta), gd["out"].view, gd["xhat"].view, gd["rstd"].view,
                   eps=c.eps, relu=c.relu, pe=mv(c.pe), pos=mv(c.pos), pre=gd["pre"].view)
        return gd
    from st_amd import chains
    a_in, r_in = GI(c.A, pad_cols=(32, 32)), GI(c.R, pad_cols=(0, 8))
    if c.kind == "f1":
        from st_amd.functional import Rows, attn_work
        H, d = c.H, N
        q_rows, k_rows = Rows.packed(c.q_len, dev), Rows.packed(c.k_len, dev)
        ch = be.chain(lambda dv: chains.blocks_of(c.wo.to(dv)) + chains.blocks_of(c.wq.to(dv)))
        work = attn_work(q_rows, k_rows, False, d // H, H)[0] if be.gpu else None
        kv = mv(c.kv)
        gd = dict(out0=_go(M, d, dev, True), xhat0=_go(M, d, dev, True), rstd0=Guarded.vec(M, F32, dev), q=_go(M, d, dev),
                  O=_go(M, d, dev, True), ores=_go(M, d, dev, True), lse=Guarded.vec(H * M, F32, dev))
        be.attn_f1_fwd(a_in, ch, (r_in, mv(c.bo), mv(c.g0), mv(c.be0), gd["out0"].view, gd["xhat0"].view, gd["rstd0"].view),
                       (1, mv(c.bq), gd["q"].view), kv[:, :d], kv[:, d:], gd["O"].view, gd["lse"].view, q_rows.off, q_rows.len, k_rows.off,
                       k_rows.len, H, int(c.q_len.max()), (d // H) ** -0.5, work=work, max_k=int(c.k_len.max()), ores=gd["ores"].view,
                       eps=c.eps)
        return gd
    d = N
    if d == 512:
        ch = be.chain(lambda dv: chains.encoder512_blocks(c.wo.to(dv), c.w1.to(dv), c.w2.to(dv), None))
    else:
        ch = be.chain(lambda dv: chains.blocks_of(c.wo.to(dv)) + chains.ffn_blocks(c.w1.to(dv), c.w2.to(dv)), split=bool(c.impl.get("split")) if split is None else split)
    gd = dict(out0=_go(M, d, dev, True), xhat0=_go(M, d, dev, True), rstd0=Guarded.vec(M, F32, dev), H=_go(M, c.d_ff, dev, True),
              out1=_go(M, d, dev, True), xhat1=_go(M, d, dev, True), rstd1=Guarded.vec(M, F32, dev))
    bits = (torch.zeros(be.mask_words(M, d, c.d_ff), dtype=torch.int64, device=dev),) if be.gpu else ()
    be.row_chain(a_in, ch, pre=(r_in, mv(c.bo), mv(c.g0), mv(c.be0), gd["out0"].view, gd["xhat0"].view, gd["rstd0"].view),
                 ffn=(c.d_ff, mv(c.b1), mv(c.b2), mv(c.g1), mv(c.be1), gd["H"].view, gd["out1"].view, gd["xhat1"].view, gd["rstd1"].view,
                      None, None) + bits, eps=c.eps)
    return gd


def references(c, got):
    """[(stage name, {output name of ``got``: fp64 reference}, the stage's beta as ``out`` shows it in a constant row or None)]:
    each stage from the operands the kernel read - the case's own for the first, the kernel's outputs for the later ones."""
    if c.kind == "gemm_ln":
        r = ref.gemm_ln(c.X, c.W, c.bias, c.res, c.gamma, c.beta, c.eps, relu=c.relu, pe=c.pe, pos=c.pos)
        shown = c.beta if c.pe is None else c.beta + c.pe[c.pos.long()]
        return [("ln", dict(out=r["out"], xhat=r["xhat"], rstd=r["rstd"], pre=r["pre"]), shown)]
    r0 = ref.gemm_ln(c.A, c.wo, c.bo, c.R, c.g0, c.be0, c.eps)
    st = [("ln0", dict(out0=r0["out"], xhat0=r0["xhat"], rstd0=r0["rstd"]), c.be0)]
    if c.kind == "chain":
        r1 = ref.gemm_ln(got["H"], c.w2, c.b2, got["out0"], c.g1, c.be1, c.eps)
        st.append(("hidden", dict(H=ref.hidden(got["out0"], c.w1, c.b1)), None))
        st.append(("ln1", dict(out1=r1["out"], xhat1=r1["xhat"], rstd1=r1["rstd"]), None))
    return st


def rstd_figure(got, want):
    """max |got / ref - 1| (a non-finite value counts as infinite)."""
    f = (got.double() / want.double() - 1).abs()
    return float(torch.nan_to_num(f, nan=float("inf")).max())


def verify(c, gd, report=None, asserted=True):
    """Every output of ``launch`` against the case's references.  report: a list that receives (case id, stage, worst rstd figure,
    worst row of xhat, worst row of out, asserted) BEFORE anything is asserted.  asserted = False: the accuracy bounds are
    reported only (guards, finiteness and the constant rows hold regardless)."""
    for nm, x in gd.items():
        x.assert_intact("%s: %s" % (c.id, nm))
    got = {nm: x.view.detach().cpu() for nm, x in gd.items()}
    stages = references(c, got)
    rows_of = lambda a, b: max(float(torch.nan_to_num(r, nan=float("inf")).max()) for name, r in local_figures(a, b) if name == "row")
    for stage, refs, _ in stages:
        rs = [nm for nm in refs if nm.startswith("rstd")]
        if rs:
            xh, o = [nm for nm in refs if nm.startswith("xhat")][0], [nm for nm in refs if nm.startswith("out")][0]
            row = (c.id, stage, rstd_figure(got[rs[0]], refs[rs[0]]), rows_of(got[xh], refs[xh]), rows_of(got[o], refs[o]), asserted)
            print("ln_stats %s %s: worst rstd error %.3e (bound %.1e), worst row of xhat %.3e, of out %.3e%s"
                  % (row[0], row[1], row[2], L_RSTD, row[3], row[4], "" if asserted else " (reported only)"))
            if report is not None:
                report.append(row)
    for nm, t in got.items():
        assert bool(torch.isfinite(t.float()).all()), "%s %s: non-finite output" % (c.id, nm)
    for stage, refs, shown in stages:
        if c.const is not None and shown is not None:
            xh, o, rs = ([nm for nm in refs if nm.startswith(p)][0] for p in ("xhat", "out", "rstd"))
            assert bool((got[xh][c.const] == 0).all()), "%s %s: xhat of a constant row is not zero (max |xhat| %.3e)" % (
                c.id, stage, float(got[xh][c.const].float().abs().max()))
            want = (shown.to(F32) if shown.dim() == 2 else shown.to(F32).expand(c.M, -1))[c.const].to(BF16)
            assert torch.equal(got[o][c.const], want), "%s %s: out of a constant row is not bf16(beta) bit for bit" % (c.id, stage)
            f = rstd_figure(got[rs][c.const], torch.full((int(c.const.sum()),), float(c.eps) ** -0.5, dtype=F64))
            assert f <= L_RSTD, "%s %s: rstd of a constant row is not eps^-1/2: off by %.3e > %.1e" % (c.id, stage, f, L_RSTD)
        if not asserted:
            continue
        for nm, want in sorted(refs.items(), key=lambda kv: not kv[0].startswith("rstd")):       # (the statistic first)
            what = "%s %s" % (c.id, nm)
            if nm.startswith("rstd"):
                f = (got[nm].double() / want - 1).abs()
                bad = ~(f <= L_RSTD)
                if bool(bad.any()):
                    idx = torch.nonzero(bad).flatten()
                    w = int(torch.nan_to_num(f, nan=float("inf")).argmax())
                    raise AssertionError("%s: rstd bound violated: %d of %d rows, worst row %d: |got / ref - 1| = %.3e > %.1e (got %.7g, ref "
                                         "%.7g; first failing %d, last %d)" % (what, idx.numel(), f.numel(), w, float(f[w]), L_RSTD,
                                                                               float(got[nm][w]), float(want[w]), int(idx[0]), int(idx[-1])))
            else:
                check(got[nm], want, L_BF16, what, tol_local=L_BF16)


def run(kw, be, report=None, asserted=True):
    c = build(**kw)
    verify(c, launch(c, be), report=report, asserted=asserted)
    return c


def table(report):
    """The report of a run as text: one line per case and LayerNorm stage."""
    lines = ["# worst |rstd / fp64 - 1| per case (bound %.0e) and the worst row of xhat / out against the unrounded fp64 reference (bound %.0e)"
             % (L_RSTD, L_BF16), "%-44s %-5s %-11s %-11s %-11s %s" % ("case", "stage", "rstd", "xhat row", "out row", "")]
    for cid, stage, f, xh, o, asserted in report:
        flag = ("" if f <= L_RSTD else "ABOVE THE BOUND") if asserted else "reported only"
        lines.append("%-44s %-5s %-11.3e %-11.3e %-11.3e %s" % (cid, stage, f, xh, o, flag))
    return "\n".join(lines) + "\n"
