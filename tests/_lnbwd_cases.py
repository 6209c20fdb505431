"""Input families and checks of the LayerNorm-backward tests: st_ln_bwd, st_gemm_lnbwd and the HEAD, FFN and TAIL stages of
st_row_chain_bwd against the plain fp64 reference tests/_lnbwd_ref.py, on inputs that are NOT the benign ones of
tests/test_kernels_gpu.py.  Shared by tests/test_lnbwd_fp64_gpu.py (the kernels), tests/test_lnbwd_fp64_cpu.py (the emulation, with
defects injected, so that the checks are known to see them) and tools/local_bounds.py (family "ln_bwd").  A ``Backend`` says whose
ln_bwd / gemm_lnbwd / row_chain_bwd run and where; operands, guards, references and assertions are the same code for all of them.

Families (xhat is a truly normalised row - mean 0, mean square 1 - rounded to bf16, except in ``legacy``):
  legacy       the inputs of tests/test_kernels_gpu.py: rstd = |N(0, 1)| + 0.5, xhat = N(0, 1) not normalised, gamma = 1 +- 0.2, dy = N(0, 1)
  rstd-wide    rstd log-uniform over [1e-3, 1e3], shuffled across rows: the rows of one workgroup span the range
  common-mode  dy gamma = a + b xhat + sigma N(0, 1): the gradient lies almost wholly in the LayerNorm's null space, dx is what the
               cancellation leaves.  st_ln_bwd takes dy as an operand: CM_OPERAND.  The fused kernels round dy = bf16(dY W + aux)
               inside (aux carries a + b xhat, dY W the noise; head0 / chains without HEAD: G / DS carries all of it): CM_FUSED,
               chosen on the CPU (tests/LOCAL_BOUNDS.md)
  gamma-hard   gamma = +-2^u, u uniform over [-4, 4], 30 % negative, exact zeros in a few columns
  dead-rows    a band of rows with dy = 0 (dY = 0 and aux = 0; chains: dP = 0, G = 0, DS = 0): every output row of the band is
               +-0 in every element, its delta is 0, it adds nothing to any column sum
  mask-edge    st_ln_bwd's mask holds +0.0, -0.0, the smallest positive and the smallest negative bf16 subnormal next to ordinary
               values: dx is exactly zero where mask <= 0 and scaled elsewhere - the positive subnormal counts as positive

A chain is referenced stage by stage FROM THE TENSORS THE KERNEL ITSELF WROTE for the stage before: dH from its ds_a, ds_b from
its dH and ds_a, dctx from its ds_b, delta from its dctx as stored times O + Ores as handed, dbias of st_gemm_lnbwd and of the chains
from its own stored dx (st_ln_bwd sums before rounding and is referenced from the inputs).  An upstream rounding is never charged to a
stage.

Bounds - none is tuned against a kernel (tests/LOCAL_BOUNDS.md, "The LayerNorm backward family"):
  dx, ds_a, dH, ds_b, dctx   L_BF16 = 1e-2: whole tensor, column by column (against max(own norm, 0.25 x typical)) and row by row
                             against the row's OWN reference norm, no floor (check_local(own_rows=True))
  delta                      L_DELTA, element by element against the own-output sum
  dgamma / dbeta / dbias     L_COL[kind], element by element
  (the last two: 3 x the larger figure of two fp32 evaluations against fp64 over all cases - the emulation as it is, CPU, and SERIAL:
  every column sum and delta's 64 products accumulated serially, the contraction in chunks of 32; never above the bounds already
  in force)
  exact                      dead rows, mask edge, guards intact, everything finite."""
import contextlib
import math
import types

import torch

from tests import _emul as em
from tests import _lnbwd_ref as ref
from tests._local import Guarded, check, check_local, guarded_input, local_figures, rel

BF16, F32, F64, I32 = torch.bfloat16, torch.float32, torch.float64, torch.int32

L_BF16 = 1e-2
CM_OPERAND = (64.0, 16.0, 0.125)
CM_CANDIDATES = ((8.0, 4.0, 1.0), (4.0, 2.0, 1.0), (2.0, 1.0, 1.0), (1.0, 0.5, 1.0))      # strongest first
CM_FUSED = (4.0, 2.0, 1.0)           # the strongest candidate that keeps the emulation below L_BF16 / 3 on every row (tools/local_bounds.py)
# 3 x the larger of the CPU and SERIAL backends' worst figures over all cases, rounded up to two digits, capped by IN_FORCE
# (tools/local_bounds.py prints the figures, tests/LOCAL_BOUNDS.md has the table, tests/test_lnbwd_fp64_cpu.py asserts the relation)
L_DELTA = 2.1e-5                                                        # 3 x 6.8e-6
L_COL = {"ln_bwd": dict(dgamma=1.3e-5, dbeta=2.9e-6, dbias=5e-3),       # 3 x 4.1e-6, 9.5e-7, 1.79e-3 (5.4e-3: capped)
         "gemm_lnbwd": dict(dgamma=1.8e-3, dbeta=4.2e-3, dbias=4.4e-5),  # 3 x 5.7e-4, 1.39e-3, 1.46e-5
         "chain": dict(dgamma=1.9e-3, dbeta=1.8e-3, dbias=5.4e-5)}       # 3 x 6.3e-4, 5.9e-4, 1.79e-5
IN_FORCE = {"ln_bwd": dict(dgamma=3e-3, dbeta=3e-3, dbias=5e-3), "gemm_lnbwd": dict(dgamma=5e-3, dbeta=5e-3, dbias=8e-3),
            "chain": dict(dgamma=5e-3, dbeta=5e-3, dbias=5e-3)}      # tests/test_kernels_gpu.py: L_LNBWD, L_GEMM_LNBWD, L_CHAIN_BWD

FAMILIES = ("legacy", "rstd-wide", "common-mode", "gamma-hard", "dead-rows")
D, D_FF = 256, 512                    # the chains: d_model 256, the smallest d_ff with more than one hidden chunk

# ---- the kernels, each at the smallest shape that selects it ----------------------------------------------------------------------------
IMPLS = {
    # st_ln_bwd (csrc/st_misc.hip): a workgroup takes 4 waves x 2 x 64 / (N / 8) = 32 / 16 / 8 rows per trip at N = 128 / 256 / 512 (M = 70:
    # the last row group of a wave is ragged), at most 256 workgroups - past 256 x 16 = 4,096 rows at N = 256 the grid-stride loop runs twice
    "ln_bwd-n128": dict(kind="ln_bwd", M=70, N=128),
    "ln_bwd-n256": dict(kind="ln_bwd", M=70, N=256),
    "ln_bwd-n512": dict(kind="ln_bwd", M=70, N=512),
    "ln_bwd-n128-mask": dict(kind="ln_bwd", M=70, N=128, mask=True),
    "ln_bwd-n256-mask": dict(kind="ln_bwd", M=70, N=256, mask=True),
    "ln_bwd-n512-mask": dict(kind="ln_bwd", M=70, N=512, mask=True),
    "ln_bwd-n256-drop": dict(kind="ln_bwd", M=70, N=256, p=0.2),
    "ln_bwd-stride-n256": dict(kind="ln_bwd", M=4100, N=256),
    "ln_bwd-stride-n256-mask": dict(kind="ln_bwd", M=4100, N=256, mask=True),
    # st_gemm_lnbwd (csrc/st_gemm_lnbwd.hip): 4 waves unless N = 256, Kc >= 512 and 16,384 < M <= 32,768 (128-row tiles on 8 waves) or
    # N = 512 and M > 8,192 (8 waves: 64-row tiles at Kc < 1,024, 128-row tiles from there)
    "gemm_lnbwd-n128": dict(kind="gemm_lnbwd", M=70, N=128, K=128),
    "gemm_lnbwd-n256": dict(kind="gemm_lnbwd", M=70, N=256, K=256),
    "gemm_lnbwd-n512": dict(kind="gemm_lnbwd", M=70, N=512, K=512),
    "gemm_lnbwd-n256-noaux": dict(kind="gemm_lnbwd", M=70, N=256, K=256, aux=False),
    "gemm_lnbwd-n256-drop": dict(kind="gemm_lnbwd", M=70, N=256, K=256, p=0.1),
    "gemm_lnbwd-tall-n256": dict(kind="gemm_lnbwd", M=16400, N=256, K=512),
    "gemm_lnbwd-tiles-n512": dict(kind="gemm_lnbwd", M=8200, N=512, K=512),
    "gemm_lnbwd-tall-n512": dict(kind="gemm_lnbwd", M=8200, N=512, K=1024),
    # st_row_chain_bwd (csrc/st_rowchain.hip: row_tiles, split_parts_for): 32-row workgroups up to 8,192 rows, with the scratch and two or
    # more hidden chunks one workgroup per chunk and row block; HEAD + FFN + TAIL past 8,192 rows: the pipelined kernel on 64-row
    # workgroups, past 16,384 on 96-row ones, column sums through the workspace and st_colsum_fold (folded at once, or deferred)
    "chain-32row": dict(kind="chain", M=70, parts="head3+ffn+tail"),
    "chain-32row-drop": dict(kind="chain", M=70, parts="head3+ffn+tail", p=0.1),
    "chain-split": dict(kind="chain", M=70, parts="head3+ffn+tail", split=True),
    "chain-pipe64": dict(kind="chain", M=8200, parts="head3+ffn+tail"),
    "chain-pipe96": dict(kind="chain", M=16400, parts="head3+ffn+tail"),
    "chain-pipe64-deferred": dict(kind="chain", M=8200, parts="head3+ffn+tail", deferred=True),
    "chain-pipe96-deferred": dict(kind="chain", M=16400, parts="head3+ffn+tail", deferred=True),
    "chain-head0": dict(kind="chain", M=70, parts="head0+ffn+tail"),
    "chain-ffn+tail": dict(kind="chain", M=70, parts="ffn+tail"),
    "chain-tail": dict(kind="chain", M=70, parts="tail"),
}


def cases():
    """[(id, dict(impl=, family=))]: every family through every kernel; mask-edge through the masked st_ln_bwd cases."""
    out = []
    for iid, impl in IMPLS.items():
        for fam in FAMILIES + (("mask-edge",) if impl.get("mask") else ()):
            out.append(("%s-%s" % (iid, fam), dict(impl=iid, family=fam)))
    return out


def g(*shape, seed=0, scale=1.0, dtype=BF16):
    """The seeded operands of tests/test_kernels_gpu.py."""
    gen = torch.Generator().manual_seed(seed)
    return (torch.randn(*shape, generator=gen) * scale).to(dtype)


def band(M):
    """The dead rows: a band across the first 32-row tile boundary and the last two rows (a ragged last tile)."""
    rows = torch.zeros(M, dtype=torch.bool)
    rows[30:38] = True
    rows[M - 2:] = True
    return rows


def _ln_side(M, N, family, seed):
    """One LayerNorm's saved tensors and scale under a family: xhat bf16 [M, N], rstd fp32 [M], gamma fp32 [N]."""
    xhat, rstd, gamma = g(M, N, seed=seed), g(M, seed=seed + 1, dtype=F32).abs() + 0.5, 1 + 0.2 * g(N, seed=seed + 2, dtype=F32)
    if family == "legacy":
        return xhat, rstd, gamma
    x = g(M, N, seed=seed, dtype=F64)
    x = x - x.mean(1, keepdim=True)
    xhat = (x / x.pow(2).mean(1, keepdim=True).sqrt()).to(BF16)
    gen = torch.Generator().manual_seed(seed + 3)
    if family == "rstd-wide":
        rstd = (10.0 ** torch.linspace(-3, 3, M, dtype=F64))[torch.randperm(M, generator=gen)].to(F32)
    if family == "gamma-hard":
        gamma = 2.0 ** (8 * torch.rand(N, generator=gen, dtype=F64) - 4)
        gamma = torch.where(torch.rand(N, generator=gen) < 0.3, -gamma, gamma).to(F32)
        gamma[[5, N // 2, N - 1]] = 0.0
    return xhat, rstd, gamma


def _common(xhat, gamma, cm, seed, noise=True):
    """(a + b xhat [+ sigma N(0, 1)]) / gamma, rounded to bf16 once."""
    a, b, sigma = cm
    t = a + b * xhat.to(F64)
    if noise:
        t = t + sigma * g(*xhat.shape, seed=seed, dtype=F64)
    return (t / gamma.to(F64)).to(BF16)


def _edge_mask(M, N, seed):
    m = g(M, N, seed=seed)
    bits = m.view(torch.int16).clone()
    k = (torch.arange(M).view(-1, 1) + torch.arange(N).view(1, -1)) % 8
    for i, v in enumerate((0x0000, -0x8000, 0x0001, -0x8000 + 1)):          # +0.0, -0.0, +2^-133, -2^-133
        bits[k == i] = v
    return bits.view(BF16)


def build(impl, family, cm=None):
    """One case: the operands as the kernel gets them.  cm: another (a, b, sigma) for the common-mode family (the CPU derivation)."""
    o = types.SimpleNamespace(impl=IMPLS[impl], iid=impl, family=family, id="%s-%s" % (impl, family), kind=IMPLS[impl]["kind"])
    i, M = o.impl, IMPLS[impl]["M"]
    o.M, o.p = M, i.get("p", 0.0)
    o.dead = band(M) if family == "dead-rows" else None
    o.drop_salt = 11
    norm_fam = family if family in ("rstd-wide", "gamma-hard") else ("legacy" if family == "legacy" else "normalised")
    if o.kind == "ln_bwd":
        N = o.N = i["N"]
        o.xhat, o.rstd, o.gamma = _ln_side(M, N, norm_fam, 2)
        o.dy = _common(o.xhat, o.gamma, cm or CM_OPERAND, 1) if family == "common-mode" else g(M, N, seed=1)
        if o.dead is not None:
            o.dy[o.dead] = 0
        o.mask = None
        if i.get("mask"):
            o.mask = _edge_mask(M, N, 5) if family == "mask-edge" else g(M, N, seed=5)
        o.mask_scale = 2.0 if i.get("mask") else 1.0
        return o
    if o.kind == "gemm_lnbwd":
        N, K = i["N"], i["K"]
        o.N, o.K = N, K
        o.xhat, o.rstd, o.gamma = _ln_side(M, N, norm_fam, 4)
        a, b, sigma = cm or CM_FUSED
        o.dY, o.W = g(M, K, seed=1, scale=sigma if family == "common-mode" else 1.0), g(K, N, seed=2, scale=K ** -0.5)
        o.aux = g(M, N, seed=3) if i.get("aux", True) else None
        if family == "common-mode" and o.aux is not None:
            o.aux = _common(o.xhat, o.gamma, (a, b, sigma), 0, noise=False)
        if o.dead is not None:
            o.dY[o.dead] = 0
            if o.aux is not None:
                o.aux[o.dead] = 0
        return o
    parts = i["parts"].split("+")
    o.nb = 3 if "head3" in parts else 0
    o.has_head, o.has_ffn, o.has_tail = parts[0].startswith("head"), "ffn" in parts, "tail" in parts
    o.N, d, dff = D, D, D_FF
    a, b, sigma = cm or CM_FUSED
    common = family == "common-mode"
    o.wp, o.w1, o.w2, o.wo = g(768, d, seed=1, scale=d ** -0.5), g(dff, d, seed=2, scale=d ** -0.5), g(d, dff, seed=3, scale=dff ** -0.5), \
        g(d, d, seed=4, scale=d ** -0.5)
    o.xa, o.ra, o.ga = _ln_side(M, d, norm_fam, 20)
    o.xb, o.rb, o.gb = _ln_side(M, d, norm_fam, 30)
    o.dP = g(M, 768, seed=5, scale=sigma / math.sqrt(3.0) if common else 0.3)
    o.G, o.DS = g(M, d, seed=6, scale=0.3), g(M, d, seed=7, scale=0.3)
    if common:
        o.G = _common(o.xa, o.ga, (a, b, sigma), 6, noise=o.nb == 0)
        if o.has_ffn:
            o.DS = _common(o.xb, o.gb, (a, b, sigma), 7)
    o.Hbits = g(M, dff, seed=14).float() > 0
    o.O, o.Ores = g(M, d, seed=15), g(M, d, seed=16, scale=2.0 ** -9)
    if o.dead is not None:
        for t in (o.dP, o.G, o.DS):
            t[o.dead] = 0
    o.mask_scale = 1.0 / 0.9
    o.drop_salt = 31
    return o


# ---- backends ---------------------------------------------------------------------------------------------------------------------------
def drop_pair(c, device):
    """(the seed on ``device``, the emulation's Drop) of a case whose kernel regenerates a dropout mask, or (None, None)."""
    if not c.p:
        return None, None
    seed = torch.tensor([1234567], dtype=I32)
    return seed.to(device), em.Drop(seed, c.drop_salt, c.p)


class Backend:
    """Whose kernels run, on which device.  ln_bwd: a function with tests._emul.ln_bwd's signature (the emulation, or one with a defect);
    the emulated gemm_lnbwd and chains are composed of it.  tamper(c, out): changes the outputs after the launch (a defect in what a
    kernel writes).  gpu: st_amd.native."""

    def __init__(self, device, ln_bwd=None, tamper=None, gpu=False, gemm=None):
        self.device, self.gpu, self._ln_bwd, self.tamper, self._gemm = device, gpu, ln_bwd, tamper, gemm

    @contextlib.contextmanager
    def _swapped(self):
        saved = em.ln_bwd, em.gemm
        try:
            em.ln_bwd, em.gemm = self._ln_bwd, self._gemm or em.gemm
            yield
        finally:
            em.ln_bwd, em.gemm = saved

    def drop(self, c):
        seed, e = drop_pair(c, self.device)
        if e is None:
            return None
        if self.gpu:
            from st_amd import native as nv
            return nv.Drop(seed, c.drop_salt, c.p)
        return e

    def ln_bwd(self, *a, **kw):
        if self.gpu:
            from st_amd import native as nv
            return nv.ln_bwd(*a, **kw)
        return self._ln_bwd(*a, dtype=F32, **kw)

    def gemm_lnbwd(self, *a, **kw):
        if self.gpu:
            from st_amd import native as nv
            return nv.gemm_lnbwd(*a, **kw)
        with self._swapped():
            return em.gemm_lnbwd(*a, dtype=F32, dbias_rounded=True, **kw)

    def row_chain_bwd(self, *a, **kw):
        if self.gpu:
            from st_amd import native as nv
            return nv.row_chain_bwd(*a, **kw)
        with self._swapped():
            return em.row_chain_bwd(*a, dtype=F32, dbias_rounded=True, **kw)

    def relu_bits(self, H):
        if self.gpu:
            from st_amd import native as nv
            return nv.relu_bits_from(H)
        return em.relu_bits_from(H)

    def chain(self, blocks, split=False):
        from st_amd import chains
        if not self.gpu:
            return chains.Chain(None, len(blocks), blocks)
        from st_amd import native as nv
        cs = chains.ChainSet(self.device)
        cid = cs.add(blocks)
        cs.finalize().rebuild()
        ch = cs.chain(cid)
        if split:
            ch.split_work = torch.zeros(nv.split_work_words(), dtype=I32, device=self.device)
        return ch


def _serial(x):
    """The column sum of x [M, N] accumulated serially down the rows in x's own precision (a loop: torch's cumsum accumulates in double)."""
    acc = torch.zeros(x.shape[1], dtype=x.dtype)
    for r in range(x.shape[0]):
        acc += x[r]
    return acc


def serial_ln_bwd(dy, xhat, rstd, gamma, dx, dgamma=None, dbeta=None, dbias=None, mask=None, drop=None, mask_scale=1.0, dtype=F32,
                  dbias_rounded=False):
    """tests._emul.ln_bwd with every column sum accumulated serially down the rows (fp32: the least favourable order)."""
    d, xh = dy.to(dtype), xhat.to(dtype)
    if em._on(drop):
        d = d * em.keep_rc(drop, torch.arange(d.shape[0]), torch.arange(d.shape[1]), d.shape[1]) * drop.scale
    gg = d * gamma.to(dtype)
    v = rstd.to(dtype).unsqueeze(-1) * (gg - gg.mean(-1, keepdim=True) - xh * (gg * xh).mean(-1, keepdim=True))
    if mask is not None:
        v = v * (mask.to(dtype) > 0) * mask_scale
    dx.copy_(v.to(BF16))
    for acc, t in ((dgamma, d * xh), (dbeta, d), (dbias, dx.to(dtype) if dbias_rounded else v)):
        if acc is not None:
            acc += _serial(t.contiguous())
    return dx


def chunked_gemm(X, Y, out, aux=None, epi=None, y_cmajor=False, delta=None, head_dim=0, aux2=None, dtype=F32, add_once=True):
    """tests._emul.gemm for the data-gradient products of this family (Y [Kc, N] as stored), the contraction accumulated serially
    over chunks of 32 - one MFMA step - and delta's products one by one: another summation order, hence other bf16 values of dy
    that land on the far side of a rounding boundary.  EPI_BF16_ADD only in the fused kernels' form (acc + aux rounded once)."""
    assert add_once
    from st_amd import native as nv
    epi = nv.EPI_BF16 if epi is None else epi
    assert y_cmajor and epi in (nv.EPI_BF16, nv.EPI_BF16_ADD, nv.EPI_BF16_DELTA)
    Xl, Yl = X.to(dtype), Y.to(dtype)
    M, N = Xl.shape[0], Yl.shape[1]
    acc = torch.zeros(M, N, dtype=dtype)
    for k0 in range(0, Xl.shape[1], 32):
        acc = acc + Xl[:, k0:k0 + 32] @ Yl[k0:k0 + 32]
    if epi == nv.EPI_BF16_ADD:
        acc = acc + aux[:M, :N].to(dtype)
    out[:M, :N] = acc.to(out.dtype)
    if epi == nv.EPI_BF16_DELTA:
        prod = out[:M, :N].to(dtype) * (aux[:M, :N].to(dtype) + (aux2[:M, :N].to(dtype) if aux2 is not None else 0.0))
        prod = prod.view(M, N // head_dim, head_dim)
        s = torch.zeros(M, N // head_dim, dtype=dtype)
        for j in range(head_dim):
            s = s + prod[:, :, j]
        delta.view(N // head_dim, -1)[:, :M] = s.t()
    return out


CPU = Backend("cpu", ln_bwd=em.ln_bwd)                            # the emulation as the other kernel tests use it
SERIAL = Backend("cpu", ln_bwd=serial_ln_bwd, gemm=chunked_gemm)      # another order of every sum: the second sample the bounds are taken over


def cpu_backend(ln_bwd=None, tamper=None):
    return Backend("cpu", ln_bwd=ln_bwd or em.ln_bwd, tamper=tamper)


def gpu_backend():
    return Backend("cuda", gpu=True)


# ---- running a case -------------------------------------------------------------------------------------------------------------------
CHAIN_INIT = dict(dga=1.0, dba=2.0, dbia=3.0, dgb=-1.0, dbb=-2.0, dbib=-3.0)          # accumulate semantics: the sums start from these


def chain_blocks(c, f):
    from st_amd import chains
    b = []
    if c.nb:
        b += chains.t_blocks(chains.blocks_of(f(c.wp)))
    if c.has_ffn:
        b += chains.ffn_blocks_bwd(f(c.w1), f(c.w2))
    if c.has_tail:
        b += chains.t_blocks(chains.blocks_of(f(c.wo)))
    return b


def launch(c, be):
    """The case by the backend's kernels: outputs in guards, strided bf16 operands in NaN surroundings.  -> {output name: Guarded}"""
    dev = be.device
    mv = lambda t: None if t is None else t.to(dev)
    GI = lambda t, **kw: None if t is None else guarded_input(t, dev, **kw)
    GO = lambda rows, cols, contiguous=False: Guarded(rows, cols, BF16, dev, pad_cols=(0, 0) if contiguous else (64, 64))
    GV = lambda n: Guarded.vec(n, F32, dev)
    M, N = c.M, c.N
    if c.kind in ("ln_bwd", "gemm_lnbwd"):
        gd = dict(dx=GO(M, N), dgamma=GV(N), dbeta=GV(N), dbias=GV(N))
        for nm in ("dgamma", "dbeta", "dbias"):
            gd[nm].view.fill_(1.0)
        acc = [gd[nm].view for nm in ("dgamma", "dbeta", "dbias")]
        if c.kind == "ln_bwd":
            be.ln_bwd(GI(c.dy), mv(c.xhat), mv(c.rstd), mv(c.gamma), gd["dx"].view, *acc, mask=mv(c.mask), drop=be.drop(c),
                      mask_scale=c.mask_scale)
        else:
            be.gemm_lnbwd(GI(c.dY), mv(c.W), GI(c.aux), mv(c.xhat), mv(c.rstd), mv(c.gamma), gd["dx"].view, *acc, drop=be.drop(c))
    else:
        gd = {}
        if c.has_head:
            gd.update(ds_a=GO(M, D, True), dga=GV(D), dba=GV(D), dbia=GV(D))
        if c.has_ffn:
            gd.update(dH=GO(M, D_FF, True), ds_b=GO(M, D, True), dgb=GV(D), dbb=GV(D), dbib=GV(D))
        if c.has_tail:
            gd.update(dctx=GO(M, D), delta=GV(4 * M))
        for nm, v in CHAIN_INIT.items():
            if nm in gd:
                gd[nm].view.fill_(v)
        o = {k: v.view for k, v in gd.items()}
        ch = be.chain(chain_blocks(c, mv), split=bool(c.impl.get("split")))
        H = (c.Hbits.to(BF16)).to(dev)
        kw = dict(head=(c.nb, GI(c.dP) if c.nb else None, GI(c.G), mv(c.xa), mv(c.ra), mv(c.ga), be.drop(c), o["ds_a"], o["dga"], o["dba"],
                        o["dbia"]) if c.has_head else None,
                  ds_in=None if c.has_head else mv(c.DS),
                  ffn=(D_FF, be.relu_bits(H), c.mask_scale, o["dH"], mv(c.xb), mv(c.rb), mv(c.gb), o["ds_b"], o["dgb"], o["dbb"],
                       o["dbib"]) if c.has_ffn else None,
                  tail=(GI(c.O), GI(c.Ores), o["dctx"], o["delta"]) if c.has_tail else None)
        if be.gpu and c.impl.get("deferred"):
            from st_amd import native as nv
            nv.fold_deferred = True
            try:
                be.row_chain_bwd(ch, M, **kw)
                assert len(nv._fold_pending) == 1, "%s: the launch left no column-sum workspace to fold" % c.id
                nv.flush_colsum_folds()
            finally:
                nv.fold_deferred = False
        else:
            be.row_chain_bwd(ch, M, **kw)
    if dev != "cpu":
        torch.cuda.synchronize()
    if be.tamper is not None:
        be.tamper(c, gd)
    return gd


def references(c, got):
    """[(output name, fp64 reference, bound)]: each stage from the operands the kernel read - the case's own for the first, the
    kernel's outputs for the later ones.  Column sums include the value the accumulator started from."""
    if c.kind == "ln_bwd":
        keep, sc = ref.keep_of(drop_pair(c, "cpu")[1], c.M, c.N)
        r = ref.ln_bwd(c.dy, c.xhat, c.rstd, c.gamma, keep, sc, c.mask, c.mask_scale)
        return [("dx", r["dx"], L_BF16)] + [(nm, r[nm] + 1.0, L_COL["ln_bwd"][nm]) for nm in ("dgamma", "dbeta", "dbias")]
    if c.kind == "gemm_lnbwd":
        keep, sc = ref.keep_of(drop_pair(c, "cpu")[1], c.M, c.N)
        r = ref.gemm_lnbwd(c.dY, c.W, c.aux, c.xhat, c.rstd, c.gamma, keep, sc)
        lc = L_COL["gemm_lnbwd"]
        return [("dx", r["dx"], L_BF16), ("dgamma", r["dgamma"] + 1.0, lc["dgamma"]), ("dbeta", r["dbeta"] + 1.0, lc["dbeta"]),
                ("dbias", ref.colsum(got["dx"]) + 1.0, lc["dbias"])]
    out, lc, M = [], L_COL["chain"], c.M
    ds = c.DS
    if c.has_head:
        keep, sc = ref.keep_of(drop_pair(c, "cpu")[1], M, D)
        r = ref.gemm_lnbwd(c.dP, c.wp, c.G, c.xa, c.ra, c.ga, keep, sc) if c.nb else ref.ln_bwd(c.G, c.xa, c.ra, c.ga, keep, sc)
        out += [("ds_a", r["dx"], L_BF16), ("dga", r["dgamma"] + CHAIN_INIT["dga"], lc["dgamma"]),
                ("dba", r["dbeta"] + CHAIN_INIT["dba"], lc["dbeta"]), ("dbia", ref.colsum(got["ds_a"]) + CHAIN_INIT["dbia"], lc["dbias"])]
        ds = got["ds_a"]
    if c.has_ffn:
        out.append(("dH", ref.masked_dgrad(ds, c.w2, c.Hbits, c.mask_scale), L_BF16))
        r = ref.gemm_lnbwd(got["dH"], c.w1, ds, c.xb, c.rb, c.gb)
        out += [("ds_b", r["dx"], L_BF16), ("dgb", r["dgamma"] + CHAIN_INIT["dgb"], lc["dgamma"]),
                ("dbb", r["dbeta"] + CHAIN_INIT["dbb"], lc["dbeta"]), ("dbib", ref.colsum(got["ds_b"]) + CHAIN_INIT["dbib"], lc["dbias"])]
        ds = got["ds_b"]
    if c.has_tail:
        out += [("dctx", ref.dgrad(ds, c.wo), L_BF16), ("delta", ref.delta_of(got["dctx"], c.O, c.Ores), L_DELTA)]
    return out


def _worst(t):
    return float(torch.nan_to_num(t, nan=float("inf")).max()) if t.numel() else 0.0


def figures(got, want, own_rows=True):
    """{"rel", "row", "column"} of a matrix, {"element"} of a vector: the figures the bounds apply to."""
    f = {name: _worst(r) for name, r in local_figures(got, want, own_rows=own_rows)}
    if got.dim() > 1:
        f["rel"] = rel(got, want)
    return f


def verify(c, gd, report=None, asserted=True, own_rows=True):
    """Every output of ``launch`` against the case's references.  report: a list that receives (case id, output, figures, bound)
    BEFORE anything is asserted.  asserted = False: the accuracy bounds are reported only (guards, finiteness and the exact checks
    hold regardless).  own_rows = False: rows against max(own norm, 0.25 x typical) - the floor every other kernel test uses."""
    for nm, x in gd.items():
        x.assert_intact("%s: %s" % (c.id, nm))
    got = {nm: x.view.detach().cpu() for nm, x in gd.items()}
    refs = references(c, got)
    for nm, want, bound in refs:
        f = figures(got[nm], want, own_rows)
        print("ln_bwd %s %s: %s (bound %.1e)" % (c.id, nm, ", ".join("%s %.3e" % kv for kv in sorted(f.items())), bound))
        if report is not None:
            report.append((c.id, nm, f, bound))
    for nm, t in got.items():
        assert bool(torch.isfinite(t.float()).all()), "%s %s: non-finite output" % (c.id, nm)
    if c.dead is not None:
        for nm, t in got.items():
            if t.dim() == 2:
                assert bool((t[c.dead] == 0).all()), "%s %s: a dead row is not zero (max |value| %.3e)" % (c.id, nm, float(t[c.dead].float().abs().max()))
            elif nm == "delta":
                d = t.view(4, c.M)[:, c.dead]
                assert bool((d == 0).all()), "%s delta: a dead row's delta is not zero (max |value| %.3e)" % (c.id, float(d.abs().max()))
    if c.kind == "ln_bwd" and c.mask is not None:
        off = ~(c.mask.double() > 0)
        assert bool((got["dx"][off] == 0).all()), "%s dx: not zero where mask <= 0 (%d elements)" % (c.id, int((got["dx"][off] != 0).sum()))
    if not asserted:
        return refs
    for nm, want, bound in refs:
        what = "%s %s" % (c.id, nm)
        if got[nm].dim() > 1:
            check(got[nm], want, bound, what)
        check_local(got[nm], want, bound, what, own_rows=own_rows)
    return refs


def run(kw, be, report=None, asserted=True, own_rows=True):
    c = build(**kw)
    verify(c, launch(c, be), report=report, asserted=asserted, own_rows=own_rows)
    return c


def table(report):
    """The report of a run as text: one line per case and output."""
    lines = ["# worst figure per case and output against the fp64 reference: matrices - whole-tensor relative L2, worst row against its OWN norm, worst "
             "column; vectors - worst element", "%-40s %-7s %-11s %-11s %-11s %-9s %s" % ("case", "output", "rel / elem", "row", "column", "bound", "")]
    for cid, nm, f, bound in report:
        first = f.get("rel", f.get("element", 0.0))
        flag = "" if max(f.values()) <= bound else "ABOVE THE BOUND"
        lines.append("%-40s %-7s %-11.3e %-11s %-11s %-9.1e %s" % (cid, nm, first, "%.3e" % f["row"] if "row" in f else "-",
                                                                  "%.3e" % f["column"] if "column" in f else "-", bound, flag))
    return "\n".join(lines) + "\n"
