"""Cases and checks of the slow-path attention tests (st_attn_dense_fwd / _bwd, st_attn_probs), shared by
tests/test_slow_attention_gpu.py (the kernels), tests/test_slow_attention_cpu.py (the emulation, with defects injected, so the
checks are known to see them) and tools/local_bounds.py (where the fp32 bounds come from).  A ``Backend`` says whose entry points
run and where; everything else - inputs, guards, fp64 reference, assertions - is the same code for all three."""
import math
import types

import torch

from tests import _attn_ref as ref
from tests import _emul as em
from tests._local import Guarded, check, guarded_input

BF16, F32, F64, I32 = torch.bfloat16, torch.float32, torch.float64, torch.int32

# Bounds (tests/LOCAL_BOUNDS.md, "slow-path attention"): whole tensor and every row / column / element alike.  The dense kernels keep
# P and dS in fp32 and round their bf16 outputs once -> L_BF16 (the rounding alone takes 3.5e-3 of it); lse / delta / P: 3 x the
# emulation's fp32-vs-fp64 figure over these cases (tools/local_bounds.py, family "dense": lse 3.5e-7, P 5.1e-6, delta 1.3e-5 -> at
# most 3.9e-5) is far below L_F32, which therefore is the bound in force.
L_BF16, L_F32 = 1e-2, 2e-3
L_DENSE = dict(O=L_BF16, dQ=L_BF16, dK=L_BF16, dV=L_BF16, lse=L_F32, delta=L_F32, P=L_F32)
L_PROBS64 = 1e-4          # st_attn_probs against fp64: 3 x measured (family "probs": 1.5e-6 -> 4.5e-6) is below the family's 1e-4 (L_PROBS)
# A live row of P sums to 1: the kernel divides the stored fp32 exponentials by their fp32 sum - at most 64 serial additions per
# thread (Lk <= 16384), 6 shuffles, 3 adds, one reciprocal, one product: < 80 roundings of 2^-24 = 4.8e-6.
ROWSUM = 1e-5

# B, H, d_k, Lq, Lk: B and H no powers of two where it matters (the block index is taken apart by % and /)
GRID = [(1, 1, 8, 1, 1),
        (3, 3, 32, 5, 63), (3, 3, 32, 5, 64), (3, 3, 32, 5, 65),                         # one wave / wave boundary
        (2, 2, 64, 7, 255), (2, 2, 64, 7, 256), (2, 2, 64, 7, 257), (2, 2, 64, 7, 600),   # block stride on keys
        (2, 2, 64, 257, 9), (2, 2, 64, 300, 9),                                           # block stride on queries (key-side kernel)
        (2, 2, 64, 257, 300),                                                             # both
        (2, 1, 128, 7, 300),                                                              # head-column loop
        (2, 3, 96, 300, 9),                                                               # head-column loop, partial second pass
        (2, 3, 8, 20, 70), (2, 3, 16, 20, 70)]                                            # narrow heads
MASKS = ("none", "rand30", "dead", "utt", "bytes")
LDS_FLOATS = 16384


class Backend:
    """Whose attn_dense_fwd / attn_dense_bwd / attn_probs run (st_amd.native or tests._emul), on which device."""

    def __init__(self, kernels, device, drop_cls):
        self.k, self.device, self.drop_cls = kernels, device, drop_cls

    def drop(self, c):
        return self.drop_cls(torch.tensor([c.seed], dtype=I32, device=self.device), c.salt, c.p) if c.p > 0 else None


CPU = Backend(em, "cpu", em.Drop)


def gpu_backend():
    from st_amd import native as nv
    return Backend(nv, "cuda", nv.Drop)


def make_mask(kind, B, Lq, Lk, gen):
    """uint8 [B, Lq, Lk], nonzero = masked (None: no mask)."""
    if kind == "none":
        return None
    m = (torch.rand(B, Lq, Lk, generator=gen) < 0.3).to(torch.uint8)
    if kind == "dead":                      # one dead query row per utterance, one key masked for every query
        for b in range(B):
            m[b, (3 * b + 1) % Lq] = 1
            m[b, :, (Lk - 1 - 2 * b) % Lk] = 1
    elif kind == "utt":                     # one whole utterance masked
        m[B - 1] = 1
    elif kind == "bytes":                   # the contract is "nonzero = masked"
        m = m * torch.where(torch.rand(B, Lq, Lk, generator=gen) < 0.5, 2, 255).to(torch.uint8)
    else:
        assert kind == "rand30", kind
    return m


def build(B, H, dk, Lq, Lk, mask="none", operands="separate", sharp=1.0, needle=False, p=0.0, salt=7, seed=1234567, backward=True,
          gseed=0):
    """One case: bf16 inputs, mask, the emulation's keep set for (seed, salt, p) and the fp64 reference of every output.
    operands: "separate", "kv" (K | V one [Mk, 2d] matrix), "qkv" (one fused [M, 3d] matrix; Lq == Lk), "k_is_v".
    sharp: the scale of Q, K, V.  needle: query 0 of every (b, h) puts nearly all its mass on key Lk - 1 and query 1 on key 256."""
    gen = torch.Generator().manual_seed(7919 * gseed + 31 * Lq + Lk + dk)
    d, scale = H * dk, 1.0 / math.sqrt(dk)
    rn = lambda r, s: (torch.randn(r, d, generator=gen) * s).to(BF16)
    Q, K = rn(B * Lq, sharp), rn(B * Lk, sharp)
    V = K if operands == "k_is_v" else rn(B * Lk, sharp)
    dO = rn(B * Lq, 1.0) if backward else None
    if needle:
        pairs = [(0, Lk - 1)] + ([(1, 256)] if Lk > 257 and Lq > 1 else [])
        for b in range(B):
            for h in range(H):
                cs = slice(h * dk, (h + 1) * dk)
                for q, k in pairs:
                    qv = Q[b * Lq + q, cs].float()
                    K[b * Lk + k, cs] = (qv * (40.0 / (scale * float(qv.pow(2).sum())))).to(BF16)      # score 40: e^-40 for the rest
    m = make_mask(mask, B, Lq, Lk, gen)
    c = types.SimpleNamespace(B=B, H=H, dk=dk, Lq=Lq, Lk=Lk, d=d, scale=scale, Q=Q, K=K, V=V, dO=dO, mask=m, operands=operands, p=p,
                              salt=salt, seed=seed, keep=None, keep_scale=1.0)
    c.dead_q = m.ne(0).all(-1) if m is not None else torch.zeros(B, Lq, dtype=torch.bool)
    c.dead_k = m.ne(0).all(1) if m is not None else torch.zeros(B, Lk, dtype=torch.bool)
    if p > 0:
        de = em.Drop(torch.tensor([seed], dtype=I32), salt, p)
        c.keep = torch.stack([em.keep_qk(de, bh, Lq, Lk) for bh in range(B * H)])
        c.keep_scale = de.scale
    names = ("O", "lse", "P", "delta", "dQ", "dK", "dV")
    c.ref = dict(zip(names, ref.dense_attention(Q, K, V, m, dO, B, H, Lq, Lk, scale, keep=c.keep, keep_scale=c.keep_scale)))
    return c


def variant(c, **kw):
    """The case with some fields replaced (its reference is NOT recomputed)."""
    c = types.SimpleNamespace(**vars(c))
    for k, v in kw.items():
        setattr(c, k, v)
    return c


def place(c, dev):
    """The operands as the kernels take them: strided views whose surroundings are NaN."""
    d = c.d
    if c.operands == "qkv":
        f = guarded_input(torch.cat([c.Q, c.K, c.V], 1), dev)
        Q, K, V = f[:, :d], f[:, d:2 * d], f[:, 2 * d:]
    elif c.operands == "kv":
        f = guarded_input(torch.cat([c.K, c.V], 1), dev)
        Q, K, V = guarded_input(c.Q, dev), f[:, :d], f[:, d:]
    elif c.operands == "k_is_v":
        Q = guarded_input(c.Q, dev)
        K = V = guarded_input(c.K, dev)
    else:
        Q, K, V = (guarded_input(t, dev) for t in (c.Q, c.K, c.V))
    return Q, K, V, (None if c.dO is None else guarded_input(c.dO, dev)), (None if c.mask is None else c.mask.to(dev))


def fwd_guards(c, dev, want_P=True):
    g = dict(O=Guarded(c.B * c.Lq, c.d, BF16, dev), lse=Guarded.vec(c.H * c.B * c.Lq, F32, dev))
    if want_P:           # (8 guard rows: any Lk keeps the window 16-byte aligned)
        g["P"] = Guarded(c.B * c.H * c.Lq, c.Lk, F32, dev, pad_rows=8, pad_cols=(0, 0), shape=(c.B, c.H, c.Lq, c.Lk))
    return g


def bwd_guards(c, dev):
    return dict(delta=Guarded.vec(c.H * c.B * c.Lq, F32, dev), dQ=Guarded(c.B * c.Lq, c.d, BF16, dev),
                dK=Guarded(c.B * c.Lk, c.d, BF16, dev), dV=Guarded(c.B * c.Lk, c.d, BF16, dev))


def intact(g, what):
    for nm, gd in g.items():
        gd.assert_intact("%s %s" % (what, nm))


def unwritten(g, what):
    """No element of any buffer - its window included - was written."""
    for nm, gd in g.items():
        gd.assert_intact("%s %s" % (what, nm))
        gd.assert_untouched(torch.ones(gd.rows, dtype=torch.bool), "%s %s" % (what, nm))


def launch(c, be, want_P=True, backward=True, what="dense"):
    """Forward (and backward) of case c by the backend's kernels: every output in a guard, every operand in NaN surroundings;
    the guards are looked at after each launch.  -> namespace(g = the guards by output name, ops, drop)."""
    dev = be.device
    Q, K, V, dO, mask = place(c, dev)
    drop = be.drop(c)
    g = fwd_guards(c, dev, want_P)
    be.k.attn_dense_fwd(Q, K, V, mask, g["O"].view, g["lse"].view, c.B, c.H, c.Lq, c.Lk, c.scale, drop=drop,
                        probs=g["P"].view if want_P else None)
    intact(g, what + " after the forward:")
    if backward:
        g.update(bwd_guards(c, dev))
        be.k.attn_dense_bwd(Q, K, V, mask, dO, g["lse"].view, g["delta"].view, g["dQ"].view, g["dK"].view, g["dV"].view, c.B, c.H, c.Lq,
                            c.Lk, c.scale, drop=drop)
        intact(g, what + " after the backward:")
    return types.SimpleNamespace(g=g, ops=(Q, K, V, dO, mask), drop=drop)


def _first(cond):
    return torch.nonzero(cond)[0].tolist()


def verify(c, o, what="dense", tol=L_DENSE):
    """Every output of ``launch`` against the case's fp64 reference: the exact assertions first (dead rows, dead keys, masked
    entries, row sums), then whole-tensor and local bounds through ``check`` (non-finite values fail too)."""
    B, H, Lq, Lk = c.B, c.H, c.Lq, c.Lk
    intact(o.g, what)
    out = {nm: gd.view.detach().cpu() for nm, gd in o.g.items()}
    dq_rows, dk_rows = c.dead_q.reshape(-1), c.dead_k.reshape(-1)                   # rows of the [B L, d] matrices
    dq_vec = c.dead_q.reshape(1, -1).expand(H, -1).reshape(-1)                      # entries of the [H, B Lq] vectors
    for nm in ("O", "dQ"):
        if nm in out and bool((out[nm][dq_rows].float() != 0).any()):
            raise AssertionError("%s %s: dead row (every key masked) not exactly zero: row %d" %
                                 (what, nm, int(torch.nonzero(dq_rows)[_first(out[nm][dq_rows].float() != 0)[0]])))
    for nm in ("dK", "dV"):
        if nm in out and bool((out[nm][dk_rows].float() != 0).any()):
            raise AssertionError("%s %s: dead key (masked for every query) not exactly zero: row %d" %
                                 (what, nm, int(torch.nonzero(dk_rows)[_first(out[nm][dk_rows].float() != 0)[0]])))
    if not bool((out["lse"][dq_vec] == float("inf")).all()):
        raise AssertionError("%s lse: dead row without lse = +inf: entry %d" %
                             (what, int(torch.nonzero(dq_vec)[_first(out["lse"][dq_vec] != float("inf"))[0]])))
    if "delta" in out and bool((out["delta"][dq_vec] != 0).any()):
        raise AssertionError("%s delta: dead row with delta != 0" % what)
    if "P" in out:
        P = out["P"]
        if c.mask is not None:
            hit = (P != 0) & c.mask.ne(0).view(B, 1, Lq, Lk)
            if bool(hit.any()):
                raise AssertionError("%s P: masked entry not exactly zero at (b, h, q, k) = %s (dead row: %s, dead key: %s)" % (
                    what, _first(hit), bool(c.dead_q[_first(hit)[0], _first(hit)[2]]), bool(c.dead_k[_first(hit)[0], _first(hit)[3]])))
        live = ~c.dead_q.view(B, 1, Lq).expand(B, H, Lq)
        off = ((P.double().sum(-1) - 1).abs() > ROWSUM) & live
        if bool(off.any()):
            i = _first(off)
            raise AssertionError("%s P: live row (b, h, q) = %s sums to %.9g" % (what, i, float(P.double().sum(-1)[tuple(i)])))
    for nm in ("O", "P", "dQ", "dK", "dV", "delta"):
        if nm in out:
            check(out[nm], c.ref[nm], tol[nm], "%s %s" % (what, nm), tol_local=tol[nm])
    if bool((~dq_vec).any()):
        check(out["lse"][~dq_vec], c.ref["lse"][~dq_vec], tol["lse"], "%s lse" % what, tol_local=tol["lse"])


def run(c, be, what="dense", **kw):
    o = launch(c, be, what=what, **kw)
    verify(c, o, what)
    return o


# ---- the kept set, read out exactly ------------------------------------------------------------------------------------------------
def blocks(L, dk):
    """Starts of d_k-wide blocks that cover 0 .. L - 1 (the last one overlaps its neighbour when d_k does not divide L)."""
    s = list(range(0, L - dk + 1, dk))
    return s if s[-1] + dk == L else s + [L - dk]


def build_readout(B, H, dk, Lq, Lk, p, salt=13):
    """Small scores (P near uniform: no kept entry can round to a bf16 zero), no mask."""
    c = build(B, H, dk, Lq, Lk, sharp=0.5, p=p, salt=salt)
    assert float(c.ref["P"].min()) * c.keep_scale > 1e-6
    return c


def _onehot(c, rows_per_utt, r0):
    """[B rows_per_utt, d]: row r0 + i of every utterance is the unit vector i of every head."""
    X = torch.zeros(c.B * rows_per_utt, c.d, dtype=BF16)
    for b in range(c.B):
        for h in range(c.H):
            X[b * rows_per_utt + r0 + torch.arange(c.dk), h * c.dk + torch.arange(c.dk)] = 1
    return X


def read_keep_fwd(c, be):
    """The forward's kept set [B H, Lq, Lk]: with V one-hot over keys k0 .. k0 + d_k - 1, O[q, i] = Pd[q, k0 + i]."""
    got = torch.zeros(c.B, c.H, c.Lq, c.Lk, dtype=torch.bool)
    for k0 in blocks(c.Lk, c.dk):
        o = launch(variant(c, V=_onehot(c, c.Lk, k0), operands="separate"), be, want_P=False, backward=False, what="read-out of O")
        O = o.g["O"].view.detach().cpu().float()
        assert bool(torch.isfinite(O).all()), "read-out of O: non-finite output"
        got[..., k0:k0 + c.dk] = O.view(c.B, c.Lq, c.H, c.dk).permute(0, 2, 1, 3) != 0
    return got.view(c.B * c.H, c.Lq, c.Lk)


def read_keep_bwd(c, be):
    """The key-side kernel's kept set: with dO one-hot over queries q0 .. q0 + d_k - 1, dV[k, i] = Pd[q0 + i, k]."""
    got = torch.zeros(c.B, c.H, c.Lq, c.Lk, dtype=torch.bool)
    for q0 in blocks(c.Lq, c.dk):
        o = launch(variant(c, dO=_onehot(c, c.Lq, q0)), be, want_P=False, what="read-out of dV")
        dV = o.g["dV"].view.detach().cpu().float()
        assert bool(torch.isfinite(dV).all()), "read-out of dV: non-finite output"
        got[:, :, q0:q0 + c.dk, :] = dV.view(c.B, c.Lk, c.H, c.dk).permute(0, 2, 3, 1) != 0
    return got.view(c.B * c.H, c.Lq, c.Lk)


def assert_keep_equal(got, keep, what):
    """No tolerance: output == 0 exactly where keep_qk says dropped, != 0 where it says kept."""
    bad = got != keep
    if bool(bad.any()):
        bh, q, k = _first(bad)
        raise AssertionError("%s: the kept set differs from keep_qk in %d of %d pairs, first at (bh, q, k) = (%d, %d, %d): %s, keep_qk says %s"
                             % (what, int(bad.sum()), bad.numel(), bh, q, k, "kept" if got[bh, q, k] else "dropped",
                                "kept" if keep[bh, q, k] else "dropped"))


def assert_same_bits(a, b, what):
    a, b = a.detach().cpu().contiguous(), b.detach().cpu().contiguous()
    same = a.view(torch.int32) == b.view(torch.int32)
    if a.shape != b.shape or not bool(same.all()):
        raise AssertionError("%s: not bit-identical, first difference at %s" % (what, _first(~same)))


# ---- the case lists -----------------------------------------------------------------------------------------------------------------
def case_id(kw):
    s = "%dx%dx%d-%dx%d-%s" % (kw["B"], kw["H"], kw["dk"], kw["Lq"], kw["Lk"], kw.get("mask", "none"))
    for k in ("operands", "sharp", "needle", "p"):
        if k in kw:
            s += "-%s%s" % (k, kw[k])
    return s


def dense_cases():
    """Every dense case of the GPU test that is compared with the fp64 reference, as build() keywords."""
    cases = []
    for i, (B, H, dk, Lq, Lk) in enumerate(GRID):
        for mask in (("none", "utt") if Lq * Lk == 1 else MASKS):
            cases.append(dict(B=B, H=H, dk=dk, Lq=Lq, Lk=Lk, mask=mask, gseed=i))
    for B, H, dk, L in [(2, 3, 32, 70), (2, 2, 64, 260)]:                                 # where the operands come from
        for operands in ("qkv", "kv", "k_is_v", "separate"):
            cases.append(dict(B=B, H=H, dk=dk, Lq=L, Lk=L, mask="dead", operands=operands, gseed=20))
    cases.append(dict(B=2, H=2, dk=64, Lq=7, Lk=300, mask="rand30", operands="kv", gseed=21))
    cases.append(dict(B=2, H=2, dk=64, Lq=7, Lk=300, mask="rand30", operands="k_is_v", gseed=21))
    for B, H, dk, Lq, Lk in [(3, 3, 32, 5, 65), (2, 2, 64, 7, 600), (2, 2, 64, 257, 300), (2, 1, 128, 7, 300), (2, 3, 96, 300, 9)]:
        for mask in ("none", "rand30"):                                                  # sharp attention
            cases.append(dict(B=B, H=H, dk=dk, Lq=Lq, Lk=Lk, mask=mask, sharp=3.0, gseed=30))
    for B, H, dk, Lq, Lk in [(2, 2, 64, 7, 257), (2, 2, 64, 7, 600), (2, 2, 64, 257, 300), (2, 1, 128, 7, 300), (3, 3, 32, 5, 65)]:
        cases.append(dict(B=B, H=H, dk=dk, Lq=Lq, Lk=Lk, needle=True, gseed=40))          # needles at Lk - 1 and at key 256
    cases.append(dict(B=2, H=2, dk=64, Lq=7, Lk=600, needle=True, sharp=3.0, mask="bytes", gseed=41))
    for B, H, dk, Lq, Lk, p in [(2, 3, 16, 5, 6, 0.5), (2, 3, 16, 5, 8, 0.5), (3, 3, 32, 5, 65, 0.1), (2, 2, 64, 257, 300, 0.1),
                                (2, 2, 64, 257, 300, 0.5), (2, 3, 96, 300, 9, 0.5), (2, 1, 128, 7, 300, 0.1)]:
        for mask in ("none", "dead"):                                                    # dropout, P requested with it
            cases.append(dict(B=B, H=H, dk=dk, Lq=Lq, Lk=Lk, mask=mask, p=p, gseed=50))
    return [(case_id(kw), kw) for kw in cases]


def lds_cases():
    """B = H = 1, d_k = 8: the largest extents each kernel accepts, and what the next one up must do.
    (name, accepted build() keywords, refused Lq, refused Lk)"""
    dk = 8
    lk_bwd, lk_fwd, lq_kv = (LDS_FLOATS - 6 * dk - 4) // 2, LDS_FLOATS - 5 * dk - 4, (LDS_FLOATS - 10 * dk) // 2
    assert 2 * lk_bwd + 6 * dk + 4 == LDS_FLOATS and 2 * lq_kv + 10 * dk == LDS_FLOATS
    return [("bwd_query_side", dict(B=1, H=1, dk=dk, Lq=2, Lk=lk_bwd, mask="rand30", gseed=60), 2, lk_bwd + 1),
            ("fwd", dict(B=1, H=1, dk=dk, Lq=2, Lk=lk_fwd, mask="rand30", backward=False, gseed=61), 2, lk_fwd + 1),
            ("bwd_key_side", dict(B=1, H=1, dk=dk, Lq=lq_kv, Lk=3, mask="rand30", gseed=62), lq_kv + 1, 3)]


# ---- st_attn_probs --------------------------------------------------------------------------------------------------------------------
PROBS_SHAPES = [(3, 3, 32), (2, 2, 64), (2, 1, 128)]
PROBS_LK = (65, 256, 257, 600)


def probs_cases():
    cases = []
    for B, H, dk in PROBS_SHAPES:
        for Lk in PROBS_LK:
            for packed in (False, True):
                for causal in (False, True):
                    for prescaled in (False, True):
                        cases.append(dict(B=B, H=H, dk=dk, Lk=Lk, packed=packed, causal=causal, prescaled=prescaled))
    return cases


def build_probs(B, H, dk, Lk, packed, causal, prescaled):
    """Ragged lengths (1 included); causal: self-attention (Lq = Lk, the diagonal crosses the 256-key stride), else 9 queries."""
    gen = torch.Generator().manual_seed(B * 1000 + Lk + dk)
    d, scale = H * dk, 1.0 / math.sqrt(dk)
    k_len = {3: [Lk, 1, Lk - 5], 2: [Lk, Lk // 2 + 1] if H == 2 else [1, Lk]}[B]
    Lq = Lk if causal else 9
    q_len = list(k_len) if causal else {3: [9, 7, 1], 2: [1, 9] if H == 2 else [9, 4]}[B]
    offs = lambda lens, L: [sum(lens[:b]) for b in range(B)] if packed else [b * L for b in range(B)]
    q_off, k_off = offs(q_len, Lq), offs(k_len, Lk)
    Mq, Mk = (sum(q_len), sum(k_len)) if packed else (B * Lq, B * Lk)
    Q = (torch.randn(Mq, d, generator=gen) * 1.5).to(BF16)
    K = (torch.randn(Mk, d, generator=gen) * 1.5).to(BF16)
    if prescaled:
        K = (K.float() * (scale * math.log2(math.e))).to(BF16)
    c = types.SimpleNamespace(B=B, H=H, dk=dk, Lq=Lq, Lk=Lk, d=d, scale=scale, Q=Q, K=K, q_len=q_len, k_len=k_len, q_off=q_off, k_off=k_off,
                              causal=causal, prescaled=prescaled)
    c.ref = ref.attention_probs(Q, K, q_len, k_len, (q_off, k_off), H, Lq, Lk, causal, scale, prescaled)
    q, k = torch.arange(Lq).view(1, Lq, 1), torch.arange(Lk).view(1, 1, Lk)
    z = (q >= torch.tensor(q_len).view(B, 1, 1)) | (k >= torch.tensor(k_len).view(B, 1, 1))
    c.zero = (z | (k > q)) if causal else z.expand(B, Lq, Lk)                    # [B, Lq, Lk]: must be exactly 0
    return c


def run_probs(c, be, what="attn_probs", tamper=None):
    dev = be.device
    ti = lambda v: torch.tensor(v, dtype=I32, device=dev)
    gd = Guarded(c.B * c.H * c.Lq, c.Lk, F32, dev, pad_rows=8, pad_cols=(0, 0), shape=(c.B, c.H, c.Lq, c.Lk))
    be.k.attn_probs(guarded_input(c.Q, dev), guarded_input(c.K, dev), ti(c.q_off), ti(c.q_len), ti(c.k_off), ti(c.k_len), c.H, c.Lq, c.Lk,
                    c.causal, c.scale, k_prescaled=c.prescaled, out=gd.view)
    if tamper is not None:
        tamper(gd.view)
    gd.assert_intact(what)
    P = gd.view.detach().cpu()
    hit = (P != 0) & c.zero.view(c.B, 1, c.Lq, c.Lk)
    if bool(hit.any()):
        raise AssertionError("%s: an entry of a padding query, past k_len or past the diagonal is not exactly zero at (b, h, q, k) = %s"
                             % (what, _first(hit)))
    check(P, c.ref, L_PROBS64, what, tol_local=L_PROBS64)
    return P


# ---- the module boundary: MultiHeadAttention in training mode through the dense path -----------------------------------------------------
def run_module_dropout(device):
    """MultiHeadAttention(...).train(), p = 0.1, a foreign mask and k is not v: output and input gradients against an fp64 module
    that applies keep_qk for the (seed, salt) rng.site handed out; the returned attns equal the eval-mode ones (deviation A1)."""
    import transformer.Attention as A
    from st_amd import rng
    from tests._local import rel

    B, Lq, Lk, d, H = 2, 70, 300, 128, 4
    dk = d // H
    torch.manual_seed(5)
    mha = A.MultiHeadAttention(H, d, dk, dk, dropout=0.1)
    gen = torch.Generator().manual_seed(6)
    x = [torch.randn(B, L, d, generator=gen).to(BF16).float() for L in (Lq, Lk, Lk)]
    dy = torch.randn(B, Lq, d, generator=gen)
    mask = torch.rand(B, Lq, Lk, generator=gen) < 0.3
    mask[1, 17] = True                                                    # a dead row
    W = {n: p.detach().double() for n, p in mha.named_parameters()}
    mha = mha.to(device).train()
    mha.return_attn = True
    rng.manual_seed(4242)
    xs = [t.to(device).requires_grad_(True) for t in x]
    out, attn = mha(*xs, mask.to(device))
    (out * dy.to(device)).sum().backward()
    seed, salt = int(rng.seed_tensor(device).item()), rng._salt
    # fp64, fp32 master weights
    de = em.Drop(torch.tensor([seed], dtype=I32), salt, 0.1)
    keep = torch.stack([em.keep_qk(de, bh, Lq, Lk) for bh in range(B * H)]).view(B, H, Lq, Lk).double() * de.scale
    x64 = [t.double().requires_grad_(True) for t in x]
    proj = lambda t, n, L: (t @ W["linear_%s.weight" % n].t() + W["linear_%s.bias" % n]).view(B, L, H, dk).transpose(1, 2)
    q, k, v = proj(x64[0], "q", Lq), proj(x64[1], "k", Lk), proj(x64[2], "v", Lk)
    s = (q @ k.transpose(-1, -2) / math.sqrt(dk)).masked_fill(mask.view(B, 1, Lq, Lk), float("-inf"))
    dead = mask.all(-1).view(B, 1, Lq, 1)
    P = torch.softmax(s.masked_fill(dead, 0.0), -1) * (~dead)
    ctx = ((P * keep) @ v).transpose(1, 2).reshape(B, Lq, d)
    y = torch.nn.functional.layer_norm(ctx @ W["output_linear.weight"].t() + W["output_linear.bias"] + x64[0], (d,), W["layernorm.weight"],
                                       W["layernorm.bias"], 1e-6)
    grads = torch.autograd.grad((y * dy.double()).sum(), x64)
    assert torch.isfinite(out).all()
    assert rel(out.detach().cpu(), y.detach()) < 2e-2, rel(out.detach().cpu(), y.detach())
    assert rel(attn.detach().cpu(), P.detach()) < 2e-2
    for nm, t, gref in zip("qkv", xs, grads):
        assert torch.isfinite(t.grad).all()
        assert rel(t.grad.cpu(), gref) < 6e-2, (nm, rel(t.grad.cpu(), gref))
    mha.eval()
    with torch.no_grad():
        _, attn_eval = mha(*[t.detach() for t in xs], mask.to(device))
    assert_same_bits(attn, attn_eval, "attns in training mode against eval mode (A1: the probabilities before dropout)")
