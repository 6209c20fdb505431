"""Cases and checks of the sharp-score attention tests: every family of the fast attention kernels (st_attn_fwd / st_attn_bwd:
csrc/st_attn.hip, st_attn64.hip, st_attn_xs.hip, st_attn_bwd64.hip) against the plain fp64 reference
tests/_attn_ref.packed_attention, with q and k of the size a trained model has (1 - 3 x N(0, 0.7): peaky attention at 3).  Shared
by tests/test_sharp_attention_gpu.py (the kernels), tests/test_sharp_attention_cpu.py (the emulation, with defects injected, so
the checks are known to see them), tools/local_bounds.py (family "sharp") and tools/attn_sharp_table.py.  A ``Backend`` says
whose attn_fwd / attn_bwd run and where; inputs, guards, reference, floors and assertions are the same code for all of them.

Bounds - none is tuned against a kernel:
  whole tensor   relL2(kernel - fp64) <= MARGIN x floor for O, dQ, dK, dV, floor = relL2(emulation - fp64) of the emulation run
                 with dtype = float64: the kernels' bf16 rounding points with exact arithmetic in between.  MARGIN = 1.25 is what
                 the project calls "as accurate as" (test_attention_backward_streams_stay_accurate_when_attention_is_sharp); two
                 correct implementations agree within 1 % (profiles/r05_bwd64_accuracy.txt), an operand rounded twice stands at
                 1.4 x or more.  Every floor is below L_BF16 = 1e-2 (asserted on the CPU), so MARGIN x floor is never looser than
                 the tolerances the other attention tests use.
  O + Ores       (two-term P) L_OSUM, see there.
  local          every row, column (O, dQ, dK, dV) and element (lse, delta) at L_ATTN, as in tests/test_kernels_gpu.py.
  exact          guards intact, rows of no utterance untouched, everything finite."""
import contextlib
import functools
import math
import os
import types

import torch

from tests import _attn_ref as ref
from tests import _emul as em
from tests._local import Guarded, check_local, guarded_input, rel

BF16, F32, F64, I32 = torch.bfloat16, torch.float32, torch.float64, torch.int32
K_LOG2_SCALE = math.log2(math.e)

MARGIN = 1.25
L_BF16 = 1e-2
L_ATTN = dict(O=1.5e-2, lse=2e-3, dQ=2.5e-2, dK=2.5e-2, dV=2e-2, delta=2e-3)       # tests/LOCAL_BOUNDS.md ("attention", and "sharp scores")
# O + Ores of the two-term-P forward against fp64, whole tensor and row by row.  What the sum must keep: Ores is bf16 of a remainder
# of at most 2^-9 |O| -> 2^-18 |O| = 3.8e-6 per element; P's second term likewise 2^-18 P; the fp32 arithmetic of both sides of an
# exp2(score - lse): a score of up to 2^6 (log2 units, the largest these inputs give is ~40) carries 2^-24 x 2^6 = 3.8e-6 absolute, and
# so does its subtraction from the maximum - P, and with it a row of O, is off by up to ln 2 x 7.6e-6 = 5.3e-6; a d_k-long fp32 dot
# product adds ~sqrt(128) x 2^-24 x 2^6 = 4.3e-5 to a score in the worst case of all products as large as the sum.  Together below
# 1e-4.  One-term P (the defect this bound is there for) leaves 2^-9 P per probability: with the few keys a peaky row looks at,
# 2^-9 / sqrt(12) .. 2^-9 = 5.6e-4 .. 2e-3 of the row.
L_OSUM = 1e-4
P_DROP = 26 / 256

OUT_FWD, OUT_BWD = ("O", "lse"), ("dQ", "dK", "dV")


class Backend:
    """Whose attn_fwd / attn_bwd run (st_amd.native or an object with tests._emul's signatures), on which device.  dtype: handed to
    the emulation (None: the backend takes no such keyword).  gpu: the environment switches and the key-split scratch exist."""

    def __init__(self, kernels, device, drop_cls, dtype=None, gpu=False):
        self.k, self.device, self.drop_cls, self.dtype, self.gpu = kernels, device, drop_cls, dtype, gpu

    def drop(self, c):
        return self.drop_cls(torch.tensor([c.seed], dtype=I32, device=self.device), c.salt, c.p) if c.p > 0 else None

    def _kw(self, kw):
        return kw if self.dtype is None else dict(kw, dtype=self.dtype)

    def fwd(self, *a, **kw):
        return self.k.attn_fwd(*a, **self._kw(kw))

    def bwd(self, *a, **kw):
        return self.k.attn_bwd(*a, **self._kw(kw))

    @contextlib.contextmanager
    def switches(self, env, split=True):
        """The development switches of the dispatch (ST_ATTN_XS, ST_ATTN_BWD64: read again through env_refresh) for the calls inside;
        split = False: st_attn_bwd gets no key-split scratch (the wrapper asks st_attn_bwd_split_kib how much to hand over)."""
        if not self.gpu:
            yield
            return
        from st_amd import native as nv
        cdll = nv.load()._cdll
        old = {k: os.environ.get(k) for k in env}
        kib = cdll.st_attn_bwd_split_kib
        try:
            os.environ.update(env)
            nv.env_refresh()
            if not split:
                cdll.st_attn_bwd_split_kib = lambda *a: 0
            yield
        finally:
            cdll.st_attn_bwd_split_kib = kib
            for k, v in old.items():
                if v is None:
                    os.environ.pop(k, None)
                else:
                    os.environ[k] = v
            nv.env_refresh()


CPU = Backend(em, "cpu", em.Drop, dtype=F32)            # the emulation as the other kernel tests use it
CPU64 = Backend(em, "cpu", em.Drop, dtype=F64)          # ... with exact arithmetic between its bf16 rounding points: the floor


def gpu_backend():
    from st_amd import native as nv
    return Backend(nv, "cuda", nv.Drop, gpu=True)


# ---- the case list --------------------------------------------------------------------------------------------------------------------
# family, name, d_k, q_lens (None: self-attention), k_lens, then keywords: causal, packed, prescaled, ores, fwd / bwd (run that pass),
# o_given (the two-launch backward: O handed over, parts 1 then 2), env, split.  H = 2 throughout.  Shapes: the smallest at which the
# dispatch of csrc/st_attn.hip (key_split, fwd_long64, bwd_long64, fwd_xs) reaches each kernel, with a one-row utterance, tails that
# are no multiple of 32 / 64 / 128 and more than one tile where the kernel loops.
XQ, XK = [64, 1, 40], [256, 300, 129]                 # few queries against many keys (xsplit_for: 3 workgroups per dQ item)
_FAMILIES = [
    ("general", "dk64-causal", 64, None, [64, 40, 1], dict(causal=True)),
    ("general", "dk32-causal", 32, None, [129, 33, 1], dict(causal=True)),
    ("general", "dk128", 128, None, [200, 64], {}),
    ("general", "dk64", 64, None, [128, 65], {}),
    ("general", "dk64-padded", 64, None, [128, 65], dict(packed=False)),
    ("psplit", "dk64-causal", 64, None, [64, 40, 1], dict(causal=True, ores=True)),
    ("psplit", "dk32-cross", 32, [33, 64, 2], [200, 65, 129], dict(ores=True)),
    ("ks2", "dk32", 32, XQ, XK, {}),
    ("ks2", "dk32-nosplit", 32, XQ, XK, dict(split=False, fwd=False)),
    ("ks2", "dk128", 128, XQ, XK, {}),
    ("ks2", "dk128-nosplit", 128, XQ, XK, dict(split=False, fwd=False)),
    ("ks2", "dk64-xs0", 64, XQ, XK, dict(env={"ST_ATTN_XS": "0"})),
    ("ks2", "dk64-xs0-nosplit", 64, XQ, XK, dict(env={"ST_ATTN_XS": "0"}, split=False, fwd=False)),
    ("xs", "dk64", 64, XQ, XK, dict(bwd=False)),
    ("xs", "dk64-ores", 64, XQ, XK, dict(ores=True, bwd=False)),
    ("fwd64", "plain", 64, None, [257, 129, 191], dict(bwd=False)),
    ("fwd64", "prescaled", 64, None, [257, 129, 191], dict(prescaled=True, bwd=False)),
    ("bwd64", "prescaled", 64, None, [257, 129, 191], dict(prescaled=True, fwd=False)),
    ("bwd64", "prescaled-padded", 64, None, [191, 130], dict(prescaled=True, packed=False, fwd=False)),
    ("bwd64", "plain", 64, None, [257, 129, 191], dict(fwd=False)),                       # plain keys: the general kernels serve them
    ("bwd64", "plain-padded", 64, None, [191, 130], dict(packed=False, fwd=False)),
    ("two-launch", "ks1-dk64", 64, None, [128, 65], dict(o_given=True, fwd=False)),
    ("two-launch", "ks2-dk32", 32, XQ, XK, dict(o_given=True, fwd=False)),
]
_DROPOUT = [("general", "dk64-causal"), ("psplit", "dk32-cross"), ("ks2", "dk128"), ("xs", "dk64"), ("fwd64", "plain"), ("bwd64", "prescaled"),
            ("two-launch", "ks1-dk64")]
SHARP = (1, 2, 3)


def cases():
    """[(id, build() keywords)]: every family at s = 1, 2, 3 and, at s = 3, one case per family with dropout p = 26 / 256."""
    out = []
    for fam, name, dk, ql, kl, kw in _FAMILIES:
        for s in SHARP:
            out.append(("%s-%s-s%d" % (fam, name, s), dict(kw, family=fam, name=name, dk=dk, q_lens=ql, k_lens=kl, s=s)))
        if (fam, name) in _DROPOUT:
            out.append(("%s-%s-s3-drop" % (fam, name), dict(kw, family=fam, name=name, dk=dk, q_lens=ql, k_lens=kl, s=3, p=P_DROP)))
    return out


def build(family, name, dk, q_lens, k_lens, s, causal=False, packed=True, prescaled=False, ores=False, fwd=True, bwd=True, o_given=False,
          env=None, split=True, p=0.0, H=2, salt=11, seed=7654321):
    """One case: the bf16 operands as the kernel gets them and the fp64 reference of every output.  Q, K = 0.7 s N(0, 1) rounded
    once; V = 0.7 N(0, 1); dO = 0.5 N(0, 1); pre-scaled keys K~ = bf16(k32 scale log2 e) from the fp32 keys, as the projection's
    epilogue forms them.  (Padded layouts: the rows between the utterances hold finite values nobody may use.)"""
    self_attn = q_lens is None
    ql = list(k_lens) if self_attn else list(q_lens)
    kl, B, d, scale = list(k_lens), len(k_lens), H * dk, 1.0 / math.sqrt(dk)
    if packed:
        q_off, k_off = [sum(ql[:i]) for i in range(B)], [sum(kl[:i]) for i in range(B)]
        Mq, Mk = sum(ql), sum(kl)
    else:
        q_off, k_off = [i * max(ql) for i in range(B)], [i * max(kl) for i in range(B)]
        Mq, Mk = B * max(ql), B * max(kl)
    gen = torch.Generator().manual_seed(1000 * dk + 10 * sum(kl) + s)
    rn = lambda rows, sc: torch.randn(rows, d, generator=gen) * sc
    q32, k32, V, dO = rn(Mq, 0.7 * s), rn(Mk, 0.7 * s), rn(Mk, 0.7).to(BF16), rn(Mq, 0.5).to(BF16)
    Q = q32.to(BF16)
    K = (k32 * (scale * K_LOG2_SCALE)).to(BF16) if prescaled else k32.to(BF16)
    c = types.SimpleNamespace(family=family, name=name, id="%s-%s-s%d%s" % (family, name, s, "-drop" if p > 0 else ""), H=H, dk=dk, d=d,
                              scale=scale, s=s, B=B, q_len=ql, k_len=kl, q_off=q_off, k_off=k_off, Mq=Mq, Mk=Mk, max_q=max(ql), max_k=max(kl),
                              causal=causal, packed=packed, prescaled=prescaled, ores=ores, fwd=fwd, bwd=bwd, o_given=o_given,
                              env=dict(env or {}), split=split, p=p, salt=salt, seed=seed, Q=Q, K=K, V=V, dO=dO, keep=None, keep_scale=1.0)
    if p > 0:
        de = em.Drop(torch.tensor([seed], dtype=I32), salt, p)
        c.keep = [em.keep_qk(de, b * H + h, ql[b], kl[b]) for b in range(B) for h in range(H)]
        c.keep_scale = de.scale
    c.rows = dict(q=_utt_rows(q_off, ql, Mq), k=_utt_rows(k_off, kl, Mk))
    names = ("O", "lse", "delta", "dQ", "dK", "dV")
    c.ref = dict(zip(names, ref.packed_attention(Q, K, V, dO, q_off, ql, k_off, kl, H, causal, scale, k_prescaled=prescaled, keep=c.keep,
                                                 keep_scale=c.keep_scale)))
    # what the backward is handed: lse and delta of the reference in fp32 (0 in the rows of no utterance), so that a backward is judged
    # on its own roundings; the two-launch form gets the reference's O rounded to bf16 and writes delta = rowsum(dO O) itself
    c.lse_in, c.delta_in = c.ref["lse"].to(F32), c.ref["delta"].to(F32)
    c.O_in = c.ref["O"].to(BF16)
    c.delta_of_O = (dO.double() * c.O_in.double()).view(Mq, H, dk).sum(-1).t().reshape(-1)
    if o_given:
        # ... and is judged on its own roundings too: dQ / dK as exact arithmetic makes them of the delta it forms from that O.  (Against
        # the reference's own delta the rounding of O alone - not the backward's - moves single rows of dQ by 3.7e-2 at s = 3: what
        # Ores is there for in the product.)
        c.ref.update(zip(OUT_BWD, ref.packed_attention(Q, K, V, dO, q_off, ql, k_off, kl, H, causal, scale, k_prescaled=prescaled, keep=c.keep,
                                                       keep_scale=c.keep_scale, delta_in=c.delta_of_O)[3:]))
    return c


def _utt_rows(off, lens, total):
    m = torch.zeros(total, dtype=torch.bool)
    for o, n in zip(off, lens):
        m[o:o + n] = True
    return m


def side(nm):
    return "k" if nm in ("dK", "dV") else "q"


# ---- running a case -------------------------------------------------------------------------------------------------------------------
def launch(c, be, what=None):
    """The case's forward and / or backward by the backend's kernels: outputs in guards, operands in NaN surroundings.
    -> {output name: Guarded}"""
    dev, what = be.device, what or c.id
    Q, K, V, dO = (guarded_input(t, dev) for t in (c.Q, c.K, c.V, c.dO))
    ti = lambda v: torch.tensor(v, dtype=I32, device=dev)
    meta = [ti(c.q_off), ti(c.q_len), ti(c.k_off), ti(c.k_len)]
    drop = be.drop(c)
    g = {}
    with be.switches(c.env, c.split):
        if c.fwd:
            g["O"], g["lse"] = Guarded(c.Mq, c.d, BF16, dev), Guarded.vec(c.H * c.Mq, F32, dev)
            if c.ores:
                g["Ores"] = Guarded(c.Mq, c.d, BF16, dev)
            be.fwd(Q, K, V, g["O"].view, g["lse"].view, *meta, c.H, c.max_q, c.causal, c.scale, drop=drop, max_k=c.max_k,
                   ores=g["Ores"].view if c.ores else None, k_prescaled=c.prescaled)
            intact(g, what + " after the forward")
        if c.bwd:
            b = dict(dQ=Guarded(c.Mq, c.d, BF16, dev), dK=Guarded(c.Mk, c.d, BF16, dev), dV=Guarded(c.Mk, c.d, BF16, dev))
            out = [b[n].view for n in OUT_BWD]
            lse = c.lse_in.to(dev)
            tail = (*meta, c.H, c.max_q, c.max_k, c.causal, c.scale)
            if c.o_given:
                b["delta"] = Guarded.vec(c.H * c.Mq, F32, dev)
                for parts in (1, 2):
                    be.bwd(Q, K, V, guarded_input(c.O_in, dev), dO, lse, b["delta"].view, *out, *tail, parts=parts, drop=drop,
                           k_prescaled=c.prescaled)
            else:
                be.bwd(Q, K, V, None, dO, lse, c.delta_in.to(dev), *out, *tail, drop=drop, k_prescaled=c.prescaled)
            g.update(b)
            intact(g, what + " after the backward")
    return g


def intact(g, what):
    for nm, gd in g.items():
        gd.assert_intact("%s: %s" % (what, nm))


def outputs(c, g):
    """The guards' windows on the CPU, and O + Ores in fp64 where the forward formed P of two terms (a.psplit of st_attn_fwd: Ores
    given, at most 64 queries; the dropout variants are not held to it)."""
    out = {nm: gd.view.detach().cpu() for nm, gd in g.items()}
    if "Ores" in out and c.max_q <= 64 and c.p == 0:
        out["O+Ores"] = out["O"].double() + out["Ores"].double()
    return out


def errors(c, out):
    """relL2 against the fp64 reference over the utterances' rows, per bf16 output (and O + Ores)."""
    e = {}
    for nm in ("O", "dQ", "dK", "dV", "O+Ores"):
        if nm in out:
            rows = c.rows[side(nm)]
            e[nm] = rel(out[nm][rows], c.ref["O" if nm == "O+Ores" else nm][rows])
    return e


@functools.lru_cache(maxsize=None)
def _floors(key):
    c = build(**dict(key))
    return errors(c, outputs(c, launch(c, CPU64, what=c.id + " (floor)")))


def floors(kw):
    """The case's floors: the emulation with exact arithmetic between its bf16 rounding points against the fp64 reference."""
    return _floors(tuple(sorted((k, (tuple(v) if isinstance(v, list) else tuple(sorted(v.items())) if isinstance(v, dict) else v))
                                for k, v in kw.items())))


def verify(c, g, floor, what=None, report=None):
    """Every output of ``launch`` against the case's reference.  report: a list that receives (output, floor, error, ratio) rows."""
    what = what or c.id
    intact(g, what)
    out = outputs(c, g)
    H = c.H
    for nm, gd in g.items():
        rows = c.rows[side(nm)]
        t = out[nm]
        if t.dim() == 1:          # lse / delta: [H, rows]
            live = t.view(H, -1)[:, rows]
            assert bool(torch.isnan(t.view(H, -1)[:, ~rows]).all()), "%s %s: an entry of a row that belongs to no utterance was written" % (what, nm)
        else:
            live = t[rows]
            if not bool(rows.all()):
                gd.assert_untouched(~rows, "%s %s" % (what, nm))
        assert bool(torch.isfinite(live.float()).all()), "%s %s: non-finite output" % (what, nm)
    failed = []
    for nm, e in errors(c, out).items():
        bound = L_OSUM if nm == "O+Ores" else MARGIN * floor[nm]
        print("sharp %s %s: relL2 vs fp64 %.3e, floor %.3e, ratio %.3f (bound %.3e)" % (what, nm, e, floor[nm], e / floor[nm], bound))
        if report is not None:
            report.append((nm, floor[nm], e, e / floor[nm]))
        if not e <= bound:
            failed.append("%s: relL2 %.3e > %.3e (floor %.3e, ratio %.3f)" % (nm, e, bound, floor[nm], e / floor[nm]))
    if failed:
        raise AssertionError("%s: less accurate than its rounding points allow - %s" % (what, "; ".join(failed)))
    for nm in ("O", "dQ", "dK", "dV"):
        if nm in out:
            rows = c.rows[side(nm)]
            check_local(out[nm][rows], c.ref[nm][rows], L_ATTN[nm], "%s %s" % (what, nm))
    if "O+Ores" in out:
        check_local(out["O+Ores"][c.rows["q"]], c.ref["O"][c.rows["q"]], L_OSUM, "%s O + Ores" % what)
    for nm, r in (("lse", c.ref["lse"]), ("delta", c.delta_of_O)):
        if nm in out:
            rows = c.rows["q"]
            check_local(out[nm].view(H, -1)[:, rows].reshape(-1), r.view(H, -1)[:, rows].reshape(-1), L_ATTN[nm], "%s %s" % (what, nm))


def run(kw, be, report=None):
    c = build(**kw)
    verify(c, launch(c, be), floors(kw), report=report)
    return c
