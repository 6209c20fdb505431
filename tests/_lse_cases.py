"""The vocabulary log-sum-exp family: the logits-row families, the checks and the per-kernel runners that
tests/test_lse_fp64_gpu.py (the HIP kernels through st_amd.native) and tests/test_lse_fp64_cpu.py (the emulations, and the same
checks shown to see injected defects) share; tools/local_bounds.py measures the two bounds L_LSE and P_REL from the fp32 restatements
at the end of this file.  Reference: tests/_lse_ref.py (plain fp64).  Where the bounds come from: tests/LOCAL_BOUNDS.md.

Eight kernels carry their own log-sum-exp over the vocabulary (include/st_hip.h): st_ce_fwd / st_ce_bwd, st_ce_smooth_fwd / _bwd,
st_ce_eval_fwd, st_ctc_gather / st_ctc_dlogits (16-byte loads when ldl % 4 == 0, scalar loads otherwise), st_ctc_vocab_lp,
st_beam_advance without and with `work`, st_beam_pre_beam; st_ctc_best_path shares the rows for its arg-max.  Every logits buffer
is a guarded_input whose columns >= V and surroundings are NaN; every output lives in a Guarded buffer."""
import math

import numpy as np
import torch

from tests import _lse_ref as ref
from tests._local import Guarded, check, guarded_input, guarded_like

F32, F64, BF16, I32, I64 = torch.float32, torch.float64, torch.bfloat16, torch.int32, torch.int64
INF = float("inf")

VS = (2, 5, 257, 513, 2049, 4337, 5120)      # one past the pass widths 256 / 512 / 2,048, production, the register kernels' limit
FAMILIES = ("legacy", "uniform", "one-hot", "ramp-up", "ramp-down", "peaked", "offset", "masked", "pad-counted")
NO_EXEMPTION = ("legacy", "peaked", "offset")             # families on which no choice may use the near-tie exemption
EXEMPT_SHARE = 0.02
IGNORE = -100
BEAM = 4
L_CE, L_BF16 = 6e-3, 1e-2                                 # the bounds in force for the bf16 gradients (tests/test_kernels_gpu.py)

# Measured by tools/local_bounds.py (family "lse"), never against a kernel - tests/LOCAL_BOUNDS.md has the tables:
#   L_LSE = 3 x the larger worst (|err| - ulp32(|ref|) / 2, clipped at 0) of two fp32 restatements of the sum against fp64
#   P_REL = 3 x the worst relative error of exp(x - lse32) in them, over the entries with p_ref >= 2^-100
L_LSE = 1.1e-5
P_REL = 1.0e-4
L_LSE_MAX = math.log(5120.0 / 5119.0) / 4                 # a dropped column at the largest V stands four bounds out
P_REL_MAX = 2.0 ** -10


def smooth_cfg(V):
    """The smoothed target the family is run with: (confidence, smooth, zero_col) - the mass 0.1 spread over the V - 2 columns that
    are neither the target nor column 0."""
    return 0.9, 0.1 / max(V - 2, 1), 0


PLAIN = (1.0, 0.0, -1)


def pre_beam_k(V):
    return min(V, 12)


# ---- the row families -----------------------------------------------------------------------------------------------------------------
class Case:
    """x f32 [R, V] (R a multiple of 4, at most 16), target i64 [R] (a finite column, or IGNORE), masked bool [R, V]; onehot: the
    column j of every row of one-hot@j; single: the row with one finite column."""

    def __init__(self, family, V, x, target, onehot=None, single=None, seed=0):
        self.family, self.V, self.x, self.target, self.onehot, self.single, self.seed = family, V, x, target, onehot, single, seed
        self.masked = torch.isinf(x) & (x < 0)
        self.valid = target != IGNORE
        self.tclamp = target.clamp_min(0)
        self.x64 = x.to(F64)
        self.lse = ref.lse(x)
        self.lp = ref.log_softmax(x)
        self.p = torch.exp(self.lp)
        fin = torch.where(self.masked, torch.zeros_like(self.x64), self.x64)
        self.max_abs = fin.abs().max(-1).values

    @property
    def R(self):
        return self.x.shape[0]


ONE_HOT_COLUMNS = (0, 1, 3, 4, 255, 256, 511, 512, 2047, 2048)


def onehot_columns(V):
    js = sorted({j for j in ONE_HOT_COLUMNS + (V - 2, V - 1) if 0 <= j < V})
    return (js * 4)[:-(-len(js) // 4) * 4]                # cycled up to a multiple of 4 rows


def _gen(family, V, seed):
    g = torch.Generator().manual_seed(seed)
    randn = lambda *s: torch.randn(*s, generator=g)
    randint = lambda n: torch.randint(0, V, (n,), generator=g)
    onehot = single = None
    if family in ("legacy", "pad-counted"):
        x, t = randn(8, V) * 3, randint(8)
        if family == "pad-counted":
            x[:, V - 7:] = -1e30
            t = torch.randint(0, V - 7, (8,), generator=g)
        else:
            t[1] = IGNORE
    elif family == "uniform":
        x = torch.tensor([0.0, -7.5, 100.0]).repeat_interleave(4).view(12, 1).expand(12, V).contiguous()
        t = randint(12)
    elif family == "one-hot":
        onehot = onehot_columns(V)
        x = torch.full((len(onehot), V), -40.0)
        x[torch.arange(len(onehot)), torch.tensor(onehot)] = 0.0
        # the target is j in every other row only: where it is j the whole gradient row cancels to ~V e^-40 (fp32 legitimately gives 0 at
        # the target), and the whole-tensor bound needs rows of ordinary size to be a statement at all
        t = torch.tensor(onehot)
        t[1::2] = (t[1::2] + 1) % V
    elif family in ("ramp-up", "ramp-down"):
        col = torch.arange(V, dtype=F64) / max(V - 1, 1)
        if family == "ramp-down":
            col = 1.0 - col
        x = (torch.tensor([0.0, -60.0, -120.0, 13.25], dtype=F64).view(4, 1) + 120.0 * col.view(1, V)).to(F32)
        t = randint(4)
    elif family == "peaked":
        x, t, at = randn(8, V), randint(8), randint(8)
        x[torch.arange(8), at] += torch.tensor([12.0] * 4 + [60.0] * 4)
        t[::2] = at[::2]                                   # the peak is the target in half of the rows
    elif family == "offset":
        x = randn(16, V) * 3 + torch.tensor([30.0, 100.0, 1000.0, -1000.0]).repeat_interleave(4).view(16, 1)
        t = randint(16)
    elif family == "masked":
        x = randn(8, V) * 3
        m = torch.rand(8, V, generator=g) < 0.3
        if V > 5:
            m[:, :4] = True
            m[:, V - 1] = True
            keep = V // 2
        else:                                              # only as many leading columns as leave one finite
            m[:] = False
            m[:, :min(4, V - 1)] = True
            keep = V - 1
        m[:, keep] &= torch.rand(8, generator=g) < 0.5
        for r in range(8):
            if bool(m[r].all()):
                m[r, keep] = False
        single = 7
        m[single] = True
        m[single, keep] = False
        x[m] = -INF
        t = torch.stack([torch.nonzero(~m[r]).flatten()[int(torch.randint(0, int((~m[r]).sum()), (1,), generator=g))] for r in range(8)])
    else:
        raise ValueError(family)
    return Case(family, V, x.to(F32).contiguous(), t.to(I64), onehot=onehot, single=single, seed=seed)


def family_vs(family):
    return tuple(V for V in VS if family != "pad-counted" or V > 16)


_CACHE = {}


def build(family, V):
    """The family's rows at V (built once, shared and left unchanged).  On the families of NO_EXEMPTION the seed is the first one for
    which the reference alone shows no pair of adjacent candidates closer than twice the log-probability bound, in any of the choice
    lists the kernels form (tests/test_lse_fp64_cpu.py asserts that)."""
    key = (family, V)
    if key not in _CACHE:
        for k in range(64):
            c = _gen(family, V, 1000 * FAMILIES.index(family) + V + 104729 * k)
            if family not in NO_EXEMPTION or not reference_near_ties(c):
                break
        else:
            raise AssertionError("no seed without a near tie for %s at V = %d" % (family, V))
        _CACHE[key] = c
    return _CACHE[key]


# ---- bounds and checks ----------------------------------------------------------------------------------------------------------------
def logp_bound(lse_ref, value_ref):
    """L_LSE + ulp32(|lse|) + ulp32(|ref|) of a derived log-probability (inf where the reference is infinite)."""
    return L_LSE + ref.ulp32(lse_ref) + torch.where(torch.isinf(value_ref), torch.full_like(value_ref, INF), ref.ulp32(value_ref))


class Report:
    """kernel x family x output -> the worst err / bound ratio over the V, with the figures at that point."""

    def __init__(self):
        self.rows = {}
        self.choices = {}          # (kernel, family) -> [rows, rows that used the near-tie exemption]

    def add(self, kernel, c, output, err, bound):
        err, bound = err.reshape(-1), bound.reshape(-1)
        if not err.numel():
            return
        ratio = torch.where(bound > 0, err / bound.clamp_min(1e-300), torch.where(err > 0, torch.full_like(err, INF), torch.zeros_like(err)))
        ratio = torch.nan_to_num(ratio, nan=INF, posinf=INF)
        i = int(ratio.argmax())
        key = (kernel, c.family, output)
        if key not in self.rows or float(ratio[i]) >= self.rows[key][0]:
            self.rows[key] = (float(ratio[i]), float(err[i]), float(bound[i]), c.V)

    def choice(self, kernel, c, rows, used):
        a = self.choices.setdefault((kernel, c.family), [0, 0])
        a[0] += rows
        a[1] += used

    def exempt_share(self):
        rows = sum(a[0] for a in self.choices.values())
        return sum(a[1] for a in self.choices.values()) / max(rows, 1)

    def table(self):
        out = ["# kernel x family x output: the worst |got - ref| / bound over the V of the family, with the figures at that point",
               "# L_LSE = %.3g, P_REL = %.3g (tests/_lse_cases.py); the exact (equality) checks follow the figures" % (L_LSE, P_REL),
               "%-28s %-12s %-16s %10s %10s %8s %6s" % ("kernel", "family", "output", "worst err", "bound", "ratio", "at V")]
        held = {}
        for (k, f, o), (ratio, err, bound, V) in sorted(self.rows.items()):
            if o.endswith(" (exact)"):
                held.setdefault((k, f), []).append(o[:-8] + ("" if ratio == 0 else " FAILED"))
            else:
                out.append("%-28s %-12s %-16s %10.3e %10.3e %8.3f %6d" % (k, f, o, err, bound, ratio, V))
        out.append("# exact checks (held unless marked)")
        for (k, f), names in sorted(held.items()):
            out.append("%-28s %-12s %s" % (k, f, ", ".join(names)))
        out.append("# choices (ids / back / toks): rows compared, rows that used the near-tie exemption")
        for (k, f), (rows, used) in sorted(self.choices.items()):
            out.append("%-28s %-12s %6d %4d" % (k, f, rows, used))
        out.append("# share of rows using the exemption: %.4f (cap %.2f)" % (self.exempt_share(), EXEMPT_SHARE))
        return "\n".join(out) + "\n"


def _cpu64(t):
    return t.detach().to("cpu").to(F64)


def within(rep, kernel, c, output, got, want, bound):
    """|got - want| <= bound element by element; where want is infinite got must equal it; nothing is NaN."""
    got, want = _cpu64(got), want.to(F64)
    bound = torch.as_tensor(bound, dtype=F64).expand_as(want)
    what = "%s %s V=%d %s" % (kernel, c.family, c.V, output)
    assert got.shape == want.shape, "%s: shape %s, reference %s" % (what, tuple(got.shape), tuple(want.shape))
    assert not bool(torch.isnan(got).any()), "%s: %d NaN values" % (what, int(torch.isnan(got).sum()))
    inf = torch.isinf(want)
    assert bool((got[inf] == want[inf]).all()), "%s: an infinite reference value is not reproduced exactly" % what
    err = (got[~inf] - want[~inf]).abs()
    b = bound[~inf]
    if rep is not None:
        rep.add(kernel, c, output, err, b)
    bad = ~(err <= b)
    if bool(bad.any()):
        i = int(torch.nan_to_num(err / b.clamp_min(1e-300), nan=INF).argmax())
        flat = torch.nonzero(~inf.reshape(-1)).flatten()[i]
        raise AssertionError("%s: %d of %d elements off bound; worst |err| %.3e > %.3e at flat index %d (got %.9g, reference %.9g)"
                             % (what, int(bad.sum()), err.numel(), float(err[i]), float(b[i]), int(flat), float(got[~inf][i]),
                                float(want[~inf][i])))


def exact(rep, kernel, c, output, ok, msg):
    ok = torch.as_tensor(ok)
    if rep is not None:
        rep.add(kernel, c, output + " (exact)", (~ok).to(F64).reshape(-1), torch.zeros(ok.numel(), dtype=F64))
    assert bool(ok.all()), "%s %s V=%d %s: %s (%d of %d)" % (kernel, c.family, c.V, output, msg, int((~ok).sum()), ok.numel())


def check_lse(rep, kernel, c, got, rows=None):
    """|got - ref| <= L_LSE + ulp32(|ref|); the single-finite-column row equals that logit bit for bit."""
    want = c.lse if rows is None else c.lse[rows]
    within(rep, kernel, c, "lse", got, want, L_LSE + ref.ulp32(want))
    if c.single is not None and (rows is None or c.single in rows.tolist()):
        i = c.single if rows is None else rows.tolist().index(c.single)
        only = c.x[c.single][~c.masked[c.single]]
        exact(rep, kernel, c, "lse single", got.detach().cpu()[i].view(1) == only, "the row with one finite column must return that logit")


def check_grad(rep, kernel, c, output, got_units, want, p_ref):
    """|got - ref| <= 2^-8 |ref| + P_REL p_ref + 2^-126 in probability units (one bf16 rounding; the fp32 error of the probability
    before the target is subtracted; values below the smallest normal fp32 may flush)."""
    within(rep, kernel, c, output, got_units, want, want.abs() * 2.0 ** -8 + P_REL * p_ref + 2.0 ** -126)


def near_ties(v, b):
    """Of a sorted candidate list's values and bounds [n, k + 1]: which adjacent pairs lie closer than twice the bound."""
    return ref.gaps(v) < 2 * torch.maximum(b[:, :-1], b[:, 1:])


def check_choice(rep, kernel, c, got_ids, table, bound_table, k):
    """got_ids i64 [n, k] against the reference's list (best first, lower index on ties).  A row may differ only by candidates whose
    reference values lie within twice the log-probability bound of the ones they stand for (adjacent near ties, at the cut or within
    the list); such rows are counted, never on the families of NO_EXEMPTION."""
    idx, v = ref.best(table, k)
    got_ids = got_ids.detach().cpu().to(I64)
    what = "%s %s V=%d choice" % (kernel, c.family, c.V)
    assert got_ids.shape == idx[:, :k].shape, what
    assert bool(((got_ids >= 0) & (got_ids < table.shape[1])).all()), "%s: an index outside the table" % what
    differ = (got_ids != idx[:, :k]).any(1)
    used = 0
    for i in torch.nonzero(differ).flatten().tolist():
        assert c.family not in NO_EXEMPTION, "%s: row %d differs from the reference list: got %s, reference %s" % (
            what, i, got_ids[i].tolist(), idx[i, :k].tolist())
        assert len(set(got_ids[i].tolist())) == k, "%s: row %d names a candidate twice: %s" % (what, i, got_ids[i].tolist())
        gv, gb = table[i, got_ids[i]], bound_table[i, got_ids[i]]
        d = (gv - v[i, :k]).abs()
        d = torch.where(torch.isnan(d), torch.zeros_like(d), d)
        lim = 2 * torch.maximum(gb, bound_table[i, idx[i, :k]])
        assert bool((d <= lim).all()) and bool(near_ties(v[i:i + 1], bound_table[i:i + 1].gather(1, idx[i:i + 1])).any()), \
            "%s: row %d is not the reference list and no near tie explains it: got %s, reference %s" % (
                what, i, got_ids[i].tolist(), idx[i, :k].tolist())
        used += 1
    if rep is not None:
        rep.choice(kernel, c, got_ids.shape[0], used)
    return idx, v


def beam_tables(c):
    """st_beam_advance's candidate table of the case: utterance b = rows b * BEAM .. + BEAM - 1 with scores that fall by 1.5 per
    slot -> (scores f32 [B, BEAM], table f64 [B, BEAM * V], bound table)."""
    B, V = c.R // BEAM, c.V
    scores = (-1.5 * torch.arange(BEAM, dtype=F32).view(1, BEAM) - 0.125 * torch.arange(B, dtype=F32).view(B, 1)).contiguous()
    table = (scores.to(F64).view(B, BEAM, 1) + c.lp.view(B, BEAM, V))
    bound = logp_bound(c.lse.view(B, BEAM, 1).expand(B, BEAM, V), table)
    return scores, table.reshape(B, BEAM * V), bound.reshape(B, BEAM * V)


def reference_near_ties(c):
    """Does the reference alone show adjacent candidates closer than twice the bound, in st_beam_pre_beam's or st_beam_advance's list?"""
    k = pre_beam_k(c.V)
    idx, v = ref.best(c.lp, k)
    hit = bool(near_ties(v, logp_bound(c.lse.view(-1, 1), c.lp).gather(1, idx)).any())
    if c.V >= BEAM + 1:
        _, table, bound = beam_tables(c)
        idx, v = ref.best(table, BEAM)
        hit = hit or bool(near_ties(v, bound.gather(1, idx)).any())
    return hit


# ---- backends -------------------------------------------------------------------------------------------------------------------------
class Backend:
    def __init__(self, name, dev, **fns):
        self.name, self.dev = name, dev
        self.__dict__.update(fns)


def gpu_backend():
    from st_amd import native as nv
    nv.load(build_if_missing=False)
    names = ("ce_fwd", "ce_bwd", "ce_smooth_fwd", "ce_smooth_bwd", "ce_eval_fwd", "ctc_gather", "ctc_dlogits", "ctc_vocab_lp",
             "beam_advance", "beam_work_words", "beam_pre_beam", "ctc_best_path")
    return Backend("gpu", "cuda", **{n: getattr(nv, n) for n in names})


def _vocab_lp32(logits, V, off, length, T_cap, lse, lpT):
    """Plain fp32 torch restatement of st_ctc_vocab_lp."""
    x = logits[:, :V].float()
    lse.copy_(torch.logsumexp(x, -1))
    lpT.zero_()
    for b in range(off.numel()):
        o, n = int(off[b]), int(length[b])
        lpT[b, :, :n] = (x[o:o + n] - lse[o:o + n].view(-1, 1)).t()


def _pre_beam32(logits, V, ids, lp):
    """Plain fp32 torch restatement of st_beam_pre_beam (stable sort: lower id on ties)."""
    x = logits[:, :V].float()
    v, i = torch.sort(x, dim=-1, descending=True, stable=True)
    K = ids.shape[1]
    ids.copy_(i[:, :K].to(I32))
    lp.copy_(v[:, :K] - torch.logsumexp(x, -1, keepdim=True))


def _best_path32(logits, V, out):
    x = logits[:, :V]
    cols = torch.arange(V).expand_as(x)
    out.copy_(torch.where(x == x.max(-1, keepdim=True).values, cols, torch.full_like(cols, V)).min(-1).values.to(I32))
    return out


def cpu_backend():
    from tests import _emul as em
    from tests import _emul_ce as emc
    from tests import _emul_eval as eme
    return Backend("cpu", "cpu", ce_fwd=em.ce_fwd, ce_bwd=em.ce_bwd, ce_smooth_fwd=emc.ce_smooth_fwd, ce_smooth_bwd=emc.ce_smooth_bwd,
                   ce_eval_fwd=eme.ce_eval_fwd, ctc_gather=em.ctc_gather, ctc_dlogits=em.ctc_dlogits, ctc_vocab_lp=_vocab_lp32,
                   beam_advance=em.beam_advance, beam_work_words=em.beam_work_words, beam_pre_beam=_pre_beam32,
                   ctc_best_path=_best_path32)


# ---- buffers --------------------------------------------------------------------------------------------------------------------------
def logits_buffer(be, x, ld_mod4=None):
    """x inside a NaN buffer: the window is wider than V, so columns >= V are NaN like the surroundings.  ld_mod4: None (any), True
    (leading dimension divisible by 4 and 16-byte aligned rows), False (not divisible by 4)."""
    R, V = x.shape
    w = V + 3 if ld_mod4 is None else (V + 3) // 4 * 4 + 4 + (0 if ld_mod4 else 1)
    t = torch.full((R, w), float("nan"), dtype=F32)
    t[:, :V] = x
    view = guarded_input(t, be.dev, pad_rows=8)            # (8 rows: the window starts 16-byte aligned at any width)
    assert ld_mod4 is None or (view.stride(0) % 4 == 0) == ld_mod4
    return view


def out_like(be, shape, dtype):
    """A Guarded output of ``shape`` (contiguous: row guards; 1-D: guard elements on either side)."""
    if len(shape) == 2:
        return Guarded(shape[0], shape[1], dtype, be.dev, pad_cols=(0, 0), pad_rows=8)
    return guarded_like(torch.empty(shape, dtype=dtype), be.dev, pad_rows=8)


def _dev(be, t):
    return t.to(be.dev)


# ---- the runners: one kernel (pair), one case -----------------------------------------------------------------------------------------
def run_ce(be, c, rep, smooth):
    """st_ce_fwd / st_ce_bwd (smooth False) or st_ce_smooth_fwd / _bwd (smooth: 'smoothed' with a denominator, or 'plain' = (1, 0, -1))."""
    R, V = c.R, c.V
    kernel = "st_ce" if not smooth else "st_ce_smooth[%s]" % smooth
    conf, sm, zc = smooth_cfg(V) if smooth == "smoothed" else PLAIN
    lg, tgt = logits_buffer(be, c.x), _dev(be, c.target)
    vp = (V + 8) // 8 * 8
    g_lse, g_sums, g_dl = out_like(be, (R,), F32), out_like(be, (4 if smooth else 3,), F32), out_like(be, (R, vp), BF16)
    go = _dev(be, torch.tensor([32.0]))
    n = float(c.valid.sum())
    denom = _dev(be, torch.tensor([12.0])) if smooth == "smoothed" else None
    D = 12.0 if denom is not None else n
    if not smooth:
        be.ce_fwd(lg, tgt, IGNORE, g_lse.view, g_sums.view, V=V)
        be.ce_bwd(lg, tgt, IGNORE, g_lse.view, g_sums.view, go, g_dl.view, V=V)
    else:
        be.ce_smooth_fwd(lg, tgt, IGNORE, conf, sm, zc, g_lse.view, g_sums.view, V=V, denom=denom)
        be.ce_smooth_bwd(lg, tgt, IGNORE, conf, sm, zc, g_lse.view, g_sums.view, go, g_dl.view, V=V, denom=denom)
    for gd, nm in ((g_lse, "lse"), (g_sums, "sums"), (g_dl, "dlogits")):
        gd.assert_intact("%s %s V=%d %s" % (kernel, c.family, V, nm))
    check_lse(rep, kernel, c, g_lse.view)
    # ---- sums: the number of rows times the per-row bound (+ 4 ulp32(max |x|) for the smoothed four-term sum on offset rows)
    vz = c.valid.to(F64)
    loss = torch.where(c.valid, ref.row_loss(c.x, c.tclamp, conf, sm, zc), torch.zeros(R, dtype=F64))
    nll = torch.where(c.valid, ref.nll(c.x, c.tclamp), torch.zeros(R, dtype=F64))
    extra = 4 * ref.ulp32(c.max_abs) if (smooth == "smoothed" and c.family == "offset") else torch.zeros(R, dtype=F64)
    per_row = lambda v: float((logp_bound(c.lse, torch.where(torch.isinf(v), torch.zeros_like(v), v)) + extra)[c.valid].max())
    sums = g_sums.view.detach().cpu()
    exact(rep, kernel, c, "sums[1]", sums[1:2].to(F64) == n, "the number of counted rows")
    within(rep, kernel, c, "sums[0]", sums[0:1], loss.sum().view(1), n * per_row(loss))
    within(rep, kernel, c, "sums[2]", sums[2:3], (loss.sum() / D).view(1), n * per_row(loss) / D + ref.ulp32(loss.sum() / D))
    if smooth:
        within(rep, kernel, c, "sums[3]", sums[3:4], (nll.sum() / n).view(1), per_row(nll) + ref.ulp32(nll.sum() / n))
    # ---- the gradient: whole tensor and per row / column as before, then element by element in probability units
    scale = 32.0 / D
    want = ref.grad_ce(c.x, c.tclamp, conf, sm, zc) * vz.view(-1, 1)
    got = g_dl.view.detach().cpu()
    check(got[:, :V], want * scale, 6e-3, "%s %s V=%d dlogits" % (kernel, c.family, V), tol_local=L_CE)
    q_sum = ref.smoothed_target(R, V, c.tclamp, conf, sm, zc).sum(-1, keepdim=True)
    check_grad(rep, kernel, c, "dlogits", got[:, :V].to(F64) / scale, want, c.p * q_sum * vz.view(-1, 1))
    exact(rep, kernel, c, "dlogits pad", got[:, V:].view(torch.int16) == 0, "columns >= V must be bit-zero")
    m = c.masked & c.valid.view(-1, 1)
    if bool(m.any()):
        q = ref.smoothed_target(R, V, c.tclamp, conf, sm, zc)
        s32 = torch.tensor(32.0, dtype=F32) / torch.tensor(D, dtype=F32)
        expect = ((torch.zeros(R, V, dtype=F32) - q.to(F32)) * s32).to(BF16)      # (Q * 0 - q) * scale, in fp32, one bf16 rounding
        exact(rep, kernel, c, "dlogits masked", got[:, :V][m] == expect[m], "a masked column's gradient is exactly bf16(-q * scale)")


def run_eval(be, c, rep, smooth):
    """st_ce_eval_fwd at the plain (1, 0, -1) or the smoothed target: the numerator, NLL, arg-max flag and state columns."""
    R, V = c.R, c.V
    kernel = "st_ce_eval[%s]" % smooth
    conf, sm, zc = smooth_cfg(V) if smooth == "smoothed" else PLAIN
    g_rows = out_like(be, (R, 4), F32)
    be.ce_eval_fwd(logits_buffer(be, c.x), _dev(be, c.target), IGNORE, conf, sm, zc, g_rows.view, V=V)
    g_rows.assert_intact("%s %s V=%d rows" % (kernel, c.family, V))
    got = g_rows.view.detach().cpu()
    zero = torch.zeros(R, dtype=F64)
    loss = torch.where(c.valid, ref.row_loss(c.x, c.tclamp, conf, sm, zc), zero)
    nll = torch.where(c.valid, ref.nll(c.x, c.tclamp), zero)
    extra = 4 * ref.ulp32(c.max_abs) if (smooth == "smoothed" and c.family == "offset") else zero
    within(rep, kernel, c, "row_loss", got[:, 0], loss, logp_bound(c.lse, loss) + extra)
    within(rep, kernel, c, "row_nll", got[:, 1], nll, logp_bound(c.lse, nll))
    first = ref.best(c.x64, 1)[0][:, 0]
    exact(rep, kernel, c, "row_hit", got[:, 2].to(F64) == ((first == c.target) & c.valid).to(F64), "the arg-max flag (lowest column among equal maxima)")
    exact(rep, kernel, c, "state", got[:, 3].to(F64) == c.valid.to(F64), "the row state")


def run_ctc(be, c, rep, aligned):
    """st_ctc_gather / st_ctc_dlogits over two utterances (the second shorter), 16-byte loads (aligned) or scalar loads."""
    R, V = c.R, c.V
    kernel = "st_ctc_gather[%s]" % ("16-byte" if aligned else "scalar")
    lens = [R - R // 3, R // 3]
    B, T, C = 2, lens[0], 4
    rowmap = torch.cat([torch.arange(lens[0]), T + torch.arange(lens[1])]).to(I64)
    bof = torch.cat([torch.zeros(lens[0], dtype=I64), torch.ones(lens[1], dtype=I64)])
    cols = torch.tensor([[0, min(1, V - 1), V - 1, V // 2], [0, min(1, V - 1), max(V - 2, 0), V - 1]], dtype=I32)
    scat = torch.full((B, C), -1, dtype=I32)
    scat[:, 1] = cols[:, 1]                               # one label column per utterance is overwritten by the small gradient
    gen = torch.Generator().manual_seed(c.seed + 1)
    gsmall = torch.randn(B, T, C, generator=gen) * 0.05
    roww, go = torch.tensor([1.0, 2.0]), torch.tensor([2.0])
    lg = logits_buffer(be, c.x, ld_mod4=aligned)
    vp = (V + 8) // 8 * 8
    g_lse, g_lp, g_dl = out_like(be, (R,), F32), out_like(be, (B, T, C), F32), out_like(be, (R, vp), BF16)
    be.ctc_gather(lg, _dev(be, rowmap), T, _dev(be, cols), g_lse.view, g_lp.view, V=V)
    be.ctc_dlogits(lg, g_lse.view, _dev(be, rowmap), T, _dev(be, roww), _dev(be, scat), _dev(be, gsmall), _dev(be, go), g_dl.view, V=V)
    for gd, nm in ((g_lse, "lse"), (g_lp, "lp"), (g_dl, "dlogits")):
        gd.assert_intact("%s %s V=%d %s" % (kernel, c.family, V, nm))
    check_lse(rep, kernel, c, g_lse.view)
    lp = g_lp.view.detach().cpu().view(B * T, C)
    want = c.lp.gather(1, cols[bof].to(I64))
    within(rep, kernel, c, "lp", lp[rowmap], want, logp_bound(c.lse.view(-1, 1), want))
    absent = torch.ones(B * T, dtype=torch.bool)
    absent[rowmap] = False
    exact(rep, kernel, c, "lp absent", torch.isnan(lp[absent]), "frames past an utterance's length are left untouched")
    got = g_dl.view.detach().cpu()
    w = (roww[bof] * go).to(F64).view(-1, 1)
    dense = torch.ones(R, V, dtype=torch.bool)
    dense[torch.arange(R), scat[bof, 1].to(I64)] = False
    want_g = torch.where(dense, c.p, torch.zeros_like(c.p))
    got_d = torch.where(dense, got[:, :V].to(F64), torch.zeros_like(c.p))
    check(got_d, want_g * w, 1e-2, "%s %s V=%d dlogits" % (kernel, c.family, V), tol_local=L_BF16)
    check_grad(rep, kernel, c, "dlogits", got_d / w, want_g, want_g)
    exact(rep, kernel, c, "dlogits pad", got[:, V:].view(torch.int16) == 0, "columns >= V must be bit-zero")
    exact(rep, kernel, c, "dlogits label", got[torch.arange(R), scat[bof, 1].to(I64)] == (gsmall.view(B * T, C)[rowmap, 1] * go).to(BF16),
          "the label column holds bf16(gsmall * grad_out)")
    if bool(c.masked.any()):
        exact(rep, kernel, c, "dlogits masked", got[:, :V][c.masked & dense] == 0, "a masked column's probability is exactly 0")


def run_vocab_lp(be, c, rep, ragged):
    """st_ctc_vocab_lp over all rows as two utterances of equal length, or (ragged) over all but the first row: a row count that is
    no multiple of 4 (the kernel takes four rows per workgroup), the second utterance shorter."""
    rows = torch.arange(1 if ragged else 0, c.R)
    n, V, T_cap = rows.numel(), c.V, 64
    kernel = "st_ctc_vocab_lp[ragged]" if ragged else "st_ctc_vocab_lp"
    lens = [n - n // 3, n // 3] if ragged else [n // 2, n // 2]
    off, length = torch.tensor([0, lens[0]], dtype=I32), torch.tensor(lens, dtype=I32)
    g_lse, g_lpT = out_like(be, (n,), F32), out_like(be, (2, V, T_cap), F32)
    be.ctc_vocab_lp(logits_buffer(be, c.x[rows]), V, _dev(be, off), _dev(be, length), T_cap, g_lse.view, g_lpT.view)
    g_lse.assert_intact("%s lse" % kernel), g_lpT.assert_intact("%s lpT" % kernel)
    check_lse(rep, kernel, c, g_lse.view, rows=rows)
    got = g_lpT.view.detach().cpu()
    for b in range(2):
        o, m = int(off[b]), lens[b]
        want = c.lp[rows][o:o + m].t()
        within(rep, kernel, c, "lpT", got[b, :, :m], want, logp_bound(c.lse[rows][o:o + m].view(1, -1), want))
        exact(rep, kernel, c, "lpT tail", got[b, :, m:].view(torch.int32) == 0, "frames past a length are zero")


def run_beam(be, c, rep, wide):
    """st_beam_advance (wide: with `work`) over R / BEAM utterances: the new scores, the trellis row, tokens and order."""
    V, B = c.V, c.R // BEAM
    kernel = "st_beam_advance[%s]" % ("work" if wide else "NULL")
    scores0, table, bound = beam_tables(c)
    S, t = 2, 1
    g_sc, g_tok, g_len, g_ord = (out_like(be, (B, BEAM), F32), out_like(be, (B * BEAM,), I64), out_like(be, (B,), I64),
                                 out_like(be, (B * BEAM,), I64))
    g_hs, g_back, g_toks = out_like(be, (S, B, BEAM), F32), out_like(be, (S, B, BEAM), I64), out_like(be, (S, B, BEAM), I64)
    g_sc.view.copy_(scores0)
    g_tok.view.fill_(1)
    g_len.view.fill_(3)
    done = torch.zeros(B, dtype=torch.bool, device=be.dev)
    step = _dev(be, torch.tensor([t], dtype=I64))
    work = torch.zeros(be.beam_work_words(B, BEAM), dtype=I64, device=be.dev) if wide else None
    be.beam_advance(logits_buffer(be, c.x), V, BEAM, step, V + 9, g_sc.view, g_tok.view, done, g_len.view, g_hs.view, g_back.view,
                    g_toks.view, g_ord.view, work=work)
    for gd, nm in ((g_sc, "scores"), (g_tok, "tokens"), (g_len, "lengths"), (g_ord, "order"), (g_hs, "hist_scores"), (g_back, "back"),
                   (g_toks, "toks")):
        gd.assert_intact("%s %s V=%d %s" % (kernel, c.family, V, nm))
    back, toks = g_back.view.detach().cpu(), g_toks.view.detach().cpu()
    exact(rep, kernel, c, "range", (back[t] >= 0) & (back[t] < BEAM) & (toks[t] >= 0) & (toks[t] < V), "back-pointers and tokens in range")
    flat = back[t] * V + toks[t]
    idx, v = check_choice(rep, kernel, c, flat, table, bound, BEAM)
    got_v = table.gather(1, flat)
    within(rep, kernel, c, "scores", g_sc.view, got_v, bound.gather(1, flat))
    exact(rep, kernel, c, "hist_scores", g_hs.view.detach().cpu()[t] == scores0, "the trellis row holds the old scores")
    exact(rep, kernel, c, "trellis row 0", torch.isnan(g_hs.view.detach().cpu()[0]), "only row *step of the trellis is written")
    exact(rep, kernel, c, "tokens", g_tok.view.detach().cpu().view(B, BEAM) == toks[t], "tokens are the trellis row's tokens")
    exact(rep, kernel, c, "order", g_ord.view.detach().cpu().view(B, BEAM) == back[t] + BEAM * torch.arange(B).view(B, 1), "order = origin + b * beam")
    exact(rep, kernel, c, "lengths", g_len.view.detach().cpu() == 4, "every live utterance grows by one")
    if c.family == "uniform":
        exact(rep, kernel, c, "uniform ids", flat == torch.arange(BEAM).view(1, BEAM), "the first `beam` flat indices of the best-scoring row")
    if c.family == "one-hot":
        exact(rep, kernel, c, "one-hot first", flat[:, 0] == torch.tensor(c.onehot)[::BEAM], "the first candidate is j of the best-scoring row")


def run_pre_beam(be, c, rep):
    """st_beam_pre_beam: the K best of every row's log-softmax."""
    R, V, K = c.R, c.V, pre_beam_k(c.V)
    kernel = "st_beam_pre_beam"
    g_ids, g_lp = out_like(be, (R, K), I32), out_like(be, (R, K), F32)
    be.beam_pre_beam(logits_buffer(be, c.x), V, g_ids.view, g_lp.view)
    g_ids.assert_intact("%s ids" % kernel), g_lp.assert_intact("%s lp" % kernel)
    bound = logp_bound(c.lse.view(-1, 1), c.lp)
    ids = g_ids.view.detach().cpu().to(I64)
    check_choice(rep, kernel, c, ids, c.lp, bound, K)
    within(rep, kernel, c, "lp", g_lp.view, c.lp.gather(1, ids), bound.gather(1, ids))
    if c.family == "uniform":
        exact(rep, kernel, c, "uniform ids", ids == torch.arange(K).view(1, K), "all candidates tie: ids 0 .. K - 1")
    if c.family == "one-hot":
        exact(rep, kernel, c, "one-hot first", ids[:, 0] == torch.tensor(c.onehot), "the first candidate is j")


def run_best_path(be, c, rep):
    """st_ctc_best_path: the arg-max of every row (lower id on ties)."""
    g_out = out_like(be, (c.R,), I32)
    be.ctc_best_path(logits_buffer(be, c.x), c.V, g_out.view)
    g_out.assert_intact("st_ctc_best_path out")
    exact(rep, "st_ctc_best_path", c, "arg-max", g_out.view.detach().cpu().to(I64) == ref.best(c.x64, 1)[0][:, 0], "the row arg-max")


# kernel id -> (runner, keyword arguments, the families it runs, the smallest V)
RUNNERS = {
    "ce": (run_ce, dict(smooth=None), FAMILIES, 2),
    "ce_smooth": (run_ce, dict(smooth="smoothed"), FAMILIES[:-1], 2),
    "ce_smooth_plain": (run_ce, dict(smooth="plain"), FAMILIES[:-1], 2),
    "ce_eval": (run_eval, dict(smooth="smoothed"), FAMILIES[:-1], 2),
    "ce_eval_plain": (run_eval, dict(smooth="plain"), FAMILIES[:-1], 2),
    "ctc_gather_16byte": (run_ctc, dict(aligned=True), FAMILIES, 2),
    "ctc_gather_scalar": (run_ctc, dict(aligned=False), FAMILIES, 2),
    "ctc_vocab_lp": (run_vocab_lp, dict(ragged=False), FAMILIES[:-1], 2),
    "ctc_vocab_lp_ragged": (run_vocab_lp, dict(ragged=True), FAMILIES[:-1], 2),
    "beam_advance": (run_beam, dict(wide=False), FAMILIES[:-1], BEAM + 1),
    "beam_advance_work": (run_beam, dict(wide=True), FAMILIES[:-1], BEAM + 1),
    "beam_pre_beam": (run_pre_beam, {}, FAMILIES[:-1], 2),
    "ctc_best_path": (run_best_path, {}, ("one-hot", "masked"), 2),
}


def cases():
    return [("%s-%s" % (k, f), (k, f)) for k, (_, _, fams, _) in RUNNERS.items() for f in fams]


def run(kernel, family, be, rep=None, vs=None):
    fn, kw, _, v_min = RUNNERS[kernel]
    for V in (vs or family_vs(family)):
        if V >= v_min:
            fn(be, build(family, V), rep, **kw)


# ---- fp32 restatements of the sum (tools/local_bounds.py measures L_LSE and P_REL from these; tests/test_lse_fp64_cpu.py injects
#      the defects) ---------------------------------------------------------------------------------------------------------------------
_F = np.float32
_LOG2E, _LN2 = _F(1.4426950408889634), _F(0.6931471805599453)


def expf32(d):
    """__expf as the kernels get it: exp2(fp32(d x log2 e)), in fp32."""
    with np.errstate(all="ignore"):
        return np.exp2((np.asarray(d, dtype=_F) * _LOG2E).astype(_F)).astype(_F)


def logf32(s):
    with np.errstate(all="ignore"):
        return (np.log2(np.asarray(s, dtype=_F)).astype(_F) * _LN2).astype(_F)


def lse32_batched(x, V=None, threads=256, per=8, defect=None):
    """The kernels' order: `threads` threads take `per` columns each per pass with a running (max, sum) rescaled by exp(mx - mn)
    (guarded: a pass whose maximum is still -inf adds nothing), then a tree merge to the row maximum.  x: f32 [R, >= V].
    defect: None, 'drop_last' (column V - 1 not read), 'double_2048' (column 2,048 read twice), 'read_V' (column V read),
    'no_max' (no maximum subtracted), 'no_rescale' (the running maximum updated without rescaling the sum)."""
    x = np.asarray(x, dtype=_F)
    V = x.shape[1] if V is None else V
    R = x.shape[0]
    n = V + 1 if defect == "read_V" else V - 1 if defect == "drop_last" else V
    row = x[:, :n]
    if defect == "double_2048" and V > 2048:
        row = np.concatenate([row, x[:, 2048:2049]], 1)
    width = threads * per
    passes = -(-row.shape[1] // width)
    pad = np.full((R, passes * width), -np.inf, dtype=_F)
    pad[:, :row.shape[1]] = row
    blk = pad.reshape(R, passes, per, threads)
    mx, sm = np.full((R, threads), -np.inf, dtype=_F), np.zeros((R, threads), dtype=_F)
    with np.errstate(all="ignore"):
        for p in range(passes):
            xb = blk[:, p]
            mn = np.fmax(mx, np.fmax.reduce(xb, axis=1))          # (fmaxf: a NaN operand is ignored by the maximum, not by the sum)
            if defect == "no_max":
                mn = np.zeros_like(mn)
            live = mn > -np.inf
            base = np.where(live, mn, _F(0))
            bs = np.zeros((R, threads), dtype=_F)
            for u in range(per):
                bs = (bs + expf32(xb[:, u] - base)).astype(_F)
            scale = np.ones_like(sm) if defect == "no_rescale" else expf32(np.where(live, mx - base, _F(0)))
            sm = np.where(live, (sm * scale).astype(_F) + bs, sm).astype(_F)
            mx = np.where(live, mn, mx)
        gm = mx.max(1, keepdims=True)
        s = np.where(mx > -np.inf, (sm * expf32(mx - gm)).astype(_F), _F(0)).astype(_F)
        while s.shape[1] > 1:
            s = (s[:, 0::2] + s[:, 1::2]).astype(_F)
        return (gm[:, 0] + logf32(s[:, 0])).astype(_F)


def lse32_serial(x, V=None):
    """A plain serial max-then-sum in fp32."""
    x = np.asarray(x, dtype=_F)
    row = x[:, :x.shape[1] if V is None else V]
    m = row.max(1, keepdims=True)
    s = np.cumsum(expf32(row - m), axis=1, dtype=_F)[:, -1]
    return (m[:, 0] + logf32(s)).astype(_F)


def lse32_gather_today(x, V=None, guarded=False):
    """st_ctc_gather's element-by-element update as it stood before the guard (scalar path: thread tid takes columns tid, tid + 256,
    ...): `if (x > mx) { sum = sum * exp(mx - x) + 1; mx = x; } else sum += exp(x - mx);`.  guarded: with `else if (mx > -inf)`."""
    x = np.asarray(x, dtype=_F)
    V = x.shape[1] if V is None else V
    R, threads = x.shape[0], 256
    n = -(-V // threads)
    pad = np.full((R, n * threads), np.nan, dtype=_F)
    pad[:, :V] = x[:, :V]
    blk = pad.reshape(R, n, threads)
    have = (np.arange(n * threads) < V).reshape(n, threads)
    mx, sm = np.full((R, threads), -np.inf, dtype=_F), np.zeros((R, threads), dtype=_F)
    with np.errstate(all="ignore"):
        for i in range(n):
            v = blk[:, i]
            up = v > mx
            s_up = ((sm * expf32(mx - v)).astype(_F) + _F(1)).astype(_F)
            s_else = (sm + expf32(v - mx)).astype(_F)
            if guarded:
                s_else = np.where(mx > -np.inf, s_else, sm)
            new_s, new_m = np.where(up, s_up, s_else), np.where(up, v, mx)
            sm, mx = np.where(have[i], new_s, sm).astype(_F), np.where(have[i], new_m, mx).astype(_F)
        gm = mx.max(1, keepdims=True)
        s = np.where(mx == -np.inf, _F(0), (sm * expf32(mx - gm)).astype(_F)).astype(_F)
        while s.shape[1] > 1:
            s = (s[:, 0::2] + s[:, 1::2]).astype(_F)
        return (gm[:, 0] + logf32(s[:, 0])).astype(_F)


def measure_bounds():
    """-> (L_LSE, P_REL, rows): both bounds as tests/LOCAL_BOUNDS.md defines them, and per (order, family) the worst figures."""
    rows, worst_l, worst_p = [], 0.0, 0.0
    for name, fn in (("batched", lse32_batched), ("serial", lse32_serial)):
        for family in FAMILIES:
            wl = wp = 0.0
            for V in family_vs(family):
                c = build(family, V)
                l32 = fn(c.x.numpy())
                err = (torch.from_numpy(l32).to(F64) - c.lse).abs() - ref.ulp32(c.lse) / 2
                wl = max(wl, float(err.clamp_min(0).max()))
                p32 = torch.from_numpy(expf32(c.x.numpy() - l32[:, None])).to(F64)
                big = c.p >= 2.0 ** -100
                wp = max(wp, float(((p32 - c.p).abs() / c.p.clamp_min(1e-300))[big].max()))
            rows.append((name, family, wl, wp))
            worst_l, worst_p = max(worst_l, wl), max(worst_p, wp)
    return 3 * worst_l, 3 * worst_p, rows
