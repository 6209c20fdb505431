"""fp64 restatement of st_ctc_beam_search (csrc/st_ctc_beam.hip) keyed by label TUPLES, and the frame-local check of its trace.

The beam of an utterance is a list of entries (labels, pb, pnb) in slot order.  A frame's candidates are accumulated in a
dictionary keyed by the label tuple, so contributions to one label sequence merge by construction, whichever parent they came
through.  Candidate rule, tie rule and L_cap rule are the kernel's (include/st_hip.h): stay candidates are numbered by slot,
extensions ``beam + slot * K + j``; log-sums into one target are formed in candidate order; the ``beam`` best totals are kept,
the lower number first on ties, a total of -inf never; a prefix of L_cap labels is not extended.  Values are kept relative to the
frame's best total, the normaliser apart, as the kernel does (in fp64 that changes nothing).

Besides the n-best, ``search`` reports, from the reference alone: the SELECTION MARGIN (the smallest gap over all frames between
the last kept and the first dropped candidate), the number of RE-CREATION MERGES (an extension that lands on a beam entry whose
recorded parent is not the extending entry - the event a (parent, token) identity misses), and the bound accumulated over T.

THE PER-FRAME BOUND (derived from the kernel's operation count, eps = 2^-24 the unit roundoff of fp32).  Given the fp32 (pb, pnb)
of the frame before - taken as exact: they are the kernel's own numbers - a new value takes
  total(p) = m + log(1 + exp(n - m)) on the hardware's exp2 / log2 (1 ulp each), x = n - m <= 0, e = exp(x) <= 1:  the subtract
      moves the result by <= 0.28 eps (|x| e / (1 + e) <= 0.28); the scaling x log2(e) by <= 0.37 eps (|x| e <= 1 / e, weight
      1 / (1 + e) <= 1); exp2 (1 ulp: relative 2 eps on e, weight e / (1 + e) <= 1/2) by <= eps; the sum 1 + e in [1, 2]
      (half an ulp = eps, weight <= 1) by <= eps; log2 (1 ulp: relative 2 eps of a result <= ln 2) and its scaling by ln 2 (eps of
      the same) by <= 2.1 eps; 4.75 eps in all; the final add by eps |total|:      LA(v) = (5 + |v|) eps for every log-sum;
  + x_t(c): one add, eps |term|;
  for a stay entry that an extension merges into: one more log-sum of two terms, LA(v) on top of the larger error of its terms
      (a log-sum is a convex combination of its operands' errors);
  - m0, the frame's best total: one subtract, eps |v_rel|, and m0's own error: the best candidate's value error plus the LA of
      its total.
With M the largest magnitude among the numbers involved (the operands, the emission, the unnormalised results, m0):
  value: (5 + M) + M + (5 + M) = (10 + 3 M) eps;  m0: (10 + 3 M) + (5 + M) eps;  subtract: M eps  ->  bound = (25 + 8 M) eps.
A total used for selection is the log-sum of (pb', pnb'): a convex combination plus one LA - inside 2 x bound for a comparison
of two candidates.  The bound accumulated over an utterance is the sum over its frames of the frame's largest bound; an exact
comparison of hypotheses is only meaningful where the reference's selection margin is at least 100 times that
(``margin_ok``)."""
import math

import numpy as np

EPS = 2.0 ** -24
NINF = float("-inf")


def logadd(a, b):
    m, n = (a, b) if a >= b else (b, a)
    if n == NINF:
        return m
    return m + math.log1p(math.exp(n - m))


def bound_of(mag):
    return (25.0 + 8.0 * mag) * EPS


def _mag(*xs):
    return max([1.0] + [abs(x) for x in xs if x != NINF and not math.isnan(x)])


class Cand(object):
    """One target of a frame: its label tuple, (pb, pnb), the lowest candidate number that feeds it, the slot and token it was
    made from (token -1: the slot's own prefix), the largest magnitude that went into it, the numbers that fed it."""

    __slots__ = ("labels", "pb", "pnb", "number", "slot", "token", "mag", "feeds")

    def __init__(self, labels, number, slot, token):
        self.labels, self.number, self.slot, self.token = labels, number, slot, token
        self.pb, self.pnb, self.mag, self.feeds = NINF, NINF, 1.0, []

    @property
    def total(self):
        return logadd(self.pb, self.pnb)


def frame_candidates(entries, ids_t, lp_t, lpb_t, blank, beam, L_cap):
    """entries: [(labels, pb, pnb)] in slot order; ids_t / lp_t: the row's K classes -> {labels: Cand}, in candidate order."""
    K = len(ids_t)
    out = {}
    classes = [(j, int(ids_t[j])) for j in range(K) if int(ids_t[j]) != blank]
    for s, (labels, pb, pnb) in enumerate(entries):                    # stay candidates: numbers 0 .. beam - 1
        tot = logadd(pb, pnb)
        c = out[labels] = Cand(labels, s, s, -1)
        c.pb = tot + lpb_t
        c.mag = _mag(pb, pnb, tot, lpb_t, c.pb)
        c.feeds.append(s)
        for j, k in classes:
            if labels and k == labels[-1]:
                c.pnb = pnb + float(lp_t[j])
                c.mag = _mag(c.mag, lp_t[j], c.pnb)
                break
    for s, (labels, pb, pnb) in enumerate(entries):                    # extensions: numbers beam + s K + j
        if len(labels) >= L_cap:
            continue
        tot = logadd(pb, pnb)
        for j, k in classes:
            base = pb if (labels and k == labels[-1]) else tot
            term = base + float(lp_t[j])
            key = labels + (k,)
            number = beam + s * K + j
            c = out.get(key)
            if c is None:
                c = out[key] = Cand(key, number, s, k)
            c.pnb = logadd(c.pnb, term)
            c.mag = _mag(c.mag, pb, pnb, tot, lp_t[j], term, c.pnb)
            c.feeds.append(number)
    return out


def select(cands, beam):
    """-> (kept, dropped): the finite candidates sorted by (total descending, number ascending), split at ``beam``."""
    live = sorted((c for c in cands.values() if c.total > NINF), key=lambda c: (-c.total, c.number))
    return live[:beam], live[beam:]


class Result(object):
    """hyps: [(labels, score)] best first; trace: per frame [(prev_slot, token, pb_rel, pnb_rel)] of the live slots; norms: the
    normaliser after every frame; margin; recreations; bound (accumulated over the frames)."""

    __slots__ = ("hyps", "trace", "norms", "margin", "recreations", "bound")


def search(ids, lp, lpb, blank, beam, L_cap):
    """ids i32 [T, K], lp [T, K], lpb [T] of ONE utterance (the kernel's inputs, any float type) -> Result."""
    T = len(lpb)
    entries, eids, pars = [((), 0.0, NINF)], [0], [-1]
    next_eid, norm = 1, 0.0
    res = Result()
    res.trace, res.norms, res.margin, res.recreations, res.bound = [], [], float("inf"), 0, 0.0
    for t in range(T):
        cands = frame_candidates(entries, ids[t], [float(x) for x in lp[t]], float(lpb[t]), blank, beam, L_cap)
        K = len(ids[t])
        for c in cands.values():                  # an extension that lands on a beam entry it is not the recorded parent of
            if c.token < 0:
                for number in c.feeds[1:]:
                    if pars[c.slot] != eids[(number - beam) // K]:
                        res.recreations += 1
        kept, dropped = select(cands, beam)
        if not kept:
            entries, eids, pars = [], [], []
            res.trace.append([])
            res.norms.append(norm)
            continue
        if dropped:
            res.margin = min(res.margin, kept[-1].total - dropped[0].total)
        best = kept[0].total
        res.bound += max(bound_of(_mag(c.mag, best)) for c in kept)
        norm += best
        new_e, new_i, new_p, rec = [], [], [], []
        for c in kept:
            new_e.append((c.labels, c.pb - best, c.pnb - best))
            rec.append((c.slot, c.token, c.pb - best, c.pnb - best))
            if c.token < 0:
                new_i.append(eids[c.slot])
                new_p.append(pars[c.slot])
            else:
                new_i.append(next_eid)
                new_p.append(eids[c.slot])
                next_eid += 1
        entries, eids, pars = new_e, new_i, new_p
        res.trace.append(rec)
        res.norms.append(norm)
    res.hyps = [(labels, norm + logadd(pb, pnb)) for labels, pb, pnb in entries]
    return res


def margin_ok(res):
    """The rule for exact comparisons: the selection margin is at least 100 times the accumulated bound."""
    return res.margin >= 100.0 * res.bound


def ctc_likelihood(lp_full, labels, blank):
    """fp64 CTC forward log-likelihood of ``labels`` under lp_full [T, V] (the textbook alpha recursion)."""
    T = len(lp_full)
    ext = [blank]
    for k in labels:
        ext += [k, blank]
    S = len(ext)
    if T == 0:
        return 0.0 if not labels else NINF
    a = [NINF] * S
    a[0] = float(lp_full[0][blank])
    if S > 1:
        a[1] = float(lp_full[0][ext[1]])
    for t in range(1, T):
        n = [NINF] * S
        for s in range(S):
            v = a[s]
            if s > 0:
                v = logadd(v, a[s - 1])
            if s > 1 and ext[s] != blank and ext[s] != ext[s - 2]:
                v = logadd(v, a[s - 2])
            n[s] = v + float(lp_full[t][ext[s]]) if v > NINF else NINF
        a = n
    return logadd(a[S - 1], a[S - 2]) if S > 1 else a[0]


def check_trace(ids, lp, lpb, blank, beam, L_cap, trace, norms, score, tokens=None, lens=None):
    """The frame-local check of ONE utterance.  trace: [T][beam] records (prev_slot, token, pb_rel, pnb_rel) of the beam after
    every frame (a dead slot: prev_slot < 0); norms [T]; score [beam] (and optionally tokens [beam][L_cap], lens [beam]) as the
    kernel returned them.  Raises AssertionError naming frame and slot; returns (the largest ratio error / bound it saw, the bound
    accumulated over the frames: what the normaliser - and with it a score - can be off by)."""
    T = len(lpb)
    entries = [((), 0.0, NINF)]
    norm_prev, worst, acc = 0.0, 0.0, 0.0
    for t in range(T):
        cands = frame_candidates(entries, ids[t], [float(x) for x in lp[t]], float(lpb[t]), blank, beam, L_cap)
        kept_ref, _ = select(cands, len(cands))
        n_fin = len(kept_ref)
        recs = [(int(r[0]), int(r[1]), float(r[2]), float(r[3])) for r in trace[t]]
        live = [r for r in recs if r[0] >= 0]
        assert all(r[0] >= 0 for r in recs[:len(live)]), "frame %d: a dead slot stands before a live one" % t
        assert len(live) == min(beam, n_fin), "frame %d: %d entries kept, %d finite candidates, beam %d" % (t, len(live), n_fin, beam)
        if not live:
            assert float(norms[t]) == norm_prev, "frame %d: the normaliser moved without a live entry" % t
            entries = []
            continue
        best = kept_ref[0].total
        m0 = float(norms[t]) - norm_prev
        new_entries, seen, kept_tot, frame_bound = [], set(), [], 0.0
        for slot, (prev, token, pb, pnb) in enumerate(live):
            assert prev < len(entries), "frame %d slot %d: parent slot %d is not live" % (t, slot, prev)
            labels = entries[prev][0] + ((token,) if token >= 0 else ())
            assert labels in cands, "frame %d slot %d: %r is no candidate of this frame" % (t, slot, labels)
            assert labels not in seen, "frame %d slot %d: the label sequence %r appears twice" % (t, slot, labels)
            seen.add(labels)
            c = cands[labels]
            bound = bound_of(_mag(c.mag, best))
            frame_bound = max(frame_bound, bound)
            for name, got, want in (("pb", pb, c.pb - best), ("pnb", pnb, c.pnb - best)):
                if want == NINF or got == NINF:
                    assert got == want, "frame %d slot %d: %s is %r, fp64 %r" % (t, slot, name, got, want)
                    continue
                err = abs(got - want)
                worst = max(worst, err / bound)
                assert err <= bound, "frame %d slot %d %r: %s_rel %.9g, fp64 %.9g, error %.3e > bound %.3e" % (
                    t, slot, labels, name, got, want, err, bound)
            kept_tot.append(c.total)
            new_entries.append((labels, pb, pnb))
        assert abs(m0 - best) <= frame_bound + 1e-12 * abs(float(norms[t])), \
            "frame %d: the normaliser moved by %.9g, the fp64 best total is %.9g (bound %.3e)" % (t, m0, best, frame_bound)
        dropped = [c.total for c in kept_ref if c.labels not in seen]
        if dropped:
            assert max(dropped) - min(kept_tot) <= 2.0 * frame_bound, \
                "frame %d: a dropped candidate beats a kept one by %.3e > 2 x bound %.3e" % (t, max(dropped) - min(kept_tot), frame_bound)
        for a, b in zip(kept_tot, kept_tot[1:]):
            assert b - a <= 2.0 * frame_bound, "frame %d: the kept entries are not best first (%.9g before %.9g)" % (t, a, b)
        entries, norm_prev = new_entries, float(norms[t])
        acc += frame_bound
    # the normalisers telescope to the returned scores; the returned labels are the trace's
    for slot in range(beam):
        got = float(score[slot])
        if slot >= len(entries):
            assert got == NINF, "slot %d: score %r of a dead slot" % (slot, got)
            if lens is not None:
                assert int(lens[slot]) == 0 and all(int(k) == -1 for k in tokens[slot]), "slot %d: labels in a dead slot" % slot
            continue
        labels, pb, pnb = entries[slot]
        want = norm_prev + logadd(pb, pnb)
        tol = 2.0 * EPS * max(1.0, abs(want)) + (5.0 + abs(logadd(pb, pnb))) * EPS
        assert abs(got - want) <= tol, "slot %d: score %.9g, normaliser + relative total %.9g (tolerance %.3e)" % (slot, got, want, tol)
        if lens is not None:
            n = int(lens[slot])
            assert tuple(int(k) for k in tokens[slot][:n]) == labels and all(int(k) == -1 for k in tokens[slot][n:]), \
                "slot %d: tokens %r, the trace spells %r" % (slot, list(tokens[slot]), labels)
    return worst, acc


def trace_arrays(res, beam):
    """The reference's own trace in the kernel's layout: records [T][beam] (dead: (-1, -1, -inf, -inf)), norms, score [beam]."""
    recs = [list(fr) + [(-1, -1, NINF, NINF)] * (beam - len(fr)) for fr in res.trace]
    score = [s for _, s in res.hyps] + [NINF] * (beam - len(res.hyps))
    return recs, list(res.norms), score


def inputs_of(lp_full, K, blank):
    """The kernel's inputs from full log-probabilities [T, V]: the K best classes of every row, best first, lower id on ties
    (st_beam_pre_beam's order) -> (ids i32 [T, K], lp f32 [T, K], lpb f32 [T])."""
    lp_full = np.asarray(lp_full, dtype=np.float32)
    T, V = lp_full.shape
    order = np.lexsort((np.broadcast_to(np.arange(V), (T, V)), -lp_full.astype(np.float64)), axis=1)[:, :K]
    return order.astype(np.int32), np.take_along_axis(lp_full, order, 1), lp_full[:, blank].copy()
