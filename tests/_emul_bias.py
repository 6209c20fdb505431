"""NumPy float32 emulation of the automaton walk of csrc/st_bias.hip over the host arrays of a ``st_amd.biasing.DeviceAutomaton`` -
the same values, the same order of the same fp32 operations, so the kernels' increments can be compared BIT for bit - and the
derived bound of that walk against the fp64 definition over the same rounded tables (``DeviceAutomaton.rounded_model()``)."""
import numpy as np

F = np.float32
MAX_DEPTH = 32


def find_child(h, S, node, t):
    lo, hi = min(max(int(h["child_lo"][node]), 0), S), min(max(int(h["child_lo"][node + 1]), 0), S)
    if lo >= hi:
        return -1
    i = lo + int(np.searchsorted(h["tok"][lo:hi], t))
    return i if i < hi and int(h["tok"][i]) == t else -1


def next_state(tables, s, c):
    """delta(s, c) as the kernels walk it: at most MAX_DEPTH fail moves."""
    h, S = tables.host, tables.S
    s, c = min(max(int(s), 0), S - 1), int(c)
    ch = find_child(h, S, s, c)
    it = 0
    while it < MAX_DEPTH and ch < 0 and s != 0:
        s = min(max(int(h["fail"][s]), 0), S - 1)
        ch = find_child(h, S, s, c)
        it += 1
    return ch if ch >= 0 else 0


def delta(tables, s, c, eos, terms=None):
    """-> (Delta(s, c) as np.float32, the state after c; -1 after eos) for a live state s.  ``terms``: a list that receives the
    operands of the position's additions (for the bound)."""
    h = tables.host
    s = min(max(int(s), 0), tables.S - 1)
    c = int(c)
    if c >= 0 and c == eos:
        if terms is not None:
            terms.append(float(h["phi"][s]))
        return F(-h["phi"][s]), -1
    s2 = next_state(tables, s, c)
    d = F(h["cash"][s2] + F(h["phi"][s2] - h["phi"][s]))
    if terms is not None:
        terms += [float(h["cash"][s2]), float(h["phi"][s2]), float(h["phi"][s])]
    return d, s2


def score_rows(tables, state, cand, eos, done=None, beam=1):
    """st_bias_score's raw output: f32 [n, K]; NaN where the kernel writes nothing (the rows of a done utterance)."""
    n, K = cand.shape
    out = np.full((n, K), np.nan, dtype=F)
    for i in range(n):
        if done is not None and done[i // beam]:
            continue
        if state[i] < 0:
            out[i] = 0.0
            continue
        for j in range(K):
            out[i, j] = delta(tables, state[i], cand[i, j], eos)[0]
    return out


def fuse(lp, scale, raw):
    """lp = fmaf(scale, raw, lp) in float32: ONE rounding of the exact scale x raw + lp.  The fp64 product of two floats is exact;
    the fp64 sum is exact too when the operands are dyadic numbers of few bits, as the tests draw them (lp a multiple of 2^-10
    below 16 in magnitude, dyadic weights and scale), so the single rounding to float32 here is fmaf's."""
    return (np.float64(F(scale)) * raw.astype(np.float64) + lp.astype(np.float64)).astype(F)


def score_seq(tables, tokens, lens, eos, terms=None):
    """st_bias_score_seq's output: f32 [M, L_cap].  ``terms``: a list that receives one operand list per scored position."""
    M, L = tokens.shape
    out = np.zeros((M, L), dtype=F)
    for m in range(M):
        s = 0
        for t in range(min(max(int(lens[m]), 0), L)):
            if s < 0:
                break
            pos = [] if terms is not None else None
            out[m, t], s = delta(tables, s, tokens[m, t], eos, pos)
            if terms is not None:
                terms.append(pos)
    return out


def advance(tables, state, order, tokens, eos, beam, done=None):
    """st_bias_advance as a NumPy permutation (out of place)."""
    out = state.copy()
    for i in range(state.shape[0]):
        if done is not None and done[i // beam]:
            continue
        base = (i // beam) * beam
        p = int(order[i])
        if p < base or p >= base + beam:
            p = i
        c = int(tokens[i])
        out[i] = -1 if (state[p] < 0 or (c >= 0 and c == eos)) else next_state(tables, state[p], c)
    return out


def walk_bound(terms):
    """|fp32 Delta - fp64 Delta over the same table values| of one position: cash + (phi' - phi) is two fp32 operations, each
    rounding a value of magnitude at most sum |operands| by a relative 2^-24; -phi (one operand) is exact."""
    return 0.0 if len(terms) < 2 else 2 * 2.0 ** -24 * sum(abs(t) for t in terms)
