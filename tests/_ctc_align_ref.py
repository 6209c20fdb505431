"""fp64 NumPy restatement of the CTC forced alignment (csrc/st_ctc_align.hip): the Viterbi path through the extended label
sequence l' = [0, c_0, 0, c_1, ..., 0] (class 0 = blank; a label may equal class 0 and is then an ordinary label state), with
the kernel's TIE RULE: predecessors are tried in the order stay (s), s-1, s-2 and a later candidate wins only if it is strictly
greater; at the end the blank state S-1 wins ties against the label state S-2.  Equivalently: of all best alignments, the one
that is lexicographically largest in its state sequence read from the LAST frame to the first (what
tests/test_ctc_align_cpu.py checks by enumeration).  Test infrastructure only."""
import numpy as np

NEG = -np.inf


def extended(classes):
    """-> (l' as class indices [S], skip allowed into state s [S])."""
    tl = len(classes)
    ext = np.zeros(2 * tl + 1, dtype=np.int64)
    ext[1::2] = np.asarray(classes, dtype=np.int64)
    skip = np.zeros(2 * tl + 1, dtype=bool)
    skip[2:] = ext[2:] != ext[:-2]           # (blank states: 0 == 0, never)
    return ext, skip


def states_of(path, T_in):
    """The state sequence of a returned path (label position or -1 per frame) - blank states are placed where monotonicity
    forces them: the blank before the next label that follows."""
    states, nxt = [], 0                       # nxt: the label position that comes next
    for t in range(T_in):
        j = int(path[t])
        if j >= 0:
            states.append(2 * j + 1)
            nxt = j + 1
        else:
            states.append(2 * nxt)
    return states


def align_one(lp, classes, T_in):
    """lp [T, C] (any float dtype; computed in fp64), classes: the tl label classes, T_in frames used ->
    (path int32 [T], spans int32 [tl, 2], score float64, best float64 = the recursion's end value)."""
    lp = np.asarray(lp, dtype=np.float64)
    T, tl = lp.shape[0], len(classes)
    S = 2 * tl + 1
    path = np.full(T, -1, dtype=np.int32)
    spans = np.full((tl, 2), -1, dtype=np.int32)
    T_in = max(0, min(int(T_in), T))
    if T_in == 0:
        return path, spans, NEG, NEG
    ext, skip = extended(classes)
    v = np.full(S, NEG)
    v[0] = lp[0, 0]
    if S > 1:
        v[1] = lp[0, ext[1]]
    bp = np.zeros((T_in, S), dtype=np.int8)
    for t in range(1, T_in):
        best = v.copy()
        code = np.zeros(S, dtype=np.int8)
        one = np.concatenate(([NEG], v[:-1]))
        m = one > best
        best[m], code[m] = one[m], 1
        two = np.where(skip, np.concatenate(([NEG, NEG], v[:-2]))[:S], NEG)
        m = two > best
        best[m], code[m] = two[m], 2
        v = best + lp[t, ext]
        bp[t] = code
    s = S - 1
    if S > 1 and v[S - 2] > v[S - 1]:
        s = S - 2
    if v[s] == NEG:
        return path, spans, NEG, NEG
    best_value = float(v[s])
    score = 0.0
    for t in range(T_in - 1, -1, -1):
        path[t] = (s >> 1) if (s & 1) else -1
        score += lp[t, ext[s]]
        s -= int(bp[t, s]) if t > 0 else 0
    for j in range(tl):
        frames = np.nonzero(path[:T_in] == j)[0]
        spans[j] = (frames[0], frames[-1] + 1)
    return path, spans, float(score), best_value


def align_batch(lp, classes, in_len, tgt_len):
    """lp [B, T, C], classes [B, L], lengths [B] (clamped to [0, T] / [0, L] as the kernel clamps them; classes clamped to
    [0, C - 1]) -> (path int32 [B, T], spans int32 [B, L, 2], score float32 [B], best float64 [B])."""
    lp, classes = np.asarray(lp), np.asarray(classes)
    B, T, C = lp.shape
    L = classes.shape[1]
    path = np.full((B, T), -1, dtype=np.int32)
    spans = np.full((B, L, 2), -1, dtype=np.int32)
    score = np.full(B, NEG, dtype=np.float32)
    best = np.full(B, NEG, dtype=np.float64)
    for b in range(B):
        tl = max(0, min(int(tgt_len[b]), L))
        cls = np.clip(classes[b, :tl], 0, C - 1)
        p, sp, sc, bv = align_one(lp[b], cls, in_len[b])
        path[b], spans[b, :tl], score[b], best[b] = p, sp, np.float32(sc), bv
    return path, spans, score, best
