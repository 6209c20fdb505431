"""NumPy float32 emulation of the trie walk of csrc/st_ngram.hip over the host arrays of a ``st_amd.ngram.DeviceTrie`` - the same
values, the same order of the same fp32 additions, so the kernels' raw scores can be compared BIT for bit - and the derived bound
of that walk against the fp64 definition (``NGramLM.logp`` over the same rounded values)."""
import numpy as np

F = np.float32
NINF = F(-np.inf)


def find_child(h, nodes, V, node, t):
    lo, hi = max(int(h["child_lo"][node]), V), min(int(h["child_lo"][node + 1]), nodes)
    i = lo + int(np.searchsorted(h["tok"][lo:hi], t))
    return i if i < hi and int(h["tok"][i]) == t else -1


def valid_history(trie, hist):
    """``hist`` oldest first (-1 = no token) -> the valid tokens, most recent first: up to the first id outside [0, V)."""
    out = []
    for t in list(hist)[::-1][:trie.order - 1]:
        t = int(t)
        if t < 0 or t >= trie.V:
            break
        out.append(t)
    return out


def score(trie, hist, c, terms=None):
    """The raw score of candidate ``c`` after ``hist`` (oldest first) as the kernels compute it, np.float32.  ``terms``: a list
    that receives the summands (for the bound)."""
    h, V, nodes = trie.host, trie.V, trie.nodes
    c = int(c)
    if c < 0 or c >= V:
        return NINF
    rec = valid_history(trie, hist)
    k = len(rec)
    bo = [F(0.0)] * k
    node = -1
    for j in range(k):
        node = rec[0] if j == 0 else find_child(h, nodes, V, node, rec[j])
        if node < 0:
            break
        bo[j] = h["bo"][node]
    val, m = h["logp"][c], 1
    if val == F(np.inf):
        val = F(trie.oov_logp)
    else:
        node = c
        for j in range(k):
            node = find_child(h, nodes, V, node, rec[j])
            if node < 0:
                break
            val, m = h["logp"][node], j + 2
    val = F(val)
    if terms is not None:
        terms.append(float(val))
    with np.errstate(invalid="ignore"):
        for j in range(m, k + 1):
            val = F(val + bo[j - 1])
            if terms is not None:
                terms.append(float(bo[j - 1]))
    return val


def score_rows(trie, hist, cand, eos, done=None, beam=1):
    """st_ngram_score's raw output: f32 [n, K]; NaN where the kernel writes nothing (the rows of a done utterance)."""
    n, K = cand.shape
    out = np.full((n, K), np.nan, dtype=F)
    for i in range(n):
        if done is not None and done[i // beam]:
            continue
        if hist[i, -1] >= 0 and hist[i, -1] == eos:
            out[i] = 0.0
            continue
        for j in range(K):
            out[i, j] = score(trie, hist[i], cand[i, j])
    return out


def score_seq(trie, tokens, lens, bos):
    """st_ngram_score_seq's output: f32 [M, L_cap]."""
    M, L = tokens.shape
    out = np.zeros((M, L), dtype=F)
    for m in range(M):
        for t in range(min(int(lens[m]), L)):
            hist = ([-1] * 4 + [bos] + [int(x) for x in tokens[m, :t]])[-(trie.order - 1):]
            out[m, t] = score(trie, hist, tokens[m, t])
    return out


def advance(hist, order, tokens, eos, beam, done=None):
    """st_ngram_advance as a NumPy permutation (out of place)."""
    out = hist.copy()
    for i in range(hist.shape[0]):
        if done is not None and done[i // beam]:
            continue
        p = hist[int(order[i])]
        out[i] = p if (p[-1] >= 0 and p[-1] == eos) else np.concatenate([p[1:], [int(tokens[i])]])
    return out


def walk_bound(order, terms):
    """|fp32 walk - fp64 sum of the same terms|: at most N additions, each rounding a partial sum that is at most sum |terms|
    in magnitude by a relative 2^-24."""
    return order * 2.0 ** -24 * sum(abs(t) for t in terms)
