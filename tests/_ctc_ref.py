"""fp64 restatement of the CTC prefix scorer (Watanabe et al. 2017, Algorithm 2) that csrc/st_ctc_decode.hip implements -
test infrastructure only.  x: log-probabilities [T, V] (numpy float64) of one utterance; a prefix's state is
(gamma_n [T], gamma_b [T], psi, last) with last = -1 for the empty prefix.  ``extend_batch`` runs many extensions at once
(rows = independent (state, token) pairs, ragged lengths) so the GPU tests can check thousands of waves against it."""
import numpy as np

NEG = -np.inf


def empty_state(x, blank):
    T = x.shape[0]
    return np.full(T, NEG), np.cumsum(x[:, blank]), 0.0, -1


def extend_batch(xc, xb, gn, gb, last, c, T, blank, eos):
    """Rows n: xc / xb [N, Tm] = x_t(c_n) / x_t(blank) of row n's utterance, gn / gb [N, Tm] its prefix's state, last [N],
    c [N] the tokens, T [N] the frame counts (frames >= T[n] are ignored).  -> (psi_h [N], hn [N, Tm], hb [N, Tm]); EOS rows:
    psi = logaddexp(gn[T-1], gb[T-1]) (state rows meaningless), blank rows: -inf."""
    N, Tm = xc.shape
    T = np.asarray(T)
    phi = np.where((c == last)[:, None], gb, np.logaddexp(gn, gb))
    hn = np.full((N, Tm), NEG)
    hb = np.full((N, Tm), NEG)
    hn[:, 0] = np.where(last < 0, xc[:, 0], NEG)
    with np.errstate(invalid="ignore"):
        for t in range(1, Tm):
            hn[:, t] = np.logaddexp(hn[:, t - 1], phi[:, t - 1]) + xc[:, t]
            hb[:, t] = np.logaddexp(hn[:, t - 1], hb[:, t - 1]) + xb[:, t]
    terms = np.full((N, Tm), NEG)
    terms[:, 0] = hn[:, 0]
    terms[:, 1:] = phi[:, :-1] + xc[:, 1:]
    terms[np.arange(Tm)[None, :] >= T[:, None]] = NEG
    mx = terms.max(1)
    with np.errstate(invalid="ignore", divide="ignore"):
        psi = np.where(np.isfinite(mx), mx + np.log(np.exp(terms - np.where(np.isfinite(mx), mx, 0.0)[:, None]).sum(1)), NEG)
    idx = np.maximum(T - 1, 0)
    end = np.logaddexp(gn[np.arange(N), idx], gb[np.arange(N), idx])
    psi = np.where(c == eos, end, np.where(c == blank, NEG, psi))
    return psi, hn, hb


def extend(x, state, c, blank, eos):
    """One extension g -> g.c of one utterance: -> (psi(g.c), new state or None for EOS / blank)."""
    gn, gb, _, last = state
    T = x.shape[0]
    psi, hn, hb = extend_batch(x[None, :, c], x[None, :, blank], gn[None], gb[None], np.array([last]), np.array([c]), [T],
                               blank, eos)
    if c in (blank, eos):
        return float(psi[0]), None
    return float(psi[0]), (hn[0], hb[0], float(psi[0]), c)


def prefix_scores(x, labels, blank, eos):
    """psi of every prefix of ``labels`` (psi(empty) first) and psi(labels . EOS) = log p_ctc(labels | x)."""
    st = empty_state(x, blank)
    out = [0.0]
    for c in labels:
        p, st = extend(x, st, c, blank, eos)
        out.append(p)
    p_end, _ = extend(x, st, eos, blank, eos)
    return out, p_end


def increments(x, labels, blank, eos):
    """Delta(c | g) along ``labels`` followed by EOS: they telescope to log p_ctc(labels | x)."""
    psis, end = prefix_scores(x, labels, blank, eos)
    return [b - a for a, b in zip(psis, psis[1:] + [end])]
