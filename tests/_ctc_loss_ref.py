"""fp64 truth of the CTC loss csrc/st_ctc_loss.hip implements - test infrastructure only.

Two independent statements of the same definition (Graves et al. 2006 over the extended sequence l' = [0, c_0, 0, c_1, ..., 0],
S = 2 tl + 1 states, ONE skip rule for every state: s-2 -> s iff l'(s) != l'(s-2); a label may equal the blank class 0 and is
then an ordinary label state that emits column 0):

* ``alpha_beta`` - numpy, explicit alpha AND beta recursions, vectorised over batch and states: nll, the occupancies
  occ[b, t, k] = sum over states s with l'(s) = k of exp(alpha_t(s) + beta_t(s) - lp[b, t, k] + nll), and the gradient in the
  convention st_ctc_dlogits consumes, g = coef (exp(lp) - occ) below in_len, 0 past it, 0 where nll is infinite.
* ``nll_torch`` - a differentiable torch restatement of the FORWARD recursion alone (T sequential logsumexp steps, any device):
  autograd through it gives d nll / d lp = -occ without ever writing a beta recursion.
"""
import numpy as np
import torch

NEG = -np.inf


def _extended(classes, tgt_len):
    """-> ext [B, S_max] (class per state, 0 at blank states), live [B, S_max] (s < 2 tl + 1), skip [B, S_max]"""
    classes = np.asarray(classes).astype(np.int64)
    B, L = classes.shape
    S = 2 * L + 1
    ext = np.zeros((B, S), dtype=np.int64)
    ext[:, 1::2] = classes
    live = np.arange(S)[None, :] < (2 * np.asarray(tgt_len)[:, None] + 1)
    skip = np.zeros((B, S), dtype=bool)
    skip[:, 2:] = ext[:, 2:] != ext[:, :-2]
    return ext, live, skip


def _lae(*xs):
    m = np.maximum.reduce(xs)
    ms = np.where(np.isfinite(m), m, 0.0)
    with np.errstate(divide="ignore"):
        return np.where(np.isfinite(m), ms + np.log(sum(np.exp(x - ms) for x in xs)), NEG)


def alpha_beta(lp, classes, in_len, tgt_len, coef=None):
    """lp [B, T, C] (anything float; frames past in_len may hold NaN: they are never used), classes [B, L] ints in [0, C),
    in_len / tgt_len [B].  -> dict(nll [B] (+inf: no alignment), occ [B, T, C], g [B, T, C], roww [B]) in float64."""
    lp = np.asarray(lp, dtype=np.float64)
    B, T, C = lp.shape
    il, tl = np.asarray(in_len).astype(np.int64), np.asarray(tgt_len).astype(np.int64)
    coef = np.ones(B) if coef is None else np.asarray(coef, dtype=np.float64)
    ext, live, skip = _extended(classes, tl)
    S = ext.shape[1]
    frame_ok = np.arange(T)[None, :] < il[:, None]
    em = np.take_along_axis(np.where(frame_ok[:, :, None], lp, 0.0), np.broadcast_to(ext[:, None, :], (B, T, S)), axis=2)
    em = np.where(live[:, None, :], em, NEG)
    sh1 = lambda a: np.concatenate([np.full((B, 1), NEG), a], 1)[:, :S]            # the value of state s - 1 at s
    sh2 = lambda a: np.concatenate([np.full((B, 2), NEG), a], 1)[:, :S]
    up1 = lambda a: np.concatenate([a, np.full((B, 1), NEG)], 1)[:, 1:]            # ... of state s + 1
    up2 = lambda a: np.concatenate([a, np.full((B, 2), NEG)], 1)[:, 2:]
    skip_up = np.concatenate([skip, np.zeros((B, 2), dtype=bool)], 1)[:, 2:]       # s -> s + 2 allowed iff l'(s + 2) != l'(s)
    alpha = np.full((B, T, S), NEG)
    beta = np.full((B, T, S), NEG)
    with np.errstate(invalid="ignore"):
        a = np.full((B, S), NEG)
        a[:, 0] = 0.0                                        # before frame 0: probability 1 in state 0
        for t in range(T):
            a = _lae(a, sh1(a), np.where(skip, sh2(a), NEG)) + em[:, t]
            alpha[:, t] = a
        last = np.maximum(il - 1, 0)
        b_ = np.full((B, S), NEG)
        for t in range(T - 1, -1, -1):
            init = np.where((np.arange(S)[None, :] == 2 * tl[:, None]) | (np.arange(S)[None, :] == 2 * tl[:, None] - 1), em[:, t], NEG)
            rec = _lae(b_, up1(b_), np.where(skip_up, up2(b_), NEG)) + em[:, t]
            b_ = np.where((t == last)[:, None], init, np.where((t < last)[:, None], rec, NEG))
            beta[:, t] = b_
        rows = np.arange(B)
        end = alpha[rows, last]
        ll = _lae(end[rows, 2 * tl], np.where(tl > 0, end[rows, np.maximum(2 * tl - 1, 0)], NEG))
        ll = np.where(il > 0, ll, NEG)
        nll = -ll
        fin = np.isfinite(nll)
        # occupancies: the states of a class accumulated in the probability domain
        post = np.exp(alpha + beta - em + np.where(fin, nll, 0.0)[:, None, None])
        post = np.where(np.isfinite(alpha) & np.isfinite(beta) & frame_ok[:, :, None] & fin[:, None, None], post, 0.0)
    occ = np.zeros((B, T, C))
    for s in range(S):
        occ[rows, :, ext[:, s]] += post[:, :, s]              # (one state per utterance at a time: no index repeats)
    soft = np.where(frame_ok[:, :, None] & fin[:, None, None], np.exp(np.where(frame_ok[:, :, None], lp, 0.0)), 0.0)
    g = coef[:, None, None] * (soft - occ)
    return dict(nll=nll, occ=occ, g=g, roww=np.where(fin, coef, 0.0))


def nll_torch(lp, classes, in_len, tgt_len):
    """Differentiable restatement: lp [B, T, C] (float64 for truth), classes [B, L] int64, in_len / tgt_len [B] int tensors on
    lp's device.  -> nll [B]; an utterance without an alignment comes back > 1e200 (a finite stand-in for +inf keeps autograd
    free of NaN) - mask it with ``torch.where`` before reducing.  Frames past in_len are never read."""
    B, T, C = lp.shape
    L = classes.shape[1]
    S = 2 * L + 1
    dev, big = lp.device, -1e300 if lp.dtype == torch.float64 else -1e30
    il, tl = in_len.to(dev).long(), tgt_len.to(dev).long()
    ext = torch.zeros(B, S, dtype=torch.long, device=dev)
    ext[:, 1::2] = classes.to(dev).long()
    neg = torch.tensor(big, dtype=lp.dtype, device=dev)
    live = torch.arange(S, device=dev).view(1, -1) < (2 * tl + 1).view(-1, 1)
    skip = torch.zeros(B, S, dtype=torch.bool, device=dev)
    skip[:, 2:] = ext[:, 2:] != ext[:, :-2]
    a = torch.full((B, S), big, dtype=lp.dtype, device=dev)
    a[:, 0] = 0.0
    out = torch.full((B,), -big, dtype=lp.dtype, device=dev)
    i_last, i_prev = (2 * tl).view(-1, 1), (2 * tl - 1).clamp_min(0).view(-1, 1)
    for t in range(T):
        ok = (t < il).view(-1, 1)
        em = torch.where(ok & live, torch.where(ok, lp[:, t], neg).gather(1, ext), neg)
        a1 = torch.cat([neg.expand(B, 1), a], 1)[:, :S]
        a2 = torch.where(skip, torch.cat([neg.expand(B, 2), a], 1)[:, :S], neg)
        a = (torch.logsumexp(torch.stack([a, a1, a2], 0), 0) + em).clamp_min(big)
        fin = il - 1 == t
        if bool(fin.any()):
            last = a.gather(1, i_last).squeeze(1)
            prev = torch.where(tl > 0, a.gather(1, i_prev).squeeze(1), neg)
            out = torch.where(fin, -torch.logaddexp(last, prev), out)
    return out


def is_inf(nll):
    """The restatement's stand-in for an infinite loss."""
    return nll > 1e200 if nll.dtype == torch.float64 else nll > 1e29
