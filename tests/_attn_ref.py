"""Plain fp64 references of the attention kernels - the slow path (csrc/st_attn_dense.hip, st_attn_probs of csrc/st_misc.hip) and
the packed kernels st_attn_fwd / st_attn_bwd (packed_attention): torch on the CPU, written from the definitions in the kernels'
header comments.  The only bf16 values are the inputs; nothing in between is rounded, no output is rounded - unlike
tests/_emul.py, which keeps the kernels' bf16 rounding points."""
import math

import torch

F64 = torch.float64


def _heads(X, B, L, H):
    """bf16 row matrix [B L, H d_k] (any leading dimension) -> fp64 [B, H, L, d_k]"""
    return X.detach().cpu().to(F64).reshape(B, L, H, -1).transpose(1, 2)


def _rows(X, B, L):
    """[B, H, L, d_k] -> [B L, H d_k]"""
    return X.transpose(1, 2).reshape(B * L, -1)


def dense_attention(Q, K, V, mask, dO, B, H, Lq, Lk, scale, keep=None, keep_scale=1.0):
    """st_attn_dense_fwd / _bwd:  s = scale q.k (masked: -inf), P = softmax(s), Pd = keep / (1 - p) P, O = Pd V,
    dP = dO V^T, delta = sum_k Pd dP, dS = P (keep / (1 - p) dP - delta), dQ = scale dS K, dK = scale dS^T Q, dV = Pd^T dO;
    a row with every key masked: P = 0, O = 0, lse = +inf, delta = 0, zero gradients.
    Q [B Lq, H d_k], K / V [B Lk, H d_k], dO like Q (None: forward only); mask [B, Lq, Lk], nonzero = masked, or None;
    keep: bool [B H, Lq, Lk] (tests/_emul.keep_qk per head slot) with keep_scale = 1 / (1 - p) as the kernels quantise it.
    -> O [B Lq, H d_k], lse [H B Lq], P [B, H, Lq, Lk], delta [H B Lq], dQ, dK, dV (fp64; the last four None without dO)."""
    q, k, v = _heads(Q, B, Lq, H), _heads(K, B, Lk, H), _heads(V, B, Lk, H)
    s = scale * (q @ k.transpose(-1, -2))
    if mask is not None:
        s = s.masked_fill(mask.detach().cpu().ne(0).view(B, 1, Lq, Lk), float("-inf"))
    dead = torch.isneginf(s).all(-1, keepdim=True)
    m = torch.where(dead, torch.zeros_like(s[..., :1]), s.amax(-1, keepdim=True))
    e = torch.exp(s - m)
    z = e.sum(-1, keepdim=True)
    P = torch.where(dead, torch.zeros_like(e), e / torch.where(dead, torch.ones_like(z), z))
    lse = torch.where(dead, torch.full_like(z, float("inf")), m + torch.log(torch.where(dead, torch.ones_like(z), z))).squeeze(-1)
    w = torch.ones_like(P) if keep is None else keep.view(B, H, Lq, Lk).to(F64) * keep_scale
    Pd = P * w
    O = Pd @ v
    flat = lambda t: t.permute(1, 0, 2).reshape(-1)                      # [B, H, Lq] -> [H, B Lq]
    if dO is None:
        return _rows(O, B, Lq), flat(lse), P, None, None, None, None
    do = _heads(dO, B, Lq, H)
    dP = do @ v.transpose(-1, -2)
    delta = (Pd * dP).sum(-1)
    dS = P * (w * dP - delta.unsqueeze(-1))
    dQ, dK, dV = scale * (dS @ k), scale * (dS.transpose(-1, -2) @ q), Pd.transpose(-1, -2) @ do
    return _rows(O, B, Lq), flat(lse), P, flat(delta), _rows(dQ, B, Lq), _rows(dK, B, Lk), _rows(dV, B, Lk)


def packed_attention(Q, K, V, dO, q_off, q_len, k_off, k_len, H, causal, scale, k_prescaled=False, keep=None, keep_scale=1.0,
                     delta_in=None):
    """st_attn_fwd / st_attn_bwd (include/st_hip.h; csrc/st_attn_common.cuh, AttnArgs): utterance b owns rows q_off[b] ..
    q_off[b] + q_len[b] - 1 of Q / O / dO / dQ and k_off[b] .. k_off[b] + k_len[b] - 1 of K / V / dK / dV (packed or padded: the
    offsets say), head h columns h d_k .. of each.  Per (b, h):
        s = scale q.k (causal: keys > the query masked), P = softmax(s), Pd = keep / (1 - p) P, O = Pd V,
        lse = log2 sum_k exp(s) = m + log2 l (the kernels' log2 domain: P = exp2(s log2 e - lse)),
        dP = dO V^T, delta = sum_k Pd dP (= rowsum(dO O)), dS = P (keep / (1 - p) dP - delta),
        dQ = scale dS K, dK = scale dS^T Q, dV = Pd^T dO.
    k_prescaled: K holds K~ = bf16(scale log2(e) k); the key is then k = K~ / (scale log2 e) - the score is ln 2 (q . K~) - and dK is
    still the gradient of that UNSCALED key.  keep: None or a list over (b H + h) of bool [q_len[b], k_len[b]]
    (tests/_emul.keep_qk per head slot), keep_scale = 1 / (1 - p) as the kernels quantise it.  delta_in ([H, rows of Q] flat): the
    delta the backward under test was handed or formed from a rounded O - dS = P (keep / (1 - p) dP - delta_in), so that dQ and dK
    are what exact arithmetic makes of THAT delta (the returned delta is sum_k Pd dP either way).
    -> O [rows of Q, H d_k], lse [H, rows of Q] flat, delta likewise, dQ, dK, dV: fp64, unrounded; rows of no utterance hold 0."""
    Qd, Kd, Vd, dOd = (t.detach().cpu().to(F64) for t in (Q, K, V, dO))
    if k_prescaled:
        Kd = Kd / (scale * math.log2(math.e))
    Mq, Mk, d = Qd.shape[0], Kd.shape[0], Qd.shape[1]
    dk = d // H
    O, dQ = torch.zeros(Mq, d, dtype=F64), torch.zeros(Mq, d, dtype=F64)
    dK, dV = torch.zeros(Mk, d, dtype=F64), torch.zeros(Mk, d, dtype=F64)
    lse, delta = torch.zeros(H, Mq, dtype=F64), torch.zeros(H, Mq, dtype=F64)
    for b in range(len(q_len)):
        qo, ql, ko, kl = int(q_off[b]), int(q_len[b]), int(k_off[b]), int(k_len[b])
        if ql == 0 or kl == 0:
            continue
        qs, ks = slice(qo, qo + ql), slice(ko, ko + kl)
        for h in range(H):
            cs = slice(h * dk, (h + 1) * dk)
            q, k, v, do = Qd[qs, cs], Kd[ks, cs], Vd[ks, cs], dOd[qs, cs]
            s = scale * (q @ k.t())
            if causal:
                s = s.masked_fill(torch.arange(kl).view(1, -1) > torch.arange(ql).view(-1, 1), float("-inf"))
            m = s.amax(-1, keepdim=True)
            e = torch.exp(s - m)
            l = e.sum(-1, keepdim=True)
            P = e / l
            w = torch.ones_like(P) if keep is None else keep[b * H + h].to(F64) * keep_scale
            Pd = P * w
            dP = do @ v.t()
            dl = (Pd * dP).sum(-1, keepdim=True)
            dS = P * (w * dP - (dl if delta_in is None else delta_in.to(F64).view(H, Mq)[h, qs].unsqueeze(-1)))
            O[qs, cs] = Pd @ v
            lse[h, qs] = ((m + torch.log(l)) / math.log(2.0)).squeeze(-1)
            delta[h, qs] = dl.squeeze(-1)
            dQ[qs, cs], dK[ks, cs], dV[ks, cs] = scale * (dS @ k), scale * (dS.t() @ q), Pd.t() @ do
    return O, lse.reshape(-1), delta.reshape(-1), dQ, dK, dV


def attention_probs(Q, K, q_len, k_len, offsets, H, Lq, Lk, causal, scale, k_prescaled=False):
    """st_attn_probs: P [B, H, Lq, Lk] = softmax over keys of scale Q K^T with keys >= k_len[b] (and, causal, keys > the query)
    masked out; zeros there and in the rows of query positions >= q_len[b].  Utterance b owns rows off[b] .. off[b] + len[b] - 1
    of the row matrices (offsets = (q_off, k_off)), head h columns h d_k ..  k_prescaled: K holds scale log2(e) k, so the
    score is ln 2 (q . K)."""
    q_off, k_off = offsets
    B = len(q_len)
    Qd, Kd = Q.detach().cpu().to(F64), K.detach().cpu().to(F64)
    P = torch.zeros(B, H, Lq, Lk, dtype=F64)
    for b in range(B):
        lq, lk, qo, ko = int(q_len[b]), int(k_len[b]), int(q_off[b]), int(k_off[b])
        if lq == 0 or lk == 0:
            continue
        q = Qd[qo:qo + lq].reshape(lq, H, -1).transpose(0, 1)
        k = Kd[ko:ko + lk].reshape(lk, H, -1).transpose(0, 1)
        s = (q @ k.transpose(-1, -2)) * (math.log(2.0) if k_prescaled else scale)
        if causal:
            s = s.masked_fill(torch.ones(lq, lk, dtype=torch.bool).triu(1), float("-inf"))
        P[b, :, :lq, :lk] = torch.softmax(s, -1)
    return P
