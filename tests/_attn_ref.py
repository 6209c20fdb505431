"""Plain fp64 references of the slow-path attention kernels (csrc/st_attn_dense.hip, st_attn_probs of csrc/st_misc.hip): torch on
the CPU, written from the definitions in the kernels' header comments.  The only bf16 values are the inputs; nothing in between
is rounded, no output is rounded - unlike tests/_emul.py, which keeps the kernels' bf16 rounding points."""
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
