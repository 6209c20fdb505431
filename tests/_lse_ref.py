"""Plain fp64 reference of the vocabulary log-sum-exp family (tests/test_lse_fp64_gpu.py, tests/test_lse_fp64_cpu.py): the only
rounded values are the fp32 logits as handed to the kernels.  A -inf logit is a column of probability zero (the row has a finite
column); 0 x -inf inside a target-weighted sum is 0, so a masked column the smoothed target gives no mass to costs nothing and one
it gives mass to makes the loss +inf.  Everything here is torch on the CPU, row by row over x f32 / f64 [R, V]."""
import torch

F64 = torch.float64


def lse(x):
    return torch.logsumexp(x.to(F64), -1)


def log_softmax(x):
    return x.to(F64) - lse(x).unsqueeze(-1)


def softmax(x):
    return torch.exp(log_softmax(x))


def ulp32(v):
    """Spacing of fp32 at |v| (fp64 tensor): 2^(floor(log2 |v|) - 23), the smallest normal's spacing below it."""
    a = torch.as_tensor(v, dtype=F64).abs().clamp_min(2.0 ** -126)
    return torch.exp2(torch.floor(torch.log2(a)) - 23)


def smoothed_target(R, V, target, confidence, smooth, zero_col):
    """q f64 [R, V] of include/st_hip.h: confidence at the target, 0 at zero_col (when it is not the target), smooth elsewhere."""
    q = torch.full((R, V), float(smooth), dtype=F64)
    if zero_col >= 0:
        q[:, zero_col] = 0.0
    q.scatter_(1, target.view(-1, 1), float(confidence))
    return q


def row_loss(x, target, confidence=1.0, smooth=0.0, zero_col=-1):
    """-sum_v q[v] log-softmax(x)[v] per row (0 x -inf = 0); (1, 0, -1) is the plain loss lse - x[t]."""
    lp = log_softmax(x)
    q = smoothed_target(x.shape[0], x.shape[1], target, confidence, smooth, zero_col)
    return -torch.where(q == 0, torch.zeros_like(lp), q * lp).sum(-1)


def nll(x, target):
    return -log_softmax(x).gather(1, target.view(-1, 1)).squeeze(1)


def grad_ce(x, target, confidence=1.0, smooth=0.0, zero_col=-1):
    """d row_loss / d logits = Q softmax - q, in probability units (the kernels multiply it by *grad_out / D)."""
    q = smoothed_target(x.shape[0], x.shape[1], target, confidence, smooth, zero_col)
    return q.sum(-1, keepdim=True) * softmax(x) - q


def grad_ctc(x):
    """st_ctc_dlogits' dense term in probability units (divided by roww[b] * *grad_out): the softmax."""
    return softmax(x)


def best(values, k):
    """The candidate list of every row of an fp64 [n, m] table, best first, lower index on ties -> (ids i64, values), both
    [n, min(k + 1, m)]: the k chosen ones and the first one LEFT OUT (the gap at the cut is part of the list's gaps)."""
    v, idx = torch.sort(values.to(F64), dim=-1, descending=True, stable=True)
    return idx[:, :k + 1], v[:, :k + 1]


def gaps(v):
    """v[:, r] - v[:, r + 1] of a sorted candidate list; a tie among masked (-inf) candidates counts as a gap of 0."""
    d = v[:, :-1] - v[:, 1:]
    return torch.where(torch.isnan(d), torch.zeros_like(d), d)
