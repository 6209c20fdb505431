"""A plain fp64 reference of the LayerNorm the kernels form behind a GEMM (st_gemm_ln, the LayerNorm stages of st_row_chain /
st_row_chain512, the PRE stage of st_attn_f1_fwd): everything in float64, the only rounded values are the operands as they are handed
to the kernel, no output is rounded.  The statistic as include/st_hip.h states it: mean and BIASED variance over the N columns of a
row, rstd = (var + eps)^-1/2 - eps inside the root."""
import torch

F64 = torch.float64


def gemm_ln(X, W, bias, res, gamma, beta, eps, relu=False, pe=None, pos=None):
    """v = X W^T + bias [relu] (+ res); -> dict(pre=v, mean, var, rstd, xhat, out) with out = xhat gamma + beta (+ pe[pos])."""
    v = X.to(F64) @ W.to(F64).t() + bias.to(F64)
    if relu:
        v = torch.relu(v)
    if res is not None:
        v = v + res.to(F64)
    n = v.shape[1]
    mean = v.sum(1, keepdim=True) / n
    d = v - mean
    var = (d * d).sum(1, keepdim=True) / n
    rstd = (var + float(eps)) ** -0.5
    xhat = d * rstd
    out = xhat * gamma.to(F64) + beta.to(F64)
    if pe is not None:
        out = out + pe.to(F64)[pos.long()]
    return dict(pre=v, mean=mean.squeeze(1), var=var.squeeze(1), rstd=rstd.squeeze(1), xhat=xhat, out=out)


def hidden(cur, W1, b1):
    """relu(cur W1^T + b1): the feed-forward's hidden activation from the ``cur`` the kernel itself wrote."""
    return torch.relu(cur.to(F64) @ W1.to(F64).t() + b1.to(F64))
