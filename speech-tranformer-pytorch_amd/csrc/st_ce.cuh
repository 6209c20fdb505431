// Cross-entropy over ragged logits rows: ONE kernel body for the plain loss (st_ce_fwd / st_ce_bwd in st_misc.hip,
// train.py:40,120: nn.CrossEntropyLoss(ignore_index = 0)) and for the loss against a smoothed target (st_ce_smooth_fwd /
// st_ce_smooth_bwd in st_loss.hip: transformer/Loss.py:LabelSmoothingLoss, nn.CrossEntropyLoss(label_smoothing = e)),
// templated on `bool Smooth`.  Every smoothing term sits behind `if constexpr (Smooth)`: the <false> instantiation is the
// kernel the plain loss always ran - same loads, same reduction order - and <true> at (confidence 1, smooth 0, no zero
// column, no denominator) computes the same bits, because its extra factors are then exactly 1 and 0.
// One workgroup of 256 threads per row.
#pragma once
#include "st_common.cuh"

namespace {      // (internal to each translation unit that includes this file: st_misc.hip <false>, st_loss.hip <true>)

// The smoothed target of a row with target t: q[v] = confidence (v == t), 0 (v == zero_col != t), smooth (any other v < V).
// denom: device scalar the loss sum is divided by (NULL: the number of non-ignored rows).  Unused by <false>.
struct CeSmooth {
  float confidence, smooth;
  int zero_col;
  const float* denom;
};

// forward: lse[r] = logsumexp(logits[r, :V]); row_loss[r] = lse[r] - logits[r, target[r]] (0 for target == ignore); a second,
// one-workgroup kernel sums them (1,200 workgroups adding to ONE address serialise in the L2: 43 us measured that way).
// Smooth: one more per-row reduction, sum_v logits[r, v] over v < V, in the same pass; then with hasz = (zero_col >= 0 &&
// zero_col != t) and Q = sum_v q[v] = confidence + smooth (V - 1 - hasz):
//   row_loss[r] = -sum_v q[v] (x[v] - lse) = Q lse - (confidence - smooth) x[t] - smooth sum_v x[v] + smooth x[zero_col] hasz
template <bool Smooth>
__global__ __launch_bounds__(256) void ce_fwd_kernel(const float* __restrict__ logits, int ldl, int V, const long long* __restrict__ target,
                                                     const long long* __restrict__ index, int ignore, float* __restrict__ lse,
                                                     float* __restrict__ row_loss, CeSmooth sp) {
  __shared__ float red[4];
  __shared__ float redx[4];
  const int r = blockIdx.x, tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
  const float* row = logits + (size_t)r * ldl;
  float mx = -INFINITY, sm = 0.f, xs = 0.f;
  // A masked (-inf) zero column carries no target mass: it stays out of the sum of the logits (0 x -inf is 0 in the loss).  A
  // finite one is summed and taken back below, as ever.
  int zskip = -1;
  if constexpr (Smooth) {
    if (sp.zero_col >= 0 && sp.zero_col != target[index ? index[r] : r] && row[sp.zero_col] == -INFINITY) zskip = sp.zero_col;
  }
  for (int v0 = 0; v0 < V; v0 += 256 * 8) {
    float x[8];
#pragma unroll
    for (int u = 0; u < 8; ++u) x[u] = (v0 + u * 256 + tid < V) ? row[v0 + u * 256 + tid] : -INFINITY;
    if constexpr (Smooth) {
#pragma unroll
      for (int u = 0; u < 8; ++u) xs += (v0 + u * 256 + tid < V && v0 + u * 256 + tid != zskip) ? x[u] : 0.f;
    }
    float bm = x[0];
#pragma unroll
    for (int u = 1; u < 8; ++u) bm = fmaxf(bm, x[u]);
    const float mn = fmaxf(mx, bm);
    if (mn > -INFINITY) {
      float bs = 0.f;
#pragma unroll
      for (int u = 0; u < 8; ++u) bs += __expf(x[u] - mn);
      sm = sm * __expf(mx - mn) + bs;
      mx = mn;
    }
  }
  float wm = mx;
#pragma unroll
  for (int o = 32; o; o >>= 1) wm = fmaxf(wm, __shfl_xor(wm, o, 64));
  if (lane == 0) red[wave] = wm;
  if constexpr (Smooth) {
#pragma unroll
    for (int o = 32; o; o >>= 1) xs += __shfl_xor(xs, o, 64);
    if (lane == 0) redx[wave] = xs;
  }
  __syncthreads();
  const float gm = fmaxf(fmaxf(red[0], red[1]), fmaxf(red[2], red[3]));
  float s = (mx > -INFINITY) ? sm * __expf(mx - gm) : 0.f;
#pragma unroll
  for (int o = 32; o; o >>= 1) s += __shfl_xor(s, o, 64);
  __syncthreads();
  if (lane == 0) red[wave] = s;
  __syncthreads();
  if (tid == 0) {
    const float l = gm + __logf(red[0] + red[1] + red[2] + red[3]);
    lse[r] = l;
    const long long t = target[index ? index[r] : r];
    if (t != ignore && (t < 0 || t >= V)) __builtin_trap();
    if constexpr (Smooth) {
      float loss = 0.f;
      if (t != ignore) {
        const bool hasz = sp.zero_col >= 0 && sp.zero_col != t;
        const float Q = sp.confidence + sp.smooth * (float)(V - 1 - (hasz ? 1 : 0));
        // (smooth == 0 gives no column but the target any mass: a masked column must not turn 0 x -inf into NaN)
        const float xsum = sp.smooth != 0.f ? redx[0] + redx[1] + redx[2] + redx[3] : 0.f;
        loss = Q * l - (sp.confidence - sp.smooth) * row[t] - sp.smooth * xsum;
        if (hasz && zskip < 0) loss += sp.smooth * row[sp.zero_col];
      }
      row_loss[r] = loss;
    } else {
      row_loss[r] = t != ignore ? l - row[t] : 0.f;
    }
  }
}

// sums[0] = sum of row_loss, [1] = number of non-ignored rows, [2] = the loss sums[0] / sums[1].  Smooth: the loss is
// sums[0] / *denom when a denominator is given, and sums[3] = the plain token-mean NLL sum(lse[r] - logits[r][t]) / sums[1].
template <bool Smooth>
__global__ __launch_bounds__(256) void ce_sum_kernel(const float* __restrict__ row_loss, const long long* __restrict__ target,
                                                     const long long* __restrict__ index, int ignore, int R, float* __restrict__ sums,
                                                     const float* __restrict__ logits, int ldl, const float* __restrict__ lse,
                                                     CeSmooth sp) {
  __shared__ float red[Smooth ? 3 : 2][4];
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
  float a = 0.f, n = 0.f, p = 0.f;
  for (int r = tid; r < R; r += 256) {
    a += row_loss[r];
    const long long t = target[index ? index[r] : r];
    n += t != ignore ? 1.f : 0.f;
    if constexpr (Smooth) p += t != ignore ? lse[r] - logits[(size_t)r * ldl + t] : 0.f;
  }
#pragma unroll
  for (int o = 32; o; o >>= 1) { a += __shfl_xor(a, o, 64); n += __shfl_xor(n, o, 64); }
  if (lane == 0) { red[0][wave] = a; red[1][wave] = n; }
  if constexpr (Smooth) {
#pragma unroll
    for (int o = 32; o; o >>= 1) p += __shfl_xor(p, o, 64);
    if (lane == 0) red[2][wave] = p;
  }
  __syncthreads();
  if (tid == 0) {
    const float tot = red[0][0] + red[0][1] + red[0][2] + red[0][3], cnt = red[1][0] + red[1][1] + red[1][2] + red[1][3];
    sums[0] = tot;
    sums[1] = cnt;
    if constexpr (Smooth) {
      sums[2] = tot / (sp.denom ? *sp.denom : cnt);
      sums[3] = (red[2][0] + red[2][1] + red[2][2] + red[2][3]) / cnt;
    } else {
      sums[2] = tot / cnt;      // the loss (nn.CrossEntropyLoss: mean over the non-ignored tokens; 0 / 0 = nan as there)
    }
  }
}

// backward: dlogits[r][v] = (exp(logits[r][v] - lse[r]) - [v == target[r]]) * go / count for target[r] != ignore, else 0 (bf16)
// Smooth: (Q exp(logits[r][v] - lse[r]) - q[v]) * go / D, D = *denom or the count.
template <bool Smooth>
__global__ __launch_bounds__(256) void ce_bwd_kernel(const float* __restrict__ logits, int ldl, int V, const long long* __restrict__ target,
                                                     const long long* __restrict__ index, int ignore, const float* __restrict__ lse,
                                                     const float* __restrict__ sums,
                                                     const float* __restrict__ go, bf16* __restrict__ dl, int ldd, CeSmooth sp) {
  const int r = blockIdx.x, tid = threadIdx.x;
  const float* row = logits + (size_t)r * ldl;
  bf16* out = dl + (size_t)r * ldd;
  const long long t = target[index ? index[r] : r];
  float scale;
  if constexpr (Smooth) {
    scale = (t != ignore && sums[1] > 0.f) ? *go / (sp.denom ? *sp.denom : sums[1]) : 0.f;
  } else {
    scale = (t != ignore && sums[1] > 0.f) ? *go / sums[1] : 0.f;
  }
  const float l = lse[r];
  float Q = 1.f;
  if constexpr (Smooth) {
    const bool hasz = sp.zero_col >= 0 && sp.zero_col != t;
    Q = sp.confidence + sp.smooth * (float)(V - 1 - (hasz ? 1 : 0));
  }
  for (int v = tid * 8; v < ldd; v += 256 * 8) {      // ldd % 8 == 0; columns >= V get zeros
    bf16x8 o;
#pragma unroll
    for (int e = 0; e < 8; ++e) {
      const int c = v + e;
      float g = 0.f;
      if constexpr (Smooth) {
        if (c < V && scale != 0.f)
          g = (Q * __expf(row[c] - l) - (c == t ? sp.confidence : c == sp.zero_col ? 0.f : sp.smooth)) * scale;
      } else {
        if (c < V && scale != 0.f) g = (__expf(row[c] - l) - (c == t ? 1.f : 0.f)) * scale;
      }
      o[e] = (bf16)g;
    }
    *reinterpret_cast<bf16x8*>(out + v) = o;
  }
}

}  // namespace
