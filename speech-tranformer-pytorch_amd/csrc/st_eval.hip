// Forward-only validation over ragged logits rows (gfx950): st_ce_eval_fwd / st_eval_note of include/st_hip.h.
// st_ce_eval_fwd: per row, in ONE pass over the logits, the criterion's numerator (the formula of ce_fwd_kernel<true> in
// st_ce.cuh), the plain NLL and whether the arg-max over the vocabulary is the target.  st_eval_note: the fixed-order fp64
// sum of those rows, ADDED into an epoch accumulator in device memory - no host read between the first batch of a validation
// pass and its last.  The training loss kernels (st_ce.cuh) are shared with the training step and stay as they are: this is a
// body of its own in a translation unit of its own.  Unlike them it never traps: a target outside [0, V) that is not the
// ignored index is counted (state 2 below), not executed on.
// Bandwidth kernel over R x V fp32, one workgroup of 256 threads per row; plain C++, vector stores.
#include "st_common.cuh"

namespace {

// The order the arg-max is taken in: a larger value wins, and among equal values the LOWER column - at every level of the
// reduction (a thread's 8 values of a chunk, the chunks of the loop, the lanes of a wave, the four waves).  NaN never wins.
__device__ __forceinline__ bool eval_better(float v, int i, float bv, int bi) { return v > bv || (v == bv && i < bi); }

__global__ __launch_bounds__(256) void ce_eval_fwd_kernel(const float* __restrict__ logits, int ldl, int V,
                                                          const long long* __restrict__ target, const long long* __restrict__ index,
                                                          int ignore, float confidence, float smooth, int zero_col,
                                                          float* __restrict__ rows) {
  __shared__ float red_m[4];
  __shared__ int red_i[4];
  __shared__ float red_x[4];
  __shared__ float red_s[4];
  const int r = blockIdx.x, tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
  const float* row = logits + (size_t)r * ldl;
  // running maximum WITH its column (bv, bi), the exponential sum rescaled to it, the plain sum of the logits
  float bv = -INFINITY, sm = 0.f, xs = 0.f;
  int bi = 0x7fffffff;
  // (a masked zero column that carries no target mass stays out of the sum of the logits: ce_fwd_kernel<true> in st_ce.cuh)
  const int zskip = (zero_col >= 0 && zero_col != target[index ? index[r] : r] && row[zero_col] == -INFINITY) ? zero_col : -1;
  for (int v0 = 0; v0 < V; v0 += 256 * 8) {
    float x[8];
#pragma unroll
    for (int u = 0; u < 8; ++u) x[u] = (v0 + u * 256 + tid < V) ? row[v0 + u * 256 + tid] : -INFINITY;
    const float mx = bv;
#pragma unroll
    for (int u = 0; u < 8; ++u) {      // (columns in ascending order: the first of equal values is kept)
      const int c = v0 + u * 256 + tid;
      if (c < V) {
        xs += c != zskip ? x[u] : 0.f;
        if (eval_better(x[u], c, bv, bi)) { bv = x[u]; bi = c; }
      }
    }
    if (bv > -INFINITY) {
      float bs = 0.f;
#pragma unroll
      for (int u = 0; u < 8; ++u) bs += __expf(x[u] - bv);
      sm = sm * __expf(mx - bv) + bs;
    }
  }
  float wv = bv;
  int wi = bi;
#pragma unroll
  for (int o = 32; o; o >>= 1) {
    const float ov = __shfl_xor(wv, o, 64);
    const int oi = __shfl_xor(wi, o, 64);
    if (eval_better(ov, oi, wv, wi)) { wv = ov; wi = oi; }
    xs += __shfl_xor(xs, o, 64);
  }
  if (lane == 0) { red_m[wave] = wv; red_i[wave] = wi; red_x[wave] = xs; }
  __syncthreads();
  float gm = red_m[0];
  int gi = red_i[0];
#pragma unroll
  for (int w = 1; w < 4; ++w)
    if (eval_better(red_m[w], red_i[w], gm, gi)) { gm = red_m[w]; gi = red_i[w]; }
  float s = (bv > -INFINITY) ? sm * __expf(bv - gm) : 0.f;
#pragma unroll
  for (int o = 32; o; o >>= 1) s += __shfl_xor(s, o, 64);
  if (lane == 0) red_s[wave] = s;
  __syncthreads();
  if (tid == 0) {
    const long long t = target[index ? index[r] : r];
    f32x4 out = {0.f, 0.f, 0.f, 0.f};      // {row_loss, row_nll, row_hit, state}; ignored rows: all zero
    if (t != ignore) {
      if (t < 0 || t >= V) {
        out[3] = 2.f;                      // a stray label: counted by st_eval_note, contributes nothing else
      } else {
        const float l = gm + __logf(red_s[0] + red_s[1] + red_s[2] + red_s[3]);
        const float xt = row[t];
        const bool hasz = zero_col >= 0 && zero_col != t;
        const float Q = confidence + smooth * (float)(V - 1 - (hasz ? 1 : 0));
        const float xsum = smooth != 0.f ? red_x[0] + red_x[1] + red_x[2] + red_x[3] : 0.f;      // (0 x -inf must not become NaN)
        float loss = Q * l - (confidence - smooth) * xt - smooth * xsum;
        if (hasz && zskip < 0) loss += smooth * row[zero_col];
        out[0] = loss;
        out[1] = l - xt;
        out[2] = gi == (int)t ? 1.f : 0.f;
        out[3] = 1.f;
      }
    }
    *reinterpret_cast<f32x4*>(rows + (size_t)r * 4) = out;
  }
}

// One workgroup: thread i adds rows i, i + 256, .. in fp64, then lanes and waves in a fixed order - the sums do not depend on
// anything but the rows.  (R workgroups adding to one address is what st_ce.cuh measured at 43 us.)
__global__ __launch_bounds__(256) void eval_note_kernel(const float* __restrict__ rows, int R, const float* __restrict__ denom,
                                                        double* __restrict__ acc, float* __restrict__ last) {
  __shared__ double red[5][4];
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
  double a[5] = {0.0, 0.0, 0.0, 0.0, 0.0};      // loss, NLL, hits, tokens, bad targets
  for (int r = tid; r < R; r += 256) {
    const f32x4 q = *reinterpret_cast<const f32x4*>(rows + (size_t)r * 4);
    a[0] += (double)q[0];
    a[1] += (double)q[1];
    a[2] += (double)q[2];
    a[3] += q[3] == 1.f ? 1.0 : 0.0;
    a[4] += q[3] == 2.f ? 1.0 : 0.0;
  }
#pragma unroll
  for (int k = 0; k < 5; ++k) {
#pragma unroll
    for (int o = 32; o; o >>= 1) a[k] += __shfl_xor(a[k], o, 64);
    if (lane == 0) red[k][wave] = a[k];
  }
  __syncthreads();
  if (tid == 0) {
    double t[5];
#pragma unroll
    for (int k = 0; k < 5; ++k) t[k] = ((red[k][0] + red[k][1]) + red[k][2]) + red[k][3];
    const double den = denom ? (double)*denom : t[3];
    acc[0] += t[0];
    acc[1] += den;
    acc[2] += t[1];
    acc[3] += t[3];
    acc[4] += t[2];
    acc[5] += 1.0;
    acc[6] += t[4];
    const f32x4 out = {(float)(t[0] / den), (float)(t[1] / t[3]), (float)(t[2] / t[3]), (float)t[3]};      // no token: 0 / 0 = nan
    *reinterpret_cast<f32x4*>(last) = out;
  }
}

}  // namespace

extern "C" int st_ce_eval_fwd(hipStream_t stream, const float* logits, int ldl, int R, int V, const long long* target,
                              const long long* target_index, int ignore_index, float confidence, float smooth, int zero_col,
                              float* rows) {
  if (R <= 0) return 0;
  if (!logits || !target || !rows || V <= 0 || ldl < V || zero_col >= V || ((size_t)rows & 15)) return -1;
  hipLaunchKernelGGL(ce_eval_fwd_kernel, dim3(R), dim3(256), 0, stream, logits, ldl, V, target, target_index, ignore_index,
                     confidence, smooth, zero_col < 0 ? -1 : zero_col, rows);
  ST_CHECK_LAUNCH();
  return 0;
}

extern "C" int st_eval_note(hipStream_t stream, const float* rows, int R, const float* denom, double* acc, float* last) {
  if (R < 0 || (R > 0 && !rows) || !acc || !last || ((size_t)rows & 15) || ((size_t)last & 15) || ((size_t)acc & 7)) return -1;
  hipLaunchKernelGGL(eval_note_kernel, dim3(1), dim3(256), 0, stream, rows, R, denom, acc, last);
  ST_CHECK_LAUNCH();
  return 0;
}
