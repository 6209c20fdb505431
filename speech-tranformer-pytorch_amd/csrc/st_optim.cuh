// The two kernels of the optimizer update over the flat parameter arena, each ONE body for every form of its entry point
// (st_grad_norm, st_adam_clip in st_optim.hip, which instantiates them all): the plain forms, and the forms with a non-finite
// verdict (GUARD) and an averaged copy of the weights (AVG), chosen by which optional pointers the caller gives.  The template
// switches only ADD statements: with both off the arithmetic, its order and the stores are those of the plain kernels.
// A third switch, WIN, serves gradient accumulation over micro-batches (the win pointer of both entry points): the gradient
// buffer holds a SUM whose denominator win[0] is a device scalar known only after the last micro-batch; dividing by 1.0f is
// exact, so at win[0] == 1 the WIN forms compute what the forms without it compute, bit for bit.
#pragma once
#include "st_common.cuh"

#ifndef ST_ADAM_SC1
#define ST_ADAM_SC1 0
#endif

namespace {

// Global-norm gradient clipping + Adam over the flat parameter arena, one pass (train.py:45-46: clip_grad_norm_ then
// ScheduledOptim.step; Adam(betas, eps) of transformer/Optim.py).  Same arithmetic as torch's fused Adam kernel
// (bias corrections from the step count, denom = sqrt(v) / sqrt(bc2) + eps, p -= lr / bc1 * m / denom); the clipped
// gradient is written back, as clip_grad_norm_ leaves it.  lr / step / gnorm are device scalars, so a captured graph
// replays with the current learning rate.
// found_inf / avg: GUARD - a non-zero *found_inf makes the whole launch a no-op, nothing is written; AVG - the exponential
// moving average of the parameters, avg += w * (p_new - avg) in the same pass, w = 1 - d, d = decay or (decay_warmup)
// min(decay, (1 + step) / (10 + step)).  Two switches, so that the guard alone streams exactly what the plain kernel streams.
// win: WIN - the coefficient is also divided by win[0] (still ONE scalar, formed before the loop), and ZEROS are
// stored to g where the clipped gradient would go: the update is the next window's zero_grad at no extra traffic.  Under WIN a
// non-zero *found_inf still clears g (the skipped window's sum must not leak into the next one) and writes nothing else.
template <bool GUARD, bool AVG, bool WIN = false>
__global__ __launch_bounds__(256) void adam_clip_kernel(float* __restrict__ p, float* __restrict__ g, float* __restrict__ m,
                                                        float* __restrict__ v, size_t n4, const float* lr_p,
                                                        const float* step_p, const float* gnorm_p, float max_norm,
                                                        float beta1, float beta2, float eps, float grad_scale,
                                                        const float* found_inf, float* __restrict__ avg, float decay,
                                                        int decay_warmup, const float* win) {
  if (GUARD && *found_inf != 0.0f) {      // (uniform over the grid: every workgroup reads the same scalar)
    if (WIN) {
      const f32x4 zero = {0.f, 0.f, 0.f, 0.f};
      for (size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x; i < n4; i += (size_t)gridDim.x * blockDim.x)
        store16<ST_ADAM_SC1>(g + i * 4, zero);
    }
    return;
  }
  const float lr = *lr_p, step = *step_p;
  // grad_scale: what the buffer still has to be multiplied by to be THE gradient (1 / world behind a summing all-reduce:
  // the rank average costs no pass of its own); *gnorm_p is the norm of the scaled gradient (st_grad_norm's grad_scale)
  float coef = (gnorm_p ? fminf(max_norm / (*gnorm_p + 1e-6f), 1.0f) : 1.0f) * grad_scale;
  if (WIN) coef = coef / *win;      // the window's denominator; *gnorm_p is the norm of the DIVIDED gradient (st_grad_norm with win)
  const float bc1 = 1.0f - powf(beta1, step), bc2 = 1.0f - powf(beta2, step);
  const float step_size = lr / bc1, bc2_sqrt = sqrtf(bc2);
  float w = 0.0f;
  if (AVG) w = 1.0f - (decay_warmup ? fminf(decay, (1.0f + step) / (10.0f + step)) : decay);
  const bool averaging = AVG && w != 0.0f;          // (w == 0: the average keeps its bits, -0.0 included)
  for (size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x; i < n4; i += (size_t)gridDim.x * blockDim.x) {
    f32x4 gg = *reinterpret_cast<const f32x4*>(g + i * 4);
    f32x4 mm = *reinterpret_cast<const f32x4*>(m + i * 4);
    f32x4 vv = *reinterpret_cast<const f32x4*>(v + i * 4);
    f32x4 pp = *reinterpret_cast<const f32x4*>(p + i * 4);
    f32x4 aa = {0.f, 0.f, 0.f, 0.f};
    if (averaging) aa = *reinterpret_cast<const f32x4*>(avg + i * 4);
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      const float ge = gg[e] * coef;
      gg[e] = WIN ? 0.0f : ge;
      mm[e] = mm[e] + (1.0f - beta1) * (ge - mm[e]);          // lerp(m, g, 1 - beta1), as torch
      vv[e] = beta2 * vv[e] + (1.0f - beta2) * ge * ge;
      const float denom = sqrtf(vv[e]) / bc2_sqrt + eps;
      pp[e] -= step_size * mm[e] / denom;
    }
    store16<ST_ADAM_SC1>(g + i * 4, gg);
    store16<ST_ADAM_SC1>(m + i * 4, mm);
    store16<ST_ADAM_SC1>(v + i * 4, vv);
    store16<ST_ADAM_SC1>(p + i * 4, pp);
    if (averaging) {
#pragma unroll
      for (int e = 0; e < 4; ++e) aa[e] = aa[e] + w * (pp[e] - aa[e]);
      store16<ST_ADAM_SC1>(avg + i * 4, aa);
    }
  }
}

// Global L2 norm of the flat gradient buffer (clip_grad_norm_'s total_norm, train.py:45) as ONE launch: every workgroup
// leaves the sum of squares of its grid-stride slice in `partial`, takes a ticket, and the last one adds the partials up (in
// index order: the result does not depend on the arrival order), writes *gnorm, advances the optimiser's step counter
// (*step += 1, optional) and resets the ticket for the next launch.  Replaces torch.linalg.vector_norm (52 MB at 2.6 TB/s
// plus a memset) and the separate step increment: three graph nodes -> one.
// GUARD (guard given): the same single writer also leaves the verdict - a non-finite norm does not advance the step,
// sets guard[0] and counts up guard[1]; a finite one clears guard[0].
// WIN (win given): the norm is divided by the window's denominator win[0], and a denominator <= 0 is a bad verdict too.
template <bool GUARD, bool WIN = false>
__global__ __launch_bounds__(1024) void grad_norm_kernel(const float* __restrict__ g, size_t n4, float* partial, unsigned* ticket,
                                                        float* __restrict__ gnorm, float* step, float grad_scale, float* guard,
                                                        const float* win) {
  __shared__ float red[16];      // 1024 threads x four 16-byte loads in flight = 64 KB per workgroup, 16 MB over the chip
                                 // (256 threads: 4 MB in flight = ~2 TB/s at ~2 us memory latency: 18 us for 52 MB)
  __shared__ bool last;
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
  float acc[4] = {0.f, 0.f, 0.f, 0.f};
  const size_t stride = (size_t)gridDim.x * 1024;
  size_t i = blockIdx.x * (size_t)1024 + tid;
  for (; i + 3 * stride < n4; i += 4 * stride) {      // four 16-byte loads in flight per thread
    f32x4 v[4];
#pragma unroll
    for (int u = 0; u < 4; ++u) v[u] = *reinterpret_cast<const f32x4*>(g + (i + u * stride) * 4);
#pragma unroll
    for (int u = 0; u < 4; ++u)
#pragma unroll
      for (int e = 0; e < 4; ++e) acc[e] = fmaf(v[u][e], v[u][e], acc[e]);
  }
  for (; i < n4; i += stride) {
    const f32x4 v = *reinterpret_cast<const f32x4*>(g + i * 4);
#pragma unroll
    for (int e = 0; e < 4; ++e) acc[e] = fmaf(v[e], v[e], acc[e]);
  }
  float s = (acc[0] + acc[1]) + (acc[2] + acc[3]);
#pragma unroll
  for (int o = 32; o; o >>= 1) s += __shfl_xor(s, o, 64);
  if (lane == 0) red[wave] = s;
  __syncthreads();
  if (tid == 0) {
    // write-through store, acknowledged before the ticket is drawn; the last workgroup reads with device-scope loads.  No
    // fence: an agent-scope release writes the whole L2 back (tools/dev/merge_probe.hip: +60-80 us on 512 workgroups)
    float bs = 0.f;
#pragma unroll
    for (int w = 0; w < 16; ++w) bs += red[w];
    __hip_atomic_store(partial + blockIdx.x, bs, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
    ST_PUBLISH_FENCE();
    __builtin_amdgcn_s_waitcnt(0);
    last = __hip_atomic_fetch_add(ticket, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) == gridDim.x - 1;
  }
  __syncthreads();
  if (!last) return;
  ST_MERGER_FENCE();
  double t = 0.0;
  if (tid < 256)
    for (int i = tid; i < (int)gridDim.x; i += 256) t += (double)__hip_atomic_load(partial + i, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  __shared__ double redd[256];
  if (tid < 256) redd[tid] = t;
  __syncthreads();
  for (int o = 128; o; o >>= 1) {
    if (tid < o) redd[tid] += redd[tid + o];
    __syncthreads();
  }
  if (tid == 0) {
    float norm = (float)sqrt(redd[0]) * grad_scale;      // ||grad_scale * g||
    if (WIN) norm = norm / *win;
    *gnorm = norm;
    if (GUARD) {
      // NaN and +-inf elements, and a workgroup's fp32 sum of squares that overflowed, all arrive here as a NaN or inf norm
      const bool bad = !(fabsf(norm) <= 3.402823466e38f) || (WIN && !(*win > 0.0f));
      if (!bad) *step += 1.0f;
      guard[0] = bad ? 1.0f : 0.0f;
      if (bad) guard[1] += 1.0f;
    } else if (step) {
      *step += 1.0f;
    }
    __hip_atomic_store(ticket, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  }
}

}  // namespace
