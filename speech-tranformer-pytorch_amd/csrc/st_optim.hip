// The optimizer update (gfx950): st_grad_norm and st_adam_clip - every instantiation of the two bodies of st_optim.cuh, chosen by
// which optional pointers are given (a guard against non-finite gradients, an averaged copy of the weights, a gradient-
// accumulation window) - and the in-place exchange of two flat buffers that puts the averaged weights under the model.  HBM
// streams like their neighbours in st_misc.hip: 16-byte accesses.  Gradient accumulation over micro-batches adds the two
// one-thread launches that keep the window's state (denominator, loss sums, count) in device memory: st_accum_note,
// st_window_close.
#include "st_optim.cuh"

namespace {

// a <-> b, grid-stride, two 16-byte loads and two 16-byte stores per element
__global__ __launch_bounds__(256) void swap_kernel(float* __restrict__ a, float* __restrict__ b, size_t n4) {
  for (size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x; i < n4; i += (size_t)gridDim.x * blockDim.x) {
    const f32x4 x = *reinterpret_cast<const f32x4*>(a + i * 4);
    const f32x4 y = *reinterpret_cast<const f32x4*>(b + i * 4);
    *reinterpret_cast<f32x4*>(a + i * 4) = y;
    *reinterpret_cast<f32x4*>(b + i * 4) = x;
  }
}

// One micro-batch noted in the window (see st_accum_note in include/st_hip.h); one thread, plain stores.
__global__ void accum_note_kernel(const float* __restrict__ sums, const float* d, float* __restrict__ win, float* __restrict__ out) {
  if (threadIdx.x != 0 || blockIdx.x != 0) return;
  const float s = sums[0], n = sums[1];
  win[1] += s;
  if (n > 0.0f) win[2] += sums[3] * n;      // (no token: sums[3] is 0 / 0, and the sum of no NLL is 0)
  win[3] += 1.0f;
  if (d) {
    const float dd = *d;
    win[0] += dd;
    out[0] = s / dd;
  } else {
    win[0] = 1.0f;
    out[0] = s;
  }
}

__global__ void window_close_kernel(float* __restrict__ win, float* __restrict__ out) {
  if (threadIdx.x != 0 || blockIdx.x != 0) return;
  const float d = win[0];
  out[0] = win[1] / d;
  out[1] = win[2] / d;
  out[2] = d;
  out[3] = win[3];
  win[0] = 0.0f;
  win[1] = 0.0f;
  win[2] = 0.0f;
  win[3] = 0.0f;
}

}  // namespace

extern "C" int st_grad_norm_blocks(void) { return 1024; }

extern "C" int st_grad_norm(hipStream_t stream, const float* g, long long n, float* scratch, float* gnorm, float* step,
                            float grad_scale, float* guard, const float* win) {
  // scratch: st_grad_norm_blocks() + 1 floats, the last one (the ticket) zero before the first call.  One grid for all four
  // forms, so the same partial sums and the same merge order; guard NULL = no verdict (step, if given, always advances)
  if (n <= 0 || (n & 3) || !g || !scratch || !gnorm || (!step && (guard || win))) return -1;
  const size_t n4 = (size_t)n / 4;
  // one workgroup per CU: the tickets are same-address atomics, which serialise (~15 ns each: 1024 workgroups spent 15 us on
  // them, ce_fwd's 1,200 once 43 us)
  int blocks = (int)((n4 + 1023) / 1024);
  if (blocks > 256) blocks = 256;
#define ST_NORM_LAUNCH(...)                                                                                          \
  hipLaunchKernelGGL((grad_norm_kernel<__VA_ARGS__>), dim3(blocks), dim3(1024), 0, stream, g, n4, scratch,                \
                     reinterpret_cast<unsigned*>(scratch + 1024), gnorm, step, grad_scale, guard, win)
  if (win) {
    if (guard) ST_NORM_LAUNCH(true, true);
    else ST_NORM_LAUNCH(false, true);
  } else {
    if (guard) ST_NORM_LAUNCH(true);
    else ST_NORM_LAUNCH(false);
  }
#undef ST_NORM_LAUNCH
  ST_CHECK_LAUNCH();
  return 0;
}

extern "C" int st_adam_clip(hipStream_t stream, long long n, float* p, float* g, float* m, float* v, const float* lr,
                            const float* step, const float* gnorm, float max_norm, float beta1, float beta2, float eps,
                            float grad_scale, const float* found_inf, float* avg, float decay, int decay_warmup,
                            const float* win) {
  if (n <= 0) return 0;
  if ((n & 3) || !p || !g || !m || !v || !lr || !step) return -1;
  if (avg && !(decay >= 0.0f && decay <= 1.0f)) return -1;
  const size_t n4 = (size_t)n / 4;
  int blocks = (int)((n4 + 255) / 256);
  if (blocks > 4096) blocks = 4096;
#define ST_ADAM_LAUNCH(GUARD, AVG, WIN)                                                                                      \
  hipLaunchKernelGGL((adam_clip_kernel<GUARD, AVG, WIN>), dim3(blocks), dim3(256), 0, stream, p, g, m, v, n4, lr, step, gnorm, \
                     max_norm, beta1, beta2, eps, grad_scale, found_inf, avg, decay, decay_warmup, win)
  if (win) {
    if (found_inf && avg) ST_ADAM_LAUNCH(true, true, true);
    else if (found_inf) ST_ADAM_LAUNCH(true, false, true);
    else if (avg) ST_ADAM_LAUNCH(false, true, true);
    else ST_ADAM_LAUNCH(false, false, true);
  } else {
    if (found_inf && avg) ST_ADAM_LAUNCH(true, true, false);
    else if (found_inf) ST_ADAM_LAUNCH(true, false, false);
    else if (avg) ST_ADAM_LAUNCH(false, true, false);
    else ST_ADAM_LAUNCH(false, false, false);
  }
#undef ST_ADAM_LAUNCH
  ST_CHECK_LAUNCH();
  return 0;
}

extern "C" int st_accum_note(hipStream_t stream, const float* sums, const float* d, float* win, float* out) {
  if (!sums || !win || !out) return -1;
  hipLaunchKernelGGL(accum_note_kernel, dim3(1), dim3(64), 0, stream, sums, d, win, out);
  ST_CHECK_LAUNCH();
  return 0;
}

extern "C" int st_window_close(hipStream_t stream, float* win, float* out) {
  if (!win || !out) return -1;
  hipLaunchKernelGGL(window_close_kernel, dim3(1), dim3(64), 0, stream, win, out);
  ST_CHECK_LAUNCH();
  return 0;
}

extern "C" int st_swap_f32(hipStream_t stream, float* a, float* b, long long n) {
  if (n <= 0) return 0;
  if ((n & 3) || !a || !b || ((size_t)a & 15) || ((size_t)b & 15)) return -1;
  const float *lo = a < b ? a : b, *hi = a < b ? b : a;
  if (lo + n > hi) return -1;      // overlapping (or equal) buffers
  const size_t n4 = (size_t)n / 4;
  int blocks = (int)((n4 + 255) / 256);
  if (blocks > 4096) blocks = 4096;
  hipLaunchKernelGGL(swap_kernel, dim3(blocks), dim3(256), 0, stream, a, b, n4);
  ST_CHECK_LAUNCH();
  return 0;
}
