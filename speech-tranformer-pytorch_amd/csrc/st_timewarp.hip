// SpecAugment's time warp (gfx950): the plan launch that draws the warp pair (c, c') of every utterance next to its masks, and
// the two augmenting feature kernels of st_augment.hip with the warp applied before the masks - an output frame is the fp32
// blend of two neighbouring source frames (st_warp_pos, st_augment.cuh).  Same grids and access widths as their neighbours; an
// output chunk reads up to two source chunks.  The definition is spelled out in include/st_hip.h (st_specaug_plan_warp).
#include "st_augment.cuh"

namespace {

// Lanes 0 .. B * nm - 1: the masks, as specaug_plan_kernel (same counters, same key: the same bits); lanes B * nm .. B * nm + B - 1:
// the warp pair of one utterance each.
__global__ __launch_bounds__(256) void specaug_plan_warp_kernel(const unsigned* __restrict__ seed, unsigned salt,
                                                                const int* __restrict__ len, int B, int interval, int right,
                                                                int n_time, int time_width, int permille, int n_freq,
                                                                int freq_width, int mel_bins, int time_warp,
                                                                int* __restrict__ table, int* __restrict__ warp) {
  const int nm = n_time + n_freq, i = blockIdx.x * 256 + threadIdx.x;
  if (i >= B * nm + B) return;
  const uint32_t key = st_hash32(*seed + salt * 0x9e3779b9u);
  if (i >= B * nm) {
    const int b = i - B * nm, l = len[b], W = time_warp;
    const int n = l > 0 ? (l - 1) * interval + 1 + right : 0;
    int c = 0, cp = 0;
    if (W >= 1 && n >= 2 * W + 3) {
      const uint32_t wkey = st_hash32(key ^ ST_WARP_KEY);
      c = W + 1 + st_aug_pick(st_hash32((uint32_t)(b * 2) ^ wkey), n - 2 * W - 2);
      cp = c - W + st_aug_pick(st_hash32((uint32_t)(b * 2 + 1) ^ wkey), 2 * W + 1);
    }
    warp[2 * b] = c;
    warp[2 * b + 1] = cp;
    return;
  }
  const int b = i / nm, j = i - b * nm;
  const uint32_t ctr = (uint32_t)(b * 64 + j) * 2u;
  const uint32_t bits0 = st_hash32(ctr ^ key), bits1 = st_hash32((ctr + 1u) ^ key);
  int n, cap;
  if (j < n_time) {
    const int l = len[b];
    n = l > 0 ? (l - 1) * interval + 1 + right : 0;
    cap = min(time_width, (int)((long long)n * permille / 1000));
  } else {
    n = mel_bins;
    cap = min(freq_width, mel_bins);
  }
  const int width = st_aug_pick(bits0, cap + 1);
  table[2 * i] = st_aug_pick(bits1, n - width + 1);
  table[2 * i + 1] = width;
}

// pack_rows_aug_kernel (st_augment.hip) + warp: same grid, same 16-byte accesses, masks and the warp pair through LDS.  Row t,
// slot k shows OUTPUT frame u; its two source frames come from the stacked input itself: raw frame g stands in row
// ceil(g / interval), slot left - (that row's frame - g) (right == 0 and left >= interval - 1: the host checks).  An utterance
// with the pair (0, 0) takes pack_rows_aug_kernel's path, chunk for chunk.
__global__ __launch_bounds__(256) void pack_rows_warp_kernel(const float* __restrict__ x, int T, int F, int rpb, const int* off,
                                                             const int* len, bf16* __restrict__ out,
                                                             const int* __restrict__ table, const int* __restrict__ warp,
                                                             int n_time, int n_freq, int mel_bins, int left, int interval) {
  __shared__ int masks[2 * ST_AUG_MAX_MASKS + 2];
  const int b = blockIdx.z, cpr = F >> 2, nm = n_time + n_freq;
  st_aug_load(masks, table, b, nm);
  if ((int)threadIdx.x >= 254) masks[2 * ST_AUG_MAX_MASKS + threadIdx.x - 254] = warp[2 * b + threadIdx.x - 254];
  __syncthreads();
  const int cw = min(cpr, 256);
  const int t = blockIdx.y * rpb + (int)threadIdx.x / cw;
  const int l = len[b];
  if ((int)threadIdx.x >= rpb * cw || t >= l) return;
  const int t_raw = (l - 1) * interval + 1;
  const int wc = masks[2 * ST_AUG_MAX_MASKS], wcp = masks[2 * ST_AUG_MAX_MASKS + 1];
  const bool warped = st_warp_live(wc, wcp, t_raw);
  const float* xb = x + (size_t)b * T * F;
  bf16* dst = out + (size_t)(off[b] + t) * F;
  for (int c = (int)threadIdx.x % cw; c < cpr; c += cw) {
    const int k = 4 * c / mel_bins, f = 4 * c - k * mel_bins;
    const int u = st_stack_src(k, t * interval, left, 0, t_raw);
    f32x4 v = {0.f, 0.f, 0.f, 0.f};
    if (!(u >= 0 && st_aug_hit(masks, 0, n_time, u))) {
      if (u < 0 || !warped) {
        v = *reinterpret_cast<const f32x4*>(xb + (size_t)t * F + 4 * c);
      } else {
        int fr;
        const int g = st_warp_pos(u, t_raw, wc, wcp, &fr);
        const int r0 = (g + interval - 1) / interval;
        v = *reinterpret_cast<const f32x4*>(xb + (size_t)r0 * F + (left - (r0 * interval - g)) * mel_bins + f);
        if (fr) {
          const int r1 = (g + interval) / interval;
          const f32x4 w = *reinterpret_cast<const f32x4*>(xb + (size_t)r1 * F + (left - (r1 * interval - g - 1)) * mel_bins + f);
#pragma unroll
          for (int e = 0; e < 4; ++e) v[e] = st_warp_blend(v[e], w[e], fr);
        }
      }
#pragma unroll
      for (int e = 0; e < 4; ++e)
        if (st_aug_hit(masks, n_time, nm, f + e)) v[e] = 0.f;
    }
    bf16x4 o = {(bf16)v[0], (bf16)v[1], (bf16)v[2], (bf16)v[3]};
    *reinterpret_cast<bf16x4*>(dst + 4 * c) = o;
  }
}

// feat_stack_aug_kernel (st_augment.hip) + warp, applied after CMVN and before stacking: each of the two source frames is
// normalised (with the statistics of the unwarped utterance), then they are blended; masks in output coordinates.
__global__ __launch_bounds__(128) void feat_stack_warp_kernel(const float* __restrict__ x, int T, int F,
                                                              const int* __restrict__ in_len, const float* __restrict__ stats,
                                                              int left, int right, int interval,
                                                              const int* __restrict__ out_off, const int* __restrict__ out_len,
                                                              bf16* __restrict__ out, int ld, const int* __restrict__ table,
                                                              const int* __restrict__ warp, int n_time, int n_freq) {
  __shared__ int masks[2 * ST_AUG_MAX_MASKS];
  const int b = blockIdx.z, r = blockIdx.y, nm = n_time + n_freq;
  st_aug_load(masks, table, b, nm);
  __syncthreads();
  if (r >= out_len[b]) return;
  const int len = in_len[b], t = r * interval;
  const int wc = warp[2 * b], wcp = warp[2 * b + 1];          // (uniform over the workgroup: two scalar loads)
  const bool warped = st_warp_live(wc, wcp, len);
  const int blocks = 1 + left + right;
  const float* xb = x + (size_t)b * T * F;
  const float* st = stats ? stats + (size_t)b * 2 * (F + 1) : nullptr;
  const float cnt = st ? st[F] : 1.f;
  bf16* dst = out + (size_t)(out_off[b] + r) * ld;
  for (int c = threadIdx.x; c < blocks * F; c += blockDim.x) {
    const int k = c / F, f = c - k * F;
    const int u = st_stack_src(k, t, left, right, len);
    float v = 0.f;
    if (u >= 0 && !st_aug_hit(masks, 0, n_time, u) && !st_aug_hit(masks, n_time, nm, f)) {
      int fr = 0;
      const int g = warped ? st_warp_pos(u, len, wc, wcp, &fr) : u;
      v = xb[(size_t)g * F + f];
      float w = fr ? xb[(size_t)(g + 1) * F + f] : v;
      if (st) {
        const float mean = st[f] / cnt;
        const float var = st[F + 1 + f] / cnt - mean * mean;
        v = (v - mean) / sqrtf(var);
        w = (w - mean) / sqrtf(var);
      }
      if (fr) v = st_warp_blend(v, w, fr);
    }
    dst[c] = (bf16)v;
  }
}

bool bad_masks(int n_time, int n_freq) { return n_time < 0 || n_freq < 0 || n_time + n_freq > ST_AUG_MAX_MASKS; }

}  // namespace

extern "C" int st_specaug_plan_warp(hipStream_t stream, const unsigned* seed, unsigned salt, const int* len, int B, int interval,
                                    int right, int n_time, int time_width, int time_ratio_permille, int n_freq, int freq_width,
                                    int mel_bins, int time_warp, int* table, int* warp) {
  if (bad_masks(n_time, n_freq) || interval < 1 || right < 0 || time_width < 0 || freq_width < 0 || mel_bins < 1 ||
      time_ratio_permille < 0 || time_ratio_permille > 1000 || time_warp < 0 || time_warp > ST_WARP_MAX_FRAMES || !seed || !warp)
    return -1;
  if (B <= 0) return 0;
  if (B > (1 << 24)) return -1;      // (b * 64 + j) * 2 + d is a 32-bit counter
  const long long n = (long long)B * (n_time + n_freq + 1);
  hipLaunchKernelGGL(specaug_plan_warp_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, stream, seed, salt, len, B,
                     interval, right, n_time, time_width, time_ratio_permille, n_freq, freq_width, mel_bins, time_warp, table, warp);
  ST_CHECK_LAUNCH();
  return 0;
}

extern "C" int st_pack_rows_warp(hipStream_t stream, const float* x, int B, int T, int F, const int* off, const int* len,
                                 void* out, const int* table, const int* warp, int n_time, int n_freq, int mel_bins, int left,
                                 int right, int interval) {
  if (bad_masks(n_time, n_freq) || left < 0 || interval < 1 || mel_bins < 4 || (mel_bins & 3) ||
      (long long)mel_bins * (1 + left) != F || !warp)
    return -1;
  if (right != 0 || left < interval - 1) return -1;            // a raw frame must stand in a slot of the stacked input
  if ((long long)T * interval > ST_WARP_MAX_FRAMES) return -1;      // st_warp_pos computes in 32 bits
  if (B <= 0 || T <= 0) return 0;
  const int cpr = F >> 2, rpb = cpr >= 256 ? 1 : 256 / cpr;    // frames per workgroup, as st_pack_rows
  hipLaunchKernelGGL(pack_rows_warp_kernel, dim3(1, (T + rpb - 1) / rpb, B), dim3(256), 0, stream, x, T, F, rpb, off, len,
                     (bf16*)out, table, warp, n_time, n_freq, mel_bins, left, interval);
  ST_CHECK_LAUNCH();
  return 0;
}

extern "C" int st_feat_stack_warp(hipStream_t stream, const float* x, int B, int T, int F, const int* in_len,
                                  const float* stats, int left, int right, int interval, const int* out_off,
                                  const int* out_len, int max_out_len, void* out, int ld, const int* table, const int* warp,
                                  int n_time, int n_freq) {
  if (bad_masks(n_time, n_freq) || left < 0 || right < 0 || right > left || interval < 1 || F < 1 ||
      ld < (long long)F * (1 + left + right) || !warp)
    return -1;
  if (T > ST_WARP_MAX_FRAMES) return -1;      // st_warp_pos computes in 32 bits
  if (B <= 0 || T <= 0 || max_out_len <= 0) return 0;
  hipLaunchKernelGGL(feat_stack_warp_kernel, dim3(1, max_out_len, B), dim3(128), 0, stream, x, T, F, in_len, stats, left, right,
                     interval, out_off, out_len, (bf16*)out, ld, table, warp, n_time, n_freq);
  ST_CHECK_LAUNCH();
  return 0;
}
