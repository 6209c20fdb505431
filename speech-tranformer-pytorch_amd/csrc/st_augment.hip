// SpecAugment inside the training step (gfx950): the per-utterance mask plan drawn from the dropout seed in device memory, and
// the two feature kernels of st_misc.hip - the ragged pack and the feature front-end - with the masks applied on the way to
// bf16 rows.  HBM- and launch-bound like their neighbours: same grids, same access widths, the utterance's mask table (at most
// 64 pairs) in LDS.  The draw is spelled out in include/st_hip.h (st_specaug_plan).
#include "st_augment.cuh"

namespace {

// table[b][j] = (start, width) of mask j of utterance b; one lane per mask.
__global__ __launch_bounds__(256) void specaug_plan_kernel(const unsigned* __restrict__ seed, unsigned salt,
                                                           const int* __restrict__ len, int B, int interval, int right,
                                                           int n_time, int time_width, int permille, int n_freq,
                                                           int freq_width, int mel_bins, int* __restrict__ table) {
  const int nm = n_time + n_freq, i = blockIdx.x * 256 + threadIdx.x;
  if (i >= B * nm) return;
  const int b = i / nm, j = i - b * nm;
  const uint32_t key = st_hash32(*seed + salt * 0x9e3779b9u);
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

// pack_rows_kernel (st_misc.hip) + masks: same grid, same 16-byte loads; a float4 chunk lies inside one context slot
// (mel_bins % 4 == 0), so one source frame per chunk.  A chunk under a time mask is not loaded at all.
__global__ __launch_bounds__(256) void pack_rows_aug_kernel(const float* __restrict__ x, int T, int F, int rpb, const int* off,
                                                            const int* len, bf16* __restrict__ out,
                                                            const int* __restrict__ table, int n_time, int n_freq, int mel_bins,
                                                            int left, int right, int interval) {
  __shared__ int masks[2 * ST_AUG_MAX_MASKS];
  const int b = blockIdx.z, cpr = F >> 2, nm = n_time + n_freq;
  st_aug_load(masks, table, b, nm);
  __syncthreads();
  const int cw = min(cpr, 256);
  const int t = blockIdx.y * rpb + (int)threadIdx.x / cw;
  const int l = len[b];
  if ((int)threadIdx.x >= rpb * cw || t >= l) return;
  const int t_raw = (l - 1) * interval + 1 + right;
  const float* src = x + ((size_t)b * T + t) * F;
  bf16* dst = out + (size_t)(off[b] + t) * F;
  for (int c = (int)threadIdx.x % cw; c < cpr; c += cw) {
    const int k = 4 * c / mel_bins, f = 4 * c - k * mel_bins;
    const int frame = st_stack_src(k, t * interval, left, right, t_raw);
    f32x4 v = {0.f, 0.f, 0.f, 0.f};
    if (!(frame >= 0 && st_aug_hit(masks, 0, n_time, frame))) {
      v = *reinterpret_cast<const f32x4*>(src + 4 * c);
#pragma unroll
      for (int e = 0; e < 4; ++e)
        if (st_aug_hit(masks, n_time, nm, f + e)) v[e] = 0.f;
    }
    bf16x4 o = {(bf16)v[0], (bf16)v[1], (bf16)v[2], (bf16)v[3]};
    *reinterpret_cast<bf16x4*>(dst + 4 * c) = o;
  }
}

// feat_stack_kernel (st_misc.hip) + masks, applied after CMVN and before stacking: an element whose raw (frame, bin) lies
// under a mask is 0, whatever the statistics.
__global__ __launch_bounds__(128) void feat_stack_aug_kernel(const float* __restrict__ x, int T, int F,
                                                             const int* __restrict__ in_len, const float* __restrict__ stats,
                                                             int left, int right, int interval,
                                                             const int* __restrict__ out_off, const int* __restrict__ out_len,
                                                             bf16* __restrict__ out, int ld, const int* __restrict__ table,
                                                             int n_time, int n_freq) {
  __shared__ int masks[2 * ST_AUG_MAX_MASKS];
  const int b = blockIdx.z, r = blockIdx.y, nm = n_time + n_freq;
  st_aug_load(masks, table, b, nm);
  __syncthreads();
  if (r >= out_len[b]) return;
  const int len = in_len[b], t = r * interval;
  const int blocks = 1 + left + right;
  const float* xb = x + (size_t)b * T * F;
  const float* st = stats ? stats + (size_t)b * 2 * (F + 1) : nullptr;
  const float cnt = st ? st[F] : 1.f;
  bf16* dst = out + (size_t)(out_off[b] + r) * ld;
  for (int c = threadIdx.x; c < blocks * F; c += blockDim.x) {
    const int k = c / F, f = c - k * F;
    const int src = st_stack_src(k, t, left, right, len);
    float v = 0.f;
    if (src >= 0 && !st_aug_hit(masks, 0, n_time, src) && !st_aug_hit(masks, n_time, nm, f)) {
      v = xb[(size_t)src * F + f];
      if (st) {
        const float mean = st[f] / cnt;
        const float var = st[F + 1 + f] / cnt - mean * mean;
        v = (v - mean) / sqrtf(var);
      }
    }
    dst[c] = (bf16)v;
  }
}

bool bad_masks(int n_time, int n_freq) { return n_time < 0 || n_freq < 0 || n_time + n_freq > ST_AUG_MAX_MASKS; }

}  // namespace

extern "C" int st_specaug_plan(hipStream_t stream, const unsigned* seed, unsigned salt, const int* len, int B, int interval,
                               int right, int n_time, int time_width, int time_ratio_permille, int n_freq, int freq_width,
                               int mel_bins, int* table) {
  if (bad_masks(n_time, n_freq) || interval < 1 || right < 0 || time_width < 0 || freq_width < 0 || mel_bins < 1 ||
      time_ratio_permille < 0 || time_ratio_permille > 1000 || !seed)
    return -1;
  const long long n = (long long)B * (n_time + n_freq);
  if (B <= 0 || n == 0) return 0;
  if (B > (1 << 24)) return -1;      // (b * 64 + j) * 2 + d is a 32-bit counter
  hipLaunchKernelGGL(specaug_plan_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, stream, seed, salt, len, B, interval,
                     right, n_time, time_width, time_ratio_permille, n_freq, freq_width, mel_bins, table);
  ST_CHECK_LAUNCH();
  return 0;
}

extern "C" int st_pack_rows_aug(hipStream_t stream, const float* x, int B, int T, int F, const int* off, const int* len,
                                void* out, const int* table, int n_time, int n_freq, int mel_bins, int left, int right,
                                int interval) {
  if (bad_masks(n_time, n_freq) || left < 0 || right < 0 || right > left || interval < 1 || mel_bins < 4 || (mel_bins & 3) ||
      (long long)mel_bins * (1 + left + right) != F)
    return -1;
  if (B <= 0 || T <= 0) return 0;
  const int cpr = F >> 2, rpb = cpr >= 256 ? 1 : 256 / cpr;    // frames per workgroup, as st_pack_rows
  hipLaunchKernelGGL(pack_rows_aug_kernel, dim3(1, (T + rpb - 1) / rpb, B), dim3(256), 0, stream, x, T, F, rpb, off, len,
                     (bf16*)out, table, n_time, n_freq, mel_bins, left, right, interval);
  ST_CHECK_LAUNCH();
  return 0;
}

extern "C" int st_feat_stack_aug(hipStream_t stream, const float* x, int B, int T, int F, const int* in_len,
                                 const float* stats, int left, int right, int interval, const int* out_off,
                                 const int* out_len, int max_out_len, void* out, int ld, const int* table, int n_time,
                                 int n_freq) {
  if (bad_masks(n_time, n_freq) || left < 0 || right < 0 || right > left || interval < 1 || F < 1 ||
      ld < (long long)F * (1 + left + right))
    return -1;
  if (B <= 0 || T <= 0 || max_out_len <= 0) return 0;
  hipLaunchKernelGGL(feat_stack_aug_kernel, dim3(1, max_out_len, B), dim3(128), 0, stream, x, T, F, in_len, stats, left, right,
                     interval, out_off, out_len, (bf16*)out, ld, table, n_time, n_freq);
  ST_CHECK_LAUNCH();
  return 0;
}
