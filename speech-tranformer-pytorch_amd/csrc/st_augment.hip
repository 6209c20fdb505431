// The feature kernel family (gfx950): the feature front-end (CMVN, context stacking, subsampling -> bf16 rows), SpecAugment's
// per-utterance plan drawn from the dropout seed in device memory, and the ragged pack with the plan applied on the way to bf16
// rows.  ONE body per family, the variant a template argument: the plan with or without the warp lanes, the augmenting pack
// with or without the warp, the front-end plain / with masks / with masks and warp - an instantiation holds no code and no
// run-time test of a feature it does not have.  HBM- and launch-bound like their neighbours in st_misc.hip (the plain
// pack_rows_kernel stays there: it is the one the training step launches).  The utterance's mask table (at most 64 pairs) lives
// in LDS.  The draw, the warp's map and the order (warp, then masks) are spelled out in include/st_hip.h (st_specaug_plan,
// st_specaug_plan_warp); the helpers, the slot rule st_stack_src among them, in st_augment.cuh.
#include "st_augment.cuh"

namespace {

enum { FEAT_PLAIN, FEAT_MASKS, FEAT_WARP };      // feat_stack_kernel's variants: each one is its predecessor plus a feature

// Lanes 0 .. B * nm - 1: table[b][j] = (start, width) of mask j of utterance b.  WARP: lanes B * nm .. B * nm + B - 1 draw the warp
// pair of one utterance each (counters and key of their own: the masks do not depend on the warp).
template <bool WARP>
__global__ __launch_bounds__(256) void specaug_plan_kernel(const unsigned* __restrict__ seed, unsigned salt,
                                                           const int* __restrict__ len, int B, int interval, int right,
                                                           int n_time, int time_width, int permille, int n_freq,
                                                           int freq_width, int mel_bins, int time_warp, int* __restrict__ table,
                                                           int* __restrict__ warp) {
  const int nm = n_time + n_freq, i = blockIdx.x * 256 + threadIdx.x;
  if (i >= B * nm + (WARP ? B : 0)) return;
  const uint32_t key = st_hash32(*seed + salt * 0x9e3779b9u);
  if constexpr (WARP) {
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

// pack_rows_kernel (st_misc.hip) + masks: same grid, same 16-byte accesses; a float4 chunk lies inside one context slot
// (mel_bins % 4 == 0), so one source frame per chunk.  A chunk under a time mask is not loaded at all.
// WARP: the warp pair rides behind the masks in LDS.  Row t, slot k shows OUTPUT frame u; its two source frames come from the
// stacked input itself: raw frame g stands in row ceil(g / interval), slot left - (that row's frame - g) (right == 0 and
// left >= interval - 1: the host checks).  An utterance with the pair (0, 0) takes the plain path, chunk for chunk.
template <bool WARP>
__global__ __launch_bounds__(256) void pack_rows_aug_kernel(const float* __restrict__ x, int T, int F, int rpb, const int* off,
                                                            const int* len, bf16* __restrict__ out,
                                                            const int* __restrict__ table, int n_time, int n_freq, int mel_bins,
                                                            int left, int right, int interval, const int* __restrict__ warp) {
  __shared__ int masks[2 * ST_AUG_MAX_MASKS + (WARP ? 2 : 0)];
  const int b = blockIdx.z, cpr = F >> 2, nm = n_time + n_freq;
  st_aug_load(masks, table, b, nm);
  if constexpr (WARP)
    if ((int)threadIdx.x >= 254) masks[2 * ST_AUG_MAX_MASKS + threadIdx.x - 254] = warp[2 * b + threadIdx.x - 254];
  __syncthreads();
  const int cw = min(cpr, 256);
  const int t = blockIdx.y * rpb + (int)threadIdx.x / cw;
  const int l = len[b];
  if ((int)threadIdx.x >= rpb * cw || t >= l) return;
  const int rt = WARP ? 0 : right;
  const int t_raw = (l - 1) * interval + 1 + rt;
  const int wc = WARP ? masks[2 * ST_AUG_MAX_MASKS] : 0, wcp = WARP ? masks[2 * ST_AUG_MAX_MASKS + 1] : 0;
  const bool warped = WARP && st_warp_live(wc, wcp, t_raw);
  const float* xb = x + (size_t)b * T * F;                      // the utterance: where the warp finds its source rows
  // the row itself - one address, associated as each instantiation's predecessor had it: the other form costs the masked pack
  // 0.3 us at F = 320 (LABNOTES, "the feature kernel family") and the warping pack six instructions
  const float* src = WARP ? xb + (size_t)t * F : x + ((size_t)b * T + t) * F;
  bf16* dst = out + (size_t)(off[b] + t) * F;
  for (int c = (int)threadIdx.x % cw; c < cpr; c += cw) {
    const int k = 4 * c / mel_bins, f = 4 * c - k * mel_bins;
    const int u = st_stack_src(k, t * interval, left, rt, t_raw);
    f32x4 v = {0.f, 0.f, 0.f, 0.f};
    if (!(u >= 0 && st_aug_hit(masks, 0, n_time, u))) {
      if (u < 0 || !warped) {
        v = *reinterpret_cast<const f32x4*>(src + 4 * c);
      } else if constexpr (WARP) {
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

// Feature front-end (reference Dataset.py: cmvn :89-92, concat_frame :121-143, subsampling :145-153) fused with the ragged
// pack: raw padded fp32 features [B, T, F] -> bf16 row matrix [sum(out_len), F * (1 + left + right)] in the layout the encoder
// front-end GEMM consumes.  Output row r of utterance b stands at frame t = r * interval; slot k of the row shows frame
// st_stack_src(k, t).  stats: per-utterance Kaldi CMVN statistics [B, 2, F + 1] (sums | count, sums of squares) or null.  One
// workgroup per output row.
// FEAT_MASKS: applied after CMVN and before stacking - an element whose raw (frame, bin) lies under a mask is 0, whatever the
// statistics, and loads nothing.  FEAT_WARP: the warp comes before the masks (which live in output coordinates): each of the
// two source frames is normalised (with the statistics of the unwarped utterance), then they are blended.
template <int MODE>
__global__ __launch_bounds__(128) void feat_stack_kernel(const float* __restrict__ x, int T, int F,
                                                         const int* __restrict__ in_len, const float* __restrict__ stats,
                                                         int left, int right, int interval, const int* __restrict__ out_off,
                                                         const int* __restrict__ out_len, bf16* __restrict__ out, int ld,
                                                         const int* __restrict__ table, const int* __restrict__ warp,
                                                         int n_time, int n_freq) {
  constexpr bool MASKS = MODE != FEAT_PLAIN, WARP = MODE == FEAT_WARP;
  __shared__ int masks[2 * ST_AUG_MAX_MASKS];                   // (FEAT_PLAIN never touches it: no LDS is allocated)
  const int b = blockIdx.z, r = blockIdx.y, nm = n_time + n_freq;
  if constexpr (MASKS) {
    st_aug_load(masks, table, b, nm);
    __syncthreads();
  }
  if (r >= out_len[b]) return;
  const int len = in_len[b], t = r * interval;
  const int wc = WARP ? warp[2 * b] : 0, wcp = WARP ? warp[2 * b + 1] : 0;      // (uniform over the workgroup: two scalar loads)
  const bool warped = WARP && st_warp_live(wc, wcp, len);
  const int blocks = 1 + left + right;
  const float* xb = x + (size_t)b * T * F;
  const float* st = stats ? stats + (size_t)b * 2 * (F + 1) : nullptr;
  const float cnt = st ? st[F] : 1.f;
  bf16* dst = out + (size_t)(out_off[b] + r) * ld;
  for (int c = threadIdx.x; c < blocks * F; c += blockDim.x) {
    const int k = c / F, f = c - k * F;
    const int u = st_stack_src(k, t, left, right, len);         // frame this element shows (-1: stays zero)
    bool live = u >= 0;
    if constexpr (MASKS) live = live && !st_aug_hit(masks, 0, n_time, u) && !st_aug_hit(masks, n_time, nm, f);
    float v = 0.f;
    if (live) {
      int g = u, fr = 0;
      if constexpr (WARP)
        if (warped) g = st_warp_pos(u, len, wc, wcp, &fr);
      v = xb[(size_t)g * F + f];
      float w = v;
      if constexpr (WARP)
        if (fr) w = xb[(size_t)(g + 1) * F + f];
      if (st) {
        const float mean = st[f] / cnt;
        const float var = st[F + 1 + f] / cnt - mean * mean;
        v = (v - mean) / sqrtf(var);
        if constexpr (WARP) w = (w - mean) / sqrtf(var);
      }
      if constexpr (WARP)
        if (fr) v = st_warp_blend(v, w, fr);
    }
    dst[c] = (bf16)v;
  }
}

// ---- the checked launchers: one per family, every argument check once ------------------------------------------------------------
bool bad_masks(int n_time, int n_freq) { return n_time < 0 || n_freq < 0 || n_time + n_freq > ST_AUG_MAX_MASKS; }
bool bad_stacking(int left, int right, int interval) { return left < 0 || right < 0 || right > left || interval < 1; }

template <bool WARP>
int plan_launch(hipStream_t stream, const unsigned* seed, unsigned salt, const int* len, int B, int interval, int right, int n_time,
                int time_width, int permille, int n_freq, int freq_width, int mel_bins, int* table, int time_warp, int* warp) {
  if (bad_masks(n_time, n_freq) || interval < 1 || right < 0 || time_width < 0 || freq_width < 0 || mel_bins < 1 || permille < 0 ||
      permille > 1000 || !seed)
    return -1;
  if constexpr (WARP)
    if (time_warp < 0 || time_warp > ST_WARP_MAX_FRAMES || !warp) return -1;
  const long long n = (long long)B * (n_time + n_freq + (WARP ? 1 : 0));      // lanes
  if (B <= 0 || n == 0) return 0;
  if (B > (1 << 24)) return -1;      // (b * 64 + j) * 2 + d is a 32-bit counter
  hipLaunchKernelGGL(specaug_plan_kernel<WARP>, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, stream, seed, salt, len, B,
                     interval, right, n_time, time_width, permille, n_freq, freq_width, mel_bins, time_warp, table, warp);
  ST_CHECK_LAUNCH();
  return 0;
}

template <bool WARP>
int pack_launch(hipStream_t stream, const float* x, int B, int T, int F, const int* off, const int* len, void* out,
                const int* table, const int* warp, int n_time, int n_freq, int mel_bins, int left, int right, int interval) {
  if (bad_masks(n_time, n_freq) || bad_stacking(left, right, interval) || mel_bins < 4 || (mel_bins & 3) ||
      (long long)mel_bins * (1 + left + right) != F)
    return -1;
  if constexpr (WARP) {
    if (!warp || right != 0 || left < interval - 1) return -1;      // a raw frame must stand in a slot of the stacked input
    if ((long long)T * interval > ST_WARP_MAX_FRAMES) return -1;    // st_warp_pos computes in 32 bits
  }
  if (B <= 0 || T <= 0) return 0;
  const int cpr = F >> 2, rpb = cpr >= 256 ? 1 : 256 / cpr;    // frames per workgroup, as st_pack_rows
  hipLaunchKernelGGL(pack_rows_aug_kernel<WARP>, dim3(1, (T + rpb - 1) / rpb, B), dim3(256), 0, stream, x, T, F, rpb, off, len,
                     (bf16*)out, table, n_time, n_freq, mel_bins, left, right, interval, warp);
  ST_CHECK_LAUNCH();
  return 0;
}

template <int MODE>
int feat_launch(hipStream_t stream, const float* x, int B, int T, int F, const int* in_len, const float* stats, int left, int right,
                int interval, const int* out_off, const int* out_len, int max_out_len, void* out, int ld, const int* table,
                const int* warp, int n_time, int n_freq) {
  const bool empty = B <= 0 || T <= 0 || max_out_len <= 0;
  if constexpr (MODE == FEAT_PLAIN)
    if (empty) return 0;      // st_feat_stack takes an empty batch before it looks at the geometry
  if (bad_stacking(left, right, interval) || ld < (long long)F * (1 + left + right)) return -1;
  if constexpr (MODE != FEAT_PLAIN)
    if (bad_masks(n_time, n_freq) || F < 1) return -1;
  if constexpr (MODE == FEAT_WARP)
    if (!warp || T > ST_WARP_MAX_FRAMES) return -1;      // st_warp_pos computes in 32 bits
  if (empty) return 0;
  hipLaunchKernelGGL(feat_stack_kernel<MODE>, dim3(1, max_out_len, B), dim3(128), 0, stream, x, T, F, in_len, stats, left, right,
                     interval, out_off, out_len, (bf16*)out, ld, table, warp, n_time, n_freq);
  ST_CHECK_LAUNCH();
  return 0;
}

}  // namespace

extern "C" int st_specaug_plan(hipStream_t stream, const unsigned* seed, unsigned salt, const int* len, int B, int interval,
                               int right, int n_time, int time_width, int time_ratio_permille, int n_freq, int freq_width,
                               int mel_bins, int* table) {
  return plan_launch<false>(stream, seed, salt, len, B, interval, right, n_time, time_width, time_ratio_permille, n_freq, freq_width,
                            mel_bins, table, 0, nullptr);
}

extern "C" int st_specaug_plan_warp(hipStream_t stream, const unsigned* seed, unsigned salt, const int* len, int B, int interval,
                                    int right, int n_time, int time_width, int time_ratio_permille, int n_freq, int freq_width,
                                    int mel_bins, int time_warp, int* table, int* warp) {
  return plan_launch<true>(stream, seed, salt, len, B, interval, right, n_time, time_width, time_ratio_permille, n_freq, freq_width,
                           mel_bins, table, time_warp, warp);
}

extern "C" int st_pack_rows_aug(hipStream_t stream, const float* x, int B, int T, int F, const int* off, const int* len,
                                void* out, const int* table, int n_time, int n_freq, int mel_bins, int left, int right,
                                int interval) {
  return pack_launch<false>(stream, x, B, T, F, off, len, out, table, nullptr, n_time, n_freq, mel_bins, left, right, interval);
}

extern "C" int st_pack_rows_warp(hipStream_t stream, const float* x, int B, int T, int F, const int* off, const int* len,
                                 void* out, const int* table, const int* warp, int n_time, int n_freq, int mel_bins, int left,
                                 int right, int interval) {
  return pack_launch<true>(stream, x, B, T, F, off, len, out, table, warp, n_time, n_freq, mel_bins, left, right, interval);
}

extern "C" int st_feat_stack(hipStream_t stream, const float* x, int B, int T, int F, const int* in_len,
                             const float* stats, int left, int right, int interval, const int* out_off,
                             const int* out_len, int max_out_len, void* out, int ld) {
  return feat_launch<FEAT_PLAIN>(stream, x, B, T, F, in_len, stats, left, right, interval, out_off, out_len, max_out_len, out, ld,
                                 nullptr, nullptr, 0, 0);
}

extern "C" int st_feat_stack_aug(hipStream_t stream, const float* x, int B, int T, int F, const int* in_len,
                                 const float* stats, int left, int right, int interval, const int* out_off,
                                 const int* out_len, int max_out_len, void* out, int ld, const int* table, int n_time,
                                 int n_freq) {
  return feat_launch<FEAT_MASKS>(stream, x, B, T, F, in_len, stats, left, right, interval, out_off, out_len, max_out_len, out, ld,
                                 table, nullptr, n_time, n_freq);
}

extern "C" int st_feat_stack_warp(hipStream_t stream, const float* x, int B, int T, int F, const int* in_len,
                                  const float* stats, int left, int right, int interval, const int* out_off,
                                  const int* out_len, int max_out_len, void* out, int ld, const int* table, const int* warp,
                                  int n_time, int n_freq) {
  return feat_launch<FEAT_WARP>(stream, x, B, T, F, in_len, stats, left, right, interval, out_off, out_len, max_out_len, out, ld,
                                table, warp, n_time, n_freq);
}
