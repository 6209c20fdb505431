// Helpers of the feature kernel family (st_augment.hip): where a stacked row's context slot comes from, whether a raw
// (frame, bin) lies under a mask of the utterance's table, and where the time warp sends an output frame.
#pragma once
#include "st_common.cuh"

#define ST_AUG_MAX_MASKS 64      // time + frequency masks of one utterance: the table one workgroup keeps in LDS

// THE slot rule: raw frame that feeds context slot k of the stacked row standing at raw frame t, or -1 when the slot stays zero
// (reference Dataset.py:121-143: middle, then left contexts, then right contexts, in closed form).  Slot `left` is the frame itself, slot
// left - i - 1 the frame i + 1 to the left, slot RIGHT + i + 1 (the reference indexes the right blocks with the right width,
// :139-141) the frame i + 1 to the right; a later rule overwrites an earlier one, a rule whose frame does not exist writes nothing.
__device__ __forceinline__ int st_stack_src(int k, int t, int left, int right, int len) {
  int src = -1;
  if (k == left) src = t;
  if (k < left && t >= left - k) src = t - (left - k);
  if (k > right && k <= 2 * right && t + (k - right) < len) src = t + (k - right);
  return src;
}

// pick(bits, n): uniform in [0, n) from 32 random bits, integers only
__device__ __forceinline__ int st_aug_pick(uint32_t bits, int n) { return (int)(((uint64_t)bits * (uint64_t)(uint32_t)n) >> 32); }

// The utterance's mask table, (start, width) pairs, copied into LDS by the first 2 * n lanes (the caller synchronises).
__device__ __forceinline__ void st_aug_load(int* lds, const int* __restrict__ table, int b, int n) {
  if ((int)threadIdx.x < 2 * n) lds[threadIdx.x] = table[(size_t)b * 2 * n + threadIdx.x];
}
// v in [start, start + width) for one of the pairs lo .. hi - 1 (one unsigned compare per pair; width 0 never matches)
__device__ __forceinline__ bool st_aug_hit(const int* lds, int lo, int hi, int v) {
  bool hit = false;
  for (int j = lo; j < hi; ++j) hit |= (unsigned)(v - lds[2 * j]) < (unsigned)lds[2 * j + 1];
  return hit;
}

// ---- the time warp (include/st_hip.h, st_specaug_plan_warp) ------------------------------------------------------------------
#define ST_WARP_KEY 0x77617270u          // "warp": the warp draw's key is hash32(key ^ ST_WARP_KEY), its counters are its own
#define ST_WARP_MAX_FRAMES 32767         // raw frames of an utterance up to which st_warp_pos is exact in 32 bits (the hosts refuse more)

// Is (c, c') a warp of an utterance of n raw frames?  (0, 0) is the plan's "not warped"; any pair outside 1 .. n - 2 is treated
// the same way, so a table that was not planned for these lengths cannot send a read outside the utterance.
__device__ __forceinline__ bool st_warp_live(int c, int cp, int n) { return c >= 1 && cp >= 1 && c <= n - 2 && cp <= n - 2; }

// Source position of output frame u (0 <= u < n) under the live warp (c, c'): the piecewise linear map with s(0) = 0, s(c') = c,
// s(n - 1) = n - 1 in 16.16 fixed point, floor(num * 65536 / den) -> frame g (returned) and fraction *fr.  32-bit arithmetic:
// num <= (n - 1)^2 < 2^30 and (num mod den) << 16 < 2^31 for n <= ST_WARP_MAX_FRAMES.  g <= n - 1, and g + 1 <= n - 1 when *fr > 0.
__device__ __forceinline__ int st_warp_pos(int u, int n, int c, int cp, int* fr) {
  uint32_t num, den;
  if (u < cp) {
    num = (uint32_t)u * (uint32_t)c;
    den = (uint32_t)cp;
  } else {
    num = (uint32_t)c * (uint32_t)(n - 1 - cp) + (uint32_t)(u - cp) * (uint32_t)(n - 1 - c);
    den = (uint32_t)(n - 1 - cp);
  }
  const uint32_t g = num / den;
  *fr = (int)(((num - g * den) << 16) / den);
  return (int)g;
}

// a + (fr / 65536) * (b - a), every operation rounded to fp32 on its own (no contraction: a host can mirror it bit for bit)
__device__ __forceinline__ float st_warp_blend(float a, float b, int fr) {
  return __fadd_rn(a, __fmul_rn((float)fr * (1.f / 65536.f), __fsub_rn(b, a)));
}
