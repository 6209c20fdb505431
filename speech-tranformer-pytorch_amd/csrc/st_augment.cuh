// SpecAugment helpers shared by the kernels of st_augment.hip: where a stacked row's context slot comes from, and whether a
// raw (frame, bin) lies under a mask of the utterance's table.
#pragma once
#include "st_common.cuh"

#define ST_AUG_MAX_MASKS 64      // time + frequency masks of one utterance: the table one workgroup keeps in LDS

// Raw frame that feeds context slot k of the stacked row standing at raw frame t, or -1 when the slot stays zero: the rule of
// feat_stack_kernel (st_misc.hip; reference Dataset.py:121-143) in closed form.  Slot `left` is the frame itself, slot
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
