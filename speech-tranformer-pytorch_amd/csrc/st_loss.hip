// Label-smoothed cross-entropy over ragged logits rows (gfx950): st_ce_smooth_fwd / st_ce_smooth_bwd of include/st_hip.h.
// transformer/Loss.py:LabelSmoothingLoss (the recipe's label smoothing 0.1, with the reference's PAD-column quirk and its
// division by all rows) and nn.CrossEntropyLoss(label_smoothing = e) as the SAME two-launch forward / one-launch backward
// the plain loss runs (st_ce_fwd / st_ce_bwd, st_misc.hip): these entry points launch the <true> instantiation of the
// kernels in st_ce.cuh.  Bandwidth kernels over R x V fp32: the forward reads the logits once, the backward reads them
// again and writes R x ldd bf16.
#include "st_hip.h"
#include "st_ce.cuh"

extern "C" int st_ce_smooth_fwd(hipStream_t stream, const float* logits, int ldl, int R, int V, const long long* target,
                                const long long* target_index, int ignore_index, float confidence, float smooth, int zero_col,
                                const float* denom, float* lse, float* row_loss, float* sums) {
  if (R <= 0) return 0;
  if (!logits || !target || !lse || !row_loss || !sums || V <= 0 || ldl < V || zero_col >= V) return -1;
  const CeSmooth sp{confidence, smooth, zero_col < 0 ? -1 : zero_col, denom};
  hipLaunchKernelGGL(ce_fwd_kernel<true>, dim3(R), dim3(256), 0, stream, logits, ldl, V, target, target_index, ignore_index, lse,
                     row_loss, sp);
  hipLaunchKernelGGL(ce_sum_kernel<true>, dim3(1), dim3(256), 0, stream, row_loss, target, target_index, ignore_index, R, sums,
                     logits, ldl, lse, sp);
  ST_CHECK_LAUNCH();
  return 0;
}

extern "C" int st_ce_smooth_bwd(hipStream_t stream, const float* logits, int ldl, int R, int V, const long long* target,
                                const long long* target_index, int ignore_index, float confidence, float smooth, int zero_col,
                                const float* denom, const float* lse, const float* sums, const float* grad_out, void* dlogits,
                                int ldd) {
  if (R <= 0) return 0;
  if (!logits || !target || !lse || !sums || !grad_out || !dlogits || V <= 0 || ldl < V || ldd < V || (ldd & 7) || zero_col >= V)
    return -1;
  const CeSmooth sp{confidence, smooth, zero_col < 0 ? -1 : zero_col, denom};
  hipLaunchKernelGGL(ce_bwd_kernel<true>, dim3(R), dim3(256), 0, stream, logits, ldl, V, target, target_index, ignore_index, lse,
                     sums, grad_out, (bf16*)dlogits, ldd, sp);
  ST_CHECK_LAUNCH();
  return 0;
}
