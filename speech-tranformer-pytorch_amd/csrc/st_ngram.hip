// Back-off n-gram language model for shallow fusion (st_amd/ngram.py): the score of every pre-beam candidate, the histories of
// the hypotheses a beam step chose, and teacher-forced scores of token lists.
//
// The model is a trie keyed in REVERSE (st_amd.ngram.DeviceTrie): the node of the n-gram (w_1 .. w_m) is reached by w_m,
// w_{m-1}, .., w_1.  Node v < V is the unigram of token v (logp = +inf: the token has no unigram); the children of a node are
// the consecutive nodes child_lo[node] .. child_lo[node + 1] - 1, sorted by tok.  The table is suffix-closed (completed on the
// host), so "walk until a child is missing" finds the longest stored n-gram.
//
// Score of candidate c after the history h_k .. h_1 (h_1 the most recent, k <= N - 1 valid tokens):
//   bo_j  = back-off of the node reached by h_1, .., h_j (0 from the first missing child on)          - one walk per history
//   m     = depth reached by c, h_1, h_2, ..; logp_m = that node's logp (no unigram: oov_logp, m = 1)  - one walk per candidate
//   score = logp_m + bo_m + bo_{m+1} + .. + bo_k                           fp32, in that order, additions only
// so a NumPy float32 emulation (tests/_emul_ngram.py) is bit-equal.
#include "st_ngram.cuh"                                    // Trie, find_child, walk_history, score_candidate, trie_ok

namespace {

// ---- st_ngram_score: one wave (= one workgroup) per hypothesis row, lane j = candidate j.  The row index is the workgroup's,
//      so the history and its back-off walk are uniform: one walk per wave, through the scalar unit
__global__ __launch_bounds__(64) void ngram_score_kernel(Trie T, int H, const int* __restrict__ hist, const int* __restrict__ cand, int K,
                                                         int beam, const unsigned char* __restrict__ done, int eos, float scale,
                                                         float bias, float* __restrict__ lm_out, float* __restrict__ lp) {
  const int i = blockIdx.x, lane = threadIdx.x;
  if (done && done[i / beam]) return;                      // a finished utterance: nothing is read or written
  int h[MAX_H];
#pragma unroll
  for (int j = 0; j < MAX_H; ++j) h[j] = j < H ? hist[(size_t)i * H + (H - 1 - j)] : -1;
  const size_t at = (size_t)i * K + lane;
  if (h[0] >= 0 && h[0] == eos) {                          // frozen (emitted EOS): raw 0, lp untouched
    if (lm_out && lane < K) lm_out[at] = 0.f;
    return;
  }
  float bo[MAX_H];
  const int k = walk_history(T, h, H, bo);                 // (uniform: before the lanes part ways)
  if (lane >= K) return;
  const float lm = score_candidate(T, cand[at], h, k, bo);
  if (lm_out) lm_out[at] = lm;
  if (lp) lp[at] += scale > 0.f ? fmaf(scale, lm, bias) : bias;   // (one rounding; -inf stays -inf; scale = 0 never meets an infinite lm)
}

// ---- st_ngram_advance: one workgroup per utterance; thread (s, j) reads slot j + 1 of its parent's history (or the chosen
//      token) BEFORE the barrier, writes after it: two children of one parent and overwritten parents are both right
__global__ __launch_bounds__(256) void ngram_advance_kernel(int* __restrict__ hist, int H, const long long* __restrict__ order,
                                                            const long long* __restrict__ tokens,
                                                            const unsigned char* __restrict__ done, int eos, int beam) {
  const int b = blockIdx.x, tid = threadIdx.x, base = b * beam;
  if (done && done[b]) return;
  const int s = tid / H, j = tid % H;
  int v = 0;
  const bool mine = s < beam;
  if (mine) {
    long long p = order[base + s];
    if (p < base || p >= base + beam) p = base + s;        // (never a row of another utterance)
    const int* ph = hist + (size_t)p * H;
    const bool frozen = ph[H - 1] >= 0 && ph[H - 1] == eos;
    v = frozen ? ph[j] : (j + 1 < H ? ph[j + 1] : (int)tokens[base + s]);
  }
  __syncthreads();
  if (mine) hist[(size_t)(base + s) * H + j] = v;
}

// ---- st_ngram_score_seq: one thread per (list, position): log p(tokens[m][t] | BOS, tokens[m][:t])
__global__ __launch_bounds__(256) void ngram_score_seq_kernel(Trie T, int H, const int* __restrict__ tokens, const int* __restrict__ lens,
                                                              int M, int L_cap, int bos, float* __restrict__ out) {
  const long long e = (long long)blockIdx.x * 256 + threadIdx.x;
  if (e >= (long long)M * L_cap) return;
  const int m = (int)(e / L_cap), t = (int)(e % L_cap);
  if (t >= min(lens[m], L_cap)) {
    out[e] = 0.f;
    return;
  }
  const int* row = tokens + (size_t)m * L_cap;
  int h[MAX_H];
#pragma unroll
  for (int j = 0; j < MAX_H; ++j) h[j] = j >= H ? -1 : (t - 1 - j >= 0 ? row[t - 1 - j] : (t - 1 - j == -1 ? bos : -1));
  float bo[MAX_H];
  const int k = walk_history(T, h, H, bo);
  out[e] = score_candidate(T, row[t], h, k, bo);
}

}  // namespace

extern "C" int st_ngram_score(hipStream_t stream, const int* child_lo, const int* tok, const float* logp, const float* bo, int nodes,
                              int V, int order, float oov_logp, const int* hist, const int* cand, int n, int K, int beam,
                              const unsigned char* done, int eos, float scale, float bias, float* lm_out, float* lp) {
  if (n <= 0) return 0;
  if (!trie_ok(child_lo, tok, logp, bo, nodes, V, order) || !hist || !cand || K <= 0 || K > 64 || beam <= 0 || (n % beam) ||
      !(scale >= 0.f) || !(bias == bias) || !(oov_logp <= 0.f))
    return -1;
  const Trie T{child_lo, tok, logp, bo, nodes, V, oov_logp};
  hipLaunchKernelGGL(ngram_score_kernel, dim3(n), dim3(64), 0, stream, T, order - 1, hist, cand, K, beam, done, eos, scale, bias,
                     lm_out, lp);
  ST_CHECK_LAUNCH();
  return 0;
}

extern "C" int st_ngram_advance(hipStream_t stream, int* hist, int order, const long long* parent, const long long* tokens,
                                const unsigned char* done, int eos, int B, int beam) {
  if (B <= 0) return 0;
  if (!hist || !parent || !tokens || order < 2 || order > MAX_H + 1 || beam <= 0 || beam * (order - 1) > 256) return -1;
  hipLaunchKernelGGL(ngram_advance_kernel, dim3(B), dim3(256), 0, stream, hist, order - 1, parent, tokens, done, eos, beam);
  ST_CHECK_LAUNCH();
  return 0;
}

extern "C" int st_ngram_score_seq(hipStream_t stream, const int* child_lo, const int* tok, const float* logp, const float* bo,
                                  int nodes, int V, int order, float oov_logp, const int* tokens, const int* lens, int M, int L_cap,
                                  int bos, float* out) {
  if (M <= 0 || L_cap <= 0) return 0;
  if (!trie_ok(child_lo, tok, logp, bo, nodes, V, order) || !tokens || !lens || !out || !(oov_logp <= 0.f)) return -1;
  const Trie T{child_lo, tok, logp, bo, nodes, V, oov_logp};
  const long long total = (long long)M * L_cap;
  if (total > 0x7fffffffLL * 256) return -1;
  hipLaunchKernelGGL(ngram_score_seq_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, stream, T, order - 1, tokens, lens, M,
                     L_cap, bos, out);
  ST_CHECK_LAUNCH();
  return 0;
}
