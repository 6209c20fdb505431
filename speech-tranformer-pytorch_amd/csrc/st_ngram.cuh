// The trie walk of the back-off n-gram language model, shared by csrc/st_ngram.hip (scores of pre-beam candidates, teacher-forced
// scores) and csrc/st_ctc_beam.hip (the LM term inside the CTC prefix beam search).  ONE copy of the arithmetic: every kernel that
// scores a token is bit-equal to the NumPy float32 emulation tests/_emul_ngram.py.
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
#pragma once
#include "st_common.cuh"

namespace {

constexpr int MAX_H = 4;                                   // history tokens of an order-5 model

struct Trie {
  const int* child_lo; const int* tok; const float* logp; const float* bo; int nodes; int V; float oov;
};

// the child of `node` with token t (binary search among its sorted children: <= 13 rounds at V = 5120), -1 if there is none
__device__ __forceinline__ int find_child(const Trie& T, int node, int t) {
  int lo = max(T.child_lo[node], T.V), hi = min(T.child_lo[node + 1], T.nodes);
  while (lo < hi) {
    const int mid = (lo + hi) >> 1;
    if (T.tok[mid] < t) lo = mid + 1; else hi = mid;
  }
  return (lo < min(T.child_lo[node + 1], T.nodes) && T.tok[lo] == t) ? lo : -1;
}

// h[0] = the most recent token; -> k = the number of valid tokens (the history ends at the first id outside [0, V)) and
// bo[j - 1] = the back-off of the context of length j, j = 1 .. k
__device__ __forceinline__ int walk_history(const Trie& T, const int (&h)[MAX_H], int H, float (&bo)[MAX_H]) {
  int k = 0;
  while (k < H && h[k] >= 0 && h[k] < T.V) ++k;
  int node = -1;
#pragma unroll
  for (int j = 0; j < MAX_H; ++j) {
    bo[j] = 0.f;
    if (j < k && (j == 0 || node >= 0)) {
      node = j == 0 ? h[0] : find_child(T, node, h[j]);
      if (node >= 0) bo[j] = T.bo[node];
    }
  }
  return k;
}

__device__ __forceinline__ float score_candidate(const Trie& T, int c, const int (&h)[MAX_H], int k, const float (&bo)[MAX_H]) {
  if (c < 0 || c >= T.V) return -INFINITY;
  float val = T.logp[c];
  int m = 1, node = c;
  if (val == INFINITY) {
    val = T.oov;                                           // no unigram (and then no longer n-gram ends in c)
  } else {
    for (int j = 0; j < k; ++j) {
      node = find_child(T, node, h[j]);
      if (node < 0) break;
      val = T.logp[node];
      m = j + 2;
    }
  }
#pragma unroll
  for (int j = 1; j <= MAX_H; ++j)
    if (j >= m && j <= k) val += bo[j - 1];
  return val;
}

inline bool trie_ok(const int* child_lo, const int* tok, const float* logp, const float* bo, int nodes, int V, int order) {
  return child_lo && tok && logp && bo && V > 0 && V <= 5120 && nodes >= V && order >= 2 && order <= MAX_H + 1;
}

}  // namespace
