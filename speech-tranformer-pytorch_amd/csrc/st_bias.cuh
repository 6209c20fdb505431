// The automaton walk of contextual biasing (st_amd/biasing.py), shared by the kernels of csrc/st_bias.hip.  ONE copy of the
// arithmetic: every kernel that scores a token is bit-equal to the NumPy float32 emulation tests/_emul_bias.py.
//
// The phrases are an Aho-Corasick automaton (st_amd.biasing.DeviceAutomaton): node 0 is the root, nodes are numbered
// breadth-first, the children of a node are the consecutive nodes child_lo[node] .. child_lo[node + 1] - 1 sorted by tok;
// fail[node] = the longest proper suffix of the node's path that is a path itself (strictly shallower; depth <= 32).
//   delta(s, c): while s has no child c and s is not the root: s = fail[s]; then the child if there is one, else the root
//   Delta(s, c) = cash[s'] + (phi[s'] - phi[s]), s' = delta(s, c)      fp32, in that order;  Delta(s, eos) = -phi[s]
// The walk cannot hang or leave the tables WHATEVER they hold: the fail loop runs at most MAX_DEPTH times, every state is
// clamped to [0, S), every child range to [0, S].
#pragma once
#include "st_common.cuh"

namespace {

constexpr int BIAS_MAX_DEPTH = 32;                         // tokens of the longest phrase = the longest fail chain
constexpr int BIAS_MAX_STATES = 65536;

struct Automaton {
  const int* child_lo; const int* tok; const int* fail; const float* cash; const float* phi; int S;
};

__device__ __forceinline__ int bias_clamp_state(const Automaton& A, int s) { return min(max(s, 0), A.S - 1); }

// the child of `node` (in [0, S)) with token t: binary search among its sorted children (<= 17 rounds), -1 if there is none
__device__ __forceinline__ int bias_find_child(const Automaton& A, int node, int t) {
  int lo = min(max(A.child_lo[node], 0), A.S);
  const int end = min(max(A.child_lo[node + 1], 0), A.S);
  int hi = end;
  while (lo < hi) {
    const int mid = (lo + hi) >> 1;
    if (A.tok[mid] < t) lo = mid + 1; else hi = mid;
  }
  return (lo < end && A.tok[lo] == t) ? lo : -1;
}

// delta(s, c), s in [0, S)
__device__ __forceinline__ int bias_next(const Automaton& A, int s, int c) {
  int ch = bias_find_child(A, s, c);
  for (int it = 0; it < BIAS_MAX_DEPTH && ch < 0 && s != 0; ++it) {
    s = bias_clamp_state(A, A.fail[s]);
    ch = bias_find_child(A, s, c);
  }
  return ch >= 0 ? ch : 0;
}

// Delta(s, c) for a live state s in [0, S); *s_next = the state after c (-1: frozen by eos)
__device__ __forceinline__ float bias_delta(const Automaton& A, int s, int c, int eos, int* s_next) {
  if (c >= 0 && c == eos) {
    *s_next = -1;
    return -A.phi[s];
  }
  const int s2 = bias_next(A, s, c);
  *s_next = s2;
  return A.cash[s2] + (A.phi[s2] - A.phi[s]);
}

inline bool automaton_ok(const int* child_lo, const int* tok, const int* fail, int S) {
  return child_lo && tok && fail && S >= 1 && S <= BIAS_MAX_STATES;
}

}  // namespace
