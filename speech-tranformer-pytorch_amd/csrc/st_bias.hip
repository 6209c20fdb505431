// Contextual biasing (st_amd/biasing.py): the phrase reward of every pre-beam candidate, the automaton states of the hypotheses
// a beam step chose, and teacher-forced per-position rewards of token lists.
//
// The phrases are an Aho-Corasick automaton (st_amd.biasing.DeviceAutomaton): node 0 the root, breadth-first numbering, the
// children of a node the consecutive nodes child_lo[node] .. child_lo[node + 1] - 1 sorted by tok, fail links to strictly
// shallower nodes.  Appending token c to a hypothesis in state s moves it to s' = delta(s, c) and adds
//   Delta(s, c) = cash[s'] + (phi[s'] - phi[s])     fp32, in that order;   Delta(s, eos) = -phi[s]
// (cash: the completed phrases' rewards, phi: the provisional reward of the match in progress), so a NumPy float32 emulation
// (tests/_emul_bias.py) is bit-equal.  State -1 = frozen (the hypothesis has emitted EOS): increment 0.
#include "st_bias.cuh"                                     // Automaton, bias_next, bias_delta, automaton_ok

namespace {

// ---- st_bias_score: one wave (= one workgroup) per hypothesis row, lane j = candidate j; the parent state is the row's
__global__ __launch_bounds__(64) void bias_score_kernel(Automaton A, const int* __restrict__ state, const int* __restrict__ cand, int K,
                                                        int beam, const unsigned char* __restrict__ done, int eos, float scale,
                                                        float* __restrict__ raw, float* __restrict__ lp) {
  const int i = blockIdx.x, lane = threadIdx.x;
  if (done && done[i / beam]) return;                      // a finished utterance: nothing is read or written
  const int s0 = state[i];
  const size_t at = (size_t)i * K + lane;
  if (s0 < 0) {                                            // frozen (emitted EOS): raw 0, lp untouched
    if (raw && lane < K) raw[at] = 0.f;
    return;
  }
  if (lane >= K) return;
  int s_next;
  const float d = bias_delta(A, bias_clamp_state(A, s0), cand[at], eos, &s_next);
  if (raw) raw[at] = d;
  if (lp) lp[at] = fmaf(scale, d, lp[at]);                 // (one rounding; d is finite, so -inf stays -inf)
}

// ---- st_bias_advance: one workgroup per utterance; thread s reads its parent's state and walks BEFORE the barrier, writes
//      after it: two children of one parent and overwritten parents are both right
__global__ __launch_bounds__(256) void bias_advance_kernel(Automaton A, int* __restrict__ state, const long long* __restrict__ order,
                                                           const long long* __restrict__ tokens,
                                                           const unsigned char* __restrict__ done, int eos, int beam) {
  const int b = blockIdx.x, s = threadIdx.x, base = b * beam;
  if (done && done[b]) return;
  const bool mine = s < beam;
  int v = -1;
  if (mine) {
    long long p = order[base + s];
    if (p < base || p >= base + beam) p = base + s;        // (never a row of another utterance)
    const int ps = state[p];
    const long long t = tokens[base + s];
    const int c = (t < 0 || t > 0x7fffffffLL) ? -1 : (int)t;
    if (ps >= 0 && !(c >= 0 && c == eos)) v = bias_next(A, bias_clamp_state(A, ps), c);
  }
  __syncthreads();
  if (mine) state[base + s] = v;
}

// ---- st_bias_score_seq: one lane per list, the positions in order (the state is a chain; lists are short)
__global__ __launch_bounds__(64) void bias_score_seq_kernel(Automaton A, const int* __restrict__ tokens, const int* __restrict__ lens,
                                                            int M, int L_cap, int eos, float* __restrict__ out) {
  const int m = blockIdx.x * 64 + threadIdx.x;
  if (m >= M) return;
  const int* row = tokens + (size_t)m * L_cap;
  float* o = out + (size_t)m * L_cap;
  const int len = min(max(lens[m], 0), L_cap);
  int s = 0;
  for (int t = 0; t < L_cap; ++t) {
    float d = 0.f;
    if (t < len && s >= 0) d = bias_delta(A, s, row[t], eos, &s);
    o[t] = d;
  }
}

}  // namespace

extern "C" int st_bias_score(hipStream_t stream, const int* child_lo, const int* tok, const int* fail, const float* cash,
                             const float* phi, int S, const int* state, const int* cand, int n, int K, int beam,
                             const unsigned char* done, int eos, float scale, float* raw, float* lp) {
  if (n <= 0) return 0;
  if (!automaton_ok(child_lo, tok, fail, S) || !cash || !phi || !state || !cand || K <= 0 || K > 64 || beam <= 0 || (n % beam) ||
      !(scale >= 0.f) || !(scale < INFINITY))
    return -1;
  const Automaton A{child_lo, tok, fail, cash, phi, S};
  hipLaunchKernelGGL(bias_score_kernel, dim3(n), dim3(64), 0, stream, A, state, cand, K, beam, done, eos, scale, raw, lp);
  ST_CHECK_LAUNCH();
  return 0;
}

extern "C" int st_bias_advance(hipStream_t stream, const int* child_lo, const int* tok, const int* fail, int S, int* state,
                               const long long* parent, const long long* tokens, const unsigned char* done, int eos, int B,
                               int beam) {
  if (B <= 0) return 0;
  if (!automaton_ok(child_lo, tok, fail, S) || !state || !parent || !tokens || beam <= 0 || beam > 256) return -1;
  const Automaton A{child_lo, tok, fail, nullptr, nullptr, S};
  hipLaunchKernelGGL(bias_advance_kernel, dim3(B), dim3(256), 0, stream, A, state, parent, tokens, done, eos, beam);
  ST_CHECK_LAUNCH();
  return 0;
}

extern "C" int st_bias_score_seq(hipStream_t stream, const int* child_lo, const int* tok, const int* fail, const float* cash,
                                 const float* phi, int S, const int* tokens, const int* lens, int M, int L_cap, int eos,
                                 float* out) {
  if (M <= 0 || L_cap <= 0) return 0;
  if (!automaton_ok(child_lo, tok, fail, S) || !cash || !phi || !tokens || !lens || !out) return -1;
  const Automaton A{child_lo, tok, fail, cash, phi, S};
  hipLaunchKernelGGL(bias_score_seq_kernel, dim3((unsigned)((M + 63) / 64)), dim3(64), 0, stream, A, tokens, lens, M, L_cap, eos, out);
  ST_CHECK_LAUNCH();
  return 0;
}
