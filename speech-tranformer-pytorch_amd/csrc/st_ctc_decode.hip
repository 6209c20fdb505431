// Joint CTC / attention beam search (Watanabe et al. 2017, "Hybrid CTC/Attention Architecture for End-to-End Speech
// Recognition", Algorithm 2): the CTC head's per-frame log-probabilities, the CTC prefix scorer, the attention pre-beam and
// the joint form of st_beam_advance, plus the frame arg-max of greedy CTC decoding.
//
// Notation (transformer/Decode.py, DESIGN.md "Joint CTC / attention decoding"): x_t(k) = log-softmax of the CTC logits of
// frame t; per hypothesis g the state gamma_n[t] / gamma_b[t] (alignments of frames 0..t that collapse to g and end in a
// non-blank / blank frame) and psi(g) = log CTC prefix probability.  Extension h = g.c (c not blank, not EOS):
//   phi_t        = gamma_b[t](g) if c == last(g), else logaddexp(gamma_n[t](g), gamma_b[t](g))
//   gamma_n[0](h) = x_0(c) if g is empty else -inf;  gamma_b[0](h) = -inf
//   gamma_n[t](h) = logaddexp(gamma_n[t-1](h), phi_{t-1}) + x_t(c)
//   gamma_b[t](h) = logaddexp(gamma_n[t-1](h), gamma_b[t-1](h)) + x_t(blank)
//   psi(h)        = logsumexp({gamma_n[0](h)} u {phi_{t-1} + x_t(c) : 1 <= t < T})
// psi(g.EOS) = logaddexp(gamma_n[T-1](g), gamma_b[T-1](g)) = log p_ctc(g | x); c = blank scores -inf.
//
// Both recurrences have the form y <- logaddexp(y, a) + b.  In the probability domain that is the affine map
// Y <- e^b Y + e^(a+b); as a pair (M, C) = (b, a + b) meaning y <- logaddexp(y + M, C), two maps compose in closed form:
// (M2, C2) o (M1, C1) = (M1 + M2, logaddexp(C1 + M2, C2)).  So one wave solves a 1,000-frame chain as a log-semiring scan:
// every lane composes the maps of its contiguous chunk of frames, a 6-step shuffle scan gives each lane the composition of
// the chunks before it, and the lanes replay their chunks from that value - 2 x (CH + 6) dependent steps instead of T.
#include "st_common.cuh"

namespace {

__device__ __forceinline__ float lae(float a, float b) {       // logaddexp, branch-free (v_exp_f32 / v_log_f32)
  const float m = fmaxf(a, b);
  const float r = m + __logf(1.f + __expf(fminf(a, b) - m));
  return m == -INFINITY ? -INFINITY : r;
}

// 64-bit ordering key of a candidate: monotone image of the value in the high word, 0x7fffffff - index in the low word
// (larger value first, lower index on ties; 0 = no candidate) - the order of st_beam_advance's keys
__device__ __forceinline__ unsigned long long cand_key(float x, int idx) {
  const unsigned u = __float_as_uint(x);
  const unsigned m = (u & 0x80000000u) ? ~u : (u | 0x80000000u);
  return ((unsigned long long)m << 32) | (unsigned)(0x7fffffff - idx);
}
__device__ __forceinline__ float cand_key_value(unsigned long long k) {
  const unsigned m = (unsigned)(k >> 32);
  return __uint_as_float((m & 0x80000000u) ? (m & 0x7fffffffu) : ~m);
}
__device__ __forceinline__ int cand_key_index(unsigned long long k) { return 0x7fffffff - (int)(unsigned)(k & 0xffffffffu); }

__device__ __forceinline__ unsigned long long wave_max_u64(unsigned long long k) {      // uniform
#pragma unroll
  for (int o = 32; o; o >>= 1) {
    const unsigned lo = __shfl_xor((unsigned)k, o, 64), hi = __shfl_xor((unsigned)(k >> 32), o, 64);
    const unsigned long long q = ((unsigned long long)hi << 32) | lo;
    k = q > k ? q : k;
  }
  return k;
}
__device__ __forceinline__ float wave_max_f(float v) {
#pragma unroll
  for (int o = 32; o; o >>= 1) v = fmaxf(v, __shfl_xor(v, o, 64));
  return v;
}
__device__ __forceinline__ float wave_sum_f(float v) {
#pragma unroll
  for (int o = 32; o; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}

// ---- st_ctc_vocab_lp (1): log-sum-exp of every packed CTC logits row, one wave per row, a running (max, sum) ------------
__global__ __launch_bounds__(256) void ctc_row_lse_kernel(const float* __restrict__ logits, int ldl, int R, int V,
                                                          float* __restrict__ lse) {
  const int row = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
  if (row >= R) return;
  const float* p = logits + (size_t)row * ldl;
  float m = -INFINITY, s = 0.f;
  for (int v0 = 0; v0 < V; v0 += 64 * 8) {
    float x[8];
#pragma unroll
    for (int u = 0; u < 8; ++u) x[u] = (v0 + u * 64 + lane < V) ? p[v0 + u * 64 + lane] : -INFINITY;
    float bm = x[0];
#pragma unroll
    for (int u = 1; u < 8; ++u) bm = fmaxf(bm, x[u]);
    const float mn = fmaxf(m, bm);
    if (mn > -INFINITY) {
      float bs = 0.f;
#pragma unroll
      for (int u = 0; u < 8; ++u) bs += __expf(x[u] - mn);
      s = s * __expf(m - mn) + bs;
      m = mn;
    }
  }
#pragma unroll
  for (int o = 32; o; o >>= 1) {
    const float om = __shfl_xor(m, o, 64), os = __shfl_xor(s, o, 64);
    const float mn = fmaxf(m, om);
    if (mn > -INFINITY) s = s * __expf(m - mn) + os * __expf(om - mn);
    m = mn;
  }
  if (lane == 0) lse[row] = m + __logf(s);
}

// ---- st_ctc_vocab_lp (2): lpT[b][v][t] = logits[off[b] + t][v] - lse, through a 64 x 64 LDS tile (rows read along the
//      vocabulary, written along the frames: both coalesced); frames t >= len[b] are written as 0
__global__ __launch_bounds__(256) void ctc_vocab_lp_kernel(const float* __restrict__ logits, int ldl, int V, const int* __restrict__ off,
                                                           const int* __restrict__ len, int T_cap, const float* __restrict__ lse,
                                                           float* __restrict__ lpT) {
  __shared__ float tile[64][65];
  const int b = blockIdx.z, t0 = blockIdx.x * 64, v0 = blockIdx.y * 64, tid = threadIdx.x;
  const int T = len[b], o = off[b], c = tid & 63;
#pragma unroll
  for (int k = 0; k < 16; ++k) {
    const int r = (tid >> 6) + 4 * k, t = t0 + r;
    float x = 0.f;
    if (t < T && v0 + c < V) x = logits[(size_t)(o + t) * ldl + v0 + c] - lse[o + t];
    tile[r][c] = x;
  }
  __syncthreads();
#pragma unroll
  for (int k = 0; k < 16; ++k) {
    const int r = (tid >> 6) + 4 * k, v = v0 + r;
    if (v < V) lpT[((size_t)b * V + v) * T_cap + t0 + c] = tile[c][r];
  }
}

// ---- st_ctc_prefix_init: the empty prefix in every beam slot of utterance b: gamma_n = -inf, gamma_b[t] = sum_{tau <= t}
//      x_tau(blank) (a wave scan over contiguous per-lane chunks), psi = 0, last = -1, not frozen
__global__ __launch_bounds__(64) void ctc_prefix_init_kernel(const float* __restrict__ lpT, int V, int T_cap, const int* __restrict__ len,
                                                             int beam, int blank, float* __restrict__ gam, float* __restrict__ psi,
                                                             int* __restrict__ last, unsigned char* __restrict__ frozen) {
  const int b = blockIdx.x, lane = threadIdx.x, T = min(len[b], T_cap), ch = T_cap / 64, t0 = lane * ch;
  const float* xb = lpT + ((size_t)b * V + blank) * T_cap;
  float s = 0.f;
  for (int k = 0; k < ch; ++k)
    if (t0 + k < T) s += xb[t0 + k];
  float inc = s;
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) {
    const float u = __shfl_up(inc, o, 64);
    if (lane >= o) inc += u;
  }
  float run = __shfl_up(inc, 1, 64);
  if (lane == 0) run = 0.f;
  for (int k = 0; k < ch; ++k) {
    const int t = t0 + k;
    float gb = -INFINITY;
    if (t < T) {
      run += xb[t];
      gb = run;
    }
    for (int s2 = 0; s2 < beam; ++s2) {
      float* g = gam + (size_t)(b * beam + s2) * 2 * T_cap;
      g[t] = -INFINITY;
      g[T_cap + t] = gb;
    }
  }
  if (lane < beam) {
    psi[b * beam + lane] = 0.f;
    last[b * beam + lane] = -1;
    frozen[b * beam + lane] = 0;
  }
}

template <int CH>
__device__ __forceinline__ void load_chunk(const float* __restrict__ p, float (&v)[CH]) {
  if constexpr (CH % 4 == 0) {
#pragma unroll
    for (int k = 0; k < CH; k += 4) {
      const f32x4 q = *reinterpret_cast<const f32x4*>(p + k);
      v[k] = q[0]; v[k + 1] = q[1]; v[k + 2] = q[2]; v[k + 3] = q[3];
    }
  } else {
#pragma unroll
    for (int k = 0; k < CH; ++k) v[k] = p[k];
  }
}
template <int CH>
__device__ __forceinline__ void store_chunk(float* __restrict__ p, const float (&v)[CH]) {
  if constexpr (CH % 4 == 0) {
#pragma unroll
    for (int k = 0; k < CH; k += 4) {
      f32x4 q;
      q[0] = v[k]; q[1] = v[k + 1]; q[2] = v[k + 2]; q[3] = v[k + 3];
      *reinterpret_cast<f32x4*>(p + k) = q;
    }
  } else {
#pragma unroll
    for (int k = 0; k < CH; ++k) p[k] = v[k];
  }
}

// In-wave log-semiring scan: the lane's chunk maps composed as (M, C) -> the value entering the lane's chunk (y_{-1} = -inf)
__device__ __forceinline__ float scan_entry(float M, float C, int lane) {
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) {
    const float Mo = __shfl_up(M, o, 64), Co = __shfl_up(C, o, 64);
    if (lane >= o) {            // (the earlier lanes' composition first, then this lane's)
      C = lae(Co + M, C);
      M = Mo + M;
    }
  }
  const float in = __shfl_up(C, 1, 64);
  return lane == 0 ? -INFINITY : in;
}

// ---- st_ctc_prefix_score: one wave per (hypothesis i, candidate j), 4 waves per workgroup; lane l owns frames
//      [l CH, (l + 1) CH) of T_cap = 64 CH
template <int CH>
__global__ __launch_bounds__(256) void ctc_prefix_score_kernel(const float* __restrict__ lpT, int V, int T_cap, const int* __restrict__ len,
                                                               int beam, int blank, int eos, const int* __restrict__ cand, int K, int n,
                                                               const float* __restrict__ gam, const float* __restrict__ psi,
                                                               const int* __restrict__ last, const unsigned char* __restrict__ frozen,
                                                               const unsigned char* __restrict__ done, float* __restrict__ cand_gam,
                                                               float* __restrict__ cand_psi, float* __restrict__ delta) {
  const int w = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
  if (w >= n * K) return;
  const int i = w / K, b = i / beam;
  if (done && done[b]) return;                         // a finished utterance: nothing is read or written
  const float psi_g = psi[i];
  if (frozen[i]) {                                     // emitted EOS below the top of its beam: the CTC state stays, increments 0
    if (lane == 0) {
      delta[w] = 0.f;
      cand_psi[w] = psi_g;
    }
    return;
  }
  const int c = cand[w], T = min(len[b], T_cap);
  const float* gn = gam + (size_t)i * 2 * T_cap;
  const float* gb = gn + T_cap;
  if (c == eos) {
    if (lane == 0) {
      const float p = T > 0 ? lae(gn[T - 1], gb[T - 1]) : -INFINITY;
      cand_psi[w] = p;
      delta[w] = p == -INFINITY ? -INFINITY : p - psi_g;
    }
    return;
  }
  if (c == blank || c < 0 || c >= V) {
    if (lane == 0) {
      cand_psi[w] = -INFINITY;
      delta[w] = -INFINITY;
    }
    return;
  }
  const bool rep = c == last[i], empty = last[i] < 0;
  const int t0 = lane * CH;
  float xc[CH], xb[CH], pn[CH], pb[CH];
  load_chunk<CH>(lpT + ((size_t)b * V + c) * T_cap + t0, xc);
  load_chunk<CH>(lpT + ((size_t)b * V + blank) * T_cap + t0, xb);
  load_chunk<CH>(gn + t0, pn);
  load_chunk<CH>(gb + t0, pb);
  // phi_{t-1} for the lane's frames t (frame t0 - 1 comes from the lane before); -inf outside [1, T).  Everything below is
  // branch-free: frame t = 0 (lane 0, k = 0) and the frames past T are selects, not control flow
  float ph[CH], tm[CH];                                // tm[k]: the frame's term of psi(h)
  {
    float an = __shfl_up(pn[CH - 1], 1, 64), ab = __shfl_up(pb[CH - 1], 1, 64);
#pragma unroll
    for (int k = 0; k < CH; ++k) {
      const int t = t0 + k;
      const float p = rep ? ab : lae(an, ab);
      ph[k] = (t >= 1 && t < T) ? p : -INFINITY;
      an = pn[k];
      ab = pb[k];
    }
  }
  const float g0 = (lane == 0 && empty) ? xc[0] : -INFINITY;      // gamma_n[0](h)
  // ---- gamma_n(h): frame t in [1, T) is the map (x_t(c), phi_{t-1} + x_t(c)), frames past T the identity (0, -inf), frame 0
  //      the constant (-inf, g0) - lane 0's composition then has M = -inf, which no C below depends on
  float M = 0.f, C = -INFINITY, mx = -INFINITY;
#pragma unroll
  for (int k = 0; k < CH; ++k) {
    const float m = t0 + k < T ? xc[k] : 0.f;
    tm[k] = ph[k] + xc[k];
    if (k == 0) tm[0] = lane == 0 ? g0 : tm[0];
    C = lae(C + m, tm[k]);
    M += m;
    mx = fmaxf(mx, tm[k]);
  }
  if (lane == 0) M = -INFINITY;
  float y = scan_entry(M, C, lane);
  float hn[CH];
#pragma unroll
  for (int k = 0; k < CH; ++k) {
    y = lae(y, ph[k]) + xc[k];
    if (k == 0) y = lane == 0 ? g0 : y;
    hn[k] = t0 + k < T ? y : -INFINITY;
  }
  // ---- gamma_b(h): frame t in [1, T) is (x_t(blank), gamma_n[t-1](h) + x_t(blank)), frame 0 the constant (-inf, -inf)
  float hb[CH];
  {
    float an = __shfl_up(hn[CH - 1], 1, 64);
    M = 0.f;
    C = -INFINITY;
#pragma unroll
    for (int k = 0; k < CH; ++k) {
      const int t = t0 + k;
      const bool in = t >= 1 && t < T;
      const float m = in ? xb[k] : 0.f;
      C = lae(C + m, in ? an + xb[k] : -INFINITY);
      M += m;
      an = hn[k];
    }
    if (lane == 0) M = -INFINITY;
    y = scan_entry(M, C, lane);
    an = __shfl_up(hn[CH - 1], 1, 64);
#pragma unroll
    for (int k = 0; k < CH; ++k) {
      y = lae(y, an) + xb[k];
      if (k == 0) y = lane == 0 ? -INFINITY : y;
      hb[k] = t0 + k < T ? y : -INFINITY;
      an = hn[k];
    }
  }
  // ---- psi(h): a wave log-sum-exp of the terms
  const float gm = wave_max_f(mx);
  const float gs = gm > -INFINITY ? gm : 0.f;
  float sm = 0.f;
#pragma unroll
  for (int k = 0; k < CH; ++k) sm += __expf(tm[k] - gs);
  sm = wave_sum_f(sm);
  const float ps = gm > -INFINITY ? gm + __logf(sm) : -INFINITY;
  float* out = cand_gam + (size_t)w * 2 * T_cap;
  store_chunk<CH>(out + t0, hn);
  store_chunk<CH>(out + T_cap + t0, hb);
  if (lane == 0) {
    cand_psi[w] = ps;
    delta[w] = ps == -INFINITY ? -INFINITY : ps - psi_g;
  }
}

// ---- st_beam_pre_beam: one workgroup per hypothesis row: log-softmax over the V logits, then the K best (best first, lower
//      id on ties): K rounds of a workgroup-wide key maximum; only the thread that owned the winner rescans its columns
template <int NU>
__global__ __launch_bounds__(256) void beam_pre_beam_kernel(const float* __restrict__ logits, int ldl, int V, int K, int* __restrict__ ids,
                                                            float* __restrict__ lp) {
  __shared__ float s_red[2][4];
  __shared__ unsigned long long s_key[2][4];
  const int row = blockIdx.x, tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
  const float* lg = logits + (size_t)row * ldl;
  float x[NU];
#pragma unroll
  for (int u = 0; u < NU; ++u) x[u] = lg[u * 256 + tid < V ? u * 256 + tid : 0];
#pragma unroll
  for (int u = 0; u < NU; ++u)
    if (u * 256 + tid >= V) x[u] = -INFINITY;
  float m = x[0];
#pragma unroll
  for (int u = 1; u < NU; ++u) m = fmaxf(m, x[u]);
  m = wave_max_f(m);
  if (lane == 0) s_red[0][wave] = m;
  __syncthreads();
  m = fmaxf(fmaxf(s_red[0][0], s_red[0][1]), fmaxf(s_red[0][2], s_red[0][3]));
  float sm = 0.f;
#pragma unroll
  for (int u = 0; u < NU; ++u) sm += __expf(x[u] - m);
  sm = wave_sum_f(sm);
  if (lane == 0) s_red[1][wave] = sm;
  __syncthreads();
  sm = (s_red[1][0] + s_red[1][1]) + (s_red[1][2] + s_red[1][3]);
  const float lse = m + __logf(sm);
  unsigned taken = 0u;
  auto local_best = [&]() {
    unsigned long long k = 0ull;
#pragma unroll
    for (int u = 0; u < NU; ++u) {
      const int col = u * 256 + tid;
      const unsigned long long q = (col < V && !((taken >> u) & 1u)) ? cand_key(x[u], col) : 0ull;
      k = q > k ? q : k;
    }
    return k;
  };
  unsigned long long mine = local_best();
  for (int r = 0; r < K; ++r) {
    const unsigned long long wm = wave_max_u64(mine);
    if (lane == 0) s_key[r & 1][wave] = wm;           // (ping-pong buffers: one barrier per round)
    __syncthreads();
    unsigned long long best = s_key[r & 1][0];
#pragma unroll
    for (int q = 1; q < 4; ++q) best = s_key[r & 1][q] > best ? s_key[r & 1][q] : best;
    if (mine == best && best != 0ull) {                // (keys are distinct: exactly one owner)
      const int col = cand_key_index(best);
      ids[(size_t)row * K + r] = col;
      lp[(size_t)row * K + r] = cand_key_value(best) - lse;
      taken |= 1u << (col >> 8);
      mine = local_best();
    }
  }
}

// ---- st_beam_advance_joint: one workgroup per utterance.  Wave 0 takes the `beam` best of the beam x K joint candidates
//      scores[s] + (1 - w) lp[s][j] + w delta[s][j] (16 keys per lane, `beam` rounds of a wave maximum), then the workgroup
//      writes st_beam_advance's state update, moves the CTC state of the survivors, the lineage table, the next decoder
//      input and the step counter.
struct JointArgs {
  const int* ids; const float* lp; const float* delta; int K; float w; int beam; int B; const long long* step; int eos;
  float* scores; long long* tokens; unsigned char* done; long long* lengths; float* hist_scores; long long* back; long long* toks;
  long long* order; int* anc; int S; long long* step_next; unsigned* ticket; const float* emb; int emb_rows; const float* pe;
  int pe_rows; bf16* x_next; int D; int T_cap; const float* cand_gam; const float* cand_psi; float* gam; float* psi; int* last;
  unsigned char* frozen;
};

__global__ __launch_bounds__(256) void beam_advance_joint_kernel(JointArgs a) {
  __shared__ float s_old[16], s_best[16], s_psi[16];
  __shared__ long long s_oldtok[16], s_tok[16];
  __shared__ int s_flat[16], s_last[16], s_src[16];
  __shared__ unsigned char s_frz[16];
  __shared__ int s_anc[16][128];
  const int b = blockIdx.x, tid = threadIdx.x, lane = tid & 63, beam = a.beam, K = a.K;
  const long long step = *a.step;
  const int t = (int)step, base = b * beam;
  const bool live_u = !a.done[b];
  int* const anc = t < a.S ? a.anc : nullptr;          // (a step past the table's columns: the table is left alone)
  if (tid < beam) {
    s_old[tid] = a.scores[base + tid];
    s_oldtok[tid] = a.tokens[base + tid];
    if (a.gam) {
      s_psi[tid] = a.psi[base + tid];
      s_last[tid] = a.last[base + tid];
      s_frz[tid] = a.frozen[base + tid];
    }
  }
  if (anc)
    for (int e = tid; e < beam * t; e += 256) s_anc[e / t][e % t] = anc[(size_t)(base + e / t) * a.S + e % t];
  __syncthreads();
  if (tid < 64) {
    const int nc = beam * K;                           // <= 1024: 16 per lane
    unsigned long long kk[16];
#pragma unroll
    for (int q = 0; q < 16; ++q) {
      const int f = q * 64 + lane;
      kk[q] = 0ull;
      if (f < nc) {
        const int s = f / K;
        const size_t at = (size_t)(base + s) * K + f % K;
        const float dl = a.delta[at];
        const float v = s_old[s] + (1.f - a.w) * a.lp[at] + (a.w > 0.f ? a.w * dl : 0.f);
        kk[q] = cand_key(v, f);
      }
    }
    for (int r = 0; r < beam; ++r) {
      unsigned long long m = kk[0];
#pragma unroll
      for (int q = 1; q < 16; ++q) m = kk[q] > m ? kk[q] : m;
      const unsigned long long best = wave_max_u64(m);
#pragma unroll
      for (int q = 0; q < 16; ++q)
        if (kk[q] == best) kk[q] = 0ull;
      if (lane == 0) {
        s_flat[r] = cand_key_index(best);
        s_best[r] = cand_key_value(best);
      }
    }
  }
  __syncthreads();
  // ---- the state update (one thread per beam slot), as st_beam_advance
  if (tid < beam) {
    const int s = tid;
    const size_t at = ((size_t)step * a.B + b) * beam + s;
    const int flat = s_flat[s];
    const int origin = live_u ? flat / K : s, j = flat % K;
    const long long tk = live_u ? (long long)a.ids[(size_t)(base + origin) * K + j] : s_oldtok[s];
    a.hist_scores[at] = s_old[s];
    a.back[at] = origin;
    a.toks[at] = tk;
    a.order[base + s] = origin + (long long)base;
    s_tok[s] = tk;
    s_src[s] = -1;
    if (live_u) {
      a.scores[base + s] = s_best[s];
      a.tokens[base + s] = tk;
      if (s == 0) {
        a.lengths[b] += 1;
        if (tk == a.eos) a.done[b] = 1;
      }
      if (a.gam) {                                     // the CTC state of the new hypothesis: from its parent and candidate
        const bool pf = s_frz[origin];
        a.psi[base + s] = pf ? s_psi[origin] : a.cand_psi[(size_t)(base + origin) * K + j];
        a.last[base + s] = pf ? s_last[origin] : (int)tk;
        a.frozen[base + s] = (pf || tk == a.eos) ? 1 : 0;
        if (!pf && tk != a.eos) s_src[s] = (base + origin) * K + j;
      }
    }
  }
  __syncthreads();
  if (a.gam) {
    const int n4 = 2 * a.T_cap / 4;
    for (int s = 0; s < beam; ++s) {
      const int src = s_src[s];
      if (src < 0) continue;
      const f32x4* from = reinterpret_cast<const f32x4*>(a.cand_gam + (size_t)src * 2 * a.T_cap);
      f32x4* to = reinterpret_cast<f32x4*>(a.gam + (size_t)(base + s) * 2 * a.T_cap);
      for (int e = tid; e < n4; e += 256) to[e] = from[e];
    }
  }
  // ---- the lineage table: slot s takes over its origin's positions 0 .. step - 1 and finds position `step` in the origin's
  //      slot (a done utterance: the identity)
  if (anc) {
    for (int s = 0; s < beam; ++s) {
      const int o = live_u ? s_flat[s] / K : s;
      for (int p = tid; p < t; p += 256) anc[(size_t)(base + s) * a.S + p] = s_anc[o][p];
      if (tid == 0) anc[(size_t)(base + s) * a.S + t] = base + o;
    }
  }
  // ---- the next step's decoder input: bf16(emb[token] + pe[step + 1])
  if (a.x_next && step + 1 < a.pe_rows) {
    const int D4 = a.D / 4;
    for (int e = tid; e < beam * D4; e += 256) {
      const int s = e / D4, ch = e % D4;
      const long long tk = s_tok[s];
      if (tk < 0 || tk >= a.emb_rows) __builtin_trap();
      const f32x4 ev = *reinterpret_cast<const f32x4*>(a.emb + (size_t)tk * a.D + ch * 4);
      const f32x4 pp = *reinterpret_cast<const f32x4*>(a.pe + (size_t)(step + 1) * a.D + ch * 4);
      bf16x4 o;
#pragma unroll
      for (int k = 0; k < 4; ++k) o[k] = (bf16)(ev[k] + pp[k]);
      *reinterpret_cast<bf16x4*>(a.x_next + (size_t)(base + s) * a.D + ch * 4) = o;
    }
  }
  // ---- the step counter: every workgroup has read it before it draws its ticket; the last one advances it
  if (a.step_next && tid == 0) {
    if (atomicAdd(a.ticket, 1u) == (unsigned)(a.B - 1)) {
      *a.ticket = 0u;
      *a.step_next = step + 1;
    }
  }
}

// ---- st_ctc_best_path: the arg-max of every CTC logits row (lower id on ties), one wave per row
__global__ __launch_bounds__(256) void ctc_best_path_kernel(const float* __restrict__ logits, int ldl, int R, int V, int* __restrict__ out) {
  const int row = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
  if (row >= R) return;
  const float* p = logits + (size_t)row * ldl;
  float m = -INFINITY;
  int mi = 0x7fffffff;
  for (int v = lane; v < V; v += 64) {
    const float x = p[v];
    if (x > m || mi == 0x7fffffff) {
      m = x;
      mi = v;
    }
  }
#pragma unroll
  for (int o = 32; o; o >>= 1) {
    const float om = __shfl_xor(m, o, 64);
    const int oi = __shfl_xor(mi, o, 64);
    if (om > m || (om == m && oi < mi)) {
      m = om;
      mi = oi;
    }
  }
  if (lane == 0) out[row] = mi;
}

}  // namespace

extern "C" int st_ctc_vocab_lp(hipStream_t stream, const float* logits, int ldl, int R, int V, const int* off, const int* len, int B,
                               int T_cap, float* lse, float* lpT) {
  if (R <= 0 || B <= 0) return 0;
  if (!logits || !off || !len || !lse || !lpT || V <= 0 || ldl < V || T_cap <= 0 || (T_cap % 64)) return -1;
  hipLaunchKernelGGL(ctc_row_lse_kernel, dim3((R + 3) / 4), dim3(256), 0, stream, logits, ldl, R, V, lse);
  hipLaunchKernelGGL(ctc_vocab_lp_kernel, dim3(T_cap / 64, (V + 63) / 64, B), dim3(256), 0, stream, logits, ldl, V, off, len, T_cap, lse,
                     lpT);
  ST_CHECK_LAUNCH();
  return 0;
}

extern "C" int st_ctc_prefix_init(hipStream_t stream, const float* lpT, int V, int T_cap, const int* len, int B, int beam, int blank,
                                  float* gam, float* psi, int* last, unsigned char* frozen) {
  if (B <= 0) return 0;
  if (!lpT || !len || !gam || !psi || !last || !frozen || V <= 0 || T_cap <= 0 || (T_cap % 64) || beam <= 0 || beam > 64 ||
      blank < 0 || blank >= V)
    return -1;
  hipLaunchKernelGGL(ctc_prefix_init_kernel, dim3(B), dim3(64), 0, stream, lpT, V, T_cap, len, beam, blank, gam, psi, last, frozen);
  ST_CHECK_LAUNCH();
  return 0;
}

extern "C" int st_ctc_prefix_score(hipStream_t stream, const float* lpT, int V, int T_cap, const int* len, int B, int beam, int blank,
                                   int eos, const int* cand, int K, const float* gam, const float* psi, const int* last,
                                   const unsigned char* frozen, const unsigned char* done, float* cand_gam, float* cand_psi,
                                   float* delta) {
  if (B <= 0) return 0;
  if (!lpT || !len || !cand || !gam || !psi || !last || !frozen || !cand_gam || !cand_psi || !delta || V <= 0 || beam <= 0 ||
      K <= 0 || K > 64 || blank < 0 || blank >= V || T_cap <= 0 || (T_cap % 64))
    return -1;
  const int n = B * beam;
  const dim3 grid((n * K + 3) / 4), blk(256);
#define ST_PREFIX_CASE(CH)                                                                                                 \
  case CH:                                                                                                                 \
    hipLaunchKernelGGL((ctc_prefix_score_kernel<CH>), grid, blk, 0, stream, lpT, V, T_cap, len, beam, blank, eos, cand, K, n, gam, \
                       psi, last, frozen, done, cand_gam, cand_psi, delta);                                                 \
    break;
  switch (T_cap / 64) {
    ST_PREFIX_CASE(1)
    ST_PREFIX_CASE(2)
    ST_PREFIX_CASE(4)
    ST_PREFIX_CASE(8)
    ST_PREFIX_CASE(12)
    ST_PREFIX_CASE(16)
    ST_PREFIX_CASE(24)
    ST_PREFIX_CASE(32)
    default:
      return -1;
  }
#undef ST_PREFIX_CASE
  ST_CHECK_LAUNCH();
  return 0;
}

extern "C" int st_beam_pre_beam(hipStream_t stream, const float* logits, int ldl, int V, int n, int K, int* ids, float* lp) {
  if (n <= 0) return 0;
  if (!logits || !ids || !lp || V <= 0 || V > 20 * 256 || ldl < V || K <= 0 || K > 64 || K > V) return -1;
  hipLaunchKernelGGL((beam_pre_beam_kernel<20>), dim3(n), dim3(256), 0, stream, logits, ldl, V, K, ids, lp);
  ST_CHECK_LAUNCH();
  return 0;
}

extern "C" int st_beam_advance_joint(hipStream_t stream, const int* ids, const float* lp, const float* delta, int K, float ctc_weight,
                                     int beam, int B, const long long* step, int eos, float* scores, long long* tokens,
                                     unsigned char* done, long long* lengths, float* hist_scores, long long* back, long long* toks,
                                     long long* order, int* anc, int S, long long* step_next, void* ticket, const float* emb,
                                     int emb_rows, const float* pe, int pe_rows, void* x_next, int D, int T_cap,
                                     const float* cand_gam, const float* cand_psi, float* gam, float* psi, int* last,
                                     unsigned char* frozen) {
  if (B <= 0) return 0;
  if (!ids || !lp || !delta || beam <= 0 || beam > 16 || K < beam || K > 64 || !(ctc_weight >= 0.f && ctc_weight < 1.f) || !step ||
      !scores || !tokens || !done || !lengths || !hist_scores || !back || !toks || !order)
    return -1;
  if (anc && (S <= 0 || S > 128)) return -1;
  if (step_next && (step_next != step || !ticket)) return -1;
  if (x_next && (!emb || !pe || emb_rows <= 0 || pe_rows <= 0 || D <= 0 || (D & 3))) return -1;
  const bool ctc = gam != nullptr;
  if (ctc && (!cand_gam || !cand_psi || !psi || !last || !frozen || T_cap <= 0 || (T_cap & 1))) return -1;
  JointArgs a{ids, lp, delta, K, ctc_weight, beam, B, step, eos, scores, tokens, done, lengths, hist_scores, back, toks, order, anc, S,
              step_next, (unsigned*)ticket, emb, emb_rows, pe, pe_rows, (bf16*)x_next, D, T_cap, cand_gam, cand_psi, gam, psi, last,
              frozen};
  hipLaunchKernelGGL(beam_advance_joint_kernel, dim3(B), dim3(256), 0, stream, a);
  ST_CHECK_LAUNCH();
  return 0;
}

extern "C" int st_ctc_best_path(hipStream_t stream, const float* logits, int ldl, int R, int V, int* out) {
  if (R <= 0) return 0;
  if (!logits || !out || V <= 0 || ldl < V) return -1;
  hipLaunchKernelGGL(ctc_best_path_kernel, dim3((R + 3) / 4), dim3(256), 0, stream, logits, ldl, R, V, out);
  ST_CHECK_LAUNCH();
  return 0;
}
