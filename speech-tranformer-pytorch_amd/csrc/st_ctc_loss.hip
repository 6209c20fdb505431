// CTC loss of the joint CTC / attention objective (BASELINE config 4) with lengths and labels on the DEVICE: nothing here touches
// host memory, so the two launches sit inside a captured training step (torch's ctc_loss builds its length tables from pageable
// host memory and cannot).
//
// Notation (Graves et al. 2006): lp[b][t][k] log-probabilities over the utterance's small alphabet (class 0 = blank; what
// st_ctc_gather writes), labels c_0 .. c_{tl-1} (class indices), extended sequence l' = [0, c_0, 0, c_1, ..., 0] of S = 2 tl + 1
// states.  alpha_t(s) = lae(alpha_{t-1}(s), alpha_{t-1}(s-1), [l'(s) != l'(s-2)] alpha_{t-1}(s-2)) + lp_t(l'(s)); beta the same
// from the other end.  ONE rule for every state: a label may equal class 0 (this repository's ground truth ends every utterance
// with id 0) - it is an ordinary label state that emits column 0; blank states never skip because l'(s) = l'(s-2) = 0 there.
//
// st_ctc_loss_fwd: the recursions are T dependent steps, so latency per frame is the whole cost.  One WAVE per (utterance,
// direction) - alpha and beta of an utterance run side by side on different CUs.  beta is alpha of the mirrored problem (labels
// and frames reversed, state s <-> S-1-s), so both directions are the same code.  Lane j holds the state pairs (blank 2q, label
// 2q+1), q = j P .. j P + P - 1, in registers: one step needs the label value of pair q - 1, i.e. ONE shift by a lane (DPP
// wave_shr:1), no LDS, no barrier.  The two emissions a lane needs per frame (column 0, column c_q) are prefetched a whole chunk
// of frames ahead (column 0 is uniform: scalar loads).  Every 8 frames the wave subtracts its maximum from all states and adds
// it to a double offset: the stored values stay within ~100 of 0 (ulp 8e-6) instead of running to the log-likelihood (-6,000 at
// T = 1,000: ulp 5e-4 per step, the 0.03 .. 0.1 of accumulated error tests/test_fullsize_gpu.py notes for fp32 CTC).
//
// st_ctc_loss_grad: fully parallel.  One wave per frame: p(s) = exp(alpha + beta - lp + (offsets + nll)) for the S states into
// LDS, then thread k sums the states of class k IN LABEL ORDER (a plain loop over the <= 255 label positions: no float atomics,
// bitwise reproducible) and writes g = coef (exp(lp) - occ) - the convention st_ctc_dlogits consumes (softmax_term = 0: -coef occ alone, the derivative
// of coef nll with respect to lp itself).
#include "st_common.cuh"

namespace {

// The recursions run in BASE 2 (v_exp_f32 / v_log_f32 are base-2 instructions: no scaling multiply and no range fix-up of a
// full logf on the dependent chain): alpha, beta and their offsets are stored in units of log2.  Same branch-free shape as lae
// of csrc/st_ctc_decode.hip; the clamp of the maximum keeps an all -inf input at -inf (log2 0) instead of -inf - -inf = NaN.
__device__ __forceinline__ float lae2(float a, float b) {
  const float m = fmaxf(fmaxf(a, b), -3.0e38f);
  return m + __builtin_amdgcn_logf(__builtin_amdgcn_exp2f(a - m) + __builtin_amdgcn_exp2f(b - m));
}
__device__ __forceinline__ float lae3(float a, float b, float c) {
  const float m = fmaxf(fmaxf(fmaxf(a, b), c), -3.0e38f);
  return m + __builtin_amdgcn_logf(__builtin_amdgcn_exp2f(a - m) + __builtin_amdgcn_exp2f(b - m) + __builtin_amdgcn_exp2f(c - m));
}
constexpr float LOG2E = 1.4426950408889634f;
constexpr double LN2 = 0.6931471805599453;

// the value of the lane below (lane 0: -inf) - DPP wave_shr:1, a register move
__device__ __forceinline__ float lane_below(float v) {
  return __int_as_float(__builtin_amdgcn_update_dpp(__float_as_int(-INFINITY), __float_as_int(v), 0x138, 0xf, 0xf, false));
}
__device__ __forceinline__ float wave_max_f(float v) {
#pragma unroll
  for (int o = 32; o; o >>= 1) v = fmaxf(v, __shfl_xor(v, o, 64));
  return v;
}

constexpr int RENORM = 8;        // frames between two renormalisations (a power of two; the chunk lengths are multiples)

__host__ __device__ inline int ctc_off_blocks(int T) { return T / RENORM + 2; }

// workspace: alpha f32 [B][T][S_cap] | beta f32 [B][T][S_cap] | offsets f64 [B][2][T / 8 + 2]   (S_cap = 2 L + 2: the last slot of
// a row is where the lanes without a state drop their stores - never read)
struct CtcWs {
  float* alpha;
  float* beta;
  double* offs;
};
__host__ __device__ inline long long ctc_ws_bytes(int B, int T, int L) {
  return 2ll * B * T * (2 * L + 2) * 4 + 16ll * B * ctc_off_blocks(T);
}
__host__ __device__ inline CtcWs ctc_ws(void* ws, int B, int T, int L) {
  CtcWs w;
  w.alpha = (float*)ws;
  w.beta = w.alpha + (size_t)B * T * (2 * L + 2);
  w.offs = (double*)(w.beta + (size_t)B * T * (2 * L + 2));
  return w;
}

template <int P, int CH>
__global__ __launch_bounds__(64) void ctc_recursion_kernel(const float* __restrict__ lp, int T, int C, const long long* __restrict__ classes,
                                                           int L, const int* __restrict__ in_len, const int* __restrict__ tgt_len,
                                                           CtcWs w, float* __restrict__ nll) {
  const int b = blockIdx.x, lane = threadIdx.x;
  const bool rev = blockIdx.y != 0;
  const int Tb = min(max(in_len[b], 0), T), tl = min(max(tgt_len[b], 0), L), S = 2 * tl + 1, S_cap = 2 * L + 2;
  const int nb = ctc_off_blocks(T);
  double* offs = w.offs + ((size_t)b * 2 + (rev ? 1 : 0)) * nb;
  if (Tb == 0) {
    if (!rev && lane == 0) nll[b] = INFINITY;
    return;
  }
  float* out = (rev ? w.beta : w.alpha) + (size_t)b * T * S_cap;
  const float* row0 = lp + (size_t)b * T * C;
  const long long* cls = classes + (size_t)b * L;
  // pair q: blank state 2q (exists for q <= tl), label state 2q + 1 (q < tl) of this direction's sequence.  The lanes past the
  // last state run the same arithmetic on values nobody reads (a state is fed from s, s - 1, s - 2 only: nothing flows back)
  int col[P];
  unsigned ib[P], il[P];         // where the pair's two states go in a frame's row of the workspace
  bool xb[P], xl[P], sk[P];
#pragma unroll
  for (int p = 0; p < P; ++p) {
    const int q = lane * P + p;
    xb[p] = q <= tl;
    xl[p] = q < tl;
    int c = 0, cp = -1;
    if (xl[p]) {
      c = min(max((int)cls[rev ? tl - 1 - q : q], 0), C - 1);
      if (q > 0) cp = min(max((int)cls[rev ? tl - q : q - 1], 0), C - 1);
    }
    col[p] = c;
    sk[p] = xl[p] && q > 0 && c != cp;
    ib[p] = xb[p] ? (unsigned)(rev ? S - 1 - 2 * q : 2 * q) : (unsigned)(S_cap - 1);
    il[p] = xl[p] ? (unsigned)(rev ? S - 2 - 2 * q : 2 * q + 1) : (unsigned)(S_cap - 1);
  }
  float ab[P], al[P];            // the state before frame 0: probability 1 in blank state 0
#pragma unroll
  for (int p = 0; p < P; ++p) {
    ab[p] = (lane == 0 && p == 0) ? 0.f : -INFINITY;
    al[p] = -INFINITY;
  }
  double off = 0.0;
  if (lane == 0) offs[0] = 0.0;
  const float l2e = LOG2E;
  float e0[CH], ec[CH][P], n0[CH], nc[CH][P];
  auto fetch = [&](int tau0, float (&f0)[CH], float (&fc)[CH][P]) {
#pragma unroll
    for (int k = 0; k < CH; ++k) {
      const int tau = tau0 + k;
      const bool in = tau < Tb;
      const float* r = row0 + (size_t)(in ? (rev ? Tb - 1 - tau : tau) : 0) * C;
      f0[k] = in ? r[0] : 0.f;
#pragma unroll
      for (int p = 0; p < P; ++p) fc[k][p] = in ? r[col[p]] : 0.f;
    }
  };
  fetch(0, e0, ec);
  for (int tau0 = 0; tau0 < Tb; tau0 += CH) {
    fetch(tau0 + CH, n0, nc);                    // the next chunk's emissions are in flight while this one is consumed
#pragma unroll
    for (int k = 0; k < CH; ++k) {
      const int tau = tau0 + k;
      if (tau < Tb) {                            // (uniform)
        float pl = lane_below(al[P - 1]);
#pragma unroll
        for (int p = 0; p < P; ++p) {
          const float vb = __builtin_fmaf(e0[k], l2e, lae2(ab[p], pl));
          const float vl = __builtin_fmaf(ec[k][p], l2e, lae3(al[p], ab[p], sk[p] ? pl : -INFINITY));
          pl = al[p];
          ab[p] = vb;
          al[p] = vl;
        }
        if ((k & (RENORM - 1)) == RENORM - 1) {
          float m = -INFINITY;
#pragma unroll
          for (int p = 0; p < P; ++p) m = fmaxf(m, fmaxf(xb[p] ? ab[p] : -INFINITY, xl[p] ? al[p] : -INFINITY));
          m = wave_max_f(m);
          m = m == -INFINITY ? 0.f : m;
#pragma unroll
          for (int p = 0; p < P; ++p) {
            ab[p] -= m;
            al[p] -= m;
          }
          off += (double)m;
          if (lane == 0) offs[(tau + 1) / RENORM] = off;
        }
        float* o = out + (size_t)(rev ? Tb - 1 - tau : tau) * S_cap;
#pragma unroll
        for (int p = 0; p < P; ++p) {
          o[ib[p]] = ab[p];
          o[il[p]] = al[p];
        }
      }
    }
#pragma unroll
    for (int k = 0; k < CH; ++k) {
      e0[k] = n0[k];
#pragma unroll
      for (int p = 0; p < P; ++p) ec[k][p] = nc[k][p];
    }
  }
  if (!rev) {                                    // log-likelihood: the last blank and the last label state of the last frame
    float v = -INFINITY;
#pragma unroll
    for (int p = 0; p < P; ++p) {
      const int q = lane * P + p;
      if (q == tl) v = lae2(v, ab[p]);
      if (q == tl - 1) v = lae2(v, al[p]);
    }
    const float m = wave_max_f(v);
    const float ms = m == -INFINITY ? 0.f : m;
    float sm = __builtin_amdgcn_exp2f(v - ms);   // (at most two lanes are not -inf)
#pragma unroll
    for (int o = 32; o; o >>= 1) sm += __shfl_xor(sm, o, 64);
    if (lane == 0) nll[b] = m == -INFINITY ? INFINITY : (float)(-LN2 * ((double)(m + __builtin_amdgcn_logf(sm)) + off));
  }
}

constexpr int GRAD_FRAMES = 16;      // frames per workgroup (4 waves x 4 frames)

__global__ __launch_bounds__(256) void ctc_grad_kernel(const float* __restrict__ lp, int T, int C, const long long* __restrict__ classes,
                                                       int L, const int* __restrict__ in_len, const int* __restrict__ tgt_len,
                                                       const float* __restrict__ coef, CtcWs w, const float* __restrict__ nll,
                                                       float* __restrict__ g, float* __restrict__ roww, int softmax_term) {
  __shared__ float s_p[4][512];
  __shared__ int s_cls[256];
  const int b = blockIdx.y, tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
  const int Tb = min(max(in_len[b], 0), T), tl = min(max(tgt_len[b], 0), L), S = 2 * tl + 1, S_cap = 2 * L + 2;
  const float nl = nll[b], cf = coef[b];
  const bool fin = nl < INFINITY && nl > -INFINITY;          // (NaN: not finite either)
  if (blockIdx.x == 0 && tid == 0) roww[b] = fin ? cf : 0.f;
  for (int j = tid; j < tl; j += 256) s_cls[j] = min(max((int)classes[(size_t)b * L + j], 0), C - 1);
  __syncthreads();
  const int nb = ctc_off_blocks(T);
  const double* offA = w.offs + (size_t)b * 2 * nb;
  const double* offB = offA + nb;
  for (int i = 0; i < GRAD_FRAMES / 4; ++i) {                // (uniform trip count: the barriers below are the workgroup's)
    const int t = blockIdx.x * GRAD_FRAMES + i * 4 + wave;
    const bool live = fin && t < Tb;
    const size_t at = (size_t)b * T + t;
    if (live) {
      const float cst = (float)(offA[(t + 1) / RENORM] + offB[(Tb - t) / RENORM] + (double)nl * (1.0 / LN2));      // log2 units
      const float* a = w.alpha + at * S_cap;
      const float* be = w.beta + at * S_cap;
      const float* r = lp + at * C;
      for (int s = lane; s < S; s += 64) {
        const int k = (s & 1) ? s_cls[s >> 1] : 0;
        const float va = a[s], vb = be[s];
        s_p[wave][s] = (va > -INFINITY && vb > -INFINITY) ? __builtin_amdgcn_exp2f(__builtin_fmaf(-r[k], LOG2E, va + vb + cst)) : 0.f;
      }
    }
    __syncthreads();
    if (t < T) {
      for (int k = lane; k < C; k += 64) {
        float v = 0.f;
        if (live) {
          float occ = 0.f;
          if (k == 0)
            for (int j = 0; j <= tl; ++j) occ += s_p[wave][2 * j];
          for (int j = 0; j < tl; ++j)
            if (s_cls[j] == k) occ += s_p[wave][2 * j + 1];
          v = cf * ((softmax_term ? __expf(lp[at * C + k]) : 0.f) - occ);
        }
        g[at * C + k] = v;
      }
    }
    __syncthreads();
  }
}

bool ctc_args_ok(const void* lp, int B, int T, int C, const void* classes, int L, const void* in_len, const void* tgt_len, const void* ws,
                 long long ws_bytes) {
  return lp && in_len && tgt_len && ws && T > 0 && C >= 2 && L >= 0 && L <= 255 && (classes || L == 0) &&
         ws_bytes >= ctc_ws_bytes(B, T, L);
}

}  // namespace

extern "C" int st_ctc_loss_ws_kib(int B, int T, int L) {
  if (B < 0 || T < 0 || L < 0 || L > 255) return -1;
  return (int)((ctc_ws_bytes(B, T, L) + 1023) / 1024);
}

extern "C" int st_ctc_loss_fwd(hipStream_t stream, const float* lp, int B, int T, int C, const long long* classes, int L, const int* in_len,
                               const int* tgt_len, void* ws, long long ws_bytes, float* nll) {
  if (B <= 0) return 0;
  if (!ctc_args_ok(lp, B, T, C, classes, L, in_len, tgt_len, ws, ws_bytes) || !nll) return -1;
  const CtcWs w = ctc_ws(ws, B, T, L);
  const dim3 grid(B, 2), blk(64);
  if (L <= 63)
    hipLaunchKernelGGL((ctc_recursion_kernel<1, 16>), grid, blk, 0, stream, lp, T, C, classes, L, in_len, tgt_len, w, nll);
  else if (L <= 127)
    hipLaunchKernelGGL((ctc_recursion_kernel<2, 16>), grid, blk, 0, stream, lp, T, C, classes, L, in_len, tgt_len, w, nll);
  else
    hipLaunchKernelGGL((ctc_recursion_kernel<4, 8>), grid, blk, 0, stream, lp, T, C, classes, L, in_len, tgt_len, w, nll);
  ST_CHECK_LAUNCH();
  return 0;
}

extern "C" int st_ctc_loss_grad(hipStream_t stream, const float* lp, int B, int T, int C, const long long* classes, int L, const int* in_len,
                                const int* tgt_len, const float* coef, void* ws, long long ws_bytes, const float* nll, float* g,
                                float* roww, int softmax_term) {
  if (B <= 0) return 0;
  if (!ctc_args_ok(lp, B, T, C, classes, L, in_len, tgt_len, ws, ws_bytes) || !coef || !nll || !g || !roww) return -1;
  const CtcWs w = ctc_ws(ws, B, T, L);
  hipLaunchKernelGGL(ctc_grad_kernel, dim3((T + GRAD_FRAMES - 1) / GRAD_FRAMES, B), dim3(256), 0, stream, lp, T, C, classes, L, in_len,
                     tgt_len, coef, w, nll, g, roww, softmax_term);
  ST_CHECK_LAUNCH();
  return 0;
}
