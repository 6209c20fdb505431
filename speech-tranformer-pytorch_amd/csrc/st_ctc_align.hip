// CTC forced alignment: the Viterbi (best-path) alignment of a transcript through the CTC head's lattice - the max-plus sibling of
// the alpha recursion of csrc/st_ctc_loss.hip, plus back-pointers and a backtrace.  Same inputs as st_ctc_loss_fwd (lp f32
// [B, T, C] over the utterance's small alphabet, class 0 = blank; classes i64 [B, L]; device-resident lengths): nothing is read
// from host memory, so the launch can be captured.
//
// Extended sequence l' = [0, c_0, 0, c_1, ..., 0], S = 2 tl + 1 states; v_0(0) = lp_0(0), v_0(1) = lp_0(c_0);
// v_t(s) = lp_t(l'(s)) + max(v_{t-1}(s), v_{t-1}(s-1), [l'(s) != l'(s-2)] v_{t-1}(s-2)) - ONE skip rule for every state, as in the
// loss (a label may equal class 0: an ordinary label state that emits column 0).  TIE RULE (part of the contract, what
// tests/_ctc_align_ref.py restates): the predecessors are tried in the order stay, s-1, s-2 and a later one wins only if it is
// strictly greater; the end state is S-1 unless S-2 is strictly better.
//
// Arithmetic: fp32 in natural units - max-plus needs no exp / log, so no LOG2E scale (which would cost exactness); every 8 frames
// the wave maximum is subtracted from all states, so the stored magnitudes stay small.  With integer-valued lp every operation
// is exact.
//
// Forward sweep: one WAVE per utterance, lane j holds the state pairs (blank 2q, label 2q+1), q = j P .. j P + P - 1, in registers;
// the label value of pair q - 1 arrives by one DPP wave_shr:1; the two emissions a lane needs per frame are prefetched a chunk of
// frames ahead.  T dependent steps: latency per frame is the whole cost.  Per frame and lane the back-pointers (2 bits per state:
// how far below s the best predecessor lies) are packed into one byte (P <= 2) or halfword (P = 4) and stored off the dependent
// chain - into LDS when the utterance's frames fit (128 KiB: 1,024 frames at P = 4, 2,048 at P <= 2), else into ``ws``.
//
// Backtrace: a wave-uniform walk in chunks of 64 frames.  Every lane first loads ITS OWN back-pointer word of each of the chunk's
// frames from LDS (64 independent reads in flight), then the walk takes the word of the lane that owns the current state with
// v_readlane: scalar shifts and a subtract per frame, no memory access on the dependent chain.  A back-pointer block that lives
// in ``ws`` is first copied back into LDS with 16-byte loads.  The chunk's entries are packed into scalar registers, four to a
// word, and lane i then takes path[t0 + i]: the path goes out as
// coalesced stores, span boundaries (path[t] != path[t + 1]) are staged in LDS and stored at the end, and the score is the fp64
// sum of lp along the path (independent loads, a fixed-order reduction: reproducible; exact for integer-valued lp).
#include <type_traits>

#include "st_common.cuh"

namespace {

// the value of the lane below (lane 0: -inf) - DPP wave_shr:1, a register move            (as in csrc/st_ctc_loss.hip)
__device__ __forceinline__ float lane_below(float v) {
  return __int_as_float(__builtin_amdgcn_update_dpp(__float_as_int(-INFINITY), __float_as_int(v), 0x138, 0xf, 0xf, false));
}
// the maximum over the wave, in every lane, without the LDS crossbar: a running maximum along each row of 16 lanes (DPP row_shr
// 1, 2, 4, 8), the row totals carried across (row_bcast:15 into rows 1 and 3, row_bcast:31 into rows 2 and 3), lane 63 read out
__device__ __forceinline__ float wave_max_f(float v) {
  const int ninf = __float_as_int(-INFINITY);
  v = fmaxf(v, __int_as_float(__builtin_amdgcn_update_dpp(ninf, __float_as_int(v), 0x111, 0xf, 0xf, false)));
  v = fmaxf(v, __int_as_float(__builtin_amdgcn_update_dpp(ninf, __float_as_int(v), 0x112, 0xf, 0xf, false)));
  v = fmaxf(v, __int_as_float(__builtin_amdgcn_update_dpp(ninf, __float_as_int(v), 0x114, 0xf, 0xf, false)));
  v = fmaxf(v, __int_as_float(__builtin_amdgcn_update_dpp(ninf, __float_as_int(v), 0x118, 0xf, 0xf, false)));
  v = fmaxf(v, __int_as_float(__builtin_amdgcn_update_dpp(ninf, __float_as_int(v), 0x142, 0xa, 0xf, false)));
  v = fmaxf(v, __int_as_float(__builtin_amdgcn_update_dpp(ninf, __float_as_int(v), 0x143, 0xc, 0xf, false)));
  return __int_as_float(__builtin_amdgcn_readlane(__float_as_int(v), 63));
}

constexpr int RENORM = 8;                  // frames between two renormalisations (the chunk lengths are multiples)
constexpr int BP_LDS_BYTES = 128 * 1024;   // back-pointers held in LDS
constexpr int CLS_BYTES = 256 * 4;         // the clamped classes of the label positions
constexpr int SPAN_BYTES = 512 * 4;        // spans staged before their coalesced store
constexpr int BP_OFFSET = CLS_BYTES + SPAN_BYTES;      // (a multiple of 16: the block copy from ws stores 16 bytes per lane)
constexpr int WALK = 64;                   // frames per backtrace chunk: one path entry per lane

__host__ __device__ inline int align_pairs(int L) { return L <= 63 ? 1 : (L <= 127 ? 2 : 4); }
__host__ __device__ inline int align_bp_bytes(int L) { return align_pairs(L) == 4 ? 2 : 1; }      // per lane and frame
__host__ __device__ inline int align_lds_frames(int L) { return BP_LDS_BYTES / (64 * align_bp_bytes(L)); }
// ws: back-pointers [B][T][64] of the launch's word size, needed only when a frame count above the LDS capacity can occur
__host__ __device__ inline long long align_ws_bytes(int B, int T, int L) {
  return T > align_lds_frames(L) ? (long long)B * T * 64 * align_bp_bytes(L) : 0;
}

typedef uint4 __attribute__((may_alias)) bp_copy_t;      // the 16-byte pieces in which a block of back-pointers returns from ws

template <int P> struct BpWord { typedef unsigned char type; };
template <> struct BpWord<4> { typedef unsigned short type; };

template <int P, int CH>
__global__ __launch_bounds__(64) void ctc_align_kernel(const float* __restrict__ lp, int T, int C, const long long* __restrict__ classes,
                                                       int L, const int* __restrict__ in_len, const int* __restrict__ tgt_len,
                                                       unsigned char* __restrict__ ws, int* __restrict__ path,
                                                       int* __restrict__ spans, float* __restrict__ score) {
  typedef typename BpWord<P>::type bp_t;
  constexpr int F = BP_LDS_BYTES / (64 * (int)sizeof(bp_t));           // frames of back-pointers LDS holds
  constexpr int LOGP = P == 1 ? 0 : (P == 2 ? 1 : 2);
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  int* s_cls = (int*)smem;
  int* s_span = (int*)(smem + CLS_BYTES);
  bp_t* s_bp = (bp_t*)(smem + BP_OFFSET);
  const int b = blockIdx.x, lane = threadIdx.x;
  const int Tb = min(max(in_len[b], 0), T), tl = min(max(tgt_len[b], 0), L), S = 2 * tl + 1;
  const float* row0 = lp + (size_t)b * T * C;
  const long long* cls = classes + (size_t)b * L;
  int* pth = path + (size_t)b * T;
  const bool in_ws = Tb > F;                                           // (uniform) this utterance's back-pointers live in ws
  bp_t* g_bp = (bp_t*)ws + (size_t)b * T * 64;                         // (touched only when in_ws: then T > F and ws is sized)
  for (int j = lane; j < tl; j += 64) s_cls[j] = min(max((int)cls[j], 0), C - 1);
  for (int i = lane; i < 2 * L; i += 64) s_span[i] = -1;
  // pair q: blank state 2q (exists for q <= tl), label state 2q + 1 (q < tl).  The lanes past the last state run the same
  // arithmetic on values nobody reads (a state is fed from s, s - 1, s - 2 only: nothing flows back)
  int col[P];
  bool xb[P], xl[P], sk[P];
#pragma unroll
  for (int p = 0; p < P; ++p) {
    const int q = lane * P + p;
    xb[p] = q <= tl;
    xl[p] = q < tl;
    int c = 0, cp = -1;
    if (xl[p]) {
      c = min(max((int)cls[q], 0), C - 1);
      if (q > 0) cp = min(max((int)cls[q - 1], 0), C - 1);
    }
    col[p] = c;
    sk[p] = xl[p] && q > 0 && c != cp;
  }
  float ab[P], al[P];            // the state before frame 0: blank state 0 alone
#pragma unroll
  for (int p = 0; p < P; ++p) {
    ab[p] = (lane == 0 && p == 0) ? 0.f : -INFINITY;
    al[p] = -INFINITY;
  }
  float e0[CH], ec[CH][P], n0[CH], nc[CH][P];
  auto fetch = [&](int tau0, float (&f0)[CH], float (&fc)[CH][P]) {
#pragma unroll
    for (int k = 0; k < CH; ++k) {
      // (frames past the length re-read the last one: unconditional loads stay a chunk ahead, their values are never used)
      const float* r = row0 + (size_t)min(tau0 + k, Tb - 1) * C;
      f0[k] = r[0];
#pragma unroll
      for (int p = 0; p < P; ++p) fc[k][p] = r[col[p]];
    }
  };
  if (Tb > 0) fetch(0, e0, ec);
  // one chunk of frames; compiled four times - back-pointers to LDS or to ws, all CH frames inside the utterance or its ragged last
  // chunk - so that a frame of the common form carries no branch
  auto sweep = [&](auto ws_c, auto full_c, int tau0) {
    constexpr bool WS = decltype(ws_c)::value, FULL = decltype(full_c)::value;
#pragma unroll
    for (int k = 0; k < CH; ++k) {
      const int tau = tau0 + k;
      if (FULL || tau < Tb) {                    // (uniform)
        float pl = lane_below(al[P - 1]);
        unsigned word = 0;
#pragma unroll
        for (int p = 0; p < P; ++p) {
          // stay, s-1, s-2 in this order; a later candidate wins only if strictly greater
          float vb = ab[p];
          unsigned cb = 0;
          if (pl > vb) { vb = pl; cb = 1; }
          float vl = al[p];
          unsigned cl = 0;
          if (ab[p] > vl) { vl = ab[p]; cl = 1; }
          const float skip = sk[p] ? pl : -INFINITY;
          if (skip > vl) { vl = skip; cl = 2; }
          word |= (cb | (cl << 2)) << (4 * p);
          pl = al[p];
          ab[p] = e0[k] + vb;
          al[p] = ec[k][p] + vl;
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
        }
        if (WS) g_bp[(size_t)tau * 64 + lane] = (bp_t)word;
        else s_bp[tau * 64 + lane] = (bp_t)word;
      }
    }
  };
  for (int tau0 = 0; tau0 < Tb; tau0 += CH) {
    fetch(tau0 + CH, n0, nc);                    // the next chunk's emissions are in flight while this one is consumed
    const bool full = tau0 + CH <= Tb;
    if (in_ws) {
      if (full) sweep(std::true_type(), std::true_type(), tau0);
      else sweep(std::true_type(), std::false_type(), tau0);
    } else {
      if (full) sweep(std::false_type(), std::true_type(), tau0);
      else sweep(std::false_type(), std::false_type(), tau0);
    }
#pragma unroll
    for (int k = 0; k < CH; ++k) {
      e0[k] = n0[k];
#pragma unroll
      for (int p = 0; p < P; ++p) ec[k][p] = nc[k][p];
    }
  }
  // the end: the last blank S-1, or the last label S-2 if that is strictly better
  float vB = -INFINITY, vL = -INFINITY;
#pragma unroll
  for (int p = 0; p < P; ++p) {
    const int q = lane * P + p;
    if (q == tl) vB = ab[p];
    if (q == tl - 1) vL = al[p];
  }
  vB = wave_max_f(vB);
  vL = wave_max_f(vL);
  const bool feasible = Tb > 0 && fmaxf(vB, vL) > -INFINITY;
  __threadfence_block();
  __syncthreads();                               // back-pointers, s_cls and s_span are in place
  double acc = 0.0;
  if (feasible) {
    int s = __builtin_amdgcn_readfirstlane(vL > vB ? S - 2 : S - 1);
    int carry = -2;                              // path[t + 1] of the chunk's last frame (-2: there is none)
    for (int base = (Tb - 1) / F * F; base >= 0; base -= F) {         // (one block unless the back-pointers live in ws)
      const int n = min(F, Tb - base);
      if (in_ws) {                               // pull the block back through LDS: 16 bytes per lane and load
        __syncthreads();
        const bp_copy_t* src = (const bp_copy_t*)(g_bp + (size_t)base * 64);
        bp_copy_t* dst = (bp_copy_t*)s_bp;
        const int n16 = n * 64 * (int)sizeof(bp_t) / 16;
        for (int i = lane; i < n16; i += 64) dst[i] = src[i];
        __syncthreads();
      }
      for (int t0 = (base + n - 1) / WALK * WALK; t0 >= base; t0 -= WALK) {
        const int kmax = min(WALK - 1, base + n - 1 - t0);
        int w[WALK];
#pragma unroll
        for (int k = 0; k < WALK; ++k) w[k] = k <= kmax ? (int)s_bp[(t0 - base + k) * 64 + lane] : 0;
        int ent[WALK / 4];                       // (uniform) the chunk's path entries + 1, four to a word: scalar registers
#pragma unroll
        for (int g = 0; g < WALK / 4; ++g) ent[g] = 0;
#pragma unroll
        for (int k = WALK - 1; k >= 0; --k) {
          if (k <= kmax) {                       // (uniform) state s emits frame t0 + k
            ent[k >> 2] |= ((s & 1) ? ((s + 1) >> 1) : 0) << (8 * (k & 3));
            if (t0 + k > 0) {
              const int q = s >> 1;
              const int word = __builtin_amdgcn_readlane(w[k], q >> LOGP);
              s -= (word >> (4 * (q & (P - 1)) + 2 * (s & 1))) & 3;
            }
          }
        }
        int packed = 0;                          // lane i takes entry i: its word, then its byte (frames past kmax: 0 - 1 = -1)
#pragma unroll
        for (int g = 0; g < WALK / 4; ++g) packed = (lane >> 2) == g ? ent[g] : packed;
        const int mine = ((packed >> (8 * (lane & 3))) & 0xff) - 1;
        const int t = t0 + lane;
        const bool live = lane <= kmax;
        int nb = __shfl_down(mine, 1, 64);
        if (lane == kmax) nb = carry;
        if (live) {
          pth[t] = mine;
          if (mine != nb) {                      // a boundary between frames t and t + 1
            if (mine >= 0) s_span[2 * mine + 1] = t + 1;
            if (nb >= 0) s_span[2 * nb] = t + 1;
          }
          if (t == 0 && mine >= 0) s_span[2 * mine] = 0;
          acc += (double)row0[(size_t)t * C + (mine >= 0 ? s_cls[mine] : 0)];
        }
        carry = __builtin_amdgcn_readlane(mine, 0);
      }
    }
#pragma unroll
    for (int o = 32; o; o >>= 1) acc += __shfl_xor(acc, o, 64);
  }
  for (int t = (feasible ? Tb : 0) + lane; t < T; t += 64) pth[t] = -1;
  if (lane == 0) score[b] = feasible ? (float)acc : -INFINITY;
  __syncthreads();
  int* sp = spans + (size_t)b * L * 2;
  for (int i = lane; i < 2 * L; i += 64) sp[i] = s_span[i];
}

template <int P, int CH>
int launch_align(hipStream_t stream, const float* lp, int B, int T, int C, const long long* classes, int L, const int* in_len,
                 const int* tgt_len, void* ws, int* path, int* spans, float* score) {
  static bool attr_set = false;
  if (!attr_set) {
    (void)hipFuncSetAttribute(reinterpret_cast<const void*>(&ctc_align_kernel<P, CH>), hipFuncAttributeMaxDynamicSharedMemorySize,
                              BP_OFFSET + BP_LDS_BYTES);
    attr_set = true;
  }
  const int frames = T < align_lds_frames(L) ? T : align_lds_frames(L);
  const size_t smem = BP_OFFSET + (size_t)frames * 64 * align_bp_bytes(L);
  hipLaunchKernelGGL((ctc_align_kernel<P, CH>), dim3(B), dim3(64), smem, stream, lp, T, C, classes, L, in_len, tgt_len,
                     (unsigned char*)ws, path, spans, score);
  ST_CHECK_LAUNCH();
  return 0;
}

}  // namespace

extern "C" int st_ctc_align_ws_kib(int B, int T, int L) {
  if (B < 0 || T < 0 || L < 0 || L > 255) return -1;
  const long long kib = (align_ws_bytes(B, T, L) + 1023) / 1024;
  return kib > 0x7fffffffll ? -1 : (int)kib;
}

extern "C" int st_ctc_align(hipStream_t stream, const float* lp, int B, int T, int C, const long long* classes, int L, const int* in_len,
                            const int* tgt_len, void* ws, long long ws_bytes, int* path, int* spans, float* score) {
  if (B <= 0) return 0;
  if (!lp || !in_len || !tgt_len || !path || !score || T <= 0 || C < 2 || L < 0 || L > 255 || ((!classes || !spans) && L > 0)) return -1;
  const long long need = align_ws_bytes(B, T, L);
  if (need > 0 && (!ws || ws_bytes < need || ((size_t)ws & 15))) return -1;
  if (L <= 63) return launch_align<1, 16>(stream, lp, B, T, C, classes, L, in_len, tgt_len, ws, path, spans, score);
  if (L <= 127) return launch_align<2, 16>(stream, lp, B, T, C, classes, L, in_len, tgt_len, ws, path, spans, score);
  return launch_align<4, 8>(stream, lp, B, T, C, classes, L, in_len, tgt_len, ws, path, spans, score);
}
