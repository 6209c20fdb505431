// CTC prefix beam search (Graves; Hannun et al. 2014) over the K best classes of every encoder row: per utterance the `beam` most
// probable LABEL PREFIXES, each the sum over all its alignments, with scores - the encoder-only first pass of a two-pass
// recogniser.  Inputs are what st_beam_pre_beam leaves for the CTC head's logits (ids / lp [R][K]) plus the blank's
// log-probability per row; lengths and offsets are device-resident: nothing is read from host memory, the launch can be captured.
//
// One WAVE per utterance, T dependent frames.  A beam slot holds (pb, pnb) - the log-probability of its alignments that end in
// blank / in its last label - RELATIVE to the best total of the frame before; the running normaliser is an fp64 scalar, so the
// resolution between hypotheses does not decay with T.  Per frame:
//   candidates  stay s (number s): pb' = total(s) + lpb, pnb' = pnb(s) + x(last(s)) if last(s) is among the row's K best;
//               extension (p, j) (number beam + p K + j), c = ids[j] != blank, len(p) < L_cap: pnb' = (c == last(p) ? pb(p) :
//               total(p)) + x(c).  At most beam (K + 1) = 272: lane l owns the numbers l, l + 64, ... (rounds past the last candidate
//               are skipped; the stay candidates, the only ones with two sides to add, all sit in round 0).
//   merging     an extension p.c that spells the labels of a beam entry q adds into q's pnb' (after q's own repeat term: candidate
//               order) and is no candidate of its own.  Only p = q without its last label can do that, and the beam holds distinct
//               prefixes, so at most one extension lands on each q.  IDENTITY IS BY LABELS, not by lineage: every slot keeps its
//               label sequence in an LDS buffer, its length and a 64-bit rolling hash; (len(p) + 1 == len(q), c == last(q),
//               hash(p) M + c + 1 == hash(q)) selects the pairs, and the wave then compares the two sequences label by label - a
//               hash collision costs a compare, never a wrong merge, and a prefix that left the beam and came back through its own
//               parent still meets its child.  The compare is rare: a slot remembers in which slot its parent prefix sits (it was
//               extended from it, or was compared with it once), the update carries that through the beam's reordering, and only
//               a slot that does not know its parent is searched for one.
//   selection   `beam` rounds of a wave maximum of the totals (DPP), then the lowest round and lane among the equal ones: best
//               first, lower candidate number on ties; a total of -inf is never kept.
//   update      a kept stay keeps its label buffer; a kept extension takes a free one (32 buffers: the 16 of the old beam are not
//               reused within the frame, a dropped parent can still be copied from) and copies its parent's labels.
// No back-pointer records and no backtrace: the labels of the final beam are in LDS, and any number of frames fits (no workspace).
// Arithmetic: fp32, natural units; log-sums as max + log(1 + exp(min - max)) on the hardware's exp2 / log2; fixed order, no float
// atomics: two launches are bit-equal.  The rows of the next three frames are in flight while a frame is processed.
#include "st_common.cuh"

namespace {

constexpr int MAXB = 16;                   // beam slots
constexpr int MAXK = 16;                   // classes per row
constexpr int NBUF = 2 * MAXB;             // label buffers
constexpr int LSTRIDE = 256;               // labels per buffer (L_cap <= 255)
constexpr int CPL = 5;                     // candidates per lane: 64 x 5 >= 16 x 17
constexpr unsigned long long HASH_M = 0x9E3779B97F4A7C15ull;

struct TraceRec {
  int prev, token;
  float pb, pnb;
};

// the maximum over the wave, in every lane (DPP row_shr 1, 2, 4, 8, row_bcast 15 / 31, lane 63 read out: csrc/st_ctc_align.hip)
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

__device__ __forceinline__ float logadd(float a, float b) {
  const float m = fmaxf(a, b), n = fminf(a, b);
  if (n == -INFINITY) return m;
  // the hardware's exp2 / log2 (1 ulp each) around a sum in [1, 2]: absolute error <= 5 x 2^-24 before the final add (the budget
  // tests/_ctc_beam_ref.py derives); the library's expf / log1pf cost ~100 instructions a log-sum on a chain of T frames
  return m + __logf(1.f + __expf(n - m));
}

__global__ __launch_bounds__(64) void ctc_beam_kernel(const int* __restrict__ ids, const float* __restrict__ lp,
                                                      const float* __restrict__ lpb, const int* __restrict__ off,
                                                      const int* __restrict__ len, int K, int beam, int blank, int L_cap,
                                                      int* __restrict__ tokens, int* __restrict__ lens, float* __restrict__ score,
                                                      TraceRec* __restrict__ trace, double* __restrict__ trace_norm, int T_trace) {
  __shared__ __attribute__((aligned(16))) int s_seq[NBUF * LSTRIDE];
  __shared__ float s_pb[MAXB], s_pnb[MAXB], s_tot[MAXB];
  __shared__ int s_last[MAXB], s_len[MAXB], s_buf[MAXB], s_jq[MAXB], s_merge[MAXB];
  __shared__ int s_par[MAXB];              // the slot that holds this slot's labels without the last one, where that is KNOWN (else -1)
  __shared__ int s_new[MAXB];              // where an old slot's own prefix went in the new beam (-1: dropped)
  __shared__ unsigned long long s_hash[MAXB];
  __shared__ unsigned s_dead[MAXB];        // bit j: extension (p, j) has merged into a beam entry
  __shared__ float s_cpb[64 * CPL], s_cpnb[64 * CPL];
  __shared__ int s_fid[MAXK];
  __shared__ float s_flp[MAXK];
  const int b = blockIdx.x, lane = threadIdx.x;
  const int Tb = max(len[b], 0);
  const size_t row0 = (size_t)max(off[b], 0);
  const int ncand = beam + beam * K;
  // the candidates of this lane: parent slot and class index (stay: j = -1; past the last candidate: p = -1)
  const int nr = (ncand + 63) >> 6;        // rounds of 64 candidates: lane l owns the numbers l, l + 64, ...
  int cp[CPL], cj[CPL];
#pragma unroll
  for (int r = 0; r < CPL; ++r) {
    const int idx = lane + 64 * r;
    cp[r] = idx < beam ? idx : (idx < ncand ? (idx - beam) / K : -1);
    cj[r] = idx < beam || idx >= ncand ? -1 : (idx - beam) % K;
  }
  if (lane < MAXB) {                       // the empty prefix in slot 0
    s_pb[lane] = lane == 0 ? 0.f : -INFINITY;
    s_pnb[lane] = -INFINITY;
    s_last[lane] = -1;
    s_len[lane] = 0;
    s_hash[lane] = 0;
    s_buf[lane] = 0;
    s_par[lane] = -1;
  }
  int nlive = 1;
  unsigned used = 1u;                      // label buffers of the live slots
  double norm = 0.0;
  // lanes 0 .. K-1 carry a row's ids, 16 .. 16+K-1 its lp, lane 32 its blank: one load per lane and frame, three frames ahead
  auto fetch = [&](int t) -> int {
    const size_t row = row0 + (size_t)min(t, Tb - 1);      // (frames past the length re-read the last one; never used)
    int v = 0;
    if (lane < K) v = ids[row * K + lane];
    else if (lane >= 16 && lane < 16 + K) v = __float_as_int(lp[row * K + lane - 16]);
    else if (lane == 32) v = __float_as_int(lpb[row]);
    return v;
  };
  int cur = 0, n1 = 0, n2 = 0;
  if (Tb > 0) {
    cur = fetch(0);
    n1 = fetch(1);
    n2 = fetch(2);
  }
  __syncthreads();
  for (int t = 0; t < Tb; ++t) {
    const int n3 = fetch(t + 3);
    // ---- A: the frame's row into LDS
    if (lane < K) s_fid[lane] = cur;
    else if (lane >= 16 && lane < 16 + K) s_flp[lane - 16] = __int_as_float(cur);
    const float lpb_t = __int_as_float(__builtin_amdgcn_readlane(cur, 32));
    cur = n1;
    n1 = n2;
    n2 = n3;
    __syncthreads();
    // ---- B: per slot: total, the place of its last label among the row's classes
    if (lane < MAXB) {
      s_tot[lane] = logadd(s_pb[lane], s_pnb[lane]);
      int jq = -1;
      const int last = s_last[lane];
      if (lane < nlive && last >= 0 && last != blank)
        for (int j = K - 1; j >= 0; --j) jq = s_fid[j] == last ? j : jq;
      s_jq[lane] = jq;
      s_merge[lane] = -1;
      s_dead[lane] = 0u;
      s_new[lane] = -1;
    }
    __syncthreads();
    // ---- C: which extension p.c spells the labels of which beam entry q.  Where q's parent prefix is known to sit in slot
    //         s_par[q] (q was extended from it, or an earlier frame compared them; the update below follows both through the
    //         beam) nothing is searched ...
    if (lane < nlive && s_par[lane] >= 0 && s_jq[lane] >= 0) {
      s_merge[lane] = s_par[lane];
      atomicOr(&s_dead[s_par[lane]], 1u << s_jq[lane]);      // (several q may share a parent; integer OR: order-free)
    }
    __syncthreads();
    //         ... else the pairs (q, p) = (pair >> 4, pair & 15) are filtered by length, last label and hash, and the wave compares
    //         the two label sequences, four labels per lane and pass
    for (int r = 0; 4 * r < nlive; ++r) {  // (64 pairs = 4 values of q per pass)
      const int q = (lane + 64 * r) >> 4, p = lane & 15;
      bool hit = false;
      if (q < nlive && p < nlive && p != q && s_par[q] < 0 && s_jq[q] >= 0 && s_len[p] + 1 == s_len[q])
        hit = s_hash[p] * HASH_M + (unsigned long long)(s_last[q] + 1) == s_hash[q];
      unsigned long long mask = __ballot(hit);
      while (mask) {                       // (uniform)
        const int pair = __ffsll((long long)mask) - 1 + 64 * r;
        mask &= mask - 1;
        const int qq = pair >> 4, pp = pair & 15, n = s_len[pp];
        const int4* a = (const int4*)(s_seq + s_buf[pp] * LSTRIDE);
        const int4* c = (const int4*)(s_seq + s_buf[qq] * LSTRIDE);
        bool diff = false;
        for (int i = lane; 4 * i < n; i += 64) {             // (labels past n: whatever the buffers hold - masked)
          const int4 x = a[i], y = c[i];
          diff |= x.x != y.x || (4 * i + 1 < n && x.y != y.y) || (4 * i + 2 < n && x.z != y.z) || (4 * i + 3 < n && x.w != y.w);
        }
        if (!__any(diff) && lane == 0) {
          s_merge[qq] = pp;
          s_par[qq] = pp;
          s_dead[pp] |= 1u << s_jq[qq];
        }
      }
    }
    __syncthreads();
    // ---- D: the candidates
    float tot[CPL];
#pragma unroll
    for (int r = 0; r < CPL; ++r) {
      tot[r] = -INFINITY;
      if (r >= nr) continue;               // (uniform)
      const int idx = lane + 64 * r, p = cp[r], j = cj[r];
      float vb = -INFINITY, vnb = -INFINITY;
      if (p >= 0 && p < nlive) {
        if (j < 0) {                       // stay (round 0 only): blank, repeat, and the extension that spells the same labels
          vb = s_tot[p] + lpb_t;
          const int jq = s_jq[p];
          if (jq >= 0) vnb = s_pnb[p] + s_flp[jq];
          const int m = s_merge[p];
          if (m >= 0) vnb = logadd(vnb, (s_last[p] == s_last[m] ? s_pb[m] : s_tot[m]) + s_flp[jq]);
          tot[r] = logadd(vb, vnb);
        } else {                           // an extension ends in its label: its total is pnb
          const int c = s_fid[j];
          if (c != blank && s_len[p] < L_cap && !((s_dead[p] >> j) & 1u)) vnb = (c == s_last[p] ? s_pb[p] : s_tot[p]) + s_flp[j];
          tot[r] = vnb;
        }
      }
      s_cpb[idx] = vb;
      s_cpnb[idx] = vnb;
    }
    // ---- E: the `beam` best totals, best first, lower candidate number on ties
    unsigned taken = 0u;
    int nsel = 0, mysel = 0;
    float m0 = -INFINITY;
    for (int round = 0; round < beam; ++round) {
      float v = -INFINITY;
      int br = 0;
#pragma unroll
      for (int r = 0; r < CPL; ++r)
        if (!((taken >> r) & 1u) && tot[r] > v) {
          v = tot[r];
          br = r;
        }
      const float m = wave_max_f(v);
      if (!(m > -INFINITY)) break;
      unsigned long long eq = 0ull;        // the lowest number among the equal ones: the lowest round, then the lowest lane
      int wr = 0;
      for (; wr < nr; ++wr) {
        eq = __ballot(v == m && br == wr);
        if (eq) break;
      }
      if (!eq) break;
      const int w = __ffsll((long long)eq) - 1;
      const int widx = w + 64 * wr;
      if (lane == w) taken |= 1u << br;
      if (lane == round) mysel = widx;
      if (round == 0) m0 = m;
      ++nsel;
    }
    const bool live = lane < nsel;
    if (live && mysel < beam) s_new[mysel] = lane;
    __syncthreads();                       // (s_cpb / s_cpnb / s_new are in place)
    // ---- F: the new beam
    int par = -1, tok = -1, o_last = -1, o_len = 0, o_buf = 0, npar = -1;
    unsigned long long o_hash = 0;
    float npb = -INFINITY, npnb = -INFINITY;
    if (live) {
      if (mysel < beam) par = mysel;
      else {
        par = (mysel - beam) / K;
        tok = s_fid[(mysel - beam) % K];
      }
      o_last = s_last[par];
      o_len = s_len[par];
      o_buf = s_buf[par];
      o_hash = s_hash[par];
      npb = s_cpb[mysel] - m0;
      npnb = s_cpnb[mysel] - m0;
      // the slot of the parent prefix in the new beam: a kept prefix keeps the one it knew, an extension knows its maker
      const int known = tok >= 0 ? par : s_par[par];
      npar = known >= 0 ? s_new[known] : -1;
    }
    const bool is_ext = live && tok >= 0;
    const unsigned long long exts = __ballot(is_ext);
    int nbuf = o_buf;
    if (is_ext) {                          // the rank-th free buffer (the old beam's buffers stay readable)
      unsigned f = ~used;
      for (int i = __popcll(exts & ((1ull << lane) - 1ull)); i > 0; --i) f &= f - 1u;
      nbuf = __ffs((int)f) - 1;
    }
    __syncthreads();                       // (every lane has read the old slots)
    // a buffer is 64 lanes x 16 bytes: one pass per extension copies all of it (labels past n: whatever the parent's buffer holds);
    // a destination is never a source, so the next parent's labels are read before this one's are stored
    // (the lane of an extension is wave-uniform: its registers are read with v_readlane, not through the LDS crossbar)
    auto of_lane = [](int v, int l) { return __builtin_amdgcn_readlane(v, __builtin_amdgcn_readfirstlane(l)); };
    int4 seq = make_int4(0, 0, 0, 0);
    if (exts) seq = ((const int4*)(s_seq + of_lane(o_buf, __ffsll((long long)exts) - 1) * LSTRIDE))[lane];
    for (unsigned long long mask = exts; mask; mask &= mask - 1) {
      const int l = __ffsll((long long)mask) - 1;
      const int dst = of_lane(nbuf, l) * LSTRIDE, n = of_lane(o_len, l), tk = of_lane(tok, l);
      const unsigned long long rest = mask & (mask - 1);
      int4 nxt = seq;
      if (rest) nxt = ((const int4*)(s_seq + of_lane(o_buf, __ffsll((long long)rest) - 1) * LSTRIDE))[lane];
      int4 v = seq;
      if ((n >> 2) == lane) {              // the new label goes out with its lane's 16 bytes
        const int k = n & 3;
        v.x = k == 0 ? tk : v.x;
        v.y = k == 1 ? tk : v.y;
        v.z = k == 2 ? tk : v.z;
        v.w = k == 3 ? tk : v.w;
      }
      ((int4*)(s_seq + dst))[lane] = v;
      seq = nxt;
    }
    if (lane < MAXB) {
      s_par[lane] = npar;
      s_pb[lane] = npb;
      s_pnb[lane] = npnb;
      s_last[lane] = live ? (tok >= 0 ? tok : o_last) : -1;
      s_len[lane] = live ? o_len + (tok >= 0 ? 1 : 0) : 0;
      s_hash[lane] = live ? (tok >= 0 ? o_hash * HASH_M + (unsigned long long)(tok + 1) : o_hash) : 0ull;
      s_buf[lane] = live ? nbuf : 0;
    }
    used = 0u;
    for (int s = 0; s < nsel; ++s) used |= 1u << of_lane(nbuf, s);
    nlive = nsel;
    if (nsel > 0) norm += (double)m0;
    if (trace && t < T_trace) {
      if (lane < beam) {
        TraceRec rec;
        rec.prev = par;
        rec.token = tok;
        rec.pb = npb;
        rec.pnb = npnb;
        trace[((size_t)b * T_trace + t) * beam + lane] = rec;
      }
      if (lane == 0) trace_norm[(size_t)b * T_trace + t] = norm;
    }
    __syncthreads();
  }
  // ---- the n-best: slots are in selection order = best first
  if (lane < beam) {
    const bool live = lane < nlive;
    lens[(size_t)b * beam + lane] = live ? s_len[lane] : 0;
    score[(size_t)b * beam + lane] = live ? (float)(norm + (double)logadd(s_pb[lane], s_pnb[lane])) : -INFINITY;
  }
  for (int r = 0; r < beam; ++r) {
    const int n = r < nlive ? s_len[r] : 0;
    const int* a = s_seq + s_buf[r] * LSTRIDE;
    int* out = tokens + ((size_t)b * beam + r) * L_cap;
    for (int i = lane; i < L_cap; i += 64) out[i] = i < n ? a[i] : -1;
  }
}

bool beam_shape_ok(int B, int T, int beam, int L_cap) {
  return B >= 0 && T >= 0 && beam >= 1 && beam <= MAXB && L_cap >= 1 && L_cap < LSTRIDE;
}

}  // namespace

extern "C" int st_ctc_beam_ws_kib(int B, int T, int beam, int L_cap) { return beam_shape_ok(B, T, beam, L_cap) ? 0 : -1; }

extern "C" int st_ctc_beam_search(hipStream_t stream, const int* ids, const float* lp, const float* lpb, const int* off, const int* len,
                                  int B, int K, int beam, int blank, int L_cap, int* tokens, int* lens, float* score, void* trace,
                                  double* trace_norm, int T_trace) {
  if (B <= 0) return 0;
  if (!ids || !lp || !lpb || !off || !len || !tokens || !lens || !score || K < 1 || K > MAXK || !beam_shape_ok(B, 0, beam, L_cap))
    return -1;
  if (trace && (!trace_norm || T_trace < 1)) return -1;
  hipLaunchKernelGGL(ctc_beam_kernel, dim3(B), dim3(64), 0, stream, ids, lp, lpb, off, len, K, beam, blank, L_cap, tokens, lens,
                     score, (TraceRec*)trace, trace_norm, T_trace);
  ST_CHECK_LAUNCH();
  return 0;
}
