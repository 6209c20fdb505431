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
//
// LANGUAGE MODEL (st_ctc_beam_search_lm: the kernel body with LM = true; the LM-less entry is the other instantiation: the
// instruction stream it had before the template, up to the encoding of two branches - LABNOTES 2026-10-21).  The search ranks
// a prefix h by log p_ctc,t(h) + G(h), G(h) = sum over its labels of
// fmaf(lambda, lm(h_i | BOS h_1 .. h_{i-1}), beta) with lm the back-off n-gram score of csrc/st_ngram.cuh.  G depends on the
// labels alone, so (pb, pnb) stay pure CTC numbers and a slot carries one more fp32, g: a stay keeps it, an extension p.c gets
// g(p) + fmaf(lambda, lm(c | hist(p)), beta), an extension that merges into a beam entry adds CTC mass only.  Selection keeps the
// `beam` best tot + g; the frame's normaliser is the largest CTC total among the kept (relative values stay <= 0).
//   what a walk costs is a chain of dependent global loads on the one wave's T-chain, so walks are made once per PREFIX, not
//   once per frame: every label buffer (a prefix keeps its buffer for as long as it lives in the beam, through every reordering)
//   owns the history of its prefix - tokens, valid length, the back-off of every context length: ONE walk_history when the slot
//   is created - and a 2-way x 32-set cache (token -> fmaf(lambda, lm, beta)).  Per frame the live extensions (not merged, not at
//   L_cap, not blank, CTC term > -inf) look their token up; the misses of ALL slots are compacted into a list and walked one per
//   lane, in parallel, and inserted (way = frame parity: two tokens of one set settle into the two ways).  Values are pure
//   functions of (prefix, token): the cache cannot change a result.
// After the last frame the EOS term fmaf(lambda, lm(EOS | hist(h)), beta) is added (final_eos) to g and to the rank the last frame
// selected by, and the beam is re-sorted by that, slot order on ties.
#include "st_ngram.cuh"

namespace {

constexpr int MAXB = 16;                   // beam slots
constexpr int MAXK = 16;                   // classes per row
constexpr int NBUF = 2 * MAXB;             // label buffers
constexpr int LSTRIDE = 256;               // labels per buffer (L_cap <= 255)
constexpr int CPL = 5;                     // candidates per lane: 64 x 5 >= 16 x 17
constexpr unsigned long long HASH_M = 0x9E3779B97F4A7C15ull;

constexpr int CSETS = 32;                  // sets of a prefix's (token -> weighted LM term) cache; 2 ways each
constexpr int CENT = 2 * CSETS;

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

struct LmArgs {
  Trie T;
  int H, bos, eos, final_eos;              // H = order - 1 history tokens
  float scale, bias;                       // lambda, beta
  float* fused;
  float* trace_g;
};

// fmaf(lambda, lm, beta); lambda = 0 never meets an infinite lm (st_ngram_score's rule)
__device__ __forceinline__ float lm_term(const LmArgs& A, float lm) { return A.scale > 0.f ? fmaf(A.scale, lm, A.bias) : A.bias; }

template <bool LM>
__global__ __launch_bounds__(64) void ctc_beam_kernel(const int* __restrict__ ids, const float* __restrict__ lp,
                                                      const float* __restrict__ lpb, const int* __restrict__ off,
                                                      const int* __restrict__ len, int K, int beam, int blank, int L_cap,
                                                      int* __restrict__ tokens, int* __restrict__ lens, float* __restrict__ score,
                                                      TraceRec* __restrict__ trace, double* __restrict__ trace_norm, int T_trace,
                                                      LmArgs A) {
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
  // LM state.  Per SLOT: g.  Per label BUFFER (it moves with its prefix): the history, most recent token first, its valid
  // length, its back-offs, and the cache {token, weighted term} (token -1: empty).  Per candidate: the weighted term of a miss,
  // then g of the candidate; the list of the frame's misses
  __shared__ float s_g[LM ? MAXB : 1];
  __shared__ int s_hh[LM ? NBUF * MAX_H : 1], s_hk[LM ? NBUF : 1];
  __shared__ float s_hbo[LM ? NBUF * MAX_H : 1];
  __shared__ __attribute__((aligned(8))) int2 s_cache[LM ? NBUF * CENT : 1];
  __shared__ float s_cg[LM ? 64 * CPL : 1];
  __shared__ short s_miss[LM ? 64 * CPL : 1];
  __shared__ float s_rank[LM ? MAXB : 1];
  __shared__ int s_pos[LM ? MAXB : 1];
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
  if constexpr (LM) {                      // the empty prefix (buffer 0): history (BOS), g = 0, an empty cache
    if (lane < MAXB) s_g[lane] = lane == 0 ? 0.f : -INFINITY;
    s_cache[lane] = make_int2(-1, 0);
    if (lane == 0) {
      int h[MAX_H] = {A.bos, -1, -1, -1};
      float bo[MAX_H];
      s_hk[0] = walk_history(A.T, h, A.H, bo);
#pragma unroll
      for (int j = 0; j < MAX_H; ++j) {
        s_hh[j] = h[j];
        s_hbo[j] = bo[j];
      }
    }
  }
  int nlive = 1;
  float myrank = lane == 0 ? 0.f : -INFINITY;   // (LM) the rank this slot was selected with in the last frame
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
    float tot[CPL], rk[CPL], wt[CPL];      // CTC total; rank = total + g (LM-less: the total); the weighted LM term
    unsigned missed = 0u;
    int nmiss = 0;
#pragma unroll
    for (int r = 0; r < CPL; ++r) {
      tot[r] = -INFINITY;
      wt[r] = 0.f;
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
          if constexpr (LM) {
            if (vnb > -INFINITY) {         // a live extension: its weighted term from the prefix's cache, or a miss
              if (A.scale > 0.f) {
                const int2* set = s_cache + s_buf[p] * CENT + 2 * (c & (CSETS - 1));
                const int2 e0 = set[0], e1 = set[1];
                if (e0.x == c) wt[r] = __int_as_float(e0.y);
                else if (e1.x == c) wt[r] = __int_as_float(e1.y);
                else missed |= 1u << r;
              } else {
                wt[r] = A.bias;
              }
            }
          }
        }
      }
      s_cpb[idx] = vb;
      s_cpnb[idx] = vnb;
      if constexpr (LM) {                  // the misses of the frame, compacted: one lane each below
        const unsigned long long mm = __ballot((missed >> r) & 1u);
        if ((missed >> r) & 1u) s_miss[nmiss + __popcll(mm & ((1ull << lane) - 1ull))] = (short)idx;
        nmiss += __popcll(mm);
      }
    }
    if constexpr (LM) {
      if (nmiss > 0) {                     // (uniform)
        __syncthreads();
        for (int i = lane; i < nmiss; i += 64) {
          const int idx = s_miss[i], p = (idx - beam) / K, c = s_fid[(idx - beam) % K], buf = s_buf[p];
          int h[MAX_H];
          float bo[MAX_H];
#pragma unroll
          for (int j = 0; j < MAX_H; ++j) {
            h[j] = s_hh[buf * MAX_H + j];
            bo[j] = s_hbo[buf * MAX_H + j];
          }
          const float w = lm_term(A, score_candidate(A.T, c, h, s_hk[buf], bo));
          s_cg[idx] = w;
          s_cache[buf * CENT + 2 * (c & (CSETS - 1)) + (t & 1)] = make_int2(c, __float_as_int(w));   // (one 8-byte store: never torn)
        }
        __syncthreads();
      }
#pragma unroll
      for (int r = 0; r < CPL; ++r) {
        rk[r] = -INFINITY;
        if (r >= nr) continue;             // (uniform)
        const int idx = lane + 64 * r, p = cp[r];
        if (p >= 0 && p < nlive) {
          if ((missed >> r) & 1u) wt[r] = s_cg[idx];
          const float gp = s_g[p], gc = cj[r] < 0 ? gp : gp + wt[r];
          rk[r] = tot[r] + gc;
          s_cg[idx] = gc;
        }
      }
    } else {
#pragma unroll
      for (int r = 0; r < CPL; ++r) rk[r] = tot[r];
    }
    // ---- E: the `beam` best totals, best first, lower candidate number on ties
    unsigned taken = 0u;
    int nsel = 0, mysel = 0;
    float m0 = -INFINITY;
    for (int round = 0; round < beam; ++round) {
      float v = -INFINITY, vt = -INFINITY;
      int br = 0;
#pragma unroll
      for (int r = 0; r < CPL; ++r)
        if (!((taken >> r) & 1u) && rk[r] > v) {
          v = rk[r];
          if constexpr (LM) vt = tot[r];
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
      if constexpr (LM) myrank = lane == round ? m : myrank;
      if constexpr (LM) m0 = fmaxf(m0, __int_as_float(__builtin_amdgcn_readlane(__float_as_int(vt), __builtin_amdgcn_readfirstlane(w))));   // the largest CTC total kept
      else if (round == 0) m0 = m;
      ++nsel;
    }
    const bool live = lane < nsel;
    if (live && mysel < beam) s_new[mysel] = lane;
    __syncthreads();                       // (s_cpb / s_cpnb / s_new are in place)
    // ---- F: the new beam
    int par = -1, tok = -1, o_last = -1, o_len = 0, o_buf = 0, npar = -1;
    unsigned long long o_hash = 0;
    float npb = -INFINITY, npnb = -INFINITY, ng = -INFINITY;
    int ph[MAX_H] = {-1, -1, -1, -1};
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
      if constexpr (LM) {
        ng = s_cg[mysel];
        if (tok >= 0) {                    // the history of the new prefix: its label, then its parent's
          ph[0] = tok;
#pragma unroll
          for (int j = 1; j < MAX_H; ++j) ph[j] = s_hh[o_buf * MAX_H + j - 1];
        }
      }
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
      if constexpr (LM) s_cache[of_lane(nbuf, l) * CENT + lane] = make_int2(-1, 0);     // a new prefix: an empty cache
      seq = nxt;
    }
    if constexpr (LM) {
      if (is_ext) {                        // ... and ONE walk of its history, the new slots in parallel (a new buffer is no old one)
        float bo[MAX_H];
        s_hk[nbuf] = walk_history(A.T, ph, A.H, bo);
#pragma unroll
        for (int j = 0; j < MAX_H; ++j) {
          s_hh[nbuf * MAX_H + j] = ph[j];
          s_hbo[nbuf * MAX_H + j] = bo[j];
        }
      }
      if (lane < MAXB) s_g[lane] = ng;
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
      if constexpr (LM)
        if (A.trace_g && lane < beam) A.trace_g[((size_t)b * T_trace + t) * beam + lane] = ng;
    }
    __syncthreads();
  }
  // ---- the n-best: slots are in selection order = best first
  if constexpr (!LM) {
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
  } else {
    // ---- with the LM: the EOS term (one walk per live slot, in parallel) joins the rank the last frame selected by (total + g,
    //      both relative to the frame before: slot order = that rank's order), then best first, slot order on ties (a rank of
    //      -inf - EOS vetoed - goes last among the live ones).  Without the EOS term, or with lambda = beta = 0, nothing moves
    float rel = -INFINITY, fu = -INFINITY, key = -INFINITY;
    if (lane < nlive) {
      rel = logadd(s_pb[lane], s_pnb[lane]);
      fu = s_g[lane];
      key = myrank;
      if (A.final_eos) {
        const int buf = s_buf[lane];
        int h[MAX_H];
        float bo[MAX_H];
#pragma unroll
        for (int j = 0; j < MAX_H; ++j) {
          h[j] = s_hh[buf * MAX_H + j];
          bo[j] = s_hbo[buf * MAX_H + j];
        }
        const float e = lm_term(A, score_candidate(A.T, A.eos, h, s_hk[buf], bo));
        fu += e;
        key += e;
      }
    }
    if (lane < MAXB) s_rank[lane] = key;
    __syncthreads();
    if (lane < MAXB) {
      int pos = lane;
      if (lane < nlive) {
        const float mine = s_rank[lane];
        pos = 0;
        for (int j = 0; j < nlive; ++j) pos += (s_rank[j] > mine || (s_rank[j] == mine && j < lane)) ? 1 : 0;
      }
      s_pos[lane] = pos;
      if (lane < beam) {
        const bool live = lane < nlive;
        lens[(size_t)b * beam + pos] = live ? s_len[lane] : 0;
        score[(size_t)b * beam + pos] = live ? (float)(norm + (double)rel) : -INFINITY;
        A.fused[(size_t)b * beam + pos] = fu;
      }
    }
    __syncthreads();
    for (int r = 0; r < beam; ++r) {
      const int n = r < nlive ? s_len[r] : 0;
      const int* a = s_seq + s_buf[r] * LSTRIDE;
      int* out = tokens + ((size_t)b * beam + s_pos[r]) * L_cap;
      for (int i = lane; i < L_cap; i += 64) out[i] = i < n ? a[i] : -1;
    }
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
  hipLaunchKernelGGL(ctc_beam_kernel<false>, dim3(B), dim3(64), 0, stream, ids, lp, lpb, off, len, K, beam, blank, L_cap, tokens,
                     lens, score, (TraceRec*)trace, trace_norm, T_trace, LmArgs{});
  ST_CHECK_LAUNCH();
  return 0;
}

extern "C" int st_ctc_beam_search_lm(hipStream_t stream, const int* ids, const float* lp, const float* lpb, const int* off,
                                     const int* len, int B, int K, int beam, int blank, int L_cap, int* tokens, int* lens, float* score,
                                     void* trace, double* trace_norm, int T_trace, const int* child_lo, const int* tok,
                                     const float* logp, const float* bo, int nodes, int V, int order, float oov_logp, int bos, int eos,
                                     float scale, float bias, int final_eos, float* fused, float* trace_g) {
  if (B <= 0) return 0;
  if (!ids || !lp || !lpb || !off || !len || !tokens || !lens || !score || K < 1 || K > MAXK || !beam_shape_ok(B, 0, beam, L_cap))
    return -1;
  if (trace && (!trace_norm || T_trace < 1)) return -1;
  if (!trie_ok(child_lo, tok, logp, bo, nodes, V, order) || !(oov_logp <= 0.f) || !(scale >= 0.f) || !(scale < INFINITY) ||
      !(bias == bias) || !(fabsf(bias) < INFINITY) || !fused || (trace_g && !trace))
    return -1;
  LmArgs A;
  A.T = Trie{child_lo, tok, logp, bo, nodes, V, oov_logp};
  A.H = order - 1;
  A.bos = bos;
  A.eos = eos;
  A.final_eos = final_eos;
  A.scale = scale;
  A.bias = bias;
  A.fused = fused;
  A.trace_g = trace_g;
  hipLaunchKernelGGL(ctc_beam_kernel<true>, dim3(B), dim3(64), 0, stream, ids, lp, lpb, off, len, K, beam, blank, L_cap, tokens,
                     lens, score, (TraceRec*)trace, trace_norm, T_trace, A);
  ST_CHECK_LAUNCH();
  return 0;
}
