// HBM-bound companions of the MFMA kernels (gfx950): LayerNorm backward, column sums
// (bias gradients), embedding + positional encoding, ragged pack / unpack, fp32 -> bf16
// parameter shadow.  All of them stream rows with >= 8-byte per-lane accesses along the
// feature axis (coalesced 256-512 B per wave per row).
#include "st_common.cuh"
#include "st_ce.cuh"

#ifndef ST_ADAM_SC1
#define ST_ADAM_SC1 0      // development: st_zero's stores write-through (store16_wt), as the optimizer kernels' switch of st_optim.cuh
#endif

namespace {

// ---------------------------------------------------------------------------------------------
// LayerNorm backward (nn.LayerNorm(d, eps=1e-6) of Attention.py:62,94 / SubLayers.py:18,27 /
// Models.py:32).  With g = dy * gamma:
//   dx = rstd * (g - mean(g) - xhat * mean(g * xhat))
//   dgamma += sum_rows dy * xhat,  dbeta += sum_rows dy,  dbias += sum_rows dx
// (dbias is the bias gradient of the Linear that feeds the LN: same column sum, free here.)
// `mask` (optional, bf16 [M,N]): dx is zeroed where mask <= 0 - the ReLU that sits between the
// Linear and the LN in the encoder front-end (Models.py:28-33).
// Each lane owns 8 consecutive columns (16-byte loads); a row takes N/8 lanes, so a wave streams
// 64 / (N/8) rows at a time and two such row groups are in flight per iteration.
// ---------------------------------------------------------------------------------------------
template <int N, bool DROP>
__global__ __launch_bounds__(256) void ln_bwd_kernel(const bf16* __restrict__ dy, int lddy,
                                                     const bf16* __restrict__ xhat, const float* __restrict__ rstd,
                                                     const float* __restrict__ gamma, const bf16* __restrict__ mask,
                                                     bf16* __restrict__ dx, int lddx, float* dgamma, float* dbeta,
                                                     float* dbias, int M, DropArgs drop, float mask_scale) {
  constexpr int LPR = N / 8;        // lanes per row
  constexpr int RPW = 64 / LPR;     // rows per wave per pass
  constexpr int UNR = 2;
  __shared__ float red[3][4 * RPW][N];
  const int wave = threadIdx.x >> 6, l = threadIdx.x & 63;
  const int slot = l / LPR, c0 = (l % LPR) * 8;
  float gm[8], ag[8], ab[8], ax[8];
#pragma unroll
  for (int e = 0; e < 8; ++e) { gm[e] = gamma[c0 + e]; ag[e] = ab[e] = ax[e] = 0.f; }
  const Drop dr = make_drop(drop);   // dropout on the LayerNorm OUTPUT (SubLayers.py:27): dy <- dy * keep / (1-p)

  const int stride = gridDim.x * 4 * RPW * UNR;
  for (int base = (blockIdx.x * 4 + wave) * RPW * UNR; base < M; base += stride) {
    bf16x8 vdy[UNR], vxh[UNR], vmk[UNR];
    float rs[UNR];
    bool ok[UNR];
#pragma unroll
    for (int u = 0; u < UNR; ++u) {
      const int row = base + u * RPW + slot;
      ok[u] = row < M;
      vdy[u] = gload8(dy + (size_t)row * lddy + c0, ok[u]);
      vxh[u] = gload8(xhat + (size_t)row * N + c0, ok[u]);
      if (mask) vmk[u] = gload8(mask + (size_t)row * N + c0, ok[u]);
      rs[u] = ok[u] ? rstd[row] : 0.f;
    }
#pragma unroll
    for (int u = 0; u < UNR; ++u) {
      const int row = base + u * RPW + slot;
      float g[8], xh[8], s1 = 0.f, s2 = 0.f;
      uint32_t bits[2] = {0, 0};
      if (DROP) {
        bits[0] = dr.bits(drop_counter_rc(row, c0, N));
        bits[1] = dr.bits(drop_counter_rc(row, c0 + 4, N));
      }
#pragma unroll
      for (int e = 0; e < 8; ++e) {
        float d = (float)vdy[u][e];
        if (DROP) d = dr.keep(bits[e >> 2], e & 3) ? d * dr.scale : 0.f;
        xh[e] = (float)vxh[u][e];
        g[e] = d * gm[e];
        s1 += g[e];
        s2 += g[e] * xh[e];
        ag[e] += d * xh[e];
        ab[e] += d;
      }
#pragma unroll
      for (int o = LPR / 2; o >= 1; o >>= 1) {
        s1 += __shfl_xor(s1, o, 64);
        s2 += __shfl_xor(s2, o, 64);
      }
      const float m1 = s1 * (1.f / N), m2 = s2 * (1.f / N);
      bf16x8 out;
#pragma unroll
      for (int e = 0; e < 8; ++e) {
        float v = rs[u] * (g[e] - m1 - xh[e] * m2);
        if (mask) v = ((float)vmk[u][e] > 0.f) ? v * mask_scale : 0.f;   // ReLU (+dropout) in front of the LN (front-end)
        out[e] = (bf16)v;
        ax[e] += v;
      }
      if (ok[u]) *reinterpret_cast<bf16x8*>(dx + (size_t)row * lddx + c0) = out;
    }
  }
#pragma unroll
  for (int e = 0; e < 8; ++e) {
    red[0][wave * RPW + slot][c0 + e] = ag[e];
    red[1][wave * RPW + slot][c0 + e] = ab[e];
    red[2][wave * RPW + slot][c0 + e] = ax[e];
  }
  __syncthreads();
  for (int c = threadIdx.x; c < N; c += 256) {
    float t0 = 0.f, t1 = 0.f, t2 = 0.f;
#pragma unroll
    for (int k = 0; k < 4 * RPW; ++k) { t0 += red[0][k][c]; t1 += red[1][k][c]; t2 += red[2][k][c]; }
    if (dgamma) atomicAdd(dgamma + c, t0);
    if (dbeta) atomicAdd(dbeta + c, t1);
    if (dbias) atomicAdd(dbias + c, t2);
  }
}

// row_pos[off[b] + t] = t, row_seq[off[b] + t] = b  for t < len[b]
__global__ void row_index_kernel(const int* off, const int* len, int* row_pos, int* row_seq) {
  const int b = blockIdx.y, t = blockIdx.x * blockDim.x + threadIdx.x;
  if (t < len[b]) {
    row_pos[off[b] + t] = t;
    if (row_seq) row_seq[off[b] + t] = b;
  }
}

// Ragged pack: padded fp32 [B, T, F] -> row matrix bf16 [rows, F] (Models.py:42 input, train.py:33).
// A 256-thread workgroup takes `rpb` consecutive frames of one utterance (a frame of 80 features is 20 float4 chunks: one
// workgroup per frame is 32,000 workgroups of 20 busy lanes - 19 us of dispatch for 14 MB).
__global__ __launch_bounds__(256) void pack_rows_kernel(const float* __restrict__ x, int T, int F, int rpb, const int* off,
                                                        const int* len, bf16* __restrict__ out) {
  const int b = blockIdx.z, cpr = F >> 2;                       // float4 chunks per frame
  const int cw = min(cpr, 256);                                 // chunks of a frame handled per pass
  const int t = blockIdx.y * rpb + (int)threadIdx.x / cw;
  if ((int)threadIdx.x >= rpb * cw || t >= len[b]) return;
  const float* src = x + ((size_t)b * T + t) * F;
  bf16* dst = out + (size_t)(off[b] + t) * F;
  for (int c = (int)threadIdx.x % cw; c < cpr; c += cw) {
    const f32x4 v = *reinterpret_cast<const f32x4*>(src + 4 * c);
    bf16x4 o = {(bf16)v[0], (bf16)v[1], (bf16)v[2], (bf16)v[3]};
    *reinterpret_cast<bf16x4*>(dst + 4 * c) = o;
  }
}

// Ragged unpack: bf16 row matrix [rows, D] -> padded fp32 [B, T, D], zero past len[b].
__global__ void unpack_rows_kernel(const bf16* __restrict__ x, int ld, int T, int D, const int* off, const int* len,
                                   float* __restrict__ out) {
  const int b = blockIdx.z, t = blockIdx.y;
  const bool ok = t < len[b];
  const bf16* src = x + (size_t)(off[b] + (ok ? t : 0)) * ld;
  float* dst = out + ((size_t)b * T + t) * D;
  for (int f = threadIdx.x * 4; f < D; f += blockDim.x * 4) {
    f32x4 o = {0.f, 0.f, 0.f, 0.f};
    if (ok) {
      const bf16x4 v = *reinterpret_cast<const bf16x4*>(src + f);
      o[0] = (float)v[0]; o[1] = (float)v[1]; o[2] = (float)v[2]; o[3] = (float)v[3];
    }
    *reinterpret_cast<f32x4*>(dst + f) = o;
  }
}

// Ragged gather of a padded fp32 gradient [B, T, D] into a bf16 row matrix (backward of unpack).
__global__ void pack_grad_kernel(const float* __restrict__ g, int T, int D, const int* off, const int* len,
                                 bf16* __restrict__ out, int ld) {
  const int b = blockIdx.z, t = blockIdx.y;
  if (t >= len[b]) return;
  const float* src = g + ((size_t)b * T + t) * D;
  bf16* dst = out + (size_t)(off[b] + t) * ld;
  for (int f = threadIdx.x * 4; f < D; f += blockDim.x * 4) {
    const f32x4 v = *reinterpret_cast<const f32x4*>(src + f);
    bf16x4 o = {(bf16)v[0], (bf16)v[1], (bf16)v[2], (bf16)v[3]};
    *reinterpret_cast<bf16x4*>(dst + f) = o;
  }
}

// Decoder input: out[off[b]+t] = E[tok[b,t]] + PE[t]   (Models.py:84 + repair R3; Embedding.py:26)
// A token id outside [0, V) traps (nn.Embedding device-asserts on it): reading / accumulating at emb + id * D would
// silently touch neighbouring slots of the flat parameter / gradient arena.
__global__ void embed_pe_fwd_kernel(const long long* __restrict__ tok, int L, const float* __restrict__ emb, int V,
                                    const float* __restrict__ pe, int D, const int* off, const int* len,
                                    bf16* __restrict__ out) {
  const int b = blockIdx.z, t = blockIdx.y;
  if (t >= len[b]) return;
  const long long id = tok[(size_t)b * L + t];
  if (id < 0 || id >= V) __builtin_trap();
  const float* e = emb + (size_t)id * D;
  const float* p = pe + (size_t)t * D;
  bf16* dst = out + (size_t)(off[b] + t) * D;
  for (int f = threadIdx.x * 4; f < D; f += blockDim.x * 4) {
    const f32x4 a = *reinterpret_cast<const f32x4*>(e + f);
    const f32x4 c = *reinterpret_cast<const f32x4*>(p + f);
    bf16x4 o = {(bf16)(a[0] + c[0]), (bf16)(a[1] + c[1]), (bf16)(a[2] + c[2]), (bf16)(a[3] + c[3])};
    *reinterpret_cast<bf16x4*>(dst + f) = o;
  }
}

// dE[tok] += dy ; the padding_idx row (Models.py:74, Constants.PAD) never receives gradient.
__global__ void embed_bwd_kernel(const long long* __restrict__ tok, int L, const bf16* __restrict__ dy, int ld, int D,
                                 const int* off, const int* len, int pad_idx, float* demb, int V) {
  const int b = blockIdx.z, t = blockIdx.y;
  if (t >= len[b]) return;
  const long long id = tok[(size_t)b * L + t];
  if (id == pad_idx) return;
  if (id < 0 || id >= V) __builtin_trap();
  const bf16* src = dy + (size_t)(off[b] + t) * ld;
  float* dst = demb + (size_t)id * D;
  for (int f = threadIdx.x; f < D; f += blockDim.x) atomicAdd(dst + f, (float)src[f]);
}

__global__ void cast_bf16_kernel(const float* __restrict__ src, bf16* __restrict__ dst, size_t n8) {
  for (size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x; i < n8; i += (size_t)gridDim.x * blockDim.x) {
    const f32x4 a = *reinterpret_cast<const f32x4*>(src + i * 8);
    const f32x4 b = *reinterpret_cast<const f32x4*>(src + i * 8 + 4);
    bf16x8 o = {(bf16)a[0], (bf16)a[1], (bf16)a[2], (bf16)a[3], (bf16)b[0], (bf16)b[1], (bf16)b[2], (bf16)b[3]};
    *reinterpret_cast<bf16x8*>(dst + i * 8) = o;
  }
}

// Zero the rows [*valid, cap) of a list of row matrices - the rows a packed bucket layout (st_amd.functional.Rows.bucket
// with a capacity) leaves to no utterance - in ONE launch per step instead of a whole-matrix memset per buffer (72 of
// them in a config-2 step: 0.4 ms).  table: 4 x int64 per entry - base address, bytes per row (a multiple of 16), capacity
// in rows, address of the layout's device-resident int32 "valid rows"; entries with a null base are skipped.
__global__ __launch_bounds__(256) void zero_tails_kernel(const long long* __restrict__ table, int n_max) {
  const int e = blockIdx.x;
  if (e >= n_max) return;
  const long long* d = table + (size_t)e * 4;
  char* base = reinterpret_cast<char*>(d[0]);
  if (!base) return;
  const long long row_bytes = d[1], cap = d[2];
  long long valid = *reinterpret_cast<const int*>(d[3]);
  valid = valid < 0 ? 0 : (valid > cap ? cap : valid);
  f32x4* p = reinterpret_cast<f32x4*>(base + valid * row_bytes);
  const long long n16 = (cap - valid) * row_bytes / 16;
  const f32x4 z = {0.f, 0.f, 0.f, 0.f};
  for (long long i = blockIdx.y * 256ll + threadIdx.x; i < n16; i += (long long)gridDim.y * 256) p[i] = z;
}

// ---- hardware probes (tests/test_probe_gpu.py): pin the fragment layouts the kernels rely on -------
__global__ void probe_tr16_kernel(const bf16* in, bf16* out) {
  __shared__ __attribute__((aligned(16))) bf16 tile[16 * 64];
  for (int i = threadIdx.x; i < 16 * 64; i += 64) tile[i] = in[i];
  __syncthreads();
  const int l = threadIdx.x;
  // natural-order fragment: c = hi*8 .. hi*8+7 of operand row (l & 31), tile stored [c][row], stride 64
  const bf16x8 f = frag_tr(tile, 64, 0, (l >> 5) * 8, (l >> 5) * 8 + 4);
  *reinterpret_cast<bf16x8*>(out + l * 8) = f;
}

__global__ void probe_mfma_kernel(const bf16* A, const bf16* Bt, float* D) {
  // A [32][16] row-major, Bt [32][16] row-major (= B^T); D[i][j] written row-major [32][32]
  const int l = threadIdx.x, hi = l >> 5;
  const bf16x8 a = *reinterpret_cast<const bf16x8*>(A + (l & 31) * 16 + hi * 8);
  const bf16x8 b = *reinterpret_cast<const bf16x8*>(Bt + (l & 31) * 16 + hi * 8);
  const f32x16 c = mfma32(a, b, zero16());
  for (int r = 0; r < 16; ++r) D[acc_row(r, hi) * 32 + (l & 31)] = c[r];
}

}  // namespace

extern "C" int st_ln_bwd(hipStream_t stream, const void* dy, int lddy, const void* xhat, const float* rstd,
                         const float* gamma, const void* mask, void* dx, int lddx, float* dgamma, float* dbeta,
                         float* dbias, int M, int N, const unsigned* drop_seed, unsigned drop_salt, int drop_thresh,
                         float drop_scale, float mask_scale) {
  if (M <= 0) return 0;
  if ((lddy & 7) || (lddx & 7)) return -1;
  const int rows_per_block = 4 * (64 / (N / 8)) * 2;
  int blocks = (M + rows_per_block - 1) / rows_per_block;
  // one workgroup per CU: every workgroup ends with 3 N same-address fp32 atomics (dgamma / dbeta / dbias),
  // and those serialise - 1024 workgroups took 30 us on [24060, 256], 256 take 16 us (measured)
  if (blocks > 256) blocks = 256;
  DropArgs drop;
  const bool on = drop_seed != nullptr && drop_thresh > 0;
  drop.seed = on ? drop_seed : nullptr; drop.salt = drop_salt; drop.thresh = on ? drop_thresh : 0;
  drop.scale = on ? drop_scale : 1.f;
  if (!(mask_scale > 0.f)) mask_scale = 1.f;
#define ST_LN_BWD_(NN, DR)                                                                                    \
  hipLaunchKernelGGL((ln_bwd_kernel<NN, DR>), dim3(blocks), dim3(256), 0, stream, (const bf16*)dy, lddy,      \
                     (const bf16*)xhat, rstd, gamma, (const bf16*)mask, (bf16*)dx, lddx, dgamma, dbeta, dbias, M, \
                     drop, mask_scale)
#define ST_LN_BWD(NN) do { if (on) ST_LN_BWD_(NN, true); else ST_LN_BWD_(NN, false); } while (0)
  if (N == 128) ST_LN_BWD(128);
  else if (N == 256) ST_LN_BWD(256);
  else if (N == 512) ST_LN_BWD(512);
  else return -2;
#undef ST_LN_BWD
#undef ST_LN_BWD_
  ST_CHECK_LAUNCH();
  return 0;
}

extern "C" int st_row_index(hipStream_t stream, const int* off, const int* len, int B, int max_len, int* row_pos,
                            int* row_seq) {
  if (B <= 0 || max_len <= 0) return 0;
  hipLaunchKernelGGL(row_index_kernel, dim3((max_len + 255) / 256, B), dim3(256), 0, stream, off, len, row_pos, row_seq);
  ST_CHECK_LAUNCH();
  return 0;
}

extern "C" int st_pack_rows(hipStream_t stream, const float* x, int B, int T, int F, const int* off, const int* len,
                            void* out) {
  if (B <= 0 || T <= 0) return 0;
  if (F & 3) return -1;
  const int cpr = F >> 2, rpb = cpr >= 256 ? 1 : 256 / cpr;    // frames per workgroup
  hipLaunchKernelGGL(pack_rows_kernel, dim3(1, (T + rpb - 1) / rpb, B), dim3(256), 0, stream, x, T, F, rpb, off, len, (bf16*)out);
  ST_CHECK_LAUNCH();
  return 0;
}

extern "C" int st_unpack_rows(hipStream_t stream, const void* x, int ld, int B, int T, int D, const int* off,
                              const int* len, float* out) {
  if (B <= 0 || T <= 0) return 0;
  if ((D & 3) || (ld & 3)) return -1;
  hipLaunchKernelGGL(unpack_rows_kernel, dim3(1, T, B), dim3(64), 0, stream, (const bf16*)x, ld, T, D, off, len, out);
  ST_CHECK_LAUNCH();
  return 0;
}

extern "C" int st_pack_grad(hipStream_t stream, const float* g, int B, int T, int D, const int* off, const int* len,
                            void* out, int ld) {
  if (B <= 0 || T <= 0) return 0;
  if ((D & 3) || (ld & 3)) return -1;
  hipLaunchKernelGGL(pack_grad_kernel, dim3(1, T, B), dim3(64), 0, stream, g, T, D, off, len, (bf16*)out, ld);
  ST_CHECK_LAUNCH();
  return 0;
}

extern "C" int st_embed_pe_fwd(hipStream_t stream, const long long* tok, int B, int L, const float* emb, int V,
                               const float* pe, int D, const int* off, const int* len, void* out) {
  if (B <= 0 || L <= 0) return 0;
  if ((D & 3) || V <= 0) return -1;
  hipLaunchKernelGGL(embed_pe_fwd_kernel, dim3(1, L, B), dim3(64), 0, stream, tok, L, emb, V, pe, D, off, len, (bf16*)out);
  ST_CHECK_LAUNCH();
  return 0;
}

extern "C" int st_embed_bwd(hipStream_t stream, const long long* tok, int B, int L, const void* dy, int ld, int D,
                            const int* off, const int* len, int pad_idx, float* demb, int V) {
  if (B <= 0 || L <= 0) return 0;
  if (V <= 0) return -1;
  hipLaunchKernelGGL(embed_bwd_kernel, dim3(1, L, B), dim3(64), 0, stream, tok, L, (const bf16*)dy, ld, D, off, len,
                     pad_idx, demb, V);
  ST_CHECK_LAUNCH();
  return 0;
}

// Beam-search decode: hypotheses inherit the self-attention K|V history of the hypothesis they extend (Decode.py re-runs
// the whole prefix instead; Beam.py:65 back-pointers).  cache [L][n][S][W] bf16; for every layer, every position
// t <= *step and every utterance (beam consecutive rows): row u*beam+s <- old row order[u*beam+s] (same utterance),
// in place: a workgroup holds the utterance's beam rows of one position in registers between its loads and stores.
__global__ __launch_bounds__(256) void cache_reorder_kernel(bf16* cache, const long long* __restrict__ order,
                                                            const long long* __restrict__ step, int n, int S, int W, int beam) {
  const int t = blockIdx.x, u = blockIdx.y, l = blockIdx.z;
  if (t > (int)*step) return;
  const int cpr = W / 8, total = beam * cpr;          // 16-byte chunks per row / per utterance
  bf16x8 v[8];
#pragma unroll
  for (int p = 0; p < 8; ++p) {
    const int id = p * 256 + threadIdx.x;
    if (id < total) {
      const long long src = order[u * beam + id / cpr];
      v[p] = *reinterpret_cast<const bf16x8*>(cache + (((size_t)l * n + src) * S + t) * W + (id % cpr) * 8);
    }
  }
  __syncthreads();
#pragma unroll
  for (int p = 0; p < 8; ++p) {
    const int id = p * 256 + threadIdx.x;
    if (id < total)
      *reinterpret_cast<bf16x8*>(cache + (((size_t)l * n + u * beam + id / cpr) * S + t) * W + (id % cpr) * 8) = v[p];
  }
}

// Beam.advance (Beam.py:43-74) for every utterance at once: one workgroup per utterance.
//   word_lk[j][v] = logits[j][v] - logsumexp(logits[j][:V])           (the `prob_projection` log-softmax, Decode.py:102)
//   the `beam` best of scores[j] + word_lk[j][v] over the beam x V candidates, best first (Beam.py:53-57, ties: lowest
//   flat index), origin = flat / V, token = flat % V (Beam.py:63-66); an utterance whose best hypothesis just emitted EOS
//   is done (Beam.py:70-72) and frozen from then on: scores / tokens keep their values, its back-pointers are the identity.
// State (all device memory, updated in place): scores f32 [B][beam]; tokens i64 [B*beam]; done u8 [B]; lengths i64 [B];
// the trellis hist_scores f32 / back i64 / toks i64 [S][B][beam] at row *step; order i64 [B*beam] (the cache rows the
// hypotheses inherit, for st_cache_reorder).
// candidate (x, xi) precedes (y, yi) in the result order: larger value first, lower flat index on ties
__device__ __forceinline__ bool beam_before(float x, int xi, float y, int yi) { return x > y || (x == y && xi < yi); }

// The KLOC best candidates of this thread that come strictly AFTER (lim, limi) in the result order (lim = +inf: all),
// best first.  A thread's candidates are flat = j * V + v, v = tid, tid + 512, ...  (a short compare chain per candidate:
// the 64 lanes of a wave insert at different times, so a deep per-thread list would be paid by every candidate)
template <int KLOC, bool FIRST>
__device__ __forceinline__ void beam_local_best(const float* lg, int ldl, int V, int beam, const float* scores_b, const float* s_lse,
                                                int tid, float lim, int limi, float (&val)[KLOC], int (&idx)[KLOC]) {
#pragma unroll
  for (int i = 0; i < KLOC; ++i) { val[i] = -INFINITY; idx[i] = 0x7fffffff; }
  // (unit = one batch of 12 loads of one row; the next unit's loads are issued before this one's compare chains).  Row j's
  // columns are dealt to the threads rotated by 53 j: the best next tokens of the hypotheses of one beam tend to be the SAME
  // tokens, and with one column -> one thread for all rows a single thread would own most of the winners (measured on the
  // benchmark model: five refill scans per step, 114 us instead of 50)
  const int nbatch = (V + 512 * 12 - 1) / (512 * 12), units = beam * nbatch;
  float nx[12];
#pragma unroll
  for (int u = 0; u < 12; ++u) nx[u] = (u * 512 + tid < V) ? lg[u * 512 + tid] : -INFINITY;
  for (int un = 0; un < units; ++un) {
    const int j = un / nbatch, v0 = (un % nbatch) * 512 * 12;
    const int vs = (tid + j * 53) & 511;
    const float base = scores_b[j] - s_lse[j];
    {
      float xs[12];
#pragma unroll
      for (int u = 0; u < 12; ++u) xs[u] = nx[u];
      if (un + 1 < units) {
        const int j2 = (un + 1) / nbatch, w0 = ((un + 1) % nbatch) * 512 * 12;
        const int vs2 = (tid + j2 * 53) & 511;
        const float* row2 = lg + (size_t)j2 * ldl;
#pragma unroll
        for (int u = 0; u < 12; ++u) nx[u] = (w0 + u * 512 + vs2 < V) ? row2[w0 + u * 512 + vs2] : -INFINITY;
      }
#pragma unroll
      for (int u = 0; u < 12; ++u) {
        float x = base + xs[u];
        int xi = j * V + v0 + u * 512 + vs;
        const bool in_range = (v0 + u * 512 + vs < V) && (FIRST || beam_before(lim, limi, x, xi));
        if (in_range && beam_before(x, xi, val[KLOC - 1], idx[KLOC - 1])) {
#pragma unroll
          for (int i = 0; i < KLOC; ++i) {
            const bool better = beam_before(x, xi, val[i], idx[i]);
            const float tv = better ? val[i] : x;
            const int ti = better ? idx[i] : xi;
            val[i] = better ? x : val[i];
            idx[i] = better ? xi : idx[i];
            x = tv; xi = ti;
          }
        }
      }
    }
  }
}

__global__ __launch_bounds__(512) void beam_advance_kernel(const float* __restrict__ logits, int ldl, int V, int beam, int B,
                                                           const long long* __restrict__ step_p, int eos, float* scores,
                                                           long long* tokens, unsigned char* done, long long* lengths,
                                                           float* hist_scores, long long* back, long long* toks,
                                                           long long* order) {
  constexpr int KLOC = 2, KMAX = 16;
  __shared__ float s_lse[KMAX], s_sc[KMAX];
  __shared__ float s_wv[2][8];
  __shared__ int s_wi[2][8], s_wt[2][8];
  __shared__ float s_best[KMAX];
  __shared__ int s_bidx[KMAX];
  const int b = blockIdx.x, tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
  const long long step = *step_p;
  const float* lg = logits + (size_t)b * beam * ldl;
  if (tid < beam) s_sc[tid] = scores[b * beam + tid];
  // ---- log-sum-exp of every hypothesis row: half-wave g takes row g (beam <= 16), one pass with a running (max, sum);
  //      loads issued in batches of 16 (32 workgroups cannot hide a dependent global load per element)
  {
    const int g = tid >> 5, l32 = tid & 31;
    float mx = -INFINITY, sm = 0.f;
    if (g < beam) {
      const float* row = lg + (size_t)g * ldl;
      for (int v0 = 0; v0 < V; v0 += 32 * 16) {
        float x[16];
#pragma unroll
        for (int u = 0; u < 16; ++u) x[u] = (v0 + u * 32 + l32 < V) ? row[v0 + u * 32 + l32] : -INFINITY;
        float bm = x[0];
#pragma unroll
        for (int u = 1; u < 16; ++u) bm = fmaxf(bm, x[u]);
        const float mn = fmaxf(mx, bm);
        if (mn > -INFINITY) {
          float bs = 0.f;
#pragma unroll
          for (int u = 0; u < 16; ++u) bs += __expf(x[u] - mn);
          sm = sm * __expf(mx - mn) + bs;
          mx = mn;
        }
      }
    }
#pragma unroll
    for (int o = 16; o; o >>= 1) {
      const float om = __shfl_xor(mx, o, 64), os = __shfl_xor(sm, o, 64);
      const float mn = fmaxf(mx, om);
      if (mn > -INFINITY) sm = sm * __expf(mx - mn) + os * __expf(om - mn);
      mx = mn;
    }
    if (g < beam && l32 == 0) s_lse[g] = mx + __logf(sm);
  }
  __syncthreads();
  float val[KLOC];
  int idx[KLOC];
  beam_local_best<KLOC, true>(lg, ldl, V, beam, s_sc, s_lse, tid, INFINITY, -1, val, idx);
  // ---- merge: `beam` rounds of a workgroup-wide arg-max over the threads' current heads; a thread whose KLOC candidates are
  //      all taken (it holds more than KLOC of the winners: rare) refills from the ones after its last
  int head = 0;
  for (int rnd = 0; rnd < beam; ++rnd) {
    float x = -INFINITY;
    int xi = 0x7fffffff;
#pragma unroll
    for (int i = 0; i < KLOC; ++i)
      if (head == i) { x = val[i]; xi = idx[i]; }
    int xt = tid;
#pragma unroll
    for (int o = 32; o; o >>= 1) {
      const float ov = __shfl_xor(x, o, 64);
      const int oi = __shfl_xor(xi, o, 64), ot = __shfl_xor(xt, o, 64);
      if (beam_before(ov, oi, x, xi)) { x = ov; xi = oi; xt = ot; }
    }
    const int pp = rnd & 1;       // ping-pong exchange buffers: one barrier per round
    if (lane == 0) { s_wv[pp][wave] = x; s_wi[pp][wave] = xi; s_wt[pp][wave] = xt; }
    __syncthreads();
    float bx = s_wv[pp][0];
    int bi = s_wi[pp][0], bt = s_wt[pp][0];
#pragma unroll
    for (int w = 1; w < 8; ++w)
      if (beam_before(s_wv[pp][w], s_wi[pp][w], bx, bi)) { bx = s_wv[pp][w]; bi = s_wi[pp][w]; bt = s_wt[pp][w]; }
    if (tid == 0) { s_best[rnd] = bx; s_bidx[rnd] = bi; }
    if (tid == bt && ++head == KLOC) {
      beam_local_best<KLOC, false>(lg, ldl, V, beam, s_sc, s_lse, tid, bx, bi, val, idx);
      head = 0;
    }
  }
  __syncthreads();
  // ---- the state update (one thread per beam slot)
  if (tid < beam) {
    const int s = tid;
    const bool live = !done[b];
    const size_t at = ((size_t)step * B + b) * beam + s;
    const int flat = s_bidx[s];
    const long long origin = live ? flat / V : s, token = flat % V;
    hist_scores[at] = s_sc[s];
    back[at] = origin;
    toks[at] = token;
    order[b * beam + s] = origin + (long long)b * beam;
    if (live) {
      scores[b * beam + s] = s_best[s];
      tokens[b * beam + s] = token;
      if (s == 0) {
        lengths[b] += 1;
        if (token == eos) done[b] = 1;
      }
    }
  }
}

// The same step over more of the chip (the kernel above keeps one compute unit per utterance busy for 43 us:
// ~20 dependent batches of loads that 32 workgroups cannot hide, then ~12 vector instructions per candidate on one CU):
//   (1) beam_row_best_kernel - one workgroup per HYPOTHESIS row (B * beam of them), the row's V logits in registers with
//       every load issued before the first use: log-sum-exp, then the row's `beam` best candidates score + log-probability
//       (the utterance's winners are among them), as 64-bit keys in `work`;
//   (2) the merge - by the wave of the utterance's row that finishes last (a ticket per utterance): the `beam` best of its
//       beam x beam keys, and the state update (beam_merge_wave).  One launch.
// Wave reductions run on DPP (row butterflies + row_bcast), not ds_bpermute.  Across lanes candidates are ordered through
// one 64-bit key (monotone image of the score in the high word, 0x7fffffff - flat index in the low word: larger score
// first, lower flat index on ties - the order of beam_before); inside a thread the scan runs in increasing flat index with
// strict comparisons, which is the same order.
__device__ __forceinline__ unsigned long long beam_key(float x, int flat) {
  const unsigned u = __float_as_uint(x);
  const unsigned m = (u & 0x80000000u) ? ~u : (u | 0x80000000u);
  return ((unsigned long long)m << 32) | (unsigned)(0x7fffffff - flat);
}
__device__ __forceinline__ float beam_key_value(unsigned long long k) {
  const unsigned m = (unsigned)(k >> 32);
  return __uint_as_float((m & 0x80000000u) ? (m & 0x7fffffffu) : ~m);
}
__device__ __forceinline__ int beam_key_flat(unsigned long long k) { return 0x7fffffff - (int)(unsigned)(k & 0xffffffffu); }

// DPP moves: quad_perm [1,0,3,2] = 0xB1, [2,3,0,1] = 0x4E, row_half_mirror = 0x141, row_mirror = 0x140 (after these four a
// butterfly has every lane of a 16-lane row hold the row's result), row_bcast15 = 0x142 (rows 1, 3 take lane 15 of rows 0, 2),
// row_bcast31 = 0x143 (rows 2, 3 take lane 31): the wave's result is in lane 63.  Lanes a row mask leaves out keep `old`.
template <int CTRL, int ROWS>
__device__ __forceinline__ int dpp_i(int old, int v) { return __builtin_amdgcn_update_dpp(old, v, CTRL, ROWS, 0xf, false); }
template <int CTRL, int ROWS>
__device__ __forceinline__ float dpp_f(float old, float v) { return __int_as_float(dpp_i<CTRL, ROWS>(__float_as_int(old), __float_as_int(v))); }
__device__ __forceinline__ float row16_max(float v) {
  v = fmaxf(v, dpp_f<0xB1, 0xf>(v, v));
  v = fmaxf(v, dpp_f<0x4E, 0xf>(v, v));
  v = fmaxf(v, dpp_f<0x141, 0xf>(v, v));
  return fmaxf(v, dpp_f<0x140, 0xf>(v, v));
}
__device__ __forceinline__ float row16_sum(float v) {
  v += dpp_f<0xB1, 0xf>(0.f, v);
  v += dpp_f<0x4E, 0xf>(0.f, v);
  v += dpp_f<0x141, 0xf>(0.f, v);
  return v + dpp_f<0x140, 0xf>(0.f, v);
}
__device__ __forceinline__ float wave_max_dpp(float v) {       // -> lane 63's value, uniform
  v = row16_max(v);
  v = fmaxf(v, dpp_f<0x142, 0xa>(v, v));
  v = fmaxf(v, dpp_f<0x143, 0xc>(v, v));
  return __int_as_float(__builtin_amdgcn_readlane(__float_as_int(v), 63));
}
__device__ __forceinline__ float wave_sum_dpp(float v) {
  v = row16_sum(v);
  v += dpp_f<0x142, 0xa>(0.f, v);
  v += dpp_f<0x143, 0xc>(0.f, v);
  return __int_as_float(__builtin_amdgcn_readlane(__float_as_int(v), 63));
}
template <int CTRL, int ROWS>
__device__ __forceinline__ unsigned long long key_max_step(unsigned long long k) {
  const unsigned lo = (unsigned)dpp_i<CTRL, ROWS>((int)(unsigned)k, (int)(unsigned)k);
  const unsigned hi = (unsigned)dpp_i<CTRL, ROWS>((int)(unsigned)(k >> 32), (int)(unsigned)(k >> 32));
  const unsigned long long o = ((unsigned long long)hi << 32) | lo;
  return o > k ? o : k;
}
__device__ __forceinline__ unsigned long long wave_max_key(unsigned long long k) {    // uniform
  k = key_max_step<0xB1, 0xf>(k);
  k = key_max_step<0x4E, 0xf>(k);
  k = key_max_step<0x141, 0xf>(k);
  k = key_max_step<0x140, 0xf>(k);
  k = key_max_step<0x142, 0xa>(k);
  k = key_max_step<0x143, 0xc>(k);
  const unsigned lo = (unsigned)__builtin_amdgcn_readlane((int)(unsigned)k, 63), hi = (unsigned)__builtin_amdgcn_readlane((int)(unsigned)(k >> 32), 63);
  return ((unsigned long long)hi << 32) | lo;
}

// The merge, run by ONE wave (the wave of the utterance's hypothesis rows that drew the last ticket): the `beam` best of the
// utterance's beam x beam keys, the lineage table, the state update, the NEXT step's decoder input (embedding + positional
// encoding of the tokens just chosen: st_embed_step's arithmetic) and the step counter.
__device__ __forceinline__ void beam_merge_wave(int (*s_anc)[128], const unsigned long long* work, int b, int lane, int V, int beam, int B,
                                                const long long* __restrict__ step_p, int eos, float* scores, long long* tokens,
                                                unsigned char* done, long long* lengths, float* hist_scores, long long* back,
                                                long long* toks, long long* order, int* anc, int S, long long* step_next,
                                                unsigned* ticket, const float* __restrict__ emb, int emb_rows,
                                                const float* __restrict__ pe, int pe_rows, bf16* x_next, int D) {
  const int n = beam * beam;          // n <= 256
  const long long step = *step_p;
  unsigned long long c[4];
#pragma unroll
  for (int i = 0; i < 4; ++i)
    c[i] = i * 64 + lane < n ? __hip_atomic_load(work + (size_t)b * n + i * 64 + lane, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) : 0ull;
  const float old = lane < beam ? scores[b * beam + lane] : 0.f;
  const long long old_tok = lane < beam ? tokens[b * beam + lane] : 0;
  // (the utterance's rows of the lineage table, asked for before the merge rounds: one memory round trip, hidden)
  const int t = (int)step;
  int r[16][2];
  if (anc) {
#pragma unroll
    for (int s = 0; s < 16; ++s)
#pragma unroll
      for (int h = 0; h < 2; ++h)
        if (s < beam && lane + 64 * h < t) r[s][h] = anc[((size_t)b * beam + s) * S + lane + 64 * h];
  }
  float bestv = 0.f;
  int flat = 0;
  for (int r = 0; r < beam; ++r) {
    const unsigned long long m01 = c[0] > c[1] ? c[0] : c[1], m23 = c[2] > c[3] ? c[2] : c[3];
    const unsigned long long best = wave_max_key(m01 > m23 ? m01 : m23);
#pragma unroll
    for (int i = 0; i < 4; ++i)
      if (c[i] == best) c[i] = 0ull;
    if (lane == r) { bestv = beam_key_value(best); flat = beam_key_flat(best); }
  }
  const bool live_u = !done[b];
  // ---- the lineage table of st_decode_self_attn: the new hypothesis in slot s inherits positions 0 .. step - 1 from its
  //      origin and finds position `step` in the origin's slot (a done utterance: the identity)
  if (anc) {
#pragma unroll
    for (int s = 0; s < 16; ++s)
#pragma unroll
      for (int h = 0; h < 2; ++h)
        if (s < beam && lane + 64 * h < t) s_anc[s][lane + 64 * h] = r[s][h];
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "workgroup");      // (one wave writes and reads the staging rows: no barrier)
    for (int s = 0; s < beam; ++s) {
      const int o = live_u ? __shfl(flat, s, 64) / V : s;
      for (int p = lane; p < t; p += 64) anc[((size_t)b * beam + s) * S + p] = s_anc[o][p];
      if (lane == 0) anc[((size_t)b * beam + s) * S + t] = b * beam + o;
    }
  }
  // ---- the state update (one lane per beam slot), as in beam_advance_kernel
  long long token = old_tok;
  if (lane < beam) {
    const int s = lane;
    const size_t at = ((size_t)step * B + b) * beam + s;
    const long long origin = live_u ? flat / V : s, tk = flat % V;
    hist_scores[at] = old;
    back[at] = origin;
    toks[at] = tk;
    order[b * beam + s] = origin + (long long)b * beam;
    if (live_u) {
      token = tk;
      scores[b * beam + s] = bestv;
      tokens[b * beam + s] = tk;
      if (s == 0) {
        lengths[b] += 1;
        if (tk == eos) done[b] = 1;
      }
    }
  }
  // ---- the next step's decoder input for this utterance's hypotheses: bf16(emb[token] + pe[step + 1])
  if (x_next && step + 1 < pe_rows) {
    for (int s = 0; s < beam; ++s) {
      const long long tk = __shfl(token, s, 64);
      if (tk < 0 || tk >= emb_rows) __builtin_trap();
      for (int ch = lane; ch < D / 4; ch += 64) {
        const f32x4 e = *reinterpret_cast<const f32x4*>(emb + (size_t)tk * D + ch * 4);
        const f32x4 pp = *reinterpret_cast<const f32x4*>(pe + (size_t)(step + 1) * D + ch * 4);
        bf16x4 o;
#pragma unroll
        for (int k = 0; k < 4; ++k) o[k] = (bf16)(e[k] + pp[k]);
        *reinterpret_cast<bf16x4*>(x_next + ((size_t)b * beam + s) * D + ch * 4) = o;
      }
    }
  }
  // ---- the step counter: every utterance's wave has read it by the time it draws its ticket, the last one advances it
  if (step_next && lane == 0) {
    if (atomicAdd(ticket, 1u) == (unsigned)(B - 1)) {
      *ticket = 0u;
      *step_next = step + 1;
    }
  }
}

struct BeamState {       // what the merge updates (see st_beam_advance)
  const long long* step; int eos, B; float* scores; long long* tokens; unsigned char* done; long long* lengths;
  float* hist_scores; long long* back; long long* toks; long long* order; int* anc; int S; long long* step_next;
  unsigned* ticket; unsigned* row_tickets; const float* emb; int emb_rows; const float* pe; int pe_rows; bf16* x_next; int D;
};

template <int NU>
__global__ __launch_bounds__(256) void beam_row_best_kernel(const float* __restrict__ logits, int ldl, int V, int beam,
                                                            unsigned long long* work, BeamState st) {
  constexpr int NW = 4;
  __shared__ float s_red[2][NW];
  __shared__ unsigned long long s_cand[NW * 16];
  __shared__ int s_anc[16][128];
  const float* __restrict__ scores = st.scores;
  const int row = blockIdx.x, j = row % beam, tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
  const float* lg = logits + (size_t)row * ldl;
  float x[NU];
#pragma unroll
  for (int u = 0; u < NU; ++u) x[u] = lg[u * 256 + tid < V ? u * 256 + tid : 0];      // (no branch around any load)
  const float sc = scores[row];
  if (tid < NW * 16) s_cand[tid] = 0ull;
#pragma unroll
  for (int u = 0; u < NU; ++u)
    if (u * 256 + tid >= V) x[u] = -INFINITY;
  // ---- log-sum-exp of the row
  float m = x[0];
#pragma unroll
  for (int u = 1; u < NU; ++u) m = fmaxf(m, x[u]);
  m = wave_max_dpp(m);
  if (lane == 0) s_red[0][wave] = m;
  __syncthreads();
  m = fmaxf(fmaxf(s_red[0][0], s_red[0][1]), fmaxf(s_red[0][2], s_red[0][3]));
  float sm = 0.f;
#pragma unroll
  for (int u = 0; u < NU; ++u) sm += __expf(x[u] - m);
  sm = wave_sum_dpp(sm);
  if (lane == 0) s_red[1][wave] = sm;
  __syncthreads();
  sm = (s_red[1][0] + s_red[1][1]) + (s_red[1][2] + s_red[1][3]);
  const float base = sc - (m + __logf(sm));                   // score - lse, as the kernel above forms it
  // ---- the thread's two best candidates (first) / its two best after `lim` in the result order (refill), as keys (0 = none)
  unsigned long long k0, k1;
  auto local_best = [&](unsigned long long lim, bool first) {
    const float limv = beam_key_value(lim);
    const int limf = beam_key_flat(lim);
    const float nan = __int_as_float(0x7fc00000);
    float v0 = nan, v1 = nan;             // (NaN = empty: !(c <= NaN) holds for every c)
    int e0 = -1, e1 = -1;
#pragma unroll
    for (int u = 0; u < NU; ++u) {
      const int col = u * 256 + tid;
      const float c = base + x[u];
      bool ok = col < V && !(c <= v1);
      if (!first) ok = ok && (c < limv || (c == limv && j * V + col > limf));
      const bool top = !(c <= v0);
      v1 = ok ? (top ? v0 : c) : v1;
      e1 = ok ? (top ? e0 : col) : e1;
      v0 = (ok && top) ? c : v0;
      e0 = (ok && top) ? col : e0;
    }
    k0 = e0 >= 0 ? beam_key(v0, j * V + e0) : 0ull;
    k1 = e1 >= 0 ? beam_key(v1, j * V + e1) : 0ull;
  };
  local_best(0ull, true);
  // ---- every wave: its `beam` best, best first (shuffles only, no barrier)
  int head = 0;
  unsigned long long w = wave_max_key(k0);
  for (int r = 0; r < beam && w != 0ull; ++r) {
    if (lane == 0) s_cand[wave * 16 + r] = w;
    const unsigned long long mine = head == 0 ? k0 : k1;
    if (mine == w && ++head == 2) {        // (keys are distinct: one lane advances; past its second candidate it rescans)
      local_best(w, false);
      head = 0;
    }
    w = wave_max_key(head == 0 ? k0 : k1);
  }
  __syncthreads();
  // ---- wave 0: the row's `beam` best of the four lists; they leave through the L2 (write-through), then the utterance's
  //      ticket: the wave of the LAST of its `beam` rows merges them (no fence: see row_chain_split_kernel)
  if (wave != 0) return;
  unsigned long long c = s_cand[lane];
  for (int r = 0; r < beam; ++r) {
    const unsigned long long best = wave_max_key(c);
    if (c == best) c = 0ull;
    if (lane == 0) __hip_atomic_store(work + (size_t)row * beam + r, best, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
  }
  ST_PUBLISH_FENCE();
  __builtin_amdgcn_s_waitcnt(0);
  const int b = row / beam;
  int last = 0;
  if (lane == 0) {
    last = __hip_atomic_fetch_add(st.row_tickets + b, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) == (unsigned)(beam - 1);
    if (last) __hip_atomic_store(st.row_tickets + b, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  }
  if (!__builtin_amdgcn_readfirstlane(last)) return;
  ST_MERGER_FENCE();
  beam_merge_wave(s_anc, work, b, lane, V, beam, st.B, st.step, st.eos, st.scores, st.tokens, st.done, st.lengths, st.hist_scores,
                  st.back, st.toks, st.order, st.anc, st.S, st.step_next, st.ticket, st.emb, st.emb_rows, st.pe, st.pe_rows,
                  st.x_next, st.D);
}


// One beam-search step's decoder input: out[i] = bf16(emb[tokens[i]] + pe[*step])   (Models.py:84,87 with repair R3)
__global__ __launch_bounds__(256) void embed_step_kernel(const long long* __restrict__ tokens, const float* __restrict__ emb, int V,
                                                         const float* __restrict__ pe, const long long* __restrict__ step_p,
                                                         bf16* __restrict__ out, int n, int D) {
  const int per_row = D / 4, id = blockIdx.x * 256 + threadIdx.x;
  if (id >= n * per_row) return;
  const int i = id / per_row, c = (id % per_row) * 4;
  const long long t = tokens[i];
  if (t < 0 || t >= V) __builtin_trap();
  const f32x4 e = *reinterpret_cast<const f32x4*>(emb + (size_t)t * D + c);
  const f32x4 p = *reinterpret_cast<const f32x4*>(pe + (size_t)*step_p * D + c);
  bf16x4 o;
#pragma unroll
  for (int k = 0; k < 4; ++k) o[k] = (bf16)(e[k] + p[k]);
  *reinterpret_cast<bf16x4*>(out + (size_t)i * D + c) = o;
}

extern "C" int st_embed_step(hipStream_t stream, const long long* tokens, const float* emb, int V, const float* pe, const long long* step,
                             void* out, int n, int D) {
  if (n <= 0) return 0;
  if (!tokens || !emb || !pe || !step || !out || (D & 3)) return -1;
  hipLaunchKernelGGL(embed_step_kernel, dim3((n * (D / 4) + 255) / 256), dim3(256), 0, stream, tokens, emb, V, pe, step, (bf16*)out, n, D);
  ST_CHECK_LAUNCH();
  return 0;
}

// Decode-shaped self-attention (Decode.py:96-98 with a KV cache): one wave per (hypothesis, head), ONE query each.
// Appends the step's K | V (columns [d, 3d) of qkv) to cache [n][S][2d] at position t = *step (row = the hypothesis' own
// slot) and attends over positions 0 .. t: scores on the VALU (lane = key, 64 keys per pass), softmax by wave reductions,
// P V with lane = value column.  d_k = 64.  Replaces cache.index_copy_ + st_attn_fwd (whose 128-query tile holds one query
// per hypothesis here).
// `anc` (optional, int32 [n][S]): the lineage table - position p < t of hypothesis i is read from cache row anc[i][p], the
// slot the ancestor that produced it sat in (st_beam_advance maintains the table; every entry is a valid row at all times) -
// so the cache rows never move (without it: own rows, and st_cache_reorder permutes the cache after every step).
// A launch here is a chain of memory round trips with nothing to hide behind, so everything that can be asked for early
// is: the step counter, the lineage entries and q first, then the key AND value chunks of the first 64 positions
// (registers), and only then the arithmetic.
__global__ __launch_bounds__(256) void decode_self_attn_kernel(const bf16* __restrict__ qkv, int ldq, bf16* cache, const long long* __restrict__ step_p,
                                                               const int* __restrict__ anc, bf16* __restrict__ ctx, int ldc, int n, int S, int H,
                                                               float scale) {
  const int wave = threadIdx.x >> 6, l = threadIdx.x & 63;
  const int item = blockIdx.x * 4 + wave, i = item / H, h = item % H;
  if (i >= n) return;
  const int d = H * 64, t = (int)*step_p;
  const bf16* row = qkv + (size_t)i * ldq;
  // lane = (position group g = l / 8, 8-column chunk ch = l % 8): one load instruction fetches 16 bytes of the rows of eight
  // positions (positions j * 8 + g, j = 0 .. 7 per 64-position pass) - whole 128-byte head segments, for keys and values alike;
  // a score is the sum of the eight chunk lanes' partial dot products, and the probability of position (j, g) then sits in
  // exactly the lanes that hold that position's value chunks (no broadcasts in P V)
  const int g = l >> 3, ch = l & 7;
  int ak[2][8];                     // cache rows of this lane's positions
#pragma unroll
  for (int p = 0; p < 2; ++p)
#pragma unroll
    for (int j = 0; j < 8; ++j) ak[p][j] = anc ? anc[(size_t)i * S + min(p * 64 + j * 8 + g, S - 1)] : i;
  // the step's K | V into the cache (lanes 0-7: K, 8-15: V; 16 bytes each)
  if (l < 16) {
    const int part = l >> 3, c = (l & 7) * 8;
    *reinterpret_cast<bf16x8*>(cache + ((size_t)i * S + t) * 2 * d + part * d + h * 64 + c) =
        *reinterpret_cast<const bf16x8*>(row + d + part * d + h * 64 + c);
  }
  const bf16x8 qraw = *reinterpret_cast<const bf16x8*>(row + h * 64 + ch * 8);
  bf16x8 kraw[8], vraw[8];
  auto fetch = [&](int p, int off, bf16x8 (&dst)[8]) {      // off: 0 = keys, d = values (the newest position is read from qkv)
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      const int k = p * 64 + j * 8 + g;
      bf16x8 v = {};
      if (k <= t) {
        const bf16* r = (k == t) ? row + d + off + h * 64 : cache + ((size_t)ak[p][j] * S + k) * 2 * d + off + h * 64;
        v = *reinterpret_cast<const bf16x8*>(r + ch * 8);
      }
      dst[j] = v;
    }
  };
  fetch(0, 0, kraw);
  fetch(0, d, vraw);
  float q[8];
#pragma unroll
  for (int e = 0; e < 8; ++e) q[e] = (float)qraw[e] * scale;
  float sc[2][8];
  auto scores = [&](int p) {
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      float acc = 0.f;
#pragma unroll
      for (int e = 0; e < 8; ++e) acc = fmaf(q[e], (float)kraw[j][e], acc);
      acc += __shfl_xor(acc, 1, 64);
      acc += __shfl_xor(acc, 2, 64);
      acc += __shfl_xor(acc, 4, 64);
      sc[p][j] = (p * 64 + j * 8 + g <= t) ? acc : -INFINITY;
    }
  };
  scores(0);
  if (t >= 64) {                    // (S > 64 only)
    fetch(1, 0, kraw);
    scores(1);
  } else {
#pragma unroll
    for (int j = 0; j < 8; ++j) sc[1][j] = -INFINITY;
  }
  float mx = -INFINITY;
#pragma unroll
  for (int p = 0; p < 2; ++p)
#pragma unroll
    for (int j = 0; j < 8; ++j) mx = fmaxf(mx, sc[p][j]);
#pragma unroll
  for (int o = 8; o < 64; o <<= 1) mx = fmaxf(mx, __shfl_xor(mx, o, 64));
  float pr[2][8], sm = 0.f;
#pragma unroll
  for (int p = 0; p < 2; ++p)
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      pr[p][j] = sc[p][j] > -INFINITY ? __expf(sc[p][j] - mx) : 0.f;
      sm += pr[p][j];
    }
#pragma unroll
  for (int o = 8; o < 64; o <<= 1) sm += __shfl_xor(sm, o, 64);
  const float inv = 1.f / sm;
  float out[8] = {};
  auto accumulate = [&](int p) {
#pragma unroll
    for (int j = 0; j < 8; ++j)
#pragma unroll
      for (int e = 0; e < 8; ++e) out[e] = fmaf(pr[p][j], (float)vraw[j][e], out[e]);
  };
  accumulate(0);
  if (t >= 64) {
    fetch(1, d, vraw);
    accumulate(1);
  }
#pragma unroll
  for (int o = 8; o < 64; o <<= 1)
#pragma unroll
    for (int e = 0; e < 8; ++e) out[e] += __shfl_xor(out[e], o, 64);
  if (g == 0) {
    bf16x8 r;
#pragma unroll
    for (int e = 0; e < 8; ++e) r[e] = (bf16)(out[e] * inv);
    *reinterpret_cast<bf16x8*>(ctx + (size_t)i * ldc + h * 64 + ch * 8) = r;
  }
}

extern "C" int st_decode_self_attn(hipStream_t stream, const void* qkv, int ldq, void* cache, const long long* step, const int* anc,
                                   void* ctx, int ldc, int n, int S, int H, int d_k, float scale) {
  if (n <= 0) return 0;
  if (d_k != 64 || H <= 0 || S <= 0 || S > 128 || (ldq & 7) || (ldc & 7) || !qkv || !cache || !step || !ctx) return -1;
  hipLaunchKernelGGL(decode_self_attn_kernel, dim3((n * H + 3) / 4), dim3(256), 0, stream, (const bf16*)qkv, ldq, (bf16*)cache, step, anc,
                     (bf16*)ctx, ldc, n, S, H, scale);
  ST_CHECK_LAUNCH();
  return 0;
}

extern "C" int st_beam_advance(hipStream_t stream, const float* logits, int ldl, int V, int beam, int B, const long long* step,
                               int eos, float* scores, long long* tokens, unsigned char* done, long long* lengths,
                               float* hist_scores, long long* back, long long* toks, long long* order, void* work, int* anc,
                               int S, long long* step_next, const float* emb, int emb_rows, const float* pe, int pe_rows,
                               void* x_next, int D) {
  if (B <= 0) return 0;
  if (beam <= 0 || beam > 16 || V <= 0 || ldl < V || !logits || !step || !scores || !tokens || !done || !lengths || !hist_scores ||
      !back || !toks || !order)
    return -1;
  const bool wide = work && V <= 20 * 256;
  if (anc && (!wide || S <= 0 || S > 128)) return -1;       // (the lineage table is maintained by the merging wave)
  if (step_next && (!wide || step_next != step)) return -1;
  if (x_next && (!wide || !emb || !pe || emb_rows <= 0 || pe_rows <= 0 || D <= 0 || (D & 3))) return -1;
  if (wide) {                           // B * beam workgroups: see beam_row_best_kernel
    unsigned long long* w = (unsigned long long*)work;
    BeamState st{step, eos, B, scores, tokens, done, lengths, hist_scores, back, toks, order, anc, S, step_next,
                 (unsigned*)(w + (size_t)B * beam * beam), (unsigned*)(w + (size_t)B * beam * beam + 1), emb, emb_rows, pe, pe_rows,
                 (bf16*)x_next, D};
    hipLaunchKernelGGL((beam_row_best_kernel<20>), dim3(B * beam), dim3(256), 0, stream, logits, ldl, V, beam, w, st);
  } else {
    hipLaunchKernelGGL(beam_advance_kernel, dim3(B), dim3(512), 0, stream, logits, ldl, V, beam, B, step, eos, scores, tokens, done,
                       lengths, hist_scores, back, toks, order);
  }
  ST_CHECK_LAUNCH();
  return 0;
}

extern "C" int st_cache_reorder(hipStream_t stream, void* cache, const long long* order, const long long* step, int L,
                                int n, int S, int W, int beam) {
  if (L <= 0 || n <= 0 || S <= 0) return 0;
  if ((W & 7) || beam <= 0 || (n % beam) || beam * (W / 8) > 2048) return -1;
  hipLaunchKernelGGL(cache_reorder_kernel, dim3(S, n / beam, L), dim3(256), 0, stream, (bf16*)cache, order, step, n, S, W, beam);
  ST_CHECK_LAUNCH();
  return 0;
}

// ---- cross-entropy over ragged logits rows (train.py:40,120: nn.CrossEntropyLoss(ignore_index = 0), mean over the
//      non-ignored tokens).  One workgroup per row.  The kernels live in st_ce.cuh, shared with the smoothed loss of
//      st_loss.hip: these entry points launch the <false> instantiation, which contains none of the smoothing terms.
extern "C" int st_ce_fwd(hipStream_t stream, const float* logits, int ldl, int R, int V, const long long* target,
                         const long long* target_index, int ignore_index, float* lse, float* row_loss, float* sums) {
  if (R <= 0) return 0;
  if (!logits || !target || !lse || !row_loss || !sums || V <= 0 || ldl < V) return -1;
  hipLaunchKernelGGL(ce_fwd_kernel<false>, dim3(R), dim3(256), 0, stream, logits, ldl, V, target, target_index, ignore_index, lse,
                     row_loss, CeSmooth{});
  hipLaunchKernelGGL(ce_sum_kernel<false>, dim3(1), dim3(256), 0, stream, row_loss, target, target_index, ignore_index, R, sums,
                     logits, ldl, lse, CeSmooth{});
  ST_CHECK_LAUNCH();
  return 0;
}

extern "C" int st_ce_bwd(hipStream_t stream, const float* logits, int ldl, int R, int V, const long long* target,
                         const long long* target_index, int ignore_index, const float* lse, const float* sums, const float* grad_out, void* dlogits, int ldd) {
  if (R <= 0) return 0;
  if (!logits || !target || !lse || !sums || !grad_out || !dlogits || V <= 0 || ldl < V || ldd < V || (ldd & 7)) return -1;
  hipLaunchKernelGGL(ce_bwd_kernel<false>, dim3(R), dim3(256), 0, stream, logits, ldl, V, target, target_index, ignore_index, lse,
                     sums, grad_out, (bf16*)dlogits, ldd, CeSmooth{});
  ST_CHECK_LAUNCH();
  return 0;
}

extern "C" int st_cast_bf16(hipStream_t stream, const float* src, void* dst, long long n) {
  if (n <= 0) return 0;
  if (n & 7) return -1;
  const size_t n8 = (size_t)n / 8;
  int blocks = (int)((n8 + 255) / 256);
  if (blocks > 2048) blocks = 2048;
  hipLaunchKernelGGL(cast_bf16_kernel, dim3(blocks), dim3(256), 0, stream, src, (bf16*)dst, n8);
  ST_CHECK_LAUNCH();
  return 0;
}

extern "C" int st_zero_tails(hipStream_t stream, const long long* table, int n_max) {
  if (n_max <= 0) return 0;
  if (!table) return -1;
  hipLaunchKernelGGL(zero_tails_kernel, dim3(n_max, 16), dim3(256), 0, stream, table, n_max);
  ST_CHECK_LAUNCH();
  return 0;
}

// zero_grad of the flat gradient buffer (train.py:37): 16-byte stores, four per thread and iteration, one workgroup per CU slot -
// torch's fill kernel wrote config 2's 53 MB at 2 TB/s (27 us per step in the round-6 kernel trace).
namespace {
__global__ __launch_bounds__(256) void zero_kernel(f32x4* __restrict__ p, size_t n16) {
  const f32x4 z = {0.f, 0.f, 0.f, 0.f};
  const size_t stride = (size_t)gridDim.x * 256;
  size_t i = blockIdx.x * (size_t)256 + threadIdx.x;
  for (; i + 3 * stride < n16; i += 4 * stride) {
    store16<ST_ADAM_SC1>(p + i, z); store16<ST_ADAM_SC1>(p + i + stride, z); store16<ST_ADAM_SC1>(p + i + 2 * stride, z); store16<ST_ADAM_SC1>(p + i + 3 * stride, z);
  }
  for (; i < n16; i += stride) store16<ST_ADAM_SC1>(p + i, z);
}
}  // namespace

// bytes: a multiple of 16; ptr 16-byte aligned
extern "C" int st_zero(hipStream_t stream, void* ptr, long long bytes) {
  if (bytes <= 0) return 0;
  if (!ptr || (bytes & 15) || ((size_t)ptr & 15)) return -1;
  const size_t n16 = (size_t)bytes / 16;
  int blocks = (int)((n16 + 1023) / 1024);
  if (blocks > 2048) blocks = 2048;
  hipLaunchKernelGGL(zero_kernel, dim3(blocks), dim3(256), 0, stream, (f32x4*)ptr, n16);
  ST_CHECK_LAUNCH();
  return 0;
}

// ---- CTC head (BASELINE config 4: joint CTC + attention objective, transformer/Loss.py:CTCAttentionLoss) ----------------------
// torch's ctc_loss (PyTorch-ROCm, as the task prescribes for the loss heads) reads, of the [T, B, V] log-probabilities, only
// the blank column and the columns of the utterance's own labels; its gradient with respect to normalised log-probabilities
// (Graves eq. 16) is softmax - occupancy, dense in V only through the softmax term.  So the [T, B, V] log-softmax tensor
// (555 MB fp32 at config 2) is never built: st_ctc_gather takes the ragged logits rows of the encoder-side projection,
// writes each row's log-sum-exp and the <= C log-probabilities ctc_loss will read (lp[b][t][k] = logits[row(b, t)][cols[b][k]] -
// lse), and st_ctc_dlogits turns ctc_loss's small gradient back into the bf16 logits gradient the projection's backward GEMMs
// read: w[b] * softmax everywhere, the small gradient's entries at the label columns.
namespace {
__global__ __launch_bounds__(256) void ctc_gather_kernel(const float* __restrict__ logits, int ldl, int V, const long long* __restrict__ rowmap,
                                                         int T, const int* __restrict__ cols, int C, float* __restrict__ lse,
                                                         float* __restrict__ lp) {
  __shared__ float red[8];
  const int r = blockIdx.x, tid = threadIdx.x;
  const long long bt = rowmap[r];
  const float* row = logits + (size_t)r * ldl;
  // ONE pass over the row: per-thread running (max, sum of exp) pairs, merged across the workgroup (16-byte loads where the
  // row is aligned for them)
  float mx = -INFINITY, sum = 0.f;
  auto take = [&](float x) {
    if (x > mx) { sum = sum * __expf(mx - x) + 1.f; mx = x; }
    else if (mx > -INFINITY) sum += __expf(x - mx);        // (a masked logit before the first finite one: exp(-inf + inf) is NaN)
  };
  if ((ldl & 3) == 0) {
    const f32x4* row4 = reinterpret_cast<const f32x4*>(row);
    for (int v = tid; v < (V >> 2); v += 256) {
      const f32x4 x = row4[v];
      take(x[0]); take(x[1]); take(x[2]); take(x[3]);
    }
    for (int v = (V & ~3) + tid; v < V; v += 256) take(row[v]);
  } else {
    for (int v = tid; v < V; v += 256) take(row[v]);
  }
  float wmx = mx;
  for (int o = 32; o > 0; o >>= 1) wmx = fmaxf(wmx, __shfl_xor(wmx, o, 64));
  if ((tid & 63) == 0) red[tid >> 6] = wmx;
  __syncthreads();
  const float gmx = fmaxf(fmaxf(red[0], red[1]), fmaxf(red[2], red[3]));
  sum = (mx == -INFINITY) ? 0.f : sum * __expf(mx - gmx);
  mx = gmx;
  for (int o = 32; o > 0; o >>= 1) sum += __shfl_xor(sum, o, 64);
  if ((tid & 63) == 0) red[4 + (tid >> 6)] = sum;
  __syncthreads();
  const float l = mx + __logf(red[4] + red[5] + red[6] + red[7]);
  if (tid == 0) lse[r] = l;
  if (bt < 0) return;                  // (a row that belongs to no utterance: packed bucket tails)
  const int b = (int)(bt / T);
  for (int k = tid; k < C; k += 256) lp[(size_t)bt * C + k] = row[cols[b * C + k]] - l;
}

__global__ __launch_bounds__(256) void ctc_dlogits_kernel(const float* __restrict__ logits, int ldl, int V, const float* __restrict__ lse,
                                                          const long long* __restrict__ rowmap, int T, const float* __restrict__ roww,
                                                          const int* __restrict__ scat, int C, const float* __restrict__ gsmall,
                                                          const float* __restrict__ go, bf16* __restrict__ dl, int ldd) {
  const int r = blockIdx.x, tid = threadIdx.x;
  const long long bt = rowmap[r];
  const float* row = logits + (size_t)r * ldl;
  bf16* out = dl + (size_t)r * ldd;
  const int b = bt < 0 ? 0 : (int)(bt / T);
  const float g = *go, w = bt < 0 ? 0.f : roww[b] * g, l = lse[r];
  const bool al = (ldl & 3) == 0;
  for (int v = tid * 8; v < ldd; v += 256 * 8) {      // ldd % 8 == 0; columns >= V get zeros
    bf16x8 o;
    if (al && v + 8 <= V && w != 0.f) {
      const f32x4 x0 = *reinterpret_cast<const f32x4*>(row + v), x1 = *reinterpret_cast<const f32x4*>(row + v + 4);
#pragma unroll
      for (int e = 0; e < 4; ++e) { o[e] = (bf16)(__expf(x0[e] - l) * w); o[4 + e] = (bf16)(__expf(x1[e] - l) * w); }
    } else {
#pragma unroll
      for (int e = 0; e < 8; ++e) o[e] = (bf16)((v + e < V && w != 0.f) ? __expf(row[v + e] - l) * w : 0.f);
    }
    *reinterpret_cast<bf16x8*>(out + v) = o;
  }
  if (bt < 0) return;
  // the label columns: written by the SAME thread that wrote the dense 16-byte group they lie in (program order then decides;
  // a second thread's 2-byte store could reach the L2 before the first thread's 16-byte one - a barrier orders execution,
  // not the arrival of global stores)
  for (int k = 0; k < C; ++k) {
    const int c = scat[b * C + k];
    if (c >= 0 && ((c >> 3) & 255) == tid) out[c] = (bf16)(gsmall[(size_t)bt * C + k] * g);
  }
}
}  // namespace

extern "C" int st_ctc_gather(hipStream_t stream, const float* logits, int ldl, int R, int V, const long long* rowmap, int T,
                             const int* cols, int C, float* lse, float* lp) {
  if (R <= 0) return 0;
  if (!logits || !rowmap || !cols || !lse || !lp || V <= 0 || ldl < V || T <= 0 || C <= 0) return -1;
  hipLaunchKernelGGL(ctc_gather_kernel, dim3(R), dim3(256), 0, stream, logits, ldl, V, rowmap, T, cols, C, lse, lp);
  ST_CHECK_LAUNCH();
  return 0;
}

extern "C" int st_ctc_dlogits(hipStream_t stream, const float* logits, int ldl, int R, int V, const float* lse, const long long* rowmap,
                              int T, const float* roww, const int* scat, int C, const float* gsmall, const float* grad_out,
                              void* dlogits, int ldd) {
  if (R <= 0) return 0;
  if (!logits || !lse || !rowmap || !roww || !scat || !gsmall || !grad_out || !dlogits || V <= 0 || ldl < V || ldd < V || (ldd & 7) ||
      T <= 0 || C <= 0)
    return -1;
  hipLaunchKernelGGL(ctc_dlogits_kernel, dim3(R), dim3(256), 0, stream, logits, ldl, V, lse, rowmap, T, roww, scat, C, gsmall, grad_out,
                     (bf16*)dlogits, ldd);
  ST_CHECK_LAUNCH();
  return 0;
}

// ---- attention maps (return_attns: reference transformer/Attention.py:89,96, Models.py:53-54,107-109) ------------------------
// The fused attention kernels never materialise the [B, h, Lq, Lk] probabilities; when a caller asks for them
// (Encoder / Decoder / Transformer.forward(return_attns=True)) this kernel recomputes ONE sublayer's map from its projected
// queries and keys: one workgroup per (utterance, head, query), scores in LDS, max / sum by block reductions.  A
// diagnostic path (every head width that is a multiple of 8; nothing here is on the training step).
namespace {
__global__ __launch_bounds__(256) void attn_probs_kernel(const bf16* __restrict__ Q, int ldq, const bf16* __restrict__ K, int ldk,
                                                         float* __restrict__ P, const int* __restrict__ q_off,
                                                         const int* __restrict__ q_len, const int* __restrict__ k_off,
                                                         const int* __restrict__ k_len, int H, int d_k, int Lq, int Lk, int causal,
                                                         float scale) {
  extern __shared__ float sm_probs[];      // [Lk] scores, then [d_k] the query, then [8] reduction slots
  float* sc = sm_probs;
  float* qv = sm_probs + Lk;
  float* red = qv + d_k;
  const int q = blockIdx.x % Lq, h = (blockIdx.x / Lq) % H, b = blockIdx.x / (Lq * H);
  float* out = P + ((size_t)(b * H + h) * Lq + q) * Lk;
  const int lq = q_len[b], lk = k_len[b];
  const int kend = q >= lq ? 0 : (causal ? min(lk, q + 1) : lk);      // rows of padding positions: all zeros
  if (kend > 0) {
    const bf16* qr = Q + (size_t)(q_off[b] + q) * ldq + h * d_k;
    for (int i = threadIdx.x; i < d_k; i += 256) qv[i] = (float)qr[i];
    __syncthreads();
    float mx = -INFINITY;
    for (int k = threadIdx.x; k < kend; k += 256) {
      const bf16* kr = K + (size_t)(k_off[b] + k) * ldk + h * d_k;
      float acc = 0.f;
      for (int i = 0; i < d_k; i += 8) {
        const bf16x8 v = *reinterpret_cast<const bf16x8*>(kr + i);
#pragma unroll
        for (int e = 0; e < 8; ++e) acc = fmaf(qv[i + e], (float)v[e], acc);
      }
      acc *= scale;
      sc[k] = acc;
      mx = fmaxf(mx, acc);
    }
    for (int o = 32; o > 0; o >>= 1) mx = fmaxf(mx, __shfl_xor(mx, o, 64));
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = mx;
    __syncthreads();
    mx = fmaxf(fmaxf(red[0], red[1]), fmaxf(red[2], red[3]));
    float sum = 0.f;
    for (int k = threadIdx.x; k < kend; k += 256) {
      const float e = __expf(sc[k] - mx);
      sc[k] = e;
      sum += e;
    }
    for (int o = 32; o > 0; o >>= 1) sum += __shfl_xor(sum, o, 64);
    if ((threadIdx.x & 63) == 0) red[4 + (threadIdx.x >> 6)] = sum;
    __syncthreads();
    const float inv = 1.f / (red[4] + red[5] + red[6] + red[7]);
    for (int k = threadIdx.x; k < kend; k += 256) out[k] = sc[k] * inv;
  }
  for (int k = kend + threadIdx.x; k < Lk; k += 256) out[k] = 0.f;
}
}  // namespace

extern "C" int st_attn_probs(hipStream_t stream, const void* Q, int ldq, const void* K, int ldk, float* P, const int* q_off,
                             const int* q_len, const int* k_off, const int* k_len, int B, int H, int d_k, int Lq, int Lk,
                             int causal, float scale, int k_prescaled) {
  if (B <= 0 || H <= 0 || Lq <= 0 || Lk <= 0) return 0;
  if (!Q || !K || !P || !q_off || !q_len || !k_off || !k_len) return -1;
  if (k_prescaled) scale = 0.6931471805599453f;      // K holds scale * log2(e) * k: q . K is the score in the log2 domain
  if (d_k <= 0 || (d_k & 7) || (ldq & 7) || (ldk & 7)) return -2;
  const size_t smem = (size_t)(Lk + d_k + 8) * sizeof(float);
  if (smem > 64 * 1024 || (long long)B * H * Lq > 0x7fffffffLL) return -3;
  hipLaunchKernelGGL(attn_probs_kernel, dim3(B * H * Lq), dim3(256), smem, stream, (const bf16*)Q, ldq, (const bf16*)K, ldk, P, q_off,
                     q_len, k_off, k_len, H, d_k, Lq, Lk, causal, scale);
  ST_CHECK_LAUNCH();
  return 0;
}

extern "C" int st_probe_tr16(hipStream_t stream, const void* in, void* out) {
  hipLaunchKernelGGL(probe_tr16_kernel, dim3(1), dim3(64), 0, stream, (const bf16*)in, (bf16*)out);
  ST_CHECK_LAUNCH();
  return 0;
}

extern "C" int st_probe_mfma(hipStream_t stream, const void* A, const void* Bt, float* D) {
  hipLaunchKernelGGL(probe_mfma_kernel, dim3(1), dim3(64), 0, stream, (const bf16*)A, (const bf16*)Bt, D);
  ST_CHECK_LAUNCH();
  return 0;
}

namespace {
// st_clock_probe: dense MFMA work on every SIMD, the shader clock against the 100 MHz wall clock
__global__ __launch_bounds__(256) void clock_probe_kernel(long long* out, int iters) {
  const int l = threadIdx.x & 63;
  bf16x8 a, b;
#pragma unroll
  for (int e = 0; e < 8; ++e) {       // (pseudo-random operands: the clock the part holds depends on how many bits toggle)
    a[e] = (bf16)(0.001f * (float)((st_hash32(l * 8 + e + 17u * blockIdx.x) & 1023u)) - 0.5f);
    b[e] = (bf16)(0.001f * (float)((st_hash32(l * 8 + e + 977u) & 1023u)) - 0.5f);
  }
  f32x16 acc[4] = {zero16(), zero16(), zero16(), zero16()};
  __syncthreads();
  const long long t0 = clock64(), w0 = wall_clock64();
  for (int i = 0; i < iters; ++i) {
#pragma unroll
    for (int j = 0; j < 4; ++j) acc[j] = mfma32(a, b, acc[j]);
  }
  const long long t1 = clock64(), w1 = wall_clock64();
  float s = 0.f;
#pragma unroll
  for (int j = 0; j < 4; ++j)
#pragma unroll
    for (int e = 0; e < 16; ++e) s += acc[j][e];
  if (threadIdx.x == 0) {
    out[2 * blockIdx.x] = t1 - t0;
    out[2 * blockIdx.x + 1] = w1 - w0;
  }
  if (s == 123456.789f) out[0] = 0;      // (keeps the accumulators alive)
}
}  // namespace

extern "C" int st_clock_probe(hipStream_t stream, long long* out, int n_wg, int iters) {
  if (!out || n_wg <= 0 || iters <= 0) return -1;
  hipLaunchKernelGGL(clock_probe_kernel, dim3(n_wg), dim3(256), 0, stream, out, iters);
  ST_CHECK_LAUNCH();
  return 0;
}

extern "C" int st_version(void) { return ST_ABI_VERSION; }
