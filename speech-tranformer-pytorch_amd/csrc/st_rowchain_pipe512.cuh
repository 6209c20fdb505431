// Row chains at d_model = 512 (BASELINE config 3's encoder): the pipelined forward chain of st_rowchain_pipe.cuh with 512-wide
// activations - included by st_rowchain.hip.
//
//   PRE   cur = LN(A Wo^T + bo + R) g0 + be0                       Wo [512, 512]                       4 blocks of 256 x 256
//   FFN   h = relu(cur W1^T + b1), cur = LN(h W2^T + b2 + cur)     W1 [d_ff, 512], W2 [512, d_ff]      4 per 256 hidden columns
//   POST  P = cur Wp^T + bp (q | k | v: 1,536 columns)             Wp [1536, 512]                      12 blocks
//
// 64-row workgroups (two 66 KB activation tiles of pitch 1,040 bytes: a third does not fit the 160 KB), 8 waves of 32 output
// columns per block as everywhere; a GEMM over 512 input columns is two blocks (column halves of the activation tile) into one
// accumulator, one with 512 output columns two accumulators.  Weight stream per workgroup: 32 blocks = 4 MB for 64 rows - at
// the CU's 64 B/clk as long as the 2,048 MFMA clocks per block: the per-GEMM path this replaces re-reads every activation
// from HBM between its four launches per layer (242 us at 24,060 rows).
//
// Tiles: TA holds A, then xhat0, then - as its two column halves - the hidden chunks (ping-pong) / the staged projection
// blocks, and xhat1 in between; TB holds R, then out0 (the LayerNorm output replaces the residual in place), then out1.
// Stream positions (st_amd.chains.encoder512_blocks): PRE 2 h + j | FFN p0 + 4 c + {W1 j = 0, 1; W2 h = 0, 1} | POST q0 + 2 u + j
// (h: output-column half, j: input-column half, c: hidden chunk, u: 256-column block of the projection).
#pragma once

namespace {

constexpr int DM5 = 512;
constexpr int PT5 = DM5 + 8;      // LDS row pitch in elements (1,040 B = 260 dwords: the 528-byte pitch's bank pattern)

// [64][512] tile: global (rows past M as zeros) -> registers -> LDS; 8 pieces of 16 bytes per thread
struct Tile5Regs { bf16x8 v[8]; };
__device__ __forceinline__ void tile5_load(const Ctx<2>& c, const bf16* g, int ld, Tile5Regs& t) {
#pragma unroll
  for (int p = 0; p < 8; ++p) {
    const int id = c.tid + p * 512, rr = id >> 6, cc = id & 63;
    t.v[p] = gload8(g + (size_t)(c.row0 + rr) * ld + cc * 8, rr < c.nvalid);
  }
}
__device__ __forceinline__ void tile5_store(const Ctx<2>& c, const Tile5Regs& t, bf16* lds) {
#pragma unroll
  for (int p = 0; p < 8; ++p) {
    const int id = c.tid + p * 512, rr = id >> 6, cc = id & 63;
    *reinterpret_cast<bf16x8*>(lds + rr * PT5 + cc * 8) = t.v[p];
  }
}

// LayerNorm over 512 columns: acc[h] (bias - bias[0] inside) + res; each wave holds 2 x 32 columns of every row.  As epi_ln_p: one
// pass over the distances from the row's pivot bias[0] + res[row][0].  RPIV = false: the accumulators already hold acc - pivot
// (acc_init_pivot: the second LayerNorm).  What the pivot costs this kernel: 236 -> 244 VGPRs without the projection; with it (at the
// 256-register limit either way) 12 -> 16 bytes of scratch per lane, 32 -> 60 with dropout; per step of BASELINE config 3 nothing
// beyond the spread of two runs of one build (profiles/ln_stats_bench.json; with the second LayerNorm's residual pivot subtracted in
// the epilogue it was +0.014 ms of 11.2 and outside that spread in two rounds of three).
template <bool DROP, bool RPIV = true>
__device__ __forceinline__ void epi_ln512_p(const Ctx<2>& c, f32x16 (&acc)[2][2], const bf16* res, const BiasRegs (&gamma)[2],
                                            const BiasRegs (&beta)[2], float eps, const Drop& d, bf16* t_xhat, bf16* t_out, float* red2,
                                            float* g_rstd) {
  constexpr int MT = 2;
  bf16x4 rr[2][MT][4];
#pragma unroll
  for (int h = 0; h < 2; ++h)
#pragma unroll
    for (int mt = 0; mt < MT; ++mt)
#pragma unroll
      for (int g = 0; g < 4; ++g)
        rr[h][mt][g] = *reinterpret_cast<const bf16x4*>(res + (mt * 32 + c.r) * PT5 + h * 256 + c.wave * 32 + 8 * g + 4 * c.hi);
  float pv[MT];
#pragma unroll
  for (int mt = 0; mt < MT; ++mt) pv[mt] = RPIV ? (float)res[(mt * 32 + c.r) * PT5] : 0.f;      // (false: acc_init_pivot took it)
  float s[MT], q[MT];
#pragma unroll
  for (int mt = 0; mt < MT; ++mt) {
    float s0 = 0.f, s1 = 0.f, q0 = 0.f, q1 = 0.f;
#pragma unroll
    for (int h = 0; h < 2; ++h)
#pragma unroll
      for (int g = 0; g < 4; ++g)
#pragma unroll
        for (int e = 0; e < 4; e += 2) {
          const float v0 = acc[h][mt][4 * g + e] + ((float)rr[h][mt][g][e] - pv[mt]), v1 = acc[h][mt][4 * g + e + 1] + ((float)rr[h][mt][g][e + 1] - pv[mt]);
          acc[h][mt][4 * g + e] = v0;
          acc[h][mt][4 * g + e + 1] = v1;
          s0 += v0; s1 += v1;
          q0 = fmaf(v0, v0, q0); q1 = fmaf(v1, v1, q1);
        }
    s[mt] = s0 + s1;
    q[mt] = q0 + q1;
  }
#pragma unroll
  for (int mt = 0; mt < MT; ++mt) {
    s[mt] = wave_sum32(s[mt]);
    q[mt] = wave_sum32(q[mt]);
  }
#pragma unroll
  for (int mt = 0; mt < MT; ++mt)
    *reinterpret_cast<f32x2*>(red2 + (mt * 32 + c.r) * RED2_PITCH + 2 * c.wave) = f32x2{s[mt], q[mt]};
  __syncthreads();
  f32x4 pp[MT][4];
#pragma unroll
  for (int mt = 0; mt < MT; ++mt)
#pragma unroll
    for (int w4 = 0; w4 < 4; ++w4) pp[mt][w4] = *reinterpret_cast<const f32x4*>(red2 + (mt * 32 + c.r) * RED2_PITCH + 4 * w4);
  float rstd[MT], nm[MT];
#pragma unroll
  for (int mt = 0; mt < MT; ++mt) {
    const float ss = (pp[mt][0][0] + pp[mt][0][2]) + (pp[mt][1][0] + pp[mt][1][2]) + ((pp[mt][2][0] + pp[mt][2][2]) + (pp[mt][3][0] + pp[mt][3][2]));
    const float qq = (pp[mt][0][1] + pp[mt][0][3]) + (pp[mt][1][1] + pp[mt][1][3]) + ((pp[mt][2][1] + pp[mt][2][3]) + (pp[mt][3][1] + pp[mt][3][3]));
    const float mean = ss * (1.f / DM5);      // (of the distances from the pivot)
    const float var = fmaxf(qq * (1.f / DM5) - mean * mean, 0.f);
    rstd[mt] = rsqrtf(var + eps);
    nm[mt] = -mean * rstd[mt];
  }
#pragma unroll
  for (int h = 0; h < 2; ++h)
#pragma unroll
    for (int mt = 0; mt < MT; ++mt)
#pragma unroll
      for (int g = 0; g < 4; ++g) {
        const int jl = h * 256 + c.wave * 32 + 8 * g + 4 * c.hi, row = mt * 32 + c.r;
        uint32_t bits = 0;
        if (DROP) bits = d.bits(drop_counter_rc(c.row0 + row, jl, DM5));
        bf16x4 xh, o;
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          const float n = fmaf(acc[h][mt][4 * g + e], rstd[mt], nm[mt]);
          float v = fmaf(n, gamma[h].v[g][e], beta[h].v[g][e]);
          if (DROP && d.on()) v = d.keep(bits, e) ? v * d.scale : 0.f;
          xh[e] = (bf16)n;
          o[e] = (bf16)v;
        }
        *reinterpret_cast<bf16x4*>(t_xhat + row * PT5 + jl) = xh;
        *reinterpret_cast<bf16x4*>(t_out + row * PT5 + jl) = o;
      }
  if (g_rstd && c.wave == 0 && c.hi == 0) {
#pragma unroll
    for (int mt = 0; mt < MT; ++mt)
      if (mt * 32 + c.r < c.nvalid) g_rstd[c.row0 + mt * 32 + c.r] = rstd[mt];
  }
}

// PRE + FFN [+ POST of six 256-column blocks]
template <bool POST, bool DROP>
__global__ __launch_bounds__(512, 1) void row_chain512_kernel(ChainArgs a) {
  constexpr int MT = 2, RB = 64, TE = RB * PT5;
  __shared__ __attribute__((aligned(16))) bf16 tiles[2 * TE];
  __shared__ __attribute__((aligned(16))) float red2[MT * 32 * RED2_PITCH];
  Ctx<MT> c;
  c.tid = threadIdx.x; c.wave = __builtin_amdgcn_readfirstlane(c.tid >> 6); c.l = c.tid & 63; c.hi = c.l >> 5; c.r = c.l & 31;
  c.row0 = blockIdx.x * RB; c.nvalid = min(RB, a.M - c.row0);
  const bf16x8* sbase = a.wfrag + (size_t)c.wave * a.wave_frags * 64;
  auto blk = [&](int b) { return sbase + (size_t)b * 16 * 64; };
  c.ws = sbase;
#pragma unroll
  for (int i = 0; i < 8; ++i) c.ring[i] = sbase[i * 64 + c.l];
  int touched;
  {
    const int nlines = NW * a.wave_frags * 8;
    const int ln = min(((int)blockIdx.x >> 3) * 512 + c.tid, nlines - 1);
    __builtin_amdgcn_sched_barrier(0);
    touched = *reinterpret_cast<const int*>(reinterpret_cast<const char*>(a.wfrag) + (size_t)ln * 128);
    __builtin_amdgcn_sched_barrier(0);
  }
  bf16* TA = tiles; bf16* TB = tiles + TE;
  const Drop d1 = make_drop(a.drop1), d2 = make_drop(a.drop2), off = make_drop(DropArgs{nullptr, 0u, 0, 1.f});
  const int nc = a.nc, p0 = 4, q0 = p0 + 4 * nc;
  auto W1 = [&](int ch, int j) { return blk(p0 + 4 * ch + j); };
  auto W2 = [&](int ch, int h) { return blk(p0 + 4 * ch + 2 + h); };
  auto PB = [&](int u, int j) { return blk(q0 + 2 * u + j); };
  auto desc = [&](const bf16* t, bf16* g, int ld) { return tile_out_desc(c, t, g, ld, PT5); };
  auto bits_at = [&](int ch) {
    return a.relu_bits ? a.relu_bits + ((size_t)(blockIdx.x * nc + ch) * NW + c.wave) * 64 + c.l : nullptr;
  };
  NoSide ns;
  BiasRegs nb1;
  f32x16 acc2[2][MT];      // PRE's accumulators, then the feed-forward's second GEMM

  // ---- PRE: output_linear + residual + LayerNorm
  {
    Tile5Regs ra, rr;
    BiasRegs bo[2], g0[2], be0[2];
    tile5_load(c, a.A, a.lda, ra);
    bias_load(c, a.bo, bo[0]);
    bias_load(c, a.bo + 256, bo[1]);
    const float pb0 = a.bo[0];                // the bias part of the LayerNorm's pivot (epi_ln512_p): asked for with the vector
    tile5_store(c, ra, TA);
    __builtin_amdgcn_sched_barrier(0);
    tile5_load(c, a.R, a.ldr, rr);            // (asked for once A is here: st_rowchain_pipe.cuh)
#pragma unroll
    for (int h = 0; h < 2; ++h) {
      bias_load(c, a.g0 + h * 256, g0[h]);
      bias_load(c, a.be0 + h * 256, be0[h]);
    }
    __syncthreads();
    acc_init(acc2[0], bo[0], pb0);
    acc_init(acc2[1], bo[1], pb0);
    block_mma_pt<PT5>(c, blk(0), blk(1), TA, acc2[0], ns);
    tile5_store(c, rr, TB);                   // the residual arrived under the block
    block_mma_pt<PT5>(c, blk(1), blk(2), TA + 256, acc2[0], ns);
    block_mma_pt<PT5>(c, blk(2), blk(3), TA, acc2[1], ns);
    block_mma_pt<PT5>(c, blk(3), W1(0, 0), TA + 256, acc2[1], ns);
    bias_load(c, a.b1, nb1);
    __syncthreads();                          // residual visible; every wave is past its MFMAs on the A tile
    epi_ln512_p<false>(c, acc2, TB, g0, be0, a.eps, off, TA, TB, red2, a.rstd0);      // xhat0 -> TA, out0 replaces the residual in TB
    __syncthreads();
  }
  bf16* cur = TB;

  // ---- FFN
  const int dff = nc * 256;
  f32x16 acc1[MT];
  {
    BiasRegs b2[2];
    bias_load(c, a.b2, b2[0]);
    bias_load(c, a.b2 + 256, b2[1]);
    const float pb2 = a.b2[0];
    acc_init(acc1, nb1);
    if (nc > 1) bias_load(c, a.b1 + 256, nb1);
    {       // W1_0: its two blocks carry the copies of xhat0 (TA) and out0 (TB)
      CopySide<MT, 2> cs{c, {desc(TA, a.xhat0, DM5), desc(TA + 256, a.xhat0 ? a.xhat0 + 256 : nullptr, DM5)}};
      block_mma_pt<PT5>(c, W1(0, 0), W1(0, 1), cur, acc1, cs);
    }
    {
      CopySide<MT, 2> cs{c, {desc(TB, a.out0, DM5), desc(TB + 256, a.out0 ? a.out0 + 256 : nullptr, DM5)}};
      block_mma_pt<PT5>(c, W1(0, 1), nc > 1 ? W1(1, 0) : W2(0, 0), cur + 256, acc1, cs);
    }
    acc_init_pivot(c, acc2[0], b2[0], pb2, cur, PT5);      // (cur = out0, complete: the second LayerNorm's whole pivot)
    acc_init_pivot(c, acc2[1], b2[1], pb2, cur, PT5);
  }
  __syncthreads();        // every wave is past its copies of xhat0: TA's halves take the hidden chunks
  {
    EpiSide<true, DROP, MT, PT5> e0{c, acc1, TA, d1, 0, dff, 1.f, bits_at(0)};
    e0.all();
  }
  __syncthreads();
  // hidden chunk c lives in TA's column half (c & 1); its copy to H rides under W1_(c+1)
  for (int ch = 0; ch + 1 < nc; ++ch) {
    bf16* hc = TA + (ch & 1) * 256;
    bf16* hn = TA + ((ch + 1) & 1) * 256;
    acc_init(acc1, nb1);
    if (ch + 2 < nc) bias_load(c, a.b1 + (ch + 2) * 256, nb1);
    {
      CopySide<MT, 1> cs{c, {desc(hc, a.H ? a.H + ch * 256 : nullptr, dff)}};
      block_mma_pt<PT5>(c, W1(ch + 1, 0), W1(ch + 1, 1), cur, acc1, cs);
    }
    block_mma_pt<PT5>(c, W1(ch + 1, 1), W2(ch, 0), cur + 256, acc1, ns);
    {
      EpiSide<true, DROP, MT, PT5> es{c, acc1, hn, d1, (ch + 1) * 256, dff, 1.f, bits_at(ch + 1)};
      block_mma_pt<PT5>(c, W2(ch, 0), W2(ch, 1), hc, acc2[0], es);
    }
    block_mma_pt<PT5>(c, W2(ch, 1), ch + 2 < nc ? W1(ch + 2, 0) : W2(ch + 1, 0), hc, acc2[1], ns);
    __syncthreads();
  }
  {
    BiasRegs g1[2], be1[2];
    bf16* hl = TA + ((nc - 1) & 1) * 256;
#pragma unroll
    for (int h = 0; h < 2; ++h) {
      bias_load(c, a.g1 + h * 256, g1[h]);
      bias_load(c, a.be1 + h * 256, be1[h]);
    }
    if (POST) bias_load(c, a.bp, nb1);
    {
      CopySide<MT, 1> cs{c, {desc(hl, a.H ? a.H + (nc - 1) * 256 : nullptr, dff)}};
      block_mma_pt<PT5>(c, W2(nc - 1, 0), W2(nc - 1, 1), hl, acc2[0], cs);
    }
    block_mma_pt<PT5>(c, W2(nc - 1, 1), PB(0, 0), hl, acc2[1], ns);
    __syncthreads();      // every wave is past its MFMAs on and its copy of the last chunk: TA takes xhat1
    epi_ln512_p<DROP, false>(c, acc2, cur, g1, be1, a.eps, d2, TA, cur, red2, a.rstd1);      // xhat1 -> TA, out1 replaces cur in place
    __syncthreads();
  }

  if (POST) {
    // six 256-column blocks of the projection, two weight blocks each; block u's accumulators are finished beside block u + 1's
    // second weight block into TA's column half (u & 1), a staged block leaves beside block u + 2's first
    f32x16 accA[MT], accB[MT];
    auto stage = [&](int u) { return TA + (u & 1) * 256; };
    auto pdesc = [&](int u) { return desc(stage(u), a.P ? a.P + u * 256 : nullptr, a.ldp); };
    auto oscale = [&](int u) { return (u == 2 || u == 3) ? a.post_kscale : 1.f; };      // the key columns 512 .. 1023
    acc_init(accA, nb1);
    bias_load(c, a.bp + 256, nb1);
    {
      CopySide<MT, 2> cs{c, {desc(TA, a.xhat1, DM5), desc(TA + 256, a.xhat1 ? a.xhat1 + 256 : nullptr, DM5)}};
      block_mma_pt<PT5>(c, PB(0, 0), PB(0, 1), cur, accA, cs);
    }
    {
      CopySide<MT, 2> cs{c, {desc(TB, a.out1, DM5), desc(TB + 256, a.out1 ? a.out1 + 256 : nullptr, DM5)}};
      block_mma_pt<PT5>(c, PB(0, 1), PB(1, 0), cur + 256, accA, cs);
    }
    __syncthreads();      // TA free
#define ST_P512(U, ACC_NEW, ACC_OLD)                                                                                   \
    {                                                                                                                  \
      acc_init(ACC_NEW, nb1);                                                                                          \
      if (U + 1 < 6) bias_load(c, a.bp + (U + 1) * 256, nb1);                                                          \
      if (U >= 2) {                                                                                                    \
        CopySide<MT, 1> cs{c, {pdesc(U - 2)}};                                                                         \
        block_mma_pt<PT5>(c, PB(U, 0), PB(U, 1), cur, ACC_NEW, cs);                                                    \
      } else {                                                                                                         \
        block_mma_pt<PT5>(c, PB(U, 0), PB(U, 1), cur, ACC_NEW, ns);                                                    \
      }                                                                                                                \
      EpiSide<false, false, MT, PT5> es{c, ACC_OLD, stage(U - 1), off, 0, 0, oscale(U - 1), nullptr};                  \
      block_mma_pt<PT5>(c, PB(U, 1), PB(U + 1, 0), cur + 256, ACC_NEW, es);                                            \
      __syncthreads();                                                                                                 \
    }
    ST_P512(1, accB, accA)
    ST_P512(2, accA, accB)
    ST_P512(3, accB, accA)
    ST_P512(4, accA, accB)
    ST_P512(5, accB, accA)
#undef ST_P512
    {       // the last block's epilogue and the last two copies are exposed
      EpiSide<false, false, MT, PT5> es{c, accB, stage(5), off, 0, 0, oscale(5), nullptr};
      es.all();
    }
    tile_out_now(c, pdesc(4));
    __syncthreads();
    tile_out_now(c, pdesc(5));
  } else {
    tile_out_now(c, desc(TA, a.xhat1, DM5));
    tile_out_now(c, desc(TA + 256, a.xhat1 ? a.xhat1 + 256 : nullptr, DM5));
    tile_out_now(c, desc(TB, a.out1, DM5));
    tile_out_now(c, desc(TB + 256, a.out1 ? a.out1 + 256 : nullptr, DM5));
  }
  if (touched == 0x5a5a5a5a && a.M < 0) red2[0] = 1.f;      // (never true: keeps the warm-up load alive)
}

}  // namespace
