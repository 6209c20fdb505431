/* st_hip.h - C ABI of libst_hip.so, the MI355X (gfx950) kernels behind the
 * speech-transformer training step.
 *
 * The reference (ZhengkunTian/Speech-Tranformer-Pytorch) has no FFI: its hot
 * path is the nn.Module surface of transformer/{Attention,SubLayers,Layers,
 * Embedding,Models}.py.  The drop-in keeps those Python names (package
 * speech-tranformer-pytorch_amd/transformer) and binds THIS library through
 * ctypes (speech-tranformer-pytorch_amd/st_amd/native.py); INTEGRATION.md shows
 * the stub.  Every entry point below names the reference lines it replaces.
 *
 * Conventions
 *  - plain pointers and sizes only; all pointers are DEVICE pointers;
 *  - every call is asynchronous on `stream` (a hipStream_t),
 *    holds no global state and never synchronises the device (it is called
 *    from the autograd engine thread as well as the main thread);
 *  - return 0 on success, a positive hipError_t if the launch failed, a
 *    negative value for an argument the kernels do not support (the Python
 *    wrapper raises RuntimeError / ValueError);
 *  - "bf16" buffers are IEEE bfloat16 (uint16 storage); activations are row
 *    matrices [rows, ld]; utterance b owns rows off[b] .. off[b]+len[b]-1
 *    (packed or padded - the kernels only see offsets and lengths);
 *  - leading dimensions are in ELEMENTS and must be multiples of 8.
 */
#ifndef ST_HIP_H
#define ST_HIP_H

#ifdef __cplusplus
extern "C" {
#endif

typedef struct ihipStream_t* st_stream_t; /* == hipStream_t, spelled in plain C: no HIP header needed */

/* Library ABI version.  A host binding must refuse a library whose st_version() differs from the header it was written against:
 * through ctypes / dlsym a stale libst_hip.so would be called with shifted arguments.
 * This header is the ONLY copy of the ABI: every source under csrc/ is compiled against it (csrc/st_common.cuh includes it, so a
 * definition that disagrees with its declaration stops the build), st_version() returns this macro, and st_amd/native.py
 * parses this file at import for its argument types, ABI_VERSION and the EPI_* constants.  To add an entry point: declare
 * it here (parameter types: pointers, st_stream_t, int, unsigned, float, long, long long - the binding refuses anything
 * else), define it in csrc/, write its wrapper in st_amd/native.py.
 * The number is not a counter.  It is a FINGERPRINT of the declarations below (their names, order and parameter types, and the
 * ST_EPI_* values; comments, whitespace, parameter names and `const` do not count), computed by native.abi_fingerprint():
 *   change a declaration - importing st_amd.native fails - paste the number its message prints.
 * So it cannot be forgotten, and there is nothing in it to assert by value: no test may spell it out. */
#define ST_ABI_VERSION 1672992706
int st_version(void);

/* Re-read the development switches that choose between a specialised attention kernel and the general one
 * (ST_ATTN_FWD64=0, ST_ATTN_XS=0, ST_ATTN_BWD64=0|e).  They are read from the environment once, at the first
 * attention call; a host that changes one afterwards (same-process A/B runs in tests/ and tools/dev/) calls this. */
int st_env_refresh(void);

/* Epilogue selector of st_gemm. */
enum {
  ST_EPI_BF16 = 0,       /* D(bf16) = acc (+ bias)                                   */
  ST_EPI_BF16_RELU = 1,  /* D(bf16) = relu(acc + bias)      SubLayers.py:25          */
  ST_EPI_F32 = 2,        /* D(f32)  = acc (+ bias)          Models.py:151 (logits)   */
  ST_EPI_BF16_MASK = 3,  /* D(bf16) = acc * (aux > 0)       ReLU backward            */
  ST_EPI_BF16_ADD = 4,   /* D(bf16) = bf16(bf16(acc + bias) + aux): residual-gradient add.  TWO roundings - the GEMM result
                            is rounded to bf16 before the addend joins it (the fused st_gemm_lnbwd rounds acc + aux once
                            and differs by that rounding).  aux may be D itself (in place: same pointer, same ld) */
  ST_EPI_F32_ATOMIC = 5, /* D(f32) += acc (atomic, split-K)                          */
  ST_EPI_F32_ATOMIC_T = 6, /* D^T(f32)[j][i] += acc: weight gradients, coalesced atomics */
  ST_EPI_BF16_DELTA = 7  /* D(bf16) = acc, and delta[h][i] = sum_{j in head h} D(i,j) * (aux(i,j) + aux2(i,j)); aux2
                            (nullable, bf16, ld = ldaux) = st_attn_fwd's Ores: what rounding O to bf16 dropped */
};

/* Training-mode dropout (nn.Dropout in Attention.py:89, SubLayers.py:25,27,
 * Models.py:31).  Every entry point that can drop takes the same four
 * arguments: drop_seed (DEVICE pointer to a 32-bit seed; NULL = no dropout),
 * drop_salt (per-call-site constant), drop_thresh (round(256 p); an element
 * is kept iff its 8-bit draw >= thresh) and drop_scale (256 / (256 - thresh)).
 * Masks are a pure function of (*drop_seed, salt, element index): backward
 * entry points regenerate them from the same arguments, and a captured HIP
 * graph draws new masks on every replay once *drop_seed is advanced. */

/* D[i][j] = sum_c X(i,c) * Y(j,c), bf16 operands, fp32 accumulate (MFMA).
 * x_cmajor / y_cmajor: operand stored [c][rows] instead of [rows][c].
 * Replaces the three GEMMs of every nn.Linear on the path
 * (Attention.py:74-76,92; SubLayers.py:25-26; Models.py:145,151 and their
 * autograd backward): forward (0,0), dgrad (0,1), wgrad (1,1).
 * M rows of X, N rows of Y, Kc contraction length; `splits` > 1 only with
 * ST_EPI_F32_ATOMIC / ST_EPI_F32_ATOMIC_T (the latter stores the transposed
 * result: D is [N, ldd >= M]).
 * bias: fp32 [N], read and added to the accumulator - EXCEPT with
 * ST_EPI_F32_ATOMIC_T, where a non-NULL bias is the fp32 [N] bias-GRADIENT
 * accumulator: bias[j] += sum_c Y(j,c) (the column sums of dy, i.e. the
 * nn.Linear bias gradient, produced by the weight-gradient launch itself).
 * ST_EPI_BF16_DELTA (the dgrad that produces the attention backward's dO = d(context), aux = the forward
 * context O): `bias` is the fp32 OUTPUT delta [N / head, M] and `splits` carries the head width (32 or 64).
 * Dropout: ST_EPI_BF16_RELU drops after the ReLU (SubLayers.py:25);
 * ST_EPI_BF16_MASK multiplies the surviving (aux > 0) elements by drop_scale
 * (backward of the former; aux is the dropped activation). */
int st_gemm(st_stream_t stream, int x_cmajor, int y_cmajor, const void* X, int ldx, const void* Y, int ldy, void* D,
            int ldd, int M, int N, int Kc, float* bias, const void* aux, int ldaux, int epi, int splits,
            const unsigned* drop_seed, unsigned drop_salt, int drop_thresh, float drop_scale, const void* aux2);

/* D (bf16 [M, N]) = X Y^T + bias (operands row-major as st_gemm's plain forward form) with the output columns
 * [col_lo, col_hi) - multiples of 32 - multiplied by `scale` in fp32 BEFORE their one rounding to bf16: the q | k | v
 * projection of Attention.py:74-76 with its key block pre-scaled by scale * log2(e) for st_attn_fwd / st_attn_bwd's
 * k_prescaled mode (the row chains do the same through st_row_chain's post_kscale). */
int st_gemm_kscale(st_stream_t stream, const void* X, int ldx, const void* Y, int ldy, void* D, int ldd, int M, int N, int Kc,
                   float* bias, int col_lo, int col_hi, float scale);

/* D (bf16 [M, N]) = X Y^T (y_cmajor as st_gemm) for FEW output tiles and a LONG contraction (the vocabulary projection's input
 * gradient, Models.py:151 backward: 1,206 x 256 over 4,344): the contraction is cut `splits` ways over workgroups, every
 * split leaves its fp32 partial tile in `work` (write-through) and the last one to finish a tile adds them in split order
 * and rounds once - no atomic adds; the result does not depend on arrival order (it differs from st_gemm's in fp32
 * summation order only).  work: device scratch of 4096 + tiles * splits * 65536 bytes (tiles = ceil(M / 128) *
 * ceil(N / 128) <= 1024) whose first 4096 bytes are zero before the first call (tickets; the launch leaves them zero). */
int st_gemm_splitk(st_stream_t stream, int y_cmajor, const void* X, int ldx, const void* Y, int ldy, void* D, int ldd, int M,
                   int N, int Kc, int splits, void* work, long long work_bytes);

/* st_gemm whose Y operand (and bias) is a stack of equally shaped blocks lying y_block_stride (bias_block_stride)
 * elements apart in memory - the same nn.Linear weight of consecutive identical layers as the parameter arena
 * lays them out.  Forward (0,0): N = blocks * y_block_rows output columns, block b = rows [b * y_block_rows, ..);
 * dgrad (0,1): Kc = blocks * y_block_rows, i.e. D = sum_b X[:, block b] W_b.  y_block_rows: a power of two >= 128
 * (0 = plain st_gemm).  Used for the decoder-encoder attention of ALL decoder layers at once: their key/value
 * projections of the encoder output (Attention.py:75-76, one launch instead of one per layer) and the matching
 * input gradient.  Not available for the split-K / DELTA epilogues. */
int st_gemm_stacked(st_stream_t stream, int x_cmajor, int y_cmajor, const void* X, int ldx, const void* Y, int ldy,
                    void* D, int ldd, int M, int N, int Kc, float* bias, const void* aux, int ldaux, int epi, int splits,
                    const unsigned* drop_seed, unsigned drop_salt, int drop_thresh, float drop_scale, int y_block_rows,
                    long y_block_stride, long bias_block_stride);

/* Weight-stationary streaming GEMM for the short-contraction products (csrc/st_gemm_ws.hip): D (bf16) = epi(X W^T + bias)
 * with K = 256, N a multiple of 256, X [M, K] and W [N, K] natural.  epi: 0 = identity, 1 = ReLU (+ dropout, as
 * ST_EPI_BF16_RELU).  w_block_rows > 0: W / bias are stacks of equally spaced blocks as in st_gemm_stacked
 * (w_block_rows a power-of-two multiple of 256).  Replaces st_gemm(0, 0, ...) for Attention.py:74-76, SubLayers.py:25. */
int st_gemm_ws(st_stream_t stream, const void* X, int ldx, const void* W, int ldw, void* D, int ldd, int M, int N, int K,
               const float* bias, int epi, const unsigned* drop_seed, unsigned drop_salt, int drop_thresh,
               float drop_scale, int w_block_rows, long w_block_stride, long bias_block_stride);

/* n weight-gradient problems in ONE launch (the decoder's are ~20 workgroups
 * each: launched one by one they are pure latency).  Problem q:
 *   dW[q][N_out, K_in] (f32, ld lddw) += dY[q]^T X[q],  db[q][N_out] += colsum(dY[q])   (db or db[q] may be NULL)
 * with X[q] bf16 [tokens, K_in] (ld ldx), dY[q] bf16 [tokens, N_out] (ld lddy),
 * i.e. st_gemm(1, 1, X, ldx, dY, lddy, dW, lddw, K_in, N_out, tokens, db, .., ST_EPI_F32_ATOMIC_T, splits[q]).
 * All arrays are HOST arrays of length n (the descriptors travel in the kernel arguments). */
int st_wgrad_group(st_stream_t stream, int n, const void* const* X, const int* ldx, const void* const* dY,
                   const int* lddy, float* const* dW, const int* lddw, float* const* db, const int* tokens,
                   const int* K_in, const int* N_out, const int* splits);

/* The same contract for ENCODER-sized token counts (st_wgrad.hip): 256 x 256 output tiles, one 8-wave workgroup per
 * CU.  splits[q] cuts problem q's token axis; the caller picks it so that the launch has about one workgroup per CU:
 * sum_q ceil(K_in/256) * ceil(N_out/256) * splits[q] ~ 256 (st_amd/functional.py: flush_deferred_wgrads). */
int st_wgrad_wide(st_stream_t stream, int n, const void* const* X, const int* ldx, const void* const* dY,
                  const int* lddy, float* const* dW, const int* lddw, float* const* db, const int* tokens,
                  const int* K_in, const int* N_out, const int* splits);

/* out = LayerNorm(act(X W^T + bias) + res) * gamma + beta (+ pe[pos[row]]),
 * N = d_model in {128, 256, 512}.  Replaces output_linear + residual +
 * layernorm (Attention.py:92-94), fc2 + residual + layernorm
 * (SubLayers.py:26-27) and, with relu=1 and the PE add, the encoder front-end
 * (Models.py:28-33,42-44).  Saves xhat (bf16 [M,N]) and rstd (f32 [M]) for the
 * backward; `pre` (optional) receives the pre-LN value (front-end ReLU mask).
 * drop_where: 1 = dropout on act(X W^T + bias) before the LayerNorm
 * (Models.py:31), 2 = dropout on the LayerNorm output (SubLayers.py:27).
 *
 * The statistic (the contract of every LayerNorm in this library: here, st_row_chain, st_row_chain512, the PRE stage of
 * st_attn_f1_fwd and - the same code, not measured on its own - of st_attn_sf1_fwd): v = act(X W^T + bias) + res in fp32; mean = sum v / N; var = sum (v - mean)^2 / N - the
 * BIASED variance over the N columns; rstd = (var + eps)^-1/2 with eps INSIDE the root; xhat = (v - mean) rstd; rstd, xhat
 * and out come from the same mean and variance.  Accuracy: rstd within 1e-4 (relative, every row) of the same quantities
 * computed in fp64 from the operands as given - for rows whose mean lies up to 512 row standard deviations from zero (through
 * the bias or the residual), for rows whose variance is comparable to eps or far below it, and for a constant row, whose xhat is
 * +-0 in every element, whose out is bf16(beta) and whose rstd is eps^-1/2.  (This kernel and the 32-row chain kernels take
 * the mean first and the squared deviations then; the pipelined chain kernels sum once, about a per-row pivot - see
 * st_row_chain.  tests/test_ln_stats_gpu.py holds to it: every kernel variant st_gemm_ln dispatches to without dropout, the
 * 32-row, split and pipelined 64- / 96-row kernels of st_row_chain, st_row_chain512 and st_attn_f1_fwd; measured:
 * profiles/ln_stats_accuracy.txt.) */
int st_gemm_ln(st_stream_t stream, const void* X, int ldx, const void* W, int M, int N, int K, const float* bias,
               const void* res, int ldres, const float* gamma, const float* beta, float eps, int relu,
               const float* pe, const int* pos, void* out, int ldo, void* xhat, float* rstd, void* pre,
               const unsigned* drop_seed, unsigned drop_salt, int drop_thresh, float drop_scale, int drop_where);

/* Data-gradient GEMM + LayerNorm backward in one launch (the backward analogue of st_gemm_ln):
 *   dy = bf16(dY W (+ aux)),  dx = LayerNorm-backward(dy; xhat, rstd, gamma),  dgamma/dbeta += ..., dbias += colsum(dx)
 * dY bf16 [M, Kc], W bf16 [Kc, N] (ld ldw: an nn.Linear weight [out = Kc, in = N] as stored), N = d_model in
 * {128, 256, 512}; identical to st_gemm(0, 1, .., ST_EPI_BF16[_ADD]) followed by st_ln_bwd, without dy going to
 * HBM.  Used where a sublayer's input gradient is the previous sublayer's LayerNorm output gradient
 * (SubLayers.py:25-27 -> Attention.py:94 backward, and so on down the stack).  drop_*: the forward dropped the
 * LayerNorm output (st_gemm_ln with drop_where = 2, SubLayers.py:27); the same mask is regenerated here.
 * tests/test_lnbwd_fp64_gpu.py holds it to fp64 with that one rounding of dy: every row of dx within 1e-2 of its OWN norm (rstd over
 * six orders of magnitude, a dy that lies in the LayerNorm's null space), dbias = the column sum of dx AS STORED (bf16) within 4.4e-5. */
int st_gemm_lnbwd(st_stream_t stream, const void* dY, int lddy, const void* W, int ldw, int M, int N, int Kc,
                  const void* aux, int ldaux, const void* xhat, const float* rstd, const float* gamma, void* dx,
                  int lddx, float* dgamma, float* dbeta, float* dbias, const unsigned* drop_seed, unsigned drop_salt,
                  int drop_thresh, float drop_scale);

/* ---- row chains for decoder-sized row counts (csrc/st_rowchain.hip) ---------------------------------------------
 * Everything the decoder does between two attention kernels is row-wise; one launch runs it for blocks of 32 rows:
 *   PRE   cur = LN(A Wo^T + bo + R) * g0 + be0               (Attention.py:92-94)   out0 / xhat0 / rstd0 as st_gemm_ln
 *                                                                                    (each may be NULL when nothing outside the chain reads it)
 *   FFN   H   = dropout1(relu(cur W1^T + b1))                (SubLayers.py:25)      [M, d_ff], saved for the backward
 *                                                                                    (H may be NULL: inference - it stays on the chip)
 *         cur = dropout2(LN(H W2^T + b2 + cur) * g1 + be1)   (SubLayers.py:26-27)   out1 / xhat1 / rstd1
 *   POST  P   = cur Wp^T + bp, Wp [256 post_blocks, 256]     (Attention.py:74-76 of the NEXT attention)
 * PRE is present iff R != NULL, FFN iff d_ff > 0, POST iff post_blocks > 0; without PRE the chain input is A.
 * d_model = 256, d_ff % 256 == 0.  The weights are read from per-wave fragment streams: every GEMM is cut into
 * 256 x 256 blocks, consumed in the order  Wo | (W1 rows c*256.., W2 columns c*256..) for c = 0.. | Wp rows u*256..;
 * n_blocks = their number.  st_wfrag_build lays the blocks out (table: 4 x int64 per block on the device - address of
 * the block's first element in a row-major bf16 matrix, its leading dimension (| 1 << 32: read the block transposed),
 * 16 * (position of the block in its chain) | wave stride (n_blocks * 16 + st_wfrag_depth()) << 32, address of the
 * chain's buffer); a chain's buffer holds 8 * (n_blocks * 16 + st_wfrag_depth()) * 512 bf16.  One table may fill any
 * number of chains.  Rebuild after every weight update.
 * next_blocks > 0: another chain of that many blocks is stored right behind this one and runs next - the launch warms the
 * L2 with its streams too (the streams are read once per step, from HBM).
 * Both dropout sites read the device seed *drop_seed (NULL = off) with their own salt / threshold / scale.
 * split_work (optional; split_bytes = its size): zero-initialised device scratch of (256 + 256 * 8192) * 4 bytes (256 tickets, then the partial sums; only the tickets need the zeroes).  With it, a
 * chain that has an FFN part and whose M / 32 row blocks x (d_ff / 256) fit 256 workgroups runs d_ff / 256 workgroups per row
 * block: each does PRE, ONE 256-wide chunk of the hidden dimension and leaves its partial of the second GEMM in the
 * scratch; the last of a row block's workgroups adds them (in chunk order: the result does not depend on arrival order, but
 * differs in rounding from the one-workgroup chain) and finishes the chain.  Launches that share the scratch must be
 * ordered on one stream.
 * Both LayerNorms keep st_gemm_ln's contract of the statistic (biased variance over the 256 columns, eps inside the root, rstd
 * within 1e-4 of fp64 on off-centre, tiny-spread and constant rows) at every M.  Past 8,192 rows the pipelined kernels
 * (csrc/st_rowchain_pipe.cuh) form it from ONE pass: the fp32 sum and sum of squares of v - pivot, pivot = the row's residual
 * at column 0 plus the bias there.  Its domain: the loss of such a pass is 2^-24 rho^2 of rstd, rho = |mean of (v - pivot)| /
 * row std - of order one as long as column 0 of the row lies within a few standard deviations of the row's mean, whatever that
 * mean is.  (About zero instead of the pivot - the form before - the same law put rstd off by 1.5e-4 at a row mean of 32
 * standard deviations and 4.6e-2 at 512: profiles/ln_stats_accuracy_before.txt.) */
int st_wfrag_depth(void);
int st_wfrag_build(st_stream_t stream, const long long* table, int n_blocks);
int st_row_chain(st_stream_t stream, int M, const void* wfrag, int n_blocks, int next_blocks, float eps, const void* A,
                 int lda,
                 const void* R, int ldr, const float* bo, const float* g0, const float* be0, void* out0, void* xhat0,
                 float* rstd0, int d_ff, const float* b1, const float* b2, const float* g1, const float* be1, void* H,
                 unsigned long long* relu_bits, void* out1, void* xhat1, float* rstd1, const unsigned* drop_seed,
                 unsigned drop1_salt,
                 int drop1_thresh, float drop1_scale, unsigned drop2_salt, int drop2_thresh, float drop2_scale,
                 int post_blocks, const float* bp, void* P, int ldp, void* split_work, long long split_bytes,
                 float post_kscale);
/* post_kscale (post_blocks == 3: a q | k | v projection; 0 or 1 = plain): the KEY block leaves as (acc + bias) * post_kscale,
 * scaled in fp32 before its one rounding to bf16 - pass scale * log2(e) and hand the result to st_attn_fwd / st_attn_bwd /
 * st_attn_probs with k_prescaled = 1 (below). */

/* The same chain at d_model = 512 (BASELINE config 3's encoder; csrc/st_rowchain_pipe512.cuh): A, R, out0, xhat0, out1, xhat1 are
 * [M, 512] (leading dimension 512 for the outputs), the weight stream holds 256 x 256 blocks in the order
 *   Wo: (h, j) -> 2 h + j  |  per hidden chunk c of 256: W1 (c, j = 0, 1), W2 (h = 0, 1; c)  |  per 256-column block u of the
 *   projection: (u, j = 0, 1)          (h: output-column half, j: input-column half of the 512-wide matrices)
 * - st_amd.chains.encoder512_blocks spells it.  PRE and FFN are both required; post_blocks is 0 or 6 (a q | k | v projection
 * to 1,536 columns, key columns 512 .. 1023 scaled by post_kscale as st_row_chain does).  64-row workgroups; relu_bits:
 * st_row_chain512_mask_words(M, d_ff) words.  n_blocks = 4 + 4 d_ff / 256 + 2 post_blocks.
 * The statistic of both LayerNorms: st_gemm_ln's contract over the 512 columns, from one pass about the per-row pivot at every M
 * (as st_row_chain's pipelined kernels: same domain, same accuracy). */
int st_row_chain512(st_stream_t stream, int M, const void* wfrag, int n_blocks, int next_blocks, float eps, const void* A, int lda,
                    const void* R, int ldr, const float* bo, const float* g0, const float* be0, void* out0, void* xhat0,
                    float* rstd0, int d_ff, const float* b1, const float* b2, const float* g1, const float* be1, void* H,
                    unsigned long long* relu_bits, void* out1, void* xhat1, float* rstd1, const unsigned* drop_seed,
                    unsigned drop1_salt, int drop1_thresh, float drop1_scale, unsigned drop2_salt, int drop2_thresh,
                    float drop2_scale, int post_blocks, const float* bp, void* P, int ldp, float post_kscale);
int st_row_chain512_mask_words(int M, int d_ff);

/* relu_bits (st_row_chain: optional output, st_row_chain_bwd: input): which hidden values of the feed-forward sublayer are
 * > 0 after ReLU and dropout (the mask of SubLayers.py:25's backward), one bit per value in a layout private to the two
 * kernels; st_row_chain_mask_words(M, d_ff) 64-bit words.  The backward chain reads these instead of H. */
int st_row_chain_mask_words(int M, int d_ff);

/* The backward of a row chain in one launch; the chain's stream holds the TRANSPOSED weight blocks (st_wfrag_build table
 * entry [1] = leading dimension | 1 << 32) in the order HEAD | FFN | TAIL:
 *   HEAD  (xhat_a != NULL)  dy = sum_u dP[:, 256u..] Wp_u + G (G may be NULL; head_blocks may be 0: dy = G);  ds_a = LayerNorm-backward(dropout-backward(dy);
 *         xhat_a, rstd_a, gamma_a);  dgamma_a / dbeta_a / dbias_a accumulated atomically        (== st_gemm_lnbwd)
 *   FFN   (d_ff > 0)  dH = (ds W2) masked by H > 0, x mask_scale (== st_gemm ST_EPI_BF16_MASK);  ds_b = LayerNorm-backward(
 *         dH W1 + ds; xhat_b, rstd_b, gamma_b) and its column sums
 *   TAIL  (O != NULL)  dctx = ds Wo;  delta[h * M + i] = sum over head h's 64 columns of dctx (O + Ores)   (== ST_EPI_BF16_DELTA)
 * ds = the running gradient: ds_a after HEAD, ds_b after FFN, the input DS [M, 256] without HEAD.  Heads are 64 columns.
 * Reference lines: the backward of Attention.py:74-76,92-94 and SubLayers.py:24-28.
 * split_work / split_bytes: as st_row_chain - d_ff / 256 workgroups per row block at decoder-sized M (HEAD replicated, one
 * chunk of the hidden dimension each, the last arriver adds the partial dy in chunk order and runs the second LayerNorm
 * backward and TAIL).
 * tests/test_lnbwd_fp64_gpu.py holds every stage to fp64 from the tensors the launch itself wrote for the stage before: delta is formed
 * from dctx AS STORED (the bf16 values) times O + Ores (within 2.1e-5, element by element), dbias_a / dbias_b from ds_a / ds_b as stored. */
int st_row_chain_bwd(st_stream_t stream, int M, const void* wfrag, int n_blocks, int next_blocks, int head_blocks,
                     const void* dP, int ldp, const void* G, int ldg, const void* xhat_a, const float* rstd_a,
                     const float* gamma_a, const unsigned* drop_seed, unsigned drop_salt, int drop_thresh, float drop_scale,
                     void* ds_a, float* dgamma_a, float* dbeta_a, float* dbias_a, const void* DS, int d_ff,
                     const unsigned long long* relu_bits, float mask_scale, void* dH, const void* xhat_b, const float* rstd_b, const float* gamma_b, void* ds_b,
                     float* dgamma_b, float* dbeta_b, float* dbias_b, const void* O, const void* Ores, int ldo, void* dctx,
                     int lddc, float* delta, void* split_work, long long split_bytes, float* colsum_ws, long long colsum_bytes);
/* colsum_ws (optional; ABI 4): encoder-sized launches (HEAD + FFN + TAIL at M > 8192: st_row_chain_bwd_colsum_rows(..) > 0 workgroups) write
 * their six column sums per workgroup - [rows][dgamma_a, dbeta_a, dbias_a, dgamma_b, dbeta_b, dbias_b][256] floats, every float of
 * it - instead of adding them atomically (251 workgroups adding to the same 768 floats queue for ~4 us per LayerNorm: 66 -> 58 us per
 * launch at 24,060 rows); the d* pointers are then left alone and st_colsum_fold adds the rows to them: any time before the
 * gradients are read, several workspaces per launch.  Other launches ignore colsum_ws and add atomically. */
int st_row_chain_bwd_colsum_rows(int M, int has_head, int d_ff, int has_tail);
int st_colsum_fold(st_stream_t stream, int n, const float* const* ws, const int* rows, float* const* dst /* 6 n, NULL = skip */);

/* LayerNorm backward: dx, and atomically accumulated dgamma / dbeta / dbias
 * (dbias = column sum of dx = bias gradient of the Linear feeding the LN).
 * mask (optional bf16 [M,N]): dx is zeroed where mask <= 0 (front-end ReLU,
 * Models.py:28-33) and scaled by mask_scale elsewhere (1/(1-p) of the dropout
 * between that ReLU and the LN).  drop_*: the forward dropped the LayerNorm
 * OUTPUT (st_gemm_ln drop_where = 2): dy is masked / rescaled first.
 * tests/test_lnbwd_fp64_gpu.py holds it to fp64: every row of dx within 1e-2 of its OWN norm, dbias summed from the fp32 values BEFORE
 * their rounding (unlike the fused kernels), a mask of -0.0 or +0.0 zeroes, a positive subnormal keeps. */
int st_ln_bwd(st_stream_t stream, const void* dy, int lddy, const void* xhat, const float* rstd, const float* gamma,
              const void* mask, void* dx, int lddx, float* dgamma, float* dbeta, float* dbias, int M, int N,
              const unsigned* drop_seed, unsigned drop_salt, int drop_thresh, float drop_scale, float mask_scale);

/* Rows per work-list tile of the attention kernel that serves a problem of
 * this shape (the kernels are chosen by shape: 128-row workgroups, except
 * the forward for <= 64 queries against >= 256 keys with 64-wide heads -
 * the decoder-encoder attention - which runs 32-query workgroups).
 * which: 0 = st_attn_fwd (query tiles), 1 = st_attn_bwd work_q (query tiles),
 * 2 = st_attn_bwd work_k (key tiles). */
int st_attn_tile_rows(int which, int d_k, int max_q, int max_k, int causal);

/* Fused masked attention forward: softmax(Q K^T * scale, keys >= k_len[b]
 * and (causal) keys > query masked) V, per head; replaces Attention.py:82-90
 * and the dense masks of Utils.py:41-70.  lse (f32 [H, q_rows_total], log2
 * domain) is saved for the backward.  d_k in {32, 64, 128}.
 * work (optional, device int32 [n_work]): the (utterance, query tile) pairs
 * to run, packed (b << 16) | tile and sorted by decreasing cost, so the
 * ragged batch is list-scheduled longest-first; a tile is
 * st_attn_tile_rows(0, ...) query rows; NULL = enumerate every tile of every
 * utterance up to max_q.  drop_*: dropout on the attention
 * probabilities (Attention.py:89); pass the same values to st_attn_bwd.
 * k_prescaled: K holds scale * log2(e) * (key projection) - scaled once, in the fp32 epilogue of the GEMM that produced it
 * (st_row_chain's post_kscale) - so q . K is the score in the log2 domain and no kernel multiplies per score; forward,
 * backward and st_attn_probs of one sublayer must agree on it.  Results are those of k_prescaled = 0 on the unscaled keys
 * up to the one rounding of K; dK (st_attn_bwd) is the gradient of the UNSCALED key projection either way. */
int st_attn_fwd(st_stream_t stream, const void* Q, int ldq, const void* K, int ldk, const void* V, int ldv, void* O,
                int ldo, void* Ores, float* lse, const int* q_off, const int* q_len, const int* k_off, const int* k_len, int B,
                int H, int d_k, int max_q, int max_k, int q_rows_total, int causal, float scale, const int* work,
                int n_work, const unsigned* drop_seed, unsigned drop_salt, int drop_thresh, float drop_scale, int k_prescaled);

/* The decoder-encoder attention of Layers.py:41 TOGETHER with what stands between it and the self-attention in front of it:
 * cur = LN(ctxA Wo^T + bo + R) (the self-attention's output_linear + residual + layernorm, Attention.py:92-94; out0 / xhat0 /
 * rstd0 as st_row_chain's PRE writes them) and q = cur Wq^T + bq (Attention.py:74; Qout [rows, 256]), then st_attn_fwd on
 * that q - one launch instead of st_row_chain(PRE + POST) + st_attn_fwd.  wfrag: the two-block fragment stream of that chain
 * (st_wfrag_build), n_blocks == 2, next_blocks as st_row_chain.  Only for the shapes st_attn_f1_applicable reports
 * (d_model 256, d_k 64, max_q <= 64, max_k >= 256: the few-queries forward); otherwise -10 - callers then issue the two
 * launches.  Results are those of the two launches (same arithmetic, same order). */
int st_attn_f1_applicable(int d_model, int d_k, int max_q, int max_k);
int st_attn_f1_fwd(st_stream_t stream, const void* ctxA, int lda, const void* R, int ldr, const void* wfrag, int n_blocks,
                   int next_blocks, float eps, const float* bo, const float* g0, const float* be0, void* out0, void* xhat0,
                   float* rstd0, const float* bq, void* Qout, int ldq, const void* K, int ldk, const void* V, int ldv, void* O,
                   int ldo, void* Ores, float* lse, const int* q_off, const int* q_len, const int* k_off, const int* k_len,
                   int B, int H, int d_k, int max_q, int max_k, int q_rows_total, float scale, const int* work, int n_work,
                   const unsigned* drop_seed, unsigned drop_salt, int drop_thresh, float drop_scale);

/* st_attn_f1_fwd with the decoder's causal SELF-attention (Layers.py:39) computed in front of the chain stage, by the same launch:
 * qkv_q / qkv_k / qkv_v = the layer's q | k | v projection (leading dimension ld_qkv, head h at columns h * 64; queries and keys
 * are the utterance's own <= 64 target positions: q_off / q_len), Os / Oress / lses = what st_attn_fwd(causal = 1) writes
 * for it (Os and lses bit for bit, Oress - may be NULL - to its own precision), its dropout (Attention.py:89) with its own salt / threshold / scale on the shared device seed.
 * The context goes from there straight into output_linear + LayerNorm + q projection and the decoder-encoder attention: the
 * three launches st_attn_fwd + st_row_chain + st_attn_fwd as one.  Same shapes as st_attn_f1_fwd (-10 otherwise); H <= 8. */
int st_attn_sf1_fwd(st_stream_t stream, const void* qkv_q, const void* qkv_k, const void* qkv_v, int ld_qkv, void* Os, void* Oress,
                    int ldos, float* lses, unsigned sdrop_salt, int sdrop_thresh, float sdrop_scale, const void* R, int ldr,
                    const void* wfrag, int n_blocks, int next_blocks, float eps, const float* bo, const float* g0,
                    const float* be0, void* out0, void* xhat0, float* rstd0, const float* bq, void* Qout, int ldq, const void* K,
                    int ldk, const void* V, int ldv, void* O, int ldo, void* Ores, float* lse, const int* q_off,
                    const int* q_len, const int* k_off, const int* k_len, int B, int H, int d_k, int max_q, int max_k,
                    int q_rows_total, float scale, const int* work, int n_work, const unsigned* drop_seed, unsigned drop_salt,
                    int drop_thresh, float drop_scale);

/* Attention backward (autograd of Attention.py:82-90): dQ, dK, dV from
 * Q, K, V, O, dO, lse; `delta` is f32 [H, q_rows_total] scratch.  Two kernels:
 * parts & 1 = dQ (also writes delta), parts & 2 = dK/dV (reads delta); 3 = both.
 * O == NULL: delta is an input (st_gemm ST_EPI_BF16_DELTA wrote it with dO) and parts == 3 runs as ONE launch.
 * k_prescaled as st_attn_fwd.  It also selects the kernel: long non-causal problems with 64-wide heads (max_q, max_k > 128,
 * O == NULL) run the hand-scheduled streams of csrc/st_attn_bwd64.hip ONLY with k_prescaled = 1; with plain keys the general
 * kernels serve them (they scale the fp32 score; the streams would scale a bf16 operand and round it again - 2-4x the error
 * at the scores of a trained model, profiles/attn_sharp_accuracy_before.txt).  Same results contract either way.
 * work_q / work_k: optional work lists (see st_attn_fwd) over query tiles
 * (dQ kernel) and key tiles (dK/dV kernel) of st_attn_tile_rows(1 / 2, ...) rows. */
int st_attn_bwd(st_stream_t stream, const void* Q, int ldq, const void* K, int ldk, const void* V, int ldv,
                const void* O, int ldo, const void* dO, int lddo, const float* lse, float* delta, void* dQ, int lddq,
                void* dK, int lddk, void* dV, int lddv, const int* q_off, const int* q_len, const int* k_off,
                const int* k_len, int B, int H, int d_k, int max_q, int max_k, int q_rows_total, int causal,
                float scale, int parts, const int* work_q, int n_work_q, const int* work_k, int n_work_k,
                const unsigned* drop_seed, unsigned drop_salt, int drop_thresh, float drop_scale, int k_prescaled,
                void* split_work, long long split_bytes);
/* split_work (optional; ABI 4): st_attn_bwd_split_kib(..) KiB of scratch for the merged launch (parts = 3, O = NULL) of a few-queries /
 * many-keys problem (max_q <= 64, max_k >= 256, not causal: the decoder-encoder attention) - every dQ item's key tiles are then cut over
 * up to four workgroups, fp32 partials merged by the last arriver in part order (deterministic).  Its first 16 KiB (tickets) must be
 * zero before the first launch (the kernel leaves them zero); launches on one stream may share it.  0 KiB: the shape does not split. */
int st_attn_bwd_split_kib(int B, int H, int d_k, int max_q, int max_k, int causal);

/* row_pos[off[b]+t] = t (and row_seq[...] = b if non-null), t < len[b]:
 * the per-row position the PE add needs (Embedding.py:21-29). */
int st_row_index(st_stream_t stream, const int* off, const int* len, int B, int max_len, int* row_pos, int* row_seq);

/* Padded fp32 features [B,T,F] -> bf16 row matrix (train.py:33, Models.py:42). */
int st_pack_rows(st_stream_t stream, const float* x, int B, int T, int F, const int* off, const int* len, void* out);
/* Feature front-end fused with the ragged pack (reference Dataset.py: cmvn :89-92, concat_frame :121-143,
 * subsampling :145-153): raw padded fp32 features x [B,T,F] (in_len[b] valid frames) -> bf16 row matrix
 * out [sum(out_len), ld >= F*(1+left+right)]; output row r of utterance b is frame r*interval with its left /
 * right context blocks exactly where the reference writes them (right blocks indexed with the RIGHT width,
 * :139-141; right <= left).  stats: per-utterance Kaldi CMVN statistics f32 [B, 2, F+1] or NULL. */
int st_feat_stack(st_stream_t stream, const float* x, int B, int T, int F, const int* in_len, const float* stats,
                  int left, int right, int interval, const int* out_off, const int* out_len, int max_out_len,
                  void* out, int ld);
/* bf16 row matrix -> padded fp32 [B,T,D], zero past len[b] (Encoder/Decoder return value). */
int st_unpack_rows(st_stream_t stream, const void* x, int ld, int B, int T, int D, const int* off, const int* len,
                   float* out);
/* Backward of st_unpack_rows: padded fp32 gradient -> bf16 row matrix. */
int st_pack_grad(st_stream_t stream, const float* g, int B, int T, int D, const int* off, const int* len, void* out,
                 int ld);

/* Decoder input: out[off[b]+t] = emb[tok[b,t]] + pe[t]  (Models.py:84,87 with repair R3).  emb has V rows; a token id
   outside [0, V) traps the kernel (nn.Embedding's device assert). */
int st_embed_pe_fwd(st_stream_t stream, const long long* tok, int B, int L, const float* emb, int V, const float* pe,
                    int D, const int* off, const int* len, void* out);
/* demb[tok] += dy (f32 atomics); row pad_idx receives nothing (Models.py:74); ids outside [0, V) trap. */
int st_embed_bwd(st_stream_t stream, const long long* tok, int B, int L, const void* dy, int ld, int D,
                 const int* off, const int* len, int pad_idx, float* demb, int V);

/* One beam-search step's decoder input (Models.py:84,87): out bf16 [n, D] = emb[tokens[i]] + pe[*step] (emb f32 [V, D],
   pe f32 [>= *step + 1, D], *step a device scalar); ids outside [0, V) trap. */
int st_embed_step(st_stream_t stream, const long long* tokens, const float* emb, int V, const float* pe, const long long* step,
                  void* out, int n, int D);

/* Decode-shaped self-attention of one beam-search step (Decode.py:96-98 with a KV cache): one query per hypothesis.
   qkv bf16 [n, ldq] = this step's q | k | v (3 * H * 64 columns); cache bf16 [n][S][2 * H * 64] of ONE layer; appends k | v
   at position *step (device scalar) and writes ctx [n, ldc] = softmax(q K^T * scale) V over positions 0 .. *step.
   d_k = 64, S <= 128.  `anc`: NULL, or the lineage table int32 [n][S] that st_beam_advance maintains - position p < *step of
   hypothesis i is then read from cache row anc[i][p] (the slot the ancestor that produced it sat in), the step's own K | V
   still goes to row i: the cache rows never move and st_cache_reorder is not needed.  Every entry of the table must be a
   valid row at all times (initialise it to anc[i][p] = i). */
int st_decode_self_attn(st_stream_t stream, const void* qkv, int ldq, void* cache, const long long* step, const int* anc,
                        void* ctx, int ldc, int n, int S, int H, int d_k, float scale);

/* Beam.advance (Beam.py:43-74) for all B utterances in one launch, from the raw vocabulary logits f32 [B * beam, ldl] (V
   valid columns): log-softmax per hypothesis (Decode.py:102), the `beam` best of score + log-probability over beam x V
   (best first; Beam.py:53-57), back-pointer = flat / V, token = flat % V (Beam.py:63-66), done once the best hypothesis emits
   `eos` (Beam.py:70-72; a done utterance is frozen: identity back-pointers, scores / tokens unchanged).  Device state,
   updated in place: scores f32 [B, beam], tokens i64 [B * beam], done u8 [B], lengths i64 [B], the trellis hist_scores f32 /
   back i64 / toks i64 [S, B, beam] at row *step (device scalar), order i64 [B * beam] = the cache rows the hypotheses
   inherit (input of st_cache_reorder).  beam <= 16.  `work`: NULL, or ZEROED device scratch of B * beam * beam + 1 + B 8-byte words - with
   it (and V <= 5120) the step runs over B * beam workgroups instead of one per utterance (the `beam` best of every hypothesis
   row; the wave of an utterance's row that finishes last merges them - a ticket per utterance, no second launch); same
   results.  A -inf logit: see MASKED LOGITS (at st_ce_fwd).  Only with `work`:
   `anc`: NULL, or the lineage table int32 [B * beam][S] of st_decode_self_attn (S <= 128): the hypothesis placed in slot s
   takes over positions 0 .. *step - 1 of its origin's row of the table and gets the origin's slot as position *step.
   `step_next`: NULL, or `step` itself: the launch also advances the device step counter, *step += 1, once every utterance
   has used the old value.
   `x_next`: NULL, or bf16 [B * beam, D]: the NEXT step's decoder input, bf16(emb[token] + pe[*step + 1]) for the tokens
   just chosen (st_embed_step's arithmetic; emb f32 [emb_rows, D], pe f32 [pe_rows, D]; skipped when *step + 1 == pe_rows). */
int st_beam_advance(st_stream_t stream, const float* logits, int ldl, int V, int beam, int B, const long long* step, int eos,
                    float* scores, long long* tokens, unsigned char* done, long long* lengths, float* hist_scores,
                    long long* back, long long* toks, long long* order, void* work, int* anc, int S, long long* step_next,
                    const float* emb, int emb_rows, const float* pe, int pe_rows, void* x_next, int D);

/* Joint CTC / attention beam search (csrc/st_ctc_decode.hip; Watanabe et al. 2017, Algorithm 2).  x_t(k) = log-softmax of the
   CTC head's logits of frame t; per hypothesis the CTC state gamma f32 [n][2][T_cap] (row 0 gamma_n, row 1 gamma_b), psi f32 [n]
   (log prefix probability), last int32 [n] (last token, -1 for the empty prefix), frozen u8 [n] (emitted EOS: later
   increments are 0).  T_cap is a multiple of 64 and >= every len[b].

   st_ctc_vocab_lp: logits f32 [R][ldl] (packed encoder rows; utterance b owns rows off[b] .. off[b] + len[b] - 1) ->
   lse[r] = logsumexp(logits[r][:V]) and the vocabulary-major table lpT f32 [B][V][T_cap] = logits - lse (frames t >= len[b]: 0),
   transposed through LDS tiles.  A -inf logit gives lpT = -inf: see MASKED LOGITS (at st_ce_fwd). */
int st_ctc_vocab_lp(st_stream_t stream, const float* logits, int ldl, int R, int V, const int* off, const int* len, int B, int T_cap,
                    float* lse, float* lpT);

/* The empty prefix in every slot of every utterance (n = B * beam, beam <= 64): gamma_n = -inf, gamma_b[t] = sum_{tau <= t}
   x_tau(blank) for t < len[b] (-inf beyond), psi = 0, last = -1, frozen = 0. */
int st_ctc_prefix_init(st_stream_t stream, const float* lpT, int V, int T_cap, const int* len, int B, int beam, int blank, float* gam,
                       float* psi, int* last, unsigned char* frozen);

/* For every hypothesis i < B * beam and candidate j < K (token cand[i][j], int32): the CTC prefix score of i's prefix
   extended by it, psi(h) -> cand_psi f32 [n][K], its increment delta[i][j] = psi(h) - psi(i) (-inf when psi(h) = -inf), and
   the extension's state -> cand_gam f32 [n][K][2][T_cap].  cand == eos: psi(h) = log p_ctc(prefix), no state written;
   cand == blank (or out of range): -inf.  A frozen hypothesis gets delta 0 and cand_psi = psi(i), no state written.  `done`:
   NULL or u8 [B] - hypotheses of a done utterance are skipped (nothing written).  T_cap / 64 in {1, 2, 4, 8, 12, 16, 24, 32};
   K <= 64. */
int st_ctc_prefix_score(st_stream_t stream, const float* lpT, int V, int T_cap, const int* len, int B, int beam, int blank, int eos,
                        const int* cand, int K, const float* gam, const float* psi, const int* last, const unsigned char* frozen,
                        const unsigned char* done, float* cand_gam, float* cand_psi, float* delta);

/* The attention pre-beam: for each of n rows of decoder logits f32 [n][ldl], log-softmax over the first V columns and its K best
   (best first, lower id on ties) -> ids int32 [n][K], lp f32 [n][K].  V <= 5120, K <= min(64, V).  -inf logits: MASKED LOGITS. */
int st_beam_pre_beam(st_stream_t stream, const float* logits, int ldl, int V, int n, int K, int* ids, float* lp);

/* st_beam_advance over beam x K joint candidates: candidate (s, j) = token ids[b * beam + s][j] with score
   scores[b][s] + (1 - w) lp[.][j] + w delta[.][j] (0 <= w < 1; beam <= 16, beam <= K <= 64), the `beam` best (best first,
   lower s * K + j on ties); then the same state update, trellis row, order, lineage table (anc, S <= 128), next decoder input
   (x_next) and step counter (step_next == step, ticket = a zeroed 4-byte device word) as st_beam_advance.  `gam` non-NULL: the
   CTC state of every new hypothesis of a live utterance is moved from its parent and candidate - psi <- cand_psi, last <- token,
   gamma <- cand_gam; a frozen parent passes its psi / last / frozen on unchanged; choosing EOS freezes.  T_cap even. */
int st_beam_advance_joint(st_stream_t stream, const int* ids, const float* lp, const float* delta, int K, float ctc_weight, int beam,
                          int B, const long long* step, int eos, float* scores, long long* tokens, unsigned char* done,
                          long long* lengths, float* hist_scores, long long* back, long long* toks, long long* order, int* anc, int S,
                          long long* step_next, void* ticket, const float* emb, int emb_rows, const float* pe, int pe_rows,
                          void* x_next, int D, int T_cap, const float* cand_gam, const float* cand_psi, float* gam, float* psi,
                          int* last, unsigned char* frozen);

/* Greedy CTC decoding: out int32 [R] = arg-max of logits[r][:V] (lower id on ties). */
int st_ctc_best_path(st_stream_t stream, const float* logits, int ldl, int R, int V, int* out);

/* Beam-search decode (transformer/Decode.py with a KV cache): cache bf16 [L][n][S][W]; for every layer, position
   t <= *step (device scalar) and utterance (beam consecutive hypothesis rows), row u*beam+s <- row order[u*beam+s]
   (device int64 [n], a row of the same utterance: Beam.py:65 back-pointers), in place. */
int st_cache_reorder(st_stream_t stream, void* cache, const long long* order, const long long* step, int L, int n, int S,
                     int W, int beam);

/* fp32 master parameters -> bf16 shadow, n a multiple of 8. */
int st_cast_bf16(st_stream_t stream, const float* src, void* dst, long long n);

/* clip_grad_norm_ + Adam over the flat fp32 parameter buffer in one pass (train.py:45-46, transformer/Optim.py:
 * Adam(betas = (beta1, beta2), eps)): g *= min(1, max_norm / (*gnorm + 1e-6)) (gnorm NULL: no clipping), then the
 * update of torch.optim.Adam at step count *step (already incremented) and learning rate *lr - all three device
 * scalars.  n: elements, a multiple of 4; p, g, m (exp_avg), v (exp_avg_sq): fp32 [n].
 * grad_scale: the buffer holds gradient / grad_scale - 1 / world behind a SUMMING all-reduce (train_multi.py:161-163:
 * Horovod averages), 1 otherwise; the factor is applied together with the clip coefficient (g is left holding the
 * clipped, averaged gradient), *gnorm must be the norm of the scaled gradient (st_grad_norm with the same grad_scale).
 * Three optional pointers add behaviour, one kernel body (csrc/st_optim.cuh); each may be NULL independently, and with all
 * three NULL this is the plain update above.
 * found_inf (device f32, or NULL): when *found_inf != 0 the launch writes nothing - p, g, m, v and avg keep their bits (g is
 * NOT clipped or scaled either).  Pass guard of st_grad_norm.  With found_inf NULL and avg NULL the results are bit-identical
 * to the plain update.
 * avg (fp32 [n], or NULL): the exponential moving average of the parameters, updated after the parameter update in the same
 * pass: avg += w * (p_new - avg), w = 1.0f - d in fp32, d = decay, or with decay_warmup != 0 d = min(decay, (1 + t) / (10 + t))
 * with t = *step (the count of APPLIED updates, already incremented).  decay in [0, 1]; w == 0 leaves avg untouched.
 * win (device f32 [4], or NULL): the update over a gradient-accumulation window (st_accum_note below).  The coefficient every
 * gradient element is multiplied by is min(1, max_norm / (*gnorm + 1e-6)) * grad_scale / win[0], one fp32 scalar formed before
 * the loop; *gnorm is st_grad_norm's with the same win.  g is left holding ZEROS, not the clipped gradient: the update is the
 * next window's zero_grad.  Under *found_inf != 0 the zeros are the only thing written - p, m, v and avg keep their bits.  With
 * win[0] == 1 and found_inf clear p, m, v and avg equal those of the form with win NULL bit for bit. */
int st_adam_clip(st_stream_t stream, long long n, float* p, float* g, float* m, float* v, const float* lr,
                 const float* step, const float* gnorm, float max_norm, float beta1, float beta2, float eps,
                 float grad_scale, const float* found_inf, float* avg, float decay, int decay_warmup, const float* win);

/* Zero the unassigned tail rows of a list of row matrices in one launch (packed bucket layouts: the rows behind the
 * batch's last utterance belong to nobody; the kernels never write them, so they must read as zeros).  table (device,
 * int64 [n_max][4]): base address, bytes per row (% 16 == 0), capacity in rows, address of a device int32 holding the
 * number of valid rows; entries with a null base address are skipped. */
int st_zero_tails(st_stream_t stream, const long long* table, int n_max);
/* zero_grad of a flat buffer (train.py:37; ABI 4): `bytes` (a multiple of 16) at the 16-byte aligned `ptr` set to zero with wide stores. */
int st_zero(st_stream_t stream, void* ptr, long long bytes);

/* total_norm of clip_grad_norm_ (train.py:45) over the flat fp32 gradient buffer g [n] (n % 4 == 0) as one launch:
 * *gnorm = grad_scale * ||g||_2 (partials added in a fixed order, fp64), and - when step is not NULL - *step += 1, the optimiser's
 * step count st_adam_clip then reads.  scratch: st_grad_norm_blocks() + 1 floats owned by the caller, the last one
 * zero before the first call (the kernel leaves it zero).  Two optional pointers add behaviour, one kernel body
 * (csrc/st_optim.cuh); with either of them step is required.
 * guard (device f32 [2], or NULL): a verdict.  Same grid, same partial sums, same fixed-order fp64 merge: for finite input *gnorm
 * equals the value of the form without a guard bit for bit.  The workgroup that finishes the reduction is the single writer of
 * the verdict: a finite norm -> *step += 1, guard[0] = 0; otherwise step is left alone, guard[0] = 1 and guard[1] += 1 (a running
 * count of skipped steps).  *gnorm is written in both cases.  Non-finite: any NaN or +-inf element, and ALSO finite elements
 * whose sum of squares overflows fp32 within one workgroup's partial sum (the partials are fp32; the norm is then inf).
 * win (device f32 [4], or NULL): the norm over a gradient-accumulation window (st_accum_note below), *gnorm = grad_scale * ||g||
 * / win[0].  Without a guard there is no verdict (*step += 1 always); with a guard the verdict is ALSO bad when win[0] <= 0 (a
 * window without a single token: nothing to divide by).  Partial sums and the fixed-order fp64 merge are unchanged: with
 * win[0] == 1 and finite input *gnorm equals that of the form with win NULL bit for bit (a division by 1.0f is exact). */
int st_grad_norm_blocks(void);
int st_grad_norm(st_stream_t stream, const float* g, long long n, float* scratch, float* gnorm, float* step,
                 float grad_scale, float* guard, const float* win);

/* MASKED LOGITS - one contract for the eight entry points that form a log-sum-exp over the vocabulary (st_ce_fwd / st_ce_bwd,
 * st_ce_smooth_fwd / _bwd, st_ce_eval_fwd, st_ctc_gather / st_ctc_dlogits, st_ctc_vocab_lp, st_beam_advance with and without
 * `work`, st_beam_pre_beam) and for st_ctc_best_path: a logit of -inf is a column of probability zero, PROVIDED the row has a finite
 * column.  lse is then the log-sum-exp of the finite columns (bit for bit the logit of a row with a single finite column); the
 * column's log-probability (lp, lpT, a candidate's score) is -inf and it is chosen only after every finite candidate, lower index
 * first; its softmax and plain-loss gradient are exactly 0, its smoothed gradient exactly bf16(-q[v] * scale).  In a loss, a masked
 * column the target distribution gives no mass to (q[v] = 0: zero_col, or every column but the target when smooth = 0) costs
 * nothing - 0 x -inf is 0 - and one it gives mass to makes the row's loss +inf (a masked target included); never NaN.  A row
 * WITHOUT a finite column is undefined, and so is +inf or NaN anywhere in a row.  Columns >= V are never read by any of them.
 * tests/test_lse_fp64_gpu.py holds all of this against fp64. */

/* Cross-entropy over ragged logits rows (train.py:40,120: nn.CrossEntropyLoss(ignore_index = 0), mean over the
 * non-ignored tokens).  logits f32 [R, ldl] (V valid columns; padding columns holding -1e30 may be counted as valid),
 * target i64 [R], or - with target_index (i64 [R]) - any i64 vector read as target[target_index[r]] (the padded
 * ground truth of train.py:40 addressed through the ragged rows' positions: no gather launch).  st_ce_fwd: lse[r] = logsumexp(logits[r, :V]) (f32 [R], kept for the backward); row_loss[r] (f32 [R],
 * scratch) = lse[r] - logits[r, target[r]] on the non-ignored rows; sums (f32 [3]): [0] = their sum, [1] = their number,
 * [2] = the loss sums[0] / sums[1].  st_ce_bwd: dlogits (bf16 [R, ldd], ldd % 8 == 0, columns >= V zero) = (softmax - onehot) * *grad_out /
 * sums[1] on the non-ignored rows, 0 elsewhere - the operand of the vocabulary projection's backward GEMMs. */
int st_ce_fwd(st_stream_t stream, const float* logits, int ldl, int R, int V, const long long* target,
              const long long* target_index, int ignore_index, float* lse, float* row_loss, float* sums);
int st_ce_bwd(st_stream_t stream, const float* logits, int ldl, int R, int V, const long long* target,
              const long long* target_index, int ignore_index, const float* lse, const float* sums, const float* grad_out,
              void* dlogits, int ldd);

/* CTC head of the joint CTC + attention objective (BASELINE config 4; transformer/Loss.py:CTCAttentionLoss - the reference's
 * train_attn_and_ctc.py is empty, the head is the standard hybrid one).  Around ctc_loss (PyTorch-ROCm, or st_ctc_loss_* below) these two
 * kernels stand where the [T, B, V] log-softmax tensor and its gradient would be.  logits f32 [R, ldl]: the ragged rows of
 * the encoder-side vocabulary projection (V valid columns; padding columns at -1e30 may be counted); rowmap i64 [R]: row r is
 * frame t of utterance b with rowmap[r] = b * T + t (negative: the row belongs to nobody); cols i32 [B, C]: the vocabulary
 * column of class k of utterance b (class 0 = blank, classes 1.. = the utterance's labels as ctc_loss is given them).
 * st_ctc_gather: lse[r] = logsumexp(logits[r, :V]); lp (f32 [B, T, C]) [b][t][k] = logits[r][cols[b][k]] - lse[r] on the
 * rows that exist (the rest of lp is left untouched: ctc_loss does not read frames past an input length).
 * st_ctc_dlogits: dlogits (bf16 [R, ldd], ldd % 8 == 0) = *grad_out * (roww[b] * softmax(logits[r]) everywhere, columns >= V
 * zero; then column scat[b][k] (i32 [B, C], -1 = none) overwritten with gsmall[b][t][k]) - gsmall (f32 [B, T, C]) being
 * ctc_loss's gradient with respect to lp (which already contains the softmax term at those columns, Graves eq. 16) and
 * roww[b] the weight of utterance b's loss in the reduction (0 for an utterance whose loss is infinite: zero_infinity).
 * -inf logits (masked vocabulary entries): lp = -inf, softmax 0 - see MASKED LOGITS above. */
int st_ctc_gather(st_stream_t stream, const float* logits, int ldl, int R, int V, const long long* rowmap, int T, const int* cols,
                  int C, float* lse, float* lp);
int st_ctc_dlogits(st_stream_t stream, const float* logits, int ldl, int R, int V, const float* lse, const long long* rowmap, int T,
                   const float* roww, const int* scat, int C, const float* gsmall, const float* grad_out, void* dlogits, int ldd);

/* CTC loss with lengths and labels on the DEVICE (csrc/st_ctc_loss.hip): nothing is read from host memory, so both launches can
 * be captured into a HIP graph.  lp f32 [B, T, C]: log-probabilities over the utterance's small alphabet, class 0 = blank (what
 * st_ctc_gather writes), C >= 2; classes i64 [B, L]: class indices into C (L <= 255; a label MAY be class 0: it is an ordinary
 * label state that emits column 0 - one generic skip rule, s-2 -> s iff l'(s) != l'(s-2), covers it); in_len / tgt_len i32 [B]
 * on the device (clamped to [0, T] / [0, L]; tgt_len 0 = the single blank state).  ws: st_ctc_loss_ws_kib(B, T, L) KiB (host
 * query; -1: unsupported), holding alpha, beta (f32 [B, T, 2 L + 2] each, base-2 logarithms renormalised every 8 frames) and their f64 offsets.
 * st_ctc_loss_fwd: nll f32 [B] = -log p(labels | lp), +inf where no alignment exists; one wave per (utterance, direction).
 * st_ctc_loss_grad: g f32 [B, T, C] = coef[b] (exp(lp) - occ) for t < in_len[b], 0 past it - occ[b][t][k] the posterior
 * probability that frame t emits class k (each frame's occupancies sum to 1), i.e. -coef occ is the exact derivative of
 * coef nll with respect to lp and coef exp(lp) the log-softmax's share: the convention st_ctc_dlogits consumes; roww f32 [B] =
 * coef[b].  softmax_term = 0 leaves the exp(lp) term out (g = -coef occ: what an autograd node over lp returns).  Where nll[b] is
 * infinite g = 0 and roww[b] = 0 (zero_infinity).  The states of a class are accumulated in label
 * order: no float atomics, bitwise reproducible. */
int st_ctc_loss_ws_kib(int B, int T, int L);
int st_ctc_loss_fwd(st_stream_t stream, const float* lp, int B, int T, int C, const long long* classes, int L, const int* in_len,
                    const int* tgt_len, void* ws, long long ws_bytes, float* nll);
int st_ctc_loss_grad(st_stream_t stream, const float* lp, int B, int T, int C, const long long* classes, int L, const int* in_len,
                     const int* tgt_len, const float* coef, void* ws, long long ws_bytes, const float* nll, float* g, float* roww,
                     int softmax_term);

/* CTC forced alignment (csrc/st_ctc_align.hip): the Viterbi (best-path) alignment of the labels through the same lattice, on the
 * inputs of st_ctc_loss_fwd (lp need not be normalised: plain numbers; nothing is read from host memory, so the launch can be
 * captured).  v_0(0) = lp_0(0), v_0(1) = lp_0(c_0); v_t(s) = lp_t(l'(s)) + max(v_{t-1}(s), v_{t-1}(s-1), [l'(s) != l'(s-2)]
 * v_{t-1}(s-2)) in fp32, natural units, the wave maximum subtracted every 8 frames (integer-valued lp: every operation exact).
 * TIE RULE: predecessors are tried in the order stay, s-1, s-2, a later one wins only if strictly greater; the end state is the
 * last blank S-1 unless the last label S-2 is strictly better.
 * path i32 [B, T]: for t < in_len[b] the label position j in [0, tl) whose label state emits frame t, -1 for a blank state (a
 * label equal to class 0 is a label); -1 at and past in_len[b].  spans i32 [B, L, 2]: [start, end) frames of label position j
 * (contiguous, at least one frame), (-1, -1) for j >= tl.  score f32 [B]: the sum of lp along the path, accumulated in fp64 and
 * rounded once.  No alignment (in_len = 0, in_len < tl + adjacent repeats): score -inf, path and spans all -1.  Every byte of the
 * three outputs is written.  ws: st_ctc_align_ws_kib(B, T, L) KiB (host query, no launch; -1: unsupported; 0 when every frame count
 * fits the LDS copy of the back-pointers: 2,048 frames for L <= 127, 1,024 above), 16-byte aligned. */
int st_ctc_align_ws_kib(int B, int T, int L);
int st_ctc_align(st_stream_t stream, const float* lp, int B, int T, int C, const long long* classes, int L, const int* in_len,
                 const int* tgt_len, void* ws, long long ws_bytes, int* path, int* spans, float* score);

/* CTC prefix beam search (csrc/st_ctc_beam.hip): per utterance the `beam` most probable label prefixes under the CTC head, each
 * the sum over its alignments, with scores - one wave per utterance, one launch per batch, nothing read from host memory.
 * ids i32 / lp f32 [R][K]: the K (1..16) best classes of every packed row's log-softmax, best first (what st_beam_pre_beam writes
 * with n = R); lpb f32 [R]: the blank's log-probability of every row (blank is always a candidate, among the K best or not);
 * off, len i32 [B]: utterance b owns rows off[b] .. off[b] + len[b] - 1 (rows outside are never read).  beam 1..16, L_cap 1..255.
 * Recursion per frame t, C_t = the non-blank classes among the row's K: stay p (candidate number = slot): pb' = total(p) + lpb_t,
 * pnb' = pnb(p) + x_t(last(p)) if last(p) in C_t; extension p.c, c in C_t, len(p) < L_cap (number beam + slot K + j):
 * pnb' = (c == last(p) ? pb(p) : total(p)) + x_t(c); total = logaddexp(pb, pnb).  An extension that spells the labels of a beam
 * entry ADDS into that entry (identity by label sequence, checked label by label - never by lineage or hash alone), log-sums in
 * candidate order; the `beam` best totals are kept, lower candidate number on ties, a total of -inf never.  fp32 natural units
 * relative to the frame's best total, the normaliser carried in fp64; fixed order, no atomics: launches are bit-equal.
 * tokens i32 [B][beam][L_cap] (-1 past a length), lens i32 [B][beam], score f32 [B][beam] best first (normaliser + relative total,
 * rounded once); slots past the live prefixes: score -inf, length 0, tokens -1; len[b] = 0: the empty prefix with score 0 in slot
 * 0.  Every byte of the three outputs is written.
 * trace (NULL: not written): 16-byte records {i32 prev_slot, i32 token (-1: same prefix), f32 pb_rel, f32 pnb_rel} of the beam AFTER
 * frame t, [B][T_trace][beam] (a dead slot: -1, -1, -inf, -inf); trace_norm f64 [B][T_trace]: the normaliser after frame t (the sum
 * of the frames' best totals).  Frames t >= len[b] and t >= T_trace are not written.
 * st_ctc_beam_ws_kib: host query, no launch: -1 for an unsupported shape, else 0 - the label sequences of the beam live in LDS and
 * no state grows with the frame count, so any len[b] is supported without a workspace. */
int st_ctc_beam_ws_kib(int B, int T, int beam, int L_cap);
int st_ctc_beam_search(st_stream_t stream, const int* ids, const float* lp, const float* lpb, const int* off, const int* len, int B,
                       int K, int beam, int blank, int L_cap, int* tokens, int* lens, float* score, void* trace,
                       double* trace_norm, int T_trace);

/* st_ctc_beam_search with an n-gram language model fused into the search (the same kernel body, the same single launch; the trie
 * arrays child_lo .. oov_logp as for st_ngram_* below, order 2..5, V <= 5120).  A prefix h is ranked by log p_ctc,t(h) + G(h),
 * G(h) = sum_{i <= |h|} fmaf(scale, lm(h_i | bos, h_1 .. h_{i-1}), bias), lm the back-off score of st_ngram_score (a token without a
 * unigram: oov_logp; -inf vetoes it; scale = 0: the term is bias, nothing is looked up).  G depends on the labels alone: (pb, pnb)
 * stay pure CTC numbers and every slot carries one fp32 g - a stay keeps it, an extension p.c gets g(p) + the term of c after the
 * last order - 1 labels of p (bos before the first, nothing before that), an extension that merges into a beam entry adds CTC mass
 * only.  Selection keeps the `beam` best total + g, lower candidate number on ties, a rank of -inf never; the frame's normaliser
 * is the LARGEST CTC total among the kept candidates (with scale = bias = 0 that is the first one: every output is then bit-equal
 * to st_ctc_beam_search's).  After the last frame, if final_eos, fmaf(scale, lm(eos | h), bias) is added, and the beam is re-sorted
 * by the last frame's rank + that term, best first, slot order on ties (a rank of -inf - eos vetoed - goes last among the live
 * prefixes; without the term nothing moves).
 * tokens / lens / score as st_ctc_beam_search (score: the pure log p_ctc) in that order; fused f32 [B][beam] = G(h) (+ the eos
 * term), -inf in a dead slot: score + fused is the rank.  trace_g (NULL: not written; needs trace) f32 [B][T_trace][beam]: g of the
 * slot after frame t, -inf for a dead slot.  -1: a bad shape, scale < 0 / NaN / inf, bias not finite, oov_logp > 0, fused NULL,
 * trace_g without trace.  Nothing is read from host memory; launches are bit-equal. */
int st_ctc_beam_search_lm(st_stream_t stream, const int* ids, const float* lp, const float* lpb, const int* off, const int* len, int B,
                          int K, int beam, int blank, int L_cap, int* tokens, int* lens, float* score, void* trace,
                          double* trace_norm, int T_trace, const int* child_lo, const int* tok, const float* logp, const float* bo,
                          int nodes, int V, int order, float oov_logp, int bos, int eos, float scale, float bias, int final_eos,
                          float* fused, float* trace_g);

/* Back-off n-gram language model for shallow fusion (csrc/st_ngram.hip; st_amd/ngram.py builds the arrays).  The model is a trie
 * keyed in REVERSE - the node of the n-gram (w_1 .. w_m) is reached by w_m, w_{m-1}, .., w_1 - over token ids [0, V), V <= 5120,
 * order N in 2..5: node v < V is the unigram of token v (logp[v] = +inf: no unigram), the children of a node are the consecutive
 * nodes child_lo[node] .. child_lo[node + 1] - 1 sorted by tok; child_lo i32 [nodes + 1], tok i32 / logp f32 / bo f32 [nodes],
 * natural log, suffix-closed (an n-gram's suffix without its oldest token is stored too).  Score of candidate c after the history
 * h_k .. h_1 (h_1 most recent; the history ends at the first id outside [0, V), k <= N - 1): m = the depth the walk c, h_1, h_2, ..
 * reaches and logp_m its value (no unigram: oov_logp, m = 1); bo_j = the back-off of the node reached by h_1 .. h_j (0 from the
 * first missing child on); score = logp_m + bo_m + .. + bo_k in fp32, in that order, additions only.  Device memory only is read:
 * every entry can be captured into a graph.
 *
 * st_ngram_score: one wave per hypothesis row i < n = B * beam, lane j = candidate cand[i][j] (i32 [n][K], K <= 64); hist i32
 * [n][N - 1] oldest first, -1 = no token.  lm_out (NULL: not written) f32 [n][K] = the raw score; lp (NULL: not updated) f32
 * [n][K]: lp += scale * lm + bias (scale >= 0; with scale = 0 only the bias is added; -inf stays -inf, no NaN).  A candidate outside
 * [0, V) scores -inf.  A row whose most recent token is `eos` is frozen: raw 0, lp untouched.  done: NULL or u8 [B] - the rows of a
 * done utterance are skipped, nothing written.
 *
 * st_ngram_advance: hist[i] <- shift(hist[parent[i]]) . tokens[i], in place, one workgroup per utterance (every parent value is
 * read before any is written); parent / tokens: the i64 [n] vectors `order` / `tokens` of st_beam_advance_joint (global rows of
 * the same utterance).  A frozen parent (most recent token eos) passes its history on unchanged; done (NULL or u8 [B]): skipped.
 * beam * (N - 1) <= 256.
 *
 * st_ngram_score_seq: teacher-forced: tokens i32 [M][L_cap], lens i32 [M] -> out f32 [M][L_cap] = log p(tokens[m][t] | bos,
 * tokens[m][:t]) for t < lens[m], 0 elsewhere; one thread per (list, position), the arithmetic of st_ngram_score. */
int st_ngram_score(st_stream_t stream, const int* child_lo, const int* tok, const float* logp, const float* bo, int nodes, int V,
                   int order, float oov_logp, const int* hist, const int* cand, int n, int K, int beam, const unsigned char* done,
                   int eos, float scale, float bias, float* lm_out, float* lp);
int st_ngram_advance(st_stream_t stream, int* hist, int order, const long long* parent, const long long* tokens,
                     const unsigned char* done, int eos, int B, int beam);
int st_ngram_score_seq(st_stream_t stream, const int* child_lo, const int* tok, const float* logp, const float* bo, int nodes, int V,
                       int order, float oov_logp, const int* tokens, const int* lens, int M, int L_cap, int bos, float* out);

/* Contextual biasing: phrases ("hot words") the search and the rescoring reward (csrc/st_bias.hip; st_amd/biasing.py builds the
 * arrays).  The phrases are an Aho-Corasick automaton of S <= 65536 states over token ids >= 0, phrases of 1..32 tokens: node 0 is
 * the root, nodes are numbered breadth-first, the children of a node are the consecutive nodes child_lo[node] ..
 * child_lo[node + 1] - 1 sorted by tok; child_lo i32 [S + 1], tok i32 / fail i32 / cash f32 / phi f32 [S].  fail[node]: the longest
 * proper suffix of the node's path that is a path (strictly shallower).  cash[node]: the sum of w_p |p| over the phrases that are
 * suffixes of the node's path; phi[node] = depth x the largest weight of a phrase that continues beyond the node (0: none) - the
 * provisional reward of a match in progress.  delta(s, c): while s has no child c and s is not the root, s = fail[s]; then the
 * child if there is one, else the root (any id without an edge, negative ones too, leads to the root).  Appending c in state s adds
 *   Delta(s, c) = cash[s'] + (phi[s'] - phi[s]),  s' = delta(s, c)     in fp32, in that order;   Delta(s, eos) = -phi[s]
 * so a list closed by eos has collected exactly the reward of its complete phrase occurrences.  State -1 = frozen (eos emitted).
 * No table content can hang a kernel or make it read out of bounds: the fail loop runs at most 32 times, states are clamped to
 * [0, S), child ranges to [0, S].  Device memory only is read: every entry can be captured into a graph.
 *
 * st_bias_score: one wave per hypothesis row i < n = B * beam, lane j = candidate cand[i][j] (i32 [n][K], K <= 64); state i32 [n].
 * raw (NULL: not written) f32 [n][K] = Delta(state[i], cand[i][j]); lp (NULL: not updated) f32 [n][K]: lp = fmaf(scale, Delta, lp)
 * (scale finite, >= 0; -inf stays -inf).  A frozen row (state < 0): raw 0, lp untouched.  done: NULL or u8 [B] - the rows of a done
 * utterance are skipped, nothing read or written.
 *
 * st_bias_advance: state[i] <- -1 if state[parent[i]] < 0 or tokens[i] == eos, else delta(state[parent[i]], tokens[i]); in place,
 * one workgroup per utterance (every parent state is read before any is written); parent / tokens: the i64 [n] vectors `order` /
 * `tokens` of st_beam_advance_joint (a parent outside the utterance counts as the row itself).  done (NULL or u8 [B]): skipped.
 * beam <= 256.
 *
 * st_bias_score_seq: teacher-forced: tokens i32 [M][L_cap], lens i32 [M] -> out f32 [M][L_cap] = Delta of position t from the
 * root, for t < lens[m]; 0 elsewhere and after an eos.  One lane per list, the arithmetic of st_bias_score. */
int st_bias_score(st_stream_t stream, const int* child_lo, const int* tok, const int* fail, const float* cash, const float* phi, int S,
                  const int* state, const int* cand, int n, int K, int beam, const unsigned char* done, int eos, float scale,
                  float* raw, float* lp);
int st_bias_advance(st_stream_t stream, const int* child_lo, const int* tok, const int* fail, int S, int* state,
                    const long long* parent, const long long* tokens, const unsigned char* done, int eos, int B, int beam);
int st_bias_score_seq(st_stream_t stream, const int* child_lo, const int* tok, const int* fail, const float* cash, const float* phi,
                      int S, const int* tokens, const int* lens, int M, int L_cap, int eos, float* out);

/* Attention probabilities of ONE attention sublayer, materialised (reference transformer/Attention.py:89,96: the `attns`
 * MultiHeadAttention.forward returns; Models.py:53-54,107-109 collect them under return_attns): P (f32 [B, H, Lq, Lk],
 * dense) = softmax over keys of scale * Q K^T with keys >= k_len[b] (and, when causal, keys > the query) masked out -
 * zeros there and in the rows of query positions >= q_len[b].  Q, K: bf16 row matrices (utterance b owns rows
 * off[b] .. off[b] + len[b] - 1, head h columns h * d_k ..), d_k % 8 == 0.  A diagnostic path: the fused attention kernels
 * never write these maps. */
int st_attn_probs(st_stream_t stream, const void* Q, int ldq, const void* K, int ldk, float* P, const int* q_off,
                  const int* q_len, const int* k_off, const int* k_len, int B, int H, int d_k, int Lq, int Lk, int causal,
                  float scale, int k_prescaled);

/* Attention under an ARBITRARY dense mask / with keys and values from different tensors - the general form of
 * Attention.py:82-90 that no reference call site uses (they all pass a key-padding or key-padding | causal mask and k == v,
 * which st_attn_fwd serves through lengths): a slow path (one workgroup per (utterance, head, query) / key, fp32 FMAs) that
 * closes the module boundary.  Padded layout: utterance b owns query rows b Lq .. of Q / O / dO / dQ and key rows b Lk .. of
 * K / V / dK / dV; head h = columns h d_k ..; d_k % 8 == 0.  mask: uint8 [B, Lq, Lk], nonzero = masked (NULL: none); a row
 * with every key masked yields a zero context and zero gradients (the reference: NaN).  lse / delta: f32 [H, B Lq] (natural
 * log); P (nullable, f32 [B, H, Lq, Lk]): the probabilities before dropout (Attention.py:96).  drop_*: as everywhere.
 * Limits: a workgroup keeps one query's scores (one key's, on the key side of the backward) in 64 KiB = 16384 floats of LDS -
 *   st_attn_dense_fwd                Lk + 5 d_k + 4   <= 16384
 *   st_attn_dense_bwd, query side    2 Lk + 6 d_k + 4 <= 16384
 *   st_attn_dense_bwd, key side      2 Lq + 10 d_k    <= 16384
 * - and B H max(Lq, Lk) < 2^31; beyond them the call returns -3 and launches nothing.  The backward's range is the smaller one:
 * a caller that will differentiate checks all three before the forward (st_amd.native.attn_dense_check). */
int st_attn_dense_fwd(st_stream_t stream, const void* Q, int ldq, const void* K, int ldk, const void* V, int ldv,
                      const unsigned char* mask, void* O, int ldo, float* lse, float* P, int B, int H, int d_k, int Lq, int Lk,
                      float scale, const unsigned* drop_seed, unsigned drop_salt, int drop_thresh, float drop_scale);
int st_attn_dense_bwd(st_stream_t stream, const void* Q, int ldq, const void* K, int ldk, const void* V, int ldv,
                      const unsigned char* mask, const void* dO, int lddo, const float* lse, float* delta, void* dQ, int lddq,
                      void* dK, int lddk, void* dV, int lddv, int B, int H, int d_k, int Lq, int Lk, float scale,
                      const unsigned* drop_seed, unsigned drop_salt, int drop_thresh, float drop_scale);

/* Hardware probes used by tests to pin the MFMA / transposing-LDS-read layouts. */
int st_probe_tr16(st_stream_t stream, const void* in, void* out);
int st_probe_mfma(st_stream_t stream, const void* A, const void* Bt, float* D);

/* The shader clock this part sustains under dense matrix work (the normaliser of bench.py's MFMA roofline: the nominal 2.4 GHz is
 * not what an MI355X holds under chip-wide MFMA load).  n_wg workgroups of 256 threads (give one per CU) each run `iters` rounds of
 * four independent 32 x 32 x 16 bf16 MFMAs per wave on non-trivial operands and leave {shader-clock ticks (s_memtime), wall ticks
 * (s_memrealtime, 100 MHz)} of wave 0 in out[2 wg], out[2 wg + 1]: MHz = 100 ticks / wall.  ~2 ms at iters = 30000. */
int st_clock_probe(st_stream_t stream, long long* out, int n_wg, int iters);

/* Cross-entropy against a smoothed target over ragged logits rows (transformer/Loss.py:LabelSmoothingLoss;
   nn.CrossEntropyLoss(label_smoothing = e)).  Row r with target t != ignore_index has the target
   distribution q[v] = confidence (v == t), 0 (v == zero_col, v != t; zero_col < 0: none), smooth (every other v < V);
   Q = sum_v q[v].  row_loss[r] = -sum_v q[v] (logits[r][v] - lse[r]); ignored rows: 0.
   sums f32 [4]: [0] sum of row_loss, [1] number of non-ignored rows, [2] the loss = sums[0] / D with D = *denom
   (device f32 scalar) or, denom NULL, sums[1]; [3] the plain token-mean NLL sum(lse - logits[r][t]) / sums[1].
   V is the TRUE vocabulary: columns >= V (the -1e30 padding columns of the vocabulary projection) are never read into
   any sum.  target / target_index / ignore_index / lse / row_loss as st_ce_fwd.  zero_col >= V: refused.
   At (confidence 1, smooth 0, zero_col -1, denom NULL) both calls compute st_ce_fwd / st_ce_bwd bit for bit: the kernels
   are one body (csrc/st_ce.cuh).  -inf logits: row_loss is +inf when q gives a masked column mass, see MASKED LOGITS (at st_ce_fwd). */
int st_ce_smooth_fwd(st_stream_t stream, const float* logits, int ldl, int R, int V, const long long* target,
                     const long long* target_index, int ignore_index, float confidence, float smooth, int zero_col,
                     const float* denom, float* lse, float* row_loss, float* sums);
/* dlogits bf16 [R, ldd] = (Q exp(logits - lse) - q) * *grad_out / D on the non-ignored rows, 0 on ignored rows and in
   columns >= V. */
int st_ce_smooth_bwd(st_stream_t stream, const float* logits, int ldl, int R, int V, const long long* target,
                     const long long* target_index, int ignore_index, float confidence, float smooth, int zero_col,
                     const float* denom, const float* lse, const float* sums, const float* grad_out, void* dlogits, int ldd);

/* SpecAugment (Park et al. 2019: time and frequency masks; the time warp follows below) inside the training step.  Masks are
 * drawn per utterance from the dropout seed in device memory (drop_seed above), so a captured graph draws new masks on every
 * replay; they are applied by the kernel that converts the features to bf16 rows anyway, so no extra byte moves.
 *
 * The draw (integers only).  key = hash32(*seed + salt * 0x9e3779b9), hash32 = the dropout hash of csrc/st_common.cuh.  For
 * utterance b, mask j (time masks j = 0 .. n_time - 1, then the frequency masks) and draw d in {0, 1}:
 *   bits_d = hash32(((b * 64 + j) * 2 + d) ^ key),      pick(bits, n) = (uint64(bits) * n) >> 32
 *   time mask:       cap = min(time_width, T_raw * time_ratio_permille / 1000)   (integer division)
 *                    width = pick(bits_0, cap + 1),  start = pick(bits_1, T_raw - width + 1)
 *   frequency mask:  cap = min(freq_width, mel_bins),  width = pick(bits_0, cap + 1),  start = pick(bits_1, mel_bins - width + 1)
 * Width 0 = no mask; masked elements become 0.0 (the mean after CMVN).  Masks live in RAW coordinates: frames of the
 * unstacked utterance, bins of one raw frame.
 *
 * st_specaug_plan: table int32 [B, n_time + n_freq, 2] = (start, width) of every mask of every utterance, one small launch.
 * T_raw = (len[b] - 1) * interval + 1 + right (0 when len[b] < 1) with len on the DEVICE: pass (interval 1, right 0) with raw
 * lengths, or the stacking geometry with the lengths of already stacked / subsampled rows - then T_raw is the last raw frame
 * that can appear in a row, plus one.  n_time + n_freq <= 64. */
int st_specaug_plan(st_stream_t stream, const unsigned* seed, unsigned salt, const int* len, int B, int interval, int right,
                    int n_time, int time_width, int time_ratio_permille, int n_freq, int freq_width, int mel_bins, int* table);
/* st_pack_rows with the masks of `table` applied: x fp32 [B, T, F], F = mel_bins * (1 + left + right), rows ALREADY stacked /
 * subsampled as st_feat_stack would (left = right = 0, interval = 1: plain frames).  Column c = context slot k = c / mel_bins,
 * bin f = c % mel_bins; row r, slot k hold raw frame src(k, r * interval) by st_feat_stack's rule (csrc/st_augment.cuh) with
 * the utterance's T_raw (as st_specaug_plan computes it) for the raw length - the true raw length is not known here, so a
 * right-context slot that the reference's right-width indexing lays over another slot counts as the right context.  An
 * element is zeroed iff its source frame lies in a time mask or its bin in a frequency mask.  mel_bins % 4 == 0. */
int st_pack_rows_aug(st_stream_t stream, const float* x, int B, int T, int F, const int* off, const int* len, void* out,
                     const int* table, int n_time, int n_freq, int mel_bins, int left, int right, int interval);
/* st_feat_stack with the masks of `table` (planned with the raw lengths in_len, interval 1, right 0; mel_bins = F) applied
 * after CMVN and before stacking. */
int st_feat_stack_aug(st_stream_t stream, const float* x, int B, int T, int F, const int* in_len, const float* stats, int left,
                      int right, int interval, const int* out_off, const int* out_len, int max_out_len, void* out, int ld,
                      const int* table, int n_time, int n_freq);

/* SpecAugment's time warp (csrc/st_augment.hip): the utterance's time axis is resampled by a piecewise linear map that moves
 * one source frame by up to time_warp = W frames and keeps both ends fixed.  Integers only up to the blend, so
 * tests/_timewarp_ref.py restates it exactly.  n = the utterance's T_raw, as st_specaug_plan computes it.
 *
 * The draw.  key as above; wkey = hash32(key ^ 0x77617270); bits_d = hash32((b * 2 + d) ^ wkey) for d in {0, 1} - counters and
 * key of its own: the masks of a policy do not depend on W.
 *   W < 1 or n < 2 W + 3:  the utterance is not warped, its entry is (0, 0);
 *   otherwise              c  = W + 1 + pick(bits_0, n - 2 W - 2)     the source frame that moves, W + 1 <= c <= n - 2 - W
 *                          c' = c - W + pick(bits_1, 2 W + 1)         where it lands,              1 <= c' <= n - 2
 * The map.  Output frame u (0 <= u < n) shows source position s(u) = num / den:
 *   u < c':     num = u * c,                                        den = c'
 *   otherwise:  num = c * (n - 1 - c') + (u - c') * (n - 1 - c),    den = n - 1 - c'
 *   q = floor(num * 65536 / den),  g = q >> 16,  fr = q & 0xffff;   s(0) = 0, s(c') = c, s(n - 1) = n - 1 exactly; q is
 *   monotone in u, 0 <= g <= n - 1, and g + 1 <= n - 1 whenever fr > 0.
 *   frame u = x[g] + (fr / 65536) * (x[g + 1] - x[g]): subtraction, product and sum each rounded to fp32 (no fused
 *   multiply-add); x[g + 1] is not read when fr == 0, and the frame is then x[g] unchanged.
 * The kernels compute q in 32 bits (g = num / den, fr = ((num - g * den) << 16) / den), which is the definition while
 * num < 2^31; the two feature entry points therefore refuse inputs that could hold an utterance of more than 32,767 raw
 * frames (T * interval > 32767) instead of computing something else.  A table entry outside 1 .. n - 2 counts as (0, 0).
 * Order, as in the paper: warp first, then the masks - masks live in OUTPUT (warped) coordinates, an element under a mask is
 * +0.0 and loads nothing.
 *
 * st_specaug_plan_warp: ONE launch writes both tables - `table` bit for bit as st_specaug_plan, and warp int32 [B, 2] =
 * (c, c').  0 <= time_warp <= 32767. */
int st_specaug_plan_warp(st_stream_t stream, const unsigned* seed, unsigned salt, const int* len, int B, int interval, int right,
                         int n_time, int time_width, int time_ratio_permille, int n_freq, int freq_width, int mel_bins,
                         int time_warp, int* table, int* warp);
/* st_pack_rows_aug with the warp of `warp` applied first.  Row r, slot k show OUTPUT frame u = src(k, r * interval); the
 * source frames g and g + 1 are fetched from the stacked input itself: raw frame g stands in row r' = ceil(g / interval), slot
 * left - (r' * interval - g).  That needs right == 0 and left >= interval - 1 (every raw frame below T_raw is in some row);
 * any other geometry, and T * interval > 32767, return -1.  An utterance with the entry (0, 0) takes exactly the loads and
 * conversions of st_pack_rows_aug; so does a slot without a source frame. */
int st_pack_rows_warp(st_stream_t stream, const float* x, int B, int T, int F, const int* off, const int* len, void* out,
                      const int* table, const int* warp, int n_time, int n_freq, int mel_bins, int left, int right, int interval);
/* st_feat_stack_aug with the warp applied after CMVN and before stacking, any geometry: each of the two source frames is
 * normalised with the statistics of the unwarped utterance, then they are blended.  Both tables planned with the raw lengths
 * in_len (interval 1, right 0).  T > 32767 returns -1. */
int st_feat_stack_warp(st_stream_t stream, const float* x, int B, int T, int F, const int* in_len, const float* stats, int left,
                       int right, int interval, const int* out_off, const int* out_len, int max_out_len, void* out, int ld,
                       const int* table, const int* warp, int n_time, int n_freq);

/* Exchange two fp32 buffers in place (n % 4 == 0, both 16-byte aligned, not overlapping): the averaged weights (st_adam_clip's
 * avg) go under the model and back.  A pointer swap is not possible - parameter views and captured graphs hold addresses into
 * the arena. */
int st_swap_f32(st_stream_t stream, float* a, float* b, long long n);

/* Gradient accumulation over micro-batches with an on-device denominator.
 * A WINDOW of micro-batches adds the gradients of their SUM losses into the flat gradient buffer; what the window divides by
 * (its token count, say) is known only after the last one, and never on the host.  win (device f32 [4]) is the window's state:
 * [0] the denominator, [1] the sum of row losses, [2] the sum of plain NLL, [3] micro-batches noted.  Counts stay exact in
 * fp32 up to 2^24.
 *
 * st_accum_note: one micro-batch joins the window, after its loss forward (one thread).  sums: the f32 [4] that
 * st_ce_smooth_fwd left (run with a denominator of 1.0).  win[1] += sums[0]; win[2] += sums[3] * sums[1] (nothing when
 * sums[1] == 0: the NLL mean of no token is 0 / 0, their sum is 0); win[3] += 1; win[0] += *d - or, d NULL, win[0] = 1 (a SUM
 * criterion: no division).  out[0] = the micro-batch's own loss, sums[0] / *d (d NULL: sums[0]).  d may point into sums. */
int st_accum_note(st_stream_t stream, const float* sums, const float* d, float* win, float* out);
/* (The window's norm and update: st_grad_norm and st_adam_clip with their win pointer.)
 * The window's results, then a fresh window (one thread; after the update in stream order): out f32 [4] = {win[1] / win[0],
 * win[2] / win[0], win[0], win[3]} = {loss, plain NLL, denominator, micro-batches}; win = 0. */
int st_window_close(st_stream_t stream, float* win, float* out);

/* Forward-only validation (csrc/st_eval.hip; st_amd/evaluate.py:EvalStep): teacher-forced loss, NLL and token accuracy of a
 * dev set without a host read per batch.  Neither kernel traps, allocates or reads host memory: both can be captured.
 *
 * st_ce_eval_fwd: logits f32 [R, ldl], the first V columns are vocabulary (columns >= V - the -1e30 padding of the vocabulary
 * projection - are never read); target / target_index / ignore_index address the ground truth as in st_ce_fwd; (confidence,
 * smooth, zero_col) is the smoothed target of st_ce_smooth_fwd, (1, 0, -1) the plain loss.  One workgroup per row, one pass.
 * -inf logits as in st_ce_smooth_fwd (MASKED LOGITS, at st_ce_fwd); a masked column is never the arg-max of a row with a finite one.
 * rows f32 [R, 4] (16-byte aligned), row r = {row_loss, row_nll, row_hit, state}:
 *   state 1 (a counted token): row_loss = st_ce_smooth_fwd's row_loss (the criterion's numerator), row_nll = lse - x[t],
 *           row_hit = 1 if argmax_{v < V} x[v] == t else 0 - among equal maxima the LOWEST column is the arg-max;
 *   state 0 (t == ignore_index): 0, 0, 0;
 *   state 2 (t outside [0, V) and not ignore_index - a stray label): 0, 0, 0.  The row is counted, never dereferenced. */
int st_ce_eval_fwd(st_stream_t stream, const float* logits, int ldl, int R, int V, const long long* target,
                   const long long* target_index, int ignore_index, float confidence, float smooth, int zero_col, float* rows);
/* One workgroup sums the R rows of st_ce_eval_fwd in a fixed order, in fp64 (no atomics; the result depends on the rows
 * alone), and ADDS into the epoch accumulator acc, fp64 [8] on the device:
 *   [0] loss numerator   [1] loss denominator: the batch's counted tokens, or *denom (device f32 scalar) when denom is given
 *   [2] NLL sum          [3] counted tokens     [4] hits     [5] batches noted     [6] stray labels (state 2)     [7] spare
 * fp64 because an epoch adds 10^6 - 10^7 token losses: an fp32 running sum loses the digits checkpoints are compared by.
 * last f32 [4] (16-byte aligned) is overwritten with this batch's {loss = numerator / denominator, nll, accuracy, tokens};
 * a batch without a counted token leaves nan means (0 / 0), as nn.CrossEntropyLoss does.  R may be 0. */
int st_eval_note(st_stream_t stream, const float* rows, int R, const float* denom, double* acc, float* last);

#ifdef __cplusplus
}
#endif
#endif /* ST_HIP_H */
