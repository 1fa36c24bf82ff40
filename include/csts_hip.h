/* csts_hip.h -- C ABI of libcsts_hip.so, the MI355X (gfx950) kernel library behind the CSTS hot path.
 *
 * The reference (BolinLai/CSTS) owns no native code: its "FFI" for this path is the set of torch.nn ops
 * its model calls.  Each entry point below replaces one such op (forward and backward),
 * and cites the reference call site it stands in for (paths relative to the reference root).
 *
 * Conventions
 *   - plain pointers + sizes, no torch types; every pointer is DEVICE memory unless stated otherwise.
 *   - tensors are token-major: (B, N = T*H*W, C) row-major, C fastest; "dt" arguments are CSTS_F32 / CSTS_BF16.
 *   - every function enqueues work on `stream` and returns immediately: 0 on success, negative on a
 *     rejected call (then csts_last_error() -- thread local -- describes why).  No allocation, no
 *     synchronisation, no global state: workspaces are supplied by the caller (size queries alongside),
 *     calls are safe from any host thread (e.g. the autograd worker) and are hipGraph-capturable.
 */
#ifndef CSTS_HIP_H
#define CSTS_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#ifndef __HIP_PLATFORM_AMD__
typedef struct ihipStream_t* hipStream_t;
#endif

enum { CSTS_F32 = 0, CSTS_BF16 = 1, CSTS_HALF = 1 };   /* CSTS_HALF: the 16-bit type of the build (see csts_half_kind) */
enum { CSTS_GEMM_NT = 0, CSTS_GEMM_NN = 1, CSTS_GEMM_TN = 2 };
enum { CSTS_EPI_NONE = 0, CSTS_EPI_GELU = 1, CSTS_EPI_DGELU = 2 };
enum { CSTS_MASK_NONE = 0, CSTS_MASK_SPATIAL = 1 };

/* Version of this header's struct layouts and call semantics.  Bumped whenever a struct grows or a field changes meaning
 * (2: csts_gemm_args.res_up; 3: compact k|v rows, 16-bit build, loss scaler in csts_opt_args; 4: csts_opt_args.extra_sq, factored AdamW; 5: grouped stencil weight gradients; 6: csts_copy_token_segments, csts_wgrad_grouped8_limited; 7: csts_wgrad_grouped5, csts_gemm algo 500; 8: csts_opt_rule, csts_opt_step, csts_opt_factored_step, csts_opt_factored.tensor replaces pad_; 10: csts_audio_pixel_attn; 11: csts_attention_track, csts_attention_rescale; 12: csts_resample_wav, csts_resample_len; 13: csts_attn_route; 14: 4:2:0 frames, csts_yuv_to_rgb, csts_*_sample_yuv; still 14: csts_stream_*, then csts_resample_stream, csts_resample_ready, csts_resample_first_input, csts_live_track_*, csts_group_*, csts_group_live_* (new entry points only, no struct or call changed)).  csts_abi_version() returns the value the
 * LIBRARY was built with: a caller must compare it with the CSTS_ABI_VERSION it was compiled against and refuse a mismatch
 * (the Python binding does, csts_amd/lib.py::load). */
#define CSTS_ABI_VERSION 14
const char* csts_last_error(void);
int csts_abi_version(void);
int csts_half_kind(void);   /* the 16-bit type behind CSTS_BF16 in THIS library: 0 bfloat16 (libcsts_hip.so), 1 IEEE half (libcsts_hip_f16.so) */

/* ---- GEMM: nn.Linear (attention.py:88-89,130,159; common.py:20-33; custom_multimodal_builder.py:223-224),
 *      the (1,8,8) fusion Conv3d as a skinny GEMM (custom_multimodal_builder.py:227-229) and the patch-embed
 *      Conv3d after im2col (stem_helper.py:27-38); plus their data- and weight-gradients.
 *      NT: C = A[M,K] B[N,K]^T ; NN: C = A[M,K] B[K,N] ; TN: C = A[K,M]^T B[K,N].
 *      epilogue: v = acc + bias[n]; GELU: aux[m,n] = v, v = gelu_erf(v); DGELU: v *= gelu'(aux[m,n]);
 *                v *= row_scale[m / rows_per_scale] (drop-path, common.py:46-59); v += residual[m % res_row_mod, n].
 *      res_up = {Ti, Hi, Wi, To, Ho, Wo} (To > 0): `residual` is the COARSE token grid [B * Ti*Hi*Wi][ldr] of the decoder's
 *                skip and row m of C is fine token (b, to, ho, wo) of [B * To*Ho*Wo]: the epilogue adds
 *                nn.Upsample(mode='trilinear', align_corners=False)(residual)[m, n] (attention.py:463-471), computed with the
 *                arithmetic of csts_trilinear_fwd -- the upsampled skip never goes through HBM.  To, Ho, Wo powers of two,
 *                split_k == 1, res_row_mod == 0; not for the persistent LDS-DMA kernels (the library picks accordingly).
 *      split_k > 1: with a workspace, deterministic partial slabs + finishing pass (full epilogue);
 *                   without, fp32 atomic accumulation into a pre-zeroed f32 C (bias only). */
typedef struct {
  int layout;
  const void* A; int a_dt; int64_t lda;
  const void* B; int b_dt; int64_t ldb;
  void* C; int c_dt; int64_t ldc;
  int64_t M, N, K;
  const float* bias;
  int epilogue;
  void* aux; int aux_dt; int64_t ldaux;
  const void* residual; int r_dt; int64_t ldr; int64_t res_row_mod;
  const float* row_scale; int64_t rows_per_scale;
  int compute;   /* CSTS_BF16: v_mfma_f32_32x32x16_bf16 ; CSTS_F32: v_mfma_f32_32x32x2_f32 (exact fp32) */
  int split_k;
  void* workspace; size_t ws_bytes;   /* optional: makes split_k deterministic (partial slabs + finishing pass) */
  float* colsum;   /* optional, TN + bf16 v2 kernel only: colsum[m] = sum_k A[k,m] (the bias gradient of a Linear) */
  int tile_rows;   /* 0 = library heuristic; 64 / 128 / 256 force the bf16 kernel's row tile (tuning sweeps) */
  int algo;        /* 0 = library heuristic; 2 = register-staged kernel; 1000 * wg_per_cu + 300 + 10 * (tile_rows / 64) + stages = persistent LDS-DMA NT kernel; 1000 * wg_per_cu + 400 + variant = 8-wave LDS-DMA NT kernel, needs K % 64 == 0 (tuning sweeps); 500 = the streaming thin-operand NT kernel (gemm5.hip: K = 96 / 192 / 384, N % 96 == 0, M % 32 == 0; 503 / 506: 96 / 192 columns per workgroup at K = 192) */
  int res_up[6];   /* {Ti, Hi, Wi, To, Ho, Wo}; all 0 = plain residual */
} csts_gemm_args;
int csts_gemm(const csts_gemm_args* args, hipStream_t stream);
size_t csts_gemm_splitk_workspace(int64_t M, int64_t N, int64_t K, int split_k);
/* Host-only queries of the ONE routing decision csts_gemm launches by (a forced args->algo included; a call csts_gemm would reject
   because its forced algo cannot run the problem returns -1 here too, with csts_last_error set).
   csts_gemm_plan: *nsplit = k-splits, and the kernel as a code in *v2 with its row tile in *tile_rows:
     -1 gemm_tiny_kernel (tile_rows 0) ; 0 gemm_kernel (fp32 / unaligned operands, tile_rows 128) ;
     1 gemm2_kernel<.., tile_rows / 64, 2> (register-staged 16-bit kernel) ; 30 + stages gemm3_kernel<tile_rows / 64, stages> (persistent
     LDS-DMA NT kernel) ; 400 + variant gemm4_kernel (8-wave LDS-DMA NT kernel, tile_rows 0) ; 500 gemm5_kernel (streaming thin-operand NT
     kernel, tile_rows 0). */
int csts_gemm_plan(const csts_gemm_args* args, int* v2, int* tile_rows, int* nsplit);
/* The same route by NAME, with every template argument, as rocprofv3 prints it (for attributing live timings); *nsplit = k-splits. */
int csts_gemm_kernel_name(const csts_gemm_args* a, char* buf, int buflen, int* nsplit);
int csts_gemm_v2_eligible(const csts_gemm_args* args);   /* 1 when the fast bf16 kernel (and fused colsum) applies */

/* Grouped weight gradients: every dW[M,N] = dY[tokens,M]^T X[tokens,N] of a backward pass (nn.Linear weight gradients of
 * attention.py:88-89, common.py:20-21 ...) as (tile, token-chunk) work items of ONE launch; items live in DEVICE memory.
 * A (dY) is bf16 or fp32 for the whole launch (a_f32), B (X) bf16, C fp32 (the gradient itself, or one chunk's partial slab
 * to be summed by csts_reduce_rows_batched); tile_rows (64 | 128, or 256 with bf16 dY) x 128 tiles, one height per launch.
 * colsum (optional): bias-gradient partial sum over the item's tokens for the tile's rows (written by n0 == 0 tiles). */
typedef struct {
  const void* A; const void* B; float* C; float* colsum;
  int64_t lda, ldb, ldc;
  int64_t kbeg, kend;
  int M, N, m0, n0;
} csts_wgrad_item;
int csts_wgrad_grouped(const csts_wgrad_item* device_items, int nitems, int a_f32, int tile_rows, hipStream_t stream);
/* the same items as 192 x 384 tiles on 8-wave workgroups (bf16 dY; M % 192 == 0 and N % 384 == 0 layers): half the operand
 * bytes per FLOP through the L2 -> CU path */
int csts_wgrad_grouped8(const csts_wgrad_item* device_items, int nitems, hipStream_t stream);
/* the same launch on at most max_wgs workgroups (a multiple of 8 below it, >= 8), each walking several items: the kernel's 144 KB of LDS
 * take a whole CU, so a launch of max_wgs < 256 workgroups leaves the other CUs to whatever runs beside it (round 5: the grouped weight
 * gradients of the 384- / 768-channel stages beside the memory-bound end of the backward pass).  max_wgs <= 0: one workgroup per item. */
int csts_wgrad_grouped8_limited(const csts_wgrad_item* device_items, int nitems, int max_wgs, hipStream_t stream);
/* the thin layers (M % 96 == 0, N % 96 == 0, bf16 dY, token ranges in multiples of 16) as 96 x 96 tiles, one item per WAVE: eight
 * consecutive slots of one XCD's list per 8-wave workgroup (nitems = 8 x the longest list, position slot * 8 + xcd, padding A == NULL);
 * every wave streams its token range through a private LDS-DMA ring -- no workgroup barrier (round 5).  Item fields as above except
 * M: the STAGE STEP -- M > 1: the item takes the 16-token stages kbeg, kbeg + 16 M, ... < kend (the M items of a tile interleave) */
int csts_wgrad_grouped5(const csts_wgrad_item* device_items, int nitems, hipStream_t stream);

/* ---- LayerNorm: nn.LayerNorm(C, eps=1e-6) block norms (attention.py:192,214) and nn.LayerNorm(hd, eps=1e-5)
 *      on pooled q/k/v (attention.py:108,112,116).  mean/rstd are fp32 [rows]; dgamma,dbeta one [2*C] buffer. */
int csts_layernorm_fwd(const void* x, int x_dt, const float* gamma, const float* beta, void* y, int y_dt, float* mean,
                       float* rstd, int64_t rows, int C, float eps, hipStream_t stream);
/* same, normalising x + addend (dtype of x) and writing that sum to sum_out: the decoder's skip `feat + en_feat`
 * (custom_multimodal_builder.py:467-479) folded into the next block's norm1 (attention.py:192,238) */
int csts_layernorm_fwd_add(const void* x, const void* addend, void* sum_out, int x_dt, const float* gamma, const float* beta,
                           void* y, int y_dt, float* mean, float* rstd, int64_t rows, int C, float eps, hipStream_t stream);
size_t csts_layernorm_bwd_workspace(int64_t rows, int C);
/* addend (optional, dtype of dx): dx = LN'(dy) + addend -- the residual-branch gradient of x + f(LN(x)) (attention.py:242,247)
 * folded in.  dx_bf16 (optional): a bf16 copy of dx for the GEMMs that consume it next (they round to bf16 while staging
 * anyway, so results are unchanged while they read half the bytes).  dgamma == dbeta == NULL defers the cross-workgroup second stage: workspace then holds
 * csts_layernorm_bwd_workspace(rows, C) / (2*C*4) partial rows of [2*C] for csts_reduce_rows(_batched). */
int csts_layernorm_bwd(const void* dy, int dy_dt, const void* x, int x_dt, const float* gamma, const float* mean,
                       const float* rstd, void* dx, int dx_dt, const void* addend, void* dx_bf16, float* dgamma,
                       float* dbeta, void* workspace, size_t ws_bytes, int64_t rows, int C, hipStream_t stream);
/* same with two extras.  dy2 (optional, dtype and shape of dy): the LayerNorm output had a second consumer (a block that
 * changes the channel count feeds norm2's output to fc1 AND to its skip projection, attention.py:243-246) -- the kernel reads
 * dy + dy2 instead of autograd adding the two first.  copy_row_scale (optional): the bf16 copy is multiplied by a per-sample
 * scale (row r: copy_row_scale[r / rows_per_scale]; dx itself is not scaled) -- the stochastic-depth factor of the residual
 * branch that consumes this gradient next (drop_path, common.py:46-59; x + drop_path(f(x)) at attention.py:242,247), which then
 * needs no pass of its own over dx. */
int csts_layernorm_bwd_ex(const void* dy, const void* dy2, int dy_dt, const void* x, int x_dt, const float* gamma, const float* mean,
                          const float* rstd, void* dx, int dx_dt, const void* addend, void* dx_bf16,
                          const float* copy_row_scale, int64_t rows_per_scale, float* dgamma, float* dbeta,
                          void* workspace, size_t ws_bytes, int64_t rows, int C, hipStream_t stream);
/* two stacked tensors of `rows` rows each (dy, x, dx, mean, rstd contiguous: [2][rows]...) with their own gammas in one
 * launch (norm_k and norm_v of one attention); dgb0/dgb1 = [2*C] dgamma|dbeta of each, or both NULL to defer the second
 * stage: workspace = 2 x csts_layernorm_bwd_workspace(rows, C), tensor i's partial rows at offset i * that size */
int csts_layernorm_bwd2(const void* dy, int dy_dt, const void* x, int x_dt, const float* gamma0, const float* gamma1,
                        const float* mean, const float* rstd, void* dx, int dx_dt, float* dgb0, float* dgb1,
                        void* workspace, size_t ws_bytes, int64_t rows, int C, hipStream_t stream);
int csts_reduce_rows(const float* ws, float* out, int64_t nrows, int64_t ncols, float scale, hipStream_t stream);
/* many deferred second stages (LayerNorm dgamma/dbeta, stencil dweight) in ONE launch; descriptors in DEVICE memory */
typedef struct { const float* ws; float* out; int64_t nrows; int64_t ncols; float scale; int pad_; } csts_reduce_desc;
int csts_reduce_rows_batched(const csts_reduce_desc* device_descs, int n, int64_t max_ncols, hipStream_t stream);
/* same contract for wide, shallow reductions (few rows, many columns): needs ncols % 4 == 0 and 16-byte aligned ws / out */
int csts_reduce_rows_wide(const csts_reduce_desc* device_descs, int n, int64_t max_ncols, hipStream_t stream);

/* ---- depthwise 3x3x3 token stencils: attention_pool's Conv3d (attention.py:11-49,104-116) and
 *      attention_upsample's ConvTranspose3d (attention.py:251-289,344-348).  "fine" is the larger grid.
 *      weight is the reference layout (hd, 1, 3, 3, 3) fp32, shared by all heads (channel c uses c % HD). */
typedef struct {
  int B, C, HD;
  int Tf, Hf, Wf, Tc, Hc, Wc;      /* coarse = floor((fine-1)/stride)+1 */
  int st, sh, sw;
  int64_t fine_batch_stride, fine_token_stride, coarse_batch_stride, coarse_token_stride;  /* elements */
} csts_dwconv_geom;
int csts_dwconv_strided(const csts_dwconv_geom* g, const void* fine, int fine_dt, const float* weight, void* coarse,
                        int coarse_dt, hipStream_t stream);     /* pool fwd ; upsample bwd-data */
int csts_dwconv_transposed(const csts_dwconv_geom* g, const void* coarse, int coarse_dt, const float* weight, void* fine,
                           int fine_dt, hipStream_t stream);    /* upsample fwd ; pool bwd-data */
size_t csts_dwconv_wgrad_workspace(const csts_dwconv_geom* g);
/* dweight NULL: second stage deferred (workspace = rows of [HD*27] partials, rows = workspace bytes / (HD*27*4)) */
int csts_dwconv_wgrad(const csts_dwconv_geom* g, const void* fine, int fine_dt, const void* coarse, int coarse_dt,
                      float* dweight, void* workspace, size_t ws_bytes, hipStream_t stream);

/* two tensors that share one geometry (the k and v pools of one attention) in one launch each; workspace of wgrad2 =
 * 2 x csts_dwconv_wgrad_workspace(g), slot i's partial rows at offset i * that size */
int csts_dwconv_transposed2(const csts_dwconv_geom* g, const void* const coarse[2], int coarse_dt, const float* const weight[2],
                            void* const fine[2], int fine_dt, hipStream_t stream);
int csts_dwconv_wgrad2(const csts_dwconv_geom* g, const void* const fine[2], int fine_dt, const void* const coarse[2],
                       int coarse_dt, float* const dweight[2], void* workspace, size_t ws_bytes, hipStream_t stream);
/* Grouped first stage: every stencil weight gradient of a backward pass (the q / k / v pools of all blocks, attention.py:104-116,
 * and the decoder's transposed convs, :344-348) in ONE launch instead of one ~24 us latency-bound launch each.  Item i is one
 * csts_dwconv_wgrad problem whose partial rows go to its own workspace (csts_dwconv_wgrad_grouped_workspace(&geom) bytes -- the
 * grouped launch cuts a tensor into fewer, longer token chunks than the single one; rows = bytes / (HD*27*4)); the second stage
 * (the row sums) is the caller's, exactly as with dweight NULL above.  _plan runs on the
 * host: it validates the items and writes the DEVICE TABLE IMAGE (nitems * CSTS_DWCONV_WGRAD_TABLE_ENTRY bytes, items
 * re-ordered longest workgroups first) into table_host and the grid size into *nblocks; the caller copies the image to device
 * memory in stream order and passes that address to csts_dwconv_wgrad_grouped.  All items of a call share dtype dt. */
typedef struct {
  csts_dwconv_geom geom;
  const void* fine; const void* coarse;
  void* workspace;
} csts_dwconv_wgrad_item;
#define CSTS_DWCONV_WGRAD_TABLE_ENTRY 128
size_t csts_dwconv_wgrad_grouped_workspace(const csts_dwconv_geom* g);
int csts_dwconv_wgrad_grouped_plan(const csts_dwconv_wgrad_item* items, int nitems, void* table_host, size_t table_bytes, int* nblocks);
int csts_dwconv_wgrad_grouped(const void* table_dev, int nitems, int nblocks, int dt, hipStream_t stream);

/* attention_pool fused (attention.py:11-49): depthwise Conv3d k=3 p=1 stride s of the head-split q/k/v slot + LayerNorm(hd)
 * of the pooled rows, for nslots (1 or 2) tensors sharing the geometry.  conv_out = pre-LN pooled tensor (needed by
 * backward), y = normalised tensor, mean/rstd fp32 [B * N_coarse * heads]; all tensors of dtype dt. */
typedef struct {
  csts_dwconv_geom geom;        /* coarse strides describe conv_out AND y */
  int nslots;
  const void* fine[2];
  const float* weight[2]; const float* gamma[2]; const float* beta[2];
  void* conv_out[2]; void* y[2];
  float* mean[2]; float* rstd[2];
  int dt; float eps;
} csts_pool_ln_args;
int csts_pool_ln_fwd(const csts_pool_ln_args* args, hipStream_t stream);

/* ---- residual-path resampling: MaxPool3d skip (attention.py:193-195,234-236,240), nn.Upsample trilinear skip
 *      (attention.py:463-467,471) and F.interpolate of the patch feature (custom_multimodal_builder.py:479).
 *      maxpool: kernel = stride+1 where stride>1 else 1, padding = kernel/2.  trilinear: out = in*stride,
 *      align_corners=False; optional fused `addend` (same shape as y). */
typedef struct {
  int B, C;
  int Ti, Hi, Wi, To, Ho, Wo;
  int st, sh, sw;
} csts_pool_geom;
int csts_maxpool_fwd(const csts_pool_geom* g, const void* x, int dt, void* y, uint8_t* argmax, hipStream_t stream);
int csts_maxpool_bwd(const csts_pool_geom* g, const void* dy, int dt, const uint8_t* argmax, void* dx, hipStream_t stream);
int csts_trilinear_fwd(const csts_pool_geom* g, const void* x, int x_dt, const void* addend, int addend_dt, void* y,
                       int y_dt, hipStream_t stream);
int csts_trilinear_bwd(const csts_pool_geom* g, const void* dy, int dy_dt, void* dx, int dx_dt, hipStream_t stream);

/* ---- fused attention core softmax(q k^T scale [same-frame mask]) v  (attention.py:154-158,384-388;
 *      av_attention.py:137-141,334-350).  q/k/v/o are (B, N, H, hd) views given by element strides
 *      {batch, token, head}; hd contiguous.  LSE/delta are fp32 (B, H, Nq); LSE is in the log2 domain.
 *      delta is SCRATCH of csts_attn_bwd, not a result: the two-kernel backward writes rowsum(dO * O) into it (the dQ kernel
 *      leaves it for the dK/dV kernel), the one-pass backward (16-bit, head_dim 96, no mask, Nk <= 128, Nq >= 1024) keeps the
 *      sums in LDS and leaves the buffer untouched.  It must be given either way; read nothing back from it.
 *      Every argument, the query-split plan and the workspace size are checked before the first launch: a call that returns
 *      non-zero has written nothing.  csts_attn_bwd_workspace returns 0 for a problem the calls refuse (a non-positive
 *      B / H / Nq / Nk, a head_dim other than 96 / 192, NULL).
 *      Launch, workspace and query share ONE route: which forward / dQ / dK/dV kernel runs and with how many query splits is
 *      decided once, from dtype, head_dim, B, H, Nq, Nk, mask_mode and the CSTS_ATTN_* switches.  csts_attn_route (host-only:
 *      it reads no operand pointer and no stride, launches nothing, needs no device) writes that route to buf as
 *      "fwd;dq;dkv;reduce" -- kernel names as the source spells them, without spaces; dq is empty on the one-pass path, where dkv
 *      is attn_bwd_fused_kernel; reduce is attn_dkv_reduce_kernel or empty -- and returns -1 for the problems
 *      csts_attn_bwd_workspace returns 0 for. */
typedef struct {
  const void* Q; const void* K; const void* V; void* O; float* LSE;
  const void* dO; float* delta; void* dQ; void* dK; void* dV;
  int dtype, B, H, Nq, Nk, head_dim;
  int64_t q_strides[3], k_strides[3], v_strides[3], o_strides[3];
  int64_t do_strides[3], dq_strides[3], dk_strides[3], dv_strides[3];
  float scale;
  int mask_mode, mask_T, mask_HW;
} csts_attn_args;
int csts_attn_fwd(const csts_attn_args* a, hipStream_t stream);
size_t csts_attn_bwd_workspace(const csts_attn_args* a);
int csts_attn_bwd(const csts_attn_args* a, void* workspace, size_t ws_bytes, hipStream_t stream);
int csts_attn_probs(const csts_attn_args* a, float* probs /* (B,H,Nq,Nk) */, hipStream_t stream);
int csts_attn_route(const csts_attn_args* a, char* buf, int buflen, int* nsplit, int* q_chunk);

/* ---- patch embedding: Conv3d k(3,7,7) s(2,4,4) p(1,3,3) + flatten/transpose (stem_helper.py:27-38) as
 *      im2col + csts_gemm; separable positional embedding (custom_multimodal_builder.py:362-370). */
typedef struct {
  int B, Cin, T, H, W;
  int kernel[3], stride[3], padding[3];
  int To, Ho, Wo;
  int Kpad;
} csts_im2col_geom;
int csts_im2col(const csts_im2col_geom* g, const void* x, int x_dt, void* col, int col_dt, hipStream_t stream);
int csts_posembed_build(const float* spatial, const float* temporal, float* pos, int T, int HW, int C, hipStream_t stream);

/* ---- layout / reductions */
int csts_transpose_batched(const void* in, int in_dt, void* out, int out_dt, int64_t batch, int R, int Cc,
                           hipStream_t stream);   /* token fold for the (1,8,8) fusion convs */
/* Many bf16 matrices (R x C, both % 8 == 0, 16-byte aligned) transposed in one launch: one 64 x 64 tile per entry of a DEVICE
 * table.  Keeps the [in][out] twins of the Linear weights' bf16 shadows, so that the data gradient dX = dY W runs as an
 * NT GEMM (k-contiguous operands) like the forward (nn.Linear backward: attention.py:130,159; common.py:27-33). */
typedef struct { const void* src; void* dst; int R, C, r0, c0; } csts_transpose_tile;
int csts_transpose_multi(const csts_transpose_tile* device_tiles, int ntiles, hipStream_t stream);
size_t csts_colsum_workspace(int64_t batch, int64_t M, int64_t N);
int csts_colsum(const void* X, int dt, const float* row_weight, float* out, int64_t batch, int64_t M, int64_t N,
                void* workspace, size_t ws_bytes, hipStream_t stream);   /* bias / pos-embed / classifier grads */
int csts_axpby(const void* a, int a_dt, const void* b, int b_dt, void* out, int out_dt, int64_t n, float alpha, float beta,
               hipStream_t stream);

int csts_add2(const void* a, int a_dt, const void* b, int b_dt, float* out, void* out_bf16, int64_t n,
              hipStream_t stream);
/* same; the bf16 copy (only the copy) is multiplied by copy_scale[i / elems_per_scale]: the per-sample stochastic-depth scale of
 * the residual branch that consumes this gradient next (see csts_layernorm_bwd_ex) */
int csts_add2_scaled_copy(const void* a, int a_dt, const void* b, int b_dt, float* out, void* out_bf16, const float* copy_scale,
                          int64_t elems_per_scale, int64_t n, hipStream_t stream);   /* out = a + b (fp32) and optionally its bf16 copy: the two gradients of an encoder
                                      * feature that the decoder skip re-uses (custom_multimodal_builder.py:467-479) */

/* ---- Rows a strided K/V pool reads.  The K and V pools are 3x3x3 depthwise convs with stride (1, s, s), padding 1
 *      (attention.py:11-49,104-116): output cell o of an axis reads fine cells o*s - 1, o*s, o*s + 1, so for s >= 3 only
 *      (3/s)^2 of the token rows of k|v are ever consumed (14 % at s = 8, 3.5 % at s = 16).  Those rows form a COMPACT grid
 *      (T, Hc, Wc): compact cell ch <-> fine cell ((ch + 1) / 3) * s + (ch + 1) % 3 - 1, Hc = 3 * ceil(H / s) - 1 (minus one
 *      more when the last cell would fall outside H), and the pool over it is the SAME conv with stride (1, 3, 3): the k|v
 *      halves of the qkv Linear are computed for these rows only (rows are independent: identical values).
 *      gather: dst[b,t,ch,cw,:] = src[b,t,h,w,:]; scatter_add (data gradient back to all rows): dst[b,t,h,w,:] += src[b,t,ch,cw,:]. */
typedef struct { int B, C, T, H, W, sh, sw, Hc, Wc; } csts_kv_rows_geom;
int csts_rows_gather(const csts_kv_rows_geom* g, const void* src, int dt, void* dst, hipStream_t stream);
int csts_rows_scatter_add(const csts_kv_rows_geom* g, const void* src, int src_dt, void* dst, int dst_dt, hipStream_t stream);

/* ---- Token-axis concatenation / split of (B, N, C) tensors in ONE launch (round 5): the fusion head joins the visual tokens with
 *      the pooled audio tokens (custom_multimodal_builder.py:421-423 torch.cat(dim=1), :448) and cuts the fused sequences apart again
 *      (:432,454-455 x[:, :N], x[:, N:]); through torch those are cat / slice / copy / fill / add nodes in both directions.
 *      Segment i copies n rows of C contiguous elements per batch element: dst[b * dst_bs + dst_off + r * C + c] =
 *      src[b * src_bs + src_off + r * C + c] (offsets and batch strides in elements; all multiples of 16 bytes).  nseg <= 4. */
typedef struct { const void* src; void* dst; int64_t src_bs, dst_bs, src_off, dst_off; int n; int pad_; } csts_token_segment;
int csts_copy_token_segments(const csts_token_segment* segs, int nseg, int B, int C, int dt, hipStream_t stream);

int csts_scale_rows(const void* x, int x_dt, const float* row_scale, int64_t rows_per_scale, void* out, int out_dt,
                    int64_t M, int64_t N, hipStream_t stream);   /* drop-path backward (common.py:46-59) */

/* ---- element dropout, nn.Dropout(MVIT.DROPOUT_RATE) in train mode (csts_amd/csrc/dropout.hip): pos_drop
 *      (custom_multimodal_builder.py:375-377), proj_drop (attention.py:159-161,390; av_attention.py:148,353), Mlp.drop on the
 *      GELU output and on fc2's output (common.py:26-34).
 *      Mask function: a pure function of (key, site, e, thr), whatever the grid, stream or tile shape.  key: one 64-bit word per
 *      forward, in DEVICE memory (never read by the host: no sync, graph-capturable); e: the element's flat row-major index in
 *      the site's logical (rows, cols) tensor.  Philox4x32-10 (Salmon et al., SC'11; multipliers 0xD2511F53 / 0xCD9E8D57, key
 *      increments 0x9E3779B9 / 0xBB67AE85) with key (lo32(key), hi32(key)) on the counter (lo32(e >> 2), hi32(e >> 2), site, 0);
 *      element e takes output word e & 3 and is DROPPED iff word < thr, thr = floor(p * 2^32) (computed by the caller in double;
 *      an integer compare, no float in the decision).  A kept element is multiplied by scale = 1.0f / (1.0f - p) (fp32).
 *      Sites: 0 video pos_drop, 1 audio pos_drop; 2 + 3*i + {0 attention proj, 1 MLP hidden, 2 MLP out} for the i-th Block in
 *      module registration order: blocks.0..15, blocks_audio.0..3, temporal_fusion, spatial_fusion, decode_block1..4.
 *      dropout_fwd: y = residual + row_scale[r / rows_per_scale] * keep * scale * z (residual / row_scale optional, both NULL =
 *                   the in-place form; y == z allowed), one dtype for z, residual and y.
 *      dropout_bwd: out = dy * row_scale[r / rows_per_scale] * keep * scale (row_scale optional), into fp32 or the 16-bit type --
 *                   the masked form of csts_scale_rows; in place when out == dy (same dtype).
 *      All tensors contiguous and 16-byte aligned.  dropout_mask: out[e] = 1 if dropped (n elements, out 8-byte aligned).
 *      dropout_mask_host: the same function on the CPU (HOST memory) for elements first .. first + count - 1. */
int csts_dropout_fwd(const void* z, const void* residual, const float* row_scale, int64_t rows_per_scale, void* y, int dt,
                     const uint64_t* key, uint32_t site, uint32_t thr, float scale, int64_t rows, int64_t cols, hipStream_t stream);
int csts_dropout_bwd(const void* dy, int dy_dt, const float* row_scale, int64_t rows_per_scale, void* out, int out_dt,
                     const uint64_t* key, uint32_t site, uint32_t thr, float scale, int64_t rows, int64_t cols, hipStream_t stream);
int csts_dropout_mask(const uint64_t* key, uint32_t site, uint32_t thr, uint8_t* out, int64_t n, hipStream_t stream);
int csts_dropout_mask_host(uint32_t key0, uint32_t key1, uint32_t site, uint32_t thr, uint64_t first, int64_t count, uint8_t* out);

int csts_rowdot2(const void* a, int a_dt, const void* b, int b_dt, float* out, int64_t M, int C,
                 hipStream_t stream);   /* out[m] = <a[m,:], b[m,:]>: gradient of a per-row weight */

/* ---- audio -> pixel attention map of the spatial fusion block (MVIT.SPATIAL_AUDIO_ATTN: av_attention.py:356-370
 *      min-max-rescaled probabilities of audio token t over the HW video tokens of frame t, per head; averaged over the
 *      heads into the per-token weight of custom_multimodal_builder.py:438-440).  qkv = the block's (B, T*HW + T, 3C) QKV
 *      projection; audio_attn (optional) = (B, H, T, HW) per-head maps; wmap = (B, T*HW).  The backward writes
 *      d(q of the audio tokens) and d(k) into a ZERO-INITIALISED buffer shaped like qkv. */
int csts_audio_attn_fwd(const void* qkv, int dt, float* audio_attn, float* wmap, int B, int T, int HW, int C, int H,
                        float scale, hipStream_t stream);
int csts_audio_attn_bwd(const void* qkv, int dt, const float* d_wmap, void* dqkv, int B, int T, int HW, int C, int H,
                        float scale, hipStream_t stream);

/* ---- fusion glue (custom_multimodal_builder.py:454-461 re-weighting, :493-494 token mean) */
int csts_reweight_fwd(const float* x, const float* w, float* y, int64_t BT, int HW, int C, hipStream_t stream);
int csts_reweight_bwd(const float* x, const float* w, const float* dy, float* dx, float* dw, int64_t BT, int HW, int C,
                      hipStream_t stream);
int csts_token_mean_fwd(const float* x, float* out, int64_t B, int N, int C, hipStream_t stream);
int csts_token_mean_bwd(const float* dout, float* dx, int64_t B, int N, int C, hipStream_t stream);

/* ---- head + losses: classifier Conv3d(96,1,1) (custom_multimodal_builder.py:301,481), frame_softmax
 *      (slowfast/utils/utils.py:5-12), KLDiv (slowfast/models/losses.py:59-82), sim_matrix
 *      (slowfast/utils/utils.py:15-24), EgoNCE (slowfast/models/losses.py:157-170). */
int csts_rowdot_fwd(const void* x, int x_dt, const float* w, const float* bias, float* out, int64_t M, int C,
                    hipStream_t stream);
int csts_rowdot_dx(const float* dout, const float* w, void* dx, int dx_dt, int64_t M, int C, hipStream_t stream);
int csts_softmax_fwd(const float* x, float* p, int64_t rows, int n, float temperature, hipStream_t stream);
int csts_softmax_bwd(const float* x, const float* dp, float* dx, int64_t rows, int n, float temperature, hipStream_t stream);
int csts_kldiv_fwd(const float* p, const float* q, float* loss, float* rowloss_ws, int64_t rows, int n, float scale,
                   hipStream_t stream);
int csts_kldiv_bwd(const float* p, const float* q, const float* grad_out, float* dp, int64_t rows, int n, float scale,
                   hipStream_t stream);
int csts_rownorm_fwd(const float* a, float* a_normed, float* norms, int64_t rows, int D, float eps, hipStream_t stream);
int csts_rownorm_bwd(const float* a, const float* norms, const float* d_normed, float* da, int64_t rows, int D, float eps,
                     hipStream_t stream);
int csts_egonce_fwd(const float* sim, float* loss, float* lse_row, float* lse_col, int n, float temperature,
                    hipStream_t stream);
int csts_egonce_bwd(const float* sim, const float* lse_row, const float* lse_col, const float* grad_out, float* dsim, int n,
                    float temperature, hipStream_t stream);

/* ---- optimizer step ("next" row): clip_grad_norm_(params, max_norm) (tools/train_avgaze_net.py:105-106)
 *      + torch.optim.AdamW (slowfast/models/optimizer.py:85-93; eps 1e-8, decoupled weight decay, per-tensor decay so that
 *      1-D parameters and biases get 0, optimizer.py:48-50,98-104) over the whole parameter set in three launches, and the
 *      refresh of the bf16 shadow weights the GEMMs read.  All pointers are DEVICE memory.  The parameter set is described
 *      as chunks of at most chunk_elems elements that never straddle a tensor (chunk -> tensor id + element offset).
 *      state = {step (incremented by the call), total gradient L2 norm (out), clip coefficient (out)} fp32[3];
 *      lr is read from device memory, so a captured graph follows the schedule.  grads[i] == NULL skips tensor i. */
typedef struct {
  void* p; void* m; void* v;   /* fp32 parameter, exp_avg, exp_avg_sq */
  void* w16;                   /* optional bf16 shadow of p (NULL: none) */
  int64_t n;
  float weight_decay; int pad_;
} csts_opt_tensor;
typedef struct {
  const int32_t* chunk_tensor; const int64_t* chunk_off; int nchunks; int chunk_elems;
  const csts_opt_tensor* tensors; const void* const* grads; int ntensors;
  float* partial;              /* fp32[nchunks] workspace */
  float* state;                /* fp32[4]: step count, total gradient norm, clip coefficient (x 1 / loss scale), skipped (0 / 1) */
  const float* lr;
  float beta1, beta2, eps, max_grad_norm;   /* max_grad_norm <= 0: no clipping */
  int grad_dt;                 /* dtype of EVERY gradient: CSTS_F32, or CSTS_BF16 = the library's 16-bit type (data-parallel buckets that
                                * travelled in 16 bits: read once, accumulated in fp32 here) */
  /* optional dynamic loss scaling, torch.cuda.amp.GradScaler (tools/train_avgaze_net.py:99-109,277): scaler = fp32[2] device
   * {scale, growth tracker}.  Gradients are the gradients of scale * loss: the norm / clip / update use g / scale
   * (scaler.unscale_); a non-finite norm SKIPS the step (no parameter, moment or step-count change; state[3] = 1) and multiplies
   * the scale by backoff; growth_interval consecutive good steps multiply it by growth (scaler.update()). */
  float* scaler; float growth, backoff; int growth_interval;
  /* optional: extra_sq[0 .. n_extra_sq) device floats added to the sum of squared gradients before the norm is taken -- the
   * squared norms of gradients that are never materialised (csts_adamw_factored); they are in the same (loss-scaled) units as
   * the gradients */
  const float* extra_sq; int n_extra_sq;
} csts_opt_args;
int csts_adamw_step(const csts_opt_args* args, hipStream_t stream);

/* Update rule of the optimizer step (SOLVER.OPTIMIZING_METHOD, slowfast/models/optimizer.py:82-108) and the value clip
 * (SOLVER.CLIP_GRAD_VAL, tools/train_avgaze_net.py:103-104).  g below is the unscaled gradient, clipped; wd the tensor's weight decay.
 *   CSTS_OPT_ADAMW  torch.optim.AdamW: what csts_adamw_step computes (bit-identical with clip_value <= 0).
 *   CSTS_OPT_ADAM   torch.optim.Adam (amsgrad off): g += wd p, then the moments, bias corrections and step of AdamW, no decoupled decay.
 *   CSTS_OPT_SGD    torch.optim.SGD: d = g + wd p; with momentum != 0, buf = d on the buffer's first step, else
 *                   buf = momentum buf + (1 - dampening) d, and d = d + momentum buf (nesterov) or buf; p -= lr d.  m is the momentum
 *                   buffer, v unused; with momentum == 0 m and v are unused.
 * m and v may be NULL where the rule does not use them (csts_opt_factored_step refuses NULL where it does; csts_opt_step's table is
 * device memory: a tensor whose required buffer is NULL is left untouched).  clip_value > 0: every unscaled gradient element is
 * clamped to [-clip_value, clip_value] before weight decay (clip_grad_value_ after scaler.unscale_); it excludes max_grad_norm > 0.
 * The norm pass still runs (the loss scaler's non-finite check, state[1] for logging); the clip coefficient is then 1 / scale.
 * buf_step (SGD with momentum only, else ignored): fp32[ntensors] device memory, per tensor (index of csts_opt_args.tensors, or
 * csts_opt_factored.tensor) the step count (state[0]) at which its momentum buffer was initialised, 0 = never.  The update writes it;
 * set it to a value no step count takes (e.g. -1) when a buffer is loaded from a checkpoint.  A step the loss scaler skips leaves it
 * alone, so a captured graph replays the "first step" correctly.  csts_opt_step: three launches for every rule (like csts_adamw_step);
 * csts_opt_factored_step: csts_adamw_factored with a rule. */
enum { CSTS_OPT_ADAMW = 0, CSTS_OPT_ADAM = 1, CSTS_OPT_SGD = 2 };
typedef struct {
  int kind;
  float momentum, dampening; int nesterov;     /* CSTS_OPT_SGD only (0 for the other rules); nesterov needs momentum > 0, dampening 0 */
  float clip_value;                            /* <= 0: off */
  int pad_;
  float* buf_step;
} csts_opt_rule;
int csts_opt_step(const csts_opt_args* args, const csts_opt_rule* rule, hipStream_t stream);

/* Factored AdamW: the weight gradient of a fusion conv (custom_multimodal_builder.py:227-229) is dW[N][K] = dY[T][N]^T A[T][K]
 * with T = B * T' token rows (32 at b = 4, 16 frames) for N x K = 768 x 49152 -- a rank-T update.  Instead of writing dW to
 * memory (151 MB, read twice by the clip norm and the update) the optimizer forms g = dY^T A ON THE FLY, in fp32, inside the
 * update of p / m / v (same AdamW arithmetic, same clip coefficient and loss-scale handling as csts_adamw_step, whose `state`
 * it reads -- call it after csts_adamw_step of the same iteration).  csts_factored_sqnorm gives the squared Frobenius norm of
 * every item's never-materialised gradient for that step's clip norm (csts_opt_args.extra_sq) as
 * sum_{t,t'} (dY dY^T)[t,t'] (A A^T)[t,t'], from T x T Gram matrices.  dy fp32 [T][N]; a [T][K] in a_dt; T <= 64, K % 256 == 0,
 * N % 16 == 0.  workspace: csts_factored_sqnorm_workspace(items) bytes.  Round 5: csts_adamw_factored takes T <= 256 when every
 * item's `a` is in the library's 16-bit type (the MFMA form of the update has no T x K tile in LDS: it loops over T) -- the
 * data-parallel chain's W * B * T' gathered rows at eight ranks; for T > 64 the caller forms the two Gram matrices with csts_gemm
 * (A A^T and dY dY^T, split-K) and their inner product with csts_rowdot2 + csts_reduce_rows (csts_amd/optim.py). */
typedef struct {
  float* p; float* m; float* v; void* w16;
  const float* dy; const void* a; int a_dt;
  int N, K, T; float weight_decay;
  int tensor;                  /* index into csts_opt_rule.buf_step (SGD with momentum; ignored otherwise) */
} csts_opt_factored;
size_t csts_factored_sqnorm_workspace(const csts_opt_factored* items, int nitems);
int csts_factored_sqnorm(const csts_opt_factored* items, int nitems, float* out_sq, void* workspace, size_t ws_bytes, hipStream_t stream);
int csts_adamw_factored(const csts_opt_factored* items, int nitems, const float* state, const float* lr, float beta1, float beta2,
                        float eps, hipStream_t stream);
int csts_opt_factored_step(const csts_opt_factored* items, int nitems, const csts_opt_rule* rule, const float* state, const float* lr,
                           float beta1, float beta2, float eps, hipStream_t stream);

/* ---- evaluation metric ("next" row): metrics.adaptive_f1 (slowfast/utils/metrics.py:9-74) with the
 *      per-frame min-max rescale of its callers (tools/test_avgaze_net.py:66-68, tools/train_avgaze_net.py:125-127) folded
 *      in (rescale != 0).  preds, labels_hm: fp32 [nframes][hw]; tracked[f] != 0 marks the fixation frames that count
 *      (metrics.py:64-65); thresholds fp32 [nthr] (nthr <= 64).  out = {f1, recall, precision, index of the best threshold}. */
size_t csts_adaptive_f1_workspace(int64_t nframes, int nthr);
int csts_adaptive_f1(const float* preds, const float* labels_hm, const uint8_t* tracked, const float* thresholds, int nthr,
                     int64_t nframes, int hw, int rescale, float* out, void* workspace, size_t ws_bytes, hipStream_t stream);

/* ---- gaze meters: TrainGazeMeter / ValGazeMeter / TestGazeMeter (slowfast/utils/meters.py:19-146,200-475) as running
 *      statistics in ONE caller-owned device buffer, so the metric can live inside a captured training step.
 *      f1_counts: the count launch of csts_adaptive_f1 alone.  counts[f] = {tp[nthr], fg_preds[nthr], fg_labels} (int32) of frame
 *        f; these integers are all the metric needs of a frame, so ranks exchange them instead of the predictions.
 *      gaze_meter_update: one workgroup.  frame_types[f * type_stride] (fp64, 8-byte aligned) is the gaze type of frame f: pass
 *        &labels[0][2] and the row length of the (nframes, L) label matrix.  The kernel
 *        1. forms recall / precision / f1 per threshold over the frames with type == fixation_type and picks the first
 *           maximum, with the fp32 arithmetic of csts_adaptive_f1 (no such frame: NaN, as torch.mean of an empty selection);
 *        2. adds to the data-set sums, per threshold, sum tp / (fg_labels + 1e-6) and sum tp / (fg_preds + 1e-6) in fp64 and
 *           the number of tracked frames in int64: sufficient statistics of TestGazeMeter.finalize_metrics (meters.py:132-146),
 *           which keeps every prediction and calls adaptive_f1 once;
 *        3. adds recall w, precision w, w to the epoch totals (fp64); w = mb_size if mb_size >= 0 (TrainGazeMeter, meters.py:
 *           272-280: batch size x ranks), otherwise the number of frames with type == weight_type.  ValGazeMeter and
 *           TestGazeMeter count labels[:, 2] == 1 (meters.py:87-88,409-410) although adaptive_f1 tracks type 0 on every data set
 *           but egteagaze; the reference is followed literally, so their callers pass weight_type 1;
 *        4. writes {f1, recall, precision, threshold index} of this batch into slot (iterations % window) of a ring and
 *           increments the iteration counter, which lives in the buffer: a replayed graph needs no changed argument.
 *        No allocation, no synchronisation, no host read.
 *      state (8-byte aligned, gaze_meter_state_bytes(nthr, window) bytes, zero = empty; gaze_meter_reset zeroes it):
 *        int64 iterations, tracked frames | fp64 sum recall w, sum precision w, sum w | fp64 recall sums[nthr], precision
 *        sums[nthr] | fp32 ring[window][4].
 *      gaze_meter_update_host: the same rule (the same function) on HOST memory. */
int csts_f1_counts(const float* preds, const float* labels_hm, const float* thresholds, int nthr, int64_t nframes, int hw, int rescale,
                   int* counts, hipStream_t stream);
size_t csts_gaze_meter_state_bytes(int nthr, int window);
int csts_gaze_meter_reset(void* state, int nthr, int window, hipStream_t stream);
int csts_gaze_meter_update(const int* counts, const double* frame_types, int64_t type_stride, int64_t nframes, int nthr,
                           int fixation_type, int weight_type, int64_t mb_size, int window, void* state, hipStream_t stream);
int csts_gaze_meter_update_host(const int* counts, const double* frame_types, int64_t type_stride, int64_t nframes, int nthr,
                                int fixation_type, int weight_type, int64_t mb_size, int window, void* state);

/* ---- input pipeline on the device ("next" row): what the reference does on the CPU just before the
 *      model is called.  frames_normalize: uint8 (B, T*H*W, C) -> fp32 (B, C, T*H*W), (x/255 - mean)/std
 *      (slowfast/datasets/utils.py:290-307, ego4d_avgaze_forecast.py:294-296).  stft_logpower: fp32 waveform (B, n) ->
 *      log(|STFT|^2 + eps) (B, n_fft/2+1, csts_stft_frames(n, n_fft, hop)), librosa.stft semantics (center, zero padding,
 *      periodic Hann of win samples centred in n_fft; data/preprocess.py:276-290).  audio_windows: (B, 1, T, nbins, width)
 *      windows of the spectrogram centred on centers[b][t] (ego4d_avgaze_forecast.py:214-219).  gaze_heatmaps: labels
 *      (nframes, label_stride) with x, y in [0,1] -> (nframes, H, W) OpenCV-Gaussian maps normalised to sum 1
 *      (ego4d_avgaze_forecast.py:318-326,404-422). */
int csts_frames_normalize(const uint8_t* frames_thwc, float* out_cthw, int B, int64_t thw, int C, const float mean[3],
                          const float std[3], hipStream_t stream);
int csts_stft_frames(int n, int n_fft, int hop);
int csts_stft_logpower(const float* wav, float* spec, int B, int n, int n_fft, int hop, int win, float eps, hipStream_t stream);
int csts_audio_windows(const float* spec, const int* centers, float* out, int B, int T, int nbins, int cols, int width,
                       hipStream_t stream);
int csts_gaze_heatmaps(const float* labels, int label_stride, float* heatmaps, int64_t nframes, int H, int W, int ksize,
                       hipStream_t stream);

/* ---- spatial sampling on the device (csts_amd/csrc/spatial.hip): slowfast/datasets/utils.py::spatial_sampling(frames,
 *      gaze_loc=label, ...) of the reference (ego4d_avgaze_forecast.py:302-311, aria_avgaze_forecast.py): short-side scale
 *      jitter, gaze-aware crop and horizontal flip in train mode (spatial_idx -1, transform.py:43-97,155-197,235-262), a
 *      short-side resize to S and a uniform crop in test mode (spatial_idx 0/1/2, transform.py:327-387).
 *      Per clip: frames (T, H, W, 3) uint8 channels-last, labels (T, L) fp64 with x, y in columns 0, 1 (L >= 2, T <= 64); every
 *      clip of a call has one H, W.  Rule (fp64, no contraction; u0..u3 in [0, 1)):
 *        size = train ? rint(min + (max - min) u0)  [inv_uniform: rint(1 / (1/max + (1/min - 1/max) u0))]  : S   (half to even)
 *        no resize if the short side == size, else short -> size, long -> floor(long / short * size)   => new h, new w
 *        train, new h == new w == S: offsets 0, labels returned untouched (not clipped).
 *        train otherwise, per axis of extent E (x: new w, u1; y: new h, u2): E == S -> 0; else g = sort(label * E),
 *          low = max(0, max(g) - S), high = min(E - S, min(g)); while low > high drop g's first element if len(g) is even,
 *          its last if odd; offset = int(low) if low == high else int(low + (high - low) u).  (Where the reference would
 *          empty g -- one point left outside [0, E] -- the offset is min(E - S, low).)
 *        test: offsets ceil((E - S) / 2); along the long axis (y if new h > new w, else x) idx 0 -> 0, idx 2 -> E - S.
 *        labels (unless untouched) = clip((label * E - offset) / S, 0, 1) in columns 0, 1; columns >= 2 copied.
 *        flip = train && random_flip && u3 < 0.5: label x -> 1 - x, pixels mirrored in x.
 *      Variates: u[b][0..3] = Philox4x32-10 with key (lo32(key), hi32(key)) on the counters (lo32(b), hi32(b), 0x53504154, j),
 *      j = 0 gives u0, u1 and j = 1 gives u2, u3, from the word pairs (w0, w1) and (w2, w3) as ((a >> 5) * 2^26 + (b >> 6)) * 2^-53.
 *      key: one 64-bit word in DEVICE memory (no host sync, graph-capturable); unused (may be NULL) in test mode.
 *      Train mode needs S <= min <= max; min / max are unused in test mode.
 *      spatial_params: labels (B, T, L) -> params int32 [B][5] = {new h, new w, y0, x0, flip}, labels_out (B, T, L) fp64.
 *      spatial_sample: frames (B, T, H, W, 3) uint8 + params -> fp32 (B, 3, T, S, S),
 *        out[b][c][t][i][j] = (bilerp(y0 + i, x0 + j') / 255 - mean[c]) * (1 / std[c]), j' = flip ? S - 1 - j : j; bilerp =
 *        F.interpolate(bilinear, align_corners=False, no antialias) of the clip to (new h, new w): scale = in / out (fp32),
 *        src = max((dst + 0.5) scale - 0.5, 0), i0 = min(floor(src), in - 1), i1 = min(i0 + 1, in - 1), lambda = src - i0.
 *        Unresized clips equal frames_normalize bit for bit.  Params outside the rule's range give a NaN clip.  W <= 6000,
 *        frames and out 16-byte aligned.
 *      clip_sample: spatial_sample with an index table in front of it, for clips that are windows of ONE resident video
 *        video_nhwc (N, H, W, 3) uint8, N >= 1: out[b][c][t] is what spatial_sample writes for the frame
 *        video[min(max(frames_idx[b][t], 0), N - 1)] under params[b] (the clamp of temporal_sampling, decoder.py:26-27), bit
 *        for bit the result of gathering the frames into (B, T, H, W, 3) first.  frames_idx int32 [B][T] is read on the DEVICE
 *        when the kernel runs (no host sync, graph-capturable; rewriting the table between replays resamples).  A frame starts
 *        at byte idx * H * W * 3, at any alignment; only video and out must be 16-byte aligned.  T <= 64, W <= 6000.
 *      spatial_rule_host: the rule on HOST memory from explicit variates uniforms[B][4] (NULL allowed in test mode).
 *      spatial_uniforms_host: u[i][0..3] of clips first .. first + count - 1 (HOST memory). */
int csts_spatial_params(const uint64_t* key, const double* labels, int B, int T, int L, int H, int W, int S, int min_scale,
                        int max_scale, int spatial_idx, int random_flip, int inv_uniform, int* params, double* labels_out,
                        hipStream_t stream);
int csts_spatial_sample(const uint8_t* frames_thwc, const int* params, float* out, int B, int T, int H, int W, int S,
                        const float mean[3], const float std[3], hipStream_t stream);
int csts_clip_sample(const uint8_t* video_nhwc, int64_t N, const int* frames_idx, const int* params, float* out, int B, int T,
                     int H, int W, int S, const float mean[3], const float std[3], hipStream_t stream);
int csts_spatial_rule_host(const double* labels, int B, int T, int L, int H, int W, int S, int min_scale, int max_scale,
                           int spatial_idx, int random_flip, int inv_uniform, const double* uniforms, int* params,
                           double* labels_out);
int csts_spatial_uniforms_host(uint32_t key0, uint32_t key1, uint64_t first, int64_t count, double* out);

/* ---- batch assembly from many recordings (csts_amd/csrc/batch.hip, csts_amd/datasets.py): the clips of one batch come from B
 *      different recordings, possibly of B frame sizes, all resident in arenas.  Every table below is DEVICE memory, read when
 *      the kernel runs: no host sync, no allocation, no atomics, graph-capturable; rewriting the tables between replays
 *      assembles the next batch.
 *      batch_params: csts_spatial_params with the frame size of clip b taken from clips[b] = {byte offset, N, H, W} (int64; only
 *        H, W are read here).  Clip b draws the variates u[b] of the rule above, so a batch of equal sizes equals
 *        csts_spatial_params bit for bit.  A row with H or W below 1 or outside the rule's range gives params {-1 x 5} (a NaN clip
 *        in every sample pass) and NaN labels.
 *      batch_sample: the pixel rule of csts_spatial_sample / csts_clip_sample, clip b read from its own recording: frame t of
 *        clip b is frame min(max(frames_idx[b][t], 0), N_b - 1) of the (N_b, H_b, W_b, 3) uint8 recording that starts at byte
 *        clips[b][0] of arena_u8.  A recording starts at any byte; only arena_u8 and out must be 16-byte aligned.  LDS is sized
 *        from max_W (<= 6000).  A row gives a NaN clip and reads nothing if [offset, offset + N H W 3) leaves [0, arena_bytes), or
 *        W > max_W, or N, H or W is below 1; no byte at or past arena_bytes is ever read.  out fp32 (B, 3, T, S, S), T <= 64.
 *      audio_gather: window (b, t) = spec_b[:, c - width/2 : c + width/2] with c = centers[b][t] clamped to
 *        [width/2, usable_b - 1 - width/2]; spec_b starts at float specs[b][0] of spec_arena and has rows of specs[b][1] floats, of
 *        which the first specs[b][2] = usable_b are read (the trimmed spectrogram of ego4d_avgaze_forecast.py:215); specs int64
 *        [B][3].  out (B, 1, T, nbins, width), width even, B * T <= 65535.  A row with a negative offset, usable > stride or usable <
 *        width + 1 gives NaN windows and reads nothing; the caller vouches that offset + nbins * stride stays inside the arena. */
int csts_batch_params(const uint64_t* key, const double* labels, const int64_t* clips, int B, int T, int L, int S, int min_scale,
                      int max_scale, int spatial_idx, int random_flip, int inv_uniform, int* params, double* labels_out,
                      hipStream_t stream);
int csts_batch_sample(const uint8_t* arena_u8, int64_t arena_bytes, const int64_t* clips, const int* frames_idx, const int* params,
                      float* out, int B, int T, int S, int max_W, const float mean[3], const float std[3], hipStream_t stream);
int csts_audio_gather(const float* spec_arena, const int64_t* specs, const int* centers, float* out, int B, int T, int nbins,
                      int width, hipStream_t stream);

/* ---- 4:2:0 YUV frames (csts_amd/csrc/yuv.hip, yuv_shared.h; csts_amd/inputs.py): pictures the way video sources deliver them --
 *      NV12 from hardware decoders, I420 (yuv420p) from software ones -- 1.5 bytes per pixel, converted where they are read.
 *      Layouts.  One frame is H * 3 / 2 rows of W bytes, H and W even, rows unpadded (padded rows: "Decoder surfaces" below):
 *        CSTS_YUV_NV12: the Y plane H x W, then H / 2 rows of interleaved U V U V ...
 *        CSTS_YUV_I420: the Y plane H x W, then the U plane (H/2) x (W/2), then the V plane (H/2) x (W/2), each contiguous.
 *      Pixel (y, x) uses Y[y][x] and the chroma sample (y >> 1, x >> 1): nearest replication, no chroma interpolation.
 *      Arithmetic, all int32 (>> is the arithmetic shift), so a pixel is an exact function of three bytes:
 *        y' = Y - yoff, u' = U - 128, v' = V - 128          yoff = 16 (limited range) or 0 (full_range != 0)
 *        R = clamp((CY y' + CRV v' + 2^19) >> 20, 0, 255)
 *        G = clamp((CY y' + CGU u' + CGV v' + 2^19) >> 20, 0, 255)
 *        B = clamp((CY y' + CBU u' + 2^19) >> 20, 0, 255)
 *      {CY, CRV, CGU, CGV, CBU} = round(c 2^20) of the rationals c = {sy, 2 sc (1 - Kr), -2 sc Kb (1 - Kb) / Kg,
 *      -2 sc Kr (1 - Kr) / Kg, 2 sc (1 - Kb)}, Kg = 1 - Kr - Kb, sy = 255/219 and sc = 255/224 (limited) or 1 (full);
 *      CSTS_YUV_BT601: Kr 0.299, Kb 0.114; CSTS_YUV_BT709: Kr 0.2126, Kb 0.0722:
 *        bt601 limited {1220945, 1673555, -410793, -852458, 2115221}    bt601 full {1048576, 1470104, -360853, -748826, 1858077}
 *        bt709 limited {1220945, 1879825, -223607, -558796, 2215014}    bt709 full {1048576, 1651297, -196424, -490864, 1945738}
 *      The accumulators stay below 5.74e8 in magnitude and the result is within 1 of clip(rint(real-valued matrix)) for every
 *      byte triple.  The rule is this library's own statement (the reference decodes with PyAV's to_rgb(), whose swscale
 *      arithmetic is not restated here).
 *      yuv_to_rgb: frames (N, H * 3 / 2, W) -> out (N, H, W, 3) RGB, one streaming pass with 16-byte loads and stores.  frames_yuv
 *        may start at any byte and a frame of H W 3 / 2 bytes at any byte of it; out may start at any byte too (a chunk of a
 *        larger tensor) and must not overlap the input.  H <= 131070.  yuv_to_rgb_host: the same pixel function over HOST memory.
 *      *_sample_yuv: csts_spatial_sample / csts_clip_sample / csts_batch_sample with 4:2:0 pictures in place of RGB ones: frames
 *        (B, T, H * 3 / 2, W), a video (N, H * 3 / 2, W), or an arena whose clip table stays {byte offset, N, H, W} with H the luma
 *        height, a recording occupying N H W 3 / 2 bytes.  Each of the four taps of an output pixel is converted to integer R, G,
 *        B by the rule above and the fp32 expressions of the RGB pass follow in the same order: the result equals, bit for bit,
 *        the RGB function on yuv_to_rgb of the pictures.  Every guarantee of the RGB functions holds: tables read on the DEVICE
 *        when the kernel runs, no host sync, no allocation, graph-capturable, bad params or a bad clip row give a NaN clip and
 *        read nothing, no byte at or past the end of the source is read, W <= 6000, source and out 16-byte aligned.  Odd H or W
 *        is refused (-1) where it is an argument and gives a NaN clip where it stands in a device table.
 *      The inverse rule, rgb_to_yuv (rgb_luma / rgb_chroma of yuv_shared.h), all int32, >> the arithmetic shift:
 *        luma, per pixel:        Y = clamp(((YR R + YG G + YB B + 2^19) >> 20) + yoff, 0, 255)
 *        chroma, per 2 x 2 block, SR, SG, SB = the sums of its four pixels per channel (0..1020) -- a box filter, the counterpart
 *        of the nearest-chroma decode, where the four pixels share one pair:
 *                                U = clamp(((UR SR + UG SG + UB SB + 2^21) >> 22) + 128, 0, 255),  V likewise with VR, VG, VB
 *      {YR, YG, YB | UR, UG, UB | VR, VG, VB} = round(c 2^20) of the rationals c = {ty Kr, ty Kg, ty Kb | -tc Kr / (2 (1 - Kb)),
 *      -tc Kg / (2 (1 - Kb)), tc / 2 | tc / 2, -tc Kg / (2 (1 - Kr)), -tc Kb / (2 (1 - Kr))}, ty = 219/255 and tc = 224/255
 *      (limited) or 1 (full):
 *        bt601 limited {269262, 528618, 102662 | -155423, -305128, 460551 | 460551, -385654, -74897}
 *        bt601 full    {313524, 615514, 119538 | -176932, -347356, 524288 | 524288, -439026, -85262}
 *        bt709 limited {191455, 644067, 65019 | -105533, -355018, 460551 | 460551, -418321, -42230}
 *        bt709 full    {222927, 749942, 75707 | -120138, -404150, 524288 | 524288, -476214, -48074}
 *      The accumulators stay within 2^29 (524288 * 1020 + 2^21) in magnitude and every output is within 1 of floor(real-valued matrix + 0.5) (a
 *      coefficient is off by at most 2^-21 per term).  YUV -> RGB -> YUV is not the identity.
 *      rgb_to_yuv: frames (N, H, W, 3) RGB -> out (N, H * 3 / 2, W) in `layout`, H and W even, one streaming pass with the
 *        staging of yuv_to_rgb: input and output may start at any byte and must not overlap.  H <= 131070.  rgb_to_yuv_host:
 *        the same functions over HOST memory.
 *      Decoder surfaces (the *_win entry points).  A decoder delivers a picture inside an allocation: rows of a pitch wider than
 *        the picture, a coded height taller than it, the chroma plane behind pitch * coded height.  A SURFACE is what the tensor
 *        holds: a tight frame of the allocated size, Hs * 3 / 2 rows of Ws bytes in `layout` exactly as above (chroma from byte
 *        Hs * Ws of a frame; i420: U then V, Hs / 2 rows of Ws / 2 bytes each).  A WINDOW (top, left, H, W) is the picture inside
 *        it: all four even, H, W >= 2, top + H <= Hs, left + W <= Ws; luma (y, x) of the picture is luma (top + y, left + x) of the
 *        surface and its chroma sample (y >> 1, x >> 1) is sample (top / 2 + (y >> 1), left / 2 + (x >> 1)).  A decoder's
 *        surface is the window (0, 0, H, W); a region of interest is any other.  Each *_win function takes the arguments of its
 *        tight twin and Hs, Ws, top, left next to H, W, and equals, bit for bit, the twin on the tight H x W copy of the window:
 *          f_win(surface, ..., H, W, Hs, Ws, top, left)  ==  f(repack(surface), ..., H, W)
 *        No byte of the surface outside the window takes part in a result.  Addresses come from the surface (frame stride
 *        Hs Ws 3 / 2, row pitch Ws, plane offsets Hs Ws and (Hs / 2)(Ws / 2)); clamps, scales, marker and crop geometry, grids and
 *        LDS sizes come from H and W: every limit the twin states for H and W holds for the window (W <= 6000 for the samplers
 *        and the ingest, W <= 8192 and H <= 65534 for the overlay, H <= 131070 for yuv_to_rgb).  The surface's first byte obeys
 *        the twin's alignment rule; the window starts wherever it starts.  Ws <= CSTS_YUV_MAX_WS.  A bad window -- an odd value,
 *        H or W below 2, a window that leaves the surface, Ws over the limit -- returns -1 before any launch.  The tight entry
 *        points are the *_win ones at Hs = H, Ws = W, top = left = 0: one kernel each.
 *        csts_gaze_overlay_yuv_win: out is a surface like frames_yuv, (N, Hs * 3 / 2, Ws).  Its window is csts_gaze_overlay_yuv of
 *        the window (the per-pixel luma rule, the per-block chroma rule); every byte outside the window equals the byte of
 *        frames_yuv.  In place (out == frames_yuv) the bytes outside are not written at all; otherwise, unless the window is the
 *        whole surface, the surface is first copied (one device-to-device copy on `stream`) and the window drawn in place on the copy.
 *        csts_yuv_to_rgb_win: out is the tight (N, H, W, 3). */
enum { CSTS_YUV_NV12 = 1, CSTS_YUV_I420 = 2 };
enum { CSTS_YUV_BT601 = 0, CSTS_YUV_BT709 = 1 };
#define CSTS_YUV_MAX_WS 32768
int csts_rgb_to_yuv(const uint8_t* frames_nhwc, uint8_t* out_yuv, int64_t N, int H, int W, int layout, int matrix, int full_range,
                    hipStream_t stream);
int csts_rgb_to_yuv_host(const uint8_t* frames_nhwc, uint8_t* out_yuv, int64_t N, int H, int W, int layout, int matrix,
                         int full_range);
int csts_yuv_to_rgb(const uint8_t* frames_yuv, uint8_t* out_nhwc, int64_t N, int H, int W, int layout, int matrix, int full_range,
                    hipStream_t stream);
int csts_yuv_to_rgb_host(const uint8_t* frames_yuv, uint8_t* out_nhwc, int64_t N, int H, int W, int layout, int matrix,
                         int full_range);
int csts_spatial_sample_yuv(const uint8_t* frames_yuv, const int* params, float* out, int B, int T, int H, int W, int S,
                            const float mean[3], const float std[3], int layout, int matrix, int full_range, hipStream_t stream);
int csts_clip_sample_yuv(const uint8_t* video_yuv, int64_t N, const int* frames_idx, const int* params, float* out, int B, int T,
                         int H, int W, int S, const float mean[3], const float std[3], int layout, int matrix, int full_range,
                         hipStream_t stream);
int csts_batch_sample_yuv(const uint8_t* arena_u8, int64_t arena_bytes, const int64_t* clips, const int* frames_idx,
                          const int* params, float* out, int B, int T, int S, int max_W, const float mean[3], const float std[3],
                          int layout, int matrix, int full_range, hipStream_t stream);
int csts_yuv_to_rgb_win(const uint8_t* frames_yuv, uint8_t* out_nhwc, int64_t N, int H, int W, int Hs, int Ws, int top, int left,
                        int layout, int matrix, int full_range, hipStream_t stream);
int csts_yuv_to_rgb_win_host(const uint8_t* frames_yuv, uint8_t* out_nhwc, int64_t N, int H, int W, int Hs, int Ws, int top, int left,
                             int layout, int matrix, int full_range);
int csts_spatial_sample_yuv_win(const uint8_t* frames_yuv, const int* params, float* out, int B, int T, int H, int W, int Hs, int Ws,
                                int top, int left, int S, const float mean[3], const float std[3], int layout, int matrix,
                                int full_range, hipStream_t stream);
int csts_clip_sample_yuv_win(const uint8_t* video_yuv, int64_t N, const int* frames_idx, const int* params, float* out, int B, int T,
                             int H, int W, int Hs, int Ws, int top, int left, int S, const float mean[3], const float std[3],
                             int layout, int matrix, int full_range, hipStream_t stream);

/* ---- audio at any sample rate (csts_amd/csrc/resample.hip, csts_amd/inputs.py::resample_audio): band-limited resampling by the
 *      rational ratio up / down (reduced: gcd 1), the step the reference does offline with ffmpeg (data/preprocess.py::
 *      extract_audio, -ar 24000 -ac 1).  Rule, per waveform x of n samples and a filter h of 2 * half + 1 taps (taps, DEVICE
 *      memory, fp32; inputs.resample_filter designs the windowed sinc scipy.signal.resample_poly uses):
 *        n_out = ceil(n * up / down)                                             = csts_resample_len(n, up, down)
 *        y[m]  = sum_i x[i] * h[half + m * down - i * up]   over 0 <= i < n with the h index in [0, 2 * half],
 *      i.e. zero extension at both ends and zero phase: scipy.signal.resample_poly(x, up, down) for that h.  The products are
 *      accumulated in fp32 in the order of i.  wav: (B, C, n) contiguous, fp32 (CSTS_WAV_F32) or int16 (CSTS_WAV_I16, scaled by
 *      1 / 32768); x is the mean of the C channels (summed in the order of c, divided by C), taken while the samples are staged:
 *      the downmix has no pass of its own.  out fp32 (B, n_out).  Positions are 64-bit.  No host sync, no allocation, no atomics:
 *      graph-capturable.  Limits: B <= 65535, C <= 64, n <= CSTS_RESAMPLE_MAX_N, up, down, half <= CSTS_RESAMPLE_MAX_RATIO, and
 *      the phase-major filter table with the input span of one run of CSTS_RESAMPLE_RUN outputs must fit the kernel's LDS:
 *        up * (ceil((2 half + 1) / up) | 1) + s + s / 32 + 1 <= CSTS_RESAMPLE_MAX_LDS_FLOATS,
 *        s = ((CSTS_RESAMPLE_RUN - 1) * down + 2 * half) / up + 2   (integer divisions).
 *      A call outside them, or with a null pointer, returns -1 and launches nothing (csts_resample_len returns -1). */
enum { CSTS_WAV_F32 = 0, CSTS_WAV_I16 = 1 };
#define CSTS_RESAMPLE_RUN 256
#define CSTS_RESAMPLE_MAX_LDS_FLOATS 16384
#define CSTS_RESAMPLE_MAX_RATIO (1 << 20)
#define CSTS_RESAMPLE_MAX_N ((int64_t)1 << 40)
int64_t csts_resample_len(int64_t n, int up, int down);
int csts_resample_wav(const void* wav, int in_kind, int B, int C, int64_t n, const float* taps, int up, int down, int half,
                      float* out, hipStream_t stream);

/* ---- the same resampling on a live stream (csts_amd/csrc/resample.hip, csts_amd/inputs.py::StreamResampler): a range of the
 *      outputs of a stream from a buffer that holds only part of it.  Output m of the rule above reads the inputs
 *        csts_resample_first_input(m) = max(ceil((m * down - half) / up), 0)  ..  floor((m * down + half) / up),
 *      so it is final once the latter is in.  After n_in inputs the final outputs are [0, csts_resample_ready(n_in, ...)):
 *        open stream   (closed = 0):  max(0, floor((n_in * up - half - 1) / down) + 1)
 *        ended stream  (closed = 1):  ceil(n_in * up / down)                   (the offline zero extension past the last sample)
 *      Both return -1 outside the limits above (n_in in [0, CSTS_RESAMPLE_MAX_N], m >= 0).  An open stream holds back between
 *      10 and 30 outputs for the filters of inputs.resample_rule, and must keep n_in - first_input(ready(n_in)) <=
 *      2 * half / up + 2 input samples per channel from one call to the next.
 *      csts_resample_stream: buf (C, len) contiguous, fp32 or int16 as csts_resample_wav's wav, holds the stream samples
 *      [x_base, x_base + len); out[m - m0] receives output m for m in [m0, m1), by the kernel and the arithmetic of
 *      csts_resample_wav (B = 1): the same products in the same order, so the bits are those of csts_resample_wav on the whole
 *      waveform, however the stream was cut (runs of CSTS_RESAMPLE_RUN outputs start at m0; a sum does not depend on its run).
 *        n_total < 0   the stream is open: every input an output reads is in the buffer, m1 <= csts_resample_ready(x_base + len, 0);
 *        n_total >= 0  the stream ended at that length: x_base + len == n_total and m1 <= ceil(n_total * up / down); the sums are
 *                      cut at n_total - 1.
 *      In both, csts_resample_first_input(m0) >= x_base, 0 <= m0 <= m1, len >= 1, x_base + len <= CSTS_RESAMPLE_MAX_N, and the
 *      limits of csts_resample_wav on C, the ratio and the LDS table hold.  m0 == m1 returns 0 and launches nothing.  A call
 *      outside these conditions returns -1, sets csts_last_error and launches nothing; the kernel additionally keeps every read
 *      inside [0, len) of the buffer.  No host sync, no allocation, no atomics: graph-capturable. */
int64_t csts_resample_ready(int64_t n_in, int up, int down, int half, int closed);
int64_t csts_resample_first_input(int64_t m, int up, int down, int half);
int csts_resample_stream(const void* buf, int in_kind, int C, int64_t len, int64_t x_base, int64_t n_total, const float* taps, int up,
                         int down, int half, int64_t m0, int64_t m1, float* out, hipStream_t stream);

/* ---- gaze head of the inference path (csts_amd/csrc/decode.hip): one read of a frame's logits gives every consumer of a
 *      prediction what it needs.  logits: nframes = B * T frames of H * W cells each, the (B, 1, T, H, W) model output, fp32
 *      (dt CSTS_F32) or the 16-bit type of the library (dt CSTS_BF16); arithmetic is fp32 in both libraries.  Rule, per frame,
 *      with z[i] = logits[i] * (1 / temperature) (temperature > 0; 2 on this path):
 *        preds[i]    = exp(z[i] - max z) / sum_j exp(z[j] - max z)          frame_softmax, slowfast/utils/utils.py:5-12
 *        rescaled[i] = (preds[i] - min preds) / (max preds - min preds + 1e-6)   tools/test_avgaze_net.py:68-70
 *        i*          = the lowest flat index whose logit is the frame's maximum (the softmax is monotone, so this is the
 *                      maximum of the heat map; comparing logits keeps two cells apart whose probabilities round alike)
 *        points      = {(i* mod W) / W, (i* div W) / H}: x then y in [0, 1), the inverse of the centre rule mu_x = round(x W),
 *                      mu_y = round(y H) of _get_gaussian_map (ego4d_avgaze_forecast.py:404-407)
 *        peak        = preds[i*]
 *      Outputs fp32: preds and rescaled [nframes][H * W], points [nframes][2], peak [nframes]; each may be NULL and is then
 *      skipped.  One workgroup per frame holds the frame in registers, so H * W <= CSTS_GAZE_DECODE_MAX_HW (32 values per lane
 *      of 256); nframes >= 1.  128-bit accesses when H * W is a multiple of 4 and logits, preds and rescaled are 16-byte
 *      aligned, scalar ones otherwise.  One launch; no allocation, no synchronisation, no host read: graph-capturable. */
#define CSTS_GAZE_DECODE_MAX_HW 8192
int csts_gaze_decode(const void* logits, int dt, int64_t nframes, int H, int W, float temperature, float* preds, float* rescaled,
                     float* points, float* peak, hipStream_t stream);

/* ---- gaze track of a whole video (csts_amd/csrc/decode.hip): P heat maps preds [P][H * W] fp32 (the preds of gaze_decode of
 *      every window), each predicting one video frame, become one map per output frame f in [0, F).
 *      order[offsets[f] .. offsets[f + 1]) lists the rows of preds that target frame f, in ascending row order (offsets
 *      int32 [F + 1], non-decreasing, order int32 with values in [0, P); both in DEVICE memory).  Rule, per frame, with
 *      n = offsets[f + 1] - offsets[f]:
 *        m        = (((0 + row_0) + row_1) + ... + row_{n-1}) * (1 / n)      fp32, rows added in list order
 *        heatmaps = m;  rescaled = (m - min m) / (max m - min m + 1e-6)
 *        i*       = the lowest flat index whose m is the maximum;  points = {(i* mod W) / W, (i* div W) / H};  peak = m[i*]
 *        count    = n
 *      exactly as csts_gaze_decode defines rescaled, points and peak, on the mean map.  n == 0 (no window predicts the frame):
 *      heatmaps and rescaled 0, points NaN, peak 0, count 0.  Outputs: heatmaps and rescaled [F][H * W], points [F][2],
 *      peak [F] fp32, count [F] int32; each may be NULL and is then skipped.  One workgroup per output frame keeps the sum in
 *      registers: H * W <= CSTS_GAZE_DECODE_MAX_HW, 1 <= F < 2^31.  No atomics: the result is deterministic.  128-bit accesses
 *      when H * W is a multiple of 4 and preds, heatmaps and rescaled are 16-byte aligned, scalar ones otherwise.  One launch;
 *      no allocation, no synchronisation, no host read: graph-capturable. */
int csts_gaze_track(const float* preds, const int* order, const int* offsets, int64_t F, int H, int W, float* heatmaps,
                    float* rescaled, float* points, float* peak, int* count, hipStream_t stream);

/* ---- filling the gaze track between predictions (csts_amd/csrc/decode.hip): the model predicts T frames per window,
 *      SAMPLING_RATE + 1 frames apart, so the track of csts_gaze_track is sparse.  This gives every frame between two
 *      neighbouring predictions a map: what the num_repeat loops of slowfast/visualization/visualization.py (vis_video :105-127,
 *      vis_video_forecasting :146-169) do by holding a map over the following frames.  heatmaps [F][H * W] fp32 and count [F]
 *      int32 are the outputs of csts_gaze_track.  Rule, per frame n:
 *        count[n] > 0 (predicted):  neighbours (n, n); the frame passes through, m = heatmaps[n].
 *        count[n] == 0:  a = the largest predicted frame below n, b = the smallest predicted frame above n.
 *                        both exist and b - a <= max_gap (filled):  neighbours (a, b);
 *                          mode 0 (hold):    m = heatmaps[a]
 *                          mode 1 (linear):  m = wa * heatmaps[a] + wb * heatmaps[b] in fp32 (two products, one sum, no
 *                                            contraction), wa = (float)(b - n) / (float)(b - a), wb = (float)(n - a) / (float)(b - a):
 *                                            a convex combination, so still a probability map
 *                        otherwise (unpredicted):  neighbours (-1, -1); maps 0, points NaN, peak 0.
 *        out_heatmaps = m;  out_rescaled, out_points, out_peak from m exactly as csts_gaze_track derives them from its mean
 *        (min-max with + 1e-6, the lowest flat index of the maximum), by the same device function: a predicted frame comes out
 *        with the bits csts_gaze_track wrote, a held frame with those of frame a.
 *      Nothing is extrapolated before the first or after the last predicted frame.  Each workgroup finds a and b itself by
 *      scanning count at most max_gap - 1 frames each way: no table from the host, no sort, nothing read back.  Outputs:
 *      out_heatmaps and out_rescaled [F][H * W], out_points [F][2], out_peak [F] fp32, out_neighbours [F][2] int32; each may be
 *      NULL and is then skipped; with all NULL nothing is launched.  No output may overlap heatmaps or count, in whole or in
 *      part: a workgroup reads other frames' maps while their workgroups write.  An output that STARTS at heatmaps is
 *      refused (-1); any other overlap is the caller's to avoid.  One workgroup per output frame keeps the map in registers: H * W <= CSTS_GAZE_DECODE_MAX_HW,
 *      1 <= F < 2^31, 1 <= max_gap <= CSTS_GAZE_FILL_MAX_GAP.  128-bit accesses when H * W is a multiple of 4 and heatmaps,
 *      out_heatmaps and out_rescaled are 16-byte aligned, scalar ones otherwise.  One launch; no allocation, no
 *      synchronisation, no host read: graph-capturable. */
#define CSTS_GAZE_FILL_MAX_GAP 1024
int csts_gaze_track_fill(const float* heatmaps, const int* count, int64_t F, int H, int W, int mode, int max_gap,
                         float* out_heatmaps, float* out_rescaled, float* out_points, float* out_peak, int* out_neighbours,
                         hipStream_t stream);

/* ---- gaze overlay (csts_amd/csrc/overlay.hip): the heat map of a gaze track blended onto the source frames and a disc at the
 *      gaze point, what slowfast/visualization/visualization.py (vis_inference, vis_video_forecasting) draws with cv2: map
 *      resized to the frame, JET colours, 0.6 frame + 0.4 heat, a filled green circle.  cv2 is not a dependency, so the rule
 *      below is this project's own statement of it; it is not pinned against cv2's pixels.
 *      frames_nhwc (N, H, W, 3) uint8 RGB; rescaled (N, mh, mw) fp32 in [0, 1], the `rescaled` of gaze_decode / gaze_track (no
 *      min-max here); centers int32 [N][2] = marker centre (X, Y) in source pixels, X < 0: no marker and an untouched frame;
 *      centers NULL: no markers at all; params int32 [5] in DEVICE memory = {new h, new w, y0, x0, flip}, the row
 *      csts_spatial_sample / csts_clip_sample took: how the S x S crop the map covers was cut from the frame; out (N, H, W, 3)
 *      uint8, may alias frames_nhwc (the op is elementwise per pixel).  Rule per output pixel (n, Y, X), nh = new h, nw = new w:
 *        inside the crop  iff  y0 * 2H <= (2Y + 1) * nh < (y0 + S) * 2H  and  x0 * 2W <= (2X + 1) * nw < (x0 + S) * 2W  (64-bit
 *                         integers): the pixel centre, taken through the resize H -> nh, lies in the crop's extent.  flip is
 *                         ignored (test mode never flips).  A row outside the sampler's range (nh < S, nw < S, an offset outside
 *                         [0, n - S], a side above 2^24) has no inside.
 *        outside the crop, or a frame whose centre X < 0:  out = frame, byte for byte.
 *        inside, crop coordinates:  cy = (Y + 0.5) * nh / H - 0.5 - y0, then the map position my = (cy + 0.5) * mh / S - 0.5; x
 *                         alike.  Both are evaluated EXACTLY, as the rational my = A / D with A = ((2Y + 1) nh - 2H y0) mh - H S
 *                         and D = 2 H S in 64-bit integers.
 *        inside, bilinear sample with the edge clamp of spatial_sample:  src = max(my, 0), i0 = min(floor(src), mh - 1),
 *                         i1 = min(i0 + 1, mh - 1), lambda = src - i0 = fl((A mod D) / D) (0 where A <= 0); then in fp32
 *                         top = fma(lx, m[i0][j1] - m[i0][j0], m[i0][j0]), bot likewise on row i1, v = fma(ly, bot - top, top).
 *        inside, quantise:  q = min(255, (int)(v * 255))   (fp32 product, truncation)
 *        heat colour (integers, the classic JET):  r = clamp(383 - |4q - 765|, 0, 255), g = clamp(383 - |4q - 510|, 0, 255),
 *                         b = clamp(383 - |4q - 255|, 0, 255)
 *        blend:           out_c = (uint8) rintf((1 - alpha) * frame_c + alpha * heat_c), fp32 without contraction, 0 <= alpha <= 1
 *                         (at the default 0.4 the exact value is a multiple of 0.2, never a tie)
 *        marker:          where (X - cX)^2 + (Y - cY)^2 <= radius^2 (radius >= 0) the pixel is (0, 255, 0), inside or outside
 *                         the crop.
 *      One launch, no allocation, no host read (params and centers are read on the device): graph-capturable.  The map is staged
 *      in LDS per workgroup: mh * mw <= CSTS_GAZE_DECODE_MAX_HW.  96-bit loads and stores, 4 pixels a lane, when W % 4 == 0 and
 *      frames and out are 4-byte aligned; byte accesses otherwise, with the same bytes out.  N >= 1, H <= 65535, W <= 8192,
 *      S <= 4096, N * ceil(H / 32) < 2^31. */
int csts_gaze_overlay(const uint8_t* frames_nhwc, const float* rescaled, const int* centers, const int* params, uint8_t* out,
                      int64_t N, int H, int W, int S, int mh, int mw, float alpha, int radius, hipStream_t stream);

/* ---- gaze overlay in 4:2:0 (csts_amd/csrc/overlay.hip): the same picture drawn onto NV12 / I420 frames (the layouts and colour
 *      rules of "4:2:0 YUV frames" above) and written in the same layout: 1.5 bytes in and 1.5 bytes out per pixel, no RGB picture
 *      in memory.  frames_yuv and out (N, H * 3 / 2, W) uint8, at any byte; every other argument as csts_gaze_overlay takes it.
 *      Let D be what csts_gaze_overlay gives on csts_yuv_to_rgb(frames_yuv), and M the drawn mask: a pixel is in M when it lies
 *      inside the crop of a frame whose centre X is not negative (or centers is NULL), or under the disc -- geometry only,
 *      whatever alpha and the pixel's value.  Then
 *        luma of a pixel in M        = the luma rule of rgb_to_yuv on D at that pixel;   outside M = its source byte;
 *        chroma of a 2 x 2 block with at least one pixel in M = the chroma rule on the sums of D over its four pixels (the undrawn
 *                                      ones are the forward rule of their source bytes);   with none = its source bytes,
 *      i.e. out = where(M, rgb_to_yuv(D), frames), M per pixel for luma and per block (any) for chroma.  The shaded RGB is that
 *      of csts_gaze_overlay bit for bit (the same functions).  Consequences: an untouched frame, row pair or block comes back byte
 *      for byte; a drawn pixel at alpha = 0 is re-encoded and may differ from its source luma (YUV -> RGB -> Y is not the
 *      identity).  out == frames_yuv renders in place (a workgroup reads its bytes before it writes them and none reads bytes
 *      another writes); any other overlap is refused (-1), as are odd H or W, W > 8192, H > 65534, mh * mw >
 *      CSTS_GAZE_DECODE_MAX_HW, and nothing is written then.  One launch, no allocation, no host read: graph-capturable.
 *      N * ceil(H / 32) * ceil(W / 2048) < 2^31. */
int csts_gaze_overlay_yuv(const uint8_t* frames_yuv, const float* rescaled, const int* centers, const int* params, uint8_t* out,
                          int64_t N, int H, int W, int S, int mh, int mw, float alpha, int radius, int layout, int matrix,
                          int full_range, hipStream_t stream);
/* the same on the window of a decoder surface ("Decoder surfaces" above): frames_yuv and out (N, Hs * 3 / 2, Ws) */
int csts_gaze_overlay_yuv_win(const uint8_t* frames_yuv, const float* rescaled, const int* centers, const int* params, uint8_t* out,
                              int64_t N, int H, int W, int Hs, int Ws, int top, int left, int S, int mh, int mw, float alpha,
                              int radius, int layout, int matrix, int full_range, hipStream_t stream);

/* ---- gaze overlay of a group (csts_amd/csrc/overlay.hip, csts_amd.GazeLiveGroup): the frames several streams pushed in one tick,
 *      each stream of its own H x W, drawn by ONE launch from a job table, and their marker centres by one more.
 *      jobs int64 [njobs][13], one row per job, in DEVICE memory, read when the kernel runs:
 *        {0 source address, 1 destination address, 2 K frames, 3 H, 4 W, 5 new h, 6 new w, 7 y0, 8 x0, 9 flip (ignored, as
 *         csts_gaze_overlay ignores it), 10 first row, 11 first workgroup, 12 vector flag}
 *      columns 5..9 are the job's params row; first row = where the job's K rows start in rescaled [P][mh * mw] fp32 and centers
 *      int32 [P][2] (NULL: no markers): the sum of K of the jobs before it when the table holds every job of P = the sum of K
 *      (group_points_source requires that), and at least that for the overlays, whose table may leave jobs out; first workgroup =
 *      the sum of K * ceil(H / 32) of the table's jobs before it.  The frames of a job are uint8 (K, H, W, 3), or (K, H * 3 / 2, W) in the one 4:2:0
 *      layout, matrix and range of the call.  S, mh, mw, alpha and radius are one per call.  jobs_host is the HOST copy of the same
 *      table: the entry validates it and sizes the launch from it before anything is launched, as csts_group_ingest does
 *      (csts_amd.infer.overlay_group_table is the rule of columns 10..12 in Python).
 *      The grid is the sum of K * ceil(H / 32) over the jobs.  A workgroup finds its job by binary search over column 11 (the
 *      table is read through the scalar path: every index is uniform over the workgroup), then frame (g - first workgroup) /
 *      bands and band (g - first workgroup) % bands, and from there on runs the code of csts_gaze_overlay /
 *      csts_gaze_overlay_yuv's vector kernel on that band (one device function each): out of job j equals
 *      csts_gaze_overlay(frames_j, rescaled[first row ..], centers[first row ..], params_j) byte for byte.
 *      group_gaze_overlay: the vector flag chooses, per job, the 96-bit path (4 pixels a lane) or the byte path inside the one
 *        launch; it may be set only when W % 4 == 0 and source and destination are 4-byte aligned, and may always be clear.
 *      group_gaze_overlay_yuv: every job must be on the vector path (flag 1: W % 4 == 0, 4-byte aligned); a job that is not goes
 *        through csts_gaze_overlay_yuv on its own (csts_amd.ops.group_gaze_overlay does that).  Even H, W; H <= 65534.
 *      The dynamic LDS is that of the WIDEST job of the call (8 bytes a column + the map + 3.5 KB): a wide job lowers the
 *      occupancy of the narrow jobs beside it (with a 64 x 64 map a workgroup takes 19.5 KB + 8 W bytes of a CU's 160 KB: five
 *      workgroups a CU at W = 1088, four at W = 1920, one at W = 8192).  The launch is not split for that: a tick's streams
 *      come from like cameras, and a second launch costs more than the occupancy.  csts_dyn_lds_optin is called above 64 KB.
 *      A job whose row on the device disagrees with the launch (frame past K, W wider than the LDS) writes nothing.
 *      In place (destination == source) is legal per job.  Otherwise no job's destination may overlap its own source, another
 *      job's source or another job's destination: refused (-1), as are njobs outside 1..65535, a null address, K < 1, H > 65535,
 *      W > 8192, a first row or first workgroup that is not the running sum, a vector flag on a job that cannot take it, P or
 *      the grid >= 2^31.  One launch, no allocation, no host read of device memory, no atomics: graph-capturable.
 *      group_points_source: points fp32 [P][2] = (x, y) on the S x S crop (csts_gaze_decode's `points`) -> points_source fp64
 *        [P][2] and centers int32 [P][2]; columns 0, 1 and 12 of the table are not read.  For row p of job j (binary search over
 *        column 10), in IEEE double arithmetic without contraction, each operation rounded once:
 *          x_src = ((double)x * S + x0) / new w,  y_src = ((double)y * S + y0) / new h     (points_source)
 *          X = (int)floor(x_src * W),  Y = (int)floor(y_src * H);  a NaN in either coordinate gives centers (-1, -1) and leaves
 *          the NaN in points_source
 *        -- csts_amd.infer.points_to_source followed by marker_centers, bit for bit.  One thread per row, one launch. */
int csts_group_gaze_overlay(const int64_t* jobs, const int64_t* jobs_host, int njobs, const float* rescaled, const int* centers,
                            int S, int mh, int mw, float alpha, int radius, hipStream_t stream);
int csts_group_gaze_overlay_yuv(const int64_t* jobs, const int64_t* jobs_host, int njobs, const float* rescaled, const int* centers,
                                int S, int mh, int mw, float alpha, int radius, int layout, int matrix, int full_range,
                                hipStream_t stream);
int csts_group_points_source(const int64_t* jobs, const int64_t* jobs_host, int njobs, const float* points, int S,
                             double* points_source, int* centers, hipStream_t stream);

/* ---- fusion attention maps (csts_amd/csrc/fusion_maps.hip): the audio-visual correlation map of the spatial fusion block, what
 *      vis_av_st_fusion of slowfast/visualization/visualization.py:172-228 draws per head: for every frame, how strongly each image
 *      region attends to that frame's audio token.  It reads what the block's forward already holds and forms no (N, N) matrix.
 *      qkv (B, N, 3C) packed q | k | v rows of the block, fp32 (dt CSTS_F32) or the library's 16-bit type (dt CSTS_BF16), C =
 *      heads * head_dim, N = T' h w + T' (the video tokens of the grid (T', h, w), then one audio token per frame); lse
 *      (B, heads, N) fp32 = the log-sum-exp of every query row in the LOG2 domain, as csts_attn_fwd writes it (the spatial mask
 *      is inside it; the mask never hides a frame's own audio token, so none is applied here); T = input frames, S = crop side.
 *      Rule, all fp32, with c = y w + x, HW = h w:
 *        column[b][k][t][c]   = exp2f(fl(fl(s * fl(scale * 1.4426950408889634f)) - lse[b][k][t HW + c])),
 *                               s = <q[b][t HW + c][k][:], key[b][T' HW + t][k][:]> : lane l of a wave multiplies elements l, l + 64,
 *                               ... and adds them in that order, then a 64-lane xor butterfly (offsets 32 .. 1) adds the lanes.
 *                               This is attn[:, :, HW t : HW (t + 1), THW + t] of visualization.py:190.
 *        column_mean[b][t][c] = ((0 + column[b][0][t][c]) + column[b][1][t][c] + ...) / heads   (heads ascending, one division)
 *        index g of maps / range:  g < heads: head g of column;  g == heads: column_mean.
 *        time, input frame j:   u = max((j + 0.5) T' / T - 0.5, 0) = max(A / D, 0) with A = (2j + 1) T' - T, D = 2T in integers;
 *                               t0 = min(floor(u), T' - 1), t1 = min(t0 + 1, T' - 1), lambda = fl((A mod D) / D) (0 where A <= 0);
 *                               m_j = fl(fl((1 - lambda) * col[t0]) + fl(lambda * col[t1]))   -- the temporal part of
 *                               F.upsample(mode='trilinear', align_corners=False); T == T' gives lambda = 0, m_j = col[j].
 *        space:                 lattice point p of the S x S crop sits on a map axis of n cells at max((p + 0.5) n / S - 0.5, 0),
 *                               the same rational with (p, S, n) for (j, T, T'); neighbours clamped to n - 1; the sample is
 *                               top = fma(lx, m[i0][j1] - m[i0][j0], m[i0][j0]), bot likewise on row i1, v = fma(ly, bot - top, top):
 *                               exactly what csts_gaze_overlay evaluates at that pixel of an identity crop.
 *        range[b][g][j]       = (lo, hi) = the minimum and maximum of v over the S x S lattice.  A bilinear patch is extremal at
 *                               its corners, so only the first and last lattice point of every run that shares (i0) on an axis
 *                               are evaluated: at most 2h x 2w points.  No lattice point sits on a cell centre, so (lo, hi) lie
 *                               strictly inside the coarse map's own extrema.
 *        maps[b][g][j][c]     = (m_j[c] - lo) / (hi - lo + 1e-6)
 *      Bilinear weights sum to one, so upsampling this rescaled coarse map equals the reference's order (upsample, then per-frame
 *      min-max) up to rounding: csts_gaze_overlay draws maps[b][g][j] (mh = h, mw = w) unchanged.  Cells between lattice points
 *      may leave [0, 1] by what the patch overshoots; the overlay clamps its quantised value.
 *      Outputs fp32: column (B, heads, T', h, w), column_mean (B, T', h, w), maps (B, heads + 1, T, h, w), range
 *      (B, heads + 1, T, 2); none may be NULL.  Sizes: B, heads >= 1; 1 <= head_dim <= CSTS_AUDIO_PIXEL_MAX_HD; 1 <= h, w <=
 *      CSTS_AUDIO_PIXEL_MAX_SIDE, h w <= CSTS_AUDIO_PIXEL_MAX_HW; 1 <= T, T', S <= 65536; B heads T', B (T (heads + 1) + T') and
 *      N * 3C below 2^31.  Two launches on `stream` (the column, then everything derived from it); no allocation, no
 *      synchronisation, no host read: graph-capturable.  No atomics: deterministic. */
#define CSTS_AUDIO_PIXEL_MAX_HD 256
#define CSTS_AUDIO_PIXEL_MAX_SIDE 128
#define CSTS_AUDIO_PIXEL_MAX_HW 4096
int csts_audio_pixel_attn(const void* qkv, int dt, const float* lse, int B, int heads, int head_dim, int Tp, int h, int w, int T,
                          int S, float scale, float* column, float* column_mean, float* maps, float* range, hipStream_t stream);

/* ---- whole-recording attention track (csts_amd/csrc/fusion_maps.hip): the fusion attention maps of every window of a recording
 *      (csts_audio_pixel_attn's `column`, windows concatenated) become one map per video frame, head and head mean -- for the
 *      attention what csts_gaze_track is for the heat maps.
 *      column [Wn][heads][T'][h * w] fp32.  A pair is p = w * T + j: window w, input frame j of its T input frames; it lands on
 *      the video frame frames_idx[w][j].  order[offsets[f] .. offsets[f + 1]) lists the pairs of output frame f in [0, F) in
 *      ascending p (offsets int32 [F + 1], non-decreasing, order int32 with values in [0, Wn * T); both in DEVICE memory): the
 *      lists csts_gaze_track takes, here of input frames.  A pair whose frame lies outside [0, F) is in no list: it is dropped.
 *      Rule, all fp32, per output frame f and index g in [0, heads] (g == heads: the head mean), n = offsets[f + 1] - offsets[f]:
 *        m_p          = the map csts_audio_pixel_attn mixes for (window w, input frame j, g) before it rescales it:
 *                       fl(fl((1 - lambda) col[t0]) + fl(lambda col[t1])) with (t0, t1, lambda) of input frame j on the axis
 *                       (T, T') as stated there; for g == heads col[t] is the head mean ((0 + c_0) + c_1 + ...) / heads of the
 *                       coarse map t, taken BEFORE the mix.  One device function serves both entries: the bits are equal.
 *        mixed[f][g]  = (((0 + m_p0) + m_p1) + ... ) * (1 / n), pairs added in list order: the mean of csts_gaze_track.
 *        range[f][g]  = (lo, hi) = the extrema of the bilinear upsample of mixed[f][g] over the S x S crop lattice, from the end
 *                       pixels of every cell interval, by the device function csts_audio_pixel_attn evaluates them with.
 *        maps[f][g]   = (mixed[f][g] - lo) / (hi - lo + 1e-6)
 *        count[f]     = n
 *        n == 0 (no pair lands on the frame):  mixed and maps 0, range (NaN, NaN), count 0.
 *      The mean comes before the rescale: the extrema of a mean are not the mean of the extrema, and a picture rescaled by its own
 *      extrema is what csts_gaze_overlay draws.  A frame exactly one pair hits therefore carries, bit for bit, the maps and range
 *      csts_audio_pixel_attn gives for that window and input frame ((0 + m) * 1 = m).
 *      Outputs: mixed, maps [F][heads + 1][h * w], range [F][heads + 1][2] fp32, count [F] int32; none may be NULL.  Sizes: Wn,
 *      heads, F >= 1; 1 <= h, w <= CSTS_AUDIO_PIXEL_MAX_SIDE, h w <= CSTS_AUDIO_PIXEL_MAX_HW; 1 <= T, T', S <= 65536; Wn T and
 *      F (heads + 1) below 2^31.  Two launches on `stream`: one workgroup per (f, g) walks its pair list with the sum in LDS, then
 *      csts_attention_rescale with valid = count.  No atomics (deterministic), no allocation, no synchronisation, no host read:
 *      graph-capturable. */
int csts_attention_track(const float* column, const int* order, const int* offsets, int64_t F, int Wn, int heads, int Tp, int h,
                         int w, int T, int S, float* mixed, float* maps, float* range, int* count, hipStream_t stream);

/* ---- extrema and rescale of coarse maps (csts_amd/csrc/fusion_maps.hip): mixed [F][G][h * w] fp32, G = nmaps_per_frame ->
 *      range[f][g] = (lo, hi), the extrema of the bilinear upsample of mixed[f][g] over the S x S lattice, and maps[f][g] =
 *      (mixed[f][g] - lo) / (hi - lo + 1e-6), exactly as csts_attention_track states them (it is that entry's second launch).
 *      valid int32 [F] in DEVICE memory or NULL: a frame with valid[f] <= 0 gets maps 0 and range (NaN, NaN); NULL: every frame
 *      is valid.  Called alone after a fill of `mixed` (csts_gaze_track_fill on the maps viewed as one tall map per frame), with
 *      valid = predicted or filled.  maps must not be mixed.  Sizes as above; F G below 2^31.  One launch, one workgroup per
 *      (f, g); no allocation, no synchronisation, no host read: graph-capturable. */
int csts_attention_rescale(const float* mixed, const int* valid, int nmaps_per_frame, int64_t F, int h, int w, int S, float* maps,
                           float* range, hipStream_t stream);

/* ---- live stream (csts_amd/csrc/stream.hip, csts_amd/stream.py): frames and audio of an endless recording arrive in pieces; what
 *      the windows read lives in two device rings whose size does not depend on the length of the stream.  Every table below is
 *      DEVICE memory read when the kernel runs; no atomics, no allocation, no synchronisation.
 *      stream_stft: columns [f0, f1) of csts_stft_logpower's spectrogram of the endless signal, column f written to
 *        ring[bin][f mod ring_cols]; ring fp32 (n_fft / 2 + 1, ring_cols).  buf holds the samples [s_base, s_base + m) of the signal.
 *        Column f reads the samples [f hop + (n_fft - win) / 2 - n_fft / 2, + win) (= [120 f - 120, 120 f + 120) for 511 / 120 / 240);
 *        samples before 0 are zero and, with n_total >= 0 (the signal ended after n_total samples), so are those at or past n_total,
 *        which is what csts_stft_logpower does at the two ends of a waveform; n_total < 0: the signal goes on.  A column that needs
 *        any other sample outside the buffer is refused (-1) before launch, as are f1 - f0 > ring_cols and n_total > s_base + m.
 *        The arithmetic of a column is csts_stft_logpower's, term for term (one device function, stft_shared.h): column f equals
 *        column f of the spectrogram of the whole signal bit for bit.
 *      stream_audio_windows: out (B, 1, T, nbins, width), window (b, t) = ring columns (centers[b][t] - width / 2 + j) mod ring_cols,
 *        j in [0, width); centers int64 [B][T] are GLOBAL column numbers and newest is the last column written.  A window that does
 *        not lie wholly inside the live span [max(newest - ring_cols + 1, 0), newest] is NaN and reads nothing.  width even and
 *        <= ring_cols, B * T <= 65535.
 *      stream_ingest / stream_ingest_yuv: pairs int32 [npairs][2] = (frame in chunk, slot): frame pairs[p][0] of the chunk -- uint8
 *        (K, H, W, 3), or (K, H * 3 / 2, W) in a 4:2:0 layout -- is sampled into ring[slot] of the crop ring fp32 (R, 3, S, S) by the
 *        pixel rule of csts_clip_sample / csts_clip_sample_yuv under the ONE parameter row params int32 [5]: ring[slot] equals
 *        csts_clip_sample(...)[0, :, 0] of that frame bit for bit.  A chunk frame no pair names is not read and no other slot is
 *        written.  A pair with the frame outside [0, K) or the slot outside [0, R) writes nothing; bad params give a NaN slot.  No
 *        byte at or past the end of the chunk is read; chunk and ring 16-byte aligned, W <= 6000, 1 <= npairs <= 65535.
 *        stream_ingest_yuv_win: the chunk is (K, Hs * 3 / 2, Ws) and its frames are the windows ("Decoder surfaces" above).
 *      stream_gather: out fp32 (B, 3, T, S, S), out[b][:, t] = ring[slots[b][t]]; slots int32 [B][T]; a slot outside [0, R) gives
 *        a NaN frame and reads nothing.  T <= 64, B <= 65535. */
int csts_stream_stft(const float* buf, int64_t s_base, int64_t m, int64_t n_total, int64_t f0, int64_t f1, float* ring, int ring_cols,
                     int n_fft, int hop, int win, float eps, hipStream_t stream);
int csts_stream_audio_windows(const float* ring, int ring_cols, int64_t newest, const int64_t* centers, float* out, int B, int T,
                              int nbins, int width, hipStream_t stream);
int csts_stream_ingest(const uint8_t* chunk_khwc, int K, int H, int W, const int* pairs, int npairs, const int* params, float* ring,
                       int R, int S, const float mean[3], const float std[3], hipStream_t stream);
int csts_stream_ingest_yuv(const uint8_t* chunk_yuv, int K, int H, int W, const int* pairs, int npairs, const int* params, float* ring,
                           int R, int S, const float mean[3], const float std[3], int layout, int matrix, int full_range,
                           hipStream_t stream);
int csts_stream_ingest_yuv_win(const uint8_t* chunk_yuv, int K, int H, int W, int Hs, int Ws, int top, int left, const int* pairs,
                               int npairs, const int* params, float* ring, int R, int S, const float mean[3], const float std[3],
                               int layout, int matrix, int full_range, hipStream_t stream);
int csts_stream_gather(const float* ring, int R, const int* slots, float* out, int B, int T, int S, hipStream_t stream);

/* ---- stream group (csts_amd/csrc/stream.hip, csts_amd.GazeStreamGroup): N streams share one arena of crop rings, fp32
 *      (streams * R, 3, S, S) -- ring slot r of stream i is arena slot i * R + r -- and one of spectrum rings, fp32
 *      (streams, n_fft / 2 + 1, ring_cols); what several streams pushed in one tick goes in with ONE launch per stage, from a job
 *      table.  Every table is DEVICE memory read when the kernel runs (a workgroup finds its job from its block index alone, so
 *      the reads are uniform); no atomics, no allocation, no synchronisation, no host read of device memory.  jobs_host is the
 *      HOST copy of the same job table: the entry validates it and sizes the launch from it before anything is launched.  The
 *      arithmetic is the single-stream kernels' (one device function each): a column, a crop, a window has the bits it has there.
 *      group_stft: jobs int64 [njobs][8] = {address of the job's fp32 sample buffer, s_base, m, n_total, f0, f1, stream, first
 *        workgroup of the job = the number of columns of the jobs before it}, each as csts_stream_stft takes them; column f of
 *        stream i goes to rings[i][bin][f mod ring_cols].  The grid is the total column count.  Refused (-1) before launch: a
 *        column that needs a sample outside its job's buffer, f1 - f0 > ring_cols, n_total > s_base + m, a stream outside
 *        [0, streams), two jobs naming one stream, a first workgroup that is not the running column count.  A job with f1 == f0
 *        is legal and writes nothing; a table of such jobs launches nothing.  1 <= njobs <= 65535.
 *      group_audio_windows: csts_stream_audio_windows with the ring looked up per batch row: rings (streams, nbins, ring_cols),
 *        stream_of int32 [B], newest int64 [streams] = the last column written of every stream (-1: none), centers int64 [B][T] ->
 *        out (B, 1, T, nbins, width).  Row b reads the ring of stream_of[b] under that stream's live span
 *        [max(newest - ring_cols + 1, 0), newest]; a window outside it, or a stream_of outside [0, streams), is NaN and reads
 *        nothing.  width even and <= ring_cols, B * T <= 65535.
 *      group_ingest / group_ingest_yuv: jobs int64 [njobs][6] = {chunk address, chunk bytes, K, H, W, LDS row capacity for that
 *        W}: the chunks several streams pushed, each uint8 (K, H, W, 3) -- or (K, H * 3 / 2, W) in a 4:2:0 layout, the same
 *        layout, matrix and range for all -- of its own size; the row capacity is (3 W + 30) rounded up to 16 (for 4:2:0 the luma
 *        one, (W + 30) rounded up to 16).  params int32 [njobs][5]: the parameter row of each job.  pairs int32 [npairs][3] =
 *        (job, frame in chunk, arena slot): that frame is sampled into arena[slot] by the pixel rule of csts_stream_ingest under
 *        the job's row.  The grid is (ceil(S / 4), npairs), the dynamic LDS that of the widest job (144 KB at W = 6000).  A pair
 *        whose job, frame or arena slot is out of range writes nothing; bad params give a NaN slot; no byte at or past a job's
 *        chunk end is read.  Refused (-1) before launch, per job: a chunk that is null or not 16-byte aligned, W > 6000, chunk
 *        bytes that are not K frames, a row capacity that is not the one W asks for, odd H or W in a 4:2:0 layout.
 *        1 <= njobs, npairs <= 65535, the arena 16-byte aligned.
 *      The clip gather of a group is csts_stream_gather on the arena, R = streams * R, with arena slots. */
int csts_group_stft(const int64_t* jobs, const int64_t* jobs_host, int njobs, float* rings, int streams, int ring_cols, int n_fft,
                    int hop, int win, float eps, hipStream_t stream);
int csts_group_audio_windows(const float* rings, int streams, int ring_cols, const int* stream_of, const int64_t* newest,
                             const int64_t* centers, float* out, int B, int T, int nbins, int width, hipStream_t stream);
int csts_group_ingest(const int64_t* jobs, const int64_t* jobs_host, int njobs, const int* params, const int* pairs, int npairs,
                      float* arena, int64_t arena_slots, int S, const float mean[3], const float std[3], hipStream_t stream);
int csts_group_ingest_yuv(const int64_t* jobs, const int64_t* jobs_host, int njobs, const int* params, const int* pairs, int npairs,
                          float* arena, int64_t arena_slots, int S, const float mean[3], const float std[3], int layout, int matrix,
                          int full_range, hipStream_t stream);

/* ---- live gaze track (csts_amd/csrc/stream.hip, GazeStream(live=...)): a forecast window predicts frames the camera has not
 *      delivered yet, so the track row of a frame can be had the moment the frame arrives.  The track lives in a ring of Rt slots
 *      whose size does not depend on the length of the stream: sum fp32 [Rt][H * W], count int32 [Rt], frame int64 [Rt] = the
 *      frame number a slot holds, -1 when empty; frame t lives in slot t mod Rt.  All in DEVICE memory.
 *      live_track_add: maps [P][H * W] fp32 (the preds of newly run windows) and target_idx int64 [P], walked in ascending p:
 *        t = target_idx[p] < 0:           the row is skipped
 *        frame[t mod Rt] != t:            the slot restarts: sum = 0 + maps[p], count = 1, frame = t (a stale slot is recycled
 *                                         here; there is no clearing pass)
 *        frame[t mod Rt] == t:            sum += maps[p], count += 1
 *      so a slot's sum is (((0 + row_0) + row_1) + ...) over the rows that target its frame, in the order of the calls and in
 *      ascending p inside a call: the sum of csts_gaze_track when the windows are added in the order they ran.  One workgroup
 *      per slot takes the rows of its slot: no atomics, one launch, a slot no row names is not touched.  The caller keeps
 *      targets in window order and never names a target t while frame t - Rt is still to be read (csts_amd.ops.live_track_add
 *      refuses that on the host).  1 <= P <= 65535, 1 <= Rt <= 65535, H * W <= CSTS_GAZE_DECODE_MAX_HW.
 *      live_track_rows: the K frames n = f0 .. f0 + K - 1, one workgroup each.  With c(t) = count[t mod Rt] when t >= 0 and
 *      frame[t mod Rt] == t, else 0 (a slot that holds another frame is empty for t), row n is row n of
 *      csts_gaze_track_fill(mode, max_gap) on the track whose frame t has count c(t) and heatmaps sum * (1 / count), i.e.
 *        c(n) > 0:   neighbours (n, n), m = the mean of frame n
 *        c(n) == 0:  a = the largest t in [n - max_gap + 1, n) with c(t) > 0, b = the smallest t in (n, a + max_gap] with
 *                    c(t) > 0; both exist: neighbours (a, b), m = mean_a (mode 0) or wa * mean_a + wb * mean_b (mode 1, the
 *                    weights and the arithmetic of csts_gaze_track_fill); otherwise neighbours (-1, -1), maps 0, points NaN,
 *                    peak 0
 *        heatmaps = m; rescaled, points, peak from m by the device function csts_gaze_track and csts_gaze_track_fill use;
 *        out_count = c(n).
 *      Outputs heatmaps and rescaled [K][H * W], points [K][2], peak [K] fp32, out_count [K] and neighbours [K][2] int32; each
 *      may be NULL and is then skipped; with all NULL nothing is launched.  The ring is only read.  0 <= f0,
 *      f0 + K + max_gap < 2^31, 1 <= K <= 65535, 1 <= max_gap <= CSTS_GAZE_FILL_MAX_GAP.  128-bit accesses when H * W is a
 *      multiple of 4 and the maps are 16-byte aligned.  One launch each; no allocation, no synchronisation, no host read:
 *      graph-capturable (f0 is a launch argument). */
int csts_live_track_add(const float* maps, const int64_t* target_idx, int P, int H, int W, float* sum, int* count, int64_t* frame,
                        int Rt, hipStream_t stream);
int csts_live_track_rows(const float* sum, const int* count, const int64_t* frame, int Rt, int64_t f0, int K, int H, int W, int mode,
                         int max_gap, float* heatmaps, float* rescaled, float* points, float* peak, int* out_count, int* neighbours,
                         hipStream_t stream);

/* ---- live track of a stream group (csts_amd/csrc/stream.hip, csts_amd.GazeLiveGroup): the track rings of `streams` slots in one
 *      arena, sum fp32 [streams][Rt][H * W], count int32 [streams][Rt], frame int64 [streams][Rt] (-1: empty); frame t of slot i
 *      lives at [i][t mod Rt], and the ring of slot i is exactly the ring csts_live_track_add / csts_live_track_rows work on.  One
 *      launch serves every slot; the tables are DEVICE memory read when the kernel runs, by block index alone (uniform reads); no
 *      atomics, no allocation, no synchronisation, no host read.  The arithmetic is the single-stream kernels' (one device function
 *      each for the slot and for the row): a track slot and a row have the bits they have there.
 *      group_live_add: maps [P][H * W] fp32, target_idx int64 [P], stream_of int32 [P].  Grid (Rt, streams): workgroup (s, i) is
 *        csts_live_track_add's workgroup s on the ring of slot i, restricted to the rows with stream_of[p] == i -- the same two
 *        walks, the same restart / carry-on rule, additions in ascending p.  A row whose stream lies outside [0, streams) or whose
 *        target is negative is ignored; a ring slot no row names is not touched.  The caller never names a target t on slot i
 *        while frame t - Rt of that slot is still to be read (csts_amd.ops.group_live_add refuses that on the host).
 *        1 <= P, Rt, streams <= 65535, streams * Rt < 2^31, H * W <= CSTS_GAZE_DECODE_MAX_HW, maps must not be sum.
 *      group_live_rows: stream_of int32 [K], frame_of int64 [K].  Grid (K): workgroup k answers frame frame_of[k] of slot
 *        stream_of[k] by the rule of csts_live_track_rows on that slot's ring, into row k of the outputs (shapes, NULL outputs and
 *        128-bit accesses as there).  A row whose stream lies outside [0, streams), or whose frame is negative, is the unpredicted
 *        row: maps 0, points NaN, peak 0, count 0, neighbours (-1, -1).  The caller keeps frame_of[k] + max_gap < 2^31
 *        (neighbours are int32; csts_amd.ops.group_live_rows checks the host copy).  1 <= K, Rt <= 65535, 1 <= streams,
 *        streams * Rt < 2^31, mode 0 | 1, 1 <= max_gap <= CSTS_GAZE_FILL_MAX_GAP; no output may be the arena.
 *      Both refuse (-1) before the launch and need no GPU to do so.  Graph-capturable. */
int csts_group_live_add(const float* maps, const int64_t* target_idx, const int* stream_of, int P, int H, int W, float* sum,
                        int* count, int64_t* frame, int streams, int Rt, hipStream_t stream);
int csts_group_live_rows(const float* sum, const int* count, const int64_t* frame, int streams, int Rt, const int* stream_of,
                         const int64_t* frame_of, int K, int H, int W, int mode, int max_gap, float* heatmaps, float* rescaled,
                         float* points, float* peak, int* out_count, int* neighbours, hipStream_t stream);

/* ---- live attention ring (csts_amd/csrc/fusion_maps.hip, GazeStream(live=..., attention=True)): the whole-recording attention
 *      track lands on the frames a window SAW, so when frame n arrives no window that shows n can have run: there is nothing to
 *      fill between.  The live rule is HOLD THE NEWEST MAP: frame n shows the map of the newest frame at most max_age back that
 *      some window that has run did see.  The per-frame sums of csts_attention_track live in a ring of Ra slots whose size does
 *      not depend on the length of the stream: sum fp32 [Ra][heads + 1][h * w], count int32 [Ra], frame int64 [Ra] = the frame a
 *      slot holds, -1 when empty; frame t lives in slot t mod Ra.  All in DEVICE memory.
 *      live_attention_add: column [Wn][heads][T'][h * w] fp32 and frames_idx int64 [Wn][T] of the windows a step ran.  The pairs
 *        p = w T + j are walked in ascending p, each adding m_p of csts_attention_track, for every g in [0, heads], to the slot
 *        of t = frames_idx[p] by the rule of csts_live_track_add:
 *          t < 0:                  the pair is skipped
 *          frame[t mod Ra] != t:   the slot restarts: sum = 0.f + m_p, count = 1, frame = t
 *          frame[t mod Ra] == t:   sum += m_p, count += 1
 *        so a slot's sum is (((0 + m_p0) + m_p1) + ...) over the pairs that land on its frame, in the order of the calls and in
 *        ascending p inside one: the sum of csts_attention_track over the windows added so far, in the order they ran.  ONE
 *        workgroup owns a whole slot -- all (heads + 1) h w cells, the count and the tag: plain loads and stores, no atomics.  A
 *        slot no pair names is not touched.  Input frames do not ascend from window to window (window w + 1's first input lies
 *        before window w's last), so the caller keeps two conditions (csts_amd.ops.live_attention_add refuses what breaks them,
 *        csts_amd.attention_ring_slots sizes the ring for them): a pair never lands on a slot that holds a NEWER frame, and
 *        never on one whose frame is still to be read.  1 <= Wn T <= 65535, 1 <= Ra <= 65535, h, w as csts_attention_track.
 *      live_attention_rows: the K frames n = f0 .. f0 + K - 1; grid (K, heads + 1).  With c(t) = count[t mod Ra] when
 *        frame[t mod Ra] == t, else 0:
 *          g*           = the largest t in [max(0, n - max_age), n] with c(t) > 0
 *          out_frame[k] = g*, or -1 when there is none;  out_count[k] = c(g*), or 0
 *          mixed[k][g]  = sum[g* mod Ra][g] * (1.f / (float)c(g*)): the mean of csts_attention_track
 *          maps[k][g], range[k][g] = csts_attention_rescale of mixed[k][g], by its device functions
 *          none:          mixed and maps 0, range (NaN, NaN)
 *        Row n therefore equals rows g* of csts_attention_track over everything added so far (F = n + 1), bit for bit, as long
 *        as no frame of [n - max_age, n] has been recycled.  mixed, maps [K][heads + 1][h * w], range [K][heads + 1][2] fp32,
 *        out_frame [K] int64, out_count [K] int32; each may be NULL and is then skipped, except that maps and range come
 *        together; with all NULL nothing is launched.  The ring is only read.  f0 >= 0, 1 <= K <= 65535, 0 <= max_age <= 65535.
 *      128-bit accesses when h * w is a multiple of 4 and the buffers are 16-byte aligned.  One launch each; no allocation, no
 *      synchronisation, no host read: graph-capturable.  Both refuse (-1) before the launch and need no GPU to do so.  Added
 *      entry points leave CSTS_ABI_VERSION as it is: no existing signature or struct changes. */
int csts_live_attention_add(const float* column, const int64_t* frames_idx, int Wn, int heads, int Tp, int h, int w, int T, float* sum,
                            int* count, int64_t* frame, int Ra, hipStream_t stream);
int csts_live_attention_rows(const float* sum, const int* count, const int64_t* frame, int Ra, int64_t f0, int K, int heads, int h,
                             int w, int S, int max_age, float* mixed, float* maps, float* range, int64_t* out_frame, int* out_count,
                             hipStream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* CSTS_HIP_H */
