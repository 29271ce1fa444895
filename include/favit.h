/*
 * favit.h -- C ABI of libfavit.so: the MI355X (gfx950 / CDNA4) kernels behind the
 * focused-attention ViT encoder forward/backward hot path.
 *
 * The reference (zser092/Focused-Attention-ViT) has NO native/FFI layer: its hot path
 * is the Python nn.Module surface of models/{vit,mhla,vit_mhla,sppp,sppp_mhla,attention}.py
 * executing aten ops.  This header is the new boundary UNDER that surface: each entry
 * point replaces the aten op sequence of the cited reference lines.  The host-side
 * mirror of the reference classes (the models package of focused-attention-vit_amd) binds these
 * with ctypes (focused-attention-vit_amd/_abi.py); INTEGRATION.md shows the stub.
 *
 * Conventions
 *   - plain pointers + sizes only; every pointer is a DEVICE pointer owned by the caller
 *   - `stream` is a hipStream_t passed as void* (NULL = default stream); all work is
 *     enqueued asynchronously on it, nothing synchronises, nothing allocates
 *   - return 0 on success, a negative FAVIT_ERR_* otherwise; never throws
 *   - dtype codes: FAVIT_F32 (exact fp32 path, f32 MFMA) / FAVIT_BF16 (bf16 operands,
 *     fp32 accumulation, bf16 MFMA) / FAVIT_FP8 (GEMM operands only: OCP e4m3 / e5m2 bytes
 *     with per-tensor scales, fp32 accumulation, fp8 MFMA)
 *   - kernels are stateless and thread-compatible
 *   - focused-attention-vit_amd/_abi.py READS this file and derives the whole ctypes binding from it, so keep its form:
 *     constants as `#define FAVIT_X <integer>` or enumerators with explicit values, structs as
 *     `typedef struct tag { ... } favit_x_t;` with array lengths that are literals or FAVIT_* constants, prototypes
 *     with the scalar types int, int32_t, int64_t, uint32_t, uint64_t and float.  Anything else fails the import.
 */
#ifndef FAVIT_H_
#define FAVIT_H_

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define FAVIT_ABI_VERSION 8
#define FAVIT_FP8_AMAX_SLOTS 256   /* partial maxima per tensor with delayed fp8 scaling (favit_fp8_quantize) */

/* FAVIT_F32X3: valid only as favit_gemm_t.in_dtype (see favit_gemm_t); additive in ABI 8 (the value was
 * FAVIT_ERR_INVALID before). */
enum { FAVIT_F32 = 0, FAVIT_BF16 = 1, FAVIT_FP8 = 2, FAVIT_F32X3 = 3 };
/* OCP 8-bit float formats of gfx950 (NOT the MI300X fnuz encodings) */
enum { FAVIT_E4M3 = 0, FAVIT_E5M2 = 1 };

enum {
  FAVIT_OK = 0,
  FAVIT_ERR_INVALID = -1,     /* bad argument (null pointer, non-positive size, bad enum) */
  FAVIT_ERR_UNSUPPORTED = -2, /* shape/dtype combination this build has no kernel for */
  FAVIT_ERR_ALIGN = -3,       /* pointer / leading dimension alignment requirement violated */
  FAVIT_ERR_LAUNCH = -4       /* hipLaunchKernel reported an error */
};

enum {
  FAVIT_ACT_NONE = 0,
  FAVIT_ACT_GELU = 1,           /* out = GELU(v); aux_out (optional) receives the pre-activation v                   */
  FAVIT_ACT_DGELU = 2,          /* out = v * GELU'(aux_in)            (aux_in = the saved pre-activation)            */
  FAVIT_ACT_GELU_SAVEGRAD = 3,  /* out = GELU(v); aux_out (required) receives GELU'(v) instead of v                  */
  FAVIT_ACT_MULAUX = 4          /* out = v * aux_in                   (aux_in = the saved GELU' of mode 3)           */
};
enum { FAVIT_POOL_MEAN = 0, FAVIT_POOL_MAX = 1, FAVIT_POOL_ATTENTION = 2 };

int favit_abi_version(void);
const char* favit_strerror(int code);

/* Dropout epoch: `device_word` (8-byte aligned device pointer, or NULL to switch the feature off) is read by every
 * kernel that draws a dropout mask -- effective seed = seed + *device_word * 0x9E3779B97F4A7C15 -- at EXECUTION time.
 * A training step captured once in a HIP graph has its dropout seeds frozen into the kernel arguments; with the
 * graph's first node incrementing the word, every replay still draws fresh masks, and the forward and backward
 * kernels of one replay (which recompute the same masks) agree.  Process-wide; the caller owns the word. */
int favit_set_dropout_epoch(const uint64_t* device_word);

/* Health word (v7): `device_words` = four zero-initialised uint32 on the device (16-byte aligned), or NULL to switch
 * it off.  favit_cross_entropy and favit_adamw -- which read every logit row / every gradient and write every
 * parameter anyway -- note the FIRST non-finite value they meet, at no memory traffic and without atomics in a clean
 * run:  [0] flags: 1 = a loss row of an in-range label was non-finite (non-finite logits), 2 = a gradient handed to
 * AdamW was non-finite, 4 = an updated parameter is non-finite;  [1] = (AdamW launches so far) + 1 when bit 1 was
 * first set, [2] = the same for bits 2 | 4, [3] = AdamW launches so far.  bench.py registers one and refuses to print
 * a metric line for a poisoned run; a harness can poll it every N steps without synchronising per step.  Process-wide;
 * the caller owns the words (and keeps them alive while captured HIP graphs hold their address). */
int favit_set_health_word(uint32_t* device_words);

/* ------------------------------------------------------------------------------------
 * GEMM with fused epilogue: every nn.Linear on the path and the dense QK^T / attn.V
 * contractions.   C[m,n] = epilogue( alpha * sum_k A[m,k] * B[n,k] )
 *   replaces: aten::addmm / mm / bmm behind models/vit.py:40,72,74,95,100,119,121,252,
 *             models/mhla.py:37,38, models/attention.py:30-33,63,75,131,144 and their
 *             autograd backward (dX = dY.W, dW = dY^T.X, db = colsum dY).
 * Operand layouts ("kmajor" = the contraction index is contiguous in memory):
 *   a_kmajor=1: A[m*lda + k]   a_kmajor=0: A[k*lda + m]
 *   b_kmajor=1: B[n*ldb + k]   b_kmajor=0: B[k*ldb + n]
 *   forward  Y = X.W^T      : A=X (kmajor), B=W (kmajor)
 *   dX = dY.W               : A=dY (kmajor), B=W with b_kmajor=0
 *   dW = dY^T.X             : A=dY with a_kmajor=0, B=X with b_kmajor=0, K = tokens
 * Epilogue order: v=alpha*acc; v+=bias[n]; aux_out=v; act; dropout; v+=residual; C (=|+=) v.
 *   act=GELU: v=gelu_erf(v) (models/vit.py:135); act=DGELU: v*=gelu'(aux_in[m,n]).
 *   dropout_p>0: v = keep(seed, m*N+n) ? v/(1-p) : 0  (nn.Dropout sites models/vit.py:102,
 *   136,138, models/mhla.py:159; the same (seed,index) draw is reused by the backward GEMMs).
 *   keep(seed, i): one 32-bit counter-based draw per element PAIR (i >> 1); element i takes its low (i even) or high
 *   16 bits and is kept when they are >= floor(p * 65536) -- p is realised to 1 / 65536, in every kernel of the library.
 * accumulate=1 (or split_k>1) adds into C with fp32 atomics; C must then be FAVIT_F32.
 * a_rowsum (a_kmajor=0 only): a_rowsum[m] += sum_k A[m,k]  (bias gradient, fused).
 * Batched: z in [0,batch): ptr += (z / batch_inner) * s?o + (z % batch_inner) * s?i.
 * in_dtype = FAVIT_FP8: A and B hold fp8 bytes (a_fp8_fmt / b_fp8_fmt = FAVIT_E4M3 | FAVIT_E5M2; B must
 *   be E4M3), both k-major, K a multiple of 64 and 16-byte aligned rows, batch = 1; the true operands
 *   are A*scale_a[0] and B*scale_b[0] (device scalars written by favit_fp8_quantize, NULL = 1), i.e.
 *   v = alpha*scale_a*scale_b*acc.  aux_in (DGELU) is bf16 in this mode.
 * in_dtype = FAVIT_F32X3: operands are fp32 in memory and out_dtype is FAVIT_F32, exactly as for FAVIT_F32; only
 *   the inner product differs.  It is the three-pass split product on the bf16 MFMA:
 *       hi = bf16_rne(x),  lo = bf16_rne(x - float(hi))          (round to nearest even, both parts)
 *       acc += hi_a*hi_b + hi_a*lo_b + lo_a*hi_b                 (fp32 MFMA accumulators)
 *   The dropped lo_a*lo_b term and the residual of the split are ~2^-17 relative: rel-L2 against an fp64 product
 *   about 4e-6 at every K, against 4e-7 for FAVIT_F32.  Epilogue, a_rowsum (which sums the UNSPLIT fp32 values),
 *   split_k and accumulate behave as for FAVIT_F32.  It is a request, not a guarantee: a problem the split kernel
 *   does not cover (batched, K not a multiple of 16, operands not 16-byte aligned, too few tiles to fill the
 *   device) runs the exact-fp32 kernel it runs under FAVIT_F32, which is never less accurate;
 *   favit_gemm_last_kernel() says which one ran.
 * ---------------------------------------------------------------------------------- */
typedef struct favit_gemm_t {
  const void* A;
  const void* B;
  void* C;
  const float* bias;     /* [N] fp32 or NULL */
  const void* aux_in;    /* DGELU: pre-activation [M,N], dtype = in_dtype; else NULL */
  void* aux_out;         /* optional copy of the pre-activation [M,N], dtype = out_dtype */
  const float* residual; /* [M,N] fp32 or NULL */
  float* a_rowsum;       /* [M] fp32 or NULL */
  int64_t M, N, K;
  int64_t lda, ldb, ldc, ld_aux_in, ld_aux_out, ld_res;
  int64_t sAo, sAi, sBo, sBi, sCo, sCi; /* batch strides in elements */
  int32_t batch, batch_inner;
  int32_t a_kmajor, b_kmajor;
  int32_t in_dtype, out_dtype;
  int32_t act;
  int32_t accumulate;
  int32_t split_k; /* 0 = library decides */
  float alpha;
  float dropout_p;
  int32_t fp8_fmt;        /* FAVIT_FP8 only: bit 0 = A is E5M2, bit 1 = B is E5M2 (unsupported) */
  uint64_t dropout_seed;
  const float* scale_a;   /* FAVIT_FP8 only: device scalars (dequantisation factors) or NULL */
  const float* scale_b;
} favit_gemm_t;

int favit_gemm(const favit_gemm_t* g, void* stream);
/* Diagnostic: the kernel family ("p4" 256x128 tiles, "p7" 256x256, "pp" ping-pong, "s64" 64-row, "t128"
 * 128x128 / exact-fp32, "p4f" / "p4f128" the exact-fp32 DMA kernel with 256- / 128-row tiles, "p4x3" / "p4x3_128"
 * the FAVIT_F32X3 split-bf16 form of those two) the calling host thread's last favit_gemm dispatched to.  Static
 * string, never NULL. */
const char* favit_gemm_last_kernel(void);

/* LayerNorm fused into a small-M forward GEMM (v7):  C = epilogue( LN(x; gamma, beta, eps) . B^T )  in ONE launch, for
 * the short-token configurations where a block's forward is a chain of 5-15 us launches.  `g` describes the GEMM as for
 * favit_gemm with A ignored: bf16 k-major weights B [N, K], K = the LayerNorm width (a multiple of 64, <= 512, not 320 /
 * 448), every epilogue of favit_gemm (bias, GELU variants, dropout, residual), no split-K / batch / accumulate.
 * x: fp32 rows of ldx.  Also written: xn [M, K] bf16 (the normalised rows, the A operand of the weight-gradient GEMM),
 * mean [M], rstd [M] (fp32) for favit_layernorm_bwd.  Same arithmetic as favit_layernorm_fwd followed by favit_gemm
 * (two-pass variance, bf16 rounding of xn before the product); FAVIT_ERR_UNSUPPORTED for other shapes / dtypes (the
 * caller then issues the two launches). */
int favit_ln_gemm(const favit_gemm_t* g, const float* x, int64_t ldx, const float* gamma, const float* beta, float eps,
                  void* xn, float* mean, float* rstd, void* stream);

/* Grouped weight-gradient GEMMs: `count` (<= 48) problems dW_i = dY_i^T . X_i that share the token
 * dimension K (the four nn.Linear layers of one transformer block, or of several consecutive blocks) as
 * ONE launch.  Every problem must be bf16 in / fp32 out with a_kmajor = b_kmajor = 0, no epilogue other
 * than a_rowsum (bias gradient, always ADDED to its destination) and accumulate; returns
 * FAVIT_ERR_UNSUPPORTED otherwise (the caller then issues them one by one).  The number of K-splits is
 * chosen by a cost model (v7): with enough tiles in the launch it is 1, and then no workspace is used. */
#define FAVIT_GEMM_GROUP_MAX 48   /* problems per grouped launch, plain or ragged */
int favit_gemm_grouped_tn(const favit_gemm_t* gs, int32_t count, void* stream);
/* The same launch with a caller-provided device workspace of favit_gemm_grouped_tn_workspace(gs, count) bytes:
 * every K-split writes its partial results to a slab of the workspace with plain stores and a second kernel adds
 * the slabs in a fixed order (no fp32 atomics: faster -- atomics run at ~1.3 TB/s chip-wide -- and bitwise
 * reproducible).  A NULL / too small workspace falls back to the atomic path. */
int64_t favit_gemm_grouped_tn_workspace(const favit_gemm_t* gs, int32_t count);
int favit_gemm_grouped_tn_ws(const favit_gemm_t* gs, int32_t count, void* workspace, int64_t workspace_bytes,
                             void* stream);
/* The grouped launch for problems whose token counts (K) differ -- the blocks of a pruned encoder.  Consecutive
 * problems of one K with at most 64 tiles together form a chunk; every chunk gets its own number of K-splits.  Chunks
 * with one split write dW from the tile epilogue, the others go through per-chunk slabs of the workspace
 * (favit_gemm_grouped_tn_ragged_workspace bytes; 0 when no chunk is split, and then no reduction kernel runs) that a
 * second kernel adds in split order.  Every K must be a positive multiple of 32.  A workspace smaller than the query's
 * answer is FAVIT_ERR_INVALID; without a workspace (the first form) split chunks add with fp32 atomics.  A group with
 * one K gets exactly the plan and the result of favit_gemm_grouped_tn*.  Nothing is launched when a call is refused. */
int favit_gemm_grouped_tn_ragged(const favit_gemm_t* gs, int32_t count, void* stream);
int64_t favit_gemm_grouped_tn_ragged_workspace(const favit_gemm_t* gs, int32_t count);
int favit_gemm_grouped_tn_ragged_ws(const favit_gemm_t* gs, int32_t count, void* workspace, int64_t workspace_bytes,
                                    void* stream);
/* Diagnostic: K-splits of the calling host thread's last grouped launch (1 = tiles wrote dW directly); after a ragged
 * launch the largest split count among its chunks. */
int favit_gemm_grouped_last_splits(void);
/* Diagnostic, host only (nothing is launched): the chunks, per-chunk K-splits and per-XCD unit queues a grouped launch
 * of these problems gets (ragged != 0: the plan of favit_gemm_grouped_tn_ragged).  out (cap values) receives
 * {nchunks, units, longest queue in tiles, workspace bytes}, per chunk {first problem, tiles, K, splits, tokens per
 * split}, per queue {n, unit ids}; returns the number of values written or a negative FAVIT_ERR_*. */
int favit_gemm_grouped_plan(const favit_gemm_t* gs, int32_t count, int32_t ragged, int64_t* out, int32_t cap);

/* ------------------------------------------------------------------------------------
 * FP8 operand preparation (BASELINE.json configs[3] "fp8 MFMA path"; no reference counterpart:
 * the reference is fp32 only).  Per-tensor scaling, computed on the device:
 *   favit_fp8_amax:     amax[0] = max(amax[0], max |src[i]|)   (caller zeroes amax first)
 *   favit_fp8_quantize: q = sat(src * fmax / amax[0]) in OCP e4m3 (fmax 448) or e5m2 (fmax 57344),
 *                       round-to-nearest-even; scale_inv[0] = amax / fmax (the GEMM's scale_a/b).
 *     dst   [rows, ld_dst]   same orientation as src (NULL to skip)
 *     dst_t [cols, ld_t]     transposed copy (NULL to skip); columns rows..ld_t-1 are zero-filled,
 *                            so ld_t (a multiple of 64) can serve as a padded GEMM K
 *     colsum [cols] fp32     optional: colsum[c] += sum_r src[r,c] (bias gradient of an fp8 Linear)
 *     amax_next, amax_clear  optional, both or neither (delayed scaling).  Then amax, amax_next and amax_clear are
 *                            three DIFFERENT arrays of FAVIT_FP8_AMAX_SLOTS floats (rotating roles): the scale comes
 *                            from max(amax[0..]) -- what this site's previous call measured --, max |src| is taken in
 *                            the same pass into amax_next (atomics spread over the slots), amax_clear is zeroed
 *                            for the call after next.  No separate favit_fp8_amax pass.
 * src dtype is FAVIT_F32 or FAVIT_BF16, row stride ld_src (elements).
 * ---------------------------------------------------------------------------------- */
int favit_fp8_amax(const void* src, int src_dtype, int64_t rows, int64_t cols, int64_t ld_src, float* amax,
                   void* stream);
int favit_fp8_quantize(const void* src, int src_dtype, int64_t rows, int64_t cols, int64_t ld_src, void* dst,
                       int64_t ld_dst, void* dst_t, int64_t ld_t, int fmt, const float* amax, float* scale_inv,
                       float* colsum, float* amax_next, float* amax_clear, void* stream);

/* dst[i] = (dst_dtype) src[i] */
int favit_cast(const void* src, int src_dtype, void* dst, int dst_dtype, int64_t n, void* stream);

/* ------------------------------------------------------------------------------------
 * LayerNorm over the last dim (nn.LayerNorm, eps 1e-5, biased variance):
 *   models/vit.py:155,157,251; models/vit_mhla.py:45,64,88,107,188,241.
 * x is the fp32 residual stream with row stride ldx (lets the head normalise x[:,0]
 * only); y has dtype y_dtype; mean/rstd [rows] are saved for backward.
 * Backward: dx = LN'(dy) (+ dres if given); dres is read with the SAME row stride as dx is written with (lddx), so
 * a strided dx takes an equally strided dres; optional low-precision copy dx_lp ([rows, D] contiguous, the
 * dtype of dy), optionally with the dropout mask (lp_dropout_p, lp_dropout_seed; element index row*D + col, as
 * favit_dropout) of the branch it feeds; dx itself is never masked; the
 * affine gradients are produced as `nparts` partial sums in a [2][nparts][D] workspace
 * (dbeta_part = dgamma_part + nparts*D) and folded into dgamma[D] and dbeta[D]: deterministically (no atomics)
 * with accumulate=0, ADDED to them with the rows split eight ways and fp32 atomics with accumulate=1;
 * dgamma = NULL skips the fold (the caller folds the workspace later, favit_reduce_rows_multi, or not at all).
 * ---------------------------------------------------------------------------------- */
int favit_layernorm_fwd(const float* x, int64_t ldx, const float* gamma, const float* beta, void* y, int y_dtype,
                        float* mean, float* rstd, int64_t rows, int32_t D, float eps, void* stream);
int favit_layernorm_bwd(const void* dy, int dy_dtype, const float* x, int64_t ldx, const float* gamma,
                        const float* mean, const float* rstd, const float* dres, float* dx, int64_t lddx,
                        void* dx_lp, int lp_dtype, float* dgamma_part, float* dbeta_part, int32_t nparts,
                        float* dgamma, float* dbeta, int32_t accumulate, int64_t rows, int32_t D,
                        float lp_dropout_p, uint64_t lp_dropout_seed, void* stream);
/* fp8 mode (ABI 8): the same two passes, the bf16 tensor they write (y / dx_lp) ALSO leaving as fp8 in q [rows, D]
 * (fmt = FAVIT_E4M3 | FAVIT_E5M2) with delayed scaling -- amax / scale_inv / amax_next / amax_clear exactly as in
 * favit_fp8_quantize (three different arrays of FAVIT_FP8_AMAX_SLOTS floats; all required).  Bytes, scale and
 * history are bit-identical to favit_layernorm_* followed by favit_fp8_quantize on the bf16 tensor; the stand-alone
 * pass (one read of the tensor + one write) is what is saved.  y and dy / dx_lp are bf16 here.  No reference
 * counterpart (the reference is fp32 only); consumers: the fp8 GEMMs of BASELINE.json configs[3]. */
int favit_layernorm_fwd_q8(const float* x, int64_t ldx, const float* gamma, const float* beta, void* y, float* mean,
                           float* rstd, int64_t rows, int32_t D, float eps, void* q, int fmt, const float* amax,
                           float* scale_inv, float* amax_next, float* amax_clear, void* stream);
int favit_layernorm_bwd_q8(const void* dy, const float* x, int64_t ldx, const float* gamma, const float* mean,
                           const float* rstd, const float* dres, float* dx, int64_t lddx, void* dx_lp,
                           float* dgamma_part, float* dbeta_part, int32_t nparts, float* dgamma, float* dbeta,
                           int32_t accumulate, int64_t rows, int32_t D, float lp_dropout_p, uint64_t lp_dropout_seed,
                           void* q, int fmt, const float* amax, float* scale_inv, float* amax_next, float* amax_clear,
                           void* stream);
/* The classification head as exact-fp32 dot products (ABI 8): y[M,N] = x[M,K] (row stride ldx) . w[N,K]^T + bias, and its
 * backward dx[M,K] (NULL: skipped) = dy . w, dw[N,K] (+)= dy^T . x, db[N] (NULL: skipped) (+)= column sums of dy
 * (accumulate = 1 adds to dw / db).  N <= 64 (FAVIT_ERR_UNSUPPORTED beyond: those heads are GEMMs); no atomics.
 * Reference: nn.Linear(embed_dim, num_classes) on the normalised CLS row, models/vit.py:259,306,
 * models/vit_mhla.py:156,249, models/sppp_mhla.py:240,318. */
#define FAVIT_SMALL_LINEAR_MAX_N 64
int favit_small_linear_fwd(const float* x, int64_t ldx, const float* w, const float* bias, float* y, int32_t M, int32_t N,
                           int32_t K, void* stream);
int favit_small_linear_bwd(const float* dy, const float* x, int64_t ldx, const float* w, float* dx, float* dw, float* db,
                           int32_t accumulate, int32_t M, int32_t N, int32_t K, void* stream);
/* out[c] (+)= sum_r in[r*ld + c] */
int favit_reduce_rows(const float* in, int64_t ld, float* out, int64_t rows, int32_t cols, int32_t accumulate,
                      void* stream);
#define FAVIT_REDUCE_ROWS_MULTI_MAX 32   /* entries per favit_reduce_rows_multi / _multi_ragged launch */
/* n (<= 32) stacked-pair reductions in ONE launch: entry e adds the column sums of in[e] ([2][rows][cols], contiguous)
 * to out0[e] / out1[e] ([cols] each).  Used for the dgamma / dbeta partials of several favit_layernorm_bwd calls
 * (each called with dgamma = NULL): the arguments are HOST arrays of n device pointers. */
int favit_reduce_rows_multi(int32_t n, const float* const* in, float* const* out0, float* const* out1, int64_t rows,
                            int32_t cols, void* stream);
/* The same for entries of different row counts in ONE launch: rows is a HOST array of n row counts, cols is shared.
 * Every entry keeps the row split (rows >= 512: eight ways) and the summation order it has in a launch of its own. */
int favit_reduce_rows_multi_ragged(int32_t n, const float* const* in, float* const* out0, float* const* out1,
                                   const int64_t* rows, int32_t cols, void* stream);

/* ------------------------------------------------------------------------------------
 * MHLA (models/mhla.py).  latent_proj (mhla.py:41,105-106) is one Linear(hd,hd) shared
 * by K, V and all heads; it is folded algebraically into the qkv projection:
 *   Weff[s,h] = Wl . Wqkv[s,h] , beff[s,h] = Wl . bqkv[s,h] + bl   for s in {k,v}
 * so that one GEMM produces q, k~, v~.  fold_bwd maps the gradients of (Weff, beff)
 * back to the real parameters qkv.{weight,bias} and latent_proj.{weight,bias}.
 * ---------------------------------------------------------------------------------- */
int favit_mhla_fold_fwd(const float* wqkv, const float* bqkv, const float* wl, const float* bl, void* weff,
                        int weff_dtype, float* weff_f32 /* optional fp32 copy */, float* beff, int32_t D,
                        int32_t H, void* stream);
/* accumulate=1: the four outputs are added to (gradient buffers), else overwritten */
#define FAVIT_FOLD_MAX 32       /* blocks per favit_mhla_fold_fwd_multi launch */
#define FAVIT_FOLD_BWD_MAX 16   /* layers per favit_mhla_fold_bwd_multi launch */
/* The forward fold of n (<= 32) independent blocks -- e.g. every layer of an encoder -- in ONE launch.
 * The arguments are HOST arrays of n device pointers; weff[i] / beff[i] as in favit_mhla_fold_fwd. */
int favit_mhla_fold_fwd_multi(int32_t n, const float* const* wqkv, const float* const* bqkv, const float* const* wl,
                              const float* const* bl, void* const* weff, int weff_dtype, float* const* beff,
                              int32_t D, int32_t H, void* stream);

int favit_mhla_fold_bwd(const float* dweff, const float* dbeff, const float* wqkv, const float* bqkv,
                        const float* wl, float* dwqkv, float* dbqkv, float* dwl, float* dbl, int32_t D, int32_t H,
                        int32_t accumulate, void* stream);
/* The backward fold of n (<= 16) layers in ONE launch, always ACCUMULATING into the gradient buffers (HOST arrays of n
 * device pointers, as favit_mhla_fold_fwd_multi).  dwqkv[i] = dbqkv[i] = NULL for every layer: frozen qkv projection
 * (the fine-tuning setup of experiments/sppp_mhla_pretrained.py:236-247), only dwl / dbl are produced. */
int favit_mhla_fold_bwd_multi(int32_t n, const float* const* dweff, const float* const* dbeff, const float* const* wqkv,
                              const float* const* bqkv, const float* const* wl, float* const* dwqkv,
                              float* const* dbqkv, float* const* dwl, float* const* dbl, int32_t D, int32_t H,
                              void* stream);

/* Windowed attention core: window index rule (mhla.py:46-83, closed form in-kernel, the
 * duplicated pad indices take part in the softmax), gather (117-126, never materialised),
 * scores / sqrt(hd) (130-133), optional mask[B,L,L]!=0 keep (136-143), softmax + dropout
 * (146-147), attn.V (151-154), head merge (157).  qkv is the [B*L, 3D] output of the folded
 * projection (column = s*D + h*hd + d); out is [B*L, D] (column = h*hd + d).
 * Backward recomputes the probabilities and writes dqkv [B*L, 3D].
 * mask: one byte per (b, query, key), any non-zero byte keeps the key; NULL = no mask.
 * A query row whose window keys are ALL masked (PyTorch's softmax gives NaN there; ordinary with a padding mask
 * mask[b, :, j] = j < n_b: the rows n_b + W/2 <= i < L - W/2, the last W/2 rows keep the pad copies of key 0 in
 * their windows) follows the contract of favit_sdpa_fwd below: its row of out is 0
 * (and its lse, where the forward leaves one, is -inf), and in bwd it gets dq = 0 and adds nothing to dk or dv.  No
 * other row is affected and nothing non-finite is written.  A masked slot of a live row has P = 0 exactly.  This
 * holds for both pairs of entry points below, in every dtype, head size and kernel selection. */
int favit_mhla_attn_fwd(const void* qkv, void* out, const uint8_t* mask, int32_t B, int32_t L, int32_t H,
                        int32_t hd, int32_t W, int dtype, float dropout_p, uint64_t seed, void* stream);
int favit_mhla_attn_bwd(const void* qkv, const void* dout, void* dqkv, const uint8_t* mask, int32_t B, int32_t L,
                        int32_t H, int32_t hd, int32_t W, int dtype, float dropout_p, uint64_t seed,
                        void* stream);
/* The same attention core with the forward's softmax statistics handed to backward (ABI 6): `lse` fp32 [B, H, L] =
 * log sum_w exp(s_w) of every row's window (pad copies counted, mask applied), `o` = the forward's output.  With them
 * backward recomputes no softmax for rows outside a workgroup's block (P = exp(s - lse); delta = dO . O for the halo
 * rows: o is in bf16, so delta of those rows carries its rounding, ~2^-9 relative) -- the cfg2 launch takes 66 us
 * against 79.  favit_mhla_attn_lse_supported: 1 where both entry points run (bf16, hd = 64, odd W <= 7, or <= 11 with
 * L > 16; L >= W + 1), else the callers use the pair above.
 * A query row whose window keys are all masked (contract above): fwd writes o = 0 and lse = -inf for it, and bwd,
 * given that pair, gives it dq = 0 and adds nothing to dk or dv (P = 0 on every slot, delta = dO . 0 = 0). */
int favit_mhla_attn_lse_supported(int32_t L, int32_t hd, int32_t W, int dtype);
int favit_mhla_attn_fwd_lse(const void* qkv, void* out, float* lse, const uint8_t* mask, int32_t B, int32_t L, int32_t H,
                            int32_t hd, int32_t W, int dtype, float dropout_p, uint64_t seed, void* stream);
int favit_mhla_attn_bwd_lse(const void* qkv, const void* dout, const void* o, const float* lse, void* dqkv,
                            const uint8_t* mask, int32_t B, int32_t L, int32_t H, int32_t hd, int32_t W, int dtype,
                            float dropout_p, uint64_t seed, void* stream);

/* ------------------------------------------------------------------------------------
 * Row softmax for the dense attention variants (models/vit.py:96, attention.py:71,140,
 * nn.MultiheadAttention): S fp32 [Z, Lq, Lk] (already scaled by the GEMM alpha).
 * mask (uint8, 0 = -inf) is addressed mask[(z / H) * m_sb + q * m_sq + k].
 * P (dtype p_dtype) gets softmax(S); if dropout_p>0, Pd gets the dropped+rescaled P.
 * Backward: dS = P * (dPd*keep/(1-p) - sum_k(...)) in ds_dtype.
 * dropout: inverted, counter-based on (seed, (z*Lq + q)*Lk + k) -- with z = b*H + h the draw of favit_sdpa_fwd.
 * A row whose keys are ALL masked (PyTorch's softmax gives NaN there) follows the contract of favit_sdpa_fwd below:
 * fwd stores P = 0 (and Pd = 0) for the whole row, so the P.V GEMM gives o = 0 for it; bwd then gives dS = 0 for it
 * (dS = P * (...) with P = 0 and finite dPd), so dq = 0 and the row adds nothing to dk or dv.  No other row is
 * affected and nothing non-finite is written.  A masked entry of a live row has P = 0 exactly.
 * ---------------------------------------------------------------------------------- */
int favit_softmax_fwd(const float* S, void* P, void* Pd, int p_dtype, const uint8_t* mask, int64_t m_sb,
                      int64_t m_sq, int32_t H, int64_t Z, int32_t Lq, int32_t Lk, float dropout_p, uint64_t seed,
                      void* stream);
int favit_softmax_bwd(const void* P, int p_dtype, const float* dPd, void* dS, int ds_dtype, int64_t Z, int32_t Lq,
                      int32_t Lk, float dropout_p, uint64_t seed, void* stream);

/* ------------------------------------------------------------------------------------
 * Device-side input transforms (reference utils/data_utils.py:21-81): crop (+ zero padding) ->
 * optional flip -> Pillow-exact bilinear resize (8-bit two-pass resampling, 22-bit fixed-point coefficients:
 * bit-identical to PIL.Image.resize(BILINEAR), which is what torchvision's Resize / RandomResizedCrop run on PIL
 * images) -> output window -> ToTensor (/255) -> Normalize, for a batch of raw uint8 HWC images on the device.
 *   src [B,Hs,Ws,C] uint8; params int32 [B,12] (device) = crop top, left, h, w (in the padded source), pad,
 *   resized h, w, window origin y, x, flip_src, flip_out, 0; tmp uint8 [B,ch_max,S,C] workspace (ch_max >= every
 *   crop height); out fp32 [B,C,S,S]; out_u8 (optional) the resized bytes [B,S,S,C]; mean / std: HOST arrays [C].
 * ---------------------------------------------------------------------------------- */
int favit_image_transform(const uint8_t* src, uint8_t* tmp, float* out, uint8_t* out_u8, const int32_t* params, int32_t B,
                          int32_t Hs, int32_t Ws, int32_t C, int32_t ch_max, int32_t S, const float* mean,
                          const float* std, void* stream);
/* The same transform for a batch of images of DIFFERENT sizes (a folder of photographs): src is one packed uint8
 * buffer of HWC images laid back to back, src_desc int64 [B,3] (device) = byte offset, Hs, Ws of each image.  params,
 * out, out_u8, mean, std and every byte of arithmetic are those of favit_image_transform (only the horizontal pass
 * reads the source); reads outside [0,Hs) x [0,Ws) of an image are zero padding, never bytes of its neighbour.
 * tmp: uint8 [B,ch_max,S,C] workspace = B * ch_max * S * C bytes, ch_max >= every crop height (params[:,2]).
 * The descriptors are device memory and are NOT validated here: the caller guarantees
 * 0 <= offset and offset + Hs*Ws*C <= size of src for every row (data.py checks its host arrays before the upload). */
int favit_image_transform_ragged(const uint8_t* src, const int64_t* src_desc, uint8_t* tmp, float* out,
                                 uint8_t* out_u8, const int32_t* params, int32_t B, int32_t C, int32_t ch_max,
                                 int32_t S, const float* mean, const float* std, void* stream);

/* ------------------------------------------------------------------------------------
 * SLIC superpixels on the device: replaces the per-image D2H -> skimage.segmentation.slic -> H2D
 * hop of SuperpixelSegmentation.segment (reference models/sppp.py:44-74).  scikit-image is an unpinned third-party
 * dependency absent from the image: parity with skimage is UNPINNED; the algorithm (csrc/slic.hip header) is the
 * published SLIC as skimage parametrises it, integer-exact after the colour conversion, and is checked against
 * the CPU restatement oracle/slic_oracle.py.
 *   features: img fp32 [B,3,H,W] -> feat int16 [B,H*W,4] = round(16 * CIELAB(gaussian_sigma(rescale(img)))) clamped to +-8191, lane 3 = 0;
 *             rescale != 0: every image is first rescaled to [0, 1] by its own minimum and maximum over all channels,
 *             as scikit-image >= 0.19 does before smoothing (the reference passes mean/std-normalised tensors,
 *             models/sppp_mhla.py:278); 0 = no rescale (scikit-image < 0.19).  ws: device workspace of
 *             favit_slic_features_workspace(B, H, W) bytes (min / max per image and the horizontal pass of the
 *             separable gaussian)
 *   cluster : (feat values must lie in [-8191, 8191], as `features` produces them: the distance arithmetic relies on it)
 *             k-means, K <= 64 centres seeded at init_yx [K,2] (int32 y, x), window +-2*step, distance
 *             256*spatial^2 + coef*dq^2 (int64), `iters` rounds -> labels uint8 [B,H*W]; ws: 8-byte aligned device
 *             workspace of favit_slic_cluster_workspace(K, B) bytes (per-centre sums and coordinates)
 *   connect : 4-connected components in raster order, components < min_size merged into a labelled neighbour,
 *             consecutive labels from 0 -> out int64 [B,H*W]; n_regions int32 [B] (-1: more than 2048 components,
 *             out = the cluster map); ws_comp / ws_aux: int32 [B,H*W] workspaces.
 * ---------------------------------------------------------------------------------- */
int64_t favit_slic_features_workspace(int32_t B, int32_t H, int32_t W);
int favit_slic_features(const float* img, int16_t* feat, int32_t B, int32_t H, int32_t W, float sigma, int32_t rescale,
                        float* ws, void* stream);
int64_t favit_slic_cluster_workspace(int32_t K, int32_t B);
int favit_slic_cluster(const int16_t* feat, uint8_t* labels, const int32_t* init_yx, int32_t K, int32_t B, int32_t H,
                       int32_t W, int32_t step, int64_t coef, int32_t iters, void* ws, void* stream);
int favit_slic_connect(const uint8_t* labels, int32_t* ws_comp, int32_t* ws_aux, int64_t* out, int32_t* n_regions,
                       int32_t B, int32_t H, int32_t W, int32_t min_size, void* stream);

/* ------------------------------------------------------------------------------------
 * Fused scaled-dot-product attention for the dense variants (replaces, on one kernel family, the reference's
 *   scores = q @ k^T * scale -> masked_fill(mask == 0, -inf) -> softmax -> dropout -> @ v
 * of models/vit.py:95-100 (MultiHeadAttention), models/attention.py:63-75 (CrossAttention, one head,
 * scale 1/sqrt(embed_dim)) and 131-144 (MultiHeadCrossAttention), and of the nn.MultiheadAttention branch
 * models/vit_mhla.py:57-62).  No [B*H, Lq, Lk] tensor is written to memory.
 * Element (b, h, l, d) of a matrix lives at ptr + b*str[1] + h*str[2] + l*str[0] + d (strides in elements,
 * str = {row stride, batch stride, head stride}; multiples of 16 bytes), so q / k / v can be column blocks of
 * one fused projection output and o / dq / dk / dv are written in place, head-merged.
 * mask (uint8, 0 = -inf, NULL = none) is addressed mask[b*m_sb + q*m_sq + k]  (key-keep [B,Lk]: m_sq = 0).
 * fwd writes o and lse [B*H, Lq] (row log-sum-exp of the scaled, masked scores); bwd needs q, k, v, o, dout,
 * lse and a workspace delta [B*H, Lq], and writes dq, dk, dv (probabilities are recomputed; deterministic).
 * A query row whose keys are ALL masked (PyTorch's softmax gives NaN there): its row of o is 0, its lse is -inf, and
 * in bwd it gets dq = 0 and adds nothing to dk or dv (the recomputed probabilities of masked entries are 0 whatever
 * lse holds, and delta = dO . O = 0); no other row is affected and nothing non-finite is written to o, dq, dk or dv.
 * dropout: inverted, counter-based on (seed, ((b*H + h)*Lq + q)*Lk + k), the same draw in fwd and bwd.
 * dtype FAVIT_BF16 (bf16 MFMA, fp32 accumulate / softmax) or FAVIT_F32 (exact-fp32 MFMA); hd % 16 == 0.
 * ---------------------------------------------------------------------------------- */
typedef struct favit_sdpa {
  const void* q;
  const void* k;
  const void* v;
  void* o;               /* fwd: output; bwd: input */
  float* lse;            /* fwd: output; bwd: input */
  const void* dout;      /* bwd only from here */
  void* dq;
  void* dk;
  void* dv;
  float* delta;
  const uint8_t* mask;
  int64_t m_sb, m_sq;
  int64_t q_str[3], k_str[3], v_str[3], o_str[3], do_str[3], dq_str[3], dk_str[3], dv_str[3];
  int32_t B, H, Lq, Lk, hd, dtype;
  float scale, dropout_p;
  uint64_t seed;
} favit_sdpa_t;
int favit_sdpa_fwd(const favit_sdpa_t* s, void* stream);
int favit_sdpa_bwd(const favit_sdpa_t* s, void* stream);

/* ------------------------------------------------------------------------------------
 * Patch embedding front end.
 * patchify: einops 'b c (h p1) (w p2) -> b (h w) (p1 p2 c)' (models/vit.py:38-39),
 *   img fp32 NCHW -> rows [B*N, P*P*C] of out_dtype (channel fastest).
 * embed_prologue: cat(cls, tokens) + pos_embed (models/vit.py:292-296,
 *   models/vit_mhla.py:229-233); pos may be NULL (SPPP path adds its own encoding).
 * ---------------------------------------------------------------------------------- */
int favit_patchify_fwd(const float* img, void* out, int out_dtype, int32_t B, int32_t C, int32_t HW, int32_t P,
                       void* stream);
int favit_patchify_bwd(const float* dpatch, float* dimg, int32_t B, int32_t C, int32_t HW, int32_t P, void* stream);
int favit_embed_prologue_fwd(const float* tok, const float* cls, const float* pos, float* x, int32_t B, int32_t N,
                             int32_t D, void* stream);
/* dtok (dtype dtok_dtype, [B*N, D], feeds the patch-embedding weight-gradient GEMM), dcls, dpos may be NULL */
int favit_embed_prologue_bwd(const float* dx, void* dtok, int dtok_dtype, float* dcls, float* dpos, int32_t B,
                             int32_t N, int32_t D, void* stream);

/* Row cut of the fp32 residual stream (CLS-only encoders: only the token rows the CLS head can see are computed,
 * DESIGN.md section 9).  Every image keeps its first a and its last b rows, stored one after the other; a + b <= n_in.
 * fwd: y[B, a + b, D] from x[B, n_in, D].
 * bwd: dx[B, n_in, D] = dy[B, a + b, D] scattered back with zeros in the cut rows (written by the kernel itself);
 *      dx_lp (may be NULL; lp_dtype FAVIT_F32 or FAVIT_BF16) receives the same values in the compute dtype. */
int favit_rows_cut_fwd(const float* x, float* y, int32_t B, int32_t n_in, int32_t a, int32_t b, int32_t D, void* stream);
int favit_rows_cut_bwd(const float* dy, float* dx, void* dx_lp, int lp_dtype, int32_t B, int32_t n_in, int32_t a,
                       int32_t b, int32_t D, void* stream);

/* ------------------------------------------------------------------------------------
 * One MHLA encoder block per call (additive in ABI 8): the kernel chain of a pre-LN block
 *   x1 = x + proj(attn(qkv(LN1(x))));  x2 = x1 + fc2(gelu(fc1(LN2(x1))))        (models/mhla.py:205-222)
 * in bf16 compute without mask or dropout, issued by ONE host call per direction.  The calls below launch nothing of
 * their own: they go through favit_layernorm_fwd / _bwd, favit_gemm and the favit_mhla_attn_*_lse pair with the
 * arguments a caller issuing the nine launches one by one would pass, so results are bit-identical to that sequence.
 * Everything the forward leaves for the backward lives in ONE caller-owned device allocation, the tape; the
 * backward's intermediate and result buffers in a second one.  Both are carved by the layout queries (pure host
 * arithmetic; every offset a multiple of 256 bytes; slots in the order of the enums' names below):
 *   tape:  xn1 bf16 [M, D], mu1, rs1 fp32 [M], qkv bf16 [M, 3D], o bf16 [M, D], lse fp32 [B, H, n] (empty unless
 *          training), x1 fp32 [M, D], xn2 bf16 [M, D], mu2, rs2 fp32 [M], h, pre bf16 [M, hidden], x2 fp32 [M, D]
 *          (M = B * n; x2 is the block's output)
 *   bwd:   dpre bf16 [M, hidden], dxn2 bf16 [M, D], g1_f32 fp32 / g1_lp bf16 [M, D] (the stream gradient between the
 *          two branches), do bf16 [M, D], dqkv bf16 [M, 3D], dxn1 bf16 [M, D], g_out_f32 fp32 / g_out_lp bf16 [M, D]
 *          (the gradient of x; g_out_lp empty unless want_lp_out), part1, part2 fp32 [2, nparts, D] (dgamma / dbeta
 *          partial sums of LayerNorm 1 / 2, nparts = min(2048, (M + 3) / 4); NOT folded here: the caller runs
 *          favit_reduce_rows_multi over them)
 * The layout queries return the total size in bytes, or a negative FAVIT_ERR_* for a geometry the chains do not take:
 * D a multiple of 64 with D / H == 64, hidden a multiple of 8, and (n, W) accepted by favit_mhla_attn_lse_supported.
 * fwd / bwd validate every argument BEFORE the first launch (null pointers, a tape / bwd allocation smaller than its
 * layout or not 256-byte aligned, the geometry above; bwd also needs training != 0): on such a return nothing has
 * been launched and the caller issues the launches itself.  A failing launch returns that entry point's code at once.
 * Not part of the chain: weight gradients (dW = dY^T . X from dpre / dqkv / g_lp / g1_lp and the tape), the
 * latent_proj fold, the fold of part1 / part2 and the row cuts.
 * ---------------------------------------------------------------------------------- */
#define FAVIT_BLOCK_TAPE_SLOTS 13
#define FAVIT_BLOCK_BWD_SLOTS 11
enum {   /* index of every tape slot in offsets_out */
  FAVIT_TAPE_XN1 = 0, FAVIT_TAPE_MU1 = 1, FAVIT_TAPE_RS1 = 2, FAVIT_TAPE_QKV = 3, FAVIT_TAPE_O = 4, FAVIT_TAPE_LSE = 5,
  FAVIT_TAPE_X1 = 6, FAVIT_TAPE_XN2 = 7, FAVIT_TAPE_MU2 = 8, FAVIT_TAPE_RS2 = 9, FAVIT_TAPE_H = 10, FAVIT_TAPE_PRE = 11,
  FAVIT_TAPE_X2 = 12
};
enum {   /* index of every slot of the backward's allocation in offsets_out */
  FAVIT_BWD_DPRE = 0, FAVIT_BWD_DXN2 = 1, FAVIT_BWD_G1_F32 = 2, FAVIT_BWD_G1_LP = 3, FAVIT_BWD_DO = 4,
  FAVIT_BWD_DQKV = 5, FAVIT_BWD_DXN1 = 6, FAVIT_BWD_G_OUT_F32 = 7, FAVIT_BWD_G_OUT_LP = 8, FAVIT_BWD_PART1 = 9,
  FAVIT_BWD_PART2 = 10
};
typedef struct favit_mhla_block {
  const float* x;       /* block input: fp32 [B*n, D], the residual stream */
  void* tape;           /* tape_bytes >= the tape layout's size */
  const float* g1;      /* norm1 weight, bias; norm2 weight, bias: fp32 [D] */
  const float* b1;
  const float* g2;
  const float* b2;
  const void* weff;     /* folded qkv weight bf16 [3D, D] and bias fp32 [3D] (favit_mhla_fold_fwd) */
  const float* beff;
  const void* wproj;    /* bf16 [D, D], fp32 [D] */
  const float* bproj;
  const void* wfc1;     /* bf16 [hidden, D], fp32 [hidden] */
  const float* bfc1;
  const void* wfc2;     /* bf16 [D, hidden], fp32 [D] */
  const float* bfc2;
  int64_t tape_bytes;
  int32_t B, n, D, H, W, hidden;
  int32_t training;     /* != 0: the forward saves lse and the backward may follow */
  float eps;
} favit_mhla_block_t;
int64_t favit_mhla_block_tape_layout(const favit_mhla_block_t* desc, int64_t* offsets_out /* [13] or NULL */);
int64_t favit_mhla_block_bwd_layout(const favit_mhla_block_t* desc, int32_t want_lp_out,
                                    int64_t* offsets_out /* [11] or NULL */);
int favit_mhla_block_fwd(const favit_mhla_block_t* desc, void* stream);
/* g_f32 / g_lp: the gradient of x2, fp32 and bf16 [M, D]. */
int favit_mhla_block_bwd(const favit_mhla_block_t* desc, const float* g_f32, const void* g_lp, void* bwd_buffers,
                         int64_t bwd_bytes, int32_t want_lp_out, void* stream);

/* The same block in two halves with a row cut between them (additive in ABI 8).  In a CLS-only
 * encoder the next block reads n_mlp <= n rows per image of this block's output, and everything after proj is
 * row-wise, so the MLP half (LN2, fc1, fc2 + residual and their backward) runs on B * n_mlp rows:
 *   attn_fwd (LN1, qkv, attention, proj + residual on B * n rows; x1 lands in the tape)
 *   -> the caller cuts x1 to x1c fp32 [B * n_mlp, D] (favit_rows_cut_fwd) -> mlp_fwd (x2 fp32 [B * n_mlp, D])
 *   mlp_bwd (dpre, dxn2, LayerNorm 2 backward: g1_f32 on B * n_mlp rows)
 *   -> the caller expands g1_f32 to B * n rows, fp32 and bf16 (favit_rows_cut_bwd) -> attn_bwd (g_out on B * n rows)
 * The four calls of a block share its descriptor and ONE tape / ONE bwd allocation, carved by the two queries below:
 * the slots and their order are those above, with xn2, mu2, rs2, h, pre, x2 and dpre, dxn2, g1_f32, part2 sized by
 * Mm = B * n_mlp (part2: nparts = min(2048, (Mm + 3) / 4)), every other slot by M = B * n, and g1_lp empty when
 * n_mlp < n (the row cut writes that copy into memory of the caller's).  n_mlp == n reproduces the offsets of
 * favit_mhla_block_tape_layout / _bwd_layout; n_mlp <= 0 or n_mlp > n is FAVIT_ERR_INVALID.  x1c is read by mlp_fwd
 * and mlp_bwd only (non-NULL, 16-byte aligned; it has to outlive mlp_bwd).  Validation is that of fwd / bwd: on a
 * negative return other than FAVIT_ERR_LAUNCH nothing has been launched. */
typedef struct favit_mhla_block_mlp {
  const float* x1c;     /* fp32 [B * n_mlp, D]: the kept rows of x1 */
  int32_t n_mlp;        /* rows per image of the MLP half, 1 .. n */
  int32_t reserved;
} favit_mhla_block_mlp_t;
int64_t favit_mhla_block_tape_layout2(const favit_mhla_block_t* desc, const favit_mhla_block_mlp_t* rows,
                                      int64_t* offsets_out /* [13] or NULL */);
int64_t favit_mhla_block_bwd_layout2(const favit_mhla_block_t* desc, const favit_mhla_block_mlp_t* rows,
                                     int32_t want_lp_out, int64_t* offsets_out /* [11] or NULL */);
int favit_mhla_block_attn_fwd(const favit_mhla_block_t* desc, const favit_mhla_block_mlp_t* rows, void* stream);
int favit_mhla_block_mlp_fwd(const favit_mhla_block_t* desc, const favit_mhla_block_mlp_t* rows, void* stream);
/* g_f32 / g_lp: the gradient of x2, fp32 and bf16 [B * n_mlp, D]. */
int favit_mhla_block_mlp_bwd(const favit_mhla_block_t* desc, const favit_mhla_block_mlp_t* rows, const float* g_f32,
                             const void* g_lp, void* bwd_buffers, int64_t bwd_bytes, int32_t want_lp_out, void* stream);
/* g1_f32 / g1_lp: the gradient of x1 expanded to [B * n, D], fp32 and bf16 (zeros in the cut rows). */
int favit_mhla_block_attn_bwd(const favit_mhla_block_t* desc, const favit_mhla_block_mlp_t* rows, const float* g1_f32,
                              const void* g1_lp, void* bwd_buffers, int64_t bwd_bytes, int32_t want_lp_out, void* stream);

/* Inverted dropout with a counter-based RNG (nn.Dropout sites, models/vit.py:136,138,
 * 102, mhla.py:159); the mask is recomputed from (seed, index) in backward. */
int favit_dropout(const void* x, void* y, int dtype, int64_t n, float p, uint64_t seed, void* stream);

/* Stochastic depth (DropPath; additive in ABI 8; csrc/drop_path.hip): per sample b a residual
 * branch is dropped with probability p and the survivors are scaled by scale = 1.0f / (1.0f - p).  Sample b is kept
 * iff the library's dropout draw keeps index b under (seed, p): the index is the sample number and nothing else, and
 * the dropout epoch word is mixed into the seed as in every other drawing kernel.
 * Both refuse p outside [0, 1), non-positive sizes and NULL pointers with FAVIT_ERR_INVALID, and D % 8 != 0 (every
 * access is 16 bytes wide) or n * D >= 2^31 with FAVIT_ERR_UNSUPPORTED; nothing is launched then.
 *
 * out[b, r, :] = x[b, r, :] + (keep(b) ? scale * y[b, r, :] : 0)      b < B, r < n
 * x, out: fp32 [B*n, D] contiguous; y: [B*n, D] of y_dtype (FAVIT_F32 | FAVIT_BF16).
 * out may alias y (same dtype) or x.  Rows of a dropped sample are NOT read from y. */
int favit_drop_path_add(const float* x, const void* y, int y_dtype, float* out, int32_t B, int32_t n, int32_t D,
                        float p, uint64_t seed, void* stream);
/* g_lp[b, r, :] = (lp_dtype) (keep(b) ? scale * g[b, r, :] : 0), optionally also times the element dropout mask of
 * the branch's output dropout (lp_dropout_p / _seed, element index row*D + col and scaling exactly as
 * favit_layernorm_bwd's lp copy).  g: fp32 [B*n, D]; g_lp: [B*n, D] of lp_dtype (FAVIT_F32 | FAVIT_BF16).
 * Rows of a dropped sample are NOT read from g. */
int favit_drop_path_bwd(const float* g, void* g_lp, int lp_dtype, int32_t B, int32_t n, int32_t D, float p,
                        uint64_t seed, float lp_dropout_p, uint64_t lp_dropout_seed, void* stream);

/* ------------------------------------------------------------------------------------
 * SPPP (models/sppp.py, models/sppp_mhla.py); the label map [B,HW,HW] int64 is an input.
 * map_patches (sppp.py:91-128): dominant label per patch (max count, ties -> smallest
 *   label), token rank = first-appearance order of the dominant labels in raster scan.
 *   Outputs: patch_rank[B,N] int32, n_tokens[B] int32, perm[B,N] int32 (patches grouped
 *   by rank, raster order inside), offs[B,N+1] int32 (group offsets into perm).
 * pool (sppp.py:192-223): mean / max / 'attention' pooling of patch embeddings
 *   emb[B,N,D] fp32 into tokens [B,R,D] fp32 (R = the common token count).
 * centroids (sppp_mhla.py:226-262): per LABEL s<S mean (x/w, y/h), empty -> 0.5.
 * posenc (sppp.py:267-300): x + [sin(cx*f), cos(cy*f)], CLS centroid (0.5,0.5)
 *   prepended when n_cent < L; cent == NULL selects the index-sinusoid branch (sppp.py:257-266).
 * ---------------------------------------------------------------------------------- */
/* dom_ws: caller-provided workspace [B,N] int64, receives the dominant label of every patch */
int favit_sppp_map_patches(const int64_t* seg, int32_t* patch_rank, int32_t* n_tokens, int32_t* perm,
                           int32_t* offs, int64_t* dom_ws, int32_t B, int32_t HW, int32_t P, void* stream);
int favit_sppp_pool_fwd(const float* emb, const int32_t* perm, const int32_t* offs, float* out, int32_t* argmax,
                        int32_t kind, int32_t B, int32_t N, int32_t R, int32_t D, void* stream);
int favit_sppp_pool_bwd(const float* dout, const float* emb, const int32_t* patch_rank, const int32_t* perm,
                        const int32_t* offs, const int32_t* argmax, float* demb, int32_t kind, int32_t B,
                        int32_t N, int32_t R, int32_t D, void* stream);
int favit_sppp_centroids(const int64_t* seg, float* cent, int32_t B, int32_t HW, int32_t S, void* stream);
int favit_sppp_posenc_fwd(const float* x, const float* cent, float* y, int32_t B, int32_t L, int32_t D,
                          int32_t n_cent, void* stream);

/* ------------------------------------------------------------------------------------
 * Harness-side pieces of the training step (experiments/mhla_pretrained.py:363-367):
 * mean cross-entropy with its gradient, and a fused multi-tensor AdamW step.
 * ---------------------------------------------------------------------------------- */
int favit_cross_entropy(const float* logits, const int64_t* labels, float* loss_rows, float* dlogits, int32_t B,
                        int32_t C, float grad_scale, void* stream);
/* p_bf16 (optional, [n] bf16): refreshed compute-dtype copy of the updated parameters */
int favit_adamw(float* p, const float* g, float* m, float* v, void* p_bf16, int64_t n, float lr, float beta1,
                float beta2, float eps, float weight_decay, float bias_c1, float bias_c2, float grad_scale,
                void* stream);

/* ------------------------------------------------------------------------------------
 * Stabilisers of the training step (additive in ABI 8): label smoothing, global-norm gradient clipping and
 * skipping a non-finite update, all without a host sync.
 * ---------------------------------------------------------------------------------- */
/* favit_cross_entropy with nn.CrossEntropyLoss(label_smoothing = eps), 0 <= eps < 1 (else FAVIT_ERR_INVALID):
 *   loss_rows[b] = lse - (1 - eps) * x[label] - eps * mean_c(x)
 *   dlogits      = (softmax - (1 - eps) * onehot - eps / C) * grad_scale
 * eps = 0 runs favit_cross_entropy itself (bit-identical).  Out-of-range labels and the health word as there. */
int favit_cross_entropy_ls(const float* logits, const int64_t* labels, float* loss_rows, float* dlogits, int32_t B,
                           int32_t C, float grad_scale, float label_smoothing, void* stream);

#define FAVIT_GRAD_NORM_MAX_BUFS 16
/* Global L2 norm of n (0..16) flat fp32 buffers, bufs[i] / lens[i] (host arrays, copied by value into the launch):
 * any 4-byte-aligned address, any length >= 0 (a NULL buffer needs length 0).
 *   out[0] = scale * sqrt(sum_i sum_j bufs[i][j]^2)      (scale: AdamW's grad_scale, 1 / world)
 *   out[1] = max_norm > 0 ? min(1, max_norm / (out[0] + 1e-6f)) : 1      (torch.nn.utils.clip_grad_norm_)
 * If out[0] is not finite, out[1] = NaN and, with skipped != NULL, *skipped (device uint32) is incremented.
 * Squares and sums are double precision; out[0] is within 1e-6 relative of a float64 evaluation (its own fp32
 * rounding and that of `scale` are the only ones).  Two launches: a fixed grid whose workgroups each store one
 * partial into `ws`, and one workgroup that adds the partials in a fixed order.  No atomics: the same inputs at the
 * same addresses give the same bits in every run.  ws: device workspace of ws_bytes >= favit_grad_norm_workspace()
 * bytes, 8-byte aligned, contents irrelevant on entry. */
int64_t favit_grad_norm_workspace(void);
int favit_grad_norm(int32_t n, const float* const* bufs, const int64_t* lens, float scale, float max_norm,
                    float* out, uint32_t* skipped, void* ws, int64_t ws_bytes, void* stream);

/* favit_adamw with the gradient (g[i] * grad_scale) * coef[0]; coef is a DEVICE scalar (favit_grad_norm's out + 1)
 * read when the kernel executes.  coef[0] == 1.0f is bit-identical to favit_adamw.  skip_nonfinite != 0 and a
 * non-finite coef[0]: p, m, v and p_bf16 are left untouched; the launch still counts itself in the health word and
 * sets its gradient flag.  skip_nonfinite == 0: a NaN coefficient propagates into p, m and v, as in torch. */
int favit_adamw_clip(float* p, const float* g, float* m, float* v, void* p_bf16, int64_t n, float lr, float beta1,
                     float beta2, float eps, float weight_decay, float bias_c1, float bias_c2, float grad_scale,
                     const float* coef, int32_t skip_nonfinite, void* stream);

/* ------------------------------------------------------------------------------------
 * Averaged weights (additive in ABI 8): an exponential moving average of the parameters kept by the AdamW launch
 * itself, and the exchange that puts it in the parameters' place for evaluation.
 * ---------------------------------------------------------------------------------- */
/* favit_adamw / favit_adamw_clip, and in the same pass, with p_new the parameter this launch writes,
 *   ema[i] = fmaf(ema_decay, ema[i], (1 - ema_decay) * p_new[i])       0 <= ema_decay <= 1 (else FAVIT_ERR_INVALID)
 * ema: [n] fp32 on the device, 4-byte aligned, not overlapping p.  p, m, v and p_bf16 get exactly the bits of the
 * entry point without the average.  ema_decay == 0 copies p_new (for finite ema).  A launch skipped by
 * skip_nonfinite leaves ema untouched like everything else.  38 bytes of traffic per element instead of 30. */
int favit_adamw_ema(float* p, const float* g, float* m, float* v, void* p_bf16, float* ema, int64_t n, float lr,
                    float beta1, float beta2, float eps, float weight_decay, float bias_c1, float bias_c2,
                    float grad_scale, float ema_decay, void* stream);
int favit_adamw_clip_ema(float* p, const float* g, float* m, float* v, void* p_bf16, float* ema, int64_t n, float lr,
                         float beta1, float beta2, float eps, float weight_decay, float bias_c1, float bias_c2,
                         float grad_scale, const float* coef, int32_t skip_nonfinite, float ema_decay, void* stream);

/* Exchange two flat fp32 buffers of n elements in one pass: a[i], b[i] = b[i], a[i]; with a_bf16 != NULL also
 * a_bf16[i] = bf16(new a[i]) (the compute-dtype mirror of a).  a and b must not overlap (a == b is refused).  No
 * address changes, so a captured graph that reads a / a_bf16 stays valid; two calls restore every bit. */
int favit_swap_params(float* a, float* b, void* a_bf16, int64_t n, void* stream);

/* ------------------------------------------------------------------------------------
 * Segmented AdamW (additive in ABI 8): ONE launch over one arena that holds every parameter group, with a learning
 * rate and a weight decay per segment.  For every element of segment s, p, m, v, p_bf16 and ema get exactly the bits
 * the single-group entry point of the same form (plain / _clip / _ema / _clip_ema, chosen by coef and ema being
 * non-NULL) gives for the same inputs with lr[s] and weight_decay[s].  The table travels by value in the kernel
 * arguments: no device table, no copy per step, nothing that must outlive the call; changed rates are picked up by
 * the next call.  Segment ends are multiples of FAVIT_ADAMW_SEG_ALIGN elements (one wave x 16 bytes per lane), so a
 * wave never straddles two segments; padding elements between groups are zero in p, g, m, v (and ema) and stay zero.
 * Refused with FAVIT_ERR_INVALID before anything is launched: count outside 1..FAVIT_ADAMW_MAX_SEGMENTS, an end that
 * is not a multiple of the alignment or not strictly ascending, end[count-1] != n, a NULL p / g / m / v, p / g / m / v
 * / ema not 16-byte aligned, p_bf16 not 8-byte aligned, skip_nonfinite without coef, ema with ema_decay outside [0, 1].
 * Health word: as the single-group launches, and the whole arena counts as ONE AdamW launch.
 * ---------------------------------------------------------------------------------- */
#define FAVIT_ADAMW_MAX_SEGMENTS 64
#define FAVIT_ADAMW_SEG_ALIGN    256   /* elements */
typedef struct favit_adamw_multi {
  float* p; const float* g; float* m; float* v;   /* [n] fp32 each, 16-byte aligned */
  void* p_bf16;            /* [n] bf16 mirror of p, 8-byte aligned, or NULL */
  float* ema;              /* [n] fp32 average, 16-byte aligned, or NULL */
  int64_t n;               /* arena length, a multiple of FAVIT_ADAMW_SEG_ALIGN */
  int32_t count;           /* 1..FAVIT_ADAMW_MAX_SEGMENTS */
  int32_t skip_nonfinite;  /* with coef: a non-finite coef[0] writes nothing but the health word */
  int64_t end[FAVIT_ADAMW_MAX_SEGMENTS];  /* exclusive ends, strictly ascending, multiples of the alignment, end[count-1] == n */
  float lr[FAVIT_ADAMW_MAX_SEGMENTS];
  float weight_decay[FAVIT_ADAMW_MAX_SEGMENTS];
  float beta1, beta2, eps, bias_c1, bias_c2, grad_scale, ema_decay;
  const float* coef;       /* device scalar of favit_grad_norm (out + 1), or NULL for the unclipped form */
} favit_adamw_multi_t;
int favit_adamw_multi(const favit_adamw_multi_t* d, void* stream);
int favit_adamw_multi_max_segments(void);
int favit_adamw_multi_align(void);

/* ------------------------------------------------------------------------------------
 * Batch mixing (additive in ABI 8): Mixup / CutMix of a batch with its own flip (timm's Mixup), and the loss of the
 * mixed targets.  Row b is paired with row p = B-1-b; with B odd the middle row is its own partner and never changes.
 * ---------------------------------------------------------------------------------- */
/* In place on x, fp32 [B, C, H, W]; lam [B] fp32 and box [B, 4] int32 = (y0, y1, x0, x1), half-open, are DEVICE arrays
 * read when the kernel executes.  With a, q the values of rows b and p before the call, per row b:
 *   box non-empty (y0 < y1 and x0 < x1): pixels with y0 <= y < y1 and x0 <= x < x1, in every channel, become q; the
 *                                        others keep their bits (CutMix; lam[b] is not read by the image side)
 *   box empty, lam[b] != 1:              x = fmaf(lam, a, (1 - lam) * q)                              (Mixup)
 *   box empty, lam[b] == 1:              the row keeps its bits
 * One work item owns the same 16 bytes (4 bytes when W % 4 != 0 or x is not 16-byte aligned) of both rows of a pair,
 * reads both old values and writes both new ones, so in place is safe: a full Mixup reads and writes the batch once, a
 * CutMix row moves only the 16-byte groups its box meets, a pair of unchanged rows moves nothing.  The box only
 * selects between the two in-range addresses, so no lam / box content can cause an out-of-range access.  C * H * W
 * must be below 2^31 (else FAVIT_ERR_UNSUPPORTED).  B == 1 succeeds and does nothing. */
int favit_batch_mix(float* x, const float* lam, const int32_t* box, int32_t B, int32_t C, int32_t H, int32_t W,
                    void* stream);
/* favit_cross_entropy_ls against the target  t[b] = lam[b] * onehot(labels[b]) + (1 - lam[b]) * onehot(labels[B-1-b]):
 *   loss_rows[b] = lse - (1 - eps) * (lam * x[y_b] + (1 - lam) * x[y_p]) - eps * mean_c(x)
 *   dlogits      = (softmax - (1 - eps) * (lam * [c == y_b] + (1 - lam) * [c == y_p]) - eps / C) * grad_scale
 * lam: DEVICE array [B], read when the kernel executes (a captured graph sees the values of each replay).  lam[b] == 1
 * gives the bits of favit_cross_entropy_ls with the same eps (eps = 0: of favit_cross_entropy) for finite logits.  An
 * own or a partner label out of range gives a NaN loss row, never an out-of-range read.  Health word as there. */
int favit_cross_entropy_mix(const float* logits, const int64_t* labels, const float* lam, float* loss_rows,
                            float* dlogits, int32_t B, int32_t C, float grad_scale, float label_smoothing,
                            void* stream);

/* ------------------------------------------------------------------------------------
 * Device RandAugment and Random Erasing (additive in ABI 8).  torchvision's RandAugment(num_ops, magnitude, bins) ops
 * on RGB PIL images, in the arithmetic Pillow runs in C: the augmented bytes are bit-identical to Pillow's.
 * ---------------------------------------------------------------------------------- */
/* src_u8 [B,S,S,C] uint8 (the out_u8 of favit_image_transform*), C == 3, S <= 2048 -> out fp32 [B,C,S,S] =
 * Normalize(ToTensor(augmented bytes)) with the expression of favit_image_transform, and out_u8 (optional) the
 * augmented bytes [B,S,S,C].  All ops of an image run inside ONE launch (one workgroup per image).
 *   scratch: uint8 [2,B,S,S,C] workspace (2 * B * S * S * C bytes), never NULL
 *   ops: int32 [B, n_ops, 8] DEVICE rows (op, p0 .. p6), 0 <= n_ops <= favit_randaugment_max_ops():
 *     0 identity
 *     1 affine, NEAREST: p0..p5 = a0, a1, a2', a3, a4, a5' in 16.16 fixed point, FIX(v) = floor(v * 65536 + 0.5),
 *       a2' = FIX(a2 + a0/2 + a1/2), a5' = FIX(a5 + a3/2 + a4/2); output (x, y) takes source pixel
 *       ((a2' + a1 y + a0 x) >> 16, (a5' + a4 y + a3 x) >> 16), or the fill p6 = r | g << 8 | b << 16 outside the image
 *     2 blend deg + f * (src - deg) in fp32 (unfused), truncated (clipped first unless 0 <= f <= 1): p0 = degenerate
 *       image (0 black: Brightness; 1 luma L = (19595 R + 38470 G + 7471 B + 0x8000) >> 16: Color; 2 the constant
 *       int(mean(L) + 0.5): Contrast; 3 the 3x3 SMOOTH filter with its border copied: Sharpness), p1 = bits of f
 *     3 v & p0 (Posterize)      4 v < p0 ? v : 255 - v (Solarize)
 *     5 ImageOps.autocontrast   6 ImageOps.equalize      (per channel, from the histogram of the current image)
 *     any other op id is treated as identity; no table content can cause an out-of-range access
 *   erase_box (optional): int32 [B,4] DEVICE rows (y0, y1, x0, x1), half open; inside a non-empty box out takes the
 *     erase fill instead (out_u8 never does): erase_value, a HOST array of 3 floats, per channel -- or, with
 *     erase_normal != 0, one standard-normal value per element: Box-Muller sqrt(-2 log u1) cos(2 pi u2) on the
 *     draws 2 idx and 2 idx + 1 of the library's counter-based generator under erase_seed, idx = ((b*C + c)*S + y)*S + x
 *     (a function of the seed and the element alone).
 * An all-identity table without erase_box gives the bits of favit_image_transform's out. */
#define FAVIT_RANDAUGMENT_MAX_OPS 8
enum {   /* the op ids of the table above */
  FAVIT_AUG_IDENTITY = 0, FAVIT_AUG_AFFINE = 1, FAVIT_AUG_BLEND = 2, FAVIT_AUG_MASK = 3, FAVIT_AUG_SOLARIZE = 4,
  FAVIT_AUG_AUTOCONTRAST = 5, FAVIT_AUG_EQUALIZE = 6
};
int favit_randaugment_max_ops(void);
int favit_randaugment(const uint8_t* src_u8, uint8_t* scratch, float* out, uint8_t* out_u8, const int32_t* ops,
                      int32_t n_ops, const int32_t* erase_box, const float* erase_value, int32_t erase_normal,
                      uint64_t erase_seed, int32_t B, int32_t S, int32_t C, const float* mean, const float* std,
                      void* stream);
/* The erase alone, in place on x fp32 [B,C,H,W]: box, value (HOST array of max(C, 3) floats; channels past the third
 * take the third), normal and seed as above with idx = ((b*C + c)*H + y)*W + x.  A box is clipped to the image; only
 * the 16-byte groups it meets are touched (single elements when W % 4 != 0 or x is not 16-byte aligned), every other
 * bit of x is left alone.  C * H * W must be below 2^31 and B below 65536 (else FAVIT_ERR_UNSUPPORTED). */
int favit_random_erase(float* x, const int32_t* box, const float* value, int32_t normal, uint64_t seed, int32_t B,
                       int32_t C, int32_t H, int32_t W, void* stream);

/* ------------------------------------------------------------------------------------
 * Knowledge distillation (additive in ABI 8; csrc/distill.hip): the loss of the labels and the
 * distance to a frozen teacher's logits in one launch.  x = logits, z = teacher, both fp32 [B, C] contiguous.
 * ---------------------------------------------------------------------------------- */
/*   base[b] = the loss row of favit_cross_entropy_mix with the same lam and label_smoothing (lam == NULL: unmixed,
 *             the row of favit_cross_entropy_ls)
 *   soft (hard == 0):  kd[b] = tau^2 * sum_c q_c (log q_c - log p_c),  q = softmax(z / tau), p = softmax(x / tau),
 *             evaluated through the two log-softmaxes, so an underflowed q_c contributes 0 and not 0 * inf
 *   hard (hard != 0):  kd[b] = lse(x) - x[argmax_c z_c], the lowest index on ties; tau is not used
 *   loss_rows[b] = (1 - alpha) * base[b] + alpha * kd[b];   kd_rows[b] = kd[b] when kd_rows != NULL (for logging)
 *   dlogits[b,c] = grad_scale * ((1 - alpha) * (softmax(x)_c - target_c) + alpha * d_c),  target as in
 *             favit_cross_entropy_mix;  soft: d_c = tau * (p_c - q_c);  hard: d_c = softmax(x)_c - [c == argmax z]
 * The teacher gets no gradient.  The mean of the soft kd over the rows is Hinton's loss,
 * kl_div(reduction = 'batchmean') * tau^2.  DeiT's code divides by B * C instead: the two differ by the factor 1 / C,
 * which a caller who wants DeiT's weighting folds into alpha.
 * alpha == 0 calls the existing entry point (favit_cross_entropy_mix with lam, else favit_cross_entropy_ls, which at
 * label_smoothing == 0 is favit_cross_entropy) and so gives its bits; the teacher is not read and kd_rows not written.
 * Refused with FAVIT_ERR_INVALID before any launch: alpha outside [0, 1]; tau not finite or <= 0 when soft;
 * label_smoothing outside [0, 1); NULL logits, teacher, labels or loss_rows; B <= 0 or C <= 0.
 * An own or (with lam) a partner label out of range gives a NaN loss row, never an out-of-range read; every other row
 * keeps its bits and all of dlogits stays finite.  A non-finite value in teacher row b makes loss_rows[b] (and
 * kd_rows[b]) NaN; every other row keeps its bits.  Health word as in the sibling loss kernels: a non-finite row whose
 * labels are valid raises the loss flag.
 * One launch, one wave per row, four rows per 256-thread workgroup, any C >= 1; no workspace, no atomics other than
 * the health word.  Rows of 128 < C <= 1024 are read once and held in registers; shorter and longer rows are walked in memory. */
int favit_cross_entropy_distill(const float* logits, const float* teacher, const int64_t* labels,
                                const float* lam /* [B] device or NULL: unmixed */,
                                float* loss_rows, float* kd_rows /* or NULL */, float* dlogits /* or NULL */,
                                int32_t B, int32_t C, float grad_scale, float label_smoothing,
                                float alpha, float tau, int32_t hard, void* stream);

/* ------------------------------------------------------------------------------------
 * Evaluation metrics (additive in ABI 8; csrc/eval.hip): loss, top-k hits, per-class counts
 * and a confusion matrix of a batch of logits, ADDED to a device-resident state.  Nothing synchronises; a validation
 * pass reads the state once at its end.  x = logits fp32 [B, C] with row stride ld >= C (elements), y = labels
 * int64 [B].
 * ---------------------------------------------------------------------------------- */
#define FAVIT_EVAL_MAX_TOPK 4       /* k values per launch */
#define FAVIT_EVAL_STATE_WORDS 10   /* 8-byte words of `state`: the slots below, HITS being FAVIT_EVAL_MAX_TOPK words */
enum {   /* index of every slot in `state`; LOSS_SUM and BATCH_MEAN_SUM hold doubles, the others int64 */
  FAVIT_EVAL_SLOT_LOSS_SUM = 0, FAVIT_EVAL_SLOT_BATCH_MEAN_SUM = 1, FAVIT_EVAL_SLOT_ROWS = 2,
  FAVIT_EVAL_SLOT_BATCHES = 3, FAVIT_EVAL_SLOT_IGNORED = 4, FAVIT_EVAL_SLOT_NONFINITE = 5, FAVIT_EVAL_SLOT_HITS = 6
};
/* Per row b, written to the caller's loss_rows fp32 [B], pred_rows int32 [B], rank_rows int32 [B] (all three required:
 * they are the hand-off between the two launches, and a per-sample result):
 *   loss[b] = lse(x_b) - x_b[y_b]                       the row of favit_cross_entropy, by the same expressions
 *   pred[b] = argmax_c x_b[c], the lowest index on ties
 *   rank[b] = #{c : x_c > x_y} + #{c < y : x_c == x_y}  the label's place in a stable descending sort: top-k hits
 *             iff rank < k, and rank == 0 iff pred == y
 *   y_b outside [0, C): the row is IGNORED: loss = NaN, pred = rank = -1, only the `ignored` counter moves and the
 *             logits of the row are not read (a batch padded with labels of -1 is evaluated this way)
 *   y_b valid and loss[b] not finite (a NaN or +inf anywhere in the row, -inf at the label, an all -inf row; a -inf on
 *             another class is legitimate and stays finite): pred = rank = -1; the row counts in rows, nonfinite and
 *             class_total[y] and adds its loss to both sums (a NaN model shows a NaN loss), hits no k and enters
 *             neither class_correct nor confusion.
 * Added to state (FAVIT_EVAL_STATE_WORDS 8-byte words, 8-byte aligned, zeroed by the caller before the first launch):
 *   LOSS_SUM (double) += the sum of the valid rows' losses;  BATCH_MEAN_SUM (double) += that sum / valid rows and
 *   BATCHES += 1 -- a launch without a valid row adds nothing to either and is no batch;  ROWS += valid rows;
 *   IGNORED, NONFINITE += those rows;  HITS + i += rows with rank < k_i, i < n_topk (k_i >= C always hits).
 * Optional (NULL: skipped), int64, zeroed by the caller:  class_total [C] += valid rows per label;  class_correct [C]
 *   += rows with pred == y per label;  confusion [C * C] += 1 at [y * C + pred].
 * Two launches: one wave per row, four rows per 256-thread workgroup, any C >= 1; then ONE workgroup that adds the
 * row records in a fixed order, the losses in double precision, looping when B exceeds its 256 threads.  No atomics on
 * floats: the same inputs give the same bits of `state` in every run.  The per-class and confusion counts are integer
 * atomics (integer adds commute, so they are reproducible as well).
 * Refused with FAVIT_ERR_INVALID before any launch, the state untouched: NULL logits, labels, state, loss_rows,
 * pred_rows or rank_rows; C < 1; B < 0; ld < C; n_topk outside 0..FAVIT_EVAL_MAX_TOPK; a k_i < 1 with i < n_topk
 * (the k beyond n_topk are not read).  B == 0 is FAVIT_OK and changes nothing.  The health word is not touched. */
int favit_eval_metrics(const float* logits, int64_t ld, const int64_t* labels, float* loss_rows, int32_t* pred_rows,
                       int32_t* rank_rows, int64_t* state, int64_t* class_total /* [C] or NULL */,
                       int64_t* class_correct /* [C] or NULL */, int64_t* confusion /* [C * C] or NULL */, int32_t B,
                       int32_t C, int32_t n_topk, int32_t k0, int32_t k1, int32_t k2, int32_t k3, void* stream);

/* ------------------------------------------------------------------------------------
 * Attention maps (additive in ABI 8; csrc/attn_maps.hip): the probabilities that the fused
 * attention kernels never write, recomputed from the qkv a forward stored, and attention rollout (Abnar and Zuidema)
 * over a stack of head-mean maps.  Diagnostics: no backward, no dropout; every output is fp32.
 * ---------------------------------------------------------------------------------- */
#define FAVIT_MAPS_MAX_WINDOW 15              /* largest window of favit_mhla_attn_probs */
#define FAVIT_SDPA_PROBS_MAX_WAVE_FLOATS 4096 /* favit_sdpa_probs: H * hd + 2 * H may not exceed this (LDS per wave) */
#define FAVIT_ROLLOUT_MAX_LAYERS 32           /* blocks per favit_attn_rollout launch */
#define FAVIT_ROLLOUT_MAX_L 16384             /* tokens per image in favit_attn_rollout: two fp32 rows of L in LDS */
/* Window probabilities of the MHLA core.  qkv: the folded projection output [B*L, 3D] of the attention forward above
 * (column = s*D + h*hd + d, D = H*hd), fp32 or bf16 (dtype), 16-byte aligned.  Slot w of row i is the key
 * win_idx(i, w) of the window rule (csrc/common.h; the table functional.window_indices returns): pad copies are slots
 * of their own, as in the forward, and a key's total weight is the sum of its slots.  Scores q . k~ / sqrt(hd) are
 * accumulated in fp32 and the softmax runs over the W slots of the row.
 *   head_mean = 0: probs fp32 [B, H, L, W];  head_mean = 1: probs fp32 [B, L, W], the probabilities of the heads
 *   summed in ascending head order in fp32, then multiplied by 1 / H.
 * mask: as in the forward (uint8 [B, L, L], non-zero keeps the key, NULL = none), and its contract: a masked slot of a
 * live row is exactly 0, a row whose slots are all masked is all zeros, nothing non-finite is written for finite qkv.
 * Runs for odd W <= FAVIT_MAPS_MAX_WINDOW, hd in {16, 32, 64, 128}, any L >= 1 (L < W included), one launch, eight
 * lanes per token row.  Even or non-positive W, a NULL qkv / probs, B, L, H < 1, another dtype or head_mean outside
 * {0, 1}: FAVIT_ERR_INVALID; another W or hd, or B*L >= 2^28: FAVIT_ERR_UNSUPPORTED; a misaligned qkv:
 * FAVIT_ERR_ALIGN.  Nothing is launched or written then. */
int favit_mhla_attn_probs(const void* qkv, float* probs, const uint8_t* mask, int32_t B, int32_t L, int32_t H,
                          int32_t hd, int32_t W, int dtype, int32_t head_mean, void* stream);
/* The dense counterpart: softmax(scale * q k^T) of the self-attention whose q and k are the column blocks 0 and D of
 * qkv [B*L, 3D] (fp32 or bf16, 16-byte aligned).  key_keep: uint8 [B, L] (0 masks the key for every query of the
 * sample) or NULL.  probs: fp32 [B, H, L, L] (head_mean = 0) or [B, L, L] (head_mean = 1, ascending head order, then
 * 1 / H).  A masked key has probability exactly 0 and a sample whose keys are all masked has all-zero rows.  One wave
 * per query row; hd % 16 == 0, H*hd + 2*H <= FAVIT_SDPA_PROBS_MAX_WAVE_FLOATS (else FAVIT_ERR_UNSUPPORTED), any
 * L >= 1; scale must be finite and > 0 (else FAVIT_ERR_INVALID, as for the arguments listed above). */
int favit_sdpa_probs(const void* qkv, float* probs, const uint8_t* key_keep, int32_t B, int32_t L, int32_t H,
                     int32_t hd, int dtype, float scale, int32_t head_mean, void* stream);
/* Attention rollout of n blocks (1 <= n <= FAVIT_ROLLOUT_MAX_LAYERS) in ONE launch.  probs / widths: HOST arrays of n
 * entries in block order; probs[k] is block k's head-mean map on the device, fp32 [B, L, W_k] in the slot layout above
 * where widths[k] = W_k is odd and > 0, or fp32 [B, L, L] where widths[k] = 0 (a dense block); the two kinds may mix.
 * In row-vector form, r = e_cls_row, and for k = n-1 .. 0:
 *   r'[j] = residual * r[j] + (1 - residual) * sum_i r[i] * P_k[i -> j]          out fp32 [B, L] = the last r
 * (P_k[i -> j] of a banded block: the sum of the slots of row i that hold key j).  0 <= residual <= 1.
 * One workgroup per image keeps r in LDS as two rows of L floats that swap after every block, so L is bounded by LDS
 * alone: L <= FAVIT_ROLLOUT_MAX_L (128 KiB of the CU's 160; FAVIT_ERR_UNSUPPORTED beyond).  Every key j GATHERS its
 * sources in a fixed order -- the rows j - W/2 .. j + W/2 whose window holds j, ascending; for j = L - 1 then the pad
 * copies of the short windows that start at 0; for j = 0 the pad copies of the windows cut at L; a dense block sums
 * the rows in ascending order -- so there are no atomics and the same inputs give the same bits in every run.
 * A row of P_k that is all zero (a fully masked row) hands nothing on: the mass r[i] that reached it is lost except
 * for its residual share, and out then sums to less than 1.
 * FAVIT_ERR_INVALID before any launch: NULL probs, widths, out or probs[k]; n, B, L < 1; n above the limit; cls_row
 * outside [0, L); an even or negative widths[k]; residual outside [0, 1] or NaN. */
int favit_attn_rollout(int32_t n, const float* const* probs, const int32_t* widths, float* out, int32_t cls_row,
                       int32_t B, int32_t L, float residual, void* stream);

/* ------------------------------------------------------------------------------------
 * Position-embedding resampling (additive in ABI 8; csrc/pos_resample.hip): a square grid of
 * fp32 token rows, separably resampled to another grid side.  x: fp32 [n_prefix + g_in^2, D], y: fp32
 * [n_prefix + g_out^2, D], both contiguous and 16-byte aligned, D % 4 == 0, n_prefix 0 or 1 (the CLS row).
 *   y[p, :] = x[p, :]                                                          for p < n_prefix
 *   y[n_prefix + a*g_out + b, :] = sum_i sum_j M[a,i] * M[b,j] * x[n_prefix + i*g_in + j, :]
 * M [g_out, g_in] comes in compressed-row form, DEVICE arrays built by the caller: rowptr int32 [g_out + 1]
 * (ascending, rowptr[0] = 0), cols int32 [rowptr[g_out]] with every entry in [0, g_in), vals fp32 of the same length.
 * The kernel trusts the table (focused-attention-vit_amd/kernels.py builds it on the host in float64 -- bicubic with
 * or without antialiasing, functional.pos_resample_matrix -- checks it, uploads it once and caches it per device).
 * The products (M[a,i] * M[b,j]) * x are accumulated in fp32 with fused multiply-adds in table order, i outer, j inner.
 * BOTH DIRECTIONS are this one entry point: the backward of y = R x is dx = R^T dy, the same operation with the
 * compressed rows of M^T and the two grid sides swapped (prefix rows are copied in both).  It is a gather, one thread
 * per four columns of an output row: no atomics, the same inputs give the same bits in every run.  A row of M whose
 * only entry is 1 copies its source row bit for bit (an identity M is a copy).  One launch; nothing is allocated or
 * copied, so it can be captured into a HIP graph.
 * FAVIT_ERR_INVALID: a NULL pointer, x == y, g_in or g_out < 1, n_prefix outside {0, 1}, D < 4 or D % 4 != 0;
 * FAVIT_ERR_UNSUPPORTED: n_prefix + g^2 > FAVIT_POS_RESAMPLE_MAX_L on either side; FAVIT_ERR_ALIGN: x or y not
 * 16-byte aligned.  Nothing is launched or written then. */
#define FAVIT_POS_RESAMPLE_MAX_L 16384        /* token rows on either side of favit_pos_resample */
int favit_pos_resample(const float* x, float* y, const int32_t* rowptr, const int32_t* cols, const float* vals,
                       int32_t g_in, int32_t g_out, int32_t n_prefix, int32_t D, void* stream);

/* ------------------------------------------------------------------------------------
 * Mean-pooled classification head (additive in ABI 8; csrc/head_pool.hip): the mean over the
 * token rows [first, L) of the encoder output, fused with the final LayerNorm in either order.  Everything is fp32;
 * x and dx are [B, L, D] contiguous; n = L - first (first = 1 leaves the CLS row out, as timm's global_pool='avg').
 * Norm-first (the model's `norm` on every token, then the mean):
 *   ln_meanpool_fwd   y[b] = (1/n) sum_{i >= first} LN(x[b,i]) = gamma * s[b] + beta, s[b] = (1/n) sum_i xhat[b,i];
 *                     writes y [B,D], s [B,D] and mean / rstd [B,n] of the pooled rows.
 *   ln_meanpool_bwd   dx[b,i] = the LayerNorm input gradient of the upstream row dy[b] / n (from the saved mean / rstd)
 *                     for i >= first and ZEROS below (every element of dx is written: no memset by the caller);
 *                     dgamma (+)= sum_b dy[b] * s[b], dbeta (+)= sum_b dy[b] (accumulate = 1 adds; both NULL: skipped).
 * Pool-first (timm's fc_norm: the mean, then favit_layernorm_fwd / _bwd on the B pooled rows):
 *   meanpool_fwd      p[b] = (1/n) sum_{i >= first} x[b,i]
 *   meanpool_bwd      dx[b,i] = dp[b] / n for i >= first and zeros below.
 * Forward reads x once: a workgroup sums a chunk of one image's rows (the arithmetic per row is favit_layernorm_fwd's)
 * into ws IN FP64 (the division by n rounds to fp32 once: s and p are the correctly rounded means of their fp32 terms),
 * which a second small launch folds in chunk order; ws holds favit_head_pool_workspace bytes (a negative
 * FAVIT_ERR_* for a refused geometry) and need not be initialised.  Backward reads x once (norm-first) or not at all
 * and writes dx once.  No atomics and no counters: the same inputs give the same bits in every run and graph replay;
 * nothing is allocated or synchronised.
 * FAVIT_ERR_INVALID: a NULL pointer, B, L or D < 1, first outside [0, L), only one of dgamma / dbeta;
 * FAVIT_ERR_UNSUPPORTED: D % 4 != 0 or D > 2048 (favit_layernorm_fwd's widths); FAVIT_ERR_ALIGN: x, dx, dy, dp, ws,
 * gamma or beta not 16-byte aligned.  Nothing is launched or written then. */
int64_t favit_head_pool_workspace(int32_t B, int32_t L, int32_t first, int32_t D);
int favit_ln_meanpool_fwd(const float* x, const float* gamma, const float* beta, float* y, float* s, float* mean,
                          float* rstd, void* ws, int32_t B, int32_t L, int32_t first, int32_t D, float eps,
                          void* stream);
int favit_ln_meanpool_bwd(const float* dy, const float* x, const float* gamma, const float* s, const float* mean,
                          const float* rstd, float* dx, float* dgamma, float* dbeta, int32_t accumulate, int32_t B,
                          int32_t L, int32_t first, int32_t D, void* stream);
int favit_meanpool_fwd(const float* x, float* p, void* ws, int32_t B, int32_t L, int32_t first, int32_t D,
                       void* stream);
int favit_meanpool_bwd(const float* dp, float* dx, int32_t B, int32_t L, int32_t first, int32_t D, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* FAVIT_H_ */
