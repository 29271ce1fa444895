// One MHLA encoder block per call: the forward chain and the input-gradient chain of a pre-LN block
//   x1 = x + proj(attn(qkv(LN1(x))));  x2 = x1 + fc2(gelu(fc1(LN2(x1))))
// issued from ONE host call each.  Nothing here launches a kernel of its own: every step goes
// through the library's extern "C" entry points (favit_layernorm_*, favit_gemm, favit_mhla_attn_*_lse), with the
// arguments the Python chains (functional.MHLAChain / MLPChain / EncoderOp) build for the same block, so kernel
// selection, validation and favit_gemm_last_kernel are the ones every other caller sees.  What is saved is host work:
// nine wrapper calls, their allocations and their descriptors per block and direction.
#include <string.h>

#include "favit.h"

namespace {
constexpr int64_t ALIGN = 256;
constexpr int TAPE_N = FAVIT_BLOCK_TAPE_SLOTS, BWD_N = FAVIT_BLOCK_BWD_SLOTS;
enum { T_XN1, T_MU1, T_RS1, T_QKV, T_O, T_LSE, T_X1, T_XN2, T_MU2, T_RS2, T_H, T_PRE, T_X2 };
enum { G_DPRE, G_DXN2, G_G1_F32, G_G1_LP, G_DO, G_DQKV, G_DXN1, G_OUT_F32, G_OUT_LP, G_PART1, G_PART2 };

inline int64_t up(int64_t v) { return (v + ALIGN - 1) / ALIGN * ALIGN; }

// geometry only: what both layout queries and both chains need to hold
int check_geometry(const favit_mhla_block_t* d) {
  if (!d) return FAVIT_ERR_INVALID;
  if (d->B <= 0 || d->n <= 0 || d->D <= 0 || d->H <= 0 || d->W <= 0 || d->hidden <= 0 || !(d->eps > 0.f))
    return FAVIT_ERR_INVALID;
  if (d->D % 64 != 0 || d->D % d->H != 0 || d->D / d->H != 64) return FAVIT_ERR_UNSUPPORTED;
  if (d->hidden % 8 != 0) return FAVIT_ERR_UNSUPPORTED;
  if (!favit_mhla_attn_lse_supported(d->n, 64, d->W, FAVIT_BF16)) return FAVIT_ERR_UNSUPPORTED;
  if ((int64_t)d->B * d->n >= (int64_t)1 << 31) return FAVIT_ERR_UNSUPPORTED;
  return FAVIT_OK;
}

int64_t layout(const int64_t* sizes, int n, int64_t* offsets) {
  int64_t off = 0;
  for (int i = 0; i < n; ++i) {
    if (offsets) offsets[i] = off;
    off += up(sizes[i]);
  }
  return off;
}

void tape_sizes(const favit_mhla_block_t* d, int64_t* s) {
  const int64_t M = (int64_t)d->B * d->n, D = d->D, Hd = d->hidden;
  s[T_XN1] = M * D * 2; s[T_MU1] = M * 4; s[T_RS1] = M * 4;
  s[T_QKV] = M * 3 * D * 2; s[T_O] = M * D * 2;
  s[T_LSE] = d->training ? (int64_t)d->B * d->H * d->n * 4 : 0;
  s[T_X1] = M * D * 4;
  s[T_XN2] = M * D * 2; s[T_MU2] = M * 4; s[T_RS2] = M * 4;
  s[T_H] = M * Hd * 2; s[T_PRE] = M * Hd * 2;
  s[T_X2] = M * D * 4;
}

int32_t ln_parts(int64_t rows) { return (int32_t)((rows + 3) / 4 < 2048 ? (rows + 3) / 4 : 2048); }

void bwd_sizes(const favit_mhla_block_t* d, int want_lp_out, int64_t* s) {
  const int64_t M = (int64_t)d->B * d->n, D = d->D, Hd = d->hidden;
  const int64_t part = 2 * (int64_t)ln_parts(M) * D * 4;
  s[G_DPRE] = M * Hd * 2; s[G_DXN2] = M * D * 2;
  s[G_G1_F32] = M * D * 4; s[G_G1_LP] = M * D * 2;
  s[G_DO] = M * D * 2; s[G_DQKV] = M * 3 * D * 2; s[G_DXN1] = M * D * 2;
  s[G_OUT_F32] = M * D * 4; s[G_OUT_LP] = want_lp_out ? M * D * 2 : 0;
  s[G_PART1] = part; s[G_PART2] = part;
}

// a bf16-in GEMM without batch, split or dropout: the fields every GEMM of the two chains shares
favit_gemm_t gemm_base(const void* A, const void* B, void* C, int64_t M, int64_t N, int64_t K, int64_t ldb, int b_kmajor,
                       int out_dtype) {
  favit_gemm_t g;
  memset(&g, 0, sizeof(g));
  g.A = A; g.B = B; g.C = C;
  g.M = M; g.N = N; g.K = K;
  g.lda = K; g.ldb = ldb; g.ldc = N;
  g.batch = 1; g.batch_inner = 1;
  g.a_kmajor = 1; g.b_kmajor = b_kmajor;
  g.in_dtype = FAVIT_BF16; g.out_dtype = out_dtype;
  g.act = FAVIT_ACT_NONE;
  g.alpha = 1.0f;
  return g;
}

int check_params(const favit_mhla_block_t* d) {
  if (!d->x || !d->tape || !d->g1 || !d->b1 || !d->g2 || !d->b2 || !d->weff || !d->beff || !d->wproj || !d->bproj ||
      !d->wfc1 || !d->bfc1 || !d->wfc2 || !d->bfc2)
    return FAVIT_ERR_INVALID;
  if (((uintptr_t)d->tape % ALIGN) != 0 || ((uintptr_t)d->x % 16) != 0) return FAVIT_ERR_ALIGN;
  return FAVIT_OK;
}
}  // namespace

extern "C" int64_t favit_mhla_block_tape_layout(const favit_mhla_block_t* desc, int64_t* offsets_out) {
  const int rc = check_geometry(desc);
  if (rc != FAVIT_OK) return rc;
  int64_t s[TAPE_N];
  tape_sizes(desc, s);
  return layout(s, TAPE_N, offsets_out);
}

extern "C" int64_t favit_mhla_block_bwd_layout(const favit_mhla_block_t* desc, int32_t want_lp_out, int64_t* offsets_out) {
  const int rc = check_geometry(desc);
  if (rc != FAVIT_OK) return rc;
  int64_t s[BWD_N];
  bwd_sizes(desc, want_lp_out, s);
  return layout(s, BWD_N, offsets_out);
}

extern "C" int favit_mhla_block_fwd(const favit_mhla_block_t* d, void* stream) {
  int rc = check_geometry(d);
  if (rc != FAVIT_OK) return rc;
  if ((rc = check_params(d)) != FAVIT_OK) return rc;
  int64_t s[TAPE_N], o[TAPE_N];
  tape_sizes(d, s);
  if (d->tape_bytes < layout(s, TAPE_N, o)) return FAVIT_ERR_INVALID;
  // ---- nothing has been launched above this line ----
  char* t = reinterpret_cast<char*>(d->tape);
  const int64_t M = (int64_t)d->B * d->n;
  const int32_t D = d->D, Hd = d->hidden;
  float* x1 = reinterpret_cast<float*>(t + o[T_X1]);
  if ((rc = favit_layernorm_fwd(d->x, D, d->g1, d->b1, t + o[T_XN1], FAVIT_BF16, reinterpret_cast<float*>(t + o[T_MU1]),
                                reinterpret_cast<float*>(t + o[T_RS1]), M, D, d->eps, stream)) != FAVIT_OK)
    return rc;
  favit_gemm_t g = gemm_base(t + o[T_XN1], d->weff, t + o[T_QKV], M, 3 * D, D, D, 1, FAVIT_BF16);
  g.bias = d->beff;
  g.ld_aux_out = 3 * D; g.ld_res = 3 * D;
  if ((rc = favit_gemm(&g, stream)) != FAVIT_OK) return rc;
  rc = d->training ? favit_mhla_attn_fwd_lse(t + o[T_QKV], t + o[T_O], reinterpret_cast<float*>(t + o[T_LSE]), nullptr,
                                             d->B, d->n, d->H, 64, d->W, FAVIT_BF16, 0.f, 0, stream)
                   : favit_mhla_attn_fwd(t + o[T_QKV], t + o[T_O], nullptr, d->B, d->n, d->H, 64, d->W, FAVIT_BF16, 0.f, 0,
                                         stream);
  if (rc != FAVIT_OK) return rc;
  g = gemm_base(t + o[T_O], d->wproj, x1, M, D, D, D, 1, FAVIT_F32);
  g.bias = d->bproj; g.residual = d->x;
  g.ld_aux_out = D; g.ld_res = D;
  if ((rc = favit_gemm(&g, stream)) != FAVIT_OK) return rc;
  if ((rc = favit_layernorm_fwd(x1, D, d->g2, d->b2, t + o[T_XN2], FAVIT_BF16, reinterpret_cast<float*>(t + o[T_MU2]),
                                reinterpret_cast<float*>(t + o[T_RS2]), M, D, d->eps, stream)) != FAVIT_OK)
    return rc;
  g = gemm_base(t + o[T_XN2], d->wfc1, t + o[T_H], M, Hd, D, D, 1, FAVIT_BF16);
  g.bias = d->bfc1; g.act = FAVIT_ACT_GELU_SAVEGRAD; g.aux_out = t + o[T_PRE];
  g.ld_aux_out = Hd; g.ld_res = Hd;
  if ((rc = favit_gemm(&g, stream)) != FAVIT_OK) return rc;
  g = gemm_base(t + o[T_H], d->wfc2, t + o[T_X2], M, D, Hd, Hd, 1, FAVIT_F32);
  g.bias = d->bfc2; g.residual = x1;
  g.ld_aux_out = D; g.ld_res = D;
  return favit_gemm(&g, stream);
}

extern "C" int favit_mhla_block_bwd(const favit_mhla_block_t* d, const float* g_f32, const void* g_lp, void* bwd_buffers,
                                    int64_t bwd_bytes, int32_t want_lp_out, void* stream) {
  int rc = check_geometry(d);
  if (rc != FAVIT_OK) return rc;
  if ((rc = check_params(d)) != FAVIT_OK) return rc;
  if (!d->training || !g_f32 || !g_lp || !bwd_buffers) return FAVIT_ERR_INVALID;
  if (((uintptr_t)bwd_buffers % ALIGN) != 0 || ((uintptr_t)g_f32 % 16) != 0 || ((uintptr_t)g_lp % 16) != 0)
    return FAVIT_ERR_ALIGN;
  int64_t s[TAPE_N], o[TAPE_N], bs[BWD_N], b[BWD_N];
  tape_sizes(d, s);
  if (d->tape_bytes < layout(s, TAPE_N, o)) return FAVIT_ERR_INVALID;
  bwd_sizes(d, want_lp_out, bs);
  if (bwd_bytes < layout(bs, BWD_N, b)) return FAVIT_ERR_INVALID;
  // ---- nothing has been launched above this line ----
  char* t = reinterpret_cast<char*>(d->tape);
  char* w = reinterpret_cast<char*>(bwd_buffers);
  const int64_t M = (int64_t)d->B * d->n;
  const int32_t D = d->D, Hd = d->hidden, np = ln_parts(M);
  float* g1 = reinterpret_cast<float*>(w + b[G_G1_F32]);
  float* part1 = reinterpret_cast<float*>(w + b[G_PART1]);
  float* part2 = reinterpret_cast<float*>(w + b[G_PART2]);
  // dpre = (g . W2) * gelu'(pre): dX = dY.W with the weight [N, K] read mn-major
  favit_gemm_t g = gemm_base(g_lp, d->wfc2, w + b[G_DPRE], M, Hd, D, Hd, 0, FAVIT_BF16);
  g.act = FAVIT_ACT_MULAUX; g.aux_in = t + o[T_PRE]; g.ld_aux_in = Hd;
  if ((rc = favit_gemm(&g, stream)) != FAVIT_OK) return rc;
  g = gemm_base(w + b[G_DPRE], d->wfc1, w + b[G_DXN2], M, D, Hd, D, 0, FAVIT_BF16);
  g.ld_aux_in = D;
  if ((rc = favit_gemm(&g, stream)) != FAVIT_OK) return rc;
  // LayerNorm 2 backward: the partial sums stay in part2 (dgamma = NULL: the caller folds them later)
  if ((rc = favit_layernorm_bwd(w + b[G_DXN2], FAVIT_BF16, reinterpret_cast<const float*>(t + o[T_X1]), D, d->g2,
                                reinterpret_cast<const float*>(t + o[T_MU2]), reinterpret_cast<const float*>(t + o[T_RS2]),
                                g_f32, g1, D, w + b[G_G1_LP], FAVIT_BF16, part2, part2 + (int64_t)np * D, np, nullptr,
                                nullptr, 1, M, D, 0.f, 0, stream)) != FAVIT_OK)
    return rc;
  g = gemm_base(w + b[G_G1_LP], d->wproj, w + b[G_DO], M, D, D, D, 0, FAVIT_BF16);
  g.ld_aux_in = D;
  if ((rc = favit_gemm(&g, stream)) != FAVIT_OK) return rc;
  if ((rc = favit_mhla_attn_bwd_lse(t + o[T_QKV], w + b[G_DO], t + o[T_O], reinterpret_cast<const float*>(t + o[T_LSE]),
                                    w + b[G_DQKV], nullptr, d->B, d->n, d->H, 64, d->W, FAVIT_BF16, 0.f, 0, stream)) !=
      FAVIT_OK)
    return rc;
  g = gemm_base(w + b[G_DQKV], d->weff, w + b[G_DXN1], M, D, 3 * D, D, 0, FAVIT_BF16);
  g.ld_aux_in = D;
  if ((rc = favit_gemm(&g, stream)) != FAVIT_OK) return rc;
  return favit_layernorm_bwd(w + b[G_DXN1], FAVIT_BF16, d->x, D, d->g1, reinterpret_cast<const float*>(t + o[T_MU1]),
                             reinterpret_cast<const float*>(t + o[T_RS1]), g1, reinterpret_cast<float*>(w + b[G_OUT_F32]), D,
                             want_lp_out ? w + b[G_OUT_LP] : nullptr, FAVIT_BF16, part1, part1 + (int64_t)np * D, np, nullptr,
                             nullptr, 1, M, D, 0.f, 0, stream);
}
