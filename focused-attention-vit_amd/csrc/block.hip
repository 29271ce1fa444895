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

// n_mlp: token rows per image of the MLP half (LN2, fc1, fc2 and their backward); n_mlp == d->n is the whole block
// on one row count (DESIGN.md section 12 has the narrowed block)
int check_rows(const favit_mhla_block_t* d, const favit_mhla_block_mlp_t* r) {
  if (!r) return FAVIT_ERR_INVALID;
  if (r->n_mlp <= 0 || r->n_mlp > d->n) return FAVIT_ERR_INVALID;
  return FAVIT_OK;
}

void tape_sizes(const favit_mhla_block_t* d, int32_t n_mlp, int64_t* s) {
  const int64_t M = (int64_t)d->B * d->n, Mm = (int64_t)d->B * n_mlp, D = d->D, Hd = d->hidden;
  s[FAVIT_TAPE_XN1] = M * D * 2; s[FAVIT_TAPE_MU1] = M * 4; s[FAVIT_TAPE_RS1] = M * 4;
  s[FAVIT_TAPE_QKV] = M * 3 * D * 2; s[FAVIT_TAPE_O] = M * D * 2;
  s[FAVIT_TAPE_LSE] = d->training ? (int64_t)d->B * d->H * d->n * 4 : 0;
  s[FAVIT_TAPE_X1] = M * D * 4;
  s[FAVIT_TAPE_XN2] = Mm * D * 2; s[FAVIT_TAPE_MU2] = Mm * 4; s[FAVIT_TAPE_RS2] = Mm * 4;
  s[FAVIT_TAPE_H] = Mm * Hd * 2; s[FAVIT_TAPE_PRE] = Mm * Hd * 2;
  s[FAVIT_TAPE_X2] = Mm * D * 4;
}

int32_t ln_parts(int64_t rows) { return (int32_t)((rows + 3) / 4 < 2048 ? (rows + 3) / 4 : 2048); }

// narrowed (n_mlp < n): g1 leaves the MLP half in fp32 on n_mlp rows; the row cut writes the expanded pair itself
void bwd_sizes(const favit_mhla_block_t* d, int32_t n_mlp, int want_lp_out, int64_t* s) {
  const int64_t M = (int64_t)d->B * d->n, Mm = (int64_t)d->B * n_mlp, D = d->D, Hd = d->hidden;
  s[FAVIT_BWD_DPRE] = Mm * Hd * 2; s[FAVIT_BWD_DXN2] = Mm * D * 2;
  s[FAVIT_BWD_G1_F32] = Mm * D * 4; s[FAVIT_BWD_G1_LP] = n_mlp == d->n ? M * D * 2 : 0;
  s[FAVIT_BWD_DO] = M * D * 2; s[FAVIT_BWD_DQKV] = M * 3 * D * 2; s[FAVIT_BWD_DXN1] = M * D * 2;
  s[FAVIT_BWD_G_OUT_F32] = M * D * 4; s[FAVIT_BWD_G_OUT_LP] = want_lp_out ? M * D * 2 : 0;
  s[FAVIT_BWD_PART1] = 2 * (int64_t)ln_parts(M) * D * 4; s[FAVIT_BWD_PART2] = 2 * (int64_t)ln_parts(Mm) * D * 4;
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

// ---- the four launch sequences; every argument has been validated by the caller ----
// LN1, qkv, attention, proj + residual on B * n rows: x1 lands in the tape
int attn_half_fwd(const favit_mhla_block_t* d, const int64_t* o, void* stream) {
  int rc;
  char* t = reinterpret_cast<char*>(d->tape);
  const int64_t M = (int64_t)d->B * d->n;
  const int32_t D = d->D;
  if ((rc = favit_layernorm_fwd(d->x, D, d->g1, d->b1, t + o[FAVIT_TAPE_XN1], FAVIT_BF16,
                                reinterpret_cast<float*>(t + o[FAVIT_TAPE_MU1]),
                                reinterpret_cast<float*>(t + o[FAVIT_TAPE_RS1]), M, D, d->eps, stream)) != FAVIT_OK)
    return rc;
  favit_gemm_t g = gemm_base(t + o[FAVIT_TAPE_XN1], d->weff, t + o[FAVIT_TAPE_QKV], M, 3 * D, D, D, 1, FAVIT_BF16);
  g.bias = d->beff;
  g.ld_aux_out = 3 * D; g.ld_res = 3 * D;
  if ((rc = favit_gemm(&g, stream)) != FAVIT_OK) return rc;
  rc = d->training ? favit_mhla_attn_fwd_lse(t + o[FAVIT_TAPE_QKV], t + o[FAVIT_TAPE_O],
                                             reinterpret_cast<float*>(t + o[FAVIT_TAPE_LSE]), nullptr, d->B, d->n, d->H, 64,
                                             d->W, FAVIT_BF16, 0.f, 0, stream)
                   : favit_mhla_attn_fwd(t + o[FAVIT_TAPE_QKV], t + o[FAVIT_TAPE_O], nullptr, d->B, d->n, d->H, 64, d->W,
                                         FAVIT_BF16, 0.f, 0, stream);
  if (rc != FAVIT_OK) return rc;
  g = gemm_base(t + o[FAVIT_TAPE_O], d->wproj, t + o[FAVIT_TAPE_X1], M, D, D, D, 1, FAVIT_F32);
  g.bias = d->bproj; g.residual = d->x;
  g.ld_aux_out = D; g.ld_res = D;
  return favit_gemm(&g, stream);
}

// LN2, fc1, fc2 + residual on Mm rows of x1 (the tape's x1, or the caller's cut copy of it)
int mlp_half_fwd(const favit_mhla_block_t* d, const float* x1, int64_t Mm, const int64_t* o, void* stream) {
  int rc;
  char* t = reinterpret_cast<char*>(d->tape);
  const int32_t D = d->D, Hd = d->hidden;
  if ((rc = favit_layernorm_fwd(x1, D, d->g2, d->b2, t + o[FAVIT_TAPE_XN2], FAVIT_BF16,
                                reinterpret_cast<float*>(t + o[FAVIT_TAPE_MU2]),
                                reinterpret_cast<float*>(t + o[FAVIT_TAPE_RS2]), Mm, D, d->eps, stream)) != FAVIT_OK)
    return rc;
  favit_gemm_t g = gemm_base(t + o[FAVIT_TAPE_XN2], d->wfc1, t + o[FAVIT_TAPE_H], Mm, Hd, D, D, 1, FAVIT_BF16);
  g.bias = d->bfc1; g.act = FAVIT_ACT_GELU_SAVEGRAD; g.aux_out = t + o[FAVIT_TAPE_PRE];
  g.ld_aux_out = Hd; g.ld_res = Hd;
  if ((rc = favit_gemm(&g, stream)) != FAVIT_OK) return rc;
  g = gemm_base(t + o[FAVIT_TAPE_H], d->wfc2, t + o[FAVIT_TAPE_X2], Mm, D, Hd, Hd, 1, FAVIT_F32);
  g.bias = d->bfc2; g.residual = x1;
  g.ld_aux_out = D; g.ld_res = D;
  return favit_gemm(&g, stream);
}

// dpre, dxn2, LayerNorm 2 backward on Mm rows; g1_lp == nullptr: a row cut follows and writes the copy
int mlp_half_bwd(const favit_mhla_block_t* d, const float* x1, int64_t Mm, const float* g_f32, const void* g_lp,
                 const int64_t* o, char* w, const int64_t* b, void* g1_lp, void* stream) {
  int rc;
  char* t = reinterpret_cast<char*>(d->tape);
  const int32_t D = d->D, Hd = d->hidden, np = ln_parts(Mm);
  float* part2 = reinterpret_cast<float*>(w + b[FAVIT_BWD_PART2]);
  // dpre = (g . W2) * gelu'(pre): dX = dY.W with the weight [N, K] read mn-major
  favit_gemm_t g = gemm_base(g_lp, d->wfc2, w + b[FAVIT_BWD_DPRE], Mm, Hd, D, Hd, 0, FAVIT_BF16);
  g.act = FAVIT_ACT_MULAUX; g.aux_in = t + o[FAVIT_TAPE_PRE]; g.ld_aux_in = Hd;
  if ((rc = favit_gemm(&g, stream)) != FAVIT_OK) return rc;
  g = gemm_base(w + b[FAVIT_BWD_DPRE], d->wfc1, w + b[FAVIT_BWD_DXN2], Mm, D, Hd, D, 0, FAVIT_BF16);
  g.ld_aux_in = D;
  if ((rc = favit_gemm(&g, stream)) != FAVIT_OK) return rc;
  // LayerNorm 2 backward: the partial sums stay in part2 (dgamma = NULL: the caller folds them later)
  return favit_layernorm_bwd(w + b[FAVIT_BWD_DXN2], FAVIT_BF16, x1, D, d->g2,
                             reinterpret_cast<const float*>(t + o[FAVIT_TAPE_MU2]),
                             reinterpret_cast<const float*>(t + o[FAVIT_TAPE_RS2]), g_f32,
                             reinterpret_cast<float*>(w + b[FAVIT_BWD_G1_F32]), D, g1_lp, FAVIT_BF16, part2,
                             part2 + (int64_t)np * D, np, nullptr, nullptr, 1, Mm, D, 0.f, 0, stream);
}

// do, attention backward, dxn1, LayerNorm 1 backward on B * n rows
int attn_half_bwd(const favit_mhla_block_t* d, const float* g1, const void* g1_lp, const int64_t* o, char* w,
                  const int64_t* b, int want_lp_out, void* stream) {
  int rc;
  char* t = reinterpret_cast<char*>(d->tape);
  const int64_t M = (int64_t)d->B * d->n;
  const int32_t D = d->D, np = ln_parts(M);
  float* part1 = reinterpret_cast<float*>(w + b[FAVIT_BWD_PART1]);
  favit_gemm_t g = gemm_base(g1_lp, d->wproj, w + b[FAVIT_BWD_DO], M, D, D, D, 0, FAVIT_BF16);
  g.ld_aux_in = D;
  if ((rc = favit_gemm(&g, stream)) != FAVIT_OK) return rc;
  if ((rc = favit_mhla_attn_bwd_lse(t + o[FAVIT_TAPE_QKV], w + b[FAVIT_BWD_DO], t + o[FAVIT_TAPE_O],
                                    reinterpret_cast<const float*>(t + o[FAVIT_TAPE_LSE]), w + b[FAVIT_BWD_DQKV], nullptr,
                                    d->B, d->n, d->H, 64, d->W, FAVIT_BF16, 0.f, 0, stream)) != FAVIT_OK)
    return rc;
  g = gemm_base(w + b[FAVIT_BWD_DQKV], d->weff, w + b[FAVIT_BWD_DXN1], M, D, 3 * D, D, 0, FAVIT_BF16);
  g.ld_aux_in = D;
  if ((rc = favit_gemm(&g, stream)) != FAVIT_OK) return rc;
  return favit_layernorm_bwd(w + b[FAVIT_BWD_DXN1], FAVIT_BF16, d->x, D, d->g1,
                             reinterpret_cast<const float*>(t + o[FAVIT_TAPE_MU1]),
                             reinterpret_cast<const float*>(t + o[FAVIT_TAPE_RS1]), g1,
                             reinterpret_cast<float*>(w + b[FAVIT_BWD_G_OUT_F32]), D,
                             want_lp_out ? w + b[FAVIT_BWD_G_OUT_LP] : nullptr, FAVIT_BF16, part1, part1 + (int64_t)np * D,
                             np, nullptr, nullptr, 1, M, D, 0.f, 0, stream);
}

// what every chain call checks before its first launch; fills the tape offsets
int check_call(const favit_mhla_block_t* d, int32_t n_mlp, int64_t* o) {
  int rc = check_params(d);
  if (rc != FAVIT_OK) return rc;
  int64_t s[TAPE_N];
  tape_sizes(d, n_mlp, s);
  return d->tape_bytes < layout(s, TAPE_N, o) ? FAVIT_ERR_INVALID : FAVIT_OK;
}

// the same for a backward call: training, the gradient pair and the arena; fills the arena offsets
int check_bwd_call(const favit_mhla_block_t* d, int32_t n_mlp, const float* g_f32, const void* g_lp, void* bwd_buffers,
                   int64_t bwd_bytes, int32_t want_lp_out, int64_t* o, int64_t* b) {
  int rc = check_params(d);
  if (rc != FAVIT_OK) return rc;
  if (!d->training || !g_f32 || !g_lp || !bwd_buffers) return FAVIT_ERR_INVALID;
  if (((uintptr_t)bwd_buffers % ALIGN) != 0 || ((uintptr_t)g_f32 % 16) != 0 || ((uintptr_t)g_lp % 16) != 0)
    return FAVIT_ERR_ALIGN;
  int64_t s[TAPE_N], bs[BWD_N];
  tape_sizes(d, n_mlp, s);
  if (d->tape_bytes < layout(s, TAPE_N, o)) return FAVIT_ERR_INVALID;
  bwd_sizes(d, n_mlp, want_lp_out, bs);
  if (bwd_bytes < layout(bs, BWD_N, b)) return FAVIT_ERR_INVALID;
  return FAVIT_OK;
}

int check_x1c(const favit_mhla_block_mlp_t* r) {
  if (!r->x1c) return FAVIT_ERR_INVALID;
  return ((uintptr_t)r->x1c % 16) != 0 ? FAVIT_ERR_ALIGN : FAVIT_OK;
}
}  // namespace

extern "C" int64_t favit_mhla_block_tape_layout(const favit_mhla_block_t* desc, int64_t* offsets_out) {
  const int rc = check_geometry(desc);
  if (rc != FAVIT_OK) return rc;
  int64_t s[TAPE_N];
  tape_sizes(desc, desc->n, s);
  return layout(s, TAPE_N, offsets_out);
}

extern "C" int64_t favit_mhla_block_bwd_layout(const favit_mhla_block_t* desc, int32_t want_lp_out, int64_t* offsets_out) {
  const int rc = check_geometry(desc);
  if (rc != FAVIT_OK) return rc;
  int64_t s[BWD_N];
  bwd_sizes(desc, desc->n, want_lp_out, s);
  return layout(s, BWD_N, offsets_out);
}

extern "C" int favit_mhla_block_fwd(const favit_mhla_block_t* d, void* stream) {
  int rc = check_geometry(d);
  if (rc != FAVIT_OK) return rc;
  int64_t o[TAPE_N];
  if ((rc = check_call(d, d->n, o)) != FAVIT_OK) return rc;
  // ---- nothing has been launched above this line ----
  if ((rc = attn_half_fwd(d, o, stream)) != FAVIT_OK) return rc;
  return mlp_half_fwd(d, reinterpret_cast<const float*>(reinterpret_cast<char*>(d->tape) + o[FAVIT_TAPE_X1]),
                      (int64_t)d->B * d->n, o, stream);
}

extern "C" int favit_mhla_block_bwd(const favit_mhla_block_t* d, const float* g_f32, const void* g_lp, void* bwd_buffers,
                                    int64_t bwd_bytes, int32_t want_lp_out, void* stream) {
  int rc = check_geometry(d);
  if (rc != FAVIT_OK) return rc;
  int64_t o[TAPE_N], b[BWD_N];
  if ((rc = check_bwd_call(d, d->n, g_f32, g_lp, bwd_buffers, bwd_bytes, want_lp_out, o, b)) != FAVIT_OK) return rc;
  // ---- nothing has been launched above this line ----
  char* w = reinterpret_cast<char*>(bwd_buffers);
  const float* x1 = reinterpret_cast<const float*>(reinterpret_cast<char*>(d->tape) + o[FAVIT_TAPE_X1]);
  if ((rc = mlp_half_bwd(d, x1, (int64_t)d->B * d->n, g_f32, g_lp, o, w, b, w + b[FAVIT_BWD_G1_LP], stream)) != FAVIT_OK)
    return rc;
  return attn_half_bwd(d, reinterpret_cast<const float*>(w + b[FAVIT_BWD_G1_F32]), w + b[FAVIT_BWD_G1_LP], o, w, b,
                       want_lp_out, stream);
}

// ---- the block in two halves with a row cut between them ----
extern "C" int64_t favit_mhla_block_tape_layout2(const favit_mhla_block_t* desc, const favit_mhla_block_mlp_t* rows,
                                                 int64_t* offsets_out) {
  int rc = check_geometry(desc);
  if (rc != FAVIT_OK) return rc;
  if ((rc = check_rows(desc, rows)) != FAVIT_OK) return rc;
  int64_t s[TAPE_N];
  tape_sizes(desc, rows->n_mlp, s);
  return layout(s, TAPE_N, offsets_out);
}

extern "C" int64_t favit_mhla_block_bwd_layout2(const favit_mhla_block_t* desc, const favit_mhla_block_mlp_t* rows,
                                                int32_t want_lp_out, int64_t* offsets_out) {
  int rc = check_geometry(desc);
  if (rc != FAVIT_OK) return rc;
  if ((rc = check_rows(desc, rows)) != FAVIT_OK) return rc;
  int64_t s[BWD_N];
  bwd_sizes(desc, rows->n_mlp, want_lp_out, s);
  return layout(s, BWD_N, offsets_out);
}

extern "C" int favit_mhla_block_attn_fwd(const favit_mhla_block_t* d, const favit_mhla_block_mlp_t* r, void* stream) {
  int rc = check_geometry(d);
  if (rc != FAVIT_OK) return rc;
  if ((rc = check_rows(d, r)) != FAVIT_OK) return rc;
  int64_t o[TAPE_N];
  if ((rc = check_call(d, r->n_mlp, o)) != FAVIT_OK) return rc;
  // ---- nothing has been launched above this line ----
  return attn_half_fwd(d, o, stream);
}

extern "C" int favit_mhla_block_mlp_fwd(const favit_mhla_block_t* d, const favit_mhla_block_mlp_t* r, void* stream) {
  int rc = check_geometry(d);
  if (rc != FAVIT_OK) return rc;
  if ((rc = check_rows(d, r)) != FAVIT_OK) return rc;
  if ((rc = check_x1c(r)) != FAVIT_OK) return rc;
  int64_t o[TAPE_N];
  if ((rc = check_call(d, r->n_mlp, o)) != FAVIT_OK) return rc;
  // ---- nothing has been launched above this line ----
  return mlp_half_fwd(d, r->x1c, (int64_t)d->B * r->n_mlp, o, stream);
}

extern "C" int favit_mhla_block_mlp_bwd(const favit_mhla_block_t* d, const favit_mhla_block_mlp_t* r, const float* g_f32,
                                        const void* g_lp, void* bwd_buffers, int64_t bwd_bytes, int32_t want_lp_out,
                                        void* stream) {
  int rc = check_geometry(d);
  if (rc != FAVIT_OK) return rc;
  if ((rc = check_rows(d, r)) != FAVIT_OK) return rc;
  if ((rc = check_x1c(r)) != FAVIT_OK) return rc;
  int64_t o[TAPE_N], b[BWD_N];
  if ((rc = check_bwd_call(d, r->n_mlp, g_f32, g_lp, bwd_buffers, bwd_bytes, want_lp_out, o, b)) != FAVIT_OK) return rc;
  // ---- nothing has been launched above this line ----
  char* w = reinterpret_cast<char*>(bwd_buffers);
  return mlp_half_bwd(d, r->x1c, (int64_t)d->B * r->n_mlp, g_f32, g_lp, o, w, b,
                      r->n_mlp == d->n ? w + b[FAVIT_BWD_G1_LP] : nullptr, stream);
}

extern "C" int favit_mhla_block_attn_bwd(const favit_mhla_block_t* d, const favit_mhla_block_mlp_t* r, const float* g1_f32,
                                         const void* g1_lp, void* bwd_buffers, int64_t bwd_bytes, int32_t want_lp_out,
                                         void* stream) {
  int rc = check_geometry(d);
  if (rc != FAVIT_OK) return rc;
  if ((rc = check_rows(d, r)) != FAVIT_OK) return rc;
  int64_t o[TAPE_N], b[BWD_N];
  if ((rc = check_bwd_call(d, r->n_mlp, g1_f32, g1_lp, bwd_buffers, bwd_bytes, want_lp_out, o, b)) != FAVIT_OK) return rc;
  // ---- nothing has been launched above this line ----
  return attn_half_bwd(d, g1_f32, g1_lp, o, reinterpret_cast<char*>(bwd_buffers), b, want_lp_out, stream);
}
