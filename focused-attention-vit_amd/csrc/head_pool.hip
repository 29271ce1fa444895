// Mean-pooled classification head (gfx950): the token mean over rows [first, L) of the fp32 encoder output, fused with
// the final LayerNorm in either order.
//   norm-first  y[b] = (1/n) sum_i LN(x[b,i]) = gamma * s[b] + beta,  s[b] = (1/n) sum_i xhat[b,i]
//   pool-first  p[b] = (1/n) sum_i x[b,i]   (favit_layernorm_fwd / _bwd then run on the B pooled rows)
// Forward reads x once: a workgroup owns a chunk of one image's rows, its waves walk the chunk with the row kept in
// registers (one row per wave, or two for D <= 512, exactly as ln_fwd_kernel / ln_fwd_half_kernel do), and the chunk's
// column sums go to a workspace that a second small launch folds in chunk order.  The sums are carried in fp64 from the
// first add to the division by n (two VALU operations per element under a pass that waits for HBM), so s and p are the
// correctly rounded means of the fp32 terms: the LayerNorm behind a mean over ~1000 rows multiplies the error of p by
// 1 / std(p), and an fp32 running sum of that length was measured at 2.3x the error of torch's mean there.
// Backward reads x once (norm-first) or not at all (pool-first) and writes every row of dx once, zeros below `first`
// included.  No atomics, no counters: every sum has one fixed order, so the same inputs give the same bits in every
// run and in every graph replay.
#include "common.h"

namespace {

constexpr int HP_ROWS = 64;          // rows a workgroup aims to own: B = 256, L = 197 gives 1024 workgroups, 4 per CU
constexpr int HP_MAX_D = 2048;       // favit_layernorm_fwd's limit (8 float4 per lane, one row per wave)

// rows [0, n) of an image in `nchunks` chunks of `per` rows (the last one shorter, never empty)
inline void hp_split(int n, int& nchunks, int& per) {
  const int want = (n + HP_ROWS - 1) / HP_ROWS;
  per = (n + want - 1) / want;
  nchunks = (n + per - 1) / per;
}

template <bool HALF>
__device__ __forceinline__ float row_sum(float v) {
  if constexpr (HALF) return half_wave_sum(v); else return wave_sum(v);
}

// ws[(b * nchunks + c), :] = sum over the chunk's rows of xhat (NORM) or x, one workgroup per (image, chunk).
// HALF: 32 lanes per row and two rows per wave (D <= 512), else 64 lanes per row; NV float4 per lane.
template <int NV, bool HALF, bool NORM>
__global__ __launch_bounds__(256) void pool_partial_kernel(const float* __restrict__ x, double* __restrict__ ws,
                                                           float* __restrict__ mean, float* __restrict__ rstd, int L,
                                                           int first, int D, int nchunks, int per, float eps) {
  constexpr int LPR = HALF ? 32 : 64, SLOTS = 256 / LPR;
  __shared__ double red[SLOTS][LPR * 4 * NV];
  const int b = blockIdx.x / nchunks, c = blockIdx.x - b * nchunks;
  const int n = L - first;
  const int r0 = c * per, r1 = min(n, r0 + per);          // pooled rows [r0, r1) of image b
  const int slot = threadIdx.x / LPR, l = threadIdx.x % LPR;
  const int nchunk = D >> 2;
  double acc[NV][4];
#pragma unroll
  for (int k = 0; k < NV; ++k) acc[k][0] = acc[k][1] = acc[k][2] = acc[k][3] = 0.0;
  const int iters = (r1 - r0 + SLOTS - 1) / SLOTS;
  for (int it = 0; it < iters; ++it) {
    const int r = r0 + it * SLOTS + slot;
    const bool live = r < r1;
    const int rr = live ? r : r1 - 1;                     // a dead slot recomputes the chunk's last row and adds nothing
    const float* xr = x + ((long)b * L + first + rr) * D;
    float4 v[NV];
    float s = 0.f;
#pragma unroll
    for (int k = 0; k < NV; ++k) {
      const int i4 = l + LPR * k;
      v[k] = (i4 < nchunk) ? *reinterpret_cast<const float4*>(xr + 4 * i4) : make_float4(0.f, 0.f, 0.f, 0.f);
      s += (v[k].x + v[k].y) + (v[k].z + v[k].w);
    }
    if constexpr (NORM) {
      const float mu = row_sum<HALF>(s) / (float)D;
      float q = 0.f;
#pragma unroll
      for (int k = 0; k < NV; ++k) {
        if (l + LPR * k < nchunk) {
          const float a = v[k].x - mu, bb = v[k].y - mu, cc = v[k].z - mu, d = v[k].w - mu;
          q += (a * a + bb * bb) + (cc * cc + d * d);
        }
      }
      const float rs = rsqrtf(row_sum<HALF>(q) / (float)D + eps);
      if (live) {
        if (l == 0) {
          mean[(long)b * n + r] = mu;
          rstd[(long)b * n + r] = rs;
        }
#pragma unroll
        for (int k = 0; k < NV; ++k) {
          if (l + LPR * k < nchunk) {
            acc[k][0] += (double)((v[k].x - mu) * rs); acc[k][1] += (double)((v[k].y - mu) * rs);
            acc[k][2] += (double)((v[k].z - mu) * rs); acc[k][3] += (double)((v[k].w - mu) * rs);
          }
        }
      }
    } else if (live) {
#pragma unroll
      for (int k = 0; k < NV; ++k) {
        acc[k][0] += (double)v[k].x; acc[k][1] += (double)v[k].y; acc[k][2] += (double)v[k].z; acc[k][3] += (double)v[k].w;
      }
    }
  }
  // fold the slots of the workgroup in slot order, then one partial row per workgroup
#pragma unroll
  for (int k = 0; k < NV; ++k) {
    const int i4 = l + LPR * k;
    if (i4 < nchunk) {
      *reinterpret_cast<double2*>(&red[slot][4 * i4]) = make_double2(acc[k][0], acc[k][1]);
      *reinterpret_cast<double2*>(&red[slot][4 * i4 + 2]) = make_double2(acc[k][2], acc[k][3]);
    }
  }
  __syncthreads();
  for (int i = threadIdx.x; i < D; i += 256) {
    double t = red[0][i];
#pragma unroll
    for (int k = 1; k < SLOTS; ++k) t += red[k][i];
    ws[(long)blockIdx.x * D + i] = t;
  }
}

// s[b] = (sum of image b's chunk partials, in chunk order) / n; with gamma: y[b] = s[b] * gamma + beta, else y[b] = s[b]
__global__ __launch_bounds__(256) void pool_fold_kernel(const double* __restrict__ ws, const float* __restrict__ gamma,
                                                        const float* __restrict__ beta, float* __restrict__ y,
                                                        float* __restrict__ s, int nchunks, int D, int n) {
  const int b = blockIdx.x, i = blockIdx.y * 256 + threadIdx.x;
  if (i >= D) return;
  const double* w = ws + (long)b * nchunks * D + i;
  double acc = w[0];
  for (int c = 1; c < nchunks; ++c) acc += w[(long)c * D];
  const float t = (float)(acc / (double)n);
  if (gamma) {
    s[(long)b * D + i] = t;
    y[(long)b * D + i] = t * gamma[i] + beta[i];
  } else {
    y[(long)b * D + i] = t;
  }
}

// dx[b, r] = LayerNorm input gradient of the upstream row (dy[b] / n) for r >= first, zeros below; one workgroup per
// (image, chunk of ALL L rows).  The upstream row is the same for every row of an image: it stays in registers.
template <int NV, bool HALF>
__global__ __launch_bounds__(256) void ln_meanpool_bwd_kernel(const float* __restrict__ dy, const float* __restrict__ x,
                                                              const float* __restrict__ gamma,
                                                              const float* __restrict__ mean,
                                                              const float* __restrict__ rstd, float* __restrict__ dx,
                                                              int L, int first, int D, int nchunks, int per) {
  constexpr int LPR = HALF ? 32 : 64, SLOTS = 256 / LPR;
  const int b = blockIdx.x / nchunks, c = blockIdx.x - b * nchunks;
  const int n = L - first;
  const int r0 = c * per, r1 = min(L, r0 + per);          // rows [r0, r1) of image b, CLS rows included
  const int slot = threadIdx.x / LPR, l = threadIdx.x % LPR;
  const int nchunk = D >> 2;
  const float invD = 1.0f / (float)D, fn = (float)n;
  float4 g[NV];
  float s1 = 0.f;
#pragma unroll
  for (int k = 0; k < NV; ++k) {
    const int i4 = l + LPR * k;
    if (i4 < nchunk) {
      const float4 d = *reinterpret_cast<const float4*>(dy + (long)b * D + 4 * i4);
      const float4 gm = *reinterpret_cast<const float4*>(gamma + 4 * i4);
      g[k] = make_float4(__fdiv_rn(d.x, fn) * gm.x, __fdiv_rn(d.y, fn) * gm.y, __fdiv_rn(d.z, fn) * gm.z,
                         __fdiv_rn(d.w, fn) * gm.w);
    } else {
      g[k] = make_float4(0.f, 0.f, 0.f, 0.f);
    }
    s1 += (g[k].x + g[k].y) + (g[k].z + g[k].w);
  }
  const float c1 = row_sum<HALF>(s1) * invD;
  const int iters = (r1 - r0 + SLOTS - 1) / SLOTS;
  for (int it = 0; it < iters; ++it) {
    const int r = r0 + it * SLOTS + slot;
    const bool live = r < r1;
    const int rr = live ? r : r1 - 1;
    const bool pooled = rr >= first;
    const int rp = pooled ? rr : first;                   // a row below `first` computes row `first` and stores zeros
    const float mu = mean[(long)b * n + (rp - first)], rs = rstd[(long)b * n + (rp - first)];
    const float* xr = x + ((long)b * L + rp) * D;
    float4 xh[NV];
    float s2 = 0.f;
#pragma unroll
    for (int k = 0; k < NV; ++k) {
      const int i4 = l + LPR * k;
      if (i4 < nchunk) {
        const float4 xv = *reinterpret_cast<const float4*>(xr + 4 * i4);
        xh[k] = make_float4((xv.x - mu) * rs, (xv.y - mu) * rs, (xv.z - mu) * rs, (xv.w - mu) * rs);
        s2 += (g[k].x * xh[k].x + g[k].y * xh[k].y) + (g[k].z * xh[k].z + g[k].w * xh[k].w);
      } else {
        xh[k] = make_float4(0.f, 0.f, 0.f, 0.f);
      }
    }
    const float c2 = row_sum<HALF>(s2) * invD;
    if (live) {
      float* dxr = dx + ((long)b * L + rr) * D;
#pragma unroll
      for (int k = 0; k < NV; ++k) {
        const int i4 = l + LPR * k;
        if (i4 < nchunk) {
          float4 o = make_float4(rs * (g[k].x - c1 - xh[k].x * c2), rs * (g[k].y - c1 - xh[k].y * c2),
                                 rs * (g[k].z - c1 - xh[k].z * c2), rs * (g[k].w - c1 - xh[k].w * c2));
          if (!pooled) o = make_float4(0.f, 0.f, 0.f, 0.f);
          *reinterpret_cast<float4*>(dxr + 4 * i4) = o;
        }
      }
    }
  }
}

// dgamma (+)= sum_b dy[b] * s[b], dbeta (+)= sum_b dy[b]: 64 columns per workgroup, the B rows dealt to its 4 waves
__global__ __launch_bounds__(256) void ln_meanpool_dgb_kernel(const float* __restrict__ dy, const float* __restrict__ s,
                                                              float* __restrict__ dgamma, float* __restrict__ dbeta,
                                                              int B, int D, int accumulate) {
  __shared__ float red[2][4][64];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int col = blockIdx.x * 64 + lane;
  float ag = 0.f, ab = 0.f;
  if (col < D) {
    for (int b = wave; b < B; b += 4) {
      const float d = dy[(long)b * D + col];
      ag += d * s[(long)b * D + col];
      ab += d;
    }
  }
  red[0][wave][lane] = ag;
  red[1][wave][lane] = ab;
  __syncthreads();
  if (wave == 0 && col < D) {
    const float tg = (red[0][0][lane] + red[0][1][lane]) + (red[0][2][lane] + red[0][3][lane]);
    const float tb = (red[1][0][lane] + red[1][1][lane]) + (red[1][2][lane] + red[1][3][lane]);
    dgamma[col] = accumulate ? dgamma[col] + tg : tg;
    dbeta[col] = accumulate ? dbeta[col] + tb : tb;
  }
}

// dx[b, r] = dp[b] / n for r >= first, zeros below: one wave per row, one workgroup per (image, chunk of ALL L rows)
__global__ __launch_bounds__(256) void meanpool_bwd_kernel(const float* __restrict__ dp, float* __restrict__ dx, int L,
                                                           int first, int D, int nchunks, int per) {
  const int b = blockIdx.x / nchunks, c = blockIdx.x - b * nchunks;
  const int r0 = c * per, r1 = min(L, r0 + per);
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int nchunk = D >> 2;
  const float fn = (float)(L - first);
  for (int i4 = lane; i4 < nchunk; i4 += 64) {
    const float4 d = *reinterpret_cast<const float4*>(dp + (long)b * D + 4 * i4);
    const float4 o = make_float4(__fdiv_rn(d.x, fn), __fdiv_rn(d.y, fn), __fdiv_rn(d.z, fn), __fdiv_rn(d.w, fn));
    for (int r = r0 + wave; r < r1; r += 4)
      *reinterpret_cast<float4*>(dx + ((long)b * L + r) * D + 4 * i4) = r >= first ? o : make_float4(0.f, 0.f, 0.f, 0.f);
  }
}

inline bool aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }

// FAVIT_OK, or why this geometry is refused; `rows` is what the launch splits into chunks (n forward, L backward)
int hp_check(int32_t B, int32_t L, int32_t first, int32_t D, int rows, int& nchunks, int& per) {
  if (B <= 0 || L <= 0 || first < 0 || first >= L || D <= 0) return FAVIT_ERR_INVALID;
  if ((D & 3) || D > HP_MAX_D) return FAVIT_ERR_UNSUPPORTED;
  hp_split(rows, nchunks, per);
  if ((long)B * nchunks > 0x7fffffffL) return FAVIT_ERR_UNSUPPORTED;
  return FAVIT_OK;
}

// the width classes of favit_layernorm_fwd: two rows per wave up to D = 512, one beyond
#define HP_DISPATCH(D, MACRO)                                                  \
  do {                                                                         \
    if ((D) <= 512) {                                                          \
      const int nv__ = ((D) + 127) / 128;                                      \
      if (nv__ <= 1) { MACRO(1, true); }                                       \
      else if (nv__ == 2) { MACRO(2, true); }                                  \
      else if (nv__ == 3) { MACRO(3, true); }                                  \
      else { MACRO(4, true); }                                                 \
    } else {                                                                   \
      const int nv__ = ((D) + 255) / 256;                                      \
      if (nv__ <= 3) { MACRO(3, false); }                                      \
      else if (nv__ == 4) { MACRO(4, false); }                                 \
      else { MACRO(8, false); }                                                \
    }                                                                          \
  } while (0)

template <bool NORM>
int pool_fwd_impl(const float* x, const float* gamma, const float* beta, float* y, float* s, float* mean, float* rstd,
                  void* ws, int32_t B, int32_t L, int32_t first, int32_t D, float eps, void* stream) {
  if (!x || !y || !ws || (NORM && (!gamma || !beta || !s || !mean || !rstd))) return FAVIT_ERR_INVALID;
  int nchunks, per;
  const int rc = hp_check(B, L, first, D, L - first, nchunks, per);
  if (rc != FAVIT_OK) return rc;
  if (!aligned16(x) || !aligned16(ws) || (NORM && (!aligned16(gamma) || !aligned16(beta)))) return FAVIT_ERR_ALIGN;
  hipStream_t st = as_stream(stream);
  const dim3 grid((unsigned)((long)B * nchunks));
#define HP_FWD(NV, HALF)                                                                                          \
  hipLaunchKernelGGL((pool_partial_kernel<NV, HALF, NORM>), grid, dim3(256), 0, st, x, (double*)ws, mean, rstd,  \
                     (int)L, (int)first, (int)D, nchunks, per, eps)
  HP_DISPATCH(D, HP_FWD);
#undef HP_FWD
  FAVIT_CHECK_LAUNCH();
  hipLaunchKernelGGL(pool_fold_kernel, dim3((unsigned)B, (unsigned)((D + 255) / 256)), dim3(256), 0, st,
                     (const double*)ws, NORM ? gamma : nullptr, beta, y, s, nchunks, (int)D, (int)(L - first));
  FAVIT_CHECK_LAUNCH();
  return FAVIT_OK;
}

}  // namespace

extern "C" int64_t favit_head_pool_workspace(int32_t B, int32_t L, int32_t first, int32_t D) {
  int nchunks, per;
  const int rc = hp_check(B, L, first, D, L - first, nchunks, per);
  if (rc != FAVIT_OK) return rc;
  return (int64_t)B * nchunks * D * (int64_t)sizeof(double);
}

extern "C" int favit_ln_meanpool_fwd(const float* x, const float* gamma, const float* beta, float* y, float* s,
                                     float* mean, float* rstd, void* ws, int32_t B, int32_t L, int32_t first,
                                     int32_t D, float eps, void* stream) {
  return pool_fwd_impl<true>(x, gamma, beta, y, s, mean, rstd, ws, B, L, first, D, eps, stream);
}

extern "C" int favit_meanpool_fwd(const float* x, float* p, void* ws, int32_t B, int32_t L, int32_t first, int32_t D,
                                  void* stream) {
  return pool_fwd_impl<false>(x, nullptr, nullptr, p, nullptr, nullptr, nullptr, ws, B, L, first, D, 0.f, stream);
}

extern "C" int favit_ln_meanpool_bwd(const float* dy, const float* x, const float* gamma, const float* s,
                                     const float* mean, const float* rstd, float* dx, float* dgamma, float* dbeta,
                                     int32_t accumulate, int32_t B, int32_t L, int32_t first, int32_t D, void* stream) {
  if (!dy || !x || !gamma || !s || !mean || !rstd || !dx || (dgamma == nullptr) != (dbeta == nullptr))
    return FAVIT_ERR_INVALID;
  int nchunks, per;
  const int rc = hp_check(B, L, first, D, L, nchunks, per);
  if (rc != FAVIT_OK) return rc;
  if (!aligned16(dy) || !aligned16(x) || !aligned16(gamma) || !aligned16(dx)) return FAVIT_ERR_ALIGN;
  hipStream_t st = as_stream(stream);
  const dim3 grid((unsigned)((long)B * nchunks));
#define HP_BWD(NV, HALF)                                                                                           \
  hipLaunchKernelGGL((ln_meanpool_bwd_kernel<NV, HALF>), grid, dim3(256), 0, st, dy, x, gamma, mean, rstd, dx,     \
                     (int)L, (int)first, (int)D, nchunks, per)
  HP_DISPATCH(D, HP_BWD);
#undef HP_BWD
  FAVIT_CHECK_LAUNCH();
  if (dgamma) {
    hipLaunchKernelGGL(ln_meanpool_dgb_kernel, dim3((unsigned)((D + 63) / 64)), dim3(256), 0, st, dy, s, dgamma, dbeta,
                       (int)B, (int)D, (int)accumulate);
    FAVIT_CHECK_LAUNCH();
  }
  return FAVIT_OK;
}

extern "C" int favit_meanpool_bwd(const float* dp, float* dx, int32_t B, int32_t L, int32_t first, int32_t D,
                                  void* stream) {
  if (!dp || !dx) return FAVIT_ERR_INVALID;
  int nchunks, per;
  const int rc = hp_check(B, L, first, D, L, nchunks, per);
  if (rc != FAVIT_OK) return rc;
  if (!aligned16(dp) || !aligned16(dx)) return FAVIT_ERR_ALIGN;
  hipLaunchKernelGGL(meanpool_bwd_kernel, dim3((unsigned)((long)B * nchunks)), dim3(256), 0, as_stream(stream), dp, dx,
                     (int)L, (int)first, (int)D, nchunks, per);
  FAVIT_CHECK_LAUNCH();
  return FAVIT_OK;
}
