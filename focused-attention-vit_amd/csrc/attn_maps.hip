// Attention maps: the probabilities the fused attention kernels never write, recomputed from a stored qkv, and
// attention rollout over a stack of head-mean maps in one launch (favit.h: favit_mhla_attn_probs, favit_sdpa_probs,
// favit_attn_rollout).  Small VALU kernels: no MFMA, no atomics, plain vector stores.
#include "common.h"
#include <math.h>

namespace {

constexpr int MAPS_MAX_W = FAVIT_MAPS_MAX_WINDOW;

// ---------------------------------------------------------------------------------------------------------------
// Window probabilities.  Eight consecutive lanes share one token row (b, i) and walk its heads in ascending order;
// lane g of the eight holds hd / 8 dims of q and of each of the W keys, the partial scores are summed inside the
// group (DPP, common.h) and every lane of the group ends up with the W probabilities.  Lanes of rows past B * L
// compute row 0 again (the DPP sum wants whole groups) and store nothing.
template <typename T, int HD>
__global__ __launch_bounds__(256) void mhla_probs_kernel(const T* __restrict__ qkv, float* __restrict__ probs,
                                                         const uint8_t* __restrict__ mask, int B, int L, int H, int W,
                                                         float scale, int head_mean) {
  constexpr int DPL = HD / 8;
  const long rows = (long)B * L;
  const long grp = ((long)blockIdx.x * blockDim.x + threadIdx.x) >> 3;
  const int g = threadIdx.x & 7;
  const bool live = grp < rows;
  const long row = live ? grp : 0;
  const int b = (int)(row / L), i = (int)(row - (long)b * L);
  const int hw = W / 2;
  const long D = (long)H * HD, ld = 3 * D;
  int key[MAPS_MAX_W];
  bool keep[MAPS_MAX_W];
#pragma unroll
  for (int w = 0; w < MAPS_MAX_W; ++w) {
    key[w] = w < W ? win_idx(i, w, L, W, hw) : 0;
    keep[w] = w < W && (!mask || mask[((long)b * L + i) * L + key[w]] != 0);
  }
  float mean[MAPS_MAX_W];
#pragma unroll
  for (int w = 0; w < MAPS_MAX_W; ++w) mean[w] = 0.f;
  const float inv_h = 1.0f / (float)H;
  for (int h = 0; h < H; ++h) {
    float q[DPL];
    vload<T, DPL>(qkv + row * ld + (long)h * HD + g * DPL, q);
    float s[MAPS_MAX_W];
    float m = -INFINITY;
#pragma unroll
    for (int w = 0; w < MAPS_MAX_W; ++w) {
      s[w] = 0.f;
      if (w < W) {
        float k[DPL];
        vload<T, DPL>(qkv + ((long)b * L + key[w]) * ld + D + (long)h * HD + g * DPL, k);
        float acc = 0.f;
#pragma unroll
        for (int d = 0; d < DPL; ++d) acc = fmaf(q[d], k[d], acc);
        s[w] = dpp_sum8(acc) * scale;
        if (keep[w]) m = fmaxf(m, s[w]);
      }
    }
    float sum = 0.f;
#pragma unroll
    for (int w = 0; w < MAPS_MAX_W; ++w) {
      s[w] = keep[w] ? expf(s[w] - m) : 0.f;       // (a row without a live slot: every s is 0, m is never used)
      sum += s[w];
    }
    const float inv = sum > 0.f ? 1.0f / sum : 0.f;
    if (head_mean) {
#pragma unroll
      for (int w = 0; w < MAPS_MAX_W; ++w) mean[w] += s[w] * inv;
    } else if (live) {
      float* o = probs + (((long)b * H + h) * L + i) * W;
#pragma unroll
      for (int w = 0; w < MAPS_MAX_W; ++w)
        if (w < W && (w & 7) == g) o[w] = s[w] * inv;
    }
  }
  if (head_mean && live) {
    float* o = probs + row * W;
#pragma unroll
    for (int w = 0; w < MAPS_MAX_W; ++w)
      if (w < W && (w & 7) == g) o[w] = mean[w] * inv_h;
  }
}

template <typename T, int HD>
int launch_mhla_probs(const void* qkv, float* probs, const uint8_t* mask, int B, int L, int H, int W, int head_mean,
                      hipStream_t st) {
  const long groups = (long)B * L;
  const long blocks = (groups + 31) / 32;            // 256 threads = 32 groups of eight lanes
  hipLaunchKernelGGL((mhla_probs_kernel<T, HD>), dim3((unsigned)blocks), dim3(256), 0, st, (const T*)qkv, probs, mask,
                     B, L, H, W, (float)(1.0 / sqrt((double)HD)), head_mean);
  FAVIT_CHECK_LAUNCH();
  return FAVIT_OK;
}

template <typename T>
int dispatch_mhla_probs(const void* qkv, float* probs, const uint8_t* mask, int B, int L, int H, int hd, int W,
                        int head_mean, hipStream_t st) {
  switch (hd) {
    case 16: return launch_mhla_probs<T, 16>(qkv, probs, mask, B, L, H, W, head_mean, st);
    case 32: return launch_mhla_probs<T, 32>(qkv, probs, mask, B, L, H, W, head_mean, st);
    case 64: return launch_mhla_probs<T, 64>(qkv, probs, mask, B, L, H, W, head_mean, st);
    case 128: return launch_mhla_probs<T, 128>(qkv, probs, mask, B, L, H, W, head_mean, st);
  }
  return FAVIT_ERR_UNSUPPORTED;
}

// ---------------------------------------------------------------------------------------------------------------
// Dense probabilities.  One wave per query row (b, i), four rows per workgroup.  The wave keeps the row's q of every
// head in LDS as fp32 [D], lane l owns the keys l, l + 64, ...  Pass 1 leaves per head the maximum and the reciprocal
// of the sum of exp (online, then folded across the wave) in LDS; pass 2 recomputes each score and writes
// exp(s - m) / sum, or its mean over the heads in ascending order.  LDS per wave: D + 2 H floats.
template <typename T>
__device__ __forceinline__ float dense_score(const float* __restrict__ q, const T* __restrict__ k, int hd) {
  float acc = 0.f;
  for (int d = 0; d < hd; d += 8) {
    float kv[8];
    vload<T, 8>(k + d, kv);
#pragma unroll
    for (int e = 0; e < 8; ++e) acc = fmaf(q[d + e], kv[e], acc);
  }
  return acc;
}

template <typename T>
__global__ __launch_bounds__(256) void sdpa_probs_kernel(const T* __restrict__ qkv, float* __restrict__ probs,
                                                         const uint8_t* __restrict__ key_keep, int B, int L, int H,
                                                         int hd, float scale, int head_mean) {
  extern __shared__ float lds[];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const long D = (long)H * hd, ld = 3 * D;
  float* q = lds + (long)wave * (D + 2 * H);
  float* mx = q + D;
  float* inv = mx + H;
  const long grow = (long)blockIdx.x * 4 + wave;
  const bool live = grow < (long)B * L;              // (a wave past the last row computes row 0 and stores nothing)
  const long row = live ? grow : 0;
  const int b = (int)(row / L), i = (int)(row - (long)b * L);
  const T* qrow = qkv + row * ld;
  for (int d = lane; d < D; d += 64) q[d] = to_f32(qrow[d]);
  __syncthreads();
  const T* kbase = qkv + (long)b * L * ld + D;
  const uint8_t* kk = key_keep ? key_keep + (long)b * L : nullptr;
  for (int h = 0; h < H; ++h) {
    float m = -INFINITY, l = 0.f;
    for (int j = lane; j < L; j += 64) {
      if (kk && kk[j] == 0) continue;
      const float s = dense_score<T>(q + h * hd, kbase + (long)j * ld + h * hd, hd) * scale;
      const float mn = fmaxf(m, s);
      l = l * expf(m - mn) + expf(s - mn);           // (m = -inf only while l = 0: exp(-inf) = 0)
      m = mn;
    }
    const float mw = wave_max(m);
    l = wave_sum(m == -INFINITY ? 0.f : l * expf(m - mw));
    if (lane == 0) {
      mx[h] = l > 0.f ? mw : 0.f;
      inv[h] = l > 0.f ? 1.0f / l : 0.f;
    }
  }
  __syncthreads();
  if (!live) return;
  const float inv_h = 1.0f / (float)H;
  for (int j = lane; j < L; j += 64) {
    const bool keep = !kk || kk[j] != 0;
    float mean = 0.f;
    for (int h = 0; h < H; ++h) {
      float p = 0.f;
      if (keep) p = expf(dense_score<T>(q + h * hd, kbase + (long)j * ld + h * hd, hd) * scale - mx[h]) * inv[h];
      if (head_mean) mean += p;
      else probs[(((long)b * H + h) * L + i) * L + j] = p;
    }
    if (head_mean) probs[row * L + j] = mean * inv_h;
  }
}

// ---------------------------------------------------------------------------------------------------------------
// Rollout.  One workgroup per image; r lives in LDS as two buffers of L floats that swap roles after every block, so
// the whole stack is one launch and r never visits memory.  Each thread owns the keys j = t, t + 1024, ... and GATHERS
// what flows into key j in a fixed order, so there are no atomics and the same inputs give the same bits.
struct RolloutTable {
  const float* probs[FAVIT_ROLLOUT_MAX_LAYERS];
  int widths[FAVIT_ROLLOUT_MAX_LAYERS];
};

// sum_i r[i] * P[i -> j] of a banded block, P = [L, W] of one image.  Row i holds key j in a slot of its own when
// |i - j| <= W/2 (in ascending i below); the pad copies of the short windows follow: those that start at 0 repeat
// key L - 1 in their last slots, those cut at L repeat key 0 in their first slots (win_idx, common.h).
__device__ __forceinline__ float rollout_gather_band(const float* __restrict__ r, const float* __restrict__ P, int j,
                                                     int L, int W) {
  const int h = W / 2;
  float acc = 0.f;
  const int i0 = max(0, j - h), i1 = min(L - 1, j + h);
  for (int i = i0; i <= i1; ++i) {
    const int lo = max(0, i - h), n = min(L, i + h + 1) - lo;
    const int w = (n == W || lo == 0) ? j - lo : (W - n) + (j - lo);
    acc = fmaf(r[i], P[(long)i * W + w], acc);
  }
  if (j == L - 1) {                                  // windows that start at 0 and are short: slots n .. W - 1
    for (int i = 0; i <= min(h, L - 1); ++i) {
      const int n = min(L, i + h + 1);
      for (int w = n; w < W; ++w) acc = fmaf(r[i], P[(long)i * W + w], acc);
    }
  }
  if (j == 0) {                                      // windows cut at L that do not start at 0: slots 0 .. W - n - 1
    for (int i = max(h + 1, L - h); i < L; ++i) {
      const int n = L - (i - h);
      for (int w = 0; w < W - n; ++w) acc = fmaf(r[i], P[(long)i * W + w], acc);
    }
  }
  return acc;
}

__global__ __launch_bounds__(1024) void rollout_kernel(RolloutTable tab, int n, float* __restrict__ out, int cls_row,
                                                       int L, float residual) {
  extern __shared__ float lds[];
  float* cur = lds;
  float* nxt = lds + L;
  const int b = blockIdx.x;
  for (int j = threadIdx.x; j < L; j += blockDim.x) cur[j] = j == cls_row ? 1.0f : 0.0f;
  __syncthreads();
  const float mix = 1.0f - residual;
  for (int k = n - 1; k >= 0; --k) {
    const int W = tab.widths[k];
    if (W > 0) {
      const float* P = tab.probs[k] + (long)b * L * W;
      for (int j = threadIdx.x; j < L; j += blockDim.x)
        nxt[j] = residual * cur[j] + mix * rollout_gather_band(cur, P, j, L, W);
    } else {
      const float* P = tab.probs[k] + (long)b * L * L;
      for (int j = threadIdx.x; j < L; j += blockDim.x) {
        float acc = 0.f;
        for (int i = 0; i < L; ++i) {
          const float ri = cur[i];                   // (the same for every thread: rows without mass are skipped)
          if (ri != 0.f) acc = fmaf(ri, P[(long)i * L + j], acc);
        }
        nxt[j] = residual * cur[j] + mix * acc;
      }
    }
    __syncthreads();
    float* t = cur;
    cur = nxt;
    nxt = t;
  }
  for (int j = threadIdx.x; j < L; j += blockDim.x) out[(long)b * L + j] = cur[j];
}

}  // namespace

extern "C" int favit_mhla_attn_probs(const void* qkv, float* probs, const uint8_t* mask, int32_t B, int32_t L,
                                     int32_t H, int32_t hd, int32_t W, int dtype, int32_t head_mean, void* stream) {
  if (!qkv || !probs || B < 1 || L < 1 || H < 1 || hd < 1) return FAVIT_ERR_INVALID;
  if (W < 1 || W % 2 == 0) return FAVIT_ERR_INVALID;
  if (dtype != FAVIT_F32 && dtype != FAVIT_BF16) return FAVIT_ERR_INVALID;
  if (head_mean != 0 && head_mean != 1) return FAVIT_ERR_INVALID;
  if (W > MAPS_MAX_W || (hd != 16 && hd != 32 && hd != 64 && hd != 128)) return FAVIT_ERR_UNSUPPORTED;
  if ((long)B * L > 0x7fffffffL / 8) return FAVIT_ERR_UNSUPPORTED;    // (eight lanes per row in a 32-bit grid)
  if (reinterpret_cast<uintptr_t>(qkv) & 15) return FAVIT_ERR_ALIGN;
  hipStream_t st = as_stream(stream);
  return dtype == FAVIT_F32 ? dispatch_mhla_probs<float>(qkv, probs, mask, B, L, H, hd, W, head_mean, st)
                            : dispatch_mhla_probs<bf16_t>(qkv, probs, mask, B, L, H, hd, W, head_mean, st);
}

extern "C" int favit_sdpa_probs(const void* qkv, float* probs, const uint8_t* key_keep, int32_t B, int32_t L,
                                int32_t H, int32_t hd, int dtype, float scale, int32_t head_mean, void* stream) {
  if (!qkv || !probs || B < 1 || L < 1 || H < 1 || hd < 1) return FAVIT_ERR_INVALID;
  if (dtype != FAVIT_F32 && dtype != FAVIT_BF16) return FAVIT_ERR_INVALID;
  if (head_mean != 0 && head_mean != 1) return FAVIT_ERR_INVALID;
  if (!(scale > 0.f) || !isfinite(scale)) return FAVIT_ERR_INVALID;
  const long per_wave = (long)H * hd + 2L * H;
  if (hd % 16 != 0 || per_wave > FAVIT_SDPA_PROBS_MAX_WAVE_FLOATS) return FAVIT_ERR_UNSUPPORTED;
  if (((long)B * L + 3) / 4 > 0x7fffffffL) return FAVIT_ERR_UNSUPPORTED;
  if (reinterpret_cast<uintptr_t>(qkv) & 15) return FAVIT_ERR_ALIGN;
  hipStream_t st = as_stream(stream);
  const unsigned blocks = (unsigned)(((long)B * L + 3) / 4);
  const size_t bytes = (size_t)(4 * per_wave) * sizeof(float);
  if (dtype == FAVIT_F32)
    hipLaunchKernelGGL(sdpa_probs_kernel<float>, dim3(blocks), dim3(256), bytes, st, (const float*)qkv, probs, key_keep,
                       (int)B, (int)L, (int)H, (int)hd, scale, (int)head_mean);
  else
    hipLaunchKernelGGL(sdpa_probs_kernel<bf16_t>, dim3(blocks), dim3(256), bytes, st, (const bf16_t*)qkv, probs,
                       key_keep, (int)B, (int)L, (int)H, (int)hd, scale, (int)head_mean);
  FAVIT_CHECK_LAUNCH();
  return FAVIT_OK;
}

extern "C" int favit_attn_rollout(int32_t n, const float* const* probs, const int32_t* widths, float* out,
                                  int32_t cls_row, int32_t B, int32_t L, float residual, void* stream) {
  if (!probs || !widths || !out || n < 1 || n > FAVIT_ROLLOUT_MAX_LAYERS) return FAVIT_ERR_INVALID;
  if (B < 1 || L < 1 || cls_row < 0 || cls_row >= L) return FAVIT_ERR_INVALID;
  if (!(residual >= 0.f && residual <= 1.f)) return FAVIT_ERR_INVALID;
  RolloutTable tab;
  for (int k = 0; k < FAVIT_ROLLOUT_MAX_LAYERS; ++k) {
    tab.probs[k] = nullptr;
    tab.widths[k] = 0;
  }
  for (int k = 0; k < n; ++k) {
    if (!probs[k] || widths[k] < 0 || (widths[k] > 0 && widths[k] % 2 == 0)) return FAVIT_ERR_INVALID;
    tab.probs[k] = probs[k];
    tab.widths[k] = widths[k];
  }
  if (L > FAVIT_ROLLOUT_MAX_L) return FAVIT_ERR_UNSUPPORTED;
  const int lds = 2 * L * (int)sizeof(float);
  if (lds > 65536) favit_ensure_dyn_lds(reinterpret_cast<const void*>(rollout_kernel), lds);
  hipLaunchKernelGGL(rollout_kernel, dim3((unsigned)B), dim3(1024), (size_t)lds, as_stream(stream),
                     tab, (int)n, out, (int)cls_row, (int)L, residual);
  FAVIT_CHECK_LAUNCH();
  return FAVIT_OK;
}
