// Stochastic depth (DropPath) on the fp32 residual stream: per SAMPLE, a residual branch is
// dropped with probability p and the survivors are scaled by 1 / (1 - p).  Two row-streaming kernels, bound by HBM:
//   favit_drop_path_add   out = x + (keep(b) ? scale * y : 0)          (behind a proj / fc2 GEMM without residual)
//   favit_drop_path_bwd   g_lp = keep(b) ? scale * g : 0, in the compute dtype, optionally under the element mask of
//                         the branch's output dropout (what favit_layernorm_bwd's low-precision copy carries elsewhere)
// The draw is the library's dropout draw (common.h) with the SAMPLE number as its index -- the same draw in every row
// layout, so a CLS-only encoder draws the masks of the dense one -- and the dropout epoch word mixed into the seed.
// Access: one thread owns 8 consecutive columns of one row (D % 8 == 0): fp32 as two 16-byte accesses, bf16 as one.
// Grid as the row cuts of norm_elem.hip: x walks the (row, 8-column group) pairs of one sample with 32-bit index
// math, y the samples; keep(b) is uniform over a workgroup, and a dropped sample's branch rows are never read.
#include "common.h"

namespace {

struct f32x8 { float4 lo, hi; };

__device__ __forceinline__ f32x8 load8(const float* p) {
  f32x8 v;
  v.lo = *reinterpret_cast<const float4*>(p);
  v.hi = *reinterpret_cast<const float4*>(p + 4);
  return v;
}
__device__ __forceinline__ f32x8 load8(const bf16_t* p) {
  const bf16x8 t = *reinterpret_cast<const bf16x8*>(p);
  f32x8 v;
  v.lo = make_float4((float)t[0], (float)t[1], (float)t[2], (float)t[3]);
  v.hi = make_float4((float)t[4], (float)t[5], (float)t[6], (float)t[7]);
  return v;
}
__device__ __forceinline__ void store8(float* p, const f32x8& v) {
  *reinterpret_cast<float4*>(p) = v.lo;
  *reinterpret_cast<float4*>(p + 4) = v.hi;
}
__device__ __forceinline__ void store8(bf16_t* p, const f32x8& v) {
  bf16x8 t;
  t[0] = (bf16_t)v.lo.x; t[1] = (bf16_t)v.lo.y; t[2] = (bf16_t)v.lo.z; t[3] = (bf16_t)v.lo.w;
  t[4] = (bf16_t)v.hi.x; t[5] = (bf16_t)v.hi.y; t[6] = (bf16_t)v.hi.z; t[7] = (bf16_t)v.hi.w;
  *reinterpret_cast<bf16x8*>(p) = t;
}

// x, y, out may alias (out == x, or out == y of the same dtype): every thread reads its 8 elements before it writes
// them, and no other thread touches them -- so none of the three is __restrict__.
template <typename YT>
__global__ __launch_bounds__(256) void drop_path_add_kernel(const float* x, const YT* y, float* out, int B, int n, int D,
                                                            uint32_t thresh, float scale, uint64_t seed,
                                                            const unsigned long long* epoch) {
  const unsigned dvn = (unsigned)D >> 3;
  const unsigned idx = blockIdx.x * 256u + threadIdx.x;
  if (idx >= (unsigned)n * dvn) return;                 // (n * D < 2^31: checked by the host)
  seed = favit_eff_seed(seed, epoch);
  for (int b = blockIdx.y; b < B; b += gridDim.y) {
    const long off = ((long)b * n) * D + (long)idx * 8;  // idx = r * dvn + dv -> r * D + 8 dv
    const bool keep = favit_keep(seed, (uint64_t)b, thresh);      // (uniform over the workgroup)
    if (!keep && out == x) continue;                               // in place: a dropped sample's rows stay as they are
    f32x8 o = load8(x + off);
    if (keep) {
      const f32x8 yv = load8(y + off);
      o.lo = make_float4(fmaf(scale, yv.lo.x, o.lo.x), fmaf(scale, yv.lo.y, o.lo.y), fmaf(scale, yv.lo.z, o.lo.z),
                         fmaf(scale, yv.lo.w, o.lo.w));
      o.hi = make_float4(fmaf(scale, yv.hi.x, o.hi.x), fmaf(scale, yv.hi.y, o.hi.y), fmaf(scale, yv.hi.z, o.hi.z),
                         fmaf(scale, yv.hi.w, o.hi.w));
    }
    store8(out + off, o);
  }
}

template <typename LpT>
__global__ __launch_bounds__(256) void drop_path_bwd_kernel(const float* __restrict__ g, LpT* __restrict__ g_lp, int B,
                                                            int n, int D, uint32_t thresh, float scale, uint64_t seed,
                                                            uint32_t lp_thresh, float lp_scale, uint64_t lp_seed,
                                                            const unsigned long long* epoch) {
  const unsigned dvn = (unsigned)D >> 3;
  const unsigned idx = blockIdx.x * 256u + threadIdx.x;
  if (idx >= (unsigned)n * dvn) return;
  seed = favit_eff_seed(seed, epoch);
  if (lp_thresh) lp_seed = favit_eff_seed(lp_seed, epoch);
  for (int b = blockIdx.y; b < B; b += gridDim.y) {
    const long off = ((long)b * n) * D + (long)idx * 8;
    f32x8 v;
    v.lo = v.hi = make_float4(0.f, 0.f, 0.f, 0.f);
    if (favit_keep(seed, (uint64_t)b, thresh)) {
      v = load8(g + off);
      v.lo.x *= scale; v.lo.y *= scale; v.lo.z *= scale; v.lo.w *= scale;
      v.hi.x *= scale; v.hi.y *= scale; v.hi.z *= scale; v.hi.w *= scale;
      if (lp_thresh) {         // the element mask of the branch's output dropout: element index row * D + col
        bool k0, k1, k2, k3, k4, k5, k6, k7;
        favit_keep2(lp_seed, (uint64_t)off, lp_thresh, k0, k1);
        favit_keep2(lp_seed, (uint64_t)off + 2, lp_thresh, k2, k3);
        favit_keep2(lp_seed, (uint64_t)off + 4, lp_thresh, k4, k5);
        favit_keep2(lp_seed, (uint64_t)off + 6, lp_thresh, k6, k7);
        v.lo.x = k0 ? v.lo.x * lp_scale : 0.f; v.lo.y = k1 ? v.lo.y * lp_scale : 0.f;
        v.lo.z = k2 ? v.lo.z * lp_scale : 0.f; v.lo.w = k3 ? v.lo.w * lp_scale : 0.f;
        v.hi.x = k4 ? v.hi.x * lp_scale : 0.f; v.hi.y = k5 ? v.hi.y * lp_scale : 0.f;
        v.hi.z = k6 ? v.hi.z * lp_scale : 0.f; v.hi.w = k7 ? v.hi.w * lp_scale : 0.f;
      }
    }
    store8(g_lp + off, v);
  }
}

// INVALID / UNSUPPORTED / 0 for the shape and rate both entry points share (one sample's elements are indexed with
// 32 bits; 16-byte accesses need D % 8 == 0 and 16-byte aligned bases)
inline int drop_path_args(int32_t B, int32_t n, int32_t D, float p) {
  if (B <= 0 || n <= 0 || D <= 0 || !(p >= 0.f && p < 1.f)) return FAVIT_ERR_INVALID;
  if (D % 8 != 0 || (long)n * D >= (1L << 31)) return FAVIT_ERR_UNSUPPORTED;
  return FAVIT_OK;
}

inline bool aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }

inline dim3 drop_path_grid(int32_t B, int32_t n, int32_t D) {
  return dim3((unsigned)(((long)n * (D / 8) + 255) / 256), (unsigned)(B < 65535 ? B : 65535));
}

}  // namespace

extern "C" int favit_drop_path_add(const float* x, const void* y, int y_dtype, float* out, int32_t B, int32_t n,
                                   int32_t D, float p, uint64_t seed, void* stream) {
  if (!x || !y || !out || (y_dtype != FAVIT_F32 && y_dtype != FAVIT_BF16)) return FAVIT_ERR_INVALID;
  const int rc = drop_path_args(B, n, D, p);
  if (rc != FAVIT_OK) return rc;
  if (!aligned16(x) || !aligned16(y) || !aligned16(out)) return FAVIT_ERR_ALIGN;
  const uint32_t th = dropout_threshold(p);
  const float scale = 1.0f / (1.0f - p);
  const dim3 grid = drop_path_grid(B, n, D);
  hipStream_t st = as_stream(stream);
  if (y_dtype == FAVIT_F32)
    hipLaunchKernelGGL((drop_path_add_kernel<float>), grid, dim3(256), 0, st, x, (const float*)y, out, B, n, D, th, scale,
                       seed, favit_dropout_epoch_ptr_());
  else
    hipLaunchKernelGGL((drop_path_add_kernel<bf16_t>), grid, dim3(256), 0, st, x, (const bf16_t*)y, out, B, n, D, th,
                       scale, seed, favit_dropout_epoch_ptr_());
  FAVIT_CHECK_LAUNCH();
  return FAVIT_OK;
}

extern "C" int favit_drop_path_bwd(const float* g, void* g_lp, int lp_dtype, int32_t B, int32_t n, int32_t D, float p,
                                   uint64_t seed, float lp_dropout_p, uint64_t lp_dropout_seed, void* stream) {
  if (!g || !g_lp || (lp_dtype != FAVIT_F32 && lp_dtype != FAVIT_BF16)) return FAVIT_ERR_INVALID;
  if (!(lp_dropout_p >= 0.f && lp_dropout_p < 1.f)) return FAVIT_ERR_INVALID;
  const int rc = drop_path_args(B, n, D, p);
  if (rc != FAVIT_OK) return rc;
  if (!aligned16(g) || !aligned16(g_lp)) return FAVIT_ERR_ALIGN;
  const uint32_t th = dropout_threshold(p), lp_th = dropout_threshold(lp_dropout_p);
  const float scale = 1.0f / (1.0f - p), lp_scale = 1.0f / (1.0f - lp_dropout_p);
  const dim3 grid = drop_path_grid(B, n, D);
  hipStream_t st = as_stream(stream);
  if (lp_dtype == FAVIT_F32)
    hipLaunchKernelGGL((drop_path_bwd_kernel<float>), grid, dim3(256), 0, st, g, (float*)g_lp, B, n, D, th, scale, seed,
                       lp_th, lp_scale, lp_dropout_seed, favit_dropout_epoch_ptr_());
  else
    hipLaunchKernelGGL((drop_path_bwd_kernel<bf16_t>), grid, dim3(256), 0, st, g, (bf16_t*)g_lp, B, n, D, th, scale, seed,
                       lp_th, lp_scale, lp_dropout_seed, favit_dropout_epoch_ptr_());
  FAVIT_CHECK_LAUNCH();
  return FAVIT_OK;
}
