// Device RandAugment and Random Erasing (additive in ABI 8): torchvision's RandAugment ops on PIL images, restated in
// the arithmetic Pillow runs in C so that the augmented bytes are BIT-IDENTICAL to Pillow's, applied to the resized
// bytes the image transform writes, then ToTensor + Normalize (the expression of resample_v_kernel, image.hip) and the
// erase box of the image in the same write.
//
// One workgroup per image chains every op of the image inside ONE launch, with a barrier between ops.  The geometric
// ops and the 3x3 filter are not in place, so the ops ping-pong between two caller-provided uint8 planes [2,B,S,S,C]
// (150,528 B per image at S = 224: a batch's planes stay in L2); the source bytes are only read.  The planes are
// written and re-read by other threads of the workgroup within the launch, so no pointer to them is const __restrict__
// (nothing may move those loads to the scalar cache or above a barrier).
//
// What Pillow computes in Python doubles (affine matrices and their 16.16 fixed-point form, Posterize masks, Solarize
// thresholds, enhancement factors) arrives in the op table, computed by the host; the device does what Pillow does in
// C: integers and fp32.  fp32 blends and filter taps are never fused (mul_rn / add_rn below): Pillow truncates
// in1 + alpha * (in2 - in1), and a fused rounding can move a value across an integer.  AutoContrast's LUT needs the image's min / max and is the one double-precision computation here (again
// unfused).
//
// Op table: int32 [B, n_ops, 8] rows (op, p0 .. p6):
//   0 identity
//   1 affine NEAREST   p0..p5 = a0, a1, a2', a3, a4, a5' in 16.16 fixed point, p6 = fill r | g << 8 | b << 16
//   2 blend            p0 = degenerate (0 black, 1 luma, 2 mean luma, 3 SMOOTH filter), p1 = bits of the fp32 factor
//   3 and-mask         p0 = mask                                   (Posterize)
//   4 solarize         p0 = threshold t: v -> v < t ? v : 255 - v
//   5 autocontrast     6 equalize
// An unknown op id is treated as identity (the host refuses it before the upload); no table content can cause an
// out-of-range access: every gathered source coordinate is checked against the image.
#include "common.h"

// No fused multiply-add anywhere below: Pillow's C is compiled without it, and hipcc contracts a * b + c by default.
// HIP's __fmul_rn / __fadd_rn do NOT prevent that: they are plain operators defined in a header, outside this pragma,
// and __fadd_rn(d, __fmul_rn(f, s - d)) compiles to one v_fmac_f32.  With it a Contrast blend at factor 1.45 came out
// one level low in 32 of 3072 bytes (by the arithmetic: where 1.45 (s - d) is an integer, fp32(1.45) (s - d) is a
// rounding tie).
#pragma clang fp contract(off)

namespace {

// products and sums that must round on their own, defined HERE, under the pragma
__device__ __forceinline__ float mul_rn(float a, float b) { return a * b; }
__device__ __forceinline__ float add_rn(float a, float b) { return a + b; }
__device__ __forceinline__ double mul_rn(double a, double b) { return a * b; }
__device__ __forceinline__ double add_rn(double a, double b) { return a + b; }

constexpr int AUG_THREADS = 1024;
constexpr int AUG_MAX_OPS = FAVIT_RANDAUGMENT_MAX_OPS;

struct EraseFill {
  float v[3];          // per-channel constant
  int normal;          // 1: one standard-normal value per element instead
  uint64_t seed;
};

// Standard-normal value of element idx = ((b*C + c)*H + y)*W + x: Box-Muller on two draws of the library's
// counter-based generator (2 idx -> u1 in (0, 1], 2 idx + 1 -> u2 in [0, 1), both multiples of 2^-24).  A function of
// (seed, idx) alone, so it does not depend on the launch geometry.
__device__ __forceinline__ float normal_value(uint64_t seed, uint64_t idx) {
  const uint32_t r1 = favit_rand_u32(seed, 2 * idx), r2 = favit_rand_u32(seed, 2 * idx + 1);
  const float u1 = (float)((r1 >> 8) + 1u) * 0x1p-24f, u2 = (float)(r2 >> 8) * 0x1p-24f;
  const float r = sqrtf(mul_rn(-2.0f, logf(u1)));
  return mul_rn(r, cosf(mul_rn(6.283185307179586f, u2)));
}

__device__ __forceinline__ int luma(const uint8_t* p) {
  return (19595 * (int)p[0] + 38470 * (int)p[1] + 7471 * (int)p[2] + 0x8000) >> 16;
}

// ImagingBlend(deg, src, f): deg + f * (src - deg) in fp32, truncated; clipped first unless 0 <= f <= 1
__device__ __forceinline__ uint8_t blend8(int deg, int src, float f, bool inside) {
  const float v = add_rn((float)deg, mul_rn(f, (float)(src - deg)));
  if (inside) return (uint8_t)(int)v;
  return v <= 0.0f ? (uint8_t)0 : (v >= 255.0f ? (uint8_t)255 : (uint8_t)(int)v);
}

// one row of the 3x3 SMOOTH filter: the three taps left to right
__device__ __forceinline__ float smooth_row(const uint8_t* p, int C, float kc, float k1) {
  return add_rn(add_rn(mul_rn((float)p[-C], k1), mul_rn((float)p[0], kc)), mul_rn((float)p[C], k1));
}

// src [B,S,S,C] (C == 3), planes [2,B,S,S,C]; one workgroup per image
__global__ __launch_bounds__(AUG_THREADS) void randaugment_kernel(const uint8_t* src, uint8_t* planes, float* __restrict__ out,
                                                                  uint8_t* __restrict__ out_u8,
                                                                  const int32_t* __restrict__ ops, int n_ops,
                                                                  const int32_t* __restrict__ erase, EraseFill fill,
                                                                  int B, int S, float3 mean, float3 stdv) {
  constexpr int C = 3;
  __shared__ int hist[C][256];
  __shared__ uint8_t lut[C][256];
  __shared__ int red[4];                 // luma sum; lo / hi scratch
  const int b = blockIdx.x, tid = threadIdx.x;
  const int npix = S * S;
  const long n = (long)npix * C;
  const uint8_t* cur = src + (long)b * n;
  int plane = 0;

  for (int slot = 0; slot < n_ops; ++slot) {
    const int32_t* row = ops + ((long)b * n_ops + slot) * 8;
    const int op = row[0];
    if (op < FAVIT_AUG_AFFINE || op > FAVIT_AUG_EQUALIZE) continue;            // identity: nothing moves
    uint8_t* dst = planes + ((long)plane * B + b) * n;

    if (op == FAVIT_AUG_AFFINE) {
      const int a0 = row[1], a1 = row[2], a2 = row[3], a3 = row[4], a4 = row[5], a5 = row[6];
      const uint8_t f0 = (uint8_t)(row[7] & 255), f1 = (uint8_t)((row[7] >> 8) & 255), f2 = (uint8_t)((row[7] >> 16) & 255);
      for (int i = tid; i < npix; i += AUG_THREADS) {
        const int y = i / S, x = i - y * S;
        // Pillow accumulates these in 32-bit ints (far below 2^31 for the rows the host builds; unsigned here so that
        // no table content is undefined behaviour), then shifts arithmetically
        const int sx = (int)((unsigned)a2 + (unsigned)a1 * (unsigned)y + (unsigned)a0 * (unsigned)x) >> 16;
        const int sy = (int)((unsigned)a5 + (unsigned)a4 * (unsigned)y + (unsigned)a3 * (unsigned)x) >> 16;
        uint8_t* o = dst + (long)i * C;
        if (sx >= 0 && sx < S && sy >= 0 && sy < S) {
          const uint8_t* q = cur + ((long)sy * S + sx) * C;
          o[0] = q[0]; o[1] = q[1]; o[2] = q[2];
        } else {
          o[0] = f0; o[1] = f1; o[2] = f2;
        }
      }
    } else if (op == FAVIT_AUG_BLEND) {
      const int kind = row[1];
      const float f = __int_as_float(row[2]);
      const bool inside = f >= 0.0f && f <= 1.0f;
      if (kind == 3) {                                             // Sharpness: degenerate = SMOOTH, border copied
        const float k1 = 1.0f / 13.0f, k5 = 5.0f / 13.0f;
        for (long i = tid; i < n; i += AUG_THREADS) {
          const int pix = (int)(i / C);
          const int y = pix / S, x = pix - y * S;
          const uint8_t* p = cur + i;
          int deg = p[0];
          if (y > 0 && y < S - 1 && x > 0 && x < S - 1) {
            float ss = 0.5f;
            ss = add_rn(ss, smooth_row(p + (long)S * C, C, k1, k1));
            ss = add_rn(ss, smooth_row(p, C, k5, k1));
            ss = add_rn(ss, smooth_row(p - (long)S * C, C, k1, k1));
            deg = ss <= 0.0f ? 0 : (ss >= 255.0f ? 255 : (int)ss);
          }
          dst[i] = blend8(deg, p[0], f, inside);
        }
      } else {
        int mean_l = 0;
        if (kind == 2) {                                           // Contrast: int(mean(L) + 0.5), exact integer sum
          if (tid == 0) red[0] = 0;
          __syncthreads();
          int part = 0;
          for (int i = tid; i < npix; i += AUG_THREADS) part += luma(cur + (long)i * C);
          atomicAdd(&red[0], part);
          __syncthreads();
          // floor(sum / npix + 1/2) in integers: the quotient is a multiple of 1 / npix, so the double-precision
          // int(mean + 0.5) of Pillow's Python side cannot round across an integer and equals this
          mean_l = (int)((2L * red[0] + npix) / (2L * npix));
        }
        for (int i = tid; i < npix; i += AUG_THREADS) {
          const uint8_t* p = cur + (long)i * C;
          uint8_t* o = dst + (long)i * C;
          const int deg = kind == 1 ? luma(p) : (kind == 2 ? mean_l : 0);
          o[0] = blend8(deg, p[0], f, inside);
          o[1] = blend8(deg, p[1], f, inside);
          o[2] = blend8(deg, p[2], f, inside);
        }
      }
    } else {                                                       // the LUT ops
      if (op == FAVIT_AUG_MASK || op == FAVIT_AUG_SOLARIZE) {
        const int a = row[1];
        for (int i = tid; i < C * 256; i += AUG_THREADS) {
          const int v = i & 255;
          lut[i >> 8][v] = (uint8_t)(op == FAVIT_AUG_MASK ? (v & a) : (v < a ? v : 255 - v));
        }
      } else {
        for (int i = tid; i < C * 256; i += AUG_THREADS) hist[i >> 8][i & 255] = 0;
        __syncthreads();
        for (long i = tid; i < n; i += AUG_THREADS) atomicAdd(&hist[(int)(i % C)][cur[i]], 1);
        __syncthreads();
        if (op == FAVIT_AUG_EQUALIZE) {
          // ImageOps.equalize: step = (n - h[last nonzero]) / 255; lut[i] = (step / 2 + sum_{j<i} h[j]) / step, clipped
          if (tid < C) {
            const int c = tid;
            int last = -1, levels = 0;
            for (int v = 0; v < 256; ++v)
              if (hist[c][v]) { last = v; ++levels; }
            const int step = levels > 1 ? (npix - hist[c][last]) / 255 : 0;
            int acc = step / 2;
            for (int v = 0; v < 256; ++v) {
              int q = v;
              if (step > 0) {
                q = acc / step;
                q = q > 255 ? 255 : q;
              }
              acc += hist[c][v];
              lut[c][v] = (uint8_t)q;
            }
          }
        } else {
          // ImageOps.autocontrast: lut[i] = clip(int(i * scale + (-lo * scale))), scale = 255.0 / (hi - lo), in double
          if (tid < C) {
            int lo = 0, hi = 255;
            while (lo < 256 && !hist[tid][lo]) ++lo;
            while (hi >= 0 && !hist[tid][hi]) --hi;
            red[1 + tid] = lo | (hi << 16);
          }
          __syncthreads();
          for (int i = tid; i < C * 256; i += AUG_THREADS) {
            const int c = i >> 8, v = i & 255;
            const int lo = red[1 + c] & 0xffff, hi = red[1 + c] >> 16;
            int q = v;
            if (hi > lo) {
              const double scale = 255.0 / (double)(hi - lo);
              const double offset = mul_rn(-(double)lo, scale);
              const double t = add_rn(mul_rn((double)v, scale), offset);
              q = (int)t;                                          // truncation towards zero, as Python's int()
              q = q < 0 ? 0 : (q > 255 ? 255 : q);
            }
            lut[c][v] = (uint8_t)q;
          }
        }
      }
      __syncthreads();
      for (long i = tid; i < n; i += AUG_THREADS) dst[i] = lut[(int)(i % C)][cur[i]];
    }
    __syncthreads();            // the plane is complete (and LDS is free) before the next op reads it
    cur = dst;
    plane ^= 1;
  }

  // ToTensor + Normalize with the expression of resample_v_kernel, the erase box in the same write
  const int* eb = erase ? erase + 4 * (long)b : nullptr;
  const int ey0 = eb ? eb[0] : 0, ey1 = eb ? eb[1] : 0, ex0 = eb ? eb[2] : 0, ex1 = eb ? eb[3] : 0;
  const float m[3] = {mean.x, mean.y, mean.z}, sd[3] = {stdv.x, stdv.y, stdv.z};
  if (out_u8)
    for (long i = tid; i < n; i += AUG_THREADS) out_u8[(long)b * n + i] = cur[i];
  for (long i = tid; i < n; i += AUG_THREADS) {                    // i = (c*S + y)*S + x: coalesced fp32 stores
    const int c = (int)(i / npix);
    const int pix = (int)(i - (long)c * npix);
    const int y = pix / S, x = pix - y * S;
    float r;
    if (y >= ey0 && y < ey1 && x >= ex0 && x < ex1) {
      r = fill.normal ? normal_value(fill.seed, (uint64_t)b * (uint64_t)n + (uint64_t)i) : fill.v[c];
    } else {
      const float tv = (float)cur[(long)pix * C + c] / 255.0f;
      r = (tv - m[c]) / sd[c];
    }
    out[(long)b * n + i] = r;
  }
}

// x [B,C,H,W] fp32 in place.  blockIdx.y = image; the work items of an image are the (channel, box line, 16-byte
// group) triples its box meets (VEC == 1: single elements): nothing outside them is loaded or stored.
template <int VEC>
__global__ __launch_bounds__(256) void random_erase_kernel(float* __restrict__ x, const int32_t* __restrict__ box,
                                                           EraseFill fill, int C, int H, int W) {
  const int b = blockIdx.y;
  int y0 = box[4 * (long)b + 0], y1 = box[4 * (long)b + 1], x0 = box[4 * (long)b + 2], x1 = box[4 * (long)b + 3];
  y0 = y0 < 0 ? 0 : y0; x0 = x0 < 0 ? 0 : x0;                      // whatever the table holds, stay inside the image
  y1 = y1 > H ? H : y1; x1 = x1 > W ? W : x1;
  if (y0 >= y1 || x0 >= x1) return;
  const int g0 = x0 / VEC, ng = (x1 + VEC - 1) / VEC - g0, nh = y1 - y0;
  const long items = (long)C * nh * ng;
  const long chw = (long)C * H * W;
  for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < items; i += (long)gridDim.x * 256) {
    const int g = (int)(i % ng);
    const long t = i / ng;
    const int y = y0 + (int)(t % nh), c = (int)(t / nh);
    const int xs = (g0 + g) * VEC;
    const long e = ((long)c * H + y) * W + xs;                     // element index inside the image
    float v[VEC];
#pragma unroll
    for (int k = 0; k < VEC; ++k)
      v[k] = fill.normal ? normal_value(fill.seed, (uint64_t)b * (uint64_t)chw + (uint64_t)(e + k)) : fill.v[c < 3 ? c : 2];
    float* p = x + (long)b * chw + e;
    if constexpr (VEC == 4) {
      if (xs >= x0 && xs + 4 <= x1) {
        *reinterpret_cast<float4*>(p) = make_float4(v[0], v[1], v[2], v[3]);
        continue;
      }
    }
#pragma unroll
    for (int k = 0; k < VEC; ++k)
      if (xs + k >= x0 && xs + k < x1) p[k] = v[k];
  }
}

int make_fill(EraseFill& f, const float* value, int32_t normal, uint64_t seed, int C) {
  if (!normal && !value) return FAVIT_ERR_INVALID;
  for (int c = 0; c < 3; ++c) f.v[c] = (!normal && value) ? value[c < C ? c : C - 1] : 0.0f;
  f.normal = normal ? 1 : 0;
  f.seed = seed;
  return FAVIT_OK;
}

}  // namespace

extern "C" int favit_randaugment_max_ops(void) { return AUG_MAX_OPS; }

extern "C" int favit_randaugment(const uint8_t* src_u8, uint8_t* scratch, float* out, uint8_t* out_u8,
                                 const int32_t* ops, int32_t n_ops, const int32_t* erase_box,
                                 const float* erase_value, int32_t erase_normal, uint64_t erase_seed, int32_t B,
                                 int32_t S, int32_t C, const float* mean, const float* std, void* stream) {
  if (!src_u8 || !scratch || !out || !ops || !mean || !std || B <= 0 || S <= 0 || n_ops < 0) return FAVIT_ERR_INVALID;
  if (n_ops > AUG_MAX_OPS) return FAVIT_ERR_INVALID;
  if (C != 3 || S > 2048) return FAVIT_ERR_UNSUPPORTED;            // RGB; S bounds the luma sum and the fixed point
  EraseFill f = {{0.0f, 0.0f, 0.0f}, 0, 0};
  if (erase_box) {
    const int rc = make_fill(f, erase_value, erase_normal, erase_seed, C);
    if (rc != FAVIT_OK) return rc;
  }
  const float3 m = make_float3(mean[0], mean[1], mean[2]), sd = make_float3(std[0], std[1], std[2]);
  hipLaunchKernelGGL(randaugment_kernel, dim3((unsigned)B), dim3(AUG_THREADS), 0, as_stream(stream), src_u8, scratch, out,
                     out_u8, ops, (int)n_ops, erase_box, f, (int)B, (int)S, m, sd);
  FAVIT_CHECK_LAUNCH();
  return FAVIT_OK;
}

extern "C" int favit_random_erase(float* x, const int32_t* box, const float* value, int32_t normal, uint64_t seed,
                                  int32_t B, int32_t C, int32_t H, int32_t W, void* stream) {
  if (!x || !box || B <= 0 || C <= 0 || H <= 0 || W <= 0) return FAVIT_ERR_INVALID;
  if ((long)C * H * W > 0x7fffffffL || B > 65535) return FAVIT_ERR_UNSUPPORTED;
  EraseFill f;
  const int rc = make_fill(f, value, normal, seed, C);
  if (rc != FAVIT_OK) return rc;
  const bool v4 = (W & 3) == 0 && (reinterpret_cast<uintptr_t>(x) & 15) == 0;
  // the largest box has C * H * (W / VEC) items; 8 workgroups per image cover S = 224 in a few strides
  const long items = (long)C * H * (v4 ? W / 4 : W);
  long gx = (items + 255) / 256;
  if (gx > 8) gx = 8;
  const dim3 grid((unsigned)gx, (unsigned)B);
  if (v4)
    hipLaunchKernelGGL(random_erase_kernel<4>, grid, dim3(256), 0, as_stream(stream), x, box, f, (int)C, (int)H, (int)W);
  else
    hipLaunchKernelGGL(random_erase_kernel<1>, grid, dim3(256), 0, as_stream(stream), x, box, f, (int)C, (int)H, (int)W);
  FAVIT_CHECK_LAUNCH();
  return FAVIT_OK;
}
