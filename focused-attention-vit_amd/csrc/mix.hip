// Batch mixing (Mixup / CutMix of a batch with its own flip) and the cross-entropy of the mixed targets.
#include "common.h"

extern "C" unsigned* favit_health_ptr_(void);

// One row's parameters as the image side sees them.  mode: 0 = unchanged, 1 = Mixup (blend), 2 = CutMix (paste box).
struct MixRow {
  float lam, w;
  int y0, y1, x0, x1, mode;
};
__device__ __forceinline__ MixRow mix_row(const float* __restrict__ lam, const int32_t* __restrict__ box, int r) {
  MixRow m;
  m.lam = lam[r];
  m.w = 1.0f - m.lam;
  m.y0 = box[4 * (long)r + 0];
  m.y1 = box[4 * (long)r + 1];
  m.x0 = box[4 * (long)r + 2];
  m.x1 = box[4 * (long)r + 3];
  m.mode = (m.y0 < m.y1 && m.x0 < m.x1) ? 2 : (m.lam == 1.0f ? 0 : 1);
  return m;
}
// does the row change anything in the VEC pixels of line y that start at column xs?
template <int VEC>
__device__ __forceinline__ bool mix_needs(const MixRow& m, int y, int xs) {
  if (m.mode == 2) return y >= m.y0 && y < m.y1 && xs < m.x1 && xs + VEC > m.x0;
  return m.mode == 1;
}
// new value of the row's pixel (y, x): a = its own old value, q = the partner's
__device__ __forceinline__ float mix_apply(const MixRow& m, float a, float q, bool in_y, int x) {
  if (m.mode == 2) return (in_y && x >= m.x0 && x < m.x1) ? q : a;
  return fmaf(m.lam, a, m.w * q);
}

// x: [B, C, H, W] fp32, in place.  blockIdx.y walks the pairs (b, B-1-b), blockIdx.x grid-strides over the n_items =
// C * H * (W / VEC) groups of one image; a thread owns the same group of both rows, so every old value is read before
// either row is written.  The box only decides between xb[i] and xp[i], both in range whatever lam / box hold.
template <int VEC>
__global__ __launch_bounds__(256) void batch_mix_kernel(float* __restrict__ x, const float* __restrict__ lam,
                                                        const int32_t* __restrict__ box, int B, int H, int Wg,
                                                        long n_items) {
  const long chw = n_items * VEC;
  for (int pair = blockIdx.y; pair < B / 2; pair += gridDim.y) {
    const MixRow mb = mix_row(lam, box, pair), mp = mix_row(lam, box, B - 1 - pair);
    if (mb.mode == 0 && mp.mode == 0) continue;          // nothing to do: no pixel is loaded
    float* xb = x + (long)pair * chw;
    float* xp = x + (long)(B - 1 - pair) * chw;
    for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < n_items; i += (long)gridDim.x * 256) {
      const unsigned u = (unsigned)i;                    // (n_items < 2^31: checked by the host)
      const int xs = (int)(u % (unsigned)Wg) * VEC, y = (int)((u / (unsigned)Wg) % (unsigned)H);
      const bool nb = mix_needs<VEC>(mb, y, xs), np = mix_needs<VEC>(mp, y, xs);
      if (!nb && !np) continue;                          // outside both boxes: no load, no store
      const bool yb = y >= mb.y0 && y < mb.y1, yp = y >= mp.y0 && y < mp.y1;
      if constexpr (VEC == 4) {
        const float4 a = *reinterpret_cast<const float4*>(xb + i * 4);
        const float4 q = *reinterpret_cast<const float4*>(xp + i * 4);
        if (nb) {
          float4 r;
          r.x = mix_apply(mb, a.x, q.x, yb, xs);
          r.y = mix_apply(mb, a.y, q.y, yb, xs + 1);
          r.z = mix_apply(mb, a.z, q.z, yb, xs + 2);
          r.w = mix_apply(mb, a.w, q.w, yb, xs + 3);
          *reinterpret_cast<float4*>(xb + i * 4) = r;
        }
        if (np) {
          float4 r;
          r.x = mix_apply(mp, q.x, a.x, yp, xs);
          r.y = mix_apply(mp, q.y, a.y, yp, xs + 1);
          r.z = mix_apply(mp, q.z, a.z, yp, xs + 2);
          r.w = mix_apply(mp, q.w, a.w, yp, xs + 3);
          *reinterpret_cast<float4*>(xp + i * 4) = r;
        }
      } else {
        const float a = xb[i], q = xp[i];
        if (nb) xb[i] = mix_apply(mb, a, q, yb, xs);
        if (np) xp[i] = mix_apply(mp, q, a, yp, xs);
      }
    }
  }
}

extern "C" int favit_batch_mix(float* x, const float* lam, const int32_t* box, int32_t B, int32_t C, int32_t H,
                               int32_t W, void* stream) {
  if (!x || !lam || !box || B <= 0 || C <= 0 || H <= 0 || W <= 0) return FAVIT_ERR_INVALID;
  const long chw = (long)C * H * W;
  if (chw > 0x7fffffffL) return FAVIT_ERR_UNSUPPORTED;
  if (B == 1) return FAVIT_OK;
  const bool v4 = (W & 3) == 0 && (reinterpret_cast<uintptr_t>(x) & 15) == 0;
  const int Wg = v4 ? W / 4 : W;
  const long n_items = (long)C * H * Wg;
  // a streaming kernel: about 2048 workgroups in all, the rest by grid stride
  const int pairs = B / 2;
  const unsigned gy = (unsigned)(pairs < 2048 ? pairs : 2048);
  long gx = (n_items + 255) / 256;
  const long cap = 2048 / gy;
  if (gx > cap) gx = cap;
  if (gx < 1) gx = 1;
  const dim3 grid((unsigned)gx, gy);
  if (v4)
    hipLaunchKernelGGL(batch_mix_kernel<4>, grid, dim3(256), 0, as_stream(stream), x, lam, box, B, H, Wg, n_items);
  else
    hipLaunchKernelGGL(batch_mix_kernel<1>, grid, dim3(256), 0, as_stream(stream), x, lam, box, B, H, Wg, n_items);
  FAVIT_CHECK_LAUNCH();
  return FAVIT_OK;
}

// cross_entropy_kernel (norm_elem.hip) against the two-class target lam * onehot(y_b) + (1 - lam) * onehot(y_p), y_p the
// label of row B-1-row: one wave per row, the same reductions in the same order.  The target logit and the indicator
// enter as lam * a + (1 - lam) * b, which is a (resp. 1 or 0) exactly when lam == 1, and every expression they feed has
// the shape of its counterpart there: lam == 1 gives that kernel's bits.
template <bool LS>
__global__ __launch_bounds__(256) void cross_entropy_mix_kernel(const float* __restrict__ logits,
                                                                const int64_t* __restrict__ labels,
                                                                const float* __restrict__ lam_rows,
                                                                float* __restrict__ loss_rows,
                                                                float* __restrict__ dlogits, int B, int C,
                                                                float grad_scale, float ls_eps,
                                                                unsigned* __restrict__ health) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int row = blockIdx.x * 4 + wave;
  if (row >= B) return;
  const float* lr = logits + (long)row * C;
  float m = -INFINITY;
  for (int c = lane; c < C; c += 64) m = fmaxf(m, lr[c]);
  m = wave_max(m);
  float s = 0.f;
  for (int c = lane; c < C; c += 64) s += __expf(lr[c] - m);
  s = wave_sum(s);
  const float lse = m + __logf(s);
  float xmean = 0.f;
  if constexpr (LS) {
    float t = 0.f;
    for (int c = lane; c < C; c += 64) t += lr[c];
    xmean = wave_sum(t) / (float)C;
  }
  const float lam = lam_rows[row], w = 1.0f - lam;
  const int64_t own64 = labels[row], par64 = labels[B - 1 - row];
  const bool own_ok = own64 >= 0 && own64 < C, par_ok = par64 >= 0 && par64 < C;
  const bool lab_ok = own_ok && par_ok;              // either out of range: NaN row, never an OOB read
  const int own = own_ok ? (int)own64 : -1, par = par_ok ? (int)par64 : -1;
  if (lane == 0) {
    float lrow = __builtin_nanf("");
    if (lab_ok) {
      const float zt = fmaf(lam, lr[own], w * lr[par]);
      if constexpr (LS) lrow = lse - (1.0f - ls_eps) * zt - ls_eps * xmean;
      else lrow = lse - zt;
    }
    loss_rows[row] = lrow;
    if (health && lab_ok && !isfinite(lrow) && !(atomicOr(health, 1u) & 1u)) health[1] = health[3] + 1;
  }
  if (dlogits) {
    const float inv = 1.0f / s;
    if constexpr (LS) {
      // (the two weights are scaled per row, not per class: no product in the loop that could fuse with the
      // subtraction and round differently from cross_entropy_kernel's softmax - hot)
      const float hot = 1.0f - ls_eps, uni = ls_eps / (float)C;
      const float hot_own = hot * lam, hot_par = hot * w;
      for (int c = lane; c < C; c += 64) {
        const float t = (c == own ? hot_own : 0.f) + (c == par ? hot_par : 0.f);
        dlogits[(long)row * C + c] = (__expf(lr[c] - m) * inv - t - uni) * grad_scale;
      }
    } else {
      for (int c = lane; c < C; c += 64) {
        const float t = (c == own ? lam : 0.f) + (c == par ? w : 0.f);
        dlogits[(long)row * C + c] = (__expf(lr[c] - m) * inv - t) * grad_scale;
      }
    }
  }
}

extern "C" int favit_cross_entropy_mix(const float* logits, const int64_t* labels, const float* lam, float* loss_rows,
                                       float* dlogits, int32_t B, int32_t C, float grad_scale, float label_smoothing,
                                       void* stream) {
  if (!(label_smoothing >= 0.f && label_smoothing < 1.f)) return FAVIT_ERR_INVALID;
  if (!logits || !labels || !lam || !loss_rows || B <= 0 || C <= 0) return FAVIT_ERR_INVALID;
  // eps = 0 takes the unsmoothed instantiation, as favit_cross_entropy_ls does
  if (label_smoothing == 0.f)
    hipLaunchKernelGGL(cross_entropy_mix_kernel<false>, dim3((B + 3) / 4), dim3(256), 0, as_stream(stream), logits, labels, lam, loss_rows, dlogits, B, C, grad_scale, 0.0f, favit_health_ptr_());
  else
    hipLaunchKernelGGL(cross_entropy_mix_kernel<true>, dim3((B + 3) / 4), dim3(256), 0, as_stream(stream), logits, labels, lam, loss_rows, dlogits, B, C, grad_scale, label_smoothing, favit_health_ptr_());
  FAVIT_CHECK_LAUNCH();
  return FAVIT_OK;
}
