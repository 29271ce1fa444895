// Knowledge distillation: the cross-entropy of the (mixed, smoothed) labels and the distance to a frozen teacher's
// logits in one launch (favit.h: favit_cross_entropy_distill).
#include "common.h"

#include <cmath>
#ifdef FAVIT_PROBE
#include <cstdlib>
#endif

extern "C" unsigned* favit_health_ptr_(void);

// One wave per row, lane l owns the classes l, l + 64, ...  NREG == 0 walks the two rows in memory on every pass;
// NREG > 0 (C <= 64 * NREG) loads both rows once into NREG registers per lane each and walks those.
template <int NREG>
struct DistillRow {
  const float* __restrict__ p;
  float r[NREG > 0 ? NREG : 1];
  __device__ __forceinline__ void load(const float* row, int lane, int C) {
    p = row;
    if constexpr (NREG > 0) {
#pragma unroll
      for (int i = 0; i < NREG; ++i) {
        const int c = lane + 64 * i;
        r[i] = c < C ? row[c] : 0.f;
      }
    }
  }
};
// f(c, x_c, z_c) for every class of the lane, ascending in c
template <int NREG, class F>
__device__ __forceinline__ void distill_each(const DistillRow<NREG>& x, const DistillRow<NREG>& z, int lane, int C, F f) {
  if constexpr (NREG > 0) {
#pragma unroll
    for (int i = 0; i < NREG; ++i) {
      const int c = lane + 64 * i;
      if (c < C) f(c, x.r[i], z.r[i]);
    }
  } else {
    for (int c = lane; c < C; c += 64) f(c, x.p[c], z.p[c]);
  }
}

// base: cross_entropy_mix_kernel's row (lam_rows == NULL: lam = 1 and the partner is the row itself, which is
// cross_entropy_kernel's row); eps = 0 makes the smoothing terms vanish exactly.
// kd, soft: tau^2 * sum_c q_c (log q_c - log p_c), q = softmax(z / tau), p = softmax(x / tau), through the two
// log-softmaxes: an underflowed q_c multiplies a finite difference and contributes 0.
// kd, hard: lse(x) - x[argmax z], the lowest index on ties.
template <bool HARD, int NREG>
__global__ __launch_bounds__(256) void cross_entropy_distill_kernel(
    const float* __restrict__ logits, const float* __restrict__ teacher, const int64_t* __restrict__ labels,
    const float* __restrict__ lam_rows, float* __restrict__ loss_rows, float* __restrict__ kd_rows,
    float* __restrict__ dlogits, int B, int C, float grad_scale, float ls_eps, float alpha, float tau,
    unsigned* __restrict__ health) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int row = blockIdx.x * 4 + wave;
  if (row >= B) return;
  DistillRow<NREG> x, z;
  x.load(logits + (long)row * C, lane, C);
  z.load(teacher + (long)row * C, lane, C);

  // pass 1: the two maxima, the row sum of x (smoothing), whether z is finite, and the teacher's class
  float mx = -INFINITY, mz = -INFINITY, xs = 0.f;
  bool zfin = true;
  int zi = 0x7fffffff;                 // (the lane's first class that holds its maximum; ascending c and a strict >)
  distill_each<NREG>(x, z, lane, C, [&](int c, float xv, float zv) {
    mx = fmaxf(mx, xv);
    xs += xv;
    zfin = zfin && isfinite(zv);
    if (zv > mz) { mz = zv; zi = c; }
  });
  if constexpr (HARD) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
      const float ov = __shfl_xor(mz, o, 64);
      const int oi = __shfl_xor(zi, o, 64);
      if (ov > mz || (ov == mz && oi < zi)) { mz = ov; zi = oi; }
    }
    if (zi >= C) zi = 0;               // (no finite entry or NaN only: the row is NaN below, the index stays in range)
  } else {
    mz = wave_max(mz);
  }
  mx = wave_max(mx);
  zfin = __all(zfin);
  const float xmean = wave_sum(xs) / (float)C;

  // pass 2: the sums at temperature 1 (x) and, soft, at tau (x and z)
  const float it = 1.0f / tau;
  float s1 = 0.f, sxt = 0.f, szt = 0.f;
  distill_each<NREG>(x, z, lane, C, [&](int, float xv, float zv) {
    s1 += __expf(xv - mx);
    if constexpr (!HARD) {
      sxt += __expf((xv - mx) * it);
      szt += __expf((zv - mz) * it);
    }
  });
  s1 = wave_sum(s1);
  const float lse = mx + __logf(s1);
  float lxt = 0.f, lzt = 0.f, kd;
  if constexpr (HARD) {
    kd = lse - x.p[zi];
  } else {
    sxt = wave_sum(sxt);
    szt = wave_sum(szt);
    lxt = __logf(sxt);
    lzt = __logf(szt);
    // pass 3: the divergence
    float k = 0.f;
    distill_each<NREG>(x, z, lane, C, [&](int, float xv, float zv) {
      const float lq = (zv - mz) * it - lzt, lp = (xv - mx) * it - lxt;
      k += __expf(lq) * (lq - lp);
    });
    kd = tau * tau * wave_sum(k);
  }
  if (!zfin) kd = __builtin_nanf("");  // a non-finite teacher row: NaN loss row, whatever the kind

  const bool mixed = lam_rows != nullptr;
  const float lam = mixed ? lam_rows[row] : 1.0f, w = 1.0f - lam;
  const int64_t own64 = labels[row], par64 = mixed ? labels[B - 1 - row] : own64;
  const bool own_ok = own64 >= 0 && own64 < C, par_ok = par64 >= 0 && par64 < C;
  const bool lab_ok = own_ok && par_ok;              // either out of range: NaN row, never an OOB read
  const int own = own_ok ? (int)own64 : -1, par = par_ok ? (int)par64 : -1;
  if (lane == 0) {
    float lrow = __builtin_nanf("");
    if (lab_ok) {
      const float zt = fmaf(lam, x.p[own], w * x.p[par]);
      const float base = lse - (1.0f - ls_eps) * zt - ls_eps * xmean;
      lrow = (1.0f - alpha) * base + alpha * kd;
    }
    loss_rows[row] = lrow;
    if (kd_rows) kd_rows[row] = kd;
    if (health && lab_ok && !isfinite(lrow) && !(atomicOr(health, 1u) & 1u)) health[1] = health[3] + 1;
  }
  if (dlogits) {
    const float inv1 = 1.0f / s1, invx = 1.0f / sxt, invz = 1.0f / szt;
    const float hot = 1.0f - ls_eps, uni = ls_eps / (float)C;
    const float hot_own = hot * lam, hot_par = hot * w, wb = 1.0f - alpha;
    float* dr = dlogits + (long)row * C;
    distill_each<NREG>(x, z, lane, C, [&](int c, float xv, float zv) {
      const float sm = __expf(xv - mx) * inv1;
      const float t = (c == own ? hot_own : 0.f) + (c == par ? hot_par : 0.f);
      float d;
      if constexpr (HARD) d = sm - (c == zi ? 1.f : 0.f);
      else d = tau * (__expf((xv - mx) * it) * invx - __expf((zv - mz) * it) * invz);
      dr[c] = (wb * (sm - t - uni) + alpha * d) * grad_scale;
    });
  }
}

extern "C" int favit_cross_entropy_mix(const float*, const int64_t*, const float*, float*, float*, int32_t, int32_t,
                                       float, float, void*);
extern "C" int favit_cross_entropy_ls(const float*, const int64_t*, float*, float*, int32_t, int32_t, float, float,
                                      void*);

// Rows of more than two and at most sixteen strides of the wave are held in registers (16 values per lane and row);
// shorter rows cost less walked in memory, where the loops run once or twice instead of sixteen predicated times
// (DESIGN.md section 15 has the measurements behind both bounds).
static constexpr int DISTILL_REG_MIN_C = 129, DISTILL_REG_MAX_C = 1024;

extern "C" int favit_cross_entropy_distill(const float* logits, const float* teacher, const int64_t* labels,
                                           const float* lam, float* loss_rows, float* kd_rows, float* dlogits,
                                           int32_t B, int32_t C, float grad_scale, float label_smoothing, float alpha,
                                           float tau, int32_t hard, void* stream) {
  if (!(alpha >= 0.f && alpha <= 1.f)) return FAVIT_ERR_INVALID;
  if (!(label_smoothing >= 0.f && label_smoothing < 1.f)) return FAVIT_ERR_INVALID;
  if (!hard && !(std::isfinite(tau) && tau > 0.f)) return FAVIT_ERR_INVALID;
  if (!logits || !teacher || !labels || !loss_rows || B <= 0 || C <= 0) return FAVIT_ERR_INVALID;
  if (alpha == 0.f) {
    // the loss of before, by the entry point of before (its bits); the teacher is not read and kd_rows not written
    if (lam) return favit_cross_entropy_mix(logits, labels, lam, loss_rows, dlogits, B, C, grad_scale, label_smoothing, stream);
    return favit_cross_entropy_ls(logits, labels, loss_rows, dlogits, B, C, grad_scale, label_smoothing, stream);
  }
  bool in_regs = C >= DISTILL_REG_MIN_C && C <= DISTILL_REG_MAX_C;
#ifdef FAVIT_PROBE
  if (const char* e = std::getenv("FAVIT_DISTILL_DBG")) in_regs = e[0] == 's' ? false : (e[0] == 'r' ? C <= DISTILL_REG_MAX_C : in_regs);   // "stream": rows stay in memory; "regs": C <= 1024 in registers
#endif
  const dim3 grid((B + 3) / 4), block(256);
  const float t = hard ? 1.0f : tau;
#define FAVIT_DISTILL_LAUNCH(HARD, NREG)                                                                              \
  hipLaunchKernelGGL((cross_entropy_distill_kernel<HARD, NREG>), grid, block, 0, as_stream(stream), logits, teacher, \
                     labels, lam, loss_rows, kd_rows, dlogits, B, C, grad_scale, label_smoothing, alpha, t,           \
                     favit_health_ptr_())
  if (hard) {
    if (in_regs) FAVIT_DISTILL_LAUNCH(true, 16);
    else FAVIT_DISTILL_LAUNCH(true, 0);
  } else {
    if (in_regs) FAVIT_DISTILL_LAUNCH(false, 16);
    else FAVIT_DISTILL_LAUNCH(false, 0);
  }
#undef FAVIT_DISTILL_LAUNCH
  FAVIT_CHECK_LAUNCH();
  return FAVIT_OK;
}
