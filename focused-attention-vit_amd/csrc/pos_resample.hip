// Separable resampling of a square grid of fp32 token rows (a learned pos_embed) to another grid side, and its
// adjoint (favit.h: favit_pos_resample).  ONE entry point serves both directions: the forward
// passes the compressed rows of M [g_out, g_in], the backward the compressed rows of M^T with the two sides swapped.
// A gather: every thread owns four consecutive columns of one output row and walks the taps of its grid row and of
// its grid column in table order, so there are no atomics and the same inputs give the same bits in every run.
#include "common.h"

namespace {

// y[n_prefix + a * g_out + b, :] = sum_i sum_j M[a, i] * M[b, j] * x[n_prefix + i * g_in + j, :], i and j over the
// stored entries of rows a and b.  The accumulator starts at -0.0f, the one value v + acc == v holds for bit by bit
// (a +0.0f start would turn an input of -0.0f into +0.0f), so a one-tap row of weight 1 copies its source row.
__global__ __launch_bounds__(256) void pos_resample_kernel(const float4* __restrict__ x, float4* __restrict__ y,
                                                           const int* __restrict__ rowptr, const int* __restrict__ cols,
                                                           const float* __restrict__ vals, int g_in, int g_out,
                                                           int n_prefix, int D4) {
  const long total = (long)(n_prefix + g_out * g_out) * D4;
  const long idx = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (idx >= total) return;
  const int row = (int)(idx / D4), c = (int)(idx - (long)row * D4);
  if (row < n_prefix) {               // the prefix rows sit at the same offset on both sides
    y[idx] = x[idx];
    return;
  }
  const int p = row - n_prefix, a = p / g_out, b = p - a * g_out;
  const int a0 = rowptr[a], a1 = rowptr[a + 1], b0 = rowptr[b], b1 = rowptr[b + 1];
  const float z = (a1 > a0 && b1 > b0) ? -0.0f : 0.0f;      // (a row of M^T may be empty: an unread source row)
  float4 acc = make_float4(z, z, z, z);
  for (int i = a0; i < a1; ++i) {
    const float wi = vals[i];
    const float4* src = x + ((long)n_prefix + (long)cols[i] * g_in) * D4 + c;
    for (int j = b0; j < b1; ++j) {
      const float w = wi * vals[j];
      const float4 v = src[(long)cols[j] * D4];
      acc.x = fmaf(w, v.x, acc.x);
      acc.y = fmaf(w, v.y, acc.y);
      acc.z = fmaf(w, v.z, acc.z);
      acc.w = fmaf(w, v.w, acc.w);
    }
  }
  y[idx] = acc;
}

}  // namespace

extern "C" int favit_pos_resample(const float* x, float* y, const int32_t* rowptr, const int32_t* cols,
                                  const float* vals, int32_t g_in, int32_t g_out, int32_t n_prefix, int32_t D,
                                  void* stream) {
  if (!x || !y || !rowptr || !cols || !vals || x == y) return FAVIT_ERR_INVALID;
  if (g_in < 1 || g_out < 1 || n_prefix < 0 || n_prefix > 1 || D < 4 || D % 4 != 0) return FAVIT_ERR_INVALID;
  if ((long)g_in * g_in + n_prefix > FAVIT_POS_RESAMPLE_MAX_L || (long)g_out * g_out + n_prefix > FAVIT_POS_RESAMPLE_MAX_L)
    return FAVIT_ERR_UNSUPPORTED;
  if ((reinterpret_cast<uintptr_t>(x) | reinterpret_cast<uintptr_t>(y)) & 15) return FAVIT_ERR_ALIGN;
  const int D4 = D / 4;
  const long total = (long)(n_prefix + g_out * g_out) * D4;
  hipLaunchKernelGGL(pos_resample_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, as_stream(stream),
                     reinterpret_cast<const float4*>(x), reinterpret_cast<float4*>(y), (const int*)rowptr,
                     (const int*)cols, vals, (int)g_in, (int)g_out, (int)n_prefix, D4);
  FAVIT_CHECK_LAUNCH();
  return FAVIT_OK;
}
