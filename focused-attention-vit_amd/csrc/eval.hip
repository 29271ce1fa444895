// Evaluation metrics: loss, argmax and the rank of the label per row, folded into a device-resident state of top-k
// hits, per-class counts and a confusion matrix without a host sync (favit.h: favit_eval_metrics; DESIGN.md
// section 16).
#include "common.h"

namespace {

constexpr int EVAL_STATE_WORDS = FAVIT_EVAL_SLOT_HITS + FAVIT_EVAL_MAX_TOPK;
static_assert(EVAL_STATE_WORDS == FAVIT_EVAL_STATE_WORDS, "favit.h: FAVIT_EVAL_STATE_WORDS");
static_assert(sizeof(double) == 8 && sizeof(long long) == 8, "the state is a block of 8-byte words");

struct EvalTopk {
  int n;
  int k[FAVIT_EVAL_MAX_TOPK];
};

__device__ __forceinline__ int wave_sum_i32(int v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}
__device__ __forceinline__ long long wave_sum_i64(long long v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}
__device__ __forceinline__ double wave_sum_f64(double v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}

// Launch 1: one wave per row, lane l owns the classes l, l + 64, ...  The loss is cross_entropy_kernel's
// (norm_elem.hip): m = max, s = sum exp(x - m), lse = m + log s, loss = lse - x[y].  With fmaxf / __expf that loss is
// finite exactly when the row is usable -- a NaN (fmaxf drops it, the sum keeps it), a +inf (inf - inf), a -inf at
// the label (lse + inf) and an all -inf row (-inf - -inf) all leave it non-finite, while a -inf on another class adds
// exp(-inf) = 0 -- so no separate scan of the row is needed.
__global__ __launch_bounds__(256) void eval_rows_kernel(const float* __restrict__ logits, long ld,
                                                        const int64_t* __restrict__ labels,
                                                        float* __restrict__ loss_rows, int* __restrict__ pred_rows,
                                                        int* __restrict__ rank_rows, int B, int C) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int row = blockIdx.x * 4 + wave;
  if (row >= B) return;
  const int64_t lab64 = labels[row];
  if (lab64 < 0 || lab64 >= C) {                     // ignored (a padded batch's rows): the logits are not read
    if (lane == 0) {
      loss_rows[row] = __builtin_nanf("");
      pred_rows[row] = -1;
      rank_rows[row] = -1;
    }
    return;
  }
  const int lab = (int)lab64;
  const float* lr = logits + (long)row * ld;
  // pass 1: the maximum and the lane's first class that holds it (ascending c and a strict >)
  float m = -INFINITY, mz = -INFINITY;
  int zi = 0x7fffffff;
  for (int c = lane; c < C; c += 64) {
    const float v = lr[c];
    m = fmaxf(m, v);
    if (v > mz) { mz = v; zi = c; }
  }
  m = wave_max(m);
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    const float ov = __shfl_xor(mz, o, 64);
    const int oi = __shfl_xor(zi, o, 64);
    if (ov > mz || (ov == mz && oi < zi)) { mz = ov; zi = oi; }
  }
  // pass 2: the sum, and the classes that sort in front of the label (greater, or equal with a lower index)
  const float xy = lr[lab];
  float s = 0.f;
  int ahead = 0;
  for (int c = lane; c < C; c += 64) {
    const float v = lr[c];
    s += __expf(v - m);
    ahead += (v > xy || (v == xy && c < lab)) ? 1 : 0;
  }
  s = wave_sum(s);
  ahead = wave_sum_i32(ahead);
  if (lane == 0) {
    const float loss = (m + __logf(s)) - xy;
    const bool ok = isfinite(loss) && zi < C;        // (a finite loss has a finite maximum, so zi is a class)
    loss_rows[row] = loss;
    pred_rows[row] = ok ? zi : -1;
    rank_rows[row] = ok ? ahead : -1;
  }
}

// Launch 2: ONE workgroup.  Thread t takes the rows t, t + 256, ... in ascending order into private sums (doubles
// for the loss), the workgroup folds them -- shuffles inside a wave, then waves 0..3 in that order -- and thread 0
// adds the result to the state.  Which thread adds which row in which order depends on B alone: no float atomics,
// the same bits in every run.  The per-class and confusion counts are integer atomics (integer adds commute).
__global__ __launch_bounds__(256) void eval_fold_kernel(const int64_t* __restrict__ labels,
                                                        const float* __restrict__ loss_rows,
                                                        const int* __restrict__ pred_rows,
                                                        const int* __restrict__ rank_rows,
                                                        long long* __restrict__ state,
                                                        unsigned long long* __restrict__ class_total,
                                                        unsigned long long* __restrict__ class_correct,
                                                        unsigned long long* __restrict__ confusion, int B, int C,
                                                        EvalTopk topk) {
  __shared__ double red_f[4];
  __shared__ long long red_i[4][4 + FAVIT_EVAL_MAX_TOPK];
  double lsum = 0.0;
  long long cnt[4 + FAVIT_EVAL_MAX_TOPK];            // rows, ignored, nonfinite, (unused), hits[0..3]
#pragma unroll
  for (int i = 0; i < 4 + FAVIT_EVAL_MAX_TOPK; ++i) cnt[i] = 0;
  for (int b = threadIdx.x; b < B; b += 256) {
    const int64_t lab64 = labels[b];
    if (lab64 < 0 || lab64 >= C) { cnt[1] += 1; continue; }
    const int lab = (int)lab64, rank = rank_rows[b], pred = pred_rows[b];
    lsum += (double)loss_rows[b];
    cnt[0] += 1;
    if (class_total) atomicAdd(class_total + lab, 1ull);
    if (rank < 0 || pred < 0 || pred >= C) { cnt[2] += 1; continue; }     // a non-finite row hits no k
#pragma unroll
    for (int i = 0; i < FAVIT_EVAL_MAX_TOPK; ++i) cnt[4 + i] += (i < topk.n && rank < topk.k[i]) ? 1 : 0;
    if (class_correct && pred == lab) atomicAdd(class_correct + lab, 1ull);
    if (confusion) atomicAdd(confusion + (long)lab * C + pred, 1ull);
  }
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  lsum = wave_sum_f64(lsum);
#pragma unroll
  for (int i = 0; i < 4 + FAVIT_EVAL_MAX_TOPK; ++i) cnt[i] = wave_sum_i64(cnt[i]);
  if (lane == 0) {
    red_f[wave] = lsum;
#pragma unroll
    for (int i = 0; i < 4 + FAVIT_EVAL_MAX_TOPK; ++i) red_i[wave][i] = cnt[i];
  }
  __syncthreads();
  if (threadIdx.x != 0) return;
  const double sum = ((red_f[0] + red_f[1]) + red_f[2]) + red_f[3];
#pragma unroll
  for (int i = 0; i < 4 + FAVIT_EVAL_MAX_TOPK; ++i) cnt[i] = ((red_i[0][i] + red_i[1][i]) + red_i[2][i]) + red_i[3][i];
  double* fstate = reinterpret_cast<double*>(state);
  if (cnt[0] > 0) {                                  // a launch without a valid row is no batch
    fstate[FAVIT_EVAL_SLOT_LOSS_SUM] += sum;
    fstate[FAVIT_EVAL_SLOT_BATCH_MEAN_SUM] += sum / (double)cnt[0];
    state[FAVIT_EVAL_SLOT_ROWS] += cnt[0];
    state[FAVIT_EVAL_SLOT_BATCHES] += 1;
    state[FAVIT_EVAL_SLOT_NONFINITE] += cnt[2];
#pragma unroll
    for (int i = 0; i < FAVIT_EVAL_MAX_TOPK; ++i) state[FAVIT_EVAL_SLOT_HITS + i] += cnt[4 + i];
  }
  state[FAVIT_EVAL_SLOT_IGNORED] += cnt[1];
}

}  // namespace

extern "C" int favit_eval_metrics(const float* logits, int64_t ld, const int64_t* labels, float* loss_rows,
                                  int32_t* pred_rows, int32_t* rank_rows, int64_t* state, int64_t* class_total,
                                  int64_t* class_correct, int64_t* confusion, int32_t B, int32_t C, int32_t n_topk,
                                  int32_t k0, int32_t k1, int32_t k2, int32_t k3, void* stream) {
  if (!logits || !labels || !state || !loss_rows || !pred_rows || !rank_rows) return FAVIT_ERR_INVALID;
  if (C < 1 || B < 0 || ld < C) return FAVIT_ERR_INVALID;
  if (n_topk < 0 || n_topk > FAVIT_EVAL_MAX_TOPK) return FAVIT_ERR_INVALID;
  EvalTopk topk;
  topk.n = n_topk;
  const int32_t ks[FAVIT_EVAL_MAX_TOPK] = {k0, k1, k2, k3};
  for (int i = 0; i < FAVIT_EVAL_MAX_TOPK; ++i) {
    if (i < n_topk && ks[i] < 1) return FAVIT_ERR_INVALID;
    topk.k[i] = i < n_topk ? ks[i] : 0;
  }
  if (B == 0) return FAVIT_OK;
  hipStream_t st = as_stream(stream);
  hipLaunchKernelGGL(eval_rows_kernel, dim3((B + 3) / 4), dim3(256), 0, st, logits, (long)ld, labels, loss_rows,
                     pred_rows, rank_rows, (int)B, (int)C);
  FAVIT_CHECK_LAUNCH();
  hipLaunchKernelGGL(eval_fold_kernel, dim3(1), dim3(256), 0, st, labels, (const float*)loss_rows,
                     (const int*)pred_rows, (const int*)rank_rows, reinterpret_cast<long long*>(state),
                     reinterpret_cast<unsigned long long*>(class_total),
                     reinterpret_cast<unsigned long long*>(class_correct),
                     reinterpret_cast<unsigned long long*>(confusion), (int)B, (int)C, topk);
  FAVIT_CHECK_LAUNCH();
  return FAVIT_OK;
}
