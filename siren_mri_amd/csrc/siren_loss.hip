// siren_loss.hip — the k-space weighted SSE of image_mse (loss_functions.py:66-101) on gfx950:
//   forward : d = m (pred - tgt), loss = w sum d^2           (one launch, deterministic)
//   backward: dpred = m (d (g 2 w))                           (one launch; g = upstream scalar)
// The mask m (the high-frequency mask of utils.py:25-40, or none) broadcasts over the leading
// dimensions: element e uses m[e % mask_n]. Replaces the subtract / dot / scale / scale / multiply
// chain of the autograd path (six small launches) with two.
#include "siren_common.h"

namespace siren {

constexpr int SSE_THREADS = 256;

struct SseFwdArgs {
  const float* pred;
  const float* tgt;
  const float* mask;   // null: no mask
  float* d;            // [n] m (pred - tgt), kept for the backward
  float* loss;         // [1]
  float* partial;      // [LOSS_SLOTS] per-block sums (workspace)
  unsigned* counter;   // zero between launches (the last block resets it)
  int64_t n, mask_n;
  float weight;
};

// Per-thread sums over a fixed grid-stride order, then block_sum_handoff (siren_common.h): the result
// does not depend on scheduling.
__global__ __launch_bounds__(SSE_THREADS) void sse_fwd_kernel(SseFwdArgs a) {
  float acc = 0.f;
  const int64_t stride = (int64_t)gridDim.x * SSE_THREADS;
  const int64_t tid0 = (int64_t)blockIdx.x * SSE_THREADS + threadIdx.x;
  // 16-byte groups when every pointer and the mask period allow it, then the scalar tail
  const bool vec = ((((uintptr_t)a.pred | (uintptr_t)a.tgt | (uintptr_t)a.d | (uintptr_t)a.mask) & 15) == 0) &&
                   (!a.mask || a.mask_n % 4 == 0);
  const int64_t n4 = vec ? a.n / 4 : 0;
  for (int64_t q = tid0; q < n4; q += stride) {
    f32x4 v = ((const f32x4*)a.pred)[q] - ((const f32x4*)a.tgt)[q];
    if (a.mask) v = *(const f32x4*)(a.mask + (4 * q) % a.mask_n) * v;
    ((f32x4*)a.d)[q] = v;
#pragma unroll
    for (int j = 0; j < 4; ++j) acc = fmaf(v[j], v[j], acc);
  }
  for (int64_t e = 4 * n4 + tid0; e < a.n; e += stride) {
    float v = a.pred[e] - a.tgt[e];
    if (a.mask) v = a.mask[e % a.mask_n] * v;
    a.d[e] = v;
    acc = fmaf(v, v, acc);
  }
  block_sum_handoff<SSE_THREADS / 64>(acc, a.partial, a.counter, blockIdx.x, gridDim.x, a.loss, a.weight);
}

struct SseBwdArgs {
  const float* d;
  const float* mask;
  const float* g;      // [1] upstream gradient of the loss
  float* out;          // [n]
  int64_t n, mask_n;
  float scale;         // 2 w
};

__global__ __launch_bounds__(SSE_THREADS) void sse_bwd_kernel(SseBwdArgs a) {
  const float k = a.g[0] * a.scale;
  const int64_t stride = (int64_t)gridDim.x * SSE_THREADS;
  const int64_t tid0 = (int64_t)blockIdx.x * SSE_THREADS + threadIdx.x;
  const bool vec = ((((uintptr_t)a.d | (uintptr_t)a.out | (uintptr_t)a.mask) & 15) == 0) &&
                   (!a.mask || a.mask_n % 4 == 0);
  const int64_t n4 = vec ? a.n / 4 : 0;
  for (int64_t q = tid0; q < n4; q += stride) {
    f32x4 v = ((const f32x4*)a.d)[q] * k;
    if (a.mask) v = *(const f32x4*)(a.mask + (4 * q) % a.mask_n) * v;
    ((f32x4*)a.out)[q] = v;
  }
  for (int64_t e = 4 * n4 + tid0; e < a.n; e += stride) {
    float v = a.d[e] * k;
    if (a.mask) v = a.mask[e % a.mask_n] * v;
    a.out[e] = v;
  }
}

}  // namespace siren
