// siren_wave.hip — the wave-equation fitting loss (loss_functions.py:358-382 of the reference, wave_pml)
// on gfx950, on the rows R = B N of a one-output SIREN of (t, x, y) and of its first and second
// derivatives:
//
//   pred [R]        model output u
//   jac  [R, 3]     diff_operators.jacobian(y, x): u_t = jac[r][0]
//   hess [R, 3, 3]  diff_operators.hessian(y, x), or null: u_tt = h[0][0], lap = h[1][1] + h[2][2]
//   src, slow [R]   the source's boundary values; the squared slowness
//   mask [R] uint8  the Dirichlet mask (torch.bool storage)
//
//   out[0]  dirichlet            (N / 1e1) sum  mask ? |pred - src| : 0
//   out[1]  neumann              (N / 1e2) sum  mask ? |u_t| : 0
//   out[2]  diff_constraint_hom  hess ? sum |u_tt - (1 / slow) lap| : 0      (every row, masked or not)
//
// N is the rows of one batch element (the reference's x.shape[1]), not R. src is read on masked rows
// only: the reference selects y[mask] - src[mask] first, so whatever an unmasked row holds there (NaN
// included) reaches no result.
//
// The forward is one launch (the three deterministic sums of block_sums_handoff, one ticket); the
// backward is one launch that recomputes dL/dpred, dL/djac and dL/dhess from the same operands and the
// upstream 3-vector and writes every element of the three (the columns and entries the loss does not
// read get 0), so nothing is saved between the two and the callers' buffers need no clearing. sign(0) =
// 0, as torch's abs backward. The differences are formed without contraction (__fsub_rn / __fmul_rn /
// __fadd_rn), so pred == src and u_tt == lap / slow give gradients of exactly 0. A bandwidth-light
// elementwise pass (about 64 bytes per row in, 52 out; rows 12 and 36 bytes apart: plain dword loads
// and stores): nothing architecture-specific beyond the hand-off.
#include "siren_common.h"

namespace siren {

constexpr int WAVE_THREADS = 256;
constexpr int WAVE_TERMS = 3;
constexpr int WAVE_MAX_BLOCKS = 256;  // one per CU; 3 x 256 slots of LOSS_SLOTS
static_assert(WAVE_TERMS * WAVE_MAX_BLOCKS <= LOSS_SLOTS, "three slots per workgroup");

struct WaveArgs {
  const float* pred;          // [R]
  const float* jac;           // [R, 3]
  const float* hess;          // [R, 3, 3] or null
  const float* src;           // [R]
  const float* slow;          // [R]
  const unsigned char* mask;  // [R]
  const float* g;             // [3] upstream gradient of the three terms (backward)
  float* out;                 // [3] the terms (forward)
  float* dpred;               // [R] (backward)
  float* djac;                // [R, 3] (backward)
  float* dhess;               // [R, 3, 3] or null (backward)
  float* partial;             // [LOSS_SLOTS] per-block sums, term k of block b in slot k nblocks + b (forward)
  unsigned* counter;          // zero between launches (the last block resets it)
  int64_t rows;
  float w[WAVE_TERMS];        // N / 10, N / 100, 1
};

DEV float wave_sign(float x) { return x > 0.f ? 1.f : (x < 0.f ? -1.f : 0.f); }

// e = u_tt - (1 / slow) (h11 + h22) in the reference's order of operations; inv = 1 / slow
DEV float wave_residual(const float* h, float slow, float* inv) {
  *inv = __fdiv_rn(1.f, slow);
  return __fsub_rn(h[0], __fmul_rn(*inv, __fadd_rn(h[4], h[8])));
}

// Per-thread sums over a fixed grid-stride order, then block_sums_handoff (siren_common.h).
template <bool HESS>
__global__ __launch_bounds__(WAVE_THREADS) void wave_fwd_kernel(WaveArgs a) {
  float acc[WAVE_TERMS] = {0.f, 0.f, 0.f};
  const int64_t stride = (int64_t)gridDim.x * WAVE_THREADS;
  for (int64_t r = (int64_t)blockIdx.x * WAVE_THREADS + threadIdx.x; r < a.rows; r += stride) {
    if (a.mask[r]) {
      acc[0] = __fadd_rn(acc[0], fabsf(__fsub_rn(a.pred[r], a.src[r])));
      acc[1] = __fadd_rn(acc[1], fabsf(a.jac[r * 3]));
    }
    if (HESS) {
      float inv;
      acc[2] = __fadd_rn(acc[2], fabsf(wave_residual(a.hess + r * 9, a.slow[r], &inv)));
    }
  }
  block_sums_handoff<WAVE_THREADS / 64, WAVE_TERMS>(acc, a.partial, a.counter, blockIdx.x, gridDim.x, a.out, a.w);
}

// dpred = mask ? g0 w0 sign(pred - src) : 0;  djac[0] = mask ? g1 w1 sign(u_t) : 0, djac[1] = djac[2] = 0
// q = g2 sign(e): dhess[0][0] = q, dhess[1][1] = dhess[2][2] = -q / slow, the six others 0
template <bool HESS>
__global__ __launch_bounds__(WAVE_THREADS) void wave_bwd_kernel(WaveArgs a) {
  const float k0 = __fmul_rn(a.g[0], a.w[0]), k1 = __fmul_rn(a.g[1], a.w[1]), k2 = a.g[2];
  const int64_t stride = (int64_t)gridDim.x * WAVE_THREADS;
  for (int64_t r = (int64_t)blockIdx.x * WAVE_THREADS + threadIdx.x; r < a.rows; r += stride) {
    float dp = 0.f, dj = 0.f;
    if (a.mask[r]) {
      dp = __fmul_rn(k0, wave_sign(__fsub_rn(a.pred[r], a.src[r])));
      dj = __fmul_rn(k1, wave_sign(a.jac[r * 3]));
    }
    a.dpred[r] = dp;
    a.djac[r * 3] = dj;
    a.djac[r * 3 + 1] = 0.f;
    a.djac[r * 3 + 2] = 0.f;
    if (HESS) {
      float inv;
      const float q = __fmul_rn(k2, wave_sign(wave_residual(a.hess + r * 9, a.slow[r], &inv)));
      const float ql = -__fmul_rn(q, inv);
      float* d = a.dhess + r * 9;
#pragma unroll
      for (int k = 0; k < 9; ++k) d[k] = k == 0 ? q : ((k == 4 || k == 8) ? ql : 0.f);
    }
  }
}

}  // namespace siren
