// siren_kloss.hip — the k-space loss family of the MRI fork (loss_functions.py:12-64, 103-190) on
// gfx950, on the SIREN's own output layout (as siren_kspace.hip's ksse kernels):
//
//   pred, tgt, dpred : [B, N, C]
//   k0, mask         : [B, C, N]  (optional: the loss is then taken of y = DC(pred), and the backward
//                                  carries the DC's coefficient)
//
//   asinh  w sum (asinh(s y) / d - asinh(s t) / d)^2                 image_asinh       per channel
//   cubic  w sum (c(y) - c(t))^2, c(x) = sign(x) cbrt(|x| + eps)     image_mse_cubic   per channel
//   smape  w sum |y - t| / (eps + |t| + |y|)                         image_smape       per channel
//   l1     w sum |y - t|                                             kspace_l1         per channel
//   perp   w sum_pixels |y_re t_im - y_im t_re| / (|y| + eps)        image_perp        C == 2
//   log    w sum_pixels wm (log(|y| + eps) - log(|t| + eps))^2
//                       + wp (2 - cos(arg y - arg t))                image_mse_log     C == 2
//
// The forward is one launch (the deterministic sum of block_sum_handoff); the backward is
// one launch that recomputes dL/dy from pred and tgt, so nothing is saved between the two. The zero
// cases follow torch's autograd, which the reference runs on: sign(0) = 0, d|x|/dx = 0 at 0, the
// gradients of a complex magnitude and of a complex angle are 0 at 0, arg 0 = 0. Differences that
// are 0 for y == t are formed without contraction (__fmul_rn / __fsub_rn), so such a pixel's
// gradient is exactly 0. Bandwidth-bound elementwise passes: accurate OCML math, nothing
// architecture-specific beyond the hand-off.
#include "siren_common.h"

namespace siren {

constexpr int KL_THREADS = 256;

enum { KL_ASINH = 0, KL_CUBIC = 1, KL_SMAPE = 2, KL_L1 = 3, KL_PERP = 4, KL_LOG = 5 };

struct KlossArgs {
  const float* pred;   // [B, N, C]
  const float* k0;     // [B, C, N] (null: no data consistency)
  const float* mask;   // [B, C, N]
  const float* tgt;    // [B, N, C]
  const float* g;      // [1] upstream gradient of the loss (backward)
  float* out;          // forward: [1] the loss; backward: [B, N, C] dL / dpred
  float* partial;      // [LOSS_SLOTS] per-block sums (workspace, forward)
  unsigned* counter;   // zero between launches (the last block resets it)
  int64_t batch, npix;
  int C;
  float noise;
  float weight, eps, scale, divisor, mag_weight, phase_weight;  // siren_kloss_desc
};

DEV float kl_sign(float x) { return x > 0.f ? 1.f : (x < 0.f ? -1.f : 0.f); }

// one channel of the per-channel kinds: the summand f(y, t) and df/dy
template <int KIND>
DEV float kl_chan_value(const KlossArgs& a, float y, float t) {
  if (KIND == KL_ASINH) {
    const float d = __fsub_rn(__fdiv_rn(asinhf(__fmul_rn(a.scale, y)), a.divisor),
                              __fdiv_rn(asinhf(__fmul_rn(a.scale, t)), a.divisor));
    return __fmul_rn(d, d);
  } else if (KIND == KL_CUBIC) {
    const float cy = kl_sign(y) * cbrtf(__fadd_rn(fabsf(y), a.eps));
    const float ct = kl_sign(t) * cbrtf(__fadd_rn(fabsf(t), a.eps));
    const float d = __fsub_rn(cy, ct);
    return __fmul_rn(d, d);
  } else if (KIND == KL_SMAPE) {
    return __fdiv_rn(fabsf(__fsub_rn(y, t)), __fadd_rn(__fadd_rn(a.eps, fabsf(t)), fabsf(y)));
  } else {
    return fabsf(__fsub_rn(y, t));
  }
}

template <int KIND>
DEV float kl_chan_grad(const KlossArgs& a, float y, float t) {
  if (KIND == KL_ASINH) {
    const float sy = __fmul_rn(a.scale, y);
    const float d = __fsub_rn(__fdiv_rn(asinhf(sy), a.divisor), __fdiv_rn(asinhf(__fmul_rn(a.scale, t)), a.divisor));
    // d/dy asinh(s y) / div = s / (div sqrt(1 + (s y)^2))
    return 2.f * d * (a.scale / (a.divisor * sqrtf(fmaf(sy, sy, 1.f))));
  } else if (KIND == KL_CUBIC) {
    const float ry = cbrtf(__fadd_rn(fabsf(y), a.eps));
    const float sg = kl_sign(y);
    const float d = __fsub_rn(sg * ry, kl_sign(t) * cbrtf(__fadd_rn(fabsf(t), a.eps)));
    // d/dy sign(y) (|y| + eps)^(1/3) = 1 / (3 r^2), r = cbrt(|y| + eps); 0 at y = 0 (sign(0) = 0)
    return sg == 0.f ? 0.f : 2.f * d / (3.f * ry * ry);
  } else if (KIND == KL_SMAPE) {
    const float d = __fsub_rn(y, t);
    const float den = __fadd_rn(__fadd_rn(a.eps, fabsf(t)), fabsf(y));
    return kl_sign(d) / den - fabsf(d) * kl_sign(y) / (den * den);
  } else {
    return kl_sign(__fsub_rn(y, t));
  }
}

// a pixel's unit vector and magnitude: arg 0 = 0, so the unit vector of 0 is (1, 0)
DEV void kl_polar(float re, float im, float& m, float& ur, float& ui) {
  m = hypotf(re, im);
  if (m > 0.f) {
    ur = __fdiv_rn(re, m);
    ui = __fdiv_rn(im, m);
  } else {
    ur = 1.f;
    ui = 0.f;
  }
}

// the complex kinds, one pixel (y, t: real and imaginary channel)
template <int KIND>
DEV float kl_pix_value(const KlossArgs& a, const float* y, const float* t) {
  if (KIND == KL_PERP) {
    const float cr = __fsub_rn(__fmul_rn(y[0], t[1]), __fmul_rn(y[1], t[0]));
    return __fdiv_rn(fabsf(cr), __fadd_rn(hypotf(y[0], y[1]), a.eps));
  } else {
    float my, yr, yi, mt, tr, ti;
    kl_polar(y[0], y[1], my, yr, yi);
    kl_polar(t[0], t[1], mt, tr, ti);
    const float dl = __fsub_rn(logf(__fadd_rn(my, a.eps)), logf(__fadd_rn(mt, a.eps)));
    const float cs = __fadd_rn(__fmul_rn(yr, tr), __fmul_rn(yi, ti));  // cos(arg y - arg t)
    return __fadd_rn(__fmul_rn(a.mag_weight, __fmul_rn(dl, dl)), __fmul_rn(a.phase_weight, __fsub_rn(2.f, cs)));
  }
}

template <int KIND>
DEV void kl_pix_grad(const KlossArgs& a, const float* y, const float* t, float* gy) {
  if (KIND == KL_PERP) {
    const float cr = __fsub_rn(__fmul_rn(y[0], t[1]), __fmul_rn(y[1], t[0]));
    float m, ur, ui;
    kl_polar(y[0], y[1], m, ur, ui);
    if (!(m > 0.f)) ur = 0.f;  // d|y|/dy = 0 at 0
    const float den = __fadd_rn(m, a.eps);
    const float s = kl_sign(cr), q = fabsf(cr) / (den * den);
    gy[0] = s * t[1] / den - q * ur;
    gy[1] = -s * t[0] / den - q * ui;
  } else {
    float my, yr, yi, mt, tr, ti;
    kl_polar(y[0], y[1], my, yr, yi);
    kl_polar(t[0], t[1], mt, tr, ti);
    if (!(my > 0.f)) {  // |y| and arg y have zero gradients at 0
      gy[0] = gy[1] = 0.f;
      return;
    }
    const float le = __fadd_rn(my, a.eps);
    const float dl = __fsub_rn(logf(le), logf(__fadd_rn(mt, a.eps)));
    const float sn = __fsub_rn(__fmul_rn(yi, tr), __fmul_rn(yr, ti));  // sin(arg y - arg t)
    const float km = 2.f * a.mag_weight * dl / le;                       // d/d|y| of the magnitude term
    const float kp = a.phase_weight * sn / my;                           // d/d(arg y) of the phase term, over |y|
    gy[0] = km * yr - kp * yi;
    gy[1] = km * yi + kp * yr;
  }
}

// y = DC(pred) (or pred) of channel c of pixel q = b N + n
DEV float kl_y(const KlossArgs& a, int64_t q, int64_t b, int64_t n, int c) {
  const float v = a.pred[q * a.C + c];
  if (!a.k0) return v;
  const int64_t pl = (b * a.C + c) * a.npix + n;
  return dc_value(v, a.k0[pl], a.mask[pl], a.noise);
}

// Per-thread sums over a fixed grid-stride order, then block_sum_handoff (siren_common.h).
template <int KIND>
__global__ __launch_bounds__(KL_THREADS) void kloss_fwd_kernel(KlossArgs a) {
  float acc = 0.f;
  const int64_t nq = a.batch * a.npix;
  const int64_t stride = (int64_t)gridDim.x * KL_THREADS;
  for (int64_t q = (int64_t)blockIdx.x * KL_THREADS + threadIdx.x; q < nq; q += stride) {
    const int64_t b = q / a.npix, n = q - b * a.npix;
    if (KIND == KL_PERP || KIND == KL_LOG) {  // C == 2: (real, imaginary)
      const float y[2] = {kl_y(a, q, b, n, 0), kl_y(a, q, b, n, 1)};
      const float t[2] = {a.tgt[q * 2], a.tgt[q * 2 + 1]};
      acc = __fadd_rn(acc, kl_pix_value<KIND>(a, y, t));
    } else {
      for (int c = 0; c < a.C; ++c)
        acc = __fadd_rn(acc, kl_chan_value<KIND>(a, kl_y(a, q, b, n, c), a.tgt[q * a.C + c]));
    }
  }
  block_sum_handoff<KL_THREADS / 64>(acc, a.partial, a.counter, blockIdx.x, gridDim.x, a.out, a.weight);
}

// dL/dpred = g w dL/dy dc_coef(mask)
template <int KIND>
__global__ __launch_bounds__(KL_THREADS) void kloss_bwd_kernel(KlossArgs a) {
  const float k = a.g[0] * a.weight;
  const int64_t nq = a.batch * a.npix;
  const int64_t stride = (int64_t)gridDim.x * KL_THREADS;
  for (int64_t q = (int64_t)blockIdx.x * KL_THREADS + threadIdx.x; q < nq; q += stride) {
    const int64_t b = q / a.npix, n = q - b * a.npix;
    if (KIND == KL_PERP || KIND == KL_LOG) {
      const float y[2] = {kl_y(a, q, b, n, 0), kl_y(a, q, b, n, 1)};
      const float t[2] = {a.tgt[q * 2], a.tgt[q * 2 + 1]};
      float gy[2];
      kl_pix_grad<KIND>(a, y, t, gy);
#pragma unroll
      for (int c = 0; c < 2; ++c) {
        float v = k * gy[c];
        if (a.mask) v *= dc_coef(a.mask[(b * 2 + c) * a.npix + n], a.noise);
        a.out[q * 2 + c] = v;
      }
    } else {
      for (int c = 0; c < a.C; ++c) {
        float v = k * kl_chan_grad<KIND>(a, kl_y(a, q, b, n, c), a.tgt[q * a.C + c]);
        if (a.mask) v *= dc_coef(a.mask[(b * a.C + c) * a.npix + n], a.noise);
        a.out[q * a.C + c] = v;
      }
    }
  }
}

}  // namespace siren
