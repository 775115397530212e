// siren_kfft.hip — a batched 2-D FFT of small square slices and the image-domain (IFT) k-space loss
// of the MRI fork (ift_image_mse, loss_functions.py:192-229) on gfx950, on the SIREN's own output
// layout (as siren_kloss.hip):
//
//   x, out, pred, tgt, dpred : [B, N, 2]  (real, imaginary), N = side^2, pixels row-major (lin2img)
//   k0, mask                 : [B, 2, N]  (optional: the loss is then taken of y = DC(pred), and the
//                                          backward carries the DC's coefficient)
//   img_mask                 : [N] (batch stride 0) or [B, N], optional, on the magnitude images
//
//   loss = img_weight    sum m (|ifft2 y| - |ifft2 t|)^2
//        + l1_weight     sum |y|                     (complex magnitudes)
//        + kspace_weight sum (y - t)^2               (both channels)
//
// side is 8, 16, 32, 64 or 128. One workgroup owns one slice and keeps it in LDS for the whole
// transform: radix-2 decimation in frequency, in place, a row pass (lanes along a row) then a column
// pass (lanes along a row again, one column each), so neither pass meets a bank conflict beyond the
// short butterflies' 2-way one; the result lies bit-reversed in both indices and is read from there
// (the row stride is padded by one element for that read). Twiddles come from a per-workgroup table
// of sincospif of the exact rational -2 j / side. The butterflies are written without contraction
// freedom (__fmaf_rn / __fmul_rn), so every transform of the same values gives the same bits: a slice
// with y == t bitwise has an image term and an image gradient of exactly 0. ifft2's 1 / side^2 is a
// power of two, applied once on the way out; fft2 is unscaled (torch's conventions).
//
// The loss forward is one launch: transform t and keep |x_t| in registers (the thread that owns a
// pixel owns it in both transforms), load y into the tile while summing the two k-space terms,
// transform y, sum the image term; a fixed tree per slice, and the last workgroup adds the slice sums
// in slice order (the hand-off of siren_common.h, one slot per slice). The backward is one launch that
// recomputes everything from pred and tgt: g_x = 2 w m (|x_y| - |x_t|) x_y / |x_y| (0 at |x_y| = 0,
// torch's gradient of a complex magnitude), the forward transform of g_x over side^2 (the adjoint of
// ifft2), plus the k-space terms' gradients, times the upstream gradient and the DC's coefficient.
#include "siren_common.h"

namespace siren {

template <int L>
struct KfGeom {
  static constexpr int S = 1 << L;                 // side
  static constexpr int N = S * S;                  // pixels of a slice
  static constexpr int LD = S + 1;                 // row stride of the tile, in complex elements
  static constexpr int T = N < 1024 ? N : 1024;    // threads of the slice's workgroup
  static constexpr int PPT = N / T;                // pixels a thread owns: p = j T + threadIdx.x
};

// side 128: 128 * 129 * 8 + 64 * 8 = 132,608 bytes
template <int L>
struct KfTile {
  float2 v[KfGeom<L>::S * KfGeom<L>::LD];
  float2 tw[KfGeom<L>::S / 2];  // exp(-2 pi i j / side)
};

struct KfftArgs {
  const float* x;  // [B, N, 2]
  float* out;      // [B, N, 2]
  int inverse;
};

struct KiftArgs {
  const float* pred;      // [B, N, 2]
  const float* k0;        // [B, 2, N] (null: no data consistency)
  const float* mask;      // [B, 2, N]
  const float* tgt;       // [B, N, 2]
  const float* img_mask;  // [N] or [B, N] (null: none)
  const float* g;         // [1] upstream gradient of the loss (backward)
  float* out;             // forward: [1] the loss; backward: [B, N, 2] dL / dpred
  float* partial;         // [LOSS_SLOTS] per-slice sums (workspace, forward)
  unsigned* counter;      // zero between launches (the last workgroup resets it)
  int64_t img_mask_bstride;  // 0 or N
  float noise;
  float img_weight, l1_weight, kspace_weight;  // siren_kift_desc
};

template <int L>
DEV void kf_twiddles(KfTile<L>& t) {
  using G = KfGeom<L>;
  for (int j = threadIdx.x; j < G::S / 2; j += G::T) {
    float sn, cs;
    sincospif(-(float)(2 * j) / (float)G::S, &sn, &cs);
    t.tw[j] = make_float2(cs, sn);
  }
}

// threadIdx.x, opaque to the compiler: what is computed from two calls' values is not shared
DEV int kf_tid() {
  int tid = threadIdx.x;
  asm volatile("" : "+v"(tid));
  return tid;
}

// a' = a + b, b' = (a - b) w
DEV void kf_bfly(float2& a, float2& b, float2 w) {
  const float dr = __fsub_rn(a.x, b.x), di = __fsub_rn(a.y, b.y);
  a.x = __fadd_rn(a.x, b.x);
  a.y = __fadd_rn(a.y, b.y);
  b.x = __fmaf_rn(dr, w.x, -__fmul_rn(di, w.y));
  b.y = __fmaf_rn(dr, w.y, __fmul_rn(di, w.x));
}

// The per-pixel loops are unrolled (a thread's pixels live in registers); left alone, the scheduler
// hoists every pixel's global loads to the front (side 128: 16 pixels x 8 loads) and spills. Nothing
// moves across the end of a group of four pixels.
DEV void kf_group(int j) {
  if ((j & 3) == 3) __builtin_amdgcn_sched_barrier(0);
}

// where pixel p's value lies: in natural order (before a transform), bit-reversed in both indices (after)
template <int L>
DEV int kf_nat(int p) {
  return (p >> L) * KfGeom<L>::LD + (p & (KfGeom<L>::S - 1));
}
template <int L>
DEV int kf_rev(int p) {
  const unsigned r = __brev((unsigned)(p >> L)) >> (32 - L), c = __brev((unsigned)(p & (KfGeom<L>::S - 1))) >> (32 - L);
  return (int)r * KfGeom<L>::LD + (int)c;
}

// The unscaled 2-D DFT (inverse: conjugate twiddles) of the tile, in place; natural order in,
// bit-reversed out. Barriers: the caller's before (the tile is filled), one after every stage.
template <int L>
DEV void kf_transform(KfTile<L>& t, bool inverse) {
  using G = KfGeom<L>;
#pragma unroll
  for (int pass = 0; pass < 2; ++pass) {
#pragma unroll
    for (int s = 0; s < L; ++s) {
      const int lh = L - 1 - s, h = 1 << lh;  // the butterflies' span
      // The butterflies' addresses depend on the thread alone, so the compiler would share them among
      // a kernel's transforms and keep all 2 L PPT / 2 of them in registers (side 128: it spilled).
      // Each stage derives its own from an opaque copy of the thread index (kf_tid).
      const int tid = kf_tid();
      for (int q = tid; q < G::N / 2; q += G::T) {
        // rows: butterfly b of row `line`; columns: butterfly b of column `line` (lanes along the row)
        const int line = pass == 0 ? q >> (L - 1) : q & (G::S - 1);
        const int b = pass == 0 ? q & (G::S / 2 - 1) : q >> L;
        const int k = b & (h - 1);
        const int i0 = ((b >> lh) << (lh + 1)) + k;
        float2 w = t.tw[k << s];
        if (inverse) w.y = -w.y;
        float2* p0 = pass == 0 ? t.v + line * G::LD + i0 : t.v + i0 * G::LD + line;
        float2* p1 = p0 + (pass == 0 ? h : h * G::LD);
        float2 a = *p0, c = *p1;
        kf_bfly(a, c, w);
        *p0 = a;
        *p1 = c;
      }
      __syncthreads();
    }
  }
}

// y = DC(pred) (or pred) of pixel p of a slice, both channels
DEV float2 kf_y(const KiftArgs& a, int64_t slice, int64_t npix, int p) {
  const int64_t q = (slice * npix + p) * 2;
  float2 y = make_float2(a.pred[q], a.pred[q + 1]);
  if (a.k0) {
    const int64_t pl = slice * 2 * npix + p;
    y.x = dc_value(y.x, a.k0[pl], a.mask[pl], a.noise);
    y.y = dc_value(y.y, a.k0[pl + npix], a.mask[pl + npix], a.noise);
  }
  return y;
}

// tgt's slice into the tile, ifft2, |x_t| of the thread's pixels; leaves the tile free (barrier)
template <int L>
DEV void kf_target_magnitudes(KfTile<L>& t, const float* tgt, int64_t slice, float* mt) {
  using G = KfGeom<L>;
  const float inv_n = 1.f / (float)G::N;
#pragma unroll
  for (int j = 0, tid = kf_tid(); j < G::PPT; ++j) {
    const int p = j * G::T + tid;
    const int64_t q = (slice * G::N + p) * 2;
    t.v[kf_nat<L>(p)] = make_float2(tgt[q], tgt[q + 1]);
  }
  __syncthreads();
  kf_transform<L>(t, true);
#pragma unroll
  for (int j = 0, tid = kf_tid(); j < G::PPT; ++j) {
    const float2 x = t.v[kf_rev<L>(j * G::T + tid)];
    mt[j] = hypotf(__fmul_rn(x.x, inv_n), __fmul_rn(x.y, inv_n));
    kf_group(j);
  }
  __syncthreads();
}

template <int L>
__global__ __launch_bounds__(KfGeom<L>::T) void kfft2_kernel(KfftArgs a) {
  using G = KfGeom<L>;
  __shared__ KfTile<L> t;
  const int64_t slice = blockIdx.x;
  kf_twiddles<L>(t);
#pragma unroll
  for (int j = 0, tid = kf_tid(); j < G::PPT; ++j) {
    const int p = j * G::T + tid;
    const int64_t q = (slice * G::N + p) * 2;
    t.v[kf_nat<L>(p)] = make_float2(a.x[q], a.x[q + 1]);
  }
  __syncthreads();
  kf_transform<L>(t, a.inverse != 0);
  const float scale = a.inverse ? 1.f / (float)G::N : 1.f;
#pragma unroll
  for (int j = 0, tid = kf_tid(); j < G::PPT; ++j) {
    const int p = j * G::T + tid;
    const int64_t q = (slice * G::N + p) * 2;
    const float2 x = t.v[kf_rev<L>(p)];
    a.out[q] = __fmul_rn(x.x, scale);
    a.out[q + 1] = __fmul_rn(x.y, scale);
  }
}

template <int L>
__global__ __launch_bounds__(KfGeom<L>::T) void kift_fwd_kernel(KiftArgs a) {
  using G = KfGeom<L>;
  __shared__ KfTile<L> t;
  __shared__ float red[16];
  __shared__ float slots[LOSS_SLOTS];
  __shared__ unsigned ticket;
  const int64_t slice = blockIdx.x;
  const float inv_n = 1.f / (float)G::N;
  kf_twiddles<L>(t);
  float mt[G::PPT];
  kf_target_magnitudes<L>(t, a.tgt, slice, mt);
  // y into the tile; the two k-space terms on the way
  float s_l1 = 0.f, s_ks = 0.f, s_img = 0.f;
#pragma unroll
  for (int j = 0, tid = kf_tid(); j < G::PPT; ++j) {
    const int p = j * G::T + tid;
    const int64_t q = (slice * G::N + p) * 2;
    const float2 y = kf_y(a, slice, G::N, p);
    const float d0 = __fsub_rn(y.x, a.tgt[q]), d1 = __fsub_rn(y.y, a.tgt[q + 1]);
    s_l1 = __fadd_rn(s_l1, hypotf(y.x, y.y));
    s_ks = __fadd_rn(s_ks, __fmaf_rn(d1, d1, __fmul_rn(d0, d0)));
    t.v[kf_nat<L>(p)] = y;
    kf_group(j);
  }
  __syncthreads();
  kf_transform<L>(t, true);
#pragma unroll
  for (int j = 0, tid = kf_tid(); j < G::PPT; ++j) {
    const int p = j * G::T + tid;
    const float2 x = t.v[kf_rev<L>(p)];
    const float d = __fsub_rn(hypotf(__fmul_rn(x.x, inv_n), __fmul_rn(x.y, inv_n)), mt[j]);
    const float m = a.img_mask ? a.img_mask[slice * a.img_mask_bstride + p] : 1.f;
    s_img = __fadd_rn(s_img, __fmul_rn(m, __fmul_rn(d, d)));
    kf_group(j);
  }
  float acc = __fmul_rn(a.img_weight, s_img);
  acc = __fadd_rn(acc, __fmul_rn(a.l1_weight, s_l1));
  acc = __fadd_rn(acc, __fmul_rn(a.kspace_weight, s_ks));
  // the slice's sum: a fixed tree that does not depend on the batch
  acc = wave_sum(acc);
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = acc;
  __syncthreads();
  if (threadIdx.x == 0) {
    float s = 0.f;
#pragma unroll
    for (int w = 0; w < (G::T + 63) / 64; ++w) s += red[w];
    ticket = handoff_publish(a.partial + blockIdx.x, s, a.counter);
  }
  __syncthreads();
  if (ticket != gridDim.x - 1) return;
  // the last workgroup: the slice sums in slice order
  for (unsigned b = threadIdx.x; b < gridDim.x; b += G::T) slots[b] = handoff_take(a.partial + b);
  __syncthreads();
  if (threadIdx.x == 0) {
    float tot = 0.f;
    for (unsigned b = 0; b < gridDim.x; ++b) tot = __fadd_rn(tot, slots[b]);
    a.out[0] = tot;
    handoff_rearm(a.counter);
  }
}

template <int L>
__global__ __launch_bounds__(KfGeom<L>::T) void kift_bwd_kernel(KiftArgs a) {
  using G = KfGeom<L>;
  __shared__ KfTile<L> t;
  const int64_t slice = blockIdx.x;
  const float inv_n = 1.f / (float)G::N;
  const float g0 = a.g[0];
  kf_twiddles<L>(t);
  float mt[G::PPT];
  kf_target_magnitudes<L>(t, a.tgt, slice, mt);
#pragma unroll
  for (int j = 0, tid = kf_tid(); j < G::PPT; ++j) {
    const int p = j * G::T + tid;
    t.v[kf_nat<L>(p)] = kf_y(a, slice, G::N, p);
    kf_group(j);
  }
  __syncthreads();
  kf_transform<L>(t, true);
  // g_x = 2 w m (|x_y| - |x_t|) x_y / |x_y|, 0 at |x_y| = 0
  float2 gx[G::PPT];
#pragma unroll
  for (int j = 0, tid = kf_tid(); j < G::PPT; ++j) {
    const int p = j * G::T + tid;
    const float2 v = t.v[kf_rev<L>(p)];
    const float xr = __fmul_rn(v.x, inv_n), xi = __fmul_rn(v.y, inv_n);
    const float my = hypotf(xr, xi);
    const float m = a.img_mask ? a.img_mask[slice * a.img_mask_bstride + p] : 1.f;
    const float k = __fmul_rn(__fmul_rn(2.f * a.img_weight, m), __fsub_rn(my, mt[j]));
    gx[j] = my > 0.f ? make_float2(__fmul_rn(k, __fdiv_rn(xr, my)), __fmul_rn(k, __fdiv_rn(xi, my)))
                     : make_float2(0.f, 0.f);
    kf_group(j);
  }
  __syncthreads();  // every bit-reversed read is done before the natural-order writes
#pragma unroll
  for (int j = 0, tid = kf_tid(); j < G::PPT; ++j) t.v[kf_nat<L>(j * G::T + tid)] = gx[j];
  __syncthreads();
  kf_transform<L>(t, false);
#pragma unroll
  for (int j = 0, tid = kf_tid(); j < G::PPT; ++j) {
    const int p = j * G::T + tid;
    const int64_t q = (slice * G::N + p) * 2;
    const float2 v = t.v[kf_rev<L>(p)];
    const float2 y = kf_y(a, slice, G::N, p);
    const float my = hypotf(y.x, y.y);
    float d0 = __fmul_rn(v.x, inv_n), d1 = __fmul_rn(v.y, inv_n);
    if (my > 0.f) {  // d|y|/dy = 0 at 0
      d0 = __fmaf_rn(a.l1_weight, __fdiv_rn(y.x, my), d0);
      d1 = __fmaf_rn(a.l1_weight, __fdiv_rn(y.y, my), d1);
    }
    d0 = __fmaf_rn(2.f * a.kspace_weight, __fsub_rn(y.x, a.tgt[q]), d0);
    d1 = __fmaf_rn(2.f * a.kspace_weight, __fsub_rn(y.y, a.tgt[q + 1]), d1);
    d0 *= g0;
    d1 *= g0;
    if (a.mask) {
      const int64_t pl = slice * 2 * G::N + p;
      d0 *= dc_coef(a.mask[pl], a.noise);
      d1 *= dc_coef(a.mask[pl + G::N], a.noise);
    }
    a.out[q] = d0;
    a.out[q + 1] = d1;
    kf_group(j);
  }
}

}  // namespace siren
