// siren_helmholtz.hip — the Helmholtz fitting loss (loss_functions.py:385-457 of the reference,
// helmholtz_pml, the forward problem) on gfx950, on the rows R = B N of a two-output SIREN of (x0, x1),
// the complex field u = pred[0] + i pred[1], and of its first and second derivatives:
//
//   x    [R, 2]        coordinates (model_in)
//   pred [R, 2]        u
//   jac  [R, 2, 2]     jac[c][d] = d pred_c / d x_d:  u_d = jac[0][d] + i jac[1][d]
//   hess [R, 2, 2, 2]  hess[c][j][k], only j == k is read:  u_dd = hess[0][d][d] + i hess[1][d][d]
//   src  [R, 2]        source_boundary_values
//   slow [R, 2]        the squared slowness m = slow[0] + i slow[1]
//   k    [1]           the wavenumber, on the device
//
// The perfectly matched layer begins at |x_d| = 1 - L, L = 0.5, with strength a0 = 5:
//   dw = max(-(x0 + 0.5), 0)  de = max(x0 - 0.5, 0)  ds = max(-(x1 + 0.5), 0)  dn = max(x1 - 0.5, 0)
//   px = a0 (dw^2 + de^2) / L^2     py = a0 (dn^2 + ds^2) / L^2     px' = 2 a0 (de - dw) / L^2   (py' alike)
//   ex = 1 - i px,  ey = 1 - i py,  A = ey / ex,  B = ex / ey,  C = ex ey
//   A_x0 = i px' ey / ex^2 = i px' A / ex,   B_x1 = i py' B / ey
// The reference differentiates through A u_0 and B u_1 by autograd; by the product rule that is
//   e = A_x0 u_0 + A u_00 + B_x1 u_1 + B u_11 + k^2 C m u
// which is linear in pred, jac and the diagonal of hess with per-row complex coefficients of x.
//
//   out[0]  diff_constraint_on   (N / 1e3) sum over rows and c of  src_c != 0 ? |e_c - src_c| : 0
//   out[1]  diff_constraint_off  sum over rows and c of            src_c == 0 ? |e_c| : 0
//   out[2]  data_term            0 (the forward problem has none)
//
// c = 0 is the real, c = 1 the imaginary channel; on or off is decided per element. N is the rows of one
// batch element. The forward is one launch (two deterministic sums behind one hand-off ticket); the
// backward is one launch that recomputes the coefficients and e and writes every element of dpred, djac
// and dhess (the four off-diagonal entries of a row's dhess get 0), so nothing is saved between the two
// and the callers' buffers need no clearing. With q_c = (src_c != 0 ? g0 w0 : g1) sign(e_c - src_c) and
// q = q0 + i q1, an operand v that enters as Z v receives conj(Z) q. sign(0) = 0, as torch's abs backward.
// Products and sums are formed without contraction (__fmul_rn / __fadd_rn / __fsub_rn), so the two
// kernels see the same e; strictly inside the layer's inner edge A = B = C = 1 and A_x0 = B_x1 = 0
// exactly. A bandwidth-light elementwise pass (88 bytes per row in, 56 out, plain dword loads and
// stores: the operands are only 4-byte aligned); nothing architecture-specific beyond the hand-off.
#include "siren_common.h"

namespace siren {

constexpr int HELM_THREADS = 256;
constexpr int HELM_TERMS = 2;         // the sums; out[2] is written as 0
constexpr int HELM_MAX_BLOCKS = 256;  // one per CU; 2 x 256 slots of LOSS_SLOTS
static_assert(HELM_TERMS * HELM_MAX_BLOCKS <= LOSS_SLOTS, "two slots per workgroup");

struct HelmArgs {
  const float* x;     // [R, 2]
  const float* pred;  // [R, 2]
  const float* jac;   // [R, 2, 2]
  const float* hess;  // [R, 2, 2, 2]
  const float* src;   // [R, 2]
  const float* slow;  // [R, 2]
  const float* k;     // [1] the wavenumber
  const float* g;     // [3] upstream gradient of the three terms (backward; g[2] is not read)
  float* out;         // [3] the terms (forward)
  float* dpred;       // [R, 2] (backward)
  float* djac;        // [R, 2, 2] (backward)
  float* dhess;       // [R, 2, 2, 2] (backward)
  float* partial;     // [LOSS_SLOTS] per-block sums, term k of block b in slot k nblocks + b (forward)
  unsigned* counter;  // zero between launches (the last block resets it)
  int64_t rows;
  float w[HELM_TERMS];  // N / 1e3, 1
};

struct Cx {
  float r, i;
};

DEV Cx cx_mul(Cx a, Cx b) {
  return {__fsub_rn(__fmul_rn(a.r, b.r), __fmul_rn(a.i, b.i)), __fadd_rn(__fmul_rn(a.r, b.i), __fmul_rn(a.i, b.r))};
}
// conj(z) q
DEV Cx cx_conj_mul(Cx z, Cx q) {
  return {__fadd_rn(__fmul_rn(z.r, q.r), __fmul_rn(z.i, q.i)), __fsub_rn(__fmul_rn(z.r, q.i), __fmul_rn(z.i, q.r))};
}
DEV Cx cx_add(Cx a, Cx b) { return {__fadd_rn(a.r, b.r), __fadd_rn(a.i, b.i)}; }
DEV float helm_sign(float v) { return v > 0.f ? 1.f : (v < 0.f ? -1.f : 0.f); }

// The five complex coefficients of a row: e = Ax u_0 + A u_00 + Bx u_1 + B u_11 + K u, K = k^2 C m.
struct HelmCoef {
  Cx A, Ax, B, Bx, K;
};

// p = a0 (lo^2 + hi^2) / L^2 and its derivative 2 a0 (hi - lo) / L^2 for the distances lo = max(-(t + 0.5), 0),
// hi = max(t - 0.5, 0) into the layer on the two sides of one axis (a0 / L^2 = 20)
DEV void helm_pml(float t, float* p, float* dp) {
  const float lo = fmaxf(-__fadd_rn(t, 0.5f), 0.f), hi = fmaxf(__fsub_rn(t, 0.5f), 0.f);
  *p = __fmul_rn(20.f, __fadd_rn(__fmul_rn(lo, lo), __fmul_rn(hi, hi)));
  *dp = __fmul_rn(40.f, __fsub_rn(hi, lo));
}

DEV HelmCoef helm_coef(float x0, float x1, Cx m, float k2) {
  float px, dpx, py, dpy;
  helm_pml(x0, &px, &dpx);
  helm_pml(x1, &py, &dpy);
  const Cx ex = {1.f, -px}, ey = {1.f, -py};
  const float nx = __fdiv_rn(1.f, __fadd_rn(1.f, __fmul_rn(px, px))), ny = __fdiv_rn(1.f, __fadd_rn(1.f, __fmul_rn(py, py)));
  const Cx ix = {nx, __fmul_rn(px, nx)}, iy = {ny, __fmul_rn(py, ny)};  // 1 / ex, 1 / ey
  HelmCoef c;
  c.A = cx_mul(ey, ix);
  c.B = cx_mul(ex, iy);
  const Cx ax = cx_mul(c.A, ix), bx = cx_mul(c.B, iy);
  c.Ax = {-__fmul_rn(dpx, ax.i), __fmul_rn(dpx, ax.r)};  // i px' (A / ex)
  c.Bx = {-__fmul_rn(dpy, bx.i), __fmul_rn(dpy, bx.r)};
  const Cx cm = cx_mul(cx_mul(ex, ey), m);
  c.K = {__fmul_rn(k2, cm.r), __fmul_rn(k2, cm.i)};
  return c;
}

DEV HelmCoef helm_row_coef(const HelmArgs& a, int64_t r, float k2) {
  return helm_coef(a.x[r * 2], a.x[r * 2 + 1], Cx{a.slow[r * 2], a.slow[r * 2 + 1]}, k2);
}

// e of row r, the terms added in the order of the formula above
DEV Cx helm_residual(const HelmArgs& a, int64_t r, const HelmCoef& c) {
  const float* j = a.jac + r * 4;
  const float* h = a.hess + r * 8;
  Cx e = cx_mul(c.Ax, Cx{j[0], j[2]});
  e = cx_add(e, cx_mul(c.A, Cx{h[0], h[4]}));
  e = cx_add(e, cx_mul(c.Bx, Cx{j[1], j[3]}));
  e = cx_add(e, cx_mul(c.B, Cx{h[3], h[7]}));
  return cx_add(e, cx_mul(c.K, Cx{a.pred[r * 2], a.pred[r * 2 + 1]}));
}

// Per-thread sums over a fixed grid-stride order, then block_sums_handoff (siren_common.h).
__global__ __launch_bounds__(HELM_THREADS) void helmholtz_fwd_kernel(HelmArgs a) {
  float acc[HELM_TERMS] = {0.f, 0.f};
  const float k = a.k[0], k2 = __fmul_rn(k, k);
  const int64_t stride = (int64_t)gridDim.x * HELM_THREADS;
  for (int64_t r = (int64_t)blockIdx.x * HELM_THREADS + threadIdx.x; r < a.rows; r += stride) {
    const Cx e = helm_residual(a, r, helm_row_coef(a, r, k2));
    const float ec[2] = {e.r, e.i};
#pragma unroll
    for (int c = 0; c < 2; ++c) {
      const float s = a.src[r * 2 + c];
      if (s != 0.f)
        acc[0] = __fadd_rn(acc[0], fabsf(__fsub_rn(ec[c], s)));
      else
        acc[1] = __fadd_rn(acc[1], fabsf(ec[c]));
    }
  }
  if (blockIdx.x == 0 && threadIdx.x == 0) a.out[2] = 0.f;
  block_sums_handoff<HELM_THREADS / 64, HELM_TERMS>(acc, a.partial, a.counter, blockIdx.x, gridDim.x, a.out, a.w);
}

__global__ __launch_bounds__(HELM_THREADS) void helmholtz_bwd_kernel(HelmArgs a) {
  const float k = a.k[0], k2 = __fmul_rn(k, k);
  const float gon = __fmul_rn(a.g[0], a.w[0]), goff = a.g[1];
  const int64_t stride = (int64_t)gridDim.x * HELM_THREADS;
  for (int64_t r = (int64_t)blockIdx.x * HELM_THREADS + threadIdx.x; r < a.rows; r += stride) {
    const HelmCoef c = helm_row_coef(a, r, k2);
    const Cx e = helm_residual(a, r, c);
    const float s0 = a.src[r * 2], s1 = a.src[r * 2 + 1];
    Cx q;
    q.r = s0 != 0.f ? __fmul_rn(gon, helm_sign(__fsub_rn(e.r, s0))) : __fmul_rn(goff, helm_sign(e.r));
    q.i = s1 != 0.f ? __fmul_rn(gon, helm_sign(__fsub_rn(e.i, s1))) : __fmul_rn(goff, helm_sign(e.i));
    const Cx u = cx_conj_mul(c.K, q), u0 = cx_conj_mul(c.Ax, q), u00 = cx_conj_mul(c.A, q);
    const Cx u1 = cx_conj_mul(c.Bx, q), u11 = cx_conj_mul(c.B, q);
    a.dpred[r * 2] = u.r;
    a.dpred[r * 2 + 1] = u.i;
    float* dj = a.djac + r * 4;
    dj[0] = u0.r;
    dj[1] = u1.r;
    dj[2] = u0.i;
    dj[3] = u1.i;
    float* dh = a.dhess + r * 8;
    dh[0] = u00.r;
    dh[1] = 0.f;
    dh[2] = 0.f;
    dh[3] = u11.r;
    dh[4] = u00.i;
    dh[5] = 0.f;
    dh[6] = 0.f;
    dh[7] = u11.i;
  }
}

}  // namespace siren
