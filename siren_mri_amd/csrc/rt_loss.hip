// rt_loss.hip — image and k-space losses, data consistency, Fourier features and the sin/cos probe
// (kernels in siren_loss.hip, siren_kspace.hip, siren_kloss.hip, siren_sdf.hip, siren_wave.hip, siren_helmholtz.hip,
// siren_kfft.hip). Included by siren_runtime.hip.
namespace {

// The hand-off workspace of a loss forward, checked and sliced; 0 or SIREN_ENOSPACE (message set), as
// every other entry point answers a missing or short workspace (check_buffers).
int loss_slots(const char* what, void* workspace, int64_t ws_bytes, float** partial, unsigned** counter) {
  if (!workspace || ws_bytes < siren_sse_workspace_bytes())
    return fail(SIREN_ENOSPACE, "%s: workspace of %lld bytes, need %lld", what, (long long)ws_bytes,
                (long long)siren_sse_workspace_bytes());
  loss_workspace_slice(workspace, partial, counter);
  return SIREN_OK;
}

// the forms of a k-space loss kernel, by SIREN_KLOSS_* (kind checked by kloss_check)
#define SIREN_KINDS(K) \
  {SIREN_K(K<KL_ASINH>), SIREN_K(K<KL_CUBIC>), SIREN_K(K<KL_SMAPE>), SIREN_K(K<KL_L1>), SIREN_K(K<KL_PERP>), SIREN_K(K<KL_LOG>)}
const Kernel<KlossArgs> kKlossFwd[SIREN_KLOSS_KINDS] = SIREN_KINDS(kloss_fwd_kernel);
const Kernel<KlossArgs> kKlossBwd[SIREN_KLOSS_KINDS] = SIREN_KINDS(kloss_bwd_kernel);

// the argument checks both entry points share; 0 or SIREN_EINVAL (message set)
int kloss_check(const char* what, int kind, const siren_kloss_desc* desc, const float* k0, const float* mask,
                int64_t batch, int64_t npix, int channels) {
  if (kind < 0 || kind >= SIREN_KLOSS_KINDS)
    return fail(SIREN_EINVAL, "%s: kind %d outside [0, %d)", what, kind, (int)SIREN_KLOSS_KINDS);
  if (!desc) return fail(SIREN_EINVAL, "%s: null descriptor", what);
  if (channels < 1 || channels > KSPACE_MAXC)
    return fail(SIREN_EINVAL, "%s: channels %d outside [1, %d]", what, channels, KSPACE_MAXC);
  if ((kind == SIREN_KLOSS_PERP || kind == SIREN_KLOSS_LOG) && channels != 2)
    return fail(SIREN_EINVAL, "%s: kind %d (%s) takes complex pixels, channels == 2, got %d", what, kind,
                kind == SIREN_KLOSS_PERP ? "perp" : "log", channels);
  if ((!k0) != (!mask)) return fail(SIREN_EINVAL, "%s: k0 and mask go together (data consistency)", what);
  if (batch < 0 || npix < 0)
    return fail(SIREN_EINVAL, "%s: bad sizes (batch=%lld, npix=%lld)", what, (long long)batch, (long long)npix);
  return SIREN_OK;
}

KlossArgs kloss_args(const siren_kloss_desc* d, const float* pred, const float* k0, const float* mask,
                     const float* tgt, int64_t batch, int64_t npix, int channels, float noise) {
  KlossArgs a;
  memset(&a, 0, sizeof(a));
  a.pred = pred;
  a.k0 = k0;
  a.mask = mask;
  a.tgt = tgt;
  a.batch = batch;
  a.npix = npix;
  a.C = channels;
  a.noise = noise;
  a.weight = d->weight;
  a.eps = d->eps;
  a.scale = d->scale;
  a.divisor = d->divisor;
  a.mag_weight = d->mag_weight;
  a.phase_weight = d->phase_weight;
  return a;
}

// the forms of the signed-distance loss kernels, by D - 2 (dims checked by sdf_check)
const Kernel<SdfArgs> kSdfFwd[2] = {SIREN_K(sdf_fwd_kernel<2>), SIREN_K(sdf_fwd_kernel<3>)};
const Kernel<SdfArgs> kSdfBwd[2] = {SIREN_K(sdf_bwd_kernel<2>), SIREN_K(sdf_bwd_kernel<3>)};

// the argument checks both entry points share; 0 or SIREN_EINVAL (message set)
int sdf_check(const char* what, const float* pred, const float* grad, const float* sdf, const float* nrm,
              int64_t rows, int dims) {
  if (dims != 2 && dims != 3) return fail(SIREN_EINVAL, "%s: dims %d is neither 2 nor 3", what, dims);
  if (rows < 0) return fail(SIREN_EINVAL, "%s: bad size (rows=%lld)", what, (long long)rows);
  if (rows > 0 && (!pred || !grad || !sdf || !nrm)) return fail(SIREN_EINVAL, "%s: null pointer", what);
  return SIREN_OK;
}

// the reference's constants (loss_functions.py:481-484) over the row count: each term is a mean
SdfArgs sdf_args(const float* pred, const float* grad, const float* sdf, const float* nrm, int64_t rows) {
  SdfArgs a;
  memset(&a, 0, sizeof(a));
  a.pred = pred;
  a.grad = grad;
  a.sdf = sdf;
  a.nrm = nrm;
  a.rows = rows;
  const double c[SDF_TERMS] = {3e3, 1e2, 1e2, 5e1};
  for (int k = 0; k < SDF_TERMS; ++k) a.w[k] = rows > 0 ? (float)(c[k] / (double)rows) : 0.f;
  return a;
}

// the forms of the wave-equation loss kernels, by whether the Hessian is given
const Kernel<WaveArgs> kWaveFwd[2] = {SIREN_K(wave_fwd_kernel<false>), SIREN_K(wave_fwd_kernel<true>)};
const Kernel<WaveArgs> kWaveBwd[2] = {SIREN_K(wave_bwd_kernel<false>), SIREN_K(wave_bwd_kernel<true>)};

// the argument checks both entry points share; 0 or SIREN_EINVAL (message set)
int wave_check(const char* what, const float* pred, const float* jac, const float* src, const float* slow,
               const unsigned char* mask, int64_t rows, int64_t rows_per_batch) {
  if (rows < 0) return fail(SIREN_EINVAL, "%s: bad size (rows=%lld)", what, (long long)rows);
  if (rows > 0 && rows_per_batch < 1)
    return fail(SIREN_EINVAL, "%s: bad size (rows_per_batch=%lld)", what, (long long)rows_per_batch);
  if (rows > 0 && (!pred || !jac || !src || !slow || !mask)) return fail(SIREN_EINVAL, "%s: null pointer", what);
  return SIREN_OK;
}

// the reference's constants (loss_functions.py:380-382): sums, the first two times N / 10 and N / 100
// with N the rows of one batch element
WaveArgs wave_args(const float* pred, const float* jac, const float* hess, const float* src, const float* slow,
                   const unsigned char* mask, int64_t rows, int64_t rows_per_batch) {
  WaveArgs a;
  memset(&a, 0, sizeof(a));
  a.pred = pred;
  a.jac = jac;
  a.hess = hess;
  a.src = src;
  a.slow = slow;
  a.mask = mask;
  a.rows = rows;
  a.w[0] = (float)((double)rows_per_batch / 1e1);
  a.w[1] = (float)((double)rows_per_batch / 1e2);
  a.w[2] = 1.f;
  return a;
}

// the Helmholtz loss kernels
const Kernel<HelmArgs> kHelmFwd = SIREN_K(helmholtz_fwd_kernel);
const Kernel<HelmArgs> kHelmBwd = SIREN_K(helmholtz_bwd_kernel);

// the argument checks both entry points share; 0 or SIREN_EINVAL (message set)
int helm_check(const char* what, const float* x, const float* pred, const float* jac, const float* hess,
               const float* src, const float* slow, const float* k, int64_t rows, int64_t rows_per_batch) {
  if (rows < 0) return fail(SIREN_EINVAL, "%s: bad size (rows=%lld)", what, (long long)rows);
  if (rows > 0 && rows_per_batch < 1)
    return fail(SIREN_EINVAL, "%s: bad size (rows_per_batch=%lld)", what, (long long)rows_per_batch);
  if (rows > 0 && (!x || !pred || !jac || !hess || !src || !slow || !k)) return fail(SIREN_EINVAL, "%s: null pointer", what);
  return SIREN_OK;
}

// the reference's constants (loss_functions.py:455-456): sums, the first times N / 1e3 with N the rows of
// one batch element
HelmArgs helm_args(const float* x, const float* pred, const float* jac, const float* hess, const float* src,
                   const float* slow, const float* k, int64_t rows, int64_t rows_per_batch) {
  HelmArgs a;
  memset(&a, 0, sizeof(a));
  a.x = x;
  a.pred = pred;
  a.jac = jac;
  a.hess = hess;
  a.src = src;
  a.slow = slow;
  a.k = k;
  a.rows = rows;
  a.w[0] = (float)((double)rows_per_batch / 1e3);
  a.w[1] = 1.f;
  return a;
}

// the forms of a transform kernel, by log2 side - 3 (side checked by kfft_log2); one workgroup of
// KfGeom<log2 side>::T threads per slice
#define SIREN_SIDES(K) {SIREN_K(K<3>), SIREN_K(K<4>), SIREN_K(K<5>), SIREN_K(K<6>), SIREN_K(K<7>)}
const Kernel<KfftArgs> kKfft2[5] = SIREN_SIDES(kfft2_kernel);
const Kernel<KiftArgs> kKiftFwd[5] = SIREN_SIDES(kift_fwd_kernel);
const Kernel<KiftArgs> kKiftBwd[5] = SIREN_SIDES(kift_bwd_kernel);
template <class Args>
int launch_slices(const Kernel<Args> (&k)[5], int lg, int64_t slices, const char* what, void* stream, const Args& a) {
  return launch_kernel(k[lg - 3], dim3((unsigned)slices), std::min(1u << (2 * lg), 1024u), 0, what, (hipStream_t)stream, a);
}

// log2 of a supported side (8, 16, 32, 64, 128), or -1
int kfft_log2(int side) {
  for (int lg = 3; lg <= 7; ++lg)
    if (side == (1 << lg)) return lg;
  return -1;
}

// the argument checks the two loss entry points share; 0 or SIREN_EINVAL (message set)
int kift_check(const char* what, const siren_kift_desc* desc, const float* pred, const float* k0, const float* mask,
               const float* tgt, const float* img_mask, int64_t img_mask_bstride, int64_t batch, int side) {
  if (kfft_log2(side) < 0) return fail(SIREN_EINVAL, "%s: side %d is not one of 8, 16, 32, 64, 128", what, side);
  if (!desc) return fail(SIREN_EINVAL, "%s: null descriptor", what);
  if (!pred || !tgt) return fail(SIREN_EINVAL, "%s: null pointer", what);
  if ((!k0) != (!mask)) return fail(SIREN_EINVAL, "%s: k0 and mask go together (data consistency)", what);
  if (batch < 1 || batch > LOSS_SLOTS)
    return fail(SIREN_EINVAL, "%s: batch %lld outside [1, %d] (one workspace slot per slice)", what, (long long)batch,
                LOSS_SLOTS);
  if (img_mask && img_mask_bstride != 0 && img_mask_bstride != (int64_t)side * side)
    return fail(SIREN_EINVAL, "%s: img_mask batch stride %lld is neither 0 nor side^2", what,
                (long long)img_mask_bstride);
  return SIREN_OK;
}

KiftArgs kift_args(const siren_kift_desc* d, const float* pred, const float* k0, const float* mask, const float* tgt,
                   const float* img_mask, int64_t img_mask_bstride, float noise) {
  KiftArgs a;
  memset(&a, 0, sizeof(a));
  a.pred = pred;
  a.k0 = k0;
  a.mask = mask;
  a.tgt = tgt;
  a.img_mask = img_mask;
  a.img_mask_bstride = img_mask ? img_mask_bstride : 0;
  a.noise = noise;
  a.img_weight = d->img_weight;
  a.l1_weight = d->l1_weight;
  a.kspace_weight = d->kspace_weight;
  return a;
}
}  // namespace

extern "C" {

int64_t siren_sse_workspace_bytes(void) { return (int64_t)LOSS_SLOTS * 4 + 256; }

int siren_sse_forward(const float* pred, const float* tgt, const float* mask, int64_t n, int64_t mask_n,
                      float weight, float* d, float* loss, void* workspace, int64_t ws_bytes, void* stream) {
  if (n < 0 || !loss || (n > 0 && (!pred || !tgt || !d)) || (mask && mask_n <= 0))
    return fail(SIREN_EINVAL, "sse_forward: bad arguments (n=%lld, mask_n=%lld)", (long long)n, (long long)mask_n);
  SseFwdArgs a;
  if (int rc = loss_slots("sse_forward", workspace, ws_bytes, &a.partial, &a.counter)) return rc;
  a.pred = pred;
  a.tgt = tgt;
  a.mask = mask;
  a.d = d;
  a.loss = loss;
  a.n = n;
  a.mask_n = mask ? mask_n : 1;
  a.weight = weight;
  // 16 elements per thread: few enough blocks that the hand-off counter (one agent-scope add per
  // block, all on one address) stays off the critical path (262144 elements: 64 blocks)
  const unsigned blocks = (unsigned)std::max<int64_t>(1, std::min<int64_t>(LOSS_SLOTS, cdiv(n, 16 * SSE_THREADS)));
  hipLaunchKernelGGL(sse_fwd_kernel, dim3(blocks), dim3(SSE_THREADS), 0, (hipStream_t)stream, a);
  return check_launch("sse_forward");
}

int siren_sse_backward(const float* d, const float* mask, int64_t n, int64_t mask_n, const float* g, float scale,
                       float* out, void* stream) {
  if (n < 0 || (n > 0 && (!d || !g || !out)) || (mask && mask_n <= 0))
    return fail(SIREN_EINVAL, "sse_backward: bad arguments (n=%lld, mask_n=%lld)", (long long)n, (long long)mask_n);
  if (n == 0) return SIREN_OK;
  SseBwdArgs a;
  a.d = d;
  a.mask = mask;
  a.g = g;
  a.out = out;
  a.n = n;
  a.mask_n = mask ? mask_n : 1;
  a.scale = scale;
  const unsigned blocks = (unsigned)std::max<int64_t>(1, std::min<int64_t>(4096, cdiv(n, 4 * SSE_THREADS)));
  hipLaunchKernelGGL(sse_bwd_kernel, dim3(blocks), dim3(SSE_THREADS), 0, (hipStream_t)stream, a);
  return check_launch("sse_backward");
}

int siren_dc_forward(const float* pred, const float* k0, const float* mask, int64_t batch, int64_t npix,
                     int channels, float noise, float* out, void* stream) {
  if (batch < 0 || npix < 0 || channels < 1 || channels > KSPACE_MAXC || (batch * npix > 0 && (!pred || !k0 || !mask || !out)))
    return fail(SIREN_EINVAL, "dc_forward: bad arguments (batch=%lld, npix=%lld, channels=%d)", (long long)batch,
                (long long)npix, channels);
  if (batch * npix == 0) return SIREN_OK;
  DcArgs a{pred, k0, mask, out, batch, npix, channels, noise, 0};
  const unsigned blocks = (unsigned)std::max<int64_t>(1, std::min<int64_t>(4096, cdiv(batch * npix, KS_THREADS)));
  hipLaunchKernelGGL(dc_kernel, dim3(blocks), dim3(KS_THREADS), 0, (hipStream_t)stream, a);
  return check_launch("dc_forward");
}

int siren_dc_backward(const float* g, const float* mask, int64_t batch, int64_t npix, int channels, float noise,
                      float* dpred, void* stream) {
  if (batch < 0 || npix < 0 || channels < 1 || channels > KSPACE_MAXC || (batch * npix > 0 && (!g || !mask || !dpred)))
    return fail(SIREN_EINVAL, "dc_backward: bad arguments");
  if (batch * npix == 0) return SIREN_OK;
  DcArgs a{g, nullptr, mask, dpred, batch, npix, channels, noise, 1};
  const unsigned blocks = (unsigned)std::max<int64_t>(1, std::min<int64_t>(4096, cdiv(batch * npix, KS_THREADS)));
  hipLaunchKernelGGL(dc_kernel, dim3(blocks), dim3(KS_THREADS), 0, (hipStream_t)stream, a);
  return check_launch("dc_backward");
}

int siren_kspace_sse_forward(const float* pred, const float* k0, const float* mask, const float* tgt,
                             const float* hf, int64_t batch, int64_t npix, int channels, float noise, float weight,
                             float* d, float* loss, void* workspace, int64_t ws_bytes, void* stream) {
  if (batch < 0 || npix < 0 || channels < 1 || channels > KSPACE_MAXC || !loss || (!k0) != (!mask) ||
      (batch * npix > 0 && (!pred || !tgt || !d)))
    return fail(SIREN_EINVAL, "kspace_sse_forward: bad arguments (batch=%lld, npix=%lld, channels=%d)",
                (long long)batch, (long long)npix, channels);
  KsseFwdArgs a{pred, k0, mask, tgt, hf, d, loss, nullptr, nullptr, batch, npix, channels, noise, weight};
  if (int rc = loss_slots("kspace_sse_forward", workspace, ws_bytes, &a.partial, &a.counter)) return rc;
  // 8 coordinates per thread: few blocks for the hand-off counter (32 x 16384 coordinates: 256)
  const unsigned blocks =
      (unsigned)std::max<int64_t>(1, std::min<int64_t>(LOSS_SLOTS, cdiv(batch * npix, 8 * KS_THREADS)));
  hipLaunchKernelGGL(ksse_fwd_kernel, dim3(blocks), dim3(KS_THREADS), 0, (hipStream_t)stream, a);
  return check_launch("kspace_sse_forward");
}

int siren_kspace_sse_backward(const float* d, const float* mask, const float* hf, int64_t batch, int64_t npix,
                              int channels, float noise, const float* g, float scale, float* dpred, void* stream) {
  if (batch < 0 || npix < 0 || channels < 1 || channels > KSPACE_MAXC || (batch * npix > 0 && (!d || !g || !dpred)))
    return fail(SIREN_EINVAL, "kspace_sse_backward: bad arguments");
  if (batch * npix == 0) return SIREN_OK;
  KsseBwdArgs a{d, mask, hf, g, dpred, batch, npix, channels, noise, scale};
  const unsigned blocks = (unsigned)std::max<int64_t>(1, std::min<int64_t>(4096, cdiv(batch * npix, KS_THREADS)));
  hipLaunchKernelGGL(ksse_bwd_kernel, dim3(blocks), dim3(KS_THREADS), 0, (hipStream_t)stream, a);
  return check_launch("kspace_sse_backward");
}

int siren_kspace_loss_forward(int kind, const siren_kloss_desc* desc, const float* pred, const float* k0,
                              const float* mask, const float* tgt, int64_t batch, int64_t npix, int channels,
                              float noise, float* loss, void* workspace, int64_t ws_bytes, void* stream) {
  if (int rc = kloss_check("kspace_loss_forward", kind, desc, k0, mask, batch, npix, channels)) return rc;
  if (!loss || (batch * npix > 0 && (!pred || !tgt))) return fail(SIREN_EINVAL, "kspace_loss_forward: null pointer");
  KlossArgs a = kloss_args(desc, pred, k0, mask, tgt, batch, npix, channels, noise);
  if (int rc = loss_slots("kspace_loss_forward", workspace, ws_bytes, &a.partial, &a.counter)) return rc;
  a.out = loss;
  // 8 coordinates per thread, as kspace_sse_forward: few blocks for the hand-off counter
  const unsigned blocks =
      (unsigned)std::max<int64_t>(1, std::min<int64_t>(LOSS_SLOTS, cdiv(batch * npix, 8 * KL_THREADS)));
  return launch_kernel(kKlossFwd[kind], dim3(blocks), KL_THREADS, 0, "kspace_loss_forward", (hipStream_t)stream, a);
}

int siren_kspace_loss_backward(int kind, const siren_kloss_desc* desc, const float* pred, const float* k0,
                               const float* mask, const float* tgt, int64_t batch, int64_t npix, int channels,
                               float noise, const float* g, float* dpred, void* stream) {
  if (int rc = kloss_check("kspace_loss_backward", kind, desc, k0, mask, batch, npix, channels)) return rc;
  if (batch * npix > 0 && (!pred || !tgt || !g || !dpred))
    return fail(SIREN_EINVAL, "kspace_loss_backward: null pointer");
  if (batch * npix == 0) return SIREN_OK;
  KlossArgs a = kloss_args(desc, pred, k0, mask, tgt, batch, npix, channels, noise);
  a.g = g;
  a.out = dpred;
  const unsigned blocks = (unsigned)std::max<int64_t>(1, std::min<int64_t>(4096, cdiv(batch * npix, KL_THREADS)));
  return launch_kernel(kKlossBwd[kind], dim3(blocks), KL_THREADS, 0, "kspace_loss_backward", (hipStream_t)stream, a);
}

int siren_sdf_loss_forward(const float* pred, const float* grad, const float* sdf, const float* nrm, int64_t rows,
                           int dims, float* out4, void* workspace, int64_t ws_bytes, void* stream) {
  if (int rc = sdf_check("sdf_loss_forward", pred, grad, sdf, nrm, rows, dims)) return rc;
  if (!out4) return fail(SIREN_EINVAL, "sdf_loss_forward: null pointer");
  SdfArgs a = sdf_args(pred, grad, sdf, nrm, rows);
  if (int rc = loss_slots("sdf_loss_forward", workspace, ws_bytes, &a.partial, &a.counter)) return rc;
  a.out = out4;
  // one row per thread per iteration; four slots per workgroup, so at most LOSS_SLOTS / 4 = 256 of them
  // (rows == 0: one workgroup writes the four zeros)
  const unsigned blocks = (unsigned)std::max<int64_t>(1, std::min<int64_t>(SDF_MAX_BLOCKS, cdiv(rows, SDF_THREADS)));
  return launch_kernel(kSdfFwd[dims - 2], dim3(blocks), SDF_THREADS, 0, "sdf_loss_forward", (hipStream_t)stream, a);
}

int siren_sdf_loss_backward(const float* pred, const float* grad, const float* sdf, const float* nrm, int64_t rows,
                            int dims, const float* g4, float* dpred, float* dgrad, void* stream) {
  if (int rc = sdf_check("sdf_loss_backward", pred, grad, sdf, nrm, rows, dims)) return rc;
  if (rows > 0 && (!g4 || !dpred || !dgrad)) return fail(SIREN_EINVAL, "sdf_loss_backward: null pointer");
  if (rows == 0) return SIREN_OK;
  SdfArgs a = sdf_args(pred, grad, sdf, nrm, rows);
  a.g = g4;
  a.dpred = dpred;
  a.dgrad = dgrad;
  const unsigned blocks = (unsigned)std::max<int64_t>(1, std::min<int64_t>(4096, cdiv(rows, SDF_THREADS)));
  return launch_kernel(kSdfBwd[dims - 2], dim3(blocks), SDF_THREADS, 0, "sdf_loss_backward", (hipStream_t)stream, a);
}

int siren_wave_loss_forward(const float* pred, const float* jac, const float* hess, const float* src,
                            const float* slow, const unsigned char* mask, int64_t rows, int64_t rows_per_batch,
                            float* out3, void* workspace, int64_t ws_bytes, void* stream) {
  if (int rc = wave_check("wave_loss_forward", pred, jac, src, slow, mask, rows, rows_per_batch)) return rc;
  if (!out3) return fail(SIREN_EINVAL, "wave_loss_forward: null pointer");
  WaveArgs a = wave_args(pred, jac, hess, src, slow, mask, rows, rows_per_batch);
  if (int rc = loss_slots("wave_loss_forward", workspace, ws_bytes, &a.partial, &a.counter)) return rc;
  a.out = out3;
  // one row per thread per iteration; three slots per workgroup, at most WAVE_MAX_BLOCKS = 256 of them
  // (rows == 0: one workgroup writes the three zeros)
  const unsigned blocks = (unsigned)std::max<int64_t>(1, std::min<int64_t>(WAVE_MAX_BLOCKS, cdiv(rows, WAVE_THREADS)));
  return launch_kernel(kWaveFwd[hess ? 1 : 0], dim3(blocks), WAVE_THREADS, 0, "wave_loss_forward", (hipStream_t)stream, a);
}

int siren_wave_loss_backward(const float* pred, const float* jac, const float* hess, const float* src,
                             const float* slow, const unsigned char* mask, int64_t rows, int64_t rows_per_batch,
                             const float* g3, float* dpred, float* djac, float* dhess, void* stream) {
  if (int rc = wave_check("wave_loss_backward", pred, jac, src, slow, mask, rows, rows_per_batch)) return rc;
  if ((!hess) != (!dhess)) return fail(SIREN_EINVAL, "wave_loss_backward: hess and dhess go together");
  if (rows > 0 && (!g3 || !dpred || !djac)) return fail(SIREN_EINVAL, "wave_loss_backward: null pointer");
  if (rows == 0) return SIREN_OK;
  WaveArgs a = wave_args(pred, jac, hess, src, slow, mask, rows, rows_per_batch);
  a.g = g3;
  a.dpred = dpred;
  a.djac = djac;
  a.dhess = dhess;
  const unsigned blocks = (unsigned)std::max<int64_t>(1, std::min<int64_t>(4096, cdiv(rows, WAVE_THREADS)));
  return launch_kernel(kWaveBwd[hess ? 1 : 0], dim3(blocks), WAVE_THREADS, 0, "wave_loss_backward", (hipStream_t)stream, a);
}

int siren_helmholtz_loss_forward(const float* x, const float* pred, const float* jac, const float* hess,
                                 const float* src, const float* slow, const float* k, int64_t rows,
                                 int64_t rows_per_batch, float* out3, void* workspace, int64_t ws_bytes, void* stream) {
  if (int rc = helm_check("helmholtz_loss_forward", x, pred, jac, hess, src, slow, k, rows, rows_per_batch)) return rc;
  if (!out3) return fail(SIREN_EINVAL, "helmholtz_loss_forward: null pointer");
  HelmArgs a = helm_args(x, pred, jac, hess, src, slow, k, rows, rows_per_batch);
  if (int rc = loss_slots("helmholtz_loss_forward", workspace, ws_bytes, &a.partial, &a.counter)) return rc;
  if (rows == 0) {  // three zeros, no launch
    if (hipMemsetAsync(out3, 0, 3 * sizeof(float), (hipStream_t)stream) != hipSuccess)
      return fail(SIREN_ELAUNCH, "helmholtz_loss_forward: %s", hipGetErrorString(hipGetLastError()));
    return SIREN_OK;
  }
  a.out = out3;
  // one row per thread per iteration; two slots per workgroup, at most HELM_MAX_BLOCKS = 256 of them
  const unsigned blocks = (unsigned)std::min<int64_t>(HELM_MAX_BLOCKS, cdiv(rows, HELM_THREADS));
  return launch_kernel(kHelmFwd, dim3(blocks), HELM_THREADS, 0, "helmholtz_loss_forward", (hipStream_t)stream, a);
}

int siren_helmholtz_loss_backward(const float* x, const float* pred, const float* jac, const float* hess,
                                  const float* src, const float* slow, const float* k, int64_t rows,
                                  int64_t rows_per_batch, const float* g3, float* dpred, float* djac, float* dhess,
                                  void* stream) {
  if (int rc = helm_check("helmholtz_loss_backward", x, pred, jac, hess, src, slow, k, rows, rows_per_batch)) return rc;
  if (rows > 0 && (!g3 || !dpred || !djac || !dhess)) return fail(SIREN_EINVAL, "helmholtz_loss_backward: null pointer");
  if (rows == 0) return SIREN_OK;
  HelmArgs a = helm_args(x, pred, jac, hess, src, slow, k, rows, rows_per_batch);
  a.g = g3;
  a.dpred = dpred;
  a.djac = djac;
  a.dhess = dhess;
  const unsigned blocks = (unsigned)std::min<int64_t>(4096, cdiv(rows, HELM_THREADS));
  return launch_kernel(kHelmBwd, dim3(blocks), HELM_THREADS, 0, "helmholtz_loss_backward", (hipStream_t)stream, a);
}

int siren_kspace_fft2(const float* x, float* out, int64_t batch, int side, int inverse, void* stream) {
  const int lg = kfft_log2(side);
  if (lg < 0) return fail(SIREN_EINVAL, "kspace_fft2: side %d is not one of 8, 16, 32, 64, 128", side);
  if (batch < 0 || batch > 0x7fffffff)
    return fail(SIREN_EINVAL, "kspace_fft2: bad batch %lld", (long long)batch);
  if (batch > 0 && (!x || !out)) return fail(SIREN_EINVAL, "kspace_fft2: null pointer");
  if (batch == 0) return SIREN_OK;
  KfftArgs a{x, out, inverse ? 1 : 0};
  return launch_slices(kKfft2, lg, batch, "kspace_fft2", stream, a);
}

int siren_kspace_ift_loss_forward(const siren_kift_desc* desc, const float* pred, const float* k0, const float* mask,
                                  const float* tgt, const float* img_mask, int64_t img_mask_batch_stride,
                                  int64_t batch, int side, float noise, float* loss, void* workspace,
                                  int64_t ws_bytes, void* stream) {
  if (int rc = kift_check("kspace_ift_loss_forward", desc, pred, k0, mask, tgt, img_mask, img_mask_batch_stride, batch,
                          side))
    return rc;
  if (!loss) return fail(SIREN_EINVAL, "kspace_ift_loss_forward: null pointer");
  KiftArgs a = kift_args(desc, pred, k0, mask, tgt, img_mask, img_mask_batch_stride, noise);
  if (int rc = loss_slots("kspace_ift_loss_forward", workspace, ws_bytes, &a.partial, &a.counter)) return rc;
  a.out = loss;
  return launch_slices(kKiftFwd, kfft_log2(side), batch, "kspace_ift_loss_forward", stream, a);
}

int siren_kspace_ift_loss_backward(const siren_kift_desc* desc, const float* pred, const float* k0, const float* mask,
                                   const float* tgt, const float* img_mask, int64_t img_mask_batch_stride,
                                   int64_t batch, int side, float noise, const float* g, float* dpred,
                                   void* stream) {
  if (int rc = kift_check("kspace_ift_loss_backward", desc, pred, k0, mask, tgt, img_mask, img_mask_batch_stride,
                          batch, side))
    return rc;
  if (!g || !dpred) return fail(SIREN_EINVAL, "kspace_ift_loss_backward: null pointer");
  KiftArgs a = kift_args(desc, pred, k0, mask, tgt, img_mask, img_mask_batch_stride, noise);
  a.g = g;
  a.out = dpred;
  return launch_slices(kKiftBwd, kfft_log2(side), batch, "kspace_ift_loss_backward", stream, a);
}

int siren_fourier_features(const float* x, const float* B, int64_t rows, int cin, int m, float* out, void* stream) {
  if (rows < 0 || cin < 1 || m < 1 || (rows > 0 && (!x || !B || !out)))
    return fail(SIREN_EINVAL, "fourier_features: bad arguments (rows=%lld, cin=%d, m=%d)", (long long)rows, cin, m);
  if (rows == 0) return SIREN_OK;
  FourierArgs a{x, B, out, rows, cin, m};
  const unsigned blocks = (unsigned)std::max<int64_t>(1, std::min<int64_t>(4096, cdiv(rows * m, KS_THREADS)));
  hipLaunchKernelGGL(fourier_kernel, dim3(blocks), dim3(KS_THREADS), 0, (hipStream_t)stream, a);
  return check_launch("fourier_features");
}

int siren_sincos_f32(const float* x, float* s, float* c, int64_t n, int impl, void* stream) {
  if (n < 0 || (impl != 0 && impl != 1) || (n > 0 && (!x || !s || !c)))
    return fail(SIREN_EINVAL, "sincos_f32: bad arguments (n=%lld, impl=%d)", (long long)n, impl);
  if (n == 0) return SIREN_OK;
  hipLaunchKernelGGL(sincos_probe_kernel, dim3(grid1d(n, 4096)), dim3(256), 0, (hipStream_t)stream, x, s, c, n, impl);
  return check_launch("sincos_f32");
}

}  // extern "C"
