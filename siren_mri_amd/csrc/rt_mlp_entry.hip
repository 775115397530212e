// rt_mlp_entry.hip — the entry points of the SIREN layer stack (siren_mlp_*) over rt_mlp.hip's layout and
// launch plan, with the fused image loss. Included by siren_runtime.hip.
namespace {

// Which forward carries a fused image loss: the bf16 register-resident forward (its output-layer
// epilogue, fused_fwd_reg_kernel<.., LOSS>) or the per-layer path's output kernel (last_fwd_kernel
// <.., LOSS>: fp32 mode, and bf16 shapes that are not the fused forward's); 0 = none applies.
int loss_path(const siren_mlp_desc* d) {
  const int O = d->dims[d->num_layers];
  if (!d->outermost_linear) return 0;
  const bool fused = d->prec == SIREN_PREC_BF16 && g_fused_forward && fused_shape(d);
  if (fused)
    return (g_fwd_reg && d->num_layers >= 3 && !g_freg_magic && (fused_wide(d) || O == 1)) ? 1 : 0;
  if (d->ff_B) return 0;  // (a Fourier-feature input is a register-forward form)
  return O <= 8 ? 2 : 0;
}

int loss_path_fail(const siren_mlp_desc* d) {
  if (!d->outermost_linear) return fail(SIREN_EINVAL, "fused loss: needs outermost_linear");
  if (g_freg_magic) return fail(SIREN_EINVAL, "fused loss: not with option freg_magic");
  return fail(SIREN_EINVAL, "fused loss: shape not supported (bf16 fused shapes: the register forward's "
                            "forms with 3+ layers and 1 output for 1..4 inputs; per-layer path: <= 8 outputs)");
}

// What siren_mlp_forward and siren_mlp_forward_loss check after the descriptor.
int forward_args_check(const Layout& lo, const float* x, const float* y, const void* saved, int64_t saved_bytes,
                       const void* workspace, int64_t workspace_bytes) {
  int rc = check_buffers(saved, saved_bytes, lo.saved_bytes, false, workspace, workspace_bytes, lo.ws_bytes);
  if (rc) return rc;
  if (!x || !y) return fail(SIREN_EINVAL, "null x or y");
  return SIREN_OK;
}
}  // namespace

extern "C" {

int siren_mlp_check(const siren_mlp_desc* d) {
  if (!d) return fail(SIREN_EINVAL, "null descriptor");
  const int L = d->num_layers;
  if (L < 2 || L > SIREN_MAX_LAYERS)
    return fail(SIREN_EINVAL, "num_layers=%d outside [2, %d]", L, SIREN_MAX_LAYERS);
  if (d->prec != SIREN_PREC_F32 && d->prec != SIREN_PREC_BF16)
    return fail(SIREN_EINVAL, "unknown precision %d", d->prec);
  if (d->batch < 1 || d->rows_per_batch < 1)
    return fail(SIREN_EINVAL, "empty input (batch=%lld rows=%lld)", (long long)d->batch,
                (long long)d->rows_per_batch);
  if (d->batch > 65535) return fail(SIREN_EINVAL, "batch %lld > 65535", (long long)d->batch);
  const int kmax = 512;  // MFMA K bound of the GEMM kernels (fp32: two register chunks of 256)
  if (d->dims[0] < 1 || (wide_input(d) && first_kp(d) > kmax))
    return fail(SIREN_EINVAL, "in_features=%d unsupported (1..%d)", d->dims[0], kmax);
  if (d->dims[L] < 1 || d->dims[L] > 8)
    return fail(SIREN_EINVAL, "out_features=%d unsupported (1..8)", d->dims[L]);
  const int hmax = 512;
  for (int l = 1; l < L; ++l)
    if (d->dims[l] < 32 || d->dims[l] % 32 != 0 || d->dims[l] > hmax)
      return fail(SIREN_EINVAL, "hidden width dims[%d]=%d must be a multiple of 32 in [32, %d]",
                  l, d->dims[l], hmax);
  if (d->dims[0] > 4 && d->dims[1] > 512)
    return fail(SIREN_EINVAL, "in_features > 4 needs first hidden width <= 512");
  if ((int64_t)d->batch * d->rows_per_batch * (d->dims[1] / 8) >= (int64_t)1 << 31)
    return fail(SIREN_EINVAL, "too many rows for one call");
  for (int l = 0; l < L; ++l)
    if (!d->weight[l] || !d->bias[l]) return fail(SIREN_EINVAL, "layer %d: null weight/bias", l);
  for (int l = 1; l + 1 < L; ++l)
    if (!aligned16(d->weight[l])) return fail(SIREN_EINVAL, "layer %d weight not 16-B aligned", l);
  if (d->ff_B) {
    if (d->ff_in < 1 || d->ff_in > 4 || d->dims[0] % 2 || d->ff_in * (d->dims[0] / 2) > 32)
      return fail(SIREN_EINVAL, "fourier input: ff_in=%d raw coordinates (1..4) for %d features (even)", d->ff_in,
                  d->dims[0]);
    if (d->prec != SIREN_PREC_BF16 || !g_fused_forward || !g_fwd_reg || !fused_shape(d) || !fused_wide(d) || L < 3 ||
        d->dims[1] != 256)
      return fail(SIREN_EINVAL, "fourier input: needs the bf16 register-resident forward's wide first layer "
                                "(6..16 features, hidden 256)");
  }
  return SIREN_OK;
}

int64_t siren_mlp_saved_bytes(const siren_mlp_desc* d) {
  if (siren_mlp_check(d)) return -1;
  return layout_of(d).saved_bytes;
}

int64_t siren_mlp_workspace_bytes(const siren_mlp_desc* d) {
  if (siren_mlp_check(d)) return -1;
  return layout_of(d).ws_bytes;
}

int siren_mlp_forward(const siren_mlp_desc* d, const float* x, float* y, void* saved,
                      int64_t saved_bytes, void* workspace, int64_t workspace_bytes, void* stream) {
  int rc = siren_mlp_check(d);
  if (rc) return rc;
  const Layout lo = layout_of(d);
  if ((rc = forward_args_check(lo, x, y, saved, saved_bytes, workspace, workspace_bytes))) return rc;
  hipStream_t st = (hipStream_t)stream;
  g_err.clear();
  if (d->prec == SIREN_PREC_BF16)
    return forward_impl<kPrecBF16>(d, x, y, (char*)saved, (char*)workspace, st);
  return forward_impl<kPrecF32>(d, x, y, (char*)saved, (char*)workspace, st);
}

int siren_mlp_backward(const siren_mlp_desc* d, const float* x, const float* dy, const void* saved,
                       int64_t saved_bytes, void* workspace, int64_t workspace_bytes,
                       float* const* dweight, float* const* dbias, float* dx, void* stream) {
  return siren_mlp_backward_ex(d, x, dy, nullptr, saved, saved_bytes, workspace, workspace_bytes, dweight, dbias, dx,
                               stream);
}

int siren_mlp_loss_check(const siren_mlp_desc* d, const siren_loss_desc* l) {
  int rc = siren_mlp_check(d);
  if (rc) return rc;
  if (!l) return fail(SIREN_EINVAL, "null loss descriptor");
  const int path = loss_path(d);
  if (!path) return loss_path_fail(d);
  if (!l->target || !l->dy || !l->loss || !l->loss_workspace)
    return fail(SIREN_EINVAL, "fused loss: null target / dy / loss / workspace");
  if (l->loss_workspace_bytes < siren_sse_workspace_bytes())
    return fail(SIREN_ENOSPACE, "fused loss: workspace %lld < %lld bytes", (long long)l->loss_workspace_bytes,
                (long long)siren_sse_workspace_bytes());
  if ((l->k0 == nullptr) != (l->mask == nullptr) || (l->k0 == nullptr) != (l->y_dc == nullptr))
    return fail(SIREN_EINVAL, "fused loss: k0, mask and y_dc are given together or not at all");
  if (l->hf && l->hf_len != d->rows_per_batch)
    return fail(SIREN_EINVAL, "fused loss: hf has %lld entries for %lld rows per weight set", (long long)l->hf_len,
                (long long)d->rows_per_batch);
  const Geo g = geo_of(d);
  const int64_t wgs = path == 1 ? std::min<int64_t>(cdiv(g.rows, FREG_WG_ROWS), std::max<int64_t>(1, 256 / g.nb)) * g.nb
                                : g.nb;  // (per-layer path: at most LOSS_SLOTS / nb workgroups per weight set)
  if (wgs > LOSS_SLOTS) return fail(SIREN_EINVAL, "fused loss: %lld workgroups > %d", (long long)wgs, LOSS_SLOTS);
  return SIREN_OK;
}

int siren_mlp_forward_loss(const siren_mlp_desc* d, const siren_loss_desc* l, const float* x, float* y, void* saved,
                           int64_t saved_bytes, void* workspace, int64_t workspace_bytes, void* stream) {
  int rc = siren_mlp_loss_check(d, l);
  if (rc) return rc;
  const Layout lo = layout_of(d);
  if ((rc = forward_args_check(lo, x, y, saved, saved_bytes, workspace, workspace_bytes))) return rc;
  g_err.clear();
  const Geo g = geo_of(d);
  if (loss_path(d) == 1) {
    char* wbuf = saved ? (char*)saved : (char*)workspace;
    return fused_forward_reg(d, g, lo, x, y, (char*)saved, wbuf, (hipStream_t)stream, l);
  }
  if (d->prec == SIREN_PREC_BF16)
    return forward_impl<kPrecBF16>(d, x, y, (char*)saved, (char*)workspace, (hipStream_t)stream, l);
  return forward_impl<kPrecF32>(d, x, y, (char*)saved, (char*)workspace, (hipStream_t)stream, l);
}

int siren_mlp_backward_ex(const siren_mlp_desc* d, const float* x, const float* dy, const float* dy_scale,
                          const void* saved, int64_t saved_bytes, void* workspace, int64_t workspace_bytes,
                          float* const* dweight, float* const* dbias, float* dx, void* stream) {
  int rc = siren_mlp_check(d);
  if (rc) return rc;
  const Layout lo = layout_of(d);
  if ((rc = check_buffers(saved, saved_bytes, lo.saved_bytes, true, workspace, workspace_bytes, lo.ws_bytes))) return rc;
  if (!x || !dy || !dweight || !dbias) return fail(SIREN_EINVAL, "null argument");
  for (int l = 0; l < d->num_layers; ++l)
    if (!dweight[l] || !dbias[l]) return fail(SIREN_EINVAL, "layer %d: null gradient output", l);
  if (d->ff_B && dx) return fail(SIREN_EINVAL, "fourier input: no input gradient (dx must be NULL)");
  g_err.clear();
  return backward_impl(d, x, dy, (const char*)saved, (char*)workspace, dweight, dbias, dx, (hipStream_t)stream, dy_scale);
}

int64_t siren_mlp_backward_plan(const siren_mlp_desc* d, int flags, char* out, int64_t cap) {
  if (siren_mlp_check(d)) return -1;
  if (d->ff_B && (flags & 1)) return fail(SIREN_EINVAL, "fourier input: no input gradient (dx must be NULL)"), -1;
  const BwdPlan p = plan_backward(d, geo_of(d), layout_of(d), flags & 1, flags & 2, flags & 4);
  if (p.error) return fail(SIREN_EINVAL, "%s", p.error), -1;
  return text_out(plan_text(p), out, cap);
}

}  // extern "C"
