// rt_adam.hip — the multi-tensor Adam step (siren_adam_*, kernels in siren_adam.hip). Included by
// siren_runtime.hip.
extern "C" {

int siren_adam_scalars_table(double* t, const float* table, int64_t n, float* out, void* stream) {
  if (!t || !table || n < 1 || !out) return fail(SIREN_EINVAL, "adam_scalars_table: null pointer or empty table");
  hipLaunchKernelGGL(adam_scalars_table_kernel, dim3(1), dim3(1), 0, (hipStream_t)stream, t, table, n, out);
  return check_launch("adam_scalars_table");
}

int siren_adam_scalars(double* t, double lr, double beta1, double beta2, float* out, void* stream) {
  if (!t || !out) return fail(SIREN_EINVAL, "adam_scalars: null pointer");
  hipLaunchKernelGGL(adam_scalars_kernel, dim3(1), dim3(1), 0, (hipStream_t)stream, t, lr, beta1, beta2, out);
  return check_launch("adam_scalars");
}

int64_t siren_adam_num_blocks(const siren_adam_desc* d) {
  if (!d || d->num_tensors <= 0 || d->num_tensors > SIREN_ADAM_MAX_TENSORS) return 0;
  int64_t maxn = 0;
  for (int t = 0; t < d->num_tensors; ++t) maxn = std::max(maxn, d->numel[t]);
  return maxn > 0 ? (int64_t)grid1d(maxn, 1024) * d->num_tensors : 0;
}

int siren_adam_step(const siren_adam_desc* d, void* stream) {
  if (!d || d->num_tensors < 0 || d->num_tensors > SIREN_ADAM_MAX_TENSORS)
    return fail(SIREN_EINVAL, "adam: num_tensors outside [0, %d]", SIREN_ADAM_MAX_TENSORS);
  if (d->num_tensors == 0) return SIREN_OK;
  AdamArgs a;
  memset(&a, 0, sizeof(a));
  int64_t maxn = 0;
  for (int t = 0; t < d->num_tensors; ++t) {
    if (!d->param[t] || !d->grad[t] || !d->exp_avg[t] || !d->exp_avg_sq[t] || d->numel[t] < 0)
      return fail(SIREN_EINVAL, "adam: tensor %d has a null pointer or negative size", t);
    a.param[t] = d->param[t];
    a.grad[t] = d->grad[t];
    a.exp_avg[t] = d->exp_avg[t];
    a.exp_avg_sq[t] = d->exp_avg_sq[t];
    a.numel[t] = d->numel[t];
    maxn = std::max(maxn, d->numel[t]);
  }
  a.one_minus_beta1 = d->one_minus_beta1;
  a.beta2 = d->beta2;
  a.one_minus_beta2 = d->one_minus_beta2;
  a.eps = d->eps;
  a.weight_decay = d->weight_decay;
  a.step = d->step_size;
  a.bc2_sqrt = d->bias_correction2_sqrt;
  a.dev = d->dev_scalars;
  a.steps = d->dev_steps;
  a.table = d->dev_table;
  a.table_n = d->table_n;
  if (a.steps && (!a.table || a.table_n < 1)) return fail(SIREN_EINVAL, "adam: dev_steps without a table");
  a.maximize = d->maximize;
  if (maxn == 0) {
    if (a.steps) return fail(SIREN_EINVAL, "adam: dev_steps with no elements (the counters would not advance)");
    return SIREN_OK;
  }
  hipLaunchKernelGGL(adam_kernel, dim3(grid1d(maxn, 1024), (unsigned)d->num_tensors), dim3(256), 0,
                     (hipStream_t)stream, a);
  return check_launch("adam");
}

}  // extern "C"
