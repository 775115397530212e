// rt_jvp.hip — analytic derivatives of the SIREN stack (siren_jvp_*): tangent-stream layout and the
// launch plan of their forward and backward pass. Included by siren_runtime.hip after rt_mlp.hip.
namespace {

// ============================================================================================
// Analytic derivatives (tangent streams): layout and orchestration.
// saved = [prepared weights][P_l phase tensors, l = 0..L-2][U_l fp32 tangent planes, l = 0..L-2]
// ============================================================================================
struct JLayout {
  Layout base;             // prepared-weight offsets (w_op_off / wt_op_off / weights_bytes)
  int C, Su, S, Sb;        // tangents, stored U planes, forward streams, adjoint streams
  int64_t p_off[SIREN_MAX_LAYERS], u_off[SIREN_MAX_LAYERS];
  int64_t saved_bytes;
  int64_t d_off[2], raw_off, part_off, ws_bytes;
};

Split jtn_split(const Geo& g, int64_t stacked_rows, int M, int N) {
  const int64_t tiles = cdiv(M, 128) * cdiv(N, 128);
  return split_rows(stacked_rows, tiles, g.nb, 32);
}
Split jcol_split(const Geo& g) { return split_rows(g.rows, 1, g.nb, 64); }

JLayout jlayout_of(const siren_mlp_desc* d, int order) {
  const Geo g = geo_of(d);
  JLayout jl;
  memset(&jl, 0, sizeof(jl));
  jl.base = layout_of(d);
  jl.C = d->dims[0];
  // stored U planes: the C tangents, then the Laplacian's V or the Hessian's C (C + 1) / 2 pair streams
  jl.Su = jl.C + (order == SIREN_JVP_LAPLACE ? 1 : order == SIREN_JVP_HESSIAN ? jl.C * (jl.C + 1) / 2 : 0);
  jl.S = 1 + jl.Su;
  jl.Sb = 1 + jl.Su;  // adjoints [a_bar; u_bar^k (; V_bar / V_bar^{jk})] mirror the forward streams
  int64_t off = jl.base.weights_bytes;
  for (int l = 0; l + 1 < g.L; ++l) {
    jl.p_off[l] = off;
    off = align_up(off + g.total * d->dims[l + 1] * g.phase_sz, 256);
  }
  for (int l = 0; l + 1 < g.L; ++l) {
    jl.u_off[l] = off;
    off = align_up(off + (int64_t)jl.Su * g.total * d->dims[l + 1] * 4, 256);
  }
  jl.saved_bytes = off;
  off = align_up(jl.base.weights_bytes, 256);  // workspace (prepared weights first when no saved)
  const int64_t act = (int64_t)jl.Sb * g.total * max_hidden(d);
  for (int k = 0; k < 2; ++k) {
    jl.d_off[k] = off;
    off = align_up(off + act * g.grad_sz, 256);
  }
  jl.raw_off = off;
  off = align_up(off + act * 4, 256);
  int64_t part = 0;
  for (int l = 1; l + 1 < g.L; ++l) {
    const int M = d->dims[l + 1], N = d->dims[l];
    const Split s = jtn_split(g, (int64_t)jl.Sb * g.rows, M, N);
    part = std::max(part, s.nsplit * split_stride(g, (int64_t)M * N + M));
  }
  {
    const Split s = jcol_split(g);
    const int F = d->dims[g.L - 1], O = d->dims[g.L];
    part = std::max(part, s.nsplit * split_stride(g, (int64_t)O * F + O));
    const int F0 = d->dims[1], C = d->dims[0];
    part = std::max(part, s.nsplit * split_stride(g, (int64_t)F0 * C + F0));
  }
  jl.part_off = off;
  off = align_up(off + part * 4, 256);
  jl.ws_bytes = off;
  return jl;
}

int jvp_check(const siren_mlp_desc* d, int order) {
  int rc = siren_mlp_check(d);
  if (rc) return rc;
  if (order != SIREN_JVP_GRADIENT && order != SIREN_JVP_LAPLACE && order != SIREN_JVP_JACOBIAN &&
      order != SIREN_JVP_HESSIAN)
    return fail(SIREN_EINVAL, "derivative mode %d unsupported (1 gradient, 2 Laplacian, 3 Jacobian, 4 Hessian)", order);
  if (!d->outermost_linear) return fail(SIREN_EINVAL, "analytic derivatives need outermost_linear");
  if (d->dims[0] > 4) return fail(SIREN_EINVAL, "analytic derivatives support in_features <= 4");
  if (order == SIREN_JVP_HESSIAN && d->dims[0] > 3)
    return fail(SIREN_EINVAL, "the analytic Hessian supports in_features <= 3 (got %d)", d->dims[0]);
  if (order == SIREN_JVP_HESSIAN && d->dims[d->num_layers] > FUSED_MAXO)
    return fail(SIREN_EINVAL, "the analytic Hessian supports out_features <= %d", FUSED_MAXO);
  return SIREN_OK;
}

template <int PREC>
int jvp_forward_impl(const siren_mlp_desc* d, int order, const float* x, float* grad, float* lap,
                     char* saved, char* ws, hipStream_t st, const char* primal = nullptr) {
  const Geo g = geo_of(d);
  const JLayout jl = jlayout_of(d, order);
  char* base = saved ? saved : ws;
  int rc = prep_weights<PREC>(d, g, jl.base, base, st);
  if (rc) return rc;
  // without a saved buffer the per-layer tensors still need a home: use the saved layout inside
  // the workspace tail (jvp workspace queries include it in that case, see siren_jvp_workspace_bytes)
  char* store = saved ? saved : ws + jl.ws_bytes;
  // primal given: layer l's phases are the plain forward's saved P_l (siren_mlp_forward's layout),
  // and only the tangent streams run (stacked rows N .. S N)
  auto pptr = [&](int l) -> char* { return primal ? (char*)primal + jl.base.saved_off[l] : store + jl.p_off[l]; };
  const bool hess = order == SIREN_JVP_HESSIAN;
  {
    JFirstArgs a;
    a.x = x;
    a.W = d->weight[0];
    a.bias = d->bias[0];
    a.P = primal ? nullptr : store + jl.p_off[0];
    a.U = (float*)(store + jl.u_off[0]);
    a.N = g.rows;
    a.C = d->dims[0];
    a.F = d->dims[1];
    a.Su = jl.Su;
    a.w_bstride = d->weights_batched ? (int64_t)d->dims[1] * d->dims[0] : 0;
    a.b_bstride = d->weights_batched ? d->dims[1] : 0;
    a.w0 = d->w0;
    hipLaunchKernelGGL(jvp_first_kernel<PREC>, dim3(grid1d(g.rows * a.F, std::max<int64_t>(1, 4096 / g.nb)), (unsigned)g.nb),
                       dim3(256), 0, st, a);
    if ((rc = check_launch("jvp_first"))) return rc;
  }
  for (int l = 1; l + 1 < g.L; ++l) {
    JNTArgs a;
    a.P = pptr(l - 1);
    a.U = (const float*)(store + jl.u_off[l - 1]);
    a.D = nullptr;
    a.W = PREC == kPrecBF16 ? (const void*)(base + jl.base.w_op_off[l]) : (const void*)d->weight[l];
    a.bias = d->bias[l];
    a.Pout = pptr(l);
    a.Uout = (float*)(store + jl.u_off[l]);
    a.N = g.rows;
    a.srow0 = primal ? g.rows : 0;
    a.S = jl.S;
    a.C = jl.C;
    a.lap = order == SIREN_JVP_LAPLACE;
    a.w_bstride = d->weights_batched ? (int64_t)d->dims[l + 1] * d->dims[l] : 0;
    a.b_bstride = d->weights_batched ? d->dims[l + 1] : 0;
    a.K = d->dims[l];
    a.Nout = d->dims[l + 1];
    a.w0 = d->w0;
    // (the row-stacked tile carries the tangents alone: not for the modes with second-order streams)
    if (PREC == kPrecF32 && primal && !a.lap && !hess && g_jvp_tan && jl.C >= 1 && jl.C <= 4 && a.Nout <= JADJ_BN &&
        a.K % JNT_KC == 0) {
      // the tangent streams only, stacked by row: one phase load and cosine per element
      JTanArgs t;
      t.P = a.P;
      t.U = a.U;
      t.W = a.W;
      t.Uout = a.Uout;
      t.N = g.rows;
      t.Su = jl.Su;
      t.w_bstride = a.w_bstride;
      t.K = a.K;
      t.Nout = a.Nout;
      t.w0 = a.w0;
      const dim3 tg((unsigned)cdiv(g.rows, JADJ_ROWS), (unsigned)g.nb);
      // (fp32 only: the primal stream is given by the fp32 forward alone, jvp_primal_check)
      constexpr int TP = kPrecF32;
      switch (jl.C) {
        case 1: hipLaunchKernelGGL((jvp_tan_kernel<TP, 1>), tg, dim3(512), 0, st, t); break;
        case 2: hipLaunchKernelGGL((jvp_tan_kernel<TP, 2>), tg, dim3(512), 0, st, t); break;
        case 3: hipLaunchKernelGGL((jvp_tan_kernel<TP, 3>), tg, dim3(512), 0, st, t); break;
        default: hipLaunchKernelGGL((jvp_tan_kernel<TP, 4>), tg, dim3(512), 0, st, t); break;
      }
      if ((rc = check_launch("jvp_tan"))) return rc;
      continue;
    }
    dim3 grid((unsigned)cdiv((int64_t)jl.S * g.rows - a.srow0, JNT_BM), (unsigned)cdiv(a.Nout, JNT_BN), (unsigned)g.nb);
    if (a.lap) hipLaunchKernelGGL((jvp_nt_kernel<PREC, JMODE_FWD, true>), grid, dim3(256), 0, st, a);
    else if (hess) hipLaunchKernelGGL((jvp_nt_kernel<PREC, JMODE_FWD, false, true>), grid, dim3(256), 0, st, a);
    else hipLaunchKernelGGL((jvp_nt_kernel<PREC, JMODE_FWD>), grid, dim3(256), 0, st, a);
    if ((rc = check_launch("jvp_nt fwd"))) return rc;
  }
  {
    const int l = g.L - 1;
    JLastArgs a;
    a.P = pptr(l - 1);
    a.U = (const float*)(store + jl.u_off[l - 1]);
    a.W = d->weight[l];
    a.grad = grad;
    a.lap = order == SIREN_JVP_LAPLACE ? lap : nullptr;
    a.jac = order == SIREN_JVP_JACOBIAN;
    a.N = g.rows;
    a.C = jl.C;
    a.F = d->dims[l];
    a.O = d->dims[l + 1];
    a.Su = jl.Su;
    a.w_bstride = d->weights_batched ? (int64_t)d->dims[l + 1] * d->dims[l] : 0;
    a.w0 = d->w0;
    const dim3 lgrid((unsigned)std::min<int64_t>(cdiv(g.rows, 8), 4096 / g.nb + 1), (unsigned)g.nb);
    if (hess) {  // grad is the per-channel Hessian [rows][O][C][C]
      switch (jl.C) {
        case 1: hipLaunchKernelGGL((jvp_last_hess_kernel<PREC, 1>), lgrid, dim3(256), 0, st, a); break;
        case 2: hipLaunchKernelGGL((jvp_last_hess_kernel<PREC, 2>), lgrid, dim3(256), 0, st, a); break;
        default: hipLaunchKernelGGL((jvp_last_hess_kernel<PREC, 3>), lgrid, dim3(256), 0, st, a); break;
      }
    } else {
      hipLaunchKernelGGL(jvp_last_kernel<PREC>, lgrid, dim3(256), 0, st, a);
    }
    if ((rc = check_launch("jvp_last"))) return rc;
  }
  return SIREN_OK;
}

// jvp_hess_combine_kernel for C = 1..3 tangents (jvp_check)
template <int PREC, bool TOP>
void launch_hess_combine(int C, dim3 grid, hipStream_t st, const JCombArgs& a) {
  switch (C) {
    case 1: hipLaunchKernelGGL((jvp_hess_combine_kernel<PREC, 1, TOP>), grid, dim3(256), 0, st, a); break;
    case 2: hipLaunchKernelGGL((jvp_hess_combine_kernel<PREC, 2, TOP>), grid, dim3(256), 0, st, a); break;
    default: hipLaunchKernelGGL((jvp_hess_combine_kernel<PREC, 3, TOP>), grid, dim3(256), 0, st, a); break;
  }
}

// jvp_tn2_kernel (fp32 weight gradient of a hidden layer): dW of 256 rows (the layer's width M), input
// width a multiple of 4; option jvp_tn2 (default on)
bool jvp_tn2_ok(int M, int N) { return g_jvp_tn2 && M == 256 && N % 4 == 0; }
Split jtn2_split(const Geo& g, int64_t stacked_rows, int N) {
  const int64_t want = std::max<int64_t>(1, 256 / (cdiv(N, JTN2_BN) * g.nb));
  Split s;
  s.rows_per_split = std::max<int64_t>(JTN2_KC, align_up(cdiv(stacked_rows, want), JTN2_KC));
  s.nsplit = std::max<int64_t>(1, cdiv(stacked_rows, s.rows_per_split));
  return s;
}

// jvp_adj_kernel's shapes: 2..4 adjoint streams (gradient with C <= 3, Laplacian with C <= 2) and a
// layer below of at most 256 features (one column tile)
bool jvp_adj_fused(int S, int lap, int Nout) {
  return g_jvp_adj && S >= 2 && S <= 4 && !(lap && S < 3) && Nout <= JADJ_BN;
}

template <int PREC>
int jvp_backward_impl(const siren_mlp_desc* d, int order, const float* x, const float* dout,
                      const char* saved, char* ws, float* const* dW, float* const* db, float* dx, hipStream_t st,
                      const char* primal = nullptr) {
  const Geo g = geo_of(d);
  const JLayout jl = jlayout_of(d, order);
  auto pptr = [&](int l) -> const char* { return primal ? primal + jl.base.saved_off[l] : saved + jl.p_off[l]; };
  const int lapmode = order == SIREN_JVP_LAPLACE;
  const bool hess = order == SIREN_JVP_HESSIAN;
  float* part = (float*)(ws + jl.part_off);
  int rc = SIREN_OK;
  int cur = 0;
  {
    const int l = g.L - 1;
    const Split s = jcol_split(g);
    JCombArgs a;
    a.P = pptr(l - 1);
    a.U = (const float*)(saved + jl.u_off[l - 1]);
    a.raw = nullptr;
    a.gbar = lapmode ? nullptr : dout;
    a.lbar = lapmode ? dout : nullptr;
    a.WL = d->weight[l];
    a.D = ws + jl.d_off[cur];
    a.part = part;
    a.N = g.rows;
    a.rows_per_split = s.rows_per_split;
    a.C = jl.C;
    a.F = d->dims[l];
    a.O = d->dims[l + 1];
    a.Su = jl.Su;
    a.S = jl.Sb;
    a.top = 1;
    a.lap = lapmode;
    a.split_stride = split_stride(g, (int64_t)a.O * a.F + a.O);
    a.w_bstride = d->weights_batched ? (int64_t)d->dims[l + 1] * d->dims[l] : 0;
    a.w0 = d->w0;
    a.jac = order == SIREN_JVP_JACOBIAN;
    if (hess)
      launch_hess_combine<PREC, true>(jl.C, dim3((unsigned)s.nsplit, (unsigned)g.nb), st, a);
    else if (a.jac)
      hipLaunchKernelGGL(jvp_combine_jac_kernel<PREC>, dim3((unsigned)s.nsplit, (unsigned)g.nb), dim3(256), 0, st, a);
    else
      hipLaunchKernelGGL(jvp_combine_kernel<PREC>, dim3((unsigned)s.nsplit, (unsigned)g.nb), dim3(256), 0, st, a);
    if ((rc = check_launch("jvp_combine top"))) return rc;
    if ((rc = launch_reduce(part, s.nsplit, a.split_stride, g.nb, (int64_t)a.O * a.F + a.O,
                            (int64_t)a.O * a.F, dW[l], db[l], st)))
      return rc;
  }
  for (int l = g.L - 2; l >= 1; --l) {
    const int M = d->dims[l + 1], N = d->dims[l];
    {
      const Split s = jtn_split(g, (int64_t)jl.Sb * g.rows, M, N);
      JTNArgs a;
      a.D = ws + jl.d_off[cur];
      a.P = pptr(l - 1);
      a.U = (const float*)(saved + jl.u_off[l - 1]);
      a.part = part;
      a.N = g.rows;
      a.rows_per_split = s.rows_per_split;
      a.split_stride = split_stride(g, (int64_t)M * N + M);
      a.S = jl.Sb;
      a.Su = jl.Su;
      a.C = jl.C;
      a.M = M;
      a.Kin = N;
      a.w0 = d->w0;
      if (PREC == kPrecF32 && !hess && jvp_tn2_ok(M, N)) {  // (jvp_tn2_kernel has no pair-stream operand)
        // fp32: all 256 dW rows per workgroup (jvp_tn2_kernel), with its own, smaller split count
        const Split s2 = jtn2_split(g, (int64_t)jl.Sb * g.rows, N);
        a.rows_per_split = s2.rows_per_split;
        dim3 grid2((unsigned)cdiv(N, JTN2_BN), (unsigned)s2.nsplit, (unsigned)g.nb);
        if (lapmode) hipLaunchKernelGGL((jvp_tn2_kernel<true>), grid2, dim3(512), 0, st, a);
        else hipLaunchKernelGGL((jvp_tn2_kernel<false>), grid2, dim3(512), 0, st, a);
        if ((rc = check_launch("jvp_tn2"))) return rc;
        if ((rc = launch_reduce(part, s2.nsplit, a.split_stride, g.nb, (int64_t)M * N + M, (int64_t)M * N,
                                dW[l], db[l], st)))
          return rc;
      } else {
        dim3 grid((unsigned)(cdiv(M, 128) * cdiv(N, 128)), (unsigned)s.nsplit, (unsigned)g.nb);
        if (lapmode) hipLaunchKernelGGL((jvp_tn_kernel<PREC, true>), grid, dim3(256), 0, st, a);
        else if (hess) hipLaunchKernelGGL((jvp_tn_kernel<PREC, false, true>), grid, dim3(256), 0, st, a);
        else hipLaunchKernelGGL((jvp_tn_kernel<PREC>), grid, dim3(256), 0, st, a);
        if ((rc = check_launch("jvp_tn"))) return rc;
        if ((rc = launch_reduce(part, s.nsplit, a.split_stride, g.nb, (int64_t)M * N + M, (int64_t)M * N,
                                dW[l], db[l], st)))
          return rc;
      }
    }
    if (!hess && jvp_adj_fused(jl.Sb, lapmode, N)) {  // (jvp_adj_kernel's combine has no pair streams)
      // adjoint GEMM + combine in one launch (jvp_adj_kernel)
      JAdjArgs a;
      a.D = ws + jl.d_off[cur];
      a.W = saved + jl.base.wt_op_off[l];
      a.P = pptr(l - 1);
      a.U = (const float*)(saved + jl.u_off[l - 1]);
      a.Dout = ws + jl.d_off[cur ^ 1];
      a.N = g.rows;
      a.Su = jl.Su;
      a.w_bstride = d->weights_batched ? (int64_t)M * N : 0;
      a.K = M;
      a.Nout = N;
      a.w0 = d->w0;
      const dim3 grid((unsigned)cdiv(g.rows, JADJ_ROWS), (unsigned)g.nb);
      switch (jl.Sb * 2 + lapmode) {
        case 4: hipLaunchKernelGGL((jvp_adj_kernel<PREC, 2, false>), grid, dim3(512), 0, st, a); break;
        case 6: hipLaunchKernelGGL((jvp_adj_kernel<PREC, 3, false>), grid, dim3(512), 0, st, a); break;
        case 7: hipLaunchKernelGGL((jvp_adj_kernel<PREC, 3, true>), grid, dim3(512), 0, st, a); break;
        case 8: hipLaunchKernelGGL((jvp_adj_kernel<PREC, 4, false>), grid, dim3(512), 0, st, a); break;
        default: hipLaunchKernelGGL((jvp_adj_kernel<PREC, 4, true>), grid, dim3(512), 0, st, a); break;
      }
      if ((rc = check_launch("jvp_adj"))) return rc;
      cur ^= 1;
      continue;
    }
    {
      JNTArgs a;
      memset(&a, 0, sizeof(a));
      a.D = ws + jl.d_off[cur];
      a.W = saved + jl.base.wt_op_off[l];
      a.Uout = (float*)(ws + jl.raw_off);
      a.N = g.rows;
      a.S = jl.Sb;
      a.C = jl.C;
      a.w_bstride = d->weights_batched ? (int64_t)M * N : 0;
      a.K = M;
      a.Nout = N;
      a.w0 = d->w0;
      dim3 grid((unsigned)cdiv((int64_t)jl.Sb * g.rows, JNT_BM), (unsigned)cdiv(N, JNT_BN), (unsigned)g.nb);
      hipLaunchKernelGGL((jvp_nt_kernel<PREC, JMODE_BWD>), grid, dim3(256), 0, st, a);
      if ((rc = check_launch("jvp_nt bwd"))) return rc;
    }
    {
      const Split s = jcol_split(g);
      JCombArgs a;
      memset(&a, 0, sizeof(a));
      a.P = pptr(l - 1);
      a.U = (const float*)(saved + jl.u_off[l - 1]);
      a.raw = (const float*)(ws + jl.raw_off);
      a.D = ws + jl.d_off[cur ^ 1];
      a.N = g.rows;
      a.rows_per_split = s.rows_per_split;
      a.C = jl.C;
      a.F = N;
      a.Su = jl.Su;
      a.S = jl.Sb;
      a.top = 0;
      a.lap = lapmode;
      a.w0 = d->w0;
      if (hess) launch_hess_combine<PREC, false>(jl.C, dim3((unsigned)s.nsplit, (unsigned)g.nb), st, a);
      else hipLaunchKernelGGL(jvp_combine_kernel<PREC>, dim3((unsigned)s.nsplit, (unsigned)g.nb), dim3(256), 0, st, a);
      if ((rc = check_launch("jvp_combine"))) return rc;
      cur ^= 1;
    }
  }
  {
    const Split s = jcol_split(g);
    JFirstBwdArgs a;
    a.D = ws + jl.d_off[cur];
    a.x = x;
    a.W = d->weight[0];
    a.dx = dx;
    a.part = part;
    a.N = g.rows;
    a.rows_per_split = s.rows_per_split;
    a.C = d->dims[0];
    a.F = d->dims[1];
    a.S = jl.Sb;
    a.split_stride = split_stride(g, (int64_t)a.F * a.C + a.F);
    a.w_bstride = d->weights_batched ? (int64_t)d->dims[1] * d->dims[0] : 0;
    hipLaunchKernelGGL(jvp_first_bwd_kernel<PREC>, dim3((unsigned)s.nsplit, (unsigned)g.nb), dim3(256), 0, st, a);
    if ((rc = check_launch("jvp_first_bwd"))) return rc;
    if ((rc = launch_reduce(part, s.nsplit, a.split_stride, g.nb, (int64_t)a.F * a.C + a.F,
                            (int64_t)a.F * a.C, dW[0], db[0], st)))
      return rc;
    if (dx) {
      hipLaunchKernelGGL(jvp_first_dx_kernel<PREC>, dim3((unsigned)std::min<int64_t>(cdiv(g.rows, 8), 4096 / g.nb + 1), (unsigned)g.nb),
                         dim3(256), 0, st, a);
      if ((rc = check_launch("jvp_first_dx"))) return rc;
    }
  }
  return SIREN_OK;
}

// the plain forward's saved buffer as the primal stream of a jvp (fp32 mode: its phases are the
// jvp's fp32 phases; siren_mlp_forward's layout)
int jvp_primal_check(const siren_mlp_desc* d, const void* primal, int64_t primal_bytes) {
  if (!primal) return SIREN_OK;
  if (d->prec != SIREN_PREC_F32) return fail(SIREN_EINVAL, "jvp primal: fp32 mode only");
  if (!d->outermost_linear) return fail(SIREN_EINVAL, "jvp primal: needs outermost_linear");
  const Layout lo = layout_of(d);
  if (primal_bytes < lo.saved_bytes)
    return fail(SIREN_ENOSPACE, "jvp primal: saved buffer %lld < %lld bytes", (long long)primal_bytes,
                (long long)lo.saved_bytes);
  for (int l = 0; l + 1 < d->num_layers; ++l)
    if (lo.saved_off[l] < 0) return fail(SIREN_EINVAL, "jvp primal: layer %d phases not kept", l);
  return SIREN_OK;
}
}  // namespace

extern "C" {

int64_t siren_jvp_saved_bytes(const siren_mlp_desc* d, int order) {
  if (jvp_check(d, order)) return -1;
  return jlayout_of(d, order).saved_bytes;
}

int64_t siren_jvp_workspace_bytes(const siren_mlp_desc* d, int order) {
  if (jvp_check(d, order)) return -1;
  const JLayout jl = jlayout_of(d, order);
  return jl.ws_bytes + jl.saved_bytes;  // room for the per-layer tensors when no saved buffer is given
}

int siren_jvp_forward_ex(const siren_mlp_desc* d, int order, const float* x, float* grad, float* lap,
                         void* saved, int64_t saved_bytes, void* workspace, int64_t workspace_bytes,
                         const void* primal, int64_t primal_bytes, void* stream) {
  int rc = jvp_check(d, order);
  if (rc) return rc;
  if ((rc = jvp_primal_check(d, primal, primal_bytes))) return rc;
  const JLayout jl = jlayout_of(d, order);
  const int64_t need = saved ? jl.ws_bytes : jl.ws_bytes + jl.saved_bytes;
  if ((rc = check_buffers(saved, saved_bytes, jl.saved_bytes, false, workspace, workspace_bytes, need))) return rc;
  if (!x || !grad || (order == SIREN_JVP_LAPLACE && !lap)) return fail(SIREN_EINVAL, "null x/grad/lap");
  g_err.clear();
  hipStream_t st = (hipStream_t)stream;
  if (d->prec == SIREN_PREC_BF16)
    return jvp_forward_impl<kPrecBF16>(d, order, x, grad, lap, (char*)saved, (char*)workspace, st);
  return jvp_forward_impl<kPrecF32>(d, order, x, grad, lap, (char*)saved, (char*)workspace, st, (const char*)primal);
}

int siren_jvp_forward(const siren_mlp_desc* d, int order, const float* x, float* grad, float* lap,
                      void* saved, int64_t saved_bytes, void* workspace, int64_t workspace_bytes,
                      void* stream) {
  return siren_jvp_forward_ex(d, order, x, grad, lap, saved, saved_bytes, workspace, workspace_bytes, nullptr, 0,
                              stream);
}

int siren_jvp_backward_ex(const siren_mlp_desc* d, int order, const float* x, const float* dgrad,
                          const void* saved, int64_t saved_bytes, void* workspace, int64_t workspace_bytes,
                          float* const* dweight, float* const* dbias, float* dx, const void* primal,
                          int64_t primal_bytes, void* stream) {
  int rc = jvp_check(d, order);
  if (rc) return rc;
  if ((rc = jvp_primal_check(d, primal, primal_bytes))) return rc;
  const JLayout jl = jlayout_of(d, order);
  if ((rc = check_buffers(saved, saved_bytes, jl.saved_bytes, true, workspace, workspace_bytes, jl.ws_bytes))) return rc;
  if (!x || !dgrad || !dweight || !dbias) return fail(SIREN_EINVAL, "null argument");
  for (int l = 0; l < d->num_layers; ++l)
    if (!dweight[l] || !dbias[l]) return fail(SIREN_EINVAL, "layer %d: null gradient output", l);
  g_err.clear();
  hipStream_t st = (hipStream_t)stream;
  if (d->prec == SIREN_PREC_BF16)
    return jvp_backward_impl<kPrecBF16>(d, order, x, dgrad, (const char*)saved, (char*)workspace, dweight, dbias, dx, st);
  return jvp_backward_impl<kPrecF32>(d, order, x, dgrad, (const char*)saved, (char*)workspace, dweight, dbias, dx, st,
                                     (const char*)primal);
}

int siren_jvp_backward(const siren_mlp_desc* d, int order, const float* x, const float* dgrad,
                       const void* saved, int64_t saved_bytes, void* workspace, int64_t workspace_bytes,
                       float* const* dweight, float* const* dbias, float* dx, void* stream) {
  return siren_jvp_backward_ex(d, order, x, dgrad, saved, saved_bytes, workspace, workspace_bytes, dweight, dbias, dx,
                               nullptr, 0, stream);
}

}  // extern "C"
