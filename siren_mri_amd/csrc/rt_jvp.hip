// rt_jvp.hip — analytic derivatives of the SIREN stack (siren_jvp_*): tangent-stream layout and the
// launch plan of their forward and backward pass. Included by siren_runtime.hip after rt_mlp.hip.
namespace {

// ============================================================================================
// Analytic derivatives (tangent streams): layout, launch plan and its walk.
// saved = [prepared weights][P_l phase tensors, l = 0..L-2][U_l fp32 tangent planes, l = 0..L-2]
// ============================================================================================
struct JLayout {
  Layout base;             // prepared-weight offsets (w_op_off / wt_op_off / weights_bytes)
  int C, Su, S;            // tangents, stored U planes, streams: the forward's, and the adjoints
                           // [a_bar; u_bar^k (; V_bar / V_bar^{jk})] that mirror them
  int64_t p_off[SIREN_MAX_LAYERS], u_off[SIREN_MAX_LAYERS];
  int64_t saved_bytes;
  int64_t d_off[2], raw_off, part_off, part_elems, ws_bytes;
};

// Split-K geometry of a hidden layer's weight gradient over the row-stacked streams (jvp_tn_kernel;
// jvp_tn2_kernel: jtn2_split), and of the first / output layer's
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
  const int64_t act = (int64_t)jl.S * g.total * max_hidden(d);
  for (int k = 0; k < 2; ++k) {
    jl.d_off[k] = off;
    off = align_up(off + act * g.grad_sz, 256);
  }
  jl.raw_off = off;
  off = align_up(off + act * 4, 256);
  // partial slabs: the most any launch of plan_jvp_backward writes, under either weight-gradient kernel.
  // (jtn2_split never asks for more than jtn_split: both round rows to 32, and jtn_split's wanted count
  // 1024 / (tiles nb), with tiles <= 4 cdiv(N, 128), is at least jtn2_split's 256 / (cdiv(N, 128) nb).)
  int64_t part = 0;
  for (int l = 1; l + 1 < g.L; ++l) {
    const int M = d->dims[l + 1], N = d->dims[l];
    const int64_t stacked = (int64_t)jl.S * g.rows;
    part = std::max(part, std::max(jtn_split(g, stacked, M, N).nsplit, jtn2_split(g, stacked, N).nsplit) *
                              split_stride(g, slab_elems(d, l)));
  }
  part = std::max(part, jcol_split(g).nsplit * split_stride(g, std::max(slab_elems(d, g.L - 1), slab_elems(d, 0))));
  jl.part_off = off;
  jl.part_elems = part;
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

// ---------------------------------------------------------------------------- which kernel a layer takes
// The second-order streams of an order, as the index of a kernel table: none (gradient, Jacobian), the
// Laplacian's one, or the Hessian's pair streams. jvp_nt_kernel <JMODE_FWD>, jvp_tn_kernel, jvp_last_hess_kernel
// and jvp_hess_combine_kernel have a pair-stream form; jvp_tan_kernel, jvp_tn2_kernel and jvp_adj_kernel
// have no pair-stream operand, so the Hessian never takes them (the three predicates below).
enum JMode { JM_PLAIN, JM_LAP, JM_HESS };
inline JMode jmode(int order) {
  return order == SIREN_JVP_LAPLACE ? JM_LAP : order == SIREN_JVP_HESSIAN ? JM_HESS : JM_PLAIN;
}
// Row-stacked tangents (jvp_tan_kernel, option jvp_tan): a hidden layer's tangent streams alone, stacked by
// row, with one phase load and cosine per element. Only where the primal stream is given, so fp32
// (jvp_primal_rule); the tile carries the tangents alone, so no order with a second-order stream; one
// column tile, so a layer of at most JADJ_BN features.
bool jvp_tan_ok(const Geo& g, int order, bool primal_given, int Nout) {
  return g.prec == kPrecF32 && primal_given && jmode(order) == JM_PLAIN && g_jvp_tan && Nout <= JADJ_BN;
}
// All-rows weight gradient (jvp_tn2_kernel, jvp_tn2_ok): an fp32 kernel, with its own, smaller split count.
bool jvp_dw_rows(const Geo& g, int order, int M, int N) {
  return g.prec == kPrecF32 && jmode(order) != JM_HESS && jvp_tn2_ok(M, N);
}
// Fused adjoint (jvp_adj_kernel, option jvp_adj): the adjoint GEMM and the combine in one launch. Its forms
// carry 2..4 adjoint streams (gradient and Jacobian with C <= 3, Laplacian with C <= 2; with at least one
// input there are never fewer than 2, nor fewer than 3 with the Laplacian's) and one column tile, so a
// layer below of at most JADJ_BN features.
bool jvp_adj_fused(int order, int S, int Nout) {
  return g_jvp_adj && jmode(order) != JM_HESS && S <= 4 && Nout <= JADJ_BN;
}

// ---------------------------------------------------------------------------- the plan
enum JKern {
  J_FIRST,      // first layer: phases and tangents from x
  J_NT_FWD,     // hidden layer forward, all streams (with a primal: the tangent streams) on jvp_nt_kernel
  J_TAN,        //   the tangent streams on jvp_tan_kernel
  J_LAST,       // output layer: the derivative itself
  J_COMB,       // adjoints of a layer's streams from the cotangent (output layer: with its dW / db slabs) or from `raw`
  J_REDUCE,     // the slabs of the launch before it summed into dW / db of their layer
  J_TN,         // hidden layer weight gradient (jvp_tn_kernel or jvp_tn2_kernel)
  J_ADJ,        // hidden layer adjoint GEMM + combine in one launch
  J_NT_BWD,     // hidden layer adjoint GEMM into `raw` (a J_COMB follows)
  J_FIRST_BWD,  // first layer weight gradient
  J_FIRST_DX    // input gradient
};
struct JLaunch {
  JKern kern;
  const void* fn;    // Kernel<Args>::fn of the Args the kind takes, and its profiler name
  const char* sym;
  const char* what;  // its name in a launch error
  int layer;
  int cur;           // which adjoint buffer holds the layer's adjoints (the other receives the layer below's)
  dim3 grid;
  unsigned block;
  int64_t rows_per_split;
  int64_t nsplit;    // slabs written to `part` (J_REDUCE: read); 0: none
};
struct JvpPlan {
  int n = 0;
  JLaunch steps[4 * SIREN_MAX_LAYERS + 8];  // (at most 4 per hidden layer and 6 around them)

  template <class K>
  JLaunch& add(JKern kern, const K& k, const char* what, int layer, int cur, dim3 grid, unsigned block) {
    assert(n < (int)(sizeof(steps) / sizeof(steps[0])));
    return steps[n++] = JLaunch{kern, (const void*)k.fn, k.sym, what, layer, cur, grid, block, 0, 0};
  }
};

inline dim3 grid3(int64_t x, int64_t y = 1, int64_t z = 1) { return dim3((unsigned)x, (unsigned)y, (unsigned)z); }

// the two precisions' forms of a kernel template, [kPrecF32 / kPrecBF16] (last index of the tables below)
#define JVP_P(K) {SIREN_K(K<0>), SIREN_K(K<1>)}
#define JVP_PA(K, ...) {SIREN_K(K<0, __VA_ARGS__>), SIREN_K(K<1, __VA_ARGS__>)}

JvpPlan plan_jvp_forward(const siren_mlp_desc* d, const Geo& g, const JLayout& jl, int order, bool primal_given) {
  static const Kernel<JFirstArgs> kFirst[2] = JVP_P(jvp_first_kernel);
  static const Kernel<JNTArgs> kNt[3][2] = {JVP_PA(jvp_nt_kernel, JMODE_FWD), JVP_PA(jvp_nt_kernel, JMODE_FWD, true),
                                            JVP_PA(jvp_nt_kernel, JMODE_FWD, false, true)};  // [JMode]
  static const Kernel<JTanArgs> kTan[4] = {SIREN_K(jvp_tan_kernel<0, 1>), SIREN_K(jvp_tan_kernel<0, 2>),
                                           SIREN_K(jvp_tan_kernel<0, 3>), SIREN_K(jvp_tan_kernel<0, 4>)};  // [C - 1], fp32
  static const Kernel<JLastArgs> kLast[2] = JVP_P(jvp_last_kernel);
  static const Kernel<JLastArgs> kLastHess[3][2] = {JVP_PA(jvp_last_hess_kernel, 1), JVP_PA(jvp_last_hess_kernel, 2),
                                                    JVP_PA(jvp_last_hess_kernel, 3)};  // [C - 1]
  JvpPlan p;
  const int P = g.prec, C = jl.C;
  const JMode m = jmode(order);
  const int64_t nb = g.nb;
  assert(C >= 1 && C <= (m == JM_HESS ? 3 : 4));  // jvp_check
  p.add(J_FIRST, kFirst[P], "jvp_first", 0, 0, grid3(grid1d(g.rows * d->dims[1], std::max<int64_t>(1, 4096 / nb)), nb), 256);
  for (int l = 1; l + 1 < g.L; ++l) {
    const int K = d->dims[l], Nout = d->dims[l + 1];
    assert(K % JNT_KC == 0);  // a hidden width: a multiple of 32 (siren_mlp_check)
    if (jvp_tan_ok(g, order, primal_given, Nout)) {
      p.add(J_TAN, kTan[C - 1], "jvp_tan", l, 0, grid3(cdiv(g.rows, JADJ_ROWS), nb), 512);
      continue;
    }
    // primal given: only the tangent streams run (stacked rows N .. S N)
    const int64_t stacked = (int64_t)jl.S * g.rows - (primal_given ? g.rows : 0);
    p.add(J_NT_FWD, kNt[m][P], "jvp_nt fwd", l, 0, grid3(cdiv(stacked, JNT_BM), cdiv(Nout, JNT_BN), nb), 256);
  }
  // (the Hessian's result is the per-channel Hessian [rows][O][C][C])
  p.add(J_LAST, m == JM_HESS ? kLastHess[C - 1][P] : kLast[P], "jvp_last", g.L - 1, 0,
        grid3(std::min<int64_t>(cdiv(g.rows, 8), 4096 / nb + 1), nb), 256);
  return p;
}

JvpPlan plan_jvp_backward(const siren_mlp_desc* d, const Geo& g, const JLayout& jl, int order, bool want_dx) {
  static const Kernel<int> kReduce = {nullptr, "siren::reduce_kernel"};  // (not via fn: launch_reduce)
  static const Kernel<JCombArgs> kComb[2] = JVP_P(jvp_combine_kernel), kCombJac[2] = JVP_P(jvp_combine_jac_kernel);
  static const Kernel<JCombArgs> kCombHess[3][2][2] = {  // [C - 1][output layer]
      {JVP_PA(jvp_hess_combine_kernel, 1, false), JVP_PA(jvp_hess_combine_kernel, 1, true)},
      {JVP_PA(jvp_hess_combine_kernel, 2, false), JVP_PA(jvp_hess_combine_kernel, 2, true)},
      {JVP_PA(jvp_hess_combine_kernel, 3, false), JVP_PA(jvp_hess_combine_kernel, 3, true)}};
  static const Kernel<JTNArgs> kTn[3][2] = {JVP_P(jvp_tn_kernel), JVP_PA(jvp_tn_kernel, true),
                                            JVP_PA(jvp_tn_kernel, false, true)};  // [JMode]
  static const Kernel<JTNArgs> kTn2[2] = {SIREN_K(jvp_tn2_kernel<false>), SIREN_K(jvp_tn2_kernel<true>)};  // [lap], fp32
  // 2, 3 or 4 streams; 3 and 4 also with the Laplacian's among them
  static const Kernel<JAdjArgs> kAdj[5][2] = {JVP_PA(jvp_adj_kernel, 2, false), JVP_PA(jvp_adj_kernel, 3, false),
                                              JVP_PA(jvp_adj_kernel, 3, true), JVP_PA(jvp_adj_kernel, 4, false),
                                              JVP_PA(jvp_adj_kernel, 4, true)};
  static const Kernel<JNTArgs> kNtBwd[2] = JVP_PA(jvp_nt_kernel, JMODE_BWD);
  static const Kernel<JFirstBwdArgs> kFirstBwd[2] = JVP_P(jvp_first_bwd_kernel), kFirstDx[2] = JVP_P(jvp_first_dx_kernel);
  JvpPlan p;
  const int P = g.prec, C = jl.C, S = jl.S;
  const JMode m = jmode(order);
  const int lap = m == JM_LAP;
  const int64_t nb = g.nb;
  assert(C >= 1 && C <= (m == JM_HESS ? 3 : 4) && S >= 2 + lap);  // jvp_check
  int cur = 0;
  // launch `a` writes s.nsplit slabs of dW / db[a.layer] to `part`; the reduce launch that sums them follows
  auto writes = [&](JLaunch& a, const Split& s) {
    assert(s.nsplit * split_stride(g, slab_elems(d, a.layer)) <= jl.part_elems);
    a.rows_per_split = s.rows_per_split;
    a.nsplit = s.nsplit;
    p.add(J_REDUCE, kReduce, "reduce", a.layer, cur, grid3(reduce_blocks(nb, slab_elems(d, a.layer))), 256).nsplit = s.nsplit;
  };
  const Split col = jcol_split(g);
  const dim3 col_grid = grid3(col.nsplit, nb);
  writes(p.add(J_COMB, m == JM_HESS ? kCombHess[C - 1][1][P] : order == SIREN_JVP_JACOBIAN ? kCombJac[P] : kComb[P],
               "jvp_combine top", g.L - 1, cur, col_grid, 256),
         col);
  for (int l = g.L - 2; l >= 1; --l) {
    const int M = d->dims[l + 1], N = d->dims[l];
    const int64_t stacked = (int64_t)S * g.rows;
    if (jvp_dw_rows(g, order, M, N)) {
      const Split s = jtn2_split(g, stacked, N);
      writes(p.add(J_TN, kTn2[lap], "jvp_tn2", l, cur, grid3(cdiv(N, JTN2_BN), s.nsplit, nb), 512), s);
    } else {
      const Split s = jtn_split(g, stacked, M, N);
      writes(p.add(J_TN, kTn[m][P], "jvp_tn", l, cur, grid3(cdiv(M, 128) * cdiv(N, 128), s.nsplit, nb), 256), s);
    }
    if (jvp_adj_fused(order, S, N)) {
      p.add(J_ADJ, kAdj[S == 2 ? 0 : 2 * S - 5 + lap][P], "jvp_adj", l, cur, grid3(cdiv(g.rows, JADJ_ROWS), nb), 512);
    } else {
      p.add(J_NT_BWD, kNtBwd[P], "jvp_nt bwd", l, cur, grid3(cdiv(stacked, JNT_BM), cdiv(N, JNT_BN), nb), 256);
      p.add(J_COMB, m == JM_HESS ? kCombHess[C - 1][0][P] : kComb[P], "jvp_combine", l, cur, col_grid, 256).rows_per_split =
          col.rows_per_split;
    }
    cur ^= 1;
  }
  writes(p.add(J_FIRST_BWD, kFirstBwd[P], "jvp_first_bwd", 0, cur, col_grid, 256), col);
  if (want_dx)
    p.add(J_FIRST_DX, kFirstDx[P], "jvp_first_dx", 0, cur, grid3(std::min<int64_t>(cdiv(g.rows, 8), 4096 / nb + 1), nb), 256)
        .rows_per_split = col.rows_per_split;
  return p;
}

// The two plans as text, one line per launch (siren_jvp_plan).
std::string jvp_plan_text(const siren_mlp_desc* d, const JLayout& jl, int order, int flags, const JvpPlan& fwd,
                          const JvpPlan& bwd) {
  char buf[256];
  snprintf(buf, sizeof(buf), "# order=%d prec=%s flags=%d streams=%d fwd=%d bwd=%d\n", order,
           d->prec == SIREN_PREC_BF16 ? "bf16" : "fp32", flags, jl.S, fwd.n, bwd.n);
  std::string t = buf;
  for (const JvpPlan* p : {&fwd, &bwd})
    for (int i = 0; i < p->n; ++i) {
      const JLaunch& s = p->steps[i];
      int k = snprintf(buf, sizeof(buf), "%s %s layer=%d cur=%d grid=(%u,%u,%u) block=%u", p == &fwd ? "fwd" : "bwd", s.sym,
                       s.layer, s.cur, s.grid.x, s.grid.y, s.grid.z, s.block);
      if (s.nsplit) k += snprintf(buf + k, sizeof(buf) - k, " slab=part nsplit=%lld", (long long)s.nsplit);
      snprintf(buf + k, sizeof(buf) - k, "\n");
      t += buf;
    }
  return t;
}

// ---------------------------------------------------------------------------- the walk
// One call's buffers (a forward call has no dout / dW / db / dx, a backward call no out / lap), and the
// launcher of every kind of plan step.
struct JvpWalk {
  const siren_mlp_desc* d;
  const Geo& g;
  const JLayout& jl;
  int order;
  const float* x;
  float *out, *lap;     // forward: the derivative (Laplacian: scratch of the gradient's size, and the result)
  const float* dout;    // backward: the cotangent
  const char* weights;  // the prepared weights: the saved buffer, or the workspace of a forward without one
  char* store;          // the per-layer phases and tangents: the saved buffer, or the workspace's tail
  char* ws;
  const char* primal;   // the plain forward's saved buffer (its phases are the primal stream), or null
  float *const *dW, *const *db;
  float* dx;
  hipStream_t st;

  int dims(int l) const { return d->dims[l]; }
  // layer l's phases: with a primal the plain forward's saved P_l (siren_mlp_forward's layout)
  char* P(int l) const { return primal ? (char*)primal + jl.base.saved_off[l] : store + jl.p_off[l]; }
  float* U(int l) const { return (float*)(store + jl.u_off[l]); }
  char* adj(int k) const { return ws + jl.d_off[k]; }
  float* raw() const { return (float*)(ws + jl.raw_off); }
  float* part() const { return (float*)(ws + jl.part_off); }
  int64_t w_bstride(int l) const { return bstride(d, (int64_t)dims(l + 1) * dims(l)); }
  // what the kernels of layer l share: the phases and tangents of the layer below it
  template <class Args>
  Args below(int l) const {
    Args a{};
    a.P = P(l - 1);
    a.U = U(l - 1);
    a.N = g.rows;
    a.Su = jl.Su;
    a.w0 = d->w0;
    return a;
  }

  JFirstArgs first_args() const {
    JFirstArgs a{};
    a.x = x;
    a.W = d->weight[0];
    a.bias = d->bias[0];
    a.P = primal ? nullptr : P(0);
    a.U = U(0);
    a.N = g.rows;
    a.C = dims(0);
    a.F = dims(1);
    a.Su = jl.Su;
    a.w_bstride = w_bstride(0);
    a.b_bstride = bstride(d, dims(1));
    a.w0 = d->w0;
    return a;
  }
  JNTArgs nt_args(const JLaunch& s) const {
    const int l = s.layer;
    JNTArgs a{};
    a.N = g.rows;
    a.S = jl.S;
    a.C = jl.C;
    a.w_bstride = w_bstride(l);
    a.w0 = d->w0;
    if (s.kern == J_NT_FWD) {
      a.P = P(l - 1);
      a.U = U(l - 1);
      a.W = g.prec == kPrecBF16 ? (const void*)(weights + jl.base.w_op_off[l]) : (const void*)d->weight[l];
      a.bias = d->bias[l];
      a.Pout = P(l);
      a.Uout = U(l);
      a.srow0 = primal ? g.rows : 0;
      a.lap = order == SIREN_JVP_LAPLACE;
      a.b_bstride = bstride(d, dims(l + 1));
      a.K = dims(l);
      a.Nout = dims(l + 1);
    } else {  // J_NT_BWD: raw[s] = D[s] W_l
      a.D = adj(s.cur);
      a.W = weights + jl.base.wt_op_off[l];
      a.Uout = raw();
      a.K = dims(l + 1);
      a.Nout = dims(l);
    }
    return a;
  }
  JTanArgs tan_args(const JLaunch& s) const {
    const int l = s.layer;
    JTanArgs a = below<JTanArgs>(l);
    a.W = d->weight[l];  // (fp32: the weights as they are)
    a.Uout = U(l);
    a.w_bstride = w_bstride(l);
    a.K = dims(l);
    a.Nout = dims(l + 1);
    return a;
  }
  JLastArgs last_args(const JLaunch& s) const {
    const int l = s.layer;
    JLastArgs a = below<JLastArgs>(l);
    a.W = d->weight[l];
    a.grad = out;
    a.lap = order == SIREN_JVP_LAPLACE ? lap : nullptr;
    a.jac = order == SIREN_JVP_JACOBIAN;
    a.C = jl.C;
    a.F = dims(l);
    a.O = dims(l + 1);
    a.w_bstride = w_bstride(l);
    return a;
  }
  JCombArgs comb_args(const JLaunch& s) const {
    const int l = s.layer;
    const int lapmode = order == SIREN_JVP_LAPLACE;
    JCombArgs a = below<JCombArgs>(l);
    a.rows_per_split = s.rows_per_split;
    a.C = jl.C;
    a.F = dims(l);
    a.S = jl.S;
    a.top = l == g.L - 1;
    a.lap = lapmode;
    if (a.top) {  // from the cotangent, with the output layer's dW / db slabs
      a.gbar = lapmode ? nullptr : dout;
      a.lbar = lapmode ? dout : nullptr;
      a.WL = d->weight[l];
      a.D = adj(s.cur);
      a.part = part();
      a.O = dims(l + 1);
      a.split_stride = split_stride(g, slab_elems(d, l));
      a.w_bstride = w_bstride(l);
      a.jac = order == SIREN_JVP_JACOBIAN;
    } else {  // from the adjoint GEMM's raw output, into the other adjoint buffer
      a.raw = raw();
      a.D = adj(s.cur ^ 1);
    }
    return a;
  }
  JTNArgs tn_args(const JLaunch& s) const {
    const int l = s.layer;
    JTNArgs a = below<JTNArgs>(l);
    a.D = adj(s.cur);
    a.part = part();
    a.rows_per_split = s.rows_per_split;
    a.split_stride = split_stride(g, slab_elems(d, l));
    a.S = jl.S;
    a.C = jl.C;
    a.M = dims(l + 1);
    a.Kin = dims(l);
    return a;
  }
  JAdjArgs adj_args(const JLaunch& s) const {
    const int l = s.layer;
    JAdjArgs a = below<JAdjArgs>(l);
    a.D = adj(s.cur);
    a.W = weights + jl.base.wt_op_off[l];
    a.Dout = adj(s.cur ^ 1);
    a.w_bstride = w_bstride(l);
    a.K = dims(l + 1);
    a.Nout = dims(l);
    return a;
  }
  JFirstBwdArgs first_bwd_args(const JLaunch& s) const {
    JFirstBwdArgs a{};
    a.D = adj(s.cur);
    a.x = x;
    a.W = d->weight[0];
    a.dx = dx;
    a.part = part();
    a.N = g.rows;
    a.rows_per_split = s.rows_per_split;
    a.C = dims(0);
    a.F = dims(1);
    a.S = jl.S;
    a.split_stride = split_stride(g, slab_elems(d, 0));
    a.w_bstride = w_bstride(0);
    return a;
  }

  template <class Args>
  int go(const JLaunch& s, const Args& a) const {
    return launch_kernel(Kernel<Args>{(void (*)(Args))s.fn, s.sym}, s.grid, s.block, 0, s.what, st, a);
  }
  int run(const JLaunch& s) const {
    switch (s.kern) {
      case J_FIRST: return go(s, first_args());
      case J_NT_FWD:
      case J_NT_BWD: return go(s, nt_args(s));
      case J_TAN: return go(s, tan_args(s));
      case J_LAST: return go(s, last_args(s));
      case J_COMB: return go(s, comb_args(s));
      case J_TN: return go(s, tn_args(s));
      case J_ADJ: return go(s, adj_args(s));
      case J_FIRST_BWD:
      case J_FIRST_DX: return go(s, first_bwd_args(s));
      case J_REDUCE: {
        const int l = s.layer;
        const int64_t sz = slab_elems(d, l);
        return launch_reduce(part(), s.nsplit, split_stride(g, sz), g.nb, sz, sz - dims(l + 1), dW[l], db[l], st);
      }
    }
    return SIREN_OK;
  }
  int walk(const JvpPlan& p) const {
    for (int i = 0; i < p.n; ++i)
      if (int rc = run(p.steps[i])) return rc;
    return SIREN_OK;
  }
};

int jvp_forward_impl(const siren_mlp_desc* d, int order, const float* x, float* grad, float* lap, char* saved, char* ws,
                     hipStream_t st, const char* primal) {
  const Geo g = geo_of(d);
  const JLayout jl = jlayout_of(d, order);
  char* weights = saved ? saved : ws;
  if (int rc = g.prec == kPrecBF16 ? prep_weights<kPrecBF16>(d, g, jl.base, weights, st)
                                   : prep_weights<kPrecF32>(d, g, jl.base, weights, st))
    return rc;
  // without a saved buffer the per-layer tensors still need a home: use the saved layout inside
  // the workspace tail (jvp workspace queries include it in that case, see siren_jvp_workspace_bytes)
  char* store = saved ? saved : ws + jl.ws_bytes;
  const JvpWalk w{d, g, jl, order, x, grad, lap, nullptr, weights, store, ws, primal, nullptr, nullptr, nullptr, st};
  return w.walk(plan_jvp_forward(d, g, jl, order, primal != nullptr));
}

int jvp_backward_impl(const siren_mlp_desc* d, int order, const float* x, const float* dout, const char* saved, char* ws,
                      float* const* dW, float* const* db, float* dx, hipStream_t st, const char* primal) {
  const Geo g = geo_of(d);
  const JLayout jl = jlayout_of(d, order);
  const JvpWalk w{d, g, jl, order, x, nullptr, nullptr, dout, saved, (char*)saved, ws, primal, dW, db, dx, st};
  return w.walk(plan_jvp_backward(d, g, jl, order, dx != nullptr));
}

// The plain forward's saved buffer as the primal stream of a jvp: fp32 mode with outermost_linear only
// (its phases are then the jvp's fp32 phases; siren_mlp_forward's layout)
int jvp_primal_rule(const siren_mlp_desc* d) {
  if (d->prec != SIREN_PREC_F32) return fail(SIREN_EINVAL, "jvp primal: fp32 mode only");
  if (!d->outermost_linear) return fail(SIREN_EINVAL, "jvp primal: needs outermost_linear");
  return SIREN_OK;
}
int jvp_primal_check(const siren_mlp_desc* d, const void* primal, int64_t primal_bytes) {
  if (!primal) return SIREN_OK;
  if (int rc = jvp_primal_rule(d)) return rc;
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

int64_t siren_jvp_plan(const siren_mlp_desc* d, int order, int flags, char* out, int64_t cap) {
  if (jvp_check(d, order)) return -1;
  if ((flags & 2) && jvp_primal_rule(d)) return -1;
  const Geo g = geo_of(d);
  const JLayout jl = jlayout_of(d, order);
  return text_out(jvp_plan_text(d, jl, order, flags, plan_jvp_forward(d, g, jl, order, flags & 2),
                                plan_jvp_backward(d, g, jl, order, flags & 1)),
                  out, cap);
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
  return jvp_forward_impl(d, order, x, grad, lap, (char*)saved, (char*)workspace, (hipStream_t)stream, (const char*)primal);
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
  return jvp_backward_impl(d, order, x, dgrad, (const char*)saved, (char*)workspace, dweight, dbias, dx, (hipStream_t)stream,
                           (const char*)primal);
}

int siren_jvp_backward(const siren_mlp_desc* d, int order, const float* x, const float* dgrad,
                       const void* saved, int64_t saved_bytes, void* workspace, int64_t workspace_bytes,
                       float* const* dweight, float* const* dbias, float* dx, void* stream) {
  return siren_jvp_backward_ex(d, order, x, dgrad, saved, saved_bytes, workspace, workspace_bytes, dweight, dbias, dx,
                               nullptr, 0, stream);
}

}  // extern "C"
