// rt_encoder.hip — the conv encoder (siren_enc_*, siren_conv_*, siren_sumsq_*; kernels in
// siren_encoder.hip and siren_conv.hip). Included by siren_runtime.hip.
namespace {

// shared checks; fills the plane geometry and the block split of a [P, C] pass
int enc_setup(EncArgs& a, int64_t P, int C, void* ws, int64_t ws_bytes, bool need_ws, int64_t rows_per_block_min,
              const char* what) {
  memset(&a, 0, sizeof(a));
  if (P < 0 || C < 8 || C > ENC_MAXC || (C & (C - 1)) != 0)
    return fail(SIREN_EINVAL, "%s: C = %d must be a power of two in [8, %d] (P = %lld)", what, C, ENC_MAXC, (long long)P);
  if (need_ws && (!ws || ws_bytes < siren_enc_workspace_bytes()))
    return fail(SIREN_ENOSPACE, "%s: workspace %lld < %lld bytes", what, (long long)ws_bytes,
                (long long)siren_enc_workspace_bytes());
  a.P = P;
  a.C = C;
  a.part = (float*)ws;
  a.ticket = ws ? (unsigned*)((char*)ws + ENC_WS_FLOATS * 4) : nullptr;
  const int ppi = 256 / (C / 8);
  int64_t nblk = std::min<int64_t>(ENC_MAX_BLOCKS, std::max<int64_t>(1, cdiv(P, rows_per_block_min)));
  a.chunk = align_up(cdiv(std::max<int64_t>(P, 1), nblk), ppi);
  return SIREN_OK;
}

// conv_fwd_k5_kernel in the stage-fill form of option conv_dma
template <int EPI>
void launch_conv_fwd_k5(dim3 grid, hipStream_t st, const ConvFArgs& a) {
  if (g_conv_dma == 2) hipLaunchKernelGGL((conv_fwd_k5_kernel<EPI, 2>), grid, dim3(512), 0, st, a);
  else if (g_conv_dma == 1) hipLaunchKernelGGL((conv_fwd_k5_kernel<EPI, 1>), grid, dim3(512), 0, st, a);
  else hipLaunchKernelGGL((conv_fwd_k5_kernel<EPI, 0>), grid, dim3(512), 0, st, a);
}

// Native shapes of the generic encoder convolutions (siren_conv.hip conv_*_gen_kernel).
int conv_shape_check(int kind, int N, int H, int W, int CI, int CO, int KS) {
  if (N < 1 || H < 1) return fail(SIREN_EINVAL, "conv: empty input");
  if (KS != 3 && KS != 5 && KS != 7) return fail(SIREN_EINVAL, "conv: filter size %d not native (3, 5, 7)", KS);
  if (CI == 2) {  // conv_theta (conv_t_fwd_kernel / conv_t_wrw_kernel)
    if (CO < 32 || CO > 128 || CO % 32 != 0) return fail(SIREN_EINVAL, "conv (2 channels): %d output channels (32, 64, 96, 128)", CO);
    if (kind == 0 && W != CT_W) return fail(SIREN_EINVAL, "conv fwd (2 channels): needs W = %d (W = %d)", CT_W, W);
    if (kind != 0 && (W < CT_PX || W % CT_PX != 0)) return fail(SIREN_EINVAL, "conv wrw (2 channels): W = %d not a multiple of %d", W, CT_PX);
    return SIREN_OK;
  }
  if (CI != 64 && CI != 128) return fail(SIREN_EINVAL, "conv: %d input channels not native (2, 64, 128)", CI);
  if (kind == 0) {
    if (W != CF_W || H % 2 != 0) return fail(SIREN_EINVAL, "conv fwd: needs W = %d and H even (H = %d, W = %d)", CF_W, H, W);
    if (CO < 64 || CO % 64 != 0) return fail(SIREN_EINVAL, "conv fwd: %d output channels (a multiple of 64)", CO);
  } else {
    if (W < CW_PX || W % CW_PX != 0) return fail(SIREN_EINVAL, "conv wrw: W = %d not a multiple of %d", W, CW_PX);
    const int cow = CI == 64 ? 128 : 64;
    if (CO % cow != 0) return fail(SIREN_EINVAL, "conv wrw: %d output channels (a multiple of %d)", CO, cow);
  }
  return SIREN_OK;
}
// conv_theta weight gradient: splits of 64-pixel chunks (one workgroup each, ~3 per CU) and the
// partial slab of one split ([CO][32 NNT] floats)
int conv_t_nsplit(int N, int H, int W) {
  return (int)std::max<int64_t>(1, std::min<int64_t>(768, (int64_t)N * H * (W / CT_PX)));
}
int64_t conv_t_slab(int CO, int KS) { return (int64_t)CO * 32 * ((KS * 16 + 31) / 32); }
int conv_wrw_nsplit(int N, int H, int CI, int CO, int KS) {
  const int64_t rows = (int64_t)N * H;
  const int64_t blocks = (int64_t)KS * (CO / (CI == 64 ? 128 : 64));
  return (int)std::max<int64_t>(1, std::min<int64_t>(rows, std::max<int64_t>(1, 256 / blocks)));
}

int sumsq_setup(SumsqArgs& a, int n, const float* const* src, const int64_t* numel) {
  if (n < 1 || n > SUMSQ_MAX) return fail(SIREN_EINVAL, "sumsq: %d tensors (1..%d)", n, SUMSQ_MAX);
  if (!src || !numel) return fail(SIREN_EINVAL, "sumsq: null table");
  memset(&a, 0, sizeof(a));
  a.n = n;
  int64_t t = 0;
  for (int i = 0; i < n; ++i) {
    if (!src[i] || numel[i] < 0) return fail(SIREN_EINVAL, "sumsq: tensor %d", i);
    a.src[i] = src[i];
    a.begin[i] = t;
    t += numel[i];
  }
  a.begin[n] = t;
  return SIREN_OK;
}
}  // namespace

extern "C" {

int64_t siren_enc_workspace_bytes(void) { return ENC_WS_FLOATS * 4 + 256; }

int64_t siren_conv_wrw_workspace_bytes(int N, int H, int W) {
  const int64_t rows = (int64_t)N * H;
  const int64_t nsplit = std::max<int64_t>(1, std::min<int64_t>(25, rows));
  return nsplit * CW_SLAB * 4;
}

int siren_conv_wrw_k5(const void* x, const void* dy, int N, int H, int W, int C, float* dw, void* ws, int64_t ws_bytes,
                      void* stream) {
  if (C != CW_C || N < 1 || H < 1 || W < CW_PX || W % CW_PX != 0)
    return fail(SIREN_EINVAL, "conv_wrw_k5: needs C = %d and W a multiple of %d (C = %d, N = %d, H = %d, W = %d)", CW_C,
                CW_PX, C, N, H, W);
  if (!x || !dy || !dw) return fail(SIREN_EINVAL, "conv_wrw_k5: null pointer");
  const int64_t rows = (int64_t)N * H;
  const int nsplit = (int)std::max<int64_t>(1, std::min<int64_t>(25, rows));
  if (!ws || ws_bytes < (int64_t)nsplit * CW_SLAB * 4)
    return fail(SIREN_ENOSPACE, "conv_wrw_k5: workspace %lld < %lld bytes", (long long)ws_bytes,
                (long long)nsplit * CW_SLAB * 4);
  ConvWArgs a;
  memset(&a, 0, sizeof(a));
  a.x = (const bf16*)x;
  a.dy = (const bf16*)dy;
  a.part = (float*)ws;
  a.dw = dw;
  a.N = N;
  a.H = H;
  a.W = W;
  a.nsplit = nsplit;
  a.rows_per_split = cdiv(rows, nsplit);
  hipStream_t st = (hipStream_t)stream;
  const dim3 wg((unsigned)nsplit, CW_K, 2);
  if (g_wrw_dma >= 2 && W % (2 * CW_PX) == 0) hipLaunchKernelGGL((conv_wrw_k5_kernel<true, 2 * CW_PX>), wg, dim3(512), 0, st, a);
  else if (g_wrw_dma) hipLaunchKernelGGL((conv_wrw_k5_kernel<true>), wg, dim3(512), 0, st, a);
  else hipLaunchKernelGGL((conv_wrw_k5_kernel<false>), wg, dim3(512), 0, st, a);
  int rc = check_launch("conv_wrw_k5");
  if (rc) return rc;
  hipLaunchKernelGGL(conv_wrw_reduce_kernel, dim3((unsigned)cdiv(CW_SLAB, 256)), dim3(256), 0, st, a);
  return check_launch("conv_wrw_reduce");
}

int siren_conv_fwd_k5(const void* x, const void* w, const void* bias, int relu, void* y, int N, int H, int W, int C,
                      void* stream) {
  if (C != CW_C || W != CF_W || N < 1 || H < 2 || H % 2 != 0)
    return fail(SIREN_EINVAL, "conv_fwd_k5: needs C = %d, W = %d and H even (C = %d, N = %d, H = %d, W = %d)", CW_C,
                CF_W, C, N, H, W);
  if (!x || !w || !y) return fail(SIREN_EINVAL, "conv_fwd_k5: null pointer");
  if (relu && !bias) return fail(SIREN_EINVAL, "conv_fwd_k5: relu needs a bias (the ReLU is part of the bias epilogue)");
  ConvFArgs a;
  memset(&a, 0, sizeof(a));
  a.x = (const bf16*)x;
  a.w = (const bf16*)w;
  a.bias = (const bf16*)bias;
  a.y = (bf16*)y;
  a.N = N;
  a.H = H;
  a.relu = relu ? 1 : 0;
  launch_conv_fwd_k5<EPI_PLAIN>(dim3((unsigned)(N * (H / 2))), (hipStream_t)stream, a);
  return check_launch("conv_fwd_k5");
}

int siren_conv_fwd_k5_res(const void* x, const void* w, const void* cb, const void* t, void* a_out, void* out, int N,
                          int H, int W, int C, void* stream) {
  if (C != CW_C || W != CF_W || N < 1 || H < 2 || H % 2 != 0)
    return fail(SIREN_EINVAL, "conv_fwd_k5_res: needs C = %d, W = %d and H even (C = %d, N = %d, H = %d, W = %d)", CW_C,
                CF_W, C, N, H, W);
  if (!x || !w || !cb || !t || !a_out || !out) return fail(SIREN_EINVAL, "conv_fwd_k5_res: null pointer");
  ConvFArgs a;
  memset(&a, 0, sizeof(a));
  a.x = (const bf16*)x;
  a.w = (const bf16*)w;
  a.y = (bf16*)a_out;
  a.N = N;
  a.H = H;
  a.g2 = (const bf16*)t;
  a.cb = (const bf16*)cb;
  a.y2 = (bf16*)out;
  launch_conv_fwd_k5<EPI_RESFWD>(dim3((unsigned)(N * (H / 2))), (hipStream_t)stream, a);
  return check_launch("conv_fwd_k5_res");
}

int siren_conv_dgrad_k5_fused(int mode, const void* dy, const void* wf, const void* g2, const void* m, const void* pa,
                              const void* cb, void* out, void* out2, float* db, int N, int H, int W, int C, void* ws,
                              int64_t ws_bytes, void* stream) {
  if (C != CW_C || W != CF_W || N < 1 || H < 2 || H % 2 != 0)
    return fail(SIREN_EINVAL, "conv_dgrad_k5_fused: needs C = %d, W = %d and H even (C = %d, N = %d, H = %d, W = %d)",
                CW_C, CF_W, C, N, H, W);
  if (mode != 1 && mode != 2) return fail(SIREN_EINVAL, "conv_dgrad_k5_fused: mode %d (1 relu, 2 residual tail)", mode);
  if (!dy || !wf || !m || !out || !db || (mode == 2 && (!g2 || !pa || !cb || !out2)))
    return fail(SIREN_EINVAL, "conv_dgrad_k5_fused: null pointer");
  const int64_t nblk = (int64_t)N * (H / 2);
  if (!ws || ws_bytes < nblk * CW_C * 4)
    return fail(SIREN_ENOSPACE, "conv_dgrad_k5_fused: workspace %lld < %lld bytes", (long long)ws_bytes,
                (long long)(nblk * CW_C * 4));
  ConvFArgs a;
  memset(&a, 0, sizeof(a));
  a.x = (const bf16*)dy;
  a.w = (const bf16*)wf;
  a.y = (bf16*)out;
  a.N = N;
  a.H = H;
  a.g2 = (const bf16*)g2;
  a.m = (const bf16*)m;
  a.pa = (const bf16*)pa;
  a.cb = (const bf16*)cb;
  a.y2 = (bf16*)out2;
  a.part = (float*)ws;
  hipStream_t st = (hipStream_t)stream;
  if (mode == 1) {
    launch_conv_fwd_k5<EPI_RELU>(dim3((unsigned)nblk), st, a);
  } else {
    launch_conv_fwd_k5<EPI_RES>(dim3((unsigned)nblk), st, a);
  }
  int rc = check_launch("conv_dgrad_k5_fused");
  if (rc) return rc;
  hipLaunchKernelGGL(conv_chan_reduce_kernel, dim3(CW_C), dim3(256), 0, st, (const float*)ws, (int)nblk, db);
  return check_launch("conv_chan_reduce");
}

int siren_conv_check(int kind, int N, int H, int W, int CI, int CO, int KS) {
  return conv_shape_check(kind, N, H, W, CI, CO, KS);
}

int siren_conv_fwd(const void* x, const void* w, const void* bias, int relu, void* y, int N, int H, int W, int CI,
                   int CO, int KS, void* stream) {
  int rc = conv_shape_check(0, N, H, W, CI, CO, KS);
  if (rc) return rc;
  if (!x || !w || !y) return fail(SIREN_EINVAL, "conv fwd: null pointer");
  if (relu && !bias) return fail(SIREN_EINVAL, "conv fwd: relu needs a bias (the ReLU is part of the bias epilogue)");
  ConvGArgs a;
  memset(&a, 0, sizeof(a));
  a.x = (const bf16*)x;
  a.w = (const bf16*)w;
  a.bias = (const bf16*)bias;
  a.y = (bf16*)y;
  a.N = N;
  a.H = H;
  a.W = W;
  a.CO = CO;
  a.relu = relu ? 1 : 0;
  hipStream_t st = (hipStream_t)stream;
  if (CI == 2) {
    ConvTArgs t;
    memset(&t, 0, sizeof(t));
    t.x = a.x;
    t.w = a.w;
    t.bias = a.bias;
    t.y = a.y;
    t.N = N;
    t.H = H;
    t.W = W;
    t.CO = CO;
    t.relu = a.relu;
    t.rows_per_block = CT_RPB;
    const dim3 tg((unsigned)cdiv((int64_t)N * H, CT_RPB));
#define SIREN_CT(K)                                                                              \
  switch (CO / 32) {                                                                             \
    case 1: hipLaunchKernelGGL((conv_t_fwd_kernel<K, 1>), tg, dim3(256), 0, st, t); break;      \
    case 2: hipLaunchKernelGGL((conv_t_fwd_kernel<K, 2>), tg, dim3(256), 0, st, t); break;      \
    case 3: hipLaunchKernelGGL((conv_t_fwd_kernel<K, 3>), tg, dim3(256), 0, st, t); break;      \
    default: hipLaunchKernelGGL((conv_t_fwd_kernel<K, 4>), tg, dim3(256), 0, st, t); break;     \
  }
    if (KS == 3) { SIREN_CT(3) }
    else if (KS == 5) { SIREN_CT(5) }
    else { SIREN_CT(7) }
#undef SIREN_CT
    return check_launch("conv_t_fwd");
  }
  const bool big = KS <= 5 && CO % 128 == 0;  // 128-channel tiles (the 7x7 stages need 64 to fit in LDS)
  const dim3 grid((unsigned)(N * (H / 2)), (unsigned)(CO / (big ? 128 : 64)));
#define SIREN_CF(K, C, T)                                                                           \
  do {                                                                                              \
    if (g_conv_dma == 2) hipLaunchKernelGGL((conv_fwd_gen_kernel<K, C, T, true>), grid, dim3(512), 0, st, a); \
    else hipLaunchKernelGGL((conv_fwd_gen_kernel<K, C, T, false>), grid, dim3(512), 0, st, a);      \
  } while (0)
  if (KS == 3) {
    if (CI == 64) { if (big) SIREN_CF(3, 64, 128); else SIREN_CF(3, 64, 64); }
    else { if (big) SIREN_CF(3, 128, 128); else SIREN_CF(3, 128, 64); }
  } else if (KS == 5) {
    if (CI == 64) { if (big) SIREN_CF(5, 64, 128); else SIREN_CF(5, 64, 64); }
    else { if (big) SIREN_CF(5, 128, 128); else SIREN_CF(5, 128, 64); }
  } else {
    if (CI == 64) SIREN_CF(7, 64, 64);
    else SIREN_CF(7, 128, 64);
  }
#undef SIREN_CF
  return check_launch("conv_fwd_gen");
}

int64_t siren_conv_wrw_ws_bytes(int N, int H, int W, int CI, int CO, int KS) {
  if (conv_shape_check(1, N, H, W, CI, CO, KS)) return -1;
  if (CI == 2) return (int64_t)conv_t_nsplit(N, H, W) * conv_t_slab(CO, KS) * 4;
  return (int64_t)conv_wrw_nsplit(N, H, CI, CO, KS) * KS * KS * CO * CI * 4;
}

int siren_conv_wrw(const void* x, const void* dy, int N, int H, int W, int CI, int CO, int KS, float* dw, void* ws,
                   int64_t ws_bytes, void* stream) {
  int rc = conv_shape_check(1, N, H, W, CI, CO, KS);
  if (rc) return rc;
  if (!x || !dy || !dw) return fail(SIREN_EINVAL, "conv wrw: null pointer");
  if (CI == 2) {
    const int ns = conv_t_nsplit(N, H, W);
    const int64_t need = (int64_t)ns * conv_t_slab(CO, KS) * 4;
    if (!ws || ws_bytes < need) return fail(SIREN_ENOSPACE, "conv wrw: workspace %lld < %lld bytes", (long long)ws_bytes, (long long)need);
    ConvTArgs t;
    memset(&t, 0, sizeof(t));
    t.x = (const bf16*)x;
    t.dy = (const bf16*)dy;
    t.part = (float*)ws;
    t.dw = dw;
    t.N = N;
    t.H = H;
    t.W = W;
    t.CO = CO;
    t.nsplit = ns;
    t.chunks_per_split = cdiv((int64_t)N * H * (W / CT_PX), ns);
    hipStream_t st = (hipStream_t)stream;
    const dim3 rg((unsigned)cdiv((int64_t)CO * KS * KS * 2, 16));
#define SIREN_CTW(K)                                                                               \
  {                                                                                                \
    switch (CO / 32) {                                                                             \
      case 1: hipLaunchKernelGGL((conv_t_wrw_kernel<K, 1>), dim3(ns), dim3(256), 0, st, t); break; \
      case 2: hipLaunchKernelGGL((conv_t_wrw_kernel<K, 2>), dim3(ns), dim3(256), 0, st, t); break; \
      case 3: hipLaunchKernelGGL((conv_t_wrw_kernel<K, 3>), dim3(ns), dim3(256), 0, st, t); break; \
      default: hipLaunchKernelGGL((conv_t_wrw_kernel<K, 4>), dim3(ns), dim3(256), 0, st, t); break; \
    }                                                                                              \
    if ((rc = check_launch("conv_t_wrw"))) return rc;                                              \
    hipLaunchKernelGGL((conv_t_wrw_reduce_kernel<K>), rg, dim3(256), 0, st, t);                    \
  }
    if (KS == 3) SIREN_CTW(3)
    else if (KS == 5) SIREN_CTW(5)
    else SIREN_CTW(7)
#undef SIREN_CTW
    return check_launch("conv_t_wrw_reduce");
  }
  const int nsplit = conv_wrw_nsplit(N, H, CI, CO, KS);
  const int64_t need = (int64_t)nsplit * KS * KS * CO * CI * 4;
  if (!ws || ws_bytes < need) return fail(SIREN_ENOSPACE, "conv wrw: workspace %lld < %lld bytes", (long long)ws_bytes, (long long)need);
  ConvGArgs a;
  memset(&a, 0, sizeof(a));
  a.x = (const bf16*)x;
  a.dy = (const bf16*)dy;
  a.part = (float*)ws;
  a.dw = dw;
  a.N = N;
  a.H = H;
  a.W = W;
  a.CO = CO;
  a.nsplit = nsplit;
  a.rows_per_split = cdiv((int64_t)N * H, nsplit);
  hipStream_t st = (hipStream_t)stream;
  const int cow = CI == 64 ? 128 : 64;
  const dim3 grid((unsigned)nsplit, (unsigned)KS, (unsigned)(CO / cow));
  const int64_t slab = (int64_t)KS * KS * CO * CI;
  const dim3 rgrid((unsigned)cdiv(slab, 256));
#define SIREN_CW(K, C, B)                                                               \
  {                                                                                      \
    if (g_wrw_dma == 3 && W % 128 == 0)                                                  \
      hipLaunchKernelGGL((conv_wrw_gen_kernel<K, C, B, true>), grid, dim3(512), 0, st, a); \
    else                                                                                 \
      hipLaunchKernelGGL((conv_wrw_gen_kernel<K, C, B>), grid, dim3(512), 0, st, a);      \
    if ((rc = check_launch("conv_wrw_gen"))) return rc;                                  \
    hipLaunchKernelGGL((conv_wrw_gen_reduce_kernel<K, C>), rgrid, dim3(256), 0, st, a);   \
  }
  if (KS == 3) { if (CI == 64) SIREN_CW(3, 64, 4) else SIREN_CW(3, 128, 2) }
  else if (KS == 5) { if (CI == 64) SIREN_CW(5, 64, 4) else SIREN_CW(5, 128, 2) }
  else { if (CI == 64) SIREN_CW(7, 64, 4) else SIREN_CW(7, 128, 2) }
#undef SIREN_CW
  return check_launch("conv_wrw_gen_reduce");
}

int64_t siren_sumsq_workspace_bytes(int64_t total) {
  return 256 + (int64_t)std::max<int64_t>(1, cdiv(total, SUMSQ_CHUNK)) * 4;
}

int siren_sumsq_forward(int n, const float* const* src, const int64_t* numel, float* out, void* ws, int64_t ws_bytes,
                        void* stream) {
  SumsqArgs a;
  int rc = sumsq_setup(a, n, src, numel);
  if (rc) return rc;
  if (!out || !ws || ws_bytes < siren_sumsq_workspace_bytes(a.begin[n]))
    return fail(SIREN_ENOSPACE, "sumsq: workspace (zeroed, siren_sumsq_workspace_bytes) missing or small");
  a.counter = (unsigned*)ws;
  a.part = (float*)((char*)ws + 256);
  a.out = out;
  const int64_t nb = std::max<int64_t>(1, cdiv(a.begin[n], SUMSQ_CHUNK));
  hipLaunchKernelGGL(sumsq_fwd_kernel, dim3((unsigned)nb), dim3(256), 0, (hipStream_t)stream, a);
  return check_launch("sumsq_fwd");
}

int siren_sumsq_backward(int n, const float* const* src, const int64_t* numel, const float* g, float* const* dst,
                         void* stream) {
  SumsqArgs a;
  int rc = sumsq_setup(a, n, src, numel);
  if (rc) return rc;
  if (!g || !dst) return fail(SIREN_EINVAL, "sumsq backward: null argument");
  for (int i = 0; i < n; ++i) {
    if (!dst[i]) return fail(SIREN_EINVAL, "sumsq backward: null output %d", i);
    a.dst[i] = dst[i];
  }
  a.g = g;
  if (a.begin[n] == 0) return SIREN_OK;
  hipLaunchKernelGGL(sumsq_bwd_kernel, dim3((unsigned)cdiv(a.begin[n], 256)), dim3(256), 0, (hipStream_t)stream, a);
  return check_launch("sumsq_bwd");
}

int siren_enc_prep(int n, const float* const* w, const float* const* b, const int64_t* geom, void* const* wb,
                   void* const* wf, void* const* bb, void* stream) {
  if (n < 1 || n > ENC_PREP_MAX) return fail(SIREN_EINVAL, "enc_prep: %d filters (1..%d)", n, ENC_PREP_MAX);
  if (!w || !geom || !wb) return fail(SIREN_EINVAL, "enc_prep: null table");
  EncPrepArgs a;
  memset(&a, 0, sizeof(a));
  a.nseg = n;
  int64_t t = 0;
  for (int i = 0; i < n; ++i) {
    EncPrepSeg& g = a.seg[i];
    const int64_t* q = geom + 7 * i;
    g.co = (int)q[0];
    g.ci = (int)q[1];
    g.k = (int)q[2];
    g.s_co = q[3];
    g.s_ci = q[4];
    g.s_kh = q[5];
    g.s_kw = q[6];
    if (g.co < 1 || g.ci < 1 || g.k < 1) return fail(SIREN_EINVAL, "enc_prep: filter %d shape", i);
    g.w = w[i];
    g.b = b ? b[i] : nullptr;
    g.wb = (bf16*)wb[i];
    g.wf = wf ? (bf16*)wf[i] : nullptr;
    g.bb = bb ? (bf16*)bb[i] : nullptr;
    if (!g.w || !g.wb || (g.bb && !g.b)) return fail(SIREN_EINVAL, "enc_prep: filter %d null pointer", i);
    g.begin = t;
    t += (int64_t)g.co * g.ci * g.k * g.k + (g.bb ? g.co : 0);
  }
  a.total = t;
  hipLaunchKernelGGL(enc_prep_kernel, dim3((unsigned)cdiv(t, 256)), dim3(256), 0, (hipStream_t)stream, a);
  return check_launch("enc_prep");
}

int siren_enc_relu_bwd(const void* g1, const void* g2, const void* y, void* out, float* db, int64_t P, int C, void* ws,
                       int64_t ws_bytes, void* stream) {
  EncArgs a;
  int rc = enc_setup(a, P, C, ws, ws_bytes, db != nullptr, 512, "enc_relu_bwd");
  if (rc) return rc;
  if (!g1 || !y || !out) return fail(SIREN_EINVAL, "enc_relu_bwd: null plane");
  if (P == 0) return SIREN_OK;
  a.g1 = (const bf16*)g1;
  a.g2 = (const bf16*)g2;
  a.y = (const bf16*)y;
  a.out = (bf16*)out;
  a.db = db;
  hipLaunchKernelGGL(enc_relu_bwd_kernel, dim3((unsigned)cdiv(P, a.chunk)), dim3(256), 0, (hipStream_t)stream, a);
  return check_launch("enc_relu_bwd");
}

int siren_enc_bias_relu(void* y, const void* cb, int64_t P, int C, void* stream) {
  EncArgs a;
  int rc = enc_setup(a, P, C, nullptr, 0, false, 512, "enc_bias_relu");
  if (rc) return rc;
  if (!y) return fail(SIREN_EINVAL, "enc_bias_relu: null plane");
  if (P == 0) return SIREN_OK;
  a.out = (bf16*)y;
  a.cb = (const bf16*)cb;
  hipLaunchKernelGGL(enc_bias_relu_kernel, dim3((unsigned)std::min<int64_t>(cdiv(P * C / 8, 256), 8192)), dim3(256), 0,
                     (hipStream_t)stream, a);
  return check_launch("enc_bias_relu");
}

int siren_enc_res_fwd(const void* a_pre, const void* cb, const void* x, void* out, int64_t P, int C, void* stream) {
  EncArgs a;
  int rc = enc_setup(a, P, C, nullptr, 0, false, 512, "enc_res_fwd");
  if (rc) return rc;
  if (!a_pre || !x || !out) return fail(SIREN_EINVAL, "enc_res_fwd: null plane");
  if (P == 0) return SIREN_OK;
  a.cb = (const bf16*)cb;
  a.a = (const bf16*)a_pre;
  a.g1 = (const bf16*)x;
  a.out = (bf16*)out;
  hipLaunchKernelGGL(enc_res_fwd_kernel, dim3((unsigned)std::min<int64_t>(cdiv(P * C / 8, 256), 8192)), dim3(256), 0,
                     (hipStream_t)stream, a);
  return check_launch("enc_res_fwd");
}

int siren_enc_res_bwd(const void* g1, const void* g2, const void* out, const void* a_pre, const void* cb, void* gskip,
                      void* ga, float* db, int64_t P, int C, void* ws, int64_t ws_bytes, void* stream) {
  EncArgs a;
  int rc = enc_setup(a, P, C, ws, ws_bytes, db != nullptr, 512, "enc_res_bwd");
  if (rc) return rc;
  if (!g1 || !out || !a_pre || !gskip || !ga) return fail(SIREN_EINVAL, "enc_res_bwd: null plane");
  if (P == 0) return SIREN_OK;
  a.g1 = (const bf16*)g1;
  a.g2 = (const bf16*)g2;
  a.y = (const bf16*)out;
  a.a = (const bf16*)a_pre;
  a.cb = (const bf16*)cb;
  a.out = (bf16*)gskip;
  a.out2 = (bf16*)ga;
  a.db = db;
  hipLaunchKernelGGL(enc_res_bwd_kernel, dim3((unsigned)cdiv(P, a.chunk)), dim3(256), 0, (hipStream_t)stream, a);
  return check_launch("enc_res_bwd");
}

int siren_enc_pixfc_fwd(const void* a_pre, const void* cb, const float* w, const float* bias, float* e, int B,
                        int64_t P, int C, void* ws, int64_t ws_bytes, void* stream) {
  EncArgs a;
  // chunks of >= 512 pixels, at most ENC_MAX_BLOCKS blocks over the B images (32 x 32 at C4's 128^2)
  const int64_t min_rows = std::max<int64_t>(512, cdiv(std::max<int64_t>(P, 1), std::max<int64_t>(1, ENC_MAX_BLOCKS / std::max(B, 1))));
  int rc = enc_setup(a, P, C, ws, ws_bytes, true, min_rows, "enc_pixfc_fwd");
  if (rc) return rc;
  if (!a_pre || !w || !bias || !e || B < 1) return fail(SIREN_EINVAL, "enc_pixfc_fwd: null pointer or B < 1");
  const int64_t nchunk = cdiv(P, a.chunk);
  if (nchunk * B > ENC_MAX_BLOCKS || (int64_t)B * C > ENC_WS_FLOATS)
    return fail(SIREN_EINVAL, "enc_pixfc_fwd: %lld blocks > %d", (long long)(nchunk * B), ENC_MAX_BLOCKS);
  if (P == 0) return fail(SIREN_EINVAL, "enc_pixfc_fwd: no pixels");
  a.a = (const bf16*)a_pre;
  a.cb = (const bf16*)cb;
  a.w = w;
  a.bias = bias;
  a.e = e;
  a.B = B;
  hipLaunchKernelGGL(enc_pixfc_fwd_kernel, dim3((unsigned)nchunk, (unsigned)B), dim3(256), 0, (hipStream_t)stream, a);
  return check_launch("enc_pixfc_fwd");
}

int siren_enc_pixfc_bwd(const float* g, const void* a_pre, const void* cb, const float* w, void* ga, float* db,
                        float* gw, int B, int64_t P, int C, void* ws, int64_t ws_bytes, void* stream) {
  EncArgs a;
  int rc = enc_setup(a, P, C, ws, ws_bytes, true, 32, "enc_pixfc_bwd");  // 512 blocks at 128^2 (128: 177 us, C4)
  if (rc) return rc;
  if (!g || !a_pre || !w || !ga || !db || !gw || B < 1) return fail(SIREN_EINVAL, "enc_pixfc_bwd: null pointer or B < 1");
  if (P == 0) return fail(SIREN_EINVAL, "enc_pixfc_bwd: no pixels");
  a.gin = g;
  a.a = (const bf16*)a_pre;
  a.cb = (const bf16*)cb;
  a.w = w;
  a.out = (bf16*)ga;
  a.db = db;
  a.e = gw;
  a.B = B;
  hipLaunchKernelGGL(enc_pixfc_bwd_kernel, dim3((unsigned)cdiv(P, a.chunk)), dim3(256), 0, (hipStream_t)stream, a);
  return check_launch("enc_pixfc_bwd");
}

}  // extern "C"
