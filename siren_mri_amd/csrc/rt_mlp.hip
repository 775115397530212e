// rt_mlp.hip — the SIREN layer stack: buffer layout, weight preparation and the launch plan of the
// forward and the backward pass. Its entry points are in rt_mlp_entry.hip. Included by siren_runtime.hip.
namespace {

constexpr int kTargetBlocks = 1024;  // ~4 workgroups per CU on 256 CUs

// Wide inputs (in_features > 16: Fourier-feature coordinates) run layer 0 on the MFMA GEMM path;
// its prepared weights are zero-padded along K to a whole number of MFMA K-steps (16 bf16 / 4 f32).
constexpr int kValuMaxIn = 16;
inline bool wide_input(const siren_mlp_desc* d) { return d->dims[0] > kValuMaxIn; }
inline int first_kp(const siren_mlp_desc* d) {
  return (int)align_up(d->dims[0], d->prec == SIREN_PREC_BF16 ? 16 : 4);
}

// Wide first layer (5..16 inputs: Fourier features): the register-resident forward only, with at
// most FREG_WIDE_MAXH hidden layers; P_0 is kept (the layer-1 backward reads it).
bool fused_wide(const siren_mlp_desc* d) { return d->dims[0] > FUSED_MAXC && d->dims[0] <= 16; }
// Shapes the single-kernel forward (siren_fused.hip) covers: bf16, 1..4 inputs, 1..8 outputs,
// every hidden width 256, up to FUSED_MAXH hidden MFMA layers.
bool fused_shape(const siren_mlp_desc* d) {
  if (d->prec != SIREN_PREC_BF16) return false;
  if (d->dims[d->num_layers] > FUSED_MAXO) return false;
  if (fused_wide(d)) {
    if (!g_fwd_reg || d->num_layers - 2 < 1 || d->num_layers - 2 > FREG_WIDE_MAXH) return false;
  } else if (d->dims[0] > FUSED_MAXC) {
    return false;
  }
  const int F = d->dims[1];
  if (F != 256) return false;
  for (int l = 1; l < d->num_layers; ++l)
    if (d->dims[l] != F) return false;
  return d->num_layers - 2 <= FUSED_MAXH;
}

// bf16 stacks of the fused/ring shapes do not keep P_0: the layer-1 ring kernels recompute it from
// x (C <= 4 inputs) — 2 B per row-feature less written by the forward and read twice by the
// backward. Decided from the descriptor alone, so forward and backward always agree.
// Every row count qualifies: x moves by LDS-DMA through buffer resources whose bounds are checked
// per dword (a 16-byte piece straddling the end loads its valid dwords and zeros,
// tools/probe_lds_oob.hip) and whose base may sit 8 bytes past a 16-byte boundary (a weight set's x
// rows when rows_per_batch x C is not a multiple of 4; the forward reads x the same way). Keeping
// P_0 instead (the round-2 rule for such shapes) made the register-resident forward's layer-0
// phase-code stores differ from run to run in a few words (tools/det_saved.py), so the stored-P_0
// path is no longer taken by fused shapes.
bool p0_recompute(const siren_mlp_desc* d) {
  if (g_keep_p0 || !fused_shape(d) || fused_wide(d) || d->num_layers < 3) return false;
  const int64_t C = d->dims[0], total = d->batch * d->rows_per_batch;
  return total * C >= 1;
}

int max_hidden(const siren_mlp_desc* d) {
  int m = 0;
  for (int l = 1; l < d->num_layers; ++l) m = std::max(m, d->dims[l]);
  return m;
}

// Split-K geometry of the weight-gradient reductions.
struct Split {
  int64_t nsplit, rows_per_split;
};
Split split_rows(int64_t rows, int64_t blocks_per_split, int64_t nb, int64_t granule) {
  int64_t want = std::max<int64_t>(1, kTargetBlocks / std::max<int64_t>(1, blocks_per_split * nb));
  int64_t rps = align_up(cdiv(rows, want), granule);
  rps = std::max<int64_t>(rps, granule);
  Split s;
  s.rows_per_split = rps;
  s.nsplit = std::max<int64_t>(1, cdiv(rows, rps));
  return s;
}

Split tn_split(const Geo& g, int M, int N) {
  const int64_t tiles = cdiv(M, TN_BM) * cdiv(N, TN_BN);
  return split_rows(g.rows, tiles, g.nb, 64);
}
Split valu_split(const Geo& g) { return split_rows(g.rows, 1, g.nb, 64); }
// dw_ring_bf16_kernel: one workgroup per CU, each a contiguous row range of one weight set
Split dw_ring_split(const Geo& g) {
  const int64_t want = std::max<int64_t>(1, 256 / g.nb);
  Split s;
  s.rows_per_split = std::max<int64_t>(32, align_up(cdiv(g.rows, want), 32));
  s.nsplit = std::max<int64_t>(1, cdiv(g.rows, s.rows_per_split));
  return s;
}

// Distance between consecutive split slabs (all weight sets of one split), padded to float4.
int64_t split_stride(const Geo& g, int64_t slab) { return align_up(g.nb * slab, 4); }

// pair_ring_bf16_kernel: npair input-gradient / weight-gradient workgroup pairs per weight set
// (a multiple of 8, so the grid is a multiple of 16 and every pair shares an XCD); with nb <= 16
// weight sets all 2 * npair * nb workgroups are resident together (one per CU). Past that (configs
// 4/5: 32 slices, 512 workgroups) the two workgroups of a pair are still dispatched next to each
// other (speed only; correctness never depends on residency).
constexpr int64_t kMaxPairs = 128;
bool pair_ok(const Geo& g) { return g.nb <= 64; }
int64_t pair_count(const Geo& g) {
  const int64_t ntiles = cdiv(g.rows, 32);
  const int64_t np = std::max<int64_t>(8, (kMaxPairs / g.nb) / 8 * 8);
  return std::min<int64_t>(np, align_up(ntiles, 8));
}

// rt_jvp.hip's all-rows weight-gradient tile, which the fp32 backward and its workspace size use too
Split jtn2_split(const Geo& g, int64_t stacked_rows, int N);
bool jvp_tn2_ok(int M, int N);

struct Layout {
  // saved
  int64_t saved_off[SIREN_MAX_LAYERS];
  int64_t saved_bytes;
  // workspace
  int64_t w_op_off[SIREN_MAX_LAYERS];
  int64_t wt_op_off[SIREN_MAX_LAYERS];
  int64_t pp_off[2];     // phase ping-pong (forward without saved buffer)
  int64_t dz_off[2];     // dZ ping-pong
  int64_t part_off;
  int64_t partL_off;      // output-layer partial slabs of the fused top backward layer
  int64_t partB_off;      // first-layer partial slabs of the paired bottom layer (P_0 recompute)
  int64_t part2_off;      // second slab buffer of consecutive pair launches (-1: none)
  int64_t xcopy_off;      // 16-byte aligned copy of x (P_0 recompute with a misaligned x)
  bool p0_rec;
  int64_t ws_bytes;
  int64_t weights_bytes;  // prepared MFMA weights (front of `saved`, or of the workspace)
  int64_t frag_off;       // fused-forward fragment-order hidden weights (-1: shape not eligible)
};

Layout layout_of(const siren_mlp_desc* d) {
  const Geo g = geo_of(d);
  Layout lo;
  memset(&lo, 0, sizeof(lo));
  // saved = [prepared MFMA weights][one phase tensor per sine layer 0..L-2]
  int64_t off = 0;
  for (int l = 0; l < SIREN_MAX_LAYERS; ++l) lo.w_op_off[l] = lo.wt_op_off[l] = -1;
  if (wide_input(d)) {
    lo.w_op_off[0] = off;
    off = align_up(off + g.nb * (int64_t)d->dims[1] * first_kp(d) * g.op_sz, 256);
    lo.wt_op_off[0] = off;
    off = align_up(off + g.nb * (int64_t)d->dims[1] * d->dims[0] * g.op_sz, 256);
  }
  for (int l = 1; l + 1 < g.L; ++l) {
    const int64_t n = g.nb * (int64_t)d->dims[l + 1] * d->dims[l];
    if (g.prec == SIREN_PREC_BF16) {
      lo.w_op_off[l] = off;
      off = align_up(off + n * g.op_sz, 256);
    } else {
      lo.w_op_off[l] = -1;
    }
    lo.wt_op_off[l] = off;
    off = align_up(off + n * g.op_sz, 256);
  }
  lo.frag_off = -1;
  if (fused_shape(d) && g.L > 2) {
    // hidden-layer fragments, then (register-resident forward) the output-layer fragments
    lo.frag_off = off;
    // + the rows' weight bounds of the forward's magic-form check ([nb][L - 2][F] f32)
    off = align_up(off + g.nb * ((int64_t)(g.L - 2) * d->dims[1] * d->dims[1] + FREG_WL_BYTES / 2) * 2 +
                       g.nb * (int64_t)(g.L - 2) * d->dims[1] * 4, 256);
  }
  lo.weights_bytes = off;
  lo.p0_rec = p0_recompute(d);
  for (int l = 0; l + 1 < g.L; ++l) {
    if (l == 0 && lo.p0_rec) {
      lo.saved_off[0] = -1;
      continue;
    }
    lo.saved_off[l] = off;
    off = align_up(off + g.total * d->dims[l + 1] * g.phase_sz, 256);
  }
  lo.saved_bytes = off;

  // workspace = [prepared weights when no saved buffer][phase ping-pong][dZ ping-pong][partials]
  off = align_up(lo.weights_bytes, 256);
  const int64_t act = g.total * (int64_t)max_hidden(d);
  for (int k = 0; k < 2; ++k) {
    lo.pp_off[k] = off;
    off = align_up(off + act * g.phase_sz, 256);
  }
  for (int k = 0; k < 2; ++k) {
    lo.dz_off[k] = off;
    off = align_up(off + act * g.grad_sz, 256);
  }
  int64_t part = 0;
  for (int l = 1; l + 1 < g.L; ++l) {
    const int M = d->dims[l + 1], N = d->dims[l];
    const Split s = tn_split(g, M, N);
    part = std::max(part, s.nsplit * split_stride(g, (int64_t)M * N + M));
    part = std::max(part, dw_ring_split(g).nsplit * split_stride(g, (int64_t)M * N + M));
    part = std::max(part, pair_count(g) * split_stride(g, (int64_t)M * N + M));
    part = std::max(part, jtn2_split(g, g.rows, N).nsplit * split_stride(g, (int64_t)M * N + M));
  }
  {
    const Split s = valu_split(g);
    const int F = d->dims[g.L - 1], O = d->dims[g.L];
    part = std::max(part, s.nsplit * split_stride(g, (int64_t)O * F + O));
    const int F0 = d->dims[1], C = d->dims[0];
    const Split s0 = wide_input(d) ? tn_split(g, F0, C) : s;
    part = std::max(part, s0.nsplit * split_stride(g, (int64_t)F0 * C + F0));
    // fused bottom layer: one first-layer slab per input-gradient workgroup (<= 256)
    part = std::max(part, (int64_t)256 * split_stride(g, (int64_t)F0 * C + F0));
  }
  lo.part_off = off;
  off = align_up(off + part * 4, 256);
  lo.partL_off = off;
  if (g.L >= 3) {
    const int F = d->dims[g.L - 1], O = d->dims[g.L];
    const int64_t ns = std::max(std::max(tn_split(g, F, d->dims[g.L - 2]).nsplit, dw_ring_split(g).nsplit),
                                pair_count(g));
    off = align_up(off + ns * split_stride(g, (int64_t)O * F + O) * 4, 256);
  }
  lo.partB_off = off;
  // (the bottom pair's input-gradient role: one first-layer slab per pair)
  if (lo.p0_rec) off = align_up(off + kMaxPairs * split_stride(g, (int64_t)d->dims[1] * d->dims[0] + d->dims[1]) * 4, 256);
  lo.xcopy_off = off;
  if (lo.p0_rec) off = align_up(off + g.total * d->dims[0] * 4, 256);
  // paired 256x256 layers alternate between part and part2: a pair launch reduces the previous
  // one's slabs in its weight-gradient role's tail (pair_ring_bf16_kernel)
  lo.part2_off = -1;
  if (fused_shape(d) && g.L >= 4) {
    lo.part2_off = off;
    off = align_up(off + pair_count(g) * split_stride(g, (int64_t)256 * 256 + 256) * 4, 256);
  }
  lo.ws_bytes = off;
  return lo;
}

int launch_reduce(const float* part, int64_t nsplit, int64_t sstride, int64_t nb, int64_t slab,
                  int64_t n_first, float* out0, float* out1, hipStream_t st) {
  const int64_t total = nb * slab;
  hipLaunchKernelGGL(reduce_kernel, dim3((unsigned)cdiv(total, 128)), dim3(256), 0, st, part,
                     (int)nsplit, sstride, (int)total, (int)slab, (int)n_first, out0, out1);
  return check_launch("reduce");
}

// Up to REDUCE_MAXSEG reductions (same arguments as launch_reduce) in one launch.
struct ReduceList {
  ReduceMultiArgs a;
  int64_t blocks = 0;
  ReduceList() { memset(&a, 0, sizeof(a)); }
  void add(const float* part, int64_t nsplit, int64_t sstride, int64_t nb, int64_t slab, int64_t n_first, float* out0,
           float* out1) {
    ReduceSeg& g = a.seg[a.nseg++];
    g.part = part;
    g.nsplit = (int)nsplit;
    g.split_stride = sstride;
    g.total = (int)(nb * slab);
    g.slab = (int)slab;
    g.n_first = (int)n_first;
    g.out0 = out0;
    g.out1 = out1;
    g.blocks = (int)cdiv(nb * slab, 128);
    blocks += g.blocks;
  }
  int launch(hipStream_t st) {
    if (a.nseg == 0) return SIREN_OK;
    hipLaunchKernelGGL(reduce_multi_kernel, dim3((unsigned)blocks), dim3(256), 0, st, a);
    return check_launch("reduce_multi");
  }
};

// Convert every MFMA layer's weights (bf16 copy + transpose) into `dst` in one launch.
template <int PREC>
int prep_weights(const siren_mlp_desc* d, const Geo& g, const Layout& lo, char* dst, hipStream_t st) {
  PrepArgs pa;
  memset(&pa, 0, sizeof(pa));
  int64_t maxn = 0;
  int k = 0;
  for (int l = wide_input(d) ? 0 : 1; l + 1 < g.L; ++l, ++k) {
    pa.W[k] = d->weight[l];
    pa.Wop[k] = lo.w_op_off[l] >= 0 ? dst + lo.w_op_off[l] : nullptr;
    pa.Wt[k] = dst + lo.wt_op_off[l];
    pa.O[k] = d->dims[l + 1];
    pa.I[k] = d->dims[l];
    pa.Kp[k] = l == 0 ? first_kp(d) : d->dims[l];
    maxn = std::max(maxn, (int64_t)pa.O[k] * pa.Kp[k]);
  }
  if (k == 0) return SIREN_OK;
  pa.nb = g.nb;
  hipLaunchKernelGGL(prep_weights_kernel<PREC>, dim3(grid1d(g.nb * maxn, 512), (unsigned)k),
                     dim3(256), 0, st, pa);
  return check_launch("prep_weights");
}

template <int PREC, int IT, int MAXO>
void launch_last_fwd(const LastFwdArgs& a, int64_t nb, hipStream_t st) {
  if (a.lloss) {  // fused image loss: at most SSE_MAX_BLOCKS workgroups (the hand-off's slots)
    const unsigned gx = (unsigned)std::max<int64_t>(1, std::min<int64_t>(cdiv(a.rows_per_batch, 8),
                                                                        std::max<int64_t>(1, SSE_MAX_BLOCKS / nb)));
    hipLaunchKernelGGL((last_fwd_kernel<PREC, IT, MAXO, true>), dim3(gx, (unsigned)nb), dim3(256), 0, st, a);
    return;
  }
  const unsigned gx = (unsigned)std::max<int64_t>(1, std::min<int64_t>(cdiv(a.rows_per_batch, 8),
                                                                      std::max<int64_t>(1, 4096 / nb)));
  hipLaunchKernelGGL((last_fwd_kernel<PREC, IT, MAXO>), dim3(gx, (unsigned)nb), dim3(256), 0, st, a);
}

template <int PREC>
int dispatch_last_fwd(const LastFwdArgs& a, int64_t nb, hipStream_t st) {
  const int it = (int)cdiv(a.F, 256);
  if (a.O <= 2) {
    if (it == 1) launch_last_fwd<PREC, 1, 2>(a, nb, st);
    else if (it == 2) launch_last_fwd<PREC, 2, 2>(a, nb, st);
    else launch_last_fwd<PREC, 4, 2>(a, nb, st);
  } else {
    if (it == 1) launch_last_fwd<PREC, 1, 8>(a, nb, st);
    else if (it == 2) launch_last_fwd<PREC, 2, 8>(a, nb, st);
    else launch_last_fwd<PREC, 4, 8>(a, nb, st);
  }
  return check_launch("last_fwd");
}

template <int PREC>
int dispatch_last_bwd(const LastBwdArgs& a, int64_t nsplit, int64_t nb, hipStream_t st) {
  const int it = (int)cdiv(a.F, 256);
  dim3 grid((unsigned)nsplit, (unsigned)nb);
  if (a.O <= 2) {
    if (it == 1) hipLaunchKernelGGL((last_bwd_kernel<PREC, 1, 2>), grid, dim3(256), 0, st, a);
    else if (it == 2) hipLaunchKernelGGL((last_bwd_kernel<PREC, 2, 2>), grid, dim3(256), 0, st, a);
    else hipLaunchKernelGGL((last_bwd_kernel<PREC, 4, 2>), grid, dim3(256), 0, st, a);
  } else {
    if (it == 1) hipLaunchKernelGGL((last_bwd_kernel<PREC, 1, 8>), grid, dim3(256), 0, st, a);
    else if (it == 2) hipLaunchKernelGGL((last_bwd_kernel<PREC, 2, 8>), grid, dim3(256), 0, st, a);
    else hipLaunchKernelGGL((last_bwd_kernel<PREC, 4, 8>), grid, dim3(256), 0, st, a);
  }
  return check_launch("last_bwd");
}

template <int PREC>
int dispatch_first_bwd(const FirstBwdArgs& a, int64_t nsplit, int64_t nb, hipStream_t st) {
  const int it = (int)cdiv(a.F, 256);
  dim3 grid((unsigned)nsplit, (unsigned)nb);
  if (a.ffB) {  // Fourier-feature input: the MFMA weight-gradient kernel forms the features itself
    if (!(PREC == kPrecBF16 && a.F == 256 && a.C > 4 && a.rows_per_split % 32 == 0 && !a.dx))
      return fail(SIREN_EINVAL, "fourier input: first-layer backward needs the bf16 wide MFMA path and no dx");
    hipLaunchKernelGGL(first_bwd_wide_mfma_kernel, grid, dim3(256), 0, st, a);
    return check_launch("first_bwd_wide_mfma (fourier input)");
  }
  if (a.C <= 4) {
    if (it == 1) hipLaunchKernelGGL((first_bwd_kernel<PREC, 1, 4>), grid, dim3(256), 0, st, a);
    else if (it == 2) hipLaunchKernelGGL((first_bwd_kernel<PREC, 2, 4>), grid, dim3(256), 0, st, a);
    else hipLaunchKernelGGL((first_bwd_kernel<PREC, 4, 4>), grid, dim3(256), 0, st, a);
  } else if (a.F <= 256 && (!a.dx || (PREC == kPrecBF16 && a.F == 256))) {
    // weight gradient without dx; the input gradient (bf16 mode) as its own MFMA launch
    FirstBwdArgs aw = a;
    aw.dx = nullptr;
    if (PREC == kPrecBF16 && a.F == 256 && a.rows_per_split % 32 == 0)
      hipLaunchKernelGGL(first_bwd_wide_mfma_kernel, grid, dim3(256), 0, st, aw);
    else if (a.C == 16) hipLaunchKernelGGL((first_bwd_wide_kernel<PREC, 16>), grid, dim3(256), 0, st, aw);
    else hipLaunchKernelGGL((first_bwd_wide_kernel<PREC, 0>), grid, dim3(256), 0, st, aw);
    if (a.dx) {
      int rc = check_launch("first_bwd_wide");
      if (rc) return rc;
      const int64_t ntile = cdiv(a.rows_per_batch, 32);
      hipLaunchKernelGGL(first_dx_wide_kernel, dim3((unsigned)cdiv(ntile, 4), (unsigned)nb), dim3(256), 0, st, a);
    }
  } else {
    if (it == 1) hipLaunchKernelGGL((first_bwd_kernel<PREC, 1, 16>), grid, dim3(256), 0, st, a);
    else hipLaunchKernelGGL((first_bwd_kernel<PREC, 2, 16>), grid, dim3(256), 0, st, a);
  }
  return check_launch("first_bwd");
}

// One hidden-layer GEMM launch (MODE_FWD or MODE_DX). Persistent grid: one 512-thread workgroup
// per CU (~131 KB LDS each), spread over weight sets and 256-column tiles.
dim3 nt_grid(const NTArgs& a, int64_t nb, int prec) {
  const int ntn = (int)cdiv(a.N, 256);
  const int kmax = a.K <= 256 ? 256 : 512;  // siren_mlp_check bounds K by 512 (bf16) / 256 (f32)
  const int bm = prec == kPrecBF16 ? 64 * 256 / kmax : 32;
  const int64_t tiles = cdiv(a.rows_per_batch, bm);
  const int64_t per = std::max<int64_t>(1, 256 / std::max<int64_t>(1, nb * ntn));
  return dim3((unsigned)std::min<int64_t>(tiles, per), (unsigned)nb, (unsigned)ntn);
}

dim3 ring_grid(const NTArgs& a, int64_t nb) {
  const int64_t tiles = cdiv(a.rows_per_batch, RING_BM);
  const int64_t per = std::max<int64_t>(1, 256 / nb);
  return dim3((unsigned)std::min<int64_t>(tiles, per), (unsigned)nb, 1);
}

// Bottom 256x256 input-gradient layer with the first layer folded in (dx_ring_bf16_kernel BOTC).
int launch_dx_ring_bot(const NTArgs& a, int64_t nb, int C, bool dxout, bool rec, int kclass, hipStream_t st) {
  const dim3 grid = ring_grid(a, nb);
  tmark_begin(kclass, st);
#define SIREN_RING_BOT(CC)                                                                              \
  if (rec) {                                                                                             \
    if (dxout) hipLaunchKernelGGL((dx_ring_bf16_kernel<CC, true, true>), grid, dim3(512), 0, st, a);     \
    else hipLaunchKernelGGL((dx_ring_bf16_kernel<CC, false, true>), grid, dim3(512), 0, st, a);          \
  } else {                                                                                               \
    if (dxout) hipLaunchKernelGGL((dx_ring_bf16_kernel<CC, true>), grid, dim3(512), 0, st, a);           \
    else hipLaunchKernelGGL((dx_ring_bf16_kernel<CC, false>), grid, dim3(512), 0, st, a);                \
  }
  switch (C) {
    case 1: SIREN_RING_BOT(1) break;
    case 2: SIREN_RING_BOT(2) break;
    case 3: SIREN_RING_BOT(3) break;
    default: SIREN_RING_BOT(4) break;
  }
#undef SIREN_RING_BOT
  tmark_end(kclass, st);
  return check_launch("dx_ring first-layer");
}

template <int PREC, int MODE, bool TOP = false, bool BOT = false>
int launch_nt(const NTArgs& a, int64_t nb, int kclass, hipStream_t st) {
  const int kmax = a.K <= 256 ? 256 : 512;
  if constexpr (PREC == kPrecF32 && (MODE == MODE_FWD || MODE == MODE_DX) && !TOP && !BOT) {
    // fp32 hidden layers on the row-stacked tile (jvp_tan_kernel JT_FWD / JT_DX: 128 rows x all
    // 256 output features per workgroup, 8 waves; nt_f32_kernel's products, K order and epilogues)
    if (g_f32_rows && a.K % JNT_KC == 0 && a.K <= 512 && a.N <= JADJ_BN && a.lda == a.K &&
        (MODE == MODE_FWD || a.Paux)) {
      JTanArgs t;
      memset(&t, 0, sizeof(t));
      t.P = MODE == MODE_FWD ? a.A : a.Paux;
      t.U = MODE == MODE_DX ? (const float*)a.A : nullptr;
      t.W = a.W;
      t.bias = a.bias;
      t.Uout = (float*)a.C;
      t.N = a.rows_per_batch;
      t.Su = 1;
      t.w_bstride = a.w_bstride;
      t.b_bstride = a.bias_bstride;
      t.K = a.K;
      t.Nout = a.N;
      t.w0 = a.w0;
      const dim3 grid((unsigned)cdiv(a.rows_per_batch, 2 * JADJ_ROWS), (unsigned)nb);
      tmark_begin(kclass, st);
      if constexpr (MODE == MODE_FWD) hipLaunchKernelGGL((jvp_tan_kernel<kPrecF32, 2, JT_FWD>), grid, dim3(512), 0, st, t);
      else hipLaunchKernelGGL((jvp_tan_kernel<kPrecF32, 2, JT_DX>), grid, dim3(512), 0, st, t);
      tmark_end(kclass, st);
      return check_launch(MODE == MODE_FWD ? "f32 rows fwd" : "f32 rows dx");
    }
  }
  if constexpr (PREC == kPrecBF16 && MODE == MODE_DX && !TOP && !BOT) {
    if (g_dx_ring && a.K == 256 && a.N == 256) {
      tmark_begin(SIREN_KCLASS_DX_RING, st);
      hipLaunchKernelGGL((dx_ring_bf16_kernel<0, false>), ring_grid(a, nb), dim3(512), 0, st, a);
      tmark_end(SIREN_KCLASS_DX_RING, st);
      return check_launch("dx_ring");
    }
  }
  const dim3 grid = nt_grid(a, nb, PREC);
  tmark_begin(kclass, st);
  if constexpr (PREC == kPrecBF16) {
    if (kmax == 256) hipLaunchKernelGGL((nt_bf16_kernel<MODE, 256, TOP, BOT>), grid, dim3(512), 0, st, a);
    else hipLaunchKernelGGL((nt_bf16_kernel<MODE, 512, TOP, BOT>), grid, dim3(512), 0, st, a);
  } else {
    static_assert(PREC == kPrecBF16 || !(TOP || BOT), "backward fusions are bf16-mode paths");
    if (kmax == 256) hipLaunchKernelGGL((nt_f32_kernel<MODE>), grid, dim3(512), 0, st, a);
    else hipLaunchKernelGGL((nt_f32_kernel<MODE, 512>), grid, dim3(512), 0, st, a);
  }
  tmark_end(kclass, st);
  static const char* const names[] = {"nt_gemm fwd", "nt_gemm dx", "nt_gemm first", "nt_gemm dx-input"};
  return check_launch(names[MODE]);
}

// Register-resident forward (siren_fwdreg.hip): one weight-prep launch, one forward launch.
int fused_forward_reg(const siren_mlp_desc* d, const Geo& g, const Layout& lo, const float* x, float* y,
                      char* saved, char* wbuf, hipStream_t st, const siren_loss_desc* L = nullptr) {
  const int F = d->dims[1], nh = g.L - 2;
  _Float16* wreg = (_Float16*)(wbuf + lo.frag_off);
  _Float16* wlreg = wreg + g.nb * (int64_t)nh * F * F;
  float* wbound = (float*)(wlreg + g.nb * (FREG_WL_BYTES / 2));
  {
    RegPrepArgs p;
    memset(&p, 0, sizeof(p));
    for (int l = 1; l + 1 < g.L; ++l) {
      p.W[l - 1] = d->weight[l];
      p.Wt[l - 1] = saved ? (bf16*)(saved + lo.wt_op_off[l]) : nullptr;  // the backward's W^T
    }
    p.WL = d->weight[g.L - 1];
    p.out = wreg;
    p.outL = wlreg;
    p.wbound = g_freg_magic ? wbound : nullptr;  // (the magic form's check only)
    p.nb = g.nb;
    p.nh = nh;
    p.O = d->dims[g.L];
    p.k1 = d->w0 * kInv2Pi;
    const int64_t work = g.nb * ((int64_t)nh * F * F / 8 + FREG_WL_BYTES / 16 + (int64_t)nh * F * 64);
    hipLaunchKernelGGL(prep_reg_kernel, dim3(grid1d(work, 1024)), dim3(256), 0, st, p);
    int rc = check_launch("prep_reg");
    if (rc) return rc;
  }
  FwdRegArgs a;
  memset(&a, 0, sizeof(a));
  a.x = x;
  a.W0 = d->weight[0];
  a.b0 = d->bias[0];
  a.Wreg = wreg;
  a.WLreg = wlreg;
  for (int l = 1; l + 1 < g.L; ++l) a.bias[l - 1] = d->bias[l];
  a.bL = d->bias[g.L - 1];
  a.wbound = wbound;
  a.P0 = (saved && lo.saved_off[0] >= 0) ? saved + lo.saved_off[0] : nullptr;
  a.Pb = saved ? saved + lo.saved_off[1] : nullptr;
  a.pstride = (saved && nh >= 2) ? lo.saved_off[2] - lo.saved_off[1] : 0;
  a.y = y;
  a.rows_per_batch = g.rows;
  a.batched = d->weights_batched ? 1 : 0;
  a.O = d->dims[g.L];
  a.nh = nh;
  a.sine_out = d->outermost_linear ? 0 : 1;
  a.cin = d->dims[0];
  a.w0 = d->w0;
  a.ffB = d->ff_B;
  a.ffin = d->ff_B ? d->ff_in : 0;
  if (L) {
    a.ltgt = L->target;
    a.lk0 = L->k0;
    a.lmask = L->mask;
    a.lhf = L->hf;
    a.ldc = L->y_dc;
    a.ldy = L->dy;
    a.lloss = L->loss;
    a.lpart = (float*)L->loss_workspace;
    a.lcounter = (unsigned*)((char*)L->loss_workspace + SSE_MAX_BLOCKS * 4);
    a.lnoise = L->noise;
    a.lweight = L->weight;
  }
  const int64_t tiles = cdiv(g.rows, FREG_WG_ROWS);
  const int64_t per = std::max<int64_t>(1, 256 / g.nb);
  dim3 grid((unsigned)std::min<int64_t>(tiles, per), (unsigned)g.nb);
  using KernelFn = void (*)(FwdRegArgs);
#define SIREN_FREG_FORMS(CC, OC) {fused_fwd_reg_kernel<CC, OC, 0>, fused_fwd_reg_kernel<CC, OC, 1>}
  static const KernelFn table[2][FUSED_MAXC][2] = {
      {SIREN_FREG_FORMS(1, 0), SIREN_FREG_FORMS(2, 0), SIREN_FREG_FORMS(3, 0), SIREN_FREG_FORMS(4, 0)},
      {SIREN_FREG_FORMS(1, 1), SIREN_FREG_FORMS(2, 1), SIREN_FREG_FORMS(3, 1), SIREN_FREG_FORMS(4, 1)}};
  static const KernelFn wide[2][2][2] = {{SIREN_FREG_FORMS(16, 0), SIREN_FREG_FORMS(16, 1)},
                                         {SIREN_FREG_FORMS(17, 0), SIREN_FREG_FORMS(17, 1)}};
#undef SIREN_FREG_FORMS
  const int ffi = d->ff_B ? 1 : 0;  // C = 17: the Fourier-feature input (siren_mlp_check: wide shapes only)
  const KernelFn* k = fused_wide(d) ? wide[ffi][a.O == 1 ? 1 : 0] : table[a.O == 1 ? 1 : 0][d->dims[0] - 1];
  if (L) {  // the fused-loss forms (siren_mlp_loss_check admitted this shape)
    static const KernelFn lnarrow[FUSED_MAXC] = {fused_fwd_reg_kernel<1, 1, 0, true>, fused_fwd_reg_kernel<2, 1, 0, true>,
                                                 fused_fwd_reg_kernel<3, 1, 0, true>, fused_fwd_reg_kernel<4, 1, 0, true>};
    static const KernelFn lwide[2][2] = {{fused_fwd_reg_kernel<16, 0, 0, true>, fused_fwd_reg_kernel<16, 1, 0, true>},
                                         {fused_fwd_reg_kernel<17, 0, 0, true>, fused_fwd_reg_kernel<17, 1, 0, true>}};
    const KernelFn kl = fused_wide(d) ? lwide[ffi][a.O == 1 ? 1 : 0] : lnarrow[d->dims[0] - 1];
    a.wbound = nullptr;  // the fract form alone (no magic-form exit test on an unwritten bound)
    tmark_begin(SIREN_KCLASS_FWD_FUSED, st);
    hipLaunchKernelGGL(kl, grid, dim3(512), 0, st, a);
    tmark_end(SIREN_KCLASS_FWD_FUSED, st);
    return check_launch("fused_fwd_reg (loss)");
  }
  tmark_begin(SIREN_KCLASS_FWD_FUSED, st);
  // magic form (option freg_magic): both forms are launched, the one whose form does not apply to
  // these weights exits at its start (siren_fwdreg.hip); otherwise the fract form alone
  if (g_freg_magic) hipLaunchKernelGGL(k[1], grid, dim3(512), 0, st, a);
  else a.wbound = nullptr;
  hipLaunchKernelGGL(k[0], grid, dim3(512), 0, st, a);
  tmark_end(SIREN_KCLASS_FWD_FUSED, st);
  return check_launch("fused_fwd_reg");
}

int fused_forward(const siren_mlp_desc* d, const Geo& g, const Layout& lo, const float* x, float* y,
                  char* saved, char* wbuf, hipStream_t st) {
  const int F = d->dims[1], nh = g.L - 2;
  if (g_fwd_reg && nh > 0) return fused_forward_reg(d, g, lo, x, y, saved, wbuf, st);
  if (nh > 0) {
    FragPrepArgs fp;
    memset(&fp, 0, sizeof(fp));
    for (int l = 1; l + 1 < g.L; ++l) {
      fp.W[l - 1] = d->weight[l];
      // the backward's W^T copies, written by the same launch (prep_weights is skipped)
      fp.Wt[l - 1] = saved ? (bf16*)(saved + lo.wt_op_off[l]) : nullptr;
    }
    fp.out = (bf16*)(wbuf + lo.frag_off);
    fp.nb = g.nb;
    fp.F = F;
    fp.nh = nh;
    fp.f16 = g_fwd_pipe ? 1 : 0;  // the pipe kernel multiplies in fp16 (sin values need no bf16 range)
    hipLaunchKernelGGL(prep_frag_kernel, dim3(grid1d(g.nb * nh * (int64_t)F * F / 8, 1024)), dim3(256), 0,
                       st, fp);
    int rc = check_launch("prep_frag");
    if (rc) return rc;
  }
  FusedFwdArgs a;
  memset(&a, 0, sizeof(a));
  a.x = x;
  a.W0 = d->weight[0];
  a.b0 = d->bias[0];
  a.Wfrag = nh > 0 ? (const bf16*)(wbuf + lo.frag_off) : nullptr;
  for (int l = 1; l + 1 < g.L; ++l) a.bias[l - 1] = d->bias[l];
  a.WL = d->weight[g.L - 1];
  a.bL = d->bias[g.L - 1];
  for (int l = 0; l + 1 < g.L; ++l) a.P[l] = (saved && lo.saved_off[l] >= 0) ? saved + lo.saved_off[l] : nullptr;
  a.y = y;
  a.prof = g_fused_prof;
  a.dbg = g_fwd_dbg;
  a.rows_per_batch = g.rows;
  a.batched = d->weights_batched ? 1 : 0;
  a.C = d->dims[0];
  a.F = F;
  a.O = d->dims[g.L];
  a.nh = nh;
  a.sine_out = d->outermost_linear ? 0 : 1;
  a.w0 = d->w0;
  const int64_t tiles = cdiv(g.rows, FUSED_BM);
  const int64_t per = std::max<int64_t>(1, 256 / g.nb);
  dim3 grid((unsigned)std::min<int64_t>(tiles, per), (unsigned)g.nb);
  tmark_begin(SIREN_KCLASS_FWD_FUSED, st);
  using KernelFn = void (*)(FusedFwdArgs);
  static const KernelFn table[FUSED_MAXC] = {fused_fwd_bf16_kernel<256, 1>, fused_fwd_bf16_kernel<256, 2>,
                                             fused_fwd_bf16_kernel<256, 3>, fused_fwd_bf16_kernel<256, 4>};
  static const KernelFn pipe[2][FUSED_MAXC] = {
      {fused_fwd_pipe_kernel<1, 0>, fused_fwd_pipe_kernel<2, 0>, fused_fwd_pipe_kernel<3, 0>, fused_fwd_pipe_kernel<4, 0>},
      {fused_fwd_pipe_kernel<1, 1>, fused_fwd_pipe_kernel<2, 1>, fused_fwd_pipe_kernel<3, 1>, fused_fwd_pipe_kernel<4, 1>}};
  const bool use_pipe = g_fwd_pipe && nh > 0;
  hipLaunchKernelGGL((use_pipe ? pipe[a.O == 1 ? 1 : 0] : table)[a.C - 1], grid,
                     dim3(use_pipe ? 64 * SIREN_PIPE_NW : 512), 0, st, a);
  tmark_end(SIREN_KCLASS_FWD_FUSED, st);
  return check_launch("fused_fwd");
}

// L: the fused image loss in the output layer's epilogue (siren_mlp_forward_loss on the per-layer
// path; the register forward has its own, fused_forward_reg)
template <int PREC>
int forward_impl(const siren_mlp_desc* d, const float* x, float* y, char* saved, char* ws,
                 hipStream_t st, const siren_loss_desc* L = nullptr) {
  const Geo g = geo_of(d);
  const Layout lo = layout_of(d);
  char* wbuf = saved ? saved : ws;  // prepared weights live in `saved` so backward reuses them
  const bool fused = PREC == kPrecBF16 && g_fused_forward && fused_shape(d);
  if (fused && !L) return fused_forward(d, g, lo, x, y, saved, wbuf, st);  // prepares its own weights
  int rc = prep_weights<PREC>(d, g, lo, wbuf, st);
  if (rc) return rc;
  auto phase_buf = [&](int l) -> char* {
    if (saved && lo.saved_off[l] >= 0) return saved + lo.saved_off[l];
    return ws + lo.pp_off[l & 1];  // (P_0 of a recompute stack: only layer 1 reads it)
  };
  // Layer 0: MFMA GEMM for wide inputs, VALU otherwise.
  if (wide_input(d)) {
    NTArgs a;
    a.A = x;
    a.W = wbuf + lo.w_op_off[0];
    a.bias = d->bias[0];
    a.Paux = nullptr;
    a.C = phase_buf(0);
    a.rows_per_batch = g.rows;
    a.w_bstride = d->weights_batched ? (int64_t)d->dims[1] * first_kp(d) : 0;
    a.bias_bstride = d->weights_batched ? d->dims[1] : 0;
    a.K = first_kp(d);
    a.N = d->dims[1];
    a.lda = d->dims[0];
    a.a_vec = (d->dims[0] % 4 == 0) && aligned16(x);
    a.w0 = d->w0;
    if ((rc = launch_nt<PREC, MODE_FIRST>(a, g.nb, 0, st))) return rc;
  } else {
    FirstFwdArgs a;
    a.x = x;
    a.W = d->weight[0];
    a.b = d->bias[0];
    a.P = phase_buf(0);
    a.rows_per_batch = g.rows;
    a.w_bstride = d->weights_batched ? (int64_t)d->dims[1] * d->dims[0] : 0;
    a.b_bstride = d->weights_batched ? d->dims[1] : 0;
    a.C = d->dims[0];
    a.F = d->dims[1];
    a.w0 = d->w0;
    const unsigned gx = grid1d(g.rows * (a.F / 8), std::max<int64_t>(1, 4096 / g.nb));
    if (a.C <= 4)
      hipLaunchKernelGGL((first_fwd_kernel<PREC, 4>), dim3(gx, (unsigned)g.nb), dim3(256), 0, st, a);
    else
      hipLaunchKernelGGL((first_fwd_kernel<PREC, 16>), dim3(gx, (unsigned)g.nb), dim3(256), 0, st, a);
    if ((rc = check_launch("first_fwd"))) return rc;
  }
  // Hidden MFMA layers.
  for (int l = 1; l + 1 < g.L; ++l) {
    NTArgs a;
    a.A = phase_buf(l - 1);
    a.W = PREC == kPrecBF16 ? (const void*)(wbuf + lo.w_op_off[l]) : (const void*)d->weight[l];
    a.bias = d->bias[l];
    a.Paux = nullptr;
    a.C = phase_buf(l);
    a.rows_per_batch = g.rows;
    a.w_bstride = d->weights_batched ? (int64_t)d->dims[l + 1] * d->dims[l] : 0;
    a.bias_bstride = d->weights_batched ? d->dims[l + 1] : 0;
    a.K = d->dims[l];
    a.N = d->dims[l + 1];
    a.lda = a.K;
    a.a_vec = 0;
    a.w0 = d->w0;
    if ((rc = launch_nt<PREC, MODE_FWD>(a, g.nb, SIREN_KCLASS_FWD_GEMM, st))) return rc;
  }
  // Output layer (VALU).
  {
    const int l = g.L - 1;
    LastFwdArgs a;
    a.P = phase_buf(l - 1);
    a.W = d->weight[l];
    a.b = d->bias[l];
    a.y = y;
    a.rows_per_batch = g.rows;
    a.w_bstride = d->weights_batched ? (int64_t)d->dims[l + 1] * d->dims[l] : 0;
    a.b_bstride = d->weights_batched ? d->dims[l + 1] : 0;
    a.F = d->dims[l];
    a.O = d->dims[l + 1];
    a.sine_out = d->outermost_linear ? 0 : 1;
    a.w0 = d->w0;
    a.ltgt = a.lk0 = a.lmask = a.lhf = nullptr;
    a.ldc = a.ldy = a.lloss = a.lpart = nullptr;
    a.lcounter = nullptr;
    a.lnoise = a.lweight = 0.f;
    if (L) {
      a.ltgt = L->target;
      a.lk0 = L->k0;
      a.lmask = L->mask;
      a.lhf = L->hf;
      a.ldc = L->y_dc;
      a.ldy = L->dy;
      a.lloss = L->loss;
      a.lpart = (float*)L->loss_workspace;
      a.lcounter = (unsigned*)((char*)L->loss_workspace + SSE_MAX_BLOCKS * 4);
      a.lnoise = L->noise;
      a.lweight = L->weight;
    }
    if ((rc = dispatch_last_fwd<PREC>(a, g.nb, st))) return rc;
  }
  return SIREN_OK;
}

// One pair_ring_bf16_kernel launch for hidden layer l (kind: see backward_impl) and the
// reductions of its partial slabs.
template <int PREC>
int launch_pair(const siren_mlp_desc* d, const Geo& g, const Layout& lo, int kind, int l, const float* x,
                const TopArgs& ta, char* ws, const char* saved, float* part, float* const* dW, float* const* db,
                float* dx, int cur, ReduceList& pend, hipStream_t st) {
  const int M = d->dims[l + 1], N = d->dims[l], C = d->dims[0], F0 = d->dims[1], O = d->dims[g.L];
  const int64_t npair = pair_count(g);
  TNArgs w;
  memset(&w, 0, sizeof(w));
  w.D = ws + lo.dz_off[cur];
  w.P = kind == 3 ? (const void*)x : (const void*)(saved + lo.saved_off[l - 1]);
  w.part = part;
  w.rows_per_batch = g.rows;
  w.rows_per_split = 0;  // ranges come from the pair index
  w.split_stride = split_stride(g, (int64_t)M * N + M);
  w.M = M;
  w.N = N;
  w.w0 = d->w0;
  w.top = ta;
  w.pair_roles = g_pair_roles;
  w.prof = g_ring_prof ? g_ring_prof + (int64_t)(g_ring_prof_n++) * 256 * 8 * RING_NPROF : nullptr;
  NTArgs a;
  memset(&a, 0, sizeof(a));
  a.A = ws + lo.dz_off[cur];
  a.W = saved + lo.wt_op_off[l];
  a.Paux = kind == 3 ? nullptr : (const void*)(saved + lo.saved_off[l - 1]);
  a.C = ws + lo.dz_off[cur ^ 1];
  a.rows_per_batch = g.rows;
  a.w_bstride = d->weights_batched ? (int64_t)M * N : 0;
  a.K = M;
  a.N = N;
  a.lda = M;
  a.w0 = d->w0;
  a.top = ta;
  a.prof = w.prof;
  a.stagger = g_dx_stagger ? 1 : 0;
  const int64_t bot_stride = split_stride(g, (int64_t)F0 * C + F0);
  if (kind == 3) {
    w.rec_W0 = d->weight[0];
    w.rec_w0_bstride = d->weights_batched ? (int64_t)F0 * C : 0;
    w.rec_b0 = d->bias[0];
    w.rec_b0_bstride = d->weights_batched ? F0 : 0;
    a.C = dx;
    a.bot.x = x;
    a.bot.W0 = d->weight[0];
    a.bot.w0_bstride = w.rec_w0_bstride;
    a.bot.b0 = d->bias[0];
    a.bot.b0_bstride = w.rec_b0_bstride;
    a.bot.part = (float*)(ws + lo.partB_off);
    a.bot.split_stride = bot_stride;
    a.bot.C = C;
  }
  const int64_t nx = npair, nw = npair;  // input-gradient / weight-gradient workgroups (slabs)
  const dim3 grid((unsigned)(2 * npair), (unsigned)g.nb);
  const int kcls = kind == 1 ? SIREN_KCLASS_PAIR_RING : kind == 2 ? SIREN_KCLASS_PAIR_RING_TOP : SIREN_KCLASS_PAIR_RING_BOT;
  tmark_begin(kcls, st);
  const ReduceMultiArgs prev = pend.a;  // the previous pair launch's slabs, reduced in this one's tail
  if (kind == 1) {
    hipLaunchKernelGGL((pair_ring_bf16_kernel<0, false, false, 0, 0>), grid, dim3(512), 0, st, a, w, prev);
  } else if (kind == 2) {
    if (O == 1) hipLaunchKernelGGL((pair_ring_bf16_kernel<0, false, false, 1, 0>), grid, dim3(512), 0, st, a, w, prev);
    else hipLaunchKernelGGL((pair_ring_bf16_kernel<0, false, false, 2, 0>), grid, dim3(512), 0, st, a, w, prev);
  } else {
#define SIREN_PAIR_BOT(CC)                                                                                         \
  if (dx) hipLaunchKernelGGL((pair_ring_bf16_kernel<CC, true, true, 0, CC>), grid, dim3(512), 0, st, a, w, prev);   \
  else hipLaunchKernelGGL((pair_ring_bf16_kernel<CC, false, true, 0, CC>), grid, dim3(512), 0, st, a, w, prev);
    switch (C) {
      case 1: SIREN_PAIR_BOT(1) break;
      case 2: SIREN_PAIR_BOT(2) break;
      case 3: SIREN_PAIR_BOT(3) break;
      default: SIREN_PAIR_BOT(4) break;
    }
#undef SIREN_PAIR_BOT
  }
  tmark_end(kcls, st);
  int rc = check_launch("pair_ring");
  if (rc) return rc;
  // this launch's slabs: reduced by the next pair launch, or by a reduce_multi launch (flush)
  ReduceList red;
  red.add(part, nw, w.split_stride, g.nb, (int64_t)M * N + M, (int64_t)M * N, dW[l], db[l]);
  if (kind == 2) red.add(ta.partL, nw, ta.partL_stride, g.nb, (int64_t)O * M + O, (int64_t)O * M, dW[g.L - 1], db[g.L - 1]);
  if (kind == 3) red.add(a.bot.part, nx, bot_stride, g.nb, (int64_t)F0 * C + F0, (int64_t)F0 * C, dW[0], db[0]);
  pend = red;
  return SIREN_OK;
}

template <int PREC>
int backward_impl(const siren_mlp_desc* d, const float* x, const float* dy, const char* saved,
                  char* ws, float* const* dW, float* const* db, float* dx, hipStream_t st,
                  const float* dy_scale = nullptr) {
  const Geo g = geo_of(d);
  const Layout lo = layout_of(d);
  int rc = SIREN_OK;
  float* part = (float*)(ws + lo.part_off);
  auto P = [&](int l) -> const void* { return saved + lo.saved_off[l]; };
  const int O = d->dims[g.L], C = d->dims[0], F0 = d->dims[1];
  // slab reduction of the last pair launch, not yet issued (see launch_pair)
  ReduceList pend;
  int npair_launches = 0;
  auto flush = [&]() -> int {
    const int r = pend.launch(st);
    pend = ReduceList();
    return r;
  };
  // bf16-mode fusions (siren_gemm.hip TopArgs / BotArgs): the output layer's backward folds into
  // the top hidden layer's kernels, the first layer's weight gradient into the bottom one's.
  const bool fuse = PREC == kPrecBF16 && g_fused_backward && g.L >= 3;
  // P_0 not kept (p0_recompute): layer 1 runs on the ring kernels that rebuild it from x, whatever
  // the options say; they DMA x in 16-byte pieces, so a misaligned x is copied first.
  const bool rec = lo.p0_rec;
  if (rec && !aligned16(x)) {
    if (hipMemcpyAsync(ws + lo.xcopy_off, x, g.total * C * sizeof(float), hipMemcpyDeviceToDevice, st) != hipSuccess)
      return fail(SIREN_ELAUNCH, "x copy: %s", hipGetErrorString(hipGetLastError()));
    x = (const float*)(ws + lo.xcopy_off);
  }
  const bool top_ok = fuse && d->outermost_linear && O <= TOP_MAXO && (g.rows * O) % 4 == 0 && g.rows * O >= 4 &&
                      aligned16(dy) && !(rec && g.L == 3);
  // output layer folded into the top layer's ring kernels (256x256 top layer below another layer)
  const bool ring_top = top_ok && g_ring_top && g.L >= 4 && d->dims[g.L - 1] == 256 && d->dims[g.L - 2] == 256;
  const bool top = ring_top || (top_ok && g_fuse_top && d->dims[g.L - 1] <= 256);
  // first-layer fusion: the ring kernel (256x256 bottom layer) also produces dx; the older
  // kernel only without dx
  const bool ring_bot = rec || (fuse && g_dx_ring && !wide_input(d) && C <= BOT_MAXC && F0 == 256 &&
                                d->dims[2] == 256 && !(top && g.L == 3) && (g.rows * C) % 4 == 0 &&
                                g.rows * C >= 4 && aligned16(x));
  const bool bot = ring_bot || (fuse && !dx && !wide_input(d) && C <= BOT_MAXC && F0 <= 256 &&
                                (g.rows * C) % 4 == 0 && g.rows * C >= 4 && aligned16(x) &&
                                !(top && g.L == 3));  // one hidden layer: the output-layer fusion only
  int cur = 0;  // dz ping-pong index holding dZ of the current layer
  // Output layer: dZ_{L-2}, dW_{L-1}, db_{L-1}.
  if (!top) {
    const int l = g.L - 1;
    const Split s = valu_split(g);
    LastBwdArgs a;
    a.P = P(l - 1);
    a.W = d->weight[l];
    a.b = d->bias[l];
    a.dy = dy;
    a.dy_scale = dy_scale;
    a.dZ = ws + lo.dz_off[cur];
    a.part = part;
    a.rows_per_batch = g.rows;
    a.rows_per_split = s.rows_per_split;
    a.F = d->dims[l];
    a.O = d->dims[l + 1];
    a.split_stride = split_stride(g, (int64_t)a.O * a.F + a.O);
    a.w_bstride = d->weights_batched ? (int64_t)d->dims[l + 1] * d->dims[l] : 0;
    a.b_bstride = d->weights_batched ? d->dims[l + 1] : 0;
    a.sine_out = d->outermost_linear ? 0 : 1;
    a.w0 = d->w0;
    if ((rc = dispatch_last_bwd<PREC>(a, s.nsplit, g.nb, st))) return rc;
    if ((rc = launch_reduce(part, s.nsplit, a.split_stride, g.nb, (int64_t)a.O * a.F + a.O,
                            (int64_t)a.O * a.F, dW[l], db[l], st)))
      return rc;
  }
  TopArgs ta;
  memset(&ta, 0, sizeof(ta));
  if (top) {
    const int FL = d->dims[g.L - 1];
    ta.Ptop = P(g.L - 2);
    ta.dy = dy;
    ta.dy_scale = dy_scale;
    ta.WL = d->weight[g.L - 1];
    ta.wl_bstride = d->weights_batched ? (int64_t)O * FL : 0;
    ta.partL = (float*)(ws + lo.partL_off);
    ta.partL_stride = split_stride(g, (int64_t)O * FL + O);
    ta.O = O;
  }
  // Hidden MFMA layers, top to bottom.
  for (int l = g.L - 2; l >= 1; --l) {
    const int M = d->dims[l + 1], N = d->dims[l];
    const bool is_top = top && l == g.L - 2;
    const bool is_bot = bot && l == 1;
    const bool rec1 = rec && l == 1;
    const bool ring_t = ring_top && l == g.L - 2;
    if (PREC == kPrecBF16 && g_bwd_ring && !is_top && !is_bot && !rec1 && M == 256 && N == 256) {
      // both gradients of a middle layer in one pass (bwd_ring_bf16_kernel)
      const Split s = dw_ring_split(g);
      BwdArgs b;
      memset(&b, 0, sizeof(b));
      b.dZ = (const bf16*)(ws + lo.dz_off[cur]);
      b.P = (const uint16_t*)P(l - 1);
      b.Wt = (const bf16*)(saved + lo.wt_op_off[l]);
      b.dZo = (bf16*)(ws + lo.dz_off[cur ^ 1]);
      b.part = part;
      b.rows_per_batch = g.rows;
      b.rows_per_split = s.rows_per_split;
      b.split_stride = split_stride(g, (int64_t)M * N + M);
      b.w_bstride = d->weights_batched ? (int64_t)M * N : 0;
      b.w0 = d->w0;
      if ((rc = flush())) return rc;
      tmark_begin(SIREN_KCLASS_BWD_FUSED, st);
      hipLaunchKernelGGL(bwd_ring_bf16_kernel, dim3((unsigned)s.nsplit, (unsigned)g.nb), dim3(256), 0, st, b);
      tmark_end(SIREN_KCLASS_BWD_FUSED, st);
      if ((rc = check_launch("bwd_ring"))) return rc;
      if ((rc = launch_reduce(part, s.nsplit, b.split_stride, g.nb, (int64_t)M * N + M, (int64_t)M * N, dW[l],
                              db[l], st)))
        return rc;
      cur ^= 1;
      continue;
    }
    if (PREC == kPrecBF16 && g_pair_ring && pair_ok(g) && M == 256 && N == 256) {
      // both gradients in one launch on co-scheduled workgroup pairs (pair_ring_bf16_kernel):
      // 1 = middle layer, 2 = top layer with the output layer folded in, 3 = bottom layer with the
      // first layer folded in and P_0 rebuilt from x
      const int kind = (rec1 && !is_top)                                   ? 3
                       : (ring_t && !is_bot)                               ? 2
                       : (!is_top && !is_bot && !rec1 && g_dw_ring && g_dx_ring) ? 1
                                                                           : 0;
      if (kind) {
        // consecutive pair launches alternate slab buffers (the pending reduction reads the other
        // one); without a second buffer the pending reduction goes first
        float* pp = part;
        if (!g_tail_reduce && (rc = flush())) return rc;
        if (lo.part2_off >= 0) {
          if (npair_launches++ & 1) pp = (float*)(ws + lo.part2_off);
        } else if ((rc = flush())) {
          return rc;
        }
        if ((rc = launch_pair<PREC>(d, g, lo, kind, l, x, ta, ws, saved, pp, dW, db, dx, cur, pend, st))) return rc;
        if (kind == 3) return flush();  // first layer done
        cur ^= 1;
        continue;
      }
    }
    if ((rc = flush())) return rc;  // the per-layer kernels below reuse `part`
    const bool ring = rec1 || ring_t || (PREC == kPrecBF16 && g_dw_ring && !is_top && M == 256 && N == 256);
    {
      const Split s = ring ? dw_ring_split(g) : tn_split(g, M, N);
      int64_t nsplit_used = s.nsplit;
      TNArgs a;
      memset(&a, 0, sizeof(a));
      a.D = ws + lo.dz_off[cur];
      a.P = rec1 ? (const void*)x : P(l - 1);
      a.part = part;
      a.rows_per_batch = g.rows;
      a.rows_per_split = s.rows_per_split;
      a.split_stride = split_stride(g, (int64_t)M * N + M);
      if (rec1) {
        a.rec_W0 = d->weight[0];
        a.rec_w0_bstride = d->weights_batched ? (int64_t)F0 * C : 0;
        a.rec_b0 = d->bias[0];
        a.rec_b0_bstride = d->weights_batched ? F0 : 0;
      }
      a.M = M;
      a.N = N;
      a.p_vec = 0;
      a.w0 = d->w0;
      a.top = ta;
      dim3 grid((unsigned)(cdiv(M, TN_BM) * cdiv(N, TN_BN)), (unsigned)s.nsplit, (unsigned)g.nb);
      const int kcls = PREC != kPrecBF16 || !ring ? SIREN_KCLASS_DW_GEMM
                       : rec1                     ? SIREN_KCLASS_DW_RING_REC
                       : ring_t                   ? SIREN_KCLASS_DW_RING_TOP
                                                  : SIREN_KCLASS_DW_RING;
      tmark_begin(kcls, st);
      if constexpr (PREC == kPrecBF16) {
        const dim3 rg((unsigned)s.nsplit, (unsigned)g.nb);
        if (rec1) {
          switch (C) {
            case 1: hipLaunchKernelGGL((dw_ring_bf16_kernel<1>), rg, dim3(512), 0, st, a); break;
            case 2: hipLaunchKernelGGL((dw_ring_bf16_kernel<2>), rg, dim3(512), 0, st, a); break;
            case 3: hipLaunchKernelGGL((dw_ring_bf16_kernel<3>), rg, dim3(512), 0, st, a); break;
            default: hipLaunchKernelGGL((dw_ring_bf16_kernel<4>), rg, dim3(512), 0, st, a); break;
          }
        } else if (ring_t) {
          if (O == 1) hipLaunchKernelGGL((dw_ring_bf16_kernel<0, 1>), rg, dim3(512), 0, st, a);
          else hipLaunchKernelGGL((dw_ring_bf16_kernel<0, 2>), rg, dim3(512), 0, st, a);
        } else if (ring)
          hipLaunchKernelGGL((dw_ring_bf16_kernel<0>), rg, dim3(512), 0, st, a);
        else if (is_top) hipLaunchKernelGGL((tn_dw_kernel<PREC, false, true>), grid, dim3(256), 0, st, a);
        else hipLaunchKernelGGL((tn_dw_kernel<PREC, false>), grid, dim3(256), 0, st, a);
      } else if (g_f32_rows && jvp_tn2_ok(M, N)) {
        // fp32: jvp_tn2_kernel over the primal stream alone (S = 1: X = sin(P_{l-1}), D = dZ_l):
        // all 256 dW rows per workgroup, so each X element is formed once per launch
        JTNArgs j;
        memset(&j, 0, sizeof(j));
        const Split s2 = jtn2_split(g, g.rows, N);
        j.D = a.D;
        j.P = a.P;
        j.U = nullptr;
        j.part = part;
        j.N = g.rows;
        j.rows_per_split = s2.rows_per_split;
        j.split_stride = a.split_stride;
        j.S = 1;
        j.Su = 0;
        j.C = 0;
        j.M = M;
        j.Kin = N;
        j.w0 = d->w0;
        nsplit_used = s2.nsplit;
        hipLaunchKernelGGL((jvp_tn2_kernel<false>), dim3((unsigned)cdiv(N, JTN2_BN), (unsigned)s2.nsplit, (unsigned)g.nb),
                           dim3(512), 0, st, j);
      } else {
        hipLaunchKernelGGL((tn_dw_kernel<PREC, false>), grid, dim3(256), 0, st, a);
      }
      tmark_end(kcls, st);
      if ((rc = check_launch("tn_dw"))) return rc;
      if ((rc = launch_reduce(part, nsplit_used, a.split_stride, g.nb, (int64_t)M * N + M,
                              (int64_t)M * N, dW[l], db[l], st)))
        return rc;
      if (is_top &&
          (rc = launch_reduce(ta.partL, s.nsplit, ta.partL_stride, g.nb, (int64_t)O * M + O, (int64_t)O * M,
                              dW[g.L - 1], db[g.L - 1], st)))
        return rc;
    }
    {
      NTArgs a;
      memset(&a, 0, sizeof(a));
      a.A = ws + lo.dz_off[cur];
      a.W = saved + lo.wt_op_off[l];
      a.bias = nullptr;
      a.Paux = rec1 ? nullptr : P(l - 1);
      a.C = ws + lo.dz_off[cur ^ 1];
      a.rows_per_batch = g.rows;
      a.w_bstride = d->weights_batched ? (int64_t)M * N : 0;
      a.bias_bstride = 0;
      a.K = M;
      a.N = N;
      a.lda = M;
      a.a_vec = 0;
      a.w0 = d->w0;
      a.top = ta;
      a.stagger = g_dx_stagger ? 1 : 0;
      const int64_t bot_stride = split_stride(g, (int64_t)F0 * C + F0);
      if (is_bot) {
        a.bot.x = x;
        a.bot.W0 = d->weight[0];
        a.bot.w0_bstride = d->weights_batched ? (int64_t)F0 * C : 0;
        a.bot.b0 = d->bias[0];
        a.bot.b0_bstride = d->weights_batched ? F0 : 0;
        a.bot.part = part;
        a.bot.split_stride = bot_stride;
        a.bot.C = C;
      }
      if constexpr (PREC == kPrecBF16) {
        if (is_bot && ring_bot) {
          a.C = dx;  // [rows, C] f32, or not written
          rc = launch_dx_ring_bot(a, g.nb, C, dx != nullptr, rec1, SIREN_KCLASS_DX_RING_BOT, st);
        } else if (ring_t) {
          tmark_begin(SIREN_KCLASS_DX_RING_TOP, st);
          if (O == 1) hipLaunchKernelGGL((dx_ring_bf16_kernel<0, false, false, 1>), ring_grid(a, g.nb), dim3(512), 0, st, a);
          else hipLaunchKernelGGL((dx_ring_bf16_kernel<0, false, false, 2>), ring_grid(a, g.nb), dim3(512), 0, st, a);
          tmark_end(SIREN_KCLASS_DX_RING_TOP, st);
          rc = check_launch("dx_ring top");
        } else if (is_top && is_bot) rc = launch_nt<PREC, MODE_DX, true, true>(a, g.nb, SIREN_KCLASS_DX_GEMM, st);
        else if (is_top) rc = launch_nt<PREC, MODE_DX, true, false>(a, g.nb, SIREN_KCLASS_DX_GEMM, st);
        else if (is_bot) rc = launch_nt<PREC, MODE_DX, false, true>(a, g.nb, SIREN_KCLASS_DX_GEMM, st);
        else rc = launch_nt<PREC, MODE_DX>(a, g.nb, SIREN_KCLASS_DX_GEMM, st);
      } else {
        rc = launch_nt<PREC, MODE_DX>(a, g.nb, SIREN_KCLASS_DX_GEMM, st);
      }
      if (rc) return rc;
      if (is_bot) {
        const int64_t nslab = ring_bot ? ring_grid(a, g.nb).x : nt_grid(a, g.nb, PREC).x;
        if ((rc = launch_reduce(part, nslab, bot_stride, g.nb, (int64_t)F0 * C + F0, (int64_t)F0 * C, dW[0],
                                db[0], st)))
          return rc;
        return SIREN_OK;  // first layer done
      }
      cur ^= 1;
    }
  }
  if ((rc = flush())) return rc;
  // First layer.
  if (wide_input(d)) {
    const int F0 = d->dims[1], C = d->dims[0];
    const Split s = tn_split(g, F0, C);
    TNArgs a;
    a.D = ws + lo.dz_off[cur];
    a.P = x;
    a.part = part;
    a.rows_per_batch = g.rows;
    a.rows_per_split = s.rows_per_split;
    a.split_stride = split_stride(g, (int64_t)F0 * C + F0);
    a.M = F0;
    a.N = C;
    a.p_vec = (C % 4 == 0) && aligned16(x);
    dim3 grid((unsigned)(cdiv(F0, TN_BM) * cdiv(C, TN_BN)), (unsigned)s.nsplit, (unsigned)g.nb);
    hipLaunchKernelGGL((tn_dw_kernel<PREC, true>), grid, dim3(256), 0, st, a);
    if ((rc = check_launch("tn_dw first"))) return rc;
    if ((rc = launch_reduce(part, s.nsplit, a.split_stride, g.nb, (int64_t)F0 * C + F0,
                            (int64_t)F0 * C, dW[0], db[0], st)))
      return rc;
    if (dx) {
      NTArgs n;
      n.A = ws + lo.dz_off[cur];
      n.W = saved + lo.wt_op_off[0];
      n.bias = nullptr;
      n.Paux = nullptr;
      n.C = dx;
      n.rows_per_batch = g.rows;
      n.w_bstride = d->weights_batched ? (int64_t)F0 * C : 0;
      n.bias_bstride = 0;
      n.K = F0;
      n.N = C;
      n.lda = F0;
      n.a_vec = 0;
      n.w0 = d->w0;
      if ((rc = launch_nt<PREC, MODE_DXLIN>(n, g.nb, 0, st))) return rc;
    }
  } else {
    const Split s = valu_split(g);
    FirstBwdArgs a;
    memset(&a, 0, sizeof(a));
    a.dZ = ws + lo.dz_off[cur];
    a.x = x;
    a.ffB = d->ff_B;
    a.ffin = d->ff_B ? d->ff_in : 0;
    a.W = d->weight[0];
    a.dx = dx;
    a.part = part;
    a.rows_per_batch = g.rows;
    a.rows_per_split = s.rows_per_split;
    a.F = d->dims[1];
    a.C = d->dims[0];
    a.split_stride = split_stride(g, (int64_t)a.F * a.C + a.F);
    a.w_bstride = d->weights_batched ? (int64_t)d->dims[1] * d->dims[0] : 0;
    if ((rc = dispatch_first_bwd<PREC>(a, s.nsplit, g.nb, st))) return rc;
    if ((rc = launch_reduce(part, s.nsplit, a.split_stride, g.nb, (int64_t)a.F * a.C + a.F,
                            (int64_t)a.F * a.C, dW[0], db[0], st)))
      return rc;
  }
  return SIREN_OK;
}

}  // namespace
