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
// jvp_tn2_kernel (fp32 weight gradient of a hidden layer, here and in rt_jvp.hip): all 256 dW rows (the
// layer's width M) per workgroup over `stacked_rows` rows; option jvp_tn2 (default on). Its input width N
// must be a multiple of 4, which a hidden width (a multiple of 32, siren_mlp_check) always is.
bool jvp_tn2_ok(int M, int N) {
  assert(N % 4 == 0);
  return g_jvp_tn2 && M == 256;
}
Split jtn2_split(const Geo& g, int64_t stacked_rows, int N) {
  const int64_t want = std::max<int64_t>(1, 256 / (cdiv(N, JTN2_BN) * g.nb));
  Split s;
  s.rows_per_split = std::max<int64_t>(JTN2_KC, align_up(cdiv(stacked_rows, want), JTN2_KC));
  s.nsplit = std::max<int64_t>(1, cdiv(stacked_rows, s.rows_per_split));
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

inline int64_t reduce_blocks(int64_t nb, int64_t slab) { return cdiv(nb * slab, 128); }
int launch_reduce(const float* part, int64_t nsplit, int64_t sstride, int64_t nb, int64_t slab,
                  int64_t n_first, float* out0, float* out1, hipStream_t st) {
  const int64_t total = nb * slab;
  hipLaunchKernelGGL(reduce_kernel, dim3((unsigned)reduce_blocks(nb, slab)), dim3(256), 0, st, part,
                     (int)nsplit, sstride, (int)total, (int)slab, (int)n_first, out0, out1);
  return check_launch("reduce");
}

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

// Elements between the weight sets of a parameter of n elements (0: shared weights).
inline int64_t bstride(const siren_mlp_desc* d, int64_t n) { return d->weights_batched ? n : 0; }

// A kernel and the name a profiler prints for it. Every table below lists exactly the forms the
// library instantiates: adding an entry adds a kernel to the code object.
template <class... Args>
struct Kernel {
  void (*fn)(Args...);
  const char* sym;
};
#define SIREN_K(...) {__VA_ARGS__, "siren::" #__VA_ARGS__}
// the forms of a VALU layer kernel for 256, 512 and 1024 features per row (template argument IT)
#define SIREN_IT(K, P, ...) {SIREN_K(K<P, 1, __VA_ARGS__>), SIREN_K(K<P, 2, __VA_ARGS__>), SIREN_K(K<P, 4, __VA_ARGS__>)}
inline int it_index(int F) { return F <= 256 ? 0 : F <= 512 ? 1 : 2; }
// the forms of a first-layer fusion for C = 1..4 inputs: M(C, ...) names one
#define SIREN_C4(M, ...) {M(1, __VA_ARGS__), M(2, __VA_ARGS__), M(3, __VA_ARGS__), M(4, __VA_ARGS__)}

template <class... Args>
int launch_kernel(const Kernel<Args...>& k, dim3 grid, unsigned block, int kclass, const char* what, hipStream_t st,
           const Args&... a) {
  tmark_begin(kclass, st);
  hipLaunchKernelGGL(k.fn, grid, dim3(block), 0, st, a...);
  tmark_end(kclass, st);
  return check_launch(what);
}

// The fused-loss fields of a forward kernel's arguments (FwdRegArgs, LastFwdArgs).
template <class Args>
void set_loss(Args& a, const siren_loss_desc& L) {
  a.ltgt = L.target;
  a.lk0 = L.k0;
  a.lmask = L.mask;
  a.lhf = L.hf;
  a.ldc = L.y_dc;
  a.ldy = L.dy;
  a.lloss = L.loss;
  loss_workspace_slice(L.loss_workspace, &a.lpart, &a.lcounter);
  a.lnoise = L.noise;
  a.lweight = L.weight;
}

// Output layer forward (VALU), [prec][fused loss][O > 2][it_index].
int launch_last_fwd(int prec, const LastFwdArgs& a, int64_t nb, hipStream_t st) {
  static const Kernel<LastFwdArgs> k[2][2][2][3] = {
      {{SIREN_IT(last_fwd_kernel, 0, 2, false), SIREN_IT(last_fwd_kernel, 0, 8, false)},
       {SIREN_IT(last_fwd_kernel, 0, 2, true), SIREN_IT(last_fwd_kernel, 0, 8, true)}},
      {{SIREN_IT(last_fwd_kernel, 1, 2, false), SIREN_IT(last_fwd_kernel, 1, 8, false)},
       {SIREN_IT(last_fwd_kernel, 1, 2, true), SIREN_IT(last_fwd_kernel, 1, 8, true)}}};
  // fused image loss: at most LOSS_SLOTS workgroups
  const int64_t cap = a.lloss ? LOSS_SLOTS : 4096;
  const unsigned gx = (unsigned)std::max<int64_t>(1, std::min<int64_t>(cdiv(a.rows_per_batch, 8),
                                                                      std::max<int64_t>(1, cap / nb)));
  return launch_kernel(k[prec][a.lloss ? 1 : 0][a.O <= 2 ? 0 : 1][it_index(a.F)], dim3(gx, (unsigned)nb), 256, 0,
                "last_fwd", st, a);
}

// One hidden-layer GEMM launch (MODE_FWD or MODE_DX). Persistent grid: one 512-thread workgroup
// per CU (~131 KB LDS each), spread over weight sets and 256-column tiles.
dim3 nt_grid(int64_t rows, int K, int N, int64_t nb, int prec) {
  const int ntn = (int)cdiv(N, 256);
  const int kmax = K <= 256 ? 256 : 512;  // siren_mlp_check bounds K by 512 (bf16) / 256 (f32)
  const int bm = prec == kPrecBF16 ? 64 * 256 / kmax : 32;
  const int64_t tiles = cdiv(rows, bm);
  const int64_t per = std::max<int64_t>(1, 256 / std::max<int64_t>(1, nb * ntn));
  return dim3((unsigned)std::min<int64_t>(tiles, per), (unsigned)nb, (unsigned)ntn);
}

dim3 ring_grid(int64_t rows, int64_t nb) {
  const int64_t tiles = cdiv(rows, RING_BM);
  const int64_t per = std::max<int64_t>(1, 256 / nb);
  return dim3((unsigned)std::min<int64_t>(tiles, per), (unsigned)nb, 1);
}

// The tiled GEMM kernels, [MODE_*][K > 256]; the bf16 input gradient also with the output layer
// (top) and / or the first layer (bot) folded in (both at once is never planned: a stack with one
// hidden layer takes one fusion only).
const Kernel<NTArgs>& nt_kernel(int prec, int mode, int K, bool top = false, bool bot = false) {
  static const Kernel<NTArgs> f32[4][2] = {{SIREN_K(nt_f32_kernel<0, 256>), SIREN_K(nt_f32_kernel<0, 512>)},
                                           {SIREN_K(nt_f32_kernel<1, 256>), SIREN_K(nt_f32_kernel<1, 512>)},
                                           {SIREN_K(nt_f32_kernel<2, 256>), SIREN_K(nt_f32_kernel<2, 512>)},
                                           {SIREN_K(nt_f32_kernel<3, 256>), SIREN_K(nt_f32_kernel<3, 512>)}};
#define SIREN_NT(MODE, TOP, BOT) {SIREN_K(nt_bf16_kernel<MODE, 256, TOP, BOT>), SIREN_K(nt_bf16_kernel<MODE, 512, TOP, BOT>)}
  static const Kernel<NTArgs> bf16[4][2] = {SIREN_NT(0, false, false), SIREN_NT(1, false, false),
                                            SIREN_NT(2, false, false), SIREN_NT(3, false, false)};
  static const Kernel<NTArgs> fused[3][2] = {SIREN_NT(1, false, true), SIREN_NT(1, true, false), SIREN_NT(1, true, true)};
#undef SIREN_NT
  const int k = K <= 256 ? 0 : 1;
  if (prec != kPrecBF16) return f32[mode][k];
  return top || bot ? fused[2 * top + bot - 1][k] : bf16[mode][k];
}
const char* const kNTNames[] = {"nt_gemm fwd", "nt_gemm dx", "nt_gemm first", "nt_gemm dx-input"};

// Which kernel a hidden layer's plain GEMM (MODE_FWD / MODE_DX, nothing folded in) runs on: the
// tiled kernels above, fp32 on the row-stacked tile (jvp_tan_kernel JT_FWD / JT_DX: 128 rows x all
// 256 output features per workgroup, 8 waves; nt_f32_kernel's products, K order and epilogues), or
// the bf16 256x256 input gradient on the ring kernel.
enum NTForm { NT_TILED, NT_ROWS, NT_RING };
NTForm nt_form(int prec, int mode, int K, int N) {
  if (mode != MODE_FWD && mode != MODE_DX) return NT_TILED;
  if (prec == kPrecF32 && g_f32_rows && K % JNT_KC == 0 && K <= 512 && N <= JADJ_BN) return NT_ROWS;
  if (prec == kPrecBF16 && mode == MODE_DX && g_dx_ring && K == 256 && N == 256) return NT_RING;
  return NT_TILED;
}
const Kernel<JTanArgs> kRows[2] = {SIREN_K(jvp_tan_kernel<0, 2, 1>), SIREN_K(jvp_tan_kernel<0, 2, 2>)};  // JT_FWD, JT_DX
dim3 rows_grid(int64_t rows, int64_t nb) { return dim3((unsigned)cdiv(rows, 2 * JADJ_ROWS), (unsigned)nb); }
int launch_rows(int mode, const NTArgs& a, int64_t nb, int kclass, hipStream_t st) {
  JTanArgs t;
  memset(&t, 0, sizeof(t));
  t.P = mode == MODE_FWD ? a.A : a.Paux;
  t.U = mode == MODE_DX ? (const float*)a.A : nullptr;
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
  return launch_kernel(kRows[mode == MODE_FWD ? 0 : 1], rows_grid(a.rows_per_batch, nb), 512, kclass,
                mode == MODE_FWD ? "f32 rows fwd" : "f32 rows dx", st, t);
}

// The GEMM of layer l as NTArgs: forward [rows, in] x W_l^T (layer 0: in padded to first_kp), or the
// input gradient [rows, out] x W_l. A, W, C: the operands as the kernel reads / writes them.
NTArgs nt_args(const siren_mlp_desc* d, const Geo& g, int l, bool fwd, const void* A, const void* W, void* C) {
  NTArgs a;
  memset(&a, 0, sizeof(a));
  const int in = fwd && l == 0 ? first_kp(d) : d->dims[l], out = d->dims[l + 1];
  a.A = A;
  a.W = W;
  a.C = C;
  a.rows_per_batch = g.rows;
  a.w_bstride = bstride(d, (int64_t)out * in);
  a.K = fwd ? in : out;
  a.N = fwd ? out : in;
  a.lda = fwd ? d->dims[l] : out;
  a.w0 = d->w0;
  if (fwd) {
    a.bias = d->bias[l];
    a.bias_bstride = bstride(d, out);
  }
  return a;
}

// The weight gradient of layer l as TNArgs: D = dZ_l, P = the layer's input, one slab per split.
TNArgs tn_args(const siren_mlp_desc* d, const Geo& g, int l, const void* D, const void* P, float* part,
               int64_t rows_per_split) {
  TNArgs a;
  memset(&a, 0, sizeof(a));
  a.D = D;
  a.P = P;
  a.part = part;
  a.rows_per_batch = g.rows;
  a.rows_per_split = rows_per_split;
  a.M = d->dims[l + 1];
  a.N = d->dims[l];
  a.split_stride = split_stride(g, (int64_t)a.M * a.N + a.M);
  a.w0 = d->w0;
  return a;
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
  if (L) set_loss(a, *L);
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
    NTArgs a = nt_args(d, g, 0, true, x, wbuf + lo.w_op_off[0], phase_buf(0));
    a.a_vec = (d->dims[0] % 4 == 0) && aligned16(x);
    if ((rc = launch_kernel(nt_kernel(PREC, MODE_FIRST, a.K), nt_grid(g.rows, a.K, a.N, g.nb, PREC), 512, 0,
                     kNTNames[MODE_FIRST], st, a)))
      return rc;
  } else {
    static const Kernel<FirstFwdArgs> k[2][2] = {{SIREN_K(first_fwd_kernel<0, 4>), SIREN_K(first_fwd_kernel<0, 16>)},
                                                 {SIREN_K(first_fwd_kernel<1, 4>), SIREN_K(first_fwd_kernel<1, 16>)}};
    FirstFwdArgs a;
    a.x = x;
    a.W = d->weight[0];
    a.b = d->bias[0];
    a.P = phase_buf(0);
    a.rows_per_batch = g.rows;
    a.w_bstride = bstride(d, (int64_t)d->dims[1] * d->dims[0]);
    a.b_bstride = bstride(d, d->dims[1]);
    a.C = d->dims[0];
    a.F = d->dims[1];
    a.w0 = d->w0;
    const unsigned gx = grid1d(g.rows * (a.F / 8), std::max<int64_t>(1, 4096 / g.nb));
    if ((rc = launch_kernel(k[PREC][a.C <= 4 ? 0 : 1], dim3(gx, (unsigned)g.nb), 256, 0, "first_fwd", st, a))) return rc;
  }
  // Hidden MFMA layers.
  for (int l = 1; l + 1 < g.L; ++l) {
    const NTArgs a = nt_args(d, g, l, true, phase_buf(l - 1),
                             PREC == kPrecBF16 ? (const void*)(wbuf + lo.w_op_off[l]) : (const void*)d->weight[l],
                             phase_buf(l));
    if (nt_form(PREC, MODE_FWD, a.K, a.N) == NT_ROWS)
      rc = launch_rows(MODE_FWD, a, g.nb, SIREN_KCLASS_FWD_GEMM, st);
    else
      rc = launch_kernel(nt_kernel(PREC, MODE_FWD, a.K), nt_grid(g.rows, a.K, a.N, g.nb, PREC), 512,
                  SIREN_KCLASS_FWD_GEMM, kNTNames[MODE_FWD], st, a);
    if (rc) return rc;
  }
  // Output layer (VALU).
  const int l = g.L - 1;
  LastFwdArgs a;
  memset(&a, 0, sizeof(a));
  a.P = phase_buf(l - 1);
  a.W = d->weight[l];
  a.b = d->bias[l];
  a.y = y;
  a.rows_per_batch = g.rows;
  a.w_bstride = bstride(d, (int64_t)d->dims[l + 1] * d->dims[l]);
  a.b_bstride = bstride(d, d->dims[l + 1]);
  a.F = d->dims[l];
  a.O = d->dims[l + 1];
  a.sine_out = d->outermost_linear ? 0 : 1;
  a.w0 = d->w0;
  if (L) set_loss(a, *L);
  return launch_last_fwd(PREC, a, g.nb, st);
}

// The backward pass as data: plan_backward decides every launch from the descriptor, the options
// and the alignment of x and dy; backward_impl walks the plan; siren_mlp_backward_plan prints it.
enum OutForm { OUT_LAST_BWD, OUT_TILED, OUT_RING };  // output layer: its own kernel, or folded into the top layer's
// first layer: folded into layer 1's ring / tiled kernels, wide MFMA (tn_dw RAW + MODE_DXLIN), or the VALU kernels
enum FirstForm { FIRST_RING, FIRST_TILED, FIRST_MFMA, FIRST_VALU };
enum Slab { SLAB_NONE, SLAB_PART, SLAB_PART2, SLAB_PARTL, SLAB_PARTB };  // Layout part / part2 / partL / partB
// where a launch's partial slabs are summed: a reduce launch right after it, the tail of the next
// pair launch, or a reduce_multi launch further down
enum Reduce { RED_NONE, RED_OWN, RED_NEXT_PAIR, RED_FLUSH };
enum Kern {
  K_XCOPY,         // x copied to a 16-byte aligned buffer (the ring kernels DMA it in 16-byte pieces)
  K_LAST_BWD,      // output layer on its own kernel
  K_REDUCE,        // the slabs out[0] summed into dW / db of their layer
  K_REDUCE_MULTI,  // the slabs of pair launch `src` summed in one launch
  K_PAIR,          // both gradients of a 256x256 layer on co-scheduled workgroup pairs (pair_ring_bf16_kernel): a
                   //   middle layer, the top layer with the output layer (top), layer 1 with the first layer (bot, rec)
  K_DW_TILED,      // weight gradient: 128x128-tile split-K kernel (top: output layer folded in; layer 0: raw x)
  K_DW_RING,       //   ring kernel: middle layer, top layer (top), layer 1 rebuilding P_0 from x (rec)
  K_DW_ROWS,       //   fp32 all-rows tile (jvp_tn2_kernel)
  K_DX_TILED,      // input gradient: tiled kernel (top / bot: output / first layer folded in; layer 0: MODE_DXLIN)
  K_DX_RING,       //   ring kernel: middle layer, top layer (top), layer 1 with the first layer (bot)
  K_DX_ROWS,       //   fp32 row-stacked tile (jvp_tan_kernel JT_DX)
  K_FIRST          // first layer on the VALU kernels (dx_out: the launch also, or only, writes dx)
};
using PairKernel = Kernel<NTArgs, TNArgs, ReduceMultiArgs>;
struct SlabUse {
  Slab buf;
  int layer;  // whose dW / db the slabs are partial sums of
  int64_t nsplit;
};
struct Launch {
  Kern kern;
  const void* fn;    // Kernel<Args>::fn of the Args the kind takes, and its profiler name
  const char* sym;
  const char* what;  // its name in a launch error
  int kclass, layer;
  int cur;           // which dZ buffer holds the layer's dZ (the other receives the input gradient)
  dim3 grid;
  unsigned block;
  bool top, bot, rec, dx_out;  // output / first layer folded in, P_0 rebuilt from x, writes dx (not dZ_{l-1})
  bool p_vec;        // layer-0 K_DW_TILED: x rows are read as 16-byte vectors (C % 4 == 0, aligned x)
  int64_t rows_per_split;
  SlabUse out[2];    // slabs written (K_REDUCE: read)
  Reduce reduce;
  int src = -1;      // K_REDUCE_MULTI: the pair launch it reduces; K_PAIR: the one its tail reduces (-1: none)
};
struct BwdPlan {
  const char* error = nullptr;  // a shape the kernels do not cover (SIREN_EINVAL)
  bool copy_x = false;
  OutForm out = OUT_LAST_BWD;
  FirstForm first = FIRST_VALU;
  int pair_roles = 3, stagger = 0;  // debug_pair_roles / dx_stagger, passed to the ring kernels
  int n = 0, npair = 0;  // launches; pair launches among them
  int cur = 0;  // (while planning) dZ ping-pong index holding dZ of the current layer
  Launch steps[6 * SIREN_MAX_LAYERS];  // (at most 5 per hidden layer and 7 around them)

  template <class K>
  Launch& add(Kern kern, const K& k, const char* what, int kclass, int layer, dim3 grid, unsigned block) {
    assert(n < (int)(sizeof(steps) / sizeof(steps[0])));
    return steps[n++] = Launch{kern, (const void*)k.fn, k.sym, what, kclass, layer, cur, grid, block};
  }
};

// dW_l then db_l: one partial slab
inline int64_t slab_elems(const siren_mlp_desc* d, int l) { return (int64_t)d->dims[l + 1] * d->dims[l] + d->dims[l + 1]; }

BwdPlan plan_backward(const siren_mlp_desc* d, const Geo& g, const Layout& lo, bool want_dx, bool x_aligned16,
                      bool dy_aligned16) {
  static const Kernel<int> kCopy = {nullptr, "hipMemcpyAsync"}, kReduce = {nullptr, "siren::reduce_kernel"};  // (not via fn)
  static const Kernel<ReduceMultiArgs> kReduceMulti = SIREN_K(reduce_multi_kernel);
  BwdPlan p;
  const int prec = g.prec, L = g.L, O = d->dims[L], C = d->dims[0], F0 = d->dims[1];
  const int c4 = std::min(C, 4) - 1, topo = O == 1 ? 1 : 2;  // table indices of the first- / output-layer fusions
  const bool bf16 = prec == kPrecBF16;
  const unsigned nb = (unsigned)g.nb;
  p.pair_roles = g_pair_roles;
  p.stagger = g_dx_stagger ? 1 : 0;
  // bf16-mode fusions (siren_gemm.hip TopArgs / BotArgs): the output layer's backward folds into
  // the top hidden layer's kernels, the first layer's weight gradient into the bottom one's.
  const bool fuse = bf16 && g_fused_backward && L >= 3;
  // P_0 not kept (p0_recompute): layer 1 runs on the ring kernels that rebuild it from x, whatever
  // the options say; they DMA x in 16-byte pieces, so a misaligned x is copied first.
  const bool rec = lo.p0_rec;
  p.copy_x = rec && !x_aligned16;
  if (p.copy_x) p.add(K_XCOPY, kCopy, "x copy", 0, 0, dim3(0, 0, 0), 0);
  const bool x16 = x_aligned16 || p.copy_x;
  const bool top_ok = fuse && d->outermost_linear && O <= TOP_MAXO && (g.rows * O) % 4 == 0 && g.rows * O >= 4 &&
                      dy_aligned16 && !(rec && L == 3);
  // output layer folded into the top layer's ring kernels (256x256 top layer below another layer)
  const bool ring_top = top_ok && g_ring_top && L >= 4 && d->dims[L - 1] == 256 && d->dims[L - 2] == 256;
  const bool top = ring_top || (top_ok && g_fuse_top && d->dims[L - 1] <= 256);
  // first-layer fusion: the ring kernel (256x256 bottom layer) also produces dx; the tiled kernel
  // only without dx. One hidden layer: the output-layer fusion only.
  const bool bot_ok = fuse && !wide_input(d) && C <= BOT_MAXC && (g.rows * C) % 4 == 0 && g.rows * C >= 4 && x16 &&
                      !(top && L == 3);
  const bool ring_bot = rec || (bot_ok && g_dx_ring && F0 == 256 && d->dims[2] == 256);
  const bool bot = ring_bot || (bot_ok && !want_dx && F0 <= 256);
  p.out = ring_top ? OUT_RING : top ? OUT_TILED : OUT_LAST_BWD;
  p.first = ring_bot ? FIRST_RING : bot ? FIRST_TILED : wide_input(d) ? FIRST_MFMA : FIRST_VALU;

  // a launch that writes s.nsplit slabs of dW / db[layer] to `part`, and the reduce launch that sums them
  auto writes = [&](Launch& a, int layer, const Split& s) {
    a.rows_per_split = s.rows_per_split;
    a.out[0] = {SLAB_PART, layer, s.nsplit};
    a.reduce = RED_OWN;
  };
  auto reduce_of = [&](int layer, Slab buf, int64_t nsplit) {
    p.add(K_REDUCE, kReduce, "reduce", 0, layer, dim3((unsigned)reduce_blocks(g.nb, slab_elems(d, layer))), 256).out[0] = {
        buf, layer, nsplit};
  };
  int pend = -1;  // the pair launch whose slabs are not reduced yet
  auto reduce_pending = [&] {
    if (pend < 0) return;
    int64_t blocks = 0;
    for (const SlabUse& u : p.steps[pend].out)
      if (u.buf != SLAB_NONE) blocks += reduce_blocks(g.nb, slab_elems(d, u.layer));
    p.steps[pend].reduce = RED_FLUSH;
    p.add(K_REDUCE_MULTI, kReduceMulti, "reduce_multi", 0, p.steps[pend].layer, dim3((unsigned)blocks), 256).src = pend;
    pend = -1;
  };

  if (!top) {  // output layer: dZ_{L-2}, dW_{L-1}, db_{L-1}
    static const Kernel<LastBwdArgs> k[2][2][3] = {{SIREN_IT(last_bwd_kernel, 0, 2), SIREN_IT(last_bwd_kernel, 0, 8)},
                                                   {SIREN_IT(last_bwd_kernel, 1, 2), SIREN_IT(last_bwd_kernel, 1, 8)}};
    const Split s = valu_split(g);
    writes(p.add(K_LAST_BWD, k[prec][O <= 2 ? 0 : 1][it_index(d->dims[L - 1])], "last_bwd", 0, L - 1,
                 dim3((unsigned)s.nsplit, nb), 256),
           L - 1, s);
    reduce_of(L - 1, SLAB_PART, s.nsplit);
  }
  // Hidden MFMA layers, top to bottom.
  for (int l = L - 2; l >= 1; --l) {
    const int M = d->dims[l + 1], N = d->dims[l];
    const bool is_top = top && l == L - 2, is_bot = bot && l == 1, rec1 = rec && l == 1, ring_t = ring_top && l == L - 2;
    const bool sq256 = bf16 && M == 256 && N == 256;
    if (sq256 && g_pair_ring && pair_ok(g) &&
        ((rec1 && !is_top) || (ring_t && !is_bot) || (!is_top && !is_bot && !rec1 && g_dw_ring && g_dx_ring))) {
      static const PairKernel mid[3] = {SIREN_K(pair_ring_bf16_kernel<0, false, false, 0, 0>),
                                        SIREN_K(pair_ring_bf16_kernel<0, false, false, 1, 0>),
                                        SIREN_K(pair_ring_bf16_kernel<0, false, false, 2, 0>)};
#define SIREN_PAIR_BOT(CC, DX) SIREN_K(pair_ring_bf16_kernel<CC, DX, true, 0, CC>)
      static const PairKernel low[2][4] = {SIREN_C4(SIREN_PAIR_BOT, false), SIREN_C4(SIREN_PAIR_BOT, true)};
#undef SIREN_PAIR_BOT
      // consecutive pair launches alternate slab buffers (the pending reduction reads the other
      // one); without a second buffer, or without the tail reduction, the pending one goes first
      if (!g_tail_reduce || lo.part2_off < 0) reduce_pending();
      const int64_t np = pair_count(g);
      const bool pb = rec1 && !is_top, pt = !pb && ring_t;
      Launch& s = p.add(K_PAIR, pb ? low[want_dx ? 1 : 0][c4] : mid[pt ? topo : 0], "pair_ring",
                        pb ? SIREN_KCLASS_PAIR_RING_BOT : pt ? SIREN_KCLASS_PAIR_RING_TOP : SIREN_KCLASS_PAIR_RING, l,
                        dim3((unsigned)(2 * np), nb), 512);
      s.top = pt;
      s.bot = s.rec = s.dx_out = pb;
      s.out[0] = {lo.part2_off >= 0 && (p.npair & 1) ? SLAB_PART2 : SLAB_PART, l, np};
      if (pt) s.out[1] = {SLAB_PARTL, L - 1, np};
      if (pb) s.out[1] = {SLAB_PARTB, 0, np};
      s.src = pend;
      if (pend >= 0) p.steps[pend].reduce = RED_NEXT_PAIR;
      pend = p.n - 1;
      ++p.npair;
      p.cur ^= 1;
      if (!pb) continue;
      reduce_pending();  // first layer done
      return p;
    }
    reduce_pending();  // the per-layer kernels below reuse `part`
    {                  // weight gradient
      static const Kernel<TNArgs> tiled[2][2] = {{SIREN_K(tn_dw_kernel<0, false, false>), {nullptr, nullptr}},
                                                 {SIREN_K(tn_dw_kernel<1, false, false>), SIREN_K(tn_dw_kernel<1, false, true>)}};
      static const Kernel<TNArgs> mid[3] = {SIREN_K(dw_ring_bf16_kernel<0, 0>), SIREN_K(dw_ring_bf16_kernel<0, 1>),
                                            SIREN_K(dw_ring_bf16_kernel<0, 2>)};
#define SIREN_DW_REC(CC, Z) SIREN_K(dw_ring_bf16_kernel<CC, Z>)
      static const Kernel<TNArgs> recs[4] = SIREN_C4(SIREN_DW_REC, 0);
#undef SIREN_DW_REC
      static const Kernel<JTNArgs> rows_k = SIREN_K(jvp_tn2_kernel<false>);
      const bool ring = rec1 || ring_t || (sq256 && g_dw_ring && !is_top);
      // fp32: jvp_tn2_kernel over the primal stream alone (S = 1: X = sin(P_{l-1}), D = dZ_l):
      // all 256 dW rows per workgroup, so each X element is formed once per launch
      const bool rows = !bf16 && g_f32_rows && jvp_tn2_ok(M, N);
      const Split s = ring ? dw_ring_split(g) : rows ? jtn2_split(g, g.rows, N) : tn_split(g, M, N);
      const unsigned ns = (unsigned)s.nsplit;
      Launch& a =
          ring   ? p.add(K_DW_RING, rec1 ? recs[c4] : mid[ring_t ? topo : 0], "tn_dw",
                         rec1 ? SIREN_KCLASS_DW_RING_REC : ring_t ? SIREN_KCLASS_DW_RING_TOP : SIREN_KCLASS_DW_RING, l,
                         dim3(ns, nb), 512)
          : rows ? p.add(K_DW_ROWS, rows_k, "tn_dw", SIREN_KCLASS_DW_GEMM, l, dim3((unsigned)cdiv(N, JTN2_BN), ns, nb), 512)
                 : p.add(K_DW_TILED, tiled[prec][is_top ? 1 : 0], "tn_dw", SIREN_KCLASS_DW_GEMM, l,
                         dim3((unsigned)(cdiv(M, TN_BM) * cdiv(N, TN_BN)), ns, nb), 256);
      writes(a, l, s);
      a.top = is_top;
      a.rec = rec1;
      if (is_top) a.out[1] = {SLAB_PARTL, L - 1, s.nsplit};
      reduce_of(l, SLAB_PART, s.nsplit);
      if (is_top) reduce_of(L - 1, SLAB_PARTL, s.nsplit);
    }
    {  // input gradient
#define SIREN_DX_BOT(CC, DX, REC) SIREN_K(dx_ring_bf16_kernel<CC, DX, REC, 0>)
      static const Kernel<NTArgs> low[2][2][4] = {{SIREN_C4(SIREN_DX_BOT, false, false), SIREN_C4(SIREN_DX_BOT, true, false)},
                                                  {SIREN_C4(SIREN_DX_BOT, false, true), SIREN_C4(SIREN_DX_BOT, true, true)}};
#undef SIREN_DX_BOT
      static const Kernel<NTArgs> mid[3] = {SIREN_K(dx_ring_bf16_kernel<0, false, false, 0>),
                                            SIREN_K(dx_ring_bf16_kernel<0, false, false, 1>),
                                            SIREN_K(dx_ring_bf16_kernel<0, false, false, 2>)};
      const NTForm form = is_top || is_bot ? NT_TILED : nt_form(prec, MODE_DX, M, N);
      const dim3 rg = ring_grid(g.rows, g.nb);
      Launch& a =
          is_bot && ring_bot ? p.add(K_DX_RING, low[rec1 ? 1 : 0][want_dx ? 1 : 0][c4], "dx_ring first-layer",
                                     SIREN_KCLASS_DX_RING_BOT, l, rg, 512)
          : ring_t           ? p.add(K_DX_RING, mid[topo], "dx_ring top", SIREN_KCLASS_DX_RING_TOP, l, rg, 512)
          : form == NT_RING  ? p.add(K_DX_RING, mid[0], "dx_ring", SIREN_KCLASS_DX_RING, l, rg, 512)
          : form == NT_ROWS
              ? p.add(K_DX_ROWS, kRows[1], "f32 rows dx", SIREN_KCLASS_DX_GEMM, l, rows_grid(g.rows, g.nb), 512)
              : p.add(K_DX_TILED, nt_kernel(prec, MODE_DX, M, is_top, is_bot), kNTNames[MODE_DX], SIREN_KCLASS_DX_GEMM, l,
                      nt_grid(g.rows, M, N, g.nb, prec), 512);
      a.top = is_top;
      a.bot = is_bot;
      a.rec = rec1;
      a.dx_out = is_bot && ring_bot;  // [rows, C] f32, or not written
      p.cur ^= 1;
      if (!is_bot) continue;
      a.out[0] = {SLAB_PART, 0, a.grid.x};  // one first-layer slab per workgroup; first layer done
      a.reduce = RED_OWN;
      reduce_of(0, SLAB_PART, a.grid.x);
      return p;
    }
  }
  reduce_pending();
  // First layer.
  if (wide_input(d)) {
    static const Kernel<TNArgs> raw[2] = {SIREN_K(tn_dw_kernel<0, true, false>), SIREN_K(tn_dw_kernel<1, true, false>)};
    const Split s = tn_split(g, F0, C);
    Launch& a = p.add(K_DW_TILED, raw[prec], "tn_dw first", 0, 0,
                      dim3((unsigned)(cdiv(F0, TN_BM) * cdiv(C, TN_BN)), (unsigned)s.nsplit, nb), 256);
    writes(a, 0, s);
    a.p_vec = C % 4 == 0 && x_aligned16;
    reduce_of(0, SLAB_PART, s.nsplit);
    if (want_dx)
      p.add(K_DX_TILED, nt_kernel(prec, MODE_DXLIN, F0), kNTNames[MODE_DXLIN], 0, 0, nt_grid(g.rows, F0, C, g.nb, prec), 512)
          .dx_out = true;
    return p;
  }
  static const Kernel<FirstBwdArgs> narrow[2][3] = {SIREN_IT(first_bwd_kernel, 0, 4), SIREN_IT(first_bwd_kernel, 1, 4)};
  static const Kernel<FirstBwdArgs> k16[2][2] = {{SIREN_K(first_bwd_kernel<0, 1, 16>), SIREN_K(first_bwd_kernel<0, 2, 16>)},
                                                 {SIREN_K(first_bwd_kernel<1, 1, 16>), SIREN_K(first_bwd_kernel<1, 2, 16>)}};
  static const Kernel<FirstBwdArgs> wide[2][2] = {{SIREN_K(first_bwd_wide_kernel<0, 0>), SIREN_K(first_bwd_wide_kernel<0, 16>)},
                                                  {SIREN_K(first_bwd_wide_kernel<1, 0>), SIREN_K(first_bwd_wide_kernel<1, 16>)}};
  static const Kernel<FirstBwdArgs> mfma = SIREN_K(first_bwd_wide_mfma_kernel), dxw = SIREN_K(first_dx_wide_kernel);
  const Split s = valu_split(g);
  const dim3 grid((unsigned)s.nsplit, nb);
  const bool mfma_ok = bf16 && F0 == 256 && s.rows_per_split % 32 == 0;
  // 5..16 inputs: the weight gradient without dx; the input gradient (bf16 mode) as its own MFMA launch
  const bool split_dx = C > 4 && F0 <= 256 && (!want_dx || (bf16 && F0 == 256));
  if (d->ff_B && !(mfma_ok && C > 4 && !want_dx)) {
    p.error = "fourier input: first-layer backward needs the bf16 wide MFMA path and no dx";
    return p;
  }
  Launch& a =
      d->ff_B    ? p.add(K_FIRST, mfma, "first_bwd_wide_mfma (fourier input)", 0, 0, grid, 256)  // forms the features itself
      : C <= 4   ? p.add(K_FIRST, narrow[prec][it_index(F0)], "first_bwd", 0, 0, grid, 256)
      : split_dx ? p.add(K_FIRST, mfma_ok ? mfma : wide[prec][C == 16 ? 1 : 0], want_dx ? "first_bwd_wide" : "first_bwd", 0,
                         0, grid, 256)
                 : p.add(K_FIRST, k16[prec][F0 <= 256 ? 0 : 1], "first_bwd", 0, 0, grid, 256);
  writes(a, 0, s);
  a.dx_out = want_dx && !split_dx;
  if (want_dx && split_dx) {
    Launch& x = p.add(K_FIRST, dxw, "first_bwd", 0, 0, dim3((unsigned)cdiv(cdiv(g.rows, 32), 4), nb), 256);
    x.rows_per_split = s.rows_per_split;
    x.dx_out = true;
  }
  reduce_of(0, SLAB_PART, s.nsplit);
  return p;
}

// The plan as text, one line per launch (siren_mlp_backward_plan).
std::string plan_text(const BwdPlan& p) {
  static const char* const outs[] = {"last_bwd", "tiled", "ring"};
  static const char* const firsts[] = {"ring", "tiled", "mfma", "valu"};
  static const char* const slabs[] = {"", "part", "part2", "partL", "partB"};
  static const char* const reds[] = {"", " reduce=own", " reduce=next_pair", " reduce=flush"};
  char buf[256];
  snprintf(buf, sizeof(buf), "# out=%s first=%s xcopy=%d launches=%d\n", outs[p.out], firsts[p.first], p.copy_x ? 1 : 0, p.n);
  std::string t = buf;
  for (int i = 0; i < p.n; ++i) {
    const Launch& s = p.steps[i];
    const SlabUse* u = s.kern == K_REDUCE_MULTI ? p.steps[s.src].out : s.out;
    int k = snprintf(buf, sizeof(buf), "%s class=%d layer=%d grid=(%u,%u,%u) block=%u", s.sym, s.kclass, s.layer, s.grid.x,
                     s.grid.y, s.grid.z, s.block);
    if (u[0].buf != SLAB_NONE) k += snprintf(buf + k, sizeof(buf) - k, " slab=%s", slabs[u[0].buf]);
    if (u[1].buf != SLAB_NONE) k += snprintf(buf + k, sizeof(buf) - k, "+%s", slabs[u[1].buf]);
    if (u[0].buf != SLAB_NONE) k += snprintf(buf + k, sizeof(buf) - k, " nsplit=%lld", (long long)u[0].nsplit);
    if (u[1].buf != SLAB_NONE) k += snprintf(buf + k, sizeof(buf) - k, "+%lld", (long long)u[1].nsplit);
    if (s.kern == K_DW_TILED && s.layer == 0) k += snprintf(buf + k, sizeof(buf) - k, " p_vec=%d", s.p_vec ? 1 : 0);
    snprintf(buf + k, sizeof(buf) - k, "%s\n", reds[s.reduce]);
    t += buf;
  }
  return t;
}
// A plan text into the caller's buffer, cut to fit and terminated; returns the bytes the whole text needs.
int64_t text_out(const std::string& t, char* out, int64_t cap) {
  if (out && cap > 0) {
    const size_t n = std::min<size_t>(t.size(), (size_t)cap - 1);
    memcpy(out, t.data(), n);
    out[n] = 0;
  }
  return (int64_t)t.size() + 1;
}

// One backward call's buffers, and the launcher of every kind of plan step.
struct BwdWalk {
  const siren_mlp_desc* d;
  const Geo& g;
  const Layout& lo;
  const BwdPlan& p;
  const float *x, *dy, *dy_scale;
  const char* saved;
  char* ws;
  float *const *dW, *const *db;
  float* dx;
  hipStream_t st;
  TopArgs ta;  // the output layer folded into the top hidden layer's kernels (zeros: it is not)

  const void* P(int l) const { return saved + lo.saved_off[l]; }
  char* dz(int k) const { return ws + lo.dz_off[k]; }
  float* slab(Slab s) const {
    const int64_t off[] = {0, lo.part_off, lo.part2_off, lo.partL_off, lo.partB_off};
    return (float*)(ws + off[s]);
  }
  void set_top() {
    memset(&ta, 0, sizeof(ta));
    if (p.out == OUT_LAST_BWD) return;
    const int L = g.L;
    ta.Ptop = P(L - 2);
    ta.dy = dy;
    ta.dy_scale = dy_scale;
    ta.WL = d->weight[L - 1];
    ta.wl_bstride = bstride(d, (int64_t)d->dims[L] * d->dims[L - 1]);
    ta.partL = slab(SLAB_PARTL);
    ta.partL_stride = split_stride(g, slab_elems(d, L - 1));
    ta.O = d->dims[L];
  }
  // the slabs launch i wrote, as the segments of a reduce_multi launch or of a pair launch's tail
  ReduceMultiArgs segments(int i) const {
    ReduceMultiArgs r;
    memset(&r, 0, sizeof(r));
    for (int k = 0; i >= 0 && k < 2 && p.steps[i].out[k].buf != SLAB_NONE; ++k) {
      const SlabUse& u = p.steps[i].out[k];
      const int64_t sz = slab_elems(d, u.layer);
      ReduceSeg& s = r.seg[r.nseg++];
      s.part = slab(u.buf);
      s.nsplit = (int)u.nsplit;
      s.split_stride = split_stride(g, sz);
      s.total = (int)(g.nb * sz);
      s.slab = (int)sz;
      s.n_first = (int)(sz - d->dims[u.layer + 1]);
      s.out0 = dW[u.layer];
      s.out1 = db[u.layer];
      s.blocks = (int)reduce_blocks(g.nb, sz);
    }
    return r;
  }
  template <class... Args>
  int go(const Launch& s, const Args&... a) const {
    return launch_kernel(Kernel<Args...>{(void (*)(Args...))s.fn, s.sym}, s.grid, s.block, s.kclass, s.what, st, a...);
  }
  TNArgs dw_args(const Launch& s) const {
    const int l = s.layer;
    TNArgs w = tn_args(d, g, l, dz(s.cur), l && !s.rec ? P(l - 1) : x, slab(s.out[0].buf), s.rows_per_split);
    if (s.rec) {  // P_0 rebuilt from x
      w.rec_W0 = d->weight[0];
      w.rec_w0_bstride = bstride(d, (int64_t)d->dims[1] * d->dims[0]);
      w.rec_b0 = d->bias[0];
      w.rec_b0_bstride = bstride(d, d->dims[1]);
    }
    w.p_vec = s.p_vec;
    w.top = ta;
    return w;
  }
  NTArgs dx_args(const Launch& s) const {
    const int l = s.layer;
    NTArgs a = nt_args(d, g, l, false, dz(s.cur), saved + lo.wt_op_off[l], s.dx_out ? (void*)dx : dz(s.cur ^ 1));
    a.Paux = s.rec || l == 0 ? nullptr : P(l - 1);
    a.top = ta;
    a.stagger = p.stagger;
    if (s.bot) {  // the first layer folded in: its slabs are the launch's layer-0 ones
      const SlabUse& u = s.out[1].buf != SLAB_NONE ? s.out[1] : s.out[0];
      a.bot.x = x;
      a.bot.W0 = d->weight[0];
      a.bot.w0_bstride = bstride(d, (int64_t)d->dims[1] * d->dims[0]);
      a.bot.b0 = d->bias[0];
      a.bot.b0_bstride = bstride(d, d->dims[1]);
      a.bot.part = slab(u.buf);
      a.bot.split_stride = split_stride(g, slab_elems(d, 0));
      a.bot.C = d->dims[0];
    }
    return a;
  }

  int run(const Launch& s) {
    const int l = s.layer;
    switch (s.kern) {
      case K_XCOPY:
        if (hipMemcpyAsync(ws + lo.xcopy_off, x, g.total * d->dims[0] * sizeof(float), hipMemcpyDeviceToDevice, st) !=
            hipSuccess)
          return fail(SIREN_ELAUNCH, "x copy: %s", hipGetErrorString(hipGetLastError()));
        x = (const float*)(ws + lo.xcopy_off);
        return SIREN_OK;
      case K_LAST_BWD: {
        LastBwdArgs a;
        a.P = P(l - 1);
        a.W = d->weight[l];
        a.b = d->bias[l];
        a.dy = dy;
        a.dy_scale = dy_scale;
        a.dZ = dz(s.cur);
        a.part = slab(s.out[0].buf);
        a.rows_per_batch = g.rows;
        a.rows_per_split = s.rows_per_split;
        a.F = d->dims[l];
        a.O = d->dims[l + 1];
        a.split_stride = split_stride(g, slab_elems(d, l));
        a.w_bstride = bstride(d, (int64_t)a.O * a.F);
        a.b_bstride = bstride(d, a.O);
        a.sine_out = d->outermost_linear ? 0 : 1;
        a.w0 = d->w0;
        return go(s, a);
      }
      case K_REDUCE: {
        const int64_t sz = slab_elems(d, l);
        return launch_reduce(slab(s.out[0].buf), s.out[0].nsplit, split_stride(g, sz), g.nb, sz, sz - d->dims[l + 1], dW[l],
                             db[l], st);
      }
      case K_REDUCE_MULTI:
        return go(s, segments(s.src));
      case K_PAIR: {
        TNArgs w = dw_args(s);
        NTArgs a = dx_args(s);
        w.pair_roles = p.pair_roles;
        w.prof = a.prof = ring_profile_next();
        return go(s, a, w, segments(s.src));  // (the previous pair launch's slabs: reduced in this one's tail)
      }
      case K_DW_TILED:
      case K_DW_RING:
        return go(s, dw_args(s));
      case K_DW_ROWS: {
        const TNArgs w = dw_args(s);
        JTNArgs j;
        memset(&j, 0, sizeof(j));
        j.D = w.D;
        j.P = w.P;
        j.part = w.part;
        j.N = g.rows;
        j.rows_per_split = s.rows_per_split;
        j.split_stride = w.split_stride;
        j.S = 1;
        j.M = w.M;
        j.Kin = w.N;
        j.w0 = d->w0;
        return go(s, j);
      }
      case K_DX_TILED:
      case K_DX_RING:
        return go(s, dx_args(s));
      case K_DX_ROWS:
        return launch_rows(MODE_DX, dx_args(s), g.nb, s.kclass, st);
      case K_FIRST: {
        FirstBwdArgs a;
        memset(&a, 0, sizeof(a));
        a.dZ = dz(s.cur);
        a.x = x;
        a.ffB = d->ff_B;
        a.ffin = d->ff_B ? d->ff_in : 0;
        a.W = d->weight[0];
        a.dx = s.dx_out ? dx : nullptr;
        a.part = slab(SLAB_PART);
        a.rows_per_batch = g.rows;
        a.rows_per_split = s.rows_per_split;
        a.F = d->dims[1];
        a.C = d->dims[0];
        a.split_stride = split_stride(g, slab_elems(d, 0));
        a.w_bstride = bstride(d, (int64_t)a.F * a.C);
        return go(s, a);
      }
    }
    return SIREN_OK;
  }
};

int backward_impl(const siren_mlp_desc* d, const float* x, const float* dy, const char* saved, char* ws,
                  float* const* dW, float* const* db, float* dx, hipStream_t st, const float* dy_scale = nullptr) {
  const Geo g = geo_of(d);
  const Layout lo = layout_of(d);
  const BwdPlan p = plan_backward(d, g, lo, dx != nullptr, aligned16(x), aligned16(dy));
  if (p.error) return fail(SIREN_EINVAL, "%s", p.error);
  BwdWalk w{d, g, lo, p, x, dy, dy_scale, saved, ws, dW, db, dx, st, {}};
  w.set_top();
  for (int i = 0; i < p.n; ++i)
    if (int rc = w.run(p.steps[i])) return rc;
  return SIREN_OK;
}

}  // namespace
