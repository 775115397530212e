// rt_common.hip — what every host part of the runtime shares: the error message, size helpers, the
// row geometry of a descriptor, the execution options and their table, launch checks and the optional
// per-kernel-class timing. Included by siren_runtime.hip (not a translation unit of its own).
namespace {

thread_local std::string g_err;

int fail(int code, const char* fmt, ...) __attribute__((format(printf, 2, 3)));
int fail(int code, const char* fmt, ...) {
  char buf[512];
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(buf, sizeof(buf), fmt, ap);
  va_end(ap);
  g_err = buf;
  return code;
}

inline int64_t align_up(int64_t v, int64_t a) { return (v + a - 1) / a * a; }
inline int64_t cdiv(int64_t a, int64_t b) { return (a + b - 1) / b; }
inline bool aligned16(const void* p) { return ((uintptr_t)p & 15) == 0; }

// Effective batching: shared weights collapse every row into one weight set.
struct Geo {
  int L;
  int64_t nb;     // weight sets
  int64_t rows;   // rows per weight set
  int64_t total;  // all rows
  int prec;
  int64_t phase_sz, grad_sz, op_sz;
};

Geo geo_of(const siren_mlp_desc* d) {
  Geo g;
  g.L = d->num_layers;
  if (d->weights_batched) {
    g.nb = d->batch;
    g.rows = d->rows_per_batch;
  } else {
    g.nb = 1;
    g.rows = d->batch * d->rows_per_batch;
  }
  g.total = d->batch * d->rows_per_batch;
  g.prec = d->prec;
  g.phase_sz = d->prec == SIREN_PREC_BF16 ? 2 : 4;
  g.grad_sz = g.phase_sz;
  g.op_sz = g.phase_sz;
  return g;
}

// Execution options (siren_config_set / siren_config_get). The launch code reads these plain
// globals; kOptions below is the one list of their names, ranges and defaults, and writes the
// defaults into them when the library is loaded.
int g_fused_forward, g_fused_backward, g_ring_top, g_fuse_top, g_fwd_pipe, g_fwd_reg, g_freg_magic, g_dx_ring,
 g_dw_ring, g_pair_ring, g_pair_roles, g_dx_stagger, g_tail_reduce, g_jvp_adj, g_jvp_tan, g_jvp_tn2,
    g_f32_rows, g_wrw_dma, g_conv_dma, g_keep_p0, g_fwd_dbg;

struct Option {
  const char* name;
  int* var;
  int min, max, def;
};
const Option kOptions[] = {
    {"fused_forward", &g_fused_forward, 0, 1, 1},    // bf16 fused shapes (fused_shape): the forward as one kernel
    {"fused_backward", &g_fused_backward, 0, 1, 1},  // bf16 backward: first / output layer folded into their neighbours
    {"fuse_output_layer", &g_fuse_top, 0, 1, 0},     // output-layer fusion into the tiled kernels: slower than last_bwd, off
    {"ring_output_fusion", &g_ring_top, 0, 1, 1},    // output layer folded into the top 256x256 layer's ring kernels
    {"fused_forward_pipe", &g_fwd_pipe, 0, 1, 1},  // fused forward: half-tile MFMA/VALU pipelined kernel
    {"fused_forward_reg", &g_fwd_reg, 0, 1, 1},    // fused forward: activations resident in registers (siren_fwdreg.hip)
    // its hidden layers in the magic epilogue form where the weights allow it: off by default — the
    // forward ~3-5 % faster, but the bf16 PSNR at step 500 lands 0.085 dB under the reference (54.891
    // vs 54.967 dB fract form; both forms track to 0.01 dB up to step 480, then the spiky regime)
    {"freg_magic", &g_freg_magic, 0, 1, 0},
    {"dx_ring", &g_dx_ring, 0, 1, 1},      // 256x256 input-gradient layers on the 4-stage ring kernel
    {"dw_ring", &g_dw_ring, 0, 1, 1},      // 256x256 weight-gradient layers on the 4-stage ring kernel
    {"pair_ring", &g_pair_ring, 0, 1, 1},  // both gradients of a ring layer in one launch (pair_ring_bf16_kernel)
    {"debug_pair_roles", &g_pair_roles, 0, 3, 3},  // debug timing: which pair_ring roles run (results are wrong unless 3)
    {"dx_stagger", &g_dx_stagger, 0, 1, 0},  // middle/top input-gradient ring: staggered wave halves (slower: +5-9 us/step)
    {"pair_tail_reduce", &g_tail_reduce, 0, 1, 1},  // a pair launch reduces the previous pair launch's slabs (no reduce launch)
    {"jvp_adj", &g_jvp_adj, 0, 1, 1},    // analytic-derivative backward: adjoint GEMM + combine in one launch (jvp_adj_kernel)
    {"jvp_tan", &g_jvp_tan, 0, 1, 1},    // tangent streams of a hidden layer stacked by row (jvp_tan_kernel)
    {"jvp_tn2", &g_jvp_tn2, 0, 1, 1},    // fp32 analytic-derivative weight gradients on jvp_tn2_kernel
    {"f32_rows", &g_f32_rows, 0, 1, 1},  // fp32 hidden layers' forward / input gradient on the row-stacked tile
    // the 5x5 weight-gradient convolution's chunks filled by LDS-DMA (conv_wrw_k5_kernel DMA): 2 is 128-pixel
    // chunks where W allows, C4 -0.33..-0.52 ms/step (profiles/r6_ab_wrw_128px.txt); the DMA fill itself C4 -0.05 ms/step,
    // 5 of 6 one-box pairs (profiles/r6_ab_wrw_dma.txt); 3: the other shapes' weight gradients too
    {"wrw_dma", &g_wrw_dma, 0, 3, 2},
    // the 5x5 encoder convolutions' stages: 0 register staging, 1 LDS-DMA, 2 LDS-DMA with per-workgroup
    // source offsets (conv_fwd_k5_kernel DMA; 2 is C4 -2 %, profiles/r6_ab_conv_dma2.txt)
    {"conv_dma", &g_conv_dma, 0, 2, 2},
    {"debug_keep_p0", &g_keep_p0, 0, 1, 0},   // debug: fused shapes keep P_0 (the stored-P_0 path, see p0_recompute)
    {"debug_fwd_skip", &g_fwd_dbg, 0, 31, 0},  // debug timing: fused_fwd_pipe_kernel skip bits (results wrong unless 0)
};
[[maybe_unused]] const int g_options_defaulted = [] {
  for (const Option& o : kOptions) *o.var = o.def;
  return 0;
}();

const Option* find_option(const char* key) {
  for (const Option& o : kOptions)
    if (key && strcmp(key, o.name) == 0) return &o;
  return nullptr;
}

// The two pointer-valued options (device addresses; set-only, siren_config_get answers -1).
long long* g_ring_prof = nullptr;   // debug_ring_profile: pair_ring segment cycle counters, one block per launch
int g_ring_prof_n = 0;              // (launches counted since debug_ring_profile was set)
long long* g_fused_prof = nullptr;  // debug_fused_profile: per-workgroup phase cycle counters of the fused forward
inline long long* ring_profile_next() {  // the next pair launch's counter block (null: profiling is off)
  return g_ring_prof ? g_ring_prof + (int64_t)(g_ring_prof_n++) * 256 * 8 * RING_NPROF : nullptr;
}

// The buffer checks of the stack entry points (siren_mlp_*, siren_jvp_*): the saved buffer (a backward
// pass requires it, a forward pass may go without) and the workspace hold what the layout needs.
int check_buffers(const void* saved, int64_t saved_bytes, int64_t saved_need, bool saved_required,
                  const void* workspace, int64_t workspace_bytes, int64_t workspace_need) {
  if (saved_required ? (!saved || saved_bytes < saved_need) : (saved && saved_bytes < saved_need))
    return fail(SIREN_ENOSPACE, "saved buffer %lld < %lld bytes", (long long)saved_bytes, (long long)saved_need);
  if (workspace_bytes < workspace_need || !workspace)
    return fail(SIREN_ENOSPACE, "workspace %lld < %lld bytes", (long long)workspace_bytes,
                (long long)workspace_need);
  return SIREN_OK;
}

// The hand-off workspace of the loss kernels (siren_sse_workspace_bytes()): LOSS_SLOTS sums, then the
// counter.
void loss_workspace_slice(void* workspace, float** partial, unsigned** counter) {
  *partial = (float*)workspace;
  *counter = (unsigned*)((char*)workspace + LOSS_SLOTS * 4);
}

int check_launch(const char* what) {
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) return fail(SIREN_ELAUNCH, "%s: %s", what, hipGetErrorString(e));
  return SIREN_OK;
}

// Optional per-kernel-class timing (bench / profiling only): while enabled, every launch of the
// selected class is bracketed by a hipEventRecord pair on its own stream.
struct Timing {
  int cls = 0;
  int cap = 0;
  int used = 0;
  hipEvent_t* ev = nullptr;
};
Timing g_timing;

inline void tmark_begin(int cls, hipStream_t st) {
  if (g_timing.cls == cls && g_timing.used < g_timing.cap)
    (void)hipEventRecord(g_timing.ev[2 * g_timing.used], st);
}
inline void tmark_end(int cls, hipStream_t st) {
  if (g_timing.cls == cls && g_timing.used < g_timing.cap) {
    (void)hipEventRecord(g_timing.ev[2 * g_timing.used + 1], st);
    ++g_timing.used;
  }
}

inline unsigned grid1d(int64_t work, int64_t cap = 4096) {
  return (unsigned)std::max<int64_t>(1, std::min<int64_t>(cdiv(work, 256), cap));
}
}  // namespace

extern "C" {

const char* siren_last_error(void) { return g_err.c_str(); }

int siren_timing_enable(int kernel_class, int max_launches) {
  siren_timing_disable();
  if (kernel_class <= 0 || max_launches <= 0) return SIREN_OK;
  g_timing.ev = new hipEvent_t[2 * (size_t)max_launches];
  for (int i = 0; i < 2 * max_launches; ++i) {
    if (hipEventCreate(&g_timing.ev[i]) != hipSuccess) {
      for (int k = 0; k < i; ++k) (void)hipEventDestroy(g_timing.ev[k]);
      delete[] g_timing.ev;
      g_timing = Timing();
      return fail(SIREN_ELAUNCH, "hipEventCreate failed");
    }
  }
  g_timing.cls = kernel_class;
  g_timing.cap = max_launches;
  g_timing.used = 0;
  return SIREN_OK;
}

int siren_timing_collect(double* total_ms, int64_t* launches) {
  double tot = 0.0;
  for (int i = 0; i < g_timing.used; ++i) {
    if (hipEventSynchronize(g_timing.ev[2 * i + 1]) != hipSuccess)
      return fail(SIREN_ELAUNCH, "hipEventSynchronize failed");
    float ms = 0.f;
    if (hipEventElapsedTime(&ms, g_timing.ev[2 * i], g_timing.ev[2 * i + 1]) != hipSuccess)
      return fail(SIREN_ELAUNCH, "hipEventElapsedTime failed");
    tot += ms;
  }
  if (total_ms) *total_ms = tot;
  if (launches) *launches = g_timing.used;
  return SIREN_OK;
}

void siren_timing_disable(void) {
  if (g_timing.ev) {
    for (int i = 0; i < 2 * g_timing.cap; ++i) (void)hipEventDestroy(g_timing.ev[i]);
    delete[] g_timing.ev;
  }
  g_timing = Timing();
}

int siren_config_set(const char* key, int64_t value) {
  if (key && strcmp(key, "debug_ring_profile") == 0) {  // device pointer or 0
    g_ring_prof = (long long*)(intptr_t)value;
    g_ring_prof_n = 0;
    return SIREN_OK;
  }
  if (key && strcmp(key, "debug_fused_profile") == 0) {  // device pointer or 0
    g_fused_prof = (long long*)(intptr_t)value;
    return SIREN_OK;
  }
  const Option* o = find_option(key);
  if (!o || value < o->min || value > o->max)
    return fail(SIREN_EINVAL, "unknown option %s=%lld", key ? key : "(null)", (long long)value);
  *o->var = (int)value;
  return SIREN_OK;
}

int64_t siren_config_get(const char* key) {
  const Option* o = find_option(key);
  return o ? *o->var : -1;
}

const char* siren_version(void) {
  static char buf[128];
  snprintf(buf, sizeof(buf), "siren_mri_amd gfx950 hip %d.%d", HIP_VERSION_MAJOR, HIP_VERSION_MINOR);
  return buf;
}

}  // extern "C"
