// siren_runtime.hip — host-side orchestration behind the C ABI declared in include/siren_mri_amd.h.
// One call launches every kernel of a forward or a backward pass on the caller's stream; nothing
// here allocates, frees or synchronises. This translation unit is the kernels followed by the host
// parts, one per subsystem (rt_*.hip), included like the kernel files rather than linked.
#include <string>
#include <cstdio>
#include <cstring>
#include <algorithm>
#include <cstdarg>
#include <cassert>

#include "../../include/siren_mri_amd.h"
#include "siren_valu.hip"
#include "siren_gemm.hip"
#include "siren_jvp.hip"
#include "siren_fused.hip"
#define SIREN_FWDREG_DECL_ONLY  // its kernels: siren_fwdreg_inst.hip (a translation unit of its own)
#include "siren_fwdreg.hip"
#include "siren_adam.hip"
#include "siren_loss.hip"
#include "siren_kspace.hip"
#include "siren_kloss.hip"
#include "siren_sdf.hip"
#include "siren_wave.hip"
#include "siren_helmholtz.hip"
#include "siren_kfft.hip"
#include "siren_encoder.hip"
#include "siren_conv.hip"
#include "siren_f64.hip"
#include "siren_hyper.hip"

using namespace siren;

// Host parts, in dependency order: each has at most one anonymous namespace of helpers and one
// extern "C" block of entry points. rt_common.hip comes first (errors, geometry, options, timing);
// rt_mlp_entry.hip and rt_jvp.hip build on rt_mlp.hip; the others need rt_common.hip alone.
// The order is also the order in which the compiler first meets each kernel template's use, which
// is the order of the kernels in the code object (for the stack's kernels: the order of rt_mlp.hip's
// kernel tables). Reordering the parts or the tables is harmless but reorders the code object, so
// two builds are compared kernel by kernel (tools/compare_code_objects.py), not by hash.
#include "rt_common.hip"
#include "rt_mlp.hip"
#include "rt_hyper.hip"
#include "rt_f64.hip"
#include "rt_mlp_entry.hip"
#include "rt_jvp.hip"
#include "rt_encoder.hip"
#include "rt_loss.hip"
#include "rt_adam.hip"
