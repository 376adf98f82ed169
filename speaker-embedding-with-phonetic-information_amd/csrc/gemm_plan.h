// Where a spliced-GEMM launch is decided: which kernel, its grid and LDS, the lanes and workgroup groups of a persistent
// launch, the K-walk groups the kernel reads.  Plain host code - no HIP runtime call, no pointer of GemmArgs is dereferenced -
// so a plan can be asked for without a device, at any CU count (xv_plan_gemm); the launcher (kernels.hip) only carries it out.
#pragma once
#include <stddef.h>

#include "kernels.h"

namespace xv {

// Everything the decision reads from the process and the device.
struct GemmPolicy {
  int cus;           // CUs of the device; the others are the XVEC_DEBUG knobs (knobs.h)
  int variant;       // gemm_variant: 1 = 128x128 / 2-stage, 2 = 256x128 / 3-stage ring, 4 = stream-K (persistent; falls back to 2 / 1
                     // when the launch has too few tiles or an odd shape), 0 = by precision and K length (default, see PlanGemm)
  int sk_max_mf;     // sk_mf: frame fragments per wave of stream-K: 8 (512-row tiles) where the LDS allows, else 4; 4 forces the 256-row tiles
  int sk_max_lanes;  // sk_lanes: most column lanes of a stream-K launch (4, 2, 1)
  int stagger_pct;   // gemm_stagger: start-stagger window of the 256x128 variant, percent of the modelled tile time
};
// The fields clamped as the knobs are (a value outside a knob's list is its default).
GemmPolicy MakeGemmPolicy(int cus, int variant, int sk_mf, int sk_lanes, int stagger_pct);
inline GemmPolicy DefaultGemmPolicy(int cus) { return MakeGemmPolicy(cus, 0, 8, 4, 85); }
// The knobs of this process (read once: thread-safe, and a process does not change its mind) with the CU count of the
// CURRENT device (kernels.hip).
GemmPolicy CurrentGemmPolicy();

enum GemmKernel : int {
  kGemmTile = 0,    // tdnn_gemm_kernel<PREC, EPI>
  kGemmV2 = 1,      // tdnn_gemm_kernel_v2<PREC, EPI>
  kGemmSk = 2,      // tdnn_gemm_kernel_sk<PREC, EPI, mf>
  kGemmP8 = 3,      // tdnn_gemm_kernel_p8<PREC, EPI>
  kGemmSplitK = 4,  // tdnn_gemm_kernel<PREC, kEpiSplitK> followed by splitk_reduce_kernel<PREC, EPI>
};

struct GemmPlan {
  bool ok;              // false: the launch is refused (nothing else is meaningful)
  int kernel;           // GemmKernel
  int precision, epilogue;
  int mf;               // kGemmSk: 4 or 8, else 0
  int grid_x, grid_y, block;
  int lds;              // dynamic LDS bytes
  size_t sk_ws_bytes;   // stream-K workspace (kGemmSk, kGemmP8), else 0
  GemmArgs args;        // the caller's arguments + what the kernel reads of the plan (sk_ws, sk_flags, sk_epoch, sk_error: the launcher's)
};
GemmPlan PlanGemm(const GemmArgs& a, int precision, int epilogue, const GemmPolicy& policy);
// The instantiation a plan launches as last_gemm_kernel() spells it, e.g. "tdnn_gemm_kernel_sk<fp16mx,act,8>"
void GemmKernelName(const GemmPlan& p, char* buf, size_t cap);

}  // namespace xv
