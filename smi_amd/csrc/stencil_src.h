// stencil_src.h -- the Jacobi update with a source term,
//   out = 0.25f * ((((S + W) + E) + N) + g),
// on the host side: the single-step launches (stencil.hip) and the depths of
// the fused source sweep (stencilk.h, "Source instantiations"), used by
// smi_stencil_step_source and the source runs of stencil_run.cpp.
#pragma once

#include "stencil_common.h"

namespace smi {

// The source sweep (sweepk_src_kernel<K>, stencilk_k<K>_src.hip) exists for
// K = 3 .. SWEEPK_SRC_MAX: the deepest pass (<= 12) whose kernel compiles for
// gfx950 with no scratch and two waves per SIMD (DESIGN.md section 5 has the
// register count of every K).
constexpr int SWEEPK_SRC_MAX = 9;
#define SMI_FOR_K_SRC(X) X(3) X(4) X(5) X(6) X(7) X(8) X(9)

// launch_sweep_res / launch_edge_res with src == nullptr; else the same
// kernels' source instantiations (g read at the cell's own address of src),
// plain (resid == nullptr) or residual.
int launch_sweep_src(const SweepArgs &a, const float *src, unsigned int *resid, hipStream_t s);
int launch_edge_src(const SweepArgs &a, int side_mask, const float *src, unsigned int *resid, hipStream_t s);

// The bands of a multi-rank source pass (bandk_src_kernel<K>, bandk_k<K>_src.hip,
// K = 3 .. SWEEPK_SRC_MAX): launch_bandk with the source term.  src: this
// rank's tile of g; g_halo: g's depth-K staging (the layout of a.h), received
// once per K-phase.  max_waves / stop as launch_bandk.
int launch_bandk_src(int K, BandKArgs a, const HaloK &g_halo, const float *src, int max_waves, hipStream_t s,
                     hipEvent_t stop = nullptr);

}  // namespace smi
