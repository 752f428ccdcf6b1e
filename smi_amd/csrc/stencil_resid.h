// stencil_resid.h -- the residual variants of the single-step launches
// (stencil.hip), used by smi_stencil_step_residual and the checked step of
// smi_stencil_solve (stencil_run.cpp).
#pragma once

#include "stencil_common.h"

namespace smi {

// launch_sweep / launch_edge with resid == nullptr; else the same kernels'
// residual instantiations, which also max-accumulate the bit pattern of
// |out - in| over the cells they store into *resid (one atomic per wave).
int launch_sweep_res(const SweepArgs &a, unsigned int *resid, hipStream_t s);
int launch_edge_res(const SweepArgs &a, int side_mask, unsigned int *resid, hipStream_t s);

}  // namespace smi
