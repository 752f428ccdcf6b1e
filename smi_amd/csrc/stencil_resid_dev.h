// stencil_resid_dev.h -- device pieces every residual kernel shares: the bit
// pattern of |o - c|, the wave-wide unsigned maximum and the filtered post
// into the residual word (single step: stencil.hip; K-step passes:
// stencilk.h, stencil_bandk.h).
#pragma once

#include <hip/hip_runtime.h>

namespace smi {

// Bit pattern of |o - c|: one IEEE fp32 subtraction (subnormals kept), the
// sign bit cleared.  inf - inf and any NaN operand give a NaN pattern.
__device__ __forceinline__ unsigned int absdiff_bits(float o, float c) {
    return __builtin_bit_cast(unsigned int, __fsub_rn(o, c)) & 0x7fffffffu;
}

// Unsigned max over the 64 lanes of a wave, left in lane 63 (DPP; a lane
// without a source keeps the identity 0).  row_shr 1, 2, 4, 8 leave each
// row's max in its lane 15; row_bcast:15 folds rows 0 -> 1 and 2 -> 3,
// row_bcast:31 folds lane 31 into rows 2 and 3.  Call with all lanes active.
template <int CTRL, int ROW_MASK>
__device__ __forceinline__ unsigned int dpp_or0(unsigned int x) {
    return (unsigned int)__builtin_amdgcn_update_dpp(0, (int)x, CTRL, ROW_MASK, 0xf, false);
}
__device__ __forceinline__ unsigned int wave_max_u32(unsigned int v) {
    v = max(v, dpp_or0<0x111, 0xf>(v));
    v = max(v, dpp_or0<0x112, 0xf>(v));
    v = max(v, dpp_or0<0x114, 0xf>(v));
    v = max(v, dpp_or0<0x118, 0xf>(v));
    v = max(v, dpp_or0<0x142, 0xa>(v));
    v = max(v, dpp_or0<0x143, 0xc>(v));
    return v;
}

// A wave's maximum into the residual word (one lane calls this).  The word
// only grows, so a wave that cannot raise it sends no atomic: every atomic on
// the one address is a serial round trip to the memory side (~8 ns each; an
// 8192^2 step has ~22 k waves, and posting all of them took 0.265 ms against
// the plain step's 0.090, profiles/solve/).  The reading is a device-scope
// load; one that is stale can only be too low and costs an atomic that
// changes nothing.
__device__ __forceinline__ void resid_post(unsigned int *resid, unsigned int m) {
    if (m == 0) return;
    if (m > __hip_atomic_load(resid, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) atomicMax(resid, m);
}

}  // namespace smi
