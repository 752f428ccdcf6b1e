// stencilk.h -- K Jacobi steps per pass over HBM (deep temporal blocking).
//
// Same per-cell arithmetic as every other stencil kernel here
// (stencil_smi.cl:153-156, global-edge cells copied per :143-151), applied K
// times inside one streaming pass.  Each wave owns a 256-column window of the
// input and walks it down a block of rows; every incoming input row advances
// a pipeline of K levels (level l lags l rows behind the input) and only
// level K is stored.  The window is 256 input columns wide but stores only
// the central 256-2KC (KC = K rounded up to whole float4 lanes): each level
// loses one valid column per side, so adjacent windows overlap by 2KC
// columns instead of fetching strip-edge extras (no cross-lane broadcasts).
// HBM traffic per pass is that of a single step, so the algorithmic
// 8 B/cell/step move up to K times faster.
//
// Register pipeline.  Level l keeps its last three rows in a 3-slot ring,
// slot = (input row index) mod 3; the loop body covers 6 input rows (two
// batches of 3, each batch's loads issued one batch ahead), so every slot
// index is a compile-time constant and no value is ever moved between
// registers.  The first 2K+1 input rows of a row block prime the pipeline;
// that prologue is unrolled with compile-time row indices and evaluates
// level l only from input row 2l on (the rows it must produce).  Global-edge
// copy rules cost nothing in the loop (ROW_* below); only the strips holding
// column 0 or Y-1 add a per-lane select.
//
// The kernel computes an arbitrary output rectangle [row_lo,row_hi) x
// [col_lo,col_hi) of the tile from input cells within K of it, so it is the
// single-tile sweep (whole tile) and, in multi-rank runs, the interior sweep
// that stays K rows / KC columns clear of every halo-facing side.
//
// Window apron: K >= 9 uses 16 columns (4 lanes) per side, so a window
// stores 224 columns = 7 whole 128-byte lines at a line-aligned offset
// (strip starts are multiples of 224 columns); smaller K keep the minimal
// float4 apron.  Round 2 (tools/sweepbench, 8192^2, K=12, ping-pong): the
// aligned apron + the pre-loop drain + the batch issue barrier run a pass in
// 0.117 ms vs 0.122 ms; the same grid streaming its loads and stores with no
// levels takes 0.106 ms and the levels alone (cache-resident inputs) 0.094
// ms, so the pass is now within ~10 % of its memory floor for this traffic
// (594 MB, 1.1x the 537 MB minimum: window and row-block aprons).
//
// Measured alternative (round 2, tools/sweepbench): an LDS-DMA input ring
// with hand-placed vmcnt waits and independent level groups reached 3
// waves/SIMD at 145 VGPRs but ran 0.129 ms per 12-step pass at 8192^2 vs
// 0.110 ms for this kernel in the same harness (2 waves/SIMD; single-buffer
// timing): the per-step ds_read + sched barriers turned
// the pass issue-stall bound (SQ_WAIT_INST_ANY 2.7x, VALU instructions 1.23x;
// profiles/r02/).
//
// Scaled levels (round 2).  x 0.25 is a power-of-two scaling, and IEEE
// round-to-nearest commutes with power-of-two scaling whenever nothing
// overflows and no rounding happens in the subnormal range.  So level l can
// carry u_l = 4^l v_l: u_l = ((S'+W')+E')+N' over the level-(l-1) values u,
// with no multiply (copied edge cells: u_l = 4 u_{l-1}), and the store
// writes u_K * 4^-K.  This is bit-identical to the reference arithmetic
// when every finite nonzero input of the wave's cone has magnitude in
// [2^-100, 2^101): then every level-l value is a multiple of 2^(-123-2l)
// (>= 2^-147 for l <= 12, so each x 0.25 of the reference order is exact,
// subnormal or not), and |u| < 2^(2K+101) <= 2^125 never overflows; Inf and
// NaN propagate the same either way.  Each wave checks its inputs as they
// stream in (frexp exponents) and a block that fails walks again with the
// exact arithmetic.  The multiply was 2 of the 12 VALU instructions of a
// level step (4 of 16.3 issue-slot units, packed ops at half rate).
//
// Residual instantiations (RES; sweepk_res_kernel<K>, one translation unit per
// K in stencilk_k<K>_res.hip).  When the level-K row of a cell is stored, the
// level-(K-1) row of the same cell is the centre slot of the last ring, so
// |x_T - x_{T-1}| of the pass's final step is one subtraction away: same
// loads, level arithmetic and stores as the plain instantiation, plus a
// per-lane running maximum of the bit pattern of |v_K - v_{K-1}| (the
// contract of smi_stencil_step_residual: one fp32 subtraction and fabs,
// subnormals kept, any NaN wins; a copied global-edge cell contributes
// |c - c|, which is 0, or NaN for an Inf / NaN cell).
//   Scaled walk: the ring holds u_K = 4^K v_K and u_{K-1} = 4^(K-1) v_{K-1}.
// Both are unscaled first, u_K * 4^-K (the store's own product) and
// u_{K-1} * 4^-(K-1), then subtracted.  Under the wave's guard both products
// are exact for the same reason the store's is: the scaled levels equal 4^l
// times the reference's level values EXACTLY (no overflow, every x 0.25 of the
// reference exact), the reference's v_l is itself an fp32 number (normal or
// subnormal, a multiple of 2^(-123-2l) >= 2^-149), and a power-of-two product
// whose exact result is representable is not rounded.  So the two operands of
// the subtraction are bit for bit the exact walk's, and so is the difference.
//   A wave whose guard fails walks its block again with the exact arithmetic
// and discards the scaled walk's maximum: the maximum lives in a register,
// is reset at the start of every walk and is posted only after a walk that
// counts -- at most one atomic per wave, behind the filter of the single-step
// kernels (resid_post).
//   Lanes and rows that do not store hold values of incomplete cones (apron
// lanes, rows outside [o0, o1), columns outside [col_lo, col_hi)): the
// store's hardware range check drops them, a register maximum must mask them
// out itself (`stl` and the row's in_block below).
//
// Source instantiations (SRC; sweepk_src_kernel<K>, one translation unit per K
// in stencilk_k<K>_src.hip, K = 3 .. SWEEPK_SRC_MAX of stencil_common.h).  Every
// level adds one operand per cell, out = 0.25 * ((((S + W) + E) + N) + g),
// g the cell of a second array `src` that travels as a kernel argument of its
// own (SweepKArgs and the plain kernels' code stay as they are).  Level l at
// input row t produces row t - l and needs the g row of that row, so a g row
// is loaded with input row t (same clamped row and column, same batches, also
// walking upwards) and stays live for K more inputs: the K rows t-1 .. t-K
// are held in registers, G[j] = g of row t-1-j, level l reads G[l-1].
//   Ring by rotation.  The 6-row loop body gives compile-time slots only to
// rings of 3 or 6; G is instead written as a shift register (every input row
// moves G[j-1] to G[j] and enters the new row at G[0]).  Inside the unrolled
// body the shifts are register renaming and cost nothing; what remains is the
// loop's back edge, where the K live rows return to their home registers: by
// count 4K v_mov per 6 input rows (2/3 of a v_mov per level per row, against
// ~14 VALU of level work; a per-row rotation would cost 4, a body unrolled to
// lcm(6, K) rows -- 66 at K = 11 -- would not fit the instruction cache).  What
// the compiler emits is somewhat more: sweepk_src_kernel<8> holds 1626
// v_mov_b32 and 172 64-bit moves for 1168 level steps (all 13 walks, their
// prologues and both loop halves: ~1.7 moves per level step, static count).
//   Exact arithmetic only: run<ROW, CE, false>.  Under scaled levels g would
// need a 4^(l-1) multiply per level, the multiply the scaling exists to
// remove; so there is no guard, no second walk and no note().  The ROW_TOP /
// ROW_BOT prologue copies and the CE column selects take the centre value, so
// g never reaches a global-edge cell (a NaN there does not leak), and rows or
// lanes of incomplete cones hold garbage with or without g.  There is no
// residual variant and no ring or pair kernel with a source.  Multi-rank source
// runs take single steps by default; under smi_stencil_set_source_bands(1) this
// kernel is the interior of their K-step passes (an interior rectangle's cone
// never leaves the tile, so it needs no g halo) beside bandk_src_kernel<K>
// (stencil_bandk.h), which reads g's depth-K halos (stencil_run.cpp).
#pragma once

#include <type_traits>

#include <hip/hip_ext.h>

#include "stencil_common.h"
#include "stencil_resid_dev.h"

#ifndef SMI_SWEEPK_SCALED
#define SMI_SWEEPK_SCALED 1
#endif
// experiment switches (tools/sweepbench builds; the library uses the defaults)
#ifndef SMI_SWEEPK_NT_LOADS
#define SMI_SWEEPK_NT_LOADS 0
#endif
#ifndef SMI_SWEEPK_TASK_ORDER
#define SMI_SWEEPK_TASK_ORDER 0
#endif
#ifndef SMI_SWEEPK_ALT
#define SMI_SWEEPK_ALT 0
#endif

namespace smi {

typedef float f32x2 __attribute__((ext_vector_type(2)));
typedef unsigned int u32x4 __attribute__((ext_vector_type(4)));

// lane i <- lane i-1 / i+1 (DPP wave_shr:1 / wave_shl:1).  Lanes 0 / 63 get
// whatever the hardware leaves (they only ever feed non-stored columns), so
// the destination needs no initialisation.
__device__ __forceinline__ float shr1_any(float v) {
    return __builtin_bit_cast(float, __builtin_amdgcn_mov_dpp(__builtin_bit_cast(int, v), 0x138, 0xf, 0xf, true));
}
__device__ __forceinline__ float shl1_any(float v) {
    return __builtin_bit_cast(float, __builtin_amdgcn_mov_dpp(__builtin_bit_cast(int, v), 0x130, 0xf, 0xf, true));
}

template <int I, int N, typename F>
__device__ __forceinline__ void static_for_from(F &f) {
    if constexpr (I < N) {
        f(std::integral_constant<int, I>{});
        static_for_from<I + 1, N>(f);
    }
}
// f(integral_constant<0>) ... f(integral_constant<N-1>), fully unrolled
template <int N, typename F>
__device__ __forceinline__ void static_for(F &&f) {
    static_for_from<0, N>(f);
}

// How a wave treats the global edge rows (stencil_smi.cl:143-151: rows 0 and
// X-1 are copied unchanged every step).
//   ROW_NONE  the wave's cone never reaches an edge row: no selects at all.
//   ROW_TOP   the wave's first output row is row 0 (walk downwards).  Row 0
//             of level l is produced at input t = K + l <= 2K, i.e. only in
//             the compile-time prologue, so the copy is a handful of
//             constant-index register moves there -- nothing in the loop.
//   ROW_BOT   the wave's last output row is row X-1: the wave walks UPWARDS
//             (N and S swap roles in the loads, never in the arithmetic
//             order), so row X-1 is again its prologue row t - l = K.
//   ROW_FULL  anything else that touches an edge row (blocks spanning both
//             edges, tiny row blocks from a tuning override): per-cell
//             row selects.
// Column edges add one per-lane select per level step: CE bit 0 for the
// strip holding column 0, bit 1 for the one holding column Y-1 (both only
// when one window spans the whole tile); every other wave runs the plain
// 12-instruction step.
enum { ROW_NONE = 0, ROW_TOP = 1, ROW_BOT = 2, ROW_FULL = 3, ROW_UP = 4 };
// ROW_UP: a ROW_NONE block that walks upwards (alternating walk directions,
// SMI_SWEEPK_ALT): row block rb walks down for even rb and up for odd rb, so
// the 2K apron rows two neighbouring blocks share are read by both at the
// same time (the ends of both walks, or the starts of both) and the second
// read hits L2.  Needs an even number of row blocks (launch_sweepk).
__host__ __device__ constexpr bool walks_up(int row) { return row == ROW_BOT || row == ROW_UP; }

template <int K, int U, bool RES = false, bool SRC = false>
struct SweepK {
    static_assert(K >= SWEEPK_MIN && K <= SWEEPK_MAX, "3 <= K <= 12");
    static_assert(!(RES && SRC), "the source sweep has no residual variant");
    static_assert(U % 3 == 0, "batch must be a multiple of the 3-slot ring");
    static constexpr int LL = sweepk_apron_lanes(K);  // lanes per window side that never store
    static constexpr int KC = 4 * LL;                  // window apron in columns (>= K)
    static constexpr int PRO = 2 * K + 1;   // prologue input rows (the last one stores the first output row)
    static constexpr bool kScaled = SMI_SWEEPK_SCALED != 0;
    static constexpr int kExpLo = -99, kExpHi = 101;      // frexp exponent range of the scaled walk's inputs
    static constexpr float kUnscale = 1.0f / (float)(1u << (2 * K));  // 4^-K (exact: K <= 12)
    static constexpr float kUnscalePrev = 4.0f * kUnscale;            // 4^-(K-1): level K-1 (RES)

    const float *__restrict__ in;
    float *__restrict__ out;
    int rows, cols;
    int o0, o1;       // output rows of this wave
    int r_begin;      // input row of t = 0 (o0 - K walking down, o1 - 1 + K walking up)
    int cl;           // clamped load column of this lane
    int voff;         // store byte offset in the row (out of range: no store)
    int row_bytes;
    bool copyL, copyR, gT, gB;
    float4 W[K][3];   // level 0..K-1, slot = input row index mod 3
    // RES only: the residual word, this lane's running maximum of the walk in
    // progress, and whether the lane stores (voff in range)
    unsigned int *resid;
    unsigned int rmax;
    bool stl;
    // SRC only: the source array and the g rows of the last K input rows,
    // G[j] = g of the row of input t-1-j (a shift register, see the header)
    const float *__restrict__ src;
    float4 G[SRC ? K : 1];

    // the g row that travels with input row t (same clamped row, same columns)
    template <bool REV>
    __device__ __forceinline__ float4 ldg(int t) const {
        const int r = min(max(REV ? r_begin - t : r_begin + t, 0), rows - 1);
        return *reinterpret_cast<const float4 *>(src + (size_t)r * cols + cl);
    }
    __device__ __forceinline__ void shift_g(const float4 &g) {
        static_for<K - 1>([&](auto J) { G[K - 1 - J] = G[K - 2 - J]; });
        G[0] = g;
    }

    template <bool REV>
    __device__ __forceinline__ float4 ld(int t) const {
        const int r = min(max(REV ? r_begin - t : r_begin + t, 0), rows - 1);
#if SMI_SWEEPK_NT_LOADS
        typedef float V4 __attribute__((ext_vector_type(4)));
        const V4 v = __builtin_nontemporal_load(reinterpret_cast<const V4 *>(in + (size_t)r * cols + cl));
        return make_float4(v.x, v.y, v.z, v.w);
#else
        return *reinterpret_cast<const float4 *>(in + (size_t)r * cols + cl);
#endif
    }

    // One level step of 4 cells per lane.  SC (scaled): the operands carry
    // 4^(l-1) times their level-(l-1) values, so the sum ((S+W)+E)+N is
    // 4^l times the level-l value and the x 0.25 is skipped (copied edge
    // cells are scaled by 4 instead); see "Scaled levels" above.
    // g: the cells' source term (SRC only; added last, before the multiply).
    template <int ROW, int CE, bool SC>
    __device__ __forceinline__ float4 step(int i, const float4 &n, const float4 &c, const float4 &s,
                                           const float4 &g) const {
        const float w = shr1_any(c.w);
        const float e = shl1_any(c.x);
        // ((S + W) + E) element-wise, then (+ N) (and x 0.25) on packed
        // pairs (v_pk_add_f32 / v_pk_mul_f32: same IEEE single-precision
        // round-to-nearest results as the scalar ops, never contracted)
        float b0 = __fadd_rn(__fadd_rn(s.x, w), c.y);
        float b1 = __fadd_rn(__fadd_rn(s.y, c.x), c.z);
        float b2 = __fadd_rn(__fadd_rn(s.z, c.y), c.w);
        float b3 = __fadd_rn(__fadd_rn(s.w, c.z), e);
        if constexpr (SC) {
            // opaque: keeps the instruction selector from re-pairing the
            // scalar adds into v_pk_add_f32 with register moves for operands
            asm("" : "+v"(b0), "+v"(b1), "+v"(b2), "+v"(b3));
        }
        f32x2 o01 = f32x2{b0, b1} + f32x2{n.x, n.y};
        f32x2 o23 = f32x2{b2, b3} + f32x2{n.z, n.w};
        if constexpr (SRC) {
            static_assert(!(SRC && SC), "the source sweep runs the exact arithmetic only");
            o01 = o01 + f32x2{g.x, g.y};
            o23 = o23 + f32x2{g.z, g.w};
        }
        if constexpr (!SC) {
            const f32x2 q = {0.25f, 0.25f};
            o01 = o01 * q;
            o23 = o23 * q;
        }
        float4 o;
        o.x = o01.x;
        o.y = o01.y;
        o.z = o23.x;
        o.w = o23.y;
        if constexpr (ROW == ROW_FULL) {
            static_assert(!SC, "ROW_FULL blocks run the exact arithmetic only");
            const bool rcopy = (i == 0 && gT) || (i == rows - 1 && gB);
            o.x = (rcopy || copyL) ? c.x : o.x;
            o.y = rcopy ? c.y : o.y;
            o.z = rcopy ? c.z : o.z;
            o.w = (rcopy || copyR) ? c.w : o.w;
        } else {
            if constexpr (CE & 1) o.x = copyL ? (SC ? c.x * 4.0f : c.x) : o.x;
            if constexpr (CE & 2) o.w = copyR ? (SC ? c.w * 4.0f : c.w) : o.w;
        }
        return o;
    }

    // level l (1..K) at input t from the level l-1 rows of inputs t-2, t-1, t
    // (slots PH+1, PH+2, PH mod 3).  Walking down, input t-2 is the upper
    // row (N) and input t the lower (S); walking up they swap.
    template <int ROW, int CE, bool SC, int PH>
    __device__ __forceinline__ float4 level(int l, int t, const float4 (&P)[3]) const {
        const float4 &g = G[SRC ? l - 1 : 0];  // the g row of row t - l (unused without SRC)
        if constexpr (walks_up(ROW))
            return step<ROW, CE, SC>(r_begin - (t - l), P[PH], P[(PH + 2) % 3], P[(PH + 1) % 3], g);
        else
            return step<ROW, CE, SC>(r_begin + t - l, P[(PH + 1) % 3], P[(PH + 2) % 3], P[PH], g);
    }

    // Scaled-path guard: frexp exponents of every input the wave consumes
    // (0 for zeros, Inf and NaN); the scaled levels are exact when every one
    // lies in [-99, 101] (finite nonzero magnitudes in [2^-100, 2^101)).
    int emin, emax;
    __device__ __forceinline__ void note(const float4 &x) {
        const int e0 = __builtin_amdgcn_frexp_expf(x.x), e1 = __builtin_amdgcn_frexp_expf(x.y);
        const int e2 = __builtin_amdgcn_frexp_expf(x.z), e3 = __builtin_amdgcn_frexp_expf(x.w);
        emin = min(emin, min(e0, e1));
        emax = max(emax, max(e0, e1));
        emin = min(emin, min(e2, e3));
        emax = max(emax, max(e2, e3));
    }

    // Input row t arrives with value x (SRC: and its g row gx); PH = t mod 3.
    template <int ROW, int CE, bool SC, int PH>
    __device__ __forceinline__ void advance(int t, const float4 &x, const float4 &gx) {
        W[0][PH] = x;
        if constexpr (SC) note(x);
        float4 v;
        static_for<K>([&](auto L) {
            constexpr int l = L + 1;
            v = level<ROW, CE, SC, PH>(l, t, W[l - 1]);
            if constexpr (l < K) W[l][PH] = v;
        });
        store_row<walks_up(ROW), SC>(t, v, W[K - 1][(PH + 2) % 3]);
        if constexpr (SRC) shift_g(gx);
    }

    // Branch-free predicated store of the level-K row produced by input t:
    // a buffer store through a per-row descriptor whose record count is the
    // row's bytes (0 for rows outside [o0, o1)); lanes that must not store
    // carry an offset beyond it and the hardware range check drops them.  No
    // branch splits the unrolled rows, so the scheduler interleaves their
    // dependency chains.  Nontemporal: the output is not re-read this pass.
    // cs: the level-(K-1) row of the same cells (the centre slot of the last
    // ring); RES takes |v - c| of the stored cells from it.
    template <bool REV, bool SC>
    __device__ __forceinline__ void store_row(int t, const float4 &vs, const float4 &cs) {
        float4 v = vs;
        if constexpr (SC) {  // 4^K u -> u: exact (see "Scaled levels")
            const f32x2 q = {kUnscale, kUnscale};
            const f32x2 a = f32x2{vs.x, vs.y} * q, b = f32x2{vs.z, vs.w} * q;
            v = make_float4(a.x, a.y, b.x, b.y);
        }
        const int j = REV ? o1 - 1 - (t - 2 * K) : o0 + (t - 2 * K);
        const bool in_block = REV ? j >= o0 : j < o1;
        const int jj = __builtin_amdgcn_readfirstlane(min(max(j, 0), rows - 1));
        const int nrec = __builtin_amdgcn_readfirstlane(in_block ? row_bytes : 0);
        __amdgpu_buffer_rsrc_t rs =
            __builtin_amdgcn_make_buffer_rsrc(out + (size_t)jj * cols, (short)0, nrec, 0x00020000);
        const u32x4 d = {__builtin_bit_cast(unsigned int, v.x), __builtin_bit_cast(unsigned int, v.y),
                         __builtin_bit_cast(unsigned int, v.z), __builtin_bit_cast(unsigned int, v.w)};
        __builtin_amdgcn_raw_buffer_store_b128(d, rs, voff, 0, 2 /* nt */);
        if constexpr (RES) {
            float4 c = cs;
            if constexpr (SC) {  // 4^(K-1) u -> u: exact (see "Residual instantiations")
                const f32x2 q = {kUnscalePrev, kUnscalePrev};
                const f32x2 a = f32x2{cs.x, cs.y} * q, b = f32x2{cs.z, cs.w} * q;
                c = make_float4(a.x, a.y, b.x, b.y);
            }
            const unsigned int m = max(max(absdiff_bits(v.x, c.x), absdiff_bits(v.y, c.y)),
                                       max(absdiff_bits(v.z, c.z), absdiff_bits(v.w, c.w)));
            // only the cells the store above really writes
            rmax = max(rmax, (in_block && stl) ? m : 0u);
        }
    }

    // Walks the block; returns false (wave-uniform) when SC and some input
    // left the range where the scaled levels are exact -- the caller then
    // walks the block again with SC = false.
    template <int ROW, int CE, bool SC>
    __device__ __forceinline__ bool run() {
        constexpr bool REV = walks_up(ROW);
        emin = 0;
        emax = 0;
        if constexpr (RES) rmax = 0;  // a walk that does not count leaves nothing behind
        // prologue: input rows 0 .. 2K, compile-time indices; level l starts
        // at input 2l (the first row it must produce)
        static_for<PRO>([&](auto T) {
            constexpr int t = T;
            W[0][t % 3] = ld<REV>(t);
            if constexpr (SC) note(W[0][t % 3]);
            float4 v;
            static_for<K>([&](auto L) {
                constexpr int l = L + 1;
                if constexpr (t >= 2 * l) {
                    v = level<ROW, CE, SC, t % 3>(l, t, W[l - 1]);
                    // the edge row (0 walking down, X-1 walking up) is input t - l == K
                    if constexpr ((ROW == ROW_TOP || ROW == ROW_BOT) && t - l == K) {
                        v = W[l - 1][(t + 2) % 3];
                        if constexpr (SC) v = make_float4(v.x * 4.0f, v.y * 4.0f, v.z * 4.0f, v.w * 4.0f);
                    }
                    if constexpr (l < K) W[l][t % 3] = v;
                }
            });
            if constexpr (t == 2 * K) store_row<REV, SC>(t, v, W[K - 1][(t + 2) % 3]);
            if constexpr (SRC) shift_g(ldg<REV>(t));
        });
        // steady state: 2U input rows per iteration, loads one batch ahead
        const int n_in = (o1 - o0) + 2 * K;
        float4 A[U], B[U];
        float4 GA[SRC ? U : 1], GB[SRC ? U : 1];  // SRC: the batches' g rows
#pragma unroll
        for (int u = 0; u < U; ++u) A[u] = ld<REV>(PRO + u);
        if constexpr (SRC) {
#pragma unroll
            for (int u = 0; u < U; ++u) GA[u] = ldg<REV>(PRO + u);
        }
        // Drain before the loop.  Without it the wait-count pass merges the
        // loads pending from the prologue into the loop header's state and
        // waits there for the store issued a few instructions earlier (a full
        // store round trip per iteration); with it every wait in the loop
        // targets a load or store issued >= 2 rows of work before.
        __builtin_amdgcn_s_waitcnt(0x0F70);  // vmcnt(0) expcnt(7) lgkmcnt(15)
        for (int t = PRO; t < n_in; t += 2 * U) {
#pragma unroll
            for (int u = 0; u < U; ++u) B[u] = ld<REV>(t + U + u);
            if constexpr (SRC) {
#pragma unroll
                for (int u = 0; u < U; ++u) GB[u] = ldg<REV>(t + U + u);
            }
            __builtin_amdgcn_sched_barrier(0);  // issue the batch here, a whole batch ahead of its use
            static_for<U>([&](auto V) {
                constexpr int ph = (PRO + V) % 3;
                advance<ROW, CE, SC, ph>(t + V, A[V], GA[SRC ? V : 0]);
            });
            if (t + U >= n_in) break;  // uniform
#pragma unroll
            for (int u = 0; u < U; ++u) A[u] = ld<REV>(t + 2 * U + u);
            if constexpr (SRC) {
#pragma unroll
                for (int u = 0; u < U; ++u) GA[u] = ldg<REV>(t + 2 * U + u);
            }
            __builtin_amdgcn_sched_barrier(0);
            static_for<U>([&](auto V) {
                constexpr int ph = (PRO + U + V) % 3;
                advance<ROW, CE, SC, ph>(t + U + V, B[V], GB[SRC ? V : 0]);
            });
        }
        if constexpr (SC) {
            const bool bad = emin < kExpLo || emax > kExpHi;
            if (__builtin_amdgcn_ballot_w64(bad) != 0) {
                // the exact walk rewrites this block; its stores land after
                // the scaled walk's (same wave, drained first)
                __builtin_amdgcn_s_waitcnt(0x0F70);
                return false;
            }
        }
        return true;
    }

    // scaled walk first (SMI_SWEEPK_SCALED, default on), the exact walk for
    // blocks whose inputs leave its range
    template <int ROW, int CE>
    __device__ __forceinline__ void go() {
        if constexpr (kScaled && ROW != ROW_FULL && !SRC) {
            if (run<ROW, CE, true>()) {
                post();
                return;
            }
        }
        run<ROW, CE, false>();
        post();
    }

    // RES: the maximum of the walk that counted, one filtered atomic per wave
    // (every lane of the wave is here: all control flow above is wave-uniform)
    __device__ __forceinline__ void post() {
        if constexpr (RES) {
            const unsigned int m = wave_max_u32(rmax);
            if ((threadIdx.x & 63) == 63) resid_post(resid, m);
        }
    }
};

// The interior task of one wave: row block rb of strip `strip`.
template <int K, bool RES = false, bool SRC = false>
__device__ __forceinline__ void sweepk_task(const SweepKArgs &a, int strip, int rb, int nrb, int lane,
                                            unsigned int *resid = nullptr, const float *src = nullptr) {
    using S = SweepK<K, 3, RES, SRC>;
    constexpr int SW = 256 - 2 * S::KC;  // output columns per window
    S w;
    w.in = a.in;
    w.out = a.out;
    w.rows = a.rows;
    w.cols = a.cols;
    // balanced row blocks: every block of a tall rectangle has >= ht/2 rows
    const int out_rows = a.row_hi - a.row_lo;
    w.o0 = a.row_lo + (int)((long)rb * out_rows / nrb);
    w.o1 = a.row_lo + (int)((long)(rb + 1) * out_rows / nrb);
    // strips start at whole 128-byte lines (col_lo rounded down to 32
    // columns): a multi-rank interior starts KC columns in, and windows
    // stored from there would straddle a line at both ends of every row
    const int cs = (a.col_lo & ~31) + strip * SW;
    const int cb = cs - S::KC + 4 * lane;
    w.cl = min(max(cb, 0), a.cols - 4);
    const bool st = lane >= S::LL && lane < 64 - S::LL && cb >= a.col_lo && cb < a.col_hi;
    w.row_bytes = a.cols * 4;
    w.voff = st ? cb * 4 : 0x7ffffff0;
    if constexpr (RES) {
        w.resid = resid;
        w.stl = st;
    }
    if constexpr (SRC) w.src = src;
    w.copyL = a.gL && cb == 0;
    w.copyR = a.gR && cb + 4 == a.cols;
    w.gT = a.gT;
    w.gB = a.gB;
    // rows any level touches: [o0 - 2K, o1 + K + 5); columns: [cs - KC, cs - KC + 256)
    const bool touchT = a.gT && w.o0 - 2 * K <= 0;
    const bool touchB = a.gB && w.o1 + K + 6 >= a.rows;
    const int ce = ((a.gL && cs - S::KC <= 0) ? 1 : 0) | ((a.gR && cs - S::KC + 256 >= a.cols) ? 2 : 0);
    int row = ROW_NONE;
    if (touchT && !touchB && w.o0 == 0)
        row = ROW_TOP;
    else if (touchB && !touchT && w.o1 == a.rows)
        row = ROW_BOT;
    else if (touchT || touchB)
        row = ROW_FULL;
#if SMI_SWEEPK_ALT
    if (row == ROW_NONE && (rb & 1)) row = ROW_UP;
#endif
    w.r_begin = walks_up(row) ? w.o1 - 1 + K : w.o0 - K;
    switch (row * 4 + ce) {
    case 0: w.template go<ROW_NONE, 0>(); break;
    case 1: w.template go<ROW_NONE, 1>(); break;
    case 2: w.template go<ROW_NONE, 2>(); break;
    case 3: w.template go<ROW_NONE, 3>(); break;
    case 4: w.template go<ROW_TOP, 0>(); break;
    case 5: w.template go<ROW_TOP, 1>(); break;
    case 6: w.template go<ROW_TOP, 2>(); break;
    case 7: w.template go<ROW_TOP, 3>(); break;
    case 8: w.template go<ROW_BOT, 0>(); break;
    case 9: w.template go<ROW_BOT, 1>(); break;
    case 10: w.template go<ROW_BOT, 2>(); break;
    case 11: w.template go<ROW_BOT, 3>(); break;
#if SMI_SWEEPK_ALT
    case 16: w.template go<ROW_UP, 0>(); break;
    case 17: w.template go<ROW_UP, 1>(); break;
    case 18: w.template go<ROW_UP, 2>(); break;
    case 19: w.template go<ROW_UP, 3>(); break;
#endif
    default: w.template go<ROW_FULL, 3>(); break;
    }
}

// experiment switch (tools/sweepbench builds): waves per SIMD the register
// allocation must allow (amdgpu_waves_per_eu); the library uses the default
#ifdef SMI_SWEEPK_WPE
#define SMI_SWEEPK_WPE_ATTR __attribute__((amdgpu_waves_per_eu(SMI_SWEEPK_WPE, SMI_SWEEPK_WPE)))
#else
#define SMI_SWEEPK_WPE_ATTR
#endif

template <int K>
__global__ __launch_bounds__(256) SMI_SWEEPK_WPE_ATTR void sweepk_kernel(SweepKArgs a, int nstrips, int nrb) {
    const int lb = xcd_remap(blockIdx.x, gridDim.x);
    const int lane = threadIdx.x & 63;
    const int task = __builtin_amdgcn_readfirstlane(lb * 4 + (int)(threadIdx.x >> 6));
#if SMI_SWEEPK_TASK_ORDER == 1  // experiment: consecutive tasks walk consecutive row blocks of one strip
    const int strip = task / nrb;
    const int rb = task - strip * nrb;
    if (strip >= nstrips) return;
#else
    const int rb = task / nstrips;
    const int strip = task - rb * nstrips;
#endif
    if (rb >= nrb) return;  // wave-uniform
    sweepk_task<K>(a, strip, rb, nrb, lane);
}

// The residual instantiation: the same tasks, each wave also posting the
// maximum of |v_K - v_{K-1}| over the cells it stores into *resid.
//   Registers: the residual needs a few more than the plain walk, and at
// K = 12 (248 VGPRs plain) the allocator would take 264 and drop the kernel to
// one wave per SIMD; asked for exactly two waves it fits 253 without a spill
// (asked for "two or more" it spills 12).  Smaller K keep an open upper end.
#ifdef SMI_SWEEPK_WPE
#define SMI_SWEEPK_RES_WPE_ATTR SMI_SWEEPK_WPE_ATTR
#else
#define SMI_SWEEPK_RES_WPE_ATTR __attribute__((amdgpu_waves_per_eu(2, K >= 12 ? 2 : 8)))
#endif
template <int K>
__global__ __launch_bounds__(256) SMI_SWEEPK_RES_WPE_ATTR void sweepk_res_kernel(SweepKArgs a, int nstrips, int nrb,
                                                                             unsigned int *__restrict__ resid) {
    const int lb = xcd_remap(blockIdx.x, gridDim.x);
    const int lane = threadIdx.x & 63;
    const int task = __builtin_amdgcn_readfirstlane(lb * 4 + (int)(threadIdx.x >> 6));
    const int rb = task / nstrips;
    const int strip = task - rb * nstrips;
    if (rb >= nrb) return;  // wave-uniform
    sweepk_task<K, true>(a, strip, rb, nrb, lane, resid);
}

// The source instantiation: the same tasks, every level adding the cell of
// `src` ("Source instantiations" above).  Two waves per SIMD are the floor the
// launch geometry (one round of resident waves) is tuned for.
#ifdef SMI_SWEEPK_WPE
#define SMI_SWEEPK_SRC_WPE_ATTR SMI_SWEEPK_WPE_ATTR
#else
#define SMI_SWEEPK_SRC_WPE_ATTR __attribute__((amdgpu_waves_per_eu(2, 8)))
#endif
template <int K>
__global__ __launch_bounds__(256) SMI_SWEEPK_SRC_WPE_ATTR void sweepk_src_kernel(SweepKArgs a, int nstrips, int nrb,
                                                                             const float *__restrict__ src) {
    const int lb = xcd_remap(blockIdx.x, gridDim.x);
    const int lane = threadIdx.x & 63;
    const int task = __builtin_amdgcn_readfirstlane(lb * 4 + (int)(threadIdx.x >> 6));
    const int rb = task / nstrips;
    const int strip = task - rb * nstrips;
    if (rb >= nrb) return;  // wave-uniform
    sweepk_task<K, false, true>(a, strip, rb, nrb, lane, nullptr, src);
}

// the kernel of a kind and the arguments it takes besides (a, nstrips, nrb)
template <int K, Kind KD, class F>
auto sweepk_with_kernel(const Variant &v, F &&f) {
    static_assert(variant_k(Family::Sweep, KD).has(K), "no such sweep instantiation");
    if constexpr (KD == Kind::Res)
        return f(sweepk_res_kernel<K>, v.resid);
    else if constexpr (KD == Kind::Src)
        return f(sweepk_src_kernel<K>, v.src);
    else
        return f(sweepk_kernel<K>);
}

template <int K, Kind KD>
int sweepk_launch(const SweepKArgs &a, int nstrips, int nrb, const Variant &v, hipStream_t s, hipEvent_t start,
                  hipEvent_t stop) {
    const dim3 grid((unsigned int)(((long)nstrips * nrb + 3) / 4));
    return sweepk_with_kernel<K, KD>(v, [&](auto kernel, auto... extra) {
        return launch_kernel(kernel, grid, 0, s, start, stop, a, nstrips, nrb, extra...);
    });
}

template <int K, Kind KD>
int sweepk_resident() {
    static int cache[64] = {};
    return sweepk_with_kernel<K, KD>(
        Variant{}, [](auto kernel, auto...) { return resident_waves(reinterpret_cast<const void *>(kernel), cache); });
}

}  // namespace smi

// One translation unit per K and kind (stencilk_k<K>.hip, stencilk_k<K>_res.hip,
// stencilk_k<K>_src.hip) so the instantiations compile in parallel.
#define SMI_SWEEPK_INSTANCE(K, KIND)                                                                     \
    namespace smi {                                                                                      \
    template int sweepk_launch<K, Kind::KIND>(const SweepKArgs &, int, int, const Variant &, hipStream_t, \
                                              hipEvent_t, hipEvent_t);                                   \
    template int sweepk_resident<K, Kind::KIND>();                                                       \
    }
