// stencil.hip -- the stencil_smi hot path on gfx950.
//
// Reference pipeline replaced (ryutakashino/SMI, examples/kernels/stencil_smi.cl):
//   Read    :20-115   streams the tile + 1-cell halo ring from 4 DDR banks
//   Stencil :117-165  out = 0.25*(S+W+E+N), global-edge cells copied
//   Write   :167-234  stores the result, tees edge rows/cols to the neighbours
//   Convert{Send,Receive}* :236-386  per-element SMI_Push/SMI_Pop halo bridges
// MI355X design: one sweep kernel streams each 256-column strip of the tile
// down its rows with 16-byte loads (one float4 per lane, one wave per strip),
// keeps the north/centre/south rows in registers, gets the west/east
// neighbours across lanes with DPP wave shifts, and fetches only the two
// strip-edge cells per row separately.  Each cell is read once from HBM and
// written once (8 B/cell/step algorithmic).  In multi-rank runs an edge
// kernel computes the tile's halo-facing rows/columns first (fusing the
// column pack that Write's send_left/send_right tee did), the halo
// exchange runs on a dedicated stream through the transport (RCCL over xGMI),
// and the interior sweep overlaps it.
#include <algorithm>

#include "stencil_common.h"
#include "stencil_resid_dev.h"

namespace smi {

// One wave = one strip of 256 columns x `ht` rows; 4 waves per block take 4
// consecutive (row-block, strip) tasks, strip fastest.  U rows are fetched
// per batch and the next batch is in flight while the current one computes.
// All control values are wave-uniform (readfirstlane) and every load is
// unconditional with a clamped address, so the loop body has no divergent
// control flow around its loads and the compiler emits counted vmcnt waits.
//
// RES: the residual variant (smi_stencil_step_residual).  Same loads,
// arithmetic and stores; every lane also keeps the largest bit pattern of
// |o - c| over the cells it stores (c is the centre value already in
// registers), the wave folds the 64 lanes with DPP and its last lane issues at most
// one atomic max on *resid.  Patterns of non-negative floats order like the
// floats and every NaN pattern lies above +inf, so an unsigned max is the
// exact max-norm and carries a NaN without a branch.
//
// SRC: the update with a source term (smi_stencil_step_source),
// out = 0.25 * ((((S + W) + E) + N) + g): one more float4 load per row, of
// `src` at the row's own address, fetched with the row's batch, and one more
// add per cell.  Copied cells select the centre value after the arithmetic,
// so g never reaches a global-edge cell.
template <int U, bool NT, bool RES, bool SRC = false>
__device__ __forceinline__ void sweep_body(const float *__restrict__ in, float *__restrict__ out,
                                           const SweepArgs &a, int nstrips, int nrb, int ht,
                                           unsigned int *resid, const float *__restrict__ src = nullptr) {
    const int lb = xcd_remap(blockIdx.x, gridDim.x);
    const int lane = threadIdx.x & 63;
    const int task = __builtin_amdgcn_readfirstlane(lb * 4 + (int)(threadIdx.x >> 6));
    const int rb = task / nstrips;
    const int strip = task - rb * nstrips;
    if (rb >= nrb) return;  // wave-uniform

    const int rows = a.rows, cols = a.cols;
    const int r0 = rb * ht;
    const int r1 = min(r0 + ht, rows);
    const int cs = strip * 256;
    const int nl = min(64, (cols - cs) >> 2);  // active lanes of this strip
    const bool act = lane < nl;
    const int c0 = cs + 4 * min(lane, nl - 1);  // clamped: inactive lanes re-read lane nl-1
    const bool first_strip = strip == 0;
    const bool last_strip = cs + 256 >= cols;
    const int mT = a.mode[0], mB = a.mode[1], mL = a.mode[2], mR = a.mode[3];
    const bool own_first_col = first_strip && lane == 0;
    const bool own_last_col = last_strip && lane == nl - 1;
    const bool skipL = own_first_col && mL == SMI_SIDE_SKIP;
    const bool skipR = own_last_col && mR == SMI_SIDE_SKIP;
    const bool copyL = own_first_col && mL == SMI_SIDE_COPY;
    const bool copyR = own_last_col && mR == SMI_SIDE_COPY;
    const bool plain_store = act && !skipL && !skipR;
    const bool part_store = act && (skipL || skipR);
    // uniform base pointers for the out-of-tile rows / strip-edge columns
    const float *top = mT == SMI_SIDE_HALO ? a.halo[0] : in;
    const float *bot = mB == SMI_SIDE_HALO ? a.halo[1] : in + (size_t)(rows - 1) * cols;
    const bool west_halo = first_strip && mL == SMI_SIDE_HALO;
    const bool east_halo = last_strip && mR == SMI_SIDE_HALO;
    // west edge of row r: in[r*cols + cs-1]  |  halo_left[r]  |  (unused) in[r*cols]
    const float *wbase = first_strip ? (west_halo ? a.halo[2] : in) : in + cs - 1;
    const int wstride = west_halo ? 1 : cols;
    const float *ebase = last_strip ? (east_halo ? a.halo[3] : in) : in + cs + 256;
    const int estride = east_halo ? 1 : cols;

    auto rowp = [&](int r) -> const float * {
        return r < 0 ? top : (r >= rows ? bot : in + (size_t)r * cols);
    };
    auto ld4 = [&](int r) -> float4 { return *reinterpret_cast<const float4 *>(rowp(r) + c0); };
    auto ldw = [&](int r) -> float { return wbase[(size_t)r * wstride]; };
    auto lde = [&](int r) -> float { return ebase[(size_t)r * estride]; };
    // SRC: g of row r (always a row of the tile)
    auto ldg = [&](int r) -> float4 { return *reinterpret_cast<const float4 *>(src + (size_t)r * cols + c0); };

    unsigned int rmax = 0;  // RES: this lane's largest |o - c| pattern
    auto do_row = [&](int r, float4 n, float4 c, float4 s, float ew, float ee, float4 g) {
        const bool row_skip = (r == 0 && mT == SMI_SIDE_SKIP) || (r == rows - 1 && mB == SMI_SIDE_SKIP);
        const bool row_copy = (r == 0 && mT == SMI_SIDE_COPY) || (r == rows - 1 && mB == SMI_SIDE_COPY);
        float w = wave_shr1(c.w);
        float e = wave_shl1(c.x);
        w = lane == 0 ? ew : w;
        e = lane == nl - 1 ? ee : e;
        float4 o;
        if constexpr (SRC) {
            o.x = jacobi_src(s.x, w, c.y, n.x, g.x);
            o.y = jacobi_src(s.y, c.x, c.z, n.y, g.y);
            o.z = jacobi_src(s.z, c.y, c.w, n.z, g.z);
            o.w = jacobi_src(s.w, c.z, e, n.w, g.w);
        } else {
            o.x = jacobi(s.x, w, c.y, n.x);
            o.y = jacobi(s.y, c.x, c.z, n.y);
            o.z = jacobi(s.z, c.y, c.w, n.z);
            o.w = jacobi(s.w, c.z, e, n.w);
        }
        o.x = (copyL || row_copy) ? c.x : o.x;
        o.y = row_copy ? c.y : o.y;
        o.z = row_copy ? c.z : o.z;
        o.w = (copyR || row_copy) ? c.w : o.w;
        if (row_skip) return;  // wave-uniform
        if constexpr (RES) {
            // the cells stored below, and only those: a SKIP column's cell and
            // the clamped lanes of a partial strip (copies of lane nl-1) stay out
            const unsigned int dx = skipL ? 0u : absdiff_bits(o.x, c.x);
            const unsigned int dw = skipR ? 0u : absdiff_bits(o.w, c.w);
            const unsigned int d = max(max(dx, absdiff_bits(o.y, c.y)), max(absdiff_bits(o.z, c.z), dw));
            rmax = max(rmax, act ? d : 0u);
        }
        float *op = out + (size_t)r * cols + c0;
        if (plain_store) store4<NT>(op, o);
        if (part_store) {
            if (!skipL) op[0] = o.x;
            op[1] = o.y;
            op[2] = o.z;
            if (!skipR) op[3] = o.w;
        }
        if (own_first_col && !skipL && a.send_left) a.send_left[r] = o.x;
        if (own_last_col && !skipR && a.send_right) a.send_right[r] = o.w;
    };

    float4 n = ld4(r0 - 1);
    float4 c = ld4(r0);
    float4 sA[U];
    float wA[U], eA[U];
    float4 gA[SRC ? U : 1];
#pragma unroll
    for (int u = 0; u < U; ++u) {
        const int r = min(r0 + u, r1 - 1);
        sA[u] = ld4(r + 1);
        wA[u] = ldw(r);
        eA[u] = lde(r);
        if constexpr (SRC) gA[u] = ldg(r);
    }
    for (int r = r0; r < r1; r += U) {
        float4 sB[U];
        float wB[U], eB[U];
        float4 gB[SRC ? U : 1];
        const bool more = r + U < r1;  // uniform
        if (more) {
#pragma unroll
            for (int u = 0; u < U; ++u) {
                const int rr = min(r + U + u, r1 - 1);
                sB[u] = ld4(rr + 1);
                wB[u] = ldw(rr);
                eB[u] = lde(rr);
                if constexpr (SRC) gB[u] = ldg(rr);
            }
        }
#pragma unroll
        for (int u = 0; u < U; ++u) {
            if (r + u < r1) {
                do_row(r + u, n, c, sA[u], wA[u], eA[u], gA[SRC ? u : 0]);
                n = c;
                c = sA[u];
            }
        }
        if (more) {
#pragma unroll
            for (int u = 0; u < U; ++u) {
                sA[u] = sB[u];
                wA[u] = wB[u];
                eA[u] = eB[u];
                if constexpr (SRC) gA[u] = gB[u];
            }
        }
    }
    if constexpr (RES) {
        rmax = wave_max_u32(rmax);  // all 64 lanes are here: every exit above is wave-uniform
        if (lane == 63) resid_post(resid, rmax);
    }
}

template <int U, bool NT>
__global__ __launch_bounds__(256) void sweep_kernel(const float *__restrict__ in,
                                                    float *__restrict__ out, SweepArgs a,
                                                    int nstrips, int nrb, int ht) {
    sweep_body<U, NT, false>(in, out, a, nstrips, nrb, ht, nullptr);
}

template <int U, bool NT>
__global__ __launch_bounds__(256) void sweep_res_kernel(const float *__restrict__ in,
                                                        float *__restrict__ out, SweepArgs a,
                                                        int nstrips, int nrb, int ht,
                                                        unsigned int *__restrict__ resid) {
    sweep_body<U, NT, true>(in, out, a, nstrips, nrb, ht, resid);
}

// The source instantiations, plain and residual: `src` is a kernel argument of
// its own, so SweepArgs and the kernels above keep their layout and code.
template <int U, bool NT>
__global__ __launch_bounds__(256) void sweep_src_kernel(const float *__restrict__ in,
                                                        float *__restrict__ out, SweepArgs a,
                                                        int nstrips, int nrb, int ht,
                                                        const float *__restrict__ src) {
    sweep_body<U, NT, false, true>(in, out, a, nstrips, nrb, ht, nullptr, src);
}

template <int U, bool NT>
__global__ __launch_bounds__(256) void sweep_src_res_kernel(const float *__restrict__ in,
                                                            float *__restrict__ out, SweepArgs a,
                                                            int nstrips, int nrb, int ht,
                                                            const float *__restrict__ src,
                                                            unsigned int *__restrict__ resid) {
    sweep_body<U, NT, true, true>(in, out, a, nstrips, nrb, ht, resid, src);
}

// Cells of the tile's halo-facing sides (those with side_mask bit set),
// computed with the true side modes (COPY / HALO); also packs the new
// first / last column for the left / right neighbours.  One thread per cell:
// [0, cols) row 0, [cols, 2cols) row rows-1, then col 0, then col cols-1.
// Returns the cell's |v - in| pattern for the residual variant (RES; costs the
// one load of the centre value a computed cell does not otherwise need), 0
// for a thread without a cell.  A corner cell is visited by two threads, which
// a maximum does not notice.  SRC: a computed cell adds its cell of `src`
// (one scalar load); a copied cell does not read it.
template <bool RES, bool SRC = false>
__device__ __forceinline__ unsigned int edge_cell(const SweepArgs &a, int side_mask, const float *src = nullptr) {
    const int rows = a.rows, cols = a.cols;
    int t = blockIdx.x * blockDim.x + threadIdx.x;
    int r, c, side;
    if (t < cols) { r = 0; c = t; side = 0; }
    else if ((t -= cols) < cols) { r = rows - 1; c = t; side = 1; }
    else if ((t -= cols) < rows) { r = t; c = 0; side = 2; }
    else if ((t -= rows) < rows) { r = t; c = cols - 1; side = 3; }
    else return 0;
    if (!(side_mask & (1 << side))) return 0;
    const float *in = a.in;
    const size_t idx = (size_t)r * cols + c;
    const bool copy = (r == 0 && a.mode[0] == SMI_SIDE_COPY) ||
                      (r == rows - 1 && a.mode[1] == SMI_SIDE_COPY) ||
                      (c == 0 && a.mode[2] == SMI_SIDE_COPY) ||
                      (c == cols - 1 && a.mode[3] == SMI_SIDE_COPY);
    float v;
    if (copy) {
        v = in[idx];
    } else {
        // select the address, then load once: no load of an unused halo
        // pointer or of an out-of-tile offset can be speculated
        const float *np = r > 0 ? in + idx - cols : a.halo[0] + c;
        const float *sp = r < rows - 1 ? in + idx + cols : a.halo[1] + c;
        const float *wp = c > 0 ? in + idx - 1 : a.halo[2] + r;
        const float *ep = c < cols - 1 ? in + idx + 1 : a.halo[3] + r;
        if constexpr (SRC)
            v = jacobi_src(*sp, *wp, *ep, *np, src[idx]);
        else
            v = jacobi(*sp, *wp, *ep, *np);
    }
    a.out[idx] = v;
    if (c == 0 && a.send_left) a.send_left[r] = v;
    if (c == cols - 1 && a.send_right) a.send_right[r] = v;
    if constexpr (RES) return absdiff_bits(v, in[idx]);
    return 0;
}

__global__ __launch_bounds__(256) void edge_kernel(SweepArgs a, int side_mask) { edge_cell<false>(a, side_mask); }

__global__ __launch_bounds__(256) void edge_res_kernel(SweepArgs a, int side_mask,
                                                       unsigned int *__restrict__ resid) {
    // every lane returns from edge_cell (with 0 if it has no cell) before the
    // wave folds: one atomic max per wave
    const unsigned int m = wave_max_u32(edge_cell<true>(a, side_mask));
    if ((threadIdx.x & 63) == 63) resid_post(resid, m);
}

__global__ __launch_bounds__(256) void edge_src_kernel(SweepArgs a, int side_mask, const float *__restrict__ src) {
    edge_cell<false, true>(a, side_mask, src);
}

__global__ __launch_bounds__(256) void edge_src_res_kernel(SweepArgs a, int side_mask, const float *__restrict__ src,
                                                           unsigned int *__restrict__ resid) {
    const unsigned int m = wave_max_u32(edge_cell<true, true>(a, side_mask, src));
    if ((threadIdx.x & 63) == 63) resid_post(resid, m);
}

// Pack the first / last column of a tile (the initial halos that the
// reference's artificial timestep t=0 sends, stencil_smi.cl:26-29,183-224).
__global__ __launch_bounds__(256) void pack_cols_kernel(const float *in, int rows, int cols,
                                                        float *left, float *right) {
    const int r = blockIdx.x * blockDim.x + threadIdx.x;
    if (r >= rows) return;
    if (left) left[r] = in[(size_t)r * cols];
    if (right) right[r] = in[(size_t)r * cols + cols - 1];
}

// ---------------------------------------------------------------- host --
Tuning g_tune;

int check_tile(const float *in, const float *out, int rows, int cols) {
    SMI_ARG_CHECK(in && out, "NULL tile buffer");
    SMI_ARG_CHECK(in != out, "in and out must differ");
    SMI_ARG_CHECK(rows >= 1 && cols >= 4 && cols % 4 == 0, "tile must be >=1 x >=4 with y_local % 4 == 0");
    SMI_ARG_CHECK(aligned16(in) && aligned16(out), "tile buffers must be 16-byte aligned");
    return SMI_SUCCESS;
}

int check_src(const float *src, const float *buf0, const float *buf1, int rows, int cols) {
    SMI_ARG_CHECK(src, "NULL source array");
    SMI_ARG_CHECK(aligned16(src), "the source array must be 16-byte aligned");
    const size_t n = (size_t)std::max(rows, 0) * (size_t)std::max(cols, 0);
    auto overlaps = [&](const float *b) { return b && src < b + n && b < src + n; };
    SMI_ARG_CHECK(!overlaps(buf0) && !overlaps(buf1), "the source array must not overlap a tile buffer");
    return SMI_SUCCESS;
}

int resident_waves(const void *kernel, int (&cache)[64]) {
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= 64) return 0;
    if (cache[dev]) return cache[dev];
    int per_cu = 0, cus = 0;
    if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, kernel, 256, 0) != hipSuccess) return 0;
    if (hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess) return 0;
    cache[dev] = per_cu * cus * 4;
    return cache[dev];
}

// strips x row blocks of `ht` rows of a single-step sweep (four tasks per workgroup)
struct SweepGeom {
    int nstrips, nrb, ht;
};

// the kernel of (U, NT, kind).  The source kernels exist for U <= 8 only
// (launch_sweep below).
template <int U, bool NT>
static int launch_sweep_unt(const SweepArgs &a, const SweepGeom &g, const Variant &v, hipStream_t s) {
    const dim3 grid((unsigned int)(((long)g.nstrips * g.nrb + 3) / 4));
    auto go = [&](auto kernel, auto... extra) {
        return launch_kernel(kernel, grid, 0, s, nullptr, nullptr, a.in, a.out, a, g.nstrips, g.nrb, g.ht, extra...);
    };
    if constexpr (U <= 8) {
        if (v.kind() == Kind::SrcRes) return go(sweep_src_res_kernel<U, NT>, v.src, v.resid);
        if (v.kind() == Kind::Src) return go(sweep_src_kernel<U, NT>, v.src);
    }
    if (v.kind() == Kind::Res) return go(sweep_res_kernel<U, NT>, v.resid);
    SMI_ARG_CHECK(v.kind() == Kind::Plain, "sweep: no source kernel at this many rows in flight");
    return go(sweep_kernel<U, NT>);
}
template <int U>
static int launch_sweep_u(const SweepArgs &a, const SweepGeom &g, const Variant &v, hipStream_t s) {
    return g_tune.nt ? launch_sweep_unt<U, true>(a, g, v, s) : launch_sweep_unt<U, false>(a, g, v, s);
}

int launch_sweep(const SweepArgs &a, const Variant &v, hipStream_t s) {
    const int ht = std::max(1, g_tune.ht);
    const SweepGeom g{(a.cols + 255) / 256, (a.rows + ht - 1) / ht, ht};
    int tok = -1;
    if (prof_enabled()) SMI_TRY(prof_begin(SMI_PROF_STENCIL_SWEEP, s, &tok, 1, (double)a.rows * a.cols));
    // Rows in flight.  The source kernels fetch a g row with every row of a
    // batch: twice the float4 registers in flight, so 16 rows in flight run
    // as 8 there; any other setting means 8 for them and 4 for the plain ones.
    int u = g_tune.u;
    if (v.src)
        u = u == 1 || u == 2 || u == 4 ? u : 8;
    else
        u = u == 1 || u == 2 || u == 8 || u == 16 ? u : 4;
    switch (u) {
    case 1: SMI_TRY(launch_sweep_u<1>(a, g, v, s)); break;
    case 2: SMI_TRY(launch_sweep_u<2>(a, g, v, s)); break;
    case 4: SMI_TRY(launch_sweep_u<4>(a, g, v, s)); break;
    case 8: SMI_TRY(launch_sweep_u<8>(a, g, v, s)); break;
    default: SMI_TRY(launch_sweep_u<16>(a, g, v, s)); break;
    }
    if (tok >= 0) SMI_TRY(prof_end(tok, s));
    return SMI_SUCCESS;
}

int launch_edge(const SweepArgs &a, int side_mask, const Variant &v, hipStream_t s) {
    const long cells = 2L * a.cols + 2L * a.rows;
    const dim3 grid((unsigned int)((cells + 255) / 256));
    int tok = -1;
    if (prof_enabled()) SMI_TRY(prof_begin(SMI_PROF_STENCIL_EDGE, s, &tok));
    switch (v.kind()) {
    case Kind::Plain: SMI_TRY(launch_kernel(edge_kernel, grid, 0, s, nullptr, nullptr, a, side_mask)); break;
    case Kind::Res: SMI_TRY(launch_kernel(edge_res_kernel, grid, 0, s, nullptr, nullptr, a, side_mask, v.resid)); break;
    case Kind::Src: SMI_TRY(launch_kernel(edge_src_kernel, grid, 0, s, nullptr, nullptr, a, side_mask, v.src)); break;
    case Kind::SrcRes:
        SMI_TRY(launch_kernel(edge_src_res_kernel, grid, 0, s, nullptr, nullptr, a, side_mask, v.src, v.resid));
        break;
    }
    if (tok >= 0) SMI_TRY(prof_end(tok, s));
    return SMI_SUCCESS;
}

int launch_pack_cols(const float *in, int rows, int cols, float *left, float *right, hipStream_t s) {
    hipLaunchKernelGGL(pack_cols_kernel, dim3((rows + 255) / 256), dim3(256), 0, s, in, rows, cols, left, right);
    SMI_HIP_CHECK(hipGetLastError());
    return SMI_SUCCESS;
}

}  // namespace smi

using namespace smi;

extern "C" {

int smi_stencil_set_tuning(int rows_per_wave, int rows_in_flight, int nontemporal_stores, int overlap) {
    if (rows_per_wave > 0) g_tune.ht = rows_per_wave;
    if (rows_in_flight > 0) {
        SMI_ARG_CHECK(rows_in_flight == 1 || rows_in_flight == 2 || rows_in_flight == 4 ||
                          rows_in_flight == 8 || rows_in_flight == 16,
                      "rows_in_flight must be 1, 2, 4, 8 or 16");
        g_tune.u = rows_in_flight;
    }
    if (nontemporal_stores >= 0) g_tune.nt = nontemporal_stores != 0;
    if (overlap >= 0) g_tune.overlap = overlap != 0;
    return SMI_SUCCESS;
}

int smi_stencil_get_tuning(int *rows_per_wave, int *rows_in_flight, int *nontemporal_stores, int *overlap) {
    if (rows_per_wave) *rows_per_wave = g_tune.ht;
    if (rows_in_flight) *rows_in_flight = g_tune.u;
    if (nontemporal_stores) *nontemporal_stores = g_tune.nt;
    if (overlap) *overlap = g_tune.overlap;
    return SMI_SUCCESS;
}

static int step_args(const float *in, float *out, int x_local, int y_local, const int mode[4],
                     const float *const halo[4], float *send_left, float *send_right, SweepArgs *args) {
    SweepArgs &a = *args;
    SMI_TRY(check_tile(in, out, x_local, y_local));
    SMI_ARG_CHECK(mode, "NULL mode array");
    a = SweepArgs{};
    a.in = in;
    a.out = out;
    a.rows = x_local;
    a.cols = y_local;
    for (int k = 0; k < 4; ++k) {
        SMI_ARG_CHECK(mode[k] >= SMI_SIDE_COPY && mode[k] <= SMI_SIDE_SKIP, "bad side mode");
        a.mode[k] = mode[k];
        a.halo[k] = halo ? halo[k] : nullptr;
        if (mode[k] == SMI_SIDE_HALO) SMI_ARG_CHECK(a.halo[k] != nullptr, "HALO side without halo vector");
    }
    a.send_left = send_left;
    a.send_right = send_right;
    return SMI_SUCCESS;
}

int smi_stencil_step(const float *in, float *out, int x_local, int y_local, const int mode[4],
                     const float *const halo[4], float *send_left, float *send_right,
                     SMI_Stream stream) {
    SweepArgs a;
    SMI_TRY(step_args(in, out, x_local, y_local, mode, halo, send_left, send_right, &a));
    return launch_sweep(a, Variant{}, (hipStream_t)stream);
}

int smi_stencil_step_residual(const float *in, float *out, int x_local, int y_local, const int mode[4],
                              const float *const halo[4], float *send_left, float *send_right,
                              unsigned int *resid_bits, SMI_Stream stream) {
    SweepArgs a;
    SMI_TRY(step_args(in, out, x_local, y_local, mode, halo, send_left, send_right, &a));
    SMI_ARG_CHECK(resid_bits && ((uintptr_t)resid_bits & 3u) == 0, "resid_bits must be a 4-byte aligned device word");
    return launch_sweep(a, Variant{resid_bits}, (hipStream_t)stream);
}

int smi_stencil_step_source(const float *in, float *out, const float *src, int x_local, int y_local,
                            const int mode[4], const float *const halo[4], float *send_left, float *send_right,
                            unsigned int *resid_bits, SMI_Stream stream) {
    SweepArgs a;
    SMI_TRY(step_args(in, out, x_local, y_local, mode, halo, send_left, send_right, &a));
    SMI_TRY(check_src(src, in, out, x_local, y_local));
    SMI_ARG_CHECK(((uintptr_t)resid_bits & 3u) == 0, "resid_bits must be a 4-byte aligned device word");
    return launch_sweep(a, Variant{resid_bits, src}, (hipStream_t)stream);
}

}  // extern "C"
