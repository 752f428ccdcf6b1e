// stencil_bandk.hip -- host side of the halo-facing bands of a K-step pass
// (kernels: stencil_bandk.h, one instantiation per K in bandk_k<K>.hip) and
// the initial depth-K pack.
#include <cstdlib>

#include "stencil_common.h"
#include "stencil_src.h"

namespace smi {

#define SMI_BANDK_DECL(K) \
    int bandk_launch_k##K(const BandKArgs &a, int waves, hipStream_t s, hipEvent_t start, hipEvent_t stop);
SMI_FOR_K_3_12(SMI_BANDK_DECL)
SMI_FOR_K_13_20(SMI_BANDK_DECL)
#define SMI_BANDL_DECL(K) \
    int bandl_launch_k##K(const BandKArgs &a, int blocks, hipStream_t s, hipEvent_t start, hipEvent_t stop);
SMI_FOR_K_13_20(SMI_BANDL_DECL)
// [K - SWEEPK_MIN] / [K - SWEEPD_MIN]; plan_bands refuses a K outside 3..20
#define SMI_BANDK_ENTRY(K) bandk_launch_k##K,
#define SMI_BANDL_ENTRY(K) bandl_launch_k##K,
static constexpr decltype(bandk_launch_k3) *kBandK[] = {SMI_FOR_K_3_12(SMI_BANDK_ENTRY)
                                                        SMI_FOR_K_13_20(SMI_BANDK_ENTRY)};
static constexpr decltype(bandl_launch_k13) *kBandL[] = {SMI_FOR_K_13_20(SMI_BANDL_ENTRY)};
// the residual instantiations (bandk_k<K>_res.hip), [K - SWEEPK_MIN]
#define SMI_BANDK_RES_DECL(K)                                                                    \
    int bandk_res_launch_k##K(const BandKArgs &a, int waves, unsigned int *resid, hipStream_t s, \
                              hipEvent_t start, hipEvent_t stop);
SMI_FOR_K_3_12(SMI_BANDK_RES_DECL)
#define SMI_BANDK_RES_ENTRY(K) bandk_res_launch_k##K,
static constexpr decltype(bandk_res_launch_k3) *kBandKRes[] = {SMI_FOR_K_3_12(SMI_BANDK_RES_ENTRY)};

// the source instantiations (bandk_k<K>_src.hip), [K - SWEEPK_MIN], K = 3 .. SWEEPK_SRC_MAX
#define SMI_BANDK_SRC_DECL(K)                                                                       \
    int bandk_src_launch_k##K(const BandKArgs &a, const HaloK &gh, const float *src, int waves,     \
                              hipStream_t s, hipEvent_t start, hipEvent_t stop);
SMI_FOR_K_SRC(SMI_BANDK_SRC_DECL)
#define SMI_BANDK_SRC_ENTRY(K) bandk_src_launch_k##K,
static constexpr decltype(bandk_src_launch_k3) *kBandKSrc[] = {SMI_FOR_K_SRC(SMI_BANDK_SRC_ENTRY)};
static_assert(sizeof(kBandKSrc) / sizeof(kBandKSrc[0]) == SWEEPK_SRC_MAX - SWEEPK_MIN + 1,
              "SMI_FOR_K_SRC lists K = 3 .. SWEEPK_SRC_MAX");

static int compute_units() {
    static int cached[64] = {};
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= 64) return 0;
    if (!cached[dev]) {
        int cus = 0;
        if (hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess) return 0;
        cached[dev] = cus;
    }
    return cached[dev];
}

int plan_bands(int K, BandKArgs *ap, bool lean) {
    BandKArgs &a = *ap;
    const int X = a.rows, Y = a.cols;
    a.kc = kc_of(K);
    SMI_ARG_CHECK(K >= SWEEPK_MIN && K <= SWEEPD_MAX, "bandk: K must be 3..20");
    SMI_ARG_CHECK(X >= 2 * K && Y >= 2 * a.kc && Y % 4 == 0, "bandk: tile smaller than 2K x 2KC");
    // one wave per 64 - 2K cells along a band (stencil_bandk.h)
    // lean kernel: two cells per lane, pair-aligned windows (BandL::SW)
    a.sw = lean ? 128 - 2 * (K + (K & 1)) : 64 - 2 * K;
    a.rlo = a.has[0] ? K : 0;
    a.rhi = a.has[1] ? X - K : X;
    const int nrow = (Y + a.sw - 1) / a.sw;
    const int ncol = a.rhi > a.rlo ? (a.rhi - a.rlo + a.sw - 1) / a.sw : 0;
    const int waves_of[4] = {a.has[0] ? nrow : 0, a.has[1] ? nrow : 0, a.has[2] ? ncol : 0, a.has[3] ? ncol : 0};
    int n = 0;
    for (int k = 0; k < 4; ++k) {
        a.first[k] = n;
        n += waves_of[k];
    }
    a.first[4] = n;
    a.prio = 1;
#ifdef SMI_LOOPBACK_REHEARSAL
    if (const char *v = getenv("SMI_REH_BAND_PRIO")) a.prio = atoi(v) != 0;  // priority A/B
    // timing experiments (results are wrong): no band work at all, or only
    // the row walks (top / bottom bands) or only the transposed column walks
    if (getenv("SMI_REH_NOBANDS")) a.first[1] = a.first[2] = a.first[3] = a.first[4] = 0;
    if (const char *m = getenv("SMI_REH_BANDS")) {
        if (m[0] == 'r') {
            a.first[3] = a.first[4] = a.first[2];
        } else if (m[0] == 'c') {
            const int nl = a.first[3] - a.first[2], nr = a.first[4] - a.first[3];
            a.first[1] = a.first[2] = 0;
            a.first[3] = nl;
            a.first[4] = nl + nr;
        }
    }
#endif
    return SMI_SUCCESS;
}

int launch_bandk(int K, BandKArgs a, int max_waves, hipStream_t s, hipEvent_t stop, unsigned int *resid) {
    SMI_ARG_CHECK(!resid || K <= SWEEPK_MAX, "bandk: the residual pass runs K <= 12");
    const bool lean = K >= SWEEPD_MIN && g_tune.band_lean;
    SMI_TRY(plan_bands(K, &a, lean));
    const int segs = a.first[4];
    if (segs == 0) {
        if (stop) SMI_HIP_CHECK(hipEventRecord(stop, s));
        return SMI_SUCCESS;
    }
    // one wave per segment, or at most max_waves (> 0) waves looping over them
    const int n = max_waves > 0 ? std::min(segs, std::max(4, max_waves)) : segs;
    // timed by the dispatch itself (as the K-step sweep, stencilk.hip); the
    // caller's ordering event is then recorded right after the launch
    hipEvent_t start = nullptr, kstop = stop, after = nullptr;
    int tok = -1;
    if (prof_enabled()) {
        SMI_TRY(prof_launch(SMI_PROF_STENCIL_EDGE, &tok, K, 0.0, &start, &kstop));
        after = stop;
    }
    if (lean) {
        // the lean kernel beside the interior: one workgroup (4 waves) per CU
        // at most, fewer when max_waves asks for fewer
        const int cus = compute_units();
        SMI_ARG_CHECK(cus > 0, "bandl: compute-unit query failed");
        int blocks = std::min(cus, (segs + 3) / 4);
        if (max_waves > 0) blocks = std::min(blocks, std::max(1, max_waves / 4));
        SMI_TRY(kBandL[K - SWEEPD_MIN](a, blocks, s, start, kstop));
    } else if (resid) {
        SMI_TRY(kBandKRes[K - SWEEPK_MIN](a, n, resid, s, start, kstop));
    } else {
        SMI_TRY(kBandK[K - SWEEPK_MIN](a, n, s, start, kstop));
    }
    if (after) SMI_HIP_CHECK(hipEventRecord(after, s));
    return SMI_SUCCESS;
}

// The bands of a source pass (bandk_src_kernel): launch_bandk's one wave per
// segment or max_waves looping waves, timed the same way under its own
// profiling entry.  There is no lean and no residual variant.
int launch_bandk_src(int K, BandKArgs a, const HaloK &g_halo, const float *src, int max_waves, hipStream_t s,
                     hipEvent_t stop) {
    SMI_ARG_CHECK(src, "bandk: NULL source");
    SMI_ARG_CHECK(K >= SWEEPK_MIN && K <= SWEEPK_SRC_MAX,
                  "bandk: the source pass runs K = 3.." + std::to_string(SWEEPK_SRC_MAX));
    SMI_TRY(plan_bands(K, &a, false));
    const int segs = a.first[4];
    if (segs == 0) {
        if (stop) SMI_HIP_CHECK(hipEventRecord(stop, s));
        return SMI_SUCCESS;
    }
    const int n = max_waves > 0 ? std::min(segs, std::max(4, max_waves)) : segs;
    hipEvent_t start = nullptr, kstop = stop, after = nullptr;
    int tok = -1;
    if (prof_enabled()) {
        SMI_TRY(prof_launch(SMI_PROF_STENCIL_EDGE, &tok, K, 0.0, &start, &kstop));
        after = stop;
    }
    SMI_TRY(kBandKSrc[K - SWEEPK_MIN](a, g_halo, src, n, s, start, kstop));
    if (after) SMI_HIP_CHECK(hipEventRecord(after, s));
    return SMI_SUCCESS;
}

// Initial depth-K sends from the current tile: columns 0..KC-1 and
// Y-KC..Y-1 packed [row][k], and the four K x KC corner blocks.
__global__ __launch_bounds__(256) void packk_kernel(const float *in, int X, int Y, int K, int KC, HaloK h) {
    const int t = blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= X * KC) return;
    const int p = t / KC, k = t - p * KC;
    const float *row = in + (size_t)p * Y;
    const float vl = row[k], vr = row[Y - KC + k];
    h.send_left[t] = vl;
    h.send_right[t] = vr;
    if (p < K) {
        h.send_corner[0][p * KC + k] = vl;
        h.send_corner[1][p * KC + k] = vr;
    }
    if (p >= X - K) {
        h.send_corner[2][(p - (X - K)) * KC + k] = vl;
        h.send_corner[3][(p - (X - K)) * KC + k] = vr;
    }
}

int launch_packk(const float *in, int rows, int cols, int K, const HaloK &h, hipStream_t s) {
    const int KC = kc_of(K);
    SMI_ARG_CHECK(cols >= 2 * KC && rows >= K, "packk: tile smaller than 2KC columns");
    const int n = rows * KC;
    hipLaunchKernelGGL(packk_kernel, dim3((n + 255) / 256), dim3(256), 0, s, in, rows, cols, K, KC, h);
    SMI_HIP_CHECK(hipGetLastError());
    return SMI_SUCCESS;
}


}  // namespace smi
