// stencil_bandk.hip -- host side of the halo-facing bands of a K-step pass
// (kernels: stencil_bandk.h, one instantiation per K in bandk_k<K>.hip) and
// the initial depth-K pack.
#include <cstdlib>

#include "stencil_common.h"

namespace smi {

// [K - SWEEPK_MIN][kind]; nullptr where the kind has no instantiation at K.
// The lean kernel (plain only): [K - SWEEPD_MIN].
using BandKLaunch = decltype(bandk_launch<SWEEPK_MIN, Kind::Plain>);
template <int K, Kind KD>
constexpr BandKLaunch *bandk_entry() {
    if constexpr (variant_k(Family::Band, KD).has(K))
        return bandk_launch<K, KD>;
    else
        return nullptr;
}
#define SMI_BANDK_ROW(K) \
    {bandk_entry<K, Kind::Plain>(), bandk_entry<K, Kind::Res>(), bandk_entry<K, Kind::Src>()},
#define SMI_BANDL_ENTRY(K) bandl_launch<K>,
static constexpr BandKLaunch *kBandK[][3] = {SMI_FOR_K_3_12(SMI_BANDK_ROW) SMI_FOR_K_13_20(SMI_BANDK_ROW)};
static constexpr decltype(bandl_launch<SWEEPD_MIN>) *kBandL[] = {SMI_FOR_K_13_20(SMI_BANDL_ENTRY)};
static_assert(sizeof(kBandK) / sizeof(kBandK[0]) == SWEEPD_MAX - SWEEPK_MIN + 1, "kBandK lists K = 3 .. SWEEPD_MAX");
static_assert(sizeof(kBandL) / sizeof(kBandL[0]) == SWEEPD_MAX - SWEEPD_MIN + 1, "kBandL lists K = 13 .. SWEEPD_MAX");
static_assert(variant_k(Family::Band, Kind::SrcRes).hi < SWEEPK_MIN, "a fourth kind needs a fourth column");

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
    SMI_ARG_CHECK(variant_k(Family::Band, Kind::Plain).has(K), "bandk: K must be 3..20");
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

int launch_bandk(int K, BandKArgs a, const Variant &v, int max_waves, hipStream_t s, hipEvent_t stop) {
    const Kind kind = v.kind();
    SMI_ARG_CHECK(kind != Kind::SrcRes && (!v.src || v.g_halo), "bandk: the source pass takes g's halos and no residual");
    SMI_ARG_CHECK(kind != Kind::Res || K <= variant_k(Family::Band, kind).hi, "bandk: the residual pass runs K <= 12");
    SMI_ARG_CHECK(kind != Kind::Src || variant_k(Family::Band, kind).has(K),
                  "bandk: the source pass runs K = 3.." + std::to_string(variant_k(Family::Band, kind).hi));
    const bool lean = variant_k(Family::BandLean, kind).has(K) && g_tune.band_lean;
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
    } else {
        SMI_TRY(kBandK[K - SWEEPK_MIN][(int)kind](a, n, v, s, start, kstop));
    }
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
