// stencilk.hip -- host side of the K-step sweep (kernel: stencilk.h, one
// instantiation per K in stencilk_k<K>.hip).
#include <cstdlib>

#include "stencil_common.h"
#include "stencil_src.h"

namespace smi {

#define SMI_SWEEPK_DECL(K)                                                                           \
    int sweepk_launch_k##K(const SweepKArgs &a, int nstrips, int nrb, int blocks, hipStream_t s,         \
                           hipEvent_t start, hipEvent_t stop);                                           \
    int sweepk_resident_k##K();
SMI_FOR_K_3_12(SMI_SWEEPK_DECL)
#define SMI_SWEEPK_ENTRY(K) {sweepk_launch_k##K, sweepk_resident_k##K},
static constexpr struct {
    decltype(sweepk_launch_k3) *launch;
    decltype(sweepk_resident_k3) *resident;
} kSweepK[] = {SMI_FOR_K_3_12(SMI_SWEEPK_ENTRY)};  // [K - SWEEPK_MIN]; K checked by check_sweepk

// the residual instantiations (stencilk_k<K>_res.hip)
#define SMI_SWEEPK_RES_DECL(K)                                                                           \
    int sweepk_res_launch_k##K(const SweepKArgs &a, int nstrips, int nrb, int blocks, unsigned int *r,   \
                               hipStream_t s, hipEvent_t start, hipEvent_t stop);                        \
    int sweepk_res_resident_k##K();
SMI_FOR_K_3_12(SMI_SWEEPK_RES_DECL)
#define SMI_SWEEPK_RES_ENTRY(K) {sweepk_res_launch_k##K, sweepk_res_resident_k##K},
static constexpr struct {
    decltype(sweepk_res_launch_k3) *launch;
    decltype(sweepk_res_resident_k3) *resident;
} kSweepKRes[] = {SMI_FOR_K_3_12(SMI_SWEEPK_RES_ENTRY)};

// the source instantiations (stencilk_k<K>_src.hip), K = 3 .. SWEEPK_SRC_MAX
#define SMI_SWEEPK_SRC_DECL(K)                                                                           \
    int sweepk_src_launch_k##K(const SweepKArgs &a, int nstrips, int nrb, int blocks, const float *src,  \
                               hipStream_t s, hipEvent_t start, hipEvent_t stop);                        \
    int sweepk_src_resident_k##K();
SMI_FOR_K_SRC(SMI_SWEEPK_SRC_DECL)
#define SMI_SWEEPK_SRC_ENTRY(K) {sweepk_src_launch_k##K, sweepk_src_resident_k##K},
static constexpr struct {
    decltype(sweepk_src_launch_k3) *launch;
    decltype(sweepk_src_resident_k3) *resident;
} kSweepKSrc[] = {SMI_FOR_K_SRC(SMI_SWEEPK_SRC_ENTRY)};
static_assert(sizeof(kSweepKSrc) / sizeof(kSweepKSrc[0]) == SWEEPK_SRC_MAX - SWEEPK_MIN + 1,
              "SMI_FOR_K_SRC lists K = 3 .. SWEEPK_SRC_MAX");

int sweepk_window_cols(int K) { return 256 - 8 * sweepk_apron_lanes(K); }

int launch_sweepk(int K, const SweepKArgs &a, hipStream_t s) { return launch_sweepk_ex(K, a, 0, 0, true, s); }

// Strips and row blocks of a K-step sweep over a's output rectangle.
// ht > 0: rows per wave as given; else automatic (g_tune.htk, or one round
// of resident waves -- minus `reserve` waves left to the comm stream's
// kernels in a multi-rank run, smi_stencil_set_bands).
static void sweepk_geometry(int K, const SweepKArgs &a, int ht_req, int reserve, bool res, bool src, int *nstrips_,
                            int *nrb_) {
    const int sw = sweepk_window_cols(K);
    const int nstrips = (a.col_hi - (a.col_lo & ~31) + sw - 1) / sw;  // line-aligned strips (stencilk.h)
    const int out_rows = a.row_hi - a.row_lo;
    int ht = ht_req > 0 ? ht_req : g_tune.htk;
    if (ht <= 0) {
        // auto: one round of resident waves, each a tall row block of its
        // strip.  Multi-rank interior: either leave `reserve` waves to the
        // comm stream's kernels (one round of the rest), or cut the interior
        // into several rounds so that workgroups retire during the pass and
        // the comm stream's kernels are dispatched then.
        int waves = src   ? kSweepKSrc[K - SWEEPK_MIN].resident()
                    : res ? kSweepKRes[K - SWEEPK_MIN].resident()
                          : kSweepK[K - SWEEPK_MIN].resident();
        const bool single = a.gT && a.gB && a.gL && a.gR;
        int rounds = single ? 1 : std::max(1, g_tune.rounds_multi);
        if (!single && reserve > 0) {
            waves = std::max(64, waves - reserve);
            rounds = 1;
        }
        const int per_strip = std::max(1, waves * rounds / nstrips);
        ht = std::max(2 * K, (out_rows + per_strip - 1) / per_strip);
    }
    *nstrips_ = nstrips;
    *nrb_ = (out_rows + ht - 1) / ht;
}

static int check_sweepk(int K, const SweepKArgs &a) {
    SMI_ARG_CHECK(K >= SWEEPK_MIN && K <= SWEEPK_MAX, "sweepk: steps per pass must be 3..12");
    return check_sweep_rect("sweepk", a);
}

// prof: record the launch under SMI_PROF_STENCIL_SWEEPK.  stop (nullable):
// an event the launch's dispatch records when the kernel completes (or an
// ordinary record when there is nothing to launch).  resid (nullable): run
// the residual instantiation, which also max-accumulates |v_K - v_{K-1}| of
// the cells it stores into *resid (K <= 12 only).  src (nullable): run the
// source instantiation (K <= SWEEPK_SRC_MAX; it has no residual variant).
int launch_sweepk_ex(int K, const SweepKArgs &a, int ht_req, int reserve, bool prof, hipStream_t s,
                     hipEvent_t stop, unsigned int *resid, const float *src) {
    if (a.row_hi <= a.row_lo || a.col_hi <= a.col_lo) {
        if (stop) SMI_HIP_CHECK(hipEventRecord(stop, s));
        return SMI_SUCCESS;
    }
    // deeper passes: the rotating-ring sweep (stencild.h); its geometry has
    // no row-block override, and wave slots reserved for the band kernel
    // (smi_stencil_set_bands) come off its one round of waves
    const bool deep = K > SWEEPK_MAX;
    SMI_ARG_CHECK(!(deep && resid), "sweepk: the residual pass runs K <= 12");
    SMI_ARG_CHECK(!src || (K <= SWEEPK_SRC_MAX && !resid),
                  "sweepk: the source pass runs K <= " + std::to_string(SWEEPK_SRC_MAX) + " and takes no residual");
    int nstrips = 0, nrb = 0;
    if (deep) {
        SMI_ARG_CHECK(ht_req <= 0, "sweepk: K > 12 has no row-block override");
    } else {
        SMI_TRY(check_sweepk(K, a));
        sweepk_geometry(K, a, ht_req, reserve, resid != nullptr, src != nullptr, &nstrips, &nrb);
    }
    // Timing (profiling on).  Back-to-back single-tile passes: one chained
    // marker per pass (the end marker of pass i is the begin of pass i+1):
    // the least host time per launch -- dispatch-carried start / stop events
    // cost ~5 us more host time per launch, which a short timed run (the
    // driver's 20 steps = 2 passes) sees (tools/exp/timed_overhead.py).  A
    // multi-rank pass (`stop` given: the comm stream waits for the interior)
    // is timed by its dispatch (start / stop handed to the launch; the
    // caller's ordering event is recorded right after it).
    hipEvent_t start = nullptr, kstop = stop, after = nullptr;
    int tok = -1;
    bool marker = false;
    if (prof && prof_enabled()) {
        const double units = (double)(a.row_hi - a.row_lo) * (a.col_hi - a.col_lo) * K;
        if (stop) {
            SMI_TRY(prof_launch(SMI_PROF_STENCIL_SWEEPK, &tok, K, units, &start, &kstop));
            after = stop;
        } else {
            SMI_TRY(prof_begin(SMI_PROF_STENCIL_SWEEPK, s, &tok, K, units, true));
            marker = true;
        }
    }
    if (deep) {
        SMI_TRY(launch_sweepd(K, a, reserve, s, start, kstop));
    } else {
        const int blocks = (int)(((long)nstrips * nrb + 3) / 4);
        if (src)
            SMI_TRY(kSweepKSrc[K - SWEEPK_MIN].launch(a, nstrips, nrb, blocks, src, s, start, kstop));
        else if (resid)
            SMI_TRY(kSweepKRes[K - SWEEPK_MIN].launch(a, nstrips, nrb, blocks, resid, s, start, kstop));
        else
            SMI_TRY(kSweepK[K - SWEEPK_MIN].launch(a, nstrips, nrb, blocks, s, start, kstop));
    }
    if (after) SMI_HIP_CHECK(hipEventRecord(after, s));
    if (marker) SMI_TRY(prof_end(tok, s));
    return SMI_SUCCESS;
}

}  // namespace smi
