// stencilk.hip -- host side of the K-step sweep (kernel: stencilk.h, one
// instantiation per K in stencilk_k<K>.hip).
#include "stencil_common.h"

namespace smi {

// [K - SWEEPK_MIN][kind]; an empty entry where the kind has no instantiation at K
struct SweepKEntry {
    decltype(sweepk_launch<SWEEPK_MIN, Kind::Plain>) *launch = nullptr;
    decltype(sweepk_resident<SWEEPK_MIN, Kind::Plain>) *resident = nullptr;
};
template <int K, Kind KD>
constexpr SweepKEntry sweepk_entry() {
    if constexpr (variant_k(Family::Sweep, KD).has(K))
        return {sweepk_launch<K, KD>, sweepk_resident<K, KD>};
    else
        return {};
}
#define SMI_SWEEPK_ROW(K) \
    {sweepk_entry<K, Kind::Plain>(), sweepk_entry<K, Kind::Res>(), sweepk_entry<K, Kind::Src>()},
static constexpr SweepKEntry kSweepK[][3] = {SMI_FOR_K_3_12(SMI_SWEEPK_ROW)};
static_assert(sizeof(kSweepK) / sizeof(kSweepK[0]) == SWEEPK_MAX - SWEEPK_MIN + 1,
              "SMI_FOR_K_3_12 lists K = 3 .. SWEEPK_MAX");
static_assert(variant_k(Family::Sweep, Kind::SrcRes).hi < SWEEPK_MIN, "a fourth kind needs a fourth column");

int sweepk_window_cols(int K) { return 256 - 8 * sweepk_apron_lanes(K); }

// Strips and row blocks of a K-step sweep over a's output rectangle: rows per
// wave from g_tune.htk, or automatic (one round of `e`'s resident waves --
// minus `reserve` waves left to the comm stream's kernels in a multi-rank run,
// smi_stencil_set_bands).
static void sweepk_geometry(int K, const SweepKArgs &a, const SweepKEntry &e, int reserve, int *nstrips_, int *nrb_) {
    const int sw = sweepk_window_cols(K);
    const int nstrips = (a.col_hi - (a.col_lo & ~31) + sw - 1) / sw;  // line-aligned strips (stencilk.h)
    const int out_rows = a.row_hi - a.row_lo;
    int ht = g_tune.htk;
    if (ht <= 0) {
        // auto: one round of resident waves, each a tall row block of its
        // strip.  Multi-rank interior: either leave `reserve` waves to the
        // comm stream's kernels (one round of the rest), or cut the interior
        // into several rounds so that workgroups retire during the pass and
        // the comm stream's kernels are dispatched then.
        int waves = e.resident();
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

// The launch is recorded under SMI_PROF_STENCIL_SWEEPK.  stop (nullable): an
// event the launch's dispatch records when the kernel completes (or an
// ordinary record when there is nothing to launch).  v.resid: the residual
// instantiation, which also max-accumulates |v_K - v_{K-1}| of the cells it
// stores into *resid (K <= 12 only).  v.src: the source instantiation
// (K <= SWEEPK_SRC_MAX; it has no residual variant).
int launch_sweepk(int K, const SweepKArgs &a, const Variant &v, int reserve, hipStream_t s, hipEvent_t stop) {
    if (a.row_hi <= a.row_lo || a.col_hi <= a.col_lo) {
        if (stop) SMI_HIP_CHECK(hipEventRecord(stop, s));
        return SMI_SUCCESS;
    }
    // deeper passes: the rotating-ring sweep (stencild.h); wave slots reserved
    // for the band kernel (smi_stencil_set_bands) come off its one round of waves
    const bool deep = K > SWEEPK_MAX;
    constexpr int src_max = variant_k(Family::Sweep, Kind::Src).hi;
    SMI_ARG_CHECK(!(deep && v.resid), "sweepk: the residual pass runs K <= 12");
    SMI_ARG_CHECK(!v.src || (K <= src_max && !v.resid),
                  "sweepk: the source pass runs K <= " + std::to_string(src_max) + " and takes no residual");
    SweepKEntry e;
    int nstrips = 0, nrb = 0;
    if (!deep) {
        SMI_ARG_CHECK(variant_k(Family::Sweep, v.kind()).has(K), "sweepk: steps per pass must be 3..12");
        SMI_TRY(check_sweep_rect("sweepk", a));
        e = kSweepK[K - SWEEPK_MIN][(int)v.kind()];
        sweepk_geometry(K, a, e, reserve, &nstrips, &nrb);
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
    if (prof_enabled()) {
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
        SMI_TRY(e.launch(a, nstrips, nrb, v, s, start, kstop));
    }
    if (after) SMI_HIP_CHECK(hipEventRecord(after, s));
    if (marker) SMI_TRY(prof_end(tok, s));
    return SMI_SUCCESS;
}

}  // namespace smi
