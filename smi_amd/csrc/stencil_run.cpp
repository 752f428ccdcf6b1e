// stencil_run.cpp -- the stencil_smi program on one rank's tile.
//
// Reference host + Convert kernels replaced: examples/host/stencil_smi.cpp
// (rank map :133-134, ping-pong half :344) and the eight
// Convert{Send,Receive}{Top,Bottom,Left,Right} kernels of
// examples/kernels/stencil_smi.cl:236-386, whose per-element SMI_Push/SMI_Pop
// streams become one transport group of bulk sends/receives per exchange.
#include <sched.h>

#include <chrono>
#include <cstdlib>

#include "stencil_common.h"

namespace smi {

struct Neighbours {
    int top = -1, bottom = -1, left = -1, right = -1;   // stencil_smi.cl:242,257,269,293
    int tl = -1, tr = -1, bl = -1, br = -1;             // diagonals (depth-2 corners only)
};

// The pass-boundary join of the K-step passes.  interior(t) reads the bands
// band(t-1) wrote on the comm stream.  A stream wait on its event costs a
// barrier packet on the main stream -- ~7-10 us between two interiors even
// when band(t-1) finished long before (tools/streambench).
// band(t-1) runs beside interior(t-1) and normally ends well inside it, so the
// host watches it instead: once hipEventQuery reports it complete (its
// end-of-kernel release done), interior(t) is enqueued behind interior(t-1)
// with no wait packet, and its own dispatch acquire makes the bands visible.
// Should interior(t-1) finish first, the host still waits for band(t-1): a
// wait packet on the library's own interior stream measured far worse than
// the host's few microseconds (0.70 vs 0.91 of a lone tile).
// The host only waits for work already enqueued, so no rank's host can block
// another's (every exchange up to t-1 was posted before).
static bool host_join_enabled() {
#ifdef SMI_LOOPBACK_REHEARSAL
    if (const char *v = getenv("SMI_HOST_JOIN")) return atoi(v) != 0;  // rehearsal A/B
#endif
    return g_tune.host_join != 0;
}

#ifdef SMI_LOOPBACK_REHEARSAL
// rehearsal: a host thread that falls behind -- SMI_REH_STALL_US of busy
// host time before every SMI_REH_STALL_EVERY-th pass's interior is enqueued
// (the same point under either join), to price what a descheduled host costs
static void rehearsal_stall(int kpass) {
    static const long us = getenv("SMI_REH_STALL_US") ? atol(getenv("SMI_REH_STALL_US")) : 0;
    static const int every = getenv("SMI_REH_STALL_EVERY") ? std::max(1, atoi(getenv("SMI_REH_STALL_EVERY"))) : 10;
    if (us <= 0 || kpass % every != every / 2) return;
    const auto t0 = std::chrono::steady_clock::now();
    while (std::chrono::steady_clock::now() - t0 < std::chrono::microseconds(us)) {
    }
}
#else
static void rehearsal_stall(int) {}
#endif

// The wait: a short spin (the band normally ended long before, and a wake-up
// after a sleep would cost the pass more than it saves), then the core is
// yielded between polls, so that rank threads sharing the job's cores (the
// in-process groups, the C++ hosts) reach their own transport rendezvous --
// which band(t-1)'s exchange may be waiting for.  A band that never finishes
// (a peer that failed, so exchange(t-2) never completes) is an error after
// kJoinTimeout rather than a spin forever.
static constexpr int kJoinSpinPolls = 64;
static constexpr std::chrono::seconds kJoinTimeout{300};

static int join_band(hipEvent_t band_prev) {
    const auto t0 = std::chrono::steady_clock::now();
    for (unsigned polls = 0;; ++polls) {
        const hipError_t q = hipEventQuery(band_prev);
        if (q == hipSuccess) return SMI_SUCCESS;
        if (q != hipErrorNotReady) SMI_HIP_CHECK(q);
        if (polls < kJoinSpinPolls) continue;
        if ((polls & 1023) == 0 && std::chrono::steady_clock::now() - t0 > kJoinTimeout) {
            set_error("smi_stencil_run: the band kernel of the previous pass did not finish within 300 s "
                      "(a peer rank stopped exchanging halos?)");
            return SMI_ERR_COMM;
        }
        sched_yield();
    }
}

// The stream the multi-rank interior runs on.  HIP maps streams onto
// GPU_MAX_HW_QUEUES (default 4) hardware queues per priority and shares a
// queue between streams beyond that; RCCL makes streams of its own.  A
// caller's stream at normal priority created after the communicator landed
// on a queue RCCL's work also uses, and the interior then serialised with the
// exchange: 0.70-0.79 of a lone tile instead of 0.92-0.94 in the interior-rank
// rehearsal (profiles/r05/rehearsal/queues/).  The comm stream is at the
// highest priority; an interior stream there as well gets a queue of its own.
// So a caller's stream at the highest priority is used as it is; any other
// is joined to an interior stream of the communicator at that priority (a
// wait only when the caller's stream still has work pending) and joins it
// back at the end of the run.
static int interior_stream(Comm *c, hipStream_t user, hipStream_t *out, bool *own) {
    int least = 0, greatest = 0, prio = 0;
    SMI_HIP_CHECK(hipDeviceGetStreamPriorityRange(&least, &greatest));
    SMI_HIP_CHECK(hipStreamGetPriority(user, &prio));
    *out = user;
    *own = false;
    if (prio == greatest) return SMI_SUCCESS;
    if (!c->interior_stream) {
        // made on the communicator's device whatever the calling thread's
        // current device is (the stream lives as long as the communicator)
        int cur = 0;
        SMI_HIP_CHECK(hipGetDevice(&cur));
        if (cur != c->device) SMI_HIP_CHECK(hipSetDevice(c->device));
        const hipError_t e = hipStreamCreateWithPriority(&c->interior_stream, hipStreamNonBlocking, greatest);
        if (cur != c->device) SMI_HIP_CHECK(hipSetDevice(cur));
        SMI_HIP_CHECK(e);
    }
    const hipError_t q = hipStreamQuery(user);
    if (q == hipErrorNotReady) {
        hipEvent_t ev;
        SMI_TRY(comm_event(c, 3, &ev));
        SMI_HIP_CHECK(hipEventRecord(ev, user));
        SMI_HIP_CHECK(hipStreamWaitEvent(c->interior_stream, ev, 0));
    } else if (q != hipSuccess) {
        SMI_HIP_CHECK(q);
    }
    *out = c->interior_stream;
    *own = true;
    return SMI_SUCCESS;
}

// One rank's tile during a run: what every phase reads, and the ping-pong
// index its passes flip.
struct Tile {
    Comm *c;
    float *buf[2];
    int rows, cols;
    Neighbours nb;
    int side_mask;        // bit 0..3: neighbour on side top, bottom, left, right
    // src: this rank's tile of the source term (a source run); resid: the
    // residual word while the final phase of a residual run is enqueued;
    // g_halo: set by a K-phase of a source run
    Variant v;
    int cur;              // index of the buffer holding the current state
    const float *in() const { return buf[cur]; }
    float *out() const { return buf[cur ^ 1]; }
    bool has(int side) const { return (side_mask >> side) & 1; }
};

// One halo exchange: up to eight messages in the order top, bottom, left,
// right, tl, tr, bl, br (peer < 0: no such neighbour).  The kernels see the
// receive side as const; the transport writes it.
struct HaloMsg {
    int peer;
    const float *send, *recv;
    size_t bytes;
};
struct HaloMsgs {
    HaloMsg m[8];
};

// the one place a receive-side `const float *` of the device-facing halo
// structs becomes the transport's writable buffer
static void *recv_buf(const HaloMsg &m) { return const_cast<float *>(m.recv); }

// The side messages at depth d rows / dc columns: the tile's first / last d
// rows are sent straight from it, its packed first / last dc columns from the
// staging; no corners (the depth-2 and depth-K phases add theirs).
static HaloMsgs side_msgs(const Tile &t, const float *tile, int d, int dc, const float *top, const float *bot,
                          const float *left, const float *right, const float *send_left, const float *send_right) {
    const size_t rb = (size_t)d * t.cols * sizeof(float), cb = (size_t)t.rows * dc * sizeof(float);
    HaloMsgs x;
    x.m[0] = {t.nb.top, tile, top, rb};
    x.m[1] = {t.nb.bottom, tile + (size_t)(t.rows - d) * t.cols, bot, rb};
    x.m[2] = {t.nb.left, send_left, left, cb};
    x.m[3] = {t.nb.right, send_right, right, cb};
    for (int k = 4; k < 8; ++k) x.m[k] = {-1, nullptr, nullptr, 0};
    return x;
}

// Depth-2 exchange (once per pair of steps): two rows / two columns per
// side neighbour, one corner cell per diagonal neighbour.
static HaloMsgs msgs2(const Tile &t, const float *tile, const Halo2 &h) {
    HaloMsgs x = side_msgs(t, tile, 2, 2, h.top2, h.bot2, h.left2, h.right2, h.send_left2, h.send_right2);
    const int diag[4] = {t.nb.tl, t.nb.tr, t.nb.bl, t.nb.br};
    for (int k = 0; k < 4; ++k) x.m[4 + k] = {diag[k], h.send_corner + k, h.corner + k, sizeof(float)};
    return x;
}

// Depth-K exchange (once per K steps): K rows / KC = kc_of(K) columns per
// side neighbour, one K x KC block per diagonal neighbour.
static HaloMsgs msgsk(const Tile &t, const float *tile, int K, const HaloK &h) {
    HaloMsgs x = side_msgs(t, tile, K, kc_of(K), h.top, h.bot, h.left, h.right, h.send_left, h.send_right);
    const int diag[4] = {t.nb.tl, t.nb.tr, t.nb.bl, t.nb.br};
    const size_t kb = (size_t)K * kc_of(K) * sizeof(float);
    for (int k = 0; k < 4; ++k) x.m[4 + k] = {diag[k], h.send_corner[k], h.corner[k], kb};
    return x;
}

// Posts the messages in one transport group, each peer's send before its
// receive.  depth_k: the exchange of a K-step phase (the rehearsal switches
// act on that one only).
static int exchange(Comm *c, const HaloMsgs &x, bool depth_k, hipStream_t s) {
    Transport *tp = c->transport.get();
#ifdef SMI_LOOPBACK_REHEARSAL
    if (depth_k && getenv("SMI_LOOPBACK_NOXCHG")) return SMI_SUCCESS;  // rehearsal: price bands + interior alone
    const char *fused = getenv("SMI_LOOPBACK_FUSED"), *heavy = getenv("SMI_LOOPBACK_HEAVY");
    if (depth_k && (fused || heavy) && x.m[0].peer == 0 && x.m[2].peer == 0 && x.m[4].peer == 0) {
        // rehearsal, own neighbour on every side: the same 8 messages as one
        // copy kernel (like one RCCL group), message i landing in the receive
        // buffer of the opposite message; HEAVY: with rcclGenericKernel's
        // footprint, SMI_LOOPBACK_HEAVY workgroups (RCCL's channels)
        const void *src[8];
        void *dst[8];
        size_t by[8];
        for (int i = 0; i < 8; ++i) {
            src[i] = x.m[i].send;
            dst[i] = recv_buf(x.m[i < 4 ? i ^ 1 : 11 - i]);
            by[i] = x.m[i].bytes;
        }
        return fused ? launch_copies(src, dst, by, 8, s) : launch_heavy_copies(src, dst, by, 8, atoi(heavy), s);
    }
#endif
    Group grp(tp);
    SMI_TRY(grp.begin(s));
    for (const HaloMsg &m : x.m) {
        if (m.peer < 0) continue;
        SMI_TRY(tp->send(m.send, m.bytes, m.peer));
        SMI_TRY(tp->recv(recv_buf(m), m.bytes, m.peer));
    }
    return grp.end();
}

// Halo staging.  Depth 2 (its inner row/column doubles as the depth-1
// halo): top2 | bot2 | left2 | right2 | corner(4) | send_left2 |
// send_right2 | send_corner(4); then depth K (16-byte aligned): top | bot
// (K x cols) | left | right | send_left | send_right (rows x KC, [row][k])
// | 4 + 4 K x KC corners.  The regions are sized for the deepest phase; a
// shallower phase (the remainder pass) lays its depth out densely from
// the start of each region.  Every pointer is a valid allocation, also for
// sides without a neighbour (their values are never used; the kernels rely
// on it).
static size_t halo2_elems(int rows, int cols) { return (4 * (size_t)cols + 8 * (size_t)rows + 8 + 3) / 4 * 4; }
static size_t halok_elems(int rows, int cols, int kmax) {
    const size_t kc = kc_of(kmax);
    return kmax ? 2 * (size_t)kmax * cols + 4 * (size_t)rows * kc + 8 * (size_t)kmax * kc : 0;
}

static Halo2 halo2_layout(float *base, int rows, int cols) {
    const size_t c2 = 2 * (size_t)cols, r2 = 2 * (size_t)rows;
    float *left2 = base + 2 * c2, *corner = left2 + 2 * r2, *send_left2 = corner + 4;
    Halo2 h;
    h.top2 = base;
    h.bot2 = base + c2;
    h.left2 = left2;
    h.right2 = left2 + r2;
    h.corner = corner;
    h.send_left2 = send_left2;
    h.send_right2 = send_left2 + r2;
    h.send_corner = send_left2 + 2 * r2;
    return h;
}

static HaloK halok_layout(float *base, int rows, int cols, int kmax) {
    const size_t rb = (size_t)kmax * cols, cb = (size_t)rows * kc_of(kmax), kb = (size_t)kmax * kc_of(kmax);
    float *left = base + 2 * rb, *corners = left + 4 * cb;
    HaloK h;
    h.top = base;
    h.bot = base + rb;
    h.left = left;
    h.right = left + cb;
    h.send_left = left + 2 * cb;
    h.send_right = left + 3 * cb;
    for (int k = 0; k < 4; ++k) {
        h.corner[k] = corners + k * kb;
        h.send_corner[k] = corners + (4 + k) * kb;
    }
    return h;
}

// K-step passes: the interior sweep of a tile with neighbours on side_mask
// (bit 0..3: top, bottom, left, right) stays K rows / 4*ceil(K/4) columns
// clear of every halo-facing side (the band kernel computes those bands
// beside it); global edges are handled inside the sweep (stencilk.h).
static SweepKArgs interior_rect(int rows, int cols, int K, int side_mask) {
    const int kc = kc_of(K);
    SweepKArgs a{};
    a.rows = rows;
    a.cols = cols;
    a.row_lo = (side_mask & 1) ? K : 0;
    a.row_hi = (side_mask & 2) ? rows - K : rows;
    a.col_lo = (side_mask & 4) ? kc : 0;
    a.col_hi = (side_mask & 8) ? cols - kc : cols;
    a.gT = !(side_mask & 1);
    a.gB = !(side_mask & 2);
    a.gL = !(side_mask & 4);
    a.gR = !(side_mask & 8);
    return a;
}

static int ensure_halo(Comm *c, size_t elems) {
    if (c->halo_elems < elems) {
        if (c->halo) SMI_HIP_CHECK(hipFree(c->halo));
        c->halo = nullptr;
        SMI_HIP_CHECK(hipMalloc(&c->halo, elems * sizeof(float)));
        c->halo_elems = elems;
    }
    return SMI_SUCCESS;
}

static Neighbours neighbours_of(int rank, int px, int py) {
    // rank -> (i_px, i_py), examples/host/stencil_smi.cpp:133-134
    const int ipx = rank / py, ipy = rank % py;
    Neighbours nb;
    if (ipx > 0) nb.top = (ipx - 1) * py + ipy;
    if (ipx < px - 1) nb.bottom = (ipx + 1) * py + ipy;
    if (ipy > 0) nb.left = ipx * py + ipy - 1;
    if (ipy < py - 1) nb.right = ipx * py + ipy + 1;
    if (nb.top >= 0 && nb.left >= 0) nb.tl = (ipx - 1) * py + ipy - 1;
    if (nb.top >= 0 && nb.right >= 0) nb.tr = (ipx - 1) * py + ipy + 1;
    if (nb.bottom >= 0 && nb.left >= 0) nb.bl = (ipx + 1) * py + ipy - 1;
    if (nb.bottom >= 0 && nb.right >= 0) nb.br = (ipx + 1) * py + ipy + 1;
    return nb;
}

// The phases of a run: K-step passes of the configured K (clipped to what the
// tile holds: a multi-rank tile needs 2K x 2K).  A remainder of 3 or more
// steps is spread over the passes instead -- the same number of passes,
// balanced to within one step (T = 20 at K = 12: 10 + 10, not 12 + 8; a pass
// costs about one HBM sweep whatever its depth, and the deeper one of an
// unbalanced split pays for its extra levels: 8192^2 T = 20 0.2308 -> 0.2245
// ms, T = 30 0.3247 -> 0.3178 ms, profiles/r02/plan_split.jsonl); a remainder
// of 1 or 2 steps stays a pair and/or a single step (12 + 1 beats 7 + 6).
// Every phase starts from halos of the current state, so the split changes
// scheduling only, never a bit of the result.
struct Plan {
    int nph = 0;
    int k[4] = {0, 0, 0, 0};  // steps per pass
    int n[4] = {0, 0, 0, 0};  // passes
    bool resid_last = false;  // the last phase is the residual pass of smi_stencil_run_residual
    int passes() const { return n[0] + n[1] + n[2] + n[3]; }
    void add(int steps, int count) {
        if (count > 0) {
            k[nph] = steps;
            n[nph] = count;
            ++nph;
        }
    }
};

// The configured steps per pass as far as this tile can hold them (0: no
// K-step passes), before the deep sweep's own height rule.
static int tile_fuse(int rows, int cols, bool multi) {
    const int fuse = g_tune.fuse;
    int K = fuse >= SWEEPK_MIN ? fuse : 0;
    if (K && multi) {
        // a multi-rank tile holds the K-row bands and the float4-aligned
        // K-column bands (4 * ceil(K / 4) wide) of both sides
        K = std::min(K, rows / 2);
        while (K > 0 && 8 * ((K + 3) / 4) > cols) --K;
    }
    return K;
}

// K-step passes for `rest` steps under the balanced-remainder rule above;
// returns the steps left to shallower phases (0, 1 or 2 -- or all of them
// when rest < K and cannot be one pass of its own)
static int add_k_passes(Plan &p, int K, int rest) {
    const int passes = rest / K + 1, base = rest / passes, extra = rest % passes;
    if (rest % K >= SWEEPK_MIN && base >= SWEEPK_MIN) {
        p.add(base + 1, extra);
        p.add(base, passes - extra);
        return 0;
    }
    p.add(K, rest / K);
    return rest % K;
}

static Plan make_plan(int rows, int cols, int timesteps, bool multi) {
    Plan p;
    const int fuse = g_tune.fuse;
    int K = tile_fuse(rows, cols, multi);
    if (K > SWEEPK_MAX) {
        // deep passes (stencild.h) need a tall enough sweep rectangle (a
        // multi-rank interior loses K rows per side with a neighbour; the
        // plan does not know which sides have one and assumes both)
        if (!sweepd_fits(K, interior_rect(rows, cols, K, multi ? 1 | 2 : 0))) K = SWEEPK_MAX;
    }
    if (cols < 8 || K < SWEEPK_MIN) K = 0;
    int rest = K ? add_k_passes(p, K, timesteps) : timesteps;
    if (fuse >= 2 && rows >= 4 && cols >= 8) {
        p.add(2, rest / 2);
        rest %= 2;
    }
    p.add(1, rest);
    return p;
}

// smi_stencil_run_residual: the run ends in ONE pass whose kernels also take
// |x_T - x_{T-1}|.  That is a pass of K_r = min(steps per pass, 12,
// timesteps) steps under the tile's clipping rules (the residual lives in the
// K = 3..12 sweep and the one-wave-per-segment band kernel; the rotating-ring
// sweep and the lean band kernel have none), after timesteps - K_r steps
// planned as smi_stencil_run plans them; or, when K_r < 3 (a fusion setting
// of 1 or 2, fewer than 3 steps, tiles that run single steps only), one
// single residual step after timesteps - 1 planned steps.  The residual pass
// is its own last phase; make_plan yields at most 3 phases (two balanced
// depths, or K + pair + single), so 4 still hold every schedule.
static Plan make_plan_residual(int rows, int cols, int timesteps, bool multi) {
    int kr = std::min(std::min(tile_fuse(rows, cols, multi), variant_k(Family::Sweep, Kind::Res).hi), timesteps);
    if (cols < 8 || kr < SWEEPK_MIN) kr = 1;
    Plan p = make_plan(rows, cols, timesteps - kr, multi);
    p.add(kr, 1);
    p.resid_last = true;
    return p;
}

// A source run (smi_stencil_run_source; stencilk.h "Source instantiations").
// One tile with cols >= 8: passes of min(steps per pass, SWEEPK_SRC_MAX) steps
// under make_plan's balanced-remainder rule; a remainder of 1 or 2 steps runs
// as single steps (there is no pair kernel with a source), and so does a
// fusion setting below 3.  Multi-rank: single steps through the depth-1
// exchange phase by default; with smi_stencil_set_source_bands(1) the same
// rule at the K the tile holds (tile_fuse: 2K x 2KC), the bands by
// bandk_src_kernel, and a remainder of 1 or 2 as single steps in a phase of
// their own.  At most 2 phases.  resid: the checked step of
// smi_stencil_solve_source, one single residual step (the fused source sweep
// and band kernel have no residual variant).
static Plan make_plan_source(int rows, int cols, int timesteps, bool multi, bool resid) {
    Plan p;
    int K = 0;
    if (cols >= 8 && !resid && (!multi || g_tune.source_bands))
        K = std::min(multi ? tile_fuse(rows, cols, true) : g_tune.fuse, variant_k(Family::Sweep, Kind::Src).hi);
    p.add(1, K >= SWEEPK_MIN ? add_k_passes(p, K, timesteps) : timesteps);
    p.resid_last = resid;
    return p;
}
static_assert(variant_k(Family::Band, Kind::Src).hi == variant_k(Family::Sweep, Kind::Src).hi &&
                  variant_k(Family::Band, Kind::Res).hi == variant_k(Family::Sweep, Kind::Res).hi,
              "the planners take a K-step pass's depth from the sweep; its bands run the same K");

// The schedule of a run of `kind`: smi_stencil_run (Plain), smi_stencil_run_residual
// (Res), a source run (Src) or the checked source step (SrcRes).
static Plan plan_for(Kind kind, int rows, int cols, int timesteps, bool multi) {
    switch (kind) {
    case Kind::Plain: return make_plan(rows, cols, timesteps, multi);
    case Kind::Res: return make_plan_residual(rows, cols, timesteps, multi);
    default: return make_plan_source(rows, cols, timesteps, multi, kind == Kind::SrcRes);
    }
}

// single-step / pair arguments (halo views and buffers set by the phases)
static SweepArgs step_args(const Tile &t) {
    SweepArgs a{};
    a.rows = t.rows;
    a.cols = t.cols;
    for (int k = 0; k < 4; ++k) a.mode[k] = t.has(k) ? SMI_SIDE_HALO : SMI_SIDE_COPY;
    return a;
}
static Sweep2Args pair_args(const Tile &t) {
    Sweep2Args a2{};
    a2.rows = t.rows;
    a2.cols = t.cols;
    for (int k = 0; k < 4; ++k) a2.skip[k] = t.has(k);
    return a2;
}

// The single-tile run: no halos, no exchange, no events.
static int run_single(Tile &t, const Plan &plan, unsigned int *resid, hipStream_t s) {
    SweepArgs a = step_args(t);
    Sweep2Args a2 = pair_args(t);
    for (int ph = 0; ph < plan.nph; ++ph) {
        const int K = plan.k[ph];
        t.v.resid = plan.resid_last && ph == plan.nph - 1 ? resid : nullptr;
        SweepKArgs ak = interior_rect(t.rows, t.cols, K, 0);
        for (int p = 0; p < plan.n[ph]; ++p, t.cur ^= 1) {
            if (K >= SWEEPK_MIN) {
                ak.in = t.in();
                ak.out = t.out();
                SMI_TRY(launch_sweepk(K, ak, t.v, 0, s));
            } else if (K == 2) {
                a2.in = t.in();
                a2.out = t.out();
                SMI_TRY(launch_sweep2(a2, s));
            } else {
                a.in = t.in();
                a.out = t.out();
                SMI_TRY(launch_sweep(a, t.v, s));
            }
        }
    }
    return SMI_SUCCESS;
}

// Who records a pass's two ordering events.  ByDispatch (K-step passes): the
// ring / interior launches are handed the event as `stop` and record it by
// their own dispatch (no marker packets between kernels; ~4 us per pass,
// tools/streambench).  AfterLaunch (pairs, single steps): their kernels
// ignore `stop`, and pass() records the event after them.
enum class Events { ByDispatch, AfterLaunch };

// The pass scheduler of a multi-rank run.
// Schedule (two streams, no host synchronisation between passes):
//   comm stream : [wait interior(t-1)] band(t) -> rec E_edge(t) -> exchange(t)
//   main stream : [wait E_edge(t-1)] interior(t)    -> rec E_int(t)
// The band kernel (the depth-K bands; the depth-2 / depth-1 phases use
// their ring / edge kernels) reads in(t) (interior cells from interior(t-1),
// halo-facing cells from its own predecessor) and the halos of
// exchange(t-1); the interior reads only in(t), never a halo vector, so
// neither the halo-facing cells nor the xGMI exchange sit on its path.
// Each phase (K-step passes, the remainder pass, pairs, singles) starts
// from halos of the current state: the neighbours' current edges (for
// the first phase the reference's artificial timestep t=0,
// stencil_smi.cl:26-29,183-224).
struct PassSched {
    hipStream_t s, cs;  // main (interior) stream, comm stream
    hipEvent_t ev_edge, ev_int, ev_edge_alt;
    bool overlap, host_join;
    int kpass;             // K-step passes of the current phase
    hipEvent_t last_band;  // completion of the phase's last band kernel (host join)

    int phase_start() {
        SMI_HIP_CHECK(hipEventRecord(ev_int, s));
        SMI_HIP_CHECK(hipStreamWaitEvent(cs, ev_int, 0));
        return SMI_SUCCESS;
    }

    // One pass of a phase: bands (comm stream) + interior (main stream).
    // ring(st, stop) / interior(st, stop): the launches, stop (nullable) as
    // under Events; xchg(tile, st): the halo exchange of the pass's result
    // `next` (nullptr: the phase's last pass, whose result the next phase
    // exchanges at the depth it needs).
    template <class Ring, class Interior, class Xchg>
    int pass(const Ring &ring, const Interior &interior, const Xchg &xchg, const float *next, Events ev) {
        const bool carried = ev == Events::ByDispatch;
        if (overlap && carried && host_join) {
            // K-step passes, host-observed join (see join_band above):
            // band(t) carries ev_band[t & 1]; interior(t) follows band(t-1)
            // with no wait packet when the host has seen band(t-1) finish
            hipEvent_t ev_cur = (kpass & 1) ? ev_edge_alt : ev_edge, ev_prev = (kpass & 1) ? ev_edge : ev_edge_alt;
            SMI_TRY(ring(cs, ev_cur));
            rehearsal_stall(kpass);
            if (kpass > 0) SMI_TRY(join_band(ev_prev));
            SMI_TRY(interior(s, ev_int));
            if (next) SMI_TRY(xchg(next, cs));
            SMI_HIP_CHECK(hipStreamWaitEvent(cs, ev_int, 0));
            last_band = ev_cur;
            ++kpass;
        } else if (overlap) {
            // Overlapped, the main stream waits for the bands on the device.
            // The interior is enqueued before the exchange: posting the
            // transport's sends/receives costs host time (RCCL group, or
            // event + copy per message in-process) that must not delay the
            // interior's launch -- the trace of an interior rank showed the
            // main stream idle ~100 us per pass behind the exchange calls.
            SMI_TRY(ring(cs, carried ? ev_edge : nullptr));
            if (!carried) SMI_HIP_CHECK(hipEventRecord(ev_edge, cs));
            if (carried) {
                rehearsal_stall(kpass);
                ++kpass;
            }
            SMI_TRY(interior(s, carried ? ev_int : nullptr));
            if (!carried) SMI_HIP_CHECK(hipEventRecord(ev_int, s));
            SMI_HIP_CHECK(hipStreamWaitEvent(s, ev_edge, 0));
            if (next) SMI_TRY(xchg(next, cs));
            SMI_HIP_CHECK(hipStreamWaitEvent(cs, ev_int, 0));
        } else {
            // No overlap: everything but the exchange on the main stream.
            SMI_HIP_CHECK(hipEventRecord(ev_edge, cs));
            SMI_HIP_CHECK(hipStreamWaitEvent(s, ev_edge, 0));
            SMI_TRY(ring(s, nullptr));
            SMI_TRY(interior(s, nullptr));
            SMI_HIP_CHECK(hipEventRecord(ev_int, s));
            SMI_HIP_CHECK(hipStreamWaitEvent(cs, ev_int, 0));
            if (next) SMI_TRY(xchg(next, cs));
        }
        return SMI_SUCCESS;
    }
};

// ---- K steps per pass (depth-K halos)
// t.v.src (a source run): the source instantiations of both kernels, and g's own
// depth-K halos in gk -- a second staging, exchanged here once for the phase
// (g is constant over a run, but the phases differ in depth; nothing is kept
// across calls: the caller may change src between runs).
static int k_passes(Tile &t, PassSched &sc, int K, int npass, const HaloK &hk, const HaloK &gk) {
    SweepKArgs ak = interior_rect(t.rows, t.cols, K, t.side_mask);
    BandKArgs bk{};
    bk.rows = t.rows;
    bk.cols = t.cols;
    for (int k = 0; k < 4; ++k) bk.has[k] = t.has(k);
    bk.pack = t.side_mask != 0;
    bk.h = hk;
    // t.v.resid: the residual pass -- both kernels' residual instantiations, one word
    Variant v = t.v;
    if (v.src) v.g_halo = &gk;
    auto ring = [&](hipStream_t st, hipEvent_t stop) { return launch_bandk(K, bk, v, g_tune.band_reserve, st, stop); };
    auto interior = [&](hipStream_t st, hipEvent_t stop) {
        return launch_sweepk(K, ak, v, g_tune.band_reserve, st, stop);
    };
    auto xchgk = [&](const float *tile, hipStream_t st) { return exchange(t.c, msgsk(t, tile, K, hk), true, st); };
    SMI_TRY(launch_packk(t.in(), t.rows, t.cols, K, hk, sc.cs));
    SMI_TRY(xchgk(t.in(), sc.cs));
    if (v.src) {
        // g's halos, directly behind the state's on the comm stream: every
        // rank posts the two exchanges in this order
        SMI_TRY(launch_packk(v.src, t.rows, t.cols, K, gk, sc.cs));
        SMI_TRY(exchange(t.c, msgsk(t, v.src, K, gk), true, sc.cs));
    }
    sc.kpass = 0;
    for (int p = 0; p < npass; ++p, t.cur ^= 1) {
        bk.in = ak.in = t.in();
        bk.out = ak.out = t.out();
        SMI_TRY(sc.pass(ring, interior, xchgk, p < npass - 1 ? ak.out : nullptr, Events::ByDispatch));
    }
    // whatever runs next on the main stream reads the last bands:
    // joined on the host as well (no wait packet on the interior
    // stream, see join_band)
    if (sc.host_join && sc.last_band) SMI_TRY(join_band(sc.last_band));
    return SMI_SUCCESS;
}

// ---- pairs of steps (depth-2 halos)
static int pair_passes(Tile &t, PassSched &sc, int npass, const Halo2 &h2) {
    Sweep2Args a2 = pair_args(t);
    auto ring = [&](hipStream_t st, hipEvent_t) { return launch_ring2(a2, h2, st); };
    auto interior = [&](hipStream_t st, hipEvent_t) { return launch_sweep2(a2, st); };
    auto xchg2 = [&](const float *tile, hipStream_t st) { return exchange(t.c, msgs2(t, tile, h2), false, st); };
    SMI_TRY(launch_pack2(t.in(), t.rows, t.cols, h2, sc.cs));
    SMI_TRY(xchg2(t.in(), sc.cs));
    for (int p = 0; p < npass; ++p, t.cur ^= 1) {
        a2.in = t.in();
        a2.out = t.out();
        SMI_TRY(sc.pass(ring, interior, xchg2, p < npass - 1 ? a2.out : nullptr, Events::AfterLaunch));
    }
    return SMI_SUCCESS;
}

// ---- single steps (depth-1 halos: the inner row / column of the depth-2
// staging -- row -1, row X, col -1, col Y -- and the packed depth-1 sends)
static int single_steps(Tile &t, PassSched &sc, int npass, const Halo2 &h2) {
    SweepArgs a = step_args(t);
    a.halo[0] = h2.top2 + t.cols;
    a.halo[1] = h2.bot2;
    a.halo[2] = h2.left2 + t.rows;
    a.halo[3] = h2.right2;
    float *s_left = h2.send_left2 + t.rows, *s_right = h2.send_right2;  // staging only
    a.send_left = t.nb.left >= 0 ? s_left : nullptr;
    a.send_right = t.nb.right >= 0 ? s_right : nullptr;
    SweepArgs inner = a;  // interior launch: halo-facing sides left to the edge kernel
    for (int k = 0; k < 4; ++k)
        if (inner.mode[k] == SMI_SIDE_HALO) inner.mode[k] = SMI_SIDE_SKIP;
    inner.send_left = inner.send_right = nullptr;
    // (t.v.src: the source kernels, each rank reading its own tile of src)
    auto edge = [&](hipStream_t st, hipEvent_t) { return launch_edge(a, t.side_mask, t.v, st); };
    auto interior = [&](hipStream_t st, hipEvent_t) { return launch_sweep(inner, t.v, st); };
    // without overlap the full sweep reads the halos itself
    auto no_edge = [&](hipStream_t, hipEvent_t) { return (int)SMI_SUCCESS; };
    auto full = [&](hipStream_t st, hipEvent_t) { return launch_sweep(a, t.v, st); };
    auto xchg1 = [&](const float *tile, hipStream_t st) {
        const HaloMsgs x = side_msgs(t, tile, 1, 1, a.halo[0], a.halo[1], a.halo[2], a.halo[3], s_left, s_right);
        return exchange(t.c, x, false, st);
    };
    SMI_TRY(launch_pack_cols(t.in(), t.rows, t.cols, a.send_left, a.send_right, sc.cs));
    SMI_TRY(xchg1(t.in(), sc.cs));
    for (int p = 0; p < npass; ++p, t.cur ^= 1) {
        a.in = inner.in = t.in();
        a.out = inner.out = t.out();
        const float *next = p < npass - 1 ? a.out : nullptr;
        if (sc.overlap)
            SMI_TRY(sc.pass(edge, interior, xchg1, next, Events::AfterLaunch));
        else
            SMI_TRY(sc.pass(no_edge, full, xchg1, next, Events::AfterLaunch));
    }
    return SMI_SUCCESS;
}

// The multi-rank run: streams and events, the phases, the join back to the
// caller's stream.
static int run_multi(Tile &t, const Plan &plan, unsigned int *resid, hipStream_t user) {
    Comm *c = t.c;
    PassSched sc{};
    sc.s = user;
    sc.cs = c->comm_stream;
    hipEvent_t ev_fin;
    SMI_TRY(comm_event(c, 0, &sc.ev_edge));
    SMI_TRY(comm_event(c, 1, &sc.ev_int));
    SMI_TRY(comm_event(c, 2, &sc.ev_edge_alt));
    SMI_TRY(comm_event(c, 4, &ev_fin));
    sc.overlap = g_tune.overlap != 0;
    bool own_stream = false;
    if (sc.overlap) SMI_TRY(interior_stream(c, user, &sc.s, &own_stream));
    sc.host_join = sc.overlap && host_join_enabled();

    int kmax = 0;  // deepest K-step phase (sizes the depth-K staging)
    for (int i = 0; i < plan.nph; ++i) kmax = std::max(kmax, plan.k[i] >= SWEEPK_MIN ? plan.k[i] : 0);
    // a source run with a K-phase: g's depth-K staging behind the state's
    const size_t need2 = halo2_elems(t.rows, t.cols), needk = halok_elems(t.rows, t.cols, kmax);
    SMI_TRY(ensure_halo(c, need2 + needk + (t.v.src ? needk : 0)));
    const Halo2 h2 = halo2_layout(c->halo, t.rows, t.cols);

    for (int ph = 0; ph < plan.nph; ++ph) {
        const int K = plan.k[ph], npass = plan.n[ph];
        t.v.resid = plan.resid_last && ph == plan.nph - 1 ? resid : nullptr;
        SMI_TRY(sc.phase_start());
        if (K >= SWEEPK_MIN)
            SMI_TRY(k_passes(t, sc, K, npass, halok_layout(c->halo + need2, t.rows, t.cols, kmax),
                             halok_layout(c->halo + need2 + (t.v.src ? needk : 0), t.rows, t.cols, kmax)));
        else if (K == 2)
            SMI_TRY(pair_passes(t, sc, npass, h2));
        else
            SMI_TRY(single_steps(t, sc, npass, h2));
    }
    // the caller's stream owns the result: join the comm stream (and the
    // interior stream when the run had one)
    SMI_HIP_CHECK(hipEventRecord(sc.ev_edge, sc.cs));
    SMI_HIP_CHECK(hipStreamWaitEvent(user, sc.ev_edge, 0));
    if (own_stream) {
        SMI_HIP_CHECK(hipEventRecord(ev_fin, sc.s));
        SMI_HIP_CHECK(hipStreamWaitEvent(user, ev_fin, 0));
    }
    return SMI_SUCCESS;
}

// the tile / grid arguments smi_stencil_run and smi_stencil_solve share
static int check_grid(const Comm *c, const float *buf0, const float *buf1, int x_local, int y_local, int px, int py) {
    SMI_TRY(check_tile(buf0, buf1, x_local, y_local));
    SMI_ARG_CHECK(px >= 1 && py >= 1 && px * py == c->size, "px*py must equal the communicator size");
    return SMI_SUCCESS;
}

static int find_comm(SMI_Comm comm, Comm **c) {
    *c = lookup_comm(comm);
    if (*c) return SMI_SUCCESS;
    set_error("unknown communicator");
    return SMI_ERR_BAD_COMM;
}

// smi_stencil_run (resid == nullptr), or smi_stencil_run_residual: the
// schedule of make_plan_residual, whose last pass's kernels also
// max-accumulate |x_T - x_{T-1}| into *resid (timesteps >= 1; one step is the
// checked step of smi_stencil_solve: a single residual step, stencil.hip).
// v.src: a source run, the schedule of make_plan_source; with v.resid it is the
// one checked step of smi_stencil_solve_source.
static int run_steps(Comm *c, float *buf0, float *buf1, int x_local, int y_local, int px, int py, int timesteps,
                     SMI_Stream stream_, int *result_index, const Variant &v) {
    unsigned int *const resid = v.resid;
    const float *const src = v.src;
    SMI_TRY(check_grid(c, buf0, buf1, x_local, y_local, px, py));
    if (src) SMI_TRY(check_src(src, buf0, buf1, x_local, y_local));
    SMI_ARG_CHECK(!(src && resid) || timesteps == 1, "a source run takes its residual from one single step");
    SMI_ARG_CHECK(timesteps >= 0, "timesteps < 0");
    SMI_ARG_CHECK(result_index, "NULL result_index");
    SMI_ARG_CHECK(!resid || timesteps >= 1, "a residual run takes at least one step");
    Tile t{c, {buf0, buf1}, x_local, y_local, neighbours_of(c->rank, px, py), 0, Variant{nullptr, src}, 0};
#ifdef SMI_LOOPBACK_REHEARSAL
    // Timing-rehearsal build only (never the product library; built by
    // `smi_amd/build.py --rehearsal`, driven by tools/rehearsal.py): with
    // SMI_LOOPBACK=1 a 1x1 run is its own neighbour on every side and
    // diagonal, so one GPU replays the full per-pass work of an interior rank
    // of a large decomposition (band kernel, 8-way exchange through the
    // transport, interior sweep) with the same stream schedule.  The halos
    // then wrap around, so the numbers differ from the stencil's.
    Neighbours &nb = t.nb;
    if (px == 1 && py == 1 && c->size == 1 && getenv("SMI_LOOPBACK"))
        nb.top = nb.bottom = nb.left = nb.right = nb.tl = nb.tr = nb.bl = nb.br = 0;
#endif
    const int side_nb[4] = {t.nb.top, t.nb.bottom, t.nb.left, t.nb.right};
    for (int k = 0; k < 4; ++k)
        if (side_nb[k] >= 0) t.side_mask |= 1 << k;

    const bool multi = t.side_mask != 0;
    const Plan plan = plan_for(v.kind(), t.rows, t.cols, timesteps, multi);
    *result_index = plan.passes() & 1;
    prof_break_chain();  // markers chain only between this run's own passes
    if (timesteps == 0) return SMI_SUCCESS;
    return multi ? run_multi(t, plan, resid, (hipStream_t)stream_) : run_single(t, plan, resid, (hipStream_t)stream_);
}


}  // namespace smi

using namespace smi;

extern "C" {

int smi_stencil_set_fusion(int steps_per_pass, int rows_per_wave, int rows_in_flight) {
    if (steps_per_pass > 0) {
        SMI_ARG_CHECK(steps_per_pass <= SWEEPD_MAX, "steps_per_pass must be 1..20");
        g_tune.fuse = steps_per_pass;
    }
    // rows_per_wave / rows_in_flight tune the kernel of the current setting
    const bool deep = g_tune.fuse >= SWEEPK_MIN;
    if (rows_per_wave > 0) (deep ? g_tune.htk : g_tune.ht2) = rows_per_wave;
    if (rows_per_wave < 0 && deep) g_tune.htk = 0;  // automatic: one round of resident waves
    if (rows_in_flight > 0 && !deep) {
        SMI_ARG_CHECK(rows_in_flight == 1 || rows_in_flight == 2 || rows_in_flight == 4 || rows_in_flight == 8,
                      "rows_in_flight must be 1, 2, 4 or 8");
        g_tune.u2 = rows_in_flight;
    }
    // the K-step sweep's pipeline depth is fixed at build time;
    // rows_in_flight is accepted and ignored there
    return SMI_SUCCESS;
}

int smi_stencil_get_fusion(int *steps_per_pass, int *rows_per_wave, int *rows_in_flight) {
    const bool deep = g_tune.fuse >= SWEEPK_MIN;
    if (steps_per_pass) *steps_per_pass = g_tune.fuse;
    if (rows_per_wave) *rows_per_wave = deep ? g_tune.htk : g_tune.ht2;
    if (rows_in_flight) *rows_in_flight = deep ? g_tune.uk : g_tune.u2;
    return SMI_SUCCESS;
}

int smi_stencil_set_bands(int reserve_waves, int interior_rounds) {
    SMI_ARG_CHECK(reserve_waves <= 65536 && interior_rounds <= 64, "reserve_waves / interior_rounds out of range");
    if (reserve_waves >= 0) g_tune.band_reserve = reserve_waves;
    if (interior_rounds >= 0) g_tune.rounds_multi = std::max(1, interior_rounds);
    return SMI_SUCCESS;
}

int smi_stencil_get_bands(int *reserve_waves, int *interior_rounds) {
    if (reserve_waves) *reserve_waves = g_tune.band_reserve;
    if (interior_rounds) *interior_rounds = g_tune.rounds_multi;
    return SMI_SUCCESS;
}

int smi_stencil_set_band_kernel(int lean) {
    SMI_ARG_CHECK(lean <= 1, "band kernel: 0 (one wave per segment) or 1 (lean, beside the interior)");
    if (lean >= 0) g_tune.band_lean = lean;
    return SMI_SUCCESS;
}

int smi_stencil_get_band_kernel(int *lean) {
    if (lean) *lean = g_tune.band_lean;
    return SMI_SUCCESS;
}

int smi_stencil_set_join(int host_join) {
    SMI_ARG_CHECK(host_join <= 1, "pass join: 0 (device-side wait) or 1 (host-observed)");
    if (host_join >= 0) g_tune.host_join = host_join;
    return SMI_SUCCESS;
}

int smi_stencil_get_join(int *host_join) {
    if (host_join) *host_join = g_tune.host_join;
    return SMI_SUCCESS;
}

int smi_stencil_set_deep(int ce16, int rev16, int waves) {
    SMI_ARG_CHECK(ce16 <= 256 && rev16 <= 256 && waves <= (1 << 20), "deep sweep settings out of range");
    if (ce16 >= 0) g_tune.deep_ce16 = ce16;
    if (rev16 >= 0) g_tune.deep_rev16 = rev16;
    if (waves >= 0) g_tune.deep_waves = waves;
    return SMI_SUCCESS;
}

int smi_stencil_get_deep(int *ce16, int *rev16, int *waves) {
    if (ce16) *ce16 = g_tune.deep_ce16;
    if (rev16) *rev16 = g_tune.deep_rev16;
    if (waves) *waves = g_tune.deep_waves;
    return SMI_SUCCESS;
}

int smi_stencil_deep_geometry(int rows, int cols, int K, int side_mask, int *waves, int *strips, int *row_blocks,
                              int *row_blocks_edge, int *min_block_rows) {
    SMI_ARG_CHECK(rows >= 1 && cols >= 4 && cols % 4 == 0, "tile must be >= 1 x 4, cols % 4 == 0");
    SMI_ARG_CHECK(side_mask >= 0 && side_mask < 16, "side_mask: bits 0..3");
    const SweepKArgs a = interior_rect(rows, cols, K, side_mask);
    SMI_ARG_CHECK(sweepd_fits(K, a), "K outside 13..20 or sweep rectangle shorter than 4K rows");
    SweepDGeom g;
    SMI_TRY(sweepd_geometry(K, a, 0, &g));
    int hmin = rows;
    for (int pass = 0; pass < 2; ++pass) {
        const int nb = pass ? g.nrb_ce : g.nrb;
        if (pass ? (g.tasks == g.n_int * g.nrb) : g.n_int == 0) continue;
        for (int rb = 0; rb < nb; ++rb) {
            int o0, o1;
            sweepd_block_rows(a, rb, nb, g.wlast, &o0, &o1);
            hmin = std::min(hmin, o1 - o0);
        }
    }
    if (waves) *waves = g.tasks;
    if (strips) *strips = g.nstrips;
    if (row_blocks) *row_blocks = g.nrb;
    if (row_blocks_edge) *row_blocks_edge = g.tasks == g.n_int * g.nrb ? 0 : g.nrb_ce;
    if (min_block_rows) *min_block_rows = hmin;
    return SMI_SUCCESS;
}

static int plan_query(Kind kind, int x_local, int y_local, int px, int py, int rank, int timesteps,
                      SMI_StencilPhase *phases, int max_phases, int *nphases, int *neighbours, int *result_index) {
    SMI_ARG_CHECK(x_local >= 1 && y_local >= 4 && y_local % 4 == 0, "tile must be >= 1 x 4, y_local % 4 == 0");
    SMI_ARG_CHECK(px >= 1 && py >= 1 && rank >= 0 && rank < px * py, "rank outside the px x py grid");
    const bool residual = kind == Kind::Res;
    SMI_ARG_CHECK(timesteps >= (residual ? 1 : 0), residual ? "a residual run takes at least one step" : "timesteps < 0");
    SMI_ARG_CHECK(nphases && (phases || max_phases == 0), "NULL output");
    const Neighbours nb = neighbours_of(rank, px, py);
    const bool multi = nb.top >= 0 || nb.bottom >= 0 || nb.left >= 0 || nb.right >= 0;
    const Plan p = plan_for(kind, x_local, y_local, timesteps, multi);
    SMI_ARG_CHECK(max_phases >= p.nph, "max_phases too small (4 always suffice)");
    for (int i = 0; i < p.nph; ++i) {
        phases[i].steps_per_pass = p.k[i];
        phases[i].passes = p.n[i];
    }
    *nphases = p.nph;
    if (neighbours) {
        const int v[8] = {nb.top, nb.bottom, nb.left, nb.right, nb.tl, nb.tr, nb.bl, nb.br};
        for (int i = 0; i < 8; ++i) neighbours[i] = v[i];
    }
    if (result_index) *result_index = p.passes() & 1;
    return SMI_SUCCESS;
}

int smi_stencil_plan(int x_local, int y_local, int px, int py, int rank, int timesteps, SMI_StencilPhase *phases,
                     int max_phases, int *nphases, int *neighbours, int *result_index) {
    return plan_query(Kind::Plain, x_local, y_local, px, py, rank, timesteps, phases, max_phases, nphases,
                      neighbours, result_index);
}

int smi_stencil_plan_source(int x_local, int y_local, int px, int py, int rank, int timesteps, SMI_StencilPhase *phases,
                            int max_phases, int *nphases, int *neighbours, int *result_index) {
    return plan_query(Kind::Src, x_local, y_local, px, py, rank, timesteps, phases, max_phases, nphases,
                      neighbours, result_index);
}

int smi_stencil_source_max_depth(int *k) {
    SMI_ARG_CHECK(k, "NULL output");
    *k = variant_k(Family::Sweep, Kind::Src).hi;
    return SMI_SUCCESS;
}

int smi_stencil_plan_residual(int x_local, int y_local, int px, int py, int rank, int timesteps,
                              SMI_StencilPhase *phases, int max_phases, int *nphases, int *neighbours,
                              int *result_index) {
    return plan_query(Kind::Res, x_local, y_local, px, py, rank, timesteps, phases, max_phases, nphases, neighbours,
                      result_index);
}

int smi_stencil_set_solve_check(int fused) {
    SMI_ARG_CHECK(fused <= 1, "solve check: 0 (a single residual step) or 1 (a fused K-step residual pass)");
    if (fused >= 0) g_tune.solve_fused = fused;
    return SMI_SUCCESS;
}

int smi_stencil_get_solve_check(int *fused) {
    if (fused) *fused = g_tune.solve_fused;
    return SMI_SUCCESS;
}

int smi_stencil_set_source_bands(int fused) {
    SMI_ARG_CHECK(fused <= 1, "source bands: 0 (multi-rank source runs take single steps) or 1 (K-step passes)");
    if (fused >= 0) g_tune.source_bands = fused;
    return SMI_SUCCESS;
}

int smi_stencil_get_source_bands(int *fused) {
    if (fused) *fused = g_tune.source_bands;
    return SMI_SUCCESS;
}

int smi_stencil_run_residual(SMI_Comm comm, float *buf0, float *buf1, int x_local, int y_local, int px, int py,
                             int timesteps, unsigned int *resid_bits, SMI_Stream stream_, int *result_index) {
    Comm *c = nullptr;
    SMI_TRY(find_comm(comm, &c));
    SMI_ARG_CHECK(timesteps >= 1, "a residual run takes at least one step");
    SMI_ARG_CHECK(resid_bits && ((uintptr_t)resid_bits & 3u) == 0, "resid_bits must be a 4-byte aligned device word");
    return run_steps(c, buf0, buf1, x_local, y_local, px, py, timesteps, stream_, result_index, Variant{resid_bits});
}

int smi_stencil_run(SMI_Comm comm, float *buf0, float *buf1, int x_local, int y_local, int px, int py,
                    int timesteps, SMI_Stream stream_, int *result_index) {
    Comm *c = nullptr;
    SMI_TRY(find_comm(comm, &c));
    return run_steps(c, buf0, buf1, x_local, y_local, px, py, timesteps, stream_, result_index, Variant{});
}

int smi_stencil_run_source(SMI_Comm comm, float *buf0, float *buf1, const float *src, int x_local, int y_local, int px,
                           int py, int timesteps, SMI_Stream stream_, int *result_index) {
    // the source array first: refused before the communicator is looked up, so before any device call
    SMI_TRY(check_src(src, buf0, buf1, x_local, y_local));
    Comm *c = nullptr;
    SMI_TRY(find_comm(comm, &c));
    return run_steps(c, buf0, buf1, x_local, y_local, px, py, timesteps, stream_, result_index, Variant{nullptr, src});
}

// smi_stencil_solve (src == nullptr) and smi_stencil_solve_source: the same
// loop, the runs between check points and the checked step taking src.
static int solve_steps(SMI_Comm comm, float *buf0, float *buf1, const float *src, int x_local, int y_local, int px,
                       int py, float tol, int max_steps, int check_every, SMI_Stream stream_, int *result_index,
                       int *steps_done, float *residual, int *converged) {
    // the scalar arguments first: no device, no communicator needed to refuse them
    SMI_ARG_CHECK(tol >= 0.0f, "tol must be >= 0 and not NaN");  // false for a NaN
    SMI_ARG_CHECK(max_steps >= 0, "max_steps < 0");
    SMI_ARG_CHECK(check_every >= 1, "check_every must be >= 1");
    SMI_ARG_CHECK(result_index && steps_done && residual, "NULL result_index, steps_done or residual");
    Comm *c = nullptr;
    SMI_TRY(find_comm(comm, &c));
    SMI_TRY(check_grid(c, buf0, buf1, x_local, y_local, px, py));
    hipStream_t s = (hipStream_t)stream_;
    if (!c->resid) SMI_HIP_CHECK(hipMalloc(&c->resid, 2 * sizeof(unsigned int)));
    if (!c->resid_host) SMI_HIP_CHECK(hipHostMalloc(&c->resid_host, sizeof(unsigned int), hipHostMallocDefault));
    unsigned int *local = c->resid, *global = c->resid + 1;

    float *buf[2] = {buf0, buf1};
    int cur = 0, done = 0, idx = 0;
    float r = __builtin_inff();
    while (done < max_steps) {
        const int next = (int)std::min((long)done + check_every, (long)max_steps);
        if (g_tune.solve_fused && !src) {
            // smi_stencil_set_solve_check(1): the steps up to the check point
            // as one residual run, whose last K-step pass carries the residual
            SMI_HIP_CHECK(hipMemsetAsync(local, 0, sizeof(unsigned int), s));
            SMI_TRY(run_steps(c, buf[cur], buf[cur ^ 1], x_local, y_local, px, py, next - done, stream_, &idx, Variant{local}));
            cur ^= idx;
        } else {
            // the unchecked steps, exactly as smi_stencil_run plans that many
            SMI_TRY(run_steps(c, buf[cur], buf[cur ^ 1], x_local, y_local, px, py, next - done - 1, stream_, &idx,
                              Variant{nullptr, src}));
            cur ^= idx;
            // the checked step; its kernels run on this communicator's streams,
            // all ordered after `stream` here and joined back to it at the end
            SMI_HIP_CHECK(hipMemsetAsync(local, 0, sizeof(unsigned int), s));
            SMI_TRY(run_steps(c, buf[cur], buf[cur ^ 1], x_local, y_local, px, py, 1, stream_, &idx, Variant{local, src}));
            cur ^= idx;
        }
        done = next;
        // the same word on every rank: one integer-max allreduce of the
        // patterns (order-free, so the word smi_reduce + smi_bcast gave; the
        // float SMI_MAX starts from FLT_MIN, fold.h, and would turn a
        // residual of 0 into 1.17549435e-38)
        SMI_TRY(smi_allreduce(comm, local, global, 1, SMI_INT, SMI_MAX, 0, stream_));
        SMI_HIP_CHECK(hipMemcpyAsync(c->resid_host, global, sizeof(unsigned int), hipMemcpyDeviceToHost, s));
        SMI_HIP_CHECK(hipStreamSynchronize(s));
        r = __builtin_bit_cast(float, *c->resid_host);
        if (r <= tol) break;  // never for a NaN
    }
    *result_index = cur;
    *steps_done = done;
    *residual = r;
    if (converged) *converged = r <= tol;
    return SMI_SUCCESS;
}

int smi_stencil_solve(SMI_Comm comm, float *buf0, float *buf1, int x_local, int y_local, int px, int py, float tol,
                      int max_steps, int check_every, SMI_Stream stream_, int *result_index, int *steps_done,
                      float *residual, int *converged) {
    return solve_steps(comm, buf0, buf1, nullptr, x_local, y_local, px, py, tol, max_steps, check_every, stream_,
                       result_index, steps_done, residual, converged);
}

int smi_stencil_solve_source(SMI_Comm comm, float *buf0, float *buf1, const float *src, int x_local, int y_local,
                             int px, int py, float tol, int max_steps, int check_every, SMI_Stream stream_,
                             int *result_index, int *steps_done, float *residual, int *converged) {
    SMI_TRY(check_src(src, buf0, buf1, x_local, y_local));
    return solve_steps(comm, buf0, buf1, src, x_local, y_local, px, py, tol, max_steps, check_every, stream_,
                       result_index, steps_done, residual, converged);
}

}  // extern "C"
