/*
 * stencil.h -- the stencil_smi hot path: 4-point Jacobi with streamed halos.
 *
 * Replaces the stencil_smi application's device pipeline
 *   Read / Stencil / Write            examples/kernels/stencil_smi.cl:20-234
 *   Convert{Send,Receive}{Top,Bottom,Left,Right}
 *                                     examples/kernels/stencil_smi.cl:236-386
 * and the host decomposition (rank = i_px*PY + i_py, tile rows
 * [i_px*X_LOCAL, ..), cols [i_py*Y_LOCAL, ..))
 *                                     examples/host/stencil_smi.cpp:48-62,133-134
 * Arithmetic contract (bit-exact): interior cell
 *   out = 0.25f * (((S + W) + E) + N)    S=x[i+1][j] W=x[i][j-1] E=x[i][j+1] N=x[i-1][j]
 * in IEEE fp32 round-to-nearest with no contraction (stencil_smi.cl:153-156);
 * cells on the global edge are copied unchanged (stencil_smi.cl:143-151).
 *
 * Layout: a rank's tile is x_local rows of y_local fp32, row-major, dense
 * (row pitch = y_local), 16-byte aligned; y_local must be a multiple of 4.
 */
#ifndef SMI_STENCIL_H
#define SMI_STENCIL_H

#include "communicator.h"

#ifdef __cplusplus
extern "C" {
#endif

/* How a tile side is treated by one sweep. */
typedef enum {
    SMI_SIDE_COPY = 0,  /* side lies on the global edge: copy its cells      */
    SMI_SIDE_HALO = 1,  /* neighbour values come from the halo vector        */
    SMI_SIDE_SKIP = 2   /* leave the side's cells unwritten (computed apart) */
} SMI_SideMode;

/* Side order in the arrays below. */
enum { SMI_TOP = 0, SMI_BOTTOM = 1, SMI_LEFT = 2, SMI_RIGHT = 3 };

/* One Jacobi step of one tile, enqueued on `stream`.
 *   halo[SMI_TOP] / halo[SMI_BOTTOM]: y_local values of the row above / below
 *   halo[SMI_LEFT] / halo[SMI_RIGHT]: x_local values of the column left/right
 * (required, i.e. non-NULL, exactly for sides in SMI_SIDE_HALO mode).
 * send_left / send_right (nullable) receive the tile's new first / last
 * column, packed -- the fused equivalent of Write's tee into send_left /
 * send_right (stencil_smi.cl:201-224).  `in` and `out` must not overlap. */
int smi_stencil_step(const float *in, float *out, int x_local, int y_local,
                     const int mode[4], const float *const halo[4],
                     float *send_left, float *send_right, SMI_Stream stream);

/* smi_stencil_step, and additionally max-accumulates the bit pattern of
 * |out - in| over the cells this call writes into *resid_bits (device memory,
 * 4-byte aligned; the caller zeroes it; calls may accumulate into one word).
 * Each difference is one fp32 subtraction and fabs (subnormals kept); the
 * patterns of non-negative floats order like the floats and every NaN pattern
 * lies above +inf, so the word ends up holding max |out - in| exactly, or a
 * NaN if any difference is one.  Cells of SMI_SIDE_SKIP sides are not written
 * and do not contribute; copied (SMI_SIDE_COPY) cells contribute |c - c|.
 * Same loads, arithmetic and stores as smi_stencil_step: no extra pass. */
int smi_stencil_step_residual(const float *in, float *out, int x_local, int y_local,
                              const int mode[4], const float *const halo[4],
                              float *send_left, float *send_right,
                              unsigned int *resid_bits, SMI_Stream stream);

/* Full run of the stencil_smi program on this rank's tile: `timesteps`
 * Jacobi steps over the PX x PY decomposition of `comm` (PX*PY == size),
 * halos exchanged every step with the four neighbours through RCCL on a
 * dedicated stream, overlapped with the interior sweep.  buf0 holds the
 * initial tile; buf1 is scratch of the same size.  On return *result_index
 * (0 or 1) names the buffer holding the final tile (like the reference's
 * half timesteps%2, stencil_smi.cpp:344; with fusion the index is
 * (K-step passes + pairs + remaining single steps) % 2).  Asynchronous w.r.t. the host
 * except for transport rendezvous and, with neighbours, the K-step passes'
 * pass-boundary join: before enqueueing interior(t) the host waits for the
 * band kernel of pass t-1 (it ends inside interior(t-1)), so the call returns
 * about one pass before the GPU finishes.  With neighbours the interior runs
 * on `stream` if that is at the highest stream priority, else on a
 * highest-priority stream of the communicator joined to `stream` at the start
 * and end of the call (a normal-priority stream can share a hardware queue
 * with RCCL's streams).  Results are identical either way. */
int smi_stencil_run(SMI_Comm comm, float *buf0, float *buf1, int x_local,
                    int y_local, int px, int py, int timesteps,
                    SMI_Stream stream, int *result_index);

/* smi_stencil_run for timesteps >= 1 that also returns the residual of its
 * final step: the bit pattern of max |x_T - x_{T-1}| over this rank's tile is
 * max-accumulated into *resid_bits (device memory, 4-byte aligned; the caller
 * zeroes it; calls may accumulate into one word) -- the contract of
 * smi_stencil_step_residual (one fp32 subtraction and fabs per cell,
 * subnormals kept, a NaN if any difference is one, copied global-edge cells
 * contribute |c - c|), taken inside the last pass of the run: no extra load,
 * no extra pass, no extra exchange and no host synchronisation beyond the
 * run's own.  The residual is rank-local: the function does no reduce (a
 * caller with its own convergence loop reduces the words of its ranks as it
 * sees fit; smi_stencil_solve does so with an integer-max smi_allreduce).  The word
 * is complete when the work enqueued on `stream` has finished.
 * Schedule (smi_stencil_plan_residual): the last launch is one pass of
 * K_r = min(steps_per_pass, 12, timesteps) steps, K_r clipped like every
 * K-step pass of smi_stencil_run on this tile (half the smaller tile side in
 * a multi-rank run, ...); the timesteps - K_r steps before it are planned
 * exactly as smi_stencil_run plans that many.  If K_r < 3 (steps_per_pass 1
 * or 2, fewer than 3 steps, tiles that run single steps only) the last launch
 * is one single residual step after timesteps - 1 planned steps.  In a
 * multi-rank run the last pass is an ordinary K_r-step pass (depth-K_r
 * exchange, band kernel, interior sweep) whose two kernels both post into the
 * word; every cell of the tile is counted by exactly the kernel that stores it.
 * The grid is bit-identical to smi_stencil_run(timesteps); *result_index
 * follows the launch count of this schedule and may differ from
 * smi_stencil_run's. */
int smi_stencil_run_residual(SMI_Comm comm, float *buf0, float *buf1, int x_local, int y_local,
                             int px, int py, int timesteps, unsigned int *resid_bits,
                             SMI_Stream stream, int *result_index);

/* Jacobi steps until the residual of a checked step is <= tol, or max_steps.
 * The residual of step t is r_t = max over the global grid of
 * |x_t - x_{t-1}| (the contract of smi_stencil_step_residual: exact, no
 * summation order; NaN if any difference is NaN).  Check points are
 * t_j = min(j * check_every, max_steps), j = 1, 2, ...: the steps between two
 * check points run as smi_stencil_run runs that many steps (same plan under
 * the current fusion setting), step t_j itself is one single step with the
 * residual fused into its kernels.  The local bit pattern then goes through
 * one integer-max smi_allreduce (include/smi/allreduce.h), so every rank sees
 * the same r_t and stops at the same step: the first check point with
 * r_t <= tol (a NaN never satisfies it), or max_steps -- which still returns
 * SMI_SUCCESS, with *converged = 0.
 *   *steps_done   steps taken
 *   *residual     the last r_t checked (+inf if max_steps == 0)
 *   *converged    (nullable) residual <= tol
 *   *result_index the buffer holding x_{steps_done}; it is bit-identical to
 *                 smi_stencil_run(timesteps = steps_done) from the same start
 * tol >= 0 and not NaN, max_steps >= 0, check_every >= 1; tile rules as for
 * smi_stencil_run.  Collective: every rank of `comm` calls it with the same
 * tol, max_steps and check_every; it issues bulk operations on `comm`.
 * SYNCHRONOUS with the host at every check point: 4 bytes are copied back
 * and `stream` is synchronised there, so a check costs one single step (8
 * B/cell where the fused passes move 8 B/cell per up to 20 steps), the
 * reduce + bcast and a host round trip; choose check_every so that this is
 * small beside the steps in between. */
int smi_stencil_solve(SMI_Comm comm, float *buf0, float *buf1, int x_local, int y_local,
                      int px, int py, float tol, int max_steps, int check_every,
                      SMI_Stream stream, int *result_index, int *steps_done,
                      float *residual, int *converged);

/* ---- Jacobi with a source term: -laplace(u) = f, with g = h^2 f ------------
 * Arithmetic contract (bit-exact):
 *   interior cell:     out = 0.25f * ((((S + W) + E) + N) + g)
 *   global-edge cell:  out = in        (g is ignored there)
 * S, W, E, N as above, g the cell of the caller's array `src`; IEEE fp32 round
 * to nearest, no contraction, subnormals kept; g is added last, after N and
 * before the multiply.  `src` has the tile's shape and layout (x_local x
 * y_local fp32, dense, row-major, 16-byte aligned), overlaps neither buffer
 * and is never written.  Its cells on the global edge may be read but never
 * reach a result: a NaN there does not leak.  The residual contract is that of
 * smi_stencil_step_residual, unchanged.
 *   g = -0.0f everywhere makes the update bit-identical to the plain one for
 * every input, because x + (-0) = x, including x = -0.  g = +0.0f does not,
 * because -0 + +0 = +0: cells whose four-neighbour sum is -0 come out +0.
 * A NULL, misaligned or overlapping `src` is an argument error like a bad
 * buf0 / buf1, refused before any device call. */

/* smi_stencil_step with the source term (all three side modes, send_left /
 * send_right); resid_bits nullable: non-NULL also takes the residual as
 * smi_stencil_step_residual does.  One more 16-byte load of `src` per four
 * cells and one more add per cell: 12 B/cell where the plain step moves 8. */
int smi_stencil_step_source(const float *in, float *out, const float *src, int x_local, int y_local,
                            const int mode[4], const float *const halo[4], float *send_left,
                            float *send_right, unsigned int *resid_bits /* nullable */, SMI_Stream stream);

/* smi_stencil_run with the source term; each rank passes its own tile of
 * `src`.  Schedule (smi_stencil_plan_source).  One tile with y_local >= 8:
 * fused passes of min(steps_per_pass, KS) steps, KS =
 * smi_stencil_source_max_depth, with the balanced-remainder rule of
 * smi_stencil_run (a remainder >= 3 is spread over the passes); a remainder of
 * 1 or 2 runs as single steps (no pairs), and steps_per_pass < 3 runs single
 * steps only.  Multi-rank, by default: single steps only, through the depth-1
 * exchange of smi_stencil_run.  With smi_stencil_set_source_bands(1): K-step
 * passes like smi_stencil_run's, K = min(steps_per_pass, KS) clipped to what
 * the tile holds (2K rows, 8 ceil(K/4) columns), the same remainder rules, the
 * halo-facing bands by a band kernel that adds g; the depth-K halos of `src`
 * are exchanged once per K-phase (at most twice per call) and are not kept
 * across calls.  A fused source pass moves 12 B/cell per up to KS steps and
 * runs the exact arithmetic at every level. */
int smi_stencil_run_source(SMI_Comm comm, float *buf0, float *buf1, const float *src, int x_local,
                           int y_local, int px, int py, int timesteps, SMI_Stream stream, int *result_index);

/* The loop of smi_stencil_solve with the source term: source runs between the
 * check points (fused across ranks too under smi_stencil_set_source_bands(1))
 * and one single source residual step at each, the same integer-max reduce and
 * bcast (the fused source pass has no residual variant, and
 * smi_stencil_set_solve_check does not affect this function). */
int smi_stencil_solve_source(SMI_Comm comm, float *buf0, float *buf1, const float *src, int x_local,
                             int y_local, int px, int py, float tol, int max_steps, int check_every,
                             SMI_Stream stream, int *result_index, int *steps_done, float *residual,
                             int *converged);

/* Multi-rank source runs.  0 (default): single steps.  1: K-step passes, K = min(steps_per_pass,
 * KS) clipped like smi_stencil_run clips K on this tile; g's depth-K halos are exchanged once per
 * K-phase.  Bit-identical grids for both settings.  fused = -1 keeps the setting. */
int smi_stencil_set_source_bands(int fused);
int smi_stencil_get_source_bands(int *fused);

/* The deepest fused source pass, KS (6..12): the largest K whose sweep keeps
 * its level rings and the K live rows of g in registers at two waves per SIMD
 * without scratch.  Host only. */
int smi_stencil_source_max_depth(int *k);

/* How smi_stencil_solve takes the residual at a check point.  0 (default): as
 * described above -- smi_stencil_run for the steps before the check point,
 * then one single residual step.  1: the steps up to each check point run as
 * one smi_stencil_run_residual, so the residual comes out of the last K-step
 * pass and the single step (8 B/cell for one step) is not run at all.
 * *steps_done, *residual, *converged and the grid are identical for both
 * settings; only *result_index and the time may differ (DESIGN.md section 7
 * has the measured cost of a check under both).  fused = -1 keeps the setting. */
int smi_stencil_set_solve_check(int fused);
int smi_stencil_get_solve_check(int *fused);

/* Tuning knobs of the sweep kernel (row-block height, rows in flight per
 * wave, non-temporal stores, 1 = overlap halo exchange with the interior).
 * Pass <= 0 / < 0 to keep a value.  Bit-exact results for every setting. */
int smi_stencil_set_tuning(int rows_per_wave, int rows_in_flight,
                           int nontemporal_stores, int overlap);
int smi_stencil_get_tuning(int *rows_per_wave, int *rows_in_flight,
                           int *nontemporal_stores, int *overlap);

/* Temporal blocking: steps_per_pass = K in 1..20 fuses up to K Jacobi steps
 * into one pass over HBM (same per-cell arithmetic, bit-identical result).
 * K = 13..20 runs the rotating-ring sweep, which needs a sweep rectangle
 * of at least 4K rows (the tile, or a multi-rank interior: the tile minus K
 * rows per side with a neighbour); K is clipped to 12 otherwise.
 * Multi-rank runs then exchange depth-K halos -- K rows / KC = 4 ceil(K/4)
 * columns per side neighbour and a K x KC corner block per diagonal
 * neighbour -- once per K steps; a band kernel computes the halo-facing bands
 * (K rows / KC columns deep) while the interior sweep runs.  A run is planned as K-step passes;
 * a remainder r = timesteps % K >= 3 is spread over ceil(timesteps / K)
 * passes balanced to within one step (20 = 10 + 10), r = 1 or 2 adds a pair
 * and/or a single step (smi_stencil_plan).  In a multi-rank run K is
 * clipped to half the smaller tile side; tiles smaller than 4 x 8 run single
 * steps only.
 * rows_per_wave: rows per wave of the active fused kernel (K >= 3: -1 =
 * automatic, one round of resident waves); rows_in_flight (1, 2, 4 or 8)
 * tunes the two-step kernel and is ignored for K >= 3.  Pass 0 to keep. */
int smi_stencil_set_fusion(int steps_per_pass, int rows_per_wave, int rows_in_flight);
int smi_stencil_get_fusion(int *steps_per_pass, int *rows_per_wave, int *rows_in_flight);

/* Multi-rank K-step passes: the interior sweep runs beside the band kernel
 * (the halo-facing bands, on the comm stream) and the exchange.
 * reserve_waves = wave slots the interior sweep leaves free for them, and
 * the band kernel then runs as that many waves looping over its segments
 * (0 = none reserved: one band wave per segment, run in the interior's
 * tail), interior_rounds =
 * rounds of resident waves the interior sweep is cut into (default 1).  Pass
 * < 0 to keep.  Scheduling only: bit-identical results for every setting. */
int smi_stencil_set_bands(int reserve_waves, int interior_rounds);
int smi_stencil_get_bands(int *reserve_waves, int *interior_rounds);

/* Multi-rank K-step passes with K >= 13 (scheduling only, bit-neutral): the
 * kernel that computes the halo-facing bands.  1 (default) = the lean kernel
 * (<= 64 VGPRs, one workgroup per CU, its levels staged through LDS) that
 * runs beside the interior sweep; 0 = one wave per band segment, which only
 * finds wave slots in the interior's tail.  lean = -1 keeps the setting. */
int smi_stencil_set_band_kernel(int lean);
int smi_stencil_get_band_kernel(int *lean);

/* Multi-rank K-step passes (scheduling only, bit-neutral): how interior(t)
 * is ordered after the band kernel of pass t-1.  1 (default) = on the host:
 * smi_stencil_run waits for band(t-1) to finish (it ends inside
 * interior(t-1)) and then enqueues interior(t) with no wait packet between
 * two interiors (~5 us per pass less than a device-side wait); the host is
 * then about one pass ahead of the GPU, so a host thread held up for longer
 * than one pass (~150 us at 8192^2, K = 20) idles the GPU for the excess.
 * 0 = on the device: a stream wait per pass; the host enqueues the whole
 * run without waiting and absorbs host stalls of any length behind the
 * queued passes, at ~3 % more GPU time per pass.
 * host_join = -1 keeps the setting. */
int smi_stencil_set_join(int host_join);
int smi_stencil_get_join(int *host_join);

/* The rotating-ring sweep (K = 13..20) launches one round of waves whose
 * row blocks are shortened where a wave has more work per row: ce16 / rev16
 * = the extra work of a wave holding a global-edge column / of the
 * upward-walking bottom block, in 16ths of a plain wave's; waves = the
 * launch's waves (0 = every resident wave slot).  Pass < 0 to keep.
 * Scheduling only: bit-identical results for every setting. */
int smi_stencil_set_deep(int ce16, int rev16, int waves);
int smi_stencil_get_deep(int *ce16, int *rev16, int *waves);

/* The rotating-ring sweep's work split for one K-step pass (K = 13..20) of a
 * rows x cols tile whose sides with a neighbour are set in side_mask (bit 0
 * top, 1 bottom, 2 left, 3 right; the sweep then covers the tile minus K rows
 * / KC columns there, as in smi_stencil_run): waves launched, column strips,
 * row blocks per interior strip and per edge-column strip, and the output
 * rows of the shortest block (every block must exceed K).  Host only; with
 * no device, set the launch's waves first (smi_stencil_set_deep). */
int smi_stencil_deep_geometry(int rows, int cols, int K, int side_mask, int *waves, int *strips, int *row_blocks,
                              int *row_blocks_edge, int *min_block_rows);

/* One phase of a planned run: `passes` launches of `steps_per_pass` steps. */
typedef struct {
    int steps_per_pass;
    int passes;
} SMI_StencilPhase;

/* The schedule smi_stencil_run follows on `rank` of a px x py decomposition
 * of x_local x y_local tiles under the current fusion setting, computed on
 * the host (no device needed): the phases in order (4 always suffice), the
 * neighbour ranks top, bottom, left, right, top-left, top-right,
 * bottom-left, bottom-right (-1 on the global edge; nullable; the rank map
 * of stencil_smi.cpp:133-134) and the index of the buffer that will hold
 * the result (nullable). */
int smi_stencil_plan(int x_local, int y_local, int px, int py, int rank, int timesteps,
                     SMI_StencilPhase *phases, int max_phases, int *nphases, int neighbours[8],
                     int *result_index);

/* The schedule smi_stencil_run_residual follows (timesteps >= 1), same
 * arguments and outputs: the phases smi_stencil_plan gives for the steps
 * before the final pass, then the final residual pass as a last phase of its
 * own, (K_r, 1) or (1, 1).  smi_stencil_plan yields at most 3 phases (two
 * balanced depths, or K-step passes + a pair + a single step), so 4 still
 * always suffice. */
int smi_stencil_plan_residual(int x_local, int y_local, int px, int py, int rank, int timesteps,
                              SMI_StencilPhase *phases, int max_phases, int *nphases,
                              int neighbours[8], int *result_index);

/* The schedule smi_stencil_run_source follows, same arguments and outputs: at
 * most 2 phases, none with steps_per_pass == 2 or > KS.  A multi-rank plan
 * follows smi_stencil_set_source_bands: [(1, timesteps)] at 0. */
int smi_stencil_plan_source(int x_local, int y_local, int px, int py, int rank, int timesteps,
                            SMI_StencilPhase *phases, int max_phases, int *nphases, int neighbours[8],
                            int *result_index);

#ifdef __cplusplus
}
#endif
#endif /* SMI_STENCIL_H */
