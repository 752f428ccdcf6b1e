/*
 * kmeans.h -- the kmeans_smi consumer of SMI_Reduce / SMI_Bcast.
 *
 * Replaces the three kernels of examples/kernels/kmeans_smi.cl and the
 * device part of examples/host/kmeans_smi.cpp (ryutakashino/SMI):
 *   SendCentroids    kmeans_smi.cl:14-34    centroids of iteration i: the
 *                                            initial ones, then the updated ones
 *   ComputeDistance  kmeans_smi.cl:36-88    per point and cluster k a squared
 *                                            distance; the first k with the
 *                                            strictly smallest one wins
 *   ComputeMeans     kmeans_smi.cl:90-209   per-cluster sums and counts,
 *                                            SMI_Reduce to rank 0 (fp32 add on
 *                                            port 0, int add on port 2),
 *                                            SMI_Bcast (ports 1, 3), divide
 *
 * Arithmetic contract (the reference's semantics, quirks included):
 *   - distance: points are read as `width`-wide vectors (W, VTYPE in
 *     examples/include/kmeans.h.in; 16 in the reference build,
 *     examples/CMakeLists.txt:5) and the inner loop ASSIGNS the squared
 *     difference instead of adding it (kmeans_smi.cl:68-71), so only the
 *     last lane of every vector counts:
 *       dist_k = ((0 + d_{W-1}^2) + d_{2W-1}^2) + ...   (fp32, mul then add)
 *     width = 1 is the plain squared Euclidean distance.
 *   - assignment: min starts at +inf and cluster k replaces it only if
 *     dist_k < min (kmeans_smi.cl:75-83): ties keep the lower k, NaN never
 *     wins, a point whose distances are all NaN / +inf goes to cluster 0.
 *   - sums: per cluster and dimension, this rank's points in point order,
 *     fp32 adds from +0 (kmeans_smi.cl:113-127); counts exact.  Assignments
 *     outside [0, clusters) belong to no cluster (`index == k` never holds).
 *   - across ranks: the fold of reduce.h (canonical rank order), then
 *     centroid = sum / (float)count with IEEE division (kmeans_smi.cl:200);
 *     an empty cluster becomes 0/0 = NaN, as in the reference.
 */
#ifndef SMI_KMEANS_H
#define SMI_KMEANS_H

#include "communicator.h"

#ifdef __cplusplus
extern "C" {
#endif

/* ComputeDistance on n points (row-major n x dims, device memory):
 * assignment[p] = cluster of point p under `centroids` (clusters x dims).
 * dims must be a multiple of width, 1 <= clusters <= 256 and
 * clusters * dims / width <= 16384. */
int smi_kmeans_assign(const float *points, int n, int dims, const float *centroids, int clusters,
                      int width, int *assignment, SMI_Stream stream);

/* The accumulation half of ComputeMeans on one rank: sums (clusters x dims)
 * and counts (clusters) of the points assigned to each cluster, in point
 * order.  Scratch is stream-ordered device memory. */
int smi_kmeans_accumulate(const float *points, int n, int dims, const int *assignment, int clusters,
                          float *sums, int *counts, SMI_Stream stream);

/* The whole kmeans_smi program on this rank's n_local points: `iterations`
 * rounds of assign, accumulate, SMI_Reduce to rank 0, SMI_Bcast and divide.
 * `centroids` (clusters x dims, device) holds the initial centroids on entry
 * -- the same on every rank, as after the host's MPI_Bcast
 * (kmeans_smi.cpp:164) -- and the final ones on return, on every rank.  All
 * work is enqueued on `stream`; the call does not synchronise the host. */
int smi_kmeans(SMI_Comm comm, const float *points, int n_local, int dims, int clusters, int width,
               float *centroids, int iterations, SMI_Stream stream);

/* The cross-rank half of ComputeMeans in one kernel: row r of `sums`
 * (clusters*dims floats, row pitch `ld_sums` elements) and row r of `counts`
 * (clusters ints, row pitch `ld_counts` elements) are rank r's contribution,
 * 1 <= nranks <= 64.  centroids[k][d] = fold(sums column) /
 * (float)fold(counts column): both folds are the rank-order SMI_ADD fold of
 * reduce.h (4 slots for the floats, 1 for the ints, which wrap), the division
 * is IEEE.  An empty cluster gives 0/0 = NaN; a -0 sum becomes +0 through the
 * fold's +0 start.  The bits are those of smi_reduce_fold on the sums, on the
 * counts, and the divide of smi_kmeans. */
int smi_kmeans_means(const float *sums, const int *counts, int nranks, size_t ld_sums,
                     size_t ld_counts, int clusters, int dims, float *centroids, SMI_Stream stream);

/* How smi_kmeans brings the sums and counts of all ranks together.
 * 0 (default): the reference's four collectives (reduce and bcast of the
 * sums, of the counts) and a divide.  1: one transfer group per iteration --
 * every rank sends its record (sums and counts, adjacent) to every other
 * rank -- and one smi_kmeans_means launch over the n records; a record above
 * 256 KiB takes two smi_allreduce calls and the divide instead.  The
 * centroids are bit-identical in both modes, on every rank.  fused = -1
 * keeps the setting.  Process-wide; the same value on every rank. */
int smi_kmeans_set_means(int fused);
int smi_kmeans_get_means(int *fused);

#ifdef __cplusplus
}
#endif
#endif /* SMI_KMEANS_H */
