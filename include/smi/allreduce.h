/*
 * allreduce.h -- the reduce of reduce.h with the result on every rank.
 *
 * The reference has no such call: its kmeans_smi pairs SMI_Reduce to rank 0
 * with SMI_Bcast (examples/kernels/kmeans_smi.cl:132-192) and calls the pair
 * an allreduce.  On a fully connected node the pair costs two transfer
 * rounds through the root's links and one fold on the root while the other
 * ranks wait; here every rank folds, and the rounds carry no root.
 *
 * Arithmetic contract: on every rank, every element of `recvbuf` holds
 * exactly the bits smi_reduce leaves in its root's `recvbuf` -- the
 * rank-order fold of reduce.h (S = 4 rotating slots for float/double, 1 for
 * the integer types; init 0 / *_MIN / *_MAX with the FLT_MIN / DBL_MIN start
 * of SMI_MAX; integer adds wrap).  All ranks therefore hold byte-identical
 * results: a convergence decision taken from the result is the same on every
 * rank.  The result depends on neither the path taken nor the piece size.
 */
#ifndef SMI_ALLREDUCE_H
#define SMI_ALLREDUCE_H

#include <stddef.h>
#include "communicator.h"
#include "data_types.h"
#include "reduce.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Reduce `count` elements of every rank's device buffer `sendbuf` into every
 * rank's device buffer `recvbuf`, enqueued on `stream`.  `sendbuf == recvbuf`
 * (in place) is allowed; any other overlap of the two ranges is refused
 * (SMI_ERR_INVALID_ARG) before any device call.  `count == 0` returns
 * SMI_SUCCESS without communication.  Argument checks and status codes are
 * those of smi_reduce (unknown communicator, more than 64 ranks, bad op,
 * unsupported type, NULL buffers), buffer alignment rules too; `port` is
 * informational, as there.  Collective: matched with the other ranks' bulk
 * operations in issue order.  The host is not synchronised beyond what the
 * transport's rendezvous needs.
 * Schedule: messages up to 256 KiB take one transfer group in which every
 * rank sends its whole buffer to every other rank, then one rank-order fold
 * of the n rows on every rank -- one round and one kernel.  Larger messages
 * take smi_reduce's owner-chunk pipeline (pieces of smi_set_pipeline_bytes()
 * bytes) with its gather replaced by an all-gather of the folded pieces. */
int smi_allreduce(SMI_Comm comm, const void *sendbuf, void *recvbuf, size_t count,
                  SMI_Datatype type, SMI_Op op, int port, SMI_Stream stream);

#ifdef __cplusplus
}
#endif
#endif /* SMI_ALLREDUCE_H */
