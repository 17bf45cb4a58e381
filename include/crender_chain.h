/*
 * crender_chain.h — C ABI of the swap chain's shared slot: one slot of a crender_pipeline (crender_hip.h) runs
 * its frames on a stream the CALLER owns instead of a stream of the pipeline's own.  Same conventions as
 * crender_hip.h, whose version number (CRENDER_ABI_VERSION) covers this header too: an int status (CRENDER_OK or
 * a CRENDER_E* code, text in crender_last_error()), nothing synchronised unless said.  Host code only: no kernel.
 *
 * Why.  A chain of `depth` overlaps its frames on `depth` streams, and the stream of the caller (where the inputs
 * are produced and the results consumed) is one more.  The HIP runtime maps a process's streams onto
 * GPU_MAX_HW_QUEUES hardware queues, 4 unless the environment says otherwise before the runtime starts; two
 * streams on one queue run one after the other.  A chain of 4 with four streams of its own therefore needs five
 * queues.  The caller's stream is idle while a burst of frames is submitted, so the chain's last slot can run
 * there: three streams of the chain's own and the caller's, four frames in flight on four queues.
 *
 * Contract.
 *   Ownership   The shared stream belongs to the caller.  It must stay alive from crender_pipeline_share_stream
 *               until the slot is shared with another stream or crender_pipeline_unshare returns.  The pipeline
 *               never synchronises or destroys it.
 *   Ordering    Frames of the shared slot are ordinary work on that stream: they run behind whatever the caller
 *               enqueued there before, and whatever the caller enqueues there later runs behind them.  Frames of
 *               the other slots are ordered exactly as before.  crender_pipeline_join still orders the joining
 *               stream behind ALL frames in flight, the shared slot's included.
 *   Results     Bit-identical to the chain with streams of its own: no kernel, no launch argument and no plan
 *               changes, only the queue one slot's launches are put on.
 *   Destroy     crender_pipeline_destroy synchronises and destroys every stream it finds in the pipeline: call
 *               crender_pipeline_unshare first.  After it the pipeline owns all of its streams again.
 *   NULL        A NULL stream is the LEGACY default stream (torch's default stream is it).  Work on it synchronises
 *               implicitly with every BLOCKING stream of the process (hipStreamCreate, or flags without
 *               hipStreamNonBlocking): the shared slot's frames then wait for such streams' earlier work and hold
 *               back their later work, which the chain's own non-blocking streams never do.  Results do not
 *               change; an application that owns blocking streams and wants them to overlap with the frames
 *               shares a non-blocking stream of its own instead, or none.
 *   Device      Call these with the pipeline's device current, as for crender_pipeline_create.
 *   Threads     Like the rest of a pipeline's calls: one thread at a time per pipeline.
 */
#ifndef CRENDER_CHAIN_H
#define CRENDER_CHAIN_H

#include "crender_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Slot `slot` (0 .. depth - 1) runs its frames on `stream` from now on.  A NULL `stream` is the default stream
 * of the current device.  Allowed only with no frame in flight (before the first frame, or after
 * crender_pipeline_join): CRENDER_EINVAL otherwise, and for a NULL pipeline or a slot outside the chain.
 * The slot's own stream is synchronised (it is idle: its frames were joined) and destroyed, which gives its
 * hardware queue back to the runtime.  Sharing a slot that is already shared replaces the stream; the new one is
 * ordered behind the old one with an event, and the old one is the caller's again when the call returns. */
CRENDER_API int crender_pipeline_share_stream(crender_pipeline *p, int slot, void *stream);

/* Every shared slot gets a fresh non-blocking stream of its own, ordered behind the stream it shared (an event;
 * no host synchronisation) — frames in flight there are waited for by crender_pipeline_destroy like any others.
 * Nothing to do, and CRENDER_OK, for a pipeline that shares nothing.  CRENDER_EINVAL for a NULL pipeline.  Should
 * the runtime refuse a new stream, the shared one is synchronised and the slot is left without a stream (destroy
 * skips it): CRENDER_EHIP. */
CRENDER_API int crender_pipeline_unshare(crender_pipeline *p);

/* The lowest shared slot, or -1 (also for NULL). */
CRENDER_API int crender_pipeline_shared_slot(const crender_pipeline *p);

/* How many of its `depth` streams the pipeline owns: depth minus the shared slots (-1 for NULL). */
CRENDER_API int crender_pipeline_owned_streams(const crender_pipeline *p);

#ifdef __cplusplus
}
#endif
#endif /* CRENDER_CHAIN_H */
