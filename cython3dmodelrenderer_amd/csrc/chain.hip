// chain.hip — the swap chain's shared slot (include/crender_chain.h): one slot of a crender_pipeline runs on a
// stream the caller owns, so that a chain of 4 needs three streams of its own and fits, with the caller's, the
// HIP runtime's default of four hardware queues.  Host code only: the pipeline's streams are plain members of
// the handle (plan.h), and everything that launches reads them from there, so handing a slot another stream is
// all it takes.
//
// abi.hip knows nothing of this.  Its entry points, read against a slot whose s[k] is the caller's stream:
//   crender_pipeline_frame    The first frame after a join (or with new inputs) records `mark` on the caller and
//                             makes EVERY slot wait for it, the shared slot included: a stream waiting for an event
//                             recorded on itself waits for work that is ahead of it anyway.  Frames of the shared
//                             slot are launched on the caller's stream like any other work of the caller's.
//                             The optional timing events of that slot land on the caller's stream: they time
//                             the same launches.
//   crender_pipeline_join     records done[k] on the caller's own stream and makes the caller wait for it: again
//                             a wait for work already ahead on that stream.  A join from ANOTHER stream than the
//                             shared one orders that stream behind the shared slot's frames, as it should.
//   crender_pipeline_timing_end   synchronises s[k]: the caller's stream, with the frames on it.
//   crender_pipeline_destroy  synchronises and DESTROYS s[k].  It must never see a borrowed stream:
//                             crender_pipeline_unshare first (a NULL s[k], the default stream, it skips).
// A shared default stream is s[k] == NULL, which every HIP call above takes as the default stream.
//
// Which slots of which pipelines are borrowed is kept here, keyed by handle, with the borrowed stream beside it:
// a record counts only while s[k] still IS that stream, so a record left behind by a pipeline destroyed without
// crender_pipeline_unshare says nothing about a later pipeline at the same address (whose s[k] are new streams).
#include <mutex>
#include <unordered_map>

#include "common.h"
#include "plan.h"
#include "../../include/crender_chain.h"

using namespace crender_detail;

namespace {

struct Borrowed {
    bool on[kMaxPipelineDepth] = {};
    hipStream_t st[kMaxPipelineDepth] = {};
};
std::mutex g_lock;
std::unordered_map<const crender_pipeline *, Borrowed> g_borrowed;

// (with g_lock held)
bool is_borrowed(const crender_pipeline *p, const Borrowed &b, int k) { return b.on[k] && p->s[k] == b.st[k]; }

int count_borrowed(const crender_pipeline *p, int *lowest)
{
    std::lock_guard<std::mutex> hold(g_lock);
    auto it = g_borrowed.find(p);
    int n = 0;
    if (lowest) *lowest = -1;
    if (it == g_borrowed.end()) return 0;
    for (int k = p->depth - 1; k >= 0; --k)
        if (is_borrowed(p, it->second, k)) { ++n; if (lowest) *lowest = k; }
    return n;
}

}  // namespace

extern "C" {

int crender_pipeline_share_stream(crender_pipeline *p, int slot, void *stream)
{
    if (!p) return fail(CRENDER_EINVAL, "crender_pipeline_share_stream: null pipeline");
    if (slot < 0 || slot >= p->depth) return fail(CRENDER_EINVAL, "crender_pipeline_share_stream: bad slot");
    if (p->n != 0) return fail(CRENDER_EINVAL, "crender_pipeline_share_stream: frames in flight (join first)");
    hipStream_t to = static_cast<hipStream_t>(stream);
    std::lock_guard<std::mutex> hold(g_lock);
    Borrowed &b = g_borrowed[p];
    if (is_borrowed(p, b, slot)) {
        if (to == b.st[slot]) return CRENDER_OK;
        // the slot's earlier frames (joined, but perhaps by another stream than `to`) stay ahead of its next ones
        CR_HIP(hipEventRecord(p->done[slot], b.st[slot]));
        CR_HIP(hipStreamWaitEvent(to, p->done[slot], 0));
    } else if (p->s[slot]) {
        CR_HIP(hipStreamSynchronize(p->s[slot]));
        CR_HIP(hipStreamDestroy(p->s[slot]));
    }
    p->s[slot] = to;
    b.on[slot] = true;
    b.st[slot] = to;
    return CRENDER_OK;
}

int crender_pipeline_unshare(crender_pipeline *p)
{
    if (!p) return fail(CRENDER_EINVAL, "crender_pipeline_unshare: null pipeline");
    std::lock_guard<std::mutex> hold(g_lock);
    auto it = g_borrowed.find(p);
    if (it == g_borrowed.end()) return CRENDER_OK;
    const Borrowed b = it->second;
    g_borrowed.erase(it);
    int rc = CRENDER_OK;
    for (int k = 0; k < p->depth; ++k) {
        if (!is_borrowed(p, b, k)) continue;
        hipStream_t own = nullptr;
        hipError_t e = hipStreamCreateWithFlags(&own, hipStreamNonBlocking);
        if (e == hipSuccess) e = hipEventRecord(p->done[k], b.st[k]);
        if (e == hipSuccess) e = hipStreamWaitEvent(own, p->done[k], 0);
        if (e != hipSuccess) {
            // no stream to hand the slot over to: wait its frames out here, and leave destroy nothing to touch
            (void)hipStreamSynchronize(b.st[k]);
            if (own) (void)hipStreamDestroy(own);
            own = nullptr;
            rc = fail_hip(e, "crender_pipeline_unshare");
        }
        p->s[k] = own;
    }
    return rc;
}

int crender_pipeline_shared_slot(const crender_pipeline *p)
{
    if (!p) return -1;
    int lowest = -1;
    (void)count_borrowed(p, &lowest);
    return lowest;
}

int crender_pipeline_owned_streams(const crender_pipeline *p)
{
    if (!p) return -1;
    return p->depth - count_borrowed(p, nullptr);
}

}  // extern "C"
