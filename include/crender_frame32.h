/*
 * crender_frame32.h — C ABI of the swap chain's frame kernel for small scenes on 32-pixel tiles (csrc/frame32.hip).
 * Same conventions as crender_hip.h, whose version number (CRENDER_ABI_VERSION) covers this header too: an int
 * status (CRENDER_OK or a CRENDER_E* code, text in crender_last_error()), nothing synchronised.
 *
 * What.  A look-ahead frame of a crender_pipeline (crender_pipeline_set_lookahead) is ONE launch: the frame's raster
 * pass and the binning wavefronts of the slot's next frame.  The library's general frame kernel carries every path
 * a 32-pixel plan can take.  The frames a chain renders of a small scene take one of them: direct bins, the fused
 * clear, no winner plane, no fused light, no triangle order, lists of small records swept run-wise.  This unit is
 * a kernel with that one path, launched in the general kernel's place when — and only when — a frame qualifies.
 * Its stores: where the three planes begin on 16-byte boundaries and the width is a multiple of 4, every tile of
 * full width — empty or covered — is stored as whole rows in 16-byte write-through stores; a tile cut at the right
 * edge, and every tile of a frame without such rows, is stored pixel by pixel.  The planes hold the same words
 * either way, and nothing outside the frame's rows is ever written.
 *
 * Contract.
 *   Results     Bit-identical planes: every sample goes through the same device functions (raster_math.h), the
 *               depth keys keep the triangle index in the compared bits, so the tie rule is the general kernel's.
 *   Plans       The plans are shared with the general kernels and a chain may alternate between the two from frame
 *               to frame: the kernel leaves every cross-frame word of a plan (the other parity's counters, the
 *               heavy tiles' flags and helper slots, the statistics, the usage record) exactly as the general
 *               kernel does, and crender_plan_debug_check holds after every frame.
 *   Eligibility A frame takes the kernel when its pipeline slot looks ahead and the plan has 32-pixel tiles and
 *               direct bins; the flags have CRENDER_FUSED_CLEAR and CRENDER_OVERLAPPED_FRAMES and not
 *               CRENDER_FUSED_GURO; no winner plane, triangle order or normal-z array is set; no raster path is
 *               forced (crender_plan_set_raster_path, crender_set_default_raster_path) and the plan's own choice
 *               is the general kernel; the frame's byte offsets fit 32 bits.  Every other frame is rendered by
 *               crender_pipeline_submit's code, unchanged.
 *   Threads     Like the rest of a pipeline's calls: one thread at a time per pipeline.
 */
#ifndef CRENDER_FRAME32_H
#define CRENDER_FRAME32_H

#include "crender_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* crender_pipeline_submit with the small-scene kernel where the frame qualifies: the next frame of the pipeline
 * from the arguments bound to its slot (crender_pipeline_bind), `stream` the caller's stream.  Same errors. */
CRENDER_API int crender_frame32_submit(crender_pipeline *p, void *stream);

/* 1 if the pipeline's last frame submitted through crender_frame32_submit took the small-scene kernel, 0 if it
 * was rendered by the general code (or none was submitted, or for NULL). */
CRENDER_API int crender_frame32_last(const crender_pipeline *p);

#ifdef __cplusplus
}
#endif
#endif /* CRENDER_FRAME32_H */
