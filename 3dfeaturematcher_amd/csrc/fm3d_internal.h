// fm3d_internal.h -- entry points shared by the library's own translation units (not the C ABI).
#pragma once

#include <hip/hip_runtime.h>

#include "fm3d.h"

// stage one frame pair (queryOffset 0) and queue the whole path with the survivor records compacted
// into recordsDev (device, capacity nA); returns without waiting (the context is then pending).  As
// fm3d_pipeline_submit for linked contexts: a member queues its front half only
int fm3d_internal_submit_to(fm3d_ctx* c, const void* descA, int nA, const void* descB, int nB, int dim, int type,
                            const fm3d_point2f* kpts1, const fm3d_point2f* kpts2, const uint8_t* img1,
                            const uint8_t* img2, int width, int height, fm3d_record* recordsDev);
// a link member's submitted pair whose leader has not launched it: its LM alone + records, queued
int fm3d_internal_flush(fm3d_ctx* c);
bool fm3d_internal_front_only(const fm3d_ctx* c);
// queue the whole path on the inputs fm3d_pipeline_upload staged
int fm3d_internal_enqueue(fm3d_ctx* c, fm3d_record* recordsDev);
// wait for the pending run: counts, guards, stats
int fm3d_internal_finish(fm3d_ctx* c, int* nKept, fm3d_pipeline_stats* stats);
// the survivor count of the queued run on the device (valid in stream order after the run)
const int* fm3d_internal_kept_dev(fm3d_ctx* c);
hipStream_t fm3d_internal_stream(fm3d_ctx* c);
int fm3d_internal_prepare(fm3d_ctx* c);
// the device memory one context of this settings may grow to for a frame pair of nA x nB rows:
// its LM slabs (the largest launch) + a conservative estimate of the per-pair buffers
int fm3d_internal_memory_need(fm3d_ctx* c, int64_t nA, int64_t nB, int dim, int type, int width, int height,
                              size_t* bytes);
// Test probe of FM3D_DEBUG_POISON (tests/test_gpu_poison.py; C linkage, so that ctypes finds it): a
// fresh local DevBuf of `bytes` bytes (> 0), ensured and copied back to out with nothing written
extern "C" int fm3d_internal_alloc_probe(fm3d_ctx* c, size_t bytes, uint8_t* out);
// Test accessors of the LM's image-2 layout (tests/test_gpu_lm_img2_layout.py; C linkage).
// The column-major copy of image 2's pyramid level with its guard: *w, *h the level's size, *hs the
// column stride, *bytes = (w + 2) hs + the guard past the last column; out (may be null) takes them
extern "C" int fm3d_internal_level_cols(fm3d_ctx* c, int level, uint8_t* out, int* w, int* h, int* hs,
                                        size_t* bytes);
// the layout the context's last LM launch read image 2 in: 1 columns, 0 rows, -1 no launch yet
extern "C" int fm3d_internal_lm_img2_cols(const fm3d_ctx* c);
