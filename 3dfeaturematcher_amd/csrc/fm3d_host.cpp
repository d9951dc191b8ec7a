// fm3d_host.cpp -- C ABI (include/fm3d.h): context life cycle, staging, matcher routing, DLT, LM,
// the pipeline and the small one-off entry points.
//
// The heavy per-keypoint work runs in the HIP kernels of fm3d_match.hip, fm3d_misc.hip and
// fm3d_lm2.hip; the context-free host algebra is fm3d_algebra.cpp's, the detectors and extractors
// are fm3d_features.cpp's.  There is no CPU fallback: without a GPU every compute entry point
// fails with FM3D_ERR_HIP.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cfloat>
#include <climits>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "fm3d.h"
#include "fm3d_ctx.h"
#include "fm3d_kernels.h"

using fm3d::LevelDesc;

using namespace fm3d_host;

// (declared in fm3d_ctx.h: the detectors of fm3d_features.cpp compact with it too)
int fm3d_host::ensure_scan_tmp(fm3d_ctx* c, int n) {
    HIPCHK(c, c->scanTmp.ensure(fm3d::scan_tmp_bytes(n < 1 ? 1 : n)));
    HIPCHK(c, c->count.ensure(64));
    return FM3D_OK;
}

namespace {

void install_g12(fm3d_ctx* c, const double g[16]) {
    std::memcpy(c->g12, g, sizeof(c->g12));
    camera2_from_g12(c->g12, c->R2, c->t2);
    c->haveG12 = true;
    c->gateStaged = false;  // the staged pair's epipolar lines belong to the previous pose
}

bool good_max_px(double v) { return v > 0. && v <= DBL_MAX; }  // finite and > 0 (false for NaN)

// the gate's device inputs from keypoints already on the device (kp1: nA queries, kp2: nB train
// rows), queued on the context stream
int make_gate(fm3d_ctx* c, const fm3d_point2f* kp1, int nA, const fm3d_point2f* kp2, int nB, double maxPx,
              fm3d::EpiGate* g) {
    HIPCHK(c, c->gLines.ensure((size_t)nA * sizeof(float4) + 16));
    HIPCHK(c, c->gUV.ensure((size_t)nB * sizeof(float2) + 16));
    double E[9];
    epipolar_matrix(c->R2, c->t2, E);
    fm3d::launch_epipolar_setup(c->cam, E, kp1, nA, kp2, nB, c->gLines.as<float4>(), c->gUV.as<float2>(), c->stream);
    HIPCHK(c, hipGetLastError());
    g->lines = c->gLines.as<float4>();
    g->uv = c->gUV.as<float2>();
    g->tau = maxPx * 2.0 / (c->cam.fx + c->cam.fy);
    return FM3D_OK;
}

int ensure_offsets(fm3d_ctx* c) {
    if (c->nOff > 0) return FM3D_OK;
    const int R = c->s.pixelsRay;
    std::vector<int2> off;
    for (int i = -R; i <= R; i++)      // extractPixelsContour (:345-351): i outer (x), j inner (y)
        for (int j = -R; j <= R; j++)
            if (i * i + j * j <= R * R) off.push_back(make_int2(i, j));
    c->nOff = (int)off.size();
    // pad to a multiple of the LM kernel's 64-entry chunk with offsets that are never
    // inside the image
    while (off.size() % 64) off.push_back(make_int2(1 << 20, 1 << 20));
    c->nOffPad = (int)off.size();
    HIPCHK(c, c->offsets.ensure(off.size() * sizeof(int2)));
    HIPCHK(c, hipMemcpy(c->offsets.p, off.data(), off.size() * sizeof(int2), hipMemcpyHostToDevice));
    return FM3D_OK;
}

int upload(fm3d_ctx* c, DevBuf& b, const void* src, size_t bytes) {
    HIPCHK(c, b.ensure(bytes));
    if (bytes) HIPCHK(c, hipMemcpyAsync(b.p, src, bytes, hipMemcpyHostToDevice, c->stream));
    return FM3D_OK;
}

// The staging buffers are refilled only after the H2D copies of the previous call out of them
// have run (c->evStage, recorded after them on the context stream).
int staging_wait(fm3d_ctx* c) {
    HIPCHK(c, hipEventSynchronize(c->evStage));
    return FM3D_OK;
}

// bytes from a host array to a device buffer through the pinned staging buffer h: one memcpy, one
// DMA copy (1 MiB pieces issued as they were copied, and the memcpy split over host threads, were
// both slower on the C2 and C4 lines)
int upload_pinned(fm3d_ctx* c, DevBuf& dst, HostBuf& h, const void* src, size_t bytes) {
    HIPCHK(c, dst.ensure(bytes));
    if (!bytes) return FM3D_OK;
    HIPCHK(c, h.ensure(bytes));
    std::memcpy(h.p, src, bytes);
    HIPCHK(c, hipMemcpyAsync(dst.p, h.p, bytes, hipMemcpyHostToDevice, c->stream));
    return FM3D_OK;
}

// rows of bytes padded to dimPad (multiple of 128) with value 128 (x - 128 == 0: no effect on d2)
void pad_u8(uint8_t* o, const uint8_t* x, int n, int dim, int dimPad) {
    if (dim == dimPad) {
        std::memcpy(o, x, (size_t)n * dim);
        return;
    }
    for (int i = 0; i < n; i++) {
        std::memcpy(o + (size_t)i * dimPad, x + (size_t)i * dim, dim);
        std::memset(o + (size_t)i * dimPad + dim, 128, dimPad - dim);
    }
}
// stage descriptors on the device (asynchronous H2D from the pinned staging buffers; the stream
// orders every later use); returns the effective kernel type
// (waitStaging false: the caller waited for the staging buffers already, stage_pipeline)
int stage_descriptors(fm3d_ctx* c, const void* descA, int nA, const void* descB, int nB, int dim, int type,
                      int* effType, int* dimPad, bool waitStaging = true, bool speculate = false) {
    if (dim <= 0 || nA < 0 || nB < 0) return fail(c, FM3D_ERR_INVALID, "bad descriptor shape");
    int r;
    if (waitStaging && (r = staging_wait(c))) return r;
    c->specU8 = false;
    int t = type;
    if (type == FM3D_DESC_F32 && ((dim + 127) / 128) * 128 <= 256) {
        // float rows as the reference hands them to knnMatch (descriptorsmatcher.cpp:114-117): to the
        // device as they are; one kernel packs them into padded u8 rows and flags any element that is not
        // an integer in [0, 255].  Integer-valued rows (SIFT) take the u8 kernel -- exact, the same
        // ranking and distances as the float scan -- others the float kernels.  The choice of kernels
        // needs the flag: one host wait for this context's copies and the pack (the float path waits
        // on the device once more anyway, run_match)
        const int dp = ((dim + 127) / 128) * 128;
        int r2;
        if ((r2 = upload_pinned(c, c->A, c->hA, descA, (size_t)nA * dim * 4))) return r2;
        if ((r2 = upload_pinned(c, c->B, c->hB, descB, (size_t)nB * dim * 4))) return r2;
        HIPCHK(c, c->A8.ensure((size_t)nA * dp + 16));
        HIPCHK(c, c->B8.ensure((size_t)nB * dp + 16));
        HIPCHK(c, c->u8Flag.ensure(64));
        HIPCHK(c, c->hFlag.ensure(64));
        HIPCHK(c, hipMemsetAsync(c->u8Flag.p, 0, sizeof(int), c->stream));
        fm3d::launch_f32_pack_u8(c->A.as<float>(), nA, c->B.as<float>(), nB, dim, dp, c->A8.as<uint8_t>(),
                                 c->B8.as<uint8_t>(), c->u8Flag.as<int>(), c->stream);
        HIPCHK(c, hipGetLastError());
        *c->hFlag.as<int>() = -1;  // "not arrived" (the previous pair's copies into it have run: staging_wait)
        HIPCHK(c, hipMemcpyAsync(c->hFlag.p, c->u8Flag.p, sizeof(int), hipMemcpyDeviceToHost, c->stream));
        if (speculate) {
            // no host wait (fm3d_pipeline_submit_dlt_pair): the u8 matcher runs on the packed rows, and
            // the wait re-runs the front half on the float rows if the flag then says they were not
            // integers (redo_float_front)
            std::swap(c->A, c->A8);
            std::swap(c->B, c->B8);
            *dimPad = dp;
            *effType = FM3D_DESC_U8;
            c->specU8 = true;
            return FM3D_OK;
        }
        HIPCHK(c, hipEventRecord(c->evStage, c->stream));
        HIPCHK(c, hipEventSynchronize(c->evStage));
        if (*c->hFlag.as<int>() == 0) {
            std::swap(c->A, c->A8);  // the packed rows become the matcher's inputs
            std::swap(c->B, c->B8);
            *dimPad = dp;
            *effType = FM3D_DESC_U8;
        } else {
            *dimPad = dim;
            *effType = FM3D_DESC_F32;
        }
        return FM3D_OK;
    }
    if (t == FM3D_DESC_U8) {
        int dp = ((dim + 127) / 128) * 128;
        if (dp > 256) return fail(c, FM3D_ERR_UNSUPPORTED, "u8 descriptors longer than 256 bytes");
        const size_t ba = (size_t)nA * dp, bb = (size_t)nB * dp;
        if (dim == dp) {  // rows already padded (SIFT's 128 bytes): the copy overlapped with the DMA
            if ((r = upload_pinned(c, c->A, c->hA, descA, ba))) return r;
            if ((r = upload_pinned(c, c->B, c->hB, descB, bb))) return r;
        } else {
            HIPCHK(c, c->hA.ensure(ba + 1));
            HIPCHK(c, c->hB.ensure(bb + 1));
            pad_u8(c->hA.as<uint8_t>(), (const uint8_t*)descA, nA, dim, dp);
            pad_u8(c->hB.as<uint8_t>(), (const uint8_t*)descB, nB, dim, dp);
            HIPCHK(c, c->A.ensure(ba));
            HIPCHK(c, c->B.ensure(bb));
            if (ba) HIPCHK(c, hipMemcpyAsync(c->A.p, c->hA.p, ba, hipMemcpyHostToDevice, c->stream));
            if (bb) HIPCHK(c, hipMemcpyAsync(c->B.p, c->hB.p, bb, hipMemcpyHostToDevice, c->stream));
        }
        *dimPad = dp;
    } else if (t == FM3D_DESC_F32) {
        if ((r = upload_pinned(c, c->A, c->hA, descA, (size_t)nA * dim * 4))) return r;
        if ((r = upload_pinned(c, c->B, c->hB, descB, (size_t)nB * dim * 4))) return r;
        *dimPad = dim;
    } else if (t == FM3D_DESC_BITS) {
        int words = (dim + 3) / 4;
        int wp = (words == 4 || words == 8 || words == 16) ? words : 16;
        if (words > 16) return fail(c, FM3D_ERR_UNSUPPORTED, "binary descriptors longer than 64 bytes");
        const size_t ba = (size_t)nA * wp * 4, bb = (size_t)nB * wp * 4;
        HIPCHK(c, c->hA.ensure(ba + 1));
        HIPCHK(c, c->hB.ensure(bb + 1));
        std::memset(c->hA.p, 0, ba);
        std::memset(c->hB.p, 0, bb);
        for (int i = 0; i < nA; i++) std::memcpy(c->hA.as<uint8_t>() + (size_t)i * wp * 4, (const uint8_t*)descA + (size_t)i * dim, dim);
        for (int i = 0; i < nB; i++) std::memcpy(c->hB.as<uint8_t>() + (size_t)i * wp * 4, (const uint8_t*)descB + (size_t)i * dim, dim);
        HIPCHK(c, c->A.ensure(ba));
        HIPCHK(c, c->B.ensure(bb));
        if (ba) HIPCHK(c, hipMemcpyAsync(c->A.p, c->hA.p, ba, hipMemcpyHostToDevice, c->stream));
        if (bb) HIPCHK(c, hipMemcpyAsync(c->B.p, c->hB.p, bb, hipMemcpyHostToDevice, c->stream));
        *dimPad = wp * 4;
    } else {
        return fail(c, FM3D_ERR_INVALID, "unknown descriptor type");
    }
    HIPCHK(c, hipEventRecord(c->evStage, c->stream));
    *effType = t;
    return FM3D_OK;
}

// FM3D_BITS_MFMA=0 keeps 256-bit binary rows on the popcount kernel (A/B comparisons)
bool bits_mfma() {
    const char* e = getenv("FM3D_BITS_MFMA");
    return !(e && e[0] == '0');
}

// FM3D_F32_MFMA=0 keeps float rows on the exact VALU scan (A/B comparisons)
bool f32_mfma() {
    const char* e = getenv("FM3D_F32_MFMA");
    return !(e && e[0] == '0');
}

// knn2 + NNDR flags on staged descriptors (device), results in c->idx/key/fkey/cand/flag
// the look-back state of one fused-compaction launch of nBlocks blocks on c's stream
bool stage_events() {
    const char* e = getenv("FM3D_STAGE_EVENTS");
    return !(e && e[0] == '0');
}

// match_ms (row constants, knn, NNDR and its compaction: one stage since NNDR is fused into the
// match's last launch; nndr_ms stays 0) and triangulate_ms, when the step recorded its stage events
void stage_times(fm3d_ctx* c, fm3d_pipeline_stats* stats) {
    float ms = 0;
    stats->match_ms = stats->nndr_ms = stats->triangulate_ms = 0;  // 0 when the step recorded no stage events
    if (!c->stageEv) return;
    hipEventElapsedTime(&ms, c->ev[2], c->ev[3]);
    stats->match_ms = ms;
    stats->nndr_ms = 0;
    hipEventElapsedTime(&ms, c->ev[3], c->ev[5]);
    stats->triangulate_ms = ms;
}

int make_lookback(fm3d_ctx* c, int nBlocks, fm3d::LookBack* lb) {
    if (!c->lbCtr.p) {
        HIPCHK(c, c->lbCtr.ensure(64));
        HIPCHK(c, hipMemsetAsync(c->lbCtr.p, 0, 64, c->stream));  // each launch leaves it at 0
    }
    bool zero = false;
    if (c->lbSt.bytes < (size_t)nBlocks * 8) {
        HIPCHK(c, c->lbSt.ensure((size_t)nBlocks * 8 * 2));
        zero = true;
    }
    if (++c->lbEpoch == 0) {  // the 32-bit tag wrapped: 0 is the zeroed words' "not yet"
        c->lbEpoch = 1;
        zero = true;
    }
    if (zero) HIPCHK(c, hipMemsetAsync(c->lbSt.p, 0, c->lbSt.bytes, c->stream));  // epoch 0: "not yet"
    lb->st = c->lbSt.as<unsigned long long>();
    lb->ctr = c->lbCtr.as<unsigned>();
    lb->epoch = c->lbEpoch;
    return FM3D_OK;
}

// The buffers of one k = 2 search: the forward search's are the context's own; the cross-check's
// reverse search runs the same routes with the two sides' rows swapped and its
// own constants, unpacked / pair copies, part lists and top-2 lists.
struct KnnSide {
    DevBuf &A, &B;              // query rows, train rows (as stage_descriptors left them)
    DevBuf &cqA, &ctB;          // u8: query constants, packed train constants
    DevBuf &A8, &B8;            // 256-bit rows unpacked: queries 0/1, train rows -1/+1
    DevBuf &partIdx, &partKey;  // the parts' lists
    DevBuf &bPairs;             // float rows: the row-pair copy of the train side
    DevBuf &idx, &key, &fkey;   // the merged top-2 lists
};

// the k = 2 search of nA query rows over nB train rows into b.idx / b.key / b.fkey.  deferMerge: the
// int8-MFMA routes leave their parts' lists in b.partIdx / b.partKey and set *mergeParts (the fused
// NNDR launch merges them).  gate (fm3d_kernels.h EpiGate): every type takes its gated kernels.
int knn2_search(fm3d_ctx* c, const KnnSide& b, int nA, int nB, int type, int dimPad, bool deferMerge, int* mergeParts,
                const fm3d::EpiGate* gate) {
    *mergeParts = 1;
    HIPCHK(c, b.idx.ensure((size_t)nA * 2 * sizeof(int) + 16));
    HIPCHK(c, b.key.ensure((size_t)nA * 2 * sizeof(int) + 16));
    HIPCHK(c, b.fkey.ensure((size_t)nA * 2 * sizeof(float) + 16));
    if (c->nCU <= 0) {
        int n = 0;
        HIPCHK(c, hipDeviceGetAttribute(&n, hipDeviceAttributeMultiprocessorCount, c->device));
        c->nCU = n > 0 ? n : 1;
    }
    if (type == FM3D_DESC_U8) {
        const int nAPad = nA, nBPad = nB;
        HIPCHK(c, b.cqA.ensure((size_t)(nAPad + 1) * sizeof(int)));
        HIPCHK(c, b.ctB.ensure((size_t)(nBPad + 1) * sizeof(int)));
        fm3d::launch_rowconst_u8(b.A.as<uint8_t>(), nA, b.B.as<uint8_t>(), nB, dimPad, b.cqA.as<int>(),
                                 b.ctB.as<int>(), c->stream);
        const int parts = fm3d::knn2_u8_parts(nA, nB, c->nCU, fm3d::knn2_i8_queries_per_block(dimPad, 0),
                                              fm3d::knn2_i8_tile_rows(dimPad, 0));
        if (parts > 1) {
            HIPCHK(c, b.partIdx.ensure((size_t)parts * nA * 2 * sizeof(int) + 16));
            HIPCHK(c, b.partKey.ensure((size_t)parts * nA * 2 * sizeof(int) + 16));
        }
        if (deferMerge && parts > 1) *mergeParts = parts;
        fm3d::launch_knn2_i8(b.A.as<uint8_t>(), nA, b.B.as<uint8_t>(), nB, dimPad, 0, b.cqA.as<int>(),
                             b.ctB.as<int>(), parts, b.partIdx.as<int>(), b.partKey.as<int>(), b.idx.as<int>(),
                             b.key.as<int>(), c->stream, *mergeParts > 1, gate);
    } else if (type == FM3D_DESC_F32 && gate) {
        // no bf16 prefilter here (its bound knows nothing of the gate): the exact scan of the rows inside it
        const int parts = fm3d::knn2_parts(nA, nB, dimPad, c->nCU);
        if (parts > 1) {
            HIPCHK(c, b.partIdx.ensure((size_t)parts * nA * 2 * sizeof(int) + 16));
            HIPCHK(c, b.partKey.ensure((size_t)parts * nA * 2 * sizeof(float) + 16));
        }
        fm3d::launch_knn2_f32_gated(b.A.as<float>(), nA, b.B.as<float>(), nB, dimPad, parts, b.partIdx.as<int>(),
                                    b.partKey.as<float>(), b.idx.as<int>(), b.fkey.as<float>(), *gate, c->stream);
    } else if (type == FM3D_DESC_F32 && (dimPad == 64 || dimPad == 128) && nB >= 64 &&
               (long long)nA * nB >= (1LL << 22) && f32_mfma()) {
        // float rows (SURF): the bf16 MFMA prefilter lists each query's possible top-2 rows, whose exact
        // FLANN-order distances decide (fm3d_match.hip); the same result as the full exact scan
        const int parts = fm3d::knn2_f32_mfma_parts(nA, nB, c->nCU);
        HIPCHK(c, c->f32Work.ensure(fm3d::knn2_f32_mfma_bytes(nA, nB, dimPad, parts)));
        // one fused pass; when more than 1/8 of the queries overflow its lists, the two-pass form (whose
        // lists hold only the rows under the final bound); FM3D_F32_FUSED=0 starts with the two-pass form
        const char* fe = getenv("FM3D_F32_FUSED");
        bool fused = !(fe && fe[0] == '0');
        int nResc = 0;
        for (;;) {
            fm3d::launch_knn2_f32_mfma(b.A.as<float>(), nA, b.B.as<float>(), nB, dimPad, parts, fused, c->f32Work.p,
                                       b.idx.as<int>(), b.fkey.as<float>(), c->stream);
            HIPCHK(c, hipMemcpyAsync(&nResc, fm3d::knn2_f32_mfma_rescan_count(c->f32Work.p, nA, nB, dimPad, parts),
                                     sizeof(int), hipMemcpyDeviceToHost, c->stream));
            HIPCHK(c, hipStreamSynchronize(c->stream));
            if (!fused || nResc <= nA / 8) break;
            fused = false;
        }
        if (nResc > 0 && nResc <= nA / 8) {
            // the queries whose bound held more rows than the candidate list: an exact wave-per-query scan
            fm3d::launch_knn2_f32_mfma_rescan(b.A.as<float>(), b.B.as<float>(), nB, dimPad, c->f32Work.p, nA, parts,
                                              nResc, b.idx.as<int>(), b.fkey.as<float>(), c->stream);
        } else if (nResc > 0) {
            // descriptors with no margin between neighbours (e.g. uniform noise in high dimension):
            // the full exact scan for every query
            const int p2 = fm3d::knn2_parts(nA, nB, dimPad, c->nCU);
            if (p2 > 1) {
                HIPCHK(c, b.partIdx.ensure((size_t)p2 * nA * 2 * sizeof(int) + 16));
                HIPCHK(c, b.partKey.ensure((size_t)p2 * nA * 2 * sizeof(float) + 16));
            }
            HIPCHK(c, b.bPairs.ensure(fm3d::knn2_f32_pairs_bytes(nB, dimPad) + 16));
            fm3d::launch_knn2_f32(b.A.as<float>(), nA, b.B.as<float>(), nB, dimPad, p2, b.partIdx.as<int>(),
                                  b.partKey.as<float>(), b.bPairs.as<float>(), b.idx.as<int>(), b.fkey.as<float>(),
                                  c->stream);
        }
    } else if (type == FM3D_DESC_F32) {
        const int parts = (dimPad == 64 || dimPad == 128) ? fm3d::knn2_parts(nA, nB, dimPad, c->nCU) : 1;
        if (parts > 1) {
            HIPCHK(c, b.partIdx.ensure((size_t)parts * nA * 2 * sizeof(int) + 16));
            HIPCHK(c, b.partKey.ensure((size_t)parts * nA * 2 * sizeof(float) + 16));
        }
        HIPCHK(c, b.bPairs.ensure(fm3d::knn2_f32_pairs_bytes(nB, dimPad) + 16));
        fm3d::launch_knn2_f32(b.A.as<float>(), nA, b.B.as<float>(), nB, dimPad, parts, b.partIdx.as<int>(),
                              b.partKey.as<float>(), b.bPairs.as<float>(), b.idx.as<int>(), b.fkey.as<float>(),
                              c->stream);
    } else if (dimPad == 32 && bits_mfma()) {
        // 256-bit rows (ORB): unpacked to int8 and matched on the int8 MFMA kernel (exact integer
        // Hamming distances popc(b) - a.b', same ranking rule)
        HIPCHK(c, b.A8.ensure((size_t)nA * 256 + 16));
        HIPCHK(c, b.B8.ensure((size_t)nB * 256 + 16));
        HIPCHK(c, b.ctB.ensure((size_t)(nB + 1) * sizeof(int)));
        fm3d::launch_unpack_bits(b.A.as<uint8_t>(), nA, b.B.as<uint8_t>(), nB, b.A8.as<uint8_t>(),
                                 b.B8.as<uint8_t>(), b.ctB.as<int>(), c->stream);
        const int parts = fm3d::knn2_u8_parts(nA, nB, c->nCU, fm3d::knn2_i8_queries_per_block(256, 1),
                                              fm3d::knn2_i8_tile_rows(256, 1));
        if (parts > 1) {
            HIPCHK(c, b.partIdx.ensure((size_t)parts * nA * 2 * sizeof(int) + 16));
            HIPCHK(c, b.partKey.ensure((size_t)parts * nA * 2 * sizeof(int) + 16));
        }
        if (deferMerge && parts > 1) *mergeParts = parts;
        fm3d::launch_knn2_i8(b.A8.as<uint8_t>(), nA, b.B8.as<uint8_t>(), nB, 256, 1, nullptr, b.ctB.as<int>(),
                             parts, b.partIdx.as<int>(), b.partKey.as<int>(), b.idx.as<int>(), b.key.as<int>(),
                             c->stream, *mergeParts > 1, gate);
    } else {
        const int parts = fm3d::knn2_parts(nA, nB, dimPad, c->nCU);
        if (parts > 1) {
            HIPCHK(c, b.partIdx.ensure((size_t)parts * nA * 2 * sizeof(int) + 16));
            HIPCHK(c, b.partKey.ensure((size_t)parts * nA * 2 * sizeof(int) + 16));
        }
        fm3d::launch_knn2_bits(b.A.as<uint8_t>(), nA, b.B.as<uint8_t>(), nB, dimPad, parts, b.partIdx.as<int>(),
                               b.partKey.as<int>(), b.idx.as<int>(), b.key.as<int>(), c->stream, gate);
    }
    HIPCHK(c, hipGetLastError());
    return FM3D_OK;
}

// compactOut / compactCount (the pipeline): NNDR, the parts' merge (int keys) and the stable
// compaction of the kept matches in one launch (launch_nndr_compact); else the NNDR flags and
// candidates in c->flag / c->cand
// gate (the guided matchers, fm3d_kernels.h EpiGate): every type takes its gated kernels
// crossCheck 1 / 2 (with compactOut only): the reverse search over the same rows
// (and the same gate, transposed), then the NNDR launch's mutual form; 0 adds nothing
int run_match(fm3d_ctx* c, int nA, int nB, int type, int dimPad, double eps, int queryOffset, bool wantKnn,
              fm3d_dmatch* compactOut = nullptr, int* compactCount = nullptr, const fm3d::EpiGate* gate = nullptr,
              int crossCheck = 0) {
    const bool fuse = compactOut != nullptr && !wantKnn;
    if (crossCheck && !fuse) return fail(c, FM3D_ERR_INVALID, "the cross-check needs the compacted output");
    int mergeParts = 1;  // > 1: the parts' lists are merged by launch_nndr_compact
    HIPCHK(c, c->idx.ensure((size_t)nA * 2 * sizeof(int) + 16));
    HIPCHK(c, c->key.ensure((size_t)nA * 2 * sizeof(int) + 16));
    HIPCHK(c, c->fkey.ensure((size_t)nA * 2 * sizeof(float) + 16));
    HIPCHK(c, c->cand.ensure((size_t)nA * sizeof(fm3d_dmatch) + 16));
    HIPCHK(c, c->flag.ensure((size_t)nA * sizeof(int) + 16));
    if (wantKnn) HIPCHK(c, c->knnOut.ensure((size_t)nA * 2 * sizeof(fm3d_dmatch) + 16));
    {
        const KnnSide fwd{c->A, c->B, c->cqA, c->ctB, c->A8, c->B8, c->partIdx, c->partKey, c->bPairs, c->idx, c->key, c->fkey};
        int r;
        if ((r = knn2_search(c, fwd, nA, nB, type, dimPad, fuse, &mergeParts, gate))) return r;
    }
    if (crossCheck) {
        // rev[j]: train row j's two nearest queries.  With a gate both searches rank the same
        // admissible pairs: the reverse kernels evaluate the forward predicate with the sides swapped
        const KnnSide rev{c->B, c->A, c->rCq, c->rCt, c->rA8, c->rB8, c->rPartIdx, c->rPartKey, c->rPairs, c->rIdx, c->rKey, c->rFkey};
        fm3d::EpiGate rg{};
        if (gate) {
            rg = *gate;
            rg.transposed = true;
        }
        int r, revParts = 1;
        if ((r = knn2_search(c, rev, nB, nA, type, dimPad, false, &revParts, gate ? &rg : nullptr))) return r;
        fm3d::LookBack lb;
        if ((r = make_lookback(c, fm3d::nndr_compact_blocks(nA), &lb))) return r;
        const fm3d::MutualCheck mc{c->rIdx.as<int>(), c->rKey.as<int>(), c->rFkey.as<float>(), crossCheck};
        fm3d::launch_nndr_mutual_compact(type, c->idx.as<int>(), c->key.as<int>(), c->fkey.as<float>(),
                                         c->partIdx.as<int>(), c->partKey.as<int>(), mergeParts, nA, eps, queryOffset,
                                         mc, compactOut, compactCount, lb, c->stream);
    } else if (fuse) {
        fm3d::LookBack lb;
        int r;
        if ((r = make_lookback(c, fm3d::nndr_compact_blocks(nA), &lb))) return r;
        fm3d::launch_nndr_compact(type, c->idx.as<int>(), c->key.as<int>(), c->fkey.as<float>(), c->partIdx.as<int>(),
                                  c->partKey.as<int>(), mergeParts, nA, eps, queryOffset, compactOut, compactCount, lb,
                                  c->stream);
    } else {
        fm3d::launch_nndr(type, c->idx.as<int>(), c->key.as<int>(), c->fkey.as<float>(), nA, nB, eps, queryOffset,
                          wantKnn ? c->knnOut.as<fm3d_dmatch>() : nullptr, c->cand.as<fm3d_dmatch>(), c->flag.as<int>(),
                          c->stream);
    }
    HIPCHK(c, hipGetLastError());
    return FM3D_OK;
}

void fill_lm_cycles(const fm3d_ctx* c, const unsigned long long* cnt, fm3d_lm_stats* st) {
    st->groups = c->lmGroups;
    st->passes = (int64_t)cnt[3];
    st->cycles_terms = (int64_t)cnt[4];
    st->cycles_chain = (int64_t)cnt[5];
    st->cycles_control = (int64_t)cnt[6];
    st->cycles_total = (int64_t)cnt[7];
    st->wall_ticks_sum = (int64_t)cnt[8];
    st->wall_ticks_max = (int64_t)cnt[9];
    st->wall_clock_khz = c->wallKhz;
    for (int k = 0; k < 4; k++) {
        st->class_passes[k] = (int64_t)cnt[10 + k];
        st->class_cycles[k] = (int64_t)cnt[14 + k];
    }
    st->last_group_start_ticks = (int64_t)(cnt[18] - cnt[20]);
    st->last_group_end_ticks = (int64_t)(cnt[19] - cnt[20]);
    st->cycles_wait = (int64_t)cnt[24];
    st->chain_rounds = (int64_t)cnt[21];
    st->chain_chunks = (int64_t)cnt[22];
    st->queue_empty_ticks = cnt[25] ? (int64_t)(cnt[25] - cnt[20]) : 0;
}

// The LM kernel's camera: the settings' camera with a principal point of -0.0 replaced by +0.0.
// The kernel's isPixelGood compares bit patterns (0 <= u <= xmax as bits(u) <= bits(xmax)), which
// differs from the reference's comparison only for u == -0.0; u = xd*fx + cx (and the image-1
// centre, the same sum) is -0.0 only when cx is -0.0 and xd*fx is -0.0.  With +0.0 that sum is
// +0.0: the reference's test is true for both zeros, and the bilinear sample at a +-0 coordinate is
// the same.  Every other principal point (zero, negative, outside the image) gives the reference's
// bits: a negative u or NaN lies above bits(xmax) as the reference's comparison is false, and the
// fused a2 = r2 + 2x^2 differs only where x*x is subnormal, where u's float sample coordinate
// rounds to the same value (tests/test_gpu_parity.py::test_principal_point_zero_and_negative).
fm3d::Camera lm_camera(const fm3d::Camera& cam) {
    fm3d::Camera k = cam;
    if (k.cx == 0.) k.cx = 0.;  // -0.0 -> +0.0
    if (k.cy == 0.) k.cy = 0.;
    return k;
}

// One frame pair's points for an LM launch: its context (pyramids c->lvlDesc, pose c->R2/t2,
// outputs c->lm*, per-pair counters c->pcnt + 16 bytes) and the points (c->pts): P of them, or
// P their bound when Pdev holds the count on the device (the pipeline: no host sync)
struct LMSrc {
    fm3d_ctx* c;
    int P;
    const int* Pdev;
};

// LM normals over the points of nProb frame pairs in ONE launch on c's stream (c's slabs, queue
// and launch counters): the slots that find one pair's points used up take the next pair's, so
// a second pair fills the launch's end-of-queue tail (fm3d_pipeline_link).  Every problem's
// context must be ordered before this stream by the caller (its points, pyramids).
// the LM launch's workgroups for Ptot points (Ptot < 0: as many as the GPU holds): the settings'
// lmWaves, or every CU at the kernel's occupancy, bounded by the points, the slabs' HBM budget and
// their 32-bit offsets
int lm_groups(fm3d_ctx* c, const void* kptr, int slots, long Ptot, long* out) {
    long groups = c->s.lmWaves;
    if (groups <= 0) {
        int cus = 0, perCU = 0;
        HIPCHK(c, hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, c->device));
        HIPCHK(c, hipOccupancyMaxActiveBlocksPerMultiprocessor(&perCU, kptr, fm3d::kLM2Threads, 0));
        if (perCU < 1) perCU = 1;
        groups = (long)cus * perCU;
    }
    if (Ptot >= 0) {
        const long needed = (Ptot + slots - 1) / slots;
        if (groups > needed) groups = needed;
    }
    const size_t ents = (size_t)c->nOffPad * slots;
    // per slot and entry: rays (2 doubles) + I1, fvec dI, two Jacobian dI (float) + compact index
    const size_t perGroup = ents * (2 * sizeof(double) + 5 * 4);
    const size_t budget = (size_t)48 << 30;  // HBM budget for the per-slot pixel slabs
    long cap = (long)(budget / perGroup);
    if (cap < 1) cap = 1;
    if (groups > cap) groups = cap;
    // the summed passes address a slab array with a 32-bit byte offset
    const long cap32 = (long)((((size_t)1 << 32) - ((size_t)1 << 20)) / (ents * sizeof(double) * (FM3D_RAY_AOS ? 2 : 1)));
    if (groups > cap32) groups = cap32;
    if (groups < 1) groups = 1;
    *out = groups;
    return FM3D_OK;
}

int run_lm_multi(fm3d_ctx* c, const LMSrc* src, int nProb, fm3d_lm_stats* stats, hipEvent_t e0, hipEvent_t e1) {
    int r;
    if (nProb < 1 || nProb > fm3d::kLMMaxProblems) return fail(c, FM3D_ERR_INVALID, "bad LM problem count");
    if ((r = ensure_offsets(c))) return r;
    const fm3d::Camera cam = lm_camera(c->cam);
    const int levels = c->s.pyramids;
    long Ptot = 0;
    for (int j = 0; j < nProb; j++) {
        fm3d_ctx* q = src[j].c;
        if (q->pyr1.empty()) return fail(c, FM3D_ERR_INVALID, "fm3d_set_images (NormalOptimizer::setImages) not called");
        if (!q->haveG12) return fail(c, FM3D_ERR_INVALID, "g12 not set (SingleCameraTriangulator::setg12)");
        if (q != c && (q->device != c->device || q->s.pyramids != levels || q->s.pixelsRay != c->s.pixelsRay ||
                       std::memcmp(&q->cam, &c->cam, sizeof(c->cam)) != 0 || q->s.boundWidth != c->s.boundWidth ||
                       q->s.boundHeight != c->s.boundHeight || q->s.zThresholdMax != c->s.zThresholdMax ||
                       q->s.epsilonLMMIN != c->s.epsilonLMMIN || q->s.lmReduction != c->s.lmReduction))
            return fail(c, FM3D_ERR_INVALID, "linked contexts need one device, camera and LM settings");
        const int P = src[j].P;
        HIPCHK(c, q->lmNormals.ensure((size_t)(P + 1) * 3 * sizeof(double)));
        HIPCHK(c, q->lmStatus.ensure((size_t)(P + 1) * sizeof(int)));
        HIPCHK(c, q->lmInfo.ensure((size_t)(P + 1) * 8 * sizeof(int)));
        HIPCHK(c, q->lmNfev.ensure((size_t)(P + 1) * 8 * sizeof(int)));
        HIPCHK(c, q->lmMdat.ensure((size_t)(P + 1) * sizeof(int)));
        HIPCHK(c, q->pcnt.ensure(64));
        Ptot += P;
    }
    HIPCHK(c, c->lmQueue.ensure(64 * sizeof(int)));
    HIPCHK(c, c->lmStat.ensure(256));
    // persistent workgroups of fm3d::kLM2Slots term waves (one point each) + a chain wave, or in the
    // tree-reduction mode kLM2Slots + 1 term waves; slots refill from the queue (fm3d_lm2.hip)
    // the settings field alone picks the mode (no environment override: ADVICE r05; the tree mode
    // fails the parity gate, profiles/r05_full_parity.json)
    if (c->s.lmReduction != 0 && c->s.lmReduction != 1)
        return fail(c, FM3D_ERR_INVALID, "lmReduction must be 0 (pixel order) or 1 (tree)");
    const bool tree = c->s.lmReduction != 0;
    const int slots = fm3d::kLM2Slots + (tree ? 1 : 0);
    // one pose for all problems: the single-pose kernel (entry 0 of the table serves them all)
    bool multiPose = false;
    for (int j = 1; j < nProb; j++)
        multiPose |= std::memcmp(src[j].c->R2, src[0].c->R2, sizeof(c->R2)) != 0 ||
                     std::memcmp(src[j].c->t2, src[0].c->t2, sizeof(c->t2)) != 0;
    const void* kptr = tree ? (multiPose ? reinterpret_cast<const void*>(fm3d::lm2_kernel<true, true>)
                                         : reinterpret_cast<const void*>(fm3d::lm2_kernel<false, true>))
                            : (multiPose ? reinterpret_cast<const void*>(fm3d::lm2_kernel<true, false>)
                                         : reinterpret_cast<const void*>(fm3d::lm2_kernel<false, false>));
    long groups = 0;
    int r0;
    if ((r0 = lm_groups(c, kptr, slots, Ptot, &groups))) return r0;
    const size_t ents = (size_t)c->nOffPad * slots;
    // +8 KiB: the passes prefetch up to eight 64-entry chunks past a slot's last entry
    HIPCHK(c, c->slab.ensure(ents * 2 * sizeof(double) * groups + 16384));
    HIPCHK(c, c->slabI1.ensure(ents * 5 * 4 * groups + 16384));
    fm3d::LMParams p{};
    p.nProb = nProb;
    p.cam = cam;
    {   // per problem: its pose as a small global table (re-read per chunk by the LM kernel), and
        // the problem table; both from pinned memory (the copies may run after this returns)
        HIPCHK(c, hipEventSynchronize(c->evProj));  // the previous launch's copies out of hProj ran
        const size_t pcBytes = (sizeof(fm3d::ProjConst) + 255) / 256 * 256;
        HIPCHK(c, c->hProj.ensure(pcBytes * nProb + sizeof(fm3d::LMProblem) * nProb));
        char* hp = c->hProj.as<char>();
        fm3d::LMProblem* hpr = (fm3d::LMProblem*)(hp + pcBytes * nProb);
        HIPCHK(c, c->lmProj.ensure(pcBytes * nProb + sizeof(fm3d::LMProblem) * nProb));
        const size_t Gn = (size_t)groups * slots * c->nOffPad;  // entries per slab array
        for (int j = 0; j < nProb; j++) {
            fm3d_ctx* q = src[j].c;
            fm3d::ProjConst& pc = *(fm3d::ProjConst*)(hp + pcBytes * j);
            std::memcpy(pc.R, q->R2, sizeof(pc.R));
            std::memcpy(pc.t, q->t2, sizeof(pc.t));
            pc.cam = cam;
            pc.k2d = 2. * cam.k[2];
            pc.k3d = 2. * cam.k[3];
            pc.slabRX = (const char*)c->slab.p;
            pc.slabRY = FM3D_RAY_AOS ? pc.slabRX + sizeof(double) : pc.slabRX + Gn * sizeof(double);
            pc.slabI1 = (const char*)c->slabI1.p;
            pc.slabDF = (char*)c->slabI1.p + Gn * 4;
            pc.slabDJ0 = pc.slabDF + Gn * 4;
            pc.slabDJ1 = pc.slabDJ0 + Gn * 4;
            fm3d::LMProblem& pr = hpr[j];
            pr.points = q->pts.as<double>();
            pr.Pdev = src[j].Pdev;
            pr.P = src[j].P;
            pr.lvl = q->lvlDesc.as<LevelDesc>();
            pr.normals = q->lmNormals.as<double>();
            pr.status = q->lmStatus.as<int>();
            pr.info = q->lmInfo.as<int>();
            pr.nfev = q->lmNfev.as<int>();
            pr.mdat = q->lmMdat.as<int>();
            pr.stat = (unsigned long long*)(q->pcnt.as<char>() + 16);
            pr.projOff = (unsigned)(pcBytes * j);
        }
        HIPCHK(c, hipMemcpyAsync(c->lmProj.p, hp, pcBytes * nProb + sizeof(fm3d::LMProblem) * nProb,
                                 hipMemcpyHostToDevice, c->stream));
        HIPCHK(c, hipEventRecord(c->evProj, c->stream));
        p.proj = c->lmProj.as<fm3d::ProjConst>();
        p.prob = (const fm3d::LMProblem*)(c->lmProj.as<char>() + pcBytes * nProb);
    }
    p.levels = levels;
    p.offsets = c->offsets.as<int2>();
    p.nOff = c->nOff;
    p.nOffPad = c->nOffPad;
    p.boundW = c->s.boundWidth;
    p.boundH = c->s.boundHeight;
    p.epsfcn = c->s.epsilonLMMIN;
    p.cmax = (int)(2 * c->s.zThresholdMax);  // isInBoundingBox: int cMax = 2*z_threshold_max_ (:648)
    p.queue = c->lmQueue.as<int>();
    p.slab = c->slab.as<double>();
    p.slabI1 = c->slabI1.as<float>();
    p.nWaves = groups;
    p.statEval = c->lmStat.as<unsigned long long>();
    p.statPix = c->lmStat.as<unsigned long long>() + 1;
    p.overflow = (int*)(c->lmStat.as<unsigned long long>() + 2);
    p.statPass = c->lmStat.as<unsigned long long>() + 3;
    c->lmGroups = groups;
    {   // guards against a broken state machine (never expected to trigger): passes per slot
        // <= its points x levels x (300 evaluations + QR passes), and a wall-clock limit
        const long long perSlot = (Ptot + groups * slots - 1) / (groups * slots) + 1;
        p.maxIter = perSlot * (long long)(levels + 1) * 1600 + 10000;
        int khz = 0;
        if (hipDeviceGetAttribute(&khz, hipDeviceAttributeWallClockRate, c->device) != hipSuccess || khz <= 0) khz = 100000;
        const char* ms = getenv("FM3D_LM_MAX_SECONDS");  // watchdog (tests lower it; fractions allowed)
        const double secs = ms && atof(ms) > 0 ? atof(ms) : 300.;
        p.maxTicks = (long long)((double)khz * 1000. * secs);
        c->wallKhz = khz;
        const char* co = getenv("FM3D_LM_COOP");  // A/B switch for the tail help
        p.coop = co ? atoi(co) : 1;
        if (tree) p.coop = 0;  // a helper's chunks would leave the lanes' chunk order of the tree
        const char* sf = getenv("FM3D_LM_SAFE");  // test switch: the guarded pass forms only
        p.safe = sf ? atoi(sf) : 0;
    }
    // the counters (incl. the overflow word) are reset for every call, also for P == 0; with points,
    // the queue, the min-start word and every problem's statuses / info / nfev too -- one kernel
    {
        fm3d::LMReset rz{};
        rz.stat = c->lmStat.as<unsigned long long>();
        rz.queue = Ptot > 0 ? c->lmQueue.as<int>() : nullptr;
        rz.nProb = nProb;
        for (int j = 0; j < nProb; j++) {
            fm3d_ctx* q = src[j].c;
            rz.pcnt16[j] = q->pcnt.as<int>() + 4;
            rz.status[j] = q->lmStatus.as<int>();
            rz.info[j] = q->lmInfo.as<int>();
            rz.nfev[j] = q->lmNfev.as<int>();
            rz.P[j] = Ptot > 0 && src[j].P > 0 ? src[j].P : 0;
        }
        if (Ptot > 0) HIPCHK(c, hipEventRecord(e0, c->stream));
        fm3d::launch_lm_reset(rz, c->stream);
        HIPCHK(c, hipGetLastError());
    }
    if (Ptot > 0) {
        // one launch: every slot runs its point through all levels, coarsest first
        // (optimize_pyramid :225-241)
        // through the runtime's launch by address (not a call through a cast function pointer, which
        // the host sanitizers' function-type check rejects: tests/test_sanitizers.py)
        void* kargs[] = {&p};
        HIPCHK(c, hipLaunchKernel(kptr, dim3((unsigned)groups), dim3(fm3d::kLM2Threads), kargs, 0, c->stream));
        HIPCHK(c, hipEventRecord(e1, c->stream));
    }
    if (stats) {
        std::memset(stats, 0, sizeof(*stats));
        stats->points_in = Ptot;
    }
    return FM3D_OK;
}

// LM normals over c's own points (c->pts: P, or the bound P with the count at Pdev)
int run_lm(fm3d_ctx* c, int P, const int* Pdev, fm3d_lm_stats* stats, hipEvent_t e0, hipEvent_t e1) {
    const LMSrc one{c, P, Pdev};
    return run_lm_multi(c, &one, 1, stats, e0, e1);
}

// the two images into pinned staging and their pyramids (pyrDown chain) on the context stream;
// sync: wait for them before returning (fm3d_set_images: the caller may read them back at once)
int set_images_impl(fm3d_ctx* c, const uint8_t* img1, const uint8_t* img2, int width, int height, int stride,
                    bool sync = true, bool waitStaging = true) {
    if (!img1 || !img2 || width <= 0 || height <= 0 || stride < width)
        return fail(c, FM3D_ERR_INVALID, "bad image arguments");
    const int levels = c->s.pyramids;
    if (levels < 0 || levels > 7) return fail(c, FM3D_ERR_UNSUPPORTED, "pyramids must be in [0, 7]");
    int r;
    if (waitStaging && (r = staging_wait(c))) return r;
    c->w = width;
    c->h = height;
    c->lw.assign(levels + 1, 0);
    c->lh.assign(levels + 1, 0);
    c->pyr1.resize(levels + 1);
    c->pyr2.resize(levels + 1);
    c->lw[0] = width;
    c->lh[0] = height;
    for (int L = 1; L <= levels; L++) {  // cv::pyrDown size ((w+1)/2, (h+1)/2)
        c->lw[L] = (c->lw[L - 1] + 1) / 2;
        c->lh[L] = (c->lh[L - 1] + 1) / 2;
    }
    // the zero guards: cleared when a level's buffer is new or the image size changed, not per frame
    // pair -- nothing but the guard clearing writes past a level's w x h pixels, so they stay zero
    // (each clear is a fill kernel, which in a stream of frame pairs waits for CUs behind the other
    // pairs' LM launches)
    bool fresh = c->pyrGuardW != width || c->pyrGuardH != height || c->pyrGuardLevels != levels;
    for (int L = 0; L <= levels; L++) {
        size_t bytes = (size_t)c->lw[L] * c->lh[L] + kGuard(c->lw[L]);
        void* p1 = c->pyr1[L].p;
        void* p2 = c->pyr2[L].p;
        HIPCHK(c, c->pyr1[L].ensure(bytes));
        HIPCHK(c, c->pyr2[L].ensure(bytes));
        fresh |= c->pyr1[L].p != p1 || c->pyr2[L].p != p2;
    }
    for (int L = 0; fresh && L <= levels; L++) {
        // a level's pixels are overwritten (level 0 by the copy below, the others by pyrDown): the
        // guard past them is what needs clearing
        const size_t img = (size_t)c->lw[L] * c->lh[L];
        HIPCHK(c, hipMemsetAsync((char*)c->pyr1[L].p + img, 0, c->pyr1[L].bytes - img, c->stream));
        HIPCHK(c, hipMemsetAsync((char*)c->pyr2[L].p + img, 0, c->pyr2[L].bytes - img, c->stream));
    }
    c->pyrGuardW = width;
    c->pyrGuardH = height;
    c->pyrGuardLevels = levels;
    const size_t wh = (size_t)width * height;
    HIPCHK(c, c->hImg.ensure(2 * wh));
    for (int y = 0; y < height; y++) {
        std::memcpy(c->hImg.as<uint8_t>() + (size_t)y * width, img1 + (size_t)y * stride, width);
        std::memcpy(c->hImg.as<uint8_t>() + wh + (size_t)y * width, img2 + (size_t)y * stride, width);
    }
    HIPCHK(c, hipMemcpyAsync(c->pyr1[0].p, c->hImg.p, wh, hipMemcpyHostToDevice, c->stream));
    HIPCHK(c, hipMemcpyAsync(c->pyr2[0].p, c->hImg.as<uint8_t>() + wh, wh, hipMemcpyHostToDevice, c->stream));
    for (int L = 1; L <= levels; L++) {
        fm3d::launch_pyrdown(c->pyr1[L - 1].as<uint8_t>(), c->lw[L - 1], c->lh[L - 1], c->pyr1[L].as<uint8_t>(),
                             c->stream);
        fm3d::launch_pyrdown(c->pyr2[L - 1].as<uint8_t>(), c->lw[L - 1], c->lh[L - 1], c->pyr2[L].as<uint8_t>(),
                             c->stream);
    }
    HIPCHK(c, hipGetLastError());
    HIPCHK(c, c->hTab.ensure((levels + 1) * sizeof(LevelDesc)));
    LevelDesc* d = c->hTab.as<LevelDesc>();
    for (int L = 0; L <= levels; L++) d[L] = LevelDesc{c->pyr1[L].as<uint8_t>(), c->pyr2[L].as<uint8_t>(), c->lw[L], c->lh[L]};
    HIPCHK(c, c->lvlDesc.ensure((levels + 1) * sizeof(LevelDesc)));
    HIPCHK(c, hipMemcpyAsync(c->lvlDesc.p, d, (levels + 1) * sizeof(LevelDesc), hipMemcpyHostToDevice, c->stream));
    HIPCHK(c, hipEventRecord(c->evStage, c->stream));
    if (sync) HIPCHK(c, hipStreamSynchronize(c->stream));
    return FM3D_OK;
}

}  // namespace

extern "C" {

const char* fm3d_version(void) { return "fm3d 0.1 (gfx950)"; }

int fm3d_ctx_create(const fm3d_settings* s, int device, fm3d_ctx** out) {
    if (!s || !out) return FM3D_ERR_INVALID;
    *out = nullptr;
    if (s->dltSolver != 0 && s->dltSolver != 1) return FM3D_ERR_INVALID;  // cvSVD or the legacy Jacobi
    if (!(s->guidedMatchPx >= 0. && s->guidedMatchPx <= DBL_MAX)) return FM3D_ERR_INVALID;  // 0 = off; NaN fails
    if (s->crossCheck < 0 || s->crossCheck > 2) return FM3D_ERR_INVALID;  // off, mutual nearest, symmetric ratio
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess || n <= 0) return FM3D_ERR_HIP;
    if (device < 0 || device >= n) return FM3D_ERR_INVALID;
    if (hipSetDevice(device) != hipSuccess) return FM3D_ERR_HIP;
    fm3d_ctx* c = new fm3d_ctx();
    c->s = *s;
    c->device = device;
    if (hipStreamCreateWithFlags(&c->stream, hipStreamNonBlocking) != hipSuccess) {
        delete c;
        return FM3D_ERR_HIP;
    }
    c->ownStream = true;
    // test hook: the look-back tag to start from (tests/test_gpu_c2_pipeline.py runs across its wrap)
    if (const char* le = getenv("FM3D_DEBUG_LB_EPOCH")) c->lbEpoch = (unsigned)strtoul(le, nullptr, 0);
    for (auto& e : c->ev) hipEventCreate(&e);
    hipEventCreateWithFlags(&c->evStage, hipEventDisableTiming);
    hipEventCreateWithFlags(&c->evProj, hipEventDisableTiming);
    hipEventCreateWithFlags(&c->evFront, hipEventDisableTiming);
    hipEventCreateWithFlags(&c->evLm, hipEventDisableTiming);
    c->cam.fx = s->Fx;
    c->cam.fy = s->Fy;
    c->cam.cx = s->Cx;
    c->cam.cy = s->Cy;
    c->cam.k[0] = s->k0;
    c->cam.k[1] = s->k1;
    c->cam.k[2] = s->p1;
    c->cam.k[3] = s->p2;
    c->cam.k[4] = s->k2;
    *out = c;
    return FM3D_OK;
}

void fm3d_ctx_destroy(fm3d_ctx* c) {
    if (!c) return;
    hipSetDevice(c->device);
    hipStreamSynchronize(c->stream);
    if (c->linkLeader) {
        auto& v = c->linkLeader->linkMembers;
        v.erase(std::remove(v.begin(), v.end(), c), v.end());
    }
    for (fm3d_ctx* m : c->linkMembers) m->linkLeader = nullptr;
    delete c;
}

const char* fm3d_last_error(const fm3d_ctx* c) { return c ? c->err.c_str() : "null context"; }

int fm3d_ctx_set_stream(fm3d_ctx* c, void* stream) {
    if (!c) return FM3D_ERR_INVALID;
    hipSetDevice(c->device);
    hipStreamSynchronize(c->stream);
    if (c->ownStream) hipStreamDestroy(c->stream);
    if (stream) {
        c->stream = (hipStream_t)stream;
        c->ownStream = false;
    } else {
        HIPCHK(c, hipStreamCreateWithFlags(&c->stream, hipStreamNonBlocking));
        c->ownStream = true;
    }
    return FM3D_OK;
}

int fm3d_knn2(fm3d_ctx* c, const void* descA, int nA, const void* descB, int nB, int dim, int type, fm3d_dmatch* out) {
    if (!c || (!descA && nA) || (!descB && nB) || (!out && nA)) return fail(c, FM3D_ERR_INVALID, "null argument");
    hipSetDevice(c->device);
    int t, dp, r;
    if ((r = stage_descriptors(c, descA, nA, descB, nB, dim, type, &t, &dp))) return r;
    if ((r = run_match(c, nA, nB, t, dp, 0.0, 0, true))) return r;
    if (nA) HIPCHK(c, hipMemcpyAsync(out, c->knnOut.p, (size_t)nA * 2 * sizeof(fm3d_dmatch), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    return FM3D_OK;
}

int fm3d_match_nndr(fm3d_ctx* c, const void* descA, int nA, const void* descB, int nB, int dim, int type,
                    double epsilon, fm3d_dmatch* matches, int* nMatches) {
    if (!c || !nMatches || (!descA && nA) || (!descB && nB) || (!matches && nA))
        return fail(c, FM3D_ERR_INVALID, "null argument");
    hipSetDevice(c->device);
    int t, dp, r;
    if ((r = stage_descriptors(c, descA, nA, descB, nB, dim, type, &t, &dp))) return r;
    if ((r = run_match(c, nA, nB, t, dp, epsilon, 0, false))) return r;
    if ((r = ensure_scan_tmp(c, nA))) return r;
    HIPCHK(c, c->matches.ensure((size_t)(nA + 1) * sizeof(fm3d_dmatch)));
    fm3d::launch_compact_dmatch(c->cand.as<fm3d_dmatch>(), c->flag.as<int>(), nA, c->matches.as<fm3d_dmatch>(),
                                c->count.as<int>(), c->scanTmp.p, c->stream);
    HIPCHK(c, hipGetLastError());
    int n = 0;
    HIPCHK(c, hipMemcpyAsync(&n, c->count.p, sizeof(int), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    if (n) HIPCHK(c, hipMemcpy(matches, c->matches.p, (size_t)n * sizeof(fm3d_dmatch), hipMemcpyDeviceToHost));
    *nMatches = n;
    return FM3D_OK;
}

namespace {
// descriptors and keypoints of a guided call onto the device, and its gate
int stage_guided(fm3d_ctx* c, const void* descA, int nA, const void* descB, int nB, int dim, int type,
                 const fm3d_point2f* kpts1, const fm3d_point2f* kpts2, double maxPx, int* t, int* dp,
                 fm3d::EpiGate* gate) {
    if (!c->haveG12) return fail(c, FM3D_ERR_INVALID, "g12 not set (SingleCameraTriangulator::setg12)");
    if (!good_max_px(maxPx)) return fail(c, FM3D_ERR_INVALID, "maxPx must be finite and > 0");
    hipSetDevice(c->device);
    int r;
    if ((r = stage_descriptors(c, descA, nA, descB, nB, dim, type, t, dp))) return r;
    if ((r = upload(c, c->kp1, kpts1, (size_t)nA * sizeof(fm3d_point2f)))) return r;
    if ((r = upload(c, c->kp2, kpts2, (size_t)nB * sizeof(fm3d_point2f)))) return r;
    c->gateStaged = false;  // (a staged pipeline pair's keypoints are replaced, as fm3d_triangulate replaces them)
    return make_gate(c, c->kp1.as<fm3d_point2f>(), nA, c->kp2.as<fm3d_point2f>(), nB, maxPx, gate);
}
}  // namespace

int fm3d_epipolar_lines(fm3d_ctx* c, const fm3d_point2f* kpts1, int n1, float* lines) {
    if (!c || n1 < 0 || (!kpts1 && n1) || (!lines && n1)) return fail(c, FM3D_ERR_INVALID, "null argument");
    if (!c->haveG12) return fail(c, FM3D_ERR_INVALID, "g12 not set (SingleCameraTriangulator::setg12)");
    hipSetDevice(c->device);
    int r;
    if ((r = upload(c, c->kp1, kpts1, (size_t)n1 * sizeof(fm3d_point2f)))) return r;
    c->gateStaged = false;
    fm3d::EpiGate g{};
    if ((r = make_gate(c, c->kp1.as<fm3d_point2f>(), n1, nullptr, 0, 1.0, &g))) return r;
    if (n1) HIPCHK(c, hipMemcpyAsync(lines, c->gLines.p, (size_t)n1 * sizeof(float4), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    return FM3D_OK;
}

int fm3d_knn2_guided(fm3d_ctx* c, const void* descA, int nA, const void* descB, int nB, int dim, int type,
                     const fm3d_point2f* kpts1, const fm3d_point2f* kpts2, double maxPx, fm3d_dmatch* out) {
    if (!c || (!descA && nA) || (!descB && nB) || (!out && nA) || (!kpts1 && nA) || (!kpts2 && nB))
        return fail(c, FM3D_ERR_INVALID, "null argument");
    int t, dp, r;
    fm3d::EpiGate gate{};
    if ((r = stage_guided(c, descA, nA, descB, nB, dim, type, kpts1, kpts2, maxPx, &t, &dp, &gate))) return r;
    if ((r = run_match(c, nA, nB, t, dp, 0.0, 0, true, nullptr, nullptr, &gate))) return r;
    if (nA) HIPCHK(c, hipMemcpyAsync(out, c->knnOut.p, (size_t)nA * 2 * sizeof(fm3d_dmatch), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    return FM3D_OK;
}

int fm3d_match_nndr_guided(fm3d_ctx* c, const void* descA, int nA, const void* descB, int nB, int dim, int type,
                           const fm3d_point2f* kpts1, const fm3d_point2f* kpts2, double epsilon, double maxPx,
                           fm3d_dmatch* matches, int* nMatches) {
    if (!c || !nMatches || (!descA && nA) || (!descB && nB) || (!matches && nA) || (!kpts1 && nA) || (!kpts2 && nB))
        return fail(c, FM3D_ERR_INVALID, "null argument");
    int t, dp, r;
    fm3d::EpiGate gate{};
    if ((r = stage_guided(c, descA, nA, descB, nB, dim, type, kpts1, kpts2, maxPx, &t, &dp, &gate))) return r;
    if ((r = run_match(c, nA, nB, t, dp, epsilon, 0, false, nullptr, nullptr, &gate))) return r;
    if ((r = ensure_scan_tmp(c, nA))) return r;
    HIPCHK(c, c->matches.ensure((size_t)(nA + 1) * sizeof(fm3d_dmatch)));
    fm3d::launch_compact_dmatch(c->cand.as<fm3d_dmatch>(), c->flag.as<int>(), nA, c->matches.as<fm3d_dmatch>(),
                                c->count.as<int>(), c->scanTmp.p, c->stream);
    HIPCHK(c, hipGetLastError());
    int n = 0;
    HIPCHK(c, hipMemcpyAsync(&n, c->count.p, sizeof(int), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    if (n) HIPCHK(c, hipMemcpy(matches, c->matches.p, (size_t)n * sizeof(fm3d_dmatch), hipMemcpyDeviceToHost));
    *nMatches = n;
    return FM3D_OK;
}

namespace {
// the compacted matches of a cross-checked call (c->matches, c->count) to the host
int mutual_download(fm3d_ctx* c, fm3d_dmatch* matches, int* nMatches) {
    int n = 0;
    HIPCHK(c, hipMemcpyAsync(&n, c->count.p, sizeof(int), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    if (n) HIPCHK(c, hipMemcpy(matches, c->matches.p, (size_t)n * sizeof(fm3d_dmatch), hipMemcpyDeviceToHost));
    *nMatches = n;
    return FM3D_OK;
}
}  // namespace

int fm3d_match_mutual(fm3d_ctx* c, const void* descA, int nA, const void* descB, int nB, int dim, int type,
                      double epsilon, int mode, fm3d_dmatch* matches, int* nMatches) {
    if (!c || !nMatches || (!descA && nA) || (!descB && nB) || (!matches && nA))
        return fail(c, FM3D_ERR_INVALID, "null argument");
    if (mode != 1 && mode != 2) return fail(c, FM3D_ERR_INVALID, "mode must be 1 (mutual nearest) or 2 (symmetric ratio)");
    hipSetDevice(c->device);
    int t, dp, r;
    if ((r = stage_descriptors(c, descA, nA, descB, nB, dim, type, &t, &dp))) return r;
    if ((r = ensure_scan_tmp(c, nA))) return r;
    HIPCHK(c, c->matches.ensure((size_t)(nA + 1) * sizeof(fm3d_dmatch)));
    if ((r = run_match(c, nA, nB, t, dp, epsilon, 0, false, c->matches.as<fm3d_dmatch>(), c->count.as<int>(), nullptr,
                       mode)))
        return r;
    return mutual_download(c, matches, nMatches);
}

int fm3d_match_mutual_guided(fm3d_ctx* c, const void* descA, int nA, const void* descB, int nB, int dim, int type,
                             const fm3d_point2f* kpts1, const fm3d_point2f* kpts2, double epsilon, double maxPx,
                             int mode, fm3d_dmatch* matches, int* nMatches) {
    if (!c || !nMatches || (!descA && nA) || (!descB && nB) || (!matches && nA) || (!kpts1 && nA) || (!kpts2 && nB))
        return fail(c, FM3D_ERR_INVALID, "null argument");
    if (mode != 1 && mode != 2) return fail(c, FM3D_ERR_INVALID, "mode must be 1 (mutual nearest) or 2 (symmetric ratio)");
    int t, dp, r;
    fm3d::EpiGate gate{};
    if ((r = stage_guided(c, descA, nA, descB, nB, dim, type, kpts1, kpts2, maxPx, &t, &dp, &gate))) return r;
    if ((r = ensure_scan_tmp(c, nA))) return r;
    HIPCHK(c, c->matches.ensure((size_t)(nA + 1) * sizeof(fm3d_dmatch)));
    if ((r = run_match(c, nA, nB, t, dp, epsilon, 0, false, c->matches.as<fm3d_dmatch>(), c->count.as<int>(), &gate,
                       mode)))
        return r;
    return mutual_download(c, matches, nMatches);
}

int fm3d_setg12(fm3d_ctx* c, const double T1[3], const double T2[3], const double r1[3], const double r2[3],
                double g12[16]) {
    if (!c || !T1 || !T2 || !r1 || !r2) return fail(c, FM3D_ERR_INVALID, "null argument");
    double g[16];
    fm3d_g12_from_poses(&c->s, T1, T2, r1, r2, g);
    install_g12(c, g);
    if (g12) std::memcpy(g12, g, sizeof(g));
    return FM3D_OK;
}

int fm3d_set_g12(fm3d_ctx* c, const double g12[16]) {
    if (!c || !g12) return fail(c, FM3D_ERR_INVALID, "null argument");
    install_g12(c, g12);
    return FM3D_OK;
}

int fm3d_get_camera2(const fm3d_ctx* c, double R2[9], double t2[3]) {
    if (!c || !c->haveG12) return FM3D_ERR_INVALID;
    std::memcpy(R2, c->R2, sizeof(c->R2));
    std::memcpy(t2, c->t2, sizeof(c->t2));
    return FM3D_OK;
}

int fm3d_triangulate(fm3d_ctx* c, const fm3d_point2f* kpts1, int n1, const fm3d_point2f* kpts2, int n2,
                     const fm3d_dmatch* matches, int K, double* points, uint8_t* inlierMask, int* nPoints) {
    if (!c || !nPoints || K < 0) return fail(c, FM3D_ERR_INVALID, "bad argument");
    if (!c->haveG12) return fail(c, FM3D_ERR_INVALID, "g12 not set (SingleCameraTriangulator::setg12)");
    hipSetDevice(c->device);
    for (int i = 0; i < K; i++)
        if (matches[i].queryIdx < 0 || matches[i].queryIdx >= n1 || matches[i].trainIdx < 0 || matches[i].trainIdx >= n2)
            return fail(c, FM3D_ERR_INVALID, "match index out of range");  // std::vector::at would throw
    int r;
    if ((r = upload(c, c->kp1, kpts1, (size_t)n1 * sizeof(fm3d_point2f)))) return r;
    if ((r = upload(c, c->kp2, kpts2, (size_t)n2 * sizeof(fm3d_point2f)))) return r;
    if ((r = upload(c, c->matches, matches, (size_t)K * sizeof(fm3d_dmatch)))) return r;
    HIPCHK(c, c->triPts.ensure((size_t)(K + 1) * 3 * sizeof(double)));
    HIPCHK(c, c->triMask.ensure((size_t)(K + 1) * sizeof(int)));
    HIPCHK(c, c->triMask8.ensure((size_t)(K + 1)));
    HIPCHK(c, c->pts.ensure((size_t)(K + 1) * 3 * sizeof(double)));
    HIPCHK(c, c->srcIdx.ensure((size_t)(K + 1) * sizeof(int)));
    if ((r = ensure_scan_tmp(c, K))) return r;
    fm3d::TriParams p{};
    p.cam = c->cam;
    std::memcpy(p.g12, c->g12, sizeof(p.g12));
    p.zmin = c->s.zThresholdMin;
    p.zmax = c->s.zThresholdMax;
    p.kp1 = c->kp1.as<fm3d_point2f>();
    p.kp2 = c->kp2.as<fm3d_point2f>();
    p.matches = c->matches.as<fm3d_dmatch>();
    p.K = K;
    p.queryOffset = 0;
    p.pts = c->triPts.as<double>();
    p.mask = c->triMask.as<int>();
    p.mask8 = c->triMask8.as<uint8_t>();
    p.dltSolver = c->s.dltSolver;
    fm3d::launch_triangulate(p, c->stream);
    fm3d::launch_compact_points(c->triPts.as<double>(), c->triMask.as<int>(), K, nullptr, c->pts.as<double>(),
                                c->count.as<int>(), c->srcIdx.as<int>(), c->scanTmp.p, c->stream);
    HIPCHK(c, hipGetLastError());
    int n = 0;
    HIPCHK(c, hipMemcpyAsync(&n, c->count.p, sizeof(int), hipMemcpyDeviceToHost, c->stream));
    if (inlierMask && K) HIPCHK(c, hipMemcpyAsync(inlierMask, c->triMask8.p, K, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    if (n && points) HIPCHK(c, hipMemcpy(points, c->pts.p, (size_t)n * 3 * sizeof(double), hipMemcpyDeviceToHost));
    *nPoints = n;
    return FM3D_OK;
}

int fm3d_set_images(fm3d_ctx* c, const uint8_t* img1, const uint8_t* img2, int width, int height, int stride) {
    if (!c) return FM3D_ERR_INVALID;
    hipSetDevice(c->device);
    return set_images_impl(c, img1, img2, width, height, stride);
}

int fm3d_get_pyramid_level(const fm3d_ctx* cc, int which, int level, uint8_t* out, int* w, int* h) {
    fm3d_ctx* c = const_cast<fm3d_ctx*>(cc);
    if (!c || level < 0 || level >= (int)c->pyr1.size() || (which != 1 && which != 2)) return FM3D_ERR_INVALID;
    hipSetDevice(c->device);
    if (w) *w = c->lw[level];
    if (h) *h = c->lh[level];
    if (out) {
        const DevBuf& b = which == 1 ? c->pyr1[level] : c->pyr2[level];
        HIPCHK(c, hipMemcpy(out, b.p, (size_t)c->lw[level] * c->lh[level], hipMemcpyDeviceToHost));
    }
    return FM3D_OK;
}

int fm3d_optimize_normals(fm3d_ctx* c, double* points, int P, double* normals, int32_t* status, int32_t* info,
                          int32_t* nfev, int* nKept, fm3d_lm_stats* stats) {
    if (!c || !nKept || P < 0 || (P && (!points || !normals))) return fail(c, FM3D_ERR_INVALID, "bad argument");
    hipSetDevice(c->device);
    int r;
    if ((r = upload(c, c->pts, points, (size_t)P * 3 * sizeof(double)))) return r;
    if ((r = run_lm(c, P, nullptr, stats, c->ev[0], c->ev[1]))) return r;
    std::vector<double> nrm((size_t)P * 3);
    std::vector<int> st(P), inf((size_t)P * 8), nf((size_t)P * 8);
    unsigned long long cnt[26] = {};
    if (P) {
        HIPCHK(c, hipMemcpyAsync(nrm.data(), c->lmNormals.p, nrm.size() * sizeof(double), hipMemcpyDeviceToHost, c->stream));
        HIPCHK(c, hipMemcpyAsync(st.data(), c->lmStatus.p, st.size() * sizeof(int), hipMemcpyDeviceToHost, c->stream));
        HIPCHK(c, hipMemcpyAsync(inf.data(), c->lmInfo.p, inf.size() * sizeof(int), hipMemcpyDeviceToHost, c->stream));
        HIPCHK(c, hipMemcpyAsync(nf.data(), c->lmNfev.p, nf.size() * sizeof(int), hipMemcpyDeviceToHost, c->stream));
        HIPCHK(c, hipMemcpyAsync(cnt, c->lmStat.p, sizeof(cnt), hipMemcpyDeviceToHost, c->stream));
    }
    HIPCHK(c, hipStreamSynchronize(c->stream));
    int overflow = 0;  // lmStat is reset by run_lm for every call (P == 0 included)
    HIPCHK(c, hipMemcpy(&overflow, c->lmStat.as<unsigned long long>() + 2, sizeof(int), hipMemcpyDeviceToHost));
    if (overflow) return fail(c, FM3D_ERR_HIP, "LM kernel iteration guard tripped (internal error)");
    float ms = 0.f;
    if (P) hipEventElapsedTime(&ms, c->ev[0], c->ev[1]);
    // erase semantics (normaloptimizer.cpp:366,378): stable compaction, input order kept
    int kept = 0;
    bool nanPlane = false;
    for (int i = 0; i < P; i++) {
        if (status) status[i] = st[i];
        if (info) std::memcpy(&info[(size_t)8 * i], &inf[(size_t)8 * i], 8 * sizeof(int));
        if (nfev) std::memcpy(&nfev[(size_t)8 * i], &nf[(size_t)8 * i], 8 * sizeof(int));
        if (st[i] == FM3D_ST_NAN_PLANE) nanPlane = true;
        if (st[i] == FM3D_ST_OK) {
            for (int k = 0; k < 3; k++) {
                points[3 * kept + k] = points[3 * i + k];
                normals[3 * kept + k] = nrm[3 * i + k];
            }
            kept++;
        }
    }
    *nKept = kept;
    if (stats) {
        stats->points_in = P;
        stats->points_kept = kept;
        stats->evaluations = (int64_t)cnt[0];
        stats->pixel_evaluations = (int64_t)cnt[1];
        for (int i = 0; i < P; i++)
            if (st[i] >= 0 && st[i] < 8) stats->drops[st[i]]++;
        stats->kernel_ms = ms;
        fill_lm_cycles(c, cnt, stats);
    }
    if (nanPlane && c->s.strictNanExit)
        return fail(c, FM3D_ERR_NAN_PLANE, "projectPointToPlane hit NaN (reference: exit(-6))");
    return FM3D_OK;
}

// ---------------- whole pipeline, device resident ----------------
}  // extern "C"
namespace {
#define PENDING_CHECK(c)                                                                            \
    do {                                                                                            \
        if ((c)->pending)                                                                           \
            return fail((c), FM3D_ERR_INVALID, "a submitted frame pair is pending: fm3d_pipeline_wait first"); \
    } while (0)

// the inputs of one frame pair into HBM on the context stream (pinned staging, asynchronous):
// descriptors, keypoints, both images and their pyramids (a6, normaloptimizer.cpp:206-221)
int stage_pipeline(fm3d_ctx* c, const void* descA, int nA, const void* descB, int nB, int dim, int type,
                   const fm3d_point2f* kpts1, const fm3d_point2f* kpts2, const uint8_t* img1, const uint8_t* img2,
                   int width, int height, int queryOffset, bool speculate = false) {
    if (!kpts1 || !kpts2) return fail(c, FM3D_ERR_INVALID, "null argument");
    int t, dp, r;
    // the previous pair's copies out of the staging buffers have run: one wait, then every H2D of
    // this pair is queued without another (the call returns before they execute)
    if ((r = staging_wait(c))) return r;
    if ((r = stage_descriptors(c, descA, nA, descB, nB, dim, type, &t, &dp, false, speculate))) return r;
    if ((r = upload_pinned(c, c->kp1, c->hK1, kpts1, (size_t)nA * sizeof(fm3d_point2f)))) return r;
    if ((r = upload_pinned(c, c->kp2, c->hK2, kpts2, (size_t)nB * sizeof(fm3d_point2f)))) return r;
    if (img1 || img2) {
        if ((r = set_images_impl(c, img1, img2, width, height, width, false, false))) return r;  // records evStage
    } else {  // no images (C2's match + DLT needs none): the context keeps the ones it has, if any
        HIPCHK(c, hipEventRecord(c->evStage, c->stream));
    }
    if (!c->haveG12) {
        double g[16];
        if ((r = fm3d_setg12(c, c->s.pos1, c->s.pos2, c->s.pos1 + 3, c->s.pos2 + 3, g))) return r;
    }
    if ((r = ensure_offsets(c))) return r;
    c->stNA = nA;
    c->stNB = nB;
    c->stDim = dim;
    c->stType = t;
    c->stDimPad = dp;
    c->stQueryOffset = queryOffset;
    c->staged = true;
    c->gateStaged = false;
    return FM3D_OK;
}

// The front half on the staged inputs (ev[2..5]) is match -> NNDR -> compaction (front_match), then DLT
// triangulation -> compaction (front_dlt), sized by the query count: the match count K and the
// inlier count P stay on the device (c->pcnt[0], [1]) and bound nothing the host launches, so the
// stages queue without a host round trip (c->matches, c->pts, c->srcIdx hold K / P entries)
int front_match(fm3d_ctx* c) {
    const int nA = c->stNA, nB = c->stNB;
    int r;
    hipEvent_t* ev = c->ev;
    HIPCHK(c, c->pcnt.ensure(64));
    int* cnt = c->pcnt.as<int>();
    // Fm3d.guidedMatchPx: the epipolar gate over the staged keypoints (kp1 holds this share's queries),
    // its lines and (u, v) computed once per upload and pose
    fm3d::EpiGate gate{};
    const bool guided = c->s.guidedMatchPx > 0.;
    if (guided) {
        if (!c->gateStaged) {
            if ((r = make_gate(c, c->kp1.as<fm3d_point2f>(), nA, c->kp2.as<fm3d_point2f>(), nB, c->s.guidedMatchPx, &gate)))
                return r;
            c->gateStaged = true;
        }
        gate.lines = c->gLines.as<float4>();
        gate.uv = c->gUV.as<float2>();
        gate.tau = c->s.guidedMatchPx * 2.0 / (c->cam.fx + c->cam.fy);
    }
    HIPCHK(c, hipEventRecord(ev[2], c->stream));
    // a1: match + NNDR (+ the stable compaction of the kept matches, fused into the NNDR launch)
    if ((r = ensure_scan_tmp(c, nA))) return r;
    HIPCHK(c, c->matches.ensure((size_t)(nA + 1) * sizeof(fm3d_dmatch)));
    if ((r = run_match(c, nA, nB, c->stType, c->stDimPad, c->s.nndrEpsilon, c->stQueryOffset, false,
                       c->matches.as<fm3d_dmatch>(), cnt + 0, guided ? &gate : nullptr, c->s.crossCheck)))
        return r;
    // the stage boundaries (ev[3]: match + NNDR done, ev[5]: DLT done) only when asked for: a timed
    // event between two launches costs the C2 step 4-10 us of gap (rocprofv3 trace, round 5);
    // FM3D_STAGE_EVENTS=0 leaves only the step's own ev[2] / ev[1]
    c->stageEv = stage_events();
    if (c->stageEv) HIPCHK(c, hipEventRecord(ev[3], c->stream));
    return FM3D_OK;
}

int front_dlt(fm3d_ctx* c) {
    const int nA = c->stNA;
    int r;
    hipEvent_t* ev = c->ev;
    int* cnt = c->pcnt.as<int>();
    // a4, a5: triangulate (matches are device resident; K <= nA)
    HIPCHK(c, c->triPts.ensure((size_t)(nA + 1) * 3 * sizeof(double)));
    HIPCHK(c, c->triMask.ensure((size_t)(nA + 1) * sizeof(int)));
    HIPCHK(c, c->pts.ensure((size_t)(nA + 1) * 3 * sizeof(double)));
    HIPCHK(c, c->srcIdx.ensure((size_t)(nA + 1) * sizeof(int)));
    fm3d::TriParams tp{};
    tp.cam = c->cam;
    std::memcpy(tp.g12, c->g12, sizeof(tp.g12));
    tp.zmin = c->s.zThresholdMin;
    tp.zmax = c->s.zThresholdMax;
    tp.kp1 = c->kp1.as<fm3d_point2f>();
    tp.kp2 = c->kp2.as<fm3d_point2f>();
    tp.matches = c->matches.as<fm3d_dmatch>();
    tp.K = nA;
    tp.Kdev = cnt + 0;
    tp.queryOffset = c->stQueryOffset;
    tp.pts = c->triPts.as<double>();
    tp.mask = c->triMask.as<int>();
    tp.mask8 = nullptr;
    tp.dltSolver = c->s.dltSolver;
    {   // DLT with the inliers' compaction fused (launch_triangulate_compact)
        fm3d::LookBack lb;
        if ((r = make_lookback(c, fm3d::triangulate_compact_blocks(nA), &lb))) return r;
        fm3d::launch_triangulate_compact(tp, c->pts.as<double>(), c->srcIdx.as<int>(), cnt + 1, lb, c->stream,
                                         c->frontHostCnt);
    }
    HIPCHK(c, hipGetLastError());
    if (c->stageEv) HIPCHK(c, hipEventRecord(ev[5], c->stream));
    return FM3D_OK;
}

int pipeline_front(fm3d_ctx* c) {
    int r;
    if ((r = front_match(c))) return r;
    return front_dlt(c);
}

// the survivor records of c's pair (after its LM normals, in stream order), then one D2H of the
// counts, the pair's LM counters and the LM launch's counters (lmStat: the launching context's)
int enqueue_epilogue(fm3d_ctx* c, fm3d_record* out, const void* lmStat) {
    const int nA = c->stNA;
    int* cnt = c->pcnt.as<int>();
    HIPCHK(c, c->recTmp.ensure((size_t)(nA + 1) * sizeof(fm3d_record)));
    HIPCHK(c, c->recFlag.ensure((size_t)(nA + 1) * sizeof(int)));
    if (!out) {
        HIPCHK(c, c->records.ensure((size_t)(nA + 1) * sizeof(fm3d_record)));
        out = c->records.as<fm3d_record>();
    }
    c->pendOut = out;
    fm3d::launch_make_records(c->matches.as<fm3d_dmatch>(), c->srcIdx.as<int>(), nA, cnt + 1, c->pts.as<double>(),
                              c->lmNormals.as<double>(), c->lmStatus.as<int>(), c->recTmp.as<fm3d_record>(),
                              c->recFlag.as<int>(), c->stream);
    fm3d::launch_compact_records(c->recTmp.as<fm3d_record>(), c->recFlag.as<int>(), nA, cnt + 1, out, cnt + 2,
                                 c->scanTmp.p, c->stream);
    HIPCHK(c, hipGetLastError());
    HIPCHK(c, c->hSmall.ensure(sizeof(PipeSmall)));
    PipeSmall* hs = c->hSmall.as<PipeSmall>();
    HIPCHK(c, hipMemcpyAsync(hs->cnt, cnt, sizeof(hs->cnt) + sizeof(hs->prob), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipMemcpyAsync(hs->lm, lmStat, sizeof(hs->lm), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipEventRecord(c->ev[1], c->stream));
    return FM3D_OK;
}

// the whole path on the staged inputs, queued on the context stream: front half, LM normals over
// the device-counted inliers (a6-a15; the pyramids were built at staging: images are inputs of the
// path), survivor records (compacted into out, or the internal buffer), then one D2H of the counts
// and the LM counters into pinned memory.  Nothing here waits for the device.
int enqueue_full(fm3d_ctx* c, fm3d_record* out, fm3d_lm_stats* ls) {
    int r;
    if ((r = pipeline_front(c))) return r;
    if ((r = run_lm(c, c->stNA, c->pcnt.as<int>() + 1, ls, c->ev[6], c->ev[7]))) return r;
    return enqueue_epilogue(c, out, c->lmStat.p);
}

// the leader's pair with its members' queued front halves: ONE LM launch over all these pairs'
// points on the leader's stream (after every member's front half), then each pair's records on
// its own stream
int enqueue_linked(fm3d_ctx* c, const std::vector<fm3d_ctx*>& ms, fm3d_lm_stats* ls) {
    int r;
    if ((r = pipeline_front(c))) return r;
    std::vector<LMSrc> src;
    for (fm3d_ctx* m : ms) {
        HIPCHK(c, hipStreamWaitEvent(c->stream, m->evFront, 0));
        src.push_back({m, m->stNA, m->pcnt.as<int>() + 1});
        HIPCHK(c, hipEventRecord(m->ev[6], c->stream));
    }
    src.push_back({c, c->stNA, c->pcnt.as<int>() + 1});
    if ((r = run_lm_multi(c, src.data(), (int)src.size(), ls, c->ev[6], c->ev[7]))) return r;
    // each member gets its own copy of the launch's counters (on this stream, before evLm): the
    // leader's next run_lm_multi resets c->lmStat, possibly before a member's epilogue has read it
    for (fm3d_ctx* m : ms) {
        HIPCHK(m, m->lmStat.ensure(256));
        HIPCHK(c, hipMemcpyAsync(m->lmStat.p, c->lmStat.p, sizeof(PipeSmall::lm), hipMemcpyDeviceToDevice, c->stream));
    }
    HIPCHK(c, hipEventRecord(c->evLm, c->stream));
    if ((r = enqueue_epilogue(c, c->subOut, c->lmStat.p))) return r;
    for (fm3d_ctx* m : ms) {
        HIPCHK(c, hipEventRecord(m->ev[7], c->stream));
        m->subLm = *ls;
        m->lmGroups = c->lmGroups;
        m->wallKhz = c->wallKhz;
        hipSetDevice(m->device);
        HIPCHK(m, hipStreamWaitEvent(m->stream, c->evLm, 0));
        if ((r = enqueue_epilogue(m, m->subOut, m->lmStat.p))) return r;
        m->frontOnly = false;
    }
    return FM3D_OK;
}

// after the stream ran enqueue_full: guards, counts and stats (t0: the event the total starts at)
int finalize_full(fm3d_ctx* c, const fm3d_lm_stats& ls, hipEvent_t t0, bool staged_in_step, int* nKept,
                  fm3d_pipeline_stats* stats) {
    hipEvent_t* ev = c->ev;
    HIPCHK(c, hipStreamSynchronize(c->stream));
    const PipeSmall* hs = c->hSmall.as<PipeSmall>();
    const int K = hs->cnt[0], P = hs->cnt[1], kept = hs->cnt[2];
    c->stK = K;
    c->stP = P;
    // the LM watchdog (maxIter / FM3D_LM_MAX_SECONDS) leaves points in kLMRunning: an error, not drops
    if (hs->lm[2]) return fail(c, FM3D_ERR_HIP, "LM kernel iteration guard tripped (internal error)");
    if (c->s.strictNanExit && P > 0) {  // reference exit(-6) on a NaN plane hit (:465-469)
        std::vector<int> st(P);
        HIPCHK(c, hipMemcpy(st.data(), c->lmStatus.p, (size_t)P * sizeof(int), hipMemcpyDeviceToHost));
        for (int i = 0; i < P; i++)
            if (st[i] == FM3D_ST_NAN_PLANE)
                return fail(c, FM3D_ERR_NAN_PLANE, "projectPointToPlane hit NaN (reference: exit(-6))");
    }
    if (nKept) *nKept = kept;
    if (stats) {
        std::memset(stats, 0, sizeof(*stats));
        stats->queries = c->stNA;
        stats->trains = c->stNB;
        stats->matches = K;
        stats->inliers = P;
        stats->kept = kept;
        float ms;
        stage_times(c, stats);
        ms = 0;
        if (staged_in_step) hipEventElapsedTime(&ms, ev[8], ev[2]);
        stats->pyramid_ms = ms;  // the inputs' H2D + pyramids (fm3d_pipeline_submit only)
        ms = 0;
        hipEventElapsedTime(&ms, ev[6], ev[7]);
        stats->lm_ms = ms;
        hipEventElapsedTime(&ms, t0, ev[1]);
        stats->total_ms = ms;
        stats->lm = ls;
        stats->lm.points_in = P;
        stats->lm.points_kept = kept;
        stats->lm.evaluations = (int64_t)hs->prob[0];  // this pair's (a launch may hold two)
        stats->lm.pixel_evaluations = (int64_t)hs->prob[1];
        stats->lm.kernel_ms = stats->lm_ms;
        fill_lm_cycles(c, hs->lm, &stats->lm);
    }
    return FM3D_OK;
}
}  // namespace
extern "C" {

int fm3d_pipeline_upload(fm3d_ctx* c, const void* descA, int nA, const void* descB, int nB, int dim, int type,
                         const fm3d_point2f* kpts1, const fm3d_point2f* kpts2, const uint8_t* img1, const uint8_t* img2,
                         int width, int height, int queryOffset) {
    if (!c) return FM3D_ERR_INVALID;
    PENDING_CHECK(c);
    hipSetDevice(c->device);
    int r;
    if ((r = stage_pipeline(c, descA, nA, descB, nB, dim, type, kpts1, kpts2, img1, img2, width, height, queryOffset)))
        return r;
    HIPCHK(c, hipStreamSynchronize(c->stream));
    return FM3D_OK;
}

int fm3d_pipeline_run(fm3d_ctx* c, fm3d_record* recordsDev, int* nKept, fm3d_pipeline_stats* stats) {
    if (!c || !c->staged) return fail(c, FM3D_ERR_INVALID, "fm3d_pipeline_upload not called");
    PENDING_CHECK(c);
    hipSetDevice(c->device);
    fm3d_lm_stats ls{};
    int r;
    if ((r = enqueue_full(c, recordsDev, &ls))) return r;
    return finalize_full(c, ls, c->ev[2], false, nKept, stats);
}

}  // extern "C"
namespace {
// one frame pair staged and queued on c's stream (records into out: device, or null = internal);
// a link member queues its front half only, a leader joins its queued members' pairs
int submit_impl(fm3d_ctx* c, const void* descA, int nA, const void* descB, int nB, int dim, int type,
                const fm3d_point2f* kpts1, const fm3d_point2f* kpts2, const uint8_t* img1, const uint8_t* img2,
                int width, int height, int queryOffset, fm3d_record* out) {
    PENDING_CHECK(c);
    hipSetDevice(c->device);
    HIPCHK(c, hipEventRecord(c->ev[8], c->stream));
    int r;
    if ((r = stage_pipeline(c, descA, nA, descB, nB, dim, type, kpts1, kpts2, img1, img2, width, height, queryOffset)))
        return r;
    c->subLm = fm3d_lm_stats{};
    c->subOut = out;
    if (c->linkLeader) {  // member: the front half now, the LM with the leader's next pair
        if ((r = pipeline_front(c))) return r;
        HIPCHK(c, hipEventRecord(c->evFront, c->stream));
        c->frontOnly = true;
    } else if (!c->linkMembers.empty()) {
        std::vector<fm3d_ctx*> ms;  // the members with a pair queued since this leader's last launch
        for (fm3d_ctx* m : c->linkMembers)
            if (m->frontOnly) ms.push_back(m);
        if ((r = ms.empty() ? enqueue_full(c, out, &c->subLm) : enqueue_linked(c, ms, &c->subLm))) return r;
    } else {
        if ((r = enqueue_full(c, out, &c->subLm))) return r;
    }
    c->pending = true;
    return FM3D_OK;
}

// a member whose leader took no pair since its submit: its LM alone, on its own stream
int flush_member(fm3d_ctx* c) {
    if (!c->frontOnly) return FM3D_OK;
    hipSetDevice(c->device);
    int r;
    if ((r = run_lm(c, c->stNA, c->pcnt.as<int>() + 1, &c->subLm, c->ev[6], c->ev[7]))) return r;
    if ((r = enqueue_epilogue(c, c->subOut, c->lmStat.p))) return r;
    c->frontOnly = false;
    return FM3D_OK;
}
}  // namespace
extern "C" {

int fm3d_pipeline_submit(fm3d_ctx* c, const void* descA, int nA, const void* descB, int nB, int dim, int type,
                         const fm3d_point2f* kpts1, const fm3d_point2f* kpts2, const uint8_t* img1, const uint8_t* img2,
                         int width, int height, int queryOffset) {
    if (!c) return FM3D_ERR_INVALID;
    return submit_impl(c, descA, nA, descB, nB, dim, type, kpts1, kpts2, img1, img2, width, height, queryOffset,
                       nullptr);
}

int fm3d_pipeline_link(fm3d_ctx* member, fm3d_ctx* leader) {
    if (!member || !leader || member == leader) return FM3D_ERR_INVALID;
    if (member->pending || leader->pending) return fail(member, FM3D_ERR_INVALID, "a submitted frame pair is pending");
    if (member->linkLeader || !member->linkMembers.empty() || leader->linkLeader)
        return fail(member, FM3D_ERR_INVALID, "a context is linked already");
    if ((int)leader->linkMembers.size() + 1 >= fm3d::kLMMaxProblems)
        return fail(member, FM3D_ERR_INVALID, "a leader takes at most 3 members");
    if (member->device != leader->device) return fail(member, FM3D_ERR_INVALID, "linked contexts need one device");
    member->linkLeader = leader;
    leader->linkMembers.push_back(member);
    return FM3D_OK;
}

int fm3d_pipeline_wait(fm3d_ctx* c, fm3d_record* out, int cap, int* nKept, fm3d_pipeline_stats* stats) {
    if (!c) return FM3D_ERR_INVALID;
    if (!c->pending) return fail(c, FM3D_ERR_INVALID, "no frame pair submitted (fm3d_pipeline_submit)");
    if (c->pendingDlt) return fail(c, FM3D_ERR_INVALID, "a front half is pending: fm3d_pipeline_wait_dlt");
    if (c->pendingNcc) return fail(c, FM3D_ERR_INVALID, "an NCC scoring is pending: fm3d_pipeline_wait_ncc");
    hipSetDevice(c->device);
    int r;
    if ((r = flush_member(c))) return r;
    c->pending = false;
    int kept = 0;
    if ((r = finalize_full(c, c->subLm, c->ev[8], true, &kept, stats))) return r;
    if (out && kept > cap) return fail(c, FM3D_ERR_INVALID, "record buffer too small");
    if (out && kept)
        HIPCHK(c, hipMemcpy(out, c->pendOut, (size_t)kept * sizeof(fm3d_record), hipMemcpyDeviceToHost));
    if (nKept) *nKept = kept;
    return FM3D_OK;
}

}  // extern "C"

// ---- internal entry points of the multi-GPU host (fm3d_mgpu.cpp; fm3d_internal.h, not the C ABI)
int fm3d_internal_submit_to(fm3d_ctx* c, const void* descA, int nA, const void* descB, int nB, int dim, int type,
                            const fm3d_point2f* kpts1, const fm3d_point2f* kpts2, const uint8_t* img1,
                            const uint8_t* img2, int width, int height, fm3d_record* recordsDev) {
    if (!c) return FM3D_ERR_INVALID;
    return submit_impl(c, descA, nA, descB, nB, dim, type, kpts1, kpts2, img1, img2, width, height, 0, recordsDev);
}

int fm3d_internal_flush(fm3d_ctx* c) { return c ? flush_member(c) : FM3D_ERR_INVALID; }
bool fm3d_internal_front_only(const fm3d_ctx* c) { return c && c->frontOnly; }

int fm3d_internal_enqueue(fm3d_ctx* c, fm3d_record* recordsDev) {
    if (!c || !c->staged) return fail(c, FM3D_ERR_INVALID, "fm3d_pipeline_upload not called");
    PENDING_CHECK(c);
    hipSetDevice(c->device);
    HIPCHK(c, hipEventRecord(c->ev[8], c->stream));
    c->subLm = fm3d_lm_stats{};
    int r;
    if ((r = enqueue_full(c, recordsDev, &c->subLm))) return r;
    c->pending = true;
    return FM3D_OK;
}

int fm3d_internal_finish(fm3d_ctx* c, int* nKept, fm3d_pipeline_stats* stats) {
    if (!c || !c->pending) return fail(c, FM3D_ERR_INVALID, "nothing pending");
    hipSetDevice(c->device);
    c->pending = false;
    return finalize_full(c, c->subLm, c->ev[8], true, nKept, stats);
}

const int* fm3d_internal_kept_dev(fm3d_ctx* c) { return c->pcnt.as<int>() + 2; }
hipStream_t fm3d_internal_stream(fm3d_ctx* c) { return c->stream; }
// the device memory one context may take: its largest LM launch's slabs (every CU filled) plus the
// per-pair buffers of nA queries against nB train rows of dim elements (a conservative estimate of
// what the pipeline's DevBufs grow to: descriptors, their u8 / unpacked copies, per-query match,
// triangulation, LM and record arrays, the matchers' part lists, pyramids)
int fm3d_internal_memory_need(fm3d_ctx* c, int64_t nA, int64_t nB, int dim, int type, int width, int height,
                              size_t* bytes) {
    hipSetDevice(c->device);
    int r;
    if ((r = ensure_offsets(c))) return r;
    const bool tree = c->s.lmReduction != 0;
    const int slots = fm3d::kLM2Slots + (tree ? 1 : 0);
    const void* kptr = tree ? reinterpret_cast<const void*>(fm3d::lm2_kernel<true, true>)
                            : reinterpret_cast<const void*>(fm3d::lm2_kernel<true, false>);
    long groups = 0;
    if ((r = lm_groups(c, kptr, slots, -1, &groups))) return r;
    const size_t ents = (size_t)c->nOffPad * slots;
    size_t need = ents * (2 * sizeof(double) + 5 * 4) * groups + 32768;
    const size_t rowIn = type == FM3D_DESC_F32 ? (size_t)dim * 4 : (size_t)dim;
    const size_t rowWork = 256 + (type == FM3D_DESC_F32 ? (size_t)dim * 4 : 0);  // u8 / unpacked / pair copies
    need += (size_t)(nA + nB) * (rowIn + rowWork) + (size_t)nB * 64;
    if (c->s.guidedMatchPx > 0.) need += (size_t)nA * 16 + (size_t)nB * 8;  // the gate's lines and (u, v)
    // the cross-check's reverse search: unpacked / pair copies of both sides, row constants, the
    // train rows' top-2 lists and 16 parts of them
    if (c->s.crossCheck != 0) need += (size_t)(nA + nB) * (rowWork + 8) + (size_t)nB * (24 + 16 * 16);
    need += (size_t)nA * 1536;  // per query: top-2 lists + 16 parts, matches, points, masks, LM arrays, records
    need += (size_t)width * height * 4 + ((size_t)16 << 20);  // pyramids with guards, small buffers
    *bytes = need;
    return FM3D_OK;
}

int fm3d_internal_prepare(fm3d_ctx* c) {  // the device count buffer, before a collective names it
    hipSetDevice(c->device);
    HIPCHK(c, c->pcnt.ensure(64));
    return FM3D_OK;
}

namespace {
// the staged pair's front half with its counts written to page-locked memory by the DLT kernel
int queue_front_counts(fm3d_ctx* c) {
    int r;
    HIPCHK(c, c->hSmall.ensure(sizeof(PipeSmall)));
    PipeSmall* hs = c->hSmall.as<PipeSmall>();
    // the counts reach the page-locked buffer from the DLT kernel itself (no copy launch)
    void* dcnt = nullptr;
    HIPCHK(c, hipHostGetDevicePointer(&dcnt, hs->cnt, 0));
    c->frontHostCnt = (int*)dcnt;
    r = pipeline_front(c);
    c->frontHostCnt = nullptr;
    if (r) return r;
    HIPCHK(c, hipEventRecord(c->ev[1], c->stream));
    return FM3D_OK;
}

// after ev[1] of queue_front_counts: the counts it left in page-locked memory, and the stage times
void report_front_counts(fm3d_ctx* c, int* nInliers, fm3d_pipeline_stats* stats) {
    const PipeSmall* hs = c->hSmall.as<PipeSmall>();
    const int K = hs->cnt[0], P = hs->cnt[1];
    c->stK = K;
    c->stP = P;
    if (nInliers) *nInliers = P;
    if (stats) {
        std::memset(stats, 0, sizeof(*stats));
        stats->queries = c->stNA;
        stats->trains = c->stNB;
        stats->matches = K;
        stats->inliers = P;
        float ms;
        stage_times(c, stats);
        hipEventElapsedTime(&ms, c->ev[2], c->ev[1]);
        stats->total_ms = ms;
    }
}

// after a speculative front half (stage_descriptors' speculate): when the pack kernel flagged an
// element that is not an integer in [0, 255], the float rows (still on the device) go through the
// float matchers and the front half runs again, as the non-speculative staging would have run it
int redo_float_front(fm3d_ctx* c) {
    if (!c->specU8) return FM3D_OK;
    c->specU8 = false;
    const int flag = *c->hFlag.as<int>();
    if (flag == 0) return FM3D_OK;
    if (flag < 0) return fail(c, FM3D_ERR_HIP, "the float rows' flag never arrived");
    std::swap(c->A, c->A8);
    std::swap(c->B, c->B8);
    c->stType = FM3D_DESC_F32;
    c->stDimPad = c->stDim;
    int r;
    if ((r = queue_front_counts(c))) return r;
    HIPCHK(c, hipEventSynchronize(c->ev[1]));
    return FM3D_OK;
}
}  // namespace
extern "C" {

int fm3d_pipeline_submit_dlt(fm3d_ctx* c) {
    if (!c || !c->staged) return fail(c, FM3D_ERR_INVALID, "fm3d_pipeline_upload not called");
    PENDING_CHECK(c);
    hipSetDevice(c->device);
    int r;
    if ((r = queue_front_counts(c))) return r;
    c->pending = true;
    c->pendingDlt = true;
    return FM3D_OK;
}

int fm3d_pipeline_submit_dlt_pair(fm3d_ctx* c, const void* descA, int nA, const void* descB, int nB, int dim,
                                  int type, const fm3d_point2f* kpts1, const fm3d_point2f* kpts2, int queryOffset) {
    if (!c) return FM3D_ERR_INVALID;
    PENDING_CHECK(c);
    hipSetDevice(c->device);
    int r;
    if ((r = stage_pipeline(c, descA, nA, descB, nB, dim, type, kpts1, kpts2, nullptr, nullptr, 0, 0, queryOffset,
                            true)))
        return r;
    if ((r = queue_front_counts(c))) return r;
    c->pending = true;
    c->pendingDlt = true;
    return FM3D_OK;
}

int fm3d_pipeline_wait_dlt(fm3d_ctx* c, int* nInliers, fm3d_pipeline_stats* stats) {
    if (!c) return FM3D_ERR_INVALID;
    if (!c->pendingDlt) return fail(c, FM3D_ERR_INVALID, "no front half submitted (fm3d_pipeline_submit_dlt)");
    hipSetDevice(c->device);
    hipEvent_t* ev = c->ev;
    c->pending = false;
    c->pendingDlt = false;
    HIPCHK(c, hipEventSynchronize(ev[1]));
    int r;
    if ((r = redo_float_front(c))) return r;
    report_front_counts(c, nInliers, stats);
    return FM3D_OK;
}

int fm3d_pipeline_run_dlt(fm3d_ctx* c, int* nInliers, fm3d_pipeline_stats* stats) {
    int r;
    if ((r = fm3d_pipeline_submit_dlt(c))) return r;
    return fm3d_pipeline_wait_dlt(c, nInliers, stats);
}

}  // extern "C"
namespace {
// fm3d_pipeline_run(_dlt)_verified's argument rules, before any launch
int check_verified(fm3d_ctx* c, const fm3d_verify_opts* o, const fm3d_verify_report* rep) {
    if (!c || !o || !rep) return fail(c, FM3D_ERR_INVALID, "null argument");
    if (!c->staged) return fail(c, FM3D_ERR_INVALID, "fm3d_pipeline_upload not called");
    PENDING_CHECK(c);
    if (o->hypotheses < 1) return fail(c, FM3D_ERR_INVALID, "hypotheses must be >= 1");
    if (o->refineIters < 0 || o->refineIters > 16) return fail(c, FM3D_ERR_INVALID, "refineIters must be in 0 .. 16");
    if (!good_max_px(o->maxPx)) return fail(c, FM3D_ERR_INVALID, "maxPx must be finite and > 0");
    if (o->reserved != 0) return fail(c, FM3D_ERR_INVALID, "reserved must be 0");
    if (o->poseFromModel != 0 && o->poseFromModel != 1) return fail(c, FM3D_ERR_INVALID, "poseFromModel must be 0 or 1");
    if (o->poseFromModel) {
        if (!good_max_px(o->baseline)) return fail(c, FM3D_ERR_INVALID, "baseline must be finite and > 0");
        if (c->s.guidedMatchPx > 0.)
            return fail(c, FM3D_ERR_INVALID,
                        "poseFromModel with guidedMatchPx > 0: the gate needs the pose this call is about to find");
    }
    if (c->stQueryOffset != 0)
        return fail(c, FM3D_ERR_UNSUPPORTED, "a staged queryOffset != 0: a share sees only its own matches");
    if (o->hypotheses > fm3d::kVerifyMaxHyps) return fail(c, FM3D_ERR_UNSUPPORTED, "more than 2^20 hypotheses");
    return FM3D_OK;
}

// The match half, one wait for K, the verification of those matches where they lie (verify_staged:
// its own wait), and the pose's installation.  *go: a model (and, when asked for, its pose) exists, the
// verified matches and their count are where front_dlt reads them.  Otherwise nothing further may be
// launched on this pair: its counts are zero on both sides.
int front_verified(fm3d_ctx* c, const fm3d_verify_opts* o, fm3d_verify_report* rep, bool* go) {
    int r;
    *go = false;
    std::memset(rep, 0, sizeof(*rep));
    rep->best = -1;
    if ((r = front_match(c))) return r;
    int* cnt = c->pcnt.as<int>();
    int K = 0;
    HIPCHK(c, hipMemcpyAsync(&K, cnt + 0, sizeof(int), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    if (K < 0 || K > c->stNA) return fail(c, FM3D_ERR_HIP, "match count out of range");
    rep->matches = K;
    if (K >= 8) {  // fewer: no sample exists, every hypothesis is invalid
        bool havePose = false;
        double g[16];
        if ((r = verify_staged(c, o, K, rep, &havePose, g))) return r;
        *go = rep->best >= 0 && (!o->poseFromModel || havePose);
        if (*go && o->poseFromModel) {
            install_g12(c, g);
            rep->poseInstalled = 1;
        }
    }
    std::memcpy(rep->g12, c->g12, sizeof(rep->g12));
    if (!*go) {
        rep->verified = 0;
        for (int k = 0; k < 4; k++) rep->votes[k] = 0;
        c->stK = c->stP = 0;
        HIPCHK(c, hipMemsetAsync(cnt, 0, 4 * sizeof(int), c->stream));
        HIPCHK(c, hipStreamSynchronize(c->stream));
    }
    return FM3D_OK;
}

void empty_stats(const fm3d_ctx* c, fm3d_pipeline_stats* stats) {
    if (!stats) return;
    std::memset(stats, 0, sizeof(*stats));
    stats->queries = c->stNA;
    stats->trains = c->stNB;
}
}  // namespace
extern "C" {

int fm3d_pipeline_run_verified(fm3d_ctx* c, const fm3d_verify_opts* o, fm3d_record* recordsDev, int* nKept,
                               fm3d_pipeline_stats* stats, fm3d_verify_report* rep) {
    int r;
    if ((r = check_verified(c, o, rep))) return r;
    hipSetDevice(c->device);
    bool go;
    if ((r = front_verified(c, o, rep, &go))) return r;
    if (!go) {
        if (nKept) *nKept = 0;
        empty_stats(c, stats);
        return FM3D_OK;
    }
    fm3d_lm_stats ls{};
    if ((r = front_dlt(c))) return r;
    if ((r = run_lm(c, c->stNA, c->pcnt.as<int>() + 1, &ls, c->ev[6], c->ev[7]))) return r;
    if ((r = enqueue_epilogue(c, recordsDev, c->lmStat.p))) return r;
    return finalize_full(c, ls, c->ev[2], false, nKept, stats);
}

int fm3d_pipeline_run_dlt_verified(fm3d_ctx* c, const fm3d_verify_opts* o, int* nInliers, fm3d_pipeline_stats* stats,
                                   fm3d_verify_report* rep) {
    int r;
    if ((r = check_verified(c, o, rep))) return r;
    hipSetDevice(c->device);
    bool go;
    if ((r = front_verified(c, o, rep, &go))) return r;
    if (!go) {
        if (nInliers) *nInliers = 0;
        empty_stats(c, stats);
        return FM3D_OK;
    }
    // as queue_front_counts: the DLT kernel stores (K, P) in page-locked memory itself
    HIPCHK(c, c->hSmall.ensure(sizeof(PipeSmall)));
    void* dcnt = nullptr;
    HIPCHK(c, hipHostGetDevicePointer(&dcnt, c->hSmall.as<PipeSmall>()->cnt, 0));
    c->frontHostCnt = (int*)dcnt;
    r = front_dlt(c);
    c->frontHostCnt = nullptr;
    if (r) return r;
    HIPCHK(c, hipEventRecord(c->ev[1], c->stream));
    HIPCHK(c, hipEventSynchronize(c->ev[1]));
    report_front_counts(c, nInliers, stats);
    return FM3D_OK;
}

int fm3d_pipeline_submit_ncc(fm3d_ctx* c, int Hphi, int Htheta, double span) {
    if (!c || !c->staged) return fail(c, FM3D_ERR_INVALID, "fm3d_pipeline_upload not called");
    PENDING_CHECK(c);
    if (Hphi <= 0 || Htheta <= 0 || Hphi * Htheta > 32) return fail(c, FM3D_ERR_INVALID, "1 <= Hphi * Htheta <= 32");
    if (!c->haveG12) return fail(c, FM3D_ERR_INVALID, "fm3d_set_g12 / fm3d_setg12 not called");
    hipSetDevice(c->device);
    hipEvent_t* ev = c->ev;
    int r;
    c->nccP = 0;
    if ((r = pipeline_front(c))) return r;
    const int nA = c->stNA;
    const int H = Hphi * Htheta;
    HIPCHK(c, hipEventRecord(ev[6], c->stream));
    if (nA > 0) {
        if ((r = ensure_offsets(c))) return r;
        HIPCHK(c, c->nccS.ensure((size_t)nA * H * sizeof(double)));
        HIPCHK(c, c->nccN.ensure((size_t)nA * 3 * sizeof(double)));
        HIPCHK(c, c->nccB.ensure((size_t)nA * sizeof(int)));
        fm3d::NccParams p{};
        p.points = c->pts.as<double>();
        p.P = nA;  // the bound; the inlier count is on the device
        p.Pdev = c->pcnt.as<int>() + 1;
        p.cam = lm_camera(c->cam);  // the kernel's bit-pattern isPixelGood (fm3d_ncc.hip ncc_geometry)
        std::memcpy(p.R2, c->R2, sizeof(p.R2));
        std::memcpy(p.t2, c->t2, sizeof(p.t2));
        p.img1 = c->pyr1[0].as<uint8_t>();
        p.img2 = c->pyr2[0].as<uint8_t>();
        p.w = c->lw[0];
        p.h = c->lh[0];
        p.offsets = c->offsets.as<int2>();
        p.nOff = c->nOff;
        p.nOffPad = c->nOffPad;
        p.boundW = c->s.boundWidth;
        p.boundH = c->s.boundHeight;
        p.cmax = (int)(2 * c->s.zThresholdMax);
        p.Hphi = Hphi;
        p.Htheta = Htheta;
        p.span = span;
        p.scores = c->nccS.as<double>();
        p.normals = c->nccN.as<double>();
        p.best = c->nccB.as<int>();
        fm3d::launch_ncc_hypotheses(p, c->stream);
        HIPCHK(c, hipGetLastError());
    }
    HIPCHK(c, hipEventRecord(ev[7], c->stream));
    HIPCHK(c, c->hSmall.ensure(sizeof(PipeSmall)));
    PipeSmall* hs = c->hSmall.as<PipeSmall>();
    HIPCHK(c, hipMemcpyAsync(hs->cnt, c->pcnt.p, sizeof(hs->cnt), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipEventRecord(ev[1], c->stream));
    c->pending = true;
    c->pendingNcc = true;
    c->nccHPending = H;
    return FM3D_OK;
}

int fm3d_pipeline_wait_ncc(fm3d_ctx* c, int* nPoints, fm3d_pipeline_stats* stats) {
    if (!c) return FM3D_ERR_INVALID;
    if (!c->pendingNcc) return fail(c, FM3D_ERR_INVALID, "no NCC scoring submitted (fm3d_pipeline_submit_ncc)");
    hipSetDevice(c->device);
    hipEvent_t* ev = c->ev;
    c->pending = false;
    c->pendingNcc = false;
    HIPCHK(c, hipEventSynchronize(ev[1]));
    const PipeSmall* hs = c->hSmall.as<PipeSmall>();
    const int K = hs->cnt[0], P = hs->cnt[1];
    c->stK = K;
    c->stP = P;
    c->nccH = c->nccHPending;
    c->nccP = P;  // the score rows fm3d_pipeline_ncc_download returns (set only by a successful run)
    if (nPoints) *nPoints = P;
    if (stats) {
        std::memset(stats, 0, sizeof(*stats));
        stats->queries = c->stNA;
        stats->trains = c->stNB;
        stats->matches = K;
        stats->inliers = P;
        stats->kept = P;
        float ms;
        stage_times(c, stats);
        hipEventElapsedTime(&ms, ev[6], ev[7]);
        stats->lm_ms = ms;  // the normal stage: here the NCC scoring
        hipEventElapsedTime(&ms, ev[2], ev[1]);
        stats->total_ms = ms;
    }
    return FM3D_OK;
}

int fm3d_pipeline_run_ncc(fm3d_ctx* c, int Hphi, int Htheta, double span, int* nPoints, fm3d_pipeline_stats* stats) {
    int r;
    if ((r = fm3d_pipeline_submit_ncc(c, Hphi, Htheta, span))) return r;
    return fm3d_pipeline_wait_ncc(c, nPoints, stats);
}

int fm3d_pipeline_ncc_download(fm3d_ctx* c, double* scores, double* normals, int32_t* best) {
    if (!c || !c->staged) return FM3D_ERR_INVALID;
    PENDING_CHECK(c);
    hipSetDevice(c->device);
    // the rows of the last successful fm3d_pipeline_run_ncc (a later run / run_dlt does not resize them)
    const size_t P = (size_t)c->nccP;
    if (P && scores) HIPCHK(c, hipMemcpy(scores, c->nccS.p, P * c->nccH * sizeof(double), hipMemcpyDeviceToHost));
    if (P && normals) HIPCHK(c, hipMemcpy(normals, c->nccN.p, P * 3 * sizeof(double), hipMemcpyDeviceToHost));
    if (P && best) HIPCHK(c, hipMemcpy(best, c->nccB.p, P * sizeof(int), hipMemcpyDeviceToHost));
    return FM3D_OK;
}

int fm3d_pipeline_dlt_download(fm3d_ctx* c, fm3d_dmatch* matches, double* points, int32_t* matchIdx) {
    if (!c || !c->staged) return FM3D_ERR_INVALID;
    PENDING_CHECK(c);
    hipSetDevice(c->device);
    if (matches && c->stK) HIPCHK(c, hipMemcpy(matches, c->matches.p, (size_t)c->stK * sizeof(fm3d_dmatch), hipMemcpyDeviceToHost));
    if (points && c->stP) HIPCHK(c, hipMemcpy(points, c->pts.p, (size_t)c->stP * 3 * sizeof(double), hipMemcpyDeviceToHost));
    if (matchIdx && c->stP) HIPCHK(c, hipMemcpy(matchIdx, c->srcIdx.p, (size_t)c->stP * sizeof(int), hipMemcpyDeviceToHost));
    return FM3D_OK;
}

int fm3d_records_download(fm3d_ctx* c, const fm3d_record* recordsDev, int n, fm3d_record* out) {
    if (!c || n < 0 || (n && !out)) return FM3D_ERR_INVALID;
    hipSetDevice(c->device);
    const void* src = recordsDev ? (const void*)recordsDev : c->records.p;
    if (n) HIPCHK(c, hipMemcpy(out, src, (size_t)n * sizeof(fm3d_record), hipMemcpyDeviceToHost));
    return FM3D_OK;
}

int fm3d_features_frames(fm3d_ctx* c, const double* points, const double* normals, int P, double* frames) {
    if (!c || P < 0 || (P && (!points || !normals || !frames))) return FM3D_ERR_INVALID;
    if (P == 0) return FM3D_OK;
    hipSetDevice(c->device);
    double g[3];
    int r;
    if ((r = fm3d_gravity(&c->s, g))) return fail(c, r, "gravity: singular rodriguesIC rotation");
    DevBuf a, b, f;
    HIPCHK(c, a.ensure((size_t)P * 3 * sizeof(double)));
    HIPCHK(c, b.ensure((size_t)P * 3 * sizeof(double)));
    HIPCHK(c, f.ensure((size_t)P * 16 * sizeof(double)));
    HIPCHK(c, hipMemcpyAsync(a.p, points, (size_t)P * 3 * sizeof(double), hipMemcpyHostToDevice, c->stream));
    HIPCHK(c, hipMemcpyAsync(b.p, normals, (size_t)P * 3 * sizeof(double), hipMemcpyHostToDevice, c->stream));
    fm3d::launch_features_frames(a.as<double>(), b.as<double>(), P, g, f.as<double>(), c->stream);
    HIPCHK(c, hipGetLastError());
    HIPCHK(c, hipMemcpyAsync(frames, f.p, (size_t)P * 16 * sizeof(double), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    return FM3D_OK;
}

int fm3d_export_patches(fm3d_ctx* c, const double* frames, int P, uint8_t* patches, double* imagePoints) {
    if (!c || P < 0 || (P && (!frames || !patches))) return FM3D_ERR_INVALID;
    if (c->pyr1.empty()) return fail(c, FM3D_ERR_INVALID, "fm3d_set_images not called");
    const int size = fm3d_patch_size(&c->s);
    if (size <= 0) return fail(c, FM3D_ERR_INVALID, "patch size <= 0 (Neighborhoods.epsilon / cmPerPixel)");
    if (P == 0) return FM3D_OK;
    hipSetDevice(c->device);
    const size_t per = (size_t)size * size;
    DevBuf f, rt, out, pts;
    HIPCHK(c, f.ensure((size_t)P * 16 * sizeof(double)));
    HIPCHK(c, rt.ensure((size_t)P * 12 * sizeof(double)));
    HIPCHK(c, out.ensure((size_t)P * per));
    if (imagePoints) HIPCHK(c, pts.ensure((size_t)P * per * 2 * sizeof(double)));
    HIPCHK(c, hipMemcpyAsync(f.p, frames, (size_t)P * 16 * sizeof(double), hipMemcpyHostToDevice, c->stream));
    fm3d::launch_export_patches(f.as<double>(), P, size, c->s.neighEpsilon, c->s.cmPerPixel * 0.01, c->cam,
                                c->pyr1[0].as<uint8_t>(), c->lw[0], c->lh[0], rt.as<double>(), out.as<uint8_t>(),
                                imagePoints ? pts.as<double>() : nullptr, c->stream);
    HIPCHK(c, hipGetLastError());
    HIPCHK(c, hipMemcpyAsync(patches, out.p, (size_t)P * per, hipMemcpyDeviceToHost, c->stream));
    if (imagePoints)
        HIPCHK(c, hipMemcpyAsync(imagePoints, pts.p, (size_t)P * per * 2 * sizeof(double), hipMemcpyDeviceToHost,
                                 c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    return FM3D_OK;
}

int fm3d_square_neighborhoods(fm3d_ctx* c, const double* frames, int P, double* out) {
    if (!c || P < 0 || (P && (!frames || !out))) return FM3D_ERR_INVALID;
    const int size = fm3d_patch_size(&c->s);
    if (size <= 0) return fail(c, FM3D_ERR_INVALID, "neighbourhood size <= 0 (Neighborhoods.epsilon / cmPerPixel)");
    if (P == 0) return FM3D_OK;
    hipSetDevice(c->device);
    // chunks of frames bound the device buffer (~512 MB of points); the copy of chunk k overlaps
    // nothing here -- the host buffer is the boundary
    const size_t perFrame = (size_t)size * size * 3 * sizeof(double);
    const int chunk = (int)std::max<size_t>(1, std::min<size_t>((size_t)P, ((size_t)512 << 20) / perFrame));
    DevBuf f, o;
    HIPCHK(c, f.ensure((size_t)chunk * 16 * sizeof(double)));
    HIPCHK(c, o.ensure((size_t)chunk * perFrame));
    for (int p0 = 0; p0 < P; p0 += chunk) {
        const int n = std::min(chunk, P - p0);
        HIPCHK(c, hipMemcpyAsync(f.p, frames + (size_t)16 * p0, (size_t)n * 16 * sizeof(double),
                                 hipMemcpyHostToDevice, c->stream));
        fm3d::launch_square_neighborhoods(f.as<double>(), n, size, c->s.neighEpsilon, c->s.cmPerPixel * 0.01,
                                          o.as<double>(), c->stream);
        HIPCHK(c, hipGetLastError());
        HIPCHK(c, hipMemcpyAsync(out + (size_t)p0 * size * size * 3, o.p, (size_t)n * perFrame,
                                 hipMemcpyDeviceToHost, c->stream));
        HIPCHK(c, hipStreamSynchronize(c->stream));
    }
    return FM3D_OK;
}

int fm3d_circular_neighborhoods(fm3d_ctx* c, const double* points, const double* normals, int P, double* out) {
    if (!c || P < 0 || (P && (!points || !out))) return FM3D_ERR_INVALID;
    if (c->s.neighMethod != 1) return fail(c, FM3D_ERR_INVALID, "Neighborhoods.method is not circular");
    const int T = c->s.neighThetas, Rn = c->s.neighRays;
    if (T <= 0 || Rn <= 0) return fail(c, FM3D_ERR_INVALID, "Neighborhoods.thetas / rays <= 0");
    if (P == 0) return FM3D_OK;
    hipSetDevice(c->device);
    // the constructor's lookup table (neighborhoodsgenerator.cpp:50-64), libm sin as the reference
    const double eps = c->s.neighEpsilon;
    const double rayIncrement = eps / Rn, thetaIncrement = 2 * M_PI / T;
    const int S = T * Rn;
    std::vector<double> lut((size_t)S * 3);
    for (int i = 1; i <= Rn; i++)
        for (int j = 0; j < T; j++) {
            const double t = j * thetaIncrement;
            double* e = &lut[3 * ((size_t)(i - 1) * T + j)];
            e[0] = (double)i * rayIncrement;
            e[1] = std::sin(t);
            e[2] = 2 * (std::sin(t / 2)) * (std::sin(t / 2));
        }
    // chunks of points bound the device buffer (~512 MB of samples)
    const size_t perPoint = (size_t)S * 3 * sizeof(double);
    const int chunk = (int)std::max<size_t>(1, std::min<size_t>((size_t)P, ((size_t)512 << 20) / perPoint));
    DevBuf L, X, N, O;
    HIPCHK(c, L.ensure(lut.size() * sizeof(double)));
    HIPCHK(c, X.ensure((size_t)chunk * 3 * sizeof(double)));
    if (normals) HIPCHK(c, N.ensure((size_t)chunk * 3 * sizeof(double)));
    HIPCHK(c, O.ensure((size_t)chunk * perPoint));
    HIPCHK(c, hipMemcpyAsync(L.p, lut.data(), lut.size() * sizeof(double), hipMemcpyHostToDevice, c->stream));
    for (int p0 = 0; p0 < P; p0 += chunk) {
        const int n = std::min(chunk, P - p0);
        HIPCHK(c, hipMemcpyAsync(X.p, points + (size_t)3 * p0, (size_t)n * 3 * sizeof(double), hipMemcpyHostToDevice,
                                 c->stream));
        if (normals)
            HIPCHK(c, hipMemcpyAsync(N.p, normals + (size_t)3 * p0, (size_t)n * 3 * sizeof(double),
                                     hipMemcpyHostToDevice, c->stream));
        fm3d::launch_circular_neighborhoods(X.as<double>(), normals ? N.as<double>() : nullptr, n, S, L.as<double>(),
                                            eps, O.as<double>(), c->stream);
        HIPCHK(c, hipGetLastError());
        HIPCHK(c, hipMemcpyAsync(out + (size_t)p0 * S * 3, O.p, (size_t)n * perPoint, hipMemcpyDeviceToHost,
                                 c->stream));
        HIPCHK(c, hipStreamSynchronize(c->stream));
    }
    return FM3D_OK;
}

int fm3d_ncc_hypotheses(fm3d_ctx* c, const double* points, int P, int Hphi, int Htheta, double span, double* scores,
                        double* normals, int32_t* best) {
    if (!c || P < 0 || Hphi <= 0 || Htheta <= 0 || Hphi * Htheta > 32 || (P && (!points || !scores || !normals || !best)))
        return FM3D_ERR_INVALID;
    if (c->pyr1.empty()) return fail(c, FM3D_ERR_INVALID, "fm3d_set_images (NormalOptimizer::setImages) not called");
    if (!c->haveG12) return fail(c, FM3D_ERR_INVALID, "fm3d_set_g12 / fm3d_setg12 not called");
    if (P == 0) return FM3D_OK;
    hipSetDevice(c->device);
    int r;
    if ((r = ensure_offsets(c))) return r;
    const int H = Hphi * Htheta;
    DevBuf X, S, N, B;
    HIPCHK(c, X.ensure((size_t)P * 3 * sizeof(double)));
    HIPCHK(c, S.ensure((size_t)P * H * sizeof(double)));
    HIPCHK(c, N.ensure((size_t)P * 3 * sizeof(double)));
    HIPCHK(c, B.ensure((size_t)P * sizeof(int)));
    HIPCHK(c, hipMemcpyAsync(X.p, points, (size_t)P * 3 * sizeof(double), hipMemcpyHostToDevice, c->stream));
    fm3d::NccParams p{};
    p.points = X.as<double>();
    p.P = P;
    p.cam = lm_camera(c->cam);  // the kernel's bit-pattern isPixelGood (fm3d_ncc.hip ncc_geometry)
    std::memcpy(p.R2, c->R2, sizeof(p.R2));
    std::memcpy(p.t2, c->t2, sizeof(p.t2));
    p.img1 = c->pyr1[0].as<uint8_t>();
    p.img2 = c->pyr2[0].as<uint8_t>();
    p.w = c->lw[0];
    p.h = c->lh[0];
    p.offsets = c->offsets.as<int2>();
    p.nOff = c->nOff;
    p.nOffPad = c->nOffPad;
    p.boundW = c->s.boundWidth;
    p.boundH = c->s.boundHeight;
    p.cmax = (int)(2 * c->s.zThresholdMax);
    p.Hphi = Hphi;
    p.Htheta = Htheta;
    p.span = span;
    p.scores = S.as<double>();
    p.normals = N.as<double>();
    p.best = B.as<int>();
    fm3d::launch_ncc_hypotheses(p, c->stream);
    HIPCHK(c, hipGetLastError());
    HIPCHK(c, hipMemcpyAsync(scores, S.p, (size_t)P * H * sizeof(double), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipMemcpyAsync(normals, N.p, (size_t)P * 3 * sizeof(double), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipMemcpyAsync(best, B.p, (size_t)P * sizeof(int), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    return FM3D_OK;
}

int fm3d_pyrdown(fm3d_ctx* c, const uint8_t* src, int width, int height, uint8_t* dst) {
    if (!c || !src || !dst || width <= 0 || height <= 0) return FM3D_ERR_INVALID;
    hipSetDevice(c->device);
    DevBuf a, b;
    HIPCHK(c, a.ensure((size_t)width * height));
    const int dw = (width + 1) / 2, dh = (height + 1) / 2;
    HIPCHK(c, b.ensure((size_t)dw * dh));
    HIPCHK(c, hipMemcpy(a.p, src, (size_t)width * height, hipMemcpyHostToDevice));
    fm3d::launch_pyrdown(a.as<uint8_t>(), width, height, b.as<uint8_t>(), c->stream);
    HIPCHK(c, hipGetLastError());
    HIPCHK(c, hipStreamSynchronize(c->stream));
    HIPCHK(c, hipMemcpy(dst, b.p, (size_t)dw * dh, hipMemcpyDeviceToHost));
    return FM3D_OK;
}

int fm3d_neighborhood(fm3d_ctx* c, const double X[3], double* xy, int cap, int* m) {
    // host restatement of extractPixelsContour (used to cross-check the kernel's own)
    if (!c || !X || !m) return FM3D_ERR_INVALID;
    const double I[9] = {1, 0, 0, 0, 1, 0, 0, 0, 1}, Z[3] = {0, 0, 0};
    double cx, cy;
    fm3d::project1(c->cam, I, Z, X[0], X[1], X[2], cx, cy);
    const int R = c->s.pixelsRay;
    int n = 0;
    for (int i = -R; i <= R; i++)
        for (int j = -R; j <= R; j++)
            if (i * i + j * j <= R * R) {
                double px = cx + i, py = cy + j;
                if (px < 0 || py < 0 || px >= c->s.boundWidth || py >= c->s.boundHeight) continue;
                if (n < cap && xy) {
                    xy[2 * n] = px;
                    xy[2 * n + 1] = py;
                }
                n++;
            }
    *m = n;
    return FM3D_OK;
}

int fm3d_plane_to_image2(fm3d_ctx* c, const double X[3], const double n[3], double* xy, double* uv, int32_t* status,
                         int cap, int* m) {
    if (!c || !X || !n || !m || cap < 0) return FM3D_ERR_INVALID;
    if (!c->haveG12) return fail(c, FM3D_ERR_INVALID, "no camera-2 pose: call fm3d_setg12 / fm3d_set_g12 first");
    hipSetDevice(c->device);
    int r;
    if ((r = ensure_offsets(c))) return r;
    const int N = c->nOff;
    DevBuf bxy, buv, bkeep, bst;
    HIPCHK(c, bxy.ensure((size_t)N * 16));
    HIPCHK(c, buv.ensure((size_t)N * 16));
    HIPCHK(c, bkeep.ensure((size_t)N * 4));
    HIPCHK(c, bst.ensure((size_t)N * 4));
    fm3d::PlaneProjParams p{};
    p.cam = c->cam;
    std::memcpy(p.R2, c->R2, sizeof(p.R2));
    std::memcpy(p.t2, c->t2, sizeof(p.t2));
    for (int k = 0; k < 3; k++) {
        p.X[k] = X[k];
        p.n[k] = n[k];
    }
    p.cmax = (double)(int)(2 * c->s.zThresholdMax);
    p.offsets = c->offsets.as<int2>();
    p.nOff = N;
    p.boundW = c->s.boundWidth;
    p.boundH = c->s.boundHeight;
    p.w = c->w;  // isPixelGood bounds of the images set with fm3d_set_images (0: none)
    p.h = c->h;
    p.xy = bxy.as<double>();
    p.uv = buv.as<double>();
    p.keep = bkeep.as<int>();
    p.status = bst.as<int>();
    fm3d::launch_plane_project(p, c->stream);
    HIPCHK(c, hipGetLastError());
    HIPCHK(c, hipStreamSynchronize(c->stream));
    std::vector<double> hxy((size_t)2 * N), huv((size_t)2 * N);
    std::vector<int> hk(N), hs(N);
    HIPCHK(c, hipMemcpy(hxy.data(), bxy.p, (size_t)N * 16, hipMemcpyDeviceToHost));
    HIPCHK(c, hipMemcpy(huv.data(), buv.p, (size_t)N * 16, hipMemcpyDeviceToHost));
    HIPCHK(c, hipMemcpy(hk.data(), bkeep.p, (size_t)N * 4, hipMemcpyDeviceToHost));
    HIPCHK(c, hipMemcpy(hs.data(), bst.p, (size_t)N * 4, hipMemcpyDeviceToHost));
    int k = 0;
    for (int t = 0; t < N; t++) {
        if (!hk[t]) continue;
        if (k < cap) {
            if (xy) { xy[2 * k] = hxy[2 * t]; xy[2 * k + 1] = hxy[2 * t + 1]; }
            if (uv) { uv[2 * k] = huv[2 * t]; uv[2 * k + 1] = huv[2 * t + 1]; }
            if (status) status[k] = hs[t];
        }
        k++;
    }
    *m = k;
    return FM3D_OK;
}

int fm3d_undistort(fm3d_ctx* c, const double* xy, int n, double* out) {
    if (!c || n < 0 || (n && (!xy || !out))) return FM3D_ERR_INVALID;
    hipSetDevice(c->device);
    DevBuf a, b;
    HIPCHK(c, a.ensure((size_t)n * 16 + 16));
    HIPCHK(c, b.ensure((size_t)n * 16 + 16));
    HIPCHK(c, hipMemcpy(a.p, xy, (size_t)n * 16, hipMemcpyHostToDevice));
    fm3d::launch_undistort(c->cam, a.as<double>(), n, b.as<double>(), c->stream);
    HIPCHK(c, hipGetLastError());
    HIPCHK(c, hipStreamSynchronize(c->stream));
    HIPCHK(c, hipMemcpy(out, b.p, (size_t)n * 16, hipMemcpyDeviceToHost));
    return FM3D_OK;
}

int fm3d_math_probe(fm3d_ctx* c, int fn, const double* x, const double* y, int n, double* out) {
    if (!c || n < 0 || fn < 0 || fn >= FM3D_PROBE_COUNT || !x || !out) return FM3D_ERR_INVALID;
    const bool binary = fm3d::math_probe_binary(fn);
    if (binary && !y) return FM3D_ERR_INVALID;
    if (n == 0) return FM3D_OK;
    hipSetDevice(c->device);
    const size_t bytes = (size_t)n * sizeof(double);
    DevBuf a, b, o;
    HIPCHK(c, a.ensure(bytes));
    if (binary) HIPCHK(c, b.ensure(bytes));
    HIPCHK(c, o.ensure(bytes));
    HIPCHK(c, hipMemcpy(a.p, x, bytes, hipMemcpyHostToDevice));
    if (binary) HIPCHK(c, hipMemcpy(b.p, y, bytes, hipMemcpyHostToDevice));
    fm3d::launch_math_probe(fn, a.as<double>(), binary ? b.as<double>() : nullptr, n, o.as<double>(), c->stream);
    HIPCHK(c, hipGetLastError());
    HIPCHK(c, hipStreamSynchronize(c->stream));
    HIPCHK(c, hipMemcpy(out, o.p, bytes, hipMemcpyDeviceToHost));
    return FM3D_OK;
}

}  // extern "C"
