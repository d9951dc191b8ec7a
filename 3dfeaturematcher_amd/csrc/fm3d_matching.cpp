// fm3d_matching.cpp -- descriptor staging, the routing of the k = 2 search to the kernels of
// fm3d_match.hip by type and shape, NNDR and the cross-check (run_match: the pipeline's too), and the
// one-shot matcher entry points.
#include <cstdlib>
#include <cstring>
#include <utility>

#include "fm3d_ctx.h"

using namespace fm3d_host;

namespace {

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
}  // namespace
int fm3d_host::stage_descriptors(fm3d_ctx* c, const void* descA, int nA, const void* descB, int nB, int dim,
                                 int type, int* effType, int* dimPad, bool waitStaging, bool speculate) {
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
        HIPCHK(c, c->fwd.q8.ensure((size_t)nA * dp + 16));
        HIPCHK(c, c->fwd.t8.ensure((size_t)nB * dp + 16));
        HIPCHK(c, c->u8Flag.ensure(64));
        HIPCHK(c, c->hFlag.ensure(64));
        HIPCHK(c, hipMemsetAsync(c->u8Flag.p, 0, sizeof(int), c->stream));
        fm3d::launch_f32_pack_u8(c->A.as<float>(), nA, c->B.as<float>(), nB, dim, dp, c->fwd.q8.as<uint8_t>(),
                                 c->fwd.t8.as<uint8_t>(), c->u8Flag.as<int>(), c->stream);
        HIPCHK(c, hipGetLastError());
        *c->hFlag.as<int>() = -1;  // "not arrived" (the previous pair's copies into it have run: staging_wait)
        HIPCHK(c, hipMemcpyAsync(c->hFlag.p, c->u8Flag.p, sizeof(int), hipMemcpyDeviceToHost, c->stream));
        if (speculate) {
            // no host wait (fm3d_pipeline_submit_dlt_pair): the u8 matcher runs on the packed rows, and
            // the wait re-runs the front half on the float rows if the flag then says they were not
            // integers (redo_float_front)
            std::swap(c->A, c->fwd.q8);
            std::swap(c->B, c->fwd.t8);
            *dimPad = dp;
            *effType = FM3D_DESC_U8;
            c->specU8 = true;
            return FM3D_OK;
        }
        HIPCHK(c, hipEventRecord(c->evStage, c->stream));
        HIPCHK(c, hipEventSynchronize(c->evStage));
        if (*c->hFlag.as<int>() == 0) {
            std::swap(c->A, c->fwd.q8);  // the packed rows become the matcher's inputs
            std::swap(c->B, c->fwd.t8);
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

namespace {

// the parts' top-2 lists of a split search (int and float keys have one size)
int ensure_parts(fm3d_ctx* c, KnnWork& b, int parts, int nA) {
    if (parts <= 1) return FM3D_OK;
    HIPCHK(c, b.partIdx.ensure((size_t)parts * nA * 2 * sizeof(int) + 16));
    HIPCHK(c, b.partKey.ensure((size_t)parts * nA * 2 * sizeof(int) + 16));
    return FM3D_OK;
}

// the k = 2 search of nA query rows A over nB train rows B (as stage_descriptors left them) into
// b.idx / b.key / b.fkey.  deferMerge: the int8-MFMA routes leave their parts' lists in b.partIdx /
// b.partKey and set *mergeParts (the fused NNDR launch merges them).  gate (fm3d_kernels.h EpiGate):
// every type takes its gated kernels.
int knn2_search(fm3d_ctx* c, const DevBuf& A, const DevBuf& B, KnnWork& b, int nA, int nB, int type, int dimPad,
                bool deferMerge, int* mergeParts, const fm3d::EpiGate* gate) {
    *mergeParts = 1;
    int r;
    HIPCHK(c, b.idx.ensure((size_t)nA * 2 * sizeof(int) + 16));
    HIPCHK(c, b.key.ensure((size_t)nA * 2 * sizeof(int) + 16));
    HIPCHK(c, b.fkey.ensure((size_t)nA * 2 * sizeof(float) + 16));
    if (c->nCU <= 0) {
        int n = 0;
        HIPCHK(c, hipDeviceGetAttribute(&n, hipDeviceAttributeMultiprocessorCount, c->device));
        c->nCU = n > 0 ? n : 1;
    }
    if (type == FM3D_DESC_U8) {
        // (stage_descriptors pads to one of the two; the kernel has no other form)
        if (dimPad != 128 && dimPad != 256) return fail(c, FM3D_ERR_UNSUPPORTED, "u8 rows are matched at 128 or 256 bytes");
        const int nAPad = nA, nBPad = nB;
        HIPCHK(c, b.cq.ensure((size_t)(nAPad + 1) * sizeof(int)));
        HIPCHK(c, b.ct.ensure((size_t)(nBPad + 1) * sizeof(int)));
        fm3d::launch_rowconst_u8(A.as<uint8_t>(), nA, B.as<uint8_t>(), nB, dimPad, b.cq.as<int>(),
                                 b.ct.as<int>(), c->stream);
        const int parts = fm3d::knn2_u8_parts(nA, nB, c->nCU, fm3d::knn2_i8_queries_per_block(dimPad, 0),
                                              fm3d::knn2_i8_tile_rows(dimPad, 0));
        if ((r = ensure_parts(c, b, parts, nA))) return r;
        if (deferMerge && parts > 1) *mergeParts = parts;
        fm3d::launch_knn2_i8(A.as<uint8_t>(), nA, B.as<uint8_t>(), nB, dimPad, 0, b.cq.as<int>(),
                             b.ct.as<int>(), parts, b.partIdx.as<int>(), b.partKey.as<int>(), b.idx.as<int>(),
                             b.key.as<int>(), c->stream, *mergeParts > 1, gate);
    } else if (type == FM3D_DESC_F32 && gate) {
        // no bf16 prefilter here (its bound knows nothing of the gate): the exact scan of the rows inside it
        const int parts = fm3d::knn2_parts(nA, nB, dimPad, c->nCU);
        if ((r = ensure_parts(c, b, parts, nA))) return r;
        fm3d::launch_knn2_f32_gated(A.as<float>(), nA, B.as<float>(), nB, dimPad, parts, b.partIdx.as<int>(),
                                    b.partKey.as<float>(), b.idx.as<int>(), b.fkey.as<float>(), *gate, c->stream);
    } else if (type == FM3D_DESC_F32 && (dimPad == 64 || dimPad == 128) && nB >= 64 &&
               (long long)nA * nB >= (1LL << 22) && env_on("FM3D_F32_MFMA")) {
        // (FM3D_F32_MFMA=0 keeps float rows on the exact VALU scan: A/B comparisons)
        // float rows (SURF): the bf16 MFMA prefilter lists each query's possible top-2 rows, whose exact
        // FLANN-order distances decide (fm3d_match.hip); the same result as the full exact scan
        const int parts = fm3d::knn2_f32_mfma_parts(nA, nB, c->nCU);
        HIPCHK(c, c->f32Work.ensure(fm3d::knn2_f32_mfma_bytes(nA, nB, dimPad, parts)));
        // one fused pass; when more than 1/8 of the queries overflow its lists, the two-pass form (whose
        // lists hold only the rows under the final bound); FM3D_F32_FUSED=0 starts with the two-pass form
        bool fused = env_on("FM3D_F32_FUSED");
        int nResc = 0;
        for (;;) {
            fm3d::launch_knn2_f32_mfma(A.as<float>(), nA, B.as<float>(), nB, dimPad, parts, fused, c->f32Work.p,
                                       b.idx.as<int>(), b.fkey.as<float>(), c->stream);
            HIPCHK(c, hipMemcpyAsync(&nResc, fm3d::knn2_f32_mfma_rescan_count(c->f32Work.p, nA, nB, dimPad, parts),
                                     sizeof(int), hipMemcpyDeviceToHost, c->stream));
            HIPCHK(c, hipStreamSynchronize(c->stream));
            if (!fused || nResc <= nA / 8) break;
            fused = false;
        }
        if (nResc > 0 && nResc <= nA / 8) {
            // the queries whose bound held more rows than the candidate list: an exact wave-per-query scan
            fm3d::launch_knn2_f32_mfma_rescan(A.as<float>(), B.as<float>(), nB, dimPad, c->f32Work.p, nA, parts,
                                              nResc, b.idx.as<int>(), b.fkey.as<float>(), c->stream);
        } else if (nResc > 0) {
            // descriptors with no margin between neighbours (e.g. uniform noise in high dimension):
            // the full exact scan for every query
            const int p2 = fm3d::knn2_parts(nA, nB, dimPad, c->nCU);
            if ((r = ensure_parts(c, b, p2, nA))) return r;
            HIPCHK(c, b.pairs.ensure(fm3d::knn2_f32_pairs_bytes(nB, dimPad) + 16));
            fm3d::launch_knn2_f32(A.as<float>(), nA, B.as<float>(), nB, dimPad, p2, b.partIdx.as<int>(),
                                  b.partKey.as<float>(), b.pairs.as<float>(), b.idx.as<int>(), b.fkey.as<float>(),
                                  c->stream);
        }
    } else if (type == FM3D_DESC_F32) {
        const int parts = (dimPad == 64 || dimPad == 128) ? fm3d::knn2_parts(nA, nB, dimPad, c->nCU) : 1;
        if ((r = ensure_parts(c, b, parts, nA))) return r;
        HIPCHK(c, b.pairs.ensure(fm3d::knn2_f32_pairs_bytes(nB, dimPad) + 16));
        fm3d::launch_knn2_f32(A.as<float>(), nA, B.as<float>(), nB, dimPad, parts, b.partIdx.as<int>(),
                              b.partKey.as<float>(), b.pairs.as<float>(), b.idx.as<int>(), b.fkey.as<float>(),
                              c->stream);
    } else if (dimPad == 32 && env_on("FM3D_BITS_MFMA")) {  // =0 keeps them on the popcount kernel (A/B)
        // 256-bit rows (ORB): unpacked to int8 and matched on the int8 MFMA kernel (exact integer
        // Hamming distances popc(b) - a.b', same ranking rule)
        HIPCHK(c, b.q8.ensure((size_t)nA * 256 + 16));
        HIPCHK(c, b.t8.ensure((size_t)nB * 256 + 16));
        HIPCHK(c, b.ct.ensure((size_t)(nB + 1) * sizeof(int)));
        fm3d::launch_unpack_bits(A.as<uint8_t>(), nA, B.as<uint8_t>(), nB, b.q8.as<uint8_t>(),
                                 b.t8.as<uint8_t>(), b.ct.as<int>(), c->stream);
        const int parts = fm3d::knn2_u8_parts(nA, nB, c->nCU, fm3d::knn2_i8_queries_per_block(256, 1),
                                              fm3d::knn2_i8_tile_rows(256, 1));
        if ((r = ensure_parts(c, b, parts, nA))) return r;
        if (deferMerge && parts > 1) *mergeParts = parts;
        fm3d::launch_knn2_i8(b.q8.as<uint8_t>(), nA, b.t8.as<uint8_t>(), nB, 256, 1, nullptr, b.ct.as<int>(),
                             parts, b.partIdx.as<int>(), b.partKey.as<int>(), b.idx.as<int>(), b.key.as<int>(),
                             c->stream, *mergeParts > 1, gate);
    } else {
        const int parts = fm3d::knn2_parts(nA, nB, dimPad, c->nCU);
        if ((r = ensure_parts(c, b, parts, nA))) return r;
        fm3d::launch_knn2_bits(A.as<uint8_t>(), nA, B.as<uint8_t>(), nB, dimPad, parts, b.partIdx.as<int>(),
                               b.partKey.as<int>(), b.idx.as<int>(), b.key.as<int>(), c->stream, gate);
    }
    HIPCHK(c, hipGetLastError());
    return FM3D_OK;
}

}  // namespace

// (options: fm3d_ctx.h MatchOpts)
int fm3d_host::run_match(fm3d_ctx* c, int nA, int nB, int type, int dimPad, const MatchOpts& o) {
    const bool fuse = o.compactOut != nullptr && !o.wantKnn;
    if (o.crossCheck && !fuse) return fail(c, FM3D_ERR_INVALID, "the cross-check needs the compacted output");
    int mergeParts = 1;  // > 1: the parts' lists are merged by launch_nndr_compact
    KnnWork& f = c->fwd;
    HIPCHK(c, f.idx.ensure((size_t)nA * 2 * sizeof(int) + 16));
    HIPCHK(c, f.key.ensure((size_t)nA * 2 * sizeof(int) + 16));
    HIPCHK(c, f.fkey.ensure((size_t)nA * 2 * sizeof(float) + 16));
    HIPCHK(c, c->cand.ensure((size_t)nA * sizeof(fm3d_dmatch) + 16));
    HIPCHK(c, c->flag.ensure((size_t)nA * sizeof(int) + 16));
    if (o.wantKnn) HIPCHK(c, c->knnOut.ensure((size_t)nA * 2 * sizeof(fm3d_dmatch) + 16));
    int r;
    if ((r = knn2_search(c, c->A, c->B, f, nA, nB, type, dimPad, fuse, &mergeParts, o.gate))) return r;
    if (o.crossCheck) {
        // rev[j]: train row j's two nearest queries.  With a gate both searches rank the same
        // admissible pairs: the reverse kernels evaluate the forward predicate with the sides swapped
        fm3d::EpiGate rg{};
        if (o.gate) {
            rg = *o.gate;
            rg.transposed = true;
        }
        int revParts = 1;
        if ((r = knn2_search(c, c->B, c->A, c->rev, nB, nA, type, dimPad, false, &revParts, o.gate ? &rg : nullptr)))
            return r;
        fm3d::LookBack lb;
        if ((r = make_lookback(c, fm3d::nndr_compact_blocks(nA), &lb))) return r;
        const fm3d::MutualCheck mc{c->rev.idx.as<int>(), c->rev.key.as<int>(), c->rev.fkey.as<float>(), o.crossCheck};
        fm3d::launch_nndr_mutual_compact(type, f.idx.as<int>(), f.key.as<int>(), f.fkey.as<float>(),
                                         f.partIdx.as<int>(), f.partKey.as<int>(), mergeParts, nA, o.eps,
                                         o.queryOffset, mc, o.compactOut, o.compactCount, lb, c->stream);
    } else if (fuse) {
        fm3d::LookBack lb;
        if ((r = make_lookback(c, fm3d::nndr_compact_blocks(nA), &lb))) return r;
        fm3d::launch_nndr_compact(type, f.idx.as<int>(), f.key.as<int>(), f.fkey.as<float>(), f.partIdx.as<int>(),
                                  f.partKey.as<int>(), mergeParts, nA, o.eps, o.queryOffset, o.compactOut,
                                  o.compactCount, lb, c->stream);
    } else {
        fm3d::launch_nndr(type, f.idx.as<int>(), f.key.as<int>(), f.fkey.as<float>(), nA, nB, o.eps, o.queryOffset,
                          o.wantKnn ? c->knnOut.as<fm3d_dmatch>() : nullptr, c->cand.as<fm3d_dmatch>(),
                          c->flag.as<int>(), c->stream);
    }
    HIPCHK(c, hipGetLastError());
    return FM3D_OK;
}

namespace {

// One one-shot matcher call: the six entry points differ in whether keypoints gate the search and in
// what comes back -- the two neighbours of every query, the NNDR matches, or the cross-checked ones.
enum class MatchOut { Knn, Nndr, Mutual };
struct OneShot {
    MatchOut kind;
    const void* descA;
    int nA;
    const void* descB;
    int nB, dim, type;
    fm3d_dmatch* out;
    int* nMatches = nullptr;  // not Knn
    double eps = 0.0;
    bool guided = false;  // kpts1, kpts2 and maxPx count
    const fm3d_point2f *kpts1 = nullptr, *kpts2 = nullptr;
    double maxPx = 0.0;
    int mode = 0;  // Mutual: 1 or 2
};

int ensure_matches(fm3d_ctx* c, int nA) {
    if (int r = ensure_scan_tmp(c, nA)) return r;
    HIPCHK(c, c->matches.ensure((size_t)(nA + 1) * sizeof(fm3d_dmatch)));
    return FM3D_OK;
}

int match_once(fm3d_ctx* c, const OneShot& a) {
    const bool knn = a.kind == MatchOut::Knn;
    const int nA = a.nA, nB = a.nB;
    if (!c || (!knn && !a.nMatches) || (!a.descA && nA) || (!a.descB && nB) || (!a.out && nA) ||
        (a.guided && ((!a.kpts1 && nA) || (!a.kpts2 && nB))))
        return fail(c, FM3D_ERR_INVALID, "null argument");
    if (a.kind == MatchOut::Mutual && a.mode != 1 && a.mode != 2)
        return fail(c, FM3D_ERR_INVALID, "mode must be 1 (mutual nearest) or 2 (symmetric ratio)");
    if (a.guided) {
        if (!c->haveG12) return fail(c, FM3D_ERR_INVALID, "g12 not set (SingleCameraTriangulator::setg12)");
        if (!good_max_px(a.maxPx)) return fail(c, FM3D_ERR_INVALID, "maxPx must be finite and > 0");
    }
    hipSetDevice(c->device);
    int t, dp, r;
    if ((r = stage_descriptors(c, a.descA, nA, a.descB, nB, a.dim, a.type, &t, &dp))) return r;
    fm3d::EpiGate gate{};
    MatchOpts o;
    o.eps = a.eps;
    o.wantKnn = knn;
    if (a.guided) {  // the keypoints onto the device, and the gate
        if ((r = upload(c, c->kp1, a.kpts1, (size_t)nA * sizeof(fm3d_point2f)))) return r;
        if ((r = upload(c, c->kp2, a.kpts2, (size_t)nB * sizeof(fm3d_point2f)))) return r;
        c->gateStaged = false;  // (a staged pipeline pair's keypoints are replaced, as fm3d_triangulate replaces them)
        if ((r = make_gate(c, c->kp1.as<fm3d_point2f>(), nA, c->kp2.as<fm3d_point2f>(), nB, a.maxPx, &gate))) return r;
        o.gate = &gate;
    }
    if (a.kind == MatchOut::Mutual) {  // the compaction is fused into the NNDR launch
        if ((r = ensure_matches(c, nA))) return r;
        o.compactOut = c->matches.as<fm3d_dmatch>();
        o.compactCount = c->count.as<int>();
        o.crossCheck = a.mode;
    }
    if ((r = run_match(c, nA, nB, t, dp, o))) return r;
    if (knn) {
        if (nA) HIPCHK(c, hipMemcpyAsync(a.out, c->knnOut.p, (size_t)nA * 2 * sizeof(fm3d_dmatch), hipMemcpyDeviceToHost, c->stream));
        HIPCHK(c, hipStreamSynchronize(c->stream));
        return FM3D_OK;
    }
    if (a.kind == MatchOut::Nndr) {
        if ((r = ensure_matches(c, nA))) return r;
        fm3d::launch_compact_dmatch(c->cand.as<fm3d_dmatch>(), c->flag.as<int>(), nA, c->matches.as<fm3d_dmatch>(),
                                    c->count.as<int>(), c->scanTmp.p, c->stream);
        HIPCHK(c, hipGetLastError());
    }
    int n = 0;  // count -> wait -> copy n matches
    HIPCHK(c, hipMemcpyAsync(&n, c->count.p, sizeof(int), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    if (n) HIPCHK(c, hipMemcpy(a.out, c->matches.p, (size_t)n * sizeof(fm3d_dmatch), hipMemcpyDeviceToHost));
    *a.nMatches = n;
    return FM3D_OK;
}

}  // namespace

extern "C" {

int fm3d_knn2(fm3d_ctx* c, const void* descA, int nA, const void* descB, int nB, int dim, int type, fm3d_dmatch* out) {
    return match_once(c, {MatchOut::Knn, descA, nA, descB, nB, dim, type, out});
}

int fm3d_match_nndr(fm3d_ctx* c, const void* descA, int nA, const void* descB, int nB, int dim, int type,
                    double epsilon, fm3d_dmatch* matches, int* nMatches) {
    return match_once(c, {MatchOut::Nndr, descA, nA, descB, nB, dim, type, matches, nMatches, epsilon});
}

int fm3d_knn2_guided(fm3d_ctx* c, const void* descA, int nA, const void* descB, int nB, int dim, int type,
                     const fm3d_point2f* kpts1, const fm3d_point2f* kpts2, double maxPx, fm3d_dmatch* out) {
    return match_once(c, {MatchOut::Knn, descA, nA, descB, nB, dim, type, out, nullptr, 0.0, true, kpts1, kpts2, maxPx});
}

int fm3d_match_nndr_guided(fm3d_ctx* c, const void* descA, int nA, const void* descB, int nB, int dim, int type,
                           const fm3d_point2f* kpts1, const fm3d_point2f* kpts2, double epsilon, double maxPx,
                           fm3d_dmatch* matches, int* nMatches) {
    return match_once(c, {MatchOut::Nndr, descA, nA, descB, nB, dim, type, matches, nMatches, epsilon, true, kpts1, kpts2,
                          maxPx});
}

int fm3d_match_mutual(fm3d_ctx* c, const void* descA, int nA, const void* descB, int nB, int dim, int type,
                      double epsilon, int mode, fm3d_dmatch* matches, int* nMatches) {
    return match_once(c, {MatchOut::Mutual, descA, nA, descB, nB, dim, type, matches, nMatches, epsilon, false, nullptr,
                          nullptr, 0.0, mode});
}

int fm3d_match_mutual_guided(fm3d_ctx* c, const void* descA, int nA, const void* descB, int nB, int dim, int type,
                             const fm3d_point2f* kpts1, const fm3d_point2f* kpts2, double epsilon, double maxPx,
                             int mode, fm3d_dmatch* matches, int* nMatches) {
    return match_once(c, {MatchOut::Mutual, descA, nA, descB, nB, dim, type, matches, nMatches, epsilon, true, kpts1,
                          kpts2, maxPx, mode});
}

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

}  // extern "C"
