// fm3d_tail.cpp -- fm3d_pipeline_describe(_any): the reference's tail (main.cpp:157-183) for points and
// normals that already lie in HBM.  Frames and the patch camera in one launch over all n points, then
// chunk after chunk the patches into a context buffer and their descriptors read from it in place;
// the descriptor rows (and the frames) leave in one copy at the end and the host waits once.  The
// frame and patch kernels are fm3d_features_frames' and fm3d_export_patches' own and the descriptors
// come from the describer behind fm3d_extract_descriptors_from_patches (fm3d_patchdesc.cpp), so the
// bytes are theirs: DESIGN.md §3.5b.  The _any form adds ORB's rows, and the zero rows the reference
// keeps for a BRISK or FREAK keypoint that its border filter drops.
#include <cstdlib>

#include "fm3d_features.h"

using namespace fm3d_host;

int fm3d_host::describe_chunk() {
    // patches per chunk launch (DESIGN.md §3.5b has the comparison); one grid.y holds 65,535
    constexpr int kDescribeChunk = 4096, kChunkMax = 65535;
    const char* e = getenv("FM3D_DESCRIBE_CHUNK");
    if (!e || !*e) return kDescribeChunk;
    const long v = strtol(e, nullptr, 10);
    return (int)std::min<long>(std::max<long>(v, 1), kChunkMax);
}

namespace {

// both entry points: `any` admits the binary extractors
int describe(fm3d_ctx* c, bool any, int source, const fm3d_record* recordsDev, int n, void* desc, double* frames,
             uint8_t* patches, fm3d_describe_stats* stats) {
    if (!c) return FM3D_ERR_INVALID;
    if (n < 0 || (n && !desc)) return fail(c, FM3D_ERR_INVALID, "null argument or n < 0");
    if (source != FM3D_DESCRIBE_RECORDS && source != FM3D_DESCRIBE_NCC)
        return fail(c, FM3D_ERR_INVALID, "source is neither FM3D_DESCRIBE_RECORDS nor FM3D_DESCRIBE_NCC");
    if (c->pipe.state != PairState::Idle)
        return fail(c, FM3D_ERR_INVALID, "a submitted frame pair is pending: fm3d_pipeline_wait first");
    if (source == FM3D_DESCRIBE_NCC) {
        if (recordsDev) return fail(c, FM3D_ERR_INVALID, "FM3D_DESCRIBE_NCC takes no record buffer");
        if (n != c->nccP) return fail(c, FM3D_ERR_INVALID, "n is not the last fm3d_pipeline_run_ncc's point count");
        if ((size_t)n * 3 * sizeof(double) > c->pts.bytes || (size_t)n * 3 * sizeof(double) > c->nccN.bytes)
            return fail(c, FM3D_ERR_INVALID, "the NCC run's points / normals are not on the context");
    } else if (!recordsDev && (size_t)n * sizeof(fm3d_record) > c->records.bytes) {
        return fail(c, FM3D_ERR_INVALID, "the context's record buffer holds fewer than n records");
    }
    if (c->pyr1.empty()) return fail(c, FM3D_ERR_INVALID, "fm3d_set_images not called");
    const int size = fm3d_patch_size(&c->s);
    if (size <= 0) return fail(c, FM3D_ERR_INVALID, "patch size <= 0 (Neighborhoods.epsilon / cmPerPixel)");
    const fm3d_settings& S = c->s;
    PatchDesc d;
    int r;
    if ((r = patch_desc_kind(c, any, &d))) return r;
    if (stats) std::memset(stats, 0, sizeof(*stats));
    if (n == 0) return FM3D_OK;

    double g[3];
    if ((r = fm3d_gravity(&S, g))) return fail(c, r, "gravity: singular rodriguesIC rotation");
    // the describer's refusals, tables and scratch by the chunk (each first use may wait for its upload),
    // then this call's buffers: n x (frame, R t, row) and one chunk of patches.  BRISK and FREAK, if they
    // run at all, need no patch for their zero rows
    const bool zeros = d.kind == PatchDesc::Binary;
    const int chunk = std::min(describe_chunk(), n);
    const size_t per = (size_t)size * size;
    if ((r = patch_desc_prepare(c, size, chunk, &d))) return r;
    HIPCHK(c, c->tailFrames.ensure((size_t)n * 16 * sizeof(double)));
    HIPCHK(c, c->tailRT.ensure((size_t)n * 12 * sizeof(double)));
    if (!zeros) HIPCHK(c, c->tailDesc.ensure((size_t)n * d.rowBytes));
    if (!zeros || patches) HIPCHK(c, c->tailPatch.ensure((size_t)chunk * per));

    HIPCHK(c, hipEventRecord(c->ev[EV_TAIL_START], c->stream));
    const bool ncc = source == FM3D_DESCRIBE_NCC;
    const fm3d_record* rec = ncc ? nullptr : recordsDev ? recordsDev : c->records.as<fm3d_record>();
    fm3d::launch_tail_frames(rec, ncc ? c->pts.as<double>() : nullptr, ncc ? c->nccN.as<double>() : nullptr, n, g,
                             c->tailFrames.as<double>(), c->tailRT.as<double>(), c->stream);
    uint8_t* pbuf = c->tailPatch.as<uint8_t>();
    int chunks = 0;
    for (int p0 = 0; p0 < n && (!zeros || patches); p0 += chunk, chunks++) {
        const int m = std::min(chunk, n - p0);
        fm3d::launch_patches(c->tailRT.as<double>() + 12 * (size_t)p0, m, size, S.neighEpsilon, S.cmPerPixel * 0.01,
                             c->cam, c->pyr1[0].as<uint8_t>(), c->lw[0], c->lh[0], pbuf, c->stream);
        if (zeros) HIPCHK(c, hipGetLastError());  // the patches are the caller's only
        else if ((r = patch_desc_queue(c, d, pbuf, p0, m, c->tailDesc.p))) return r;
        // only a caller who asks for the patches has them copied out, chunk by chunk, behind their descriptors
        if (patches)
            HIPCHK(c, hipMemcpyAsync(patches + per * p0, pbuf, per * m, hipMemcpyDeviceToHost, c->stream));
    }
    int kept = n;
    if (d.kind == PatchDesc::SurfOriented)
        HIPCHK(c, hipMemcpyAsync(&kept, c->pdKept.p, sizeof(int), hipMemcpyDeviceToHost, c->stream));
    if (frames)
        HIPCHK(c, hipMemcpyAsync(frames, c->tailFrames.p, (size_t)n * 16 * sizeof(double), hipMemcpyDeviceToHost,
                                 c->stream));
    if (zeros)
        std::memset(desc, 0, (size_t)n * d.rowBytes);
    else
        HIPCHK(c, hipMemcpyAsync(desc, c->tailDesc.p, (size_t)n * d.rowBytes, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipEventRecord(c->ev[EV_END], c->stream));
    HIPCHK(c, hipEventSynchronize(c->ev[EV_END]));  // the call's one wait
    if (kept != n) return fail(c, FM3D_ERR_INVALID, "patch keypoint dropped by SURF (no orientation sample)");
    if (stats) {
        stats->points = n;
        stats->patchSize = size;
        stats->cols = d.cols;
        stats->type = d.type;
        stats->chunks = chunks;
        float ms = 0;
        hipEventElapsedTime(&ms, c->ev[EV_TAIL_START], c->ev[EV_END]);
        stats->total_ms = ms;
    }
    return FM3D_OK;
}

}  // namespace

extern "C" int fm3d_pipeline_describe(fm3d_ctx* c, int source, const fm3d_record* recordsDev, int n, void* desc,
                                      double* frames, uint8_t* patches, fm3d_describe_stats* stats) {
    return describe(c, false, source, recordsDev, n, desc, frames, patches, stats);
}

extern "C" int fm3d_pipeline_describe_any(fm3d_ctx* c, int source, const fm3d_record* recordsDev, int n, void* desc,
                                          double* frames, uint8_t* patches, fm3d_describe_stats* stats) {
    return describe(c, true, source, recordsDev, n, desc, frames, patches, stats);
}
