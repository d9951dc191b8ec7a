// fm3d_tail.cpp -- fm3d_pipeline_describe(_any): the reference's tail (main.cpp:157-183) for points and
// normals that already lie in HBM.  Frames and the patch camera in one launch over all n points, then
// chunk after chunk the patches into a context buffer and their descriptors read from it in place;
// the descriptor rows (and the frames) leave in one copy at the end and the host waits once.  The
// kernels are the one-shot calls' own (fm3d_features_frames, fm3d_export_patches,
// fm3d_extract_descriptors_from_patches), so the bytes are theirs: DESIGN.md §3.5b.  The _any form adds
// the binary extractors: ORB's rows from launch_orb_patch_desc on each chunk, and the zero rows the
// reference keeps for a BRISK or FREAK keypoint that its border filter drops.
#include <algorithm>
#include <cmath>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "fm3d_ctx.h"

using namespace fm3d_host;

namespace {

// patches per chunk launch (DESIGN.md §3.5b has the comparison); one grid.y holds 65,535
constexpr int kDescribeChunk = 4096;
constexpr int kChunkMax = 65535;

}  // namespace

int fm3d_host::describe_chunk() {
    const char* e = getenv("FM3D_DESCRIBE_CHUNK");
    if (!e || !*e) return kDescribeChunk;
    const long v = strtol(e, nullptr, 10);
    return (int)std::min<long>(std::max<long>(v, 1), kChunkMax);
}

namespace {

// The per-patch constants of a chunk are the same for every chunk: the centred keypoint
// (descriptorsmatcher.cpp:146-158), and for SIFT the patch's level row and index.  Built once per
// (capacity, patch edge, keypoint angle) and kept; a smaller capacity reads a prefix.
int ensure_tables(fm3d_ctx* c, int cap, int size, float angle) {
    if (cap <= c->tailCap && size == c->tailSize && angle == c->tailAngle) return FM3D_OK;
    c->tailCap = 0;
    const float center = (float)(int)std::floor(size / 2);
    const fm3d_keypoint k{center, center, (float)size, angle, 1.f, 0, 0};
    const size_t per = (size_t)size * size;
    std::vector<fm3d_keypoint> kp((size_t)cap, k);
    std::vector<fm3d::SiftLevel> GL((size_t)cap);
    std::vector<int> lvl((size_t)cap);
    for (int p = 0; p < cap; p++) {
        GL[p] = {size, size, (long long)(p * per)};
        lvl[p] = p;
    }
    HIPCHK(c, c->tailKp.ensure(kp.size() * sizeof(fm3d_keypoint)));
    HIPCHK(c, c->tailGL.ensure(GL.size() * sizeof(fm3d::SiftLevel)));
    HIPCHK(c, c->tailLvl.ensure(lvl.size() * sizeof(int)));
    HIPCHK(c, hipMemcpyAsync(c->tailKp.p, kp.data(), kp.size() * sizeof(fm3d_keypoint), hipMemcpyHostToDevice, c->stream));
    HIPCHK(c, hipMemcpyAsync(c->tailGL.p, GL.data(), GL.size() * sizeof(fm3d::SiftLevel), hipMemcpyHostToDevice,
                             c->stream));
    HIPCHK(c, hipMemcpyAsync(c->tailLvl.p, lvl.data(), lvl.size() * sizeof(int), hipMemcpyHostToDevice, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));  // the vectors leave scope
    c->tailCap = cap;
    c->tailSize = size;
    c->tailAngle = angle;
    return FM3D_OK;
}

// the level-0 blur taps of the patches' SIFT pyramid, kept per sigma
int ensure_taps(fm3d_ctx* c) {
    std::vector<float> taps;
    if (int r = sift_patch_taps(c, taps)) return r;
    const float sigma = (float)c->s.siftSigma;
    if (c->tailNTaps == (int)taps.size() && c->tailSigma == sigma) return FM3D_OK;
    c->tailNTaps = 0;
    HIPCHK(c, c->tailTaps.ensure(128 * sizeof(float)));
    HIPCHK(c, hipMemcpyAsync(c->tailTaps.p, taps.data(), taps.size() * sizeof(float), hipMemcpyHostToDevice, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    c->tailNTaps = (int)taps.size();
    c->tailSigma = sigma;
    return FM3D_OK;
}

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
    const int ex = S.extractorType;
    const bool sift = ex == FM3D_FEAT_SIFT, surf = ex == FM3D_FEAT_SURF;
    const bool orb = any && ex == FM3D_FEAT_ORB;
    const bool zeros = any && (ex == FM3D_FEAT_BRISK || ex == FM3D_FEAT_FREAK);  // if it runs at all: see below
    if (!sift && !surf && !orb && !zeros)
        return fail(c, FM3D_ERR_UNSUPPORTED,
                    any ? "the settings' extractor type has no GPU implementation"
                        : "only the SURF and SIFT extractors describe patches on the GPU");
    if (stats) std::memset(stats, 0, sizeof(*stats));
    if (n == 0) return FM3D_OK;

    int r, cols = 0, type = 0;
    if ((r = fm3d_descriptor_info(c, &cols, &type))) return r;
    double g[3];
    if ((r = fm3d_gravity(&S, g))) return fail(c, r, "gravity: singular rodriguesIC rotation");
    // the centred keypoint's wavelet against the patch (SURFInvoker's drop): one answer for every patch
    if (surf && size + 1 < surf_patch_gws(size))
        return fail(c, FM3D_ERR_INVALID, "patch keypoint dropped by SURF (descriptor row missing)");
    if (zeros) {
        // BRISK's and FREAK's border filters keep the centred keypoint from an edge of 634 and 680 only;
        // below, every row is the reference's Mat::zeros row and no patch is needed for it
        int kept = 0;
        if ((r = fm3d_patch_keypoint_kept(c, size, &kept))) return fail(c, r, "patch keypoint: no keep rule");
        if (kept)
            return fail(c, FM3D_ERR_UNSUPPORTED,
                        "BRISK / FREAK keep the centred keypoint of a " + std::to_string(size) +
                            " px patch: no batched form, use fm3d_extract_descriptors_from_patches_any");
    }
    hipSetDevice(c->device);
    // ORB: the settings, the keep rule ("ORB drops the first patch's keypoint..."), the offset table of
    // the centred keypoint and the border guard of launch_orb_patch_desc
    if (orb && (r = orb_patch_prepare(c, size))) return r;
    const bool oriented = surf && !S.surfUpright;
    const int chunk = std::min(describe_chunk(), n);
    const size_t per = (size_t)size * size;
    const size_t rowBytes = (size_t)cols * (type == FM3D_DESC_BITS ? 1 : sizeof(float));

    // first-use tables (each may wait for its upload), then every buffer: n x (frame, R t, row), the
    // rest by the chunk
    if (sift) {
        if ((r = ensure_taps(c))) return r;
    } else if (surf && (r = ensure_surf_dw(c))) {
        return r;
    }
    if ((sift || surf) && (r = ensure_tables(c, chunk, size, sift || oriented ? -1.f : 360.f - 90.f))) return r;
    HIPCHK(c, c->tailFrames.ensure((size_t)n * 16 * sizeof(double)));
    HIPCHK(c, c->tailRT.ensure((size_t)n * 12 * sizeof(double)));
    if (!zeros) HIPCHK(c, c->tailDesc.ensure((size_t)n * rowBytes));
    if (!zeros || patches) HIPCHK(c, c->tailPatch.ensure((size_t)chunk * per));
    const size_t sumPer = (size_t)(size + 1) * (size + 1);
    if (sift) {
        HIPCHK(c, c->siftBase.ensure((size_t)chunk * per * sizeof(float)));
        HIPCHK(c, c->siftG.ensure((size_t)chunk * per * sizeof(float)));
    } else if (oriented) {
        if ((r = ensure_scan_tmp(c, chunk))) return r;
        HIPCHK(c, c->sfSum.ensure((size_t)chunk * sumPer * sizeof(int)));
        HIPCHK(c, c->sfAng.ensure((size_t)(chunk + 1) * sizeof(float)));
        HIPCHK(c, c->sfFlag.ensure((size_t)(chunk + 1) * sizeof(int)));
        HIPCHK(c, c->sfPos.ensure((size_t)(chunk + 1) * sizeof(int)));
        HIPCHK(c, c->sfKp.ensure((size_t)chunk * sizeof(fm3d_keypoint)));
        HIPCHK(c, c->tailSum.ensure(sizeof(int)));
    }

    HIPCHK(c, hipEventRecord(c->ev[EV_TAIL_START], c->stream));
    const bool ncc = source == FM3D_DESCRIBE_NCC;
    const fm3d_record* rec = ncc ? nullptr : recordsDev ? recordsDev : c->records.as<fm3d_record>();
    fm3d::launch_tail_frames(rec, ncc ? c->pts.as<double>() : nullptr, ncc ? c->nccN.as<double>() : nullptr, n, g,
                             c->tailFrames.as<double>(), c->tailRT.as<double>(), c->stream);
    if (oriented) {
        // the compacted keypoints start as the table's rows: a chunk that drops one (an error at the
        // end) leaves its last rows as they were, and the describe launch still reads valid keypoints
        HIPCHK(c, hipMemsetAsync(c->tailSum.p, 0, sizeof(int), c->stream));
        HIPCHK(c, hipMemcpyAsync(c->sfKp.p, c->tailKp.p, (size_t)chunk * sizeof(fm3d_keypoint), hipMemcpyDeviceToDevice,
                                 c->stream));
    }
    const fm3d_keypoint* tkp = c->tailKp.as<fm3d_keypoint>();
    uint8_t* pbuf = c->tailPatch.as<uint8_t>();
    int chunks = 0;
    for (int p0 = 0; p0 < n && (!zeros || patches); p0 += chunk, chunks++) {
        const int m = std::min(chunk, n - p0);
        fm3d::launch_patches(c->tailRT.as<double>() + 12 * (size_t)p0, m, size, S.neighEpsilon, S.cmPerPixel * 0.01,
                             c->cam, c->pyr1[0].as<uint8_t>(), c->lw[0], c->lh[0], pbuf, c->stream);
        float* rows = reinterpret_cast<float*>(c->tailDesc.as<char>() + (size_t)p0 * rowBytes);
        if (zeros) {
            // the patches are the caller's only
        } else if (orb) {
            orb_patch_describe(c, pbuf, m, size, reinterpret_cast<uint8_t*>(rows));
        } else if (sift) {
            fm3d::SiftResize rp{};
            rp.sw = rp.dw = size;
            rp.sh = rp.dh = size;
            rp.doubled = 0;
            fm3d::launch_sift_init(pbuf, c->siftBase.as<float>(), rp, m, c->stream);
            fm3d::launch_sift_blur(c->siftBase.as<float>(), c->siftG.as<float>(), nullptr, size, size,
                                   c->tailTaps.as<float>(), c->tailNTaps, m, c->stream);
            fm3d::launch_sift_desc(c->siftG.as<float>(), c->tailGL.as<fm3d::SiftLevel>(), S.siftOctaveLayers, 0, tkp,
                                   c->tailLvl.as<int>(), m, rows, c->stream);
        } else if (oriented) {
            fm3d::launch_integral_batch(pbuf, size, size, m, c->sfSum.as<int>(), c->stream);
            fm3d::launch_surf_orient(tkp, sizeof(fm3d_keypoint), m, c->sfSum.as<int>(), sumPer, size, size,
                                     surf_ori_samples(), c->sfFlag.as<int>(), c->sfAng.as<float>(), c->stream);
            fm3d::launch_surf_keep(tkp, m, size, size, c->sfFlag.as<int>(), c->sfPos.as<int>(), c->count.as<int>(),
                                   c->scanTmp.p, c->sfKp.as<fm3d_keypoint>(), nullptr, c->sfAng.as<float>(), c->stream);
            fm3d::launch_add_count(c->count.as<int>(), c->tailSum.as<int>(), c->stream);
            fm3d::launch_surf_describe(pbuf, per, size, size, c->sfKp.as<fm3d_keypoint>(), m, c->sfDW.as<float>(),
                                       S.surfExtended, 0, rows, c->stream);
        } else {
            fm3d::launch_surf_describe(pbuf, per, size, size, tkp, m, c->sfDW.as<float>(), S.surfExtended, 1, rows,
                                       c->stream);
        }
        HIPCHK(c, hipGetLastError());
        // only a caller who asks for the patches has them copied out, chunk by chunk, behind their descriptors
        if (patches)
            HIPCHK(c, hipMemcpyAsync(patches + per * p0, pbuf, per * m, hipMemcpyDeviceToHost, c->stream));
    }
    int kept = n;
    if (oriented) HIPCHK(c, hipMemcpyAsync(&kept, c->tailSum.p, sizeof(int), hipMemcpyDeviceToHost, c->stream));
    if (frames)
        HIPCHK(c, hipMemcpyAsync(frames, c->tailFrames.p, (size_t)n * 16 * sizeof(double), hipMemcpyDeviceToHost,
                                 c->stream));
    if (zeros)
        std::memset(desc, 0, (size_t)n * rowBytes);
    else
        HIPCHK(c, hipMemcpyAsync(desc, c->tailDesc.p, (size_t)n * rowBytes, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipEventRecord(c->ev[EV_END], c->stream));
    HIPCHK(c, hipEventSynchronize(c->ev[EV_END]));  // the call's one wait
    if (kept != n) return fail(c, FM3D_ERR_INVALID, "patch keypoint dropped by SURF (no orientation sample)");
    if (stats) {
        stats->points = n;
        stats->patchSize = size;
        stats->cols = cols;
        stats->type = type;
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
