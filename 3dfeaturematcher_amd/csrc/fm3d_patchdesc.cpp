// fm3d_patchdesc.cpp -- the patch describer: m equal-sized patches on the device become m descriptor
// rows on the device, each patch described at its centred keypoint (extractDescriptorsFromPatches,
// descriptorsmatcher.cpp:133-174).  The one-shot calls below upload their patches to it and
// fm3d_pipeline_describe (fm3d_tail.cpp) hands it the chunks it projected: DESIGN.md §3.5b.
#include <string>

#include "fm3d_features.h"

using namespace fm3d_host;

namespace {

// The per-patch constants are the same for every chunk and every call: the centred keypoint, and for
// SIFT the patch's level row and index.  Built once per (capacity, patch edge, keypoint angle) and
// kept; a smaller capacity reads a prefix.
int ensure_tables(fm3d_ctx* c, int cap, int size, float angle) {
    if (cap <= c->pdCap && size == c->pdSize && angle == c->pdAngle) return FM3D_OK;
    c->pdCap = 0;
    const size_t per = (size_t)size * size;
    std::vector<fm3d_keypoint> kp((size_t)cap, patch_keypoint(size, angle));
    std::vector<fm3d::SiftLevel> GL((size_t)cap);
    std::vector<int> lvl((size_t)cap);
    for (int p = 0; p < cap; p++) {
        GL[p] = {size, size, (long long)(p * per)};
        lvl[p] = p;
    }
    int r;
    if ((r = upload(c, c->pdKp, kp.data(), kp.size() * sizeof(fm3d_keypoint))) ||
        (r = upload(c, c->pdGL, GL.data(), GL.size() * sizeof(fm3d::SiftLevel))) ||
        (r = upload(c, c->pdLvl, lvl.data(), lvl.size() * sizeof(int))))
        return r;
    HIPCHK(c, hipStreamSynchronize(c->stream));  // the vectors leave scope
    c->pdCap = cap;
    c->pdSize = size;
    c->pdAngle = angle;
    return FM3D_OK;
}

// SIFT on a patch (SIFT::operator()(patch, Mat(), {kp}, desc, true), kp of octave 0): firstOctave 0, one
// octave, and the descriptor reads level 0 of it, blur(patch, sig_diff) -- so every patch needs only
// that level.  Its taps, kept per sigma.
int ensure_taps(fm3d_ctx* c) {
    int r;
    const float sigma = (float)c->s.siftSigma;
    const float sigDiff = std::sqrt(std::max(sigma * sigma - 0.5f * 0.5f, 0.01f));
    std::vector<float> taps;
    if ((r = sift_check_settings(c)) || (r = sift_blur_taps(c, sigDiff, taps))) return r;
    if (c->pdNTaps == (int)taps.size() && c->pdSigma == sigma) return FM3D_OK;
    c->pdNTaps = 0;
    HIPCHK(c, c->pdTaps.ensure(128 * sizeof(float)));
    HIPCHK(c, hipMemcpyAsync(c->pdTaps.p, taps.data(), taps.size() * sizeof(float), hipMemcpyHostToDevice, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    c->pdNTaps = (int)taps.size();
    c->pdSigma = sigma;
    return FM3D_OK;
}

// ORB on patches of one edge, before any launch: orb_check_settings, the keep rule's answer, the offset
// table of the centred keypoint (built on first use and after a change of pattern, orbPatchSize or angle;
// the only wait) and launch_orb_patch_desc's border guard against the table's own reach
int orb_prepare(fm3d_ctx* c, int size, int kept) {
    int r;
    if ((r = orb_check_settings(c))) return r;
    if (!kept)
        return fail(c, FM3D_ERR_INVALID, "ORB drops the first patch's keypoint (the reference's rows would have 0 columns)");
    // every patch's keypoint has angle -1, so one table serves them all
    const float angle = patch_keypoint(size, -1.f).angle;
    const int patchSize = c->s.orbPatchSize;
    std::vector<int> xy = orb_pattern(c, patchSize);
    if (!c->orbTabReach || patchSize != c->orbTabPatchSize || angle != c->orbTabAngle || xy != c->orbTabPattern) {
        c->orbTabReach = 0;
        int2 tab[512];
        if ((r = upload(c, c->orbPat, xy.data(), 1024 * sizeof(int)))) return r;
        HIPCHK(c, c->orbOffTab.ensure(sizeof(tab)));
        fm3d::launch_orb_offset_table(c->orbPat.as<int>(), angle, c->orbOffTab.as<int2>(), c->stream);
        HIPCHK(c, hipGetLastError());
        HIPCHK(c, hipMemcpyAsync(tab, c->orbOffTab.p, sizeof(tab), hipMemcpyDeviceToHost, c->stream));
        HIPCHK(c, hipStreamSynchronize(c->stream));  // xy is read, tab is written
        long reach = 0;
        for (const int2& o : tab) reach = std::max({reach, std::labs((long)o.x), std::labs((long)o.y)});
        if (reach > (1 << 20)) return fail(c, FM3D_ERR_INVALID, "ORB pattern offsets out of range");
        c->orbTabPattern.swap(xy);
        c->orbTabPatchSize = patchSize;
        c->orbTabAngle = angle;
        c->orbTabReach = (int)reach + 3;  // the 7 x 7 blur around the farthest test point
    }
    // launch_orb_patch_desc has no border branch: every read of the blur lies inside the patch
    const int ctr = size / 2;
    if (ctr - c->orbTabReach < 0 || ctr + c->orbTabReach >= size)
        return fail(c, FM3D_ERR_INVALID, "ORB pattern reaches past the patch border");
    return FM3D_OK;
}

// both one-shot entry points: `any` admits the binary extractors
int one_shot(fm3d_ctx* c, bool any, const uint8_t* patches, int P, int size, void* desc) {
    if (!c || P < 0 || size <= 0 || (P && (!patches || !desc))) return FM3D_ERR_INVALID;
    PatchDesc d;
    int r;
    if ((r = patch_desc_kind(c, any, &d))) return r;
    // the binary rows start as Mat::zeros and a dropped keypoint's empty row copies nothing
    if (d.type == FM3D_DESC_BITS && P) std::memset(desc, 0, (size_t)P * d.rowBytes);
    if (d.kind == PatchDesc::Binary) {  // BRISK / FREAK: compute on each patch, kept or dropped
        const fm3d_keypoint k = patch_keypoint(size, -1.f);
        for (int p = 0; p < P; p++) {
            fm3d_keypoint ko;
            int m = 0;
            uint8_t* row = static_cast<uint8_t*>(desc) + (size_t)p * d.rowBytes;
            if ((r = fm3d_compute(c, patches + (size_t)p * size * size, size, size, &k, 1, &ko, nullptr, &m, row))) return r;
        }
        return FM3D_OK;
    }
    // SIFT's constructor checks its settings whatever the patch count
    if (d.kind == PatchDesc::Sift && (r = sift_check_settings(c))) return r;
    if (P == 0) return FM3D_OK;
    // ORB goes through the tail's chunks, uploaded one after the other.  SURF and SIFT take all P at once:
    // SIFT's launches are the faster the larger (profiles/describe_refactor.json has both)
    const int cap = d.kind == PatchDesc::Orb ? std::min(describe_chunk(), P) : P;
    if ((r = patch_desc_prepare(c, size, cap, &d))) return r;
    const size_t per = (size_t)size * size;
    HIPCHK(c, c->tailPatch.ensure((size_t)cap * per));
    HIPCHK(c, c->tailDesc.ensure((size_t)P * d.rowBytes));
    for (int p0 = 0; p0 < P; p0 += cap) {
        const int m = std::min(cap, P - p0);
        HIPCHK(c, hipMemcpyAsync(c->tailPatch.p, patches + per * p0, per * m, hipMemcpyHostToDevice, c->stream));
        if ((r = patch_desc_queue(c, d, c->tailPatch.as<uint8_t>(), p0, m, c->tailDesc.p))) return r;
    }
    if (d.kind == PatchDesc::SurfOriented) {  // a dropped keypoint is refused before any row leaves
        int kept = 0;
        HIPCHK(c, hipMemcpyAsync(&kept, c->pdKept.p, sizeof(int), hipMemcpyDeviceToHost, c->stream));
        HIPCHK(c, hipStreamSynchronize(c->stream));
        if (kept != P) return fail(c, FM3D_ERR_INVALID, "patch keypoint dropped by SURF (no orientation sample)");
    }
    HIPCHK(c, hipMemcpyAsync(desc, c->tailDesc.p, (size_t)P * d.rowBytes, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    return FM3D_OK;
}

}  // namespace

namespace fm3d_host {

fm3d_keypoint patch_keypoint(int size, float angle) {
    const float center = (float)(int)std::floor(size / 2);
    return {center, center, (float)size, angle, 1.f, 0, 0};
}

int patch_desc_kind(fm3d_ctx* c, bool any, PatchDesc* d) {
    const int ex = c->s.extractorType;
    if (ex == FM3D_FEAT_SURF)
        d->kind = c->s.surfUpright ? PatchDesc::SurfUpright : PatchDesc::SurfOriented;
    else if (ex == FM3D_FEAT_SIFT)
        d->kind = PatchDesc::Sift;
    else if (any && ex == FM3D_FEAT_ORB)
        d->kind = PatchDesc::Orb;
    else if (any && (ex == FM3D_FEAT_BRISK || ex == FM3D_FEAT_FREAK))
        d->kind = PatchDesc::Binary;
    else
        return fail(c, FM3D_ERR_UNSUPPORTED,
                    any ? "the settings' extractor type has no GPU implementation"
                        : "only the SURF and SIFT extractors describe patches on the GPU");
    d->size = 0;
    if (int r = fm3d_descriptor_info(c, &d->cols, &d->type)) return r;
    d->rowBytes = (size_t)d->cols * (d->type == FM3D_DESC_BITS ? 1 : sizeof(float));
    return FM3D_OK;
}

int patch_desc_prepare(fm3d_ctx* c, int size, int cap, PatchDesc* d) {
    int r, kept = 0;
    d->size = size;
    hipSetDevice(c->device);
    // every patch of one edge has the same keypoint: whether the extractor keeps it is one answer
    if ((r = fm3d_patch_keypoint_kept(c, size, &kept))) return fail(c, r, "patch keypoint: no keep rule");
    if (!kept && (d->kind == PatchDesc::SurfUpright || d->kind == PatchDesc::SurfOriented))
        return fail(c, FM3D_ERR_INVALID, "patch keypoint dropped by SURF (descriptor row missing)");
    if (d->kind == PatchDesc::Binary) {
        // kept from an edge of 634 (BRISK) and 680 (FREAK) only; below, every row is the reference's Mat::zeros row
        if (kept)
            return fail(c, FM3D_ERR_UNSUPPORTED,
                        "BRISK / FREAK keep the centred keypoint of a " + std::to_string(size) +
                            " px patch: no batched form, use fm3d_extract_descriptors_from_patches_any");
        return FM3D_OK;
    }
    if (d->kind == PatchDesc::Orb) return orb_prepare(c, size, kept);
    const size_t per = (size_t)size * size;
    if (d->kind == PatchDesc::Sift) {
        if ((r = ensure_taps(c)) || (r = ensure_tables(c, cap, size, -1.f))) return r;
        HIPCHK(c, c->siftBase.ensure((size_t)cap * per * sizeof(float)));
        HIPCHK(c, c->siftG.ensure((size_t)cap * per * sizeof(float)));
        return FM3D_OK;
    }
    // an upright keypoint has SURFInvoker's 270 degrees, an oriented one leaves surf_keep with its own
    const bool oriented = d->kind == PatchDesc::SurfOriented;
    if ((r = ensure_surf_dw(c)) || (r = ensure_tables(c, cap, size, oriented ? -1.f : 360.f - 90.f))) return r;
    if (!oriented) return FM3D_OK;
    if ((r = ensure_scan_tmp(c, cap))) return r;
    HIPCHK(c, c->sfSum.ensure((size_t)cap * (size + 1) * (size + 1) * sizeof(int)));
    HIPCHK(c, c->sfAng.ensure((size_t)(cap + 1) * sizeof(float)));
    HIPCHK(c, c->sfFlag.ensure((size_t)(cap + 1) * sizeof(int)));
    HIPCHK(c, c->sfPos.ensure((size_t)(cap + 1) * sizeof(int)));
    HIPCHK(c, c->sfKp.ensure((size_t)cap * sizeof(fm3d_keypoint)));
    HIPCHK(c, c->pdKept.ensure(sizeof(int)));
    return FM3D_OK;
}

int patch_desc_queue(fm3d_ctx* c, const PatchDesc& d, const uint8_t* patchesDev, int p0, int m, void* rowsDev) {
    const fm3d_settings& S = c->s;
    const int size = d.size;
    const size_t per = (size_t)size * size;
    const fm3d_keypoint* kp = c->pdKp.as<fm3d_keypoint>();
    rowsDev = static_cast<char*>(rowsDev) + (size_t)p0 * d.rowBytes;
    float* rows = static_cast<float*>(rowsDev);
    switch (d.kind) {
    case PatchDesc::Binary:  // nothing to queue: the callers do not come here
        break;
    case PatchDesc::Orb:
        fm3d::launch_orb_patch_desc(patchesDev, m, size, c->orbOffTab.as<int2>(), orb_blur_kernel(),
                                    static_cast<uint8_t*>(rowsDev), c->stream);
        break;
    case PatchDesc::Sift: {  // one init and one blur launch for all patches
        fm3d::SiftResize rp{};
        rp.sw = rp.dw = rp.sh = rp.dh = size;  // no resize, not doubled
        fm3d::launch_sift_init(patchesDev, c->siftBase.as<float>(), rp, m, c->stream);
        fm3d::launch_sift_blur(c->siftBase.as<float>(), c->siftG.as<float>(), nullptr, size, size, c->pdTaps.as<float>(),
                               c->pdNTaps, m, c->stream);
        fm3d::launch_sift_desc(c->siftG.as<float>(), c->pdGL.as<fm3d::SiftLevel>(), S.siftOctaveLayers, 0, kp,
                               c->pdLvl.as<int>(), m, rows, c->stream);
        break;
    }
    case PatchDesc::SurfOriented:
        if (p0 == 0) {
            // the first chunk is the largest.  The compacted keypoints start as the table's rows: a chunk
            // that drops one (an error at the end) still hands the describe launch valid keypoints
            HIPCHK(c, hipMemsetAsync(c->pdKept.p, 0, sizeof(int), c->stream));
            HIPCHK(c, hipMemcpyAsync(c->sfKp.p, kp, (size_t)m * sizeof(fm3d_keypoint), hipMemcpyDeviceToDevice, c->stream));
        }
        // each keypoint's orientation on its patch's integral image; one without an orientation sample
        // would lose its row (never for the centred keypoint of a patch this size, but counted)
        fm3d::launch_integral_batch(patchesDev, size, size, m, c->sfSum.as<int>(), c->stream);
        fm3d::launch_surf_orient(kp, sizeof(fm3d_keypoint), m, c->sfSum.as<int>(), (size_t)(size + 1) * (size + 1), size,
                                 size, surf_ori(), c->sfFlag.as<int>(), c->sfAng.as<float>(), c->stream);
        fm3d::launch_surf_keep(kp, m, size, size, c->sfFlag.as<int>(), c->sfPos.as<int>(), c->count.as<int>(),
                               c->scanTmp.p, c->sfKp.as<fm3d_keypoint>(), nullptr, c->sfAng.as<float>(), c->stream);
        fm3d::launch_add_count(c->count.as<int>(), c->pdKept.as<int>(), c->stream);
        kp = c->sfKp.as<fm3d_keypoint>();
        [[fallthrough]];
    case PatchDesc::SurfUpright:
        fm3d::launch_surf_describe(patchesDev, per, size, size, kp, m, c->sfDW.as<float>(), S.surfExtended,
                                   d.kind == PatchDesc::SurfUpright, rows, c->stream);
        break;
    }
    HIPCHK(c, hipGetLastError());
    return FM3D_OK;
}

}  // namespace fm3d_host

extern "C" int fm3d_extract_descriptors_from_patches(fm3d_ctx* c, const uint8_t* patches, int P, int size, float* desc) {
    return one_shot(c, false, patches, P, size, desc);
}

extern "C" int fm3d_extract_descriptors_from_patches_any(fm3d_ctx* c, const uint8_t* patches, int P, int size,
                                                          void* desc) {
    return one_shot(c, true, patches, P, size, desc);
}
