// fm3d_features.cpp -- C ABI (include/fm3d.h): fm3d_detect / fm3d_compute over the detectors and
// extractors of the fm3d_feat_*.cpp files, and the patch keypoint's keep rule.
#include "fm3d_features.h"

using namespace fm3d_host;

namespace {
// one detector call into a host vector (the entries' cap / count protocol)
template <class F>
int detect_into(F&& f, std::vector<fm3d_keypoint>& k) {
    int cap = 4096, n = 0, r;
    for (;;) {
        k.resize(cap);
        if ((r = f(k.data(), cap, &n))) return r;
        if (n <= cap) break;
        cap = n;
    }
    k.resize(n);
    return FM3D_OK;
}

// the settings' detector as it stands (STATIC, or one ADAPTIVE detector call with threshold thr)
int detect_static(fm3d_ctx* c, const uint8_t* img, int w, int h, std::vector<fm3d_keypoint>& k) {
    const fm3d_settings& S = c->s;
    switch (S.detectorType) {
    case FM3D_FEAT_SURF:
        return detect_into([&](fm3d_keypoint* p, int cap, int* n) { return fm3d_surf_detect(c, img, w, h, p, cap, n, nullptr); }, k);
    case FM3D_FEAT_ORB:
        return detect_into([&](fm3d_keypoint* p, int cap, int* n) { return fm3d_orb_detect(c, img, w, h, p, cap, n, nullptr); }, k);
    case FM3D_FEAT_SIFT:
        return detect_into([&](fm3d_keypoint* p, int cap, int* n) { return fm3d_sift_detect(c, img, w, h, p, cap, n, nullptr); }, k);
    case FM3D_FEAT_FAST:
        return fast_detect(c, img, w, h, S.fastThreshold, S.fastNonmax != 0, k);
    case FM3D_FEAT_STAR:
        return star_detect(c, img, w, h, S.starMaxSize, S.starResponse, S.starLineThreshold, S.starLineBinarized,
                           S.starSuppression, k);
    case FM3D_FEAT_MSER:
    {
        std::vector<int> per;
        return mser_detect(c, img, 1, w, h,
                           mser_params(S.mserDelta, S.mserMinArea, S.mserMaxArea, S.mserMaxVariation,
                                       S.mserMinDiversity),
                           k, per);
    }
    default:
        return fail(c, FM3D_ERR_UNSUPPORTED, "the settings' detector type has no GPU implementation");
    }
}

// DynamicAdaptedFeatureDetector(AdjusterAdapter::create(type), min, max, iters)::detect
// (features2d/src/dynamic.cpp): detect, then raise / lower the adjuster's threshold until the count
// is in [min, max], the threshold leaves the adjuster's range, the iterations run out or it
// oscillates.  FastAdjuster(20, true, 1, 200): FastFeatureDetector(thresh, true), -- / ++ by one;
// SurfAdjuster(400, 2, 1000): the default SURF (4 octaves, 2 layers, not upright) at hessianThreshold
// thresh, * 0.9 (floored at 1.1) / * 1.1; StarAdjuster(30, 2, 200): StarFeatureDetector(16,
// cvRound(thresh), 10, 8, 3), the same scaling.  The keypoints are the last call's.
int detect_adaptive(fm3d_ctx* c, const uint8_t* img, int w, int h, std::vector<fm3d_keypoint>& k) {
    const fm3d_settings S = c->s;
    const bool fast = S.detectorType == FM3D_FEAT_FAST, star = S.detectorType == FM3D_FEAT_STAR;
    if (!fast && !star && S.detectorType != FM3D_FEAT_SURF)
        return fail(c, FM3D_ERR_UNSUPPORTED, "ADAPTIVE runs the FAST, SURF and STAR adjusters");
    double thresh = fast ? 20 : star ? 30 : 400;
    const double minT = fast ? 1 : 2, maxT = fast ? 200 : star ? 200 : 1000;
    bool down = false, up = false, good = false;
    int iters = S.adaptiveMaxIters, r = FM3D_OK;
    k.clear();
    while (iters > 0 && !(down && up) && !good && thresh > minT && thresh < maxT) {
        if (fast) {
            r = fast_detect(c, img, w, h, (int)thresh, true, k);
        } else if (star) {
            r = star_detect(c, img, w, h, 16, (int)std::nearbyint(thresh), 10, 8, 3, k);
        } else {
            fm3d_settings t = S;  // FeatureDetector::create("SURF") + set("hessianThreshold", thresh)
            t.detectorMode = 0;
            t.surfHessianThreshold = thresh;
            t.surfOctaves = 4;
            t.surfOctaveLayers = 2;
            t.surfExtended = 0;
            t.surfUpright = 0;
            c->s = t;
            r = detect_static(c, img, w, h, k);
            c->s = S;
        }
        if (r) return r;
        if ((int)k.size() < S.adaptiveMinFeatures) {
            down = true;
            if (fast)
                thresh -= 1;
            else if ((thresh *= 0.9) < 1.1)
                thresh = 1.1;
        } else if ((int)k.size() > S.adaptiveMaxFeatures) {
            up = true;
            if (fast)
                thresh += 1;
            else
                thresh *= 1.1;
        } else {
            good = true;
        }
        iters--;
    }
    return FM3D_OK;
}
}  // namespace

extern "C" {

int fm3d_detect(fm3d_ctx* c, const uint8_t* img, int w, int h, fm3d_keypoint* kpts, int cap, int* n) {
    if (!c || !img || !n || w <= 0 || h <= 0 || cap < 0 || (cap > 0 && !kpts)) return FM3D_ERR_INVALID;
    hipSetDevice(c->device);
    std::vector<fm3d_keypoint> k;
    int r = c->s.detectorMode == 1 ? detect_adaptive(c, img, w, h, k) : detect_static(c, img, w, h, k);
    if (r) return r;
    for (int i = 0; i < (int)k.size() && i < cap; i++) kpts[i] = k[i];
    *n = (int)k.size();
    return FM3D_OK;
}

int fm3d_descriptor_info(const fm3d_ctx* c, int* cols, int* type) {
    if (!c || !cols || !type) return FM3D_ERR_INVALID;
    switch (c->s.extractorType) {
    case FM3D_FEAT_SURF:
        *cols = c->s.surfExtended ? 128 : 64;
        *type = FM3D_DESC_F32;
        return FM3D_OK;
    case FM3D_FEAT_SIFT:
        *cols = 128;
        *type = FM3D_DESC_F32;
        return FM3D_OK;
    case FM3D_FEAT_ORB:
        *cols = 32;
        *type = FM3D_DESC_BITS;
        return FM3D_OK;
    case FM3D_FEAT_BRISK:
    case FM3D_FEAT_FREAK:
        *cols = 64;
        *type = FM3D_DESC_BITS;
        return FM3D_OK;
    default:
        return FM3D_ERR_UNSUPPORTED;
    }
}

int fm3d_compute(fm3d_ctx* c, const uint8_t* img, int w, int h, const fm3d_keypoint* kpts, int n, fm3d_keypoint* kout,
                 int32_t* kept, int* nOut, void* desc) {
    switch (c ? c->s.extractorType : FM3D_FEAT_OTHER) {
    case FM3D_FEAT_SURF:
        return fm3d_surf_compute(c, img, w, h, kpts, n, kout, kept, nOut, static_cast<float*>(desc));
    case FM3D_FEAT_SIFT:
        return fm3d_sift_compute(c, img, w, h, kpts, n, kout, kept, nOut, static_cast<float*>(desc));
    case FM3D_FEAT_ORB:
        return fm3d_orb_compute(c, img, w, h, kpts, n, kout, kept, nOut, static_cast<uint8_t*>(desc));
    case FM3D_FEAT_BRISK:
        return fm3d_brisk_compute(c, img, w, h, kpts, n, kout, kept, nOut, static_cast<uint8_t*>(desc));
    case FM3D_FEAT_FREAK:
        return fm3d_freak_compute(c, img, w, h, kpts, n, kout, kept, nOut, static_cast<uint8_t*>(desc));
    default:
        return c ? fail(c, FM3D_ERR_UNSUPPORTED, "the settings' extractor type has no GPU implementation")
                 : FM3D_ERR_INVALID;
    }
}

int fm3d_patch_keypoint_kept_for(const fm3d_settings* s, int size, int* kept) {
    if (!s || !kept || size <= 0) return FM3D_ERR_INVALID;
    // the keypoint of every patch of this edge, on a size x size image
    const fm3d_keypoint k = patch_keypoint(size, -1.f);
    const float ctr = k.x, ks = k.size;
    switch (s->extractorType) {
    case FM3D_FEAT_SURF:  // fm3d_surf_compute: the wavelet, 2 * cvRound(2 s) wide, against the image
        *kept = size + 1 >= 2 * (int)std::lrint(2 * (ks * 1.2f / 9.0f));
        return FM3D_OK;
    case FM3D_FEAT_SIFT:
        *kept = 1;
        return FM3D_OK;
    case FM3D_FEAT_ORB: {  // fm3d_orb_compute: runByImageBorder(edgeThreshold) on the rounded position
        const int b = s->orbEdgeThreshold;
        const long i = std::lrint(ctr);
        *kept = b <= 0 || (size > 2 * b && i >= b && i < b + (size - 2 * b));
        return FM3D_OK;
    }
    case FM3D_FEAT_BRISK: {  // brisk_compute: the scale's pattern size as the border
        const int b = brisk_border(ks);
        *kept = !(ctr < (float)b || ctr >= (float)(size - b));
        return FM3D_OK;
    }
    case FM3D_FEAT_FREAK: {  // freak_compute
        const float ps = (float)freak_border(ks);
        *kept = !(ctr <= ps || ctr >= size - ps);
        return FM3D_OK;
    }
    default:
        return FM3D_ERR_UNSUPPORTED;
    }
}

int fm3d_patch_keypoint_kept(const fm3d_ctx* c, int size, int* kept) {
    return c ? fm3d_patch_keypoint_kept_for(&c->s, size, kept) : FM3D_ERR_INVALID;
}

}  // extern "C"
