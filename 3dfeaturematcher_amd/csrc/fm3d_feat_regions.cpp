// fm3d_feat_regions.cpp -- C ABI (include/fm3d.h): the STAR and MSER detectors, the host side of
// fm3d_star.hip and fm3d_mser.hip.
#include <cstdlib>
#include <string>

#include "fm3d_features.h"

using namespace fm3d_host;

namespace {

// StarDetector(maxSize, response, lineProj, lineBin, supp)(img) (features2d/src/stardetector.cpp):
// the pattern set on the host (StarDetectorComputeResponses' loop), the integrals, responses and tile
// suppression on the GPU (fm3d_star.hip), keypoints in tile order.  Undefined in OpenCV (and
// FM3D_ERR_INVALID here): min(w, h) <= 6, maxSize > 128; a suppression window wider than the border
// (the reference reads outside the image) too.
int star_patterns(int w, int h, int maxSize, fm3d::StarPat& P) {
    static const int sizes0[17] = {1, 2, 3, 4, 6, 8, 11, 12, 16, 22, 23, 32, 45, 46, 64, 90, 128};
    static const int pairs[12][2] = {{1, 0}, {3, 1}, {4, 2}, {5, 3}, {7, 4}, {8, 5},
                                     {9, 6}, {11, 8}, {13, 10}, {14, 11}, {15, 12}, {16, 14}};
    const int st = w + 1, mn = std::min(w, h);
    if (maxSize > 128 || mn <= 6) return 0;
    int np = 0;
    while (np < 12 && !(sizes0[pairs[np][0]] >= maxSize ||
                        sizes0[pairs[np + 1][0]] + sizes0[pairs[np + 1][0]] / 2 >= mn))
        np++;
    if (np == 0) return 0;
    np = std::min(np + 1, 12);  // the first pattern past the range stays, for the size rejection
    memset(&P, 0, sizeof(P));
    P.np = np;
    P.maxIdx = pairs[np - 1][0];
    int area[17];
    for (int i = 0; i <= P.maxIdx; i++) {
        const int u = sizes0[i], t = u + u / 2;
        int* o = P.ofs + 8 * i;
        o[0] = (u + 1) * st + u + 1;
        o[1] = -u * st + u + 1;
        o[2] = (u + 1) * st - u;
        o[3] = -u * st - u;
        o[4] = (t + 1) * st + 1;
        o[5] = -t;
        o[6] = t + 1;
        o[7] = -t * st + 1;
        area[i] = (2 * u + 1) * (2 * u + 1) + t * t + (t + 1) * (t + 1);
        P.sizes1[i] = u;
    }
    P.sizes1[0] = -P.sizes1[0];
    P.sizes1[1] = -P.sizes1[1];
    P.sizes1[P.maxIdx] = -P.sizes1[P.maxIdx];
    P.border = sizes0[P.maxIdx] + sizes0[P.maxIdx] / 2;
    P.nsimd = w - 2 * P.border >= 0 ? 4 * ((w - 2 * P.border) / 4) : 0;
    for (int i = 0; i < np; i++) {
        const int inner = area[pairs[i][1]], outer = area[pairs[i][0]] - inner;
        P.inv[2 * i] = 1.f / (float)outer;
        P.inv[2 * i + 1] = 1.f / (float)inner;
    }
    return np;
}

// the image, its integrals and StarDetectorComputeResponses' maps on the device (starR, starZ)
int star_responses(fm3d_ctx* c, const uint8_t* img, int w, int h, int maxSize, fm3d::StarPat& P) {
    if (!star_patterns(w, h, maxSize, P))
        return fail(c, FM3D_ERR_INVALID, "STAR: undefined for min(w, h) <= 6 or MaxSize > 128");
    // FM3D_STAR_TILT=rows: the one-workgroup row walk (A/B knob); default: the diagonal scans
    const char* tilt = getenv("FM3D_STAR_TILT");
    const bool rows = tilt && std::string(tilt) == "rows";
    if (rows && (w > fm3d::star_tilted_max_width() || fm3d::star_tilted_lds_bytes(w) > 160 * 1024))
        return fail(c, FM3D_ERR_INVALID, "STAR: image wider than 6,000 pixels for the row walk");
    const long long W1H1 = (long long)(w + 1) * (h + 1), WH = (long long)w * h;
    if (W1H1 > INT32_MAX / 4) return fail(c, FM3D_ERR_INVALID, "image too large for STAR");
    HIPCHK(c, c->starImg.ensure((size_t)WH));
    HIPCHK(c, c->starS.ensure((size_t)W1H1 * sizeof(int)));
    HIPCHK(c, c->starT.ensure((size_t)W1H1 * sizeof(int)));
    HIPCHK(c, c->starF.ensure((size_t)W1H1 * sizeof(int)));
    HIPCHK(c, c->starR.ensure((size_t)WH * sizeof(float)));
    HIPCHK(c, c->starZ.ensure((size_t)WH * sizeof(short)));
    HIPCHK(c, hipMemcpyAsync(c->starImg.p, img, (size_t)WH, hipMemcpyHostToDevice, c->stream));
    fm3d::launch_integral(c->starImg.as<uint8_t>(), w, h, c->starS.as<int>(), c->stream);
    if (rows) {
        fm3d::launch_star_tilted(c->starImg.as<uint8_t>(), w, h, c->starT.as<int>(), c->starF.as<int>(), c->stream);
    } else {
        HIPCHK(c, c->starWork.ensure(fm3d::star_diag_bytes(w, h)));
        fm3d::launch_star_tilted_diag(c->starImg.as<uint8_t>(), w, h, c->starWork.p, c->starT.as<int>(),
                                      c->starF.as<int>(), c->stream);
    }
    fm3d::launch_star_resp(c->starS.as<int>(), c->starT.as<int>(), c->starF.as<int>(), w, h, P, c->starR.as<float>(),
                           c->starZ.as<short>(), c->stream);
    HIPCHK(c, hipGetLastError());
    return FM3D_OK;
}

// MSER (fm3d_mser.hip): the floods of `count` images (two per image, slot = 2 * image + pass), then the
// regions' records and point offsets.  regs: every slot's regions in slot order ({colour, head node,
// count, slot}); off: their prefix (points before each).
int mser_flood(fm3d_ctx* c, const uint8_t* img, int count, int w, int h, const fm3d::MserParams& P,
               fm3d::MserLayout& L, std::vector<int4>& regs, std::vector<long long>& off) {
    if (w <= 0 || h <= 0 || count <= 0) return fail(c, FM3D_ERR_INVALID, "MSER: empty image");
    if ((long long)(w + 2) * (h + 2) >= (1LL << 28) - 1 || w > 65535 || h > 65535)
        return fail(c, FM3D_ERR_INVALID, "MSER: image too large");
    if ((long long)2 * count * w * h >= (1LL << 30)) return fail(c, FM3D_ERR_INVALID, "MSER: batch too large");
    const int slots = 2 * count;
    L = fm3d::mser_layout(w, h);
    HIPCHK(c, c->msImg.ensure((size_t)count * w * h));
    HIPCHK(c, c->msPad.ensure((size_t)slots * L.padBytes));
    HIPCHK(c, c->msWork.ensure(L.visInLds ? 16 : (size_t)slots * L.visWords * sizeof(unsigned)));
    HIPCHK(c, c->msHeap.ensure((size_t)slots * L.heapEntries * sizeof(int2)));
    HIPCHK(c, c->msNode.ensure((size_t)slots * L.nodes * sizeof(int2)));
    HIPCHK(c, c->msHist.ensure((size_t)slots * L.hists * sizeof(fm3d::MserHist)));
    HIPCHK(c, c->msReg.ensure((size_t)slots * L.regCap * sizeof(int4)));
    HIPCHK(c, c->msCnt.ensure((size_t)slots * sizeof(int)));
    HIPCHK(c, hipMemcpyAsync(c->msImg.p, img, (size_t)count * w * h, hipMemcpyHostToDevice, c->stream));
    fm3d::launch_mser_flood(c->msImg.as<uint8_t>(), count, L, P, c->msPad.as<uint8_t>(), c->msWork.as<unsigned>(),
                            c->msHeap.as<int2>(), c->msNode.as<int2>(), c->msHist.as<fm3d::MserHist>(),
                            c->msReg.as<int4>(), c->msCnt.as<int>(), c->stream);
    HIPCHK(c, hipGetLastError());
    std::vector<int> cnt(slots, 0);
    HIPCHK(c, hipMemcpyAsync(cnt.data(), c->msCnt.p, (size_t)slots * sizeof(int), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    long long total = 0;
    for (int k = 0; k < slots; k++) {
        if (cnt[k] < 0 || cnt[k] > L.regCap) return fail(c, FM3D_ERR_HIP, "MSER: region count out of range");
        total += cnt[k];
    }
    regs.resize((size_t)total);
    for (int k = 0, at = 0; k < slots; at += cnt[k], k++)
        if (cnt[k])
            HIPCHK(c, hipMemcpyAsync(regs.data() + at, c->msReg.as<int4>() + (size_t)k * L.regCap,
                                     (size_t)cnt[k] * sizeof(int4), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    off.assign(regs.size() + 1, 0);
    for (int k = 0, i = 0; k < slots; k++)
        for (int j = 0; j < cnt[k]; j++, i++) {
            if (regs[i].z <= 0 || regs[i].z > (long long)w * h) return fail(c, FM3D_ERR_HIP, "MSER: bad region size");
            regs[i].w = k;
            off[i + 1] = off[i] + regs[i].z;
        }
    return FM3D_OK;
}

// the region points (gathered from the ranked node lists) and each region's fitEllipse keypoint + kept flag
int mser_fit(fm3d_ctx* c, const fm3d::MserLayout& L, int count, const std::vector<int4>& regs,
             const std::vector<long long>& off) {
    const int n = (int)regs.size();
    if (n == 0) return FM3D_OK;
    const long long tot = off[n];
    HIPCHK(c, c->msOff.ensure((size_t)(n + 1) * sizeof(long long)));
    HIPCHK(c, c->msRegC.ensure((size_t)n * sizeof(int4)));
    HIPCHK(c, c->msXY.ensure((size_t)tot * sizeof(int2)));
    HIPCHK(c, c->msScr.ensure((size_t)tot * 5 * sizeof(double)));
    HIPCHK(c, c->msKp.ensure((size_t)(n + 1) * sizeof(fm3d_keypoint)));
    HIPCHK(c, c->msFlag.ensure((size_t)(n + 1) * sizeof(int)));
    HIPCHK(c, hipMemcpyAsync(c->msOff.p, off.data(), (size_t)(n + 1) * sizeof(long long), hipMemcpyHostToDevice,
                             c->stream));
    HIPCHK(c, hipMemcpyAsync(c->msRegC.p, regs.data(), (size_t)n * sizeof(int4), hipMemcpyHostToDevice, c->stream));
    HIPCHK(c, c->msRank.ensure(fm3d::mser_rank_bytes(L.nodes, 2 * count)));
    const fm3d::MserRank K =
        fm3d::launch_mser_rank(c->msNode.as<int2>(), L.nodes, 2 * count, c->msRank.as<int>(), c->stream);
    fm3d::launch_mser_fit(c->msRegC.as<int4>(), n, K, L.nodes, c->msOff.as<long long>(), L, c->msXY.as<int2>(),
                          c->msScr.as<double>(), c->msKp.as<fm3d_keypoint>(), c->msFlag.as<int>(), nullptr, c->stream);
    HIPCHK(c, hipGetLastError());
    return FM3D_OK;
}

}  // namespace

namespace fm3d_host {

int star_detect(fm3d_ctx* c, const uint8_t* img, int w, int h, int maxSize, int respThr, int lineProj, int lineBin,
                int supp, std::vector<fm3d_keypoint>& k) {
    k.clear();
    fm3d::StarPat P;
    if (!star_patterns(w, h, maxSize, P))
        return fail(c, FM3D_ERR_INVALID, "STAR: undefined for min(w, h) <= 6 or MaxSize > 128");
    const int delta = supp / 2;
    if (delta < 0 || delta > P.border) return fail(c, FM3D_ERR_INVALID, "STAR: Suppression wider than the border");
    fm3d::StarNms N{P.border, delta, 0, 0, respThr, lineProj, lineBin};
    if (h - 2 * P.border > 0 && w - 2 * P.border > 0) {
        N.ny = (h - 2 * P.border + delta) / (delta + 1);
        N.nx = (w - 2 * P.border + delta) / (delta + 1);
    }
    const int nslot = 2 * N.nx * N.ny;
    int r;
    if ((r = ensure_scan_tmp(c, std::max(nslot, 1)))) return r;
    HIPCHK(c, c->starKp.ensure((size_t)(nslot + 1) * sizeof(fm3d_keypoint)));
    HIPCHK(c, c->starFlag.ensure((size_t)(nslot + 1) * sizeof(int)));
    HIPCHK(c, c->starPos.ensure((size_t)(nslot + 1) * sizeof(int)));
    if ((r = star_responses(c, img, w, h, maxSize, P))) return r;
    if (nslot == 0) {
        HIPCHK(c, hipStreamSynchronize(c->stream));
        return FM3D_OK;
    }
    fm3d::launch_star_nms(c->starR.as<float>(), c->starZ.as<short>(), w, h, N, c->starKp.as<fm3d_keypoint>(),
                          c->starFlag.as<int>(), c->stream);
    fm3d::launch_exclusive_scan(c->starFlag.as<int>(), nslot, c->starPos.as<int>(), c->count.as<int>(), c->scanTmp.p,
                                c->stream);
    HIPCHK(c, hipGetLastError());
    int nk = 0;
    HIPCHK(c, hipMemcpyAsync(&nk, c->count.p, sizeof(int), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    if (nk == 0) return FM3D_OK;
    HIPCHK(c, c->starOut.ensure((size_t)nk * sizeof(fm3d_keypoint)));
    fm3d::launch_star_scatter(c->starKp.as<fm3d_keypoint>(), c->starFlag.as<int>(), c->starPos.as<int>(), nslot,
                              c->starOut.as<fm3d_keypoint>(), c->stream);
    HIPCHK(c, hipGetLastError());
    k.resize(nk);
    HIPCHK(c, hipMemcpyAsync(k.data(), c->starOut.p, (size_t)nk * sizeof(fm3d_keypoint), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    return FM3D_OK;
}

fm3d::MserParams mser_params(int delta, int minArea, int maxArea, double maxVariation, double minDiversity) {
    fm3d::MserParams P;
    P.delta = delta;
    P.minArea = minArea;
    P.maxArea = maxArea;
    P.maxVariation = maxVariation;
    P.minDiversity = minDiversity;
    return P;
}

// MserFeatureDetector::detect on `count` images: the kept keypoints of each image in region order,
// image after image; per[i] = image i's count
int mser_detect(fm3d_ctx* c, const uint8_t* img, int count, int w, int h, const fm3d::MserParams& P,
                std::vector<fm3d_keypoint>& k, std::vector<int>& per) {
    k.clear();
    per.assign(count, 0);
    fm3d::MserLayout L;
    std::vector<int4> regs;
    std::vector<long long> off;
    int r;
    if ((r = mser_flood(c, img, count, w, h, P, L, regs, off))) return r;
    const int n = (int)regs.size();
    for (int i = 0; i < n; i++)
        if (regs[i].z < 5) return fail(c, FM3D_ERR_INVALID, "MSER: a region under 5 points (fitEllipse throws)");
    if (n == 0) return FM3D_OK;
    if ((r = mser_fit(c, L, count, regs, off))) return r;
    if ((r = ensure_scan_tmp(c, n))) return r;
    HIPCHK(c, c->msPos.ensure((size_t)(n + 1) * sizeof(int)));
    fm3d::launch_exclusive_scan(c->msFlag.as<int>(), n, c->msPos.as<int>(), c->count.as<int>(), c->scanTmp.p, c->stream);
    HIPCHK(c, hipGetLastError());
    int nk = 0;
    std::vector<int> pos(n);
    HIPCHK(c, hipMemcpyAsync(&nk, c->count.p, sizeof(int), hipMemcpyDeviceToHost, c->stream));
    if (count > 1) HIPCHK(c, hipMemcpyAsync(pos.data(), c->msPos.p, (size_t)n * sizeof(int), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    if (count == 1) {
        per[0] = nk;
    } else {  // image i's keypoints: the kept regions of slots 2i and 2i + 1
        std::vector<int> first(count + 1, n);  // image i's first region (n: past the end)
        for (int i = n - 1; i >= 0; i--) first[regs[i].w >> 1] = i;
        for (int i = count - 1; i >= 0; i--)
            if (first[i] == n) first[i] = first[i + 1];  // an image without regions
        auto at = [&](int f) { return f < n ? pos[f] : nk; };
        for (int i = 0; i < count; i++) per[i] = at(first[i + 1]) - at(first[i]);
    }
    if (nk == 0) return FM3D_OK;
    HIPCHK(c, c->msOut.ensure((size_t)nk * sizeof(fm3d_keypoint)));
    fm3d::launch_star_scatter(c->msKp.as<fm3d_keypoint>(), c->msFlag.as<int>(), c->msPos.as<int>(), n,
                              c->msOut.as<fm3d_keypoint>(), c->stream);
    HIPCHK(c, hipGetLastError());
    k.resize(nk);
    HIPCHK(c, hipMemcpyAsync(k.data(), c->msOut.p, (size_t)nk * sizeof(fm3d_keypoint), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    return FM3D_OK;
}

}  // namespace fm3d_host

extern "C" {

int fm3d_mser_detect(fm3d_ctx* c, const uint8_t* img, int w, int h, int delta, int minArea, int maxArea,
                     double maxVariation, double minDiversity, fm3d_keypoint* kpts, int cap, int* n) {
    int32_t count = 0;  // a batch of one image
    return fm3d_mser_detect_batch(c, img, 1, w, h, delta, minArea, maxArea, maxVariation, minDiversity, kpts, cap,
                                  &count, n);
}

int fm3d_mser_detect_batch(fm3d_ctx* c, const uint8_t* imgs, int count, int w, int h, int delta, int minArea,
                           int maxArea, double maxVariation, double minDiversity, fm3d_keypoint* kpts, int cap,
                           int32_t* counts, int* total) {
    if (!c || !imgs || !counts || !total || count <= 0 || w <= 0 || h <= 0 || cap < 0 || (cap > 0 && !kpts))
        return FM3D_ERR_INVALID;
    hipSetDevice(c->device);
    std::vector<fm3d_keypoint> k;
    std::vector<int> per;
    int r;
    if ((r = mser_detect(c, imgs, count, w, h, mser_params(delta, minArea, maxArea, maxVariation, minDiversity), k,
                         per)))
        return r;
    for (int i = 0; i < (int)k.size() && i < cap; i++) kpts[i] = k[i];
    for (int i = 0; i < count; i++) counts[i] = per[i];
    *total = (int)k.size();
    return FM3D_OK;
}

int fm3d_mser_regions(fm3d_ctx* c, const uint8_t* img, int w, int h, int delta, int minArea, int maxArea,
                      double maxVariation, double minDiversity, int32_t* color, int32_t* count, int cap, int32_t* pts,
                      int64_t ptsCap, int* nRegions, int64_t* nPoints) {
    if (!c || !img || !nRegions || !nPoints || w <= 0 || h <= 0 || cap < 0 || ptsCap < 0 ||
        (cap > 0 && (!color || !count)) || (ptsCap > 0 && !pts))
        return FM3D_ERR_INVALID;
    hipSetDevice(c->device);
    fm3d::MserLayout L;
    std::vector<int4> regs;
    std::vector<long long> off;
    int r;
    const fm3d::MserParams P = mser_params(delta, minArea, maxArea, maxVariation, minDiversity);
    if ((r = mser_flood(c, img, 1, w, h, P, L, regs, off))) return r;
    const int n = (int)regs.size();
    if ((r = mser_fit(c, L, 1, regs, off))) return r;  // gathers the region points into msXY
    const long long tot = off[n];
    for (int i = 0; i < n && i < cap; i++) {
        color[i] = regs[i].x;
        count[i] = regs[i].z;
    }
    const long long m = std::min<long long>(tot, ptsCap);
    if (m > 0)
        HIPCHK(c, hipMemcpyAsync(pts, c->msXY.p, (size_t)m * sizeof(int2), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    *nRegions = n;
    *nPoints = tot;
    return FM3D_OK;
}

int fm3d_star_responses(fm3d_ctx* c, const uint8_t* img, int w, int h, int maxSize, float* resp, int16_t* sizes,
                        int* border) {
    if (!c || !img || !resp || !sizes || !border || w <= 0 || h <= 0) return FM3D_ERR_INVALID;
    hipSetDevice(c->device);
    fm3d::StarPat P;
    int r;
    if ((r = star_responses(c, img, w, h, maxSize, P))) return r;
    HIPCHK(c, hipMemcpyAsync(resp, c->starR.p, (size_t)w * h * sizeof(float), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipMemcpyAsync(sizes, c->starZ.p, (size_t)w * h * sizeof(int16_t), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    *border = P.border;
    return FM3D_OK;
}

int fm3d_star_detect(fm3d_ctx* c, const uint8_t* img, int w, int h, int maxSize, int response, int lineThreshold,
                     int lineBinarized, int suppression, fm3d_keypoint* kpts, int cap, int* n) {
    if (!c || !img || !n || w <= 0 || h <= 0 || cap < 0 || (cap > 0 && !kpts)) return FM3D_ERR_INVALID;
    hipSetDevice(c->device);
    std::vector<fm3d_keypoint> k;
    int r;
    if ((r = star_detect(c, img, w, h, maxSize, response, lineThreshold, lineBinarized, suppression, k))) return r;
    for (int i = 0; i < (int)k.size() && i < cap; i++) kpts[i] = k[i];
    *n = (int)k.size();
    return FM3D_OK;
}

}  // extern "C"
