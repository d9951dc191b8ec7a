// fm3d_feat_binary.cpp -- C ABI (include/fm3d.h): the BRISK and FREAK extractors, the host side of
// fm3d_brisk.hip and fm3d_freak.hip.
#include "fm3d_features.h"
#include "fm3d_freak.h"

using namespace fm3d_host;

// ---------------------------------------------------------------- BRISK extractor
// cv::BRISK's descriptor on given keypoints (OpenCV 2.4.9 brisk.cpp; oracle/orc_brisk.c): what OpenCV's
// constructor precomputes (pattern points per scale and rotation, the short pairs, the size list) and
// its per-keypoint bookkeeping (scale, rotation bin, border filter) stay on the host, in the same
// float / double expressions and glibc calls; the intensities and bits run on the GPU.
namespace {
namespace brisk {
constexpr int kScales = 64, kRot = 1024, kPoints = 60;
const int kNum[5] = {1, 10, 14, 15, 20};
void radii(float* r) {
    const double f = 0.85 * 1.0;
    r[0] = (float)(f * 0.);
    r[1] = (float)(f * 2.9);
    r[2] = (float)(f * 4.9);
    r[3] = (float)(f * 7.4);
    r[4] = (float)(f * 10.8);
}
float scale_factor(int scale) {
    const float lb_scale = (float)(std::log(30.0) / std::log(2.0));
    const float step = lb_scale / kScales;
    return (float)std::pow(2.0, (double)(scale * step));
}
void point(int scale, int rot, int i, float& px, float& py, float& sg, int* ringOut = nullptr) {
    float r[5];
    radii(r);
    const float sc = scale_factor(scale);
    const double theta = (double)rot * 2 * M_PI / (double)kRot;
    int ring = 0, num = i;
    while (num >= kNum[ring]) num -= kNum[ring++];
    const double alpha = (double)num * 2 * M_PI / (double)kNum[ring];
    const float rr = sc * r[ring];
    px = (float)(rr * std::cos(alpha + theta));
    py = (float)(rr * std::sin(alpha + theta));
    sg = ring == 0 ? 1.3f * sc * 0.5f : (float)(1.3f * sc * (double)r[ring] * std::sin(M_PI / kNum[ring]));
    if (ringOut) *ringOut = ring;
}
int size_of(int scale) {
    float r[5];
    radii(r);
    const float sc = scale_factor(scale);
    int best = 0;
    for (int i = 0; i < kPoints; i++) {
        float x, y, sg;
        int ring;
        point(scale, 0, i, x, y, sg, &ring);
        best = std::max(best, (int)std::ceil(sc * r[ring] + sg) + 1);
    }
    return best;
}
int kscale(float size) {
    const float log2c = 0.693147180559945f;
    const float lb = (float)(logf(30.f) / log2c);
    const float b06 = 12.0f * 0.6f;
    int s = (int)(kScales / lb * (logf(size / b06) / log2c) + 0.5);
    return std::min(std::max(s, 0), kScales - 1);
}
int theta(float angle) {
    if (angle == -1) return 0;
    int t = (int)(kRot * (angle / 360.0) + 0.5);
    if (t < 0) t += kRot;
    if (t >= kRot) t -= kRot;
    return t;
}
std::vector<int> short_pairs() {  // (i, j) interleaved, in generation order
    const float dMin = (float)(8.2 * 1.0), dMax = (float)(5.85 * 1.0);
    const float dMin_sq = dMin * dMin, dMax_sq = dMax * dMax;
    float X[kPoints], Y[kPoints], sg;
    for (int i = 0; i < kPoints; i++) point(0, 0, i, X[i], Y[i], sg);
    std::vector<int> p;
    for (int i = 1; i < kPoints; i++)
        for (int j = 0; j < i; j++) {
            const float dx = X[j] - X[i], dy = Y[j] - Y[i];
            const float n2 = dx * dx + dy * dy;
            if (n2 > dMin_sq) continue;
            if (n2 < dMax_sq) {
                p.push_back(i);
                p.push_back(j);
            }
        }
    return p;
}
}  // namespace brisk

int brisk_compute(fm3d_ctx* c, const uint8_t* img, int w, int h, const fm3d_keypoint* kpts, int n, fm3d_keypoint* kout,
                  int32_t* kept, int* nOut, uint8_t* desc) {
    static const std::vector<int> pairs = brisk::short_pairs();
    static const std::vector<int> sizes = [] {
        std::vector<int> v(brisk::kScales);
        for (int s = 0; s < brisk::kScales; s++) v[s] = brisk::size_of(s);
        return v;
    }();
    *nOut = 0;
    // runByKeypointSize(FLT_EPSILON), then the scale-dependent border (RoiPredicate), order kept
    std::vector<fm3d_keypoint> K;
    std::vector<int> src, combo;
    std::vector<long> keys;
    for (int q = 0; q < n; q++) {
        const fm3d_keypoint& k = kpts[q];
        if (!(k.size >= FLT_EPSILON)) continue;
        const int sc = brisk::kscale(k.size), b = sizes[sc];
        if (k.x < (float)b || k.x >= (float)(w - b) || k.y < (float)b || k.y >= (float)(h - b)) continue;
        K.push_back(k);
        src.push_back(q);
        keys.push_back((long)sc * brisk::kRot + brisk::theta(k.angle));
    }
    const int m = (int)K.size();
    if (m == 0) return FM3D_OK;
    // the pattern rows in use
    std::vector<long> uniq(keys);
    std::sort(uniq.begin(), uniq.end());
    uniq.erase(std::unique(uniq.begin(), uniq.end()), uniq.end());
    std::vector<float> pat(uniq.size() * brisk::kPoints * 4, 0.f);
    for (size_t u = 0; u < uniq.size(); u++)
        for (int i = 0; i < brisk::kPoints; i++) {
            float* p = &pat[(u * brisk::kPoints + i) * 4];
            brisk::point((int)(uniq[u] / brisk::kRot), (int)(uniq[u] % brisk::kRot), i, p[0], p[1], p[2]);
        }
    std::vector<int> pidx(m);
    for (int i = 0; i < m; i++) pidx[i] = (int)(std::lower_bound(uniq.begin(), uniq.end(), keys[i]) - uniq.begin());
    const long long W1H1 = (long long)(w + 1) * (h + 1);
    if (W1H1 > INT32_MAX / 4) return fail(c, FM3D_ERR_INVALID, "image too large for BRISK");
    HIPCHK(c, c->brImg.ensure((size_t)w * h));
    HIPCHK(c, c->brSum.ensure((size_t)W1H1 * sizeof(int)));
    HIPCHK(c, c->brKp.ensure((size_t)m * sizeof(fm3d_keypoint)));
    HIPCHK(c, c->brIdx.ensure((size_t)m * sizeof(int)));
    HIPCHK(c, c->brPat.ensure(pat.size() * sizeof(float)));
    HIPCHK(c, c->brPairs.ensure(pairs.size() * sizeof(int)));
    HIPCHK(c, c->brDesc.ensure((size_t)m * 64));
    HIPCHK(c, hipMemcpyAsync(c->brImg.p, img, (size_t)w * h, hipMemcpyHostToDevice, c->stream));
    HIPCHK(c, hipMemcpyAsync(c->brKp.p, K.data(), (size_t)m * sizeof(fm3d_keypoint), hipMemcpyHostToDevice, c->stream));
    HIPCHK(c, hipMemcpyAsync(c->brIdx.p, pidx.data(), (size_t)m * sizeof(int), hipMemcpyHostToDevice, c->stream));
    HIPCHK(c, hipMemcpyAsync(c->brPat.p, pat.data(), pat.size() * sizeof(float), hipMemcpyHostToDevice, c->stream));
    HIPCHK(c, hipMemcpyAsync(c->brPairs.p, pairs.data(), pairs.size() * sizeof(int), hipMemcpyHostToDevice, c->stream));
    fm3d::launch_integral(c->brImg.as<uint8_t>(), w, h, c->brSum.as<int>(), c->stream);
    fm3d::launch_brisk_desc(c->brImg.as<uint8_t>(), c->brSum.as<int>(), w, c->brKp.as<fm3d_keypoint>(),
                            c->brIdx.as<int>(), m, c->brPat.as<float4>(), c->brPairs.as<int2>(), (int)pairs.size() / 2,
                            c->brDesc.as<uint8_t>(), c->stream);
    HIPCHK(c, hipGetLastError());
    HIPCHK(c, hipMemcpyAsync(desc, c->brDesc.p, (size_t)m * 64, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    for (int i = 0; i < m; i++) {
        kout[i] = K[i];
        if (kept) kept[i] = src[i];
    }
    *nOut = m;
    return FM3D_OK;
}

// ---------------------------------------------------------------- FREAK extractor
// cv::FREAK() on given keypoints (OpenCV 2.4.9 freak.cpp; oracle/orc_freak.c): FREAK::buildPattern's
// tables (the 43 points of each of the 64 scales and 256 orientations in glibc's double cos / sin, the
// pattern sizes, the orientation weights) and the per-keypoint scale and border filter stay on the
// host in the same float / double expressions and glibc calls; intensities, orientation and bits run
// on the GPU (fm3d_freak.hip).
namespace freak {
constexpr float kPatternScale = 22.0f;  // cv::FREAK() defaults
constexpr int kOctaves = 4;
struct Pattern {
    std::vector<float4> lut;  // (x, y, sigma, 0) per (scale, orientation, point)
    int sizes[fm3d::kFreakScales];
    int op[4 * fm3d::kFreakOrientPairs];  // (i, j, weight_dx, weight_dy)
};
const Pattern& pattern() {
    static const Pattern P = [] {
        Pattern p;
        const int n[8] = {6, 6, 6, 6, 6, 6, 6, 1};
        const double bigR = 2.0 / 3.0, smallR = 2.0 / 24.0;
        const double unitSpace = (bigR - smallR) / 21.0;
        const double radius[8] = {bigR, bigR - 6 * unitSpace, bigR - 11 * unitSpace, bigR - 15 * unitSpace,
                                  bigR - 18 * unitSpace, bigR - 20 * unitSpace, smallR, 0.0};
        const double sigma[8] = {radius[0] / 2.0, radius[1] / 2.0, radius[2] / 2.0, radius[3] / 2.0,
                                 radius[4] / 2.0, radius[5] / 2.0, radius[6] / 2.0, radius[6] / 2.0};
        const double scaleStep = std::pow(2.0, (double)kOctaves / fm3d::kFreakScales);
        p.lut.resize((size_t)fm3d::kFreakScales * fm3d::kFreakOrient * fm3d::kFreakPoints);
        for (int s = 0; s < fm3d::kFreakScales; s++) {
            const double scalingFactor = std::pow(scaleStep, (double)s);
            p.sizes[s] = 0;
            for (int r = 0; r < fm3d::kFreakOrient; r++) {
                const double theta = (double)r * 2 * M_PI / (double)fm3d::kFreakOrient;
                int q = 0;
                for (int i = 0; i < 8; i++)
                    for (int k = 0; k < n[i]; k++) {
                        const double beta = M_PI / n[i] * (i % 2);
                        const double alpha = (double)k * 2 * M_PI / (double)n[i] + beta + theta;
                        float4& pt = p.lut[((size_t)s * fm3d::kFreakOrient + r) * fm3d::kFreakPoints + q];
                        pt.x = (float)(radius[i] * std::cos(alpha) * scalingFactor * kPatternScale);
                        pt.y = (float)(radius[i] * std::sin(alpha) * scalingFactor * kPatternScale);
                        pt.z = (float)(sigma[i] * scalingFactor * kPatternScale);
                        pt.w = 0.f;
                        const int sizeMax = (int)std::ceil((radius[i] + sigma[i]) * scalingFactor * kPatternScale) + 1;
                        if (p.sizes[s] < sizeMax) p.sizes[s] = sizeMax;
                        q++;
                    }
            }
        }
        for (int m = fm3d::kFreakOrientPairs; m--;) {
            const int i = FM3D_FREAK_ORIENT_PAIRS[2 * m], j = FM3D_FREAK_ORIENT_PAIRS[2 * m + 1];
            const float dx = p.lut[i].x - p.lut[j].x, dy = p.lut[i].y - p.lut[j].y;
            const float norm_sq = dx * dx + dy * dy;
            p.op[4 * m] = i;
            p.op[4 * m + 1] = j;
            p.op[4 * m + 2] = (int)((dx / norm_sq) * 4096.0 + 0.5);
            p.op[4 * m + 3] = (int)((dy / norm_sq) * 4096.0 + 0.5);
        }
        return p;
    }();
    return P;
}
int kscale(float size) {
    const float sizeCst = (float)(fm3d::kFreakScales / (0.693147180559945 * kOctaves));
    int s = (int)(logf(size / 7) * sizeCst + 0.5);
    return std::min(std::max(s, 0), fm3d::kFreakScales - 1);
}
// the compressed pair index (FREAK::DEF_PAIRS) -> (i, j < i) of the 903 pairs in generation order
int2 pair_of(int k) {
    int a = 1;
    while (k >= a) k -= a++;
    return make_int2(a, k);
}
}  // namespace freak

int freak_compute(fm3d_ctx* c, const uint8_t* img, int w, int h, const fm3d_keypoint* kpts, int n, fm3d_keypoint* kout,
                  int32_t* kept, int* nOut, uint8_t* desc) {
    const freak::Pattern& P = freak::pattern();
    *nOut = 0;
    // runByKeypointSize(FLT_EPSILON) (NaN dropped), then FREAK's scale-dependent border, order kept
    std::vector<fm3d_keypoint> K;
    std::vector<int> src, scl;
    for (int q = 0; q < n; q++) {
        const fm3d_keypoint& k = kpts[q];
        if (!(k.size >= FLT_EPSILON && k.size <= FLT_MAX)) continue;
        const int s = freak::kscale(k.size);
        const float ps = (float)P.sizes[s];
        if (k.x <= ps || k.y <= ps || k.x >= w - ps || k.y >= h - ps) continue;
        K.push_back(k);
        src.push_back(q);
        scl.push_back(s);
    }
    const int m = (int)K.size();
    if (m == 0) return FM3D_OK;
    const long long W1H1 = (long long)(w + 1) * (h + 1);
    if (W1H1 > INT32_MAX / 4) return fail(c, FM3D_ERR_INVALID, "image too large for FREAK");
    std::vector<int2> pairs(FM3D_FREAK_NB_PAIRS);
    for (int k = 0; k < FM3D_FREAK_NB_PAIRS; k++)
        pairs[k] = freak::pair_of(c->freakUserPairs.empty() ? FM3D_FREAK_DEF_PAIRS[k] : c->freakUserPairs[k]);
    if (c->frLut.bytes == 0) {  // the whole pattern, once per context (8.4 MB)
        HIPCHK(c, c->frLut.ensure(P.lut.size() * sizeof(float4)));
        HIPCHK(c, c->frOp.ensure(sizeof(P.op)));
        HIPCHK(c, hipMemcpy(c->frLut.p, P.lut.data(), P.lut.size() * sizeof(float4), hipMemcpyHostToDevice));
        HIPCHK(c, hipMemcpy(c->frOp.p, P.op, sizeof(P.op), hipMemcpyHostToDevice));
    }
    HIPCHK(c, c->frImg.ensure((size_t)w * h));
    HIPCHK(c, c->frSum.ensure((size_t)W1H1 * sizeof(int)));
    HIPCHK(c, c->frKp.ensure((size_t)m * sizeof(fm3d_keypoint)));
    HIPCHK(c, c->frScale.ensure((size_t)m * sizeof(int)));
    HIPCHK(c, c->frPairs.ensure(pairs.size() * sizeof(int2)));
    HIPCHK(c, c->frAng.ensure((size_t)m * sizeof(float)));
    HIPCHK(c, c->frDesc.ensure((size_t)m * 64));
    HIPCHK(c, hipMemcpyAsync(c->frImg.p, img, (size_t)w * h, hipMemcpyHostToDevice, c->stream));
    HIPCHK(c, hipMemcpyAsync(c->frKp.p, K.data(), (size_t)m * sizeof(fm3d_keypoint), hipMemcpyHostToDevice, c->stream));
    HIPCHK(c, hipMemcpyAsync(c->frScale.p, scl.data(), (size_t)m * sizeof(int), hipMemcpyHostToDevice, c->stream));
    HIPCHK(c, hipMemcpyAsync(c->frPairs.p, pairs.data(), pairs.size() * sizeof(int2), hipMemcpyHostToDevice, c->stream));
    fm3d::launch_integral(c->frImg.as<uint8_t>(), w, h, c->frSum.as<int>(), c->stream);
    fm3d::launch_freak_desc(c->frImg.as<uint8_t>(), c->frSum.as<int>(), w, c->frKp.as<fm3d_keypoint>(),
                            c->frScale.as<int>(), m, c->frLut.as<float4>(), c->frOp.as<int4>(), c->frPairs.as<int2>(),
                            c->frAng.as<float>(), c->frDesc.as<uint8_t>(), c->stream);
    HIPCHK(c, hipGetLastError());
    std::vector<float> ang(m);
    HIPCHK(c, hipMemcpyAsync(desc, c->frDesc.p, (size_t)m * 64, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipMemcpyAsync(ang.data(), c->frAng.p, (size_t)m * sizeof(float), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    for (int i = 0; i < m; i++) {
        kout[i] = K[i];
        kout[i].angle = ang[i];  // FREAK's orientation normalisation sets the keypoint angle
        if (kept) kept[i] = src[i];
    }
    *nOut = m;
    return FM3D_OK;
}

}  // namespace

namespace fm3d_host {
int brisk_border(float kpSize) { return brisk::size_of(brisk::kscale(kpSize)); }
int freak_border(float kpSize) { return freak::pattern().sizes[freak::kscale(kpSize)]; }
}  // namespace fm3d_host

extern "C" {

int fm3d_freak_compute(fm3d_ctx* c, const uint8_t* img, int w, int h, const fm3d_keypoint* kpts, int n,
                       fm3d_keypoint* kout, int32_t* kept, int* nOut, uint8_t* desc) {
    if (!c || !img || !nOut || w <= 0 || h <= 0 || n < 0 || (n > 0 && (!kpts || !kout || !desc)))
        return FM3D_ERR_INVALID;
    hipSetDevice(c->device);
    return freak_compute(c, img, w, h, kpts, n, kout, kept, nOut, desc);
}

int fm3d_freak_set_pairs(fm3d_ctx* c, const int32_t* pairs, int n) {
    if (!c || (pairs && n != FM3D_FREAK_NB_PAIRS)) return FM3D_ERR_INVALID;
    if (pairs)
        for (int k = 0; k < n; k++)
            if (pairs[k] < 0 || pairs[k] >= 903) return fail(c, FM3D_ERR_INVALID, "a FREAK pair index outside [0, 903)");
    c->freakUserPairs.clear();
    if (pairs) c->freakUserPairs.assign(pairs, pairs + n);
    return FM3D_OK;
}

int fm3d_brisk_compute(fm3d_ctx* c, const uint8_t* img, int w, int h, const fm3d_keypoint* kpts, int n,
                       fm3d_keypoint* kout, int32_t* kept, int* nOut, uint8_t* desc) {
    if (!c || !img || !nOut || w <= 0 || h <= 0 || n < 0 || (n > 0 && (!kpts || !kout || !desc)))
        return FM3D_ERR_INVALID;
    hipSetDevice(c->device);
    return brisk_compute(c, img, w, h, kpts, n, kout, kept, nOut, desc);
}

}  // extern "C"
