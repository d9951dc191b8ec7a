// fm3d_features.cpp -- C ABI (include/fm3d.h): the detectors and extractors (SURF, ORB, SIFT, FAST,
// STAR, BRISK, FREAK, MSER), fm3d_detect / fm3d_compute and the descriptors from patches.
//
// The host side of each: what OpenCV's constructors precompute (layer tables, patterns, kernels,
// resize tables) in the reference's expressions, the launches of the fm3d_*.hip kernels and the
// host bookkeeping between them (sorting, retaining, duplicate removal).
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
#include "fm3d_freak.h"
#include "fm3d_kernels.h"

using namespace fm3d_host;

namespace {

// ---------------- SURF plan (host side of fm3d_surf.hip; the oracle's orc_surf.c formulas) ----------------
int cv_round_h(double v) { return (int)std::lrint(v); }

// resizeHaarPattern (surf.cpp) in float, cvRound to nearest even
void surf_resize_haar(const int src[][5], fm3d::SurfHF* dst, int n, int oldSize, int newSize, int widthStep) {
    const float ratio = (float)newSize / oldSize;
    for (int k = 0; k < n; k++) {
        const int dx1 = cv_round_h(ratio * src[k][0]), dy1 = cv_round_h(ratio * src[k][1]);
        const int dx2 = cv_round_h(ratio * src[k][2]), dy2 = cv_round_h(ratio * src[k][3]);
        dst[k].p0 = dy1 * widthStep + dx1;
        dst[k].p1 = dy2 * widthStep + dx1;
        dst[k].p2 = dy1 * widthStep + dx2;
        dst[k].p3 = dy2 * widthStep + dx2;
        dst[k].w = src[k][4] / ((float)(dx2 - dx1) * (dy2 - dy1));
    }
}

struct SurfPlan {
    std::vector<fm3d::SurfLayer> L;
    std::vector<fm3d::SurfMid> M;
    size_t detFloats = 0;
    long long hTotal = 0, mTotal = 0, candCap = 0;
};

// fastHessianDetector's layer table: (nOctaveLayers + 2) * nOctaves layers, size (9 + 6*layer) <<
// octave, sample step 1 << octave; calcLayerDetAndTrace skips layers larger than the image
SurfPlan surf_plan(int w, int h, int octaves, int layers) {
    static const int dx_s[3][5] = {{0, 2, 3, 7, 1}, {3, 2, 6, 7, -2}, {6, 2, 9, 7, 1}};
    static const int dy_s[3][5] = {{2, 0, 7, 3, 1}, {2, 3, 7, 6, -2}, {2, 6, 7, 9, 1}};
    static const int dxy_s[4][5] = {{1, 1, 4, 4, 1}, {5, 1, 8, 4, -1}, {1, 5, 4, 8, -1}, {5, 5, 8, 8, 1}};
    SurfPlan P;
    for (int o = 0; o < octaves; o++)
        for (int l = 0; l < layers + 2; l++) {
            fm3d::SurfLayer y{};
            y.size = (9 + 6 * l) << o;
            y.step = 1 << o;
            y.rows = h / y.step;
            y.cols = w / y.step;
            y.off = P.detFloats;
            P.detFloats += (size_t)y.rows * y.cols;
            y.first = P.hTotal;
            if (y.size <= h && y.size <= w) {
                y.si = 1 + (h - y.size) / y.step;
                y.sj = 1 + (w - y.size) / y.step;
                y.margin = (y.size / 2) / y.step;
                surf_resize_haar(dx_s, y.hf, 3, 9, y.size, w + 1);
                surf_resize_haar(dy_s, y.hf + 3, 3, 9, y.size, w + 1);
                surf_resize_haar(dxy_s, y.hf + 6, 4, 9, y.size, w + 1);
            }
            P.hTotal += (long long)y.si * y.sj;
            P.L.push_back(y);
        }
    for (int o = 0; o < octaves; o++)
        for (int l = 1; l <= layers; l++) {
            const int idx = o * (layers + 2) + l;
            fm3d::SurfMid m{};
            m.layer = idx;
            m.octave = o;
            m.rows = P.L[idx].rows;
            m.cols = P.L[idx].cols;
            m.margin = (P.L[idx + 1].size / 2) / P.L[idx].step + 1;
            m.first = P.mTotal;
            P.mTotal += (long long)m.rows * m.cols;
            // strict maxima of a 3x3 neighbourhood: at most one per 2x2 block
            P.candCap += (long long)((m.rows + 1) / 2) * ((m.cols + 1) / 2);
            P.M.push_back(m);
        }
    P.candCap += 16;
    return P;
}

// getGaussianKernel(20, 3.3, CV_32F) outer product: SURFInvoker's descriptor weights DW
std::vector<float> surf_dw() {
    float g[20];
    const double scale2X = -0.5 / (3.3 * 3.3);
    double sum = 0;
    for (int i = 0; i < 20; i++) {
        const double x = i - (20 - 1) * 0.5;
        g[i] = (float)std::exp(scale2X * x * x);
        sum += g[i];
    }
    sum = 1. / sum;
    for (int i = 0; i < 20; i++) g[i] = (float)(g[i] * sum);
    std::vector<float> dw(400);
    for (int i = 0; i < 20; i++)
        for (int j = 0; j < 20; j++) dw[i * 20 + j] = g[i] * g[j];
    return dw;
}

// SURFInvoker's orientation samples (the constructor's apt / aptw): the disc of radius 6, i (x)
// outer, j (y) inner, weights G(i) * G(j), G = getGaussianKernel(13, 2.5, CV_32F)
const fm3d::SurfOri& surf_ori() {
    static const fm3d::SurfOri ori = [] {
        fm3d::SurfOri o{};
        float g[13];
        const double scale2X = -0.5 / (2.5 * 2.5);
        double sum = 0;
        for (int i = 0; i < 13; i++) {
            const double x = i - (13 - 1) * 0.5;
            g[i] = (float)std::exp(scale2X * x * x);
            sum += g[i];
        }
        sum = 1. / sum;
        for (int i = 0; i < 13; i++) g[i] = (float)(g[i] * sum);
        for (int i = -6; i <= 6; i++)
            for (int j = -6; j <= 6; j++)
                if (i * i + j * j <= 36) {
                    o.ax[o.n] = i;
                    o.ay[o.n] = j;
                    o.w[o.n++] = g[i + 6] * g[j + 6];
                }
        return o;
    }();
    return ori;
}

// ---------------- ORB (host side of fm3d_orb.hip; the oracle's orc_orb.c formulas) ----------------
// getScale (orb.cpp): (float)pow(scaleFactor, level)
float orb_scale(double scaleFactor, int level) { return (float)std::pow(scaleFactor, (double)level); }

struct OrbPlan {
    std::vector<fm3d::OrbLevel> L;
    long long total = 0;
};

// the pyramid levels: size cvRound(cols * (1 / getScale)), concatenated pixel after pixel
OrbPlan orb_plan(int w, int h, double scaleFactor, int nl) {
    OrbPlan P;
    for (int l = 0; l < nl; l++) {
        const float scale = 1 / orb_scale(scaleFactor, l);
        fm3d::OrbLevel v;
        v.w = (int)std::lrint((float)(w * scale));
        v.h = (int)std::lrint((float)(h * scale));
        v.first = P.total;
        P.total += (long long)std::max(v.w, 0) * std::max(v.h, 0);
        P.L.push_back(v);
    }
    return P;
}

short sat_short(float v) {
    const long i = std::lrint(v);
    return (short)(i < -32768 ? -32768 : (i > 32767 ? 32767 : i));
}

// resize(INTER_LINEAR)'s fixed-point tables for src (sw x sh) -> dst (dw x dh), packed as
// [xofs dw][yofs dh] ints then [alpha 2dw][beta 2dh] shorts; returns xmax
int orb_resize_tabs(int sw, int sh, int dw, int dh, std::vector<int>& ofs, std::vector<short>& ab) {
    const double scale_x = 1. / ((double)dw / sw), scale_y = 1. / ((double)dh / sh);
    int xmax = dw;
    for (int dx = 0; dx < dw; dx++) {
        float fx = (float)((dx + 0.5) * scale_x - 0.5);
        int sx = (int)std::floor(fx);
        fx -= sx;
        if (sx < 0) {
            fx = 0;
            sx = 0;
        }
        if (sx + 1 >= sw) {
            xmax = std::min(xmax, dx);
            if (sx >= sw - 1) {
                fx = 0;
                sx = sw - 1;
            }
        }
        ofs.push_back(sx);
        ab.push_back(sat_short((1.f - fx) * 2048));
        ab.push_back(sat_short(fx * 2048));
    }
    for (int dy = 0; dy < dh; dy++) {
        float fy = (float)((dy + 0.5) * scale_y - 0.5);
        const int sy = (int)std::floor(fy);
        fy -= sy;
        ofs.push_back(sy);
        ab.push_back(sat_short((1.f - fy) * 2048));
        ab.push_back(sat_short(fy * 2048));
    }
    return xmax;
}

// VResizeLinearVec_32s8u's columns: the 16-wide loop, then the 4-wide one while x < width - 4
int orb_vresize_sse_end(int width) {
    int x = 0;
    for (; x <= width - 16; x += 16) {}
    for (; x < width - 4; x += 4) {}
    return x;
}

// image -> level 0, then every level from the previous one (orb.cpp's pyramid loop)
int orb_build_pyramid(fm3d_ctx* c, const uint8_t* img, int w, int h, const OrbPlan& P) {
    const int nl = (int)P.L.size();
    HIPCHK(c, c->orbPyr.ensure((size_t)P.total + 64));
    HIPCHK(c, c->orbLev.ensure(P.L.size() * sizeof(fm3d::OrbLevel)));
    HIPCHK(c, hipMemcpyAsync(c->orbPyr.p, img, (size_t)w * h, hipMemcpyHostToDevice, c->stream));
    HIPCHK(c, hipMemcpyAsync(c->orbLev.p, P.L.data(), P.L.size() * sizeof(fm3d::OrbLevel), hipMemcpyHostToDevice,
                             c->stream));
    std::vector<int> ofs;
    std::vector<short> ab;
    std::vector<int> xmax(nl, 0);
    std::vector<size_t> oOfs(nl, 0), oAb(nl, 0);
    for (int l = 1; l < nl; l++) {
        oOfs[l] = ofs.size();
        oAb[l] = ab.size();
        xmax[l] = orb_resize_tabs(P.L[l - 1].w, P.L[l - 1].h, P.L[l].w, P.L[l].h, ofs, ab);
    }
    const size_t ofsBytes = ofs.size() * sizeof(int);
    HIPCHK(c, c->orbTab.ensure(ofsBytes + ab.size() * sizeof(short) + 64));
    if (!ofs.empty()) {
        HIPCHK(c, hipMemcpyAsync(c->orbTab.p, ofs.data(), ofsBytes, hipMemcpyHostToDevice, c->stream));
        HIPCHK(c, hipMemcpyAsync(static_cast<char*>(c->orbTab.p) + ofsBytes, ab.data(), ab.size() * sizeof(short),
                                 hipMemcpyHostToDevice, c->stream));
    }
    const int* T = c->orbTab.as<int>();
    const short* A = reinterpret_cast<const short*>(static_cast<const char*>(c->orbTab.p) + ofsBytes);
    uint8_t* pyr = c->orbPyr.as<uint8_t>();
    for (int l = 1; l < nl; l++) {
        const fm3d::OrbLevel &s0 = P.L[l - 1], &d0 = P.L[l];
        if (d0.w <= 0 || d0.h <= 0 || s0.w <= 0 || s0.h <= 0) continue;
        fm3d::launch_orb_resize(pyr + s0.first, s0.w, s0.h, pyr + d0.first, d0.w, d0.h, T + oOfs[l], A + oAb[l],
                                T + oOfs[l] + d0.w, A + oAb[l] + 2 * d0.w, xmax[l], orb_vresize_sse_end(d0.w),
                                c->stream);
    }
    HIPCHK(c, hipGetLastError());
    HIPCHK(c, hipStreamSynchronize(c->stream));  // ofs / ab leave scope
    return FM3D_OK;
}

// KeyPointsFilter::retainBest with libstdc++'s own nth_element / partition (the order they leave
// decides which tied keypoints survive and the output order)
int orb_retain_best(fm3d_keypoint* k, int n, int npts) {
    if (npts >= 0 && n > npts) {
        if (npts == 0) return 0;
        auto greater = [](const fm3d_keypoint& a, const fm3d_keypoint& b) { return a.response > b.response; };
        std::nth_element(k, k + npts, k + n, greater);
        const float amb = k[npts - 1].response;
        return (int)(std::partition(k + npts, k + n, [amb](const fm3d_keypoint& p) { return p.response >= amb; }) - k);
    }
    return n;
}

// the 512-point pattern: the caller's, else makeRandomPattern(patchSize) (cv::RNG(0x34985739))
std::vector<int> orb_pattern(const fm3d_ctx* c, int patchSize) {
    std::vector<int> xy = c->orbUserPattern;
    if (xy.empty()) {
        uint64_t state = 0x34985739;
        const int a = -patchSize / 2, b = patchSize / 2 + 1;
        for (int i = 0; i < 1024; i++) {
            state = (uint64_t)(unsigned)state * 4164903690U + (unsigned)(state >> 32);
            xy.push_back((int)((unsigned)state % (unsigned)(b - a) + (unsigned)a));
        }
    }
    return xy;
}

int orb_upload_pattern(fm3d_ctx* c, int patchSize) {
    const std::vector<int> xy = orb_pattern(c, patchSize);
    HIPCHK(c, c->orbPat.ensure(1024 * sizeof(int)));
    HIPCHK(c, hipMemcpyAsync(c->orbPat.p, xy.data(), 1024 * sizeof(int), hipMemcpyHostToDevice, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    return FM3D_OK;
}

fm3d::OrbBlurK orb_blur_kernel() {
    fm3d::OrbBlurK k;
    float g[7];
    const double scale2X = -0.5 / (2.0 * 2.0);
    double sum = 0;
    for (int i = 0; i < 7; i++) {
        const double x = i - 3.0;
        g[i] = (float)std::exp(scale2X * x * x);
        sum += g[i];
    }
    sum = 1. / sum;
    for (int i = 0; i < 7; i++) g[i] = (float)(g[i] * sum);
    for (int i = 0; i < 7; i++) k.ik[i] = (int)std::lrint(g[i] * 256.f);
    for (int i = 0; i < 4; i++) k.fk[i] = (float)(k.ik[3 + i] * (1. / 65536));
    return k;
}

// blurred levels + descriptors of the (device) keypoints kp[0..n) in level coordinates
int orb_describe(fm3d_ctx* c, const OrbPlan& P, int n, uint8_t* desc) {
    if (n <= 0) return FM3D_OK;
    int r;
    if ((r = orb_upload_pattern(c, c->s.orbPatchSize))) return r;
    HIPCHK(c, c->orbR.ensure((size_t)P.total * sizeof(int) + 64));
    HIPCHK(c, c->orbBlur.ensure((size_t)P.total + 64));
    HIPCHK(c, c->orbDesc.ensure((size_t)n * 32));
    fm3d::launch_orb_blur(c->orbPyr.as<uint8_t>(), c->orbLev.as<fm3d::OrbLevel>(), (int)P.L.size(), P.total,
                          orb_blur_kernel(), c->orbR.as<int>(), c->orbBlur.as<uint8_t>(), c->stream);
    fm3d::launch_orb_desc(c->orbBlur.as<uint8_t>(), c->orbLev.as<fm3d::OrbLevel>(), c->orbKp.as<fm3d_keypoint>(), n,
                          c->orbPat.as<int>(), c->orbDesc.as<uint8_t>(), c->stream);
    HIPCHK(c, hipGetLastError());
    HIPCHK(c, hipMemcpyAsync(desc, c->orbDesc.p, (size_t)n * 32, hipMemcpyDeviceToHost, c->stream));
    return FM3D_OK;
}

int orb_check_settings(fm3d_ctx* c) {
    const fm3d_settings& S = c->s;
    if (S.orbNumLevels < 1 || S.orbNumLevels > 64 || !(S.orbScaleFactor > 1.0) || S.orbNumFeatures < 0 ||
        S.orbEdgeThreshold < 0 || S.orbPatchSize < 2 || S.orbPatchSize > 124 || S.orbFastThreshold < 0)
        return fail(c, FM3D_ERR_INVALID, "ORB NumLevels / ScaleFactor / NumFeatures / edgeThreshold / patchSize out of range");
    // the descriptor reads pattern points up to patchSize/2 * sqrt(2) + 1 from the centre and the
    // blur 3 more: inside the edge border, as OpenCV's defaults guarantee
    if (S.orbEdgeThreshold < (int)std::ceil(S.orbPatchSize / 2 * 1.4143) + 4)
        return fail(c, FM3D_ERR_INVALID, "ORB edgeThreshold too small for patchSize (reads past the level border)");
    return FM3D_OK;
}

// ---------------- SIFT (host side of fm3d_sift.hip; the oracle's orc_sift.c formulas) ----------------
// the pyramid plan: level sizes and offsets, Gaussian levels nOct * (L + 3), DoG levels nOct * (L + 2)
struct SiftPlan {
    int firstOctave = 0, nOct = 0, L = 0;
    std::vector<fm3d::SiftLevel> G, D;
    long long gTotal = 0, dTotal = 0;
};

// false when an octave would be empty (OpenCV's resize asserts there)
bool sift_plan(int w, int h, int firstOctave, int nOct, int L, SiftPlan& P) {
    P = SiftPlan{};
    P.firstOctave = firstOctave;
    P.nOct = nOct;
    P.L = L;
    int ow = firstOctave < 0 ? 2 * w : w, oh = firstOctave < 0 ? 2 * h : h;
    for (int o = 0; o < nOct; o++) {
        if (o > 0) {
            ow /= 2;
            oh /= 2;
        }
        if (ow < 1 || oh < 1) return false;
        for (int i = 0; i < L + 3; i++) {
            P.G.push_back({ow, oh, P.gTotal});
            P.gTotal += (long long)ow * oh;
        }
        for (int i = 0; i < L + 2; i++) {
            P.D.push_back({ow, oh, P.dTotal});
            P.dTotal += (long long)ow * oh;
        }
    }
    return true;
}

int sift_num_octaves(int w, int h, int firstOctave) {
    const int bw = firstOctave < 0 ? 2 * w : w, bh = firstOctave < 0 ? 2 * h : h;
    return (int)std::lrint(std::log((double)std::min(bw, bh)) / std::log(2.) - 2) - firstOctave;
}

// getGaussianKernel(cvRound(sigma*8+1)|1, sigma, CV_32F)
std::vector<float> sift_gauss_kernel(double sigma) {
    const int n = (int)std::lrint(sigma * 4 * 2 + 1) | 1;
    std::vector<float> cf(n);
    const double scale2X = -0.5 / (sigma * sigma);
    double sum = 0;
    for (int i = 0; i < n; i++) {
        const double x = i - (n - 1) * 0.5;
        cf[i] = (float)std::exp(scale2X * x * x);
        sum += cf[i];
    }
    sum = 1. / sum;
    for (int i = 0; i < n; i++) cf[i] = (float)(cf[i] * sum);
    return cf;
}

constexpr int kSiftMaxTaps = 65;  // the blur tile's LDS (r <= 32: sigma up to ~8)

// createInitialImage + buildGaussianPyramid (+ buildDoGPyramid) into siftG / siftD
int sift_build(fm3d_ctx* c, const uint8_t* img, int w, int h, const SiftPlan& P, bool dog) {
    const fm3d_settings& S = c->s;
    const int L = P.L, nl = L + 3;
    // the blur kernels: [0] sig_diff of the initial image, [i] sig[i] of the octave levels
    std::vector<std::vector<float>> taps(nl);
    {
        const float sigma = (float)S.siftSigma;
        const float sd = P.firstOctave < 0 ? std::sqrt(std::max(sigma * sigma - 0.5f * 0.5f * 4, 0.01f))
                                           : std::sqrt(std::max(sigma * sigma - 0.5f * 0.5f, 0.01f));
        taps[0] = sift_gauss_kernel(sd);
        const double k = std::pow(2., 1. / L);
        for (int i = 1; i < nl; i++) {
            const double sig_prev = std::pow(k, (double)(i - 1)) * S.siftSigma;
            const double sig_total = sig_prev * k;
            taps[i] = sift_gauss_kernel(std::sqrt(sig_total * sig_total - sig_prev * sig_prev));
        }
    }
    for (auto& t : taps)
        if ((int)t.size() > kSiftMaxTaps)
            return fail(c, FM3D_ERR_UNSUPPORTED, "SIFT sigma too large for the GPU blur tile (kernel > 65 taps)");
    std::vector<float> tapBuf((size_t)nl * 128, 0.f);
    for (int i = 0; i < nl; i++) std::copy(taps[i].begin(), taps[i].end(), tapBuf.begin() + (size_t)i * 128);
    HIPCHK(c, c->siftTaps.ensure(tapBuf.size() * sizeof(float)));
    HIPCHK(c, hipMemcpyAsync(c->siftTaps.p, tapBuf.data(), tapBuf.size() * sizeof(float), hipMemcpyHostToDevice,
                             c->stream));
    HIPCHK(c, c->siftImg.ensure((size_t)w * h));
    HIPCHK(c, hipMemcpyAsync(c->siftImg.p, img, (size_t)w * h, hipMemcpyHostToDevice, c->stream));
    HIPCHK(c, c->siftG.ensure((size_t)P.gTotal * sizeof(float) + 64));
    if (dog) HIPCHK(c, c->siftD.ensure((size_t)P.dTotal * sizeof(float) + 64));
    const int bw = P.G[0].w, bh = P.G[0].h;
    HIPCHK(c, c->siftBase.ensure((size_t)bw * bh * sizeof(float)));
    float* G = c->siftG.as<float>();
    float* D = dog ? c->siftD.as<float>() : nullptr;
    const float* T = c->siftTaps.as<float>();
    {
        fm3d::SiftResize rp{};
        rp.sw = w;
        rp.sh = h;
        rp.dw = bw;
        rp.dh = bh;
        rp.doubled = P.firstOctave < 0;
        rp.scx = 1. / ((double)bw / w);
        rp.scy = 1. / ((double)bh / h);
        rp.xmax = bw;
        for (int dx = 0; dx < bw; dx++) {  // resize's xmax: the first column whose right tap leaves the row
            const float fx = (float)((dx + 0.5) * rp.scx - 0.5);
            if ((int)std::floor(fx) + 1 >= w) {
                rp.xmax = dx;
                break;
            }
        }
        fm3d::launch_sift_init(c->siftImg.as<uint8_t>(), c->siftBase.as<float>(), rp, 1, c->stream);
        fm3d::launch_sift_blur(c->siftBase.as<float>(), G, nullptr, bw, bh, T, (int)taps[0].size(), 1, c->stream);
    }
    for (int o = 0; o < P.nOct; o++)
        for (int i = 0; i < nl; i++) {
            const fm3d::SiftLevel& d = P.G[o * nl + i];
            if (o == 0 && i == 0) continue;
            if (i == 0) {
                const fm3d::SiftLevel& s = P.G[(o - 1) * nl + L];
                fm3d::launch_sift_down(G + s.first, s.w, s.h, G + d.first, d.w, d.h, 1. / ((double)d.w / s.w),
                                       1. / ((double)d.h / s.h), c->stream);
            } else {
                const fm3d::SiftLevel& s = P.G[o * nl + i - 1];
                fm3d::launch_sift_blur(G + s.first, G + d.first, D ? D + P.D[o * (L + 2) + i - 1].first : nullptr, d.w,
                                       d.h, T + (size_t)i * 128, (int)taps[i].size(), 1, c->stream);
            }
        }
    HIPCHK(c, hipGetLastError());
    HIPCHK(c, c->siftGL.ensure(P.G.size() * sizeof(fm3d::SiftLevel)));
    HIPCHK(c, hipMemcpyAsync(c->siftGL.p, P.G.data(), P.G.size() * sizeof(fm3d::SiftLevel), hipMemcpyHostToDevice,
                             c->stream));
    if (dog) {
        HIPCHK(c, c->siftDL.ensure(P.D.size() * sizeof(fm3d::SiftLevel)));
        HIPCHK(c, hipMemcpyAsync(c->siftDL.p, P.D.data(), P.D.size() * sizeof(fm3d::SiftLevel), hipMemcpyHostToDevice,
                                 c->stream));
    }
    // the host vectors leave scope: finish the copies
    HIPCHK(c, hipStreamSynchronize(c->stream));
    return FM3D_OK;
}

int sift_check_settings(fm3d_ctx* c) {
    const fm3d_settings& S = c->s;
    if (S.siftOctaveLayers < 1 || S.siftOctaveLayers > 16 || S.siftNumFeatures < 0 || !(S.siftSigma > 0) ||
        !(S.siftContrastThreshold >= 0) || !(S.siftEdgeThreshold >= 0))
        return fail(c, FM3D_ERR_INVALID, "SIFT NumOctaveLayers / NumFeatures / Sigma / thresholds out of range");
    return FM3D_OK;
}

// KeyPointsFilter::removeDuplicated: KeyPoint_LessThan order with the index as the last key, the
// first of each group of equal (pt, size, angle) kept, input order preserved
int sift_remove_duplicated(std::vector<fm3d_keypoint>& k) {
    const int n = (int)k.size();
    if (n < 2) return n;
    std::vector<int> idx(n);
    for (int i = 0; i < n; i++) idx[i] = i;
    std::sort(idx.begin(), idx.end(), [&](int i, int j) {
        const fm3d_keypoint &a = k[i], &b = k[j];
        if (a.x != b.x) return a.x < b.x;
        if (a.y != b.y) return a.y < b.y;
        if (a.size != b.size) return a.size > b.size;
        if (a.angle != b.angle) return a.angle < b.angle;
        if (a.response != b.response) return a.response > b.response;
        if (a.octave != b.octave) return a.octave > b.octave;
        if (a.class_id != b.class_id) return a.class_id > b.class_id;
        return i < j;
    });
    std::vector<uint8_t> mask(n, 1);
    for (int i = 1, j = 0; i < n; i++) {
        const fm3d_keypoint &a = k[idx[i]], &b = k[idx[j]];
        if (a.x != b.x || a.y != b.y || a.size != b.size || a.angle != b.angle)
            j = i;
        else
            mask[idx[i]] = 0;
    }
    int j = 0;
    for (int i = 0; i < n; i++)
        if (mask[i]) k[j++] = k[i];
    k.resize(j);
    return j;
}

void sift_unpack_octave(const fm3d_keypoint& k, int& octave, int& layer) {
    octave = k.octave & 255;
    layer = (k.octave >> 8) & 255;
    octave = octave < 128 ? octave : (-128 | octave);
}

// SIFT::operator()(img, Mat(), kpts, desc, true) on keypoints that passed runByKeypointSize:
// the pyramid from firstOctave = min(0, octaves), nOctaves = max - first + 1 (reused when the detect
// call just built the same levels), calcDescriptors.  desc: m x 128 floats (host)
int sift_describe(fm3d_ctx* c, const uint8_t* img, int w, int h, const std::vector<fm3d_keypoint>& k, float* desc,
                  const SiftPlan* built) {
    const int m = (int)k.size(), L = c->s.siftOctaveLayers;
    if (m == 0) return FM3D_OK;
    int firstOctave = 0, maxOctave = INT_MIN, actualNLayers = 0;
    for (const auto& q : k) {
        int o, l;
        sift_unpack_octave(q, o, l);
        firstOctave = std::min(firstOctave, o);
        maxOctave = std::max(maxOctave, o);
        actualNLayers = std::max(actualNLayers, l - 2);
    }
    firstOctave = std::min(firstOctave, 0);
    if (firstOctave < -1 || actualNLayers > L)
        return fail(c, FM3D_ERR_INVALID, "SIFT compute: a keypoint octave < -1 or layer > nOctaveLayers + 2");
    const int nOct = maxOctave - firstOctave + 1;
    int r;
    SiftPlan P;
    if (built && built->firstOctave == firstOctave && built->nOct >= nOct) {
        P = *built;
    } else {
        if (!sift_plan(w, h, firstOctave, nOct, L, P))
            return fail(c, FM3D_ERR_INVALID, "SIFT compute: a keypoint octave the image cannot hold");
        if ((r = sift_build(c, img, w, h, P, false))) return r;
    }
    HIPCHK(c, c->siftKp.ensure((size_t)m * sizeof(fm3d_keypoint)));
    HIPCHK(c, c->siftDesc.ensure((size_t)m * 128 * sizeof(float)));
    HIPCHK(c, hipMemcpyAsync(c->siftKp.p, k.data(), (size_t)m * sizeof(fm3d_keypoint), hipMemcpyHostToDevice,
                             c->stream));
    fm3d::launch_sift_desc(c->siftG.as<float>(), c->siftGL.as<fm3d::SiftLevel>(), L, firstOctave,
                           c->siftKp.as<fm3d_keypoint>(), nullptr, m, c->siftDesc.as<float>(), c->stream);
    HIPCHK(c, hipGetLastError());
    HIPCHK(c, hipMemcpyAsync(desc, c->siftDesc.p, (size_t)m * 128 * sizeof(float), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    return FM3D_OK;
}

// extractDescriptorsFromPatches with the SIFT extractor (descriptorsmatcher.cpp:133-174, 302-310): per
// patch SIFT::operator()(patch, Mat(), {kp}, desc, true) with kp = (center, size, angle -1, octave 0):
// firstOctave 0, one octave, and the descriptor reads level 0 of it, blur(patch, sig_diff) -- so every
// patch needs only that level (batched: one init and one blur launch for all patches)
int sift_patches(fm3d_ctx* c, const uint8_t* patches, int P, int size, float* desc) {
    int r;
    if ((r = sift_check_settings(c))) return r;
    if (P == 0) return FM3D_OK;
    hipSetDevice(c->device);
    const fm3d_settings& S = c->s;
    const float center = (float)(int)std::floor(size / 2);
    const fm3d_keypoint k{center, center, (float)size, -1.f, 1.f, 0, 0};
    const float sigma = (float)S.siftSigma;
    const std::vector<float> taps = sift_gauss_kernel(std::sqrt(std::max(sigma * sigma - 0.5f * 0.5f, 0.01f)));
    if ((int)taps.size() > kSiftMaxTaps)
        return fail(c, FM3D_ERR_UNSUPPORTED, "SIFT sigma too large for the GPU blur tile (kernel > 65 taps)");
    const size_t per = (size_t)size * size;
    std::vector<fm3d::SiftLevel> GL((size_t)P);
    std::vector<int> lvl((size_t)P);
    for (int p = 0; p < P; p++) {
        GL[p] = {size, size, (long long)(p * per)};
        lvl[p] = p;
    }
    std::vector<fm3d_keypoint> kp((size_t)P, k);
    HIPCHK(c, c->siftTaps.ensure(128 * sizeof(float)));
    HIPCHK(c, c->siftImg.ensure((size_t)P * per));
    HIPCHK(c, c->siftBase.ensure((size_t)P * per * sizeof(float)));
    HIPCHK(c, c->siftG.ensure((size_t)P * per * sizeof(float)));
    HIPCHK(c, c->siftGL.ensure((size_t)P * sizeof(fm3d::SiftLevel)));
    HIPCHK(c, c->siftPos.ensure((size_t)P * sizeof(int)));
    HIPCHK(c, c->siftKp.ensure((size_t)P * sizeof(fm3d_keypoint)));
    HIPCHK(c, c->siftDesc.ensure((size_t)P * 128 * sizeof(float)));
    HIPCHK(c, hipMemcpyAsync(c->siftTaps.p, taps.data(), taps.size() * sizeof(float), hipMemcpyHostToDevice, c->stream));
    HIPCHK(c, hipMemcpyAsync(c->siftImg.p, patches, (size_t)P * per, hipMemcpyHostToDevice, c->stream));
    HIPCHK(c, hipMemcpyAsync(c->siftGL.p, GL.data(), GL.size() * sizeof(fm3d::SiftLevel), hipMemcpyHostToDevice,
                             c->stream));
    HIPCHK(c, hipMemcpyAsync(c->siftPos.p, lvl.data(), lvl.size() * sizeof(int), hipMemcpyHostToDevice, c->stream));
    HIPCHK(c, hipMemcpyAsync(c->siftKp.p, kp.data(), kp.size() * sizeof(fm3d_keypoint), hipMemcpyHostToDevice,
                             c->stream));
    fm3d::SiftResize rp{};
    rp.sw = rp.dw = size;
    rp.sh = rp.dh = size;
    rp.doubled = 0;
    fm3d::launch_sift_init(c->siftImg.as<uint8_t>(), c->siftBase.as<float>(), rp, P, c->stream);
    fm3d::launch_sift_blur(c->siftBase.as<float>(), c->siftG.as<float>(), nullptr, size, size, c->siftTaps.as<float>(),
                           (int)taps.size(), P, c->stream);
    fm3d::launch_sift_desc(c->siftG.as<float>(), c->siftGL.as<fm3d::SiftLevel>(), S.siftOctaveLayers, 0,
                           c->siftKp.as<fm3d_keypoint>(), c->siftPos.as<int>(), P, c->siftDesc.as<float>(), c->stream);
    HIPCHK(c, hipGetLastError());
    HIPCHK(c, hipMemcpyAsync(desc, c->siftDesc.p, (size_t)P * 128 * sizeof(float), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    return FM3D_OK;
}

// FastFeatureDetector(thr, nonmax).detect (features2d/src/fast.cpp): FAST-9 on the image itself, the
// ORB level-0 kernels with no edge border; KeyPoint(x, y, 7, -1, score) in raster order, the score 0
// without non-max suppression (FAST_t computes it only for the suppression)
int fast_detect(fm3d_ctx* c, const uint8_t* img, int w, int h, int thr, bool nonmax, std::vector<fm3d_keypoint>& k) {
    k.clear();
    thr = std::min(std::max(thr, 0), 255);
    const long long total = (long long)w * h;
    if (total > INT32_MAX / 2) return fail(c, FM3D_ERR_INVALID, "image too large for FAST");
    const fm3d::OrbLevel lv{w, h, 0};
    int r;
    if ((r = ensure_scan_tmp(c, (int)total))) return r;
    HIPCHK(c, c->orbPyr.ensure((size_t)total + 64));
    HIPCHK(c, c->orbLev.ensure(sizeof(fm3d::OrbLevel)));
    HIPCHK(c, c->orbMap.ensure((size_t)total * sizeof(uint16_t) + 64));
    HIPCHK(c, c->orbFlag.ensure((size_t)(total + 1) * sizeof(int)));
    HIPCHK(c, c->orbPos.ensure((size_t)(total + 1) * sizeof(int)));
    HIPCHK(c, hipMemcpyAsync(c->orbPyr.p, img, (size_t)total, hipMemcpyHostToDevice, c->stream));
    HIPCHK(c, hipMemcpyAsync(c->orbLev.p, &lv, sizeof(lv), hipMemcpyHostToDevice, c->stream));
    fm3d::launch_orb_fast(c->orbPyr.as<uint8_t>(), c->orbLev.as<fm3d::OrbLevel>(), 1, total, thr, 0, nonmax ? 1 : 0,
                          c->orbMap.as<uint16_t>(), c->orbFlag.as<int>(), c->stream);
    fm3d::launch_exclusive_scan(c->orbFlag.as<int>(), (int)total, c->orbPos.as<int>(), c->count.as<int>(), c->scanTmp.p,
                                c->stream);
    HIPCHK(c, hipGetLastError());
    int nc = 0;
    HIPCHK(c, hipMemcpyAsync(&nc, c->count.p, sizeof(int), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    if (nc == 0) return FM3D_OK;
    HIPCHK(c, c->orbKp.ensure((size_t)(nc + 1) * sizeof(fm3d_keypoint)));
    fm3d::launch_orb_fast_scatter(c->orbMap.as<uint16_t>(), c->orbLev.as<fm3d::OrbLevel>(), 1, total,
                                  c->orbFlag.as<int>(), c->orbPos.as<int>(), c->orbKp.as<fm3d_keypoint>(), c->stream);
    k.resize(nc);
    HIPCHK(c, hipMemcpyAsync(k.data(), c->orbKp.p, (size_t)nc * sizeof(fm3d_keypoint), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    if (!nonmax)
        for (auto& q : k) q.response = 0.f;
    return FM3D_OK;
}

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

int surf_upload_image(fm3d_ctx* c, const uint8_t* img, int w, int h) {
    HIPCHK(c, c->sfImg.ensure((size_t)w * h));
    HIPCHK(c, hipMemcpyAsync(c->sfImg.p, img, (size_t)w * h, hipMemcpyHostToDevice, c->stream));
    if (c->sfDW.bytes == 0) {
        const std::vector<float> dw = surf_dw();
        HIPCHK(c, c->sfDW.ensure(400 * sizeof(float)));
        HIPCHK(c, hipMemcpyAsync(c->sfDW.p, dw.data(), 400 * sizeof(float), hipMemcpyHostToDevice, c->stream));
        HIPCHK(c, hipStreamSynchronize(c->stream));  // dw leaves scope
    }
    return FM3D_OK;
}

}  // namespace

// what fm3d_pipeline_describe (fm3d_tail.cpp) shares with the one-shot patch descriptors below
namespace fm3d_host {

int surf_patch_gws(int size) { return 2 * cv_round_h(2 * ((float)size * 1.2f / 9.0f)); }

int ensure_surf_dw(fm3d_ctx* c) {
    if (c->sfDW.bytes) return FM3D_OK;
    const std::vector<float> dw = surf_dw();
    HIPCHK(c, c->sfDW.ensure(400 * sizeof(float)));
    HIPCHK(c, hipMemcpyAsync(c->sfDW.p, dw.data(), 400 * sizeof(float), hipMemcpyHostToDevice, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));  // dw leaves scope
    return FM3D_OK;
}

const fm3d::SurfOri& surf_ori_samples() { return surf_ori(); }

int sift_patch_taps(fm3d_ctx* c, std::vector<float>& taps) {
    if (int r = sift_check_settings(c)) return r;
    const float sigma = (float)c->s.siftSigma;
    taps = sift_gauss_kernel(std::sqrt(std::max(sigma * sigma - 0.5f * 0.5f, 0.01f)));
    if ((int)taps.size() > kSiftMaxTaps)
        return fail(c, FM3D_ERR_UNSUPPORTED, "SIFT sigma too large for the GPU blur tile (kernel > 65 taps)");
    return FM3D_OK;
}

int orb_patch_prepare(fm3d_ctx* c, int size) {
    int r, kept = 0;
    if ((r = orb_check_settings(c))) return r;
    if ((r = fm3d_patch_keypoint_kept(c, size, &kept))) return fail(c, r, "patch keypoint: no keep rule");
    if (!kept)
        return fail(c, FM3D_ERR_INVALID, "ORB drops the first patch's keypoint (the reference's rows would have 0 columns)");
    // descriptorsmatcher.cpp:146-158: every patch's keypoint has angle -1, so one table serves them all
    const float angle = -1.f;
    const int patchSize = c->s.orbPatchSize;
    std::vector<int> xy = orb_pattern(c, patchSize);
    if (!c->orbTabReach || patchSize != c->orbTabPatchSize || angle != c->orbTabAngle || xy != c->orbTabPattern) {
        c->orbTabReach = 0;
        hipSetDevice(c->device);
        int2 tab[512];
        HIPCHK(c, c->orbPat.ensure(1024 * sizeof(int)));
        HIPCHK(c, c->orbOffTab.ensure(sizeof(tab)));
        HIPCHK(c, hipMemcpyAsync(c->orbPat.p, xy.data(), 1024 * sizeof(int), hipMemcpyHostToDevice, c->stream));
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

void orb_patch_describe(fm3d_ctx* c, const uint8_t* patchesDev, int m, int size, uint8_t* rowsDev) {
    fm3d::launch_orb_patch_desc(patchesDev, m, size, c->orbOffTab.as<int2>(), orb_blur_kernel(), rowsDev, c->stream);
}

}  // namespace fm3d_host

extern "C" {

int fm3d_surf_detect(fm3d_ctx* c, const uint8_t* img, int w, int h, fm3d_keypoint* kpts, int cap, int* n,
                     float* desc) {
    if (!c || !img || !n || w <= 0 || h <= 0 || cap < 0 || (cap > 0 && !kpts)) return FM3D_ERR_INVALID;
    const fm3d_settings& S = c->s;
    if (S.detectorType != FM3D_FEAT_SURF || (desc && S.extractorType != FM3D_FEAT_SURF))
        return fail(c, FM3D_ERR_UNSUPPORTED, "only the STATIC SURF detector / extractor runs on the GPU");
    if (S.surfOctaves < 1 || S.surfOctaveLayers < 1 || S.surfHessianThreshold < 0)
        return fail(c, FM3D_ERR_INVALID, "SURF NumOctaves / NumOctaveLayers / HessianThreshold out of range");
    hipSetDevice(c->device);
    int r;
    if ((r = surf_upload_image(c, img, w, h))) return r;
    const SurfPlan P = surf_plan(w, h, S.surfOctaves, S.surfOctaveLayers);
    HIPCHK(c, c->sfSum.ensure((size_t)(w + 1) * (h + 1) * sizeof(int)));
    HIPCHK(c, c->sfDet.ensure(P.detFloats * sizeof(float) + 16));
    HIPCHK(c, c->sfTr.ensure(P.detFloats * sizeof(float) + 16));
    HIPCHK(c, c->sfLayers.ensure(P.L.size() * sizeof(fm3d::SurfLayer)));
    HIPCHK(c, c->sfMids.ensure(P.M.size() * sizeof(fm3d::SurfMid)));
    HIPCHK(c, c->sfCand.ensure((size_t)P.candCap * sizeof(fm3d::SurfCand)));
    HIPCHK(c, c->sfCount.ensure(64));
    HIPCHK(c, hipMemcpyAsync(c->sfLayers.p, P.L.data(), P.L.size() * sizeof(fm3d::SurfLayer), hipMemcpyHostToDevice,
                             c->stream));
    HIPCHK(c, hipMemcpyAsync(c->sfMids.p, P.M.data(), P.M.size() * sizeof(fm3d::SurfMid), hipMemcpyHostToDevice,
                             c->stream));
    HIPCHK(c, hipMemsetAsync(c->sfDet.p, 0, P.detFloats * sizeof(float), c->stream));
    HIPCHK(c, hipMemsetAsync(c->sfTr.p, 0, P.detFloats * sizeof(float), c->stream));
    HIPCHK(c, hipMemsetAsync(c->sfCount.p, 0, 64, c->stream));
    fm3d::launch_integral(c->sfImg.as<uint8_t>(), w, h, c->sfSum.as<int>(), c->stream);
    fm3d::launch_surf_hessian(c->sfSum.as<int>(), w, c->sfLayers.as<fm3d::SurfLayer>(), (int)P.L.size(), P.hTotal,
                              c->sfDet.as<float>(), c->sfTr.as<float>(), c->stream);
    fm3d::launch_surf_maxima(c->sfDet.as<float>(), c->sfTr.as<float>(), c->sfLayers.as<fm3d::SurfLayer>(),
                             c->sfMids.as<fm3d::SurfMid>(), (int)P.M.size(), P.mTotal, (float)S.surfHessianThreshold,
                             c->sfCand.as<fm3d::SurfCand>(), c->sfCount.as<int>(), (int)P.candCap, c->stream);
    HIPCHK(c, hipGetLastError());
    int nc = 0;
    HIPCHK(c, hipMemcpyAsync(&nc, c->sfCount.p, sizeof(int), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    if (nc > P.candCap) return fail(c, FM3D_ERR_HIP, "SURF candidate buffer overflow");
    const size_t sortBytes = fm3d::surf_sort_tmp_bytes(nc);
    HIPCHK(c, c->sfSortTmp.ensure(sortBytes + 16));
    fm3d::launch_surf_sort(c->sfCand.as<fm3d::SurfCand>(), nc, c->sfSortTmp.p, sortBytes, c->stream);
    if ((r = ensure_scan_tmp(c, nc))) return r;
    HIPCHK(c, c->sfFlag.ensure((size_t)(nc + 1) * sizeof(int)));
    HIPCHK(c, c->sfPos.ensure((size_t)(nc + 1) * sizeof(int)));
    HIPCHK(c, c->sfKp.ensure((size_t)(nc + 1) * sizeof(fm3d_keypoint)));
    int nk = 0;
    if (nc > 0) {
        const float* ang = nullptr;
        if (!S.surfUpright) {  // SURFInvoker's orientation; keypoints without a sample are removed
            HIPCHK(c, c->sfAng.ensure((size_t)(nc + 1) * sizeof(float)));
            fm3d::launch_surf_orient(c->sfCand.p, sizeof(fm3d::SurfCand), nc, c->sfSum.as<int>(), 0, w, h, surf_ori(),
                                     c->sfFlag.as<int>(), c->sfAng.as<float>(), c->stream);
            ang = c->sfAng.as<float>();
        }
        fm3d::launch_surf_upright(c->sfCand.as<fm3d::SurfCand>(), c->sfCount.as<int>(), nc, w, h, c->sfFlag.as<int>(),
                                  c->sfPos.as<int>(), c->count.as<int>(), c->scanTmp.p, c->sfKp.as<fm3d_keypoint>(),
                                  nullptr, ang, c->stream);
        HIPCHK(c, hipGetLastError());
        HIPCHK(c, hipMemcpyAsync(&nk, c->count.p, sizeof(int), hipMemcpyDeviceToHost, c->stream));
        HIPCHK(c, hipStreamSynchronize(c->stream));
    }
    const int nw = std::min(nk, cap);
    const int dsize = S.surfExtended ? 128 : 64;
    if (desc && nw > 0) {
        HIPCHK(c, c->sfDesc.ensure((size_t)nw * dsize * sizeof(float)));
        fm3d::launch_surf_describe(c->sfImg.as<uint8_t>(), 0, w, h, c->sfKp.as<fm3d_keypoint>(), nw, c->sfDW.as<float>(),
                                   S.surfExtended, S.surfUpright, c->sfDesc.as<float>(), c->stream);
        HIPCHK(c, hipGetLastError());
        HIPCHK(c, hipMemcpyAsync(desc, c->sfDesc.p, (size_t)nw * dsize * sizeof(float), hipMemcpyDeviceToHost,
                                 c->stream));
    }
    if (nw > 0)
        HIPCHK(c, hipMemcpyAsync(kpts, c->sfKp.p, (size_t)nw * sizeof(fm3d_keypoint), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    *n = nk;
    return FM3D_OK;
}

int fm3d_surf_compute(fm3d_ctx* c, const uint8_t* img, int w, int h, const fm3d_keypoint* kpts, int n,
                      fm3d_keypoint* kout, int32_t* kept, int* nOut, float* desc) {
    if (!c || !img || !nOut || w <= 0 || h <= 0 || n < 0 || (n > 0 && (!kpts || !kout || !desc)))
        return FM3D_ERR_INVALID;
    const fm3d_settings& S = c->s;
    if (S.extractorType != FM3D_FEAT_SURF) return fail(c, FM3D_ERR_UNSUPPORTED, "only the SURF extractor runs on the GPU");
    *nOut = 0;
    if (n == 0) return FM3D_OK;
    // a kept keypoint of size < 0.36 has an empty window: OpenCV's resize asserts (a window narrower
    // than the 21 x 21 patch, size < 7.5, is enlarged by the kernel as OpenCV's INTER_AREA does)
    for (int q = 0; q < n; q++) {
        const float sz = kpts[q].size, s = sz * 1.2f / 9.0f;
        const int gws = 2 * (int)std::lrint(2 * s);
        if (!(sz >= FLT_EPSILON) || h + 1 < gws || w + 1 < gws) continue;  // dropped anyway
        if ((int)((20 + 1) * s) < 1)
            return fail(c, FM3D_ERR_INVALID, "SURF compute: keypoint size < 0.36 (an empty window; OpenCV asserts)");
    }
    hipSetDevice(c->device);
    int r;
    if ((r = surf_upload_image(c, img, w, h))) return r;
    if ((r = ensure_scan_tmp(c, n))) return r;
    HIPCHK(c, c->sfKin.ensure((size_t)n * sizeof(fm3d_keypoint)));
    HIPCHK(c, c->sfKp.ensure((size_t)n * sizeof(fm3d_keypoint)));
    HIPCHK(c, c->sfFlag.ensure((size_t)(n + 1) * sizeof(int)));
    HIPCHK(c, c->sfPos.ensure((size_t)(n + 1) * sizeof(int)));
    HIPCHK(c, c->sfSrc.ensure((size_t)(n + 1) * sizeof(int)));
    HIPCHK(c, hipMemcpyAsync(c->sfKin.p, kpts, (size_t)n * sizeof(fm3d_keypoint), hipMemcpyHostToDevice, c->stream));
    const float* ang = nullptr;
    if (!S.surfUpright) {  // the orientation needs the integral image (SURF::operator() computes it)
        HIPCHK(c, c->sfSum.ensure((size_t)(w + 1) * (h + 1) * sizeof(int)));
        HIPCHK(c, c->sfAng.ensure((size_t)(n + 1) * sizeof(float)));
        fm3d::launch_integral(c->sfImg.as<uint8_t>(), w, h, c->sfSum.as<int>(), c->stream);
        fm3d::launch_surf_orient(c->sfKin.p, sizeof(fm3d_keypoint), n, c->sfSum.as<int>(), 0, w, h, surf_ori(),
                                 c->sfFlag.as<int>(), c->sfAng.as<float>(), c->stream);
        ang = c->sfAng.as<float>();
    }
    fm3d::launch_surf_keep(c->sfKin.as<fm3d_keypoint>(), n, w, h, c->sfFlag.as<int>(), c->sfPos.as<int>(),
                           c->count.as<int>(), c->scanTmp.p, c->sfKp.as<fm3d_keypoint>(), c->sfSrc.as<int>(), ang,
                           c->stream);
    HIPCHK(c, hipGetLastError());
    int nk = 0;
    HIPCHK(c, hipMemcpyAsync(&nk, c->count.p, sizeof(int), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    const int dsize = S.surfExtended ? 128 : 64;
    if (nk > 0) {
        HIPCHK(c, c->sfDesc.ensure((size_t)nk * dsize * sizeof(float)));
        fm3d::launch_surf_describe(c->sfImg.as<uint8_t>(), 0, w, h, c->sfKp.as<fm3d_keypoint>(), nk, c->sfDW.as<float>(),
                                   S.surfExtended, S.surfUpright, c->sfDesc.as<float>(), c->stream);
        HIPCHK(c, hipGetLastError());
        HIPCHK(c, hipMemcpyAsync(desc, c->sfDesc.p, (size_t)nk * dsize * sizeof(float), hipMemcpyDeviceToHost,
                                 c->stream));
        HIPCHK(c, hipMemcpyAsync(kout, c->sfKp.p, (size_t)nk * sizeof(fm3d_keypoint), hipMemcpyDeviceToHost, c->stream));
        if (kept)
            HIPCHK(c, hipMemcpyAsync(kept, c->sfSrc.p, (size_t)nk * sizeof(int), hipMemcpyDeviceToHost, c->stream));
    }
    HIPCHK(c, hipStreamSynchronize(c->stream));
    *nOut = nk;
    return FM3D_OK;
}

int fm3d_extract_descriptors_from_patches_any(fm3d_ctx* c, const uint8_t* patches, int P, int size, void* desc) {
    if (!c || P < 0 || size <= 0 || (P && (!patches || !desc))) return FM3D_ERR_INVALID;
    const int ex = c->s.extractorType;
    if (ex == FM3D_FEAT_SURF || ex == FM3D_FEAT_SIFT)
        return fm3d_extract_descriptors_from_patches(c, patches, P, size, static_cast<float*>(desc));
    if (ex != FM3D_FEAT_ORB && ex != FM3D_FEAT_BRISK && ex != FM3D_FEAT_FREAK)
        return fail(c, FM3D_ERR_UNSUPPORTED, "the settings' extractor type has no GPU implementation");
    // descriptorsmatcher.cpp:142-172: the centred keypoint per patch, compute on each patch; the rows
    // start as Mat::zeros and a dropped keypoint's empty row copies nothing
    const int cols = ex == FM3D_FEAT_ORB ? 32 : 64;
    uint8_t* d = static_cast<uint8_t*>(desc);
    std::memset(d, 0, (size_t)P * cols);
    if (ex == FM3D_FEAT_ORB) {
        // every patch has the same keypoint, so the keep rule and the rotated pattern are settled once;
        // then the tail's kernel on chunks of the tail's size, uploaded one after the other
        if (P == 0) return FM3D_OK;
        int r;
        if ((r = orb_patch_prepare(c, size))) return r;
        hipSetDevice(c->device);
        const int chunk = std::min(describe_chunk(), P);
        const size_t per = (size_t)size * size;
        HIPCHK(c, c->tailPatch.ensure((size_t)chunk * per));
        HIPCHK(c, c->tailDesc.ensure((size_t)P * cols));
        for (int p0 = 0; p0 < P; p0 += chunk) {
            const int m = std::min(chunk, P - p0);
            HIPCHK(c, hipMemcpyAsync(c->tailPatch.p, patches + per * p0, per * m, hipMemcpyHostToDevice, c->stream));
            orb_patch_describe(c, c->tailPatch.as<uint8_t>(), m, size, c->tailDesc.as<uint8_t>() + (size_t)p0 * cols);
            HIPCHK(c, hipGetLastError());
        }
        HIPCHK(c, hipMemcpyAsync(d, c->tailDesc.p, (size_t)P * cols, hipMemcpyDeviceToHost, c->stream));
        HIPCHK(c, hipStreamSynchronize(c->stream));
        return FM3D_OK;
    }
    const float center = (float)(int)std::floor(size / 2);
    const fm3d_keypoint k{center, center, (float)size, -1.f, 1.f, 0, 0};
    for (int p = 0; p < P; p++) {
        fm3d_keypoint ko;
        int m = 0, r;
        const uint8_t* img = patches + (size_t)p * size * size;
        r = ex == FM3D_FEAT_BRISK ? fm3d_brisk_compute(c, img, size, size, &k, 1, &ko, nullptr, &m, d + (size_t)p * cols)
                                  : fm3d_freak_compute(c, img, size, size, &k, 1, &ko, nullptr, &m, d + (size_t)p * cols);
        if (r) return r;
    }
    return FM3D_OK;
}

int fm3d_extract_descriptors_from_patches(fm3d_ctx* c, const uint8_t* patches, int P, int size, float* desc) {
    if (!c || P < 0 || size <= 0 || (P && (!patches || !desc))) return FM3D_ERR_INVALID;
    const fm3d_settings& S = c->s;
    if (S.extractorType == FM3D_FEAT_SIFT) return sift_patches(c, patches, P, size, desc);
    if (S.extractorType != FM3D_FEAT_SURF)
        return fail(c, FM3D_ERR_UNSUPPORTED, "only the SURF and SIFT extractors describe patches on the GPU");
    if (P == 0) return FM3D_OK;
    // descriptorsmatcher.cpp:146-158: one keypoint per patch at (center, center), center =
    // (int)floor(size / 2), size = the patch edge, angle -1, response 1, octave 0, class_id 0
    const float center = (float)(int)std::floor(size / 2);
    fm3d_keypoint k{center, center, (float)size, -1.f, 1.f, 0, 0};
    const float s = k.size * 1.2f / 9.0f;
    const int gws = 2 * cv_round_h(2 * s);
    if (size + 1 < gws) return fail(c, FM3D_ERR_INVALID, "patch keypoint dropped by SURF (descriptor row missing)");
    if (S.surfUpright) k.angle = 360.f - 90.f;
    hipSetDevice(c->device);
    const size_t per = (size_t)size * size;
    const int dsize = S.surfExtended ? 128 : 64;
    std::vector<fm3d_keypoint> kp((size_t)P, k);
    HIPCHK(c, c->sfImg.ensure((size_t)P * per));
    HIPCHK(c, c->sfKp.ensure((size_t)P * sizeof(fm3d_keypoint)));
    HIPCHK(c, c->sfDesc.ensure((size_t)P * dsize * sizeof(float)));
    HIPCHK(c, hipMemcpyAsync(c->sfImg.p, patches, (size_t)P * per, hipMemcpyHostToDevice, c->stream));
    HIPCHK(c, hipMemcpyAsync(c->sfKp.p, kp.data(), kp.size() * sizeof(fm3d_keypoint), hipMemcpyHostToDevice, c->stream));
    if (!S.surfUpright) {
        // every patch keypoint's orientation on that patch's integral image; a patch whose keypoint
        // has no orientation sample would lose its descriptor row (never for the centred keypoint
        // of a patch this size, but checked)
        const int r = ensure_scan_tmp(c, P);
        if (r) return r;
        const size_t sumPer = (size_t)(size + 1) * (size + 1);
        HIPCHK(c, c->sfSum.ensure((size_t)P * sumPer * sizeof(int)));
        HIPCHK(c, c->sfAng.ensure((size_t)(P + 1) * sizeof(float)));
        HIPCHK(c, c->sfFlag.ensure((size_t)(P + 1) * sizeof(int)));
        HIPCHK(c, c->sfPos.ensure((size_t)(P + 1) * sizeof(int)));
        HIPCHK(c, c->sfKin.ensure((size_t)P * sizeof(fm3d_keypoint)));
        HIPCHK(c, hipMemcpyAsync(c->sfKin.p, kp.data(), kp.size() * sizeof(fm3d_keypoint), hipMemcpyHostToDevice,
                                 c->stream));
        fm3d::launch_integral_batch(c->sfImg.as<uint8_t>(), size, size, P, c->sfSum.as<int>(), c->stream);
        fm3d::launch_surf_orient(c->sfKin.p, sizeof(fm3d_keypoint), P, c->sfSum.as<int>(), sumPer, size, size,
                                 surf_ori(), c->sfFlag.as<int>(), c->sfAng.as<float>(), c->stream);
        fm3d::launch_surf_keep(c->sfKin.as<fm3d_keypoint>(), P, size, size, c->sfFlag.as<int>(), c->sfPos.as<int>(),
                               c->count.as<int>(), c->scanTmp.p, c->sfKp.as<fm3d_keypoint>(), nullptr,
                               c->sfAng.as<float>(), c->stream);
        HIPCHK(c, hipGetLastError());
        int nk = 0;
        HIPCHK(c, hipMemcpyAsync(&nk, c->count.p, sizeof(int), hipMemcpyDeviceToHost, c->stream));
        HIPCHK(c, hipStreamSynchronize(c->stream));
        if (nk != P) return fail(c, FM3D_ERR_INVALID, "patch keypoint dropped by SURF (no orientation sample)");
    }
    if (c->sfDW.bytes == 0) {
        const std::vector<float> dw = surf_dw();
        HIPCHK(c, c->sfDW.ensure(400 * sizeof(float)));
        HIPCHK(c, hipMemcpyAsync(c->sfDW.p, dw.data(), 400 * sizeof(float), hipMemcpyHostToDevice, c->stream));
        HIPCHK(c, hipStreamSynchronize(c->stream));
    }
    fm3d::launch_surf_describe(c->sfImg.as<uint8_t>(), per, size, size, c->sfKp.as<fm3d_keypoint>(), P,
                               c->sfDW.as<float>(), S.surfExtended, S.surfUpright, c->sfDesc.as<float>(), c->stream);
    HIPCHK(c, hipGetLastError());
    HIPCHK(c, hipMemcpyAsync(desc, c->sfDesc.p, (size_t)P * dsize * sizeof(float), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    return FM3D_OK;
}

int fm3d_orb_set_pattern(fm3d_ctx* c, const int32_t* xy, int npoints) {
    if (!c || (xy && npoints != 512)) return FM3D_ERR_INVALID;
    c->orbUserPattern.clear();
    if (xy) c->orbUserPattern.assign(xy, xy + 1024);
    c->orbTabReach = 0;  // the patch path's offset table is of the old pattern
    return FM3D_OK;
}

int fm3d_orb_detect(fm3d_ctx* c, const uint8_t* img, int w, int h, fm3d_keypoint* kpts, int cap, int* n,
                    uint8_t* desc) {
    if (!c || !img || !n || w <= 0 || h <= 0 || cap < 0 || (cap > 0 && !kpts)) return FM3D_ERR_INVALID;
    const fm3d_settings& S = c->s;
    if (S.detectorType != FM3D_FEAT_ORB || (desc && S.extractorType != FM3D_FEAT_ORB))
        return fail(c, FM3D_ERR_UNSUPPORTED, "the settings' detector (extractor) is not ORB");
    int r;
    if ((r = orb_check_settings(c))) return r;
    hipSetDevice(c->device);
    const int nl = S.orbNumLevels, half = S.orbPatchSize / 2;
    // computeKeyPoints: features per level
    std::vector<int> nper(nl);
    {
        const float factor = (float)(1.0 / S.orbScaleFactor);
        float nd = S.orbNumFeatures * (1 - factor) / (1 - (float)std::pow((double)factor, (double)nl));
        int sum = 0;
        for (int l = 0; l < nl - 1; l++) {
            nper[l] = (int)std::lrint(nd);
            sum += nper[l];
            nd *= factor;
        }
        nper[nl - 1] = std::max(S.orbNumFeatures - sum, 0);
    }
    const OrbPlan P = orb_plan(w, h, S.orbScaleFactor, nl);
    if ((r = orb_build_pyramid(c, img, w, h, P))) return r;
    // FAST + non-max + border over all levels, compacted in level-major raster order
    if (P.total > INT32_MAX / 2) return fail(c, FM3D_ERR_INVALID, "image too large for the ORB pyramid");
    const int tot = (int)P.total;
    if ((r = ensure_scan_tmp(c, tot))) return r;
    HIPCHK(c, c->orbMap.ensure((size_t)tot * sizeof(uint16_t) + 64));
    HIPCHK(c, c->orbFlag.ensure((size_t)(tot + 1) * sizeof(int)));
    HIPCHK(c, c->orbPos.ensure((size_t)(tot + 1) * sizeof(int)));
    fm3d::launch_orb_fast(c->orbPyr.as<uint8_t>(), c->orbLev.as<fm3d::OrbLevel>(), nl, P.total, S.orbFastThreshold,
                          S.orbEdgeThreshold, 1, c->orbMap.as<uint16_t>(), c->orbFlag.as<int>(), c->stream);
    fm3d::launch_exclusive_scan(c->orbFlag.as<int>(), tot, c->orbPos.as<int>(), c->count.as<int>(), c->scanTmp.p,
                                c->stream);
    HIPCHK(c, hipGetLastError());
    int nc = 0;
    HIPCHK(c, hipMemcpyAsync(&nc, c->count.p, sizeof(int), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    HIPCHK(c, c->orbKp.ensure((size_t)(nc + 1) * sizeof(fm3d_keypoint)));
    fm3d::launch_orb_fast_scatter(c->orbMap.as<uint16_t>(), c->orbLev.as<fm3d::OrbLevel>(), nl, P.total,
                                  c->orbFlag.as<int>(), c->orbPos.as<int>(), c->orbKp.as<fm3d_keypoint>(), c->stream);
    std::vector<fm3d_keypoint> k((size_t)nc + 1);
    if (nc > 0)
        HIPCHK(c, hipMemcpyAsync(k.data(), c->orbKp.p, (size_t)nc * sizeof(fm3d_keypoint), hipMemcpyDeviceToHost,
                                 c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    // per level: retainBest(2 * n), Harris, retainBest(n)
    std::vector<int> start(nl + 1, 0);
    for (int i = 0; i < nc; i++) start[k[i].octave + 1]++;
    for (int l = 0; l < nl; l++) start[l + 1] += start[l];
    std::vector<fm3d_keypoint> kb;
    std::vector<int> bstart(nl + 1, 0);
    for (int l = 0; l < nl; l++) {
        const int m = orb_retain_best(k.data() + start[l], start[l + 1] - start[l], 2 * nper[l]);
        kb.insert(kb.end(), k.begin() + start[l], k.begin() + start[l] + m);
        bstart[l + 1] = (int)kb.size();
    }
    const int nb = (int)kb.size();
    if (nb > 0) {
        HIPCHK(c, hipMemcpyAsync(c->orbKp.p, kb.data(), (size_t)nb * sizeof(fm3d_keypoint), hipMemcpyHostToDevice,
                                 c->stream));
        fm3d::launch_orb_harris(c->orbPyr.as<uint8_t>(), c->orbLev.as<fm3d::OrbLevel>(), c->orbKp.as<fm3d_keypoint>(),
                                nb, c->stream);
        HIPCHK(c, hipGetLastError());
        HIPCHK(c, hipMemcpyAsync(kb.data(), c->orbKp.p, (size_t)nb * sizeof(fm3d_keypoint), hipMemcpyDeviceToHost,
                                 c->stream));
        HIPCHK(c, hipStreamSynchronize(c->stream));
    }
    std::vector<fm3d_keypoint> kf;
    for (int l = 0; l < nl; l++) {
        const int m = orb_retain_best(kb.data() + bstart[l], bstart[l + 1] - bstart[l], nper[l]);
        const float sf = orb_scale(S.orbScaleFactor, l);
        for (int i = 0; i < m; i++) {
            fm3d_keypoint q = kb[bstart[l] + i];
            q.octave = l;
            q.size = S.orbPatchSize * sf;
            kf.push_back(q);
        }
    }
    const int nf = (int)kf.size(), nw = std::min(nf, cap);
    if (nf > 0) {
        fm3d::OrbUmax um{};
        {  // computeKeyPoints' umax
            const int vmax = (int)std::floor(half * std::sqrt(2.f) / 2 + 1);
            const int vmin = (int)std::ceil(half * std::sqrt(2.f) / 2);
            for (int v = 0; v <= vmax; ++v) um.u[v] = (int)std::lrint(std::sqrt((double)half * half - v * v));
            for (int v = half, v0 = 0; v >= vmin; --v) {
                while (um.u[v0] == um.u[v0 + 1]) ++v0;
                um.u[v] = v0;
                ++v0;
            }
        }
        HIPCHK(c, hipMemcpyAsync(c->orbKp.p, kf.data(), (size_t)nf * sizeof(fm3d_keypoint), hipMemcpyHostToDevice,
                                 c->stream));
        fm3d::launch_orb_angle(c->orbPyr.as<uint8_t>(), c->orbLev.as<fm3d::OrbLevel>(), c->orbKp.as<fm3d_keypoint>(), nf,
                               half, um, c->stream);
        HIPCHK(c, hipGetLastError());
        if (desc && nw > 0 && (r = orb_describe(c, P, nw, desc))) return r;
        HIPCHK(c, hipMemcpyAsync(kf.data(), c->orbKp.p, (size_t)nf * sizeof(fm3d_keypoint), hipMemcpyDeviceToHost,
                                 c->stream));
        HIPCHK(c, hipStreamSynchronize(c->stream));
    }
    for (int i = 0; i < nw; i++) {
        fm3d_keypoint q = kf[i];
        if (q.octave != 0) {
            const float sf = orb_scale(S.orbScaleFactor, q.octave);
            q.x *= sf;
            q.y *= sf;
        }
        kpts[i] = q;
    }
    *n = nf;
    return FM3D_OK;
}

int fm3d_sift_detect(fm3d_ctx* c, const uint8_t* img, int w, int h, fm3d_keypoint* kpts, int cap, int* n,
                     float* desc) {
    if (!c || !img || !n || w <= 0 || h <= 0 || cap < 0 || (cap > 0 && !kpts)) return FM3D_ERR_INVALID;
    const fm3d_settings& S = c->s;
    if (S.detectorType != FM3D_FEAT_SIFT || (desc && S.extractorType != FM3D_FEAT_SIFT))
        return fail(c, FM3D_ERR_UNSUPPORTED, "the settings' detector (extractor) is not SIFT");
    int r;
    if ((r = sift_check_settings(c))) return r;
    hipSetDevice(c->device);
    const int L = S.siftOctaveLayers, firstOctave = -1;
    const int nOct = sift_num_octaves(w, h, firstOctave);
    std::vector<fm3d_keypoint> k;
    SiftPlan P;
    if (nOct >= 1) {
        if (!sift_plan(w, h, firstOctave, nOct, L, P))
            return fail(c, FM3D_ERR_INVALID, "SIFT: an octave of the image would be empty");
        if ((r = sift_build(c, img, w, h, P, true))) return r;
        // findScaleSpaceExtrema: flags over every (octave, layer 1..L, row, column), compacted in that order
        std::vector<fm3d::SiftScan> scan;
        long long total = 0;
        for (int o = 0; o < nOct; o++)
            for (int i = 1; i <= L; i++) {
                const fm3d::SiftLevel& d = P.D[o * (L + 2) + i];
                scan.push_back({total, o * (L + 2) + i, o, i, 0});
                total += (long long)d.w * d.h;
            }
        if (total > INT32_MAX / 2) return fail(c, FM3D_ERR_INVALID, "image too large for the SIFT scan");
        const int tot = (int)total;
        const int threshold = (int)std::floor(0.5 * S.siftContrastThreshold / L * 255 * 1);
        HIPCHK(c, c->siftScan.ensure(scan.size() * sizeof(fm3d::SiftScan)));
        HIPCHK(c, hipMemcpyAsync(c->siftScan.p, scan.data(), scan.size() * sizeof(fm3d::SiftScan), hipMemcpyHostToDevice,
                                 c->stream));
        if ((r = ensure_scan_tmp(c, tot))) return r;
        HIPCHK(c, c->siftFlag.ensure((size_t)(tot + 1) * sizeof(int)));
        HIPCHK(c, c->siftPos.ensure((size_t)(tot + 1) * sizeof(int)));
        fm3d::launch_sift_extrema(c->siftD.as<float>(), c->siftDL.as<fm3d::SiftLevel>(), c->siftScan.as<fm3d::SiftScan>(),
                                  (int)scan.size(), total, threshold, c->siftFlag.as<int>(), c->stream);
        fm3d::launch_exclusive_scan(c->siftFlag.as<int>(), tot, c->siftPos.as<int>(), c->count.as<int>(), c->scanTmp.p,
                                    c->stream);
        HIPCHK(c, hipGetLastError());
        int nc = 0;
        HIPCHK(c, hipMemcpyAsync(&nc, c->count.p, sizeof(int), hipMemcpyDeviceToHost, c->stream));
        HIPCHK(c, hipStreamSynchronize(c->stream));
        if (nc > 0) {
            HIPCHK(c, c->siftCand.ensure((size_t)nc * sizeof(fm3d::SiftCand)));
            HIPCHK(c, c->siftAng.ensure((size_t)nc * 36 * sizeof(float)));
            HIPCHK(c, c->siftNpk.ensure((size_t)nc * sizeof(int)));
            fm3d::launch_sift_cand_scatter(c->siftDL.as<fm3d::SiftLevel>(), c->siftScan.as<fm3d::SiftScan>(),
                                           (int)scan.size(), total, c->siftFlag.as<int>(), c->siftPos.as<int>(),
                                           c->siftCand.as<fm3d::SiftCand>(), c->stream);
            fm3d::launch_sift_adjust(c->siftD.as<float>(), c->siftDL.as<fm3d::SiftLevel>(), L,
                                     (float)S.siftContrastThreshold, (float)S.siftEdgeThreshold, (float)S.siftSigma,
                                     c->siftCand.as<fm3d::SiftCand>(), nc, c->stream);
            fm3d::launch_sift_orient(c->siftG.as<float>(), c->siftGL.as<fm3d::SiftLevel>(), L,
                                     c->siftCand.as<fm3d::SiftCand>(), nc, c->siftAng.as<float>(),
                                     c->siftNpk.as<int>(), c->stream);
            HIPCHK(c, hipGetLastError());
            std::vector<fm3d::SiftCand> cand(nc);
            std::vector<int> npk(nc);
            std::vector<float> ang((size_t)nc * 36);
            HIPCHK(c, hipMemcpyAsync(cand.data(), c->siftCand.p, (size_t)nc * sizeof(fm3d::SiftCand),
                                     hipMemcpyDeviceToHost, c->stream));
            HIPCHK(c, hipMemcpyAsync(npk.data(), c->siftNpk.p, (size_t)nc * sizeof(int), hipMemcpyDeviceToHost, c->stream));
            HIPCHK(c, hipMemcpyAsync(ang.data(), c->siftAng.p, ang.size() * sizeof(float), hipMemcpyDeviceToHost,
                                     c->stream));
            HIPCHK(c, hipStreamSynchronize(c->stream));
            for (int q = 0; q < nc; q++) {
                const fm3d::SiftCand& C = cand[q];
                if (!C.ok) continue;
                for (int p = 0; p < npk[q]; p++)
                    k.push_back({C.x, C.y, C.size, ang[(size_t)q * 36 + p], C.response, C.koct, -1});
            }
        }
        sift_remove_duplicated(k);
        if (S.siftNumFeatures > 0) k.resize(orb_retain_best(k.data(), (int)k.size(), S.siftNumFeatures));
        for (auto& q : k) {  // firstOctave -1: back to the image's coordinates
            const float scale = 1.f / (float)(1 << -firstOctave);
            q.octave = (q.octave & ~255) | ((q.octave + firstOctave) & 255);
            q.x *= scale;
            q.y *= scale;
            q.size *= scale;
        }
    }
    const int nf = (int)k.size(), nw = std::min(nf, cap);
    for (int i = 0; i < nw; i++) kpts[i] = k[i];
    *n = nf;
    if (desc && nw > 0) {
        // the reference's separate compute (runByKeypointSize keeps all: detected sizes are > 0)
        std::vector<fm3d_keypoint> kd(k.begin(), k.begin() + nw);
        if ((r = sift_describe(c, img, w, h, kd, desc, nOct >= 1 ? &P : nullptr))) return r;
    }
    return FM3D_OK;
}

int fm3d_sift_compute(fm3d_ctx* c, const uint8_t* img, int w, int h, const fm3d_keypoint* kpts, int n,
                      fm3d_keypoint* kout, int32_t* kept, int* nOut, float* desc) {
    if (!c || !img || !nOut || w <= 0 || h <= 0 || n < 0 || (n > 0 && (!kpts || !kout || !desc)))
        return FM3D_ERR_INVALID;
    if (c->s.extractorType != FM3D_FEAT_SIFT) return fail(c, FM3D_ERR_UNSUPPORTED, "the settings' extractor is not SIFT");
    int r;
    if ((r = sift_check_settings(c))) return r;
    hipSetDevice(c->device);
    // DescriptorExtractor::compute: runByKeypointSize(FLT_EPSILON) (runByImageBorder(0) keeps all)
    std::vector<fm3d_keypoint> k;
    std::vector<int> src;
    for (int i = 0; i < n; i++)
        if (!(kpts[i].size < FLT_EPSILON || kpts[i].size > FLT_MAX)) {
            k.push_back(kpts[i]);
            src.push_back(i);
        }
    if ((r = sift_describe(c, img, w, h, k, desc, nullptr))) return r;
    for (size_t i = 0; i < k.size(); i++) {
        kout[i] = k[i];
        if (kept) kept[i] = src[i];
    }
    *nOut = (int)k.size();
    return FM3D_OK;
}

int fm3d_sift_pyramid(fm3d_ctx* c, const uint8_t* img, int w, int h, int firstOctave, int nOctaves, int dog,
                      float* out, int32_t* sizes, int64_t* total) {
    if (!c || !img || !total || w <= 0 || h <= 0 || firstOctave < -1 || firstOctave > 0 || nOctaves < 1)
        return FM3D_ERR_INVALID;
    int r;
    if ((r = sift_check_settings(c))) return r;
    hipSetDevice(c->device);
    SiftPlan P;
    if (!sift_plan(w, h, firstOctave, nOctaves, c->s.siftOctaveLayers, P))
        return fail(c, FM3D_ERR_INVALID, "SIFT: an octave of the image would be empty");
    const std::vector<fm3d::SiftLevel>& Lv = dog ? P.D : P.G;
    *total = dog ? P.dTotal : P.gTotal;
    if (sizes)
        for (size_t i = 0; i < Lv.size(); i++) {
            sizes[2 * i] = Lv[i].w;
            sizes[2 * i + 1] = Lv[i].h;
        }
    if (!out) return FM3D_OK;
    if ((r = sift_build(c, img, w, h, P, dog != 0))) return r;
    HIPCHK(c, hipMemcpyAsync(out, dog ? c->siftD.p : c->siftG.p, (size_t)*total * sizeof(float), hipMemcpyDeviceToHost,
                             c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    return FM3D_OK;
}

int fm3d_fast_detect(fm3d_ctx* c, const uint8_t* img, int w, int h, int threshold, int nonmax, fm3d_keypoint* kpts,
                     int cap, int* n) {
    if (!c || !img || !n || w <= 0 || h <= 0 || cap < 0 || (cap > 0 && !kpts)) return FM3D_ERR_INVALID;
    hipSetDevice(c->device);
    std::vector<fm3d_keypoint> k;
    int r;
    if ((r = fast_detect(c, img, w, h, threshold, nonmax != 0, k))) return r;
    for (int i = 0; i < (int)k.size() && i < cap; i++) kpts[i] = k[i];
    *n = (int)k.size();
    return FM3D_OK;
}

// ---------------------------------------------------------------- BRISK extractor
// cv::BRISK's descriptor on given keypoints (OpenCV 2.4.9 brisk.cpp; oracle/orc_brisk.c): what OpenCV's
// constructor precomputes (pattern points per scale and rotation, the short pairs, the size list) and
// its per-keypoint bookkeeping (scale, rotation bin, border filter) stay on the host, in the same
// float / double expressions and glibc calls; the intensities and bits run on the GPU.
}  // extern "C"
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

fm3d::MserParams mser_params(int delta, int minArea, int maxArea, double maxVariation, double minDiversity) {
    fm3d::MserParams P;
    P.delta = delta;
    P.minArea = minArea;
    P.maxArea = maxArea;
    P.maxVariation = maxVariation;
    P.minDiversity = minDiversity;
    return P;
}

// MserFeatureDetector::detect: the kept keypoints in region order
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
}  // namespace

// for fm3d_patch_keypoint_kept: the border that brisk_compute / freak_compute hold a keypoint's size to
namespace fm3d_host {
int brisk_border(float kpSize) { return brisk::size_of(brisk::kscale(kpSize)); }
int freak_border(float kpSize) { return freak::pattern().sizes[freak::kscale(kpSize)]; }
}  // namespace fm3d_host

extern "C" {
int fm3d_mser_detect(fm3d_ctx* c, const uint8_t* img, int w, int h, int delta, int minArea, int maxArea,
                     double maxVariation, double minDiversity, fm3d_keypoint* kpts, int cap, int* n) {
    if (!c || !img || !n || w <= 0 || h <= 0 || cap < 0 || (cap > 0 && !kpts)) return FM3D_ERR_INVALID;
    hipSetDevice(c->device);
    std::vector<fm3d_keypoint> k;
    std::vector<int> per;
    int r;
    if ((r = mser_detect(c, img, 1, w, h, mser_params(delta, minArea, maxArea, maxVariation, minDiversity), k, per)))
        return r;
    for (int i = 0; i < (int)k.size() && i < cap; i++) kpts[i] = k[i];
    *n = (int)k.size();
    return FM3D_OK;
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

int fm3d_orb_compute(fm3d_ctx* c, const uint8_t* img, int w, int h, const fm3d_keypoint* kpts, int n,
                     fm3d_keypoint* kout, int32_t* kept, int* nOut, uint8_t* desc) {
    if (!c || !img || !nOut || w <= 0 || h <= 0 || n < 0 || (n > 0 && (!kpts || !kout || !desc)))
        return FM3D_ERR_INVALID;
    const fm3d_settings& S = c->s;
    if (S.extractorType != FM3D_FEAT_ORB) return fail(c, FM3D_ERR_UNSUPPORTED, "the settings' extractor is not ORB");
    int r;
    if ((r = orb_check_settings(c))) return r;
    *nOut = 0;
    if (n == 0) return FM3D_OK;
    const int b = S.orbEdgeThreshold;
    // runByKeypointSize(FLT_EPSILON) (NaN kept), runByImageBorder(edgeThreshold) on rounded positions
    std::vector<int> src;
    int L = 0;
    for (int i = 0; i < n; i++) {
        const float sz = kpts[i].size;
        if (sz < FLT_EPSILON || sz > FLT_MAX) continue;
        if (b > 0) {
            if (h <= 2 * b || w <= 2 * b) continue;
            const long ix = std::lrint(kpts[i].x), iy = std::lrint(kpts[i].y);
            if (!(ix >= b && ix < b + (w - 2 * b) && iy >= b && iy < b + (h - 2 * b))) continue;
        }
        if (kpts[i].octave < 0) return fail(c, FM3D_ERR_INVALID, "ORB compute: keypoint with a negative octave");
        if (kpts[i].octave >= 64) return fail(c, FM3D_ERR_INVALID, "ORB compute: keypoint octave >= 64");
        L = std::max(L, kpts[i].octave + 1);
        src.push_back(i);
    }
    if (src.empty()) return FM3D_OK;
    // grouped by octave (input order within a level), positions in level coordinates
    std::vector<fm3d_keypoint> k;
    std::vector<int> order;
    for (int l = 0; l < L; l++) {
        const float inv = 1 / orb_scale(S.orbScaleFactor, l);
        for (int i : src) {
            if (kpts[i].octave != l) continue;
            fm3d_keypoint q = kpts[i];
            if (l != 0) {
                q.x *= inv;
                q.y *= inv;
            }
            k.push_back(q);
            order.push_back(i);
        }
    }
    hipSetDevice(c->device);
    const OrbPlan P = orb_plan(w, h, S.orbScaleFactor, L);
    for (const fm3d_keypoint& q : k) {  // the descriptor's reads stay inside the level
        const fm3d::OrbLevel& lv = P.L[q.octave];
        const long ix = std::lrint(q.x), iy = std::lrint(q.y);
        const int reach = (int)std::ceil(S.orbPatchSize / 2 * 1.4143) + 4;
        if (ix < reach || iy < reach || ix >= lv.w - reach || iy >= lv.h - reach)
            return fail(c, FM3D_ERR_INVALID, "ORB compute: keypoint octave inconsistent with its position");
    }
    if ((r = orb_build_pyramid(c, img, w, h, P))) return r;
    const int m = (int)k.size();
    HIPCHK(c, c->orbKp.ensure((size_t)m * sizeof(fm3d_keypoint)));
    HIPCHK(c, hipMemcpyAsync(c->orbKp.p, k.data(), (size_t)m * sizeof(fm3d_keypoint), hipMemcpyHostToDevice, c->stream));
    if ((r = orb_describe(c, P, m, desc))) return r;
    HIPCHK(c, hipStreamSynchronize(c->stream));
    for (int i = 0; i < m; i++) {
        fm3d_keypoint q = k[i];
        if (q.octave != 0) {
            const float sf = orb_scale(S.orbScaleFactor, q.octave);
            q.x *= sf;
            q.y *= sf;
        }
        kout[i] = q;
        if (kept) kept[i] = order[i];
    }
    *nOut = m;
    return FM3D_OK;
}

int fm3d_patch_keypoint_kept_for(const fm3d_settings* s, int size, int* kept) {
    if (!s || !kept || size <= 0) return FM3D_ERR_INVALID;
    // descriptorsmatcher.cpp:146-158: the keypoint of every patch of this edge, on a size x size image
    const float ctr = (float)(int)std::floor(size / 2), ks = (float)size;
    switch (s->extractorType) {
    case FM3D_FEAT_SURF:  // fm3d_surf_compute: the wavelet against the image
        *kept = size + 1 >= surf_patch_gws(size);
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
