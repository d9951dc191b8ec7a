// fm3d_host.cpp -- C ABI (include/fm3d.h): context life cycle, g12, images and pyramids, DLT, the
// small one-off entry points, and the helpers the other host files share (fm3d_ctx.h).
//
// The matchers are fm3d_matching.cpp's, the LM host fm3d_lm.cpp's, the staged pipeline
// fm3d_pipeline.cpp's, the context-free host algebra fm3d_algebra.cpp's, the detectors and
// extractors fm3d_features.cpp's.  There is no CPU fallback: without a GPU every compute entry
// point fails with FM3D_ERR_HIP.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cfloat>
#include <cmath>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "fm3d.h"
#include "fm3d_ctx.h"
#include "fm3d_internal.h"
#include "fm3d_kernels.h"

using fm3d::LevelDesc;

using namespace fm3d_host;

namespace fm3d_host {  // (declared in fm3d_ctx.h)

int ensure_scan_tmp(fm3d_ctx* c, int n) {
    HIPCHK(c, c->scanTmp.ensure(fm3d::scan_tmp_bytes(n < 1 ? 1 : n)));
    HIPCHK(c, c->count.ensure(64));
    return FM3D_OK;
}

void install_g12(fm3d_ctx* c, const double g[16]) {
    std::memcpy(c->g12, g, sizeof(c->g12));
    camera2_from_g12(c->g12, c->R2, c->t2);
    c->haveG12 = true;
    c->gateStaged = false;  // the staged pair's epipolar lines belong to the previous pose
}

bool good_max_px(double v) { return v > 0. && v <= DBL_MAX; }  // finite and > 0 (false for NaN)

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

// the two images into pinned staging and their pyramids (pyrDown chain) on the context stream;
// sync: wait for them before returning (fm3d_set_images: the caller may read them back at once)
int set_images_impl(fm3d_ctx* c, const uint8_t* img1, const uint8_t* img2, int width, int height, int stride,
                    bool sync, bool waitStaging) {
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
    c->pyr2t.resize(levels + 1);
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
        void* pt = c->pyr2t[L].p;
        HIPCHK(c, c->pyr1[L].ensure(bytes));
        HIPCHK(c, c->pyr2[L].ensure(bytes));
        HIPCHK(c, c->pyr2t[L].ensure(kColBytes(c->lw[L], c->lh[L])));
        fresh |= c->pyr1[L].p != p1 || c->pyr2[L].p != p2 || c->pyr2t[L].p != pt;
    }
    for (int L = 0; fresh && L <= levels; L++) {
        // a level's pixels are overwritten (level 0 by the copy below, the others by pyrDown): the
        // guard past them is what needs clearing
        const size_t img = (size_t)c->lw[L] * c->lh[L];
        HIPCHK(c, hipMemsetAsync((char*)c->pyr1[L].p + img, 0, c->pyr1[L].bytes - img, c->stream));
        HIPCHK(c, hipMemsetAsync((char*)c->pyr2[L].p + img, 0, c->pyr2[L].bytes - img, c->stream));
        // the column-major copy's guard cells lie between its columns: the whole buffer (the copy's
        // writers touch the same cells for every frame pair of this geometry)
        HIPCHK(c, hipMemsetAsync(c->pyr2t[L].p, 0, c->pyr2t[L].bytes, c->stream));
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
    fm3d::launch_level_transpose(c->pyr2[0].as<uint8_t>(), width, height, c->pyr2t[0].as<uint8_t>(), kColStride(height),
                                 c->stream);
    for (int L = 1; L <= levels; L++) {
        fm3d::launch_pyrdown(c->pyr1[L - 1].as<uint8_t>(), c->lw[L - 1], c->lh[L - 1], c->pyr1[L].as<uint8_t>(),
                             c->stream);
        fm3d::launch_pyrdown(c->pyr2[L - 1].as<uint8_t>(), c->lw[L - 1], c->lh[L - 1], c->pyr2[L].as<uint8_t>(),
                             c->stream, c->pyr2t[L].as<uint8_t>(), kColStride(c->lh[L]));
    }
    HIPCHK(c, hipGetLastError());
    HIPCHK(c, c->hTab.ensure((levels + 1) * sizeof(LevelDesc)));
    LevelDesc* d = c->hTab.as<LevelDesc>();
    for (int L = 0; L <= levels; L++)
        d[L] = LevelDesc{c->pyr1[L].as<uint8_t>(), c->pyr2[L].as<uint8_t>(), c->lw[L], c->lh[L],
                         c->pyr2t[L].as<uint8_t>(), kColStride(c->lh[L])};
    HIPCHK(c, c->lvlDesc.ensure((levels + 1) * sizeof(LevelDesc)));
    HIPCHK(c, hipMemcpyAsync(c->lvlDesc.p, d, (levels + 1) * sizeof(LevelDesc), hipMemcpyHostToDevice, c->stream));
    HIPCHK(c, hipEventRecord(c->evStage, c->stream));
    if (sync) HIPCHK(c, hipStreamSynchronize(c->stream));
    return FM3D_OK;
}

// the DLT's parameters over c's keypoints, matches (K of them, or K their bound) and pose, into
// c->triPts / c->triMask
fm3d::TriParams tri_params(fm3d_ctx* c, int K, int queryOffset) {
    fm3d::TriParams p{};
    p.cam = c->cam;
    std::memcpy(p.g12, c->g12, sizeof(p.g12));
    p.zmin = c->s.zThresholdMin;
    p.zmax = c->s.zThresholdMax;
    p.kp1 = c->kp1.as<fm3d_point2f>();
    p.kp2 = c->kp2.as<fm3d_point2f>();
    p.matches = c->matches.as<fm3d_dmatch>();
    p.K = K;
    p.queryOffset = queryOffset;
    p.pts = c->triPts.as<double>();
    p.mask = c->triMask.as<int>();
    p.dltSolver = c->s.dltSolver;
    return p;
}

// the NCC scoring's parameters but its points and outputs: c's pose, level-0 images and circle offsets
fm3d::NccParams ncc_params(fm3d_ctx* c, int Hphi, int Htheta, double span) {
    fm3d::NccParams p{};
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
    return p;
}

}  // namespace fm3d_host

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
    hipEventCreateWithFlags(&c->pipe.evFront, hipEventDisableTiming);
    hipEventCreateWithFlags(&c->pipe.evLm, hipEventDisableTiming);
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
    if (c->pipe.linkLeader) {
        auto& v = c->pipe.linkLeader->pipe.linkMembers;
        v.erase(std::remove(v.begin(), v.end(), c), v.end());
    }
    for (fm3d_ctx* m : c->pipe.linkMembers) m->pipe.linkLeader = nullptr;
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
    fm3d::TriParams p = tri_params(c, K, 0);
    p.mask8 = c->triMask8.as<uint8_t>();
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

int fm3d_internal_level_cols(fm3d_ctx* c, int level, uint8_t* out, int* w, int* h, int* hs, size_t* bytes) {
    if (!c || level < 0 || level >= (int)c->pyr2t.size()) return FM3D_ERR_INVALID;
    hipSetDevice(c->device);
    const size_t n = kColBytes(c->lw[level], c->lh[level]);
    if (w) *w = c->lw[level];
    if (h) *h = c->lh[level];
    if (hs) *hs = kColStride(c->lh[level]);
    if (bytes) *bytes = n;
    if (out) HIPCHK(c, hipMemcpy(out, c->pyr2t[level].p, n, hipMemcpyDeviceToHost));
    return FM3D_OK;
}

int fm3d_internal_lm_img2_cols(const fm3d_ctx* c) { return c ? c->lmCols : -1; }

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
    fm3d::NccParams p = ncc_params(c, Hphi, Htheta, span);
    p.points = X.as<double>();
    p.P = P;
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
