// fm3d_localize.cpp -- 2D-3D localisation, the host side: fm3d_localize_points'
// orchestration, the matcher in front of it (fm3d_localize_model) and the context-free algebra (quartic,
// P3P, count, Gauss-Newton step).  The arithmetic is include/fm3d_pnp.h's; the kernels are
// fm3d_localize.hip's.
#include <hip/hip_runtime.h>

#include <cfloat>
#include <cmath>
#include <cstring>
#include <string>
#include <vector>

#include "fm3d.h"
#include "fm3d_ctx.h"
#include "fm3d_kernels.h"
#include "fm3d_pnp.h"

using namespace fm3d_host;
namespace pnp = fm3d_pnp;

namespace {

// one block carved in 256-byte steps
struct Carver {
    size_t off = 0;
    size_t take(size_t bytes) {
        const size_t at = off;
        off += (bytes + 255) & ~(size_t)255;
        return at;
    }
};

// the caller's optional and required outputs of one localisation
struct LocalizeOut {
    double* g;
    uint8_t* inlierMask;
    fm3d_dmatch* inliers;
    int *nInliers, *best;
    int32_t* counts;
    double* models;
    int32_t* roundCounts;
    double* roundModels;
    int* roundsAdopted;
};

// the rules of fm3d_localize_opts, before any launch
int check_opts(fm3d_ctx* c, const fm3d_localize_opts* o) {
    if (o->samples < 1) return fail(c, FM3D_ERR_INVALID, "samples must be >= 1");
    if (!(o->maxPx > 0. && o->maxPx <= DBL_MAX)) return fail(c, FM3D_ERR_INVALID, "maxPx must be finite and > 0");
    if (!(o->minFacingCos >= 0. && o->minFacingCos <= 1.)) return fail(c, FM3D_ERR_INVALID, "minFacingCos must be in 0 .. 1");
    if (o->refineIters < 0 || o->refineIters > pnp::kMaxIters)
        return fail(c, FM3D_ERR_INVALID, "refineIters must be in 0 .. 16");
    if (o->samples > fm3d::kVerifyMaxHyps / pnp::kSlots) return fail(c, FM3D_ERR_UNSUPPORTED, "more than 2^18 samples");
    return FM3D_OK;
}

// what the outputs hold until a model exists
void clear_outputs(const LocalizeOut& out, int M, int H, int R) {
    for (int k = 0; k < 16; k++) out.g[k] = 0.;
    *out.nInliers = 0;
    *out.best = -1;
    if (M) std::memset(out.inlierMask, 0, (size_t)M);
    // until a round runs: no best model gives c_0 = -1, and every round -2 and a zero candidate
    if (out.roundCounts) {
        out.roundCounts[0] = -1;
        for (int r = 0; r < R; r++) out.roundCounts[1 + r] = -2;
    }
    if (out.roundModels && R) std::memset(out.roundModels, 0, (size_t)R * pnp::kModel * sizeof(double));
    if (out.roundsAdopted) *out.roundsAdopted = 0;
    if (out.counts)
        for (int h = 0; h < H; h++) out.counts[h] = -1;
    if (out.models) std::memset(out.models, 0, (size_t)H * pnp::kModel * sizeof(double));
}

// The localisation of M >= 3 matches, on the host (hMatches) or already on the device (dMatches, valid
// until the call returns), in one scoped block; one wait at the end.  Arguments checked by the callers.
int localize_run(fm3d_ctx* c, const double* pts, const double* nrm, int nPts, const fm3d_point2f* kpts, int nKpts,
                 const fm3d_dmatch* hMatches, const fm3d_dmatch* dMatches, int M, const fm3d_localize_opts* o,
                 const LocalizeOut& out) {
    const int H = o->samples * pnp::kSlots, R = o->refineIters;
    const bool normals = nrm != nullptr;
    const fm3d::Camera& cam = c->cam;
    const double tau = o->maxPx * 2.0 / (cam.fx + cam.fy);
    const double tau2 = tau * tau, cos2 = o->minFacingCos * o->minFacingCos;
    hipStream_t st = c->stream;
    HIPCHK(c, hipSetDevice(c->device));
    int nCU = 0;
    HIPCHK(c, hipDeviceGetAttribute(&nCU, hipDeviceAttributeMultiprocessorCount, c->device));
    const int Mpad = fm3d::verify_pad(M);
    const size_t bP = (size_t)nPts * 3 * sizeof(double), bK = (size_t)nKpts * sizeof(fm3d_point2f);
    Carver cv;
    const size_t oP = cv.take(bP), oNr = cv.take(normals ? bP : 0), oK = cv.take(bK);
    const size_t oM = cv.take(hMatches ? (size_t)M * sizeof(fm3d_dmatch) : 0);
    const size_t oPl = cv.take((size_t)fm3d::localize_planes(normals) * Mpad * sizeof(double));
    const size_t oMod = cv.take((size_t)H * pnp::kModel * sizeof(double)), oCnt = cv.take((size_t)H * sizeof(int));
    const size_t oBest = cv.take(sizeof(int)), oCur = cv.take(pnp::kModel * sizeof(double));
    const size_t oFlag = cv.take((size_t)M * sizeof(int)), oMask = cv.take((size_t)M);
    const size_t oOut = cv.take((size_t)(M + 1) * sizeof(fm3d_dmatch)), oN = cv.take(sizeof(int));
    const size_t oTmp = cv.take(fm3d::scan_tmp_bytes(M));
    const size_t oRef = R ? cv.take(fm3d::localize_refine_bytes(M, R)) : 0;
    DevBuf buf;
    HIPCHK(c, buf.ensure(cv.off));
    char* const pool = buf.as<char>();
    HIPCHK(c, hipMemcpyAsync(pool + oP, pts, bP, hipMemcpyHostToDevice, st));
    if (normals) HIPCHK(c, hipMemcpyAsync(pool + oNr, nrm, bP, hipMemcpyHostToDevice, st));
    HIPCHK(c, hipMemcpyAsync(pool + oK, kpts, bK, hipMemcpyHostToDevice, st));
    if (hMatches) {
        HIPCHK(c, hipMemcpyAsync(pool + oM, hMatches, (size_t)M * sizeof(fm3d_dmatch), hipMemcpyHostToDevice, st));
        dMatches = (const fm3d_dmatch*)(pool + oM);
    }
    const fm3d::LocalizeIn in{(const fm3d_point2f*)(pool + oK), (const double*)(pool + oP),
                              normals ? (const double*)(pool + oNr) : nullptr, nKpts, nPts};
    fm3d::launch_localize(cam, in, dMatches, M, o->samples, o->seed, tau2, cos2, nCU, (double*)(pool + oPl),
                          (double*)(pool + oMod), (int*)(pool + oCnt), (int*)(pool + oBest), (double*)(pool + oCur),
                          (int*)(pool + oFlag), (uint8_t*)(pool + oMask), st, R == 0);
    int *dRoundCounts = nullptr, *dAdopted = nullptr;
    double* dRoundModels = nullptr;
    if (R)  // every round queued now: the call keeps its one sync at the end
        fm3d::launch_localize_refine(M, normals, R, tau2, cos2, (const double*)(pool + oPl), (const int*)(pool + oCnt),
                                     (const int*)(pool + oBest), (double*)(pool + oCur), pool + oRef,
                                     (int*)(pool + oFlag), (uint8_t*)(pool + oMask), &dRoundCounts, &dRoundModels,
                                     &dAdopted, st);
    fm3d::launch_compact_dmatch(dMatches, (const int*)(pool + oFlag), M, (fm3d_dmatch*)(pool + oOut), (int*)(pool + oN),
                                pool + oTmp, st);
    HIPCHK(c, hipGetLastError());
    int n = 0;
    double cur[pnp::kModel];
    HIPCHK(c, hipMemcpyAsync(&n, pool + oN, sizeof(int), hipMemcpyDeviceToHost, st));
    HIPCHK(c, hipMemcpyAsync(out.best, pool + oBest, sizeof(int), hipMemcpyDeviceToHost, st));
    HIPCHK(c, hipMemcpyAsync(cur, pool + oCur, sizeof(cur), hipMemcpyDeviceToHost, st));
    HIPCHK(c, hipMemcpyAsync(out.inlierMask, pool + oMask, (size_t)M, hipMemcpyDeviceToHost, st));
    if (out.counts) HIPCHK(c, hipMemcpyAsync(out.counts, pool + oCnt, (size_t)H * sizeof(int), hipMemcpyDeviceToHost, st));
    if (out.models)
        HIPCHK(c, hipMemcpyAsync(out.models, pool + oMod, (size_t)H * pnp::kModel * sizeof(double), hipMemcpyDeviceToHost, st));
    if (R) {
        if (out.roundCounts)
            HIPCHK(c, hipMemcpyAsync(out.roundCounts, dRoundCounts, (size_t)(R + 1) * sizeof(int), hipMemcpyDeviceToHost, st));
        if (out.roundModels)
            HIPCHK(c, hipMemcpyAsync(out.roundModels, dRoundModels, (size_t)R * pnp::kModel * sizeof(double),
                                     hipMemcpyDeviceToHost, st));
        if (out.roundsAdopted) HIPCHK(c, hipMemcpyAsync(out.roundsAdopted, dAdopted, sizeof(int), hipMemcpyDeviceToHost, st));
    }
    HIPCHK(c, hipStreamSynchronize(st));
    if (n < 0 || n > M) return fail(c, FM3D_ERR_HIP, "localize: inlier count out of range");
    if (n) HIPCHK(c, hipMemcpy(out.inliers, pool + oOut, (size_t)n * sizeof(fm3d_dmatch), hipMemcpyDeviceToHost));
    *out.nInliers = n;
    if (*out.best >= 0) {
        for (int r = 0; r < 3; r++) {
            for (int k = 0; k < 3; k++) out.g[r * 4 + k] = cur[r * 3 + k];
            out.g[r * 4 + 3] = cur[9 + r];
        }
        out.g[15] = 1.;
    }
    if (R == 0 && out.roundCounts && *out.best >= 0) out.roundCounts[0] = n;  // c_0: the best model's count
    return FM3D_OK;
}

bool accepts(const double* m, const double* uv, const double* X, const double* nrm, int i, double tau2, double cos2) {
    const double *p = uv + 2 * (size_t)i, *q = X + 3 * (size_t)i;
    if (!nrm) return pnp::inlier(m, p[0], p[1], q[0], q[1], q[2], tau2);
    const double* n = nrm + 3 * (size_t)i;
    return pnp::inlier_n(m, p[0], p[1], q[0], q[1], q[2], n[0], n[1], n[2], tau2, cos2);
}

}  // namespace

extern "C" {

int fm3d_quartic_roots(const double coef[5], double roots[4], int* nRoots) {
    if (!coef || !roots) return FM3D_ERR_INVALID;
    const int n = pnp::quartic_roots(coef[4], coef[3], coef[2], coef[1], coef[0], roots[0], roots[1], roots[2], roots[3]);
    if (nRoots) *nRoots = n < 0 ? 0 : n;
    return n < 0 ? 1 : 0;
}

int fm3d_p3p(const double X[9], const double uv[6], double models[48], int32_t valid[4]) {
    if (!X || !uv || !models) return FM3D_ERR_INVALID;
    double pX[3][3], puv[3][2], m[pnp::kSlots][pnp::kModel];
    bool ok[pnp::kSlots];
    for (int k = 0; k < 3; k++) {
        for (int r = 0; r < 3; r++) pX[k][r] = X[3 * k + r];
        for (int r = 0; r < 2; r++) puv[k][r] = uv[2 * k + r];
    }
    const int n = pnp::p3p(pX, puv, m, ok);
    for (int k = 0; k < pnp::kSlots; k++) {
        for (int e = 0; e < pnp::kModel; e++) models[k * pnp::kModel + e] = m[k][e];
        if (valid) valid[k] = ok[k] ? 1 : 0;
    }
    return n;
}

int fm3d_pnp_count(const double model[12], const double* uv, const double* X, const double* nrm, int n, double tau,
                   double minFacingCos, uint8_t* mask) {
    if (!model || n < 0 || ((!uv || !X) && n)) return FM3D_ERR_INVALID;
    const double tau2 = tau * tau, cos2 = minFacingCos * minFacingCos;
    int cnt = 0;
    for (int i = 0; i < n; i++) {
        const bool in = accepts(model, uv, X, nrm, i, tau2, cos2);
        if (mask) mask[i] = in ? 1 : 0;
        cnt += in;
    }
    return cnt;
}

int fm3d_pnp_step(const double model[12], const double* uv, const double* X, const double* nrm, int n, double tau,
                  double minFacingCos, double out[12], double sums[28]) {
    if (!model || !out || n < 0 || ((!uv || !X) && n)) return FM3D_ERR_INVALID;
    const double tau2 = tau * tau, cos2 = minFacingCos * minFacingCos;
    // the sums in the contract's order: per tile of 1,024 slots the leaves (slot k * 256 + t belongs to
    // leaf t), a balanced tree over the 256 leaves, then the tiles in order from +0.0
    double S[pnp::kSums];
    for (int j = 0; j < pnp::kSums; j++) S[j] = 0.;
    std::vector<double> leaf((size_t)pnp::kSums * pnp::kLanes);
    for (int base = 0; base < n; base += pnp::kTile) {
        for (int t = 0; t < pnp::kLanes; t++) {
            double T[4][pnp::kSums];
            bool in[4];
            for (int k = 0; k < 4; k++) {
                const int i = base + k * pnp::kLanes + t;
                in[k] = i < n && accepts(model, uv, X, nrm, i, tau2, cos2);
                if (in[k]) pnp::terms(model, uv[2 * (size_t)i], uv[2 * (size_t)i + 1], X[3 * (size_t)i], X[3 * (size_t)i + 1],
                                      X[3 * (size_t)i + 2], T[k]);
            }
            for (int j = 0; j < pnp::kSums; j++)
                leaf[(size_t)j * pnp::kLanes + t] =
                    fm3d_epi8::leaf4(in[0] ? T[0][j] : 0., in[1] ? T[1][j] : 0., in[2] ? T[2][j] : 0., in[3] ? T[3][j] : 0.);
        }
        for (int j = 0; j < pnp::kSums; j++) {
            double* l = &leaf[(size_t)j * pnp::kLanes];
            for (int w = pnp::kLanes / 2; w >= 1; w >>= 1)
                for (int i = 0; i < w; i++) l[i] = l[2 * i] + l[2 * i + 1];
            S[j] = S[j] + l[0];
        }
    }
    if (sums)
        for (int k = 0; k < pnp::kSums; k++) sums[k] = S[k];
    return pnp::step_solve(S, model, out) ? 0 : 1;
}

int fm3d_localize_points(fm3d_ctx* c, const double* pts, const double* nrm, int nPts, const fm3d_point2f* kpts, int nKpts,
                         const fm3d_dmatch* matches, int nMatches, const fm3d_localize_opts* o, double g[16],
                         uint8_t* inlierMask, fm3d_dmatch* inliers, int* nInliers, int* best, int32_t* counts,
                         double* models, int32_t* roundCounts, double* roundModels, int* roundsAdopted) {
    const int M = nMatches;
    if (!c || !o || !g || !nInliers || !best || nPts < 0 || nKpts < 0 || M < 0 || (!pts && nPts) || (!kpts && nKpts) ||
        ((!matches || !inlierMask || !inliers) && M))
        return fail(c, FM3D_ERR_INVALID, "null argument");
    if (int r = check_opts(c, o)) return r;
    for (int i = 0; i < M; i++)
        if (matches[i].queryIdx < 0 || matches[i].queryIdx >= nKpts || matches[i].trainIdx < 0 || matches[i].trainIdx >= nPts)
            return fail(c, FM3D_ERR_INVALID, "match index out of range");
    const LocalizeOut out{g, inlierMask, inliers, nInliers, best, counts, models, roundCounts, roundModels, roundsAdopted};
    clear_outputs(out, M, o->samples * pnp::kSlots, o->refineIters);
    if (M < 3) return FM3D_OK;  // no sample exists: every hypothesis is invalid
    return localize_run(c, pts, nrm, nPts, kpts, nKpts, matches, nullptr, M, o, out);
}

int fm3d_localize_model(fm3d_ctx* c, const void* descImg, const fm3d_point2f* kpts, int nKpts, const void* descModel,
                        const double* pts, const double* nrm, int nPts, int dim, int type, double epsilon,
                        const fm3d_localize_opts* o, fm3d_dmatch* matches, int* nMatches, double g[16],
                        uint8_t* inlierMask, fm3d_dmatch* inliers, int* nInliers, int* best, int32_t* counts,
                        double* models, int32_t* roundCounts, double* roundModels, int* roundsAdopted) {
    if (!c || !o || !g || !nMatches || !nInliers || !best || nKpts < 0 || nPts < 0 || (!descImg && nKpts) ||
        (!descModel && nPts) || (!kpts && nKpts) || (!pts && nPts) || ((!matches || !inlierMask || !inliers) && nKpts))
        return fail(c, FM3D_ERR_INVALID, "null argument");
    int r;
    if ((r = check_opts(c, o))) return r;
    hipSetDevice(c->device);
    // the matcher with the compaction fused into the NNDR launch, as the pipeline's front half runs it
    int t, dp;
    if ((r = stage_descriptors(c, descImg, nKpts, descModel, nPts, dim, type, &t, &dp))) return r;
    if ((r = ensure_scan_tmp(c, nKpts))) return r;
    HIPCHK(c, c->matches.ensure((size_t)(nKpts + 1) * sizeof(fm3d_dmatch)));
    MatchOpts mo;
    mo.eps = epsilon;
    mo.compactOut = c->matches.as<fm3d_dmatch>();
    mo.compactCount = c->count.as<int>();
    mo.crossCheck = c->s.crossCheck;
    if ((r = run_match(c, nKpts, nPts, t, dp, mo))) return r;
    int M = 0;  // the one wait: the launches behind it are sized by the count
    HIPCHK(c, hipMemcpyAsync(&M, c->count.p, sizeof(int), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    if (M < 0 || M > nKpts) return fail(c, FM3D_ERR_HIP, "match count out of range");
    *nMatches = M;
    const LocalizeOut out{g, inlierMask, inliers, nInliers, best, counts, models, roundCounts, roundModels, roundsAdopted};
    clear_outputs(out, M, o->samples * pnp::kSlots, o->refineIters);
    if (M) HIPCHK(c, hipMemcpyAsync(matches, c->matches.p, (size_t)M * sizeof(fm3d_dmatch), hipMemcpyDeviceToHost, c->stream));
    if (M < 3) {
        HIPCHK(c, hipStreamSynchronize(c->stream));
        return FM3D_OK;
    }
    r = localize_run(c, pts, nrm, nPts, kpts, nKpts, nullptr, c->matches.as<fm3d_dmatch>(), M, o, out);
    if (r) hipStreamSynchronize(c->stream);  // the copy of the matches above names the caller's memory
    return r;
}

}  // extern "C"
