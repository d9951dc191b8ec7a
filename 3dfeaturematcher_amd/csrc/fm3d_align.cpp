// fm3d_align.cpp -- 3D-3D alignment, the host side: fm3d_align_points'
// orchestration, the matcher in front of it (fm3d_match_models) and the context-free algebra (sampler,
// three-point model, count, refit).  The arithmetic is include/fm3d_rigid3.h's; the kernels are
// fm3d_align.hip's.
#include <hip/hip_runtime.h>

#include <cfloat>
#include <cmath>
#include <cstring>
#include <string>
#include <vector>

#include "fm3d.h"
#include "fm3d_ctx.h"
#include "fm3d_kernels.h"
#include "fm3d_rigid3.h"

using namespace fm3d_host;
namespace r3 = fm3d_rigid3;

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

// the caller's optional and required outputs of one alignment
struct AlignOut {
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

// the rules of fm3d_align_opts, before any launch
int check_opts(fm3d_ctx* c, const fm3d_align_opts* o) {
    if (o->hypotheses < 1) return fail(c, FM3D_ERR_INVALID, "hypotheses must be >= 1");
    if (!(o->maxDist > 0. && o->maxDist <= DBL_MAX)) return fail(c, FM3D_ERR_INVALID, "maxDist must be finite and > 0");
    if (!(o->minNormalCos >= -1. && o->minNormalCos <= 1.))
        return fail(c, FM3D_ERR_INVALID, "minNormalCos must be in -1 .. 1");
    if (o->refineIters < 0 || o->refineIters > r3::kMaxIters)
        return fail(c, FM3D_ERR_INVALID, "refineIters must be in 0 .. 16");
    if (o->hypotheses > fm3d::kVerifyMaxHyps) return fail(c, FM3D_ERR_UNSUPPORTED, "more than 2^20 hypotheses");
    return FM3D_OK;
}

// what the outputs hold until a model exists
void clear_outputs(const AlignOut& out, int M, int H, int R) {
    for (int k = 0; k < 16; k++) out.g[k] = 0.;
    *out.nInliers = 0;
    *out.best = -1;
    if (M) std::memset(out.inlierMask, 0, (size_t)M);
    // until a round runs: no best model gives c_0 = -1, and every round -2 and a zero candidate
    if (out.roundCounts) {
        out.roundCounts[0] = -1;
        for (int r = 0; r < R; r++) out.roundCounts[1 + r] = -2;
    }
    if (out.roundModels && R) std::memset(out.roundModels, 0, (size_t)R * r3::kModel * sizeof(double));
    if (out.roundsAdopted) *out.roundsAdopted = 0;
    if (out.counts)
        for (int h = 0; h < H; h++) out.counts[h] = -1;
    if (out.models) std::memset(out.models, 0, (size_t)H * r3::kModel * sizeof(double));
}

// The alignment of M >= 3 matches, on the host (hMatches) or already on the device (dMatches, valid
// until the call returns), in one scoped block; one wait at the end.  Arguments checked by the callers.
int align_run(fm3d_ctx* c, const double* ptsA, const double* nrmA, int nA, const double* ptsB, const double* nrmB,
              int nB, const fm3d_dmatch* hMatches, const fm3d_dmatch* dMatches, int M, const fm3d_align_opts* o,
              const AlignOut& out) {
    const int H = o->hypotheses, R = o->refineIters;
    const bool nrm = nrmA != nullptr;
    const double tau2 = o->maxDist * o->maxDist, minCos = o->minNormalCos;
    hipStream_t st = c->stream;
    HIPCHK(c, hipSetDevice(c->device));
    int nCU = 0;
    HIPCHK(c, hipDeviceGetAttribute(&nCU, hipDeviceAttributeMultiprocessorCount, c->device));
    const int Mpad = fm3d::verify_pad(M);
    const size_t bA = (size_t)nA * 3 * sizeof(double), bB = (size_t)nB * 3 * sizeof(double);
    Carver cv;
    const size_t oPA = cv.take(bA), oPB = cv.take(bB), oNA = cv.take(nrm ? bA : 0), oNB = cv.take(nrm ? bB : 0);
    const size_t oM = cv.take(hMatches ? (size_t)M * sizeof(fm3d_dmatch) : 0);
    const size_t oPl = cv.take((size_t)fm3d::align_planes(nrm) * Mpad * sizeof(double));
    const size_t oMod = cv.take((size_t)H * r3::kModel * sizeof(double)), oCnt = cv.take((size_t)H * sizeof(int));
    const size_t oBest = cv.take(sizeof(int)), oCur = cv.take(r3::kModel * sizeof(double));
    const size_t oFlag = cv.take((size_t)M * sizeof(int)), oMask = cv.take((size_t)M);
    const size_t oOut = cv.take((size_t)(M + 1) * sizeof(fm3d_dmatch)), oN = cv.take(sizeof(int));
    const size_t oTmp = cv.take(fm3d::scan_tmp_bytes(M));
    const size_t oRef = R ? cv.take(fm3d::align_refine_bytes(M, R)) : 0;
    DevBuf buf;
    HIPCHK(c, buf.ensure(cv.off));
    char* const pool = buf.as<char>();
    HIPCHK(c, hipMemcpyAsync(pool + oPA, ptsA, bA, hipMemcpyHostToDevice, st));
    HIPCHK(c, hipMemcpyAsync(pool + oPB, ptsB, bB, hipMemcpyHostToDevice, st));
    if (nrm) {
        HIPCHK(c, hipMemcpyAsync(pool + oNA, nrmA, bA, hipMemcpyHostToDevice, st));
        HIPCHK(c, hipMemcpyAsync(pool + oNB, nrmB, bB, hipMemcpyHostToDevice, st));
    }
    if (hMatches) {
        HIPCHK(c, hipMemcpyAsync(pool + oM, hMatches, (size_t)M * sizeof(fm3d_dmatch), hipMemcpyHostToDevice, st));
        dMatches = (const fm3d_dmatch*)(pool + oM);
    }
    const fm3d::AlignIn in{(const double*)(pool + oPA), nrm ? (const double*)(pool + oNA) : nullptr,
                           (const double*)(pool + oPB), nrm ? (const double*)(pool + oNB) : nullptr, nA, nB};
    fm3d::launch_align(in, dMatches, M, H, o->seed, tau2, minCos, nCU, (double*)(pool + oPl), (double*)(pool + oMod),
                       (int*)(pool + oCnt), (int*)(pool + oBest), (double*)(pool + oCur), (int*)(pool + oFlag),
                       (uint8_t*)(pool + oMask), st, R == 0);
    int *dRoundCounts = nullptr, *dAdopted = nullptr;
    double* dRoundModels = nullptr;
    if (R)  // every round queued now: the call keeps its one sync at the end
        fm3d::launch_align_refine(M, nrm, R, tau2, minCos, (const double*)(pool + oPl), (const int*)(pool + oCnt),
                                  (const int*)(pool + oBest), (double*)(pool + oCur), pool + oRef, (int*)(pool + oFlag),
                                  (uint8_t*)(pool + oMask), &dRoundCounts, &dRoundModels, &dAdopted, st);
    fm3d::launch_compact_dmatch(dMatches, (const int*)(pool + oFlag), M, (fm3d_dmatch*)(pool + oOut), (int*)(pool + oN),
                                pool + oTmp, st);
    HIPCHK(c, hipGetLastError());
    int n = 0;
    double cur[r3::kModel];
    HIPCHK(c, hipMemcpyAsync(&n, pool + oN, sizeof(int), hipMemcpyDeviceToHost, st));
    HIPCHK(c, hipMemcpyAsync(out.best, pool + oBest, sizeof(int), hipMemcpyDeviceToHost, st));
    HIPCHK(c, hipMemcpyAsync(cur, pool + oCur, sizeof(cur), hipMemcpyDeviceToHost, st));
    HIPCHK(c, hipMemcpyAsync(out.inlierMask, pool + oMask, (size_t)M, hipMemcpyDeviceToHost, st));
    if (out.counts) HIPCHK(c, hipMemcpyAsync(out.counts, pool + oCnt, (size_t)H * sizeof(int), hipMemcpyDeviceToHost, st));
    if (out.models)
        HIPCHK(c, hipMemcpyAsync(out.models, pool + oMod, (size_t)H * r3::kModel * sizeof(double), hipMemcpyDeviceToHost, st));
    if (R) {
        if (out.roundCounts)
            HIPCHK(c, hipMemcpyAsync(out.roundCounts, dRoundCounts, (size_t)(R + 1) * sizeof(int), hipMemcpyDeviceToHost, st));
        if (out.roundModels)
            HIPCHK(c, hipMemcpyAsync(out.roundModels, dRoundModels, (size_t)R * r3::kModel * sizeof(double),
                                     hipMemcpyDeviceToHost, st));
        if (out.roundsAdopted) HIPCHK(c, hipMemcpyAsync(out.roundsAdopted, dAdopted, sizeof(int), hipMemcpyDeviceToHost, st));
    }
    HIPCHK(c, hipStreamSynchronize(st));
    if (n < 0 || n > M) return fail(c, FM3D_ERR_HIP, "align: inlier count out of range");
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

// the sums of one pass over the pairs `in` marks, in the contract's order: per tile of 1,024 slots the
// leaves (slot k * 256 + t belongs to leaf t), a balanced tree over the 256 leaves, then the tiles in
// order from +0.0.  value(i, j): pair i's term of sum j.
template <int J, typename F>
void tiled_sums(int n, const std::vector<uint8_t>& in, F value, double (&S)[J]) {
    for (int j = 0; j < J; j++) S[j] = 0.;
    double leaf[r3::kLanes];
    for (int base = 0; base < n; base += r3::kTile)
        for (int j = 0; j < J; j++) {
            for (int t = 0; t < r3::kLanes; t++) {
                double v[4];
                for (int k = 0; k < 4; k++) {
                    const int i = base + k * r3::kLanes + t;
                    v[k] = i < n && in[i] ? value(i, j) : 0.;
                }
                leaf[t] = fm3d_epi8::leaf4(v[0], v[1], v[2], v[3]);
            }
            for (int w = r3::kLanes / 2; w >= 1; w >>= 1)
                for (int i = 0; i < w; i++) leaf[i] = leaf[2 * i] + leaf[2 * i + 1];
            S[j] = S[j] + leaf[0];
        }
}

bool accepts(const double* m, const double* a, const double* b, const double* na, const double* nb, int i, double tau2,
             double minCos) {
    const double *p = a + 3 * (size_t)i, *q = b + 3 * (size_t)i;
    if (!na) return r3::inlier(m, p[0], p[1], p[2], q[0], q[1], q[2], tau2);
    const double *u = na + 3 * (size_t)i, *v = nb + 3 * (size_t)i;
    return r3::inlier_n(m, p[0], p[1], p[2], q[0], q[1], q[2], u[0], u[1], u[2], v[0], v[1], v[2], tau2, minCos);
}

}  // namespace

extern "C" {

int fm3d_ransac_sample3(uint64_t seed, int h, int M, int32_t idx[3]) {
    if (!idx || h < 0 || M < 0) return FM3D_ERR_INVALID;
    int s[3];
    const bool ok = r3::sample3(seed, (uint32_t)h, (uint32_t)M, s);
    for (int k = 0; k < 3; k++) idx[k] = s[k];
    return ok ? 0 : 1;
}

int fm3d_rigid_from3(const double a[9], const double b[9], double model[12]) {
    if (!a || !b || !model) return FM3D_ERR_INVALID;
    double pa[3][3], pb[3][3];
    for (int k = 0; k < 3; k++)
        for (int r = 0; r < 3; r++) {
            pa[k][r] = a[3 * k + r];
            pb[k][r] = b[3 * k + r];
        }
    return r3::rigid_from3(pa, pb, model) ? 0 : 1;
}

int fm3d_rigid_count(const double model[12], const double* a, const double* b, const double* na, const double* nb,
                     int n, double maxDist, double minNormalCos, uint8_t* mask) {
    if (!model || n < 0 || ((!a || !b) && n) || (na == nullptr) != (nb == nullptr)) return FM3D_ERR_INVALID;
    const double tau2 = maxDist * maxDist;
    int cnt = 0;
    for (int i = 0; i < n; i++) {
        const bool in = accepts(model, a, b, na, nb, i, tau2, minNormalCos);
        if (mask) mask[i] = in ? 1 : 0;
        cnt += in;
    }
    return cnt;
}

int fm3d_rigid_refit(const double model[12], const double* a, const double* b, const double* na, const double* nb,
                     int n, double maxDist, double minNormalCos, double out[12], double sums[16]) {
    if (!model || !out || n < 0 || ((!a || !b) && n) || (na == nullptr) != (nb == nullptr)) return FM3D_ERR_INVALID;
    const double tau2 = maxDist * maxDist;
    std::vector<uint8_t> in((size_t)n);
    for (int i = 0; i < n; i++) in[i] = accepts(model, a, b, na, nb, i, tau2, minNormalCos) ? 1 : 0;
    double S1[r3::kSums1], S2[r3::kSums2], ca[3], cb[3];
    tiled_sums(n, in, [&](int i, int j) { return j < 3 ? a[3 * (size_t)i + j] : j < 6 ? b[3 * (size_t)i + j - 3] : 1.; }, S1);
    r3::centroids(S1, ca, cb);
    tiled_sums(n, in, [&](int i, int j) { return r3::slot2(true, a[3 * (size_t)i + j / 3], ca[j / 3], b[3 * (size_t)i + j % 3], cb[j % 3]); },
               S2);
    if (sums) {
        for (int k = 0; k < r3::kSums1; k++) sums[k] = S1[k];
        for (int k = 0; k < r3::kSums2; k++) sums[r3::kSums1 + k] = S2[k];
    }
    return r3::refit_solve(S1, S2, out) ? 0 : 1;
}

int fm3d_align_points(fm3d_ctx* c, const double* ptsA, const double* nrmA, int nA, const double* ptsB,
                      const double* nrmB, int nB, const fm3d_dmatch* matches, int nMatches, const fm3d_align_opts* o,
                      double g[16], uint8_t* inlierMask, fm3d_dmatch* inliers, int* nInliers, int* best,
                      int32_t* counts, double* models, int32_t* roundCounts, double* roundModels, int* roundsAdopted) {
    const int M = nMatches;
    if (!c || !o || !g || !nInliers || !best || nA < 0 || nB < 0 || M < 0 || (!ptsA && nA) || (!ptsB && nB) ||
        ((!matches || !inlierMask || !inliers) && M))
        return fail(c, FM3D_ERR_INVALID, "null argument");
    if ((nrmA == nullptr) != (nrmB == nullptr)) return fail(c, FM3D_ERR_INVALID, "normals: both arrays or neither");
    if (int r = check_opts(c, o)) return r;
    for (int i = 0; i < M; i++)
        if (matches[i].queryIdx < 0 || matches[i].queryIdx >= nA || matches[i].trainIdx < 0 || matches[i].trainIdx >= nB)
            return fail(c, FM3D_ERR_INVALID, "match index out of range");
    const AlignOut out{g, inlierMask, inliers, nInliers, best, counts, models, roundCounts, roundModels, roundsAdopted};
    clear_outputs(out, M, o->hypotheses, o->refineIters);
    if (M < 3) return FM3D_OK;  // no sample exists: every hypothesis is invalid
    return align_run(c, ptsA, nrmA, nA, ptsB, nrmB, nB, matches, nullptr, M, o, out);
}

int fm3d_match_models(fm3d_ctx* c, const void* descA, const double* ptsA, const double* nrmA, int nA, const void* descB,
                      const double* ptsB, const double* nrmB, int nB, int dim, int type, double epsilon,
                      const fm3d_align_opts* o, fm3d_dmatch* matches, int* nMatches, double g[16], uint8_t* inlierMask,
                      fm3d_dmatch* inliers, int* nInliers, int* best, int32_t* counts, double* models,
                      int32_t* roundCounts, double* roundModels, int* roundsAdopted) {
    if (!c || !o || !g || !nMatches || !nInliers || !best || nA < 0 || nB < 0 || (!descA && nA) || (!descB && nB) ||
        (!ptsA && nA) || (!ptsB && nB) || ((!matches || !inlierMask || !inliers) && nA))
        return fail(c, FM3D_ERR_INVALID, "null argument");
    if ((nrmA == nullptr) != (nrmB == nullptr)) return fail(c, FM3D_ERR_INVALID, "normals: both arrays or neither");
    int r;
    if ((r = check_opts(c, o))) return r;
    hipSetDevice(c->device);
    // the matcher with the compaction fused into the NNDR launch, as the pipeline's front half runs it
    int t, dp;
    if ((r = stage_descriptors(c, descA, nA, descB, nB, dim, type, &t, &dp))) return r;
    if ((r = ensure_scan_tmp(c, nA))) return r;
    HIPCHK(c, c->matches.ensure((size_t)(nA + 1) * sizeof(fm3d_dmatch)));
    MatchOpts mo;
    mo.eps = epsilon;
    mo.compactOut = c->matches.as<fm3d_dmatch>();
    mo.compactCount = c->count.as<int>();
    mo.crossCheck = c->s.crossCheck;
    if ((r = run_match(c, nA, nB, t, dp, mo))) return r;
    int M = 0;  // the one wait: the launches behind it are sized by the count
    HIPCHK(c, hipMemcpyAsync(&M, c->count.p, sizeof(int), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    if (M < 0 || M > nA) return fail(c, FM3D_ERR_HIP, "match count out of range");
    *nMatches = M;
    const AlignOut out{g, inlierMask, inliers, nInliers, best, counts, models, roundCounts, roundModels, roundsAdopted};
    clear_outputs(out, M, o->hypotheses, o->refineIters);
    if (M) HIPCHK(c, hipMemcpyAsync(matches, c->matches.p, (size_t)M * sizeof(fm3d_dmatch), hipMemcpyDeviceToHost, c->stream));
    if (M < 3) {
        HIPCHK(c, hipStreamSynchronize(c->stream));
        return FM3D_OK;
    }
    r = align_run(c, ptsA, nrmA, nA, ptsB, nrmB, nB, nullptr, c->matches.as<fm3d_dmatch>(), M, o, out);
    if (r) hipStreamSynchronize(c->stream);  // the copy of the matches above names the caller's memory
    return r;
}

}  // extern "C"
