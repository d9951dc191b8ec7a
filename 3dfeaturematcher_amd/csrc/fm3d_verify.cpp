// fm3d_verify.cpp -- geometric verification, the host side: fm3d_verify_matches'
// orchestration (with the refinement rounds of fm3d_verify_matches_refined), the same stage on a staged
// pipeline pair (verify_staged, for fm3d_pipeline_run(_dlt)_verified in fm3d_pipeline.cpp) and the
// context-free algebra (sampler, eight-point model, count, normal matrix and refit, pose from E).
// The arithmetic is include/fm3d_epi8.h's; the kernels are fm3d_verify.hip's.
#include <hip/hip_runtime.h>

#include <cfloat>
#include <cmath>
#include <cstring>
#include <string>
#include <vector>

#include "fm3d.h"
#include "fm3d_ctx.h"
#include "fm3d_epi8.h"
#include "fm3d_kernels.h"

using namespace fm3d_host;

namespace {

// one block carved in 256-byte steps: a local one per fm3d_verify_matches call, the context's for a staged pair
struct Carver {
    size_t off = 0;
    size_t take(size_t bytes) {
        const size_t at = off;
        off += (bytes + 255) & ~(size_t)255;
        return at;
    }
};

}  // namespace

int fm3d_ransac_sample(uint64_t seed, int h, int M, int32_t idx[8]) {
    if (!idx || h < 0 || M < 0) return FM3D_ERR_INVALID;
    int s[8];
    const bool ok = fm3d_epi8::sample8(seed, (uint32_t)h, (uint32_t)M, s);
    for (int k = 0; k < 8; k++) idx[k] = s[k];
    return ok ? 0 : 1;
}

int fm3d_epipolar_from8(const double x1[16], const double x2[16], double E[9]) {
    if (!x1 || !x2 || !E) return FM3D_ERR_INVALID;
    fm3d_epi8::Mat89 A;
    for (int k = 0; k < 8; k++) fm3d_epi8::set_row(A, k, x1[2 * k], x1[2 * k + 1], x2[2 * k], x2[2 * k + 1]);
    double e[9];
    return fm3d_epi8::model8(A, E, e) ? 0 : 1;
}

int fm3d_epipolar_null8(const double x1[16], const double x2[16], double e[9]) {
    if (!x1 || !x2 || !e) return FM3D_ERR_INVALID;
    fm3d_epi8::Mat89 A;
    for (int k = 0; k < 8; k++) fm3d_epi8::set_row(A, k, x1[2 * k], x1[2 * k + 1], x2[2 * k], x2[2 * k + 1]);
    if (fm3d_epi8::null8(A, e)) return 0;
    for (int k = 0; k < 9; k++) e[k] = 0.;
    return 1;
}

int fm3d_epipolar_count(const double E[9], const double* x1, const double* x2, int n, double tau, uint8_t* mask) {
    if (!E || n < 0 || ((!x1 || !x2) && n)) return FM3D_ERR_INVALID;
    const double tau2 = tau * tau;
    int cnt = 0;
    for (int i = 0; i < n; i++) {
        const bool in = fm3d_epi8::inlier(E, x1[2 * i], x1[2 * i + 1], x2[2 * i], x2[2 * i + 1], tau2);
        if (mask) mask[i] = in ? 1 : 0;
        cnt += in;
    }
    return cnt;
}

int fm3d_pose_from_epipolar(const double E[9], const double* x1, const double* x2, int n, double baseline,
                            double g12[16], int32_t votes[4]) {
    if (!E || !g12 || n < 0 || ((!x1 || !x2) && n)) return FM3D_ERR_INVALID;
    double R[2][9], u2[3];
    if (!fm3d_epi8::pose_candidates(E, R, u2)) return 1;
    int vt[4] = {0, 0, 0, 0};
    for (int k = 0; k < 4; k++) {
        double t[3];
        fm3d_epi8::pose_direction(k, u2, t);
        for (int i = 0; i < n; i++)
            vt[k] += fm3d_epi8::pose_vote(R[k >> 1], t, x1[2 * i], x1[2 * i + 1], x2[2 * i], x2[2 * i + 1]) ? 1 : 0;
    }
    fm3d_epi8::pose_g12(fm3d_epi8::pose_pick(vt), R, u2, baseline, g12);
    if (votes)
        for (int k = 0; k < 4; k++) votes[k] = vt[k];
    return 0;
}

// The 45 sums of a_i a_i^T over the pairs E accepts, in the contract's order: per tile of 1,024 slots
// the leaves (slot k * 256 + t belongs to leaf t), a balanced tree over the 256 leaves, then the tiles
// in order from +0.0.  Returns the number of pairs in.
static int normal45(const double E[9], const double* x1, const double* x2, int n, double tau2, double N45[45]) {
    using namespace fm3d_epi8;
    for (int j = 0; j < kPairs; j++) N45[j] = 0.;
    std::vector<double> a((size_t)kRefitTile * 9);
    std::vector<uint8_t> in(kRefitTile);
    double leaf[kRefitLanes];
    int cnt = 0;
    for (int base = 0; base < n; base += kRefitTile) {
        for (int s = 0; s < kRefitTile; s++) {
            const int i = base + s;
            double r[9] = {0., 0., 0., 0., 0., 0., 0., 0., 0.};
            in[s] = 0;
            if (i < n) {
                in[s] = inlier(E, x1[2 * i], x1[2 * i + 1], x2[2 * i], x2[2 * i + 1], tau2) ? 1 : 0;
                row9(x1[2 * i], x1[2 * i + 1], x2[2 * i], x2[2 * i + 1], r);
            }
            cnt += in[s];
            for (int k = 0; k < 9; k++) a[(size_t)s * 9 + k] = r[k];
        }
        int j = 0;
        for (int r = 0; r < 9; r++)
            for (int c = r; c < 9; c++, j++) {
                for (int t = 0; t < kRefitLanes; t++) {
                    double v[4];
                    for (int k = 0; k < 4; k++) {
                        const int s = k * kRefitLanes + t;
                        const double(&as)[9] = *reinterpret_cast<const double(*)[9]>(&a[(size_t)s * 9]);
                        v[k] = slot(in[s] != 0, as, r, c);
                    }
                    leaf[t] = leaf4(v[0], v[1], v[2], v[3]);
                }
                for (int w = kRefitLanes / 2; w >= 1; w >>= 1)
                    for (int i = 0; i < w; i++) leaf[i] = leaf[2 * i] + leaf[2 * i + 1];
                N45[j] = N45[j] + leaf[0];
            }
    }
    return cnt;
}

int fm3d_epipolar_normal45(const double E[9], const double* x1, const double* x2, int n, double tau, double N45[45]) {
    if (!E || !N45 || n < 0 || ((!x1 || !x2) && n)) return FM3D_ERR_INVALID;
    return normal45(E, x1, x2, n, tau * tau, N45);
}

int fm3d_epipolar_refit(const double E[9], const double* x1, const double* x2, int n, double tau, double Eout[9]) {
    if (!E || !Eout || n < 0 || ((!x1 || !x2) && n)) return FM3D_ERR_INVALID;
    double N45[45];
    normal45(E, x1, x2, n, tau * tau, N45);
    fm3d_epi8::Mat99 S, V;
    return fm3d_epi8::refit45(N45, S, V, Eout) ? 0 : 1;
}

int fm3d_host::verify_staged(fm3d_ctx* c, const fm3d_verify_opts* o, int K, fm3d_verify_report* rep, bool* havePose,
                             double g12[16]) {
    const int M = K, H = o->hypotheses, R = o->refineIters;
    const bool pose = o->poseFromModel != 0;
    const fm3d::Camera& cam = c->cam;
    const double tau = o->maxPx * 2.0 / (cam.fx + cam.fy);
    const double tau2 = tau * tau;
    hipStream_t st = c->stream;
    *havePose = false;
    // fm3d_verify_matches_refined's carving, without the inputs: they are the context's
    const int Mpad = fm3d::verify_pad(M);
    Carver cv;
    const size_t oXY = cv.take((size_t)4 * Mpad * sizeof(double));
    const size_t oMod = cv.take((size_t)H * 9 * sizeof(double)), oCnt = cv.take((size_t)H * sizeof(int));
    const size_t oBest = cv.take(sizeof(int)), oE = cv.take(9 * sizeof(double));
    const size_t oFlag = cv.take((size_t)M * sizeof(int)), oMask = cv.take((size_t)M);
    const size_t oRef = R ? cv.take(fm3d::verify_refine_bytes(M, R)) : 0;
    const size_t oPose = cv.take(fm3d::verify_pose_bytes());
    HIPCHK(c, c->verWork.ensure(cv.off));
    HIPCHK(c, c->verMatches.ensure((size_t)(c->pipe.nA + 1) * sizeof(fm3d_dmatch)));
    char* const pool = c->verWork.as<char>();
    int* const cnt = c->pcnt.as<int>();
    HIPCHK(c, hipEventRecord(c->ev[EV_VERIFY_START], st));
    fm3d::launch_verify(cam, c->kp1.as<fm3d_point2f>(), c->kp2.as<fm3d_point2f>(), c->matches.as<fm3d_dmatch>(), M, H,
                        o->seed, tau2, c->nCU, (double*)(pool + oXY), (double*)(pool + oMod), (int*)(pool + oCnt),
                        (int*)(pool + oBest), (double*)(pool + oE), (int*)(pool + oFlag), (uint8_t*)(pool + oMask), st,
                        R == 0);
    int *dRoundCounts = nullptr, *dAdopted = nullptr;
    double* dRoundModels = nullptr;
    if (R)
        fm3d::launch_verify_refine(M, R, tau2, (const double*)(pool + oXY), (const int*)(pool + oCnt),
                                   (const int*)(pool + oBest), (double*)(pool + oE), pool + oRef, (int*)(pool + oFlag),
                                   (uint8_t*)(pool + oMask), &dRoundCounts, &dRoundModels, &dAdopted, st);
    // the verified matches and their count where the DLT reads them (c->scanTmp holds stNA >= M items)
    fm3d::launch_compact_dmatch(c->matches.as<fm3d_dmatch>(), (const int*)(pool + oFlag), M,
                                c->verMatches.as<fm3d_dmatch>(), cnt + 0, c->scanTmp.p, st);
    double* dCand = nullptr;
    int *dValid = nullptr, *dVotes = nullptr;
    if (pose)
        fm3d::launch_verify_pose(M, (const double*)(pool + oXY), (const int*)(pool + oFlag), (const int*)(pool + oBest),
                                 (const double*)(pool + oE), pool + oPose, &dCand, &dValid, &dVotes, st);
    HIPCHK(c, hipGetLastError());
    HIPCHK(c, hipEventRecord(c->ev[EV_VERIFY_END], st));
    std::swap(c->matches, c->verMatches);
    struct {
        double cand[fm3d_epi8::kPoseDoubles];
        int32_t pv[8];
    } hp{};
    static_assert(sizeof(hp) == fm3d_epi8::kPoseDoubles * sizeof(double) + 8 * sizeof(int), "the pose block's layout");
    int n = 0, best = -1, adopted = 0;
    HIPCHK(c, hipMemcpyAsync(&n, cnt + 0, sizeof(int), hipMemcpyDeviceToHost, st));
    HIPCHK(c, hipMemcpyAsync(&best, pool + oBest, sizeof(int), hipMemcpyDeviceToHost, st));
    HIPCHK(c, hipMemcpyAsync(rep->E, pool + oE, 9 * sizeof(double), hipMemcpyDeviceToHost, st));
    if (R) HIPCHK(c, hipMemcpyAsync(&adopted, dAdopted, sizeof(int), hipMemcpyDeviceToHost, st));
    if (pose) HIPCHK(c, hipMemcpyAsync(&hp, pool + oPose, sizeof(hp), hipMemcpyDeviceToHost, st));
    HIPCHK(c, hipStreamSynchronize(st));
    if (n < 0 || n > M) return fail(c, FM3D_ERR_HIP, "verify: inlier count out of range");
    float ms = 0;
    hipEventElapsedTime(&ms, c->ev[EV_VERIFY_START], c->ev[EV_VERIFY_END]);
    rep->verify_ms = ms;
    rep->best = best;
    rep->verified = best >= 0 ? n : 0;
    rep->roundsAdopted = adopted;
    if (pose && best >= 0 && hp.pv[0]) {
        double Rc[2][9], u2[3];
        std::memcpy(Rc, hp.cand, sizeof(Rc));
        std::memcpy(u2, hp.cand + 18, sizeof(u2));
        for (int k = 0; k < 4; k++) rep->votes[k] = hp.pv[1 + k];
        fm3d_epi8::pose_g12(fm3d_epi8::pose_pick(hp.pv + 1), Rc, u2, o->baseline, g12);
        *havePose = true;
    }
    return FM3D_OK;
}

int fm3d_host::verify_staged_queue(fm3d_ctx* c, const fm3d_verify_opts* o) {
    const int Mcap = c->pipe.nA > 0 ? c->pipe.nA : 1, H = o->hypotheses, R = o->refineIters;
    const fm3d::Camera& cam = c->cam;
    const double tau = o->maxPx * 2.0 / (cam.fx + cam.fy);
    const double tau2 = tau * tau;
    hipStream_t st = c->stream;
    // verify_staged's carving by the bound, and the match count's own word: the compaction reads it while
    // it writes c->pcnt[0]
    const int Mpad = fm3d::verify_pad(Mcap);
    Carver cv;
    const size_t oK = cv.take(sizeof(int)), oXY = cv.take((size_t)4 * Mpad * sizeof(double));
    const size_t oMod = cv.take((size_t)H * 9 * sizeof(double)), oCnt = cv.take((size_t)H * sizeof(int));
    const size_t oBest = cv.take(sizeof(int)), oE = cv.take(9 * sizeof(double));
    const size_t oFlag = cv.take((size_t)Mcap * sizeof(int)), oMask = cv.take((size_t)Mcap);
    const size_t oRef = R ? cv.take(fm3d::verify_refine_bytes(Mcap, R)) : 0;
    HIPCHK(c, c->verWork.ensure(cv.off));
    HIPCHK(c, c->verMatches.ensure((size_t)(c->pipe.nA + 1) * sizeof(fm3d_dmatch)));
    HIPCHK(c, c->hVer.ensure(sizeof(fm3d::VerifySmall)));
    fm3d::VerifySmall* hv = c->hVer.as<fm3d::VerifySmall>();
    *hv = fm3d::VerifySmall{-1, -1, -1, 0, {0., 0., 0., 0., 0., 0., 0., 0., 0.}};  // until the kernel's stores arrive
    void* dhv = nullptr;
    HIPCHK(c, hipHostGetDevicePointer(&dhv, hv, 0));
    char* const pool = c->verWork.as<char>();
    int* const cnt = c->pcnt.as<int>();
    const int* const Mdev = (const int*)(pool + oK);
    HIPCHK(c, hipEventRecord(c->ev[EV_VERIFY_START], st));
    HIPCHK(c, hipMemcpyAsync(pool + oK, cnt + 0, sizeof(int), hipMemcpyDeviceToDevice, st));
    fm3d::launch_verify(cam, c->kp1.as<fm3d_point2f>(), c->kp2.as<fm3d_point2f>(), c->matches.as<fm3d_dmatch>(), Mcap,
                        H, o->seed, tau2, c->nCU, (double*)(pool + oXY), (double*)(pool + oMod), (int*)(pool + oCnt),
                        (int*)(pool + oBest), (double*)(pool + oE), (int*)(pool + oFlag), (uint8_t*)(pool + oMask), st,
                        R == 0, Mdev);
    int *dRoundCounts = nullptr, *dAdopted = nullptr;
    double* dRoundModels = nullptr;
    if (R)
        fm3d::launch_verify_refine(Mcap, R, tau2, (const double*)(pool + oXY), (const int*)(pool + oCnt),
                                   (const int*)(pool + oBest), (double*)(pool + oE), pool + oRef, (int*)(pool + oFlag),
                                   (uint8_t*)(pool + oMask), &dRoundCounts, &dRoundModels, &dAdopted, st, Mdev);
    // the verified matches and their count where the DLT reads them (c->scanTmp holds stNA >= Mcap items)
    fm3d::launch_compact_dmatch(c->matches.as<fm3d_dmatch>(), (const int*)(pool + oFlag), Mcap,
                                c->verMatches.as<fm3d_dmatch>(), cnt + 0, c->scanTmp.p, st, Mdev);
    fm3d::launch_verify_report(Mdev, (const int*)(pool + oBest), (const double*)(pool + oE), dAdopted, cnt + 0,
                               (fm3d::VerifySmall*)dhv, st);
    HIPCHK(c, hipGetLastError());
    HIPCHK(c, hipEventRecord(c->ev[EV_VERIFY_END], st));
    std::swap(c->matches, c->verMatches);
    return FM3D_OK;
}

int fm3d_host::verify_report(fm3d_ctx* c, fm3d_verify_report* rep) {
    const fm3d::VerifySmall hv = *c->hVer.as<fm3d::VerifySmall>();
    if (hv.matches < 0 || hv.matches > c->pipe.nA) return fail(c, FM3D_ERR_HIP, "match count out of range");
    if (hv.verified < 0 || hv.verified > hv.matches) return fail(c, FM3D_ERR_HIP, "verify: inlier count out of range");
    std::memset(rep, 0, sizeof(*rep));
    rep->matches = hv.matches;
    rep->best = hv.best;
    rep->verified = hv.best >= 0 ? hv.verified : 0;
    rep->roundsAdopted = hv.adopted;
    std::memcpy(rep->E, hv.E, sizeof(rep->E));
    std::memcpy(rep->g12, c->g12, sizeof(rep->g12));
    float ms = 0;
    hipEventElapsedTime(&ms, c->ev[EV_VERIFY_START], c->ev[EV_VERIFY_END]);
    rep->verify_ms = ms;
    return FM3D_OK;
}

int fm3d_verify_matches(fm3d_ctx* c, const fm3d_point2f* kpts1, int n1, const fm3d_point2f* kpts2, int n2,
                        const fm3d_dmatch* matches, int nMatches, int hypotheses, double maxPx, uint64_t seed,
                        double E[9], uint8_t* inlierMask, fm3d_dmatch* inliers, int* nInliers, int* best,
                        int32_t* counts, double* models) {
    return fm3d_verify_matches_refined(c, kpts1, n1, kpts2, n2, matches, nMatches, hypotheses, maxPx, seed, 0, E,
                                       inlierMask, inliers, nInliers, best, counts, models, nullptr, nullptr, nullptr);
}

int fm3d_verify_matches_refined(fm3d_ctx* c, const fm3d_point2f* kpts1, int n1, const fm3d_point2f* kpts2, int n2,
                                const fm3d_dmatch* matches, int nMatches, int hypotheses, double maxPx, uint64_t seed,
                                int refineIters, double E[9], uint8_t* inlierMask, fm3d_dmatch* inliers, int* nInliers,
                                int* best, int32_t* counts, double* models, int32_t* roundCounts, double* roundModels,
                                int* roundsAdopted) {
    const int M = nMatches, H = hypotheses, R = refineIters;
    if (!c || !E || !nInliers || !best || n1 < 0 || n2 < 0 || M < 0 || (!kpts1 && n1) || (!kpts2 && n2) ||
        ((!matches || !inlierMask || !inliers) && M))
        return fail(c, FM3D_ERR_INVALID, "null argument");
    if (H < 1) return fail(c, FM3D_ERR_INVALID, "hypotheses must be >= 1");
    if (!(maxPx > 0. && maxPx <= DBL_MAX)) return fail(c, FM3D_ERR_INVALID, "maxPx must be finite and > 0");
    for (int i = 0; i < M; i++)
        if (matches[i].queryIdx < 0 || matches[i].queryIdx >= n1 || matches[i].trainIdx < 0 || matches[i].trainIdx >= n2)
            return fail(c, FM3D_ERR_INVALID, "match index out of range");
    if (R < 0 || R > fm3d_epi8::kRefitMaxIters) return fail(c, FM3D_ERR_INVALID, "refineIters must be in 0 .. 16");
    if (H > fm3d::kVerifyMaxHyps) return fail(c, FM3D_ERR_UNSUPPORTED, "more than 2^20 hypotheses");

    for (int k = 0; k < 9; k++) E[k] = 0.;
    *nInliers = 0;
    *best = -1;
    if (M) std::memset(inlierMask, 0, (size_t)M);
    // until a round runs: no best model gives c_0 = -1, and every round -2 and a zero candidate
    if (roundCounts) {
        roundCounts[0] = -1;
        for (int r = 0; r < R; r++) roundCounts[1 + r] = -2;
    }
    if (roundModels && R) std::memset(roundModels, 0, (size_t)R * 9 * sizeof(double));
    if (roundsAdopted) *roundsAdopted = 0;
    if (M < 8) {  // no sample exists: every hypothesis is invalid
        if (counts)
            for (int h = 0; h < H; h++) counts[h] = -1;
        if (models) std::memset(models, 0, (size_t)H * 9 * sizeof(double));
        return FM3D_OK;
    }

    const fm3d::Camera& cam = c->cam;
    const double tau = maxPx * 2.0 / (cam.fx + cam.fy);
    const double tau2 = tau * tau;

    hipStream_t st = c->stream;
    HIPCHK(c, hipSetDevice(c->device));
    int nCU = 0;
    HIPCHK(c, hipDeviceGetAttribute(&nCU, hipDeviceAttributeMultiprocessorCount, c->device));
    const int Mpad = fm3d::verify_pad(M);
    Carver cv;
    const size_t oK1 = cv.take((size_t)n1 * sizeof(fm3d_point2f)), oK2 = cv.take((size_t)n2 * sizeof(fm3d_point2f));
    const size_t oM = cv.take((size_t)M * sizeof(fm3d_dmatch)), oXY = cv.take((size_t)4 * Mpad * sizeof(double));
    const size_t oMod = cv.take((size_t)H * 9 * sizeof(double)), oCnt = cv.take((size_t)H * sizeof(int));
    const size_t oBest = cv.take(sizeof(int)), oE = cv.take(9 * sizeof(double));
    const size_t oFlag = cv.take((size_t)M * sizeof(int)), oMask = cv.take((size_t)M);
    const size_t oOut = cv.take((size_t)(M + 1) * sizeof(fm3d_dmatch)), oN = cv.take(sizeof(int));
    const size_t oTmp = cv.take(fm3d::scan_tmp_bytes(M));
    const size_t oRef = R ? cv.take(fm3d::verify_refine_bytes(M, R)) : 0;
    DevBuf buf;
    HIPCHK(c, buf.ensure(cv.off));
    char* const pool = buf.as<char>();
    HIPCHK(c, hipMemcpyAsync(pool + oK1, kpts1, (size_t)n1 * sizeof(fm3d_point2f), hipMemcpyHostToDevice, st));
    HIPCHK(c, hipMemcpyAsync(pool + oK2, kpts2, (size_t)n2 * sizeof(fm3d_point2f), hipMemcpyHostToDevice, st));
    HIPCHK(c, hipMemcpyAsync(pool + oM, matches, (size_t)M * sizeof(fm3d_dmatch), hipMemcpyHostToDevice, st));
    fm3d::launch_verify(cam, (const fm3d_point2f*)(pool + oK1), (const fm3d_point2f*)(pool + oK2),
                        (const fm3d_dmatch*)(pool + oM), M, H, seed, tau2, nCU, (double*)(pool + oXY),
                        (double*)(pool + oMod), (int*)(pool + oCnt), (int*)(pool + oBest), (double*)(pool + oE),
                        (int*)(pool + oFlag), (uint8_t*)(pool + oMask), st, R == 0);
    int *dRoundCounts = nullptr, *dAdopted = nullptr;
    double* dRoundModels = nullptr;
    if (R)  // every round queued now: the call keeps its one sync at the end
        fm3d::launch_verify_refine(M, R, tau2, (const double*)(pool + oXY), (const int*)(pool + oCnt),
                                   (const int*)(pool + oBest), (double*)(pool + oE), pool + oRef, (int*)(pool + oFlag),
                                   (uint8_t*)(pool + oMask), &dRoundCounts, &dRoundModels, &dAdopted, st);
    fm3d::launch_compact_dmatch((const fm3d_dmatch*)(pool + oM), (const int*)(pool + oFlag), M,
                                (fm3d_dmatch*)(pool + oOut), (int*)(pool + oN), pool + oTmp, st);
    HIPCHK(c, hipGetLastError());
    int n = 0;
    HIPCHK(c, hipMemcpyAsync(&n, pool + oN, sizeof(int), hipMemcpyDeviceToHost, st));
    HIPCHK(c, hipMemcpyAsync(best, pool + oBest, sizeof(int), hipMemcpyDeviceToHost, st));
    HIPCHK(c, hipMemcpyAsync(E, pool + oE, 9 * sizeof(double), hipMemcpyDeviceToHost, st));
    HIPCHK(c, hipMemcpyAsync(inlierMask, pool + oMask, (size_t)M, hipMemcpyDeviceToHost, st));
    if (counts) HIPCHK(c, hipMemcpyAsync(counts, pool + oCnt, (size_t)H * sizeof(int), hipMemcpyDeviceToHost, st));
    if (models) HIPCHK(c, hipMemcpyAsync(models, pool + oMod, (size_t)H * 9 * sizeof(double), hipMemcpyDeviceToHost, st));
    if (R) {
        if (roundCounts)
            HIPCHK(c, hipMemcpyAsync(roundCounts, dRoundCounts, (size_t)(R + 1) * sizeof(int), hipMemcpyDeviceToHost, st));
        if (roundModels)
            HIPCHK(c, hipMemcpyAsync(roundModels, dRoundModels, (size_t)R * 9 * sizeof(double), hipMemcpyDeviceToHost, st));
        if (roundsAdopted) HIPCHK(c, hipMemcpyAsync(roundsAdopted, dAdopted, sizeof(int), hipMemcpyDeviceToHost, st));
    }
    HIPCHK(c, hipStreamSynchronize(st));
    if (n < 0 || n > M) return fail(c, FM3D_ERR_HIP, "verify: inlier count out of range");
    if (n) HIPCHK(c, hipMemcpy(inliers, pool + oOut, (size_t)n * sizeof(fm3d_dmatch), hipMemcpyDeviceToHost));
    *nInliers = n;
    if (R == 0 && roundCounts && *best >= 0) roundCounts[0] = n;  // c_0: the best model's count
    return FM3D_OK;
}
