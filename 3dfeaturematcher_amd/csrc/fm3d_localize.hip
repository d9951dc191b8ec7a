// fm3d_localize.hip -- 2D-3D localisation of an image against a feature model: a RANSAC
// fit of the camera pose Xc = R X + t to matches between model points and keypoints, up to four P3P
// models per sample, every hypothesis scored against every match (with the model's normals as an
// optional second test), and the rounds of a Gauss-Newton refit of the best model on the matches it
// accepts.  The arithmetic is include/fm3d_pnp.h's (shared with the host entry points and restated in
// tests/pnp_pyref.py); the kernels only distribute it, in fm3d_align.hip's shapes.
#include <hip/hip_runtime.h>

#include "fm3d_device.h"
#include "fm3d_kernels.h"
#include "fm3d_pnp.h"

namespace fm3d {
namespace {

namespace pnp = fm3d_pnp;

constexpr int kHypThreads = 64;
constexpr int kScoreThreads = 256;
constexpr int kScorePer = 4;    // matches a lane keeps in registers
constexpr int kScoreHyps = 64;  // most hypotheses one workgroup scores
constexpr int kM = pnp::kModel;
static_assert(kScoreThreads * kScorePer == kVerifyTile, "a scoring workgroup covers one tile of matches");
static_assert(kScoreThreads == pnp::kLanes && kVerifyTile == pnp::kTile, "the refit sums run over the scoring kernel's tile");
static_assert(kScorePer == 4, "leaf4 adds a lane's four slots");

// pl: P planes of Mpad doubles -- u v X.x X.y X.z, with the normal n.xyz behind them; the pad holds NaN,
// which no model accepts, and so does a match whose index lies outside its array (the entry points
// refuse those on the host; the matcher's own never do)
__global__ __launch_bounds__(256) void localize_gather_kernel(Camera cam, LocalizeIn in,
                                                              const fm3d_dmatch* __restrict__ matches, int M, int Mpad,
                                                              double* __restrict__ pl) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= Mpad) return;
    const bool nrm = in.nrm != nullptr;
    double v[8];
#pragma unroll
    for (int k = 0; k < 8; k++) v[k] = __builtin_nan("");
    if (i < M) {
        const fm3d_dmatch m = matches[i];
        const int q = m.queryIdx, t = m.trainIdx;
        if (q >= 0 && q < in.nKpts && t >= 0 && t < in.nPts) {
            const fm3d_point2f kp = in.kpts[q];
            undistort1(cam, (double)kp.x, (double)kp.y, v[0], v[1]);
#pragma unroll
            for (int k = 0; k < 3; k++) v[2 + k] = in.pts[(size_t)t * 3 + k];
            if (nrm) {
#pragma unroll
                for (int k = 0; k < 3; k++) v[5 + k] = in.nrm[(size_t)t * 3 + k];
            }
        }
    }
    const int P = nrm ? 8 : 5;
#pragma unroll
    for (int k = 0; k < 8; k++)
        if (k < P) pl[(size_t)k * Mpad + i] = v[k];
}

// one thread per sample: its three matches, the quartic and the four slots' solves in registers (named
// coefficients and roots, loops of constant trip count: nothing is indexed at run time); hypothesis
// 4 h + k is slot k of sample h
__global__ __launch_bounds__(kHypThreads) void localize_hypothesis_kernel(const double* __restrict__ pl, int M, int Mpad,
                                                                          int S, unsigned long long seed,
                                                                          double* __restrict__ models,
                                                                          int* __restrict__ count) {
    const int h = blockIdx.x * kHypThreads + threadIdx.x;
    if (h >= S) return;
    int idx[3];
    double m[pnp::kSlots][kM];
    bool ok[pnp::kSlots];
    if (pnp::r3::sample3(seed, (uint32_t)h, (uint32_t)M, idx)) {
        double X[3][3], uv[3][2];
#pragma unroll
        for (int k = 0; k < 3; k++) {
            const int i = idx[k];  // in [0, M)
            uv[k][0] = pl[i];
            uv[k][1] = pl[(size_t)Mpad + i];
#pragma unroll
            for (int r = 0; r < 3; r++) X[k][r] = pl[(size_t)(2 + r) * Mpad + i];
        }
        pnp::p3p(X, uv, m, ok);
    } else {
#pragma unroll
        for (int k = 0; k < pnp::kSlots; k++) {
            pnp::zero_model(m[k]);
            ok[k] = false;
        }
    }
#pragma unroll
    for (int k = 0; k < pnp::kSlots; k++) {
#pragma unroll
        for (int e = 0; e < kM; e++) models[((size_t)h * pnp::kSlots + k) * kM + e] = m[k][e];
        count[h * pnp::kSlots + k] = ok[k] ? 0 : -1;
    }
}

// a lane's four slots of tile `tile`: every plane's values in registers
template <int P>
__device__ __forceinline__ void load_slots(const double* __restrict__ pl, int Mpad, int tile, int tid,
                                           double (&v)[kScorePer][P]) {
#pragma unroll
    for (int k = 0; k < kScorePer; k++) {
        const size_t i = (size_t)tile * kVerifyTile + k * kScoreThreads + tid;  // < Mpad
#pragma unroll
        for (int p = 0; p < P; p++) v[k][p] = pl[(size_t)p * Mpad + i];
    }
}

template <bool N>
__device__ __forceinline__ bool accepts(const double* m, const double* v, double tau2, double cos2) {
    if constexpr (N)
        return pnp::inlier_n(m, v[0], v[1], v[2], v[3], v[4], v[5], v[6], v[7], tau2, cos2);
    else
        return pnp::inlier(m, v[0], v[1], v[2], v[3], v[4], tau2);
}

// Workgroup (bx, by): the tile of 1024 matches bx against the hc hypotheses from by * hc.  A lane
// keeps four matches' values (20 doubles, 32 with normals: N is a template instance of its own); a
// hypothesis's twelve coefficients have one address per wave (scalar loads); a wave counts with
// ballots, the workgroup adds its four waves in LDS, and one atomicAdd per (workgroup, hypothesis) with
// a non-zero count goes to count[h] -- integers, exact in any order.  An invalid hypothesis keeps its
// -1: nothing is added to it (its word never changes, so reading it beside the other workgroups'
// atomics is safe).
template <bool N>
__global__ __launch_bounds__(kScoreThreads) void localize_score_kernel(const double* __restrict__ pl, int Mpad,
                                                                       const double* __restrict__ models, int H, int hc,
                                                                       double tau2, double cos2, int* count) {
    __shared__ int sCnt[kScoreThreads / 64][kScoreHyps];
    constexpr int P = N ? 8 : 5;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    double v[kScorePer][P];
    load_slots<P>(pl, Mpad, blockIdx.x, tid, v);
    const int h0 = blockIdx.y * hc;
    const int nh = min(hc, H - h0);
    for (int j = 0; j < nh; j++) {
        const double* __restrict__ mp = models + (size_t)(h0 + j) * kM;
        double m[kM];
#pragma unroll
        for (int k = 0; k < kM; k++) m[k] = mp[k];
        int c = 0;
#pragma unroll
        for (int k = 0; k < kScorePer; k++) c += __popcll(__ballot(accepts<N>(m, v[k], tau2, cos2)));
        if (lane == 0) sCnt[wave][j] = c;
    }
    __syncthreads();
    if (tid < nh) {
        int s = 0;
#pragma unroll
        for (int w = 0; w < kScoreThreads / 64; w++) s += sCnt[w][tid];
        if (s && count[h0 + tid] >= 0) atomicAdd(&count[h0 + tid], s);
    }
}

// the largest count, the lowest h on ties; no valid hypothesis: best = -1 and the zero model
__global__ __launch_bounds__(256) void localize_argmax_kernel(const int* __restrict__ count,
                                                              const double* __restrict__ models, int H,
                                                              int* __restrict__ best, double* __restrict__ model) {
    __shared__ int sC[256], sH[256];
    const int tid = threadIdx.x;
    int bc = -1, bh = 0x7fffffff;
    for (int h = tid; h < H; h += 256) {
        const int c = count[h];
        if (c > bc) {
            bc = c;
            bh = h;
        }
    }
    sC[tid] = bc;
    sH[tid] = bh;
    __syncthreads();
    for (int o = 128; o > 0; o >>= 1) {
        if (tid < o) {
            const int c = sC[tid + o], h = sH[tid + o];
            if (c > sC[tid] || (c == sC[tid] && h < sH[tid])) {
                sC[tid] = c;
                sH[tid] = h;
            }
        }
        __syncthreads();
    }
    if (tid < kM) {
        const bool any = sC[0] >= 0;
        model[tid] = any ? models[(size_t)sH[0] * kM + tid] : 0.;
        if (tid == 0) *best = any ? sH[0] : -1;
    }
}

template <bool N>
__global__ __launch_bounds__(256) void localize_mask_kernel(const double* __restrict__ pl, int M, int Mpad,
                                                            const int* __restrict__ best,
                                                            const double* __restrict__ model, double tau2, double cos2,
                                                            int* __restrict__ flag, uint8_t* __restrict__ mask) {
    constexpr int P = N ? 8 : 5;
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= M) return;
    double m[kM], v[P];
#pragma unroll
    for (int k = 0; k < kM; k++) m[k] = model[k];
#pragma unroll
    for (int p = 0; p < P; p++) v[p] = pl[(size_t)p * Mpad + i];
    const bool in = *best >= 0 && accepts<N>(m, v, tau2, cos2);
    flag[i] = in ? 1 : 0;
    mask[i] = in ? 1 : 0;
}

// ---------------- refinement: the Gauss-Newton step on the accepted matches, round by round ----------------
// st: the rounds' state on the device.  Every kernel of a round tests st[kStDone] first.
enum { kStDone = 0, kStCount = 1, kStValid = 2, kStCand = 3, kStAdopted = 4, kStWords = 8 };

// c_0 and the flags: no best model leaves every round undone
__global__ __launch_bounds__(64) void localize_refine_init_kernel(const int* __restrict__ best,
                                                                  const int* __restrict__ count, int rounds,
                                                                  int* __restrict__ st, int* __restrict__ roundCounts,
                                                                  double* __restrict__ roundModels) {
    const int tid = threadIdx.x;
    const int b = *best;
    const int c0 = b >= 0 ? count[b] : -1;
    if (tid == 0) {
        st[kStDone] = b < 0;
        st[kStCount] = c0;
        st[kStValid] = 0;
        st[kStCand] = -1;
        st[kStAdopted] = 0;
        roundCounts[0] = c0;
    }
    for (int r = tid; r < rounds; r += 64) roundCounts[1 + r] = -2;
    for (int k = tid; k < rounds * kM; k += 64) roundModels[k] = 0.;
}

// one sum of a tile from the lanes' leaves: the wave's 64 leaves through an xor butterfly (strides
// 1 .. 32: the balanced tree's bits in every lane, IEEE addition being commutative); lane 0 keeps it
__device__ __forceinline__ double wave_tree(double s) {
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) s = s + __shfl_xor(s, o);
    return s;
}

// Workgroup bx: the 28 sums of tile bx under the current model -- J^T J's upper triangle, J^T r and the
// count, each slot +0.0 unless its match is in.  A lane holds the four slots k * 256 + tid, keeps
// fm3d_pnp::jacobian's fourteen values of each and forms leaf4 of their products; the four waves add
// through LDS as (w0 + w1) + (w2 + w3).
template <bool N>
__global__ __launch_bounds__(kScoreThreads) void localize_refit_sum_kernel(const double* __restrict__ pl, int Mpad,
                                                                           const double* __restrict__ cur, double tau2,
                                                                           double cos2, const int* __restrict__ st,
                                                                           double* __restrict__ partial) {
    __shared__ double sW[kScoreThreads / 64][pnp::kSums];
    constexpr int P = N ? 8 : 5;
    if (st[kStDone]) return;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    double m[kM];
#pragma unroll
    for (int k = 0; k < kM; k++) m[k] = cur[k];
    double v[kScorePer][P];
    load_slots<P>(pl, Mpad, blockIdx.x, tid, v);
    bool in[kScorePer];
    double J[kScorePer][14];
#pragma unroll
    for (int k = 0; k < kScorePer; k++) {
        in[k] = accepts<N>(m, v[k], tau2, cos2);
        pnp::jacobian(m, v[k][0], v[k][1], v[k][2], v[k][3], v[k][4], J[k]);
    }
    int n = 0;
#pragma unroll
    for (int i = 0; i < 6; i++)
#pragma unroll
        for (int k = i; k < 7; k++) {
            // (i, 6) is entry i of J^T r: its sum's index follows the 21 of J^T J
            const int j = k == 6 ? pnp::kJtJ + i : n++;
            double s = fm3d_epi8::leaf4(pnp::slot(in[0], pnp::term(J[0], i, k)), pnp::slot(in[1], pnp::term(J[1], i, k)),
                                        pnp::slot(in[2], pnp::term(J[2], i, k)), pnp::slot(in[3], pnp::term(J[3], i, k)));
            s = wave_tree(s);
            if (lane == 0) sW[wave][j] = s;
        }
    {
        double s = fm3d_epi8::leaf4(pnp::slot(in[0], 1.), pnp::slot(in[1], 1.), pnp::slot(in[2], 1.), pnp::slot(in[3], 1.));
        s = wave_tree(s);
        if (lane == 0) sW[wave][pnp::kSums - 1] = s;
    }
    __syncthreads();
    if (tid < pnp::kSums)
        partial[(size_t)blockIdx.x * pnp::kSums + tid] = (sW[0][tid] + sW[1][tid]) + (sW[2][tid] + sW[3][tid]);
}

// One workgroup of one wave: 28 threads add the tile partials in tile order from +0.0, thread 0
// solves.  cand: the new model (zero when invalid); st: the valid flag and the candidate's count, 0
// for the count kernel to add to, -1 when there is nothing to count.
__global__ __launch_bounds__(64) void localize_refit_solve_kernel(const double* __restrict__ partial, int tiles,
                                                                  const double* __restrict__ cur, int* __restrict__ st,
                                                                  double* __restrict__ cand) {
    __shared__ double sS[pnp::kSums];
    const int tid = threadIdx.x;
    if (st[kStDone]) return;
    if (tid < pnp::kSums) {
        double s = 0.;
        for (int t = 0; t < tiles; t++) s = s + partial[(size_t)t * pnp::kSums + tid];
        sS[tid] = s;
    }
    __syncthreads();
    if (tid == 0) {
        double S[pnp::kSums], m[kM], out[kM];
#pragma unroll
        for (int k = 0; k < pnp::kSums; k++) S[k] = sS[k];
#pragma unroll
        for (int k = 0; k < kM; k++) m[k] = cur[k];
        const bool valid = pnp::step_solve(S, m, out);
#pragma unroll
        for (int k = 0; k < kM; k++) cand[k] = out[k];
        st[kStValid] = valid ? 1 : 0;
        st[kStCand] = valid ? 0 : -1;
    }
}

// c' of a valid candidate: the scoring kernel's count for one model, behind the rounds' flags
// (integers: the atomicAdd per workgroup is exact in any order)
template <bool N>
__global__ __launch_bounds__(kScoreThreads) void localize_count_kernel(const double* __restrict__ pl, int Mpad,
                                                                       const double* __restrict__ cand, double tau2,
                                                                       double cos2, int* __restrict__ st) {
    __shared__ int sCnt[kScoreThreads / 64];
    constexpr int P = N ? 8 : 5;
    if (st[kStDone] || !st[kStValid]) return;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    double m[kM];
#pragma unroll
    for (int k = 0; k < kM; k++) m[k] = cand[k];
    double v[kScorePer][P];
    load_slots<P>(pl, Mpad, blockIdx.x, tid, v);
    int c = 0;
#pragma unroll
    for (int k = 0; k < kScorePer; k++) c += __popcll(__ballot(accepts<N>(m, v[k], tau2, cos2)));
    if (lane == 0) sCnt[wave] = c;
    __syncthreads();
    if (tid == 0) {
        const int n = (sCnt[0] + sCnt[1]) + (sCnt[2] + sCnt[3]);
        if (n) atomicAdd(&st[kStCand], n);
    }
}

// The rule of round r: adopt the candidate iff it is valid and keeps at least as many matches;
// otherwise the current model is final and every later round is skipped.
__global__ __launch_bounds__(64) void localize_adopt_kernel(int r, int* __restrict__ st, const double* __restrict__ cand,
                                                            double* __restrict__ cur, int* __restrict__ roundCounts,
                                                            double* __restrict__ roundModels) {
    const int tid = threadIdx.x;
    if (st[kStDone]) return;
    const int valid = st[kStValid], cc = st[kStCand], c0 = st[kStCount];
    const bool adopt = valid && cc >= c0;
    __syncthreads();  // every thread has read the state before thread 0 changes it
    if (tid < kM) {
        const double e = cand[tid];
        roundModels[r * kM + tid] = e;
        if (adopt) cur[tid] = e;
    }
    if (tid == 0) {
        roundCounts[1 + r] = cc;
        if (adopt) {
            st[kStCount] = cc;
            st[kStAdopted] = st[kStAdopted] + 1;
        } else {
            st[kStDone] = 1;
        }
    }
}

template <bool N>
void refine_rounds(int M, int rounds, double tau2, double cos2, const double* pl, double* model, double* part,
                   double* cand, int* st, int* rc, double* rm, const int* best, int* flag, uint8_t* mask, hipStream_t s) {
    const int Mpad = verify_pad(M), tiles = Mpad / kVerifyTile;
    for (int r = 0; r < rounds; r++) {
        localize_refit_sum_kernel<N><<<tiles, kScoreThreads, 0, s>>>(pl, Mpad, model, tau2, cos2, st, part);
        localize_refit_solve_kernel<<<1, 64, 0, s>>>(part, tiles, model, st, cand);
        localize_count_kernel<N><<<tiles, kScoreThreads, 0, s>>>(pl, Mpad, cand, tau2, cos2, st);
        localize_adopt_kernel<<<1, 64, 0, s>>>(r, st, cand, model, rc, rm);
    }
    localize_mask_kernel<N><<<(M + 255) / 256, 256, 0, s>>>(pl, M, Mpad, best, model, tau2, cos2, flag, mask);
}

}  // namespace

size_t localize_refine_bytes(int M, int rounds) {
    const size_t tiles = (size_t)verify_pad(M) / kVerifyTile;
    return tiles * pnp::kSums * sizeof(double) + kM * sizeof(double) + (size_t)rounds * kM * sizeof(double) +
           (size_t)(kStWords + 1 + rounds) * sizeof(int);
}

void launch_localize_refine(int M, bool normals, int rounds, double tau2, double cos2, const double* planes,
                            const int* count, const int* best, double* model, void* work, int* flag, uint8_t* mask,
                            int** roundCounts, double** roundModels, int** adopted, hipStream_t s) {
    const int tiles = verify_pad(M) / kVerifyTile;
    double* part = (double*)work;
    double* cand = part + (size_t)tiles * pnp::kSums;
    double* rm = cand + kM;
    int* st = (int*)(rm + (size_t)rounds * kM);
    int* rc = st + kStWords;
    localize_refine_init_kernel<<<1, 64, 0, s>>>(best, count, rounds, st, rc, rm);
    if (normals)
        refine_rounds<true>(M, rounds, tau2, cos2, planes, model, part, cand, st, rc, rm, best, flag, mask, s);
    else
        refine_rounds<false>(M, rounds, tau2, cos2, planes, model, part, cand, st, rc, rm, best, flag, mask, s);
    *roundCounts = rc;
    *roundModels = rm;
    *adopted = st + kStAdopted;
}

void launch_localize(const Camera& cam, const LocalizeIn& in, const fm3d_dmatch* matches, int M, int samples,
                     unsigned long long seed, double tau2, double cos2, int nCU, double* planes, double* models,
                     int* count, int* best, double* model, int* flag, uint8_t* mask, hipStream_t s, bool withMask) {
    const int Mpad = verify_pad(M), H = samples * pnp::kSlots;
    const bool normals = in.nrm != nullptr;
    localize_gather_kernel<<<(Mpad + 255) / 256, 256, 0, s>>>(cam, in, matches, M, Mpad, planes);
    localize_hypothesis_kernel<<<(samples + kHypThreads - 1) / kHypThreads, kHypThreads, 0, s>>>(planes, M, Mpad, samples,
                                                                                               seed, models, count);
    // hypotheses per workgroup: 64, halved while the grid has fewer than four workgroups per CU
    // (the chunks go to grid.y: at most 65535, which 64 per workgroup keeps for H <= kVerifyMaxHyps)
    const int tiles = Mpad / kVerifyTile;
    int hc = kScoreHyps;
    while (hc > 1 && (long long)tiles * ((H + hc - 1) / hc) < 4ll * nCU && (H + hc / 2 - 1) / (hc / 2) <= 65535)
        hc >>= 1;
    const dim3 grid(tiles, (H + hc - 1) / hc);
    if (normals) {
        localize_score_kernel<true><<<grid, kScoreThreads, 0, s>>>(planes, Mpad, models, H, hc, tau2, cos2, count);
        localize_argmax_kernel<<<1, 256, 0, s>>>(count, models, H, best, model);
        if (withMask)
            localize_mask_kernel<true><<<(M + 255) / 256, 256, 0, s>>>(planes, M, Mpad, best, model, tau2, cos2, flag, mask);
    } else {
        localize_score_kernel<false><<<grid, kScoreThreads, 0, s>>>(planes, Mpad, models, H, hc, tau2, cos2, count);
        localize_argmax_kernel<<<1, 256, 0, s>>>(count, models, H, best, model);
        if (withMask)
            localize_mask_kernel<false><<<(M + 255) / 256, 256, 0, s>>>(planes, M, Mpad, best, model, tau2, cos2, flag, mask);
    }
}

}  // namespace fm3d
