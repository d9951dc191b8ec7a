// fm3d_align.hip -- 3D-3D alignment of two feature models: a RANSAC fit of a rigid
// transform b = R a + t to matched points, every hypothesis scored against every match (with the
// normals as an optional second test), and the rounds of a refit of the best model on the pairs it
// accepts.  The arithmetic is include/fm3d_rigid3.h's (shared with the host entry points and restated
// in tests/align_pyref.py); the kernels only distribute it, in fm3d_verify.hip's shapes.
#include <hip/hip_runtime.h>

#include "fm3d_kernels.h"
#include "fm3d_rigid3.h"

namespace fm3d {
namespace {

namespace r3 = fm3d_rigid3;

constexpr int kHypThreads = 64;
constexpr int kScoreThreads = 256;
constexpr int kScorePer = 4;    // matches a lane keeps in registers
constexpr int kScoreHyps = 64;  // most hypotheses one workgroup scores
constexpr int kM = r3::kModel;
static_assert(kScoreThreads * kScorePer == kVerifyTile, "a scoring workgroup covers one tile of matches");
static_assert(kScoreThreads == r3::kLanes && kVerifyTile == r3::kTile, "the refit sums run over the scoring kernel's tile");
static_assert(kScorePer == 4, "leaf4 adds a lane's four slots");

// pl: P planes of Mpad doubles -- a.x a.y a.z b.x b.y b.z, with normals na.xyz nb.xyz behind them; the
// pad holds NaN, which no model accepts, and so does a match whose index lies outside its array (the
// entry points refuse those on the host; the matcher's own never do)
__global__ __launch_bounds__(256) void align_gather_kernel(AlignIn in, const fm3d_dmatch* __restrict__ matches, int M,
                                                           int Mpad, double* __restrict__ pl) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= Mpad) return;
    const bool nrm = in.nrmA != nullptr;
    double v[12];
#pragma unroll
    for (int k = 0; k < 12; k++) v[k] = __builtin_nan("");
    if (i < M) {
        const fm3d_dmatch m = matches[i];
        const int q = m.queryIdx, t = m.trainIdx;
        if (q >= 0 && q < in.nA && t >= 0 && t < in.nB) {
#pragma unroll
            for (int k = 0; k < 3; k++) {
                v[k] = in.ptsA[(size_t)q * 3 + k];
                v[3 + k] = in.ptsB[(size_t)t * 3 + k];
            }
            if (nrm) {
#pragma unroll
                for (int k = 0; k < 3; k++) {
                    v[6 + k] = in.nrmA[(size_t)q * 3 + k];
                    v[9 + k] = in.nrmB[(size_t)t * 3 + k];
                }
            }
        }
    }
    const int P = nrm ? 12 : 6;
#pragma unroll
    for (int k = 0; k < 12; k++)
        if (k < P) pl[(size_t)k * Mpad + i] = v[k];
}

// one thread per hypothesis: the sample, its three pairs and the solve in registers (the 3 x 3 SVD has
// no run-time-indexed entries)
__global__ __launch_bounds__(kHypThreads) void align_hypothesis_kernel(const double* __restrict__ pl, int M, int Mpad,
                                                                       int H, unsigned long long seed,
                                                                       double* __restrict__ models,
                                                                       int* __restrict__ count) {
    const int h = blockIdx.x * kHypThreads + threadIdx.x;
    if (h >= H) return;
    int idx[3];
    double m[kM];
    bool ok = r3::sample3(seed, (uint32_t)h, (uint32_t)M, idx);
    if (ok) {
        double a[3][3], b[3][3];
#pragma unroll
        for (int k = 0; k < 3; k++) {
            const int i = idx[k];  // in [0, M)
#pragma unroll
            for (int r = 0; r < 3; r++) {
                a[k][r] = pl[(size_t)r * Mpad + i];
                b[k][r] = pl[(size_t)(3 + r) * Mpad + i];
            }
        }
        ok = r3::rigid_from3(a, b, m);
    } else {
        r3::zero_model(m);
    }
#pragma unroll
    for (int k = 0; k < kM; k++) models[(size_t)h * kM + k] = m[k];
    count[h] = ok ? 0 : -1;
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
__device__ __forceinline__ bool accepts(const double* m, const double* v, double tau2, double minCos) {
    if constexpr (N)
        return r3::inlier_n(m, v[0], v[1], v[2], v[3], v[4], v[5], v[6], v[7], v[8], v[9], v[10], v[11], tau2, minCos);
    else
        return r3::inlier(m, v[0], v[1], v[2], v[3], v[4], v[5], tau2);
}

// Workgroup (bx, by): the tile of 1024 matches bx against the hc hypotheses from by * hc.  A lane
// keeps four matches' coordinates (24 doubles, 48 with normals: N is a template instance of its own);
// a hypothesis's twelve coefficients have one address per wave (scalar loads); a wave counts with
// ballots, the workgroup adds its four waves in LDS, and one atomicAdd per (workgroup, hypothesis) with
// a non-zero count goes to count[h] -- integers, exact in any order.  An invalid hypothesis keeps its
// -1: nothing is added to it (its word never changes, so reading it beside the other workgroups'
// atomics is safe).
template <bool N>
__global__ __launch_bounds__(kScoreThreads) void align_score_kernel(const double* __restrict__ pl, int Mpad,
                                                                    const double* __restrict__ models, int H, int hc,
                                                                    double tau2, double minCos, int* count) {
    __shared__ int sCnt[kScoreThreads / 64][kScoreHyps];
    constexpr int P = N ? 12 : 6;
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
        for (int k = 0; k < kScorePer; k++) c += __popcll(__ballot(accepts<N>(m, v[k], tau2, minCos)));
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
__global__ __launch_bounds__(256) void align_argmax_kernel(const int* __restrict__ count,
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
__global__ __launch_bounds__(256) void align_mask_kernel(const double* __restrict__ pl, int M, int Mpad,
                                                         const int* __restrict__ best, const double* __restrict__ model,
                                                         double tau2, double minCos, int* __restrict__ flag,
                                                         uint8_t* __restrict__ mask) {
    constexpr int P = N ? 12 : 6;
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= M) return;
    double m[kM], v[P];
#pragma unroll
    for (int k = 0; k < kM; k++) m[k] = model[k];
#pragma unroll
    for (int p = 0; p < P; p++) v[p] = pl[(size_t)p * Mpad + i];
    const bool in = *best >= 0 && accepts<N>(m, v, tau2, minCos);
    flag[i] = in ? 1 : 0;
    mask[i] = in ? 1 : 0;
}

// ---------------- refinement: the refit on the accepted pairs, round by round ----------------
// st: the rounds' state on the device.  Every kernel of a round tests st[kStDone] first.
enum { kStDone = 0, kStCount = 1, kStValid = 2, kStCand = 3, kStAdopted = 4, kStWords = 8 };

// c_0 and the flags: no best model leaves every round undone
__global__ __launch_bounds__(64) void align_refine_init_kernel(const int* __restrict__ best,
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

// Workgroup bx, first pass: the seven sums of tile bx under the current model -- the coordinates of a
// and of b and the count, each slot +0.0 unless its pair is in.  A lane holds the four slots
// k * 256 + tid and forms leaf4 of them; the four waves add through LDS as (w0 + w1) + (w2 + w3).
template <bool N>
__global__ __launch_bounds__(kScoreThreads) void align_refit_sum1_kernel(const double* __restrict__ pl, int Mpad,
                                                                         const double* __restrict__ cur, double tau2,
                                                                         double minCos, const int* __restrict__ st,
                                                                         double* __restrict__ partial1) {
    __shared__ double sW[kScoreThreads / 64][r3::kSums1];
    constexpr int P = N ? 12 : 6;
    if (st[kStDone]) return;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    double m[kM];
#pragma unroll
    for (int k = 0; k < kM; k++) m[k] = cur[k];
    double v[kScorePer][P];
    load_slots<P>(pl, Mpad, blockIdx.x, tid, v);
    bool in[kScorePer];
#pragma unroll
    for (int k = 0; k < kScorePer; k++) in[k] = accepts<N>(m, v[k], tau2, minCos);
#pragma unroll
    for (int j = 0; j < r3::kSums1; j++) {
        double s;
        if (j < 6)
            s = fm3d_epi8::leaf4(r3::slot(in[0], v[0][j]), r3::slot(in[1], v[1][j]), r3::slot(in[2], v[2][j]),
                                 r3::slot(in[3], v[3][j]));
        else
            s = fm3d_epi8::leaf4(r3::slot(in[0], 1.), r3::slot(in[1], 1.), r3::slot(in[2], 1.), r3::slot(in[3], 1.));
        s = wave_tree(s);
        if (lane == 0) sW[wave][j] = s;
    }
    __syncthreads();
    if (tid < r3::kSums1)
        partial1[(size_t)blockIdx.x * r3::kSums1 + tid] = (sW[0][tid] + sW[1][tid]) + (sW[2][tid] + sW[3][tid]);
}

// Workgroup bx, second pass: every workgroup first adds the first pass's tile partials in tile order
// from +0.0 (seven threads; the same bits in every workgroup and in the solve) for the centroids, then
// the nine centred cross sums of tile bx in the first pass's shape.
template <bool N>
__global__ __launch_bounds__(kScoreThreads) void align_refit_sum2_kernel(const double* __restrict__ pl, int Mpad,
                                                                         const double* __restrict__ cur, double tau2,
                                                                         double minCos, const int* __restrict__ st,
                                                                         const double* __restrict__ partial1,
                                                                         double* __restrict__ partial2) {
    __shared__ double sS1[r3::kSums1];
    __shared__ double sW[kScoreThreads / 64][r3::kSums2];
    constexpr int P = N ? 12 : 6;
    if (st[kStDone]) return;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int tiles = Mpad / kVerifyTile;
    if (tid < r3::kSums1) {
        double s = 0.;
        for (int t = 0; t < tiles; t++) s = s + partial1[(size_t)t * r3::kSums1 + tid];
        sS1[tid] = s;
    }
    __syncthreads();
    double S1[r3::kSums1], ca[3], cb[3];
#pragma unroll
    for (int k = 0; k < r3::kSums1; k++) S1[k] = sS1[k];
    r3::centroids(S1, ca, cb);
    double m[kM];
#pragma unroll
    for (int k = 0; k < kM; k++) m[k] = cur[k];
    double v[kScorePer][P];
    load_slots<P>(pl, Mpad, blockIdx.x, tid, v);
    bool in[kScorePer];
#pragma unroll
    for (int k = 0; k < kScorePer; k++) in[k] = accepts<N>(m, v[k], tau2, minCos);
#pragma unroll
    for (int r = 0; r < 3; r++)
#pragma unroll
        for (int c = 0; c < 3; c++) {
            double s = fm3d_epi8::leaf4(
                r3::slot2(in[0], v[0][r], ca[r], v[0][3 + c], cb[c]), r3::slot2(in[1], v[1][r], ca[r], v[1][3 + c], cb[c]),
                r3::slot2(in[2], v[2][r], ca[r], v[2][3 + c], cb[c]), r3::slot2(in[3], v[3][r], ca[r], v[3][3 + c], cb[c]));
            s = wave_tree(s);
            if (lane == 0) sW[wave][r * 3 + c] = s;
        }
    __syncthreads();
    if (tid < r3::kSums2)
        partial2[(size_t)blockIdx.x * r3::kSums2 + tid] = (sW[0][tid] + sW[1][tid]) + (sW[2][tid] + sW[3][tid]);
}

// One workgroup of one wave: sixteen threads add the two passes' tile partials in tile order from
// +0.0, thread 0 solves.  cand: the new model (zero when invalid); st: the valid flag and the
// candidate's count, 0 for the count kernel to add to, -1 when there is nothing to count.
__global__ __launch_bounds__(64) void align_refit_solve_kernel(const double* __restrict__ partial1,
                                                               const double* __restrict__ partial2, int tiles,
                                                               int* __restrict__ st, double* __restrict__ cand) {
    __shared__ double sS[r3::kSums1 + r3::kSums2];
    const int tid = threadIdx.x;
    if (st[kStDone]) return;
    if (tid < r3::kSums1 + r3::kSums2) {
        const bool first = tid < r3::kSums1;
        const double* __restrict__ p = first ? partial1 + tid : partial2 + (tid - r3::kSums1);
        const int stride = first ? r3::kSums1 : r3::kSums2;
        double s = 0.;
        for (int t = 0; t < tiles; t++) s = s + p[(size_t)t * stride];
        sS[tid] = s;
    }
    __syncthreads();
    if (tid == 0) {
        double S1[r3::kSums1], S2[r3::kSums2], m[kM];
#pragma unroll
        for (int k = 0; k < r3::kSums1; k++) S1[k] = sS[k];
#pragma unroll
        for (int k = 0; k < r3::kSums2; k++) S2[k] = sS[r3::kSums1 + k];
        const bool valid = r3::refit_solve(S1, S2, m);
#pragma unroll
        for (int k = 0; k < kM; k++) cand[k] = m[k];
        st[kStValid] = valid ? 1 : 0;
        st[kStCand] = valid ? 0 : -1;
    }
}

// c' of a valid candidate: the scoring kernel's count for one model, behind the rounds' flags
// (integers: the atomicAdd per workgroup is exact in any order)
template <bool N>
__global__ __launch_bounds__(kScoreThreads) void align_count_kernel(const double* __restrict__ pl, int Mpad,
                                                                    const double* __restrict__ cand, double tau2,
                                                                    double minCos, int* __restrict__ st) {
    __shared__ int sCnt[kScoreThreads / 64];
    constexpr int P = N ? 12 : 6;
    if (st[kStDone] || !st[kStValid]) return;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    double m[kM];
#pragma unroll
    for (int k = 0; k < kM; k++) m[k] = cand[k];
    double v[kScorePer][P];
    load_slots<P>(pl, Mpad, blockIdx.x, tid, v);
    int c = 0;
#pragma unroll
    for (int k = 0; k < kScorePer; k++) c += __popcll(__ballot(accepts<N>(m, v[k], tau2, minCos)));
    if (lane == 0) sCnt[wave] = c;
    __syncthreads();
    if (tid == 0) {
        const int n = (sCnt[0] + sCnt[1]) + (sCnt[2] + sCnt[3]);
        if (n) atomicAdd(&st[kStCand], n);
    }
}

// The rule of round r: adopt the candidate iff it is valid and keeps at least as many matches;
// otherwise the current model is final and every later round is skipped.
__global__ __launch_bounds__(64) void align_adopt_kernel(int r, int* __restrict__ st, const double* __restrict__ cand,
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
void refine_rounds(int M, int rounds, double tau2, double minCos, const double* pl, double* model, double* p1,
                   double* p2, double* cand, int* st, int* rc, double* rm, const int* best, int* flag, uint8_t* mask,
                   hipStream_t s) {
    const int Mpad = verify_pad(M), tiles = Mpad / kVerifyTile;
    for (int r = 0; r < rounds; r++) {
        align_refit_sum1_kernel<N><<<tiles, kScoreThreads, 0, s>>>(pl, Mpad, model, tau2, minCos, st, p1);
        align_refit_sum2_kernel<N><<<tiles, kScoreThreads, 0, s>>>(pl, Mpad, model, tau2, minCos, st, p1, p2);
        align_refit_solve_kernel<<<1, 64, 0, s>>>(p1, p2, tiles, st, cand);
        align_count_kernel<N><<<tiles, kScoreThreads, 0, s>>>(pl, Mpad, cand, tau2, minCos, st);
        align_adopt_kernel<<<1, 64, 0, s>>>(r, st, cand, model, rc, rm);
    }
    align_mask_kernel<N><<<(M + 255) / 256, 256, 0, s>>>(pl, M, Mpad, best, model, tau2, minCos, flag, mask);
}

}  // namespace

size_t align_refine_bytes(int M, int rounds) {
    const size_t tiles = (size_t)verify_pad(M) / kVerifyTile;
    return tiles * (r3::kSums1 + r3::kSums2) * sizeof(double) + kM * sizeof(double) +
           (size_t)rounds * kM * sizeof(double) + (size_t)(kStWords + 1 + rounds) * sizeof(int);
}

void launch_align_refine(int M, bool normals, int rounds, double tau2, double minCos, const double* planes,
                         const int* count, const int* best, double* model, void* work, int* flag, uint8_t* mask,
                         int** roundCounts, double** roundModels, int** adopted, hipStream_t s) {
    const int tiles = verify_pad(M) / kVerifyTile;
    double* p1 = (double*)work;
    double* p2 = p1 + (size_t)tiles * r3::kSums1;
    double* cand = p2 + (size_t)tiles * r3::kSums2;
    double* rm = cand + kM;
    int* st = (int*)(rm + (size_t)rounds * kM);
    int* rc = st + kStWords;
    align_refine_init_kernel<<<1, 64, 0, s>>>(best, count, rounds, st, rc, rm);
    if (normals)
        refine_rounds<true>(M, rounds, tau2, minCos, planes, model, p1, p2, cand, st, rc, rm, best, flag, mask, s);
    else
        refine_rounds<false>(M, rounds, tau2, minCos, planes, model, p1, p2, cand, st, rc, rm, best, flag, mask, s);
    *roundCounts = rc;
    *roundModels = rm;
    *adopted = st + kStAdopted;
}

void launch_align(const AlignIn& in, const fm3d_dmatch* matches, int M, int H, unsigned long long seed, double tau2,
                  double minCos, int nCU, double* planes, double* models, int* count, int* best, double* model,
                  int* flag, uint8_t* mask, hipStream_t s, bool withMask) {
    const int Mpad = verify_pad(M);
    const bool normals = in.nrmA != nullptr;
    align_gather_kernel<<<(Mpad + 255) / 256, 256, 0, s>>>(in, matches, M, Mpad, planes);
    align_hypothesis_kernel<<<(H + kHypThreads - 1) / kHypThreads, kHypThreads, 0, s>>>(planes, M, Mpad, H, seed, models,
                                                                                      count);
    // hypotheses per workgroup: 64, halved while the grid has fewer than four workgroups per CU
    // (the chunks go to grid.y: at most 65535, which 64 per workgroup keeps for H <= kVerifyMaxHyps)
    const int tiles = Mpad / kVerifyTile;
    int hc = kScoreHyps;
    while (hc > 1 && (long long)tiles * ((H + hc - 1) / hc) < 4ll * nCU && (H + hc / 2 - 1) / (hc / 2) <= 65535)
        hc >>= 1;
    const dim3 grid(tiles, (H + hc - 1) / hc);
    if (normals) {
        align_score_kernel<true><<<grid, kScoreThreads, 0, s>>>(planes, Mpad, models, H, hc, tau2, minCos, count);
        align_argmax_kernel<<<1, 256, 0, s>>>(count, models, H, best, model);
        if (withMask)
            align_mask_kernel<true><<<(M + 255) / 256, 256, 0, s>>>(planes, M, Mpad, best, model, tau2, minCos, flag, mask);
    } else {
        align_score_kernel<false><<<grid, kScoreThreads, 0, s>>>(planes, Mpad, models, H, hc, tau2, minCos, count);
        align_argmax_kernel<<<1, 256, 0, s>>>(count, models, H, best, model);
        if (withMask)
            align_mask_kernel<false><<<(M + 255) / 256, 256, 0, s>>>(planes, M, Mpad, best, model, tau2, minCos, flag, mask);
    }
}

}  // namespace fm3d
