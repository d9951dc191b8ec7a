// fm3d_verify.hip -- geometric verification of matches: a RANSAC fit of the
// essential matrix, every hypothesis scored against every match, the rounds of a least-squares
// refit of the best model on its inliers, and the final model's pose candidates with their cheirality
// votes.  The arithmetic is include/fm3d_epi8.h's (shared with the
// host entry points and restated in tests/verify_pyref.py and tests/verify_refit_pyref.py); the
// kernels only distribute it.
#include <hip/hip_runtime.h>

#include "fm3d_epi8.h"
#include "fm3d_kernels.h"

namespace fm3d {
namespace {

constexpr int kHypThreads = 64;     // hypotheses per workgroup: 64 x 576 B of LDS
constexpr int kScoreThreads = 256;
constexpr int kScorePer = 4;        // matches a lane keeps in registers
constexpr int kScoreHyps = 64;      // most hypotheses one workgroup scores
static_assert(kScoreThreads * kScorePer == kVerifyTile, "a scoring workgroup covers one tile of matches");

// M: the match count, or its bound when Mdev holds the count on the device (the device-count forms:
// every grid and the planes' stride Mpad are sized by the bound).  One address for every thread, so
// a scalar load; a count outside [0, M] is clamped, so nothing is indexed past the bound.
__device__ __forceinline__ int dev_matches(const int* __restrict__ Mdev, int M) {
    if (!Mdev) return M;
    const int d = *Mdev;
    return d < 0 ? 0 : (d < M ? d : M);
}

// a tile of 1,024 slots that lies entirely past the device count holds only NaN: it adds nothing to a
// count, and the solve never reads its partials.  The same for every thread of the workgroup.
__device__ __forceinline__ bool tile_past_count(const int* __restrict__ Mdev, int Mpad) {
    return Mdev && (long long)blockIdx.x * kVerifyTile >= dev_matches(Mdev, Mpad);
}

// xy: four planes of Mpad doubles (x1, y1, x2, y2); the pad -- every slot from the count to Mpad, whole
// tiles of it with a device count -- holds NaN, which no model accepts
__global__ __launch_bounds__(256) void verify_coords_kernel(Camera cam, const fm3d_point2f* __restrict__ kp1,
                                                            const fm3d_point2f* __restrict__ kp2,
                                                            const fm3d_dmatch* __restrict__ matches, int M,
                                                            const int* __restrict__ Mdev, int Mpad,
                                                            double* __restrict__ xy) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= Mpad) return;
    M = dev_matches(Mdev, M);
    double x1, y1, x2, y2;
    x1 = y1 = x2 = y2 = __builtin_nan("");
    if (i < M) {
        const fm3d_dmatch m = matches[i];
        const fm3d_point2f a = kp1[m.queryIdx], b = kp2[m.trainIdx];
        undistort1(cam, (double)a.x, (double)a.y, x1, y1);
        undistort1(cam, (double)b.x, (double)b.y, x2, y2);
    }
    xy[i] = x1;
    xy[(size_t)Mpad + i] = y1;
    xy[(size_t)2 * Mpad + i] = x2;
    xy[(size_t)3 * Mpad + i] = y2;
}

// a thread's 8 x 9 system in LDS, entry (r, c) of thread t at word (r * 9 + c) * 64 + t: the pivots
// index it at run time (a register array would go to scratch), and the lanes of a wave never share
// a bank
struct LdsMat {
    double* p;
    __device__ double& operator()(int r, int c) { return p[(r * 9 + c) * kHypThreads]; }
};

__global__ __launch_bounds__(kHypThreads) void verify_hypothesis_kernel(const double* __restrict__ xy, int M,
                                                                        const int* __restrict__ Mdev, int Mpad,
                                                                        int H, unsigned long long seed,
                                                                        double* __restrict__ models,
                                                                        int* __restrict__ count) {
    __shared__ double sA[72 * kHypThreads];
    const int h = blockIdx.x * kHypThreads + threadIdx.x;
    if (h >= H) return;
    M = dev_matches(Mdev, M);  // fewer than 8: no sample exists, every hypothesis is invalid
    LdsMat A{sA + threadIdx.x};
    int idx[8];
    double E[9], e[9];
    bool ok = fm3d_epi8::sample8(seed, (uint32_t)h, (uint32_t)M, idx);
    if (ok) {
#pragma unroll
        for (int k = 0; k < 8; k++) {
            const int i = idx[k];
            fm3d_epi8::set_row(A, k, xy[i], xy[(size_t)Mpad + i], xy[(size_t)2 * Mpad + i], xy[(size_t)3 * Mpad + i]);
        }
        ok = fm3d_epi8::model8(A, E, e);
    } else {
#pragma unroll
        for (int k = 0; k < 9; k++) E[k] = 0.;
    }
#pragma unroll
    for (int k = 0; k < 9; k++) models[(size_t)h * 9 + k] = E[k];
    count[h] = ok ? 0 : -1;
}

// Workgroup (bx, by): the tile of 1024 matches bx against the hc hypotheses from by * hc.  A lane
// keeps four matches' coordinates; a hypothesis's nine coefficients have one address per wave (scalar
// loads); a wave counts with ballots, the workgroup adds its four waves in LDS, and one atomicAdd per
// (workgroup, hypothesis) with a non-zero count goes to count[h] -- integers, exact in any order.  An
// invalid hypothesis is the zero model: den == 0 accepts nothing, its count stays -1.
__global__ __launch_bounds__(kScoreThreads) void verify_score_kernel(const double* __restrict__ xy,
                                                                     const int* __restrict__ Mdev, int Mpad,
                                                                     const double* __restrict__ models, int H, int hc,
                                                                     double tau2, int* __restrict__ count) {
    __shared__ int sCnt[kScoreThreads / 64][kScoreHyps];
    if (tile_past_count(Mdev, Mpad)) return;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    double x1[kScorePer], y1[kScorePer], x2[kScorePer], y2[kScorePer];
#pragma unroll
    for (int k = 0; k < kScorePer; k++) {
        const size_t i = (size_t)blockIdx.x * kVerifyTile + k * kScoreThreads + tid;  // < Mpad
        x1[k] = xy[i];
        y1[k] = xy[(size_t)Mpad + i];
        x2[k] = xy[(size_t)2 * Mpad + i];
        y2[k] = xy[(size_t)3 * Mpad + i];
    }
    const int h0 = blockIdx.y * hc;
    const int nh = min(hc, H - h0);
    for (int j = 0; j < nh; j++) {
        const double* __restrict__ m = models + (size_t)(h0 + j) * 9;
        double E[9];
#pragma unroll
        for (int k = 0; k < 9; k++) E[k] = m[k];
        int c = 0;
#pragma unroll
        for (int k = 0; k < kScorePer; k++)
            c += __popcll(__ballot(fm3d_epi8::inlier(E, x1[k], y1[k], x2[k], y2[k], tau2)));
        if (lane == 0) sCnt[wave][j] = c;
    }
    __syncthreads();
    if (tid < nh) {
        int s = 0;
#pragma unroll
        for (int w = 0; w < kScoreThreads / 64; w++) s += sCnt[w][tid];
        if (s) atomicAdd(&count[h0 + tid], s);
    }
}

// the largest count, the lowest h on ties; no valid hypothesis: best = -1 and a zero E
__global__ __launch_bounds__(256) void verify_argmax_kernel(const int* __restrict__ count,
                                                            const double* __restrict__ models, int H,
                                                            int* __restrict__ best, double* __restrict__ E) {
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
    if (tid < 9) {
        const bool any = sC[0] >= 0;
        E[tid] = any ? models[(size_t)sH[0] * 9 + tid] : 0.;
        if (tid == 0) *best = any ? sH[0] : -1;
    }
}

__global__ __launch_bounds__(256) void verify_mask_kernel(const double* __restrict__ xy, int M,
                                                          const int* __restrict__ Mdev, int Mpad,
                                                          const int* __restrict__ best, const double* __restrict__ Eb,
                                                          double tau2, int* __restrict__ flag,
                                                          uint8_t* __restrict__ mask) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= dev_matches(Mdev, M)) return;
    double E[9];
#pragma unroll
    for (int k = 0; k < 9; k++) E[k] = Eb[k];
    const bool in = *best >= 0 &&
                    fm3d_epi8::inlier(E, xy[i], xy[(size_t)Mpad + i], xy[(size_t)2 * Mpad + i], xy[(size_t)3 * Mpad + i], tau2);
    flag[i] = in ? 1 : 0;
    mask[i] = in ? 1 : 0;
}

// ---------------- refinement: the refit on the inliers, round by round ----------------
// st: the rounds' state on the device.  Every kernel of a round tests st[kStDone] first.
enum { kStDone = 0, kStCount = 1, kStValid = 2, kStCand = 3, kStAdopted = 4, kStWords = 8 };

static_assert(kScoreThreads == fm3d_epi8::kRefitLanes && kVerifyTile == fm3d_epi8::kRefitTile,
              "the normal matrix is summed over the scoring kernel's tile");

// c_0 and the flags: no best model leaves every round undone
__global__ __launch_bounds__(64) void verify_refine_init_kernel(const int* __restrict__ best,
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
    for (int k = tid; k < rounds * 9; k += 64) roundModels[k] = 0.;
}

// Workgroup bx: the 45 sums of tile bx under the current model.  A lane holds the four slots
// k * 256 + tid, evaluates the predicate itself and forms leaf4 of their products; the wave's 64
// leaves go through an xor butterfly (strides 1 .. 32: the balanced tree's bits in every lane, IEEE
// addition being commutative), the four waves through LDS as (w0 + w1) + (w2 + w3).
__global__ __launch_bounds__(kScoreThreads) void verify_normal_kernel(const double* __restrict__ xy,
                                                                      const int* __restrict__ Mdev, int Mpad,
                                                                      const double* __restrict__ Ecur, double tau2,
                                                                      const int* __restrict__ st,
                                                                      double* __restrict__ partial) {
    __shared__ double sW[kScoreThreads / 64][fm3d_epi8::kPairs];
    if (st[kStDone]) return;
    if (tile_past_count(Mdev, Mpad)) return;  // its partials stay what they were: the solve stops before them
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    double E[9];
#pragma unroll
    for (int k = 0; k < 9; k++) E[k] = Ecur[k];
    static_assert(kScorePer == 4, "leaf4 adds a lane's four slots");
    double a[kScorePer][9];
    bool in[kScorePer];
#pragma unroll
    for (int k = 0; k < kScorePer; k++) {
        const size_t i = (size_t)blockIdx.x * kVerifyTile + k * kScoreThreads + tid;  // < Mpad
        const double x1 = xy[i], y1 = xy[(size_t)Mpad + i], x2 = xy[(size_t)2 * Mpad + i], y2 = xy[(size_t)3 * Mpad + i];
        in[k] = fm3d_epi8::inlier(E, x1, y1, x2, y2, tau2);
        fm3d_epi8::row9(x1, y1, x2, y2, a[k]);
    }
    int j = 0;
#pragma unroll
    for (int r = 0; r < 9; r++)
#pragma unroll
        for (int c = r; c < 9; c++, j++) {
            double s = fm3d_epi8::leaf4(fm3d_epi8::slot(in[0], a[0], r, c), fm3d_epi8::slot(in[1], a[1], r, c),
                                        fm3d_epi8::slot(in[2], a[2], r, c), fm3d_epi8::slot(in[3], a[3], r, c));
#pragma unroll
            for (int o = 1; o < 64; o <<= 1) s = s + __shfl_xor(s, o);
            if (lane == 0) sW[wave][j] = s;
        }
    __syncthreads();
    if (tid < fm3d_epi8::kPairs)
        partial[(size_t)blockIdx.x * fm3d_epi8::kPairs + tid] = (sW[0][tid] + sW[1][tid]) + (sW[2][tid] + sW[3][tid]);
}

// S and V of the solve in LDS: the rotations index them at run time
struct LdsMat99 {
    double* p;
    __device__ double& operator()(int r, int c) { return p[r * 9 + c]; }
};

// the solve's rows over the lanes of its one wave: row k on lane k (the lanes from 9 on only follow)
struct WaveTeam {
    int lane;
    __device__ int first() const { return lane; }
    __device__ int step() const { return 64; }
    __device__ void sync() const { __syncthreads(); }
};

// One workgroup of one wave: 45 threads add the tile partials in tile order from +0.0 -- with a device
// count only the ceil(count / 1024) leading tiles', the ones the normal kernel wrote for this pair, so
// the sums are those of a run sized by the count and no older pair's partial is read; every lane runs
// the Jacobi iteration on the S and V in LDS, lane k updating row k of a rotation; thread 0 projects.
// cand: E' (zero when invalid); st: the valid flag and the candidate's count, 0 for the count kernel
// to add to, -1 when there is nothing to count.
__global__ __launch_bounds__(64) void verify_solve_kernel(const double* __restrict__ partial, int tiles,
                                                          const int* __restrict__ Mdev, int* __restrict__ st,
                                                          double* __restrict__ cand) {
    __shared__ double sN[fm3d_epi8::kPairs], sS[81], sV[81], sE[9];
    __shared__ int sOk;
    const int tid = threadIdx.x;
    if (st[kStDone]) return;
    if (Mdev) tiles = (dev_matches(Mdev, tiles * kVerifyTile) + kVerifyTile - 1) / kVerifyTile;
    if (tid < fm3d_epi8::kPairs) {
        double s = 0.;
        for (int t = 0; t < tiles; t++) s = s + partial[(size_t)t * fm3d_epi8::kPairs + tid];
        sN[tid] = s;
    }
    __syncthreads();
    LdsMat99 S{sS}, V{sV};
    if (tid == 0) sOk = fm3d_epi8::refit_load(sN, S) ? 1 : 0;
    __syncthreads();
    const bool ok = sOk != 0;  // the same in every lane: the barriers below are met by all or none
    if (ok) fm3d_epi8::jacobi_null9(S, V, sE, WaveTeam{tid});
    if (tid == 0) {
        double E[9];
        const bool valid = fm3d_epi8::refit_project(ok, sE, E);
#pragma unroll
        for (int k = 0; k < 9; k++) cand[k] = E[k];
        st[kStValid] = valid ? 1 : 0;
        st[kStCand] = valid ? 0 : -1;
    }
}

// c' of a valid E': verify_score_kernel's count for one model, behind the rounds' flags (integers:
// the atomicAdd per workgroup is exact in any order)
__global__ __launch_bounds__(kScoreThreads) void verify_count_kernel(const double* __restrict__ xy,
                                                                     const int* __restrict__ Mdev, int Mpad,
                                                                     const double* __restrict__ cand, double tau2,
                                                                     int* __restrict__ st) {
    __shared__ int sCnt[kScoreThreads / 64];
    if (st[kStDone] || !st[kStValid]) return;
    if (tile_past_count(Mdev, Mpad)) return;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    double E[9];
#pragma unroll
    for (int k = 0; k < 9; k++) E[k] = cand[k];
    int c = 0;
#pragma unroll
    for (int k = 0; k < kScorePer; k++) {
        const size_t i = (size_t)blockIdx.x * kVerifyTile + k * kScoreThreads + tid;  // < Mpad
        c += __popcll(__ballot(
            fm3d_epi8::inlier(E, xy[i], xy[(size_t)Mpad + i], xy[(size_t)2 * Mpad + i], xy[(size_t)3 * Mpad + i], tau2)));
    }
    if (lane == 0) sCnt[wave] = c;
    __syncthreads();
    if (tid == 0) {
        const int n = (sCnt[0] + sCnt[1]) + (sCnt[2] + sCnt[3]);
        if (n) atomicAdd(&st[kStCand], n);
    }
}

// The rule of round r: adopt E' iff it is valid and keeps at least as many matches; otherwise the
// current model is final and every later round is skipped.
__global__ __launch_bounds__(64) void verify_adopt_kernel(int r, int* __restrict__ st, const double* __restrict__ cand,
                                                          double* __restrict__ Ecur, int* __restrict__ roundCounts,
                                                          double* __restrict__ roundModels) {
    const int tid = threadIdx.x;
    if (st[kStDone]) return;
    const int valid = st[kStValid], cc = st[kStCand], cur = st[kStCount];
    const bool adopt = valid && cc >= cur;
    __syncthreads();  // every thread has read the state before thread 0 changes it
    if (tid < 9) {
        const double e = cand[tid];
        roundModels[r * 9 + tid] = e;
        if (adopt) Ecur[tid] = e;
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

// ---------------- the pose of the final model (fm3d_pipeline_run_verified) ----------------
// pv: the pose stage's integers -- the valid flag, then the four candidates' votes
enum { kPvValid = 0, kPvVotes = 1 };

// One wave behind the final model: thread 0 builds the two rotations and u_2 of E (cand:
// fm3d_epi8::kPoseDoubles doubles, zero when there is none) and the valid flag; the votes start at 0.
__global__ __launch_bounds__(64) void verify_pose_candidates_kernel(const int* __restrict__ best,
                                                                    const double* __restrict__ Eb,
                                                                    double* __restrict__ cand, int* __restrict__ pv) {
    if (threadIdx.x != 0) return;
    double E[9], R[2][9], u2[3];
#pragma unroll
    for (int k = 0; k < 9; k++) E[k] = Eb[k];
    const bool ok = *best >= 0 && fm3d_epi8::pose_candidates(E, R, u2);
#pragma unroll
    for (int k = 0; k < 9; k++) {
        cand[k] = ok ? R[0][k] : 0.;
        cand[9 + k] = ok ? R[1][k] : 0.;
    }
#pragma unroll
    for (int k = 0; k < 3; k++) cand[18 + k] = ok ? u2[k] : 0.;
    pv[kPvValid] = ok ? 1 : 0;
#pragma unroll
    for (int k = 0; k < 4; k++) pv[kPvVotes + k] = 0;
}

// Workgroup bx: the votes of tile bx, in verify_score_kernel's shape.  A lane keeps four slots'
// coordinates; a slot votes only when it is a match (i < M: the pad holds NaN and has no flag) that the
// final model accepts (flag).  The 21 candidate doubles have one address per wave (scalar loads); a
// wave counts with ballots, the four waves add in LDS, and one atomicAdd per (workgroup, candidate)
// with a non-zero count goes to the votes -- integers, exact in any order.
__global__ __launch_bounds__(kScoreThreads) void verify_pose_vote_kernel(const double* __restrict__ xy, int M, int Mpad,
                                                                         const int* __restrict__ flag,
                                                                         const double* __restrict__ cand,
                                                                         int* __restrict__ pv) {
    __shared__ int sCnt[kScoreThreads / 64][4];
    if (!pv[kPvValid]) return;  // the same word for every thread: all leave, or none
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    double x1[kScorePer], y1[kScorePer], x2[kScorePer], y2[kScorePer];
    bool in[kScorePer];
#pragma unroll
    for (int k = 0; k < kScorePer; k++) {
        const size_t i = (size_t)blockIdx.x * kVerifyTile + k * kScoreThreads + tid;  // < Mpad
        x1[k] = xy[i];
        y1[k] = xy[(size_t)Mpad + i];
        x2[k] = xy[(size_t)2 * Mpad + i];
        y2[k] = xy[(size_t)3 * Mpad + i];
        in[k] = i < (size_t)M && flag[i] != 0;
    }
    double R[2][9], u2[3];
#pragma unroll
    for (int k = 0; k < 9; k++) {
        R[0][k] = cand[k];
        R[1][k] = cand[9 + k];
    }
#pragma unroll
    for (int k = 0; k < 3; k++) u2[k] = cand[18 + k];
#pragma unroll
    for (int j = 0; j < 4; j++) {
        double t[3];
        fm3d_epi8::pose_direction(j, u2, t);
        int c = 0;
#pragma unroll
        for (int k = 0; k < kScorePer; k++)
            c += __popcll(__ballot(in[k] && fm3d_epi8::pose_vote(R[j >> 1], t, x1[k], y1[k], x2[k], y2[k])));
        if (lane == 0) sCnt[wave][j] = c;
    }
    __syncthreads();
    if (tid < 4) {
        int s = 0;
#pragma unroll
        for (int w = 0; w < kScoreThreads / 64; w++) s += sCnt[w][tid];
        if (s) atomicAdd(&pv[kPvVotes + tid], s);
    }
}

// What the host reads of a verification it never waited for, stored to page-locked memory (host: a
// device pointer to it) with system-scope stores, as the DLT kernel stores its counts: a caller that
// waits for the stream reads it without a copy launch.  One wave; Mdev holds the match stage's count,
// verified the compaction's.
__global__ __launch_bounds__(64) void verify_report_kernel(const int* __restrict__ Mdev, const int* __restrict__ best,
                                                           const double* __restrict__ E,
                                                           const int* __restrict__ adopted,
                                                           const int* __restrict__ verified, VerifySmall* host) {
    const int tid = threadIdx.x;
    if (tid < 9) __hip_atomic_store(&host->E[tid], E[tid], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
    if (tid == 0) {
        __hip_atomic_store(&host->matches, *Mdev, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
        __hip_atomic_store(&host->verified, *verified, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
        __hip_atomic_store(&host->best, *best, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
        __hip_atomic_store(&host->adopted, adopted ? *adopted : 0, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
    }
}

}  // namespace

void launch_verify_report(const int* Mdev, const int* best, const double* E, const int* adopted, const int* verified,
                          VerifySmall* host, hipStream_t s) {
    verify_report_kernel<<<1, 64, 0, s>>>(Mdev, best, E, adopted, verified, host);
}

size_t verify_pose_bytes() { return fm3d_epi8::kPoseDoubles * sizeof(double) + 8 * sizeof(int); }

void launch_verify_pose(int M, const double* xy, const int* flag, const int* best, const double* E, void* work,
                        double** cand, int** valid, int** votes, hipStream_t s) {
    const int Mpad = verify_pad(M);
    double* cd = (double*)work;
    int* pv = (int*)(cd + fm3d_epi8::kPoseDoubles);
    verify_pose_candidates_kernel<<<1, 64, 0, s>>>(best, E, cd, pv);
    verify_pose_vote_kernel<<<Mpad / kVerifyTile, kScoreThreads, 0, s>>>(xy, M, Mpad, flag, cd, pv);
    *cand = cd;
    *valid = pv + kPvValid;
    *votes = pv + kPvVotes;
}

size_t verify_refine_bytes(int M, int rounds) {
    const size_t tiles = (size_t)verify_pad(M) / kVerifyTile;
    return tiles * fm3d_epi8::kPairs * sizeof(double) + 9 * sizeof(double) + (size_t)rounds * 9 * sizeof(double) +
           (size_t)(kStWords + 1 + rounds) * sizeof(int);
}

void launch_verify_refine(int M, int rounds, double tau2, const double* xy, const int* count, const int* best,
                          double* E, void* work, int* flag, uint8_t* mask, int** roundCounts, double** roundModels,
                          int** adopted, hipStream_t s, const int* Mdev) {
    const int Mpad = verify_pad(M), tiles = Mpad / kVerifyTile;
    double* partial = (double*)work;
    double* cand = partial + (size_t)tiles * fm3d_epi8::kPairs;
    double* rm = cand + 9;
    int* st = (int*)(rm + (size_t)rounds * 9);
    int* rc = st + kStWords;
    verify_refine_init_kernel<<<1, 64, 0, s>>>(best, count, rounds, st, rc, rm);
    for (int r = 0; r < rounds; r++) {
        verify_normal_kernel<<<tiles, kScoreThreads, 0, s>>>(xy, Mdev, Mpad, E, tau2, st, partial);
        verify_solve_kernel<<<1, 64, 0, s>>>(partial, tiles, Mdev, st, cand);
        verify_count_kernel<<<tiles, kScoreThreads, 0, s>>>(xy, Mdev, Mpad, cand, tau2, st);
        verify_adopt_kernel<<<1, 64, 0, s>>>(r, st, cand, E, rc, rm);
    }
    verify_mask_kernel<<<(M + 255) / 256, 256, 0, s>>>(xy, M, Mdev, Mpad, best, E, tau2, flag, mask);
    *roundCounts = rc;
    *roundModels = rm;
    *adopted = st + kStAdopted;
}

int verify_pad(int M) { return (int)(((long long)M + kVerifyTile - 1) / kVerifyTile * kVerifyTile); }

void launch_verify(const Camera& cam, const fm3d_point2f* kp1, const fm3d_point2f* kp2, const fm3d_dmatch* matches,
                   int M, int H, unsigned long long seed, double tau2, int nCU, double* xy, double* models, int* count,
                   int* best, double* E, int* flag, uint8_t* mask, hipStream_t s, bool withMask, const int* Mdev) {
    const int Mpad = verify_pad(M);
    verify_coords_kernel<<<(Mpad + 255) / 256, 256, 0, s>>>(cam, kp1, kp2, matches, M, Mdev, Mpad, xy);
    verify_hypothesis_kernel<<<(H + kHypThreads - 1) / kHypThreads, kHypThreads, 0, s>>>(xy, M, Mdev, Mpad, H, seed,
                                                                                       models, count);
    // hypotheses per workgroup: 64, halved while the grid has fewer than four workgroups per CU
    const int tiles = Mpad / kVerifyTile;
    // (the chunks go to grid.y: at most 65535, which 64 per workgroup keeps for H <= kVerifyMaxHyps)
    int hc = kScoreHyps;
    while (hc > 1 && (long long)tiles * ((H + hc - 1) / hc) < 4ll * nCU && (H + hc / 2 - 1) / (hc / 2) <= 65535)
        hc >>= 1;
    verify_score_kernel<<<dim3(tiles, (H + hc - 1) / hc), kScoreThreads, 0, s>>>(xy, Mdev, Mpad, models, H, hc, tau2,
                                                                                 count);
    verify_argmax_kernel<<<1, 256, 0, s>>>(count, models, H, best, E);
    if (withMask) verify_mask_kernel<<<(M + 255) / 256, 256, 0, s>>>(xy, M, Mdev, Mpad, best, E, tau2, flag, mask);
}

}  // namespace fm3d
