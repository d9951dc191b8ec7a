// fm3d_verify.hip -- geometric verification of matches: a RANSAC fit of the
// essential matrix, every hypothesis scored against every match.  The arithmetic is
// include/fm3d_epi8.h's (shared with the host entry points and restated in tests/verify_pyref.py);
// the kernels only distribute it.
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

// xy: four planes of Mpad doubles (x1, y1, x2, y2); the pad holds NaN, which no model accepts
__global__ __launch_bounds__(256) void verify_coords_kernel(Camera cam, const fm3d_point2f* __restrict__ kp1,
                                                            const fm3d_point2f* __restrict__ kp2,
                                                            const fm3d_dmatch* __restrict__ matches, int M, int Mpad,
                                                            double* __restrict__ xy) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= Mpad) return;
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

__global__ __launch_bounds__(kHypThreads) void verify_hypothesis_kernel(const double* __restrict__ xy, int M, int Mpad,
                                                                        int H, unsigned long long seed,
                                                                        double* __restrict__ models,
                                                                        int* __restrict__ count) {
    __shared__ double sA[72 * kHypThreads];
    const int h = blockIdx.x * kHypThreads + threadIdx.x;
    if (h >= H) return;
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
__global__ __launch_bounds__(kScoreThreads) void verify_score_kernel(const double* __restrict__ xy, int Mpad,
                                                                     const double* __restrict__ models, int H, int hc,
                                                                     double tau2, int* __restrict__ count) {
    __shared__ int sCnt[kScoreThreads / 64][kScoreHyps];
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

__global__ __launch_bounds__(256) void verify_mask_kernel(const double* __restrict__ xy, int M, int Mpad,
                                                          const int* __restrict__ best, const double* __restrict__ Eb,
                                                          double tau2, int* __restrict__ flag,
                                                          uint8_t* __restrict__ mask) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= M) return;
    double E[9];
#pragma unroll
    for (int k = 0; k < 9; k++) E[k] = Eb[k];
    const bool in = *best >= 0 &&
                    fm3d_epi8::inlier(E, xy[i], xy[(size_t)Mpad + i], xy[(size_t)2 * Mpad + i], xy[(size_t)3 * Mpad + i], tau2);
    flag[i] = in ? 1 : 0;
    mask[i] = in ? 1 : 0;
}

}  // namespace

int verify_pad(int M) { return (int)(((long long)M + kVerifyTile - 1) / kVerifyTile * kVerifyTile); }

void launch_verify(const Camera& cam, const fm3d_point2f* kp1, const fm3d_point2f* kp2, const fm3d_dmatch* matches,
                   int M, int H, unsigned long long seed, double tau2, int nCU, double* xy, double* models, int* count,
                   int* best, double* E, int* flag, uint8_t* mask, hipStream_t s) {
    const int Mpad = verify_pad(M);
    verify_coords_kernel<<<(Mpad + 255) / 256, 256, 0, s>>>(cam, kp1, kp2, matches, M, Mpad, xy);
    verify_hypothesis_kernel<<<(H + kHypThreads - 1) / kHypThreads, kHypThreads, 0, s>>>(xy, M, Mpad, H, seed, models,
                                                                                       count);
    // hypotheses per workgroup: 64, halved while the grid has fewer than four workgroups per CU
    const int tiles = Mpad / kVerifyTile;
    // (the chunks go to grid.y: at most 65535, which 64 per workgroup keeps for H <= kVerifyMaxHyps)
    int hc = kScoreHyps;
    while (hc > 1 && (long long)tiles * ((H + hc - 1) / hc) < 4ll * nCU && (H + hc / 2 - 1) / (hc / 2) <= 65535)
        hc >>= 1;
    verify_score_kernel<<<dim3(tiles, (H + hc - 1) / hc), kScoreThreads, 0, s>>>(xy, Mpad, models, H, hc, tau2, count);
    verify_argmax_kernel<<<1, 256, 0, s>>>(count, models, H, best, E);
    verify_mask_kernel<<<(M + 255) / 256, 256, 0, s>>>(xy, M, Mpad, best, E, tau2, flag, mask);
}

}  // namespace fm3d
