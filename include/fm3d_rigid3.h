/*
 * fm3d_rigid3.h -- the arithmetic of the 3D-3D alignment, host and device.
 *
 * A RANSAC fit of a rigid transform b = R a + t to matched 3D points: the counter-based sampler of
 * fm3d_epi8.h taking three matches, the three-point solve from the 3 x 3 cross matrix by OpenCV 2.4's
 * JacobiSVD (fm3d_cvsvd.h, fed as fm3d_epi8::svd_e feeds it) with the third singular pair completed by
 * cross products, the distance test with an optional test of the normals, and the refit of a model
 * on the pairs it accepts in two passes of sums in §3.1d's fixed order.  Everything is fp64 in the
 * operand order written here, compiled without FMA contraction, so the host library, the kernels of
 * fm3d_align.hip and the Python restatement (tests/align_pyref.py) give the same bits.  This header is
 * the only place the arithmetic lives.
 *
 * A model is twelve doubles: R row-major in m[0..8], t in m[9..11].
 */
#ifndef FM3D_RIGID3_H
#define FM3D_RIGID3_H

#include <float.h>
#include <math.h>
#include <stdint.h>

#include "fm3d_epi8.h"

namespace fm3d_rigid3 {

constexpr int kModel = 12;         // doubles of a model
constexpr int kSums1 = 7;          // the first pass: the sums of a (3), of b (3) and the count
constexpr int kSums2 = 9;          // the second pass: the centred cross sums, row-major
constexpr int kTile = fm3d_epi8::kRefitTile;    // slots of one summation tile (the scoring kernel's tile)
constexpr int kLanes = fm3d_epi8::kRefitLanes;  // leaves of a tile's tree: slot k * 256 + t belongs to leaf t
constexpr int kMaxIters = fm3d_epi8::kRefitMaxIters;

// the first three distinct draws of hypothesis h (fm3d_epi8::draw, a = 0 .. 63), in their order; false
// when 64 attempts give fewer (M < 3 always)
FM3D_CVSVD_HD bool sample3(uint64_t seed, uint32_t h, uint32_t M, int idx[3]) {
    int n = 0;
    idx[0] = idx[1] = idx[2] = -1;
    if (M < 3) return false;
    for (int a = 0; a < fm3d_epi8::kAttempts && n < 3; a++) {
        const int v = (int)fm3d_epi8::draw(seed, h, a, M);
        if (v != idx[0] && v != idx[1] && v != idx[2]) {
            // idx[n] = v with n a run-time index: a select per slot keeps idx in registers
#pragma unroll
            for (int k = 0; k < 3; k++) idx[k] = k == n ? v : idx[k];
            n++;
        }
    }
    return n == 3;
}

FM3D_CVSVD_HD bool finite(double v) { return fabs(v) <= DBL_MAX; }

FM3D_CVSVD_HD void zero_model(double m[kModel]) {
#pragma unroll
    for (int k = 0; k < kModel; k++) m[k] = 0.;
}

// R x for the row-major R of a model
FM3D_CVSVD_HD double rot_row(const double* m, int k, double x, double y, double z) {
    return (m[3 * k] * x + m[3 * k + 1] * y) + m[3 * k + 2] * z;
}

// The model from the cross matrix H[r][c] = sum (a - ca)[r] (b - cb)[c] (row-major) and the two
// centroids.  H = U S V^T by fm3d_epi8::svd_e: u_0, u_1, v_0, v_1 of the two leading pairs; the third
// pair is u_2 = u_0 x u_1, v_2 = v_0 x v_1, so both bases are right-handed and R = V U^T is proper:
//   R[r][c] = (v_0[r] u_0[c] + v_1[r] u_1[c]) + v_2[r] u_2[c],   t[r] = cb[r] - rot_row(R, r, ca).
// Invalid (false, the zero model): a non-finite entry of H (tested before the SVD), W[1] <= DBL_MIN,
// or a non-finite entry among the twelve.
FM3D_CVSVD_HD bool rigid_solve(const double H[9], const double ca[3], const double cb[3], double m[kModel]) {
    bool ok = true;
#pragma unroll
    for (int k = 0; k < 9; k++) ok = ok && finite(H[k]);
    double u[2][3], v[2][3], W[3], u2[3], v2[3];
    ok = ok && fm3d_epi8::svd_e(H, u, v, W);
    if (ok) {
        fm3d_epi8::cross3(u[0], u[1], u2);
        fm3d_epi8::cross3(v[0], v[1], v2);
#pragma unroll
        for (int r = 0; r < 3; r++)
#pragma unroll
            for (int c = 0; c < 3; c++) m[r * 3 + c] = (v[0][r] * u[0][c] + v[1][r] * u[1][c]) + v2[r] * u2[c];
#pragma unroll
        for (int r = 0; r < 3; r++) m[9 + r] = cb[r] - rot_row(m, r, ca[0], ca[1], ca[2]);
#pragma unroll
        for (int k = 0; k < kModel; k++) ok = ok && finite(m[k]);
    }
    if (!ok) zero_model(m);
    return ok;
}

// the minimal solve: a, b the three sampled pairs (a[k], b[k]: x, y, z).  Centroids
// ca = ((a_0 + a_1) + a_2) / 3; H from +0.0 in k order.
FM3D_CVSVD_HD bool rigid_from3(const double a[3][3], const double b[3][3], double m[kModel]) {
    double ca[3], cb[3], H[9];
#pragma unroll
    for (int r = 0; r < 3; r++) {
        ca[r] = ((a[0][r] + a[1][r]) + a[2][r]) / 3.;
        cb[r] = ((b[0][r] + b[1][r]) + b[2][r]) / 3.;
    }
#pragma unroll
    for (int r = 0; r < 3; r++)
#pragma unroll
        for (int c = 0; c < 3; c++) {
            double s = 0.;
#pragma unroll
            for (int k = 0; k < 3; k++) s = s + (a[k][r] - ca[r]) * (b[k][c] - cb[c]);
            H[r * 3 + c] = s;
        }
    return rigid_solve(H, ca, cb, m);
}

// the distance test: |R a + t - b|^2 <= tau2 (a NaN fails)
FM3D_CVSVD_HD bool inlier(const double* m, double ax, double ay, double az, double bx, double by, double bz,
                          double tau2) {
    const double d0 = (rot_row(m, 0, ax, ay, az) + m[9]) - bx;
    const double d1 = (rot_row(m, 1, ax, ay, az) + m[10]) - by;
    const double d2 = (rot_row(m, 2, ax, ay, az) + m[11]) - bz;
    return (d0 * d0 + d1 * d1) + d2 * d2 <= tau2;
}

// the test of the normals: (R n_a) . n_b >= minCos (a NaN fails)
FM3D_CVSVD_HD bool normal_ok(const double* m, double nax, double nay, double naz, double nbx, double nby, double nbz,
                             double minCos) {
    const double r0 = rot_row(m, 0, nax, nay, naz), r1 = rot_row(m, 1, nax, nay, naz), r2 = rot_row(m, 2, nax, nay, naz);
    return (r0 * nbx + r1 * nby) + r2 * nbz >= minCos;
}

// both tests, both evaluated: no branch per pair in the scoring loop
FM3D_CVSVD_HD bool inlier_n(const double* m, double ax, double ay, double az, double bx, double by, double bz,
                            double nax, double nay, double naz, double nbx, double nby, double nbz, double tau2,
                            double minCos) {
    const int near = inlier(m, ax, ay, az, bx, by, bz, tau2), facing = normal_ok(m, nax, nay, naz, nbx, nby, nbz, minCos);
    return (near & facing) != 0;
}

// ---------------- the refit on the accepted pairs ("Refit") ----------------

// a slot's value in a sum: v when the pair is in, +0.0 otherwise (a select: a NaN adds nothing)
FM3D_CVSVD_HD double slot(bool in, double v) { return in ? v : 0.; }

// the centroids from the first pass's sums S1 = (sum a, sum b, count)
FM3D_CVSVD_HD void centroids(const double S1[kSums1], double ca[3], double cb[3]) {
    const double n = S1[6];
#pragma unroll
    for (int r = 0; r < 3; r++) {
        ca[r] = S1[r] / n;
        cb[r] = S1[3 + r] / n;
    }
}

// a slot's value in the second pass, entry (r, c): the centred product
FM3D_CVSVD_HD double slot2(bool in, double ar, double car, double bc, double cbc) {
    return in ? (ar - car) * (bc - cbc) : 0.;
}

// the refit from the two passes' sums; invalid (false, the zero model): a non-finite sum, fewer than
// three pairs in, or rigid_solve's reasons
FM3D_CVSVD_HD bool refit_solve(const double S1[kSums1], const double S2[kSums2], double m[kModel]) {
    bool ok = true;
#pragma unroll
    for (int k = 0; k < kSums1; k++) ok = ok && finite(S1[k]);
    ok = ok && S1[6] >= 3.;
    if (!ok) {
        zero_model(m);
        return false;
    }
    double ca[3], cb[3];
    centroids(S1, ca, cb);
    return rigid_solve(S2, ca, cb, m);
}

}  // namespace fm3d_rigid3

#endif /* FM3D_RIGID3_H */
