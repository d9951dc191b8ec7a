/*
 * fm3d_epi8.h -- the arithmetic of the geometric verification, host and device.
 *
 * A RANSAC fit of the essential matrix to matches: a counter-based sampler, the eight-point null
 * vector by Gauss-Jordan elimination with full pivoting, the projection onto the essential manifold
 * by OpenCV 2.4's JacobiSVD (fm3d_cvsvd.h) and the Sampson test without a division.  Everything is
 * fp64 in the operand order written here, compiled without FMA contraction, so the host library, the
 * kernels of fm3d_verify.hip and the numpy restatement (tests/verify_pyref.py) give the same bits.
 * The refit of a model on its own inliers follows: the 45 sums of the normal matrix in a fixed order,
 * a cyclic Jacobi eigen-iteration on the symmetric 9 x 9 and the same projection
 * (tests/verify_refit_pyref.py).  Last, the pose of a model: the four decompositions and one pair's
 * cheirality vote (verify_pyref.pose).  This header is the only place the arithmetic lives.
 */
#ifndef FM3D_EPI8_H
#define FM3D_EPI8_H

#include <float.h>
#include <math.h>
#include <stdint.h>

#include "fm3d_cvsvd.h"

namespace fm3d_epi8 {

constexpr int kAttempts = 64;  // draws per hypothesis

// draw a of hypothesis h: splitmix64's finaliser over a Weyl counter, then the top 32 bits scaled
// to [0, M) (M < 2^31)
FM3D_CVSVD_HD uint32_t draw(uint64_t seed, uint32_t h, int a, uint32_t M) {
    uint64_t z = seed + 0x9E3779B97F4A7C15ull * (1ull + 64ull * (uint64_t)h + (uint64_t)a);
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    z ^= z >> 31;
    return (uint32_t)(((z >> 32) * (uint64_t)M) >> 32);
}

// the first eight distinct draws of hypothesis h; false when 64 attempts give fewer (M < 8 always)
FM3D_CVSVD_HD bool sample8(uint64_t seed, uint32_t h, uint32_t M, int idx[8]) {
    int n = 0;
#pragma unroll
    for (int k = 0; k < 8; k++) idx[k] = -1;
    if (M < 8) return false;
    for (int a = 0; a < kAttempts && n < 8; a++) {
        const int v = (int)draw(seed, h, a, M);
        bool fresh = true;
#pragma unroll
        for (int k = 0; k < 8; k++) fresh = fresh && idx[k] != v;
        if (fresh) {
            // idx[n] = v with n a run-time index: a select per slot keeps idx in registers
#pragma unroll
            for (int k = 0; k < 8; k++) idx[k] = k == n ? v : idx[k];
            n++;
        }
    }
    return n == 8;
}

// the 8 x 9 system on the host: a plain array (the hypothesis kernel keeps its own in LDS)
struct Mat89 {
    double a[72];
    FM3D_CVSVD_HD double& operator()(int r, int c) { return a[r * 9 + c]; }
};

// row k of the system from the pair (x1, y1) <-> (x2, y2): e is the row-major E of x2^T E x1 = 0
template <typename Mat>
FM3D_CVSVD_HD void set_row(Mat& A, int k, double x1, double y1, double x2, double y2) {
    A(k, 0) = x2 * x1;
    A(k, 1) = x2 * y1;
    A(k, 2) = x2;
    A(k, 3) = y2 * x1;
    A(k, 4) = y2 * y1;
    A(k, 5) = y2;
    A(k, 6) = x1;
    A(k, 7) = y1;
    A(k, 8) = 1.;
}

// The unit null vector of the 8 x 9 system by Gauss-Jordan elimination with full pivoting (A is
// destroyed).  Step s: the pivot is the entry of largest magnitude in rows s..7 over the columns
// not yet chosen, the first met in row-then-column order on ties (a NaN is never larger); no pivot,
// a zero or a non-finite one: false.  Rows swapped, every other row reduced over all nine columns.
// x[free] = 1, x[c_s] = -A[s][free] / A[s][c_s] on the final A, scaled by 1 / sqrt(sum of squares in
// index order); a sum that is not finite: false.
template <typename Mat>
FM3D_CVSVD_HD bool null8(Mat& A, double e[9]) {
    int col[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    unsigned used = 0;
    for (int s = 0; s < 8; s++) {
        double best = -1.;
        int br = -1, bc = -1;
        for (int r = s; r < 8; r++)
            for (int c = 0; c < 9; c++) {
                if (used >> c & 1u) continue;
                const double v = fabs(A(r, c));
                if (v > best) {
                    best = v;
                    br = r;
                    bc = c;
                }
            }
        if (br < 0) return false;
        const double p = A(br, bc);
        if (p == 0. || !(fabs(p) <= DBL_MAX)) return false;
        if (br != s)
            for (int j = 0; j < 9; j++) {
                const double t = A(s, j);
                A(s, j) = A(br, j);
                A(br, j) = t;
            }
        for (int r = 0; r < 8; r++) {
            if (r == s) continue;
            const double f = A(r, bc) / p;
            if (f != 0.)
                for (int j = 0; j < 9; j++) A(r, j) = A(r, j) - f * A(s, j);
        }
        used |= 1u << bc;
#pragma unroll
        for (int k = 0; k < 8; k++) col[k] = k == s ? bc : col[k];
    }
    int fr = 0;
#pragma unroll
    for (int c = 0; c < 9; c++)
        if (!(used >> c & 1u)) fr = c;
    double x[9];
#pragma unroll
    for (int c = 0; c < 9; c++) x[c] = 1.;
#pragma unroll
    for (int s = 0; s < 8; s++) {
        const double v = -A(s, fr) / A(s, col[s]);
#pragma unroll
        for (int c = 0; c < 9; c++) x[c] = c == col[s] ? v : x[c];
    }
    double ss = 0.;
#pragma unroll
    for (int c = 0; c < 9; c++) ss += x[c] * x[c];
    if (!(ss <= DBL_MAX)) return false;
    const double inv = 1. / sqrt(ss);
#pragma unroll
    for (int c = 0; c < 9; c++) e[c] = x[c] * inv;
    return true;
}

// The left and right singular vectors of a row-major 3 x 3 E in fm3d_cv::jacobi_svd's sorted order:
// u_i = At[perm[i]] * (1 / W[i]) for i = 0, 1 and v_i = Vt[perm[i]].  False unless W[1] > DBL_MIN.
FM3D_CVSVD_HD bool svd_e(const double E[9], double (&u)[2][3], double (&v)[2][3], double (&W)[3]) {
    double At[3][3], Vt[3][3];
    int perm[3];
#pragma unroll
    for (int i = 0; i < 3; i++)
#pragma unroll
        for (int k = 0; k < 3; k++) At[i][k] = E[k * 3 + i];
    fm3d_cv::jacobi_svd<3, 3>(At, W, Vt, perm);
    if (!(W[1] > DBL_MIN)) return false;
#pragma unroll
    for (int i = 0; i < 2; i++) {
        double a[3];
        fm3d_cv::pick_row<3, 3>(At, perm[i], a);
        fm3d_cv::pick_row<3, 3>(Vt, perm[i], v[i]);
        const double s = 1. / W[i];
#pragma unroll
        for (int k = 0; k < 3; k++) u[i][k] = a[k] * s;
    }
    return true;
}

// the nearest essential matrix in shape: singular values (1, 1, 0) on e's singular vectors
FM3D_CVSVD_HD bool project_essential(const double e[9], double E[9]) {
    double u[2][3], v[2][3], W[3];
    if (!svd_e(e, u, v, W)) return false;
#pragma unroll
    for (int r = 0; r < 3; r++)
#pragma unroll
        for (int c = 0; c < 3; c++) E[r * 3 + c] = u[0][r] * v[0][c] + u[1][r] * v[1][c];
    return true;
}

// the model of eight pairs whose rows are already in A; an invalid one is all zero (false)
template <typename Mat>
FM3D_CVSVD_HD bool model8(Mat& A, double E[9], double e[9]) {
    const bool ok = null8(A, e) && project_essential(e, E);
    if (!ok) {
#pragma unroll
        for (int k = 0; k < 9; k++) E[k] = 0.;
    }
    return ok;
}

// Sampson's test without the division: r^2 <= tau2 * den with den > 0 (a NaN fails)
FM3D_CVSVD_HD bool inlier(const double E[9], double x1, double y1, double x2, double y2, double tau2) {
    const double l0 = (E[0] * x1 + E[1] * y1) + E[2];
    const double l1 = (E[3] * x1 + E[4] * y1) + E[5];
    const double l2 = (E[6] * x1 + E[7] * y1) + E[8];
    const double m0 = (E[0] * x2 + E[3] * y2) + E[6];
    const double m1 = (E[1] * x2 + E[4] * y2) + E[7];
    const double r = (x2 * l0 + y2 * l1) + l2;
    const double den = ((l0 * l0 + l1 * l1) + m0 * m0) + m1 * m1;
    return (den > 0.) & (r * r <= tau2 * den);  // both evaluated: no branch per pair in the scoring loop
}

// ---------------- the refit on the inliers ("Refinement") ----------------

constexpr int kPairs = 45;         // the entries (r, c), r <= c, of the symmetric 9 x 9, row by row
constexpr int kRefitTile = 1024;   // slots of one summation tile (the scoring kernel's tile)
constexpr int kRefitLanes = 256;   // leaves of a tile's tree: slot k * 256 + t belongs to leaf t
constexpr int kJacobiSweeps = 30;
constexpr int kRefitMaxIters = 16;

// the coefficients of one pair: set_row's nine entries
FM3D_CVSVD_HD void row9(double x1, double y1, double x2, double y2, double (&a)[9]) {
    a[0] = x2 * x1;
    a[1] = x2 * y1;
    a[2] = x2;
    a[3] = y2 * x1;
    a[4] = y2 * y1;
    a[5] = y2;
    a[6] = x1;
    a[7] = y1;
    a[8] = 1.;
}

// a slot's value for the entry (r, c): a[r] * a[c] when the pair is in, +0.0 otherwise (a select, not
// a product with 0: a NaN adds nothing)
FM3D_CVSVD_HD double slot(bool in, const double (&a)[9], int r, int c) { return in ? a[r] * a[c] : 0.; }

// a thread's leaf of a tile: the four slots k * 256 + t as (v0 + v1) + (v2 + v3)
FM3D_CVSVD_HD double leaf4(double v0, double v1, double v2, double v3) { return (v0 + v1) + (v2 + v3); }

// a symmetric 9 x 9 (and its eigenvectors) on the host; the solve kernel keeps its own in LDS
struct Mat99 {
    double a[81];
    FM3D_CVSVD_HD double& operator()(int r, int c) { return a[r * 9 + c]; }
};

// how the rows of a rotation are shared out: one thread on the host; the solve kernel gives row k to
// lane k and puts a barrier where one lane reads what another wrote
struct OneThread {
    FM3D_CVSVD_HD int first() const { return 0; }
    FM3D_CVSVD_HD int step() const { return 1; }
    FM3D_CVSVD_HD void sync() const {}
};

// The eigenvector of the smallest eigenvalue of the symmetric S (both triangles stored; destroyed)
// by cyclic Jacobi rotations, V the accumulated rotations.  Pairs (p, q), p = 0..7, q = p+1..8; a pair
// rotates iff |S[p][q]| > 10 DBL_EPSILON sqrt(S[p][p] S[q][q]) (false for a NaN):
//   theta = (S[q][q] - S[p][p]) / (2 S[p][q]),  t = sign(theta) / (|theta| + sqrt(theta theta + 1)),
//   c = 1 / sqrt(t t + 1),  s = t c,  h = t S[p][q];
//   S[p][p] -= h, S[q][q] += h, S[p][q] = S[q][p] = 0;
//   for k != p, q: (S[k][p], S[k][q]) = (c S[k][p] - s S[k][q], s S[k][p] + c S[k][q]), mirrored;
//   for every k:   (V[k][p], V[k][q]) = (c V[k][p] - s V[k][q], s V[k][p] + c V[k][q]).
// It stops after a sweep without a rotation, after 30 sweeps at most.  e: the column of V under the
// smallest S[j][j], the lowest j on ties.  Only + - * / sqrt.  The rows k of one rotation do not
// depend on each other, so `team` may spread them over threads that all run this function on the same
// S, V and e: every thread takes the same branches, and an entry's value does not depend on who
// computes it.
template <typename Mat, typename Team>
FM3D_CVSVD_HD void jacobi_null9(Mat& S, Mat& V, double* e, const Team& team) {
    for (int r = team.first(); r < 9; r += team.step())
        for (int c = 0; c < 9; c++) V(r, c) = r == c ? 1. : 0.;
    team.sync();
    for (int sweep = 0; sweep < kJacobiSweeps; sweep++) {
        bool rotated = false;
        for (int p = 0; p < 8; p++)
            for (int q = p + 1; q < 9; q++) {
                const double apq = S(p, q), app = S(p, p), aqq = S(q, q);
                const double thr = (10. * DBL_EPSILON) * sqrt(app * aqq);
                if (!(fabs(apq) > thr)) continue;
                rotated = true;
                const double theta = (aqq - app) / (2. * apq);
                const double t = (theta < 0. ? -1. : 1.) / (fabs(theta) + sqrt(theta * theta + 1.));
                const double c = 1. / sqrt(t * t + 1.);
                const double s = t * c;
                const double h = t * apq;
                team.sync();  // every thread has read the three entries
                if (team.first() == 0) {
                    S(p, p) = app - h;
                    S(q, q) = aqq + h;
                    S(p, q) = 0.;
                    S(q, p) = 0.;
                }
                for (int k = team.first(); k < 9; k += team.step()) {
                    if (k != p && k != q) {
                        const double akp = S(k, p), akq = S(k, q);
                        const double np = c * akp - s * akq, nq = s * akp + c * akq;
                        S(k, p) = np;
                        S(p, k) = np;
                        S(k, q) = nq;
                        S(q, k) = nq;
                    }
                    const double vkp = V(k, p), vkq = V(k, q);
                    V(k, p) = c * vkp - s * vkq;
                    V(k, q) = s * vkp + c * vkq;
                }
                team.sync();
            }
        if (!rotated) break;
    }
    int m = 0;
    double least = S(0, 0);
    for (int j = 1; j < 9; j++) {
        const double d = S(j, j);
        if (d < least) {
            least = d;
            m = j;
        }
    }
    for (int k = team.first(); k < 9; k += team.step()) e[k] = V(k, m);
    team.sync();
}

// The normal matrix N45 (the 45 sums, r <= c row by row) into S; false when the refit is invalid from
// the start: a non-finite entry, or fewer than 8 pairs in (N[8][8] is their count: a[8] = 1)
template <typename Mat>
FM3D_CVSVD_HD bool refit_load(const double* N45, Mat& S) {
    bool ok = true;
    int j = 0;
    for (int r = 0; r < 9; r++)
        for (int c = r; c < 9; c++) {
            const double v = N45[j++];
            ok = ok && fabs(v) <= DBL_MAX;
            S(r, c) = v;
            S(c, r) = v;
        }
    return ok && N45[kPairs - 1] >= 8.;
}

// E' from the eigenvector; invalid (false, a zero E): a non-finite entry of e or a projection that fails
FM3D_CVSVD_HD bool refit_project(bool ok, const double* e, double E[9]) {
    if (ok) {
        double ev[9];
#pragma unroll
        for (int k = 0; k < 9; k++) {
            ev[k] = e[k];
            ok = ok && fabs(ev[k]) <= DBL_MAX;
        }
        ok = ok && project_essential(ev, E);
    }
    if (!ok) {
#pragma unroll
        for (int k = 0; k < 9; k++) E[k] = 0.;
    }
    return ok;
}

// the refit from the normal matrix on one thread (S, V: workspace)
template <typename Mat>
FM3D_CVSVD_HD bool refit45(const double* N45, Mat& S, Mat& V, double E[9]) {
    double e[9];
    const bool ok = refit_load(N45, S);
    if (ok) jacobi_null9(S, V, e, OneThread());
    return refit_project(ok, e, E);
}

// ---------------- the pose from a model ("Pose") ----------------

constexpr int kPoseDoubles = 21;  // the candidates as one block: R[0] (9), R[1] (9), u_2 (3)

FM3D_CVSVD_HD double dot3(const double a[3], const double b[3]) { return (a[0] * b[0] + a[1] * b[1]) + a[2] * b[2]; }

FM3D_CVSVD_HD void cross3(const double a[3], const double b[3], double c[3]) {
    c[0] = a[1] * b[2] - a[2] * b[1];
    c[1] = a[2] * b[0] - a[0] * b[2];
    c[2] = a[0] * b[1] - a[1] * b[0];
}

// The four decompositions of E share two rotations and one direction: with svd_e's u_0, u_1, v_0, v_1,
// u_2 = u_0 x u_1 and v_2 = v_0 x v_1,
//   R[0] = U W V^T   =  u_1 v_0^T - u_0 v_1^T + u_2 v_2^T,
//   R[1] = U W^T V^T = -u_1 v_0^T + u_0 v_1^T + u_2 v_2^T   (row-major),
// and candidate k = 0 .. 3 is (R[k >> 1], t = u_2 for an even k, -u_2 for an odd one).  False when
// svd_e fails (R and u2 are then not written).
FM3D_CVSVD_HD bool pose_candidates(const double E[9], double (&R)[2][9], double (&u2)[3]) {
    double u[2][3], v[2][3], W[3], v2[3];
    if (!svd_e(E, u, v, W)) return false;
    cross3(u[0], u[1], u2);
    cross3(v[0], v[1], v2);
#pragma unroll
    for (int r = 0; r < 3; r++)
#pragma unroll
        for (int c = 0; c < 3; c++) {
            R[0][r * 3 + c] = (u[1][r] * v[0][c] + (-u[0][r]) * v[1][c]) + u2[r] * v2[c];
            R[1][r * 3 + c] = ((-u[1][r]) * v[0][c] + u[0][r] * v[1][c]) + u2[r] * v2[c];
        }
    return true;
}

// candidate k's translation direction
FM3D_CVSVD_HD void pose_direction(int k, const double u2[3], double t[3]) {
    const double sg = (k & 1) ? -1. : 1.;
#pragma unroll
    for (int j = 0; j < 3; j++) t[j] = sg * u2[j];
}

// One pair's vote for (R, t): the depths z1, z2 of the point nearest both rays z1 a and z2 b - t, with
// a = R (x1, y1, 1) and b = (x2, y2, 1), are both > 0.  The two quotients are formed: a sign test in
// their place would vote differently when one underflows to zero.
FM3D_CVSVD_HD bool pose_vote(const double R[9], const double t[3], double x1, double y1, double x2, double y2) {
    const double p[3] = {x1, y1, 1.}, b[3] = {x2, y2, 1.};
    const double a[3] = {dot3(R, p), dot3(R + 3, p), dot3(R + 6, p)};
    const double aa = dot3(a, a), ab = dot3(a, b), bb = dot3(b, b), at = dot3(a, t), bt = dot3(b, t);
    const double det = aa * bb - ab * ab;
    const double z1 = (ab * bt - bb * at) / det, z2 = (aa * bt - ab * at) / det;
    return z1 > 0. && z2 > 0.;
}

// the candidate with most votes, the lowest index on ties
FM3D_CVSVD_HD int pose_pick(const int votes[4]) {
    int bk = 0;
    for (int k = 1; k < 4; k++)
        if (votes[k] > votes[bk]) bk = k;
    return bk;
}

// g12 = [R | baseline t] of candidate k, row-major 4 x 4
FM3D_CVSVD_HD void pose_g12(int k, const double (&R)[2][9], const double u2[3], double baseline, double g12[16]) {
    const double* Rb = R[k >> 1];
    double t[3];
    pose_direction(k, u2, t);
    for (int r = 0; r < 3; r++) {
        for (int c = 0; c < 3; c++) g12[r * 4 + c] = Rb[r * 3 + c];
        g12[r * 4 + 3] = baseline * t[r];
    }
    g12[12] = g12[13] = g12[14] = 0.;
    g12[15] = 1.;
}

}  // namespace fm3d_epi8

#endif /* FM3D_EPI8_H */
