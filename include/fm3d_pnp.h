/*
 * fm3d_pnp.h -- the arithmetic of the 2D-3D localisation, host and device.
 *
 * A RANSAC fit of a camera pose Xc = R X + t to matches between a model's points X and an image's
 * keypoints (u, v) (undistorted, normalised): fm3d_rigid3's sampler taking three matches, the P3P
 * solve by elimination to a quartic (up to four models per sample), the quartic by Ferrari's method,
 * the reprojection test without a division with an optional test of the model's normals, and the
 * refit of a model on the matches it accepts by one Gauss-Newton step per round, its 28 sums in
 * §3.1d's fixed order.  Everything is fp64 in the operand order written here -- only + - * /, sqrt
 * and comparisons -- compiled without FMA contraction, so the host library, the kernels of
 * fm3d_localize.hip and the Python restatement (tests/pnp_pyref.py) give the same bits.  This header
 * is the only place the arithmetic lives.
 *
 * A model is fm3d_rigid3's twelve doubles: R row-major in m[0..8], t in m[9..11].
 */
#ifndef FM3D_PNP_H
#define FM3D_PNP_H

#include <float.h>
#include <math.h>
#include <stdint.h>

#include "fm3d_rigid3.h"

namespace fm3d_pnp {

namespace r3 = fm3d_rigid3;

constexpr int kModel = r3::kModel;
constexpr int kSlots = 4;          // models of one sample: slot k belongs to root k of the quartic
constexpr int kJtJ = 21;           // the upper triangle of J^T J, row by row
constexpr int kSums = 28;          // the refit's sums: J^T J (21), J^T r (6), the count
constexpr int kBisect = 64;        // bisection steps on the resolvent cubic
constexpr int kTile = r3::kTile;
constexpr int kLanes = r3::kLanes;
constexpr int kMaxIters = r3::kMaxIters;

using r3::finite;
using r3::rot_row;
using r3::slot;
using r3::zero_model;

FM3D_CVSVD_HD double nan_value() { return __builtin_nan(""); }

// ---------------- the quartic ("Quartic") ----------------

// the real roots of y^2 + b y + c in the order (-b - s) / 2, (-b + s) / 2 with s = sqrt(b b - 4 c);
// none (two NaN) unless b b - 4 c >= 0
FM3D_CVSVD_HD void quadratic(double b, double c, double& y0, double& y1) {
    const double disc = b * b - 4. * c;
    y0 = y1 = nan_value();
    if (disc >= 0.) {
        const double s = sqrt(disc);
        y0 = (-b - s) / 2.;
        y1 = (-b + s) / 2.;
    }
}

// one Newton step on the monic x^4 + a3 x^3 + a2 x^2 + a1 x + a0 (Horner); a step that is not finite
// (a zero derivative at a double root) leaves x
FM3D_CVSVD_HD double newton(double x, double a3, double a2, double a1, double a0) {
    const double f = (((x + a3) * x + a2) * x + a1) * x + a0;
    const double d = ((4. * x + 3. * a3) * x + 2. * a2) * x + a1;
    const double xn = x - f / d;
    return finite(xn) ? xn : x;
}

// The real roots of c4 x^4 + c3 x^3 + c2 x^2 + c1 x + c0 in four fixed positions, NaN where there is
// none; returns their number, -1 when the polynomial is invalid (|c4| not > DBL_MIN, a monic
// coefficient not finite).
//   monic:     a_k = c_k / c4
//   depressed: x = y - a3 / 4,  e = a3 / 4,  e2 = e e:
//              p = a2 - 6 e2,  q = (a1 - 2 a2 e) + 8 (e2 e),  r = ((a0 - a1 e) + a2 e2) - 3 (e2 e2)
//   q == 0 (biquadratic): z0, z1 = quadratic(p, r); positions 0, 1 = -sqrt(z0), +sqrt(z0) when
//              z0 >= 0, positions 2, 3 = -sqrt(z1), +sqrt(z1) when z1 >= 0
//   otherwise: the resolvent f(m) = ((m + p) m + c1) m - c0 with c1 = (p p) / 4 - r, c0 = (q q) / 8
//              has f(0) < 0: kBisect steps on [0, 1 + max(|p|, |c1|, c0)] (mid = (lo + hi) / 2;
//              f(mid) < 0 moves lo, anything else hi), m = (lo + hi) / 2, required > 0;
//              s = sqrt(2 m), t = q / (2 s), w = p / 2 + m;
//              positions 0, 1 = quadratic(-s, w + t), positions 2, 3 = quadratic(s, w - t)
//   every root: x = y - e, then two Newton steps on the monic quartic.
FM3D_CVSVD_HD int quartic_roots(double c4, double c3, double c2, double c1q, double c0q, double& x0, double& x1,
                                double& x2, double& x3) {
    x0 = x1 = x2 = x3 = nan_value();
    if (!(fabs(c4) > DBL_MIN)) return -1;
    const double a3 = c3 / c4, a2 = c2 / c4, a1 = c1q / c4, a0 = c0q / c4;
    if (!(finite(a3) && finite(a2) && finite(a1) && finite(a0))) return -1;
    const double e = a3 / 4., e2 = e * e;
    const double p = a2 - 6. * e2;
    const double q = (a1 - 2. * a2 * e) + 8. * (e2 * e);
    const double r = ((a0 - a1 * e) + a2 * e2) - 3. * (e2 * e2);
    double y0, y1, y2, y3;
    y0 = y1 = y2 = y3 = nan_value();
    if (q == 0.) {
        double z0, z1;
        quadratic(p, r, z0, z1);
        if (z0 >= 0.) {
            const double s = sqrt(z0);
            y0 = -s;
            y1 = s;
        }
        if (z1 >= 0.) {
            const double s = sqrt(z1);
            y2 = -s;
            y3 = s;
        }
    } else {
        const double c1 = (p * p) / 4. - r, c0 = (q * q) / 8.;
        double big = fabs(p);
        big = fabs(c1) > big ? fabs(c1) : big;
        big = c0 > big ? c0 : big;
        double lo = 0., hi = 1. + big;
        for (int i = 0; i < kBisect; i++) {
            const double mid = (lo + hi) / 2.;
            const double f = ((mid + p) * mid + c1) * mid - c0;
            const bool below = f < 0.;
            lo = below ? mid : lo;
            hi = below ? hi : mid;
        }
        const double m = (lo + hi) / 2.;
        if (m > 0. && finite(m)) {
            const double s = sqrt(2. * m), t = q / (2. * s), w = p / 2. + m;
            quadratic(-s, w + t, y0, y1);
            quadratic(s, w - t, y2, y3);
        }
    }
    // a NaN stays a NaN through the shift and the polish
    x0 = newton(newton(y0 - e, a3, a2, a1, a0), a3, a2, a1, a0);
    x1 = newton(newton(y1 - e, a3, a2, a1, a0), a3, a2, a1, a0);
    x2 = newton(newton(y2 - e, a3, a2, a1, a0), a3, a2, a1, a0);
    x3 = newton(newton(y3 - e, a3, a2, a1, a0), a3, a2, a1, a0);
    return (int)(x0 == x0) + (int)(x1 == x1) + (int)(x2 == x2) + (int)(x3 == x3);
}

// ---------------- the minimal solve: P3P by elimination ("P3P") ----------------

FM3D_CVSVD_HD double dot3(const double a[3], const double b[3]) { return (a[0] * b[0] + a[1] * b[1]) + a[2] * b[2]; }

FM3D_CVSVD_HD double dist2(const double a[3], const double b[3]) {
    const double d0 = a[0] - b[0], d1 = a[1] - b[1], d2 = a[2] - b[2];
    return (d0 * d0 + d1 * d1) + d2 * d2;
}

// the unit bearing of a normalised image point: (u, v, 1) / sqrt((u u + v v) + 1)
FM3D_CVSVD_HD void bearing(double u, double v, double j[3]) {
    const double n = sqrt((u * u + v * v) + 1.);
    j[0] = u / n;
    j[1] = v / n;
    j[2] = 1. / n;
}

// slot k of a sample from root v of the quartic: the distances s0 = sqrt(b2 / q(v)), s1 = u s0,
// s2 = v s0 with u = N(v) / D(v), the camera points C_i = s_i j_i and fm3d_rigid3::rigid_from3(X, C).
// Invalid (false, the zero model): not v > 0, D(v) == 0, not u > 0, a value that is not finite, or
// rigid_from3's reasons.
FM3D_CVSVD_HD bool p3p_slot(double v, const double X[3][3], const double j[3][3], double b2, double q1, double N0,
                            double N1, double N2, double D0, double D1, double m[kModel]) {
    bool ok = v > 0.;
    const double Dv = D0 + D1 * v;
    const double Nv = (N2 * v + N1) * v + N0;
    ok = ok && Dv != 0.;
    const double u = Nv / Dv;
    ok = ok && u > 0.;
    const double qv = (v * v + q1 * v) + 1.;
    const double s0 = sqrt(b2 / qv), s1 = u * s0, s2 = v * s0;
    ok = ok && finite(s0) && finite(s1) && finite(s2);
    if (ok) {
        double C[3][3];
#pragma unroll
        for (int r = 0; r < 3; r++) {
            C[0][r] = s0 * j[0][r];
            C[1][r] = s1 * j[1][r];
            C[2][r] = s2 * j[2][r];
        }
        ok = r3::rigid_from3(X, C, m);
    } else {
        zero_model(m);
    }
    return ok;
}

// The up to four models of three matches: X[i] the model points, uv[i] the normalised image points.
// With j_i the bearings, ca = j1 . j2, cb = j0 . j2, cg = j0 . j1, a2 = |X1 - X2|^2, b2 = |X0 - X2|^2,
// c2 = |X0 - X1|^2 (each required > 0, else no model) and k = a2 - c2, the polynomials in v, lowest
// coefficient first:
//   q = (1, q1, 1),  q1 = -2 cb
//   N = (b2 + k, k q1, k - b2)            [b2 - b2 v^2 + k q]
//   D = (2 b2 cg, -(2 b2 ca))             [2 b2 (cg - ca v)]
//   W = (b2 - c2, -(c2 q1), -c2)          [b2 - c2 q]
// and the products
//   NN = (N0 N0, 2 (N0 N1), 2 (N0 N2) + N1 N1, 2 (N1 N2), N2 N2)
//   ND = (N0 D0, N0 D1 + N1 D0, N1 D1 + N2 D0, N2 D1, 0)
//   DD = (D0 D0, 2 (D0 D1), D1 D1)
//   WD = (W0 DD0, W0 DD1 + W1 DD0, (W0 DD2 + W1 DD1) + W2 DD0, W1 DD2 + W2 DD1, W2 DD2)
// give the quartic's coefficients A_k = (b2 NN_k - D0 ND_k) + WD_k  [b2 N^2 - 2 b2 cg N D + W D^2].
// Slot k is root k's (quartic_roots' position k); ok[k] says whether models[k] is one.  Returns the
// number of valid slots.
FM3D_CVSVD_HD int p3p(const double X[3][3], const double uv[3][2], double models[kSlots][kModel], bool ok[kSlots]) {
    double j[3][3];
#pragma unroll
    for (int i = 0; i < 3; i++) bearing(uv[i][0], uv[i][1], j[i]);
    const double ca = dot3(j[1], j[2]), cb = dot3(j[0], j[2]), cg = dot3(j[0], j[1]);
    const double a2 = dist2(X[1], X[2]), b2 = dist2(X[0], X[2]), c2 = dist2(X[0], X[1]);
    double v0, v1, v2, v3;
    v0 = v1 = v2 = v3 = nan_value();
    const double k = a2 - c2, q1 = -2. * cb;
    const double N0 = b2 + k, N1 = k * q1, N2 = k - b2;
    const double D0 = 2. * b2 * cg, D1 = -(2. * b2 * ca);
    if (a2 > 0. && b2 > 0. && c2 > 0.) {
        const double W0 = b2 - c2, W1 = -(c2 * q1), W2 = -c2;
        const double NN0 = N0 * N0, NN1 = 2. * (N0 * N1), NN2 = 2. * (N0 * N2) + N1 * N1, NN3 = 2. * (N1 * N2), NN4 = N2 * N2;
        const double ND0 = N0 * D0, ND1 = N0 * D1 + N1 * D0, ND2 = N1 * D1 + N2 * D0, ND3 = N2 * D1;
        const double DD0 = D0 * D0, DD1 = 2. * (D0 * D1), DD2 = D1 * D1;
        const double WD0 = W0 * DD0, WD1 = W0 * DD1 + W1 * DD0, WD2 = (W0 * DD2 + W1 * DD1) + W2 * DD0,
                     WD3 = W1 * DD2 + W2 * DD1, WD4 = W2 * DD2;
        const double A0 = (b2 * NN0 - D0 * ND0) + WD0, A1 = (b2 * NN1 - D0 * ND1) + WD1, A2 = (b2 * NN2 - D0 * ND2) + WD2,
                     A3 = (b2 * NN3 - D0 * ND3) + WD3, A4 = (b2 * NN4 - D0 * 0.) + WD4;
        quartic_roots(A4, A3, A2, A1, A0, v0, v1, v2, v3);
    }
    ok[0] = p3p_slot(v0, X, j, b2, q1, N0, N1, N2, D0, D1, models[0]);
    ok[1] = p3p_slot(v1, X, j, b2, q1, N0, N1, N2, D0, D1, models[1]);
    ok[2] = p3p_slot(v2, X, j, b2, q1, N0, N1, N2, D0, D1, models[2]);
    ok[3] = p3p_slot(v3, X, j, b2, q1, N0, N1, N2, D0, D1, models[3]);
    return (int)ok[0] + (int)ok[1] + (int)ok[2] + (int)ok[3];
}

// ---------------- the predicate ("Predicate") ----------------

// the camera-frame point Xc = R X + t
FM3D_CVSVD_HD void camera_point(const double* m, double X, double Y, double Z, double& x, double& y, double& z) {
    x = rot_row(m, 0, X, Y, Z) + m[9];
    y = rot_row(m, 1, X, Y, Z) + m[10];
    z = rot_row(m, 2, X, Y, Z) + m[11];
}

// the reprojection test on Xc: z > 0 and (x - u z)^2 + (y - v z)^2 <= tau2 z^2 (a NaN fails)
FM3D_CVSVD_HD bool near_xc(double x, double y, double z, double u, double v, double tau2) {
    const double ex = x - u * z, ey = y - v * z;
    const int front = z > 0., close = ex * ex + ey * ey <= tau2 * (z * z);
    return (front & close) != 0;
}

FM3D_CVSVD_HD bool inlier(const double* m, double u, double v, double X, double Y, double Z, double tau2) {
    double x, y, z;
    camera_point(m, X, Y, Z, x, y, z);
    return near_xc(x, y, z, u, v, tau2);
}

// The test of the normals.  The model's normals point away from the camera that built them (the LM
// starts from X / |X| and keeps that side), so a camera that sees the same side of the surface has
// d = (R n) . Xc >= 0; the match passes when d >= 0 and d d >= c2 (Xc . Xc), c2 = minFacingCos^2
// (the cosine between the normal and the viewing ray, for a unit normal, without a division).
// Both tests are evaluated: no branch per match in the scoring loop.
FM3D_CVSVD_HD bool inlier_n(const double* m, double u, double v, double X, double Y, double Z, double nx, double ny,
                            double nz, double tau2, double c2) {
    double x, y, z;
    camera_point(m, X, Y, Z, x, y, z);
    const double r0 = rot_row(m, 0, nx, ny, nz), r1 = rot_row(m, 1, nx, ny, nz), r2 = rot_row(m, 2, nx, ny, nz);
    const double d = (r0 * x + r1 * y) + r2 * z;
    const int near = near_xc(x, y, z, u, v, tau2);
    const int front = d >= 0., steep = d * d >= c2 * ((x * x + y * y) + z * z);
    return (near & front & steep) != 0;
}

// ---------------- the refit: one Gauss-Newton step ("Refit") ----------------

// The 28 terms of one match under model m: with P = R X, (x, y, z) = P + t, iz = 1 / z,
// a = iz, b = -(x iz) iz, c = -(y iz) iz, the residual r = (x iz - u, y iz - v) and the Jacobian's rows
// over (omega, delta t)
//   J0 = (b Py, a Pz - b Px, -(a Py), a, 0, b)
//   J1 = (c Py - a Pz, -(c Px), a Px, 0, a, c),
// T[0..20] = J0[i] J0[k] + J1[i] J1[k] for i <= k row by row, T[21..26] = J0[i] r0 + J1[i] r1, T[27] = 1.
// J[0..5] = J0, J[6..11] = J1, J[12..13] = r: what a lane of the sum kernel keeps per match
FM3D_CVSVD_HD void jacobian(const double* m, double u, double v, double X, double Y, double Z, double J[14]) {
    const double Px = rot_row(m, 0, X, Y, Z), Py = rot_row(m, 1, X, Y, Z), Pz = rot_row(m, 2, X, Y, Z);
    const double x = Px + m[9], y = Py + m[10], z = Pz + m[11];
    const double iz = 1. / z;
    const double xi = x * iz, yi = y * iz;
    const double a = iz, b = -(xi * iz), c = -(yi * iz);
    J[0] = b * Py;
    J[1] = a * Pz - b * Px;
    J[2] = -(a * Py);
    J[3] = a;
    J[4] = 0.;
    J[5] = b;
    J[6] = c * Py - a * Pz;
    J[7] = -(c * Px);
    J[8] = a * Px;
    J[9] = 0.;
    J[10] = a;
    J[11] = c;
    J[12] = xi - u;
    J[13] = yi - v;
}

// entry (i, k) of J^T J (k <= 5) or entry i of J^T r (k == 6) from jacobian()'s fourteen
FM3D_CVSVD_HD double term(const double J[14], int i, int k) { return J[i] * J[k == 6 ? 12 : k] + J[6 + i] * J[k == 6 ? 13 : 6 + k]; }

FM3D_CVSVD_HD void terms(const double* m, double u, double v, double X, double Y, double Z, double T[kSums]) {
    double J[14];
    jacobian(m, u, v, X, Y, Z, J);
    int n = 0;
#pragma unroll
    for (int i = 0; i < 6; i++)
#pragma unroll
        for (int k = i; k < 6; k++) T[n++] = term(J, i, k);
#pragma unroll
    for (int i = 0; i < 6; i++) T[kJtJ + i] = term(J, i, 6);
    T[kSums - 1] = 1.;
}

// The step from the sums S and the current model: J^T J delta = -(J^T r) by Cholesky (A = L L^T, column
// by column, every entry s = A[i][j] - L[i][0] L[j][0] - ... in k order; forward then backward
// substitution in the same manner), omega = delta[0..2], the Cayley map of a = omega / 2
//   C = ((1 - a.a) I + 2 a a^T + 2 [a]x) / (1 + a.a),   R' = C R (rows by rot-row order),   t' = t + delta[3..5].
// Invalid (false, the zero model): a sum that is not finite, fewer than three matches in, a pivot
// that is not > 0, an entry of the new model that is not finite.
FM3D_CVSVD_HD bool step_solve(const double S[kSums], const double* m, double out[kModel]) {
    bool ok = true;
#pragma unroll
    for (int k = 0; k < kSums; k++) ok = ok && finite(S[k]);
    ok = ok && S[kSums - 1] >= 3.;
    double A[6][6], L[6][6], g[6], yv[6], d[6];
    {
        int n = 0;
#pragma unroll
        for (int i = 0; i < 6; i++)
#pragma unroll
            for (int k = i; k < 6; k++) {
                A[i][k] = S[n];
                A[k][i] = S[n];
                n++;
            }
    }
#pragma unroll
    for (int i = 0; i < 6; i++) {
        g[i] = -S[kJtJ + i];
#pragma unroll
        for (int k = 0; k < 6; k++) L[i][k] = 0.;
    }
#pragma unroll
    for (int j = 0; j < 6; j++) {
        double s = A[j][j];
#pragma unroll
        for (int k = 0; k < j; k++) s = s - L[j][k] * L[j][k];
        ok = ok && s > 0.;
        const double piv = sqrt(s);
        L[j][j] = piv;
#pragma unroll
        for (int i = j + 1; i < 6; i++) {
            double e = A[i][j];
#pragma unroll
            for (int k = 0; k < j; k++) e = e - L[i][k] * L[j][k];
            L[i][j] = e / piv;
        }
    }
#pragma unroll
    for (int i = 0; i < 6; i++) {
        double s = g[i];
#pragma unroll
        for (int k = 0; k < i; k++) s = s - L[i][k] * yv[k];
        yv[i] = s / L[i][i];
    }
#pragma unroll
    for (int i = 5; i >= 0; i--) {
        double s = yv[i];
#pragma unroll
        for (int k = i + 1; k < 6; k++) s = s - L[k][i] * d[k];
        d[i] = s / L[i][i];
    }
    const double a0 = d[0] / 2., a1 = d[1] / 2., a2 = d[2] / 2.;
    const double aa = (a0 * a0 + a1 * a1) + a2 * a2;
    const double den = 1. + aa, e = 1. - aa;
    const double C[9] = {(e + 2. * (a0 * a0)) / den,        (2. * (a0 * a1) - 2. * a2) / den, (2. * (a0 * a2) + 2. * a1) / den,
                         (2. * (a1 * a0) + 2. * a2) / den, (e + 2. * (a1 * a1)) / den,        (2. * (a1 * a2) - 2. * a0) / den,
                         (2. * (a2 * a0) - 2. * a1) / den, (2. * (a2 * a1) + 2. * a0) / den, (e + 2. * (a2 * a2)) / den};
#pragma unroll
    for (int r = 0; r < 3; r++)
#pragma unroll
        for (int c = 0; c < 3; c++) out[r * 3 + c] = rot_row(C, r, m[c], m[3 + c], m[6 + c]);
#pragma unroll
    for (int r = 0; r < 3; r++) out[9 + r] = m[9 + r] + d[3 + r];
#pragma unroll
    for (int k = 0; k < kModel; k++) ok = ok && finite(out[k]);
    if (!ok) zero_model(out);
    return ok;
}

}  // namespace fm3d_pnp

#endif /* FM3D_PNP_H */
