// pnp_main.cpp -- include/fm3d_pnp.h (the arithmetic of the 2D-3D localisation) on
// the host, over its edge cases: built with g++ -fsanitize=address,undefined by
// tests/test_pnp_host.py and run directly.  No GPU code is involved.
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <limits>
#include <vector>

#include "fm3d_pnp.h"

namespace pnp = fm3d_pnp;

static int fails = 0;
#define CHECK(c)                                            \
    do {                                                    \
        if (!(c)) {                                         \
            std::printf("FAILED %s:%d %s\n", __FILE__, __LINE__, #c); \
            fails++;                                        \
        }                                                   \
    } while (0)

static int roots(double c4, double c3, double c2, double c1, double c0, double x[4]) {
    return pnp::quartic_roots(c4, c3, c2, c1, c0, x[0], x[1], x[2], x[3]);
}

static bool is_zero(const double* m) {
    for (int k = 0; k < pnp::kModel; k++)
        if (m[k] != 0.) return false;
    return true;
}

// a rotation about (1, 2, 3) / sqrt(14) by the Cayley map: exact enough to project through
static void pose(double m[12]) {
    const double a[3] = {0.02, 0.04, 0.06};
    const double aa = a[0] * a[0] + a[1] * a[1] + a[2] * a[2], d = 1 + aa, e = 1 - aa;
    const double C[9] = {(e + 2 * a[0] * a[0]) / d, (2 * a[0] * a[1] - 2 * a[2]) / d, (2 * a[0] * a[2] + 2 * a[1]) / d,
                         (2 * a[1] * a[0] + 2 * a[2]) / d, (e + 2 * a[1] * a[1]) / d, (2 * a[1] * a[2] - 2 * a[0]) / d,
                         (2 * a[2] * a[0] - 2 * a[1]) / d, (2 * a[2] * a[1] + 2 * a[0]) / d, (e + 2 * a[2] * a[2]) / d};
    for (int k = 0; k < 9; k++) m[k] = C[k];
    m[9] = 0.1;
    m[10] = -0.2;
    m[11] = 0.3;
}

static void project(const double* m, const double X[3], double uv[2]) {
    double x, y, z;
    pnp::camera_point(m, X[0], X[1], X[2], x, y, z);
    uv[0] = x / z;
    uv[1] = y / z;
}

int main() {
    const double nan = std::numeric_limits<double>::quiet_NaN(), inf = std::numeric_limits<double>::infinity();
    double x[4];
    // the quartic: four roots, two, none, biquadratic, a zero leading coefficient, a double root, extremes
    CHECK(roots(1, -10, 35, -50, 24, x) == 4 && std::fabs(x[0] * x[1] * x[2] * x[3] - 24) < 1e-9);
    CHECK(roots(1, -3, 3, -3, 2, x) == 2);
    CHECK(roots(1, 0, 1, 0, 1, x) == 0 && x[0] != x[0]);
    CHECK(roots(1, 0, -5, 0, 4, x) == 4 && x[0] == -1 && x[1] == 1 && x[2] == -2 && x[3] == 2);
    CHECK(roots(0, 1, 2, 3, 4, x) == -1 && roots(1e-320, 1, 2, 3, 4, x) == -1);
    CHECK(roots(1, -6, 13, -12, 4, x) >= 0);
    CHECK(roots(nan, 1, 1, 1, 1, x) == -1 && roots(1, nan, 1, 1, 1, x) == -1 && roots(1, inf, 1, 1, 1, x) == -1);
    CHECK(roots(1, 1e200, 1e200, 1e200, 1e200, x) >= -1 && roots(1e-300, 1e300, 1, 1, 1, x) == -1);
    CHECK(roots(1, 0, 0, 0, 0, x) == 4);

    // P3P: a noise-free sample, collinear and coincident points, NaN and infinite inputs
    double m0[12];
    pose(m0);
    const double X[3][3] = {{-0.4, 0.3, 2.0}, {0.5, 0.2, 1.7}, {0.1, -0.6, 2.2}};
    double uv[3][2], models[pnp::kSlots][pnp::kModel];
    bool ok[pnp::kSlots];
    for (int k = 0; k < 3; k++) project(m0, X[k], uv[k]);
    CHECK(pnp::p3p(X, uv, models, ok) >= 1);
    double bestErr = 1e300;
    for (int k = 0; k < pnp::kSlots; k++) {
        CHECK(ok[k] || is_zero(models[k]));
        if (!ok[k]) continue;
        double e = 0;
        for (int j = 0; j < 12; j++) e = std::fmax(e, std::fabs(models[k][j] - m0[j]));
        bestErr = std::fmin(bestErr, e);
    }
    CHECK(bestErr < 1e-8);
    const double line[3][3] = {{0, 0, 1}, {1, 2, 3}, {2, 4, 5}};
    CHECK(pnp::p3p(line, uv, models, ok) == 0 && is_zero(models[0]) && is_zero(models[3]));
    const double twice[3][3] = {{-0.4, 0.3, 2.0}, {-0.4, 0.3, 2.0}, {0.1, -0.6, 2.2}};
    CHECK(pnp::p3p(twice, uv, models, ok) == 0);
    for (int k = 0; k < 3; k++)
        for (int j = 0; j < 5; j++)
            for (double bad : {nan, inf, -inf, 1e308, 0.}) {
                double Xb[3][3], ub[3][2];
                for (int a = 0; a < 3; a++) {
                    for (int b = 0; b < 3; b++) Xb[a][b] = X[a][b];
                    for (int b = 0; b < 2; b++) ub[a][b] = uv[a][b];
                }
                if (j < 3)
                    Xb[k][j] = bad;
                else
                    ub[k][j - 3] = bad;
                const int n = pnp::p3p(Xb, ub, models, ok);
                CHECK(n >= 0 && n <= 4);
                for (int s = 0; s < pnp::kSlots; s++) {
                    CHECK(ok[s] || is_zero(models[s]));
                    for (int e = 0; e < 12; e++) CHECK(pnp::finite(models[s][e]));
                }
            }

    // the predicate: exactly at the threshold and either side, behind the camera, NaN
    const double id[12] = {1, 0, 0, 0, 1, 0, 0, 0, 1, 0, 0, 0};
    const double tau = 0x1p-8, tau2 = tau * tau, u = 0.25 - tau;
    CHECK(pnp::inlier(id, u, 0.125, 0.5, 0.25, 2.0, tau2));
    CHECK(pnp::inlier(id, std::nextafter(u, 1.), 0.125, 0.5, 0.25, 2.0, tau2));
    CHECK(!pnp::inlier(id, std::nextafter(u, -1.), 0.125, 0.5, 0.25, 2.0, tau2));
    CHECK(!pnp::inlier(id, -0.25, -0.125, 0.5, 0.25, -2.0, 1.0) && !pnp::inlier(id, 0., 0., 0., 0., 0., 1.0));
    CHECK(!pnp::inlier(id, nan, 0.125, 0.5, 0.25, 2.0, tau2) && !pnp::inlier(id, 0.25, 0.125, 0.5, nan, 2.0, tau2));
    CHECK(pnp::inlier_n(id, 0.25, 0.125, 0.5, 0.25, 2.0, 0., 0., 1., tau2, 0.25));
    CHECK(!pnp::inlier_n(id, 0.25, 0.125, 0.5, 0.25, 2.0, 0., 0., -1., tau2, 0.));
    CHECK(!pnp::inlier_n(id, 0.25, 0.125, 0.5, 0.25, 2.0, nan, 0., 1., tau2, 0.));

    // the step: sums over exact matches leave the pose; too few matches, NaN sums and a singular system
    const int n = 40;
    std::vector<double> S(pnp::kSums, 0.), T(pnp::kSums);
    for (int i = 0; i < n; i++) {
        const double P[3] = {std::sin(1.0 + i) * 0.8, std::cos(2.0 * i) * 0.6, 1.6 + 0.7 * std::fabs(std::sin(3.0 * i))};
        double q[2];
        project(m0, P, q);
        pnp::terms(m0, q[0] + 1e-4 * std::sin(5.0 * i), q[1], P[0], P[1], P[2], T.data());
        for (int k = 0; k < pnp::kSums; k++) S[k] += T[k];
    }
    double out[12];
    CHECK(pnp::step_solve(S.data(), m0, out));
    for (int k = 0; k < 12; k++) CHECK(std::fabs(out[k] - m0[k]) < 1e-3);
    std::vector<double> S2 = S;
    S2[pnp::kSums - 1] = 2.;
    CHECK(!pnp::step_solve(S2.data(), m0, out) && is_zero(out));
    S2 = S;
    S2[5] = nan;
    CHECK(!pnp::step_solve(S2.data(), m0, out) && is_zero(out));
    S2.assign(pnp::kSums, 0.);
    S2[pnp::kSums - 1] = 10.;
    CHECK(!pnp::step_solve(S2.data(), m0, out) && is_zero(out));
    pnp::terms(m0, 0., 0., 0., 0., 0., T.data());  // z = t_z: finite
    pnp::terms(id, 0., 0., 0., 0., 0., T.data());  // z = 0: non-finite terms, no trap
    CHECK(!pnp::finite(T[0]) || T[0] == T[0]);

    std::printf(fails ? "pnp_main: %d FAILED\n" : "pnp_main: ok\n", fails);
    return fails ? 1 : 0;
}
