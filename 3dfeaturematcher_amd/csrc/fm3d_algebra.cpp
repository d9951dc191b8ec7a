// fm3d_algebra.cpp -- the C ABI's context-free host algebra (include/fm3d.h): setg12, Rodrigues both
// ways, Matx44d::inv, the epipolar matrix, gravity, the patch size.
//
// It restates the reference's scalar fp64 code with the same operation order as
// oracle/fm3d_oracle.c, and -ffp-contract=off is part of that contract.  No HIP header and no
// fm3d_ctx: the file also builds with a plain host compiler (tests/native/Makefile).
#include <algorithm>
#include <cfloat>
#include <cmath>
#include <cstring>

#include "fm3d.h"
#include "fm3d_algebra.h"
#include "fm3d_cvsvd.h"

namespace {

// ---------------- host algebra (same operation order as the oracle) ----------------
void rodrigues_v2m(const double r[3], double R[9]) {
    double rx = r[0], ry = r[1], rz = r[2];
    double theta = std::sqrt(rx * rx + ry * ry + rz * rz);
    if (theta < DBL_EPSILON) {
        for (int k = 0; k < 9; k++) R[k] = (k % 4 == 0) ? 1. : 0.;
        return;
    }
    const double I[9] = {1, 0, 0, 0, 1, 0, 0, 0, 1};
    double c = std::cos(theta), s = std::sin(theta), c1 = 1. - c;
    double itheta = theta ? 1. / theta : 0.;
    rx *= itheta;
    ry *= itheta;
    rz *= itheta;
    const double rrt[9] = {rx * rx, rx * ry, rx * rz, rx * ry, ry * ry, ry * rz, rx * rz, ry * rz, rz * rz};
    const double rxm[9] = {0, -rz, ry, rz, 0, -rx, -ry, rx, 0};
    for (int k = 0; k < 9; k++) R[k] = c * I[k] + c1 * rrt[k] + s * rxm[k];
}

// cvRodrigues2 matrix -> vector: R replaced by its polar factor U V^T from OpenCV 2.4's SVD
// (include/fm3d_cvsvd.h, the same JacobiSVD the oracle restates), then the skew part and trace
void rodrigues_m2v(const double Rin[9], double r[3]) {
    double R[9];
    fm3d_cv::polar3(Rin, R);
    double rx = R[7] - R[5], ry = R[2] - R[6], rz = R[3] - R[1];
    double s = std::sqrt((rx * rx + ry * ry + rz * rz) * 0.25);
    double c = (R[0] + R[4] + R[8] - 1) * 0.5;
    c = c > 1. ? 1. : c < -1. ? -1. : c;
    double theta = std::acos(c);
    if (s < 1e-5) {
        double t;
        if (c > 0)
            rx = ry = rz = 0;
        else {
            t = (R[0] + 1) * 0.5;
            rx = std::sqrt(t > 0. ? t : 0.);
            t = (R[4] + 1) * 0.5;
            ry = std::sqrt(t > 0. ? t : 0.) * (R[1] < 0 ? -1. : 1.);
            t = (R[8] + 1) * 0.5;
            rz = std::sqrt(t > 0. ? t : 0.) * (R[2] < 0 ? -1. : 1.);
            if (std::fabs(rx) < std::fabs(ry) && std::fabs(rx) < std::fabs(rz) && (R[5] > 0) != (ry * rz > 0)) rz = -rz;
            theta /= std::sqrt(rx * rx + ry * ry + rz * rz);
            rx *= theta;
            ry *= theta;
            rz *= theta;
        }
    } else {
        double vth = 1 / (2 * s);
        vth *= theta;
        rx *= vth;
        ry *= vth;
        rz *= vth;
    }
    r[0] = rx;
    r[1] = ry;
    r[2] = rz;
}

void compose(const double R[9], const double T[3], double G[16]) {  // tools.cpp:87-99
    G[0] = R[0]; G[1] = R[1]; G[2] = R[2]; G[3] = T[0];
    G[4] = R[3]; G[5] = R[4]; G[6] = R[5]; G[7] = T[1];
    G[8] = R[6]; G[9] = R[7]; G[10] = R[8]; G[11] = T[2];
    G[12] = 0; G[13] = 0; G[14] = 0; G[15] = 1;
}

void inv4(const double Ain[16], double B[16]) {  // Matx44d::inv(DECOMP_LU)
    double A[16];
    std::memcpy(A, Ain, sizeof(A));
    for (int i = 0; i < 16; i++) B[i] = (i % 5 == 0) ? 1. : 0.;
    for (int i = 0; i < 4; i++) {
        int k = i;
        for (int j = i + 1; j < 4; j++)
            if (std::fabs(A[j * 4 + i]) > std::fabs(A[k * 4 + i])) k = j;
        if (k != i) {
            for (int j = i; j < 4; j++) std::swap(A[i * 4 + j], A[k * 4 + j]);
            for (int j = 0; j < 4; j++) std::swap(B[i * 4 + j], B[k * 4 + j]);
        }
        double d = -1 / A[i * 4 + i];
        for (int j = i + 1; j < 4; j++) {
            double alpha = A[j * 4 + i] * d;
            for (int kk = i + 1; kk < 4; kk++) A[j * 4 + kk] += alpha * A[i * 4 + kk];
            for (int kk = 0; kk < 4; kk++) B[j * 4 + kk] += alpha * B[i * 4 + kk];
        }
        A[i * 4 + i] = -d;
    }
    for (int i = 3; i >= 0; i--)
        for (int j = 0; j < 4; j++) {
            double s = B[i * 4 + j];
            for (int kk = i + 1; kk < 4; kk++) s -= A[i * 4 + kk] * B[kk * 4 + j];
            B[i * 4 + j] = s * A[i * 4 + i];
        }
}

void mul4(const double a[16], const double b[16], double c[16]) {
    for (int i = 0; i < 4; i++)
        for (int j = 0; j < 4; j++) {
            double s = 0;
            for (int k = 0; k < 4; k++) s += a[i * 4 + k] * b[k * 4 + j];
            c[i * 4 + j] = s;
        }
}

}  // namespace

void fm3d_host::camera2_from_g12(const double g12[16], double R2[9], double t2[3]) {
    double R[9] = {g12[0], g12[1], g12[2], g12[4], g12[5], g12[6], g12[8], g12[9], g12[10]};
    double r[3];
    rodrigues_m2v(R, r);  // decomposeTransformation (tools.cpp:101-114)
    rodrigues_v2m(r, R2); // cvProjectPoints2 converts r2 back to a matrix
    t2[0] = g12[3];
    t2[1] = g12[7];
    t2[2] = g12[11];
}

// E = [t2]x R2, each entry (T[r][0] R2[0][c] + T[r][1] R2[1][c]) + T[r][2] R2[2][c]
void fm3d_host::epipolar_matrix(const double R2[9], const double t2[3], double E[9]) {
    const double T[9] = {0., -t2[2], t2[1], t2[2], 0., -t2[0], -t2[1], t2[0], 0.};
    for (int r = 0; r < 3; r++)
        for (int k = 0; k < 3; k++)
            E[r * 3 + k] = (T[r * 3 + 0] * R2[0 * 3 + k] + T[r * 3 + 1] * R2[1 * 3 + k]) + T[r * 3 + 2] * R2[2 * 3 + k];
}

using namespace fm3d_host;

extern "C" {

int fm3d_epipolar_matrix(const double g12[16], double E[9]) {
    if (!g12 || !E) return FM3D_ERR_INVALID;
    double R2[9], t2[3];
    camera2_from_g12(g12, R2, t2);
    epipolar_matrix(R2, t2, E);
    return FM3D_OK;
}

int fm3d_g12_from_poses(const fm3d_settings* s, const double T1[3], const double T2[3], const double r1[3],
                        const double r2[3], double g[16]) {
    if (!s || !T1 || !T2 || !r1 || !r2 || !g) return FM3D_ERR_INVALID;
    double RIC[9], R1[9], R2[9], gIC[16], g1[16], g2[16], a[16], b[16], cc[16], d[16];
    rodrigues_v2m(s->rodriguesIC, RIC);  // SingleCameraTriangulator ctor (:42-65)
    compose(RIC, s->translationIC, gIC);
    rodrigues_v2m(r1, R1);
    rodrigues_v2m(r2, R2);
    compose(R1, T1, g1);
    compose(R2, T2, g2);
    inv4(gIC, a);
    inv4(g2, b);
    mul4(a, b, cc);
    mul4(cc, g1, d);
    mul4(d, gIC, g);
    return FM3D_OK;
}

int fm3d_camera2_from_g12(const double g12[16], double R2[9], double t2[3]) {
    if (!g12 || !R2 || !t2) return FM3D_ERR_INVALID;
    camera2_from_g12(g12, R2, t2);
    return FM3D_OK;
}

int fm3d_gravity(const fm3d_settings* s, double g[3]) {
    // NormalOptimizer ctor (normaloptimizer.cpp:160-178): Rodrigues(rodriguesIC).inv() * (0,0,-1),
    // OpenCV 2.4's closed-form 3x3 Matx inverse, Matx * Vec accumulated from 0 in index order
    if (!s || !g) return FM3D_ERR_INVALID;
    double a[9], b[9];
    rodrigues_v2m(s->rodriguesIC, a);
#define A(i, j) a[(i)*3 + (j)]
    double d = A(0, 0) * (A(1, 1) * A(2, 2) - A(2, 1) * A(1, 2)) - A(0, 1) * (A(1, 0) * A(2, 2) - A(2, 0) * A(1, 2)) +
               A(0, 2) * (A(1, 0) * A(2, 1) - A(2, 0) * A(1, 1));
    if (d == 0) return FM3D_ERR_INVALID;
    d = 1 / d;
    b[0] = (A(1, 1) * A(2, 2) - A(1, 2) * A(2, 1)) * d;
    b[1] = (A(0, 2) * A(2, 1) - A(0, 1) * A(2, 2)) * d;
    b[2] = (A(0, 1) * A(1, 2) - A(0, 2) * A(1, 1)) * d;
    b[3] = (A(1, 2) * A(2, 0) - A(1, 0) * A(2, 2)) * d;
    b[4] = (A(0, 0) * A(2, 2) - A(0, 2) * A(2, 0)) * d;
    b[5] = (A(0, 2) * A(1, 0) - A(0, 0) * A(1, 2)) * d;
    b[6] = (A(1, 0) * A(2, 1) - A(1, 1) * A(2, 0)) * d;
    b[7] = (A(0, 1) * A(2, 0) - A(0, 0) * A(2, 1)) * d;
    b[8] = (A(0, 0) * A(1, 1) - A(0, 1) * A(1, 0)) * d;
#undef A
    const double v[3] = {0, 0, -1};
    for (int i = 0; i < 3; i++) {
        double acc = 0;
        for (int k = 0; k < 3; k++) acc += b[i * 3 + k] * v[k];
        g[i] = acc;
    }
    return FM3D_OK;
}

int fm3d_patch_size(const fm3d_settings* s) {
    if (!s) return FM3D_ERR_INVALID;
    // numberOfPointsPerEdge (neighborhoodsgenerator.cpp:136-137)
    return 2 * ((int)floor(s->neighEpsilon / (0.01 * s->cmPerPixel)));
}

}  // extern "C"
