// fm3d_probe.hip -- the shared math headers evaluated on the device, one element per thread
// (fm3d_math_probe, include/fm3d.h; tests/test_gpu_math_probe.py).
//
// The kernel only calls include/fm3d_crmath.h, fm3d_detmath.h, fm3d_cvmath.h and fm3d_fastdiv.h on
// operands the caller chooses, built with the flags of every other kernel, so a test can compare
// the device build of those headers with the host build (the oracle's) and with IEEE arithmetic
// on inputs the pipelines never produce.  Every helper call sits inside `if (i < n)` with no
// clamped index: the lanes past n of the last wave are inactive, as the helpers that ballot
// (mdiv, recip_z_lo) see them in a kernel's partial wave.
#include <hip/hip_runtime.h>

#include "fm3d_crmath.h"
#include "fm3d_cvmath.h"
#include "fm3d_fastdiv.h"
#include "fm3d_kernels.h"

namespace fm3d {

namespace {

// one function of x[i] / of (x[i], y[i]); fn is grid-uniform, so the switch costs nothing per lane
#define PROBE1(code, expr)          \
    case code:                      \
        if (i < n) {                \
            const double a = x[i];  \
            out[i] = (expr);        \
        }                           \
        break
#define PROBE2(code, expr)                    \
    case code:                                \
        if (i < n) {                          \
            const double a = x[i], b = y[i];  \
            out[i] = (expr);                  \
        }                                     \
        break

// flatten: every header function inlined (a call would pass fm3d_cr_reduce's quadrant through scratch)
__global__ __launch_bounds__(256) __attribute__((flatten)) void math_probe_kernel(int fn, const double* __restrict__ x,
                                                         const double* __restrict__ y, int n,
                                                         double* __restrict__ out) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    switch (fn) {
        PROBE1(FM3D_PROBE_SIN_CR, fm3d_sin_cr(a));
        PROBE1(FM3D_PROBE_COS_CR, fm3d_cos_cr(a));
        PROBE1(FM3D_PROBE_SINCOS_SEL_CR0, fm3d_sincos_sel_cr(a, 0));
        PROBE1(FM3D_PROBE_SINCOS_SEL_CR1, fm3d_sincos_sel_cr(a, 1));
        PROBE2(FM3D_PROBE_ATAN2_CR, fm3d_atan2_cr(a, b));
        PROBE1(FM3D_PROBE_EXP_CR, fm3d_exp_cr(a));
        PROBE2(FM3D_PROBE_HYPOT_CR, fm3d_hypot_cr(a, b));
        PROBE1(FM3D_PROBE_SIN, fm3d_sin(a));
        PROBE1(FM3D_PROBE_COS, fm3d_cos(a));
        PROBE2(FM3D_PROBE_ATAN2, fm3d_atan2(a, b));
        PROBE1(FM3D_PROBE_ACOS, fm3d_acos(a));
        PROBE1(FM3D_PROBE_EXP, fm3d_exp(a));
        PROBE2(FM3D_PROBE_MDIV, mdiv(a, b, 1.0 / b, mdiv_ok(b)));
        PROBE2(FM3D_PROBE_MDIV_FAST, mdiv_fast(a, b, 1.0 / b));
        PROBE1(FM3D_PROBE_RECIP_Z, recip_z(a));
        PROBE1(FM3D_PROBE_RECIP_Z_LO, recip_z_lo(a));
        PROBE2(FM3D_PROBE_DIV_NN, div_nn(a, b, div_nn_ok(a)));
        PROBE2(FM3D_PROBE_DIV_F64, a / b);
        PROBE1(FM3D_PROBE_SQRT_F64, sqrt(a));
        PROBE2(FM3D_PROBE_DIV_F32, (double)((float)a / (float)b));
        PROBE1(FM3D_PROBE_SQRT_F32, (double)sqrtf((float)a));
        PROBE1(FM3D_PROBE_CV_EXP_SSE, (double)fm3d_cv_exp_sse((float)a));
        PROBE1(FM3D_PROBE_CV_EXP_SCALAR, (double)fm3d_cv_exp_scalar((float)a));
        PROBE2(FM3D_PROBE_CV_ATAN2_DEG, (double)fm3d_cv_atan2_deg((float)a, (float)b));
        PROBE1(FM3D_PROBE_CV_EXP2F, (double)fm3d_cv_exp2f((float)a));
        PROBE1(FM3D_PROBE_CV_ROUNDF, (double)fm3d_cv_roundf((float)a));
        PROBE1(FM3D_PROBE_CV_ROUND, (double)fm3d_cv_round(a));
        PROBE1(FM3D_PROBE_CV_FLOORF, (double)fm3d_cv_floorf((float)a));
        default:
            break;
    }
}

#undef PROBE1
#undef PROBE2

}  // namespace

bool math_probe_binary(int fn) {
    switch (fn) {
        case FM3D_PROBE_ATAN2_CR:
        case FM3D_PROBE_HYPOT_CR:
        case FM3D_PROBE_ATAN2:
        case FM3D_PROBE_MDIV:
        case FM3D_PROBE_MDIV_FAST:
        case FM3D_PROBE_DIV_NN:
        case FM3D_PROBE_DIV_F64:
        case FM3D_PROBE_DIV_F32:
        case FM3D_PROBE_CV_ATAN2_DEG:
            return true;
        default:
            return false;
    }
}

void launch_math_probe(int fn, const double* x, const double* y, int n, double* out, hipStream_t s) {
    if (n <= 0) return;
    math_probe_kernel<<<(n + 255) / 256, 256, 0, s>>>(fn, x, y, n, out);
}

}  // namespace fm3d
