// fm3d_algebra.h -- the two host fp64 helpers of fm3d_algebra.cpp that fm3d_host.cpp calls directly
// (private; no HIP, so that fm3d_algebra.cpp builds with a plain host compiler).
#pragma once

namespace fm3d_host {

// decomposeTransformation + cvProjectPoints2's conversion: camera 2's rotation matrix and translation
void camera2_from_g12(const double g12[16], double R2[9], double t2[3]);
// E = [t2]x R2
void epipolar_matrix(const double R2[9], const double t2[3], double E[9]);

}  // namespace fm3d_host
