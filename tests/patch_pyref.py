"""An independent restatement of the patch export's geometry -- feature frame -> (R, t) -> pixel -- in
mpmath at 50 digits (tests/test_patch_cases_oracle.py holds the oracle against it).

What the product and the oracle compute (csrc/fm3d_patch.hip frame_camera_kernel + project1,
oracle/fm3d_oracle.c orc_frame_camera + orc_project1) is OpenCV 2.4's cvRodrigues2 round trip of
decomposeTransformation and cvProjectPoints2.  This file shares no code with either: the polar factor
is U V of mpmath.svd_r (not the one-sided Jacobi), acos / sin / cos are mpmath's, and every sum is
taken at 50 digits.  It mirrors only cvRodrigues2's BRANCH DECISIONS -- the thresholds (s < 1e-5,
c > 0, theta < DBL_EPSILON) and the half turn's sign rules -- because those are part of the contract:
a reflection, say, has no rotation vector, and what comes out is what those rules make of it.

A decision on a quantity that is zero in exact arithmetic (the trace of a reflection, an off-diagonal
entry of a diagonal matrix) would hang on the 1e-50 noise of the SVD, so every quantity a decision
looks at is first chopped at 1e-40: far above that noise, and far below anything a frame of doubles
can produce that is not zero (the smallest are squares of ulps, 1e-33).

Only full-rank, finite frames have a unique polar factor; the others are not this file's business.
"""
import sys

import numpy as np

DBL_EPSILON = sys.float_info.epsilon

IDENTITY, HALF, HALF_FLIP, GENERIC = "identity", "half", "half_flip", "generic"


def _mp():
    import mpmath
    return mpmath


def _chop(v):
    mpmath = _mp()
    return mpmath.mpf(0) if abs(v) < mpmath.mpf("1e-40") else v


def frame_camera(F, dps=50):
    """(R (3 x 3 mpmath matrix), t (3 mpf), branch) of one 4 x 4 frame of doubles: the rotation and
    translation cvProjectPoints2 projects with, and the cvRodrigues2 branch that produced it"""
    mpmath = _mp()
    F = np.asarray(F, dtype=np.float64).reshape(4, 4)
    with mpmath.workdps(dps):
        A = mpmath.matrix([[mpmath.mpf(float(F[i, j])) for j in range(3)] for i in range(3)])
        U, _, V = mpmath.svd_r(A)  # A = U diag(S) V
        R = (U * V).apply(_chop)
        # matrix -> vector
        rx, ry, rz = R[2, 1] - R[1, 2], R[0, 2] - R[2, 0], R[1, 0] - R[0, 1]
        s = _chop(mpmath.sqrt((rx * rx + ry * ry + rz * rz) / 4))
        c = _chop((R[0, 0] + R[1, 1] + R[2, 2] - 1) / 2)
        c = min(max(c, mpmath.mpf(-1)), mpmath.mpf(1))
        theta = mpmath.acos(c)
        if s < mpmath.mpf(1e-5):
            if c > 0:
                branch = IDENTITY
                rx = ry = rz = mpmath.mpf(0)
            else:
                branch = HALF
                half = lambda d: mpmath.sqrt(max(_chop((d + 1) / 2), mpmath.mpf(0)))
                rx = half(R[0, 0])
                ry = half(R[1, 1]) * (-1 if R[0, 1] < 0 else 1)
                rz = half(R[2, 2]) * (-1 if R[0, 2] < 0 else 1)
                if abs(rx) < abs(ry) and abs(rx) < abs(rz) and (R[1, 2] > 0) != (ry * rz > 0):
                    branch = HALF_FLIP
                    rz = -rz
                k = theta / mpmath.sqrt(rx * rx + ry * ry + rz * rz)
                rx, ry, rz = rx * k, ry * k, rz * k
        else:
            branch = GENERIC
            k = theta / (2 * s)
            rx, ry, rz = rx * k, ry * k, rz * k
        # vector -> matrix
        theta = mpmath.sqrt(rx * rx + ry * ry + rz * rz)
        if theta < mpmath.mpf(DBL_EPSILON):
            R2 = mpmath.eye(3)
        else:
            a = mpmath.matrix([rx / theta, ry / theta, rz / theta])
            K = mpmath.matrix([[0, -a[2], a[1]], [a[2], 0, -a[0]], [-a[1], a[0], 0]])
            R2 = mpmath.cos(theta) * mpmath.eye(3) + (1 - mpmath.cos(theta)) * (a * a.T) + mpmath.sin(theta) * K
        t = [mpmath.mpf(float(F[i, 3])) for i in range(3)]
        return R2, t, branch


def project(cam, R, t, X, Y, dps=50):
    """cvProjectPoints2 of the plane point (X, Y, 0): z -> 1/z (1 for z == 0), the radial and
    tangential distortion, the intrinsics; (u, v) as mpf"""
    mpmath = _mp()
    with mpmath.workdps(dps):
        X, Y = mpmath.mpf(float(X)), mpmath.mpf(float(Y))
        x = R[0, 0] * X + R[0, 1] * Y + t[0]
        y = R[1, 0] * X + R[1, 1] * Y + t[1]
        z = R[2, 0] * X + R[2, 1] * Y + t[2]
        z = 1 / z if z != 0 else mpmath.mpf(1)
        x, y = x * z, y * z
        k1, k2, p1, p2, k3 = (mpmath.mpf(float(v)) for v in cam.k)
        r2 = x * x + y * y
        cdist = 1 + k1 * r2 + k2 * r2 ** 2 + k3 * r2 ** 3
        xd = x * cdist + p1 * (2 * x * y) + p2 * (r2 + 2 * x * x)
        yd = y * cdist + p1 * (r2 + 2 * y * y) + p2 * (2 * x * y)
        return xd * mpmath.mpf(float(cam.fx)) + mpmath.mpf(float(cam.cx)), \
            yd * mpmath.mpf(float(cam.fy)) + mpmath.mpf(float(cam.cy))


def image_points(cam, F, eps, cmpp, size, index=None):
    """the projections of the reference grid's points (i*size + j, i outer; all of them, or those of
    `index`) through frame F -> ((n, 2) float64, branch).  The grid's coordinates are the doubles the
    reference computes (-eps + inc*i with inc = cmPerPixel * 0.01): they are inputs here, not results."""
    R, t, branch = frame_camera(F)
    inc = cmpp * 0.01
    index = range(size * size) if index is None else index
    out = np.zeros((len(index), 2))
    for n, k in enumerate(index):
        i, j = divmod(int(k), size)
        u, v = project(cam, R, t, -eps + inc * i, -eps + inc * j)
        out[n] = float(u), float(v)
    return out, branch
