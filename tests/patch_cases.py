"""The case table of stage 4's rare branches -- feature frames, the cvRodrigues2 round trip, the
projection and the border rule of the patch export -- shared by tests/test_patch_cases_oracle.py (the
oracle against the 50-digit restatement tests/patch_pyref.py, CPU) and tests/test_gpu_patch_cases.py
(csrc/fm3d_patch.hip against the oracle, bit for bit).  Every case is a pure function of constants.

A case is a name, a group and either a 4 x 4 frame or a (point, normal) pair that computeFeaturesFrames
turns into one.  A group fixes what one device context fixes: the camera and (eps, cmPerPixel).  The
image is image 1 of the synthetic frame pair (640 x 480, no zero pixel) for every group.

rank: FULL (a unique polar factor: the pyref applies), DEFICIENT (a zero singular value: polar3's
random left vectors; oracle against GPU only) or NONFINITE (NaN / inf somewhere in the frame or in
the projection; oracle against GPU only).
branch: the cvRodrigues2 branch a FULL case must take (patch_pyref's names).
tol: the oracle-against-pyref bound in pixels -- 1e-9, or 1e-6 within 1e-5 rad of a half turn, where
acos near -1 turns the few ulps the double polar factor leaves in the trace (<= 1e-15) into
<= sqrt(2e-15) = 4.5e-8 rad, < 5e-7 px at eps = 0.02, Z = 2, fx = 358 (those cases stay at that size).
"""
import dataclasses
import importlib
import math
import sys

import numpy as np

import patch_pyref

DBL_EPSILON = sys.float_info.epsilon
DBL_MIN = sys.float_info.min
FULL, DEFICIENT, NONFINITE = "full", "deficient", "nonfinite"
WIDTH, HEIGHT = 640, 480

# gravity of the CPU test, and the rodriguesIC whose fm3d_gravity is (0, -1, -cos(pi/2)): g0 == 0 and
# g1 == -1 exactly, so the frame cases' cross products meet the same conditions on the device (x = g x n
# is exactly 0 for n parallel to g, exactly (-1, 0, 0) for n = (0, 0, 1))
GRAVITY = (0.0, -1.0, 0.0)
RODRIGUES_IC = (math.pi / 2, 0.0, 0.0)

T0 = (0.05, -0.03, 2.0)


def synth():
    return importlib.import_module("3dfeaturematcher_amd.synth")


def frame_pair():
    """the synthetic pair whose distorted camera and image 1 the cases use"""
    return synth().make_frame_pair(8, seed=11)


def pinhole(fx=256.0, fy=256.0, cx=320.0, cy=240.0):
    return synth().Camera(fx, fy, cx, cy, (0.0, 0.0, 0.0, 0.0, 0.0))


# group -> (camera, eps, cmPerPixel, patch size); camera "synth" = frame_pair().cam
GROUPS = {
    "small": ("synth", 0.02, 0.25, 16),
    "full": ("synth", 0.16, 0.25, 128),
    "pin_small": ("pinhole", 0.02, 0.25, 16),
    "pin_full": ("pinhole", 0.16, 0.25, 128),
    "exact": ("pinhole", 1.0, 25.0, 8),
}


def group_camera(group, pair):
    return pair.cam if GROUPS[group][0] == "synth" else pinhole()


@dataclasses.dataclass
class Case:
    name: str
    group: str
    frame: np.ndarray = None  # (4, 4), or None for a frame case
    point: tuple = None       # frame cases: the point and normal(g) -> the normal
    normal: object = None
    rank: str = FULL
    branch: str = None
    tol: float = 1e-9
    zero_sv: bool = False     # a singular value <= DBL_MIN (polar3's loop runs)
    border: bool = False      # the oracle's inside share must lie in [0.1, 0.9]
    exact: tuple = ()         # coordinates the oracle's image points must contain exactly: ("u", 640.0), ...


def rot(axis, angle):
    """Rodrigues' formula in doubles (the cases are whatever doubles come out: inputs, not results)"""
    a = np.asarray(axis, dtype=np.float64)
    a = a / math.sqrt(float(a @ a))
    K = np.array([[0, -a[2], a[1]], [a[2], 0, -a[0]], [-a[1], a[0], 0]])
    return math.cos(angle) * np.eye(3) + (1 - math.cos(angle)) * np.outer(a, a) + math.sin(angle) * K


def half_turn(a):
    a = np.asarray(a, dtype=np.float64)
    return 2 * np.outer(a, a) - np.eye(3)


def frame(R, t=T0):
    F = np.eye(4)
    F[:3, :3] = R
    F[:3, 3] = t
    return F


AXIS = (0.3, -0.5, 0.8)
_A = np.array([0.48, -0.6, 0.64])  # a unit vector of short doubles

_I, _H, _HF, _G = patch_pyref.IDENTITY, patch_pyref.HALF, patch_pyref.HALF_FLIP, patch_pyref.GENERIC


def rotation_cases():
    c = [
        Case("identity", "small", frame(np.eye(3)), branch=_I),
        Case("half_z", "small", frame(np.diag([-1.0, -1.0, 1.0])), branch=_H, tol=1e-6),
        Case("half_x", "small", frame(np.diag([1.0, -1.0, -1.0])), branch=_H, tol=1e-6),
        Case("half_y", "small", frame(np.diag([-1.0, 1.0, -1.0])), branch=_H, tol=1e-6),
        Case("half_generic_axis", "small", frame(half_turn(_A)), branch=_H, tol=1e-6),
        Case("half_yz_flip", "small", frame(half_turn([0.0, 0.6, -0.8])), branch=_HF, tol=1e-6),
    ]
    for ang, br in ((1e-7, _I), (9e-6, _I), (1.1e-5, _G)):
        c.append(Case(f"small_angle_{ang:g}", "small", frame(rot(AXIS, ang)), branch=br))
    # 1.1e-5 rad from the half turn is outside the 1e-5 within which the looser bound applies
    for d, br, tol in ((1e-7, _H, 1e-6), (9e-6, _H, 1e-6), (1.1e-5, _G, 1e-9)):
        c.append(Case(f"pi_minus_{d:g}", "small", frame(rot(AXIS, math.pi - d)), branch=br, tol=tol))
    shear = np.array([[1.3, 0.2, 0.0], [0.0, 0.8, 0.1], [0.0, 0.0, 1.1]])
    c += [
        Case("generic_1.1", "small", frame(rot(AXIS, 1.1)), branch=_G),
        Case("sheared_scaled", "small", frame(rot(AXIS, 0.7) @ shear), branch=_G),
        # no rotation vector exists: s = 0 and c = 0 exactly, so the half-turn rules make one up
        Case("reflection", "small", frame(np.diag([1.0, 1.0, -1.0])), branch=_H),
        Case("generic_1.1_full", "full", frame(rot(AXIS, 1.1)), branch=_G),  # size*size > 256: grid.x > 1
    ]
    return c


def _cross(g, n):
    return np.array([g[1] * n[2] - g[2] * n[1], g[2] * n[0] - g[0] * n[2], g[0] * n[1] - g[1] * n[0]])


# |g x n| = d for n = g + (d, 0, 0) with g0 == 0 (the products that cancel are the same doubles)
BELOW_EPS, ABOVE_EPS = 2.0e-16, 2.5e-16


def frame_cases():
    """(point, normal) pairs for computeFeaturesFrames; a normal is a function of the gravity vector"""
    k = lambda v: (lambda g: np.array(v, dtype=np.float64))
    F = lambda name, normal, **kw: Case(name, "small", point=T0, normal=normal, **kw)
    return [
        F("n_fronto", k([0.0, 0.0, 1.0]), branch=_H, tol=1e-6),  # the frame diag(-1, -1, 1)
        F("n_fronto_1e-9", k([0.0, 1e-9, 1.0]), branch=_H, tol=1e-6),
        F("n_gravity", lambda g: np.array(g, dtype=np.float64), rank=DEFICIENT, zero_sv=True),
        F("n_2.5_gravity", lambda g: 2.5 * np.array(g), rank=DEFICIENT, zero_sv=True),
        F("n_minus_gravity", lambda g: -np.array(g), rank=DEFICIENT, zero_sv=True),
        F("n_zero", k([0.0, 0.0, 0.0]), rank=DEFICIENT, zero_sv=True),
        F("n_1e-200", k([1e-200, 0.0, 1e-200]), rank=DEFICIENT, zero_sv=True),
        # normalize3's s > DBL_EPSILON, either side
        F("n_below_eps", lambda g: np.array(g) + np.array([BELOW_EPS, 0.0, 0.0]), rank=DEFICIENT, zero_sv=True),
        F("n_above_eps", lambda g: np.array(g) + np.array([ABOVE_EPS, 0.0, 0.0]), branch=_G),
        F("n_nan", k([math.nan, 0.0, 1.0]), rank=NONFINITE),
        F("n_inf", k([math.inf, 0.0, 1.0]), rank=NONFINITE),
    ]


QUARTER_X = np.array([[1.0, 0.0, 0.0], [0.0, 0.0, -1.0], [0.0, 1.0, 0.0]])  # z_cam = Y of the plane point


def projection_cases():
    return [
        # every sample has z == 0: project1 takes 1 for 1/z
        Case("t_z0", "small", frame(np.eye(3), (0.05, -0.03, 0.0)), branch=_I),
        Case("t_behind", "small", frame(np.eye(3), (0.05, -0.03, -2.0)), branch=_I),
        # the plane contains the camera centre: z = Y, exactly 0 in grid row j = 8, +-0.0025 beside it.
        # x/z reaches 8, where the synthetic camera's r^6 term puts points 2e7 px out (an ulp there is
        # 4e-9 px), so the case uses the camera without distortion
        Case("plane_through_centre", "pin_small", frame(QUARTER_X, (0.0, 0.0, 0.0)), branch=_G),
        # z = 1e-60 in row j = 8: x/z = 2e58, r^2 and r^4 finite, r^6 = inf -- cvProjectPoints2's
        # 1 / (1 + 0 r^2 + 0 r^4 + 0 r^6) is NaN there, the kernel's r6 - r6 test
        Case("r6_overflow", "small", frame(QUARTER_X, (0.0, 0.0, 1e-60)), rank=NONFINITE),
    ]


def border_cases():
    """128 x 128 patches straddling every border and corner of the 640 x 480 image.  The synthetic
    camera's radial terms fold the projection back before it reaches the left border or any corner
    (its distorted radius peaks at 0.949 = 340 px, the left border lies 344 px and the corners 370 px
    and more from the principal point; test_distorted_camera_cannot_reach_left_border_or_corners
    asserts it), so those use the camera without distortion."""
    B = lambda name, group, t: Case(name, group, frame(rot(AXIS, 0.05), t), branch=_G, border=True)
    return [
        B("border_right", "full", (2.0, 0.0, 2.0)),
        B("border_bottom", "full", (0.0, 1.5, 2.0)),
        B("border_top", "full", (0.0, -1.74, 2.0)),
        B("border_left", "pin_full", (-2.45, 0.1, 2.0)),
        B("corner_top_left", "pin_full", (-2.45, -1.8, 2.0)),
        B("corner_bottom_left", "pin_full", (-2.55, 1.9, 2.0)),
        B("corner_top_right", "pin_full", (2.45, -1.9, 2.0)),
        B("corner_bottom_right", "pin_full", (2.55, 1.8, 2.0)),
    ]


EXACT_T = ((2.0, 1.6875, 1.0), (1.75, 1.4375, 1.0), (-0.5, -0.1875, 1.0))


def exact_border_cases():
    """identity, z = 1, fx = fy = 256, an 8 x 8 grid of step 0.25: every coordinate is a multiple of 32
    with no rounding anywhere, and samples fall at u == cols, v == rows, u == 0 and v == 0 exactly"""
    hi, lo = (("u", float(WIDTH)), ("v", float(HEIGHT))), (("u", 0.0), ("v", 0.0))
    return [Case(f"exact_border_{n}", "exact", frame(np.eye(3), t), branch=_I, exact=e)
            for n, (t, e) in enumerate(zip(EXACT_T, (hi, hi, lo)))]


def all_cases():
    return rotation_cases() + frame_cases() + projection_cases() + border_cases() + exact_border_cases()


def case_normals(cases, g):
    """(points, normals) of the frame cases among `cases`, for gravity g"""
    fc = [c for c in cases if c.frame is None]
    return np.array([c.point for c in fc], dtype=np.float64), np.array([c.normal(g) for c in fc], dtype=np.float64)


def frames_of(cases, frames_from_normals):
    """(n, 4, 4): the cases' own frames, and for frame cases the rows of frames_from_normals in order"""
    out, k = [], 0
    for c in cases:
        if c.frame is None:
            out.append(frames_from_normals[k])
            k += 1
        else:
            out.append(c.frame)
    return np.array(out, dtype=np.float64).reshape(-1, 4, 4)


def inside(pts, w=WIDTH, h=HEIGHT):
    """isPixelGood(p, 1.0): both borders included"""
    u, v = pts[..., 0], pts[..., 1]
    return (u >= 0) & (u <= w) & (v >= 0) & (v <= h)


def gravity_cross_norm(g, n):
    x = _cross(np.asarray(g, dtype=np.float64), np.asarray(n, dtype=np.float64))
    return math.sqrt(float((x * x).sum()))


def branch_frames():
    """the frames that take each branch, for tests that want them at chosen indices: identity snap,
    half turn with and without the flip, generic, a zero singular value"""
    rank1 = frame(np.array([[0.0, 0.0, 0.0], [0.0, 0.0, -1.0], [0.0, 0.0, 0.0]]))  # x = y = 0, z = g
    return np.array([frame(rot(AXIS, 9e-6)), frame(half_turn([0.0, 0.6, -0.8])), frame(np.diag([-1.0, -1.0, 1.0])),
                     frame(rot(AXIS, 1.1)), rank1])
