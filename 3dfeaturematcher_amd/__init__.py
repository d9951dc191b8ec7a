"""3dfeaturematcher_amd -- MI355X-native hot path of caomw/3DFeatureMatcher.

Python mirror of the reference's operator interface for the path
(``DescriptorsMatcher`` / ``SingleCameraTriangulator`` / ``NormalOptimizer``,
``main.cpp:91-155``), bound with ctypes to the C ABI of ``libfm3d.so``
(``include/fm3d.h``).  All compute runs in the HIP kernels of the library; there
is no CPU fallback -- constructing a context without the library or without a
GPU raises ``Fm3dError``.

The package directory name starts with a digit, so import it with
``importlib.import_module("3dfeaturematcher_amd")``.
"""
from __future__ import annotations

import ctypes
import os

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
# FM3D_LIB selects another in-tree build of the same library (A/B performance experiments)
LIB_PATH = os.environ.get("FM3D_LIB") or os.path.join(_HERE, "libfm3d.so")

FM3D_OK = 0
ERR_INVALID, ERR_HIP, ERR_UNSUPPORTED, ERR_NOMEM, ERR_PARSE, ERR_NAN_PLANE = -1, -2, -3, -4, -5, -6
FEAT_SURF, FEAT_ORB, FEAT_SIFT, FEAT_FAST, FEAT_STAR, FEAT_BRISK, FEAT_FREAK, FEAT_MSER, FEAT_OTHER = 0, 1, 2, 3, 4, 5, 6, 7, -1  # fm3d_settings.detectorType / extractorType
DESC_F32, DESC_U8, DESC_BITS = 0, 1, 2
ST_OK, ST_NO_PIXELS, ST_ABORT_BBOX, ST_ABORT_PIX1, ST_ABORT_PIX2, ST_NAN_PLANE, ST_NAN_NORMAL = range(7)

# every symbol include/fm3d.h declares (tests check the library exports all of them)
EXPORTS = (
    "fm3d_settings_default", "fm3d_settings_load", "fm3d_settings_lookup", "fm3d_ctx_create", "fm3d_ctx_destroy", "fm3d_last_error",
    "fm3d_ctx_set_stream", "fm3d_knn2", "fm3d_match_nndr", "fm3d_setg12", "fm3d_g12_from_poses",
    "fm3d_camera2_from_g12", "fm3d_set_g12", "fm3d_get_camera2", "fm3d_triangulate", "fm3d_set_images",
    "fm3d_get_pyramid_level", "fm3d_optimize_normals", "fm3d_pipeline_upload", "fm3d_pipeline_run",
    "fm3d_records_download", "fm3d_pyrdown", "fm3d_neighborhood", "fm3d_undistort", "fm3d_version",
    "fm3d_gravity", "fm3d_features_frames", "fm3d_patch_size", "fm3d_export_patches", "fm3d_square_neighborhoods",
    "fm3d_circular_neighborhoods", "fm3d_surf_detect", "fm3d_surf_compute", "fm3d_extract_descriptors_from_patches", "fm3d_extract_descriptors_from_patches_any", "fm3d_pipeline_run_dlt", "fm3d_pipeline_dlt_download", "fm3d_pipeline_run_ncc",
    "fm3d_pipeline_ncc_download",
    "fm3d_orb_detect", "fm3d_orb_compute", "fm3d_orb_set_pattern", "fm3d_sift_detect", "fm3d_sift_compute",
    "fm3d_sift_pyramid", "fm3d_fast_detect", "fm3d_star_detect", "fm3d_brisk_compute", "fm3d_star_responses", "fm3d_detect", "fm3d_descriptor_info", "fm3d_compute",
    "fm3d_ncc_hypotheses", "fm3d_mgpu_create", "fm3d_mgpu_destroy", "fm3d_mgpu_last_error", "fm3d_mgpu_set_g12",
    "fm3d_mgpu_pipeline_upload", "fm3d_mgpu_pipeline_run", "fm3d_share_queries", "fm3d_merge_shares",
    "fm3d_plane_to_image2", "fm3d_pipeline_submit", "fm3d_pipeline_wait",
    "fm3d_mgpu_submit", "fm3d_mgpu_wait", "fm3d_pipeline_link", "fm3d_freak_compute", "fm3d_freak_set_pairs",
    "fm3d_mser_detect", "fm3d_mser_detect_batch", "fm3d_mser_regions", "fm3d_pipeline_submit_dlt", "fm3d_pipeline_submit_dlt_pair",
    "fm3d_pipeline_submit_ncc", "fm3d_pipeline_wait_ncc", "fm3d_pipeline_wait_dlt", "fm3d_device_count",
    "fm3d_epipolar_matrix", "fm3d_epipolar_lines", "fm3d_knn2_guided", "fm3d_match_nndr_guided",
    "fm3d_match_mutual", "fm3d_match_mutual_guided", "fm3d_math_probe",
    "fm3d_verify_matches", "fm3d_ransac_sample", "fm3d_epipolar_from8", "fm3d_epipolar_null8", "fm3d_epipolar_count",
    "fm3d_pose_from_epipolar",
    "fm3d_verify_matches_refined", "fm3d_epipolar_normal45", "fm3d_epipolar_refit",
    "fm3d_pipeline_run_verified", "fm3d_pipeline_run_dlt_verified",
    "fm3d_pipeline_submit_verified", "fm3d_pipeline_wait_verified", "fm3d_pipeline_submit_dlt_verified",
    "fm3d_pipeline_wait_dlt_verified",
    "fm3d_pipeline_describe",
    "fm3d_pipeline_describe_any", "fm3d_patch_keypoint_kept", "fm3d_patch_keypoint_kept_for",
    "fm3d_align_points", "fm3d_match_models", "fm3d_ransac_sample3", "fm3d_rigid_from3", "fm3d_rigid_count",
    "fm3d_rigid_refit",
    "fm3d_localize_points", "fm3d_localize_model", "fm3d_quartic_roots", "fm3d_p3p", "fm3d_pnp_count", "fm3d_pnp_step",
)

# include/fm3d.h's FM3D_PROBE_* table by position (fm3d_math_probe), and its functions of two arguments
PROBE_FNS = (
    "sin_cr", "cos_cr", "sincos_sel_cr0", "sincos_sel_cr1", "atan2_cr", "exp_cr", "hypot_cr",
    "sin", "cos", "atan2", "acos", "exp",
    "mdiv", "mdiv_fast", "recip_z", "recip_z_lo", "div_nn",
    "div_f64", "sqrt_f64", "div_f32", "sqrt_f32",
    "cv_exp_sse", "cv_exp_scalar", "cv_atan2_deg", "cv_exp2f", "cv_roundf", "cv_round", "cv_floorf",
)
PROBE_BINARY = frozenset(("atan2_cr", "hypot_cr", "atan2", "mdiv", "mdiv_fast", "div_nn", "div_f64", "div_f32",
                          "cv_atan2_deg"))


class Fm3dError(RuntimeError):
    def __init__(self, code, msg=""):
        super().__init__(f"fm3d error {code}: {msg}")
        self.code = code


class Settings(ctypes.Structure):
    """fm3d_settings (the build/settings.yml keys of the path)."""
    _fields_ = [
        ("Fx", ctypes.c_double), ("Fy", ctypes.c_double), ("Cx", ctypes.c_double), ("Cy", ctypes.c_double),
        ("p1", ctypes.c_double), ("p2", ctypes.c_double), ("k0", ctypes.c_double), ("k1", ctypes.c_double),
        ("k2", ctypes.c_double), ("rodriguesIC", ctypes.c_double * 3), ("translationIC", ctypes.c_double * 3),
        ("zThresholdMin", ctypes.c_double), ("zThresholdMax", ctypes.c_double), ("epsilonLMMIN", ctypes.c_double),
        ("pixelsRay", ctypes.c_int), ("pyramids", ctypes.c_int), ("nndrEpsilon", ctypes.c_double),
        ("pos1", ctypes.c_double * 6), ("pos2", ctypes.c_double * 6), ("boundWidth", ctypes.c_int),
        ("boundHeight", ctypes.c_int), ("strictNanExit", ctypes.c_int), ("lmWaves", ctypes.c_int),
        ("neighEpsilon", ctypes.c_double), ("cmPerPixel", ctypes.c_double),
        ("neighMethod", ctypes.c_int), ("neighThetas", ctypes.c_int), ("neighRays", ctypes.c_int),
        ("detectorType", ctypes.c_int), ("extractorType", ctypes.c_int), ("surfHessianThreshold", ctypes.c_double),
        ("surfOctaves", ctypes.c_int), ("surfOctaveLayers", ctypes.c_int), ("surfExtended", ctypes.c_int),
        ("surfUpright", ctypes.c_int),
        ("orbNumFeatures", ctypes.c_int), ("orbScaleFactor", ctypes.c_double), ("orbNumLevels", ctypes.c_int),
        ("orbEdgeThreshold", ctypes.c_int), ("orbPatchSize", ctypes.c_int), ("orbFastThreshold", ctypes.c_int),
        ("siftNumFeatures", ctypes.c_int), ("siftOctaveLayers", ctypes.c_int),
        ("siftContrastThreshold", ctypes.c_double), ("siftEdgeThreshold", ctypes.c_double),
        ("siftSigma", ctypes.c_double),
        ("detectorMode", ctypes.c_int), ("fastThreshold", ctypes.c_int), ("fastNonmax", ctypes.c_int),
        ("adaptiveMinFeatures", ctypes.c_int), ("adaptiveMaxFeatures", ctypes.c_int), ("adaptiveMaxIters", ctypes.c_int),
        ("starMaxSize", ctypes.c_int), ("starResponse", ctypes.c_int), ("starLineThreshold", ctypes.c_int),
        ("starLineBinarized", ctypes.c_int), ("starSuppression", ctypes.c_int),
        ("briskThreshold", ctypes.c_int), ("briskOctaves", ctypes.c_int),
        ("mserDelta", ctypes.c_int), ("mserMinArea", ctypes.c_int), ("mserMaxArea", ctypes.c_int),
        ("mserMaxVariation", ctypes.c_double), ("mserMinDiversity", ctypes.c_double),
        ("mserMaxEvolution", ctypes.c_int), ("mserAreaThreshold", ctypes.c_double),
        ("mserMinMargin", ctypes.c_double), ("mserEdgeBlurSize", ctypes.c_int),
        ("lmReduction", ctypes.c_int),
        ("dltSolver", ctypes.c_int),
        ("guidedMatchPx", ctypes.c_double),
        ("crossCheck", ctypes.c_int),
    ]

    @staticmethod
    def default() -> "Settings":
        s = Settings()
        _check(lib().fm3d_settings_default(ctypes.byref(s)))
        return s

    @staticmethod
    def load(path: str) -> "Settings":
        s = Settings()
        _check(lib().fm3d_settings_load(path.encode(), ctypes.byref(s)))
        return s

    def camera(self):
        """(fx, fy, cx, cy, (k1, k2, p1, p2, k3)) in OpenCV order."""
        return self.Fx, self.Fy, self.Cx, self.Cy, (self.k0, self.k1, self.p1, self.p2, self.k2)

    def set_camera(self, cam) -> None:
        self.Fx, self.Fy, self.Cx, self.Cy = cam.fx, cam.fy, cam.cx, cam.cy
        self.k0, self.k1, self.p1, self.p2, self.k2 = cam.k


DMATCH = np.dtype([("queryIdx", "<i4"), ("trainIdx", "<i4"), ("imgIdx", "<i4"), ("distance", "<f4")])
KEYPOINT = np.dtype([("x", "<f4"), ("y", "<f4"), ("size", "<f4"), ("angle", "<f4"), ("response", "<f4"),
                     ("octave", "<i4"), ("class_id", "<i4")])  # cv::KeyPoint (fm3d_keypoint)
RECORD = np.dtype([("queryIdx", "<i4"), ("trainIdx", "<i4"), ("distance", "<f4"), ("status", "<i4"),
                   ("point", "<f8", (3,)), ("normal", "<f8", (3,))])


class LMStats(ctypes.Structure):
    _fields_ = [("points_in", ctypes.c_int64), ("points_kept", ctypes.c_int64), ("evaluations", ctypes.c_int64),
                ("pixel_evaluations", ctypes.c_int64), ("drops", ctypes.c_int64 * 8), ("kernel_ms", ctypes.c_double),
                ("groups", ctypes.c_int64), ("passes", ctypes.c_int64), ("cycles_terms", ctypes.c_int64),
                ("cycles_chain", ctypes.c_int64), ("cycles_control", ctypes.c_int64), ("cycles_total", ctypes.c_int64),
                ("wall_ticks_sum", ctypes.c_int64), ("wall_ticks_max", ctypes.c_int64),
                ("wall_clock_khz", ctypes.c_int64), ("class_passes", ctypes.c_int64 * 4),
                ("class_cycles", ctypes.c_int64 * 4), ("last_group_start_ticks", ctypes.c_int64),
                ("last_group_end_ticks", ctypes.c_int64), ("cycles_wait", ctypes.c_int64),
                ("chain_rounds", ctypes.c_int64), ("chain_chunks", ctypes.c_int64),
                ("queue_empty_ticks", ctypes.c_int64)]

    def as_dict(self):
        d = {k: getattr(self, k) for k, _ in self._fields_}
        for k in ("drops", "class_passes", "class_cycles"):
            d[k] = list(d[k])
        return d


class PipelineStats(ctypes.Structure):
    _fields_ = [("queries", ctypes.c_int64), ("trains", ctypes.c_int64), ("matches", ctypes.c_int64),
                ("inliers", ctypes.c_int64), ("kept", ctypes.c_int64), ("match_ms", ctypes.c_double),
                ("nndr_ms", ctypes.c_double), ("triangulate_ms", ctypes.c_double), ("pyramid_ms", ctypes.c_double),
                ("lm_ms", ctypes.c_double), ("total_ms", ctypes.c_double), ("lm", LMStats)]

    def as_dict(self):
        d = {k: getattr(self, k) for k, _ in self._fields_ if k != "lm"}
        d["lm"] = self.lm.as_dict()
        return d


class DescribeStats(ctypes.Structure):
    """fm3d_describe_stats (fm3d_pipeline_describe)."""
    _fields_ = [("points", ctypes.c_int64), ("patchSize", ctypes.c_int32), ("cols", ctypes.c_int32),
                ("type", ctypes.c_int32), ("chunks", ctypes.c_int32), ("total_ms", ctypes.c_double)]

    def as_dict(self):
        return {k: getattr(self, k) for k, _ in self._fields_}


DESCRIBE_SOURCES = {"records": 0, "ncc": 1}  # FM3D_DESCRIBE_RECORDS, FM3D_DESCRIBE_NCC


class VerifyOpts(ctypes.Structure):
    """fm3d_verify_opts (fm3d_pipeline_run_verified / fm3d_pipeline_run_dlt_verified)."""
    _fields_ = [("hypotheses", ctypes.c_int32), ("refineIters", ctypes.c_int32), ("maxPx", ctypes.c_double),
                ("seed", ctypes.c_uint64), ("poseFromModel", ctypes.c_int32), ("reserved", ctypes.c_int32),
                ("baseline", ctypes.c_double)]


class VerifyReport(ctypes.Structure):
    """fm3d_verify_report."""
    _fields_ = [("matches", ctypes.c_int32), ("verified", ctypes.c_int32), ("best", ctypes.c_int32),
                ("roundsAdopted", ctypes.c_int32), ("poseInstalled", ctypes.c_int32), ("votes", ctypes.c_int32 * 4),
                ("E", ctypes.c_double * 9), ("g12", ctypes.c_double * 16), ("verify_ms", ctypes.c_double)]

    def as_dict(self):
        d = {k: getattr(self, k) for k, _ in self._fields_}
        d["votes"] = np.array(self.votes, dtype=np.int32)
        d["E"] = np.array(self.E, dtype=np.float64).reshape(3, 3)
        d["g12"] = np.array(self.g12, dtype=np.float64).reshape(4, 4)
        return d


class AlignOpts(ctypes.Structure):
    """fm3d_align_opts (fm3d_align_points / fm3d_match_models)."""
    _fields_ = [("hypotheses", ctypes.c_int32), ("refineIters", ctypes.c_int32), ("maxDist", ctypes.c_double),
                ("minNormalCos", ctypes.c_double), ("seed", ctypes.c_uint64)]


class LocalizeOpts(ctypes.Structure):
    """fm3d_localize_opts (fm3d_localize_points / fm3d_localize_model)."""
    _fields_ = [("samples", ctypes.c_int32), ("refineIters", ctypes.c_int32), ("maxPx", ctypes.c_double),
                ("minFacingCos", ctypes.c_double), ("seed", ctypes.c_uint64)]


def _verified_submit_argtypes(L) -> None:
    """the verified submit / wait calls' signatures (include/fm3d.h); an FM3D_LIB build from before them
    (tools/verify_stream_bench.py's A/B) simply has none to describe"""
    vp, ci, pi = ctypes.c_void_p, ctypes.c_int, ctypes.POINTER(ctypes.c_int)
    po, pr, ps = ctypes.POINTER(VerifyOpts), ctypes.POINTER(VerifyReport), ctypes.POINTER(PipelineStats)
    for name, args in (("fm3d_pipeline_submit_verified", [vp, po, vp, ci, vp, ci, ci, ci, vp, vp, vp, vp, ci, ci]),
                       ("fm3d_pipeline_wait_verified", [vp, vp, ci, pi, ps, pr]),
                       ("fm3d_pipeline_submit_dlt_verified", [vp, po]),
                       ("fm3d_pipeline_wait_dlt_verified", [vp, pi, ps, pr])):
        if hasattr(L, name):
            getattr(L, name).argtypes = args
            getattr(L, name).restype = ctypes.c_int


_LIB = None


def lib():
    """Load libfm3d.so (built by __graft_entry__.build()); raises if absent."""
    global _LIB
    if _LIB is None:
        if not os.path.exists(LIB_PATH):
            raise Fm3dError(ERR_HIP, f"{LIB_PATH} missing: build it with __graft_entry__.build()")
        L = ctypes.CDLL(LIB_PATH)
        L.fm3d_last_error.restype = ctypes.c_char_p
        L.fm3d_version.restype = ctypes.c_char_p
        L.fm3d_mgpu_last_error.restype = ctypes.c_char_p
        _verified_submit_argtypes(L)
        _LIB = L
    return _LIB


def _check(code, ctx=None):
    if code != FM3D_OK:
        msg = ""
        if ctx is not None:
            msg = (lib().fm3d_last_error(ctx) or b"").decode(errors="replace")
        raise Fm3dError(code, msg)


def _ptr(a, t=ctypes.c_double):
    return a.ctypes.data_as(ctypes.POINTER(t))


def _vp(a):
    return ctypes.c_void_p(a.ctypes.data) if a is not None else None


class Context:
    """One fm3d_ctx: device buffers + a HIP stream on one GPU."""

    def __init__(self, settings: Settings | None = None, device: int = 0):
        self.settings = settings if settings is not None else Settings.default()
        self._h = ctypes.c_void_p()
        rc = lib().fm3d_ctx_create(ctypes.byref(self.settings), ctypes.c_int(device), ctypes.byref(self._h))
        if rc != FM3D_OK:
            raise Fm3dError(rc, "fm3d_ctx_create failed (no HIP device / runtime?)")

    @property
    def handle(self):
        return self._h

    def close(self):
        if self._h:
            lib().fm3d_ctx_destroy(self._h)
            self._h = ctypes.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def check(self, code):
        _check(code, self._h)

    def set_stream(self, hip_stream: int | None):
        self.check(lib().fm3d_ctx_set_stream(self._h, ctypes.c_void_p(hip_stream or 0)))


def _desc_type(desc: np.ndarray, binary: bool) -> int:
    if binary:
        return DESC_BITS
    if desc.dtype == np.uint8:
        return DESC_U8
    if desc.dtype == np.float32:
        return DESC_F32
    raise TypeError("descriptors must be uint8 (SIFT-like), float32 or binary uint8 (binary=True)")


def _check_max_px(max_px) -> None:
    """fm3d_knn2_guided's rule, before any device work: finite and > 0."""
    v = float(max_px)
    if not (v > 0.0 and v != float("inf")):
        raise Fm3dError(ERR_INVALID, "maxPx must be finite and > 0")


class DescriptorsMatcher:
    """DescriptorsMatcher (DescriptorsMatcher/descriptorsmatcher.h:39-111), matcher + NNDR part.

    Feature detection/description (descriptorsmatcher.cpp:110-115) is upstream of
    the hot path: this class takes the descriptor matrices directly.
    """

    def __init__(self, ctx: Context, binary: bool = False):
        self.ctx = ctx
        self.binary = binary

    def knn_match(self, desc_a: np.ndarray, desc_b: np.ndarray) -> np.ndarray:
        """knnMatch(A, B, k=2) (descriptorsmatcher.cpp:89-105) -> (nA, 2) DMATCH array."""
        a = np.ascontiguousarray(desc_a)
        b = np.ascontiguousarray(desc_b)
        out = np.zeros((a.shape[0], 2), dtype=DMATCH)
        self.ctx.check(lib().fm3d_knn2(self.ctx.handle, _vp(a), a.shape[0], _vp(b), b.shape[0], a.shape[1],
                                       _desc_type(a, self.binary), _vp(out)))
        return out

    def compareWithNNDRImages(self, epsilon: float, image_a: np.ndarray, image_b: np.ndarray,
                              matches: np.ndarray | None = None):
        """compareWithNNDR (descriptorsmatcher.cpp:107-131) with the detection it starts with: the
        settings' detector + extractor on both images on the GPU (SURF; SIFT; or ORB: detect, then
        compute on the detected keypoints as the reference's two calls, Hamming matching as its binary
        extractor types select, :64), knnMatch, NNDR.  Returns (matches appended as the reference
        does, kpts_a, kpts_b, desc_a, desc_b)."""
        S = self.ctx.settings
        if S.detectorMode == 1 or S.detectorType in (FEAT_SIFT, FEAT_FAST, FEAT_STAR) or S.extractorType != S.detectorType:
            # the reference's two calls with any detector / extractor pair built here (fm3d_detect,
            # fm3d_compute): detect, then compute on the detected keypoints
            feats = Features(self.ctx)
            ka, _, da = feats.compute(image_a, feats.detect(image_a))
            kb, _, db = feats.compute(image_b, feats.detect(image_b))
            binary = S.extractorType in (FEAT_ORB, FEAT_BRISK, FEAT_FREAK)
            m = DescriptorsMatcher(self.ctx, binary=binary).compareWithNNDR(epsilon, da, db, matches)
            return m, ka, kb, da, db
        if S.detectorType == FEAT_ORB and S.extractorType == FEAT_ORB:
            orb = ORB(self.ctx)
            ka, _, da = orb.compute(image_a, orb.detect(image_a))
            kb, _, db = orb.compute(image_b, orb.detect(image_b))
            m = DescriptorsMatcher(self.ctx, binary=True).compareWithNNDR(epsilon, da, db, matches)
            return m, ka, kb, da, db
        surf = SURF(self.ctx)
        ka, da = surf.detect(image_a, with_descriptors=True)
        kb, db = surf.detect(image_b, with_descriptors=True)
        m = self.compareWithNNDR(epsilon, da, db, matches)
        return m, ka, kb, da, db

    def compareWithNNDR(self, epsilon: float, desc_a: np.ndarray, desc_b: np.ndarray,
                        matches: np.ndarray | None = None) -> np.ndarray:
        """compareWithNNDR (descriptorsmatcher.cpp:107-131).  Like the reference, new
        matches are APPENDED to `matches` (the reference pushes back without clearing)."""
        a = np.ascontiguousarray(desc_a)
        b = np.ascontiguousarray(desc_b)
        out = np.zeros(max(a.shape[0], 1), dtype=DMATCH)
        n = ctypes.c_int(0)
        self.ctx.check(lib().fm3d_match_nndr(self.ctx.handle, _vp(a), a.shape[0], _vp(b), b.shape[0], a.shape[1],
                                             _desc_type(a, self.binary), ctypes.c_double(epsilon), _vp(out),
                                             ctypes.byref(n)))
        new = out[:n.value].copy()
        return new if matches is None else np.concatenate([matches, new])

    def knn_match_guided(self, desc_a: np.ndarray, desc_b: np.ndarray, kp1: np.ndarray, kp2: np.ndarray,
                         max_px: float) -> np.ndarray:
        """knn_match over the train rows whose keypoint lies within max_px pixels of the query
        keypoint's epipolar line under the context's g12 (fm3d_knn2_guided) -> (nA, 2) DMATCH array,
        trainIdx -1 where fewer than two rows pass."""
        a = np.ascontiguousarray(desc_a)
        b = np.ascontiguousarray(desc_b)
        k1 = np.ascontiguousarray(kp1, dtype=np.float32).reshape(-1, 2)
        k2 = np.ascontiguousarray(kp2, dtype=np.float32).reshape(-1, 2)
        if k1.shape[0] != a.shape[0] or k2.shape[0] != b.shape[0]:
            raise ValueError("one keypoint per descriptor row")
        _check_max_px(max_px)
        out = np.zeros((a.shape[0], 2), dtype=DMATCH)
        self.ctx.check(lib().fm3d_knn2_guided(self.ctx.handle, _vp(a), a.shape[0], _vp(b), b.shape[0], a.shape[1],
                                              _desc_type(a, self.binary), _vp(k1), _vp(k2), ctypes.c_double(max_px),
                                              _vp(out)))
        return out

    def compareWithNNDRGuided(self, epsilon: float, desc_a: np.ndarray, desc_b: np.ndarray, kp1: np.ndarray,
                              kp2: np.ndarray, max_px: float, matches: np.ndarray | None = None) -> np.ndarray:
        """compareWithNNDR over the rows that pass knn_match_guided's gate.  A query with a single
        row on its line is dropped, as the reference's size() >= 2 rule drops it.  New matches are
        appended to `matches`, as compareWithNNDR appends them."""
        a = np.ascontiguousarray(desc_a)
        b = np.ascontiguousarray(desc_b)
        k1 = np.ascontiguousarray(kp1, dtype=np.float32).reshape(-1, 2)
        k2 = np.ascontiguousarray(kp2, dtype=np.float32).reshape(-1, 2)
        if k1.shape[0] != a.shape[0] or k2.shape[0] != b.shape[0]:
            raise ValueError("one keypoint per descriptor row")
        _check_max_px(max_px)
        out = np.zeros(max(a.shape[0], 1), dtype=DMATCH)
        n = ctypes.c_int(0)
        self.ctx.check(lib().fm3d_match_nndr_guided(self.ctx.handle, _vp(a), a.shape[0], _vp(b), b.shape[0],
                                                    a.shape[1], _desc_type(a, self.binary), _vp(k1), _vp(k2),
                                                    ctypes.c_double(epsilon), ctypes.c_double(max_px), _vp(out),
                                                    ctypes.byref(n)))
        new = out[:n.value].copy()
        return new if matches is None else np.concatenate([matches, new])

    def compareWithNNDRMutual(self, epsilon: float, desc_a: np.ndarray, desc_b: np.ndarray, mode: int = 1,
                              matches: np.ndarray | None = None) -> np.ndarray:
        """compareWithNNDR with the cross-check (fm3d_match_mutual): mode 1 keeps a match (i, j) only
        when query i is also the nearest query of train row j; mode 2 also asks row j's two nearest
        queries to pass the ratio test.  New matches are appended to `matches`."""
        a = np.ascontiguousarray(desc_a)
        b = np.ascontiguousarray(desc_b)
        if mode not in (1, 2):
            raise Fm3dError(ERR_INVALID, "mode must be 1 (mutual nearest) or 2 (symmetric ratio)")
        out = np.zeros(max(a.shape[0], 1), dtype=DMATCH)
        n = ctypes.c_int(0)
        self.ctx.check(lib().fm3d_match_mutual(self.ctx.handle, _vp(a), a.shape[0], _vp(b), b.shape[0], a.shape[1],
                                               _desc_type(a, self.binary), ctypes.c_double(epsilon), int(mode),
                                               _vp(out), ctypes.byref(n)))
        new = out[:n.value].copy()
        return new if matches is None else np.concatenate([matches, new])

    def compareWithNNDRMutualGuided(self, epsilon: float, desc_a: np.ndarray, desc_b: np.ndarray, kp1: np.ndarray,
                                    kp2: np.ndarray, max_px: float, mode: int = 1,
                                    matches: np.ndarray | None = None) -> np.ndarray:
        """compareWithNNDRMutual over the pairs that pass knn_match_guided's gate, in both directions
        (fm3d_match_mutual_guided)."""
        a = np.ascontiguousarray(desc_a)
        b = np.ascontiguousarray(desc_b)
        k1 = np.ascontiguousarray(kp1, dtype=np.float32).reshape(-1, 2)
        k2 = np.ascontiguousarray(kp2, dtype=np.float32).reshape(-1, 2)
        if k1.shape[0] != a.shape[0] or k2.shape[0] != b.shape[0]:
            raise ValueError("one keypoint per descriptor row")
        _check_max_px(max_px)
        if mode not in (1, 2):
            raise Fm3dError(ERR_INVALID, "mode must be 1 (mutual nearest) or 2 (symmetric ratio)")
        out = np.zeros(max(a.shape[0], 1), dtype=DMATCH)
        n = ctypes.c_int(0)
        self.ctx.check(lib().fm3d_match_mutual_guided(self.ctx.handle, _vp(a), a.shape[0], _vp(b), b.shape[0],
                                                      a.shape[1], _desc_type(a, self.binary), _vp(k1), _vp(k2),
                                                      ctypes.c_double(epsilon), ctypes.c_double(max_px), int(mode),
                                                      _vp(out), ctypes.byref(n)))
        new = out[:n.value].copy()
        return new if matches is None else np.concatenate([matches, new])


class SURF:
    """The settings' SURF detector / extractor (DescriptorsMatcher::generateDetector /
    generateExtractor, descriptorsmatcher.cpp:176-359; OpenCV 2.4 nonfree SURF, upright) on the GPU."""

    def __init__(self, ctx: Context):
        self.ctx = ctx

    @property
    def descriptorSize(self) -> int:
        return 128 if self.ctx.settings.surfExtended else 64

    def detect(self, image: np.ndarray, with_descriptors: bool = False):
        """FeatureDetector::detect (descriptorsmatcher.cpp:110-111): KEYPOINT records in
        KeypointGreater order; with_descriptors: (keypoints, descriptors) of the same call."""
        img = np.ascontiguousarray(image, dtype=np.uint8)
        h, w = img.shape
        # one detection with room for one keypoint per 64 pixels; again only if more were found
        cap = max(4096, w * h // 64)
        while True:
            k = np.zeros(cap, dtype=KEYPOINT)
            d = np.zeros((cap, self.descriptorSize), dtype=np.float32) if with_descriptors else None
            n = ctypes.c_int(0)
            self.ctx.check(lib().fm3d_surf_detect(self.ctx.handle, _ptr(img, ctypes.c_uint8), w, h, _vp(k), cap,
                                                  ctypes.byref(n), _ptr(d, ctypes.c_float) if d is not None else None))
            if n.value <= cap:
                break
            cap = n.value
        k = k[:n.value]
        return (k, d[:n.value]) if with_descriptors else k

    def compute(self, image: np.ndarray, keypoints: np.ndarray):
        """DescriptorExtractor::compute (descriptorsmatcher.cpp:113-114): (kept keypoints, input index
        of each, descriptors float32 n x 128|64)."""
        img = np.ascontiguousarray(image, dtype=np.uint8)
        h, w = img.shape
        kin = np.ascontiguousarray(keypoints, dtype=KEYPOINT)
        n = len(kin)
        kout = np.zeros(max(n, 1), dtype=KEYPOINT)
        kept = np.zeros(max(n, 1), dtype=np.int32)
        desc = np.zeros((max(n, 1), self.descriptorSize), dtype=np.float32)
        m = ctypes.c_int(0)
        self.ctx.check(lib().fm3d_surf_compute(self.ctx.handle, _ptr(img, ctypes.c_uint8), w, h, _vp(kin), n,
                                               _vp(kout), _ptr(kept, ctypes.c_int32), ctypes.byref(m),
                                               _ptr(desc, ctypes.c_float)))
        return kout[:m.value], kept[:m.value], desc[:m.value]

    def extractDescriptorsFromPatches(self, patches: np.ndarray) -> np.ndarray:
        """DescriptorsMatcher::extractDescriptorsFromPatches (descriptorsmatcher.cpp:133-174): one
        keypoint per square patch at (floor(size/2), floor(size/2)), size = the patch edge, angle -1,
        then the extractor: (P, 128|64) float32."""
        P = np.ascontiguousarray(patches, dtype=np.uint8)
        if P.ndim != 3 or P.shape[1] != P.shape[2]:
            raise ValueError("patches: (P, size, size) uint8")
        out = np.zeros((max(P.shape[0], 1), self.descriptorSize), dtype=np.float32)
        self.ctx.check(lib().fm3d_extract_descriptors_from_patches(self.ctx.handle, _ptr(P, ctypes.c_uint8),
                                                                   P.shape[0], P.shape[1], _ptr(out, ctypes.c_float)))
        return out[:P.shape[0]]


class ORB:
    """The settings' ORB detector / extractor (FeatureOptions DetectorType / ExtractorType ORB,
    descriptorsmatcher.cpp:273-279, 336-341: cv::ORB(NumFeatures, ScaleFactor, NumLevels) of OpenCV
    2.4) on the GPU.  Descriptors are 32 bytes (Hamming)."""

    descriptorSize = 32

    def __init__(self, ctx: Context):
        self.ctx = ctx

    def set_pattern(self, xy) -> None:
        """the 512 rBRIEF test points (OpenCV's bit_pattern_31_ for patchSize 31); None: the default
        makeRandomPattern(orbPatchSize)"""
        if xy is None:
            self.ctx.check(lib().fm3d_orb_set_pattern(self.ctx.handle, None, 0))
            return
        p = np.ascontiguousarray(xy, dtype=np.int32).reshape(-1)
        if p.size != 1024:
            raise ValueError("pattern: 512 (x, y) points")
        self.ctx.check(lib().fm3d_orb_set_pattern(self.ctx.handle, _ptr(p, ctypes.c_int32), 512))

    def detect(self, image: np.ndarray, with_descriptors: bool = False):
        """FeatureDetector::detect (descriptorsmatcher.cpp:110-111): KEYPOINT records, level-major;
        with_descriptors: (keypoints, (n, 32) uint8) of ORB::operator()'s one call"""
        img = np.ascontiguousarray(image, dtype=np.uint8)
        h, w = img.shape
        cap = max(1024, self.ctx.settings.orbNumFeatures * 2)
        while True:
            k = np.zeros(cap, dtype=KEYPOINT)
            d = np.zeros((cap, 32), dtype=np.uint8) if with_descriptors else None
            n = ctypes.c_int(0)
            self.ctx.check(lib().fm3d_orb_detect(self.ctx.handle, _ptr(img, ctypes.c_uint8), w, h, _vp(k), cap,
                                                 ctypes.byref(n), _ptr(d, ctypes.c_uint8) if d is not None else None))
            if n.value <= cap:
                break
            cap = n.value
        k = k[:n.value]
        return (k, d[:n.value]) if with_descriptors else k

    def compute(self, image: np.ndarray, keypoints: np.ndarray):
        """DescriptorExtractor::compute (descriptorsmatcher.cpp:113-114): (kept keypoints level-major,
        input index of each, (m, 32) uint8)"""
        img = np.ascontiguousarray(image, dtype=np.uint8)
        h, w = img.shape
        kin = np.ascontiguousarray(keypoints, dtype=KEYPOINT)
        n = len(kin)
        kout = np.zeros(max(n, 1), dtype=KEYPOINT)
        kept = np.zeros(max(n, 1), dtype=np.int32)
        desc = np.zeros((max(n, 1), 32), dtype=np.uint8)
        m = ctypes.c_int(0)
        self.ctx.check(lib().fm3d_orb_compute(self.ctx.handle, _ptr(img, ctypes.c_uint8), w, h, _vp(kin), n, _vp(kout),
                                              _ptr(kept, ctypes.c_int32), ctypes.byref(m), _ptr(desc, ctypes.c_uint8)))
        return kout[:m.value], kept[:m.value], desc[:m.value]


class SIFT:
    """The settings' SIFT detector / extractor (FeatureOptions DetectorType / ExtractorType SIFT,
    descriptorsmatcher.cpp:243-257, 302-315: cv::SIFT(NumFeatures, NumOctaveLayers, ContrastThreshold,
    EdgeThreshold, Sigma) of OpenCV 2.4 nonfree) on the GPU.  Descriptors are 128 floats holding the
    integers 0..255 (the matcher takes them on its exact integer path)."""

    descriptorSize = 128

    def __init__(self, ctx: Context):
        self.ctx = ctx

    def detect(self, image: np.ndarray, with_descriptors: bool = False):
        """FeatureDetector::detect (descriptorsmatcher.cpp:110-111): KEYPOINT records in the
        reference's order; with_descriptors: (keypoints, (n, 128) float32) -- the extractor's compute
        on the same image"""
        img = np.ascontiguousarray(image, dtype=np.uint8)
        h, w = img.shape
        cap = max(4096, self.ctx.settings.siftNumFeatures * 2)
        while True:
            k = np.zeros(cap, dtype=KEYPOINT)
            d = np.zeros((cap, 128), dtype=np.float32) if with_descriptors else None
            n = ctypes.c_int(0)
            self.ctx.check(lib().fm3d_sift_detect(self.ctx.handle, _ptr(img, ctypes.c_uint8), w, h, _vp(k), cap,
                                                  ctypes.byref(n), _ptr(d, ctypes.c_float) if d is not None else None))
            if n.value <= cap:
                break
            cap = n.value
        k = k[:n.value]
        return (k, d[:n.value]) if with_descriptors else k

    def pyramid(self, image: np.ndarray, first_octave: int = -1, octaves: int | None = None, dog: bool = False):
        """buildGaussianPyramid (dog False) / buildDoGPyramid levels, octave-major: float32 images"""
        img = np.ascontiguousarray(image, dtype=np.uint8)
        h, w = img.shape
        if octaves is None:
            bw, bh = (2 * w, 2 * h) if first_octave < 0 else (w, h)
            octaves = int(np.rint(np.log(min(bw, bh)) / np.log(2.0) - 2)) - first_octave
        nl = octaves * (self.ctx.settings.siftOctaveLayers + (2 if dog else 3))
        sizes = np.zeros(2 * nl, dtype=np.int32)
        tot = ctypes.c_int64(0)
        args = (self.ctx.handle, _ptr(img, ctypes.c_uint8), w, h, first_octave, octaves, 1 if dog else 0)
        self.ctx.check(lib().fm3d_sift_pyramid(*args, None, _ptr(sizes, ctypes.c_int32), ctypes.byref(tot)))
        out = np.zeros(max(tot.value, 1), dtype=np.float32)
        self.ctx.check(lib().fm3d_sift_pyramid(*args, _ptr(out, ctypes.c_float), None, ctypes.byref(tot)))
        levels, o = [], 0
        for i in range(nl):
            lw, lh = int(sizes[2 * i]), int(sizes[2 * i + 1])
            levels.append(out[o:o + lw * lh].reshape(lh, lw))
            o += lw * lh
        return levels

    def compute(self, image: np.ndarray, keypoints: np.ndarray):
        """DescriptorExtractor::compute (descriptorsmatcher.cpp:113-114): (kept keypoints, input index
        of each, (m, 128) float32)"""
        img = np.ascontiguousarray(image, dtype=np.uint8)
        h, w = img.shape
        kin = np.ascontiguousarray(keypoints, dtype=KEYPOINT)
        n = len(kin)
        kout = np.zeros(max(n, 1), dtype=KEYPOINT)
        kept = np.zeros(max(n, 1), dtype=np.int32)
        desc = np.zeros((max(n, 1), 128), dtype=np.float32)
        m = ctypes.c_int(0)
        self.ctx.check(lib().fm3d_sift_compute(self.ctx.handle, _ptr(img, ctypes.c_uint8), w, h, _vp(kin), n,
                                               _vp(kout), _ptr(kept, ctypes.c_int32), ctypes.byref(m),
                                               _ptr(desc, ctypes.c_float)))
        return kout[:m.value], kept[:m.value], desc[:m.value]

    extractDescriptorsFromPatches = SURF.extractDescriptorsFromPatches  # the C ABI picks the settings' extractor


class Features:
    """The settings' detector and extractor, whatever their types (descriptorsmatcher.cpp:176-359):
    STATIC SURF / ORB / SIFT / FAST / STAR or ADAPTIVE FAST / SURF / STAR detection (fm3d_detect), SURF / SIFT / ORB / BRISK /
    FREAK description (fm3d_compute) on any keypoints."""

    def __init__(self, ctx: Context):
        self.ctx = ctx

    def descriptor_info(self):
        """(columns, numpy dtype) of the extractor's rows"""
        cols, typ = ctypes.c_int(0), ctypes.c_int(0)
        self.ctx.check(lib().fm3d_descriptor_info(self.ctx.handle, ctypes.byref(cols), ctypes.byref(typ)))
        return cols.value, (np.uint8 if typ.value == DESC_BITS else np.float32)

    def detect(self, image: np.ndarray) -> np.ndarray:
        """feature_detector_->detect (descriptorsmatcher.cpp:110-111): KEYPOINT records"""
        img = np.ascontiguousarray(image, dtype=np.uint8)
        h, w = img.shape
        cap = 4096
        while True:
            k = np.zeros(cap, dtype=KEYPOINT)
            n = ctypes.c_int(0)
            self.ctx.check(lib().fm3d_detect(self.ctx.handle, _ptr(img, ctypes.c_uint8), w, h, _vp(k), cap,
                                             ctypes.byref(n)))
            if n.value <= cap:
                return k[:n.value]
            cap = n.value

    def compute(self, image: np.ndarray, keypoints: np.ndarray):
        """descriptor_extractor_->compute (descriptorsmatcher.cpp:113-114): (kept keypoints, input index
        of each, descriptor rows)"""
        img = np.ascontiguousarray(image, dtype=np.uint8)
        h, w = img.shape
        cols, dt = self.descriptor_info()
        kin = np.ascontiguousarray(keypoints, dtype=KEYPOINT)
        n = len(kin)
        kout = np.zeros(max(n, 1), dtype=KEYPOINT)
        kept = np.zeros(max(n, 1), dtype=np.int32)
        desc = np.zeros((max(n, 1), cols), dtype=dt)
        m = ctypes.c_int(0)
        self.ctx.check(lib().fm3d_compute(self.ctx.handle, _ptr(img, ctypes.c_uint8), w, h, _vp(kin), n, _vp(kout),
                                          _ptr(kept, ctypes.c_int32), ctypes.byref(m), _vp(desc)))
        return kout[:m.value], kept[:m.value], desc[:m.value]

    def patch_keypoint_kept(self, size: int) -> bool:
        """fm3d_patch_keypoint_kept: whether the settings' extractor keeps the centred keypoint of a
        size x size patch (extractDescriptorsFromPatches' keypoint); one answer for every patch of a size"""
        kept = ctypes.c_int(0)
        self.ctx.check(lib().fm3d_patch_keypoint_kept(self.ctx.handle, int(size), ctypes.byref(kept)))
        return bool(kept.value)

    def set_freak_pairs(self, pairs=None):
        """fm3d_freak_set_pairs: FREAK's 512 selected pairs (indices into the 903 point pairs); None restores
        the default table (include/fm3d_freak.h)"""
        if pairs is None:
            self.ctx.check(lib().fm3d_freak_set_pairs(self.ctx.handle, None, 0))
        else:
            a = np.ascontiguousarray(pairs, dtype=np.int32)
            self.ctx.check(lib().fm3d_freak_set_pairs(self.ctx.handle, _ptr(a, ctypes.c_int32), len(a)))

    def fast(self, image: np.ndarray, threshold: int = 10, nonmax: bool = True) -> np.ndarray:
        """cv::FastFeatureDetector(threshold, nonmax).detect: KEYPOINT records in raster order"""
        img = np.ascontiguousarray(image, dtype=np.uint8)
        h, w = img.shape
        cap = 4096
        while True:
            k = np.zeros(cap, dtype=KEYPOINT)
            n = ctypes.c_int(0)
            self.ctx.check(lib().fm3d_fast_detect(self.ctx.handle, _ptr(img, ctypes.c_uint8), w, h, threshold,
                                                  1 if nonmax else 0, _vp(k), cap, ctypes.byref(n)))
            if n.value <= cap:
                return k[:n.value]
            cap = n.value


    def extractDescriptorsFromPatches(self, patches: np.ndarray) -> np.ndarray:
        """DescriptorsMatcher::extractDescriptorsFromPatches (descriptorsmatcher.cpp:133-174) with any of
        the settings' extractors: (P, cols) rows of the extractor's type (zero rows where the extractor
        drops the centred keypoint)"""
        P = np.ascontiguousarray(patches, dtype=np.uint8)
        if P.ndim != 3 or P.shape[1] != P.shape[2]:
            raise ValueError("patches must be (P, size, size)")
        cols, dt = self.descriptor_info()
        out = np.zeros((P.shape[0], cols), dtype=dt)
        self.ctx.check(lib().fm3d_extract_descriptors_from_patches_any(self.ctx.handle, _ptr(P, ctypes.c_uint8),
                                                                       P.shape[0], P.shape[1], _vp(out)))
        return out

    def star(self, image: np.ndarray, max_size: int = 45, response: int = 30, line_threshold: int = 10,
             line_binarized: int = 8, suppression: int = 5) -> np.ndarray:
        """cv::StarFeatureDetector(maxSize, response, lineThreshold, lineBinarized, suppression).detect:
        KEYPOINT records in tile order"""
        img = np.ascontiguousarray(image, dtype=np.uint8)
        h, w = img.shape
        cap = 4096
        while True:
            k = np.zeros(cap, dtype=KEYPOINT)
            n = ctypes.c_int(0)
            self.ctx.check(lib().fm3d_star_detect(self.ctx.handle, _ptr(img, ctypes.c_uint8), w, h, max_size, response,
                                                  line_threshold, line_binarized, suppression, _vp(k), cap,
                                                  ctypes.byref(n)))
            if n.value <= cap:
                return k[:n.value]
            cap = n.value


    def star_responses(self, image: np.ndarray, max_size: int = 45):
        """StarDetectorComputeResponses: (border, float32 responses, int16 signed sizes)"""
        img = np.ascontiguousarray(image, dtype=np.uint8)
        h, w = img.shape
        R = np.zeros((h, w), np.float32)
        Z = np.zeros((h, w), np.int16)
        b = ctypes.c_int(0)
        self.ctx.check(lib().fm3d_star_responses(self.ctx.handle, _ptr(img, ctypes.c_uint8), w, h, max_size,
                                                 _ptr(R, ctypes.c_float), _ptr(Z, ctypes.c_int16), ctypes.byref(b)))
        return b.value, R, Z

    def mser(self, image: np.ndarray, delta: int = 5, min_area: int = 60, max_area: int = 14400,
             max_variation: float = 0.25, min_diversity: float = 0.2) -> np.ndarray:
        """cv::MserFeatureDetector(delta, minArea, maxArea, maxVariation, minDiversity, ...).detect:
        KEYPOINT records in region order"""
        img = np.ascontiguousarray(image, dtype=np.uint8)
        h, w = img.shape
        cap = 4096
        while True:
            k = np.zeros(cap, dtype=KEYPOINT)
            n = ctypes.c_int(0)
            self.ctx.check(lib().fm3d_mser_detect(self.ctx.handle, _ptr(img, ctypes.c_uint8), w, h, delta, min_area,
                                                  max_area, ctypes.c_double(max_variation),
                                                  ctypes.c_double(min_diversity), _vp(k), cap, ctypes.byref(n)))
            if n.value <= cap:
                return k[:n.value]
            cap = n.value

    def mser_batch(self, images, delta: int = 5, min_area: int = 60, max_area: int = 14400,
                   max_variation: float = 0.25, min_diversity: float = 0.2):
        """mser() on several images of one size in one call (fm3d_mser_detect_batch: every image's floods
        side by side): a list of KEYPOINT arrays, each equal to mser(image)"""
        imgs = np.ascontiguousarray(np.stack([np.asarray(i, dtype=np.uint8) for i in images]))
        count, h, w = imgs.shape
        cap = 4096 * count
        counts = np.zeros(count, np.int32)
        while True:
            k = np.zeros(cap, dtype=KEYPOINT)
            tot = ctypes.c_int(0)
            self.ctx.check(lib().fm3d_mser_detect_batch(
                self.ctx.handle, _ptr(imgs, ctypes.c_uint8), count, w, h, delta, min_area, max_area,
                ctypes.c_double(max_variation), ctypes.c_double(min_diversity), _vp(k), cap,
                _ptr(counts, ctypes.c_int32), ctypes.byref(tot)))
            if tot.value <= cap:
                break
            cap = tot.value
        out, off = [], 0
        for c in counts:
            out.append(k[off:off + int(c)].copy())
            off += int(c)
        return out

    def mser_regions(self, image: np.ndarray, delta: int = 5, min_area: int = 60, max_area: int = 14400,
                     max_variation: float = 0.25, min_diversity: float = 0.2):
        """MSER::operator()(img, msers): [(colour -1 | +1, (k, 2) int32 points (x, y) in region-list order)]"""
        img = np.ascontiguousarray(image, dtype=np.uint8)
        h, w = img.shape
        cap, pcap = 1024, 1 << 18
        while True:
            color = np.zeros(cap, np.int32)
            count = np.zeros(cap, np.int32)
            pts = np.zeros((pcap, 2), np.int32)
            nr, npt = ctypes.c_int(0), ctypes.c_int64(0)
            self.ctx.check(lib().fm3d_mser_regions(
                self.ctx.handle, _ptr(img, ctypes.c_uint8), w, h, delta, min_area, max_area,
                ctypes.c_double(max_variation), ctypes.c_double(min_diversity), _ptr(color, ctypes.c_int32),
                _ptr(count, ctypes.c_int32), cap, _ptr(pts, ctypes.c_int32), ctypes.c_int64(pcap), ctypes.byref(nr),
                ctypes.byref(npt)))
            if nr.value <= cap and npt.value <= pcap:
                break
            cap, pcap = max(cap, nr.value), max(pcap, npt.value)
        out, off = [], 0
        for i in range(nr.value):
            out.append((int(color[i]), pts[off:off + count[i]].copy()))
            off += int(count[i])
        return out


class SingleCameraTriangulator:
    """SingleCameraTriangulator (Triangulator/singlecameratriangulator.h:52-93), hot-path methods."""

    def __init__(self, ctx: Context):
        self.ctx = ctx
        self._kp1 = self._kp2 = self._matches = None

    def setg12(self, T1, T2, r1, r2) -> np.ndarray:
        g = np.zeros(16)
        f64 = lambda v: np.ascontiguousarray(v, dtype=np.float64)
        self.ctx.check(lib().fm3d_setg12(self.ctx.handle, _ptr(f64(T1)), _ptr(f64(T2)), _ptr(f64(r1)),
                                         _ptr(f64(r2)), _ptr(g)))
        return g.reshape(4, 4)

    def set_g12(self, g12) -> None:
        self.ctx.check(lib().fm3d_set_g12(self.ctx.handle, _ptr(np.ascontiguousarray(g12, dtype=np.float64))))

    def camera2(self):
        R2 = np.zeros(9)
        t2 = np.zeros(3)
        self.ctx.check(lib().fm3d_get_camera2(self.ctx.handle, _ptr(R2), _ptr(t2)))
        return R2.reshape(3, 3), t2

    def epipolar_lines(self, kp1) -> np.ndarray:
        """fm3d_epipolar_lines: the unit-normal epipolar line (a, b, c, 0) in camera 2's undistorted
        normalised plane of every image-1 keypoint -> (n, 4) float32; (0, 0, inf, 0) for a
        degenerate line."""
        k1 = np.ascontiguousarray(kp1, dtype=np.float32).reshape(-1, 2)
        out = np.zeros((k1.shape[0], 4), dtype=np.float32)
        self.ctx.check(lib().fm3d_epipolar_lines(self.ctx.handle, _vp(k1), k1.shape[0], _vp(out)))
        return out

    def verifyMatches(self, kp1, kp2, matches, max_px, hypotheses: int = 1024, seed: int = 0, debug: bool = False,
                      refine: int = 0):
        """fm3d_verify_matches: a RANSAC fit of the essential matrix to the matches,
        `hypotheses` eight-point models scored against every match within max_px pixels -> (E (3, 3),
        mask (K,) bool, inliers (DMATCH, input order), best); with debug also counts (H,) int32 (-1 for an
        invalid hypothesis) and models (H, 3, 3).  No valid model: a zero E, no inliers, best -1.  Uses
        the camera of the context's settings, not g12.
        refine (0 .. 16, fm3d_verify_matches_refined): that many rounds of a least-squares refit of the
        best model on its own inliers, each adopted iff valid and no worse in count; E, mask and inliers
        are the final model's.  With refine > 0 and debug three more: roundCounts (refine + 1,) int32
        (c_0, then each round's count: -1 an invalid refit, -2 a round not run), roundModels
        (refine, 3, 3) and the number of rounds adopted."""
        _check_max_px(max_px)
        H = int(hypotheses)
        if H < 1:
            raise Fm3dError(ERR_INVALID, "hypotheses must be >= 1")
        R = int(refine)
        if not 0 <= R <= 16:
            raise Fm3dError(ERR_INVALID, "refine must be in 0 .. 16")
        k1 = np.ascontiguousarray(kp1, dtype=np.float32).reshape(-1, 2)
        k2 = np.ascontiguousarray(kp2, dtype=np.float32).reshape(-1, 2)
        m = np.ascontiguousarray(matches, dtype=DMATCH)
        K = m.shape[0]
        E = np.zeros(9)
        mask = np.zeros(max(K, 1), dtype=np.uint8)
        out = np.zeros(max(K, 1), dtype=DMATCH)
        n, best = ctypes.c_int(0), ctypes.c_int(-1)
        counts = np.zeros(H, dtype=np.int32) if debug else None
        models = np.zeros((H, 9)) if debug else None
        head = (self.ctx.handle, _vp(k1), k1.shape[0], _vp(k2), k2.shape[0], _vp(m), K, H, ctypes.c_double(float(max_px)),
                ctypes.c_uint64(int(seed) & 0xFFFFFFFFFFFFFFFF))
        tail = (_ptr(E), _ptr(mask, ctypes.c_uint8), _vp(out), ctypes.byref(n), ctypes.byref(best), _vp(counts),
                _vp(models))
        if R == 0:
            self.ctx.check(lib().fm3d_verify_matches(*head, *tail))
        else:
            rc = np.zeros(R + 1, dtype=np.int32) if debug else None
            rm = np.zeros((R, 9)) if debug else None
            adopted = ctypes.c_int(0)
            self.ctx.check(lib().fm3d_verify_matches_refined(*head, ctypes.c_int(R), *tail, _vp(rc), _vp(rm),
                                                             ctypes.byref(adopted)))
        res = (E.reshape(3, 3), mask[:K].astype(bool), out[:n.value].copy(), best.value)
        if debug:
            res += (counts, models.reshape(H, 3, 3))
            if R:
                res += (rc, rm.reshape(R, 3, 3), adopted.value)
        return res

    def plane_to_image2(self, X, n):
        """fm3d_plane_to_image2 (device kernel): extractPixelsContour(X) and the level-0 projection of
        those pixels through the plane (X, n) into image 2 -- (image-1 pixels (m, 2), image-2 uv
        (m, 2), status (m,))."""
        X = np.ascontiguousarray(X, dtype=np.float64)
        n = np.ascontiguousarray(n, dtype=np.float64)
        R = self.ctx.settings.pixelsRay
        cap = (2 * R + 1) ** 2
        xy = np.zeros((cap, 2))
        uv = np.zeros((cap, 2))
        st = np.zeros(cap, dtype=np.int32)
        m = ctypes.c_int(0)
        self.ctx.check(lib().fm3d_plane_to_image2(self.ctx.handle, _ptr(X), _ptr(n), _ptr(xy), _ptr(uv),
                                                  _ptr(st, ctypes.c_int32), cap, ctypes.byref(m)))
        k = m.value
        return xy[:k], uv[:k], st[:k]

    def setKeypoints(self, kpts1: np.ndarray, kpts2: np.ndarray, matches: np.ndarray) -> None:
        """setKeypoints (:145-171): keypoint positions (N, 2) float32 + DMATCH array."""
        self._kp1 = np.ascontiguousarray(kpts1, dtype=np.float32)
        self._kp2 = np.ascontiguousarray(kpts2, dtype=np.float32)
        self._matches = np.ascontiguousarray(matches, dtype=DMATCH)

    def triangulate(self):
        """triangulate (:173-230) -> (points (P, 3) float64, outliersMask (K,) bool)."""
        K = self._matches.shape[0]
        pts = np.zeros((max(K, 1), 3))
        mask = np.zeros(max(K, 1), dtype=np.uint8)
        n = ctypes.c_int(0)
        self.ctx.check(lib().fm3d_triangulate(self.ctx.handle, _vp(self._kp1), self._kp1.shape[0], _vp(self._kp2),
                                              self._kp2.shape[0], _vp(self._matches), K, _ptr(pts),
                                              _ptr(mask, ctypes.c_uint8), ctypes.byref(n)))
        return pts[:n.value].copy(), mask[:K].astype(bool)

    def projectReferencePointsToImageWithFrames(self, referenceNeighborhood, featuresFrames, image_points=False):
        """singlecameratriangulator.cpp:769-849 on image 1 of setImages: (P, size, size) uint8 patches,
        patch[j, i] = sample of reference point (i, j); optionally the (P, size*size, 2) projections.
        The reference neighbourhood must be the square one of the settings (it is rebuilt on the GPU)."""
        F = np.ascontiguousarray(featuresFrames, dtype=np.float64).reshape(-1, 16)
        size = lib().fm3d_patch_size(ctypes.byref(self.ctx.settings))
        if referenceNeighborhood is not None and len(referenceNeighborhood) != size * size:
            raise ValueError(f"reference neighbourhood has {len(referenceNeighborhood)} points, settings give {size}^2")
        n = F.shape[0]
        patches = np.zeros((max(n, 1), size, size), dtype=np.uint8)
        pts = np.zeros((max(n, 1), size * size, 2)) if image_points else None
        self.ctx.check(lib().fm3d_export_patches(self.ctx.handle, _ptr(F), n, _ptr(patches, ctypes.c_uint8),
                                                 _ptr(pts) if pts is not None else None))
        return (patches[:n], pts[:n]) if image_points else patches[:n]


class NeighborhoodsGenerator:
    """NeighborhoodsGenerator (Triangulator/neighborhoodsgenerator.h:78-97): the square method and the
    circular one (Neighborhoods.method; the reference constructor exits with -10 on anything else,
    here ValueError)."""

    def __init__(self, settings: Settings):
        if settings.neighMethod not in (0, 1):
            raise ValueError("Unsupported method for plane neighborhood extraction")  # :69-73 exit(-10)
        self.settings = settings

    def computeCircularNeighborhoodsByNormals(self, ctx: "Context", points, normals=None) -> np.ndarray:
        """neighborhoodsgenerator.cpp:160-224: (P, thetas*rays, 3) samples on concentric circles in the
        tangent plane of every point, ray outer / angle inner; normals None -> the initial guess X/|X|
        (the reference fills its empty normals Mat the same way).  points / normals: (P, 3) (the
        reference's 3 x N Mats, transposed).  Computed on the GPU of ctx."""
        X = np.ascontiguousarray(points, dtype=np.float64).reshape(-1, 3)
        N = None if normals is None or len(normals) == 0 else np.ascontiguousarray(normals, dtype=np.float64).reshape(-1, 3)
        if N is not None and N.shape != X.shape:
            raise ValueError("normals and points differ in shape")
        n, S = X.shape[0], self.settings.neighThetas * self.settings.neighRays
        out = np.zeros((max(n, 1), max(S, 1), 3))
        ctx.check(lib().fm3d_circular_neighborhoods(ctx.handle, _ptr(X), _ptr(N) if N is not None else None, n,
                                                    _ptr(out)))
        return out[:n, :S]

    def computeCircularNeighborhoodByNormal(self, ctx: "Context", point, normal=(0.0, 0.0, 0.0)) -> np.ndarray:
        """neighborhoodsgenerator.cpp:226-277 (one point; a zero normal -> X/|X|): (thetas*rays, 3)."""
        nz = not any(float(v) != 0.0 for v in normal)
        return self.computeCircularNeighborhoodsByNormals(ctx, [point], None if nz else [normal])[0]

    def size(self) -> int:
        return lib().fm3d_patch_size(ctypes.byref(self.settings))

    def computeSquareNeighborhoodsByNormals(self, ctx: "Context", featuresFrames) -> np.ndarray:
        """neighborhoodsgenerator.cpp:76-132 (main.cpp:187): (P, size*size, 3) points of the square
        grid transformed by each feature frame, point order i*size + j; computed on the GPU of ctx."""
        F = np.ascontiguousarray(featuresFrames, dtype=np.float64).reshape(-1, 16)
        n, size = F.shape[0], self.size()
        out = np.zeros((max(n, 1), size * size, 3))
        ctx.check(lib().fm3d_square_neighborhoods(ctx.handle, _ptr(F), n, _ptr(out)))
        return out[:n]

    def getReferenceSquaredNeighborhood(self) -> np.ndarray:
        """neighborhoodsgenerator.cpp:134-158: (size*size, 3) points (-eps + inc*i, -eps + inc*j, 0),
        i outer."""
        eps, inc, n = self.settings.neighEpsilon, self.settings.cmPerPixel * 0.01, self.size()
        out = np.zeros((n * n, 3))
        for i in range(n):
            for j in range(n):
                out[i * n + j, 0] = -eps + inc * i
                out[i * n + j, 1] = -eps + inc * j
        return out


class NormalOptimizer:
    """NormalOptimizer (Triangulator/normaloptimizer.h:43-59), hot-path methods."""

    def __init__(self, ctx: Context, sct: SingleCameraTriangulator | None = None):
        self.ctx = ctx
        self.sct = sct
        self.last_status = self.last_info = self.last_nfev = None
        self.last_stats = None

    def setImages(self, img1: np.ndarray, img2: np.ndarray) -> None:
        a = np.ascontiguousarray(img1, dtype=np.uint8)
        b = np.ascontiguousarray(img2, dtype=np.uint8)
        if a.shape != b.shape or a.ndim != 2:
            raise ValueError("two gray images of the same size expected")
        h, w = a.shape
        self.ctx.check(lib().fm3d_set_images(self.ctx.handle, _ptr(a, ctypes.c_uint8), _ptr(b, ctypes.c_uint8), w, h, w))

    def pyramid(self, which: int, level: int) -> np.ndarray:
        w = ctypes.c_int(0)
        h = ctypes.c_int(0)
        self.ctx.check(lib().fm3d_get_pyramid_level(self.ctx.handle, which, level, None, ctypes.byref(w),
                                                    ctypes.byref(h)))
        out = np.zeros((h.value, w.value), dtype=np.uint8)
        self.ctx.check(lib().fm3d_get_pyramid_level(self.ctx.handle, which, level, _ptr(out, ctypes.c_uint8),
                                                    ctypes.byref(w), ctypes.byref(h)))
        return out

    def getGravity(self) -> np.ndarray:
        """getGravity (normaloptimizer.cpp:185-188): Rodrigues(rodriguesIC)^-1 (0, 0, -1)."""
        g = np.zeros(3)
        _check(lib().fm3d_gravity(ctypes.byref(self.ctx.settings), _ptr(g)))
        return g

    def nccHypotheses(self, points3D: np.ndarray, hphi: int = 4, htheta: int = 4, span: float = 0.4):
        """NCC scoring of hphi x htheta candidate normals per point (fm3d_ncc_hypotheses; BASELINE's
        "patch NCC over 16 / 32 normal hypotheses" -- an extension, the reference has no NCC search):
        (scores (P, H) float64, -2 = invalid; best normals (P, 3); best index (P,), -1 = none).
        Needs setImages and the camera-2 pose of the triangulator."""
        X = np.ascontiguousarray(points3D, dtype=np.float64).reshape(-1, 3)
        n, H = X.shape[0], hphi * htheta
        scores = np.zeros((max(n, 1), H))
        normals = np.zeros((max(n, 1), 3))
        best = np.zeros(max(n, 1), dtype=np.int32)
        self.ctx.check(lib().fm3d_ncc_hypotheses(self.ctx.handle, _ptr(X), n, hphi, htheta, ctypes.c_double(span),
                                                 _ptr(scores), _ptr(normals), _ptr(best, ctypes.c_int32)))
        return scores[:n], normals[:n], best[:n]

    def computeFeaturesFrames(self, points3D: np.ndarray, normals: np.ndarray) -> np.ndarray:
        """computeFeaturesFrames (normaloptimizer.cpp:454-504): (P, 4, 4) frames, on the GPU."""
        P = np.ascontiguousarray(points3D, dtype=np.float64).reshape(-1, 3)
        N = np.ascontiguousarray(normals, dtype=np.float64).reshape(-1, 3)
        n = min(P.shape[0], N.shape[0])  # the reference walks both vectors together
        frames = np.zeros((max(n, 1), 4, 4))
        self.ctx.check(lib().fm3d_features_frames(self.ctx.handle, _ptr(P), _ptr(N), n, _ptr(frames)))
        return frames[:n]

    def startVisualizerThread(self):  # PCL viewer: out of scope, no-op
        pass

    def stopVisualizerThread(self):
        pass

    def computeOptimizedNormals(self, points3D: np.ndarray):
        """computeOptimizedNormals (normaloptimizer.cpp:321-452).

        Returns (kept points, normals): failed points are erased (stable order),
        exactly like the reference mutates its std::vector.  Per-input-point status,
        lmdif info and evaluation counts are left in last_status / last_info / last_nfev.
        """
        P = np.ascontiguousarray(points3D, dtype=np.float64).reshape(-1, 3).copy()
        n = P.shape[0]
        normals = np.zeros((max(n, 1), 3))
        status = np.zeros(max(n, 1), dtype=np.int32)
        info = np.zeros((max(n, 1), 8), dtype=np.int32)
        nfev = np.zeros((max(n, 1), 8), dtype=np.int32)
        kept = ctypes.c_int(0)
        st = LMStats()
        self.ctx.check(lib().fm3d_optimize_normals(self.ctx.handle, _ptr(P), n, _ptr(normals),
                                                   _ptr(status, ctypes.c_int32), _ptr(info, ctypes.c_int32),
                                                   _ptr(nfev, ctypes.c_int32), ctypes.byref(kept), ctypes.byref(st)))
        self.last_status, self.last_info, self.last_nfev = status[:n], info[:n], nfev[:n]
        self.last_stats = st.as_dict()
        k = kept.value
        return P[:k].copy(), normals[:k].copy()


class Pipeline:
    """Whole hot path with inputs resident in HBM (bench / multi-GPU shards)."""

    def __init__(self, ctx: Context):
        self.ctx = ctx
        self.n_queries = 0

    def upload(self, desc_a, desc_b, kp1, kp2, img1, img2, binary=False, query_offset=0):
        """fm3d_pipeline_upload; img1 = img2 = None stages no images (C2's match + DLT)"""
        a = np.ascontiguousarray(desc_a)
        b = np.ascontiguousarray(desc_b)
        k1 = np.ascontiguousarray(kp1, dtype=np.float32)
        k2 = np.ascontiguousarray(kp2, dtype=np.float32)
        if img1 is None and img2 is None:
            i1 = i2 = None
            h = w = 0
        else:
            i1 = np.ascontiguousarray(img1, dtype=np.uint8)
            i2 = np.ascontiguousarray(img2, dtype=np.uint8)
            h, w = i1.shape
        self.n_queries = a.shape[0]
        self.ctx.check(lib().fm3d_pipeline_upload(self.ctx.handle, _vp(a), a.shape[0], _vp(b), b.shape[0],
                                                  a.shape[1], _desc_type(a, binary), _vp(k1), _vp(k2),
                                                  None if i1 is None else _ptr(i1, ctypes.c_uint8),
                                                  None if i2 is None else _ptr(i2, ctypes.c_uint8), w, h,
                                                  query_offset))

    def run(self, records_dev_ptr: int | None = None):
        """One pass; returns (n_kept, stats dict).  records_dev_ptr: device buffer
        (e.g. a torch tensor's data_ptr()) with room for n_queries records."""
        n = ctypes.c_int(0)
        st = PipelineStats()
        self.ctx.check(lib().fm3d_pipeline_run(self.ctx.handle, ctypes.c_void_p(records_dev_ptr or 0),
                                               ctypes.byref(n), ctypes.byref(st)))
        return n.value, st.as_dict()

    def submit(self, desc_a, desc_b, kp1, kp2, img1, img2, binary=False, query_offset=0):
        """fm3d_pipeline_submit: stage one frame pair (H2D through pinned buffers, pyramids) and queue the
        whole path on the context stream without waiting.  The arrays are copied before it returns."""
        a = np.ascontiguousarray(desc_a)
        b = np.ascontiguousarray(desc_b)
        k1 = np.ascontiguousarray(kp1, dtype=np.float32)
        k2 = np.ascontiguousarray(kp2, dtype=np.float32)
        i1 = np.ascontiguousarray(img1, dtype=np.uint8)
        i2 = np.ascontiguousarray(img2, dtype=np.uint8)
        h, w = i1.shape
        self.n_queries = a.shape[0]
        self.ctx.check(lib().fm3d_pipeline_submit(self.ctx.handle, _vp(a), a.shape[0], _vp(b), b.shape[0],
                                                  a.shape[1], _desc_type(a, binary), _vp(k1), _vp(k2),
                                                  _ptr(i1, ctypes.c_uint8), _ptr(i2, ctypes.c_uint8), w, h,
                                                  query_offset))

    def link(self, leader: "Pipeline"):
        """fm3d_pipeline_link(self, leader): this context's pairs join the leader's LM launches."""
        self.ctx.check(lib().fm3d_pipeline_link(self.ctx.handle, leader.ctx.handle))

    def wait(self, out: np.ndarray | None = None):
        """fm3d_pipeline_wait: (survivor records (host), stats dict) of the submitted frame pair.  out: a
        RECORD array with room for n_queries records (reused across calls), or None to allocate."""
        if out is None:
            out = np.zeros(max(self.n_queries, 1), dtype=RECORD)
        n = ctypes.c_int(0)
        st = PipelineStats()
        self.ctx.check(lib().fm3d_pipeline_wait(self.ctx.handle, _vp(out), len(out), ctypes.byref(n),
                                                ctypes.byref(st)))
        return out[:n.value], st.as_dict()

    def run_dlt(self):
        """C2's path: match -> NNDR -> triangulate only; returns (n_inliers, stats dict)"""
        n = ctypes.c_int(0)
        st = PipelineStats()
        self.ctx.check(lib().fm3d_pipeline_run_dlt(self.ctx.handle, ctypes.byref(n), ctypes.byref(st)))
        return n.value, st.as_dict()

    @staticmethod
    def _verify_opts(max_px, hypotheses, seed, refine, pose_from_model, baseline) -> VerifyOpts:
        """verifyMatches' argument checks (and the baseline's), before the library is called"""
        _check_max_px(max_px)
        H = int(hypotheses)
        if H < 1:
            raise Fm3dError(ERR_INVALID, "hypotheses must be >= 1")
        R = int(refine)
        if not 0 <= R <= 16:
            raise Fm3dError(ERR_INVALID, "refine must be in 0 .. 16")
        b = float(baseline)
        if pose_from_model and not (b > 0.0 and b != float("inf")):
            raise Fm3dError(ERR_INVALID, "baseline must be finite and > 0")
        return VerifyOpts(H, R, float(max_px), int(seed) & 0xFFFFFFFFFFFFFFFF, 1 if pose_from_model else 0, 0, b)

    def run_verified(self, max_px, hypotheses: int = 1024, seed: int = 0, refine: int = 0, pose_from_model: bool = False,
                     baseline: float = 1.0, records_dev_ptr: int | None = None):
        """fm3d_pipeline_run_verified (DESIGN.md §3.1d "In the pipeline"): run() with the staged pair's
        matches verified on the device (verifyMatches' max_px, hypotheses, seed, refine) and only the
        verified ones triangulated and optimised.  pose_from_model: the camera-2 pose comes from the
        model (pose_from_epipolar over the verified matches, |t| = baseline) and STAYS installed in the
        context; otherwise the context's pose is kept.  Returns (n_kept, stats dict, report dict):
        matches, verified, best, roundsAdopted, poseInstalled, votes (4,), E (3, 3), g12 (4, 4),
        verify_ms.  No model: zero records, the pose unchanged."""
        o = self._verify_opts(max_px, hypotheses, seed, refine, pose_from_model, baseline)
        n = ctypes.c_int(0)
        st, rep = PipelineStats(), VerifyReport()
        self.ctx.check(lib().fm3d_pipeline_run_verified(self.ctx.handle, ctypes.byref(o),
                                                        ctypes.c_void_p(records_dev_ptr or 0), ctypes.byref(n),
                                                        ctypes.byref(st), ctypes.byref(rep)))
        return n.value, st.as_dict(), rep.as_dict()

    def run_dlt_verified(self, max_px, hypotheses: int = 1024, seed: int = 0, refine: int = 0,
                         pose_from_model: bool = False, baseline: float = 1.0):
        """fm3d_pipeline_run_dlt_verified: run_dlt() on the verified matches, options as run_verified;
        returns (n_inliers, stats dict, report dict).  dlt_results(stats["matches"], n_inliers) then
        gives the verified matches and their points."""
        o = self._verify_opts(max_px, hypotheses, seed, refine, pose_from_model, baseline)
        n = ctypes.c_int(0)
        st, rep = PipelineStats(), VerifyReport()
        self.ctx.check(lib().fm3d_pipeline_run_dlt_verified(self.ctx.handle, ctypes.byref(o), ctypes.byref(n),
                                                            ctypes.byref(st), ctypes.byref(rep)))
        return n.value, st.as_dict(), rep.as_dict()

    def submit_verified(self, desc_a, desc_b, kp1, kp2, img1, img2, max_px, hypotheses: int = 1024, seed: int = 0,
                        refine: int = 0, binary=False) -> None:
        """fm3d_pipeline_submit_verified (DESIGN.md §3.1d "Submit / wait"): submit() with the pair's matches
        verified on the device, in filter mode (the context's pose is kept), queued without waiting: the
        match count never leaves the device.  The arrays are copied before it returns."""
        o = self._verify_opts(max_px, hypotheses, seed, refine, False, 1.0)
        a = np.ascontiguousarray(desc_a)
        b = np.ascontiguousarray(desc_b)
        k1 = np.ascontiguousarray(kp1, dtype=np.float32)
        k2 = np.ascontiguousarray(kp2, dtype=np.float32)
        i1 = np.ascontiguousarray(img1, dtype=np.uint8)
        i2 = np.ascontiguousarray(img2, dtype=np.uint8)
        h, w = i1.shape
        self.n_queries = a.shape[0]
        self.ctx.check(lib().fm3d_pipeline_submit_verified(self.ctx.handle, ctypes.byref(o), _vp(a), a.shape[0], _vp(b),
                                                           b.shape[0], a.shape[1], _desc_type(a, binary), _vp(k1),
                                                           _vp(k2), _vp(i1), _vp(i2), w, h))

    def wait_verified(self, out: np.ndarray | None = None):
        """fm3d_pipeline_wait_verified: (survivor records (host), stats dict, report dict) of the pair
        submit_verified queued, byte for byte run_verified's.  out: as for wait()."""
        if out is None:
            out = np.zeros(max(self.n_queries, 1), dtype=RECORD)
        n = ctypes.c_int(0)
        st, rep = PipelineStats(), VerifyReport()
        self.ctx.check(lib().fm3d_pipeline_wait_verified(self.ctx.handle, _vp(out), len(out), ctypes.byref(n),
                                                         ctypes.byref(st), ctypes.byref(rep)))
        return out[:n.value], st.as_dict(), rep.as_dict()

    def submit_dlt_verified(self, max_px, hypotheses: int = 1024, seed: int = 0, refine: int = 0) -> None:
        """fm3d_pipeline_submit_dlt_verified: run_dlt_verified's front half on the staged pair, filter
        mode, queued on the context stream (returns at once)"""
        o = self._verify_opts(max_px, hypotheses, seed, refine, False, 1.0)
        self.ctx.check(lib().fm3d_pipeline_submit_dlt_verified(self.ctx.handle, ctypes.byref(o)))

    def wait_dlt_verified(self):
        """fm3d_pipeline_wait_dlt_verified: (n_inliers, stats dict, report dict) of the submitted
        verified front half; dlt_results(stats["matches"], n_inliers) gives its matches and points"""
        n = ctypes.c_int(0)
        st, rep = PipelineStats(), VerifyReport()
        self.ctx.check(lib().fm3d_pipeline_wait_dlt_verified(self.ctx.handle, ctypes.byref(n), ctypes.byref(st),
                                                             ctypes.byref(rep)))
        return n.value, st.as_dict(), rep.as_dict()

    def submit_dlt(self) -> None:
        """fm3d_pipeline_submit_dlt: C2's path queued on the context stream (returns at once)"""
        self.ctx.check(lib().fm3d_pipeline_submit_dlt(self.ctx.handle))

    def submit_dlt_pair(self, desc_a, desc_b, kp1, kp2, binary=False, query_offset=0) -> None:
        """fm3d_pipeline_submit_dlt_pair: stage a pair from host memory (no images) and queue C2's path,
        with no host wait (float rows are checked on the device; wait_dlt redoes non-integer ones)"""
        a = np.ascontiguousarray(desc_a)
        b = np.ascontiguousarray(desc_b)
        k1 = np.ascontiguousarray(kp1, dtype=np.float32)
        k2 = np.ascontiguousarray(kp2, dtype=np.float32)
        self.n_queries = a.shape[0]
        self.ctx.check(lib().fm3d_pipeline_submit_dlt_pair(self.ctx.handle, _vp(a), a.shape[0], _vp(b), b.shape[0],
                                                           a.shape[1], _desc_type(a, binary), _vp(k1), _vp(k2),
                                                           query_offset))

    def wait_dlt(self):
        """fm3d_pipeline_wait_dlt: (n_inliers, stats dict) of the submitted front half"""
        n = ctypes.c_int(0)
        st = PipelineStats()
        self.ctx.check(lib().fm3d_pipeline_wait_dlt(self.ctx.handle, ctypes.byref(n), ctypes.byref(st)))
        return n.value, st.as_dict()

    def run_ncc(self, hphi: int = 4, htheta: int = 4, span: float = 0.4):
        """C3's path: match -> NNDR -> triangulate -> NCC scoring of hphi x htheta normals per inlier;
        returns (n_points, stats dict)"""
        n = ctypes.c_int(0)
        st = PipelineStats()
        self.ctx.check(lib().fm3d_pipeline_run_ncc(self.ctx.handle, hphi, htheta, ctypes.c_double(span), ctypes.byref(n),
                                                   ctypes.byref(st)))
        return n.value, st.as_dict()

    def submit_ncc(self, hphi: int = 4, htheta: int = 4, span: float = 0.4) -> None:
        """fm3d_pipeline_submit_ncc: C3's path queued on the context stream (returns at once)"""
        self.ctx.check(lib().fm3d_pipeline_submit_ncc(self.ctx.handle, hphi, htheta, ctypes.c_double(span)))

    def wait_ncc(self):
        """fm3d_pipeline_wait_ncc: (n_points, stats dict) of the submitted C3 path"""
        n = ctypes.c_int(0)
        st = PipelineStats()
        self.ctx.check(lib().fm3d_pipeline_wait_ncc(self.ctx.handle, ctypes.byref(n), ctypes.byref(st)))
        return n.value, st.as_dict()

    def ncc_results(self, n_points: int, H: int):
        """(scores (P, H), best normals (P, 3), best index (P,)) of the last run_ncc"""
        sc = np.zeros((max(n_points, 1), H))
        nr = np.zeros((max(n_points, 1), 3))
        b = np.zeros(max(n_points, 1), dtype=np.int32)
        self.ctx.check(lib().fm3d_pipeline_ncc_download(self.ctx.handle, _vp(sc), _vp(nr), _ptr(b, ctypes.c_int32)))
        return sc[:n_points], nr[:n_points], b[:n_points]

    def dlt_results(self, n_matches: int, n_inliers: int):
        """(matches (K,) DMATCH, inlier points (P, 3), match index of each point) of the last run"""
        m = np.zeros(max(n_matches, 1), dtype=DMATCH)
        pts = np.zeros((max(n_inliers, 1), 3))
        src = np.zeros(max(n_inliers, 1), dtype=np.int32)
        self.ctx.check(lib().fm3d_pipeline_dlt_download(self.ctx.handle, _vp(m), _vp(pts), _ptr(src, ctypes.c_int32)))
        return m[:n_matches], pts[:n_inliers], src[:n_inliers]

    def records(self, n: int, records_dev_ptr: int | None = None) -> np.ndarray:
        out = np.zeros(max(n, 1), dtype=RECORD)
        self.ctx.check(lib().fm3d_records_download(self.ctx.handle, ctypes.c_void_p(records_dev_ptr or 0), n,
                                                   _vp(out)))
        return out[:n]

    def describe(self, n: int, source="records", records_dev_ptr: int | None = None, frames: bool = False,
                 patches: bool = False):
        """fm3d_pipeline_describe: the tail (main.cpp:157-183) on the device for the n records of the last
        run (or of the caller's device buffer), or with source="ncc" for the last run_ncc's points and
        best normals.  Returns (descriptor rows (n, cols), frames (n, 4, 4) | None, patches
        (n, size, size) | None, stats dict); only patches=True moves a patch to the host."""
        return self._describe(lib().fm3d_pipeline_describe, n, source, records_dev_ptr, frames, patches)

    def _describe(self, call, n, source, records_dev_ptr, frames, patches):
        src = DESCRIBE_SOURCES.get(source, source)
        if not isinstance(src, int):
            raise ValueError(f"source must be one of {sorted(DESCRIBE_SOURCES)}")
        cols, typ = ctypes.c_int(0), ctypes.c_int(0)
        rc = lib().fm3d_descriptor_info(self.ctx.handle, ctypes.byref(cols), ctypes.byref(typ))
        dt = np.uint8 if rc == FM3D_OK and typ.value == DESC_BITS else np.float32
        size = max(lib().fm3d_patch_size(ctypes.byref(self.ctx.settings)), 0)
        m = max(n, 1)
        desc = np.zeros((m, max(cols.value, 1)), dtype=dt)
        fr = np.zeros((m, 4, 4)) if frames else None
        pa = np.zeros((m, size, size), dtype=np.uint8) if patches else None
        st = DescribeStats()
        self.ctx.check(call(self.ctx.handle, src, ctypes.c_void_p(records_dev_ptr or 0), n, _vp(desc), _vp(fr), _vp(pa),
                            ctypes.byref(st)))
        n = max(n, 0)
        return (desc[:n], fr[:n] if frames else None, pa[:n] if patches else None, st.as_dict())

    def describe_any(self, n: int, source="records", records_dev_ptr: int | None = None, frames: bool = False,
                     patches: bool = False):
        """fm3d_pipeline_describe_any: describe() for every extractor of the settings -- ORB rows (n, 32)
        uint8 from one launch per chunk, BRISK / FREAK (n, 64) zero rows while their border filter drops
        the centred keypoint (every patch edge below 634 / 680; from there on ERR_UNSUPPORTED), SURF and
        SIFT as describe().  The same return shape."""
        return self._describe(lib().fm3d_pipeline_describe_any, n, source, records_dev_ptr, frames, patches)


SHARE_BLOCK = 4096  # queries per block of the block-cyclic partition (fm3d_mgpu, shard.py)


def math_probe(ctx: "Context", fn_name: str, x, y=None) -> np.ndarray:
    """fm3d_math_probe: function fn_name (PROBE_FNS) of the shared math headers on the device,
    elementwise over x (and y for PROBE_BINARY; the first array is the first argument).  Float
    functions take and return floats widened exactly to double."""
    if fn_name not in PROBE_FNS:
        raise Fm3dError(ERR_INVALID, f"unknown probe function {fn_name!r}")
    x = np.ascontiguousarray(x, dtype=np.float64).ravel()
    if fn_name in PROBE_BINARY:
        if y is None:
            raise Fm3dError(ERR_INVALID, f"{fn_name} takes two arguments")
        y = np.ascontiguousarray(y, dtype=np.float64).ravel()
        if y.size != x.size:
            raise Fm3dError(ERR_INVALID, "x and y differ in length")
    else:
        y = None
    out = np.empty_like(x)
    ctx.check(lib().fm3d_math_probe(ctx.handle, ctypes.c_int(PROBE_FNS.index(fn_name)), _ptr(x),
                                    _ptr(y) if y is not None else None, ctypes.c_int(x.size), _ptr(out)))
    return out


def device_count() -> int:
    """fm3d_device_count: the GPUs HIP sees (hipGetDeviceCount), without importing torch."""
    n = ctypes.c_int(0)
    _check(lib().fm3d_device_count(ctypes.byref(n)))
    return n.value


def share_queries(n: int, shares: int, s: int, block: int = SHARE_BLOCK) -> np.ndarray:
    """fm3d_share_queries: global query indices of share s (blocks dealt round-robin)."""
    cnt = ctypes.c_int(0)
    _check(lib().fm3d_share_queries(n, shares, s, block, None, 0, ctypes.byref(cnt)))
    idx = np.zeros(max(cnt.value, 1), dtype=np.int32)
    _check(lib().fm3d_share_queries(n, shares, s, block, _ptr(idx, ctypes.c_int32), len(idx), ctypes.byref(cnt)))
    return idx[:cnt.value].astype(np.int64)


def merge_shares(parts, n: int, block: int = SHARE_BLOCK) -> np.ndarray:
    """fm3d_merge_shares (the C++ merge of fm3d_mgpu_pipeline_run, host only): parts[s] = share s's
    survivor records with local query indices -> all records with global indices, query order."""
    parts = [np.ascontiguousarray(p, dtype=RECORD) for p in parts]
    shares = len(parts)
    ptrs = (ctypes.c_void_p * max(shares, 1))(*[p.ctypes.data for p in parts])
    counts = np.array([len(p) for p in parts], dtype=np.int32)
    out = np.zeros(max(int(counts.sum()), 1), dtype=RECORD)
    k = ctypes.c_int(0)
    _check(lib().fm3d_merge_shares(n, shares, block, ptrs, _ptr(counts, ctypes.c_int32), _vp(out), ctypes.byref(k)))
    return out[:k.value]


class MultiGPU:
    """fm3d_mgpu: the whole path over several GPUs in one process -- query
    blocks dealt round-robin over `shares` logical shares (share s on devices[s % ndev]), frame B
    and the images replicated, RCCL all-gather of the survivor records, merged in query order."""

    def __init__(self, settings: Settings, devices=(0,), shares: int | None = None, block: int = SHARE_BLOCK):
        self.settings = settings
        devs = np.ascontiguousarray(devices, dtype=np.int32)
        self.ndev = len(devs)
        self.shares = shares or self.ndev
        self._h = ctypes.c_void_p()
        rc = lib().fm3d_mgpu_create(ctypes.byref(settings), self.ndev, _ptr(devs, ctypes.c_int32), self.shares, block,
                                    ctypes.byref(self._h))
        if rc != FM3D_OK:
            why = (lib().fm3d_mgpu_last_error(None) or b"").decode(errors="replace")
            raise Fm3dError(rc, "fm3d_mgpu_create failed" + (f": {why}" if why else " (no HIP devices / RCCL?)"))
        self.n_queries = 0

    def check(self, rc):
        if rc != FM3D_OK:
            raise Fm3dError(rc, lib().fm3d_mgpu_last_error(self._h).decode(errors="replace"))

    def set_g12(self, g12):
        self.check(lib().fm3d_mgpu_set_g12(self._h, _ptr(np.ascontiguousarray(g12, dtype=np.float64).ravel())))

    def upload(self, desc_a, desc_b, kp1, kp2, img1, img2, binary=False):
        a = np.ascontiguousarray(desc_a)
        b = np.ascontiguousarray(desc_b)
        k1 = np.ascontiguousarray(kp1, dtype=np.float32)
        k2 = np.ascontiguousarray(kp2, dtype=np.float32)
        i1 = np.ascontiguousarray(img1, dtype=np.uint8)
        i2 = np.ascontiguousarray(img2, dtype=np.uint8)
        h, w = i1.shape
        self.n_queries = a.shape[0]
        self.check(lib().fm3d_mgpu_pipeline_upload(self._h, _vp(a), a.shape[0], _vp(b), b.shape[0], a.shape[1],
                                                   _desc_type(a, binary), _vp(k1), _vp(k2), _ptr(i1, ctypes.c_uint8),
                                                   _ptr(i2, ctypes.c_uint8), w, h))

    def submit(self, desc_a, desc_b, kp1, kp2, img1, img2, binary=False):
        """fm3d_mgpu_submit: one frame pair staged on every device and queued (two may be in flight)."""
        a = np.ascontiguousarray(desc_a)
        b = np.ascontiguousarray(desc_b)
        k1 = np.ascontiguousarray(kp1, dtype=np.float32)
        k2 = np.ascontiguousarray(kp2, dtype=np.float32)
        i1 = np.ascontiguousarray(img1, dtype=np.uint8)
        i2 = np.ascontiguousarray(img2, dtype=np.uint8)
        h, w = i1.shape
        self.n_queries = a.shape[0]
        self.check(lib().fm3d_mgpu_submit(self._h, _vp(a), a.shape[0], _vp(b), b.shape[0], a.shape[1],
                                          _desc_type(a, binary), _vp(k1), _vp(k2), _ptr(i1, ctypes.c_uint8),
                                          _ptr(i2, ctypes.c_uint8), w, h))

    def wait(self, out: np.ndarray | None = None):
        """fm3d_mgpu_wait: (merged records of the oldest submitted pair, stats dict)."""
        if out is None:
            out = np.zeros(max(self.n_queries, 1), dtype=RECORD)
        n = ctypes.c_int(0)
        st = PipelineStats()
        self.check(lib().fm3d_mgpu_wait(self._h, _vp(out), len(out), ctypes.byref(n), ctypes.byref(st)))
        return out[:n.value], st.as_dict()

    def run(self):
        """One pass over all devices: (records in query order, stats dict)."""
        out = np.zeros(max(self.n_queries, 1), dtype=RECORD)
        n = ctypes.c_int(0)
        st = PipelineStats()
        self.check(lib().fm3d_mgpu_pipeline_run(self._h, _vp(out), ctypes.byref(n), ctypes.byref(st)))
        return out[:n.value], st.as_dict()

    def close(self):
        if self._h:
            lib().fm3d_mgpu_destroy(self._h)
            self._h = ctypes.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def g12_from_poses(settings: Settings, T1, T2, r1, r2) -> np.ndarray:
    """Context-free setg12 algebra (host only)."""
    g = np.zeros(16)
    f64 = lambda v: np.ascontiguousarray(v, dtype=np.float64)
    _check(lib().fm3d_g12_from_poses(ctypes.byref(settings), _ptr(f64(T1)), _ptr(f64(T2)), _ptr(f64(r1)),
                                     _ptr(f64(r2)), _ptr(g)))
    return g.reshape(4, 4)


def camera2_from_g12(g12):
    R2 = np.zeros(9)
    t2 = np.zeros(3)
    _check(lib().fm3d_camera2_from_g12(_ptr(np.ascontiguousarray(g12, dtype=np.float64).ravel()), _ptr(R2), _ptr(t2)))
    return R2.reshape(3, 3), t2


def epipolar_matrix(g12) -> np.ndarray:
    """E = [t2]x R2 of the guided matcher's gate, from camera2_from_g12's (R2, t2) (host only)."""
    E = np.zeros(9)
    _check(lib().fm3d_epipolar_matrix(_ptr(np.ascontiguousarray(g12, dtype=np.float64).ravel()), _ptr(E)))
    return E.reshape(3, 3)


def ransac_sample(seed: int, h: int, M: int):
    """fm3d_ransac_sample: the eight distinct match indices of hypothesis h among M matches (host only)
    -> (idx (8,) int32, valid)."""
    idx = np.zeros(8, dtype=np.int32)
    rc = lib().fm3d_ransac_sample(ctypes.c_uint64(int(seed) & 0xFFFFFFFFFFFFFFFF), ctypes.c_int(h), ctypes.c_int(M),
                                  _ptr(idx, ctypes.c_int32))
    if rc < 0:
        _check(rc)
    return idx, rc == 0


def _pairs(x, n=None):
    a = np.ascontiguousarray(x, dtype=np.float64).reshape(-1, 2)
    if n is not None and a.shape[0] != n:
        raise ValueError(f"expected {n} points, got {a.shape[0]}")
    return a


def epipolar_from8(x1, x2, null_vector: bool = False):
    """fm3d_epipolar_from8: the essential matrix (x2^T E x1 = 0) of eight pairs of normalised
    coordinates (host only) -> (E (3, 3), valid); an invalid model is zero.  null_vector: the unit null
    vector of the 8 x 9 system before the projection (fm3d_epipolar_null8)."""
    a, b = _pairs(x1, 8), _pairs(x2, 8)
    E = np.zeros(9)
    f = lib().fm3d_epipolar_null8 if null_vector else lib().fm3d_epipolar_from8
    rc = f(_ptr(a), _ptr(b), _ptr(E))
    if rc < 0:
        _check(rc)
    return E.reshape(3, 3), rc == 0


def epipolar_count(E, x1, x2, tau: float):
    """fm3d_epipolar_count: the pairs within tau (normalised units) of the model by the Sampson test
    (host only) -> (count, mask (n,) bool)."""
    a, b = _pairs(x1), _pairs(x2)
    if a.shape != b.shape:
        raise ValueError("x1 and x2 differ in length")
    mask = np.zeros(max(a.shape[0], 1), dtype=np.uint8)
    rc = lib().fm3d_epipolar_count(_ptr(np.ascontiguousarray(E, dtype=np.float64).ravel()), _ptr(a), _ptr(b),
                                   a.shape[0], ctypes.c_double(float(tau)), _ptr(mask, ctypes.c_uint8))
    if rc < 0:
        _check(rc)
    return rc, mask[:a.shape[0]].astype(bool)


def epipolar_normal45(E, x1, x2, tau: float):
    """fm3d_epipolar_normal45: the 45 entries (r <= c, row by row) of the sum of a a^T over the pairs the
    model accepts at tau, in the refit's summation order (host only) -> (N45 (45,), pairs in)."""
    a, b = _pairs(x1), _pairs(x2)
    if a.shape != b.shape:
        raise ValueError("x1 and x2 differ in length")
    N = np.zeros(45)
    rc = lib().fm3d_epipolar_normal45(_ptr(np.ascontiguousarray(E, dtype=np.float64).ravel()), _ptr(a), _ptr(b),
                                      a.shape[0], ctypes.c_double(float(tau)), _ptr(N))
    if rc < 0:
        _check(rc)
    return N, rc


def epipolar_refit(E, x1, x2, tau: float):
    """fm3d_epipolar_refit: the least-squares essential matrix of the pairs the model E accepts at tau
    (host only) -> (E' (3, 3), valid); an invalid refit is zero."""
    a, b = _pairs(x1), _pairs(x2)
    if a.shape != b.shape:
        raise ValueError("x1 and x2 differ in length")
    out = np.zeros(9)
    rc = lib().fm3d_epipolar_refit(_ptr(np.ascontiguousarray(E, dtype=np.float64).ravel()), _ptr(a), _ptr(b),
                                   a.shape[0], ctypes.c_double(float(tau)), _ptr(out))
    if rc < 0:
        _check(rc)
    return out.reshape(3, 3), rc == 0


def pose_from_epipolar(E, x1, x2, baseline: float = 1.0):
    """fm3d_pose_from_epipolar: the decomposition of E that puts most pairs in front of both cameras
    (host only) -> (g12 (4, 4) = [R | baseline t], votes (4,) int32, valid)."""
    a, b = _pairs(x1), _pairs(x2)
    if a.shape != b.shape:
        raise ValueError("x1 and x2 differ in length")
    g = np.zeros(16)
    votes = np.zeros(4, dtype=np.int32)
    rc = lib().fm3d_pose_from_epipolar(_ptr(np.ascontiguousarray(E, dtype=np.float64).ravel()), _ptr(a), _ptr(b),
                                       a.shape[0], ctypes.c_double(float(baseline)), _ptr(g),
                                       _ptr(votes, ctypes.c_int32))
    if rc < 0:
        _check(rc)
    return g.reshape(4, 4), votes, rc == 0


def _xyz(x, n=None):
    a = np.ascontiguousarray(x, dtype=np.float64).reshape(-1, 3)
    if n is not None and a.shape[0] != n:
        raise ValueError(f"expected {n} points, got {a.shape[0]}")
    return a


def _normal_pair(na, nb, a, b):
    """both normal arrays, shaped like their points, or neither (fm3d_rigid_count's rule)"""
    if (na is None) != (nb is None):
        raise Fm3dError(ERR_INVALID, "normals: both arrays or neither")
    if na is None:
        return None, None
    return _xyz(na, a.shape[0]), _xyz(nb, b.shape[0])


def ransac_sample3(seed: int, h: int, M: int):
    """fm3d_ransac_sample3: the three distinct match indices of hypothesis h among M matches (host only)
    -> (idx (3,) int32, valid)."""
    idx = np.zeros(3, dtype=np.int32)
    rc = lib().fm3d_ransac_sample3(ctypes.c_uint64(int(seed) & 0xFFFFFFFFFFFFFFFF), ctypes.c_int(h), ctypes.c_int(M),
                                   _ptr(idx, ctypes.c_int32))
    if rc < 0:
        _check(rc)
    return idx, rc == 0


def rigid_from3(a, b):
    """fm3d_rigid_from3: the rigid transform b = R a + t of three pairs of 3D points (host only)
    -> (model (12,): R row-major, then t; valid); an invalid model is zero."""
    pa, pb = _xyz(a, 3), _xyz(b, 3)
    m = np.zeros(12)
    rc = lib().fm3d_rigid_from3(_ptr(pa), _ptr(pb), _ptr(m))
    if rc < 0:
        _check(rc)
    return m, rc == 0


def rigid_count(model, a, b, max_dist: float, normals_a=None, normals_b=None, min_normal_cos: float = 0.0):
    """fm3d_rigid_count: the pairs within max_dist of the model and, with normals, facing within
    min_normal_cos (host only) -> (count, mask (n,) bool)."""
    pa, pb = _xyz(a), _xyz(b)
    if pa.shape != pb.shape:
        raise ValueError("a and b differ in length")
    na, nb = _normal_pair(normals_a, normals_b, pa, pb)
    mask = np.zeros(max(pa.shape[0], 1), dtype=np.uint8)
    rc = lib().fm3d_rigid_count(_ptr(np.ascontiguousarray(model, dtype=np.float64).ravel()), _ptr(pa), _ptr(pb), _vp(na),
                                _vp(nb), pa.shape[0], ctypes.c_double(float(max_dist)),
                                ctypes.c_double(float(min_normal_cos)), _ptr(mask, ctypes.c_uint8))
    if rc < 0:
        _check(rc)
    return rc, mask[:pa.shape[0]].astype(bool)


def rigid_refit(model, a, b, max_dist: float, normals_a=None, normals_b=None, min_normal_cos: float = 0.0,
                sums: bool = False):
    """fm3d_rigid_refit: the least-squares rigid transform of the pairs the model accepts (host only)
    -> (model' (12,), valid); an invalid refit is zero.  sums: also the 7 + 9 sums of its two passes."""
    pa, pb = _xyz(a), _xyz(b)
    if pa.shape != pb.shape:
        raise ValueError("a and b differ in length")
    na, nb = _normal_pair(normals_a, normals_b, pa, pb)
    out, S = np.zeros(12), np.zeros(16)
    rc = lib().fm3d_rigid_refit(_ptr(np.ascontiguousarray(model, dtype=np.float64).ravel()), _ptr(pa), _ptr(pb), _vp(na),
                                _vp(nb), pa.shape[0], ctypes.c_double(float(max_dist)),
                                ctypes.c_double(float(min_normal_cos)), _ptr(out), _ptr(S))
    if rc < 0:
        _check(rc)
    return (out, rc == 0, S) if sums else (out, rc == 0)


class ModelAligner:
    """3D-3D alignment of two feature models: a RANSAC fit of a rigid transform
    b = R a + t to matched points (fm3d_record points, or any (n, 3) doubles), optionally tested on the
    surface normals too, with a refit of the best model on the pairs it accepts."""

    def __init__(self, ctx: Context):
        self.ctx = ctx

    @staticmethod
    def _opts(max_dist, min_normal_cos, hypotheses, seed, refine) -> AlignOpts:
        """fm3d_align_opts' rules, before the library is called"""
        d, mc, H, R = float(max_dist), float(min_normal_cos), int(hypotheses), int(refine)
        if not (d > 0.0 and d != float("inf")):
            raise Fm3dError(ERR_INVALID, "maxDist must be finite and > 0")
        if not -1.0 <= mc <= 1.0:
            raise Fm3dError(ERR_INVALID, "minNormalCos must be in -1 .. 1")
        if H < 1:
            raise Fm3dError(ERR_INVALID, "hypotheses must be >= 1")
        if not 0 <= R <= 16:
            raise Fm3dError(ERR_INVALID, "refine must be in 0 .. 16")
        return AlignOpts(H, R, d, mc, int(seed) & 0xFFFFFFFFFFFFFFFF)

    @staticmethod
    def _outputs(K, o, debug):
        H, R = o.hypotheses, o.refineIters
        return dict(g=np.zeros(16), mask=np.zeros(max(K, 1), dtype=np.uint8), out=np.zeros(max(K, 1), dtype=DMATCH),
                    n=ctypes.c_int(0), best=ctypes.c_int(-1), counts=np.zeros(H, dtype=np.int32) if debug else None,
                    models=np.zeros((H, 12)) if debug else None,
                    rc=np.zeros(R + 1, dtype=np.int32) if debug and R else None,
                    rm=np.zeros((max(R, 1), 12)) if debug and R else None, adopted=ctypes.c_int(0))

    @staticmethod
    def _tail(b):
        return (_ptr(b["g"]), _ptr(b["mask"], ctypes.c_uint8), _vp(b["out"]), ctypes.byref(b["n"]), ctypes.byref(b["best"]),
                _vp(b["counts"]), _vp(b["models"]), _vp(b["rc"]), _vp(b["rm"]), ctypes.byref(b["adopted"]))

    @staticmethod
    def _result(b, K, o, debug):
        res = (b["g"].reshape(4, 4), b["mask"][:K].astype(bool), b["out"][:b["n"].value].copy(), b["best"].value)
        if debug:
            res += (b["counts"], b["models"])
            if o.refineIters:
                res += (b["rc"], b["rm"], b["adopted"].value)
        return res

    def align(self, pts_a, pts_b, matches, max_dist, normals_a=None, normals_b=None, min_normal_cos: float = 0.0,
              hypotheses: int = 1024, seed: int = 0, refine: int = 0, debug: bool = False):
        """fm3d_align_points: `hypotheses` three-point models scored against every match within max_dist
        (the points' unit) and, with normals, (R n_a) . n_b >= min_normal_cos -> (g (4, 4) = [R | t],
        mask (K,) bool, inliers (DMATCH, input order), best); with debug also counts (H,) int32 (-1 for
        an invalid hypothesis) and models (H, 12: R row-major, then t).  No valid model: a zero g, no
        inliers, best -1.  refine (0 .. 16): that many rounds of a least-squares refit on the pairs the
        model accepts, each adopted iff valid and no worse in count; with refine > 0 and debug three
        more: roundCounts (refine + 1,) int32 (c_0, then each round's count: -1 an invalid refit, -2 a
        round not run), roundModels (refine, 12) and the number of rounds adopted."""
        o = self._opts(max_dist, min_normal_cos, hypotheses, seed, refine)
        a, b = _xyz(pts_a), _xyz(pts_b)
        na, nb = _normal_pair(normals_a, normals_b, a, b)
        m = np.ascontiguousarray(matches, dtype=DMATCH)
        K = m.shape[0]
        buf = self._outputs(K, o, debug)
        self.ctx.check(lib().fm3d_align_points(self.ctx.handle, _vp(a), _vp(na), a.shape[0], _vp(b), _vp(nb), b.shape[0],
                                               _vp(m), K, ctypes.byref(o), *self._tail(buf)))
        return self._result(buf, K, o, debug)

    def match_and_align(self, desc_a, desc_b, pts_a, pts_b, epsilon, max_dist, normals_a=None, normals_b=None,
                        min_normal_cos: float = 0.0, hypotheses: int = 1024, seed: int = 0, refine: int = 0,
                        debug: bool = False, binary: bool = False):
        """fm3d_match_models: the context's matcher (NNDR at epsilon; the settings' crossCheck is
        honoured) on one descriptor row per point, then align() on its matches without a trip through
        the host -> (matches (DMATCH),) + align()'s result."""
        o = self._opts(max_dist, min_normal_cos, hypotheses, seed, refine)
        da, db = np.ascontiguousarray(desc_a), np.ascontiguousarray(desc_b)
        a, b = _xyz(pts_a, da.shape[0]), _xyz(pts_b, db.shape[0])
        na, nb = _normal_pair(normals_a, normals_b, a, b)
        nA = da.shape[0]
        matches = np.zeros(max(nA, 1), dtype=DMATCH)
        nm = ctypes.c_int(0)
        buf = self._outputs(nA, o, debug)
        self.ctx.check(lib().fm3d_match_models(self.ctx.handle, _vp(da), _vp(a), _vp(na), nA, _vp(db), _vp(b), _vp(nb),
                                               db.shape[0], da.shape[1], _desc_type(da, binary),
                                               ctypes.c_double(float(epsilon)), ctypes.byref(o), _vp(matches),
                                               ctypes.byref(nm), *self._tail(buf)))
        K = nm.value
        return (matches[:K].copy(),) + self._result(buf, K, o, debug)


def quartic_roots(coef):
    """fm3d_quartic_roots: the real roots of coef[4] x^4 + .. + coef[0] (host only) -> (roots (4,): NaN
    where a position holds none, their number, valid)."""
    c = np.ascontiguousarray(coef, dtype=np.float64).ravel()
    if c.shape[0] != 5:
        raise ValueError("expected five coefficients")
    roots, n = np.zeros(4), ctypes.c_int(0)
    rc = lib().fm3d_quartic_roots(_ptr(c), _ptr(roots), ctypes.byref(n))
    if rc < 0:
        _check(rc)
    return roots, n.value, rc == 0


def p3p(X, uv):
    """fm3d_p3p: the up to four poses Xc = R X + t of three model points X (3, 3) seen at the normalised
    image points uv (3, 2) (host only) -> (models (4, 12): R row-major, then t, zero when invalid;
    valid (4,) bool)."""
    px = _xyz(X, 3)
    pu = np.ascontiguousarray(uv, dtype=np.float64).reshape(3, 2)
    m, ok = np.zeros((4, 12)), np.zeros(4, dtype=np.int32)
    rc = lib().fm3d_p3p(_ptr(px), _ptr(pu), _ptr(m), _ptr(ok, ctypes.c_int32))
    if rc < 0:
        _check(rc)
    return m, ok.astype(bool)


def _uv_xyz(uv, X, normals):
    pu = np.ascontiguousarray(uv, dtype=np.float64).reshape(-1, 2)
    px = _xyz(X, pu.shape[0])
    return pu, px, None if normals is None else _xyz(normals, pu.shape[0])


def pnp_count(model, uv, X, tau: float, normals=None, min_facing_cos: float = 0.0):
    """fm3d_pnp_count: the matches whose point reprojects within tau (normalised units) of its image
    point in front of the camera and, with normals, faces it within min_facing_cos (host only)
    -> (count, mask (n,) bool)."""
    pu, px, pn = _uv_xyz(uv, X, normals)
    mask = np.zeros(max(pu.shape[0], 1), dtype=np.uint8)
    rc = lib().fm3d_pnp_count(_ptr(np.ascontiguousarray(model, dtype=np.float64).ravel()), _ptr(pu), _ptr(px), _vp(pn),
                              pu.shape[0], ctypes.c_double(float(tau)), ctypes.c_double(float(min_facing_cos)),
                              _ptr(mask, ctypes.c_uint8))
    if rc < 0:
        _check(rc)
    return rc, mask[:pu.shape[0]].astype(bool)


def pnp_step(model, uv, X, tau: float, normals=None, min_facing_cos: float = 0.0, sums: bool = False):
    """fm3d_pnp_step: one Gauss-Newton step of the reprojection error on the matches the model accepts
    (host only) -> (model' (12,), valid); an invalid step is zero.  sums: also its 28 sums."""
    pu, px, pn = _uv_xyz(uv, X, normals)
    out, S = np.zeros(12), np.zeros(28)
    rc = lib().fm3d_pnp_step(_ptr(np.ascontiguousarray(model, dtype=np.float64).ravel()), _ptr(pu), _ptr(px), _vp(pn),
                             pu.shape[0], ctypes.c_double(float(tau)), ctypes.c_double(float(min_facing_cos)), _ptr(out),
                             _ptr(S))
    if rc < 0:
        _check(rc)
    return (out, rc == 0, S) if sums else (out, rc == 0)


class ModelLocalizer:
    """2D-3D localisation of an image against a feature model: a RANSAC fit of the
    camera pose Xc = R X + t to matches between the model's points (fm3d_record points, or any (n, 3)
    doubles) and the image's keypoints, optionally tested on the model's normals too, with a
    Gauss-Newton refit of the best pose on the matches it accepts.  Uses the camera of the context's
    settings."""

    def __init__(self, ctx: Context):
        self.ctx = ctx

    @staticmethod
    def _opts(max_px, min_facing_cos, samples, seed, refine) -> LocalizeOpts:
        """fm3d_localize_opts' rules, before the library is called"""
        _check_max_px(max_px)
        mc, S, R = float(min_facing_cos), int(samples), int(refine)
        if not 0.0 <= mc <= 1.0:
            raise Fm3dError(ERR_INVALID, "minFacingCos must be in 0 .. 1")
        if S < 1:
            raise Fm3dError(ERR_INVALID, "samples must be >= 1")
        if not 0 <= R <= 16:
            raise Fm3dError(ERR_INVALID, "refine must be in 0 .. 16")
        return LocalizeOpts(S, R, float(max_px), mc, int(seed) & 0xFFFFFFFFFFFFFFFF)

    @staticmethod
    def _outputs(K, o, debug):
        H, R = 4 * o.samples, o.refineIters
        return dict(g=np.zeros(16), mask=np.zeros(max(K, 1), dtype=np.uint8), out=np.zeros(max(K, 1), dtype=DMATCH),
                    n=ctypes.c_int(0), best=ctypes.c_int(-1), counts=np.zeros(H, dtype=np.int32) if debug else None,
                    models=np.zeros((H, 12)) if debug else None,
                    rc=np.zeros(R + 1, dtype=np.int32) if debug and R else None,
                    rm=np.zeros((max(R, 1), 12)) if debug and R else None, adopted=ctypes.c_int(0))

    def localize(self, pts, kpts, matches, max_px, normals=None, min_facing_cos: float = 0.0, samples: int = 256,
                 seed: int = 0, refine: int = 0, debug: bool = False):
        """fm3d_localize_points: `samples` three-match samples of up to four P3P poses each, scored against
        every match within max_px pixels and, with normals, facing the camera within min_facing_cos
        -> (g (4, 4) = [R | t], model frame to camera frame; mask (K,) bool; inliers (DMATCH, input
        order); best); with debug also counts (4 * samples,) int32 (-1 for an invalid hypothesis) and
        models (4 * samples, 12: R row-major, then t).  matches: queryIdx into kpts, trainIdx into pts.
        No valid model: a zero g, no inliers, best -1.  refine (0 .. 16): that many rounds of a
        Gauss-Newton step on the matches the model accepts, each adopted iff valid and no worse in
        count; with refine > 0 and debug three more: roundCounts (refine + 1,) int32 (c_0, then each
        round's count: -1 an invalid step, -2 a round not run), roundModels (refine, 12) and the number
        of rounds adopted."""
        o = self._opts(max_px, min_facing_cos, samples, seed, refine)
        X = _xyz(pts)
        n = None if normals is None else _xyz(normals, X.shape[0])
        kp = np.ascontiguousarray(kpts, dtype=np.float32).reshape(-1, 2)
        m = np.ascontiguousarray(matches, dtype=DMATCH)
        K = m.shape[0]
        buf = self._outputs(K, o, debug)
        self.ctx.check(lib().fm3d_localize_points(self.ctx.handle, _vp(X), _vp(n), X.shape[0], _vp(kp), kp.shape[0], _vp(m),
                                                  K, ctypes.byref(o), *ModelAligner._tail(buf)))
        return ModelAligner._result(buf, K, o, debug)

    def match_and_localize(self, desc_img, kpts, desc_model, pts, epsilon, max_px, normals=None,
                           min_facing_cos: float = 0.0, samples: int = 256, seed: int = 0, refine: int = 0,
                           debug: bool = False, binary: bool = False):
        """fm3d_localize_model: the context's matcher (NNDR at epsilon; the settings' crossCheck is
        honoured) with the image's descriptor rows as queries and the model's as train, then localize()
        on its matches without a trip through the host -> (matches (DMATCH),) + localize()'s result."""
        o = self._opts(max_px, min_facing_cos, samples, seed, refine)
        di, dm = np.ascontiguousarray(desc_img), np.ascontiguousarray(desc_model)
        X = _xyz(pts, dm.shape[0])
        n = None if normals is None else _xyz(normals, X.shape[0])
        kp = np.ascontiguousarray(kpts, dtype=np.float32).reshape(-1, 2)
        nK = di.shape[0]
        if kp.shape[0] != nK:
            raise ValueError(f"expected {nK} keypoints, got {kp.shape[0]}")
        matches = np.zeros(max(nK, 1), dtype=DMATCH)
        nm = ctypes.c_int(0)
        buf = self._outputs(nK, o, debug)
        self.ctx.check(lib().fm3d_localize_model(self.ctx.handle, _vp(di), _vp(kp), nK, _vp(dm), _vp(X), _vp(n), X.shape[0],
                                                 di.shape[1], _desc_type(di, binary), ctypes.c_double(float(epsilon)),
                                                 ctypes.byref(o), _vp(matches), ctypes.byref(nm),
                                                 *ModelAligner._tail(buf)))
        K = nm.value
        return (matches[:K].copy(),) + ModelAligner._result(buf, K, o, debug)


class MOSAIC:
    """MOSAIC (mosaic.h:47-70, mosaic.cpp:32-73): the reference's descriptor extractor built on the
    whole pipeline.  The constructor runs the reference's seven steps on the GPU -- SURF
    compareWithNNDR on the two images, setg12, setKeypoints + triangulate, setImages +
    computeOptimizedNormals + computeFeaturesFrames, the reference square neighbourhood, and the
    normal-rectified patches of image A (projectReferencePointsToImageWithFrames).  The reference's
    computeImpl is empty (mosaic.cpp:75-79); compute() finishes it the way the reference's main()
    does (main.cpp:182-183): extractDescriptorsFromPatches of the patches, one SURF row per kept
    feature (descriptorType CV_32F, descriptorSize 128)."""

    descriptorSize = 128

    def __init__(self, ctx: Context, imgA: np.ndarray, imgB: np.ndarray, tA, tB, rA, rB):
        self.ctx = ctx
        s = ctx.settings
        self.imgA = np.ascontiguousarray(imgA, dtype=np.uint8)
        self.imgB = np.ascontiguousarray(imgB, dtype=np.uint8)
        # 2 - matches (descriptorsmatcher.cpp:107-131 from the images)
        self.dm = DescriptorsMatcher(ctx)
        self.matches, self.kptsA, self.kptsB, _, _ = self.dm.compareWithNNDRImages(s.nndrEpsilon, self.imgA, self.imgB)
        # 3 - g12 (singlecameratriangulator.cpp:123-143)
        self.sct = SingleCameraTriangulator(ctx)
        self.gAB = self.sct.setg12(tA, tB, rA, rB)
        # 4 - triangulation of the matches (:145-230)
        xy = lambda k: np.stack([k["x"], k["y"]], axis=1).astype(np.float32)
        self.sct.setKeypoints(xy(self.kptsA), xy(self.kptsB), self.matches)
        pts, self.outliersMask = self.sct.triangulate()
        # 5 - normals and feature frames (normaloptimizer.cpp:191-504)
        self.no = NormalOptimizer(ctx, self.sct)
        self.no.setImages(self.imgA, self.imgB)
        self.triangulated_points, self.normals = self.no.computeOptimizedNormals(pts)
        self.features_frames = self.no.computeFeaturesFrames(self.triangulated_points, self.normals)
        # 6 - the reference neighbourhood (neighborhoodsgenerator.cpp:134-158)
        self.ng = NeighborhoodsGenerator(s)
        self.reference_neighborhood = self.ng.getReferenceSquaredNeighborhood()
        # 7 - patches of image A (singlecameratriangulator.cpp:769-849)
        self.patches, self.image_points = self.sct.projectReferencePointsToImageWithFrames(
            self.reference_neighborhood, self.features_frames, image_points=True)

    def descriptorType(self):
        return np.float32

    def compute(self) -> np.ndarray:
        """The patch descriptors: (kept features, cols) rows of the settings' extractor (float32 for
        SURF / SIFT, uint8 for ORB / BRISK)."""
        feats = Features(self.ctx)
        if len(self.patches) == 0:
            cols, dt = feats.descriptor_info()
            return np.zeros((0, cols), dtype=dt)
        return feats.extractDescriptorsFromPatches(self.patches)
