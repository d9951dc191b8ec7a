"""The table of public entry points that tests/test_gpu_poison.py and tests/test_gpu_context_reuse.py
share: per case the context's settings, the inputs (a sequence that grows, shrinks and re-strides
the context's buffers; its first and last steps are the same input), the call and the reference
the entry point's own test compares with.

A case's run returns a flat list of arrays; two results are the same when every array has the same
shape, dtype and bytes (records field by field, so that a dtype's padding does not count).  The
references are computed once per (case, step) and shared by both test modules; nothing changes
them afterwards."""
import os

import numpy as np

from conftest import oracle_threads

KP_FIELDS = ("x", "y", "size", "angle", "response", "octave", "class_id")
_WORLD = {}
_REFS = {}


class World:
    def __init__(self, fm3d, orc, synth):
        self.fm3d, self.orc, self.synth = fm3d, orc, synth
        img = synth.make_frame_pair(2000, seed=3).img1
        self.L = np.ascontiguousarray(img[:300, :400])
        self.S = np.ascontiguousarray(img[:97, :131])
        self.T = np.ascontiguousarray(img[:131, :97])   # S's pixel count, another stride
        self.images = {"L": self.L, "S": self.S, "T": self.T}
        self._cache = {}

    def once(self, key, make):
        if key not in self._cache:
            self._cache[key] = make()
        return self._cache[key]

    def pair(self, n, seed, **kw):
        return self.once(("pair", n, seed, tuple(sorted(kw.items()))),
                         lambda: self.synth.make_frame_pair(n, seed=seed, **kw))


def world(fm3d, orc, synth):
    if "w" not in _WORLD:
        _WORLD["w"] = World(fm3d, orc, synth)
    return _WORLD["w"]


class Case:
    """name; settings(fm3d, world) -> Settings; steps: the reuse sequence's inputs (hashable keys);
    small: the inputs the poison test runs, each on a fresh context; run(world, ctx, x) -> list of
    arrays; ref(world, settings, x) -> the list run must equal, or check(world, settings, x, got)
    where the entry point's own test has an assert helper; env: variables set around every run"""


    def __init__(self, name, settings, steps, small, run, ref=None, check=None, env=None, opener=None):
        self.name, self.settings, self.steps, self.small_keys = name, settings, list(steps), list(small)
        self.run, self.ref, self.check, self.env = run, ref, check, dict(env or {})
        self.opener = opener   # (fm3d, settings) -> what run gets in place of a Context (it has close())

    def __repr__(self):
        return self.name


class _Env:
    def __init__(self, env):
        self.env, self.old = env, {}

    def __enter__(self):
        for k, v in self.env.items():
            self.old[k] = os.environ.get(k)
            os.environ[k] = v

    def __exit__(self, *a):
        for k, v in self.old.items():
            if v is None:
                del os.environ[k]
            else:
                os.environ[k] = v


def open_ctx(fm3d, case, w):
    s = case.settings(fm3d, w)
    return case.opener(fm3d, s) if case.opener else fm3d.Context(s)


def run_on(case, w, ctx, x):
    with _Env(case.env):
        return [np.asarray(a) for a in case.run(w, ctx, x)]


def run_fresh(fm3d, case, w, x):
    ctx = open_ctx(fm3d, case, w)
    try:
        return run_on(case, w, ctx, x)
    finally:
        ctx.close()


def _same_array(a, b, what):
    assert a.dtype == b.dtype and a.shape == b.shape, (what, a.dtype, b.dtype, a.shape, b.shape)
    if a.dtype.names:
        for f in a.dtype.names:
            assert np.ascontiguousarray(a[f]).tobytes() == np.ascontiguousarray(b[f]).tobytes(), (what, f)
    else:
        assert np.ascontiguousarray(a).tobytes() == np.ascontiguousarray(b).tobytes(), what


def assert_same(got, want, what):
    assert len(got) == len(want), (what, len(got), len(want))
    for i, (a, b) in enumerate(zip(got, want)):
        _same_array(np.asarray(a), np.asarray(b), f"{what}: output {i}")


def check_reference(case, w, x, got):
    s = case.settings(w.fm3d, w)
    if case.check is not None:
        case.check(w, s, x, got)
        return
    key = (case.name, x)
    if key not in _REFS:
        _REFS[key] = [np.asarray(a) for a in case.ref(w, s, x)]
    want = _REFS[key]
    assert len(got) == len(want), (case.name, x, len(got), len(want))
    for i, (a, b) in enumerate(zip(got, want)):
        if b.dtype.names:   # keypoints: the fields the oracle fills
            assert len(a) == len(b), (case.name, x, i, len(a), len(b))
            for f in KP_FIELDS if "class_id" in b.dtype.names else b.dtype.names:
                assert np.array_equal(a[f], b[f]), (case.name, x, i, f)
        else:
            assert a.shape == b.shape and np.array_equal(a, b, equal_nan=b.dtype.kind == "f"), (case.name, x, i)


def _settings(**kw):
    def make(fm3d, w):
        s = fm3d.Settings.default()
        for k, v in kw.items():
            setattr(s, k, getattr(fm3d, v) if isinstance(v, str) else v)
        return s
    return make


IMG_STEPS = ["L", "S", "T", "L"]
CASES = []


def case(*a, **kw):
    CASES.append(Case(*a, **kw))


# ---------------------------------------------------------------- detectors and extractors on images
def _surf(upright, extended):
    def run(w, ctx, x):
        k, d = w.fm3d.SURF(ctx).detect(w.images[x], with_descriptors=True)
        return [k, d]

    def ref(w, s, x):
        img = w.images[x]
        ko = w.orc.surf_detect(img, s.surfHessianThreshold, s.surfOctaves, s.surfOctaveLayers, upright=bool(upright))
        _, kept, do = w.orc.surf_describe(img, ko, extended=bool(extended), upright=bool(upright))
        assert np.array_equal(kept, np.arange(len(ko)))
        return [ko, do]
    name = f"surf_{'upright' if upright else 'oriented'}_{128 if extended else 64}"
    case(name, _settings(surfUpright=upright, surfExtended=extended, surfHessianThreshold=100.0), IMG_STEPS, ["S"], run, ref)


for _u in (1, 0):
    for _e in (1, 0):
        _surf(_u, _e)


def _sift_kw(s):
    return dict(nfeatures=s.siftNumFeatures, nOctaveLayers=s.siftOctaveLayers, contrastThreshold=s.siftContrastThreshold,
                edgeThreshold=s.siftEdgeThreshold, sigma=s.siftSigma)


def _sift_run(w, ctx, x):
    k, d = w.fm3d.SIFT(ctx).detect(w.images[x], with_descriptors=True)
    return [k, d]


def _sift_ref(w, s, x):
    img = w.images[x]
    ko = w.orc.sift_detect(img, **_sift_kw(s))
    assert len(ko) > 0
    return [ko, w.orc.sift_compute(img, ko)[2]]


case("sift", _settings(detectorType="FEAT_SIFT", extractorType="FEAT_SIFT"), IMG_STEPS, ["S"], _sift_run, _sift_ref)


def _orb_kw(s):
    return dict(nfeatures=s.orbNumFeatures, scaleFactor=s.orbScaleFactor, nlevels=s.orbNumLevels,
                edgeThreshold=s.orbEdgeThreshold, patchSize=s.orbPatchSize, fastThreshold=s.orbFastThreshold)


def _orb_run(w, ctx, x):
    k, d = w.fm3d.ORB(ctx).detect(w.images[x], with_descriptors=True)
    return [k, d]


def _orb_ref(w, s, x):
    ko, do = w.orc.orb_detect(w.images[x], **_orb_kw(s))
    return [ko, do]


case("orb", _settings(detectorType="FEAT_ORB", extractorType="FEAT_ORB"), IMG_STEPS, ["S"], _orb_run, _orb_ref)

case("fast", _settings(detectorType="FEAT_FAST", fastThreshold=10, fastNonmax=1), IMG_STEPS, ["S"],
     lambda w, ctx, x: [w.fm3d.Features(ctx).detect(w.images[x]), w.fm3d.Features(ctx).fast(w.images[x], 25, False)],
     lambda w, s, x: [w.orc.fast_detect(w.images[x], 10, True), w.orc.fast_detect(w.images[x], 25, False)])

for _kind, _lo, _hi in (("FAST", 100, 120), ("SURF", 40, 50)):
    case(f"adaptive_{_kind.lower()}",
         _settings(detectorType="FEAT_" + _kind, detectorMode=1, adaptiveMinFeatures=_lo, adaptiveMaxFeatures=_hi,
                   adaptiveMaxIters=30), IMG_STEPS, ["S"],
         lambda w, ctx, x: [w.fm3d.Features(ctx).detect(w.images[x])],
         lambda w, s, x, kind=_kind, lo=_lo, hi=_hi: [w.orc.adaptive_detect(w.images[x], kind, lo, hi, 30)])

STAR = (16, 20, 10, 8, 3)
case("star", _settings(), IMG_STEPS, ["S"],
     lambda w, ctx, x: [w.fm3d.Features(ctx).star(w.images[x], *STAR)],
     lambda w, s, x: [w.orc.star_detect(w.images[x], *STAR)])

MSER = dict(min_area=10, max_area=800)   # every image here fits the LDS bitmap (kMserLdsBits pixels)


def _mser_run(w, ctx, x):
    F = w.fm3d.Features(ctx)
    img = w.images[x]
    flip = np.ascontiguousarray(img[::-1])
    return [F.mser(img, **MSER)] + list(F.mser_batch([img, flip, img], **MSER))


def _mser_ref(w, s, x):
    img = w.images[x]
    a, b = w.orc.mser_detect(img, **MSER), w.orc.mser_detect(np.ascontiguousarray(img[::-1]), **MSER)
    return [a, a, b, a]


case("mser", _settings(), IMG_STEPS, ["S"], _mser_run, _mser_ref)


# ---------------------------------------------------------------- extractors on caller keypoints
KP_STEPS = [800, 5, 0, 800]


def caller_keypoints(fm3d, n, w, h):
    """keypoints of every size and border position (tests/test_gpu_brisk.py's recipe), a prefix of one
    draw so that the five are the first five of the 800"""
    rng = np.random.default_rng(17)
    k = np.zeros(800, dtype=fm3d.KEYPOINT)
    k["x"] = rng.uniform(-5, w + 5, 800)
    k["y"] = rng.uniform(-5, h + 5, 800)
    k["size"] = rng.choice([0.0, 1e-9, 3.0, 7.0, 7.2, 9.0, 12.5, 20.0, 31.0, 44.6, 64.0, 90.0], 800)
    k["size"][:5] = [7.0, 20.0, 0.0, 31.0, 9.0]
    k["angle"] = np.where(rng.random(800) < 0.3, -1.0, rng.uniform(0, 360, 800))
    k["response"] = rng.random(800)
    return k[:n].copy()


def _compute_run(w, ctx, n):
    h, wd = w.L.shape
    kc, kept, d = w.fm3d.Features(ctx).compute(w.L, caller_keypoints(w.fm3d, n, wd, h))
    return [kc, kept, d]


def _compute_ref(fn, **kw):
    def ref(w, s, n):
        h, wd = w.L.shape
        ko, kept, do = getattr(w.orc, fn)(w.L, caller_keypoints(w.fm3d, n, wd, h), **kw)
        return [ko, kept, do]
    return ref


case("brisk_compute", _settings(extractorType="FEAT_BRISK"), KP_STEPS, [5], _compute_run, _compute_ref("brisk_compute"))
case("freak_compute", _settings(extractorType="FEAT_FREAK"), KP_STEPS, [5], _compute_run, _compute_ref("freak_compute"))


def _surf_compute_run(w, ctx, n):
    h, wd = w.L.shape
    k = caller_keypoints(w.fm3d, n, wd, h)
    k["size"] = np.where(k["size"] < 0.36, 0.0, k["size"])   # a kept size below 0.36 is refused (test_gpu_surf.py)
    k["angle"] = -1
    kc, kept, d = w.fm3d.SURF(ctx).compute(w.L, k)
    return [kc, kept, d]


def _surf_compute_ref(upright):
    def ref(w, s, n):
        h, wd = w.L.shape
        k = caller_keypoints(w.fm3d, n, wd, h)
        k["size"] = np.where(k["size"] < 0.36, 0.0, k["size"])
        k["angle"] = -1
        ko, kept, do = w.orc.surf_describe(w.L, k, extended=True, upright=upright)
        return [ko, kept, do]
    return ref


case("surf_compute_upright", _settings(surfUpright=1), KP_STEPS, [5], _surf_compute_run, _surf_compute_ref(True))
case("surf_compute_oriented", _settings(surfUpright=0), KP_STEPS, [5], _surf_compute_run, _surf_compute_ref(False))


# ---------------------------------------------------------------- matchers
# name -> (oracle type, dim, binary, integer-valued floats, environment)
MATCH_KINDS = {
    "u8-128": (1, 128, False, False, {}),
    "u8-100": (1, 100, False, False, {}),            # padded to the kernel's row on the host
    "f32-64": (0, 64, False, False, {}),
    "f32-128-int": (0, 128, False, True, {}),        # integer-valued floats: packed to u8 on the device
    "f32-36": (0, 36, False, False, {}),
    "bits-32-mfma": (2, 32, True, False, {"FM3D_BITS_MFMA": "1"}),
    "bits-32-valu": (2, 32, True, False, {"FM3D_BITS_MFMA": "0"}),
    "bits-64": (2, 64, True, False, {}),
    "f32-128": (0, 128, False, False, {}),           # the prefilter sequence only
}
MATCH_STEPS = [(600, 9001), (5, 2), (130, 1), (40, 0), (300, 4099), (600, 9001)]
PREFILTER_STEPS = [(2048, 2051), (5, 2), (2048, 2051)]   # nA * nB >= 2^22: the bf16 prefilter
MATCH_EPS = 0.9
_ROWS = {}


def match_rows(kind, nA, nB):
    """random rows; every second query is a train row with a little noise, so that the ratio test keeps
    some matches and drops others"""
    key = (kind, nA, nB)
    if key not in _ROWS:
        typ, dim, _, integer, _ = MATCH_KINDS[kind]
        rng = np.random.default_rng([nA, nB, dim, typ])
        if typ == 0 and not integer:
            A = rng.normal(0, 0.1, (nA, dim)).astype(np.float32)
            B = rng.normal(0, 0.1, (nB, dim)).astype(np.float32)
            if nB:
                A[::2] = B[(np.arange(0, nA, 2) * 7) % nB] + rng.normal(0, 0.03, (len(A[::2]), dim)).astype(np.float32)
        else:
            hi = 256 if typ != 0 else 200
            A = rng.integers(0, hi, (nA, dim), dtype=np.uint8)
            B = rng.integers(0, hi, (nB, dim), dtype=np.uint8)
            if nB:
                near = B[(np.arange(0, nA, 2) * 7) % nB].copy()
                near[:, ::5] ^= rng.integers(0, 8, near[:, ::5].shape, dtype=np.uint8)
                A[::2] = near
            if typ == 0:
                A, B = A.astype(np.float32), B.astype(np.float32)
        A.setflags(write=False)
        B.setflags(write=False)
        _ROWS[key] = (A, B)
    return _ROWS[key]


def _match(kind, steps, small, suffix=""):
    typ, dim, binary, _, env = MATCH_KINDS[kind]

    def run(w, ctx, x):
        A, B = match_rows(kind, *x)
        dm = w.fm3d.DescriptorsMatcher(ctx, binary=binary)
        got = dm.knn_match(A, B)
        out = [got["trainIdx"], np.where(got["trainIdx"] >= 0, got["distance"], 0)]
        if x[1] >= 1:
            m = dm.compareWithNNDR(MATCH_EPS, A, B)
            out += [m["queryIdx"], m["trainIdx"], m["distance"]]
        return out

    def ref(w, s, x):
        A, B = match_rows(kind, *x)
        idx, dist = w.orc.knn2(A, B, typ, oracle_threads())
        out = [idx, np.where(idx >= 0, dist, 0)]
        if x[1] >= 1:
            out += list(w.orc.nndr(idx, dist, MATCH_EPS))
        return out

    case(f"match_{kind}{suffix}", _settings(), steps, small, run, ref, env=env)


for _k in MATCH_KINDS:
    if _k != "f32-128":
        _match(_k, MATCH_STEPS, [(5, 2), (300, 4099)])
for _k in ("f32-64", "f32-128"):
    _match(_k, PREFILTER_STEPS, [(2048, 2051)], "_prefilter")


# ---------------------------------------------------------------- the guided matcher and the cross-check
GATE_STEPS = [(402, 3000), (5, 2), (402, 3000)]
GATE_PX = 8.0


def _gate_settings(fm3d, w):
    s = fm3d.Settings.default()
    s.set_camera(w.synth.Camera.reference(640))
    return s


def _gate_ctx(w, ctx):
    w.fm3d.SingleCameraTriangulator(ctx).set_g12(w.synth.reference_g12())


def _gate_inputs(w, kind, x):
    """tests/test_cross_check.py's rows (equal distances are common) and keypoints; the reference gate from
    the library's undistortion on a context of its own, once per shape"""
    import test_cross_check as tcc
    a, b = tcc.descriptors(kind, x[0], x[1], 7)
    k1, k2 = tcc.keypoints(*x)

    def gate():
        ctx = w.fm3d.Context(_gate_settings(w.fm3d, w))
        try:
            _gate_ctx(w, ctx)
            return tcc.gate_of(w.fm3d, ctx, k1, k2, GATE_PX)[1]
        finally:
            ctx.close()
    return a, b, k1, k2, gate


def _dm_list(m):
    return [m["queryIdx"], m["trainIdx"], m["distance"]]


def _guided(kind):
    import test_cross_check as tcc
    typ, _, binary = tcc.KINDS[kind]

    def run(w, ctx, x):
        a, b, k1, k2, _ = _gate_inputs(w, kind, x)
        _gate_ctx(w, ctx)
        dm = w.fm3d.DescriptorsMatcher(ctx, binary=binary)
        m = dm.knn_match_guided(a, b, k1, k2, GATE_PX)
        return [m["trainIdx"], np.where(m["trainIdx"] >= 0, m["distance"], 0)] + _dm_list(
            dm.compareWithNNDRGuided(MATCH_EPS, a, b, k1, k2, GATE_PX))

    def ref(w, s, x):
        a, b, k1, k2, gate = _gate_inputs(w, kind, x)
        idx, dist = tcc.knn_ref(w.orc, a, b, typ, w.once(("gate", x), gate))
        return [idx, np.where(idx >= 0, dist, 0)] + list(w.orc.nndr(idx, dist, MATCH_EPS))

    case(f"guided_{kind}", _gate_settings, GATE_STEPS, [(5, 2), (402, 3000)], run, ref)


def _cross(kind, mode, guided):
    import test_cross_check as tcc
    typ, _, binary = tcc.KINDS[kind]

    def run(w, ctx, x):
        a, b, k1, k2, _ = _gate_inputs(w, kind, x)
        _gate_ctx(w, ctx)
        dm = w.fm3d.DescriptorsMatcher(ctx, binary=binary)
        if guided:
            return _dm_list(dm.compareWithNNDRMutualGuided(0.98, a, b, k1, k2, GATE_PX, mode=mode))
        return _dm_list(dm.compareWithNNDRMutual(0.98, a, b, mode=mode))

    def ref(w, s, x):
        a, b, k1, k2, gate = _gate_inputs(w, kind, x)
        fwd, rev = w.once(("two_way", kind, x, guided),
                          lambda: tcc.two_way(w.orc, a, b, typ, w.once(("gate", x), gate) if guided else None))
        return list(tcc.mutual_ref(w.orc, fwd, rev, 0.98, mode))

    case(f"cross{mode}_{'guided_' if guided else ''}{kind}", _gate_settings, GATE_STEPS, [(5, 2), (402, 3000)], run, ref)


for _k in ("u8-128", "f32-64", "bits-32"):
    _guided(_k)
    for _m in (1, 2):
        _cross(_k, _m, False)
    _cross(_k, 1, True)


# ---------------------------------------------------------------- extractDescriptorsFromPatches
PATCH_STEPS = [24, 3, 24]


def patch_stack(n):
    """128 x 128 patches with an oriented ramp under noise (tests/test_gpu_surf.py's recipe); a prefix of
    one draw"""
    rng = np.random.default_rng(19)
    patches = rng.integers(0, 256, (24, 128, 128), dtype=np.uint8)
    yy, xx = np.mgrid[0:128, 0:128]
    for i in range(24):
        a = i * 15 * np.pi / 180
        patches[i] = np.clip(patches[i] // 4 + 96 + 0.6 * ((xx - 64) * np.cos(a) + (yy - 64) * np.sin(a)), 0, 255)
    return patches[:n].copy()


def _centred(fm3d):
    kp = np.zeros(1, dtype=fm3d.KEYPOINT)
    kp["x"] = kp["y"] = 64
    kp["size"], kp["angle"], kp["response"] = 128, -1, 1
    return kp


def _patches_run(w, ctx, n):
    return [w.fm3d.Features(ctx).extractDescriptorsFromPatches(patch_stack(n))]


def _patches_ref(row):
    def ref(w, s, n):
        return [np.stack([row(w, s, p, _centred(w.fm3d)) for p in patch_stack(n)])]
    return ref


case("patches_surf_upright", _settings(extractorType="FEAT_SURF", surfUpright=1), PATCH_STEPS, [3], _patches_run,
     _patches_ref(lambda w, s, p, kp: w.orc.surf_describe(p, kp, extended=True, upright=True)[2][0]))
case("patches_surf_oriented", _settings(extractorType="FEAT_SURF", surfUpright=0), PATCH_STEPS, [3], _patches_run,
     _patches_ref(lambda w, s, p, kp: w.orc.surf_describe(p, kp, extended=True, upright=False)[2][0]))
case("patches_sift", _settings(extractorType="FEAT_SIFT"), PATCH_STEPS, [3], _patches_run,
     _patches_ref(lambda w, s, p, kp: w.orc.sift_compute(p, kp)[2][0]))
case("patches_orb", _settings(extractorType="FEAT_ORB"), PATCH_STEPS, [3], _patches_run,
     _patches_ref(lambda w, s, p, kp: w.orc.orb_compute(p, kp, edgeThreshold=s.orbEdgeThreshold,
                                                        patchSize=s.orbPatchSize)[2][0]))
for _ex in ("BRISK", "FREAK"):   # the centred keypoint needs a pattern larger than the patch: zero rows
    case(f"patches_{_ex.lower()}", _settings(extractorType="FEAT_" + _ex), PATCH_STEPS, [3], _patches_run,
         lambda w, s, n: [np.zeros((n, 64), dtype=np.uint8)])


# ---------------------------------------------------------------- geometry on the frame pairs
PAIRS = {"big": (3000, 11), "small": (400, 2)}
PAIR_STEPS = ["big", "small", "big"]
RAY = 16


def pair_of(w, x):
    return w.pair(*PAIRS[x])


def _pair_settings(**kw):
    def make(fm3d, w):
        big, small = pair_of(w, "big"), pair_of(w, "small")
        assert big.cam == small.cam   # one context serves both pairs
        s = fm3d.Settings.default()
        s.set_camera(big.cam)
        s.pixelsRay = RAY
        for k, v in kw.items():
            setattr(s, k, v)
        return s
    return make


def oracle_chain(w, x):
    """the oracle's matches and triangulated points of a pair, once"""
    def make():
        p = pair_of(w, x)
        q, t, d = w.orc.match_nndr(p.desc1, p.desc2, w.orc.U8, 0.55, oracle_threads())
        pts, mask = w.orc.triangulate(p.cam, p.g12, 1.5, 2.4, p.kp1, p.kp2, q, t)
        return q, t, d, pts, mask
    return w.once(("chain", x), make)


def _tri_run(w, ctx, x):
    p = pair_of(w, x)
    q, t, d, _, _ = oracle_chain(w, x)
    m = np.zeros(len(q), dtype=w.fm3d.DMATCH)
    m["queryIdx"], m["trainIdx"], m["distance"] = q, t, d
    sct = w.fm3d.SingleCameraTriangulator(ctx)
    sct.set_g12(p.g12)
    sct.setKeypoints(p.kp1, p.kp2, m)
    pts, mask = sct.triangulate()
    return [pts, mask]


case("triangulate", _pair_settings(), PAIR_STEPS, ["small"], _tri_run,
     lambda w, s, x: [oracle_chain(w, x)[3], oracle_chain(w, x)[4]])

POINT_STEPS = [120, 7, 0, 120]
EXTRA_POINTS = np.array([[-1.3, -0.95, 2.0], [5.0, 5.0, 2.0], [0.0, 0.0, 2.0]])   # a trimmed neighbourhood, no pixels


def lm_points(w, n):
    return np.concatenate([EXTRA_POINTS, oracle_chain(w, "big")[3]])[:n]


def _normals_run(w, ctx, n):
    p = pair_of(w, "big")
    sct = w.fm3d.SingleCameraTriangulator(ctx)
    sct.set_g12(p.g12)
    no = w.fm3d.NormalOptimizer(ctx, sct)
    no.setImages(p.img1, p.img2)
    kept, normals = no.computeOptimizedNormals(lm_points(w, n))
    if n == 0:
        return [kept, normals]
    return [kept, normals, no.last_status, no.last_info[:, :4], no.last_nfev[:, :4]]


def _normals_ref(tree):
    def ref(w, s, n):
        p, P = pair_of(w, "big"), lm_points(w, n)
        if n == 0:
            return [np.zeros((0, 3)), np.zeros((0, 3))]
        R2, t2 = w.fm3d.camera2_from_g12(p.g12)
        mode = w.orc.DETMATH | (w.orc.TREE | w.orc.GRAM if tree else 0)
        r = w.orc.optimize_normals(p.cam, R2, t2, p.img1, p.img2, s.pyramids, P, RAY, s.boundWidth, s.boundHeight,
                                   mode=mode, nthreads=oracle_threads())
        ok = r["status"] == 0
        return [P[ok], r["normals"][ok], r["status"], r["info"][:, :4], r["nfev"][:, :4]]
    return ref


case("normals", _pair_settings(), POINT_STEPS, [7], _normals_run, _normals_ref(False))
case("normals_tree", _pair_settings(lmReduction=1), POINT_STEPS, [7], _normals_run, _normals_ref(True))

NCC_STEPS = [300, 5, 300]


def _ncc_points(w, n):
    p = pair_of(w, "big")
    return np.concatenate([[[0.0, 0.0, 0.0], [5.0, 5.0, 2.0]], p.points])[:n]


def _ncc_run(w, ctx, n):
    p = pair_of(w, "big")
    sct = w.fm3d.SingleCameraTriangulator(ctx)
    sct.set_g12(p.g12)
    no = w.fm3d.NormalOptimizer(ctx, sct)
    no.setImages(p.img1, p.img2)
    sc, nb, b = no.nccHypotheses(_ncc_points(w, n), 3, 4, 0.4)
    return [sc, nb, b]


def _ncc_ref(w, s, n):
    p = pair_of(w, "big")
    R2, t2 = w.fm3d.camera2_from_g12(p.g12)
    return list(w.orc.ncc_hypotheses(p.cam, R2, t2, p.img1, p.img2, _ncc_points(w, n), RAY, 3, 4, 0.4, bound=(640, 480)))


case("ncc_hypotheses", _pair_settings(boundWidth=640, boundHeight=480), NCC_STEPS, [5], _ncc_run, _ncc_ref)


# ---------------------------------------------------------------- frames, patch export, neighbourhoods
FRAME_STEPS = [60, 3, 0, 60]


def _frame_inputs(w, n):
    pts = oracle_chain(w, "big")[3][:n]
    nrm = pts + np.random.default_rng(5).normal(0, 0.3, (60, 3))[:n]
    return pts, nrm / np.linalg.norm(nrm, axis=1, keepdims=True)


def _frames_run(w, ctx, n):
    p = pair_of(w, "big")
    pts, nrm = _frame_inputs(w, n)
    s = ctx.settings
    no = w.fm3d.NormalOptimizer(ctx)
    no.setImages(p.img1, p.img2)
    frames = no.computeFeaturesFrames(pts, nrm)
    ng = w.fm3d.NeighborhoodsGenerator(s)
    patches, ipts = w.fm3d.SingleCameraTriangulator(ctx).projectReferencePointsToImageWithFrames(
        ng.getReferenceSquaredNeighborhood(), frames, image_points=True)
    sq = ng.computeSquareNeighborhoodsByNormals(ctx, frames)
    return [frames, patches, ipts, sq]


def _circular_run(w, ctx, n):
    pts, nrm = _frame_inputs(w, n)
    ng = w.fm3d.NeighborhoodsGenerator(ctx.settings)
    return [ng.computeCircularNeighborhoodsByNormals(ctx, pts, nrm), ng.computeCircularNeighborhoodsByNormals(ctx, pts)]


def _circular_ref(w, s, n):
    pts, nrm = _frame_inputs(w, n)
    return [w.orc.circular_neighborhoods(pts, nrm, s.neighEpsilon, s.neighThetas, s.neighRays),
            w.orc.circular_neighborhoods(pts, None, s.neighEpsilon, s.neighThetas, s.neighRays)]


def _frames_ref(w, s, n):
    p = pair_of(w, "big")
    orc = w.orc
    pts, nrm = _frame_inputs(w, n)
    frames = orc.features_frames(pts, nrm, orc.gravity(list(s.rodriguesIC)))
    patches, ipts = orc.export_patches(p.cam, p.img1, frames, s.neighEpsilon, s.cmPerPixel, mode=orc.DETMATH,
                                       image_points=True)
    return [frames, patches, ipts, orc.square_neighborhoods(frames.reshape(-1, 16), s.neighEpsilon, s.cmPerPixel)]


case("frames_patches_square", _pair_settings(neighEpsilon=0.16, cmPerPixel=0.25), FRAME_STEPS, [3], _frames_run, _frames_ref)
case("circular_neighbourhoods", _pair_settings(neighMethod=1, neighThetas=15, neighRays=5), FRAME_STEPS, [3],
     _circular_run, _circular_ref)


# ---------------------------------------------------------------- verify, align, localize
# (matches M, hypotheses or samples, refine rounds)
VERIFY_STEPS = [(1800, 512, 3), (9, 1, 0), (1025, 64, 1), (1800, 512, 3)]
MODEL_STEPS = [(1800, 512, 3), (3, 1, 0), (1025, 64, 1), (1800, 512, 3)]


def _tuple_of(arrays):
    return tuple(a if a.ndim else a.item() for a in arrays)


def _verify_case(w):
    import verify_pyref
    return w.once("verify_case", lambda: verify_pyref.reference_case(w.synth, w.orc))


def _verify_settings(fm3d, w):
    s = fm3d.Settings.default()
    s.set_camera(_verify_case(w)["pair"].cam)
    return s


def _verify_run(w, ctx, x):
    import test_gpu_verify_refit as tvr
    M, H, R = x
    c = _verify_case(w)
    m = tvr.shape_matches(c, M)
    p = c["pair"]
    return list(w.fm3d.SingleCameraTriangulator(ctx).verifyMatches(p.kp1, p.kp2, m, 1.0, hypotheses=H, seed=0, debug=True,
                                                                  refine=R))


def _verify_check(w, s, x, got):
    import test_gpu_verify_refit as tvr
    import verify_pyref as vp
    import verify_refit_pyref as rr
    M, H, R = x
    c = _verify_case(w)
    m, p = tvr.shape_matches(c, M), c["pair"]

    def make():
        x1, x2 = vp.coords(w.orc, p.cam, p.kp1, p.kp2, m)
        tau = vp.tau_of(p.cam, 1.0)
        ran = vp.ransac(w.orc, x1, x2, H, tau, 0)
        return ran, rr.refined(w.orc, ran, x1, x2, tau, R)
    ran, want = w.once(("verify_ref", x), make)
    tvr.assert_same(w.fm3d, _tuple_of(got), ran, want, m, R)


case("verify_matches", _verify_settings, VERIFY_STEPS, [(9, 1, 0), (1025, 64, 1)], _verify_run, check=_verify_check)


def _align_run(w, ctx, x):
    import align_pyref
    import test_gpu_align as tga
    M, H, R = x
    big = w.once("align_big", lambda: align_pyref.model_pair(N=1800))
    return list(w.fm3d.ModelAligner(ctx).align(big["A"], big["B"], big["matches"][:M], tga.MAX_DIST, big["nA"], big["nB"],
                                               0.9, hypotheses=H, seed=0, refine=R, debug=True))


def _align_check(w, s, x, got):
    import align_pyref
    import test_gpu_align as tga
    M, H, R = x
    big = w.once("align_big", lambda: align_pyref.model_pair(N=1800))
    m = big["matches"][:M]
    want = w.once(("align_ref", x), lambda: align_pyref.align(w.orc, big["A"], big["B"], m, tga.MAX_DIST, H, 0, R,
                                                              big["nA"], big["nB"], 0.9))
    tga.assert_same(w.fm3d, _tuple_of(got), want, m)


case("align_points", _settings(), MODEL_STEPS, [(3, 1, 0), (1025, 64, 1)], _align_run, check=_align_check)


def _pnp_scene(w):
    import pnp_pyref
    return w.once("pnp_big", lambda: pnp_pyref.scene(N=1800))


def _pnp_settings(fm3d, w):
    s = fm3d.Settings.default()
    s.set_camera(_pnp_scene(w)["cam"])
    return s


def _pnp_run(w, ctx, x):
    import test_gpu_pnp as tgp
    M, H, R = x
    big = _pnp_scene(w)
    return list(w.fm3d.ModelLocalizer(ctx).localize(big["X"], big["kpts"], big["matches"][:M], tgp.MAX_PX, big["n"], 0.5,
                                                    samples=H, seed=0, refine=R, debug=True))


def _pnp_check(w, s, x, got):
    import pnp_pyref
    import test_gpu_pnp as tgp
    M, H, R = x
    big = _pnp_scene(w)
    m = big["matches"][:M]
    want = w.once(("pnp_ref", x), lambda: pnp_pyref.localize(w.orc, big["cam"], big["X"], big["kpts"], m, tgp.MAX_PX, H, 0,
                                                             R, big["n"], 0.5))
    tgp.assert_same(w.fm3d, _tuple_of(got), want, m)


case("localize_points", _pnp_settings, MODEL_STEPS, [(3, 1, 0), (1025, 64, 1)], _pnp_run, check=_pnp_check)


# ---------------------------------------------------------------- the staged pipeline
PIPE_EPS, PIPE_CMPP = 0.645, 1.0   # 128 x 128 patches (tests/test_gpu_pipeline_describe.py)
PIPE_VERIFY = dict(hypotheses=64, seed=0, refine=1)
_pipe_settings = _pair_settings(neighEpsilon=PIPE_EPS, cmPerPixel=PIPE_CMPP)


def _counts(st):
    return np.array([st["queries"], st["trains"], st["matches"], st["inliers"], st["kept"]], dtype=np.int64)


def _pipe_run(w, ctx, x):
    p = pair_of(w, x)
    w.fm3d.SingleCameraTriangulator(ctx).set_g12(p.g12)
    pipe = w.fm3d.Pipeline(ctx)
    pipe.upload(p.desc1, p.desc2, p.kp1, p.kp2, p.img1, p.img2)
    n, st = pipe.run()
    rec = pipe.records(n).copy()
    desc, frames, _, _ = pipe.describe(n, frames=True)
    P, st2 = pipe.run_dlt()
    m, pts, src = pipe.dlt_results(st2["matches"], P)
    Pn, st3 = pipe.run_ncc(4, 4, 0.4)
    sc, nb, b = pipe.ncc_results(Pn, 16)
    n4, st4, rep = pipe.run_verified(1.0, **PIPE_VERIFY)
    rec4 = pipe.records(n4).copy()
    return [_counts(st), rec, desc, frames, _counts(st2), m, pts, src, _counts(st3), sc, nb, b, _counts(st4), rec4,
            np.array([rep["matches"], rep["verified"], rep["best"], rep["roundsAdopted"]]), rep["E"]]


def _fresh(case_name):
    """check: the bytes a fresh context of the case gives for this input, computed once"""
    def fresh(w, x):
        c = next(c for c in CASES if c.name == case_name)
        return w.once(("fresh", case_name, x), lambda: run_fresh(w.fm3d, c, w, x))
    return fresh


def _pipe_check(w, s, x, got):
    assert_same(got, _fresh("pipeline")(w, x), f"pipeline {x} vs a fresh context")
    if x != "small":
        return
    orc, p = w.orc, pair_of(w, x)
    (cnt, rec, desc, frames, cnt2, m, pts, src, cnt3, sc, nb, b, cnt4, rec4, rep, E) = got
    q, t, d, opts, mask = oracle_chain(w, x)

    def make():
        R2, t2 = w.fm3d.camera2_from_g12(p.g12)
        lm = orc.optimize_normals(p.cam, R2, t2, p.img1, p.img2, s.pyramids, opts, RAY, mode=orc.DETMATH,
                                  nthreads=oracle_threads())
        ncc = orc.ncc_hypotheses(p.cam, R2, t2, p.img1, p.img2, opts, RAY, 4, 4, 0.4, bound=(s.boundWidth, s.boundHeight),
                                 zmax=s.zThresholdMax)
        ok = lm["status"] == 0
        fr = orc.features_frames(opts[ok], lm["normals"][ok], orc.gravity(list(s.rodriguesIC)))
        pa = orc.export_patches(p.cam, p.img1, fr, PIPE_EPS, PIPE_CMPP, mode=orc.DETMATH)
        kp = _centred(w.fm3d)
        rows = np.stack([orc.surf_describe(a, kp, extended=bool(s.surfExtended), upright=bool(s.surfUpright))[2][0]
                         for a in pa])
        return lm, ncc, fr, rows
    lm, ncc, fr, rows = w.once(("pipe_oracle", x), make)
    ok = lm["status"] == 0
    assert list(cnt[2:]) == [len(q), len(opts), int(ok.sum())] and cnt[4] > 50
    assert np.array_equal(rec["queryIdx"], q[mask][ok]) and np.array_equal(rec["trainIdx"], t[mask][ok])
    assert np.array_equal(rec["point"], opts[ok]) and np.array_equal(rec["normal"], lm["normals"][ok])
    assert np.array_equal(frames, fr, equal_nan=True) and np.array_equal(desc, rows)
    assert np.array_equal(m["queryIdx"], q) and np.array_equal(m["trainIdx"], t) and np.array_equal(m["distance"], d)
    assert np.array_equal(pts, opts) and np.array_equal(src, np.nonzero(mask)[0])
    assert np.array_equal(sc, ncc[0]) and np.array_equal(nb, ncc[1], equal_nan=True) and np.array_equal(b, ncc[2])
    # the verified run under the known pose keeps a subset of the plain run's records, in order
    assert rep[0] == len(q) and 8 <= rep[1] <= rep[0] and rep[2] >= 0
    assert cnt4[2] == rep[1] and len(rec4) == cnt4[4] > 0
    pos = np.searchsorted(rec["queryIdx"], rec4["queryIdx"])
    assert (rec["queryIdx"][pos] == rec4["queryIdx"]).all()
    for f in ("trainIdx", "point", "normal"):
        assert np.array_equal(rec[f][pos], rec4[f]), f


case("pipeline", _pipe_settings, PAIR_STEPS, ["small"], _pipe_run, check=_pipe_check)


# ---------------------------------------------------------------- the multi-GPU run on one device
def _mgpu_run(w, mg, x):
    p = pair_of(w, x)
    mg.set_g12(p.g12)
    mg.upload(p.desc1, p.desc2, p.kp1, p.kp2, p.img1, p.img2)
    rec, st = mg.run()
    return [rec, _counts(st)]


def _mgpu_check(w, s, x, got):
    """byte-identical to fm3d_pipeline_run of the whole pair (tests/test_gpu_parity.py)"""
    def make():
        ctx = w.fm3d.Context(s)
        try:
            w.fm3d.SingleCameraTriangulator(ctx).set_g12(pair_of(w, x).g12)
            p, pipe = pair_of(w, x), w.fm3d.Pipeline(ctx)
            pipe.upload(p.desc1, p.desc2, p.kp1, p.kp2, p.img1, p.img2)
            n, st = pipe.run()
            return [pipe.records(n).copy(), _counts(st)]
        finally:
            ctx.close()
    want = w.once(("mgpu_ref", x), make)
    assert_same([got[0]], [want[0]], f"mgpu {x}: records vs fm3d_pipeline_run")
    assert list(got[1][2:]) == list(want[1][2:]) and len(got[0]) > 50


case("mgpu_one_device", _pair_settings(pyramids=1), PAIR_STEPS, ["small"], _mgpu_run, check=_mgpu_check,
     opener=lambda fm3d, s: fm3d.MultiGPU(s, devices=[0], shares=4, block=256))
