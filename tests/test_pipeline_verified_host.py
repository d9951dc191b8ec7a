"""fm3d_pipeline_run_verified / fm3d_pipeline_run_dlt_verified without a GPU (DESIGN.md §3.1d "In the
pipeline"): the exports, the two structures' layout against the C compiler's, the argument rules that
need no device, the Python wrappers' checks, and fm3d_pose_from_epipolar -- now built from the shared
functions of include/fm3d_epi8.h that the vote kernel runs -- against the restatement, bit for bit."""
import ctypes
import math
import os
import subprocess

import numpy as np
import pytest

import verify_pyref as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("fm3d_pipeline_run_verified", "fm3d_pipeline_run_dlt_verified")


def test_exports_listed(fm3d):
    for n in NAMES:
        assert n in fm3d.EXPORTS and hasattr(fm3d.lib(), n)


def c_layout(tmp_path, struct, fields):
    """(sizeof, [offsetof ...]) of a structure of include/fm3d.h from the C compiler"""
    src = '#include <stdio.h>\n#include <stddef.h>\n#include "fm3d.h"\nint main(void){'
    src += f'printf("%zu\\n", sizeof({struct}));'
    src += "".join(f'printf("%zu\\n", offsetof({struct}, {f}));' for f in fields) + "return 0;}"
    c, exe = tmp_path / f"{struct}.c", tmp_path / struct
    c.write_text(src)
    subprocess.run(["gcc", "-I", os.path.join(ROOT, "include"), str(c), "-o", str(exe)], check=True)
    out = [int(v) for v in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split()]
    return out[0], out[1:]


@pytest.mark.parametrize("struct, mirror", [("fm3d_verify_opts", "VerifyOpts"), ("fm3d_verify_report", "VerifyReport")])
def test_struct_layouts(fm3d, tmp_path, struct, mirror):
    cls = getattr(fm3d, mirror)
    fields = [f for f, _ in cls._fields_]
    size, offs = c_layout(tmp_path, struct, fields)
    assert size == ctypes.sizeof(cls)
    assert offs == [getattr(cls, f).offset for f in fields]


def test_null_context_or_options(fm3d):
    L = fm3d.lib()
    o, rep, st, n = fm3d.VerifyOpts(64, 0, 1.0, 0, 0, 0, 1.0), fm3d.VerifyReport(), fm3d.PipelineStats(), ctypes.c_int(7)
    assert L.fm3d_pipeline_run_verified(None, ctypes.byref(o), None, ctypes.byref(n), ctypes.byref(st),
                                        ctypes.byref(rep)) == fm3d.ERR_INVALID
    assert L.fm3d_pipeline_run_dlt_verified(None, ctypes.byref(o), ctypes.byref(n), ctypes.byref(st),
                                            ctypes.byref(rep)) == fm3d.ERR_INVALID
    assert L.fm3d_pipeline_run_verified(None, None, None, None, None, None) == fm3d.ERR_INVALID
    assert L.fm3d_pipeline_run_dlt_verified(None, None, None, None, None) == fm3d.ERR_INVALID


class NoLibrary:
    """a context whose use would be a call into the library"""
    handle = None

    def check(self, code):
        raise AssertionError("the library was called")


BAD = [dict(max_px=0.0), dict(max_px=-1.0), dict(max_px=math.nan), dict(max_px=math.inf), dict(hypotheses=0),
       dict(hypotheses=-5), dict(refine=-1), dict(refine=17), dict(pose_from_model=True, baseline=0.0),
       dict(pose_from_model=True, baseline=-2.0), dict(pose_from_model=True, baseline=math.nan),
       dict(pose_from_model=True, baseline=math.inf)]


@pytest.mark.parametrize("method", ["run_verified", "run_dlt_verified"])
@pytest.mark.parametrize("bad", BAD, ids=lambda d: ",".join(f"{k}={v}" for k, v in d.items()))
def test_wrappers_refuse_before_the_library(fm3d, monkeypatch, method, bad):
    def no_lib():
        raise AssertionError("the library was loaded for a call")

    pipe = fm3d.Pipeline(NoLibrary())
    monkeypatch.setattr(fm3d, "lib", no_lib)
    kw = dict(max_px=1.0)
    kw.update(bad)
    with pytest.raises(fm3d.Fm3dError) as e:
        getattr(pipe, method)(**kw)
    assert e.value.code == fm3d.ERR_INVALID


def test_wrapper_options(fm3d):
    o = fm3d.Pipeline._verify_opts(2.5, 77, -1, 3, True, 0.25)
    assert (o.hypotheses, o.refineIters, o.maxPx, o.seed, o.poseFromModel, o.reserved, o.baseline) == \
        (77, 3, 2.5, 2 ** 64 - 1, 1, 0, 0.25)
    assert fm3d.Pipeline._verify_opts(1.0, 1, 0, 0, False, 1.0).poseFromModel == 0


def test_pose_from_epipolar_still_equals_restatement(fm3d, synth, orc):
    """the move of the candidates and of the per-pair vote into fm3d_epi8.h changes no bit: the
    reference case's model on its inliers, on every match (wrong pairs vote too) and on none"""
    case = ref.reference_case(synth, orc)
    r, x1, x2 = case["ref"], case["x1"], case["x2"]
    base = float(np.linalg.norm(case["pair"].g12[:3, 3]))
    assert r["best"] >= 0
    for sel in (r["mask"], np.ones(len(x1), dtype=bool), np.zeros(len(x1), dtype=bool)):
        g, votes, ok = fm3d.pose_from_epipolar(r["E"], x1[sel], x2[sel], base)
        gr, vr = ref.pose(orc, r["E"], x1[sel], x2[sel], base)
        assert ok and np.array_equal(votes, vr) and g.tobytes() == gr.tobytes()
    assert votes.sum() == 0
    # every other valid hypothesis of the run: other singular vectors, other signs
    models, counts = r["models"], r["counts"]
    for h in np.nonzero(counts >= 0)[0][:40]:
        g, votes, ok = fm3d.pose_from_epipolar(models[h], x1[:300], x2[:300], 1.0)
        gr, vr = ref.pose(orc, models[h], x1[:300], x2[:300], 1.0)
        assert ok and np.array_equal(votes, vr) and g.tobytes() == gr.tobytes()
    g, votes, ok = fm3d.pose_from_epipolar(np.zeros((3, 3)), x1[:8], x2[:8], 1.0)
    assert not ok
