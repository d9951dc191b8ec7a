"""The verified runs as submit / wait (DESIGN.md §3.1d "Submit / wait") without a GPU: the four exports,
the null-argument rules that need no device, and the Python wrappers' checks, which run before the
library is called."""
import ctypes
import math

import numpy as np
import pytest

NAMES = ("fm3d_pipeline_submit_verified", "fm3d_pipeline_wait_verified", "fm3d_pipeline_submit_dlt_verified",
         "fm3d_pipeline_wait_dlt_verified")


def test_exports_listed(fm3d):
    for n in NAMES:
        assert n in fm3d.EXPORTS and hasattr(fm3d.lib(), n)
        assert getattr(fm3d.lib(), n).argtypes is not None


def test_null_context_options_or_report(fm3d):
    L = fm3d.lib()
    o, rep, st, n = fm3d.VerifyOpts(64, 0, 1.0, 0, 0, 0, 1.0), fm3d.VerifyReport(), fm3d.PipelineStats(), ctypes.c_int(7)
    d = np.zeros((8, 128), dtype=np.uint8)
    k = np.zeros((8, 2), dtype=np.float32)
    dp, kp = ctypes.c_void_p(d.ctypes.data), ctypes.c_void_p(k.ctypes.data)
    assert L.fm3d_pipeline_submit_verified(None, ctypes.byref(o), dp, 8, dp, 8, 128, fm3d.DESC_U8, kp, kp, None, None,
                                           0, 0) == fm3d.ERR_INVALID
    assert L.fm3d_pipeline_submit_verified(None, None, None, 0, None, 0, 0, 0, None, None, None, None, 0,
                                           0) == fm3d.ERR_INVALID
    assert L.fm3d_pipeline_submit_dlt_verified(None, ctypes.byref(o)) == fm3d.ERR_INVALID
    assert L.fm3d_pipeline_submit_dlt_verified(None, None) == fm3d.ERR_INVALID
    assert L.fm3d_pipeline_wait_verified(None, None, 0, ctypes.byref(n), ctypes.byref(st),
                                         ctypes.byref(rep)) == fm3d.ERR_INVALID
    assert L.fm3d_pipeline_wait_verified(None, None, 0, None, None, None) == fm3d.ERR_INVALID
    assert L.fm3d_pipeline_wait_dlt_verified(None, ctypes.byref(n), ctypes.byref(st), ctypes.byref(rep)) == fm3d.ERR_INVALID
    assert L.fm3d_pipeline_wait_dlt_verified(None, None, None, None) == fm3d.ERR_INVALID
    assert n.value == 7


class NoLibrary:
    """a context whose use would be a call into the library"""
    handle = None

    def check(self, code):
        raise AssertionError("the library was called")


BAD = [dict(max_px=0.0), dict(max_px=-1.0), dict(max_px=math.nan), dict(max_px=math.inf), dict(hypotheses=0),
       dict(hypotheses=-5), dict(refine=-1), dict(refine=17)]


@pytest.mark.parametrize("method", ["submit_verified", "submit_dlt_verified"])
@pytest.mark.parametrize("bad", BAD, ids=lambda d: ",".join(f"{k}={v}" for k, v in d.items()))
def test_wrappers_refuse_before_the_library(fm3d, monkeypatch, method, bad):
    def no_lib():
        raise AssertionError("the library was loaded for a call")

    pipe = fm3d.Pipeline(NoLibrary())
    monkeypatch.setattr(fm3d, "lib", no_lib)
    kw = dict(max_px=1.0)
    kw.update(bad)
    if method == "submit_verified":
        d, k, im = np.zeros((8, 128), dtype=np.uint8), np.zeros((8, 2), dtype=np.float32), np.zeros((8, 8), dtype=np.uint8)
        kw.update(desc_a=d, desc_b=d, kp1=k, kp2=k, img1=im, img2=im)
    with pytest.raises(fm3d.Fm3dError) as e:
        getattr(pipe, method)(**kw)
    assert e.value.code == fm3d.ERR_INVALID


def test_wrappers_are_filter_mode(fm3d, monkeypatch):
    """the submit wrappers take no pose option and always pass poseFromModel = 0"""
    seen = []

    class Lib:
        def fm3d_pipeline_submit_dlt_verified(self, handle, opts):
            o = opts._obj
            seen.append((o.hypotheses, o.refineIters, o.maxPx, o.seed, o.poseFromModel, o.reserved))
            return fm3d.FM3D_OK

    class Ctx:
        handle = None

        def check(self, code):
            assert code == fm3d.FM3D_OK

    monkeypatch.setattr(fm3d, "lib", lambda: Lib())
    fm3d.Pipeline(Ctx()).submit_dlt_verified(2.5, hypotheses=77, seed=-1, refine=3)
    assert seen == [(77, 3, 2.5, 2 ** 64 - 1, 0, 0)]
    with pytest.raises(TypeError):
        fm3d.Pipeline(Ctx()).submit_dlt_verified(1.0, pose_from_model=True)
