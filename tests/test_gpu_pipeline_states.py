"""Which staged-pipeline call may follow which: one literal
table of situations x calls through the Python Pipeline.  A cell is ACCEPTED or the Fm3dError's code
and message; the messages are API.  The table was taken from the library before the pair state became
one enumeration and must not change with it.

A refused call has no side effect: after each one in a pending row the pending work is waited for with
its own wait, and its counts, matches, points and records (or NCC scores) equal, bit for bit, the same
work run undisturbed on a second context.

The pair is synth.make_frame_pair(300, width=160, height=120, seed=5): 270 matches and 208 inliers at
nndrEpsilon 0.55 ("sift") by the oracle; pixelsRay = 8, pyramids = 1, 64 verification hypotheses."""
import ctypes

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

INV = -1  # FM3D_ERR_INVALID
ACCEPTED = "accepted"
UPLOAD = (INV, "fm3d_pipeline_upload not called")
PENDING = (INV, "a submitted frame pair is pending: fm3d_pipeline_wait first")
NO_FULL = (INV, "no frame pair submitted (fm3d_pipeline_submit)")
NO_DLT = (INV, "no front half submitted (fm3d_pipeline_submit_dlt)")
NO_NCC = (INV, "no NCC scoring submitted (fm3d_pipeline_submit_ncc)")
IS_DLT = (INV, "a front half is pending: fm3d_pipeline_wait_dlt")
IS_NCC = (INV, "an NCC scoring is pending: fm3d_pipeline_wait_ncc")
LINK_PENDING = (INV, "a submitted frame pair is pending")
SILENT = (INV, "")  # the downloads refuse an unstaged context without a message

COLS = ("upload", "run", "submit", "wait", "link", "run_dlt", "submit_dlt", "submit_dlt_pair", "wait_dlt",
        "run_verified", "run_dlt_verified", "submit_ncc", "wait_ncc", "run_ncc", "ncc_results", "dlt_results")
A = ACCEPTED
TABLE = {
    # fresh: nothing staged
    "fresh": (A, UPLOAD, A, NO_FULL, A, UPLOAD, UPLOAD, A, NO_DLT,
              UPLOAD, UPLOAD, UPLOAD, NO_NCC, UPLOAD, SILENT, SILENT),
    # staged by upload, nothing queued
    "idle": (A, A, A, NO_FULL, A, A, A, A, NO_DLT,
             A, A, A, NO_NCC, A, A, A),
    # the full path queued by submit
    "full": (PENDING, PENDING, PENDING, A, LINK_PENDING, PENDING, PENDING, PENDING, NO_DLT,
             PENDING, PENDING, PENDING, NO_NCC, PENDING, PENDING, PENDING),
    # a link member's front half queued by submit; its leader has not submitted
    "member": (PENDING, PENDING, PENDING, A, LINK_PENDING, PENDING, PENDING, PENDING, NO_DLT,
               PENDING, PENDING, PENDING, NO_NCC, PENDING, PENDING, PENDING),
    # the DLT front half queued by submit_dlt
    "dlt": (PENDING, PENDING, PENDING, IS_DLT, LINK_PENDING, PENDING, PENDING, PENDING, A,
            PENDING, PENDING, PENDING, NO_NCC, PENDING, PENDING, PENDING),
    # ... by submit_dlt_pair on non-integer float rows of 64 columns: the u8 matcher ran on speculation
    # and wait_dlt re-runs the front half on the float rows
    "dlt_spec": (PENDING, PENDING, PENDING, IS_DLT, LINK_PENDING, PENDING, PENDING, PENDING, A,
                 PENDING, PENDING, PENDING, NO_NCC, PENDING, PENDING, PENDING),
    # the front half and the NCC scoring queued by submit_ncc
    "ncc": (PENDING, PENDING, PENDING, IS_NCC, LINK_PENDING, PENDING, PENDING, PENDING, NO_DLT,
            PENDING, PENDING, PENDING, A, PENDING, PENDING, PENDING),
}
PENDING_ROWS = ("full", "member", "dlt", "dlt_spec", "ncc")
NCC_H = 16  # submit_ncc's default 4 x 4 hypotheses


@pytest.fixture(scope="module")
def pairs(synth):
    return {k: synth.make_frame_pair(300, width=160, height=120, seed=5, desc=k) for k in ("sift", "orb")}


def float_rows(kind, d):
    """64 float columns, none an integer, of a pair's descriptors (the speculative u8 path's inputs)"""
    cols = d[:, :64] if kind == "sift" else np.unpackbits(d[:, :8], axis=1)
    return cols.astype(np.float32) + np.float32(0.25)


def make_pipe(fm3d, pair, kind):
    s = fm3d.Settings.default()
    s.set_camera(pair.cam)
    s.pixelsRay, s.pyramids = 8, 1
    s.nndrEpsilon = 0.55 if kind == "sift" else 0.8
    c = fm3d.Context(s, device=0)
    fm3d.SingleCameraTriangulator(c).set_g12(pair.g12)
    return fm3d.Pipeline(c)


class Situation:
    """a context brought into one row's situation (and the leader of the member row)"""

    def __init__(self, fm3d, pair, kind, row):
        self.fm3d, self.pair, self.kind, self.row = fm3d, pair, kind, row
        self.binary = kind == "orb"
        self.pipes = [make_pipe(fm3d, pair, kind)]
        p, fp = self.pipes[0], pair
        full = (fp.desc1, fp.desc2, fp.kp1, fp.kp2, fp.img1, fp.img2)
        if row in ("idle", "dlt", "ncc"):
            p.upload(*full, binary=self.binary)
        if row == "member":
            self.pipes.append(make_pipe(fm3d, pair, kind))
            p.link(self.pipes[1])
        if row in ("full", "member"):
            p.submit(*full, binary=self.binary)
        elif row == "dlt":
            p.submit_dlt()
        elif row == "dlt_spec":
            p.submit_dlt_pair(float_rows(kind, fp.desc1), float_rows(kind, fp.desc2), fp.kp1, fp.kp2)
        elif row == "ncc":
            p.submit_ncc()

    def call(self, col):
        p, fp = self.pipes[0], self.pair
        full = (fp.desc1, fp.desc2, fp.kp1, fp.kp2, fp.img1, fp.img2)
        if col in ("upload", "submit"):
            return getattr(p, col)(*full, binary=self.binary)
        if col == "submit_dlt_pair":
            return p.submit_dlt_pair(fp.desc1, fp.desc2, fp.kp1, fp.kp2, binary=self.binary)
        if col == "link":
            self.pipes.append(make_pipe(self.fm3d, fp, self.kind))
            return p.link(self.pipes[-1])
        if col in ("run_verified", "run_dlt_verified"):
            return getattr(p, col)(2.0, hypotheses=64)
        if col == "ncc_results":
            return p.ncc_results(0, NCC_H)
        if col == "dlt_results":
            return p.dlt_results(0, 0)
        return getattr(p, col)()

    def finish(self):
        """the pending work through its own wait -> everything it computed, as comparable values"""
        p = self.pipes[0]
        if self.row in ("full", "member"):
            rec, st = p.wait()
            out = [st["kept"], rec.tobytes()]
        elif self.row == "ncc":
            P, st = p.wait_ncc()
            out = [P] + [a.tobytes() for a in p.ncc_results(P, NCC_H)]
        else:
            P, st = p.wait_dlt()
            out = [P]
        out += [st["queries"], st["trains"], st["matches"], st["inliers"]]
        return out + [a.tobytes() for a in p.dlt_results(st["matches"], st["inliers"])]

    def close(self):
        for p in self.pipes:
            p.ctx.close()


_UNDISTURBED = {}


def undisturbed(fm3d, pair, kind, row):
    """a pending row's work with nothing between its submit and its wait (computed once per row)"""
    if (kind, row) not in _UNDISTURBED:
        s = Situation(fm3d, pair, kind, row)
        try:
            out = s.finish()
        finally:
            s.close()
        assert out[-5] > 0 and out[-4] > 0, "the reference run itself needs matches and inliers"
        _UNDISTURBED[kind, row] = out
    return _UNDISTURBED[kind, row]


@pytest.mark.parametrize("row", list(TABLE))
@pytest.mark.parametrize("kind", ["sift", "orb"])
def test_state_table(fm3d, pairs, kind, row):
    pair = pairs[kind]
    wrong = []
    for col, want in zip(COLS, TABLE[row]):
        s = Situation(fm3d, pair, kind, row)
        try:
            try:
                s.call(col)
                got = ACCEPTED
            except fm3d.Fm3dError as e:
                got = (e.code, str(e).split(": ", 1)[1])
            if got != want:
                wrong.append((col, got, want))
            if got != ACCEPTED and row in PENDING_ROWS and s.finish() != undisturbed(fm3d, pair, kind, row):
                wrong.append((col, "the refused call changed the pending pair's results"))
        finally:
            s.close()
    print(row, kind, wrong)
    assert not wrong


def test_reference_counts(fm3d, orc, pairs):
    """the shapes are not empty: the oracle's 270 matches and 208 inliers on the sift pair"""
    pair = pairs["sift"]
    out = undisturbed(fm3d, pair, "sift", "dlt")
    q, t, _ = orc.match_nndr(pair.desc1, pair.desc2, orc.U8, 0.55)
    s = fm3d.Settings.default()
    pts, _ = orc.triangulate(pair.cam, pair.g12, s.zThresholdMin, s.zThresholdMax, pair.kp1, pair.kp2, q, t)
    assert (len(q), len(pts)) == (270, 208) and out[-5:-3] == [270, 208]


def test_failed_submit_leaves_idle(fm3d, pairs):
    """A submit on a context that never got images: the LM refuses after the front half is queued.
    The error is the LM's, nothing is pending afterwards and the context is as usable as a fresh one."""
    pair = pairs["sift"]
    p, fresh = make_pipe(fm3d, pair, "sift"), make_pipe(fm3d, pair, "sift")
    vp = lambda a: ctypes.c_void_p(a.ctypes.data)
    try:
        rc = fm3d.lib().fm3d_pipeline_submit(p.ctx.handle, vp(pair.desc1), 300, vp(pair.desc2), 300, 128, 1,
                                             vp(pair.kp1), vp(pair.kp2), None, None, 0, 0, 0)
        assert rc == INV
        assert fm3d.lib().fm3d_last_error(p.ctx.handle) == b"fm3d_set_images (NormalOptimizer::setImages) not called"
        got = []
        for q in (p, fresh):  # idle: the upload is accepted (a pending pair would refuse it)
            q.upload(pair.desc1, pair.desc2, pair.kp1, pair.kp2, None, None)
            P, st = q.run_dlt()
            got.append([P, st["matches"], st["inliers"]] + [a.tobytes() for a in q.dlt_results(st["matches"], P)])
        assert got[0] == got[1] and got[0][:3] == [208, 270, 208]
        for col, want in (("wait", NO_FULL), ("wait_dlt", NO_DLT), ("wait_ncc", NO_NCC)):
            with pytest.raises(fm3d.Fm3dError) as e:
                getattr(p, col)()
            assert (e.value.code, str(e.value).split(": ", 1)[1]) == want
    finally:
        p.ctx.close()
        fresh.ctx.close()
