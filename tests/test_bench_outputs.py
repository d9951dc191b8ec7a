"""bench.py's --dump-outputs writer and the --full switch (CPU only: the writer and the argument
parser; the GPU run of it is tests/test_gpu_parity.py::test_bench_plain_run_dumps_last_step)."""
import importlib.util
import os
import sys

import numpy as np
import pytest

from conftest import ROOT


@pytest.fixture(scope="module")
def bench():
    spec = importlib.util.spec_from_file_location("fm3d_bench", os.path.join(ROOT, "bench.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def _args(bench, monkeypatch, *argv):
    monkeypatch.setattr(sys, "argv", ["bench.py", *argv])
    return bench.parse()


def test_full_is_off_by_default(bench, monkeypatch):
    a = _args(bench, monkeypatch, "--gpus", "1", "--steps", "4", "--warmup", "2")
    assert a.full is False and a.dump_outputs == "" and (a.steps, a.warmup) == (4, 2)
    assert _args(bench, monkeypatch, "--full").full is True


def test_dump_outputs_types_and_values(bench, monkeypatch, tmp_path, fm3d):
    rec = np.zeros(5, dtype=fm3d.RECORD)
    rec["queryIdx"] = [3, 5, 2**31 - 1, 0, 7]
    rec["distance"] = np.float32([0.5, 1.25, 3.0, 0.1, 2.0])
    rec["point"] = np.arange(15.0).reshape(5, 3) / 7.0
    rec["normal"][2] = np.nan
    d = tmp_path / "out"
    bench.dump_outputs(_args(bench, monkeypatch, "--dump-outputs", str(d)), bench.record_fields(rec))
    assert sorted(os.listdir(d)) == sorted(n + ".npy" for n in fm3d.RECORD.names)
    for n in fm3d.RECORD.names:
        a = np.load(d / (n + ".npy"))
        assert a.dtype == (np.float32 if rec[n].dtype == np.float32 else np.float64) and a.shape == rec[n].shape
        assert np.array_equal(a, rec[n].astype(a.dtype), equal_nan=True)
    # without the option nothing is written
    bench.dump_outputs(_args(bench, monkeypatch), {"x": np.zeros(3)})
    assert sorted(os.listdir(tmp_path)) == ["out"]


def test_dump_outputs_sample_is_bounded_aligned_and_repeatable(bench, monkeypatch, tmp_path):
    monkeypatch.setattr(bench, "DUMP_LIMIT_BYTES", 4000)
    n = 1001  # 1001 x (8 + 24) B = 32 kB: past the limit
    arrays = {"idx": np.arange(n, dtype=np.int32), "xyz": np.arange(3.0 * n).reshape(n, 3), "few": np.arange(10.0)}
    got = []
    for name in ("a", "b"):
        bench.dump_outputs(_args(bench, monkeypatch, "--dump-outputs", str(tmp_path / name)), arrays)
        got.append({k: np.load(tmp_path / name / (k + ".npy")) for k in arrays})
    a, b = got
    assert sum(v.nbytes for v in a.values()) <= 4000
    assert all(np.array_equal(a[k], b[k]) for k in arrays)  # the same rows on every run
    idx = a["idx"].astype(int)
    assert 0 < len(idx) < n and np.all(np.diff(idx) > 0)  # a sample, in the original order
    assert np.array_equal(a["xyz"], arrays["xyz"][idx])  # arrays of equal length keep the same rows
    assert 0 < len(a["few"]) <= 10 and np.all(np.isin(a["few"], arrays["few"]))
