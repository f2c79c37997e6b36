"""bench.py --dump-outputs on the CPU: dump_outputs writes every array as <name>.npy in
float64, whole while they fit the byte budget; past it each large array keeps the same seeded
sample of its last axis on every call (its indices beside it) and the files stay under the
budget. A plain command line leaves the --full legs off."""
import importlib.util
import os
import sys

import numpy as np
import pytest

from conftest import ROOT


@pytest.fixture(scope="module")
def bench():
    spec = importlib.util.spec_from_file_location("bench_under_test", os.path.join(ROOT, "bench.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def _arrays():
    rng = np.random.default_rng(1)
    return {"track_rec": rng.standard_normal((3, 18, 1019)), "track_len": np.array([1019, 1019, 1000]),
            "track_countinx": np.array([3, 0, 19], dtype=np.int32), "acq_SNR": rng.standard_normal(3)}


def test_dump_whole_when_it_fits(bench, tmp_path):
    arrs = _arrays()
    bench.dump_outputs(str(tmp_path / "d"), arrs)
    assert sorted(os.listdir(tmp_path / "d")) == sorted(k + ".npy" for k in arrs)
    for k, v in arrs.items():
        got = np.load(tmp_path / "d" / (k + ".npy"))
        assert got.dtype == np.float64 and np.array_equal(got, np.asarray(v, dtype=np.float64))


def test_dump_samples_past_the_budget(bench, tmp_path, monkeypatch):
    arrs = _arrays()
    budget = 100_000  # track_rec alone holds 440 208 B
    monkeypatch.setattr(bench, "DUMP_BUDGET", budget)
    bench.dump_outputs(str(tmp_path / "a"), arrs)
    bench.dump_outputs(str(tmp_path / "b"), arrs)
    size = sum(os.path.getsize(tmp_path / "a" / f) for f in os.listdir(tmp_path / "a"))
    assert size <= budget
    cols = np.load(tmp_path / "a" / "track_rec_columns.npy")
    assert np.array_equal(cols, np.load(tmp_path / "b" / "track_rec_columns.npy"))
    idx = cols.astype(np.int64)
    assert len(idx) > 100 and np.all(np.diff(idx) > 0) and idx[-1] < 1019
    got = np.load(tmp_path / "a" / "track_rec.npy")
    assert np.array_equal(got, arrs["track_rec"][..., idx])
    # the small arrays stay whole
    assert np.array_equal(np.load(tmp_path / "a" / "track_len.npy"), arrs["track_len"].astype(np.float64))


def test_plain_command_line_has_the_full_legs_off(bench, monkeypatch):
    monkeypatch.setattr(sys, "argv", ["bench.py", "--gpus", "1", "--steps", "2", "--warmup", "1"])
    a = bench.parse()
    assert not a.full and a.dump_outputs is None and a.steps == 2 and a.warmup == 1
    monkeypatch.setattr(sys, "argv", ["bench.py", "--full", "--dump-outputs", "out"])
    a = bench.parse()
    assert a.full and a.dump_outputs == "out"
