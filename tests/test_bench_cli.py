"""CPU tests of bench.py's command line: --full is off by default, --steps
sets the timed steps, and --dump-outputs writes float32 / float64 arrays of
at most 64 MB in all, finite throughout (non-finite fields masked), a fixed
sample of the taxa when the results are larger."""

import sys

import numpy as np
import pytest

import bench


def _parse(monkeypatch, *argv):
    monkeypatch.setattr(sys, "argv", ["bench.py", *argv])
    return bench.parse()


def test_plain_run_is_the_default(monkeypatch):
    a = _parse(monkeypatch, "--gpus", "1", "--steps", "7", "--warmup", "2")
    assert (a.gpus, a.steps, a.warmup) == (1, 7, 2)
    assert a.full is False and a.dump_outputs is None
    a = _parse(monkeypatch, "--full", "--dump-outputs", "d")
    assert a.full is True and a.dump_outputs == "d"
    assert (a.steps, a.warmup) == (20, 3)


def test_steps_must_be_positive(monkeypatch):
    with pytest.raises(SystemExit):
        _parse(monkeypatch, "--steps", "0")


def _results(T, seed=5):
    rng = np.random.default_rng(seed)
    out = rng.random((T, 80))
    out[::7, 3] = np.nan
    out[1, 5], out[2, 6] = np.inf, -np.inf
    return out, rng.random((T, 3, 30)).astype(np.float32), (rng.random(T) < 0.01).astype(np.int32)


def _load(d):
    return {p.stem: np.load(p) for p in d.iterdir()}


def _restore(values, code):
    """The array a dump's finite values and non-finite codes stand for."""
    fill = np.array([0, np.nan, np.inf, -np.inf])[code.astype(np.int64)]
    return np.where(code == 0, values, fill.astype(values.dtype))


def test_dump_outputs_whole(tmp_path):
    out, pred, st = _results(333)
    bench.dump_outputs(tmp_path / "a" / "b", out, pred, st)
    got = _load(tmp_path / "a" / "b")
    assert sorted(got) == ["out", "out_nonfinite", "pred", "pred_nonfinite", "status"]
    assert got["out"].dtype == np.float64 and all(v.dtype == np.float32 for k, v in got.items() if k != "out")
    assert all(np.isfinite(v).all() for v in got.values())
    assert np.isnan(out).any() and (got["out"][np.isnan(out)] == 0).all()
    assert got["out_nonfinite"][1, 5] == 2 and got["out_nonfinite"][2, 6] == 3 and got["out_nonfinite"][0, 3] == 1
    assert not got["pred_nonfinite"].any()
    np.testing.assert_array_equal(_restore(got["out"], got["out_nonfinite"]), out)
    np.testing.assert_array_equal(got["pred"], pred)
    np.testing.assert_array_equal(got["status"], st)
    assert np.isnan(out).any()  # the caller's array is left as it was


def test_dump_outputs_samples_large_results(tmp_path, monkeypatch):
    """Above the size limit the same seeded rows of every array are written,
    the same from call to call."""
    T = 1000
    out, pred, st = _results(T)
    monkeypatch.setattr(bench, "DUMP_MAX_BYTES", 200_000)
    bench.dump_outputs(tmp_path / "a", out, pred, st)
    bench.dump_outputs(tmp_path / "b", out, pred, st)
    a, b = _load(tmp_path / "a"), _load(tmp_path / "b")
    assert sorted(a) == ["out", "out_nonfinite", "pred", "pred_nonfinite", "sample_rows", "status"]
    assert all(np.isfinite(v).all() for v in a.values())
    assert sum(v.nbytes for v in a.values()) <= 200_000
    rows = a["sample_rows"].astype(np.int64)
    assert 0 < rows.size < T and (np.diff(rows) > 0).all() and rows[-1] < T
    np.testing.assert_array_equal(_restore(a["out"], a["out_nonfinite"]), out[rows])
    np.testing.assert_array_equal(a["pred"], pred[rows])
    np.testing.assert_array_equal(a["status"], st[rows])
    for k in a:
        np.testing.assert_array_equal(a[k], b[k])


def test_dump_limit_is_under_64_mb():
    assert bench.DUMP_MAX_BYTES + 6 * 4096 <= 64_000_000  # six files and their headers
