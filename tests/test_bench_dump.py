"""bench.py --dump-outputs (CPU side): the files are float64, stay within the budget, a large output is a sample at the same
seeded positions in every run, and the arguments that cannot be honoured are refused before any GPU work."""
import os
import subprocess
import sys

import numpy as np

import bench

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _total_bytes(d):
    return sum(os.path.getsize(os.path.join(d, f)) for f in os.listdir(d))


def test_small_outputs_are_written_whole(tmp_path):
    rng = np.random.default_rng(3)
    lhs = rng.standard_normal(500) + 1j * rng.standard_normal(500)
    norms = rng.random(8)
    res = bench.dump_outputs(str(tmp_path), {"lhs": lhs, "norms": norms}, 0, 1)
    assert sorted(os.listdir(tmp_path)) == ["lhs.npy", "norms.npy"]
    got = np.load(tmp_path / "lhs.npy")
    assert got.dtype == np.float64 and got.shape == (500, 2)
    assert np.array_equal(got[:, 0] + 1j * got[:, 1], lhs)
    assert np.array_equal(np.load(tmp_path / "norms.npy"), norms)
    assert "sample" not in res["outputs"]["lhs"]


def test_large_outputs_are_a_fixed_sample_within_the_budget(tmp_path, monkeypatch):
    monkeypatch.setattr(bench, "DUMP_BUDGET_BYTES", 1 << 20)
    rng = np.random.default_rng(5)
    lhs = rng.standard_normal(1 << 18) + 1j * rng.standard_normal(1 << 18)       # 4 MB of complex128
    runs = []
    for k in range(2):
        d = tmp_path / ("run%d" % k)
        res = bench.dump_outputs(str(d), {"lhs": lhs}, 0, 1)
        assert _total_bytes(d) <= 1 << 20
        vals, idx = np.load(d / "lhs.npy"), np.load(d / "lhs_index.npy")
        assert vals.dtype == np.float64 and idx.dtype == np.float64
        i = idx.astype(np.int64)
        assert np.all(np.diff(i) > 0) and i[0] >= 0 and i[-1] < lhs.size
        assert np.array_equal(vals[:, 0] + 1j * vals[:, 1], lhs[i])
        assert res["outputs"]["lhs"]["sample"] == i.size > (1 << 20) // 32
        runs.append(i)
    assert np.array_equal(runs[0], runs[1])


def test_ranks_share_the_budget_and_name_their_files(tmp_path, monkeypatch):
    monkeypatch.setattr(bench, "DUMP_BUDGET_BYTES", 1 << 20)
    lhs = np.ones(1 << 18, dtype=np.complex128)
    for r in range(4):
        bench.dump_outputs(str(tmp_path), {"lhs": lhs}, r, 4)
    assert _total_bytes(tmp_path) <= 1 << 20
    assert sorted(os.listdir(tmp_path)) == sorted(["lhs_rank%d.npy" % r for r in range(4)] + ["lhs_rank%d_index.npy" % r for r in range(4)])


def test_arguments_that_cannot_be_honoured_are_refused(tmp_path):
    for extra in (["--steps", "0"], ["--workload", "kcycle", "--dump-outputs", str(tmp_path)]):
        out = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1"] + extra, capture_output=True, text=True, timeout=120)
        assert out.returncode == 2, out.stdout + out.stderr
        assert "error:" in out.stderr
    assert os.listdir(tmp_path) == []
