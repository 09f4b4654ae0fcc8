"""bench.py --dump-outputs (CPU only: the writer is given host tensors, no launch).

The files must be float32 / float64, stay under 64 MB in all, hold the same elements on every run with
the same arguments, and carry int64 columns exactly (float64 alone cannot: the hi32 / lo32 halves do).
"""
import importlib.util
import os

import numpy as np
import pytest
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def bench():
    spec = importlib.util.spec_from_file_location("bench_under_test", os.path.join(REPO, "bench.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)  # module level: imports and constants only
    return mod


def _load(d):
    return {f[:-4]: np.load(os.path.join(d, f)) for f in sorted(os.listdir(d))}


def test_sample_positions_fixed_sorted_with_both_ends(bench):
    a = bench.sample_positions(1_000_003, 1000, 7)
    assert np.array_equal(a, bench.sample_positions(1_000_003, 1000, 7))
    assert a[0] == 0 and a[-1] == 1_000_002 and a.size <= 1000
    assert np.all(np.diff(a) > 0)
    assert not np.array_equal(a, bench.sample_positions(1_000_003, 1000, 8))


def test_small_arrays_whole_and_int64_exact(bench, tmp_path):
    rng = np.random.default_rng(3)
    v64 = rng.integers(-2**63, 2**63 - 1, size=1001, dtype=np.int64, endpoint=True)
    v64[:3] = (-2**63, 2**63 - 1, -1)
    f32 = rng.standard_normal(17).astype(np.float32)
    i32 = rng.integers(-2**31, 2**31 - 1, size=33, dtype=np.int32)
    u8 = rng.integers(0, 256, size=50, dtype=np.uint8)
    arrays = [("a_values", torch.from_numpy(v64)), ("b_values", torch.from_numpy(f32)),
              ("c_values", torch.from_numpy(i32)), ("d_bytes", torch.from_numpy(u8))]
    bench.dump_outputs(str(tmp_path), arrays)
    got = _load(tmp_path)
    assert sorted(got) == ["a_values", "a_values_hi32", "a_values_lo32", "b_values", "c_values", "d_bytes"]
    assert got["b_values"].dtype == np.float32 and np.array_equal(got["b_values"], f32)
    for k in ("a_values", "a_values_hi32", "a_values_lo32", "c_values", "d_bytes"):
        assert got[k].dtype == np.float64
    assert np.array_equal(got["c_values"], i32) and np.array_equal(got["d_bytes"], u8)
    back = (got["a_values_hi32"].astype(np.int64) << 32) | got["a_values_lo32"].astype(np.int64)
    assert np.array_equal(back, v64)
    assert np.array_equal(got["a_values"], v64.astype(np.float64))


def test_long_arrays_sampled_within_budget_and_repeatable(bench, tmp_path, monkeypatch):
    monkeypatch.setattr(bench, "DUMP_BUDGET", 80_000)  # 10,000 float64 elements over 4 files
    v64 = np.arange(100_000, dtype=np.int64) * 3 - 7
    f64 = np.arange(50_000, dtype=np.float64) / 3
    arrays = [("a_values", torch.from_numpy(v64)), ("b_values", torch.from_numpy(f64))]
    d1, d2 = tmp_path / "one", tmp_path / "two"
    bench.dump_outputs(str(d1), arrays)
    bench.dump_outputs(str(d2), arrays)
    one, two = _load(d1), _load(d2)
    assert sum(a.nbytes for a in one.values()) <= 80_000
    for k in one:
        assert np.array_equal(one[k], two[k]), k
    pos = bench.sample_positions(100_000, 2500, bench.DUMP_SEED)
    assert np.array_equal(one["a_values"], v64[pos].astype(np.float64))
    assert one["a_values"][0] == -7 and one["a_values"][-1] == 99_999 * 3 - 7
    assert np.array_equal(one["b_values"], f64[bench.sample_positions(50_000, 2500, bench.DUMP_SEED + 1)])


def test_default_budget_is_under_64_mb(bench):
    assert bench.DUMP_BUDGET <= 64_000_000


def test_command_line_has_full_and_dump_outputs():
    import subprocess
    import sys
    out = subprocess.run([sys.executable, os.path.join(REPO, "bench.py"), "--help"], capture_output=True, text=True)
    assert out.returncode == 0, out.stderr
    assert "--full" in out.stdout and "--dump-outputs DIR" in out.stdout


def test_ranks_above_zero_write_their_own_files(bench, tmp_path):
    bench.dump_outputs(str(tmp_path), [("x", torch.arange(4, dtype=torch.int32))], rank=1, world=2)
    assert sorted(os.listdir(tmp_path)) == ["x.rank1.npy"]
