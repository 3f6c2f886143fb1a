"""bench.py plumbing: --dump-outputs files and the result line's contract."""

import json
import os
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import bench  # noqa: E402


def test_dump_outputs_dtypes_and_names(tmp_path):
    arrays = {
        "scalar": torch.tensor(0.25),
        "half": torch.arange(12, dtype=torch.bfloat16).reshape(4, 3),
        "double": torch.linspace(0, 1, 5, dtype=torch.float64),
    }
    bench.dump_outputs(str(tmp_path / "out"), arrays)
    assert sorted(os.listdir(tmp_path / "out")) == [
        "double.npy", "half.npy", "scalar.npy"]
    half = np.load(tmp_path / "out" / "half.npy")
    assert half.dtype == np.float32 and half.shape == (4, 3)
    assert np.array_equal(half, np.arange(12, dtype=np.float32).reshape(4, 3))
    assert np.load(tmp_path / "out" / "double.npy").dtype == np.float64
    assert float(np.load(tmp_path / "out" / "scalar.npy")) == 0.25


def test_dump_outputs_budget_sample_is_fixed(tmp_path, monkeypatch):
    """An array over its share of the byte budget is cut to the same seeded
    sample of its elements in every run; smaller arrays are kept whole."""
    monkeypatch.setattr(bench, "DUMP_BUDGET_BYTES", 2 * 400)
    big = torch.arange(1000, dtype=torch.float32).reshape(100, 10)
    small = torch.ones(7)
    for d in ("a", "b"):
        bench.dump_outputs(str(tmp_path / d), {"big": big, "small": small})
    a = np.load(tmp_path / "a" / "big.npy")
    b = np.load(tmp_path / "b" / "big.npy")
    assert a.shape == (100,) and np.array_equal(a, b)
    # a sample of big's own elements, in order, without repeats
    assert np.all(np.diff(a) > 0) and a.min() >= 0 and a.max() <= 999
    assert np.load(tmp_path / "a" / "small.npy").shape == (7,)
    total = sum(os.path.getsize(tmp_path / "a" / f)
                for f in os.listdir(tmp_path / "a"))
    assert total <= 2 * 400 + 2 * 128   # payload budget + two .npy headers


@pytest.mark.gpu
@pytest.mark.skipif(not torch.cuda.is_available(), reason="requires GPU")
def test_bench_dump_outputs_and_result_line(tmp_path, monkeypatch, capsys):
    """A small eager run: --steps sets the timed steps, the result line
    carries ms_per_step, and --dump-outputs writes the last step's arrays."""
    n = 3000
    out = tmp_path / "dump"
    monkeypatch.setattr(sys, "argv", [
        "bench.py", "--gpus", "1", "--steps", "2", "--warmup", "1",
        "--nodes", str(n), "--graphs", "off", "--full",
        "--dump-outputs", str(out)])
    bench.main()
    line = [ln for ln in capsys.readouterr().out.splitlines()
            if ln.startswith("{")][-1]
    res = json.loads(line)
    assert res["steps"] == 2 and res["warmup"] == 1
    assert res["metric"] == "train_step_time_ms" and res["unit"] == "ms"
    assert res["higher_is_better"] is False and res["dtype"] == "bf16"
    assert res["ms_per_step"] == res["value"] > 0

    got = {f[:-4]: np.load(out / f) for f in os.listdir(out)}
    assert sorted(got) == ["coord_mse", "grads", "loc_pred", "params",
                           "virtual_loc"]
    for name, a in got.items():
        assert a.dtype == np.float32, name
        assert np.isfinite(a).all(), name
    assert got["loc_pred"].shape == (n, 3)
    assert got["virtual_loc"].shape == (1, 3, 5)
    assert got["params"].shape == got["grads"].shape
    assert float(got["coord_mse"]) == pytest.approx(
        res["config"]["coord_mse"], rel=1e-6)
    assert sum(a.nbytes for a in got.values()) <= bench.DUMP_BUDGET_BYTES
