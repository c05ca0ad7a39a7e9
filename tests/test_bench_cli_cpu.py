"""bench.py's command line and its --dump-outputs writer (no GPU): a plain run asks for no secondary
measurement, --full switches them on, and a dumped array is float32, capped, and the same sample every time."""
import os
import sys

import numpy as np
import pytest
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if REPO not in sys.path:
    sys.path.insert(0, REPO)

import bench  # noqa: E402


def test_plain_run_is_lean_and_full_is_opt_in():
    a = bench.parse(["--gpus", "1", "--steps", "7", "--warmup", "2"])
    assert (a.steps, a.warmup, a.full, a.dump_outputs) == (7, 2, False, None)
    assert bench.parse(["--full"]).full
    f = bench.parse(["--full", "--no-probe", "--no-cpu-baseline", "--dump-outputs", "d"])
    assert f.full and f.no_probe and f.no_cpu_baseline and f.dump_outputs == "d"


@pytest.mark.parametrize("argv", [["--classes-out", "c.json"], ["--full", "--no-probe", "--classes-out", "c.json"],
                                  ["--steps", "0"], ["--warmup", "-1"]])
def test_arguments_that_cannot_be_honoured_are_errors(argv):
    with pytest.raises(SystemExit):
        bench.parse(argv)


def test_dump_outputs_float32_capped_and_repeatable(tmp_path, monkeypatch):
    monkeypatch.setattr(bench, "DUMP_MAX_ELEMS", 1000)
    big = np.arange(5000, dtype=np.float64).reshape(50, 100)
    arrays = {"small": torch.arange(12, dtype=torch.float16).reshape(3, 4), "big": big}
    bench.dump_outputs(str(tmp_path / "a"), arrays)
    bench.dump_outputs(str(tmp_path / "b"), arrays)
    small = np.load(tmp_path / "a" / "small.npy")
    assert small.dtype == np.float32 and small.shape == (3, 4) and np.array_equal(small.ravel(), np.arange(12))
    got, again = np.load(tmp_path / "a" / "big.npy"), np.load(tmp_path / "b" / "big.npy")
    assert got.dtype == np.float32 and got.shape == (1000,) and np.array_equal(got, again)
    # a sample of the flattened array at distinct, increasing positions (the values are their own indices)
    assert np.all(np.diff(got) > 0) and got[0] >= 0 and got[-1] < 5000
    assert sorted(os.listdir(tmp_path / "a")) == ["big.npy", "small.npy"]
