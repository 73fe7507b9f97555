"""bench.py's command line: a plain run is set-up, warm-up, the timed steps and the result line;
--full adds the secondary measurements; --dump-outputs writes the last timed step's outputs."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import bench  # noqa: E402

CONTRACT = ("metric", "value", "unit", "higher_is_better", "dtype", "ms_per_step")
FULL_ONLY = ("cpu_baseline", "per_frame_dropin", "config4_train", "config5_cross", "split_bf16", "one_in_flight",
             "deform_ms_per_step", "render_work_per_frame", "render_mfma")


def test_full_and_dump_are_off_by_default(monkeypatch):
    monkeypatch.setattr(sys, "argv", ["bench.py", "--gpus", "1", "--steps", "7", "--warmup", "2"])
    a = bench._args()
    assert a.steps == 7 and a.warmup == 2 and not a.full and a.dump_outputs is None
    monkeypatch.setattr(sys, "argv", ["bench.py", "--full", "--dump-outputs", "somewhere"])
    a = bench._args()
    assert a.full and a.dump_outputs == "somewhere"


def test_dump_outputs_float32_and_fixed_sample(tmp_path):
    """Small arrays are written whole, large ones as the same sorted sample on every call, all float32."""
    import torch
    n = bench.DUMP_MAX_ELEMS + 12348
    named = {"small": torch.arange(10, dtype=torch.int32).reshape(2, 5),
             "big": torch.arange(n, dtype=torch.float64).reshape(-1, 5)}
    for d in ("a", "b"):
        bench.dump_outputs(str(tmp_path / d), named)
    small, big = np.load(tmp_path / "a" / "small.npy"), np.load(tmp_path / "a" / "big.npy")
    assert small.dtype == np.float32 and np.array_equal(small, np.arange(10).reshape(2, 5))
    assert big.dtype == np.float32 and big.shape == (bench.DUMP_MAX_ELEMS,)
    assert np.all(np.diff(big) >= 0) and big[0] >= 0 and big[-1] < n  # values are their own indices
    assert len(np.unique(big)) > 0.5 * bench.DUMP_MAX_ELEMS  # spread over the array, not one corner
    assert np.array_equal(big, np.load(tmp_path / "b" / "big.npy"))
    assert sorted(os.listdir(tmp_path / "a")) == ["big.npy", "small.npy"]


@pytest.mark.gpu
def test_plain_run_times_the_steps_and_dumps_its_outputs(tmp_path):
    """A plain run of two steps: the contract keys, none of the --full measurements, and the last
    step's outputs of the avatar pipeline as float32 files of at most 64 MB in all."""
    out = tmp_path / "dump"
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "2", "--warmup", "1",
                        "--dump-outputs", str(out)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1
    d = json.loads(lines[0])
    assert all(k in d for k in CONTRACT) and d["steps"] == 2 and d["warmup"] == 1
    assert d["ms_per_step"] > 0 and abs(d["value"] - 32 * 1e3 / d["ms_per_step"]) <= 0.01 * d["value"]
    assert not any(k in d for k in FULL_ONLY)
    files = sorted(os.listdir(out))
    assert files == ["color.npy", "invdepth.npy", "radii.npy", "rotation.npy", "scaling.npy", "xyz.npy"]
    arrs = {f: np.load(out / f) for f in files}
    assert all(a.dtype == np.float32 and np.isfinite(a).all() for a in arrs.values())
    assert sum(os.path.getsize(out / f) for f in files) <= 64e6
    assert np.count_nonzero(arrs["color.npy"]) > 0 and np.count_nonzero(arrs["radii.npy"]) > 0
