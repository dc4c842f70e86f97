"""bench.py's command line and its --dump-outputs writer (no GPU needed)."""
import numpy as np
import torch

import bench


def test_plain_run_is_the_default_and_full_is_opt_in():
    a = bench.parse_args(["--gpus", "1", "--steps", "7", "--warmup", "2"])
    assert (a.full, a.dump_outputs, a.steps, a.warmup) == (False, None, 7, 2)
    b = bench.parse_args(["--full", "--dump-outputs", "out"])
    assert (b.full, b.dump_outputs) == (True, "out")


def test_dump_outputs_writes_float32_and_samples_what_exceeds_the_budget(tmp_path, monkeypatch):
    monkeypatch.setattr(bench, "DUMP_BUDGET_BYTES", 2 * 4096)            # 4096 bytes per array
    small = torch.arange(12, dtype=torch.float16).reshape(3, 4)
    big = torch.randn(5000, dtype=torch.float32)
    bench.dump_outputs(str(tmp_path), {"small": small, "big": big})
    s, b = np.load(tmp_path / "small.npy"), np.load(tmp_path / "big.npy")
    assert s.dtype == np.float32 and s.shape == (3, 4) and np.array_equal(s, small.float().numpy())
    assert b.dtype == np.float32 and b.shape == (1024,) and np.isin(b, big.numpy()).all()
    bench.dump_outputs(str(tmp_path / "again"), {"small": small, "big": big})
    assert np.array_equal(np.load(tmp_path / "again" / "big.npy"), b)             # the same fixed sample every run
    bench.dump_outputs(str(tmp_path), {"d": torch.ones(2, dtype=torch.float64)}, rank=1)
    assert np.load(tmp_path / "d_rank1.npy").dtype == np.float64
