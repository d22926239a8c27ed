"""bench.py --dump-outputs (no GPU): names, dtypes, the fixed sample of large arrays and the size budget."""
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import bench  # noqa: E402


class _Bank:
    def __init__(self, n):
        self.flat = torch.arange(n, dtype=torch.float32)
        self.grad = -self.flat


def _out():
    g = torch.Generator().manual_seed(0)
    return {"images": torch.randn(8, 3, 512, 512, generator=g).half(), "images_grad": torch.randn(8, 3, 512, 512, generator=g),
            "targets": torch.tensor([0, 1, -1, 1]), "loss_fair": torch.rand(4, generator=g, dtype=torch.float64),
            "targets_by_attr": {"gender": torch.tensor([0, 1, -1, 1])}, "grad_is_finite": True, "N_backward": 3, "note": "not an array"}


def test_dump_outputs_names_dtypes_and_budget(tmp_path):
    bench.dump_outputs(str(tmp_path), _out(), [_Bank(1000), _Bank(5 << 20)])
    files = sorted(os.listdir(tmp_path))
    assert files == sorted(["images.npy", "images_grad.npy", "targets.npy", "loss_fair.npy", "targets_by_attr.gender.npy", "grad_is_finite.npy",
                            "N_backward.npy", "lora0_weights.npy", "lora0_grad.npy", "lora1_weights.npy", "lora1_grad.npy"])
    arr = {f[:-4]: np.load(tmp_path / f) for f in files}
    assert sum(os.path.getsize(tmp_path / f) for f in files) <= 64 * 10 ** 6
    assert all(a.dtype in (np.float32, np.float64) for a in arr.values())
    assert arr["images"].dtype == np.float32 and arr["loss_fair"].dtype == np.float64 and arr["targets"].dtype == np.float64
    assert arr["targets"].tolist() == [0, 1, -1, 1] and float(arr["grad_is_finite"]) == 1.0 and float(arr["N_backward"]) == 3.0
    np.testing.assert_array_equal(arr["lora0_weights"], np.arange(1000, dtype=np.float32))     # small: whole, shape kept
    # large: a sample of the flattened array at sorted, seeded indices -- the same elements every run
    w = arr["lora1_weights"]
    assert w.ndim == 1 and 0 < w.size < (5 << 20) and np.all(np.diff(w) > 0)
    np.testing.assert_array_equal(arr["lora1_grad"], -w)


def test_dump_outputs_sample_is_reproducible(tmp_path):
    bench.dump_outputs(str(tmp_path / "a"), _out(), [])
    bench.dump_outputs(str(tmp_path / "b"), _out(), [])
    for f in os.listdir(tmp_path / "a"):
        np.testing.assert_array_equal(np.load(tmp_path / "a" / f), np.load(tmp_path / "b" / f))
