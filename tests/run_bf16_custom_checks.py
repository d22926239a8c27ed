"""``--experiment custom`` on the bf16 library (libfairdiff_hip_bf16.so) -- run as a SCRIPT in its own process, because a process's working dtype is fixed at
import:

    FD_DTYPE=bf16 python tests/run_bf16_custom_checks.py

The cases are those of tests/custom_cases.py: the restatement of exp-3 bit for bit and the non-uniform binary target on the device tail.
tests/test_custom_targets_bf16_gpu.py launches it."""
import os
import sys

import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))


def main():
    assert os.environ.get("FD_DTYPE") == "bf16", "run with FD_DTYPE=bf16"
    import custom_cases as C
    from finetune_fair_diffusion_amd import lib, ops
    dev = torch.device("cuda:0")
    assert lib.get().fd_working_dtype().decode() == "bf16" and ops.F16 == torch.bfloat16
    snaps, _, _ = C.check_restatement(dev, "exp-3")
    print("[bf16 exp-3 restated] ok", {k: v.tolist() for k, v in snaps[-1].items() if k.startswith("targets_by_attr/")})
    _, out = C.check_non_uniform_binary(dev)
    print("[bf16 gender 0.75 / 0.25] ok", out["targets"].tolist())
    print("BF16 CUSTOM TARGETS CHECKS PASSED")


if __name__ == "__main__":
    main()
