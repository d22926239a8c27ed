"""``fd_lora_merge_multi`` on the bf16 library (libfairdiff_hip_bf16.so) -- run as a SCRIPT in its own process, because a process's working dtype is fixed at
import:

    FD_DTYPE=bf16 python tests/run_bf16_loramerge_checks.py

The entry point has no working-dtype operand (fp32 in, fp32 out): the run shows that it is present in that library and passes the same table there -- the
cases, fp64 references and the gate of tests/loramerge_cases.py, out of place and in place, 17 pairs in one call, guards intact -- and that two calls give
the same bits.  tests/test_loramerge_bf16_gpu.py launches it."""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))


def main():
    assert os.environ.get("FD_DTYPE") == "bf16", "run with FD_DTYPE=bf16"
    import loramerge_cases as C
    from finetune_fair_diffusion_amd import layers, lib, ops
    dev = torch.device("cuda:0")
    assert lib.get().fd_working_dtype().decode() == "bf16" and ops.F16 == torch.bfloat16
    C.run_table(layers, dev, "bf16 library")
    p = C.Problem(layers, dev, C.MIXED_17, seed=50)
    first = p.run(layers, in_place=False, scale=-2.5)
    second = p.run(layers, in_place=False, scale=-2.5)
    assert all(np.array_equal(a.view(np.uint32), b.view(np.uint32)) for a, b in zip(first, second)), "two calls differ"
    print("[bf16 repeat] ok")
    print("BF16 LORA MERGE CHECKS PASSED")


if __name__ == "__main__":
    main()
