"""``fd_bank_norms`` on the bf16 library (libfairdiff_hip_bf16.so) -- run as a SCRIPT in its own process, because a process's working dtype is fixed at import:

    FD_DTYPE=bf16 python tests/run_bf16_banknorms_checks.py

The entry point has no working-dtype operand (fp32 in, fp64 partials, fp32 out): the run shows that it is present in that library and the same there.  The
bank, the fp64 references and the derived bound are those of tests/banknorms_cases.py: the three-buffer accuracy case and NaN in the padding slots.
tests/test_banknorms_bf16_gpu.py launches it."""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))


def main():
    assert os.environ.get("FD_DTYPE") == "bf16", "run with FD_DTYPE=bf16"
    import banknorms_cases as C
    from finetune_fair_diffusion_amd import layers, lib, ops
    dev = torch.device("cuda:0")
    assert lib.get().fd_working_dtype().decode() == "bf16" and ops.F16 == torch.bfloat16
    bank = C.make_bank(layers, dev)
    plan = bank.norm_plan()
    plan.out.fill_(C.SENTINEL)
    norms, summary = C.norms_only(ops, plan, p=bank.flat, ema=bank.ema, g=bank.grad)
    for b, name in enumerate(C.BUFFERS[:3]):
        C.check_row("bf16 library, " + name, norms[b], summary[b], C.reference(bank, getattr(bank, name)))
    assert np.all(norms[3] == C.SENTINEL) and np.all(summary[3] == C.SENTINEL), "rows of an absent buffer are not written"
    pad = C.padding_mask(bank).to(dev)
    dirty = [getattr(bank, name).clone() for name in C.BUFFERS[:3]]
    for t in dirty:
        t[pad] = float("nan")
    n, s = C.norms_only(ops, plan, p=dirty[0], ema=dirty[1], g=dirty[2])
    assert np.array_equal(n[:3].view(np.uint32), norms[:3].view(np.uint32)) and np.array_equal(s[:3].view(np.uint32), summary[:3].view(np.uint32)), \
        "NaN in the padding slots reached a result"
    print("[bf16 padding] ok")
    print("BF16 BANK NORMS CHECKS PASSED")


if __name__ == "__main__":
    main()
