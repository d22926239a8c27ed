"""``fd_cosine_logits_fwd`` / ``fd_cosine_logits_bwd`` and the zero-shot classifier on the bf16 library (libfairdiff_hip_bf16.so) -- run as a SCRIPT in its
own process, because a process's working dtype is fixed at import:

    FD_DTYPE=bf16 python tests/run_bf16_cosinehead_checks.py

The two entry points have no working-dtype operand (fp32 in, fp32 out): the run shows that they are present in that library and pass the same table
there -- the cases, fp64 references and gates of tests/cosinehead_cases.py, guards intact -- and that repeated calls give the same bits.  Then one
classifier leg: ``ZeroShotClipClassifier`` on the tiny CLIP tower against the fp32 oracle tower with the head restated in torch
(tests/zeroshot_refs.py), under the fp16 bands of that tower times 4 -- the factor the project's end-to-end bf16 checks apply to their fp16 bands
(tests/run_bf16_checks.py: 8e-2 for 2e-2, 2e-1 for 5e-2; bf16 has 8 significand bits against fp16's 11), no new number.
tests/test_cosinehead_bf16_gpu.py launches it."""
import os
import sys

import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))


def main():
    assert os.environ.get("FD_DTYPE") == "bf16", "run with FD_DTYPE=bf16"
    import cosinehead_cases as C
    import zeroshot_refs as Z
    from finetune_fair_diffusion_amd import lib, ops
    dev = torch.device("cuda:0")
    assert lib.get().fd_working_dtype().decode() == "bf16" and ops.F16 == torch.bfloat16
    C.run_table(ops, dev, "bf16 library", show=False)
    C.repeat_bits(ops, dev)
    print("[bf16 repeat] ok")
    Z.check_classifier(dev, "bf16 library", *Z.bf16_bands())
    print("BF16 COSINE HEAD CHECKS PASSED")


if __name__ == "__main__":
    main()
