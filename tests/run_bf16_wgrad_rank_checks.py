"""LoRA weight gradients at ranks 17..64 on the bf16 library (libfairdiff_hip_bf16.so) -- run as a SCRIPT in its own process, because a process's working
dtype is fixed at import:

    FD_DTYPE=bf16 python tests/run_bf16_wgrad_rank_checks.py

The problems, the fp64 reference and band B1 are those of tests/wgrad_rank_cases.py with bf16 operands (products of two bf16 numbers are exact in fp32 too):
the mixed batch at every rank, T's pad columns, and bit-equal repeats, also beside a GEMM on another stream.  tests/test_lora_wgrad_rank_bf16_gpu.py launches it."""
import os
import sys

import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
BF = torch.bfloat16


def main():
    assert os.environ.get("FD_DTYPE") == "bf16", "run with FD_DTYPE=bf16"
    import wgrad_rank_cases as W
    from finetune_fair_diffusion_amd import lib, ops
    dev = torch.device("cuda:0")
    assert lib.get().fd_working_dtype().decode() == "bf16" and ops.F16 == BF

    def names(calls):
        return [c for c in calls if c.startswith("fd_lora_wgrad")]

    # case 1: the mixed batch, one call per rank
    for R in (17, 32, 50, 64):
        probs = W.mixed(dev, BF, R)
        with W.counted(ops) as calls:
            outs = W.run(ops, probs)
        assert names(calls) == ["fd_lora_wgrad_multi"], f"R={R}: one batched call expected, got {names(calls)}"
        for p, G in zip(probs, outs):
            W.band("bf16 batched", p, G, 1.0, BF)

    # case 3: pad columns of T are not read into the result; nothing outside an embedded [R, N] window is written
    R = 50
    probs = W.mixed(dev, BF, R)
    clean = W.run(ops, probs)
    dirty = W.run(ops, [p.with_pad(1000.0) for p in probs])
    for p, a, b in zip(probs, clean, dirty):
        W.band("bf16 pads 1000", p, b, 1.0, BF)
        assert torch.equal(a, b), f"{p.M}x{p.N}: pad columns of T reached the result ({int((a != b).sum())} elements differ)"
    p, SENT = probs[1], 12345.0
    buf = torch.full((R + 6, p.N + 24), SENT, dtype=torch.float32, device=dev)
    win = buf[3:3 + R, 8:8 + p.N]
    win.zero_()
    with ops.wgrad_batch():
        ops.lora_wgrad(p.X, p.T, win, 1, buf.stride(0), R, scale=W.SCALE)
    W.band("bf16 embedded window", p, win, 0.0, BF)
    outside = torch.ones_like(buf, dtype=torch.bool)
    outside[3:3 + R, 8:8 + p.N] = False
    assert bool((buf[outside] == SENT).all()), "an element outside the R x N window of G was written"

    # case 6: bit-equal repeats, also on a second stream beside a large GEMM on the first
    a, b = W.rnd(8192, 4096, dev=dev, seed=5, dtype=BF), W.rnd(4096, 4096, dev=dev, seed=6, dtype=BF)
    second = W.run(ops, probs)
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    ops.gemm(a, b)
    with torch.cuda.stream(side):
        third = W.run(ops, probs)
    torch.cuda.synchronize()
    for p, x, y, z in zip(probs, clean, second, third):
        assert torch.equal(x, y), f"{p.M}x{p.N}: two runs differ in {int((x != y).sum())} elements"
        assert torch.equal(x, z), f"{p.M}x{p.N}: the run beside a GEMM on another stream differs in {int((x != z).sum())} elements"
    print("[bf16 determinism] ok")
    print("BF16 WGRAD RANK CHECKS PASSED")


if __name__ == "__main__":
    main()
