"""``fd_warp_affine_u8_fwd`` on the bf16 library (libfairdiff_hip_bf16.so, FD_DTYPE=bf16) -- run as a SCRIPT in its own process, because a process's
working dtype is fixed at import; tests/test_kernels_facealign_gpu.py starts it once:

    FD_DTYPE=bf16 python tests/run_bf16_facealign_checks.py

``tests/run_bf16_kernel_checks.py`` reaches ``ops.warp_affine`` with working-dtype images only; the path from uint8 images is checked here, on the cases of
tests/facealign_cases.py: the fp64 host statement at 8 x the fp16 band (8 = the ratio of the unit roundoffs, the convention of that script for
``warp_affine``), the identity and integer-shift maps bit for bit, and the mirror output bit for bit.  Every check prints its figure; failures are
collected, printed, and the exit code is non-zero, or the last line is ``BF16 FACEALIGN CHECKS PASSED``."""
import math
import os
import sys

import torch

HERE = os.path.dirname(os.path.abspath(__file__))
BF = torch.bfloat16
FAILED = []


def expect(name, ok, detail=""):
    print(f"[{name}] {'ok' if ok else 'FAILED'} {detail}")
    if not ok:
        FAILED.append(name)


def main():
    sys.path.insert(0, HERE)
    sys.path.insert(0, os.path.dirname(HERE))
    from finetune_fair_diffusion_amd import lib, ops
    import facealign_cases as FC
    dev = torch.device("cuda:0")
    assert lib.get().fd_working_dtype().decode() == "bf16" and ops.F16 == BF
    i32 = lambda a: torch.tensor(a, dtype=torch.int32, device=dev)

    u8, src, A, S, ref = FC.small_case()
    chips = ops.warp_affine(u8.to(dev), i32(src), A.to(dev), S)
    expect("dtype and shape", chips.dtype == BF and tuple(chips.shape) == (4, 3, S, S))
    tol = 8 * 2e-3
    for k in range(4):
        e = float((chips[k].float().cpu() - ref[k]).abs().max() / (ref[k].abs().max() + 1e-12))
        expect(f"aligned chip {k} from bytes 48x64->{S}", math.isfinite(e) and e <= tol, f"rel max err {e:.3e} (tol {tol:.1e})")

    u8e, Ae, want_id, want_shift = FC.exact_case(BF)
    got = ops.warp_affine(u8e.to(dev), i32([0, 0]), Ae.to(dev), 16).cpu()
    expect("identity map is bit-exact", torch.equal(got[0].view(torch.int16), want_id.view(torch.int16)))
    expect("integer shift is bit-exact", torch.equal(got[1].view(torch.int16), want_shift.view(torch.int16)))

    for Sm in (28, 27):
        u8m, srcm, Am, _, _ = FC.small_case(S=Sm, reference=False)
        c, m = ops.warp_affine(u8m.to(dev), i32(srcm), Am.to(dev), Sm, mirror=True)
        expect(f"mirror is the flip, S = {Sm}", m.dtype == BF and torch.equal(m, c.flip(3)) and not torch.equal(m, c))

    torch.cuda.synchronize()
    if FAILED:
        print("FAILED:", FAILED)
        sys.exit(1)
    print("BF16 FACEALIGN CHECKS PASSED")


if __name__ == "__main__":
    main()
