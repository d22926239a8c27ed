"""Direct tests of ``fd_warp_affine_u8_fwd`` (csrc/evaluate.hip) through ``ops.warp_affine`` on uint8 HWC images: the aligned face chips against the fp64
host statement and the oracle's image pipeline, bit-exact identity / integer-shift maps, the mirror output, more than one grid pass, and source indices
outside the batch.  tests/facealign_cases.py holds the inputs; tests/run_bf16_facealign_checks.py runs the same cases on the bf16 library."""
import os
import subprocess
import sys

import pytest
import torch

import facealign_cases as FC
from test_kernels_gpu import check

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))


@pytest.fixture(scope="module")
def ops():
    from finetune_fair_diffusion_amd import ops
    return ops


def test_aligned_chips_match_the_fp64_host_statement(ops, dev):
    """Two 48x64 images to four 28^2 chips -- two chips of one image, one spilling over a corner, one strongly minified -- at the band of the
    working-dtype kernel for this quantity (``test_warp_affine_production_size``)."""
    u8, src, A, S, ref = FC.small_case()
    chips = ops.warp_affine(u8.to(dev), torch.tensor(src, dtype=torch.int32, device=dev), A.to(dev), S)
    assert chips.dtype == ops.F16 and tuple(chips.shape) == (4, 3, S, S)
    for k in range(4):
        check(f"aligned chip {k} from bytes 48x64->{S}", chips[k], ref[k].to(dev), 2e-3)
    assert float((ref[2] == -1).float().mean()) > 0.05


def test_aligned_chips_production_size(ops, dev):
    """512^2 images to 112^2 chips with the three faces of ``test_warp_affine_production_size``, against ``oracle.nn_sfnet.image_pipeline``."""
    u8, src, A, S, ref = FC.production_case()
    chips = ops.warp_affine(u8.to(dev), torch.tensor(src, dtype=torch.int32, device=dev), A.to(dev), S)
    check("aligned chips from bytes 512->112", chips, ref.to(dev), 2e-3)
    assert float((ref[2] == -1).float().mean()) > 0.05


def test_identity_and_integer_shift_are_exact(ops, dev):
    """The identity map at S = H = W = 16 gives ``u/255*2-1`` rounded to the working dtype, bit for bit; a translation by (+3, -2) gives that shifted,
    with exactly -1 where it leaves the image."""
    u8, A, want_id, want_shift = FC.exact_case(ops.F16)
    idx = torch.zeros(2, dtype=torch.int32, device=dev)
    chips = ops.warp_affine(u8.to(dev), idx, A.to(dev), 16).cpu()
    assert torch.equal(chips[0].view(torch.int16), want_id.view(torch.int16))
    assert torch.equal(chips[1].view(torch.int16), want_shift.view(torch.int16))
    assert bool((want_shift[:, :2] == -1).all()) and bool((want_shift[:, :, 13:] == -1).all()) and bool((want_shift[:, 2:, :13] != -1).any())


@pytest.mark.parametrize("S", [28, 27])
def test_mirror_is_the_flip(ops, dev, S):
    u8, src, A, _, _ = FC.small_case(S=S, reference=False)
    idx = torch.tensor(src, dtype=torch.int32, device=dev)
    chips, mirror = ops.warp_affine(u8.to(dev), idx, A.to(dev), S, mirror=True)
    assert mirror.dtype == chips.dtype and mirror.shape == chips.shape and mirror.is_contiguous()
    assert torch.equal(mirror, chips.flip(3))
    assert torch.equal(chips, ops.warp_affine(u8.to(dev), idx, A.to(dev), S))          # the mirror output does not change the chips
    assert not torch.equal(mirror, chips)


def test_more_than_one_grid_pass(ops, dev):
    """1400 chips of 112^2 are more output pixels than the capped grid has threads: chip k cycles over four maps and is bit-equal to chip k mod 4."""
    u8, src, A, S, _ = FC.production_case(reference=False)
    n = 1400
    assert n * S * S > 65536 * 256
    src4, A4 = (src + [1]), torch.cat([A, A[:1]])
    idx = torch.tensor([src4[k % 4] for k in range(n)], dtype=torch.int32, device=dev)
    Am = A4.repeat((n + 3) // 4, 1)[:n].contiguous().to(dev)
    chips, mirror = ops.warp_affine(u8.to(dev), idx, Am, S, mirror=True)
    first, first_m = chips[:4], mirror[:4]
    assert not torch.equal(first[0], first[3])          # map 0 on image 0 and on image 1
    assert torch.equal(chips.view(n // 4, 4, 3, S, S), first.expand(n // 4, 4, 3, S, S))
    assert torch.equal(mirror.view(n // 4, 4, 3, S, S), first_m.expand(n // 4, 4, 3, S, S))
    assert torch.equal(first_m, first.flip(3))


def test_source_index_outside_the_batch_gives_the_fill(ops, dev):
    u8, src, A, S, _ = FC.small_case(reference=False)
    B = u8.shape[0]
    good = ops.warp_affine(u8.to(dev), torch.tensor(src, dtype=torch.int32, device=dev), A.to(dev), S)
    bad = list(src)
    bad[1], bad[3] = -1, B
    chips, mirror = ops.warp_affine(u8.to(dev), torch.tensor(bad, dtype=torch.int32, device=dev), A.to(dev), S, fill=0.5, mirror=True)
    for k in (1, 3):
        assert bool((chips[k] == 0.5).all()) and bool((mirror[k] == 0.5).all())
    good_half = ops.warp_affine(u8.to(dev), torch.tensor(src, dtype=torch.int32, device=dev), A.to(dev), S, fill=0.5)
    for k in (0, 2):
        assert torch.equal(chips[k], good_half[k]) and torch.equal(mirror[k], good_half[k].flip(2))
    assert not torch.equal(good[2], good_half[2])          # chip 2 reads the fill where it leaves its image


def test_bf16_library_runs_the_same_cases(dev):
    """tests/run_bf16_facealign_checks.py in one fresh child process under FD_DTYPE=bf16 (a process's working dtype is fixed at import); a child that
    crashes or runs out of time is not started again."""
    env = dict(os.environ, FD_DTYPE="bf16")
    env.pop("FAIRDIFF_LIB", None)
    try:
        r = subprocess.run([sys.executable, os.path.join(HERE, "run_bf16_facealign_checks.py")], env=env, capture_output=True, text=True, timeout=120)
    except subprocess.TimeoutExpired as e:
        out = e.stdout.decode(errors="replace") if isinstance(e.stdout, bytes) else (e.stdout or "")
        print(out[-6000:])
        pytest.fail("the bf16 face-alignment checks did not finish in 120 s (not retried)")
    print(r.stdout[-12000:])
    print(r.stderr[-3000:])
    assert r.returncode == 0, f"exit code {r.returncode} (not retried)"
    assert "BF16 FACEALIGN CHECKS PASSED" in r.stdout
