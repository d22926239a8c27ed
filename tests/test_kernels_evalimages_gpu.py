"""Direct tests of the offline evaluator's two kernels (csrc/evaluate.hip): ``fd_crop_resize_u8_fwd`` against torch's pad + bilinear interpolation of
the fp32 image ``u/255*2-1`` and, at scale one, bit for bit against that image; ``fd_eval_grid_attrs_u8`` byte for byte against its host statement
(evaluate_images.grid_attrs_host, itself pinned to the reference's arrays by tests/test_evalimages_cpu.py)."""
import ctypes
import math
import os
import subprocess
import sys

import numpy as np
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
GOLD = os.path.join(HERE, "golden")


@pytest.fixture(scope="module")
def ops():
    from finetune_fair_diffusion_amd import ops
    return ops


@pytest.fixture(scope="module")
def EI():
    from finetune_fair_diffusion_amd import evaluate_images
    return evaluate_images


def _unit(u8):
    """[B,H,W,3] uint8 -> the reference's fp32 NCHW image ``u/255*2-1``."""
    return u8.permute(0, 3, 1, 2).float() / 255 * 2 - 1


def _crop_ref(x, bb, S, fill=-1.0):
    """crop_face (Pad + Resize without antialias) of one fp32 image [3,H,W]; an empty box is a chip of ``fill``."""
    _, H, W = x.shape
    if bb[2] <= bb[0] or bb[3] <= bb[1]:
        return torch.full((3, S, S), fill)
    l, r, bt, tp = max(bb[0], 0), min(bb[2], W), max(bb[1], 0), min(bb[3], H)
    face = F.pad(x[:, bt:tp, l:r], [max(-bb[0], 0), max(bb[2] - W, 0), max(-bb[1], 0), max(bb[3] - H, 0)], value=fill)
    return F.interpolate(face[None], size=[S, S], mode="bilinear", align_corners=False)[0]


def _check_crop(ops, dev, u8, boxes, S):
    chips = ops.crop_resize_u8(u8.to(dev), torch.tensor(boxes, dtype=torch.int32, device=dev), -1.0, S)
    assert chips.dtype == ops.F16 and tuple(chips.shape) == (len(boxes), 3, S, S)
    x = _unit(u8)
    for i, bb in enumerate(boxes):
        ref = _crop_ref(x[i], bb, S)
        e = float((chips[i].float().cpu() - ref).abs().max() / (ref.abs().max() + 1e-20))
        print(f"[crop_resize_u8 {tuple(u8.shape[1:3])}->{S} box {bb}] rel max err {e:.3e} (tol 2.0e-03)")
        assert math.isfinite(e) and e <= 2e-3, (bb, e)
    return chips


def test_crop_resize_u8_matches_pad_and_interpolate(ops, dev):
    """48x64 images (H != W) to 28x28: a box inside, one over each edge, one larger than the image, one 2 pixels wide, and the no-face box."""
    H, W, S = 48, 64, 28
    boxes = [[8, 6, 50, 40], [-7, 5, 30, 42], [40, 4, 75, 39], [10, -9, 44, 25], [12, 20, 46, 60], [-10, -12, 80, 70], [30, 10, 32, 40], [-1, -1, -1, -1]]
    u8 = torch.randint(0, 256, (len(boxes), H, W, 3), generator=torch.Generator().manual_seed(21), dtype=torch.int64).to(torch.uint8)
    chips = _check_crop(ops, dev, u8, boxes, S)
    assert bool((chips[-1] == -1).all())


def test_crop_resize_u8_production_size(ops, dev):
    """512^2 -> 224^2 from an 8-pixel box (28x upsampling)."""
    u8 = torch.randint(0, 256, (1, 512, 512, 3), generator=torch.Generator().manual_seed(22), dtype=torch.int64).to(torch.uint8)
    _check_crop(ops, dev, u8, [[250, 251, 258, 259]], 224)


def test_crop_resize_u8_is_exact_at_scale_one(ops, dev):
    """A box of exactly SxS pixels: every output pixel is one tap with weight one, so the chip is ``u/255*2-1`` (a true fp32 division) rounded once to
    the working dtype, bit for bit, for all 256 byte values -- inside the image and, for a box sticking out, beside the fill."""
    S = 16
    u8 = torch.zeros((2, 24, 40, 3), dtype=torch.uint8)
    vals = torch.arange(256, dtype=torch.uint8).view(16, 16)
    u8[0, 4:20, 8:24, 0], u8[0, 4:20, 8:24, 1], u8[0, 4:20, 8:24, 2] = vals, vals.t(), vals.flip(0)
    u8[1, :16, :16] = u8[0, 4:20, 8:24]
    boxes = [[8, 4, 24, 20], [-3, -2, 13, 14]]
    chips = ops.crop_resize_u8(u8.to(dev), torch.tensor(boxes, dtype=torch.int32, device=dev), -1.0, S).cpu()
    x = _unit(u8)
    want0 = x[0, :, 4:20, 8:24].to(ops.F16)
    assert len(torch.unique(u8[0, 4:20, 8:24, 0])) == 256
    assert torch.equal(chips[0], want0), int((chips[0] != want0).sum())
    want1 = torch.full((3, S, S), -1.0)
    want1[:, 2:, 3:] = x[1, :, :14, :13]
    assert torch.equal(chips[1], want1.to(ops.F16)), int((chips[1] != want1.to(ops.F16)).sum())


def test_crop_resize_u8_refuses_bad_arguments(ops, dev):
    from finetune_fair_diffusion_amd import lib
    L = lib.get()
    stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    u8 = torch.zeros((2, 8, 8, 3), dtype=torch.uint8, device=dev)
    bx = torch.tensor([[0, 0, 8, 8]] * 2, dtype=torch.int32, device=dev)
    out = torch.full((2, 3, 4, 4), 7.0, dtype=ops.F16, device=dev)
    call = lambda img, boxes, chips, B, H, W, S: L.fd_crop_resize_u8_fwd(img, boxes, ctypes.c_float(-1.0), chips, B, H, W, S, stream)
    for a in ((None, bx.data_ptr(), out.data_ptr()), (u8.data_ptr(), None, out.data_ptr()), (u8.data_ptr(), bx.data_ptr(), None)):
        assert call(*a, 2, 8, 8, 4) == -1 and b"null" in L.fd_last_error()
    for B, H, W, S in ((0, 8, 8, 4), (2, 0, 8, 4), (2, 8, 4097, 4), (2, 8, 8, 0), (2, 8, 8, 4097)):
        assert call(u8.data_ptr(), bx.data_ptr(), out.data_ptr(), B, H, W, S) == -1 and b"fd_crop_resize_u8_fwd" in L.fd_last_error(), (B, H, W, S)
    torch.cuda.synchronize()
    assert bool((out == 7).all())                                   # refused calls launched nothing


# ----------------------------------------------------------------------------- the grid
def _grid_case(EI, ops, dev, images, boxes, preds, bars, order):
    N, H, W, _ = images.shape
    n_attr = preds.shape[0]
    pal = EI.PALETTES[:n_attr]
    ref = EI.grid_attrs_host(images, order, boxes, preds, bars, pal)
    rows, cols, shape = EI.grid_attrs_shape(N, H, W, n_attr)
    nbytes = shape[0] * shape[1] * shape[2]
    buf = torch.full((nbytes + 64,), 0xA5, dtype=torch.uint8, device=dev)
    i32 = lambda a: torch.as_tensor(np.asarray(a), dtype=torch.int32).to(dev).contiguous()
    P = max(len(p) for p in pal)
    pal_t = torch.tensor([p + [(255, 255, 255)] * (P - len(p)) for p in pal], dtype=torch.uint8, device=dev)
    out = ops.eval_grid_attrs(torch.as_tensor(images).to(dev).contiguous(), i32(order), i32(boxes), i32(preds), i32(bars), pal_t, out=buf[:nbytes].view(shape))
    got = out.cpu().numpy()
    assert bool((buf[nbytes:] == 0xA5).all()), "bytes behind the grid were written"
    bad = np.argwhere(got != ref)
    assert got.shape == ref.shape and len(bad) == 0, (n_attr, len(bad), bad[:5].tolist())
    return got, nbytes


@pytest.mark.parametrize("n_attr", [2, 3])
def test_eval_grid_attrs_matches_host_and_reference_on_goldens(dev, ops, EI, n_attr):
    g = np.load(os.path.join(GOLD, "reference_evalimages_grid.npz"))
    for case in "ab":
        im, bx, pr, pb = g[f"{case}_images"], g[f"{case}_boxes"], g[f"{case}_preds"][:n_attr], g[f"{case}_probs"][:n_attr]
        bars = EI.grid_attrs_bar_rows(torch.from_numpy(pb).to(dev))                    # computed on the device, as the evaluator does
        order = EI.device_order(torch.from_numpy(pr).to(dev).long(), torch.from_numpy(pb).to(dev))
        assert order.cpu().tolist() == EI.grid_attrs_order(pr, pb).tolist()
        got, _ = _grid_case(EI, ops, dev, im, bx, pr, bars.cpu().numpy(), order.cpu().numpy())
        assert np.array_equal(got, g[f"{case}_grid{n_attr}"])                          # the reference's own array


@pytest.mark.parametrize("N,H,W", [(7, 40, 36), (3, 41, 37)])
def test_eval_grid_attrs_matches_host_on_a_random_case(dev, ops, EI, N, H, W):
    """One, two and three strips on random bytes: a partly filled last row, a -1 row, bar_rows of -1, 0 and beyond H, every byte value, a box on the
    border, one sticking out and one narrower than two outline widths.  At H = 40 a grid has rows * 60 pixel rows, so its size is a multiple of 4 whatever
    W is; the second shape (one row of tiles, odd tile height and widths) makes the size odd for one and three strips and runs the byte-wise tail."""
    rng = np.random.RandomState(61 + N)
    images = rng.randint(0, 256, (N, H, W, 3)).astype(np.uint8)
    images[0].reshape(-1)[:256] = np.arange(256)
    boxes = np.array([[0, 0, W - 1, H - 1], [-5, 10, 20, 50], [10, 10, 12, 30], [5, 5, 30, 30], [-1, -1, -1, -1], [20, 2, 35, 9], [3, 30, 33, 38]])[:N]
    noface = 4 if N > 4 else N - 1
    boxes[noface] = -1
    tails = []
    for n_attr in (1, 2, 3):
        preds = np.stack([rng.randint(0, 2, N), rng.randint(0, 4, N), rng.randint(0, 2, N)])[:n_attr]
        bars = rng.randint(1, H - 1, (n_attr, N))
        bars[:, 0], bars[:, 1] = -1, 0
        bars[-1, 1] = H + 100
        preds[:, noface] = -1
        bars[:, noface] = 1024
        _, nbytes = _grid_case(EI, ops, dev, images, boxes, preds, bars, rng.permutation(N))
        tails.append(nbytes % 4)
    assert any(tails) == (H == 41), tails


def test_eval_grid_attrs_refuses_bad_arguments(dev, ops):
    from finetune_fair_diffusion_amd import lib
    N, H, W = 5, 16, 16
    img = torch.zeros((N, H, W, 3), dtype=torch.uint8, device=dev)
    z = torch.zeros((3, N), dtype=torch.int32, device=dev)
    bx = torch.zeros((N, 4), dtype=torch.int32, device=dev)
    pal = torch.zeros((3, 6, 3), dtype=torch.uint8, device=dev)
    out = torch.full((4 * (H + 20) * 4 * (W + 170) * 3 + 8,), 9, dtype=torch.uint8, device=dev)       # room for any of the refused shapes
    L = lib.get()
    stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    p = lambda t: t.data_ptr()
    call = lambda a, n, n_attr, rows, cols: L.fd_eval_grid_attrs_u8(a[0], a[1], a[2], a[3], a[4], a[5], a[6], n, H, W, n_attr, rows, cols, stream)
    good = [p(img), p(z), p(bx), p(z), p(z), p(pal), p(out)]
    for k in range(7):                                              # each pointer in turn
        a = list(good)
        a[k] = None
        assert call(a, N, 2, 2, 3) == -1 and b"null" in L.fd_last_error(), k
    for n_attr in (0, 4):
        assert call(good, N, n_attr, 2, 3) == -1 and b"n_attr" in L.fd_last_error()
    a = list(good)
    a[6] = p(out) + 1
    assert call(a, N, 2, 2, 3) == -1 and b"aligned" in L.fd_last_error()
    for rows, cols in ((1, 4), (2, 2), (0, 5), (3, 3), (4, 2)):    # cannot hold N, or a whole row of empty tiles
        assert call(good, N, 2, rows, cols) == -1 and b"fd_eval_grid_attrs_u8" in L.fd_last_error(), (rows, cols)
    assert call(good, 0, 2, 1, 1) == -1 and call(good, 4097, 2, 64, 65) == -1
    torch.cuda.synchronize()
    assert bool((out == 9).all())                                   # refused calls launched nothing
    # the wrapper refuses an output buffer that is not exactly the grid: the entry point cannot see its size
    shape = (2 * (H + 20), 3 * (W + 120), 3)
    ok = out[:shape[0] * shape[1] * 3].view(shape)
    for bad in (ok[:-1], ok.view(-1), ok.to(torch.int8)):
        with pytest.raises(AssertionError):
            ops.eval_grid_attrs(img, z[0], bx, z[:2], z[:2], pal[:2], out=bad)
    ops.eval_grid_attrs(img, z[0].contiguous(), bx, z[:2], z[:2], pal[:2], out=ok)
    torch.cuda.synchronize()
    assert bool((out[ok.numel():] == 9).all()) and not bool((ok == 9).all())


def test_evalimages_kernels_with_bf16_library(dev):
    """The exactness test and the grid tests again in a process that loads the bf16 library (the crop band is fp16's)."""
    if os.environ.get("FD_DTYPE", "fp16").lower() in ("bf16", "bfloat16"):
        return          # this process already runs the bf16 library
    env = dict(os.environ, FD_DTYPE="bf16")
    env.pop("FAIRDIFF_LIB", None)
    r = subprocess.run([sys.executable, "-m", "pytest", "-q", "-m", "gpu", "-p", "no:cacheprovider", os.path.abspath(__file__), "-k",
                        "exact or grid_attrs or refuses"], env=env, capture_output=True, text=True, timeout=600, cwd=os.path.dirname(HERE))
    print(r.stdout[-4000:])
    print(r.stderr[-2000:])
    assert r.returncode == 0 and " passed" in r.stdout and "failed" not in r.stdout and "skipped" not in r.stdout
