"""Direct tests of the training monitor's painter ``fd_eval_grid_attrs`` (csrc/evaluate.hip): byte for byte against its host statement
(evaluation.grid_attrs_img_host, itself pinned to the reference's train plots by tests/test_trainplots_cpu.py) and against the reference's arrays,
its refusals, and the device derivation of predictions, bars and tile order (evaluation.grid_inputs_attrs) against the host rules."""
import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
GOLD = os.path.join(HERE, "golden")
PAD = 4096          # bytes of 0xAB in front of and behind the painted grid


@pytest.fixture(scope="module")
def ops():
    from finetune_fair_diffusion_amd import ops
    return ops


@pytest.fixture(scope="module")
def E():
    from finetune_fair_diffusion_amd import evaluation
    return evaluation


@pytest.fixture(scope="module")
def EI():
    from finetune_fair_diffusion_amd import evaluate_images
    return evaluate_images


def _grid_case(E, EI, ops, dev, images, boxes, preds, bars, order):
    """Paints into the middle of a larger 0xAB-filled buffer; returns (painted array, the images as the device held them, grid bytes)."""
    N, _, H, W = images.shape
    n_attr = preds.shape[0]
    pal = EI.PALETTES[:n_attr]
    imgs_wd = torch.as_tensor(images).to(ops.F16)              # what the device holds (bf16 rounds fp16 values once more)
    ref = E.grid_attrs_img_host(imgs_wd, order, boxes, preds, bars, pal)
    rows, cols, shape = E.grid_attrs_shape(N, H, W, n_attr)
    nbytes = shape[0] * shape[1] * shape[2]
    buf = torch.full((PAD + nbytes + PAD,), 0xAB, dtype=torch.uint8, device=dev)
    i32 = lambda a: torch.as_tensor(np.asarray(a), dtype=torch.int32).to(dev).contiguous()
    P = max(len(p) for p in pal)
    pal_t = torch.tensor([p + [(255, 255, 255)] * (P - len(p)) for p in pal], dtype=torch.uint8, device=dev)
    out = ops.eval_grid_attrs_img(imgs_wd.to(dev).contiguous(), i32(order), i32(boxes), i32(preds), i32(bars), pal_t, out=buf[PAD:PAD + nbytes].view(shape))
    got = out.cpu().numpy()
    assert bool((buf[:PAD] == 0xAB).all()) and bool((buf[PAD + nbytes:] == 0xAB).all()), "bytes around the grid were written"
    bad = np.argwhere(got != ref)
    assert got.shape == ref.shape and len(bad) == 0, (n_attr, len(bad), bad[:5].tolist())
    return got, imgs_wd, nbytes


@pytest.mark.parametrize("n_attr", [2, 3])
def test_eval_grid_attrs_img_matches_host_and_reference_on_goldens(dev, ops, E, EI, n_attr):
    g = np.load(os.path.join(GOLD, "reference_trainplot_grid.npz"))
    im, bx, pr, pb = g["images"], g["boxes"], g[f"preds{n_attr}"], g["probs"][:n_attr]
    bars = EI.grid_attrs_bar_rows(torch.from_numpy(pb).to(dev))                        # computed on the device, as the monitor does
    order = EI.device_order(torch.from_numpy(pr).to(dev).long(), torch.from_numpy(pb).to(dev))
    assert order.cpu().tolist() == EI.grid_attrs_order(pr, pb).tolist()
    got, _, _ = _grid_case(E, EI, ops, dev, torch.from_numpy(im), bx, pr, bars.cpu().numpy(), order.cpu().numpy())
    if ops.F16 == torch.float16:        # the golden's pixel values are fp16: the fp16 library reproduces the reference's own array
        assert np.array_equal(got, g[f"grid{n_attr}"])


@pytest.mark.parametrize("N", [7, 1])
def test_eval_grid_attrs_img_matches_host_on_a_random_case(dev, ops, E, EI, N):
    """One, two and three strips at H = 40, W = 37 (image rows start off 4-byte boundaries; at N = 7 the last row of tiles is partly filled): values
    over the whole of [-1,1] with both ends, a -1 row, bar_rows of -1, 0 and beyond H, a box on the border, one sticking out, one narrower than two
    outline widths."""
    H, W = 40, 37
    rng = np.random.RandomState(71 + N)
    images = torch.from_numpy(rng.uniform(-1, 1, (N, 3, H, W)).astype(np.float32)).clamp(-1, 1)
    images[0, :, :2] = 1.0
    images[0, :, 2:4] = -1.0
    boxes = np.array([[0, 0, W - 1, H - 1], [-5, 10, 20, 50], [10, 10, 12, 30], [5, 5, 30, 30], [-1, -1, -1, -1], [20, 2, 35, 9], [3, 30, 33, 38]])[:N]
    noface = 4 if N > 4 else None
    for n_attr in (1, 2, 3):
        preds = np.stack([rng.randint(0, 2, N), rng.randint(0, 4, N), rng.randint(0, 2, N)])[:n_attr]
        bars = rng.randint(1, H - 1, (n_attr, N))
        bars[:, 0] = -1 if N > 1 else H + 100
        if N > 1:
            bars[:, 1] = 0
            bars[-1, 1] = H + 100
        if noface is not None:
            preds[:, noface] = -1
            bars[:, noface] = 1024
        _grid_case(E, EI, ops, dev, images, boxes, preds, bars, rng.permutation(N))


def test_eval_grid_attrs_img_refuses_bad_arguments(dev, ops):
    from finetune_fair_diffusion_amd import lib
    N, H, W = 5, 16, 16
    img = torch.zeros((N, 3, H, W), dtype=ops.F16, device=dev)
    z = torch.zeros((3, N), dtype=torch.int32, device=dev)
    bx = torch.zeros((N, 4), dtype=torch.int32, device=dev)
    pal = torch.zeros((3, 6, 3), dtype=torch.uint8, device=dev)
    out = torch.full((4 * (H + 20) * 4 * (W + 170) * 3 + 8,), 9, dtype=torch.uint8, device=dev)       # room for any of the refused shapes
    L = lib.get()
    stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    p = lambda t: t.data_ptr()
    call = lambda a, n, h, w, n_attr, rows, cols: L.fd_eval_grid_attrs(a[0], a[1], a[2], a[3], a[4], a[5], a[6], n, h, w, n_attr, rows, cols, stream)
    refused = lambda rc: rc != 0 and b"fd_eval_grid_attrs:" in L.fd_last_error()
    good = [p(img), p(z), p(bx), p(z), p(z), p(pal), p(out)]
    for k in range(7):                                              # each pointer in turn
        a = list(good)
        a[k] = None
        assert refused(call(a, N, H, W, 2, 2, 3)) and b"null" in L.fd_last_error(), k
    for n_attr in (0, 4):
        assert refused(call(good, N, H, W, n_attr, 2, 3)) and b"n_attr" in L.fd_last_error()
    for n, h, w, rows, cols in ((0, H, W, 1, 1), (4097, H, W, 64, 65), (N, 0, W, 2, 3), (N, 4097, W, 2, 3), (N, H, 0, 2, 3), (N, H, 4097, 2, 3)):
        assert refused(call(good, n, h, w, 2, rows, cols)) and b"supported 1..4096" in L.fd_last_error(), (n, h, w)
    for rows, cols in ((1, 4), (2, 2), (0, 5), (3, 3), (4, 2)):    # cannot hold N, or a whole row of empty tiles
        assert refused(call(good, N, H, W, 2, rows, cols)) and b"does not hold" in L.fd_last_error(), (rows, cols)
    a = list(good)
    a[6] = p(out) + 1
    assert refused(call(a, N, H, W, 2, 2, 3)) and b"aligned" in L.fd_last_error()
    torch.cuda.synchronize()
    assert bool((out == 9).all())                                   # refused calls launched nothing
    # the wrapper refuses an output buffer that is not exactly the grid, and images that are not the working dtype
    shape = (2 * (H + 20), 3 * (W + 120), 3)
    ok = out[:shape[0] * shape[1] * 3].view(shape)
    for bad in (ok[:-1], ok.view(-1), ok.to(torch.int8)):
        with pytest.raises(AssertionError):
            ops.eval_grid_attrs_img(img, z[0].contiguous(), bx, z[:2], z[:2], pal[:2], out=bad)
    with pytest.raises(AssertionError):
        ops.eval_grid_attrs_img(img.float(), z[0].contiguous(), bx, z[:2], z[:2], pal[:2], out=ok)
    torch.cuda.synchronize()
    assert bool((out == 9).all())
    ops.eval_grid_attrs_img(img, z[0].contiguous(), bx, z[:2], z[:2], pal[:2], out=ok)
    torch.cuda.synchronize()
    assert bool((out[ok.numel():] == 9).all()) and not bool((ok == 9).all())


def _host_inputs(EI, table, attrs):
    """preds / probs of every attribute by the host rules (first maximum wins, -1 where a face is missing), bars and order from them."""
    preds, probs = [], []
    for c0, k in attrs:
        p = table[:, c0:c0 + k]
        valid = (p != -1).all(dim=-1)
        preds.append(torch.where(valid, p.argmax(dim=-1), torch.full((len(p),), -1)).numpy())      # CPU argmax: the first maximum
        probs.append(p.max(dim=-1).values.numpy())
    preds, probs = np.stack(preds), np.stack(probs).astype(np.float32)
    return preds, probs, EI.grid_attrs_bar_rows(torch.from_numpy(probs)).numpy(), EI.grid_attrs_order(preds, probs)


@pytest.mark.parametrize("sizes", [(2, 4), (2, 4, 2)])
def test_grid_inputs_attrs_equals_the_host_rules(dev, E, EI, sizes):
    """Seeded tables with ties between classes (the first maximum must win), ties in confidence inside a group (index order), confidences of exactly
    1 (no bar; the age bar follows race's), every class of every attribute, and -1 rows."""
    attrs, c = [], 0
    for k in sizes:
        attrs.append((c, k))
        c += k
    N = 96
    g = torch.Generator().manual_seed(40 + len(sizes))
    t = torch.cat([torch.softmax(torch.randn(N, k, generator=g) * 2, dim=-1) for k in sizes], dim=1)
    for c0, k in attrs:
        t[0::7, c0:c0 + k] = 1.0 / k                                # every class ties: class 0 wins
    t[1::9, 2:6] = torch.tensor([0.1, 0.4, 0.4, 0.1])               # race classes 1 and 2 tie: 1 wins
    t[3] = t[12] = t[11]                                            # three rows of one group with equal confidences
    t[20] = t[30] = t[25]
    t[40, 2:6] = torch.tensor([0.0, 0.0, 1.0, 0.0])                 # race probability 1
    if len(sizes) == 3:
        t[41, 6:8] = torch.tensor([1.0, 0.0])                       # age probability 1 beside a race probability below 1
    t[5::11] = -1
    preds, probs, bars, order = _host_inputs(EI, t, attrs)
    for s, k in enumerate(sizes):
        assert set(preds[s].tolist()) == set(range(-1, k)), (s, sorted(set(preds[s].tolist())))
    assert (bars == -1).any()
    p_d, m_d, b_d, o_d = E.grid_inputs_attrs(t.to(dev), attrs)
    assert p_d.dtype == b_d.dtype == o_d.dtype == torch.int32 and m_d.dtype == torch.float32 and p_d.is_cuda
    assert p_d.cpu().tolist() == preds.tolist() and torch.equal(m_d.cpu(), torch.from_numpy(probs))
    assert b_d.cpu().tolist() == bars.tolist() and o_d.cpu().tolist() == order.tolist()


def test_trainplot_kernels_with_bf16_library(dev):
    """The painter's tests again in a process that loads the bf16 library."""
    if os.environ.get("FD_DTYPE", "fp16").lower() in ("bf16", "bfloat16"):
        return          # this process already runs the bf16 library
    env = dict(os.environ, FD_DTYPE="bf16")
    env.pop("FAIRDIFF_LIB", None)
    r = subprocess.run([sys.executable, "-m", "pytest", "-q", "-m", "gpu", "-p", "no:cacheprovider", os.path.abspath(__file__), "-k", "eval_grid_attrs_img"],
                       env=env, capture_output=True, text=True, timeout=600, cwd=os.path.dirname(HERE))
    print(r.stdout[-4000:])
    print(r.stderr[-2000:])
    assert r.returncode == 0 and " passed" in r.stdout and "failed" not in r.stdout and "skipped" not in r.stdout
