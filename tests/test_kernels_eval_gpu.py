"""Direct tests of the validation tail's two kernels (csrc/evaluate.hip) against their plain host statements (evaluation.tally_host /
grid_host, themselves pinned to the reference by tests/test_eval_cpu.py): integer counts and uint8 pixels, so every comparison is exact.
The module runs with whichever working dtype the process has; ``test_eval_kernels_with_bf16_library`` runs it again in a process that loads
the bf16 library."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
GOLD = os.path.join(HERE, "golden")


@pytest.fixture(scope="module")
def ops():
    from finetune_fair_diffusion_amd import ops
    return ops


@pytest.fixture(scope="module")
def E():
    from finetune_fair_diffusion_amd import evaluation
    return evaluation


def _attrs(sizes):
    out, c = [], 0
    for k in sizes:
        out.append((c, k))
        c += k
    return out


def test_eval_tally_matches_host_on_golden_tables(dev, ops, E):
    cases = json.load(open(os.path.join(GOLD, "reference_eval_metrics.json")))["cases"]
    assert len(cases) >= 100
    for c in cases:
        t = torch.tensor(c["probs"], dtype=torch.float32)
        attrs = _attrs(c["sizes"])
        got = ops.eval_tally(t.to(dev), attrs).cpu()
        ref = E.tally_host(t, attrs)
        assert torch.equal(got, ref), (c["experiment"], c["table"], c["N"], got.tolist(), ref.tolist())
        m, want = E.gap_metrics(c["experiment"], got), c["metrics"]
        for k, v in want.items():
            assert m[k] == v or (v != v and m[k] != m[k]), (c["experiment"], c["table"], c["N"], k, m[k], v)


@pytest.mark.parametrize("sizes", [[2], [4], [2, 4], [2, 4, 2]])
def test_eval_tally_matches_host_on_65536_random_rows(dev, ops, E, sizes):
    g = torch.Generator().manual_seed(4100 + sum(sizes))
    N = 1 << 16
    t = torch.cat([torch.softmax(torch.randn(N, k, generator=g) * 1.5, dim=-1) for k in sizes], dim=1)
    t[5::97, :sizes[0]] = 1.0 / sizes[0]                      # ties
    if sizes[0] == 2:
        for j, v in enumerate((0.2, 0.5, 0.8)):               # rows exactly at the fp32 value of each threshold
            t[7 + j::101, 1] = v
            t[7 + j::101, 0] = 1 - v
    t[torch.rand(N, generator=g) < 0.1] = -1                  # no face: every attribute of the row
    # a wider table with a row stride: the attributes sit in the first columns of a [N, K + 3] buffer
    wide = torch.full((N, sum(sizes) + 3), 0.123)
    wide[:, :sum(sizes)] = t
    ref = E.tally_host(t, _attrs(sizes))
    assert int(ref[0]) > 50000
    assert torch.equal(ops.eval_tally(t.to(dev), _attrs(sizes)).cpu(), ref)
    assert torch.equal(ops.eval_tally(wide.to(dev)[:, :sum(sizes)], _attrs(sizes)).cpu(), ref)


def test_eval_tally_writes_every_count_and_nothing_else(dev, ops, E):
    """The kernel zeroes what it does not count (a dirty output buffer does not leak), and writes 32 entries only."""
    from finetune_fair_diffusion_amd import lib
    import ctypes
    t = torch.tensor([[0.3, 0.7], [-1.0, -1.0], [0.9, 0.1]], device=dev)
    buf = torch.full((40,), 77, dtype=torch.int32, device=dev)
    rc = lib.get().fd_eval_tally(t.data_ptr(), 3, 2, (ctypes.c_int32 * 1)(0), (ctypes.c_int32 * 1)(2), 1, buf.data_ptr(),
                                 ctypes.c_void_p(torch.cuda.current_stream().cuda_stream))
    assert rc == 0
    torch.cuda.synchronize()
    assert torch.equal(buf[:32].cpu(), E.tally_host(t.cpu(), [(0, 2)])) and bool((buf[32:] == 77).all())


def test_eval_tally_refuses_bad_arguments(dev, ops):
    t = torch.rand(8, 6, device=dev)
    for attrs in ([], [(0, 2)] * 4, [(0, 5)], [(0, 0)], [(5, 2)], [(-1, 2)]):
        with pytest.raises(RuntimeError, match="fd_eval_tally"):
            ops.eval_tally(t, attrs)
    from finetune_fair_diffusion_amd import lib
    import ctypes
    buf = torch.full((32,), 5, dtype=torch.int32, device=dev)
    rc = lib.get().fd_eval_tally(t.data_ptr(), (1 << 20) + 1, 6, (ctypes.c_int32 * 1)(0), (ctypes.c_int32 * 1)(2), 1, buf.data_ptr(),
                                 ctypes.c_void_p(torch.cuda.current_stream().cuda_stream))
    torch.cuda.synchronize()
    assert rc != 0 and b"2^20" in lib.get().fd_last_error() and bool((buf == 5).all())          # refused: nothing was launched


def _grid_case(E, ops, dev, images, boxes, preds, maxprob, palette, n_classes=2):
    N, _, H, W = images.shape
    order = E.grid_order(preds, maxprob, n_classes)
    imgs_wd = torch.as_tensor(images).to(ops.F16)              # what the device holds (bf16 rounds the fp16 goldens once more)
    ref = E.grid_host(imgs_wd, order, boxes, preds, maxprob, palette)
    rows, cols, shape = E.grid_shape(N, H, W)
    nbytes = shape[0] * shape[1] * shape[2]
    buf = torch.full((nbytes + 64,), 0xA5, dtype=torch.uint8, device=dev)
    i32 = lambda a: torch.as_tensor(np.asarray(a), dtype=torch.int32).to(dev).contiguous()
    out = ops.eval_grid(imgs_wd.to(dev).contiguous(), i32(order), i32(boxes), i32(preds), torch.as_tensor(np.asarray(maxprob), dtype=torch.float32).to(dev),
                        torch.tensor(palette, dtype=torch.uint8, device=dev), out=buf[:nbytes].view(shape))
    got = out.cpu().numpy()
    assert bool((buf[nbytes:] == 0xA5).all()), "bytes behind the grid were written"
    bad = np.argwhere(got != ref)
    assert got.shape == ref.shape and len(bad) == 0, (len(bad), bad[:5].tolist())
    return got, imgs_wd


def test_eval_grid_matches_host_and_reference_at_64(dev, ops, E):
    g = np.load(os.path.join(GOLD, "reference_eval_grid.npz"))
    for case in "ab":
        im, bx, pr, mp = (g[f"{case}_{n}"] for n in ("images", "boxes", "preds", "maxprob"))
        got, wd = _grid_case(E, ops, dev, torch.from_numpy(im), bx, pr, mp, E.PALETTE_GENDER)
        if ops.F16 == torch.float16:        # the goldens' pixel values are fp16: the fp16 library reproduces the reference's own array
            assert np.array_equal(got, g[f"{case}_grid"])


@pytest.mark.parametrize("N", [8, 24, 25])
def test_eval_grid_matches_host_at_512(dev, ops, E, N):
    rng = np.random.RandomState(50 + N)
    H = W = 512
    images = torch.from_numpy(rng.uniform(-1, 1, (N, 3, H, W)).astype(np.float32)).clamp(-1, 1)
    images[0, :, :8] = 1.0
    images[0, :, 8:16] = -1.0
    n_classes = 4 if N == 24 else 2
    preds = rng.randint(0, n_classes, N)
    maxprob = rng.uniform(1.0 / n_classes, 1.0, N).astype(np.float32)
    maxprob[1] = 1.0
    boxes = np.zeros((N, 4), dtype=np.int64)
    for i in range(N):
        x0, y0 = rng.randint(0, 250, 2)
        boxes[i] = [x0, y0, x0 + rng.randint(100, 262), y0 + rng.randint(100, 262)]
    boxes[0] = [0, 0, 511, 511]
    boxes[1] = [-40, 30, 300, 560]
    boxes[2] = [200, 200, 203, 260]                           # narrower than two outline widths
    for i in (3, N - 1):
        preds[i], maxprob[i], boxes[i] = -1, -1.0, -1
    _grid_case(E, ops, dev, images, boxes, preds, maxprob, E.PALETTE_RACE if n_classes == 4 else E.PALETTE_GENDER, n_classes)


def test_eval_grid_refuses_bad_arguments(dev, ops):
    import ctypes
    from finetune_fair_diffusion_amd import lib
    N, H, W = 5, 16, 16
    img = torch.zeros((N, 3, H, W), dtype=ops.F16, device=dev)
    z = torch.zeros(N, dtype=torch.int32, device=dev)
    bx = torch.zeros((N, 4), dtype=torch.int32, device=dev)
    mp = torch.ones(N, device=dev)
    pal = torch.zeros((6, 3), dtype=torch.uint8, device=dev)
    out = torch.full((4 * (H + 20) * 4 * (W + 70) * 3 + 8,), 9, dtype=torch.uint8, device=dev)        # room for any of the refused shapes
    L = lib.get()
    stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    call = lambda grid_ptr, n, rows, cols: L.fd_eval_grid_u8(img.data_ptr(), z.data_ptr(), bx.data_ptr(), z.data_ptr(), mp.data_ptr(), pal.data_ptr(), grid_ptr,
                                                             n, H, W, rows, cols, stream)
    for rows, cols in ((1, 4), (2, 2), (0, 5), (3, 3), (4, 2)):        # too small, or a whole row of empty tiles
        assert call(out.data_ptr(), N, rows, cols) != 0 and b"fd_eval_grid_u8" in L.fd_last_error(), (rows, cols)
    assert call(out.data_ptr(), 0, 1, 1) != 0 and call(out.data_ptr(), 4097, 64, 65) != 0
    assert call(out.data_ptr() + 1, N, 2, 3) != 0 and b"aligned" in L.fd_last_error()
    assert call(None, N, 2, 3) != 0 and b"null" in L.fd_last_error()
    torch.cuda.synchronize()
    assert bool((out == 9).all())                                   # refused calls launched nothing
    # the wrapper refuses an output buffer that is not exactly the grid: the entry point cannot see its size
    good = out[:2 * (H + 20) * 3 * (W + 70) * 3].view(2 * (H + 20), 3 * (W + 70), 3)
    for bad in (good[:-1], good.view(-1), good.to(torch.int8), good.transpose(0, 1)):
        with pytest.raises(AssertionError):
            ops.eval_grid(img, z, bx, z, mp, pal, out=bad)
    assert bool((out == 9).all())
    ops.eval_grid(img, z, bx, z, mp, pal, out=good)
    torch.cuda.synchronize()
    assert bool((out[good.numel():] == 9).all()) and not bool((good == 9).all())


def test_eval_kernels_with_bf16_library(dev):
    if os.environ.get("FD_DTYPE", "fp16").lower() in ("bf16", "bfloat16"):
        return          # this process already runs the bf16 library
    env = dict(os.environ, FD_DTYPE="bf16")
    env.pop("FAIRDIFF_LIB", None)
    r = subprocess.run([sys.executable, "-m", "pytest", "-q", "-m", "gpu", "-p", "no:cacheprovider", os.path.abspath(__file__), "-k", "not bf16_library"],
                       env=env, capture_output=True, text=True, timeout=900, cwd=os.path.dirname(HERE))
    print(r.stdout[-4000:])
    print(r.stderr[-2000:])
    assert r.returncode == 0 and " passed" in r.stdout and "failed" not in r.stdout and "skipped" not in r.stdout
