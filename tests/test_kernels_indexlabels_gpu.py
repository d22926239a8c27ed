"""Direct tests of the index-text overlay ``fd_eval_grid_labels_u8`` (csrc/evaluate.hip) through ``ops.eval_grid_labels``: byte for byte against
its host statement (evaluation.labels_host, pinned to Pillow and to the reference's grids by tests/test_indexlabels_cpu.py) and against the
reference's own arrays on the output of each of the three painters, clipping, tiles that must get nothing, a descriptor table that points outside
the mask buffer (the kernel checks it and returns normally), and the host-side refusals.  The label masks come from the golden file: no font and
no FreeType is needed here."""
import ctypes
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
GOLD = os.path.join(HERE, "golden")
PAD = 4096          # bytes of 0xAB in front of and behind the grid
N, H, W = 5, 448, 384


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


@pytest.fixture(scope="module")
def G(dev):
    g = dict(np.load(os.path.join(GOLD, "reference_indexlabels_grid.npz")))
    b = int(g["block"])
    g["images"] = torch.from_numpy(g["blocks"]).repeat_interleave(b, dim=2).repeat_interleave(b, dim=3).contiguous()
    g["u8"] = torch.from_numpy(g["u8_blocks"]).repeat_interleave(b, dim=1).repeat_interleave(b, dim=2).contiguous()
    g["masks_d"], g["desc_d"] = torch.from_numpy(g["masks"]).to(dev), torch.from_numpy(g["desc"]).to(dev)
    return g


def i32(a, dev):
    return torch.as_tensor(np.asarray(a), dtype=torch.int32).to(dev).contiguous()


def paint(G, E, EI, ops, dev, name):
    """One of the three painters on the golden's inputs, into the middle of a 0xAB-filled buffer: (buffer, grid view, order, n_strip)."""
    pb, bx = G["probs"], i32(G["boxes"], dev)
    n = 1 if name == "grid1" else int(name[-1])
    shape = (2 * (H + 20), 3 * (W + 50 * n + 20), 3)
    nbytes = shape[0] * shape[1] * 3
    buf = torch.full((PAD + nbytes + PAD,), 0xAB, dtype=torch.uint8, device=dev)
    out = buf[PAD:PAD + nbytes].view(shape)
    if name == "grid1":
        pr = G["preds2"][0]
        order = E.grid_order(pr, pb[0])
        ops.eval_grid(G["images"].to(dev, ops.F16).contiguous(), i32(order, dev), bx, i32(pr, dev), torch.from_numpy(pb[0]).to(dev),
                      torch.tensor(E.PALETTE_GENDER, dtype=torch.uint8, device=dev), out=out)
        return buf, out, order, 1
    pr, p = G[f"preds{n}"], pb[:n]
    order = EI.grid_attrs_order(pr, p)
    bars = EI.grid_attrs_bar_rows(torch.from_numpy(p)).to(dev)
    pal = EI.PALETTES[:n]
    P = max(len(q) for q in pal)
    pal_t = torch.tensor([q + [(255, 255, 255)] * (P - len(q)) for q in pal], dtype=torch.uint8, device=dev)
    if name.startswith("u8"):
        ops.eval_grid_attrs(G["u8"].to(dev), i32(order, dev), bx, i32(pr, dev), bars, pal_t, out=out)
    else:
        ops.eval_grid_attrs_img(G["images"].to(dev, ops.F16).contiguous(), i32(order, dev), bx, i32(pr, dev), bars, pal_t, out=out)
    return buf, out, order, n


def around_is_untouched(buf):
    return bool((buf[:PAD] == 0xAB).all()) and bool((buf[-PAD:] == 0xAB).all())


@pytest.mark.parametrize("name", ["grid1", "grid2", "grid3", "u8_grid2", "u8_grid3"])
def test_labels_on_the_three_painters_equal_host_and_reference(dev, ops, E, EI, G, name):
    buf, grid, order, n = paint(G, E, EI, ops, dev, name)
    plain = grid.cpu().numpy()
    want = E.labels_host(plain, order, G["masks"], G["desc"], H, W, n, 3)
    got = ops.eval_grid_labels(grid, i32(order, dev), G["masks_d"], G["desc_d"], H, W, n)
    assert got is grid                                                        # in place
    got = got.cpu().numpy()
    assert around_is_untouched(buf), "bytes around the grid were written"
    bad = np.argwhere(got != want)
    assert len(bad) == 0 and (want != plain).any(), (name, len(bad), bad[:5].tolist())
    if name.startswith("u8") or ops.F16 == torch.float16:                     # the golden's pixel values are fp16 / bytes: the reference's own array
        assert np.array_equal(got, G[name]), (name, int((got != G[name]).sum()))


def test_unclipped_labels_leave_everything_outside_their_rectangle_untouched(dev, ops, E, G):
    Hh = Ww = 512
    for n, Nn in ((1, 3), (3, 2)):
        th, tw = Hh + 20, Ww + 50 * n + 20
        g = torch.Generator().manual_seed(5 + n)
        plain = torch.randint(0, 256, (th, Nn * tw, 3), generator=g, dtype=torch.int64).to(torch.uint8)
        order = np.arange(Nn)[::-1].copy()
        grid = plain.to(dev)
        ops.eval_grid_labels(grid, i32(order, dev), G["masks_d"], G["desc_d"], Hh, Ww, n)
        got, plain = grid.cpu().numpy(), plain.numpy()
        assert np.array_equal(got, E.labels_host(plain, order, G["masks"], G["desc"], Hh, Ww, n, Nn))
        outside = np.ones(got.shape[:2], dtype=bool)
        for t in range(Nn):
            w, h, ox, oy, _ = (int(v) for v in G["desc"][order[t]])
            assert 400 + ox + w <= Ww + 50 * n and 400 + oy + h <= Hh            # unclipped
            y0, x0 = 10 + 400 + oy, t * tw + 10 + 400 + ox
            outside[y0:y0 + h, x0:x0 + w] = False
            assert (got[y0:y0 + h, x0:x0 + w] != plain[y0:y0 + h, x0:x0 + w]).any()
        assert np.array_equal(got[outside], plain[outside])


def test_anchor_outside_the_tile_changes_nothing(dev, ops, G):
    Hh = Ww = 64
    plain = torch.randint(0, 256, (2 * 84, 3 * 184, 3), generator=torch.Generator().manual_seed(8), dtype=torch.int64).to(torch.uint8)
    grid = plain.to(dev)
    order = i32([4, 2, 0, 1, 3], dev)
    ops.eval_grid_labels(grid, order, G["masks_d"], G["desc_d"], Hh, Ww, 2)
    assert torch.equal(grid.cpu(), plain)
    for xy in ((164, 0), (0, 64), (-300, -300), (2 ** 31 - 1, 2 ** 31 - 1), (-2 ** 31, -2 ** 31)):      # just outside, and the int32 ends
        ops.eval_grid_labels(grid, order, G["masks_d"], G["desc_d"], Hh, Ww, 2, xy=xy)
        assert torch.equal(grid.cpu(), plain), xy


def test_many_tiles_and_multi_digit_labels_over_strips_and_bars(dev, ops, E, EI, G):
    """N = 130 tiles of 64 x 64 with three strips (an 11 x 12 grid, the last row partly filled) and the anchor at (12, -10): one-, two- and three-digit
    labels over strips, bars, outlines and image, clipped at the bottom and (three digits) on the right; then an anchor that clips at the left and
    at the top.  A row of -1 too."""
    Nn, Hh, Ww, n = 130, 64, 64, 3
    rng = np.random.RandomState(130)
    images = torch.from_numpy(rng.uniform(-1, 1, (Nn, 3, Hh, Ww)).astype(np.float32)).to(ops.F16)
    preds = np.stack([rng.randint(0, 2, Nn), rng.randint(0, 4, Nn), rng.randint(0, 2, Nn)])
    bars = rng.randint(-1, Hh + 20, (n, Nn))
    preds[:, 17] = -1
    boxes = np.stack([rng.randint(0, 30, Nn), rng.randint(0, 30, Nn), rng.randint(30, 64, Nn), rng.randint(30, 64, Nn)], axis=1)
    order = rng.permutation(Nn)
    pal = EI.PALETTES[:n]
    pal_t = torch.tensor([q + [(255, 255, 255)] * (5 - len(q)) for q in pal], dtype=torch.uint8, device=dev)
    grid = ops.eval_grid_attrs_img(images.to(dev).contiguous(), i32(order, dev), i32(boxes, dev), i32(preds, dev), i32(bars, dev), pal_t)
    rows, cols, shape = E.grid_attrs_shape(Nn, Hh, Ww, n)
    assert (rows, cols) == (11, 12) and tuple(grid.shape) == shape
    plain = grid.cpu().numpy()
    d = G["desc"]
    assert 12 + d[99, 0] <= 214 < 12 + d[100, 0] and -10 + d[0, 3] + d[0, 1] > Hh and -10 + d[0, 3] > 0
    want = E.labels_host(plain, order, G["masks"], d, Hh, Ww, n, cols, xy=(12, -10))
    ops.eval_grid_labels(grid, i32(order, dev), G["masks_d"], G["desc_d"], Hh, Ww, n, xy=(12, -10))
    got = grid.cpu().numpy()
    bad = np.argwhere(got != want)
    assert len(bad) == 0 and (want != plain).any(), (len(bad), bad[:5].tolist())
    # the frame and the white tiles past N are as the painter left them
    th, tw = Hh + 20, Ww + 50 * n + 20
    yy, xx = np.mgrid[0:shape[0], 0:shape[1]]
    frame = (yy % th < 10) | (yy % th >= th - 10) | (xx % tw < 10) | (xx % tw >= tw - 10) | ((yy // th) * cols + xx // tw >= Nn)
    assert np.array_equal(got[frame], plain[frame])
    # a negative anchor clips at the left and at the top
    grid2 = torch.from_numpy(plain).to(dev)
    ops.eval_grid_labels(grid2, i32(order, dev), G["masks_d"], G["desc_d"], Hh, Ww, n, xy=(-30, -40))
    assert np.array_equal(grid2.cpu().numpy(), E.labels_host(plain, order, G["masks"], d, Hh, Ww, n, cols, xy=(-30, -40)))


def test_a_bad_descriptor_or_order_entry_draws_nothing_on_its_tile(dev, ops, E, EI, G):
    """Argument checks of a bounded kernel: the table and the order are device memory the entry point cannot see, so the kernel checks every entry
    and skips the tile -- it returns normally, the tile keeps the painter's bytes and the other tiles get their labels."""
    buf, grid, order, n = paint(G, E, EI, ops, dev, "u8_grid2")
    plain = grid.cpu().numpy()
    plain_d = grid.clone()
    full = E.labels_host(plain, order, G["masks"], G["desc"], H, W, n, 3)
    th, tw = H + 20, W + 50 * n + 20
    nbytes = int(G["masks"].size)

    def run(order_, desc_, masks_d=None):
        g = plain_d.clone()
        ops.eval_grid_labels(g, i32(order_, dev), G["masks_d"] if masks_d is None else masks_d, i32(desc_, dev), H, W, n)
        torch.cuda.synchronize()
        return g.cpu().numpy()

    def only_tile_missing(got, t):
        r, c = divmod(t, 3)
        want = full.copy()
        want[r * th:(r + 1) * th, c * tw:(c + 1) * tw] = plain[r * th:(r + 1) * th, c * tw:(c + 1) * tw]
        return np.array_equal(got, want) and not np.array_equal(got, full)

    t = 2
    i = int(order[t])
    cases = {"zero w": (0, 0), "negative w": (0, -70), "zero h": (1, 0), "negative h": (1, -2 ** 31), "offset past the buffer": (4, nbytes - 10),
             "offset far past the buffer": (4, 2 ** 31 - 1), "negative offset": (4, -1), "w beyond the buffer": (0, 2 ** 31 - 1), "h beyond the buffer": (1, 2 ** 31 - 1)}
    for what, (col, val) in cases.items():
        d = G["desc"].copy()
        d[i, col] = val
        got = run(order, d)
        assert only_tile_missing(got, t), what
        assert np.array_equal(got, E.labels_host(plain, order, G["masks"], d, H, W, n, 3)), what
    # a label index the table does not hold: a table of i entries serves the images below i only
    i_hi = int(max(order))
    got = run(order, G["desc"][:i_hi])
    assert only_tile_missing(got, order.tolist().index(i_hi))
    # a mask buffer shorter than the table says: every label that reaches past its end is skipped, the others are drawn
    cut = int(G["desc"][2, 4]) + 100                                            # labels 0, 1 fit; 2, 3, 4 do not
    got = run(order, G["desc"][:N], masks_d=G["masks_d"][:cut].clone())
    assert np.array_equal(got, E.labels_host(plain, order, G["masks"][:cut], G["desc"][:N], H, W, n, 3)) and not np.array_equal(got, plain)
    # an order entry outside [0, N): the painters show such a tile white, the overlay leaves it alone
    for bad in (N, -1, 2 ** 31 - 1):
        o = order.copy()
        o[t] = bad
        assert only_tile_missing(run(o, G["desc"]), t), bad
    assert around_is_untouched(buf)


def test_labels_refuse_bad_arguments(dev, ops, G):
    from finetune_fair_diffusion_amd import lib
    Hh = Ww = 16
    shape = (2 * (Hh + 20), 3 * (Ww + 120), 3)
    out = torch.full((4 * (Hh + 20) * 4 * (Ww + 170) * 3,), 9, dtype=torch.uint8, device=dev)       # room for any of the refused shapes
    order = torch.zeros(N, dtype=torch.int32, device=dev)
    L = lib.get()
    stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    p = lambda t: t.data_ptr()
    good = [p(out), p(order), p(G["masks_d"]), p(G["desc_d"])]
    nb, nl = G["masks_d"].numel(), G["desc_d"].shape[0]
    call = lambda a, n=N, h=Hh, w=Ww, s=2, rows=2, cols=3, mb=nb, labels=nl: L.fd_eval_grid_labels_u8(a[0], a[1], a[2], mb, a[3], labels, n, h, w, s, rows, cols,
                                                                                                     0, 0, stream)
    refused = lambda rc: rc == -1 and b"fd_eval_grid_labels_u8" in L.fd_last_error()
    for k in range(4):                                              # each pointer in turn
        a = list(good)
        a[k] = None
        assert refused(call(a)) and b"null" in L.fd_last_error(), k
    for s in (0, 4):
        assert refused(call(good, s=s)) and b"n_strip" in L.fd_last_error()
    for n, h, w, rows, cols in ((0, Hh, Ww, 1, 1), (4097, Hh, Ww, 64, 65), (N, 0, Ww, 2, 3), (N, 4097, Ww, 2, 3), (N, Hh, 0, 2, 3), (N, Hh, 4097, 2, 3)):
        assert refused(call(good, n=n, h=h, w=w, rows=rows, cols=cols)) and b"supported 1..4096" in L.fd_last_error(), (n, h, w)
    for rows, cols in ((1, 4), (2, 2), (0, 5), (3, 3), (4, 2)):    # cannot hold N, or a whole row of empty tiles
        assert refused(call(good, rows=rows, cols=cols)) and b"does not hold" in L.fd_last_error(), (rows, cols)
    for labels in (0, -3):
        assert refused(call(good, labels=labels)) and b"n_labels" in L.fd_last_error()
    assert refused(call(good, mb=-1)) and b"mask_bytes" in L.fd_last_error()
    torch.cuda.synchronize()
    assert bool((out == 9).all())                                   # refused calls launched nothing
    # the wrapper refuses a grid that is not made of whole tiles of the stated geometry, and host or mistyped tables
    ok = out[:shape[0] * shape[1] * 3].view(shape)
    for bad in (ok[:-1], ok.view(-1), ok.to(torch.int8), ok[:, :-3]):
        with pytest.raises(AssertionError):
            ops.eval_grid_labels(bad, order, G["masks_d"], G["desc_d"], Hh, Ww, 2)
    with pytest.raises(AssertionError):
        ops.eval_grid_labels(ok, order, G["masks_d"], G["desc_d"], Hh, Ww, 3)
    with pytest.raises(AssertionError):
        ops.eval_grid_labels(ok, order.long(), G["masks_d"], G["desc_d"], Hh, Ww, 2)
    with pytest.raises(AssertionError):
        ops.eval_grid_labels(ok, order, G["masks_d"], G["desc_d"].view(-1), Hh, Ww, 2)
    with pytest.raises(AssertionError):
        ops.eval_grid_labels(ok, order, G["masks_d"].cpu(), G["desc_d"], Hh, Ww, 2)
    torch.cuda.synchronize()
    assert bool((out == 9).all())
    ops.eval_grid_labels(ok, order, G["masks_d"], G["desc_d"], Hh, Ww, 2, xy=(100, -30))      # label "0" on the five tiles, clipped to 16 x 16
    torch.cuda.synchronize()
    assert bool((out[ok.numel():] == 9).all()) and not bool((ok == 9).all())
