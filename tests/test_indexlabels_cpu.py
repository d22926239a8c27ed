"""Host layer of the index text on the annotated grids (no GPU): the numpy statement ``evaluation.labels_host`` on top of the three label-free
host statements against the grids the reference's plot functions recorded with their ``text`` call live (tests/golden/make_golden_indexlabels.py),
against Pillow's ``ImageDraw.text`` directly where FreeType and a font are present, the blend formula, the label atlas, the flags and the new
C-ABI entry point."""
import glob
import os

import numpy as np
import pytest
import torch

from finetune_fair_diffusion_amd import cli, evaluate_images as EI, evaluation as E, lib, train  # noqa: F401

HERE = os.path.dirname(os.path.abspath(__file__))
GOLD = os.path.join(HERE, "golden")
PATH = os.path.join(GOLD, "reference_indexlabels_grid.npz")
N, H, W = 5, 448, 384


@pytest.fixture(scope="module")
def G():
    g = dict(np.load(PATH))
    b = int(g["block"])
    g["images"] = torch.from_numpy(g["blocks"]).repeat_interleave(b, dim=2).repeat_interleave(b, dim=3).contiguous()
    g["u8"] = np.ascontiguousarray(g["u8_blocks"].repeat(b, axis=1).repeat(b, axis=2))
    return g


def label_free(G, name):
    """(label-free host grid, order, n_strip) of golden grid ``name`` from the host statements the painters are pinned to."""
    pb, bx = G["probs"], G["boxes"]
    if name == "grid1":
        pr = G["preds2"][0]
        order = E.grid_order(pr, pb[0])
        return E.grid_host(G["images"], order, bx, pr, pb[0], E.PALETTE_GENDER), order, 1
    n = int(name[-1])
    pr, p = G[f"preds{n}"], pb[:n]
    order = EI.grid_attrs_order(pr, p)
    bars = EI.grid_attrs_bar_rows(torch.from_numpy(p)).numpy()
    host = EI.grid_attrs_host(G["u8"], order, bx, pr, bars, EI.PALETTES[:n]) if name.startswith("u8") else \
        E.grid_attrs_img_host(G["images"], order, bx, pr, bars, EI.PALETTES[:n])
    return host, order, n


def find_font():
    cands = glob.glob("/usr/share/fonts/**/DejaVuSans-Bold.ttf", recursive=True)
    try:
        import matplotlib
        cands.append(os.path.join(matplotlib.get_data_path(), "fonts", "ttf", "DejaVuSans-Bold.ttf"))
    except Exception:
        pass
    return next((c for c in cands if os.path.isfile(c)), None)


def have_freetype():
    try:
        from PIL import features
        return bool(features.check("freetype2"))
    except Exception:
        return False


def test_golden_holds_what_it_claims():
    g = np.load(PATH)
    assert os.path.getsize(PATH) < 1024 * 1024
    assert g["blocks"].shape == (N, 3, H // 16, W // 16) and g["blocks"].dtype == np.float16 and g["u8_blocks"].dtype == np.uint8
    for n, name in ((1, "grid1"), (2, "grid2"), (3, "grid3"), (2, "u8_grid2"), (3, "u8_grid3")):
        assert g[name].shape == (2 * (H + 20), 3 * (W + 50 * n + 20), 3) and g[name].dtype == np.uint8
        assert (g[name][H + 20:, -(W + 50 * n + 20):] == 255).all()                       # the sixth tile is white: no label there
    d = g["desc"]
    assert d.shape == (130, 5) and d.dtype == np.int32 and g["masks"].dtype == np.uint8
    assert int(d[-1, 4]) + int(d[-1, 0]) * int(d[-1, 1]) == g["masks"].size and (np.diff(d[:, 4]) == d[:-1, 0] * d[:-1, 1]).all()
    # a whole string is not its digits side by side: "17" against "1" + "7"
    assert d[17, 0] != d[1, 0] + d[7, 0]
    # one digit clips on the right at one strip only, two digits at every width, and everything clips at the bottom
    assert 434 < 400 + d[0, 2] + d[0, 0] <= 484 and 400 + d[17, 2] + d[17, 0] > 534 and (400 + d[:, 3] + d[:, 1] > H).all()
    assert (g["preds3"][:, 3] == -1).all() and g["probs"][0, 0] == g["probs"][0, 1] and g["probs"][1, 0] == g["probs"][1, 1]
    # a box outline lies under the label: row 0's bottom edge, rows 427..430 of the image, columns 100..360
    assert g["boxes"][0].tolist() == [100, 50, 360, 430]


@pytest.mark.parametrize("name", ["grid1", "grid2", "grid3", "u8_grid2", "u8_grid3"])
def test_labels_host_on_the_label_free_host_grids_equals_the_reference(G, name):
    host, order, n = label_free(G, name)
    ref = G[name]
    assert host.shape == ref.shape and not np.array_equal(host, ref)                       # the text is what is missing
    out = E.labels_host(host, order, G["masks"], G["desc"], H, W, n, 3)
    assert out.dtype == np.uint8 and np.array_equal(out, ref), (name, int((out != ref).sum()))
    # only label rectangles changed, clipped to the inner area: per tile, columns from 400 + off_x and rows from 400 + off_y
    diff = np.argwhere((out != host).any(axis=2))
    th, tw = H + 20, W + 50 * n + 20
    ty, tx = diff[:, 0] % th - 10, diff[:, 1] % tw - 10
    assert len(diff) and ty.min() >= 400 + G["desc"][:N, 3].min() and ty.max() < H and tx.min() >= 400 and tx.max() < W + 50 * n
    # the outline under the text was blended, not replaced: tile 0 shows image 0 (the tie in index order) with its bottom edge at rows 427..430
    assert order.tolist()[:2] == [0, 1] and order.tolist()[-1] == 3


def test_labels_host_draws_nothing_for_tiles_it_must_skip(G):
    host, order, n = label_free(G, "grid2")
    d = G["desc"].copy()
    bad_order = order.copy()
    bad_order[1] = 7                                                                       # outside [0, N): a white tile in the painters, no text here
    a = E.labels_host(host, bad_order, G["masks"], d, H, W, n, 3)
    full = E.labels_host(host, order, G["masks"], d, H, W, n, 3)
    th, tw = H + 20, W + 50 * n + 20
    want = full.copy()
    want[:th, tw:2 * tw] = host[:th, tw:2 * tw]                                             # tile 1 keeps the painter's bytes, the others their labels
    assert np.array_equal(a, want) and not np.array_equal(a, full)
    for col, val in ((0, 0), (1, -3), (4, G["masks"].size), (4, -1)):                      # zero w, negative h, offset past the buffer, negative offset
        d2 = d.copy()
        d2[order[0], col] = val
        b = E.labels_host(host, order, G["masks"], d2, H, W, n, 3)
        assert np.array_equal(b[:H + 20, :tw], host[:H + 20, :tw]) and np.array_equal(b[:, tw:], full[:, tw:]), (col, val)
    assert np.array_equal(E.labels_host(host, order, G["masks"], d[:2], H, W, n, 3)[:, 2 * tw:], host[:, 2 * tw:])      # a table of two labels
    assert np.array_equal(E.labels_host(host, order, G["masks"], d, H, W, n, 3, xy=(W + 50 * n, 0)), host)              # anchor outside the tile
    assert np.array_equal(E.labels_host(host, order, G["masks"], d, H, W, n, 3, xy=(-500, -500)), host)


def test_blend_is_the_identity_at_zero_and_white_at_full_coverage():
    a = np.arange(256)
    assert np.array_equal(E.label_blend(a, 0), a) and (E.label_blend(a, 255) == 255).all()
    # in between: PIL's rounding of (a*(255-m) + 255*m) / 255, monotonic in both arguments
    m = np.arange(256)[:, None]
    t = E.label_blend(a[None, :], m).astype(np.int64)
    exact = (a[None, :] * (255 - m) + 255 * m) / 255.0
    assert (np.abs(t - exact) <= 0.5 + 1e-9).all() and (np.diff(t, axis=0) >= 0).all() and (np.diff(t, axis=1) >= 0).all()


@pytest.mark.skipif(not have_freetype() or find_font() is None, reason="needs a Pillow with FreeType and DejaVuSans-Bold.ttf")
def test_atlas_reproduces_the_golden_masks_and_labels_host_equals_imagedraw_text(G):
    import PIL
    from PIL import Image, ImageDraw, ImageFont
    font = find_font()
    L = E.IndexLabels(font, 100)
    masks, desc = L.atlas(130, "cpu")
    assert masks.dtype == torch.uint8 and desc.dtype == torch.int32 and tuple(desc.shape) == (130, 5)
    assert L.atlas(130, "cpu")[0] is masks                                                  # cached per (n, device)
    small = L.atlas(12, "cpu")
    assert tuple(small[1].shape) == (12, 5) and torch.equal(small[1], desc[:12]) and torch.equal(small[0], masks[:small[0].numel()])
    if PIL.__version__ == str(G["pillow"]) and " ".join(ImageFont.truetype(font, 100).getname()) == str(G["font"]):
        assert np.array_equal(desc.numpy(), G["desc"]) and np.array_equal(masks.numpy(), G["masks"])
    # independently of the golden: a table of five strings as labels 0..4 on random backgrounds, each tile against ImageDraw.text on its inner area
    texts = ["0", "7", "17", "128", "1023"]
    rast = [L.raster(s) for s in texts]
    offs = np.cumsum([0] + [m.size for m, _ in rast])
    tdesc = np.array([d + (int(o),) for (_, d), o in zip(rast, offs)], dtype=np.int32)
    tmasks = np.concatenate([m.reshape(-1) for m, _ in rast])
    assert tdesc[2, 0] == 139 and tdesc[1, 0] == 70                                         # DejaVuSans-Bold at 100: "17" is not 2 x 70 wide
    f = ImageFont.truetype(font, 100)
    rng = np.random.default_rng(41)
    for Wt, n in ((384, 1), (512, 3)):                                                      # inner widths 434 and 662
        IW, th, tw = Wt + 50 * n, H + 20, Wt + 50 * n + 20
        grid = rng.integers(0, 256, (2 * th, 3 * tw, 3), dtype=np.uint8)
        order = np.array([3, 0, 4, 1, 2], dtype=np.int32)
        out = E.labels_host(grid, order, tmasks, tdesc, H, Wt, n, 3)
        want = grid.copy()
        for t in range(5):
            r, c = divmod(t, 3)
            inner = want[r * th + 10:r * th + 10 + H, c * tw + 10:c * tw + 10 + IW]
            im = Image.fromarray(inner.copy())
            ImageDraw.Draw(im).text((400, 400), texts[order[t]], align="left", font=f)
            inner[...] = np.asarray(im)
        assert np.array_equal(out, want), (IW, int((out != want).sum()))
        assert (out != grid).any()


def test_index_labels_refuses_a_missing_font_and_a_pillow_without_freetype(monkeypatch, tmp_path):
    if have_freetype():
        with pytest.raises(FileNotFoundError, match="is not a file"):
            E.IndexLabels(str(tmp_path / "no-such-font.ttf"))
        with pytest.raises(ValueError, match="at least 1"):
            E.IndexLabels("default", 0)
    from PIL import features
    monkeypatch.setattr(features, "check", lambda name: False)
    with pytest.raises(RuntimeError, match="FreeType"):
        E.IndexLabels("default")


@pytest.mark.skipif(not have_freetype(), reason="needs a Pillow with FreeType")
def test_default_font_gives_a_scalable_atlas():
    a, b = E.IndexLabels("default", 100).host(11), E.IndexLabels("default", 40).host(11)
    assert a[1][10, 0] > a[1][1, 0] > b[1][1, 0] > 0 and a[0].size > b[0].size


def test_no_flag_means_no_font_and_no_new_launch(monkeypatch):
    d = cli.parse_args([], with_extras=True)
    assert d.index_font is None and d.index_font_size == 100
    assert cli.EXTRA_DEFAULTS["index_font"] is None and cli.EXTRA_DEFAULTS["index_font_size"] == 100
    a = cli.parse_args(["--index_font", "default", "--index_font_size", "60"], with_extras=True, experiment="exp-4")
    assert a.index_font == "default" and a.index_font_size == 60
    assert "--index_font" in cli.__doc__ and "--index_font" in train.__doc__ and "--index_font" in EI.__doc__
    e = EI.parse_args([])
    assert not hasattr(e, "index_font") and not hasattr(e, "index_font_size")               # the evaluator's arguments are what they were
    e = EI.parse_args(["--index_font", "/some/font.ttf"])
    assert e.index_font == "/some/font.ttf" and not hasattr(e, "index_font_size")
    # the grid helpers with labels=None: the painter's result is returned as it is and the overlay is never reached
    from finetune_fair_diffusion_amd import ops
    calls = []
    sentinel = torch.zeros(3, dtype=torch.uint8)
    monkeypatch.setattr(ops, "eval_grid_labels", lambda *a, **k: calls.append("labels"))
    for name in ("eval_grid", "eval_grid_attrs", "eval_grid_attrs_img"):
        monkeypatch.setattr(ops, name, lambda *a, _n=name, **k: (calls.append(_n), sentinel)[1])
    Nn = 4
    pd = torch.softmax(torch.randn(Nn, 8, generator=torch.Generator().manual_seed(3)), dim=-1)
    images, boxes = torch.zeros(Nn, 3, 8, 8), torch.zeros(Nn, 4, dtype=torch.int32)

    class Tr:
        attrs = [("gender", 0, 2)]
    assert E.device_grid(Tr, images, boxes, pd[:, :2].contiguous()) is sentinel
    Tr.attrs = [("gender", 0, 2), ("race", 2, 4), ("age", 6, 2)]
    assert E.device_grid_attrs(Tr, images, boxes, pd) is sentinel
    probs = [pd[:, :2], pd[:, 2:6], pd[:, 6:]]
    assert EI.device_grid(torch.zeros(Nn, 8, 8, 3, dtype=torch.uint8), boxes, probs, "gender_race") is sentinel
    assert calls == ["eval_grid", "eval_grid_attrs_img", "eval_grid_attrs"]
    # and with labels the overlay follows the painter directly, with the painter's order and geometry

    class Labels:
        def atlas(self, n, device):
            calls.append(("atlas", n))
            return "masks", "desc"
    got = []
    monkeypatch.setattr(ops, "eval_grid_labels", lambda grid, order, masks, desc, H, W, n_strip, xy=(400, 400): (got.append((masks, desc, H, W, n_strip, xy,
                                                                                                                       order.tolist())), grid)[1])
    del calls[:]
    assert E.device_grid_attrs(Tr, images, boxes, pd, labels=Labels()) is sentinel
    assert calls == ["eval_grid_attrs_img", ("atlas", Nn)] and got[0][:6] == ("masks", "desc", 8, 8, 3, (400, 400)) and sorted(got[0][6]) == list(range(Nn))


def test_new_entry_point_is_declared_additively():
    protos = lib.parse_header()
    assert len(protos["fd_eval_grid_labels_u8"][1]) == 15 and lib.ABI_VERSION == 4
    import ctypes
    assert protos["fd_eval_grid_labels_u8"][1][3] is ctypes.c_int64 and protos["fd_eval_grid_labels_u8"][1][:3] == [ctypes.c_void_p] * 3
    assert list(protos)[-1] == "fd_eval_grid_labels_u8"                                     # appended to the header
    md = open(os.path.join(os.path.dirname(HERE), "INTEGRATION.md")).read()
    row = [l for l in md.splitlines() if l.startswith("| `fd_eval_grid_labels_u8` |")]
    assert len(row) == 1 and "15 arguments" in row[0]
    if os.path.exists(lib.LIB_PATH):
        L = lib.load()
        assert L.fd_eval_grid_labels_u8 and L.fd_version() == 4
