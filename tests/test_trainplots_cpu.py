"""Host layer of the training monitor (no GPU): the numpy statement of ``fd_eval_grid_attrs`` and the tile order against the grids the reference's
training-side plot functions recorded (tests/golden/make_golden_trainplots.py), the offline statement it shares its tile painter with, the two
flags, the new C-ABI entry point and the plot-step rule."""
import os

import numpy as np
import pytest
import torch

from finetune_fair_diffusion_amd import cli, evaluate_images as EI, evaluation as E, lib, train

HERE = os.path.dirname(os.path.abspath(__file__))
GOLD = os.path.join(HERE, "golden")


def test_grid_attrs_img_host_and_order_equal_the_reference_train_plots_byte_for_byte():
    path = os.path.join(GOLD, "reference_trainplot_grid.npz")
    g = np.load(path)
    assert os.path.getsize(path) < 200 * 1024
    im, bx, pb = g["images"], g["boxes"], g["probs"]
    assert im.shape == (5, 3, 64, 64) and im.dtype == np.float16 and float(np.abs(im.astype(np.float32)).max()) == 1.0
    # what the golden claims to hold: every class over the two tables, a -1 row, p = 1, a bar inside the tile and clipped ones, boxes on and over the border
    assert set(g["preds2"][0]) == {-1, 0, 1} and set(g["preds2"][1]) | set(g["preds3"][1]) == {-1, 0, 1, 2, 3} and set(g["preds3"][2]) == {-1, 0, 1}
    assert (pb == 1).any() and (pb == np.float32(0.96875)).any() and ((pb < 0.875) & (pb > 0)).any()
    assert bx[0].tolist() == [0, 0, 63, 63] and bx[1, 0] < 0 and bx[1, 3] > 63 and bx[3].tolist() == [-1] * 4
    # rows 0 and 1 tie inside one group, and the pixel probes (exact value within one fp32 ulp of an integer) are in image 0
    assert pb[0, 0] == pb[0, 1] and pb[1, 0] == pb[1, 1] and (g["preds3"][:, 0] == g["preds3"][:, 1]).all()
    assert {np.float16(0.0039215087890625), np.float16(-0.0039215087890625)} <= set(im[0].reshape(-1).tolist())
    for n_attr in (2, 3):
        pr, p = g[f"preds{n_attr}"], pb[:n_attr]
        ref = g[f"grid{n_attr}"]
        order = EI.grid_attrs_order(pr, p)
        assert order.tolist()[:2] == [0, 1] and order.tolist()[-1] == 3                    # the tie in index order, the -1 row last
        assert EI.device_order(torch.from_numpy(pr).long(), torch.from_numpy(p)).tolist() == order.tolist()
        bars = EI.grid_attrs_bar_rows(torch.from_numpy(p)).numpy()
        out = E.grid_attrs_img_host(torch.from_numpy(im), order, bx, pr, bars, EI.PALETTES[:n_attr])
        assert out.dtype == np.uint8 and out.shape == ref.shape == E.grid_attrs_shape(5, 64, 64, n_attr)[2]
        assert np.array_equal(out, ref), (n_attr, int((out != ref).sum()))
        assert (ref[84:, -(64 + 50 * n_attr + 20):] == 255).all()                           # the sixth tile is white
    # the age bar's quirk is in the golden: row 2 (race probability 1, age probability 0.75) has NO age bar, row 1 (age 1, race 0.75) one of one row
    bars3 = EI.grid_attrs_bar_rows(torch.from_numpy(pb)).tolist()
    assert bars3[2][2] == -1 and bars3[2][1] == 0


def test_host_statement_orders_a_tie_by_index_whatever_the_reference_does():
    """The tie rule on its own (the golden can only hold it where the reference's argsort happens to agree): equal confidences keep the index order
    in the host rule and in the device rule, and the painted grid follows the order it is given."""
    preds = np.array([[1, 1, 1, 0], [2, 2, 2, 0]])
    probs = np.float32([[0.5, 0.5, 0.5, 0.5], [0.75, 0.875, 0.75, 0.75]])
    assert EI.grid_attrs_order(preds, probs).tolist() == [1, 0, 2, 3]
    assert EI.device_order(torch.from_numpy(preds).long(), torch.from_numpy(probs)).tolist() == [1, 0, 2, 3]
    im = torch.linspace(-1, 1, 4).view(4, 1, 1, 1).expand(4, 3, 8, 8).contiguous()
    bars = EI.grid_attrs_bar_rows(torch.from_numpy(probs)).numpy()
    a = E.grid_attrs_img_host(im, [1, 0, 2, 3], np.full((4, 4), -100), preds, bars, EI.PALETTES[:2])
    b = E.grid_attrs_img_host(im, [0, 1, 2, 3], np.full((4, 4), -100), preds, bars, EI.PALETTES[:2])
    assert a.shape == (2 * 28, 2 * 128, 3) and not np.array_equal(a, b) and np.array_equal(a[:28, 128:], b[:28, :128])


def test_grid_attrs_host_is_unchanged():
    """The offline statement now shares ``evaluation.paint_attrs_tiles``: its results are still the reference's arrays."""
    g = np.load(os.path.join(GOLD, "reference_evalimages_grid.npz"))
    for case in "ab":
        for n_attr in (2, 3):
            pr, pb = g[f"{case}_preds"][:n_attr], g[f"{case}_probs"][:n_attr]
            bars = EI.grid_attrs_bar_rows(torch.from_numpy(pb)).numpy()
            out = EI.grid_attrs_host(g[f"{case}_images"], EI.grid_attrs_order(pr, pb), g[f"{case}_boxes"], pr, bars, EI.PALETTES[:n_attr])
            assert np.array_equal(out, g[f"{case}_grid{n_attr}"]), (case, n_attr)
    assert EI.grid_attrs_shape is E.grid_attrs_shape


def test_pixel_rule_is_grid_hosts():
    """Every fp16 value in [-1,1] through both statements' pixel rule: the same bytes, and the truncation of the exact value."""
    bits = np.arange(1 << 16, dtype=np.uint16).view(np.float16)
    x = bits[np.isfinite(bits) & (np.abs(bits) <= 1)]
    n = len(x)
    im = torch.from_numpy(np.resize(x, (1, 3, 1, n)).copy())
    z = np.zeros((1, 1), dtype=np.int32)
    far = np.full((1, 4), -100)
    one = E.grid_host(im, [0], far, [0], np.float32([1.0]), E.PALETTE_GENDER)[10, 60:60 + n]
    two = E.grid_attrs_img_host(im, [0], far, z, z - 1, EI.PALETTES[:1])[10, 60:60 + n]
    assert np.array_equal(one, two)
    exact = np.floor((im[0, :, 0].double().numpy().T * 0.5 + 0.5) * 255).astype(np.uint8)
    assert np.array_equal(two, exact)


def test_flags():
    a = cli.parse_args(["--train_monitor", "plots", "--validation", "grids_attrs"], with_extras=True)
    assert a.train_monitor == "plots" and a.validation == "grids_attrs"
    assert cli.parse_args(["--train_monitor", "metrics"], with_extras=True, experiment="exp-4").train_monitor == "metrics"
    for bad in (["--train_monitor", "grids"], ["--train_monitor", "on"], ["--validation", "attrs"]):
        with pytest.raises(SystemExit):
            cli.parse_args(bad, with_extras=True)
    d = cli.parse_args([], with_extras=True)
    assert d.train_monitor == "off" and d.validation == "off" and d.train_plot_every_n_iter == 20
    assert cli.EXTRA_DEFAULTS["train_monitor"] == "off" and cli.EXTRA_DEFAULTS["validation"] == "off"
    assert "--train_monitor" in cli.__doc__ and "grids_attrs" in cli.__doc__
    assert train.evaluation_due("grids_attrs", 0, 5) and train.evaluation_due("grids_attrs", 10, 5) and not train.evaluation_due("grids_attrs", 3, 5)


def test_new_entry_point_is_declared_additively():
    protos = lib.parse_header()
    assert len(protos["fd_eval_grid_attrs"][1]) == 14 and protos["fd_eval_grid_attrs"] == protos["fd_eval_grid_attrs_u8"]
    assert lib.ABI_VERSION == 4
    md = open(os.path.join(os.path.dirname(HERE), "INTEGRATION.md")).read()
    row = [l for l in md.splitlines() if l.startswith("| `fd_eval_grid_attrs` |")]
    assert len(row) == 1 and "14 arguments" in row[0]
    if os.path.exists(lib.LIB_PATH):
        L = lib.load()
        assert L.fd_eval_grid_attrs and L.fd_version() == 4


def test_plot_step_rule_gives_the_reference_file_numbers():
    """Two epochs of five steps, a plot every two steps of an EPOCH: the reference tests the index inside the epoch and names the file by the
    global step before its increment -- 0, 2, 4, then 5, 7, 9 (not 6, 8)."""
    plan = [(epoch, step) for epoch in range(2) for step in range(5)]
    got = [train.train_plot_number(step, gs, 2) for gs, (_, step) in enumerate(plan)]
    assert got == [0, None, 2, None, 4, 5, None, 7, None, 9]
    assert [train.train_plot_number(step, gs, 1) for gs, (_, step) in enumerate(plan)] == list(range(10))
    assert [train.train_plot_number(step, gs, 20) for gs, (_, step) in enumerate(plan)] == [0, None, None, None, None, 5, None, None, None, None]
    # a run resumed at global step 7 keeps the epoch's indices (step 2 of epoch 1)
    assert [train.train_plot_number(step, gs, 2) for gs, (_, step) in list(enumerate(plan))[7:]] == [7, None, 9]
