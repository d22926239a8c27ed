"""Host layer of the offline evaluator (no GPU): the grid statement and the tile order against the reference-executed goldens
(tests/golden/make_golden_evalimages.py), the flags against the reference's defaults, the pixel rule, and the two new C-ABI entry points."""
import json
import os

import numpy as np
import torch

from finetune_fair_diffusion_amd import evaluate_images as EI, lib

HERE = os.path.dirname(os.path.abspath(__file__))
GOLD = os.path.join(HERE, "golden")


def _case(g, case, n_attr):
    im, bx, pr, pb = (g[f"{case}_{n}"] for n in ("images", "boxes", "preds", "probs"))
    pr, pb = pr[:n_attr], pb[:n_attr]
    bars = EI.grid_attrs_bar_rows(torch.from_numpy(pb)).numpy()
    return im, bx, pr, pb, bars


def test_grid_attrs_host_and_order_equal_the_reference_grids_byte_for_byte():
    path = os.path.join(GOLD, "reference_evalimages_grid.npz")
    g = np.load(path)
    assert os.path.getsize(path) < 200 * 1024
    assert len(np.unique(g["a_images"])) == 256                                 # every byte value is painted
    for case, N in (("a", 5), ("b", 9)):
        for n_attr in (2, 3):
            im, bx, pr, pb, bars = _case(g, case, n_attr)
            ref = g[f"{case}_grid{n_attr}"]
            assert im.shape == (N, 64, 64, 3) and im.dtype == np.uint8 and (pr == -1).any() and (pb == 1).any() and (pb == np.float32(0.96875)).any()
            order = EI.grid_attrs_order(pr, pb)
            out = EI.grid_attrs_host(im, order, bx, pr, bars, EI.PALETTES[:n_attr])
            assert out.dtype == np.uint8 and out.shape == ref.shape == EI.grid_attrs_shape(N, 64, 64, n_attr)[2]
            assert np.array_equal(out, ref), (case, n_attr, int((out != ref).sum()))
    # the goldens hold what they claim: groups of two in reverse confidence order at N = 5, every (gender, race) group at N = 9
    assert EI.grid_attrs_order(g["a_preds"][:2], g["a_probs"][:2]).tolist() == [1, 0, 4, 2, 3]
    assert EI.grid_attrs_order(g["a_preds"], g["a_probs"]).tolist() == [1, 0, 4, 2, 3]
    assert {(a, b) for a, b in zip(*g["b_preds"][:2, :8])} == {(gd, r) for gd in (0, 1) for r in range(4)}


def test_bar_rows_follow_the_reference_conditions():
    p = torch.tensor([[1.0, 0.5, 0.96875, -1.0], [0.5, 1.0, 0.25, -1.0], [0.75, 0.75, 1.0, -1.0]])
    two = EI.grid_attrs_bar_rows(p[:2]).tolist()
    assert two == [[-1, 256, 16, 1024], [256, -1, 384, 1024]]                  # each strip: its own p < 1
    three = EI.grid_attrs_bar_rows(p).tolist()
    assert three[:2] == two
    assert three[2] == [128, -1, 0, 1024]                                      # the age bar: race's condition, age's height (a bar of one row at p = 1)


def test_order_is_stable_and_device_order_agrees():
    rng = np.random.RandomState(3)
    for n_attr in (2, 3):
        N = 40
        preds = np.stack([rng.randint(0, 2, N), rng.randint(0, 4, N), rng.randint(0, 2, N)])[:n_attr]
        probs = rng.choice(np.float32([0.5, 0.625, 0.75, 1.0]), size=(n_attr, N))      # many ties
        preds[:, [5, 17]] = -1
        probs[:, [5, 17]] = -1
        order = EI.grid_attrs_order(preds, probs)
        assert sorted(order.tolist()) == list(range(N)) and order.tolist()[-2:] == [5, 17]
        key = probs[1] if n_attr == 2 else probs[0]
        for a, b in zip(order[:-3], order[1:-2]):                                        # inside a group: descending, ties in index order
            if all(preds[s, a] == preds[s, b] for s in range(n_attr)):
                assert key[a] > key[b] or (key[a] == key[b] and a < b)
        dev = EI.device_order(torch.from_numpy(preds).long(), torch.from_numpy(probs))
        assert dev.dtype == torch.int32 and dev.tolist() == order.tolist()


def test_flag_defaults_equal_the_reference():
    ref = json.load(open(os.path.join(GOLD, "reference_evalimages_cli.json")))["defaults"]
    got = vars(EI.parse_args([]))
    assert set(ref) <= set(got) and len(ref) == 9
    for k, v in ref.items():
        assert got[k] == v and type(got[k]) is type(v), (k, got[k], v)
    assert {k: got[k] for k in set(got) - set(ref)} == dict(synthetic=False, face_provider="synthetic", grid="gender_race")
    assert EI.parse_args(["--grid", "gender_race_age", "--synthetic", "--face_provider", "detector"]).grid == "gender_race_age"


def test_63_byte_values_come_out_one_lower():
    """The reference's pixel chain in fp32 does not return the decoded byte: the host statement paints the chain, and it differs from ``u`` for
    exactly 63 values, each by one."""
    u = torch.arange(256, dtype=torch.uint8)
    chain = ((((u.float() / 255) * 2 - 1) * 0.5 + 0.5) * 255).to(torch.uint8)
    im = u.view(1, 16, 16, 1).repeat(1, 1, 1, 3).numpy()
    z = np.zeros((1, 1), dtype=np.int32)
    grid = EI.grid_attrs_host(im, [0], np.full((1, 4), -100), z, z - 1, EI.PALETTES[:1])      # box far outside, no bar
    painted = grid[10:26, 60:76, 0].reshape(-1)
    assert grid.shape == (36, 86, 3) and np.array_equal(painted, chain.numpy())
    lower = np.nonzero(painted != u.numpy())[0]
    assert len(lower) == 63 and np.array_equal(painted[lower].astype(int), lower - 1)


def test_fp64_quotient_rounds_to_the_fp32_quotient():
    """The kernels form u/255 in fp64 and round it to fp32 (their translation unit is built with fast-math flags that turn an fp32 division by a constant
    into a reciprocal product): for all 256 values that is the fp32 quotient torch computes, also when the fp64 quotient itself is a reciprocal
    product, corrected or not -- and the fp32 reciprocal product is not."""
    u = np.arange(256)
    want = (torch.arange(256).float() / 255).numpy()
    assert np.array_equal((u.astype(np.float64) / 255.0).astype(np.float32), want)
    q = u.astype(np.float64) * (1.0 / 255.0)
    assert np.array_equal(q.astype(np.float32), want)
    assert np.array_equal((q + (u - 255.0 * q) * (1.0 / 255.0)).astype(np.float32), want)
    assert not np.array_equal(u.astype(np.float32) * np.float32(1.0 / 255.0), want)


def test_new_entry_points_are_declared_additively():
    protos = lib.parse_header()
    assert len(protos["fd_crop_resize_u8_fwd"][1]) == 9 and len(protos["fd_eval_grid_attrs_u8"][1]) == 14
    assert lib.ABI_VERSION == 4
    md = open(os.path.join(os.path.dirname(HERE), "INTEGRATION.md")).read()
    assert "`fd_crop_resize_u8_fwd`" in md and "`fd_eval_grid_attrs_u8`" in md
    if os.path.exists(lib.LIB_PATH):
        L = lib.load()
        assert L.fd_crop_resize_u8_fwd and L.fd_eval_grid_attrs_u8 and L.fd_version() == 4
