"""Host layer of the in-training validation (no GPU): the metrics and the grid statement against the reference-executed goldens
(tests/golden/make_golden_eval.py), the opt-in flag, the places where the validation noise is drawn, and the two new C-ABI entry points."""
import ctypes
import json
import math
import os
import random

import numpy as np
import torch

from finetune_fair_diffusion_amd import cli, evaluation as E, lib, train

HERE = os.path.dirname(os.path.abspath(__file__))
GOLD = os.path.join(HERE, "golden")


def _attrs(sizes):
    out, c = [], 0
    for k in sizes:
        out.append((c, k))
        c += k
    return out


def test_gap_metrics_equal_the_reference_exactly():
    cases = json.load(open(os.path.join(GOLD, "reference_eval_metrics.json")))["cases"]
    seen = set()
    for c in cases:
        t = torch.tensor(c["probs"], dtype=torch.float32)
        m = E.gap_metrics(c["experiment"], E.tally_host(t, _attrs(c["sizes"])))
        assert set(m) == set(c["metrics"])
        for k, v in c["metrics"].items():
            assert m[k] == v or (math.isnan(v) and math.isnan(m[k])), (c["experiment"], c["table"], c["N"], k, m[k], v)
        seen.add((c["experiment"], c["table"], c["N"]))
    assert len(seen) == 5 * 4 * 6 and {e for e, _, _ in seen} == {"exp-1", "exp-3", "exp-4", "exp-5", "exp-6"}
    # an empty valid set gives NaN, as the reference's mean() of an empty tensor does
    assert all(math.isnan(v) for c in cases if c["table"] == "no_valid" for v in c["metrics"].values())
    # exp-2 validates with exp-1's numbers
    t = torch.tensor(cases[0]["probs"], dtype=torch.float32)
    assert E.gap_metrics("exp-2", E.tally_host(t, [(0, 2)])) == E.gap_metrics("exp-1", E.tally_host(t, [(0, 2)]))


def test_tally_host_refuses_attributes_that_are_not_valid_together():
    t = torch.tensor([[0.5, 0.5, -1.0, -1.0, -1.0, -1.0]])
    try:
        E.tally_host(t, [(0, 2), (2, 4)])
    except AssertionError:
        return
    raise AssertionError("a row valid in one attribute only was accepted")


def test_grid_host_equals_the_reference_grid_byte_for_byte():
    g = np.load(os.path.join(GOLD, "reference_eval_grid.npz"))
    assert os.path.getsize(os.path.join(GOLD, "reference_eval_grid.npz")) < 200 * 1024
    for case, N in (("a", 5), ("b", 9)):
        im, bx, pr, mp, ref = (g[f"{case}_{n}"] for n in ("images", "boxes", "preds", "maxprob", "grid"))
        assert im.shape == (N, 3, 64, 64) and (pr == -1).any() and (mp == 1).any()
        out = E.grid_host(torch.from_numpy(im), E.grid_order(pr, mp), bx, pr, mp, E.PALETTE_GENDER)
        assert out.dtype == np.uint8 and out.shape == ref.shape == E.grid_shape(N, 64, 64)[2]
        assert np.array_equal(out, ref), int((out != ref).sum())


def test_validation_flag_parses_and_defaults_to_off():
    assert cli.parse_args([], with_extras=True).validation == "off"
    assert cli.parse_args(["--validation", "grids"], with_extras=True, experiment="exp-4").validation == "grids"
    assert cli.EXTRA_DEFAULTS["validation"] == "off"
    for every in (1, 200):
        assert not train.evaluation_due("off", 0, every) and not train.evaluation_due("off", every, every)
    assert train.evaluation_due("metrics", 0, 200) and train.evaluation_due("grids", 400, 200) and not train.evaluation_due("metrics", 401, 200)
    data = train.SYNTHETIC_PROMPTS
    assert len(E.validation_prompts(data)) == len(data["prompt_templates_test"]) * len(data["occupations_val_set"]) >= 1


def _loop(validation, steps, every, B=2, lat=4, P=2, n_val=3, look_ahead=True):
    """The train loop's host randomness alone (train.main's order of draws), with its look-ahead."""
    torch.manual_seed(11); random.seed(11); np.random.seed(11)
    drawn, peeked, val = [], [], []
    draw = lambda: train.draw_step_noise(B, lat, 0)
    draw_val = lambda: E.draw_val_noise(P, n_val, lat)
    gs = 0
    for i in range(steps):
        if gs == 0 and train.evaluation_due(validation, 0, every):
            val.append(draw_val())
        drawn.append(draw())
        if look_ahead and i + 1 < steps:
            peeked.append(train.peek_draw(draw, before=draw_val if train.evaluation_due(validation, gs + 1, every) else None))
        gs += 1
        if train.evaluation_due(validation, gs, every):
            val.append(draw_val())
    return drawn, peeked, val, torch.get_rng_state()


def test_off_draws_no_validation_noise_and_peek_sees_the_next_draw():
    torch.manual_seed(11); random.seed(11); np.random.seed(11)
    plain = [train.draw_step_noise(2, 4, 0) for _ in range(4)]
    end = torch.get_rng_state()
    for every in (1, 2):
        drawn, peeked, val, st = _loop("off", 4, every)
        assert not val and torch.equal(st, end)
        assert all(torch.equal(a[0], b[0]) and a[1] == b[1] for a, b in zip(drawn, plain))
    # with validation the stream is consumed at the reference's points: before the first training noise, and after each due step
    for every in (1, 2, 3):
        drawn, peeked, val, st = _loop("metrics", 5, every)
        d2, _, v2, st2 = _loop("metrics", 5, every, look_ahead=False)
        assert len(val) == 1 + 5 // every and torch.equal(st, st2)                      # the look-ahead consumes nothing
        assert all(torch.equal(a[0], b[0]) and a[1] == b[1] for a, b in zip(drawn, d2))
        assert all(torch.equal(a, b) for a, b in zip(val, v2))
        # ... and what peek returned is exactly what the next draw returned, also across an evaluation
        assert len(peeked) == 4 and all(torch.equal(p[0], d[0]) and p[1] == d[1] for p, d in zip(peeked, drawn[1:]))
        assert not torch.equal(drawn[0][0], plain[0][0])                                # the first training noise comes after the validation noise
    torch.manual_seed(11)
    first_val = E.draw_val_noise(2, 3, 4)
    assert torch.equal(_loop("grids", 1, 7)[2][0], first_val)


def test_header_declares_and_both_libraries_export_the_entry_points():
    protos = lib.parse_header()
    assert len(protos["fd_eval_tally"][1]) == 8 and len(protos["fd_eval_grid_u8"][1]) == 13
    src = open(lib.HEADER_PATH).read()
    assert "#define FD_ABI_VERSION 4" in src.replace("  ", " ") or lib.ABI_VERSION == 4
    for k, v in dict(FD_EVAL_COUNTS=E.N_COUNTS, FD_EVAL_ATTR_STRIDE=E.ATTR_STRIDE, FD_EVAL_OFF_P1_HI=E.OFF_P1_HI, FD_EVAL_OFF_P1_LO=E.OFF_P1_LO,
                     FD_EVAL_OFF_P1_MID=E.OFF_P1_MID, FD_EVAL_OFF_JOINT=E.OFF_JOINT, FD_EVAL_OFF_JOINT_VALID=E.OFF_JOINT_VALID).items():
        assert f"#define {k} {v} " in src or f"#define {k} {v}\n" in src, k
    d = os.path.dirname(lib.LIB_PATH)
    for name in ("libfairdiff_hip.so", "libfairdiff_hip_bf16.so"):
        L = ctypes.CDLL(os.path.join(d, name))
        assert L.fd_eval_tally and L.fd_eval_grid_u8 and L.fd_version() == 4
