"""Host layer of the evaluator's semantics-preservation mode (``--original_imgs_dir``; no GPU): the flag, the pairing of the two trees, the summary
written to ``semantics.json``, and the identity of the metric with the training step's image-semantics loss."""
import json

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from finetune_fair_diffusion_amd import evaluate_images as EI


def _touch_tree(root, layout):
    for p, numbers in layout.items():
        d = root / f"prompt_{p}"
        d.mkdir(parents=True)
        for j in numbers:
            (d / f"img_{j}.jpg").write_bytes(b"")
    return str(root)


def test_the_flag_is_absent_unless_given():
    assert "original_imgs_dir" not in vars(EI.parse_args([]))
    assert EI.parse_args(["--original_imgs_dir", "some/tree"]).original_imgs_dir == "some/tree"


def test_pair_paths_numeric_order_and_surplus_originals(tmp_path):
    gen = _touch_tree(tmp_path / "gen", {10: (0, 1), 2: (0, 1, 2, 10)})
    ori = _touch_tree(tmp_path / "ori", {10: (0, 1, 5), 2: (0, 1, 2, 3, 10), 7: (0,)})          # img_5, img_3 and prompt_7 are surplus
    pairs = EI.pair_paths(gen, ori)
    assert list(pairs) == [2, 10]                                                                 # prompt_10 after prompt_2
    rel = lambda path, root: path[len(root) + 1:].replace("\\", "/")  # noqa: E731
    assert [rel(g, gen) for g, _ in pairs[2]] == [f"prompt_2/img_{j}.jpg" for j in (0, 1, 2, 10)]  # img_10 after img_2
    assert [rel(g, gen) for g, _ in pairs[10]] == ["prompt_10/img_0.jpg", "prompt_10/img_1.jpg"]
    for prompt in pairs.values():
        for g, o in prompt:
            assert g.startswith(gen) and o.startswith(ori) and rel(g, gen) == rel(o, ori)


def test_pair_paths_refuses_a_missing_file_and_a_missing_folder(tmp_path):
    gen = _touch_tree(tmp_path / "gen", {0: (0, 1, 2), 1: (0, 1)})
    ori = _touch_tree(tmp_path / "ori_file", {0: (0, 2), 1: (0, 1)})
    with pytest.raises(ValueError) as e:
        EI.pair_paths(gen, ori)
    assert str(tmp_path / "ori_file" / "prompt_0" / "img_1.jpg") in str(e.value) and "(1 of" in str(e.value)
    ori = _touch_tree(tmp_path / "ori_folder", {0: (0, 1, 2)})
    with pytest.raises(ValueError) as e:
        EI.pair_paths(gen, ori)
    assert str(tmp_path / "ori_folder" / "prompt_1" / "img_0.jpg") in str(e.value) and "(2 of" in str(e.value)      # the first missing path, and how many


def test_semantics_summary_schema_and_values():
    sims = [{0: torch.tensor([1.0, 0.5, 0.75, 0.25, 0.5]), 3: torch.tensor([0.5, 0.5])},
            {0: torch.tensor([0.0, 0.5, -0.25, 0.25, 0.5]), 3: torch.tensor([1.0, 0.75])}]
    numbers = {0: [0, 1, 2, 3, 10], 3: [4, 7]}
    s = EI.semantics_summary(sims, numbers)
    assert sorted(s) == ["mean", "per_prompt"] and list(s["per_prompt"]) == ["0", "3"]
    keys = ["sim_CLIP", "sim_DINO", "min_sim_CLIP", "min_sim_DINO", "argmin_CLIP", "argmin_DINO", "pairs"]
    assert all(list(v) == keys for v in s["per_prompt"].values())
    assert s["per_prompt"]["0"] == dict(sim_CLIP=0.6, sim_DINO=0.2, min_sim_CLIP=0.25, min_sim_DINO=-0.25, argmin_CLIP=3, argmin_DINO=2, pairs=5)
    # image NUMBERS, not positions (4 and 7 are positions 0 and 1); the first minimum on a tie
    assert s["per_prompt"]["3"] == dict(sim_CLIP=0.5, sim_DINO=0.875, min_sim_CLIP=0.5, min_sim_DINO=0.75, argmin_CLIP=4, argmin_DINO=7, pairs=2)
    assert s["mean"] == dict(sim_CLIP=(0.6 + 0.5) / 2, sim_DINO=(0.2 + 0.875) / 2)                # prompts weigh the same, whatever their sizes
    assert all(type(v[k]) is int for v in s["per_prompt"].values() for k in keys[4:])
    assert json.loads(json.dumps(s)) == s
    # a similarity that is not a number is written as null, as in metrics.json
    nan = EI.semantics_summary([{0: torch.tensor([float("nan")])}, {0: torch.tensor([1.0])}], {0: [0]})
    assert nan["per_prompt"]["0"]["sim_CLIP"] is None and json.loads(json.dumps(nan)) == nan
    assert EI.semantics_summary([{}, {}], {}) == {"per_prompt": {}, "mean": {}}


def test_one_minus_the_similarity_is_the_training_loss():
    from finetune_fair_diffusion_amd.vit import feature_loss_and_grad
    g = torch.Generator().manual_seed(4)
    for n, E in ((1, 8), (7, 1024), (5, 768)):
        e, t = torch.randn(n, E, generator=g) * 3, torch.randn(n, E, generator=g) * 0.2
        sim = EI.embedding_similarity(e, t)
        loss, _ = feature_loss_and_grad(e, F.normalize(t, dim=-1), torch.ones(n))
        assert sim.dtype == torch.float32 and tuple(sim.shape) == (n,)
        assert float((1 - sim - loss).abs().max()) <= 1e-6
    e = torch.randn(3, 16, generator=g)
    assert float((EI.embedding_similarity(e, 5 * e) - 1).abs().max()) <= 1e-6


def test_synthetic_vit_state_is_seeded_and_fp16_representable():
    from finetune_fair_diffusion_amd import weights as W
    from finetune_fair_diffusion_amd.factory import TINY
    for which, (key, seed) in enumerate((("clip_vision", 21), ("dino", 22))):
        sd = EI.synthetic_vit_state(which, TINY)
        raw = W.synthetic_state_dict(W.vit_param_shapes(TINY[key]), seed=seed)
        assert list(sd) == list(raw)
        for k, v in sd.items():
            assert torch.equal(v, raw[k].half().float()) and v.dtype == torch.float32, k
    assert np.isfinite(sum(float(v.abs().sum()) for v in sd.values()))
