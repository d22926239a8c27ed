"""The CLIP text-image score on the device: ``CLIPTextModel.text_embeds`` at the ViT-H text tower's tiny configuration (head dim 64, exact gelu, a
projection) against the fp64 statement of tests/textscore_refs.py, and ``evaluate_images.main --clip_text_score`` on small trees of JPEGs against the
oracle CLIP image encoder and that statement.  tests/textscore_cases.py holds the inputs and the references; tests/test_textscore_bf16_gpu.py runs the
bf16 library on the same cases.

Bands: 2e-2 of max|ref| for the embeddings (the band tests/test_engine_gpu.py gives network outputs), 2e-2 absolute for a similarity against the
oracle (``BAND_ORACLE`` of tests/test_semantics_gpu.py), 2e-3 between two launch forms of one forward."""
import json
import os
import pickle
import sys

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
if HERE not in sys.path:
    sys.path.insert(0, HERE)
import textscore_cases as C  # noqa: E402
import textscore_refs as R  # noqa: E402

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def EI():
    from finetune_fair_diffusion_amd import evaluate_images
    return evaluate_images


@pytest.fixture(scope="module")
def TINY():
    from finetune_fair_diffusion_amd.factory import TINY
    return TINY


@pytest.fixture(scope="module")
def tower(EI, TINY, dev):
    from finetune_fair_diffusion_amd.text_encoder import CLIPTextModel
    return CLIPTextModel(TINY["clip_text_h"], EI.synthetic_text_state(TINY), dev)


@pytest.fixture(scope="module")
def rows(TINY):
    return R.rows_with_eot_at(C.EOT_AT, TINY["clip_text_h"].vocab_size)


@pytest.fixture(scope="module")
def batch_embeds(tower, rows):
    e = tower.text_embeds(rows)
    return e.float().cpu(), e.dtype, e.is_cuda


def test_text_embeds_against_the_statement(EI, TINY, rows, batch_embeds):
    """Measured on an MI355X: 6.4e-4 of max|ref| = 2.96 (per row 6.4e-4 / 5.7e-4 / 4.9e-4 / 5.4e-4); every figure of this file is in
    profiles/evalimages_textscore.md."""
    got, dtype, on_device = batch_embeds
    ref = C.text_reference(EI, TINY, rows)
    assert rows.argmax(-1).tolist() == list(C.EOT_AT)
    assert dtype == torch.float16 and on_device and tuple(got.shape) == (4, TINY["clip_text_h"].projection_dim)          # the fp16 library's working dtype
    for r, p in enumerate(C.EOT_AT):
        print(f"[text_embeds vs fp64 statement, end-of-text at {p}] rel max err {float((got[r].double() - ref[r]).abs().max() / ref.abs().max()):.3e}")
    e = float((got.double() - ref).abs().max() / ref.abs().max())
    print(f"[text_embeds vs fp64 statement] rel max err {e:.3e} (band {C.BAND_EMBEDS:.1e})  max|ref| {float(ref.abs().max()):.3f}")
    assert np.isfinite(e) and e <= C.BAND_EMBEDS
    # the rows differ by far more than the band: a wrong pooling row cannot hide in it
    spread = float((ref[:, None] - ref[None]).abs().amax(-1)[~torch.eye(4, dtype=torch.bool)].min() / ref.abs().max())
    print(f"[text_embeds] smallest distance between two rows of the reference: {spread:.3f} of max|ref|")
    assert spread > 5 * C.BAND_EMBEDS


def test_ids_behind_the_end_of_text_token_change_nothing(TINY, tower, rows, batch_embeds):
    tail = R.rows_with_eot_at(C.EOT_AT, TINY["clip_text_h"].vocab_size, tail="random")
    assert not torch.equal(tail[:3], rows[:3]) and torch.equal(tail[3], rows[3])          # position 76 has nothing behind it
    got = tower.text_embeds(tail).float().cpu()
    assert torch.equal(got, batch_embeds[0])          # bit-equal: the pooled row is the end-of-text row and the mask is causal


def test_one_row_at_a_time_equals_the_batch(tower, rows, batch_embeds):
    one = torch.cat([tower.text_embeds(rows[r:r + 1]).float().cpu() for r in range(4)])
    e = float((one - batch_embeds[0]).abs().max() / batch_embeds[0].abs().max())
    print(f"[text_embeds, one row at a time vs the batch of four] rel max diff {e:.3e} (band {C.BAND_LAUNCH_FORM:.1e})")
    assert np.isfinite(e) and e <= C.BAND_LAUNCH_FORM


def test_quick_gelu_tower_has_no_text_embeds(TINY, dev):
    from finetune_fair_diffusion_amd import weights as W
    from finetune_fair_diffusion_amd.text_encoder import CLIPTextModel
    m = CLIPTextModel(TINY["clip"], W.synthetic_state_dict(W.clip_param_shapes(TINY["clip"]), seed=3), dev)
    with pytest.raises(ValueError, match="projection_dim"):
        m.text_embeds(torch.zeros((1, 77), dtype=torch.int64))


# ------------------------------------------------------------------------------------------ the evaluator on trees
@pytest.fixture(scope="module")
def trees(tmp_path_factory):
    return C.build_trees(tmp_path_factory.mktemp("textscore_trees"))


@pytest.fixture(scope="module")
def references(EI, TINY, trees):
    """([2,10] reference scores of the generated images against the two texts, the same of the originals), computed once"""
    return C.score_reference(EI, TINY, trees[3]), C.score_reference(EI, TINY, trees[4])


def _load(save_dir, name):
    with open(os.path.join(str(save_dir), name), "rb") as f:
        return pickle.load(f)


def _bytes(save_dir, name):
    with open(os.path.join(str(save_dir), name), "rb") as f:
        return f.read()


def _cat(d):
    return torch.cat([d[0], d[1]])


def _same_pickle(dir_a, dir_b, name, n_dicts):
    """A pickle of torch tensors names each storage by its address, so two runs of one command differ in those bytes: the content is compared, bit
    for bit (keys, dtypes, shapes and the bytes of every tensor), as tests/test_evalfaces_gpu.py does."""
    a_all, b_all = _load(dir_a, name), _load(dir_b, name)
    assert len(a_all) == len(b_all) == n_dicts, name
    for a, b in zip(a_all, b_all):
        assert sorted(a) == sorted(b) == [0, 1], name
        for p in a:
            assert a[p].dtype == b[p].dtype and a[p].shape == b[p].shape, (name, p)
            assert a[p].contiguous().numpy().tobytes() == b[p].contiguous().numpy().tobytes(), (name, p)


@pytest.fixture(scope="module")
def run_flag(EI, TINY, trees, tmp_path_factory, dev):
    """The flag alone, batch size 4, grids on."""
    d = tmp_path_factory.mktemp("text4")
    return d, C.run(EI, TINY, trees[0], d, 4, prompts=trees[2], grid="gender_race")


@pytest.fixture(scope="module")
def run_pairs(EI, TINY, trees, tmp_path_factory, dev):
    """The flag with the second tree as originals, batch size 4."""
    d = tmp_path_factory.mktemp("textpairs4")
    return d, C.run(EI, TINY, trees[0], d, 4, prompts=trees[2], ori=trees[1])


def test_evaluator_against_the_oracle(EI, run_flag, references):
    """Measured on an MI355X: max |sim_clip_text - reference| 2.1e-4 over the 10 images; against the other prompt's text 0.343."""
    d, lines = run_flag
    own, other = C.own_and_other(references[0])
    # on the reference alone: the other prompt's text moves at least one image's value by five bands, so a swapped mapping cannot pass
    moved = float((own - other).abs().max())
    print("[text score reference, own prompt]   " + " ".join(f"{float(v):.4f}" for v in own))
    print("[text score reference, other prompt] " + " ".join(f"{float(v):.4f}" for v in other))
    assert moved >= C.SEPARATION, moved
    sims = _load(d, "text_alignment.pkl")
    assert isinstance(sims, list) and len(sims) == 2 and sorted(sims[0]) == [0, 1]
    for t in sims[0].values():
        assert t.dtype == torch.float32 and tuple(t.shape) == (5,) and not t.is_cuda
    got = _cat(sims[0]).double()
    e = float((got - own).abs().max())
    print(f"[sim_clip_text vs oracle image encoder and fp64 text statement] max abs err {e:.3e} (band {C.BAND_ORACLE:.1e}); against the other prompt's "
          f"text: {float((got - other).abs().max()):.3e}")
    assert torch.isfinite(got).all() and e <= C.BAND_ORACLE


def test_without_originals(EI, run_flag):
    d, lines = run_flag
    sims = _load(d, "text_alignment.pkl")
    assert sims[1] == {}
    js = json.load(open(os.path.join(str(d), "text_alignment.json")))
    assert js == EI.text_alignment_summary(sims, {0: list(C.NUMBERS), 1: list(C.NUMBERS)}, dict(enumerate(C.PROMPTS)))
    assert list(js["per_prompt"]) == ["0", "1"] and sorted(js["mean"]) == ["clip_t"]
    for p in (0, 1):
        row = js["per_prompt"][str(p)]
        assert sorted(row) == ["argmin_clip_t", "clip_t", "min_clip_t", "prompt"] and row["prompt"] == C.PROMPTS[p]
        assert row["argmin_clip_t"] == C.NUMBERS[int(sims[0][p].argmin())] and row["min_clip_t"] == float(sims[0][p].min())
    assert "clip_t_ori" not in json.dumps(js)
    line = json.loads(lines[-1])
    assert line["text_prompts"] == 2 and line["evaluated_images"] == 10 and "semantics_pairs" not in line


def test_batch_size_one_gives_the_same_scores(EI, TINY, trees, run_flag, tmp_path):
    C.run(EI, TINY, trees[0], tmp_path, 1, prompts=trees[2])
    e = float((_cat(_load(tmp_path, "text_alignment.pkl")[0]) - _cat(_load(run_flag[0], "text_alignment.pkl")[0])).abs().max())
    print(f"[sim_clip_text, batch size 1 vs 4] max abs diff {e:.3e} (band {C.BAND_LAUNCH_FORM:.1e})")
    assert np.isfinite(e) and e <= C.BAND_LAUNCH_FORM


def test_nothing_else_moves(EI, TINY, trees, run_flag, tmp_path):
    d, _ = run_flag
    lines = C.run(EI, TINY, trees[0], tmp_path, 4, grid="gender_race")
    plain = ["metrics.json", "prompt_0.jpg", "prompt_1.jpg", "test_results.pkl"]
    assert sorted(os.listdir(str(tmp_path))) == plain
    assert sorted(os.listdir(str(d))) == sorted(plain + ["text_alignment.json", "text_alignment.pkl"])
    for name in plain[:3]:
        assert _bytes(d, name) == _bytes(tmp_path, name), name
    _same_pickle(d, tmp_path, "test_results.pkl", 5)
    assert sorted(json.loads(lines[-1])) == ["evaluated_images", "images_per_s", "prompts", "seconds"]


def test_with_originals(EI, TINY, trees, run_pairs, run_flag, references, tmp_path):
    d, lines = run_pairs
    sims = _load(d, "text_alignment.pkl")
    assert sorted(sims[0]) == sorted(sims[1]) == [0, 1]
    # the originals are scored against the same text, within the band of the reference
    e_gen = float((_cat(sims[0]).double() - C.own_and_other(references[0])[0]).abs().max())
    e_ori = float((_cat(sims[1]).double() - C.own_and_other(references[1])[0]).abs().max())
    print(f"[sim_clip_text with originals vs reference] generated {e_gen:.3e}, originals {e_ori:.3e} (band {C.BAND_ORACLE:.1e})")
    assert e_gen <= C.BAND_ORACLE and e_ori <= C.BAND_ORACLE
    # the generated images went through the tower in a batch with their originals: another launch form of the run without them
    e = float((_cat(sims[0]) - _cat(_load(run_flag[0], "text_alignment.pkl")[0])).abs().max())
    print(f"[sim_clip_text, with vs without originals] max abs diff {e:.3e} (band {C.BAND_LAUNCH_FORM:.1e})")
    assert e <= C.BAND_LAUNCH_FORM
    js = json.load(open(os.path.join(str(d), "text_alignment.json")))
    assert js == EI.text_alignment_summary(sims, {0: list(C.NUMBERS), 1: list(C.NUMBERS)}, dict(enumerate(C.PROMPTS)))
    for p in ("0", "1"):
        row = js["per_prompt"][p]
        assert row["clip_t_delta"] == row["clip_t"] - row["clip_t_ori"] and row["clip_t_delta"] != 0.0
    assert sorted(js["mean"]) == ["clip_t", "clip_t_delta", "clip_t_ori"]
    line = json.loads(lines[-1])
    assert line["text_prompts"] == 2 and line["semantics_pairs"] == 10
    # the pair similarities are byte for byte those of a run without the flag
    C.run(EI, TINY, trees[0], tmp_path, 4, ori=trees[1])
    names = ["metrics.json", "semantics.json", "semantics.pkl", "test_results.pkl"]
    assert sorted(os.listdir(str(tmp_path))) == names
    assert sorted(os.listdir(str(d))) == sorted(names + ["text_alignment.json", "text_alignment.pkl"])
    for name in ("metrics.json", "semantics.json"):
        assert _bytes(d, name) == _bytes(tmp_path, name), name
    _same_pickle(d, tmp_path, "semantics.pkl", 2)
    _same_pickle(d, tmp_path, "test_results.pkl", 5)


def test_a_tree_against_itself(EI, TINY, trees, tmp_path, dev):
    C.run(EI, TINY, trees[0], tmp_path, 4, prompts=trees[2], ori=trees[0])
    sims = _load(tmp_path, "text_alignment.pkl")
    assert torch.equal(_cat(sims[0]), _cat(sims[1]))
    js = json.load(open(os.path.join(str(tmp_path), "text_alignment.json")))
    assert [js["per_prompt"][p]["clip_t_delta"] for p in ("0", "1")] == [0.0, 0.0] and js["mean"]["clip_t_delta"] == 0.0


@pytest.mark.parametrize("n", [1, 3])
def test_text_alignment_function(EI, TINY, tower, trees, references, dev, n):
    """``text_alignment`` is the evaluator's chain without a tree: one text for all images ([1,T]) and one text per image ([n,T])."""
    from finetune_fair_diffusion_amd import weights as W
    from finetune_fair_diffusion_amd.vit import VisionTransformer
    clip = VisionTransformer(TINY["clip_vision"], EI.synthetic_vit_state(0, TINY), dev, W.CLIP_IMAGE_MEAN, W.CLIP_IMAGE_STD)
    ids = EI.tokenize_prompts(C.PROMPTS[:2], TINY["clip_text_h"], synthetic=True)
    u8 = trees[3][4:4 + n].to(dev)          # the last image of prompt 0, then images of prompt 1
    ref = references[0][:, 4:4 + n]
    one = EI.text_alignment(clip, tower, u8, ids[:1])
    assert one.is_cuda and one.dtype == torch.float32 and tuple(one.shape) == (n,)
    per_image = ids[[0, 1, 0][:n]]
    each = EI.text_alignment(clip, tower, u8, per_image)
    want_each = torch.stack([ref[[0, 1, 0][j], j] for j in range(n)])
    e1, e2 = float((one.cpu().double() - ref[0]).abs().max()), float((each.cpu().double() - want_each).abs().max())
    print(f"[text_alignment, n={n}] max abs err: one text {e1:.3e}, a text per image {e2:.3e} (band {C.BAND_ORACLE:.1e})")
    assert e1 <= C.BAND_ORACLE and e2 <= C.BAND_ORACLE
