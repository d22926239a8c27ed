"""The CLIP text-image score (``evaluate_images --clip_text_score``) without a device: the fp64 statement of the text tower (tests/textscore_refs.py)
against ``transformers.CLIPTextModelWithProjection``, the tower's configs and key lists, loading both towers from one ``CLIPModel`` directory, the
summary, the folder-to-prompt mapping and every refusal (each before ``save_dir`` exists)."""
import argparse
import json
import math
import os
import sys

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
if HERE not in sys.path:
    sys.path.insert(0, HERE)
import textscore_refs as R  # noqa: E402

from finetune_fair_diffusion_amd import evaluate_images as EI  # noqa: E402
from finetune_fair_diffusion_amd import pretrained, weights as W  # noqa: E402
from finetune_fair_diffusion_amd.factory import SD15, TINY  # noqa: E402

CFG = TINY["clip_text_h"]
EOT_AT = (1, 8, 39, 76)


def _hf_text_config(c, eos):
    from transformers import CLIPTextConfig
    return CLIPTextConfig(vocab_size=c.vocab_size, hidden_size=c.hidden_size, intermediate_size=c.intermediate_size, num_hidden_layers=c.num_hidden_layers,
                          num_attention_heads=c.num_attention_heads, max_position_embeddings=c.max_position_embeddings, hidden_act=c.hidden_act,
                          projection_dim=c.projection_dim, layer_norm_eps=c.layer_norm_eps, bos_token_id=c.vocab_size - 2, eos_token_id=eos, pad_token_id=0)


@pytest.fixture(scope="module")
def hf_models():
    """transformers' tower under both of its pooling conventions (``eos_token_id == 2``: the row at ``ids.argmax``; otherwise the first position that
    holds ``eos_token_id``), with the same fp64 random weights."""
    from transformers import CLIPTextModelWithProjection
    out = {}
    for eos in (2, CFG.vocab_size - 1):
        torch.manual_seed(0)
        out[eos] = CLIPTextModelWithProjection(_hf_text_config(CFG, eos)).double().eval()
    return out


@pytest.mark.parametrize("eos", [2, CFG.vocab_size - 1])
@pytest.mark.parametrize("with_mask", [False, True])
def test_statement_equals_transformers(hf_models, eos, with_mask):
    """Measured: 3e-15 in all four cases (max |text_embeds| 3.1)."""
    m = hf_models[eos]
    ids = R.rows_with_eot_at(EOT_AT, CFG.vocab_size)
    assert ids.argmax(-1).tolist() == list(EOT_AT) and int(ids.max()) == CFG.vocab_size - 1
    mask = (torch.arange(ids.shape[1])[None] <= ids.argmax(-1)[:, None]).long() if with_mask else None          # the tokenizer's: ones up to the end-of-text token
    with torch.no_grad():
        want = m(input_ids=ids, attention_mask=mask).text_embeds
    got = R.text_embeds_ref(m.state_dict(), ids, CFG.num_attention_heads, CFG.layer_norm_eps)
    e = float((got - want).abs().max())
    print(f"[statement vs transformers, eos_token_id {eos}, mask {with_mask}] max abs diff {e:.3e} (bound 1e-10), max |ref| {float(want.abs().max()):.3f}")
    assert got.dtype == torch.float64 and tuple(got.shape) == (4, CFG.projection_dim) and e <= 1e-10
    # ids behind the end-of-text token reach neither implementation's pooled row
    tail = R.rows_with_eot_at(EOT_AT, CFG.vocab_size, tail="random")
    assert not torch.equal(tail, ids) and torch.equal(tail[:, :2], ids[:, :2])
    with torch.no_grad():
        assert float((m(input_ids=tail).text_embeds - want).abs().max()) == 0.0
    assert float((R.text_embeds_ref(m.state_dict(), tail, CFG.num_attention_heads) - got).abs().max()) == 0.0


def test_tiny_shapes_are_the_transformers_model(hf_models):
    m = hf_models[2]
    assert {k: tuple(v.shape) for k, v in m.named_parameters()} == dict(W.clip_param_shapes(CFG))
    assert W.clip_param_shapes(CFG)["text_projection.weight"] == (48, 128)
    assert CFG.projection_dim == TINY["clip_vision"].projection_dim and CFG.hidden_size // CFG.num_attention_heads == 64
    assert (CFG.vocab_size, CFG.num_hidden_layers, CFG.intermediate_size, CFG.hidden_act) == (1000, 2, 256, "gelu")


def test_vit_h14_text_tower():
    c = W.CLIP_VIT_H14_TEXT
    assert SD15["clip_text_h"] is c
    assert (c.vocab_size, c.hidden_size, c.intermediate_size, c.num_hidden_layers, c.num_attention_heads) == (49408, 1024, 4096, 24, 16)
    assert (c.max_position_embeddings, c.layer_norm_eps, c.hidden_act, c.projection_dim) == (77, 1e-5, "gelu", 1024)
    shapes = W.clip_param_shapes(c)
    assert sum(math.prod(s) for s in shapes.values()) == 354_032_640
    assert shapes["text_projection.weight"] == (1024, 1024) and "text_projection.bias" not in shapes


def test_default_config_is_unchanged():
    c = W.CLIPTextConfig()
    assert (c.hidden_act, c.projection_dim) == ("quick_gelu", 0)
    assert (c.vocab_size, c.hidden_size, c.intermediate_size, c.num_hidden_layers, c.num_attention_heads, c.max_position_embeddings) == (49408, 768, 3072, 12, 12, 77)
    want = ["text_model.embeddings.token_embedding.weight", "text_model.embeddings.position_embedding.weight"]
    for i in range(12):
        p = f"text_model.encoder.layers.{i}."
        for n in ("k_proj", "v_proj", "q_proj", "out_proj"):
            want += [p + f"self_attn.{n}.weight", p + f"self_attn.{n}.bias"]
        want += [p + "layer_norm1.weight", p + "layer_norm1.bias", p + "mlp.fc1.weight", p + "mlp.fc1.bias", p + "mlp.fc2.weight", p + "mlp.fc2.bias",
                 p + "layer_norm2.weight", p + "layer_norm2.bias"]
    want += ["text_model.final_layer_norm.weight", "text_model.final_layer_norm.bias"]
    shapes = W.clip_param_shapes(c)
    assert list(shapes) == want and len(want) == 196
    assert sum(math.prod(s) for s in shapes.values()) == 123_060_480          # the SD-v1.5 text encoder
    assert list(W.clip_param_shapes(TINY["clip"])) == [k for k in W.clip_param_shapes(CFG) if k != "text_projection.weight"]


@pytest.fixture(scope="module")
def clip_dirs(tmp_path_factory):
    """(a full tiny ``CLIPModel`` directory, a vision-only one, the full model)"""
    from transformers import CLIPConfig, CLIPModel, CLIPVisionConfig, CLIPVisionModelWithProjection
    v = TINY["clip_vision"]
    vc = CLIPVisionConfig(hidden_size=v.hidden_size, intermediate_size=v.intermediate_size, num_hidden_layers=v.num_hidden_layers,
                          num_attention_heads=v.num_attention_heads, image_size=v.image_size, patch_size=v.patch_size, hidden_act="gelu",
                          projection_dim=v.projection_dim, layer_norm_eps=v.layer_norm_eps)
    torch.manual_seed(1)
    full = CLIPModel(CLIPConfig(text_config=_hf_text_config(CFG, CFG.vocab_size - 1).to_dict(), vision_config=vc.to_dict(), projection_dim=v.projection_dim)).eval()
    d_full, d_vis = tmp_path_factory.mktemp("clip_full"), tmp_path_factory.mktemp("clip_vision_only")
    full.save_pretrained(str(d_full))
    CLIPVisionModelWithProjection(vc).save_pretrained(str(d_vis))
    return str(d_full), str(d_vis), full


def test_both_towers_load_from_one_directory(clip_dirs):
    d_full, d_vis, full = clip_dirs
    text = pretrained.load_clip_text(d_full, CFG)
    vision = pretrained.load_clip_vision(d_full, TINY["clip_vision"])
    want = full.state_dict()
    assert list(text) == list(W.clip_param_shapes(CFG)) and list(vision) == list(W.vit_param_shapes(TINY["clip_vision"]))
    for sd in (text, vision):
        for k, t in sd.items():
            assert t.dtype == torch.float32 and torch.equal(t, want[k].float()), k
    assert not any(k.startswith("vision_model.") or k == "logit_scale" for k in text)
    # the loaded tower computes what the saved model computes
    ids = R.rows_with_eot_at(EOT_AT, CFG.vocab_size, seed=3)
    with torch.no_grad():
        hf = full.double().get_text_features(input_ids=ids)
    hf = getattr(hf, "pooler_output", hf)
    assert float((R.text_embeds_ref(text, ids, CFG.num_attention_heads) - hf).abs().max()) <= 1e-10
    with pytest.raises(KeyError) as e:
        pretrained.load_clip_text(d_vis, CFG)
    assert "text_model.embeddings.token_embedding.weight" in str(e.value) and "no text tower" in str(e.value)
    assert list(pretrained.load_clip_vision(d_vis, TINY["clip_vision"])) == list(vision)


def test_model_without_projection_refuses_text_embeds():
    from finetune_fair_diffusion_amd.text_encoder import CLIPTextModel
    cfg = W.CLIPTextConfig(vocab_size=50, hidden_size=16, intermediate_size=32, num_hidden_layers=1, num_attention_heads=2)
    m = CLIPTextModel(cfg, W.synthetic_state_dict(W.clip_param_shapes(cfg), seed=0), "cpu")
    with pytest.raises(ValueError, match="projection_dim"):
        m.text_embeds(torch.zeros((1, 77), dtype=torch.int64))
    bad = W.CLIPTextConfig(vocab_size=50, hidden_size=16, intermediate_size=32, num_hidden_layers=1, num_attention_heads=2, projection_dim=8)
    with pytest.raises(KeyError, match="text_projection.weight"):
        CLIPTextModel(bad, W.synthetic_state_dict(W.clip_param_shapes(cfg), seed=0), "cpu")


def test_synthetic_inputs():
    sd = EI.synthetic_text_state(TINY)
    assert {k: tuple(v.shape) for k, v in sd.items()} == dict(W.clip_param_shapes(CFG))
    assert all(torch.equal(v, v.half().float()) for v in sd.values())
    assert torch.equal(sd["text_projection.weight"], EI.synthetic_text_state(TINY)["text_projection.weight"])          # seeded
    texts = ["a photo of a doctor", "A photo of a doctor , smiling", " ".join(["word"] * 200)]
    ids = EI.tokenize_prompts(texts, CFG, synthetic=True)
    assert ids.dtype == torch.int64 and tuple(ids.shape) == (3, 77) and int(ids.max()) == CFG.vocab_size - 1 and int(ids.min()) >= 0
    assert ids.argmax(-1).tolist() == [6, 8, 76] and (ids[:, 0] == CFG.vocab_size - 2).all()          # begin, 5 / 7 / 75 words, end-of-text
    assert (ids[0, 7:] == 0).all() and (ids[1, 9:] == 0).all()
    assert torch.equal(ids[0, 1:6], ids[1, 1:6])          # the same words, whatever their case
    for r in range(3):
        assert int((ids[r] == CFG.vocab_size - 1).sum()) == 1          # one end-of-text token, the largest id of the row
    assert tuple(EI.tokenize_prompts([], CFG, synthetic=True).shape) == (0, 77)


def test_summary():
    sims = [{0: torch.tensor([0.5, 0.1, 0.1, 0.3]), 2: torch.tensor([0.25, 0.75])}, {}]
    numbers, texts = {0: [0, 1, 2, 10], 2: [3, 4]}, {0: "a doctor", 2: "a nurse", 5: "unused"}
    js = EI.text_alignment_summary(sims, numbers, texts)
    assert json.loads(json.dumps(js)) == js and sorted(js) == ["mean", "per_prompt"] and list(js["per_prompt"]) == ["0", "2"]
    p0 = js["per_prompt"]["0"]
    assert sorted(p0) == ["argmin_clip_t", "clip_t", "min_clip_t", "prompt"]
    assert p0["prompt"] == "a doctor" and p0["argmin_clip_t"] == 1          # the image NUMBER of the first of the two minima
    assert abs(p0["clip_t"] - 0.25) < 1e-7 and abs(p0["min_clip_t"] - 0.1) < 1e-7
    assert js["per_prompt"]["2"]["argmin_clip_t"] == 3 and js["per_prompt"]["2"]["clip_t"] == 0.5
    assert sorted(js["mean"]) == ["clip_t"] and abs(js["mean"]["clip_t"] - 0.375) < 1e-7          # the mean of the per-prompt means, not of the six images
    with_ori = EI.text_alignment_summary([sims[0], {0: torch.tensor([0.5, 0.5, 0.5, 0.5]), 2: sims[0][2].clone()}], numbers, texts)
    q0, q2 = with_ori["per_prompt"]["0"], with_ori["per_prompt"]["2"]
    assert sorted(q0) == ["argmin_clip_t", "clip_t", "clip_t_delta", "clip_t_ori", "min_clip_t", "prompt"]
    assert q0["clip_t_ori"] == 0.5 and q0["clip_t_delta"] == q0["clip_t"] - 0.5 and q2["clip_t_delta"] == 0.0
    assert sorted(with_ori["mean"]) == ["clip_t", "clip_t_delta", "clip_t_ori"]
    assert with_ori["mean"]["clip_t_delta"] == (q0["clip_t_delta"] + q2["clip_t_delta"]) / 2
    assert {k: q0[k] for k in p0} == p0
    assert EI.text_alignment_summary([{}, {}], {}, {}) == {"per_prompt": {}, "mean": {}}


def _tree(root, prompts=(0, 1)):
    for p in prompts:
        os.makedirs(os.path.join(root, f"prompt_{p}"))
        open(os.path.join(root, f"prompt_{p}", "img_0.jpg"), "wb").close()
    return root


def _prompts_file(path, prompts):
    with open(path, "w") as f:
        json.dump({"test_prompts": list(prompts), "train_prompts": ["not read"]}, f)
    return str(path)


def test_folder_to_prompt_mapping(tmp_path):
    gen = _tree(str(tmp_path / "gen"), prompts=(10, 2, 0))
    prompts = [f"text {i}" for i in range(11)]
    got = EI.folder_prompts(gen, EI.load_prompts(_prompts_file(tmp_path / "p.json", prompts)))
    assert list(got.items()) == [(0, "text 0"), (2, "text 2"), (10, "text 10")]          # numeric order; prompt_10 is test_prompts[10], not [2]
    with pytest.raises(ValueError, match="prompt_10"):
        EI.folder_prompts(gen, prompts[:10])
    with open(tmp_path / "bad.json", "w") as f:
        json.dump({"test_prompts": "a string"}, f)
    with pytest.raises(ValueError, match="list of strings"):
        EI.load_prompts(str(tmp_path / "bad.json"))


def _main_args(gen, out, *more):
    return EI.parse_args(["--generated_imgs_dir", gen, "--save_dir", str(out), "--clip_text_score", *more])


def test_refusals_come_before_anything_is_written(tmp_path, clip_dirs, monkeypatch):
    """Every refusal of the flag is host work at the head of ``main``: it is raised with or without a device, and ``save_dir`` does not exist after it."""
    d_full, d_vis, _ = clip_dirs
    gen, out = _tree(str(tmp_path / "gen")), tmp_path / "out"
    two, one = _prompts_file(tmp_path / "two.json", ["a doctor", "a nurse"]), _prompts_file(tmp_path / "one.json", ["a doctor"])
    monkeypatch.delenv("FD_CLIP_VISION_DIR", raising=False)

    def refused(exc, match, *more):
        with pytest.raises(exc, match=match):
            EI.main(_main_args(gen, out, *more), log=None, cfgs=TINY)
        assert not os.path.exists(str(out))

    refused(ValueError, "--prompts_path", "--synthetic")                                        # the flag alone
    refused(FileNotFoundError, "nowhere.json", "--synthetic", "--prompts_path", str(tmp_path / "nowhere.json"))
    refused(ValueError, "prompt_1", "--synthetic", "--prompts_path", one)                    # a folder beyond the prompt list
    refused(FileNotFoundError, "FD_CLIP_VISION_DIR", "--prompts_path", two)                  # a real run without the checkpoint directory
    monkeypatch.setenv("FD_CLIP_VISION_DIR", d_vis)
    refused(KeyError, "text_model.embeddings.token_embedding.weight", "--prompts_path", two)          # a checkpoint without the text tower
    # the host side of a run that is not refused: texts, ids and weights by prompt index
    texts, ids, sd = EI._text_inputs(_main_args(gen, out, "--synthetic", "--prompts_path", two), TINY)
    assert texts == {0: "a doctor", 1: "a nurse"} and sorted(ids) == [0, 1] and tuple(ids[1].shape) == (1, 77)
    assert torch.equal(ids[1], EI.tokenize_prompts(["a nurse"], CFG, synthetic=True)) and not torch.equal(ids[0], ids[1])
    assert list(sd) == list(W.clip_param_shapes(CFG)) and not os.path.exists(str(out))


def test_real_run_reads_tokenizer_and_tower_from_the_checkpoint_directory(tmp_path, clip_dirs, monkeypatch):
    """A tiny character-level ``CLIPTokenizer`` saved beside the tiny ``CLIPModel``: the host side of a run without ``--synthetic``."""
    import shutil
    from transformers import CLIPTokenizer
    model_dir = str(tmp_path / "clip")
    shutil.copytree(clip_dirs[0], model_dir)
    chars = list("abcdefghijklmnopqrstuvwxyz,")
    vocab = {c: i for i, c in enumerate(chars + [c + "</w>" for c in chars] + ["<|startoftext|>", "<|endoftext|>"])}
    with open(tmp_path / "vocab.json", "w") as f:
        json.dump(vocab, f)
    with open(tmp_path / "merges.txt", "w") as f:
        f.write("#version: 0.2\n")
    CLIPTokenizer(str(tmp_path / "vocab.json"), str(tmp_path / "merges.txt")).save_pretrained(model_dir)
    bos, eot = vocab["<|startoftext|>"], vocab["<|endoftext|>"]
    assert eot == max(vocab.values())
    ids = EI.tokenize_prompts(["a dog", "word " * 100], CFG, synthetic=False, model_dir=model_dir)
    assert ids.dtype == torch.int64 and tuple(ids.shape) == (2, 77) and (ids[:, 0] == bos).all()
    assert ids[0, :6].tolist() == [bos, vocab["a</w>"], vocab["d"], vocab["o"], vocab["g</w>"], eot]
    assert ids.argmax(-1).tolist() == [5, 76] and int(ids[1, 76]) == eot          # padded to 77; truncation keeps the end-of-text token
    gen = _tree(str(tmp_path / "gen"))
    monkeypatch.setenv("FD_CLIP_VISION_DIR", model_dir)
    args = _main_args(gen, tmp_path / "out", "--prompts_path", _prompts_file(tmp_path / "p.json", ["a dog", "word " * 100]))
    texts, by_prompt, sd = EI._text_inputs(args, TINY)
    assert texts == {0: "a dog", 1: "word " * 100} and torch.equal(torch.cat([by_prompt[0], by_prompt[1]]), ids)
    want = pretrained.load_clip_text(model_dir, CFG)
    assert list(sd) == list(want) and all(torch.equal(sd[k], want[k]) for k in sd) and not os.path.exists(str(tmp_path / "out"))


def test_flags_are_absent_unless_given():
    base = vars(EI.parse_args([]))
    assert "clip_text_score" not in base and "prompts_path" not in base
    ns = EI.parse_args(["--clip_text_score", "--prompts_path", "p.json"])
    assert ns.clip_text_score is True and ns.prompts_path == "p.json"
    assert {k: v for k, v in vars(ns).items() if k not in ("clip_text_score", "prompts_path")} == base
    assert isinstance(ns, argparse.Namespace) and np.isfinite(EI.SYNTHETIC_TEXT_SEED)
