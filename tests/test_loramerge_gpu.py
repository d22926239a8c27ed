"""The LoRA fold end to end (GPU): a merged tiny text encoder inside the installed ``transformers.CLIPTextModel`` against the oracle's LoRA text
encoder; ``generate_image`` at 30 steps on a trainer built from merged dicts against the oracle with LoRA, under the gates the unmerged path is held
to (tests/test_engine_gpu.py::test_generate_image_matches_oracle_at_30_steps), with the unmerged product's error on the same inputs printed beside it;
the ``merge`` CLI round trip through a tiny diffusers-layout directory and ``generate`` on it against ``generate --merge_lora``; a zero ``up``; the
refusal of ``--merge_lora`` without a LoRA file."""
import filecmp
import json
import math
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import util_models as U  # noqa: E402
from finetune_fair_diffusion_amd import generate, merge, pretrained as P, weights as W  # noqa: E402
from finetune_fair_diffusion_amd.factory import TINY  # noqa: E402

pytestmark = pytest.mark.gpu


def relerr(a, b):
    a, b = a.detach().float().cpu(), b.detach().float().cpu()
    return float((a - b).abs().max() / (b.abs().max() + 1e-20))


def check(name, a, b, tol):
    e = relerr(a, b)
    print(f"[{name}] rel max err {e:.3e} (tol {tol:.1e})  max|ref|={float(b.abs().max()):.3e}")
    assert math.isfinite(e) and e <= tol, f"{name}: {e} > {tol}"


def test_merged_text_encoder_in_transformers_equals_the_oracle_with_lora(dev):
    """Both sides fp32: the installed CLIPTextModel on ``W + up @ down`` (folded on the device) against the oracle's text encoder with the LoRA layers
    in place, for the prompt and for the padded empty prompt; 1e-5 of max|ref| is test_oracle_clip_text_pinned_against_transformers' own tolerance."""
    from transformers import CLIPTextConfig as HFConfig, CLIPTextModel as HFModel
    om = U.oracle_models(train_unet=False, train_te=True, lora_up_std=0.05)
    cfg = W.CLIPTextConfig(**U.TINY_CLIP)
    merged = merge.merge_state_dict(om["sds"]["clip"], om["sds"]["te_lora"], "text_encoder", cfg, dev)
    targets = {bk for _, _, bk in merge.lora_targets("text_encoder", cfg)}
    for k, v in om["sds"]["clip"].items():
        if k in targets:
            assert merged[k].dtype == torch.float32 and merged[k].device.type == "cpu" and not torch.equal(merged[k], v), k
        else:
            assert merged[k] is v, f"{k}: a non-target tensor must pass through as the same object"
    hf = HFModel(HFConfig(hidden_act="quick_gelu", layer_norm_eps=1e-5, bos_token_id=999, eos_token_id=998, pad_token_id=998, attn_implementation="eager",
                          max_position_embeddings=77, **U.TINY_CLIP)).eval()
    sd = {k: merged[k if k.startswith("text_model.") else "text_model." + k] for k in hf.state_dict() if "position_ids" not in k}
    missing, unexpected = hf.load_state_dict(sd, strict=False)
    assert not unexpected and all("position_ids" in k for k in missing), (missing, unexpected)
    pid, pm, uid, um = U.tiny_tokens()
    ids, mask = torch.stack([pid, uid]), torch.stack([pm, um])
    with torch.no_grad():
        got = hf(input_ids=ids, attention_mask=mask)[0]
        ref = om["text_encoder"](ids, mask)[0]
        plain = om["eval_text_encoder"](ids, mask)[0]
    err, scale = float((got - ref).abs().max()), float(ref.abs().max())
    print(f"merged text encoder in transformers vs oracle with LoRA: max |err| {err:.3e} (1e-5 * max|ref| = {1e-5 * scale:.3e}); "
          f"LoRA moves the output by {float((plain - ref).abs().max()):.3e}")
    assert got.shape == ref.shape == (2, 7, 64)
    assert float((plain - ref).abs().max()) > 1e-3 * scale, "the LoRA of this test does nothing: the comparison would show nothing"
    assert err < 1e-5 * scale


def test_generate_image_on_merged_weights_matches_oracle_at_30_steps(dev):
    """The merged path rounds ``W + up @ down`` once to 16 bit where the unmerged path rounds W, down and up separately: both are held to the oracle with
    LoRA under the unmerged test's gates, and both errors are printed."""
    from oracle import fair_step as fs
    from finetune_fair_diffusion_amd.step import FairnessTrainer
    om = U.oracle_models(train_unet=True, train_te=True, lora_up_std=0.05)
    sds = om["sds"]
    tokens = U.tiny_tokens()
    noises = torch.randn(3, 4, 32, 32, generator=torch.Generator().manual_seed(1997))
    ref = fs.generate_image_no_gradient(tokens, noises, 30, om["text_encoder"], om["unet"], om["vae"], om["scheduler"], 7.5)
    b = (ref * 0.5 + 0.5).mul(255).to(torch.uint8).permute(0, 2, 3, 1).numpy().astype(np.int32)
    msds = dict(sds, unet=merge.merge_state_dict(sds["unet"], sds["unet_lora"], "unet", W.UNetConfig(**U.TINY_UNET), dev),
                clip=merge.merge_state_dict(sds["clip"], sds["te_lora"], "text_encoder", W.CLIPTextConfig(**U.TINY_CLIP), dev))
    figures = {}
    for tag, s, lora in (("unmerged", sds, True), ("merged", msds, False)):
        pm = U.product_models(s, dev, train_unet=lora, train_te=lora, eval_copies=False)
        tr = FairnessTrainer(U.make_args(train_unet=lora, train_text_encoder=lora), pm["text_encoder"], pm["unet"], pm["vae"], pm["classifier"], pm["scheduler"],
                             device=dev)
        assert (pm["unet"].lora_bank is None) == (not lora) and (pm["text_encoder"].lora_bank is None) == (not lora)
        img = generate.generate_image(tr, tokens, noises, 30)
        a = generate.to_uint8_hwc(img).astype(np.int32)
        figures[tag] = (img, relerr(img, ref), float(np.abs(a - b).mean()), int(np.abs(a - b).max()))
        print(f"[{tag}] generate_image, S=30: rel max err {figures[tag][1]:.3e}; uint8 pixels: mean |diff| = {figures[tag][2]:.4f}, max = {figures[tag][3]}")
    img, _, mean, worst = figures["merged"]
    check("generate_image on merged weights, S=30", img, ref, 3e-2)
    assert mean < 1.0 and worst <= 8


# ------------------------------------------------------------------------------------------ the CLI
def _train_argv(out_dir, steps):
    """The two-step TINY run of tests/test_engine_gpu.py::test_generate_consumes_exported_lora."""
    return ["--synthetic", "--train_unet", "--rank", "4", "--max_train_steps", str(steps), "--checkpointing_steps", "2",
            "--checkpointing_steps_long", "3", "--checkpoints_total_limit", "2", "--num_denoising_steps", "3",
            "--train_images_per_prompt_GPU", "4", "--train_GPU_batch_size", "3", "--val_GPU_batch_size", "4",
            "--lr_scheduler", "linear", "--lr_warmup_steps", "1", "--learning_rate", "1e-5", "--output_dir", str(out_dir),
            "--weight_loss_img", "0", "--weight_loss_face", "0"]


def _write_model_dir(d):
    """A tiny diffusers-layout directory from synthetic state dicts, with one tensor per weights file that no inventory knows."""
    from safetensors.torch import save_file
    unet = dict(W.synthetic_state_dict(W.unet_param_shapes(TINY["unet"]), seed=1))
    unet["extra.not_in_the_inventory"] = torch.arange(7, dtype=torch.float16)
    unet["conv_in.bias"] = unet["conv_in.bias"].half()                                   # a non-target tensor in another dtype: it must come back as it is
    te = dict(W.synthetic_state_dict(W.clip_param_shapes(TINY["clip"]), seed=3))
    te["text_model.embeddings.position_ids"] = torch.arange(77).unsqueeze(0)           # int64, as transformers 4.30 saves it
    vae = dict(W.synthetic_state_dict(W.vae_param_shapes(TINY["vae"]), seed=2))
    for sub, name, sd in (("unet", "diffusion_pytorch_model.safetensors", unet), ("text_encoder", "model.safetensors", te),
                          ("vae", "diffusion_pytorch_model.safetensors", vae)):
        os.makedirs(d / sub)
        save_file({k: v.contiguous() for k, v in sd.items()}, str(d / sub / name), metadata={"format": "pt"})
        (d / sub / "config.json").write_text(json.dumps({"_class_name": sub}))
    os.makedirs(d / "scheduler")
    (d / "scheduler" / "scheduler_config.json").write_text(json.dumps({"_class_name": "DPMSolverMultistepScheduler"}))
    (d / "model_index.json").write_text(json.dumps({"_class_name": "StableDiffusionPipeline"}))
    return unet, te


def _tree(root):
    return sorted(os.path.relpath(os.path.join(dp, f), root) for dp, _, fs in os.walk(root) for f in fs)


def test_cli_round_trip_and_generate_on_the_merged_directory(tmp_path, dev):
    from safetensors.torch import load_file
    from finetune_fair_diffusion_amd import train
    src, out = tmp_path / "model", tmp_path / "merged"
    unet_src, te_src = _write_model_dir(src)
    train.main(_train_argv(tmp_path / "run", 2), cfgs=TINY, log=lambda s: None)
    exported = tmp_path / "run" / "checkpoints" / "checkpoint_tmp-2"
    lora = ["--load_unet_lora_from", str(exported / "unet_lora.pth"), "--load_text_encoder_lora_from", str(exported / "text_encoder_lora_EMA.pth")]
    written = merge.main(merge.parse_args(["--pretrained_model_name_or_path", str(src), "--save_dir", str(out)] + lora), cfgs=TINY)
    assert [os.path.relpath(p, out) for p in written] == [os.path.join("unet", "diffusion_pytorch_model.safetensors"), os.path.join("text_encoder", "model.safetensors")]
    assert _tree(out) == _tree(src), "OUT is a complete model directory: the files of DIR, no more, no less"
    for rel in _tree(src):
        if os.path.relpath(str(out / rel), out) not in [os.path.relpath(p, out) for p in written]:
            assert filecmp.cmp(src / rel, out / rel, shallow=False), f"{rel} was not copied unchanged"
    changed = 0
    for kind, rel, source, cfg, load in (("unet", written[0], unet_src, TINY["unet"], P.load_unet), ("text_encoder", written[1], te_src, TINY["clip"], P.load_text_encoder)):
        got = load_file(rel)
        want = merge.merge_state_dict(load(str(src), cfg), torch.load(lora[1] if kind == "unet" else lora[3], map_location="cpu"), kind, cfg, dev)
        targets = {bk for _, _, bk in merge.lora_targets(kind, cfg)}
        assert list(got) and set(got) == set(source)
        for k, v in source.items():
            if k in targets:
                assert got[k].dtype == torch.float32 and torch.equal(got[k].view(torch.int32), want[k].view(torch.int32)), f"{k}: not merge_state_dict's tensor"
                changed += int(not torch.equal(got[k], v.float()))
            else:
                assert got[k].dtype == v.dtype and got[k].shape == v.shape and torch.equal(got[k].contiguous().view(torch.uint8), v.contiguous().view(torch.uint8)), k
        back = load(str(out), cfg)                       # and the readers of pretrained.py take the merged directory
        assert all(torch.equal(back[k], want[k]) for k in targets)
    assert changed > 0, "the trained LoRA changed no weight: the round trip would show nothing"
    # generate on OUT without a LoRA flag == generate --merge_lora on DIR with the LoRA files, byte for byte (one process: hash(prompt) is the same in both)
    prompts = tmp_path / "prompts.json"
    prompts.write_text(json.dumps({"test_prompts": ["a photo of a doctor", "a photo of a chef, a person"]}))
    base = ["--prompts_path", str(prompts), "--num_imgs_per_prompt", "2", "--batch_size", "2", "--num_denoising_steps", "4", "--rank", "4"]
    w0 = generate.main(generate.parse_args(base + ["--pretrained_model_name_or_path", str(out), "--save_dir", str(tmp_path / "img_merged_dir")]), cfgs=TINY)
    w1 = generate.main(generate.parse_args(base + ["--pretrained_model_name_or_path", str(src), "--save_dir", str(tmp_path / "img_merge_lora"), "--merge_lora"] + lora), cfgs=TINY)
    w2 = generate.main(generate.parse_args(base + ["--pretrained_model_name_or_path", str(src), "--save_dir", str(tmp_path / "img_plain")]), cfgs=TINY)
    assert len(w0) == len(w1) == len(w2) == 4
    assert _tree(tmp_path / "img_merged_dir") == _tree(tmp_path / "img_merge_lora")
    for rel in _tree(tmp_path / "img_merged_dir"):
        assert filecmp.cmp(tmp_path / "img_merged_dir" / rel, tmp_path / "img_merge_lora" / rel, shallow=False), f"{rel} differs between the two merged consumers"
    # a second merge into the directory just written is refused and leaves it alone
    before = _tree(out)
    with pytest.raises(FileExistsError):
        merge.main(merge.parse_args(["--pretrained_model_name_or_path", str(src), "--save_dir", str(out)] + lora), cfgs=TINY)
    assert _tree(out) == before


def test_zero_up_merged_is_plain_generation(tmp_path):
    """A fresh LoRA (all-zero up) folded in changes nothing: the JPEGs are those of plain generation, byte for byte."""
    for name, shapes, seed in (("unet", W.unet_lora_param_shapes(TINY["unet"], 4), 5), ("te", W.clip_lora_param_shapes(TINY["clip"], 4), 6)):
        sd = W.synthetic_state_dict(shapes, seed=seed)
        assert any(float(v.abs().max()) > 0 for k, v in sd.items() if ".down." in k)
        torch.save({k: torch.zeros_like(v) if ".up." in k else v for k, v in sd.items()}, tmp_path / f"{name}_zero_up.pth")
    prompts = tmp_path / "prompts.json"
    prompts.write_text(json.dumps({"test_prompts": ["a photo of a doctor"]}))
    base = ["--synthetic", "--prompts_path", str(prompts), "--num_imgs_per_prompt", "2", "--batch_size", "2", "--num_denoising_steps", "4", "--rank", "4"]
    w0 = generate.main(generate.parse_args(base + ["--save_dir", str(tmp_path / "plain")]), cfgs=TINY)
    w1 = generate.main(generate.parse_args(base + ["--save_dir", str(tmp_path / "zero"), "--merge_lora", "--load_unet_lora_from", str(tmp_path / "unet_zero_up.pth"),
                                                   "--load_text_encoder_lora_from", str(tmp_path / "te_zero_up.pth")]), cfgs=TINY)
    assert len(w0) == len(w1) == 2
    for a, b in zip(w0, w1):
        assert filecmp.cmp(a, b, shallow=False), f"{os.path.basename(b)}: a zero up changed the image"


def test_merge_lora_without_a_lora_file_is_refused(tmp_path):
    prompts = tmp_path / "prompts.json"
    prompts.write_text(json.dumps({"test_prompts": ["a photo of a doctor"]}))
    with pytest.raises(ValueError, match="--merge_lora needs"):
        generate.main(generate.parse_args(["--synthetic", "--prompts_path", str(prompts), "--save_dir", str(tmp_path / "o"), "--merge_lora"]), cfgs=TINY)
    assert not (tmp_path / "o").exists()
