"""Inputs and references of the text-score device checks, shared by tests/test_textscore_gpu.py (fp16 library) and tests/run_bf16_textscore_checks.py
(bf16 library).  Everything here is host work: the trees of JPEGs, the oracle CLIP image encoder on the fp32 statement of the resize, and the fp64
statement of the text tower (tests/textscore_refs.py) on the evaluator's own synthetic weights and token ids."""
import json
import os

import numpy as np
import torch
import torch.nn.functional as F

import textscore_refs as R

S_FACE = 64
NUMBERS = (0, 1, 2, 3, 10)          # img_10 sorts after img_3 numerically
EOT_AT = (1, 8, 39, 76)             # right behind the begin token, inside the first 64 keys, behind them (the kernel's second lane pass), the last position
# a long and a one-word prompt: with the evaluator's text seed (23) their reference scores of one image lie up to 0.34 apart (two sentences of similar
# length gave 0.055, less than SEPARATION below: a swapped mapping would have passed the band)
PROMPTS = ["a painting of a lighthouse at night , stormy sea", "dog", "never used : no folder prompt_2"]
BOXES = [[8, 6, 50, 48], [-7, 5, 35, 47], [20, 20, 70, 70], None, [0, 0, 64, 64],
         [10, 12, 40, 42], [5, 30, 45, 70], [30, 2, 62, 34], [16, 16, 48, 48], [-10, -10, 74, 74]]
BAND_EMBEDS, BAND_ORACLE, BAND_LAUNCH_FORM = 2e-2, 2e-2, 2e-3          # of max|ref| / absolute on a similarity / between two launch forms
SEPARATION = 1e-1                   # what the other prompt's text must move one reference value by: five bands


class ScriptedProvider:
    """Boxes by running image number, whatever the batch size."""

    def __init__(self):
        self.seen = 0

    def __call__(self, images):
        bb = [BOXES[(self.seen + i) % len(BOXES)] for i in range(images.shape[0])]
        self.seen += images.shape[0]
        return torch.tensor([b is not None for b in bb]), torch.tensor([b if b is not None else [-1] * 4 for b in bb], dtype=torch.int32)


def build_trees(root):
    """Two trees (generated, original) of two prompts with five 64x64 JPEGs each, unrelated images, and the prompts file -> (generated dir, original
    dir, prompts path, decoded generated [10,64,64,3] uint8, decoded originals [10,64,64,3] uint8)."""
    from PIL import Image
    rng = np.random.RandomState(11)
    dirs, decoded = [], []
    for name in ("generated", "original"):
        d = os.path.join(str(root), name)
        dirs.append(d)
        dec = []
        for p in range(2):
            os.makedirs(os.path.join(d, f"prompt_{p}"))
            for j in NUMBERS:
                path = os.path.join(d, f"prompt_{p}", f"img_{j}.jpg")
                Image.fromarray(np.kron(rng.randint(0, 256, (8, 8, 3)).astype(np.uint8), np.ones((8, 8, 1), dtype=np.uint8))).save(path)
                dec.append(np.asarray(Image.open(path).convert("RGB")))
        decoded.append(torch.from_numpy(np.stack(dec)))
    prompts_path = os.path.join(str(root), "prompts.json")
    with open(prompts_path, "w") as f:
        json.dump({"test_prompts": PROMPTS}, f)
    return dirs[0], dirs[1], prompts_path, decoded[0], decoded[1]


def text_reference(EI, TINY, ids):
    """fp64 text_embeds [B,48] of the evaluator's synthetic tower for ids [B,77]."""
    cfg = TINY["clip_text_h"]
    return R.text_embeds_ref(EI.synthetic_text_state(TINY), ids, cfg.num_attention_heads, cfg.layer_norm_eps)


def image_reference(EI, TINY, u8):
    """Unit fp32 image embeddings [n,48] of the oracle CLIP encoder on ``F.interpolate`` of the fp32 images; u8 [n,H,W,3] uint8 on the host."""
    from finetune_fair_diffusion_amd import weights as W
    from oracle import nn_vit as OV
    cfg = TINY["clip_vision"]
    model = OV.build(OV.ViTConfig(**cfg.__dict__), EI.synthetic_vit_state(0, TINY))
    x = F.interpolate(u8.permute(0, 3, 1, 2).float() / 255 * 2 - 1, size=cfg.image_size, mode="bilinear", align_corners=False)
    with torch.no_grad():
        return OV.image_features(model, x, W.CLIP_IMAGE_MEAN, W.CLIP_IMAGE_STD, normalize=True)


def score_reference(EI, TINY, u8):
    """-> [2, n] float64: the reference similarity of each image to the text of prompt 0 (row 0) and of prompt 1 (row 1)."""
    ids = EI.tokenize_prompts(PROMPTS[:2], TINY["clip_text_h"], synthetic=True)
    t = F.normalize(text_reference(EI, TINY, ids), dim=-1)
    return t @ image_reference(EI, TINY, u8).double().t()


def own_and_other(ref):
    """ref [2, 10] (images of prompt 0, then of prompt 1) -> (each image against its own prompt's text [10], against the other prompt's [10])."""
    own = torch.cat([ref[0, :5], ref[1, 5:]])
    other = torch.cat([ref[1, :5], ref[0, 5:]])
    return own, other


def run(EI, TINY, gen, save_dir, batch_size, prompts=None, ori=None, grid="off"):
    argv = ["--synthetic", "--generated_imgs_dir", gen, "--save_dir", str(save_dir), "--batch_size", str(batch_size), "--size_face", str(S_FACE), "--grid", grid]
    if prompts is not None:
        argv += ["--clip_text_score", "--prompts_path", prompts]
    if ori is not None:
        argv += ["--original_imgs_dir", ori]
    lines = []
    EI.main(EI.parse_args(argv), face_provider=ScriptedProvider(), log=lines.append, cfgs=TINY)
    return lines
