"""Offline evaluation of generated images -- the reference's ``eval-generated-images.py`` (:506-568 flags, :570-709 main) on the kernels of this
package: the fourth step after train / export / generate.

    python -m finetune_fair_diffusion_amd.evaluate_images --generated_imgs_dir out --save_dir out_results \\
        --gender_classifier_weight g.pt --race_classifier_weight r.pt --age_classifier_weight a.pt

reads ``generated_imgs_dir/prompt_{i}/img_{j}.jpg`` (what ``generate.py`` writes) in numeric order and writes into ``save_dir``

  * ``test_results.pkl`` -- ``[face_indicators_all, face_bboxs_all, gender_logits_all, race_logits_all, age_logits_all]``, each a dict from prompt
    index to a CPU tensor (bool [N], int64 [N,4], float32 [N,k]): the reference's file (:696-709);
  * ``prompt_{i}.jpg`` -- the annotated grid of ``plot_in_grid_gender_race`` (:65-168; ``--grid gender_race_age``: ``plot_in_grid_gender_race_age``
    :171-263, which the reference's main carries commented out), painted on the device in one launch and saved with ``quality=25``; with
    ``--index_font PATH|default`` each tile carries its image's index as in the reference (:150-151; one more launch, ``evaluation.IndexLabels``);
  * ``metrics.json`` (build addition) -- per prompt and as a mean, exp-4's validation numbers (``evaluation.gap_metrics("exp-4", ...)``) of the three
    test classifiers' softmax table, tallied on the device (``ops.eval_tally``): 32 integers per prompt are read back for it.  With
    ``--target_distribution "gender=..;race=..;age=.."`` (training's grammar, ``--experiment custom``) it gains a ``target_gaps`` block:
    ``{gender,race,age}_gap_to_target``, half the L1 distance of the class frequencies to the given target, from the same integers.

Images are decoded on the host (PIL) by a small prefetch pool, uploaded as uint8 HWC and never converted as a whole: the face chips are cropped
straight from the bytes (``ops.crop_resize_u8``: ``u/255*2-1`` in fp32 per tap, as the reference crops its fp32 tensor) and the grid is painted from
the bytes with the reference's four fp32 roundings (``ops.eval_grid_attrs``).  An image without a face gets the all -1 chip and is classified like
the others, as in the reference (:392, :643-645); only its indicator marks it.  The reference's aligned 112x112 chips (:321-341, :401, :475) are
computed there but never used or saved; here ``--face_metrics`` (below) builds them, from the bytes as well, for the face term's two similarities.
``grid_attrs_host`` / ``grid_attrs_order`` are the plain host statements the grid kernel and the device ordering are tested against
(tests/golden/reference_evalimages_grid.npz holds the reference's own arrays); ``warp_affine_u8_host`` is that of the aligned chips.

``--original_imgs_dir DIR`` (build addition) names a second tree of the same layout, written by ``generate.py`` from the same prompts file and seed
without the LoRA files, so that ``prompt_{i}/img_{j}.jpg`` of both trees were drawn from the same noise.  Each pair is then compared the way training
regularises it: ``sim = <normalize(e_gen), normalize(e_ori)>`` of the CLIP ViT-H/14 and the DINOv2 ViT-B/14 embeddings of the ``Resize(224)`` images,
``1 - loss_CLIP`` / ``1 - loss_DINO`` of exp-1-debias-gender/1-main-debias.py:1139-1175, :1860-1862, :1905-1910.  It adds

  * ``semantics.pkl`` -- ``[sim_clip_all, sim_dino_all]``, each a dict from prompt index to a CPU float32 tensor [N] in image order;
  * ``semantics.json`` -- per prompt the mean, the minimum and the image number of the least preserved pair, and the mean over prompts
    (``semantics_summary``);

and leaves the three files above exactly as they are without it.  The encoders' weights come from ``FD_CLIP_VISION_DIR`` / ``FD_DINO_WEIGHTS`` as in
training (``--synthetic``: ``synthetic_vit_state``).

``--face_metrics`` (build addition) reports the third thing training regularises, face realism (``FairnessTrainer._face_term``, exp-1 :1917-1932): SFNet-20
features of the landmark-aligned ``--size_aligned_face`` chip of every image with a face -- ``get_face_feats``: the chip plus its mirror, summed and
L2-normalised in fp32 -- with the chips sampled straight from the bytes (``ops.warp_affine`` on the uint8 image: chips and mirrors in one launch).

  * ``sim_face_real[j]`` -- the largest dot product with a row of the real-face database, ``1 - loss_face`` of training when the target is the nearest
    real face (``nearest_face_similarity``: the search of ``FairnessTrainer.nearest_face_feats``, once per prompt);
  * ``sim_face_ori[j]`` (with ``--original_imgs_dir``) -- ``<f_gen, f_ori>`` with the original image's own face, through the same provider, alignment
    and network: ``1 - loss_face`` when the target class already matches.

An image without a face -- for ``sim_face_ori``: a pair without two faces -- holds ``nan``, not the project's -1: both quantities live in [-1, 1], where
-1 is a value a face can have.  It adds ``faces.pkl`` = ``[landmarks_all, sim_face_real_all, sim_face_ori_all]`` (prompt index -> CPU float32
[N,5,2] / [N] / [N]; landmarks of an image without a face are -1; the third dict is empty without ``--original_imgs_dir``) and ``faces.json``
(``faces_summary``), and leaves every other file as it is without it.  Weights: ``--opensphere_model_path`` / ``--face_feats_path`` as in training
(``--synthetic``: ``synthetic_face_state`` / ``synthetic_face_db``).

``--clip_text_score --prompts_path JSON`` (build addition) reports whether the images still show what their prompt asks for (CLIP-T):
``sim_clip_text[j] = <normalize(image_embeds_j), normalize(text_embeds_i)>`` of the CLIP ViT-H/14 image tower on the ``Resize(224)`` image and the same
checkpoint's text tower (``text_encoder.CLIPTextModel.text_embeds``, once per prompt) on ``test_prompts[i]`` of the JSON ``generate.py`` read, for
the folder ``prompt_{i}``; with ``--original_imgs_dir`` the originals are scored against the same text and both scores read the embeddings the pair
similarity computes, so an image passes the CLIP tower once.  It adds ``text_alignment.pkl`` = ``[sim_text_all, sim_text_ori_all]`` (prompt index ->
CPU float32 [N] in image order; the second dict is empty without originals) and ``text_alignment.json`` (``text_alignment_summary``), and leaves every
other file as it is without it.  Weights and tokenizer: ``FD_CLIP_VISION_DIR`` (``--synthetic``: ``synthetic_text_state``, ``train.HashTokenizer``).
"""
import argparse
import glob
import json
import math
import os
import pickle
import time
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import torch
import torch.nn.functional as F

from .evaluation import (LABEL_FONT_SIZE, PALETTE_GENDER, PALETTE_RACE, IndexLabels, _json_safe, draw_labels, gap_metrics, grid_attrs_shape,  # noqa: F401
                         paint_attrs_tiles)

PALETTE_AGE = [(255, 255, 255), (255, 140, 0), (0, 100, 0)]          # white / darkorange / darkgreen (:219-224), index = pred + 1
PALETTES = [PALETTE_GENDER, PALETTE_RACE, PALETTE_AGE]
ATTR_K = (2, 4, 2)                   # gender, race, age: classes of the three test classifiers (:584, :591, :598)
TABLE_ATTRS = [(0, 2), (2, 4), (6, 2)]
DECODE_THREADS = 8                   # fixed: the pool only hides JPEG decoding behind the device work, it is not sized by the machine
SYNTHETIC_SEEDS = (9101, 9102, 9103)
SYNTHETIC_VIT_SEEDS = (21, 22)       # CLIP, DINOv2
VIT_KEYS = ("clip_vision", "dino")
SYNTHETIC_TEXT_SEED = 23             # the CLIP text tower of --clip_text_score
SYNTHETIC_FACE_SEEDS = (9111, 9112)  # SFNet-20, the face database
FACE_SHORTLIST = 8                   # candidates the fp16 scores hand to the fp32 choice (FairnessTrainer.nearest_face_feats)
FACE_NET_DEFAULT = "./data/4-opensphere_checkpoints/opensphere_checkpoints/20220424_210641/models/backbone_100000.pth"
FACE_DB_DEFAULT = "./data/3-face-features/CelebA_MobileNetLarge_08240859/face_feats.pkl"


def parse_args(input_args=None):
    p = argparse.ArgumentParser(description="Script to evaluate generated images with the three test classifiers.")
    a = p.add_argument
    a("--gpu_id", type=int, default=0)
    a("--gender_classifier_weight", type=str,
      default="./data/5-trained-test-classifiers/CelebA-MobileNetLarge-Gender-09191318/epoch=19-step=25320_MobileNetLarge.pt")
    a("--race_classifier_weight", type=str,
      default="./data/5-trained-test-classifiers/fairface-MobileNetLarge-Race4-09191318/epoch=19-step=6760_MobileNetLarge.pt")
    a("--age_classifier_weight", type=str,
      default="./data/5-trained-test-classifiers/fairface-MobileNetLarge-Age2-09191319/epoch=19-step=6760_MobileNetLarge.pt")
    a("--generated_imgs_dir", type=str,
      default="./exp-3-debias-gender-race/outputs/from-paper_finetune-text-encoder_09190230/checkpoint-12200-generated-images/test_prompts_occupation")
    a("--save_dir", type=str,
      default="./exp-3-debias-gender-race/outputs/from-paper_finetune-text-encoder_09190230/checkpoint-12200-generated-images/test_prompts_occupation_results")
    a("--batch_size", type=int, default=10, help="images per launch sequence (the reference evaluates one image at a time)")
    a("--size_face", type=int, default=224)
    a("--size_aligned_face", type=int, default=112, help="side of the aligned face chips --face_metrics builds (a multiple of 16; the reference's command lines carry it)")
    a("--synthetic", action="store_true", default=False, help="(build addition) random classifier weights")
    a("--face_provider", type=str, default="synthetic", help="(build addition) 'synthetic' or 'detector', as in train.py")
    a("--grid", type=str, default="gender_race", choices=["gender_race", "gender_race_age", "off"],
      help="(build addition) which of the reference's two grids to paint; its main runs gender_race")
    # the flags below are absent from the namespace unless given (argparse.SUPPRESS): without them the arguments are the reference's plus --grid etc.
    a("--index_font", type=str, default=argparse.SUPPRESS,
      help="(build addition) PATH of a TrueType font file, or 'default' for Pillow's embedded one: print each image's index on its tile as the reference "
           "does with Arial Bold; not given: no index text")
    a("--index_font_size", type=int, default=argparse.SUPPRESS, help=f"(build addition) point size of --index_font; default {LABEL_FONT_SIZE}, the reference's")
    a("--original_imgs_dir", type=str, default=argparse.SUPPRESS,
      help="(build addition) a tree laid out like --generated_imgs_dir, generated from the same prompts and seed without the LoRA files: adds the CLIP / "
           "DINOv2 cosine similarity of every image pair (semantics.pkl, semantics.json); not given: no such files")
    a("--face_metrics", action="store_true", default=argparse.SUPPRESS,
      help="(build addition) SFNet-20 similarity of every aligned face to the nearest real face of --face_feats_path and, with --original_imgs_dir, to the "
           "original image's face (faces.pkl, faces.json); not given: no such files")
    a("--opensphere_model_path", type=str, default=argparse.SUPPRESS, help=f"(--face_metrics) SFNet-20 backbone, training's flag; default {FACE_NET_DEFAULT}")
    a("--face_feats_path", type=str, default=argparse.SUPPRESS, help=f"(--face_metrics) face_feats.pkl of real faces, training's flag; default {FACE_DB_DEFAULT}")
    a("--clip_text_score", action="store_true", default=argparse.SUPPRESS,
      help="(build addition) CLIP ViT-H/14 cosine similarity of every image to its prompt's text (CLIP-T) and, with --original_imgs_dir, of the original "
           "images to the same text (text_alignment.pkl, text_alignment.json); needs --prompts_path; not given: no such files")
    a("--prompts_path", type=str, default=argparse.SUPPRESS,
      help="(--clip_text_score) the JSON generate.py read: test_prompts[i] is the text of the folder prompt_{i}")
    a("--target_distribution", type=str, default=argparse.SUPPRESS,
      help='(build addition) "gender=0.5,0.5;race=0.4,0.2,0.2,0.2;age=0.75,0.25", training\'s grammar over the three test classifiers (an attribute that is '
           "not named gets the uniform target): adds a target_gaps block to metrics.json; not given: the file as it is without it")
    return p.parse_args(input_args) if input_args is not None else p.parse_args()


# ------------------------------------------------------------------------------------------ host statements
def grid_attrs_order(preds, probs):
    """Tile order of ``plot_in_grid_gender_race`` (:73-108; preds / probs [2, N]: gender, race) and ``plot_in_grid_gender_race_age`` (:176-187;
    [3, N]: gender, race, age): gender 1 then 0, within it race 0..3 (within that age 0, 1), each group from the most to the least confident by the
    RACE probability (two attributes) or the GENDER probability (three), then the rows with race -1 in index order.  Ties keep the index order (the
    reference's ``argsort(descending=True)`` leaves them open).  A row in no group (gender -1 with a race) is shown nowhere in the reference and
    refused here: the evaluator's predictions are never -1, and a -1 row of a caller is -1 in every attribute."""
    preds, probs = np.asarray(preds), np.asarray(probs, dtype=np.float32)
    n_attr, N = preds.shape
    assert n_attr in (2, 3) and probs.shape == preds.shape
    key = probs[1] if n_attr == 2 else probs[0]
    out = []
    for g in (1, 0):
        for r in range(4):
            for a in ((0, 1) if n_attr == 3 else (None,)):
                m = (preds[0] == g) & (preds[1] == r)
                if a is not None:
                    m &= preds[2] == a
                idx = np.nonzero(m)[0]
                out += list(idx[np.argsort(-key[idx], kind="stable")])
    out += list(np.nonzero(preds[1] == -1)[0])
    assert sorted(out) == list(range(N)), "every image must fall in exactly one (gender, race[, age]) group or have race -1"
    return np.asarray(out, dtype=np.int32)


def grid_attrs_bar_rows(probs):
    """Last row of each strip's white bar, -1 = no bar; probs [n_attr, N] fp32 (torch, any device) -> int32 [n_attr, N].  The reference draws
    ``rectangle([(0,0),(50,(1-p)*512)])`` with p a Python float when ``p < 1``; in the three-strip grid the AGE bar's condition tests the RACE
    probability (:232) while its height is age's."""
    rows = ((1 - probs.double()) * 512).to(torch.int32)
    cond = probs < 1
    if probs.shape[0] == 3:
        cond = torch.stack([cond[0], cond[1], cond[1]])
    return torch.where(cond, rows, torch.full_like(rows, -1)).contiguous()


def grid_attrs_host(images, order, boxes, preds, bar_rows, palettes):
    """The numpy statement of ``fd_eval_grid_attrs_u8``: images [N,H,W,3] uint8, order [N] tile -> image, boxes [N,4] (x0,y0,x1,y1, both ends
    drawn), preds / bar_rows [n_attr,N] (pred -1 = no face, bar_rows -1 = no bar), palettes [n_attr][(r,g,b)] indexed by pred + 1 -> uint8 grid.
    Pixels ``trunc((((u/255)*2-1)*0.5+0.5)*255)`` in fp32; outline, strips, bars, frame and the tiles past N by ``evaluation.paint_attrs_tiles``,
    which the training-side statement ``evaluation.grid_attrs_img_host`` shares."""
    images = np.asarray(images)
    x = torch.from_numpy(images).float() / 255 * 2 - 1
    return paint_attrs_tiles((x * 0.5 + 0.5).mul(255).to(torch.uint8).numpy(), order, boxes, preds, bar_rows, palettes)


def warp_affine_u8_host(u8, src_index, A, S, fill=-1.0):
    """The numpy fp64 statement of ``fd_warp_affine_u8_fwd``: u8 [B,H,W,3] uint8, src_index [n], A [n,6] (output pixel (x, y, 1) -> sampling position in
    input pixels, ``fairness.alignment_sampling_matrix``) -> chips [n,3,S,S] float64.  A tap inside the image is ``u/255*2-1``, one outside is ``fill``;
    bilinear weights from the fractional parts of the position; a ``src_index`` entry outside [0,B) gives a chip of ``fill``."""
    u8 = np.asarray(u8)
    B, H, W, _ = u8.shape
    x = u8.astype(np.float64) / 255 * 2 - 1
    A = np.asarray(A, dtype=np.float64).reshape(-1, 6)
    oy, ox = np.mgrid[0:S, 0:S]
    out = np.full((len(A), 3, S, S), float(fill))
    for k, b in enumerate(np.asarray(src_index).reshape(-1).tolist()):
        if not 0 <= b < B:
            continue
        a = A[k]
        xs, ys = a[0] * ox + a[1] * oy + a[2], a[3] * ox + a[4] * oy + a[5]
        x0, y0 = np.floor(xs), np.floor(ys)
        lx, ly = (xs - x0)[..., None], (ys - y0)[..., None]

        def tap(yy, xx):
            inside = (yy >= 0) & (yy < H) & (xx >= 0) & (xx < W)
            v = x[b][np.clip(yy, 0, H - 1).astype(np.int64), np.clip(xx, 0, W - 1).astype(np.int64)]          # [S,S,3]
            return np.where(inside[..., None], v, float(fill))
        v = (1 - ly) * ((1 - lx) * tap(y0, x0) + lx * tap(y0, x0 + 1)) + ly * ((1 - lx) * tap(y0 + 1, x0) + lx * tap(y0 + 1, x0 + 1))
        out[k] = v.transpose(2, 0, 1)
    return out


ATTR_NAMES = ("gender", "race", "age")


def parse_targets(text):
    """``--target_distribution`` over the three test classifiers (k = 2, 4, 2) -> [(name, p)], by ``fairness.parse_target_distribution``."""
    from .fairness import parse_target_distribution
    attrs = [(n, c0, k) for n, (c0, k) in zip(ATTR_NAMES, TABLE_ATTRS)]
    return list(zip(ATTR_NAMES, parse_target_distribution(text, attrs)))


def target_gaps(counts, targets):
    """``<name>_gap_to_target`` of the three test classifiers from the 32 integers of ``ops.eval_tally`` / ``evaluation.tally_host``: half the L1
    distance between the class frequencies (fp32, ``evaluation._freq``) and the target probabilities ``targets`` = [(name, p)]."""
    from .evaluation import ATTR_STRIDE, OFF_HIST, _freq, gap_to_target
    c = [int(v) for v in (counts.tolist() if hasattr(counts, "tolist") else counts)]
    out = {}
    for a, (name, p) in enumerate(targets):
        n = c[ATTR_STRIDE * a]
        out[f"{name}_gap_to_target"] = gap_to_target([_freq(c[ATTR_STRIDE * a + OFF_HIST + k], n).item() for k in range(len(p))], p)
    return out


# ------------------------------------------------------------------------------------------ device side
def _first_argmax(p):
    """(first maximum's index, maximum) per row: a tie rule the device's ``max(dim).indices`` does not promise."""
    mx = p.max(dim=-1).values
    cols = torch.arange(p.shape[1], device=p.device).expand_as(p)
    return torch.where(p == mx[:, None], cols, torch.full_like(cols, p.shape[1])).min(dim=-1).values, mx


def device_order(preds, probs):
    """``grid_attrs_order`` with torch on the tensors' device: two stable sorts (confidence, then group)."""
    n_attr = preds.shape[0]
    noface = preds[1] == -1
    group = (1 - preds[0]) * 4 + preds[1]
    if n_attr == 3:
        group = group * 2 + preds[2]
    group = torch.where(noface, torch.full_like(group, 64), group)
    key = torch.where(noface, torch.zeros_like(probs[0]), probs[1] if n_attr == 2 else probs[0])
    by_conf = torch.sort(-key, stable=True).indices
    return by_conf[torch.sort(group[by_conf], stable=True).indices].to(torch.int32).contiguous()


def device_grid(images, boxes, probs_list, which, labels=None):
    """The annotated grid (uint8 on the device) of one prompt: images [N,H,W,3] uint8, boxes [N,4] int32, probs_list = the three softmax tables
    (gender, race, age) on the device.  Predictions, bars and the tile order are torch on the device; the painting is one launch.  ``labels``: an
    ``evaluation.IndexLabels`` -- one more launch behind the painter draws the index text (:150-151, :245-246); None: no text."""
    from . import ops
    n_attr = 2 if which == "gender_race" else 3
    pm = [_first_argmax(p) for p in probs_list[:n_attr]]
    preds = torch.stack([a for a, _ in pm]).to(torch.int32).contiguous()
    probs = torch.stack([m for _, m in pm]).float().contiguous()
    P = max(len(p) for p in PALETTES[:n_attr])
    pal = torch.tensor([p + [(255, 255, 255)] * (P - len(p)) for p in PALETTES[:n_attr]], dtype=torch.uint8, device=images.device)
    order = device_order(preds, probs)
    grid = ops.eval_grid_attrs(images, order, boxes, preds, grid_attrs_bar_rows(probs), pal)
    return draw_labels(grid, order, labels, images.shape[1], images.shape[2], n_attr)


def synthetic_classifier_state(which):
    """``--synthetic``: seeded random weights of test classifier ``which`` (0 gender, 1 race, 2 age), representable in fp16."""
    from . import weights as W
    sd = W.synthetic_state_dict(W.mobilenet_param_shapes(ATTR_K[which]), seed=SYNTHETIC_SEEDS[which], gain=1.4)
    return {k: (v.half().float() if v.is_floating_point() else v) for k, v in sd.items()}


def _default_cfgs(cfgs):
    from .factory import SD15, TINY
    return cfgs or (TINY if os.environ.get("FD_TINY") else SD15)


def synthetic_vit_state(which, cfgs=None):
    """``--synthetic --original_imgs_dir``: seeded random weights of image encoder ``which`` (0 CLIP, 1 DINOv2) at the size ``cfgs`` gives it
    (default: as in ``main``), representable in fp16."""
    from . import weights as W
    sd = W.synthetic_state_dict(W.vit_param_shapes(_default_cfgs(cfgs)[VIT_KEYS[which]]), seed=SYNTHETIC_VIT_SEEDS[which])
    return {k: (v.half().float() if v.is_floating_point() else v) for k, v in sd.items()}


def _numbered(paths, number):
    return sorted(paths, key=number)


def _prompt_number(folder):
    return int(folder.split("_")[-1])


def _image_number(path):
    return int(path.split("_")[-1].split(".")[0])


def _prompt_folders(root):
    return _numbered(glob.glob(os.path.join(root, "prompt_*")), _prompt_number)


def _image_paths(folder):
    return _numbered(glob.glob(os.path.join(folder, "img_*.jpg")), _image_number)


# ------------------------------------------------------------------------------------------ semantics preservation (--original_imgs_dir)
def pair_paths(generated_dir, original_dir):
    """{prompt index: [(generated path, original path), ...]} in the evaluator's numeric order: every ``prompt_i/img_j.jpg`` of the generated tree
    with the file at the same relative path of the original tree.  A generated image without its counterpart is refused; what the original tree
    holds beyond that is ignored."""
    pairs, missing = {}, []
    for folder in _prompt_folders(generated_dir):
        paths = _image_paths(folder)
        if not paths:
            continue
        ori = [os.path.join(original_dir, os.path.relpath(p, generated_dir)) for p in paths]
        missing += [o for o in ori if not os.path.isfile(o)]
        pairs[_prompt_number(folder)] = list(zip(paths, ori))
    if missing:
        raise ValueError(f"--original_imgs_dir: {missing[0]} is missing ({len(missing)} of the generated tree's images have no counterpart at the same "
                         "relative path; both trees must come from the same prompts file and seed)")
    return pairs


def semantics_summary(sims_by_prompt, image_numbers_by_prompt):
    """The content of ``semantics.json`` from the content of ``semantics.pkl``: ``sims_by_prompt`` = [sim_clip_all, sim_dino_all] ({prompt index:
    [N] similarities in image order}), ``image_numbers_by_prompt`` = {prompt index: the N numbers ``j`` of ``img_j.jpg``}.  ``argmin_*`` is the image
    NUMBER of the least preserved pair (the first one on a tie); ``mean`` is the mean over prompts of the per-prompt means, as in ``metrics.json``."""
    per = {}
    for i, numbers in image_numbers_by_prompt.items():
        row = {}
        for name, sims in zip(("CLIP", "DINO"), sims_by_prompt):
            s = np.asarray(sims[i], dtype=np.float64).reshape(-1)
            assert len(s) == len(numbers) and len(s) > 0, (i, name, len(s), len(numbers))
            row["sim_" + name], row["min_sim_" + name], row["argmin_" + name] = float(s.mean()), float(s.min()), int(numbers[int(s.argmin())])
        per[str(i)] = {f"{k}_{name}": row[f"{k}_{name}"] for k in ("sim", "min_sim", "argmin") for name in ("CLIP", "DINO")}
        per[str(i)]["pairs"] = len(numbers)
    mean = {k: float(np.array([m[k] for m in per.values()]).mean()) for k in (("sim_CLIP", "sim_DINO") if per else ())}
    return _json_safe({"per_prompt": per, "mean": mean})


def _resize_full(u8, S):
    """``transforms.Resize(S)`` of whole decoded images [n,H,W,3] uint8 -> [n,3,S,S] working dtype: the crop kernel on the full-image box, what
    ``FairnessTrainer.resize_small`` does to training's images."""
    from . import ops
    n, H, W, _ = u8.shape
    box = torch.tensor([[0, 0, W, H]] * n, dtype=torch.int32, device=u8.device)
    return ops.crop_resize_u8(u8, box, -1.0, S)


def embedding_similarity(e_gen, e_ori):
    """``<normalize(e_gen), normalize(e_ori)>`` per row in fp32: one minus the ``loss`` of ``vit.feature_loss_and_grad(e_gen, normalize(e_ori), w)``."""
    return (F.normalize(e_gen.float(), dim=-1) * F.normalize(e_ori.float(), dim=-1)).sum(-1)


def pair_similarity(clip, dino, u8_gen, u8_ori):
    """``1 - loss_CLIP`` and ``1 - loss_DINO`` of the training step (:1905-1910) for n pairs of decoded images: u8_gen [n,H,W,3], u8_ori [n,H',W',3]
    uint8 on the device, ``clip`` / ``dino`` the two ``vit.VisionTransformer`` -> (sim_clip [n], sim_dino [n]) fp32 on the device.  Images of one
    size go through each encoder as one batch of 2n; an encoder input size is resized once."""
    n = u8_gen.shape[0]
    e_clip, e_dino = pair_embeddings(clip, dino, u8_gen, u8_ori)
    return embedding_similarity(e_clip[:n], e_clip[n:]), embedding_similarity(e_dino[:n], e_dino[n:])


def pair_embeddings(clip, dino, u8_gen, u8_ori):
    """The embeddings ``pair_similarity`` compares: (e_clip [2n,E], e_dino [2n,E']) fp32 on the device, the n generated images' rows first.  With
    ``--clip_text_score`` the text score reads the CLIP rows too, so that an image passes the CLIP tower once."""
    n = u8_gen.shape[0]
    assert u8_ori.shape[0] == n and n >= 1, (u8_gen.shape, u8_ori.shape)
    groups = [torch.cat([u8_gen, u8_ori])] if u8_gen.shape == u8_ori.shape else [u8_gen, u8_ori]
    chips, embeds = {}, []
    for enc in (clip, dino):
        S = enc.config.image_size
        if S not in chips:
            chips[S] = [_resize_full(u, S) for u in groups]
        embeds.append(torch.cat([enc.forward(c) for c in chips[S]]))
    return embeds[0], embeds[1]


def _load_encoder(args, cfgs, device, which):
    """Image encoder ``which`` (0 CLIP, 1 DINOv2) with the weights of the run."""
    from . import weights as W
    from .vit import VisionTransformer
    key = VIT_KEYS[which]
    if args.synthetic:
        sd = synthetic_vit_state(which, cfgs)
    elif which == 0:
        from .pretrained import load_clip_vision
        sd = load_clip_vision(os.environ["FD_CLIP_VISION_DIR"], cfgs[key])
    else:
        from .pretrained import load_dino
        sd = load_dino(os.environ["FD_DINO_WEIGHTS"], cfgs[key])
    mean, std = ((W.CLIP_IMAGE_MEAN, W.CLIP_IMAGE_STD), (W.DINO_IMAGE_MEAN, W.DINO_IMAGE_STD))[which]
    return VisionTransformer(cfgs[key], sd, device, mean, std)


def _load_encoders(args, cfgs, device):
    return _load_encoder(args, cfgs, device, 0), _load_encoder(args, cfgs, device, 1)


# ------------------------------------------------------------------------------------------ text-image alignment (--clip_text_score)
def synthetic_text_state(cfgs=None):
    """``--synthetic --clip_text_score``: seeded random weights of the CLIP text tower at the size ``cfgs`` gives it (default: as in ``main``),
    representable in fp16."""
    from . import weights as W
    sd = W.synthetic_state_dict(W.clip_param_shapes(_default_cfgs(cfgs)["clip_text_h"]), seed=SYNTHETIC_TEXT_SEED)
    return {k: v.half().float() for k, v in sd.items()}


def load_prompts(path):
    """``test_prompts`` of the JSON ``generate.py`` reads: ``test_prompts[i]`` is the text of the folder ``prompt_{i}``."""
    with open(path, "r") as f:
        prompts = json.load(f)["test_prompts"]
    if not isinstance(prompts, list) or not all(isinstance(p, str) for p in prompts):
        raise ValueError(f"--prompts_path {path}: test_prompts must be a list of strings")
    return prompts


def folder_prompts(generated_dir, prompts):
    """{prompt index: text} of the ``prompt_{i}`` folders of ``generated_dir`` in numeric order; a folder beyond the prompt list is refused."""
    idx = [_prompt_number(f) for f in _prompt_folders(generated_dir)]
    beyond = [i for i in idx if not 0 <= i < len(prompts)]
    if beyond:
        raise ValueError(f"--prompts_path: the folder prompt_{beyond[0]} has no text, the file holds {len(prompts)} test_prompts "
                         "(the tree must come from this prompts file)")
    return {i: prompts[i] for i in idx}


def tokenize_prompts(texts, cfg, synthetic, model_dir=None):
    """Token ids [len(texts), max_position_embeddings] int64 on the host.  Real runs: the checkpoint directory's own ``CLIPTokenizer``, padded to the
    full length, truncation on (the end-of-text token survives truncation).  ``synthetic``: ``train.HashTokenizer`` on the tower's vocabulary (begin,
    words, end-of-text = the largest id), padded with id 0."""
    T = cfg.max_position_embeddings
    if not texts:
        return torch.zeros((0, T), dtype=torch.int64)
    if synthetic:
        from .train import HashTokenizer
        tok = HashTokenizer(cfg.vocab_size, max_len=T)
        ids = torch.zeros((len(texts), T), dtype=torch.int64)
        for r, text in enumerate(texts):
            row = tok(text)[0]
            ids[r, :len(row)] = row
        return ids
    from transformers import CLIPTokenizer
    tok = CLIPTokenizer.from_pretrained(model_dir)
    return tok(list(texts), return_tensors="pt", padding="max_length", truncation=True, max_length=T).input_ids.to(torch.int64)


def _text_inputs(args, cfgs):
    """Everything ``--clip_text_score`` needs from the host, with its refusals: -> ({prompt index: text}, {prompt index: ids [1,T]}, text tower's state
    dict).  Nothing here touches the device or ``save_dir``."""
    path = getattr(args, "prompts_path", None)
    if path is None:
        raise ValueError("--clip_text_score needs --prompts_path (the JSON generate.py read: test_prompts[i] is the text of prompt_{i})")
    if not os.path.isfile(path):
        raise FileNotFoundError(f"--prompts_path {path}: no such file")
    texts = folder_prompts(args.generated_imgs_dir, load_prompts(path))
    cfg = cfgs["clip_text_h"]
    if args.synthetic:
        sd, model_dir = synthetic_text_state(cfgs), None
    else:
        model_dir = os.environ.get("FD_CLIP_VISION_DIR")
        if not model_dir:
            raise FileNotFoundError("--clip_text_score needs FD_CLIP_VISION_DIR (CLIP ViT-H/14 directory: its checkpoint carries the text tower and its "
                                    "tokenizer files; pass --synthetic for synthetic weights)")
        from .pretrained import load_clip_text
        sd = load_clip_text(model_dir, cfg)          # KeyError on a checkpoint without the text tower
    ids = tokenize_prompts(list(texts.values()), cfg, args.synthetic, model_dir)
    return texts, {i: ids[r:r + 1] for r, i in enumerate(texts)}, sd


def text_alignment(clip_vision, clip_text, u8, input_ids):
    """CLIP-T of decoded images: u8 [n,H,W,3] uint8 on the device, input_ids [1,T] (one text for all images) or [n,T] int64 on the host ->
    ``<normalize(image_embeds), normalize(text_embeds)>`` [n] fp32 on the device.  The image side is ``pair_similarity``'s: ``Resize`` from the bytes,
    then the CLIP image tower; the text side is ``CLIPTextModel.text_embeds``."""
    e = clip_vision.forward(_resize_full(u8, clip_vision.config.image_size))
    return embedding_similarity(e, clip_text.text_embeds(input_ids))


def text_alignment_summary(sims, image_numbers_by_prompt, texts):
    """The content of ``text_alignment.json`` from the content of ``text_alignment.pkl``: ``sims`` = [sim_text_all, sim_text_ori_all] ({prompt index:
    [N] similarities in image order}; the second dict empty without ``--original_imgs_dir``), ``image_numbers_by_prompt`` = {prompt index: the N
    numbers ``j`` of ``img_j.jpg``}, ``texts`` = {prompt index: text}.  ``argmin_clip_t`` is the image NUMBER of the least aligned image (the first one
    on a tie); ``clip_t_delta = clip_t - clip_t_ori``; ``mean`` is the mean over prompts of the per-prompt means, as in ``metrics.json``."""
    sim_all, ori_all = sims
    per = {}
    for i, numbers in image_numbers_by_prompt.items():
        s = np.asarray(sim_all[i], dtype=np.float64).reshape(-1)
        assert len(s) == len(numbers) and len(s) > 0, (i, len(s), len(numbers))
        row = {"prompt": texts[i], "clip_t": float(s.mean()), "min_clip_t": float(s.min()), "argmin_clip_t": int(numbers[int(s.argmin())])}
        if ori_all:
            o = np.asarray(ori_all[i], dtype=np.float64).reshape(-1)
            assert len(o) == len(numbers), (i, len(o), len(numbers))
            row["clip_t_ori"] = float(o.mean())
            row["clip_t_delta"] = row["clip_t"] - row["clip_t_ori"]
        per[str(i)] = row
    keys = (("clip_t", "clip_t_ori", "clip_t_delta") if ori_all else ("clip_t",)) if per else ()
    mean = {k: float(np.array([m[k] for m in per.values()]).mean()) for k in keys}
    return _json_safe({"per_prompt": per, "mean": mean})


# ------------------------------------------------------------------------------------------ face realism and identity (--face_metrics)
def synthetic_face_state(size_aligned_face=112):
    """``--synthetic --face_metrics``: seeded random SFNet-20 weights for chips of ``size_aligned_face``, made as ``factory.build_trainer`` makes them."""
    from . import weights as W
    return W.synthetic_state_dict(W.sfnet20_param_shapes(in_size=size_aligned_face), seed=SYNTHETIC_FACE_SEEDS[0])


def synthetic_face_db():
    """``--synthetic --face_metrics``: 4096 seeded random unit vectors [4096,512] fp32, the stand-in of ``face_feats.pkl`` in ``factory.build_trainer``."""
    return F.normalize(torch.randn(4096, 512, generator=torch.Generator().manual_seed(SYNTHETIC_FACE_SEEDS[1])), dim=-1)


def _face_weight_paths(args):
    """(SFNet path, database path) of a ``--face_metrics`` run with real weights; a missing file is refused here, before any device work or output."""
    net, db = getattr(args, "opensphere_model_path", FACE_NET_DEFAULT), getattr(args, "face_feats_path", FACE_DB_DEFAULT)
    missing = [f"--{flag} {path}" for flag, path in (("opensphere_model_path", net), ("face_feats_path", db)) if not os.path.isfile(path)]
    if missing:
        raise FileNotFoundError("--face_metrics needs the SFNet-20 backbone and the real-face feature file of training's face term; not found: "
                                + ", ".join(missing) + " (pass --synthetic for synthetic weights)")
    return net, db


def _load_face_models(args, device):
    """-> (SFNet20, database [M,512] fp32 unit rows on the device, its working-dtype copy for the MFMA scores)"""
    from . import ops
    from .sfnet import SFNet20
    S = args.size_aligned_face
    if args.synthetic:
        sd, db = synthetic_face_state(S), synthetic_face_db()
    else:
        from .pretrained import load_face_db, load_face_net
        net_path, db_path = _face_weight_paths(args)
        sd, db = load_face_net(net_path, in_size=S), load_face_db(db_path)
    db = F.normalize(db.to(device, torch.float32), dim=-1).contiguous()
    return SFNet20(sd, device, in_size=S), db, db.to(ops.F16).contiguous()


def face_features_u8(face_net, u8_d, ind, landmarks, S):
    """``get_face_feats`` (:1176-1190) of the images with a face, from the bytes: u8_d [b,H,W,3] uint8 on the device, ind [b] bool and landmarks
    [b,5,2] (x, y) on the host -> (rows: the images with a face, features [len(rows),512] fp32 unit vectors on the device), or ``([], None)`` when
    no image has one (nothing is launched then).  One launch makes the aligned chips and their mirrors; SFNet runs on both and the sum is
    L2-normalised in fp32."""
    from . import ops
    from .fairness import alignment_sampling_matrix
    rows = ind.nonzero().view(-1).tolist()
    if not rows:
        return rows, None
    H, W = u8_d.shape[1:3]
    A = np.stack([alignment_sampling_matrix(landmarks[i].numpy(), H, W, S) for i in rows])
    A = torch.tensor(A, dtype=torch.float32).to(u8_d.device)
    idx = torch.tensor(rows, dtype=torch.int32).to(u8_d.device)
    chips, mirrored = ops.warp_affine(u8_d, idx, A, S, mirror=True)
    return rows, F.normalize(face_net.forward(chips).float() + face_net.forward(mirrored).float(), dim=-1)


def nearest_face_similarity(db, db16, query):
    """Largest dot product of each query [n,512] (fp32 unit rows on the device) with a row of the database ``db`` [M,512] fp32 (``db16``: its
    working-dtype copy) -> [n] fp32: ``FaceFeatsModel.semantic_search`` (:98-117) as ``FairnessTrainer.nearest_face_feats`` runs it -- working-dtype MFMA
    scores shortlist 8 rows per query, the winner is chosen among them in fp32 -- returning the winner's similarity instead of its row."""
    from . import ops
    n, M = query.shape[0], db.shape[0]
    q16 = torch.zeros(((n + 7) // 8 * 8, query.shape[1]), dtype=ops.F16, device=query.device)
    q16[:n] = query.to(ops.F16)
    scores = ops.gemm(db16, q16, out_dtype=torch.float32)[:, :n].t()            # [n, M]
    cand = scores.topk(min(FACE_SHORTLIST, M), dim=-1).indices
    return (db[cand] * query[:, None, :]).sum(dim=-1).max(dim=-1).values


def faces_summary(faces, image_numbers_by_prompt):
    """The content of ``faces.json`` from the content of ``faces.pkl``: ``faces`` = [landmarks_all, sim_face_real_all, sim_face_ori_all] ({prompt
    index: [N,5,2] / [N] / [N]}, ``nan`` = no face / no two-face pair; the third dict empty without ``--original_imgs_dir``),
    ``image_numbers_by_prompt`` = {prompt index: the N numbers ``j`` of ``img_j.jpg``}.  Per prompt: ``faces`` (rows with a similarity to a real
    face) and, over the rows that have the value, ``sim_face_*`` (mean), ``min_sim_face_*`` and ``argmin_face_*`` (the image NUMBER of the minimum, the
    first one on a tie), null when no row has it; with originals also ``pairs`` (rows with two faces).  ``mean``: per quantity the mean of the per-prompt
    means over the prompts that have one, null when none has."""
    _, real_all, ori_all = faces
    names = [("real", real_all)] + ([("ori", ori_all)] if ori_all else [])
    per = {}
    for i, numbers in image_numbers_by_prompt.items():
        row = {}
        for name, sims in names:
            s = np.asarray(sims[i], dtype=np.float64).reshape(-1)
            assert len(s) == len(numbers), (i, name, len(s), len(numbers))
            have = np.nonzero(~np.isnan(s))[0]
            row["faces" if name == "real" else "pairs"] = int(len(have))
            if len(have):
                first_min = have[int(s[have].argmin())]
                row["sim_face_" + name], row["min_sim_face_" + name], row["argmin_face_" + name] = float(s[have].mean()), float(s[first_min]), int(numbers[first_min])
            else:
                row["sim_face_" + name] = row["min_sim_face_" + name] = row["argmin_face_" + name] = None
        per[str(i)] = row
    mean = {}
    for name, _ in names:
        vals = [m["sim_face_" + name] for m in per.values() if m["sim_face_" + name] is not None]
        mean["sim_face_" + name] = float(np.mean(vals)) if vals else None
    return _json_safe({"per_prompt": per, "mean": mean})


def _same_size(u, size, path):
    if u.shape != size:
        raise ValueError(f"{path}: image of {u.shape[1]}x{u.shape[0]} in a prompt folder of {size[1]}x{size[0]} images "
                         "(the images of one prompt must share one size)")


def _decode(path):
    from PIL import Image
    with Image.open(path) as im:
        return np.asarray(im.convert("RGB"))


def main(args, face_provider=None, log=print, cfgs=None):
    face_metrics = bool(getattr(args, "face_metrics", False))
    if face_metrics and not args.synthetic:          # refused before any device work and before anything is written
        _face_weight_paths(args)
    text_score = bool(getattr(args, "clip_text_score", False))
    if text_score:          # its refusals are host work: before any device work and before anything is written
        texts, text_ids, text_sd = _text_inputs(args, _default_cfgs(cfgs))
    targets = parse_targets(args.target_distribution) if getattr(args, "target_distribution", None) is not None else None      # refused before any device work
    gaps = {}
    if not torch.cuda.is_available():
        raise RuntimeError("finetune_fair_diffusion_amd.evaluate_images needs an MI355X (HIP device); there is no CPU path")
    original_dir = getattr(args, "original_imgs_dir", None)
    pairs = None
    if original_dir is not None:          # both refusals come before any device work and before anything is written
        if not args.synthetic and not (os.environ.get("FD_CLIP_VISION_DIR") and os.environ.get("FD_DINO_WEIGHTS")):
            raise FileNotFoundError("--original_imgs_dir needs FD_CLIP_VISION_DIR (CLIP ViT-H/14 directory) and FD_DINO_WEIGHTS "
                                    "(dinov2_vitb14_pretrain.pth), as training's image regularisers do (pass --synthetic for synthetic weights)")
        pairs = pair_paths(args.generated_imgs_dir, original_dir)
    from PIL import Image
    from . import ops
    from .classifier import MobileNetV3Large
    device = torch.device("cuda", args.gpu_id)
    torch.cuda.set_device(device)
    if face_provider is None:
        if args.face_provider == "detector":
            from .fairness import DetectorFaceProvider
            face_provider = DetectorFaceProvider.from_installed()
        elif args.face_provider == "synthetic":
            from .fairness import SyntheticFaceProvider
            face_provider = SyntheticFaceProvider()
        else:
            raise ValueError(f"--face_provider {args.face_provider}: 'synthetic' or 'detector'")
    if args.batch_size < 1:
        raise ValueError(f"--batch_size {args.batch_size}: at least 1")
    classifiers = []
    for which, path in enumerate((args.gender_classifier_weight, args.race_classifier_weight, args.age_classifier_weight)):
        if args.synthetic:
            sd = synthetic_classifier_state(which)
        else:
            from .pretrained import load_classifier
            sd = load_classifier(path, ATTR_K[which])
        classifiers.append(MobileNetV3Large(sd, device, ATTR_K[which]))
    clip, dino = _load_encoders(args, _default_cfgs(cfgs), device) if pairs is not None else (None, None)
    if text_score:
        from .text_encoder import CLIPTextModel
        if clip is None:
            clip = _load_encoder(args, _default_cfgs(cfgs), device, 0)
        clip_text = CLIPTextModel(_default_cfgs(cfgs)["clip_text_h"], text_sd, device)
        del text_sd
    face_net, face_db, face_db16 = _load_face_models(args, device) if face_metrics else (None, None, None)

    labels = IndexLabels(args.index_font, getattr(args, "index_font_size", LABEL_FONT_SIZE)) if getattr(args, "index_font", None) and args.grid != "off" else None
    folders = _prompt_folders(args.generated_imgs_dir)
    os.makedirs(args.save_dir, exist_ok=True)
    results = [{}, {}, {}, {}, {}]          # indicators, boxes, gender / race / age logits
    metrics = {}
    semantics, numbers = [{}, {}], {}       # CLIP / DINOv2 similarities and the image numbers they belong to (--original_imgs_dir)
    text_sims = [{}, {}]                    # CLIP similarity to the prompt's text of the generated and of the original images (--clip_text_score)
    faces, n_chips = [{}, {}, {}], 0        # landmarks, similarity to the nearest real face, to the original's face (--face_metrics)
    S_al = args.size_aligned_face
    n_images, t0 = 0, time.time()
    with ThreadPoolExecutor(max_workers=DECODE_THREADS) as pool:
        for folder in folders:
            prompt_idx = _prompt_number(folder)
            paths = _image_paths(folder)
            if not paths:
                continue
            decoded = pool.map(_decode, paths)          # submitted now, consumed in order: decoding runs ahead of the device work
            imgs_d, ind_p, boxes_p, logits_p = [], [], [], [[], [], []]
            size = None
            if pairs is not None:
                paths_o = [o for _, o in pairs[prompt_idx]]
                assert [g for g, _ in pairs[prompt_idx]] == paths, (prompt_idx, "the generated tree changed after it was paired")
                decoded_o, size_o, sims_p = pool.map(_decode, paths_o), None, []
            if text_score:          # the text tower runs once per prompt
                e_text, tsims_p = clip_text.text_embeds(text_ids[prompt_idx]).float(), []
            if face_metrics:          # per prompt: unit features [N,512] of the generated and the original faces, nan rows where there is none
                lms_p = []
                feats_g = torch.full((len(paths), 512), float("nan"), dtype=torch.float32, device=device)
                feats_o = torch.full_like(feats_g, float("nan")) if pairs is not None else None
            for b0 in range(0, len(paths), args.batch_size):
                bp = paths[b0:b0 + args.batch_size]
                batch = []
                for path in bp:
                    u = next(decoded)
                    if size is None:
                        size = u.shape
                    _same_size(u, size, path)
                    batch.append(u)
                u8 = torch.from_numpy(np.stack(batch))                       # [b,H,W,3] uint8
                u8_d = u8.to(device, non_blocking=False)
                x = u8.permute(0, 3, 1, 2).float() / 255 * 2 - 1      # what the reference hands get_face (:637-639); one object: a detector provider caches by identity
                ind, boxes = face_provider(x)
                ind = torch.as_tensor(ind, dtype=torch.bool).cpu()
                boxes = torch.as_tensor(boxes).to("cpu", torch.int32)
                boxes = torch.where(ind[:, None], boxes, torch.full_like(boxes, -1)).contiguous()
                chips = ops.crop_resize_u8(u8_d, boxes.to(device), -1.0, args.size_face)
                for k, clf in enumerate(classifiers):
                    logits_p[k].append(clf(chips).float())
                if pairs is not None:
                    batch_o = []
                    for path in paths_o[b0:b0 + args.batch_size]:
                        u = next(decoded_o)
                        if size_o is None:
                            size_o = u.shape
                        _same_size(u, size_o, path)
                        batch_o.append(u)
                    u8_o = torch.from_numpy(np.stack(batch_o))
                    u8_od = u8_o.to(device)
                    e_clip, e_dino = pair_embeddings(clip, dino, u8_d, u8_od)          # generated rows, then the originals'
                    b = len(bp)
                    sims_p.append(torch.stack([embedding_similarity(e_clip[:b], e_clip[b:]), embedding_similarity(e_dino[:b], e_dino[b:])]))
                    if text_score:          # the embeddings the pair similarity just used: each image passes the CLIP tower once
                        tsims_p.append(torch.stack([embedding_similarity(e_clip[:b], e_text), embedding_similarity(e_clip[b:], e_text)]))
                elif text_score:
                    tsims_p.append(embedding_similarity(clip.forward(_resize_full(u8_d, clip.config.image_size)), e_text)[None])
                if face_metrics:
                    lms = torch.as_tensor(face_provider.landmarks(x)).to("cpu", torch.float32)
                    lms_p.append(torch.where(ind[:, None, None], lms, torch.full_like(lms, -1.0)))
                    rows, f = face_features_u8(face_net, u8_d, ind, lms, S_al)
                    if rows:
                        feats_g[torch.tensor(rows, device=device) + b0] = f
                        n_chips += len(rows)
                    if pairs is not None:          # the original images through the same provider, alignment and network
                        x_o = u8_o.permute(0, 3, 1, 2).float() / 255 * 2 - 1
                        ind_o = torch.as_tensor(face_provider(x_o)[0], dtype=torch.bool).cpu()
                        rows, f = face_features_u8(face_net, u8_od, ind_o, torch.as_tensor(face_provider.landmarks(x_o)).to("cpu", torch.float32), S_al)
                        if rows:
                            feats_o[torch.tensor(rows, device=device) + b0] = f
                            n_chips += len(rows)
                imgs_d.append(u8_d)
                ind_p.append(ind)
                boxes_p.append(boxes)
            imgs_d = torch.cat(imgs_d)
            ind, boxes = torch.cat(ind_p), torch.cat(boxes_p)
            logits = [torch.cat(l) for l in logits_p]
            probs = [torch.softmax(l, dim=-1) for l in logits]
            table = torch.cat(probs, dim=1)
            table = torch.where(ind.to(device)[:, None], table, torch.full_like(table, -1.0)).contiguous()
            counts = ops.eval_tally(table, TABLE_ATTRS).cpu()
            metrics[prompt_idx] = gap_metrics("exp-4", counts)
            if targets is not None:          # from the integers already read back
                gaps[prompt_idx] = target_gaps(counts, targets)
            if args.grid != "off":
                grid = device_grid(imgs_d, boxes.to(device), probs, args.grid, labels=labels).cpu().numpy()
                Image.fromarray(grid).save(os.path.join(args.save_dir, f"prompt_{prompt_idx}.jpg"), quality=25)
            results[0][prompt_idx] = ind
            results[1][prompt_idx] = boxes.to(torch.int64)
            for k in range(3):
                results[2 + k][prompt_idx] = logits[k].cpu()
            if pairs is not None:
                sims = torch.cat(sims_p, dim=1).cpu()          # [2, N] fp32: the prompt's one copy
                semantics[0][prompt_idx], semantics[1][prompt_idx] = sims[0].clone(), sims[1].clone()
            if text_score:
                tsims = torch.cat(tsims_p, dim=1).cpu()          # [1 or 2, N] fp32: the prompt's one copy
                text_sims[0][prompt_idx] = tsims[0].clone()
                if pairs is not None:
                    text_sims[1][prompt_idx] = tsims[1].clone()
            if pairs is not None or face_metrics or text_score:
                numbers[prompt_idx] = [_image_number(p) for p in paths]
            if face_metrics:
                have = ind.nonzero().view(-1).to(device)
                sim_real = torch.full((len(paths),), float("nan"), dtype=torch.float32, device=device)
                if len(have):          # one search per prompt
                    sim_real[have] = nearest_face_similarity(face_db, face_db16, feats_g[have])
                faces[0][prompt_idx], faces[1][prompt_idx] = torch.cat(lms_p), sim_real.cpu()
                if pairs is not None:
                    faces[2][prompt_idx] = (feats_g * feats_o).sum(dim=-1).cpu()          # nan unless both images have a face
            n_images += len(paths)
    with open(os.path.join(args.save_dir, "test_results.pkl"), "wb") as f:
        pickle.dump(results, f)
    keys = list(next(iter(metrics.values())).keys()) if metrics else []
    out = {"per_prompt": {str(i): m for i, m in metrics.items()},
           "mean": {k: float(np.array([m[k] for m in metrics.values()]).mean()) for k in keys}}
    if targets is not None:
        gkeys = list(next(iter(gaps.values())).keys()) if gaps else []
        out["target_gaps"] = {"targets": {n: list(p) for n, p in targets}, "per_prompt": {str(i): g for i, g in gaps.items()},
                              "mean": {k: float(np.array([g[k] for g in gaps.values()]).mean()) for k in gkeys}}
    with open(os.path.join(args.save_dir, "metrics.json"), "w") as f:
        json.dump(_json_safe(out), f, indent=1)
    if pairs is not None:
        with open(os.path.join(args.save_dir, "semantics.pkl"), "wb") as f:
            pickle.dump(semantics, f)
        with open(os.path.join(args.save_dir, "semantics.json"), "w") as f:
            json.dump(semantics_summary(semantics, numbers), f, indent=1)
    if face_metrics:
        with open(os.path.join(args.save_dir, "faces.pkl"), "wb") as f:
            pickle.dump(faces, f)
        with open(os.path.join(args.save_dir, "faces.json"), "w") as f:
            json.dump(faces_summary(faces, numbers), f, indent=1)
    if text_score:
        with open(os.path.join(args.save_dir, "text_alignment.pkl"), "wb") as f:
            pickle.dump(text_sims, f)
        with open(os.path.join(args.save_dir, "text_alignment.json"), "w") as f:
            json.dump(text_alignment_summary(text_sims, numbers, texts), f, indent=1)
    dt = time.time() - t0
    if log is not None:
        line = {"evaluated_images": n_images, "prompts": len(metrics), "seconds": round(dt, 3), "images_per_s": round(n_images / dt, 2) if dt > 0 else None}
        if pairs is not None:
            line["semantics_pairs"] = n_images
        if face_metrics:
            line["face_chips"] = n_chips
        if text_score:
            line["text_prompts"] = len(text_sims[0])
        log(json.dumps(line))
    return results, out


if __name__ == "__main__":
    main(parse_args())
