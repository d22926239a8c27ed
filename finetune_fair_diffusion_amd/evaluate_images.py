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
    test classifiers' softmax table, tallied on the device (``ops.eval_tally``): 32 integers per prompt are read back for it.

Images are decoded on the host (PIL) by a small prefetch pool, uploaded as uint8 HWC and never converted as a whole: the face chips are cropped
straight from the bytes (``ops.crop_resize_u8``: ``u/255*2-1`` in fp32 per tap, as the reference crops its fp32 tensor) and the grid is painted from
the bytes with the reference's four fp32 roundings (``ops.eval_grid_attrs``).  An image without a face gets the all -1 chip and is classified like
the others, as in the reference (:392, :643-645); only its indicator marks it.  The reference's aligned 112x112 chips are computed there but never
saved: they are not built.  ``grid_attrs_host`` / ``grid_attrs_order`` are the plain host statements the grid kernel and the device ordering are
tested against (tests/golden/reference_evalimages_grid.npz holds the reference's own arrays).

``--original_imgs_dir DIR`` (build addition) names a second tree of the same layout, written by ``generate.py`` from the same prompts file and seed
without the LoRA files, so that ``prompt_{i}/img_{j}.jpg`` of both trees were drawn from the same noise.  Each pair is then compared the way training
regularises it: ``sim = <normalize(e_gen), normalize(e_ori)>`` of the CLIP ViT-H/14 and the DINOv2 ViT-B/14 embeddings of the ``Resize(224)`` images,
``1 - loss_CLIP`` / ``1 - loss_DINO`` of exp-1-debias-gender/1-main-debias.py:1139-1175, :1860-1862, :1905-1910.  It adds

  * ``semantics.pkl`` -- ``[sim_clip_all, sim_dino_all]``, each a dict from prompt index to a CPU float32 tensor [N] in image order;
  * ``semantics.json`` -- per prompt the mean, the minimum and the image number of the least preserved pair, and the mean over prompts
    (``semantics_summary``);

and leaves the three files above exactly as they are without it.  The encoders' weights come from ``FD_CLIP_VISION_DIR`` / ``FD_DINO_WEIGHTS`` as in
training (``--synthetic``: ``synthetic_vit_state``).
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
    a("--size_aligned_face", type=int, default=112, help="accepted for the reference's command lines; the aligned chips are not built")
    a("--synthetic", action="store_true", default=False, help="(build addition) random classifier weights")
    a("--face_provider", type=str, default="synthetic", help="(build addition) 'synthetic' or 'detector', as in train.py")
    a("--grid", type=str, default="gender_race", choices=["gender_race", "gender_race_age", "off"],
      help="(build addition) which of the reference's two grids to paint; its main runs gender_race")
    # the three flags below are absent from the namespace unless given (argparse.SUPPRESS): without them the arguments are the reference's plus --grid etc.
    a("--index_font", type=str, default=argparse.SUPPRESS,
      help="(build addition) PATH of a TrueType font file, or 'default' for Pillow's embedded one: print each image's index on its tile as the reference "
           "does with Arial Bold; not given: no index text")
    a("--index_font_size", type=int, default=argparse.SUPPRESS, help=f"(build addition) point size of --index_font; default {LABEL_FONT_SIZE}, the reference's")
    a("--original_imgs_dir", type=str, default=argparse.SUPPRESS,
      help="(build addition) a tree laid out like --generated_imgs_dir, generated from the same prompts and seed without the LoRA files: adds the CLIP / "
           "DINOv2 cosine similarity of every image pair (semantics.pkl, semantics.json); not given: no such files")
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
    assert u8_ori.shape[0] == n and n >= 1, (u8_gen.shape, u8_ori.shape)
    groups = [torch.cat([u8_gen, u8_ori])] if u8_gen.shape == u8_ori.shape else [u8_gen, u8_ori]
    chips, sims = {}, []
    for enc in (clip, dino):
        S = enc.config.image_size
        if S not in chips:
            chips[S] = [_resize_full(u, S) for u in groups]
        e = torch.cat([enc.forward(c) for c in chips[S]])
        sims.append(embedding_similarity(e[:n], e[n:]))
    return sims[0], sims[1]


def _load_encoders(args, cfgs, device):
    from . import weights as W
    from .vit import VisionTransformer
    if args.synthetic:
        sds = [synthetic_vit_state(k, cfgs) for k in range(2)]
    else:
        from .pretrained import load_clip_vision, load_dino
        sds = [load_clip_vision(os.environ["FD_CLIP_VISION_DIR"], cfgs["clip_vision"]), load_dino(os.environ["FD_DINO_WEIGHTS"], cfgs["dino"])]
    return (VisionTransformer(cfgs["clip_vision"], sds[0], device, W.CLIP_IMAGE_MEAN, W.CLIP_IMAGE_STD),
            VisionTransformer(cfgs["dino"], sds[1], device, W.DINO_IMAGE_MEAN, W.DINO_IMAGE_STD))


def _same_size(u, size, path):
    if u.shape != size:
        raise ValueError(f"{path}: image of {u.shape[1]}x{u.shape[0]} in a prompt folder of {size[1]}x{size[0]} images "
                         "(the images of one prompt must share one size)")


def _decode(path):
    from PIL import Image
    with Image.open(path) as im:
        return np.asarray(im.convert("RGB"))


def main(args, face_provider=None, log=print, cfgs=None):
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

    labels = IndexLabels(args.index_font, getattr(args, "index_font_size", LABEL_FONT_SIZE)) if getattr(args, "index_font", None) and args.grid != "off" else None
    folders = _prompt_folders(args.generated_imgs_dir)
    os.makedirs(args.save_dir, exist_ok=True)
    results = [{}, {}, {}, {}, {}]          # indicators, boxes, gender / race / age logits
    metrics = {}
    semantics, numbers = [{}, {}], {}       # CLIP / DINOv2 similarities and the image numbers they belong to (--original_imgs_dir)
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
                ind, boxes = face_provider(u8.permute(0, 3, 1, 2).float() / 255 * 2 - 1)      # what the reference hands get_face (:637-639)
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
                    sims_p.append(torch.stack(pair_similarity(clip, dino, u8_d, torch.from_numpy(np.stack(batch_o)).to(device))))
                imgs_d.append(u8_d)
                ind_p.append(ind)
                boxes_p.append(boxes)
            imgs_d = torch.cat(imgs_d)
            ind, boxes = torch.cat(ind_p), torch.cat(boxes_p)
            logits = [torch.cat(l) for l in logits_p]
            probs = [torch.softmax(l, dim=-1) for l in logits]
            table = torch.cat(probs, dim=1)
            table = torch.where(ind.to(device)[:, None], table, torch.full_like(table, -1.0)).contiguous()
            metrics[prompt_idx] = gap_metrics("exp-4", ops.eval_tally(table, TABLE_ATTRS).cpu())
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
                numbers[prompt_idx] = [_image_number(p) for p in paths]
            n_images += len(paths)
    with open(os.path.join(args.save_dir, "test_results.pkl"), "wb") as f:
        pickle.dump(results, f)
    keys = list(next(iter(metrics.values())).keys()) if metrics else []
    out = {"per_prompt": {str(i): m for i, m in metrics.items()},
           "mean": {k: float(np.array([m[k] for m in metrics.values()]).mean()) for k in keys}}
    with open(os.path.join(args.save_dir, "metrics.json"), "w") as f:
        json.dump(_json_safe(out), f, indent=1)
    if pairs is not None:
        with open(os.path.join(args.save_dir, "semantics.pkl"), "wb") as f:
            pickle.dump(semantics, f)
        with open(os.path.join(args.save_dir, "semantics.json"), "w") as f:
            json.dump(semantics_summary(semantics, numbers), f, indent=1)
    dt = time.time() - t0
    if log is not None:
        line = {"evaluated_images": n_images, "prompts": len(metrics), "seconds": round(dt, 3), "images_per_s": round(n_images / dt, 2) if dt > 0 else None}
        if pairs is not None:
            line["semantics_pairs"] = n_images
        log(json.dumps(line))
    return results, out


if __name__ == "__main__":
    main(parse_args())
