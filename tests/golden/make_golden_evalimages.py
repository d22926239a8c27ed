"""Golden vectors of the offline evaluator (evaluate_images.py), produced by EXECUTING the reference's ``eval-generated-images.py``.

Run where the reference tree is mounted (``make_golden_eval.REF``); the outputs are committed:
  * reference_evalimages_grid.npz -- the uint8 arrays ``plot_in_grid_gender_race`` (``*_grid2``) and ``plot_in_grid_gender_race_age`` (``*_grid3``)
    hand to ``grid.save`` for N = 5 (case a) and N = 9 (case b), with their inputs: 64x64 uint8 HWC images, constant on 4x4 blocks, that enter the
    functions as ``u/255*2-1`` in fp32 (what the reference's main builds from a decoded JPEG), boxes, and the predictions / probabilities of
    gender, race and age as rows of ``*_preds`` / ``*_probs`` [3, N] (the two-attribute grid uses rows 0 and 1).  Covered: all 256 byte values;
    probabilities of exactly 1 (no bar), among them a race probability of 1 beside an age probability below 1 (the three-strip grid tests the race
    probability for the age bar) and the reverse; ``(1-p)*512 = 16``; a box touching the border and one sticking out; a -1 row; at N = 9 every
    (gender, race) group; at N = 5 groups of two whose confidence order is the reverse of their index order; no ties inside a group;
  * reference_evalimages_cli.json -- the reference's ``parse_args([])`` defaults.

Stand-ins in the lifted functions' namespace are those of make_golden_eval.py (none of them is reference text): ``transforms.ToPILImage`` does
``mul(255).byte()`` on the CHW tensor (torchvision is not installed), ``ImageFont.truetype`` returns None and ``Draw.text`` is a no-op (the font
file is in neither tree: the recorded grids carry NO index text), ``grid.save`` records the array instead of encoding it.
No reference source text is stored: only inputs and outputs.
"""
import json
import math
import os
import sys
import types

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
from make_golden import lift  # noqa: E402
from make_golden_eval import REF, _ToPILImage  # noqa: E402

SCRIPT = "eval-generated-images.py"


def _namespace(rec):
    from PIL import Image, ImageDraw, ImageOps

    class Draw:
        """ImageDraw.Draw whose ``text`` does nothing (no font file)."""
        def __init__(self, im):
            self._d = ImageDraw.Draw(im)
            self._image = self._d._image

        def rectangle(self, *a, **kw):
            return self._d.rectangle(*a, **kw)

        def text(self, *a, **kw):
            return None

    class Img:
        """PIL.Image module stand-in: ``new`` returns images whose ``save`` records the pixels instead of encoding them."""
        @staticmethod
        def new(*a, **kw):
            im = Image.new(*a, **kw)

            def save(path, **kw2):
                rec["grid"], rec["path"], rec["kw"] = np.array(im), path, kw2
            im.save = save
            return im

    ns = lift(["image_grid", "plot_in_grid_gender_race", "plot_in_grid_gender_race_age"], ref=os.path.join(REF, SCRIPT))
    ns.update(Image=Img, ImageOps=ImageOps, transforms=types.SimpleNamespace(ToPILImage=_ToPILImage),
              ImageDraw=types.SimpleNamespace(Draw=Draw), ImageFont=types.SimpleNamespace(truetype=lambda **kw: None))
    return ns


def inputs(N):
    """(images uint8 [N,64,64,3], boxes [N,4], preds [3,N], probs [3,N] fp32, indicators [N])."""
    H = W = 64
    g = torch.Generator().manual_seed(177 + N)
    blocks = torch.randint(0, 256, (N, H // 4, W // 4, 3), generator=g, dtype=torch.int64)
    blocks[0, :, :, 0] = torch.arange(256).view(16, 16)                                # every byte value
    images = blocks.to(torch.uint8).repeat_interleave(4, dim=1).repeat_interleave(4, dim=2).contiguous()
    probs = torch.empty(3, N)
    for s, k in enumerate((2, 4, 2)):                                                  # distinct values above 1/k, below 1
        probs[s] = (1.0 / k + (1 - 1.0 / k) * (torch.randperm(N, generator=g).float() + 0.37) / (N + 1))
    if N == 5:
        # rows 0, 1: one (1, 2, 0) group whose confidences rise with the index; rows 2, 4 share (0, 1) and differ in age; row 3: no face
        preds = torch.tensor([[1, 1, 0, -1, 0], [2, 2, 1, -1, 1], [0, 0, 1, -1, 0]])
        probs[:, 0] = torch.tensor([0.7, 0.6, 0.8])
        probs[:, 1] = torch.tensor([0.8, 0.9, 1.0])                                    # age probability 1: a bar of one row in the three-strip grid
        probs[:, 2] = torch.tensor([0.96875, 0.5, 0.96875])                            # (1 - p) * 512 = 16
        probs[:, 4] = torch.tensor([1.0, 0.75, 0.9])                                   # gender probability 1: no gender bar
        noface = [3]
    else:
        # rows 0..7: every (gender, race) group once, ages alternating; row 8: no face
        preds = torch.tensor([[i // 4 for i in range(8)] + [-1], [i % 4 for i in range(8)] + [-1], [i % 2 for i in range(8)] + [-1]])
        probs[1, 2] = 1.0                                                              # race probability 1 beside an age probability below 1
        probs[0, 5] = 0.96875
        probs[2, 6] = 1.0
        noface = [8]
    boxes = torch.zeros(N, 4, dtype=torch.long)
    for i in range(N):
        x0, y0 = [int(v) for v in torch.randint(0, 30, (2,), generator=g)]
        boxes[i] = torch.tensor([x0, y0, x0 + int(torch.randint(12, 34, (1,), generator=g)), y0 + int(torch.randint(12, 34, (1,), generator=g))])
    boxes[0] = torch.tensor([0, 0, 63, 63])                                            # touches the border
    boxes[1] = torch.tensor([-5, 10, 40, 70])                                          # sticks out on two sides
    ind = torch.ones(N, dtype=torch.bool)
    for i in noface:
        ind[i], boxes[i] = False, -1
        preds[:, i], probs[:, i] = -1, -1.0
    return images, boxes, preds, probs.float(), ind


def grid_golden():
    rec = {}
    ns = _namespace(rec)
    out = {}
    for case, N in (("a", 5), ("b", 9)):
        images, boxes, preds, probs, ind = inputs(N)
        x = images.permute(0, 3, 1, 2).float() / 255 * 2 - 1                           # the tensor the reference's main hands to the plot function
        for n_attr, fn in ((2, "plot_in_grid_gender_race"), (3, "plot_in_grid_gender_race_age")):
            kw = dict(face_indicators=ind, face_bboxs=boxes, preds_gender=preds[0], pred_class_probs_gender=probs[0], preds_race=preds[1],
                      pred_class_probs_race=probs[1])
            if n_attr == 3:
                kw.update(preds_age=preds[2], pred_class_probs_age=probs[2])
            ns[fn](x, "./grid.jpg", **kw)
            assert rec["kw"] == dict(quality=25)
            rows = int(math.sqrt(N))
            assert rec["grid"].shape == (rows * 84, math.ceil(N / rows) * (64 + 50 * n_attr + 20), 3), rec["grid"].shape
            out[f"{case}_grid{n_attr}"] = rec["grid"]
        out[f"{case}_images"] = images.numpy()
        out[f"{case}_boxes"] = boxes.numpy().astype(np.int32)
        out[f"{case}_preds"] = preds.numpy().astype(np.int32)
        out[f"{case}_probs"] = probs.numpy().astype(np.float32)
    assert len(np.unique(out["a_images"])) == 256
    path = os.path.join(HERE, "reference_evalimages_grid.npz")
    np.savez_compressed(path, **out)
    print("wrote", path, os.path.getsize(path), "bytes")


def cli_golden():
    ns = lift(["parse_args"], ref=os.path.join(REF, SCRIPT))
    path = os.path.join(HERE, "reference_evalimages_cli.json")
    json.dump(dict(defaults=vars(ns["parse_args"]([]))), open(path, "w"), indent=1, sort_keys=True)
    print("wrote", path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    if not os.path.isdir(REF):
        sys.exit(f"{REF} is not available: the evaluator's goldens are generated where the reference tree is mounted")
    grid_golden()
    cli_golden()
