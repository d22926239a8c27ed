"""Golden vectors of the training monitor's plots, produced by EXECUTING the reference's training-side plot functions.

Run where the reference tree is mounted (``make_golden_eval.REF``); the output is committed:
  * reference_trainplot_grid.npz -- the uint8 arrays exp-3's ``plot_in_grid_gender_race`` (``grid2``) and exp-4's
    ``plot_in_grid_gender_race_age`` (``grid3``) hand to ``grid.save`` for N = 5 images of 64x64 (a 2 x 3 grid with one white tile), with their
    inputs: ``images`` [5,3,64,64] fp16 in [-1,1] (what a training step holds, constant on 4x4 blocks), ``boxes`` [5,4], the confidences of gender,
    race and age as rows of ``probs`` [3,5] (the two-attribute grid uses rows 0 and 1) and the predictions ``preds2`` [2,5] / ``preds3`` [3,5].
    Four rows with a face cannot show four race classes AND two rows of one group: the two tables differ in row 4's race (3 / 0), so that
    together they cover every gender, race and age class; both have a -1 row.  Further covered: p = 1 (no bar), among them a race probability of
    1 beside an age probability below 1 (exp-4 tests the race probability for the age bar: no age bar) and an age probability of 1 beside a race
    probability below 1 (a bar of one row); ``(1-p)*512 = 16`` (a bar that ends inside the tile) and 64, 128, 192 (clipped to the tile); a box on
    the border and one over it; two equal confidences inside one group (rows 0 and 1: same gender, race and age, equal gender AND race
    confidence).  The reference orders a group with ``argsort(descending=True)``, which leaves ties open: with the tie at rows 0, 1 torch's CPU
    argsort on the machine that generated this file returns the index order, which the generator asserts -- a machine on which it does not must
    drop the tie from the golden (``TIE = False``) and keep it in the host-statement test only.
    Image 0 holds the pixel probes: the fp16 values whose exact ``(x*0.5+0.5)*255`` lies within one fp32 ulp of an integer without being one.
    There are two, +-0.0039215087890625 (128 - 2^-17 and 127 + 2^-17: both paint 127; a chain that rounds once more upwards, or rounds to
    nearest instead of truncating, paints 128 for the first), beside the two ends -1 and 1, and 0.

Stand-ins in the lifted functions' namespace are those of make_golden_eval.py / make_golden_evalimages.py (none of them is reference text):
``transforms.ToPILImage`` does ``mul(255).byte()`` on the CHW tensor, ``ImageFont.truetype`` returns None and ``Draw.text`` is a no-op (the
recorded grids carry NO index text), ``grid.save`` records the array instead of encoding it.
No reference source text is stored: only inputs and outputs.
"""
import math
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
from make_golden import lift  # noqa: E402
from make_golden_eval import REF, SCRIPTS, _ToPILImage  # noqa: E402

N, H, W = 5, 64, 64
TIE = True


def _namespace(rec, exp, fn):
    """``fn`` and ``image_grid`` lifted from the training script of ``exp``, with make_golden_evalimages.py's stand-ins around them."""
    import types
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

    ns = lift(["image_grid", fn], ref=os.path.join(REF, SCRIPTS[exp], "1-main-debias.py"))
    ns.update(Image=Img, ImageOps=ImageOps, transforms=types.SimpleNamespace(ToPILImage=_ToPILImage),
              ImageDraw=types.SimpleNamespace(Draw=Draw), ImageFont=types.SimpleNamespace(truetype=lambda **kw: None))
    return ns


def pixel_probes():
    """fp16 values in [-1,1] whose exact (x*0.5+0.5)*255 is within one fp32 ulp of an integer and not an integer, sorted."""
    bits = np.arange(1 << 16, dtype=np.uint16).view(np.float16)
    x = bits[np.isfinite(bits) & (np.abs(bits) <= 1)].astype(np.float64)
    v = (x * 0.5 + 0.5) * 255                                  # exact in fp64: at most 11 + 14 + 8 bits
    d = np.abs(v - np.rint(v))
    ulp = np.spacing(np.maximum(v, 1e-30).astype(np.float32)).astype(np.float64)
    return np.unique(x[(d > 0) & (d <= ulp)]).astype(np.float32)


def inputs():
    g = torch.Generator().manual_seed(313)
    images = (torch.rand(N, 3, H // 4, W // 4, generator=g) * 2 - 1).half().float()
    probes = torch.from_numpy(pixel_probes())
    assert len(probes) <= (H // 4) * (W // 4) - 3
    plane = torch.cat([probes, torch.tensor([-1.0, 1.0, 0.0])])
    for c in range(3):
        images[0, c].view(-1)[:len(plane)] = plane.roll(c)
    images = images.repeat_interleave(4, dim=2).repeat_interleave(4, dim=3).contiguous()
    assert torch.equal(images, images.half().float()) and float(images.abs().max()) <= 1
    #                      row:   0     1     2     3    4
    preds = torch.tensor([[1, 1, 0, -1, 0],                    # gender
                          [2, 2, 1, -1, 3],                    # race (0 is covered by the three-strip inputs below: see ``preds3``)
                          [0, 0, 1, -1, 0]])                   # age
    probs = torch.tensor([[0.75, 0.75, 1.0, -1.0, 0.96875],    # gender: rows 0, 1 tie; p = 1; (1-p)*512 = 16
                          [0.75, 0.75, 1.0, -1.0, 0.625],      # race: rows 0, 1 tie; p = 1 (beside an age probability below 1); (1-p)*512 = 192 > 64
                          [0.96875, 1.0, 0.75, -1.0, 0.875]])  # age: 16; p = 1 under a race probability below 1 (a bar of one row); 128; 64
    if not TIE:
        probs[0, 1], probs[1, 1] = 0.625, 0.625
    boxes = torch.tensor([[0, 0, 63, 63], [-5, 10, 40, 70], [12, 8, 40, 44], [-1, -1, -1, -1], [20, 30, 26, 50]])
    ind = torch.tensor([True, True, True, False, True])
    return images, boxes, preds, probs.float(), ind


def main():
    rec = {}
    images, boxes, preds, probs, ind = inputs()
    out = dict(images=images.numpy().astype(np.float16), boxes=boxes.numpy().astype(np.int32), probs=probs.numpy().astype(np.float32))
    # every race class needs two more rows than N = 5 leaves in one table: the two-strip grid is recorded with race (2, 2, 1, -1, 3) and the
    # three-strip grid with race (2, 2, 1, -1, 0); the other rows are shared.  Stored as ``preds2`` [2,5] and ``preds3`` [3,5].
    preds3 = preds.clone()
    preds3[1, 4] = 0
    for n_attr, exp, fn, pr in ((2, "exp-3", "plot_in_grid_gender_race", preds[:2]), (3, "exp-4", "plot_in_grid_gender_race_age", preds3)):
        ns = _namespace(rec, exp, fn)          # the training script's own copy of the function
        kw = dict(face_indicators=ind, face_bboxs=boxes, preds_gender=pr[0], pred_class_probs_gender=probs[0], preds_race=pr[1],
                  pred_class_probs_race=probs[1])
        if n_attr == 3:
            kw.update(preds_age=pr[2], pred_class_probs_age=probs[2])
        ns[fn](images, "./grid.jpg", **kw)
        assert rec["kw"] == dict(quality=25)
        rows = int(math.sqrt(N))
        assert rec["grid"].shape == (rows * (H + 20), math.ceil(N / rows) * (W + 50 * n_attr + 20), 3), rec["grid"].shape
        out[f"grid{n_attr}"] = rec["grid"]
        out[f"preds{n_attr}"] = pr.numpy().astype(np.int32)
        if TIE:
            # the tie's order as THIS machine's argsort leaves it: rows 0 and 1 form the first group, and the recorded grid shows them in index order
            key = probs[1] if n_attr == 2 else probs[0]
            assert key[torch.tensor([0, 1])].argsort(descending=True).tolist() == [0, 1], "argsort does not keep the index order here: set TIE = False"
    assert set(out["preds2"][1].tolist()) | set(out["preds3"][1].tolist()) == {-1, 0, 1, 2, 3}
    path = os.path.join(HERE, "reference_trainplot_grid.npz")
    np.savez_compressed(path, **out)
    print("wrote", path, os.path.getsize(path), "bytes;", len(pixel_probes()), "pixel probes exist,", "tie kept" if TIE else "tie dropped")


if __name__ == "__main__":
    if not os.path.isdir(REF):
        sys.exit(f"{REF} is not available: the train-plot goldens are generated where the reference tree is mounted")
    main()
