"""Golden vectors of the index text on the annotated grids, produced by EXECUTING the reference's plot functions with their ``text`` call live.

Run where the reference tree is mounted (``make_golden_eval.REF``) on a Pillow with FreeType and a DejaVuSans-Bold.ttf; the output is committed:
  * reference_indexlabels_grid.npz -- the uint8 arrays handed to ``grid.save`` for N = 5 images of 448 x 384 (a 2 x 3 grid with one white tile) by
      ``grid1``     exp-1's ``plot_in_grid``                          from the fp16 images (one strip:    inner width 434),
      ``grid2``     exp-3's ``plot_in_grid_gender_race``              from the fp16 images (two strips:   inner width 484),
      ``grid3``     exp-4's ``plot_in_grid_gender_race_age``          from the fp16 images (three strips: inner width 534),
      ``u8_grid2``  eval-generated-images.py's ``plot_in_grid_gender_race``     from the uint8 images entering as ``u/255*2-1``,
      ``u8_grid3``  eval-generated-images.py's ``plot_in_grid_gender_race_age`` likewise,
    with their inputs -- ``blocks`` [5,3,28,24] fp16 in [-1,1] and ``u8_blocks`` [5,28,24,3] uint8, each value standing for a 16 x 16 block of the
    image (the test expands them; blocky images keep the compressed file small, and the pixel rule is pinned elsewhere), ``boxes``, ``preds2`` /
    ``preds3`` and ``probs`` as in make_golden_trainplots.py (``grid1`` uses the gender rows) -- and the label atlas ``masks`` / ``desc`` of the
    strings "0" .. "129" as ``evaluation.IndexLabels.host(130)`` builds it from the same font at size 100, with ``pillow`` = the Pillow version
    and ``font`` = the font's family and style names.  A GPU test machine needs neither the font nor FreeType.

What the fixture holds: the labels "0".."4" are 70 pixels wide and start at inner column 400: they clip on the right at inner width 434 and fit
at 484 and 534; 448 < 400 + 20 + 73, so every label clips at the bottom.  Box outlines pass under the labels (row 0's bottom edge at rows
427..430 in all three widths, its right edge at image columns 357..360 under the one- and two-strip label, row 1's right edge at 297..300 under
the three-strip label); row 3 is a -1 (no face) row; rows 0 and 1 tie in confidence inside one group and the generator asserts that this
machine's argsort leaves them in index order (make_golden_trainplots.py explains).  A white bar spans inner columns 50s..50s+50 <= 150 and the
text starts at column 400: in the reference's own geometry a bar can never lie under a label, so the fixture has bars beside the labels only (the
GPU kernel test draws labels over bars and strips with another anchor, against the host statement).  Two- and three-digit labels need more than
ten / a hundred images per grid, which would not fit a committed file: they are compared with ``ImageDraw.text`` directly in
tests/test_indexlabels_cpu.py and, from ``masks``, on the GPU.

Stand-ins in the lifted functions' namespace (none of them is reference text): ``transforms.ToPILImage`` of make_golden_eval.py, ``grid.save``
records the array; ``ImageDraw`` is Pillow's own module, and ``ImageFont.truetype`` ignores the reference's path to Arial Bold (a file in neither
tree) and opens DejaVuSans-Bold at the requested size.  No reference source text and no font file is stored: only inputs and outputs.
"""
import math
import os
import sys
import types

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
from make_golden import lift  # noqa: E402
from make_golden_eval import REF, SCRIPTS, _ToPILImage  # noqa: E402

N, H, W, BLOCK = 5, 448, 384, 16
N_LABELS = 130
FONT_SIZE = 100


def find_font():
    """DejaVuSans-Bold.ttf: the system font directory, else the copy matplotlib ships."""
    cands = ["/usr/share/fonts/truetype/dejavu/DejaVuSans-Bold.ttf", "/usr/share/fonts/dejavu/DejaVuSans-Bold.ttf"]
    try:
        import matplotlib
        cands.append(os.path.join(matplotlib.get_data_path(), "fonts", "ttf", "DejaVuSans-Bold.ttf"))
    except ImportError:
        pass
    for c in cands:
        if os.path.isfile(c):
            return c
    sys.exit("DejaVuSans-Bold.ttf not found: " + ", ".join(cands))


def _namespace(rec, script, fns, font):
    from PIL import Image, ImageDraw, ImageFont, ImageOps

    class Img:
        """PIL.Image module stand-in: ``new`` returns images whose ``save`` records the pixels instead of encoding them."""
        @staticmethod
        def new(*a, **kw):
            im = Image.new(*a, **kw)

            def save(path, **kw2):
                rec["grid"], rec["path"], rec["kw"] = np.array(im), path, kw2
            im.save = save
            return im

    def truetype(font=None, size=10, **kw):
        rec.setdefault("sizes", set()).add(size)
        return ImageFont.truetype(rec["font_path"], size)      # the reference's path (Arial Bold) is ignored

    rec["font_path"] = font
    ns = lift(["image_grid"] + fns, ref=script)
    ns.update(Image=Img, ImageOps=ImageOps, transforms=types.SimpleNamespace(ToPILImage=_ToPILImage), ImageDraw=ImageDraw,
              ImageFont=types.SimpleNamespace(truetype=truetype))
    return ns


def inputs():
    g = torch.Generator().manual_seed(2718)
    blocks = (torch.rand(N, 3, H // BLOCK, W // BLOCK, generator=g) * 2 - 1).half()
    u8_blocks = torch.randint(0, 256, (N, H // BLOCK, W // BLOCK, 3), generator=g, dtype=torch.int64).to(torch.uint8)
    #                      row:   0     1     2     3    4
    preds = torch.tensor([[1, 1, 0, -1, 0],                    # gender
                          [2, 2, 1, -1, 3],                    # race
                          [0, 0, 1, -1, 0]])                   # age
    probs = torch.tensor([[0.75, 0.75, 1.0, -1.0, 0.96875],    # gender: rows 0, 1 tie; p = 1; (1-p)*512 = 16
                          [0.75, 0.75, 1.0, -1.0, 0.25],       # race: rows 0, 1 tie; p = 1; (1-p)*512 = 384: a bar down to the rows beside the label
                          [0.96875, 1.0, 0.75, -1.0, 0.875]])  # age
    boxes = torch.tensor([[100, 50, 360, 430], [-5, 10, 300, 470], [12, 8, 380, 444], [-1, -1, -1, -1], [200, 300, 330, 440]])
    ind = torch.tensor([True, True, True, False, True])
    return blocks, u8_blocks, boxes, preds, probs.float(), ind


def expand(blocks, dims):
    for d in dims:
        blocks = blocks.repeat_interleave(BLOCK, dim=d)
    return blocks.contiguous()


def main():
    import PIL
    from PIL import ImageFont, features
    from finetune_fair_diffusion_amd.evaluation import IndexLabels
    assert features.check("freetype2"), "this generator needs a Pillow with FreeType"
    font = find_font()
    rec = {}
    blocks, u8_blocks, boxes, preds, probs, ind = inputs()
    images = expand(blocks, (2, 3)).float()
    u8 = expand(u8_blocks, (1, 2))
    x_u8 = u8.permute(0, 3, 1, 2).float() / 255 * 2 - 1            # the tensor eval-generated-images.py's main hands to the plot function
    preds3 = preds.clone()
    preds3[1, 4] = 0
    out = dict(blocks=blocks.numpy(), u8_blocks=u8_blocks.numpy(), boxes=boxes.numpy().astype(np.int32), probs=probs.numpy().astype(np.float32),
               preds2=preds[:2].numpy().astype(np.int32), preds3=preds3.numpy().astype(np.int32), block=np.int32(BLOCK))
    train = lambda e: os.path.join(REF, SCRIPTS[e], "1-main-debias.py")
    offline = os.path.join(REF, "eval-generated-images.py")
    jobs = (("grid1", train("exp-1"), "plot_in_grid", 1, images, preds[:1]),
            ("grid2", train("exp-3"), "plot_in_grid_gender_race", 2, images, preds[:2]),
            ("grid3", train("exp-4"), "plot_in_grid_gender_race_age", 3, images, preds3),
            ("u8_grid2", offline, "plot_in_grid_gender_race", 2, x_u8, preds[:2]),
            ("u8_grid3", offline, "plot_in_grid_gender_race_age", 3, x_u8, preds3))
    for name, script, fn, n_attr, x, pr in jobs:
        ns = _namespace(rec, script, [fn], font)
        kw = dict(face_indicators=ind, face_bboxs=boxes, preds_gender=pr[0], pred_class_probs_gender=probs[0])
        if n_attr >= 2:
            kw.update(preds_race=pr[1], pred_class_probs_race=probs[1])
        if n_attr == 3:
            kw.update(preds_age=pr[2], pred_class_probs_age=probs[2])
        ns[fn](x, "./grid.jpg", **kw)
        assert rec["kw"] == dict(quality=25) and rec["sizes"] == {FONT_SIZE}
        rows = int(math.sqrt(N))
        assert rec["grid"].shape == (rows * (H + 20), math.ceil(N / rows) * (W + 50 * n_attr + 20), 3), rec["grid"].shape
        out[name] = rec["grid"]
        # the tie's order as THIS machine's argsort leaves it (make_golden_trainplots.py)
        key = probs[1] if n_attr == 2 else probs[0]
        assert key[torch.tensor([0, 1])].argsort(descending=True).tolist() == [0, 1], "argsort does not keep the index order here"
    masks, desc = IndexLabels(font, FONT_SIZE).host(N_LABELS)
    f = ImageFont.truetype(font, FONT_SIZE)
    out.update(masks=masks, desc=desc, pillow=np.array(PIL.__version__), font=np.array(" ".join(f.getname())), font_size=np.int32(FONT_SIZE))
    path = os.path.join(HERE, "reference_indexlabels_grid.npz")
    np.savez_compressed(path, **out)
    print("wrote", path, os.path.getsize(path), "bytes; Pillow", PIL.__version__, "font", f.getname(), "atlas", masks.size, "bytes")


if __name__ == "__main__":
    if not os.path.isdir(REF):
        sys.exit(f"{REF} is not available: the index-label goldens are generated where the reference tree is mounted")
    main()
