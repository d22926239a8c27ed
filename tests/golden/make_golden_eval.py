"""Golden vectors of the in-training validation, produced by EXECUTING the reference's own code.

Run in the build container only (needs /root/reference); the outputs are committed:
  * reference_eval_metrics.json -- for seeded probability tables (N in 1, 7, 24, 64: random rows with -1 "no face" rows, ties, one class
    only, no valid row, and probes at the fp32 neighbours of 0.2 / 0.5 / 0.8) the outputs of the four ``get_evaluate_metrics`` variants
    (exp-3, exp-4, exp-5, exp-6) and of exp-1's three inline statements in ``evaluate_process`` (the assignments of ``probs_tmp``,
    ``gender_gap`` and ``gender_pred_between_02_08``), which this maker lifts by target name and wraps as a function;
  * reference_eval_grid.npz -- the uint8 array ``plot_in_grid`` hands to ``grid.save`` for two small cases, with their inputs.

Stand-ins in the lifted functions' namespace (none of them is reference text):
  * torchvision is not installed here: ``transforms.ToPILImage`` is a class whose call does ``mul(255).byte()`` on the CHW tensor and
    builds the PIL image from the HWC array (torchvision's own rule for float tensors);
  * the reference prints the image index with ``../data/0-utils/arial-bold.ttf``, a font file neither tree has: ``ImageFont.truetype``
    returns None and the ``text`` call of the draw object is a no-op, so the recorded grids carry NO index text;
  * ``grid.save`` is intercepted (the array is recorded, no JPEG is written); ``os`` is the real module (the directory check passes on ".").
No reference source text is stored: only inputs and outputs.
"""
import ast
import json
import math
import os
import sys
import textwrap
import types

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
from make_golden import lift  # noqa: E402

REF = "/root/reference"
SCRIPTS = {"exp-1": "exp-1-debias-gender", "exp-3": "exp-3-debias-gender-race", "exp-4": "exp-4-debias-gender-race-age",
           "exp-5": "exp-5-debias-gender-race-multi-concepts", "exp-6": "exp-6-debias-race"}
KEYS = {
    "exp-1": ["gender_gap", "gender_gap_abs", "gender_pred_between_0.2_0.8"],
    "exp-3": ["gender_gap", "gender_pred_below_0.8", "race_gap", "race_pred_below_0.8", "gender_race_gap"],
    "exp-4": ["gender_gap", "gender_pred_below_0.8", "race_gap", "race_pred_below_0.8", "gender_race_gap", "age_young_freq", "age_old_freq",
              "age_pred_below_0.8", "age_gap"],
    "exp-6": ["race0_freq", "race1_freq", "race2_freq", "race3_freq", "race_gap", "race_pred_below_0.8"],
}
KEYS["exp-5"] = KEYS["exp-3"]
SIZES = {"exp-1": [2], "exp-3": [2, 4], "exp-4": [2, 4, 2], "exp-5": [2, 4], "exp-6": [4]}


def lift_exp1_inline():
    """exp-1 computes its three numbers inline in ``evaluate_process``: the statements are found by the names they assign."""
    path = f"{REF}/{SCRIPTS['exp-1']}/1-main-debias.py"
    src = open(path).read()
    fn = [n for n in ast.walk(ast.parse(src)) if isinstance(n, ast.FunctionDef) and n.name == "evaluate_process"][0]
    want = ["probs_tmp", "gender_gap", "gender_pred_between_02_08"]
    segs = {}
    for n in ast.walk(fn):
        if isinstance(n, ast.Assign) and len(n.targets) == 1 and isinstance(n.targets[0], ast.Name) and n.targets[0].id in want:
            segs.setdefault(n.targets[0].id, ast.get_source_segment(src, n))        # the first assignment of each (the generated-image branch)
    body = "\n".join(textwrap.dedent(segs[w]) for w in want)
    code = "def inline(probs_gender_all):\n" + textwrap.indent(body, "    ") + "\n    return gender_gap, abs(gender_gap), abs(gender_pred_between_02_08)\n"
    ns = dict(torch=torch)
    exec(code, ns)
    return ns["inline"]


def f32_next(v, up):
    return float(np.nextafter(np.float32(v), np.float32(2.0 if up else -2.0)))


def tables(sizes, N, seed):
    """{name: [N, sum k] fp32 table}.  Every attribute of a row is valid or -1 together (one head produces all attributes)."""
    g = torch.Generator().manual_seed(seed)
    K = sum(sizes)
    out = {}

    def soft(n, sharp):
        return torch.cat([torch.softmax(torch.randn(n, k, generator=g) * sharp, dim=-1) for k in sizes], dim=1)
    t = soft(N, 2.0)
    t[torch.randperm(N, generator=g)[: N // 5]] = -1
    out["random"] = t
    t = soft(N, 0.3)                                            # flat rows: many maxima below 0.8
    t[torch.randperm(N, generator=g)[: (N + 2) // 3]] = -1
    out["uncertain"] = t
    t = soft(N, 2.0)                                            # ties: the first maximum must win
    c = 0
    for k in sizes:
        t[0::2, c:c + k] = 1.0 / k
        if k == 4:
            t[1::4, c:c + k] = torch.tensor([0.1, 0.4, 0.4, 0.1])
        c += k
    if N > 2:
        t[N // 2] = -1
    out["ties"] = t
    t = torch.zeros(N, K)                                       # one class only (the last of each attribute), confident
    c = 0
    for k in sizes:
        t[:, c:c + k] = 0.01
        t[:, c + k - 1] = 1.0 - 0.01 * (k - 1)
        c += k
    out["one_class"] = t
    out["no_valid"] = torch.full((N, K), -1.0)
    # probes: the compared entry at the fp32 value of the literal and at its two fp32 neighbours, and the interval ends 0 and 1
    vals = [v for lit in (0.2, 0.5, 0.8) for v in (f32_next(lit, False), float(np.float32(lit)), f32_next(lit, True))] + [0.0, 1.0]
    t = torch.zeros(N, K)
    for i in range(N):
        v = vals[(i + seed) % len(vals)]
        c = 0
        for k in sizes:
            t[i, c:c + k] = (1.0 - v) / max(k - 1, 1) if v >= 0.5 else 0.0
            t[i, c + (1 if k == 2 else i % k)] = v              # two classes: p1 = v; four: the maximum (v >= 0.5) or one entry is v
            if v < 0.5:
                t[i, c + (0 if k == 2 else (i + 1) % k)] = float(np.float32(1.0) - np.float32(v))
            c += k
    out["probes"] = t
    return {k: v.float().contiguous() for k, v in out.items()}


def metrics_golden():
    fns = {"exp-1": lift_exp1_inline()}
    for e in ("exp-3", "exp-4", "exp-5", "exp-6"):
        fns[e] = lift(["get_evaluate_metrics"], ref=f"{REF}/{SCRIPTS[e]}/1-main-debias.py")["get_evaluate_metrics"]
    cases = []
    for ei, e in enumerate(sorted(fns)):
        sizes = SIZES[e]
        for N in (1, 7, 24, 64):
            for name, t in tables(sizes, N, 9000 + 10 * ei + N).items():
                parts, c = [], 0
                for k in sizes:
                    parts.append(t[:, c:c + k].clone())
                    c += k
                vals = fns[e](*parts)
                vals = [float(v) for v in vals]
                assert len(vals) == len(KEYS[e])
                cases.append(dict(experiment=e, table=name, N=N, sizes=sizes, probs=t.tolist(), metrics=dict(zip(KEYS[e], vals))))
    path = os.path.join(HERE, "reference_eval_metrics.json")
    json.dump(dict(cases=cases), open(path, "w"))
    print("wrote", path, os.path.getsize(path), "bytes;", len(cases), "cases")


class _ToPILImage:
    def __call__(self, img):
        from PIL import Image
        return Image.fromarray(img.mul(255).byte().permute(1, 2, 0).contiguous().numpy())


def grid_golden():
    from PIL import Image, ImageDraw, ImageFont, ImageOps
    rec = {}

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
            real_save = im.save

            def save(path, **kw2):
                rec["grid"], rec["path"], rec["kw"] = np.array(im), path, kw2
            im.save = save
            del real_save
            return im

    ns = lift(["image_grid", "plot_in_grid"], ref=f"{REF}/{SCRIPTS['exp-1']}/1-main-debias.py")
    ns.update(Image=Img, ImageOps=ImageOps, transforms=types.SimpleNamespace(ToPILImage=_ToPILImage),
              ImageDraw=types.SimpleNamespace(Draw=Draw), ImageFont=types.SimpleNamespace(truetype=lambda **kw: None))
    out = {}
    H = W = 64
    for case, N in (("a", 5), ("b", 9)):
        g = torch.Generator().manual_seed(77 + N)
        # random fp16-representable values, constant on 4x4 blocks (keeps the compressed file small; the pixel rule is per value)
        images = (torch.rand(N, 3, H // 4, W // 4, generator=g) * 2 - 1).half().float().repeat_interleave(4, dim=2).repeat_interleave(4, dim=3).contiguous()
        images[0, :, :4, :4] = 1.0
        images[0, :, 4:8, :4] = -1.0
        preds = torch.randint(0, 2, (N,), generator=g)
        p = torch.rand(N, generator=g) * 0.5 + 0.5
        p[1] = 1.0                                                                   # no white bar
        p[2] = 0.96875                                                               # (1 - p) * 512 = 16: bar ends inside the 64-pixel tile
        boxes = torch.zeros(N, 4, dtype=torch.long)
        for i in range(N):
            x0, y0 = [int(v) for v in torch.randint(0, 30, (2,), generator=g)]
            boxes[i] = torch.tensor([x0, y0, x0 + int(torch.randint(12, 34, (1,), generator=g)), y0 + int(torch.randint(12, 34, (1,), generator=g))])
        boxes[0] = torch.tensor([0, 0, 63, 63])                                      # touches the border
        boxes[1] = torch.tensor([-5, 10, 40, 70])                                    # sticks out on two sides
        ind = torch.ones(N, dtype=torch.bool)
        for i in ([3] if N == 5 else [4, 7]):                                        # no face: pred -1, prob -1, box -1
            ind[i], preds[i], p[i], boxes[i] = False, -1, -1.0, -1
        ns["plot_in_grid"](images, "./grid.jpg", face_indicators=ind, face_bboxs=boxes, preds_gender=preds, pred_class_probs_gender=p)
        assert rec["kw"] == dict(quality=25)
        out[f"{case}_images"] = images.numpy().astype(np.float16)
        out[f"{case}_boxes"] = boxes.numpy().astype(np.int32)
        out[f"{case}_preds"] = preds.numpy().astype(np.int32)
        out[f"{case}_maxprob"] = p.numpy().astype(np.float32)
        out[f"{case}_grid"] = rec["grid"]
        rows = int(math.sqrt(N))
        assert rec["grid"].shape == (rows * (H + 20), math.ceil(N / rows) * (W + 70), 3), rec["grid"].shape
    path = os.path.join(HERE, "reference_eval_grid.npz")
    np.savez_compressed(path, **out)
    print("wrote", path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    if not os.path.isdir(REF):
        sys.exit(f"{REF} is not available: the evaluation goldens are generated where the reference tree is mounted")
    metrics_golden()
    grid_golden()
