"""In-training validation: ``evaluate_process`` / ``evaluation_step`` of exp-1-debias-gender/1-main-debias.py (:1449-1571, :1659-1690) and
the ``get_evaluate_metrics`` variants of the other experiments (exp-3/5 :1716-1749, exp-4 :1780-1821, exp-6 :1624-1637) on FairnessTrainer.

Per validation prompt the frozen pair and then the evaluated pair generate ``val_images_per_prompt_GPU`` images with 25 denoising steps;
the classifier's probability table stays on the device, where ONE launch (``ops.eval_tally``, csrc/evaluate.hip) reduces it to integer
counts and, with ``--validation grids``, one launch (``ops.eval_grid``) paints the whole annotated grid of ``plot_in_grid`` (:151-217) as
uint8 -- the host reads back 32 integers and the finished grid instead of N x 3 x 512 x 512 images and probability tables.
``gap_metrics`` turns the counts into the reference's floats with the reference's fp32 operations; ``tally_host`` / ``grid_host`` are the
plain host statements both kernels are tested against.  ``--validation grids_attrs`` and the training monitor (step.py) paint exp-3/4/5 with one
strip per attribute instead (``device_grid_attrs``: one launch of ``ops.eval_grid_attrs_img``; host statement ``grid_attrs_img_host``).
``IndexLabels`` (``--index_font``) adds the reference's index text to any of these grids: the strings are rasterised once on the host with the
caller's font and one more launch (``ops.eval_grid_labels``; host statement ``labels_host``) blends them into the painted grid.

The EMA pass rewrites the 16-bit LoRA operand copies from ``bank.ema`` (``refresh_lora(ema=True)``) and back from ``bank.flat`` afterwards:
no fp32 parameter, EMA or optimiser buffer is copied or written.
"""
import json
import math
import os

import numpy as np
import torch

N_DENOISING_STEPS_VAL = 25           # :1453
MAX_ATTR, MAX_K = 3, 4
# layout of the int32 counts ``fd_eval_tally`` writes (include/fairdiff_hip.h): per attribute a, at 6*a: n_valid, hist[0..3], n(max < 0.8)
ATTR_STRIDE, OFF_HIST, OFF_BELOW = 6, 1, 5
OFF_P1_HI, OFF_P1_LO, OFF_P1_MID, OFF_JOINT, OFF_JOINT_VALID, N_COUNTS = 18, 19, 20, 21, 29, 32
STRIP, FRAME, BOX_WIDTH = 50, 10, 4

# class colour of the first attribute, index = pred + 1 (pred -1 = no face): the reference's PIL colour names as RGB
PALETTE_GENDER = [(255, 255, 255), (255, 0, 0), (0, 0, 255)]                                   # white / red / blue (exp-1 :179-187)
PALETTE_RACE = [(255, 255, 255), (50, 205, 50), (0, 0, 0), (165, 42, 42), (255, 165, 0)]       # white / limegreen / black / brown / orange (exp-6 :188-197)


def table_attrs(trainer_attrs):
    """[(column offset, k)] of the attributes inside the concatenated [N, sum k] probability table."""
    out, c = [], 0
    for _, _, k in trainer_attrs:
        out.append((c, k))
        c += k
    return out


def tally_host(probs, attrs):
    """The plain torch statement of ``fd_eval_tally``: probs [N, >= sum k] fp32 on the CPU (-1 rows = no face), attrs [(c0, k)] -> int32 [32]."""
    probs = probs.detach().to("cpu", torch.float32)
    assert 1 <= len(attrs) <= MAX_ATTR and all(1 <= k <= MAX_K for _, k in attrs)
    counts = torch.zeros(N_COUNTS, dtype=torch.int32)
    valid, preds = [], []
    for a, (c0, k) in enumerate(attrs):
        p = probs[:, c0:c0 + k]
        v = (p != -1).all(dim=-1)
        valid.append(v)
        pv = p[v]
        pred = pv.argmax(dim=-1) if len(pv) else torch.zeros(0, dtype=torch.long)      # first maximum wins
        preds.append(pred)
        counts[ATTR_STRIDE * a] = int(v.sum())
        for c in range(k):
            counts[ATTR_STRIDE * a + OFF_HIST + c] = int((pred == c).sum())
        counts[ATTR_STRIDE * a + OFF_BELOW] = int((pv.max(dim=-1).values < 0.8).sum()) if len(pv) else 0
    # one classifier head produces every attribute of an image: the reference's per-attribute masks coincide
    assert all(torch.equal(valid[0], v) for v in valid[1:]), "attributes of one row must be valid together"
    if attrs[0][1] == 2:
        p1 = probs[:, attrs[0][0] + 1][valid[0]]
        counts[OFF_P1_HI] = int(((p1 >= 0.5) * (p1 <= 1)).sum())
        counts[OFF_P1_LO] = int(((p1 >= 0) * (p1 <= 0.5)).sum())
        counts[OFF_P1_MID] = int(((p1 >= 0.2) * (p1 <= 0.8)).sum())
        if len(attrs) >= 2:
            for g in range(2):
                for r in range(attrs[1][1]):
                    counts[OFF_JOINT + 4 * g + r] = int(((preds[0] == g) * (preds[1] == r)).sum())
            counts[OFF_JOINT_VALID] = int((valid[0] & valid[1]).sum())
    return counts


def _first_argmax(p):
    """Index of the first maximum per row: a tie rule the device's ``argmax`` does not promise."""
    mx = p.max(dim=-1).values
    cols = torch.arange(p.shape[1], device=p.device).expand_as(p)
    return torch.where(p == mx[:, None], cols, torch.full_like(cols, p.shape[1])).min(dim=-1).values


def joint_tally_host(probs, attrs):
    """The plain host statement of the joint histogram of a custom run: probs [N, >= sum k] fp32 on the CPU (-1 rows = no face), attrs
    [(c0, k)] -> int32 [prod k]: how many rows with a face fall into each cell, the first maximum winning per attribute, cells ordered as
    ``fairness._cells`` (mixed radix over the attributes in order)."""
    from .fairness import _cells
    probs = probs.detach().to("cpu", torch.float32)
    cells = _cells([k for _, k in attrs])
    hist = torch.zeros(len(cells), dtype=torch.int32)
    for row in probs:
        if any(bool((row[c0:c0 + k] == -1).any()) for c0, k in attrs):
            continue
        hist[cells.index(tuple(int(row[c0:c0 + k].argmax()) for c0, k in attrs))] += 1
    return hist


def joint_tally(pd, attrs):
    """``joint_tally_host`` with torch on the table's device (at most ``world x B`` rows and 64 cells): first argmax per attribute, mixed-radix
    cell index, one ``torch.bincount``; rows without a face are counted in a spare bin that is cut off.  int32 [prod k]."""
    n_cells = math.prod(k for _, k in attrs)
    valid = torch.ones(pd.shape[0], dtype=torch.bool, device=pd.device)
    cell = torch.zeros(pd.shape[0], dtype=torch.long, device=pd.device)
    for c0, k in attrs:
        p = pd[:, c0:c0 + k]
        valid &= (p != -1).all(dim=-1)
        cell = cell * k + _first_argmax(p)
    cell = torch.where(valid, cell, torch.full_like(cell, n_cells))
    return torch.bincount(cell, minlength=n_cells + 1)[:n_cells].to(torch.int32)


def tally_with_joint(tr, pd):
    """The counts of one probability table on the device, as ONE int32 tensor to read back: the 32 integers of ``ops.eval_tally`` and, for a
    custom run with two or more attributes, the cells of ``joint_tally`` behind them (``split_counts`` takes them apart)."""
    from . import ops
    attrs = table_attrs(tr.attrs)
    counts = ops.eval_tally(pd, attrs)
    spec = getattr(tr, "spec", None)
    if spec is not None and spec.custom and len(attrs) >= 2:
        counts = torch.cat([counts, joint_tally(pd, attrs)])
    return counts


def split_counts(counts):
    """(the 32 counts, the joint histogram or None) of ``tally_with_joint``'s tensor."""
    return counts[:N_COUNTS], (counts[N_COUNTS:] if counts.shape[0] > N_COUNTS else None)


def gap_to_target(freqs, p):
    """Half the L1 distance between class frequencies (Python floats holding fp32 values, ``_freq(..).item()``) and the target probabilities:
    ``(|f0 - p0| + |f1 - p1| + ...) / 2``, as exp-4 writes its ``age_gap`` (exp-4 :1815-1818)."""
    return sum(abs(f - t) for f, t in zip(freqs, p)) / 2


def target_metrics(spec, counts, joint=None):
    """The validation numbers of a custom run from the integer counts: per attribute ``<name>{k}_freq``, ``<name>_pred_below_0.8`` and
    ``<name>_gap_to_target``; with two or more attributes ``joint_gap_to_target`` over the cells of ``joint`` (``joint_tally``), whose target is the
    product of the attributes' marginal targets."""
    c = [int(v) for v in (counts.tolist() if hasattr(counts, "tolist") else counts)]
    out = {}
    for a, at in enumerate(spec.attributes):
        n, below = c[ATTR_STRIDE * a], c[ATTR_STRIDE * a + OFF_BELOW]
        f = [_freq(c[ATTR_STRIDE * a + OFF_HIST + k], n).item() for k in range(at.k)]
        out.update({f"{at.name}{k}_freq": f[k] for k in range(at.k)})
        out[f"{at.name}_pred_below_0.8"] = _freq(below, n).item()
        out[f"{at.name}_gap_to_target"] = gap_to_target(f, at.p)
    if len(spec.attributes) >= 2:
        from .fairness import _cells
        if joint is None:
            raise ValueError("the joint gap of a custom run needs the joint histogram (joint_tally)")
        j = [int(v) for v in (joint.tolist() if hasattr(joint, "tolist") else joint)]
        n = sum(j)
        target = [math.prod(at.p[ci] for at, ci in zip(spec.attributes, cell)) for cell in _cells(spec.sizes)]
        out["joint_gap_to_target"] = gap_to_target([_freq(v, n).item() for v in j], target)
    return out


def _freq(c, n):
    """``(mask).float().mean()``: the fp32 sum of c ones divided by n in fp32 (NaN for the empty selection, as torch's mean)."""
    return torch.tensor(float(c), dtype=torch.float32) / torch.tensor(float(n), dtype=torch.float32)


def _pairwise_gap(freqs):
    """Mean |f_i - f_j| over the ordered pairs i != j, in fp32 and in row-major order: what the reference's
    ``cdist(f, f, p=1)`` with the diagonal dropped, ``.mean()`` computes."""
    f = torch.stack(freqs)
    n = f.shape[0]
    d = (f[:, None] - f[None, :]).abs()
    return d[~torch.eye(n, dtype=torch.bool)].reshape(n, n - 1).mean().item()


def gap_metrics(experiment, counts, spec=None, joint=None):
    """The reference's validation numbers of ``experiment`` from the integer counts of ``tally_host`` / ``ops.eval_tally``; for ``custom`` the
    distances to the target of ``spec`` (``target_metrics``; ``joint``: the cells of ``joint_tally``)."""
    if experiment == "custom":
        if spec is None:
            raise ValueError("the metrics of a custom run need its ExperimentSpec")
        return target_metrics(spec, counts, joint)
    c = [int(v) for v in (counts.tolist() if hasattr(counts, "tolist") else counts)]
    A = lambda a: (c[ATTR_STRIDE * a], c[ATTR_STRIDE * a + OFF_HIST:ATTR_STRIDE * a + OFF_HIST + 4], c[ATTR_STRIDE * a + OFF_BELOW])
    if experiment in ("exp-1", "exp-2"):
        n = c[0]
        gap = (_freq(c[OFF_P1_HI], n) - _freq(c[OFF_P1_LO], n)).item()
        return {"gender_gap": gap, "gender_gap_abs": abs(gap), "gender_pred_between_0.2_0.8": abs(_freq(c[OFF_P1_MID], n).item())}
    if experiment == "exp-6":
        n, h, below = A(0)
        f = [_freq(h[k], n) for k in range(4)]
        out = {f"race{k}_freq": f[k].item() for k in range(4)}
        out.update({"race_gap": _pairwise_gap(f), "race_pred_below_0.8": _freq(below, n).item()})
        return out
    if experiment in ("exp-3", "exp-4", "exp-5"):
        ng, hg, bg = A(0)
        nr, hr, br = A(1)
        out = {"gender_gap": abs(_freq(hg[1], ng) - _freq(hg[0], ng)).item(), "gender_pred_below_0.8": _freq(bg, ng).item(),
               "race_gap": _pairwise_gap([_freq(hr[k], nr) for k in range(4)]), "race_pred_below_0.8": _freq(br, nr).item(),
               "gender_race_gap": _pairwise_gap([_freq(c[OFF_JOINT + k], c[OFF_JOINT_VALID]) for k in range(8)])}
        if experiment == "exp-4":
            na, ha, ba = A(2)
            a0, a1 = _freq(ha[0], na).item(), _freq(ha[1], na).item()
            out.update({"age_young_freq": a0, "age_old_freq": a1, "age_pred_below_0.8": _freq(ba, na).item(),
                        "age_gap": (abs(a0 - 0.75) + abs(a1 - 0.25)) / 2})
        return out
    raise ValueError(f"no validation metrics for {experiment}")


def grid_shape(N, H, W):
    rows = int(math.sqrt(N))
    cols = math.ceil(N / rows)
    return rows, cols, (rows * (H + 2 * FRAME), cols * (W + STRIP + 2 * FRAME), 3)


def grid_order(preds, maxprob, n_classes=2):
    """Tile order of ``plot_in_grid``: exp-1 shows class 1 then class 0 (:163-173), exp-6 classes 0..3 (:160-178), each from the most to the
    least confident, then the images without a face in index order.  Ties keep the index order."""
    preds, maxprob = np.asarray(preds), np.asarray(maxprob, dtype=np.float32)
    classes = [1, 0] if n_classes == 2 else list(range(n_classes))
    out = []
    for cl in classes:
        idx = np.nonzero(preds == cl)[0]
        out += list(idx[np.argsort(-maxprob[idx], kind="stable")])
    out += list(np.nonzero(preds == -1)[0])
    return np.asarray(out, dtype=np.int32)


def grid_host(images, order, boxes, preds, maxprob, palette):
    """The numpy statement of ``fd_eval_grid_u8``: images [N,3,H,W] in [-1,1] (any float dtype), order [N] tile -> image, boxes [N,4]
    (x0,y0,x1,y1, both ends drawn), preds [N] (-1 = no face), maxprob [N] fp32, palette [(r,g,b)] indexed by pred + 1 -> uint8 grid.
    Per tile, in the reference's drawing order: pixels ``(x*0.5+0.5)*255`` truncated; a 4-pixel outline of the box in the class colour,
    clipped to the image; a 50-pixel strip of the class colour on the left; when p < 1 a white bar over columns 0..50 (the image's first
    column included) and rows 0..int((1-p)*512); a 10-pixel black frame.  Tiles past N are white."""
    N, _, H, W = images.shape
    rows, cols, shape = grid_shape(N, H, W)
    x = torch.as_tensor(images).float() * 0.5 + 0.5
    pix = x.mul(255).to(torch.uint8).permute(0, 2, 3, 1).contiguous().cpu().numpy()
    palette = np.asarray(palette, dtype=np.uint8)
    th, tw = H + 2 * FRAME, W + STRIP + 2 * FRAME
    grid = np.full(shape, 255, dtype=np.uint8)
    for t in range(N):
        i = int(order[t])
        col = palette[int(preds[i]) + 1]
        im = pix[i].copy()
        x0, y0, x1, y1 = (int(v) for v in boxes[i])
        yy, xx = np.mgrid[0:H, 0:W]
        # PIL's outline of width 4: rows y0..y0+3 and y1-3..y1 over x0..x1; columns x0..x0+3 and x1-3..x1 over the rows from ya = y0+4 towards
        # yb = y1-3, yb itself left out, in either direction (a box lower than 8 pixels -- the no-face box -1,-1,-1,-1 -- still gets those columns)
        hor = (((yy >= y0) & (yy < y0 + BOX_WIDTH)) | ((yy <= y1) & (yy > y1 - BOX_WIDTH))) & (xx >= x0) & (xx <= x1)
        ya, yb = y0 + BOX_WIDTH, y1 - BOX_WIDTH + 1
        lo, hi = (ya, yb - 1) if ya <= yb else (yb + 1, ya)
        ver = (((xx >= x0) & (xx < x0 + BOX_WIDTH)) | ((xx <= x1) & (xx > x1 - BOX_WIDTH))) & (yy >= lo) & (yy <= hi)
        im[hor | ver] = col
        tile = np.zeros((th, tw, 3), dtype=np.uint8)
        inner = tile[FRAME:FRAME + H, FRAME:FRAME + STRIP + W]
        inner[:, :STRIP] = col
        inner[:, STRIP:] = im
        p = float(np.float32(maxprob[i]))
        if p < 1:
            inner[:min(int((1 - p) * 512), H - 1) + 1, :STRIP + 1] = 255
        r, c = divmod(t, cols)
        grid[r * th:(r + 1) * th, c * tw:(c + 1) * tw] = tile
    return grid


# ------------------------------------------------------------------------------------------ grids with one strip per attribute
def grid_attrs_shape(N, H, W, n_attr):
    rows = int(math.sqrt(N))
    cols = math.ceil(N / rows)
    return rows, cols, (rows * (H + 2 * FRAME), cols * (W + STRIP * n_attr + 2 * FRAME), 3)


def paint_attrs_tiles(pix, order, boxes, preds, bar_rows, palettes):
    """The tile rule shared by ``evaluate_images.grid_attrs_host`` and ``grid_attrs_img_host``: pix [N,H,W,3] uint8, the image pixels as they are
    painted.  Per tile, in the reference's drawing order: a 4-pixel BLACK outline of the box (PIL's rule, ``grid_host``), clipped to the image; then
    from the innermost (last) attribute outwards a 50-pixel strip of the class colour on the left and its white bar over columns 0..50 of the image
    as expanded so far (one column of what lies to the right included) and rows 0..bar_rows; a 10-pixel black frame.  Tiles past N are white."""
    N, H, W, _ = pix.shape
    preds, bar_rows = np.asarray(preds), np.asarray(bar_rows)
    n_attr = preds.shape[0]
    rows, cols, shape = grid_attrs_shape(N, H, W, n_attr)
    th, tw = H + 2 * FRAME, W + STRIP * n_attr + 2 * FRAME
    grid = np.full(shape, 255, dtype=np.uint8)
    yy, xx = np.mgrid[0:H, 0:W]
    for t in range(N):
        i = int(order[t])
        im = pix[i].copy()
        x0, y0, x1, y1 = (int(v) for v in boxes[i])
        hor = (((yy >= y0) & (yy < y0 + BOX_WIDTH)) | ((yy <= y1) & (yy > y1 - BOX_WIDTH))) & (xx >= x0) & (xx <= x1)
        ya, yb = y0 + BOX_WIDTH, y1 - BOX_WIDTH + 1
        lo, hi = (ya, yb - 1) if ya <= yb else (yb + 1, ya)
        ver = (((xx >= x0) & (xx < x0 + BOX_WIDTH)) | ((xx <= x1) & (xx > x1 - BOX_WIDTH))) & (yy >= lo) & (yy <= hi)
        im[hor | ver] = 0
        for s in range(n_attr - 1, -1, -1):
            wide = np.empty((H, im.shape[1] + STRIP, 3), dtype=np.uint8)
            wide[:, :STRIP] = np.asarray(palettes[s][int(preds[s, i]) + 1], dtype=np.uint8)
            wide[:, STRIP:] = im
            if bar_rows[s, i] >= 0:
                wide[:min(int(bar_rows[s, i]), H - 1) + 1, :STRIP + 1] = 255
            im = wide
        tile = np.zeros((th, tw, 3), dtype=np.uint8)
        tile[FRAME:FRAME + H, FRAME:FRAME + im.shape[1]] = im
        r, c = divmod(t, cols)
        grid[r * th:(r + 1) * th, c * tw:(c + 1) * tw] = tile
    return grid


def grid_attrs_img_host(images, order, boxes, preds, bar_rows, palettes):
    """The numpy statement of ``fd_eval_grid_attrs``: images [N,3,H,W] in [-1,1] (any float dtype), order [N] tile -> image, boxes [N,4]
    (x0,y0,x1,y1, both ends drawn), preds / bar_rows [n_attr,N] (pred -1 = no face, bar_rows -1 = no bar), palettes [n_attr][(r,g,b)] indexed by
    pred + 1 -> uint8 grid.  Pixels by ``grid_host``'s rule, ``(x*0.5+0.5)*255`` truncated; tiles by ``paint_attrs_tiles``."""
    x = torch.as_tensor(images).float() * 0.5 + 0.5
    pix = x.mul(255).to(torch.uint8).permute(0, 2, 3, 1).contiguous().cpu().numpy()
    return paint_attrs_tiles(pix, order, boxes, preds, bar_rows, palettes)


def grid_inputs_attrs(pd, attrs):
    """(preds int32 [n,N], probs fp32 [n,N], bar_rows int32 [n,N], order int32 [N]) of the n = 2 or 3 attributes ``attrs`` = [(first column, k)] of
    the table, on the table's device.  Per attribute by the rules of ``grid_inputs``: -1 where any entry is -1, the FIRST maximum wins, the
    confidence is the row's maximum.  Bars by ``evaluate_images.grid_attrs_bar_rows`` (the age bar tests the race probability), the tile order by the
    rule of ``evaluate_images.grid_attrs_order`` with stable sorts (``device_order``)."""
    from .evaluate_images import device_order, grid_attrs_bar_rows
    assert len(attrs) in (2, 3), attrs
    preds, probs = [], []
    for c0, k in attrs:
        p = pd[:, c0:c0 + k]
        valid = (p != -1).all(dim=-1)
        mx = p.max(dim=-1).values
        cols = torch.arange(k, device=pd.device).expand_as(p)
        arg = torch.where(p == mx[:, None], cols, torch.full_like(cols, k)).min(dim=-1).values
        preds.append(torch.where(valid, arg, torch.full_like(arg, -1)))
        probs.append(mx.float())
    preds, probs = torch.stack(preds), torch.stack(probs).contiguous()
    return preds.to(torch.int32).contiguous(), probs, grid_attrs_bar_rows(probs), device_order(preds, probs)


def strip_palettes(tr):
    """One palette per strip, index = pred + 1.  The named experiments: gender, race, age, the reference's.  A custom run: by class count -- two
    classes the gender palette, four the race palette, three its first three class colours."""
    from .evaluate_images import PALETTES
    spec = getattr(tr, "spec", None)
    if spec is None or not spec.custom:
        return PALETTES[:len(tr.attrs)]
    return [PALETTE_GENDER if k == 2 else PALETTE_RACE[:k + 1] for k in spec.sizes]


def device_grid_attrs(tr, images, boxes, pd, labels=None):
    """The annotated grid with one strip per attribute (uint8 on the device), one launch of ``ops.eval_grid_attrs_img``: exp-3/5 gender and race
    (``plot_in_grid_gender_race``), exp-4 gender, race and age (``plot_in_grid_gender_race_age``).  The one-attribute experiments have their own
    reference function, which draws the box in the class colour: they get ``device_grid`` (exp-1/2 gender colours, exp-6 race colours).
    ``labels``: an ``IndexLabels`` -- the index text is drawn by one more launch behind the painter; None: the grid as it was without it."""
    if len(tr.attrs) == 1:
        return device_grid(tr, images, boxes, pd, labels=labels)
    from . import ops
    n = len(tr.attrs)
    preds, _, bar_rows, order = grid_inputs_attrs(pd, table_attrs(tr.attrs))
    palettes = strip_palettes(tr)
    P = max(len(p) for p in palettes)
    pal = torch.tensor([p + [(255, 255, 255)] * (P - len(p)) for p in palettes], dtype=torch.uint8, device=images.device)
    grid = ops.eval_grid_attrs_img(images.contiguous(), order, boxes.to(images.device, torch.int32).contiguous(), preds, bar_rows, pal)
    return draw_labels(grid, order, labels, images.shape[2], images.shape[3], n)


# ------------------------------------------------------------------------------------------ the index text
LABEL_XY = (400, 400)                # ``img_pil_draw.text((400, 400), f"{idx.item()}", align="left", font=fnt)`` (exp-1 :199-200)
LABEL_FONT_SIZE = 100


def label_blend(a, m):
    """PIL's blend of white ink under coverage m into the 8-bit channel value a: ``t = a*(255-m) + 255*m + 128; ((t >> 8) + t) >> 8``."""
    t = np.asarray(a, dtype=np.uint32) * (255 - np.asarray(m, dtype=np.uint32)) + 255 * np.asarray(m, dtype=np.uint32) + 128
    return (((t >> 8) + t) >> 8).astype(np.uint8)


def labels_host(grid, order, masks, desc, H, W, n_strip, cols, xy=LABEL_XY):
    """The numpy statement of ``fd_eval_grid_labels_u8``: a copy of ``grid`` [rows*(H+20), cols*(W+50*n_strip+20), 3] uint8 (painted by ``grid_host``,
    ``grid_attrs_img_host`` or ``evaluate_images.grid_attrs_host``) with the index text.  Tile t shows image i = order[t] and gets label i: the w x h
    coverage mask at ``masks[byte_offset:]`` with desc[i] = (w, h, off_x, off_y, byte_offset), its top-left at (xy[0] + off_x, xy[1] + off_y) of the
    tile's inner area (W + 50*n_strip by H, inside the frame).  What falls inside that area is blended as white ink (``label_blend``) over whatever the
    painter left there; the rest is clipped.  A tile whose order entry is outside [0, N), whose label the table does not hold, or whose descriptor
    does not lie inside ``masks`` gets nothing."""
    out = np.array(grid, dtype=np.uint8, copy=True)
    masks, desc = np.asarray(masks, dtype=np.uint8).reshape(-1), np.asarray(desc, dtype=np.int64).reshape(-1, 5)
    N, IW = len(order), W + STRIP * n_strip
    th, tw = H + 2 * FRAME, IW + 2 * FRAME
    for t in range(N):
        i = int(order[t])
        if not (0 <= i < N and i < len(desc)):
            continue
        w, h, ox, oy, off = (int(v) for v in desc[i])
        if w <= 0 or h <= 0 or off < 0 or off + w * h > masks.size:
            continue
        m = masks[off:off + w * h].reshape(h, w)
        x0, y0 = int(xy[0]) + ox, int(xy[1]) + oy
        ca, cb, ra, rb = max(0, -x0), min(w, IW - x0), max(0, -y0), min(h, H - y0)
        if ca >= cb or ra >= rb:
            continue
        r, c = divmod(t, cols)
        inner = out[r * th + FRAME:r * th + FRAME + H, c * tw + FRAME:c * tw + FRAME + IW]
        view = inner[y0 + ra:y0 + rb, x0 + ca:x0 + cb]
        view[...] = label_blend(view, m[ra:rb, ca:cb, None])
    return out


class IndexLabels:
    """The index text of the annotated grids: the strings "0", "1", ... rasterised with the caller's font as ``ImageDraw.text`` rasterises them for
    an RGB image with default arguments -- ``font.getmask2(s, "L", anchor="la")``, each string as a whole (advances are fractional and digits kern:
    concatenated digit masks are not the string's mask).  ``font``: the path of a TrueType / OpenType file (the reference uses Arial Bold, which is
    the user's to supply), or "default" for Pillow's embedded scalable font.  ``atlas(n, device)`` hands the kernel its two device buffers; ``xy`` is
    where the grid helpers anchor the text (the reference's (400, 400) lies outside an image smaller than that: such grids show no text)."""

    def __init__(self, font, size=LABEL_FONT_SIZE, xy=LABEL_XY):
        from PIL import ImageFont, features
        if not features.check("freetype2"):
            raise RuntimeError("index labels need a Pillow built with FreeType (PIL.features.check('freetype2') is False): install one, or run without --index_font")
        if int(size) < 1:
            raise ValueError(f"index label font size {size}: at least 1")
        if font == "default":
            if not hasattr(ImageFont, "load_default") or "size" not in ImageFont.load_default.__code__.co_varnames:
                raise RuntimeError("this Pillow has no scalable embedded font (ImageFont.load_default(size) needs Pillow 10.1): pass the path of a font file")
            self.font = ImageFont.load_default(int(size))
        else:
            if not os.path.isfile(font):
                raise FileNotFoundError(f"index label font {font!r} is not a file (pass the path of a .ttf / .otf file, or 'default')")
            self.font = ImageFont.truetype(font, int(size))
        self.name, self.size = font, int(size)
        self.xy = (int(xy[0]), int(xy[1]))          # the text's anchor inside the strip-expanded image; the reference's is fixed at (400, 400)
        self._masks, self._desc, self._bytes = [], [], 0          # host rasters of labels 0 .. len-1, grown on demand
        self._atlas = {}                                          # (n, device) -> (masks, desc) on the device

    def raster(self, text):
        """(mask uint8 [h,w], (w, h, off_x, off_y)) of one string: what ``ImageDraw.text(xy, text, font=font)`` blends at xy + (off_x, off_y)."""
        core, (ox, oy) = self.font.getmask2(text, "L", anchor="la")
        w, h = core.size
        return np.frombuffer(bytes(core), dtype=np.uint8, count=w * h).reshape(h, w), (w, h, int(ox), int(oy))

    def host(self, n):
        """(masks uint8 [bytes], desc int32 [n,5] = (w, h, off_x, off_y, byte_offset)) of the labels "0" .. str(n-1), packed in label order."""
        assert n >= 1, n
        for i in range(len(self._desc), n):
            mask, d = self.raster(str(i))
            self._masks.append(mask.reshape(-1))
            self._desc.append(d + (self._bytes,))
            self._bytes += mask.size
        desc = np.asarray(self._desc[:n], dtype=np.int32).reshape(n, 5)
        masks = np.concatenate(self._masks[:n]) if n else np.zeros(0, dtype=np.uint8)
        return np.ascontiguousarray(masks), desc

    def atlas(self, n, device):
        device = torch.device(device)
        key = (int(n), str(device))
        if key not in self._atlas:
            masks, desc = self.host(int(n))
            if masks.size == 0:
                raise RuntimeError(f"index label font {self.name!r} draws nothing for the digits")
            self._atlas[key] = (torch.from_numpy(masks).to(device), torch.from_numpy(desc).to(device))
        return self._atlas[key]


def draw_labels(grid, order, labels, H, W, n_strip):
    """The index text onto a grid the painter has just written, on the same stream directly behind it (one launch); ``labels`` None: nothing."""
    if labels is None:
        return grid
    from . import ops
    masks, desc = labels.atlas(order.shape[0], grid.device)
    return ops.eval_grid_labels(grid, order, masks, desc, H, W, n_strip, xy=getattr(labels, "xy", LABEL_XY))


# ------------------------------------------------------------------------------------------ the two functions of the reference's loop
def draw_val_noise(n_prompts, n_images, lat):
    """``noises_val`` (:1660-1663): drawn on the global CPU generator, so a run with validation consumes it exactly where the reference does."""
    return torch.randn([n_prompts, n_images, 4, lat, lat], dtype=torch.float32)


def validation_prompts(data):
    """``prompt_templates_test x occupations_val_set`` of the experiment data (:924)."""
    return [p.format(occupation=o) for p in data["prompt_templates_test"] for o in data["occupations_val_set"]]


def _frozen_pair(tr):
    """The ``_ori`` pass's models (:1469-1474): the frozen copy of whatever is being trained (exp-2: both networks are frozen anyway)."""
    a = tr.args
    te = tr.eval_te if (getattr(a, "train_text_encoder", False) or tr.prefix is not None) else tr.te
    unet = tr.eval_unet if (getattr(a, "train_unet", False) or tr.prefix is not None) else tr.unet
    return te, unet


def prefix_tokens_for(tr, toks):
    """exp-2: the token tuple of the prompt with the trainer's prefix placeholders in front, as ``train.py`` builds it for the step."""
    from .generate import prefix_tokens
    return prefix_tokens(toks, tr.prefix.n, tr.te.config.vocab_size)


def _generate(tr, te, unet, tokens, noises, prefix=None):
    vb = max(int(tr.args.val_GPU_batch_size), 1)
    enc = tr.encode_pair(te, tokens, prefix=prefix)
    out = []
    for j in range(0, noises.shape[0], vb):
        x, _, _ = tr.rollout(unet, enc, noises[j:j + vb], N_DENOISING_STEPS_VAL)
        out.append(tr.decode(x))
    return torch.cat(out)


def probability_table(tr, h):
    """[N, sum k] fp32 on the device from ``classify_begin``'s handle: softmax per attribute, -1 rows where no face was found."""
    from .step import _h2d
    pd = torch.full((h["N"], sum(k for _, _, k in tr.attrs)), -1.0, dtype=torch.float32, device=tr.device)
    if h["logits_dev"] is not None:
        pd[_h2d(h["sel"], tr.device)] = torch.cat([torch.softmax(h["logits_dev"][:, c0:c0 + k], dim=-1) for _, c0, k in tr.attrs], dim=1)
    return pd


def _gather_dev(tr, t):
    """All ranks' tensors concatenated in rank order on the device (``customized_all_gather``); the tensor itself on one rank."""
    if not tr.collectives:
        return t
    import torch.distributed as dist
    t = t.contiguous()
    gl = [torch.empty_like(t) for _ in range(dist.get_world_size())]
    dist.all_gather(gl, t)
    return torch.cat(gl)


def grid_inputs(pd, k0):
    """(preds int32 [N], maxprob fp32 [N], order int32 [N]) of the first attribute (columns 0..k0-1 of the table), on the table's device, by the
    rules of ``tally_host`` / ``grid_order``: -1 where any entry is -1, the FIRST maximum wins, classes in plot_in_grid's order (two classes: 1 then
    0; four: 0..3), each from the most to the least confident with ties in index order, then the images without a face."""
    p0 = pd[:, :k0]
    valid = (p0 != -1).all(dim=-1)
    maxprob = p0.max(dim=-1).values
    cols = torch.arange(k0, device=pd.device).expand_as(p0)
    arg = torch.where(p0 == maxprob[:, None], cols, torch.full_like(cols, k0)).min(dim=-1).values      # first maximum: a minimum has no tie rule to rely on
    preds = torch.where(valid, arg, torch.full_like(arg, -1)).to(torch.int32)
    group = torch.where(valid, (1 - arg) if k0 == 2 else arg, torch.full_like(arg, k0))
    by_conf = torch.sort(-maxprob, stable=True).indices
    order = by_conf[torch.sort(group[by_conf], stable=True).indices].to(torch.int32)
    return preds.contiguous(), maxprob.float().contiguous(), order.contiguous()


def device_grid(tr, images, boxes, pd, labels=None):
    """The annotated grid of the first attribute's predictions (uint8 on the device): predictions, confidences and the tile order are derived
    from the device table (``grid_inputs``), the painting is one launch of ``ops.eval_grid``; ``labels`` as in ``device_grid_attrs``."""
    from . import ops
    k0 = tr.attrs[0][2]
    preds, maxprob, order = grid_inputs(pd, k0)
    palette = torch.tensor(PALETTE_GENDER if k0 == 2 else PALETTE_RACE, dtype=torch.uint8, device=images.device)
    grid = ops.eval_grid(images.contiguous(), order, boxes.to(images.device, torch.int32).contiguous(), preds, maxprob, palette)
    return draw_labels(grid, order, labels, images.shape[2], images.shape[3], 1)


def _json_safe(v):
    """NaN (an empty valid set) is written as null: the line stays valid JSON for strict parsers."""
    if isinstance(v, dict):
        return {k: _json_safe(x) for k, x in v.items()}
    return None if isinstance(v, float) and math.isnan(v) else v


def evaluate_process(trainer, which, name, prompts_tokens, noises, step, mode="metrics", imgs_dir=None, log=print):
    """``evaluate_process`` (:1449-1571) for the weights the models currently hold.  ``which``: "main" or "EMA" -- it selects exp-2's prefix
    vectors; the LoRA operands are switched by ``evaluation_step``.  ``prompts_tokens``: [(prompt, token tuple)]; ``noises`` [P, n, 4, h, w] on the
    host.  Returns [{metric: value}] per prompt (every rank tallies the same gathered table; only rank 0 prints and writes).  In the JSON line a
    NaN (no valid row) is written as null.  With ``mode="grids"`` rank 0 also writes
    ``eval_{name}_{step}_{prompt}_{ori|generated}.jpg`` showing the first attribute; with ``"grids_attrs"`` the grids of exp-3/4/5 carry one strip
    per attribute (``device_grid_attrs``; the other experiments' files are the same in both modes); with ``"metrics"`` the frozen pass, which only
    feeds its grid, is not generated.  A trainer that carries ``index_labels`` (``--index_font``) gets the index text on every grid."""
    tr = trainer
    logs = []
    tr.last_eval_counts = []          # the int32 counts behind ``logs``, per prompt (what the tests compare with the host tally)
    tr.last_eval_joint = []           # custom runs with two or more attributes: the joint histogram read back with them, else None
    te_o, unet_o = _frozen_pair(tr)
    for (prompt, toks), noises_i in zip(prompts_tokens, noises):
        nd = noises_i.to(tr.device, torch.float32)
        toks_gen, toks_ori, pv = toks, toks, None
        if tr.prefix is not None:
            toks_gen = prefix_tokens_for(tr, toks)
            toks_ori = (toks[0], toks[1], toks[2], torch.ones_like(toks[3]))
            pv = tr.prefix.vectors(ema=(which == "EMA"))
        grids = mode in ("grids", "grids_attrs")
        painter = device_grid_attrs if mode == "grids_attrs" else device_grid
        passes = ([("ori", te_o, unet_o, toks_ori, None)] if grids else []) + [("generated", tr.te, tr.unet, toks_gen, pv)]
        for tag, te, unet, tk, prefix in passes:
            images = _generate(tr, te, unet, tk, nd, prefix=prefix)
            h = tr.classify_begin(images)
            pd = _gather_dev(tr, probability_table(tr, h))
            if tag == "generated":
                counts, joint = split_counts(tally_with_joint(tr, pd).cpu())          # the evaluation's read-back: 32 integers (custom: and the cells)
                tr.last_eval_counts.append(counts)
                tr.last_eval_joint.append(joint)
                logs.append(gap_metrics(tr.experiment, counts, getattr(tr, "spec", None), joint))
            if grids:
                images_all, boxes_all = _gather_dev(tr, images), _gather_dev(tr, h["boxes"].to(tr.device, torch.int32))
                if tr.rank == 0:
                    from PIL import Image
                    os.makedirs(imgs_dir, exist_ok=True)
                    grid = painter(tr, images_all, boxes_all, pd, labels=getattr(tr, "index_labels", None)).cpu().numpy()
                    Image.fromarray(grid).save(os.path.join(imgs_dir, f"eval_{name}_{step}_{prompt}_{tag}.jpg"), quality=25)
    if tr.rank == 0 and log is not None:
        keys = list(logs[0].keys()) if logs else []
        log(json.dumps(_json_safe({"eval": name, "step": step, "per_prompt": {p: m for (p, _), m in zip(prompts_tokens, logs)},
                                   "mean": {k: float(np.array([m[k] for m in logs]).mean()) for k in keys}})))
    return logs


def evaluation_step(trainer, tokenizer, prompts_val, step, noises_val=None, mode="metrics", imgs_dir=None, log=print):
    """``evaluation_step`` (:1659-1690): validation noise from the global CPU generator, the live weights ("main"), then the EMA weights ("EMA").
    The EMA pass rewrites the 16-bit LoRA operand copies from ``bank.ema`` and restores them from ``bank.flat``: the fp32 parameters, their EMA and
    the optimiser moments are never written."""
    tr = trainer
    a = tr.args
    if noises_val is None:
        noises_val = draw_val_noise(len(prompts_val), a.val_images_per_prompt_GPU, tr.unet.config.sample_size)
    tr.finish_r2_prefetch()          # the frozen U-Net may hold a prefetched rollout of the next step: completed first, not dropped
    pt = [(p, tokenizer(p)) for p in prompts_val]
    out = {"main": evaluate_process(tr, "main", "main", pt, noises_val, step, mode=mode, imgs_dir=imgs_dir, log=log)}
    nets = [n for n, on in ((tr.unet, getattr(a, "train_unet", False)), (tr.te, getattr(a, "train_text_encoder", False)))
            if on and tr.prefix is None and n.lora_bank is not None]
    try:
        for n in nets:
            n.refresh_lora(ema=True)
        out["EMA"] = evaluate_process(tr, "EMA", "EMA", pt, noises_val, step, mode=mode, imgs_dir=imgs_dir, log=log)
    finally:
        for n in nets:
            n.refresh_lora()
    if tr._side is not None and "r2" in tr._side:
        tr._side["r2"].wait_stream(torch.cuda.current_stream())      # the next step's frozen rollout starts behind the validation's use of that U-Net
    return out
