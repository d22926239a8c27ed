"""The index text end to end on the GPU: the grid helpers of the offline evaluator and of the validation / training monitor with ``labels=`` against
the host statements at the reference's geometry (448 rows: the text at (400, 400) is visible), and a train-monitor ``plots`` run of the tiny models
with and without labels -- identical training state, grids that differ inside the label rectangles only.  The label masks come from the golden file
(``GoldenLabels`` has the two members of ``evaluation.IndexLabels`` the helpers use): neither a font nor FreeType is needed here."""
import json
import os
import sys

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
from test_kernels_trainplots_gpu import _host_inputs  # noqa: E402

pytestmark = pytest.mark.gpu
GOLD = os.path.join(HERE, "golden")
N, H, W, B = 5, 448, 384, 4


class GoldenLabels:
    """The recorded atlas of DejaVuSans-Bold at 100 behind ``IndexLabels``' interface."""

    def __init__(self, g, xy=(400, 400)):
        self.masks, self.desc, self.xy, self.calls = torch.from_numpy(g["masks"]), torch.from_numpy(g["desc"]), xy, []

    def atlas(self, n, device):
        self.calls.append(n)
        return self.masks.to(device), self.desc[:n].contiguous().to(device)


@pytest.fixture(scope="module")
def G():
    g = dict(np.load(os.path.join(GOLD, "reference_indexlabels_grid.npz")))
    b = int(g["block"])
    g["images"] = torch.from_numpy(g["blocks"]).repeat_interleave(b, dim=2).repeat_interleave(b, dim=3).contiguous()
    g["u8"] = torch.from_numpy(g["u8_blocks"]).repeat_interleave(b, dim=1).repeat_interleave(b, dim=2).contiguous()
    return g


def _table(seed):
    """[N, 8] probability table (gender, race, age) with a -1 row and two equal rows."""
    g = torch.Generator().manual_seed(seed)
    t = torch.cat([torch.softmax(torch.randn(N, k, generator=g) * 2, dim=-1) for k in (2, 4, 2)], dim=1)
    t[1] = t[0]
    t[3] = -1
    return t.float().contiguous()


@pytest.mark.parametrize("which", ["gender_race", "gender_race_age"])
def test_offline_device_grid_with_labels_equals_the_host_statement(dev, G, which):
    from finetune_fair_diffusion_amd import evaluate_images as EI, evaluation as E
    n = 2 if which == "gender_race" else 3
    t = _table(11)
    t[3] = t[2].flip(0)                                           # the evaluator's predictions are never -1
    probs = [t[:, :2].contiguous(), t[:, 2:6].contiguous(), t[:, 6:].contiguous()]
    boxes = torch.from_numpy(G["boxes"])
    labels = GoldenLabels(G)
    args = (G["u8"].to(dev), boxes.to(dev), [p.to(dev) for p in probs], which)
    plain = EI.device_grid(*args).cpu().numpy()
    got = EI.device_grid(*args, labels=labels).cpu().numpy()
    preds, pb, bars, order = _host_inputs(EI, t, EI.TABLE_ATTRS[:n])
    host = EI.grid_attrs_host(G["u8"].numpy(), order, G["boxes"], preds, bars, EI.PALETTES[:n])
    assert np.array_equal(plain, host) and labels.calls == [N]
    want = E.labels_host(host, order, G["masks"], G["desc"], H, W, n, 3)
    assert np.array_equal(got, want) and (got != plain).any(), int((got != want).sum())


@pytest.mark.parametrize("n_attr", [1, 3])
def test_device_grid_attrs_with_labels_equals_the_host_statement(dev, G, n_attr):
    from finetune_fair_diffusion_amd import evaluate_images as EI, evaluation as E, ops

    class Tr:
        attrs = [("gender", 0, 2), ("race", 2, 4), ("age", 6, 2)][:n_attr]
    t = _table(12)
    pd = t[:, :2].contiguous() if n_attr == 1 else t
    images = G["images"].to(ops.F16)
    labels = GoldenLabels(G)
    args = (Tr, images.to(dev), torch.from_numpy(G["boxes"]).to(dev), pd.to(dev))
    plain = E.device_grid_attrs(*args).cpu().numpy()
    got = E.device_grid_attrs(*args, labels=labels).cpu().numpy()
    assert np.array_equal(E.device_grid_attrs(*args, labels=None).cpu().numpy(), plain)
    if n_attr == 1:
        preds, maxprob, order = (v.numpy() for v in E.grid_inputs(pd, 2))
        host = E.grid_host(images, order, G["boxes"], preds, maxprob, E.PALETTE_GENDER)
        assert np.array_equal(E.device_grid(*args, labels=labels).cpu().numpy(), got)
    else:
        preds, pb, bars, order = _host_inputs(EI, pd, E.table_attrs(Tr.attrs))
        host = E.grid_attrs_img_host(images, order, G["boxes"], preds, bars, EI.PALETTES[:n_attr])
    assert np.array_equal(plain, host)
    want = E.labels_host(host, order, G["masks"], G["desc"], H, W, n_attr, 3)
    assert np.array_equal(got, want) and (got != plain).any(), int((got != want).sum())


def _run(tmp_path_factory, labels):
    """Three steps of exp-4's driver with the tiny models and train plots every second step; ``labels`` is put on the trainer as ``--index_font`` would."""
    from finetune_fair_diffusion_amd import train
    from finetune_fair_diffusion_amd.factory import TINY
    out = tmp_path_factory.mktemp("indexlabels")
    argv = ["--experiment", "exp-4", "--synthetic", "--train_unet", "--rank", "4", "--max_train_steps", "3", "--checkpointing_steps", "100",
            "--checkpointing_steps_long", "100", "--num_denoising_steps", "3", "--train_images_per_prompt_GPU", str(B), "--train_GPU_batch_size", "3",
            "--val_GPU_batch_size", "4", "--val_images_per_prompt_GPU", "5", "--learning_rate", "2e-3", "--output_dir", str(out), "--weight_loss_img", "0",
            "--weight_loss_face", "0", "--uncertainty_threshold", "0.6", "--evaluate_every_n_iter", "5", "--train_plot_every_n_iter", "2",
            "--train_monitor", "plots"]
    holder, lines, streams = {}, [], []
    build = train.build_trainer

    def capture(*a, **kw):
        holder["tr"], models = build(*a, **kw)
        assert holder["tr"].index_labels is None                  # no flag: the trainer carries no labels
        holder["tr"].index_labels = labels
        return holder["tr"], models
    train.build_trainer = capture
    try:
        tr, n = train.main(argv, cfgs=TINY, log=lines.append)
    finally:
        train.build_trainer = build
    assert n == 3
    return [json.loads(s) for s in lines], tr, out


def test_train_plots_with_labels_leave_the_training_state_identical(dev, tmp_path_factory, G):
    from finetune_fair_diffusion_amd import evaluation as E
    labels = GoldenLabels(G, xy=(100, 150))                       # the tiny models paint 256 x 256 images: an anchor inside them
    off, tr_off, _ = _run(tmp_path_factory, None)
    on, tr_on, out_on = _run(tmp_path_factory, labels)
    assert set(os.listdir(out_on / "imgs")) == {f"train-{n}_{t}.jpg" for n in (0, 2) for t in ("generated", "ori")}
    strip = lambda r: {k: v for k, v in r.items() if k != "seconds"}
    assert len(off) == len(on) == 3 and [strip(r) for r in off] == [strip(r) for r in on] and off[0]["loss_fair"] is not None
    assert len(tr_off.banks) == len(tr_on.banks) > 0
    for x, y in zip(tr_off.banks, tr_on.banks):
        for name in ("flat", "ema", "exp_avg", "exp_avg_sq"):
            assert torch.equal(getattr(x, name).view(torch.uint8), getattr(y, name).view(torch.uint8)), name
    assert labels.calls == [B] * 4                                 # two plot steps, two sides each; nothing on the step between them
    Ht = Wt = 8 * tr_on.unet.config.sample_size
    assert Ht > 150 + 20 and Wt + 150 > 100 + 70
    rows, cols, shape = E.grid_attrs_shape(B, Ht, Wt, 3)
    for tag in ("generated", "ori"):
        a, b = tr_off.last_monitor["grids"][tag].numpy(), tr_on.last_monitor["grids"][tag].numpy()
        pd = tr_on.last_monitor["tables"][tag]
        assert torch.equal(pd, tr_off.last_monitor["tables"][tag])
        order = E.grid_inputs_attrs(pd, E.table_attrs(tr_on.attrs))[3].cpu().numpy()
        assert np.array_equal(b, E.labels_host(a, order, G["masks"], G["desc"][:B], Ht, Wt, 3, cols, xy=labels.xy)), tag
        inside = np.zeros(shape[:2], dtype=bool)
        for t in range(B):
            w, h, ox, oy, _ = (int(v) for v in G["desc"][order[t]])
            r, c = divmod(t, cols)
            y0, x0 = r * (Ht + 20) + 10 + 150 + oy, c * (Wt + 170) + 10 + 100 + ox
            inside[y0:min(y0 + h, r * (Ht + 20) + 10 + Ht), x0:x0 + w] = True
        assert (a != b).any() and np.array_equal(a[~inside], b[~inside]), tag
