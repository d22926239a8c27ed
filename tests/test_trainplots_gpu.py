"""The training monitor on the GPU with the tiny models, through ``train.main``: the gated ``train_`` metrics of every step against the host tally,
a run with the monitor on against the same run with it off, the train plots against the host statement, ``--validation grids_attrs``, and two gloo
ranks on one device."""
import json
import math
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
from test_kernels_trainplots_gpu import _host_inputs  # noqa: E402
from test_two_rank_gpu import _free_port  # noqa: E402

pytestmark = pytest.mark.gpu

KEYS = {"exp-1": {"gender_gap", "gender_gap_abs", "gender_pred_between_0.2_0.8"},
        "exp-4": {"gender_gap", "gender_pred_below_0.8", "race_gap", "race_pred_below_0.8", "gender_race_gap", "age_young_freq", "age_old_freq",
                  "age_pred_below_0.8", "age_gap"},
        "exp-6": {"race0_freq", "race1_freq", "race2_freq", "race3_freq", "race_gap", "race_pred_below_0.8"}}
B = 4
_RUNS = {}


def _run(tmp_path_factory, experiment, steps, extra):
    """One run of the driver (cached per argument list): (records, trainer, output directory, the gathered R1 table of every step)."""
    key = (experiment, steps) + tuple(extra)
    if key in _RUNS:
        return _RUNS[key]
    from finetune_fair_diffusion_amd import train
    from finetune_fair_diffusion_amd.factory import TINY
    out = tmp_path_factory.mktemp("trainplots")
    argv = ["--experiment", experiment, "--synthetic", "--train_unet", "--rank", "4", "--max_train_steps", str(steps), "--checkpointing_steps", "100",
            "--checkpointing_steps_long", "100", "--num_denoising_steps", "3", "--train_images_per_prompt_GPU", str(B), "--train_GPU_batch_size", "3",
            "--val_GPU_batch_size", "4", "--val_images_per_prompt_GPU", "5", "--learning_rate", "2e-3", "--output_dir", str(out), "--weight_loss_img", "0",
            "--weight_loss_face", "0", "--uncertainty_threshold", "0.6", "--evaluate_every_n_iter", "5"] + list(extra)
    holder, lines, tables = {}, [], []
    build = train.build_trainer

    def capture(*a, **kw):
        holder["tr"], models = build(*a, **kw)
        return holder["tr"], models

    def log(s):
        lines.append(s)
        mon = holder["tr"].last_monitor
        if "eval" not in json.loads(s) and mon is not None:
            tables.append(mon["tables"]["generated"].cpu())
    train.build_trainer = capture
    try:
        tr, n = train.main(argv, cfgs=TINY, log=log)
    finally:
        train.build_trainer = build
    assert n == steps and tr is holder["tr"]
    _RUNS[key] = ([json.loads(s) for s in lines], tr, out, tables)
    return _RUNS[key]


def _monitor_keys(rec):
    return {k for k in rec if k.startswith("train_") or k.startswith("num_faces")}


def _same(a, b):
    return a == b or (a is None and math.isnan(b))


@pytest.mark.parametrize("experiment", ["exp-1", "exp-4", "exp-6"])
def test_metrics_records_carry_the_gap_metrics_of_the_table_the_step_classified(dev, tmp_path_factory, experiment):
    from finetune_fair_diffusion_amd import evaluation as E
    recs, tr, out, tables = _run(tmp_path_factory, experiment, 2, ["--train_monitor", "metrics"])
    assert len(recs) == len(tables) == 2 and not os.path.exists(out / "imgs")
    for rec, table in zip(recs, tables):
        assert _monitor_keys(rec) == {f"train_{k}" for k in KEYS[experiment]} | {"num_faces", "num_faces_total"}
        assert table.shape == (B, sum(k for _, _, k in tr.attrs))
        want = E.gap_metrics(experiment, E.tally_host(table, E.table_attrs(tr.attrs)))
        print(experiment, rec["step"], {k: rec[f"train_{k}"] for k in want})
        for k, v in want.items():
            assert _same(rec[f"train_{k}"], v), (k, rec[f"train_{k}"], v)
        valid = (table != -1).all(dim=-1)
        assert rec["num_faces"] == int(valid.sum()) > 0 and rec["num_faces_total"] == B
        # the table is the one behind the step's own report: its second column is the record's p_class1_mean
        assert rec["p_class1_mean"] == pytest.approx(float(table[:, 1][valid].mean()), abs=1e-6)
    assert tr.last_monitor["images"] == {} and tr.last_monitor["grids"] == {} and set(tr.last_monitor["tables"]) == {"generated"}


@pytest.mark.parametrize("experiment", ["exp-1", "exp-4"])
def test_a_run_with_plots_equals_the_run_without_the_monitor(dev, tmp_path_factory, experiment):
    """Equal seeds, monitor off against plots: no random number is drawn and nothing in the step is reordered in a way that changes a result."""
    off, tr_off, out_off, _ = _run(tmp_path_factory, experiment, 3, ["--train_plot_every_n_iter", "2"])
    on, tr_on, _, _ = _run(tmp_path_factory, experiment, 3, ["--train_plot_every_n_iter", "2", "--train_monitor", "plots"])
    assert len(off) == len(on) == 3 and all(_monitor_keys(r) == set() for r in off) and all(_monitor_keys(r) for r in on)
    assert tr_off.last_monitor is None and not os.path.exists(out_off / "imgs")
    strip = lambda r: {k: v for k, v in r.items() if k != "seconds" and k not in _monitor_keys(r)}
    for a, b in zip(off, on):
        assert a["loss_fair"] == b["loss_fair"] and a["loss_fair"] is not None and a["noise_checksum"] == b["noise_checksum"]
        assert strip(a) == strip(b)
    assert len(tr_off.banks) == len(tr_on.banks) > 0
    for x, y in zip(tr_off.banks, tr_on.banks):
        for name in ("flat", "ema", "exp_avg", "exp_avg_sq"):
            assert torch.equal(getattr(x, name).view(torch.uint8), getattr(y, name).view(torch.uint8)), name
    assert float((tr_on.banks[0].flat - tr_on.banks[0].ema).abs().max()) > 0            # the steps did update


@pytest.mark.parametrize("experiment", ["exp-1", "exp-3", "exp-4"])
def test_plot_files_and_painted_arrays(dev, tmp_path_factory, experiment):
    from PIL import Image
    from finetune_fair_diffusion_amd import evaluate_images as EI, evaluation as E
    recs, tr, out, _ = _run(tmp_path_factory, experiment, 3, ["--train_plot_every_n_iter", "2", "--train_monitor", "plots"])
    # steps 0, 1, 2 of epoch 0: the reference plots the first and the third and names them by the global step before its increment
    assert set(os.listdir(out / "imgs")) == {f"train-{n}_{t}.jpg" for n in (0, 2) for t in ("generated", "ori")}
    n_attr = len(tr.attrs)
    H = W = 8 * tr.unet.config.sample_size
    shape = E.grid_shape(B, H, W)[2] if n_attr == 1 else E.grid_attrs_shape(B, H, W, n_attr)[2]
    for f in os.listdir(out / "imgs"):
        assert Image.open(out / "imgs" / f).size == (shape[1], shape[0]), f
    mon = tr.last_monitor                                         # of the third step, a plot step
    assert set(mon["grids"]) == set(mon["images"]) == set(mon["boxes"]) == set(mon["tables"]) == {"generated", "ori"}
    for tag in ("generated", "ori"):
        images, boxes, pd = mon["images"][tag], mon["boxes"][tag], mon["tables"][tag]
        assert images.shape == (B, 3, H, W) and images.is_cuda and boxes.shape == (B, 4) and pd.shape[0] == B
        got = E.device_grid_attrs(tr, images, boxes, pd).cpu().numpy()
        assert np.array_equal(got, mon["grids"][tag].numpy()) and got.shape == shape
        if n_attr == 1:
            p0 = pd.cpu()[:, :2]
            valid = (p0 != -1).all(dim=-1)
            preds = torch.where(valid, p0.argmax(dim=-1), torch.full((B,), -1)).numpy()
            maxprob = p0.max(dim=-1).values.numpy()
            ref = E.grid_host(images.cpu(), E.grid_order(preds, maxprob), boxes.cpu().numpy(), preds, maxprob, E.PALETTE_GENDER)
        else:
            preds, probs, bars, order = _host_inputs(EI, pd.cpu(), E.table_attrs(tr.attrs))
            ref = E.grid_attrs_img_host(images.cpu(), order, boxes.cpu().numpy(), preds, bars, EI.PALETTES[:n_attr])
        assert np.array_equal(got, ref), (tag, int((got != ref).sum()))
    assert torch.equal(mon["images"]["generated"], mon["images"]["generated"].clamp(-1, 1)) and not torch.equal(mon["images"]["generated"], mon["images"]["ori"])


def test_validation_grids_attrs(dev, tmp_path_factory):
    """exp-4: three strips per tile.  exp-1: the files of ``grids_attrs`` are those of ``grids``, byte for byte."""
    from PIL import Image
    from finetune_fair_diffusion_amd import evaluation as E, train
    prompts = E.validation_prompts(train.SYNTHETIC_PROMPTS)
    want = {f"eval_{n}_0_{p}_{t}.jpg" for n in ("main", "EMA") for p in prompts for t in ("ori", "generated")}
    recs, tr, out, _ = _run(tmp_path_factory, "exp-4", 1, ["--validation", "grids_attrs"])
    H = W = 8 * tr.unet.config.sample_size
    assert set(os.listdir(out / "imgs")) == want and [r["eval"] for r in recs if "eval" in r] == ["main", "EMA"]
    shape = E.grid_attrs_shape(5, H, W, 3)[2]
    for f in want:
        assert Image.open(out / "imgs" / f).size == (shape[1], shape[0]) and shape[1] == 3 * (W + 170)
    _, _, out_a, _ = _run(tmp_path_factory, "exp-1", 1, ["--validation", "grids_attrs"])
    _, _, out_g, _ = _run(tmp_path_factory, "exp-1", 1, ["--validation", "grids"])
    assert set(os.listdir(out_a / "imgs")) == set(os.listdir(out_g / "imgs")) == want
    for f in want:
        assert open(out_a / "imgs" / f, "rb").read() == open(out_g / "imgs" / f, "rb").read(), f
        assert Image.open(out_a / "imgs" / f).size[0] == 3 * (W + 70)


def test_two_ranks_gather_in_rank_order_and_only_rank_0_paints(dev, tmp_path):
    from finetune_fair_diffusion_amd import evaluate_images as EI, evaluation as E
    from finetune_fair_diffusion_amd.fairness import EXPERIMENT_ATTRS
    import run_two_rank_step as R
    env = dict(os.environ)
    for k in ("FD_DTYPE", "FAIRDIFF_LIB", "RANK", "WORLD_SIZE", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT"):
        env.pop(k, None)
    env["HSA_ENABLE_IPC_MODE_LEGACY"] = "0"
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "2", "--master-addr", "127.0.0.1",
           "--master-port", str(_free_port()), os.path.join(HERE, "run_two_rank_monitor.py"), "exp-3", str(tmp_path)]
    r = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=900)
    print(r.stdout[-3000:])
    print(r.stderr[-3000:])
    for k in range(2):
        ep = os.path.join(tmp_path, f"rank{k}.err")
        if os.path.exists(ep):
            print(f"---- rank {k} traceback\n" + open(ep).read()[-2500:])
    assert r.returncode == 0, "two-rank monitor step failed"
    r0, r1 = (torch.load(os.path.join(tmp_path, f"rank{k}.pt"), weights_only=False) for k in range(2))
    attrs = E.table_attrs(EXPERIMENT_ATTRS["exp-3"][1])
    Bg = 2 * R.B_PER_RANK
    for tag in ("generated", "ori"):
        assert not torch.equal(r0["own_images"][tag], r1["own_images"][tag])          # each rank generated from its own noise
        for r in (r0, r1):                                                             # every rank holds the concatenation in rank order
            assert torch.equal(r["images"][tag], torch.cat([r0["own_images"][tag], r1["own_images"][tag]]))
            assert torch.equal(r["tables"][tag], torch.cat([r0["own_tables"][tag], r1["own_tables"][tag]]))
            assert r["boxes"][tag].shape == (Bg, 4)
        assert torch.equal(r0["boxes"][tag], r1["boxes"][tag])
    want = E.tally_host(r0["tables"]["generated"], attrs)
    assert int(want[0]) > 0 and torch.equal(r0["counts"], want) and torch.equal(r1["counts"], want)
    assert not torch.equal(want, E.tally_host(r0["own_tables"]["generated"], attrs))  # ... which is not rank 0's own table
    # rank 0 painted 2 x B tiles, rank 1 nothing
    assert set(r0["grids"]) == {"generated", "ori"} and r1["grids"] == {}
    shape = E.grid_attrs_shape(Bg, 256, 256, 2)[2]
    for tag in ("generated", "ori"):
        preds, probs, bars, order = _host_inputs(EI, r0["tables"][tag], attrs)
        ref = E.grid_attrs_img_host(r0["images"][tag], order, r0["boxes"][tag].numpy(), preds, bars, EI.PALETTES[:2])
        assert r0["grids"][tag].numpy().shape == shape and np.array_equal(r0["grids"][tag].numpy(), ref), tag
