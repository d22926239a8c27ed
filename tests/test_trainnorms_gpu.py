"""``--log_norms`` on the GPU with the tiny models: ``FairnessTrainer.last_norms`` after ``sync_and_update`` -- an applied step, a skipped one, the
reduction alone -- against fp64 torch norms of the banks' views within the bound derived in tests/banknorms_cases.py (18 * 2^-24 + 2^-38 per norm, one
more fp32 rounding for a mean), a trainer with the option on against one with it off bit for bit, and the JSON lines of ``train.main``."""
import json
import math
import os
import sys

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import banknorms_cases as C  # noqa: E402

pytestmark = pytest.mark.gpu
NEW_KEYS = ("train_unet_lora_norm", "train_unet_lora_ema_norm", "grad_norm_unet_lora")
STATE = ("flat", "ema", "exp_avg", "exp_avg_sq")


def _train_argv(out_dir, steps, extra=()):
    """The driver arguments of tests/test_engine_gpu.py's ``_train_argv``."""
    return ["--synthetic", "--train_unet", "--rank", "4", "--max_train_steps", str(steps), "--checkpointing_steps", "2",
            "--checkpointing_steps_long", "3", "--checkpoints_total_limit", "2", "--num_denoising_steps", "3",
            "--train_images_per_prompt_GPU", "4", "--train_GPU_batch_size", "3", "--val_GPU_batch_size", "4",
            "--lr_scheduler", "linear", "--lr_warmup_steps", "1", "--learning_rate", "1e-5", "--output_dir", str(out_dir),
            "--weight_loss_img", "0", "--weight_loss_face", "0"] + list(extra)


def _trainer(dev, tmp, log_norms):
    from finetune_fair_diffusion_amd.cli import parse_args
    from finetune_fair_diffusion_amd.factory import TINY, build_trainer
    args = parse_args(["--synthetic", "--train_unet", "--train_text_encoder", "--rank", "4", "--learning_rate", "1e-3", "--output_dir", str(tmp),
                       "--weight_loss_img", "0", "--weight_loss_face", "0", "--lora_up_std", "0.05"], with_extras=True)
    tr, _ = build_trainer(args, dev, TINY, seed=args.seed, lora_up_std=args.lora_up_std)
    tr.log_norms = log_norms
    return tr


def _write_grads(tr, seed):
    """Seeded normal gradients over the WHOLE flat buffers: the padding slots hold values too, and no norm may count them."""
    g = torch.Generator().manual_seed(seed)
    for bank in tr.banks:
        bank.grad.copy_(torch.randn(bank.numel, generator=g) * 1e-3)


def _check(tag, bank, report, nonzero=False):
    """One bank's record against fp64 norms of its views as they stand now; every figure is printed before it is asserted."""
    per = {n: tuple(float(torch.linalg.vector_norm(bank.view(n, buf).double())) for buf in (bank.flat, bank.ema, bank.grad)) for n in bank.names}
    assert list(report["per_tensor"]) == bank.names
    worst = max(abs(g - r) / r for n in bank.names for g, r in zip(report["per_tensor"][n], per[n]) if r > 0)
    assert all(g == 0 for n in bank.names for g, r in zip(report["per_tensor"][n], per[n]) if r == 0), "an all-zero tensor has norm exactly 0"
    cols = [np.array([per[n][k] for n in bank.names]) for k in range(3)]
    figs = dict(param_mean=(cols[0].mean(), C.MEAN_BOUND), ema_mean=(cols[1].mean(), C.MEAN_BOUND), param_l2=(math.sqrt((cols[0] ** 2).sum()), C.BOUND),
                ema_l2=(math.sqrt((cols[1] ** 2).sum()), C.BOUND), grad_l2=(math.sqrt((cols[2] ** 2).sum()), C.BOUND))
    errs = {k: abs(report[k] - ref) / ref for k, (ref, _) in figs.items()}
    print(f"[{tag}] per-tensor max rel err {worst:.3e} (bound {C.BOUND:.3e}); " + "; ".join(f"{k} {e:.3e}" for k, e in errs.items()))
    assert worst <= C.BOUND and (not nonzero or all(min(per[n]) > 0 for n in bank.names))
    for k, (ref, bound) in figs.items():
        assert errs[k] <= bound, (tag, k, report[k], ref)
    for k, col in (("param_mean", 0), ("ema_mean", 1)):
        assert np.float32(report[k]) == np.float32(np.mean([np.float64(np.float32(report["per_tensor"][n][col])) for n in bank.names]))


@pytest.fixture(scope="module")
def pair(dev, tmp_path_factory):
    """Two trainers of equal seed that took the same ``sync_and_update``, the first with ``log_norms`` on."""
    tmp = tmp_path_factory.mktemp("trainnorms")
    on, off = _trainer(dev, tmp, True), _trainer(dev, tmp, False)
    for tr in (on, off):
        _write_grads(tr, 7)
        assert tr.sync_and_update(2) is True
    torch.cuda.synchronize()
    return on, off


def test_norms_after_an_applied_step_and_the_update_is_untouched(pair):
    on, off = pair
    assert on.bank_keys == ["unet_lora", "TE_lora"] and list(on.last_norms) == on.bank_keys and off.last_norms is None
    assert all(b._norm_plan is None for b in off.banks) and off._norms_host is None, "off: no table, no buffer"
    for key, bank in zip(on.bank_keys, on.banks):
        _check(key, bank, on.last_norms[key], nonzero=True)         # --lora_up_std above zero: no tensor is trivially zero
        assert float((bank.flat - bank.ema).abs().max()) > 0, "the step did update"
    assert (on.opt_step, on.lr_step) == (off.opt_step, off.lr_step) == (1, 1) and on.last_lr == off.last_lr > 0
    for x, y in zip(on.banks, off.banks):
        for name in STATE + ("grad",):
            assert torch.equal(getattr(x, name).view(torch.uint8), getattr(y, name).view(torch.uint8)), name


def test_skipped_step_and_reduction_alone(pair):
    on, _ = pair
    before = [{name: getattr(b, name).clone() for name in STATE} for b in on.banks]
    opt_step, decays = on.opt_step, [dict(e.__dict__) for e in on.ema]
    _write_grads(on, 8)
    name = on.banks[0].names[3]
    on.banks[0].grad_view(name).view(-1)[1] = float("inf")
    assert on.sync_and_update(2) is False
    r = on.last_norms["unet_lora"]
    assert math.isinf(r["grad_l2"]) and math.isinf(r["per_tensor"][name][2]) and sum(math.isinf(v[2]) for v in r["per_tensor"].values()) == 1
    assert math.isfinite(on.last_norms["TE_lora"]["grad_l2"])
    on.banks[0].grad_view(name).view(-1)[1] = 0.0           # the references below are taken from the banks as they stand
    for key, bank in zip(on.bank_keys, on.banks):
        rep = dict(on.last_norms[key])
        if key == "unet_lora":
            rep["grad_l2"] = float(torch.linalg.vector_norm(torch.cat([bank.grad_view(n).reshape(-1) for n in bank.names]).double()))
            rep["per_tensor"] = {n: (v[0], v[1], v[2] if n != name else float(torch.linalg.vector_norm(bank.grad_view(n).double())))
                                 for n, v in rep["per_tensor"].items()}
        _check(key + ", skipped step", bank, rep)
    # the reduction alone
    _write_grads(on, 9)
    assert on.sync_and_update(2, apply=False) is True
    for key, bank in zip(on.bank_keys, on.banks):
        _check(key + ", apply=False", bank, on.last_norms[key])
    assert on.opt_step == opt_step and [e.__dict__ for e in on.ema] == decays
    for bank, was in zip(on.banks, before):
        for k, t in was.items():
            assert torch.equal(getattr(bank, k).view(torch.uint8), t.view(torch.uint8)), f"{k} changed although nothing was applied"


def _drive(tmp, extra, experiment=None, argv=None, steps=3):
    """``train.main`` with the tiny models: (records, trainer, ``last_norms`` as it stood when each line was written)."""
    from finetune_fair_diffusion_amd import train
    from finetune_fair_diffusion_amd.factory import TINY
    holder, lines, seen = {}, [], []
    build = train.build_trainer

    def capture(*a, **kw):
        holder["tr"], models = build(*a, **kw)
        return holder["tr"], models

    def log(s):
        lines.append(s)
        seen.append(holder["tr"].last_norms)
    train.build_trainer = capture
    try:
        tr, n = train.main((argv or _train_argv(tmp, steps)) + list(extra), experiment=experiment, cfgs=TINY, log=log)
    finally:
        train.build_trainer = build
    assert n == steps and len(lines) == steps
    return [json.loads(s) for s in lines], tr, seen


def test_three_steps_of_the_driver_with_and_without_the_flag(dev, tmp_path):
    on, tr_on, seen = _drive(tmp_path / "on", ["--log_norms"])
    off, tr_off, seen_off = _drive(tmp_path / "off", [])
    # the reference's CLI trains the text encoder's LoRA by default (``--train_text_encoder``), so the driver holds two banks: the line names both
    assert tr_on.bank_keys == ["unet_lora", "TE_lora"]
    all_new = set(NEW_KEYS) | {"train_TE_lora_norm", "train_TE_lora_ema_norm", "grad_norm_TE_lora"}
    for rec in on:
        assert all(k in rec for k in NEW_KEYS) and not any(k.startswith(("train_prefix", "grad_norm_prefix")) for k in rec)
        assert all(isinstance(rec[k], float) and rec[k] > 0 for k in all_new), rec
    # the last line describes the banks the driver returns: the state after the last update, and the gradient that update saw
    for key, bank in zip(tr_on.bank_keys, tr_on.banks):
        last = seen[-1][key]
        _check("driver, last step, " + key, bank, last)
        assert (on[-1][f"train_{key}_norm"], on[-1][f"train_{key}_ema_norm"], on[-1][f"grad_norm_{key}"]) == (last["param_mean"], last["ema_mean"], last["grad_l2"])
    # step 1 runs at lr 0 (linear warm-up of one step): the ``up`` matrices are still the reference's zeros, and the mean counts them
    first = seen[0]["unet_lora"]["per_tensor"]
    ups, downs = [n for n in first if ".up." in n], [n for n in first if ".down." in n]
    assert on[0]["lr"] == 0.0 and len(ups) == len(downs) == len(first) // 2 > 0
    assert all(first[n][0] == 0.0 and first[n][1] == 0.0 for n in ups) and all(first[n][0] > 0 for n in downs)
    assert np.float32(on[0][NEW_KEYS[0]]) == np.float32(np.sum([np.float64(first[n][0]) for n in downs]) / len(first))
    # without the flag: none of the keys, the same records otherwise, and the same banks bit for bit
    assert seen_off == [None] * 3 and tr_off.banks[0]._norm_plan is None
    new = lambda r: {k for k in r if k.endswith("_norm") or k.startswith("grad_norm_")}
    assert all(new(r) == set() for r in off) and all(new(r) == all_new for r in on)
    strip = lambda r: {k: v for k, v in r.items() if k != "seconds" and k not in all_new}
    assert [strip(r) for r in on] == [strip(r) for r in off]
    assert len(tr_off.banks) == 2
    for x, y in zip(tr_on.banks, tr_off.banks):
        for name in STATE:
            assert torch.equal(getattr(x, name).view(torch.uint8), getattr(y, name).view(torch.uint8)), name


def test_exp2_line_carries_the_prefix_embedding_keys(dev, tmp_path):
    argv = ["--synthetic", "--train_num_tokens", "3", "--max_train_steps", "1", "--checkpointing_steps", "100", "--checkpointing_steps_long", "100",
            "--num_denoising_steps", "3", "--train_images_per_prompt_GPU", "4", "--train_GPU_batch_size", "3", "--val_GPU_batch_size", "4",
            "--learning_rate", "1e-4", "--output_dir", str(tmp_path / "run"), "--weight_loss_img", "0", "--weight_loss_face", "0"]
    recs, tr, seen = _drive(tmp_path, ["--log_norms"], experiment="exp-2", argv=argv, steps=1)
    assert tr.bank_keys == ["prefix_embedding"]
    keys = {k for k in recs[0] if k.endswith("_norm") or k.startswith("grad_norm_")}
    assert keys == {"train_prefix_embedding_norm", "train_prefix_embedding_ema_norm", "grad_norm_prefix_embedding"}
    rep = seen[0]["prefix_embedding"]
    assert recs[0]["train_prefix_embedding_norm"] == rep["param_mean"] > 0 and recs[0]["train_prefix_embedding_ema_norm"] == rep["ema_mean"] > 0
    _check("exp-2 prefix table", tr.banks[0], rep)
