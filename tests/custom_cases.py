"""Shared cases of the ``--experiment custom`` GPU tests (tests/test_custom_targets_gpu.py, the bf16 runner and the two-rank runner): tiny trainers
built twice from the same seeded weights -- once under a named experiment, once under the custom flags that restate it -- and what is compared."""
import contextlib
import os
import sys

import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import util_models as U  # noqa: E402

RESTATED = {          # named experiment -> the custom flags that restate it
    "exp-1": dict(num_classifier_logits=80, attributes="gender:40:2", target_solver="rank"),
    "exp-3": dict(num_classifier_logits=6, attributes="gender:0:2,race:2:4", target_solver="mc"),
    "exp-4": dict(num_classifier_logits=8, attributes="gender:0:2,race:2:4,age:6:2", target_distribution="age=0.75,0.25", asymmetric_last_attribute=True),
    "exp-6": dict(num_classifier_logits=6, attributes="race:2:4", target_solver="enumerate"),
}
B, S, STEPS, THRESHOLD = 4, 2, 2, 0.7
_SDS = {}


def build(dev, experiment="exp-1", custom=None, rank=0, world=1, batch=B, **kw):
    """A tiny trainer (LoRA on the U-Net) of ``experiment``, or of ``custom`` (the flags of ``--experiment custom``) when given."""
    from finetune_fair_diffusion_amd.fairness import experiment_spec
    from finetune_fair_diffusion_amd.step import FairnessTrainer
    args = U.make_args(train_unet=True, train_text_encoder=False, uncertainty_threshold=THRESHOLD, train_GPU_batch_size=batch,
                       train_images_per_prompt_GPU=batch, learning_rate=2e-3, **(custom or {}), **kw)
    name = "custom" if custom is not None else experiment
    ncls = experiment_spec(name, args).num_logits
    if ncls not in _SDS:
        _SDS[ncls] = U.synthetic_sds(train_unet=True, train_te=False, lora_up_std=0.05, num_classes=ncls)
    pm = U.product_models(_SDS[ncls], dev, train_unet=True, train_te=False, num_classes=ncls)
    return FairnessTrainer(args, pm["text_encoder"], pm["unet"], pm["vae"], pm["classifier"], pm["scheduler"], eval_text_encoder=pm["eval_text_encoder"],
                           eval_unet=pm["eval_unet"], experiment=name, rank=rank, world_size=world, device=dev)


def noises(step, n=B, lat=32):
    return torch.randn(n, 4, lat, lat, generator=torch.Generator().manual_seed(4242 + step))


def snapshot(tr, out):
    """Everything the restatement tests hold equal: images, probabilities, targets, uncertainties, per-image losses, every bank's flat gradient and
    the banks after the update."""
    snap = {k: out[k].detach().cpu().clone() for k in ("images", "probs", "preds", "probs_ori", "targets", "uncertainty", "loss_fair")}
    for k in ("targets_by_attr", "loss_fair_by_attr"):
        snap.update({f"{k}/{n}": v.detach().cpu().clone() for n, v in out[k].items()})
    for i, b in enumerate(tr.banks):
        snap.update({f"grad{i}": b.grad.detach().cpu().clone(), f"flat{i}": b.flat.detach().cpu().clone(), f"ema{i}": b.ema.detach().cpu().clone()})
    snap["finite"] = torch.tensor(bool(out["grad_is_finite"]))
    return snap


def run_steps(tr, steps=STEPS):
    snaps = []
    for i in range(steps):
        out = tr.train_step(U.tiny_tokens(), noises(i), S)
        torch.cuda.synchronize()
        snaps.append(snapshot(tr, out))
    return snaps


def check_restatement(dev, named):
    """Two steps under the named experiment and two under its restatement: every snapshot entry equal by ``torch.equal``.  Returns the snapshots of
    the custom run and both trainers."""
    tr_n, tr_c = build(dev, named), build(dev, custom=RESTATED[named])
    assert tr_c.experiment == "custom" and tr_c.spec.custom and not tr_n.spec.custom
    assert (tr_c.device_tail, tr_c.enumerated_targets, tr_c.attrs, tr_c.class_cdfs, tr_c.age_asym) == \
        (tr_n.device_tail, tr_n.enumerated_targets, tr_n.attrs, tr_n.class_cdfs, tr_n.age_asym)
    a, b = run_steps(tr_n), run_steps(tr_c)
    for step, (x, y) in enumerate(zip(a, b)):
        assert set(x) == set(y)
        for k in x:
            assert x[k].dtype == y[k].dtype and torch.equal(x[k], y[k]), (named, step, k)
    last = b[-1]
    assert bool(last["finite"]) and float(last["grad0"].abs().max()) > 0 and not torch.equal(b[0]["flat0"], b[1]["flat0"])      # the steps did train
    assert any(int((v != -1).sum()) > 0 for k, v in last.items() if k.startswith("targets_by_attr/")), "no target survived the threshold"
    return b, tr_n, tr_c


BINARY_75_25 = dict(num_classifier_logits=80, attributes="gender:40:2", target_distribution="gender=0.75,0.25")


def check_non_uniform_binary(dev):
    """``gender=0.75,0.25`` on the device tail: the targets and uncertainties the step used are the host statement's on the probabilities the step
    reports.  Returns (trainer, the step's report)."""
    from finetune_fair_diffusion_amd.fairness import generate_dynamic_targets
    tr = build(dev, custom=BINARY_75_25, batch=8)
    assert tr.device_tail and tr.spec.solver == "rank" and tr.target_ratio == 0.75
    out = tr.train_step(U.tiny_tokens(), noises(0, 8), S)
    torch.cuda.synchronize()
    t, u = generate_dynamic_targets(out["probs"], target_ratio=0.75, w_uncertainty=True)
    assert sorted(t.tolist()) == [0] * 6 + [1] * 2          # every synthetic image has a face: six of eight towards class 0
    t = t.clone()
    t[u > THRESHOLD] = -1
    assert torch.equal(out["targets"], t), (out["targets"], t)
    assert out["uncertainty"].dtype == torch.float32 and torch.equal(out["uncertainty"], u.to(torch.float32))
    assert int((t != -1).sum()) >= 2 and bool(out["grad_is_finite"])
    return tr, out


@contextlib.contextmanager
def count_device_reads():
    """Counts the Python-level device -> host reads (``.cpu()``, ``.item()``, ``.tolist()``, ``.numpy()`` of a device tensor) made inside the block."""
    n = [0]
    saved = {name: getattr(torch.Tensor, name) for name in ("cpu", "item", "tolist", "numpy")}

    def wrap(fn):
        def inner(self, *a, **kw):
            if self.is_cuda:
                n[0] += 1
            return fn(self, *a, **kw)
        return inner
    own = {name for name in saved if name in torch.Tensor.__dict__}
    try:
        for name, fn in saved.items():
            setattr(torch.Tensor, name, wrap(fn))
        yield n
    finally:
        for name, fn in saved.items():
            if name in own:
                setattr(torch.Tensor, name, fn)
            else:
                delattr(torch.Tensor, name)          # inherited from the base class again
