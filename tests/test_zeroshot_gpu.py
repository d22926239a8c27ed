"""``--experiment custom --classifier zero_shot`` on the MI355X with the tiny models: the classifier against the oracle's CLIP tower with the head restated
in torch (tests/zeroshot_refs.py), the full tiny training step against the oracle's ``fairness_step`` / ``fairness_step_multi`` with that restated module
as the oracle's classifier, run-to-run bits, resume, and the driver with validation."""
import json
import os
import sys

import pytest
import torch
import torch.nn.functional as F

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import custom_cases as CC  # noqa: E402
import textscore_cases as TC  # noqa: E402
import util_models as U  # noqa: E402
import zeroshot_refs as Z  # noqa: E402
from test_engine_gpu import _per_tensor_sign_guard, check  # noqa: E402
from finetune_fair_diffusion_amd import weights as W  # noqa: E402
from finetune_fair_diffusion_amd.factory import TINY  # noqa: E402

pytestmark = pytest.mark.gpu


# ------------------------------------------------------------------------------------------ the classifier
def test_zero_shot_classifier_against_the_oracle_tower(dev):
    """Logits within 2e-2 of max|ref|, d chips within 5e-2 (the bands of this tower: the head is fp32 and adds no 16-bit rounding); the non-recording
    forward gives the recording one's bits; a second tower on the same weight tensors (the regulariser's) keeps its recorded forward to itself."""
    from finetune_fair_diffusion_amd.classifier import ZeroShotClipClassifier
    from finetune_fair_diffusion_amd.ops import F16
    from finetune_fair_diffusion_amd.vit import VisionTransformer
    clf0, chips, logits, dchips = Z.check_classifier(dev, "fp16 library")
    x = chips.to(dev, F16)
    a = clf0.forward(x, record=False)
    assert clf0._ctx is None and clf0.tower._ctx is None
    b = clf0.forward(x, record=True)
    assert torch.equal(a, b) and torch.equal(a, logits), "record=False and record=True must be one kernel sequence"
    clf0._ctx = None                                                            # what the step does when it drops a recorded forward
    # the regulariser's tower and a classifier on ITS weight tensors
    _, t_hat, scale, dl = Z.classifier_inputs()
    reg = VisionTransformer(TINY["clip_vision"], Z.vision_state(), dev, W.CLIP_IMAGE_MEAN, W.CLIP_IMAGE_STD)
    clf = ZeroShotClipClassifier(VisionTransformer.sharing(reg), t_hat, scale)
    assert clf.tower is not reg and clf.tower.layers is reg.layers and clf.tower.patch.w.data_ptr() == reg.patch.w.data_ptr()
    other = (torch.rand(2, 3, 56, 56, generator=torch.Generator().manual_seed(8)) * 2 - 1).to(dev, F16)
    got = clf.forward(x, record=True)
    assert torch.equal(got, logits)
    e_reg = reg.forward(other, record=True)                                     # the regulariser records a forward of its own in between ...
    clf.forward(other, record=False)                                            # ... and the frozen side's images are classified without a record
    assert reg._ctx is not None and reg._ctx["N"] == 2 and clf._ctx["tower"]["N"] == 3
    d2 = clf.backward(dl.to(dev), 2.0 ** 10)
    assert torch.equal(d2, dchips), "another tower's forward between the classifier's forward and backward changed its gradient"
    assert reg._ctx is not None and reg._ctx["N"] == 2
    d_reg = reg.backward(torch.ones_like(e_reg), 2.0 ** 10)                     # the regulariser's record is still its own
    assert tuple(d_reg.shape) == (2, 3, 56, 56) and bool(torch.isfinite(d_reg).all()) and reg._ctx is None


# ------------------------------------------------------------------------------------------ the full tiny step
def _spy(tr, grads, apply=True):
    inner = tr.sync_and_update

    def spy(N_backward, apply_=True):
        for i, b in enumerate(tr.banks):
            grads[i] = b.grad.clone()
        return inner(N_backward) if apply else True
    tr.sync_and_update = spy


@pytest.mark.parametrize("variant", ["rank", "mc"])
def test_full_tiny_step_against_the_oracle(dev, variant):
    """B = 4, S = 4.  The oracle's classifier is the restated zero-shot module on the oracle tower, with the class directions the product derived (held to
    the fp64 statement of ``text_embeds`` first).  Input condition (oracle alone): no target and no confidence mask moves inside the forward band.
    Then: targets exactly equal; images, probabilities, per-image losses and the LoRA gradient inside the bands of tests/test_engine_gpu.py's tiny
    full-step tests (``test_full_fairness_step`` for the rank rule, ``test_full_step_multi_attribute_with_oracle_ot_targets`` for the transport targets)."""
    from oracle import fair_step as fs
    om = U.oracle_models(train_unet=True, train_te=False, lora_up_std=0.05)
    tr = Z.build_trainer(dev, variant, om["sds"])
    spec = tr.spec
    assert spec.zero_shot and tr.clf.num_classes == spec.num_logits == len(spec.prompts) and tr.device_tail == (variant == "rank")
    check(f"{variant} class directions vs the fp64 text statement", tr.clf.t_hat, Z.text_statement(spec.prompts), TC.BAND_EMBEDS)
    ref_clf = Z.ZeroShotRef(Z.oracle_tower(), tr.clf.t_hat.cpu(), tr.clf.logit_scale)
    tokens, noises = U.tiny_tokens(), Z.step_noises(variant)
    img_o, lg_o = Z.oracle_logits(om, ref_clf, tokens, noises)
    base = Z.check_step_inputs(variant, lg_o, spec.attrs, spec.class_cdfs)
    tr.target_rng.manual_seed(Z.OT_SEED)
    grads = {}
    _spy(tr, grads)
    out = tr.train_step(tokens, noises, Z.S)
    check(f"{variant} R1 images", out["images"], img_o, 3e-2)
    models_o = dict(text_encoder=om["text_encoder"], unet=om["unet"], vae=om["vae"], classifier=ref_clf, scheduler=om["scheduler"],
                    eval_text_encoder=om["text_encoder"], eval_unet=om["eval_unet"])
    for p in om["lora_params"]:
        p.grad = None
    side = TINY["clip_vision"].image_size
    names = list(om["unet_lora_layers"].state_dict().keys())
    params = list(om["unet_lora_layers"].parameters())
    if variant == "rank":
        ref = fs.fairness_step(models_o, tokens, noises, Z.S, dict(train_GPU_batch_size=3, val_GPU_batch_size=8, uncertainty_threshold=Z.THRESHOLD, factor2=0.2,
                                                                  size_face=side, slice_fn=lambda lg: lg[:, 0:2]))
        assert ref["targets"].tolist() == base.tolist()
        check("rank probs", out["probs"], ref["probs"], 2e-2)
        assert out["targets"].tolist() == ref["targets"].tolist(), (out["targets"], ref["targets"])
        check("rank loss_fair", out["loss_fair"], ref["loss_fair"], 1e-2)
        assert out["N_backward"] == ref["N_backward"] and out["grad_is_finite"]
    else:
        tg = out["targets_by_attr"]
        assert list(tg) == [a[0] for a in spec.attrs]
        for name in tg:
            assert tg[name].tolist() == base[name].tolist(), (name, tg[name], base[name])
        ref = fs.fairness_step_multi(models_o, tokens, noises, Z.S, dict(train_GPU_batch_size=3, size_face=side), spec.attrs, base)
        for name, _, _ in spec.attrs:
            check(f"mc loss_fair_{name}", out["loss_fair_by_attr"][name], ref["losses"][name], 2e-2)
        assert out["grad_is_finite"]
    refg = torch.cat([p.grad.flatten() for p in params])
    got = torch.cat([tr.banks[0].view(n, grads[0]).flatten() for n in names])
    cos = float(F.cosine_similarity(got.cpu().double(), refg.double(), dim=0))
    ratio = float(got.norm().cpu() / refg.norm())
    print(f"cosine({variant} unet grads) = {cos}  norm ratio = {ratio}")
    if variant == "rank":
        check("rank step: unet LoRA grad (all tensors)", got, refg, 3e-1)
        assert cos > 0.97
        _per_tensor_sign_guard("unet LoRA", names, tr.banks[0], grads[0], [p.grad for p in params])
    else:
        assert cos > 0.97 and 0.8 < ratio < 1.25


def test_two_runs_give_the_bit_equal_lora_gradient(dev):
    sds = U.synthetic_sds(train_unet=True, train_te=False, lora_up_std=0.05)
    flat = []
    for _ in range(2):
        tr = Z.build_trainer(dev, "rank", sds)
        grads = {}
        _spy(tr, grads)
        out = tr.train_step(U.tiny_tokens(), Z.step_noises("rank"), Z.S)
        torch.cuda.synchronize()
        assert out["grad_is_finite"] and float(grads[0].abs().max()) > 0
        flat.append((grads[0].cpu(), out["probs"].clone(), out["loss_fair"].clone()))
    assert all(torch.equal(a, b) for a, b in zip(*flat)), "two runs of one step differ"


def test_checkpoint_resumes_and_refuses_other_prompts(dev, tmp_path):
    from finetune_fair_diffusion_amd import checkpoint as ck
    sds = U.synthetic_sds(train_unet=True, train_te=False, lora_up_std=0.05)
    a = Z.build_trainer(dev, "mc", sds)
    a.train_step(U.tiny_tokens(), CC.noises(0), 2)
    path = ck.save_state(a, str(tmp_path / "checkpoint-1"), 1)
    st = torch.load(os.path.join(path, "trainer_state.pth"), map_location="cpu", weights_only=False)
    assert st["spec"] == a.spec.state() and st["spec"]["classifier"] == "zero_shot" and st["spec"]["class_prompts"][0][0] == "job"
    want = CC.snapshot(a, a.train_step(U.tiny_tokens(), CC.noises(1), 2))
    b = Z.build_trainer(dev, "mc", sds)
    assert ck.load_state(b, path) == 1
    got = CC.snapshot(b, b.train_step(U.tiny_tokens(), CC.noises(1), 2))
    for k in want:
        assert torch.equal(want[k], got[k]), k
    other = Z.VARIANTS["mc"]["class_prompts"].replace("a photo of a queen", "a photo of a king")
    c = Z.build_trainer(dev, "mc", sds, class_prompts=other)
    held = [bk.flat.clone() for bk in c.banks]
    with pytest.raises(ValueError, match="trains towards"):
        ck.load_state(c, path)
    assert all(torch.equal(bk.flat, h) for bk, h in zip(c.banks, held))
    d = Z.build_trainer(dev, "mc", sds, zero_shot_logit_scale=31.0)         # another scale is another classifier
    with pytest.raises(ValueError, match="trains towards"):
        ck.load_state(d, path)


def test_train_driver_zero_shot_with_validation_and_the_shared_tower(dev, tmp_path, monkeypatch):
    """The driver end to end with synthetic weights: the factory builds the classifier on the regulariser's weight tensors, the steps train, and
    ``--validation metrics`` reports ``<name>_gap_to_target`` for the prompted attributes.  Without ``--synthetic`` the run needs FD_CLIP_VISION_DIR even
    with the image term off, and says so before anything is loaded."""
    from finetune_fair_diffusion_amd import train
    logs = []
    argv = ["--experiment", "custom", "--synthetic", "--classifier", "zero_shot", "--class_prompts", Z.VARIANTS["mc"]["class_prompts"], "--size_face", "56",
            "--img_size_small", "56", "--validation", "metrics", "--train_monitor", "metrics", "--train_unet", "--rank", "4", "--max_train_steps", "2",
            "--checkpointing_steps", "100", "--checkpointing_steps_long", "100", "--num_denoising_steps", "2", "--train_images_per_prompt_GPU", "4",
            "--train_GPU_batch_size", "3", "--val_GPU_batch_size", "4", "--val_images_per_prompt_GPU", "4", "--evaluate_every_n_iter", "100",
            "--weight_loss_img", "1", "--weight_loss_face", "0", "--uncertainty_threshold", "0.9", "--lora_up_std", "0.05", "--output_dir", str(tmp_path)]
    tr, n = train.main(argv, cfgs=TINY, log=logs.append)
    recs = [json.loads(x) for x in logs]
    assert n == 2 and tr.spec.zero_shot and tr.clf.num_classes == 5 and tr.spec.attrs == [("job", 0, 2), ("look", 2, 3)] and tr.clf.logit_scale == 100.0
    assert tr.use_img_loss and tr.clf.tower is not tr.clip and tr.clf.tower.layers is tr.clip.layers and tr.clf._ctx is None and tr.clip._ctx is None
    evals, steps = [r for r in recs if "eval" in r], [r for r in recs if "eval" not in r]
    assert [r["eval"] for r in evals] == ["main", "EMA"]
    assert all({"job_gap_to_target", "look_gap_to_target", "joint_gap_to_target"} <= set(r["mean"]) for r in evals)
    assert len(steps) == 2 and all(r["grad_is_finite"] and "train_look_gap_to_target" in r and r["loss_CLIP"] is not None for r in steps)
    monkeypatch.delenv("FD_CLIP_VISION_DIR", raising=False)
    real = [a for a in argv if a != "--synthetic"] + ["--pretrained_model_name_or_path", str(tmp_path)]
    real[real.index("--weight_loss_img") + 1] = "0"
    with pytest.raises(FileNotFoundError, match="FD_CLIP_VISION_DIR"):
        train.main(real, cfgs=TINY, log=logs.append)
