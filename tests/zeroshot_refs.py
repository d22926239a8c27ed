"""The zero-shot classifier's references, shared by tests/test_zeroshot_gpu.py and tests/run_bf16_cosinehead_checks.py: the head restated in torch on the
oracle's CLIP image tower (``oracle.nn_vit``), the tiny configuration, the inputs, and the checks of their conditions, which need the oracle alone."""
import math
import os
import sys

import torch
import torch.nn.functional as F

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))

from finetune_fair_diffusion_amd import weights as W  # noqa: E402
from finetune_fair_diffusion_amd.factory import TINY  # noqa: E402

BAND_LOGITS, BAND_DCHIPS = 2e-2, 5e-2          # the bands tests/test_engine_gpu.py::test_vit_features_and_input_gradient_vs_oracle holds this tower to
BF16_FACTOR = 4.0                              # tests/run_bf16_checks.py: the bf16 bands of the end-to-end checks are 4x the fp16 ones (8e-2 for 2e-2, 2e-1 for 5e-2)
VISION_SEED = 9


def bf16_bands():
    return BAND_LOGITS * BF16_FACTOR, BAND_DCHIPS * BF16_FACTOR


def relerr(a, b):
    a, b = a.detach().float().cpu(), b.detach().float().cpu()
    return float((a - b).abs().max() / (b.abs().max() + 1e-20))


def check(name, a, b, tol):
    e = relerr(a, b)
    print(f"[{name}] rel max err {e:.3e} (tol {tol:.1e})  max|ref|={float(b.detach().abs().max()):.3e}")
    assert math.isfinite(e) and e <= tol, f"{name}: {e} > {tol}"


def vision_state():
    """Seeded weights of the tiny CLIP image tower, representable in fp16 (both sides load the same numbers)."""
    sd = W.synthetic_state_dict(W.vit_param_shapes(TINY["clip_vision"]), seed=VISION_SEED)
    return {k: (v.half().float() if v.is_floating_point() else v) for k, v in sd.items()}


class ZeroShotRef(torch.nn.Module):
    """The classifier restated: ``scale * normalize(tower(chips)) @ t_hat^T`` in fp32 torch, differentiable with respect to the chips."""

    def __init__(self, tower, t_hat, scale):
        super().__init__()
        self.tower, self.scale = tower, float(scale)
        self.register_buffer("t_hat", F.normalize(t_hat.float(), dim=-1))

    def forward(self, chips):
        from oracle import nn_vit as OV
        e = OV.image_features(self.tower, chips, W.CLIP_IMAGE_MEAN, W.CLIP_IMAGE_STD, normalize=False)
        return self.scale * F.normalize(e, dim=-1) @ self.t_hat.T


def oracle_tower(sd=None):
    from oracle import nn_vit as OV
    c = TINY["clip_vision"]
    cfg = OV.ViTConfig(kind="clip", image_size=c.image_size, hidden_size=c.hidden_size, num_hidden_layers=c.num_hidden_layers,
                       num_attention_heads=c.num_attention_heads, intermediate_size=c.intermediate_size, projection_dim=c.projection_dim, pos_grid=c.pos_grid)
    return OV.build(cfg, sd or vision_state())


def classifier_inputs():
    """(chips [3,3,56,56], t_hat [5, E], scale, d_logits [3,5]): two attributes of 2 and 3 classes; the class directions are the reference embeddings of
    the chips plus noise, so that the cosines are not all near zero (checked: max |cos| >= 0.3, with the oracle alone)."""
    g = torch.Generator().manual_seed(31)
    chips = (torch.rand(3, 3, 56, 56, generator=g) * 2 - 1).half().float()
    with torch.no_grad():
        e = F.normalize(ZeroShotRef(oracle_tower(), torch.eye(TINY["clip_vision"].projection_dim), 1.0)(chips), dim=-1)      # eye: the normalised embedding
    t = torch.stack([e[0], -e[0] + 0.5 * e[1], e[1], e[2], e[0] - e[2]]) + 0.6 * torch.randn(5, e.shape[1], generator=g) / math.sqrt(e.shape[1])
    return chips, F.normalize(t, dim=-1), 20.0, torch.randn(3, 5, generator=g)


def check_classifier(dev, tag, band_logits=BAND_LOGITS, band_dchips=BAND_DCHIPS):
    """``ZeroShotClipClassifier`` on the tiny tower against the restated head on the oracle tower: logits, and dL/dchips for L = sum(d_logits * logits)."""
    from finetune_fair_diffusion_amd.classifier import ZeroShotClipClassifier
    from finetune_fair_diffusion_amd.ops import F16
    from finetune_fair_diffusion_amd.vit import VisionTransformer
    chips, t_hat, scale, dl = classifier_inputs()
    ref_m = ZeroShotRef(oracle_tower(), t_hat, scale)
    x = chips.clone().requires_grad_(True)
    ref = ref_m(x)
    cos = ref.detach() / scale
    print(f"[{tag}] reference cosines: max |cos| {float(cos.abs().max()):.3f}, min |cos| {float(cos.abs().min()):.3f}")
    assert float(cos.abs().max()) >= 0.3, "the class directions are nearly orthogonal to every embedding: the comparison would show little"
    (ref * dl).sum().backward()
    clf = ZeroShotClipClassifier(VisionTransformer(TINY["clip_vision"], vision_state(), dev, W.CLIP_IMAGE_MEAN, W.CLIP_IMAGE_STD), t_hat, scale)
    assert clf.num_classes == 5 and clf._ctx is None
    got = clf.forward(chips.to(dev, F16), record=True)
    assert got.dtype == torch.float32 and tuple(got.shape) == (3, 5) and clf._ctx is not None and clf.tower._ctx is None
    check(f"{tag} zero-shot logits", got, ref, band_logits)
    dchips = clf.backward(dl.to(dev), 2.0 ** 10)
    assert clf._ctx is None and clf.tower._ctx is None and dchips.dtype == torch.float32 and tuple(dchips.shape) == tuple(chips.shape)
    check(f"{tag} zero-shot d chips", dchips, x.grad, band_dchips)
    return clf, chips, got, dchips


# ============================================================================= the full tiny training step
B, S, THRESHOLD = 4, 4, 0.7
# Prompts, noise seed and scale were chosen with the oracle alone (CPU) so that ``check_step_inputs`` holds: the hash tokenizer and the seeded text tower
# make every prompt a random direction, and most pairs rank the four faces of a prompt too closely for the forward band.
VARIANTS = {
    # exp-1-shaped: one binary attribute, the rank rule on the device tail
    "rank": dict(class_prompts="job=a photo of a nurse|a portrait of a teacher person", target_solver="rank", zero_shot_logit_scale=30.0, noise_seed=5991),
    # two attributes of 2 and 3 classes, Monte-Carlo transport targets on the host path
    "mc": dict(class_prompts="job=a photo of a nurse|a portrait of a teacher person;look=a portrait of a adult person|a photo of a queen|a portrait of a pilot person",
               target_solver="mc", zero_shot_logit_scale=30.0, noise_seed=5991),
}
OT_SEED = 4321


def step_args(variant, **kw):
    """The namespace of a tiny zero-shot custom run (``util_models.make_args`` plus the custom flags), 56-pixel chips."""
    import util_models as U
    v = {k: x for k, x in VARIANTS[variant].items() if k != "noise_seed"}
    d = dict(train_unet=True, train_text_encoder=False, uncertainty_threshold=THRESHOLD, size_face=TINY["clip_vision"].image_size, classifier="zero_shot",
             face_confidence_level=0.9, train_images_per_prompt_GPU=B, **v)
    d.update(kw)
    return U.make_args(**d)


def step_noises(variant, n=B):
    return torch.randn(n, 4, 32, 32, generator=torch.Generator().manual_seed(VARIANTS[variant]["noise_seed"]))


def text_statement(prompts):
    """Unit class directions [K, E] from the fp64 statement of ``text_embeds`` on the synthetic text tower (tests/textscore_cases.py): the reference the
    product's directions are held to."""
    import textscore_cases as TC
    from finetune_fair_diffusion_amd import evaluate_images as EI
    ids = EI.tokenize_prompts(prompts, TINY["clip_text_h"], synthetic=True)
    return F.normalize(TC.text_reference(EI, TINY, ids), dim=-1)


def build_trainer(dev, variant, sds, **kw):
    """The product's tiny trainer with the zero-shot classifier built by the factory's own constructor (synthetic text tower, hash tokenizer)."""
    import util_models as U
    from finetune_fair_diffusion_amd import factory
    from finetune_fair_diffusion_amd.fairness import experiment_spec
    from finetune_fair_diffusion_amd.step import FairnessTrainer
    args = step_args(variant, **kw)
    pm = U.product_models(sds, dev, train_unet=True, train_te=False)
    clf = factory.zero_shot_classifier(experiment_spec("custom", args), TINY, dict(clip_vision=vision_state()), dev)
    return FairnessTrainer(args, pm["text_encoder"], pm["unet"], pm["vae"], clf, pm["scheduler"], eval_text_encoder=pm["eval_text_encoder"],
                           eval_unet=pm["eval_unet"], experiment="custom", device=dev)


def oracle_logits(om, clf_ref, tokens, noises):
    """The oracle's own R1 images and the restated classifier's logits on their face chips (CPU, no gradient)."""
    from oracle import fair_step as fs
    with torch.no_grad():
        img = fs.generate_image_no_gradient(tokens, noises, S, om["text_encoder"], om["unet"], om["vae"], om["scheduler"])
        ind, _, chips = fs.SyntheticFaceProvider(TINY["clip_vision"].image_size)(img)
        assert bool(ind.all())
        return img, clf_ref(chips)


def rank_targets(logits):
    from oracle import fair_step as fs
    t, u = fs.generate_dynamic_targets(torch.softmax(logits[:, 0:2], dim=-1), w_uncertainty=True)
    t = t.clone()
    t[u > THRESHOLD] = -1
    return t


def mc_targets(logits, attrs, cdfs):
    from oracle import fair_step as fs
    probs = [torch.softmax(logits[:, c0:c0 + k], dim=-1) for _, c0, k in attrs]
    res, _ = fs.generate_dynamic_targets_multi(probs, cdfs, 100, torch.Generator().manual_seed(OT_SEED), False)
    out = {}
    for (name, _, _), (t, u) in zip(attrs, res):
        t = t.clone()
        t[u > THRESHOLD] = -1
        out[name] = t
    return out


def check_step_inputs(variant, logits, attrs, cdfs=None, trials=16):
    """The condition on the inputs, with the oracle alone: moving every reference logit by the forward band (``BAND_LOGITS`` of max |logit|, each sign
    pattern of ``trials`` seeded draws, and all up / all down per column) changes no target and no confidence mask; for the rank rule also in its closed
    form -- the sorted differences l1 - l0 lie more than four bands apart (each difference moves by at most two)."""
    band = BAND_LOGITS * float(logits.abs().max())
    g = torch.Generator().manual_seed(99)
    signs = [torch.where(torch.rand(logits.shape, generator=g) < 0.5, -1.0, 1.0) for _ in range(trials)]
    for c in range(logits.shape[1]):
        for s in (-1.0, 1.0):
            m = torch.zeros_like(logits)
            m[:, c] = s
            signs.append(m)
    if variant == "rank":
        base = rank_targets(logits)
        d = (logits[:, 1] - logits[:, 0]).sort().values
        gap = float((d[1:] - d[:-1]).min())
        print(f"[{variant}] band {band:.4f}, smallest gap of the sorted l1 - l0 {gap:.4f} ({gap / band:.1f} bands), targets {base.tolist()}")
        assert gap > 4 * band, "two faces rank too close together for the forward band"
        assert all(torch.equal(rank_targets(logits + band * s), base) for s in signs)
        assert int((base != -1).sum()) >= 2
        return base
    base = mc_targets(logits, attrs, cdfs)
    for s in signs:
        moved = mc_targets(logits + band * s, attrs, cdfs)
        assert all(torch.equal(moved[n], base[n]) for n in base), "a target or a confidence mask moves inside the forward band"
    print(f"[{variant}] band {band:.4f}, targets {({n: t.tolist() for n, t in base.items()})}")
    assert sum(int((t != -1).sum()) for t in base.values()) >= 3
    return base
