"""Command-line / YAML surface of the reference's ``1-main-debias.py`` (``parse_args``,
exp-1-debias-gender/1-main-debias.py:327-644): the same 50 flags with the same defaults and the same
YAML-overlay rule -- ``args[key] = type(args[key])(value)`` (:632-638), so keys whose default is None
cannot be set from YAML and booleans follow Python's ``bool(value)`` -- plus the build's own additions
(prefixed below), which the reference does not have:

  --num_denoising_steps  fixed S instead of ``random.choices(range(19,24))`` (:1779)
  --synthetic            synthetic weights / token ids / face provider (no network, no data.zip)
  --face_provider        detector seam: "synthetic" (default) or "detector" (insightface + face_recognition, when installed)
  --num_classifier_logits  80 (exp-1) / 6 (exp-3,5,6) / 8 (exp-4)
  --lora_up_std          std of the LoRA ``up`` init; 0 (default) = zeros like the reference, non-zero only for synthetic experiments
  --validation           off (default) / metrics / grids: the reference's ``evaluation_step`` at step 0 and every ``--evaluate_every_n_iter`` steps
                         (evaluation.py); "off" leaves the run -- JSON lines, random streams, checkpoints -- exactly as without the flag;
                         grids_attrs: as grids, with one strip per attribute in the grids of exp-3/4/5 (the reference's own validation grids)
  --train_monitor        off (default) / metrics / plots: what the reference's loop logs about every training batch.  metrics: the step's JSON line
                         gains ``train_<gap metric>`` of the gathered batch, ``num_faces`` and ``num_faces_total``; plots: also, every
                         ``--train_plot_every_n_iter`` steps of an epoch, ``<output_dir>/imgs/train-{global_step}_{generated|ori}.jpg``.  "off"
                         leaves the run exactly as without the flag; no mode draws a random number or changes a result of the step
  --index_font           PATH of a TrueType font file, or "default" for Pillow's embedded scalable font: the validation grids and the train plots
                         print each image's index (in the gathered batch) on its tile, as the reference does with Arial Bold (``plot_in_grid``
                         :199-200) -- the number pairs a tile of the ``_ori`` grid with its tile of the ``_generated`` grid.  Not given (default):
                         no index text, the grids as before.  ``--index_font_size`` (default 100, the reference's) is the point size
  --log_norms            the reference's per-step parameter norms (:2034-2045; exp-2 :2126-2130) in the step's JSON line, for the banks being trained:
                         ``train_unet_lora_norm`` / ``train_TE_lora_norm`` / ``train_prefix_embedding_norm`` (the mean of the per-tensor L2 norms)
                         and their ``_ema_norm`` twins, after the step's update, plus ``grad_norm_<bank>``: the global L2 norm of the all-reduced,
                         averaged gradient the optimiser saw (null when it is not finite).  One device-side reduction per bank and step, read back
                         asynchronously; off (default): nothing is launched and the line is unchanged

``--experiment custom`` (build addition; no script of the reference: its targets are written into each script's code) keeps exp-1's flags and trains
towards a target distribution given on the command line or in the YAML; ``fairness.experiment_spec`` resolves and checks them once, and every
malformed value is refused here with a ValueError that names the flag, before anything is loaded:

  --num_classifier_logits  required: the logit count of the classifier head behind ``--classifier_weight_path``
  --attributes           "gender:0:2,race:2:4" -- name : first logit column : classes; 1..3 attributes of 2..4 classes each, unique names matching
                         ``[a-z][a-z0-9_]*``, column ranges disjoint and inside the head
  --target_distribution  "gender=0.5,0.5;race=0.4,0.2,0.2,0.2" -- per named attribute its k non-negative class probabilities, summing to 1 within
                         1e-6; an attribute that is not named gets the uniform target
  --target_solver        rank (one two-class attribute: the binomial rank rule with ``target_ratio = p[0]`` on the device tail, exp-1's),
                         mc (Monte-Carlo transport plans whose class draws follow the target, exp-3/4/5's) or enumerate (one attribute: the exact
                         expectation over the class compositions weighted by their multinomial probability, exp-6's); not given: rank for one
                         two-class attribute, mc otherwise
  --factor1 / --factor2  one float for every attribute, or a comma list with one float per attribute
  --face_confidence_level  one float (the named experiments' ``face_*_confidence_level``)
  --asymmetric_last_attribute  exp-4's cost asymmetry for the last attribute's second class (exp-4 :1551-1556); it exists so that exp-4 can be restated
  --classifier           mobilenet (default: the trained head behind ``--classifier_weight_path``) or zero_shot: the CLIP ViT-H/14 image tower of
                         ``FD_CLIP_VISION_DIR`` against one text prompt per class, logit = logit_scale * cos(image embedding, prompt embedding)
                         (classifier.ZeroShotClipClassifier) -- no trained head, ``--classifier_weight_path`` is not read; ``--size_face`` must be the
                         tower's input size (224)
  --class_prompts        "gender=a photo of a man|a photo of a woman;age=a photo of a young person|a photo of an old person" -- zero_shot's head:
                         attributes separated by ``;``, class prompts by ``|`` (prompts contain commas); 1..3 attributes of 2..4 prompts.  The logit
                         columns follow the prompts, so ``--attributes`` and ``--num_classifier_logits`` are derived (refused if given and different)
  --zero_shot_logit_scale  zero_shot's logit scale; 0 (default) = ``exp(logit_scale)`` of the CLIP checkpoint (100 when it stores none)

``--validation`` and ``--train_monitor`` report, per attribute, ``<name>{k}_freq``, ``<name>_pred_below_0.8`` and ``<name>_gap_to_target`` (half the
L1 distance between the class frequencies and the target) and, with two or more attributes, ``joint_gap_to_target`` over the cells.

The multi-attribute experiments change a few flags and defaults (exp-3-debias-gender-race/1-main-debias.py:343-660,
exp-4-debias-gender-race-age/...:343-672, exp-5-...:343-690; exp-2-debias-gender-token/...:453-780 drops the two LoRA switches and adds
``--train_num_tokens``): ``factor{1,2}`` split per attribute,
``face_gender[_race[_age]]_confidence_level``, bigger batches, three more prompt files in exp-5 -- ``EXPERIMENT_CLI``.  exp-6
(exp-6-debias-race/1-main-debias.py:337-644) keeps exp-1's flags with other defaults and ``face_race_confidence_level``.

Pinned by tests/golden/reference_cli.json, reference_cli_multi.json and reference_cli_exp6.json (defaults and every YAML overlay of
exp-1/2/3/4/5/6, produced by running the reference's own parse_args).
"""
import argparse
import os

import yaml


_FF = "../data/2-trained-classifiers/fairface_MobileNetLarge_"
_MULTI = dict(max_train_steps=15000, weight_loss_face=0.1, uncertainty_threshold=0.4, val_images_per_prompt_GPU=24,
              face_feats_path="../data/3-face-features/FairFace_MobileNetLarge_GenderRace4_09041634/face_feats.pkl")
_GR = dict(factor1_gender=0.2, factor1_race=0.6, factor2_gender=0.2, factor2_race=0.3)
# experiment -> (changed defaults, removed flags, added float flags, added str flags)
EXPERIMENT_CLI = {
    "exp-1": ({}, [], {}, {}),
    # exp-2 (prefix-token tuning, exp-2-debias-gender-token/1-main-debias.py:453-780): no LoRA switches, one int flag (below)
    "exp-2": ({}, ["train_text_encoder", "train_unet"], {}, {}),
    "exp-3": (dict(_MULTI, train_images_per_prompt_GPU=16, classifier_weight_path=_FF + "GenderRace4_09041216/epoch=9-step=3380_MobileNetLarge.pt"),
              ["factor1", "factor2", "face_gender_confidence_level"], dict(_GR, face_gender_race_confidence_level=0.8), {}),
    "exp-4": (dict(_MULTI, train_images_per_prompt_GPU=20, classifier_weight_path=_FF + "GenderRace4Age2_09151907/epoch=9-step=3380_MobileNetLarge.pt"),
              ["factor1", "factor2", "face_gender_confidence_level"],
              dict(_GR, factor1_age=0.6, factor2_age=0.3, face_gender_race_age_confidence_level=0.75), {}),
    "exp-5": (dict(_MULTI, train_images_per_prompt_GPU=16, classifier_weight_path=_FF + "GenderRace4_09041216/epoch=9-step=3380_MobileNetLarge.pt"),
              ["factor1", "factor2", "face_gender_confidence_level"], dict(_GR, face_gender_race_confidence_level=0.8),
              dict(prompt_occupation_w_style_and_context_path="../data/1-prompts/occupation_w_style_and_context.json",
                   prompt_personal_descroptor_path="../data/1-prompts/personal_descriptor.json",   # (sic) the reference's spelling
                   prompt_sports_path="../data/1-prompts/sports.json")),
    # exp-6 (race alone, exp-6-debias-race/1-main-debias.py:337-644): exp-1's flags on the GenderRace4 classifier, race confidence level
    "exp-6": (dict(max_train_steps=12000, weight_loss_img=6, weight_loss_face=0.1, factor1=0.6, factor2=0.3, train_images_per_prompt_GPU=16,
                   val_images_per_prompt_GPU=16, classifier_weight_path=_FF + "GenderRace4_09041216/epoch=9-step=3380_MobileNetLarge.pt",
                   face_feats_path=_MULTI["face_feats_path"]),
              ["face_gender_confidence_level"], dict(face_race_confidence_level=0.9), {}),
    # custom (build addition): exp-1's flags, one confidence level for whatever the attributes are, the target specification as strings.
    # factor1 / factor2 hold one float or a comma list, so they are strings here; num_classifier_logits has no default to fall back on (0 = not given)
    # classifier / class_prompts / zero_shot_logit_scale: the zero-shot CLIP head (strings and a float, so the YAML overlay sets them)
    "custom": (dict(factor1="0.2", factor2="0.2"), ["face_gender_confidence_level"], dict(face_confidence_level=0.9, zero_shot_logit_scale=0.0),
               dict(attributes="", target_distribution="", target_solver="", classifier="mobilenet", class_prompts="")),
}
CUSTOM_STR_FLAGS = ("factor1", "factor2")


def build_parser(experiment="exp-1"):
    p = argparse.ArgumentParser(description="Script to finetune Stable Diffusion for debiasing purposes.")
    changed, removed, add_f, add_s = EXPERIMENT_CLI[experiment]

    def a(flag, **kw):
        name = flag.lstrip("-")
        if name in removed:
            return
        if name in changed:
            kw["default"] = changed[name]
        if experiment == "custom" and name in CUSTOM_STR_FLAGS:
            kw["type"] = str
        p.add_argument(flag, **kw)
    for k, v in add_f.items():
        p.add_argument("--" + k, type=float, default=v)
    for k, v in add_s.items():
        p.add_argument("--" + k, type=str, default=v)
    if experiment == "custom":
        p.add_argument("--num_classifier_logits", type=int, default=0)
        p.add_argument("--asymmetric_last_attribute", action="store_true", default=False)
    if experiment == "exp-2":
        p.add_argument("--train_num_tokens", type=int, default=5)       # number of tokens to finetune as prompt prefix (:479-484)
    # 1. experiment setting
    a("--proj_name", default="debias-SD", type=str)
    a("--pretrained_model_name_or_path", type=str, default="runwayml/stable-diffusion-v1-5")
    a("--train_text_encoder", action="store_true", default=True)
    a("--train_unet", action="store_true", default=False)
    a("--seed", type=int, default=5991)
    a("--max_train_steps", type=int, default=10000)
    a("--checkpointing_steps", type=int, default=20)
    a("--checkpoints_total_limit", type=int, default=2)
    a("--checkpointing_steps_long", type=int, default=200)
    a("--resume_from_checkpoint", type=str, default=None)
    a("--mixed_precision", type=str, default="fp16", choices=["no", "fp16", "bf16"])
    a("--rank", type=int, default=50)
    a("--train_plot_every_n_iter", type=int, default=20)
    a("--evaluate_every_n_iter", type=int, default=200)
    a("--guidance_scale", type=float, default=7.5)
    a("--EMA_decay", type=float, default=0.996)
    # 2. loss weights
    a("--weight_loss_img", type=float, default=8)
    a("--weight_loss_face", type=float, default=1)
    a("--uncertainty_threshold", type=float, default=0.2)
    a("--factor1", type=float, default=0.2)
    a("--factor2", type=float, default=0.2)
    # 3. batch sizes
    a("--train_images_per_prompt_GPU", type=int, default=8)
    a("--train_GPU_batch_size", type=int, default=4)
    a("--val_images_per_prompt_GPU", type=int, default=8)
    a("--val_GPU_batch_size", type=int, default=8)
    # 4. data / external files
    a("--prompt_occupation_path", type=str, default="../data/1-prompts/occupation.json")
    a("--classifier_weight_path", type=str, default="../data/2-trained-classifiers/CelebA_MobileNetLarge_08060852/epoch=9-step=12660_MobileNetLarge.pt")
    a("--face_feats_path", type=str, default="../data/3-face-features/CelebA_MobileNetLarge_08240859/face_feats.pkl")
    a("--opensphere_config", type=str, default="../data/4-opensphere_checkpoints/opensphere_checkpoints/20220424_210641/config.yml")
    a("--opensphere_model_path", type=str, default="../data/4-opensphere_checkpoints/opensphere_checkpoints/20220424_210641/models/backbone_100000.pth")
    a("--output_dir", type=str, default="./outputs")
    a("--logging_dir", type=str, default="logs")
    a("--report_to", type=str, default="wandb")
    # 5. optimisation
    a("--learning_rate", type=float, default=5e-5)
    a("--lr_scheduler", type=str, default="constant")
    a("--lr_warmup_steps", type=int, default=0)
    a("--lr_num_cycles", type=int, default=1)
    a("--lr_power", type=float, default=1.0)
    a("--allow_tf32", action="store_true", default=True)
    a("--adam_beta1", type=float, default=0.9)
    a("--adam_beta2", type=float, default=0.999)
    a("--adam_weight_decay", type=float, default=1e-2)
    a("--adam_epsilon", type=float, default=1e-08)
    a("--max_grad_norm", default=100.0, type=float)
    a("--img_size_small", type=int, default=224)
    a("--size_face", type=int, default=224)
    a("--size_aligned_face", type=int, default=112)
    a("--face_gender_confidence_level", type=float, default=0.9)
    a("--local_rank", type=int, default=-1)
    a("--config", type=str, default=None)
    return p


EXTRA_DEFAULTS = dict(num_denoising_steps=0, synthetic=False, face_provider="synthetic", num_classifier_logits=80, lora_up_std=0.0, validation="off",
                      train_monitor="off", index_font=None, index_font_size=100, log_norms=False)


def parse_args(input_args=None, with_extras=False, experiment="exp-1", resolve=True, cfgs=None):
    """``resolve=False`` (``factory.default_args``): the defaults of ``custom`` without checking its specification, which is not given yet.
    ``cfgs``: the model sizes of the run (default: ``factory.SD15``, or ``TINY`` under FD_TINY), read only to check ``--size_face`` of a zero-shot run."""
    p = build_parser(experiment)
    if with_extras:
        p.add_argument("--num_denoising_steps", type=int, default=0, help="0 = draw from range(19,24) like the reference")
        p.add_argument("--synthetic", action="store_true", default=False)
        p.add_argument("--face_provider", type=str, default="synthetic")
        if experiment != "custom":
            p.add_argument("--num_classifier_logits", type=int, default=80)
        p.add_argument("--lora_up_std", type=float, default=0.0)
        p.add_argument("--validation", type=str, default="off", choices=["off", "metrics", "grids", "grids_attrs"])
        p.add_argument("--train_monitor", type=str, default="off", choices=["off", "metrics", "plots"])
        p.add_argument("--index_font", type=str, default=None, help="font file, or 'default': print the image index on every grid tile; not given: no text")
        p.add_argument("--index_font_size", type=int, default=100)
        p.add_argument("--log_norms", action="store_true", default=False, help="log the LoRA / EMA parameter norms and the gradient norm of every step")
    args = p.parse_args(input_args) if input_args is not None else p.parse_args()
    if args.config:
        with open(args.config, "r") as f:
            config_data = yaml.safe_load(f)
        d = vars(args)
        for key, value in config_data.items():
            d[key] = type(d[key])(value)
        args = argparse.Namespace(**d)
    if experiment == "custom" and resolve:      # every malformed value of the target specification is refused here
        from .fairness import experiment_spec
        spec = experiment_spec(experiment, args)
        if spec.zero_shot:
            if cfgs is None:
                from .factory import SD15, TINY
                cfgs = TINY if os.environ.get("FD_TINY") else SD15
            side = cfgs["clip_vision"].image_size
            if args.size_face != side:
                raise ValueError(f"--size_face {args.size_face}: --classifier zero_shot scores the face chips with the CLIP image tower, which takes {side} x {side}")
            # the head is defined by the prompts: the two derived flags read as if they had been given
            args.num_classifier_logits = spec.num_logits
            args.attributes = ",".join(f"{n}:{c}:{k}" for n, c, k in spec.attrs)
    env_local_rank = int(os.environ.get("LOCAL_RANK", -1))
    if env_local_rank != -1 and env_local_rank != args.local_rank:
        args.local_rank = env_local_rank
    return args
