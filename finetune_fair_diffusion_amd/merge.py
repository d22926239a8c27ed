"""Folds exported LoRA files into the base weights: a plain Stable-Diffusion directory whose U-Net / text-encoder matrices already hold
``W + scale * up @ down`` -- what any diffusers version, any other consumer and ``generate.py`` without a LoRA flag load.

    python -m finetune_fair_diffusion_amd.merge --pretrained_model_name_or_path DIR --save_dir OUT \\
        [--load_unet_lora_from F] [--load_text_encoder_lora_from F] [--lora_scale 1.0] [--gpu_id 0]

The LoRA files are the ones ``export_checkpoint`` writes (``{unet,text_encoder}_lora{,_EMA}.pth``: the ``_EMA`` files are ordinary inputs, the
choice of file is the choice of weights).  The fold is fp32 on the device, one ``fd_lora_merge_multi`` call per network through
``layers.refresh_pairs(..., merge=...)``, bit-reproducible -- ``generate.py --merge_lora`` runs the same function on the same tensors, so the two
agree byte for byte.  ``OUT`` is a complete model directory: ``OUT/unet/diffusion_pytorch_model.safetensors`` and
``OUT/text_encoder/model.safetensors`` are written for the networks that were merged, with every tensor of the source file under its source name
and dtype and only the merged targets replaced (fp32); everything else of ``DIR`` is copied unchanged.  Every refusal -- no LoRA file, a missing
file, a key or shape that does not fit, a non-empty ``OUT``, no HIP device -- comes before ``OUT`` is created.
"""
import argparse
import os
import shutil

import torch

from . import weights as W

KINDS = ("unet", "text_encoder")
MAX_RANK = 64                    # fd_lora_merge_multi: 1 <= r <= 64
UNET_FILES = ("diffusion_pytorch_model.safetensors", "diffusion_pytorch_model.bin")         # as pretrained.load_unet looks for them
TE_FILES = ("model.safetensors", "pytorch_model.bin")                                      # pretrained.load_text_encoder
OUT_FILE = {"unet": os.path.join("unet", UNET_FILES[0]), "text_encoder": os.path.join("text_encoder", TE_FILES[0])}


def lora_targets(kind, cfg):
    """[(down key, up key, base key)] of every LoRA pair of one network, in the order of its LoRA inventory (``weights.unet_lora_param_shapes`` /
    ``clip_lora_param_shapes``): the keys of the exported file and the key of the base matrix [N, K] the pair is added to."""
    if kind == "unet":
        out = []
        for name in W.unet_attn_names(cfg):
            attn = name[:-len(".processor")]
            for proj, tgt in (("to_q", "to_q"), ("to_k", "to_k"), ("to_v", "to_v"), ("to_out", "to_out.0")):
                out.append((f"{name}.{proj}_lora.down.weight", f"{name}.{proj}_lora.up.weight", f"{attn}.{tgt}.weight"))
        return out
    if kind == "text_encoder":
        out = []
        for i in range(cfg.num_hidden_layers):
            for tgt in W.TE_LORA_TARGETS:
                p = f"text_model.encoder.layers.{i}.{tgt}"
                out.append((p + ".lora_linear_layer.down.weight", p + ".lora_linear_layer.up.weight", p + ".weight"))
        return out
    raise ValueError(f"kind must be one of {KINDS}, not {kind!r}")


def check_pairs(base_sd, lora_sd, kind, cfg):
    """The host half of ``merge_state_dict`` (no device): -> [(down key, up key, base key)] after every key and shape has been checked.  The rank is
    read from the file, pair by pair.  Refused by name: a pair without its twin, a pair of the inventory the file lacks, a key of the file the
    inventory does not know, a target missing from the base, a shape that does not fit, a rank outside 1..64."""
    triples = lora_targets(kind, cfg)
    known = {k for dn, un, _ in triples for k in (dn, un)}
    unknown = [k for k in lora_sd if k not in known]
    if unknown:
        raise KeyError(f"{kind} LoRA file: {unknown[0]} is not a LoRA tensor of this {kind} ({len(unknown)} such keys)")
    for dn, un, bk in triples:
        if (dn in lora_sd) != (un in lora_sd):
            have, lack = (dn, un) if dn in lora_sd else (un, dn)
            raise KeyError(f"{kind} LoRA file: {have} has no twin {lack}")
        if dn not in lora_sd:
            raise KeyError(f"{kind} LoRA file: the pair {dn} / {un} is missing")
        if bk not in base_sd:
            raise KeyError(f"{kind}: the base weights have no {bk} (target of {dn})")
        d, u, b = tuple(lora_sd[dn].shape), tuple(lora_sd[un].shape), tuple(base_sd[bk].shape)
        if len(d) != 2 or len(u) != 2 or d[0] != u[1]:
            raise ValueError(f"{kind} LoRA file: {dn} {d} and {un} {u} are not a [r, K] / [N, r] pair")
        if not 1 <= d[0] <= MAX_RANK:
            raise ValueError(f"{kind} LoRA file: {dn} has rank {d[0]}; ranks 1..{MAX_RANK} can be merged")
        if b != (u[0], d[1]):
            raise ValueError(f"{kind}: {bk} has shape {b}, but {un} {u} @ {dn} {d} is {(u[0], d[1])}")
    return triples


def merge_state_dict(base_sd, lora_sd, kind, cfg, device, scale=1.0):
    """``base_sd`` (by diffusers / transformers key, as ``pretrained.load_unet`` / ``load_text_encoder`` or ``weights.synthetic_state_dict`` give it)
    with every LoRA target replaced by ``W + scale * up @ down`` as an fp32 CPU tensor; biases and every other tensor are the SAME objects.  The base
    matrices go to ``device`` as fp32, the file into a ``ParamBank``, and one ``refresh_pairs(..., merge=...)`` call folds all pairs in place there."""
    from .layers import LoRAPair, ParamBank, refresh_pairs
    triples = check_pairs(base_sd, lora_sd, kind, cfg)
    device = torch.device(device)
    if device.type != "cuda" or not torch.cuda.is_available():
        raise RuntimeError("finetune_fair_diffusion_amd.merge needs an MI355X (HIP device); there is no CPU path")
    shapes = {k: tuple(lora_sd[k].shape) for dn, un, _ in triples for k in (dn, un)}
    bank = ParamBank(shapes, device)
    bank.load_state_dict(lora_sd)
    pairs = [LoRAPair(bank, dn, un) for dn, un, _ in triples]
    outs = [base_sd[bk].to(device, torch.float32).contiguous() for _, _, bk in triples]        # fresh device copies: folded in place
    with torch.cuda.device(device):
        refresh_pairs(pairs, scale, merge=[(o, o) for o in outs])
    merged = dict(base_sd)
    for (_, _, bk), o in zip(triples, outs):
        merged[bk] = o.cpu()
    return merged


def parse_args(input_args=None):
    p = argparse.ArgumentParser(description="Fold LoRA files into the weights of a Stable-Diffusion directory.")
    a = p.add_argument
    a("--pretrained_model_name_or_path", type=str, required=True)
    a("--save_dir", type=str, required=True)
    a("--load_unet_lora_from", type=str, default=None)
    a("--load_text_encoder_lora_from", type=str, default=None)
    a("--lora_scale", type=float, default=1.0)
    a("--gpu_id", type=int, default=0)
    return p.parse_args(input_args) if input_args is not None else p.parse_args()


def main(args, cfgs=None):
    from . import pretrained as P
    from .factory import SD15, TINY
    cfgs = cfgs or (TINY if os.environ.get("FD_TINY") else SD15)
    src, out = args.pretrained_model_name_or_path, args.save_dir
    jobs = [(kind, path) for kind, path in (("unet", args.load_unet_lora_from), ("text_encoder", args.load_text_encoder_lora_from)) if path]
    if not jobs:
        raise ValueError("nothing to merge: give --load_unet_lora_from and / or --load_text_encoder_lora_from")
    if not os.path.isdir(src):
        raise FileNotFoundError(f"{src}: not a local diffusers directory")
    for _, path in jobs:
        if not os.path.isfile(path):
            raise FileNotFoundError(path)
    if os.path.exists(out) and (not os.path.isdir(out) or os.listdir(out)):
        raise FileExistsError(f"{out} exists and is not empty")
    work = []
    for kind, path in jobs:
        files, shapes, cfg, rename = ((UNET_FILES, W.unet_param_shapes, cfgs["unet"], None) if kind == "unet" else
                                      (TE_FILES, W.clip_param_shapes, cfgs["clip"], P._clip_rename))
        raw = P._read([os.path.join(src, kind, f) for f in files])
        base = P._select(raw, shapes(cfg), kind, rename)
        lora = torch.load(path, map_location="cpu")
        triples = check_pairs(base, lora, kind, cfg)
        work.append((kind, cfg, files, rename, raw, base, lora, {bk for _, _, bk in triples}))
    if not torch.cuda.is_available():
        raise RuntimeError("finetune_fair_diffusion_amd.merge needs an MI355X (HIP device); there is no CPU path")
    device = torch.device("cuda", args.gpu_id)
    results = []
    for kind, cfg, files, rename, raw, base, lora, targets in work:
        merged = merge_state_dict(base, lora, kind, cfg, device, scale=args.lora_scale)
        tensors = {}
        for k, v in raw.items():
            k2 = rename(k) if rename else k
            tensors[k] = (merged[k2].reshape(v.shape) if k2 in targets else v).contiguous()
        results.append((kind, files, tensors))
    # nothing was refused: only now does OUT come into being
    from safetensors.torch import save_file
    replaced = {os.path.join(kind, f) for kind, files, _ in results for f in files}
    shutil.copytree(src, out, dirs_exist_ok=True,
                    ignore=lambda d, names: [n for n in names if os.path.relpath(os.path.join(d, n), src) in replaced])
    written = []
    for kind, _, tensors in results:
        path = os.path.join(out, OUT_FILE[kind])
        os.makedirs(os.path.dirname(path), exist_ok=True)
        save_file(tensors, path, metadata={"format": "pt"})
        written.append(path)
    return written


if __name__ == "__main__":
    main(parse_args())
