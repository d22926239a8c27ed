"""What folding the LoRA into the base weights buys at inference, on one MI355X: ``generate.generate_image`` at SD-v1.5 size with synthetic weights and a
rank-50 U-Net LoRA, 30 steps, batch 10, a few prompts -- the models built as ``generate.main`` builds them, with the LoRA slabs (``--mode unmerged``) or on
the folded weights of ``--merge_lora`` (``--mode merged``).  ``--mode fold`` runs the 128-pair fold alone (what to put behind
``rocprofv3 --kernel-trace --stats --``).  One JSON line per run.  ``--root DIR`` takes the package from another checkout (the parent commit's unmerged
figure on the same machine).

    python scratch/measure_lora_merge.py --mode unmerged|merged|fold [--root DIR] [--batches 3]
"""
import argparse
import json
import os
import sys
import time

import torch

p = argparse.ArgumentParser()
p.add_argument("--mode", choices=["unmerged", "merged", "fold"], required=True)
p.add_argument("--root", default=os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
p.add_argument("--batches", type=int, default=3)
p.add_argument("--rank", type=int, default=50)
args = p.parse_args()
sys.path.insert(0, os.path.abspath(args.root))
import finetune_fair_diffusion_amd  # noqa: E402  (before the first HIP call)
from finetune_fair_diffusion_amd import generate, weights as W  # noqa: E402
from finetune_fair_diffusion_amd.factory import SD15, build_trainer, default_args  # noqa: E402
from finetune_fair_diffusion_amd.train import HashTokenizer  # noqa: E402

PROMPTS = ["a photo of a doctor", "a photo of a chef, a person", "a portrait of a teacher in a classroom"]
S, B = 30, 10


def synthetic_lora(cfg, rank):
    sd = W.synthetic_state_dict(W.unet_lora_param_shapes(cfg, rank), seed=5)
    g = torch.Generator().manual_seed(15)
    return {k: torch.randn(v.shape, generator=g) * 0.02 if ".up." in k else v for k, v in sd.items()}


def main():
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    cfg = SD15["unet"]
    lora = synthetic_lora(cfg, args.rank)
    out = dict(mode=args.mode, package=os.path.dirname(finetune_fair_diffusion_amd.__file__), rank=args.rank, steps=S, batch=B)
    state_dicts = {}
    if args.mode == "unmerged":
        state_dicts["unet_lora"] = lora
    else:
        from finetune_fair_diffusion_amd.merge import merge_state_dict
        base = W.synthetic_state_dict(W.unet_param_shapes(cfg), seed=0 + 1)
        for rep in range(2):                                     # the second call: no code-object load, a warm allocator
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            merged = merge_state_dict(base, lora, "unet", cfg, dev)
            out["fold_wall_s_call_%d" % rep] = round(time.perf_counter() - t0, 4)
        state_dicts["unet"] = merged
        if args.mode == "fold":
            print(json.dumps(out))
            return
    targs = default_args(train_unet=args.mode == "unmerged", train_text_encoder=False, rank=args.rank, guidance_scale=7.5)
    tr, _ = build_trainer(targs, dev, SD15, state_dicts=state_dicts, frozen_copies=False)
    tok = HashTokenizer(SD15["clip"].vocab_size)
    lat = cfg.sample_size
    times = []
    for i in range(args.batches + 1):                            # batch 0 warms up
        tokens = tok(PROMPTS[i % len(PROMPTS)])
        noises = torch.randn(B, 4, lat, lat, generator=torch.Generator().manual_seed(1997 + i)).to(dev)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        imgs = generate.to_uint8_hwc(generate.generate_image(tr, tokens, noises, S))
        times.append(time.perf_counter() - t0)
    out.update(batch_s=[round(t, 4) for t in times[1:]], warmup_s=round(times[0], 3), images_per_s=round(B * args.batches / sum(times[1:]), 3),
               checksum=int(imgs.astype("int64").sum()))
    print(json.dumps(out))


main()
