"""exp-6 target phase on the MI355X: wall time of ``fairness.expected_transport_targets`` through the device solver
(``fd_ot_expected_targets``) against the host solver (what ``FD_OT_HOST=1`` selects), at N = 32 and N = 128 global faces, plus the
worker-thread solve time and the main thread's wait (``last_ot_ms``) of a tiny-model exp-6 step.  Prints one JSON line per measurement.

    python scratch/measure_exp6_targets.py [B ...]      (tiny-step batch sizes; default 16 32)
"""
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import finetune_fair_diffusion_amd  # noqa: E402,F401  (before the first HIP call)
from finetune_fair_diffusion_amd import ops  # noqa: E402
from finetune_fair_diffusion_amd.fairness import _corner_cost, composition_table, expected_transport_targets  # noqa: E402


def solver_phase(dev, N, reps=5):
    probs = torch.softmax(torch.randn(N, 4, generator=torch.Generator().manual_seed(N)) * 2.0, dim=-1)
    t0 = time.perf_counter()
    counts, weights = composition_table(N)
    table_s = time.perf_counter() - t0
    expected_transport_targets(probs, device=dev)              # warm-up (code object load, allocator)
    dev_ms = []
    for _ in range(reps):
        t0 = time.perf_counter()
        td, ud = expected_transport_targets(probs, device=dev)
        dev_ms.append(1e3 * (time.perf_counter() - t0))
    host_ms = []
    for _ in range(2):
        t0 = time.perf_counter()
        th, uh = expected_transport_targets(probs)
        host_ms.append(1e3 * (time.perf_counter() - t0))
    # the two kernels alone (inputs already in HBM), HIP events on the launch stream
    M = torch.from_numpy(_corner_cost([probs.numpy()], [4])).to(dev)
    c, w = torch.from_numpy(counts).to(dev), torch.from_numpy(weights).to(dev)
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
    k_ms = []
    for _ in range(reps):
        ev[0].record()
        ops.ot_expected_targets(M, c, w)
        ev[1].record()
        torch.cuda.synchronize()
        k_ms.append(ev[0].elapsed_time(ev[1]))
    print(json.dumps(dict(what="exp-6 target phase", N=N, compositions=len(counts), table_build_s=round(table_s, 3),
                          device_ms_median=round(float(np.median(dev_ms)), 3), device_ms=[round(x, 3) for x in dev_ms],
                          kernels_ms_median=round(float(np.median(k_ms)), 3), host_ms=[round(x, 1) for x in host_ms],
                          equal=bool(torch.equal(td, th)) and ud.numpy().tobytes() == uh.numpy().tobytes())), flush=True)


def tiny_step(dev, B, on_device, steps=3):
    import util_models as U
    from finetune_fair_diffusion_amd.step import FairnessTrainer
    om = U.oracle_models(train_unet=True, train_te=False, lora_up_std=0.05, num_classes=6)
    pm = U.product_models(om["sds"], dev, train_unet=True, train_te=False, num_classes=6)
    args = U.make_args(train_unet=True, train_text_encoder=False, uncertainty_threshold=0.5, train_images_per_prompt_GPU=B, val_GPU_batch_size=B)
    tr = FairnessTrainer(args, pm["text_encoder"], pm["unet"], pm["vae"], pm["classifier"], pm["scheduler"], eval_text_encoder=pm["eval_text_encoder"],
                         eval_unet=pm["eval_unet"], experiment="exp-6", device=dev)
    tr.ot_on_device = on_device
    tr.sync_and_update = lambda N_backward, apply_=True: True
    tokens = U.tiny_tokens()
    rec = []
    for i in range(steps):
        noises = torch.randn(B, 4, 32, 32, generator=torch.Generator().manual_seed(100 + i))
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        tr.train_step(tokens, noises, 3)
        torch.cuda.synchronize()
        rec.append(dict(step_ms=round(1e3 * (time.perf_counter() - t0), 1), solve_ms=round(tr.last_ot_ms[0], 2), wait_ms=round(tr.last_ot_ms[1], 3)))
    print(json.dumps(dict(what="tiny exp-6 step", B=B, solver="device" if on_device else "host", steps=rec)), flush=True)


if __name__ == "__main__":
    dev = torch.device("cuda:0")
    for N in (32, 128):
        solver_phase(dev, N)
    for B in [int(x) for x in sys.argv[1:]] or [16, 32]:
        for on_device in (True, False):
            tiny_step(dev, B, on_device)
