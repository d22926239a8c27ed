"""Headline benchmark: trained images / second of the fairness-finetuning step (BASELINE.json metric).

  python bench.py --gpus 1 --steps K --warmup W [--dump-outputs DIR] [--full]
  python -m torch.distributed.run --nnodes=1 --nproc-per-node N --master-addr 127.0.0.1 --master-port P bench.py --gpus N ...

A "step" is one full training step of exp-1-debias-gender/1-main-debias.py:1746-2029 (minus wandb/plots
and the detector side-car): R1 + R2 no-grad CFG rollouts of B images, R3 rollout with
recompute-backward, classifier, VAE forward/backward, LoRA-gradient all-reduce, AdamW + EMA.
Workload = BASELINE.json configs[1]: exp-1-debias-gender, batch 8 per GPU, S=20 DPM-Solver++ steps,
LoRA rank 4 on the U-Net, fp16, SD-v1.5 512x512, synthetic weights / prompts / noise.
One process per GPU; weak scaling (each rank trains its own B images, one RCCL all-reduce of the flat
LoRA-gradient buffer per step).

A plain run sets up, warms up, times K steps, writes the last timed step's outputs (--dump-outputs) and prints the
result line.  --full adds what takes runs of its own: the roofline step (per-launch HIP events, one stream), the
reference-schedule A/B steps and the CPU baseline; its whole process is budgeted to finish within 10 minutes.
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)

F_UNET = 0.798e12      # algorithmic FLOP per U-Net sample-forward (SURVEY.md 8d / BASELINE.md 2)
F_VAE = 2.515e12       # per 512x512 image decode
MFMA_PEAK_F16 = 2.5e15  # dense fp16 MFMA peak, MI355X_MICROARCH.md


def f_img(S):
    return 8 * S * F_UNET + 4 * F_VAE


def pmc_traffic(kernel, algorithmic_bytes_per_launch, headline):
    """HBM-side bytes per launch of the dominant kernel from the committed PMC passes (FETCH_SIZE / WRITE_SIZE cannot be read from inside a process; they are
    collected with rocprofv3 --pmc in separate runs, with the gfx950 corrections of MI355X_MICROARCH.md applied: FETCH_SIZE doubled).
    The in-situ passes (scratch/r0N_passes.sh: real data flow, the kernels in launch order; counter collection serialises the dispatches) profiled ONE
    configuration -- the headline one: fp16, batch 8, S = 20, exp-1, rank 4, full model, all loss terms -- and
    profiles/r0N_pmc_{fetch,write}_size_in_situ_step.csv hold its per-(kernel, grid) means: their dispatch-weighted mean is returned only when THIS run is
    that configuration (``headline``), i.e. for the same launch mix the roofline step times.  Any other run (other batch / S / dtype / experiment /
    --tiny) falls back to the per-shape traffic / algorithmic ratios of rounds 1-3 applied to this run's algorithmic bytes, and says so."""
    import csv
    root = os.path.join(os.path.dirname(os.path.abspath(__file__)), "profiles")
    for rnd in ("r06", "r05"):
        fp, wp = os.path.join(root, rnd + "_pmc_fetch_size_in_situ_step.csv"), os.path.join(root, rnd + "_pmc_write_size_in_situ_step.csv")
        if not (headline and os.path.exists(fp) and os.path.exists(wp)):
            continue

        def rows(path, col):
            return {(r["kernel"], r["workgroups"]): (float(r[col]), int(r["dispatches"])) for r in csv.DictReader(open(path)) if r["kernel"] == kernel}
        F, W = rows(fp, "FETCH_SIZE"), rows(wp, "WRITE_SIZE")
        keys = [k for k in F if k in W]
        n = sum(F[k][1] for k in keys)
        if n:
            traffic = sum((2.0 * F[k][0] + W[k][0]) * 1024.0 * F[k][1] for k in keys) / n
            return traffic, ("measured in situ: dispatch-weighted mean over %d launches of this kernel in a profiled bench step of the headline configuration (rocprofv3 "
                             "--pmc FETCH_SIZE x2 gfx950 correction + WRITE_SIZE, separate passes, profiles/%s_pmc_*_in_situ_step.csv); this run's mean algorithmic "
                             "bytes/launch: %.1f MB; Infinity-Cache hits are included" % (n, rnd, algorithmic_bytes_per_launch / 1e6))
    d = None
    for name in ("r03_pmc_traffic.json", "r02_pmc_traffic.json", "r01_pmc_traffic.json"):
        path = os.path.join(root, name)
        if os.path.exists(path):
            d = json.load(open(path))["kernels"].get(kernel)
            if d is not None:
                break
    if d is None:
        return None, "no PMC summary committed for " + kernel + ("" if headline else " (not the headline configuration: the in-situ passes do not apply)")
    ratio = sum(x["hbm_bytes"] for x in d["shapes"]) / sum(x["algorithmic_bytes"] for x in d["shapes"])
    return algorithmic_bytes_per_launch * ratio, "bytes/launch = mean algorithmic bytes/launch of this run (%.1f MB) x %.2f, the rocprofv3 PMC ratio " \
        "(FETCH_SIZE x2 gfx950 correction + WRITE_SIZE) / algorithmic bytes on this kernel's shapes (isolated passes of rounds 1-3%s); Infinity-Cache hits are included" % (
            algorithmic_bytes_per_launch / 1e6, ratio, "" if headline else "; not the headline configuration, so the in-situ passes do not apply")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    # one step in ~10 runs 100-250 ms long on this pool (host-side, with or without the Python GC: profiles/r02_step_time_jitter.txt);
    # four timed steps keep one such outlier from moving the line by more than ~3 %
    ap.add_argument("--steps", type=int, default=12)      # 16 s of timed region: one +40 ms step (seen once in 4 on one box) moves the mean by 3 ms instead of 10
    ap.add_argument("--warmup", type=int, default=3)      # the second step still grows the caching allocator's pools (40-step soak: step 2 is ~10 % long)
    ap.add_argument("--batch", type=int, default=8, help="train_images_per_prompt_GPU")
    ap.add_argument("--S", type=int, default=20, help="denoising steps")
    ap.add_argument("--rank", type=int, default=4, help="LoRA rank")
    ap.add_argument("--tiny", action="store_true", help="tiny model config (plumbing check only; not a valid bench line)")
    ap.add_argument("--backend", default="nccl", help="torch.distributed backend (nccl = RCCL; gloo only for single-GPU plumbing checks)")
    ap.add_argument("--share_gpu0", action="store_true", help="plumbing check: every rank uses cuda:0")
    ap.add_argument("--dtype", default="fp16", choices=["fp16", "bf16"], help="working dtype; bf16 = BASELINE configs[4] (NOT the headline line)")
    ap.add_argument("--force_collectives", action="store_true", help="initialise the process group and run the step's collectives even at world size 1 (RCCL smoke on a one-GPU box)")
    ap.add_argument("--experiment", default="exp-1", choices=["exp-1", "exp-3", "exp-4", "exp-5"], help="exp-3/4/5: multi-attribute head + OT targets (not the headline config)")
    ap.add_argument("--no_regularisers", action="store_true", help="drop the CLIP/DINOv2 image-semantics and SFNet face-realism terms (loss_fair only)")
    ap.add_argument("--full", action="store_true", help="also run everything beyond the headline figure: the roofline step, the reference-schedule "
                                                            "A/B steps and the CPU baseline (off by default: a plain run only sets up, warms up and times)")
    ap.add_argument("--dump-outputs", dest="dump_outputs", default=None, metavar="DIR",
                    help="after the timed steps, write what the last timed step computed as DIR/<name>.npy (see dump_outputs)")
    ap.add_argument("--dump_shapes", default=None, help="--full: CSV of the roofline pass's GEMM/conv launches grouped by kernel and shape")
    ap.add_argument("--no_cpu_baseline", action="store_true", help="--full: skip the CPU baseline")
    ap.add_argument("--cpu_baseline_full", action="store_true", help="--full: cfg1-size oracle step (B=2, S=4), warm-up + median of 3 (~6 min)")
    ap.add_argument("--cpu_baseline_bounded", action="store_true", help="--full: keep the bounded CPU sample (B=1, S=1) even when --steps >= 20")
    ap.add_argument("--no_roofline", action="store_true", help="--full: skip the roofline step and the reference-schedule A/B")
    a = ap.parse_args()
    if a.steps < 1 or a.warmup < 0:
        ap.error("--steps must be >= 1 and --warmup >= 0")
    roofline = a.full and not a.no_roofline

    os.environ["FD_DTYPE"] = a.dtype          # fixed before the package is imported (selects libfairdiff_hip[_bf16].so)
    import finetune_fair_diffusion_amd  # noqa: F401  (first: its __init__ puts GPU_MAX_HW_QUEUES=8 in the environment, which HIP reads when the device is initialised)
    import torch
    import torch.distributed as dist
    world = int(os.environ.get("WORLD_SIZE", "1"))
    rank = int(os.environ.get("RANK", "0"))
    local = int(os.environ.get("LOCAL_RANK", "0"))
    assert world == a.gpus, f"--gpus {a.gpus} but WORLD_SIZE={world}: launch with torch.distributed.run --nproc-per-node {a.gpus}"
    # one process per GPU: this rank's share of the host (CPU affinity inside one NUMA node, intra-op threads) before the first HIP call
    from finetune_fair_diffusion_amd import affinity
    pinned = affinity.pin_rank(local, int(os.environ.get("LOCAL_WORLD_SIZE", world)))
    if a.share_gpu0:
        local = 0
    torch.cuda.set_device(local)
    dev = torch.device("cuda", local)
    if world > 1 or a.force_collectives:
        if a.force_collectives:    # single-rank RCCL smoke: every collective of the step runs through RCCL on hardware
            os.environ["FD_FORCE_COLLECTIVES"] = "1"
            os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
            os.environ.setdefault("MASTER_PORT", "29541")
        if a.backend == "nccl":
            dist.init_process_group("nccl", device_id=dev, rank=rank, world_size=world)
        else:
            dist.init_process_group(a.backend, rank=rank, world_size=world)

    from finetune_fair_diffusion_amd import factory, ops
    args = factory.default_args(experiment=a.experiment, train_unet=True, train_text_encoder=False, rank=a.rank, train_images_per_prompt_GPU=a.batch,
                                train_GPU_batch_size=3, val_GPU_batch_size=8, mixed_precision=a.dtype,
                                size_face=64 if a.tiny else 224, img_size_small=56 if a.tiny else 224,
                                weight_loss_img=0.0 if a.no_regularisers else 8.0,   # debias-unet.yaml:4
                                weight_loss_face=0.0 if a.no_regularisers else 1.0)  # debias-unet.yaml:5
    cfgs = factory.TINY if a.tiny else factory.SD15
    tr, models = factory.build_trainer(args, dev, cfgs=cfgs, seed=0, rank=rank, world_size=world, regularisers=not a.no_regularisers, experiment=a.experiment,
                                       lora_up_std=0.01)   # up != 0 as after one warm-up optimiser step
    L = 13
    tokens = factory.synthetic_tokens(L, cfgs["clip"].vocab_size)
    hw = cfgs["unet"].sample_size
    torch.manual_seed(5991 + rank)  # set_seed(seed, device_specific=True) (:693): per-rank noise, drawn on the CPU (:1746-1749)

    # The step is handed the NEXT step's inputs as well (the train loop knows them: prompt order and noise come from the host RNG, :1746-1749), so
    # the frozen-model rollout R2 of step n+1 -- independent of step n's update -- can start underneath step n's tail (step.py r2_prefetch_steps).
    # Every timed step still executes exactly one R2 rollout's worth of work: the steps it prefetches for its successor replace the ones its
    # predecessor prefetched for it.  The noise tensors are drawn in the same RNG order as before (one draw per step), as host tensors.
    nxt = [torch.randn([a.batch, 4, hw, hw], dtype=torch.float32)]

    def one_step():
        noises = nxt[0]
        nxt[0] = torch.randn([a.batch, 4, hw, hw], dtype=torch.float32)
        return tr.train_step(tokens, noises, a.S, next_step=dict(tokens_ori=tokens, noises=nxt[0], S=a.S))

    def fence():
        torch.cuda.synchronize()      # this rank's work is done before it enters the barrier ...
        if world > 1 or a.force_collectives:
            dist.barrier()
            torch.cuda.synchronize()  # ... and the barrier's own collective has completed before the clock is read

    for _ in range(a.warmup):
        one_step()
    tr.timers = True        # phase boundaries = HIP events on the launch stream (no host sync): recorded during the timed steps
    fence()
    step_t = [time.perf_counter()]
    t0 = step_t[0]
    for _ in range(a.steps):
        out = one_step()
        step_t.append(time.perf_counter())      # host time at the end of each step's enqueue + its own syncs (no extra sync added)
    fence()
    dt = time.perf_counter() - t0
    phases_default = tr.phase_ms()
    host_phases = tr.host_phase_ms()       # host enqueue time per phase of the last timed step (launch-bound check)
    tr.timers = None
    if world > 1:
        t = torch.tensor([dt], dtype=torch.float64, device=dev)
        dist.all_reduce(t, op=dist.ReduceOp.MAX)
        dt = float(t.item())
    ms_per_step = 1e3 * dt / a.steps
    value = world * a.batch * a.steps / dt
    if a.dump_outputs and rank == 0:      # before anything else runs a step: the arrays are the last timed step's
        dump_outputs(a.dump_outputs, out, tr.banks)

    line = {
        "metric": "training-images/sec (SD-v1.5 512^2, 20-step DPM-Solver++ unroll, fairness-finetune step)",
        "value": value, "unit": "images/s", "n_gpus": world, "steps": a.steps, "warmup": a.warmup, "ms_per_step": ms_per_step,
        "higher_is_better": True, "scaling": "weak", "vs_baseline": None, "dtype": "f16" if a.dtype == "fp16" else "bf16",
        "data": "synthetic",
        "config": {"workload": ("exp-1-debias-gender, batch %d/GPU, %d denoising steps, LoRA rank %d on U-Net, fp16, SD-v1.5 512x512 (BASELINE configs[1])"
                                % (a.batch, a.S, a.rank) if a.dtype == "fp16" else
                                "NOT THE HEADLINE: configs[4]'s working precision (%s) on the configs[1] workload, batch %d/GPU, %d steps, rank %d"
                                % (a.dtype, a.batch, a.S, a.rank))
                               if not a.tiny else "TINY plumbing config (not a bench line)",
                   "global_batch": world * a.batch, "steps_per_s": a.steps / dt, "parallelism": f"dp{world}",
                   "algorithmic_flop_per_image": f_img(a.S),
                   # the reference's algorithm counts 8*S*F_unet + 4*F_vae per image; what the chip EXECUTES is in step_mfma_frac_executed (same level, below)
                   "step_mfma_frac_algorithmic": value / world * f_img(a.S) / MFMA_PEAK_F16,
                   "loss_fair_mean": float(out["loss_fair"][out["loss_fair"] != -1].mean()) if (out["loss_fair"] != -1).any() else None,
                   "loss_terms": "loss_fair" if a.no_regularisers else "loss_fair + 8*dyn*(loss_CLIP[ViT-H/14] + loss_DINO[ViT-B/14]) + 1*loss_face[SFNet-20]",
                   "loss_CLIP_mean": float(out["loss_CLIP"].mean()) if "loss_CLIP" in out else None,
                   "loss_DINO_mean": float(out["loss_DINO"].mean()) if "loss_DINO" in out else None,
                   "loss_face_mean": float(out["loss_face"][out["loss_face"] != -1].mean()) if "loss_face" in out and (out["loss_face"] != -1).any() else None,
                   "grad_is_finite": bool(out["grad_is_finite"]),
                   "peak_hbm_gb": round(torch.cuda.max_memory_allocated() / 2 ** 30, 1),
                   "hip_hw_queues": os.environ.get("GPU_MAX_HW_QUEUES", "4 (runtime default)"),
                   "rank0_cpu_affinity": None if pinned is None else {"cpus": len(pinned[0]), "first": pinned[0][0], "last": pinned[0][-1], "torch_threads": pinned[1]},
                   "r3_activation_gb_per_timestep": round(tr.last_ctx_bytes / 2 ** 30, 2),
                   "r3_timesteps_kept_in_hbm": min(a.S, 1 + max(tr.last_ctx_budget, 0)) if tr.keep_activations else 0},
    }

    # executed vs algorithmic work: with R3 consuming R1's recorded forward the step EXECUTES 6*S*F_unet + 3*F_vae per image (R1 fwd, R2
    # fwd, one backward) while the reference's algorithm counts 8*S*F_unet + 4*F_vae; both fractions are reported
    shared = bool(tr.share_r1_r3 and args.val_GPU_batch_size >= a.batch)
    f_exec = (6 if shared else 8) * a.S * F_UNET + (3 if shared else 4) * F_VAE
    line["config"]["phase_ms"] = {k: round(v, 1) for k, v in phases_default.items()}   # last timed step, shipped schedule (streams overlap phases)
    # host time between the same marks: launches, host syncs, and time BLOCKED on a full stream queue (the host runs ~2600 C-ABI calls ahead of
    # the device, scratch/prof_queue_depth.py; pure enqueue cost is ~105 ms per 20-step rollout, scratch/prof_host_rollout.py with FD_TINY=1)
    line["config"]["host_ms_between_phase_marks"] = {k: round(v, 1) for k, v in host_phases.items()}
    line["config"]["host_ms_per_step"] = [round(1e3 * (b - a_), 1) for a_, b in zip(step_t[:-1], step_t[1:])]
    hs = sorted(line["config"]["host_ms_per_step"])
    if hs:      # ``value`` is the mean over the timed region (the contract); the median and the count of slow steps say how much of it is jitter
        med = hs[len(hs) // 2] if len(hs) % 2 else 0.5 * (hs[len(hs) // 2 - 1] + hs[len(hs) // 2])
        line["config"]["host_ms_per_step_median"] = round(med, 1)
        line["config"]["steps_slower_than_median_plus_20ms"] = sum(x > med + 20.0 for x in hs)
    line["config"].update(r2_steps_prefetched_under_previous_tail=int(tr.last_r2_prefetched), r3_consumes_r1_forward=shared, r1_r2_rollouts_on_two_streams=bool(tr.concurrent_r2), backward_timesteps_on_two_streams=bool(tr.concurrent_bwd), executed_flop_per_image=f_exec,
                          step_mfma_frac_executed=value / world * f_exec / MFMA_PEAK_F16)

    if roofline:
        # roofline pass: one more identical step with per-launch HIP events on the GEMM/conv kernel family (keyed by the rocprof kernel
        # name) and the per-phase HIP events of the trainer.  EVERY rank runs the step (its collectives must be matched); rank 0 measures.
        if rank == 0:
            ops.TIMER = ops.OpTimer()
            tr.timers = True
        conc, tr.concurrent_r2, concb, tr.concurrent_bwd = tr.concurrent_r2, False, tr.concurrent_bwd, False     # kernels timed in isolation on one stream
        one_step()
        tr.concurrent_r2, tr.concurrent_bwd = conc, concb
    if rank == 0 and roofline:
        summ = ops.TIMER.summary()
        if a.dump_shapes:
            with open(a.dump_shapes, "w") as f:
                f.write("kernel,M,N,K,K2,conv_mode,act,residual,split,launches,total_ms,avg_us,tflops\n")
                for r in ops.TIMER.shape_table():
                    f.write(",".join(['"%s"' % r[0]] + [str(v) for v in r[1:10]] + ["%.3f" % r[10], "%.2f" % r[11], "%.1f" % r[12]]) + "\n")
        ops.TIMER = None
        phases = tr.phase_ms()
        tr.timers = None
        line["config"]["phase_ms_single_stream"] = {k: round(v, 1) for k, v in phases.items()}
        top = max(summ.items(), key=lambda kv: kv[1]["ms"])
        name, s = top
        achieved = s["flops"] / (s["ms"] * 1e-3) / 1e12
        headline = (a.dtype == "fp16" and a.batch == 8 and a.S == 20 and a.rank == 4 and a.experiment == "exp-1" and not a.tiny and not a.no_regularisers)
        traffic, traffic_note = pmc_traffic(name, s["bytes"] / s["launches"], headline)
        # the same kernel under the SHIPPED multi-stream schedule: its mean duration in the committed rocprofv3 kernel trace of this command (HIP events per launch
        # would perturb the concurrent schedule; the roofline step above times the kernels one stream at a time).  Headline configuration only.
        in_situ = None
        if headline:
            import csv
            for rnd in ("r06",):
                path = os.path.join(ROOT, "profiles", rnd + "_bench_step_kernel_stats_final.csv")
                if os.path.exists(path):
                    for r in csv.DictReader(open(path)):
                        if r["name"] == name:
                            us = float(r["avg_us"])
                            in_situ = {"avg_launch_us": us, "frac": s["flops"] / s["launches"] / (us * 1e-6) / MFMA_PEAK_F16, "calls": int(r["calls"]),
                                       "source": "profiles/%s_bench_step_kernel_stats_final.csv (rocprofv3 --kernel-trace of bench.py --steps 4 --warmup 2, shipped schedule, all streams on)" % rnd}
        line["roofline"] = {"bound": "mfma", "kernel": name, "achieved": achieved, "in_situ": in_situ, "peak": MFMA_PEAK_F16 / 1e12, "unit": "TFLOP/s",
                            "frac": achieved / (MFMA_PEAK_F16 / 1e12), "traffic": traffic, "traffic_note": traffic_note,
                            "launches": s["launches"], "splitk_launches": s["splitk_launches"],
                            "avg_launch_us": 1e3 * s["ms"] / s["launches"], "algorithmic_flop_per_launch": s["flops"] / s["launches"],
                            "algorithmic_bytes_per_launch": s["bytes"] / s["launches"],
                            # the same launches against the other roof: short-K shapes (K = 320) of this family are closer to HBM than to MFMA
                            "algorithmic_GBps": s["bytes"] / (s["ms"] * 1e-3) / 1e9, "hbm_frac_of_8TBps": s["bytes"] / (s["ms"] * 1e-3) / 8e12,
                            "note": "kernel = rocprofv3 kernel name (fd_gemm_kernel_name); split-K launches of the instantiation are included and "
                                    "their HIP events bracket the splitk_reduce_kernel too",
                            "family": {k: {"launches": v["launches"], "ms": round(v["ms"], 2), "tflops": round(v["flops"] / (v["ms"] * 1e-3) / 1e12, 1),
                                           "frac": round(v["flops"] / (v["ms"] * 1e-3) / MFMA_PEAK_F16, 4)}
                                       for k, v in sorted(summ.items(), key=lambda kv: -kv[1]["ms"])}}
    if world == 1 and roofline and shared:
        # A/B, informational: the reference's own schedule (R1 and R3 each run their forward rollout; FD_NO_SHARE=1), after the timed region
        tr.share_r1_r3 = False
        one_step()
        fence()
        t1 = time.perf_counter()
        one_step()
        fence()
        line["config"]["images_per_s_reference_schedule_r1_and_r3_both_forward"] = a.batch / (time.perf_counter() - t1)
        tr.share_r1_r3 = True
    if world > 1:
        dist.barrier()
    if a.experiment != "exp-1":
        line["config"]["experiment"] = a.experiment
        line["config"]["ot_solver"] = "device (fd_ot_assign_sum)" if tr.ot_on_device else "host (scipy assignment)"
        line["config"]["ot_solve_ms"], line["config"]["ot_exposed_wait_ms"] = [round(v, 2) for v in tr.last_ot_ms]
    if a.force_collectives:
        line["config"]["collectives"] = "RCCL process group of world size %d: probability all-gather + flat LoRA-gradient all-reduce executed" % world

    if rank == 0 and world == 1 and a.full and not a.no_cpu_baseline and not a.tiny:
        del tr, models
        torch.cuda.empty_cache()
        # the section-8(d) protocol (cfg1: B=2, S=4, warm-up + median of 3, ~8 min on 16 threads) whenever the run is long enough to be the driver's
        # (--steps >= 20) or on request; the default short invocation keeps the bounded sample so that it finishes within minutes
        line["cpu_baseline"] = cpu_baseline(a.S, full=a.cpu_baseline_full or (a.steps >= 20 and not a.cpu_baseline_bounded), t_start=T_START)

    if rank == 0:
        print(json.dumps(line))
    if world > 1 or a.force_collectives:
        dist.destroy_process_group()


def cpu_model():
    try:
        for ln in open("/proc/cpuinfo"):
            if ln.startswith("model name"):
                return ln.split(":", 1)[1].strip()
    except OSError:
        pass
    return "unknown"


T_START = time.perf_counter()
# wall-clock budget of the whole bench.py --full process (which must end within 10 minutes): the cfg1 CPU protocol drops from median-of-3 to
# fewer timed steps (and says so) when its warm-up step shows that three would not fit
BUDGET_S = float(os.environ.get("FD_BENCH_BUDGET_S", "540"))

DUMP_BYTES = 60 * 2 ** 20     # --dump-outputs: at most this many bytes of array data in all
DUMP_WHOLE = 1 << 18          # arrays up to this many elements are written whole; larger ones share the rest of the budget as samples


def dump_outputs(path, out, banks):
    """--dump-outputs: every array the last timed step handed its caller (``train_step``'s dict; nested dicts as ``<key>.<sub>``, numbers as
    0-d arrays) plus what it left in the trainable state (``lora<i>_weights`` after the update, ``lora<i>_grad``), as ``path/<name>.npy``.
    Floating point is written as float32 (float64 stays float64), integers and flags as float64.  An array larger than DUMP_WHOLE elements
    is written as a fixed sample: the elements of its flattened form at sorted indices drawn without replacement by numpy's default_rng(0),
    the same for every run of the same arguments, so that two builds can be compared output for output."""
    import re
    import numpy as np
    import torch
    arrays = {}

    def add(name, v):
        if isinstance(v, dict):
            for k in sorted(v):
                add("%s.%s" % (name, k), v[k])
        elif isinstance(v, torch.Tensor):
            arrays[re.sub(r"[^A-Za-z0-9_.-]", "_", name)] = v.detach()
        elif isinstance(v, (bool, int, float)):
            arrays[re.sub(r"[^A-Za-z0-9_.-]", "_", name)] = torch.tensor(float(v), dtype=torch.float64)

    for k in sorted(out):
        add(k, out[k])
    for i, bank in enumerate(banks):
        add("lora%d_weights" % i, bank.flat)
        add("lora%d_grad" % i, bank.grad)
    if any(v.is_cuda for v in arrays.values()):
        torch.cuda.synchronize()

    def npdtype(v):
        return np.float32 if v.is_floating_point() and v.dtype != torch.float64 else np.float64

    big = [n for n, v in arrays.items() if v.numel() > DUMP_WHOLE]
    small_bytes = sum(v.numel() * np.dtype(npdtype(v)).itemsize for n, v in arrays.items() if n not in big)
    share = (DUMP_BYTES - small_bytes) // len(big) if big else 0          # bytes per sampled array
    os.makedirs(path, exist_ok=True)
    for name, v in arrays.items():
        dt = npdtype(v)
        cap = max(1, share // np.dtype(dt).itemsize)
        if name in big and v.numel() > cap:
            idx = np.sort(np.random.default_rng(0).choice(v.numel(), size=cap, replace=False))
            v = v.reshape(-1)[torch.from_numpy(idx).to(v.device)]
        np.save(os.path.join(path, name + ".npy"), v.cpu().to(torch.float64).numpy().astype(dt))


def cpu_baseline(S, full=False, t_start=None):
    """SURVEY 8d / BASELINE.md 3: the oracle (fp32 PyTorch restatement of the reference's diffusers path, stock torch ops) timed on this
    box's host cores on a COMPLETE fairness step at SD-v1.5 size -- BASELINE configs[0]: exp-1, LoRA rank 4 on the text encoder only --
    i.e. R1 + R2 no-grad rollouts, R3 rollout with autograd, VAE, classifier, loss, backward.
      default   ``protocol: "bounded_sample"``: B=1, S=1, one un-timed warm-up STEP (thread pools, oneDNN primitive caches -- the same
                warm-up the protocol prescribes) + ONE timed step (~40 s each on 64 threads); keeps the default bench within minutes
      --cpu_baseline_full   ``protocol: "cfg1"``: the section-8(d) protocol itself: B=2, S=4, one warm-up step, median of 3 timed steps
                (~11 min); its result is committed under profiles/ and quoted in DESIGN.md
    ``value`` = images/s of the timed sample itself; the extrapolation to configs[1] (B=8, S=20) by algorithmic FLOPs is labelled as such.
    Threads: FD_CPU_THREADS, default min(16, logical CPUs) -- NOT os.cpu_count(): on the pool's 256-logical-CPU hosts the oracle's U-Net
    forward takes 4.7 s on 8 torch threads, 3.7 s on 16, 4.3 s on 32, 6.1 s on 64, 9.6 s on 128 and 150 s on 256
    (profiles/r03_cpu_baseline_thread_scaling.txt; the boxes expose 256 logical CPUs but far fewer usable cores to the job): the fastest
    setting is the honest baseline."""
    import statistics
    import torch
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import util_models as U
    from oracle import fair_step as fs
    ncpu = os.cpu_count() or 1
    threads = int(os.environ.get("FD_CPU_THREADS", min(ncpu, 16)))
    torch.set_num_threads(threads)
    B, Sc, reps = (2, 4, 3) if full else (1, 1, 1)
    om = U.oracle_models(rank=4, train_unet=False, train_te=True, lora_up_std=0.01, size="sd15", eval_copies=True)
    models = dict(text_encoder=om["text_encoder"], unet=om["unet"], vae=om["vae"], classifier=om["classifier"], scheduler=om["scheduler"],
                  eval_text_encoder=om["eval_text_encoder"], eval_unet=om["unet"])
    from finetune_fair_diffusion_amd import factory
    tokens = factory.synthetic_tokens(13, 49408)
    cfg = dict(train_GPU_batch_size=4, val_GPU_batch_size=8, uncertainty_threshold=0.2, factor2=0.2, size_face=224)
    noises = torch.randn(B, 4, 64, 64, generator=torch.Generator().manual_seed(5991))

    def step():
        for p in om["lora_params"]:
            p.grad = None
        t0 = time.perf_counter()
        fs.fairness_step(models, tokens, noises, Sc, cfg)
        return time.perf_counter() - t0

    warm = step()                                                  # warm-up step (thread pools, oneDNN primitive caches), never counted
    if t_start is not None and full:
        left = BUDGET_S - (time.perf_counter() - t_start)
        reps = max(1, min(reps, int(left / (1.1 * warm))))
    times = [step() for _ in range(reps)]
    dt = statistics.median(times)
    flop = B * f_img(Sc)
    return {"value": B / dt, "unit": "images/s", "cores": threads, "kind": "port", "host_cpu_count": ncpu, "cpu_model": cpu_model(),
            "protocol": ("cfg1" if reps == 3 else f"cfg1_median_of_{reps}_time_budget") if full else "bounded_sample",
            "seconds_per_step": dt, "all_step_seconds": [round(t, 2) for t in times], "warmup_step_seconds": round(warm, 2),
            "sample": f"oracle fp32 full fairness step (R1+R2+R3 fwd/bwd, VAE, classifier, loss; exp-1, TE-LoRA r=4, SD-v1.5 512x512) at B={B}, S={Sc}: "
                      f"{f'SURVEY 8(d) protocol: median of {reps} after one warm-up step' if full else 'BOUNDED SAMPLE, not the 8(d) protocol number: one timed step after one warm-up step (--cpu_baseline_full runs the protocol: cfg1 B=2, S=4, median of 3; committed under profiles/)'}; "
                      f"{threads} torch threads on {ncpu} logical CPUs ({cpu_model()})",
            "achieved_tflops": flop / dt / 1e12,
            "extrapolated_to_configs1_images_per_s": (flop / dt) / f_img(S),
            "extrapolation_note": f"EXTRAPOLATION, not a measurement: sample FLOP/s ({flop / dt / 1e12:.3f} TFLOP/s) / {f_img(S) / 1e12:.1f} algorithmic TFLOP per trained image at S={S}"}


if __name__ == "__main__":
    main()
