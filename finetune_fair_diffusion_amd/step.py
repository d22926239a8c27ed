"""The fairness-finetuning training step on one MI355X rank -- the hot path of
exp-1-debias-gender/1-main-debias.py:1746-2029 re-designed for this hardware:

* R1 / R2: no-grad CFG rollouts (``generate_image_no_gradient`` :998-1061) of the finetuned and the
  frozen original models: S fused U-Net forwards on the 2N CFG batch, one fused CFG+DPM-Solver++
  update kernel per step, VAE decode.
* R3: ``generate_image_w_gradient`` (:1063-1136) without an autograd graph: dL/dx_final is obtained once
  (classifier + VAE backward), and because the U-Net input is detached at every step the gradient of eps_i is
  the scalar ``grad_coef_i * c_i`` times dL/dx_final (scheduler.chain_coefs) -- every timestep is back-propagated
  independently.  The forward rollout keeps each timestep's activations in HBM when they fit (7.8 GB per
  timestep at batch 8; all 20 fit in 288 GB) and otherwise only its input latent [N,4,64,64], in which case the
  timestep is recomputed with recording right before its backward (the reference's gradient checkpointing, :748).
* all micro-batches of the reference (``train_GPU_batch_size`` chunks, :1889) run as ONE batch with
  per-image weights 1/n_j (identical gradient, see fairness.microbatch_weights).
* gradient sync: one RCCL all-reduce of the flat fp32 LoRA-gradient buffer + fused scale/finite
  check + one AdamW+EMA launch (replaces the 400 per-tensor collectives/launches of :1998-2029).

The loss is ``loss_fair + weight_loss_img * dynamic_weights * (loss_CLIP + loss_DINO)`` (:1904-1932) when the two image
encoders are attached (``clip_model`` / ``dino_model``, vit.py), plus ``weight_loss_face * loss_face`` (:1917-1932) when the
face-feature network and its feature database are attached (``face_net`` sfnet.py, ``face_db``); all input gradients join the
classifier's at the image and go through the VAE once.  A non-zero ``weight_loss_face`` without a face network is refused
rather than silently dropped.

``FairnessTrainer.train_step`` is the list of the step's phases and owns every phase mark; each phase is one method right below it, and data
crosses phases as return values or in the per-step record ``st`` (``_step_record``).  The device tail (exp-1 / exp-2: targets, loss, weights
and hook factors on the device, ONE read-back per step) and the host tail (exp-3..6, FD_HOST_TAIL=1) sit side by side inside each phase.
"""
import contextlib
import copy
import os
import threading
import time
from functools import partial
from types import SimpleNamespace

import torch
import torch.distributed as dist
import torch.nn.functional as F

from . import ops
from .fairness import (SyntheticFaceProvider, composition_table, expected_transport_targets, experiment_spec,
                       face_grad_factors, face_grad_factors_multi, fair_loss_and_grad, gen_dynamic_weights, gen_dynamic_weights_multi,
                       generate_dynamic_targets, mc_transport_plan, microbatch_weights, targets_from_plan)
from . import fairness_dev as FD
from . import unet as unet_mod
from .layers import F16, F32
from .lr_schedule import lr_lambda
from .sfnet import face_features, face_features_backward
from .vit import feature_loss_and_grad

_ROCTX = os.environ.get("FD_ROCTX") is not None


def _ctx_droppable_bytes(ctx):
    """Bytes of one timestep's context that lean recording does not keep (unet.TransformerBlock: the pre-gate FF projection, n1, n2)."""
    if isinstance(ctx, dict):
        n = sum(t.numel() * t.element_size() for k in ("proj", "n1", "n2") for t in (ctx.get(k),) if isinstance(t, torch.Tensor))
        return n + sum(_ctx_droppable_bytes(v) for v in ctx.values() if isinstance(v, (list, tuple)))
    if isinstance(ctx, (list, tuple)):
        return sum(_ctx_droppable_bytes(c) for c in ctx)
    return 0


def _ctx_bytes(obj, seen=None):
    """Bytes held by the tensors reachable from a recorded-forward context (unique storages)."""
    seen = set() if seen is None else seen
    if torch.is_tensor(obj):
        key = obj.untyped_storage().data_ptr()
        if key in seen:
            return 0
        seen.add(key)
        return obj.untyped_storage().nbytes()
    if isinstance(obj, dict):
        return sum(_ctx_bytes(v, seen) for v in obj.values())
    if isinstance(obj, (list, tuple)):
        return sum(_ctx_bytes(v, seen) for v in obj)
    return 0


def _record_stream(obj, stream):
    """Tell the caching allocator that the tensors of a recorded-forward context are also used on ``stream`` (they were allocated on
    the main stream): their memory is not handed out again before that stream's pending kernels have read them."""
    if torch.is_tensor(obj):
        if obj.is_cuda:
            obj.record_stream(stream)
    elif isinstance(obj, dict):
        for v in obj.values():
            _record_stream(v, stream)
    elif isinstance(obj, (list, tuple)):
        for v in obj:
            _record_stream(v, stream)


def _all_tensors(obj, out=None):
    """Every tensor reachable from a recorded-forward context (the race detector's ``bwd_keep_alive`` holds them past the backward)."""
    out = [] if out is None else out
    if torch.is_tensor(obj):
        out.append(obj)
    elif isinstance(obj, dict):
        for v in obj.values():
            _all_tensors(v, out)
    elif isinstance(obj, (list, tuple)):
        for v in obj:
            _all_tensors(v, out)
    return out


def _pow2_scale_dev(amax, target):
    """The power of two nearest to ``target / amax``, chosen ON THE DEVICE (``amax``: device tensor of any shape -> same-shape fp32, 1 where amax
    is 0 or not finite): the loss scales of the VAE / ViT / SFNet / U-Net backwards do not bounce through the host, so the tail of the step has no
    read-back between the two logits copies and the end of the step."""
    a = amax.float()
    ok = torch.isfinite(a) & (a > 0)
    s = torch.exp2(torch.round(torch.log2(target / torch.where(ok, a, torch.ones_like(a)))))
    return torch.where(ok, s, torch.ones_like(s))


def _scaled_backward(backward, grad, scale, unscale=1.0):
    """The device loss-scale idiom of every backward in the tail: the gradient enters multiplied by the power-of-two ``scale`` with gscale = 1;
    returns (result, unscale / scale) -- the caller multiplies by that exact inverse (a power-of-two multiply commutes with every rounding)."""
    return backward(grad * scale, 1.0), unscale / scale


# FD_HOST_TAIL=1 (A/B): exp-1's targets / loss assembly on the HOST as in rounds 1-3 (two logits read-backs in the tail); default: on the device
_HOST_TAIL = os.environ.get("FD_HOST_TAIL") is not None
_FINE_MARKS = os.environ.get("FD_FINE_MARKS") is not None


def _h2d(t, dev):
    """Small host tensor -> device without a blocking copy: staged through pinned memory (torch's caching host allocator) and copied
    non-blocking; ``t.to(dev)`` from pageable memory is a synchronous hipMemcpy behind everything queued on the launch stream.  The loss
    phase has nine such copies between its read-backs (loss phase 62-78 -> 55-58 ms; the whole step within noise,
    profiles/r03_step_ab_pinned_h2d.txt)."""
    return t.contiguous().pin_memory().to(dev, non_blocking=True)


class EMAState:
    """diffusers ``EMAModel`` decay schedule (no warm-up flag): decay_n = min(decay, (1+n)/(10+n)), first step copies."""

    def __init__(self, decay):
        self.decay, self.optimization_step = decay, 0

    def next_one_minus_decay(self):
        self.optimization_step += 1
        step = max(0, self.optimization_step - 1)
        d = 0.0 if step <= 0 else min((1 + step) / (10 + step), self.decay)
        return 1.0 - d


class FairnessTrainer:
    def __init__(self, args, text_encoder, unet, vae, classifier, scheduler, eval_text_encoder=None, eval_unet=None,
                 face_provider=None, experiment="exp-1", rank=0, world_size=1, device=None, clip_model=None, dino_model=None,
                 face_net=None, face_db=None, prefix_embedding=None):
        self.args = args
        self.prefix = prefix_embedding      # exp-2: trainable prompt-prefix vectors (prefix.PrefixEmbedding); every network stays frozen
        self.clip, self.dino = clip_model, dino_model
        self.use_img_loss = clip_model is not None and dino_model is not None and getattr(args, "weight_loss_img", 0) != 0
        if (clip_model is None) != (dino_model is None):
            raise ValueError("the image-semantics term needs both encoders (CLIP and DINOv2) or neither")
        self.face_net = face_net
        self.face_db = None if face_db is None else F.normalize(face_db.to(unet.device if device is None else device, F32), dim=-1)  # :88
        self.face_db16 = None if face_db is None else self.face_db.to(F16).contiguous()
        self.use_face_loss = face_net is not None and face_db is not None and getattr(args, "weight_loss_face", 0) != 0
        if (face_net is None) != (face_db is None):
            raise ValueError("the face-realism term needs both the face-feature network and its feature database, or neither")
        if self.use_img_loss and not self.use_face_loss and getattr(args, "weight_loss_face", 0) != 0:
            raise ValueError("weight_loss_face != 0 but no face-feature network / database is attached "
                             "(build_trainer(..., regularisers=True) attaches them; or pass --weight_loss_face 0)")
        # what this run trains towards, resolved once (fairness.ExperimentSpec): everything below reads the record, not the experiment's name
        self.spec = spec = experiment_spec(experiment, args)
        if self.use_img_loss or self.use_face_loss:
            self.factors1, self.factors2, self.face_conf = spec.regulariser_values(args)
        self.te, self.unet, self.vae, self.clf, self.sch = text_encoder, unet, vae, classifier, scheduler
        self.eval_te = eval_text_encoder if eval_text_encoder is not None else text_encoder
        self.eval_unet = eval_unet if eval_unet is not None else unet
        self.faces = face_provider or SyntheticFaceProvider()
        # which classifier columns carry which attribute (exp-1: CelebA attr 20 of 40x2 logits `:1370`; exp-3/5: 2+4; exp-4: 2+4+2)
        self.experiment = experiment
        self.attrs, self.class_cdfs, self.age_asym = spec.attrs, spec.class_cdfs, spec.asymmetric_last
        # exp-1 (one binary attribute): probabilities, dynamic targets, loss, dynamic weights and hook factors stay ON THE DEVICE (fairness_dev.py);
        # what the caller is told about the step (probabilities, targets, per-image losses) comes back in ONE read-back together with the
        # finite flag.  The multi-attribute experiments and exp-6 keep the host path (their OT solve has its own worker thread / device solver).
        self.device_tail = spec.solver == "rank" and not _HOST_TAIL
        # the rank rule's share of class 0 (exp-1 / exp-2: 0.5) and, for the enumeration, the target class probabilities (exp-6: uniform = None)
        self.target_ratio = spec.attributes[0].p[0] if spec.solver == "rank" else 0.5
        self.target_p = spec.attributes[0].p if (spec.solver == "enumerate" and spec.custom) else None
        # exp-6: one 4-class attribute whose targets are the expected transport plan over the exact enumeration of class compositions
        self.enumerated_targets = spec.solver == "enumerate"
        self._binom = {}
        self._pending_readback = None
        self.target_rng = torch.Generator().manual_seed(1234 + rank)
        self.rank, self.world = rank, world_size
        # collectives run whenever there is more than one rank -- or, with FD_FORCE_COLLECTIVES=1 and an initialised process group, on a
        # single rank too (the only way to drive the RCCL code path on a one-GPU box: RCCL refuses two ranks on one device)
        self.collectives = world_size > 1 or (os.environ.get("FD_FORCE_COLLECTIVES") is not None and dist.is_available() and dist.is_initialized())
        self._hbm_reserve = int(os.environ.get("FD_HBM_RESERVE_MB", "2048")) << 20      # since round 6 also without collectives: the runtime itself needs room (HSA_STATUS_ERROR_OUT_OF_RESOURCES at 0 free)
        self.device = device or unet.device
        self.banks, self.bank_keys = [], []       # keys: the reference's names in ``train_<key>_norm`` (:2034-2045; exp-2 :2126-2130)
        if getattr(args, "train_unet", False):
            self.banks.append(unet.lora_bank)
            self.bank_keys.append("unet_lora")
        if getattr(args, "train_text_encoder", False):
            self.banks.append(text_encoder.lora_bank)
            self.bank_keys.append("TE_lora")
        if self.prefix is not None:
            if self.banks:
                raise ValueError("exp-2 trains the prefix embedding only (1-main-debias.py:946): no LoRA banks next to it")
            self.banks.append(self.prefix.bank)
            self.bank_keys.append("prefix_embedding")
        self.ema = [EMAState(args.EMA_decay) for _ in self.banks]
        self.opt_step = 0
        self.lr_step = 0      # lr_scheduler.step() count: advances every step, also when the update is skipped (:2023)
        self.flag = torch.zeros(1, dtype=torch.int32, device=self.device)
        self.clf_gscale = 1024.0
        # R3 keeps per-timestep activations in HBM when they fit (MI355X: 288 GB) instead of recomputing every
        # timestep; set keep_activations=False for the pure recompute schedule of the reference (:748).
        self.keep_activations = True
        self.activation_mem_fraction = 0.85
        self.last_ctx_bytes = self.last_ctx_budget = 0
        self._full_ctx_bytes = 0              # bytes of one timestep's FULL context (measured by the first recording rollout)
        self._auto_lean = False              # the automatic mode chose lean recording once: it stays (see rollout_steps)
        # None: automatic (lean recording when S full contexts do not fit, from the second step on); True / False force it (FD_LEAN_ACTIVATIONS=1 / 0)
        self.lean_activations = {"1": True, "0": False}.get(os.environ.get("FD_LEAN_ACTIVATIONS", ""), None)
        # R1 and the forward half of R3 evaluate the same function on the same inputs (same prompt, noise, S and LoRA
        # weights; only the grad bookkeeping differs in the reference).  With deterministic, batch-invariant kernels the
        # two are bit-identical (asserted in tests), so R3 can consume R1's recorded rollout/decode/classifier forward.
        # ON by default whenever R1 runs as one chunk (val_GPU_batch_size >= B) and a separate frozen U-Net serves R2; FD_NO_SHARE=1
        # executes R1 and R3 separately, exactly like the reference (A/B measurement; same images, same gradient to rounding).
        self.share_r1_r3 = os.environ.get("FD_NO_SHARE") is None
        # per-phase wall-clock of the last step (HIP events on the launch stream; read with phase_ms()); None = off
        self.timers = None
        self._marks, self._host_marks = [], []
        # exp-3/4/5: run the Monte-Carlo OT solves on a worker thread underneath R2 (False = inline, like the reference)
        self.overlap_targets = os.environ.get("FD_NO_OT_OVERLAP") is None
        # R1 and R2 rollouts enqueued in lockstep on two HIP streams (FD_NO_CONCURRENT_R2=1: one after the other, as the reference does)
        self.concurrent_r2 = os.environ.get("FD_NO_CONCURRENT_R2") is None
        # backward of odd timesteps on the side stream (FD_NO_CONCURRENT_BWD=1: all on one stream)
        self.concurrent_bwd = os.environ.get("FD_NO_CONCURRENT_BWD") is None
        self.bwd_streams = int(os.environ.get("FD_BWD_STREAMS", "3"))     # measured: 2 -> 1647, 3 -> 1589, 4 -> 1633 ms per step (run-to-run noise ~2 %)
        self._side = None
        # ``_usable_free_bytes``: calls and allocator-snapshot walks so far, ``memory_reserved`` at the last walk, the side streams' share found by it
        self._snap_calls = self._snap_walks = self._other_stream_cache = 0
        self._snap_reserved = -1
        # race-detector knobs (tests / scratch/diag_hazard.py; never set by the product): ``bwd_virtual`` deals the timesteps to the same per-stream
        # gradient buffers but enqueues all of them on the launch stream -- same fp32 summation order as the concurrent schedule, so every
        # buffer must come out BIT-identical; ``bwd_keep_alive`` holds every consumed activation context until the backward has been joined;
        # ``debug_partials`` (a list) receives clones of the per-stream buffers before they are summed.
        self.bwd_virtual = False
        self.bwd_keep_alive = False
        self.debug_partials = None
        # R2 of the NEXT step does not depend on this step's update (frozen original models, its own noise and prompt): when the caller hands
        # over the next step's inputs (``train_step(..., next_step=...)``) its first denoising steps are enqueued on the R2 stream as soon as
        # this step's R2 has finished, i.e. underneath the VAE decode / classifier / loss / VAE backward tail, whose launches leave most of the
        # chip idle (host syncs, small kernels).  Same kernels on the same inputs: results are bit-identical with and without it.
        # same-box A/Bs.  Round 3: 0 -> 1442-1448 ms, 6 -> 1431-1436, 8 -> 1429, 10 -> 1440.  End of round 5 (medians of 6-step runs,
        # profiles/r05_step_ab_schedule_knobs_final_tree.txt): 0 -> 1317-1326, 2 -> 1309-1310, 4 -> 1307-1310, 5 -> 1309-1315, 6 -> 1309-1313, 7 -> 1315-1320, 8 -> 1316-1320,
        # 10 -> 1323-1325, 12 -> 1334-1338: the flat region moved down as the tail got shorter; 5 sits in its middle
        self.r2_prefetch_steps = int(os.environ.get("FD_R2_PREFETCH_STEPS", "5"))
        # the frozen model's forward (R2: a third of the step's U-Net passes) replayed as a hipGraph: bit-identical to the eager forward, ~2900 C-ABI
        # calls per forward become one launch -- the enqueue thread keeps a larger lead over the device in the rollout phase, where its lead is smallest
        # (fewer of the +50..95 ms steps, median -5..-15 ms in 20-step runs: profiles/r04_step_jitter_r2_graph.txt).  FD_R2_GRAPH=0 turns it off.
        self.r2_graph = os.environ.get("FD_R2_GRAPH", "1") != "0"
        self._r2_pre = None
        self._sch_r2 = None
        self.last_r2_prefetched = 0
        self.last_ot_ms = (0.0, 0.0)
        # the Monte-Carlo transport solves of exp-3/4/5 run on the GPU (csrc/assign.hip); FD_OT_HOST=1: the host solver (measurement switch)
        self.ot_on_device = os.environ.get("FD_OT_HOST") is None
        self._ot_stream = torch.cuda.Stream(device=self.device)
        self._tgt = None
        # training monitor (--train_monitor; train.py sets both): "off" / "metrics" / "plots", and whether THIS step is one the reference plots
        # (``step % train_plot_every_n_iter == 0``).  ``last_monitor``: what the last step's monitor produced (``_monitor_side``); None when off.
        self.monitor = "off"
        self.monitor_plot = False
        self.last_monitor = self._mon = None
        # ``evaluation.IndexLabels`` (--index_font; train.py sets it): the index text on the validation grids and the train plots.  None: no text.
        self.index_labels = None
        # --log_norms (train.py sets it): after every ``sync_and_update`` -- also a skipped one -- ``last_norms`` = {bank key: NormPlan.report}: the
        # per-tensor L2 norms of parameters, EMA and averaged gradient as they stand after the update, reduced on the device (``fd_bank_norms``)
        # and read back through one pinned buffer behind an event.  Off: no launch, no table, no buffer; ``last_norms`` stays None.
        self.log_norms = False
        self.last_norms = self._norms_host = None
        if self.enumerated_targets:      # the table of the usual global face count (every image has a face); other counts are built on the worker
            composition_table(world_size * getattr(args, "train_images_per_prompt_GPU", 0), self.attrs[0][2], self.target_p)

    # ------------------------------------------------------------------ per-phase timing (R1 / R2 / R3-fwd / R3-bwd / sync)
    def _mark(self, name):
        """Phase boundary: a HIP event on the launch stream (no host sync) and, with FD_ROCTX=1, a roctx range for rocprofv3 --marker-trace."""
        if self.timers is None:
            return
        ev = torch.cuda.Event(enable_timing=True)
        ev.record()
        self._marks.append((name, ev))
        self._host_marks.append((name, time.perf_counter()))
        if _ROCTX:
            if len(self._marks) > 1:
                torch.cuda.nvtx.range_pop()
            if name != "end":
                torch.cuda.nvtx.range_push(name)

    def _fine(self, name):
        """Sub-phase mark, only with FD_FINE_MARKS=1 (diagnosis of the host-bound tail; the bench line then carries the extra keys)."""
        if _FINE_MARKS:
            self._mark(name)

    def host_phase_ms(self):
        """{phase: ms} the HOST spent between the phase marks of the last step: launch-enqueue time (plus whatever host syncs the phase
        contains).  A phase whose host time equals its device time is launch-bound."""
        out = {}
        for (n0, t0), (_, t1) in zip(self._host_marks[:-1], self._host_marks[1:]):
            out[n0] = out.get(n0, 0.0) + (t1 - t0) * 1e3
        return out

    def phase_ms(self):
        """{phase: ms} of the last train_step (time from each mark to the next one), after a device sync."""
        torch.cuda.synchronize()
        out = {}
        for (n0, e0), (_, e1) in zip(self._marks[:-1], self._marks[1:]):
            out[n0] = out.get(n0, 0.0) + e0.elapsed_time(e1)
        return out

    def _side_stream(self, k=1):
        if self._side is None:
            self._side = {}
        if k not in self._side:
            self._side[k] = torch.cuda.Stream(device=self.device)
        return self._side[k]

    # ------------------------------------------------------------------ pieces
    def encode_pair(self, te, tokens, record=False, prefix=None):
        """tokens = (prompt_ids [L], prompt_mask [L], uncond_ids [L], uncond_mask [L]) -> enc [2,L,D] fp16, uncond first (:1035).
        ``prefix`` [n, D]: learned prefix-token embeddings for positions 1..n of the PROMPT sequence (exp-2 consumer)."""
        pid, pm, uid, um = tokens
        ids = torch.stack([uid, pid]).to(self.device)
        mask = torch.stack([um, pm]).to(self.device)
        return te.forward(ids, mask, record=record, prefix=None if prefix is None else (1, prefix))[0]

    def rollout_steps(self, unet, enc, noises, S, res, keep_inputs=False, record_prompt=False, keep_activations=False, sch=None):
        """CFG denoising rollout (:1038-1056) as a generator: yields after the launches of each denoising step so that two rollouts (R1
        on the current stream, R2 on the side stream) can be enqueued in lockstep; fills ``res`` = dict(lat, inputs, ctxs).
        With ``keep_activations`` the per-step backward contexts are kept for as many timesteps as fit in HBM
        (288 GB holds the whole 20-step chain at batch 8); the remaining steps are recomputed in the backward."""
        sch = self.sch if sch is None else sch       # a prefetched R2 rollout of the NEXT step brings its own scheduler object (S may differ)
        graphed = None
        if (self.r2_graph and unet is self.eval_unet and unet is not self.unet and unet.lora_bank is None
                and not keep_inputs and not keep_activations and not record_prompt and torch.cuda.current_stream() != torch.cuda.default_stream()):
            graphed = getattr(unet, "graphed", None) or unet_mod.GraphedForward(unet)
        sch.set_timesteps(S)
        unet.prepare_timesteps(sch.timesteps)
        unet.prepare_prompt(enc, record=record_prompt)
        if keep_activations and self.lean_activations is not False:
            # Lean recording (round 6; the reference's own memory lever is recompute, :748): when S timesteps of full contexts do not fit -- known from the previous
            # step's measured context size -- the transformer blocks keep half as much per token (unet.lean_record) and the backward recomputes three LayerNorms
            # and the FF1 projection per block instead of recomputing WHOLE timesteps: at S = 50, B = 8 that keeps ~45 of 50 timesteps instead of 28.
            full = self._full_ctx_bytes
            need_lean = self.lean_activations is True or (full > 0 and S * full > self.activation_mem_fraction * self._usable_free_bytes())
            if self.lean_activations is None and (need_lean or self._auto_lean):
                need_lean = self._auto_lean = True   # sticky in the automatic mode: a run whose S varies around the limit must not rebuild the allocator's pools every step
                                             # (a switch costs a device sync + ~10 s of pool refill; lean recording at a smaller S costs ~2 ms per timestep)
            if need_lean != unet.lean_record:
                # the caching allocator's pools hold blocks in the OTHER mode's sizes (28 timesteps x 16 pre-gate projections of 335 MB ...): they would sit
                # unused while the new mode's blocks come fresh from the driver until nothing is left for the runtime itself (HSA_STATUS_ERROR_OUT_OF_RESOURCES,
                # seen at S = 50 on the first lean step).  Hand them back once, at the switch (a device sync + a few ms; never in steady state).
                torch.cuda.synchronize()
                torch.cuda.empty_cache()
                self._snap_calls = 0
            unet.lean_record = need_lean
        lat = noises.clone()
        state, inputs, ctxs = {}, [], {}
        res.update(lat=lat, inputs=inputs, ctxs=ctxs)
        gs = self.args.guidance_scale
        budget = 0
        for i in range(S):
            if keep_inputs:
                inputs.append(lat.clone())
            rec = keep_activations and (i == 0 or budget > 0)
            if graphed is not None:        # the frozen model's non-recording forward as ONE hipGraph launch (unet.GraphedForward)
                eps = graphed(lat, i, True)
                sch.cfg_step(i, eps, gs, lat, state)
                yield i
                continue
            # cat([latents] * 2) (:1043): the two halves of the CFG batch share everything up to the first cross-attention (unet.forward_step(pair=True))
            eps = unet.forward_step(ops.to_f16(lat), i, record=rec, pair=True)
            if rec:
                ctxs[i] = unet._ctx
                unet._ctx = None
                if i == 0:
                    per = _ctx_bytes(ctxs[0])
                    usable = self.activation_mem_fraction * self._usable_free_bytes()
                    if not unet.lean_record:
                        self._full_ctx_bytes = per
                        if self.lean_activations is None and S * per > usable:
                            # the very first recording rollout of a run (context size unknown until now) and S full contexts do not fit: timestep 0 stays as
                            # recorded, the remaining ones are recorded lean (the backward takes either form per timestep) -- no full-mode step that fills the HBM
                            # to the last GiB before the switch (S = 50 soak of round 6: 0.66 GiB of driver-free memory at step 0)
                            unet.lean_record = self._auto_lean = True
                            per -= _ctx_droppable_bytes(ctxs[0])
                    budget = int(usable / max(per, 1))
                    self.last_ctx_bytes, self.last_ctx_budget = per, budget
                else:
                    budget -= 1
            sch.cfg_step(i, eps, gs, lat, state)
            yield i

    def _usable_free_bytes(self):
        """HBM the recording rollout (on the CURRENT stream) can still obtain without the allocator having to synchronise: what the driver
        reports free plus the cached, unallocated blocks of the caching allocator -- minus the part of that cache which sits in the pools
        of the side streams (R2 rollout, backward streams): a block freed on another stream is only handed to this one after an OOM-retry
        ``free_cached_blocks`` + device sync, i.e. a stall in the middle of the step.  The side-stream share is estimated
        from the allocator's per-stream segment snapshot."""
        free, _ = torch.cuda.mem_get_info()
        cached = torch.cuda.memory_reserved() - torch.cuda.memory_allocated()
        cur = torch.cuda.current_stream().cuda_stream
        n = self._snap_calls
        self._snap_calls = n + 1
        reserved = torch.cuda.memory_reserved()
        grown = abs(reserved - self._snap_reserved) > (1 << 30)      # the pools moved by > 1 GiB since the last walk (a new S / batch,
                                                                                      # fragmentation in a long run): the side-stream share is stale
        if n < 2 or n % 256 == 0 or grown:
            # the pools settle within two steps; the snapshot walks every block of the allocator (tens of ms of host time at 175 GB) right at
            # the start of a step, where the device queue is empty: refreshed rarely -- and whenever ``memory_reserved`` has moved
            self._snap_reserved = reserved
            self._snap_walks += 1
            other = 0
            try:
                for seg in torch.cuda.memory_snapshot():
                    if seg.get("stream", cur) != cur:
                        other += sum(b["size"] for b in seg.get("blocks", ()) if b.get("state") == "inactive")
            except Exception:
                other = cached // 2
            self._other_stream_cache = other
        # a multi-rank run shares the device with RCCL: its communicator is resident before the first step (factory.build_trainer broadcasts the LoRA init),
        # so ``free`` already excludes it; what arrives later -- channel buffers of collectives first used inside the step, the probability gather's
        # staging -- is covered by a fixed reserve (FD_HBM_RESERVE_MB; measured resident set of the single-rank RCCL soak: profiles/r05_soak_s50_collectives.txt)
        return max(free - self._hbm_reserve, 0) + max(cached - self._other_stream_cache, 0)

    def rollout(self, unet, enc, noises, S, keep_inputs=False, record_prompt=False, keep_activations=False):
        """noises [N,4,h,w] fp32 on device.  Returns (x_final, [x_i], {i: ctx})."""
        res = {}
        for _ in self.rollout_steps(unet, enc, noises, S, res, keep_inputs, record_prompt, keep_activations):
            pass
        return res["lat"], res["inputs"], res["ctxs"]

    def decode(self, lat, record=False):
        return self.vae.decode_images(lat * (1.0 / self.vae.config.scaling_factor), record=record)

    def classify_begin(self, images, record=False):
        """First half of ``classify``: face boxes from the provider, crop + resize, classifier forward -- everything ENQUEUED, nothing read
        back, so that the caller can enqueue more device work that does not need the logits before it blocks in ``classify_end``."""
        N = images.shape[0]
        ind, boxes = self.faces(images)
        sel = ind.nonzero().view(-1)
        logits_dev = None
        if len(sel):
            chips = ops.crop_resize(images[_h2d(sel, images.device)].contiguous() if len(sel) != N else images, _h2d(boxes[sel], self.device), -1.0,
                                    self.args.size_face)
            logits_dev = self.clf.forward(chips, record=record).float()
        return dict(N=N, ind=ind, boxes=boxes, sel=sel, logits_dev=logits_dev)

    def classify_end(self, h):
        """Second half: the read-back of the logits (a host sync with the launch stream) and the per-attribute host tensors."""
        N, ind, boxes, sel, logits_dev = h["N"], h["ind"], h["boxes"], h["sel"], h["logits_dev"]
        per = []
        logits = logits_dev.cpu() if logits_dev is not None else None
        if self.collectives:
            # exchange point 1 stays on the device: [N, sum k] probabilities (-1 rows = no face) for ONE all-gather of all attributes
            pd = torch.full((N, sum(k for _, _, k in self.attrs)), -1.0, dtype=F32, device=self.device)
            if logits_dev is not None:
                pd[_h2d(sel, self.device)] = torch.cat([torch.softmax(logits_dev[:, c0:c0 + k], dim=-1) for _, c0, k in self.attrs], dim=1)
            self._probs_dev = pd
        for name, c0, k in self.attrs:
            probs = torch.full((N, k), -1.0)
            preds = torch.full((N,), -1, dtype=torch.long)
            la_full = torch.full((N, k), -1.0)
            if logits is not None:
                la = logits[:, c0:c0 + k]
                la_full[sel] = la
                p = torch.softmax(la, dim=-1)
                probs[sel] = p
                preds[sel] = p.max(dim=-1).indices
            per.append(dict(name=name, preds=preds, probs=probs, logits=la_full))
        return ind, boxes, per

    def _r2_side_forwards(self, images_ori, B, consumer):
        """Classifier forward and regulariser features of the frozen side's images, enqueued on the CURRENT (R2) stream; the tensors are handed to
        ``consumer`` (the launch stream waits on the event recorded behind them)."""
        r = dict(h_o=self.classify_begin(images_ori))
        r.update(self._ori_features(images_ori, r["h_o"]["ind"], B))
        for t in (r["h_o"]["logits_dev"], r.get("clip_ori"), r.get("dino_ori"), r.get("face_ori")):
            if t is not None:
                t.record_stream(consumer)
        return r

    def _ori_features(self, images_ori, ind_o, B):
        """Regulariser features of the frozen side's images: normalised CLIP / DINOv2 embeddings and, per image with a face, its face features."""
        r = {}
        if self.use_img_loss:                                                    # :1860-1862
            e_co, e_do = self.image_features(self.resize_small(images_ori)[0])
            r.update(clip_ori=F.normalize(e_co, dim=-1), dino_ori=F.normalize(e_do, dim=-1))
        if self.use_face_loss:                                                   # :1870
            ch_o, idx_o, _ = self.aligned_faces(images_ori, ind_o)
            r["face_ori"] = torch.zeros((B, 512), dtype=F32, device=self.device)
            if len(idx_o):
                r["face_ori"][idx_o.long()] = F.normalize(face_features(self.face_net, ch_o)[0], dim=-1)
        return r

    def classify_dev(self, h):
        """``classify_end`` without the read-back (exp-1, ``device_tail``): the per-attribute tensors stay on the device."""
        N, ind, boxes, sel, logits_dev = h["N"], h["ind"], h["boxes"], h["sel"], h["logits_dev"]
        name, c0, k = self.attrs[0]
        if logits_dev is None:
            probs = torch.full((N, k), -1.0, dtype=F32, device=self.device)
            preds = torch.full((N,), -1, dtype=torch.long, device=self.device)
            lg = probs.clone()
        else:
            probs, preds, lg = FD.probs_preds(logits_dev, _h2d(sel, self.device), N, c0, k)
        return ind, boxes, [dict(name=name, preds=preds, probs=probs, logits=lg, ind_dev=_h2d(ind, self.device))]

    def _classify_read(self, h):
        """Per-attribute tensors of a ``classify_begin`` handle where this trainer's tail wants them: on the device, or read back to the host."""
        return self.classify_dev(h) if self.device_tail else self.classify_end(h)

    def _binom_tables(self, n):
        if n not in self._binom:
            self._binom[n] = tuple(t.to(self.device) for t in FD.binomial_tables(n, getattr(self, "target_ratio", 0.5)))
        return self._binom[n]

    def classify(self, images, record=False):
        """get_face + get_face_gender[_race[_age]] (:1794-1795; exp-3 :1387-1457; exp-4 :1378-1475).
        Returns indicators, boxes and per attribute (preds [N], probs [N,k] (-1 filled), logits [N,k])."""
        return self.classify_end(self.classify_begin(images, record=record))

    def resize_small(self, images):
        """``transforms.Resize(img_size_small)`` (:1860, :1905): bilinear, no antialias == the crop kernel on the full-image box."""
        N, _, H, W = images.shape
        box = torch.tensor([[0, 0, W, H]] * N, dtype=torch.int32, device=self.device)
        return ops.crop_resize(images, box, -1.0, self.args.img_size_small), box

    def image_features(self, small, record=False):
        """get_clip_feat / get_dino_feat (:1139-1175) raw embeddings (fp32) of both encoders."""
        return self.clip.forward(small, record=record), self.dino.forward(small, record=record)

    def aligned_faces(self, images, ind):
        """aligned_face_chips of get_face (:1337-1338, image_pipeline :292-312) for the images with a face.
        Returns (chips [n,3,112,112] fp16, src_index [n] int32, A [n,6] fp32) -- the last two drive the backward scatter."""
        from .fairness import alignment_sampling_matrix
        import numpy as np
        N, _, H, W = images.shape
        crop = self.args.size_aligned_face
        lms = self.faces.landmarks(images)
        sel = ind.nonzero().view(-1).tolist()
        A = np.stack([alignment_sampling_matrix(lms[i].numpy(), H, W, crop) for i in sel]) if sel else np.zeros((0, 6))
        A = _h2d(torch.tensor(A, dtype=F32), self.device)
        idx = _h2d(torch.tensor(sel, dtype=torch.int32), self.device)
        return ops.warp_affine(images, idx, A, crop), idx, A

    def nearest_face_feats(self, query):
        """FaceFeatsModel.semantic_search (:98-117): database row with the largest dot product.  fp16 MFMA scores shortlist 8
        candidates per query; the winner is chosen among them in fp32."""
        M = self.face_db.shape[0]
        q16 = torch.zeros(((query.shape[0] + 7) // 8 * 8, query.shape[1]), dtype=F16, device=self.device)
        q16[:query.shape[0]] = query.to(F16)
        scores = ops.gemm(self.face_db16, q16, out_dtype=F32)[:, :query.shape[0]].t()         # [n, M]
        cand = scores.topk(min(8, M), dim=-1).indices                                           # [n, 8]
        exact = (self.face_db[cand] * query[:, None, :]).sum(dim=-1)
        best = cand.gather(1, exact.argmax(dim=-1, keepdim=True))[:, 0]
        return self.face_db[best]

    def start_dynamic_targets(self, per, B):
        """Global dynamic targets for this rank's B images from the gathered probabilities of all ranks (:1831-1837; exp-3 :2016-2025),
        first half: ONE all-gather for all attributes (device tensors in, one host copy out), then
          * exp-1: the binomial-rank targets, inline (microseconds);
          * exp-3/4/5: the 100 Monte-Carlo transport solves of this rank start on a WORKER THREAD -- they only need the gathered
            probabilities, and nothing needs the targets before R3's loss, so they run underneath the R2 rollout that the main thread
            keeps enqueueing (the reference solves them serially between R1 and R2 on every rank, exp-3 `:1488-1536`);
          * exp-6: the same worker thread solves one transport problem per kept composition of the global faces and reduces them to the
            expected plan's targets (``fd_ot_expected_targets``, exp-6 `:1414-1483`); every rank computes the whole result from the same
            gathered probabilities, as the reference does, so there is nothing to all-reduce."""
        if getattr(self, "device_tail", False) and per[0]["probs"].is_cuda:
            pd = per[0]["probs"]
            if self.collectives:
                gl = [torch.empty_like(pd) for _ in range(self.world)]
                dist.all_gather(gl, pd.contiguous())
                pd = torch.cat(gl)
            t_all, u_all = FD.dynamic_targets(pd, self._binom_tables(pd.shape[0]), threshold=self.args.uncertainty_threshold,
                                              target_ratio=getattr(self, "target_ratio", 0.5))
            self._tgt = dict(B=B, dev=[(t_all[B * self.rank:B * (self.rank + 1)], u_all[B * self.rank:B * (self.rank + 1)])])
            return
        if not self.collectives:
            gathered = [a["probs"] for a in per]
        else:
            allp = self.gather_probs(self._probs_dev)                  # [world*B, sum k] on the host
            gathered, c = [], 0
            for _, _, k in self.attrs:
                gathered.append(allp[:, c:c + k].contiguous())
                c += k
        enumerated = getattr(self, "enumerated_targets", False)
        spec = getattr(self, "spec", None)
        self._tgt = dict(B=B, single=(len(per) == 1 and not enumerated) if spec is None else spec.solver == "rank")
        if self._tgt["single"]:
            self._tgt["res"] = [generate_dynamic_targets(gathered[0], target_ratio=getattr(self, "target_ratio", 0.5), w_uncertainty=True)]
            return

        st = self._tgt
        target_p = getattr(self, "target_p", None)

        def work():
            t0 = time.perf_counter()
            try:
                if enumerated:
                    if self.ot_on_device:       # inputs up, solves, reduction and the read-back all on the side stream of this thread
                        with torch.cuda.stream(self._ot_stream):
                            t, u = expected_transport_targets(gathered[0], device=self.device, p=target_p)
                        self._ot_stream.synchronize()
                    else:
                        t, u = expected_transport_targets(gathered[0], p=target_p)
                    st["res"] = [(t, u.float())]
                elif self.ot_on_device:       # fd_ot_assign_sum on a side stream of this thread; the summed plan stays in HBM for the all-reduce
                    with torch.cuda.stream(self._ot_stream):
                        idx, tp, sizes = mc_transport_plan(gathered, self.class_cdfs, 100, self.target_rng, self.age_asym, device=self.device)
                        if tp is not None and not self.collectives:
                            tp = tp.cpu()           # read back on THIS stream: a copy on the launch stream would wait for the queued rollout
                        st["plan"] = (idx, tp, sizes)
                    self._ot_stream.synchronize()
                else:
                    st["plan"] = mc_transport_plan(gathered, self.class_cdfs, 100, self.target_rng, self.age_asym)
            except BaseException as e:      # re-raised on the main thread by finish_dynamic_targets (a dead worker would otherwise surface
                st["error"] = e             # as KeyError('plan') here and as a collective timeout on the other ranks)
            st["solve_ms"] = 1e3 * (time.perf_counter() - t0)
        if self.overlap_targets:
            th = threading.Thread(target=work, daemon=True)
            th.start()
            self._tgt["thread"] = th
        else:
            work()

    def finish_dynamic_targets(self):
        """Second half: join the solver, ONE all-reduce of the summed plans (exchange point c11), marginals, threshold, this rank's slice.
        ``last_ot_ms`` = (host solve time, time the main thread actually waited here)."""
        st, args, B = self._tgt, self.args, self._tgt["B"]
        if "dev" in st:
            self._tgt = None
            return st["dev"]
        t0 = time.perf_counter()
        if not st["single"]:
            if "thread" in st:
                st["thread"].join()
            failed = torch.tensor([1.0 if "error" in st else 0.0])
            if self.collectives:            # every rank learns of a failed solve BEFORE the plan all-reduce, so all of them raise together
                f = failed.to(self.device)
                dist.all_reduce(f, op=dist.ReduceOp.MAX)
                failed = f.cpu()
            if float(failed) != 0:
                self._tgt = None
                raise RuntimeError("transport solve for the dynamic targets failed" +
                                   (" on this rank" if "error" in st else " on another rank")) from st.get("error")
            if "res" not in st:             # exp-3/4/5: the summed plans of all ranks (exp-6's worker already produced the targets)
                idx, tp, sizes = st["plan"]
                if tp is not None and tp.is_cuda:
                    tp.record_stream(torch.cuda.current_stream())
                if tp is not None and self.collectives:
                    t = tp.to(self.device)
                    dist.all_reduce(t, op=dist.ReduceOp.SUM)
                    tp = t
                st["res"] = targets_from_plan(idx, tp, sizes)
            self.last_ot_ms = (st.get("solve_ms", 0.0), 1e3 * (time.perf_counter() - t0))
        out = []
        for t, u in st["res"]:
            t = t.clone()
            t[u > args.uncertainty_threshold] = -1
            out.append((t[B * self.rank:B * (self.rank + 1)], u[B * self.rank:B * (self.rank + 1)]))
        self._tgt = None
        return out

    def dynamic_targets(self, per, B):
        self.start_dynamic_targets(per, B)
        return self.finish_dynamic_targets()

    # ------------------------------------------------------------------ the two exchange points of the step
    def gather_probs(self, probs):
        """(1) all-gather of the per-rank class probabilities [B,k] so every rank derives identical global targets
        (:1805-1837; the reference also gathers images/boxes/preds for plotting only)."""
        if not getattr(self, "collectives", self.world > 1):
            return probs
        pg = probs.to(self.device).contiguous()
        gl = [torch.empty_like(pg) for _ in range(self.world)]
        dist.all_gather(gl, pg)
        return torch.cat(gl).cpu()          # concatenated on the device, ONE copy to the host (it was one copy per rank)

    def finish_r2_prefetch(self):
        """Runs the remaining denoising steps of a prefetched next-step R2 rollout on its stream and makes the current stream wait for them.  The
        rollout's time embeddings and prompt projections live on the frozen U-Net object: whoever uses that U-Net between two training steps (the
        validation passes) calls this first, so the prefetch is completed instead of dropped -- the next step finds all S steps done."""
        pre = self._r2_pre
        if pre is None:
            return
        side = self._side_stream("r2")
        with torch.cuda.stream(side):
            for _ in pre["gen"]:
                pass
        pre["k"] = pre["S"]
        torch.cuda.current_stream().wait_stream(side)

    # ------------------------------------------------------------------ training monitor (--train_monitor; the reference's per-batch logs and plots)
    def _to_pinned(self, t):
        """Device tensor -> fresh pinned host tensor, copied asynchronously on the current stream (read once ``_mon["event"]`` has passed)."""
        host = torch.empty(t.shape, dtype=t.dtype, pin_memory=True)
        host.copy_(t, non_blocking=True)
        return host

    def _monitor_side(self, tag, images, h, tally):
        """One side of the monitor -- "generated" (R1, exp-3 :1978-2011) or "ori" (R2, :2052-2075) -- enqueued on the step's stream behind the
        producers of ``images`` and of ``classify_begin``'s handle ``h``; nothing is read back here and no random number is drawn.  The [B, sum k]
        probability table is gathered in rank order; with ``tally`` one ``ops.eval_tally`` launch reduces it to the 32 counts of
        ``evaluation.gap_metrics`` and they start their way to pinned memory.  On a plot step images and boxes are gathered too (every rank takes
        part, as in the reference) and rank 0 paints the grid in one launch (``evaluation.device_grid_attrs``), which follows the counts; with
        ``index_labels`` one more launch on the same stream draws the index text."""
        from . import evaluation as EV
        mon = self._mon
        plot = self.monitor == "plots" and self.monitor_plot
        if not (tally or plot):
            return
        pd = EV._gather_dev(self, EV.probability_table(self, h))
        mon["tables"][tag] = pd
        if tally:
            mon["counts"] = self._to_pinned(EV.tally_with_joint(self, pd))
        if plot:
            images_all = EV._gather_dev(self, images)
            bx = h["boxes"].to(torch.int32)
            boxes_all = EV._gather_dev(self, bx.to(self.device) if bx.is_cuda else _h2d(bx, self.device))
            mon["images"][tag], mon["boxes"][tag] = images_all, boxes_all
            if self.rank == 0:
                mon["grids"][tag] = self._to_pinned(EV.device_grid_attrs(self, images_all, boxes_all, pd, labels=self.index_labels))
        mon["event"] = torch.cuda.Event()
        mon["event"].record()

    def allreduce_grads(self):
        """(2) ONE all-reduce(SUM) per flat fp32 LoRA-gradient buffer (RCCL over xGMI on the GPU box)."""
        if getattr(self, "collectives", self.world > 1):
            for bank in self.banks:
                dist.all_reduce(bank.grad, op=dist.ReduceOp.SUM)

    # ------------------------------------------------------------------ the step: ``train_step`` lists the phases and owns every phase mark; the phases follow it
    def train_step(self, tokens, noises, S, tokens_ori=None, next_step=None):
        """``tokens``: the prompt the finetuned side sees (exp-2: ``prompt_debiaser(prompt)``, generate.prefix_tokens); ``tokens_ori``: the
        prompt of the frozen original side R2 when it differs (exp-2 :1954: the plain prompt, no prefix embedding).
        ``next_step``: optional dict(tokens_ori=, noises=, S=) -- the inputs the NEXT call will receive (noises as a host tensor): the first
        ``r2_prefetch_steps`` denoising steps of its R2 rollout are then enqueued underneath this step's tail.
        The phases below are called in enqueue order: what is queued on which stream in which order is part of the result and of the speed."""
        tokens_ori = tokens if tokens_ori is None else tokens_ori
        pre, noises = self._begin_step(tokens_ori, noises, S)
        self._mark("R1_rollout")
        st = self._step_record(tokens, tokens_ori, noises, S)
        out, dv = st.out, self.device_tail
        # ---- R1: images from the model being finetuned (:1786-1795); with ``st.conc`` R2 (frozen original, :1844-1858) runs beside it on its own stream
        g2, r2 = self._r2_start(st, pre)
        enc, r1s = self._r1_rollouts(st, g2)
        self._mark("R1_vae")
        images = self.decode(r1s[0]["lat"], record=True) if st.share else torch.cat([self.decode(r["lat"]) for r in r1s])
        if st.conc:
            images_ori, r2side, ev_r2 = self._r2_finish_on_side(st, g2, r2)
            self._prefetch_next_r2(st, next_step)       # queued behind ``ev_r2``: the launch stream never waits for a prefetch
        self._mark("classify_targets")
        gen = self._classify_generated(st, images)      # logits read-back (host tail), then the dynamic targets' solve starts underneath R2
        if st.conc:             # ---- R2: images from the frozen original models (:1844-1858)
            self._mark("R2_tail_and_regularisers")
            st.cur.wait_event(ev_r2)              # everything downstream (classifier, feature encoders, loss) consumes images_ori on ``cur``
            images_ori.record_stream(st.cur)
        else:
            self._mark("R2_rollout")
            enc_ori = self.encode_pair(self.eval_te, tokens_ori) if (self.eval_te is not self.te or st.train_prefix or tokens_ori is not tokens) else enc
            lats = [self.rollout(self.eval_unet, enc_ori, noises[j:j + st.vb], S)[0] for j in range(0, st.B, st.vb)]
            self._mark("R2_vae")
            images_ori, r2side = torch.cat([self.decode(x) for x in lats]), None
            self._mark("R2_classify_regularisers")
        ori = self._r2_complete(st, images_ori, r2side)
        tgt = self._targets(st, gen["per"])
        # ---- R3: rollout with gradient (:1889-1933), all micro-batches at once with weights 1/n_j (``st.w``)
        if st.share:            # R1's recorded rollout / decode / classifier forward IS R3's forward (``share_r1_r3``)
            gen.update(enc=enc, inputs=r1s[0]["inputs"], ctxs=r1s[0]["ctxs"])
        else:
            self._mark("R3_fwd_rollout")
            enc_g = self.encode_pair(self.te, tokens, record=st.rec_te, prefix=st.pv)
            x_final, inputs, ctxs = self.rollout(self.unet, enc_g, noises, S, keep_inputs=True, record_prompt=True, keep_activations=self.keep_activations)
            self._mark("R3_fwd_vae")
            images_g = self.decode(x_final, record=True)
            ind_g, boxes_g, per_g = self._classify_read(self.classify_begin(images_g, record=True))
            gen = dict(images=images_g, ind=ind_g, boxes=boxes_g, per=per_g, enc=enc_g, inputs=inputs, ctxs=ctxs)
        self._mark("R3_loss_and_image_grad")
        st.w_dev = _h2d(st.w, self.device) if dv else None
        dlog_full = self._fair_loss(st, gen, tgt)
        d_img = self._image_term(st, gen, ori, tgt) if self.use_img_loss else None
        d_img = self._face_term(st, gen, ori, tgt, d_img) if self.use_face_loss else d_img
        d_img = self._classifier_backward(st, gen, dlog_full, d_img)
        if d_img is not None:
            self._mark("R3_bwd_vae")
            g, step_scale, inv_gscale = self._vae_backward(st, d_img)
            self._mark("R3_bwd_unet")
            if st.train_unet or st.train_te or st.train_prefix:
                self._unet_backward(st, gen, g, step_scale, inv_gscale)
        else:
            self.vae._ctx = None
        gen["ctxs"].clear()
        for fn in st.deferred:      # the host tail's read-backs of reported values: only now, with the whole backward enqueued
            fn()
        self._mark("sync_update")       # ---- gradient sync, guard, update (:1998-2029)
        self._sync_and_report(st)
        self._mark("end")
        return out

    def _begin_step(self, tokens_ori, noises, S):
        """Takes the R2 rollout a previous step prefetched for these very inputs -- or drops it -- and moves the noise to the device; resets what the
        step accumulates (LoRA gradients, monitor, marks).  Returns (prefetch record or None, device noises)."""
        pre, self._r2_pre = self._r2_pre, None
        if pre is not None and not (pre["S"] == S and not noises.is_cuda and pre["noises_host"].shape == noises.shape and
                                    torch.equal(pre["noises_host"], noises.to(F32)) and
                                    all(torch.equal(a, b) for a, b in zip(pre["tokens_ori"], tokens_ori))):
            pre = None              # the caller changed its mind: the prefetched steps are dropped (their kernels were harmless)
        if pre is not None:         # the noise went up on the R2 stream: wait for it, and tell the allocator, BEFORE anything uses ``noises``
            torch.cuda.current_stream().wait_event(pre["ev_noise"])
            noises = pre["noises_dev"]
            noises.record_stream(torch.cuda.current_stream())
        else:
            noises = noises.to(self.device, F32)
        self.last_monitor = None
        self._mon = dict(tables={}, images={}, boxes={}, grids={}) if self.monitor != "off" else None
        for bank in self.banks:
            bank.grad.zero_()
        self._marks, self._host_marks = [], []
        return pre, noises

    def _step_record(self, tokens, tokens_ori, noises, S):
        """What every phase of one step needs to know: its inputs, what is trained, the schedule chosen for it, the micro-batch weights, and the
        three collectors -- ``out`` (the caller's dict), ``rb`` (device tail: name -> device tensor, read back ONCE at the end) and ``deferred``."""
        args, B, vb = self.args, noises.shape[0], self.args.val_GPU_batch_size
        train_te = getattr(args, "train_text_encoder", False) and self.te.lora_bank is not None
        train_unet = getattr(args, "train_unet", False) and self.unet.lora_bank is not None
        train_prefix = self.prefix is not None
        share = self.share_r1_r3 and vb >= B and self.eval_unet is not self.unet and (train_unet or train_te or train_prefix)
        # R1 (finetuned model) and R2 (frozen original, :1844-1858) are independent until the loss: with ``concurrent_r2`` their denoising
        # steps are enqueued in lockstep on two HIP streams, so the many launches that cannot fill 256 CUs on their own (16x16 / 8x8 levels,
        # tail waves, latency-bound short-K GEMMs) overlap with the other rollout's work.  Same kernels, same results.
        conc = self.concurrent_r2 and vb >= B and self.eval_unet is not self.unet
        w, N_backward = microbatch_weights(B, args.train_GPU_batch_size)
        return SimpleNamespace(tokens=tokens, tokens_ori=tokens_ori, noises=noises, S=S, B=B, vb=vb, train_te=train_te, train_unet=train_unet,
                               train_prefix=train_prefix, pv=self.prefix.vectors() if train_prefix else None, rec_te=train_te or train_prefix,
                               share=share, conc=conc, cur=torch.cuda.current_stream(),
                               side=self._side_stream("r2") if conc else None,      # its own stream: the backward's side streams must not queue behind a prefetch
                               w=w, w_dev=None, N_backward=N_backward, out={}, rb={}, deferred=[])

    def _r2_start(self, st, pre):
        """The concurrent R2 rollout as a generator on the R2 stream -- the prefetched one, already ``pre["k"]`` denoising steps ahead, or a new one."""
        self.last_r2_prefetched = 0
        if not st.conc:
            return None, {}
        if pre is not None:
            self.last_r2_prefetched = pre["k"]
            return pre["gen"], pre["res"]
        r2 = {}
        st.side.wait_stream(st.cur)
        with torch.cuda.stream(st.side):
            return self.rollout_steps(self.eval_unet, self.encode_pair(self.eval_te, st.tokens_ori), st.noises, st.S, r2), r2

    def _r1_rollouts(self, st, g2):
        """R1's denoising rollout(s): one recording rollout that R3 consumes (``st.share``) or plain ones in ``val_GPU_batch_size`` chunks.  One R2
        denoising step is enqueued on the R2 stream after each R1 step's launches.  Returns (enc, [rollout result per chunk])."""
        def lockstep(g1):
            for _ in g1:
                if st.conc:
                    with torch.cuda.stream(st.side):
                        next(g2, None)
        if st.share:
            enc, r1s = self.encode_pair(self.te, st.tokens, record=st.rec_te, prefix=st.pv), [{}]
            lockstep(self.rollout_steps(self.unet, enc, st.noises, st.S, r1s[0], keep_inputs=True, record_prompt=True, keep_activations=self.keep_activations))
        else:
            enc, r1s = self.encode_pair(self.te, st.tokens, prefix=st.pv), []
            for j in range(0, st.B, st.vb):
                r1s.append({})
                lockstep(self.rollout_steps(self.unet, enc, st.noises[j:j + st.vb], st.S, r1s[-1]))
        return enc, r1s

    def _r2_finish_on_side(self, st, g2, r2):
        """Rest of the concurrent R2 on its stream: drain, decode, the frozen side's forwards; ``ev_r2`` is what the launch stream later waits for."""
        with torch.cuda.stream(st.side):
            for _ in g2:           # (nothing left when both rollouts have S steps)
                pass
            images_ori = self.decode(r2["lat"])
            # the frozen side's classifier and regulariser forwards (:1860-1870) depend on images_ori only: enqueued HERE, on the R2 stream, they run
            # beside R1's last denoising steps instead of on the launch stream between R1's classifier and the loss
            r2side = self._r2_side_forwards(images_ori, st.B, st.cur)
        ev_r2 = torch.cuda.Event()
        ev_r2.record(st.side)         # this step's R2, not a prefetch queued behind it
        return images_ori, r2side, ev_r2

    def _prefetch_next_r2(self, st, next_step):
        """Enqueues the first ``r2_prefetch_steps`` denoising steps of the NEXT step's R2 on the R2 stream and leaves the rest in ``_r2_pre``."""
        if not (next_step is not None and self.r2_prefetch_steps > 0 and not next_step["noises"].is_cuda and
                next_step["noises"].shape[0] <= st.vb and not (st.train_te and self.eval_te is self.te)):
            return
        if self._sch_r2 is None:
            self._sch_r2 = copy.deepcopy(self.sch)
        nt, Sn = next_step.get("tokens_ori"), int(next_step["S"])
        k = min(self.r2_prefetch_steps, Sn)
        with torch.cuda.stream(st.side):
            nh = next_step["noises"].to(F32)
            nd = nh.to(self.device, non_blocking=False)
            ev_noise = torch.cuda.Event()
            ev_noise.record(st.side)
            r2n = {}
            g2n = self.rollout_steps(self.eval_unet, self.encode_pair(self.eval_te, nt), nd, Sn, r2n, sch=self._sch_r2)
            for _ in range(k):
                next(g2n, None)
        self._r2_pre = dict(gen=g2n, res=r2n, k=k, S=Sn, noises_host=nh.clone(), noises_dev=nd, ev_noise=ev_noise, tokens_ori=tuple(t.clone() for t in nt))

    def _classify_generated(self, st, images):
        """R1's images through face detection and classifier; the dynamic targets of the global batch (:1805-1837) are gathered now, solved underneath
        R2 and consumed by R3's loss.  Launch-stream order: classifier forward, logits read-back (host tail), targets, monitor."""
        h_g = self.classify_begin(images, record=st.share)
        ind, boxes, per = self._classify_read(h_g)
        self.start_dynamic_targets(per, st.B)
        st.out.update(images=images)
        if self._mon is not None:
            self._monitor_side("generated", images, h_g, tally=True)
        (st.rb if self.device_tail else st.out).update(probs=per[0]["probs"], preds=per[0]["preds"])
        return dict(images=images, ind=ind, boxes=boxes, per=per)

    def _r2_complete(self, st, images_ori, r2side):
        """What the loss needs of the frozen side, as one record.  ``r2side``: the forwards the concurrent R2 already enqueued on its stream; None
        (sequential R2): they are enqueued here, the feature encoders after the logits' read-back."""
        if r2side is not None:
            h_o, feats = r2side["h_o"], r2side
            ind_o, boxes_o, per_o = self._classify_read(h_o)
        else:
            h_o = self.classify_begin(images_ori)
            ind_o, boxes_o, per_o = self._classify_read(h_o)
            feats = self._ori_features(images_ori, ind_o, st.B)
        st.out.update(images_ori=images_ori)
        if self._mon is not None:
            self._monitor_side("ori", images_ori, h_o, tally=False)
        (st.rb if self.device_tail else st.out).update(preds_ori=per_o[0]["preds"], probs_ori=per_o[0]["probs"])
        return dict(images=images_ori, h=h_o, ind=ind_o, boxes=boxes_o, per=per_o, clip=feats.get("clip_ori"), dino=feats.get("dino_ori"), face=feats.get("face_ori"))

    def _targets(self, st, per):
        """Joins the dynamic targets' solve; [(targets, uncertainty)] per attribute, on the device (device tail) or on the host."""
        tgt = self.finish_dynamic_targets()
        if self.device_tail:
            st.rb.update(targets=tgt[0][0], uncertainty=tgt[0][1])
        else:
            st.out.update(targets=tgt[0][0], uncertainty=tgt[0][1], targets_by_attr={a["name"]: t for a, (t, _) in zip(per, tgt)})
        return tgt

    def _fair_loss(self, st, gen, tgt):
        """loss_fair and its logit gradient ``dlog_full`` [B, classes] fp32 -- device tail: one attribute, on the device; host tail: summed over
        the attributes (:1932; exp-3 :2146), on the host."""
        if self.device_tail:
            name, c0, k = self.attrs[0]
            lf, dl = FD.fair_loss_and_grad(gen["per"][0]["logits"], tgt[0][0], gen["per"][0]["ind_dev"], st.w_dev)
            dlog_full = torch.zeros((st.B, self.clf.num_classes), dtype=F32, device=self.device)
            dlog_full[:, c0:c0 + k] = dl
            st.rb["loss_fair"] = lf
            st.out.update(images_grad=gen["images"], N_backward=st.N_backward)
        else:
            loss_by_attr = {}
            dlog_full = torch.zeros((st.B, self.clf.num_classes), dtype=F32)
            for (name, c0, k), a, (t_a, _) in zip(self.attrs, gen["per"], tgt):
                loss_by_attr[name], dlog_full[:, c0:c0 + k] = fair_loss_and_grad(a["logits"], t_a, gen["ind"], st.w)
            st.out.update(loss_fair=loss_by_attr[self.attrs[0][0]], loss_fair_by_attr=loss_by_attr, images_grad=gen["images"], N_backward=st.N_backward)
        return dlog_full

    def _image_term(self, st, gen, ori, tgt):
        """Image-semantics term (:1904-1910, :1931-1932): w_i = (1/n_j) * weight_loss_img * dynamic_weight_i.  Returns its image gradient [B,3,H,W]."""
        args, dev, dv, out = self.args, self.device, self.device_tail, st.out
        images_g, targets, preds_o = gen["images"], tgt[0][0], ori["per"][0]["preds"]
        Himg, Wimg = images_g.shape[2], images_g.shape[3]
        small, fullbox = self.resize_small(images_g)
        e_c, e_d = self.image_features(small, record=True)
        self._fine("L_a_clip_dino_fwd_enqueued")
        tl, pl = [t for t, _ in tgt], [a["preds"] for a in ori["per"]]
        if dv:
            dyn = FD.dynamic_weights(gen["per"][0]["ind_dev"], targets, preds_o, self.factors1[0])
            wi = st.w_dev * args.weight_loss_img * dyn
        else:
            dyn = gen_dynamic_weights(gen["ind"], targets, preds_o, factor=self.factors1[0]) if len(tl) == 1 else \
                gen_dynamic_weights_multi(gen["ind"], tl, pl, self.factors1)
            wi = _h2d(st.w * args.weight_loss_img * dyn, dev)
        loss_clip, de_c = feature_loss_and_grad(e_c, ori["clip"], wi)
        loss_dino, de_d = feature_loss_and_grad(e_d, ori["dino"], wi)
        sc = _pow2_scale_dev(torch.stack([de_c.abs().max(), de_d.abs().max()]).float(), 1.0)      # both scales in one chain of launches
        dsmall, inv = _scaled_backward(self.clip.backward, de_c, sc[0])
        dsmall.mul_(inv)
        dd, inv = _scaled_backward(self.dino.backward, de_d, sc[1])
        dsmall.addcmul_(dd, inv)
        d_img = ops.crop_resize_bwd(dsmall, fullbox, st.B, Himg, Wimg, args.img_size_small)
        # apply_grad_hook_face (:1904, :1584-1617) acts on this path only: the classifier saw the un-hooked images
        if dv:       # the rectangle is a function of the two boxes (host); the factor of targets / original predictions (device)
            zt = torch.zeros(st.B, dtype=torch.long)
            rects, _ = face_grad_factors(gen["boxes"], ori["boxes"], zt, zt, 1.0, Himg, Wimg)
            has_box = _h2d(~(gen["boxes"] == -1).all(dim=1), dev)
            ops.rect_scale(d_img, _h2d(rects, dev), FD.hook_factors(has_box, targets, preds_o, self.factors2[0]))
            st.rb.update(loss_CLIP=loss_clip.float(), loss_DINO=loss_dino.float(), dynamic_weights=dyn)
        else:
            rects, facs = face_grad_factors(gen["boxes"], ori["boxes"], targets, preds_o, self.factors2[0], Himg, Wimg) if len(tl) == 1 else \
                face_grad_factors_multi(gen["boxes"], ori["boxes"], tl, pl, self.factors2, Himg, Wimg)
            ops.rect_scale(d_img, _h2d(rects, dev), _h2d(facs, dev))
            # (the per-image regulariser values are only reported: they are read back at the end of the step, not here)
            st.deferred.append(lambda lc=loss_clip, ld=loss_dino: out.update(
                loss_CLIP=lc.float().cpu(), loss_DINO=ld.float().cpu(), dynamic_weights=dyn,
                loss=sum(out["loss_fair_by_attr"].values()) + args.weight_loss_img * dyn * (lc.float().cpu() + ld.float().cpu())))
        self._fine("L_c_clip_dino_bwd_enqueued")
        return d_img

    def _face_term(self, st, gen, ori, tgt, d_img):
        """Face-realism term (:1917-1932): target = the original image's own face features when the target class equals the original prediction
        with confidence >= face_gender_confidence_level, else the nearest database face.  Adds its image gradient to ``d_img`` (None: a new one)."""
        args, dev, dv, out, B = self.args, self.device, self.device_tail, st.out, st.B
        images_g, ind_g, targets = gen["images"], gen["ind"], tgt[0][0]
        # exp-1 searches only for images with a target (:1926); the multi-attribute scripts search for every face (exp-3 :2135)
        if dv:
            # which faces carry a target is only known on the device: every face goes through the face network and the ones without a
            # target get weight 0 (same loss and gradient: their term is multiplied out; the reference skips them, :1926)
            ind_dev, per_o = gen["per"][0]["ind_dev"], ori["per"][0]
            from_ori = ind_dev & (targets != -1) & (targets == per_o["preds"]) & (per_o["probs"].max(dim=-1).values >= self.face_conf)
            has_d = ind_dev & (targets != -1)
            has = ind_g
            loss_face = torch.full((B,), -1.0, dtype=F32, device=dev)
        else:
            from_ori = ind_g.clone()
            for (t_a, _), a in zip(tgt, ori["per"]):
                from_ori &= (t_a != -1) & (t_a == a["preds"]) & (a["probs"].max(dim=-1).values >= self.face_conf)
            has = (ind_g & (targets != -1)) if len(tgt) == 1 else ind_g.clone()
            loss_face = torch.full((B,), -1.0)
        rows = has.nonzero().view(-1)
        if len(rows):
            chips_f, idx_f, A_f = self.aligned_faces(images_g, has)
            self._fine("L_c1_aligned_faces")
            feats, fctx = face_features(self.face_net, chips_f, record=True)
            self._fine("L_c2_sfnet_fwd_enqueued")
            near = self.nearest_face_feats(F.normalize(feats, dim=-1))
            rows_d = _h2d(rows, dev)
            use_ori = from_ori[rows_d] if dv else _h2d(from_ori[rows], dev)
            near = torch.where(use_ori[:, None], ori["face"][rows_d], near)
            wf = (st.w_dev[rows_d] * args.weight_loss_face * has_d[rows_d]) if dv else _h2d(st.w[rows] * args.weight_loss_face, dev)
            lf_rows, df = feature_loss_and_grad(feats, near, wf)
            self._fine("L_c3_nearest_and_loss_enqueued")
            if dv:
                loss_face[rows_d] = torch.where(has_d[rows_d], lf_rows.float(), torch.full_like(lf_rows, -1.0, dtype=F32))
            else:
                st.deferred.append(lambda: loss_face.__setitem__(rows, lf_rows.float().cpu()))
            dch, inv = _scaled_backward(partial(face_features_backward, self.face_net, fctx), df, _pow2_scale_dev(df.abs().max(), 1.0))
            dch.mul_(inv)
            self._fine("L_c5_sfnet_bwd_enqueued")
            if d_img is None:
                d_img = torch.zeros((B, 3, images_g.shape[2], images_g.shape[3]), dtype=F32, device=dev)
            ops.warp_affine_bwd(dch.contiguous(), idx_f, A_f, d_img, args.size_aligned_face)   # un-hooked images (:1901)
        if dv:
            st.rb["loss_face"] = loss_face
        else:
            st.deferred.append(lambda: out.update(loss_face=loss_face, loss=out.get("loss", sum(out["loss_fair_by_attr"].values())) + args.weight_loss_face * loss_face))
        self._fine("L_d_face_branch_done")
        return d_img

    def _classifier_backward(self, st, gen, dlog_full, d_img):
        """dlog_full through the classifier and the face crops back to the image, added to the regularisers' ``d_img``.  Returns dL/d(images), or None
        when no term has a gradient.  The classifier's recorded forward is consumed or dropped here."""
        dev, dv, B = self.device, self.device_tail, st.B
        sel = gen["ind"].nonzero().view(-1)
        # (device_tail: whether any logit gradient is non-zero is not known to the host -- the classifier backward runs whenever there is a face)
        if not (bool(len(sel)) and (dv or float(dlog_full.abs().sum()) > 0)):
            self.clf._ctx = None
            return d_img
        dlog = dlog_full[_h2d(sel, dev)] if dv else _h2d(dlog_full[sel], dev)
        dchips = self.clf.backward(dlog.contiguous(), self.clf_gscale)
        full = dchips
        if len(sel) != B:
            full = torch.zeros((B,) + tuple(dchips.shape[1:]), dtype=F32, device=dev)
            full[_h2d(sel, dev)] = dchips
        bx = gen["boxes"].clone()
        bx[~gen["ind"]] = 0
        d_fair = ops.crop_resize_bwd(full.contiguous(), _h2d(bx, dev), B, gen["images"].shape[2], gen["images"].shape[3], self.args.size_face)
        return d_fair if d_img is None else d_img.add_(d_fair)

    def _vae_backward(self, st, d_img):
        """dL/d(images) -> g = dL/dx_final [B,4,h,w] fp32, and the U-Net backward's scales: ``step_scale`` [S] (device) = hook (:1128) x scheduler
        recurrence (:1131) x the step's common power-of-two loss scale, whose inverse ``inv_gscale`` un-scales the LoRA gradients at the very end."""
        coefs, gs = self.sch.grad_coefs() * self.sch.chain_coefs(), self.args.guidance_scale
        dz, k = _scaled_backward(self.vae.backward_images, d_img, _pow2_scale_dev(d_img.abs().max(), 64.0), unscale=1.0 / self.vae.config.scaling_factor)
        g = dz * k
        # the U-Net backward's scale stays on the device too: the timesteps' upstream gradients are multiplied by (c_i * gscale) as device
        # scalars, the kernels run with gscale = 1 and the LoRA gradients are un-scaled ONCE, after the per-stream buffers have been summed
        gscale_dev = _pow2_scale_dev(g.abs().max() * (float(abs(coefs).max()) * max(abs(gs), abs(1 - gs))), 64.0)
        step_scale = _h2d(torch.as_tensor(coefs, dtype=F32), self.device) * gscale_dev
        st.out.update(g=g, coefs=coefs, gscale=1.0)
        return g, step_scale, 1.0 / gscale_dev

    def _unet_backward(self, st, gen, g, step_scale, inv_gscale):
        """The S per-timestep backwards are independent (the U-Net input is detached at every step, :1115): they are dealt round-robin to
        ``bwd_streams`` HIP streams, each side stream accumulating its LoRA gradients into its own buffer, so that the many launches which cannot
        fill the chip alone overlap with a neighbouring timestep's.  Then the prompt projections' and the text encoder's / prefix's backward."""
        S, gs, cur, ctxs, virtual = st.S, self.args.guidance_scale, st.cur, gen["ctxs"], self.bwd_virtual
        self.unet.prepare_backward()         # lazily built weight copies exist before any side stream can read them
        self.unet.prepare_backward_slots(S)   # per-timestep dK / dV pairs of the shared cross-attention K / V: no atomics, fixed-order sum
        nst = max(1, min(self.bwd_streams, S)) if self.concurrent_bwd else 1
        sides = [self._side_stream(k) for k in range(1, nst)]
        graveyard = [] if self.bwd_keep_alive else None
        # upstream gradient of the CFG pair eps = eps_u + gs (eps_c - eps_u): [(1 - gs) g ; gs g], built once; a timestep scales it.
        # Built on the launch stream BEFORE the side streams take their dependency on it: enqueued after ``wait_stream`` (as it was for
        # most of round 3) the side streams' first timesteps could read it while its ``cat`` was still running -- a race that showed
        # as a 4e-4 schedule-to-schedule gradient difference (once as NaN) whenever kernel timing shifted.
        gpair = torch.cat([g * (1.0 - gs), g * gs])
        for k, side in enumerate(sides, 1):
            for bank in self.banks:
                bank.grad_alt(k).zero_()
            side.wait_stream(cur)
        for i in range(S):
            k = i % nst
            on_side = k > 0
            side = sides[k - 1] if on_side else None
            with (torch.cuda.stream(side) if (on_side and not virtual) else contextlib.nullcontext()):
                if i in ctxs:
                    self.unet._ctx = ctxs.pop(i)        # activations kept from the forward rollout
                    if graveyard is not None:
                        graveyard.append(_all_tensors(self.unet._ctx))
                    if on_side and not virtual:
                        _record_stream(self.unet._ctx, side)
                else:                                   # gradient-checkpointed recompute of this timestep
                    self.unet.forward_step(ops.to_f16(gen["inputs"][i]), i, record=True, pair=True)
                for bank in self.banks:
                    bank.accum = bank.grad_alt(k) if on_side else bank.grad
                unet_mod.BWD_SLOT[0] = i
                self.unet.backward_step(gpair * step_scale[i], 1.0)
        unet_mod.BWD_SLOT[0] = None
        for bank in self.banks:
            bank.accum = bank.grad
        if self.debug_partials is not None:
            torch.cuda.synchronize()
            self.debug_partials.append([self.banks[0].grad.clone()] + [self.banks[0].grad_alt(k).clone() for k in range(1, nst)])
        for k, side in enumerate(sides, 1):
            cur.wait_stream(side)
            for bank in self.banks:
                bank.grad.add_(bank.grad_alt(k))
        graveyard = None
        denc = self.unet.finish_prompt_backward(1.0, need_denc=st.rec_te)
        if st.rec_te:
            dx0 = self.te.backward(denc.view(2, gen["enc"].shape[1], -1), 1.0)
            if st.train_prefix:     # the prefix vectors sit at positions 1..n of the PROMPT row (row 1; row 0 is the uncond sequence)
                self.prefix.bank.grad_view("token_embedding.weight")[1:].add_(dx0[1, 1:1 + self.prefix.n].float())
        for bank in self.banks:      # device-side loss scale: every bank's gradient of this step carries it exactly once
            bank.grad.mul_(inv_gscale)

    def _sync_and_report(self, st):
        """Gradient sync, guard and update; what the step reports about itself.  Device tail: everything in ``st.rb`` comes back in ONE read-back,
        taken together with the finite flag inside ``sync_and_update``, and the reported loss is assembled from it on the host."""
        args, out, rb, dv = self.args, st.out, st.rb, self.device_tail
        if dv:
            keys = sorted(rb)
            self._pending_readback = torch.cat([rb[k].reshape(-1).to(F32) for k in keys]) if keys else None
        out["grad_is_finite"] = self.sync_and_update(st.N_backward)
        if dv:
            host = self._readback_host if self._pending_readback is None else self._pending_readback.cpu()    # (a replaced sync_and_update: read here)
            self._pending_readback = None
            off = 0
            for k in keys:
                n = rb[k].numel()
                v = host[off:off + n].reshape(rb[k].shape)
                off += n
                out[k] = v.long() if rb[k].dtype == torch.long else v
            name = self.attrs[0][0]
            out.update(targets_by_attr={name: out["targets"]}, loss_fair_by_attr={name: out["loss_fair"]}, loss=out["loss_fair"].clone())
            if "loss_CLIP" in out:
                out["loss"] = out["loss"] + args.weight_loss_img * out["dynamic_weights"] * (out["loss_CLIP"] + out["loss_DINO"])
            if "loss_face" in out:
                out["loss"] = out["loss"] + args.weight_loss_face * out["loss_face"]
        if self._mon is not None:
            # behind the step's own read-back (``sync_and_update``), which has drained the stream the copies were queued on: no further wait
            self._mon.pop("event").synchronize()
            self.last_monitor, self._mon = self._mon, None

    def sync_and_update(self, N_backward, apply=True):
        args = self.args
        self.flag.zero_()
        self.allreduce_grads()
        for bank in self.banks:
            ops.grad_finite_scale(bank.grad, 1.0 / (self.world * N_backward), self.flag)
        pend, self._pending_readback = getattr(self, "_pending_readback", None), None
        if pend is not None:      # the step's reported values ride the flag's read-back: one device -> host copy per step
            host = torch.cat([self.flag.to(F32), pend]).cpu()
            finite, self._readback_host = int(host[0]) == 0, host[1:]
        else:
            finite = int(self.flag.item()) == 0  # checked after the all-reduce so every rank takes the same branch
        self.last_lr = args.learning_rate * lr_lambda(getattr(args, "lr_scheduler", "constant"), self.lr_step,
                                                      getattr(args, "lr_warmup_steps", 0), getattr(args, "max_train_steps", 1),
                                                      getattr(args, "lr_num_cycles", 1), getattr(args, "lr_power", 1.0), args.learning_rate)
        if apply:
            self.lr_step += 1
        plans = [bank.norm_plan() if self.log_norms else None for bank in self.banks]
        if finite and apply:
            self.opt_step += 1
            for bank, ema, plan in zip(self.banks, self.ema, plans):
                ops.adamw_ema(bank.flat, bank.grad, bank.exp_avg, bank.exp_avg_sq, bank.ema, self.last_lr, args.adam_beta1,
                              args.adam_beta2, args.adam_epsilon, args.adam_weight_decay, self.opt_step, ema.next_one_minus_decay(), norms=plan)
        elif self.log_norms:        # the reference logs the norms whether or not the optimiser stepped (:2034-2045): the reduction alone
            for bank, plan in zip(self.banks, plans):
                ops.adamw_ema(bank.flat, bank.grad, bank.exp_avg, bank.exp_avg_sq, bank.ema, self.last_lr, args.adam_beta1,
                              args.adam_beta2, args.adam_epsilon, args.adam_weight_decay, self.opt_step, 0.0, norms=plan, apply=False)
        if self.log_norms:
            ev = self._norms_to_host(plans)
        if finite and apply:
            if getattr(args, "train_unet", False):
                self.unet.refresh_lora()
            if getattr(args, "train_text_encoder", False):
                self.te.refresh_lora()
        if self.log_norms:          # behind everything this call enqueues: the host waits once, for the copy alone
            ev.synchronize()
            sizes = [p.out.numel() for p in plans]
            parts = self._norms_host.split(sizes)
            self.last_norms = {k: p.report(h.tolist()) for k, p, h in zip(self.bank_keys, plans, parts)}
        return finite

    def _norms_to_host(self, plans):
        """Every bank's ``NormPlan.out`` -> one pinned host buffer (kept), non-blocking copies on the current stream; returns the event behind them."""
        if self._norms_host is None:
            self._norms_host = torch.empty(sum(p.out.numel() for p in plans), dtype=F32, pin_memory=True)
        off = 0
        for p in plans:
            self._norms_host[off:off + p.out.numel()].copy_(p.out, non_blocking=True)
            off += p.out.numel()
        ev = torch.cuda.Event()
        ev.record()
        return ev
