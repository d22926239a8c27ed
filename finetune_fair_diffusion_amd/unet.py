"""MI355X-native mirror of diffusers ``UNet2DConditionModel`` + ``LoRAAttnProcessor`` for the
reference's call ``unet(latent_model_input, t, encoder_hidden_states=prompt_embeds).sample``
(exp-1-debias-gender/1-main-debias.py:1046-1050, :1118-1122; LoRA injection :798-818).

Execution model (not autograd): ``forward(..., record=True)`` keeps exactly the tensors the explicit
``backward`` needs; base weights are frozen so backward computes data gradients only, plus the
fp32 LoRA weight gradients, which are accumulated straight into the flat ``ParamBank.grad`` buffer.
Because the reference detaches the U-Net input at every denoising step (:1115) each timestep's
backward is independent given dL/d(eps_i) -- the training step (step.py) therefore re-runs this
forward per timestep with ``record=True`` (gradient-checkpointed recompute) and frees it again.

Workload structure exploited: cross-attention K/V depend only on the
prompt -> computed once per rollout for the 2 distinct sequences (uncond, cond) and shared by
every sample of that CFG half (``kv_div``); the 22 time-embedding projections depend only on t ->
one stacked GEMM per rollout for all S timesteps.
"""
import math

import torch

from . import ops
from .layers import (F16, F32, Conv3x3, Linear, LoRAPair, Norm, ParamBank, ResnetBlock, lora_linear_bwd, lora_linear_fwd)
from .weights import UNetConfig, unet_attn_names, unet_lora_param_shapes, unet_param_shapes


# Index of the timestep whose backward is being enqueued (host-side, set by the training step right before ``backward_step``): selects the
# per-timestep dK / dV slot of every cross-attention layer (``prepare_backward_slots``).  None outside a slotted backward.
BWD_SLOT = [None]


class _Out:
    def __init__(self, sample):
        self.sample = sample


class LoRAAttnProcessor:
    """Constructor-compatible stand-in for ``diffusers.models.attention_processor.LoRAAttnProcessor`` as the reference builds
    it (:811-815): carries the sizes only; the tensors live in the U-Net's flat ParamBank once ``set_attn_processor`` ran."""

    def __init__(self, hidden_size, cross_attention_dim=None, rank=4):
        self.hidden_size, self.cross_attention_dim, self.rank = hidden_size, cross_attention_dim, rank

    def to(self, *a, **k):
        return self


class AttnLoRA:
    """The four LoRALinearLayers of one LoRAAttnProcessor.  Self-attention (q, k, v project the same input): q, k, v run as ONE GEMM with stacked
    weights [3C, C]; their LoRA rank updates ride it as one second K-slab -- t = n1 . down_qkv^T [M, 3rp] against the block-diagonal up matrix
    [3C, 3rp] -- so the three pairs' 16-bit operand copies are views into four stacked buffers.  Cross-attention: k and v share ``down_kv16``."""

    def __init__(self, bank, name):
        self.q, self.k, self.v, self.out = (LoRAPair(bank, f"{name}.{p}_lora.down.weight", f"{name}.{p}_lora.up.weight")
                                            for p in ("to_q", "to_k", "to_v", "to_out"))
        dev = bank.flat.device
        rp = self.q.rp
        if self.q.K == self.k.K:
            C = self.q.N
            self.down_qkv16 = torch.zeros((3 * rp, C), dtype=F16, device=dev)                                  # [3rp, C]
            self.down_qkvT16 = torch.zeros((C, 3 * rp), dtype=F16, device=dev)                                 # [C, 3rp]
            self.up_qkv16 = torch.zeros((3 * C, 3 * rp), dtype=F16, device=dev)                                # block diagonal; off-diagonal blocks stay 0
            self.upT_qkv16 = torch.zeros((3 * rp, 3 * C), dtype=F16, device=dev)                               # [3rp, 3C]
            for i, p in enumerate((self.q, self.k, self.v)):
                p.place(self.down_qkv16[i * rp:(i + 1) * rp], self.down_qkvT16[:, i * rp:(i + 1) * rp],
                        self.up_qkv16[i * C:(i + 1) * C, i * rp:(i + 1) * rp], self.upT_qkv16[i * rp:(i + 1) * rp, i * C:(i + 1) * C])
            self.down_kv16 = self.down_qkv16[rp:]
        else:
            self.down_kv16 = torch.zeros((2 * rp, self.k.K), dtype=F16, device=dev)
            self.q.place()
            self.k.place(down16=self.down_kv16[:rp])
            self.v.place(down16=self.down_kv16[rp:])
        self.out.place()

    def pairs(self):
        return (self.q, self.k, self.v, self.out)

    def refresh(self):
        from .layers import refresh_pairs
        refresh_pairs(self.pairs())


class TransformerBlock:
    """Transformer2DModel with one BasicTransformerBlock (norm -> proj_in -> [LN, attn1, LN, attn2, LN, GEGLU-FF] -> proj_out)."""

    def __init__(self, sd, p, dev, C, heads, groups, xdim):
        self.C, self.heads, self.d, self.groups, self.xdim = C, heads, C // heads, groups, xdim
        self.p = p
        self.norm = Norm(sd, p + "norm", dev)
        self.proj_in = Linear(sd, p + "proj_in", dev, conv1x1=True)
        self.proj_out = Linear(sd, p + "proj_out", dev, conv1x1=True)
        b = p + "transformer_blocks.0."
        self.ln1, self.ln2, self.ln3 = Norm(sd, b + "norm1", dev), Norm(sd, b + "norm2", dev), Norm(sd, b + "norm3", dev)
        self.q1, self.k1, self.v1, self.o1 = (Linear(sd, b + "attn1." + n, dev) for n in ("to_q", "to_k", "to_v", "to_out.0"))
        assert self.q1.bias is None and self.k1.bias is None and self.v1.bias is None     # diffusers Attention: to_q/k/v have no bias
        self.wqkv = torch.cat([self.q1.w, self.k1.w, self.v1.w], 0).contiguous()            # [3C, C]: one GEMM, n1 is read once
        self._wqkvT = None
        self.q2, self.k2, self.v2, self.o2 = (Linear(sd, b + "attn2." + n, dev) for n in ("to_q", "to_k", "to_v", "to_out.0"))
        ff1, self.ff2 = Linear(sd, b + "ff.net.0.proj", dev), Linear(sd, b + "ff.net.2", dev)
        # GEGLU is fused into the FF1 projection: weights with (value_c, gate_c) rows adjacent; recording forwards also keep the
        # pre-gate projection (same interleaved order) for the backward
        self.ff1_wi, self.ff1_bi = ops.interleave_geglu(ff1.w, ff1.bias)
        self._ff1_wiT = None
        self.lora1 = self.lora2 = None  # AttnLoRA for attn1 / attn2
        self.name1, self.name2 = b + "attn1.processor", b + "attn2.processor"
        self.cross = None  # per-rollout cross-attention K/V cache
        self.lean = False  # recording forwards keep neither the pre-gate FF projection nor n1 / n2 (UNet2DConditionModel.lean_record; recomputed in the backward)

    # -- cross-attention K/V for the rollout's prompt embeddings (timestep invariant) ------------
    def prepare_cross(self, enc, Bk, L, record, static=False):
        """enc: [Bk*L, xdim] fp16.  Caches K, V [Bk*L,C]."""
        lo = self.lora2
        te = ops.gemm(enc, lo.down_kv16) if lo is not None else None
        rp = lo.k.rp if lo is not None else 0
        old = None
        if lo is not None:
            K = ops.gemm(enc, self.k2.w, a2=te[:, :rp], b2=lo.k.up16)
            V = ops.gemm(enc, self.v2.w, a2=te[:, rp:], b2=lo.v.up16)
        elif static:      # a captured forward (GraphedForward) holds the ADDRESSES of K / V: rewritten in place for every rollout
            old = self.cross if (self.cross is not None and self.cross.get("static") and self.cross["K"].shape == (Bk * L, self.C)) else None
            K = ops.gemm(enc, self.k2.w, out=old["K"] if old else None)
            V = ops.gemm(enc, self.v2.w, out=old["V"] if old else None)
            if old is None:   # new buffers (first rollout, or another prompt shape): graphs captured against the old addresses must not be replayed
                self.static_generation = getattr(self, "static_generation", 0) + 1
        else:
            K, V = ops.gemm(enc, self.k2.w), ops.gemm(enc, self.v2.w)
        self.cross = dict(static=bool(static and lo is None), K=K, V=V, Bk=Bk, L=L, enc=enc, te=te)
        if ops.cross_shape_ok(self.C, self.heads, L):
            # the one-launch cross-attention sub-block (ops.cross_attn_block) reads V transposed, keys zero-padded to 80: made once per rollout; a captured
            # forward holds its address like K's and V's
            self.cross["Vt80"] = ops.transpose_btc(V, Bk, L, self.C, ops.CROSS_LP, out=old.get("Vt80") if (static and old) else None)
        if record:
            self.cross["dK"] = torch.zeros((Bk * L, self.C), dtype=F32, device=enc.device)
            self.cross["dV"] = torch.zeros((Bk * L, self.C), dtype=F32, device=enc.device)

    def finish_cross_backward(self, gscale, need_denc):
        """Backward of prepare_cross from the accumulated (over steps and samples) dK/dV."""
        c, lo = self.cross, self.lora2
        if c.get("slots") is not None:      # per-timestep slots (deterministic form): summed here in timestep order, plus whatever the atomics form added
            c["dK"] += c["slots"][:, 0].sum(dim=0)
            c["dV"] += c["slots"][:, 1].sum(dim=0)
            c["slots"] = None
        dK, dV = ops.to_f16(c["dK"]), ops.to_f16(c["dV"])
        rp = lo.k.rp if lo is not None else 0
        te = c["te"]
        denc = lora_linear_bwd(dK, c["enc"], te[:, :rp] if te is not None else None, self.k2, lo.k if lo else None, gscale, need_dx=need_denc)
        denc = lora_linear_bwd(dV, c["enc"], te[:, rp:] if te is not None else None, self.v2, lo.v if lo else None, gscale, residual=denc,
                               need_dx=need_denc)
        return denc

    # -- forward -------------------------------------------------------------------------------
    def forward(self, x, B, H, W, ctx=None, pair=False):
        """x [B*HW, C].  ``pair``: x holds the N = B latents of a CFG pair whose two halves differ only in the prompt, and this is the
        first cross-attention of the U-Net: everything up to the cross-attention query (norm, proj_in, self-attention, attn2.to_q) is
        identical for the uncond and the cond half, is computed once on N samples and duplicated; returns the 2N-sample output."""
        HW, C, h, d = H * W, self.C, self.heads, self.d
        rec = ctx is not None
        g, st = ops.groupnorm(x, None, B, HW, self.groups, 1e-6, self.norm.gamma, self.norm.beta, False)
        # the three LayerNorms are their own launches behind the GEMM that produces their input (ops.gemm(..., ln=...) returns y, LayerNorm(y) and the 8 B per row
        # of statistics the backward keeps; the second-output GEMM epilogue of round 4 lost in situ and lives in scratch/ since round 5)
        h0, n1, ln1 = ops.gemm(g, self.proj_in.w, bias=self.proj_in.bias, ln=(self.ln1.gamma, self.ln1.beta, 1e-5))
        l1 = self.lora1
        # q leaves its projection multiplied by d^-0.5 * log2(e) where the attention kernels can take it that way (ops.q_prescale)
        qs = ops.q_prescale(d)
        csq = (qs, C) if qs is not None else None
        if l1 is not None:
            t1 = ops.gemm(n1, l1.down_qkv16)
            qkv = ops.gemm(n1, self.wqkv, a2=t1, b2=l1.up_qkv16, colscale=csq)
        else:
            t1 = None
            qkv = ops.gemm(n1, self.wqkv, colscale=csq)
        q, k, v = qkv[:, :C], qkv[:, C:2 * C], qkv[:, 2 * C:]           # column slices (row stride 3C): the attention kernels take strides
        o, lse = ops.attn_fwd(q, k, v, B, h, HW, HW, d, 1, need_lse=True, prescaled=qs is not None)
        l2 = self.lora2
        cr = self.cross
        if (not pair and cr.get("Vt80") is not None and self.q2.bias is None and self.o2.bias is not None
                and ops.cross_block_ok(B * HW, C, h, cr["L"], HW, l2.q.rp if l2 is not None else 0)):
            # norm2 -> attn2 (with its LoRA slabs) -> residual -> norm3 is ONE launch (csrc/crossattn.hip); a forward that does not record never sees n2, q2, o2 in
            # HBM, a recording one gets them written once for the backward
            h1, to1 = lora_linear_fwd(o, self.o1, l1.out if l1 else None, residual=h0)
            qs2 = ops.q_prescale(d)
            h2, n3, ln3, r = ops.cross_attn_block(h1, (self.ln2.gamma, self.ln2.beta, 1e-5), self.q2.w, cr["K"], cr["Vt80"], cr["L"], self.o2.w, self.o2.bias,
                                                  (self.ln3.gamma, self.ln3.beta, 1e-5), h, HW, B // cr["Bk"], lora_q=l2.q if l2 else None,
                                                  lora_o=l2.out if l2 else None, record=rec, q_prescaled=qs2 is not None)
            lean = rec and self.lean
            proj = torch.empty((n3.shape[0], self.ff1_wi.shape[0]), dtype=F16, device=n3.device) if rec and not lean else None
            gg = ops.gemm(n3, self.ff1_wi, bias=self.ff1_bi, act="geglu", aux=proj)
            h3 = ops.gemm(gg, self.ff2.w, bias=self.ff2.bias, residual=h2)
            out = ops.gemm(h3, self.proj_out.w, bias=self.proj_out.bias, residual=x, gn_stats=True)
            if rec:
                ctx.append(dict(x=x, st=st, h0=h0, ln1=ln1, n1=None if lean else n1, t1=t1, qkv=qkv, o=o, lse=lse, to1=to1, h1=h1, ln2=r["ln2"], n2=None if lean else r["n2"], tq2=r["tq2"], q2=r["q2"],
                                o2=r["o2"], lse2=r["lse2"], to2=r["to2"], h2=h2, ln3=ln3, proj=proj, pair=False, qs=qs is not None, qs2=qs2 is not None))
            return out
        (h1, n2, ln2), to1 = lora_linear_fwd(o, self.o1, l1.out if l1 else None, residual=h0, ln=(self.ln2.gamma, self.ln2.beta, 1e-5))
        qs2 = ops.q_prescale(d)
        q2, tq2 = lora_linear_fwd(n2, self.q2, l2.q if l2 else None, colscale=(qs2, C) if qs2 is not None else None)
        B2 = 2 * B if pair else B
        q2f, h1f, xf = (torch.cat([q2, q2]), torch.cat([h1, h1]), torch.cat([x, x])) if pair else (q2, h1, x)
        kv_div = B2 // cr["Bk"]
        o2, lse2 = ops.attn_fwd(q2f, cr["K"], cr["V"], B2, h, HW, cr["L"], d, kv_div, need_lse=True, prescaled=qs2 is not None)
        (h2, n3, ln3), to2 = lora_linear_fwd(o2, self.o2, l2.out if l2 else None, residual=h1f, ln=(self.ln3.gamma, self.ln3.beta, 1e-5))
        # bit-identical to projection + fd_geglu_fwd (both halves are rounded to fp16 before the gate)
        lean = rec and self.lean
        proj = torch.empty((n3.shape[0], self.ff1_wi.shape[0]), dtype=F16, device=n3.device) if rec and not lean else None
        gg = ops.gemm(n3, self.ff1_wi, bias=self.ff1_bi, act="geglu", aux=proj)
        h3 = ops.gemm(gg, self.ff2.w, bias=self.ff2.bias, residual=h2)
        out = ops.gemm(h3, self.proj_out.w, bias=self.proj_out.bias, residual=xf, gn_stats=True)      # feeds the next ResnetBlock's norm1 / conv_norm_out
        if rec:
            ctx.append(dict(x=x, st=st, h0=h0, ln1=ln1, n1=None if lean else n1, t1=t1, qkv=qkv, o=o, lse=lse, to1=to1, h1=h1, ln2=ln2, n2=None if lean else n2,
                            tq2=tq2, q2=q2f, o2=o2, lse2=lse2, to2=to2, h2=h2, ln3=ln3, proj=proj, pair=pair, qs=qs is not None, qs2=qs2 is not None))
        return out

    # -- backward ------------------------------------------------------------------------------
    def backward(self, d_out, B, H, W, c, gscale, need_dx=True):
        """d_out [B*HW, C] (B counts both halves of a paired forward).  ``need_dx=False``: nothing trainable upstream (first attention
        of the U-Net), the gradient w.r.t. the block input is not formed.  The block's 16 LoRA weight gradients are queued and run as
        one batched launch pair at the end (``ops.wgrad_batch``)."""
        with ops.wgrad_batch():
            return self._backward(d_out, B, H, W, c, gscale, need_dx)

    def _backward(self, d_out, B, H, W, c, gscale, need_dx=True):
        HW, C, h, d = H * W, self.C, self.heads, self.d
        l1, l2 = self.lora1, self.lora2
        pair = c.get("pair", False)
        dh3 = ops.gemm(d_out, self.proj_out.wT)
        dgg = ops.gemm(dh3, self.ff2.wT)
        proj = c["proj"]
        if proj is None:
            # lean recording (round 6): the 8C-wide pre-gate projection -- 40 % of a transformer block's recorded bytes -- and the LayerNorm outputs n1 / n2
            # (needed only by LoRA weight gradients) were not kept: recomputed here from the kept residual streams h2 / h0 / h1 by the SAME kernels the forward
            # ran (LayerNorm, then the FF1 projection without its gate epilogue: same tile, same k order), hence bit-identical operands and gradients.
            # Without split-K: the GEGLU launch never splits, while the bare projection would at C = 1280 up to 256 rows (another kernel, another k order)
            proj = ops.gemm(ops.layernorm(c["h2"], self.ln3.gamma, self.ln3.beta, 1e-5), self.ff1_wi, bias=self.ff1_bi, split_k=False)
        dproj = ops.geglu_bwd_interleaved(proj, dgg)
        del proj
        if self._ff1_wiT is None:
            self._ff1_wiT = self.ff1_wi.t().contiguous()
        dn3 = ops.gemm(dproj, self._ff1_wiT)
        dh2 = ops.layernorm_bwd(c["h2"], dn3, self.ln3.gamma, c["ln3"], add=dh3)
        # attn2 (cross)
        do2 = lora_linear_bwd(dh2, c["o2"], c["to2"], self.o2, l2.out if l2 else None, gscale)
        cr = self.cross
        kv_div = B // cr["Bk"]
        # dK/dV of every sample and every timestep add into ONE fp32 accumulator pair with atomics (also at kv_div == 1: the timesteps'
        # backwards run on several HIP streams, step.py, and a plain read-modify-write of the shared buffer would lose updates)
        slot = BWD_SLOT[0] if cr.get("slots") is not None else None
        if slot is not None:     # this timestep's own fp32 dK / dV pair, written without atomics (bit-reproducible; ops.attn_bwd)
            dq2, _, _ = ops.attn_bwd(c["q2"], cr["K"], cr["V"], c["o2"], do2, c["lse2"], B, h, HW, cr["L"], d, kv_div,
                                     dk_out=cr["slots"][slot, 0], dv_out=cr["slots"][slot, 1], prescaled=c.get("qs2", False))
        else:
            dq2, _, _ = ops.attn_bwd(c["q2"], cr["K"], cr["V"], c["o2"], do2, c["lse2"], B, h, HW, cr["L"], d, kv_div,
                                     dk_acc=cr["dK"], dv_acc=cr["dV"], prescaled=c.get("qs2", False))
        if pair:
            # the shared prefix received the gradient of both halves
            B = B // 2
            M = B * HW
            dq2 = ops.add(dq2[:M], dq2[M:])
            dh2 = ops.add(dh2[:M], dh2[M:])
            if need_dx:
                d_out = ops.add(d_out[:M], d_out[M:])
        n2 = c["n2"] if (c["n2"] is not None or l2 is None) else ops.layernorm(c["h1"], self.ln2.gamma, self.ln2.beta, 1e-5)
        dn2 = lora_linear_bwd(dq2, n2, c["tq2"], self.q2, l2.q if l2 else None, gscale)
        dh1 = ops.layernorm_bwd(c["h1"], dn2, self.ln2.gamma, c["ln2"], add=dh2)
        # attn1 (self)
        do1 = lora_linear_bwd(dh1, c["o"], c["to1"], self.o1, l1.out if l1 else None, gscale)
        qkv = c["qkv"]
        dqkv = torch.empty_like(qkv)                                    # dq | dk | dv as column slices: one dgrad GEMM over K = 3C
        ops.attn_bwd(qkv[:, :C], qkv[:, C:2 * C], qkv[:, 2 * C:], c["o"], do1, c["lse"], B, h, HW, HW, d, 1, dqkv=dqkv, prescaled=c.get("qs", False))
        if self._wqkvT is None:
            self._wqkvT = self.wqkv.t().contiguous()                    # [C, 3C]
        if l1 is not None:
            t1, rp = c["t1"], l1.q.rp
            n1 = c["n1"] if c["n1"] is not None else ops.layernorm(c["h0"], self.ln1.gamma, self.ln1.beta, 1e-5)
            u = ops.gemm(dqkv, l1.upT_qkv16)                             # [M, 3rp] = (dq up_q | dk up_k | dv up_v)
            for i, pair in enumerate((l1.q, l1.k, l1.v)):
                gd, gu = pair.grads()
                ops.lora_wgrad(dqkv[:, i * C:(i + 1) * C], t1[:, i * rp:(i + 1) * rp], gu, pair.r, 1, pair.r, scale=1.0 / gscale)   # d up = dy^T t
                ops.lora_wgrad(n1, u[:, i * rp:(i + 1) * rp], gd, 1, pair.K, pair.r, scale=1.0 / gscale)                           # d down = u^T n1
            dn1 = ops.gemm(dqkv, self._wqkvT, a2=u, b2=l1.down_qkvT16) if need_dx else None
        else:
            dn1 = ops.gemm(dqkv, self._wqkvT) if need_dx else None
        if not need_dx:
            return None
        dh0 = ops.layernorm_bwd(c["h0"], dn1, self.ln1.gamma, c["ln1"], add=dh1)
        dg = ops.gemm(dh0, self.proj_in.wT)
        dx, _ = ops.groupnorm_bwd(c["x"], None, dg, B, HW, self.groups, c["st"], self.norm.gamma, self.norm.beta, False, add1=d_out)
        return dx


class UNet2DConditionModel:
    def __init__(self, cfg: UNetConfig, state_dict, device):
        self.config, self.device = cfg, device
        shapes = unet_param_shapes(cfg)
        missing = [k for k in shapes if k not in state_dict]
        if missing:
            raise KeyError(f"UNet state_dict is missing {len(missing)} tensors, e.g. {missing[:3]}")
        sd, dev = state_dict, device
        boc, g, heads, xdim, n = cfg.block_out_channels, cfg.norm_num_groups, cfg.attention_head_dim, cfg.cross_attention_dim, cfg.layers_per_block
        self.temb_dim = boc[0] * 4
        w = sd["conv_in.weight"].to(dev, F32)
        self.conv_in_w = w.permute(2, 3, 1, 0).reshape(9 * cfg.in_channels, boc[0]).contiguous()
        self.conv_in_b = sd["conv_in.bias"].to(dev, F32).contiguous()
        self.time1, self.time2 = Linear(sd, "time_embedding.linear_1", dev), Linear(sd, "time_embedding.linear_2", dev)
        self.resnets, self.transformers = [], []

        def res(p):
            r = ResnetBlock(sd, p, dev, g, 1e-5)
            self.resnets.append(r)
            return r

        def tr(p, c):
            t = TransformerBlock(sd, p, dev, c, heads, g, xdim)
            self.transformers.append(t)
            return t

        self.down = []
        cout = boc[0]
        for i, t in enumerate(cfg.down_block_types):
            cout = boc[i]
            blk = dict(res=[res(f"down_blocks.{i}.resnets.{j}.") for j in range(n)],
                       attn=[tr(f"down_blocks.{i}.attentions.{j}.", cout) for j in range(n)] if t.startswith("CrossAttn") else None,
                       down=Conv3x3(sd, f"down_blocks.{i}.downsamplers.0.conv", dev) if i != len(boc) - 1 else None)
            self.down.append(blk)
        c = boc[-1]
        self.mid = dict(res=[res("mid_block.resnets.0."), res("mid_block.resnets.1.")], attn=[tr("mid_block.attentions.0.", c)])
        self.up = []
        rev = list(reversed(boc))
        for i, t in enumerate(cfg.up_block_types):
            cout = rev[i]
            blk = dict(res=[res(f"up_blocks.{i}.resnets.{j}.") for j in range(n + 1)],
                       attn=[tr(f"up_blocks.{i}.attentions.{j}.", cout) for j in range(n + 1)] if t.startswith("CrossAttn") else None,
                       up=Conv3x3(sd, f"up_blocks.{i}.upsamplers.0.conv", dev) if i != len(boc) - 1 else None)
            self.up.append(blk)
        self.norm_out = Norm(sd, "conv_norm_out", dev)
        self.conv_out = Conv3x3(sd, "conv_out", dev)
        wo = sd["conv_out.weight"].to(dev, F32)  # data-gradient as a small-Cin direct conv: [k*k*Cout_as_in, Cin_as_out]
        self.conv_out_wd = wo.flip(2, 3).permute(2, 3, 0, 1).reshape(9 * cfg.out_channels, boc[0]).contiguous()
        # stacked time-embedding projections of all resnets: one GEMM per rollout
        ws, bs, off = [], [], 0
        for r in self.resnets:
            ws.append(r.temb_w.to(dev, F16))
            bs.append(r.temb_b.to(dev, F32))
            r.temb_slice = (off, off + ws[-1].shape[0])
            off += ws[-1].shape[0]
        self.temb_proj_w = torch.cat(ws, 0).contiguous()
        self.temb_proj_b = torch.cat(bs, 0).contiguous()
        self.lora_bank = None
        self._tr_by_name = {}
        for t in self.transformers:
            self._tr_by_name[t.name1] = (t, 1)
            self._tr_by_name[t.name2] = (t, 2)
        self.temb_table = None
        self._ctx = None

    # ------------------------------------------------------------------ diffusers-compatible surface
    @property
    def attn_processors(self):
        return {n: (getattr(self._tr_by_name[n][0], f"lora{self._tr_by_name[n][1]}")) for n in unet_attn_names(self.config)}

    def set_attn_processor(self, processors):
        """``unet.set_attn_processor(unet_lora_procs)`` (:818, gen-images.py:517): a dict name -> ``LoRAAttnProcessor``
        (any object with ``hidden_size``, ``cross_attention_dim`` and ``rank``) for all 32 attention layers."""
        names = unet_attn_names(self.config)
        if set(processors) != set(names):
            raise ValueError(f"expected {len(names)} attention processors, got {len(processors)} with different names")
        ranks = {p.rank for p in processors.values()}
        if len(ranks) != 1:
            raise ValueError(f"all LoRA processors must share one rank, got {sorted(ranks)}")
        shapes = unet_lora_param_shapes(self.config, ranks.pop())
        for n, p in processors.items():
            cin = shapes[n + ".to_k_lora.down.weight"][1]
            hid = shapes[n + ".to_q_lora.down.weight"][1]
            if p.hidden_size != hid or (p.cross_attention_dim or hid) != cin:
                raise ValueError(f"{n}: processor sizes ({p.hidden_size}, {p.cross_attention_dim}) do not match the U-Net ({hid}, {cin})")
        return self.add_lora(next(iter(processors.values())).rank, seed=getattr(next(iter(processors.values())), "seed", 0))

    @property
    def dtype(self):
        return F16

    def to(self, *a, **k):
        return self

    def enable_gradient_checkpointing(self):  # nothing to enable: activations are kept in HBM or recomputed per timestep by the step
        return None

    def train(self, mode=True):
        return self

    def eval(self):
        return self

    def requires_grad_(self, flag=False):
        return self

    def add_lora(self, rank, state_dict=None, seed=0):
        """Create the 32 LoRAAttnProcessors (rank r) in one flat fp32 ParamBank (:798-818)."""
        shapes = unet_lora_param_shapes(self.config, rank)
        self.lora_bank = ParamBank(shapes, self.device)
        if state_dict is None:
            from .weights import synthetic_state_dict
            state_dict = synthetic_state_dict(shapes, seed=seed)
        self.lora_bank.load_state_dict(state_dict)
        for name, (t, which) in self._tr_by_name.items():
            setattr(t, f"lora{which}", AttnLoRA(self.lora_bank, name))
        self.refresh_lora()
        return self.lora_bank

    def refresh_lora(self, ema=False):
        from .layers import refresh_pairs
        refresh_pairs([p for t in self.transformers for lo in (t.lora1, t.lora2) if lo is not None for p in lo.pairs()], ema=ema)

    @property
    def lean_record(self):
        return self.transformers[0].lean

    @lean_record.setter
    def lean_record(self, flag):
        """Recording forwards keep 10 C instead of 20 C values per token of a transformer block (no pre-gate FF projection, no n1 / n2); the backward recomputes
        them (TransformerBlock._backward).  The training step switches it on when the rollout's activations do not all fit in HBM (step.FairnessTrainer)."""
        for t in self.transformers:
            t.lean = bool(flag)

    def prepare_backward(self):
        """Materialise every lazily built backward operand (transposed / flipped weight copies) NOW, on the current stream.  The training
        step deals the per-timestep backwards to several HIP streams; built lazily, a copy created by the first timestep on one stream
        could be read by the next timestep on another stream before its transpose kernel has run."""
        if getattr(self, "_bwd_ready", False):
            return
        for r in self.resnets:
            r.conv1.wd, r.conv2.wd
            if r.shortcut is not None:
                r.shortcut.wT
        for t in self.transformers:
            for lin in (t.proj_in, t.proj_out, t.o1, t.q2, t.k2, t.v2, t.o2, t.ff2):
                lin.wT
            if t._ff1_wiT is None:
                t._ff1_wiT = t.ff1_wi.t().contiguous()
            if t._wqkvT is None:
                t._wqkvT = t.wqkv.t().contiguous()
        for blk in self.down:
            if blk["down"] is not None:
                blk["down"].wd
        for blk in self.up:
            if blk["up"] is not None:
                blk["up"].wd, blk["up"].wd_up2p
        self._bwd_ready = True

    def prepare_backward_slots(self, S):
        """One fp32 (dK, dV) pair per timestep and cross-attention layer, zero-initialised on the CURRENT stream before the backward streams
        fork: each timestep's backward writes only its own pair (no atomics), ``finish_prompt_backward`` sums them in timestep order.
        2 x S x 154 x C floats per layer -- 250 MB over the 16 layers at S = 20."""
        for t in self.transformers:
            cr = t.cross
            if cr is not None and "dK" in cr:
                cr["slots"] = torch.zeros((S, 2) + tuple(cr["dK"].shape), dtype=F32, device=cr["dK"].device)

    def load_state_dict(self, sd, strict=False):
        """LoRA tensors by diffusers key (gen-images.py:520-521 calls exactly this with strict=False)."""
        if self.lora_bank is not None:
            self.lora_bank.load_state_dict(sd, strict=strict)
            self.refresh_lora()

    # ------------------------------------------------------------------ per-rollout preparation
    def prepare_timesteps(self, timesteps):
        """temb table [S, sum(Cout)] for all S timesteps: sinusoid -> MLP -> SiLU -> 22 stacked projections."""
        c0 = self.config.block_out_channels[0]
        half = c0 // 2
        t = torch.as_tensor(timesteps, dtype=F32).reshape(-1, 1)
        freq = torch.exp(-math.log(10000.0) * torch.arange(half, dtype=F32) / half)[None]
        emb = torch.cat([torch.cos(t * freq), torch.sin(t * freq)], -1).to(F16).to(self.device)  # flip_sin_to_cos, cast to wd
        h = ops.gemm(emb, self.time1.w, bias=self.time1.bias, act="silu")
        temb = ops.gemm(h, self.time2.w, bias=self.time2.bias, act="silu")  # SiLU(temb) feeds every time_emb_proj
        self.temb_table = ops.gemm(temb, self.temb_proj_w, bias=self.temb_proj_b)
        self.timesteps = [int(v) for v in torch.as_tensor(timesteps).reshape(-1).tolist()]

    def prepare_prompt(self, enc, record=False):
        """enc: [Bk, L, xdim] fp16 (Bk = 2 for the shared CFG pair, or 2N for per-sample embeddings)."""
        Bk, L, X = enc.shape
        e2 = enc.reshape(Bk * L, X).to(F16).contiguous()
        static = getattr(self, "graphed", None) is not None and not record
        for t in self.transformers:
            t.prepare_cross(e2, Bk, L, record, static=static)

    def finish_prompt_backward(self, gscale, need_denc=False):
        denc = None
        for t in self.transformers:
            d = t.finish_cross_backward(gscale, need_denc)
            if need_denc:
                denc = d if denc is None else ops.add(denc, d)
        return denc

    # ------------------------------------------------------------------ forward / backward
    def forward_step(self, sample, step_index, record=False, pair=False, trow=None):
        """sample: [B,4,H,W] NCHW (fp32 or fp16; cast to wd as the reference does :1043).
        Returns eps [B,4,H*W] fp32 (values are fp16-rounded, then upcast like :1051).
        ``pair``: sample holds the N latents of a CFG rollout step, standing for the batch ``cat([sample, sample])`` (:1043) whose halves
        meet different prompt embeddings only at the first cross-attention; conv_in, the first ResnetBlock and that transformer's
        self-attention are evaluated once on N samples (bit-identical to evaluating them twice).  Returns eps for the 2N batch."""
        cfg = self.config
        B, Cin, H, W = sample.shape
        pair = pair and self.down[0]["attn"] is not None
        boc = cfg.block_out_channels
        if trow is None:
            trow = self.temb_table[step_index:step_index + 1]
        ctx = [] if record else None

        def temb(r):
            a, b = r.temb_slice
            return trow[:, a:b]

        x16 = sample if sample.dtype == F16 else ops.to_f16(sample.contiguous())
        x, _, _ = ops.conv_small_cin(x16.contiguous(), self.conv_in_w, self.conv_in_b, B, H, W, Cin, boc[0], 3, 1, nchw=True)
        skips = [(torch.cat([x, x]) if pair else x, H, W)]
        for blk in self.down:
            for j, r in enumerate(blk["res"]):
                x = r.forward(x, None, B, H, W, temb(r), ctx)
                if blk["attn"] is not None:
                    x = blk["attn"][j].forward(x, B, H, W, ctx, pair=pair)
                    if pair:
                        pair, B = False, 2 * B
                skips.append((x, H, W))
            if blk["down"] is not None:
                x, H, W = ops.conv3x3(x, blk["down"].wk, B, H, W, mode=ops.CONV_STRIDE2, bias=blk["down"].bias, gn_stats=True)
                skips.append((x, H, W))
        x = self.mid["res"][0].forward(x, None, B, H, W, temb(self.mid["res"][0]), ctx)
        x = self.mid["attn"][0].forward(x, B, H, W, ctx)
        x = self.mid["res"][1].forward(x, None, B, H, W, temb(self.mid["res"][1]), ctx)
        for blk in self.up:
            for j, r in enumerate(blk["res"]):
                s, _, _ = skips.pop()
                x = r.forward(x, s, B, H, W, temb(r), ctx)
                if blk["attn"] is not None:
                    x = blk["attn"][j].forward(x, B, H, W, ctx)
            if blk["up"] is not None:
                x, H, W = ops.conv_up2(x, blk["up"], B, H, W)
        g, st = ops.groupnorm(x, None, B, H * W, cfg.norm_num_groups, 1e-5, self.norm_out.gamma, self.norm_out.beta, True)
        y, _, _ = ops.conv3x3(g, self.conv_out.wk, B, H, W, bias=self.conv_out.bias)
        eps = ops.nhwc_to_nchw(y, B, H * W, cfg.out_channels, out_dtype=F32)
        if record:
            self._ctx = dict(blocks=ctx, x_out=x, st_out=st, B=B, H=H, W=W)
        return eps

    def backward_step(self, d_eps, gscale):
        """d_eps: [B,4,H,W] fp32 = gscale * dL/d(eps).  Accumulates LoRA grads; returns nothing
        (the U-Net input is detached in the reference, so no gradient flows to the latents)."""
        cfg, c = self.config, self._ctx
        B, H, W = c["B"], c["H"], c["W"]
        boc = cfg.block_out_channels
        blocks = c["blocks"]
        dg, _, _ = ops.conv_small_cin(d_eps.contiguous(), self.conv_out_wd, None, B, H, W, cfg.out_channels, boc[0], 3, 1, nchw=True)
        dx, _ = ops.groupnorm_bwd(c["x_out"], None, dg, B, H * W, cfg.norm_num_groups, c["st_out"], self.norm_out.gamma, self.norm_out.beta, True)
        dskips = []
        # up blocks, reversed
        for bi in range(len(self.up) - 1, -1, -1):
            blk = self.up[bi]
            if blk["up"] is not None:
                H, W = H // 2, W // 2
                dx = ops.conv_up2_bwd(dx, blk["up"], B, H, W)
            for j in range(len(blk["res"]) - 1, -1, -1):
                if blk["attn"] is not None:
                    dx = blk["attn"][j].backward(dx, B, H, W, blocks.pop(), gscale)
                dx, dsk = blk["res"][j].backward(dx, B, H, W, blocks.pop())
                dskips.append(dsk)
        # mid
        dx, _ = self.mid["res"][1].backward(dx, B, H, W, blocks.pop())
        dx = self.mid["attn"][0].backward(dx, B, H, W, blocks.pop(), gscale)
        dx, _ = self.mid["res"][0].backward(dx, B, H, W, blocks.pop())
        # down blocks, reversed: every forward output that was pushed as a skip gets its skip-gradient added.
        # The up path popped skips last-in-first-out and we walked it backwards, so dskips[k] already pairs
        # with forward skip index k (skip 0 = conv_in output).
        first_attn = next(i for i, b in enumerate(self.down) if b["attn"] is not None)
        k = len(dskips) - 1
        done = False
        for bi in range(len(self.down) - 1, -1, -1):
            blk = self.down[bi]
            if blk["down"] is not None:
                dx = ops.add(dx, dskips[k]); k -= 1
                dx, H, W = ops.conv3x3(dx, blk["down"].wd, B, H, W, mode=ops.CONV_TRANS2)
            for j in range(len(blk["res"]) - 1, -1, -1):
                dx = ops.add(dx, dskips[k]); k -= 1
                last = (bi == first_attn and j == 0)
                if blk["attn"] is not None:
                    dx = blk["attn"][j].backward(dx, B, H, W, blocks.pop(), gscale, need_dx=not last)
                if last:
                    done = True  # nothing trainable upstream of the first attention: stop here
                    break
                dx, _ = blk["res"][j].backward(dx, B, H, W, blocks.pop())
            if done:
                break
        self._ctx = None

    # ------------------------------------------------------------------ drop-in call
    def __call__(self, sample, timestep, encoder_hidden_states=None):
        """diffusers-compatible call: per-sample ``encoder_hidden_states`` [B,L,D]; returns obj.sample [B,4,H,W] (wd)."""
        t = int(timestep)
        self.prepare_timesteps([t])
        self.prepare_prompt(encoder_hidden_states, record=False)
        B, _, H, W = sample.shape
        eps = self.forward_step(sample, 0, record=False)
        return _Out(eps.reshape(B, -1, H, W).to(F16))


class GraphedForward:
    """hipGraph of the NON-recording forward of a frozen U-Net (the R2 rollout of the training step: 20 of its 60 U-Net passes): one capture per
    (N, H, W, pair), replayed for every denoising step.  What changes between replays lives in static buffers the captured kernels read --
    the latents (``x``), the row of the time-embedding table (``trow``) and the cross-attention K / V (``prepare_cross(static=True)`` rewrites them
    in place for each rollout); everything the forward allocates comes from the graph's private pool.  Same kernels on the same data: eps is
    bit-identical to the eager forward (tests).  Host cost of a forward: ~2900 C-ABI calls -> one graph launch."""

    def __init__(self, unet):
        self.unet, self.graphs = unet, {}
        unet.graphed = self

    def _capture(self, key, lat, step_index):
        u = self.unet
        N, _, H, W = lat.shape
        x = torch.empty_like(lat)
        trow = torch.empty_like(u.temb_table[:1])
        x.copy_(lat)
        trow.copy_(u.temb_table[step_index:step_index + 1])
        u.forward_step(x, 0, record=False, pair=key[3], trow=trow)          # eager warm-up on this stream: per-kernel one-off attribute calls, workspaces
        g = torch.cuda.CUDAGraph()
        g.capture_begin(capture_error_mode="thread_local")
        try:
            eps = u.forward_step(x, 0, record=False, pair=key[3], trow=trow)
        finally:
            g.capture_end()
        self.graphs[key] = (g, x, trow, eps)

    def __call__(self, lat, step_index, pair):
        """lat [N,4,H,W] fp32 on the current (side) stream -> eps [2N or N,4,H*W] fp32 (a static buffer: consume it before the next call)."""
        # the key holds everything a capture depends on: the latent shape, the CFG-pair form, the prompt shape, and the generation of the static
        # K / V buffers (prepare_cross(static=True) allocates new ones when Bk * L changes; a graph captured against freed buffers is dropped)
        c0 = self.unet.transformers[0].cross
        gen = tuple(getattr(t, "static_generation", 0) for t in self.unet.transformers)
        key = (lat.shape[0], lat.shape[2], lat.shape[3], bool(pair), c0["Bk"], c0["L"], gen)
        assert all(t.cross is not None and t.cross.get("static") for t in self.unet.transformers), "GraphedForward: prepare_prompt() must run with static K / V first"
        if key not in self.graphs:
            for k in [k for k in self.graphs if k[:6] == key[:6] or k[6] != gen]:      # captured against buffers that have been replaced
                del self.graphs[k]
            self._capture(key, lat, step_index)
        g, x, trow, eps = self.graphs[key]
        x.copy_(lat)
        trow.copy_(self.unet.temb_table[step_index:step_index + 1])
        g.replay()
        return eps
