"""References, fp16-rounding emulations, mutated references and the metric for the per-tensor gates of the U-Net's two block classes (pure torch on
the CPU: no GPU, no library).  tests/test_block_refs_cpu.py holds what is derived here without a GPU; tests/test_blocks_gpu.py binds it to
``TransformerBlock`` (unet.py) and ``ResnetBlock`` (layers.py).

Reference.  The modules of oracle/nn_unet.py (``Transformer2DModel`` with a ``LoRAAttnProcessor`` on attn1 and attn2, ``ResnetBlock2D``) in fp64, loaded
from the block's slice of the synthetic U-Net: the SHAPES of ``W.unet_param_shapes(UNetConfig())`` are cut to the block's prefix and only those tensors are
drawn (the full dict is 3.4 GB).  Frozen tensors are fp16-rounded, LoRA ``down`` comes from the synthetic dict and ``up`` ~ N(0, up_std).  ``tblock_forward`` /
``resnet_forward`` restate the two modules' ``forward`` over the modules' own leaves so that the recorded h0 / h1 / h2, the shared prefix of a CFG pair, the
emulation's extra roundings and the mutations have somewhere to sit; the CPU test holds the restatement to the modules' own ``forward``.

Inputs.  Everything is seeded and fp16-representable: x, the prompt embeddings, and the upstream gradient g = round16(N(0, 1) * 1e-3 * gscale) / gscale with
gscale = 2^10 (the scaled gradient is O(1): nothing is inf, and what flushes is below 6e-8 of it); the product gets g * gscale, exactly.

Metric per tensor, in fp64:  e2 = |got - ref|_2 / |ref|_2,  emax = max|got - ref| / max|ref|.

Yardstick: the same block in fp32 arithmetic with fp16 roundings.  Variants (``VARIANTS``):
  a  a forward hook rounds the output of every leaf module, a full-backward hook rounds every leaf module's input gradient as round16(g * gscale) / gscale;
     LoRA weight gradients stay fp32
  b  a, with no forward rounding inside LayerNorm2 -> to_q -> attention -> to_out + residual -> LayerNorm3 (what the fused cross-attention kernel does); what
     that region keeps for the backward is rounded, as the kernel writes its records
  c  a, plus the roundings the kernels state between leaves: P before P.V, q * d^-0.5 log2(e) re-rounded where d % 16 == 8, the attention output, the GEGLU
     product, each residual sum
  d  a, plus dq | dk | dv rounded before the input-gradient GEMM and the two half-gradients of a CFG pair rounded before their sum
  e  a at a second input seed (against its own fp64 reference)
Band of tensor T: MARGIN x max over the variants of the emulation's statistic (tests/block_bands.py).  Nothing measured on the product enters.

Mutated references (``MUTATIONS``): wrong variants of the fp64 reference with the tensors each must move."""
import contextlib
import functools
import math
import os
import sys
import types
import warnings

import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from finetune_fair_diffusion_amd import weights as W  # noqa: E402
from oracle import nn_unet  # noqa: E402

GSCALE = 1024.0
LOG2E = 1.4426950408889634
HEADS, GROUPS, XDIM = 8, 32, 768
VARIANTS = ("a", "b", "c", "d", "e")
CAP_FWD, CAP_GRAD = 2e-2, 5e-2          # the project's engine-level tolerances (emax): no band may exceed them
PROJS = ("to_q", "to_k", "to_v", "to_out")
LORA_KEYS = tuple(f"{a}.{p}.{w}" for a in ("attn1", "attn2") for p in PROJS for w in ("down", "up"))
KV2_KEYS = tuple(f"attn2.{p}.{w}" for p in ("to_k", "to_v") for w in ("down", "up"))
T_PREFIX = {320: "down_blocks.0.attentions.0.", 640: "down_blocks.1.attentions.0.", 1280: "mid_block.attentions.0."}


def r16(t):
    return t.half().to(t.dtype)


def metric(got, ref):
    """(e2, emax) of ``got`` against ``ref``, in fp64 on the host."""
    got, ref = got.detach().double().cpu().reshape(-1), ref.detach().double().cpu().reshape(-1)
    assert got.shape == ref.shape, (got.shape, ref.shape)
    d = got - ref
    return float(d.norm() / ref.norm().clamp_min(1e-300)), float(d.abs().max() / ref.abs().max().clamp_min(1e-300))


# ============================================================================= rounding policy
class _Round(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, fwd, gs):
        ctx.gs = gs
        return r16(x) if fwd else x.view_as(x)

    @staticmethod
    def backward(ctx, g):
        return (r16(g * ctx.gs) / ctx.gs if ctx.gs else g), None, None


class _Dup(torch.autograd.Function):
    """cat([t, t]) of the CFG pair's shared prefix; ``gs``: the two half-gradients are rounded before their sum."""

    @staticmethod
    def forward(ctx, t, gs):
        ctx.gs = gs
        return torch.cat([t, t])

    @staticmethod
    def backward(ctx, g):
        n = g.shape[0] // 2
        return r16(g[:n] * ctx.gs) / ctx.gs + r16(g[n:] * ctx.gs) / ctx.gs, None


class Policy:
    """What a run of the restated forward does beyond the modules' own arithmetic: ``variant`` None = the reference, else one of VARIANTS; ``mut`` a
    mutation name or None."""

    def __init__(self, variant=None, mut=None):
        assert variant in (None,) + VARIANTS and (mut is None or mut in MUTATIONS)
        self.variant, self.mut = variant, mut
        self.hooks = variant is not None
        self.suspend = False            # b: forward hooks off inside the fused region
        self.between = variant == "c"
        self.gradr = variant == "d"

    def fwd(self, t):                   # c: a rounding the kernels state between leaves
        return _Round.apply(t, True, 0.0) if self.between else t

    def grad(self, t):                  # d: the gradient w.r.t. t is rounded
        return _Round.apply(t, False, GSCALE) if self.gradr else t

    def dup(self, t):
        if self.mut == "M3":
            return torch.cat([t.detach(), t])
        return _Dup.apply(t, GSCALE) if self.gradr else torch.cat([t, t])

    def records(self):
        """b: what the fused region keeps for the backward is fp16, as the kernel writes its records (n2, q2, o2, the 16-bit LoRA operands); the per-row
        LayerNorm statistics stay fp32."""
        if not self.suspend:
            return contextlib.nullcontext()
        return torch.autograd.graph.saved_tensors_hooks(lambda t: r16(t) if t.is_floating_point() and t.dim() and t.shape[-1] > 1 else t, lambda t: t)

    def lora_in(self, t):
        return t.detach() if self.mut == "M4" else t

    def install(self, mod):
        if not self.hooks:
            return []

        def fh(_m, _i, out):
            return out if self.suspend else r16(out)

        def bh(_m, gin, _gout):
            return tuple(None if g is None else r16(g * GSCALE) / GSCALE for g in gin)
        hs = []
        for m in mod.modules():
            if not list(m.children()):
                hs += [m.register_forward_hook(fh), m.register_full_backward_hook(bh)]
        return hs


# ============================================================================= cases
def _draw(shapes, seed):
    sd = W.synthetic_state_dict(shapes, seed=seed)
    return {n: t.half().float() for n, t in sd.items()}


def _rand16(shape, seed, scale=1.0):
    return (torch.randn(shape, generator=torch.Generator().manual_seed(seed)) * scale).half().double()


def _grad16(shape, seed):
    return (torch.randn(shape, generator=torch.Generator().manual_seed(seed)) * (1e-3 * GSCALE)).half().double() / GSCALE


def tblock_case(C, H=8, W_=8, rank=4, lora=True, pair=False, steps=1, new_enc=False, seed=0, up_std=0.02, B=4, Bk=2, L=13):
    """One transformer-block problem: weights, LoRA tensors and ``steps`` seeded (x, enc, g) triples.  ``pair``: x holds B // 2 latents.  The steps are the
    timesteps of one rollout, with one prompt, unless ``new_enc``."""
    p = T_PREFIX[C]
    cfg = W.UNetConfig()
    shapes = {n: s for n, s in W.unet_param_shapes(cfg).items() if n.startswith(p)}
    sd = _draw(shapes, seed + 1)
    lsd = None
    if lora:
        lshapes = {n: s for n, s in W.unet_lora_param_shapes(cfg, rank).items() if n.startswith(p)}
        lsd = W.synthetic_state_dict(lshapes, seed=seed + 5)
        g = torch.Generator().manual_seed(seed + 10)
        for n in lsd:
            if ".up." in n:
                lsd[n] = torch.randn(lsd[n].shape, generator=g) * up_std
    N = B // 2 if pair else B
    st = [types.SimpleNamespace(x=_rand16((N, C, H, W_), seed + 100 + 10 * s), enc=_rand16((Bk, L, XDIM), seed + 101 + (10 * s if new_enc else 0)),
                                g=_grad16((B, C, H, W_), seed + 102 + 10 * s)) for s in range(steps)]
    return types.SimpleNamespace(kind="t", prefix=p, C=C, H=H, W=W_, B=B, Bk=Bk, L=L, rank=rank, lora=lora, pair=pair, sd=sd, lora_sd=lsd, lora_shapes=lshapes if lora else None,
                                 steps=st, seed=seed, up_std=up_std)


def resnet_case(prefix, C1, C2, Cout, H=8, W_=8, seed=0, B=4):
    """One ResnetBlock problem: x [B, C1, H, W], skip [B, C2, H, W] or None (C2 = 0), an fp16 temb row [1, Cout]."""
    shapes = {n: s for n, s in W.unet_param_shapes(W.UNetConfig()).items() if n.startswith(prefix) and "time_emb_proj" not in n}
    assert shapes[prefix + "conv1.weight"][:2] == (Cout, C1 + C2), (shapes[prefix + "conv1.weight"], C1, C2, Cout)
    sd = _draw(shapes, seed + 1)
    return types.SimpleNamespace(kind="r", prefix=prefix, C1=C1, C2=C2, Cout=Cout, H=H, W=W_, B=B, sd=sd, seed=seed,
                                 x=_rand16((B, C1, H, W_), seed + 100), skip=_rand16((B, C2, H, W_), seed + 101) if C2 else None,
                                 trow=_rand16((1, Cout), seed + 103, 0.5), g=_grad16((B, Cout, H, W_), seed + 102))


# arm -> (builder, keyword arguments).  T1, T2, the C = 320 half of T8 and step 0 of T9 are one problem; T5 and the C = 1280 half of T8 another.
CASES = {
    "T1": (tblock_case, dict(C=320)),
    "T3": (tblock_case, dict(C=320, W_=6)),
    "T4": (tblock_case, dict(C=640)),
    "T5": (tblock_case, dict(C=1280)),
    "T6": (tblock_case, dict(C=320, rank=50)),
    "T7": (tblock_case, dict(C=320, pair=True)),
    "T9": (tblock_case, dict(C=320, steps=2)),
    "T10": (tblock_case, dict(C=320, lora=False, steps=2, new_enc=True)),
    "R1": (resnet_case, dict(prefix="down_blocks.0.resnets.0.", C1=320, C2=0, Cout=320)),
    "R2": (resnet_case, dict(prefix="down_blocks.1.resnets.0.", C1=320, C2=0, Cout=640)),
    "R3": (resnet_case, dict(prefix="up_blocks.2.resnets.2.", C1=640, C2=320, Cout=640)),
    "R4": (resnet_case, dict(prefix="up_blocks.0.resnets.0.", C1=1280, C2=1280, Cout=1280)),
    "R5": (resnet_case, dict(prefix="down_blocks.0.resnets.0.", C1=320, C2=0, Cout=320, H=16, W_=16)),
    "U": (lambda seed: unet_case(seed), dict()),
}
ALIASES = {"T2": "T1", "T8a": "T1", "T8b": "T5"}


@functools.lru_cache(maxsize=None)
def case(arm, seed=0):
    fn, kw = CASES[ALIASES.get(arm, arm)]
    return fn(seed=seed, **kw)


# ============================================================================= the restated forwards
def build_tblock(cs, dtype):
    m = nn_unet.Transformer2DModel(cs.C, HEADS, XDIM, GROUPS)
    m.load_state_dict({n[len(cs.prefix):]: t for n, t in cs.sd.items()}, strict=True)
    m.requires_grad_(False)
    if cs.lora:
        blk = m.transformer_blocks[0]
        for a, xd in (("attn1", None), ("attn2", XDIM)):
            proc = nn_unet.LoRAAttnProcessor(cs.C, xd, cs.rank)
            pre = f"{cs.prefix}transformer_blocks.0.{a}.processor."
            proc.load_state_dict({n[len(pre):]: t for n, t in cs.lora_sd.items() if n.startswith(pre)}, strict=True)
            getattr(blk, a).processor = proc        # registers as a child module: it follows .to(dtype) and takes the emulation's hooks
    return m.to(dtype)


def lora_params(m):
    blk = m.transformer_blocks[0]
    return {f"{a}.{p}.{w}": getattr(getattr(getattr(blk, a).processor, p + "_lora"), w).weight for a in ("attn1", "attn2") for p in PROJS for w in ("down", "up")}


def _attention(a, hs, ctx, idx, pol, dup=False, prescale_ok=True):
    """``Attention.forward`` over the module's own leaves.  ``ctx`` None: self-attention; else [Bk, L, X] with sample i reading group idx[i]."""
    p = a.processor
    src = hs if ctx is None else ctx
    q = a.to_q(hs)
    if p is not None:
        q = q + p.to_q_lora(pol.lora_in(hs))
    fused, pol.suspend = pol.suspend, False      # the prompt's K / V are made once per rollout by their own GEMMs, outside the fused kernel
    k, v = a.to_k(src), a.to_v(src)
    if p is not None:
        k = k + p.to_k_lora(pol.lora_in(src))
        v = v + p.to_v_lora(pol.lora_in(src))
    pol.suspend = fused
    q, k, v = pol.grad(q), pol.grad(k), pol.grad(v)
    if dup:
        q = pol.dup(q)
    if ctx is not None:
        k, v = k[idx], v[idx]
    B, T, C = q.shape
    h = a.heads
    d = C // h

    def split(x):
        return x.reshape(B, x.shape[1], h, d).permute(0, 2, 1, 3)
    if pol.between and d % 16 == 8:      # the pre-scaled q of ops.q_prescale: rounded once more after the multiply, exp2 of the bare QK^T
        q = pol.fwd(q * (a.scale * LOG2E))
        scores = torch.matmul(split(q), split(k).transpose(-1, -2)) * math.log(2.0)
    else:
        scores = torch.matmul(split(q), split(k).transpose(-1, -2)) * a.scale
    probs = scores.softmax(dim=-1)
    if pol.between:                      # P is rounded for the P.V product only (the denominator's rounding is second order)
        probs = probs + (r16(probs) - probs).detach()
    out = pol.fwd(torch.matmul(probs, split(v)).permute(0, 2, 1, 3).reshape(B, T, C))
    o = a.to_out[0](out)
    if p is not None:
        o = o + p.to_out_lora(pol.lora_in(out))
    return o


def _geglu(gg, x, pol):
    if not pol.between:
        return gg(x)
    a, gate = gg.proj(x).chunk(2, dim=-1)
    return pol.fwd(a * F.gelu(gate))


def tblock_forward(m, x, enc, idx, pol, pair=False):
    """``Transformer2DModel.forward`` with one BasicTransformerBlock.  x [N, C, H, W]; enc [Bk, L, X]; idx [B]: the prompt group of each sample.
    ``pair``: N = B / 2 latents; the prefix up to the cross-attention query is evaluated once and duplicated.  Returns (out [B, C, H, W], taps) with the taps
    h0 [N, HW, C], h1 [N, HW, C], h2 [B, HW, C]."""
    N, C, H, Wd = x.shape
    blk = m.transformer_blocks[0]
    h0 = m.proj_in(m.norm(x)).permute(0, 2, 3, 1).reshape(N, H * Wd, C)
    h1 = pol.fwd(_attention(blk.attn1, blk.norm1(h0), None, None, pol) + h0)
    pol.suspend = pol.variant == "b"
    with pol.records():
        a2 = _attention(blk.attn2, blk.norm2(h1), enc, idx, pol, dup=pair)
        h2 = pol.fwd(a2 + (pol.dup(h1) if pair else h1))
        n3 = blk.norm3(h2)
    if pol.suspend:                      # the fused kernel still writes h2 and LayerNorm3(h2) in fp16
        pol.suspend = False
        h2, n3 = _Round.apply(h2, True, 0.0), _Round.apply(n3, True, 0.0)
    ff = blk.ff.net[2](_geglu(blk.ff.net[0], n3, pol))
    h3 = pol.fwd(ff + (h2.detach() if pol.mut == "M2" else h2))
    B = h3.shape[0]
    out = pol.fwd(m.proj_out(h3.reshape(B, H, Wd, C).permute(0, 3, 1, 2)) + (pol.dup(x) if pair else x))
    return out, dict(h0=h0, h1=h1, h2=h2)


def _cl(t):
    """[B, C, H, W] -> the product's [B*H*W, C]."""
    return t.permute(0, 2, 3, 1).reshape(-1, t.shape[1])


def run_tblock(cs, variant=None, mut=None):
    """All gated tensors of a transformer-block case, as fp64 host tensors in the product's layouts (gradients UNscaled: divide the product's dx / denc by
    gscale).  Several steps: forward tensors and dx carry '@step', LoRA gradients and denc are summed over the steps."""
    pol = Policy(variant, mut if mut in ("M2", "M3", "M4") else None)
    dtype = torch.float64 if variant is None else torch.float32
    m = build_tblock(cs, dtype)
    hooks = pol.install(m)
    kv_div = cs.B // cs.Bk
    idx = torch.arange(cs.B) % cs.Bk if mut == "M6" else torch.arange(cs.B) // kv_div
    lp = lora_params(m) if cs.lora else {}
    for p in lp.values():
        p.requires_grad_(True)
    out = {}
    acc = {}
    try:
        for s, st in enumerate(cs.steps):
            tag = f"@{s}" if len(cs.steps) > 1 else ""
            x, enc = st.x.to(dtype).requires_grad_(True), st.enc.to(dtype).requires_grad_(True)
            y, taps = tblock_forward(m, x, enc, idx, pol, pair=cs.pair)
            out["out" + tag] = _cl(y)
            for k, t in taps.items():
                out[k + tag] = t.reshape(-1, cs.C)
            if not cs.lora:
                continue
            names = list(lp)
            gr = torch.autograd.grad(y, [x, enc] + [lp[n] for n in names], grad_outputs=st.g.to(dtype))
            out["dx" + tag] = _cl(gr[0])
            last = s == len(cs.steps) - 1
            for n, g in zip(["denc"] + names, gr[1:]):
                if mut == "M5" and not last and (n == "denc" or n in KV2_KEYS):
                    continue
                acc[n] = g.double() if n not in acc else acc[n] + g.double()
    finally:
        for h in hooks:
            h.remove()
    if "denc" in acc:
        acc["denc"] = acc["denc"].reshape(-1, XDIM)
    out.update(acc)
    if mut == "M1":
        for w in ("down", "up"):
            out[f"attn2.to_k.{w}"], out[f"attn2.to_v.{w}"] = out[f"attn2.to_v.{w}"], out[f"attn2.to_k.{w}"]
    if mut == "M7":
        for w in ("down", "up"):
            out[f"attn2.to_out.{w}"] = out[f"attn2.to_out.{w}"] / GSCALE
    return {k: v.detach().double() for k, v in out.items()}


def build_resnet(cs, dtype):
    m = nn_unet.ResnetBlock2D(cs.C1 + cs.C2, cs.Cout, temb_channels=0, groups=GROUPS, eps=1e-5)
    m.load_state_dict({n[len(cs.prefix):]: t for n, t in cs.sd.items()}, strict=True)
    return m.requires_grad_(False).to(dtype)


def resnet_forward(m, xc, trow, pol):
    """``ResnetBlock2D.forward`` on the concatenated input, with the projected time-embedding row [1, Cout] added where the module adds its projection."""
    h = m.conv1(F.silu(m.norm1(xc)))
    if trow is not None and pol.mut != "M8":
        h = h + trow[:, :, None, None]
    h = m.conv2(F.silu(m.norm2(h)))
    sc = xc
    if m.conv_shortcut is not None:
        sc = m.conv_shortcut(xc.detach() if pol.mut == "M10" else xc)
    return sc + h


def run_resnet(cs, variant=None, mut=None):
    pol = Policy(variant, mut)
    dtype = torch.float64 if variant is None else torch.float32
    m = build_resnet(cs, dtype)
    hooks = pol.install(m)
    try:
        x = cs.x.to(dtype).requires_grad_(True)
        skip = cs.skip.to(dtype).requires_grad_(True) if cs.skip is not None else None
        xc = torch.cat([x, skip], 1) if skip is not None else x
        xc.retain_grad()
        y = resnet_forward(m, xc, cs.trow.to(dtype), pol)
        y.backward(cs.g.to(dtype))
    finally:
        for h in hooks:
            h.remove()
    dcat = xc.grad
    if mut == "M9":      # the halves of the concatenated input's gradient handed out in the other order (equal widths: dx and dskip exchanged)
        dcat = torch.cat([dcat[:, cs.C2:], dcat[:, :cs.C2]], 1)
    out = dict(out=_cl(y), dx=_cl(dcat[:, :cs.C1]))
    if skip is not None:
        out["dskip"] = _cl(dcat[:, cs.C1:])
    return {k: v.detach().double() for k, v in out.items()}


# ----------------------------------------------------------------------------- the whole U-Net at the production arms
def unet_case(seed=0, H=16, L=13, t=601):
    """util_models size "d40" (C = 320 / 640, d = 40 / 80) at 16x16 latents -- 256 and 64 rows per sample, the smallest at which both levels take the fused
    cross-attention kernel -- with a CFG pair of ONE latent: eps for the two halves and the 96 LoRA gradients."""
    import util_models as U
    sds = U.synthetic_sds(rank=4, size="d40", seed=seed)
    cfg = dict(U.D40_UNET)
    return types.SimpleNamespace(kind="u", cfg=cfg, sd=sds["unet"], lora_sd=sds["unet_lora"], H=H, L=L, t=t, rank=4, seed=seed,
                                 x=_rand16((1, 4, H, H), seed + 100), enc=_rand16((2, L, cfg["cross_attention_dim"]), seed + 101),
                                 g=_grad16((2, 4, H, H), seed + 102))


def run_unet(cs, variant=None, mut=None):
    """eps [2, 4, H, W] and every LoRA gradient by its state-dict name, fp64.  The emulation variants act inside the transformer blocks through
    ``tblock_forward``; everything else takes variant a's leaf hooks, and the sinusoidal embedding is rounded as the product casts it."""
    assert mut is None
    pol = Policy(variant)
    dtype = torch.float64 if variant is None else torch.float32
    net = nn_unet.UNet2DConditionModel(nn_unet.UNetConfig(**cs.cfg))
    net.load_state_dict(cs.sd, strict=True)
    net.requires_grad_(False)
    layers = nn_unet.make_unet_lora(net, cs.rank)
    layers.load_named(cs.lora_sd)
    net.to(dtype)
    names = list(layers.state_dict().keys())
    params = list(layers.parameters())
    for p in params:
        p.requires_grad_(True)
    idx = torch.arange(2)
    for m in net.modules():
        if isinstance(m, nn_unet.Transformer2DModel):
            m.forward = (lambda x, enc, m=m: tblock_forward(m, x, enc, idx, pol)[0])
    hooks = pol.install(net)
    real = nn_unet.timestep_embedding
    if variant is not None:
        nn_unet.timestep_embedding = lambda t, dim: r16(real(t, dim))
    try:
        x = torch.cat([cs.x, cs.x]).to(dtype)
        with warnings.catch_warnings():         # conv_in's input needs no gradient: its full-backward hook says so
            warnings.simplefilter("ignore", UserWarning)
            eps = net(x, torch.tensor(cs.t), cs.enc.to(dtype)).sample
            gr = torch.autograd.grad(eps, params, grad_outputs=cs.g.to(dtype))
    finally:
        nn_unet.timestep_embedding = real
        for h in hooks:
            h.remove()
    out = {"eps": eps}
    out.update(zip(names, gr))
    return {k: v.detach().double() for k, v in out.items()}


def unet_gated(ref):
    """(gated, skipped) LoRA gradient names: a tensor whose reference norm is below 1e-3 of the largest is not gated."""
    norms = {k: float(v.norm()) for k, v in ref.items() if k != "eps"}
    top = max(norms.values())
    return [k for k, n in norms.items() if n >= 1e-3 * top], [k for k, n in norms.items() if n < 1e-3 * top]


def run(cs, variant=None, mut=None):
    return {"t": run_tblock, "r": run_resnet, "u": run_unet}[cs.kind](cs, variant, mut)


# ============================================================================= mutations
# name -> (arms it applies to, the tensors it must move)
_PREFIX_LORA = tuple(k for k in LORA_KEYS if k.startswith("attn1.") or k.startswith("attn2.to_q."))
MUTATIONS = {
    "M1": (("T1", "T7", "T9"), KV2_KEYS),
    "M2": (("T1", "T7", "T9"), ("dx",) + LORA_KEYS + ("denc",)),
    "M3": (("T7",), ("dx",) + _PREFIX_LORA),
    "M4": (("T1", "T7", "T9"), ("dx", "denc")),
    "M5": (("T9",), KV2_KEYS + ("denc",)),
    "M6": (("T1", "T7", "T9"), ("out", "h2", "dx", "denc") + tuple(k for k in LORA_KEYS if k.startswith("attn2."))),
    "M7": (("T1", "T7", "T9"), ("attn2.to_out.down", "attn2.to_out.up")),
    "M8": (("R3",), ("out", "dx", "dskip")),
    "M9": (("R3",), ("dx", "dskip")),
    "M10": (("R3",), ("dx", "dskip")),
}
MUTATION_ARMS = ("T1", "T7", "T9", "R3")


def moved_keys(arm, mut, ref):
    """The reference tensors of ``arm`` a mutation names ('dx' names dx@0 and dx@1 of a two-step arm, and so on)."""
    names = MUTATIONS[mut][1]
    return [k for k in ref if k.split("@")[0] in names]


# ============================================================================= statistics and bands
@functools.lru_cache(maxsize=None)
def reference(arm, mut=None, seed=0):
    return run(case(arm, seed), None, mut)


@functools.lru_cache(maxsize=None)
def emulation_stats(arm):
    """{tensor: {variant: (e2, emax)}} of the emulation variants of ``arm`` against the fp64 reference (variant e: second seed, its own reference)."""
    cs = case(arm)
    ref = reference(arm)
    stats = {k: {} for k in ref}
    for v in VARIANTS:
        if cs.kind == "r" and v in ("b", "c", "d"):
            continue
        if v == "e":
            got, r = run(case(arm, 1), "a"), reference(arm, None, 1)
        else:
            got, r = run(cs, v), ref
        for k in ref:
            stats[k][v] = metric(got[k], r[k])
    return stats


def variant_ratios(stats, use_emax=True):
    """Largest ratio, per statistic, of a variant to variant a and of a to a variant -> (ratio_e2, ratio_emax, where).  ``use_emax=False``: e2 only (the
    whole U-Net is gated in e2 alone)."""
    best = [1.0, 1.0]
    where = [None, None]
    for k, sv in stats.items():
        for v, val in sv.items():
            for i in ((0, 1) if use_emax else (0,)):
                a, b = sv["a"][i], val[i]
                r = max(a / b, b / a)
                if r > best[i]:
                    best[i], where[i] = r, (k, v)
    return best[0], best[1], where


def is_forward(key):
    return key.split("@")[0] in ("out", "h0", "h1", "h2")


def bands(arm):
    """{tensor: (band_e2, band_emax, emul_e2, emul_emax)}: the margins of tests/block_bands.py over the largest emulation statistic."""
    import block_bands as BB
    out = {}
    m2 = BB.MARGIN_E2_NET if arm == "U" else BB.MARGIN_E2       # the whole U-Net is gated in e2 alone, under the margin of its own emulations
    for k, sv in emulation_stats(arm).items():
        e2, em = max(v[0] for v in sv.values()), max(v[1] for v in sv.values())
        b2 = m2 * e2
        if arm == "U":      # deep gradients: where the rule's band would pass the engine-level tolerance, the tolerance is the band (never wider than the rule)
            b2 = min(b2, CAP_FWD if k == "eps" else CAP_GRAD)
        out[k] = (b2, BB.MARGIN_MAX * em, e2, em)
    return out
