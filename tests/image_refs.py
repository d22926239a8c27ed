"""References, fp16-rounding emulations, mutated references and cases for the per-tensor gates of the image-side networks' hand-written backwards (pure torch
on the CPU: no GPU, no library).  tests/test_image_refs_cpu.py holds what is derived here without a GPU; tests/test_image_blocks_gpu.py binds it to
``MobileNetV3Large`` (classifier.py), ``SFNet20`` (sfnet.py), the VAE decoder (vae.py) and the two ViTs (vit.py).  Built like tests/block_refs.py, whose ``metric``, ``r16``, rounding function and ``Policy`` it reuses.

Reference.  The arithmetic of the oracle modules (oracle/nn_mobilenet.py ``InvertedResidual`` / ``SqueezeExcitation`` / ``ConvBNAct``, oracle/nn_sfnet.py) in fp64,
and of oracle/nn_vae.py / oracle/nn_vit.py (their own modules, with leaf hooks),
restated over functional leaves so that recorded pre-activations, forced branches, the emulations' roundings and the mutations have somewhere to sit; the CPU
test holds the restatement to the modules' own ``forward``.  Weights are seeded and synthetic, given the numbers the product multiplies with: BatchNorm folded
as ``classifier._fold`` folds it (in fp64), pointwise / linear / 3x3 weights then rounded to fp16, depthwise and stem weights and every bias to fp32.

Inputs are seeded and fp16-representable; the upstream gradient is g = round16(N(0, 1) * 1e-3 * gscale) / gscale with the gscale step.py gives that network's
backward: 1024 for the classifier (``clf_gscale``), the power of two nearest to 1 / max|g| for SFNet-20 and the ViTs (``_pow2_scale_dev(.., 1.0)``), to 64 / max|g| for the VAE.

Forced branches.  Every piecewise activation of a reference run takes, element by element, the branch a CANDIDATE took -- the product, read from its records, or
an emulation variant -- in the forward and the backward alike: ReLU z > 0; hardswish / hardsigmoid z <= -3 | -3 < z < 3 | z >= 3 (the sub-gradient convention
of common.h's ``act_grad``; the forward is continuous there).  The forward applies the formula of the forced branch (ReLU: z * mask).  The gate is always
metric(candidate, reference under the candidate's branches).  ``flips`` measures, per mask, the share of elements that took another branch than the unforced
fp64 reference (cap ``FLIP_CAP``) and how far the reference's pre-activation of each such element is from the break point it crossed.

Emulation variants (``VARIANTS``): the same arithmetic in fp32 with
  a  every leaf output (convolution, linear, activation) rounded to fp16, every leaf input gradient rounded as round16(g * gscale) / gscale
  c  a, plus the roundings the product states between leaves: the pre-activation before its activation, the pooled squeeze-excite vector, the squeeze-excite
     product, each residual sum (in SFNet: the sum inside the second convolution's epilogue) -- and their counterparts in the backward, where every gradient
     tensor is written in fp16: the sum of the residual and the block gradient (a GEMM / convolution epilogue, ``ops.add``), the two squeeze-excite paths
     joined in ``avgpool_hw_bwd(add=)``, both outputs of ``scale_channels_bwd``, the output of the head's ``avgpool_hw_bwd``
  e  a at a second input seed (against its own reference)
Band of tensor T: margin x the largest emulation statistic (tests/image_bands.py).  Nothing measured on the product enters.

Mutated references (``MUTATIONS``): wrong variants of the fp64 reference with the tensors each must move."""
import functools
import os
import sys
import types

import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from finetune_fair_diffusion_amd import weights as W  # noqa: E402
from block_refs import CAP_FWD, CAP_GRAD, Policy, _Round, _cl, metric, r16, variant_ratios  # noqa: E402,F401

VARIANTS = ("a", "c", "e")
FLIP_CAP = 0.01
GS_CLF = 1024.0
CLF_GAIN = 1.4          # tests/util_models.py draws the classifier with this gain


class _Shift(torch.autograd.Function):
    """Identity whose gradient arrives one pixel to the right (mutation: a stride-2 data gradient indexed from the wrong origin)."""

    @staticmethod
    def forward(ctx, x):
        return x.view_as(x)

    @staticmethod
    def backward(ctx, g):
        return torch.roll(g, 1, dims=-1)


class ImagePolicy(Policy):
    """block_refs.Policy with a gscale of its own, functional leaves and forced branches.  ``force``: {mask name: branch tensor} or None (the run takes its own
    branches); after the run ``branch`` holds what it took and ``z`` the pre-activations it saw."""

    def __init__(self, variant=None, mut=None, gscale=GS_CLF, force=None):
        assert variant in (None, "a", "c") and (mut is None or mut in MUTATIONS)
        self.variant, self.mut, self.gs, self.force = variant, mut, gscale, force
        self.hooks = variant is not None
        self.suspend, self.between, self.gradr = False, variant == "c", False
        self.branch, self.z = {}, {}

    def leaf(self, f, *xs):
        """A leaf module: its output rounded, its input gradients rounded (what Policy.install's hooks do to an nn.Module)."""
        if not self.hooks:
            return f(*xs)
        return _Round.apply(f(*[_Round.apply(x, False, self.gs) for x in xs]), True, 0.0)

    def install(self, mod):
        """Policy.install under this policy's gscale: every leaf module's output rounded, its input gradients rounded."""
        if not self.hooks:
            return []
        hs = []
        for m in mod.modules():
            if not list(m.children()):
                hs += [m.register_forward_hook(lambda _m, _i, out: r16(out)),
                       m.register_full_backward_hook(lambda _m, gin, _go: tuple(None if g is None else r16(g * self.gs) / self.gs for g in gin))]
        return hs

    def gsum(self, t):
        """c: the gradient w.r.t. ``t`` is written in fp16 -- a sum of two gradient paths (the residual entering a GEMM epilogue or ``ops.add``, the
        squeeze-excite paths joined in ``avgpool_hw_bwd(add=)``), or the output of a backward kernel that is no leaf's input gradient."""
        return _Round.apply(t, False, self.gs) if self.between else t

    def act(self, name, z, kind):
        z = self.fwd(z)
        br = branches(z.detach(), kind) if self.force is None else self.force[name]
        assert br.shape == z.shape, (name, br.shape, z.shape)
        self.branch[name], self.z[name] = br, z.detach().double()
        return self.leaf(lambda t: _act(t, br, kind, self.mut), z)


def branches(z, kind):
    """The branch each element takes: ReLU 0 | 1; hardswish / hardsigmoid 0 | 1 | 2; a post-ReLU record y gives the ReLU's (y > 0 <=> s > 0)."""
    if kind == "relu":
        return (z > 0).to(torch.int8)
    return (z > -3).to(torch.int8) + (z >= 3).to(torch.int8)


def _act(z, br, kind, mut=None):
    if kind == "relu":
        return z * (br == 1)
    zero = z * 0
    if kind == "hardswish":
        return torch.where(br == 1, z * (z + 3) / 6, torch.where(br == 2, z, zero))
    assert kind == "hardsigmoid"
    y = torch.where(br == 1, z / 6 + 0.5, torch.where(br == 2, zero + 1, zero))
    if mut == "hsig_outside":       # the gradient 1/6 everywhere
        y = y.detach() + (z - z.detach()) / 6
    return y


BREAKS = {"relu": (0.0,), "hardswish": (-3.0, 3.0), "hardsigmoid": (-3.0, 3.0)}


def flips(cand, ref_pol, kinds):
    """{mask: (share of elements on another branch than the unforced reference, n, largest distance of such an element's reference pre-activation to a break
    point it crossed, max|z_ref|)}."""
    out = {}
    for name, br in cand.items():
        rb, z = ref_pol.branch[name], ref_pol.z[name]
        diff = br != rb
        dist = 0.0
        if bool(diff.any()):
            lo, hi = torch.minimum(br, rb)[diff], torch.maximum(br, rb)[diff]
            bp = torch.tensor(BREAKS[kinds[name]], dtype=torch.float64)
            zz = z[diff]
            for j in range(len(bp)):            # break j separates branch j from branch j + 1
                crossed = (lo <= j) & (hi > j)
                if bool(crossed.any()):
                    dist = max(dist, float((zz[crossed] - bp[j]).abs().max()))
        out[name] = (float(diff.double().mean()), diff.numel(), dist, float(z.abs().max()))
    return out


# ============================================================================= inputs and weights
def _gen(seed):
    return torch.Generator().manual_seed(seed)


def _rand16(shape, seed, scale=1.0):
    return (torch.randn(shape, generator=_gen(seed)) * scale).half().double()


def _grad16(shape, seed, gs):
    return (torch.randn(shape, generator=_gen(seed)) * (1e-3 * gs)).half().double() / gs


def _leaf(t, dtype):
    return t.detach().to(dtype).clone().requires_grad_(True)


def pow2_scale(amax, target=1.0):
    """step.py's ``_pow2_scale_dev`` on the host."""
    return float(torch.exp2(torch.round(torch.log2(torch.tensor(target / amax)))))


@functools.lru_cache(maxsize=None)
def clf_sd(seed=0, num_classes=80):
    """The classifier's synthetic state dict (fp16-representable, as util_models draws it).  The squeeze-excite ``fc2`` biases are drawn ~ N(0, 2) so that the
    hardsigmoid saturates on some channels: with the default 0.02 no element ever leaves (-3, 3) and its outer branches would go untested."""
    sd = W.synthetic_state_dict(W.mobilenet_param_shapes(num_classes), seed=seed + 4, gain=CLF_GAIN)
    g = _gen(seed + 40)
    for n in sd:
        if n.endswith("fc2.bias"):
            sd[n] = torch.randn(sd[n].shape, generator=g) * 2.0
    return {n: (t.half().float() if t.is_floating_point() else t) for n, t in sd.items()}


def fold64(sd, p):
    """``classifier._fold`` in fp64: conv (p + '0') followed by BatchNorm (p + '1', eps 1e-3) -> (weight', bias')."""
    w = sd[p + "0.weight"].double()
    g, b, m, v = (sd[p + "1." + n].double() for n in ("weight", "bias", "running_mean", "running_var"))
    s = g / torch.sqrt(v + 1e-3)
    return w * s.view(-1, 1, 1, 1), b - m * s


def _r32(t):
    return t.float().double()


def mb_block_weights(sd, i, rounded=True):
    """Folded weights of block ``i`` as the product holds them (``rounded``) or exact."""
    k, exp, cout, se, act, s = W.MBV3_SETTINGS[i]
    cin = 16 if i == 0 else W.MBV3_SETTINGS[i - 1][2]
    p = f"features.{i + 1}.block."
    pw = (lambda w, b: (r16(w), _r32(b))) if rounded else (lambda w, b: (w, b))
    dw = (lambda w, b: (_r32(w), _r32(b))) if rounded else (lambda w, b: (w, b))
    wb = types.SimpleNamespace(i=i, k=k, exp=exp, cin=cin, cout=cout, act=act, stride=s, res=(s == 1 and cin == cout), expand=None, se=None)
    j = 0
    if exp != cin:
        wb.expand = pw(*fold64(sd, p + f"{j}."))
        j += 1
    wb.dw = dw(*fold64(sd, p + f"{j}."))
    j += 1
    if se:
        wb.se = tuple(pw(sd[p + f"{j}.{fc}.weight"].double().flatten(1), sd[p + f"{j}.{fc}.bias"].double()) for fc in ("fc1", "fc2"))
        j += 1
    wb.project = pw(*fold64(sd, p + f"{j}."))
    return wb


def mb_kinds(wb, pre=""):
    """{mask name: activation} of one block."""
    out = {pre + "z_dw": wb.act}
    if wb.expand is not None:
        out[pre + "z_exp"] = wb.act
    if wb.se is not None:
        out.update({pre + "z1": "relu", pre + "z2": "hardsigmoid"})
    return out


# ============================================================================= MobileNetV3: the restated forwards
def mb_block_forward(wb, x, pol, pre=""):
    """``InvertedResidual.forward`` with folded BatchNorm.  x [B, cin, H, W] -> (out, taps); taps: z_exp, z_dw [B, exp, H, W], z1, z2, se_s [B, .]."""
    taps = {}
    if wb.res:
        x = pol.gsum(x)
    inp = x
    if wb.expand is not None:
        z = pol.leaf(lambda t: F.conv2d(t, wb.expand[0].to(t.dtype), wb.expand[1].to(t.dtype)), x)
        taps["z_exp"] = z
        x = pol.act(pre + "z_exp", z, wb.act)
    if pol.mut == "dw_shift":
        x = _Shift.apply(x)
    zd = pol.leaf(lambda t: F.conv2d(t, wb.dw[0].to(t.dtype), wb.dw[1].to(t.dtype), stride=wb.stride, padding=(wb.k - 1) // 2, groups=wb.exp), x)
    taps["z_dw"] = zd
    x = pol.act(pre + "z_dw", zd, wb.act)
    if wb.se is not None:
        (w1, b1), (w2, b2) = wb.se
        x = pol.gsum(x)
        avg = pol.fwd((x.detach() if pol.mut == "se_no_pool" else x).mean(dim=(2, 3)))
        z1 = pol.leaf(lambda t: F.linear(t, w1.to(t.dtype), b1.to(t.dtype)), avg)
        z2 = pol.leaf(lambda t: F.linear(t, w2.to(t.dtype), b2.to(t.dtype)), pol.act(pre + "z1", z1, "relu"))
        s = pol.act(pre + "z2", z2, "hardsigmoid")
        taps.update(z1=z1, z2=z2, se_s=s)
        x = pol.fwd(pol.gsum(x.detach() if pol.mut == "se_no_direct" else x) * pol.gsum(s)[:, :, None, None])
    y = pol.leaf(lambda t: F.conv2d(t, wb.project[0].to(t.dtype), wb.project[1].to(t.dtype)), x)
    if wb.res:
        y = pol.fwd(y + (inp.detach() if pol.mut == "res_drop" else inp))
    return y, taps


def mb_config(i):
    """What distinguishes one inverted-residual block's code path from another's: (k, stride, SE, activation, residual, expand present)."""
    k, exp, cout, se, act, s = W.MBV3_SETTINGS[i]
    cin = 16 if i == 0 else W.MBV3_SETTINGS[i - 1][2]
    return (k, s, se, act, s == 1 and cin == cout, exp != cin)


def _mb_arms():
    seen, arms = {}, {}
    for i in range(len(W.MBV3_SETTINGS)):
        cfg = mb_config(i)
        if cfg not in seen:
            seen[cfg] = f"B{i}"
            arms[f"B{i}"] = dict(i=i, H=7)
    return seen, arms


MB_CONFIG_ARM, MB_ARMS = _mb_arms()          # configuration -> arm; arm -> (block index, map size): the first block of each configuration, on a 7x7 map
MB_ARMS["B12x10"] = dict(i=12, H=10)         # k = 5, stride 2, SE, hardswish once more on an even map


def mb_case(i, H, seed=0, B=3):
    sd = clf_sd(seed)
    wb = mb_block_weights(sd, i)
    Ho = (H + 2 * ((wb.k - 1) // 2) - wb.k) // wb.stride + 1
    return types.SimpleNamespace(kind="mb", i=i, B=B, H=H, Ho=Ho, wb=wb, sd=sd, seed=seed, gs=GS_CLF, kinds=mb_kinds(wb),
                                 x=_rand16((B, wb.cin, H, H), seed + 100 + i), g=_grad16((B, wb.cout, Ho, Ho), seed + 200 + i, GS_CLF))


def run_mb(cs, variant=None, mut=None, force=None):
    pol = ImagePolicy(variant, mut, cs.gs, force)
    dtype = torch.float64 if variant is None else torch.float32
    x = _leaf(cs.x, dtype)
    y, taps = mb_block_forward(cs.wb, x, pol)
    y.backward(cs.g.to(dtype))
    out = dict(out=_cl(y), dx=_cl(x.grad))
    for k, t in taps.items():
        out[k] = _cl(t) if t.dim() == 4 else t
    return {k: v.detach().double() for k, v in out.items()}, pol


# ----------------------------------------------------------------------------- stem + head
def head_weights(sd, rounded=True):
    r = (lambda w: r16(w)) if rounded else (lambda w: w)
    b = _r32 if rounded else (lambda t: t)
    w0, b0 = fold64(sd, "features.0.")
    wl, bl = fold64(sd, "features.16.")
    return types.SimpleNamespace(stem=(b(w0), b(b0)), last=(r(wl), b(bl)), fc1=(r(sd["classifier.0.weight"].double()), b(sd["classifier.0.bias"].double())),
                                 fc2=(r(sd["classifier.3.weight"].double()), b(sd["classifier.3.bias"].double())))


def stem_forward(hw, chips, pol):
    z0 = pol.leaf(lambda t: F.conv2d(t, hw.stem[0].to(t.dtype), hw.stem[1].to(t.dtype), stride=2, padding=1), chips)
    return pol.act("z0", z0, "hardswish"), z0


def head_forward(hw, x, pol):
    """features.16 -> average pool -> classifier.0 -> hardswish -> classifier.3 (Dropout is the identity in eval mode)."""
    zl = pol.leaf(lambda t: F.conv2d(t, hw.last[0].to(t.dtype), hw.last[1].to(t.dtype)), x)
    avg = pol.fwd(pol.gsum(pol.act("zl", zl, "hardswish")).mean(dim=(2, 3)))
    zf = pol.leaf(lambda t: F.linear(t, hw.fc1[0].to(t.dtype), hw.fc1[1].to(t.dtype)), avg)
    logits = pol.leaf(lambda t: F.linear(t, hw.fc2[0].to(t.dtype), hw.fc2[1].to(t.dtype)), pol.act("zf", zf, "hardswish"))
    return logits, dict(zl=zl, zf=zf)


HEAD_CLASSES = 13       # not a multiple of 8: the product pads the last GEMM to 16 columns (ncls_pad); the 80-logit head never does


def sh_case(seed=0, B=3, S=9, H=3):
    """Stem (chips [B, 3, S, S], odd: 9 -> 5) and head (x [B, 160, H, H] -> 13 logits): two pieces, one arm."""
    sd = clf_sd(seed, HEAD_CLASSES)
    return types.SimpleNamespace(kind="sh", B=B, S=S, H=H, sd=sd, hw=head_weights(sd), seed=seed, gs=GS_CLF, kinds=dict(z0="hardswish", zl="hardswish", zf="hardswish"),
                                 chips=_rand16((B, 3, S, S), seed + 300, 0.5).clamp(-1, 1), g0=_grad16((B, 16, (S + 1) // 2, (S + 1) // 2), seed + 301, GS_CLF),
                                 x=_rand16((B, 160, H, H), seed + 302), gl=_grad16((B, HEAD_CLASSES), seed + 303, GS_CLF))


def run_sh(cs, variant=None, mut=None, force=None):
    pol = ImagePolicy(variant, mut, cs.gs, force)
    dtype = torch.float64 if variant is None else torch.float32
    chips, x = _leaf(cs.chips, dtype), _leaf(cs.x, dtype)
    x0, z0 = stem_forward(cs.hw, chips, pol)
    x0.backward(cs.g0.to(dtype))
    logits, taps = head_forward(cs.hw, x, pol)
    logits.backward(cs.gl.to(dtype))
    out = dict(z0=_cl(z0), x0=_cl(x0), dchips=chips.grad, zl=_cl(taps["zl"]), zf=taps["zf"], logits=logits, dxl=_cl(x.grad))
    return {k: v.detach().double() for k, v in out.items()}, pol


# ----------------------------------------------------------------------------- the whole classifier
def clf_case(seed=0, B=3, S=64):
    sd = clf_sd(seed)
    blocks = [mb_block_weights(sd, i) for i in range(len(W.MBV3_SETTINGS))]
    kinds = dict(z0="hardswish", zl="hardswish", zf="hardswish")
    for wb in blocks:
        kinds.update(mb_kinds(wb, f"b{wb.i}."))
    g = torch.zeros(B, 80, dtype=torch.float64)      # dL/dlogits on two logits, as tests/test_engine_gpu.py::test_classifier_fwd_bwd has it (0.3 * 1024 is fp16-exact)
    g[:, 40], g[:, 41] = 0.3, -0.3
    g = (g * GS_CLF).half().double() / GS_CLF
    return types.SimpleNamespace(kind="clf", B=B, S=S, sd=sd, hw=head_weights(sd), blocks=blocks, seed=seed, gs=GS_CLF, kinds=kinds,
                                 chips=_rand16((B, 3, S, S), seed + 6).clamp(-1, 1), g=g)


def run_clf(cs, variant=None, mut=None, force=None):
    """logits, dchips, ``trace{i}`` = the gradient at block i's input, and every pre-activation under 'z.<mask name>'."""
    pol = ImagePolicy(variant, None, cs.gs, force)
    dtype = torch.float64 if variant is None else torch.float32
    chips = _leaf(cs.chips, dtype)
    x, z0 = stem_forward(cs.hw, chips, pol)
    out, ins = {"z.z0": _cl(z0)}, []
    for wb in cs.blocks:
        x.retain_grad()
        ins.append(x)
        pol.mut = mut if (mut is not None and wb.i in MUTATIONS[mut][2]) else None
        x, taps = mb_block_forward(wb, x, pol, f"b{wb.i}.")
        for k, t in taps.items():
            if k != "se_s":
                out[f"z.b{wb.i}.{k}"] = _cl(t) if t.dim() == 4 else t
    pol.mut = None
    logits, taps = head_forward(cs.hw, x, pol)
    logits.backward(cs.g.to(dtype))
    out.update({"z.zl": _cl(taps["zl"]), "z.zf": taps["zf"], "logits": logits, "dchips": chips.grad})
    out.update({f"trace{i}": _cl(t.grad) for i, t in enumerate(ins)})
    return {k: v.detach().double() for k, v in out.items()}, pol


# ============================================================================= SFNet-20
SF_CH = W.SFNET20_CHANNELS


@functools.lru_cache(maxsize=None)
def sf_sd(seed=0, in_size=48):
    sd = W.synthetic_state_dict(W.sfnet20_param_shapes(in_size=in_size), seed=seed + 31)
    return {n: (t if n == "layer1.0.conv1.weight" or n.endswith(".bias") else t.half().float()) for n, t in sd.items()}     # the stem and the biases stay fp32


def _conv(pol, sd, name, x, stride=1):
    return pol.leaf(lambda t: F.conv2d(t, sd[name + ".weight"].to(t.dtype), sd[name + ".bias"].to(t.dtype), stride=stride, padding=1), x)


def sf_convblock(sd, name, x, pol, tag):
    """``_ConvBlock``: relu(conv stride 2) -- the stem on NCHW chips, the down convolutions on channels-last maps."""
    return pol.act(tag, _conv(pol, sd, name + ".conv1", x, 2), "relu")


def sf_block(sd, name, x, pol, tag):
    """``_BasicBlock``: relu(conv2(relu(conv1(x))) + x) -> (h, y)."""
    x = pol.gsum(x)
    h = pol.act(tag + ".h", _conv(pol, sd, name + ".conv1", x), "relu")
    s = pol.fwd(_conv(pol, sd, name + ".conv2", h) + (x.detach() if pol.mut == "res_drop" else x))
    return h, pol.act(tag + ".y", s, "relu")


def sf_forward(sd, x, pol, view, out):
    for i, n in enumerate(W.SFNET20_LAYERS):
        x = sf_convblock(sd, f"layer{i + 1}.0", x, pol, f"{view}.l{i + 1}.down")
        out[f"z.{view}.l{i + 1}.down"] = _cl(x)
        for j in range(1, n + 1):
            h, x = sf_block(sd, f"layer{i + 1}.{j}", x, pol, f"{view}.l{i + 1}.b{j}")
            out[f"z.{view}.l{i + 1}.b{j}.h"], out[f"z.{view}.l{i + 1}.b{j}.y"] = _cl(h), _cl(x)
    return pol.leaf(lambda t: F.linear(t, sd["fc.weight"].to(t.dtype), sd["fc.bias"].to(t.dtype)), torch.flatten(x, 1))


def _sf_grad(shape, seed):
    raw = torch.randn(shape, generator=_gen(seed)) * 1e-3
    gs = pow2_scale(float(raw.abs().max()))
    g = (raw * gs).half().double() / gs
    return g, gs


# piece arms: name -> (kind, layer, map size): the stem from NCHW chips, a down convolution on an odd and on an even map, a residual block on 3x3 and 6x6
SF_PIECES = {"S_stem": ("stem", 1, 10), "S_down7": ("down", 3, 7), "S_down6": ("down", 3, 6), "S_block3": ("block", 4, 3), "S_block6": ("block", 3, 6)}


def sf_piece_case(kind, layer, H, seed=0, N=2):
    sd = {n: t.double() for n, t in sf_sd(seed).items()}
    cin = 3 if kind == "stem" else SF_CH[layer - 2] if kind == "down" else SF_CH[layer - 1]
    C = SF_CH[layer - 1]
    Ho = H if kind == "block" else (H + 1) // 2
    x = _rand16((N, cin, H, H), seed + 400 + H, 0.5).clamp(-1, 1) if kind == "stem" else _rand16((N, cin, H, H), seed + 400 + H).abs()     # maps are post-ReLU
    g, gs = _sf_grad((N, C, Ho, Ho), seed + 500 + H)
    kinds = {"y": "relu", "h": "relu"} if kind == "block" else {"y": "relu"}
    return types.SimpleNamespace(kind="sfp", piece=kind, layer=layer, N=N, H=H, Ho=Ho, cin=cin, C=C, sd=sd, seed=seed, gs=gs, kinds=kinds, x=x, g=g)


def run_sf_piece(cs, variant=None, mut=None, force=None):
    pol = ImagePolicy(variant, mut, cs.gs, None if force is None else {"p." + k: v for k, v in force.items()})
    dtype = torch.float64 if variant is None else torch.float32
    x = _leaf(cs.x, dtype)
    out = {}
    if cs.piece == "block":
        h, y = sf_block(cs.sd, f"layer{cs.layer}.1", x, pol, "p")
        out["h"] = _cl(h)
    else:
        y = sf_convblock(cs.sd, f"layer{cs.layer}.0", x, pol, "p.y")
    y.backward(cs.g.to(dtype))
    out.update(y=_cl(y), dx=x.grad if cs.piece == "stem" else _cl(x.grad))
    pol.branch, pol.z = ({k[2:]: v for k, v in d.items()} for d in (pol.branch, pol.z))
    return {k: v.detach().double() for k, v in out.items()}, pol


def sf_case(seed=0, N=2, in_size=48):
    sd = {n: t.double() for n, t in sf_sd(seed, in_size).items()}
    g, gs = _sf_grad((N, 512), seed + 600)
    kinds = {}
    for v in ("v1", "v2"):
        for i, n in enumerate(W.SFNET20_LAYERS):
            kinds[f"{v}.l{i + 1}.down"] = "relu"
            for j in range(1, n + 1):
                kinds[f"{v}.l{i + 1}.b{j}.h"] = kinds[f"{v}.l{i + 1}.b{j}.y"] = "relu"
    return types.SimpleNamespace(kind="sf", N=N, S=in_size, sd=sd, seed=seed, gs=gs, kinds=kinds, g=g,
                                 chips=(torch.rand((N, 3, in_size, in_size), generator=_gen(seed + 601)) * 2 - 1).half().double())


def run_sf(cs, variant=None, mut=None, force=None):
    """``face_features`` / ``face_features_backward``: f = net(x) + net(flip(x)); dchips = d1 + flip(d2)."""
    pol = ImagePolicy(variant, None, cs.gs, force)
    dtype = torch.float64 if variant is None else torch.float32
    x1 = _leaf(cs.chips, dtype)
    x2 = _leaf(torch.flip(cs.chips, [3]), dtype)
    out = {}
    f = sf_forward(cs.sd, x1, pol, "v1", out) + sf_forward(cs.sd, x2, pol, "v2", out)
    f.backward(cs.g.to(dtype))
    out.update(f=f, dchips=x1.grad + (x2.grad if mut == "sf_no_flip" else torch.flip(x2.grad, [3])))
    return {k: v.detach().double() for k, v in out.items()}, pol


# ============================================================================= VAE decoder
VAE_GROUPS = 32
TINY_VAE = dict(block_out_channels=(32, 64, 64, 64))        # tests/util_models.py


def _draw16(shapes, seed):
    return {n: t.half().float() for n, t in W.synthetic_state_dict(shapes, seed=seed).items()}


def _scaled_grad(shape, seed, target):
    """Upstream gradient under the power-of-two scale step.py's ``_pow2_scale_dev(max|g|, target)`` gives it."""
    raw = torch.randn(shape, generator=_gen(seed)) * 1e-3
    gs = pow2_scale(float(raw.abs().max()), target)
    return (raw * gs).half().double() / gs, gs


def _hooked(pol, mod, fn):
    import warnings
    hooks = pol.install(mod)
    try:
        with warnings.catch_warnings():
            warnings.simplefilter("ignore", UserWarning)
            return fn()
    finally:
        for h in hooks:
            h.remove()


def vae_attn_forward(m, x, pol, taps=None):
    """``VAEAttention.forward`` over the module's own leaves; c: the scores, P, P.V and the residual sum rounded, as the batched GEMMs, the row softmax and the
    output GEMM's epilogue write them, and the gradients w.r.t. x (joined in ``groupnorm_bwd(add1=)``), q, k, v, the scores and P."""
    B, C, H, Wd = x.shape
    x = pol.gsum(x)
    h = m.group_norm(x).reshape(B, C, H * Wd).transpose(1, 2)
    q, k, v = (pol.gsum(l(h)) for l in (m.to_q, m.to_k, m.to_v))
    scale = C ** -0.5
    if pol.mut == "vae_dk_noscale":        # dk = dS^T q without the softmax scale
        kt = k.transpose(1, 2)
        s = torch.matmul(q, kt.detach()) * scale + (torch.matmul(q.detach(), kt) - torch.matmul(q.detach(), kt).detach())
    else:
        s = torch.matmul(q, k.transpose(1, 2)) * scale
    p = pol.fwd(pol.gsum(pol.gsum(pol.fwd(s)).softmax(dim=-1)))
    o = m.to_out[0](pol.fwd(torch.matmul(p, v)))
    if taps is not None:
        taps.update(q=q.reshape(-1, C), k=k.reshape(-1, C), v=v.reshape(-1, C), P=p)
    return pol.fwd(o.transpose(1, 2).reshape(B, C, H, Wd) + x)


def va_case(H, Wd, seed=0, B=2, C=128):
    p = "decoder.mid_block.attentions.0."
    shapes = {p + "group_norm.weight": (C,), p + "group_norm.bias": (C,)}
    for n in ("to_q", "to_k", "to_v", "to_out.0"):
        shapes[p + n + ".weight"], shapes[p + n + ".bias"] = (C, C), (C,)
    g, gs = _scaled_grad((B, C, H, Wd), seed + 702 + H, 64.0)
    return types.SimpleNamespace(kind="va", B=B, C=C, H=H, W=Wd, prefix=p, sd=_draw16(shapes, seed + 700), seed=seed, gs=gs, kinds={}, x=_rand16((B, C, H, Wd), seed + 701 + H), g=g)


def run_va(cs, variant=None, mut=None, force=None):
    from oracle import nn_vae
    pol = ImagePolicy(variant, mut, cs.gs)
    dtype = torch.float64 if variant is None else torch.float32
    m = nn_vae.VAEAttention(cs.C, VAE_GROUPS)
    m.load_state_dict({n[len(cs.prefix):]: t for n, t in cs.sd.items()}, strict=True)
    m.requires_grad_(False).to(dtype)
    x, taps = _leaf(cs.x, dtype), {}

    def fn():
        y = vae_attn_forward(m, x, pol, taps)
        y.backward(cs.g.to(dtype))
        return y
    y = _hooked(pol, m, fn)
    out = dict(out=_cl(y), dx=_cl(x.grad), **taps)
    return {k: v.detach().double() for k, v in out.items()}, pol


def vr_case(cin, cout, seed=0, B=2, H=8):
    """``ResnetBlock(has_temb=False, eps=1e-6)``: the decoder's kind (the U-Net arms R1..R5 all carry a time embedding and eps 1e-5)."""
    p = "decoder.mid_block.resnets.0."
    shapes = {p + "norm1.weight": (cin,), p + "norm1.bias": (cin,), p + "conv1.weight": (cout, cin, 3, 3), p + "conv1.bias": (cout,),
              p + "norm2.weight": (cout,), p + "norm2.bias": (cout,), p + "conv2.weight": (cout, cout, 3, 3), p + "conv2.bias": (cout,)}
    if cin != cout:
        shapes[p + "conv_shortcut.weight"], shapes[p + "conv_shortcut.bias"] = (cout, cin, 1, 1), (cout,)
    g, gs = _scaled_grad((B, cout, H, H), seed + 712 + cout, 64.0)
    return types.SimpleNamespace(kind="vr", B=B, cin=cin, cout=cout, H=H, prefix=p, sd=_draw16(shapes, seed + 710), seed=seed, gs=gs, kinds={},
                                 x=_rand16((B, cin, H, H), seed + 711 + cout), g=g)


def run_vr(cs, variant=None, mut=None, force=None):
    from oracle import nn_unet
    import block_refs as BR
    pol = ImagePolicy(variant, None, cs.gs)
    dtype = torch.float64 if variant is None else torch.float32
    m = nn_unet.ResnetBlock2D(cs.cin, cs.cout, None, VAE_GROUPS, eps=1e-6)
    m.load_state_dict({n[len(cs.prefix):]: t for n, t in cs.sd.items()}, strict=True)
    m.requires_grad_(False).to(dtype)
    x = _leaf(cs.x, dtype)

    def fn():
        y = pol.fwd(BR.resnet_forward(m, pol.gsum(x), None, pol))
        y.backward(cs.g.to(dtype))
        return y
    y = _hooked(pol, m, fn)
    return {k: v.detach().double() for k, v in dict(out=_cl(y), dx=_cl(x.grad)).items()}, pol


def vu_case(seed=0, B=2, C=64, H=5):
    p = "up."
    g, gs = _scaled_grad((B, C, 2 * H, 2 * H), seed + 722, 64.0)
    return types.SimpleNamespace(kind="vu", B=B, C=C, H=H, prefix=p, sd=_draw16({p + "conv.weight": (C, C, 3, 3), p + "conv.bias": (C,)}, seed + 720), seed=seed, gs=gs,
                                 kinds={}, x=_rand16((B, C, H, H), seed + 721), g=g)


def run_vu(cs, variant=None, mut=None, force=None):
    from oracle import nn_unet
    pol = ImagePolicy(variant, None, cs.gs)
    dtype = torch.float64 if variant is None else torch.float32
    m = nn_unet.Upsample2D(cs.C)
    m.load_state_dict({n[len(cs.prefix):]: t for n, t in cs.sd.items()}, strict=True)
    m.requires_grad_(False).to(dtype)
    x = _leaf(cs.x, dtype)

    def fn():
        y = m(x)
        y.backward(cs.g.to(dtype))
        return y
    y = _hooked(pol, m, fn)
    return {k: v.detach().double() for k, v in dict(out=_cl(y), dx=_cl(x.grad)).items()}, pol


def clamp_branches(y):
    """0 | 1 | 2: below, inside [-1, 1] (the closed interval of ``fd_clamp_bwd``), above."""
    return (y >= -1).to(torch.int8) + (y > 1).to(torch.int8)


def forced_clamp(pol, y):
    """images = clamp(y, -1, 1) under the forced branch: (the un-clamped y as the product rounds it, the image)."""
    y = pol.fwd(y)
    br = clamp_branches(y.detach()) if pol.force is None else pol.force["clamp"]
    pol.branch["clamp"], pol.z["clamp"] = br, y.detach().double()
    img = torch.where(br == 1, y, (br - 1).to(y.dtype))
    if pol.mut == "clamp_pass":         # the gradient passes through the saturated pixels
        img = img.detach() + (y - y.detach())
    return y, pol.leaf(lambda t: t, img)


def vht_case(piece, seed=0, B=2, H=6):
    """The decoder's head (conv_norm_out, SiLU, conv_out, clamp, to NCHW) or tail (post_quant_conv + conv_in) of the tiny config on a 6x6 map."""
    cfg = W.VAEConfig(**TINY_VAE)
    sd = _draw16(W.vae_param_shapes(cfg), seed + 2)
    if piece == "head":
        x, (g, gs) = _rand16((B, cfg.block_out_channels[0], H, H), seed + 751), _scaled_grad((B, 3, H, H), seed + 752, 64.0)
    else:
        x, (g, gs) = _rand16((B, 4, H, H), seed + 753), _scaled_grad((B, cfg.block_out_channels[-1], H, H), seed + 754, 64.0)
    return types.SimpleNamespace(kind="vht", piece=piece, B=B, H=H, cfg=cfg, sd=sd, seed=seed, gs=gs, kinds={"clamp": "clamp"} if piece == "head" else {}, x=x, g=g)


def run_vht(cs, variant=None, mut=None, force=None):
    import torch.nn as nn
    pol = ImagePolicy(variant, mut, cs.gs, force)
    dtype = torch.float64 if variant is None else torch.float32
    boc = cs.cfg.block_out_channels
    if cs.piece == "head":
        m = nn.ModuleDict(dict(norm=nn.GroupNorm(VAE_GROUPS, boc[0], eps=1e-6), conv=nn.Conv2d(boc[0], 3, 3, padding=1)))
        names = {"norm": "decoder.conv_norm_out", "conv": "decoder.conv_out"}
    else:
        m = nn.ModuleDict(dict(pq=nn.Conv2d(4, 4, 1), conv=nn.Conv2d(4, boc[-1], 3, padding=1)))
        names = {"pq": "post_quant_conv", "conv": "decoder.conv_in"}
    m.load_state_dict({f"{k}.{w}": cs.sd[f"{n}.{w}"] for k, n in names.items() for w in ("weight", "bias")}, strict=True)
    m.requires_grad_(False).to(dtype)
    x = _leaf(cs.x, dtype)

    def fn():
        if cs.piece == "head":
            y, out = forced_clamp(pol, m["conv"](F.silu(m["norm"](x))))
        else:
            y = out = m["conv"](m["pq"](x))
        out.backward(cs.g.to(dtype))
        return y, out
    y, out = _hooked(pol, m, fn)
    res = dict(img=out, dx=_cl(x.grad), **{"z.clamp": y}) if cs.piece == "head" else dict(out=_cl(out), dz=x.grad)
    return {k: v.detach().double() for k, v in res.items()}, pol


def vae_case(seed=0, B=2, H=8):
    """The whole decoder at util_models' tiny config on 8x8 latents: image [B, 3, 64, 64] (clamped) and dz."""
    cfg = W.VAEConfig(**TINY_VAE)
    g, gs = _scaled_grad((B, 3, 8 * H, 8 * H), seed + 732, 64.0)
    return types.SimpleNamespace(kind="vae", B=B, H=H, cfg=cfg, sd=_draw16(W.vae_param_shapes(cfg), seed + 2), seed=seed, gs=gs, kinds={"clamp": "clamp"},
                                 z=_rand16((B, 4, H, H), seed + 731), g=g)


def run_vae(cs, variant=None, mut=None, force=None):
    from oracle import nn_vae
    pol = ImagePolicy(variant, mut, cs.gs, force)
    dtype = torch.float64 if variant is None else torch.float32
    m = nn_vae.AutoencoderKLDecoder(nn_vae.VAEConfig(**TINY_VAE))
    m.load_state_dict(cs.sd, strict=True)
    m.requires_grad_(False).to(dtype)
    att = m.decoder.mid_block.attentions[0]
    att.forward = lambda x: vae_attn_forward(att, x, pol)
    z = _leaf(cs.z, dtype)

    def fn():
        y, img = forced_clamp(pol, m.decode(z).sample)
        img.backward(cs.g.to(dtype))
        return y, img
    y, img = _hooked(pol, m, fn)
    return {k: v.detach().double() for k, v in dict(img=img, dz=z.grad, **{"z.clamp": y}).items()}, pol


BREAKS["clamp"] = (-1.0, 1.0)


# ============================================================================= the two ViTs
VIT_TINY = dict(        # tests/test_engine_gpu.py: g = 4, 17 tokens padded to 24
    clip=dict(kind="clip", image_size=56, patch_size=14, hidden_size=160, num_hidden_layers=3, num_attention_heads=2, intermediate_size=320,
              projection_dim=48, layer_norm_eps=1e-5, pos_grid=4),
    dino=dict(kind="dino", image_size=56, patch_size=14, hidden_size=128, num_hidden_layers=3, num_attention_heads=2, intermediate_size=256,
              projection_dim=0, layer_norm_eps=1e-6, pos_grid=6))


def vit_product_numbers(kind, sd, rounded=True):
    """(oracle config, oracle state dict, LayerScale vectors) holding the numbers the product multiplies with: linear and patch weights fp16, biases and norms fp32,
    the class token plus its position and the patch positions fp16 (DINOv2: after the bicubic interpolation of the table), LayerScale folded into the
    projection it follows as ``vit._Lin`` folds it (in fp64, then fp16) -- the oracle's own ``gamma`` becomes 1."""
    from oracle import nn_vit as OV
    cfg = dict(VIT_TINY[kind])
    g = cfg["image_size"] // cfg["patch_size"]
    out, gammas = {}, {}
    r16, _r32 = (globals()["r16"], globals()["_r32"]) if rounded else ((lambda t: t), (lambda t: t))        # ``rounded=False``: the exact fold
    for n, t in sd.items():
        t = t.double()
        out[n] = r16(t) if (t.dim() >= 2 and "position" not in n and "pos_embed" not in n and "cls_token" not in n) else _r32(t)
    if kind == "clip":
        e = "vision_model.embeddings."
        pos = sd[e + "position_embedding.weight"].double()
        out[e + "class_embedding"] = r16(sd[e + "class_embedding"].double() + pos[0])
        out[e + "position_embedding.weight"] = torch.cat([torch.zeros(1, pos.shape[1], dtype=torch.float64), r16(pos[1:])])
    else:
        pos = OV.interpolate_pos_encoding(sd["pos_embed"].float(), g).double()
        out["cls_token"] = r16(sd["cls_token"].double() + pos[:, :1])
        out["pos_embed"] = torch.cat([torch.zeros(1, 1, pos.shape[2], dtype=torch.float64), r16(pos[:, 1:])], 1)
        cfg["pos_grid"] = g
        for i in range(cfg["num_hidden_layers"]):
            for ls, lin in (("ls1", "attn.proj"), ("ls2", "mlp.fc2")):
                gam = sd[f"blocks.{i}.{ls}.gamma"].double()
                gammas[f"blocks.{i}.{lin}"] = gam
                out[f"blocks.{i}.{lin}.weight"] = r16(sd[f"blocks.{i}.{lin}.weight"].double() * gam[:, None])
                out[f"blocks.{i}.{lin}.bias"] = _r32(sd[f"blocks.{i}.{lin}.bias"].double() * gam)
                out[f"blocks.{i}.{ls}.gamma"] = torch.ones_like(gam)
    return cfg, out, gammas


def _unscaled_grad(y, gam):
    """Forward value y, gradient as if the LayerScale ``gam`` folded into the projection were missing (mutation)."""
    return y.detach() + (y / gam - (y / gam).detach())


def vit_forward(m, cfg, chips, mean, std, pol, taps, pad=0, gammas=None):
    """The two oracle towers' ``forward`` over their own leaves on ((x + 1) / 2 - mean) / std; taps: each layer's h1 / h2 [N, T, D].  c: the normalised pixels
    (``fd_patchify`` writes fp16), the embedding sum, P, the attention output, each residual sum; gradients w.r.t. q, k, v and at the two fan-outs.
    ``pad``: extra zero tokens appended and attended over (mutation: the keys of rows T..Tp not masked)."""
    clip = cfg["kind"] == "clip"
    heads = cfg["num_attention_heads"]
    mt = torch.tensor(mean, dtype=chips.dtype).view(1, 3, 1, 1)
    st = torch.tensor(std, dtype=chips.dtype).view(1, 3, 1, 1)
    px = pol.fwd(((chips + 1) * 0.5 - mt) / st)
    if clip:
        vm = m.vision_model
        p = vm.embeddings.patch_embedding(px).flatten(2).transpose(1, 2)
        x = torch.cat([vm.embeddings.class_embedding.expand(p.shape[0], 1, -1), p], dim=1) + vm.embeddings.position_embedding.weight[None]
        layers, final = vm.encoder.layers, vm.post_layernorm
    else:
        p = m.patch_embed.proj(px).flatten(2).transpose(1, 2)
        x = torch.cat([m.cls_token.expand(p.shape[0], -1, -1), p], dim=1) + m.pos_embed
        layers, final = m.blocks, m.norm
    x = pol.fwd(x)
    T = x.shape[1]
    if pad:
        x = torch.cat([x, x.new_zeros(x.shape[0], pad, x.shape[2])], dim=1)
    if clip:
        x = vm.pre_layrnorm(x)
    for i, L in enumerate(layers):
        x = pol.gsum(x)
        h = (L.layer_norm1 if clip else L.norm1)(x)
        if clip:
            a = L.self_attn
            q, k, v = a.q_proj(h), a.k_proj(h), a.v_proj(h)
            proj, key = a.out_proj, None
        else:
            q, k, v = L.attn.qkv(h).chunk(3, dim=-1)
            proj, key = L.attn.proj, f"blocks.{i}.attn.proj"
        B, Tt, D = x.shape
        d = D // heads
        sh = lambda t: pol.gsum(t).reshape(B, Tt, heads, d).transpose(1, 2)  # noqa: E731
        pr = torch.softmax((sh(q) * d ** -0.5) @ sh(k).transpose(-1, -2), dim=-1)
        at = pol.fwd((pol.fwd(pr) @ sh(v)).transpose(1, 2).reshape(B, Tt, D))
        o = proj(at)
        if pol.mut == "vit_no_layerscale" and key is not None:
            o = _unscaled_grad(o, gammas[key].to(o.dtype))
        x = pol.gsum(pol.fwd(x + o))
        taps[f"h1.{i}"] = x[:, :T]
        h = (L.layer_norm2 if clip else L.norm2)(x)
        f = L.mlp.fc2(pol.leaf(F.gelu, L.mlp.fc1(h)))
        if pol.mut == "vit_no_layerscale" and key is not None:
            f = _unscaled_grad(f, gammas[f"blocks.{i}.mlp.fc2"].to(f.dtype))
        x = pol.fwd(x + f)
        taps[f"h2.{i}"] = x[:, :T]
    y = final(x[:, 0])
    return m.visual_projection(y) if clip else y


def vit_case(kind, seed=0, N=3):
    cfg = W.ViTConfig(**VIT_TINY[kind])
    sd = W.synthetic_state_dict(W.vit_param_shapes(cfg), seed=seed + 11)
    ocfg, osd, gammas = vit_product_numbers(kind, sd)
    mean, std = (W.CLIP_IMAGE_MEAN, W.CLIP_IMAGE_STD) if kind == "clip" else (W.DINO_IMAGE_MEAN, W.DINO_IMAGE_STD)
    E = cfg.projection_dim if kind == "clip" else cfg.hidden_size
    g, gs = _scaled_grad((N, E), seed + 741, 1.0)
    gg = cfg.image_size // cfg.patch_size
    return types.SimpleNamespace(kind="vit", vkind=kind, N=N, cfg=cfg, ocfg=ocfg, sd=sd, osd=osd, gammas=gammas, mean=mean, std=std, seed=seed, gs=gs, kinds={}, g=g,
                                 T=gg * gg + 1, Tp=(gg * gg + 1 + 7) // 8 * 8,
                                 chips=(torch.rand((N, 3, cfg.image_size, cfg.image_size), generator=_gen(seed + 740)) * 2 - 1).half().double())


def build_vit(cs, dtype):
    from oracle import nn_vit as OV
    m = (OV.CLIPVisionModelWithProjection if cs.vkind == "clip" else OV.DinoVisionTransformer)(OV.ViTConfig(**cs.ocfg))
    m.load_state_dict(cs.osd, strict=True)
    return m.eval().requires_grad_(False).to(dtype)


def run_vit(cs, variant=None, mut=None, force=None):
    pol = ImagePolicy(variant, mut, cs.gs)
    dtype = torch.float64 if variant is None else torch.float32
    m = build_vit(cs, dtype)
    chips, taps = _leaf(cs.chips, dtype), {}

    def fn():
        e = vit_forward(m, cs.ocfg, chips, cs.mean, cs.std, pol, taps, pad=(cs.Tp - cs.T) if mut == "vit_keys_tp" else 0, gammas=cs.gammas)
        e.backward(cs.g.to(dtype))
        return e
    e = _hooked(pol, m, fn)
    last = taps.pop(f"h2.{cs.cfg.num_hidden_layers - 1}")          # the product keeps the last layer's output as its class-token rows alone
    out = dict(emb=e, dchips=chips.grad, cls=last[:, 0], **{k: t.reshape(-1, t.shape[-1]) for k, t in taps.items()})
    return {k: v.detach().double() for k, v in out.items()}, pol


# ============================================================================= arms, mutations
CASES = {arm: (mb_case, kw) for arm, kw in MB_ARMS.items()}
CASES.update({arm: (sf_piece_case, dict(kind=k, layer=l, H=h)) for arm, (k, l, h) in SF_PIECES.items()})
CASES.update({"SH": (sh_case, {}), "CLF": (clf_case, {}), "SF": (sf_case, {})})
CASES.update({"VA64": (va_case, dict(H=8, Wd=8)), "VA40": (va_case, dict(H=5, Wd=8)), "VR_same": (vr_case, dict(cin=64, cout=64)), "VR_short": (vr_case, dict(cin=64, cout=128)),
              "VU": (vu_case, {}), "VH": (vht_case, dict(piece="head")), "VT": (vht_case, dict(piece="tail")), "VAE": (vae_case, {}), "CLIP": (vit_case, dict(kind="clip")), "DINO": (vit_case, dict(kind="dino"))})
NET_ARMS = ("CLF", "SF", "VAE", "CLIP", "DINO")            # whole networks: a margin of their own
RUN = {"mb": run_mb, "sh": run_sh, "clf": run_clf, "sfp": run_sf_piece, "sf": run_sf, "va": run_va, "vr": run_vr, "vu": run_vu, "vht": run_vht, "vae": run_vae, "vit": run_vit}

# name -> (arms, the tensors it must move, for CLF: the blocks it acts in)
_SE_BLOCKS = tuple(i for i, s in enumerate(W.MBV3_SETTINGS) if s[3])
_RES_BLOCKS = tuple(i for i in range(len(W.MBV3_SETTINGS)) if mb_config(i)[4])
MUTATIONS = {
    "se_no_pool": (("B3", "B10", "CLF"), ("dx", "dchips") + tuple(f"trace{i}" for i in range(13)), (12,)),      # ONE of fifteen blocks drops a path
    "se_no_direct": (("B3", "B10", "CLF"), ("dx", "dchips") + tuple(f"trace{i}" for i in range(13)), (12,)),
    "res_drop": (("B0", "B2", "B11", "S_block3", "CLF"), ("dx", "dchips") + tuple(f"trace{i}" for i in range(8)), (7,)),
    "dw_shift": (("B3", "B12"), ("dx",), ()),
    "hsig_outside": (("B3", "B10"), ("dx",), ()),
    "sf_no_flip": (("SF",), ("dchips",), ()),
    "clamp_pass": (("VH", "VAE"), ("dx", "dz"), ()),
    "vae_dk_noscale": (("VA64", "VA40"), ("dx",), ()),
    "vit_keys_tp": (("CLIP", "DINO"), ("emb", "dchips", "cls", "h1.0", "h2.0", "h1.1", "h2.1", "h1.2"), ()),
    "vit_no_layerscale": (("DINO",), ("dchips",), ()),
}
MUTATION_ARMS = tuple(sorted({a for arms, _, _ in MUTATIONS.values() for a in arms}))


def moved_keys(arm, mut, ref):
    return [k for k in ref if k in MUTATIONS[mut][1]]


@functools.lru_cache(maxsize=None)
def case(arm, seed=0):
    fn, kw = CASES[arm]
    return fn(seed=seed, **kw)


def run(cs, variant=None, mut=None, force=None):
    return RUN[cs.kind](cs, variant, mut, force)


@functools.lru_cache(maxsize=None)
def own_reference(arm, seed=0):
    """The unforced fp64 reference: (tensors, policy with its branches and pre-activations)."""
    return run(case(arm, seed))


def reference(arm, branch, mut=None, seed=0):
    """The fp64 reference of ``arm`` under a candidate's branches."""
    return run(case(arm, seed), None, mut, branch)[0]


@functools.lru_cache(maxsize=None)
def emulation(arm, variant):
    """(tensors, branches, reference under those branches) of one emulation variant."""
    seed, v = (1, "a") if variant == "e" else (0, variant)
    got, pol = run(case(arm, seed), v)
    return got, pol.branch, reference(arm, pol.branch, None, seed)


@functools.lru_cache(maxsize=None)
def emulation_stats(arm):
    """{tensor: {variant: (e2, emax)}} of each emulation variant against the fp64 reference under that variant's branches."""
    stats = {}
    for v in VARIANTS:
        got, _, ref = emulation(arm, v)
        for k in ref:
            stats.setdefault(k, {})[v] = metric(got[k], ref[k])
    return stats


def emulation_flips(arm, variant):
    seed = 1 if variant == "e" else 0
    return flips(emulation(arm, variant)[1], own_reference(arm, seed)[1], case(arm, seed).kinds)


FORWARD = ("out", "z_exp", "z_dw", "z1", "z2", "se_s", "z0", "x0", "zl", "zf", "logits", "y", "h", "f", "q", "k", "v", "P", "img", "emb", "cls")


def is_forward(key):
    return key in FORWARD or key.startswith("z.") or key.startswith("h1.") or key.startswith("h2.")


def bands(arm):
    """{tensor: (band_e2, band_emax, emul_e2, emul_emax)}: the margins of tests/image_bands.py over the largest emulation statistic, never above the caps."""
    import image_bands as IB
    net = arm in NET_ARMS
    m2, mm = (IB.MARGIN_E2_NET, IB.MARGIN_MAX_NET) if net else (IB.MARGIN_E2, IB.MARGIN_MAX)
    out = {}
    for k, sv in emulation_stats(arm).items():
        e2, em = max(v[0] for v in sv.values()), max(v[1] for v in sv.values())
        cap = CAP_FWD if is_forward(k) else CAP_GRAD
        out[k] = (min(m2 * e2, cap), min(mm * em, cap), e2, em)
    return out


def check_flips(arm, branch, report=print):
    """The two conditions on a candidate's masks: at most FLIP_CAP of a mask's elements off the unforced reference's branch, each within that tensor's emax band
    x max|z_ref| of the break point.  Returns (flipped elements, all elements)."""
    cs, b = case(arm), bands(arm)
    tot = [0, 0]
    bad = []
    for name, (share, n, dist, zmax) in flips(branch, own_reference(arm)[1], cs.kinds).items():
        key = name if name in b else "z." + name
        lim = b[key][1] * zmax
        tot[0] += round(share * n)
        tot[1] += n
        if share:
            report(f"[{arm}] mask {name:16s} {share * 100:.3f} % of {n} off the reference's branch; farthest {dist:.3e} from its break (limit {lim:.3e})")
        if share > FLIP_CAP or dist > lim:
            bad.append(f"{name}: {share * 100:.3f} % flipped, farthest {dist:.3e} (limit {lim:.3e})")
    assert not bad, f"{arm}: " + "; ".join(bad)
    return tuple(tot)
