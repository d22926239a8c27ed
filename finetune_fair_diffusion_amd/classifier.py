"""MI355X-native mirror of torchvision ``mobilenet_v3_large`` (eval mode, BatchNorm folded into the
convolutions) -- the face-attribute classifier of exp-1-debias-gender/1-main-debias.py:929-935 --
with the forward that scores face chips (:1369-1371) and the explicit data-gradient backward that
carries dL/dlogits back to the face chips (the reference gets it from autograd through the frozen
classifier).  Pointwise convolutions run on the MFMA GEMM, depthwise / squeeze-excite pieces on
the direct kernels of smallconv.hip.

``ZeroShotClipClassifier`` (a build addition, ``--experiment custom --classifier zero_shot``) offers the same ``forward`` / ``backward`` seam with no
trained head: the CLIP ViT-H/14 image tower and one unit vector per class prompt, logit = logit_scale * cos(image embedding, class direction).
"""
import torch

from . import ops
from .layers import F16, F32
from .weights import MBV3_SETTINGS, make_divisible, mobilenet_param_shapes


def _fold(sd, p, dev):
    """conv (p+'0') followed by BatchNorm (p+'1', eps 1e-3) -> (weight', bias')."""
    w = sd[p + "0.weight"].to(dev, F32)
    g, b = sd[p + "1.weight"].to(dev, F32), sd[p + "1.bias"].to(dev, F32)
    m, v = sd[p + "1.running_mean"].to(dev, F32), sd[p + "1.running_var"].to(dev, F32)
    s = g / torch.sqrt(v + 1e-3)
    return w * s.view(-1, 1, 1, 1), b - m * s


class _PW:  # pointwise conv / linear on the GEMM
    def __init__(self, w, b):
        self.w = w.reshape(w.shape[0], -1).to(F16).contiguous()
        self.bias = b.to(F32).contiguous()
        self.wT = self.w.t().contiguous()


class _DW:
    def __init__(self, w, b, k, stride):
        C = w.shape[0]
        self.w = w.reshape(C, k * k).t().contiguous()  # [k*k, C] fp32
        self.bias = b.contiguous()
        self.k, self.stride = k, stride


class MobileNetV3Large:
    def __init__(self, state_dict, device, num_classes=80):
        sd, dev = state_dict, device
        missing = [k for k in mobilenet_param_shapes(num_classes) if k not in sd]
        if missing:
            raise KeyError(f"classifier state_dict is missing {len(missing)} tensors, e.g. {missing[:3]}")
        self.device, self.num_classes = dev, num_classes
        w, b = _fold(sd, "features.0.", dev)
        self.stem_w = w.permute(2, 3, 1, 0).reshape(27, 16).contiguous()
        self.stem_b = b.contiguous()
        self.blocks = []
        cin = 16
        for i, (k, exp, cout, se, act, s) in enumerate(MBV3_SETTINGS):
            p = f"features.{i + 1}.block."
            j = 0
            blk = dict(k=k, exp=exp, cout=cout, act=act, stride=s, res=(s == 1 and cin == cout), expand=None, se=None)
            if exp != cin:
                blk["expand"] = _PW(*_fold(sd, p + f"{j}.", dev)); j += 1
            w, b = _fold(sd, p + f"{j}.", dev)
            blk["dw"] = _DW(w, b, k, s); j += 1
            if se:
                blk["se"] = (_PW(sd[p + f"{j}.fc1.weight"].to(dev, F32), sd[p + f"{j}.fc1.bias"].to(dev)),
                             _PW(sd[p + f"{j}.fc2.weight"].to(dev, F32), sd[p + f"{j}.fc2.bias"].to(dev)))
                j += 1
            blk["project"] = _PW(*_fold(sd, p + f"{j}.", dev))
            self.blocks.append(blk)
            cin = cout
        self.last = _PW(*_fold(sd, "features.16.", dev))
        self.fc1 = _PW(sd["classifier.0.weight"].to(dev, F32), sd["classifier.0.bias"].to(dev))
        # head padded to a multiple of 8 logits (16-byte GEMM rows); the pad columns are zero weights, sliced off on return
        self.ncls_pad = (num_classes + 7) // 8 * 8
        w2 = torch.zeros(self.ncls_pad, 1280, dtype=F32, device=dev)
        b2 = torch.zeros(self.ncls_pad, dtype=F32, device=dev)
        w2[:num_classes] = sd["classifier.3.weight"].to(dev, F32)
        b2[:num_classes] = sd["classifier.3.bias"].to(dev, F32)
        self.fc2 = _PW(w2, b2)
        self._ctx = None

    # The recording and the non-recording forward run the SAME kernel sequence (pre-activation rounded to the working dtype, then the
    # activation): the no-grad R1 pass that yields the dynamic targets and the R3 pass whose logits enter the loss are two evaluations of
    # one function in the reference (:1794-1795, :1899-1903) and must agree to the bit here too -- with the activation fused into the
    # GEMM epilogue (applied to the fp32 accumulator) only in the non-recording pass, near-tied probabilities could rank differently in the
    # two passes and flip a target (seen at B = 8 on the random-weight test classifier).  ``record`` only decides what is KEPT.
    @staticmethod
    def _pw(x, lin, act, record, residual=None):
        """1x1 conv + folded BN (+act)(+residual).  Returns (output, pre-activation or None)."""
        if act == "none":
            return ops.gemm(x, lin.w, bias=lin.bias, act=act, residual=residual), None
        z = ops.gemm(x, lin.w, bias=lin.bias)
        return ops.act_fwd(z, act), (z if record else None)

    def stem_forward(self, chips, record):
        """chips [B,3,S,S] -> (x [B*H*W, 16], H, W, record or None)."""
        B, _, H, W = chips.shape
        z0, H, W = ops.conv_small_cin(chips, self.stem_w, self.stem_b, B, H, W, 3, 16, 3, 2, nchw=True)
        x = ops.act_fwd(z0, "hardswish")
        return x, H, W, (dict(z0=z0, H0=chips.shape[2], W0=chips.shape[3]) if record else None)

    def block_forward(self, i, x, B, H, W, record):
        """Inverted-residual block ``i`` on x [B*H*W, cin] -> (y [B*Ho*Wo, cout], Ho, Wo, record or None)."""
        blk = self.blocks[i]
        c = dict(H=H, W=W) if record else None
        inp = x
        act = blk["act"]
        if blk["expand"] is not None:
            x, z = self._pw(x, blk["expand"], act, record)
            if record:
                c["z_exp"] = z
        dw = blk["dw"]
        zd, Ho, Wo = ops.dwconv(x, dw.w, dw.bias, B, H, W, blk["exp"], dw.k, dw.stride, "none")
        x = ops.act_fwd(zd, act)
        if record:
            c["z_dw"] = zd
        H, W = Ho, Wo
        if blk["se"] is not None:
            fc1, fc2 = blk["se"]
            avg = ops.avgpool_hw(x, B, H * W, blk["exp"])
            a1, z1 = self._pw(avg, fc1, "relu", record)
            s, z2 = self._pw(a1, fc2, "hardsigmoid", record)
            y = ops.scale_channels(x, s, B, H * W, blk["exp"])
            if record:
                c.update(se_x=x, se_s=s, z1=z1, z2=z2)
            x = y
        x, _ = self._pw(x, blk["project"], "none", record, residual=inp if blk["res"] else None)
        if record:
            c.update(Ho=H, Wo=W)
        return x, H, W, c

    def head_forward(self, x, B, H, W, record):
        """x [B*H*W, 160] -> (logits [B, ncls_pad], record or None)."""
        x, zl = self._pw(x, self.last, "hardswish", record)
        HWl = H * W
        avg = ops.avgpool_hw(x, B, HWl, 960)
        h, zf = self._pw(avg, self.fc1, "hardswish", record)
        logits, _ = self._pw(h, self.fc2, "none", record)
        return logits, (dict(zl=zl, zf=zf, HWl=HWl, B=B) if record else None)

    def forward(self, chips, record=False):
        """chips: [B,3,S,S] fp16 NCHW.  Returns logits [B, num_classes] fp16."""
        B = chips.shape[0]
        ctx = [] if record else None
        x, H, W, c = self.stem_forward(chips, record)
        if record:
            ctx.append(c)
        for i in range(len(self.blocks)):
            x, H, W, c = self.block_forward(i, x, B, H, W, record)
            if record:
                ctx.append(c)
        logits, c = self.head_forward(x, B, H, W, record)
        if record:
            self._ctx = dict(blocks=ctx, **c)
        return logits[:, :self.num_classes]

    __call__ = forward

    def head_backward(self, c, d_logits, gscale):
        """d_logits [B, num_classes] fp32 -> the scaled fp16 gradient of the head's input [B*HWl, 160]."""
        B = c["B"]
        dl = d_logits
        if self.ncls_pad != self.num_classes:
            dl = torch.zeros((B, self.ncls_pad), dtype=F32, device=d_logits.device)
            dl[:, :self.num_classes] = d_logits
        d = ops.to_f16(dl.contiguous(), gscale)
        d = ops.gemm(d, self.fc2.wT)
        d = ops.act_bwd(c["zf"], d, "hardswish")
        d = ops.gemm(d, self.fc1.wT)                                   # [B, 960] grad of the pooled features
        d = ops.avgpool_hw_bwd(d, B, c["HWl"], 960)
        d = ops.act_bwd(c["zl"], d, "hardswish")
        return ops.gemm(d, self.last.wT)

    def block_backward(self, i, cb, d, B):
        """The scaled fp16 gradient of block ``i``'s output -> that of its input; ``cb``: the block's record."""
        blk = self.blocks[i]
        H, W, Ho, Wo = cb["H"], cb["W"], cb["Ho"], cb["Wo"]
        d_res = d if blk["res"] else None
        d = ops.gemm(d, blk["project"].wT)                          # grad wrt SE output / dw activation
        if blk["se"] is not None:
            fc1, fc2 = blk["se"]
            dx, ds = ops.scale_channels_bwd(cb["se_x"], cb["se_s"], d, B, Ho * Wo, blk["exp"])
            dz2 = ops.act_bwd(cb["z2"], ds, "hardsigmoid")
            da1 = ops.gemm(dz2, fc2.wT)
            dz1 = ops.act_bwd(cb["z1"], da1, "relu")
            davg = ops.gemm(dz1, fc1.wT)
            d = ops.avgpool_hw_bwd(davg, B, Ho * Wo, blk["exp"], add=dx)
        d = ops.act_bwd(cb["z_dw"], d, blk["act"])
        dw = blk["dw"]
        d = ops.dwconv_bwd(d, dw.w, B, H, W, blk["exp"], dw.k, dw.stride)
        if blk["expand"] is not None:
            d = ops.act_bwd(cb["z_exp"], d, blk["act"])
            d = ops.gemm(d, blk["expand"].wT, residual=d_res)
        elif d_res is not None:
            d = ops.add(d, d_res)
        return d

    def stem_backward(self, c0, d, B, gscale):
        d = ops.act_bwd(c0["z0"], d, "hardswish")
        return ops.conv_small_cin_bwd(d, self.stem_w, B, c0["H0"], c0["W0"], 3, 16, 3, 2, scale=1.0 / gscale)

    def backward(self, d_logits, gscale, trace=None):
        """d_logits: [B, num_classes] fp32 = dL/dlogits.  Returns dL/dchips [B,3,S,S] fp32.  ``trace``: a list that receives the (scaled, fp16)
        gradient at every block's input, last block first."""
        c = self._ctx
        B, blocks = c["B"], c["blocks"]
        d = self.head_backward(c, d_logits, gscale)
        for i in reversed(range(len(self.blocks))):
            d = self.block_backward(i, blocks.pop(), d, B)
            if trace is not None:
                trace.append(d)
        dchips = self.stem_backward(blocks.pop(), d, B, gscale)
        self._ctx = None
        return dchips


class ZeroShotClipClassifier:
    """Zero-shot CLIP attribute classifier behind ``MobileNetV3Large``'s seam: ``forward(chips, record) -> logits [B, num_classes]``,
    ``backward(d_logits, gscale) -> dL/dchips [B,3,S,S] fp32``, ``num_classes``, ``_ctx``.

    ``tower``: a ``vit.VisionTransformer`` of kind "clip" that belongs to this classifier alone (``VisionTransformer.sharing(other)`` makes one on the
    weight tensors of the regulariser's tower; the recorded forwards are never shared).  ``t_hat`` [K, E]: one direction per class prompt, the logit
    columns in prompt order (``class_directions``); they are normalised here, in fp32.  ``logit_scale``: CLIP's ``exp(logit_scale)``.

    The recording and the non-recording forward run the SAME kernel sequence -- the tower's recording one, whose GELU is a kernel of its own; its
    non-recording forward fuses the GELU into the GEMM epilogue and differs by ~2e-3 -- so that R1's targets and R3's loss see equal bits (the comment
    above ``MobileNetV3Large._pw``); ``record`` only decides what is kept.  The head (``ops.cosine_logits``) is fp32 with a fixed summation order."""

    def __init__(self, tower, t_hat, logit_scale):
        if tower.proj is None:
            raise ValueError("ZeroShotClipClassifier needs a CLIP image tower (one with visual_projection)")
        K, E = t_hat.shape
        if E != tower.out_dim or not 1 <= K <= 16:
            raise ValueError(f"class directions [{K}, {E}]: the tower embeds into {tower.out_dim} dimensions, and 1..16 classes are supported")
        self.tower, self.device, self.num_classes = tower, tower.device, K
        self.t_hat = torch.nn.functional.normalize(t_hat.to(self.device, F32), dim=-1).contiguous()
        self.logit_scale = float(logit_scale)
        self._ctx = None

    def forward(self, chips, record=False):
        """chips: [B,3,S,S] working dtype NCHW in [-1,1], S = the tower's image size.  Returns logits [B, num_classes] fp32."""
        if chips.shape[2] != self.tower.config.image_size or chips.shape[3] != self.tower.config.image_size:
            raise ValueError(f"chips of {tuple(chips.shape[2:])}: the CLIP tower takes {self.tower.config.image_size} x {self.tower.config.image_size} (--size_face)")
        e = self.tower.forward(chips, record=True)
        rec, self.tower._ctx = self.tower._ctx, None          # the tower object never holds a record of ours between calls
        logits, inv_norm = ops.cosine_logits(e, self.t_hat, self.logit_scale)
        if record:
            self._ctx = dict(tower=rec, e=e, logits=logits, inv_norm=inv_norm)
        return logits

    __call__ = forward

    def backward(self, d_logits, gscale):
        """d_logits: [B, num_classes] fp32 = dL/dlogits.  Returns dL/dchips [B,3,S,S] fp32; the recorded forward is consumed."""
        c, self._ctx = self._ctx, None
        d_e = ops.cosine_logits_bwd(c["e"], self.t_hat, c["logits"], c["inv_norm"], d_logits.to(F32).contiguous(), self.logit_scale)
        self.tower._ctx = c["tower"]
        return self.tower.backward(d_e, gscale)


def class_directions(text_tower, input_ids):
    """[K, E] fp32 unit vectors on the device: ``normalize(text_embeds)`` of the tokenised class prompts ``input_ids`` [K, T] (host, int64)."""
    return torch.nn.functional.normalize(text_tower.text_embeds(input_ids).float(), dim=-1).contiguous()
