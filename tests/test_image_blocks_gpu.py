"""The image-side networks' hand-written forwards and backwards -- ``MobileNetV3Large`` (classifier.py), ``SFNet20`` with its mirrored second view (sfnet.py), the
VAE decoder (vae.py: ``VAEAttention``, ``ResnetBlock`` without a time embedding, ``conv_up2``, the whole ``AutoencoderKL``) and the two ViT towers (vit.py) --
block by block and as whole networks, tensor by tensor, against the fp64 oracle arithmetic under the product's own activation branches
(tests/image_refs.py: references, forced branches, emulations, mutations; tests/image_bands.py: margins).

Every tensor is held to  e2 <= MARGIN_E2 x (largest e2 of the fp16-rounding emulations)  and the same for emax.  The branches (ReLU, hardswish, hardsigmoid)
are read from the product's records and forced on the reference; per mask at most 1 % of the elements may differ from the unforced reference's own branch, each
within that tensor's band of the break point.  References are computed on the host, once per arm and set of branches."""
import pytest
import torch

import image_bands as IB
import image_refs as R

pytestmark = pytest.mark.gpu
H16, F32 = torch.float16, torch.float32
SUMMARY = {}        # network -> [largest e2 / emulation, largest emax / emulation, flipped mask elements, mask elements]


@pytest.fixture(scope="module")
def ops():
    from finetune_fair_diffusion_amd import ops
    assert ops.F16 == H16
    return ops


def _cl16(t, dev, scale=1.0):
    return R._cl(t * scale).half().contiguous().to(dev)


def _nchw(t, B, H, W):
    """The product's [B*H*W, C] -> the reference's [B, C, H, W], on the host."""
    return t.detach().cpu().view(B, H, W, -1).permute(0, 3, 1, 2)


def _host(out):
    torch.cuda.synchronize()
    for k, t in out.items():
        assert bool(torch.isfinite(t).all()), f"{k}: not finite"
    return {k: t.detach().double().cpu() for k, t in out.items()}


def gate(arm, got, branch, net):
    """Every reference tensor of ``arm``, computed under the product's branches, under its band; prints each figure, then asserts.  The masks themselves are
    held to the cap and the distance condition first."""
    flipped, total = R.check_flips(arm, branch)
    ref, bands = R.reference(arm, branch), R.bands(arm)
    m2, mm = (IB.MARGIN_E2_NET, IB.MARGIN_MAX_NET) if arm in R.NET_ARMS else (IB.MARGIN_E2, IB.MARGIN_MAX)
    bad, worst = [], [(0.0, None), (0.0, None)]
    for k in ref:
        e2, em = R.metric(got[k], ref[k])
        b2, bm, u2, um = bands[k]
        print(f"[{arm}] {k:18s} e2 {e2:.3e} = {e2 / u2:.2f} x emulation (band {b2:.2e})   emax {em:.3e} = {em / um:.2f} x emulation (band {bm:.2e})")
        worst = [max(worst[0], (e2 / u2, k)), max(worst[1], (em / um, k))]
        if not (e2 <= b2 and em <= bm):
            bad.append(f"{k}: e2 {e2:.3e} (band {b2:.2e}), emax {em:.3e} (band {bm:.2e})")
    print(f"[{arm}] largest e2 / emulation {worst[0][0]:.2f} on {worst[0][1]} (margin {m2}); emax {worst[1][0]:.2f} on {worst[1][1]} (margin {mm}); "
          f"{flipped} of {total} mask elements ({100.0 * flipped / max(total, 1):.4f} %) forced off the reference's own branch (cap {100 * R.FLIP_CAP:.0f} % per mask)")
    s = SUMMARY.setdefault(net, [0.0, 0.0, 0, 0])
    s[:] = [max(s[0], worst[0][0]), max(s[1], worst[1][0]), s[2] + flipped, s[3] + total]
    assert not bad, f"{arm}: " + "; ".join(bad)


# ============================================================================= MobileNetV3
@pytest.fixture(scope="module")
def clf(dev):
    from finetune_fair_diffusion_amd.classifier import MobileNetV3Large
    return MobileNetV3Large(R.clf_sd(0), dev)


def run_mb(clf, cs, dev):
    """One inverted-residual block through ``block_forward`` / ``block_backward``: tensors under image_refs' names and the branches of its records."""
    B, H, Ho = cs.B, cs.H, cs.Ho
    y, h2, w2, c = clf.block_forward(cs.i, _cl16(cs.x, dev), B, H, H, True)
    assert (h2, w2) == (Ho, Ho)
    out = dict(out=y, z_dw=c["z_dw"])
    branch = {"z_dw": R.branches(_nchw(c["z_dw"], B, Ho, Ho).double(), cs.wb.act)}
    if cs.wb.expand is not None:
        out["z_exp"] = c["z_exp"]
        branch["z_exp"] = R.branches(_nchw(c["z_exp"], B, H, H).double(), cs.wb.act)
    if cs.wb.se is not None:
        out.update(z1=c["z1"], z2=c["z2"], se_s=c["se_s"])
        branch.update(z1=R.branches(c["z1"].double().cpu(), "relu"), z2=R.branches(c["z2"].double().cpu(), "hardsigmoid"))
    dx = clf.block_backward(cs.i, c, _cl16(cs.g, dev, cs.gs), B)
    out["dx"] = dx.float() / cs.gs
    return _host(out), branch


@pytest.fixture(scope="module")
def prod(ops, clf, dev):
    """Product runs shared between the gates and the mutation test: arm -> (tensors, branches)."""
    cache = {}

    def get(arm):
        if arm not in cache:
            cs = R.case(arm)
            cache[arm] = {"mb": lambda: run_mb(clf, cs, dev), "sh": lambda: run_sh(cs, dev), "clf": lambda: run_clf(clf, cs, dev),
                          "sfp": lambda: run_sf_piece(_sfnet(dev), cs, dev), "sf": lambda: run_sf(_sfnet(dev), cs, dev), "va": lambda: run_va(cs, dev),
                          "vr": lambda: run_vr(cs, dev), "vu": lambda: run_vu(ops, cs, dev), "vae": lambda: run_vae(cs, dev), "vht": lambda: run_vht(cs, dev), "vit": lambda: run_vit(cs, dev)[:2]}[cs.kind]()
        return cache[arm]
    return get


@pytest.mark.parametrize("arm", tuple(R.MB_ARMS))
def test_mobilenet_block(prod, arm):
    cs = R.case(arm)
    if arm == "B3":
        assert (cs.wb.k, cs.wb.stride, cs.H % 2, cs.Ho) == (5, 2, 1, 4), "k = 5, stride 2 on an odd map: the (H + 1) // 2 edge of the depthwise data gradient"
    gate(arm, *prod(arm), net="MobileNetV3")


def run_sh(cs, dev):
    from finetune_fair_diffusion_amd.classifier import MobileNetV3Large
    net = MobileNetV3Large(cs.sd, dev, R.HEAD_CLASSES)
    assert net.ncls_pad == 16 and net.num_classes == 13
    B = cs.B
    x0, H, W, c0 = net.stem_forward(cs.chips.half().to(dev), True)
    dchips = net.stem_backward(c0, _cl16(cs.g0, dev, cs.gs), B, cs.gs)
    logits, c = net.head_forward(_cl16(cs.x, dev), B, cs.H, cs.H, True)
    assert logits.shape == (B, 16) and not bool(logits[:, 13:].any()), "the pad columns carry zero weights and biases"
    dxl = net.head_backward(c, cs.gl.float().to(dev), cs.gs)
    out = dict(z0=c0["z0"], x0=x0, dchips=dchips, zl=c["zl"], zf=c["zf"], logits=logits[:, :13], dxl=dxl.float() / cs.gs)
    branch = dict(z0=R.branches(_nchw(c0["z0"], B, H, W).double(), "hardswish"), zl=R.branches(_nchw(c["zl"], B, cs.H, cs.H).double(), "hardswish"),
                  zf=R.branches(c["zf"].double().cpu(), "hardswish"))
    return _host(out), branch


def test_mobilenet_stem_and_padded_head(prod):
    gate("SH", *prod("SH"), net="MobileNetV3")


def run_clf(clf, cs, dev):
    B = cs.B
    logits = clf.forward(cs.chips.half().to(dev), record=True)
    c = clf._ctx
    recs = list(c["blocks"])            # backward pops them
    out = {"logits": logits, "z.z0": recs[0]["z0"], "z.zl": c["zl"], "z.zf": c["zf"]}
    S2 = cs.S // 2
    branch = dict(z0=R.branches(_nchw(recs[0]["z0"], B, S2, S2).double(), "hardswish"), zl=None, zf=R.branches(c["zf"].double().cpu(), "hardswish"))
    for wb, cb in zip(cs.blocks, recs[1:]):
        pre = f"b{wb.i}."
        for k, hw in (("z_exp", cb["H"]), ("z_dw", cb["Ho"])):
            if k in cb:
                out["z." + pre + k] = cb[k]
                branch[pre + k] = R.branches(_nchw(cb[k], B, hw, hw).double(), wb.act)
        if wb.se is not None:
            out["z." + pre + "z1"], out["z." + pre + "z2"] = cb["z1"], cb["z2"]
            branch[pre + "z1"], branch[pre + "z2"] = R.branches(cb["z1"].double().cpu(), "relu"), R.branches(cb["z2"].double().cpu(), "hardsigmoid")
    Hl = recs[-1]["Ho"]
    branch["zl"] = R.branches(_nchw(c["zl"], B, Hl, Hl).double(), "hardswish")
    trace = []
    out["dchips"] = clf.backward(cs.g.float().to(dev), cs.gs, trace=trace)
    assert len(trace) == len(cs.blocks)
    for j, t in enumerate(trace):       # last block first
        out[f"trace{len(trace) - 1 - j}"] = t.float() / cs.gs
    return _host(out), branch


def test_whole_classifier_with_every_trace_entry(prod):
    """64x64 chips, B = 3, dL/dlogits on two logits: logits, dchips, the gradient at every block's input (``trace``) and every recorded pre-activation."""
    got, branch = prod("CLF")
    assert set(branch) == set(R.case("CLF").kinds)
    gate("CLF", got, branch, net="MobileNetV3")


# ============================================================================= SFNet-20
_SF = {}


def _sfnet(dev):
    if "net" not in _SF:
        from finetune_fair_diffusion_amd.sfnet import SFNet20
        _SF["net"] = SFNet20(R.sf_sd(0), dev, in_size=48)
    return _SF["net"]


def _scaled(fn, g16, gs):
    """step.py's ``_scaled_backward``: the gradient enters multiplied by the power-of-two scale with gscale = 1, the result is un-scaled after."""
    return fn(g16).float() * (1.0 / gs)


def run_sf_piece(net, cs, dev):
    N, H, Ho = cs.N, cs.H, cs.Ho
    g16 = _cl16(cs.g, dev, cs.gs)
    if cs.piece == "stem":
        y, h2, w2 = net.stem_forward(cs.x.half().to(dev))
        assert (h2, w2) == (Ho, Ho)
        out = dict(y=y, dx=_scaled(lambda g: net.stem_backward(("stem", y, H, H), g, N, 1.0), g16, cs.gs))
    elif cs.piece == "down":
        down = net.stages[cs.layer - 1][0]
        y, h2, w2 = net.down_forward(down, _cl16(cs.x, dev), N, H, H)
        assert (h2, w2) == (Ho, Ho)
        out = dict(y=y, dx=_scaled(lambda g: net.down_backward(("down", down, y, H, H), g, N), g16, cs.gs))
    else:
        c1, c2 = net.stages[cs.layer - 1][1][0]
        h, y = net.block_forward(c1, c2, _cl16(cs.x, dev), N, H, H)
        out = dict(h=h, y=y, dx=_scaled(lambda g: net.block_backward(("block", c1, c2, h, y, H, H), g, N), g16, cs.gs))
    branch = {k: R.branches(_nchw(out[k], N, Ho, Ho).double(), "relu") for k in cs.kinds}        # post-ReLU records: y > 0 is the mask
    return _host(out), branch


@pytest.mark.parametrize("arm", tuple(R.SF_PIECES))
def test_sfnet_piece(prod, arm):
    cs = R.case(arm)
    if arm == "S_down7":
        assert (cs.H, cs.Ho) == (7, 4), "an odd map: the (Hin + 1) // 2 of the stride-2 data gradient"
    gate(arm, *prod(arm), net="SFNet-20")


def run_sf(net, cs, dev):
    from finetune_fair_diffusion_amd.sfnet import face_features, face_features_backward
    N = cs.N
    f, ctxs = face_features(net, cs.chips.half().to(dev), record=True)
    out, branch = {"f": f}, {}
    for v, c in zip(("v1", "v2"), ctxs):
        layer, j = 0, 0
        for rec in c["ops"]:
            if rec[0] in ("stem", "down"):
                layer, j = layer + 1, 0
                y = rec[1] if rec[0] == "stem" else rec[2]
                recs = {f"{v}.l{layer}.down": y}
            else:
                j += 1
                recs = {f"{v}.l{layer}.b{j}.h": rec[3], f"{v}.l{layer}.b{j}.y": rec[4]}
            hw = cs.S >> layer
            for name, t in recs.items():
                out["z." + name] = t
                branch[name] = R.branches(_nchw(t, N, hw, hw).double(), "relu")
    out["dchips"] = face_features_backward(net, ctxs, (cs.g * cs.gs).float().to(dev), 1.0) * (1.0 / cs.gs)
    return _host(out), branch


def test_whole_sfnet_both_views(prod):
    """``face_features`` / ``face_features_backward`` at in_size 48 (maps 24, 12, 6, 3), N = 2: the summed features and dchips with the mirrored view's share."""
    got, branch = prod("SF")
    assert set(branch) == set(R.case("SF").kinds)
    gate("SF", got, branch, net="SFNet-20")


# ============================================================================= VAE decoder
def run_va(cs, dev):
    from finetune_fair_diffusion_amd.vae import VAEAttention
    att = VAEAttention(cs.sd, cs.prefix, dev, cs.C, R.VAE_GROUPS)
    ctx = []
    y = att.forward(_cl16(cs.x, dev), cs.B, cs.H, cs.W, ctx)
    c = ctx[0]
    dx = att.backward(_cl16(cs.g, dev, cs.gs), cs.B, cs.H, cs.W, c)
    return _host(dict(out=y, q=c["q"], k=c["k"], v=c["v"], P=c["P"], dx=dx.float() / cs.gs)), {}


@pytest.mark.parametrize("arm", ("VA64", "VA40"))
def test_vae_attention(prod, arm):
    """C = 128, 32 groups, single head.  VA40: a 5x8 map, 40 tokens -- no multiple of the GEMM tiles, of 16 or of 64 (the batched GEMM takes K = T in multiples
    of 8 only, so 6x6 = 36 tokens is not a shape the library accepts)."""
    cs = R.case(arm)
    assert (cs.H * cs.W) % 8 == 0 and (arm != "VA40" or (cs.H * cs.W) % 16 != 0)
    gate(arm, *prod(arm), net="VAE decoder")


def run_vr(cs, dev):
    from finetune_fair_diffusion_amd.layers import ResnetBlock
    blk = ResnetBlock(cs.sd, cs.prefix, dev, R.VAE_GROUPS, 1e-6, has_temb=False)
    assert (blk.shortcut is not None) == (cs.cin != cs.cout)
    ctx = []
    y = blk.forward(_cl16(cs.x, dev), None, cs.B, cs.H, cs.H, None, ctx)
    dx, _ = blk.backward(_cl16(cs.g, dev, cs.gs), cs.B, cs.H, cs.H, ctx[0])
    return _host(dict(out=y, dx=dx.float() / cs.gs)), {}


@pytest.mark.parametrize("arm", ("VR_same", "VR_short"))
def test_vae_resnet_without_time_embedding(prod, arm):
    gate(arm, *prod(arm), net="VAE decoder")


def run_vu(ops, cs, dev):
    from finetune_fair_diffusion_amd.layers import Conv3x3
    conv = Conv3x3(cs.sd, cs.prefix + "conv", dev)
    y, h2, w2 = ops.conv_up2(_cl16(cs.x, dev), conv, cs.B, cs.H, cs.H)
    assert (h2, w2) == (2 * cs.H, 2 * cs.H)
    dx = ops.conv_up2_bwd(_cl16(cs.g, dev, cs.gs), conv, cs.B, cs.H, cs.H)
    return _host(dict(out=y, dx=dx.float() / cs.gs)), {}


def test_vae_conv_up2_on_an_odd_map(prod):
    gate("VU", *prod("VU"), net="VAE decoder")


def run_vht(cs, dev):
    from finetune_fair_diffusion_amd.vae import AutoencoderKL
    vae = AutoencoderKL(cs.cfg, cs.sd, dev)
    B, H = cs.B, cs.H
    if cs.piece == "head":
        x = _cl16(cs.x, dev)
        img, st, y = vae.head_forward(x, B, H, H)
        pre = _nchw(y, B, H, H).double()
        dx = vae.head_backward(dict(x_out=x, st_out=st, pre=y, B=B, H=H, W=H), (cs.g * cs.gs).float().to(dev), 1.0)
        out = _host(dict(img=img, dx=dx.float() / cs.gs))
        out["z.clamp"] = pre
        return out, {"clamp": R.clamp_branches(pre)}
    x = vae.tail_forward(cs.x.float().to(dev))
    dz = vae.tail_backward(_cl16(cs.g, dev, cs.gs), B, H, H, 1.0) * (1.0 / cs.gs)
    return _host(dict(out=x, dz=dz)), {}


def test_vae_head_with_the_clamp_forced(prod):
    """conv_norm_out, SiLU, conv_out, clamp, NHWC to NCHW and their backward (``clamp_bwd``, the data gradient of conv_out as a small-Cin convolution)."""
    got, branch = prod("VH")
    assert 0.01 < float((branch["clamp"] != 1).double().mean()) < 0.9
    gate("VH", got, branch, net="VAE decoder")


def test_vae_tail_post_quant_and_conv_in(prod):
    """post_quant_conv + conv_in and their backward through ``conv_small_cin_bwd`` with k = 1."""
    gate("VT", *prod("VT"), net="VAE decoder")


def run_vae(cs, dev):
    from finetune_fair_diffusion_amd.vae import AutoencoderKL
    vae = AutoencoderKL(cs.cfg, cs.sd, dev)
    B, S = cs.B, 8 * cs.H
    img = vae.decode_images(cs.z.float().to(dev), record=True)
    pre = _nchw(vae._ctx["pre"], B, S, S).double()
    dz = vae.backward_images((cs.g * cs.gs).float().to(dev), 1.0) * (1.0 / cs.gs)      # step.py's _scaled_backward
    out = _host(dict(img=img, dz=dz))
    out["z.clamp"] = pre
    return out, {"clamp": R.clamp_branches(pre)}


def test_whole_vae_decoder_with_the_clamp_forced(prod):
    """util_models' tiny decoder on 8x8 latents, B = 2: the clamped image and dz, each on its own band, the clamp's branch read from the recorded ``pre``."""
    got, branch = prod("VAE")
    assert 0.01 < float((branch["clamp"] != 1).double().mean()) < 0.5, "some pixels saturate, most do not"
    gate("VAE", got, branch, net="VAE decoder")


# ============================================================================= the two ViTs
def run_vit(cs, dev, poison=False):
    from finetune_fair_diffusion_amd.vit import VisionTransformer
    pm = VisionTransformer(cs.cfg, cs.sd, dev, cs.mean, cs.std)
    assert (pm.T, pm.Tp) == (cs.T, cs.Tp)
    N, T, Tp, D = cs.N, cs.T, cs.Tp, cs.cfg.hidden_size
    e = pm.forward(cs.chips.half().to(dev), record=True)
    c = pm._ctx
    rows = lambda t: t.view(N, Tp, D)[:, :T].reshape(-1, D).clone()  # noqa: E731
    out = dict(emb=e, cls=c["cls"].clone())
    for i, L in enumerate(c["layers"]):
        out[f"h1.{i}"] = rows(L["h1"])
        if i:
            out[f"h2.{i - 1}"] = rows(L["x"])
    if poison:          # the padded token rows T..Tp of every recorded activation: the backward must not read them
        for t in [L[k] for L in c["layers"] for k in ("x", "h1")] + ([c["x0"]] if "x0" in c else []):
            t.view(N, Tp, D)[:, T:] = 1000.0
    out["dchips"] = pm.backward((cs.g * cs.gs).float().to(dev), 1.0) * (1.0 / cs.gs)
    torch.cuda.synchronize()
    return _host(out), {}, out["dchips"]


@pytest.mark.parametrize("arm", ("CLIP", "DINO"))
def test_whole_vit_tower(prod, arm):
    """The tiny towers of tests/test_engine_gpu.py (17 tokens padded to 24), N = 3: the embedding, dchips, each layer's h1 / h2 from the records.  Smooth
    networks: nothing is forced.  DINO keeps the interpolated position table (6x6 -> 4x4) and LayerScale."""
    import test_engine_gpu as TE
    assert TE.VIT_TINY == R.VIT_TINY
    gate(arm, *prod(arm), net="ViT")


@pytest.mark.parametrize("arm", ("CLIP", "DINO"))
def test_vit_backward_does_not_read_the_pad_rows(dev, arm):
    cs = R.case(arm)
    clean = run_vit(cs, dev)[2]
    poisoned = run_vit(cs, dev, poison=True)[2]
    assert bool(torch.isfinite(poisoned).all())
    assert torch.equal(clean, poisoned), f"{arm}: dchips moves when rows T..Tp of the recorded x / h1 are overwritten"


# ============================================================================= the gate rejects the mutated references
@pytest.mark.parametrize("arm", R.MUTATION_ARMS)
def test_gate_rejects_mutated_references(prod, arm):
    got, branch = prod(arm)
    bands = R.bands(arm)
    for mut, (arms, _, _) in R.MUTATIONS.items():
        if arm not in arms:
            continue
        bad = R.reference(arm, branch, mut)
        keys = R.moved_keys(arm, mut, bad)
        assert keys
        for k in keys:
            e2, _ = R.metric(got[k], bad[k])
            print(f"[{mut} {arm}] {k:12s} product against the mutated reference: e2 {e2:.3e} = {e2 / bands[k][0]:.1f} x band")
            assert e2 > bands[k][0], f"{mut} on {arm}: the gate accepts the mutated reference for {k}"


def test_zz_summary_per_network():
    """Last in the file: the figures of DESIGN.md's table, per network, from the gates that ran."""
    for net, (r2, rm, flipped, total) in SUMMARY.items():
        print(f"[summary] {net}: largest product / emulation e2 {r2:.2f} emax {rm:.2f}; forced branches {flipped} of {total} = {100.0 * flipped / max(total, 1):.4f} % (cap 1 % per mask)")
    assert SUMMARY
