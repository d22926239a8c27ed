"""What tests/test_image_blocks_gpu.py rests on, held without a GPU (tests/image_refs.py, tests/image_bands.py):
  the BatchNorm fold is exact and the product's own fold lands within one fp16 ulp of it;
  the restated forwards are the oracle modules' own forwards;
  the margins of image_bands.py are 1.25 x the largest ratio between emulation variants, recomputed here;
  every emulation variant leaves every mask under half the branch-flip cap, each flipped element within its tensor's band of the break point;
  no band exceeds the engine-level caps;
  every mutated reference moves each tensor it names by more than that tensor's band, measured with emulation variant a;
  every row of MBV3_SETTINGS maps to a gated arm."""
import pytest
import torch

import image_bands as IB
import image_refs as R
from finetune_fair_diffusion_amd import weights as W

BLOCK_ARMS = tuple(a for a in R.CASES if a not in R.NET_ARMS)


# ============================================================================= the fold
def _oracle_block(sd, i):
    from oracle import nn_mobilenet as OM
    k, exp, cout, se, act, s = OM.SETTINGS[i]
    cin = 16 if i == 0 else OM.SETTINGS[i - 1][2]
    m = OM.InvertedResidual(cin, k, exp, cout, se, act, s).eval()
    p = f"features.{i + 1}."
    m.load_state_dict({n[len(p):]: t for n, t in sd.items() if n.startswith(p)}, strict=True)
    return m.double()


@pytest.mark.parametrize("arm", tuple(R.MB_ARMS))
def test_folded_block_is_the_oracle_block_with_its_batchnorm(arm):
    cs = R.case(arm)
    got, _ = R.mb_block_forward(R.mb_block_weights(cs.sd, cs.i, rounded=False), cs.x, R.ImagePolicy())
    ref = _oracle_block(cs.sd, cs.i)(cs.x)
    e2, emax = R.metric(got, ref)
    print(f"[{arm}] folded restatement against the eval-mode module: e2 {e2:.2e} emax {emax:.2e}")
    assert emax < 1e-10


def test_whole_classifier_restatement_is_the_oracle_module():
    from oracle import nn_mobilenet as OM
    cs = R.case("CLF")
    m = OM.MobileNetV3Large(80).eval()
    m.load_state_dict(cs.sd, strict=True)
    ref = m.double()(cs.chips)
    pol = R.ImagePolicy()
    x, _ = R.stem_forward(R.head_weights(cs.sd, rounded=False), cs.chips, pol)
    for i in range(len(W.MBV3_SETTINGS)):
        x, _ = R.mb_block_forward(R.mb_block_weights(cs.sd, i, rounded=False), x, pol, f"b{i}.")
    got, _ = R.head_forward(R.head_weights(cs.sd, rounded=False), x, pol)
    e2, emax = R.metric(got, ref)
    print(f"[CLF] folded restatement against the eval-mode module: e2 {e2:.2e} emax {emax:.2e}")
    assert emax < 1e-10
    assert set(pol.branch) == set(cs.kinds)


def _ulp16(t):
    e = torch.floor(torch.log2(t.abs().clamp_min(2.0 ** -14)))
    return torch.exp2(e - 10)


def test_product_fold_is_within_one_fp16_ulp_of_the_fp64_fold():
    from finetune_fair_diffusion_amd import classifier as C
    sd = R.clf_sd(0)
    worst = 0.0
    prefixes = ["features.16."]
    for i in range(len(W.MBV3_SETTINGS)):
        wb = R.mb_block_weights(sd, i)
        p = f"features.{i + 1}.block."
        if wb.expand is not None:
            prefixes.append(p + "0.")
        prefixes.append(p + f"{(wb.expand is not None) + 1 + (wb.se is not None)}.")
    for p in prefixes:
        w64, b64 = R.fold64(sd, p)
        assert w64.shape[2:] == (1, 1), p
        pw = C._PW(*C._fold(sd, p, "cpu"))
        ref = R.r16(w64).flatten(1)
        ulps = ((pw.w.double() - ref).abs() / _ulp16(ref)).max()
        worst = max(worst, float(ulps))
        assert float(ulps) <= 1.0, (p, float(ulps))
        assert float((pw.bias.double() - b64).abs().max()) <= 1e-6 * float(b64.abs().max())
    for i in range(len(W.MBV3_SETTINGS)):       # depthwise weights stay fp32
        wb = R.mb_block_weights(sd, i)
        p = f"features.{i + 1}.block.{int(wb.expand is not None)}."
        w, b = C._fold(sd, p, "cpu")
        dw = C._DW(w, b, wb.k, wb.stride)
        ref = wb.dw[0].reshape(wb.exp, wb.k * wb.k).t()
        assert dw.w.dtype == torch.float32 and float((dw.w.double() - ref).abs().max()) <= 2.0 ** -22 * float(ref.abs().max())
    print(f"product fold against round16(fp64 fold): at most {worst:.2f} ulp over {len(prefixes)} pointwise convolutions")


# ============================================================================= SFNet-20: restatement, gradient scale
def test_sfnet_restatement_is_the_oracle_module():
    from oracle import nn_sfnet as OS
    cs = R.case("SF")
    m = OS.SFNet20(in_size=cs.S).eval()
    m.load_state_dict(cs.sd, strict=True)
    m.double()
    got, _ = R.run(cs)
    x = cs.chips.clone().requires_grad_(True)
    ref = m(x) + m(torch.flip(x, [3]))          # get_face_feats without its cast to fp32
    e2, emax = R.metric(got["f"], ref)
    print(f"[SF] restated face features against the module's own forward on both views: e2 {e2:.2e} emax {emax:.2e}")
    assert emax < 1e-12 and R.metric(ref, OS.get_face_feats(m, cs.chips, normalize=False))[1] < 1e-6
    (ref * cs.g).sum().backward()
    assert R.metric(got["dchips"], x.grad)[1] < 1e-12


# ============================================================================= VAE attention, the two ViTs: restatements, the LayerScale fold
@pytest.mark.parametrize("arm", ("VA64", "VA40"))
def test_vae_attention_restatement_is_the_oracle_module(arm):
    from oracle import nn_vae
    cs = R.case(arm)
    m = nn_vae.VAEAttention(cs.C, R.VAE_GROUPS)
    m.load_state_dict({n[len(cs.prefix):]: t for n, t in cs.sd.items()}, strict=True)
    m.double()
    e2, emax = R.metric(R.vae_attn_forward(m, cs.x, R.ImagePolicy()), m(cs.x))
    print(f"[{arm}] restated attention against the module's own forward: e2 {e2:.2e} emax {emax:.2e}")
    assert emax < 1e-6         # the module's softmax runs in fp32 whatever the module's dtype (upcast_softmax); the restatement keeps fp64


@pytest.mark.parametrize("arm", ("CLIP", "DINO"))
def test_vit_restatement_with_folded_layerscale_is_the_oracle_tower(arm):
    """The restated forward on the exactly folded numbers (class token + position, LayerScale inside the projections, the interpolated table) is the oracle
    tower's own forward on the raw state dict, to 1e-10 before any rounding."""
    from oracle import nn_vit as OV
    cs = R.case(arm)
    raw = (OV.CLIPVisionModelWithProjection if cs.vkind == "clip" else OV.DinoVisionTransformer)(OV.ViTConfig(**R.VIT_TINY[cs.vkind]))
    raw.load_state_dict(cs.sd, strict=True)
    raw.eval().double()
    mt, st = (torch.tensor(t, dtype=torch.float64).view(1, 3, 1, 1) for t in (cs.mean, cs.std))
    ref = raw(((cs.chips + 1) * 0.5 - mt) / st)
    ocfg, osd, _ = R.vit_product_numbers(cs.vkind, cs.sd, rounded=False)
    m = (OV.CLIPVisionModelWithProjection if cs.vkind == "clip" else OV.DinoVisionTransformer)(OV.ViTConfig(**ocfg))
    m.double().load_state_dict(osd, strict=True)
    got = R.vit_forward(m.eval(), ocfg, cs.chips, cs.mean, cs.std, R.ImagePolicy(), {})
    e2, emax = R.metric(got, ref)
    print(f"[{arm}] folded restatement against the tower's own forward: e2 {e2:.2e} emax {emax:.2e}")
    assert emax < 1e-10


def test_product_layerscale_fold_and_position_table():
    from finetune_fair_diffusion_amd import vit as V
    from oracle import nn_vit as OV
    cs = R.case("DINO")
    for i in range(cs.cfg.num_hidden_layers):
        for ls, lin in (("ls1", "attn.proj"), ("ls2", "mlp.fc2")):
            p = V._Lin(cs.sd[f"blocks.{i}.{lin}.weight"], cs.sd[f"blocks.{i}.{lin}.bias"], "cpu", scale=cs.sd[f"blocks.{i}.{ls}.gamma"])
            ref = cs.osd[f"blocks.{i}.{lin}.weight"]
            assert float(((p.w.double() - ref).abs() / _ulp16(ref)).max()) <= 1.0
    g = cs.cfg.image_size // cs.cfg.patch_size
    assert cs.cfg.pos_grid != g, "the DINOv2 arm interpolates its position table"
    assert torch.equal(V._interpolate_pos(cs.sd["pos_embed"], g), OV.interpolate_pos_encoding(cs.sd["pos_embed"].float(), g))
    assert (cs.T, cs.Tp) == (17, 24)


def test_inputs_are_fp16_and_gradient_scales_follow_step_py():
    for arm in R.CASES:
        cs = R.case(arm)
        for name in ("x", "chips", "z"):
            t = getattr(cs, name, None)
            if t is not None:
                assert torch.equal(t.half().double(), t), (arm, name)
        for name in ("g", "g0", "gl"):
            t = getattr(cs, name, None)
            if t is not None:
                assert torch.equal((t * cs.gs).half().double(), t * cs.gs) and float((t * cs.gs).abs().max()) < 6e4 / 16, (arm, name)
        if cs.kind in ("sf", "sfp", "vit"):        # _pow2_scale_dev(max|g|, 1.0) of the rounded gradient is the scale it was rounded under
            assert R.pow2_scale(float(cs.g.abs().max())) == cs.gs, arm
        elif cs.kind in ("va", "vr", "vu", "vht", "vae"):      # the VAE backward: _pow2_scale_dev(max|d_img|, 64.0)
            assert R.pow2_scale(float(cs.g.abs().max()), 64.0) == cs.gs, arm
        else:
            assert cs.gs == 1024.0          # FairnessTrainer.clf_gscale


# ============================================================================= margins, caps, flips
def _ratios(arms):
    e2, emax, rows = 1.0, 1.0, []
    for arm in arms:
        r2, rm, where = R.variant_ratios(R.emulation_stats(arm))
        rows.append(f"      {arm:9s} {r2:.3f}  {str(where[0][0]) if where[0] else '-':22s} {where[0][1] if where[0] else '-'}        {rm:.3f}  {str(where[1][0]) if where[1] else '-':22s} {where[1][1] if where[1] else '-'}")
        e2, emax = max(e2, r2), max(emax, rm)
    print("\n".join(rows))
    return e2, emax


def test_margins_are_recomputed():
    e2, emax = _ratios(BLOCK_ARMS)
    print(f"largest ratio e2 {e2:.4f} -> margin {1.25 * e2:.4f} (image_bands {IB.MARGIN_E2}); emax {emax:.4f} -> {1.25 * emax:.4f} (image_bands {IB.MARGIN_MAX})")
    assert 1.25 * e2 <= IB.MARGIN_E2 <= 1.25 * e2 * 1.06
    assert 1.25 * emax <= IB.MARGIN_MAX <= 1.25 * emax * 1.06


def test_whole_network_margins_are_recomputed():
    e2, emax = _ratios(R.NET_ARMS)
    print(f"largest ratio e2 {e2:.4f} -> margin {1.25 * e2:.4f} (image_bands {IB.MARGIN_E2_NET}); emax {emax:.4f} -> {1.25 * emax:.4f} (image_bands {IB.MARGIN_MAX_NET})")
    assert 1.25 * e2 <= IB.MARGIN_E2_NET <= 1.25 * e2 * 1.06
    assert 1.25 * emax <= IB.MARGIN_MAX_NET <= 1.25 * emax * 1.06


def test_caps_hold_and_name_the_capped_tensors():
    capped = []
    for arm in R.CASES:
        net = arm in R.NET_ARMS
        m2, mm = (IB.MARGIN_E2_NET, IB.MARGIN_MAX_NET) if net else (IB.MARGIN_E2, IB.MARGIN_MAX)
        for k, (b2, bm, e2, em) in R.bands(arm).items():
            cap = R.CAP_FWD if R.is_forward(k) else R.CAP_GRAD
            assert b2 <= cap and bm <= cap
            if m2 * e2 > cap or mm * em > cap:
                capped.append((arm, k))
                print(f"{arm} {k}: margin x emulation = e2 {m2 * e2:.2e} emax {mm * em:.2e} passes the cap {cap}: the band is the cap")
                assert 2 * e2 <= cap and 2 * em <= cap, "the emulation alone must clear the cap by a factor of two"
    assert set(capped) <= set(IB.CAPPED), (capped, IB.CAPPED)


@pytest.mark.parametrize("arm", tuple(R.CASES))
def test_emulations_flip_under_half_the_cap(arm):
    b = R.bands(arm)
    for v in R.VARIANTS:
        seed = 1 if v == "e" else 0
        tot = [0, 0]
        for name, (share, n, dist, zm) in R.emulation_flips(arm, v).items():
            key = name if name in b else "z." + name
            tot[0] += round(share * n)
            tot[1] += n
            assert share <= 0.5 * R.FLIP_CAP, f"{arm} variant {v}: {share * 100:.3f} % of mask {name} ({n} elements) left the reference's branch"
            assert dist <= b[key][1] * zm, f"{arm} variant {v} mask {name}: a flipped element's reference pre-activation is {dist:.3e} from the break, limit {b[key][1] * zm:.3e}"
        print(f"[{arm} {v}] {tot[0]} of {tot[1]} mask elements ({100.0 * tot[0] / max(tot[1], 1):.4f} %) off the unforced reference's branch (seed {seed})")


# ============================================================================= mutations, coverage of the settings table
@pytest.mark.parametrize("mut", tuple(R.MUTATIONS))
def test_mutation_moves_what_it_names(mut):
    for arm in R.MUTATIONS[mut][0]:
        got, branch, _ = R.emulation(arm, "a")
        bad, bands = R.reference(arm, branch, mut), R.bands(arm)
        keys = R.moved_keys(arm, mut, bad)
        assert keys, (arm, mut)
        for k in keys:
            e2, _ = R.metric(got[k], bad[k])
            print(f"[{mut} {arm}] {k}: variant a against the mutated reference e2 {e2:.3e} = {e2 / bands[k][0]:.1f} x band ({bands[k][0]:.2e})")
            assert e2 > bands[k][0], f"{mut} on {arm}: {k} moves by {e2:.3e}, inside its band {bands[k][0]:.2e}"


def test_every_mbv3_setting_maps_to_an_arm():
    for i in range(len(W.MBV3_SETTINGS)):
        arm = R.MB_CONFIG_ARM[R.mb_config(i)]
        assert arm in R.MB_ARMS and R.mb_config(R.MB_ARMS[arm]["i"]) == R.mb_config(i), i
    odd_s2_k5 = [a for a, kw in R.MB_ARMS.items() if kw["H"] % 2 == 1 and R.mb_config(kw["i"])[:2] == (5, 2)]
    assert odd_s2_k5, "a stride-2 k = 5 block on an odd map: the (H + 1) // 2 edge"
    assert any(kw["H"] == 10 for kw in R.MB_ARMS.values())
    assert R.HEAD_CLASSES % 8 != 0
