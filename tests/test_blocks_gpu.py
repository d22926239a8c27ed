"""``TransformerBlock`` (unet.py) and ``ResnetBlock`` (layers.py) -- forward, recorded activations, input gradients and every LoRA gradient, tensor by tensor
-- against the fp64 oracle modules, arm by arm (tests/block_refs.py: references, emulations, mutations; tests/block_bands.py: margins).

Every tensor is held to  e2 <= MARGIN_E2 x (largest e2 of the fp16-rounding emulations)  and the same for emax; the bands are 6e-4 .. 5e-3, against the 2e-2 /
5e-2 of the whole-network tests.  Shapes: 8 heads, B = 4 samples on Bk = 2 prompt groups (kv_div = 2), L = 13 tokens of 768, 8x8 latents unless the arm says
otherwise.  References are computed once per arm on the host and shared (functools caches of block_refs)."""
import contextlib
import types

import pytest
import torch

import block_bands as BB
import block_refs as R

pytestmark = pytest.mark.gpu
H16, F32 = torch.float16, torch.float32


@pytest.fixture(scope="module")
def ops():
    from finetune_fair_diffusion_amd import ops
    assert ops.F16 == H16
    return ops


@contextlib.contextmanager
def patched(obj, name, value):
    old = getattr(obj, name)
    setattr(obj, name, value)
    try:
        yield
    finally:
        setattr(obj, name, old)


def _cl16(t, dev, scale=1.0):
    return R._cl(t * scale).half().contiguous().to(dev)


def _lora_name(cs, key):
    a, p, w = key.split(".")
    return f"{cs.prefix}transformer_blocks.0.{a}.processor.{p}_lora.{w}.weight"


def make_tblock(cs, dev):
    from finetune_fair_diffusion_amd.layers import ParamBank
    from finetune_fair_diffusion_amd.unet import AttnLoRA, TransformerBlock
    blk = TransformerBlock(cs.sd, cs.prefix, dev, cs.C, R.HEADS, R.GROUPS, R.XDIM)
    bank = None
    if cs.lora:
        bank = ParamBank(cs.lora_shapes, dev)
        bank.load_state_dict(cs.lora_sd)
        blk.lora1, blk.lora2 = AttnLoRA(bank, blk.name1), AttnLoRA(bank, blk.name2)
        blk.lora1.refresh()
        blk.lora2.refresh()
    return blk, bank


def run_tblock(ops, cs, dev, *, fused=None, lean=False, slots=False, need_dx=True):
    """The product's tensors of a case under block_refs' names (gradients divided by gscale).  ``fused``: None = as the block decides; False = cross_block_ok
    answers no; the number of ``cross_attn_block`` launches is returned under '_fused'."""
    from finetune_fair_diffusion_amd import unet as U
    blk, bank = make_tblock(cs, dev)
    blk.lean = lean
    calls = [0]
    real = ops.cross_attn_block

    def spy(*a, **k):
        calls[0] += 1
        return real(*a, **k)
    N = cs.B // 2 if cs.pair else cs.B
    out = {}
    with patched(ops, "cross_attn_block", spy), patched(ops, "cross_block_ok", ops.cross_block_ok if fused is None else (lambda *a, **k: False)):
        blk.prepare_cross(cs.steps[0].enc.reshape(-1, R.XDIM).half().to(dev), cs.Bk, cs.L, record=True)
        if slots:       # what UNet2DConditionModel.prepare_backward_slots does for every transformer
            blk.cross["slots"] = torch.zeros((len(cs.steps), 2) + tuple(blk.cross["dK"].shape), dtype=F32, device=dev)
        try:
            for s, st in enumerate(cs.steps):
                tag = f"@{s}" if len(cs.steps) > 1 else ""
                ctx = []
                y = blk.forward(_cl16(st.x, dev), N, cs.H, cs.W, ctx, pair=cs.pair)
                c = ctx[0]
                out.update({"out" + tag: y, "h0" + tag: c["h0"], "h1" + tag: c["h1"], "h2" + tag: c["h2"]})
                U.BWD_SLOT[0] = s if slots else None
                dx = blk.backward(_cl16(st.g, dev, R.GSCALE), cs.B, cs.H, cs.W, c, R.GSCALE, need_dx=need_dx)
                out["dx" + tag] = dx.float() / R.GSCALE if dx is not None else None
        finally:
            U.BWD_SLOT[0] = None
        out["denc"] = blk.finish_cross_backward(R.GSCALE, need_denc=True).float() / R.GSCALE
    for k in R.LORA_KEYS:
        out[k] = bank.grad_view(_lora_name(cs, k)).clone()
    torch.cuda.synchronize()
    for k, t in out.items():
        assert t is None or bool(torch.isfinite(t).all()), f"{k}: not finite at gscale {R.GSCALE}"
    out["_fused"] = calls[0]
    return out


def gate(arm, got, ref=None, skip=(), emax=True):
    """Every reference tensor of ``arm`` under its band; prints each figure, then asserts.  Returns the arm's largest ratios to the emulation.
    ``emax=False``: the e2 band alone."""
    ref = R.reference(arm) if ref is None else ref
    bands = R.bands(R.ALIASES.get(arm.split("/")[0], arm.split("/")[0]))
    bad, worst = [], [(0.0, None), (0.0, None)]
    for k in ref:
        if k in skip:
            continue
        e2, em = R.metric(got[k], ref[k])
        b2, bm, u2, um = bands[k]
        print(f"[{arm}] {k[-58:]:20s} e2 {e2:.3e} = {e2 / u2:.2f} x emulation (band {b2:.2e})   emax {em:.3e} = {em / um:.2f} x emulation (band {bm:.2e})")
        worst = [max(worst[0], (e2 / u2, k)), max(worst[1], (em / um, k))]
        if not (e2 <= b2 and (em <= bm or not emax)):
            bad.append(f"{k}: e2 {e2:.3e} (band {b2:.2e}), emax {em:.3e} (band {bm:.2e})")
    print(f"[{arm}] largest e2 / emulation {worst[0][0]:.2f} on {worst[0][1]} (margin {BB.MARGIN_E2_NET if arm == 'U' else BB.MARGIN_E2}); emax {worst[1][0]:.2f} on {worst[1][1]} (margin {BB.MARGIN_MAX})")
    assert not bad, f"{arm}: " + "; ".join(bad)
    return worst


def differences(name, a, b, keys):
    for k in keys:
        if a[k] is not None:
            e2, em = R.metric(a[k], b[k])
            print(f"[{name}] {k:20s} e2 {e2:.3e} emax {em:.3e}{'  (bit-identical)' if torch.equal(a[k], b[k]) else ''}")


@pytest.fixture(scope="module")
def prod(ops, dev):
    """Product runs shared between tests, made on first use: name -> tensors."""
    cache = {}

    def get(name, arm, **kw):
        if name not in cache:
            cache[name] = run_tblock(ops, R.case(arm), dev, **kw)
        return cache[name]
    return get


# ============================================================================= TransformerBlock
def _fused_expected(ops, cs):
    return ops.cross_block_ok(cs.B * cs.H * cs.W, cs.C, R.HEADS, cs.L, cs.H * cs.W, 8 if cs.rank <= 8 else 64)


def test_T1_fused_cross_block_d40(ops, prod):
    cs = R.case("T1")
    assert ops.q_prescale(cs.C // R.HEADS) is not None and _fused_expected(ops, cs)
    got = prod("T1", "T1")
    assert got["_fused"] == 1
    gate("T1", got)


def test_T2_unfused_arm_same_inputs(ops, prod):
    got = prod("T2", "T1", fused=False)
    assert got["_fused"] == 0
    gate("T2", got)
    differences("T1 vs T2", prod("T1", "T1"), got, R.reference("T1"))


def test_T3_rows_per_sample_not_multiple_of_64(ops, prod):
    cs = R.case("T3")
    assert (cs.H * cs.W) % 64 != 0 and not _fused_expected(ops, cs)
    got = prod("T3", "T3")
    assert got["_fused"] == 0
    gate("T3", got)


def test_T4_fused_d80(ops, prod):
    cs = R.case("T4")
    assert ops.q_prescale(80) is None and _fused_expected(ops, cs)
    got = prod("T4", "T4")
    assert got["_fused"] == 1
    gate("T4", got)


def test_T5_d160_never_fused(ops, prod):
    assert ops.q_prescale(160) is None and not ops.cross_shape_ok(1280, R.HEADS, 13)
    got = prod("T5", "T5")
    assert got["_fused"] == 0
    gate("T5", got)


def test_T6_rank_50(ops, prod):
    cs = R.case("T6")
    assert ops.cross_shape_ok(cs.C, R.HEADS, cs.L) and not _fused_expected(ops, cs), "rank 50 pads to 64: the fused kernel takes 0, 8, 16"
    got = prod("T6", "T6")
    assert got["_fused"] == 0
    gate("T6", got)


@pytest.mark.parametrize("need_dx", (False, True))
def test_T7_cfg_pair(ops, prod, need_dx):
    got = prod(f"T7/{need_dx}", "T7", need_dx=need_dx)
    assert got["_fused"] == 0
    if not need_dx:
        assert got["dx"] is None
    gate(f"T7/dx={need_dx}", got, R.reference("T7"), skip=() if need_dx else ("dx",))


@pytest.mark.parametrize("arm,full", (("T8a", "T1"), ("T8b", "T5")))
def test_T8_lean_recording(ops, prod, arm, full):
    got = prod(arm, arm, lean=True)
    gate(arm, got)
    keys = list(R.reference(arm))
    base = prod(full, full)
    if got["_fused"]:        # the fused kernel's LayerNorm is not the stand-alone one the lean backward recomputes with: reported, not asserted
        differences(f"{arm} lean vs full, fused arm", got, base, keys)
        got, base = prod(arm + "/unfused", arm, lean=True, fused=False), prod("T2", "T1", fused=False)
    for k in keys:
        assert torch.equal(got[k], base[k]), f"{arm}: lean recording on the unfused arm is not bit-identical to the full one in {k}"


def test_T9_two_timesteps_atomics(ops, prod):
    gate("T9", prod("T9", "T9"))


def test_T9_two_timesteps_slots(ops, dev, prod):
    got = prod("T9/slots", "T9", slots=True)
    gate("T9/slots", got, R.reference("T9"))
    again = run_tblock(ops, R.case("T9"), dev, slots=True)
    for k in R.reference("T9"):
        assert torch.equal(got[k], again[k]), f"slots form: {k} differs run to run"


def test_T10_static_kv_no_lora(ops, dev):
    cs = R.case("T10")
    blk, _ = make_tblock(cs, dev)
    ref, got, ptrs = R.reference("T10"), {}, []
    for s, st in enumerate(cs.steps):
        blk.prepare_cross(st.enc.reshape(-1, R.XDIM).half().to(dev), cs.Bk, cs.L, record=False, static=True)
        assert blk.cross["static"]
        ptrs.append(tuple(blk.cross[k].data_ptr() for k in ("K", "V", "Vt80")))
        got[f"out@{s}"] = blk.forward(_cl16(st.x, dev), cs.B, cs.H, cs.W)
    assert ptrs[0] == ptrs[1] and blk.static_generation == 1, "the second prepare_cross must rewrite K, V and the transposed V in place"
    torch.cuda.synchronize()
    gate("T10", got, {k: ref[k] for k in got})


# ============================================================================= ResnetBlock
def run_resnet(ops, cs, dev, names=None):
    from finetune_fair_diffusion_amd.layers import ResnetBlock
    blk = ResnetBlock(cs.sd, cs.prefix, dev, R.GROUPS, 1e-5)
    ctx = []
    skip = _cl16(cs.skip, dev) if cs.skip is not None else None
    timer = types.SimpleNamespace(records=[], shapes=[])
    with patched(ops, "TIMER", timer if names is not None else None):
        y = blk.forward(_cl16(cs.x, dev), skip, cs.B, cs.H, cs.W, cs.trow.half().to(dev), ctx)
        dx, dskip = blk.backward(_cl16(cs.g, dev, R.GSCALE), cs.B, cs.H, cs.W, ctx[0])
    torch.cuda.synchronize()
    if names is not None:
        names += [(r[0], s[:5]) for r, s in zip(timer.records, timer.shapes)]
    out = dict(out=y, dx=dx.float() / R.GSCALE)
    if skip is not None:
        out["dskip"] = dskip.float() / R.GSCALE
    for k, t in out.items():
        assert bool(torch.isfinite(t).all()), k
    return out


@pytest.fixture(scope="module")
def prod_r(ops, dev):
    cache = {}

    def get(arm):
        if arm not in cache:
            cache[arm] = run_resnet(ops, R.case(arm), dev)
        return cache[arm]
    return get


@pytest.mark.parametrize("arm", ("R1", "R2", "R3", "R4"))
def test_resnet(prod_r, arm):
    cs = R.case(arm)
    if arm == "R3":
        assert (cs.C1 + cs.C2) // R.GROUPS == 30 and cs.C1 % 30 != 0, "a GroupNorm group straddles the concat boundary"
    gate(arm, prod_r(arm))


def test_R5_resnet_16x16(ops, dev):
    names = []
    got = run_resnet(ops, R.case("R5"), dev, names)
    for n, shape in names:
        print(f"[R5] fd_gemm_kernel_name {n}  (M, N, K, K2, conv mode) = {shape}")
    gate("R5", got)


# ============================================================================= the gate rejects the mutated references
@pytest.mark.parametrize("arm", R.MUTATION_ARMS)
def test_gate_rejects_mutated_references(prod, prod_r, arm):
    got = prod_r(arm) if arm.startswith("R") else prod("T7/True", "T7", need_dx=True) if arm == "T7" else prod(arm, arm)
    bands = R.bands(arm)
    for mut, (arms, _) in R.MUTATIONS.items():
        if arm not in arms:
            continue
        bad = R.reference(arm, mut)
        for k in R.moved_keys(arm, mut, bad):
            e2, _ = R.metric(got[k], bad[k])
            print(f"[{mut} {arm}] {k:20s} product against the mutated reference: e2 {e2:.3e} = {e2 / bands[k][0]:.1f} x band")
            assert e2 > bands[k][0], f"{mut} on {arm}: the gate accepts the mutated reference for {k}"


# ============================================================================= the whole U-Net at the production arms
def test_whole_unet_d40_every_lora_tensor(ops, dev):
    """util_models size "d40" at 16x16 latents (256 and 64 rows per sample: both levels take the fused cross-attention kernel, d = 40 is pre-scaled), a CFG
    pair of one latent: eps and each of the 96 LoRA gradient tensors on its own, in e2 against the fp64 oracle, under the band of the whole net's emulations."""
    from finetune_fair_diffusion_amd import weights as W
    from finetune_fair_diffusion_amd.unet import UNet2DConditionModel
    cs, ref = R.case("U"), R.reference("U")
    gated, skipped = R.unet_gated(ref)
    print(f"[U] {len(gated)} LoRA gradient tensors gated, {len(skipped)} under 1e-3 of the largest norm: {skipped}")
    assert len(gated) + len(skipped) == 96 and len(skipped) <= 0.05 * 96
    net = UNet2DConditionModel(W.UNetConfig(**cs.cfg), cs.sd, dev)
    bank = net.add_lora(cs.rank, cs.lora_sd)
    calls, real = [0], ops.cross_attn_block

    def spy(*a, **k):
        calls[0] += 1
        return real(*a, **k)
    with patched(ops, "cross_attn_block", spy):
        net.prepare_timesteps([cs.t])
        net.prepare_prompt(cs.enc.half().to(dev), record=True)
        eps = net.forward_step(cs.x.float().to(dev), 0, record=True, pair=True)
    assert calls[0] == 5, "six transformer blocks: the first takes the pair form, the other five the fused kernel"
    bank.grad.zero_()
    net.backward_step((cs.g * R.GSCALE).float().to(dev), R.GSCALE)
    net.finish_prompt_backward(R.GSCALE, need_denc=False)
    torch.cuda.synchronize()
    got = {"eps": eps.reshape(ref["eps"].shape)}
    got.update({n: bank.grad_view(n) for n in gated})
    assert all(bool(torch.isfinite(t).all()) for t in got.values())
    gate("U", got, {k: ref[k] for k in got}, emax=False)
