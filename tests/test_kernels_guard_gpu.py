"""Memory guards for the hot-path kernels (GPU): attention, the fused cross-attention block, GroupNorm / LayerNorm, the element-wise family, the text
encoder's attention, the LoRA weight gradients and the scheduler / optimizer kernels, each run twice on the same values --

  baseline   tight, fresh allocations through the ``ops`` wrapper: the path the fp64 tests of the other test_kernels*_gpu.py files hold to their bands;
  guarded    views of a ``guard_cases.Arena`` through ``ops._call``: every operand at exactly the alignment include/fairdiff_hip.h states for it and no
             more, with the row strides the ABI admits, NaN in every byte around the inputs (guards of a full 64-row tile, gap columns, the pad rows
             Tk..Tkr of K / V), NaN inside the outputs and the sentinel 12345 around them, workspaces of exactly the documented size

-- and then, in this order: guards bit-intact, outputs fully written and finite, outputs EQUAL BITS to the baseline.  No tolerance of its own: the one
non-deterministic form (dK / dV added with fp32 atomics by the kv_div samples that share a K / V item) is compared under the band of its direct test,
``test_kernels_gpu.ATTN_BWD_TOL``.  Shapes are the smallest that hold each edge; the dispatch thresholds they are chosen against are restated from the sources in
tests/guard_cases.py (tests/test_guard_cases_cpu.py pins those restatements to the source text) and asserted here per case."""
import ctypes
import math

import pytest
import torch

import guard_cases as GC
from guard_cases import Arena, check_case
from test_kernels_gpu import ATTN_BWD_TOL, relerr

pytestmark = pytest.mark.gpu
F32, I32 = torch.float32, torch.int32


@pytest.fixture(scope="module")
def ops():
    from finetune_fair_diffusion_amd import ops
    return ops


def rnd(*shape, dev, seed, scale=1.0, dtype=None):
    from finetune_fair_diffusion_amd import ops
    g = torch.Generator(device="cpu")
    g.manual_seed(seed)
    return (torch.randn(*shape, generator=g) * scale).to(dev).to(dtype or ops.F16)


def _run(ops, name, *args):
    ops._call(name, *args, ops._stream())
    try:
        torch.cuda.synchronize()
    except RuntimeError as e:           # a device error: nothing more is started on that device by this session
        pytest.exit(f"{name}: {e}", returncode=3)


def _atomics_band(name, got, want):
    e = relerr(got, want)
    assert math.isfinite(e) and e <= ATTN_BWD_TOL, f"{name}: {e} > {ATTN_BWD_TOL}"
    return f"rel max err {e:.2e} <= {ATTN_BWD_TOL:.0e} (atomics: the band of test_attention_fwd_bwd)"


# ============================================================================= fd_attn_fwd / fd_attn_bwd_dq / fd_attn_bwd_dkdv
# geometry (csrc/attn.hip): 64-key tiles, 128-row query blocks, 128-key blocks of 4 x 32 in the dK/dV kernel.  Tq = 130 = one block + 2 rows.
ATTN_B, ATTN_H, ATTN_TQ = 2, 2, 130
ATTN_HEADS = [(40, False), (40, True), (64, False), (80, False), (160, False)]       # (head dim, pre-scaled q)
ATTN_KEYS = [(77, 80), (65, 72), (13, 13)]                                          # (Tk, Tkr): a partial second tile inside padded rows; one key past a tile; one partial tile


@pytest.mark.parametrize("kv_div", [1, 2])
@pytest.mark.parametrize("Tk,Tkr", ATTN_KEYS)
@pytest.mark.parametrize("d,prescaled", ATTN_HEADS)
def test_attention(ops, dev, d, prescaled, Tk, Tkr, kv_div):
    B, H, Tq, H16 = ATTN_B, ATTN_H, ATTN_TQ, ops.F16
    C, Bk, LD = H * d, B // kv_div, 3 * H * d + 8          # q, k, v and dq, dk, dv as column slices of [M, 3C + 8] buffers
    assert LD % 8 == 0 and Tq % 128 == 2 and not GC.fwd_two_blocks(d, Tq, Tk, B * H)
    sc = d ** -0.5
    cs = -sc if prescaled else sc
    q, k, v, do = rnd(B * Tq, C, dev=dev, seed=1), rnd(Bk * Tk, C, dev=dev, seed=2), rnd(Bk * Tk, C, dev=dev, seed=3), rnd(B * Tq, C, dev=dev, seed=4)
    if prescaled:
        q = (q.float() * ops.q_prescale(d)).to(H16)
    pad = dict(ld=LD, period=(Tk, Tkr))
    tag = f"B{B} H{H} Tq{Tq} Tk{Tk}/{Tkr} d{d}{' pre-scaled' if prescaled else ''} kv_div{kv_div} ld{LD}"

    # ---- baselines
    o_b, lse_b = ops.attn_fwd(q, k, v, B, H, Tq, Tk, d, kv_div, need_lse=True, prescaled=prescaled)
    D_b, dq_t = torch.empty((B, H, Tq), dtype=F32, device=dev), torch.empty_like(q)
    _run(ops, "fd_attn_bwd_dq", ops._p(q), ops._p(k), ops._p(v), ops._p(do), ops._p(lse_b), ops._p(D_b), ops._p(o_b), ops._p(dq_t), B, H, Tq, Tk, Tk, d, kv_div, cs, C, C, C)
    ik, iv = rnd(Bk * Tk, C, dev=dev, seed=5, dtype=F32), rnd(Bk * Tk, C, dev=dev, seed=6, dtype=F32)       # what the atomics form adds into
    ak, av = ik.clone(), iv.clone()
    dq_b, _, _ = ops.attn_bwd(q, k, v, o_b, do, lse_b, B, H, Tq, Tk, d, kv_div, dk_acc=ak, dv_acc=av, prescaled=prescaled)
    sk, sv = torch.empty((Bk * Tk, C), dtype=F32, device=dev), torch.empty((Bk * Tk, C), dtype=F32, device=dev)
    ops.attn_bwd(q, k, v, o_b, do, lse_b, B, H, Tq, Tk, d, kv_div, dk_out=sk, dv_out=sv, prescaled=prescaled)
    assert torch.equal(dq_t, dq_b)

    def arena(*extra_inputs):
        a = Arena(dev).inp("q", q, ld=LD).inp("k", k, **pad).inp("v", v, **pad)
        for name, t in extra_inputs:
            a.inp(name, t, ld=C) if t.dtype == H16 else a.inp(name, t, align=4)
        return a

    # ---- forward
    a = arena().out("o", (B * Tq, C), H16, ld=C, align=8).out("lse", (B, H, Tq), F32, align=4).build()
    _run(ops, "fd_attn_fwd", a.p("q"), a.p("k"), a.p("v"), a.p("o"), a.p("lse"), B, H, Tq, Tk, Tkr, d, kv_div, cs, LD, LD)
    check_case(f"fd_attn_fwd {tag}", a, {"o": o_b, "lse": lse_b})

    # ---- dq: with o (writes D) and without (reads D)
    a = arena(("do", do), ("lse", lse_b), ("o", o_b)).out("D", (B, H, Tq), F32, align=4).out("dq", (B * Tq, C), H16, ld=LD, align=8).build()
    _run(ops, "fd_attn_bwd_dq", a.p("q"), a.p("k"), a.p("v"), a.p("do"), a.p("lse"), a.p("D"), a.p("o"), a.p("dq"), B, H, Tq, Tk, Tkr, d, kv_div, cs, LD, LD, LD)
    check_case(f"fd_attn_bwd_dq (writes D) {tag}", a, {"dq": dq_b, "D": D_b})
    a = arena(("do", do), ("lse", lse_b), ("D", D_b)).out("dq", (B * Tq, C), H16, ld=LD, align=8).build()
    _run(ops, "fd_attn_bwd_dq", a.p("q"), a.p("k"), a.p("v"), a.p("do"), a.p("lse"), a.p("D"), None, a.p("dq"), B, H, Tq, Tk, Tkr, d, kv_div, cs, LD, LD, LD)
    check_case(f"fd_attn_bwd_dq (reads D) {tag}", a, {"dq": dq_b})

    def dkdv(a, accumulate):
        _run(ops, "fd_attn_bwd_dkdv", a.p("q"), a.p("k"), a.p("v"), a.p("do"), a.p("lse"), a.p("D"), a.p("dk"), a.p("dv"), B, H, Tq, Tk, Tkr, d, kv_div, cs, LD, LD, LD,
             accumulate)

    # ---- dK / dV, fp16 overwrite (one sample per K / V item only).  Rows Tk..Tkr of every item are not the kernel's: they keep the sentinel.
    if kv_div == 1:
        _, dk16, dv16 = ops.attn_bwd(q, k, v, o_b, do, lse_b, B, H, Tq, Tk, d, 1, prescaled=prescaled)
        a = arena(("do", do), ("lse", lse_b), ("D", D_b))
        a.out("dk", (Bk * Tkr, C), H16, align=8, **pad).out("dv", (Bk * Tkr, C), H16, align=8, **pad).build()
        dkdv(a, 0)
        check_case(f"fd_attn_bwd_dkdv fp16 {tag}", a, {"dk": dk16, "dv": dv16})
    # ---- fp32 atomics.  One sample per item: every element receives exactly one atomicAdd, initial + value is one fp32 addition whatever the order of the
    # workgroups, so bits are the gate; kv_div samples per item add in arrival order: the band.  Both start from the same finite contents.
    for accumulate in ((1,) if kv_div == 1 else (0, 1)):
        a = arena(("do", do), ("lse", lse_b), ("D", D_b))
        a.out("dk", (Bk * Tkr, C), F32, align=4, init=ik, **pad).out("dv", (Bk * Tkr, C), F32, align=4, init=iv, **pad).build()
        dkdv(a, accumulate)
        check_case(f"fd_attn_bwd_dkdv atomics accumulate={accumulate} {tag}", a, {"dk": ak, "dv": av}, band=None if kv_div == 1 else _atomics_band)
    # ---- fp32 slabs [kv_div][Bk * Tkr][lddkv]: sample j of an item WRITES the Tk key rows of slab j, columns 0 .. H*d (include/fairdiff_hip.h); the pad rows and
    # the columns behind H*d keep the sentinel.  The slabs added in ascending order are fd_sum_slabs' result, bit for bit.
    a = arena(("do", do), ("lse", lse_b), ("D", D_b))
    a.out("dk", (kv_div * Bk * Tkr, C), F32, align=16, **pad).out("dv", (kv_div * Bk * Tkr, C), F32, align=16, **pad).build()
    dkdv(a, 2)
    check_case(f"fd_attn_bwd_dkdv slabs {tag}", a, {})
    for name, want in (("dk", sk), ("dv", sv)):
        slabs = a.tight(name).view(kv_div, Bk * Tk, C)
        total = slabs[0].clone()
        for j in range(1, kv_div):
            total += slabs[j]
        assert torch.equal(total, want), f"{tag}: {name} slabs summed in ascending order differ from the tight-layout fd_sum_slabs result"


def test_attention_forward_two_query_blocks_per_wave(ops, dev):
    """the 256-row workgroups of the long self-attention forward (attn_fwd_kernel<D, 2>): one query row and two keys past whole blocks / tiles"""
    B, H, d, Tq, Tk, Tkr = 2, 8, 40, 2049, 2050, 2056
    assert GC.fwd_two_blocks(d, Tq, Tk, B * H) and not GC.fwd_two_blocks(d, Tq, Tk, B * H // 2) and Tq % 256 == 1 and Tk % 64 == 2
    C, LD = H * d, 3 * H * d + 8
    q = (rnd(B * Tq, C, dev=dev, seed=1).float() * ops.q_prescale(d)).to(ops.F16)
    k, v = rnd(B * Tk, C, dev=dev, seed=2), rnd(B * Tk, C, dev=dev, seed=3)
    o_b, lse_b = ops.attn_fwd(q, k, v, B, H, Tq, Tk, d, 1, need_lse=True, prescaled=True)
    a = Arena(dev).inp("q", q, ld=LD).inp("k", k, ld=LD, period=(Tk, Tkr)).inp("v", v, ld=LD, period=(Tk, Tkr))
    a.out("o", (B * Tq, C), ops.F16, ld=C, align=8).out("lse", (B, H, Tq), F32, align=4).build()
    _run(ops, "fd_attn_fwd", a.p("q"), a.p("k"), a.p("v"), a.p("o"), a.p("lse"), B, H, Tq, Tk, Tkr, d, 1, -(d ** -0.5), LD, LD)
    check_case(f"fd_attn_fwd two blocks per wave B{B} H{H} Tq{Tq} Tk{Tk}/{Tkr} d{d} pre-scaled ld{LD}", a, {"o": o_b, "lse": lse_b})


@pytest.mark.parametrize("B,H,T,d", [(1, 3, 7, 40), (1, 1, 1, 8)])
def test_attn_bwd_prep_and_sum_slabs(ops, dev, B, H, T, d):
    """fd_attn_bwd_prep: one thread per (b, t, h), n = B T H = 21 (n % 4 = 1) and 1.  fd_sum_slabs refuses n % 4 != 0 (16-byte vectors only), so its sizes
    are 4 (8k + 4) with a second slab and one single vector."""
    o, do = rnd(B * T, H * d, dev=dev, seed=1), rnd(B * T, H * d, dev=dev, seed=2)
    D_b = torch.empty((B, H, T), dtype=F32, device=dev)
    _run(ops, "fd_attn_bwd_prep", ops._p(o), ops._p(do), ops._p(D_b), B, H, T, d)
    a = Arena(dev).inp("o", o, ld=H * d).inp("do", do, ld=H * d).out("D", (B, H, T), F32, align=4).build()
    _run(ops, "fd_attn_bwd_prep", a.p("o"), a.p("do"), a.p("D"), B, H, T, d)
    check_case(f"fd_attn_bwd_prep B{B} H{H} T{T} d{d} (n = {B * H * T})", a, {"D": D_b})
    for nslab, n in ((3, 8 * T * H * d + 4), (1, 4)):
        x = rnd(nslab, n, dev=dev, seed=3, dtype=F32)
        s_b = torch.empty(n, dtype=F32, device=dev)
        _run(ops, "fd_sum_slabs", ops._p(x), ops._p(s_b), nslab, n)
        a = Arena(dev).inp("in", x, align=16).out("out", (n,), F32, align=16).build()
        _run(ops, "fd_sum_slabs", a.p("in"), a.p("out"), nslab, n)
        check_case(f"fd_sum_slabs nslab{nslab} n{n}", a, {"out": s_b})


# ============================================================================= fd_cross_attn_block
class _Pair:
    def __init__(self, down16, up16, rp):
        self.down16, self.up16, self.rp = down16, up16, rp


@pytest.mark.parametrize("mode", ["plain", "plain, yn == NULL", "LoRA + recording"])
@pytest.mark.parametrize("L", [77, 13])
@pytest.mark.parametrize("M,kv_div", [(64, 1), (128, 2)])
@pytest.mark.parametrize("C", [320, 640])
def test_cross_attn_block(ops, dev, C, M, kv_div, L, mode):
    from finetune_fair_diffusion_amd import lib
    H16, heads, rps, Lp = ops.F16, 8, 64, ops.CROSS_LP
    Bk, lora, rp = M // rps // kv_div, mode.startswith("LoRA"), 8 if C == 320 else 16
    assert ops.cross_block_ok(M, C, heads, L, rps, rp if lora else 0) and Lp == 80 and L <= Lp
    x = rnd(M, C, dev=dev, seed=1)
    fp = {n: rnd(C, dev=dev, dtype=F32, seed=s) * 0.2 + o for n, s, o in (("g2", 2, 1), ("b2", 3, 0), ("g3", 4, 1), ("b3", 5, 0))}
    fp["bo"] = rnd(C, dev=dev, dtype=F32, seed=8) * 0.1
    wq, wo = rnd(C, C, dev=dev, scale=C ** -0.5, seed=6), rnd(C, C, dev=dev, scale=C ** -0.5, seed=7)
    k, v = rnd(Bk * L, C, dev=dev, seed=9), rnd(Bk * L, C, dev=dev, seed=10)
    vt = ops.transpose_btc(v, Bk, L, C, Lp)                        # columns L..Lp are zero: the contract
    assert bool((vt[:, :, L:] == 0).all())
    pairs = {}
    if lora:
        r = rp - 3
        for n, s in (("q", 20), ("o", 22)):
            down, up = torch.zeros(rp, C, dtype=H16, device=dev), torch.zeros(C, rp, dtype=H16, device=dev)
            down[:r], up[:, :r] = rnd(r, C, dev=dev, scale=C ** -0.5, seed=s), rnd(C, r, dev=dev, scale=0.3, seed=s + 1)
            pairs[n] = _Pair(down, up, rp)
    pre = C == 320
    y_b, yn_b, st_b, rec = ops.cross_attn_block(x, (fp["g2"], fp["b2"], 1e-5), wq, k, vt, L, wo, fp["bo"], (fp["g3"], fp["b3"], 1e-5), heads, rps, kv_div, need_stats=True,
                                                lora_q=pairs.get("q"), lora_o=pairs.get("o"), record=lora, q_prescaled=pre)
    a = Arena(dev).inp("x", x, ld=C).inp("wq", wq, ld=C).inp("wo", wo, ld=C).inp("k", k, ld=C).inp("vt", vt.reshape(Bk * C, Lp), ld=Lp, align=8)
    for n, t in fp.items():
        a.inp(n, t, align=16 if n == "bo" else 4)
    a.out("y", (M, C), H16, ld=C)
    want = {"y": y_b}
    if mode != "plain, yn == NULL":
        a.out("yn", (M, C), H16, ld=C).out("yn_stats", (M, 2), F32, align=4)
        want.update(yn=yn_b, yn_stats=st_b)
    if lora:
        for n, p in pairs.items():
            a.inp(f"{n}_down", p.down16, ld=C + 8).inp(f"{n}_up", p.up16, ld=rp + 8)
        for n in ("n2_out", "q_out", "o_out"):
            a.out(n, (M, C), H16, ld=C)
        a.out("tq_out", (M, rp), H16, ld=rp, align=8).out("to_out", (M, rp), H16, ld=rp, align=8)
        a.out("ln2_stats", (M, 2), F32, align=4).out("lse_out", (M // rps, heads, rps), F32, align=4)
        want.update(n2_out=rec["n2"], ln2_stats=rec["ln2"], q_out=rec["q2"], tq_out=rec["tq2"], o_out=rec["o2"], lse_out=rec["lse2"], to_out=rec["to2"])
    a.build()
    D = lib.CrossBlockDesc()
    D.x, D.ln2_gamma, D.ln2_beta, D.ln2_eps, D.wq, D.k, D.vt, D.L, D.Lp = a.address("x"), a.address("g2"), a.address("b2"), 1e-5, a.address("wq"), a.address("k"), a.address("vt"), L, Lp
    D.wo, D.bo, D.ln3_gamma, D.ln3_beta, D.ln3_eps, D.y = a.address("wo"), a.address("bo"), a.address("g3"), a.address("b3"), 1e-5, a.address("y")
    if "yn" in a.specs:
        D.yn, D.yn_stats = a.address("yn"), a.address("yn_stats")
    D.M, D.C, D.heads, D.rows_per_sample, D.kv_div, D.scale = M, C, heads, rps, kv_div, (C // heads) ** -0.5
    if lora:
        D.lora_q_down, D.ld_q_down, D.lora_q_up, D.ld_q_up = a.address("q_down"), C + 8, a.address("q_up"), rp + 8
        D.lora_o_down, D.ld_o_down, D.lora_o_up, D.ld_o_up, D.lora_rp = a.address("o_down"), C + 8, a.address("o_up"), rp + 8, rp
        D.n2_out, D.ln2_stats, D.q_out, D.tq_out = a.address("n2_out"), a.address("ln2_stats"), a.address("q_out"), a.address("tq_out")
        D.o_out, D.lse_out, D.to_out, D.q_prescaled = a.address("o_out"), a.address("lse_out"), a.address("to_out"), int(pre)
    _run(ops, "fd_cross_attn_block", ctypes.byref(D))
    check_case(f"fd_cross_attn_block C{C} M{M} rows_per_sample{rps} kv_div{kv_div} L{L}/{Lp} {mode}", a, want)


# ============================================================================= fd_small_attn_fwd / fd_small_attn_bwd
@pytest.mark.parametrize("masked", [False, True])
@pytest.mark.parametrize("T", [77, 65])            # 65: one key in the second pass of the 64 lanes
def test_small_attn(ops, dev, T, masked):
    B, H, d = 2, 2, 64
    C, sc = H * d, d ** -0.5
    q, k, v, do = (rnd(B * T, C, dev=dev, seed=s) for s in (1, 2, 3, 4))
    kv = None
    if masked:
        kv = (torch.rand(B, T, generator=torch.Generator().manual_seed(T)) < 0.6).to(I32)
        kv[:, 0] = 1
        kv = kv.to(dev)
    o_b, P_b = ops.small_attn_fwd(q, k, v, kv, B, H, T, d, sc, causal=True, save_p=True)
    dq_b, dk_b, dv_b = ops.small_attn_bwd(q, k, v, P_b, do, B, H, T, d, sc)
    tag = f"B{B} H{H} T{T} d{d} causal key_valid={int(masked)}"
    a = Arena(dev).inp("q", q, ld=C, align=2).inp("k", k, ld=C, align=2).inp("v", v, ld=C, align=2)
    if masked:
        a.inp("kv", kv, align=4)
    a.out("o", (B * T, C), ops.F16, ld=C, align=2).out("P", (B, H, T, T), F32, align=4).build()
    _run(ops, "fd_small_attn_fwd", a.p("q"), a.p("k"), a.p("v"), a.p("o"), a.p("P"), a.p("kv" if masked else None), B, H, T, d, sc, 1)
    check_case(f"fd_small_attn_fwd {tag}", a, {"o": o_b, "P": P_b})
    a = Arena(dev).inp("q", q, ld=C, align=2).inp("k", k, ld=C, align=2).inp("v", v, ld=C, align=2).inp("P", P_b, align=4).inp("do", do, ld=C, align=2)
    for n in ("dq", "dk", "dv"):
        a.out(n, (B * T, C), ops.F16, ld=C, align=2)
    a.build()
    _run(ops, "fd_small_attn_bwd", a.p("q"), a.p("k"), a.p("v"), a.p("P"), a.p("do"), a.p("dq"), a.p("dk"), a.p("dv"), B, H, T, d, sc)
    check_case(f"fd_small_attn_bwd {tag}", a, {"dq": dq_b, "dk": dk_b, "dv": dv_b})


# ============================================================================= GroupNorm
GN_C, GN_G, GN_B = 320, 32, 2
# HW -> (forward branch, backward branch) of csrc/norm.hip for C = 320, 32 groups: 51 rows per pass of the single-launch form, 8 / 24 / 12 passes at most
GN_SHAPES = {100: ("fused<8>", "fused"), 700: ("fused<24>", "two-launch"), 1300: ("two-launch", "two-launch")}


@pytest.mark.parametrize("C1,C2", [(320, 0), (160, 160)])
@pytest.mark.parametrize("HW", sorted(GN_SHAPES))
def test_groupnorm(ops, dev, HW, C1, C2):
    B, G, C, H16, eps = GN_B, GN_G, GN_C, ops.F16, 1e-5
    assert (GC.gn_fwd_branch(C, HW, G), GC.gn_bwd_branch(C, HW, G)) == GN_SHAPES[HW]
    assert HW % 51 != 0 and HW % GC.gn_chunk_rows(C, HW)[0] != 0            # the last pass / chunk of an image is partial, and the next image starts right behind it
    x1 = (rnd(B * HW, C1, dev=dev, seed=1).float() * 2 + 0.5).to(H16)
    x2 = (rnd(B * HW, C2, dev=dev, seed=2).float() - 0.3).to(H16) if C2 else None
    gamma, beta = rnd(C, dev=dev, dtype=F32, seed=3) * 0.2 + 1, rnd(C, dev=dev, dtype=F32, seed=4) * 0.2
    dy, add1 = rnd(B * HW, C, dev=dev, seed=5), rnd(B * HW, C1, dev=dev, seed=6)
    add2 = rnd(B * HW, C2, dev=dev, seed=7) if C2 else None
    tag = f"B{B} HW{HW} C{C1}+{C2} G{G} silu"

    def inputs(a):
        a.inp("x1", x1, ld=C1).inp("gamma", gamma, align=4).inp("beta", beta, align=4)
        return a.inp("x2", x2, ld=C2) if C2 else a

    y_b, st_b = ops.groupnorm(x1, x2, B, HW, G, eps, gamma, beta, True)
    a = inputs(Arena(dev)).out("y", (B * HW, C), H16, ld=C).out("mean_rstd", (B, G, 2), F32, align=4).ws("scratch", B * 64 * G * 2, align=4).build()
    _run(ops, "fd_groupnorm_fwd", a.p("x1"), C1, a.p("x2" if C2 else None), C2, B, HW, G, eps, a.p("gamma"), a.p("beta"), 1, a.p("y"), a.p("mean_rstd"), a.p("scratch"))
    check_case(f"fd_groupnorm_fwd [{GN_SHAPES[HW][0]}] {tag}, scratch {B * 64 * G * 2} floats", a, {"y": y_b, "mean_rstd": st_b})

    for adds, need_dx2 in ((True, True), (False, False)) if C2 else ((True, True), (False, True)):
        dx1_b, dx2_b = ops.groupnorm_bwd(x1, x2, dy, B, HW, G, st_b, gamma, beta, True, add1=add1 if adds else None, add2=add2 if adds else None, need_dx2=need_dx2)
        a = inputs(Arena(dev)).inp("dy", dy, ld=C).inp("mean_rstd", st_b, align=4)
        if adds:
            a.inp("add1", add1, ld=C1)
            a.inp("add2", add2, ld=C2) if C2 else None
        a.out("dx1", (B * HW, C1), H16, ld=C1).ws("scratch", B * 65 * G * 2, align=4)
        want = {"dx1": dx1_b}
        if C2 and need_dx2:
            a.out("dx2", (B * HW, C2), H16, ld=C2)
            want["dx2"] = dx2_b
        a.build()
        _run(ops, "fd_groupnorm_bwd", a.p("x1"), C1, a.p("x2" if C2 else None), C2, a.p("dy"), B, HW, G, a.p("mean_rstd"), a.p("gamma"), a.p("beta"), 1, a.p("scratch"),
             a.p("add1" if adds else None), a.p("add2" if adds and C2 else None), a.p("dx1"), a.p("dx2" if "dx2" in want else None))
        check_case(f"fd_groupnorm_bwd [{GN_SHAPES[HW][1]}] {tag}{' + add1/add2' if adds else ''}{'' if need_dx2 or not C2 else ', dx2 == NULL'}, scratch {B * 65 * G * 2} floats", a, want)


@pytest.mark.parametrize("C1,C2", [(320, 0), (160, 160)])
def test_groupnorm_from_statistics(ops, dev, C1, C2):
    """fd_groupnorm_fwd_stats_p / fd_groupnorm_fwd_stats: the apply pass alone, from per-chunk (sum, sum of squares) of 32 rows x 10 channels as the GEMM epilogues
    leave them (fd_gemm_desc.gn_stats) -- here formed in torch: both runs read the same numbers, image-major and phase-major."""
    B, HW, G, C, rows, H16, eps = GN_B, 256, GN_G, GN_C, 32, ops.F16, 1e-5
    assert HW % rows == 0 and HW % GC.gn_chunk_rows(C, HW)[0] != 0 and (HW // rows) % 4 == 0
    xs = [(rnd(B * HW, c, dev=dev, seed=1 + i).float() * 2 + 0.5).to(H16) for i, c in enumerate((C1, C2)) if c]
    gamma, beta = rnd(C, dev=dev, dtype=F32, seed=3) * 0.2 + 1, rnd(C, dev=dev, dtype=F32, seed=4) * 0.2
    sts = []
    for x in xs:
        u = x.float().view(B * HW // rows, rows, x.shape[1] // 10, 10)
        sts.append(torch.stack([u.sum((1, 3)), (u * u).sum((1, 3))], -1).contiguous())
    x2, st2 = (xs[1], sts[1]) if C2 else (None, None)
    for per, entry in ((0, "fd_groupnorm_fwd_stats_p"), (HW // rows // 4, "fd_groupnorm_fwd_stats_p"), (0, "fd_groupnorm_fwd_stats")):
        xs[0].gn_stats = (sts[0], rows, per)
        if C2:
            xs[1].gn_stats = (sts[1], rows, per)
        y_b, st_b = ops.groupnorm(xs[0], x2, B, HW, G, eps, gamma, beta, True)
        a = Arena(dev).inp("x1", xs[0], ld=C1).inp("gamma", gamma, align=4).inp("beta", beta, align=4).inp("st1", sts[0], align=8)
        if C2:
            a.inp("x2", x2, ld=C2).inp("st2", st2, align=8)
        a.out("y", (B * HW, C), H16, ld=C).out("mean_rstd", (B, G, 2), F32, align=4).build()
        head = (a.p("x1"), C1, a.p("x2" if C2 else None), C2, B, HW, G, eps, a.p("gamma"), a.p("beta"), 1, a.p("y"), a.p("mean_rstd"))
        if entry == "fd_groupnorm_fwd_stats_p":
            _run(ops, "fd_groupnorm_fwd_stats_p", *head, a.p("st1"), rows, per, a.p("st2" if C2 else None), rows if C2 else 0, per if C2 else 0)
        else:
            _run(ops, "fd_groupnorm_fwd_stats", *head, a.p("st1"), rows, a.p("st2" if C2 else None), rows if C2 else 0)
        check_case(f"{entry} B{B} HW{HW} C{C1}+{C2} rows{rows} per{per}", a, {"y": y_b, "mean_rstd": st_b})


# ============================================================================= LayerNorm
@pytest.mark.parametrize("tail", ["one row past whole workgroups", "M = 1"])
@pytest.mark.parametrize("C", [8, 320, 768, 1280, 2048])
def test_layernorm(ops, dev, C, tail):
    H16 = ops.F16
    per_wg = GC.LN_ROWS_PER_WORKGROUP[GC.ln_maxv(C)]
    M = 2 * per_wg + 1 if tail.startswith("one") else 1
    assert {8: 1, 320: 1, 768: 2, 1280: 4, 2048: 4}[C] == GC.ln_maxv(C) and M % per_wg == 1 % per_wg
    x = (rnd(M, C, dev=dev, seed=1).float() * 3 + 1).to(H16)
    gamma, beta = rnd(C, dev=dev, dtype=F32, seed=2) * 0.2 + 1, rnd(C, dev=dev, dtype=F32, seed=3) * 0.2
    dy, add = rnd(M, C, dev=dev, seed=4), rnd(M, C, dev=dev, seed=5)
    y_b, st_b = ops.layernorm(x, gamma, beta, 1e-5, save_stats=True)
    for stats in (True, False):
        a = Arena(dev).inp("x", x, ld=C).inp("gamma", gamma, align=4).inp("beta", beta, align=4).out("y", (M, C), H16, ld=C)
        want = {"y": y_b}
        if stats:
            a.out("mean_rstd", (M, 2), F32, align=4)
            want["mean_rstd"] = st_b
        a.build()
        _run(ops, "fd_layernorm_fwd", a.p("x"), a.p("gamma"), a.p("beta"), a.p("y"), a.p("mean_rstd" if stats else None), M, C, 1e-5)
        check_case(f"fd_layernorm_fwd M{M} C{C} (MAXV {GC.ln_maxv(C)}) mean_rstd={int(stats)}", a, want)
    for with_add in (True, False):
        dx_b = ops.layernorm_bwd(x, dy, gamma, st_b, add=add if with_add else None)
        a = Arena(dev).inp("x", x, ld=C).inp("dy", dy, ld=C).inp("gamma", gamma, align=4).inp("mean_rstd", st_b, align=4)
        if with_add:
            a.inp("add", add, ld=C)
        a.out("dx", (M, C), H16, ld=C).build()
        _run(ops, "fd_layernorm_bwd", a.p("x"), a.p("dy"), a.p("gamma"), a.p("mean_rstd"), a.p("add" if with_add else None), a.p("dx"), M, C)
        check_case(f"fd_layernorm_bwd M{M} C{C} (MAXV {GC.ln_maxv(C)}) add={int(with_add)}", a, {"dx": dx_b})


# ============================================================================= element-wise
@pytest.mark.parametrize("M,F", [(37, 40), (1, 8)])
def test_geglu(ops, dev, M, F):
    H16 = ops.F16
    proj, dy = rnd(M, 2 * F, dev=dev, seed=1), rnd(M, F, dev=dev, seed=2)
    a = Arena(dev).inp("proj", proj).out("y", (M, F), H16).build()
    _run(ops, "fd_geglu_fwd", a.p("proj"), a.p("y"), M, F)
    check_case(f"fd_geglu_fwd M{M} F{F}", a, {"y": ops.geglu(proj)})
    a = Arena(dev).inp("proj", proj).inp("dy", dy).out("dproj", (M, 2 * F), H16).build()
    _run(ops, "fd_geglu_bwd", a.p("proj"), a.p("dy"), a.p("dproj"), M, F)
    check_case(f"fd_geglu_bwd M{M} F{F}", a, {"dproj": ops.geglu_bwd(proj, dy)})
    Fi = F + 4                                          # the interleaved form takes F % 4: 4 (value, gate) pairs per thread, dy in 8-byte vectors
    proj, dy = rnd(M, 2 * Fi, dev=dev, seed=3), rnd(M, Fi, dev=dev, seed=4)
    a = Arena(dev).inp("proj", proj).inp("dy", dy, align=8).out("dproj", (M, 2 * Fi), H16).build()
    _run(ops, "fd_geglu_bwd_interleaved", a.p("proj"), a.p("dy"), a.p("dproj"), M, Fi)
    check_case(f"fd_geglu_bwd_interleaved M{M} F{Fi}", a, {"dproj": ops.geglu_bwd_interleaved(proj, dy)})


N_TAIL, N_ONE = 8 * 1000 + 5, 5
N_SCALAR_2ND = 4096 * 256 + 8 * 3 + 5                 # one element per thread, 4096 workgroups at most: a second grid-stride pass, 8k + 5
N_VECTOR_2ND = 8 * (4096 * 256 + 3) + 5               # eight elements per thread: the same for the 16-byte body


@pytest.mark.parametrize("n", [N_ONE, N_TAIL, N_SCALAR_2ND, N_VECTOR_2ND])
def test_flat_elementwise(ops, dev, n):
    H16 = ops.F16
    assert n % 8 == 5
    x, dy = (rnd(n, dev=dev, seed=1).float() * 3).to(H16), rnd(n, dev=dev, seed=2)
    a = Arena(dev).inp("x", x).out("y", (n,), H16).build()
    _run(ops, "fd_act_fwd", a.p("x"), a.p("y"), n, ops.ACT["silu"])
    check_case(f"fd_act_fwd silu n{n}", a, {"y": ops.act_fwd(x, "silu")})
    a = Arena(dev).inp("z", x).inp("dy", dy).out("dx", (n,), H16).build()
    _run(ops, "fd_act_bwd", a.p("z"), a.p("dy"), a.p("dx"), n, ops.ACT["gelu"])
    check_case(f"fd_act_bwd gelu n{n}", a, {"dx": ops.act_bwd(x, dy, "gelu")})
    a = Arena(dev).inp("a", x).inp("b", dy).out("y", (n,), H16).build()
    _run(ops, "fd_add", a.p("a"), a.p("b"), a.p("y"), n, 0.5, -2.0)
    check_case(f"fd_add n{n}", a, {"y": ops.add(x, dy, 0.5, -2.0)})
    a = Arena(dev).inp("a", x).out("y", (n,), H16).build()
    _run(ops, "fd_add", a.p("a"), None, a.p("y"), n, -1.5, 3.0)
    check_case(f"fd_add b == NULL n{n}", a, {"y": ops.add(x, None, -1.5, 3.0)})
    a = Arena(dev).inp("b", dy).out("y", (n,), H16, init=x).build()
    _run(ops, "fd_add", a.p("y"), a.p("b"), a.p("y"), n, 1.0, 0.25)
    check_case(f"fd_add in place n{n}", a, {"y": ops.add(x, dy, 1.0, 0.25)})
    if n == N_VECTOR_2ND:
        return                                          # the casts are scalar kernels: N_SCALAR_2ND is their second pass
    x32 = rnd(n, dev=dev, seed=3, dtype=F32) * 3
    a = Arena(dev).inp("x", x32, align=4).out("y", (n,), H16, align=2).build()
    _run(ops, "fd_cast_f32_to_f16", a.p("x"), a.p("y"), n, 0.75)
    check_case(f"fd_cast_f32_to_f16 n{n}", a, {"y": ops.to_f16(x32, 0.75)})
    a = Arena(dev).inp("x", x, align=2).out("y", (n,), F32, align=4).build()
    _run(ops, "fd_cast_f16_to_f32", a.p("x"), a.p("y"), n, 0.75)
    check_case(f"fd_cast_f16_to_f32 n{n}", a, {"y": ops.to_f32(x, 0.75)})


def test_strided_layout_kernels(ops, dev):
    H16 = ops.F16
    # fd_copy_cols: both sides strided
    M, cols = 37, 24
    src = rnd(M, cols, dev=dev, seed=1)
    dst_b = torch.empty(M, cols, dtype=H16, device=dev)
    ops.copy_cols(src, dst_b, cols)
    a = Arena(dev).inp("src", src, ld=cols + 8).out("dst", (M, cols), H16, ld=cols + 16).build()
    _run(ops, "fd_copy_cols", a.p("src"), cols + 8, a.p("dst"), cols + 16, M, cols)
    check_case(f"fd_copy_cols M{M} cols{cols} lds{cols + 8} ldd{cols + 16}", a, {"dst": dst_b})
    # fd_transpose_btc: T = 77 keys into Tp = 80, C = 72 (a partial 64-channel tile), strided x; the padding is exactly zero
    B, T, Tp, C = 2, 77, 80, 72
    x = rnd(B * T, C, dev=dev, seed=2)
    y_b = ops.transpose_btc(x, B, T, C, Tp)
    a = Arena(dev).inp("x", x, ld=C + 8).out("y", (B * C, Tp), H16, ld=Tp).build()
    _run(ops, "fd_transpose_btc", a.p("x"), C + 8, a.p("y"), B, T, C, Tp)
    check_case(f"fd_transpose_btc B{B} T{T}/{Tp} C{C} ldx{C + 8}", a, {"y": y_b.reshape(B * C, Tp)})
    got = a.tight("y").view(B, C, Tp)
    assert bool((got[:, :, T:] == 0).all()) and torch.equal(got[:, :, :T], x.view(B, T, C).permute(0, 2, 1))
    # fd_downsum2x2
    B, H, W, C = 2, 3, 5, 24
    x = rnd(B * 2 * H * 2 * W, C, dev=dev, seed=3)
    a = Arena(dev).inp("x", x, ld=C).out("y", (B * H * W, C), H16, ld=C).build()
    _run(ops, "fd_downsum2x2", a.p("x"), a.p("y"), B, H, W, C)
    check_case(f"fd_downsum2x2 B{B} H{H} W{W} C{C}", a, {"y": ops.downsum2x2(x, B, H, W, C)})
    # fd_nhwc_to_nchw (both output types) and fd_clamp_bwd with ldx > C: scalar kernels, any stride
    B, HW, C, ldx = 2, 37, 5, 8
    x = rnd(B * HW, C, dev=dev, seed=4)
    for f32 in (True, False):
        y_b = ops.nhwc_to_nchw(x, B, HW, C, out_dtype=F32 if f32 else H16, scale=1.5, lo=-1.0, hi=1.0)
        a = Arena(dev).inp("x", x, ld=ldx, align=2).out("y", (B, C, HW), F32 if f32 else H16, align=4 if f32 else 2).build()
        _run(ops, "fd_nhwc_to_nchw", a.p("x"), ldx, a.p("y"), int(f32), B, HW, C, 1.5, -1.0, 1.0)
        check_case(f"fd_nhwc_to_nchw B{B} HW{HW} C{C} ldx{ldx} {'fp32' if f32 else '16-bit'} output", a, {"y": y_b})
    dimg = rnd(B, C, HW, dev=dev, seed=5, dtype=F32)
    a = Arena(dev).inp("pre", x, ld=ldx, align=2).inp("dimg", dimg, align=4).out("dpre", (B, C, HW), F32, align=4).build()
    _run(ops, "fd_clamp_bwd", a.p("pre"), ldx, a.p("dimg"), a.p("dpre"), B, HW, C, -1.0, 1.0)
    check_case(f"fd_clamp_bwd B{B} HW{HW} C{C} ldx{ldx}", a, {"dpre": ops.clamp_bwd(x, dimg, B, HW, C)})


@pytest.mark.parametrize("cols", [7, 255, 257])           # below a wave; one short of / one past the 256 threads' first pass
def test_softmax_rows(ops, dev, cols):
    H16, rows = ops.F16, 3
    x, dp = (rnd(rows, cols, dev=dev, seed=cols).float() * 4).to(H16), rnd(rows, cols, dev=dev, seed=cols + 2)
    mask = rnd(rows, cols, dev=dev, seed=cols + 1, dtype=F32)
    mask[1, cols // 2] = -math.inf
    for m in (None, mask):
        p_b = ops.softmax_rows(x, 0.125, m, rows if m is not None else 0, rows if m is not None else 0)
        a = Arena(dev).inp("x", x, ld=cols, align=2)
        if m is not None:
            a.inp("mask", m, ld=cols, align=4)
        a.out("y", (rows, cols), H16, ld=cols, align=2).build()
        _run(ops, "fd_softmax_rows", a.p("x"), a.p("y"), rows, cols, 0.125, a.p("mask" if m is not None else None), rows if m is not None else 0, rows if m is not None else 0)
        check_case(f"fd_softmax_rows rows{rows} cols{cols} mask={int(m is not None)}", a, {"y": p_b})
    a = Arena(dev).inp("p", p_b, ld=cols, align=2).inp("dp", dp, ld=cols, align=2).out("ds", (rows, cols), H16, ld=cols, align=2).build()
    _run(ops, "fd_softmax_rows_bwd", a.p("p"), a.p("dp"), a.p("ds"), rows, cols, 0.125)
    check_case(f"fd_softmax_rows_bwd rows{rows} cols{cols}", a, {"ds": ops.softmax_rows_bwd(p_b, dp, 0.125)})


# ============================================================================= LoRA weight gradients
WGRAD_M = 130
# the arms of fd_lora_wgrad as tests/test_kernels_sharp_gpu.py::test_lora_wgrad_every_arm reaches them (csrc/lora.hip: the vectorised kernel needs N and ldx multiples
# of 8 at padded rank 8, of 4 at 16; everything else takes lora_wgrad_partial<8 / 16 / 32 / 64>); (N, R, ldx - N, arm, bytes X must be aligned to)
WGRAD_ARMS = [(320, 4, 8, "vectorised, padded rank 8", 16), (324, 4, 8, "plain 8 (N % 8 = 4)", 2), (320, 8, 4, "plain 8 (ldx % 8 = 4)", 2), (320, 16, 8, "vectorised, padded rank 16", 8),
              (322, 12, 8, "plain 16 (N % 4 = 2)", 2), (320, 16, 2, "plain 16 (ldx % 4 = 2)", 2), (320, 24, 8, "plain 32", 2), (648, 50, 8, "plain 64", 2)]


def _g_layouts(N, R):
    """(transposed?, view shape, row stride with a gap, g_stride_n, g_stride_r)"""
    return [(False, (N, R), R + 3, R + 3, 1), (True, (R, N), N + 5, 1, N + 5)]


@pytest.mark.parametrize("N,R,extra,arm,xalign", WGRAD_ARMS)
def test_lora_wgrad(ops, dev, N, R, extra, arm, xalign):
    M, RP, ldx, H16 = WGRAD_M, GC.wgrad_rp(R), N + extra, ops.F16
    vec, need = GC.wgrad_scratch(M, N, R, ldx)
    assert vec == arm.startswith("vectorised") and need <= 1 << 22        # ops.scratch never offers fewer than 4 Mi floats: both runs take the same splits
    buf = rnd(M, ldx, dev=dev, seed=1)
    X = buf[:, :N]                                      # the baseline keeps the row stride: it selects the arm
    Tm = torch.zeros(M, RP, dtype=H16, device=dev)
    Tm[:, :R] = rnd(M, R, dev=dev, seed=2)
    for trans, shape, ldg, sn, sr in _g_layouts(N, R):
        G0 = rnd(*shape, dev=dev, seed=3, dtype=F32)
        G_b = G0.clone()
        ops.lora_wgrad(X, Tm, G_b, *((1, N) if trans else (R, 1)), R, scale=0.5)
        a = Arena(dev).inp("X", X.contiguous(), ld=ldx, align=xalign).inp("T", Tm, ld=RP).out("G", shape, F32, ld=ldg, align=4, init=G0).ws("scratch", need, align=4).build()
        _run(ops, "fd_lora_wgrad", a.p("X"), ldx, a.p("T"), RP, a.p("G"), sn, sr, M, N, R, 0.5, a.p("scratch"), need)
        check_case(f"fd_lora_wgrad [{arm}] M{M} N{N} R{R} ldx{ldx} G {'[R, N]' if trans else '[N, R]'} ld{ldg} scratch {need} floats", a, {"G": G_b})


@pytest.mark.parametrize("R", [4, 12, 24, 50])           # padded ranks 8, 16 (vectorised VALU kernels) and 32, 64 (MFMA kernels)
def test_lora_wgrad_multi(ops, dev, R):
    from finetune_fair_diffusion_amd import lib
    RP, H16 = GC.wgrad_rp(R), ops.F16
    shapes = [(WGRAD_M, 320), (77, 640), (WGRAD_M, 328)]
    need = GC.wgrad_multi_scratch(shapes, RP)
    assert RP == {4: 8, 12: 16, 24: 32, 50: 64}[R] and need <= 1 << 22
    probs, a = [], Arena(dev)
    for i, (M, N) in enumerate(shapes):
        buf = rnd(M, N + 8, dev=dev, seed=10 + i)
        Tm = torch.zeros(M, RP, dtype=H16, device=dev)
        Tm[:, :R] = rnd(M, R, dev=dev, seed=20 + i)
        trans, shape, ldg, sn, sr = _g_layouts(N, R)[i % 2]
        G0 = rnd(*shape, dev=dev, seed=30 + i, dtype=F32)
        probs.append((buf[:, :N], Tm, G0.clone(), trans, M, N, ldg, sn, sr))
        a.inp(f"X{i}", buf[:, :N].contiguous(), ld=N + 8, align=16 if RP != 16 else 8).inp(f"T{i}", Tm, ld=RP + 8).out(f"G{i}", shape, F32, ld=ldg, align=4, init=G0)
    a.ws("scratch", need, align=16 if RP >= 32 else 4).build()
    with ops.wgrad_batch():
        for X, Tm, G_b, trans, M, N, _, _, _ in probs:
            ops.lora_wgrad(X, Tm, G_b, *((1, N) if trans else (R, 1)), R, scale=0.5)
    arr = lib.WgradDesc.array(len(probs))
    for i, (d, (_, _, _, _, M, N, _, sn, sr)) in enumerate(zip(arr, probs)):
        d.X, d.ldx, d.T, d.ldt, d.G, d.g_stride_n, d.g_stride_r = a.address(f"X{i}"), N + 8, a.address(f"T{i}"), RP + 8, a.address(f"G{i}"), sn, sr
        d.M, d.N, d.R, d.scale = M, N, R, 0.5
    _run(ops, "fd_lora_wgrad_multi", ctypes.byref(arr), len(probs), a.p("scratch"), need)
    check_case(f"fd_lora_wgrad_multi padded rank {RP} (R{R}) problems {shapes} scratch {need} floats", a, {f"G{i}": p[2] for i, p in enumerate(probs)})


# ============================================================================= scheduler / optimizer: flat fp32, updated in place
@pytest.mark.parametrize("n", [N_ONE, N_TAIL, N_SCALAR_2ND])
def test_scheduler_and_optimizer(ops, dev, n):
    assert n % 8 == 5
    eps, lat, x0p = rnd(2 * n, dev=dev, seed=1, dtype=F32), rnd(n, dev=dev, seed=2, dtype=F32), rnd(n, dev=dev, seed=3, dtype=F32)
    coef = (7.5, 0.8, 0.6, 0.9, 0.3, 0.1)                   # guidance, alpha_t, sigma_t, c_x, c_d0, c_d1
    for prev in (True, False):
        lat_b, x0_b = lat.clone(), torch.empty_like(lat)
        ops.cfg_dpm_step(eps, coef[0], lat_b, x0p if prev else None, x0_b, *coef[1:])
        a = Arena(dev).inp("eps", eps, align=4).out("lat", (n,), F32, align=4, init=lat).out("x0_out", (n,), F32, align=4)
        if prev:
            a.inp("x0_prev", x0p, align=4)
        a.build()
        _run(ops, "fd_cfg_dpm_step", a.p("eps"), coef[0], a.p("lat"), a.p("x0_prev" if prev else None), a.p("x0_out"), *coef[1:], n)
        check_case(f"fd_cfg_dpm_step n{n} x0_prev={int(prev)}", a, {"lat": lat_b, "x0_out": x0_b})
    g = rnd(n, dev=dev, seed=4, dtype=F32)
    g_b, flag_b = g.clone(), torch.zeros(1, dtype=I32, device=dev)
    ops.grad_finite_scale(g_b, 1.0 / 1024, flag_b)
    a = Arena(dev).out("g", (n,), F32, align=4, init=g).out("flag", (1,), I32, align=4, init=torch.zeros(1, dtype=I32)).build()
    _run(ops, "fd_grad_finite_scale", a.p("g"), n, 1.0 / 1024, a.p("flag"))
    check_case(f"fd_grad_finite_scale n{n}", a, {"g": g_b, "flag": flag_b})
    state = dict(p=rnd(n, dev=dev, seed=5, dtype=F32), m=rnd(n, dev=dev, seed=6, dtype=F32) * 0.1, v=rnd(n, dev=dev, seed=7, dtype=F32).abs() * 0.01, ema=rnd(n, dev=dev, seed=8, dtype=F32))
    hyper = (1e-3, 0.9, 0.999, 1e-8, 0.01, 3, 0.01)         # lr, beta1, beta2, eps, weight decay, step, 1 - ema decay
    for with_ema in (True, False):
        base = {k: t.clone() for k, t in state.items()}
        ops.adamw_ema(base["p"], g, base["m"], base["v"], base["ema"] if with_ema else None, *hyper)
        a = Arena(dev).inp("g", g, align=4)
        for k, t in state.items():
            if k != "ema" or with_ema:
                a.out(k, (n,), F32, align=4, init=t)
        a.build()
        _run(ops, "fd_adamw_ema", a.p("p"), a.p("g"), a.p("m"), a.p("v"), a.p("ema" if with_ema else None), n, *hyper)
        check_case(f"fd_adamw_ema n{n} ema={int(with_ema)}", a, {k: base[k] for k in a.specs if k != "g"})
