"""The sharp gates of tests/kernel_bands.py on the fp16 product library (GPU, in process).

The other test_kernels_*_gpu.py files hold every fp16 kernel to ONE statistic, max|got - ref| / max|ref| <= 2e-3 .. 5e-3 against fp32 torch; a GEMM that
drops one k-term of one row at K = 4104, or scales one column by 1 + 2^-10, stays inside it (tests/test_fp16_bands_cpu.py shows that without a GPU).  Here:
  gate B  every case of tests/gemm_cases.py -- one per kernel instantiation the product dispatcher can reach -- against an fp64 statement, with the dispatch
          asserted first, with and without the residual, under the one- or two-rounding band the epilogue path calls for, bare and with an activation
          (silu, gelu, quick_gelu) and as the fused GEGLU; the A operand of the dense cases and the input map of every convolution sit inside larger buffers
          filled with 6e4 (B, the second slab and the residual are tight allocations), and outputs are NaN-prefilled with sentinel rows behind them;
          the fp32-output accumulators (fd_lora_wgrad at all six arms, fd_lora_wgrad_multi, fd_attn_bwd_prep) under B1;
  gate C  the single-rounding ops and attention against a torch emulation of their stated arithmetic;
  and the small dispatcher arms no other test launches (fd_conv_small_cin's generic kernel, fd_conv_small_cin_bwd at k = 1 / scale != 1, fd_avgpool_hw_bwd + add).
References are fp64 torch statements evaluated on the GPU; inputs are fp16-representable values used on both sides.  Every test prints its figures."""

import math

import pytest
import torch
import torch.nn.functional as F

import gemm_cases as GC
import kernel_bands as KB

pytestmark = pytest.mark.gpu
H16 = torch.float16


@pytest.fixture(scope="module")
def ops():
    from finetune_fair_diffusion_amd import ops
    assert ops.F16 == H16, "this file checks the fp16 library (tests/run_bf16_kernel_checks.py is its bf16 counterpart)"
    return ops


def rnd(*shape, dev, seed, scale=1.0, dtype=H16):
    g = torch.Generator(device="cpu")
    g.manual_seed(seed)
    return (torch.randn(*shape, generator=g) * scale).to(dev).to(dtype)


def B(name, got, ref, S, T, roundings=1, residual=None):
    """Gate B: prints the figures, then asserts B1 and B2.  fp32 outputs take the fp32 half-ulp and have no B2."""
    rounded = got.dtype == H16
    r = KB.gate_b(got, ref, S, T, H16, rounded=rounded, roundings=roundings if rounded else 1, residual=residual if (rounded and roundings == 2) else None)
    b2 = f"B2 row {r['b2_row']:.3f} col {r['b2_col']:.3f} (margin {KB.B2_MARGINS[H16][roundings]})" if rounded else "B2 n/a (fp32 output)"
    print(f"[B {name}] {roundings if rounded else 0} rounding(s): B1 max ratio {r['b1_ratio']:.{3 if rounded else 5}f}, {r['b1_bad']} elements over; {b2}")
    assert r["ok_b1"], f"{name}: gate B1, {r['b1_bad']} elements over the band (max ratio {r['b1_ratio']:.3f})"
    assert r["ok_b2"], f"{name}: gate B2 row {r['b2_row']:.3f} col {r['b2_col']:.3f} over the margin"
    return r


def C(name, got, ref, emu, cols=None):
    """Gate C: the statistics of the kernel over those of the emulation.  ``cols``: lay flat tensors out in rows of that many elements."""
    if cols:
        n = got.numel() // cols * cols
        got, ref, emu = (t.reshape(-1)[:n].reshape(-1, cols) for t in (got, ref, emu))
    r = KB.gate_c(got, ref, emu, H16)
    print(f"[C {name}] max {r['max']:.3f} ulp (emulation {r['max_emu']:.3f}, ratio {r['max_ratio']:.3f} <= {KB.C_MARGIN_MAX}); RMS {r['rms']:.3f}, "
          f"over the emulation's: row {r['rms_row']:.3f} <= {KB.C_MARGIN_ROW}, col {r['rms_col']:.3f} <= {KB.C_MARGIN_COL}")
    assert r["ok"], f"{name}: gate C {r}"
    return r


# ============================================================================= fd_gemm: every case of the table under gate B
# epilogue activations: (fp64 / fp32 statement, Lipschitz bound).  |silu'| <= 1.0998 (quick_gelu is silu of 1.702 x over 1.702: the same bound), |gelu'| <= 1.1290.
# The accumulation term of B1 passes through the activation scaled by that bound; the activation's own fp32 operations (exp, add, divide, multiply, each a few
# 2^-24 of a value no larger than S) count as four more terms.
ACT_FN = {"silu": (F.silu, 1.1), "quick_gelu": (lambda t: t * torch.sigmoid(1.702 * t), 1.1), "gelu": (F.gelu, 1.13)}
POISON = 6e4


def _poisoned_rows(x):
    """A contiguous copy of the rows of ``x`` inside a larger allocation whose other rows are huge: a gather that leaves the operand at either end would show."""
    pad = 64
    big = torch.full((x.shape[0] + 2 * pad, x.shape[1]), POISON, dtype=x.dtype, device=x.device)
    big[pad:pad + x.shape[0]] = x
    return big[pad:pad + x.shape[0]]


def _sentinel_out(rows, N, dtype, dev):
    """(buffer, view of its first ``rows`` rows), all NaN: a row the kernel does not write stays NaN, and nothing may be written behind the last row."""
    buf = torch.full((rows + 8, N), float("nan"), dtype=dtype, device=dev)
    return buf, buf[:rows]


def _check_sentinels(tag, buf, out):
    assert bool(torch.isfinite(out.float()).all()), f"{tag}: non-finite output (a poisoned byte was read, or an element was not written)"
    assert bool(torch.isnan(buf[out.shape[0]:]).all()), f"{tag}: written behind the last row"


def _activate(c, ref, S):
    if c.act == "none":
        return ref, S
    fn, lip = ACT_FN[c.act]
    return fn(ref), lip * S


def _nhwc(x):
    Bn, Cc, Hh, Ww = x.shape
    return x.permute(0, 2, 3, 1).reshape(Bn * Hh * Ww, Cc).contiguous()


def _conv_ref(x, w, stride=1, up=False):
    """3x3 convolution, padding 1, as unfold + matmul in fp64: x [B, Cin, H, W], w [Cout, Cin, 3, 3] -> channels-last rows [B*Ho*Wo, Cout]."""
    if up:
        x = F.interpolate(x, scale_factor=2, mode="nearest")
    cols = F.unfold(x, 3, padding=1, stride=stride)                 # [B, Cin*9, L]
    return (cols.transpose(1, 2) @ w.reshape(w.shape[0], -1).t()).reshape(-1, w.shape[0])


def _up2p_ref(x, w6):
    """The four 2x2-tap phase problems of conv3x3(nearest-up2(x)) on GIVEN phase weights: x [B, H, W, C], w6 [py, px, dy, dx, N, C] -> [B, 2H, 2W, N];
    output pixel (2y + py, 2x + px) reads the low-resolution pixels (y + py + dy - 1, x + px + dx - 1) (include/fairdiff_hip.h, FD_CONV_UP2P)."""
    Bn, Hh, Ww, _ = x.shape
    xp = F.pad(x, (0, 0, 1, 1, 1, 1))
    out = x.new_zeros(Bn, 2 * Hh, 2 * Ww, w6.shape[4])
    for py in range(2):
        for px in range(2):
            acc = 0
            for dy in range(2):
                for dx in range(2):
                    acc = acc + xp[:, py + dy:py + dy + Hh, px + dx:px + dx + Ww] @ w6[py, px, dy, dx].t()
            out[:, py::2, px::2] = acc
    return out


def _unit_sums(c, rows=32):
    """fp64 statement of fd_gemm_desc.gn_stats: per 32-row chunk and 10-channel unit the (sum, sum of squares) of the STORED values, and the same on |values|."""
    M, N = c.shape
    pad = (-M) % rows
    x = torch.cat([c.double(), torch.zeros(pad, N, dtype=torch.float64, device=c.device)]).reshape((M + pad) // rows, rows, N // 10, 10)
    return torch.stack([x.sum((1, 3)), (x * x).sum((1, 3))], -1), torch.stack([x.abs().sum((1, 3)), (x * x).sum((1, 3))], -1)


def _check_stats(name, out, stored):
    """The statistics table against fp64 sums of the stored values: 320 fp32 additions per entry (B1 with the fp32 half-ulp)."""
    st = getattr(out, "gn_stats", None)
    assert st is not None and st[1] == 32, f"{name}: no statistics left behind"
    ref, S = _unit_sums(stored)
    assert st[0].shape == ref.shape, (st[0].shape, ref.shape)
    B(f"{name}: gn_stats", st[0], ref, S, 320)


def _run_dense(ops, dev, c, with_res):
    M, N, K, K2 = c.M, c.N, c.K, c.K2
    a, b = rnd(M, K, dev=dev, seed=1), rnd(N, K, dev=dev, scale=0.1, seed=2)
    # the operand sits inside a larger buffer whose other bytes are huge: a lane that read past its row, or past row M, would show
    wide = torch.full((M + 8, K + 64), 6e4, dtype=H16, device=dev)
    wide[:M, :K] = a
    aa = wide[:M, :K]
    kw = {}
    ref, S = a.double() @ b.double().t(), a.double().abs() @ b.double().abs().t()
    if K2:
        a2, b2 = rnd(M, K2, dev=dev, seed=3), rnd(N, K2, dev=dev, seed=4)
        kw.update(a2=a2, b2=b2)
        ref += a2.double() @ b2.double().t()
        S += a2.double().abs() @ b2.double().abs().t()
    ref, S = ref * c.alpha, S * abs(c.alpha)
    if c.colscale:
        f32 = float(torch.tensor(c.colscale[0], dtype=torch.float32))
        ref[:, :c.colscale[1]] *= f32
        S[:, :c.colscale[1]] *= f32
        kw.update(colscale=c.colscale)
    if "b" in c.operands:
        bias = rnd(N, dev=dev, dtype=torch.float32, seed=5)
        kw.update(bias=bias)
        ref, S = ref + bias.double(), S + bias.double().abs()
    if "r" in c.operands:
        rb = rnd(1, N, dev=dev, seed=7)
        kw.update(rowbias=rb, rows_per_batch=M)
        ref, S = ref + rb.double(), S + rb.double().abs()
    ref, S = _activate(c, ref, S)
    res = None
    if with_res:
        res = rnd(M, N, dev=dev, seed=6)
        kw.update(residual=res)
        ref, S = ref + res.double(), S + res.double().abs()
    if c.family == "skinny":        # output inside a wider buffer: nothing may be written beyond column N
        buf = torch.full((M, N + 8), 7.0, dtype=H16, device=dev)
        out = ops.gemm(aa, b, out=buf[:, :N])
        assert bool((buf[:, N:] == 7.0).all()), f"{c.id}: written beyond column N"
    else:
        sbuf, out = _sentinel_out(M, N, torch.float32 if c.out == "f32" else H16, dev)
        ops.gemm(aa, b, alpha=c.alpha, act=c.act, out=out, gn_stats=c.gn_stats, **kw)
        _check_sentinels(c.id, sbuf, out)
    return out, out, ref, S, res


def _run_geglu(ops, dev, c):
    """act = "geglu": C [M, N / 2] = value * gelu(gate) of the projection's two halves, each ROUNDED to fp16 first (gemm_epilogue_geglu_lds; bit-identical to
    fd_gemm followed by fd_geglu_fwd), with the pre-gate projection as a second output.  The projection is a one-rounding GEMM: gate B.  The gated output has a
    stored intermediate: gate C against the emulation (fp32-accumulated projection rounded to fp16, the gate in fp32, one rounding)."""
    M, N, K, Fh = c.M, c.N, c.K, c.N // 2
    a, w, bias = rnd(M, K, dev=dev, seed=1), rnd(N, K, dev=dev, scale=0.1, seed=2), rnd(N, dev=dev, dtype=torch.float32, seed=5)
    wide = torch.full((M + 8, K + 64), POISON, dtype=H16, device=dev)
    wide[:M, :K] = a
    wi, bi = ops.interleave_geglu(w, bias)
    aux = torch.full((M, N), float("nan"), dtype=H16, device=dev)
    sbuf, out = _sentinel_out(M, Fh, H16, dev)
    ops.gemm(wide[:M, :K], wi, bias=bi, act="geglu", out=out, aux=aux)
    _check_sentinels(c.id, sbuf, out)
    proj = torch.cat([aux[:, 0::2], aux[:, 1::2]], 1)              # back to [value | gate]
    x = a.double() @ w.double().t() + bias.double()
    S = a.double().abs() @ w.double().abs().t() + bias.double().abs()
    pe = (KB.mm32(a, w.t()) + bias).to(H16).float()
    emu = (pe[:, :Fh] * F.gelu(pe[:, Fh:])).to(H16)
    return out, proj, x, S, x[:, :Fh] * F.gelu(x[:, Fh:]), emu


def _run_conv(ops, dev, c, with_res):
    Bn, Hh, Ww, Cin, mode = c.conv
    N = c.N
    bias = rnd(N, dev=dev, dtype=torch.float32, seed=3) if "b" in c.operands else None
    if mode == GC.TRANS2:           # the data gradient of a stride-2 convolution N -> Cin on a [2H, 2W] map: g [B, Cin, H, W] -> dx [B, N, 2H, 2W]
        g, wf = rnd(Bn, Cin, Hh, Ww, dev=dev, seed=1), rnd(Cin, N, 3, 3, dev=dev, scale=0.05, seed=2)
        wk = wf.flip(2, 3).permute(1, 2, 3, 0).reshape(N, 9 * Cin).contiguous()
        pair = []
        for gg, ww in ((g.double(), wf.double()), (g.double().abs(), wf.double().abs())):
            xx = torch.zeros(Bn, N, 2 * Hh, 2 * Ww, dtype=torch.float64, device=dev, requires_grad=True)
            _conv_ref(xx, ww, stride=2).backward(_nhwc(gg))
            pair.append(_nhwc(xx.grad))
        (ref, S), x = pair, g
    else:
        x, w = rnd(Bn, Cin, Hh, Ww, dev=dev, seed=1), rnd(N, Cin, 3, 3, dev=dev, scale=0.05, seed=2)
        wk = w.permute(0, 2, 3, 1).reshape(N, 9 * Cin).contiguous()
        kw = dict(stride=2 if mode == GC.STRIDE2 else 1, up=mode == GC.UP2)
        ref, S = _conv_ref(x.double(), w.double(), **kw), _conv_ref(x.double().abs(), w.double().abs(), **kw)
    assert ref.shape == (c.M, N), (ref.shape, c.M, N)
    kw = {}
    if bias is not None:
        kw.update(bias=bias)
        ref, S = ref + bias.double(), S + bias.double().abs()
    if "r" in c.operands:           # one row per image
        rb = rnd(Bn, N, dev=dev, seed=5)
        kw.update(rowbias=rb)
        per = c.M // Bn
        ref, S = ref + rb.double().repeat_interleave(per, 0), S + rb.double().abs().repeat_interleave(per, 0)
    ref, S = _activate(c, ref, S)
    res = None
    if with_res:
        res = rnd(c.M, N, dev=dev, seed=4)
        kw.update(residual=res)
        ref, S = ref + res.double(), S + res.double().abs()
    sbuf, out = _sentinel_out(c.M, N, H16, dev)
    ops.conv3x3(_poisoned_rows(_nhwc(x)), wk, Bn, Hh, Ww, mode=mode, act=c.act, out=out, gn_stats=c.gn_stats, **kw)
    _check_sentinels(c.id, sbuf, out)
    return out, out, ref, S, res


def _phase_major(t):
    """[B, 2H, 2W, N] -> [4][B*H*W][N] as rows, phase = py * 2 + px"""
    return torch.stack([t[:, py::2, px::2].reshape(-1, t.shape[-1]) for py in range(2) for px in range(2)]).reshape(-1, t.shape[-1])


def _run_up2p(ops, dev, c):
    from finetune_fair_diffusion_amd import lib
    Bn, Hh, Ww, Cin, mode = c.conv
    N = c.N
    bias = rnd(N, dev=dev, dtype=torch.float32, seed=3) if "b" in c.operands else None
    if mode == GC.UP2P_BWD:         # A = dOut [B, H, W, Cin] at the high resolution; phase weights [py, px, dy, dx, Cin, N] of the forward N -> Cin
        lo_h, lo_w = Hh // 2, Ww // 2
        g, w6 = rnd(Bn, Hh, Ww, Cin, dev=dev, seed=1), rnd(2, 2, 2, 2, Cin, N, dev=dev, scale=0.05, seed=2)
        wk = w6.permute(5, 0, 1, 2, 3, 4).reshape(N, 16 * Cin).contiguous()
        pair = []
        for gg, ww in ((g.double(), w6.double()), (g.double().abs(), w6.double().abs())):
            xx = torch.zeros(Bn, lo_h, lo_w, N, dtype=torch.float64, device=dev, requires_grad=True)
            _up2p_ref(xx, ww).backward(gg)
            pair.append(xx.grad.reshape(-1, N))
        (ref, S), x, rows_out = pair, g.reshape(-1, Cin), Bn * lo_h * lo_w
    else:
        x4, w6 = rnd(Bn, Hh, Ww, Cin, dev=dev, seed=1), rnd(2, 2, 2, 2, N, Cin, dev=dev, scale=0.05, seed=2)
        wk = w6.permute(0, 1, 4, 2, 3, 5).reshape(4 * N, 4 * Cin).contiguous()
        ref, S = _up2p_ref(x4.double(), w6.double()), _up2p_ref(x4.double().abs(), w6.double().abs())
        if bias is not None:
            ref, S = ref + bias.double(), S + bias.double().abs()
        # phase-major [4][M][N] (FD_CONV_UP2P) or the channels-last result (FD_CONV_UP2PI)
        lay = _phase_major if mode == GC.UP2P else (lambda t: t.reshape(-1, N))
        ref, S, x, rows_out = lay(ref), lay(S), x4.reshape(-1, Cin), 4 * c.M
    assert ref.shape == (rows_out, N), (ref.shape, rows_out, N)
    x = _poisoned_rows(x)
    sbuf, out = _sentinel_out(rows_out, N, H16, dev)
    ptr = dict(A=x.data_ptr(), B=wk.data_ptr(), C=out.data_ptr(), gn_stats=0)
    if bias is not None:
        ptr["bias"] = bias.data_ptr()
    d = GC.descriptor(c, lib.GemmDesc, pointers=ptr)
    ops._gemm_call(d, True, out, c.gn_stats)
    _check_sentinels(c.id, sbuf, out)
    # gn_stats of FD_CONV_UP2PI: phase-major chunks of the low-resolution rows
    stored = _phase_major(out.reshape(Bn, 2 * Hh, 2 * Ww, N)) if mode == GC.UP2PI else out
    return out, stored, ref, S, None


@pytest.mark.parametrize("case_id", [c.id for c in GC.CASES])
def test_gemm_case(ops, dev, case_id):
    c = GC.BY_ID[case_id]
    T = c.K + c.K2 + len(c.operands) + (4 if c.act != "none" else 0)
    if c.act == "geglu":
        timer, ops.TIMER = ops.TIMER, ops.OpTimer()
        try:
            out, proj, x, S, ref, emu = _run_geglu(ops, dev, c)
            launched = [(r[0], s[-1]) for r, s in zip(ops.TIMER.records, ops.TIMER.shapes)]
        finally:
            ops.TIMER = timer
        assert launched == [(c.kernel, c.split)], f"{c.id}: launched {launched}, the table says {(c.kernel, c.split)}"
        tag = f"{c.id} {c.M}x{c.N}x{c.K} [{c.kernel}]"
        B(f"{tag}: pre-gate projection", proj, x, S, c.K + 1)
        C(f"{tag}: value * gelu(gate)", out, ref, emu)
        return
    for with_res in ((True, False) if "R" in c.operands else (False,)):
        timer, ops.TIMER = ops.TIMER, ops.OpTimer()
        try:
            if c.family in ("dense", "skinny"):
                out, stored, ref, S, res = _run_dense(ops, dev, c, with_res)
            elif c.family == "conv":
                out, stored, ref, S, res = _run_conv(ops, dev, c, with_res)
            else:
                out, stored, ref, S, res = _run_up2p(ops, dev, c)
            launched = [(r[0], s[-1]) for r, s in zip(ops.TIMER.records, ops.TIMER.shapes)]
        finally:
            ops.TIMER = timer
        # the dispatch, asked of the descriptor that was launched
        assert launched == [(c.kernel, c.split)], f"{c.id}: launched {launched}, the table says {(c.kernel, c.split)}"
        # Which band: the table's rule (gemm_cases.expected_roundings, restated from the source of the epilogues -- not asked of the library).  What the gate
        # makes of it: a launch labelled ONE rounding fails if the kernel rounds twice (B2 1.7 .. 3.9 on the CPU); a launch labelled two would also pass
        # if it rounded once, so the label "2" is a permission, not a finding.
        roundings = GC.expected_roundings(c, with_res)
        assert roundings in (0, 1, 2) and (roundings == 2) <= (with_res and c.out == "f16") and (not with_res or roundings == c.roundings)
        tag = f"{c.id} {c.M}x{c.N}x{c.K}+{c.K2} [{c.kernel}{' split ' + str(c.split) if c.split else ''}] {'with' if with_res else 'without'} residual"
        assert bool(torch.isfinite(out.float()).all()), f"{tag}: non-finite output"
        B(tag, out, ref, S, T - (0 if with_res or "R" not in c.operands else 1), roundings=max(roundings, 1), residual=res)
        if c.gn_stats:
            _check_stats(tag, out, stored)
        del out, stored, ref, S, res
    torch.cuda.synchronize()


# ============================================================================= fp32-output accumulators under B1
@pytest.mark.parametrize("M,N,R,ldx_extra,arm", [(1000, 320, 4, 0, "vectorised, padded rank 8"), (1000, 324, 4, 0, "plain 8 (N % 8 = 4)"), (1000, 320, 8, 4, "plain 8 (ldx % 8 = 4)"),
                                                 (1000, 320, 16, 0, "vectorised, padded rank 16"), (1000, 322, 12, 0, "plain 16 (N % 4 = 2)"), (1000, 320, 16, 2, "plain 16 (ldx % 4 = 2)"),
                                                 (1000, 320, 24, 0, "plain 32"), (4097, 648, 50, 0, "plain 64")])
def test_lora_wgrad_every_arm(ops, dev, M, N, R, ldx_extra, arm):
    """G[n, r] += scale * sum_m X[m, n] T[m, r] at ranks and alignments that reach all six kernels of fd_lora_wgrad (csrc/lora.hip: the vectorised kernel needs
    N and ldx multiples of 8 at padded rank 8, of 4 at 16; everything else takes lora_wgrad_partial<8 / 16 / 32 / 64>), X a column slice of a wider buffer.
    The arm named in the id is derived here from that condition as the source states it; the library has no query for it."""
    RP = 8 if R <= 8 else 16 if R <= 16 else 32 if R <= 32 else 64
    ldx = N + (ldx_extra or 8)
    buf = rnd(M, ldx, dev=dev, seed=1)
    X = buf[:, :N]
    vec = (RP == 8 and N % 8 == 0 and ldx % 8 == 0) or (RP == 16 and N % 4 == 0 and ldx % 4 == 0)
    assert vec == arm.startswith("vectorised"), (arm, N, ldx, RP)
    Tm = torch.zeros(M, RP, dtype=H16, device=dev)
    Tm[:, :R] = rnd(M, R, dev=dev, seed=2)
    ref = 0.5 * X.double().t() @ Tm[:, :R].double()
    S = 0.5 * X.double().abs().t() @ Tm[:, :R].double().abs()
    G = torch.ones(N, R, dtype=torch.float32, device=dev)
    ops.lora_wgrad(X, Tm, G, R, 1, R, scale=0.5)
    B(f"lora_wgrad {arm} M{M} N{N} R{R} ldx{ldx} [N, R]", G, 1 + ref, 1 + S, M + 1)
    G2 = torch.zeros(R, N, dtype=torch.float32, device=dev)
    ops.lora_wgrad(X, Tm, G2, 1, N, R, scale=0.5)
    B(f"lora_wgrad {arm} M{M} N{N} R{R} ldx{ldx} [R, N]", G2, ref.t(), S.t(), M)


@pytest.mark.parametrize("R", [4, 16])
def test_lora_wgrad_multi(ops, dev, R):
    """fd_lora_wgrad_multi: mixed M / N, strided X, both output layouts, one partial + one final launch."""
    RP = 8 if R <= 8 else 16
    probs = []
    for i, (M, N, trans) in enumerate([(1000, 320, False), (2048, 640, True), (77, 768, False), (4100, 1280, True), (333, 320, True)]):
        buf = rnd(M, N + 64, dev=dev, seed=10 + i)
        Tm = torch.zeros(M, RP, dtype=H16, device=dev)
        Tm[:, :R] = rnd(M, R, dev=dev, seed=20 + i)
        probs.append((buf[:, 32:32 + N], Tm, trans))
    outs = [torch.ones((R, X.shape[1]) if trans else (X.shape[1], R), dtype=torch.float32, device=dev) for X, _, trans in probs]
    with ops.wgrad_batch():
        for (X, Tm, trans), G in zip(probs, outs):
            ops.lora_wgrad(X, Tm, G, *((1, X.shape[1]) if trans else (R, 1)), R, scale=0.5)
    for i, ((X, Tm, trans), G) in enumerate(zip(probs, outs)):
        ref, S = 0.5 * X.double().t() @ Tm[:, :R].double(), 0.5 * X.double().abs().t() @ Tm[:, :R].double().abs()
        B(f"lora_wgrad_multi R{R} problem {i} ({X.shape[0]}x{X.shape[1]}, {'[R, N]' if trans else '[N, R]'})", G, 1 + (ref.t() if trans else ref), 1 + (S.t() if trans else S),
          X.shape[0] + 1)


@pytest.mark.parametrize("Bn,Hh,T,d", [(2, 8, 300, 40), (3, 4, 77, 80), (1, 4, 130, 160)])
def test_attn_bwd_prep(ops, dev, Bn, Hh, T, d):
    o, do = rnd(Bn * T, Hh * d, dev=dev, seed=1), rnd(Bn * T, Hh * d, dev=dev, seed=2)
    D = torch.full((Bn, Hh, T), float("nan"), dtype=torch.float32, device=dev)
    ops._call("fd_attn_bwd_prep", ops._p(o), ops._p(do), ops._p(D), Bn, Hh, T, d, ops._stream())
    prod = (o.double() * do.double()).view(Bn, T, Hh, d)
    B(f"attn_bwd_prep B{Bn} H{Hh} T{T} d{d}", D, prod.sum(-1).permute(0, 2, 1), prod.abs().sum(-1).permute(0, 2, 1), d)


# ============================================================================= gate C: single-rounding ops against an fp32 emulation
def _both(fn, *xs):
    """(fp64 statement, its fp32 emulation rounded once) of ``fn`` on the same fp16 / fp32 data."""
    ref = fn(*[x.double() for x in xs])
    emu = fn(*[x.float() for x in xs])
    return ref, emu


@pytest.mark.parametrize("Bn,HW,C1,C2,silu", [(2, 256, 320, 0, True), (3, 64, 1280, 640, True), (2, 100, 640, 320, False)])
def test_groupnorm_gate_c(ops, dev, Bn, HW, C1, C2, silu):
    G, eps = 32, 1e-5
    x1 = (rnd(Bn * HW, C1, dev=dev, seed=1).float() * 2 + 0.5).to(H16)
    x2 = (rnd(Bn * HW, C2, dev=dev, seed=2).float() - 0.3).to(H16) if C2 else None
    Cc = C1 + C2
    gamma, beta = rnd(Cc, dev=dev, dtype=torch.float32, seed=3) * 0.2 + 1, rnd(Cc, dev=dev, dtype=torch.float32, seed=4) * 0.2
    dy, add1 = rnd(Bn * HW, Cc, dev=dev, seed=5), rnd(Bn * HW, C1, dev=dev, seed=6)
    xc = torch.cat([x1, x2], 1) if C2 else x1
    outs = {}
    for key, cast in (("ref", torch.Tensor.double), ("emu", torch.Tensor.float)):
        xr = cast(xc).reshape(Bn, HW, Cc).permute(0, 2, 1).requires_grad_(True)
        y = F.group_norm(xr, G, cast(gamma), cast(beta), eps)
        y = F.silu(y) if silu else y
        y.backward(cast(dy).reshape(Bn, HW, Cc).permute(0, 2, 1))
        gx = xr.grad.permute(0, 2, 1).reshape(Bn * HW, Cc)
        outs[key] = (y.detach().permute(0, 2, 1).reshape(Bn * HW, Cc), gx[:, :C1] + cast(add1), gx[:, C1:])
    y, st = ops.groupnorm(x1, x2, Bn, HW, G, eps, gamma, beta, silu)
    dx1, dx2 = ops.groupnorm_bwd(x1, x2, dy, Bn, HW, G, st, gamma, beta, silu, add1=add1)
    tag = f"groupnorm B{Bn} HW{HW} C{C1}+{C2} silu={int(silu)}"
    C(f"{tag}: fwd", y, outs["ref"][0], outs["emu"][0].to(H16))
    C(f"{tag}: bwd dx1 (+ add)", dx1, outs["ref"][1], outs["emu"][1].to(H16))
    if C2:
        C(f"{tag}: bwd dx2", dx2, outs["ref"][2], outs["emu"][2].to(H16))


@pytest.mark.parametrize("M,Cc", [(333, 1280), (64, 768), (515, 320)])
def test_layernorm_gate_c(ops, dev, M, Cc):
    x = (rnd(M, Cc, dev=dev, seed=1).float() * 3 + 1).to(H16)
    gamma, beta = rnd(Cc, dev=dev, dtype=torch.float32, seed=2) * 0.2 + 1, rnd(Cc, dev=dev, dtype=torch.float32, seed=3) * 0.2
    dy, add = rnd(M, Cc, dev=dev, seed=4), rnd(M, Cc, dev=dev, seed=5)
    outs = {}
    for key, cast in (("ref", torch.Tensor.double), ("emu", torch.Tensor.float)):
        xr = cast(x).requires_grad_(True)
        y = F.layer_norm(xr, (Cc,), cast(gamma), cast(beta), 1e-5)
        y.backward(cast(dy))
        outs[key] = (y.detach(), xr.grad + cast(add))
    y, st = ops.layernorm(x, gamma, beta, 1e-5, save_stats=True)
    C(f"layernorm {M}x{Cc}: fwd", y, outs["ref"][0], outs["emu"][0].to(H16))
    C(f"layernorm {M}x{Cc}: bwd + add", ops.layernorm_bwd(x, dy, gamma, st, add=add), outs["ref"][1], outs["emu"][1].to(H16))


@pytest.mark.parametrize("cols", [7, 255, 256, 257, 1000, 4096])
def test_softmax_rows_gate_c(ops, dev, cols):
    rows = 64
    x = (rnd(rows, cols, dev=dev, seed=cols).float() * 4).to(H16)
    dp = rnd(rows, cols, dev=dev, seed=cols + 2)
    for scale in (0.125, 1.0):
        ref, emu = _both(lambda t: torch.softmax(t * scale, -1), x)
        p = ops.softmax_rows(x, scale)
        C(f"softmax cols={cols} scale={scale}", p, ref, emu.to(H16))
        # the backward's statement takes the probabilities the kernel is given (p as stored)
        bwd = lambda pp, dd: scale * pp * (dd - (pp * dd).sum(-1, keepdim=True))
        gref, gemu = _both(bwd, p, dp)
        C(f"softmax bwd cols={cols} scale={scale} (from the stored p)", ops.softmax_rows_bwd(p, dp, scale), gref, gemu.to(H16))


ACTS = [("silu", F.silu), ("relu", F.relu), ("hardswish", F.hardswish), ("hardsigmoid", F.hardsigmoid), ("quick_gelu", lambda t: t * torch.sigmoid(1.702 * t)), ("gelu", F.gelu)]


@pytest.mark.parametrize("act", [a for a, _ in ACTS])
def test_activations_gate_c(ops, dev, act):
    fn = dict(ACTS)[act]
    n, cols = 1031 * 1003, 1003                 # n % 8 = 5: the tail of the 8-wide body
    x, dy = (rnd(n, dev=dev, seed=3).float() * 3).to(H16), rnd(n, dev=dev, seed=4)
    outs = {}
    for key, cast in (("ref", torch.Tensor.double), ("emu", torch.Tensor.float)):
        xr = cast(x).requires_grad_(True)
        y = fn(xr)
        y.backward(cast(dy))
        outs[key] = (y.detach(), xr.grad)
    C(f"act {act}", ops.act_fwd(x, act), outs["ref"][0], outs["emu"][0].to(H16), cols=cols)
    C(f"act_bwd {act}", ops.act_bwd(x, dy, act), outs["ref"][1], outs["emu"][1].to(H16), cols=cols)


def test_geglu_and_add_gate_c(ops, dev):
    M, Fh = 300, 1280
    proj, dy = rnd(M, 2 * Fh, dev=dev, seed=1), rnd(M, Fh, dev=dev, seed=2)
    outs = {}
    for key, cast in (("ref", torch.Tensor.double), ("emu", torch.Tensor.float)):
        pr = cast(proj).requires_grad_(True)
        a_, g_ = pr.chunk(2, dim=-1)
        y = a_ * F.gelu(g_)
        y.backward(cast(dy))
        outs[key] = (y.detach(), pr.grad)
    C("geglu fwd", ops.geglu(proj), outs["ref"][0], outs["emu"][0].to(H16))
    C("geglu bwd", ops.geglu_bwd(proj, dy), outs["ref"][1], outs["emu"][1].to(H16))
    wi = torch.stack([proj[:, :Fh], proj[:, Fh:]], dim=2).reshape(M, 2 * Fh).contiguous()
    d_il = ops.geglu_bwd_interleaved(wi, dy)
    C("geglu bwd interleaved", torch.cat([d_il[:, 0::2], d_il[:, 1::2]], 1), outs["ref"][1], outs["emu"][1].to(H16))
    n, cols = 1031 * 1003, 1003
    a, b = rnd(n, dev=dev, seed=5), rnd(n, dev=dev, seed=6)
    ref, emu = _both(lambda s, t: 0.5 * s - 2.0 * t, a, b)
    C("add", ops.add(a, b, 0.5, -2.0), ref, emu.to(H16), cols=cols)
    C("add b=None", ops.add(a, None, -1.5, 3.0), -1.5 * a.double(), (-1.5 * a.float()).to(H16), cols=cols)


def test_se_pieces_and_depthwise_convolutions_gate_c(ops, dev):
    Bn, HW, Cc = 4, 49, 120
    xa, s, dy = rnd(Bn, HW, Cc, dev=dev, seed=10), rnd(Bn, Cc, dev=dev, seed=11), rnd(Bn, HW, Cc, dev=dev, seed=12)
    ref, emu = _both(lambda t: t.mean(1), xa)
    C("avgpool", ops.avgpool_hw(xa.reshape(-1, Cc), Bn, HW, Cc), ref, emu.to(H16))
    ref, emu = _both(lambda t, u: t * u[:, None], xa, s)
    C("scale_channels", ops.scale_channels(xa.reshape(-1, Cc), s, Bn, HW, Cc).reshape(Bn * HW, Cc), ref.reshape(Bn * HW, Cc), emu.to(H16).reshape(Bn * HW, Cc))
    dx, ds = ops.scale_channels_bwd(xa.reshape(-1, Cc), s, dy.reshape(-1, Cc), Bn, HW, Cc)
    ref, emu = _both(lambda t, u: t * u[:, None], dy, s)
    C("scale_channels dx", dx, ref.reshape(Bn * HW, Cc), emu.to(H16).reshape(Bn * HW, Cc))
    ref, emu = _both(lambda t, u: (t * u).sum(1), dy, xa)
    C("scale_channels ds", ds, ref, emu.to(H16))
    C2 = 72
    for k, st in [(3, 1), (3, 2), (5, 1), (5, 2)]:
        xd = rnd(Bn, C2, 15, 14, dev=dev, seed=6)
        wd, bd = rnd(C2, 1, k, k, dev=dev, dtype=torch.float32, scale=0.3, seed=7), rnd(C2, dev=dev, dtype=torch.float32, seed=8)
        wkk = wd.reshape(C2, k * k).t().contiguous()
        fwd = lambda t, w_, b_: F.hardswish(F.conv2d(t, w_, b_, stride=st, padding=(k - 1) // 2, groups=C2))
        ref, emu = _both(fwd, xd, wd, bd)
        y, Ho, Wo = ops.dwconv(_nhwc(xd), wkk, bd, Bn, 15, 14, C2, k, st, "hardswish")
        assert (Ho, Wo) == tuple(ref.shape[2:])
        C(f"dwconv k{k}s{st}", y, _nhwc(ref), _nhwc(emu).to(H16))
        g = rnd(*ref.shape, dev=dev, seed=9)
        grads = {}
        for key, cast in (("ref", torch.Tensor.double), ("emu", torch.Tensor.float)):
            xr = cast(xd).requires_grad_(True)
            F.conv2d(xr, cast(wd), None, stride=st, padding=(k - 1) // 2, groups=C2).backward(cast(g))
            grads[key] = xr.grad
        C(f"dwconv bwd k{k}s{st}", ops.dwconv_bwd(_nhwc(g), wkk, Bn, 15, 14, C2, k, st), _nhwc(grads["ref"]), _nhwc(grads["emu"]).to(H16))


# ============================================================================= gate C: attention against the emulation of csrc/attn.hip's arithmetic
def _heads(t, Bn, T, Hh, d):
    """[Bn * T, Hh * d] -> [Bn * Hh, T, d]"""
    return t.reshape(Bn, T, Hh, d).permute(0, 2, 1, 3).reshape(Bn * Hh, T, d)


def _rows_of(t, Bn, T, Hh, d):
    """[Bn * Hh, T, d] -> [Bn * T, Hh * d]"""
    return t.reshape(Bn, Hh, T, d).permute(0, 2, 1, 3).reshape(Bn * T, Hh * d)


@pytest.mark.parametrize("Bn,Hh,Tq,Tk,d,prescaled", [(2, 8, 300, 300, 40, False), (2, 8, 300, 300, 40, True), (2, 8, 200, 77, 40, True), (2, 8, 200, 77, 40, False),
                                                      (2, 4, 150, 200, 80, False), (1, 4, 100, 130, 160, False)])
def test_attention_gate_c(ops, dev, Bn, Hh, Tq, Tk, d, prescaled):
    """fd_attn_fwd, fd_attn_bwd_dq, fd_attn_bwd_dkdv with partial query and key tiles (tiles of 64 keys, 128-row query blocks)."""
    Cc, scale = Hh * d, d ** -0.5
    q, k, v, do = (rnd(Bn * T, Cc, dev=dev, seed=s) for s, T in ((1, Tq), (2, Tk), (3, Tk), (4, Tq)))
    fac = ops.q_prescale(d)
    if prescaled:
        assert fac is not None and abs(fac - scale * KB.LOG2E) < 1e-12
        qs = (q.float() * fac).to(H16)                      # what the projection's epilogue writes (one rounding)
        q_true = qs.double() / fac                          # the query the stored values stand for
    else:
        qs, q_true = q, q.double()
    qr, kr, vr = (_heads(t, Bn, T, Hh, d).requires_grad_(True) for t, T in ((q_true, Tq), (k.double(), Tk), (v.double(), Tk)))
    oref = torch.softmax(qr @ kr.transpose(1, 2) * scale, -1) @ vr
    oref.backward(_heads(do.double(), Bn, Tq, Hh, d))
    o_emu, lse2 = KB.attn_fwd_emulation(_heads(qs, Bn, Tq, Hh, d), _heads(k, Bn, Tk, Hh, d), _heads(v, Bn, Tk, Hh, d), scale, prescaled=prescaled)
    dq_e, dk_e, dv_e = KB.attn_bwd_emulation(_heads(qs, Bn, Tq, Hh, d), _heads(k, Bn, Tk, Hh, d), _heads(v, Bn, Tk, Hh, d), o_emu, _heads(do, Bn, Tq, Hh, d), lse2, scale,
                                             prescaled=prescaled)
    o, lse = ops.attn_fwd(qs, k, v, Bn, Hh, Tq, Tk, d, 1, need_lse=True, prescaled=prescaled)
    dq, dk, dv = ops.attn_bwd(qs, k, v, o, do, lse, Bn, Hh, Tq, Tk, d, 1, prescaled=prescaled)
    tag = f"attn{' (pre-scaled q)' if prescaled else ''} B{Bn} H{Hh} Tq{Tq} Tk{Tk} d{d}"
    lse_ref = torch.logsumexp(qr.detach() @ kr.detach().transpose(1, 2) * scale, -1).reshape(Bn, Hh, Tq)
    err = float((lse.double() - lse_ref).abs().max())
    # the denominator is summed from the probabilities ROUNDED to fp16 (csrc/attn.hip, attn_fwd_kernel: "the fp16-rounded probabilities the numerator is built
    # from"): |dl / l| <= 2^-11, so |d lse| <= 2^-11, plus the fp32 arithmetic on values of the size of lse
    bound = 2.0 ** -11 + 2.0 ** -16 * max(1.0, float(lse_ref.abs().max()))
    print(f"[{tag}: lse] max abs err {err:.2e} (bound {bound:.2e})")
    assert err <= bound
    C(f"{tag}: o", o, _rows_of(oref.detach(), Bn, Tq, Hh, d), _rows_of(o_emu, Bn, Tq, Hh, d))
    C(f"{tag}: dq", dq, _rows_of(qr.grad, Bn, Tq, Hh, d), _rows_of(dq_e, Bn, Tq, Hh, d))
    C(f"{tag}: dk", dk, _rows_of(kr.grad, Bn, Tk, Hh, d), _rows_of(dk_e, Bn, Tk, Hh, d))
    C(f"{tag}: dv", dv, _rows_of(vr.grad, Bn, Tk, Hh, d), _rows_of(dv_e, Bn, Tk, Hh, d))


def _small_attn_statement(q, k, v, do, key_valid, Hh, d, scale, causal):
    """softmax(q k^T scale + mask) v and its gradients from the formulas of csrc/smallattn.hip (dP = dO v^T, dS = P (dP - sum_j P dP), dq = dS k scale,
    dk = dS^T q scale, dv = P^T dO) in the dtype of the arguments: fp64 is the reference, fp32 rounded once the emulation (the kernel's math is fp32, no MFMA,
    the probabilities are saved in fp32)."""
    Bq, T, _ = q.shape
    sp = lambda t: t.view(Bq, T, Hh, d).permute(0, 2, 1, 3)
    back = lambda t: t.permute(0, 2, 1, 3).reshape(Bq, T, Hh * d)
    ok = torch.ones(Bq, 1, T, T, dtype=torch.bool, device=q.device)
    if causal:
        ok = ok & torch.ones(T, T, dtype=torch.bool, device=q.device).tril()
    if key_valid is not None:
        ok = ok & (key_valid != 0)[:, None, None, :]
    P = torch.softmax((sp(q) @ sp(k).transpose(-1, -2) * scale).masked_fill(~ok, -math.inf), -1)
    dP = sp(do) @ sp(v).transpose(-1, -2)
    dS = P * (dP - (P * dP).sum(-1, keepdim=True))
    return back(P @ sp(v)), back(dS @ sp(k) * scale), back(dS.transpose(-1, -2) @ sp(q) * scale), back(P.transpose(-1, -2) @ sp(do))


@pytest.mark.parametrize("T,d", [(63, 40), (65, 64), (77, 64), (128, 32)])
def test_small_attn_gate_c(ops, dev, T, d):
    Bq, Hh, scale = 4, 12, d ** -0.5
    Cc = Hh * d
    q, k, v, do = (rnd(Bq, T, Cc, dev=dev, seed=s) for s in (1, 2, 3, 4))
    g = torch.Generator().manual_seed(T * 1000 + d)
    kv = (torch.rand(Bq, T, generator=g) < 0.6).int()
    kv[:, 0] = 1
    kv = kv.to(dev)
    for causal, key_valid in ((True, None), (True, kv), (False, kv)):
        ref = _small_attn_statement(q.double(), k.double(), v.double(), do.double(), key_valid, Hh, d, scale, causal)
        emu = _small_attn_statement(q.float(), k.float(), v.float(), do.float(), key_valid, Hh, d, scale, causal)
        o, P = ops.small_attn_fwd(q, k, v, key_valid, Bq, Hh, T, d, scale, causal=causal, save_p=True)
        got = (o,) + tuple(ops.small_attn_bwd(q, k, v, P, do, Bq, Hh, T, d, scale))
        for name, x, r, e in zip(("o", "dq", "dk", "dv"), got, ref, emu):
            C(f"small_attn T{T} d{d} causal={int(causal)} mask={int(key_valid is not None)}: {name}", x.reshape(Bq * T, Cc), r.reshape(Bq * T, Cc), e.to(H16).reshape(Bq * T, Cc))


@pytest.mark.parametrize("Cc,Bq,HW,L,kv_div", [(320, 4, 64, 77, 2), (320, 2, 128, 5, 1), (640, 2, 64, 80, 1)])
def test_cross_attn_block_gate_c(ops, dev, Cc, Bq, HW, L, kv_div):
    """fd_cross_attn_block without LoRA slabs: LayerNorm2 -> to_q -> attention over L prompt tokens -> to_out + residual -> LayerNorm3 in one launch.  The
    emulation follows the stored intermediates csrc/crossattn.hip documents: n2 rounded to fp16 (P0); q rounded ONCE after the multiplication by
    scale log2(e) (P1, line 13 of its header comment and include/fairdiff_hip.h "Rounding contract"); the probabilities rounded to fp16 (``p16``) and o rounded
    into the tile (P2); h2 = fp16(fp16(o Wo^T + bias) + x), "the rounding sequence of the fp16 library's LDS-staged fd_gemm epilogue" (P3); LayerNorm3 of the
    stored h2."""
    Hh, d, M, Bk = 8, Cc // 8, Bq * HW, Bq // kv_div
    scale = d ** -0.5
    x = rnd(M, Cc, dev=dev, seed=1)
    g2, b2 = rnd(Cc, dev=dev, dtype=torch.float32, seed=2) * 0.2 + 1, rnd(Cc, dev=dev, dtype=torch.float32, seed=3) * 0.2
    g3, b3 = rnd(Cc, dev=dev, dtype=torch.float32, seed=4) * 0.2 + 1, rnd(Cc, dev=dev, dtype=torch.float32, seed=5) * 0.2
    wq, wo = rnd(Cc, Cc, dev=dev, scale=Cc ** -0.5, seed=6), rnd(Cc, Cc, dev=dev, scale=Cc ** -0.5, seed=7)
    bo = rnd(Cc, dev=dev, dtype=torch.float32, seed=8) * 0.1
    k, v = rnd(Bk * L, Cc, dev=dev, seed=9), rnd(Bk * L, Cc, dev=dev, seed=10)
    assert ops.cross_block_ok(M, Cc, Hh, L, HW)
    vt = ops.transpose_btc(v, Bk, L, Cc, ops.CROSS_LP)
    y, yn, _, _ = ops.cross_attn_block(x, (g2, b2, 1e-5), wq, k, vt, L, wo, bo, (g3, b3, 1e-5), Hh, HW, kv_div)
    kk, vv = (_heads(t.reshape(Bk, L, Cc).repeat_interleave(kv_div, 0).reshape(Bq * L, Cc), Bq, L, Hh, d) for t in (k, v))
    # fp64 statement
    n2 = F.layer_norm(x.double(), (Cc,), g2.double(), b2.double(), 1e-5)
    qr = _heads(n2 @ wq.double().t(), Bq, HW, Hh, d)
    o = _rows_of(torch.softmax(qr @ kk.double().transpose(1, 2) * scale, -1) @ vv.double(), Bq, HW, Hh, d)
    yr = o @ wo.double().t() + bo.double() + x.double()
    # emulation
    n2e = F.layer_norm(x.float(), (Cc,), g2, b2, 1e-5).to(H16)
    qe = (KB.mm32(n2e, wq.t()) * (scale * KB.LOG2E)).to(H16)
    oe, _ = KB.attn_fwd_emulation(_heads(qe, Bq, HW, Hh, d), kk, vv, scale, prescaled=True)
    he = (KB.mm32(_rows_of(oe, Bq, HW, Hh, d), wo.t()) + bo).to(H16)
    ye = (he.float() + x.float()).to(H16)
    tag = f"cross_attn_block C{Cc} B{Bq} HW{HW} L{L} kv_div{kv_div}"
    C(f"{tag}: y", y, yr, ye)
    C(f"{tag}: LayerNorm3(y)", yn, F.layer_norm(yr, (Cc,), g3.double(), b3.double(), 1e-5), F.layer_norm(ye.float(), (Cc,), g3, b3, 1e-5).to(H16))


# ============================================================================= the small dispatcher arms no other test launches
@pytest.mark.parametrize("Cin,Cout,k,stride,nchw,f32,act", [(5, 16, 3, 1, True, False, "none"), (4, 4, 3, 2, True, True, "hardswish"), (3, 12, 3, 1, False, False, "none"),
                                                            (4, 20, 3, 2, False, True, "none"), (6, 10, 1, 1, True, True, "none"), (4, 4, 1, 1, False, False, "hardswish")])
def test_conv_small_cin_generic_kernel(ops, dev, Cin, Cout, k, stride, nchw, f32, act):
    """conv_small_cin_kernel (the fast path needs k = 3, Cin in {3, 4}, Cout % 8 == 0 and Cout >= 16): k = 3 with Cin = 5 or Cout = 4 / 12 / 20, NHWC input,
    fp32 input at k = 1, on an odd map.  fp32 accumulation over <= 9 Cin + 1 terms, one rounding: gate B."""
    Bn, Hh, Ww = 2, 13, 11
    x = rnd(Bn, Cin, Hh, Ww, dev=dev, seed=1, dtype=torch.float32 if f32 else H16)
    w, bias = rnd(Cout, Cin, k, k, dev=dev, dtype=torch.float32, scale=0.2, seed=2), rnd(Cout, dev=dev, dtype=torch.float32, seed=3)
    wk = w.permute(2, 3, 1, 0).reshape(k * k * Cin, Cout).contiguous()
    xin = x if nchw else x.permute(0, 2, 3, 1).contiguous()
    y, Ho, Wo = ops.conv_small_cin(xin, wk, bias, Bn, Hh, Ww, Cin, Cout, k, stride, nchw=nchw, act=act)
    pad = (k - 1) // 2
    ref = F.conv2d(x.double(), w.double(), bias.double(), stride=stride, padding=pad)
    S = F.conv2d(x.double().abs(), w.double().abs(), bias.double().abs(), stride=stride, padding=pad)
    assert (Ho, Wo) == tuple(ref.shape[2:])
    tag = f"conv_small_cin generic {Cin}->{Cout} k{k} s{stride} {'nchw' if nchw else 'nhwc'} {'f32' if f32 else 'f16'} {act}"
    if act == "hardswish":          # |hardswish'| <= 1.5: the accumulation band passes through the activation scaled by that
        ref, S = F.hardswish(ref), 1.5 * S
    B(tag, y, _nhwc(ref), _nhwc(S), k * k * Cin + 1)


@pytest.mark.parametrize("k,stride,scale,Hh,Ww", [(1, 1, 1.0, 13, 11), (1, 2, 0.37, 13, 11), (3, 2, 0.37, 13, 11), (3, 1, -2.5, 8, 9)])
def test_conv_small_cin_bwd_arms(ops, dev, k, stride, scale, Hh, Ww):
    """fd_conv_small_cin_bwd at k = 1 and with scale != 1 on an odd image at stride 2 (fp32 output: B1)."""
    Bn, Cin, Cout = 2, 4, 24
    w = rnd(Cout, Cin, k, k, dev=dev, dtype=torch.float32, scale=0.2, seed=2)
    wk = w.permute(2, 3, 1, 0).reshape(k * k * Cin, Cout).contiguous()
    pad = (k - 1) // 2
    Ho, Wo = (Hh + 2 * pad - k) // stride + 1, (Ww + 2 * pad - k) // stride + 1
    g = rnd(Bn, Cout, Ho, Wo, dev=dev, seed=4)
    pair = []
    for gg, ww in ((g.double(), w.double()), (g.double().abs(), w.double().abs())):
        xx = torch.zeros(Bn, Cin, Hh, Ww, dtype=torch.float64, device=dev, requires_grad=True)
        F.conv2d(xx, ww, None, stride=stride, padding=pad).backward(gg)
        pair.append(xx.grad)
    dx = ops.conv_small_cin_bwd(_nhwc(g), wk, Bn, Hh, Ww, Cin, Cout, k, stride, scale=scale)
    B(f"conv_small_cin_bwd k{k} s{stride} scale {scale} {Hh}x{Ww}", dx, scale * pair[0], abs(scale) * pair[1], k * k * Cout + 1)


def test_avgpool_hw_bwd_with_add(ops, dev):
    Bn, HW, Cc = 3, 49, 120
    dy, add = rnd(Bn, Cc, dev=dev, seed=1), rnd(Bn * HW, Cc, dev=dev, seed=2)
    fn = lambda g, a: (g / HW)[:, None].expand(Bn, HW, Cc).reshape(Bn * HW, Cc) + a
    ref, emu = _both(fn, dy, add)
    C("avgpool_hw_bwd + add", ops.avgpool_hw_bwd(dy, Bn, HW, Cc, add=add), ref, emu.to(H16))
    ref, emu = _both(lambda g: (g / HW)[:, None].expand(Bn, HW, Cc).reshape(Bn * HW, Cc), dy)
    C("avgpool_hw_bwd", ops.avgpool_hw_bwd(dy, Bn, HW, Cc), ref, emu.to(H16))
