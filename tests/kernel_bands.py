"""The error bands of the direct kernel tests, generic over the 16-bit working dtype (pure torch: no GPU, no library).  tests/run_bf16_kernel_checks.py
binds them to bf16, tests/test_kernels_sharp_gpu.py uses them in fp16; tests/test_bf16_bands_cpu.py and tests/test_fp16_bands_cpu.py hold them without a GPU.

Gate A (coarse): ``coarse`` = max|got - ref| / max|ref|.  It does not see a dropped k-term at long K or a column scaled by one ulp; gates B and C do.

Gate B (fp32 accumulation, then the stated number of roundings to the 16-bit dtype: every fd_gemm path, and the fp32-output accumulators, which take the fp32
half-ulp in place of the 16-bit one and skip B2).  ``ref`` is the fp64 statement, ``S`` the same statement on absolute values, ``T`` the number of summed terms.
  ONE rounding (``roundings=1``):
    B1, elementwise:  |got - ref| <= 0.5 ulp(max(|ref|, |got|)) + 2 T 2^-24 S -- half an ulp of the one rounding plus the forward bound of T fp32 additions in
        any order (T u S to first order), doubled because the MFMA's internal summation order and rounding are not specified.
    B2, per row and per column:  rms((got - ref) / ulp(max(|ref|, 2^-3 rms(ref of that row / column)))) <= B2_MARGIN x the same statistic of ref rounded once.
        The floor keeps elements that cancelled to nearly zero, whose error is set by the larger terms that made them, from dominating.
  TWO roundings (``roundings=2``, ``residual`` given): the fp16 library's LDS-staged epilogue parks act(acc + bias + rowbias) in LDS in the working dtype and adds
  the residual on the way out, round(round(act(acc + bias + rowbias)) + residual) -- what an fp16 eager baseline computes too.
    B1 adds 0.5 ulp(ref - residual), the first rounding (of the pre-residual value).
    B2's yardstick is the same two-rounding statement on the fp64 reference, round16(round16(ref - residual) + residual), not the one-rounding one.
  Both are derived, not measured.  What the derivation buys (CPU, fp16, tests/test_fp16_bands_cpu.py prints it): the two-rounding arithmetic fails the
  one-rounding gate (B1 at K = 40, B2 1.7 .. 3.9 at every K), passes its own, and with one k-term dropped passes B1 at K >= 1280 but scores B2 >= 3.5: both
  parts are needed.
  B2 margins (B2_MARGINS[dtype][roundings]): 1.25 x the largest ratio, over rows and columns and every K + K2 of the GEMM-family problems, of the statistic of
  the fp32-accumulate emulation (an fp32 matmul of the 16-bit operands + second slab + bias + residual, rounded as stated) to that of the yardstick, rounded
  up to two decimals.  Recomputed by the two CPU tests:
      bf16, one rounding    K = 40 .. 11520 (run_bf16_kernel_checks.py)   largest ratio 1.000   margin 1.25 (B2_MARGIN)
      fp16, one rounding    K + K2 = 48 .. 11520 (gemm_cases.KS)          largest ratio 1.0004  margin 1.26
      fp16, two roundings   K + K2 = 48 .. 11520                          largest ratio 1.0326  margin 1.30
  (two roundings: where the fp32 accumulation error carries the pre-residual value across a rounding boundary the FIRST rounding lands on the other
  neighbour, a whole ulp of the pre-residual value away from the yardstick's; that happens to a few elements per thousand at K >= 2000.)
  Every margin is below 2, so the floor stands.

Gate C (everything whose arithmetic is fp32 over 16-bit operands with documented 16-bit stored intermediates and ONE final rounding: norms, softmax,
activations, GEGLU, elementwise, depthwise / small convolutions, attention).  The yardstick is never the kernel: it is a plain torch emulation of the stated
arithmetic on the same data (below: attn_fwd_emulation, attn_bwd_emulation; for the single-rounding ops the fp32 torch statement rounded once).  Two
statistics, both with the 2^-3 rms floor: the B2-form RMS per row and per column, and the elementwise maximum in ulps.  Each must be <= its margin x the same
statistic of the emulation.  The margins are 1.25 x the largest ratio of that statistic between emulation variants a kernel is free to differ by -- the
one-shot softmax against the online form over 64-key tiles, forward against reversed key order, both ways round -- and, for the maximum, between three seeds
of the same problem (a maximum over ~10^5 elements is a sample of a tail).  Measured on the CPU on attention problems (d = 40 / 80 / 160, Tq 100 .. 300,
Tk 77 .. 300, rows of 320 .. 640 elements; tests/test_fp16_bands_cpu.py recomputes and prints them):
      RMS per row      tiled / one-shot <= 1.485, reversed / forward <= 1.002                          -> C_MARGIN_ROW = 1.88
      RMS per column   tiled / one-shot <= 1.658, reversed / forward <= 1.003                          -> C_MARGIN_COL = 2.10
      maximum          tiled / one-shot <= 1.073, reversed / forward <= 1.000, seed to seed <= 1.180   -> C_MARGIN_MAX = 1.50
  (each rounded up with 0.02 .. 0.03 of room, since the last digit depends on the CPU's exp2).  The RMS ratios are this wide because an attention output's
  error is a handful of rounding errors of its largest probabilities, shared by all d columns of a head: a row of 8 heads holds few independent samples.  The
  planted errors of the CPU test -- one key dropped, one column scaled by 1 + 2^-8, a softmax scale off by 2^-7 -- score 10 .. 1300.
"""
import math

import torch

B2_MARGIN = 1.25                    # bf16, one rounding (the name tests/run_bf16_kernel_checks.py has always used)
B2_MARGINS = {torch.bfloat16: {1: B2_MARGIN}, torch.float16: {1: 1.26, 2: 1.30}}
C_MARGIN_ROW, C_MARGIN_COL, C_MARGIN_MAX = 1.88, 2.10, 1.50

_FORMAT = {torch.float16: (10, -14), torch.bfloat16: (7, -126)}     # (explicit mantissa bits, exponent of the smallest normal)


def ulp(x, dtype):
    """Spacing of ``dtype`` numbers at magnitude |x| (fp64 tensor): 2^(floor(log2|x|) - p); below the smallest normal the subnormal spacing
    (fp16: 2^-24 below 2^-14; bf16: 2^-133 below 2^-126)."""
    p, emin = _FORMAT[dtype]
    a = x.abs().double().clamp_min(2.0 ** emin)
    return torch.exp2(torch.floor(torch.log2(a)) - p)


def coarse(got, ref, dtype=None):
    """Gate A statistic: max|got - ref| / max|ref| (the same in every dtype)."""
    got, ref = got.detach().double(), ref.detach().double()
    return float((got - ref).abs().max() / (ref.abs().max() + 1e-300))


def _b2_stat(x, ref, dim, dtype):
    rms = ref.pow(2).mean(dim, keepdim=True).sqrt()
    u = ulp(torch.maximum(ref.abs(), 0.125 * rms), dtype)
    return ((x - ref) / u).pow(2).mean(dim).sqrt()


def _rows(t):
    return t.reshape(-1, t.shape[-1])


def gate_b(got, ref, S, T, dtype, rounded=True, roundings=1, residual=None, margin=None):
    """Gate B (module docstring).  ``rounded=False``: fp32 output (half an fp32 ulp, no B2).  ``roundings=2`` needs ``residual``.
    Returns a dict: b1_bad (elements over the B1 band), b1_ratio (max |err| / band), b2_row / b2_col (largest ratio to the yardstick; None for fp32
    outputs), ok_b1, ok_b2."""
    assert roundings in (1, 2) and (roundings == 1 or (rounded and residual is not None)), "two roundings: a 16-bit output and its residual"
    margin = B2_MARGINS[dtype][roundings] if margin is None else margin
    got, ref, S = got.detach().double(), ref.detach().double(), S.detach().double()
    err = (got - ref).abs()
    half = 0.5 * ulp(torch.maximum(ref.abs(), got.abs()), dtype) if rounded else 2.0 ** -24 * torch.maximum(ref.abs(), got.abs())
    if roundings == 2:
        res = residual.detach().double()
        half = half + 0.5 * ulp(ref - res, dtype)
    band = half + 2.0 * T * 2.0 ** -24 * S
    ratio = err / band.clamp_min(1e-300)
    out = dict(b1_bad=int((err > band).sum()), b1_ratio=float(ratio.max()), b2_row=None, b2_col=None)
    if rounded:
        r2 = _rows(ref)
        g2 = got.reshape(r2.shape)
        if roundings == 2:
            yard = ((ref - res).to(dtype).double() + res).to(dtype).double().reshape(r2.shape)
        else:
            yard = ref.to(dtype).double().reshape(r2.shape)
        for key, dim in (("b2_row", 1), ("b2_col", 0)):
            out[key] = float((_b2_stat(g2, r2, dim, dtype) / _b2_stat(yard, r2, dim, dtype).clamp_min(0.05)).max())
    out["ok_b1"] = out["b1_bad"] == 0 and math.isfinite(out["b1_ratio"])
    out["ok_b2"] = (not rounded) or (out["b2_row"] <= margin and out["b2_col"] <= margin)
    return out


def gate_c_stat(got, ref, dtype, floor=None):
    """Elementwise maximum of |got - ref| in ulps of max(|ref|, floor); floor = 2^-3 rms(ref) unless given.  ref rounded once scores <= 0.5."""
    got, ref = got.detach().double(), ref.detach().double()
    if floor is None:
        floor = 0.125 * float(ref.pow(2).mean().sqrt())
    emin = _FORMAT[dtype][1]
    return float(((got - ref).abs() / ulp(ref.abs().clamp_min(max(floor, 2.0 ** emin)), dtype)).max())


def gate_c(got, ref, emu, dtype):
    """Gate C (module docstring): the statistics of ``got`` over those of the emulation ``emu``, both against the fp64 ``ref``.
    Returns a dict: max (ulps of got), max_emu, max_ratio, rms_row / rms_col (largest per-row / per-column ratio), rms (largest RMS statistic of got), ok."""
    got, ref, emu = got.detach().double(), ref.detach().double(), emu.detach().double()
    assert got.shape == ref.shape == emu.shape, (got.shape, ref.shape, emu.shape)
    out = dict(max=gate_c_stat(got, ref, dtype), max_emu=gate_c_stat(emu, ref, dtype))
    out["max_ratio"] = out["max"] / max(out["max_emu"], 0.5)        # an emulation that hits every element exactly still allows the one rounding
    r2 = _rows(ref)
    g2, e2 = got.reshape(r2.shape), emu.reshape(r2.shape)
    out["rms"] = 0.0
    for key, dim in (("rms_row", 1), ("rms_col", 0)):
        sg, se = _b2_stat(g2, r2, dim, dtype), _b2_stat(e2, r2, dim, dtype)
        out[key] = float((sg / se.clamp_min(0.05)).max())
        out["rms"] = max(out["rms"], float(sg.max()))
    out["ok"] = all(math.isfinite(out[k]) for k in ("max", "rms_row", "rms_col")) and out["max_ratio"] <= C_MARGIN_MAX and \
        out["rms_row"] <= C_MARGIN_ROW and out["rms_col"] <= C_MARGIN_COL
    return out


# ============================================================================= emulations of the attention kernels' stated arithmetic (gate C yardsticks)
LOG2E = 1.4426950408889634


def mm32(x, y):
    """x . y with exact products summed in fp64 and rounded to fp32 once: an fp32-accumulated product whose result does not depend on the machine."""
    return (x.double() @ y.double()).float()


def attn_fwd_emulation(q, k, v, scale, tile=None, reverse=False, prescaled=False):
    """softmax(q k^T scale) v as csrc/attn.hip states it (attn_fwd_kernel): 16-bit operands, fp32 scores, p = exp2((s - m) scale log2 e) in fp32, P ROUNDED
    to the working dtype before the PV product (``pf[..] = (f16)p``), the denominator summed from the rounded probabilities (the ones column of V), the
    accumulator divided in fp32 and rounded once.  ``prescaled``: q holds q_true * scale * log2(e) rounded once by its projection (fd_gemm_desc.colscale) and the
    QK^T accumulator is the exponent's argument.  ``tile``: online softmax over key tiles of that many keys; ``reverse``: keys visited in reversed order.
    q [Z, Tq, d], k / v [Z, Tk, d] -> (o in the working dtype, lse2 fp32 = log2-domain log-sum-exp of the scaled scores)."""
    dtype = q.dtype
    sl2 = 1.0 if prescaled else scale * LOG2E
    if reverse:
        k, v = k.flip(1), v.flip(1)
    Tk = k.shape[1]
    tile = tile or Tk
    m = torch.full(q.shape[:2], -math.inf, device=q.device)
    l = torch.zeros(q.shape[:2], device=q.device)
    o = torch.zeros(q.shape[0], q.shape[1], v.shape[2], device=q.device)
    for k0 in range(0, Tk, tile):
        s = mm32(q, k[:, k0:k0 + tile].transpose(1, 2)) * sl2
        m_new = torch.maximum(m, s.max(-1).values)
        alpha = torch.exp2(m - m_new)
        p = torch.exp2(s - m_new[..., None]).to(dtype).float()
        l = l * alpha + p.sum(-1)
        o = o * alpha[..., None] + mm32(p, v[:, k0:k0 + tile])
        m = m_new
    return (o / l[..., None]).to(dtype), m + torch.log2(l)


def attn_bwd_emulation(q, k, v, o, do, lse2, scale, prescaled=False):
    """dq, dk, dv as attn_bwd_dq_kernel / attn_bwd_dkdv_kernel state them: D = rowsum(dO o O) in fp32; p = exp2(s scale log2 e - lse2) in fp32 from the saved
    log-sum-exp; dV = P^T dO with P ROUNDED to the working dtype (``pf[..] = (f16)p``); dS = p (dP - D) ROUNDED to the working dtype (``dsf[..] = (f16)(p *
    (dp - dd))``), dP = dO V^T in fp32; dq = (dS K) scale and dk = (dS^T q) scale (pre-scaled q: dS^T q' / log2 e), each rounded once."""
    dtype = q.dtype
    sl2 = 1.0 if prescaled else scale * LOG2E
    D = (do.float() * o.float()).sum(-1)
    p = torch.exp2(mm32(q, k.transpose(1, 2)) * sl2 - lse2[..., None])
    dp = mm32(do, v.transpose(1, 2))
    ds = (p * (dp - D[..., None])).to(dtype)
    dv = mm32(p.to(dtype).transpose(1, 2), do).to(dtype)
    dq = (mm32(ds, k) * scale).to(dtype)
    dk = (mm32(ds.transpose(1, 2), q) * (1.0 / LOG2E if prescaled else scale)).to(dtype)
    return dq, dk, dv
