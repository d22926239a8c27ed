"""Kernel-level parity at production shapes and edges (GPU): the C-ABI entry points that the end-to-end engine tests reach only at toy sizes with
loose bands -- text-encoder attention, row softmax with its mask, ViT patchify and the batched patch-embedding GEMM, the face-gradient rectangle
scale, the LoRA operand refresh, the slab sum, the casts, the finite check, grid-stride elementwise tails, crop-resize and face alignment at
production size -- each against a plain fp32 / fp64 PyTorch statement of the same op.  Ops that only move, cast or mask data must be bit-exact;
ops that write into part of a larger buffer must leave the rest of it untouched (sentinel fill)."""
import math

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from test_kernels_gpu import check, relerr, rnd  # noqa: F401  (same conventions and bands as the kernel suite)

pytestmark = pytest.mark.gpu

GRID = 4096 * 256          # threads of a full grid-stride launch (elementwise.hip: fd_grid_1d capped at 4096 blocks): larger sizes run a second pass


@pytest.fixture(scope="module")
def ops():
    from finetune_fair_diffusion_amd import ops
    return ops


def _bits16(t):
    return t.contiguous().view(torch.int16)


def _bits32(t):
    return t.contiguous().view(torch.int32)


def assert_bit_equal(name, got, ref):
    """Bit equality, with NaN compared as NaN (payloads may differ) and the sign of zero significant."""
    assert got.shape == ref.shape and got.dtype == ref.dtype, (name, got.shape, ref.shape, got.dtype, ref.dtype)
    gn, rn = torch.isnan(got), torch.isnan(ref)
    assert torch.equal(gn, rn), f"{name}: NaN pattern differs at {int((gn != rn).sum())} elements"
    bits = _bits16 if got.element_size() == 2 else _bits32
    diff = (bits(got) != bits(ref)) & ~rn
    if bool(diff.any()):
        i = int(diff.flatten().nonzero()[0])
        raise AssertionError(f"{name}: {int(diff.sum())} elements differ; first at {i}: got {got.flatten()[i].item()!r}, want {ref.flatten()[i].item()!r}")
    print(f"[{name}] bit-exact over {got.numel()} elements")


# ----------------------------------------------------------------------------- text-encoder attention (smallattn.hip)
def _small_attn_ref(q, k, v, key_valid, H, d, scale, causal):
    """fp64 statement: softmax(q k^T * scale + mask) v, per (batch, head); masked entries of P are 0."""
    B, T, _ = q.shape
    sp = lambda t: t.double().view(B, T, H, d).permute(0, 2, 1, 3)
    s = sp(q) @ sp(k).transpose(-1, -2) * scale
    ok = torch.ones(B, 1, T, T, dtype=torch.bool, device=q.device)
    if causal:
        ok = ok & torch.ones(T, T, dtype=torch.bool, device=q.device).tril()
    if key_valid is not None:
        ok = ok & (key_valid != 0)[:, None, None, :]
    P = torch.softmax(s.masked_fill(~ok, -math.inf), -1)
    return P, (P @ sp(v)).permute(0, 2, 1, 3).reshape(B, T, H * d), ok


def _bwd_lds_bytes(T, d):
    return (4 * T * (d + 1) + T * (T + 1)) * 4       # fd_small_attn_bwd: q, k, v, dO and dS tiles in LDS


@pytest.mark.parametrize("B,H,T,d", [(2, 12, 77, 64), (1, 2, 1, 64), (1, 2, 63, 64), (1, 2, 64, 64), (1, 2, 65, 64), (1, 2, 127, 64), (1, 2, 128, 64),
                                     (2, 3, 77, 32), (2, 3, 77, 40), (1, 2, 128, 128)])
def test_small_attention_vs_fp64(ops, dev, B, H, T, d):
    """fd_small_attn_fwd / _bwd (CLIP text encoder; production (2, 12, 77, 64)): keys j >= 64 go through the second lane pass (u = 1).  Causal on
    and off; key_valid None, the unconditional-prompt pattern [1, 1, 0, ...] and random masks with key 0 valid.  The saved P against fp64 probabilities
    (masked entries exactly 0), the output and dq / dk / dv within the attention bands.  The backward refuses shapes beyond its 160 KiB of LDS."""
    C, scale = H * d, d ** -0.5
    q, k, v = rnd(B, T, C, dev=dev, seed=1), rnd(B, T, C, dev=dev, seed=2), rnd(B, T, C, dev=dev, seed=3)
    do = rnd(B, T, C, dev=dev, seed=4)
    g = torch.Generator().manual_seed(T * 1000 + d)
    uncond = torch.zeros(B, T, dtype=torch.int32)
    uncond[:, :2] = 1
    rand = (torch.rand(B, T, generator=g) < 0.6).int()
    rand[:, 0] = 1
    bwd_ok = _bwd_lds_bytes(T, d) <= 160 * 1024
    for causal in (True, False):
        for mname, kv in (("none", None), ("uncond", uncond), ("random", rand)):
            kvd = kv.to(dev) if kv is not None else None
            tag = f"small attn B{B} H{H} T{T} d{d} causal={int(causal)} mask={mname}"
            o, P = ops.small_attn_fwd(q, k, v, kvd, B, H, T, d, scale, causal=causal, save_p=True)
            Pr, orf, ok = _small_attn_ref(q, k, v, kvd, H, d, scale, causal)
            assert bool((P[~ok.expand_as(P)] == 0).all()), f"{tag}: masked probabilities are not exactly 0"
            check(f"{tag}: P", P, Pr, 1e-5)
            check(f"{tag}: o", o, orf, 2e-3)
            if not bwd_ok:
                continue
            qr, kr, vr = (t.double().requires_grad_(True) for t in (q, k, v))
            _, oa, _ = _small_attn_ref(qr, kr, vr, kvd, H, d, scale, causal)
            oa.backward(do.double())
            dq, dk, dv = ops.small_attn_bwd(q, k, v, P, do, B, H, T, d, scale)
            check(f"{tag}: dq", dq, qr.grad, 3e-3)
            check(f"{tag}: dk", dk, kr.grad, 3e-3)
            check(f"{tag}: dv", dv, vr.grad, 3e-3)
    if not bwd_ok:
        with pytest.raises(RuntimeError, match="LDS"):
            ops.small_attn_bwd(q, k, v, P, do, B, H, T, d, scale)


# ----------------------------------------------------------------------------- row softmax (elementwise.hip)
@pytest.mark.parametrize("cols", [1, 7, 255, 256, 257, 1000, 4095, 4096])
def test_softmax_rows_widths_and_large_magnitudes(ops, dev, cols):
    """fd_softmax_rows / _bwd at every width class of the one-block-per-row kernel (16 values per thread), incl. rows whose scaled
    entries reach |x * scale| ~ 1e4 (the maximum subtraction must happen before the exponential)."""
    rows = 37
    x = rnd(rows, cols, dev=dev, seed=cols) * 4
    x[:5] = (rnd(5, cols, dev=dev, seed=cols + 1).float() * 5e3).clamp(-6e4, 6e4).half()     # |x| up to ~2e4
    for scale in (0.125, 1.0):
        xr = x.float().requires_grad_(True)
        ref = torch.softmax(xr * scale, -1)
        p = ops.softmax_rows(x, scale)
        check(f"softmax cols={cols} scale={scale}", p, ref, 2e-3)
        dp = rnd(rows, cols, dev=dev, seed=cols + 2)
        ref.backward(dp.float())
        check(f"softmax bwd cols={cols} scale={scale}", ops.softmax_rows_bwd(p, dp, scale), xr.grad, 5e-3)


def test_softmax_rows_mask_path(ops, dev):
    """The additive fp32 mask of fd_softmax_rows: row r reads mask row (r / mask_ht) * mask_t + r % mask_t (include/fairdiff_hip.h), here with
    mask_t = T query rows per head and mask_ht = H * T rows per sample -- one [T, cols] mask per sample shared by its heads.  A row whose every
    entry is masked (-inf) has no probability distribution: the kernel returns NaN there, as torch.softmax does, so that such a row cannot pass
    for a valid one downstream."""
    B, H, T, cols = 3, 4, 9, 77
    x = rnd(B * H * T, cols, dev=dev, seed=1) * 3
    g = torch.Generator().manual_seed(7)
    mask = torch.randn(B * T, cols, generator=g) * 2
    mask[torch.rand(B * T, cols, generator=g) < 0.3] = -math.inf
    mask[:, 0] = 0.0                                           # every row keeps one finite entry
    mask = mask.to(dev)
    rows = torch.arange(B * H * T, device=dev)
    mrow = (rows // (H * T)) * T + rows % T
    ref = torch.softmax(0.5 * x.float() + mask[mrow], -1)
    check("softmax masked", ops.softmax_rows(x, 0.5, mask=mask, mask_t=T, mask_ht=H * T), ref, 2e-3)
    masked_out = ref == 0
    assert bool((ops.softmax_rows(x, 0.5, mask=mask, mask_t=T, mask_ht=H * T)[masked_out] == 0).all())
    # fully masked: mask row 4 (sample 0, query row 4) -> rows h * T + 4 of sample 0
    mask2 = mask.clone()
    mask2[4] = -math.inf
    y = ops.softmax_rows(x, 0.5, mask=mask2, mask_t=T, mask_ht=H * T)
    full = (mrow == 4)
    assert bool(torch.isnan(y[full]).all()), "a fully masked row must come back NaN"
    assert not bool(torch.isnan(y[~full]).any())
    check("softmax masked (other rows)", y[~full], ref[~full], 2e-3)


# ----------------------------------------------------------------------------- patchify (ViT image regularisers)
CLIP_MEAN, CLIP_STD = (0.48145466, 0.4578275, 0.40821073), (0.26862954, 0.26130258, 0.27577711)
DINO_MEAN, DINO_STD = (0.485, 0.456, 0.406), (0.229, 0.224, 0.225)


def _patchify_ref(x, mean, std, P):
    # the C-ABI takes mean / std as fp32: the statement uses those constants, evaluated in fp64
    m = torch.tensor(mean, dtype=torch.float32, device=x.device).double()[None, :, None, None]
    s = torch.tensor(std, dtype=torch.float32, device=x.device).double()[None, :, None, None]
    xn = ((x + 1) / 2 - m) / s
    u = F.unfold(xn, kernel_size=P, stride=P)                 # [N, 3*P*P, g*g], k = c*P*P + py*P + px, patches row-major
    return u.permute(0, 2, 1).reshape(-1, u.shape[1])


def _ulp16(t):
    a = t.abs().clamp_min(2.0 ** -14)
    return torch.exp2(torch.floor(torch.log2(a)) - 10)


@pytest.mark.parametrize("N,S,P,Kp,norm", [(8, 224, 14, 592, "clip"), (8, 224, 14, 592, "dino"), (2, 56, 14, 592, "clip"), (2, 64, 16, 776, "dino")])
def test_patchify_fwd_bwd(ops, dev, N, S, P, Kp, norm):
    """fd_patchify_fwd against F.unfold of ((x + 1) / 2 - mean) / std (fp64) to one fp16 ulp, padding columns >= 3 P^2 exactly 0; 224^2 x 8 is over
    1 M outputs, so the grid-stride loop runs.  fd_patchify_bwd against autograd of that statement, with scale != 1, plain and accumulating."""
    mean, std = (CLIP_MEAN, CLIP_STD) if norm == "clip" else (DINO_MEAN, DINO_STD)
    x = (torch.rand(N, 3, S, S, generator=torch.Generator().manual_seed(S + P)) * 2 - 1).half().to(dev)
    K3 = 3 * P * P
    out = ops.patchify(x, mean, std, P, Kp)
    ref = _patchify_ref(x.double(), mean, std, P)
    assert out.shape == (N * (S // P) ** 2, Kp)
    assert bool((out[:, K3:] == 0).all()) and not bool(torch.signbit(out[:, K3:]).any())
    err = ((out[:, :K3].double() - ref).abs() / _ulp16(ref)).max().item()
    print(f"[patchify {N}x{S} P{P} Kp{Kp} {norm}] max err {err:.3f} fp16 ulp")
    assert err <= 1.0
    dp = rnd(out.shape[0], Kp, dev=dev, seed=5)
    xr = x.double().requires_grad_(True)
    for scale in (1.0 / 1024, 0.37):
        xr.grad = None
        (_patchify_ref(xr, mean, std, P) * dp[:, :K3].double()).sum().mul(scale).backward()
        got = ops.patchify_bwd(dp, std, N, S, P, scale=scale)
        check(f"patchify bwd scale={scale}", got, xr.grad, 1e-6)
        acc = rnd(N, 3, S, S, dev=dev, dtype=torch.float32, seed=6)
        got2 = ops.patchify_bwd(dp, std, N, S, P, scale=scale, out=acc.clone())
        check(f"patchify bwd accumulate scale={scale}", got2, acc.double() + xr.grad, 1e-6)


# ----------------------------------------------------------------------------- batched patch-embedding GEMM (ViT)
@pytest.mark.parametrize("Z", [1, 3, 8])
@pytest.mark.parametrize("N", [768, 1280])
def test_gemm_batched_patch_embedding(ops, dev, Z, N):
    """ops.gemm_batched_into: rows 1..256 of every sample's [264, N] token buffer = patches . W^T + bias + position table (bias and table shared
    by all z); the class-token row 0 and the pad rows 257..263 keep their sentinel.  ops.gemm_batched_from: the input gradient of the patch
    embedding, reading [Z, 256, D] row slices of a [Z, 264, D] buffer."""
    rows, K, Tp = 256, 592, 264
    a = rnd(Z * rows, K, dev=dev, seed=1)
    w = rnd(N, K, dev=dev, scale=0.05, seed=2)
    bias = rnd(N, dev=dev, dtype=torch.float32, seed=3)
    pos = rnd(rows, N, dev=dev, seed=4)
    x = torch.full((Z, Tp, N), -7.0, dtype=torch.float16, device=dev)
    ops.gemm_batched_into(a, w, x[:, 1:rows + 1], bias, pos, Z, rows)
    ref = (a.float().view(Z, rows, K) @ w.float().t()) + bias + pos.float()
    check(f"gemm_batched_into Z={Z} N={N}", x[:, 1:rows + 1], ref, 2e-3)
    assert bool((x[:, 0] == -7.0).all()) and bool((x[:, rows + 1:] == -7.0).all()), "rows outside 1..256 were written"
    buf = rnd(Z, Tp, N, dev=dev, seed=5)
    wT = rnd(K, N, dev=dev, scale=0.05, seed=6)
    got = ops.gemm_batched_from(buf[:, 1:rows + 1], wT, Z, rows)
    check(f"gemm_batched_from Z={Z} D={N}", got.view(Z, rows, K), buf[:, 1:rows + 1].float() @ wT.float().t(), 2e-3)


# ----------------------------------------------------------------------------- face-gradient rectangle scale
def test_rect_scale_bit_exact(ops, dev):
    """fd_rect_scale (the face gradient hook): inside rect_b = [x0, y0, x1, y1) (x indexes W, y indexes H) dimg *= factor_b, elsewhere unchanged.
    H != W pins the index order; empty, inverted, full-image and edge-touching rectangles; per-sample factors incl. 0 and negative."""
    B, H, W = 8, 48, 80
    rects = torch.tensor([[0, 0, 0, 0], [30, 10, 20, 40], [0, 0, W, H], [60, 30, W, H], [5, 7, 33, 19], [70, 0, W, 10], [0, 40, 10, H],
                          [W - 1, H - 1, W, H]], dtype=torch.int32)
    factors = torch.tensor([2.0, 3.0, 0.5, -1.25, 0.0, 1.0 / 3.0, 7.0, 1e-3], dtype=torch.float32)
    dimg = rnd(B, 3, H, W, dev=dev, dtype=torch.float32, seed=1)
    ys = torch.arange(H)[:, None]
    xs = torch.arange(W)[None, :]
    mask = torch.stack([(xs >= r[0]) & (xs < r[2]) & (ys >= r[1]) & (ys < r[3]) for r in rects.tolist()])[:, None].to(dev)
    ref = dimg * torch.where(mask, factors.to(dev)[:, None, None, None], torch.ones((), device=dev))
    got = ops.rect_scale(dimg.clone(), rects.to(dev), factors.to(dev))
    assert_bit_equal("rect_scale", got, ref)
    assert int(mask[0].sum()) == 0 and int(mask[1].sum()) == 0 and int(mask[2].sum()) == H * W


# ----------------------------------------------------------------------------- LoRA operand refresh
@pytest.mark.parametrize("npairs", [1, 16, 17, 40])
@pytest.mark.parametrize("scale", [1.0, 0.25])
def test_lora_refresh_multi_bit_exact(dev, npairs, scale):
    """fd_lora_refresh_multi (16 pairs per launch; 17 and 40 pairs take several): down16 = down.half(), up16 = (up * scale).half() and their
    transposes, rank padding rows / columns r..rp exactly 0, into row-strided views whose columns past the operand keep their sentinel."""
    from finetune_fair_diffusion_amd.layers import LoRAPair, ParamBank, refresh_pairs
    ranks, dims = (1, 4, 16, 50), ((320, 320), (768, 320), (320, 1280), (1280, 768))
    shapes = {}
    for i in range(npairs):
        r = ranks[i % 4]
        K, N = dims[(i // 4) % 4]
        shapes[f"d{i}"], shapes[f"u{i}"] = (r, K), (N, r)
    bank = ParamBank(shapes, dev)
    g = torch.Generator().manual_seed(npairs)
    bank.flat.copy_((torch.randn(bank.numel, generator=g) * 0.3).to(dev))
    pairs, bufs = [], []
    SENT = -7.0
    for i in range(npairs):
        p = LoRAPair(bank, f"d{i}", f"u{i}")
        assert p.rp > p.r or p.r == 16
        b = dict(d=torch.full((p.rp, p.K + 24), SENT, dtype=torch.float16, device=dev), dT=torch.full((p.K, p.rp + 8), SENT, dtype=torch.float16, device=dev),
                 u=torch.full((p.N, p.rp + 8), SENT, dtype=torch.float16, device=dev), uT=torch.full((p.rp, p.N + 16), SENT, dtype=torch.float16, device=dev))
        p.place(b["d"][:, :p.K], b["dT"][:, :p.rp], b["u"][:, :p.rp], b["uT"][:, :p.N])
        pairs.append(p)
        bufs.append(b)
    refresh_pairs(pairs, scale)
    for i, (p, b) in enumerate(zip(pairs, bufs)):
        down, up = bank.view(p.dn), bank.view(p.un)
        r, rp = p.r, p.rp
        dh, uh = down.half(), (up * scale).half()
        tag = f"pair {i} (r={r} rp={rp} K={p.K} N={p.N} scale={scale})"
        assert torch.equal(_bits16(p.down16[:r]), _bits16(dh)), tag + ": down16"
        assert torch.equal(_bits16(p.downT16[:, :r]), _bits16(dh.t())), tag + ": downT16"
        assert torch.equal(_bits16(p.up16[:, :r]), _bits16(uh)), tag + ": up16"
        assert torch.equal(_bits16(p.upT16[:r]), _bits16(uh.t())), tag + ": upT16"
        for name, pad in (("down16", p.down16[r:]), ("downT16", p.downT16[:, r:]), ("up16", p.up16[:, r:]), ("upT16", p.upT16[r:])):
            assert bool((_bits16(pad) == 0).all()), f"{tag}: {name} rank padding is not +0"
        for name, extra in (("down16", b["d"][:, p.K:]), ("downT16", b["dT"][:, rp:]), ("up16", b["u"][:, rp:]), ("upT16", b["uT"][:, p.N:])):
            assert bool((extra == SENT).all()), f"{tag}: {name} wrote past its row"
    print(f"[lora refresh {npairs} pairs scale={scale}] bit-exact")


# ----------------------------------------------------------------------------- fixed-order slab sum
def test_sum_slabs_bit_exact_sequential(ops, dev):
    """fd_sum_slabs: out[i] = in[0][i] + in[1][i] + ... in slab order (fp32), bit for bit; n = 2^21 + 4 needs more than 2048 blocks x 256
    threads x 4 floats, so the grid-stride loop runs.  n % 4 != 0 is refused on the host."""
    for n in (4, 1028, (1 << 21) + 4):
        for nslab in (1, 2, 3, 8):
            x = rnd(nslab, n, dev=dev, dtype=torch.float32, seed=nslab * 7 + n % 97) * torch.logspace(-3, 3, nslab, device=dev)[:, None]
            out = torch.full((n,), float("nan"), dtype=torch.float32, device=dev)
            ops._call("fd_sum_slabs", ops._p(x), ops._p(out), nslab, n, ops._stream())
            ref = x[0].clone()
            for s in range(1, nslab):
                ref = ref + x[s]
            assert_bit_equal(f"sum_slabs n={n} nslab={nslab}", out, ref)
    x = torch.zeros(2, 8, dtype=torch.float32, device=dev)
    with pytest.raises(RuntimeError, match="multiple of 4"):
        ops._call("fd_sum_slabs", ops._p(x), ops._p(x[1]), 1, 6, ops._stream())


# ----------------------------------------------------------------------------- casts
_SPECIAL32 = [0.0, -0.0, 2.0 ** -24, -(2.0 ** -24), 2.0 ** -25, 3 * 2.0 ** -26, -(3 * 2.0 ** -26), 1e-6, -1e-6, 2.0 ** -15, 6.1e-5, 6.1035156e-5, 1e-30,
              -1e-30, 1e-40, -1e-40, 65504.0, -65504.0, 65519.996, -65519.996, 65520.0, -65520.0, 1e6, -1e6, math.inf, -math.inf, math.nan, 1.0, -2.5]


@pytest.mark.parametrize("n", [1000, 2 * GRID + 77])
def test_casts_bit_exact(ops, dev, n):
    """fd_cast_f32_to_f16 / fd_cast_f16_to_f32 (ops.to_f16 / to_f32) against torch's round-to-nearest-even, bit for bit: fp16 subnormals, the
    rounding edge at 65520 (-> inf), +-inf, NaN, the sign of zero (also of values that round to zero), with and without a scale; n not a multiple
    of 256 and, for the second size, beyond one full grid pass.  The library is built with -ffast-math: the casts must stay IEEE (under no-signed-zeros
    the f32 -> f16 cast was once compiled to one fused multiply-convert with a +0 addend and returned +0 for -0 * scale)."""
    x = rnd(n, dev=dev, dtype=torch.float32, seed=n % 1000) * 100
    sp = torch.tensor(_SPECIAL32, dtype=torch.float32, device=dev)
    x[:len(sp)] = sp
    x[-len(sp):] = sp                                        # and in the last grid pass / the last block
    for scale in (1.0, 1024.0, 0.3):
        assert_bit_equal(f"to_f16 n={n} scale={scale}", ops.to_f16(x, scale), (x * scale).half())
    h = x.half()
    sub = torch.tensor([2.0 ** -24, -(2.0 ** -24), 1023 * 2.0 ** -24, 2.0 ** -14, -0.0, 0.0], dtype=torch.float16, device=dev)
    h[:len(sub)] = sub
    h[-len(sub):] = sub
    for scale in (1.0, 1.0 / 1024, -3.0):
        assert_bit_equal(f"to_f32 n={n} scale={scale}", ops.to_f32(h, scale), h.float() * scale)


# ----------------------------------------------------------------------------- finite check
def test_grad_finite_scale_flags_every_bad_value(ops, dev):
    """fd_grad_finite_scale over a buffer beyond one grid pass: a NaN, a -inf, +inf, and a bad value as the LAST element each set the flag;
    the scaled values equal g * scale bit for bit (non-finite ones included).  The flag is OR-only: a finite buffer never clears it."""
    n = 2 * GRID + 5
    base = rnd(n, dev=dev, dtype=torch.float32, seed=3)
    for pos, val in ((n // 2, math.nan), (GRID + 17, -math.inf), (5, math.inf), (n - 1, math.nan), (n - 1, -math.inf), (None, None)):
        g = base.clone()
        if pos is not None:
            g[pos] = val
        ref = g * 0.5
        flag = torch.zeros(1, dtype=torch.int32, device=dev)
        ops.grad_finite_scale(g, 0.5, flag)
        assert int(flag.item()) == (0 if pos is None else 1), (pos, val)
        assert_bit_equal(f"grad_finite_scale bad at {pos}", g, ref)
    flag = torch.ones(1, dtype=torch.int32, device=dev)
    g = base.clone()
    ops.grad_finite_scale(g, 2.0, flag)
    assert int(flag.item()) == 1, "the flag is OR-only: a finite buffer must not clear it"
    assert_bit_equal("grad_finite_scale x2", g, base * 2.0)


# ----------------------------------------------------------------------------- grid-stride elementwise with a tail
def test_elementwise_grid_stride_and_tail(ops, dev):
    """fd_act_fwd / fd_act_bwd / fd_add with n = 4096 x 256 x 8 + 8 x 1001 + 3: a second grid pass over the 8-wide vectors AND the n % 8 tail, which
    block 0 handles after its grid-stride loop.  The tail is also checked on its own.  fd_add with b = NULL (y = sa * a)."""
    n = GRID * 8 + 8 * 1001 + 3
    x = rnd(n, dev=dev, seed=3) * 3
    dy = rnd(n, dev=dev, seed=4)
    tail = slice(n - 11, n)
    for act, fn in [("silu", F.silu), ("relu", F.relu), ("hardswish", F.hardswish), ("hardsigmoid", F.hardsigmoid),
                    ("quick_gelu", lambda t: t * torch.sigmoid(1.702 * t)), ("gelu", F.gelu)]:
        xr = x.float().requires_grad_(True)
        r = fn(xr)
        y = ops.act_fwd(x, act)
        check(f"act {act} n={n}", y, r, 2e-3)
        check(f"act {act} tail", y[tail], r[tail], 2e-3)
        r.backward(dy.float())
        dx = ops.act_bwd(x, dy, act)
        check(f"act_bwd {act} n={n}", dx, xr.grad, 3e-3)
        check(f"act_bwd {act} tail", dx[tail], xr.grad[tail], 3e-3)
    a, b = rnd(n, dev=dev, seed=5), rnd(n, dev=dev, seed=6)
    y = ops.add(a, b, 0.5, -2.0)
    ref = 0.5 * a.float() - 2 * b.float()
    check("add", y, ref, 2e-3)
    check("add tail", y[tail], ref[tail], 2e-3)
    y = ops.add(a, None, -1.5, 3.0)
    check("add b=None", y, -1.5 * a.float(), 2e-3)
    check("add b=None tail", y[tail], -1.5 * a[tail].float(), 2e-3)


# ----------------------------------------------------------------------------- crop-resize at production size
def test_crop_resize_production_size(ops, dev):
    """fd_crop_resize_fwd / _bwd: 512^2 images cropped to 224^2 chips (img_size_small) with boxes spilling over each edge, a box larger than the image
    and an 8 px box (28x upsampling: the widest backward gather window of bilinear_taps), against F.pad + F.interpolate (align_corners=False).
    The backward is a fixed-order gather: bit-reproducible."""
    Hh = Ww = 512
    S = 224
    boxes = torch.tensor([[-40, 100, 200, 340], [350, 200, 560, 410], [100, -30, 300, 170], [150, 400, 350, 600], [-100, -50, 600, 650],
                          [250, 251, 258, 259]], dtype=torch.int32, device=dev)
    B = boxes.shape[0]
    img = (torch.rand(B, 3, Hh, Ww, generator=torch.Generator().manual_seed(11)) * 2 - 1).half().to(dev)
    chips = ops.crop_resize(img, boxes, -1.0, S)
    g = rnd(B, 3, S, S, dev=dev, dtype=torch.float32, seed=14)
    dimg = ops.crop_resize_bwd(g, boxes, B, Hh, Ww, S)
    assert torch.equal(dimg, ops.crop_resize_bwd(g, boxes, B, Hh, Ww, S))
    for i, bb in enumerate(boxes.tolist()):
        im = img[i].float().requires_grad_(True)
        l, r, bt, tp = max(bb[0], 0), min(bb[2], Ww), max(bb[1], 0), min(bb[3], Hh)
        face = F.pad(im[:, bt:tp, l:r], [max(-bb[0], 0), max(bb[2] - Ww, 0), max(-bb[1], 0), max(bb[3] - Hh, 0)], value=-1.0)
        ref = F.interpolate(face[None], size=[S, S], mode="bilinear", align_corners=False)[0]
        check(f"crop_resize 512->224 box {bb}", chips[i], ref, 2e-3)
        ref.backward(g[i])
        check(f"crop_resize bwd box {bb}", dimg[i], im.grad, 1e-4)


# ----------------------------------------------------------------------------- face alignment at production size
def test_warp_affine_production_size(ops, dev):
    """fd_warp_affine_fwd / _bwd: 512^2 images to 112^2 aligned chips through rotated similarity transforms (alignment_sampling_matrix), incl. a
    face partly outside the image and two chips of one image, against oracle.nn_sfnet.image_pipeline and its autograd (bands of
    test_face_alignment_warp_vs_oracle)."""
    from finetune_fair_diffusion_amd.fairness import alignment_sampling_matrix
    from oracle import nn_sfnet as OS
    B, Hh, Ww, crop = 2, 512, 512, 112
    imgs = (torch.rand(B, 3, Hh, Ww, generator=torch.Generator().manual_seed(5)) * 2 - 1).half().float()
    rng = np.random.RandomState(3)

    def face(size, angle, centre):
        p = (OS.SRC_LANDMARKS - 56.0) / 112 * size
        c, s = math.cos(angle), math.sin(angle)
        return p @ np.array([[c, s], [-s, c]]) + np.array(centre) + rng.randn(5, 2) * 0.5

    lms = [face(120, 0.3, (200, 220)), face(260, -0.6, (300, 330)), face(180, 1.2, (470, 60))]      # the last spills over the corner
    src = [0, 0, 1]
    idx = torch.tensor(src, dtype=torch.int32, device=dev)
    x = imgs.clone().requires_grad_(True)
    ref = torch.stack([OS.image_pipeline(x[src[i]], lms[i], crop) for i in range(len(lms))])
    gw = torch.randn(ref.shape, generator=torch.Generator().manual_seed(6))
    (ref * gw).sum().backward()
    A = torch.tensor(np.stack([alignment_sampling_matrix(l, Hh, Ww, crop) for l in lms]), dtype=torch.float32, device=dev)
    chips = ops.warp_affine(imgs.half().to(dev), idx, A, crop)
    check("aligned chips 512->112", chips, ref.detach().to(dev), 2e-3)
    assert float((ref[2] == -1).float().mean()) > 0.05
    dimg = torch.zeros(B, 3, Hh, Ww, dtype=torch.float32, device=dev)
    ops.warp_affine_bwd(gw.to(dev).contiguous(), idx, A, dimg, crop)
    check("d images (warp 512->112)", dimg, x.grad.to(dev), 1e-4)
    d2 = torch.zeros_like(dimg)
    ops.warp_affine_bwd(gw.to(dev).contiguous(), idx, A, d2, crop)
    assert torch.equal(dimg, d2)


# ----------------------------------------------------------------------------- C-ABI entry points without a Python wrapper
@pytest.mark.parametrize("B,H,T,d", [(2, 12, 77, 64), (2, 8, 1024, 40), (16, 8, 8200, 8)])
def test_attn_bwd_prep(ops, dev, B, H, T, d):
    """fd_attn_bwd_prep: D[b, h, t] = sum_c dO * O over the head's d columns (fp32); 16 x 8200 x 8 rows exceed one grid pass."""
    o, do = rnd(B * T, H * d, dev=dev, seed=1), rnd(B * T, H * d, dev=dev, seed=2)
    D = torch.full((B, H, T), float("nan"), dtype=torch.float32, device=dev)
    ops._call("fd_attn_bwd_prep", ops._p(o), ops._p(do), ops._p(D), B, H, T, d, ops._stream())
    ref = (o.double() * do.double()).view(B, T, H, d).sum(-1).permute(0, 2, 1)
    check(f"attn_bwd_prep B{B} H{H} T{T} d{d}", D, ref, 1e-5)


def test_groupnorm_fwd_stats_entry_point(ops, dev):
    """fd_groupnorm_fwd_stats (the image-major form of fd_groupnorm_fwd_stats_p, which ops.groupnorm calls): against torch and bit-equal to ops.groupnorm
    on the same producer statistics."""
    B, HW, C, G, eps = 4, 4096, 320, 32, 1e-5          # a producer shape whose tile has the statistics epilogue
    a, w = rnd(B * HW, 320, dev=dev, seed=1), rnd(C, 320, dev=dev, scale=0.1, seed=2)
    x = ops.gemm(a, w, gn_stats=True)
    assert getattr(x, "gn_stats", None) is not None
    st1, rows1 = x.gn_stats
    gamma = rnd(C, dev=dev, dtype=torch.float32, seed=3) * 0.2 + 1
    beta = rnd(C, dev=dev, dtype=torch.float32, seed=4) * 0.2
    y = torch.empty_like(x)
    mr = torch.empty((B, G, 2), dtype=torch.float32, device=dev)
    ops._call("fd_groupnorm_fwd_stats", ops._p(x), C, None, 0, B, HW, G, eps, ops._p(gamma), ops._p(beta), 1, ops._p(y), ops._p(mr), ops._p(st1), rows1,
              None, 0, ops._stream())
    ref = F.silu(F.group_norm(x.float().view(B, HW, C).permute(0, 2, 1), G, gamma, beta, eps))
    check("groupnorm_fwd_stats", y.view(B, HW, C).permute(0, 2, 1), ref, 2e-3)
    y2, st2 = ops.groupnorm(x, None, B, HW, G, eps, gamma, beta, True)
    assert torch.equal(y, y2) and torch.equal(mr, st2)
