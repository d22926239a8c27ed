"""LoRA weight gradients at ranks 17..64 (GPU, fp16 library): the batched MFMA arm of fd_lora_wgrad_multi (csrc/lora.hip, padded ranks 32 and 64) against
the fp64 product under band B1 of tests/kernel_bands.py (tests/wgrad_rank_cases.py states the band and builds the problems), and against the untouched
single-problem fd_lora_wgrad.  Every test prints its figures before it asserts."""
import ctypes

import pytest
import torch

import wgrad_rank_cases as W

pytestmark = pytest.mark.gpu
H16 = torch.float16


@pytest.fixture(scope="module")
def ops():
    from finetune_fair_diffusion_amd import ops
    assert ops.F16 == H16, "this file checks the fp16 library (tests/run_bf16_wgrad_rank_checks.py is its bf16 counterpart)"
    return ops


def _names(calls):
    return [c for c in calls if c.startswith("fd_lora_wgrad")]


@pytest.mark.parametrize("R", [17, 32, 50, 64])
def test_batched_mixed_problems(ops, dev, R):
    """Case 1: six problems of mixed M / N and both output layouts, X a column slice, G pre-filled with ones, in ONE fd_lora_wgrad_multi call."""
    probs = W.mixed(dev, H16, R)
    with W.counted(ops) as calls:
        outs = W.run(ops, probs)
    assert _names(calls) == ["fd_lora_wgrad_multi"], f"one batched call and no single-problem call expected, got {_names(calls)}"
    for p, G in zip(probs, outs):
        W.band("batched", p, G, 1.0, H16)


def _unet_views(dev, M, C=320, R=50):
    """The six problems of unet.py's self-attention LoRA backward: d up = dqkv[:, iC:(i+1)C]^T t1[:, 64i:64(i+1)] and d down = u[:, 64i:64(i+1)]^T n1."""
    rp = W.rp_of(R)
    dqkv, n1 = W.rnd(M, 3 * C, dev=dev, seed=1, dtype=H16), W.rnd(M, C, dev=dev, seed=2, dtype=H16)
    t1, u = torch.zeros(M, 3 * rp, dtype=H16, device=dev), torch.zeros(M, 3 * rp, dtype=H16, device=dev)
    for i in range(3):
        t1[:, i * rp:i * rp + R] = W.rnd(M, R, dev=dev, seed=3 + i, dtype=H16)
        u[:, i * rp:i * rp + R] = W.rnd(M, R, dev=dev, seed=6 + i, dtype=H16)
    out = []
    for i in range(3):
        out.append((dqkv[:, i * C:(i + 1) * C], t1[:, i * rp:(i + 1) * rp], False))     # gu [N, r]: strides (r, 1)
        out.append((n1, u[:, i * rp:(i + 1) * rp], True))                               # gd [r, K]: strides (1, K)
    return out


@pytest.mark.parametrize("M", [128, 4096])
def test_unet_operand_views_rank_50(ops, dev, M):
    """Case 2: the U-Net's own views (ldx = 3C, ldt = 192) are queued and meet the band."""
    R, C = 50, 320
    views = _unet_views(dev, M)
    outs = [torch.zeros((R, C) if trans else (C, R), dtype=torch.float32, device=dev) for _, _, trans in views]
    with W.counted(ops) as calls:
        with ops.wgrad_batch():
            for (X, T, trans), G in zip(views, outs):
                assert X.stride(0) == (C if trans else 3 * C) and T.stride(0) == 192
                ops.lora_wgrad(X, T, G, *((1, C) if trans else (R, 1)), R, scale=W.SCALE)
    assert _names(calls) == ["fd_lora_wgrad_multi"], _names(calls)
    for i, ((X, T, trans), G) in enumerate(zip(views, outs)):
        p = W.Problem.__new__(W.Problem)
        p.M, p.N, p.R, p.trans = M, C, R, trans
        p.ref = W.SCALE * X.double().t() @ T[:, :R].double()
        p.S = W.SCALE * X.double().abs().t() @ T[:, :R].double().abs()
        W.band(f"unet view {i}", p, G, 0.0, H16)


def test_production_shape(ops, dev):
    """Case 2, the 64 x 64 level: M = 65536, N = 320, R = 50 (42 MB of X)."""
    p = W.Problem(65536, 320, 50, False, dev, H16, seed=77, extra=64)
    with W.counted(ops) as calls:
        (G,) = W.run(ops, [p])
    assert _names(calls) == ["fd_lora_wgrad_multi"], _names(calls)
    W.band("production", p, G, 1.0, H16)


def test_pad_columns_and_output_window(ops, dev):
    """Case 3: T's pad columns R .. RP - 1 hold 1000.0: outputs are bit-equal to the run with zero pads; an [R, N] output embedded in a larger buffer of
    a finite sentinel has nothing outside its R x N window touched."""
    R = 50
    probs = W.mixed(dev, H16, R)
    clean = W.run(ops, probs)
    dirty = W.run(ops, [p.with_pad(1000.0) for p in probs])
    for p, a, b in zip(probs, clean, dirty):
        W.band("pads 1000", p, b, 1.0, H16)
        assert torch.equal(a, b), f"{p.M}x{p.N}: pad columns of T reached the result ({int((a != b).sum())} elements differ)"
    p = probs[1]                                                     # (2048, 640, [R, N])
    SENT = 12345.0
    buf = torch.full((R + 6, p.N + 24), SENT, dtype=torch.float32, device=dev)
    win = buf[3:3 + R, 8:8 + p.N]
    win.zero_()
    with ops.wgrad_batch():
        ops.lora_wgrad(p.X, p.T, win, 1, buf.stride(0), R, scale=W.SCALE)
    W.band("embedded window", p, win, 0.0, H16)
    outside = torch.ones_like(buf, dtype=torch.bool)
    outside[3:3 + R, 8:8 + p.N] = False
    assert bool((buf[outside] == SENT).all()), "an element outside the R x N window of G was written"


def test_full_batch_of_16(ops, dev):
    """Case 4: 16 problems at N = 1280, M = 300, R = 64 go out in one call with the scratch ``ops`` passes."""
    probs = [W.Problem(300, 1280, 64, bool(i & 1), dev, H16, seed=500 + i) for i in range(16)]
    with W.counted(ops) as calls:
        outs = W.run(ops, probs)
    assert _names(calls) == ["fd_lora_wgrad_multi"], _names(calls)
    for p, G in zip(probs, outs):
        W.band("full batch", p, G, 1.0, H16)


def test_mixed_ranks_in_one_context(ops, dev):
    """Case 5: ranks 4, 12, 24 and 50 interleaved in one context: one call per padded rank, every problem in its band."""
    probs = [W.Problem(M, N, R, trans, dev, H16, seed=700 + i)
             for i, (M, N, R, trans) in enumerate([(500, 320, 4, False), (300, 640, 12, True), (260, 320, 24, False), (700, 640, 50, True),
                                                   (90, 640, 4, True), (1000, 320, 50, False), (333, 328, 24, True), (64, 320, 12, False)])]
    with W.counted(ops) as calls:
        outs = W.run(ops, probs)
    assert _names(calls) == ["fd_lora_wgrad_multi"] * 4, _names(calls)
    for p, G in zip(probs, outs):
        W.band("mixed ranks", p, G, 1.0, H16)


def test_deterministic_also_beside_another_stream(ops, dev):
    """Case 6: the mixed batch at R = 50 twice gives equal bits; also when the second run is issued on a second stream while a large GEMM runs on the first."""
    probs = W.mixed(dev, H16, 50)
    first = W.run(ops, probs)
    second = W.run(ops, probs)
    a, b = W.rnd(8192, 4096, dev=dev, seed=5, dtype=H16), W.rnd(4096, 4096, dev=dev, seed=6, dtype=H16)
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    ops.gemm(a, b)
    with torch.cuda.stream(side):
        third = W.run(ops, probs)
    torch.cuda.synchronize()
    for p, x, y, z in zip(probs, first, second, third):
        assert torch.equal(x, y), f"{p.M}x{p.N}: two runs differ in {int((x != y).sum())} elements"
        assert torch.equal(x, z), f"{p.M}x{p.N}: the run beside a GEMM on another stream differs in {int((x != z).sum())} elements"


@pytest.mark.parametrize("R", [17, 32, 50, 64])
def test_single_path_meets_the_same_band(ops, dev, R):
    """Case 7: the same problems one by one through the untouched fd_lora_wgrad (the independent second implementation)."""
    probs = W.mixed(dev, H16, R)
    with W.counted(ops) as calls:
        outs = W.run(ops, probs, batched=False)
    assert _names(calls) == ["fd_lora_wgrad"] * len(probs), _names(calls)
    for p, G in zip(probs, outs):
        W.band("single", p, G, 1.0, H16)


@pytest.mark.parametrize("N,extra", [(320, 68), (324, 64)], ids=["ldx % 8 == 4", "N % 8 == 4"])
def test_unaligned_problem_takes_the_single_path(ops, dev, N, extra):
    """Case 8: what the MFMA arm cannot take is not queued; the single path computes it."""
    p = W.Problem(1000, N, 50, False, dev, H16, seed=900 + N, extra=extra)
    assert p.X.stride(0) % 8 == 4 or N % 8 == 4
    with W.counted(ops) as calls:
        (G,) = W.run(ops, [p])
    assert _names(calls) == ["fd_lora_wgrad"], _names(calls)
    W.band("unaligned", p, G, 1.0, H16)


def _descs(ops, probs, outs):
    from finetune_fair_diffusion_amd import lib
    arr = lib.WgradDesc.array(len(probs))
    for d, p, G in zip(arr, probs, outs):
        d.X, d.ldx, d.T, d.ldt, d.G = p.X.data_ptr(), p.X.stride(0), p.T.data_ptr(), p.T.stride(0), G.data_ptr()
        (d.g_stride_n, d.g_stride_r), d.M, d.N, d.R, d.scale = p.strides(), p.M, p.N, p.R, W.SCALE
    return arr


def test_host_side_refusals(ops, dev):
    """Case 8: rank 65, mixed padded ranks and a misaligned operand are refused on the host, by name; G is untouched."""
    sc = ops.scratch(1 << 22, dev)
    stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    a, b = W.Problem(100, 320, 50, False, dev, H16, seed=1), W.Problem(100, 320, 24, False, dev, H16, seed=2)
    for probs, fix, match in [([a], lambda arr: setattr(arr[0], "R", 65), "rank must be in 1..64"),
                              ([a, b], lambda arr: None, "mixed padded ranks"),
                              ([a], lambda arr: setattr(arr[0], "ldx", a.X.stride(0) + 4), "ldx"),
                              ([a], lambda arr: setattr(arr[0], "N", 316), "N must be"),
                              ([a], lambda arr: setattr(arr[0], "ldt", 56), "ldt"),
                              ([a], lambda arr: setattr(arr[0], "X", a.X.data_ptr() + 2), "X must be 16-byte aligned"),
                              ([a], lambda arr: setattr(arr[0], "T", a.T.data_ptr() + 8), "T must be 16-byte aligned")]:
        outs = [p.out(1.0) for p in probs]
        arr = _descs(ops, probs, outs)
        fix(arr)
        with pytest.raises(RuntimeError, match=match):
            ops._call("fd_lora_wgrad_multi", ctypes.byref(arr), len(probs), ctypes.c_void_p(sc.data_ptr()), sc.numel(), stream)
        torch.cuda.synchronize()
        assert all(bool((G == 1.0).all()) for G in outs), f"'{match}': something was launched"
