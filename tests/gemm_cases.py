"""One case table for the fd_gemm kernel family (data and a descriptor builder only: no GPU use, no library import).

Every kernel symbol that the product library's dispatcher (csrc/gemm.hip: gemm_tile, gemm_plan, pp_takes; gemm_halo.hip: fd_conv_halo_eligible) can select is
named by at least one case below, at the smallest M its thresholds admit -- which leaves a one-row tail in the last tile -- with K, second-slab and N tails
where the kernel allows them.  tests/test_kernel_coverage_cpu.py asserts that against the symbols of the built library and asserts every expected name,
split factor and statistics chunk height against the host-only queries, so a policy change moves a case visibly; tests/test_kernels_sharp_gpu.py runs every
case under gate B of tests/kernel_bands.py.  Symbols no case names are listed in UNREACHED with the reason the product build cannot select them.

How the thresholds give the shapes (gemm_tile, product defaults t256 = 100, t128 = 80, t160 = 160, tvae = 200, split-K up to 8):
  256x320: ceil(M/256) * N/320 >= 100 -> N = 1280: M >= 24*256 + 1 = 6145;  N = 2560: 3073 (K + K2 <= 384 there goes to the ping-pong kernel)
  128x320: ceil(M/128) * N/320 >= 80  -> N = 1280: M >= 2433;  split-K form: >= 64 k-tiles of 64 and ceil(M/128) * N/320 >= 32 -> M >= 897
  128x160: ceil(M/128) * N/160 >= 160 -> N = 1440: M >= 2177;  256x256: ceil(M/256) * N/256 >= 200 -> N = 2048: 6145
  256x128: ceil(M/256) * N/128 >= 200 -> N = 2176: M >= 2817;  512x128: N == 128 and ceil(M/512) >= 400 -> M >= 204289 (the floor, not a choice)
  128x128 / 128x64 (gemm_glds): >= 512 tiles -> N = 1224: M >= 6529;  N = 320: M >= 13057.  The four phases of the up-sampling pair count four times.
  halo kernels: square 16^2 / 32^2 / 64^2 maps, whole tiles per image: the batch sizes below are the smallest that reach each tile height.
"""
from collections import namedtuple

# conv modes (include/fairdiff_hip.h)
NORMAL, STRIDE2, UP2, TRANS2, UP2P, UP2P_BWD, UP2PI = range(7)
TAPS = {NORMAL: 9, STRIDE2: 9, UP2: 9, TRANS2: 9, UP2P: 4, UP2P_BWD: 16, UP2PI: 4}
ACT = dict(none=0, silu=1, quick_gelu=2, gelu=3, relu=4, hardswish=5, hardsigmoid=6, geglu=7)

# family: "dense" | "skinny" | "conv" (3x3 gathers, modes 0-3) | "up2p" (phase problems, modes 4-6)
# conv: (Bn, H, W, Cin, mode) with H, W the INPUT map of the launch (FD_CONV_UP2P_BWD: the high-resolution gradient), else None
# operands: letters of the epilogue operands -- b fp32 bias, r 16-bit row bias (one row per image / for the whole launch), R 16-bit residual.  A case with R
#     runs with and without it.
# act: the epilogue activation (a key of ACT).  "geglu": B and the bias interleaved (value_c, gate_c), C [M, N / 2] = value * gelu(gate) of the two halves
#     ROUNDED to the working dtype first (bit-identical to the projection followed by fd_geglu_fwd), the pre-gate projection [M, N] as a second output
# colscale: (factor, columns) or None; alpha: the accumulator's factor; out: "f16" (the working dtype) or "f32"
# kernel / split / stats_rows: what fd_gemm_kernel_name and fd_gemm_stats_rows must answer (split 0 = no split-K)
# roundings: roundings to the working dtype between the fp32 accumulator and the stored value WITH the residual (without it: always one; fp32 output: none)
Case = namedtuple("Case", "id family M N K K2 conv operands gn_stats colscale act alpha out kernel split roundings")


def _out_hw(H, W, mode):
    if mode in (NORMAL, UP2P, UP2PI):
        return H, W
    if mode == STRIDE2:
        return (H + 1) // 2, (W + 1) // 2
    if mode == UP2P_BWD:
        return H // 2, W // 2
    return 2 * H, 2 * W


def lds_epilogue(c):
    """FD_GEMM_LDS_EPILOGUE_OK (csrc/gemm_device.h) for the contiguous operands the tests pass: 16-bit output, N % 8 == 0 (ldc = ldr = ld_rowbias = N)."""
    return c.out == "f16" and c.N % 8 == 0


def expected_roundings(c, residual=True):
    """The rule behind Case.roundings: two for a 16-bit output with a residual that goes through the LDS-staged epilogue (gemm_epilogue_lds parks
    act(acc + bias + rowbias) in LDS in the working dtype and adds the residual on the way out); one for split-K (splitk_reduce_kernel sums in fp32 and
    rounds once), the skinny kernel (no epilogue operands), the plain epilogue (N % 8 != 0) and every launch without a residual; fp32 output rounds to fp32 only.
    This restates the source of the epilogues (csrc/gemm_device.h); the library has no query for it, so it selects a band and is not an independent check."""
    if c.out == "f32":
        return 0
    staged = c.family != "skinny" and c.split == 0 and lds_epilogue(c)
    return 2 if (residual and "R" in c.operands and staged) else 1


def _case(id, family, M, N, K, kernel, K2=0, conv=None, operands="", gn_stats=False, colscale=None, act="none", alpha=1.0, out="f16", split=0, roundings=None):
    assert act in ACT
    c = Case(id, family, M, N, K, K2, conv, operands, gn_stats, colscale, act, alpha, out, kernel, split, 0)
    return c._replace(roundings=expected_roundings(c) if roundings is None else roundings)


def dense(id, M, N, K, kernel, K2=8, operands="bR", **kw):
    return _case(id, "dense", M, N, K, kernel, K2=K2, operands=operands, **kw)


def skinny(id, M, N, K, kernel):
    return _case(id, "skinny", M, N, K, kernel)


def conv(id, Bn, H, W, Cin, Cout, mode, kernel, operands=None, **kw):
    Ho, Wo = _out_hw(H, W, mode)
    family = "up2p" if mode >= UP2P else "conv"
    if operands is None:        # fd_gemm: the phase problems take a bias-only epilogue
        operands = {"conv": "brR", "up2p": "" if mode == UP2P_BWD else "b"}[family]
    return _case(id, family, Bn * Ho * Wo, Cout, TAPS[mode] * Cin, kernel, conv=(Bn, H, W, Cin, mode), operands=operands, **kw)


BIG, PP, HALO, GLDS, SK = "gemm_big_kernel", "gemm_pp_kernel", "conv_halo_kernel", "gemm_glds_kernel", "gemm_skinny_kernel"

CASES = [
    # ---- gemm_glds (BK = 32; the LDS-staged epilogue where N % 8 == 0, the plain one elsewhere)
    dense("glds64", 130, 200, 72, f"{GLDS}<64, 64, false>"),
    dense("glds64 plain epilogue (N % 8 = 4)", 130, 204, 72, f"{GLDS}<64, 64, false>"),
    dense("glds64 K=40 (the attention head dim)", 65, 1280, 40, f"{GLDS}<64, 64, false>"),
    dense("glds64 f32 out", 130, 200, 72, f"{GLDS}<64, 64, false>", out="f32"),
    dense("glds64 alpha + rowbias", 130, 200, 72, f"{GLDS}<64, 64, false>", operands="brR", alpha=0.5),
    dense("glds64 silu + rowbias", 130, 200, 72, f"{GLDS}<64, 64, false>", operands="brR", act="silu"),
    dense("glds128x64", 13057, 320, 72, f"{GLDS}<128, 64, false>"),
    dense("glds128x128", 6529, 1224, 72, f"{GLDS}<128, 128, false>"),
    conv("conv glds64 normal", 1, 9, 9, 32, 40, NORMAL, f"{GLDS}<64, 64, true>"),
    conv("conv glds64 stride2 (odd map)", 2, 9, 11, 32, 40, STRIDE2, f"{GLDS}<64, 64, true>"),
    conv("conv glds64 up2", 1, 9, 9, 32, 40, UP2, f"{GLDS}<64, 64, true>"),
    conv("conv glds64 trans2", 1, 9, 9, 32, 40, TRANS2, f"{GLDS}<64, 64, true>"),
    conv("conv glds128x64", 1, 115, 115, 32, 320, NORMAL, f"{GLDS}<128, 64, true>"),
    conv("conv glds128x128", 1, 81, 81, 32, 1224, NORMAL, f"{GLDS}<128, 128, true>"),
    # ---- lockstep big tiles, dense (BK = 64: K = 328 leaves a k-tail, K2 = 8 a slab tail)
    dense("big256x320", 6145, 1280, 328, f"{BIG}<256, 320, 4, 4, 0>"),
    dense("big256x320 colscale", 6145, 1280, 328, f"{BIG}<256, 320, 4, 4, 0>", colscale=(0.2280966, 640)),
    dense("big256x320 silu + rowbias", 6145, 1280, 328, f"{BIG}<256, 320, 4, 4, 0>", operands="brR", act="silu"),
    dense("big256x320 fused geglu", 6145, 1280, 328, f"{BIG}<256, 320, 4, 4, 0>", K2=0, operands="b", act="geglu"),
    dense("big256x320 stats", 6145, 1280, 328, f"{BIG}<256, 320, 4, 4, 3>", gn_stats=True),
    dense("big128x320", 2433, 1280, 328, f"{BIG}<128, 320, 4, 4, 0>"),
    dense("big128x320 gelu", 2433, 1280, 328, f"{BIG}<128, 320, 4, 4, 0>", act="gelu"),
    dense("big128x320 stats", 2433, 1280, 328, f"{BIG}<128, 320, 4, 4, 3>", gn_stats=True),
    dense("big128x160", 2177, 1440, 328, f"{BIG}<128, 160, 4, 2, 0>"),
    dense("big128x160 stats", 2177, 1440, 328, f"{BIG}<128, 160, 4, 2, 3>", gn_stats=True),
    dense("big256x256", 6145, 2048, 328, f"{BIG}<256, 256, 2, 4, 0>"),
    dense("big256x128", 2817, 2176, 328, f"{BIG}<256, 128, 4, 2, 0>"),
    dense("big512x128", 204289, 128, 328, f"{BIG}<512, 128, 8, 2, 0>"),
    dense("split-K 128x320", 897, 1280, 4104, f"{BIG}<128, 320, 4, 4, 0>", split=8),
    dense("split-K 128x160", 300, 320, 2056, f"{BIG}<128, 160, 4, 2, 0>", split=4),
    # ---- ping-pong, dense: the FF1 projections (K + K2 <= 384, N >= 2560)
    dense("pp256 dense", 3073, 2560, 320, f"{PP}<256, 0, true>"),
    dense("pp256 dense K tail", 3073, 2560, 328, f"{PP}<256, 0, true>", K2=0),
    dense("pp256 dense quick_gelu + rowbias", 3073, 2560, 320, f"{PP}<256, 0, true>", operands="brR", act="quick_gelu"),
    dense("pp256 dense fused geglu (FF1)", 3073, 2560, 320, f"{PP}<256, 0, true>", K2=0, operands="b", act="geglu"),
    dense("pp256 dense stats", 3073, 2560, 320, f"{PP}<256, 2, true>", gn_stats=True),
    # ---- skinny (LoRA down-projections: N = rank padded to 8, or three stacked ranks): NT = ceil(N / 16), KS = 1 / 2 / 4 at K >= 320 / 640 / 1280
    skinny("skinny N12 K320", 1030, 12, 320, f"{SK}<1, 1, 1>"), skinny("skinny N20 K320", 1030, 20, 320, f"{SK}<2, 1, 1>"),
    skinny("skinny N44 K320", 1030, 44, 320, f"{SK}<3, 1, 1>"), skinny("skinny N60 K320", 1030, 60, 320, f"{SK}<4, 1, 1>"),
    skinny("skinny N8 K640", 1030, 8, 640, f"{SK}<1, 2, 1>"), skinny("skinny N24 K640", 1030, 24, 640, f"{SK}<2, 2, 1>"),
    skinny("skinny N40 K640", 1030, 40, 640, f"{SK}<3, 2, 1>"), skinny("skinny N56 K640", 1030, 56, 640, f"{SK}<4, 2, 1>"),
    skinny("skinny N8 K1280 (rank-4 LoRA at 1280 channels)", 1030, 8, 1280, f"{SK}<1, 4, 1>"), skinny("skinny N24 K1280", 1030, 24, 1280, f"{SK}<2, 4, 1>"),
    skinny("skinny N44 K1280", 1030, 44, 1280, f"{SK}<3, 4, 1>"), skinny("skinny N60 K1280", 1030, 60, 1280, f"{SK}<4, 4, 1>"),
    # ---- lockstep big tiles, 3x3 gathers (Cin % 64 == 0).  Stride-1 convolutions on the 320-wide tiles belong to the ping-pong / halo kernels, so the
    #      lockstep 320-wide tiles see the other modes; the 8-wave 256x320 form is theirs alone (gemm_plan: 16 waves for dense only)
    conv("conv big256x320 stride2 (odd map)", 1, 157, 157, 64, 1280, STRIDE2, f"{BIG}<256, 320, 2, 4, 1>"),
    conv("conv big256x320 stride2 stats", 1, 157, 157, 64, 1280, STRIDE2, f"{BIG}<256, 320, 2, 4, 4>", gn_stats=True),
    conv("conv big128x320 trans2", 1, 25, 25, 64, 1280, TRANS2, f"{BIG}<128, 320, 4, 4, 1>"),
    conv("conv big128x320 stride2 stats", 1, 99, 99, 64, 1280, STRIDE2, f"{BIG}<128, 320, 4, 4, 4>", gn_stats=True),
    conv("conv big128x160 normal", 1, 47, 47, 64, 1440, NORMAL, f"{BIG}<128, 160, 4, 2, 1>"),
    conv("conv big128x160 normal stats", 1, 47, 47, 64, 1440, NORMAL, f"{BIG}<128, 160, 4, 2, 4>", gn_stats=True),
    conv("conv big256x256 up2", 1, 40, 40, 64, 2048, UP2, f"{BIG}<256, 256, 2, 4, 1>"),
    conv("conv big256x128 trans2", 1, 27, 27, 64, 2176, TRANS2, f"{BIG}<256, 128, 4, 2, 1>"),
    conv("conv big512x128 normal", 1, 452, 452, 64, 128, NORMAL, f"{BIG}<512, 128, 8, 2, 1>"),
    conv("conv split-K 8x8 1280->1280", 3, 8, 8, 1280, 1280, NORMAL, f"{BIG}<128, 160, 4, 2, 1>", split=8),
    # ---- the up-sampling phase pairs (big tiles only; four phase problems per launch)
    conv("up2p interleaved 256x320", 1, 40, 40, 64, 1280, UP2PI, f"{BIG}<256, 320, 2, 4, 2>"),
    conv("up2p interleaved 256x320 stats", 1, 40, 40, 64, 1280, UP2PI, f"{BIG}<256, 320, 2, 4, 6>", gn_stats=True),
    conv("up2p backward 128x320", 1, 100, 100, 64, 1280, UP2P_BWD, f"{BIG}<128, 320, 4, 4, 2>"),
    conv("up2p interleaved 128x320 stats", 1, 24, 24, 64, 1280, UP2PI, f"{BIG}<128, 320, 4, 4, 6>", gn_stats=True),
    conv("up2p phase-major 128x160", 1, 24, 24, 64, 1440, UP2P, f"{BIG}<128, 160, 4, 2, 2>"),
    conv("up2p interleaved 128x160 stats", 1, 24, 24, 64, 1440, UP2PI, f"{BIG}<128, 160, 4, 2, 6>", gn_stats=True),
    conv("up2p interleaved 256x256", 1, 40, 40, 64, 2048, UP2PI, f"{BIG}<256, 256, 2, 4, 2>"),
    conv("up2p phase-major 256x128", 1, 24, 24, 64, 2176, UP2P, f"{BIG}<256, 128, 4, 2, 2>"),
    conv("up2p interleaved 512x128", 1, 452, 452, 64, 128, UP2PI, f"{BIG}<512, 128, 8, 2, 2>"),
    # ---- ping-pong, stride-1 3x3 gathers the halo kernel does not take (maps that are not 16^2 / 32^2 / 64^2)
    conv("conv pp256", 1, 79, 79, 64, 1280, NORMAL, f"{PP}<256, 1, true>"),
    conv("conv pp256 silu", 1, 79, 79, 64, 1280, NORMAL, f"{PP}<256, 1, true>", act="silu"),
    conv("conv pp256 stats", 1, 79, 79, 64, 1280, NORMAL, f"{PP}<256, 3, true>", gn_stats=True),
    conv("conv pp128", 1, 50, 50, 64, 1280, NORMAL, f"{PP}<128, 1, true>"),
    conv("conv pp128 stats", 1, 50, 50, 64, 1280, NORMAL, f"{PP}<128, 3, true>", gn_stats=True),
    # ---- halo-staged stride-1 3x3 convolutions: the six geometries, each with and without the statistics epilogue
    conv("halo 256 64^2", 2, 64, 64, 64, 1280, NORMAL, f"{HALO}<256, 64, 1, true>"),
    conv("halo 256 64^2 stats", 2, 64, 64, 64, 1280, NORMAL, f"{HALO}<256, 64, 3, true>", gn_stats=True),
    conv("halo 128 64^2", 1, 64, 64, 64, 1280, NORMAL, f"{HALO}<128, 64, 1, true>"),
    conv("halo 128 64^2 silu", 1, 64, 64, 64, 1280, NORMAL, f"{HALO}<128, 64, 1, true>", act="silu"),
    conv("halo 128 64^2 stats", 1, 64, 64, 64, 1280, NORMAL, f"{HALO}<128, 64, 3, true>", gn_stats=True),
    conv("halo 256 32^2", 7, 32, 32, 64, 1280, NORMAL, f"{HALO}<256, 32, 1, true>"),
    conv("halo 256 32^2 stats", 7, 32, 32, 64, 1280, NORMAL, f"{HALO}<256, 32, 3, true>", gn_stats=True),
    conv("halo 128 32^2", 3, 32, 32, 64, 1280, NORMAL, f"{HALO}<128, 32, 1, true>"),
    conv("halo 128 32^2 stats", 3, 32, 32, 64, 1280, NORMAL, f"{HALO}<128, 32, 3, true>", gn_stats=True),
    conv("halo 256 16^2", 25, 16, 16, 64, 1280, NORMAL, f"{HALO}<256, 16, 1, true>"),
    conv("halo 256 16^2 stats", 25, 16, 16, 64, 1280, NORMAL, f"{HALO}<256, 16, 3, true>", gn_stats=True),
    conv("halo 128 16^2", 10, 16, 16, 64, 1280, NORMAL, f"{HALO}<128, 16, 1, true>"),
    conv("halo 128 16^2 stats", 10, 16, 16, 64, 1280, NORMAL, f"{HALO}<128, 16, 3, true>", gn_stats=True),
]
BY_ID = {c.id: c for c in CASES}
assert len(BY_ID) == len(CASES), "case ids are unique"

# K + K2 of every case: the K at which tests/test_fp16_bands_cpu.py measures the B2 margin
KS = tuple(sorted({c.K + c.K2 for c in CASES}))

WORKSPACE_BYTES = 64 << 20          # ops.gemm_workspace(): split-K factors depend on it
_FAKE = 0x10000                     # a non-null operand address: the host-only queries never dereference


def descriptor(c, GemmDesc, residual=True, pointers=None):
    """The fd_gemm_desc of a case for contiguous operands (what fd_gemm_tile / fd_gemm_kernel_name / fd_gemm_stats_rows decide on).
    ``GemmDesc``: finetune_fair_diffusion_amd.lib.GemmDesc; ``pointers``: {field: address} of real operands, else placeholders."""
    p = (lambda name: (pointers or {}).get(name, _FAKE))
    d = GemmDesc()
    d.A, d.B, d.C = p("A"), p("B"), p("C")
    d.M, d.N, d.K, d.K2, d.lda, d.ldb, d.ldc, d.alpha, d.batch = c.M, c.N, c.K, c.K2, c.K, c.K, (c.N // 2 if c.act == "geglu" else c.N), c.alpha, 1
    d.act = ACT[c.act]
    if c.K2:
        d.A2, d.B2, d.lda2, d.ldb2 = p("A2"), p("B2"), c.K2, c.K2
    if "b" in c.operands:
        d.bias = p("bias")
    if "r" in c.operands:
        d.rowbias, d.ld_rowbias = p("rowbias"), c.N
        d.rows_per_batch = c.M // c.conv[0] if c.conv else c.M
    if "R" in c.operands and residual:
        d.residual, d.ldr = p("residual"), c.N
    d.out_dtype = 1 if c.out == "f32" else 0
    if c.gn_stats:
        d.gn_stats = p("gn_stats")
    if c.colscale:
        d.colscale, d.colscale_cols = c.colscale
    d.workspace, d.workspace_bytes = p("workspace"), WORKSPACE_BYTES
    if c.conv:
        Bn, H, W, Cin, mode = c.conv
        Ho, Wo = _out_hw(H, W, mode)
        d.conv, d.conv_mode, d.Bn, d.H, d.W, d.Cin, d.Ho, d.Wo, d.lda = 1, mode, Bn, H, W, Cin, Ho, Wo, Cin
    return d


# ---- kernel symbols of the shipped fp16 library that no case names, each with the reason the PRODUCT build cannot select it.  The reasons are keys of
# REASONS; tests/test_kernel_coverage_cpu.py checks them against the built library and the source.  A symbol the product build can reach may not be listed here.
REASONS = {
    "skinny_rt2": "two row tiles per wave (RT = 2): selected only through the FD_GEMM_SKINNY_RT bench_env switch of the measurement build",
    "w8": "8-wave (wgm = 2) form of a dense / 128x320 tile: selected only through the FD_GEMM_W8 bench_env switch of the measurement build",
    "conv_16_waves": "16-wave (wgm = 4) 256x320 tile with a 3x3 gather or phase pair: gemm_plan gives 16 waves to dense problems only (its conv form is the 8-wave one)",
    "pp_no_prio": "ping-pong kernel without s_setprio: policy bit 4 is set in the built policy (fd_gemm_kernel_name prints it), and only FD_GEMM_PP -- a getenv compiled "
                  "under FD_BENCH_HOOKS alone -- changes the policy at run time",
    "pp128_dense": "dense GEMMs on the 128x320 ping-pong tile: policy bit 16 is not set in the built policy (measured within +-3 % of the lockstep tile)",
}
UNREACHED = {}
for _nt in (1, 2, 3, 4):
    for _ks in (1, 2, 4):
        UNREACHED[f"{SK}<{_nt}, {_ks}, 2>"] = "skinny_rt2"
for _cv in (0, 1, 2, 3, 4, 6):
    UNREACHED[f"{BIG}<128, 320, 2, 4, {_cv}>"] = "w8"
for _cv in (0, 3):
    UNREACHED[f"{BIG}<256, 320, 2, 4, {_cv}>"] = "w8"
for _cv in (1, 2, 4, 6):
    UNREACHED[f"{BIG}<256, 320, 4, 4, {_cv}>"] = "conv_16_waves"
for _bm in (256, 128):
    for _cv in (0, 1, 2, 3):
        UNREACHED[f"{PP}<{_bm}, {_cv}, false>"] = "pp_no_prio"
for _cv in (0, 2):
    UNREACHED[f"{PP}<128, {_cv}, true>"] = "pp128_dense"
