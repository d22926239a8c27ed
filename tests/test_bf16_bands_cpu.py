"""The bands of tests/run_bf16_kernel_checks.py, without a GPU: gate B passes the fp32-accumulate emulation of a bf16 GEMM (torch's fp32 matmul of the
bf16 operands + second slab + bias + residual, rounded once to bf16) at every GEMM-family K of the script, and fails each planted error -- a dropped
k-term in one row, one column scaled by 1 + 2^-7, two adjacent columns swapped in one 16-row block, one element off by 2 ulp.  At K = 4104 the derived
elementwise band B1 is several ulp wide and the dropped term must be caught by the RMS gate B2."""
import pytest
import torch

import run_bf16_kernel_checks as K

BF = torch.bfloat16
KS = (40, 64, 288, 320, 336, 576, 640, 1024, 1280, 2880, 4104, 5120, 11520)      # K + K2 of every fd_gemm problem of the script (9 * Cin for convolutions)


def problem(M, N, Kd, K2, seed=0):
    """bf16 operands, the fp32-accumulate emulation (fp32), the fp64 reference, S and T."""
    g = torch.Generator().manual_seed(seed + Kd)
    r = lambda *s, scale=1.0: (torch.randn(*s, generator=g) * scale).to(BF)
    a, b, res = r(M, Kd), r(N, Kd, scale=0.1), r(M, N)
    a2, b2 = (r(M, K2), r(N, K2)) if K2 else (torch.zeros(M, 0, dtype=BF), torch.zeros(N, 0, dtype=BF))
    bias = torch.randn(N, generator=g)
    acc = lambda a_: a_.float() @ b.float().t() + a2.float() @ b2.float().t() + bias + res.float()
    ref = a.double() @ b.double().t() + a2.double() @ b2.double().t() + bias.double() + res.double()
    S = a.double().abs() @ b.double().abs().t() + a2.double().abs() @ b2.double().abs().t() + bias.double().abs() + res.double().abs()
    return a, b, acc, ref, S, Kd + K2 + 2


def test_ulp_and_yardstick():
    x = torch.tensor([1.0, 1.5, 2.0, 0.75, 3.3895e38, 1.1754944e-38, 1e-40], dtype=torch.float64)
    assert K.ulp_bf16(x).tolist() == [2.0 ** -7, 2.0 ** -7, 2.0 ** -6, 2.0 ** -8, 2.0 ** 120, 2.0 ** -133, 2.0 ** -133]
    ref = torch.randn(64, 64, generator=torch.Generator().manual_seed(1), dtype=torch.float64)
    assert K.gate_c_stat(ref.to(BF), ref, floor=0.0) <= 0.5          # the reference rounded once is the yardstick: half an ulp by construction


def test_gate_b_passes_the_fp32_accumulate_emulation_and_the_margin_is_the_measured_one():
    worst = 0.0
    for Kd in KS:
        M, N = (200, 1280) if Kd >= 4104 else (300, 320)
        a, b, acc, ref, S, T = problem(M, N, Kd, 8 if Kd < 1024 else 0)
        r = K.gate_b(acc(a).to(BF), ref, S, T)
        print(f"K={Kd}: B1 max ratio {r['b1_ratio']:.3f}  B2 row {r['b2_row']:.3f} col {r['b2_col']:.3f}")
        assert r["ok_b1"] and r["ok_b2"], (Kd, r)
        worst = max(worst, r["b2_row"], r["b2_col"])
    # the helper's docstring states margin = 1.25 x the largest ratio seen here (to three decimals); it must stay below 2 (else the floor is wrong)
    assert 1.25 * round(worst, 3) <= K.B2_MARGIN < 2.0, (worst, K.B2_MARGIN)


@pytest.mark.parametrize("Kd,M,N,K2", [(328, 300, 320, 8), (1280, 256, 64, 0), (4104, 200, 1280, 0)])
def test_gate_b_fails_a_dropped_k_term(Kd, M, N, K2):
    a, b, acc, ref, S, T = problem(M, N, Kd, K2)
    assert (lambda r: r["ok_b1"] and r["ok_b2"])(K.gate_b(acc(a).to(BF), ref, S, T))
    dropped = a.clone()
    dropped[17, Kd // 3] = 0                       # row 17 loses its term k = K / 3
    r = K.gate_b(acc(dropped).to(BF), ref, S, T)
    print(f"dropped k-term at K={Kd}: B1 {r['b1_bad']} elements over (max ratio {r['b1_ratio']:.2f}), B2 row {r['b2_row']:.2f} col {r['b2_col']:.2f}")
    assert not (r["ok_b1"] and r["ok_b2"])
    if Kd == 4104:
        assert not r["ok_b2"], "at K = 4104 the elementwise band is ~4.7 ulp wide: the RMS gate B2 must be the one that catches the dropped term"
        assert K.coarse(acc(dropped).to(BF), ref) < 8 * 2e-3, "the coarse gate A does not see this error -- which is why gate B exists"


@pytest.mark.parametrize("Kd,M,N,K2", [(328, 300, 320, 8), (1280, 256, 64, 0)])
def test_gate_b_fails_the_other_planted_errors(Kd, M, N, K2):
    a, b, acc, ref, S, T = problem(M, N, Kd, K2)
    good = acc(a)
    scaled = good.clone()
    scaled[:, 5] *= 1 + 2.0 ** -7
    swapped = good.clone()
    swapped[32:48, 10], swapped[32:48, 11] = good[32:48, 11], good[32:48, 10]
    off = good.to(BF).double()
    off[40, 7] += 2 * K.ulp_bf16(off[40, 7])
    for name, got in (("one column x (1 + 2^-7)", scaled.to(BF)), ("two columns swapped in a 16-row block", swapped.to(BF)), ("one element off by 2 ulp", off)):
        r = K.gate_b(got, ref, S, T)
        print(f"{name} at K={Kd}: B1 {r['b1_bad']} over (max ratio {r['b1_ratio']:.2f}), B2 row {r['b2_row']:.2f} col {r['b2_col']:.2f}")
        assert not (r["ok_b1"] and r["ok_b2"]), name


def test_scaled_column_is_caught_by_b2_where_b1_is_wide():
    a, b, acc, ref, S, T = problem(200, 1280, 4104, 0)
    scaled = acc(a)
    scaled[:, 5] *= 1 + 2.0 ** -7
    r = K.gate_b(scaled.to(BF), ref, S, T)
    assert not r["ok_b2"] and r["b2_col"] > 2.0
