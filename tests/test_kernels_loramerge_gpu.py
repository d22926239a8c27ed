"""Direct tests of ``fd_lora_merge_multi`` (csrc/lora.hip) through ``layers.refresh_pairs(..., merge=...)``: ``out = base + scale * up @ down`` in fp32
against the same product in fp64, under the first-order gate derived in tests/loramerge_cases.py (not a measured number with a margin).  Every tensor is
a view at an odd element offset of one flat buffer with sentinel guards around it; shapes are one-element rows, sizes that are no multiple of the
32 x 64 tile, ranks 1 / 4 / 50 / 64, the text encoder's fc1 at rank 50, and 17 pairs in one call (two launches)."""
import ctypes

import numpy as np
import pytest
import torch

import loramerge_cases as C
from finetune_fair_diffusion_amd import layers, lib, ops

pytestmark = pytest.mark.gpu
NAME = "fd_lora_merge_multi"


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def test_table_against_fp64(dev):
    assert lib.get().fd_working_dtype().decode() == "fp16"
    C.run_table(layers, dev, "fp16 library")


def test_ema_twin_is_the_source_with_ema(dev):
    case = C.SMALL[2]
    p = C.Problem(layers, dev, [case], seed=31)
    d, u, b = p.host[0]
    d2, u2, _ = C.inputs(case, 32)
    p.bank.view("d0", p.bank.ema).copy_(torch.from_numpy(d2))
    p.bank.view("u0", p.bank.ema).copy_(torch.from_numpy(u2))
    got = p.run(layers, in_place=False, ema=True)[0]
    C.check("ema=True", got, d2, u2, b, case[3])
    live = p.run(layers, in_place=False)[0]
    C.check("ema=False after it", live, d, u, b, case[3])
    assert not np.array_equal(_bits(got), _bits(live))


@pytest.mark.parametrize("which", ["scale 0", "zero up"])
def test_identities(dev, which):
    """scale = 0 and an all-zero up (a fresh LoRA) leave the weights as they were, in place and out of place."""
    for case in C.SMALL:
        p = C.Problem(layers, dev, [case], seed=40)
        _, _, b = p.host[0]
        if which == "zero up":
            p.bank.view("u0").zero_()
        scale = 0.0 if which == "scale 0" else case[3]
        assert np.array_equal(p.run(layers, in_place=False, scale=scale)[0], b), (which, case)
        assert np.array_equal(p.run(layers, in_place=True, scale=scale)[0], b), (which, case)


def test_two_calls_give_equal_bits_also_on_a_side_stream(dev):
    p = C.Problem(layers, dev, C.MIXED_17, seed=50)
    first = p.run(layers, in_place=False, scale=-2.5)
    second = p.run(layers, in_place=False, scale=-2.5)
    torch.cuda.synchronize()
    with torch.cuda.stream(torch.cuda.Stream()):
        third = p.run(layers, in_place=False, scale=-2.5)
    for a, b, c in zip(first, second, third):
        assert np.array_equal(_bits(a), _bits(b)) and np.array_equal(_bits(a), _bits(c))


def test_refusals_name_the_entry_point_and_leave_out_alone(dev):
    """Every refusal comes from the host before anything is launched: non-zero status, a message, ``out`` untouched -- also for the GOOD pairs of a call
    whose last pair is the bad one (the 17th: the first 16 would have been a launch of their own)."""
    L = lib.get()
    p = C.Problem(layers, dev, C.MIXED_17, seed=60)
    n = len(p.cases)

    def descs():
        arr = lib.LoraMergeDesc.array(n)
        for i, (d, (r, N, K, s)) in enumerate(zip(arr, p.cases)):
            d.down, d.up = p.bank.view(f"d{i}").data_ptr(), p.bank.view(f"u{i}").data_ptr()
            d.base, d.out, d.r, d.K, d.N, d.scale = p.base(i).data_ptr(), p.out(i).data_ptr(), r, K, N, s
        return arr

    last = n - 1
    r, N, K, _ = p.cases[last]
    bad = [("struct_size", lambda d: setattr(d, "struct_size", ctypes.sizeof(lib.LoraMergeDesc) - 8), "struct_size"),
           ("null down", lambda d: setattr(d, "down", None), "null"), ("null up", lambda d: setattr(d, "up", None), "null"),
           ("null base", lambda d: setattr(d, "base", None), "null"), ("null out", lambda d: setattr(d, "out", None), "null"),
           ("r = 0", lambda d: setattr(d, "r", 0), "rank"), ("r = 65", lambda d: setattr(d, "r", 65), "rank"),
           ("N < 0", lambda d: setattr(d, "N", -1), "extent"), ("K < 0", lambda d: setattr(d, "K", -K), "extent"),
           ("misaligned", lambda d: setattr(d, "up", d.up + 2), "aligned"),
           ("out partly over base", lambda d: setattr(d, "out", d.base + 4 * K), "overlaps base"),
           ("out over down", lambda d: setattr(d, "out", d.down), "overlaps"),
           ("out over another pair's out", lambda d: setattr(d, "out", p.out(0).data_ptr()), "overlaps")]
    for tag, spoil, word in bad:
        arr = descs()
        spoil(arr[last])
        rc = L.fd_lora_merge_multi(ctypes.byref(arr), n, ops._stream())
        msg = L.fd_last_error().decode()
        assert rc != 0 and NAME in msg and word in msg, (tag, rc, msg)
    with pytest.raises(RuntimeError, match=NAME + " failed.*overlaps base"):         # and through the wrapper
        off, num = p.bank.offsets["base0"]
        shifted = p.bank.flat[off + 2:off + 2 + num].view(p.cases[0][1], p.cases[0][2])
        layers.refresh_pairs(p.pairs[:1], 1.0, merge=[(p.base(0), shifted)])
    assert L.fd_lora_merge_multi(None, 1, None) != 0 and L.fd_lora_merge_multi(ctypes.byref(descs()), 0, None) != 0
    torch.cuda.synchronize()
    for i in range(n):
        assert bool((p.out(i) == C.SENTINEL).all()), f"a refused call wrote out of pair {i}"
    assert np.all(p.bank.outside() == C.SENTINEL)
    arr = descs()                                                                    # the same descriptors, unspoilt, are accepted
    assert L.fd_lora_merge_multi(ctypes.byref(arr), n, ops._stream()) == 0
    torch.cuda.synchronize()
    d, u, b = p.host[last]
    C.check("after the refusals", p.out(last).cpu().numpy(), d, u, b, p.cases[last][3])
