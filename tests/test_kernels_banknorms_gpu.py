"""Direct tests of ``fd_bank_norms`` (csrc/elementwise.hip) through ``ops.adamw_ema(..., apply=False, norms=...)``: per-tensor L2 norms, their mean and
the global L2 norm of up to four flat fp32 buffers against ``torch.linalg.vector_norm`` of the same values in fp64.  The gate is the bound derived in
tests/banknorms_cases.py from the accumulation scheme (CH = 8192 elements per workgroup of 256 threads: 32 fp32 squares per thread, everything after
that in fp64): 18 * 2^-24 + 2^-38 = 1.07e-6 relative -- not a measured number with a margin.  The bank holds tensors of 1, 3, CH - 1, CH, CH + 1 and
2 CH + 5 elements, a 1280 x 50 matrix and an all-zero tensor."""
import numpy as np
import pytest
import torch

import banknorms_cases as C
from finetune_fair_diffusion_amd import layers, lib, ops, weights as W

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def case(dev):
    """The bank, its references (computed once, never changed) and the result of the three-buffer call every other test compares with."""
    bank = C.make_bank(layers, dev)
    refs = {name: C.reference(bank, getattr(bank, name)) for name in C.BUFFERS}
    plan = bank.norm_plan()
    plan.out.fill_(C.SENTINEL)
    norms, summary = C.norms_only(ops, plan, p=bank.flat, ema=bank.ema, g=bank.grad)
    return bank, refs, norms, summary


def _equal_bits(a, b):
    return np.array_equal(a.view(np.uint32), b.view(np.uint32))


def test_three_buffers_against_fp64(case):
    bank, refs, norms, summary = case
    for b, name in enumerate(C.BUFFERS[:3]):
        C.check_row(name, norms[b], summary[b], refs[name])
    assert norms[:3, bank.names.index("zeros")].tolist() == [0.0, 0.0, 0.0]
    assert np.all(norms[3] == C.SENTINEL) and np.all(summary[3] == C.SENTINEL), "rows of an absent buffer are not written"


def test_one_buffer_and_all_four(case):
    bank, refs, norms, summary = case
    plan = bank.norm_plan()
    plan.out.fill_(C.SENTINEL)
    n1, s1 = C.norms_only(ops, plan, p=bank.flat)
    assert _equal_bits(n1[0], norms[0]) and _equal_bits(s1[0], summary[0]) and np.all(n1[1:] == C.SENTINEL) and np.all(s1[1:] == C.SENTINEL)
    plan.out.fill_(C.SENTINEL)
    n1, s1 = C.norms_only(ops, plan, g=bank.grad)
    assert _equal_bits(n1[2], norms[2]) and _equal_bits(s1[2], summary[2]) and np.all(n1[[0, 1, 3]] == C.SENTINEL) and np.all(s1[[0, 1, 3]] == C.SENTINEL)
    plan.extra = bank.exp_avg
    try:
        n4, s4 = C.norms_only(ops, plan, p=bank.flat, ema=bank.ema, g=bank.grad)
    finally:
        plan.extra = None
    assert _equal_bits(n4[:3], norms[:3]) and _equal_bits(s4[:3], summary[:3])
    C.check_row("exp_avg (fourth buffer)", n4[3], s4[3], refs["exp_avg"])


def test_padding_between_tensors_is_never_read(case):
    bank, refs, norms, summary = case
    pad = C.padding_mask(bank).to(bank.flat.device)
    assert int(pad.sum()) >= 11
    dirty = {name: getattr(bank, name).clone() for name in C.BUFFERS[:3]}
    for t in dirty.values():
        t[pad] = float("nan")
    n, s = C.norms_only(ops, bank.norm_plan(), p=dirty["flat"], ema=dirty["ema"], g=dirty["grad"])
    assert _equal_bits(n[:3], norms[:3]) and _equal_bits(s[:3], summary[:3]), "NaN in the padding slots reached a result"


def test_inf_stays_in_its_tensor_and_its_buffer(case):
    bank, refs, norms, summary = case
    ema = bank.ema.clone()
    k = bank.names.index("t_ch_plus_1")
    off, num = bank.offsets["t_ch_plus_1"]
    ema[off + num - 1] = float("-inf")          # the last element: the second chunk of the tensor, and its scalar tail
    n, s = C.norms_only(ops, bank.norm_plan(), p=bank.flat, ema=ema, g=bank.grad)
    assert n[1, k] == np.inf and s[1, 0] == np.inf and s[1, 1] == np.inf
    others = np.arange(len(bank.names)) != k
    assert _equal_bits(n[1, others], norms[1, others]) and _equal_bits(n[[0, 2]], norms[[0, 2]]) and _equal_bits(s[[0, 2]], summary[[0, 2]])


def test_repeats_give_equal_bits_also_on_a_side_stream(case):
    bank, refs, norms, summary = case
    plan = bank.norm_plan()
    n2, s2 = C.norms_only(ops, plan, p=bank.flat, ema=bank.ema, g=bank.grad)
    assert _equal_bits(n2[:3], norms[:3]) and _equal_bits(s2[:3], summary[:3])
    plan.out.zero_()
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        n3, s3 = C.norms_only(ops, plan, p=bank.flat, ema=bank.ema, g=bank.grad)
    torch.cuda.synchronize()
    assert _equal_bits(n3[:3], norms[:3]) and _equal_bits(s3[:3], summary[:3])


def test_refusals_name_the_entry_point_and_leave_the_outputs_alone(case, dev):
    bank, refs, norms, summary = case
    plan = bank.norm_plan()
    plan.out.fill_(C.SENTINEL)
    shifted = torch.zeros(bank.numel + 4, dtype=torch.float32, device=dev)[1:1 + bank.numel]          # 4 bytes past a 16-byte boundary
    for kw, word in ((dict(p=shifted), "aligned to 16"), (dict(), "no buffer")):
        with pytest.raises(RuntimeError, match="fd_bank_norms failed.*fd_bank_norms: .*" + word):
            C.norms_only(ops, plan, **kw)
        assert b"fd_bank_norms" in lib.get().fd_last_error()
    nseg, plan.nseg = plan.nseg, 0
    try:
        with pytest.raises(RuntimeError, match="fd_bank_norms: .*nseg = 0"):
            C.norms_only(ops, plan, p=bank.flat)
    finally:
        plan.nseg = nseg
    torch.cuda.synchronize()
    assert bool((plan.out == C.SENTINEL).all()), "a refused call wrote an output"


def test_rank_50_unet_inventory(dev):
    """The bank the reduction exists for: 256 tensors, 9.96 M floats, ~1300 chunks; data drawn on the device, references by torch in fp64 there."""
    bank = layers.ParamBank(W.unet_lora_param_shapes(W.UNetConfig(), 50), dev)
    g = torch.Generator(device=dev).manual_seed(50)
    bufs = (bank.flat, bank.ema, bank.grad)
    for t, scale in zip(bufs, C.SCALES):
        t.copy_(torch.randn(bank.numel, generator=g, device=dev) * scale)         # the padding slots too: they must not count
    plan = bank.norm_plan()
    assert plan.nseg == 256 and 1200 <= plan.nchunks <= 2048
    n, s = C.norms_only(ops, plan, p=bank.flat, ema=bank.ema, g=bank.grad)
    for b, t in enumerate(bufs):
        per = torch.stack([torch.linalg.vector_norm(bank.view(name, t).double()) for name in bank.names])
        ref = (per.cpu().numpy(), float(per.mean()), float(torch.linalg.vector_norm(per)))
        C.check_row(f"rank-50 U-Net {C.BUFFERS[b]}", n[b], s[b], ref)
