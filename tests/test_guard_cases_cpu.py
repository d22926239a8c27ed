"""The memory-guard arena of tests/guard_cases.py on CPU tensors (no GPU): its layout, what its report sees, that the gate of
tests/test_kernels_guard_gpu.py fails for the kernel bugs it exists for (torch stand-ins through the same ``check_case``) and passes for the correct
stand-in, and the bookkeeping of which entry point is guarded where."""
import ast
import os

import numpy as np
import pytest
import torch

import guard_cases as GC
from finetune_fair_diffusion_amd import lib
from test_kernel_coverage_cpu import EXEMPT

HERE = os.path.dirname(os.path.abspath(__file__))
CPU = torch.device("cpu")
H16, F32, I32 = torch.float16, torch.float32, torch.int32


def _rnd(*shape, seed, dtype=H16):
    return torch.randn(*shape, generator=torch.Generator().manual_seed(seed)).to(dtype)


def _mixed_arena():
    a = GC.Arena(CPU)
    a.inp("x", _rnd(5, 24, seed=1), ld=40, align=16)
    a.inp("kv", _rnd(2 * 13, 16, seed=2), ld=24, align=16, period=(13, 16))
    a.inp("flat2", _rnd(37, seed=3), align=2)
    a.inp("valid", torch.ones(2, 13, dtype=I32), align=4)
    a.inp("gamma", _rnd(24, seed=4, dtype=F32), align=4)
    a.out("y", (5, 24), H16, ld=32, align=8)
    a.out("lse", (2, 3, 5), F32, align=4)
    a.out("slab", (2 * 16, 8), F32, ld=12, align=16, period=(13, 16))
    a.out("acc", (7, 3), F32, ld=3, align=4, init=torch.ones(7, 3))
    a.ws("scratch", 10)
    return a.build()


def test_offsets_meet_exactly_the_stated_alignment_and_no_more():
    a = _mixed_arena()
    for name, s in a.specs.items():
        addr = a.address(name)
        assert addr % s.align == 0 and addr % (2 * s.align) == s.align, (name, addr, s.align)
        assert a.view(name).data_ptr() == addr
    assert a.specs["flat2"].align == 2 and a.specs["y"].align == 8 and a.specs["x"].align == 16 and a.specs["gamma"].align == 4


def test_views_have_the_strides_asked_for_and_a_full_tile_of_guard_on_both_sides():
    a = _mixed_arena()
    assert a.view("x").shape == (5, 24) and a.view("x").stride() == (40, 1)
    assert a.view("kv").shape == (32, 16) and a.view("kv").stride() == (24, 1) and a.tight("kv").shape == (26, 16)
    assert a.view("lse").shape == (2, 3, 5) and a.view("lse").is_contiguous()
    for dtype in a.flat:
        specs = sorted((s for s in a.specs.values() if s.dtype == dtype), key=lambda s: s.off)
        ends = [0] + [s.off + s.span for s in specs]
        for s, prev_end in zip(specs, ends):
            want = GC.TILE_ROWS * s.ld if s.strided else GC.FLAT_GUARD
            assert s.off - prev_end >= want and a.flat[dtype].numel() - (s.off + s.span) >= want, s.name


def test_views_never_overlap_and_the_guard_mask_is_the_complement_of_the_owned_elements():
    a = _mixed_arena()
    for dtype, flat in a.flat.items():
        flat.zero_()
    for name, s in a.specs.items():
        v = a.view(name)
        if s.strided:
            v[torch.from_numpy(s.valid_rows())] += 1         # through the VIEW the kernel gets: rows of stride ld, pad rows left out
        else:
            v += 1
    for dtype, flat in a.flat.items():
        counts = flat.float().numpy()
        assert counts.max() == 1, f"{dtype}: two operands share an element"
        assert np.array_equal(counts == 0, a.guard_mask(dtype))
    # gaps and pad rows are guard: x has 16 gap columns per row, kv 8 gap columns and rows 13..15 of each item
    x, kv = a.specs["x"], a.specs["kv"]
    m = a.guard_mask(H16)
    assert m[x.off + 24:x.off + 40].all() and not m[x.off:x.off + 24].any()
    assert m[kv.off + 13 * 24:kv.off + 16 * 24].all() and not m[kv.off + 16 * 24:kv.off + 16 * 24 + 16].any()


def test_poison_around_inputs_sentinel_around_outputs_nan_inside_outputs():
    a = _mixed_arena()
    h, f = a.flat[H16], a.flat[F32]
    x, kv, y, slab, acc = (a.specs[n] for n in ("x", "kv", "y", "slab", "acc"))
    assert torch.isnan(h[x.off - 64 * 40:x.off]).all() and torch.isnan(h[x.off + 24:x.off + 40]).all() and torch.isnan(h[x.off + x.span:x.off + x.span + 64 * 40]).all()
    assert torch.isnan(a.view("kv")[13:16]).all() and torch.isnan(a.view("kv")[29:32]).all() and torch.isfinite(a.tight("kv")).all()
    assert (h[y.off - 64 * 32:y.off] == GC.SENTINEL).all() and (h[y.off + 24:y.off + 32] == GC.SENTINEL).all() and torch.isnan(a.view("y")).all()
    assert (a.view("slab")[13:16] == GC.SENTINEL).all() and torch.isnan(a.tight("slab")).all()
    assert (a.view("acc") == 1).all() and (f[acc.off - GC.TILE_ROWS * 3:acc.off] == GC.SENTINEL).all()
    iv = a.specs["valid"]
    assert (a.flat[I32][iv.off - GC.FLAT_GUARD:iv.off] == GC.INT_POISON).all() and GC.INT_POISON not in (0, 1)


def _write_all_outputs(a):
    for name, s in a.specs.items():
        if s.role == "out":
            v = a.view(name)
            if s.strided:
                v[torch.from_numpy(s.valid_rows())] = 0.5
            else:
                v.fill_(0.5)


def test_a_clean_run_reports_nothing():
    a = _mixed_arena()
    _write_all_outputs(a)
    a.view("scratch").fill_(3.0)
    rep = a.report()
    assert rep == dict(guards=[], inputs=[], unwritten={}, stray={}, nonfinite={}), rep
    GC.check_case("clean", a, {"y": torch.full((5, 24), 0.5, dtype=H16)}, show=False)


@pytest.mark.parametrize("where", ["guard before", "guard behind", "gap column", "pad row", "one row behind the output", "workspace + 1", "same value, other bits"])
def test_a_planted_one_element_write_outside_the_operands_is_reported(where):
    a = _mixed_arena()
    _write_all_outputs(a)
    y, slab, ws = a.specs["y"], a.specs["slab"], a.specs["scratch"]
    h, f = a.flat[H16], a.flat[F32]
    if where == "guard before":
        h[y.off - 1] = 1.0
    elif where == "guard behind":
        h[y.off + y.span] = 1.0
    elif where == "gap column":
        h[y.off + 2 * y.ld + y.cols] = 1.0
    elif where == "pad row":
        f[slab.off + 14 * slab.ld + 3] = 1.0
    elif where == "one row behind the output":
        h[y.off + y.rows * y.ld] = 1.0
    elif where == "workspace + 1":
        f[ws.off + ws.span] = 1.0
    else:                                                   # NaN with another payload in an input's guard: bit-intact means bits
        x = a.specs["x"]
        h.view(torch.int16)[x.off - 1] = 0x7E01
    rep = a.report()
    assert len(rep["guards"]) == 1, rep
    with pytest.raises(GC.GuardFailure, match="written outside the operands"):
        GC.check_case(where, a, {}, show=False)


def test_unwritten_stray_nonfinite_and_modified_inputs_are_reported():
    a = _mixed_arena()
    _write_all_outputs(a)
    a.view("y")[4, 23] = float("nan")
    assert a.report()["unwritten"] == {"y": 1}
    with pytest.raises(GC.GuardFailure, match="still hold NaN"):
        GC.check_case("unwritten", a, {}, show=False)
    a.view("y")[4, 23] = float("inf")
    assert a.report()["nonfinite"] == {"y": 1} and not a.report()["unwritten"]
    a.view("y")[4, 23] = 0.5
    a.view("x")[0, 0] += 1
    assert a.report()["inputs"] == ["x"]
    # an output the contract leaves partly unwritten: exactly the documented part
    w = torch.zeros(4, 6, dtype=torch.bool)
    w[:3] = True
    b = GC.Arena(CPU).out("part", (4, 6), F32, ld=6, align=4, written=w).build()
    b.view("part")[:3] = 1.0
    assert b.report() == dict(guards=[], inputs=[], unwritten={}, stray={}, nonfinite={})
    GC.check_case("documented part", b, {"part": torch.ones(4, 6)}, show=False)
    b.view("part")[3, 0] = 1.0
    assert b.report()["stray"] == {"part": 1}
    b.view("part")[3, 0] = float("nan")
    b.view("part")[2, 5] = float("nan")
    assert b.report()["unwritten"] == {"part": 1}


def test_a_result_that_differs_from_the_baseline_by_one_ulp_fails_the_gate():
    a = _mixed_arena()
    _write_all_outputs(a)
    want = torch.full((5, 24), 0.5, dtype=H16)
    want.view(torch.int16)[2, 2] += 1
    with pytest.raises(GC.GuardFailure, match="differs from the tight-layout baseline in 1 of"):
        GC.check_case("ulp", a, {"y": want}, show=False)
    # ... unless the case is gated by a band, which then sees the two tensors
    seen = []
    GC.check_case("band", a, {"y": want}, band=lambda n, g, w: seen.append((n, float((g.float() - w.float()).abs().max()))) or "ok", show=False)
    assert seen and seen[0][0] == "y" and 0 < seen[0][1] < 1e-3


# ============================================================================= the gate catches what it is for
B_, H_, TQ, TK, TKR, D_ = 2, 2, 5, 13, 16, 8


def _attention_case(fault):
    C = H_ * D_
    q, k, v = _rnd(B_ * TQ, C, seed=1), _rnd(B_ * TK, C, seed=2), _rnd(B_ * TK, C, seed=3)
    base = torch.empty(B_ * TQ, C, dtype=H16)
    GC.standin_attention(q, k, v, base, H_, TQ, TK, TK)
    a = GC.Arena(CPU)
    a.inp("q", q, ld=C + 8).inp("k", k, ld=C + 8, period=(TK, TKR)).inp("v", v, ld=C + 8, period=(TK, TKR)).out("o", (B_ * TQ, C), H16, ld=C).build()
    GC.standin_attention(a.view("q"), a.view("k"), a.view("v"), a.view("o"), H_, TQ, TK, TKR, fault)
    return a, {"o": base}


def test_correct_standins_pass_the_gate():
    a, base = _attention_case(None)
    GC.check_case("attention stand-in", a, base, show=False)
    a, base = _layernorm_case(None)
    GC.check_case("layernorm stand-in", a, base, show=False)
    a, base = _scale_case(False)
    GC.check_case("element-wise stand-in", a, base, show=False)
    a, base = _groupnorm_case(0)
    GC.check_case("groupnorm stand-in", a, base, show=False)


@pytest.mark.parametrize("fault", ["pad_keys", "pad_v_rows"])
def test_an_attention_that_touches_the_pad_rows_fails_the_gate(fault):
    """rows Tk..Tkr counted as keys, or loaded under a probability of exactly 0: the NaN in them surfaces in o"""
    a, base = _attention_case(fault)
    with pytest.raises(GC.GuardFailure, match="still hold NaN"):
        GC.check_case(fault, a, base, show=False)


def _layernorm_case(R):
    M, C = 5, 16
    x = _rnd(M, C, seed=4)
    base = torch.empty(M, C, dtype=H16)
    GC.standin_layernorm(x, base, M)
    a = GC.Arena(CPU).inp("x", x, ld=C).out("y", (M, C), H16, ld=C).build()
    GC.standin_layernorm(a.view("x"), a.view("y"), M, R)
    return a, {"y": base}


def test_a_layernorm_that_writes_whole_groups_of_rows_fails_the_gate():
    a, base = _layernorm_case(4)                # ceil(5 / 4) * 4 = 8 rows written
    with pytest.raises(GC.GuardFailure, match=r"written outside the operands.*y\+80"):
        GC.check_case("layernorm R=4", a, base, show=False)


def _scale_case(round_up):
    n = 8 * 3 + 5
    x = _rnd(n, seed=5)
    base = torch.empty(n, dtype=H16)
    GC.standin_scale(x, base, n)
    a = GC.Arena(CPU).inp("x", x, align=16).out("y", (n,), H16, align=16).build()
    GC.standin_scale(a.view("x"), a.view("y"), n, round_up)
    return a, {"y": base}


def test_an_elementwise_op_that_rounds_n_up_to_8_fails_the_gate():
    a, base = _scale_case(True)
    with pytest.raises(GC.GuardFailure, match=r"written outside the operands.*y\+29"):
        GC.check_case("scale, n rounded up", a, base, show=False)


def _groupnorm_case(extra):
    Bn, G, n, slots = 2, 4, 10, 64
    x = _rnd(Bn, G, n, seed=6)
    base = torch.empty(Bn, G, 2)
    GC.standin_groupnorm_stats(x, base, torch.empty(Bn * slots * G * 2 + 1), Bn, G, slots)
    a = GC.Arena(CPU).inp("x", x).out("stats", (Bn, G, 2), F32, align=4).ws("scratch", Bn * slots * G * 2).build()
    GC.standin_groupnorm_stats(a.view("x"), a.view("stats"), a.view("scratch"), Bn, G, slots, extra)
    return a, {"stats": base}


def test_a_groupnorm_that_uses_one_scratch_float_more_than_documented_fails_the_gate():
    a, base = _groupnorm_case(1)
    with pytest.raises(GC.GuardFailure, match=r"written outside the operands.*scratch\+1024"):
        GC.check_case("groupnorm scratch + 1", a, base, show=False)


# ============================================================================= geometry restated from the sources
def test_restated_geometry_matches_the_sources():
    src = open(os.path.join(HERE, "..", "finetune_fair_diffusion_amd", "csrc", "norm.hip")).read()
    assert "#define GN_MAX_CHUNKS 64" in src and "constexpr int R1 = 4, R2 = 4, R4 = 2;" in src
    assert "if (C % CB || CB / cg > 4 || CB / 8 > 16) return false;" in src and "gn_fused_geometry(C1 + C2, HW, groups, 24, f)" in src
    assert "gn_fused_geometry(C1 + C2, HW, groups, 12, f)" in src and "if (f.nv <= 8)" in src
    assert [GC.gn_fwd_branch(320, hw, 32) for hw in (100, 408, 409, 1224, 1225)] == ["fused<8>", "fused<8>", "fused<24>", "fused<24>", "two-launch"]
    assert [GC.gn_bwd_branch(320, hw, 32) for hw in (612, 613)] == ["fused", "two-launch"]
    assert GC.gn_chunk_rows(320, 1300) == (21, 62) and GC.gn_chunk_rows(320, 100) == (6, 17)
    attn = open(os.path.join(HERE, "..", "finetune_fair_diffusion_amd", "csrc", "attn.hip")).read()
    assert "(d <= 64 && Tq >= 2048 && Tk >= 2048 && (long)BH * ((Tq + 255) / 256) >= 128) ? 2 : 1" in attn
    assert GC.fwd_two_blocks(40, 2049, 2050, 16) and not GC.fwd_two_blocks(40, 2049, 2050, 8) and not GC.fwd_two_blocks(80, 2049, 2050, 16)
    lora = open(os.path.join(HERE, "..", "finetune_fair_diffusion_amd", "csrc", "lora.hip")).read()
    assert "int nsplit = (768 + ncb - 1) / ncb;" in lora and "if (nsplit > (M + 63) / 64) nsplit = (M + 63) / 64;" in lora
    assert GC.wgrad_scratch(130, 320, 4, 328) == (True, 3 * 320 * 8) and GC.wgrad_scratch(130, 324, 4, 332) == (False, 3 * 324 * 8)


# ============================================================================= bookkeeping
def _test_functions(module):
    tree = ast.parse(open(os.path.join(HERE, module)).read())
    return {n.name: n for n in tree.body if isinstance(n, ast.FunctionDef)}


def _literals(fn, helpers, depth=2):
    out = {n.value for n in ast.walk(fn) if isinstance(n, ast.Constant) and isinstance(n.value, str) and n.value.startswith("fd_")}
    if depth:
        for c in ast.walk(fn):
            if isinstance(c, ast.Call) and isinstance(c.func, ast.Name) and c.func.id in helpers and helpers[c.func.id] is not fn:
                out |= _literals(helpers[c.func.id], helpers, depth - 1)
    return out


def test_every_launching_entry_point_is_guarded_listed_as_guarded_elsewhere_or_listed_as_the_remaining_gap():
    launching = set(lib.parse_header()) - set(EXEMPT)
    places = (GC.GUARD_TABLE, GC.ALREADY_GUARDED, GC.NOT_YET_GUARDED)
    for name in sorted(launching):
        n = sum(name in p for p in places)
        assert n == 1, f"{name} is in {n} of GUARD_TABLE / ALREADY_GUARDED / NOT_YET_GUARDED (tests/guard_cases.py): exactly one is right"
    for p in places:
        gone = sorted(set(p) - launching)
        assert not gone, f"listed but not a launching entry point of include/fairdiff_hip.h: {gone}"
    assert all(isinstance(r, str) and r for r in GC.NOT_YET_GUARDED.values())


def test_the_guard_table_names_tests_that_call_the_entry_point_by_name():
    fns = _test_functions("test_kernels_guard_gpu.py")
    for name, test in GC.GUARD_TABLE.items():
        assert test in fns and test.startswith("test_"), f"{name}: tests/test_kernels_guard_gpu.py::{test} does not exist"
        assert name in _literals(fns[test], fns), f"{name}: {test} does not launch it through ops._call by its literal name"


def test_the_tests_named_as_already_guarding_exist():
    for name, (module, test) in GC.ALREADY_GUARDED.items():
        assert test in _test_functions(module), f"{name}: tests/{module}::{test} is gone"
