"""How ``ops.wgrad_batch`` shares out LoRA weight-gradient problems of ranks 1..64 (no GPU: ``ops._call`` is a recorder and the tensors live on the CPU),
and what the header and INTEGRATION.md say about fd_lora_wgrad_multi's ranks."""
import ctypes
import os
import re

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture()
def rec(monkeypatch):
    """``ops`` with every device touch replaced: _call records (name, problems), where a problem is (X ptr, ldx, T ptr, ldt, G ptr, sn, sr, M, N, R, scale)."""
    from finetune_fair_diffusion_amd import lib, ops
    calls = []

    def call(name, *args):
        if name == "fd_lora_wgrad_multi":
            arr = ctypes.cast(args[0], ctypes.POINTER(lib.WgradDesc))
            calls.append((name, [(arr[i].X, arr[i].ldx, arr[i].T, arr[i].ldt, arr[i].G, arr[i].g_stride_n, arr[i].g_stride_r, arr[i].M, arr[i].N, arr[i].R,
                                  arr[i].scale) for i in range(args[1])], args[3]))
        else:
            X, ldx, T, ldt, G, sn, sr, M, N, R, scale = args[:11]
            calls.append((name, [(X.value, ldx, T.value, ldt, G.value, sn, sr, M, N, R, scale)], args[12]))

    monkeypatch.setattr(ops, "_call", call)
    monkeypatch.setattr(ops, "_p", lambda t: ctypes.c_void_p(t.data_ptr()))
    monkeypatch.setattr(ops, "_stream", lambda: None)
    monkeypatch.setattr(ops, "scratch", lambda n, device: _Scratch(n))
    return ops, calls


class _Scratch:
    """Stands in for the scratch tensor: only its address and size are passed on."""

    def __init__(self, n):
        self.n = n

    def numel(self):
        return self.n

    def data_ptr(self):
        return 0


def _problem(ops, M, N, R, extra=0, seed=0):
    rp = ops._wgrad_rp(R)
    X = torch.zeros(M, N + extra, dtype=ops.F16)[:, :N]
    T = torch.zeros(M, rp, dtype=ops.F16)
    G = torch.zeros(N, R)
    return X, T, G, R, 1, R, 0.25 + seed


def _desc(it):
    X, T, G, sn, sr, R, scale = it
    return (X.data_ptr(), X.stride(0), T.data_ptr(), T.stride(0), G.data_ptr(), sn, sr, X.shape[0], X.shape[1], R, scale)


def _parent_rule(pend):
    """The grouping rule of flush_wgrads before ranks above 16 were queued, restated: problems of R <= 16 whose N and ldx are multiples of 8 are queued; on exit
    they go out by padded rank (8, then 16, in order of first appearance), 16 at a time, each call with a scratch of 2^22 floats; the rest goes out at once."""
    single, by_rp = [], {}
    for it in pend:
        X, R = it[0], it[5]
        if R <= 16 and X.shape[1] % 8 == 0 and X.stride(0) % 8 == 0:
            by_rp.setdefault(8 if R <= 8 else 16, []).append(it)
        else:
            single.append(("fd_lora_wgrad", [_desc(it)], 1 << 22))
    multi = [("fd_lora_wgrad_multi", [_desc(it) for it in items[i:i + 16]], 1 << 22) for items in by_rp.values() for i in range(0, len(items), 16)]
    return single + multi


def _issue(ops, items):
    with ops.wgrad_batch():
        for X, T, G, sn, sr, R, scale in items:
            ops.lora_wgrad(X, T, G, sn, sr, R, scale=scale)


def test_rank_50_problems_are_queued_and_chunked(rec):
    ops, calls = rec
    small = [_problem(ops, 64, 320, 4, seed=i) for i in range(3)]
    big = [_problem(ops, 64, 320, 50, seed=10 + i) for i in range(18)]
    odd = _problem(ops, 64, 320, 50, extra=4, seed=99)                      # ldx % 8 == 4: not for the MFMA arm
    items = [small[0], *big[:9], small[1], odd, *big[9:], small[2]]
    _issue(ops, items)
    shape = [(name, len(ps)) for name, ps, _ in calls]
    assert shape == [("fd_lora_wgrad", 1), ("fd_lora_wgrad_multi", 3), ("fd_lora_wgrad_multi", 16), ("fd_lora_wgrad_multi", 2)], shape
    assert calls[0][1] == [_desc(odd)]
    assert calls[1][1] == [_desc(it) for it in small]
    assert calls[2][1] + calls[3][1] == [_desc(it) for it in big], "rank-50 problems keep their order across the two calls"
    assert calls[1][2] == 1 << 22 and calls[2][2] == calls[3][2] == ops.WGRAD_MFMA_SCRATCH >= 16 * 1280 * 64


def test_small_ranks_go_out_exactly_as_before(rec):
    """For R <= 16 the calls, their order and their arguments equal the parent's rule -- also with rank-50 problems issued in between, which only add calls."""
    ops, calls = rec
    mix = [_problem(ops, 100 + i, 320 if i % 3 else 640, R, extra=(4 if i == 5 else 0), seed=i) for i, R in enumerate([4, 12, 4, 8, 16, 4, 9, 3] * 5)]
    _issue(ops, mix)
    assert calls == _parent_rule(mix)
    del calls[:]
    with_big = []
    for i, it in enumerate(mix):
        with_big.append(it)
        if i % 4 == 0:
            with_big.append(_problem(ops, 64, 320, 50, seed=1000 + i))
    _issue(ops, with_big)
    assert [c for c in calls if all(p[9] <= 16 for p in c[1])] == _parent_rule(mix)
    assert sum(len(c[1]) for c in calls if c[1][0][9] == 50) == 10


@pytest.mark.parametrize("field,change", [("ldt", lambda X, T: (X, T[:, :56].contiguous())), ("T alignment", lambda X, T: (X, T.reshape(-1)[4:4 + 63 * 64].reshape(63, 64))),
                                          ("X alignment", lambda X, T: (X.reshape(-1)[4:4 + 63 * 320].reshape(63, 320), T)), ("N", lambda X, T: (X[:, :316], T))])
def test_what_the_mfma_arm_cannot_take_is_not_queued(rec, field, change):
    ops, calls = rec
    X, T, G, sn, sr, R, scale = _problem(ops, 64, 320, 50)
    X, T = change(X, T)
    _issue(ops, [(X, T[:X.shape[0]], G, sn, sr, R, scale)])
    assert [name for name, _, _ in calls] == ["fd_lora_wgrad"], f"{field}: {calls}"


def test_header_and_integration_md_state_the_four_padded_ranks():
    hdr = open(os.path.join(ROOT, "include", "fairdiff_hip.h")).read()
    m = re.search(r"/\* batched form:.*?\*/\s*#define FD_WGRAD_MAX", hdr, flags=re.S)
    assert m, "the comment above FD_WGRAD_MAX is gone"
    md = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    row = next((ln for ln in md.splitlines() if ln.startswith("| `fd_lora_wgrad_multi`")), None)
    assert row, "INTEGRATION.md has no row for fd_lora_wgrad_multi"
    for text, where in ((" ".join(m.group(0).replace("%%", "%").replace(" * ", " ").split()), "header"), (row, "INTEGRATION.md")):
        for needle in ("8, 16, 32 or 64", "17..32, 33..64", "N % 8 == 0", "ldx % 8 == 0", "ldt >= the padded rank", "ldt % 8 == 0", "X and T aligned to 16 bytes", "FD_ERR_ARG"):
            assert needle in text, f"{where}: '{needle}' missing"
