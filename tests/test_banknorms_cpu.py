"""Host layer of the per-step parameter norms (no GPU): the chunk table of ``fd_bank_norms`` for the real inventories and a hand-made bank, the
entry point in the header and in the built libraries, what ``ops.adamw_ema`` launches (``ops._call`` replaced by a recorder), the flag and the
fields of the JSON line."""
import ctypes
import json
import math
import os
import re

import pytest
import torch

from finetune_fair_diffusion_amd import cli, layers, lib, weights as W

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAME = "fd_bank_norms"
CH = layers.NORM_CHUNK
HAND_MADE = {"t1": (1,), "t3": (3,), "t_ch_minus_1": (CH - 1,), "t_ch": (CH,), "t_ch_plus_1": (CH + 1,), "t_2ch_plus_5": (2 * CH + 5,)}
INVENTORIES = {"unet rank 4": lambda: W.unet_lora_param_shapes(W.UNetConfig(), 4), "unet rank 50": lambda: W.unet_lora_param_shapes(W.UNetConfig(), 50),
               "text encoder rank 4": lambda: W.clip_lora_param_shapes(W.CLIPTextConfig(), 4), "hand-made": lambda: HAND_MADE}


def test_chunk_length_is_the_headers():
    m = re.search(r"#define\s+FD_BANK_NORMS_CH\s+(\d+)", open(os.path.join(ROOT, "include", "fairdiff_hip.h")).read())
    assert m and int(m.group(1)) == CH and CH % 1024 == 0


@pytest.mark.parametrize("which", list(INVENTORIES))
def test_chunk_table_covers_every_tensor_once_and_nothing_else(which):
    bank = layers.ParamBank(INVENTORIES[which](), "cpu")
    assert bank._norm_plan is None, "the plan is built lazily"
    plan = bank.norm_plan()
    assert bank.norm_plan() is plan, "and cached"
    extents = [bank.offsets[n] for n in bank.names]
    chunks = layers.norm_chunks(extents)
    assert plan.table.tolist() == [list(c) for c in chunks] and plan.table.dtype == torch.int64 and plan.nchunks == len(chunks)
    assert plan.nseg == len(bank.names) == len(extents) and plan.numel == bank.numel and plan.names == bank.names
    assert plan.workspace.numel() == 4 * plan.nchunks and plan.workspace.dtype == torch.float64 and plan.out.numel() == 4 * plan.nseg + 8
    cover = torch.zeros(bank.numel, dtype=torch.int32)
    owner = torch.full((bank.numel,), -1, dtype=torch.int64)         # -1: a padding slot
    for s, (off, num) in enumerate(extents):
        assert off % 4 == 0
        owner[off:off + num] = s
    last = (-1, -1)
    for seg, off, ln in chunks:
        assert 1 <= ln <= CH and 0 <= off and off + ln <= bank.numel
        assert bool((owner[off:off + ln] == seg).all()), f"chunk ({seg}, {off}, {ln}) crosses a tensor or touches padding"
        assert (seg, off) > last, "segments never decrease and the chunks of a segment ascend"
        last = (seg, off)
        cover[off:off + ln] += 1
    assert bool((cover[owner >= 0] == 1).all()) and bool((cover[owner < 0] == 0).all())
    if which == "hand-made":
        assert [c[2] for c in chunks] == [1, 3, CH - 1, CH, CH, 1, CH, CH, 5] and int((owner < 0).sum()) == 3 + 1 + 1 + 3 + 3
    if which == "unet rank 50":
        assert plan.nseg == 256 and sum(n for _, n in extents) > 9_900_000


def test_entry_point_is_declared_additively_and_exported():
    protos = lib.parse_header()
    assert NAME in protos and lib.ABI_VERSION == 4
    ret, argtypes = protos[NAME]
    assert ret is ctypes.c_int and argtypes == [ctypes.c_void_p] * 4 + [ctypes.c_int64, ctypes.c_void_p, ctypes.c_int, ctypes.c_int] + [ctypes.c_void_p] * 4
    assert "#define FD_ABI_VERSION 4" in " ".join(open(os.path.join(ROOT, "include", "fairdiff_hip.h")).read().split())
    row = [l for l in open(os.path.join(ROOT, "INTEGRATION.md")).read().splitlines() if l.startswith("| `" + NAME + "`")]
    assert len(row) == 1
    pkg = os.path.dirname(lib.LIB_PATH)
    built = [so for so in ("libfairdiff_hip.so", "libfairdiff_hip_bf16.so") if os.path.exists(os.path.join(pkg, so))]
    if not built:
        pytest.skip("the libraries are not built")
    for so in built:
        assert getattr(ctypes.CDLL(os.path.join(pkg, so)), NAME)


def test_refusals_come_before_any_launch():
    """Refused calls return -1 with a message naming the entry point and launch nothing, so host memory stands in for the buffers."""
    path = os.path.join(os.path.dirname(lib.LIB_PATH), "libfairdiff_hip.so")
    if not os.path.exists(path):
        pytest.skip("the library is not built")
    L = ctypes.CDLL(path)
    fn = getattr(L, NAME)
    fn.restype, fn.argtypes = lib.parse_header()[NAME]
    L.fd_last_error.restype = ctypes.c_char_p
    raw = ctypes.create_string_buffer(256)
    ok = (ctypes.addressof(raw) + 63) // 64 * 64
    good = dict(b0=ok, b1=None, b2=None, b3=None, n=8, table=ok, nchunks=1, nseg=1, ws=ok, norms=ok, summary=ok)

    def call(**kw):
        a = dict(good, **kw)
        return fn(a["b0"], a["b1"], a["b2"], a["b3"], a["n"], a["table"], a["nchunks"], a["nseg"], a["ws"], a["norms"], a["summary"], None)

    for kw, word in ((dict(b0=None), b"no buffer"), (dict(b0=ok + 4), b"aligned to 16"), (dict(b2=ok + 8), b"aligned to 16"), (dict(nseg=0), b"nseg = 0"),
                     (dict(nchunks=0), b"nchunks = 0"), (dict(n=0), b"n = 0"), (dict(table=None), b"null"), (dict(ws=None), b"null"), (dict(norms=None), b"null"),
                     (dict(summary=None), b"null"), (dict(ws=ok + 4), b"8 bytes")):
        assert call(**kw) == -1 and NAME.encode() in L.fd_last_error() and word in L.fd_last_error(), (kw, L.fd_last_error())


@pytest.fixture()
def rec(monkeypatch):
    """``ops`` with every device touch replaced (the method of tests/test_lora_wgrad_rank_cpu.py): _call records (name, args)."""
    from finetune_fair_diffusion_amd import ops
    calls = []
    monkeypatch.setattr(ops, "_call", lambda name, *args: calls.append((name, args)))
    monkeypatch.setattr(ops, "_p", lambda t: None if t is None else t.data_ptr())
    monkeypatch.setattr(ops, "_stream", lambda: "stream")
    return ops, calls


def test_adamw_ema_launches(rec):
    ops, calls = rec
    bank = layers.ParamBank({"a.down.weight": (4, 8), "a.up.weight": (8, 4), "b": (CH + 3,)}, "cpu")
    hyper = (5e-3, 0.9, 0.999, 1e-8, 1e-2, 7, 0.25)
    bufs = (bank.flat, bank.grad, bank.exp_avg, bank.exp_avg_sq, bank.ema)
    today = ("fd_adamw_ema", tuple(t.data_ptr() for t in bufs) + (bank.numel,) + hyper + ("stream",))
    ops.adamw_ema(*bufs, *hyper)
    assert calls == [today] and len(calls[0][1]) == 14 and bank._norm_plan is None
    del calls[:]
    plan = bank.norm_plan()
    ops.adamw_ema(*bufs, *hyper, norms=plan)
    assert [c[0] for c in calls] == ["fd_adamw_ema", NAME] and calls[0] == today
    want = (bank.flat.data_ptr(), bank.ema.data_ptr(), bank.grad.data_ptr(), None, bank.numel, plan.table.data_ptr(), 4, 3, plan.workspace.data_ptr(),
            plan.out.data_ptr(), plan.out.data_ptr() + 4 * 4 * 3, "stream")
    assert calls[1][1] == want
    del calls[:]
    ops.adamw_ema(*bufs, *hyper, norms=plan, apply=False)
    assert calls == [(NAME, want)]
    del calls[:]
    plan.extra = bank.exp_avg_sq
    ops.adamw_ema(bank.flat, None, None, None, None, *hyper, norms=plan, apply=False)
    assert calls[0][1][:4] == (bank.flat.data_ptr(), None, None, bank.exp_avg_sq.data_ptr())
    with pytest.raises(AssertionError):         # a buffer of another length would be read past its end
        ops.adamw_ema(bank.flat[:-4], None, None, None, None, *hyper, norms=plan, apply=False)


def test_flag_is_off_by_default_and_documented():
    assert cli.EXTRA_DEFAULTS["log_norms"] is False
    base = ["--synthetic", "--train_unet"]
    assert cli.parse_args(base, with_extras=True).log_norms is False
    assert cli.parse_args(base + ["--log_norms"], with_extras=True).log_norms is True
    assert not hasattr(cli.parse_args([]), "log_norms"), "the reference's own surface does not have the flag"
    from finetune_fair_diffusion_amd import train
    assert "--log_norms" in cli.__doc__ and "--log_norms" in train.__doc__
    assert "--log_norms" in open(os.path.join(ROOT, "README.md")).read()


def test_json_fields_carry_the_reference_names_and_null_for_a_non_finite_value():
    from finetune_fair_diffusion_amd import train
    bank = layers.ParamBank({"x.down.weight": (2, 3), "x.up.weight": (3, 2)}, "cpu")
    plan = bank.norm_plan()
    host = [3.0, 1.0, 0.5, 0.25, 7.0, 9.0, 0.0, 0.0] + [2.0, 10.0 ** 0.5, 0.375, 0.3, 8.0, 11.0, 0.0, 0.0]     # norms [4, 2], then (mean, l2) x 4
    r = plan.report(host)
    assert r == dict(param_mean=2.0, param_l2=10.0 ** 0.5, ema_mean=0.375, ema_l2=0.3, grad_l2=11.0,
                     per_tensor={"x.down.weight": (3.0, 0.5, 7.0), "x.up.weight": (1.0, 0.25, 9.0)})
    bad = dict(r, grad_l2=math.inf)
    nan = dict(r, grad_l2=math.nan)
    fields = train.norm_log_fields({"unet_lora": r, "TE_lora": bad, "prefix_embedding": nan})
    assert fields == dict(train_unet_lora_norm=2.0, train_unet_lora_ema_norm=0.375, grad_norm_unet_lora=11.0,
                          train_TE_lora_norm=2.0, train_TE_lora_ema_norm=0.375, grad_norm_TE_lora=None,
                          train_prefix_embedding_norm=2.0, train_prefix_embedding_ema_norm=0.375, grad_norm_prefix_embedding=None)
    line = json.dumps(dict(step=1, **fields))
    assert '"grad_norm_TE_lora": null' in line and "Infinity" not in line and "NaN" not in line and json.loads(line)["grad_norm_unet_lora"] == 11.0
