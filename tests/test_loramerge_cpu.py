"""Host layer of the LoRA fold (no GPU): the key mapping of merge.py over the real and the tiny inventories, its refusals by name, the CLI's refusals
(all before ``save_dir`` exists), what ``layers.refresh_pairs`` launches with and without ``merge=`` (``ops._call`` replaced by a recorder), the
descriptor in the header / lib.py / INTEGRATION.md, and the entry point's own refusals with host memory standing in for the buffers."""
import ctypes
import os
import re
import subprocess

import pytest
import torch

from finetune_fair_diffusion_amd import generate, layers, lib, merge, weights as W
from finetune_fair_diffusion_amd.factory import SD15, TINY

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAME = "fd_lora_merge_multi"


# ------------------------------------------------------------------------------------------ key mapping
@pytest.mark.parametrize("cfgs, rank, n_unet, n_te", [(SD15, 50, 128, 72), (TINY, 4, 128, 12)], ids=["SD-v1.5 rank 50", "TINY rank 4"])
def test_every_pair_maps_onto_a_base_matrix_of_its_shape(cfgs, rank, n_unet, n_te):
    for kind, lora_shapes, base_shapes, count in (("unet", W.unet_lora_param_shapes(cfgs["unet"], rank), W.unet_param_shapes(cfgs["unet"]), n_unet),
                                                  ("text_encoder", W.clip_lora_param_shapes(cfgs["clip"], rank), W.clip_param_shapes(cfgs["clip"]), n_te)):
        triples = merge.lora_targets(kind, cfgs["unet"] if kind == "unet" else cfgs["clip"])
        assert len(triples) == count and len(lora_shapes) == 2 * count
        assert [k for dn, un, _ in triples for k in (dn, un)] == list(lora_shapes), "the pairs come in the order of the LoRA inventory"
        assert len({bk for _, _, bk in triples}) == count, "no two pairs share a target"
        for dn, un, bk in triples:
            (r, K), (N, r2) = lora_shapes[dn], lora_shapes[un]
            assert r == r2 == rank and bk in base_shapes and tuple(base_shapes[bk]) == (N, K), (dn, bk)
    with pytest.raises(ValueError, match="kind"):
        merge.lora_targets("vae", cfgs["vae"])


def _tiny_te():
    cfg = TINY["clip"]
    base = W.synthetic_state_dict(W.clip_param_shapes(cfg), seed=3)
    lora = W.synthetic_state_dict(W.clip_lora_param_shapes(cfg, 4), seed=6)
    return cfg, base, lora


def test_check_pairs_reads_the_rank_from_the_file_and_refuses_by_name():
    cfg, base, lora = _tiny_te()
    triples = merge.check_pairs(base, lora, "text_encoder", cfg)
    assert len(triples) == 12
    wide = W.synthetic_state_dict(W.clip_lora_param_shapes(cfg, 50), seed=6)          # another rank: nothing but the file says so
    assert merge.check_pairs(base, wide, "text_encoder", cfg) == triples
    dn, un, bk = triples[7]
    with pytest.raises(KeyError, match=re.escape(dn) + " has no twin " + re.escape(un)):
        merge.check_pairs(base, {k: v for k, v in lora.items() if k != un}, "text_encoder", cfg)
    with pytest.raises(KeyError, match=re.escape(un) + " has no twin " + re.escape(dn)):
        merge.check_pairs(base, {k: v for k, v in lora.items() if k != dn}, "text_encoder", cfg)
    with pytest.raises(KeyError, match="pair " + re.escape(dn) + ".*missing"):
        merge.check_pairs(base, {k: v for k, v in lora.items() if k not in (dn, un)}, "text_encoder", cfg)
    with pytest.raises(KeyError, match="stranger.weight is not a LoRA tensor"):
        merge.check_pairs(base, dict(lora, **{"stranger.weight": torch.zeros(1)}), "text_encoder", cfg)
    with pytest.raises(KeyError, match="no " + re.escape(bk)):
        merge.check_pairs({k: v for k, v in base.items() if k != bk}, lora, "text_encoder", cfg)
    with pytest.raises(ValueError, match=re.escape(bk) + " has shape"):
        merge.check_pairs(dict(base, **{bk: torch.zeros(3, 5)}), lora, "text_encoder", cfg)
    with pytest.raises(ValueError, match="not a .* pair"):
        merge.check_pairs(base, dict(lora, **{un: torch.zeros(lora[un].shape[0], 5)}), "text_encoder", cfg)
    with pytest.raises(ValueError, match="rank 65"):
        merge.check_pairs(base, W.synthetic_state_dict(W.clip_lora_param_shapes(cfg, 65), seed=6), "text_encoder", cfg)
    with pytest.raises(RuntimeError, match="HIP device"):           # after the checks, before any device work
        merge.merge_state_dict(base, lora, "text_encoder", cfg, "cpu")


# ------------------------------------------------------------------------------------------ the CLI's refusals
def _tiny_te_dir(tmp_path):
    """A directory with a tiny text encoder only (the U-Net is not read when no U-Net LoRA file is given) and its LoRA file."""
    from safetensors.torch import save_file
    cfg, base, lora = _tiny_te()
    d = tmp_path / "model"
    (d / "text_encoder").mkdir(parents=True)
    save_file(base, str(d / "text_encoder" / "model.safetensors"))
    (d / "model_index.json").write_text("{}")
    torch.save(lora, tmp_path / "te_lora.pth")
    return d, tmp_path / "te_lora.pth", lora


def test_cli_refuses_before_save_dir_exists(tmp_path, monkeypatch):
    d, lora_path, lora = _tiny_te_dir(tmp_path)
    out = tmp_path / "out"
    common = ["--pretrained_model_name_or_path", str(d), "--save_dir", str(out)]
    te = ["--load_text_encoder_lora_from", str(lora_path)]

    def refused(argv, exc, word):
        with pytest.raises(exc, match=word):
            merge.main(merge.parse_args(argv), cfgs=TINY)
        assert not out.exists(), f"{word}: save_dir was created"

    refused(common, ValueError, "nothing to merge")
    refused(common + ["--load_text_encoder_lora_from", str(tmp_path / "absent.pth")], FileNotFoundError, "absent.pth")
    refused(["--pretrained_model_name_or_path", str(tmp_path / "nowhere"), "--save_dir", str(out)] + te, FileNotFoundError, "nowhere")
    refused(common + ["--load_unet_lora_from", str(lora_path)], FileNotFoundError, "diffusion_pytorch_model")      # DIR/unet has no weights file
    k = next(iter(lora))
    torch.save({n: v for n, v in lora.items() if n != k}, tmp_path / "half.pth")
    refused(common + ["--load_text_encoder_lora_from", str(tmp_path / "half.pth")], KeyError, "has no twin")
    torch.save(dict(lora, **{k: torch.zeros(4, 7)}), tmp_path / "shape.pth")
    refused(common + ["--load_text_encoder_lora_from", str(tmp_path / "shape.pth")], ValueError, "has shape")
    monkeypatch.setattr(torch.cuda, "is_available", lambda: False)
    refused(common + te, RuntimeError, "HIP device")
    # a save_dir that holds something is refused and left as it is; an empty one is no obstacle (the next refusal is then the device's)
    out.mkdir()
    with pytest.raises(RuntimeError, match="HIP device"):
        merge.main(merge.parse_args(common + te), cfgs=TINY)
    (out / "keep.txt").write_text("mine")
    with pytest.raises(FileExistsError, match="not empty"):
        merge.main(merge.parse_args(common + te), cfgs=TINY)
    assert sorted(os.listdir(out)) == ["keep.txt"]


def test_cli_flags_mirror_generate():
    a = merge.parse_args(["--pretrained_model_name_or_path", "m", "--save_dir", "o"])
    assert (a.load_unet_lora_from, a.load_text_encoder_lora_from, a.lora_scale, a.gpu_id) == (None, None, 1.0, 0)
    g = generate.parse_args(["--prompts_path", "p", "--save_dir", "o"])
    for flag in ("pretrained_model_name_or_path", "save_dir", "load_unet_lora_from", "load_text_encoder_lora_from", "gpu_id"):
        assert hasattr(g, flag) and hasattr(a, flag)
    assert g.merge_lora is False and generate.parse_args(["--prompts_path", "p", "--save_dir", "o", "--merge_lora"]).merge_lora is True


def test_generate_refuses_merge_lora_without_a_lora_file(tmp_path):
    with pytest.raises(ValueError, match="--merge_lora needs"):
        generate.main(generate.parse_args(["--synthetic", "--prompts_path", str(tmp_path / "p.json"), "--save_dir", str(tmp_path / "o"), "--merge_lora"]), cfgs=TINY)
    assert not (tmp_path / "o").exists()


# ------------------------------------------------------------------------------------------ what refresh_pairs launches
@pytest.fixture()
def rec(monkeypatch):
    """``ops`` with every device touch replaced (the method of tests/test_banknorms_cpu.py): _call records (name, a copy of the descriptor bytes, n)."""
    from finetune_fair_diffusion_amd import ops
    calls = []
    monkeypatch.setattr(ops, "_call", lambda name, arr, n, stream: calls.append((name, bytes(arr._obj), n, stream)))
    monkeypatch.setattr(ops, "_stream", lambda: "stream")
    return calls


def _bank():
    bank = layers.ParamBank({"a.down.weight": (4, 24), "a.up.weight": (40, 4), "b.down.weight": (50, 8), "b.up.weight": (16, 50)}, "cpu")
    return bank, [layers.LoRAPair(bank, "a.down.weight", "a.up.weight"), layers.LoRAPair(bank, "b.down.weight", "b.up.weight")]


def test_refresh_pairs_without_the_keyword_builds_the_descriptors_it_always_built(rec):
    bank, pairs = _bank()
    for ema in (False, True):
        del rec[:]
        layers.refresh_pairs(pairs, 0.5, ema=ema)
        want = lib.LoraRefreshDesc.array(2)
        for d, p in zip(want, pairs):
            buf = bank.ema if ema else bank.flat
            off_d, off_u = bank.offsets[p.dn][0], bank.offsets[p.un][0]
            d.down, d.up = buf.data_ptr() + 4 * off_d, buf.data_ptr() + 4 * off_u
            d.d16, d.ld_d16, d.dT16, d.ld_dT16 = p.down16.data_ptr(), p.K, p.downT16.data_ptr(), p.rp
            d.u16, d.ld_u16, d.uT16, d.ld_uT16 = p.up16.data_ptr(), p.rp, p.upT16.data_ptr(), p.N
            d.r, d.rp, d.K, d.N, d.scale = p.r, p.rp, p.K, p.N, 0.5
        assert rec == [("fd_lora_refresh_multi", bytes(want), 2, "stream")]
    assert [(p.r, p.rp) for p in pairs] == [(4, 8), (50, 64)]
    del rec[:]
    layers.refresh_pairs([])
    assert rec == []


def test_refresh_pairs_with_merge_launches_the_fold_instead_of_the_slab_refresh(rec):
    bank, pairs = _bank()
    base = [torch.zeros(p.N, p.K) for p in pairs]
    out = [torch.zeros(p.N, p.K) for p in pairs]
    for ema in (False, True):
        del rec[:]
        layers.refresh_pairs(pairs, -2.0, ema=ema, merge=[(base[0], base[0]), (base[1], out[1])])
        want = lib.LoraMergeDesc.array(2)
        for d, p, b, o in zip(want, pairs, base, (base[0], out[1])):
            buf = bank.ema if ema else bank.flat
            d.down, d.up = buf.data_ptr() + 4 * bank.offsets[p.dn][0], buf.data_ptr() + 4 * bank.offsets[p.un][0]
            d.base, d.out, d.r, d.K, d.N, d.scale = b.data_ptr(), o.data_ptr(), p.r, p.K, p.N, -2.0
        assert rec == [(NAME, bytes(want), 2, "stream")]
    assert all(p.down16 is None for p in pairs), "a folded pair gets no 16-bit slab"
    with pytest.raises(AssertionError):
        layers.refresh_pairs(pairs, merge=[(base[0], base[0])])                     # one entry per pair
    with pytest.raises(AssertionError):
        layers.refresh_pairs(pairs, merge=[(base[0], base[0]), (base[1].t(), out[1])])
    with pytest.raises(AssertionError):
        layers.refresh_pairs(pairs, merge=[(base[0].double(), base[0].double()), (base[1], out[1])])


# ------------------------------------------------------------------------------------------ header, mirror, library
def _header_fields(name):
    src = re.sub(r"/\*.*?\*/", " ", open(lib.HEADER_PATH).read(), flags=re.S)
    body = re.search(r"typedef struct %s \{(.*?)\} %s;" % (name, name), src, flags=re.S).group(1)
    out = []
    for decl in body.split(";"):
        decl = " ".join(decl.split())
        if not decl:
            continue
        if "*" in decl:
            out.append((decl.split("*")[-1].strip(), ctypes.c_void_p))
        else:
            t, rest = decl.split(" ", 1)
            out += [(n.strip(), {"int32_t": ctypes.c_int32, "int64_t": ctypes.c_int64, "float": ctypes.c_float}[t]) for n in rest.split(",")]
    return out


def test_descriptor_is_mirrored_and_the_entry_point_is_additive(tmp_path):
    protos = lib.parse_header()
    assert NAME in protos and lib.ABI_VERSION == 4
    assert protos[NAME] == (ctypes.c_int, [ctypes.c_void_p, ctypes.c_int, ctypes.c_void_p])
    assert "#define FD_ABI_VERSION 4" in " ".join(open(lib.HEADER_PATH).read().split())
    assert lib.LoraMergeDesc._fields_ == _header_fields("fd_lora_merge_desc") and lib.LoraMergeDesc._fields_[0] == ("struct_size", ctypes.c_int32)
    arr = lib.LoraMergeDesc.array(3)
    assert [d.struct_size for d in arr] == [ctypes.sizeof(lib.LoraMergeDesc)] * 3
    prog = ['#include <stdio.h>', '#include <stddef.h>', '#include "fairdiff_hip.h"', 'int main(void) {', 'printf("size %zu\\n", sizeof(fd_lora_merge_desc));']
    prog += ['printf("%s %%zu\\n", offsetof(fd_lora_merge_desc, %s));' % (f, f) for f, _ in lib.LoraMergeDesc._fields_] + ['return 0; }']
    (tmp_path / "layout.c").write_text("\n".join(prog))
    subprocess.run(["gcc", "-I", os.path.join(ROOT, "include"), str(tmp_path / "layout.c"), "-o", str(tmp_path / "layout")], check=True)
    got = dict(line.rsplit(" ", 1) for line in subprocess.run([str(tmp_path / "layout")], check=True, capture_output=True, text=True).stdout.splitlines())
    assert int(got["size"]) == ctypes.sizeof(lib.LoraMergeDesc)
    for f, _ in lib.LoraMergeDesc._fields_:
        assert int(got[f]) == getattr(lib.LoraMergeDesc, f).offset, f
    md = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    assert len([l for l in md.splitlines() if l.startswith("| `" + NAME + "`")]) == 1 and "fd_lora_merge_desc" in md
    for f, _ in lib.LoraMergeDesc._fields_:
        assert "`%s`" % f in [l for l in md.splitlines() if l.startswith("| `" + NAME + "`")][0], f"INTEGRATION.md's row does not name the field {f}"
    pkg = os.path.dirname(lib.LIB_PATH)
    for so in ("libfairdiff_hip.so", "libfairdiff_hip_bf16.so"):
        assert os.path.exists(os.path.join(pkg, so)), so + " missing: run __graft_entry__.build()"
        assert getattr(ctypes.CDLL(os.path.join(pkg, so)), NAME)


def test_entry_point_refuses_on_the_host_before_any_launch():
    """Refused calls return non-zero with a message naming the entry point and launch nothing, so host memory stands in for the buffers."""
    L = ctypes.CDLL(os.path.join(os.path.dirname(lib.LIB_PATH), "libfairdiff_hip.so"))
    fn = getattr(L, NAME)
    fn.restype, fn.argtypes = lib.parse_header()[NAME]
    L.fd_last_error.restype = ctypes.c_char_p
    r, N, K = 4, 6, 10
    raw = ctypes.create_string_buffer(4 * (r * K + N * r + 2 * N * K) + 64)
    p0 = (ctypes.addressof(raw) + 15) // 16 * 16
    good = dict(down=p0, up=p0 + 4 * r * K, base=p0 + 4 * (r * K + N * r), out=p0 + 4 * (r * K + N * r + N * K), r=r, K=K, N=N, scale=1.0)

    def call(n=2, **kw):
        arr = lib.LoraMergeDesc.array(2)
        for k, v in good.items():
            setattr(arr[0], k, v)
        for k, v in dict(good, N=0).items():           # an empty second pair (the same tensors: nothing of it is read or written)
            setattr(arr[1], k, v)
        for k, v in kw.items():
            setattr(arr[0], k, v)
        return fn(ctypes.byref(arr), n, None)

    for kw, word in ((dict(struct_size=0), b"struct_size"), (dict(struct_size=ctypes.sizeof(lib.LoraMergeDesc) + 8), b"struct_size"),
                     (dict(down=None), b"null"), (dict(up=None), b"null"), (dict(base=None), b"null"), (dict(out=None), b"null"),
                     (dict(up=good["up"] + 1), b"aligned to 4"), (dict(r=0), b"rank must be in 1..64"), (dict(r=65), b"rank must be in 1..64"),
                     (dict(N=-1), b"extent"), (dict(K=-1), b"extent"),
                     (dict(out=good["base"] + 4), b"overlaps base"), (dict(out=good["base"] - 4), b"overlaps"),
                     (dict(out=good["down"]), b"overlaps"), (dict(out=good["up"]), b"overlaps"), (dict(n=0), b"no pairs")):
        assert call(**kw) != 0 and NAME.encode() in L.fd_last_error() and word in L.fd_last_error(), (kw, L.fd_last_error())
    assert fn(None, 1, None) != 0 and b"no pairs" in L.fd_last_error()
