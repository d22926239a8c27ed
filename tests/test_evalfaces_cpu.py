"""Host layer of the evaluator's face metrics (no GPU): the fp64 statement of the aligned chips from the bytes against the oracle's image pipeline,
``faces_summary`` on hand-made arrays, the flags, and the new C-ABI entry point with its refusals (they come before any launch)."""
import ctypes
import math
import os

import numpy as np
import pytest
import torch

from finetune_fair_diffusion_amd import evaluate_images as EI, lib
from finetune_fair_diffusion_amd.fairness import alignment_sampling_matrix

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
NAME = "fd_warp_affine_u8_fwd"
NAN = float("nan")


def _face(rng, size, angle, centre):
    from oracle import nn_sfnet as OS
    p = (OS.SRC_LANDMARKS - 56.0) / 112 * size
    c, s = math.cos(angle), math.sin(angle)
    return p @ np.array([[c, s], [-s, c]]) + np.array(centre) + rng.randn(5, 2) * 0.3


def test_host_statement_equals_the_oracle_image_pipeline():
    """Three rotated faces on 48x64 images (H != W), the last spilling over a corner: ``warp_affine_u8_host`` through ``alignment_sampling_matrix``
    against ``oracle.nn_sfnet.image_pipeline`` of ``u8/255*2-1``.  Both are fp64 / fp32 statements of one map: band 1e-5."""
    from oracle import nn_sfnet as OS
    H, W, S = 48, 64, 28
    rng = np.random.RandomState(11)
    u8 = rng.randint(0, 256, (2, H, W, 3)).astype(np.uint8)
    lms = [_face(rng, 30, 0.3, (30, 22)), _face(rng, 44, -0.6, (36, 26)), _face(rng, 36, 1.2, (60, 5))]
    src = [0, 1, 1]
    x = torch.from_numpy(u8).permute(0, 3, 1, 2).float() / 255 * 2 - 1
    ref = torch.stack([OS.image_pipeline(x[src[i]], lms[i], S) for i in range(3)]).double().numpy()
    A = np.stack([alignment_sampling_matrix(l, H, W, S) for l in lms])
    got = EI.warp_affine_u8_host(u8, src, A, S, -1.0)
    assert got.shape == (3, 3, S, S) and got.dtype == np.float64
    err = np.abs(got - ref).max()
    print(f"[warp_affine_u8_host vs image_pipeline] max abs err {err:.3e} (tol 1.0e-05)")
    assert err <= 1e-5
    assert (got[2] == -1).mean() > 0.05 and (got[0] != -1).all()
    # a source index outside [0, B) is a chip of the fill
    bad = EI.warp_affine_u8_host(u8, [-1, 2, 0], A, S, 0.25)
    assert (bad[:2] == 0.25).all() and np.array_equal(bad[2], EI.warp_affine_u8_host(u8, [0], A[2:], S, 0.25)[0])


def test_faces_summary_on_hand_made_arrays():
    t = lambda *v: torch.tensor(v, dtype=torch.float32)
    lm = {i: torch.zeros(4, 5, 2) for i in (0, 1, 2)}
    real = {0: t(0.5, NAN, 0.25, 0.25), 1: t(NAN, NAN, NAN, NAN), 2: t(-1.0, 0.0, 1.0, -1.0)}
    ori = {0: t(NAN, NAN, 0.75, 0.5), 1: t(NAN, NAN, NAN, NAN), 2: t(1.0, 1.0, NAN, 1.0)}
    numbers = {0: [0, 1, 2, 10], 1: [0, 1, 2, 3], 2: [4, 5, 6, 7]}
    got = EI.faces_summary([lm, real, ori], numbers)
    p = got["per_prompt"]
    assert sorted(p) == ["0", "1", "2"]
    assert p["0"] == dict(faces=3, sim_face_real=1.0 / 3, min_sim_face_real=0.25, argmin_face_real=2,           # a tie at the minimum: the first image number
                          pairs=2, sim_face_ori=0.625, min_sim_face_ori=0.5, argmin_face_ori=10)
    assert p["1"] == dict(faces=0, sim_face_real=None, min_sim_face_real=None, argmin_face_real=None,
                          pairs=0, sim_face_ori=None, min_sim_face_ori=None, argmin_face_ori=None)              # a prompt with no face at all
    assert p["2"] == dict(faces=4, sim_face_real=-0.25, min_sim_face_real=-1.0, argmin_face_real=4,              # -1 is a value here, not "no face"
                          pairs=3, sim_face_ori=1.0, min_sim_face_ori=1.0, argmin_face_ori=4)
    assert got["mean"] == dict(sim_face_real=(1.0 / 3 - 0.25) / 2, sim_face_ori=(0.625 + 1.0) / 2)               # prompt 1 has no row: it is left out
    # without originals: the third dict is empty and nothing about pairs is reported
    alone = EI.faces_summary([lm, real, {}], numbers)
    assert sorted(alone["per_prompt"]["0"]) == ["argmin_face_real", "faces", "min_sim_face_real", "sim_face_real"] and sorted(alone["mean"]) == ["sim_face_real"]
    assert alone["per_prompt"]["0"]["sim_face_real"] == p["0"]["sim_face_real"]
    # no prompt has a face
    none = EI.faces_summary([{1: lm[1]}, {1: real[1]}, {}], {1: numbers[1]})
    assert none["mean"] == dict(sim_face_real=None) and none["per_prompt"]["1"]["faces"] == 0


def test_flags_are_absent_unless_given():
    ns = EI.parse_args([])
    assert not any(hasattr(ns, k) for k in ("face_metrics", "opensphere_model_path", "face_feats_path")) and ns.size_aligned_face == 112
    ns = EI.parse_args(["--face_metrics", "--opensphere_model_path", "a.pth", "--face_feats_path", "b.pkl", "--size_aligned_face", "96"])
    assert ns.face_metrics is True and ns.opensphere_model_path == "a.pth" and ns.face_feats_path == "b.pkl" and ns.size_aligned_face == 96


def test_missing_face_weights_are_refused_before_anything_is_written(tmp_path):
    out = tmp_path / "out"
    args = EI.parse_args(["--face_metrics", "--generated_imgs_dir", str(tmp_path), "--save_dir", str(out), "--opensphere_model_path", str(tmp_path / "no.pth"),
                          "--face_feats_path", str(tmp_path / "no.pkl")])
    with pytest.raises(FileNotFoundError, match="--face_metrics.*--opensphere_model_path.*--face_feats_path"):
        EI.main(args, log=None)
    assert not out.exists()
    (tmp_path / "no.pth").write_bytes(b"")          # one of the two present: the other is still named
    with pytest.raises(FileNotFoundError, match="--face_feats_path") as e:
        EI.main(args, log=None)
    assert "--opensphere_model_path" not in str(e.value) and not out.exists()


def test_entry_point_is_declared_additively():
    protos = lib.parse_header()
    assert len(protos[NAME][1]) == 12 and lib.ABI_VERSION == 4
    assert list(protos)[-1] == "fd_eval_grid_labels_u8"
    names = list(protos)
    assert names.index(NAME) == names.index("fd_crop_resize_u8_fwd") + 1
    md = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    rows = [l for l in md.splitlines() if l.startswith("| `" + NAME + "`")]
    assert len(rows) == 1 and "12 arguments" in rows[0]
    pkg = os.path.dirname(lib.LIB_PATH)
    for so in ("libfairdiff_hip.so", "libfairdiff_hip_bf16.so"):
        path = os.path.join(pkg, so)
        if os.path.exists(path):
            assert getattr(ctypes.CDLL(path), NAME)


def test_entry_point_refuses_bad_arguments_before_any_launch():
    """Null pointers and sizes outside the range return -1 with a message naming the entry point; nothing is launched, so no device is needed."""
    path = os.path.join(os.path.dirname(lib.LIB_PATH), "libfairdiff_hip.so")
    if not os.path.exists(path):
        pytest.skip("the library is not built")
    L = ctypes.CDLL(path)
    fn = getattr(L, NAME)
    fn.restype, fn.argtypes = lib.parse_header()[NAME]
    L.fd_last_error.restype = ctypes.c_char_p
    buf = ctypes.create_string_buffer(64)           # host memory: never dereferenced by a refused call
    ok = ctypes.cast(buf, ctypes.c_void_p)
    good = dict(img=ok, src_index=ok, A=ok, chips=ok, mirror=None, n=1, B=1, H=8, W=8, S=8)

    def call(**kw):
        a = dict(good, **kw)
        return fn(a["img"], a["src_index"], a["A"], ctypes.c_float(-1.0), a["chips"], a["mirror"], a["n"], a["B"], a["H"], a["W"], a["S"], None)

    bad = [dict(img=None), dict(src_index=None), dict(A=None), dict(chips=None), dict(n=0), dict(n=-3), dict(B=0), dict(H=0), dict(H=4097), dict(W=0),
           dict(W=4097), dict(S=0), dict(S=4097)]
    for kw in bad:
        assert call(**kw) == -1 and NAME.encode() in L.fd_last_error(), kw
