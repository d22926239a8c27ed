"""The evaluator's semantics-preservation mode (``evaluate_images.main --original_imgs_dir``, ``pair_similarity``) on small paired trees of JPEGs
written here, against the fp32 oracle encoders applied to the fp32 statement of the resize.  TINY encoders (56 px, patch 14) with the evaluator's
own synthetic weights.

Bands: 2e-2 absolute against the oracle and 2e-3 between two launch forms of the same forward, the bands of
``test_vit_features_and_input_gradient_vs_oracle`` for this quantity (``check(f"{kind} loss", ..., 2e-2)``, ``"embedding (no record)"``, 2e-3)."""
import json
import os
import pickle

import numpy as np
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

S_FACE = 64
ALPHAS = (0, 0.05, 0.2, 0.5, 1.0)
NUMBERS = (0, 1, 2, 3, 10)
BOXES = [[8, 6, 50, 48], [-7, 5, 35, 47], [20, 20, 70, 70], None, [0, 0, 64, 64],
         [10, 12, 40, 42], [5, 30, 45, 70], [30, 2, 62, 34], [16, 16, 48, 48], [-10, -10, 74, 74]]
BAND_ORACLE, BAND_LAUNCH_FORM = 2e-2, 2e-3


class ScriptedProvider:
    """Boxes by running image number, whatever the batch size."""

    def __init__(self):
        self.seen = 0

    def __call__(self, images):
        bb = [BOXES[(self.seen + i) % len(BOXES)] for i in range(images.shape[0])]
        self.seen += images.shape[0]
        return torch.tensor([b is not None for b in bb]), torch.tensor([b if b is not None else [-1] * 4 for b in bb], dtype=torch.int32)


@pytest.fixture(scope="module")
def EI():
    from finetune_fair_diffusion_amd import evaluate_images
    return evaluate_images


@pytest.fixture(scope="module")
def TINY():
    from finetune_fair_diffusion_amd.factory import TINY
    return TINY


def _save(arr, path):
    from PIL import Image
    Image.fromarray(arr).save(str(path))
    return np.asarray(Image.open(str(path)).convert("RGB"))


def _blocks(rng, block):
    return np.kron(rng.randint(0, 256, (8, 8, 3)).astype(np.uint8), np.ones((block, block, 1), dtype=np.uint8))


def _blend(a, o, alpha):
    return np.clip((1 - alpha) * a.astype(np.float64) + alpha * o.astype(np.float64) + 0.5, 0, 255).astype(np.uint8)


@pytest.fixture(scope="module")
def trees(tmp_path_factory):
    """Two prompts of five 64x64 pairs: the original is ``a``, the generated image is ``a`` blended with an unrelated ``o`` by alpha = 0 .. 1.
    Returns (generated dir, original dir, decoded generated [10,64,64,3], decoded originals [10,64,64,3])."""
    gen, ori = tmp_path_factory.mktemp("generated"), tmp_path_factory.mktemp("original")
    rng = np.random.RandomState(5)
    dg, do = [], []
    for p in range(2):
        (gen / f"prompt_{p}").mkdir()
        (ori / f"prompt_{p}").mkdir()
        for alpha, j in zip(ALPHAS, NUMBERS):
            a = _blocks(rng, 8)
            o = _blocks(rng, 8)
            do.append(_save(a, ori / f"prompt_{p}" / f"img_{j}.jpg"))
            dg.append(_save(_blend(a, o, alpha), gen / f"prompt_{p}" / f"img_{j}.jpg"))
    return str(gen), str(ori), torch.from_numpy(np.stack(dg)), torch.from_numpy(np.stack(do))


@pytest.fixture(scope="module")
def oracle(EI, TINY):
    """(u8_gen, u8_ori: CPU uint8 [n,H,W,3], sizes may differ) -> [2, n] fp32: the oracle encoders' cosine of each pair, CLIP then DINOv2."""
    from finetune_fair_diffusion_amd import weights as W
    from oracle import nn_vit as OV
    models = []
    for k, (key, mean, std) in enumerate((("clip_vision", W.CLIP_IMAGE_MEAN, W.CLIP_IMAGE_STD), ("dino", W.DINO_IMAGE_MEAN, W.DINO_IMAGE_STD))):
        cfg = TINY[key]
        assert cfg.image_size == 56 and cfg.patch_size == 14
        models.append((OV.build(OV.ViTConfig(**cfg.__dict__), EI.synthetic_vit_state(k, TINY)), mean, std))

    def feats(u8, m, mean, std):
        x = F.interpolate(u8.permute(0, 3, 1, 2).float() / 255 * 2 - 1, size=56, mode="bilinear", align_corners=False)
        with torch.no_grad():
            return OV.image_features(m, x, mean, std, normalize=True)

    def sims(u8_gen, u8_ori):
        return torch.stack([(feats(u8_gen, *m) * feats(u8_ori, *m)).sum(-1) for m in models]).float()
    return sims


@pytest.fixture(scope="module")
def oracle_sims(oracle, trees):
    return oracle(trees[2], trees[3])             # [2, 10], computed once


def _run(EI, TINY, gen, save_dir, batch_size, ori=None, grid="off"):
    argv = ["--synthetic", "--generated_imgs_dir", gen, "--save_dir", str(save_dir), "--batch_size", str(batch_size), "--size_face", str(S_FACE), "--grid", grid]
    if ori is not None:
        argv += ["--original_imgs_dir", ori]
    lines = []
    EI.main(EI.parse_args(argv), face_provider=ScriptedProvider(), log=lines.append, cfgs=TINY)
    return lines


def _load(save_dir, name):
    with open(os.path.join(str(save_dir), name), "rb") as f:
        return pickle.load(f)


@pytest.fixture(scope="module")
def run4(EI, TINY, trees, tmp_path_factory, dev):
    d = tmp_path_factory.mktemp("semantics4")
    lines = _run(EI, TINY, trees[0], d, 4, ori=trees[1])
    return d, _load(d, "semantics.pkl"), lines


def _stacked(sem, prompts=(0, 1)):
    return torch.stack([torch.cat([sem[k][p] for p in prompts]) for k in range(2)])


def test_end_to_end_against_the_oracle(EI, run4, oracle_sims):
    """Measured on an MI355X (max |product - oracle| over the 10 pairs, band 2e-2): CLIP 5.1e-5, DINOv2 9.2e-5; sim = 1 exactly at alpha = 0."""
    d, sem, lines = run4
    ref = oracle_sims
    # conditions on the oracle alone: the pairs span "identical" to "clearly different", so the comparison below is not passed on nothing
    for k, name in enumerate(("CLIP", "DINO")):
        for p in range(2):
            r = ref[k, 5 * p:5 * p + 5]
            print(f"[semantics oracle, {name}, prompt {p}] " + " ".join(f"{float(v):.4f}" for v in r))
            assert float(r[0]) >= 1 - 1e-6 and float(r[4]) < 0.95, (name, p, r.tolist())
            # the steps alpha 0 -> 0.5 -> 1 are wider than the band (the smallest is 0.0222, DINOv2, prompt 1): the order asserted below is resolvable
            assert float(r[0] - r[3]) > BAND_ORACLE and float(r[3] - r[4]) > BAND_ORACLE, (name, p, r.tolist())
    assert isinstance(sem, list) and len(sem) == 2 and all(sorted(s) == [0, 1] for s in sem)
    for s in sem:
        for t in s.values():
            assert t.dtype == torch.float32 and tuple(t.shape) == (5,) and not t.is_cuda
    got = _stacked(sem)
    err = (got - ref).abs()
    for k, name in enumerate(("CLIP", "DINO")):
        print(f"[semantics vs oracle, {name}] max abs err {float(err[k].max()):.3e} (band {BAND_ORACLE:.1e})  at alpha=0: 1 - sim max {float((1 - got[k, ::5]).abs().max()):.3e}")
    assert torch.isfinite(got).all() and float(err.max()) <= BAND_ORACLE, err.tolist()
    for k in range(2):
        for p in range(2):
            s = got[k, 5 * p:5 * p + 5]
            assert float(s[0]) > float(s[3]) > float(s[4]), (k, p, s.tolist())                # alpha 0, 0.5, 1
            assert abs(float(s[0]) - 1) <= 1e-5, (k, p, float(s[0]))                              # the same bytes on both sides
    js = json.load(open(os.path.join(str(d), "semantics.json")))
    assert js == EI.semantics_summary(sem, {0: list(NUMBERS), 1: list(NUMBERS)})
    assert js["per_prompt"]["0"]["argmin_CLIP"] == 10 and js["per_prompt"]["1"]["argmin_DINO"] == 10 and js["per_prompt"]["0"]["pairs"] == 5
    assert json.loads(lines[-1])["semantics_pairs"] == 10 and json.loads(lines[-1])["evaluated_images"] == 10


def test_nothing_else_moves(EI, TINY, trees, run4, tmp_path):
    d, _, _ = run4
    lines = _run(EI, TINY, trees[0], tmp_path, 4)
    assert open(os.path.join(str(d), "metrics.json"), "rb").read() == open(os.path.join(str(tmp_path), "metrics.json"), "rb").read()
    assert sorted(json.load(open(os.path.join(str(d), "metrics.json")))) == ["mean", "per_prompt"]
    with_flag, without = _load(d, "test_results.pkl"), _load(tmp_path, "test_results.pkl")
    assert len(with_flag) == len(without) == 5
    for a, b in zip(with_flag, without):
        assert sorted(a) == sorted(b) == [0, 1]
        for p in a:
            assert a[p].dtype == b[p].dtype and torch.equal(a[p], b[p])
    assert sorted(os.listdir(str(tmp_path))) == ["metrics.json", "test_results.pkl"]
    assert sorted(os.listdir(str(d))) == ["metrics.json", "semantics.json", "semantics.pkl", "test_results.pkl"]
    assert "semantics_pairs" not in json.loads(lines[-1])
    assert sorted(json.loads(lines[-1])) == ["evaluated_images", "images_per_s", "prompts", "seconds"]


def test_batch_size_one_gives_the_same_similarities(EI, TINY, trees, run4, tmp_path):
    _run(EI, TINY, trees[0], tmp_path, 1, ori=trees[1])
    e = float((_stacked(_load(tmp_path, "semantics.pkl")) - _stacked(run4[1])).abs().max())
    print(f"[semantics, batch size 1 vs 4] max abs diff {e:.3e} (band {BAND_LAUNCH_FORM:.1e})")
    assert np.isfinite(e) and e <= BAND_LAUNCH_FORM


def test_trees_of_different_sizes(EI, TINY, oracle, tmp_path, dev):
    rng = np.random.RandomState(6)
    (tmp_path / "gen" / "prompt_0").mkdir(parents=True)
    (tmp_path / "ori" / "prompt_0").mkdir(parents=True)
    dg, do = [], []
    for j, alpha in enumerate((0.0, 0.3, 1.0)):
        a, o = rng.randint(0, 256, (8, 8, 3)).astype(np.uint8), rng.randint(0, 256, (8, 8, 3)).astype(np.uint8)
        do.append(_save(np.kron(a, np.ones((10, 10, 1), dtype=np.uint8)), tmp_path / "ori" / "prompt_0" / f"img_{j}.jpg"))                  # 80x80
        dg.append(_save(np.kron(_blend(a, o, alpha), np.ones((8, 8, 1), dtype=np.uint8)), tmp_path / "gen" / "prompt_0" / f"img_{j}.jpg"))  # 64x64
    assert do[0].shape == (80, 80, 3) and dg[0].shape == (64, 64, 3)
    _run(EI, TINY, str(tmp_path / "gen"), tmp_path / "out", 2, ori=str(tmp_path / "ori"))
    got = _stacked(_load(tmp_path / "out", "semantics.pkl"), prompts=(0,))
    ref = oracle(torch.from_numpy(np.stack(dg)), torch.from_numpy(np.stack(do)))
    e = float((got - ref).abs().max())
    print(f"[semantics, 64x64 against 80x80] max abs err {e:.3e} (band {BAND_ORACLE:.1e})  oracle {ref.tolist()}")
    assert float(ref[:, 0].min()) > float(ref[:, 2].max())          # the pairs are not all alike
    assert tuple(got.shape) == (2, 3) and np.isfinite(e) and e <= BAND_ORACLE


@pytest.mark.parametrize("n", [1, 7])
def test_pair_similarity_against_the_oracle(EI, TINY, oracle, dev, n):
    """n = 1: the smallest batch; n = 7: 2 * 7 * 24 = 336 token rows, no multiple of the GEMM tiles."""
    from finetune_fair_diffusion_amd import weights as W
    from finetune_fair_diffusion_amd.vit import VisionTransformer
    clip = VisionTransformer(TINY["clip_vision"], EI.synthetic_vit_state(0, TINY), dev, W.CLIP_IMAGE_MEAN, W.CLIP_IMAGE_STD)
    dino = VisionTransformer(TINY["dino"], EI.synthetic_vit_state(1, TINY), dev, W.DINO_IMAGE_MEAN, W.DINO_IMAGE_STD)
    rng = np.random.RandomState(7 + n)
    ori = np.stack([_blocks(rng, 8) for _ in range(n)])
    other = np.stack([_blocks(rng, 8) for _ in range(n)])
    gen = np.stack([_blend(ori[i], other[i], i / max(n - 1, 1) if n > 1 else 0.5) for i in range(n)])
    ug, uo = torch.from_numpy(gen), torch.from_numpy(ori)
    sc, sd = EI.pair_similarity(clip, dino, ug.to(dev), uo.to(dev))
    for s in (sc, sd):
        assert s.is_cuda and s.dtype == torch.float32 and tuple(s.shape) == (n,)
    ref = oracle(ug, uo)
    e = float((torch.stack([sc, sd]).cpu() - ref).abs().max())
    print(f"[pair_similarity, n={n}] max abs err {e:.3e} (band {BAND_ORACLE:.1e})  oracle min {float(ref.min()):.4f} max {float(ref.max()):.4f}")
    assert float(ref.min()) < 0.98                                  # not all pairs alike
    assert np.isfinite(e) and e <= BAND_ORACLE


def test_a_missing_counterpart_is_refused_before_anything_is_written(EI, TINY, tmp_path, dev):
    for root, numbers in (("gen", (0, 1, 2)), ("ori", (0, 2))):
        (tmp_path / root / "prompt_0").mkdir(parents=True)
        for j in numbers:
            (tmp_path / root / "prompt_0" / f"img_{j}.jpg").write_bytes(b"")
    out = tmp_path / "out"
    with pytest.raises(ValueError) as e:
        _run(EI, TINY, str(tmp_path / "gen"), out, 4, ori=str(tmp_path / "ori"))
    assert str(tmp_path / "ori" / "prompt_0" / "img_1.jpg") in str(e.value)
    assert not os.path.exists(os.path.join(str(out), "test_results.pkl")) and not os.path.exists(str(out))


def test_real_weights_need_both_environment_variables(EI, TINY, trees, tmp_path, dev, monkeypatch):
    monkeypatch.delenv("FD_CLIP_VISION_DIR", raising=False)
    monkeypatch.delenv("FD_DINO_WEIGHTS", raising=False)
    args = EI.parse_args(["--generated_imgs_dir", trees[0], "--original_imgs_dir", trees[1], "--save_dir", str(tmp_path / "out")])
    with pytest.raises(FileNotFoundError) as e:
        EI.main(args, face_provider=ScriptedProvider(), log=None, cfgs=TINY)
    assert "FD_CLIP_VISION_DIR" in str(e.value) and "FD_DINO_WEIGHTS" in str(e.value)
    monkeypatch.setenv("FD_CLIP_VISION_DIR", str(tmp_path))          # one of the two is not enough
    with pytest.raises(FileNotFoundError) as e:
        EI.main(args, face_provider=ScriptedProvider(), log=None, cfgs=TINY)
    assert "FD_CLIP_VISION_DIR" in str(e.value) and "FD_DINO_WEIGHTS" in str(e.value)
    assert not os.path.exists(str(tmp_path / "out"))
