"""The offline evaluator end to end (evaluate_images.main) on a small tree of JPEGs written here: the reference's pickle, the grids, metrics.json, and
batch-size independence.  The classifiers' logits are compared with the fp32 oracle applied to the fp32 statement of the face chips."""
import json
import math
import os
import pickle

import numpy as np
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

S_FACE = 64
BOXES = [[8, 6, 50, 48], [-7, 5, 35, 47], [20, 20, 70, 70], None, [0, 0, 64, 64],
         [10, 12, 40, 42], [5, 30, 45, 70], [30, 2, 62, 34], [16, 16, 48, 48], [-10, -10, 74, 74]]      # image 3 of prompt 0 has no face


class ScriptedProvider:
    """Boxes by running image number, whatever the batch size; records what it was handed."""

    def __init__(self):
        self.seen, self.inputs = 0, []

    def __call__(self, images):
        self.inputs.append(images)
        bb = BOXES[self.seen:self.seen + images.shape[0]]
        self.seen += images.shape[0]
        return torch.tensor([b is not None for b in bb]), torch.tensor([b if b is not None else [-1] * 4 for b in bb], dtype=torch.int32)


@pytest.fixture(scope="module")
def EI():
    from finetune_fair_diffusion_amd import evaluate_images
    return evaluate_images


@pytest.fixture(scope="module")
def tree(tmp_path_factory):
    """prompt_0, prompt_1 with five 64x64 JPEGs each (img_10 sorts after img_2 numerically); returns (dir, decoded uint8 [10,64,64,3])."""
    from PIL import Image
    root = tmp_path_factory.mktemp("generated")
    rng = np.random.RandomState(5)
    decoded = []
    for p in range(2):
        d = root / f"prompt_{p}"
        d.mkdir()
        for j in (0, 1, 2, 3, 10):
            blocks = rng.randint(0, 256, (8, 8, 3)).astype(np.uint8)
            path = str(d / f"img_{j}.jpg")
            Image.fromarray(np.kron(blocks, np.ones((8, 8, 1), dtype=np.uint8))).save(path)
            decoded.append(np.asarray(Image.open(path).convert("RGB")))
    return str(root), torch.from_numpy(np.stack(decoded))


def _run(EI, tree, save_dir, batch_size, grid="gender_race"):
    prov = ScriptedProvider()
    args = EI.parse_args(["--synthetic", "--generated_imgs_dir", tree[0], "--save_dir", str(save_dir), "--batch_size", str(batch_size),
                          "--size_face", str(S_FACE), "--grid", grid])
    lines = []
    EI.main(args, face_provider=prov, log=lines.append)
    with open(os.path.join(str(save_dir), "test_results.pkl"), "rb") as f:
        return pickle.load(f), prov, lines


@pytest.fixture(scope="module")
def run4(EI, tree, tmp_path_factory, dev):
    d = tmp_path_factory.mktemp("results4")
    return (d,) + _run(EI, tree, d, 4)


def _relerr(a, b):
    return float((a.float() - b.float()).abs().max() / (b.float().abs().max() + 1e-20))


def test_pickle_layout_and_logits_against_the_oracle(EI, tree, run4):
    from oracle import nn_mobilenet
    _, res, prov, _ = run4
    u8 = tree[1]
    x = u8.permute(0, 3, 1, 2).float() / 255 * 2 - 1
    assert isinstance(res, list) and len(res) == 5 and all(sorted(d) == [0, 1] for d in res)
    # the provider saw the reference's fp32 CPU tensor, four images at a time within a prompt
    assert [t.shape[0] for t in prov.inputs] == [4, 1, 4, 1] and all(t.dtype == torch.float32 and not t.is_cuda for t in prov.inputs)
    assert torch.equal(torch.cat(prov.inputs), x)
    chips = []
    for i, bb in enumerate(BOXES):
        if bb is None:
            chips.append(torch.full((3, S_FACE, S_FACE), -1.0))           # classified like the rest
            continue
        l, r, bt, tp = max(bb[0], 0), min(bb[2], 64), max(bb[1], 0), min(bb[3], 64)
        face = F.pad(x[i][:, bt:tp, l:r], [max(-bb[0], 0), max(bb[2] - 64, 0), max(-bb[1], 0), max(bb[3] - 64, 0)], value=-1.0)
        chips.append(F.interpolate(face[None], size=[S_FACE, S_FACE], mode="bilinear", align_corners=False)[0])
    chips = torch.stack(chips)
    for p in range(2):
        sl = slice(5 * p, 5 * p + 5)
        ind, boxes = res[0][p], res[1][p]
        assert ind.dtype == torch.bool and tuple(ind.shape) == (5,) and ind.tolist() == [b is not None for b in BOXES[sl]]
        assert boxes.dtype == torch.int64 and boxes.tolist() == [b if b is not None else [-1] * 4 for b in BOXES[sl]]
        assert not any(t.is_cuda for d in res for t in d.values())
    for which, k in enumerate(EI.ATTR_K):
        m = nn_mobilenet.MobileNetV3Large(k).eval()
        m.load_state_dict(EI.synthetic_classifier_state(which), strict=True)
        with torch.no_grad():
            ref = m(chips)
        got = torch.cat([res[2 + which][0], res[2 + which][1]])
        assert got.dtype == torch.float32 and tuple(got.shape) == (10, k)
        e = _relerr(got, ref)
        print(f"[evaluator logits, classifier {which} ({k} classes)] rel max err {e:.3e} (tol 2.0e-02)  max|ref|={float(ref.abs().max()):.3e}")
        assert math.isfinite(e) and e <= 2e-2, (which, e)


def test_metrics_json_equals_the_host_tally(EI, run4):
    from finetune_fair_diffusion_amd import evaluation as E
    d, res, _, lines = run4
    got = json.load(open(os.path.join(str(d), "metrics.json")))
    assert sorted(got) == ["mean", "per_prompt"] and sorted(got["per_prompt"]) == ["0", "1"]
    per = {}
    for p in range(2):
        table = torch.cat([torch.softmax(res[2 + k][p], dim=-1) for k in range(3)], dim=1)
        table[~res[0][p]] = -1
        per[p] = E.gap_metrics("exp-4", E.tally_host(table, EI.TABLE_ATTRS))
        assert got["per_prompt"][str(p)] == E._json_safe(per[p]), (p, got["per_prompt"][str(p)], per[p])
    assert got["mean"] == E._json_safe({k: float(np.array([per[0][k], per[1][k]]).mean()) for k in per[0]})
    assert json.loads(lines[-1])["evaluated_images"] == 10


@pytest.mark.parametrize("grid,n_attr", [("gender_race", 2), ("gender_race_age", 3)])
def test_grids_are_written_at_the_expected_size(EI, tree, run4, tmp_path, grid, n_attr):
    from PIL import Image
    d = run4[0] if n_attr == 2 else tmp_path
    if n_attr == 3:
        _run(EI, tree, d, 10, grid=grid)
    for p in range(2):
        im = Image.open(os.path.join(str(d), f"prompt_{p}.jpg"))
        im.load()
        assert im.mode == "RGB" and im.size == (3 * (64 + 50 * n_attr + 20), 2 * 84)


def test_batch_size_one_gives_the_same_results(EI, tree, run4, tmp_path):
    res4 = run4[1]
    res1, prov, _ = _run(EI, tree, tmp_path, 1, grid="off")
    assert len(prov.inputs) == 10 and not os.path.exists(os.path.join(str(tmp_path), "prompt_0.jpg"))
    for p in range(2):
        assert torch.equal(res1[0][p], res4[0][p]) and torch.equal(res1[1][p], res4[1][p])
        for k in range(3):
            e = _relerr(res1[2 + k][p], res4[2 + k][p])
            assert math.isfinite(e) and e <= 2e-2, (p, k, e)


def test_images_of_one_prompt_must_share_one_size(EI, tmp_path, dev):
    from PIL import Image
    d = tmp_path / "in" / "prompt_0"
    d.mkdir(parents=True)
    Image.fromarray(np.zeros((64, 64, 3), dtype=np.uint8)).save(str(d / "img_0.jpg"))
    Image.fromarray(np.zeros((32, 64, 3), dtype=np.uint8)).save(str(d / "img_1.jpg"))
    args = EI.parse_args(["--synthetic", "--generated_imgs_dir", str(tmp_path / "in"), "--save_dir", str(tmp_path / "out"), "--size_face", "32"])
    with pytest.raises(ValueError, match="img_1.jpg"):
        EI.main(args, log=None)
