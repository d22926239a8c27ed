"""The evaluator's face metrics (``evaluate_images.main --face_metrics``) end to end on small trees of JPEGs written here, against the fp32 oracle: the
oracle's image pipeline on ``u/255*2-1``, its SFNet-20 with the evaluator's synthetic state, and the brute-force fp32 maximum over the same database.

Band: ``|sim - sim_ref| <= 2e-2 * max|1 - sim_ref|``, the band of ``loss_face`` in ``test_sfnet20_features_and_input_gradient_vs_oracle`` (``check``
is relative to the largest reference loss), here for ``1 - loss_face``."""
import json
import os
import pickle

import numpy as np
import pytest
import torch

import facealign_cases as FC

pytestmark = pytest.mark.gpu

S_FACE, S_ALIGNED = 64, 112
NUMBERS = (0, 1, 2, 3, 10)
BAND = 2e-2
BOXES = [[8, 6, 50, 48], [-7, 5, 35, 47], [20, 20, 70, 70], None, [0, 0, 64, 64],
         [10, 12, 40, 42], [5, 30, 45, 70], [30, 2, 62, 34], [16, 16, 48, 48], [-10, -10, 74, 74]]      # generated image 3 has no face
BOXES_ORI = [[6, 6, 50, 50], None, [10, 10, 60, 60], [4, 8, 44, 48], [0, 0, 64, 64],
             [12, 12, 42, 42], [5, 20, 45, 60], [28, 4, 60, 36], [16, 16, 48, 48], [2, 2, 62, 62]]       # original image 1 has no face


def _landmarks():
    """Five landmarks per image by running image number: generated 0..9, then originals 0..9.  Generated image 6 has its face partly outside the image."""
    rng = np.random.RandomState(21)
    gen = [FC.face(rng, 34, 0.2, (30, 28)), FC.face(rng, 26, -0.4, (22, 30)), FC.face(rng, 44, 0.1, (34, 33)), None, FC.face(rng, 52, 0.0, (32, 32)),
           FC.face(rng, 28, 0.7, (26, 27)), FC.face(rng, 40, -0.9, (58, 8)), FC.face(rng, 30, 0.3, (45, 18)), FC.face(rng, 30, -0.2, (32, 32)), FC.face(rng, 60, 0.05, (31, 33))]
    ori = [FC.face(rng, 36, -0.1, (29, 29)), None, FC.face(rng, 40, 0.3, (35, 35)), FC.face(rng, 32, 0.0, (24, 28)), FC.face(rng, 50, 0.1, (32, 31)),
           FC.face(rng, 28, -0.5, (27, 26)), FC.face(rng, 34, 0.4, (25, 40)), FC.face(rng, 30, -0.3, (44, 20)), FC.face(rng, 32, 0.2, (33, 31)), FC.face(rng, 56, -0.05, (32, 32))]
    return [None if l is None else torch.tensor(l, dtype=torch.float32) for l in gen + ori]


LANDMARKS = _landmarks()


class ScriptedProvider:
    """Boxes and landmarks by image: the script is indexed by the running image number of the generated tree (0..9) and, for the originals, 10 + that number;
    an image is recognised by its pixels, so the script holds whatever the batch size and whichever tree a batch comes from.  ``landmarks`` must be handed
    the very tensor ``__call__`` got last (a detector provider caches by identity)."""

    def __init__(self, known):
        self.known, self.calls, self.landmark_calls, self.last = known, [], 0, None

    def _which(self, images):
        out = []
        for im in images:
            hit = [i for i in range(self.known.shape[0]) if torch.equal(self.known[i], im)]
            assert hit, "an image the test did not write"
            out.append(hit[0])
        return out

    def __call__(self, images):
        assert images.dtype == torch.float32 and not images.is_cuda
        self.last = images
        ids = self._which(images)
        self.calls.append(ids)
        bb = [(BOXES + BOXES_ORI)[i] for i in ids]
        return torch.tensor([b is not None for b in bb]), torch.tensor([b if b is not None else [-1] * 4 for b in bb], dtype=torch.int32)

    def landmarks(self, images):
        assert images is self.last, "landmarks() was handed another tensor than the provider call before it"
        self.landmark_calls += 1
        return torch.stack([LANDMARKS[i] if LANDMARKS[i] is not None else torch.full((5, 2), -1.0) for i in self._which(images)])


@pytest.fixture(scope="module")
def EI():
    from finetune_fair_diffusion_amd import evaluate_images
    return evaluate_images


@pytest.fixture(scope="module")
def TINY():
    from finetune_fair_diffusion_amd.factory import TINY
    return TINY


@pytest.fixture(scope="module")
def trees(tmp_path_factory):
    """Two trees of two prompts with five 64x64 JPEGs each (img_10 sorts after img_2 numerically) -> (generated dir, original dir, decoded uint8
    [20,64,64,3]: generated 0..9, then originals 0..9)."""
    from PIL import Image
    rng = np.random.RandomState(9)
    roots, decoded = [], []
    for name in ("generated", "original"):
        root = tmp_path_factory.mktemp(name)
        roots.append(str(root))
        for p in range(2):
            (root / f"prompt_{p}").mkdir()
            for j in NUMBERS:
                path = str(root / f"prompt_{p}" / f"img_{j}.jpg")
                Image.fromarray(np.kron(rng.randint(0, 256, (8, 8, 3)).astype(np.uint8), np.ones((8, 8, 1), dtype=np.uint8))).save(path)
                decoded.append(np.asarray(Image.open(path).convert("RGB")))
    return roots[0], roots[1], torch.from_numpy(np.stack(decoded))


def _x(u8):
    return u8.permute(0, 3, 1, 2).float() / 255 * 2 - 1


def _run(EI, TINY, trees, save_dir, batch_size, faces=True, ori=None, grid="off"):
    prov = ScriptedProvider(_x(trees[2]))
    argv = ["--synthetic", "--generated_imgs_dir", trees[0], "--save_dir", str(save_dir), "--batch_size", str(batch_size), "--size_face", str(S_FACE),
            "--grid", grid, "--size_aligned_face", str(S_ALIGNED)]
    argv += ["--face_metrics"] if faces else []
    argv += ["--original_imgs_dir", ori] if ori is not None else []
    lines = []
    EI.main(EI.parse_args(argv), face_provider=prov, log=lines.append, cfgs=TINY)
    return prov, lines


def _load(save_dir, name):
    with open(os.path.join(str(save_dir), name), "rb") as f:
        return pickle.load(f)


def _bytes(save_dir, name):
    with open(os.path.join(str(save_dir), name), "rb") as f:
        return f.read()


@pytest.fixture(scope="module")
def run_plain(EI, TINY, trees, tmp_path_factory, dev):
    d = tmp_path_factory.mktemp("plain")
    return (d,) + _run(EI, TINY, trees, d, 4, faces=False, grid="gender_race")


@pytest.fixture(scope="module")
def run_faces(EI, TINY, trees, tmp_path_factory, dev):
    """The flag alone, batch size 4, grids on."""
    d = tmp_path_factory.mktemp("faces4")
    return (d,) + _run(EI, TINY, trees, d, 4, grid="gender_race")


@pytest.fixture(scope="module")
def run_pairs(EI, TINY, trees, tmp_path_factory, dev):
    """The flag with the second tree as originals, batch size 4."""
    d = tmp_path_factory.mktemp("pairs4")
    return (d,) + _run(EI, TINY, trees, d, 4, ori=trees[1])


@pytest.fixture(scope="module")
def oracle(EI, trees):
    """-> (unit features [20,512] fp32 of the oracle chain, nan rows without a face; sim_face_real reference [20])"""
    from oracle import nn_sfnet as OS
    net = OS.SFNet20(in_size=S_ALIGNED).eval()
    net.load_state_dict(EI.synthetic_face_state(S_ALIGNED))
    x = _x(trees[2])
    rows = [i for i in range(20) if LANDMARKS[i] is not None]
    chips = torch.stack([OS.image_pipeline(x[i], LANDMARKS[i].numpy(), S_ALIGNED) for i in rows])
    with torch.no_grad():
        f = OS.get_face_feats(net, chips)
    feats = torch.full((20, 512), float("nan"))
    feats[rows] = f
    real = torch.full((20,), float("nan"))
    real[rows] = (f @ EI.synthetic_face_db().t()).max(dim=-1).values
    return feats, real


def _bytes_of(t):
    return t.contiguous().numpy().tobytes()


def _cat(d):
    return torch.cat([d[0], d[1]])


def _bits(t):
    """fp32 bit patterns, with every nan made one value (a nan's payload is not a result)"""
    return torch.nan_to_num(t, nan=9.0).contiguous().view(torch.int32)


def _within_band(name, got, ref):
    have = ~torch.isnan(ref)
    assert torch.equal(torch.isnan(got), ~have), (name, got.tolist())
    scale = float((1 - ref[have]).abs().max())
    err = float((got[have] - ref[have]).abs().max())
    print(f"[{name}] max abs err {err:.3e} (band {BAND:.0e} * {scale:.3f} = {BAND * scale:.3e})  reference {[round(float(v), 4) for v in ref[have]]}")
    assert np.isfinite(err) and err <= BAND * scale


def test_without_the_flag_nothing_is_added(run_plain):
    d, prov, lines = run_plain
    assert prov.landmark_calls == 0 and prov.calls == [[0, 1, 2, 3], [4], [5, 6, 7, 8], [9]]
    assert sorted(os.listdir(str(d))) == ["metrics.json", "prompt_0.jpg", "prompt_1.jpg", "test_results.pkl"]
    assert sorted(json.loads(lines[-1])) == ["evaluated_images", "images_per_s", "prompts", "seconds"]


def test_the_flag_leaves_the_other_outputs_byte_identical(run_plain, run_faces):
    d0, d1 = run_plain[0], run_faces[0]
    assert sorted(os.listdir(str(d1))) == ["faces.json", "faces.pkl", "metrics.json", "prompt_0.jpg", "prompt_1.jpg", "test_results.pkl"]
    for name in ("metrics.json", "prompt_0.jpg", "prompt_1.jpg"):
        assert _bytes(d0, name) == _bytes(d1, name), name
    # a pickle of torch tensors names each storage by its address, so two runs of one command differ in those bytes: the content is compared, bit for bit
    with_flag, without = _load(d1, "test_results.pkl"), _load(d0, "test_results.pkl")
    assert len(with_flag) == len(without) == 5
    for a, b in zip(with_flag, without):
        assert sorted(a) == sorted(b) == [0, 1]
        for p in a:
            assert a[p].dtype == b[p].dtype and a[p].shape == b[p].shape and _bytes_of(a[p]) == _bytes_of(b[p]), p
    prov, lines = run_faces[1], run_faces[2]
    assert prov.landmark_calls == 4 and prov.calls == run_plain[1].calls
    assert json.loads(lines[-1])["face_chips"] == 9 and json.loads(lines[-1])["evaluated_images"] == 10


def test_similarity_to_the_nearest_real_face_against_the_oracle(EI, run_faces, oracle):
    faces = _load(run_faces[0], "faces.pkl")
    assert isinstance(faces, list) and len(faces) == 3 and sorted(faces[0]) == sorted(faces[1]) == [0, 1] and faces[2] == {}
    for p in range(2):
        lm, sim = faces[0][p], faces[1][p]
        assert lm.dtype == sim.dtype == torch.float32 and tuple(lm.shape) == (5, 5, 2) and tuple(sim.shape) == (5,) and not lm.is_cuda and not sim.is_cuda
        for j in range(5):
            want = LANDMARKS[5 * p + j]
            assert torch.equal(lm[j], want if want is not None else torch.full((5, 2), -1.0))
    got, ref = _cat(faces[1]), oracle[1][:10]
    assert torch.isnan(ref).tolist() == [b is None for b in BOXES]
    # the database is not met by accident: a random unit vector of 512 dimensions against 4096 rows
    assert 0.05 < float(ref[~torch.isnan(ref)].min()) and float(ref[~torch.isnan(ref)].max()) < 0.5
    _within_band("sim_face_real vs oracle", got, ref)
    js = json.load(open(os.path.join(str(run_faces[0]), "faces.json")))
    assert js == EI.faces_summary(faces, {0: list(NUMBERS), 1: list(NUMBERS)})
    assert js["per_prompt"]["0"]["faces"] == 4 and js["per_prompt"]["1"]["faces"] == 5 and "pairs" not in js["per_prompt"]["0"] and sorted(js["mean"]) == ["sim_face_real"]


def test_a_tree_against_itself_keeps_every_identity(EI, TINY, trees, run_faces, tmp_path):
    _run(EI, TINY, trees, tmp_path, 4, ori=trees[0])
    faces = _load(tmp_path, "faces.pkl")
    ori, real = _cat(faces[2]), _cat(faces[1])
    assert torch.isnan(ori).tolist() == [b is None for b in BOXES]
    print(f"[sim_face_ori, a tree against itself] min {float(ori[~torch.isnan(ori)].min()):.8f}")
    assert float(ori[~torch.isnan(ori)].min()) >= 1 - 1e-5
    assert torch.equal(_bits(real), _bits(_cat(_load(run_faces[0], "faces.pkl")[1])))          # the originals do not move sim_face_real


def test_similarity_to_the_original_face_against_the_oracle(EI, run_pairs, oracle):
    d, prov, lines = run_pairs
    faces = _load(d, "faces.pkl")
    feats = oracle[0]
    ref = (feats[:10] * feats[10:]).sum(-1)          # nan where either image has no face
    assert torch.isnan(ref).tolist() == [a is None or b is None for a, b in zip(BOXES, BOXES_ORI)] and int(torch.isnan(ref).sum()) == 2
    _within_band("sim_face_ori vs oracle", _cat(faces[2]), ref)
    _within_band("sim_face_real vs oracle (with originals)", _cat(faces[1]), oracle[1][:10])
    assert prov.calls == [[0, 1, 2, 3], [10, 11, 12, 13], [4], [14], [5, 6, 7, 8], [15, 16, 17, 18], [9], [19]] and prov.landmark_calls == 8
    js = json.load(open(os.path.join(str(d), "faces.json")))
    assert js == EI.faces_summary(faces, {0: list(NUMBERS), 1: list(NUMBERS)})
    assert js["per_prompt"]["0"]["pairs"] == 3 and js["per_prompt"]["1"]["pairs"] == 5 and sorted(js["mean"]) == ["sim_face_ori", "sim_face_real"]
    assert json.loads(lines[-1])["face_chips"] == 18 and json.loads(lines[-1])["semantics_pairs"] == 10
    assert sorted(os.listdir(str(d))) == ["faces.json", "faces.pkl", "metrics.json", "semantics.json", "semantics.pkl", "test_results.pkl"]


def test_batch_size_one_gives_the_same_faces(EI, TINY, trees, run_pairs, tmp_path):
    prov, _ = _run(EI, TINY, trees, tmp_path, 1, ori=trees[1])
    assert len(prov.calls) == 20 and prov.landmark_calls == 20
    one, four = _load(tmp_path, "faces.pkl"), _load(run_pairs[0], "faces.pkl")
    for k, name in enumerate(("landmarks", "sim_face_real", "sim_face_ori")):
        a, b = _cat(one[k]), _cat(four[k])
        diff = float(torch.nan_to_num(a - b, nan=0.0).abs().max())
        print(f"[{name}, batch size 1 vs 4] max abs diff {diff:.3e}")
        assert torch.equal(torch.isnan(a), torch.isnan(b))
        assert torch.equal(_bits(a), _bits(b)), (name, diff)
