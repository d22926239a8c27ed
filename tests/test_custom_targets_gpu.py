"""``--experiment custom`` on the MI355X with the tiny models: the restatements of the named experiments bit for bit, a non-uniform binary target
on the device tail, the device solvers under non-uniform capacities, validation / monitor / evaluator numbers against the target, and resume."""
import json
import os
import pickle
import sys

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import custom_cases as C  # noqa: E402
import util_models as U  # noqa: E402
from test_kernels_trainplots_gpu import _host_inputs  # noqa: E402

pytestmark = pytest.mark.gpu


# ------------------------------------------------------------------------------------------ restatements
@pytest.mark.parametrize("named", ["exp-1", "exp-3", "exp-4", "exp-6"])
def test_custom_restates_the_named_experiment_bit_for_bit(dev, named):
    snaps, tr_n, tr_c = C.check_restatement(dev, named)
    print(named, "targets", {k: v.tolist() for k, v in snaps[-1].items() if k.startswith("targets_by_attr/")})


def test_non_uniform_binary_target_on_the_device_tail(dev):
    """gender = 0.75 / 0.25: targets and uncertainties of the step are the host statement's; the step makes as many device reads as exp-1's
    (its one read-back of the report, riding the finite flag)."""
    tr, out = C.check_non_uniform_binary(dev)
    ref = C.build(dev, "exp-1", batch=8)
    ref.train_step(U.tiny_tokens(), C.noises(0, 8), C.S)
    reads = []
    for t in (ref, tr):
        with C.count_device_reads() as n:
            t.train_step(U.tiny_tokens(), C.noises(1, 8), C.S)
        reads.append(n[0])
    print("device reads per step: exp-1", reads[0], "custom 0.75/0.25", reads[1])
    assert reads[1] == reads[0] and tr._pending_readback is None and tr._readback_host is not None


# ------------------------------------------------------------------------------------------ device solvers under non-uniform capacities
P3 = (0.6, 0.3, 0.1)


@pytest.mark.parametrize("N", [5, 65])
def test_device_assignment_under_non_uniform_capacities(dev, N):
    """K = 3, p = (0.6, 0.3, 0.1), S = 3 draws, continuous random costs (a unique optimum): plan and seats of ``ops.ot_assign_sum`` are scipy's."""
    from finetune_fair_diffusion_amd import ops
    from finetune_fair_diffusion_amd.fairness import _ot_assign
    rng = np.random.RandomState(100 + N)
    M = rng.rand(N, 3)
    counts = rng.multinomial(N, P3, size=3).astype(np.int32)
    assert (counts.sum(axis=1) == N).all()
    plan, seats = ops.ot_assign_sum(torch.from_numpy(M).to(dev), torch.from_numpy(counts).to(dev), seats=True)
    torch.cuda.synchronize()
    want = np.zeros((N, 3))
    for s in range(3):
        T = _ot_assign(M, counts[s])
        want += T
        assert seats[s].cpu().tolist() == T.argmax(axis=1).tolist(), s
    assert plan.dtype == torch.float32 and np.array_equal(plan.cpu().numpy(), want.astype(np.float32))


@pytest.mark.parametrize("N", [5, 65])
def test_device_expected_targets_with_a_non_uniform_table(dev, N):
    from finetune_fair_diffusion_amd.fairness import composition_table, expected_transport_targets
    probs = torch.softmax(torch.randn(N + 2, 3, generator=torch.Generator().manual_seed(300 + N)) * 2.0, dim=-1)
    probs[1] = -1.0
    probs[N] = -1.0
    counts, w = composition_table(N, 3, P3)
    assert (counts.sum(axis=1) == N).all() and w.sum() > 0.95
    td, ud = expected_transport_targets(probs, device=dev, p=P3)
    th, uh = expected_transport_targets(probs, p=P3)
    assert torch.equal(td, th) and ud.numpy().tobytes() == uh.numpy().tobytes() and th[1] == -1
    print(f"N={N}: {len(w)} compositions kept, targets {np.bincount(th[th >= 0].numpy(), minlength=3).tolist()}")


# ------------------------------------------------------------------------------------------ validation and monitor
TWO = dict(num_classifier_logits=8, attributes="gender:0:2,age:6:2", target_distribution="age=0.75,0.25")


def test_validation_reports_the_gaps_to_the_target(dev):
    from finetune_fair_diffusion_amd import evaluation as E
    tr = C.build(dev, custom=TWO, val_images_per_prompt_GPU=6, val_GPU_batch_size=4)
    tok = lambda p: U.tiny_tokens()
    prompts = ["a", "b"]
    lat = tr.unet.config.sample_size
    noises = torch.randn(2, 6, 4, lat, lat, generator=torch.Generator().manual_seed(3))
    lines = []
    logs = E.evaluate_process(tr, "main", "main", [(p, tok(p)) for p in prompts], noises, 0, log=lines.append)
    attrs = E.table_attrs(tr.attrs)
    assert attrs == [(0, 2), (2, 2)]
    for i in range(2):
        images = E._generate(tr, tr.te, tr.unet, tok(prompts[i]), noises[i].to(dev))
        _, _, per = tr.classify(images)
        table = torch.cat([a["probs"] for a in per], dim=1)
        joint = E.joint_tally_host(table, attrs)
        assert torch.equal(tr.last_eval_joint[i], joint) and int(joint.sum()) == 6 and tr.last_eval_joint[i].dtype == torch.int32
        assert torch.equal(tr.last_eval_counts[i], E.tally_host(table, attrs))
        assert logs[i] == E.gap_metrics("custom", E.tally_host(table, attrs), tr.spec, joint)
    rec = json.loads(lines[0])
    want = {"gender0_freq", "gender1_freq", "gender_pred_below_0.8", "gender_gap_to_target", "age0_freq", "age1_freq", "age_pred_below_0.8",
            "age_gap_to_target", "joint_gap_to_target"}
    assert set(rec["mean"]) == want and all(set(m) == want for m in rec["per_prompt"].values())
    assert 0.0 <= rec["mean"]["age_gap_to_target"] <= 1.0


THREE = dict(num_classifier_logits=8, attributes="gender:0:2,race:2:4,age:6:2", target_distribution="age=0.75,0.25")


def test_three_strip_grid_of_a_custom_run(dev):
    """The grid of a three-attribute custom run is the host statement's, painted with the palettes chosen by class count."""
    from finetune_fair_diffusion_amd import evaluate_images as EI, evaluation as E
    tr = C.build(dev, custom=THREE)
    images = E._generate(tr, tr.te, tr.unet, U.tiny_tokens(), C.noises(7, 5).to(dev))
    h = tr.classify_begin(images)
    pd = E.probability_table(tr, h)
    boxes = h["boxes"].to(dev, torch.int32)
    got = E.device_grid_attrs(tr, images, boxes, pd).cpu().numpy()
    palettes = E.strip_palettes(tr)
    assert palettes == [E.PALETTE_GENDER, E.PALETTE_RACE, E.PALETTE_GENDER]
    preds, probs, bars, order = _host_inputs(EI, pd.cpu(), E.table_attrs(tr.attrs))
    ref = E.grid_attrs_img_host(images.cpu(), order, boxes.cpu().numpy(), preds, bars, palettes)
    H = W = 8 * tr.unet.config.sample_size
    assert got.shape == E.grid_attrs_shape(5, H, W, 3)[2] and np.array_equal(got, ref), int((got != ref).sum())
    k3 = C.build(dev, custom=dict(num_classifier_logits=5, attributes="a:0:3,b:3:2"))
    assert E.strip_palettes(k3) == [E.PALETTE_RACE[:4], E.PALETTE_GENDER]


def test_train_driver_custom_logs_the_gap_to_target(dev, tmp_path):
    """The driver end to end: two steps towards 75 % / 25 % age with the monitor and one validation pass."""
    from finetune_fair_diffusion_amd import train
    from finetune_fair_diffusion_amd.factory import TINY
    logs = []
    argv = ["--experiment", "custom", "--synthetic", "--attributes", "gender:0:2,age:6:2", "--num_classifier_logits", "8", "--target_distribution",
            "age=0.75,0.25", "--validation", "metrics", "--train_monitor", "metrics", "--train_unet", "--rank", "4", "--max_train_steps", "2",
            "--checkpointing_steps", "100", "--checkpointing_steps_long", "100", "--num_denoising_steps", "2", "--train_images_per_prompt_GPU", "4",
            "--train_GPU_batch_size", "3", "--val_GPU_batch_size", "4", "--val_images_per_prompt_GPU", "4", "--evaluate_every_n_iter", "100",
            "--weight_loss_img", "0", "--weight_loss_face", "0", "--uncertainty_threshold", "0.9", "--output_dir", str(tmp_path)]
    tr, n = train.main(argv, cfgs=TINY, log=logs.append)
    recs = [json.loads(x) for x in logs]
    assert n == 2 and tr.experiment == "custom" and tr.clf.num_classes == 8 and tr.spec.solver == "mc" and not tr.device_tail
    evals, steps = [r for r in recs if "eval" in r], [r for r in recs if "eval" not in r]
    assert [r["eval"] for r in evals] == ["main", "EMA"] and all("age_gap_to_target" in r["mean"] and "joint_gap_to_target" in r["mean"] for r in evals)
    assert len(steps) == 2 and all("train_age_gap_to_target" in r and "train_joint_gap_to_target" in r and r["num_faces"] == 4 for r in steps)


# ------------------------------------------------------------------------------------------ evaluator
def test_evaluator_target_gaps(dev, tmp_path):
    from PIL import Image
    from finetune_fair_diffusion_amd import evaluate_images as EI, evaluation as E
    rng = np.random.RandomState(11)
    root = tmp_path / "generated"
    for p in range(2):
        (root / f"prompt_{p}").mkdir(parents=True)
        for j in range(3):
            blocks = rng.randint(0, 256, (8, 8, 3)).astype(np.uint8)
            Image.fromarray(np.kron(blocks, np.ones((8, 8, 1), dtype=np.uint8))).save(str(root / f"prompt_{p}" / f"img_{j}.jpg"))
    base = ["--synthetic", "--generated_imgs_dir", str(root), "--size_face", "64", "--batch_size", "2"]
    text = "race=0.4,0.2,0.2,0.2;age=0.75,0.25"
    outs = {}
    for name, extra in (("plain", []), ("again", []), ("targets", ["--target_distribution", text])):
        save = tmp_path / name
        results, outs[name] = EI.main(EI.parse_args(base + ["--save_dir", str(save)] + extra), log=None)
        if name == "targets":
            logits = results[2:]
    files = sorted(os.listdir(tmp_path / "plain"))
    assert files == sorted(os.listdir(tmp_path / "again")) == sorted(os.listdir(tmp_path / "targets")) and "metrics.json" in files
    for f in files:          # without the flag: the same files, run after run; with it only metrics.json differs
        a, b, c = (open(tmp_path / d / f, "rb").read() for d in ("plain", "again", "targets"))
        if f.endswith(".pkl"):          # a pickle of tensors is not a canonical byte string (two runs without the flag differ in it): by content
            a, b, c = (pickle.loads(x) for x in (a, b, c))
            for x in (b, c):
                assert len(x) == len(a) == 5 and all(set(u) == set(v) == {0, 1} and all(torch.equal(u[k], v[k]) for k in u) for u, v in zip(a, x)), f
            continue
        assert a == b, f
        assert (a != c) if f == "metrics.json" else (a == c), f
    got = json.load(open(tmp_path / "targets" / "metrics.json"))
    plain = json.load(open(tmp_path / "plain" / "metrics.json"))
    assert "target_gaps" not in plain and {k: v for k, v in got.items() if k != "target_gaps"} == plain
    targets = EI.parse_targets(text)
    assert got["target_gaps"]["targets"] == {"gender": [0.5, 0.5], "race": [0.4, 0.2, 0.2, 0.2], "age": [0.75, 0.25]}
    per = {}
    for p in range(2):
        table = torch.cat([torch.softmax(l[p], dim=-1) for l in logits], dim=1)
        per[str(p)] = EI.target_gaps(E.tally_host(table, EI.TABLE_ATTRS), targets)
    assert got["target_gaps"]["per_prompt"] == per
    assert got["target_gaps"]["mean"] == {k: float(np.array([per["0"][k], per["1"][k]]).mean()) for k in per["0"]}


# ------------------------------------------------------------------------------------------ resume
def test_custom_checkpoint_resumes_bit_equal_and_refuses_another_target(dev, tmp_path):
    from finetune_fair_diffusion_amd import checkpoint as ck
    a = C.build(dev, custom=TWO)
    a.train_step(U.tiny_tokens(), C.noises(0), C.S)
    path = ck.save_state(a, str(tmp_path / "checkpoint-1"), 1)
    st = torch.load(os.path.join(path, "trainer_state.pth"), map_location="cpu", weights_only=False)
    assert st["spec"] == a.spec.state() and st["spec"]["attributes"][1] == ("age", 6, 2, (0.75, 0.25))
    out_a = a.train_step(U.tiny_tokens(), C.noises(1), C.S)
    want = C.snapshot(a, out_a)
    b = C.build(dev, custom=TWO)
    assert ck.load_state(b, path) == 1
    got = C.snapshot(b, b.train_step(U.tiny_tokens(), C.noises(1), C.S))
    for k in want:
        assert torch.equal(want[k], got[k]), k
    # another target: refused before anything is copied
    c = C.build(dev, custom=dict(TWO, target_distribution="age=0.5,0.5"))
    held = [(bk.flat.clone(), bk.ema.clone(), bk.exp_avg.clone(), bk.exp_avg_sq.clone()) for bk in c.banks]
    with pytest.raises(ValueError, match="target"):
        ck.load_state(c, path)
    for bk, h in zip(c.banks, held):
        assert all(torch.equal(x, y) for x, y in zip((bk.flat, bk.ema, bk.exp_avg, bk.exp_avg_sq), h))
    assert not torch.equal(c.banks[0].exp_avg, b.banks[0].exp_avg)
    # a named experiment's checkpoint carries no specification, and a named trainer refuses a custom checkpoint as well
    n = C.build(dev, "exp-4")
    pn = ck.save_state(n, str(tmp_path / "checkpoint-named"), 0)
    assert "spec" not in torch.load(os.path.join(pn, "trainer_state.pth"), map_location="cpu", weights_only=False)
    with pytest.raises(ValueError):
        ck.load_state(n, path)
