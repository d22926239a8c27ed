"""exp-6 (race debiasing, exp-6-debias-race/1-main-debias.py) on the host: the CLI surface and the exact-enumeration transport targets
against the reference's own outputs (tests/golden/make_golden_exp6.py)."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
GOLD = np.load(os.path.join(HERE, "golden", "reference_exp6_targets.npz"))
NS = [int(n) for n in GOLD["Ns"]]
NPY_NO_SIMD = "AVX512_ICL AVX512_CNL AVX512_CLX AVX512_SKX AVX512CD AVX512F AVX2 FMA3"


def test_cli_exp6_matches_reference(tmp_path):
    """parse_args(experiment="exp-6"): defaults and every YAML overlay equal the reference's own parse_args output."""
    import yaml
    from finetune_fair_diffusion_amd.cli import parse_args
    gold = json.load(open(os.path.join(HERE, "golden", "reference_cli_exp6.json")))["exp-6"]
    assert vars(parse_args([], experiment="exp-6")) == gold["defaults"]
    overlays = [f for f in gold if f != "defaults"]
    assert len(overlays) == 3
    for f in overlays:
        p = tmp_path / f
        p.write_text(yaml.safe_dump(gold[f]["yaml"]))
        d = vars(parse_args(["--config", str(p)], experiment="exp-6"))
        d["config"] = f
        assert d == gold[f]["args"], f


def test_train_preparser_accepts_exp6(monkeypatch):
    """``train --experiment exp-6`` gets past the driver's pre-parser (it stops at the missing GPU / the parsed experiment is exp-6)."""
    from finetune_fair_diffusion_amd import train
    seen = {}

    def fake_parse(argv, with_extras, experiment):
        seen["experiment"] = experiment
        raise SystemExit(0)
    monkeypatch.setattr(train, "parse_args", fake_parse)
    with pytest.raises(SystemExit):
        train.main(["--experiment", "exp-6", "--synthetic"])
    assert seen["experiment"] == "exp-6"


def test_exp6_experiment_tables():
    from finetune_fair_diffusion_amd.fairness import EXPERIMENT_ATTRS, EXPERIMENT_REG_FLAGS
    assert EXPERIMENT_ATTRS["exp-6"] == (6, [("race", 2, 4)], None, False)
    assert EXPERIMENT_REG_FLAGS["exp-6"] == (["factor1"], ["factor2"], "face_race_confidence_level")


@pytest.mark.parametrize("N", NS)
def test_composition_table_matches_reference(N):
    """The product's table for N against the table the reference kept: same length, weights bit-equal per composition, identical membership
    above the cutoff weight and the same number of cutoff-weight members (which of the equal-weight compositions at the cutoff are kept depends
    on the reference's unstable sort; the product sorts stably).  N = 0: the reference keeps the single empty composition (it seats nobody and
    adds nothing); the product's table is empty."""
    from finetune_fair_diffusion_amd.fairness import composition_table
    rc, rw = GOLD[f"N{N}_combs"], GOLD[f"N{N}_weights"]
    c, w = composition_table(N)
    assert c.dtype == np.int32 and w.dtype == np.float64 and c.shape == (len(w), 4)
    if N == 0:
        assert len(c) == 0 and rc.tolist() == [[0, 0, 0, 0]]
        return
    assert len(c) == len(rc)
    assert (c.sum(axis=1) == N).all() and (np.diff(w) <= 0).all()
    ref = {tuple(x): y for x, y in zip(rc.tolist(), rw)}
    mine = {tuple(x): y for x, y in zip(c.tolist(), w)}
    assert len(mine) == len(c)
    cut = rw.min()
    for k in ref.keys() & mine.keys():
        assert ref[k].tobytes() == mine[k].tobytes(), k
    assert {k for k, v in ref.items() if v > cut} == {k for k, v in mine.items() if v > cut}
    assert sum(v == cut for v in ref.values()) == sum(v == cut for v in mine.values())
    assert min(mine.values()) == cut
    # every composition left out weighs no more than the cutoff: the product's kept set is a valid reading of the same rule
    assert all(v == cut for k, v in ref.items() if k not in mine)


def test_composition_table_does_not_depend_on_the_cpu():
    """Without AVX-512 / AVX2 numpy sorts through another code path: the table (kept order included) is byte-identical."""
    from finetune_fair_diffusion_amd.fairness import composition_table
    code = ("import sys, numpy as np\n"
            "from numpy._core._multiarray_umath import __cpu_features__ as f\n"
            "if f.get('AVX512F') or f.get('AVX2'):\n"
            "    sys.exit(3)\n"
            "from finetune_fair_diffusion_amd.fairness import composition_table\n"
            "for N in (4, 8, 16, 32, 36):\n"
            "    c, w = composition_table(N)\n"
            "    sys.stdout.write(c.tobytes().hex() + ':' + w.tobytes().hex() + '\\n')\n")
    env = dict(os.environ, NPY_DISABLE_CPU_FEATURES=NPY_NO_SIMD, PYTHONPATH=ROOT)
    r = subprocess.run([sys.executable, "-c", code], env=env, capture_output=True, text=True, cwd=ROOT, timeout=300)
    if r.returncode != 0:
        pytest.skip(f"numpy refuses NPY_DISABLE_CPU_FEATURES on this host (exit {r.returncode}): {r.stderr.strip()[-300:]}")
    lines = r.stdout.split()
    for N, line in zip((4, 8, 16, 32, 36), lines):
        c, w = composition_table(N)
        assert line == c.tobytes().hex() + ":" + w.tobytes().hex(), N
    assert len(lines) == 5


@pytest.mark.parametrize("N", NS)
def test_expected_transport_targets_match_reference(N):
    """The host statement on the recorded reference table reproduces the reference's targets exactly and its fp64 uncertainties bit for bit."""
    from finetune_fair_diffusion_amd.fairness import expected_transport_targets
    probs = torch.from_numpy(GOLD[f"N{N}_probs"])
    t, u = expected_transport_targets(probs, table=(GOLD[f"N{N}_combs"], GOLD[f"N{N}_weights"]))
    assert t.dtype == torch.long and u.dtype == torch.float64
    assert t.tolist() == GOLD[f"N{N}_targets"].tolist()
    assert u.numpy().tobytes() == GOLD[f"N{N}_uncertainty"].tobytes()
    if N:
        assert (t != -1).sum() == N and int((probs == -1).all(dim=-1).sum()) == len(probs) - N


def test_expected_transport_targets_without_faces():
    from finetune_fair_diffusion_amd.fairness import composition_table, expected_transport_targets
    t, u = expected_transport_targets(torch.full((5, 4), -1.0))
    assert t.tolist() == [-1] * 5 and u.tolist() == [-1.0] * 5
    c, w = composition_table(0)
    assert c.shape == (0, 4) and w.shape == (0,)


def test_expected_transport_targets_own_table_agrees_with_reference_targets():
    """With the product's own (stably sorted) table the targets still equal the reference's on the golden inputs; the uncertainties move
    only by the weight of the cutoff tie group."""
    from finetune_fair_diffusion_amd.fairness import expected_transport_targets
    for N in NS:
        t, u = expected_transport_targets(torch.from_numpy(GOLD[f"N{N}_probs"]))
        assert t.tolist() == GOLD[f"N{N}_targets"].tolist(), N
        assert np.abs(u.numpy() - GOLD[f"N{N}_uncertainty"]).max(initial=0.0) < 0.05, N


def _exp6_rank_worker(rank, world, port, out):
    """Two gloo ranks through the product's own ``start / finish_dynamic_targets`` for exp-6 (host solver on the worker thread): the probability
    all-gather, the expected-transport targets of the whole global batch on every rank, no plan all-reduce, the fp32 threshold, this rank's slice."""
    import types
    import torch.distributed as dist
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world))
    dist.init_process_group("gloo", rank=rank, world_size=world)
    from finetune_fair_diffusion_amd.fairness import EXPERIMENT_ATTRS
    from finetune_fair_diffusion_amd.step import FairnessTrainer
    B = 6
    tr = FairnessTrainer.__new__(FairnessTrainer)
    tr.world, tr.rank, tr.device, tr.collectives = world, rank, torch.device("cpu"), True
    tr.args = types.SimpleNamespace(uncertainty_threshold=0.45)
    _, tr.attrs, tr.class_cdfs, tr.age_asym = EXPERIMENT_ATTRS["exp-6"]
    tr.enumerated_targets, tr.ot_on_device, tr.overlap_targets, tr._tgt = True, False, True, None
    probs = torch.softmax(torch.randn(B, 4, generator=torch.Generator().manual_seed(40 + rank)) * 2.0, dim=-1)
    if rank == 1:
        probs[2] = -1                        # an image without a face
    tr._probs_dev = probs.clone()
    tr.start_dynamic_targets([dict(probs=probs)], B)
    assert "thread" in tr._tgt
    (t, u), = tr.finish_dynamic_targets()
    out[rank] = dict(probs=probs.numpy(), t=t.numpy(), u=u.numpy(), ms=tr.last_ot_ms)
    dist.destroy_process_group()


def test_exp6_targets_through_the_step_on_two_ranks():
    import torch.multiprocessing as mp
    from finetune_fair_diffusion_amd.fairness import expected_transport_targets
    mgr = mp.Manager()
    out = mgr.dict()
    mp.spawn(_exp6_rank_worker, args=(2, 29671, out), nprocs=2, join=True)
    allp = torch.tensor(np.concatenate([out[r]["probs"] for r in range(2)]))
    t_ref, u_ref = expected_transport_targets(allp)
    t_ref[u_ref.float() > 0.45] = -1
    got_t = np.concatenate([out[r]["t"] for r in range(2)])
    got_u = np.concatenate([out[r]["u"] for r in range(2)])
    assert got_t.tolist() == t_ref.tolist() and got_u.tobytes() == u_ref.float().numpy().tobytes()
    assert got_t[6 + 2] == -1 and (got_t != -1).sum() >= 4 and (got_t == -1).sum() >= 2
    assert all(out[r]["ms"][0] > 0 for r in range(2))
