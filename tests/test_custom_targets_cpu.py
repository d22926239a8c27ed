"""``--experiment custom`` on the host: the resolved target specification (``fairness.ExperimentSpec``), its refusals, the restatements of the
named experiments through it, the three solvers under a non-uniform target, the metrics against the target and the command line."""
import itertools
import math
import types

import numpy as np
import pytest
import torch

from finetune_fair_diffusion_amd import evaluation as E
from finetune_fair_diffusion_amd import fairness as FA
from finetune_fair_diffusion_amd import fairness_dev as FD
from finetune_fair_diffusion_amd.cli import parse_args

NAMED = ["exp-1", "exp-2", "exp-3", "exp-4", "exp-5", "exp-6"]
RESTATED = {          # named experiment -> the custom flags that restate it
    "exp-1": dict(num_classifier_logits=80, attributes="gender:40:2"),
    "exp-3": dict(num_classifier_logits=6, attributes="gender:0:2,race:2:4"),
    "exp-4": dict(num_classifier_logits=8, attributes="gender:0:2,race:2:4,age:6:2", target_distribution="age=0.75,0.25", asymmetric_last_attribute=True),
    "exp-6": dict(num_classifier_logits=6, attributes="race:2:4", target_solver="enumerate"),
}


def _spec(**kw):
    return FA.experiment_spec("custom", types.SimpleNamespace(**kw))


def _probs(n, k, seed, missing=()):
    p = torch.softmax(torch.randn(n, k, generator=torch.Generator().manual_seed(seed)) * 2.0, dim=-1)
    for i in missing:
        p[i] = -1.0
    return p


# ------------------------------------------------------------------------------------------ the specification
@pytest.mark.parametrize("experiment", NAMED)
def test_spec_of_a_named_experiment_is_its_table_row(experiment):
    s = FA.experiment_spec(experiment)
    ncls, attrs, cdfs, asym = FA.EXPERIMENT_ATTRS[experiment]
    f1, f2, conf = FA.EXPERIMENT_REG_FLAGS[experiment]
    assert (s.num_logits, s.attrs, s.asymmetric_last) == (ncls, attrs, asym)
    assert (list(s.factor1_flags), list(s.factor2_flags), s.confidence_flag) == (f1, f2, conf)
    assert s.class_cdfs == cdfs          # float for float (None where nothing is drawn)
    if cdfs is not None:
        assert all(type(e) is float for c in s.class_cdfs for e in c)
    assert s.solver == {"exp-1": "rank", "exp-2": "rank", "exp-6": "enumerate"}.get(experiment, "mc") and not s.custom
    args = types.SimpleNamespace(**{k: 0.1 * (i + 1) for i, k in enumerate(f1 + f2)}, **{conf: 0.85})
    assert s.regulariser_values(args) == ([getattr(args, k) for k in f1], [getattr(args, k) for k in f2], 0.85)


@pytest.mark.parametrize("experiment", list(RESTATED))
def test_restated_spec_equals_the_named_one(experiment):
    s, n = _spec(**RESTATED[experiment]), FA.experiment_spec(experiment)
    assert (s.num_logits, s.attrs, s.class_cdfs, s.asymmetric_last, s.solver) == (n.num_logits, n.attrs, n.class_cdfs, n.asymmetric_last, n.solver)
    assert [a.p for a in s.attributes] == [a.p for a in n.attributes]
    assert s.custom and s.state() != n.state()


def test_cdf_edges_are_running_fp64_sums_ending_in_one():
    s = _spec(num_classifier_logits=6, attributes="gender:0:2,race:2:4", target_distribution="race=0.4,0.2,0.2,0.2;gender=0.7,0.3")
    assert s.class_cdfs == [[0.7, 1.0], [0.4, 0.4 + 0.2, 0.4 + 0.2 + 0.2, 1.0]]
    assert _spec(num_classifier_logits=3, attributes="x:0:3").attributes[0].p == (1 / 3, 1 / 3, 1 / 3)
    assert _spec(num_classifier_logits=3, attributes="x:0:3").class_cdfs[0][-1] == 1.0
    assert s.regulariser_values(types.SimpleNamespace(factor1="0.2,0.6", factor2=0.3, face_confidence_level=0.8)) == ([0.2, 0.6], [0.3, 0.3], 0.8)


BASE = ["--num_classifier_logits", "6", "--attributes", "gender:0:2,race:2:4"]
REFUSALS = {
    "sum off by 1e-3": (BASE + ["--target_distribution", "gender=0.5,0.501"], "--target_distribution"),
    "negative entry": (BASE + ["--target_distribution", "gender=1.2,-0.2"], "--target_distribution"),
    "wrong count": (BASE + ["--target_distribution", "gender=0.5,0.25,0.25"], "--target_distribution"),
    "unknown attribute": (BASE + ["--target_distribution", "hair=0.5,0.5"], "--target_distribution"),
    "duplicate name": (["--num_classifier_logits", "6", "--attributes", "gender:0:2,gender:2:2"], "--attributes"),
    "overlapping columns": (["--num_classifier_logits", "6", "--attributes", "gender:0:2,race:1:4"], "--attributes"),
    "column beyond the logits": (["--num_classifier_logits", "6", "--attributes", "gender:5:2"], "--attributes"),
    "four attributes": (["--num_classifier_logits", "8", "--attributes", "a:0:2,b:2:2,c:4:2,d:6:2"], "--attributes"),
    "k = 5": (["--num_classifier_logits", "8", "--attributes", "a:0:5"], "--attributes"),
    "rank with k = 4": (["--num_classifier_logits", "6", "--attributes", "race:2:4", "--target_solver", "rank"], "--target_solver"),
    "enumerate with two attributes": (BASE + ["--target_solver", "enumerate"], "--target_solver"),
    "no logit count": (["--attributes", "gender:0:2"], "--num_classifier_logits"),
    "unknown solver": (BASE + ["--target_solver", "simplex"], "--target_solver"),
    "bad name": (["--num_classifier_logits", "6", "--attributes", "Gender:0:2"], "--attributes"),
    "factor list of the wrong length": (BASE + ["--factor1", "0.1,0.2,0.3"], "--factor1"),
}


@pytest.mark.parametrize("case", list(REFUSALS))
def test_parse_args_refuses_and_names_the_flag(case):
    argv, flag = REFUSALS[case]
    with pytest.raises(ValueError, match=flag):
        parse_args(argv, with_extras=True, experiment="custom")


# ------------------------------------------------------------------------------------------ restatements on the host
def test_custom_as_exp1_equals_generate_dynamic_targets():
    probs = _probs(12, 2, 1, missing=(3, 9))
    probs[5] = probs[6]          # tied probabilities
    t, u = FA.spec_dynamic_targets(_spec(**RESTATED["exp-1"]), [probs])[0]
    tr, ur = FA.generate_dynamic_targets(probs, w_uncertainty=True)
    assert torch.equal(t, tr) and torch.equal(u, ur) and int((t == -1).sum()) == 2


@pytest.mark.parametrize("experiment", ["exp-3", "exp-4"])
def test_custom_as_multi_attribute_equals_generate_dynamic_targets_multi(experiment):
    _, attrs, cdfs, asym = FA.EXPERIMENT_ATTRS[experiment]
    probs = [_probs(9, k, 10 + i, missing=(2,)) for i, (_, _, k) in enumerate(attrs)]
    for p in probs:
        p[4] = p[5]
    got = FA.spec_dynamic_targets(_spec(**RESTATED[experiment]), probs, generator=torch.Generator().manual_seed(77), num_samples_per_device=20)
    ref = FA.generate_dynamic_targets_multi(probs, cdfs, 20, torch.Generator().manual_seed(77), age_asymmetric=asym)
    assert len(got) == len(ref) == len(attrs)
    for (t, u), (tr, ur) in zip(got, ref):
        assert torch.equal(t, tr) and torch.equal(u, ur) and int(t[2]) == -1


def test_custom_as_exp6_equals_expected_transport_targets():
    probs = _probs(9, 4, 5, missing=(0, 7))
    probs[3] = probs[4]
    t, u = FA.spec_dynamic_targets(_spec(**RESTATED["exp-6"]), [probs])[0]
    tr, ur = FA.expected_transport_targets(probs)
    assert torch.equal(t, tr) and torch.equal(u, ur)


# ------------------------------------------------------------------------------------------ the three solvers under a non-uniform target
def test_rank_rule_with_a_ratio():
    probs = _probs(12, 2, 21, missing=(1, 8))
    spec = _spec(num_classifier_logits=2, attributes="gender:0:2", target_distribution="gender=0.8,0.2")
    assert spec.solver == "rank"
    t, u = FA.spec_dynamic_targets(spec, [probs])[0]
    assert sorted(t.tolist()) == [-1] * 2 + [0] * 8 + [1] * 2 and t[1] == -1 and t[8] == -1
    faces = (t != -1).nonzero().view(-1)
    assert set(faces[probs[faces, 1].argsort()[-2:]].tolist()) == set((t == 1).nonzero().view(-1).tolist())          # the two most class-1-like faces
    td, ud = FD.dynamic_targets(probs, FD.binomial_tables(12, 0.8), target_ratio=0.8)
    assert torch.equal(td, t) and ud.dtype == torch.float32 and torch.equal(ud, u.to(torch.float32))
    # the threshold's rounding: n * ratio in fp64, compared in fp32, for every face count and a ratio that is not a dyadic fraction
    for n in range(1, 40):
        p = _probs(n, 2, 100 + n)
        for ratio in (0.3, 0.7, 0.9):
            th, uh = FA.generate_dynamic_targets(p, target_ratio=ratio, w_uncertainty=True)
            tdv, udv = FD.dynamic_targets(p, FD.binomial_tables(n, ratio), target_ratio=ratio)
            assert torch.equal(tdv, th) and torch.equal(udv, uh.to(torch.float32)), (n, ratio)


def test_monte_carlo_invariants():
    spec = _spec(num_classifier_logits=5, attributes="a:0:3,b:3:2", target_distribution="a=0.6,0.3,0.1")
    probs = [_probs(11, 3, 31, missing=(4,)), _probs(11, 2, 32, missing=(4,))]
    idx, M, counts, sizes = FA.mc_transport_problem(probs, spec.class_cdfs, 50, torch.Generator().manual_seed(1))
    assert sizes == [3, 2] and M.shape == (10, 6) and counts.shape == (50, 6) and (counts.sum(axis=1) == 10).all() and int(idx.sum()) == 10
    one = _spec(num_classifier_logits=2, attributes="g:0:2", target_distribution="g=1,0", target_solver="mc")
    assert one.class_cdfs == [[1.0, 1.0]]
    p = _probs(7, 2, 33, missing=(6,))
    t, u = FA.spec_dynamic_targets(one, [p], generator=torch.Generator().manual_seed(2), num_samples_per_device=10)[0]
    assert t.tolist() == [0] * 6 + [-1] and u.tolist() == [0.0] * 6 + [-1.0]


def test_composition_table_uniform_is_the_cached_object():
    tab = FA.composition_table(6)
    assert FA.composition_table(6, 4, (0.25, 0.25, 0.25, 0.25)) is tab and FA.composition_table(6, 4, None) is tab
    assert FA.composition_table(6, 4, (0.4, 0.2, 0.2, 0.2)) is not tab


def test_composition_table_binary_by_hand():
    """N = 5, p = (0.7, 0.3): binomial weights 0.00243, 0.02835, 0.1323, 0.3087, 0.36015, 0.16807 for n1 = 0..5; descending 4, 3, 5, 2 reaches
    0.36015 + 0.3087 + 0.16807 = 0.83692 <= 0.95 and, with 0.1323, 0.96922 > 0.95."""
    counts, w = FA.composition_table(5, 2, (0.7, 0.3))
    assert counts.dtype == np.int32 and counts.tolist() == [[4, 1], [3, 2], [5, 0], [2, 3]]
    np.testing.assert_allclose(w, [0.36015, 0.3087, 0.16807, 0.1323], rtol=1e-12)


@pytest.mark.parametrize("N", [1, 4, 7, 12])
def test_composition_table_k3_is_the_multinomial(N):
    import scipy.stats
    p = (0.6, 0.3, 0.1)
    counts, w = FA.composition_table(N, 3, p)
    every = [(a, b, N - a - b) for a in range(N + 1) for b in range(N - a + 1)]          # first class outermost
    pmf = scipy.stats.multinomial.pmf(every, N, p)
    full = pmf / np.abs(pmf).sum()
    kept = {tuple(c): v for c, v in zip(counts.tolist(), w)}
    assert len(kept) == len(counts) and (counts.sum(axis=1) == N).all()
    for c, v in kept.items():
        assert abs(v - full[every.index(c)]) <= 1e-12 * full[every.index(c)]
    # the shortest prefix of the descending weights whose mass exceeds 0.95 (strict)
    assert (np.diff(w) <= 0).all()
    assert w.sum() > 0.95 and (len(w) == 1 or w[:-1].sum() <= 0.95)
    rest = [v for c, v in zip(every, full) if c not in kept]
    assert not rest or max(rest) <= w.min() * (1 + 1e-12)


def test_enumerate_under_a_non_uniform_target_uses_its_table():
    probs = _probs(6, 3, 41, missing=(2,))
    spec = _spec(num_classifier_logits=3, attributes="r:0:3", target_distribution="r=0.6,0.3,0.1", target_solver="enumerate")
    t, u = FA.spec_dynamic_targets(spec, [probs])[0]
    tr, ur = FA.expected_transport_targets(probs, table=FA.composition_table(5, 3, (0.6, 0.3, 0.1)))
    assert torch.equal(t, tr) and torch.equal(u, ur) and t[2] == -1 and set(t.tolist()) <= {-1, 0, 1, 2}


# ------------------------------------------------------------------------------------------ metrics
def _table(n, attrs, seed, missing=()):
    t = torch.cat([_probs(n, k, seed + i) for i, (_, k) in enumerate(attrs)], dim=1)
    for i in missing:
        t[i] = -1.0
    return t


def test_age_gap_to_target_is_exp4s_age_gap():
    attrs = [(0, 2), (2, 4), (6, 2)]
    spec = _spec(**RESTATED["exp-4"])
    for seed in range(5):
        table = _table(13 + seed, attrs, 50 + 10 * seed, missing=(1,))
        counts, joint = E.tally_host(table, attrs), E.joint_tally_host(table, attrs)
        m = E.gap_metrics("custom", counts, spec, joint)
        ref = E.gap_metrics("exp-4", counts)
        assert m["age_gap_to_target"] == ref["age_gap"] and m["age0_freq"] == ref["age_young_freq"] and m["age1_freq"] == ref["age_old_freq"]
        assert m["age_pred_below_0.8"] == ref["age_pred_below_0.8"] and m["race_pred_below_0.8"] == ref["race_pred_below_0.8"]
        assert set(m) == {f"gender{k}_freq" for k in range(2)} | {f"race{k}_freq" for k in range(4)} | {f"age{k}_freq" for k in range(2)} | \
            {f"{n}_{s}" for n in ("gender", "race", "age") for s in ("pred_below_0.8", "gap_to_target")} | {"joint_gap_to_target"}


def _counts(*hists):
    c = torch.zeros(E.N_COUNTS, dtype=torch.int32)
    for a, h in enumerate(hists):
        c[E.ATTR_STRIDE * a] = sum(h)
        for k, v in enumerate(h):
            c[E.ATTR_STRIDE * a + E.OFF_HIST + k] = v
    return c


def test_gap_to_target_values():
    spec = _spec(num_classifier_logits=2, attributes="g:0:2", target_distribution="g=0.75,0.25")
    assert E.gap_metrics("custom", _counts([6, 2]), spec)["g_gap_to_target"] == 0.0
    uni = _spec(num_classifier_logits=4, attributes="r:0:4")
    m = E.gap_metrics("custom", _counts([0, 0, 9, 0]), uni)
    assert m["r_gap_to_target"] == 0.75 and "joint_gap_to_target" not in m
    two = _spec(num_classifier_logits=4, attributes="a:0:2,b:2:2", target_distribution="a=0.5,0.5;b=0.75,0.25")
    joint = torch.tensor([3, 1, 3, 1], dtype=torch.int32)          # cells (a, b) = 00 01 10 11: exactly the product target
    m = E.gap_metrics("custom", _counts([4, 4], [6, 2]), two, joint)
    assert m["a_gap_to_target"] == 0.0 and m["b_gap_to_target"] == 0.0 and m["joint_gap_to_target"] == 0.0
    m = E.gap_metrics("custom", _counts([4, 4], [6, 2]), two, torch.tensor([4, 0, 2, 2], dtype=torch.int32))
    assert m["joint_gap_to_target"] == 0.5 * (abs(0.5 - 0.375) + abs(0.0 - 0.125) + abs(0.25 - 0.375) + abs(0.25 - 0.125))
    with pytest.raises(ValueError):
        E.gap_metrics("custom", _counts([4, 4], [6, 2]), two)


@pytest.mark.parametrize("attrs", [[(0, 2), (2, 4)], [(0, 3), (3, 2), (5, 4)], [(0, 4), (4, 4), (8, 4)]])
def test_joint_tally_equals_a_brute_force_loop(attrs):
    table = _table(37, attrs, 90, missing=(0, 11, 36))
    table[5, attrs[0][0]:attrs[0][0] + attrs[0][1]] = 1.0 / attrs[0][1]          # a tie: the first maximum wins
    cells = list(itertools.product(*[range(k) for _, k in attrs]))
    brute = [0] * len(cells)
    for row in table.tolist():
        if -1.0 in row:
            continue
        cell = []
        for c0, k in attrs:
            seg = row[c0:c0 + k]
            cell.append(seg.index(max(seg)))
        brute[cells.index(tuple(cell))] += 1
    assert sum(brute) == 34 and len(brute) == math.prod(k for _, k in attrs) <= 64
    assert E.joint_tally_host(table, attrs).tolist() == brute
    got = E.joint_tally(table, attrs)
    assert got.dtype == torch.int32 and got.tolist() == brute


def test_evaluator_target_gaps_on_hand_made_counts():
    from finetune_fair_diffusion_amd import evaluate_images as EI
    targets = EI.parse_targets("age=0.75,0.25;race=0.4,0.2,0.2,0.2")
    assert targets == [("gender", (0.5, 0.5)), ("race", (0.4, 0.2, 0.2, 0.2)), ("age", (0.75, 0.25))]
    g = EI.target_gaps(_counts([3, 1], [4, 0, 0, 0], [3, 1]), targets)
    assert g == {"gender_gap_to_target": 0.25, "race_gap_to_target": (abs(1.0 - 0.4) + abs(0.0 - 0.2) + abs(0.0 - 0.2) + abs(0.0 - 0.2)) / 2, "age_gap_to_target": 0.0}
    with pytest.raises(ValueError, match="--target_distribution"):
        EI.parse_targets("hair=0.5,0.5")
    assert "target_distribution" not in vars(EI.parse_args([]))
    assert EI.parse_args(["--target_distribution", "age=0.75,0.25"]).target_distribution == "age=0.75,0.25"


# ------------------------------------------------------------------------------------------ command line
def test_cli_custom_with_and_without_yaml(tmp_path):
    argv = ["--num_classifier_logits", "8", "--attributes", "gender:0:2,age:6:2", "--target_distribution", "age=0.75,0.25", "--factor1", "0.2,0.6"]
    a = parse_args(argv, with_extras=True, experiment="custom")
    assert (a.attributes, a.target_distribution, a.target_solver, a.num_classifier_logits) == ("gender:0:2,age:6:2", "age=0.75,0.25", "", 8)
    assert a.factor1 == "0.2,0.6" and a.factor2 == "0.2" and a.face_confidence_level == 0.9 and a.asymmetric_last_attribute is False
    assert not hasattr(a, "face_gender_confidence_level") and a.train_text_encoder is True and a.validation == "off"
    s = FA.experiment_spec("custom", a)
    assert s.attrs == [("gender", 0, 2), ("age", 6, 2)] and s.solver == "mc" and s.class_cdfs == [[0.5, 1.0], [0.75, 1.0]]
    assert s.regulariser_values(a) == ([0.2, 0.6], [0.2, 0.2], 0.9)
    cfg = tmp_path / "custom.yaml"
    cfg.write_text("num_classifier_logits: 6\nattributes: 'race:2:4'\ntarget_distribution: 'race=0.4,0.2,0.2,0.2'\ntarget_solver: enumerate\n"
                   "factor2: 0.3\nface_confidence_level: 0.8\nasymmetric_last_attribute: 0\n")
    b = parse_args(["--config", str(cfg)], with_extras=True, experiment="custom")
    assert (b.attributes, b.target_solver, b.num_classifier_logits, b.factor2, b.face_confidence_level) == ("race:2:4", "enumerate", 6, "0.3", 0.8)
    sb = FA.experiment_spec("custom", b)
    assert sb.solver == "enumerate" and sb.attributes[0].p == (0.4, 0.2, 0.2, 0.2) and sb.regulariser_values(b) == ([0.2], [0.3], 0.8)
    bad = tmp_path / "bad.yaml"
    bad.write_text("num_classifier_logits: 6\nattributes: 'race:2:4'\ntarget_distribution: 'race=0.4,0.2,0.2,0.3'\n")
    with pytest.raises(ValueError, match="--target_distribution"):
        parse_args(["--config", str(bad)], with_extras=True, experiment="custom")


def test_default_args_and_checkpoint_state_of_a_custom_run():
    from finetune_fair_diffusion_amd.factory import default_args
    a = default_args("custom", num_classifier_logits=2, attributes="gender:0:2", target_distribution="gender=0.75,0.25")
    s = FA.experiment_spec("custom", a)
    assert s.solver == "rank" and s.attributes[0].p == (0.75, 0.25)
    other = FA.experiment_spec("custom", default_args("custom", num_classifier_logits=2, attributes="gender:0:2", target_distribution="gender=0.7,0.3"))
    assert s.state() == FA.experiment_spec("custom", a).state() and s.state() != other.state()
