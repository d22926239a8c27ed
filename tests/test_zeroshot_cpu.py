"""``--experiment custom --classifier zero_shot`` without a GPU: the grammar of ``--class_prompts`` and every refusal (each names its flag), the derived
``--attributes`` / ``--num_classifier_logits``, the YAML overlay, the unchanged Namespaces and checkpoint records of every run that does not give the new
flag, the two descriptor-free prototypes in the header / ``lib.py`` / INTEGRATION.md, the entry points' refusals with host memory standing in for the
buffers, and the head's backward formula against autograd in fp64."""
import ctypes
import json
import os
import re

import pytest
import torch
import yaml

from finetune_fair_diffusion_amd import lib
from finetune_fair_diffusion_amd.cli import parse_args
from finetune_fair_diffusion_amd.fairness import ExperimentSpec, experiment_spec, parse_class_prompts

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
PROMPTS = "gender=a photo of a man|a photo of a woman;age=a photo of a young person, smiling|a photo of an old person"
ZS = ["--classifier", "zero_shot", "--class_prompts", PROMPTS]
NEW_FLAGS = dict(classifier="mobilenet", class_prompts="", zero_shot_logit_scale=0.0)


def gold(name):
    return json.load(open(os.path.join(HERE, "golden", name)))


# ------------------------------------------------------------------------------------------ grammar and derived values
def test_class_prompts_grammar():
    assert parse_class_prompts(PROMPTS) == [("gender", ["a photo of a man", "a photo of a woman"]),
                                            ("age", ["a photo of a young person, smiling", "a photo of an old person"])]      # commas belong to the prompt
    assert parse_class_prompts(" a_1 = x | y | z | w ;") == [("a_1", ["x", "y", "z", "w"])]


def test_zero_shot_spec_is_derived_from_the_prompts():
    args = parse_args(ZS + ["--target_distribution", "age=0.75,0.25"], with_extras=True, experiment="custom")
    assert args.attributes == "gender:0:2,age:2:2" and args.num_classifier_logits == 4 and args.classifier == "zero_shot"
    spec = experiment_spec("custom", args)
    assert spec.zero_shot and spec.num_logits == 4 and spec.attrs == [("gender", 0, 2), ("age", 2, 2)] and spec.solver == "mc"
    assert spec.prompts == ["a photo of a man", "a photo of a woman", "a photo of a young person, smiling", "a photo of an old person"]
    assert spec.attributes[1].p == (0.75, 0.25) and spec.logit_scale == 0.0
    one = experiment_spec("custom", parse_args(["--classifier", "zero_shot", "--class_prompts", "hat=a person with a hat|a person without a hat",
                                                "--zero_shot_logit_scale", "50"], with_extras=True, experiment="custom"))
    assert one.solver == "rank" and one.num_logits == 2 and one.logit_scale == 50.0
    # the derived flags may be given when they say the same thing
    same = parse_args(ZS + ["--attributes", "gender:0:2,age:2:2", "--num_classifier_logits", "4"], with_extras=True, experiment="custom")
    assert experiment_spec("custom", same) == experiment_spec("custom", parse_args(ZS, with_extras=True, experiment="custom"))
    # --classifier_weight_path is not read: any value resolves
    parse_args(ZS + ["--classifier_weight_path", "/nonexistent/head.pt"], with_extras=True, experiment="custom")


@pytest.mark.parametrize("argv,flag", [
    (["--classifier", "resnet"], "--classifier"),
    (["--classifier", "zero_shot"], "--class_prompts"),                                                    # no prompts
    (["--classifier", "zero_shot", "--class_prompts", "a=x|y;b=x|y;c=x|y;d=x|y"], "--class_prompts"),      # four attributes
    (["--classifier", "zero_shot", "--class_prompts", "a=x"], "--class_prompts"),                          # one class
    (["--classifier", "zero_shot", "--class_prompts", "a=x|y|z|w|v"], "--class_prompts"),                  # five classes
    (["--classifier", "zero_shot", "--class_prompts", "a=x||y"], "--class_prompts"),                       # an empty prompt
    (["--classifier", "zero_shot", "--class_prompts", "a=x|x"], "--class_prompts"),                        # one prompt twice
    (["--classifier", "zero_shot", "--class_prompts", "Gender=x|y"], "--class_prompts"),                   # name
    (["--classifier", "zero_shot", "--class_prompts", "x|y"], "--class_prompts"),                          # no name
    (["--classifier", "zero_shot", "--class_prompts", "a=x|y;a=z|w"], "--class_prompts"),                  # a name twice
    (ZS + ["--attributes", "gender:0:2,age:4:2"], "--attributes"),                                         # given and different
    (ZS + ["--attributes", "gender:0:2"], "--attributes"),
    (ZS + ["--num_classifier_logits", "8"], "--num_classifier_logits"),
    (ZS + ["--zero_shot_logit_scale", "-1"], "--zero_shot_logit_scale"),
    (ZS + ["--zero_shot_logit_scale", "inf"], "--zero_shot_logit_scale"),
    (ZS + ["--size_face", "112"], "--size_face"),                                                          # the tower takes 224
    (ZS + ["--target_distribution", "race=0.5,0.5"], "--target_distribution"),                            # an attribute no prompt defines
    (ZS + ["--target_solver", "rank"], "--target_solver"),                                                 # two attributes
    (["--class_prompts", PROMPTS, "--attributes", "gender:0:2", "--num_classifier_logits", "2"], "--class_prompts"),       # prompts without zero_shot
    (["--zero_shot_logit_scale", "50", "--attributes", "gender:0:2", "--num_classifier_logits", "2"], "--zero_shot_logit_scale"),
])
def test_every_malformed_value_is_refused_in_parse_args_naming_its_flag(argv, flag):
    with pytest.raises(ValueError) as e:
        parse_args(argv, with_extras=True, experiment="custom")
    assert flag in str(e.value), (flag, str(e.value))


def test_size_face_follows_the_run_model_sizes():
    from finetune_fair_diffusion_amd.factory import TINY
    args = parse_args(ZS + ["--size_face", "56"], with_extras=True, experiment="custom", cfgs=TINY)
    assert args.size_face == 56
    with pytest.raises(ValueError, match="--size_face"):
        parse_args(ZS, with_extras=True, experiment="custom", cfgs=TINY)


def test_yaml_overlay_sets_the_new_flags(tmp_path):
    p = tmp_path / "zs.yaml"
    p.write_text(yaml.safe_dump(dict(classifier="zero_shot", class_prompts=PROMPTS, zero_shot_logit_scale=40, target_distribution="age=0.75,0.25")))
    args = parse_args(["--config", str(p)], with_extras=True, experiment="custom")
    spec = experiment_spec("custom", args)
    assert spec.zero_shot and spec.logit_scale == 40.0 and isinstance(args.zero_shot_logit_scale, float) and args.attributes == "gender:0:2,age:2:2"
    assert spec == experiment_spec("custom", parse_args(ZS + ["--zero_shot_logit_scale", "40", "--target_distribution", "age=0.75,0.25"], with_extras=True,
                                                        experiment="custom"))
    bad = tmp_path / "bad.yaml"
    bad.write_text(yaml.safe_dump(dict(classifier="zero_shot", class_prompts="a=x")))
    with pytest.raises(ValueError, match="--class_prompts"):
        parse_args(["--config", str(bad)], with_extras=True, experiment="custom")


# ------------------------------------------------------------------------------------------ nothing else moves
def test_named_experiments_parse_as_before(tmp_path):
    """Defaults and every YAML overlay of exp-1 .. exp-6 against the goldens recorded from the reference's own parsers."""
    cases = [("exp-1", gold("reference_cli.json"))] + list(gold("reference_cli_multi.json").items()) + list(gold("reference_cli_exp6.json").items())
    assert [c[0] for c in cases] == ["exp-1", "exp-2", "exp-3", "exp-4", "exp-5", "exp-6"]
    for exp, g in cases:
        d = vars(parse_args([], experiment=exp))
        assert d == g["defaults"] and not set(NEW_FLAGS) & set(d), exp
        for f in [k for k in g if k != "defaults"]:
            p = tmp_path / f"{exp}-{f}"
            p.write_text(yaml.safe_dump(g[f]["yaml"]))
            d = vars(parse_args(["--config", str(p)], experiment=exp))
            d["config"] = g[f]["args"]["config"]
            assert d == g[f]["args"], (exp, f)


def test_custom_without_the_new_flag_differs_by_the_new_defaults_only():
    """``custom`` keeps exp-1's flags with its documented changes (cli.EXPERIMENT_CLI): the Namespace before this feature, restated from exp-1's golden,
    plus exactly the three new flags at their defaults."""
    before = dict(gold("reference_cli.json")["defaults"])
    before.pop("face_gender_confidence_level")
    before.update(face_confidence_level=0.9, factor1="0.2", factor2="0.2", attributes="", target_distribution="", target_solver="", num_classifier_logits=0,
                  asymmetric_last_attribute=False)
    now = vars(parse_args([], experiment="custom", resolve=False))
    assert now == {**before, **NEW_FLAGS}
    given = ["--attributes", "gender:0:2,race:2:4", "--num_classifier_logits", "8", "--target_distribution", "race=0.4,0.2,0.2,0.2"]
    args = parse_args(given, with_extras=True, experiment="custom")
    assert (args.attributes, args.num_classifier_logits) == ("gender:0:2,race:2:4", 8) and {k: getattr(args, k) for k in NEW_FLAGS} == NEW_FLAGS


def test_state_of_every_other_spec_is_what_it_was():
    keys = {"experiment", "num_logits", "solver", "asymmetric_last", "attributes"}
    for exp in ("exp-1", "exp-2", "exp-3", "exp-4", "exp-5", "exp-6"):
        spec = experiment_spec(exp)
        assert set(spec.state()) == keys and not spec.zero_shot and spec.classifier == "mobilenet" and spec.class_prompts == ()
    args = parse_args(["--attributes", "gender:0:2,age:6:2", "--num_classifier_logits", "8", "--target_distribution", "age=0.75,0.25"], with_extras=True,
                      experiment="custom")
    spec = experiment_spec("custom", args)
    assert spec.state() == dict(experiment="custom", num_logits=8, solver="mc", asymmetric_last=False,
                                attributes=[("gender", 0, 2, (0.5, 0.5)), ("age", 6, 2, (0.75, 0.25))])
    # a spec built the way it was before the new fields existed (positional, eight values) is the same record
    old = ExperimentSpec("custom", 8, spec.attributes, "mc", False, ("factor1",), ("factor2",), "face_confidence_level")
    assert old == spec and old.state() == spec.state()
    zs = experiment_spec("custom", parse_args(ZS, with_extras=True, experiment="custom"))
    st = zs.state()
    assert set(st) == keys | {"classifier", "class_prompts", "logit_scale"} and st["classifier"] == "zero_shot" and st["logit_scale"] == 0.0
    assert st["class_prompts"][1] == ("age", ("a photo of a young person, smiling", "a photo of an old person"))
    other = experiment_spec("custom", parse_args(["--classifier", "zero_shot", "--class_prompts", PROMPTS.replace("old", "elderly")], with_extras=True,
                                                 experiment="custom"))
    assert other.state() != st and {k: v for k, v in other.state().items() if k != "class_prompts"} == {k: v for k, v in st.items() if k != "class_prompts"}


def test_zero_shot_needs_the_clip_directory_before_anything_is_read(monkeypatch, tmp_path):
    """Without ``--synthetic``: FD_CLIP_VISION_DIR is required even when the image term is off, and its absence is reported before a file is opened."""
    from finetune_fair_diffusion_amd import pretrained
    from finetune_fair_diffusion_amd.factory import SD15
    monkeypatch.delenv("FD_CLIP_VISION_DIR", raising=False)
    args = parse_args(ZS + ["--weight_loss_img", "0", "--weight_loss_face", "0", "--pretrained_model_name_or_path", str(tmp_path)], with_extras=True,
                      experiment="custom")
    args.experiment = "custom"
    opened = []
    monkeypatch.setattr(pretrained, "_read", lambda c: opened.append(c) or {})
    with pytest.raises(FileNotFoundError, match="FD_CLIP_VISION_DIR"):
        pretrained.load_pretrained(args, SD15)
    assert not opened


# ------------------------------------------------------------------------------------------ the C-ABI
FWD = ["const float* e", "int64_t lde", "const float* t_hat", "float scale", "float* logits", "float* inv_norm", "int N", "int E", "int K", "void* stream"]
BWD = ["const float* e", "int64_t lde", "const float* t_hat", "const float* logits", "const float* inv_norm", "const float* d_logits", "float scale", "float* d_e",
       "int N", "int E", "int K", "void* stream"]


def test_prototypes_in_header_lib_and_integration_md():
    text = re.sub(r"/\*.*?\*/", " ", open(lib.HEADER_PATH).read(), flags=re.S)
    protos = lib.parse_header()
    f32p, i64, f32, i32 = ctypes.c_void_p, ctypes.c_int64, ctypes.c_float, ctypes.c_int
    want = {"fd_cosine_logits_fwd": (FWD, [f32p, i64, f32p, f32, f32p, f32p, i32, i32, i32, ctypes.c_void_p]),
            "fd_cosine_logits_bwd": (BWD, [f32p, i64, f32p, f32p, f32p, f32p, f32, f32p, i32, i32, i32, ctypes.c_void_p])}
    md = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    rows = [l for l in md.splitlines() if l.startswith("| `fd_cosine_logits_fwd`, `fd_cosine_logits_bwd`")]
    assert len(rows) == 1 and "10 arguments" in rows[0] and "12 arguments" in rows[0] and "FD_ERR_ARG" in rows[0]
    for name, (params, argtypes) in want.items():
        m = re.search(r"\bint\s+" + name + r"\s*\(([^;{]*)\)\s*;", text)
        assert m, name
        assert [" ".join(p.split()) for p in m.group(1).split(",")] == params, name                     # descriptor-free: scalars and typed pointers only
        assert protos[name] == (ctypes.c_int, argtypes), name
        assert "(" + ", ".join(p.split()[-1].lstrip("*") for p in params) + ")" in rows[0], name        # the argument list, in order
    assert lib.ABI_VERSION == 4 and "#define FD_ABI_VERSION 4" in open(lib.HEADER_PATH).read()          # additive
    src = open(os.path.join(ROOT, "finetune_fair_diffusion_amd", "csrc", "Makefile")).read()
    assert re.search(r"^SRCS = .*\bcosine_head\.hip\b", src, flags=re.M)


def test_wrappers_launch_from_the_hosts_the_bf16_guard_reads():
    """``ops.cosine_logits*`` are fronts; the launches sit in ``ops.softmax_rows`` / ``ops.softmax_rows_bwd``, which tests/run_bf16_kernel_checks.py calls."""
    import test_kernel_coverage_cpu as G
    wr = G.wrappers()
    assert wr["fd_cosine_logits_fwd"] == {("ops", "softmax_rows")} and wr["fd_cosine_logits_bwd"] == {("ops", "softmax_rows_bwd")}
    calls, _ = G.exercised(os.path.join(HERE, G.BF16_SCRIPT))
    assert ("ops", "softmax_rows") in calls and ("ops", "softmax_rows_bwd") in calls
    _, literals = G.exercised(os.path.join(HERE, "test_kernels_cosinehead_gpu.py"))
    assert {"fd_cosine_logits_fwd", "fd_cosine_logits_bwd"} <= literals


@pytest.mark.parametrize("so", ["libfairdiff_hip.so", "libfairdiff_hip_bf16.so"])
def test_entry_points_refuse_bad_arguments_before_any_launch(so):
    """Host memory stands in for the buffers: every call here is refused before a launch, so no device is needed.  Both libraries."""
    path = os.path.join(os.path.dirname(lib.LIB_PATH), so)
    L = ctypes.CDLL(path)
    protos = lib.parse_header()
    for name in ("fd_cosine_logits_fwd", "fd_cosine_logits_bwd", "fd_last_error"):
        getattr(L, name).restype, getattr(L, name).argtypes = protos[name]
    buf = (ctypes.c_float * 64)()
    p = ctypes.cast(buf, ctypes.c_void_p)
    N, E, K = 2, 8, 2
    fwd = lambda e=p, lde=E, t=p, lg=p, inv=p, n=N, ee=E, k=K: L.fd_cosine_logits_fwd(e, lde, t, 1.0, lg, inv, n, ee, k, None)  # noqa: E731
    bwd = lambda lde=E, dl=p, de=p, n=N, ee=E, k=K: L.fd_cosine_logits_bwd(p, lde, p, p, p, dl, 1.0, de, n, ee, k, None)  # noqa: E731
    for name, call, word in (("fd_cosine_logits_fwd", lambda: fwd(k=17), "K = 17"), ("fd_cosine_logits_fwd", lambda: fwd(ee=0), "E = 0"),
                             ("fd_cosine_logits_fwd", lambda: fwd(ee=4097, lde=4097), "E = 4097"), ("fd_cosine_logits_fwd", lambda: fwd(lde=E - 1), "lde"),
                             ("fd_cosine_logits_fwd", lambda: fwd(inv=None), "null"), ("fd_cosine_logits_fwd", lambda: fwd(n=0), "N = 0"),
                             ("fd_cosine_logits_bwd", lambda: bwd(k=17), "K = 17"), ("fd_cosine_logits_bwd", lambda: bwd(ee=0), "E = 0"),
                             ("fd_cosine_logits_bwd", lambda: bwd(lde=E - 1), "lde"), ("fd_cosine_logits_bwd", lambda: bwd(de=None), "null"),
                             ("fd_cosine_logits_bwd", lambda: bwd(dl=None), "null")):
        assert call() == -1
        msg = L.fd_last_error().decode()
        assert msg.startswith(name + ":") and word in msg, msg
    assert all(v == 0.0 for v in buf)


# ------------------------------------------------------------------------------------------ the formula
def test_backward_formula_equals_autograd_in_fp64():
    """``d_e = scale * inv * (dl @ t_hat - (dl . c) e^)`` with c = logits / scale: the statement of include/fairdiff_hip.h against autograd of
    ``scale * normalize(e) @ t_hat^T``."""
    g = torch.Generator().manual_seed(4)
    for N, E, K, scale in ((3, 48, 5, 100.0), (1, 7, 1, -2.5), (4, 100, 16, 14.3)):
        e = (torch.randn(N, E, generator=g, dtype=torch.float64) * 3).requires_grad_(True)
        t = torch.nn.functional.normalize(torch.randn(K, E, generator=g, dtype=torch.float64), dim=-1)
        dl = torch.randn(N, K, generator=g, dtype=torch.float64)
        logits = scale * torch.nn.functional.normalize(e, dim=-1) @ t.T
        (logits * dl).sum().backward()
        with torch.no_grad():
            inv = 1.0 / e.norm(dim=-1).clamp_min(1e-12)
            c = logits / scale
            d_e = scale * inv[:, None] * (dl @ t - (dl * c).sum(-1, keepdim=True) * (e * inv[:, None]))
        assert float((d_e - e.grad).abs().max()) <= 1e-12 * float(e.grad.abs().max()), (N, E, K)
