"""Coverage guard (host only, no GPU): every entry point of the C-ABI (``lib.parse_header()``) is either called by a direct kernel test in
``tests/test_kernels*_gpu.py`` -- through the ``ops`` / ``layers`` wrapper whose body launches it, or by its literal name -- or is a host-only
query on the exempt list below.  End-to-end engine tests do not count: their loose bands would not name a wrong kernel."""
import ast
import glob
import os

from finetune_fair_diffusion_amd import lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "finetune_fair_diffusion_amd")

# host-side queries: they launch nothing, so there is no kernel to compare with a reference
EXEMPT = {
    "fd_version": "ABI revision number",
    "fd_last_error": "message of the last refused call",
    "fd_build_info": "compile-time settings string",
    "fd_working_dtype": "16-bit dtype the library was built for",
    "fd_gemm_tile": "tile the dispatcher would pick for a descriptor",
    "fd_gemm_stats_rows": "statistics chunk height the dispatcher would pick",
    "fd_gemm_kernel_name": "name of the kernel the dispatcher would pick",
}
# entry points whose direct kernel test lives beside the feature it serves: (test module, test name) -- the named test must exist and call the wrapper
ELSEWHERE = {
    "fd_ot_expected_targets": ("test_exp6_gpu.py", "test_expected_targets_kernel_matches_host"),
}
WRAPPER_MODULES = ("ops", "layers")
# The bf16 library (same sources, -DFD_BF16) is checked kernel by kernel by tests/run_bf16_kernel_checks.py.  Entry points with no working-dtype operand
# -- no ``void*`` parameter but ``stream`` -- compile to the same code in both libraries and may be listed here instead, each with its reason.
BF16_SCRIPT = "run_bf16_kernel_checks.py"
BF16_LAUNCHER = "test_kernels_bf16_gpu.py"
BF16_SAME_CODE = {
    "fd_eval_tally": "fp32 probabilities to integer counts",
    "fd_eval_grid_attrs_u8": "uint8 images to a uint8 grid",
    "fd_eval_grid_labels_u8": "paints uint8 glyph masks into a uint8 grid",
    "fd_ot_expected_targets": "fp64 costs, integer counts, fp32 weights",
}


def _launches(fn):
    """C-ABI names a Python function launches directly: ``_call("fd_x", ...)`` (also ``ops._call``) and ``_gemm_call`` (fd_gemm)."""
    names = set()
    for node in ast.walk(fn):
        if not isinstance(node, ast.Call):
            continue
        f = node.func
        callee = f.id if isinstance(f, ast.Name) else f.attr if isinstance(f, ast.Attribute) else None
        if callee == "_call" and node.args and isinstance(node.args[0], ast.Constant) and isinstance(node.args[0].value, str):
            names.add(node.args[0].value)
        elif callee == "_gemm_call":
            names.add("fd_gemm")
    return names


def wrappers():
    """{fd name: {(module, wrapper name)}} over ops.py and layers.py: public functions and methods whose body launches the entry point, and
    classes one of whose methods launches it or calls a module-level function of the same module that does (``ops.wgrad_batch``, a context
    manager whose ``__exit__`` runs ``flush_wgrads``)."""
    out = {}
    for mod in WRAPPER_MODULES:
        tree = ast.parse(open(os.path.join(PKG, mod + ".py")).read())
        top = {n.name: _launches(n) for n in tree.body if isinstance(n, (ast.FunctionDef, ast.AsyncFunctionDef))}
        for node in ast.walk(tree):
            if isinstance(node, (ast.FunctionDef, ast.AsyncFunctionDef)) and not node.name.startswith("_"):
                for name in _launches(node):
                    out.setdefault(name, set()).add((mod, node.name))
            elif isinstance(node, ast.ClassDef) and not node.name.startswith("_"):
                names = _launches(node)
                for c in ast.walk(node):
                    if isinstance(c, ast.Call) and isinstance(c.func, ast.Name) and c.func.id in top:
                        names |= top[c.func.id]
                for name in names:
                    out.setdefault(name, set()).add((mod, node.name))
    return out


def _kernel_test_files():
    return sorted(glob.glob(os.path.join(ROOT, "tests", "test_kernels*_gpu.py")))


def exercised(path):
    """(wrapper calls, literal fd_* names) found in one test module.  A wrapper call is ``ops.w(...)`` / ``layers.w(...)`` or a bare ``w(...)``
    of a name imported from those modules; a literal is the string constant ``"fd_x"`` or an attribute ``.fd_x`` (``lib.get().fd_x(...)``)."""
    tree = ast.parse(open(path).read())
    imported = {}
    for node in ast.walk(tree):
        if isinstance(node, ast.ImportFrom) and node.module and node.module.split(".")[-1] in WRAPPER_MODULES:
            for a in node.names:
                imported[a.asname or a.name] = (node.module.split(".")[-1], a.name)
    calls, literals = set(), set()
    for node in ast.walk(tree):
        if isinstance(node, ast.Constant) and isinstance(node.value, str) and node.value.startswith("fd_"):
            literals.add(node.value)
        elif isinstance(node, ast.Attribute) and node.attr.startswith("fd_"):
            literals.add(node.attr)
        if isinstance(node, ast.Call):
            f = node.func
            if isinstance(f, ast.Attribute) and isinstance(f.value, ast.Name) and f.value.id in WRAPPER_MODULES:
                calls.add((f.value.id, f.attr))
            elif isinstance(f, ast.Name) and f.id in imported:
                calls.add(imported[f.id])
    return calls, literals


def uncovered():
    protos = lib.parse_header()
    wr = wrappers()
    calls, literals = set(), set()
    for p in _kernel_test_files():
        c, l = exercised(p)
        calls |= c
        literals |= l
    missing = {}
    for name in protos:
        if name in EXEMPT or name in literals or (wr.get(name, set()) & calls) or name in ELSEWHERE:
            continue
        missing[name] = sorted(f"{m}.{w}" for m, w in wr.get(name, ()))
    return missing


def uncovered_bf16():
    protos = lib.parse_header()
    wr = wrappers()
    calls, literals = exercised(os.path.join(ROOT, "tests", BF16_SCRIPT))
    return {name: sorted(f"{m}.{w}" for m, w in wr.get(name, ())) for name in protos
            if not (name in EXEMPT or name in literals or (wr.get(name, set()) & calls) or name in BF16_SAME_CODE)}


def _prototype_text(name):
    import re
    text = open(os.path.join(ROOT, "include", "fairdiff_hip.h")).read()
    text = re.sub(r"/\*.*?\*/", " ", text, flags=re.S)
    text = re.sub(r"//[^\n]*", " ", text)
    m = re.search(r"\b" + name + r"\s*\(([^;{]*)\)\s*;", text)
    assert m, f"{name}: no prototype in include/fairdiff_hip.h"
    return m.group(1)


def test_every_launching_entry_point_has_a_bf16_kernel_check():
    missing = uncovered_bf16()
    lines = [f"  {n}  (wrappers: {', '.join(w) or 'none in ops.py / layers.py'})" for n, w in sorted(missing.items())]
    assert not missing, (f"C-ABI entry points that tests/{BF16_SCRIPT} does not exercise on the bf16 library (call the wrapper or name the entry point there, "
                         "or list it in BF16_SAME_CODE if it has no working-dtype operand):\n" + "\n".join(lines))


def test_bf16_same_code_entries_have_no_working_dtype_operand():
    import re
    protos = lib.parse_header()
    for name, reason in BF16_SAME_CODE.items():
        assert name in protos and reason, name
        params = [p.strip() for p in _prototype_text(name).split(",")]
        untyped = [p for p in params if re.search(r"\bvoid\s*\*", p) and not re.search(r"\bstream$", p)]
        assert not untyped, f"{name} takes {untyped}: an untyped operand may be a working-dtype buffer, so it needs a bf16 check of its own"
    # the rule itself: an entry point that takes a working-dtype image may not be listed
    assert any(re.search(r"\bvoid\s*\*", p) and not p.strip().endswith("stream") for p in _prototype_text("fd_eval_grid_u8").split(","))


def test_bf16_launcher_adds_nothing_to_the_fp16_guard():
    """tests/test_kernels_bf16_gpu.py matches the fp16 guard's glob: it must name no entry point and call no wrapper, so that it cannot satisfy that guard."""
    calls, literals = exercised(os.path.join(ROOT, "tests", BF16_LAUNCHER))
    assert not calls and not literals, (calls, literals)


def test_exempt_host_queries_are_still_in_the_header():
    protos = lib.parse_header()
    gone = sorted(n for n in EXEMPT if n not in protos)
    assert not gone, f"exempt names no longer declared in include/fairdiff_hip.h (drop them from EXEMPT): {gone}"


def test_every_launching_entry_point_has_a_direct_kernel_test():
    assert _kernel_test_files(), "no tests/test_kernels*_gpu.py found"
    missing = uncovered()
    lines = [f"  {n}  (wrappers: {', '.join(w) or 'none in ops.py / layers.py'})" for n, w in sorted(missing.items())]
    assert not missing, ("C-ABI entry points without a direct kernel test in tests/test_kernels*_gpu.py (call the wrapper or name the entry point "
                         "there, against a plain high-precision reference):\n" + "\n".join(lines))


def test_guard_sees_wrappers_and_calls():
    """The guard's own parsing: known wrappers are found, and a test module's calls and literals are recognised."""
    wr = wrappers()
    assert ("ops", "gemm") in wr["fd_gemm"] and ("ops", "gemm_batched_into") in wr["fd_gemm"]
    assert ("ops", "small_attn_fwd") in wr["fd_small_attn_fwd"]
    assert ("layers", "refresh_pairs") in wr["fd_lora_refresh_multi"]
    assert ("ops", "wgrad_batch") in wr["fd_lora_wgrad_multi"]
    calls, literals = exercised(os.path.join(ROOT, "tests", "test_kernels_gpu.py"))
    assert ("ops", "gemm") in calls and "fd_gemm_tile" in literals


def test_entry_points_tested_elsewhere_are_called_there():
    wr = wrappers()
    for name, (mod, test) in ELSEWHERE.items():
        tree = ast.parse(open(os.path.join(ROOT, "tests", mod)).read())
        fn = [n for n in tree.body if isinstance(n, ast.FunctionDef) and n.name == test]
        assert fn, f"{name}: tests/{mod}::{test} is gone"
        called = {c.func.attr for c in ast.walk(fn[0]) if isinstance(c, ast.Call) and isinstance(c.func, ast.Attribute)}
        called |= {c.func.id for c in ast.walk(fn[0]) if isinstance(c, ast.Call) and isinstance(c.func, ast.Name)}
        helpers = [n for n in tree.body if isinstance(n, ast.FunctionDef) and n.name in called]
        for h in helpers:           # one level of module-local helpers (``_device_targets``)
            called |= {c.func.attr for c in ast.walk(h) if isinstance(c, ast.Call) and isinstance(c.func, ast.Attribute)}
        assert {w for _, w in wr.get(name, ())} & called, f"{name}: tests/{mod}::{test} no longer calls its wrapper"
