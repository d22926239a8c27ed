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


# ============================================================================= the kernel instantiations behind fd_gemm
# fd_gemm is ONE entry point with ~100 kernel symbols behind its dispatcher; the guard above counts it once.  tests/gemm_cases.py is the table of problems
# that tests/test_kernels_sharp_gpu.py runs under the sharp gates; here, without a GPU, every gemm_* / conv_halo_* / splitk_* symbol of the built fp16 library
# must be the kernel fd_gemm_kernel_name answers for at least one case, or be listed in gemm_cases.UNREACHED with a reason -- checked where it can be.
GEMM_FAMILY = r"^(gemm_|conv_halo_|splitk_)"
FP16_LIB = os.path.join(PKG, "libfairdiff_hip.so")


def _fp16_lib():
    """The fp16 product library with the header's prototypes bound (host-only queries: nothing here touches a device)."""
    import ctypes
    L = ctypes.CDLL(FP16_LIB)
    for name, (ret, argtypes) in lib.parse_header().items():
        fn = getattr(L, name)
        fn.restype, fn.argtypes = ret, argtypes
    assert L.fd_working_dtype().decode() == "fp16"
    return L


def _query(L, case, residual=True):
    import ctypes
    import gemm_cases
    d = gemm_cases.descriptor(case, lib.GemmDesc, residual)
    buf = ctypes.create_string_buffer(128)
    split = L.fd_gemm_kernel_name(ctypes.byref(d), buf, 128)
    return buf.value.decode(), split, L.fd_gemm_stats_rows(ctypes.byref(d)), L.fd_gemm_tile(ctypes.byref(d))


def _shipped_gemm_symbols():
    import sys
    sys.path.insert(0, os.path.join(PKG, "csrc"))
    import codeobj
    return codeobj.kernel_symbols(FP16_LIB, GEMM_FAMILY)


def _pp_default_policy():
    import re
    m = re.search(r"#define\s+FD_GEMM_PP_DEFAULT\s+\(([0-9 |]+)\)", open(os.path.join(PKG, "csrc", "gemm.hip")).read())
    assert m, "FD_GEMM_PP_DEFAULT is no longer a plain OR of bits in csrc/gemm.hip"
    bits = 0
    for b in m.group(1).split("|"):
        bits |= int(b)
    return bits


def test_every_case_of_the_gemm_table_names_the_kernel_the_dispatcher_picks():
    import gemm_cases
    L = _fp16_lib()
    wrong = []
    for c in gemm_cases.CASES:
        for residual in ((True, False) if "R" in c.operands else (True,)):
            name, split, rows, tile = _query(L, c, residual)
            want_rows = 32 if c.gn_stats else None
            if name != c.kernel or split != c.split or (want_rows is not None and rows != want_rows):
                wrong.append(f"  {c.id} (residual={residual}): table says {c.kernel} split {c.split}, the library answers {name} split {split} (tile {tile}, stats rows {rows})")
    assert not wrong, "the dispatch policy moved these cases of tests/gemm_cases.py (re-derive their shapes from gemm_tile's thresholds):\n" + "\n".join(wrong)


def test_gemm_table_shapes_are_the_smallest_the_thresholds_admit():
    """One row fewer and a big-tile / gemm_glds 128-row case lands on another kernel (skinny: M >= 1024, six rows of tail kept on purpose; the halo kernels
    take whole images; the 64x64 tile and the small-M split-K branch have no lower threshold; convolution shapes are whole maps): the table tests tails, and stays as cheap as the dispatcher allows."""
    import gemm_cases
    L = _fp16_lib()
    for c in gemm_cases.CASES:
        floor_free = c.family == "skinny" or "<64, 64" in c.kernel or (c.split and "<128, 160" in c.kernel) or c.conv is not None
        if floor_free:
            continue
        smaller = c._replace(M=c.M - 1)
        name, split, _, _ = _query(L, smaller)
        assert (name, split) != (c.kernel, c.split), f"{c.id}: M = {c.M - 1} still reaches {c.kernel}"


def test_every_shipped_gemm_kernel_symbol_is_run_by_a_case_or_explained():
    import gemm_cases
    L = _fp16_lib()
    symbols = _shipped_gemm_symbols()
    assert len(symbols) > 90 and "splitk_reduce_kernel" in symbols and "gemm_skinny_kernel<1, 4, 1>" in symbols, symbols[:5]
    named = set()
    for c in gemm_cases.CASES:
        name, split, _, _ = _query(L, c)
        named.add(name)
        if split > 1:
            named.add("splitk_reduce_kernel")        # fd_gemm launches it behind every split-K GEMM
    unexplained = [s for s in symbols if s not in named and s not in gemm_cases.UNREACHED]
    assert not unexplained, ("kernel symbols of libfairdiff_hip.so that no case of tests/gemm_cases.py launches and UNREACHED does not explain:\n  " + "\n  ".join(unexplained))
    both = sorted(named & set(gemm_cases.UNREACHED))
    assert not both, f"listed as unreached but launched by a case (drop them from UNREACHED): {both}"
    stale = sorted(s for s in gemm_cases.UNREACHED if s not in symbols)
    assert not stale, f"UNREACHED names symbols the library no longer ships: {stale}"
    never_unreached = [s for s in symbols if s.startswith("gemm_glds_kernel") or s.startswith("conv_halo_kernel") or (s.startswith("gemm_skinny_kernel") and s.endswith(", 1>"))]
    assert len(never_unreached) == 6 + 12 + 12 and not set(never_unreached) & set(gemm_cases.UNREACHED)


def test_reasons_of_the_unreached_gemm_kernels_hold_for_the_product_library():
    import re
    import gemm_cases
    L = _fp16_lib()
    assert set(gemm_cases.UNREACHED.values()) <= set(gemm_cases.REASONS)
    used = set(gemm_cases.UNREACHED.values())
    # "a bench_env switch of the measurement build": the product library has no bench hooks -- bench_env() returns nullptr there (csrc/common.h), the
    # build string names none, and the one entry point only -DFD_BENCH_HOOKS exports is absent
    if used & {"skinny_rt2", "w8", "pp_no_prio"}:
        info = L.fd_build_info().decode()
        assert "bench" not in info.lower() and "hook" not in info.lower(), info
        assert not hasattr(L, "fd_bench_wg_trace"), "libfairdiff_hip.so was built with -DFD_BENCH_HOOKS: it is not the product library"
        common = open(os.path.join(PKG, "csrc", "common.h")).read()
        hooked, inert = "static inline const char* bench_env(const char* name) { return getenv(name); }", "static inline const char* bench_env(const char*) { return nullptr; }"
        assert "#ifdef FD_BENCH_HOOKS" in common and 0 < common.index(hooked) < common.index(inert), "bench_env is no longer inert in product builds"
        src = open(os.path.join(PKG, "csrc", "gemm.hip")).read()
        assert 'bench_env("FD_GEMM_SKINNY_RT")' in src and 'bench_env("FD_GEMM_W8")' in src
    # The ping-pong policy.  FD_GEMM_PP_DEFAULT can be overridden with -D (it sits behind #ifndef) and FD_GEMM_PP is read by a plain getenv that exists only
    # under #ifdef FD_BENCH_HOOKS (pp_mode(), not bench_env): so the BUILT library is asked first, through fd_gemm_kernel_name, which prints pp_mode()'s bits --
    # bit 4 as the last template argument, bits 2 / 16 / 64 as whether a dense 256x320, a dense 128x320 or a split-K problem lands on a ping-pong kernel.  The
    # absence of fd_bench_wg_trace above (exported under the same macro) is what rules FD_GEMM_PP out; the parsed default below is the second witness.
    by_id = {c.id: c for c in gemm_cases.CASES}
    for cid in ("pp256 dense", "conv pp256", "conv pp128"):
        assert _query(L, by_id[cid])[0].endswith(", true>"), f"{cid}: the built library's policy has bit 4 (s_setprio) off"
    for cid, bit in (("big256x320", 2), ("big128x320", 16), ("split-K 128x320", 64)):
        assert _query(L, by_id[cid])[0].startswith("gemm_big_kernel"), f"{cid}: the built library's policy has bit {bit} on: the ping-pong kernel takes it"
    bits = _pp_default_policy()
    assert bits & 4, "policy bit 4 (s_setprio) is off: the <..., false> ping-pong kernels are reachable and need cases"
    assert not bits & 16 and not bits & 2 and not bits & 64, "dense GEMMs / split-K on the ping-pong tiles are now in the policy: they need cases"
    # 16 waves for dense problems only: no conv or phase-pair case on the 256x320 tile may answer a 16-wave kernel
    for c in gemm_cases.CASES:
        if c.conv and "<256, 320" in c.kernel:
            assert "<256, 320, 2, 4," in _query(L, c)[0], c.id
    for s, why in gemm_cases.UNREACHED.items():
        pattern = {"skinny_rt2": r"gemm_skinny_kernel<\d, \d, 2>$", "w8": r"gemm_big_kernel<(128, 320, 2, 4, \d|256, 320, 2, 4, [03])>$",
                   "conv_16_waves": r"gemm_big_kernel<256, 320, 4, 4, [1246]>$", "pp_no_prio": r"gemm_pp_kernel<\d+, \d, false>$",
                   "pp128_dense": r"gemm_pp_kernel<128, [02], true>$"}[why]
        assert re.match(pattern, s), f"{s}: the reason {why!r} does not describe this symbol"
