"""Static inspection of the gfx950 code objects inside a built libfairdiff_hip*.so (build-time / test-time tool, no GPU needed):
splits the library's .hip_fatbin into its per-translation-unit offload bundles, unbundles the gfx950 ELF of each and returns the
disassembly and the kernel resource notes.  Used by tests/test_cpu.py to hold two build invariants: no packed-fp32 VALU instruction in any
shipped kernel ("the round-3 hazard"), and the register / scratch budgets of the hot kernels.
``python codeobj.py --diff [--renamed-ok] OLD.so NEW.so [REGEX]`` compares two builds kernel by kernel (how a refactor shows that it left the ISA
alone) and exits 1 if any kernel symbol -- or, with REGEX, any symbol it matches -- differs or exists on one side only.  A symbol whose instructions
are the same once register numbers are masked, with equal resource notes, is ``renamed``: it counts as a difference unless --renamed-ok is given."""
import os
import re
import subprocess
import tempfile

LLVM = "/opt/rocm/lib/llvm/bin"
MAGIC = b"__CLANG_OFFLOAD_BUNDLE__"


def code_objects(lib_path):
    """-> list of (index, path of the gfx950 ELF) extracted into a temporary directory (kept for the life of the process)."""
    tmp = tempfile.mkdtemp(prefix="fd_codeobj_")
    fat = os.path.join(tmp, "fat.bin")
    subprocess.run([f"{LLVM}/llvm-objcopy", "--dump-section", f".hip_fatbin={fat}", lib_path, os.path.join(tmp, "discard.so")], check=True)
    data = open(fat, "rb").read()
    idx, i = [], data.find(MAGIC)
    while i >= 0:
        idx.append(i)
        i = data.find(MAGIC, i + 1)
    idx.append(len(data))
    out = []
    for k in range(len(idx) - 1):
        b = os.path.join(tmp, f"b{k}.bin")
        open(b, "wb").write(data[idx[k]:idx[k + 1]])
        targets = subprocess.run([f"{LLVM}/clang-offload-bundler", "--list", "--type=o", f"--input={b}"], capture_output=True, text=True, check=True).stdout.split()
        t = [x for x in targets if "gfx950" in x]
        if not t:
            continue
        co = os.path.join(tmp, f"k{k}.co")
        subprocess.run([f"{LLVM}/clang-offload-bundler", "--unbundle", "--type=o", f"--input={b}", f"--targets={t[0]}", f"--output={co}"], check=True)
        out.append((k, co))
    return out


def disassembly(co):
    return subprocess.run([f"{LLVM}/llvm-objdump", "-d", co], capture_output=True, text=True, check=True).stdout


def kernel_resources(co):
    """-> {kernel name: dict(vgpr=, agpr=, sgpr=, scratch=, lds=)} from the code object's metadata notes."""
    notes = subprocess.run([f"{LLVM}/llvm-readelf", "--notes", co], capture_output=True, text=True, check=True).stdout
    res = {}
    for blk in notes.split("- .agpr_count:")[1:]:
        def f(key, blk=blk):
            m = re.search(rf"\.{key}:\s+(\S+)", blk)
            return m.group(1) if m else None
        res[f("name")] = dict(agpr=int(blk.split()[0]), vgpr=int(f("vgpr_count")), sgpr=int(f("sgpr_count")), scratch=int(f("private_segment_fixed_size")),
                              lds=int(f("group_segment_fixed_size")))
    return res


PACKED_F32 = re.compile(r"\bv_pk_(add|mul|fma)_f32\b")


def packed_f32_sites(lib_path):
    """-> list of (kernel symbol, instruction text) for every packed-fp32 VALU instruction in the library's gfx950 code."""
    sites = []
    for _, co in code_objects(lib_path):
        cur = None
        for ln in disassembly(co).splitlines():
            m = re.match(r"^[0-9a-f]+ <(\S+)>:", ln)
            if m:
                cur = m.group(1)
            elif PACKED_F32.search(ln):
                sites.append((cur, ln.strip().split("//")[0].strip()))
    return sites


_SYMBOL = re.compile(r"^[0-9a-f]+ <(\S+)>:")
_ADDRESS = re.compile(r"^\s*[0-9a-f]+:\s+")


def kernel_instructions(lib_path):
    """-> {kernel symbol: instruction text} over all gfx950 code objects of the library: the disassembly split at the ``<symbol>:`` lines, one
    instruction per line, address column and trailing ``//`` comments (address + encoding) stripped."""
    out = {}
    for _, co in code_objects(lib_path):
        cur = None
        for ln in disassembly(co).splitlines():
            m = _SYMBOL.match(ln)
            if m:
                cur = out.setdefault(m.group(1), [])
            elif cur is not None:
                ln = _ADDRESS.sub("", ln.split("//")[0]).strip()
                if ln:
                    cur.append(ln)
    return {k: "\n".join(v) for k, v in out.items()}


def _strip_signature(demangled):
    """``void gemm_big_kernel<256, 320, 4, 4, 0>(fd_gemm_desc, int, int, int)`` -> ``gemm_big_kernel<256, 320, 4, 4, 0>``: the return type of a template
    instantiation and the parameter list -- the LAST balanced parenthesis group -- dropped."""
    name = demangled.strip()
    if name.endswith(")"):
        depth = 0
        for k in range(len(name) - 1, -1, -1):
            depth += (name[k] == ")") - (name[k] == "(")
            if depth == 0:
                name = name[:k]
                break
    return name[5:] if name.startswith("void ") else name


def kernel_symbols(lib_path, only=None):
    """-> sorted demangled kernel names of the library's gfx950 code objects, template arguments included and the parameter list dropped
    (``gemm_big_kernel<256, 320, 4, 4, 0>``: how fd_gemm_kernel_name and rocprofv3 spell them).  ``only``: a regular expression the name must match.
    A kernel is a function symbol whose mangled name has a kernel descriptor in the metadata notes (``kernel_resources``); its demangled spelling is the
    one ``llvm-objdump -t --demangle`` prints for the function symbol at the SAME ADDRESS."""
    kernels = set()
    func = re.compile(r"^([0-9a-f]+)\s+\S+\s+F\s+\.text\s+[0-9a-f]+\s+(?:\.\w+\s+)?(.*)$")
    for _, co in code_objects(lib_path):
        mangled = set(kernel_resources(co))
        tables = [subprocess.run([f"{LLVM}/llvm-objdump", "-t", *flag, co], capture_output=True, text=True, check=True).stdout for flag in ((), ("--demangle",))]
        at = [{m.group(1): m.group(2) for m in map(func.match, t.splitlines()) if m} for t in tables]
        for addr, sym in at[0].items():
            if sym in mangled:
                name = _strip_signature(at[1][addr])
                if only is None or re.search(only, name):
                    kernels.add(name)
    return sorted(kernels)


# a register operand: v12, s5, a3, v[18:21], s[4:5], a[0:15]
_REGISTER = re.compile(r"\b[vsa](?:\d+|\[\d+:\d+\])(?![\w\[])")


def mask_registers(text):
    """Instruction text with every register operand replaced by one placeholder: equal for two allocations of the same instruction sequence."""
    return _REGISTER.sub("R", text)


def diff(old_lib, new_lib, only=None, renamed_ok=False):
    """Prints, per kernel symbol, identical / renamed / differs (instruction counts, resources) / only in OLD|NEW; -> number of symbols that are not
    identical or exist on one side only.  ``renamed``: same instructions once register operands are masked and the same resource notes; counted
    unless ``renamed_ok``.  ``only``: a regular expression; symbols it does not match anywhere are left out of the comparison."""
    old, new = kernel_instructions(old_lib), kernel_instructions(new_lib)
    if only:
        old, new = ({k: v for k, v in d.items() if re.search(only, k)} for d in (old, new))
    res = {}
    for tag, lib in (("old", old_lib), ("new", new_lib)):
        for _, co in code_objects(lib):
            for n, r in kernel_resources(co).items():
                res[tag, n] = r
    bad = renamed = 0
    for sym in sorted(set(old) | set(new)):
        if sym not in new or sym not in old:
            verdict = "only in OLD" if sym in old else "only in NEW"
        elif old[sym] == new[sym]:
            verdict = "identical"
        elif mask_registers(old[sym]) == mask_registers(new[sym]) and res.get(("old", sym)) == res.get(("new", sym)):
            verdict = "renamed"
        else:
            verdict = f"differs ({old[sym].count(chr(10)) + 1} -> {new[sym].count(chr(10)) + 1} instructions)  old {res.get(('old', sym))}  new {res.get(('new', sym))}"
        renamed += verdict == "renamed"
        bad += verdict != "identical" and not (renamed_ok and verdict == "renamed")
        print(f"{verdict:12s} {sym}" if verdict in ("identical", "renamed") else f"{sym}: {verdict}")
    print(f"{len(old)} -> {len(new)} kernel symbols{f' matching {only!r}' if only else ''}, {bad} not identical or on one side only"
          + (f"; {renamed} renamed (registers only, {'accepted' if renamed_ok else 'counted'})" if renamed else ""))
    return bad


if __name__ == "__main__":
    import sys
    if sys.argv[1:2] == ["--diff"]:
        args = [x for x in sys.argv[2:] if x != "--renamed-ok"]
        if len(args) not in (2, 3):
            sys.exit("usage: codeobj.py --diff [--renamed-ok] OLD.so NEW.so [REGEX]")
        sys.exit(1 if diff(*args, renamed_ok="--renamed-ok" in sys.argv[2:]) else 0)
    for lib in sys.argv[1:]:
        s = packed_f32_sites(lib)
        print(f"{lib}: {len(s)} packed-fp32 VALU instructions" + (f", e.g. {s[0]}" if s else ""))
        for _, co in code_objects(lib):
            for n, r in kernel_resources(co).items():
                if r["scratch"]:
                    print(f"   scratch {r['scratch']:4d} B  vgpr {r['vgpr']:3d}  {n}")
