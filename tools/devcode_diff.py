#!/usr/bin/env python3
"""Is the gfx950 device code of two source trees the same?   tools/devcode_diff.py <tree A> <tree B> [--keep DIR]

For every translation unit of SRCS in <tree>/trieste_amd/csrc/Makefile, with the Makefile's flags: compile device-only,
unbundle the gfx950 code object, take `llvm-objdump -d` and the symbol table, and compare tree A's with tree B's.  The
`__hip_cuid_*` symbol hashes the compile unit and is left out.  A TU whose whole disassembly differs is compared again
kernel by kernel (the order of emission may move when the host code that instantiates the kernels is rearranged): the set
of symbols with their sizes and sections, and every symbol's instructions without their addresses.

Prints one line per TU -- `identical`, `identical per symbol (order of emission moved)` or `DIFFERENT` with what differs --
and exits 0 only if no TU is DIFFERENT.  A host-only refactor of the launch layer must leave every line `identical`."""
import argparse
import os
import re
import subprocess
import sys
import tempfile
from concurrent.futures import ThreadPoolExecutor

ROCM = os.environ.get("ROCM_PATH", "/opt/rocm")
HIPCC = os.path.join(ROCM, "bin", "hipcc")
LLVM = os.path.join(ROCM, "llvm", "bin")


def make_vars(csrc):
    text = open(os.path.join(csrc, "Makefile")).read().replace("\\\n", " ")
    var = {m.group(1): m.group(2).strip() for m in re.finditer(r"^(\w+)\s*\??=\s*(.*)$", text, re.M)}
    flags = var["CXXFLAGS"].replace("$(ARCH)", var.get("ARCH", "gfx950")).replace("$(EXTRA)", "")
    return var["SRCS"].split(), flags.split()


def device_object(csrc, tu, flags, out_dir):
    bundle = os.path.join(out_dir, tu + ".bundle")
    obj = os.path.join(out_dir, tu + ".gfx950.elf")
    subprocess.run([HIPCC, *flags, "--offload-device-only", "-c", tu, "-o", bundle], cwd=csrc, check=True)
    head = open(bundle, "rb").read(24)
    if head.startswith(b"\x7fELF"):
        os.replace(bundle, obj)
    else:
        subprocess.run([os.path.join(LLVM, "clang-offload-bundler"), "--unbundle", "--type=o", "--input=" + bundle,
                        "--targets=hip-amdgcn-amd-amdhsa--gfx950", "--output=" + obj], check=True)
    dis = subprocess.run([os.path.join(LLVM, "llvm-objdump"), "-d", "--no-show-raw-insn", obj], check=True,
                         capture_output=True, text=True).stdout
    sym = subprocess.run([os.path.join(LLVM, "llvm-objdump"), "-t", obj], check=True, capture_output=True, text=True).stdout
    return dis.split("\n", 2)[-1], sym.split("SYMBOL TABLE:")[-1]   # (the first lines name the file)


def symbols(sym, with_values):
    rows = []
    for line in sym.splitlines():
        parts = line.split()
        if not parts or parts[-1].startswith("__hip_cuid_"):
            continue
        rows.append(" ".join(parts if with_values else parts[1:]))   # with or without the address
    return sorted(rows)


def per_symbol(dis):
    """{symbol: its instructions without the trailing `// address: encoding <target>` (branches are relative)"""
    out, name = {}, None
    for line in dis.splitlines():
        m = re.match(r"^[0-9a-f]+ <(.+)>:$", line)
        if m:
            name = m.group(1)
            out[name] = []
        elif name is not None and line.strip():
            out[name].append(re.sub(r"\s*//\s*[0-9A-Fa-f]+:.*$", "", line.strip()))
    return out


def compare(tu, a, b):
    (dis_a, sym_a), (dis_b, sym_b) = a, b
    if dis_a == dis_b and symbols(sym_a, True) == symbols(sym_b, True):
        return "identical", []
    notes = []
    names_a, names_b = symbols(sym_a, False), symbols(sym_b, False)
    if names_a != names_b:
        notes += ["only in A: " + s for s in sorted(set(names_a) - set(names_b))]
        notes += ["only in B: " + s for s in sorted(set(names_b) - set(names_a))]
    pa, pb = per_symbol(dis_a), per_symbol(dis_b)
    for name in sorted(set(pa) & set(pb)):
        if pa[name] != pb[name]:
            notes.append(f"instructions differ: {name} ({len(pa[name])} vs {len(pb[name])})")
    if set(pa) != set(pb):
        notes.append("the sets of disassembled symbols differ")
    return ("DIFFERENT" if notes else "identical per symbol (order of emission moved)"), notes


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("tree_a")
    ap.add_argument("tree_b")
    ap.add_argument("--keep", help="keep the code objects and listings here")
    ap.add_argument("--jobs", type=int, default=8)
    args = ap.parse_args()
    work = args.keep or tempfile.mkdtemp(prefix="devcode_diff_")
    trees = {}
    for tag, tree in (("a", args.tree_a), ("b", args.tree_b)):
        csrc = os.path.join(os.path.abspath(tree), "trieste_amd", "csrc")
        srcs, flags = make_vars(csrc)
        out_dir = os.path.join(work, tag)
        os.makedirs(out_dir, exist_ok=True)
        trees[tag] = (csrc, srcs, flags, out_dir)
    if trees["a"][1] != trees["b"][1] or trees["a"][2] != trees["b"][2]:
        print("the Makefiles' SRCS or CXXFLAGS differ: nothing to compare")
        return 2
    jobs = [(tag, tu) for tag in trees for tu in trees[tag][1]]
    with ThreadPoolExecutor(args.jobs) as pool:
        res = dict(zip(jobs, pool.map(lambda j: device_object(trees[j[0]][0], j[1], trees[j[0]][2], trees[j[0]][3]), jobs)))
    bad = 0
    for tu in trees["a"][1]:
        verdict, notes = compare(tu, res[("a", tu)], res[("b", tu)])
        nsym = len(symbols(res[("b", tu)][1], False))
        print(f"{tu:36s} {nsym:4d} symbols  {verdict}")
        for n in notes[:20]:
            print("    " + n)
        bad += verdict == "DIFFERENT"
    print("device code: " + ("DIFFERENT in %d translation unit(s)" % bad if bad else "the same in every translation unit"))
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
