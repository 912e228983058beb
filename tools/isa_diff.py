#!/usr/bin/env python3
"""Developer tool: do two trees compile the same gfx950 machine code?  The check of a refactor, without a GPU.

    python tools/isa_diff.py PARENT_TREE HEAD_TREE vbq_amd/csrc/vbq_notebook.hip [more sources] [-DVBQ_ONLY_N10]
    python tools/isa_diff.py PARENT_TREE HEAD_TREE --a-sources vbq_amd/csrc/a.hip,... --b-sources vbq_amd/csrc/b.hip,...

PARENT_TREE is a checkout of the parent OUTSIDE the repository (`git worktree add DIR REV`, or `git archive REV | tar -x
-C DIR`).  Each source (a path relative to a tree's root) is compiled device-only to assembly in both trees with the flags
of vbq_amd/build.py (HIPCC_FLAGS + extra_flags()) and each tree's own include directories.  Arguments that start with
`-` go to both compilations; --a-flags / --b-flags to one side.  The output is split per function; comments, .loc /
.file / .ident lines and the __hip_cuid_* symbol are dropped and local labels renamed by order of appearance.  One line
per kernel (and per out-of-line device function): `identical`, or the number of differing lines and the descriptor
fields of both sides.  --show SUBSTRING also prints the unified diff of the functions whose name contains it.
The exit status is 1 when anything differs.  Texts are compared; no instruction is looked for.
With --a-sources / --b-sources (comma-separated) the functions of each side are pooled over its list before they are paired:
the form for a refactor that moves functions between files, whose mangled names do not depend on the file that holds them.
A name defined twice on one side is an error.
"""
import argparse
import difflib
import os
import re
import shlex
import shutil
import subprocess
import sys
import tempfile
from concurrent.futures import ThreadPoolExecutor

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from vbq_amd.build import HIPCC_FLAGS, extra_flags  # noqa: E402

FIELDS = [("VGPRs", "next_free_vgpr"), ("SGPRs", "next_free_sgpr"), ("LDS", "group_segment_fixed_size"),
          ("scratch", "private_segment_fixed_size"), ("accum", "accum_offset")]


def compile_asm(tree, src, flags):
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    with tempfile.TemporaryDirectory() as tmp:
        out = os.path.join(tmp, "out.s")
        cmd = [hipcc] + HIPCC_FLAGS + flags + ["-I", os.path.join(tree, "include"), "-I", os.path.join(tree, "vbq_amd", "csrc"),
                                               "--cuda-device-only", "-S", os.path.join(tree, src), "-o", out]
        r = subprocess.run(cmd, capture_output=True, text=True)
        if r.returncode:
            sys.exit(f"hipcc failed on {os.path.join(tree, src)}:\n{r.stdout}{r.stderr}")
        return open(out).read()


def split(asm):
    """{mangled name: (body lines, descriptor lines or None)} of one assembly file, normalised."""
    bodies, descs, funcs, cur, desc = {}, {}, set(), None, None
    for line in asm.splitlines():
        s = line.split(";", 1)[0].strip()
        if not s or s.startswith((".loc", ".file", ".ident", ".cfi_")) or "__hip_cuid_" in s:
            continue
        if desc is not None:
            if s == ".end_amdhsa_kernel":
                desc = None
            else:
                descs[desc].append(s)
            continue
        if s.startswith(".amdhsa_kernel "):
            desc = s.split()[1]
            descs[desc] = []
            continue
        if cur is None:
            m = re.match(r"^\.type\s+([\w$.]+),@function$", s)
            if m:
                funcs.add(m.group(1))
            elif s.endswith(":") and s[:-1] in funcs:
                cur = s[:-1]
                bodies[cur] = []
            continue
        if s.startswith(".Lfunc_end"):
            cur = None
            continue
        bodies[cur].append(s)
    out = {}
    for name, body in bodies.items():
        labels = {}
        ren = lambda m: labels.setdefault(m.group(0), f".L{len(labels)}")
        out[name] = ([re.sub(r"\.L[\w$.]+", ren, s) for s in body], descs.get(name))
    return out


def count_diff(a, b):
    lo = 0
    while lo < len(a) and lo < len(b) and a[lo] == b[lo]:
        lo += 1
    hi = 0
    while hi < len(a) - lo and hi < len(b) - lo and a[-1 - hi] == b[-1 - hi]:
        hi += 1
    a, b = a[lo:len(a) - hi], b[lo:len(b) - hi]
    sm = difflib.SequenceMatcher(None, a, b)
    return sum(max(i2 - i1, j2 - j1) for op, i1, i2, j1, j2 in sm.get_opcodes() if op != "equal")


def fields(desc):
    if desc is None:
        return "no descriptor (a device function)"
    d = dict(s[len(".amdhsa_"):].split(None, 1) for s in desc if s.startswith(".amdhsa_") and len(s.split()) > 1)
    return ", ".join(f"{label} {d.get(key, '-')}" for label, key in FIELDS)


def demangle(names):
    cxxfilt = shutil.which("c++filt") or shutil.which("llvm-cxxfilt")
    if not cxxfilt or not names:
        return {n: n for n in names}
    r = subprocess.run([cxxfilt], input="\n".join(names), capture_output=True, text=True)
    # the name with its template arguments; the parameter list and the namespaces only lengthen the line
    dem = [re.sub(r"^.*?vbq::|\(.*", "", d.replace("(anonymous namespace)::", "")) for d in r.stdout.splitlines()]
    return dict(zip(names, dem)) if len(dem) == len(set(dem)) == len(names) else {n: n for n in names}


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("tree_a")
    ap.add_argument("tree_b")
    ap.add_argument("sources", nargs="*")
    ap.add_argument("--a-sources", default="")
    ap.add_argument("--b-sources", default="")
    ap.add_argument("--a-flags", default="")
    ap.add_argument("--b-flags", default="")
    ap.add_argument("--show", default=None)
    args, common = ap.parse_known_args()
    if any(not f.startswith("-") for f in common):
        ap.error("unknown arguments: " + " ".join(common))
    trees = [os.path.abspath(args.tree_a), os.path.abspath(args.tree_b)]
    side_flags = [shlex.split(args.a_flags), shlex.split(args.b_flags)]
    pools = [[s for s in p.split(",") if s] for p in (args.a_sources, args.b_sources)]
    if bool(pools[0]) != bool(pools[1]) or bool(pools[0]) == bool(args.sources):
        ap.error("give sources to compare file by file, or --a-sources and --b-sources to compare them pooled")
    # one comparison per source, or ONE of everything side A defines against everything side B defines
    groups = [(" + ".join(pools[0]) + " | " + " + ".join(pools[1]), pools)] if pools[0] else [(s, ([s], [s])) for s in args.sources]
    jobs = [(t, s, extra_flags() + common + f) for _, sides in groups for t, f, srcs in zip(trees, side_flags, sides) for s in srcs]
    with ThreadPoolExecutor(max_workers=min(8, os.cpu_count() or 1, len(jobs))) as ex:
        asms = iter(list(ex.map(lambda j: split(compile_asm(*j)), jobs)))
    differ = 0
    for title, sides in groups:
        fa, fb = {}, {}
        for pooled, srcs in zip((fa, fb), sides):
            for src in srcs:
                funcs = next(asms)
                twice = sorted(set(funcs) & set(pooled))
                if twice:
                    sys.exit(f"{src}: defined in another source of the same side as well: {', '.join(twice)}")
                pooled.update(funcs)
        names = list(fa) + [n for n in fb if n not in fa]
        dem = demangle(names)
        print(f"== {title}: {len(names)} functions")
        for n in names:
            if n not in fa or n not in fb:
                differ += 1
                print(f"{dem[n]}: only in {'A' if n in fa else 'B'}")
                continue
            (ba, da), (bb, db) = fa[n], fb[n]
            if ba == bb and da == db:
                print(f"{dem[n]}: identical ({len(ba)} lines)")
                continue
            differ += 1
            print(f"{dem[n]}: {count_diff(ba, bb)} lines differ ({len(ba)} -> {len(bb)});  A: {fields(da)};  B: {fields(db)}")
            if args.show is not None and args.show in dem[n]:
                print("\n".join(difflib.unified_diff(ba, bb, "A", "B", lineterm="", n=2)))
    return 1 if differ else 0


if __name__ == "__main__":
    sys.exit(main())
