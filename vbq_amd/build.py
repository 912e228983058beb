"""Build the HIP extension (and, for tests only, the C oracle) in-tree.

    python -m vbq_amd.build            # libvbq_hip.so, libvbq_ext.so, libvbq_budget.so, libvbq_kmeans.so and libvbq_store.so for gfx950
    python -m vbq_amd.build --oracle   # also oracle/_build/libvbq_oracle.so

hipcc cross-compiles gfx950 without a GPU; the resulting .so is git-ignored but travels
with the working tree to the GPU box.
"""
from __future__ import annotations

import os
import shutil
import subprocess
import sys

PKG = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(PKG)
CSRC = os.path.join(PKG, "csrc")
LIBDIR = os.path.join(PKG, "lib")
LIB = os.path.join(LIBDIR, "libvbq_hip.so")
INCLUDE = os.path.join(ROOT, "include")
HIP_SOURCES = ["vbq_api.hip", "vbq_quantize.hip", "vbq_quantize_fast.hip", "vbq_hist.hip", "vbq_notebook.hip", "vbq_bmshj.hip",
               "vbq_candidates.hip", "vbq_latents.hip", "vbq_host.hip", "vbq_rans.hip", "vbq_comm.hip", "vbq_xi.hip", "vbq_baselines.hip", "vbq_ranks.hip", "vbq_metrics.hip",
               "vbq_budget.hip", "vbq_reduce.hip", "vbq_transpose.hip", "vbq_rans_il.hip", "vbq_records.hip", "vbq_topk.hip", "vbq_bag.hip", "vbq_rans_map.hip", "vbq_rans_window.hip", "vbq_rans_map_window.hip",
               "vbq_rans_files.hip", "vbq_rans_sizes_files.hip", "vbq_rans_il_files.hip", "vbq_rans_map_files.hip",
               "vbq_rans_map_rates_files.hip"]
EXT = os.path.join(PKG, "ext")
EXT_LIB = os.path.join(LIBDIR, "libvbq_ext.so")
BUDGET = os.path.join(PKG, "budget")
BUDGET_LIB = os.path.join(LIBDIR, "libvbq_budget.so")
KMEANS = os.path.join(PKG, "kmeans")
KMEANS_LIB = os.path.join(LIBDIR, "libvbq_kmeans.so")
STORE = os.path.join(PKG, "store")
STORE_LIB = os.path.join(LIBDIR, "libvbq_store.so")
LINK_LIBS = ["-ldl"]
HIPCC_FLAGS = ["--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC",
               # every f32/f64 op of the reference is a separately rounded op: never contract a*b+c
               "-ffp-contract=off", "-fno-fast-math",
               # no SLP vectorisation: the v_pk_add/mul_f32 pairs it forms issue at the rate of two scalar ops but need
               # their operands in aligned register pairs -- the moves cost K1t 3 %, K1e 5 %, the one-lambda kernel 7 %
               "-fno-slp-vectorize"]
EXT_HIPCC_FLAGS = HIPCC_FLAGS + ["-fvisibility=hidden"]


def _newer(target, deps):
    if not os.path.exists(target):
        return True
    t = os.path.getmtime(target)
    return any(os.path.getmtime(d) > t for d in deps)


def hip_sources():
    return [os.path.join(CSRC, s) for s in HIP_SOURCES if os.path.exists(os.path.join(CSRC, s))]


def hip_headers():
    """Every header an object depends on: a change to any of them rebuilds every object."""
    import glob
    return sorted(glob.glob(os.path.join(CSRC, "*.h"))) + [os.path.join(INCLUDE, "vbq.h")]


def _tmp(path):
    # several ranks (or threads) may find a stale library at the same time: every builder writes its own temporary
    # file and installs it with an atomic rename, so a reader never sees a half-written object or library
    import threading
    return f"{path}.{os.getpid()}.{threading.get_ident()}.tmp"


def _compile_one(hipcc, src, obj, extra, flags=None):
    tmp = _tmp(obj)
    cmd = [hipcc] + (HIPCC_FLAGS if flags is None else flags) + extra + ["-I", INCLUDE, "-I", CSRC, "-c", src, "-o", tmp]
    r = subprocess.run(cmd, capture_output=True, text=True)
    if r.returncode != 0:
        raise RuntimeError("hipcc failed on " + os.path.basename(src) + ":\n" + r.stdout + r.stderr)
    os.replace(tmp, obj)
    return " ".join(cmd)


def extra_flags():
    extra = os.environ.get("VBQ_EXTRA_HIPCC_FLAGS", "").split()       # developer experiments only
    if os.environ.get("VBQ_ONLY_N10") == "1":   # the reference's bit depth alone (post_process.py:117): a third of the build time
        extra.append("-DVBQ_ONLY_N10")
    return extra


def _build_library(lib, srcs, headers, objdir, flags, force, verbose):
    """One object per source under `objdir` (rebuilt only when it or a header changed, in parallel), one link into `lib`; the
    flags the library was built with are written beside it as <name>.flags.txt -- flags.txt for libvbq_hip.so."""
    from concurrent.futures import ThreadPoolExecutor
    extra = extra_flags()
    flags_tag = os.path.join(objdir, "flags.txt")
    # travels with the library (the object cache does not): flags.txt, vbq_ext.flags.txt, vbq_budget.flags.txt, vbq_kmeans.flags.txt,
    # vbq_store.flags.txt
    lib_tag = os.path.join(LIBDIR, "flags.txt" if lib == LIB else os.path.basename(lib)[3:-3] + ".flags.txt")
    tag = " ".join(flags + extra)
    # A tree that arrived with its library but without the object cache (the GPU box: vbq_amd/lib/obj is not shipped) is up
    # to date when the library is newer than every source AND was built with these flags: nothing to do, and nothing
    # that needs hipcc.
    if not force and not os.path.isdir(objdir) and not _newer(lib, srcs + headers) and \
            os.path.exists(lib_tag) and open(lib_tag).read() == tag:
        return lib
    os.makedirs(objdir, exist_ok=True)
    if not os.path.exists(flags_tag) or open(flags_tag).read() != tag:
        force = True
    objs = [os.path.join(objdir, os.path.basename(s)[:-4] + ".o") for s in srcs]
    todo = [(s, o) for s, o in zip(srcs, objs) if force or _newer(o, [s] + headers)]
    if not todo and not _newer(lib, objs) and os.path.exists(lib_tag) and open(lib_tag).read() == tag:
        return lib
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    if not os.path.exists(hipcc):
        raise RuntimeError("hipcc not found: cannot build " + os.path.basename(lib) + " (ROCm toolchain required)")
    with ThreadPoolExecutor(max_workers=min(8, os.cpu_count() or 1)) as ex:
        for line in ex.map(lambda so: _compile_one(hipcc, so[0], so[1], extra, flags), todo):
            if verbose:
                print(line)
    open(flags_tag, "w").write(tag)
    tmp = _tmp(lib)
    cmd = [hipcc, "--offload-arch=gfx950", "-shared", "-fPIC"] + objs + LINK_LIBS + ["-o", tmp]
    if verbose:
        print(" ".join(cmd))
    r = subprocess.run(cmd, capture_output=True, text=True)
    if r.returncode != 0:
        raise RuntimeError("link failed:\n" + r.stdout + r.stderr)
    os.replace(tmp, lib)
    tmp = _tmp(lib_tag)
    open(tmp, "w").write(tag)
    os.replace(tmp, lib_tag)
    return lib


def build_hip(force: bool = False, verbose: bool = False) -> str:
    """libvbq_hip.so (include/vbq.h): one object per .hip source of vbq_amd/csrc under vbq_amd/lib/obj, one link."""
    return _build_library(LIB, hip_sources(), hip_headers(), os.path.join(LIBDIR, "obj"), HIPCC_FLAGS, force, verbose)


def ext_sources():
    import glob
    return sorted(glob.glob(os.path.join(EXT, "*.hip")))


def build_ext(force: bool = False, verbose: bool = False) -> str:
    """libvbq_ext.so (include/vbq_ext.h): the sources of vbq_amd/ext, with the headers of vbq_amd/csrc on the include path
    and hidden visibility -- only the extern "C" entry points leave the library.  Objects under vbq_amd/lib/obj/ext."""
    headers = hip_headers() + [os.path.join(INCLUDE, "vbq_ext.h")]
    return _build_library(EXT_LIB, ext_sources(), headers, os.path.join(LIBDIR, "obj", "ext"), EXT_HIPCC_FLAGS, force, verbose)


def budget_sources():
    import glob
    return sorted(glob.glob(os.path.join(BUDGET, "*.hip")))


def build_budget(force: bool = False, verbose: bool = False) -> str:
    """libvbq_budget.so (include/vbq_budget.h): the sources of vbq_amd/budget, built as build_ext builds vbq_amd/ext -- the
    headers of vbq_amd/csrc on the include path, hidden visibility.  Objects under vbq_amd/lib/obj/budget."""
    headers = hip_headers() + [os.path.join(INCLUDE, "vbq_budget.h")]
    return _build_library(BUDGET_LIB, budget_sources(), headers, os.path.join(LIBDIR, "obj", "budget"), EXT_HIPCC_FLAGS, force,
                          verbose)


def kmeans_sources():
    import glob
    return sorted(glob.glob(os.path.join(KMEANS, "*.hip")))


def build_kmeans(force: bool = False, verbose: bool = False) -> str:
    """libvbq_kmeans.so (include/vbq_kmeans.h): the sources of vbq_amd/kmeans, built as build_budget builds vbq_amd/budget -- the
    headers of vbq_amd/csrc on the include path, hidden visibility.  Objects under vbq_amd/lib/obj/kmeans."""
    headers = hip_headers() + [os.path.join(INCLUDE, "vbq_kmeans.h")]
    return _build_library(KMEANS_LIB, kmeans_sources(), headers, os.path.join(LIBDIR, "obj", "kmeans"), EXT_HIPCC_FLAGS, force,
                          verbose)


def store_sources():
    import glob
    return sorted(glob.glob(os.path.join(STORE, "*.hip")))


def build_store(force: bool = False, verbose: bool = False) -> str:
    """libvbq_store.so (vbq_amd/store/vbq_store.h, beside its sources): the sources of vbq_amd/store, built as build_kmeans
    builds vbq_amd/kmeans -- the headers of vbq_amd/csrc on the include path, hidden visibility.  Objects under
    vbq_amd/lib/obj/store."""
    headers = hip_headers() + [os.path.join(STORE, "vbq_store.h")]
    return _build_library(STORE_LIB, store_sources(), headers, os.path.join(LIBDIR, "obj", "store"), EXT_HIPCC_FLAGS, force,
                          verbose)


def build_oracle(force: bool = False) -> str:
    """gcc build of oracle/vbq_oracle.c (test infrastructure, never loaded by vbq_amd)."""
    odir = os.path.join(ROOT, "oracle")
    r = subprocess.run(["make", "-C", odir] + (["-B"] if force else []), capture_output=True, text=True)
    if r.returncode != 0:
        raise RuntimeError("oracle build failed:\n" + r.stdout + r.stderr)
    return os.path.join(odir, "_build", "libvbq_oracle.so")


if __name__ == "__main__":
    print(build_hip(force="--force" in sys.argv, verbose=True))
    print(build_ext(force="--force" in sys.argv, verbose=True))
    print(build_budget(force="--force" in sys.argv, verbose=True))
    print(build_kmeans(force="--force" in sys.argv, verbose=True))
    print(build_store(force="--force" in sys.argv, verbose=True))
    if "--oracle" in sys.argv:
        print(build_oracle(force="--force" in sys.argv))
