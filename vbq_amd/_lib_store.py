"""ctypes binding of libvbq_store.so (vbq_amd/store/vbq_store.h), the package's fifth native library.  No CPU fallback exists:
if the library is missing or fails to load, every op that needs it raises."""
from __future__ import annotations

import ctypes as C
import os

from ._lib import OK, VBQError

_LIB = None

ABI_VERSION = 1

# name -> (restype, argtypes); mirrors vbq_amd/store/vbq_store.h one to one (tests/test_store_host.py checks it)
SIGNATURES = {
    "vbqs_abi_version": (C.c_int, []),
    "vbqs_last_error": (C.c_char_p, []),
    "vbqs_plan_boxes": (C.c_int, [C.c_void_p, C.c_int32, C.c_int32, C.c_void_p, C.c_void_p, C.c_int64, C.c_int64, C.c_int64,
                                  C.c_int64, C.c_int32, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
}


def library_path() -> str:
    from . import build as _build
    return os.environ.get("VBQ_STORE_LIBRARY", _build.STORE_LIB)


def lib():
    """Load (once) and return the ctypes handle.  Raises VBQError when the library has not been built -- there is
    deliberately no slower path to fall back to."""
    global _LIB
    if _LIB is not None:
        return _LIB
    path = library_path()
    if not os.path.exists(path):
        raise VBQError(f"HIP extension not built: {path} is missing. Run `python -m vbq_amd.build` "
                       "(needs hipcc; cross-compiles gfx950 without a GPU).")
    try:
        h = C.CDLL(path)
    except OSError as e:
        raise VBQError(f"cannot load {path}: {e}") from e
    for name, (res, args) in SIGNATURES.items():
        try:
            fn = getattr(h, name)
        except AttributeError as e:
            raise VBQError(f"{path} does not export {name}; rebuild with `python -m vbq_amd.build --force`") from e
        fn.restype = res
        fn.argtypes = args
    if h.vbqs_abi_version() != ABI_VERSION:
        raise VBQError(f"{path}: ABI version {h.vbqs_abi_version()} != {ABI_VERSION}; rebuild with `python -m vbq_amd.build --force`")
    _LIB = h
    return h


def check(status: int, what: str):
    if status != OK:
        msg = lib().vbqs_last_error().decode("utf-8", "replace")
        raise VBQError(f"{what} failed ({status}): {msg}")
