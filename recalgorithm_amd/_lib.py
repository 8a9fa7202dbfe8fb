"""ctypes binding of librecalgo_hip.so (the C-ABI declared in include/recalgo.h, include/recalgo_cgc.h,
include/recalgo_wide.h and include/recalgo_bst.h).

The product path has NO CPU fallback: if the shared library is missing or a symbol
declared in the header is absent, loading raises immediately.
"""
from __future__ import annotations

import ctypes
import os

from . import _abi
from ._abi import RecalgoError  # noqa: F401  (raised here and by every caller as _lib.RecalgoError)

_HERE = os.path.dirname(os.path.abspath(__file__))
# (RECALGO_HIP_LIB: a developer switch — A/B runs of differently tuned builds of the same library on one GPU box)
LIB_PATH = os.environ.get("RECALGO_HIP_LIB") or os.path.join(_HERE, "librecalgo_hip.so")

P = ctypes.c_void_p  # device pointer / stream

# include/recalgo.h is the one statement of the ABI: signatures, struct layouts, constants and the version are read from it
ABI = _abi.read("recalgo.h")
SIGNATURES = ABI.functions  # name -> (restype, argtypes) of every function of the header
STRUCTS = ABI.structs  # recalgo_*_t -> ctypes.Structure subclass
CONSTANTS = ABI.constants  # RECALGO_* -> int
ABI_VERSION = CONSTANTS["RECALGO_ABI_VERSION"]  # (bumped on any signature change)
# include/recalgo_cgc.h: the second header of the same library (PLE's CGC block), with a version of its own
ABI_CGC = _abi.read("recalgo_cgc.h")
ABI_CGC_VERSION = ABI_CGC.constants["RECALGO_CGC_ABI_VERSION"]
# include/recalgo_wide.h: the third header (Wide&Deep's crossed wide column + FTRL), with a version of its own
ABI_WIDE = _abi.read("recalgo_wide.h")
ABI_WIDE_VERSION = ABI_WIDE.constants["RECALGO_WIDE_ABI_VERSION"]
# include/recalgo_bst.h: the fourth header (BST's transformer block), with a version of its own
ABI_BST = _abi.read("recalgo_bst.h")
ABI_BST_VERSION = ABI_BST.constants["RECALGO_BST_ABI_VERSION"]

_lib = None


def launch_errcheck(name: str):
    """The ctypes errcheck of a kernel-launching entry (the header's contract: it returns hipError_t): a failed launch raises."""
    def errcheck(rc, func=None, args=None):
        check(rc, name)
        return rc
    return errcheck


def load(path: str = LIB_PATH) -> ctypes.CDLL:
    """Load the HIP library (once).  Import torch first so that the process-wide HIP
    runtime (libamdhip64.so.7) is the one torch already mapped."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(path):
        raise RecalgoError(
            f"{path} not found: build it with `python -m recalgorithm_amd.build` "
            "(there is no CPU fallback for the hot path)")
    import torch  # noqa: F401  (maps torch's libamdhip64 before ours resolves its NEEDED)
    lib = ctypes.CDLL(path, mode=ctypes.RTLD_GLOBAL)
    for abi in (ABI, ABI_CGC, ABI_WIDE, ABI_BST):
        for name, (res, args) in abi.functions.items():
            try:
                fn = getattr(lib, name)
            except AttributeError as e:
                raise RecalgoError(f"{path} does not export {name}") from e
            fn.restype = res
            fn.argtypes = args
            if name in abi.launches:
                fn.errcheck = launch_errcheck(name)
    for what, got, want in (("ABI", lib.recalgo_abi_version(), ABI_VERSION),
                            ("CGC ABI", lib.recalgo_cgc_abi_version(), ABI_CGC_VERSION),
                            ("WIDE ABI", lib.recalgo_wide_abi_version(), ABI_WIDE_VERSION),
                            ("BST ABI", lib.recalgo_bst_abi_version(), ABI_BST_VERSION)):
        if got != want:
            raise RecalgoError(f"{path}: {what} version {got}, this binding expects {want} "
                               "(a stale build: python -m recalgorithm_amd.build)")
    _lib = lib
    return lib


def check(rc: int, what: str) -> None:
    if rc != 0:
        raise RecalgoError(f"{what} failed with hipError_t={rc}")
