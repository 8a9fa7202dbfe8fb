"""ctypes binding of librecalgo_hip.so (the C-ABI declared in the headers that HEADERS, MORE_HEADERS and SERVING_HEADERS below list).  The
product path has NO CPU fallback: if the shared library is missing or a symbol declared in a header is absent, loading
raises immediately."""
from __future__ import annotations

import ctypes
import os
import re

from . import _abi
from ._abi import RecalgoError  # noqa: F401  (raised here and by every caller as _lib.RecalgoError)

_HERE = os.path.dirname(os.path.abspath(__file__))
# (RECALGO_HIP_LIB: a developer switch — A/B runs of differently tuned builds of the same library on one GPU box)
LIB_PATH = os.environ.get("RECALGO_HIP_LIB") or os.path.join(_HERE, "librecalgo_hip.so")

P = ctypes.c_void_p  # device pointer / stream


def _versioned(header: str):
    """_abi.read(header) with what load() checks of it: .version, the header's ONE `RECALGO_[<KEY>_]ABI_VERSION` constant;
    .version_query, the one `recalgo_[<key>_]abi_version` function that returns it; .label, its name in error messages."""
    abi = _abi.read(header)
    defines = [c for c in abi.constants if re.fullmatch(r"RECALGO_(?:[A-Z0-9]+_)?ABI_VERSION", c)]
    queries = [f for f in abi.functions if re.fullmatch(r"recalgo_(?:[a-z0-9]+_)?abi_version", f)]
    if len(defines) != 1 or queries != [defines[0].lower()]:
        raise RecalgoError(f"include/{header}: a header of HEADERS has exactly one RECALGO_[<KEY>_]ABI_VERSION define and the "
                           f"one function recalgo_[<key>_]abi_version of the same key; found {defines} and {queries}")
    abi.version, abi.version_query = abi.constants[defines[0]], queries[0]
    abi.label = defines[0][len("RECALGO_"):-len("_VERSION")].replace("_", " ")       # `ABI`, `CGC ABI`, ..
    return abi


# The headers of the HIP library, each the one statement of its part of the ABI (signatures, struct layouts, constants, a
# version of its own, bumped on any signature change).  Three tables, one meaning: HEADERS is the list the host tests of the
# first five features pin by length and order, MORE_HEADERS (and all_headers(), the two as one) the list DIEN's host tests pin
# the same way, so both stay as those tests state them; a header added since is one more entry of SERVING_HEADERS, which no
# test pins by length.  load() and scripts/abi_record.py walk all three (every_header()).
HEADERS = {h: _versioned(h) for h in ("recalgo.h", "recalgo_cgc.h", "recalgo_wide.h", "recalgo_bst.h",
                                              "recalgo_res.h")}
MORE_HEADERS = {"recalgo_dien.h": _versioned("recalgo_dien.h")}
SERVING_HEADERS = {h: _versioned(h) for h in ("recalgo_serve.h", "recalgo_metrics.h", "recalgo_sumstep.h",
                                                      "recalgo_ragged.h", "recalgo_afm.h", "recalgo_feed.h", "recalgo_ffm.h",
                                                      "recalgo_autoint.h", "recalgo_dcnv2.h", "recalgo_flen.h",
                                                      "recalgo_gauc.h", "recalgo_esmm.h", "recalgo_maskmetrics.h")}
ABI = HEADERS["recalgo.h"]  # the first header's tables, under the names the product uses:
SIGNATURES = ABI.functions  # name -> (restype, argtypes) of every function of the header
STRUCTS = ABI.structs  # recalgo_*_t -> ctypes.Structure subclass
CONSTANTS = ABI.constants  # RECALGO_* -> int
ABI_VERSION = ABI.version
_lib = None  # the loaded library


def all_headers() -> dict:
    """HEADERS and MORE_HEADERS as one table, in that order (read at call time: a test may replace either)."""
    return {**HEADERS, **MORE_HEADERS}


def every_header() -> dict:
    """Every header of the library: all_headers() and SERVING_HEADERS, in that order (read at call time, as all_headers())."""
    return {**all_headers(), **SERVING_HEADERS}


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
        raise RecalgoError(f"{path} not found: build it with `python -m recalgorithm_amd.build` "
                           "(there is no CPU fallback for the hot path)")
    import torch  # noqa: F401  (maps torch's libamdhip64 before ours resolves its NEEDED)
    lib = ctypes.CDLL(path, mode=ctypes.RTLD_GLOBAL)
    for abi in every_header().values():
        for name, (res, args) in abi.functions.items():
            try:
                fn = getattr(lib, name)
            except AttributeError as e:
                raise RecalgoError(f"{path} does not export {name}") from e
            fn.restype, fn.argtypes = res, args
            if name in abi.launches:
                fn.errcheck = launch_errcheck(name)
        got = getattr(lib, abi.version_query)()
        if got != abi.version:
            raise RecalgoError(f"{path}: {abi.label} version {got}, this binding expects {abi.version} "
                               "(a stale build: python -m recalgorithm_amd.build)")
    _lib = lib
    return lib


def check(rc: int, what: str) -> None:
    if rc != 0:
        raise RecalgoError(f"{what} failed with hipError_t={rc}")
