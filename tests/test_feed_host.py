"""CPU-only: include/recalgo_feed.h (the `prepare` launch that also moves a captured step's batch into its static inputs,
csrc/sparse.hip) is a header of the library like the others: listed in _lib.SERVING_HEADERS, bound by load(), and held to every
per-header check of tests/test_abi.py (the pattern of tests/test_sumstep_host.py).  The support query and the refusals of the
entry are host code: made-up addresses, nothing is launched."""
import ctypes

import pytest

NAME = "recalgo_feed.h"
LAUNCHES = {"recalgo_scatter_prepare_feed"}


def test_the_header_tables():
    from recalgorithm_amd import _lib
    assert NAME in _lib.SERVING_HEADERS and NAME not in _lib.all_headers()
    abi = _lib.SERVING_HEADERS[NAME]
    assert (abi.version, abi.version_query, abi.label) == (1, "recalgo_feed_abi_version", "FEED ABI")
    assert set(abi.functions) == LAUNCHES | {"recalgo_feed_abi_version", "recalgo_scatter_prepare_feed_supported"}
    assert set(abi.launches) == LAUNCHES and not abi.structs
    lib = _lib.load()
    for name, (res, args) in abi.functions.items():
        fn = getattr(lib, name)
        assert fn.restype is res and list(fn.argtypes) == args and (fn.errcheck is not None) == (name in LAUNCHES), name
    # what recalgo_scatter_prepare takes (its one source and first slot as arrays of n_sources), then the feed, then the stream
    assert len(abi.functions["recalgo_scatter_prepare_feed"][1]) == len(_lib.SIGNATURES["recalgo_scatter_prepare"][1]) + 1 + 3


def test_every_shared_abi_check_holds_for_the_new_header(monkeypatch):
    from recalgorithm_amd import _lib, build
    from tests import test_abi as A
    union = _lib.every_header()
    monkeypatch.setattr(_lib, "HEADERS", union)
    monkeypatch.setattr(A, "HEADERS", list(union))
    lib_path = build.build(verbose=False)
    A.test_header_declares_functions(NAME)
    A.test_library_exports_every_declared_symbol(NAME, lib_path)
    A.test_ctypes_binding_matches_header(NAME, lib_path)
    A.test_loaded_functions_carry_the_table(NAME, lib_path)
    A.test_declarations_do_not_change_without_a_version_bump(NAME)
    A.test_header_arg_counts_match_binding(NAME)
    A.test_header_arg_types_match_binding(NAME)
    A.test_header_is_self_contained(NAME)
    A.test_the_headers_share_no_name()


DST, SRC = 0x7f0000001000, 0x7f0000800000
REFUSED = [("another 16-byte phase", DST, SRC + 8, 4096), ("overlap from below", DST, DST - 64, 4096),
           ("overlap from above", DST, DST + 4080, 4096), ("a negative size", DST, SRC, -1), ("no destination", None, SRC, 64)]
ACCEPTED = [("disjoint, aligned", DST, SRC, 4096), ("a common odd phase, odd length", DST + 5, SRC + 21, 1001),
            ("touching ranges", DST, DST + 4096, 4096), ("the same span: no copy", DST, DST, 4096), ("no source: no copy", DST, None, 4096),
            ("no bytes: no copy", DST, SRC + 8, 0), ("nothing at all", None, None, 0)]


def test_the_support_query():
    from recalgorithm_amd import _lib
    q = _lib.load().recalgo_scatter_prepare_feed_supported
    for what, d, s, n in ACCEPTED:
        assert q(d, s, n) == 1, what
    for what, d, s, n in REFUSED:
        assert q(d, s, n) == 0, what


@pytest.mark.parametrize("case", REFUSED, ids=[c[0] for c in REFUSED])
def test_a_refused_feed_is_an_error_before_any_launch(case):
    """No source, no flags: with an accepted feed of no bytes the call has nothing to launch and returns 0 without touching the
    device; a refused feed returns hipErrorInvalidValue from the same place."""
    from recalgorithm_amd import _lib
    lib = _lib.load()
    ws = ctypes.c_void_p(0x7f0001000000)
    call = lambda d, s, n: lib.recalgo_scatter_prepare_feed(None, 0, None, 4, ws, 256, 10, 0, None, None, 0, 0, 1, None, 0, d, s, n, None)   # noqa: E731
    assert call(DST, None, 4096) == 0 and call(DST, DST, 4096) == 0 and call(DST, SRC, 0) == 0
    _, d, s, n = case
    with pytest.raises(_lib.RecalgoError, match="hipError_t=1"):
        call(d, s, n)
