"""CPU-only: include/recalgo_afm.h (AFM's attention network as one kernel each way, csrc/afm.hip) is a header of the library
like the others: listed in _lib.SERVING_HEADERS, bound by load(), and held to every per-header check of tests/test_abi.py (the
pattern of tests/test_sumstep_host.py).  The support query's truth table on and one step past every limit, the refusals of
both launching entries on made-up addresses (nothing is launched, so no device is needed) and the workspace query."""
import ctypes

import pytest

NAME = "recalgo_afm.h"
LAUNCHES = {"recalgo_afm_attention_fwd", "recalgo_afm_attention_bwd"}
QUERIES = {"recalgo_afm_abi_version", "recalgo_afm_supported", "recalgo_afm_bwd_partial_rows", "recalgo_afm_bwd_workspace_bytes"}


def test_the_header_tables():
    from recalgorithm_amd import _lib
    assert NAME in _lib.SERVING_HEADERS and NAME not in _lib.all_headers()
    abi = _lib.SERVING_HEADERS[NAME]
    assert (abi.version, abi.version_query, abi.label) == (1, "recalgo_afm_abi_version", "AFM ABI")
    assert set(abi.functions) == LAUNCHES | QUERIES
    assert set(abi.launches) == LAUNCHES and not abi.structs
    assert {k: abi.constants[k] for k in ("RECALGO_AFM_MAX_F", "RECALGO_AFM_MAX_K", "RECALGO_AFM_MAX_T",
                                          "RECALGO_AFM_MAX_PARTIAL_ROWS")} == \
        {"RECALGO_AFM_MAX_F": 64, "RECALGO_AFM_MAX_K": 32, "RECALGO_AFM_MAX_T": 256, "RECALGO_AFM_MAX_PARTIAL_ROWS": 1024}
    lib = _lib.load()
    for name, (res, args) in abi.functions.items():
        fn = getattr(lib, name)
        assert fn.restype is res and list(fn.argtypes) == args and (fn.errcheck is not None) == (name in LAUNCHES), name


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


# (F, K, t) -> served: on and one step past every limit, K and t off their grids, the golden's shape
TRUTH = [((1, 8, 16), 0), ((2, 8, 16), 1), ((64, 8, 16), 1), ((65, 8, 16), 0),
         ((7, 0, 16), 0), ((7, 4, 16), 1), ((7, 32, 16), 1), ((7, 36, 16), 0), ((7, 6, 16), 0),
         ((7, 8, 0), 0), ((7, 8, 16), 1), ((7, 8, 256), 1), ((7, 8, 272), 0), ((7, 8, 24), 0),
         ((7, 8, 12), 0), ((64, 32, 256), 1), ((26, 16, 128), 1), ((-3, 8, 16), 0), ((7, -4, 16), 0), ((7, 8, -16), 0)]


@pytest.mark.parametrize("shape,served", TRUTH)
def test_the_support_query(shape, served):
    from recalgorithm_amd import _lib
    lib = _lib.load()
    assert lib.recalgo_afm_supported(*shape) == served
    # the size queries answer 0 for what is not served, and for an empty batch
    assert (lib.recalgo_afm_bwd_partial_rows(5, *shape) > 0) == bool(served)
    assert (lib.recalgo_afm_bwd_workspace_bytes(5, *shape) > 0) == bool(served)
    assert lib.recalgo_afm_bwd_partial_rows(0, *shape) == 0 and lib.recalgo_afm_bwd_workspace_bytes(0, *shape) == 0


def test_the_workspace_is_the_documented_rows():
    """rows = min(ceil(B / waves), 1024), waves = 4, or 2 or 1 where a workgroup's LDS does not hold four examples' state
    (F = 64, K = 32, t = 256: two); a row is [dw | db | dh] = K t + 2 t floats."""
    from recalgorithm_amd import _lib
    lib = _lib.load()
    for (F, K, t), waves in (((3, 4, 32), 4), ((26, 16, 128), 4), ((64, 8, 32), 4), ((4, 32, 256), 4), ((64, 32, 256), 2),
                             ((64, 32, 16), 4)):
        for B in (1, 3, 4, 5, 33, 130, 4096, 4097, 1 << 20):
            rows = min(-(-B // waves), 1024)
            assert lib.recalgo_afm_bwd_partial_rows(B, F, K, t) == rows, (B, F, K, t)
            assert lib.recalgo_afm_bwd_workspace_bytes(B, F, K, t) == rows * (K * t + 2 * t) * 4, (B, F, K, t)


def test_refusals_need_no_device():
    """Every refusal returns hipErrorInvalidValue through the errcheck before any launch (made-up addresses: nothing is read)."""
    from recalgorithm_amd import _lib
    lib = _lib.load()
    P = ctypes.c_void_p
    B, F, K, t = 5, 7, 8, 16
    fwd_ok = [P(0x10000 * (i + 1)) for i in range(4)] + [B, F, K, t, P(0x90000), P(0xA0000), None]      # .., out, scores, stream
    bwd_ok = [P(0x10000 * (i + 1)) for i in range(6)] + [B, F, K, t] + [P(0x100000 * (i + 1)) for i in range(5)] + [None]
    cases = {"recalgo_afm_attention_fwd": (fwd_ok, (4, 5, 6, 7), [0, 1, 2, 3, 8], [0, 1, 2, 3, 8, 9]),
             "recalgo_afm_attention_bwd": (bwd_ok, (6, 7, 8, 9), [0, 1, 2, 3, 4, 5, 10, 11, 12, 13, 14], None)}
    for name, (ok, (iB, iF, iK, it), not_null, pointers) in cases.items():
        fn = getattr(lib, name)
        refused = pytest.raises(_lib.RecalgoError, match=f"{name} failed with hipError_t=1$")

        def call(**changes):
            a = list(ok)
            for i, v in changes.items():
                a[int(i[1:])] = v
            return fn(*a)
        for i, v in ((iF, 1), (iF, 65), (iK, 6), (iK, 36), (iK, 0), (it, 12), (it, 24), (it, 272), (iB, 0), (iB, -1)):
            with refused:
                call(**{f"a{i}": v})
        with refused:                                     # the golden's shape stays unserved
            call(**{f"a{iF}": 7, f"a{iK}": 8, f"a{it}": 12})
        for i in not_null:
            with refused:
                call(**{f"a{i}": None})
        for i in (pointers or not_null):
            with refused:
                call(**{f"a{i}": P(ok[i].value + 2)})
