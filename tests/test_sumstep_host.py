"""CPU-only: include/recalgo_sumstep.h (the step's deferred sums inside the optimizer launch, csrc/tail.hip) is a header of the
library like the others: listed in _lib.SERVING_HEADERS, bound by load(), and held to every per-header check of tests/test_abi.py
(the pattern of tests/test_metrics_host.py)."""
NAME = "recalgo_sumstep.h"
LAUNCHES = {"recalgo_adam_tf1_sum_step"}


def test_the_header_tables():
    from recalgorithm_amd import _lib
    assert NAME in _lib.SERVING_HEADERS and NAME not in _lib.all_headers()
    abi = _lib.SERVING_HEADERS[NAME]
    assert (abi.version, abi.version_query, abi.label) == (1, "recalgo_sumstep_abi_version", "SUMSTEP ABI")
    assert set(abi.functions) == LAUNCHES | {"recalgo_sumstep_abi_version", "recalgo_adam_tf1_sum_step_supported",
                                             "recalgo_adam_tf1_sum_step_workspace_bytes"}
    assert set(abi.launches) == LAUNCHES and not abi.structs
    lib = _lib.load()
    for name, (res, args) in abi.functions.items():
        fn = getattr(lib, name)
        assert fn.restype is res and list(fn.argtypes) == args and (fn.errcheck is not None) == (name in LAUNCHES), name
    # the ticket buffer: 8 shard words, the top word and two lr_t slots, each on 256 bytes of its own
    assert lib.recalgo_adam_tf1_sum_step_workspace_bytes() == 11 * 256


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


def test_refusals_need_no_device():
    """The support query is host code: the bounds of the flat buffer, overlap and the table's size, on made-up addresses."""
    import ctypes
    from recalgorithm_amd import _lib
    lib = _lib.load()
    CS = _lib.STRUCTS["recalgo_colsum_t"]
    g, n = 0x10000, 1000
    at = lambda i: g + 4 * i                                          # noqa: E731
    ok = (CS * 2)(CS(0x900000, at(0), 3, 8, 8), CS(0x900000, at(8), 3, 8, 8))
    side = (CS * 1)(CS(0x900000, 0x800000, 3, 8, 1))
    q = lambda sums, ns, sd=side, nsd=1: lib.recalgo_adam_tf1_sum_step_supported(ctypes.c_void_p(g), n, None, 0, sums, ns, sd, nsd)   # noqa: E731
    assert q(ok, 2) == 1
    assert q((CS * 2)(ok[0], CS(0x900000, at(4), 3, 8, 8)), 2) == 0              # overlap
    assert q((CS * 2)(ok[0], CS(0x900000, at(996), 3, 8, 8)), 2) == 0            # across the end
    assert q((CS * 2)(ok[0], CS(0x900000, 0x800000, 3, 8, 1)), 2) == 0           # outside
    assert q(ok, 2, (CS * 1)(CS(0x900000, at(100), 3, 8, 1)), 1) == 0            # a side sum inside
    assert q((CS * 33)(*[CS(0x900000, at(8 * i), 3, 8, 8) for i in range(33)]), 33, None, 0) == 0   # 33 jobs
    assert q((CS * 32)(*[CS(0x900000, at(8 * i), 3, 8, 8) for i in range(32)]), 32, None, 0) == 1
    assert lib.recalgo_adam_tf1_sum_step_supported(ctypes.c_void_p(g + 4), n, None, 0, ok, 2, None, 0) == 0     # g not 16-byte aligned
