"""CPU-only: include/recalgo_ffm.h (FFM's field-aware term as one kernel each way and the de-duplication of a bag, csrc/ffm.hip) is
a header of the library like the others: listed in _lib.SERVING_HEADERS, bound by load(), and held to every per-header check of
tests/test_abi.py (the pattern of tests/test_afm_fused_host.py).  The support query's truth table on and one step past every
limit, the refusals of the three launching entries on made-up addresses (nothing is launched, so no device is needed), and
tests/ffm_ref.py's de-duplication against the composed path's torch.unique form on the host."""
import ctypes

import numpy as np
import pytest
import torch

from tests import ffm_ref as R

NAME = "recalgo_ffm.h"
LAUNCHES = {"recalgo_ffm_bag_distinct", "recalgo_ffm_fwd", "recalgo_ffm_bwd"}
QUERIES = {"recalgo_ffm_abi_version", "recalgo_ffm_supported"}
LIMITS = {"RECALGO_FFM_MIN_F": 2, "RECALGO_FFM_MAX_F": 32, "RECALGO_FFM_MIN_K": 4, "RECALGO_FFM_MAX_K": 64, "RECALGO_FFM_MAX_BAGS": 4}


def test_the_header_tables():
    from recalgorithm_amd import _lib
    assert NAME in _lib.SERVING_HEADERS and NAME not in _lib.all_headers()
    abi = _lib.SERVING_HEADERS[NAME]
    assert (abi.version, abi.version_query, abi.label) == (1, "recalgo_ffm_abi_version", "FFM ABI")
    assert set(abi.functions) == LAUNCHES | QUERIES
    assert set(abi.launches) == LAUNCHES
    assert {k: abi.constants[k] for k in LIMITS} == LIMITS
    assert [n for n, _ in abi.structs["recalgo_ffm_field_t"]._fields_] == ["row_base", "vocab", "bag"]
    assert [n for n, _ in abi.structs["recalgo_ffm_bag_t"]._fields_] == ["values", "offsets", "distinct", "capacity", "d_rows"]
    lib = _lib.load()
    for name, (res, args) in abi.functions.items():
        fn = getattr(lib, name)
        assert fn.restype is res and list(fn.argtypes) == args and (fn.errcheck is not None) == (name in LAUNCHES), name
    # the argument order the header states
    I, L, P = ctypes.c_int, ctypes.c_int64, ctypes.c_void_p
    assert abi.functions["recalgo_ffm_bag_distinct"][1] == [P, P, I, L, P, P, P, P]          # values, offsets, B, n, out, valid, distinct
    assert abi.functions["recalgo_ffm_fwd"][1] == [P, P, P, I, P, I, I, I, P, P, P, I, P]    # ids, fields, bags, n_bags, arena, B, F, K, out, ..
    assert abi.functions["recalgo_ffm_bwd"][1] == [P, P, P, P, I, P, I, I, I, P, P]          # g, ids, fields, bags, n_bags, arena, B, F, K, d_single


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


# (F, K, bags) -> served: on and one step past every limit, K off its grid, negatives, the golden's and the benchmark's shapes
TRUTH = [((1, 8, 0), 0), ((2, 8, 0), 1), ((32, 8, 0), 1), ((33, 8, 0), 0),
         ((7, 0, 0), 0), ((7, 4, 0), 1), ((7, 6, 0), 0), ((7, 64, 0), 1), ((7, 68, 0), 0),
         ((7, 8, 0), 1), ((7, 8, 4), 1), ((7, 8, 5), 0), ((2, 8, 2), 1), ((2, 8, 3), 0),
         ((-3, 8, 0), 0), ((7, -4, 0), 0), ((7, 8, -1), 0), ((7, 4, 1), 1), ((26, 16, 0), 1), ((32, 64, 4), 1)]


@pytest.mark.parametrize("shape,served", TRUTH)
def test_the_support_query(shape, served):
    from recalgorithm_amd import _lib, ops
    assert _lib.load().recalgo_ffm_supported(*shape) == served
    assert ops.ffm_supported(*shape) == bool(served)


def _descriptors(F, n_bags, changes=None):
    """host descriptor arrays of a call with the LAST n_bags fields multi-valued, over made-up device addresses"""
    from recalgorithm_amd import _lib
    S = _lib.SERVING_HEADERS[NAME].structs
    Field, Bag = S["recalgo_ffm_field_t"], S["recalgo_ffm_bag_t"]
    fields = [dict(row_base=100 * i, vocab=10, bag=(i - (F - n_bags) if i >= F - n_bags else -1)) for i in range(F)]
    bags = [dict(values=0x100000 * (k + 1), offsets=0x200000 * (k + 1), distinct=0x300000 * (k + 1), capacity=12, d_rows=0x400000 * (k + 1))
            for k in range(n_bags)]
    for (kind, i, field), v in (changes or {}).items():
        (fields if kind == "field" else bags)[i][field] = v
    return (Field * F)(*[Field(**f) for f in fields]), ((Bag * n_bags)(*[Bag(**b) for b in bags]) if n_bags else None)


def test_refusals_need_no_device():
    """Every refusal returns hipErrorInvalidValue through the errcheck before any launch (made-up addresses: nothing is read)."""
    from recalgorithm_amd import _lib
    lib = _lib.load()
    P = ctypes.c_void_p
    B, F, K, nb = 5, 7, 8, 2

    def refused(name):
        return pytest.raises(_lib.RecalgoError, match=f"{name} failed with hipError_t=1$")

    # ---- recalgo_ffm_bag_distinct(values, offsets, B, n, out_values, valid, distinct, stream)
    ok = [P(0x10000), P(0x20000), B, 12, P(0x30000), P(0x40000), P(0x50000), None]
    for i, v in ((2, 0), (2, -1), (3, -1), (3, (1 << 31) - B), (0, None), (1, None), (4, None), (5, None), (6, None), (4, P(0x10000)),
                 (0, P(0x10004)), (1, P(0x20004)), (4, P(0x30004)), (5, P(0x40002)), (6, P(0x50002))):
        with refused("recalgo_ffm_bag_distinct"):
            lib.recalgo_ffm_bag_distinct(*[v if j == i else a for j, a in enumerate(ok)])

    # ---- recalgo_ffm_fwd(ids, fields, bags, n_bags, arena, B, F, K, out, deferred, step_dev, step_offset, stream)
    # ---- recalgo_ffm_bwd(g, ids, fields, bags, n_bags, arena, B, F, K, d_single, stream)
    fields, bags = _descriptors(F, nb)
    fwd_ok = [P(0x10000), fields, bags, nb, P(0x20000), B, F, K, P(0x30000), None, None, 0, None]
    bwd_ok = [P(0x40000), P(0x10000), fields, bags, nb, P(0x20000), B, F, K, P(0x50000), None]
    cases = {"recalgo_ffm_fwd": (fwd_ok, dict(ids=0, fields=1, bags=2, n_bags=3, arena=4, B=5, F=6, K=7), [0, 1, 2, 4, 8],
                                 [(0, 4), (4, 8), (8, 2), (10, 4)]),
             "recalgo_ffm_bwd": (bwd_ok, dict(ids=1, fields=2, bags=3, n_bags=4, arena=5, B=6, F=7, K=8), [0, 1, 2, 3, 5, 9],
                                 [(0, 2), (1, 4), (5, 8), (9, 8)])}
    for name, (ok, at, not_null, misaligned) in cases.items():
        fn = getattr(lib, name)

        def call(**changes):
            a = list(ok)
            for k, v in changes.items():
                a[at[k] if k in at else int(k[1:])] = v
            return fn(*a)
        for k, v in (("F", 1), ("F", 33), ("K", 0), ("K", 6), ("K", 68), ("K", -4), ("B", 0), ("B", -1), ("n_bags", 5), ("n_bags", -1),
                     ("n_bags", 1), ("n_bags", 3)):           # (n_bags 1 / 3: a field names a bag outside the call / a bag nobody names)
            with refused(name):
                call(**{k: v})
        for i in not_null:
            with refused(name):
                call(**{f"a{i}": None})
        for i, off in misaligned:
            with refused(name):
                call(**{f"a{i}": P((ok[i].value if ok[i] is not None else 0x60000) + off)})
        for change in ({("field", 0, "vocab"): 0}, {("field", 3, "row_base"): -1}, {("field", 6, "bag"): 0},       # (bag 0 taken twice)
                       {("field", 6, "bag"): 2}, {("field", 0, "bag"): 1}, {("bag", 0, "offsets"): None}, {("bag", 1, "distinct"): None},
                       {("bag", 0, "values"): None}, {("bag", 1, "capacity"): -1}, {("bag", 1, "capacity"): 1 << 31},
                       {("bag", 0, "values"): 0x100004}, {("bag", 0, "offsets"): 0x200004}, {("bag", 1, "distinct"): 0x600002}):
            f2, b2 = _descriptors(F, nb, change)
            with refused(name):
                call(fields=f2, bags=b2)
    for change in ({("bag", 0, "d_rows"): None}, {("bag", 1, "d_rows"): 0x800008}):
        f2, b2 = _descriptors(F, nb, change)
        with refused("recalgo_ffm_bwd"):
            lib.recalgo_ffm_bwd(*[f2 if j == 2 else b2 if j == 3 else a for j, a in enumerate(bwd_ok)])
    # B * n_single * (F - 1) * K / 4 pieces must stay below 2^31
    f32, _ = _descriptors(32, 0)
    with refused("recalgo_ffm_fwd"):
        lib.recalgo_ffm_fwd(P(0x10000), f32, None, 0, P(0x20000), 1 << 18, 32, 64, P(0x30000), None, None, 0, None)


# ---- the de-duplication ---------------------------------------------------------------------------------------------------------------
def _composed(values, offsets):
    """the composed path's form on the host: the distinct valid ids of every bag, ascending"""
    from recalgorithm_amd.algorithm.FFM.ffm import _distinct_bags
    from recalgorithm_amd.feature_column import Ragged
    from recalgorithm_amd.variables import VariableStore, use_store
    with use_store(VariableStore(torch.device("cpu"))) as store:
        d = _distinct_bags(Ragged(torch.from_numpy(values), torch.from_numpy(offsets)))
        assert "data-dependent count" in store.data_dependent
    return d.values.numpy(), d.offsets.numpy()


def _same_sets(values, offsets):
    kept, valid, n = R.distinct(values, offsets)
    dv, do = _composed(values[:int(offsets[-1])].copy(), offsets)
    assert kept.shape == values.shape and np.array_equal(np.diff(do), n)
    for b in range(len(offsets) - 1):
        mine = kept[offsets[b]:offsets[b + 1]]
        assert sorted(mine[mine >= 0]) == list(dv[do[b]:do[b + 1]]), b
        bag = values[offsets[b]:offsets[b + 1]]
        assert valid[b] == (bag >= 0).sum() and n[b] == len(set(bag[bag >= 0]))
    assert (kept[int(offsets[-1]):] == -1).all()
    return kept, valid, n


@pytest.mark.parametrize("B", [5, 257])
def test_the_reference_deduplication_is_the_composed_one(B):
    values, offsets = R.make_bags(B, 9, seed=B)
    kept, valid, n = _same_sets(values, offsets)
    assert n[0] == 0 and valid[1] == 0 and n[1] == 0 and (valid[2], n[2]) == (3, 1) and (valid[3], n[3]) == (4, 2)
    assert offsets[5] - offsets[4] == 70
    padded = R.pad(values, len(values) + 7)
    assert np.array_equal(R.distinct(padded, offsets)[0], R.pad(kept, len(values) + 7))


def test_the_golden_batch_tag_bags(tmp_path):
    """the golden rows' manual_tag_list: 3 bags with a repeated id, 11 empty bags, 3 with an empty string among their keys — an
    OOV entry, as is the unknown key of two bags"""
    from tests import golden_util as GU
    vocab_dir = GU.write_vocab_dir(str(tmp_path / "vocabulary"))
    _, params, _ = GU.mirror_setup("model_ffm", vocab_dir)
    cat = params["one_hot_category_feature_columns"][-1].categorical_column
    assert cat.key == "manual_tag_list"
    x = cat.ids({cat.key: GU.string_batch()[0][cat.key]}, torch.device("cpu"))
    values, offsets = x.values.numpy(), x.offsets.numpy()
    bags = [values[offsets[b]:offsets[b + 1]] for b in range(48)]
    assert sum(len(set(b[b >= 0])) < (b >= 0).sum() for b in bags) == 3
    assert sum(len(b) == 0 for b in bags) == 11
    # an entry < 0 is an empty string (3 bags: rows 0, 11, 22) or a key outside the vocabulary (rows 0 and 36): 4 bags in all
    raw = GU.string_batch()[0][cat.key]
    assert sum("" in r for r in raw) == 3 and sum("manual_tag_id_36" in r for r in raw) == 2
    assert [i for i, b in enumerate(bags) if (b < 0).any()] == [0, 11, 22, 36]
    _same_sets(values, offsets)
