"""CPU-only: include/recalgo_flen.h (FLEN's field-wise bi-interaction with Dicefactor, csrc/flen.hip) is a header of the library
like the others: listed in _lib.SERVING_HEADERS, bound by load(), and held to every per-header check of tests/test_abi.py (the
pattern of tests/test_dcnv2_host.py).  The domain table against the support query, the refusals of both launching entries on
made-up addresses (nothing is launched, so no device is needed), the size queries; tests/flen_ref.py: the header's backward
formulas written out against autograd, a group of one field, and the condition that keeps the GPU parity tests honest (the float32
restatement alone meets their bound on every one of their shapes); field_groups parsing; the composed path on CPU tensors; the
model's flags and defaults, its variables on the launch-free registration pass, and what the product imports."""
import ctypes
import json
import os
import re
import subprocess
import sys

import pytest
import torch

from tests import flen_ref as R
from tests import golden_util as GU
from tests.util import assert_close

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAME = "recalgo_flen.h"
LAUNCHES = {"recalgo_flen_fwd", "recalgo_flen_bwd"}
QUERIES = {"recalgo_flen_abi_version", "recalgo_flen_supported", "recalgo_flen_bwd_partial_rows", "recalgo_flen_bwd_workspace_bytes"}
LIMITS = {"RECALGO_FLEN_MIN_F": 2, "RECALGO_FLEN_MAX_F": 64, "RECALGO_FLEN_MIN_M": 2, "RECALGO_FLEN_MAX_M": 8, "RECALGO_FLEN_MIN_K": 4,
          "RECALGO_FLEN_MAX_K": 64, "RECALGO_FLEN_LANES": 64, "RECALGO_FLEN_MAX_PARTIAL_ROWS": 512}


def test_the_header_tables():
    from recalgorithm_amd import _abi, _lib
    assert NAME in _lib.SERVING_HEADERS and NAME not in _lib.all_headers() and NAME in _lib.every_header()
    abi = _lib.SERVING_HEADERS[NAME]
    assert (abi.version, abi.version_query, abi.label) == (1, "recalgo_flen_abi_version", "FLEN ABI")
    assert _abi.read_record(NAME) == {1: _abi.declaration_hash(NAME)}
    assert set(abi.functions) == LAUNCHES | QUERIES
    assert set(abi.launches) == LAUNCHES and not abi.structs
    assert {k: abi.constants[k] for k in LIMITS} == LIMITS
    lib = _lib.load()
    assert lib.recalgo_flen_abi_version() == 1
    for name, (res, args) in abi.functions.items():
        fn = getattr(lib, name)
        assert fn.restype is res and list(fn.argtypes) == args and (fn.errcheck is not None) == (name in LAUNCHES), name
    # the argument order the header states
    I, L, P = ctypes.c_int, ctypes.c_int64, ctypes.c_void_p
    assert abi.functions["recalgo_flen_supported"] == (I, [I] * 3)                                      # F, M, K
    assert abi.functions["recalgo_flen_bwd_partial_rows"] == (I, [I] * 4)                               # B, F, M, K
    assert abi.functions["recalgo_flen_bwd_workspace_bytes"] == (L, [I] * 4)
    assert abi.functions["recalgo_flen_fwd"] == (I, [P] * 6 + [I] * 4 + [P] * 3)                        # x .. dice, .., e, h, stream
    assert abi.functions["recalgo_flen_bwd"] == (I, [P] * 7 + [I] * 4 + [P] * 6)                        # g_e .. dice, .., dx .. ws, stream


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


# (F, M, K) -> served: on and one step past every limit, K off its grid, M above F, negatives
TRUTH = [((1, 2, 8), 0), ((2, 2, 8), 1), ((64, 2, 8), 1), ((65, 2, 8), 0),
         ((7, 1, 8), 0), ((7, 2, 8), 1), ((7, 7, 8), 1), ((7, 8, 8), 0), ((8, 8, 8), 1), ((9, 9, 8), 0), ((64, 9, 8), 0), ((3, 4, 8), 0),
         ((7, 3, 0), 0), ((7, 3, 4), 1), ((7, 3, 6), 0), ((7, 3, 12), 1), ((7, 3, 62), 0), ((7, 3, 64), 1), ((7, 3, 68), 0),
         ((-7, 3, 8), 0), ((7, -3, 8), 0), ((7, 3, -8), 0),
         ((26, 4, 16), 1), ((7, 3, 8), 1), ((64, 8, 64), 1), ((2, 2, 4), 1), ((9, 8, 4), 1)]


@pytest.mark.parametrize("shape,served", TRUTH)
def test_the_support_query(shape, served):
    from recalgorithm_amd import _lib, ops
    lib = _lib.load()
    assert lib.recalgo_flen_supported(*shape) == served
    assert ops.flen_supported(*shape) == bool(served)
    F, M, K = shape
    C = LIMITS
    assert bool(served) == (C["RECALGO_FLEN_MIN_F"] <= F <= C["RECALGO_FLEN_MAX_F"]
                            and C["RECALGO_FLEN_MIN_M"] <= M <= min(F, C["RECALGO_FLEN_MAX_M"])
                            and C["RECALGO_FLEN_MIN_K"] <= K <= C["RECALGO_FLEN_MAX_K"] and K % 4 == 0)
    # the size queries answer 0 for what is not served, and for an empty batch
    assert (lib.recalgo_flen_bwd_partial_rows(5, *shape) > 0) == bool(served)
    assert (lib.recalgo_flen_bwd_workspace_bytes(5, *shape) > 0) == bool(served)
    assert lib.recalgo_flen_bwd_workspace_bytes(0, *shape) == 0
    assert lib.recalgo_flen_bwd_partial_rows(0, *shape) == 0 and lib.recalgo_flen_bwd_partial_rows(-1, *shape) == 0


def test_the_domain_is_what_the_unit_requires():
    """csrc/flen.hip: both launching entries open with RECALGO_REQUIRE lines — the batch and the shape through the one shape_ok()
    that the support query answers with, the pointers, the alignment and the Dicefactor descriptor, the grouping — and launch
    nothing before the last of them; shape_ok names every limit of the header's domain and nothing else."""
    src = open(os.path.join(ROOT, "recalgorithm_amd", "csrc", "flen.hip")).read()
    ok = re.search(r"bool shape_ok\(int F, int M, int K\) \{(.*?)\n\}", src, re.S).group(1)
    assert sorted(set(re.findall(r"RECALGO_FLEN_\w+", ok))) == sorted(k for k in LIMITS if k.startswith(("RECALGO_FLEN_MIN", "RECALGO_FLEN_MAX_F",
                                                                                                         "RECALGO_FLEN_MAX_M", "RECALGO_FLEN_MAX_K")))
    assert "(K & 3) == 0" in ok and "M <= F" in ok
    assert "recalgo_flen_supported(int F, int M, int K) { return shape_ok(F, M, K) ? 1 : 0; }" in src
    for entry in ("recalgo_flen_fwd", "recalgo_flen_bwd"):
        body = src[src.index(f"RECALGO_EXPORT int {entry}("):]
        body = body[:body.index("\n}\n")]
        req = re.findall(r"RECALGO_REQUIRE\((.*?)\);\n", body, re.S)
        assert len(req) == 4, (entry, req)
        assert req[0] == "B >= 1 && shape_ok(F, M, K)"
        assert req[2].startswith("aligned16(") and "aligned_to<4>(" in req[2] and "dice_ok(d, B, M, K)" in req[2]
        assert req[3] == "make_plan(group_of, F, M, &a.plan)"
        assert body.index("launch_") > body.index(req[-1]), "nothing is launched before the last requirement"


def test_the_workspace_is_the_documented_layout():
    """R = min(ceil(B / T), 512) rows of P + M + K floats, T = floor(64 / (K / 4)) examples per workgroup"""
    from recalgorithm_amd import _lib
    lib = _lib.load()
    for F, M, K in ((2, 2, 4), (7, 3, 8), (7, 3, 12), (26, 4, 16), (64, 8, 64), (9, 8, 4), (30, 5, 20), (30, 5, 24)):
        T = 64 // (K // 4)
        row = M * (M - 1) // 2 + M + K
        for B in (1, T, T + 1, 4096, 512 * T, 512 * T + 1, 1 << 20):
            rows = min(-(-B // T), 512)
            assert lib.recalgo_flen_bwd_partial_rows(B, F, M, K) == rows, (B, F, M, K)
            assert lib.recalgo_flen_bwd_workspace_bytes(B, F, M, K) == 4 * rows * row, (B, F, M, K)
    assert 8 * 7 // 2 + 8 + 64 == 100                                            # the widest row


def _dice(rate=0.3, mask=None):
    from recalgorithm_amd import _lib
    return _lib.STRUCTS["recalgo_dropout_t"](rate, mask, 5, 0, None)


def test_refusals_need_no_device():
    """Every refusal returns hipErrorInvalidValue through the errcheck before any launch (made-up device addresses: nothing is
    read; group_of is the host array the entries do read): an unsupported shape or B < 1, a group index outside [0, M), an empty
    group, a NULL pointer other than dice, misalignment (16 bytes for x, dx, e, g_e, h, g_h and an explicit mask, 4 for the small
    vectors), a Dicefactor rate outside (0, 1), and Dicefactor over 2^32 or more path components."""
    from recalgorithm_amd import _lib
    lib = _lib.load()
    P = ctypes.c_void_p
    B, F, M, K = 5, 7, 3, 8
    groups = (ctypes.c_int32 * 64)(*(list(R.DATASET_GROUPS) + [0] * 57))
    gp = ctypes.cast(groups, P)
    # x, group_of, r_mf, r_fm, bias, dice, B, F, M, K, e, h, stream
    fwd_ok = [P(0x10000), gp, P(0x30000), P(0x40000), P(0x50000), None, B, F, M, K, P(0x70000), P(0x80000), None]
    # g_e, g_h, x, group_of, r_mf, r_fm, dice, B, F, M, K, dx, dr_mf, dr_fm, dbias, workspace, stream
    bwd_ok = [P(0x10000), P(0x20000), P(0x30000), gp, P(0x50000), P(0x60000), None, B, F, M, K] + [P(0x100000 * (i + 1)) for i in range(5)] + [None]
    cases = {"recalgo_flen_fwd": (fwd_ok, 5, (6, 7, 8, 9), 1, [0, 1, 2, 3, 4, 10, 11], [0, 10, 11], [2, 3, 4]),
             "recalgo_flen_bwd": (bwd_ok, 6, (7, 8, 9, 10), 3, [0, 1, 2, 3, 4, 5, 11, 12, 13, 14, 15], [0, 1, 2, 11], [4, 5, 12, 13, 14, 15])}
    for name, (ok, iDice, (iB, iF, iM, iK), iG, not_null, wide, narrow) in cases.items():
        fn = getattr(lib, name)
        refused = pytest.raises(_lib.RecalgoError, match=f"{name} failed with hipError_t=1$")

        def call(**changes):
            a = list(ok)
            for i, v in changes.items():
                a[int(i[1:])] = v
            return fn(*a)
        for i, v in ((iF, 1), (iF, 65), (iF, 0), (iF, -7), (iM, 1), (iM, 9), (iM, 0), (iM, -3), (iK, 6), (iK, 68), (iK, 0), (iK, -8),
                     (iB, 0), (iB, -1)):
            with refused:
                call(**{f"a{i}": v})
        with refused:                                     # M above F
            call(**{f"a{iF}": 2})
        for bad in ([0, 1, 0, 1, 3, 2, 1], [0, 1, 0, 1, -1, 2, 1], [0, 1, 0, 1, 1, 1, 1], [1, 1, 2, 1, 2, 2, 1]):
            with refused:                                 # an index outside [0, M); an empty group (2, then 0)
                call(**{f"a{iG}": ctypes.cast((ctypes.c_int32 * 7)(*bad), P)})
        for i in not_null:
            with refused:
                call(**{f"a{i}": None})
        for i in wide:                                    # 16-byte operands: 4 and 8 bytes off
            for off in (4, 8):
                with refused:
                    call(**{f"a{i}": P(ok[i].value + off)})
        for i in narrow:
            with refused:
                call(**{f"a{i}": P(ok[i].value + 2)})
        for rate in (0.0, 1.0, -0.1, 1.5):
            d = _dice(rate)
            with refused:
                call(**{f"a{iDice}": ctypes.cast(ctypes.pointer(d), P)})
        d = _dice(0.3, 0x200004)                          # an explicit mask 4 bytes off
        with refused:
            call(**{f"a{iDice}": ctypes.cast(ctypes.pointer(d), P)})
        d = _dice(0.3)                                    # B (P + M) K = 2^32 exactly at M 8, K 64: B = 2^32 / (36 * 64) is no integer;
        with refused:                                     # M 3, K 8: (P + M) K = 48, B = ceil(2^32 / 48)
            call(**{f"a{iDice}": ctypes.cast(ctypes.pointer(d), P), f"a{iB}": -(-(1 << 32) // 48)})


def test_ops_refuse_on_the_host():
    """ops.flen_interaction raises ValueError before any launch (CPU tensors: a call that got as far as a launch would raise
    RecalgoError instead)"""
    from recalgorithm_amd import ops
    z = torch.zeros

    def call(B=4, F=7, M=3, K=8, groups=R.DATASET_GROUPS, **over):
        a = dict(fields=z(B, F * K), F=F, group_of=groups, r_mf=z(M * (M - 1) // 2), r_fm=z(M), bias=z(K))
        a.update(over)
        return ops.flen_interaction(*a.values())
    for kw in (dict(F=1, groups=(0,)), dict(F=65, groups=(0,) * 65), dict(M=1), dict(M=9), dict(K=6), dict(K=68)):
        with pytest.raises(ValueError, match=r"the kernels serve 2 <= F <= 64, 2 <= M <= min\(F, 8\) and K % 4 == 0 with 4 <= K <= 64"):
            call(**kw)
    for groups in ((0, 1, 0, 1, 3, 2, 1), (0, 1, 0, 1, 1, 1, 1), (0, 1, 2), (0, 1, 0, 1, -1, 2, 1)):
        with pytest.raises(ValueError, match="group_of must map the F=7 fields onto every one of the M=3 groups"):
            call(groups=groups)
    with pytest.raises(ValueError, match="fields must be a non-empty"):
        call(B=0)
    with pytest.raises(ValueError, match="fields must be a non-empty"):
        call(fields=z(4, 57))
    with pytest.raises(ValueError, match="r_mf has shape"):
        call(r_mf=z(4))
    with pytest.raises(ValueError, match=r"r_fm must be \[M\] and bias \[K\]"):
        call(bias=z(2, 4))
    with pytest.raises(ValueError, match="fields must be a contiguous float32 tensor on fields' device"):     # (a CPU tensor)
        call()


# ---- tests/flen_ref.py ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("masked", [False, True])
@pytest.mark.parametrize("shape", [(5, 7, 3, 8, R.DATASET_GROUPS), (4, 9, 8, 4, (0, 1, 2, 3, 3, 4, 5, 6, 7)), (3, 6, 2, 12, (1, 0, 0, 1, 1, 0))])
def test_the_headers_backward_formulas_are_autograds(shape, masked):
    v, r64, _ = R.case(*shape, seed=3, masked=masked)
    v64 = {k: (None if t is None else t.double()) for k, t in v.items()}
    by_hand = R.backward_by_hand(v64, shape[4], keep=v64["keep"])
    for k in R.NAMES[2:]:
        assert torch.allclose(by_hand[k], r64[k], rtol=1e-11, atol=1e-12), k


def test_the_pairs_are_in_combinations_order():
    assert R.pairs_of(4) == [(0, 1), (0, 2), (0, 3), (1, 2), (1, 3), (2, 3)]
    v, r64, _ = R.case(5, 7, 3, 8, R.DATASET_GROUPS, seed=3)
    x = v["x"].double().reshape(5, 7, 8)
    e = torch.stack([x[:, [0, 2]].sum(1), x[:, [1, 3, 6]].sum(1), x[:, [4, 5]].sum(1)], 1)
    assert torch.allclose(r64["e"], e.reshape(5, 24), rtol=1e-14, atol=0)
    q = torch.stack([(x[:, [0, 2]] ** 2).sum(1), (x[:, [1, 3, 6]] ** 2).sum(1), (x[:, [4, 5]] ** 2).sum(1)], 1)
    rm, rf = v["r_mf"].double(), v["r_fm"].double()
    h = v["bias"].double() + rm[0] * e[:, 0] * e[:, 1] + rm[1] * e[:, 0] * e[:, 2] + rm[2] * e[:, 1] * e[:, 2] \
        + (rf[:, None] * (e * e - q)).sum(1)
    assert torch.allclose(r64["h"], h, rtol=1e-12, atol=1e-13)


@pytest.mark.parametrize("dtype", [torch.float64, torch.float32])
def test_a_group_of_one_field_has_no_fm_term(dtype):
    """e_m = x_f and q_m = x_f^2: the FM term and dr_fm[m] are exactly 0, in either precision"""
    name = "singletons"
    B, F, M, K, groups = R.SHAPES[name]
    v, r64, r32 = R.case(*R.SHAPES[name], masked=True)
    ref = r64 if dtype == torch.float64 else r32
    single = [m for m in range(M) if groups.count(m) == 1]
    assert len(single) == 7
    assert bool((ref["dr_fm"][single] == 0).all()) and float(ref["dr_fm"][3].abs()) > 0
    x = v["x"].to(dtype).reshape(B, F, K)
    _, _, _, _, fm = R.layer(x, groups, v["r_mf"].to(dtype), v["r_fm"].to(dtype), v["bias"].to(dtype), parts=True)
    assert bool((fm[:, single] == 0).all()) and float(fm[:, 3].abs().max()) > 0


@pytest.mark.parametrize("masked", [False, True])
@pytest.mark.parametrize("name", list(R.SHAPES))
def test_the_float32_restatement_alone_meets_the_gpu_bound(name, masked):
    """What keeps tests/test_gpu_flen.py's parity test one of the kernels: at every one of its shapes the same arithmetic in
    float32 torch passes the very assertion the kernels face."""
    v, r64, r32 = R.case(*R.SHAPES[name], masked=masked)
    for k in R.NAMES:
        assert_close(r32[k], r64[k], what=f"float32 restatement {name} {k}", reduced=k in R.REDUCED, ref32=r32[k])


def test_the_large_offset_case_is_what_it_says():
    """x = 100 + N(0, 1): e_m^2 and q_m are of order 1e4 .. 1e5 and only their difference enters h, whose float32 rounding is
    that of those terms; the float32 restatement is finite and meets the bound with the floor of its own deviation"""
    from tests.afm_ref import fp32_floor
    v, r64, r32 = R.case(*R.CANCELLATION, offset=100.0)
    x = v["x"].double().reshape(67, 7, 8)
    e, _, q, _, fm = R.layer(x, R.CANCELLATION[4], v["r_mf"].double(), v["r_fm"].double(), v["bias"].double(), parts=True)
    assert float(q.min()) > 1.5e4 and float((e * e).min()) > 3e4 and float(r64["h"].abs().min()) > 1e4
    assert all(bool(torch.isfinite(r32[k]).all()) for k in R.NAMES)
    for k in R.NAMES:
        assert_close(r32[k], r64[k], what=f"float32 restatement, cancellation {k}", reduced=k in R.REDUCED, ref32=r32[k],
                     floor=fp32_floor(r64, r32, k))


# ---- field_groups ---------------------------------------------------------------------------------------------------------------------
KEYS = ["userid", "feedid", "device", "authorid", "bgm_song_id", "bgm_singer_id", "manual_tag_list"]


def test_field_groups_parsing():
    from recalgorithm_amd.algorithm.FLEN.flen import DEFAULT_FIELD_GROUPS, parse_field_groups
    assert DEFAULT_FIELD_GROUPS == "userid,device;feedid,authorid,manual_tag_list;bgm_song_id,bgm_singer_id"
    assert tuple(parse_field_groups(DEFAULT_FIELD_GROUPS, KEYS)) == R.DATASET_GROUPS
    assert parse_field_groups(" userid , device ;feedid,authorid,manual_tag_list,bgm_song_id,bgm_singer_id", KEYS) == [0, 1, 0, 1, 1, 1, 1]
    assert parse_field_groups([["feedid"], ["userid", "device"]], ["userid", "feedid", "device"]) == [1, 0, 1]
    for text, why in (("userid,device,feedid,authorid,manual_tag_list,bgm_song_id,bgm_singer_id", "at least two groups"),
                      ("userid,device;;feedid,authorid,manual_tag_list,bgm_song_id,bgm_singer_id", "none of them empty"),
                      ("userid,device;feedid,authorid,manual_tag_list;bgm_song_id", "'bgm_singer_id'\\] are in none"),
                      (DEFAULT_FIELD_GROUPS + ",userid", "'userid' appears more than once"),
                      (DEFAULT_FIELD_GROUPS + ",feed", "'feed' is no category column")):
        with pytest.raises(ValueError, match=why):
            parse_field_groups(text, KEYS)


# ---- the composed path on CPU tensors ----------------------------------------------------------------------------------------------------
def _composed(v, groups, training, rate, masks=()):
    """nn.field_wise_bi_interaction(fused=False) on a CPU store holding v's weights, forward + backward -> {e, h, dx, d..}"""
    from recalgorithm_amd import nn
    from recalgorithm_amd.variables import VariableStore, use_store
    B, M, K = v["x"].shape[0], v["r_fm"].shape[0], v["bias"].shape[0]
    store = VariableStore("cpu", seed=3)
    with use_store(store):
        store.building = True
        e, h = nn.field_wise_bi_interaction(torch.zeros_like(v["x"]), groups, rate, training, fused=False)
        assert tuple(e.shape) == (B, M * K) and tuple(h.shape) == (B, K) and not bool(e.any()) and not bool(h.any())
        store.finalize()
    assert sorted(store.vars) == ["bias", "r_fm", "r_mf"]
    assert bool((store.vars["r_mf"].data == 1).all()) and bool((store.vars["r_fm"].data == 0.5).all()) and not bool(store.vars["bias"].data.any())
    for n in ("r_mf", "r_fm", "bias"):
        store.vars[n].data.copy_(v[n])
    x = v["x"].clone().requires_grad_(True)
    nn.DROPOUT_KEEP_MASKS[:] = list(masks)
    try:
        with use_store(store):
            store.begin_call()
            e, h = nn.field_wise_bi_interaction(x, groups, rate, training, fused=False)
            torch.autograd.backward([e, h], [v["g_e"], v["g_h"]])
        assert not nn.DROPOUT_KEEP_MASKS
    finally:
        nn.DROPOUT_KEEP_MASKS[:] = []
    return {"e": e.detach(), "h": h.detach(), "dx": x.grad, "dr_mf": store.vars["r_mf"].grad.clone(), "dr_fm": store.vars["r_fm"].grad.clone(),
            "dbias": store.vars["bias"].grad.clone()}


@pytest.mark.parametrize("name", ["dataset", "interleaved", "singletons"])
def test_the_composed_path_is_the_restatement(name):
    shape = R.SHAPES[name]
    v, r64, r32 = R.case(*shape)
    got = _composed(v, shape[4], training=True, rate=0.0)
    for k in R.NAMES:
        assert_close(got[k], r64[k], what=f"composed {name} {k}", reduced=k in R.REDUCED, ref32=r32[k])
    vm, m64, m32 = R.case(*shape, masked=True)
    got = _composed(vm, shape[4], training=True, rate=R.RATE, masks=[vm["keep"]])
    for k in R.NAMES:
        assert_close(got[k], m64[k], what=f"composed {name}, injected mask, {k}", reduced=k in R.REDUCED, ref32=m32[k])
    # EVAL and PREDICT apply no Dicefactor (and consume no mask)
    got = _composed(v, shape[4], training=False, rate=R.RATE)
    for k in ("e", "h"):
        assert_close(got[k], r64[k], what=f"composed {name}, not training, {k}", ref32=r32[k])


def test_the_layer_refuses_a_bad_grouping_and_fused_on_the_host():
    from recalgorithm_amd import nn
    from recalgorithm_amd.variables import VariableStore, use_store
    with use_store(VariableStore("cpu")):
        for groups in ((0, 0, 0), (0, 2, 0), (0,), (0, 1, -1)):
            with pytest.raises(ValueError, match="group_of must map at least two fields onto every one of M >= 2 groups"):
                nn.field_wise_bi_interaction(torch.zeros(4, 8 * len(groups)), groups, fused=False)
        with pytest.raises(ValueError, match=r"fields must be \[B, F \* K\] with F = 3"):
            nn.field_wise_bi_interaction(torch.zeros(4, 8), (0, 1, 0), fused=False)
    store = VariableStore("cpu")
    with use_store(store):
        store.building = True
        nn.field_wise_bi_interaction(torch.zeros(4, 24), (0, 1, 0))
        store.finalize()
        with pytest.raises(ValueError, match=r"fused=True\): no fused kernel serves F=3 M=2 K=8 on cpu"):
            nn.field_wise_bi_interaction(torch.zeros(4, 24), (0, 1, 0), fused=True)
    assert nn.flen_fused_default(torch.zeros(4, 24), 3, 2, 8) is False


# ---- the model ---------------------------------------------------------------------------------------------------------------------
FLAG_DEFAULTS = {"batch_size": 1024, "learning_rate": 0.005, "embedding_dim": 8,
                 "field_groups": "userid,device;feedid,authorid,manual_tag_list;bgm_song_id,bgm_singer_id", "hidden_units": "512,256,128",
                 "batch_norm": True, "dropout_rate": 0.0, "dicefactor_rate": 0.0}
TWO_GROUPS = "userid,device,bgm_song_id;feedid,authorid,manual_tag_list,bgm_singer_id"


def flen_setup(vocab_dir, **overrides):
    """(model_fn, params) of algorithm/FLEN/flen.py on the dataset's columns, from its own create_feature_columns()"""
    from recalgorithm_amd import flags
    from recalgorithm_amd.algorithm.FLEN import flen as m
    flags.FLAGS.vocabulary_dir = vocab_dir
    fl = dict(FLAG_DEFAULTS, **overrides)
    flags.FLAGS.embedding_dim = fl["embedding_dim"]
    dense, cat, _ = m.create_feature_columns()
    return m.flen_model_fn, {
        "dense_feature_columns": dense, "category_feature_columns": cat, "embedding_dim": fl["embedding_dim"],
        "field_groups": fl["field_groups"], "hidden_units": m.parse_hidden_units(fl["hidden_units"]), "batch_norm": fl["batch_norm"],
        "dropout_rate": fl["dropout_rate"], "dicefactor_rate": fl["dicefactor_rate"], "learning_rate": fl["learning_rate"]}


def expected_variables(params, M, K=8):
    """name -> shape of every variable of the model but the embedding tables"""
    P = M * (M - 1) // 2
    want = {"dense_input/dense_logit/kernel": (16, 1), "dense_input/dense_logit/bias": (1,),
            "fwbi_part/r_mf": (P,), "fwbi_part/r_fm": (M,), "fwbi_part/bias": (K,)}
    widths = [16 + M * K] + [int(u) for u in params["hidden_units"]]
    for i in range(len(widths) - 1):
        sfx = "" if i == 0 else f"_{i}"
        want[f"deep_part/dense{sfx}/kernel"], want[f"deep_part/dense{sfx}/bias"] = (widths[i], widths[i + 1]), (widths[i + 1],)
        if params["batch_norm"]:
            for n in ("gamma", "beta", "moving_mean", "moving_variance"):
                want[f"deep_part/batch_normalization{sfx}/{n}"] = (widths[i + 1],)
    want["prediction_part/flen_logit/kernel"], want["prediction_part/flen_logit/bias"] = (K + widths[-1], 1), (1,)
    return want


def test_flags_defaults_and_call_surface():
    """(in a child process: a model script imported earlier in this one defines flags of the same names)"""
    code = ("import json, inspect; from recalgorithm_amd.algorithm.FLEN import flen as m, field_wise_bi_interaction as l; "
            "acts = {a.dest: a.default for a in m.FLAGS._parser._actions if a.dest != 'help'}; "
            "print(json.dumps({'flags': acts, 'parsed': {k: getattr(m.FLAGS, k) for k in acts}, "
            "'callables': [n for n in ('create_feature_columns', 'example_parser', 'flen_model_fn', 'main') if callable(getattr(m, n))], "
            "'layer': str(inspect.signature(l.field_wise_bi_interaction)), 'units': [m.parse_hidden_units(''), m.parse_hidden_units('32,16')]}))")
    env = dict(os.environ, PYTHONPATH=ROOT + os.pathsep + os.environ.get("PYTHONPATH", ""))
    r = subprocess.run([sys.executable, "-c", code], cwd=ROOT, env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    got = json.loads(r.stdout.strip().splitlines()[-1])
    assert {k: got["flags"][k] for k in FLAG_DEFAULTS} == FLAG_DEFAULTS and got["parsed"] == got["flags"]
    assert {"model_dir", "train_data", "vocabulary_dir", "train_steps", "ragged_capacity"} <= set(got["flags"])
    assert got["callables"] == ["create_feature_columns", "example_parser", "flen_model_fn", "main"]
    assert got["layer"] == "(input, group_of, dicefactor_rate=0.0, training=False, fused=None)"
    assert got["units"] == [[], [32, 16]]


@pytest.mark.parametrize("groups,M,hidden,bn", [(FLAG_DEFAULTS["field_groups"], 3, "32,16", True), (TWO_GROUPS, 2, "32,16", False),
                                                (FLAG_DEFAULTS["field_groups"], 3, "", True)])
def test_variables_on_the_registration_pass(groups, M, hidden, bn, tmp_path):
    from recalgorithm_amd.estimator import Estimator, ModeKeys, RunConfig
    vocab_dir = GU.write_vocab_dir(str(tmp_path / "vocabulary"))
    model_fn, params = flen_setup(vocab_dir, field_groups=groups, hidden_units=hidden, batch_norm=bn, dicefactor_rate=0.2)
    sfeats, labels = GU.string_batch()
    feats = {k: (v.float() if isinstance(v, torch.Tensor) else v) for k, v in sfeats.items()}
    lab = {"read_comment": labels.float()}
    est = Estimator(model_fn, params, RunConfig(device="cpu", seed=3, use_hip_graph=False))
    est.build(feats, lab)                    # registration pass only: no HIP call
    arrays = est.store.named_arrays()
    want = expected_variables(params, M)
    tables = sorted(k for k in arrays if k.endswith("/embedding_weights"))
    assert len(tables) == 7 and all(k.startswith("fwbi_part/input_layer") and arrays[k].shape[1] == 8 for k in tables), tables
    assert sorted(k for k in arrays if k not in tables) == sorted(want)
    for k, shape in want.items():
        assert tuple(arrays[k].shape) == shape, (k, arrays[k].shape, shape)
    assert bool((arrays["fwbi_part/r_mf"] == 1).all()) and bool((arrays["fwbi_part/r_fm"] == 0.5).all()) and not bool(arrays["fwbi_part/bias"].any())
    est.store.building = True
    try:
        with torch.no_grad():
            pred = est._call_model_fn(feats, None, ModeKeys.PREDICT)
            ev = est._call_model_fn(feats, lab, ModeKeys.EVAL)
    finally:
        est.store.building = False
    assert list(pred.predictions) == ["logit", "probabilities"] and tuple(pred.predictions["probabilities"].shape) == (48, 1)
    assert sorted(ev.eval_metric_ops) == ["eval_accuracy", "eval_auc"]
    with pytest.raises(ValueError, match="are in none"):
        model_fn(feats, lab, ModeKeys.TRAIN, dict(params, field_groups="userid;feedid"))


def test_the_product_imports_neither_the_tests_nor_the_oracle():
    files = [os.path.join(ROOT, "recalgorithm_amd", "algorithm", "FLEN", f) for f in ("__init__.py", "flen.py", "field_wise_bi_interaction.py")]
    files += [os.path.join(ROOT, "recalgorithm_amd", f) for f in ("ops.py", "nn.py", "_lib.py")] + [os.path.join(ROOT, "scripts", "bench_flen.py")]
    for f in files:
        src = open(f).read()
        assert not re.search(r"^\s*(from|import)\s+(tests|oracle)\b", src, re.M), f
    code = ("import sys; from recalgorithm_amd.algorithm.FLEN import flen; "
            "bad = [m for m in sys.modules if m.split('.')[0] in ('tests', 'oracle')]; assert not bad, bad")
    env = dict(os.environ, PYTHONPATH=ROOT + os.pathsep + os.environ.get("PYTHONPATH", ""))
    r = subprocess.run([sys.executable, "-c", code], cwd=ROOT, env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
