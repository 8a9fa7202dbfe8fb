"""-m gpu: every kernel entry of the old families of recalgo.h ON the edge of its domain and one step past it (tests/domain.py).

At-limit cases: one call per `at` tag, the quantity under test on its boundary, everything else the entry's smallest call.
Every output and gradient is judged against the float64 functions of oracle/ref_ops.py with tests/util.assert_close and the
float32 oracle as ref32, with the reduced= / strict_* arguments the entry's contiguous test passes (the gathers: bit-exact),
inside tests/redzone.py's guard: a structure that is exactly full shows an overrun as a touched redzone or a NaN.
Refusal cases: one call per `outside` tag.  The buffers are those of the valid neighbour; the call returns
hipErrorInvalidValue, every output is still 0xFF and a synchronize raises nothing.
B == 0 (M == 0): the at-limit case of `B >= 0` - the entry returns 0 and writes nothing, parameter gradients included (the
backwards that overwrite parameter gradients require B > 0: there B == 0 is a refusal case).
The case lists are spelled out below; tests/test_domain_host.py holds them against the table, in both directions.
"""
import ctypes
import math

import pytest
import torch

from oracle import ref_ops as R
from recalgorithm_amd import _lib
from tests.domain import BADLIVE, ENTRIES, MISALIGNED, DOMAIN, at_dims, case_id, full, outside_dims
from tests.redzone import guarded
from tests.util import assert_bit_exact, assert_close

pytestmark = pytest.mark.gpu

# entry (without recalgo_) -> the tags of its cases
AT_TAGS = {
    "embedding_gather_fwd": "B0 F1 K1 base",
    "embedding_gather_bwd": "B0 F1 K1 K64 K64,g_col1 base",
    "embedding_bag_mean_bwd": "B0 K1 K64 K64,g_col1 base",
    "sequence_gather_fwd": "B0 T1 K1",
    "sequence_gather_bwd": "B0 T1 K1 K64",
    "deepfm_sparse_fwd": "B0 F1 K4 base K64 F816 F62,K64",
    "deepfm_sparse_bwd": "B0 F1 K4 base K64",
    "scatter_rows_sorted": "M0 K1",
    "cross_fwd": "B0 d4 base d1024 d1024,L6 L1 L6",
    "cross_bwd": "B1 d4 base d1024 d1024,L6 L1 L6 defer_reduce1,null:dw,null:db",
    "gather_cross_fwd": "B0 F1 K4 base F256 F16,K64,L6 L1 L6",
    "cross_layer_fwd": "B0 d4 base d2048",
    "cross_layer_bwd": "B1 d4 base d2048",
    "cin_layer_fwd": "B0 m1 Hk1 N1 N128 D4 D8 D16 D32",
    "cin_layer_bwd": "B1 m4 m128 m128,Hk128,N128 Hk1 Hk128 N1 N128 D4 D8 D16 D32 null:g_out null:g_pool",
    "din_attention_fwd": "B0 T1 T64 T64,H8 T64,H16 T64,is_softmax0 T64,H8,is_softmax0 T64,H16,is_softmax0 H4 H8 H16",
    "din_attention_bwd": "B1 T1 T64 T64,H8 T64,H16 T64,is_softmax0 T64,H8,is_softmax0 T64,H16,is_softmax0 H4 H8 H16 base",
    "din_attention_bwd_joined": "B1 T1 T64 T64,H8 T64,H16 T64,is_softmax0 T64,H8,is_softmax0 T64,H16,is_softmax0 H4 H8 H16 base "
                                "null:dq_extra,ld_extra0",
    "senet_fwd": "B0 F1 K2,reduction_dim1 reduction_dim1 reduction_dim3 F1364,K2,reduction_dim1 F69,K64,reduction_dim32",
    "senet_bwd": "B1 F1 K2,reduction_dim1 reduction_dim1 reduction_dim3 F1077,K2,reduction_dim1 F48,K64,reduction_dim32",
    "bilinear_fwd": "B0 F3 F128,K8,type0 F128,K8,type1 F128,K8,type2 K4 K8 K16 K32 K64 type0 type2 base F31,K64,type0 "
                    "F40,K64,type1 F40,K64,type2 nv1,F69,K64,type0",
    "bilinear_bwd": "B1 F3 F128,K8,type0 F128,K8,type1 F128,K8,type2 K4 K8 K16 K32 K64 type0 type2 base F61,K64,type0 "
                    "F77,K64,type1 F77,K64,type2 nv1,F127,K64,type0",
    "pnn_features_fwd": "B0 F1 K1 method0 method1 F255 method1,K255 base",
    "pnn_features_bwd": "B0 F1 K1 method0 method1 F138 F127,K16 method1,K140 base",
    "pnn_weights_fwd": "D1 F1 K1 method0 method1",
    "pnn_weights_bwd": "D1 F1 K1 method0 method1",
    "bi_interaction_fwd": "B0 F1 K1",
    "bi_interaction_bwd": "B0 F1 K1",
    "attention_pool_fwd": "B0 P1 K1 K64 P4096,K64",
    "attention_pool_bwd": "B0 P1 K1 K64 P4096,K64 P4096",
    "ffm_pairs_fwd": "B0 F2 K1",
    "ffm_pairs_bwd": "B0 F2 K1",
}
OUTSIDE_TAGS = {
    "embedding_gather_fwd": "B-1 F0 K0 out_stride11 B1<<30",
    "embedding_gather_bwd": "B-1 F0 K0 g_stride400,K65 g_stride11 badlive:live",
    "embedding_bag_mean_bwd": "B-1 K0 g_stride400,K65 g_stride3 badlive:live",
    "sequence_gather_fwd": "B-1 T0 K0 B1<<30",
    "sequence_gather_bwd": "B-1 T0 K0 K65 badlive:live B1<<30",
    "deepfm_sparse_fwd": "B-1 F0 K0 K5 K68 null:field_sum F817 K64,F63",
    "deepfm_sparse_bwd": "B-1 F0 K0 K5 K68 badlive:live badlive:live_w1",
    "scatter_rows_sorted": "M-1 K0 null:vals K1,M549755813633",
    "cross_fwd": "B-1 d0 x_stride12,out_stride12,g_stride12,d9 x_stride1028,out_stride1028,g_stride1028,d1028 L0 L7 x_stride9 "
                 "out_stride9 x_stride4 out_stride4",
    "cross_bwd": "B0 d0 x_stride12,out_stride12,g_stride12,d9 x_stride1028,out_stride1028,g_stride1028,d1028 L0 L7 x_stride9 "
                 "g_stride9 x_stride4 g_stride4 null:workspace null:dw",
    "gather_cross_fwd": "B-1 F0 K0 x_stride12,out_stride12,K5 x_stride1028,out_stride1028,F257 L0 L7 null:ids null:arena "
                        "null:row_base null:x0 null:out x_stride9 out_stride9 x_stride4 out_stride4 mis:x0",
    "cross_layer_fwd": "null:xl B-1 d0 x_stride12,out_stride12,g_stride12,d9 x_stride2052,out_stride2052,g_stride2052,d2052 "
                       "x_stride9 out_stride9 x_stride4 out_stride4",
    "cross_layer_bwd": "null:xl null:dxl null:workspace B0 d0 x_stride12,out_stride12,g_stride12,d9 "
                       "x_stride2052,out_stride2052,g_stride2052,d2052 x_stride9 g_stride9 x_stride4 g_stride4",
    "cin_layer_fwd": "B-1 m0 Hk0 N0 N129 D5",
    "cin_layer_bwd": "B0 m3 m129 Hk0 Hk129 N0 N129 D5 null:workspace null:g_out,null:g_pool",
    "din_attention_fwd": "B-1 T0 T65 ldg8,ld_extra8,H5",
    "din_attention_bwd": "B0 T0 T65 ldg8,ld_extra8,H5 null:workspace null:g_out mis:g_out",
    "din_attention_bwd_joined": "B0 T0 T65 ldg8,ld_extra8,H5 null:workspace null:g_out mis:g_out ldg0 ldg9 ld_extra3",
    "senet_fwd": "B-1 F0 K0 reduction_dim0 reduction_dim4 K2,reduction_dim1,F1365 K64,reduction_dim32,F70",
    "senet_bwd": "B0 F0 K0 reduction_dim0 reduction_dim4 null:workspace K2,reduction_dim1,F1078 K64,reduction_dim32,F49",
    "bilinear_fwd": "B-1 F2 K8,F129 out_stride32,g_stride32,K12 type-1 type3 null:x0 null:w0 null:w1 out_stride9 "
                    "out_stride16,out_col1 out_stride4 K64,type0,F32 K64,type1,F41 K64,type2,F41 nv1,K64,type0,F70",
    "bilinear_bwd": "B0 F2 K8,F129 out_stride32,g_stride32,K12 type-1 type3 null:x0 null:w0 null:dx0 null:dw0 null:g "
                    "null:workspace null:w1 null:dx1 null:dw1 g_stride9 g_stride16,g_col1 g_stride4 K64,type0,F62 "
                    "K64,type1,F78 K64,type2,F78 nv1,K64,type0,F128",
    "pnn_features_fwd": "B-1 F0 K0 method2 ld_phi40000,F256 method1,ld_phi40000,K256 ld_phi5",
    "pnn_features_bwd": "B-1 F0 K0 method2 ld_dphi40000,F139 method1,ld_dphi40000,K141 ld_dphi5",
    "pnn_weights_fwd": "D0 F0 K0 method2",
    "pnn_weights_bwd": "D0 F0 K0 method2",
    "bi_interaction_fwd": "B-1 F0 K0 K2,B1<<30",
    "bi_interaction_bwd": "B-1 F0 K0 K2,B1<<30",
    "attention_pool_fwd": "B-1 P0 K0 K65",
    "attention_pool_bwd": "B-1 P0 K0 K65 P4097",
    "ffm_pairs_fwd": "B-1 F1 K0",
    "ffm_pairs_bwd": "B-1 F1 K0 B1<<30",
}
AT_CASES = {case_id("recalgo_" + e, t): ("recalgo_" + e, t) for e, tags in AT_TAGS.items() for t in tags.split()}
OUTSIDE_CASES = {case_id("recalgo_" + e, t): ("recalgo_" + e, t) for e, tags in OUTSIDE_TAGS.items() for t in tags.split()}

_LIVE_T = _lib.STRUCTS["recalgo_live_t"]
_REFS = {}          # inputs and references: computed once per shape, shared, left unchanged


def _cached(key, make):
    if key not in _REFS:
        _REFS[key] = make()
    return _REFS[key]


def _st():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def _nan(dev, *shape):
    return torch.full((4 * math.prod(shape),), 0xFF, dtype=torch.uint8, device=dev).view(torch.float32).view(*shape)


def _bytes(dev, n):
    return torch.full((max(int(n), 16),), 0xFF, dtype=torch.uint8, device=dev)


def _win(dev, values, stride, col=0):
    """a float input [rows, width] as columns [col, col + width) of a NaN matrix with row stride `stride`"""
    values = values.reshape(values.shape[0], -1)
    t = torch.full((values.shape[0], stride), float("nan"))
    t[:, col:col + values.shape[1]] = values
    return t.to(dev)


def _gen(*dims):
    return torch.Generator().manual_seed(sum((i + 1) * 131 * int(d) for i, d in enumerate(dims)) % (1 << 31))


def _oracle2(fn):
    """fn(dtype) -> tensors: the float64 and the float32 run, zipped per tensor"""
    return list(zip(fn(torch.float64), fn(torch.float32)))


# ---- embed.hip ------------------------------------------------------------------------------------------------------------
V = 7               # rows per table of the lookup cases: ids repeat within a batch of 5


def _gather_ref(B, F, K):
    def make():
        gen = _gen(B, F, K)
        arena = torch.randn(F * V, K, generator=gen)
        rb = torch.arange(F, dtype=torch.int64) * V
        ids = torch.randint(-1, V, (B, F), generator=gen)
        rows = torch.cat([R.embedding_lookup_single(ids[:, f], arena[f * V:(f + 1) * V]) for f in range(F)], dim=1)
        g = torch.randn(B, F * K, generator=gen)
        valid = ids >= 0
        at, pieces = (ids + rb)[valid], g.view(B, F, K)[valid]
        return dict(arena=arena, rb=rb, ids=ids, rows=rows, g=g,
                    grad=(torch.zeros(F * V, K, dtype=torch.float64).index_add_(0, at, pieces.double()),
                          torch.zeros(F * V, K).index_add_(0, at, pieces)))
    return _cached(("gather", B, F, K), make)


def drv_embedding_gather_fwd(lib, dev, v):
    B, F, K, s, c = v["B"], v["F"], v["K"], v["out_stride"], v["out_col"]
    r = _gather_ref(B, F, K)
    t = dict(ids=r["ids"].to(dev), arena=r["arena"].to(dev), row_base=r["rb"].to(dev), out=_nan(dev, B, s))
    return t, ["out"], lambda: assert_bit_exact(t["out"][:, c:c + F * K].contiguous(), r["rows"], "gather: table rows")


def drv_embedding_gather_bwd(lib, dev, v):
    B, F, K, s, c = v["B"], v["F"], v["K"], v["g_stride"], v["g_col"]
    r = _gather_ref(B, F, K)
    t = dict(ids=r["ids"].to(dev), g=_win(dev, r["g"], s, c), row_base=r["rb"].to(dev), grad_arena=torch.zeros(F * V, K, device=dev))
    return t, ["grad_arena"], lambda: assert_close(t["grad_arena"], r["grad"][0], what="gather bwd", reduced=True, ref32=r["grad"][1])


def _bags(gen, B, longest):
    lens = torch.randint(0, longest + 1, (B,), generator=gen)
    lens[-1], lens[0] = 0, longest
    offsets = torch.zeros(B + 1, dtype=torch.int64)
    offsets[1:] = lens.cumsum(0)
    values = torch.randint(-1, V, (int(offsets[-1]),), generator=gen)
    return values, offsets


def drv_embedding_bag_mean_bwd(lib, dev, v):
    B, K, s, c = v["B"], v["K"], v["g_stride"], v["g_col"]

    def make():
        gen = _gen(B, K, 3)
        values, offsets = _bags(gen, B, 3)
        table, g = torch.randn(V, K, generator=gen), torch.randn(B, K, generator=gen)

        def oracle(dt):
            tt = table.to(dt).requires_grad_(True)
            R.embedding_lookup_mean(values, offsets, tt).backward(g.to(dt))
            return [tt.grad]
        return values, offsets, g, _oracle2(oracle)
    values, offsets, g, (grad,) = _cached(("bag", B, K), make)
    t = dict(values=values.to(dev), offsets=offsets.to(dev), g=_win(dev, g, s, c), grad_table=torch.zeros(V, K, device=dev))
    return t, ["grad_table"], lambda: assert_close(t["grad_table"], grad[0], what="bag mean bwd", reduced=True, ref32=grad[1])


def _seq_ref(B, T, K):
    def make():
        gen = _gen(B, T, K, 5)
        values, offsets = _bags(gen, B, T + 2)                   # (some histories longer than T: truncated)
        table, g = torch.randn(V, K, generator=gen), torch.randn(B, T, K, generator=gen)
        rows, lens = R.sequence_lookup(values, offsets, table, T)

        def oracle(dt):
            tt = table.to(dt).requires_grad_(True)
            R.sequence_lookup(values, offsets, tt, T)[0].backward(g.to(dt))
            return [tt.grad]
        return dict(values=values, offsets=offsets, table=table, g=g, rows=rows, lens=lens.clamp(max=T), grad=_oracle2(oracle)[0])
    return _cached(("seq", B, T, K), make)


def drv_sequence_gather_fwd(lib, dev, v):
    B, T, K = v["B"], v["T"], v["K"]
    r = _seq_ref(B, T, K)
    t = dict(values=r["values"].to(dev), offsets=r["offsets"].to(dev), table=r["table"].to(dev), out=_nan(dev, B, T, K),
             seq_len=torch.full((B,), -1, dtype=torch.int32, device=dev))

    def judge():
        assert_bit_exact(t["out"], r["rows"], "sequence gather")
        assert torch.equal(t["seq_len"].cpu().long(), r["lens"]), "seq_len"
    return t, ["out", "seq_len"], judge


def drv_sequence_gather_bwd(lib, dev, v):
    B, T, K = v["B"], v["T"], v["K"]
    r = _seq_ref(B, T, K)
    t = dict(values=r["values"].to(dev), offsets=r["offsets"].to(dev), g=r["g"].to(dev), grad_table=torch.zeros(V, K, device=dev))
    return t, ["grad_table"], lambda: assert_close(t["grad_table"], r["grad"][0], what="sequence gather bwd", reduced=True,
                                                   ref32=r["grad"][1])


def _deepfm_ref(B, F, K):
    def make():
        gen = _gen(B, F, K, 7)
        arena = torch.randn(F * V, K, generator=gen) / math.sqrt(F)       # (fm2 sums F rows: 1 / sqrt(fan_in))
        w1 = torch.randn(F * V, generator=gen) / math.sqrt(F)
        bias = torch.tensor([0.37])
        ids = torch.randint(-1, V, (B, F), generator=gen)
        ge, g1, g2 = torch.randn(B, F * K, generator=gen), torch.randn(B, 1, generator=gen), torch.randn(B, 1, generator=gen)

        def oracle(dt):
            W, W1, bb = (x.to(dt).requires_grad_(True) for x in (arena, w1, bias))
            fields = [R.embedding_lookup_single(ids[:, f], W[f * V:(f + 1) * V]) for f in range(F)]
            o1 = R.indicator_first_order([ids[:, f] for f in range(F)], [W1[f * V:(f + 1) * V] for f in range(F)], bb[0])
            o2 = R.fm_second_order(fields)
            emb = torch.cat(fields, 1)
            torch.autograd.backward([emb, o1, o2], [ge.to(dt), g1.to(dt).reshape(o1.shape), g2.to(dt).reshape(o2.shape)])
            return [emb.detach(), o1.detach(), o2.detach(), sum(fields).detach(), W.grad, W1.grad]
        return dict(arena=arena, w1=w1, bias=bias, ids=ids, rb=torch.arange(F, dtype=torch.int64) * V, ge=ge, g1=g1, g2=g2,
                    o=_oracle2(oracle))
    return _cached(("deepfm", B, F, K), make)


def drv_deepfm_sparse_fwd(lib, dev, v):
    B, F, K = v["B"], v["F"], v["K"]
    r = _deepfm_ref(B, F, K)
    t = dict(ids=r["ids"].to(dev), arena=r["arena"].to(dev), w1=r["w1"].to(dev), bias=r["bias"].to(dev), row_base=r["rb"].to(dev),
             emb=_nan(dev, B, F * K), fm1=_nan(dev, B), fm2=_nan(dev, B), field_sum=_nan(dev, B, K))

    def judge():
        emb, o1, o2, fs = r["o"][:4]
        assert_bit_exact(t["emb"], emb[1], "deep_input")
        assert_close(t["fm1"], o1[0], what="fm first order", ref32=o1[1])
        assert_close(t["fm2"], o2[0], what="fm second order", ref32=o2[1])
        assert_close(t["field_sum"], fs[0], what="field_sum", ref32=fs[1])
    return t, ["emb", "fm1", "fm2", "field_sum"], judge


def drv_deepfm_sparse_bwd(lib, dev, v):
    B, F, K = v["B"], v["F"], v["K"]
    r = _deepfm_ref(B, F, K)
    emb, _, _, fs, gW, gW1 = r["o"]
    t = dict(ids=r["ids"].to(dev), emb=emb[1].to(dev), field_sum=fs[1].to(dev), g_emb=r["ge"].to(dev), g_fm1=r["g1"].reshape(-1).to(dev),
             g_fm2=r["g2"].reshape(-1).to(dev), row_base=r["rb"].to(dev), grad_arena=torch.zeros(F * V, K, device=dev),
             grad_w1=torch.zeros(F * V, device=dev))

    def judge():
        assert_close(t["grad_arena"], gW[0], what="deepfm d(table)", reduced=True, ref32=gW[1])
        assert_close(t["grad_w1"], gW1[0], what="deepfm d(w1)", reduced=True, ref32=gW1[1])
    return t, ["grad_arena", "grad_w1"], judge


def drv_scatter_rows_sorted(lib, dev, v):
    M, K, rows = v["M"], v["K"], 11

    def make():
        gen = _gen(M, K, 11)
        req = torch.randint(-1, rows, (M,), generator=gen)
        sorted_rows, perm = torch.sort(req, stable=True)
        vals, base = torch.randn(M, K, generator=gen), torch.randn(rows, K, generator=gen)
        ok = req >= 0
        return sorted_rows, perm, vals, base, base.double().index_add_(0, req[ok], vals[ok].double()), \
            base.clone().index_add_(0, req[ok], vals[ok])
    sorted_rows, perm, vals, base, ref, ref32 = _cached(("sorted", M, K), make)
    t = dict(sorted_rows=sorted_rows.to(dev), perm=perm.to(dev), vals=vals.to(dev), grad=base.to(dev).clone())
    return t, ["grad"], lambda: assert_close(t["grad"], ref, what="sorted scatter", reduced=True, ref32=ref32)


# ---- cross.hip ------------------------------------------------------------------------------------------------------------
def _cross_ref(B, d, L):
    from tests.test_gpu_windows import _cross_case
    return _cross_case(B, d, L)


def drv_cross_fwd(lib, dev, v):
    B, d, L = v["B"], v["d"], v["L"]
    x0, w, b, _, _, (ref, *_), (r32, *_) = _cross_ref(B, d, L)
    t = dict(x0=_win(dev, x0, v["x_stride"]), w=w.to(dev), b=b.to(dev), out=_nan(dev, B, v["out_stride"]))
    return t, ["out"], lambda: assert_close(t["out"][:, :d], ref, what="cross fwd", ref32=r32)


def drv_cross_bwd(lib, dev, v):
    B, d, L = v["B"], v["d"], v["L"]
    x0, w, b, g, _, (_, gx, gw, gb), (_, gx32, gw32, gb32) = _cross_ref(B, d, L)
    ws = _bytes(dev, lib.recalgo_cross_bwd_workspace_bytes(B, d, L))
    t = dict(x0=_win(dev, x0, v["x_stride"]), w=w.to(dev), b=b.to(dev), g=_win(dev, g, v["g_stride"]), dx0=_nan(dev, B, v["x_stride"]),
             dw=_nan(dev, L, d), db=_nan(dev, L, d), workspace=ws)

    def judge():
        assert_close(t["dx0"][:, :d], gx, what="cross dx0", ref32=gx32)
        if v["defer_reduce"]:       # the partial rows stay in the workspace; dw / db are their column sums
            rows = ws.view(torch.float32).view(-1, 2 * L * d).cpu()
            assert rows.shape[0] == lib.recalgo_cross_bwd_partial_rows(B) and bool(torch.isfinite(rows).all())
            dw, db = rows[:, :L * d].double().sum(0), rows[:, L * d:].double().sum(0)
            assert bool(torch.isnan(t["dw"]).all()) and bool(torch.isnan(t["db"]).all())
        else:
            dw, db = t["dw"], t["db"]
        assert_close(dw, gw, what="cross dw", reduced=True, ref32=gw32)
        assert_close(db, gb, what="cross db", reduced=True, ref32=gb32)
    return t, ["dx0", "dw", "db", "workspace"], judge


def drv_gather_cross_fwd(lib, dev, v):
    B, F, K, L = v["B"], v["F"], v["K"], v["L"]
    d = F * K
    r = _gather_ref(B, F, K)

    def make():
        gen = _gen(B, F, K, L)
        w, b = torch.randn(L, d, generator=gen) / math.sqrt(d), torch.randn(L, d, generator=gen) * 0.1
        stack = lambda dt: R.cross_stack(r["rows"].to(dt), [w[l].to(dt).unsqueeze(1) for l in range(L)],
                                         [b[l].to(dt).unsqueeze(1) for l in range(L)])
        return w, b, stack(torch.float64), stack(torch.float32)
    w, b, ref, r32 = _cached(("gather_cross", B, F, K, L), make)
    t = dict(ids=r["ids"].to(dev), arena=r["arena"].to(dev), row_base=r["rb"].to(dev), w=w.to(dev), b=b.to(dev),
             x0=_nan(dev, B, v["x_stride"]), out=_nan(dev, B, v["out_stride"]))

    def judge():
        assert_bit_exact(t["x0"][:, :d].contiguous(), r["rows"], "gather_cross x0: table rows")
        assert_close(t["out"][:, :d], ref, what="gather_cross out", ref32=r32)
    return t, ["x0", "out"], judge


def _layer_ref(B, d):
    def make():
        gen = _gen(B, d, 17)
        x0, xl = torch.randn(B, d, generator=gen), torch.randn(B, d, generator=gen)
        w, b = torch.randn(d, 1, generator=gen) / math.sqrt(d), torch.randn(d, 1, generator=gen)
        g = torch.randn(B, d, generator=gen)

        def oracle(dt):
            a = [x.to(dt).requires_grad_(True) for x in (x0, xl, w, b)]
            out = R.cross_layer(*a)
            out.backward(g.to(dt))
            return [out.detach()] + [x.grad for x in a]
        return x0, xl, w, b, g, _oracle2(oracle)
    return _cached(("cross_layer", B, d), make)


def drv_cross_layer_fwd(lib, dev, v):
    B, d = v["B"], v["d"]
    x0, xl, w, b, _, o = _layer_ref(B, d)
    t = dict(x0=_win(dev, x0, v["x_stride"]), xl=_win(dev, xl, v["x_stride"]), w=w.to(dev), b=b.to(dev), out=_nan(dev, B, v["out_stride"]))
    return t, ["out"], lambda: assert_close(t["out"][:, :d], o[0][0], what="cross_layer fwd", ref32=o[0][1])


def drv_cross_layer_bwd(lib, dev, v):
    B, d = v["B"], v["d"]
    x0, xl, w, b, g, o = _layer_ref(B, d)
    t = dict(x0=_win(dev, x0, v["x_stride"]), xl=_win(dev, xl, v["x_stride"]), w=w.to(dev), b=b.to(dev), g=_win(dev, g, v["g_stride"]),
             dx0=_nan(dev, B, v["x_stride"]), dxl=_nan(dev, B, v["x_stride"]), dw=_nan(dev, d), db=_nan(dev, d),
             workspace=_bytes(dev, lib.recalgo_cross_bwd_workspace_bytes(B, d, 1)))

    def judge():
        for k, nm in enumerate(("dx0", "dxl", "dw", "db")):
            got = t[nm][:, :d] if k < 2 else t[nm]
            assert_close(got, o[1 + k][0], what=f"cross_layer {nm}", reduced=True, ref32=o[1 + k][1])
    return t, ["dx0", "dxl", "dw", "db", "workspace"], judge


# ---- cin.hip --------------------------------------------------------------------------------------------------------------
def _cin_ref(B, m, Hk, N, D, with_go, with_gp):
    def make():
        gen = _gen(B, m, Hk, N, D)
        x0, xk = torch.randn(B, m, D, generator=gen), torch.randn(B, Hk, D, generator=gen)
        w = torch.randn(1, Hk * m, N, generator=gen) / (Hk * m) ** 0.5
        go, gp = torch.randn(B, N, D, generator=gen), torch.randn(B, N, generator=gen)

        def oracle(dt):
            a = [x.to(dt, copy=True).requires_grad_(True) for x in (x0, xk, w)]
            r = R.cin_layer(*a)
            outs, grads = ([r] if with_go else []) + ([r.sum(-1)] if with_gp else []), \
                ([go.to(dt)] if with_go else []) + ([gp.to(dt)] if with_gp else [])
            torch.autograd.backward(outs, grads)
            return [r.detach(), r.detach().sum(-1)] + [x.grad for x in a]
        return x0, xk, w, go, gp, _oracle2(oracle)
    return _cached(("cin", B, m, Hk, N, D, with_go, with_gp), make)


def drv_cin_layer_fwd(lib, dev, v):
    B, m, Hk, N, D = (v[k] for k in ("B", "m", "Hk", "N", "D"))
    x0, xk, w, _, _, o = _cin_ref(B, m, Hk, N, D, True, True)
    t = dict(x0=x0.to(dev), xk=xk.to(dev), filters=w.to(dev), out=_nan(dev, B, N, D), pool=_nan(dev, B, v["pool_stride"]))

    def judge():
        assert_close(t["out"], o[0][0], what="cin fwd", reduced=True, ref32=o[0][1])
        assert_close(t["pool"][:, :N], o[1][0], what="cin pooled", reduced=True, ref32=o[1][1])
    return t, ["out", "pool"], judge


def drv_cin_layer_bwd(lib, dev, v):
    B, m, Hk, N, D = (v[k] for k in ("B", "m", "Hk", "N", "D"))
    with_go, with_gp = bool(v["g_out"]), bool(v["g_pool"])
    x0, xk, w, go, gp, o = _cin_ref(B, m, Hk, N, D, with_go or not with_gp, with_gp or not with_go)
    t = dict(x0=x0.to(dev), xk=xk.to(dev), filters=w.to(dev), g_out=go.to(dev), g_pool=_win(dev, gp, v["pool_stride"]),
             dx0=_nan(dev, B, m, D), dxk=_nan(dev, B, Hk, D), dfilters=_nan(dev, 1, Hk * m, N),
             workspace=_bytes(dev, lib.recalgo_cin_layer_bwd_workspace_bytes(B, m, Hk, N, D)))
    factor = 2.5 if m > 32 else 1.5              # (tests/test_gpu_dispatch_arms._cin_run: the one-contraction arm of m > 32)

    def judge():
        assert_close(t["dx0"], o[2][0], what="cin dx0", reduced=True, ref32=o[2][1], strict_factor=factor)
        assert_close(t["dxk"], o[3][0], what="cin dxk", reduced=True, ref32=o[3][1], strict_factor=factor)
        assert_close(t["dfilters"], o[4][0], what="cin dW", reduced=True, ref32=o[4][1])
    return t, ["dx0", "dxk", "dfilters", "workspace"], judge


# ---- din.hip --------------------------------------------------------------------------------------------------------------
_DIN_P = ("f1_w", "f1_b", "f2_w", "f2_b", "f3_w", "f3_b")


def _din_ref(B, T, H, soft):
    def make():
        gen = _gen(B, T, H)
        q = torch.randn(B, H, generator=gen)
        lens = torch.randint(0, T + 1, (B,), generator=gen)
        lens[0] = 0
        if B > 1:
            lens[1] = T
        keys = torch.randn(B, T, H, generator=gen) * (torch.arange(T).unsqueeze(0) < lens.unsqueeze(1)).unsqueeze(-1)
        ws = [torch.randn(4 * H, 64, generator=gen) / (4 * H) ** 0.5, torch.randn(64, generator=gen) * 0.1,
              torch.randn(64, 32, generator=gen) / 8.0, torch.randn(32, generator=gen) * 0.1,
              torch.randn(32, 1, generator=gen) / 32 ** 0.5, torch.randn(1, generator=gen) * 0.1]     # (tests/test_gpu_din.make)
        g, extra = torch.randn(B, H, generator=gen), torch.randn(B, H, generator=gen)

        def oracle(dt):
            a = [x.to(dt).requires_grad_(True) for x in [q, keys] + ws]
            out = R.din_attention(a[0], a[1], lens, *a[2:], is_softmax=soft)
            out.backward(g.to(dt))
            return [out.detach()] + [x.grad for x in a]
        return q, keys, lens.to(torch.int32), ws, g, extra, _oracle2(oracle)
    return _cached(("din", B, T, H, soft), make)


def _din_inputs(dev, q, keys, lens, ws):
    return dict(query=q.to(dev), keys=keys.to(dev), keys_length=lens.to(dev), **{n: w.to(dev) for n, w in zip(_DIN_P, ws)})


def drv_din_attention_fwd(lib, dev, v):
    B, T, H = v["B"], v["T"], v["H"]
    q, keys, lens, ws, _, _, o = _din_ref(B, T, H, bool(v["is_softmax"]))
    t = dict(_din_inputs(dev, q, keys, lens, ws), out=_nan(dev, B, H))
    return t, ["out"], lambda: assert_close(t["out"], o[0][0], what="din fwd", ref32=o[0][1])


def drv_din_attention_bwd(lib, dev, v, joined=False):
    B, T, H, soft = v["B"], v["T"], v["H"], bool(v["is_softmax"])
    q, keys, lens, ws, g, extra, o = _din_ref(B, T, H, soft)
    grads = {"d_" + n: _nan(dev, *w.shape) for n, w in zip(_DIN_P, ws)}
    t = dict(_din_inputs(dev, q, keys, lens, ws), g_out=_win(dev, g, v["ldg"]) if joined else g.to(dev), dquery=_nan(dev, B, H),
             dkeys=_nan(dev, B, T, H), **grads, workspace=_bytes(dev, lib.recalgo_din_attention_bwd_workspace_bytes(B, T, H)))
    with_extra = joined and bool(v["dq_extra"])
    if joined:
        t["dq_extra"] = _win(dev, extra, max(v["ld_extra"], H))

    def judge():
        assert_close(t["dquery"], o[1][0] + extra.double() if with_extra else o[1][0], what="din dq",
                     ref32=o[1][1] + extra if with_extra else o[1][1])
        assert_close(t["dkeys"], o[2][0], what="din dkeys", ref32=o[2][1])
        for i, nm in enumerate(_DIN_P):
            if nm == "f3_b" and soft:
                # (tests/test_gpu_din.py) softmax is shift invariant: d/d(f3 bias) is pure cancellation noise; judged at the
                # scale of its terms (|d f3_w| is sum_t ds_t * h2, the same size)
                scale = float(o[7][0].abs().max())
                assert float((t["d_f3_b"].cpu().double() - o[8][0]).abs().max()) <= 1e-5 * max(scale, 1e-30)
                continue
            assert_close(t["d_" + nm], o[3 + i][0], what=f"din d{nm}", reduced=True, ref32=o[3 + i][1])
    return t, ["dquery", "dkeys", *grads, "workspace"], judge


def drv_din_attention_bwd_joined(lib, dev, v):
    return drv_din_attention_bwd(lib, dev, v, joined=True)


# ---- fibinet.hip ----------------------------------------------------------------------------------------------------------
def _senet_ref(B, F, K, Rd):
    def make():
        gen = _gen(B, F, K, Rd)
        E, g = torch.randn(B, F, K, generator=gen), torch.randn(B, F, K, generator=gen)
        w1 = torch.randn(F, Rd, generator=gen) * 2.0 / math.sqrt(F)          # (1 / sqrt(fan_in), as 0.4 is at F = 26)
        w2 = torch.randn(Rd, F, generator=gen) * 0.4

        def oracle(dt):
            a = [x.to(dt).requires_grad_(True) for x in (E, w1, w2)]
            out = R.senet(*a)
            out.backward(g.to(dt))
            return [out.detach(), a[0].grad, a[1].grad, a[2].grad, torch.relu(torch.relu(a[0].detach().mean(-1) @ a[1].detach()) @ a[2].detach())]
        return E, w1, w2, g, _oracle2(oracle)
    return _cached(("senet", B, F, K, Rd), make)


def drv_senet_fwd(lib, dev, v):
    B, F, K, Rd = v["B"], v["F"], v["K"], v["reduction_dim"]
    E, w1, w2, _, o = _senet_ref(B, F, K, Rd)
    t = dict(emb=E.to(dev), w1=w1.to(dev), w2=w2.to(dev), v_out=_nan(dev, B, F, K), a_out=_nan(dev, B, F))

    def judge():
        assert_close(t["v_out"], o[0][0], what="senet out", ref32=o[0][1], strict_slack=4 * K)      # (one gate value scales K outputs)
        assert_close(t["a_out"], o[4][0], what="senet gates", ref32=o[4][1])
    return t, ["v_out", "a_out"], judge


def drv_senet_bwd(lib, dev, v):
    B, F, K, Rd = v["B"], v["F"], v["K"], v["reduction_dim"]
    E, w1, w2, g, o = _senet_ref(B, F, K, Rd)
    t = dict(emb=E.to(dev), w1=w1.to(dev), w2=w2.to(dev), g_v=g.to(dev), d_emb=_nan(dev, B, F, K), dw1=_nan(dev, F, Rd),
             dw2=_nan(dev, Rd, F), workspace=_bytes(dev, lib.recalgo_senet_bwd_workspace_bytes(B, F, K, Rd)))

    def judge():
        assert_close(t["d_emb"], o[1][0], what="senet dE", ref32=o[1][1], strict_slack=4 * K)
        assert_close(t["dw1"], o[2][0], what="senet dw1", reduced=True, ref32=o[2][1])
        assert_close(t["dw2"], o[3][0], what="senet dw2", reduced=True, ref32=o[3][1])
    return t, ["d_emb", "dw1", "dw2", "workspace"], judge


_BTYPE = ("all", "each", "interaction")


def _bilinear_ref(btype, B, F, K, nv):
    def make():
        gen = _gen(B, F, K, nv, len(btype))
        n = {"all": None, "each": F - 1, "interaction": F * (F - 1) // 2}[btype]
        xs = [torch.randn(B, F, K, generator=gen) for _ in range(nv)]
        ws = [torch.randn(*((K, K) if n is None else (n, K, K)), generator=gen) / math.sqrt(K) for _ in range(nv)]
        P = (F - 1) * (F - 2) // 2
        g = torch.randn(B, P, nv * K, generator=gen)

        def oracle(dt):
            # (each / interaction: the oracle indexes w[k]; a list of leaf slices keeps autograd from filling a whole [n, K, K]
            # zero gradient per pair - 8001 of them at F = 128)
            xd = [x.to(dt, copy=True).requires_grad_(True) for x in xs]
            wd = [w.to(dt, copy=True).requires_grad_(True) if n is None else [s.to(dt, copy=True).requires_grad_(True) for s in w]
                  for w in ws]
            r = torch.cat([R.bilinear_interaction(x, w, btype) for x, w in zip(xd, wd)], dim=-1)
            r.backward(g.to(dt))
            dws = [w.grad if n is None else torch.stack([torch.zeros_like(s) if s.grad is None else s.grad for s in w]) for w in wd]
            return [r.detach()] + [x.grad for x in xd] + dws
        return xs, ws, g, _oracle2(oracle)
    return _cached(("bilinear", btype, B, F, K, nv), make)


def drv_bilinear_fwd(lib, dev, v):
    B, F, K, nv, W = v["B"], v["F"], v["K"], v["nv"], v["nv"] * v["K"]
    xs, ws, _, o = _bilinear_ref(_BTYPE[v["type"]], B, F, K, nv)
    P, c = (F - 1) * (F - 2) // 2, v["out_col"]
    t = dict(x0=xs[0].to(dev), w0=ws[0].to(dev), out=_nan(dev, B * P, v["out_stride"]))
    if nv == 2:
        t.update(x1=xs[1].to(dev), w1=ws[1].to(dev))
    return t, ["out"], lambda: assert_close(t["out"][:, c:c + W], o[0][0], what="bilinear out", ref32=o[0][1])


def drv_bilinear_bwd(lib, dev, v):
    B, F, K, nv, T = v["B"], v["F"], v["K"], v["nv"], v["type"]
    xs, ws, g, o = _bilinear_ref(_BTYPE[T], B, F, K, nv)
    P = (F - 1) * (F - 2) // 2
    t = dict(g=_win(dev, g.view(B * P, nv * K), v["g_stride"], v["g_col"]),
             workspace=_bytes(dev, lib.recalgo_bilinear_bwd_workspace_bytes(B, F, K, nv, T)))
    for s in range(nv):       # (interaction: only the first P slices of dw are written; the rest keep their zeros)
        t.update({f"x{s}": xs[s].to(dev), f"w{s}": ws[s].to(dev), f"dx{s}": _nan(dev, B, F, K), f"dw{s}": torch.zeros_like(ws[s]).to(dev)})

    def judge():
        for s in range(nv):
            assert_close(t[f"dx{s}"], o[1 + s][0], what=f"bilinear dx{s}", ref32=o[1 + s][1])
            assert_close(t[f"dw{s}"], o[1 + nv + s][0], what=f"bilinear dw{s}", reduced=True, ref32=o[1 + nv + s][1])
            assert float(t[f"dx{s}"][:, F - 1].abs().max()) == 0.0              # quirk B-3: the last field never participates
    return t, [n for s in range(nv) for n in (f"dx{s}", f"dw{s}")] + ["workspace"], judge


# ---- pnn.hip --------------------------------------------------------------------------------------------------------------
def _pnn_ref(B, F, K, D, method):
    """the product layer as tests/test_gpu_pnn.py judges it: lp = phi @ omega against the reference's D-iteration loop, with
    the factor that is NOT under test restated in float64 from the header's definition"""
    def make():
        gen = _gen(B, F, K, D, method)
        Rr, name = (F, "IPNN") if method == 0 else (K, "OPNN")
        emb = torch.randn(B, F * K, generator=gen) * 0.5
        pw = torch.randn(*((D, F) if method == 0 else (D, K, K)), generator=gen) / math.sqrt(Rr)
        lw, bias, g = torch.zeros(F * K, D), torch.zeros(D), torch.randn(B, D, generator=gen)

        def oracle(dt):
            e, p = emb.to(dt).requires_grad_(True), pw.to(dt).requires_grad_(True)
            lp = R.pnn_product(e, lw.to(dt), p, bias.to(dt), F, K, name)[1]
            lp.backward(g.to(dt))
            return [lp.detach(), e.grad, p.grad]
        iu = torch.triu_indices(Rr, Rr)                                    # t(r, r') = r*R - r(r-1)/2 + (r' - r): row-major r <= r'
        E = emb.double().view(B, F, K)
        gram = E @ E.transpose(1, 2) if method == 0 else E.sum(1).unsqueeze(2) * E.sum(1).unsqueeze(1)
        phi = gram[:, iu[0], iu[1]]
        c = torch.where(iu[0] == iu[1], 1.0, 2.0).double()
        p64 = pw.double()
        omega = (c.unsqueeze(1) * (p64[:, iu[0]] * p64[:, iu[1]]).t()) if method == 0 else (c.unsqueeze(1) * p64[:, iu[0], iu[1]].t())
        return emb, pw, g, phi, omega, _oracle2(oracle)
    return _cached(("pnn", B, F, K, D, method), make)


def drv_pnn_features_fwd(lib, dev, v):
    B, F, K, m, ld = v["B"], v["F"], v["K"], v["method"], v["ld_phi"]
    emb, _, _, _, omega, o = _pnn_ref(B, F, K, 3, m)
    T = omega.shape[0]
    t = dict(emb=emb.to(dev), phi=_nan(dev, B, ld))

    def judge():
        assert T == lib.recalgo_pnn_feature_count(F, K, m)
        assert_close(t["phi"][:, :T].double().cpu() @ omega, o[0][0], what="lp = phi @ omega", ref32=o[0][1])
        assert ld == T or float(t["phi"][:, T:].abs().max()) == 0.0, "the padding columns are zero-filled"
    return t, ["phi"], judge


def drv_pnn_features_bwd(lib, dev, v):
    B, F, K, m, ld = v["B"], v["F"], v["K"], v["method"], v["ld_dphi"]
    emb, _, g, _, omega, o = _pnn_ref(B, F, K, 3, m)
    dphi = (g.double() @ omega.t()).float()
    t = dict(emb=emb.to(dev), dphi=_win(dev, dphi, ld), d_emb=_nan(dev, B, F * K))
    return t, ["d_emb"], lambda: assert_close(t["d_emb"], o[1][0], what="pnn d_emb", reduced=True, ref32=o[1][1])


def drv_pnn_weights_fwd(lib, dev, v):
    D, F, K, m = v["D"], v["F"], v["K"], v["method"]
    _, pw, _, phi, omega, o = _pnn_ref(5, F, K, D, m)
    t = dict(product_w=pw.to(dev), omega=_nan(dev, *omega.shape))
    return t, ["omega"], lambda: assert_close(phi @ t["omega"].double().cpu(), o[0][0], what="lp = phi @ omega", ref32=o[0][1])


def drv_pnn_weights_bwd(lib, dev, v):
    D, F, K, m = v["D"], v["F"], v["K"], v["method"]
    _, pw, g, phi, _, o = _pnn_ref(5, F, K, D, m)
    t = dict(product_w=pw.to(dev), domega=(phi.t() @ g.double()).float().to(dev), d_product_w=_nan(dev, *pw.shape))

    def judge():
        assert_close(t["d_product_w"], o[2][0], what="d_product_w", reduced=True, ref32=o[2][1])
        if m == 1:
            assert float(torch.tril(t["d_product_w"], diagonal=-1).abs().max()) == 0.0        # quirk B-10
    return t, ["d_product_w"], judge


# ---- siblings.hip ---------------------------------------------------------------------------------------------------------
def _bi_ref(B, F, K):
    def make():
        gen = _gen(B, F, K, 23)
        e, g = torch.randn(B, F, K, generator=gen), torch.randn(B, K, generator=gen)

        def oracle(dt):
            a = e.to(dt).requires_grad_(True)
            r = 0.5 * (a.sum(1) ** 2 - (a ** 2).sum(1))                    # nfm.py:163-167
            r.backward(g.to(dt))
            return [r.detach(), a.grad]
        return e, g, _oracle2(oracle)
    return _cached(("bi", B, F, K), make)


def drv_bi_interaction_fwd(lib, dev, v):
    e, _, o = _bi_ref(v["B"], v["F"], v["K"])
    t = dict(emb=e.to(dev), out=_nan(dev, v["B"], v["K"]))
    return t, ["out"], lambda: assert_close(t["out"], o[0][0], what="bi-interaction fwd", ref32=o[0][1])


def drv_bi_interaction_bwd(lib, dev, v):
    e, g, o = _bi_ref(v["B"], v["F"], v["K"])
    t = dict(emb=e.to(dev), g=g.to(dev), d_emb=_nan(dev, *e.shape))
    return t, ["d_emb"], lambda: assert_close(t["d_emb"], o[1][0], what="bi-interaction bwd", ref32=o[1][1])


def _pool_ref(B, P, K):
    def make():
        gen = _gen(B, P, K, 29)
        pairs, att, g = torch.randn(B, P, K, generator=gen), torch.randn(B, P, generator=gen) * 3, torch.randn(B, K, generator=gen)

        def oracle(dt):
            a, b = pairs.to(dt).requires_grad_(True), att.to(dt).requires_grad_(True)
            score = torch.softmax(b, dim=1)
            r = (a * score.unsqueeze(-1)).sum(1)                           # afm.py:184-188
            r.backward(g.to(dt))
            return [r.detach(), score.detach(), a.grad, b.grad]
        return pairs, att, g, _oracle2(oracle)
    return _cached(("pool", B, P, K), make)


def drv_attention_pool_fwd(lib, dev, v):
    B, P, K = v["B"], v["P"], v["K"]
    pairs, att, _, o = _pool_ref(B, P, K)
    t = dict(pairs=pairs.to(dev), att=att.to(dev), out=_nan(dev, B, K), score=_nan(dev, B, P))

    def judge():
        assert_close(t["out"], o[0][0], what="attention pool fwd", ref32=o[0][1])
        assert_close(t["score"], o[1][0], what="attention pool score", ref32=o[1][1])
    return t, ["out", "score"], judge


def drv_attention_pool_bwd(lib, dev, v):
    B, P, K = v["B"], v["P"], v["K"]
    pairs, _, g, o = _pool_ref(B, P, K)
    t = dict(pairs=pairs.to(dev), score=o[1][1].to(dev), g=g.to(dev), d_pairs=_nan(dev, B, P, K), d_att=_nan(dev, B, P))

    def judge():
        assert_close(t["d_pairs"], o[2][0], what="attention pool d pairs", ref32=o[2][1])
        assert_close(t["d_att"], o[3][0], what="attention pool d att", reduced=True, ref32=o[3][1])
    return t, ["d_pairs", "d_att"], judge


def _ffm_ref(B, F, K):
    def make():
        gen = _gen(B, F, K, 31)
        x, g = torch.randn(B, F, F - 1, K, generator=gen), torch.randn(B, 1, generator=gen)

        def oracle(dt):
            a = x.to(dt).requires_grad_(True)
            r = sum((a[:, i, j - 1, :] * a[:, j, i, :]).sum(-1, keepdim=True) for i in range(F - 1) for j in range(i + 1, F))  # ffm.py:146-160
            r.backward(g.to(dt))
            return [r.detach(), a.grad]
        return x, g, _oracle2(oracle)
    return _cached(("ffm", B, F, K), make)


def drv_ffm_pairs_fwd(lib, dev, v):
    x, _, o = _ffm_ref(v["B"], v["F"], v["K"])
    t = dict(x=x.to(dev), out=_nan(dev, v["B"]))
    return t, ["out"], lambda: assert_close(t["out"], o[0][0], what="ffm pairs fwd", reduced=True, ref32=o[0][1])


def drv_ffm_pairs_bwd(lib, dev, v):
    x, g, o = _ffm_ref(v["B"], v["F"], v["K"])
    t = dict(x=x.to(dev), g=g.reshape(-1).to(dev), dx=_nan(dev, *x.shape))
    return t, ["dx"], lambda: assert_close(t["dx"], o[1][0], what="ffm pairs bwd", ref32=o[1][1])


# ---- one call ---------------------------------------------------------------------------------------------------------------
def _call(lib, dev, entry, v, t):
    """the entry with the arguments `v` (tests/domain.full): integers as they are; a pointer NULL, the driver's tensor, that
    tensor 4 bytes on, or a recalgo_live_t without its list - by its state in v"""
    args, keep = [], []
    for name, how in ENTRIES[entry]["args"]:
        s = v[name]
        if how == "int":
            args.append(s)
        elif s == 0:
            args.append(None)
        elif s == BADLIVE:
            keep.append(torch.zeros(16, dtype=torch.uint8, device=dev))
            keep.append((_LIVE_T * 1)(_LIVE_T(keep[0].data_ptr(), None, None, 0)))
            args.append(keep[1])
        else:
            args.append(ctypes.c_void_p(t[name].data_ptr() + (4 if s == MISALIGNED else 0)))
    return getattr(lib, entry)(*args, _st())


def _poison(t, outs):
    for n in outs:
        t[n].view(-1).view(torch.uint8).fill_(0xFF)


def _untouched(t, outs, what):
    torch.cuda.synchronize()
    for n in outs:
        assert bool((t[n].view(-1).view(torch.uint8) == 0xFF).all()), f"{what}: `{n}` was written"


def _driver(entry):
    return globals()["drv_" + entry[len("recalgo_"):]]


@pytest.mark.parametrize("cid", list(AT_CASES))
def test_at_limit(dev, cid):
    entry, tag = AT_CASES[cid]
    dims = at_dims(entry, tag)
    empty = [k for k in ("B", "M") if dims.get(k) == 0]
    with guarded():
        lib = _lib.load()
        if empty:            # buffers of the smallest call; B = 0: returns 0 and writes nothing
            v = full(entry, {**dims, empty[0]: ENTRIES[entry]["base"][empty[0]]})
            t, outs, _ = _driver(entry)(lib, dev, v)
            _poison(t, outs)
            assert _call(lib, dev, entry, {**v, empty[0]: 0}, t) == 0
            _untouched(t, outs, cid)
        else:
            v = full(entry, dims)
            t, outs, judge = _driver(entry)(lib, dev, v)
            assert _call(lib, dev, entry, v, t) == 0
            judge()


@pytest.mark.parametrize("cid", list(OUTSIDE_CASES))
def test_refused_before_any_launch(dev, cid):
    entry, tag = OUTSIDE_CASES[cid]
    rows = [r for r in DOMAIN[entry].values() if tag in r.outside]
    assert len(rows) == 1, f"{cid}: the refusal of exactly one row"
    neighbour, change = outside_dims(entry, rows[0], tag)
    with guarded():
        lib = _lib.load()
        v = full(entry, neighbour)
        t, outs, _ = _driver(entry)(lib, dev, v)
        _poison(t, outs)
        with pytest.raises(_lib.RecalgoError, match="failed with hipError_t=1$"):
            _call(lib, dev, entry, {**v, **change}, t)
        _untouched(t, outs, cid)
