"""The domain of every kernel entry of the old families of include/recalgo.h, as a table (plain Python, no device).

DOMAIN[entry] has ONE row per top-level `&&` conjunct of the entry's RECALGO_REQUIRE lines in csrc/*.hip
(tests/test_domain_host.py cuts the conjuncts out of the source and compares both ways).  A row names
  text       the conjunct, whitespace-normalised, as the source spells it;
  kind       limit | divisibility | set | stride | alignment | lds | pointer | mode;
  quantity   the argument(s) a case moves to reach / leave the conjunct's boundary ("F|K": either, by mode);
  at         tags of the tests/test_gpu_domain.py cases that run the entry ON the boundary (one per end / member);
  outside    tags of the refusal cases one step past it;
  also       other conjuncts that cannot hold once this one fails (K > 0 where 0 < reduction_dim < K is required too);
  not_driven instead of `at`: why no at-limit case exists (only: the smallest instance is too large).
A case id is "<entry without recalgo_>-<tag>".  A tag spells the case: comma-separated items NAME<int> (the argument takes
that value; "B1<<30"), null:NAME (a NULL pointer), mis:NAME (a pointer 4 bytes past a 16-byte boundary), badlive:NAME (a
recalgo_live_t with row_live but no live_list), or "base" (the entry's smallest call, ENTRIES[entry]["base"]).  An at-limit
case is base + items.  In a refusal case the items that name the row's quantity are the CHANGE, the others belong to the
valid neighbour the change is applied to: "x_stride1028,out_stride1028,d1028" refuses d = 1028 next to a valid call with
both strides 1028, so that `d <= 1024` is the only conjunct that fails.

ENTRIES[entry] also carries what evaluating a conjunct on the host needs: the argument list in header order (`*`: a
pointer, `?`: NULL by default), the defaults of the arguments a case leaves out, and the locals the entry computes before its
checks (`derive`, a restatement of those lines of the source).  evaluate() then tells, without a device, which conjuncts a
set of arguments satisfies - how the host test proves that an at-limit case is a valid call on the boundary and that a
refusal case fails exactly its own row.
"""
import re

KINDS = ("limit", "divisibility", "set", "stride", "alignment", "lds", "pointer", "mode")
BIG = "the smallest instance that reaches the bound needs more than 256 MB of device memory"
PTR, MISALIGNED, BADLIVE = 4096, 4100, -1          # host stand-ins of a pointer argument's state

UNITS = {
    "embed.hip": ["embedding_gather_fwd", "embedding_gather_bwd", "embedding_bag_mean_bwd", "sequence_gather_fwd",
                  "sequence_gather_bwd", "deepfm_sparse_fwd", "deepfm_sparse_bwd", "scatter_rows_sorted"],
    "cross.hip": ["cross_fwd", "cross_bwd", "gather_cross_fwd", "cross_layer_fwd", "cross_layer_bwd"],
    "cin.hip": ["cin_layer_fwd", "cin_layer_bwd"],
    "din.hip": ["din_attention_fwd", "din_attention_bwd", "din_attention_bwd_joined"],
    "fibinet.hip": ["senet_fwd", "senet_bwd", "bilinear_fwd", "bilinear_bwd"],
    "pnn.hip": ["pnn_features_fwd", "pnn_features_bwd", "pnn_weights_fwd", "pnn_weights_bwd"],
    "siblings.hip": ["bi_interaction_fwd", "bi_interaction_bwd", "attention_pool_fwd", "attention_pool_bwd", "ffm_pairs_fwd",
                     "ffm_pairs_bwd"],
}


class Row:
    def __init__(self, text, kind, quantity, at, outside, also, not_driven):
        self.text, self.kind, self.quantity, self.at, self.outside = text, kind, quantity, at, outside
        self.also, self.not_driven = also, not_driven

    def __repr__(self):
        return f"Row({self.text!r})"


def _tags(v):
    return () if v is None else ((v,) if isinstance(v, str) else tuple(v))


_SIMPLE = re.compile(r"^(\w+) (>=|>|<=|<) (-?\d+)$")
_MOD4 = re.compile(r"^(\w+) % 4 == 0$")
_PTR = re.compile(r"^(\w+)(?: != nullptr)?$")


def R(text, kind=None, q=None, at=None, out=None, also=(), nd=None):
    """`NAME op INT`, `NAME % 4 == 0` and `NAME != nullptr` rows fill in their own kind, quantity and tags."""
    m, d, p = _SIMPLE.match(text), _MOD4.match(text), _PTR.match(text)
    if m:
        name, op, n = m.group(1), m.group(2), int(m.group(3))
        on, off = {">=": (n, n - 1), ">": (n + 1, n), "<=": (n, n + 1), "<": (n - 1, n)}[op]
        kind, q = kind or "limit", q or name
        at = f"{name}{on}" if at is None and nd is None else at
        out = f"{name}{off}" if out is None else out
    elif d:
        name = d.group(1)
        kind = kind or ("stride" if name.endswith(("_stride", "_col")) or name.startswith("ld") else "divisibility")
        q, at = q or name, "base" if at is None else at
    elif p and kind in (None, "pointer"):
        kind, q = "pointer", q or p.group(1)
        out = f"null:{q}" if out is None else out
    assert kind in KINDS and q and out is not None, text
    return Row(text, kind, q, _tags(at), _tags(out), tuple(also), nd)


def _args(spec):
    """'ids* arena* B live?' -> [(name, 'int' | 'ptr' | 'opt')]"""
    return [(a.rstrip("*?"), "ptr" if a.endswith("*") else ("opt" if a.endswith("?") else "int")) for a in spec.split()]


ENTRIES = {}


def _entry(name, args, base, rows, defaults=None, derive=""):
    ENTRIES["recalgo_" + name] = dict(args=_args(args), base=base, rows=rows, defaults=defaults or {}, derive=derive)


_TOTAL = "total < (1ll << 31)"
_B0, _B1 = R("B >= 0"), R("B > 0")
_LIVE = R("live_ok(live)", "pointer", "live", out="badlive:live")

# ---- embed.hip ------------------------------------------------------------------------------------------------------------
_entry("embedding_gather_fwd", "ids* arena* row_base* B F K out* out_stride out_col", dict(B=5, F=3, K=4),
       [_B0, R("F > 0"), R("K > 0"), R("out_stride >= out_col + F * K", "stride", "out_stride", at="base", out="out_stride11"),
        R(_TOTAL, "limit", "B", nd=BIG, out="B1<<30")],
       dict(out_stride="out_col + F * K", out_col="0"),
       "vec = vec_of(K, out_stride, out_col); total = B * F * (K // vec)")
_entry("embedding_gather_bwd", "ids* g* row_base* B F K g_stride g_col grad_arena* live?", dict(B=5, F=3, K=4),
       [_B0, R("F > 0"), R("K > 0"), R("K <= 64", at=("K64", "K64,g_col1"), out="g_stride400,K65"),
        R("g_stride >= g_col + F * K", "stride", "g_stride", at="base", out="g_stride11"), _LIVE],
       dict(g_stride="g_col + F * K", g_col="0"))
_entry("embedding_bag_mean_bwd", "values* offsets* g* B K g_stride g_col grad_table* live?", dict(B=5, K=4),
       [_B0, R("K > 0"), R("K <= 64", at=("K64", "K64,g_col1"), out="g_stride400,K65"), R("g_stride >= g_col + K", "stride", "g_stride", at="base", out="g_stride3"),
        _LIVE],
       dict(g_stride="g_col + K", g_col="0"))
_entry("sequence_gather_fwd", "values* offsets* table* B T K out* seq_len*", dict(B=5, T=3, K=4),
       [_B0, R("T > 0"), R("K > 0"), R(_TOTAL, "limit", "B", nd=BIG, out="B1<<30")],
       derive="vec = 4 if K % 4 == 0 else 1; total = B * T * (K // vec)")
_entry("sequence_gather_bwd", "values* offsets* g* B T K grad_table* live?", dict(B=5, T=3, K=4),
       [_B0, R("T > 0"), R("K > 0"), R("K <= 64"), _LIVE, R("BT < (1ll << 31)", "limit", "B", nd=BIG, out="B1<<30")],
       derive="BT = B * T")
_DEEPFM_K = [R("K > 0", at="K4"), R("K % 4 == 0", out="K5"), R("K <= 64", out="K68")]
_entry("deepfm_sparse_fwd", "ids* arena* w1* bias* row_base* B F K emb* fm1* fm2* field_sum*", dict(B=5, F=3, K=4),
       [_B0, R("F > 0"), *_DEEPFM_K, R("field_sum != nullptr"),
        R("smem <= kLdsDefault", "lds", "F", at=("F816", "F62,K64"), out=("F817", "K64,F63"))],
       derive="smem = 4 * (F * K + 16 + F) * 4")
_entry("deepfm_sparse_bwd", "ids* emb* field_sum* g_emb* g_fm1* g_fm2* row_base* B F K grad_arena* grad_w1* live? live_w1?",
       dict(B=5, F=3, K=4),
       [_B0, R("F > 0"), *_DEEPFM_K, _LIVE, R("live_ok(live_w1)", "pointer", "live_w1", out="badlive:live_w1")])
_entry("scatter_rows_sorted", "sorted_rows* perm* vals* M K grad*", dict(M=7, K=3),
       [R("M >= 0", also=("cdiv(total, kThreads) > 0",)), R("K >= 1", also=("cdiv(total, kThreads) > 0",)), R("(M == 0 || (sorted_rows && perm && vals && grad))", "pointer", "vals", out="null:vals"),
        R("cdiv(total, kThreads) > 0", "limit", "M", nd=BIG, out="K1,M549755813633")],
       derive="total = M * K")

# ---- cross.hip ------------------------------------------------------------------------------------------------------------
_STACK = [R("d > 0", at="d4"), R("d % 4 == 0", out="x_stride12,out_stride12,g_stride12,d9"),
          R("d <= 1024", at=("d1024", "d1024,L6"), out="x_stride1028,out_stride1028,g_stride1028,d1028"), R("L >= 1"), R("L <= 6")]


def _strides(a, b):
    return [R(f"{a} % 4 == 0", out=f"{a}9"), R(f"{b} % 4 == 0", out=f"{b}9"),
            R(f"{a} >= d", "stride", a, at="base", out=f"{a}4"), R(f"{b} >= d", "stride", b, at="base", out=f"{b}4")]


_entry("cross_fwd", "x0* x_stride w* b* B d L out* out_stride", dict(B=5, d=8, L=2), [_B0, *_STACK, *_strides("x_stride", "out_stride")],
       dict(x_stride="d", out_stride="d"))
_entry("cross_bwd", "x0* x_stride w* b* g* g_stride g_x0_extra? B d L dx0* dw* db* workspace* defer_reduce", dict(B=5, d=8, L=2),
       [_B1, *_STACK, *_strides("x_stride", "g_stride"), R("workspace != nullptr"),
        R("(defer_reduce || (dw != nullptr && db != nullptr))", "mode", "dw", at=("base", "defer_reduce1,null:dw,null:db"),
          out="null:dw")],
       dict(x_stride="d", g_stride="d", defer_reduce="0"))
_entry("gather_cross_fwd", "ids* arena* row_base* B F K w* b* L x0* x_stride out* out_stride", dict(B=5, F=2, K=4, L=2),
       [_B0, R("F >= 1"), R("K >= 4", out="K0"), R("K % 4 == 0", out="x_stride12,out_stride12,K5"),
        R("d <= 1024", "limit", "F", at=("F256", "F16,K64,L6"), out="x_stride1028,out_stride1028,F257"), R("L >= 1"), R("L <= 6"),
        *[R(f"{p} != nullptr") for p in ("ids", "arena", "row_base", "x0", "out")], *_strides("x_stride", "out_stride"),
        R("aligned16(arena, x0)", "alignment", "x0", at="base", out="mis:x0")],
       dict(x_stride="F * K", out_stride="F * K"), "d = F * K")
_LAYER = [R("d > 0", at="d4"), R("d % 4 == 0", out="x_stride12,out_stride12,g_stride12,d9"),
          R("d <= 2048", out="x_stride2052,out_stride2052,g_stride2052,d2052")]
_entry("cross_layer_fwd", "x0* xl* x_stride w* b* B d out* out_stride", dict(B=5, d=8),
       [R("xl != nullptr"), _B0, *_LAYER, *_strides("x_stride", "out_stride")], dict(x_stride="d", out_stride="d"))
_entry("cross_layer_bwd", "x0* xl* x_stride w* b* g* g_stride B d dx0* dxl* dw* db* workspace*", dict(B=5, d=8),
       [R("xl != nullptr"), R("dxl != nullptr"), R("workspace != nullptr"), _B1, *_LAYER, *_strides("x_stride", "g_stride")],
       dict(x_stride="d", g_stride="d"))

# ---- cin.hip --------------------------------------------------------------------------------------------------------------
_DSET = R("d_ok(D)", "set", "D", at=("D4", "D8", "D16", "D32"), out="D5")
_entry("cin_layer_fwd", "x0* xk* filters* B m Hk N D out* pool* pool_stride pool_col", dict(B=3, m=4, Hk=3, N=5, D=4),
       [_B0, R("m > 0"), R("Hk > 0"), R("N > 0"), R("N <= 128"), _DSET], dict(pool_stride="N", pool_col="0"))
_entry("cin_layer_bwd", "x0* xk* filters* g_out* g_pool* pool_stride pool_col B m Hk N D dx0* dx0_accumulate dxk* dxk_accumulate "
       "dfilters* workspace*", dict(B=3, m=4, Hk=3, N=5, D=4),
       [_B1, R("m >= 4"), R("m <= 128", at=("m128", "m128,Hk128,N128")), R("Hk > 0"), R("Hk <= 128"), R("N > 0"), R("N <= 128"), _DSET,
        R("workspace != nullptr"),
        R("(g_out != nullptr || g_pool != nullptr)", "pointer", "g_pool", at=("null:g_out", "null:g_pool"), out="null:g_out,null:g_pool")],
       dict(pool_stride="N", pool_col="0", dx0_accumulate="0", dxk_accumulate="0"))

# ---- din.hip --------------------------------------------------------------------------------------------------------------
_DIN_W = "f1_w* f1_b* f2_w* f2_b* f3_w* f3_b*"
_DIN = [R("T >= 1"), R("T <= 64", at=("T64", "T64,H8", "T64,H16", "T64,is_softmax0", "T64,H8,is_softmax0", "T64,H16,is_softmax0")),
        R("(H == 4 || H == 8 || H == 16)", "set", "H", at=("H4", "H8", "H16"), out="ldg8,ld_extra8,H5")]
_DIN_G = [R("workspace != nullptr"), R("g_out != nullptr"), R("aligned16(g_out)", "alignment", "g_out", at="base", out="mis:g_out")]
_DIN_D = "dquery* dkeys* d_f1_w* d_f1_b* d_f2_w* d_f2_b* d_f3_w* d_f3_b* workspace*"
_entry("din_attention_fwd", f"query* keys* keys_length* {_DIN_W} B T H is_softmax out*", dict(B=5, T=3, H=4),
       [_B0, *_DIN], dict(is_softmax="1"))
_entry("din_attention_bwd", f"query* keys* keys_length* {_DIN_W} g_out* B T H is_softmax {_DIN_D}", dict(B=5, T=3, H=4),
       [_B1, *_DIN, *_DIN_G], dict(is_softmax="1"))
_entry("din_attention_bwd_joined", f"query* keys* keys_length* {_DIN_W} g_out* ldg dq_extra* ld_extra B T H is_softmax {_DIN_D}",
       dict(B=5, T=3, H=4),
       [_B1, *_DIN, *_DIN_G, R("ldg >= H", "stride", "ldg", at="base", out="ldg0"), R("ldg % 4 == 0", out="ldg9"),
        R("dq_extra == nullptr || ld_extra >= H", "stride", "ld_extra", at=("base", "null:dq_extra,ld_extra0"), out="ld_extra3")],
       dict(is_softmax="1", ldg="H", ld_extra="H"))

# ---- fibinet.hip ----------------------------------------------------------------------------------------------------------
_SENET = [R("F > 0"), R("K > 0", at="K2,reduction_dim1", out="K0", also=("reduction_dim < K",)),
          R("reduction_dim > 0"), R("reduction_dim < K", "limit", "reduction_dim", at="reduction_dim3", out="reduction_dim4")]
_SENET_X = "4 * ((2 * F * K + 3 * F + 2 * reduction_dim + 3) & ~3)"
_entry("senet_fwd", "emb* w1* w2* B F K reduction_dim v_out* a_out*", dict(B=5, F=3, K=4, reduction_dim=2),
       [_B0, *_SENET, R("smem <= kLdsMax", "lds", "F", at=("F1364,K2,reduction_dim1", "F69,K64,reduction_dim32"),
                        out=("K2,reduction_dim1,F1365", "K64,reduction_dim32,F70"))],
       derive=f"smem = ({_SENET_X} + 2 * F * reduction_dim) * 4")
_entry("senet_bwd", "emb* w1* w2* g_v* B F K reduction_dim d_emb* accumulate dw1* dw2* workspace*",
       dict(B=5, F=3, K=4, reduction_dim=2),
       [_B1, *_SENET, R("workspace != nullptr"),
        R("smem <= kLdsMax", "lds", "F", at=("F1077,K2,reduction_dim1", "F48,K64,reduction_dim32"),
          out=("K2,reduction_dim1,F1078", "K64,reduction_dim32,F49"))],
       dict(accumulate="0"), f"WR = F * reduction_dim; smem = ({_SENET_X} + 4 * 2 * WR + 2 * WR) * 4")
_BI = [R("F >= 3"),
       R("F <= 128", at=("F128,K8,type0", "F128,K8,type1", "F128,K8,type2"), out="K8,F129"),
       R("k_ok(K)", "set", "K", at=("K4", "K8", "K16", "K32", "K64"), out="out_stride32,g_stride32,K12"),
       R("type >= kAll", "mode", "type", at="type0", out="type-1"), R("type <= kInteraction", "mode", "type", at="type2", out="type3")]
_BI_PTR = dict(x1="PTR if nv == 2 else 0", w1="PTR if nv == 2 else 0", dx1="PTR if nv == 2 else 0", dw1="PTR if nv == 2 else 0",
               type="0")


# (csrc/fibinet.hip bi_smem / bi_bwd_smem1: the pair table, W of type `all`, then the waves' rows of x and x W)
_BI_LDS = ("nv = 2 if x1 else 1; n = F - 1; P = n * (n - 1) // 2; "
           "smem = ((P * 2 + 15) // 16 * 4 + (nv * K * (K + 4) if type == 0 else 0)")


def _bi_window(s, c):
    return [R(f"{s} % 4 == 0", out=f"{s}9"), R(f"{c} % 4 == 0", out=f"{s}16,{c}1"),
            R(f"{s} >= {c} + nv * K", "stride", s, at="base", out=f"{s}4")]


_entry("bilinear_fwd", "x0* w0* x1* w1* B F K type out* out_stride out_col", dict(B=3, F=4, K=4, nv=2),
       [_B0, *_BI, R("x0"), R("w0"), R("(x1 == nullptr) == (w1 == nullptr)", "pointer", "w1", out="null:w1"),
        *_bi_window("out_stride", "out_col"),
        R("smem <= kLdsMax", "lds", "F", at=("F31,K64,type0", "F40,K64,type1", "F40,K64,type2", "nv1,F69,K64,type0"), out=("K64,type0,F32", "K64,type1,F41", "K64,type2,F41", "nv1,K64,type0,F70"))],
       dict(_BI_PTR, out_stride="out_col + nv * K", out_col="0"), _BI_LDS + " + 4 * nv * (F * K + n * K)) * 4")
_entry("bilinear_bwd", "x0* w0* x1* w1* g* g_stride g_col B F K type dx0* dw0* dx1* dw1* workspace*", dict(B=3, F=4, K=4, nv=2),
       [_B1, *_BI, *[R(p) for p in ("x0", "w0", "dx0", "dw0", "g", "workspace")],
        R("(x1 == nullptr) == (w1 == nullptr)", "pointer", "w1", out="null:w1"),
        R("(x1 == nullptr) == (dx1 == nullptr)", "pointer", "dx1", out="null:dx1"),
        R("(x1 == nullptr) == (dw1 == nullptr)", "pointer", "dw1", out="null:dw1"), *_bi_window("g_stride", "g_col"),
        R("smem <= kLdsMax", "lds", "F", at=("F61,K64,type0", "F77,K64,type1", "F77,K64,type2", "nv1,F127,K64,type0"), out=("K64,type0,F62", "K64,type1,F78", "K64,type2,F78", "nv1,K64,type0,F128"))],
       dict(_BI_PTR, g_stride="g_col + nv * K", g_col="0"), _BI_LDS + " + nv * 2 * (F * K + n * K)) * 4")

# ---- pnn.hip --------------------------------------------------------------------------------------------------------------
_METHOD = R("(method == kIPNN || method == kOPNN)", "set", "method", at=("method0", "method1"), out="method2")


def _features(ld):
    lim = R("(method == kIPNN ? F : K) <= 255", "limit", "F|K", at=("F255", "method1,K255"),
            out=(f"{ld}40000,F256", f"method1,{ld}40000,K256"))
    lds = R("smem <= kLdsMax", "lds", "F|K", at=("F138", "F127,K16", "method1,K140"), out=(f"{ld}40000,F139", f"method1,{ld}40000,K141"))
    return [_B0, R("F > 0"), R("K > 0"), _METHOD, lim if ld == "ld_phi" else lds,
            R(f"{ld} >= recalgo_pnn_feature_count(F, K, method)", "stride", ld, at="base", out=f"{ld}5")]


_entry("pnn_features_fwd", "emb* B F K method phi* ld_phi", dict(B=5, F=3, K=4), _features("ld_phi"),
       dict(method="0", ld_phi="recalgo_pnn_feature_count(F, K, method)"))
_entry("pnn_features_bwd", "emb* dphi* ld_dphi B F K method d_emb* accumulate", dict(B=5, F=3, K=4), _features("ld_dphi"),
       dict(method="0", accumulate="0", ld_dphi="recalgo_pnn_feature_count(F, K, method)"),
       "R = F if method == 0 else K; smem = 4 * ((F * K if method == 0 else 2 * K) + R * (R + 1) // 2) * 4")
_WEIGHTS = [R("D > 0"), R("F > 0"), R("K > 0"), _METHOD]
_entry("pnn_weights_fwd", "product_w* D F K method omega*", dict(D=3, F=3, K=4), _WEIGHTS, dict(method="0"))
_entry("pnn_weights_bwd", "product_w* domega* D F K method d_product_w*", dict(D=3, F=3, K=4), _WEIGHTS, dict(method="0"))

# ---- siblings.hip ---------------------------------------------------------------------------------------------------------
_BI_INT = [_B0, R("F >= 1"), R("K >= 1"), R(_TOTAL, "limit", "B", nd=BIG, out="K2,B1<<30")]
_entry("bi_interaction_fwd", "emb* B F K out*", dict(B=5, F=3, K=4), _BI_INT, derive="total = B * K")
_entry("bi_interaction_bwd", "emb* g* B F K d_emb*", dict(B=5, F=3, K=4), _BI_INT, derive="total = B * K")
_POOL = [_B0, R("P >= 1"), R("K >= 1"), R("K <= 64", at=("K64", "P4096,K64"))]
_entry("attention_pool_fwd", "pairs* att* B P K out* score*", dict(B=5, P=3, K=4), _POOL)
_entry("attention_pool_bwd", "pairs* score* g* B P K d_pairs* d_att*", dict(B=5, P=3, K=4),
       [*_POOL, R("smem <= kLdsDefault", "lds", "P", at=("P4096", "P4096,K64"), out="P4097")], derive="smem = 4 * P * 4")
_entry("ffm_pairs_fwd", "x* B F K out*", dict(B=5, F=3, K=4), [_B0, R("F >= 2"), R("K >= 1")])
_entry("ffm_pairs_bwd", "x* g* B F K dx*", dict(B=5, F=3, K=4),
       [_B0, R("F >= 2"), R("K >= 1"), R(_TOTAL, "limit", "B", nd=BIG, out="B1<<30")], derive="total = B * F * (F - 1) * K")

DOMAIN = {name: {r.text: r for r in e["rows"]} for name, e in ENTRIES.items()}
assert all(len(DOMAIN[n]) == len(e["rows"]) for n, e in ENTRIES.items()), "two rows of one entry share a text"
assert sorted(ENTRIES) == sorted("recalgo_" + n for names in UNITS.values() for n in names)


# ---- tags -----------------------------------------------------------------------------------------------------------------
_ITEM = re.compile(r"^([A-Za-z_]\w*?)(-?\d+(?:<<\d+)?)$")


def parse_tag(tag):
    """'d1024,L6' -> {d: 1024, L: 6};  'null:dw' -> {dw: 0};  'mis:x0' -> {x0: MISALIGNED};  'base' -> {}"""
    out = {}
    for item in tag.split(","):
        if item == "base":
            continue
        if ":" in item:
            how, name = item.split(":")
            out[name] = {"null": 0, "mis": MISALIGNED, "badlive": BADLIVE}[how]
            continue
        m = _ITEM.match(item)
        assert m, f"tag item {item!r}"
        out[m.group(1)] = eval(m.group(2))
    return out


def case_id(entry, tag):
    return f"{entry[len('recalgo_'):]}-{tag}"


def at_dims(entry, tag):
    """the arguments of an at-limit case: base + the tag's items"""
    return {**ENTRIES[entry]["base"], **parse_tag(tag)}


def outside_dims(entry, row, tag):
    """-> (the valid neighbour's arguments, the change): the tag's items that name the row's quantity are the change"""
    items, names = parse_tag(tag), row.quantity.split("|")
    change = {k: v for k, v in items.items() if k in names}
    assert change, f"{entry} {row.text}: the tag {tag!r} does not move {row.quantity}"
    return {**ENTRIES[entry]["base"], **{k: v for k, v in items.items() if k not in names}}, change


# ---- evaluating a conjunct on the host ------------------------------------------------------------------------------------
def _cdiv(a, b):
    v = (a + b - 1) // b & 0xFFFFFFFF                  # (common.h: the quotient is cast to int)
    return v - (1 << 32) if v >= 1 << 31 else v


def _feature_count(F, K, method):
    return F * (F + 1) // 2 if method == 0 and F > 0 else (K * (K + 1) // 2 if method == 1 and K > 0 else 0)


HELPERS = dict(
    PTR=PTR, kIPNN=0, kOPNN=1, kAll=0, kEach=1, kInteraction=2, kLdsDefault=64 * 1024, kLdsMax=160 * 1024, kThreads=256,
    aligned16=lambda *p: all(x % 16 == 0 for x in p), live_ok=lambda l: l != BADLIVE, cdiv=_cdiv,
    k_ok=lambda K: K in (4, 8, 16, 32, 64), d_ok=lambda D: D in (4, 8, 16, 32), recalgo_pnn_feature_count=_feature_count,
    vec_of=lambda K, s, c: 4 if K % 4 == 0 and s % 4 == 0 and c % 4 == 0 else 1)


def c2py(text):
    """a conjunct of the source as a Python expression over the arguments (ints; a pointer is 0 or its address)"""
    t = text.replace("nullptr", "0").replace("1ll", "1").replace("&&", " and ").replace("||", " or ").replace(" / ", " // ")
    t = re.sub(r"!(?!=)", " not ", t)
    return re.sub(r"\(([^()?]+) \? ([^():]+) : ([^()]+)\)", r"(\2 if \1 else \3)", t)


def full(entry, dims, change=None):
    """every argument and derived local of a call: dims, then the defaults, then `change` on top, then `derive`"""
    e = ENTRIES[entry]
    v = dict(dims)
    todo = [n for n in e["defaults"] if n not in v]
    while todo:                                        # (a default may be written in terms of another: out_stride of out_col)
        for name in list(todo):
            try:
                v[name] = eval(e["defaults"][name], dict(HELPERS), v)
                todo.remove(name)
            except NameError:
                assert len(todo) > 1, f"{entry}: the default of {name}"
        v.pop("__builtins__", None)
    for name, how in e["args"]:
        if name not in v:
            assert how != "int", f"{entry}: no value for {name}"
            v[name] = PTR if how == "ptr" else 0
    v.update(change or {})
    exec(e["derive"], dict(HELPERS), v)
    v.pop("__builtins__", None)
    return v


def evaluate(entry, dims, change=None, rows=None):
    """{conjunct: holds?} of a call"""
    v = full(entry, dims, change)
    return {text: bool(eval(c2py(text), dict(HELPERS), v)) for text in (rows if rows is not None else DOMAIN[entry])}


# ---- cutting the conjuncts out of the source ------------------------------------------------------------------------------
def split_conjuncts(expr):
    """the top-level `&&` conjuncts of a C expression, whitespace-normalised"""
    parts, depth, cur, i = [], 0, "", 0
    while i < len(expr):
        c = expr[i]
        depth += c == "("
        depth -= c == ")"
        if depth == 0 and expr.startswith("&&", i):
            parts.append(cur)
            cur, i = "", i + 2
            continue
        cur += c
        i += 1
    return [" ".join(p.split()) for p in parts + [cur]]


def _paren(src, at):
    """src[at] == '(' -> the text between it and its match"""
    depth, i = 0, at
    while True:
        depth += src[i] == "("
        depth -= src[i] == ")"
        if depth == 0:
            return src[at + 1:i]
        i += 1


def _definition(src, entry):
    """-> (parameter names, body) of `RECALGO_EXPORT .. entry(..) { .. }`"""
    m = re.search(r"RECALGO_EXPORT\s+[\w\s]+?\b%s\s*\(" % re.escape(entry), src)
    assert m, f"{entry} is not defined"
    params = _paren(src, m.end() - 1)
    names = [re.search(r"(\w+)\s*$", p).group(1) for p in params.split(",")]
    start = src.index("{", m.end() + len(params))
    depth, i = 0, start
    while True:
        depth += src[i] == "{"
        depth -= src[i] == "}"
        if depth == 0:
            return names, src[start + 1:i]
        i += 1


def source_conjuncts(src, entry):
    """The conjuncts of `entry`'s RECALGO_REQUIRE lines.  An entry whose body only forwards to another entry of the same unit
    (recalgo_embedding_gather_fwd -> .._fwd_deferred) has the callee's conjuncts, less those over a parameter the forwarding
    entry does not have: it pins that parameter to a constant, so the conjunct is no part of ITS domain."""
    names, body = _definition(src, entry)
    found = [c for m in re.finditer(r"RECALGO_REQUIRE\s*\(", body) for c in split_conjuncts(_paren(body, m.end() - 1))]
    fwd = re.match(r"\s*return\s+(recalgo_\w+)\s*\(", body)
    if found or not fwd:
        return found
    callee_names, _ = _definition(src, fwd.group(1))
    pinned = set(callee_names) - set(names)
    return [c for c in source_conjuncts(src, fwd.group(1)) if not pinned & set(re.findall(r"[A-Za-z_]\w*", c))]
