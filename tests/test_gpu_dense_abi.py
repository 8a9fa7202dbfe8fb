"""-m gpu: the dense backward's work partition, the crossed options of the dense ABI, the gaps of strided outputs and the
step's deferred-sum launch, driven at the C ABI (include/recalgo.h) with the test's own leading dimensions, base alignments
and workspaces, against tests/dense_ref.py (float64, and float32 as the `ref32` of tests/util.assert_close).

Every output, gradient, partial-row and workspace buffer is 0xFF bytes (NaN) before the launch, a workspace is exactly as
large as its query says, and a matrix whose leading dimension exceeds its width (or whose base is shifted) carries a
recognisable pattern in the floats around its elements, which must be there bit for bit afterwards.

a. PARTITION: the classes of bwd_balance(M, K, N) (csrc/dense.hip: consecutive input-gradient tiles per workgroup, batch
   splits of the weight gradient, rows per split rounded up to 32), smallest shape found per class, evaluated at 8c0c31a:

   | shape (M, K, N)    | tiles/workgroup (tiles, ragged) | splits x rows  | empty splits | arm                                   |
   |--------------------|---------------------------------|----------------|--------------|---------------------------------------|
   | (100, 8, 8)        | 1                               | 1              | 0            | single split: no workspace            |
   | (1025, 256, 512)   | 1                               | 8 x 160        | 1            | float4 arms                           |
   | (2049, 8, 8)       | 1                               | 16 x 160       | 3            | the `% 8 == 0` split placement        |
   | (2049, 8, 50)      | 1                               | 16 x 160       | 3            | element-wise arm (N % 4 != 0)         |
   | (129, 8, 8)        | 1                               | 2 x 96         | 0            | last split 33 rows                    |
   | (257, 8, 8)        | 1                               | 3 x 96         | 0            | last split 65 rows                    |
   | (385 + 128 i, 8, 8), i = 0..12 | 1                   | (4 + i) x 128  | 0            | last split ONE row (.. (1921, 8, 8): 16) |
   | (16385, 8, 8)      | 2 (257, last workgroup 1)       | 128 x 160      | 25           | ragged last workgroup                 |
   | (27286, 8, 8)      | 3 (427, last 1)                 | 208 x 160      | 37           |                                       |
   | (38247, 8, 8)      | 4 (598, last 2)                 | 296 x 160      | 56           |                                       |
   | (49208, 8, 8)      | 5 (769, last 4)                 | 336 x 160      | 28           |                                       |
   | (60072, 8, 8)      | 6 (939, last 3)                 | 336 x 192      | 23           |                                       |
   | (35531, 82, 8)     | 7 (1112, last 6)                | 168 x 224      | 9            | K % 4 != 0: element-wise dx           |
   | (40963, 82, 8)     | 8 (1282, last 2)                | 168 x 256      | 7            | K % 4 != 0: element-wise dx           |
   | (41157, 84, 8)     | 8 (1288, whole)                 | 168 x 256      | 7            | float4 arms                           |
   | (65536, 82, 256)   | 8 (2048, whole)                 | 32 x 2048      | 0            | u = 64.0 exactly, the cap not taken: 512 workgroups, one resident round |
   | (27286, 256, 512)  | 4 (1708, whole)                 | 13 x 2112      | 0            | u = 106.7 > 64, capped: 843 workgroups, a second round |

   The tests do not restate the heuristic: whatever it becomes, each shape is checked against the reference and against
   the two separate launches.  The one fact asserted about it is that the workspace query is 0 exactly for the single-split
   shapes.  When the heuristic moves, re-derive the table and re-pick the smallest shape of each class.
b. OPTIONS: two literal tables (backward, forward) in which every pair of values of any two axes appears in a row
   (tests/test_dense_ref_host.py checks that), pruned only by the header's REQUIREs, plus BatchNorm-sum rows at empty-split shapes.
c. A derandomised Hypothesis sweep of shapes and options, which keeps visiting the partition when the heuristic changes.
d. recalgo_dense_bwd_weights_reduce on its own: chunks of 32 jobs, column-sum jobs, single-split jobs, the three arms.
e. recalgo_dense_bwd_rider with a weight-gradient rider.
f. a, b, d, e once more under tests/redzone.guarded()."""
import ctypes

import pytest
import torch
from hypothesis import HealthCheck, given, settings
from hypothesis import strategies as st

from recalgorithm_amd import _lib
from tests import dense_ref as R
from tests.redzone import guarded
from tests.util import assert_bit_exact, assert_close

pytestmark = pytest.mark.gpu

_Split, _ColSum = _lib.STRUCTS["recalgo_dense_split_t"], _lib.STRUCTS["recalgo_colsum_t"]
ACT_NONE = _lib.CONSTANTS["RECALGO_ACT_NONE"]
ACT = {"none": None, "prelu": R.PRELU, "dice": R.DICE}
assert (_lib.CONSTANTS["RECALGO_ACT_PRELU"], _lib.CONSTANTS["RECALGO_ACT_DICE"]) == (R.PRELU, R.DICE)
STRICT_MAX = 4096            # the longest contraction for which the float32 reference arms the strict guard

PARTITION_SHAPES = [(100, 8, 8), (1025, 256, 512), (2049, 8, 8), (2049, 8, 50)] + [(129 + 128 * i, 8, 8) for i in range(15)] + \
    [(16385, 8, 8), (27286, 8, 8), (38247, 8, 8), (49208, 8, 8), (60072, 8, 8), (35531, 82, 8), (40963, 82, 8), (41157, 84, 8),
     (65536, 82, 256), (27286, 256, 512)]
PARTITION_BN_SHAPES = [(1025, 256, 512), (2049, 8, 50), (27286, 8, 8), (40963, 82, 8), (41157, 84, 8)]
SINGLE_SPLIT = {(100, 8, 8), (65, 84, 50)}

_OPTION_SHAPES = ((300, 100, 52), (65, 84, 50), (1025, 128, 36), (130, 33, 68))
BWD_AXES = {"y_mask": (0, 1), "c_in": ("off", "one", "quarter_ld"), "relu_mask": ("off", "tight", "ld", "unaligned"), "bn": (0, 1),
            "dbias": (0, 1), "defer": (0, 1), "ld": ("tight", "pad4", "pad1"), "align": (16, 4), "shape": _OPTION_SHAPES}
BWD_ROWS = [
    (1, "one", "unaligned", 0, 1, 0, "pad4", 16, (65, 84, 50)),
    (1, "off", "tight", 1, 0, 1, "pad1", 4, (1025, 128, 36)),
    (0, "quarter_ld", "ld", 1, 0, 0, "tight", 16, (130, 33, 68)),
    (0, "one", "off", 1, 1, 1, "pad4", 4, (300, 100, 52)),
    (1, "quarter_ld", "unaligned", 0, 0, 1, "tight", 4, (300, 100, 52)),
    (0, "off", "tight", 0, 1, 0, "pad1", 16, (65, 84, 50)),
    (0, "quarter_ld", "ld", 0, 1, 1, "pad4", 16, (1025, 128, 36)),
    (1, "off", "off", 0, 1, 0, "pad4", 4, (130, 33, 68)),
    (1, "one", "ld", 1, 0, 0, "tight", 4, (65, 84, 50)),
    (1, "quarter_ld", "off", 0, 0, 1, "pad1", 16, (65, 84, 50)),
    (0, "off", "unaligned", 1, 1, 1, "tight", 16, (1025, 128, 36)),
    (1, "one", "tight", 1, 0, 1, "pad4", 16, (130, 33, 68)),
    (0, "off", "ld", 0, 1, 0, "pad1", 4, (300, 100, 52)),
    (1, "one", "unaligned", 0, 1, 1, "pad1", 16, (130, 33, 68)),
    (1, "one", "off", 0, 0, 0, "tight", 16, (1025, 128, 36)),
    (1, "quarter_ld", "tight", 0, 0, 1, "tight", 16, (300, 100, 52)),
    # the float4 arms with everything on, and the BatchNorm sums beside the strided / shifted operands
    (1, "quarter_ld", "ld", 1, 1, 1, "pad4", 16, (300, 100, 52)),
    (0, "one", "unaligned", 1, 1, 0, "pad1", 4, (65, 84, 50)),
    (1, "off", "off", 1, 1, 1, "pad4", 16, (1025, 128, 36)),
]
# BatchNorm sums where the weight gradient has empty trailing splits (none of the four option shapes has one at 8c0c31a)
BWD_EMPTY_SPLIT_ROWS = [
    (1, "quarter_ld", "ld", 1, 1, 1, "pad4", 16, (2049, 8, 50)),
    (0, "one", "tight", 1, 1, 0, "pad1", 4, (2049, 8, 8)),
    (1, "off", "unaligned", 1, 0, 1, "tight", 16, (1025, 256, 512)),
]
FWD_AXES = {"pair2": (0, 1), "bias": (0, 1), "relu": (0, 1), "act": ("none", "prelu", "dice"), "bn": (0, 1), "ldy": ("tight", "pad4"),
            "ldx": ("tight", "pad4", "pad1"), "align": (16, 4), "shape": _OPTION_SHAPES}
FWD_ROWS = [
    (0, 1, 1, "none", 0, "pad4", "pad1", 16, (130, 33, 68)),
    (1, 1, 0, "prelu", 1, "tight", "pad4", 4, (300, 100, 52)),
    (1, 0, 0, "dice", 1, "pad4", "tight", 16, (65, 84, 50)),
    (0, 0, 1, "none", 0, "tight", "tight", 4, (300, 100, 52)),
    (0, 1, 0, "dice", 1, "tight", "pad1", 4, (1025, 128, 36)),
    (1, 0, 1, "none", 0, "pad4", "pad4", 4, (1025, 128, 36)),
    (1, 0, 0, "prelu", 1, "tight", "pad4", 16, (130, 33, 68)),
    (0, 1, 1, "none", 1, "tight", "pad1", 4, (65, 84, 50)),
    (1, 0, 0, "prelu", 1, "pad4", "pad1", 16, (300, 100, 52)),
    (1, 1, 0, "prelu", 1, "tight", "tight", 16, (1025, 128, 36)),
    (0, 0, 0, "none", 0, "pad4", "pad4", 16, (65, 84, 50)),
    (0, 0, 0, "dice", 1, "tight", "tight", 4, (130, 33, 68)),
    (0, 1, 0, "prelu", 1, "tight", "tight", 16, (65, 84, 50)),
    (1, 0, 0, "dice", 1, "tight", "pad4", 4, (300, 100, 52)),
    # the float4 store with everything on; the BatchNorm moments of a ReLU output in a padded y
    (1, 1, 0, "dice", 1, "pad4", "pad4", 16, (1025, 128, 36)),
    (1, 1, 1, "none", 1, "pad4", "tight", 16, (300, 100, 52)),
    (0, 1, 1, "none", 1, "pad4", "pad4", 16, (1025, 128, 36)),
]


def bwd_row_valid(r):
    # the (K % 4, N % 4) axis is the "shape" axis: (300, 100, 52) and (1025, 128, 36) have both 0, (130, 33, 68) K odd,
    # (65, 84, 50) N not a multiple of 4.  No REQUIRE prunes a row: ldc >= K, ld_mask >= K and the three bn_* pointers with
    # bn_partials hold in every one.
    return True


def fwd_row_valid(r):
    return r["act"] == "none" or (r["bn"] == 1 and r["relu"] == 0)          # act_kind needs bn_partials and relu == 0


# ---- plumbing -------------------------------------------------------------------------------------------------------------------
def L():
    return _lib.load()               # (looked up per call: under redzone.guarded() it is the recording proxy)


def _stream():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def P(t):
    return None if t is None else ctypes.c_void_p(t.data_ptr())


def _nan(n, dev):
    """n floats of 0xFF bytes in a device allocation of exactly 4 n bytes."""
    return torch.full((4 * n,), 0xFF, dtype=torch.uint8, device=dev).view(torch.float32)


def _workspace(shape, dev):
    nbytes = int(L().recalgo_dense_bwd_weights_workspace_bytes(*shape))
    assert nbytes >= 0 and nbytes % 4 == 0
    return None if nbytes == 0 else _nan(nbytes // 4, dev)


class Mat:
    """[rows, cols] fp32 on the device with leading dimension `ld`, its first element `shift` floats behind a 16-byte aligned
    base.  value None: an output (0xFF bytes).  Every float of the allocation that is no element holds a pattern."""

    def __init__(self, dev, rows, cols, ld=None, shift=0, value=None):
        ld = ld or cols
        assert ld >= cols
        self.rows, self.cols, self.ld, self.shift = rows, cols, ld, shift
        self.gap = ld > cols or shift > 0
        n = shift + rows * ld
        if self.gap:
            host = -7777.0 - (torch.arange(n) % 97).float()
            body = host[shift:].view(rows, ld)[:, :cols]
            if value is None:
                body.view(torch.int32).fill_(-1)
            else:
                body.copy_(value)
        else:
            host = torch.full((n,), -1, dtype=torch.int32).view(torch.float32) if value is None else value.contiguous().view(-1)
        self.host, self.is_output = host, value is None
        self.buf = host.to(dev)
        self.v = self.buf[shift:].view(rows, ld)[:, :cols]
        assert self.v.data_ptr() % 16 == (4 * shift) % 16

    @property
    def ptr(self):
        return ctypes.c_void_p(self.v.data_ptr())

    def get(self):
        return self.v.cpu().contiguous()

    def check(self, what):
        """The floats around the elements are untouched; an input is unchanged altogether."""
        if not self.gap:
            return
        got = self.buf.cpu()
        if self.is_output:
            keep = torch.ones(got.numel(), dtype=torch.bool)
            keep[self.shift:].view(self.rows, self.ld)[:, :self.cols] = False
            assert_bit_exact(got[keep], self.host[keep], f"{what}: the floats between width and leading dimension")
        else:
            assert_bit_exact(got, self.host, f"{what}: an input")


class Inputs:
    """The operands of one (M, K, N), drawn on first use (randn, w / sqrt(K), masks = ReLU outputs: about half exactly 0), and the
    references computed from them: each once, shared, left unchanged."""
    NAMES = ("x", "g", "w", "y_mask", "c", "rm", "bn_x", "bias", "x2", "w2", "alpha")

    def __init__(self, shape, seed=0):
        self.shape, self.seed, self.t, self.refs = tuple(shape), seed, {}, {}
        K = shape[1]
        self.K2 = 48 if K % 4 == 0 else 21

    def __getitem__(self, name):
        if name not in self.t:
            M, K, N = self.shape
            gen = torch.Generator().manual_seed(((M * 1009 + K) * 1013 + N) * 31 + self.NAMES.index(name) + 977 * self.seed)
            r = lambda *s: torch.randn(*s, generator=gen)
            K2 = self.K2
            make = {"x": lambda: r(M, K), "g": lambda: r(M, N), "w": lambda: r(K, N) / K ** 0.5, "y_mask": lambda: torch.relu(r(M, N)),
                    "c": lambda: r(M, K), "rm": lambda: torch.relu(r(M, K)), "bn_x": lambda: r(M, K), "bias": lambda: r(N) * 0.1,
                    "x2": lambda: r(M, K2), "w2": lambda: r(K2, N) / K2 ** 0.5,
                    "alpha": lambda: torch.rand(N, generator=gen) * 0.5 + 0.1}
            self.t[name] = make[name]()
        return self.t[name]

    def bn_stats(self):
        if "bn_mean" not in self.t:
            bx = self["bn_x"]
            self.t["bn_mean"] = bx.mean(0)
            self.t["bn_rstd"] = 1.0 / (bx.var(0, unbiased=False) + 1e-3).sqrt()
        return self.t["bn_mean"], self.t["bn_rstd"]

    def ref_bwd(self, y_mask, c_in, relu_mask, bn):
        key = ("bwd", bool(y_mask), c_in, relu_mask != "off", bool(bn))
        if key not in self.refs:
            mean, rstd = self.bn_stats() if bn else (None, None)
            kw = dict(c_in=None if c_in == "off" else self["c"], beta=1.0 if c_in == "one" else 0.25,
                      dx_relu_mask=None if relu_mask == "off" else self["rm"], bn_x=self["bn_x"] if bn else None, bn_mean=mean,
                      bn_rstd=rstd)
            a = (self["x"], self["g"], self["y_mask"] if y_mask else None, self["w"])
            self.refs[key] = (R.bwd(*a, **kw), R.bwd(*a, dtype=torch.float32, **kw))
        return self.refs[key]

    def ref_fwd(self, pair2, bias, relu, act):
        key = ("fwd", bool(pair2), bool(bias), bool(relu), act)
        if key not in self.refs:
            a = (self["x"], self["w"], self["x2"] if pair2 else None, self["w2"] if pair2 else None, self["bias"] if bias else None,
                 bool(relu), ACT[act], self["alpha"] if act != "none" else None)
            self.refs[key] = (R.fwd(*a), R.fwd(*a, dtype=torch.float32))
        return self.refs[key]


_CASES = {}


def _inputs(shape):
    if shape not in _CASES:
        _CASES[shape] = Inputs(shape)
    return _CASES[shape]


# ---- the backward ---------------------------------------------------------------------------------------------------------------
def _launch_bwd(dev, inp, *, y_mask=0, c_in="off", relu_mask="off", bn=0, dbias=0, defer=0, ld="tight", align=16, entry="bwd",
                what=""):
    """One backward through `entry` ("bwd": recalgo_dense_bwd; "separate": recalgo_dense_bwd_input + recalgo_dense_bwd_weights, which
    have no relu_mask / bn) -> host copies of dx, dw, dbias, bn_partials."""
    M, K, N = inp.shape
    lib = L()
    pad, shift = {"tight": 0, "pad4": 4, "pad1": 1}[ld], 0 if align == 16 else 1
    x = Mat(dev, M, K, K + pad, shift, inp["x"])
    g = Mat(dev, M, N, N + pad, shift, inp["g"])
    ym = Mat(dev, M, N, N + pad, shift, inp["y_mask"]) if y_mask else None          # (the layout of g)
    w = inp["w"].to(dev)
    c = None if c_in == "off" else Mat(dev, M, K, K + (4 if c_in == "quarter_ld" else 0), 0, inp["c"])
    beta = 0.0 if c is None else (1.0 if c_in == "one" else 0.25)
    rm = None
    if relu_mask != "off":
        rm = Mat(dev, M, K, K + (4 if relu_mask == "ld" else 0), 1 if relu_mask == "unaligned" else 0, inp["rm"])
    dx = Mat(dev, M, K, K + pad, 0)
    dw, db = _nan(K * N, dev).view(K, N), _nan(N, dev) if dbias else None
    ws = _workspace(inp.shape, dev)
    bnx = mean = rstd = part = None
    if bn:
        bnx, (mean, rstd) = inp["bn_x"].to(dev), (t.to(dev) for t in inp.bn_stats())
        part = _nan(R.partial_rows(M) * 2 * K, dev).view(-1, 2 * K)
    if entry == "bwd":
        lib.recalgo_dense_bwd(x.ptr, x.ld, g.ptr, g.ld, ym and ym.ptr, P(w), M, K, N, c and c.ptr, c.ld if c else 0, beta, dx.ptr,
                              dx.ld, P(dw), P(db), P(ws), defer, P(bnx), P(mean), P(rstd), P(part), rm and rm.ptr,
                              rm.ld if rm else 0, _stream())
    else:
        assert rm is None and not bn
        lib.recalgo_dense_bwd_input(g.ptr, g.ld, ym and ym.ptr, P(w), M, N, K, c and c.ptr, c.ld if c else 0, beta, dx.ptr, dx.ld, 0,
                                    _stream())
        lib.recalgo_dense_bwd_weights(x.ptr, x.ld, g.ptr, g.ld, ym and ym.ptr, M, K, N, P(dw), P(db), P(ws), defer, _stream())
    if defer:
        jobs = (_Split * 1)(_Split(M, K, N, 0 if ws is None else ws.data_ptr(), dw.data_ptr(), 0 if db is None else db.data_ptr()))
        assert lib.recalgo_dense_bwd_weights_reduce(jobs, 1, None, 0, None, _stream()) == 0
    out = {"dx": dx.get(), "dw": dw.cpu(), "dbias": None if db is None else db.cpu(), "part": None if part is None else part.cpu()}
    for m, name in ((x, "x"), (g, "g"), (ym, "y_mask"), (c, "c_in"), (rm, "dx_relu_mask"), (dx, "dx")):
        if m is not None:
            m.check(f"{what} {name}")
    return out


def _check_bwd(out, inp, what, *, y_mask=0, c_in="off", relu_mask="off", bn=0, **_):
    M, K, N = inp.shape
    (dx, dw, db, part), (dx32, dw32, db32, part32) = inp.ref_bwd(y_mask, c_in, relu_mask, bn)
    over_n = lambda t: t if N <= STRICT_MAX else None
    over_m = lambda t: t if M <= STRICT_MAX else None
    assert_close(out["dx"], dx, what=f"{what} dx", reduced=True, ref32=over_n(dx32))
    assert_close(out["dw"], dw, what=f"{what} dw", reduced=True, ref32=over_m(dw32))
    if out["dbias"] is not None:
        assert_close(out["dbias"], db, what=f"{what} dbias", reduced=True, ref32=over_m(db32))
    if bn:
        assert_close(out["part"][:, :K], part[:, :K], what=f"{what} tile colsum(dx)", reduced=True, ref32=over_n(part32[:, :K]))
        assert_close(out["part"][:, K:], part[:, K:], what=f"{what} tile colsum(dx * xhat)", reduced=True, ref32=over_n(part32[:, K:]))
    else:
        assert out["part"] is None


def _same(a, b, what, names=("dx", "dw", "dbias")):
    for n in names:
        if a[n] is not None or b[n] is not None:
            assert_bit_exact(a[n], b[n], f"{what}: {n}")


def _bwd_case(dev, shape, what, inp=None, **opt):
    """recalgo_dense_bwd with `opt` against the reference; dw / dbias, and dx as far as the separate launches can state it, bit for
    bit against recalgo_dense_bwd_input + recalgo_dense_bwd_weights on the same operands."""
    inp = inp or _inputs(shape)
    out = _launch_bwd(dev, inp, what=what, **opt)
    _check_bwd(out, inp, what, **opt)
    sep = _launch_bwd(dev, inp, what=what + " (separate launches)", entry="separate",
                      **{**opt, "relu_mask": "off", "bn": 0, "defer": 0})
    if opt.get("relu_mask", "off") == "off":
        _same(out, sep, what + " merged vs separate launches")
    else:
        _same(out, sep, what + " merged vs separate launches", names=("dw", "dbias"))
        if opt.get("c_in", "off") == "off":            # (with c_in the mask comes before the fused multiply-add: not a host expression)
            assert_bit_exact(out["dx"], torch.where(inp["rm"] > 0, sep["dx"], torch.zeros(())), what + " dx = masked separate dx")
    return out


def _partition_case(dev, shape, variant):
    nbytes = int(L().recalgo_dense_bwd_weights_workspace_bytes(*shape))
    assert (nbytes == 0) == (shape in SINGLE_SPLIT), f"{shape}: workspace query {nbytes}"
    what = f"partition {shape} {variant}"
    if variant == "mask+dbias":
        _bwd_case(dev, shape, what, y_mask=1, dbias=1, defer=0)
    elif variant == "plain":
        _bwd_case(dev, shape, what, y_mask=0, dbias=0, defer=1)
    else:
        _bwd_case(dev, shape, what, y_mask=1, dbias=1, defer=1, bn=1, relu_mask="tight")


@pytest.mark.parametrize("variant", ["mask+dbias", "plain"])
@pytest.mark.parametrize("shape", PARTITION_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_bwd_partition_classes(dev, shape, variant):
    _partition_case(dev, shape, variant)


@pytest.mark.parametrize("shape", PARTITION_BN_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_bwd_partition_classes_with_batchnorm_sums_and_relu_mask(dev, shape):
    _partition_case(dev, shape, "bn+relu_mask")


def _bwd_row(dev, row, tag="options"):
    opt = dict(zip(BWD_AXES, row))
    shape = opt.pop("shape")
    nbytes = int(L().recalgo_dense_bwd_weights_workspace_bytes(*shape))
    assert (nbytes == 0) == (shape in SINGLE_SPLIT), f"{shape}: workspace query {nbytes}"
    _bwd_case(dev, shape, f"bwd {tag} {row}", **opt)


@pytest.mark.parametrize("row", BWD_ROWS + BWD_EMPTY_SPLIT_ROWS, ids=lambda r: "-".join(str(v) for v in r[:-1]) + "-" + "x".join(map(str, r[-1])))
def test_bwd_options_crossed(dev, row):
    _bwd_row(dev, row)


# ---- the forward ----------------------------------------------------------------------------------------------------------------
def _fwd_case(dev, shape, what, inp=None, *, pair2=0, bias=0, relu=0, act="none", bn=0, ldy="tight", ldx="tight", align=16):
    inp = inp or _inputs(shape)
    M, K, N = inp.shape
    K2 = inp.K2
    pad, shift, ypad = {"tight": 0, "pad4": 4, "pad1": 1}[ldx], 0 if align == 16 else 1, 4 if ldy == "pad4" else 0
    x = Mat(dev, M, K, K + pad, shift, inp["x"])
    x2 = Mat(dev, M, K2, K2 + pad, shift, inp["x2"]) if pair2 else None
    w, w2 = inp["w"].to(dev), inp["w2"].to(dev) if pair2 else None
    b = inp["bias"].to(dev) if bias else None
    alpha = inp["alpha"].to(dev) if act != "none" else None
    y = Mat(dev, M, N, N + ypad, 0)
    z = Mat(dev, M, N, N + ypad, 0) if act != "none" else None
    part = _nan(R.partial_rows(M) * 2 * N, dev).view(-1, 2 * N) if bn else None
    L().recalgo_dense_fwd(x.ptr, x.ld, P(w), K, x2 and x2.ptr, x2.ld if x2 else 0, P(w2), K2 if pair2 else 0, P(b), M, N, relu,
                          ACT_NONE if act == "none" else ACT[act], P(alpha), z and z.ptr, y.ptr, y.ld, P(part), None, _stream())
    (rz, ry, rp), (rz32, ry32, rp32) = inp.ref_fwd(pair2, bias, relu, act)
    strict = K + (K2 if pair2 else 0) <= STRICT_MAX
    pick = lambda t: t if strict else None
    assert_close(y.get(), ry, what=f"{what} y", reduced=True, ref32=pick(ry32))
    if z is not None:
        assert_close(z.get(), rz, what=f"{what} z", reduced=True, ref32=pick(rz32))
    if bn:
        got = part.cpu()
        assert_close(got[:, :N], rp[:, :N], what=f"{what} tile means", reduced=True, ref32=pick(rp32[:, :N]))
        assert_close(got[:, N:], rp[:, N:], what=f"{what} tile M2", reduced=True, ref32=pick(rp32[:, N:]))
    for m, name in ((x, "x"), (x2, "x2"), (y, "y"), (z, "z")):
        if m is not None:
            m.check(f"{what} {name}")


def _fwd_row(dev, row):
    opt = dict(zip(FWD_AXES, row))
    _fwd_case(dev, opt.pop("shape"), f"fwd options {row}", **opt)


@pytest.mark.parametrize("row", FWD_ROWS, ids=lambda r: "-".join(str(v) for v in r[:-1]) + "-" + "x".join(map(str, r[-1])))
def test_fwd_options_crossed(dev, row):
    _fwd_row(dev, row)


# ---- c. the sweep ---------------------------------------------------------------------------------------------------------------
SWEEP = settings(max_examples=25, deadline=None, derandomize=True, suppress_health_check=list(HealthCheck))
_dim = st.integers(1, 300)


@SWEEP
@given(M=st.integers(1, 3000), K=_dim, N=_dim, y_mask=st.sampled_from(BWD_AXES["y_mask"]), c_in=st.sampled_from(BWD_AXES["c_in"]),
       relu_mask=st.sampled_from(BWD_AXES["relu_mask"]), bn=st.sampled_from(BWD_AXES["bn"]), dbias=st.sampled_from(BWD_AXES["dbias"]),
       defer=st.sampled_from(BWD_AXES["defer"]), ld=st.sampled_from(BWD_AXES["ld"]), align=st.sampled_from(BWD_AXES["align"]))
def test_bwd_any_shape_any_options(dev, M, K, N, y_mask, c_in, relu_mask, bn, dbias, defer, ld, align):
    opt = dict(y_mask=y_mask, c_in=c_in, relu_mask=relu_mask, bn=bn, dbias=dbias, defer=defer, ld=ld, align=align)
    _bwd_case(dev, (M, K, N), f"bwd sweep {(M, K, N)} {opt}", inp=Inputs((M, K, N)), **opt)


@SWEEP
@given(M=st.integers(1, 3000), K=_dim, N=_dim, pair2=st.sampled_from((0, 1)), bias=st.sampled_from((0, 1)), relu=st.sampled_from((0, 1)),
       act=st.sampled_from(FWD_AXES["act"]), bn=st.sampled_from((0, 1)), ldy=st.sampled_from(FWD_AXES["ldy"]),
       ldx=st.sampled_from(FWD_AXES["ldx"]), align=st.sampled_from(FWD_AXES["align"]))
def test_fwd_any_shape_any_options(dev, M, K, N, pair2, bias, relu, act, bn, ldy, ldx, align):
    opt = dict(pair2=pair2, bias=bias, relu=relu, act=act, bn=bn, ldy=ldy, ldx=ldx, align=align)
    if opt["act"] != "none":
        opt["bn"], opt["relu"] = 1, 0                   # (the header's REQUIRE for act_kind)
    _fwd_case(dev, (M, K, N), f"fwd sweep {(M, K, N)} {opt}", inp=Inputs((M, K, N)), **opt)


# ---- d. recalgo_dense_bwd_weights_reduce ------------------------------------------------------------------------------------------
# split counts of table a (2, 3, 5, 8 and 9 splits, 16 with three empty, the element-wise arm, the float4 arm with an empty split)
REDUCE_POOL = [(129, 8, 8), (257, 8, 8), (513, 8, 8), (897, 8, 8), (1025, 128, 36), (2049, 8, 8), (2049, 8, 50), (1025, 256, 512)]
REDUCE_SINGLE = (100, 8, 8)
COLSUM_ROWS = (1, 15, 16, 17, 112, 113, 127, 128, 129, 512, 513)
COLSUM_N = (1, 15, 16, 17, 1000)
STEP0 = 41


def _wgrad(dev, inp, with_dbias, defer, dw_shift=0, db_shift=0):
    """recalgo_dense_bwd_weights on the operands of `inp` (masked when it has a dbias) into 0xFF buffers with a workspace of its own
    -> (dw, dbias, workspace, the job that finishes it)."""
    M, K, N = inp.shape
    x, g = inp["x"].to(dev), inp["g"].to(dev)
    ym = inp["y_mask"].to(dev) if with_dbias else None
    dw = _nan(K * N + dw_shift, dev)[dw_shift:].view(K, N)
    db = _nan(N + db_shift, dev)[db_shift:] if with_dbias else None
    ws = _workspace(inp.shape, dev)
    L().recalgo_dense_bwd_weights(P(x), K, P(g), N, P(ym), M, K, N, P(dw), P(db), P(ws), defer, _stream())
    return dw, db, ws, _Split(M, K, N, 0 if ws is None else ws.data_ptr(), dw.data_ptr(), 0 if db is None else db.data_ptr())


def _check_wgrad(dw, db, inp, what):
    M = inp.shape[0]
    (_, rw, rb, _), (_, rw32, rb32, _) = inp.ref_bwd(db is not None, "off", "off", 0)
    assert_close(dw, rw, what=f"{what} dw", reduced=True, ref32=rw32 if M <= STRICT_MAX else None)
    if db is not None:
        assert_close(db, rb, what=f"{what} dbias", reduced=True, ref32=rb32 if M <= STRICT_MAX else None)


def _colsum_job(dev, rows, n, stride, seed):
    part = torch.randn((rows - 1) * stride + n, generator=torch.Generator().manual_seed(seed * 7919 + rows * 31 + n))
    dpart, out = part.to(dev), _nan(n, dev)
    return part, dpart, out, _ColSum(dpart.data_ptr(), out.data_ptr(), rows, stride, n)


def _reduce_case(dev, n_sums, n_jobs, what, sum_shapes=None):
    """ONE recalgo_dense_bwd_weights_reduce call over n_sums column-sum jobs and n_jobs deferred weight gradients of mixed shapes
    (single-split ones strewn in between, which it must leave alone): the step counter goes up by exactly one, every sum is the
    reference's, every weight gradient is bit for bit what defer_reduce = 0 gives."""
    lib = L()
    sum_shapes = sum_shapes or [(r, n, n + 3 * (i % 2)) for i, (r, n) in enumerate(zip((17, 129, 1, 513, 112, 16), (15, 16, 1000, 17, 1, 129)))]
    sums = [_colsum_job(dev, *sum_shapes[i % len(sum_shapes)], seed=i) for i in range(n_sums)]
    direct, jobs, singles = {}, [], []
    for j in range(n_jobs):
        shape, with_db = REDUCE_POOL[j % len(REDUCE_POOL)], (j + j // len(REDUCE_POOL)) % 2 == 0
        inp = _inputs(shape)
        if (shape, with_db) not in direct:
            direct[(shape, with_db)] = _wgrad(dev, inp, with_db, 0)[:2]
        jobs.append((inp, with_db) + _wgrad(dev, inp, with_db, 1))
        if j % 5 == 2:
            one = _wgrad(dev, _inputs(REDUCE_SINGLE), j % 2 == 0, 1)
            assert one[2] is None
            singles.append(one + (one[0].clone(), None if one[1] is None else one[1].clone()))
            jobs.append(None)
    order, k = [], 0
    for jb in jobs:
        if jb is None:
            order.append(singles[k][3])
            k += 1
        else:
            order.append(jb[5])
    arr = (_Split * max(len(order), 1))(*order)
    sarr = (_ColSum * max(n_sums, 1))(*[s[3] for s in sums])
    step = torch.full((1,), STEP0, dtype=torch.int64, device=dev)
    assert lib.recalgo_dense_bwd_weights_reduce(arr, len(order), sarr, n_sums, P(step), _stream()) == 0
    assert int(step.cpu()) == STEP0 + 1, f"{what}: the step counter went from {STEP0} to {int(step.cpu())}"
    for i, (part, _, out, c) in enumerate(sums):
        assert_close(out, R.colsum(part, c.rows, c.row_stride, c.n), what=f"{what} column sum {i} ({c.rows} rows of {c.n})", reduced=True,
                     ref32=R.colsum(part, c.rows, c.row_stride, c.n, dtype=torch.float32))
    seen = set()
    for i, jb in enumerate(j for j in jobs if j is not None):
        inp, with_db, dw, db, _, _ = jb
        want = direct[(inp.shape, with_db)]
        assert_bit_exact(dw, want[0], f"{what} job {i} {inp.shape}: dw deferred vs defer_reduce = 0")
        if with_db:
            assert_bit_exact(db, want[1], f"{what} job {i} {inp.shape}: dbias deferred vs defer_reduce = 0")
        if (inp.shape, with_db) not in seen:
            seen.add((inp.shape, with_db))
            _check_wgrad(dw.cpu(), None if db is None else db.cpu(), inp, f"{what} job {i} {inp.shape}")
    for i, (dw, db, _, _, dw0, db0) in enumerate(singles):
        assert_bit_exact(dw, dw0, f"{what} single-split job {i}: dw after the reduce launch")
        if db is not None:
            assert_bit_exact(db, db0, f"{what} single-split job {i}: dbias after the reduce launch")
        _check_wgrad(dw.cpu(), None if db is None else db.cpu(), _inputs(REDUCE_SINGLE), f"{what} single-split job {i}")
    return [s[2].cpu() for s in sums]


@pytest.mark.parametrize("n_jobs", [1, 31, 32, 33, 64, 65])
def test_reduce_chunks_of_deferred_weight_gradients(dev, n_jobs):
    _reduce_case(dev, 0, n_jobs, f"reduce {n_jobs} jobs")


def _colsum_grid_case(dev):
    shapes = [(r, n, n + s) for r in COLSUM_ROWS for n in COLSUM_N for s in (0, 3)]
    a = _reduce_case(dev, len(shapes), 0, "column-sum grid", sum_shapes=shapes)
    b = _reduce_case(dev, len(shapes), 0, "column-sum grid, again", sum_shapes=shapes)
    for i, (u, v) in enumerate(zip(a, b)):
        assert_bit_exact(u, v, f"column sum {shapes[i]} twice")


def test_reduce_column_sums(dev):
    """rows around the eight-loads-in-flight loop's limit (r + 112 < rows) and the 16 row groups, n around the 16 columns of a
    workgroup, tight and padded rows: 110 jobs in one call (four launches)."""
    _colsum_grid_case(dev)


@pytest.mark.parametrize("n_sums,n_jobs", [(30, 5), (32, 0), (33, 32), (0, 0)])
def test_reduce_sums_and_jobs_share_the_chunks(dev, n_sums, n_jobs):
    _reduce_case(dev, n_sums, n_jobs, f"reduce {n_sums} sums + {n_jobs} jobs")


def test_reduce_with_nothing_to_do_and_no_counter_returns_0(dev):
    """Only the return value is checked: that nothing is launched cannot be observed at the ABI."""
    assert L().recalgo_dense_bwd_weights_reduce(None, 0, None, 0, None, _stream()) == 0
    torch.cuda.synchronize()


def _scalar_arm_case(dev, with_db, which):
    """dw or dbias at a base that is 4 but not 16 bytes aligned: one float per thread, the same slab order as the float4 arm."""
    inp = _inputs((897, 8, 8))
    want = _wgrad(dev, inp, with_db, 0)[:2]
    dw, db, ws, job = _wgrad(dev, inp, with_db, 1, dw_shift=1 if which == "dw" else 0, db_shift=1 if which == "dbias" else 0)
    assert (dw.data_ptr() % 16 == 4) == (which == "dw") and (db is None or (db.data_ptr() % 16 == 4) == (which == "dbias"))
    step = torch.full((1,), STEP0, dtype=torch.int64, device=dev)
    assert L().recalgo_dense_bwd_weights_reduce((_Split * 1)(job), 1, None, 0, P(step), _stream()) == 0
    assert int(step.cpu()) == STEP0 + 1
    assert_bit_exact(dw, want[0], "unaligned reduce: dw")
    if with_db:
        assert_bit_exact(db, want[1], "unaligned reduce: dbias")
    _check_wgrad(dw.cpu(), None if db is None else db.cpu(), inp, f"unaligned {which}")
    d0 = _wgrad(dev, inp, with_db, 0, dw_shift=1 if which == "dw" else 0, db_shift=1 if which == "dbias" else 0)
    assert_bit_exact(d0[0], want[0], "unaligned defer_reduce = 0: dw")


@pytest.mark.parametrize("with_db,which", [(0, "dw"), (1, "dw"), (1, "dbias")])
def test_reduce_scalar_arm_for_unaligned_outputs(dev, with_db, which):
    _scalar_arm_case(dev, with_db, which)


# ---- e. the weight-gradient rider -----------------------------------------------------------------------------------------------
# (main shape of table a, rider (K, N)): the rider's splits at the main shape's M — 8c0c31a: 1 | 2 | 9 | 8 with one empty | 1 | 16 |
# 208, 37 empty.  Not every kind of rider exists at every M: a split holds at least 128 rows, so at M = 129 there are one or two
# splits and never an empty one; a workgroup takes at most 64 chunks of 32 rows, so at M = 27286 there are at least 13 splits.
# (the rider's K and N are multiples of 4: recalgo_dense_bwd_rider requires the float4 arms of both GEMMs)
RIDER_CASES = [((129, 8, 8), (1024, 1024)), ((129, 8, 8), (64, 64)), ((1025, 256, 512), (64, 64)), ((1025, 256, 512), (256, 512)),
               ((1025, 256, 512), (1024, 1024)), ((27286, 8, 8), (256, 256)), ((27286, 8, 8), (8, 64))]


def _rider_case(dev, shape, rider):
    M, K, N = shape
    rK, rN = rider
    inp, rin = _inputs(shape), _inputs((M, rK, rN))
    what = f"rider {rider} beside {shape}"
    lib = L()
    x, g, ym, w = (inp[n].to(dev) for n in ("x", "g", "y_mask", "w"))
    rx, rg = rin["x"].to(dev), rin["g"].to(dev)
    outs = []
    for ride in (True, False):
        dx, dw, db, ws = _nan(M * K, dev).view(M, K), _nan(K * N, dev).view(K, N), _nan(N, dev), _workspace(shape, dev)
        rdw, rdb, rws = _nan(rK * rN, dev).view(rK, rN), _nan(rN, dev), _workspace((M, rK, rN), dev)
        if ride:
            assert lib.recalgo_dense_bwd_rider_supported(P(x), K, P(g), N, P(ym), P(w), M, K, N, P(dx), K, P(rx), rK, P(rg), rN, rK, rN) == 1
            lib.recalgo_dense_bwd_rider(P(x), K, P(g), N, P(ym), P(w), M, K, N, None, 0, 0.0, P(dx), K, P(dw), P(db), P(ws), 1, None,
                                        None, None, None, None, 0, P(rx), rK, P(rg), rN, rK, rN, P(rdw), P(rdb), P(rws),
                                        None, 0, None, None, None, 0, 0, 0, None, None, _stream())
        else:
            lib.recalgo_dense_bwd(P(x), K, P(g), N, P(ym), P(w), M, K, N, None, 0, 0.0, P(dx), K, P(dw), P(db), P(ws), 1, None, None,
                                  None, None, None, 0, _stream())
            lib.recalgo_dense_bwd_weights(P(rx), rK, P(rg), rN, None, M, rK, rN, P(rdw), P(rdb), P(rws), 1, _stream())
        jobs = (_Split * 2)(_Split(M, K, N, 0 if ws is None else ws.data_ptr(), dw.data_ptr(), db.data_ptr()),
                            _Split(M, rK, rN, 0 if rws is None else rws.data_ptr(), rdw.data_ptr(), rdb.data_ptr()))
        assert lib.recalgo_dense_bwd_weights_reduce(jobs, 2, None, 0, None, _stream()) == 0
        outs.append({"dx": dx.cpu(), "dw": dw.cpu(), "dbias": db.cpu(), "r_dw": rdw.cpu(), "r_dbias": rdb.cpu(), "part": None})
    _same(outs[0], outs[1], what + " vs recalgo_dense_bwd + a deferred recalgo_dense_bwd_weights", names=("dx", "dw", "dbias", "r_dw", "r_dbias"))
    _check_bwd(outs[0], inp, what, y_mask=1)
    (_, rw, rb, _), (_, rw32, rb32, _) = rin.ref_bwd(0, "off", "off", 0)
    assert_close(outs[0]["r_dw"], rw, what=f"{what} r_dw", reduced=True, ref32=rw32 if M <= STRICT_MAX else None)
    assert_close(outs[0]["r_dbias"], rb, what=f"{what} r_dbias", reduced=True, ref32=rb32 if M <= STRICT_MAX else None)


@pytest.mark.parametrize("shape,rider", RIDER_CASES, ids=lambda v: "x".join(map(str, v)))
def test_bwd_with_a_weight_gradient_rider(dev, shape, rider):
    _rider_case(dev, shape, rider)


# ---- f. once more behind fences -------------------------------------------------------------------------------------------------
def test_cases_under_the_redzone_guard(dev):
    """tests/test_gpu_redzone.py cannot list a new module.  a, b, d and e once more inside guarded(): every buffer above comes from
    torch.full or Tensor.to, so each lies between 0xFF fences of its own, and a workspace is exactly the size its query gave."""
    with guarded() as g:
        for shape in PARTITION_SHAPES:
            for variant in ("mask+dbias", "plain"):
                _partition_case(dev, shape, variant)
        for shape in PARTITION_BN_SHAPES:
            _partition_case(dev, shape, "bn+relu_mask")
        for row in BWD_ROWS + BWD_EMPTY_SPLIT_ROWS:
            _bwd_row(dev, row, tag="options (guarded)")
        for row in FWD_ROWS:
            _fwd_row(dev, row)
        for n_jobs in (1, 31, 32, 33, 64, 65):
            _reduce_case(dev, 0, n_jobs, f"reduce {n_jobs} jobs (guarded)")
        _colsum_grid_case(dev)
        for n_sums, n_jobs in ((30, 5), (32, 0), (33, 32), (0, 0)):
            _reduce_case(dev, n_sums, n_jobs, f"reduce {n_sums} sums + {n_jobs} jobs (guarded)")
        for with_db, which in ((0, "dw"), (1, "dw"), (1, "dbias")):
            _scalar_arm_case(dev, with_db, which)
        for shape, rider in RIDER_CASES:
            _rider_case(dev, shape, rider)
        assert {"recalgo_dense_fwd", "recalgo_dense_bwd", "recalgo_dense_bwd_input", "recalgo_dense_bwd_weights",
                "recalgo_dense_bwd_weights_workspace_bytes", "recalgo_dense_bwd_weights_reduce", "recalgo_dense_bwd_rider",
                "recalgo_dense_bwd_rider_supported"} <= g.launched
        assert g.records, "the buffers were not allocated under the guard"
