"""GPU: BST's transformer block (csrc/bst.hip, include/recalgo_bst.h).
  * each kernel pair at the C ABI against tests/bst_ref.py in float64 (ref32 = the same restatement in float32), under the
    guarded, poisoned allocations of tests/redzone.py: every output and every gradient, `out` and `pool` separately and
    together, sum and mean pooling, over T x (d, H) x B with B once above the backward grid's cap;
  * two runs are bit-equal; argument checks refuse before any launch;
  * the autograd ops of ops.py (tensor parameters) against the same reference;
  * both goldens through the mirrored bst_model_fn (variable names, PREDICT, loss, every gradient — the shared
    position_embedding's two-block sum among them —, the Adam step, EVAL); --static_sequence_length: PREDICT against the
    padded restatement, and 40 hipGraph replays of the captured step bit for bit against eager launches."""
import ctypes
import functools

import pytest
import torch

from recalgorithm_amd import _lib, ops
from tests import bst_ref as R
from tests.redzone import guarded
from tests.util import assert_bit_exact, assert_close

pytestmark = pytest.mark.gpu

TS = (1, 2, 17, 51, 64)
DH = ((16, 3), (16, 1), (8, 4), (4, 2))
CAP = 512                   # recalgo_bst_attn_bwd_partial_rows' cap (asserted below)
BS = (1, 3, CAP + 5)


def _ptr(t):
    return None if t is None else ctypes.c_void_p(t.data_ptr())


def _stream():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


@functools.lru_cache(maxsize=4)
def _references(B, T, d, H):
    """(case, attention fp64, attention fp32, n1 as the FFN kernels' fp32 input, {ffn variant: (fp64, fp32)}), computed once"""
    case = R.random_case(B, T, d, H, seed=1000 * T + 10 * d + H + B)
    a64, a32 = R.attention_reference(case, torch.float64), R.attention_reference(case, torch.float32)
    n1 = a64["n1"].to(torch.float32)
    ffn = {}
    for variant, (pooling, use_out, use_pool) in FFN_VARIANTS.items():
        ffn[variant] = tuple(R.ffn_reference(case, n1, dt, pooling, use_out, use_pool) for dt in (torch.float64, torch.float32))
    return case, a64, a32, n1, ffn


FFN_VARIANTS = {"out only": ("sum", True, False), "sum pool only": ("sum", False, True), "out and mean pool": ("mean", True, True)}


def run_attention(g, dev, case, B, T, d, H, lib=None):
    lib = lib or _lib.load()
    c = {k: g.input(v.to(torch.float32) if v.is_floating_point() else v, dev) for k, v in case.items()
         if k in ("x", "keys_length", "g_n1") + R.ATTN_PARAMS}
    n1 = torch.empty(B, T, d, device=dev)
    stats = torch.empty(B, 2, device=dev)
    lib.recalgo_bst_attn_fwd(_ptr(c["x"]), _ptr(c["pos"]), _ptr(c["keys_length"]), *[_ptr(c[k]) for k in R.ATTN_PARAMS[1:]],
                             B, T, d, H, _ptr(n1), _ptr(stats), _stream())
    outs = {"dx": torch.empty(B, T, d, device=dev), "dpos": torch.empty(T, d, device=dev)}
    outs.update({"d" + k: torch.empty_like(c[k]) for k in R.ATTN_PARAMS[1:]})
    nbytes = int(lib.recalgo_bst_attn_bwd_workspace_bytes(B, T, d, H))
    rows = int(lib.recalgo_bst_attn_bwd_partial_rows(B))
    assert nbytes == 4 * rows * (T * d + 4 * H * d * d + 2 * d) and rows == min(B, CAP)
    ws = ops._workspace(nbytes, dev)
    lib.recalgo_bst_attn_bwd(_ptr(c["x"]), _ptr(c["pos"]), _ptr(c["keys_length"]), *[_ptr(c[k]) for k in R.ATTN_PARAMS[1:6]],
                             _ptr(c["g_n1"]), B, T, d, H, _ptr(outs["dx"]), _ptr(outs["dpos"]),
                             *[_ptr(outs["d" + k]) for k in R.ATTN_PARAMS[1:]], _ptr(ws), _stream())
    outs["n1"], outs["stats"] = n1, stats
    return outs


def run_ffn(g, dev, case, n1, B, T, d, pooling, use_out, use_pool, lib=None):
    lib = lib or _lib.load()
    c = {k: g.input(case[k].to(torch.float32), dev) for k in ("g_out", "g_pool") + R.FFN_PARAMS}
    n1 = g.input(n1, dev)
    out = torch.empty(B, T, d, device=dev) if use_out else None
    pool = torch.empty(B, d, device=dev) if use_pool else None
    stats = torch.empty(B, 2, device=dev)
    mean = int(pooling == "mean")
    lib.recalgo_bst_ffn_fwd(_ptr(n1), *[_ptr(c[k]) for k in R.FFN_PARAMS], B, T, d, mean, _ptr(out), _ptr(pool), _ptr(stats),
                            _stream())
    outs = {"dn1": torch.empty(B, T, d, device=dev)}
    outs.update({"d" + k: torch.empty_like(c[k]) for k in R.FFN_PARAMS})
    nbytes = int(lib.recalgo_bst_ffn_bwd_workspace_bytes(B, d))
    assert nbytes == 4 * int(lib.recalgo_bst_ffn_bwd_partial_rows(B)) * (d * d + 3 * d)
    ws = ops._workspace(nbytes, dev)
    lib.recalgo_bst_ffn_bwd(_ptr(n1), *[_ptr(c[k]) for k in R.FFN_PARAMS[:3]], _ptr(c["g_out"]) if use_out else None,
                            _ptr(c["g_pool"]) if use_pool else None, B, T, d, mean, _ptr(outs["dn1"]),
                            *[_ptr(outs["d" + k]) for k in R.FFN_PARAMS], _ptr(ws), _stream())
    outs["out"], outs["pool"], outs["stats"] = out, pool, stats
    return outs


def _compare(got, r64, r32, names, what, T):
    for k in names:
        ref, ref32 = r64[k], r32[k]
        if k == "dpos":
            ref, ref32 = ref[:T], ref32[:T]          # (the table has rows nobody reads: their gradient is zero)
        summed = k.startswith("d") and k not in ("dx", "dn1")        # a sum over the batch: the fp32 accumulation floor applies
        assert_close(got[k], ref, what=f"{what} {k}", ref32=ref32, reduced=summed)


@pytest.mark.parametrize("B", BS)
@pytest.mark.parametrize("d,H", DH)
@pytest.mark.parametrize("T", TS)
def test_kernels_at_the_abi_against_float64(dev, T, d, H, B):
    case, a64, a32, n1, ffn = _references(B, T, d, H)
    what = f"T={T} d={d} H={H} B={B}"
    with guarded() as g:
        got = run_attention(g, dev, case, B, T, d, H)
        _compare(got, a64, a32, ["n1", "dx", "dpos"] + ["d" + k for k in R.ATTN_PARAMS[1:]], "attn " + what, T)
        for variant, (pooling, use_out, use_pool) in FFN_VARIANTS.items():
            f64, f32 = ffn[variant]
            gotf = run_ffn(g, dev, case, n1, B, T, d, pooling, use_out, use_pool)
            names = (["out"] if use_out else []) + (["pool"] if use_pool else []) + ["dn1"] + ["d" + k for k in R.FFN_PARAMS]
            _compare(gotf, f64, f32, names, f"ffn {variant} {what}", T)
        assert {"recalgo_bst_attn_fwd", "recalgo_bst_attn_bwd", "recalgo_bst_ffn_fwd", "recalgo_bst_ffn_bwd"} <= g.launched
    # (mean, rstd) of the attention's LayerNorm, as the header states them
    c = {k: (v.double() if v.is_floating_point() else v) for k, v in case.items()}
    p, _, _ = R.probabilities(c["x"], c["keys_length"], c["pos"], c["w_q"], c["w_k"])
    v = torch.einsum("bik,hkj->bhij", c["x"], c["w_v"])
    y = (p @ v).permute(0, 2, 1, 3).reshape(B, T, H * d) @ c["w_o"] + c["x"] + c["pos"][:T]
    mean = y.mean(dim=(1, 2))
    rstd = torch.rsqrt(((y - mean[:, None, None]) ** 2).mean(dim=(1, 2)) + R.LN_EPS)
    assert_close(got["stats"], torch.stack([mean, rstd], dim=1), what=f"attn stats {what}")


def test_two_runs_are_bit_equal(dev):
    B, T, d, H = CAP + 5, 51, 16, 3
    case, _, _, n1, _ = _references(B, T, d, H)
    with guarded() as g:
        a, b = (run_attention(g, dev, case, B, T, d, H) for _ in range(2))
        for k in a:
            assert_bit_exact(a[k], b[k], f"attention {k}")
        fa, fb = (run_ffn(g, dev, case, n1, B, T, d, "mean", True, True) for _ in range(2))
        for k in fa:
            assert_bit_exact(fa[k], fb[k], f"ffn {k}")


def test_argument_checks_refuse_before_any_launch(dev):
    B, T, d, H = 3, 17, 16, 3
    case, _, _, n1, _ = _references(B, T, d, H)
    lib = _lib.load()
    assert lib.recalgo_bst_attn_bwd_partial_rows(CAP + 5) == CAP == lib.recalgo_bst_ffn_bwd_partial_rows(10 ** 6)
    for T_, d_, H_, ok in ((1, 4, 1, 1), (64, 16, 4, 1), (51, 16, 3, 1), (33, 8, 4, 1), (65, 16, 3, 0), (17, 5, 3, 0), (17, 16, 5, 0),
                           (0, 16, 3, 0), (17, 20, 1, 0), (17, 16, 0, 0)):
        assert lib.recalgo_bst_supported(T_, d_, H_) == ok, (T_, d_, H_)
    with guarded() as g:
        c = {k: g.input(v.to(torch.float32) if v.is_floating_point() else v, dev) for k, v in case.items()}
        out = torch.empty(B, 65, 16, device=dev)
        args = [_ptr(c["x"]), _ptr(c["pos"]), _ptr(c["keys_length"]), *[_ptr(c[k]) for k in R.ATTN_PARAMS[1:]]]

        def refused(fn, *a):
            with pytest.raises(_lib.RecalgoError, match="failed with hipError_t=1$"):
                fn(*a)
        refused(lib.recalgo_bst_attn_fwd, *args, B, 65, d, H, _ptr(out), None, _stream())
        refused(lib.recalgo_bst_attn_fwd, *args, B, T, 5, H, _ptr(out), None, _stream())
        refused(lib.recalgo_bst_attn_fwd, *args, B, T, d, H, None, None, _stream())
        refused(lib.recalgo_bst_attn_fwd, None, *args[1:], B, T, d, H, _ptr(out), None, _stream())
        refused(lib.recalgo_bst_attn_fwd, ctypes.c_void_p(c["x"].data_ptr() + 2), *args[1:], B, T, d, H, _ptr(out), None, _stream())
        refused(lib.recalgo_bst_attn_fwd, *args, 0, T, d, H, _ptr(out), None, _stream())
        f = [_ptr(g.input(n1, dev)), *[_ptr(c[k]) for k in R.FFN_PARAMS]]
        refused(lib.recalgo_bst_ffn_fwd, *f, B, T, d, 0, None, None, None, _stream())
        refused(lib.recalgo_bst_ffn_fwd, *f, B, 65, d, 0, _ptr(out), None, None, _stream())
        refused(lib.recalgo_bst_ffn_fwd, *f, B, T, 5, 0, _ptr(out), None, None, _stream())
        refused(lib.recalgo_bst_ffn_bwd, *f[:4], None, None, B, T, d, 0, *([_ptr(out)] * 6), _stream())
        refused(lib.recalgo_bst_attn_bwd, *args[:8], _ptr(c["g_n1"]), B, T, d, H, *([_ptr(out)] * 8), None, _stream())
        torch.cuda.synchronize()
        assert bool(torch.isnan(out).all()), "a refused call wrote its output"
    x = torch.zeros(2, 65, 16, device=dev)
    kl = torch.ones(2, dtype=torch.int32, device=dev)
    w = torch.zeros(3, 16, 16, device=dev)
    with pytest.raises(ValueError, match="there is no fallback"):
        ops.bst_attention(x, kl, torch.zeros(65, 16, device=dev), w, w, w, torch.zeros(48, 16, device=dev),
                          torch.ones(16, device=dev), torch.zeros(16, device=dev))
    with pytest.raises(ValueError, match="there is no fallback"):
        ops.bst_ffn(torch.zeros(2, 3, 5, device=dev), torch.zeros(5, 5, device=dev), *([torch.zeros(5, device=dev)] * 3))


@pytest.mark.parametrize("pooling", ["sum", "mean", None])
def test_autograd_ops_against_float64(dev, pooling):
    B, T, d, H = 3, 17, 16, 3
    case, _, _, _, _ = _references(B, T, d, H)

    def run(dtype, device, attn, ffn):
        c = {k: (v.to(dtype) if v.is_floating_point() else v).to(device) for k, v in case.items()}
        leaves = {k: c[k].clone().requires_grad_(True) for k in ("x",) + R.ATTN_PARAMS + R.FFN_PARAMS}
        n1 = attn(leaves["x"], c["keys_length"], *[leaves[k] for k in R.ATTN_PARAMS])
        out, pl = ffn(n1, *[leaves[k] for k in R.FFN_PARAMS])
        loss = (out * c["g_out"]).sum() if pooling is None else (pl * c["g_pool"]).sum() + 0.5 * (out * c["g_out"]).sum()
        loss.backward()
        return {"out": out.detach(), **({} if pooling is None else {"pool": pl.detach()}), **{"d" + k: v.grad for k, v in leaves.items()}}

    def ref_ffn(n1, *p):
        out = R.ffn(n1, *p)
        return out, None if pooling is None else R.pool(out, pooling)
    r64, r32 = (run(dt, "cpu", R.attention, ref_ffn) for dt in (torch.float64, torch.float32))
    got = run(torch.float32, dev, ops.bst_attention, lambda n1, *p: ops.bst_ffn(n1, *p, pool=pooling))
    for k in r64:
        assert_close(got[k], r64[k], what=f"ops pool={pooling} {k}", ref32=r32[k], reduced=k.startswith("d") and k != "dx")


# ---- the model ------------------------------------------------------------------------------------------------------------------
from recalgorithm_amd import feature_column as fc  # noqa: E402
from recalgorithm_amd.estimator import HOUSEKEEPING_EVERY, Estimator, GraphedTrainStep, ModeKeys, RunConfig, _tree_tensors  # noqa: E402
from recalgorithm_amd.io import synth  # noqa: E402
from tests import golden_util as GU  # noqa: E402
from tests.golden_protocol import check_on_device  # noqa: E402
from tests.test_bst_host import CASE, GOLDENS, mirror_setup  # noqa: E402
from tests.test_mmoe_host import encode  # noqa: E402


@pytest.mark.parametrize("name", list(GOLDENS))
def test_model_golden(dev, name, tmp_path):
    """Both goldens through the mirrored bst_model_fn: variable names, PREDICT, loss, every gradient (the shared
    position_embedding's sum over two blocks among them), the Adam step, EVAL."""
    check_on_device(dev, CASE, name, tmp_path)


def make_bst(dev, B=256, history_len=20, blocks=2, heads=3, pooling="mean", dropout_rate=0.1, static=True, hidden=("64", "32"),
             fields=8, max_vocab=500, emb=16, seed=42):
    """A BST estimator over synthetic device-resident features (bench.py's DIN layout: profile fields + the target feed and its
    history sharing one table) -> (estimator, synth spec)."""
    from recalgorithm_amd.algorithm.BST.bst import bst_model_fn
    spec = synth.SynthSpec(n_fields=fields, max_vocab=max_vocab, with_history=True, history_len=history_len)
    cmap = {n: fc.categorical_column_with_identity(n, v) for n, v in zip(spec.names, spec.vocabs)}
    his = fc.categorical_column_with_identity("his_read_comment_7d_seq", cmap["feedid"].num_buckets)
    his.is_sequence = True
    feed = cmap.pop("feedid")
    feed.is_sequence = True
    shared = fc.shared_embedding_columns([feed, his], emb, combiner="mean")
    params = {"dense_feature_columns": [], "category_feature_columns": [fc.embedding_column(c, emb) for c in cmap.values()],
              "target_feedid_feature_columns": [shared[0]], "sequence_feature_columns": [shared[1]],
              "hidden_units": list(hidden), "dropout_rate": dropout_rate, "batch_norm": True, "learning_rate": 0.005,
              "sequence_max_length": 50, "num_transformer_block": blocks, "num_transformer_heads": heads,
              "pooling_method": pooling, "static_sequence_length": static}
    est = Estimator(model_fn=bst_model_fn, params=params, config=RunConfig(device=dev, seed=seed))
    feats, labels, _ = synth.device_features(spec, B, dev, batch_index=0)
    est.build(feats, labels)
    return est, spec


WARMUP, STEPS, N_BATCHES = 3, 40, 5


def _state(est, losses):
    torch.cuda.synchronize()
    out = {f"loss of step {i}": l.cpu() for i, l in enumerate(losses)}
    out.update({f"var {k}": v.detach().cpu().clone() for k, v in est.store.named_arrays().items()})
    for n, ar in est.store.arenas.items():
        out[f"arena {n}.m"], out[f"arena {n}.v"] = ar.m.cpu().clone(), ar.v.cpu().clone()
    out["flat_m"], out["flat_v"] = est.store.flat_m.cpu().clone(), est.store.flat_v.cpu().clone()
    out["step counter"] = est.store.opt_state["step"].cpu().clone()
    return out


def _differences(a, b):
    assert a.keys() == b.keys()
    bad = []
    for k in a:
        x, y = a[k], b[k]
        assert x.dtype == y.dtype and x.shape == y.shape, k
        if x.dtype == torch.float32:
            x, y = x.contiguous().view(torch.int32), y.contiguous().view(torch.int32)
        if not torch.equal(x, y):
            bad.append(k)
    return bad


def test_static_sequence_length_captured_step_replays_what_eager_steps_compute(dev):
    """--static_sequence_length: 40 hipGraph replays of the captured step against eager launches on rotating batches, bit for
    bit (tests/test_gpu_replay_models.py's comparison; two blocks, mean pooling, dropout; histories of 20 padded to 50, so
    the mask rows and the shared position_embedding's two-block gradient are in the captured step)."""
    assert STEPS > HOUSEKEEPING_EVERY
    (eager, spec), (graphed, _) = make_bst(dev), make_bst(dev)
    batches = [synth.device_features(spec, 256, dev, batch_index=i)[:2] for i in range(N_BATCHES)]
    keep = [[t.clone() for _, t in _tree_tensors({"f": b[0], "l": b[1]}, "b")] for b in batches]
    for _ in range(WARMUP):
        eager.train_step(*batches[0])
    le = []
    for i in range(STEPS):
        le.append(eager.train_step(*batches[i % N_BATCHES]).clone())
        if (i + 1) % HOUSEKEEPING_EVERY == 0:
            eager.store.housekeeping()
    first = _state(eager, le)
    assert int(first["step counter"]) == WARMUP + STEPS and all(torch.isfinite(l).all() for l in le)
    assert float(le[-1]) != float(le[0])
    g = GraphedTrainStep(graphed.train_step, *batches[0], warmup=WARMUP)
    lg = [g(*batches[i % N_BATCHES]).clone() for i in range(STEPS)]
    diff = _differences(first, _state(graphed, lg))
    assert not diff, f"{STEPS} replays of the captured BST step differ from eager launches in {diff[:8]} ({len(diff)} in all)"
    assert all(torch.equal(t, k) for b, kept in zip(batches, keep) for (_, t), k in zip(_tree_tensors({"f": b[0], "l": b[1]}, "b"), kept))


def test_static_sequence_length_pads_to_the_maximum(dev, tmp_path):
    """The mirror with --static_sequence_length on the golden's variables: PREDICT equals the restatement padded to
    sequence_max_length + 1 = 51 rows (42 of them padding for every example), not the golden's T = 9."""
    name = "model_bst_two_blocks_mean_dropout"
    vocab_dir = GU.write_vocab_dir(str(tmp_path / "vocabulary"))
    model_fn, params = mirror_setup(name, vocab_dir, static_sequence_length=True)
    d = GU.load(name)
    sfeats, labels = GU.string_batch()
    gv = GU.section(d, "var/")
    enc = encode(params, sfeats)
    ref = R.bst({k: torch.from_numpy(v.copy()) for k, v in gv.items()}, enc, None, params, training=False)["prob"]
    ref32 = R.bst({k: torch.from_numpy(v.copy()).float() for k, v in gv.items()},
                  {k: (v.float() if isinstance(v, torch.Tensor) and v.is_floating_point() else v) for k, v in enc.items()},
                  None, params, training=False)["prob"]
    assert float((ref - torch.from_numpy(d["predict/probabilities"])).abs().max()) > 1e-3
    feats = {k: (v.float() if isinstance(v, torch.Tensor) else v) for k, v in sfeats.items()}
    lab = {"read_comment": labels.float()}
    est = Estimator(model_fn, params, RunConfig(device=dev, seed=3, use_hip_graph=False))
    est.build(feats, lab)
    feats, lab = est._to_device(feats, lab)
    arrays = est.store.named_arrays()
    for k, v in gv.items():
        arrays[k].copy_(torch.from_numpy(v).float().reshape(arrays[k].shape))
    pr = est._call_model_fn(feats, None, ModeKeys.PREDICT)
    assert_close(pr.predictions["probabilities"], ref, what="static PREDICT", ref32=ref32)
