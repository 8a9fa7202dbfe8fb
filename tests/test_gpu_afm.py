"""-m gpu: nn.afm_attention, the owner of AFM's attention network (pair products, relu(pairs @ w + b) @ h, softmax over the pairs,
weighted sum), against tests/afm_ref.py, the float64 / float32 restatement of afm.py:162-188 through torch autograd: the output
and the gradients of the fields, w, b and h at every shape the network's kernels change path, where the scores are large, run
to run and under torch.cuda.graph; and the model, which reaches the network through this one function."""
import pytest
import torch

from recalgorithm_amd import nn, ops
from recalgorithm_amd.variables import VariableStore, use_store
from tests import afm_ref as R
from tests.util import assert_bit_exact, assert_close

pytestmark = pytest.mark.gpu


def make_step(dev, x, fused=None):
    """-> step(): nn.afm_attention forward + backward on a store of its own that holds the case's w, bias, h; returns
    [out, d_fields, dw, dbias, dh] (the last three are the variables' gradient buffers: clone them to keep a run's values)."""
    B, F, K = x["fields"].shape
    t = x["w"].shape[1]
    store = VariableStore(dev, seed=3)
    with use_store(store):
        store.building = True                # the registration pass: get_variable creates, nothing is launched
        vs = {"w": store.get_variable("attention_w", (K, t)), "bias": store.get_variable("attention_b", (t,)),
              "h": store.get_variable("attention_h", (t, 1))}
        store.finalize()                     # packs the variables: from here each has its slice of the flat gradient buffer
    with torch.no_grad():
        for k, v in vs.items():
            v.data.copy_(x[k])
    fields = x["fields"].reshape(B, F * K).to(dev).requires_grad_(True)
    g = x["g"].to(dev)

    def step():
        with use_store(store):
            store.begin_call()               # a model_fn invocation starts: drops deferred work a failed step may have left
            fields.grad = None
            out = nn.afm_attention(fields, F, K, vs["w"], vs["bias"], vs["h"], fused=fused)
            out.backward(g)
            ops.flush_dense_splits()         # the dense engine's weight gradients are split sums: without this dw, dbias are partial
        return [out.detach(), fields.grad.reshape(B, F, K), vs["w"].grad, vs["bias"].grad, vs["h"].grad]
    return step


def run_op(dev, x, fused=None):
    return {k: v.clone() for k, v in zip(R.NAMES, make_step(dev, x, fused)())}


# (B, F, K, t)
SHAPES = [(1, 2, 8, 12),         # P = 1: the softmax is 1, ds is 0
          (5, 3, 4, 32),         # P = 3
          (130, 7, 8, 12),       # the golden's shape; t not a tile multiple
          (67, 9, 16, 128),      # P = 36
          (33, 26, 16, 128),     # the bench shape's P = 325
          (3, 64, 8, 32),        # F = 64, P = 2016
          (3, 4, 32, 256)]       # K = 32, t = 256


@pytest.mark.parametrize("fused", [None, False], ids=["fused=None", "fused=False"])
@pytest.mark.parametrize("B,F,K,t", SHAPES)
def test_parity(dev, B, F, K, t, fused):
    x, r64, r32 = R.case(B, F, K, t)
    got = run_op(dev, x, fused)
    for k in R.NAMES:
        assert got[k].shape == r64[k].shape, (k, got[k].shape, r64[k].shape)
        assert_close(got[k], r64[k], what=f"nn.afm_attention B={B} F={F} K={K} t={t} {k}", reduced=k in ("dw", "dbias", "dh"),
                     ref32=r32[k])


@pytest.mark.parametrize("name", list(R.LARGE_SCORES))
def test_large_scores(dev, name):
    """bias = +1, h = +5 at (67, 9, 16, 128): scores of 550 .. 1186, a zero pair row would score relu(1) * 5 * 128 = 640.
    h scaled until the scores of (33, 7, 8, 12) span more than +-200: exp() of an unshifted score would overflow or vanish.
    Every output is finite, the softmax is the float64 one's, and parity holds with the floor of afm_ref.fp32_floor (4 x the
    float32 restatement's own deviation; what that restatement leaves outside the bare rtol: tests/test_afm_host.py)."""
    x, r64, r32 = R.case(**R.LARGE_SCORES[name])
    got = run_op(dev, x)
    for k in R.NAMES:
        assert bool(torch.isfinite(got[k]).all()), k
        assert_close(got[k], r64[k], what=f"nn.afm_attention, {name}: {k}", reduced=k in ("dw", "dbias", "dh"), ref32=r32[k],
                     floor=R.fp32_floor(r64, r32, k))


def test_two_runs_and_three_replays_give_the_same_bits(dev):
    x, _, _ = R.case(67, 9, 16, 128)
    step = make_step(dev, x)
    first = [o.clone() for o in step()]
    for name, u, w_ in zip(R.NAMES, step(), first):
        assert_bit_exact(u, w_, f"second eager run, {name}")
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        step()
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        captured = step()
    for i in range(3):
        for c in captured:
            c.zero_()
        graph.replay()
        torch.cuda.synchronize()
        for name, u, w_ in zip(R.NAMES, captured, first):
            assert_bit_exact(u, w_, f"replay {i}, {name}")


# ---- the model ---------------------------------------------------------------------------------------------------------------------
def _model_case(fused):
    from tests.test_gpu_golden import suite_case
    case = suite_case("model_afm")
    inner = case.mirror_setup

    def setup(name, vocab_dir):
        model_fn, params = inner(name, vocab_dir)
        assert "afm_fused" not in params, "not a reference parameter: absent in every existing caller"
        return model_fn, (params if fused == "absent" else dict(params, afm_fused=fused))
    case.mirror_setup = setup
    return case


@pytest.mark.parametrize("fused", ["absent", None, False], ids=["key absent", "afm_fused=None", "afm_fused=False"])
def test_the_model_reaches_the_network_through_its_owner(dev, fused, tmp_path, monkeypatch):
    """The model_afm golden (F = 7, K = 8, t = 12) through the protocol — PREDICT, the loss, every variable's gradient and
    post-step value — with a counting wrapper around nn.afm_attention: PREDICT and TRAIN each call it once, with the key's value."""
    from tests.golden_protocol import check_on_device
    calls = []
    real = nn.afm_attention

    def counted(*a, **kw):
        calls.append(kw.get("fused", "not passed"))
        return real(*a, **kw)
    monkeypatch.setattr(nn, "afm_attention", counted)
    check_on_device(dev, _model_case(fused), "model_afm", tmp_path)
    assert calls == [None if fused == "absent" else fused] * 2, calls


def test_the_model_refuses_a_fused_path_that_no_kernel_serves(dev, tmp_path):
    from recalgorithm_amd.estimator import ModeKeys
    from tests.golden_protocol import build_on_device
    est, _, feats, _ = build_on_device(dev, _model_case(True), "model_afm", tmp_path)
    with pytest.raises(ValueError, match=r"afm_attention\(fused=True\)"):
        est._call_model_fn(feats, None, ModeKeys.PREDICT)
