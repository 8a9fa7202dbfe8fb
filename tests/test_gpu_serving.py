"""-m gpu: ServingModel.serve / compile (recalgorithm_amd/export.py) on exports of the golden models.

Per model: the mirror built on the device from the golden's variables (tests/golden_protocol.py), export_model, three serving
models over that export: compiled for the buckets (16, 64) with the fused tower on up to 64 rows, compiled for bucket 16 alone,
and compiled with the tower off.  The request is the 48 golden rows as serialized tf.train.Example protos.

Of the goldens only model_deepfm decodes to a static batch: every other one embeds `manual_tag_list` and
`his_read_comment_7d_seq`, columns that are not declared sequences and hold up to four and eight values a row in the golden
batch.  Such a column shows only in a request, so compile() cannot refuse it; the first request that has one drops the graphs (model_dcn below: served eagerly from then on, a later compile()
refuses).  `<name>-static` is the golden's model without those columns, on seeded variables (BatchNorm statistics away from
(0, 1)): what its compiled graphs are judged against is the float64 oracle run on the mirror's own variables.
  * parity: serve == the golden's PREDICT (static variants: the oracle's), judged as golden_protocol.judge judges PREDICT
    (assert_close with the protocol's ref32); `-<a>x<b>` variants: towers two and three layers deep, with and without BatchNorm;
  * chunking: bucket 16 alone (three chunks) gives the same bits;
  * batch independence: requests of 1 and 17 rows return exactly those rows of the 48-row answer;
  * no stale buffers: forty alternating serves of two requests return the bits of their first answers;
  * tower off: the compiled answer is ServingModel.predict's bit for bit (the same kernels; only decoder and graph are new);
  * not compiled: serve == predict bit for bit;
  * a model with a history (model_din_dice): compile() refuses, naming the key; serve == predict bit for bit."""
import dataclasses

import numpy as np
import pytest
import torch

from recalgorithm_amd import export as E
from recalgorithm_amd import feature_column as fc
from recalgorithm_amd import nn, ops
from recalgorithm_amd.io import tfrecord as T
from tests import golden_util as GU
from tests.golden_protocol import _float_feats, _path, build_on_device, load_variables, restate32
from tests.test_gpu_golden import suite_case
from tests.util import assert_bit_exact, assert_close

pytestmark = pytest.mark.gpu

# string features that hold several values in some row of the golden batch: where a model embeds one without declaring it a
# sequence, it is a Ragged the decoder learns of from a request
BAGS = sorted(k for k, v in GU.string_batch()[0].items() if isinstance(v, list) and max(len(r) for r in v) > 1)
assert BAGS == ["his_read_comment_7d_seq", "manual_tag_list"]
# name -> per layer of the ONE tower a capture launches: whether a BatchNorm's (scale, shift) is folded into it.
# The goldens have hidden_units 16,8: the 16-unit layer (and its BatchNorm) is a tower of one layer, the 8-unit layer is narrower
# than the kernel serves and stays on the dense engine.  `-<a>x<b>[x<c>]` replaces the hidden widths: towers of two and three
# layers through nn.dense / nn.batch_normalization, with a BatchNorm behind every layer (DeepFM and PNN through
# nn.dense_relu_dropout_bn, NFM through dense, then batch_normalization, then dropout) and without one (DCN, xDeepFM).
FOLDED = {"model_deepfm": (True,), "model_dcn-static": (False,),
          "model_deepfm-static-32x16": (True, True), "model_nfm-static-32x16": (True, True),
          "model_pnn_ipnn-static-48x32x16": (True, True, True),
          "model_dcn-static-32x16": (False, False), "model_xdeepfm-static-32x16": (False, False)}
COMPILED = list(FOLDED)


def golden_records():
    """the 48 golden rows as serialized tf.train.Example protos (every string and dense feature of the shared batch)"""
    sfeats, _ = GU.string_batch()
    out = []
    for i in range(48):
        ex = {}
        for k, v in sfeats.items():
            ex[k] = ("bytes", [s.encode() for s in v[i]]) if isinstance(v, list) else ("float", [float(v[i, 0])])
        out.append(T.encode_example(ex))
    return out


def without_the_bag(case, hidden=None):
    """the case whose mirror has no column over a key of BAGS and, with `hidden`, those hidden widths"""
    def setup(name, vocab_dir):
        model_fn, params = case.mirror_setup(name, vocab_dir)
        params = {k: ([c for c in v if getattr(c, "key", None) not in BAGS] if k.endswith("_feature_columns") else v) for k, v in params.items()}
        if hidden is not None:
            params["hidden_units"] = list(hidden)
        return model_fn, params
    return dataclasses.replace(case, mirror_setup=setup)


def seed_variables(est, seed=5):
    """the variables of a trained model rather than of an initialised one: BatchNorm's statistics, scale and offset away from
    (0, 1, 1, 0), biases away from 0"""
    g = torch.Generator().manual_seed(seed)
    for k, v in est.store.named_arrays().items():
        r = torch.randn(v.shape, generator=g)
        leaf = k.split("/")[-1]
        if leaf == "moving_variance":
            v.copy_(0.5 + torch.rand(v.shape, generator=g))
        elif leaf == "gamma":
            v.copy_(1 + 0.2 * r)
        elif leaf in ("beta", "bias", "moving_mean"):
            v.copy_(0.2 * r)


def oracle_predict(case, golden, dtype):
    """PREDICT of the oracle in `dtype` on golden.var and the shared batch"""
    sfeats, _ = GU.string_batch()
    P = {k: torch.from_numpy(np.array(v)).to(dtype) for k, v in golden.var.items()}
    with torch.no_grad():
        return case.oracle(P, _float_feats(case.encode(golden.params, sfeats), dtype), None, golden.params, training=False)


def exported(dev, name, tmp_path):
    """-> (case, golden, model_fn, params, export directory); golden.ref32 is the protocol's ref32 of PREDICT; a static variant's
    golden holds the mirror's variables and the float64 oracle's PREDICT on them"""
    name, *variant = name.split("-")
    static = "static" in variant
    hidden = next((v.split("x") for v in variant if "x" in v), None)
    case = without_the_bag(suite_case(name), hidden) if static else suite_case(name)
    est, golden, _, _ = build_on_device(dev, case, name, tmp_path)
    if static:
        seed_variables(est)
        golden.var = {k: v.detach().cpu().double().numpy() for k, v in est.store.named_arrays().items()}
        golden.d = dict(golden.d)
        r64 = oracle_predict(case, golden, torch.float64)
        for key, path in case.prediction_paths(golden.d).items():
            golden.d[f"predict/{key}"] = _path(r64, path).detach().numpy()
        golden.ref32 = oracle_predict(case, golden, torch.float32)
    else:
        load_variables(est, golden.var)
        golden.ref32 = restate32(case, golden)["predict"]
    model_fn, params = est.model_fn, est.params
    recv = E.build_parsing_serving_input_receiver_fn(fc.make_parse_example_spec(GU.all_columns(params)))
    return case, golden, model_fn, params, E.export_model(est, str(tmp_path / "export"), recv)


class Setup:
    pass


@pytest.fixture(scope="module", params=COMPILED)
def served(request, dev, tmp_path_factory):
    name = request.param
    tmp = tmp_path_factory.mktemp(name)
    s = Setup()
    s.name, s.records = name, golden_records()
    s.case, s.golden, model_fn, params, export_dir = exported(dev, name, tmp)
    assert not any(getattr(c, "key", None) in BAGS for c in GU.all_columns(params))
    s.towers = []
    real = ops.serve_tower

    def counting(x, layers, out=None):
        s.towers.append((int(x.shape[0]), tuple(ly[2] is not None and ly[3] is not None for ly in layers)))
        return real(x, layers, out)
    saved = nn.SERVE_TOWER_MAX_ROWS, nn.SERVE_TOWER_PLAIN_STACKS
    ops.serve_tower = counting
    try:
        nn.SERVE_TOWER_PLAIN_STACKS = True           # (a stack without a BatchNorm takes the tower too: DCN's, xDeepFM's)
        nn.SERVE_TOWER_MAX_ROWS = 64
        s.tower = E.ServingModel(model_fn, params, export_dir, device=dev).compile(batch_sizes=(16, 64))
        s.tower16 = E.ServingModel(model_fn, params, export_dir, device=dev).compile(batch_sizes=(16,))
        s.in_compile = list(s.towers)
        nn.SERVE_TOWER_MAX_ROWS = 0
        s.plain = E.ServingModel(model_fn, params, export_dir, device=dev).compile(batch_sizes=(16, 64))
        s.eager = E.ServingModel(model_fn, params, export_dir, device=dev)
    finally:
        (nn.SERVE_TOWER_MAX_ROWS, nn.SERVE_TOWER_PLAIN_STACKS), ops.serve_tower = saved, real
    s.answer = s.tower.serve(s.records)
    return s


def _same(a, b, what):
    assert sorted(a) == sorted(b), what
    for k in a:
        assert_bit_exact(torch.from_numpy(np.ascontiguousarray(a[k])), torch.from_numpy(np.ascontiguousarray(b[k])), f"{what}: {k}")


def test_the_hidden_stack_was_captured_as_one_launch(served):
    """two warm-up calls and one capture per bucket, each with ONE tower of the model's hidden layers, every BatchNorm folded
    into its layer (a fold that is missed would leave the results right and the BatchNorm a launch of its own); none with
    the tower off"""
    L = FOLDED[served.name]
    assert served.in_compile == [(16, L)] * 3 + [(64, L)] * 3 + [(16, L)] * 3, served.in_compile
    assert served.towers == served.in_compile, "the tower ran outside the captures of the two tower models"
    assert served.tower.tower_buckets() == [16, 64] and served.plain.tower_buckets() == [] and served.plain.compiled_buckets == [16, 64]
    assert served.tower.compiled_buckets == [16, 64] and served.tower.graphs_dropped_by is None, "the request went through the graphs"


def test_parity_with_the_golden(served):
    d, ref32 = served.golden.d, {"predict": served.golden.ref32}
    got = served.answer
    for key, path in served.case.prediction_paths(d).items():
        assert key in got and got[key].shape[0] == 48
        assert_close(torch.from_numpy(got[key]), torch.from_numpy(d[f"predict/{key}"]), what=f"{served.name} served predict/{key}",
                     ref32=_path(ref32["predict"], path))


def test_three_chunks_of_sixteen_give_the_same_bits(served):
    assert [c[2] for c in E.plan_chunks(48, list(served.tower16._buckets))] == [16, 16, 16]
    _same(served.tower16.serve(served.records), served.answer, "bucket 16 alone")


def test_rows_do_not_depend_on_the_request(served):
    for lo, n in ((0, 1), (5, 1), (47, 1), (0, 17), (31, 17)):
        got = served.tower.serve(served.records[lo:lo + n])
        _same(got, {k: v[lo:lo + n] for k, v in served.answer.items()}, f"rows {lo}..{lo + n - 1} as a request of their own")


def test_no_stale_buffers(served):
    a, b = served.records[:17], served.records[20:48]
    first = served.tower.serve(a), served.tower.serve(b)
    for i in range(40):
        _same(served.tower.serve(a if i % 2 == 0 else b), first[i % 2], f"serve {i}")


def test_with_the_tower_off_the_graph_computes_what_predict_computes(served):
    want = served.eager.predict(served.records)
    _same(served.plain.serve(served.records), want, "compiled, per-layer kernels, against predict")
    _same(served.plain.serve(served.records[3:20]), served.eager.predict(served.records[3:20]), "17 rows in the bucket of 64")


def test_uncompiled_serve_is_predict(served):
    _same(served.eager.serve(served.records), served.eager.predict(served.records), "native decode + eager model_fn")
    _same(served.eager.serve(served.records[7:8]), served.eager.predict(served.records[7:8]), "one row")


def test_a_bag_that_shows_only_in_a_request_drops_the_graphs(dev, tmp_path):
    """model_dcn as the golden has it: compile() cannot know of its two bags; the first request that holds several values
    says so, is served eagerly (== predict bit for bit, == the golden), and compile() then refuses."""
    case, golden, model_fn, params, export_dir = exported(dev, "model_dcn", tmp_path)
    records = golden_records()
    model = E.ServingModel(model_fn, params, export_dir, device=dev).compile(batch_sizes=(16, 64))
    assert sorted(model._buckets) == [16, 64]
    with pytest.warns(UserWarning, match="holds several values in a record.*served eagerly"):
        got = model.serve(records)
    assert model.compiled_buckets == [] and model.graphs_dropped_by in BAGS and model.ragged_keys() == BAGS
    _same(got, model.predict(records), "model_dcn: serve against predict")
    ref32 = restate32(case, golden)
    for key, path in case.prediction_paths(golden.d).items():
        assert_close(torch.from_numpy(got[key]), torch.from_numpy(golden.d[f"predict/{key}"]), what=f"model_dcn served predict/{key}",
                     ref32=_path(ref32["predict"], path))
    with pytest.raises(NotImplementedError, match=", ".join(BAGS)):
        model.compile(batch_sizes=(16, 64))


def test_a_model_with_a_history_is_served_eagerly(dev, tmp_path):
    _, _, model_fn, params, export_dir = exported(dev, "model_din_dice", tmp_path)
    model = E.ServingModel(model_fn, params, export_dir, device=dev)
    with pytest.raises(NotImplementedError, match="his_read_comment_7d_seq"):
        model.compile(batch_sizes=(16, 64))
    records = golden_records()
    want = model.predict(records)
    _same(model.serve(records), want, "model_din_dice: serve against predict")
    assert not model._buckets
    with pytest.raises(NotImplementedError, match="his_read_comment_7d_seq"):
        model.compile()


def test_a_plain_stack_stays_on_the_per_layer_kernels(dev, tmp_path, monkeypatch):
    """nn.SERVE_TOWER_PLAIN_STACKS off (its measured setting): DCN's dense(relu) stack folds no BatchNorm, is collected under
    the switch all the same and then runs as the launches `dense` makes: no tower, predict's bits."""
    _, _, model_fn, params, export_dir = exported(dev, "model_dcn-static-32x16", tmp_path)
    calls, real = [], ops.serve_tower
    monkeypatch.setattr(ops, "serve_tower", lambda *a, **k: calls.append(1) or real(*a, **k))
    monkeypatch.setattr(nn, "SERVE_TOWER_MAX_ROWS", 64)
    monkeypatch.setattr(nn, "SERVE_TOWER_PLAIN_STACKS", False)
    model = E.ServingModel(model_fn, params, export_dir, device=dev).compile(batch_sizes=(16, 64))
    records = golden_records()
    _same(model.serve(records), E.ServingModel(model_fn, params, export_dir, device=dev).predict(records), "plain stack, compiled")
    assert not calls and model.compiled_buckets == [16, 64] and model.tower_buckets() == []
