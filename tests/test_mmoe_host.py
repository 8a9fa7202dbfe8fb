"""CPU (no kernels launched): the MMoE feature's host side.
  * tests/mmoe_ref.py (the float64 restatement the GPU tests compare against) reproduces both goldens that
    scripts/gen_golden_mmoe.py obtained by executing the reference's own algorithm/MMOE/mmoe.py on oracle/tf1_shim;
  * the generator's --check round trip (where the reference folder exists);
  * the gate-mix backward formulas as written in csrc/mmoe.hip's header comment, against float64 autograd;
  * three labels through the native TFRecord reader; the opt-in extra labels of the synthetic device batch;
  * the mirror's variables, and the multi-task tail's PREDICT / EVAL keys, on the launch-free registration pass."""
import os
import subprocess
import sys

import pytest
import torch

from tests import golden_util as GU
from tests import mmoe_ref
from tests.golden_protocol import GoldenCase, close, restate_on_host

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDENS = ["model_mmoe", "model_mmoe_dropout"]
TASKS = ["read_comment", "like", "click_avatar"]


def mirror_setup(name, vocab_dir):
    """(model_fn, params) of the mirror for golden `name`, from the mirror's own create_feature_columns()."""
    from recalgorithm_amd import flags
    from recalgorithm_amd.algorithm.MMOE import mmoe as m
    d = GU.load(name)
    fl = {k: (v.item() if v.shape == () else v) for k, v in GU.section(d, "flag/").items()}
    flags.FLAGS.vocabulary_dir = vocab_dir
    for k, v in fl.items():
        setattr(flags.FLAGS, k, v)
    dense, cat, label = m.create_feature_columns()
    assert [c.key for c in label] == str(fl["task_names"]).split(",")
    return m.mmoe_model_fn, {
        "dense_feature_columns": dense, "category_feature_columns": cat, "hidden_units": str(fl["hidden_units"]).split(","),
        "dropout_rate": float(fl["dropout_rate"]), "batch_norm": bool(fl["batch_norm"]), "learning_rate": float(fl["learning_rate"]),
        "num_experts": int(fl["num_experts"]), "num_tasks": int(fl["num_tasks"]),
        "expert_hidden_units": int(fl["expert_hidden_units"]), "task_names": str(fl["task_names"]).split(",")}


def encode(params, sfeats):
    """string features -> the restatement's feature batch (ids; (values, offsets) for multi-valued keys)."""
    from recalgorithm_amd.feature_column import NumericColumn, Ragged
    feats = {}
    for c in GU.all_columns(params):
        if isinstance(c, NumericColumn):
            feats[c.key] = sfeats[c.key].double()
            continue
        cat = c.categorical_column
        x = cat.ids({cat.key: sfeats[cat.key]}, torch.device("cpu"))
        feats[cat.key] = (x.values, x.offsets) if isinstance(x, Ragged) else x
    return feats


def multitask_case(mirror_setup, oracle, n_grads):
    """the golden-parity case of a three-task model (MMoE here, PLE in tests/test_ple_host.py): labels, predictions and EVAL
    metrics per task, six dropout calls (two hidden layers in each of three towers)"""
    return GoldenCase(mirror_setup=mirror_setup, oracle=oracle, encode=encode, tasks=TASKS,
                      predictions={f"{t}_probabilities": ("probs", t) for t in TASKS}, n_grads=n_grads, n_masks=6)


CASE = multitask_case(mirror_setup, mmoe_ref.mmoe, 46)


@pytest.mark.parametrize("name", GOLDENS)
def test_restatement_reproduces_the_golden(name, tmp_path):
    restate_on_host(CASE, name, tmp_path)


def test_generator_check_round_trip():
    from oracle import gen_golden
    if not os.path.isdir(os.path.join(gen_golden.REF, "MMOE")):
        pytest.skip("the reference folder is not on this machine")
    r = subprocess.run([sys.executable, os.path.join(ROOT, "scripts", "gen_golden_mmoe.py"), "--check"], cwd=ROOT,
                       capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "model_mmoe.npz  checked" in r.stdout and "model_mmoe_dropout.npz  checked" in r.stdout


def gate_mix_backward_formulas(x, ws, experts, selection, p_rows, d_outs, relu_experts=False):
    """The backward of csrc/mmoe.hip's header comment, written out (float64):
        c[g][e] = sum_{j: sel[g][j] = e} p_g[j];  d_expert_e = sum_g c[g][e] * d_out_g (zeroed where expert_e <= 0 if relu)
        dp_g[j] = <d_out_g, expert_{sel[g][j]}>;  dz_g = p_g * (dp_g - sum_j p_g[j] dp_g[j])
        dx = sum_g dz_g Wg^T;  dWg = x^T dz_g          (d_outs[g] None: zero)"""
    dex = [torch.zeros_like(e) for e in experts]
    dx = torch.zeros_like(x)
    dws = []
    for w, sel, p, do in zip(ws, selection, p_rows, d_outs):
        if do is None:
            dws.append(torch.zeros_like(w))
            continue
        for j, e in enumerate(sel):
            dex[e] += p[:, j:j + 1] * do
        dp = torch.stack([(do * experts[e]).sum(dim=1) for e in sel], dim=1)
        dz = p * (dp - (p * dp).sum(dim=1, keepdim=True))
        dx += dz @ w.t()
        dws.append(x.t() @ dz)
    if relu_experts:
        dex = [d * (e > 0) for d, e in zip(dex, experts)]
    return dx, dws, dex


@pytest.mark.parametrize("shape", [(29, 7, 3, 3, 8, None), (13, 5, 1, 1, 4, None),
                                   (17, 6, 4, 3, 12, [[0, 1, 3], [2, 3], [0, 1, 2, 3]]), (11, 4, 2, 2, 4, [[1, 1, 0], [0]])])
def test_gate_mix_backward_formulas_against_autograd(shape):
    B, In, E, G, H, selection = shape
    gen = torch.Generator().manual_seed(B * 131 + H)
    selection = [list(range(E)) for _ in range(G)] if selection is None else selection
    x = torch.randn(B, In, generator=gen, dtype=torch.float64, requires_grad=True)
    ws = [torch.randn(In, len(s), generator=gen, dtype=torch.float64, requires_grad=True) for s in selection]
    experts = [torch.randn(B, H, generator=gen, dtype=torch.float64, requires_grad=True) for _ in range(E)]
    d_outs = [torch.randn(B, H, generator=gen, dtype=torch.float64) for _ in range(G)]
    if G > 1:
        d_outs[1] = None                     # a gate nobody differentiates
    outs, ps = mmoe_ref.gate_mix(x, ws, experts, selection)
    loss = sum((o * d).sum() for o, d in zip(outs, d_outs) if d is not None)
    grads = torch.autograd.grad(loss, [x, *ws, *experts], allow_unused=True)
    grads = [torch.zeros_like(t) if g is None else g for g, t in zip(grads, [x, *ws, *experts])]
    with torch.no_grad():
        dx, dws, dex = gate_mix_backward_formulas(x, ws, experts, selection, ps, d_outs)
    close(dx, grads[0], "dx", tol=1e-12)
    for g, (a, b) in enumerate(zip(dws, grads[1:1 + G])):
        close(a, b, f"dW{g}", tol=1e-12)
    for e, (a, b) in enumerate(zip(dex, grads[1 + G:])):
        close(a, b, f"d_expert{e}", tol=1e-12)
    # experts that are ReLU outputs: the masked form is the gradient at the pre-activation
    pre = [torch.randn(B, H, generator=gen, dtype=torch.float64, requires_grad=True) for _ in range(E)]
    relu = [torch.relu(t) for t in pre]
    outs, ps = mmoe_ref.gate_mix(x, ws, relu, selection)
    loss = sum((o * d).sum() for o, d in zip(outs, d_outs) if d is not None)
    gpre = torch.autograd.grad(loss, pre, allow_unused=True)
    with torch.no_grad():
        _, _, dex = gate_mix_backward_formulas(x, ws, [t.detach() for t in relu], selection, ps, d_outs, relu_experts=True)
    for e, (a, b) in enumerate(zip(dex, gpre)):
        close(a, torch.zeros_like(a) if b is None else b, f"d_expert{e} (relu)", tol=1e-12)


def test_three_labels_through_the_native_reader(tmp_path):
    from recalgorithm_amd import build as B
    from recalgorithm_amd import feature_column as fc
    from recalgorithm_amd.algorithm.utils import _Dataset, eval_input_fn, parse_example
    from recalgorithm_amd.io import native, synth
    B.build_host(verbose=False)
    native.load()
    tasks = ["read_comment", "like", "click_avatar"]
    spec = synth.SynthSpec(n_fields=6, max_vocab=300, seed=5, oov_frac=0.1, with_dense=True)
    vocab_dir = str(tmp_path / "vocabulary") + "/"
    synth.write_vocabularies(spec, vocab_dir)
    path = str(tmp_path / "ex.tfrecord")
    synth.write_tfrecord(spec, path, 150, chunk=64)
    from recalgorithm_amd.algorithm._common import DENSE_FEATURES
    cols = [fc.numeric_column(k, default_value=0.0) for k in DENSE_FEATURES]
    cols += [fc.embedding_column(fc.categorical_column_with_vocabulary_file(nm, vocab_dir + nm + ".txt"), 8) for nm in spec.names]
    labels = [fc.numeric_column(t, default_value=0.0) for t in tasks]

    def parser(serialized):
        f = parse_example(serialized, fc.make_parse_example_spec(cols + labels))
        return f, {t: f.pop(t) for t in tasks}
    parser.columns_getter = lambda: (cols, labels)
    nat = eval_input_fn(path, parser, 64)
    assert isinstance(nat.upstream, native.NativeDataset)
    nb, pb = list(nat), list(_Dataset(path, parser, 64, 1, 0))
    assert len(nb) == len(pb) == 3
    seen = {t: 0.0 for t in tasks}
    for (nf, nl), (pf, pl) in zip(nb, pb):
        assert list(nl) == tasks == list(pl)
        assert not any(t in nf for t in tasks)
        for t in tasks:
            assert nl[t].dtype == torch.float32 and tuple(nl[t].shape) == (pl[t].shape[0], 1)
            assert torch.equal(nl[t], pl[t]), t
            seen[t] += float(nl[t].sum())
    assert sum(seen.values()) > 0            # (the labels are not all-default zeros)


def test_device_batch_extra_labels_are_opt_in():
    from recalgorithm_amd.io import synth
    spec = synth.SynthSpec(n_fields=4, max_vocab=100, seed=3)
    f0, l0, _ = synth.device_features(spec, 64, torch.device("cpu"))
    f1, l1, _ = synth.device_features(spec, 64, torch.device("cpu"), extra_labels=("like", "click_avatar"))
    assert list(l0) == ["read_comment"] and list(l1) == ["read_comment", "like", "click_avatar"]
    assert torch.equal(l0["read_comment"], l1["read_comment"]) and all(torch.equal(f0[k], f1[k]) for k in f0)
    assert all(tuple(l1[k].shape) == (64, 1) and l1[k].dtype == torch.float32 for k in l1)
    f2, l2, _ = synth.device_features(spec, 64, torch.device("cpu"), batch_index=1, extra_labels=("like",))
    assert torch.equal(l2["like"], synth.device_features(spec, 64, torch.device("cpu"), 1, extra_labels=("like",))[1]["like"])
    with pytest.raises(ValueError):
        synth.device_features(spec, 64, torch.device("cpu"), extra_labels=("nope",))


def check_registration_pass(case, name, tmp_path):
    """the mirror's variables and the multi-task tail's keys on the launch-free registration pass (shared with
    tests/test_ple_host.py)"""
    from recalgorithm_amd.estimator import Estimator, ModeKeys, RunConfig
    vocab_dir = GU.write_vocab_dir(str(tmp_path / "vocabulary"))
    model_fn, params = case.mirror_setup(name, vocab_dir)
    d = GU.load(name)
    tasks = params["task_names"]
    sfeats, labels = GU.string_batch()
    feats = {k: (v.float() if isinstance(v, torch.Tensor) else v) for k, v in sfeats.items()}
    lab = {t: v.float() for t, v in case.labels(d, labels).items()}
    assert list(lab) == tasks
    est = Estimator(model_fn, params, RunConfig(device="cpu", seed=3, use_hip_graph=False))
    est.build(feats, lab)                    # registration pass only: no HIP call
    arrays = est.store.named_arrays()
    gv = GU.section(d, "var/")
    assert not [k for k in gv if k not in arrays], "reference variables absent from the mirror"
    assert not [k for k in arrays if k not in gv], "mirror variables the reference does not have"
    for k, v in gv.items():
        assert tuple(arrays[k].shape) == tuple(v.shape), (k, arrays[k].shape, v.shape)
    # the multi-task tail's keys, on the same launch-free pass
    est.store.building = True
    try:
        with torch.no_grad():
            pred = est._call_model_fn(feats, None, ModeKeys.PREDICT)
            ev = est._call_model_fn(feats, lab, ModeKeys.EVAL)
    finally:
        est.store.building = False
    assert sorted(pred.predictions) == sorted(f"{t}_probabilities" for t in tasks)
    assert pred.export_outputs == {"prediction": pred.predictions}
    assert all(tuple(v.shape) == (48, 1) for v in pred.predictions.values())
    assert sorted(ev.eval_metric_ops) == sorted([f"eval_{t}_accuracy" for t in tasks] + [f"eval_{t}_auc" for t in tasks])
    assert ev.loss is not None and ev.loss.dim() == 0


@pytest.mark.parametrize("name", GOLDENS)
def test_mirror_variables_and_tail_keys_on_the_registration_pass(name, tmp_path):
    check_registration_pass(CASE, name, tmp_path)


def test_limits_raise_not_implemented():
    """outside the kernel's limits the Python side raises, like the tree's other limit guards (the limits themselves are
    checked again by the entry point; this needs the built library, not a GPU: built here if stale, as tests/test_abi.py does)"""
    from recalgorithm_amd import build, ops
    build.build(verbose=False)
    assert ops.gate_mix_supported(82, 3, 3, 512, 9) and ops.gate_mix_supported(82, 8, 9, 128, 40)
    assert not ops.gate_mix_supported(82, 3, 3, 510, 9)          # H % 4
    assert not ops.gate_mix_supported(82, 17, 3, 512, 51)        # E > 16
    assert not ops.gate_mix_supported(82, 3, 17, 512, 51)        # G > 16
    assert not ops.gate_mix_supported(513, 3, 3, 512, 3)         # In > 512
    assert not ops.gate_mix_supported(400, 3, 3, 512, 12)        # 400 * 13 floats > the 16 KiB LDS budget
    x, e = torch.zeros(4, 82), [torch.zeros(4, 510) for _ in range(3)]
    with pytest.raises(NotImplementedError):
        ops.gate_mix(x, [torch.zeros(82, 3) for _ in range(3)], e)
    with pytest.raises(ValueError):
        ops.gate_mix(x, [torch.zeros(82, 0)], [torch.zeros(4, 8) for _ in range(3)], [[]])       # a gate over no expert
    with pytest.raises(NotImplementedError):
        ops.multitask_sigmoid_cross_entropy([torch.zeros(4, 1)] * 17, [torch.zeros(4, 1)] * 17)


def test_input_grad_chain_accepts_an_offer_only_with_a_registered_consumer():
    """the gates' share of d x may leave autograd only when a consumer that returns d x has registered in its forward"""
    from recalgorithm_amd import nn
    t = torch.zeros(2, 3)
    chain = nn.InputGradChain()
    assert not chain.offer(t) and chain.first is None            # nobody would pick it up: the gates return it themselves
    chain.register_consumer()
    assert chain.offer(t) and not chain.offer(t)                 # one addend is held at a time
    assert chain.take() is t and chain.take() is None
    assert not chain.offer(t)                                    # the consumer's backward has run
