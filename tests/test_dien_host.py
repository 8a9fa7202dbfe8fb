"""CPU: DIEN's interest module without a GPU.
  * tests/dien_ref.py, the restatement the GPU tests compare against: the two places where the product departs from the
    reference's call sequence change no bit of any output or gradient (float64): the first GRU with against without
    `lengths`, and T = the batch's longest history against T padded to 64; AGRU leaves the u half of the gates gradient
    exactly zero, AUGRU does not;
  * include/recalgo_dien.h literally: names, signatures, launches, constants, the `supported` truth table, the workspace
    formulas, refusals on NULL;
  * the two header tables of _lib, and every per-header check of tests/test_abi.py on the new header;
  * nn.dien_gru / nn.dien_evolve on the launch-free registration pass: TF's variable names, shapes and initialisers;
  * the model: tests/dien_ref.dien reproduces the three goldens at the protocol's 1e-10 and the generator's --check passes;
    the two labelled differences on the whole model; the mirror's variables on the registration pass, its flags against the
    reference's text, what it refuses; three LazyAdam steps of the float64 oracle, which differ from dense Adam's."""
import ctypes
import os
import re
import subprocess
import sys

import pytest
import torch

from tests import dien_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "recalgo_dien.h")
NAME = "recalgo_dien.h"
MODULE_PARAMS = ("x", "target", "w_att") + R.CELL_PARAMS + ("eWg", "ebg", "eWc", "ebc")


def module(case, first_gru_lengths=True, pad_to=None):
    """gru -> evolve -> sum(final * g_final) in float64 -> {final, loss, att, d<every input and parameter>}"""
    p = {k: case[k].clone().requires_grad_(True) for k in MODULE_PARAMS}
    x, T = p["x"], case["x"].shape[1]
    if pad_to is not None:
        x = torch.cat([x, x.new_zeros(x.shape[0], pad_to - T, x.shape[2])], dim=1)
    h = R.gru(x, case["lengths"] if first_gru_lengths else None, *[p[k] for k in R.CELL_PARAMS])
    att, _, final = R.evolve(h, p["target"], case["lengths"], p["w_att"], p["eWg"], p["ebg"], p["eWc"], p["ebc"], case["mode"])
    loss = (final * case["g_final"]).sum()
    loss.backward()
    return {"final": final.detach(), "loss": loss.detach(), "att": att.detach()[:, :T], **{"d" + k: v.grad for k, v in p.items()}}


def _case(mode, B=7, T=9, na=16, nh=8, seed=11):
    case = R.random_case(B, T, na, nh, mode, seed)
    case["lengths"] = case["lengths"].clamp(max=T)
    assert {0, 1, T} <= set(case["lengths"].tolist())
    return case


@pytest.mark.parametrize("mode", [R.AGRU, R.AUGRU])
def test_lengths_on_the_first_gru_change_no_bit(mode):
    """The reference runs its first GRU over all T rows (dien.py:202); the product passes `lengths`.  The rows h[t >= L]
    that differ reach only replaced scores (weight exactly 0, tf.where's gradient exactly 0) and copied-through steps."""
    case = _case(mode)
    with_l, without = module(case, True), module(case, False)
    assert with_l.keys() == without.keys()
    for k in with_l:
        assert torch.equal(with_l[k], without[k]), k
    assert float(with_l["dWg"].abs().max()) > 0 and float(with_l["dx"].abs().max()) > 0


@pytest.mark.parametrize("mode", [R.AGRU, R.AUGRU])
def test_padding_to_a_static_length_changes_no_bit(mode):
    """T = the batch's longest history (the reference) against the same batch padded to 64 steps (sequence_max_length): a
    replaced score adds an exact 0 to the softmax's sum — for the examples with L >= 1; an empty history gets 1 / T of
    whatever T is, a weight no step uses."""
    case = _case(mode)
    short, padded = module(case), module(case, pad_to=64)
    some = case["lengths"] >= 1
    for k in short:
        a, b = (short[k][some], padded[k][some]) if k == "att" else (short[k], padded[k])
        assert torch.equal(a, b), k


def test_agru_leaves_the_update_gate_without_a_gradient():
    nh = 8
    agru, augru = module(_case(R.AGRU)), module(_case(R.AUGRU))
    assert bool((agru["deWg"][:, nh:] == 0).all()) and bool((agru["debg"][nh:] == 0).all())
    assert float(agru["deWg"][:, :nh].abs().min()) > 0
    assert float(augru["deWg"][:, nh:].abs().min()) > 0 and float(augru["debg"][nh:].abs().min()) > 0


def test_rows_past_the_length_and_the_empty_history():
    case = _case(R.AUGRU)
    T = case["x"].shape[1]
    h = R.gru(case["x"], case["lengths"], *[case[k] for k in R.CELL_PARAMS])
    att, states, final = R.evolve(case["h_in"], case["target"], case["lengths"], case["w_att"], case["eWg"], case["ebg"], case["eWc"],
                                  case["ebc"], R.AUGRU)
    dead = torch.arange(T)[None, :] >= case["lengths"][:, None]
    assert bool((h[dead] == 0).all()) and bool((states[dead] == 0).all())
    empty = case["lengths"] == 0
    assert bool((att[empty] == 1.0 / T).all()) and bool((final[empty] == 0).all())
    assert bool((att[~empty][dead[~empty]] == 0).all()) and torch.allclose(att.sum(dim=1), torch.ones(att.shape[0], dtype=att.dtype))
    # the reset gate is applied before the candidate's product: one step against its formula written out
    x, h0 = case["x"][:, 0], case["h_in"][:, 0]
    nh = h0.shape[1]
    g = torch.sigmoid(torch.cat([x, h0], 1) @ case["Wg"] + case["bg"])
    c = torch.tanh(x @ case["Wc"][:x.shape[1]] + (g[:, :nh] * h0) @ case["Wc"][x.shape[1]:] + case["bc"])
    assert torch.allclose(R.cell(x, h0, *[case[k] for k in R.CELL_PARAMS]), g[:, nh:] * h0 + (1 - g[:, nh:]) * c, rtol=0, atol=1e-15)


# ---- the header ---------------------------------------------------------------------------------------------------------------
DECLARED = ["recalgo_dien_abi_version", "recalgo_dien_supported", "recalgo_dien_gru_bwd_partial_rows",
            "recalgo_dien_gru_bwd_workspace_bytes", "recalgo_dien_evolve_bwd_partial_rows", "recalgo_dien_evolve_bwd_workspace_bytes",
            "recalgo_dien_gru_fwd", "recalgo_dien_gru_bwd", "recalgo_dien_evolve_fwd", "recalgo_dien_evolve_bwd"]
LAUNCHES = ["recalgo_dien_gru_fwd", "recalgo_dien_gru_bwd", "recalgo_dien_evolve_fwd", "recalgo_dien_evolve_bwd"]


def test_header_literal_expectations():
    from recalgorithm_amd import _lib, build, ops
    build.build(verbose=False)
    abi = _lib.MORE_HEADERS[NAME]
    assert list(abi.functions) == DECLARED
    assert abi.launches == LAUNCHES
    assert not abi.structs
    lib = _lib.load()
    assert lib.recalgo_dien_abi_version() == abi.version == 1 and abi.label == "DIEN ABI"
    c_int, i64, ptr = ctypes.c_int, ctypes.c_int64, ctypes.c_void_p
    F = abi.functions
    assert F["recalgo_dien_abi_version"] == (c_int, []) and F["recalgo_dien_supported"] == (c_int, [c_int] * 3)
    assert F["recalgo_dien_gru_bwd_partial_rows"] == F["recalgo_dien_evolve_bwd_partial_rows"] == (c_int, [c_int])
    assert F["recalgo_dien_gru_bwd_workspace_bytes"] == F["recalgo_dien_evolve_bwd_workspace_bytes"] == (i64, [c_int] * 3)
    assert F["recalgo_dien_gru_fwd"] == (c_int, [ptr] * 6 + [c_int] * 4 + [ptr] * 2)
    assert F["recalgo_dien_gru_bwd"] == (c_int, [ptr] * 8 + [c_int] * 4 + [ptr] * 7)
    assert F["recalgo_dien_evolve_fwd"] == (c_int, [ptr] * 8 + [c_int] * 5 + [ptr] * 4)
    assert F["recalgo_dien_evolve_bwd"] == (c_int, [ptr] * 11 + [c_int] * 5 + [ptr] * 9)
    # the sizes and limits the header states (host-side queries: no device needed)
    served = (4, 8, 12, 16)
    for T in (0, 1, 50, 64, 65):
        for na in range(0, 22):
            for nh in range(0, 22):
                assert lib.recalgo_dien_supported(T, na, nh) == int(1 <= T <= 64 and na in served and nh in served), (T, na, nh)
    for entry in (lib.recalgo_dien_gru_bwd_partial_rows, lib.recalgo_dien_evolve_bwd_partial_rows):
        assert [entry(B) for B in (0, 1, 3, 256, 257, 10 ** 6)] == [1, 1, 3, 256, 256, 256]
    assert lib.recalgo_dien_gru_bwd_workspace_bytes(4096, 16, 8) == 4 * 256 * (24 * 16 + 16 + 24 * 8 + 8)
    assert lib.recalgo_dien_gru_bwd_workspace_bytes(3, 4, 12) == 4 * 3 * (16 * 24 + 24 + 16 * 12 + 12)
    assert lib.recalgo_dien_evolve_bwd_workspace_bytes(4096, 16, 8) == 4 * 256 * (8 * 16 + 16 * 16 + 16 + 16 * 8 + 8)
    assert lib.recalgo_dien_evolve_bwd_workspace_bytes(7, 12, 16) == 4 * 7 * (16 * 12 + 32 * 32 + 32 + 32 * 16 + 16)
    assert lib.recalgo_dien_gru_bwd_workspace_bytes(8, 5, 8) == 0 and lib.recalgo_dien_evolve_bwd_workspace_bytes(8, 16, 20) == 0
    # a launch that returns an error raises through the errcheck (NULL buffers: refused before any launch)
    with pytest.raises(_lib.RecalgoError, match="recalgo_dien_gru_fwd failed with hipError_t=1$"):
        lib.recalgo_dien_gru_fwd(*([None] * 6), 1, 1, 4, 4, None, None)
    with pytest.raises(_lib.RecalgoError, match="recalgo_dien_gru_bwd failed with hipError_t=1$"):
        lib.recalgo_dien_gru_bwd(*([None] * 8), 1, 1, 4, 4, *([None] * 7))
    with pytest.raises(_lib.RecalgoError, match="recalgo_dien_evolve_fwd failed with hipError_t=1$"):
        lib.recalgo_dien_evolve_fwd(*([None] * 8), 1, 1, 4, 4, 1, *([None] * 4))
    with pytest.raises(_lib.RecalgoError, match="recalgo_dien_evolve_bwd failed with hipError_t=1$"):
        lib.recalgo_dien_evolve_bwd(*([None] * 11), 1, 1, 4, 4, 2, *([None] * 9))
    defines = {m.group(1): int(m.group(2), 0) for m in re.finditer(r"#define (RECALGO_DIEN_\w+) (0x[0-9A-Fa-f]+|\d+)", open(HEADER).read())
               if not m.group(1).endswith("_H_")}
    assert abi.constants == defines == {"RECALGO_DIEN_ABI_VERSION": 1, "RECALGO_DIEN_MAX_T": 64, "RECALGO_DIEN_MAX_NA": 16,
                                        "RECALGO_DIEN_MAX_NH": 16, "RECALGO_DIEN_MODE_GRU": 0, "RECALGO_DIEN_MODE_AGRU": 1,
                                        "RECALGO_DIEN_MODE_AUGRU": 2}
    assert (ops.DIEN_MAX_T, ops.DIEN_MAX_NA, ops.DIEN_MAX_NH) == (64, 16, 16) and ops.DIEN_MODES == {"AGRU": 1, "AUGRU": 2}
    assert (R.GRU, R.AGRU, R.AUGRU) == (0, 1, 2)


def test_the_two_header_tables():
    from recalgorithm_amd import _lib
    assert list(_lib.HEADERS) == ["recalgo.h", "recalgo_cgc.h", "recalgo_wide.h", "recalgo_bst.h", "recalgo_res.h"]
    assert list(_lib.MORE_HEADERS) == [NAME]
    assert list(_lib.all_headers()) == list(_lib.HEADERS) + [NAME]
    lib = _lib.load()
    for abi in _lib.all_headers().values():                      # load() has walked both tables
        for name, (res, args) in abi.functions.items():
            fn = getattr(lib, name)
            assert fn.restype is res and list(fn.argtypes) == args and (fn.errcheck is not None) == (name in abi.launches), name


def test_every_shared_abi_check_holds_for_the_new_header(monkeypatch):
    """tests/test_abi.py runs once per entry of _lib.HEADERS; with the table replaced by the union of both, each of its
    per-header checks is called on the new header, and the all-pairs check on the union."""
    from recalgorithm_amd import _lib, build
    from tests import test_abi as A
    union = _lib.all_headers()
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
    A.test_stale_version_fails_loudly(NAME, lib_path, monkeypatch)


def test_the_record_script_accepts_headers_of_either_table(tmp_path):
    """scripts/abi_record.py re-records the current version's line, for a header of each table — on a COPY of the tree
    (include/, the script, the package's python files): the tree's own records are never written by a test."""
    import shutil
    from recalgorithm_amd import _abi
    copy = tmp_path / "tree"
    shutil.copytree(os.path.join(ROOT, "include"), copy / "include")
    os.makedirs(copy / "scripts")
    shutil.copy(os.path.join(ROOT, "scripts", "abi_record.py"), copy / "scripts" / "abi_record.py")
    shutil.copytree(os.path.join(ROOT, "recalgorithm_amd"), copy / "recalgorithm_amd",
                    ignore=lambda d, names: [n for n in names if not (n.endswith(".py") or os.path.isdir(os.path.join(d, n)))
                                             or n in ("build", "csrc", "csrc_host", "__pycache__")])
    env = {k: v for k, v in os.environ.items() if k != "PYTHONPATH"}

    def record(header):
        return subprocess.run([sys.executable, str(copy / "scripts" / "abi_record.py"), header], capture_output=True, text=True,
                              cwd=str(copy), env=env)
    for header in ("recalgo_bst.h", NAME):
        path = copy / "include" / (os.path.splitext(header)[0] + ".abi")
        before = path.read_text()
        assert before == open(_abi.record_path(header)).read()
        out = record(header)
        assert out.returncode == 0, out.stderr
        assert out.stdout.split() == ["1", _abi.declaration_hash(header)]
        assert path.read_text() == before, f"re-recording {header} changed its record"
        path.write_text("# only the comment is left\n")              # a lost line is written again: the copy's file is the one the script writes
        assert record(header).returncode == 0 and path.read_text() == "# only the comment is left\n" + before.splitlines()[-1] + "\n"
        assert open(_abi.record_path(header)).read() == before
    out = record("recalgo_nope.h")
    assert out.returncode != 0 and NAME in out.stderr and "recalgo_res.h" in out.stderr


# ---- the variable-owning wrappers on the launch-free registration pass --------------------------------------------------------
WRAPPER_VARIABLES = {"seq_encoder/rnn/gru_cell/gates/kernel": (24, 16), "seq_encoder/rnn/gru_cell/gates/bias": (16,),
                     "seq_encoder/rnn/gru_cell/candidate/kernel": (24, 8), "seq_encoder/rnn/gru_cell/candidate/bias": (8,),
                     "seq_encoder/attention_project_matrix": (8, 16),
                     "seq_encoder/rnn/gates/kernel": (16, 16), "seq_encoder/rnn/gates/bias": (16,),
                     "seq_encoder/rnn/candidate/kernel": (16, 8), "seq_encoder/rnn/candidate/bias": (8,)}


def interest_module(store, x, target, lengths, nh, kind):
    """dien.py:199-229 through the wrappers of nn.py -> (final, att)"""
    from recalgorithm_amd import nn
    from recalgorithm_amd.variables import use_store
    with use_store(store), store.variable_scope("seq_encoder"):
        h = nn.dien_gru(x, lengths, nh)
        return nn.dien_evolve(h, target, lengths, kind)


def test_wrappers_register_tf_names_shapes_and_initialisers():
    from recalgorithm_amd.variables import VariableStore
    store = VariableStore("cpu", seed=3)
    store.building = True                         # the registration pass: no HIP call
    final, att = interest_module(store, torch.zeros(5, 9, 16), torch.zeros(5, 16), torch.ones(5, dtype=torch.int32), 8, "AUGRU")
    assert tuple(final.shape) == (5, 8) and tuple(att.shape) == (5, 9)
    assert {k: tuple(v.shape) for k, v in store.vars.items()} == WRAPPER_VARIABLES and store.order == list(WRAPPER_VARIABLES)
    for k, v in store.vars.items():
        if k.endswith("gates/bias"):
            assert bool((v.data == 1).all()), k
        elif k.endswith("candidate/bias"):
            assert bool((v.data == 0).all()), k
        else:                                     # glorot uniform: inside its limit, and not degenerate
            lim = (6.0 / sum(v.shape)) ** 0.5
            assert 0.5 * lim < float(v.data.abs().max()) <= lim, k
    def fresh():
        s = VariableStore("cpu", seed=3)
        s.building = True
        return s
    with pytest.raises(ValueError, match="there is no fallback"):
        interest_module(fresh(), torch.zeros(5, 65, 16), torch.zeros(5, 16), torch.ones(5), 8, "AGRU")
    with pytest.raises(ValueError, match="there is no fallback"):
        interest_module(fresh(), torch.zeros(5, 9, 16), torch.zeros(5, 16), torch.ones(5), 6, "AGRU")
    with pytest.raises(ValueError, match="custom_gru_type"):
        interest_module(fresh(), torch.zeros(5, 9, 16), torch.zeros(5, 16), torch.ones(5), 8, "GRU")


# ---- the goldens: tests/dien_ref.py against the reference's own sources run on oracle/tf1_shim ------------------------------------
import numpy as np  # noqa: E402

from tests import golden_util as GU  # noqa: E402
from tests.golden_protocol import GoldenCase, close, restate_on_host  # noqa: E402
from tests.test_mmoe_host import encode  # noqa: E402

GOLDENS = {"model_dien": 28, "model_dien_augru_dropout": 28, "model_dien_augru_prelu": 28}          # name -> gradient arrays


def mirror_setup(name, vocab_dir, **extra):
    """(model_fn, params) of the mirror for golden `name`, from the mirror's own create_feature_columns()."""
    from recalgorithm_amd import flags
    from recalgorithm_amd.algorithm.DIEN import dien as m
    d = GU.load(name)
    fl = {k: (v.item() if v.shape == () else v) for k, v in GU.section(d, "flag/").items()}
    flags.FLAGS.vocabulary_dir = vocab_dir
    for k, v in fl.items():
        setattr(flags.FLAGS, k, v)
    dense, cat, tgt, seq, neg, _ = m.create_feature_columns()
    return m.dien_model_fn, dict({
        "dense_feature_columns": dense, "category_feature_columns": cat, "sequence_feature_columns": seq,
        "negative_sequence_feature_columns": neg, "target_feedid_feature_columns": tgt,
        "hidden_units": str(fl["hidden_units"]).split(","), "dropout_rate": float(fl["dropout_rate"]),
        "batch_norm": bool(fl["batch_norm"]), "learning_rate": float(fl["learning_rate"]), "activation": str(fl["activation"]),
        "use_auxiliary_loss": bool(fl["use_auxiliary_loss"]), "negative_sample_number": 3,
        "custom_gru_type": str(fl["custom_gru_type"]), "gru_output_units": int(fl["gru_output_units"])}, **extra)


CASE = GoldenCase(mirror_setup=mirror_setup, oracle=R.dien, encode=encode, predictions={"probabilities": ("prob",)},
                  ordered_prediction_keys=True, n_grads=GOLDENS, n_masks=2,
                  # Dice's own BatchNorm has no `training=` (activations.py:29-37): its moving statistics stay (0, 1) for ever and
                  # are constants of the kernels' epilogue, not variables of the mirror — as for DIN
                  golden_only=r"dice_bn", skip_absent=True)
INTEREST = ("seq_encoder/rnn/gru_cell/gates/kernel", "seq_encoder/rnn/gru_cell/candidate/kernel", "seq_encoder/attention_project_matrix",
            "seq_encoder/rnn/gates/kernel", "seq_encoder/rnn/candidate/kernel")


@pytest.mark.parametrize("name", list(GOLDENS))
def test_restatement_reproduces_the_golden(name, tmp_path):
    """What the reference's unmodified dien.py and custom_grucell.py computed on the shim against tests/dien_ref.dien — which
    passes `lengths` to the first GRU too, while the reference does not: the first labelled difference, at the protocol's
    bound on every output, gradient and updated variable.  (One LazyAdam step from zero moments is one Adam step.)"""
    bn_state = {}
    golden, run = restate_on_host(CASE, name, tmp_path, bn_state=bn_state)
    feats, P, gg, ga = run["feats"], run["P"], golden.grad, golden.var_after
    lens = feats["his_read_comment_7d_seq"][1][1:] - feats["his_read_comment_7d_seq"][1][:-1]
    assert int(lens.min()) == 0 and int(lens.max()) == 8 and int((lens < 8).sum()) > 0, "the batch has padded rows and an empty history"
    assert set(WRAPPER_VARIABLES) <= set(golden.var) and all(tuple(golden.var[k].shape) == s for k, s in WRAPPER_VARIABLES.items())
    assert all(np.all(golden.var[k] == 1.0) for k in golden.var if k.endswith("gates/bias"))
    assert all(np.all(golden.var[k] == 0.0) for k in golden.var if k.endswith("candidate/bias"))
    u_half = gg["seq_encoder/rnn/gates/kernel"][:, 8:], gg["seq_encoder/rnn/gates/bias"][8:]
    if golden.params["custom_gru_type"] == "AGRU":
        assert all(np.all(t == 0.0) for t in u_half) and np.any(gg["seq_encoder/rnn/gates/kernel"][:, :8] != 0.0)
    else:
        assert all(np.any(t != 0.0) for t in u_half)
    assert bn_state
    for scope, (mean, var) in bn_state.items():
        close(0.99 * P[f"{scope}/moving_mean"].detach() + 0.01 * mean, ga[f"{scope}/moving_mean"], f"{name} {scope} moving_mean")
        close(0.99 * P[f"{scope}/moving_variance"].detach() + 0.01 * var, ga[f"{scope}/moving_variance"], f"{name} {scope} moving_variance")


def _model_run(name, tmp_path, **kw):
    vocab_dir = GU.write_vocab_dir(str(tmp_path / "vocabulary"))
    _, params = mirror_setup(name, vocab_dir)
    d = GU.load(name)
    sfeats, labels = GU.string_batch()
    P = {k: torch.from_numpy(v.copy()).requires_grad_("/moving_" not in k) for k, v in GU.section(d, "var/").items()}
    out = R.dien(P, encode(params, sfeats), {"read_comment": labels}, params, training=True,
                 dropout_masks=GU.dropout_masks(d), **kw)
    out["loss"].backward()
    return out, {k: p.grad for k, p in P.items() if p.grad is not None}


@pytest.mark.parametrize("name", list(GOLDENS))
def test_the_two_labelled_differences_change_no_bit_of_the_model(name, tmp_path):
    """The whole model in float64 on the golden's variables and batch: the first GRU with against without `lengths`, and T =
    the batch's longest history (8) against T padded to 64 — the same loss, the same probabilities, every gradient EXACTLY."""
    base, gbase = _model_run(name, tmp_path)
    assert len(gbase) == GOLDENS[name] and all(float(gbase[k].abs().max()) > 0 for k in INTEREST)
    for kw in ({"first_gru_lengths": False}, {"pad_to": 64}, {"first_gru_lengths": False, "pad_to": 64}):
        other, gother = _model_run(name, tmp_path, **kw)
        assert torch.equal(other["loss"], base["loss"]) and torch.equal(other["prob"], base["prob"]), kw
        assert gother.keys() == gbase.keys()
        for k in gbase:
            assert torch.equal(gother[k], gbase[k]), (kw, k)


def test_generator_check_round_trip():
    from oracle import gen_golden
    if not os.path.isdir(os.path.join(gen_golden.REF, "DIEN")):
        pytest.skip("the reference folder is not on this machine")
    r = subprocess.run([sys.executable, os.path.join(ROOT, "scripts", "gen_golden_dien.py"), "--check"], cwd=ROOT,
                       capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout + r.stderr
    assert all(f"{n}.npz  checked" in r.stdout for n in GOLDENS)


# ---- the mirror on the launch-free registration pass ------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(GOLDENS))
def test_mirror_variables_on_the_registration_pass(name, tmp_path):
    from recalgorithm_amd.estimator import Estimator, ModeKeys, RunConfig
    vocab_dir = GU.write_vocab_dir(str(tmp_path / "vocabulary"))
    model_fn, params = mirror_setup(name, vocab_dir)
    d = GU.load(name)
    sfeats, labels = GU.string_batch()
    feats = {k: (v.float() if isinstance(v, torch.Tensor) else v) for k, v in sfeats.items()}
    lab = {"read_comment": labels.float()}
    est = Estimator(model_fn, params, RunConfig(device="cpu", seed=3, use_hip_graph=False))
    est.build(feats, lab)                    # registration pass only: no HIP call
    arrays = est.store.named_arrays()
    gv = GU.section(d, "var/")
    assert not [k for k in gv if k not in arrays and "dice_bn" not in k], "reference variables absent from the mirror"
    gv = {k: v for k, v in gv.items() if "dice_bn" not in k}      # (never-updated constants (0, 1): see CASE)
    assert not [k for k in arrays if k not in gv], "mirror variables the reference does not have"
    for k, v in gv.items():
        assert tuple(arrays[k].shape) == tuple(v.shape), (k, arrays[k].shape, v.shape)
    shared = [k for k in arrays if "shared_embedding" in k]
    assert shared == ["target_input/sequence_input_layer/feedid_his_read_comment_7d_seq_his_read_comment_7d_seq_shared_embedding/"
                      "embedding_weights"], "ONE table for three columns, two of them over the same key"
    for k, v in arrays.items():
        if k.endswith("gates/bias"):
            assert bool((v == 1).all()), k
        elif k.endswith("candidate/bias"):
            assert bool((v == 0).all()), k
    w = arrays["seq_encoder/attention_project_matrix"]
    assert 0 < float(w.abs().max()) <= (6.0 / (8 + 16)) ** 0.5                                  # glorot-uniform
    est.store.building = True
    try:
        with torch.no_grad():
            pred = est._call_model_fn(feats, None, ModeKeys.PREDICT)
            ev = est._call_model_fn(feats, lab, ModeKeys.EVAL)
            tr = est._call_model_fn(feats, lab, ModeKeys.TRAIN)
    finally:
        est.store.building = False
    assert list(pred.predictions) == ["probabilities"] and tuple(pred.predictions["probabilities"].shape) == (48, 1)
    assert sorted(ev.eval_metric_ops) == ["eval_accuracy", "eval_auc"]
    from recalgorithm_amd.estimator import LazyAdamOptimizer
    assert type(tr.train_op.optimizer) is LazyAdamOptimizer                                     # dien.py:328


REFERENCE_FLAGS = re.compile(r'flags\.DEFINE_(string|integer|float|boolean)\(\s*"(\w+)",\s*("[^"]*"|[-\w.]+),\s*((?:"[^"]*"\s*)+)\)')


def test_flags_against_the_reference_text_and_the_call_surface():
    """Every flag of the reference's dien.py:24-53 with its kind, default and help text (read from the reference's text where
    that folder exists, else from the copy of its defaults below), plus --sequence_max_length; checked in a child process: a
    model script imported earlier in this one defines flags of the same names."""
    expected = {"model_dir": "./model_dir", "output_dir": "./output_dir", "num_epochs": 1, "train_steps": 10000,
                "shuffle_buffer_size": 10000, "num_parallel_readers": -1, "save_checkpoints_steps": 1000, "batch_size": 1024,
                "learning_rate": 0.005, "hidden_units": "512,256,128", "batch_norm": True, "dropout_rate": 0.1, "activation": "dice",
                "use_auxiliary_loss": False, "negative_sample_number": 3, "custom_gru_type": "AGRU", "gru_output_units": 8}
    helps = {}
    ref = "/root/reference/algorithm/DIEN/dien.py"
    if os.path.exists(ref):
        text = re.sub(r"^\s*#.*$", "", open(ref, encoding="utf-8").read(), flags=re.M)
        found = {m.group(2): m for m in REFERENCE_FLAGS.finditer(text)}
        assert len(found) == 20 and set(expected) <= set(found)
        for k, m in found.items():
            helps[k] = "".join(re.findall(r'"([^"]*)"', m.group(4)))
            if k in expected:
                raw = m.group(3)
                val = raw.strip('"') if m.group(1) == "string" else {"True": True, "False": False}.get(raw, None)
                val = val if val is not None else (float(raw) if m.group(1) == "float" else int(raw))
                assert val == expected[k], (k, val)
    code = ("import json; from recalgorithm_amd import flags; from recalgorithm_amd.algorithm.DIEN import dien as m, custom_grucell as c, rnn as r; "
            "F = m.FLAGS; helps = {a.dest: a.help for a in flags.FLAGS._parser._actions}; "
            "print(json.dumps({k: getattr(F, k) for k in %r + ['sequence_max_length']})); "
            "print(json.dumps({k: helps[k] for k in %r})); "
            "print(all(callable(getattr(m, n)) for n in ('create_feature_columns', 'example_parser', 'dien_model_fn', 'main')), "
            "len(m.create_feature_columns()), c.AGRUCell(8).state_size, c.AUGRUCell(8).output_size, callable(r.dynamic_rnn), "
            "list(__import__('inspect').signature(r.dynamic_rnn).parameters))") % (sorted(expected), sorted(helps))
    env = dict(os.environ, PYTHONPATH=ROOT + os.pathsep + os.environ.get("PYTHONPATH", ""))
    out = subprocess.run([sys.executable, "-c", code], cwd=ROOT, env=env, capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stderr[-2000:]
    lines = out.stdout.strip().splitlines()
    import json
    got = json.loads(lines[-3])
    assert got.pop("sequence_max_length") == 0 and got == expected
    got_help = json.loads(lines[-2])
    for k, h in got_help.items():
        assert h == helps[k], (k, h, helps[k])
    assert lines[-1] == "True 6 8 8 True ['cell', 'inputs', 'att_scores', 'sequence_length', 'dtype']"


def test_what_the_mirror_refuses(tmp_path):
    from recalgorithm_amd.estimator import Estimator, RunConfig
    vocab_dir = GU.write_vocab_dir(str(tmp_path / "vocabulary"))
    sfeats, labels = GU.string_batch()
    feats = {k: (v.float() if isinstance(v, torch.Tensor) else v) for k, v in sfeats.items()}

    def build(**extra):
        model_fn, params = mirror_setup("model_dien", vocab_dir, **extra)
        Estimator(model_fn, params, RunConfig(device="cpu", seed=3, use_hip_graph=False)).build(feats, {"read_comment": labels.float()})
    with pytest.raises(NotImplementedError, match=r"dien\.py:259-265"):
        build(use_auxiliary_loss=True)
    with pytest.raises(ValueError, match=r"1 <= T <= 64.*there is no fallback"):
        build(gru_output_units=6)
    with pytest.raises(ValueError, match=r"1 <= T <= 64.*there is no fallback"):
        build(sequence_max_length=65)
    with pytest.raises(ValueError, match="custom_gru_type"):
        build(custom_gru_type="GRU")
    build(sequence_max_length=50)


# ---- three LazyAdam steps: the trajectory the GPU test compares against -----------------------------------------------------------
def lazy_adam_setup(name, tmp_path, **extra):
    """-> (model_fn, params, start variables rounded to float32, [(string features, labels)] x 3, lr): the three 32-of-48
    sub-batches of tests/trajectory_ref.py, alphas moved off 1 as there."""
    from tests import trajectory_ref as TR
    vocab_dir = GU.write_vocab_dir(str(tmp_path / "vocabulary"))
    model_fn, params = mirror_setup(name, vocab_dir, **extra)
    d = GU.load(name)
    sfeats, labels = GU.string_batch()
    batches = [TR.cut(sfeats, labels, idx) for idx in TR.batch_indices()]
    start = {k: torch.from_numpy(v.copy()).float().double() for k, v in GU.section(d, "var/").items()}
    g = torch.Generator().manual_seed(99)
    for k in sorted(start):
        if "alpha" in k:
            start[k] = (0.25 + 0.5 * torch.rand(start[k].shape, generator=g)).float().double()
    return model_fn, params, start, batches, float(d["meta/learning_rate"])


def oracle_batches(params, batches):
    return [(encode(params, sf), {"read_comment": lb}) for sf, lb in batches]


def test_three_lazy_adam_steps_differ_from_dense_adam(tmp_path):
    """A feed row that step 1 touches and step 2 does not: LazyAdam leaves it (and its moments) alone in step 2, dense Adam
    moves it by its decaying first moment."""
    _, params, start, batches, lr = lazy_adam_setup("model_dien", tmp_path)
    ob = oracle_batches(params, batches)
    lazy, dense = (R.lazy_adam_trajectory(start, ob[:n], params, lr, lazy=flag) for n, flag in ((3, True), (3, False)))
    table = next(k for k in start if "shared_embedding" in k)
    t1, t2 = (set(lazy["touched"][i][table].tolist()) for i in (0, 1))
    rows = sorted(t1 - t2)
    assert rows, "no feed row is touched in step 1 and not in step 2"
    one, two = (R.lazy_adam_trajectory(start, ob[:n], params, lr)["final"][table] for n in (1, 2))
    r = torch.tensor(rows)
    assert bool((one[r] != start[table][r]).any(dim=1).all()), "step 1 moved the rows it touched"
    assert torch.equal(two[r], one[r]), "LazyAdam left them alone in step 2"
    dense2 = R.lazy_adam_trajectory(start, ob[:2], params, lr, lazy=False)["final"][table]
    assert bool((dense2[r] != one[r]).any(dim=1).all()), "dense Adam moved them"
    assert not torch.equal(lazy["final"][table], dense["final"][table])
    never = sorted(set(range(start[table].shape[0])) - set().union(*(set(t[table].tolist()) for t in lazy["touched"])))
    assert torch.equal(lazy["final"][table][never], start[table][never])
    # the dense variables see the same optimizer; they differ only through the tables
    assert torch.equal(R.lazy_adam_trajectory(start, ob[:1], params, lr)["final"]["seq_encoder/fcn/dense/kernel"],
                       R.lazy_adam_trajectory(start, ob[:1], params, lr, lazy=False)["final"]["seq_encoder/fcn/dense/kernel"])
