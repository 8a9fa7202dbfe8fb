"""CPU (no kernels launched): the PLE feature's host side.
  * tests/ple_ref.py (the float64 restatement the GPU tests compare against) reproduces both goldens that
    scripts/gen_golden_ple.py obtained by executing the reference's own algorithm/PLE/ple.py on oracle/tf1_shim;
  * the generator's --check round trip (where the reference folder exists);
  * the CGC backward formulas as written in include/recalgo_cgc.h (summed mode: ONE upstream gradient shared by every
    gate, E dot products per row), against float64 autograd;
  * the mirror's variables, and the multi-task tail's PREDICT / EVAL keys, on the launch-free registration pass;
  * the limits of ops.cgc_mix / ops.cgc_supported;
  * include/recalgo_cgc.h, the second ABI header: its names, signatures, launches and constants, literally, and the constants
    re-exported (the checks every header gets, its record in include/recalgo_cgc.abi among them: tests/test_abi.py)."""
import ctypes
import os
import re
import subprocess
import sys

import pytest
import torch

from tests import golden_util as GU
from tests import ple_ref
from tests.golden_protocol import close, restate_on_host
from tests.test_mmoe_host import check_registration_pass, multitask_case

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "recalgo_cgc.h")
GOLDENS = {"model_ple": 76, "model_ple_two_levels_dropout": 96}        # name -> gradient arrays


def mirror_setup(name, vocab_dir):
    """(model_fn, params) of the mirror for golden `name`, from the mirror's own create_feature_columns()."""
    from recalgorithm_amd import flags
    from recalgorithm_amd.algorithm.PLE import ple as m
    d = GU.load(name)
    fl = {k: (v.item() if v.shape == () else v) for k, v in GU.section(d, "flag/").items()}
    flags.FLAGS.vocabulary_dir = vocab_dir
    for k, v in fl.items():
        setattr(flags.FLAGS, k, v)
    dense, cat, label = m.create_feature_columns()
    assert [c.key for c in label] == str(fl["task_names"]).split(",")
    return m.ple_model_fn, {
        "dense_feature_columns": dense, "category_feature_columns": cat, "hidden_units": str(fl["hidden_units"]).split(","),
        "dropout_rate": float(fl["dropout_rate"]), "batch_norm": bool(fl["batch_norm"]), "learning_rate": float(fl["learning_rate"]),
        "num_tasks": int(fl["num_tasks"]), "expert_hidden_units": int(fl["expert_hidden_units"]),
        "task_names": str(fl["task_names"]).split(","), "num_extract_network": int(fl["num_extract_network"]),
        "num_experts_per_task": [int(x) for x in str(fl["num_experts_per_task"]).split(",")],
        "num_experts_in_shared": int(fl["num_experts_in_shared"])}


CASE = multitask_case(mirror_setup, ple_ref.ple, GOLDENS)


@pytest.mark.parametrize("name", list(GOLDENS))
def test_restatement_reproduces_the_golden(name, tmp_path):
    _, params = mirror_setup(name, GU.write_vocab_dir(str(tmp_path / "vocabulary")))
    assert params["num_experts_per_task"] == [2, 1, 3] and params["num_experts_in_shared"] == 2
    restate_on_host(CASE, name, tmp_path)


def test_generator_check_round_trip():
    from oracle import gen_golden
    if not os.path.isdir(os.path.join(gen_golden.REF, "PLE")):
        pytest.skip("the reference folder is not on this machine")
    r = subprocess.run([sys.executable, os.path.join(ROOT, "scripts", "gen_golden_ple.py"), "--check"], cwd=ROOT,
                       capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "model_ple.npz  checked" in r.stdout and "model_ple_two_levels_dropout.npz  checked" in r.stdout


def cgc_summed_backward_formulas(x, ws, experts, selection, p_rows, d, relu_experts=False):
    """The summed-mode backward of include/recalgo_cgc.h, written out (float64): every gate shares the ONE upstream d, so
        dot[e] = <d, expert_e>                       E dot products per row, not sum n_g
        d_expert_e = (sum_g c[g][e]) * d             c[g][e] = sum_{j: sel[g][j] = e} p_g[j]  (zeroed where expert_e <= 0 if relu)
        dp_g[j] = dot[sel[g][j]];  dz_g = p_g * (dp_g - sum_j p_g[j] dp_g[j]);  dx = sum_g dz_g Wg^T;  dWg = x^T dz_g"""
    E = len(experts)
    dot = torch.stack([(d * e).sum(dim=1) for e in experts], dim=1)              # [B, E]
    ctot = torch.zeros(x.shape[0], E, dtype=x.dtype)
    dx, dws = torch.zeros_like(x), []
    for w, sel, p in zip(ws, selection, p_rows):
        for j, e in enumerate(sel):
            ctot[:, e] += p[:, j]
        dp = dot[:, sel]
        dz = p * (dp - (p * dp).sum(dim=1, keepdim=True))
        dx += dz @ w.t()
        dws.append(x.t() @ dz)
    dex = [ctot[:, e:e + 1] * d for e in range(E)]
    if relu_experts:
        dex = [g * (e > 0) for g, e in zip(dex, experts)]
    return dx, dws, dex


@pytest.mark.parametrize("shape", [(29, 7, 6, 4, 8, ple_ref.ple_selection([2, 1, 1], 2, all_gate=True)),
                                   (11, 4, 2, 2, 4, [[1, 1, 0], [0]])])
def test_cgc_summed_backward_formulas_against_autograd(shape):
    B, In, E, G, H, selection = shape
    assert len(selection) == G and max(e for s in selection for e in s) == E - 1
    gen = torch.Generator().manual_seed(B * 131 + H)
    x = torch.randn(B, In, generator=gen, dtype=torch.float64, requires_grad=True)
    ws = [torch.randn(In, len(s), generator=gen, dtype=torch.float64, requires_grad=True) for s in selection]
    experts = [torch.randn(B, H, generator=gen, dtype=torch.float64, requires_grad=True) for _ in range(E)]
    d = torch.randn(B, H, generator=gen, dtype=torch.float64)
    out, ps = ple_ref.cgc(x, ws, experts, selection, sum_outputs=True)
    per_gate, _ = ple_ref.cgc(x, ws, experts, selection)
    close(out, sum(per_gate).detach(), "the summed output is the sum of the per-gate outputs", tol=1e-14)
    grads = torch.autograd.grad((out * d).sum(), [x, *ws, *experts])
    with torch.no_grad():
        dx, dws, dex = cgc_summed_backward_formulas(x, ws, experts, selection, ps, d)
    close(dx, grads[0], "dx", tol=1e-12)
    for g, (a, b) in enumerate(zip(dws, grads[1:1 + G])):
        close(a, b, f"dW{g}", tol=1e-12)
    for e, (a, b) in enumerate(zip(dex, grads[1 + G:])):
        close(a, b, f"d_expert{e}", tol=1e-12)
    # experts that are ReLU outputs: the masked form is the gradient at the pre-activation
    pre = [torch.randn(B, H, generator=gen, dtype=torch.float64, requires_grad=True) for _ in range(E)]
    relu = [torch.relu(t) for t in pre]
    out, ps = ple_ref.cgc(x, ws, relu, selection, sum_outputs=True)
    gpre = torch.autograd.grad((out * d).sum(), pre)
    with torch.no_grad():
        _, _, dex = cgc_summed_backward_formulas(x, ws, [t.detach() for t in relu], selection, ps, d, relu_experts=True)
    for e, (a, b) in enumerate(zip(dex, gpre)):
        close(a, b, f"d_expert{e} (relu)", tol=1e-12)


@pytest.mark.parametrize("name", list(GOLDENS))
def test_mirror_variables_and_tail_keys_on_the_registration_pass(name, tmp_path):
    check_registration_pass(CASE, name, tmp_path)


def test_reference_flag_defaults_and_call_surface():
    """ple.py:21-50 (checked in a child process: a model script imported earlier in this one defines flags of the same names)"""
    code = ("from recalgorithm_amd.algorithm.PLE import ple as m; from recalgorithm_amd.algorithm.PLE.extraction_network import "
            "extraction_network; F = m.FLAGS; print(F.batch_size, F.learning_rate, F.hidden_units, F.batch_norm, F.dropout_rate, "
            "F.num_extract_network, F.num_experts_per_task, F.num_experts_in_shared, F.expert_hidden_units, F.num_tasks, "
            "F.task_names); print(all(callable(getattr(m, n)) for n in ('create_feature_columns', 'example_parser', "
            "'ple_model_fn', 'main')), callable(m.example_parser.columns_getter), "
            "extraction_network.__code__.co_varnames[:6])")
    env = dict(os.environ, PYTHONPATH=ROOT + os.pathsep + os.environ.get("PYTHONPATH", ""))
    r = subprocess.run([sys.executable, "-c", code], cwd=ROOT, env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = r.stdout.strip().splitlines()
    assert lines[-2] == "1024 0.005 512,256,128 True 0.1 1 5,5,5 10 256 3 read_comment,like,click_avatar"
    assert lines[-1] == ("True True ('input', 'task_names', 'num_experts_per_task', 'num_experts_in_shared', "
                         "'expert_hidden_units', 'name')")


def test_limits():
    """the limits include/recalgo_cgc.h states (the entry points check them again; this needs the built library, not a GPU:
    built here if stale, as tests/test_abi.py does)"""
    from recalgorithm_amd import build, ops
    build.build(verbose=False)
    assert ops.cgc_supported(82, 25, 4, 256, 70, 25)             # the default extraction network
    assert ops.cgc_supported(256, 25, 3, 256, 45, 15)            # the default final CGC
    assert ops.cgc_supported(82, 7, 4, 12, 22, 8) and ops.cgc_supported(12, 7, 3, 12, 14, 5)     # the golden shapes
    assert ops.cgc_supported(512, 32, 8, 1028, 39, 32)           # 512 * 39 floats: under the 80 KiB
    assert not ops.cgc_supported(82, 25, 4, 254, 70, 25)         # H % 4
    assert not ops.cgc_supported(82, 33, 4, 256, 70, 25)         # E = 33
    assert not ops.cgc_supported(82, 25, 9, 256, 70, 25)         # G = 9
    assert not ops.cgc_supported(513, 25, 4, 256, 30, 25)        # In = 513
    assert not ops.cgc_supported(82, 25, 4, 256, 70, 33)         # a gate over 33 experts
    assert not ops.cgc_supported(512, 25, 4, 256, 41, 25)        # 512 * 41 floats > 20 480
    assert ops.CGC_MAX_EXPERTS == 32 and ops.CGC_MAX_GATES == 8
    x, e = torch.zeros(4, 82), [torch.zeros(4, 8) for _ in range(3)]
    w = [torch.zeros(82, 3)]
    with pytest.raises(NotImplementedError, match="H % 4 == 0, E <= 32, G <= 8, n_g <= 32, In <= 512"):
        ops.cgc_mix(x, w, [torch.zeros(4, 6) for _ in range(3)], [[0, 1, 2]])
    with pytest.raises(NotImplementedError):
        ops.cgc_mix(x, [torch.zeros(82, 1)] * 9, e, [[0]] * 9)                                   # G = 9
    with pytest.raises(NotImplementedError):
        ops.cgc_mix(x, [torch.zeros(82, 33)], [torch.zeros(4, 8) for _ in range(33)], [list(range(33))])       # E = 33
    with pytest.raises(NotImplementedError, match="empty batch"):
        ops.cgc_mix(torch.zeros(0, 82), w, [torch.zeros(0, 8) for _ in range(3)], [[0, 1, 2]])
    with pytest.raises(ValueError):
        ops.cgc_mix(x, [torch.zeros(82, 0)], e, [[]])                                            # a gate over no expert
    with pytest.raises(ValueError):
        ops.cgc_mix(x, w, e, [[0, 1, 3]])                                                        # an index past E
    with pytest.raises(ValueError):
        ops.cgc_mix(x, w, e, [[0, 1]])                                                           # kernel width != n_g
    with pytest.raises(ValueError):
        ops.cgc_mix(x, w, e, [[0, 1, 2], [0]])                                                   # a row without a kernel
    with pytest.raises(ValueError):
        ops.cgc_mix(x, w, e[:2] + [torch.zeros(4, 12)], [[0, 1, 2]])                             # experts of two widths


# ---- include/recalgo_cgc.h: what this feature expects of its header, literally (every generic check: tests/test_abi.py) --------
def test_second_header_literal_expectations():
    from recalgorithm_amd import _lib, build, ops
    build.build(verbose=False)
    abi = _lib.HEADERS["recalgo_cgc.h"]
    assert sorted(abi.functions) == sorted(["recalgo_cgc_abi_version", "recalgo_cgc_supported", "recalgo_cgc_partial_rows",
                                            "recalgo_cgc_fwd", "recalgo_cgc_bwd"])
    assert abi.launches == ["recalgo_cgc_fwd", "recalgo_cgc_bwd"]
    assert not abi.structs
    lib = _lib.load()
    assert lib.recalgo_cgc_abi_version() == abi.version == 1
    c_int, ptr = ctypes.c_int, ctypes.c_void_p
    assert abi.functions["recalgo_cgc_abi_version"] == (c_int, [])
    assert abi.functions["recalgo_cgc_supported"] == (c_int, [c_int] * 6)
    assert abi.functions["recalgo_cgc_partial_rows"] == (c_int, [c_int] * 3)
    assert abi.functions["recalgo_cgc_fwd"] == (c_int, [ptr, c_int, ptr, ptr, ptr, ptr] + [c_int] * 6 + [ptr, ptr, ptr])
    assert abi.functions["recalgo_cgc_bwd"] == (
        c_int, [ptr, c_int, ptr, ptr, ptr, ptr, ptr, ptr] + [c_int] * 7 + [ptr, ptr, c_int, ptr, ptr])
    # a launch that returns an error raises through the errcheck (NULL tables: refused before any launch)
    with pytest.raises(_lib.RecalgoError, match="recalgo_cgc_fwd failed with hipError_t=[1-9]"):
        lib.recalgo_cgc_fwd(None, 0, None, None, None, None, 1, 1, 1, 1, 4, 0, None, None, None)
    with pytest.raises(_lib.RecalgoError, match="recalgo_cgc_bwd failed with hipError_t=[1-9]"):
        lib.recalgo_cgc_bwd(None, 0, None, None, None, None, None, None, 1, 1, 1, 1, 4, 0, 0, None, None, 0, None, None)
    defines = {m.group(1): int(m.group(2)) for m in re.finditer(r"#define (RECALGO_CGC_\w+) (\d+)", open(HEADER).read())
               if not m.group(1).endswith("_H_")}
    assert abi.constants == defines == {"RECALGO_CGC_ABI_VERSION": 1, "RECALGO_CGC_MAX_EXPERTS": 32, "RECALGO_CGC_MAX_GATES": 8}
    assert ops.CGC_MAX_EXPERTS == defines["RECALGO_CGC_MAX_EXPERTS"] and ops.CGC_MAX_GATES == defines["RECALGO_CGC_MAX_GATES"]
