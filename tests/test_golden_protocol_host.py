"""CPU (no kernels launched): tests/golden_protocol.py's judge, the one statement of the golden-parity tolerance policy.
  * a producer that is the float64 oracle on the golden's variables passes it: the oracle reproduces the goldens at 1e-10, far
    inside every bound, the ref32 guard included;
  * one mutation of that producer's output at a time — a gradient element, a variable name, the gradient count, a prediction
    key, the masks, an Adam-updated element, a moving statistic, the eval loss, Wide&Deep's untouched buckets and FTRL slots —
    makes it raise an AssertionError that names the item.
The cases are the ones the GPU tests use (tests/test_gpu_*.py::test_model_golden), so a case's declared looseness shows here."""
import copy
import re

import pytest
import torch

from oracle import ref_ops as R
from tests import golden_protocol as GP
from tests import golden_util as GU
from tests import util
from tests import wdl_ref as W
from tests.test_bst_host import CASE as BST
from tests.test_gpu_golden import suite_case
from tests.test_gpu_wdl import GPU_CASE as WDL
from tests.test_mmoe_host import CASE as MMOE
from tests.test_ple_host import CASE as PLE
from tests.test_wdl_host import f32

CASES = {"model_ple": PLE, "model_mmoe_dropout": MMOE, "model_bst_two_blocks_mean_dropout": BST, "model_wdl": WDL,
         "model_deepfm": suite_case("model_deepfm"), "model_din_dice_dropout": suite_case("model_din_dice_dropout")}


def oracle_produce(case, name, tmp_path):
    """what produce_on_device returns, from the float64 oracle: its predictions, loss and gradients; one R.adam_tf1_step on its
    gradients (W.ftrl_dense for Wide&Deep's wide variables); its EVAL on var_after/.  The oracles do not return BatchNorm's
    batch moments, so the moving statistics' update is the golden's own."""
    _, params = case.mirror_setup(name, GU.write_vocab_dir(str(tmp_path / "vocabulary")))
    golden = GP.load_golden(case, name, params)
    run = GP.run_oracle(case, golden, torch.float64)
    P, gg = run["P"], golden.grad
    out = {"variables": [k for k in golden.var if not (case.golden_only and re.search(case.golden_only, k))], "extra": {},
           "predictions": {k: GP._path(run["predict"], path).detach() for k, path in case.prediction_paths(golden.d).items()},
           "masks_consumed": True, "loss": run["loss"].detach(), "grads": {k: run["grads"][k].detach() for k in gg},
           "before": {k: p.detach().clone() for k, p in P.items()}, "update": {}}
    wide = {}
    for k, va in golden.var_after.items():
        p = P[k].detach().clone()
        if k.startswith("wide_part/"):
            wide[k] = W.ftrl_dense(p, torch.full_like(p, f32(W.FTRL_INITIAL_ACCUMULATOR)), torch.zeros_like(p), run["grads"][k].detach(),
                                   f32(golden.d["meta/wide_part_learning_rate"]))
        elif k in gg and "moving_" not in k:
            R.adam_tf1_step(p, run["grads"][k].detach(), torch.zeros_like(p), torch.zeros_like(p), 1, golden.lr)
            out["update"][k] = p - P[k].detach()
        else:
            out["update"][k] = torch.from_numpy(va).reshape(p.shape) - p
    if wide:
        out["extra"] = {"wide_after": {k: v[0] for k, v in wide.items()},
                        "slots": {f"{k}/{s}": v[i] for k, v in wide.items() for i, s in ((1, "Ftrl"), (2, "Ftrl_1"))},
                        "wide_adam_moments": {k: 0.0 for k in wide}, "flat_grad": 0.0}
    if case.eval:
        out["eval_loss"], out["eval_metrics"] = GP.oracle_eval(case, golden, golden.var_after)
    return golden, out


@pytest.fixture(scope="module")
def runs(tmp_path_factory):
    """name -> (case, golden, produced, ref32), computed once and left unchanged; the judge's rows of these oracle runs are no
    parity rows of a kernel: the strict log is put back as it was"""
    n0, cache = len(util.STRICT_LOG), {}

    def get(name):
        if name not in cache:
            golden, produced = oracle_produce(CASES[name], name, tmp_path_factory.mktemp(name))
            cache[name] = (CASES[name], golden, produced, GP.restate32(CASES[name], golden))
        return cache[name]
    yield get
    del util.STRICT_LOG[n0:]


@pytest.mark.parametrize("name", list(CASES))
def test_the_float64_oracle_passes_the_judge(runs, name):
    case, golden, produced, ref32 = runs(name)
    assert len(golden.grad) >= 15 and produced["update"]
    GP.judge(case, golden, copy.deepcopy(produced), ref32)


def _largest_gradient(golden, produced):
    """(variable, flat index) of the largest gradient element of an Adam variable outside the embedding tables: far from the
    floors, and a well-conditioned element of the first Adam step"""
    ks = [k for k in golden.grad if "embedding_weights" not in k and not k.startswith("wide_part/") and k in produced["update"]]
    k = max(ks, key=lambda k: float(abs(golden.grad[k]).max()))
    return k, int(torch.from_numpy(golden.grad[k]).abs().reshape(-1).argmax())


# mutation -> (applies(case, golden), mutate(case, golden, produced) -> the item the AssertionError has to name)
def _scale_gradient(case, golden, p):
    k, i = _largest_gradient(golden, p)
    p["grads"][k] = p["grads"][k].clone()
    p["grads"][k].view(-1)[i] *= 1 + 1e-3
    return f"d({k})"


def _drop_variable(case, golden, p):
    return p["variables"].pop(0)


def _add_variable(case, golden, p):
    p["variables"].append("tower/one_more/kernel")
    return "tower/one_more/kernel"


def _drop_gradient(case, golden, p):
    k, _ = _largest_gradient(golden, p)
    del p["grads"][k]
    return k


def _rename_prediction(case, golden, p):
    k = next(iter(p["predictions"]))
    p["predictions"] = {(key + "_x" if key == k else key): v for key, v in p["predictions"].items()}
    return k


def _leave_a_mask(case, golden, p):
    p["masks_consumed"] = False
    return "dropout calls"


def _move_adam_element(case, golden, p):
    k, i = _largest_gradient(golden, p)
    p["update"][k] = p["update"][k].clone()
    p["update"][k].view(-1)[i] += 1e-3 * golden.lr
    return f"adam update {k}"


def _move_moving_statistic(case, golden, p):
    k = next(k for k in p["update"] if "moving_" in k)
    p["update"][k] = p["update"][k].clone()
    p["update"][k].view(-1)[0] += 1e-5
    return f"{k} update"


def _scale_eval_loss(case, golden, p):
    p["eval_loss"] = p["eval_loss"] * (1 + 1e-4)
    return "eval loss"


def _touch_an_untouched_bucket(case, golden, p):
    zero = torch.from_numpy(golden.var_after[W.WIDE_KERNEL] == 0).reshape(-1)
    kern = p["extra"]["wide_after"][W.WIDE_KERNEL].clone()
    kern.view(-1)[int(zero.nonzero()[0])] = 1e-30          # (below every tolerance: only the exact-zero check sees it)
    p["extra"]["wide_after"][W.WIDE_KERNEL] = kern
    return f"untouched bucket of {W.WIDE_KERNEL}"


def _move_ftrl_slot(case, golden, p):
    k = W.WIDE_KERNEL + "/Ftrl_1"
    p["extra"]["slots"][k] = p["extra"]["slots"][k].clone()
    i = int(p["extra"]["slots"][k].abs().reshape(-1).argmax())
    p["extra"]["slots"][k].view(-1)[i] *= 1 + 1e-3
    return k


def _has_moving(name):
    return any("moving_" in k for k in GU.section(GU.load(name), "var_after/"))


MUTATIONS = {
    "gradient element scaled by 1 + 1e-3": (lambda name: True, _scale_gradient),
    "variable missing": (lambda name: True, _drop_variable),
    "extra variable": (lambda name: True, _add_variable),
    "gradient array dropped": (lambda name: True, _drop_gradient),
    "prediction key renamed": (lambda name: True, _rename_prediction),
    "masks not all consumed": (lambda name: True, _leave_a_mask),
    "adam-updated element moved by 1e-3 lr": (lambda name: True, _move_adam_element),
    "moving statistic moved by 1e-5": (_has_moving, _move_moving_statistic),
    "eval loss scaled by 1 + 1e-4": (lambda name: CASES[name].eval, _scale_eval_loss),
    "untouched bucket not zero": (lambda name: CASES[name] is WDL, _touch_an_untouched_bucket),
    "ftrl slot element moved": (lambda name: CASES[name] is WDL, _move_ftrl_slot),
}


@pytest.mark.parametrize("name,mutation", [(n, m) for n in CASES for m, (applies, _) in MUTATIONS.items() if applies(n)])
def test_one_mutation_raises_and_names_the_item(runs, name, mutation):
    case, golden, produced, ref32 = runs(name)
    mutated = copy.deepcopy(produced)
    item = MUTATIONS[mutation][1](case, golden, mutated)
    if case.skip_absent and mutation == "gradient array dropped":
        # the original suite's declared looseness: a gradient the mirror does not report is passed over
        GP.judge(case, golden, mutated, ref32)
        return
    with pytest.raises(AssertionError, match=re.escape(item)):
        GP.judge(case, golden, mutated, ref32)


def test_the_chosen_goldens_cover_what_the_mutations_need():
    assert any(_has_moving(n) and CASES[n].skip_absent for n in CASES), "none of the original suite's goldens has BatchNorm"
    assert sum(_has_moving(n) for n in CASES) >= 4 and sum(bool(GU.dropout_masks(GU.load(n))) for n in CASES) >= 3
