"""-m gpu: the MI355X path (mirrored layer functions and model_fns -> C-ABI -> HIP kernels) against
the golden vectors produced by running the reference's OWN sources on oracle/tf1_shim
(oracle/gen_golden.py; float64).  Tolerance: north_star's 1e-5 relative (tests/util.py)."""
import numpy as np
import pytest
import torch

from recalgorithm_amd.variables import VariableStore, use_store, variable_scope
from tests import golden_util as GU
from tests.golden_protocol import GoldenCase, check_on_device
from tests.util import assert_close

pytestmark = pytest.mark.gpu


def _layer(dev, name, fn, scope=None, var_names=None):
    """fn(inputs on device) -> out; run once to create the variables, load the golden values,
    run again, back-propagate the golden upstream gradient, compare everything."""
    d = GU.load(name)
    ins = {}
    for k, v in GU.section(d, "in/").items():
        t = torch.from_numpy(v.copy())
        t = t.float().to(dev).requires_grad_(True) if t.is_floating_point() else t.to(dev)
        ins[k] = t
    store = VariableStore(dev, seed=1)

    def call():
        store.begin_call()
        if scope:
            with variable_scope(scope):
                return fn(ins)
        return fn(ins)
    with use_store(store):
        with torch.no_grad():
            call()
        gv = GU.section(d, "var/")
        for vn, val in gv.items():
            if "dice_bn" in vn:
                continue            # Dice's never-updated BN statistics (0, 1) are constants of the kernel
            v = store.vars[vn]
            v.data.copy_(torch.from_numpy(val).float().reshape(v.data.shape))
        out = call()
    assert_close(out, torch.from_numpy(d["out"]), what=f"{name} out")
    out.backward(torch.from_numpy(d["G"]).float().to(dev))
    from recalgorithm_amd import nn as _nn
    _nn.apply_parked_grads()          # deferred sums (weight-gradient splits, CrossNet's partial rows): what the optimizer does
    for k, g in GU.section(d, "grad_in/").items():
        assert_close(ins[k].grad, torch.from_numpy(g), what=f"{name} d(in {k})", reduced=True)
    for vn, g in GU.section(d, "grad_var/").items():
        if "dice_bn" in vn:
            continue
        sib = vn.replace("/bias", "/kernel")
        gsec = GU.section(d, "grad_var/")
        # f3_att/bias = sum_t ds_t is exactly 0 under softmax: judged at its sibling kernel's scale
        floor = 1e-5 * float(np.abs(gsec[sib]).max()) if vn.endswith("/bias") and sib in gsec else 0.0
        assert_close(store.vars[vn].grad, torch.from_numpy(g), what=f"{name} d(var {vn})", reduced=True, floor=floor)


def test_cross_layer_golden(dev):
    from recalgorithm_amd.algorithm.DCN.cross_layer import cross_layer, cross_network

    def stack(i):                       # the reference's loop, layer by layer (dcn.py:157-160)
        xl = i["x0"]
        for l in range(3):
            xl = cross_layer(x0=i["x0"], xl=xl, index=l)
        return xl
    _layer(dev, "layer_cross_stack", stack, scope="cross_part")
    _layer(dev, "layer_cross_single", lambda i: cross_layer(i["x0"], i["xl"], 7))


def test_cross_network_fused_golden(dev):
    """The fused L-layer kernel against the same golden (variables wl_i / bl_i live in one block)."""
    from recalgorithm_amd.algorithm.DCN.cross_layer import cross_network
    _layer(dev, "layer_cross_stack", lambda i: cross_network(i["x0"], 3), scope="cross_part")


def test_cin_layer_golden(dev):
    from recalgorithm_amd.algorithm.xDeepFM.cin_layer import cin_layer, cin_network

    def stack(i):
        _, p_plus = cin_network(i["x0"], ["6", "5"])
        return p_plus
    _layer(dev, "layer_cin_stack", stack, scope="cin_part")
    _layer(dev, "layer_cin_single", lambda i: cin_layer(i["x0"], i["xk"], 4, 3))


@pytest.mark.parametrize("branch", ["default", "softmax"])
def test_din_attention_golden(dev, branch):
    from recalgorithm_amd.algorithm.DIN.din_attention import din_attention
    _layer(dev, f"layer_din_attention_{branch}",
           lambda i: din_attention(i["query"], i["keys"], i["keys_length"], is_softmax=(branch == "softmax")),
           scope="attention_part")


def test_activations_golden(dev):
    from recalgorithm_amd.algorithm.DIN.activations import dice, prelu
    _layer(dev, "layer_prelu", lambda i: prelu(i["x"], name=1))
    _layer(dev, "layer_dice", lambda i: dice(i["x"], name=1))


def test_fibinet_layers_golden(dev):
    from recalgorithm_amd.algorithm.FiBiNET.bilinear_interaction_layer import bilinear_interaction_layer
    from recalgorithm_amd.algorithm.FiBiNET.senet import senet
    _layer(dev, "layer_senet", lambda i: senet(i["input"], 8, 2), scope="senet_part")
    for ty in ("all", "each", "interaction"):
        _layer(dev, f"layer_bilinear_{ty}", lambda i, ty=ty: bilinear_interaction_layer(i["input"], 8, ty, "orginal"),
               scope="bilinear_interaction_part")
    with pytest.raises(ValueError):
        with use_store(VariableStore(dev)):
            bilinear_interaction_layer(torch.zeros(2, 5, 8, device=dev), 8, "bogus", "x")


def suite_case(name):
    """The golden-parity case of the original suite (GU.MODELS), with the looseness it has always had: golden names are
    translated (DeepFM's first-order kernel, one slice per column), Dice's never-updated BN statistics are constants of the
    kernel and CrossNet's wl / bl live in one block, so those names may differ; gradients and updates the mirror does not
    report are passed over; PREDICT compares whatever the golden's predict/ section holds; the goldens hold no gradient count
    and no EVAL section."""
    from oracle import ref_models as M
    from tests.test_oracle_golden import _encode
    picked = {}

    def setup(name, vocab_dir):
        model_fn, params, picked["oracle"] = GU.mirror_setup(name, vocab_dir)
        return model_fn, params

    def oracle(*args, **kw):
        return getattr(M, picked["oracle"])(*args, **kw)
    return GoldenCase(mirror_setup=setup, oracle=oracle, encode=_encode, translate=GU.golden_to_oracle_vars,
                      golden_only=r"dice_bn", mirror_only=r"/(wl|bl)$", skip_absent=True, eval=False)


@pytest.mark.parametrize("name", GU.MODELS)
def test_model_golden(dev, name, tmp_path):
    check_on_device(dev, suite_case(name), name, tmp_path)
