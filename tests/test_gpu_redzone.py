"""-m gpu: the kernel-level parity tests once more, with every device allocation fenced and poisoned (tests/redzone.py).

The parity tests compare what a kernel wrote where it should; this run catches what a kernel does OUTSIDE those elements:
stores before or behind an output / gradient / partial-row buffer / workspace, a `*_workspace_bytes` query that is short
(the guarded workspace is exactly as large as the query said, not the pool's 1 MiB), output elements nobody wrote (the
allocation is NaN, not the previous arm's freed and already correct output), a ticket or counter assumed zero in
`torch.empty` scratch, and float reads past the end of an input.  No reference is restated here: the existing tests are
plain functions of (dev, *params); they are imported and called inside `guarded()` with their own parametrisations and
their own assertions.

CASES is every case of each test's own parametrize marks: the ragged shapes (last tile partly filled in every tiled
dimension) and the BASELINE ones, where the workspaces are large.  The whole file costs about as much as the tests it
re-runs, a few per cent of the GPU suite, so nothing is trimmed.  A few cases run a second time as a variant, to reach
kernels the default host path does not: "atomic" (sparse.SCATTER_MODE, the float-atomic backward kernels) and "plain"
(PLAIN_ENTRIES: the C-ABI entries whose superset is all the host layer calls).

Not run under the guard, because they capture a hipGraph, run whole training steps through the Estimator, start child
processes or build multi-GB arenas: test_gpu_big_table.py, test_gpu_models.py, test_gpu_golden.py, test_gpu_bench.py,
test_gpu_config1_tfrecord.py, test_gpu_dist*.py, test_gpu_baseline_shapes.py, and the functions named in LEFT_OUT below.

No call site needed an allow-list entry: the guard reported nothing that turned out to be intended.

The last test asserts that every kernel-launching C-ABI entry ran under the guard; it needs the whole file to have run in
the same process (a `-k` selection of single cases makes it fail, naming what is missing)."""
import functools
import inspect
import itertools

import pytest
import torch

from recalgorithm_amd import _lib, nn, ops
from recalgorithm_amd.variables import Variable
from tests import (redzone, test_gpu_cin, test_gpu_dense, test_gpu_din, test_gpu_dispatch_arms, test_gpu_dist, test_gpu_dropout,
                   test_gpu_fibinet, test_gpu_kernels, test_gpu_mmoe, test_gpu_pnn, test_gpu_property, test_gpu_siblings,
                   test_gpu_sparse, test_gpu_tailfuse)
from tests.redzone import guarded
from tests.util import assert_close

pytestmark = pytest.mark.gpu

MODULES = [test_gpu_dense, test_gpu_kernels, test_gpu_tailfuse, test_gpu_dropout, test_gpu_sparse, test_gpu_cin, test_gpu_din,
           test_gpu_dispatch_arms, test_gpu_fibinet, test_gpu_pnn, test_gpu_siblings, test_gpu_mmoe, test_gpu_property]

LEFT_OUT = {
    "test_gpu_kernels.test_cpu_tensor_is_rejected": "no device work: the call is refused on the host",
    "test_gpu_dispatch_arms.test_concat_sumsq_ticket_graph_replay": "captures a hipGraph",
    "test_gpu_dispatch_arms.test_lds_grant_grows": "a child process",
    "test_gpu_dispatch_arms.test_lds_grant_second_device": "needs a second device: skips on a machine with one",
    "test_gpu_mmoe.test_gate_mix_is_deterministic_and_capturable": "captures a hipGraph",
    "test_gpu_mmoe.test_model_golden": "model level: whole Estimator steps",
    "test_gpu_mmoe.test_default_configuration_step_against_float64": "model level: whole Estimator steps",
    "test_gpu_mmoe.test_captured_run_equals_eager_bit_for_bit": "captures a hipGraph",
    "test_gpu_mmoe.test_abandoned_step_leaves_nothing_to_the_next": "model level: whole Estimator steps",
    "test_gpu_mmoe.test_serving_returns_the_three_probabilities": "model level: export and serving",
    "test_gpu_mmoe.test_main_trains_and_prints_the_six_metrics": "a child process",
    "test_gpu_dropout.test_model_with_hash_dropout_matches_the_oracle_on_the_same_masks": "model level: whole Estimator steps",
    "test_gpu_dropout.test_captured_step_with_dropout_equals_eager": "captures a hipGraph",
    "test_gpu_sparse.test_models_train_identically_on_the_owner_and_the_atomic_paths": "model level: whole Estimator steps",
}


def _expand(fn):
    """The kwargs of every case of `fn`'s own parametrize marks."""
    axes = []
    for m in getattr(fn, "pytestmark", []):
        if m.name != "parametrize":
            continue
        names = [n.strip() for n in m.args[0].split(",")] if isinstance(m.args[0], str) else list(m.args[0])
        vals = [getattr(v, "values", v) for v in m.args[1]]
        axes.append([dict(zip(names, v if len(names) > 1 else (v,))) for v in vals])
    return [functools.reduce(lambda a, b: {**a, **b}, combo, {}) for combo in itertools.product(*axes)]


def _collect():
    cases, ids = [], []
    for mod in MODULES:
        short = mod.__name__.rsplit(".", 1)[-1]
        for name, fn in vars(mod).items():
            if not (name.startswith("test_") and inspect.isfunction(fn)) or f"{short}.{name}" in LEFT_OUT:
                continue
            for kw in _expand(fn):
                cases.append((fn, kw))
                ids.append(f"{short[9:]}.{name[5:]}[{'-'.join(str(v).replace(' ', '') for v in kw.values())}]")
    return cases, ids


def _variant(variant, fn, kws):
    for kw in kws:
        assert kw in _expand(fn), (fn.__name__, kw)              # only cases the test itself is parametrised with
        yield (fn, kw, variant), f"{variant or inspect.getmodule(fn).__name__[15:]}:{fn.__name__[5:]}[{'-'.join(str(v).replace(' ', '') for v in kw.values())}]"


# C-ABI entries the host layer never calls because it always calls their superset (deferred-Adam views, a strided or joined
# gradient, plan scans); a C caller may call either.  Under the "plain" variant a superset call that asks for nothing beyond
# the plain entry runs the plain entry, and the existing test checks its result: {superset: (plain, args -> plain args | None)}
PLAIN_ENTRIES = {
    "recalgo_sequence_gather_fwd_deferred": ("recalgo_sequence_gather_fwd", lambda a: a[:8] + a[12:] if a[8] is None else None),
    "recalgo_deepfm_sparse_fwd_deferred": ("recalgo_deepfm_sparse_fwd",
                                           lambda a: a[:12] + a[16:] if a[12] is None and a[13] is None else None),
    "recalgo_din_attention_bwd_joined": ("recalgo_din_attention_bwd",
                                         lambda a: a[:10] + a[13:] if a[11] is None and a[10] == a[15] else None),
    "recalgo_adam_tf1_step_plans": ("recalgo_adam_tf1_step", lambda a: a[:15] + a[17:] if a[15] is None else None),
}


def _collect_all():
    cases, ids = _collect()
    cases = [(fn, kw, None) for fn, kw in cases]
    extra = [
        # recalgo_dedup_rows: a kernel-level test that lives in a file of distributed tests (no process group involved)
        *_variant(None, test_gpu_dist.test_dedup_rows_kernel_against_torch, _expand(test_gpu_dist.test_dedup_rows_kernel_against_torch)),
        # sparse.SCATTER_MODE = "atomic" (a module hook of sparse.py): the float-atomic backward kernels an arena outside the
        # owner-computes plan's domain still runs - recalgo_{embedding_gather, embedding_bag_mean, sequence_gather, deepfm_sparse}_bwd
        *_variant("atomic", test_gpu_kernels.test_gather_fwd_bit_exact_and_bwd, [dict(B=1, vocabs=[5], K=16), dict(B=37, vocabs=[11, 2, 301], K=8)]),
        *_variant("atomic", test_gpu_kernels.test_bag_mean, _expand(test_gpu_kernels.test_bag_mean)),
        *_variant("atomic", test_gpu_kernels.test_sequence_gather, _expand(test_gpu_kernels.test_sequence_gather)),
        *_variant("atomic", test_gpu_kernels.test_deepfm_sparse, [dict(B=3, F=2, K=4), dict(B=130, F=6, K=8)]),
        *_variant("plain", test_gpu_kernels.test_sequence_gather, _expand(test_gpu_kernels.test_sequence_gather)),
        *_variant("plain", test_gpu_kernels.test_deepfm_sparse, [dict(B=3, F=2, K=4), dict(B=130, F=6, K=8)]),
        *_variant("plain", test_gpu_din.test_din_attention, _expand(test_gpu_din.test_din_attention)),
        *_variant("plain", test_gpu_sparse.test_plan_prefix_from_the_optimizer_launch_equals_place_scanning_itself,
                  [dict(requests=(700, 9), nb_env=None)]),
    ]
    return cases + [c for c, _ in extra], ids + [i for _, i in extra]


CASES, IDS = _collect_all()
_ran = []


def _call(fn, dev, kw, g, monkeypatch, tmp_path=None):
    """fn(dev, **kw) with the fixtures it asks for; its module's input helpers place through the guard."""
    mod = inspect.getmodule(fn)
    # test_gpu_dispatch_arms (DIN, PNN, CIN, concat_sumsq): `_aligned` places inputs only, which must come back unchanged;
    # `_shifted` also places the gradient buffers a kernel accumulates into
    for helper, const in (("_aligned", True), ("_shifted", False)):
        if hasattr(mod, helper):
            monkeypatch.setattr(mod, helper, functools.partial(getattr(mod, helper), place=functools.partial(g.input, const=const)))
    want = inspect.signature(fn).parameters
    extra = {k: v for k, v in (("monkeypatch", monkeypatch), ("tmp_path", tmp_path)) if k in want}
    assert set(want) <= {"dev", *kw, *extra}, f"{fn.__name__} asks for a fixture this file does not pass on: {set(want)}"
    fn(dev, **kw, **extra)


def test_guard_sees_device_allocations_in_backward_and_host_copies(dev, monkeypatch):
    """The guard's premise, checked on the device: allocations made inside an autograd.Function.backward (which the
    autograd engine may run on a thread of its own for device work) go through the swapped factories, `.to(device)` copies
    are placed, and empty results are NaN.  If this fails the rest of the file would silently test less."""
    M, K, N = 65, 33, 65
    gen = torch.Generator().manual_seed(3)
    x, w, b, gy = (torch.randn(*s, generator=gen) for s in ((M, K), (K, N), (N,), (M, N)))
    w /= K ** 0.5
    with guarded() as g:
        e = torch.empty(7, 5, device=dev)
        assert e.data_ptr() % 16 == 0 and bool(torch.isnan(e).all()) and g.records[-1].kind == "empty"
        xd = g.input(x, dev).requires_grad_(True)
        wd = w.to(dev)
        assert g.records[-1].kind == "to" and wd.data_ptr() % 16 == 0 and torch.equal(wd.cpu(), w)
        kv, bv = Variable("k", wd), Variable("b", b.to(dev))
        y = nn._DenseFn.apply(None, xd, kv, bv, True)
        assert g.records_at("ops.py") and not any(r.in_backward for r in g.records)
        y.backward(gy.to(dev))
        ops.flush_dense_splits()
        seen = [r for r in g.records if r.in_backward and "ops.py" in r.site]
        assert seen, "no allocation of ops.py below a backward was intercepted: " + "; ".join(r.site for r in g.records)
        assert "recalgo_dense_fwd" in redzone.LAUNCHED and any(n.startswith("recalgo_dense_bwd") for n in redzone.LAUNCHED)
        ref = torch.relu(x.double() @ w.double() + b.double())
        g2 = gy.double() * (ref > 0)
        assert_close(y, ref, what="guarded dense fwd", reduced=True)
        assert_close(xd.grad, g2 @ w.double().t(), what="guarded dense dgrad", reduced=True)
        assert_close(kv.grad, x.double().t() @ g2, what="guarded dense wgrad", reduced=True)
        assert_close(bv.grad, g2.sum(0), what="guarded dense dbias", reduced=True)


@pytest.mark.parametrize("fn,kw,variant", CASES, ids=IDS)
def test_guarded(dev, fn, kw, variant, monkeypatch, tmp_path):
    if variant == "atomic":
        from recalgorithm_amd import sparse
        monkeypatch.setattr(sparse, "SCATTER_MODE", "atomic")
    with guarded(redirect=PLAIN_ENTRIES if variant == "plain" else None) as g:
        _call(fn, dev, kw, g, monkeypatch, tmp_path)
    if variant == "plain":
        assert g.launched & {plain for plain, _ in PLAIN_ENTRIES.values()}, f"no plain entry ran: {sorted(g.launched)}"
    _ran.append(fn)


# Two arms, one after the other, on the same inputs: without the guard the second arm's `torch.empty` output can be the first
# arm's freed, already correct output, and a kernel that skips its last partial tile still passes.  Under the guard the
# buffer each arm receives was all 0xFF when it was handed out (`poisoned`, evaluated on the stream before the launch).
TWO_ARMS = [
    (test_gpu_dispatch_arms.test_din_generic_arm, dict(B=19, T=7, shift="both", flat_grads=True, is_softmax=False),
     ("ops.py", "in forward"), 2),
    (test_gpu_dispatch_arms.test_ipnn_features_bwd_general_arm, dict(B=21, F=13, K=8, shift="d_emb"),
     ("test_gpu_dispatch_arms.py", "in test_ipnn_features_bwd_general_arm"), 2),
    (test_gpu_dense.test_dense_merged_bwd_is_bit_identical_to_the_two_launches, dict(M=300, K=82, N=50),
     ("ops.py", "in dense_bwd"), 2),
]


@pytest.mark.parametrize("fn,kw,where,least", TWO_ARMS, ids=[t[0].__name__[5:] for t in TWO_ARMS])
def test_second_arm_output_is_the_guards_not_the_pools(dev, fn, kw, where, least, monkeypatch):
    assert kw in _expand(fn)
    with guarded(audit=True) as g:
        _call(fn, dev, kw, g, monkeypatch)
        outs = [r for r in g.records if r.poisoned is not None and all(w in r.site for w in where)]
        assert len(outs) >= least and bool(torch.stack([r.poisoned for r in outs]).all()), (len(outs), where)


# C-ABI entries that launch a kernel but are not driven here, each with its reason
OUT_OF_SCOPE = {
    "recalgo_exchange_plan": "row-sharded deployment only (parallel.py): driven by test_gpu_dist*.py, which are left out",
}


def test_every_kernel_entry_ran_under_the_guard():
    kernels = {n for n in _lib.SIGNATURES if not redzone.is_pure_query(n)}
    assert set(OUT_OF_SCOPE) <= kernels
    missing = kernels - set(OUT_OF_SCOPE) - redzone.LAUNCHED
    assert not missing and len(_ran) == len(CASES), (f"{len(_ran)} of {len(CASES)} guarded cases have passed in this process; "
                                                     f"C-ABI entries no guarded case launched: {sorted(missing)}")
