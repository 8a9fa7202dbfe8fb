"""CPU: the deferred work a training step leaves in recalgorithm_amd/ops.py has one reset, ops.discard_step_work(), which
VariableStore.begin_call runs when a forward begins.  Pure host bookkeeping: nothing here may touch librecalgo_hip.so."""
import pytest

from recalgorithm_amd import _lib, ops
from recalgorithm_amd.variables import VariableStore

LISTS = ("_lazy_gathers", "_dense_pending", "_colsum_pending", "_parked_l2")
SLOTS = ("_wgrad_rider", "_cross_rider")


def _fill(monkeypatch):
    for name in LISTS:
        getattr(ops, name).append(object())
    ops._dlogit_partials[12345] = object()
    for name in SLOTS:
        monkeypatch.setattr(ops, name, object())


def _assert_empty():
    for name in LISTS:
        assert getattr(ops, name) == [], name
    assert ops._dlogit_partials == {}
    for name in SLOTS:
        assert getattr(ops, name) is None, name


@pytest.fixture
def no_lib(monkeypatch):
    def load():
        raise AssertionError("the discard of a step's deferred work must not touch the library")
    monkeypatch.setattr(_lib, "load", load)
    yield
    ops.discard_step_work()


def test_discard_empties_every_step_work_container(no_lib, monkeypatch):
    pending = ops._dense_pending
    _fill(monkeypatch)
    ops.discard_step_work()
    _assert_empty()
    assert ops._dense_pending is pending          # (bench.py holds and edits the live list)


def test_begin_call_discards_what_an_abandoned_step_left(no_lib, monkeypatch):
    _fill(monkeypatch)
    VariableStore("cpu").begin_call()
    _assert_empty()
