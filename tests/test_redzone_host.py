"""tests/redzone.py on the CPU: the guard's own placement, poisoning, restore and reporting, with device_type="cpu".
The out-of-body stores here are plain tensor indexing into the guard's own buffers; no kernel is involved."""
import pytest
import torch

from tests import redzone
from tests.redzone import POISON, RZ, guarded


def _originals():
    return [getattr(owner, name) for owner, name in redzone.FACTORIES] + [torch.Tensor.to]


def test_body_is_aligned_and_poisoned():
    with guarded("cpu") as g:
        for dtype in (torch.float32, torch.float64, torch.bfloat16, torch.float16):
            e = torch.empty(5, 3, dtype=dtype)
            assert e.shape == (5, 3) and e.dtype == dtype and e.is_contiguous() and e.data_ptr() % 16 == 0
            assert bool(torch.isnan(e).all())
        assert bool(torch.isnan(torch.empty_like(torch.zeros(7))).all())
        assert bool(torch.isnan(torch.zeros(2).new_empty(9)).all())
        for dtype in (torch.int32, torch.int64):
            assert bool((torch.empty(6, dtype=dtype) == -1).all())       # the OOV id
        r = g.records[0]
        assert r.off == RZ and r.nbytes == 5 * 3 * 4 and r.buf.numel() >= 2 * RZ + r.nbytes and r.buf.numel() % 16 == 0
        assert r.body.data_ptr() == r.buf.data_ptr() + RZ
        assert bool((r.buf[:RZ] == POISON).all()) and bool((r.buf[RZ + r.nbytes:] == POISON).all())
        assert "test_redzone_host.py" in r.site and "test_body_is_aligned_and_poisoned" in r.site


def test_value_factories_keep_their_values():
    with guarded("cpu") as g:
        z, o, f = torch.zeros(3, 4), torch.ones(5, dtype=torch.int64), torch.full((2, 2), 2.5)
        zl, fl = torch.zeros_like(f), torch.full_like(o, -1)
        nz = f.new_zeros(7)
        leaf = torch.zeros(4, requires_grad=True)
        assert torch.equal(z, torch.tensor(0.0).expand(3, 4)) and torch.equal(o, torch.tensor(1).expand(5))
        assert torch.equal(f, torch.tensor(2.5).expand(2, 2)) and torch.equal(zl, torch.tensor(0.0).expand(2, 2))
        assert torch.equal(fl, torch.tensor(-1).expand(5)) and nz.shape == (7,) and float(nz.abs().sum()) == 0.0
        assert leaf.is_leaf and leaf.requires_grad
        assert len(g.records) == 7 and all(r.body.data_ptr() % 16 == 0 for r in g.records)


def test_empty_and_foreign_results_pass_through():
    transposed = torch.zeros(4, 6).t()
    with guarded("cpu") as g:
        assert torch.empty(0, 16).shape == (0, 16)
        assert torch.zeros(4, device="meta").device.type == "meta"
        assert torch.empty_like(transposed).shape == (6, 4)          # (not contiguous: left alone)
        assert g.records == []
    with guarded("cuda") as g:                   # a guard for the device leaves CPU tensors alone
        torch.zeros(4)
        assert g.records == []


def test_originals_are_restored_also_after_an_exception():
    from recalgorithm_amd import _lib, ops
    before, ws, load = _originals(), ops._workspace, _lib.load
    with pytest.raises(KeyError):
        with guarded("cpu"):
            assert _originals() != before and ops._workspace is not ws and _lib.load is not load
            raise KeyError("boom")
    assert _originals() == before and ops._workspace is ws and _lib.load is load
    with guarded("cpu"):
        pass
    assert _originals() == before and ops._workspace is ws and _lib.load is load


def test_allocations_inside_backward_are_seen():
    class Twice(torch.autograd.Function):
        @staticmethod
        def forward(ctx, x):
            out = torch.empty_like(x)
            out.copy_(x * 2)
            return out

        @staticmethod
        def backward(ctx, g):
            d = torch.empty_like(g)
            d.copy_(g * 2)
            return d + g.new_zeros(g.shape)

    with guarded("cpu") as g:
        x = torch.zeros(5, requires_grad=True)
        Twice.apply(x).sum().backward()
        assert torch.equal(x.grad, torch.full((5,), 2.0))
        assert len(g.records_at("in forward")) == 1 and len(g.records_at("in backward")) == 2
        assert [r.in_backward for r in g.records[:4]] == [False, False, True, True]


@pytest.mark.parametrize("side", ["rear", "front"])
def test_a_store_outside_the_body_is_reported(side):
    g = guarded("cpu")
    with pytest.raises(AssertionError) as ei:
        with g:
            torch.zeros(8)
            out = torch.empty(3, 5)              # <- the reported call site
            out.fill_(1.0)
            g.check()                            # a full body alone is fine
            r = g.records[-1]
            if side == "rear":
                r.buf[RZ + r.nbytes] = 0
                r.buf[RZ + r.nbytes + 7] = 1
            else:
                r.buf[RZ - 1] = 0
    msg = str(ei.value)
    assert f"{side} redzone" in msg and "test_a_store_outside_the_body_is_reported" in msg and "empty buffer (60 bytes)" in msg
    if side == "rear":
        assert "2 bytes differ" in msg and "first at byte offset 60 " in msg
    else:
        assert "1 bytes differ" in msg and "first at byte offset -1 " in msg
    assert ("front redzone" if side == "rear" else "rear redzone") not in msg


def test_inputs_are_placed_and_a_store_into_one_is_reported():
    t = torch.arange(12, dtype=torch.float32).reshape(3, 4)
    with guarded("cpu") as g:
        a, s = g.input(t), g.input(t, shifted=True)
        assert torch.equal(a, t) and torch.equal(s, t) and a.data_ptr() % 16 == 0 and s.data_ptr() % 16 == 4
        ra, rs = g.records
        assert bool((rs.buf[:RZ + 4] == POISON).all()) and bool((rs.buf[RZ + 4 + 48:] == POISON).all())
        assert bool(torch.isnan(ra.buf[RZ + 48:RZ + 64].view(torch.float32)).all())        # what an over-read sees
        assert g.input(torch.zeros(0, 3)).shape == (0, 3)
    with pytest.raises(AssertionError, match=r"registered input of the input buffer \(48 bytes\).*1 bytes differ.*offset 20 "):
        with guarded("cpu") as g:
            a = g.input(t)
            a.view(torch.uint8).view(-1)[20] += 1


def test_workspace_is_exact_and_the_caches_end_empty():
    from recalgorithm_amd import ops
    dev = torch.device("cpu")
    ops._ws_cache[("cpu", None)] = torch.zeros(4)
    with guarded("cpu") as g:
        assert not ops._ws_cache and not ops._dense_ws
        w = ops._workspace(1000, dev)
        assert w.dtype == torch.uint8 and w.numel() == 1000 and w.data_ptr() % 16 == 0 and bool((w == POISON).all())
        assert ops._workspace(3, dev).numel() == 16 and ops._workspace(0, dev).numel() == 16
        assert ops._workspace(1000, dev).data_ptr() != w.data_ptr()             # never reused inside the guard
        assert [r.kind for r in g.records] == ["workspace"] * 4 and "test_redzone_host.py" in g.records[0].site
        ops._dense_ws["k"] = torch.empty(64, dtype=torch.uint8)
        assert g.records[-1].nbytes == 64
    assert not ops._ws_cache and not ops._dense_ws
    with pytest.raises(AssertionError, match="rear redzone of the workspace buffer"):
        with guarded("cpu") as g:
            ops._workspace(32, dev)
            g.records[0].buf[RZ + 32] = 0


def test_library_calls_are_recorded():
    from recalgorithm_amd import _lib
    assert redzone.is_pure_query("recalgo_cross_bwd_workspace_bytes") and redzone.is_pure_query("recalgo_abi_version")
    assert not redzone.is_pure_query("recalgo_dense_fwd") and not redzone.is_pure_query("recalgo_copy_bytes")
    for name, (_, args) in _lib.SIGNATURES.items():          # a kernel entry ends with its stream, a query has none
        assert redzone.is_pure_query(name) == (not args or args[-1] is not _lib.P), name
    with guarded("cpu"):
        lib = _lib.load()
        assert lib.recalgo_abi_version() == _lib.ABI_VERSION
        assert lib.recalgo_cross_bwd_partial_rows(4096) > 0
    assert {"recalgo_abi_version", "recalgo_cross_bwd_partial_rows"} <= redzone.LAUNCHED
