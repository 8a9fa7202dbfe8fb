"""Guarded, poisoned device allocations for the kernel-level parity tests (plain PyTorch, no native code).

    with guarded() as g:
        test_gpu_dense.test_dense_fwd_bwd(dev, M=65, K=33, N=65, relu=True, use_bias=True)

While the guard is active the tensor factories the host layer uses (torch.empty, empty_like, zeros, zeros_like, full,
full_like, ones, Tensor.new_zeros, Tensor.new_empty: the complete set of ops.py, nn.py, sparse.py, variables.py and
parallel.py) are swapped, as attributes of `torch` / `torch.Tensor`, for wrappers.  A contiguous, strided, non-empty result
on the guarded device type becomes the body of a byte buffer of its own

    [ RZ bytes 0xFF | body: nbytes | RZ bytes 0xFF (+ < 16 bytes of padding, 0xFF too) ]

allocated with the saved factory.  The body starts 16-byte aligned (RZ % 16 == 0), so the kernels' aligned arms are still
selected, and the rear redzone starts at the first byte after the last element.  `empty*` results keep the 0xFF fill; the
other factories' values are copied in.  Tensor.to is swapped as well: a host tensor copied to the guarded device (how
most tests build their inputs) lands in such a buffer too, so what lies behind an input is 0xFF, not a neighbour's
data.  ops._workspace is swapped for a version that returns a guarded buffer of exactly
the byte count asked for (at least 16), not the grow-only pool with its 1 MiB floor; ops._ws_cache and ops._dense_ws are
emptied on entry and on exit.  _lib.load is swapped for a version that returns a recording proxy of the library, so a test
can tell which C-ABI entries ran under the guard (LAUNCHED).  Everything is put back on exit, also on an exception.

check() (called on exit unless an exception is propagating) synchronizes once and asserts that every redzone is still
all 0xFF and that every input registered with input() still equals its clone bit for bit.

What this detects, at the shapes the guarded tests run:
  * writes before the start or past the end of an output, a gradient, a partial-row buffer or a workspace (up to RZ away);
  * a `*_workspace_bytes` query that under-reports (the workspace is exactly as large as the query said);
  * output elements no kernel writes: 0xFF.. is a NaN as fp32 / bf16 / fp16 / fp64, tests/util.assert_close asserts
    isfinite and assert_bit_exact against a finite reference fails on NaN; the integer outputs of `empty*` (plans,
    dedup and live lists) are compared exactly by their tests, and 0xFF.. is -1 there;
  * a kernel that relies on a zero in `torch.empty` scratch (ticket, counter);
  * reads past the end of a FLOAT input placed with input() or `.to(device)`, where the value reaches the result (NaN);
  * writes into an input placed with input().
What it does not detect: over-reads of INTEGER inputs (0xFF.. is -1, this project's OOV id, which every lookup kernel
skips - chosen so that an over-read id cannot become a wild address); an overrun farther than RZ from the buffer; anything
inside a captured graph or a model-level / distributed test: the guard must not be active around those.

RZ = 256 KiB: one 64-row tile of the widest tested output (64 rows x 1024 columns x 4 bytes), the most a kernel that
stores a whole tile where a partial one was due can overrun by.  No kernel of csrc/ has a taller or wider store tile.
"""
from __future__ import annotations

import os
import sys

import torch

RZ = 256 << 10
POISON = 0xFF
FACTORIES = [(torch, n) for n in ("empty", "empty_like", "zeros", "zeros_like", "full", "full_like", "ones")] + \
            [(torch.Tensor, "new_zeros"), (torch.Tensor, "new_empty")]
_EMPTY_KIND = {"empty", "empty_like", "new_empty"}
_HERE = os.path.abspath(__file__)
_TORCH_DIR = os.path.dirname(os.path.abspath(torch.__file__)) + os.sep

LAUNCHED = set()         # C-ABI entries that ran under a guard in this process (queries: called; kernels: returned 0)


def _call_site():
    """('file:line in function' of the first frame outside this file and torch, whether an autograd backward is on the stack)."""
    f = sys._getframe(1)
    site, in_backward = None, False
    while f is not None:
        fn = f.f_code.co_filename
        if site is None and os.path.abspath(fn) != _HERE and not os.path.abspath(fn).startswith(_TORCH_DIR):
            site = f"{fn}:{f.f_lineno} in {f.f_code.co_name}"
        if site is not None and f.f_code.co_name == "backward":
            in_backward = True
            break
        f = f.f_back
    return site or "<unknown>", in_backward


class Record:
    __slots__ = ("buf", "off", "nbytes", "site", "in_backward", "kind", "body", "clone", "poisoned")

    def __init__(self, buf, off, nbytes, site, kind, body):
        self.buf, self.off, self.nbytes, self.kind, self.body = buf, off, nbytes, kind, body
        self.site, self.in_backward = site   # (in_backward: allocated below the `backward` of an autograd.Function)
        self.clone = None        # input(): the bytes the body must still hold at check time
        self.poisoned = None     # audit: device bool, "the whole body was 0xFF" as of the allocation, in stream order


class _LibProxy:
    """The loaded library with every recalgo_* entry wrapped to record its name (a kernel entry only when it returned 0)."""

    def __init__(self, lib, is_query, redirect, launched):
        self.__dict__.update(_lib=lib, _is_query=is_query, _redirect=redirect, _launched=launched)

    def __getattr__(self, name):
        fn = getattr(self._lib, name)
        if not name.startswith("recalgo_"):
            return fn
        query = self._is_query(name)
        other = self._redirect.get(name)           # (plain entry, its arguments from this entry's | None when they differ)

        def call(*a):
            b = other[1](a) if other is not None else None
            if b is not None:
                rc, ran = getattr(self._lib, other[0])(*b), other[0]
            else:
                rc, ran = fn(*a), name
            if query or rc == 0:
                LAUNCHED.add(ran)
                self._launched.add(ran)
            return rc
        self.__dict__[name] = call
        return call


def is_pure_query(name: str) -> bool:
    """C-ABI entries that compute a number on the host and launch nothing (they take no stream)."""
    return name in ("recalgo_abi_version", "recalgo_target_arch") or \
        name.endswith(("_supported", "_workspace_bytes", "_header_bytes", "_partial_rows", "_partial_floats", "_buckets_log2",
                       "_source_slots", "_feature_count"))


class guarded:
    def __init__(self, device_type: str = "cuda", rz: int = RZ, audit: bool = False, redirect=None):
        """audit: every `empty*` record notes whether its body was all 0xFF when handed out.  redirect: {entry: (plain entry,
        args -> the plain entry's args | None)}: calls of a superset C-ABI entry that ask for nothing beyond the plain
        entry run the plain entry instead (the host layer only ever calls the superset; a C caller may call either)."""
        assert rz % 16 == 0 and rz > 0
        self.device_type, self.rz, self.audit, self.redirect = device_type, rz, audit, dict(redirect or {})
        self.records = []
        self.launched = set()    # C-ABI entries that ran under THIS guard
        self._saved = {}
        self._active = False

    # ---- allocation -------------------------------------------------------------------------------------------------------
    def _alloc(self, nbytes, dtype, shape, device, site, kind, shift=0):
        rz = self.rz
        total = (rz + shift + nbytes + rz + 15) // 16 * 16
        buf = self._saved["full"]((total,), POISON, dtype=torch.uint8, device=device)
        off = rz + shift
        # the body as a tensor of its own over the buffer's storage == buf[off:off + nbytes].view(dtype).view(shape), but not
        # an autograd view of `buf`: the host layer returns such tensors from autograd.Function.forward and writes them in place
        item = torch.empty(0, dtype=dtype).element_size()
        assert off % item == 0
        body = self._saved["empty"](0, dtype=dtype, device=device).set_(buf.untyped_storage(), off // item, tuple(shape))
        rec = Record(buf, off, nbytes, site, kind, body)
        self.records.append(rec)
        return rec

    def _eligible(self, r) -> bool:
        return (type(r) is torch.Tensor and r.device.type == self.device_type and r.layout == torch.strided
                and r.numel() > 0 and r.is_contiguous() and not r.is_quantized)

    def _wrapper(self, name, orig):
        empty_kind = name in _EMPTY_KIND

        def factory(*a, **kw):
            r = orig(*a, **kw)
            if kw.get("out") is not None or not self._eligible(r):
                return r
            rec = self._alloc(r.numel() * r.element_size(), r.dtype, r.shape, r.device, _call_site(), name)
            g = rec.body
            if empty_kind:
                if self.audit:
                    rec.poisoned = (rec.buf[rec.off:rec.off + rec.nbytes] == POISON).all()
            else:
                g.copy_(r.detach())
            if r.requires_grad:
                g.requires_grad_(True)
            return g
        factory.__name__ = name
        return factory

    def _to_wrapper(self, orig):
        def to(t, *a, **kw):
            r = orig(t, *a, **kw)
            if (type(t) is not torch.Tensor or t.device.type == self.device_type or t.requires_grad or r.requires_grad
                    or not self._eligible(r)):
                return r
            rec = self._alloc(r.numel() * r.element_size(), r.dtype, r.shape, r.device, _call_site(), "to")
            rec.body.copy_(r)
            return rec.body
        return to

    def input(self, t, dev=None, shifted=False, const=True):
        """A device copy of `t` with 0xFF on both sides: body 16-byte aligned, or (shifted) one element past that, as
        test_gpu_dispatch_arms._shifted places it.  The copy is compared with `t`'s bytes at check time unless `const` is
        False (a helper that also places buffers a kernel is meant to write)."""
        device = torch.device(dev) if dev is not None else torch.device(self.device_type)
        t = t.detach().contiguous()
        if t.numel() == 0:
            return t.to(device)
        rec = self._alloc(t.numel() * t.element_size(), t.dtype, t.shape, device, _call_site(), "input",
                          shift=t.element_size() if shifted else 0)
        rec.body.copy_(t)
        if const:
            rec.clone = rec.buf[rec.off:rec.off + rec.nbytes].clone()
        assert rec.body.is_contiguous() and (rec.body.data_ptr() % 16 != 0) == bool(shifted)
        return rec.body

    def _workspace(self, nbytes, device):
        n = max(int(nbytes), 16)
        return self._alloc(n, torch.uint8, (n,), device, _call_site(), "workspace").body

    # ---- install / remove -------------------------------------------------------------------------------------------------
    def __enter__(self):
        from recalgorithm_amd import _lib, ops
        assert not self._active
        for owner, name in FACTORIES:
            self._saved[name] = getattr(owner, name)
        self._saved_ws, self._saved_load, self._saved_to = ops._workspace, _lib.load, torch.Tensor.to
        real_load, proxies = _lib.load, {}

        def load(*a, **kw):
            lib = real_load(*a, **kw)
            if id(lib) not in proxies:
                proxies[id(lib)] = _LibProxy(lib, is_pure_query, self.redirect, self.launched)
            return proxies[id(lib)]
        ops._ws_cache.clear()
        ops._dense_ws.clear()
        try:
            for owner, name in FACTORIES:
                setattr(owner, name, self._wrapper(name, self._saved[name]))
            torch.Tensor.to = self._to_wrapper(self._saved_to)
            ops._workspace = self._workspace
            _lib.load = load
        except BaseException:
            self._restore()
            raise
        self._active = True
        return self

    def _restore(self):
        from recalgorithm_amd import _lib, ops
        for owner, name in FACTORIES:
            setattr(owner, name, self._saved[name])
        ops._workspace, _lib.load, torch.Tensor.to = self._saved_ws, self._saved_load, self._saved_to
        ops._ws_cache.clear()
        ops._dense_ws.clear()
        ops.discard_step_work()      # (deferred work of the guarded test may hold guarded buffers)
        self._active = False

    def __exit__(self, et, ev, tb):
        try:
            if et is None:
                self.check()
        finally:
            self._restore()
            self.records = []
        return False

    # ---- the check --------------------------------------------------------------------------------------------------------
    def check(self):
        """One synchronize; every redzone still 0xFF, every registered input unchanged.  One reduced tensor comes back."""
        if not self.records:
            return
        if self.device_type == "cuda":
            torch.cuda.synchronize()
        recs = list(self.records)
        false = self._saved["zeros"]((), dtype=torch.bool, device=recs[0].buf.device)
        flags = []
        for r in recs:
            hi = r.off + r.nbytes
            flags += [(r.buf[:r.off] != POISON).any(), (r.buf[hi:] != POISON).any(),
                      (r.buf[r.off:hi] != r.clone).any() if r.clone is not None else false]
        bad = torch.stack(flags).cpu().view(-1, 3)
        if not bool(bad.any()):
            return
        msgs = []
        for r, (front, rear, body) in zip(recs, bad.tolist()):
            hi = r.off + r.nbytes
            for hit, side, diff, base in ((front, "front redzone", lambda: r.buf[:r.off] != POISON, -r.off),
                                          (rear, "rear redzone", lambda: r.buf[hi:] != POISON, r.nbytes),
                                          (body, "registered input", lambda: r.buf[r.off:hi] != r.clone, 0)):
                if hit:
                    d = diff().cpu()
                    first = int(torch.nonzero(d)[0]) + base
                    msgs.append(f"{side} of the {r.kind} buffer ({r.nbytes} bytes) allocated at {r.site} was written: "
                                f"{int(d.sum())} bytes differ, the first at byte offset {first} from the start of the body")
        raise AssertionError("redzone: " + "; ".join(msgs[:8]) + (f"; ... {len(msgs) - 8} more" if len(msgs) > 8 else ""))

    def records_at(self, where: str, kind=None):
        """The records whose call site contains `where` ('ops.py', 'in backward', ...)."""
        return [r for r in self.records if where in r.site and (kind is None or r.kind == kind)]
