"""-m gpu parity of the kernel arms the dispatchers select only off the hot path: alignment fall-backs, field counts past the
fast kernels' limits, partly filled column tiles and LDS ceilings.  Every other GPU test builds its inputs as fresh (16-byte
aligned) allocations at the reference's shapes, which always lands on the fast arm.

    arm                                        condition that selects it                         test that forces it
    -----------------------------------------  ------------------------------------------------  ------------------------------
 1  din_attention_fwd_kernel<16>               H = 16 and query, keys or out not 16-byte aligned  test_din_generic_arm
 2  din_attention_bwd_kernel<16> (both         H = 16 and query, keys, dquery or dkeys not        test_din_generic_arm,
    is_softmax branches; ldg > H read of g,    aligned; g a column block of a wider gradient;      test_din_generic_arm_joined
    fused dq_extra add)                        the query's other gradient parked in a GradJoin
 3  ipnn_features_bwd_kernel                   K % 4 != 0, or emb / d_emb not aligned, or the     test_ipnn_features_bwd_general_arm,
                                               bwd4 LDS need > 160 KiB (F = 91..127 at K = 16)     test_pnn_product_layer_unaligned
 4  cin_permute_kernel x2 + launch_contract    m > 32 fields (with and without dX^k; dx0          test_cin_many_fields,
    for dX^k and dX^0                          accumulate 0 and 1 in a two-layer stack)            test_cin_stack_many_fields
 5  cin_filter_grad_kernel<32, 2, ...>         D = 32, N > 32 (two column tiles), B not a          test_cin_filter_grad_d32
                                               multiple of the split
 6  cin_contract2_kernel<16, 2|4, ...> with a  D = 16, 17 <= m <= 32, N in (32, 64) or (96, 128)   test_cin_contract2_partial_tile
    partly filled last column tile; general    not a multiple of 32; a filter pointer not          test_cin_unaligned_filter
    contraction / input gradient for an        16-byte aligned
    unaligned filter
 7  concat_sumsq_kernel, float4 and scalar     widths / column offsets % 4 and parts aligned ->    test_concat_sumsq_arms,
    arms; the last-workgroup ticket            float4, else scalar; > 256 workgroups at B = 4097;  test_concat_sumsq_ticket_*,
                                               B = 0                                               test_concat_sumsq_empty_batch
 8  (no arm: one sum launch, six outputs)      the six DIN weight gradients in separate buffers    test_din_generic_arm (flat_grads):
                                               or in one flat buffer in the partial row's order    the two layouts are bit-equal
 9  LDS ceilings (launch_lds)                  pnn: IPNN F = 255 (the largest accepted) at K = 16;  test_ipnn_lds_ceiling,
                                               fibinet: bilinear F = 128 (the largest accepted)    test_bilinear_lds_ceiling
10  launch_lds's dynamic-LDS grant, kept per   bag_mean_bwd_kernel<4> at K = 32, 16, 64 in a fresh    test_lds_grant_grows,
    (kernel, device) as a high-water mark      process: 70 KiB granted, 38 KiB below the default,    test_lds_grant_second_device
                                               134 KiB above the grant; K = 64 on device 0, then 1

Each arm is compared with a float64 restatement (oracle.ref_ops, or a plain formula with its reference line) under the
strict `ref32` guard of tests/util.py; where a fast arm exists for the same arguments, the same inputs also run through it.
The two arms of a row are not required to agree bit for bit: their summation orders differ.  Row 8 is no such pair: wherever
the six gradient buffers lie, the same launch adds the same partial rows in the one fixed order (csrc/slab_sum.h)."""
import ctypes
import os
import subprocess
import sys

import pytest
import torch

from oracle import ref_ops as R
from recalgorithm_amd import _lib, ops
from recalgorithm_amd.variables import Variable, VariableStore
from tests.util import assert_bit_exact, assert_close

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _p(t):
    return None if t is None else ctypes.c_void_p(t.data_ptr())


def _st():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def _shifted(t, dev, place=None):
    """A contiguous device copy of `t` one float past a fresh allocation: passes ops._chk, is not 16-byte aligned.
    `place(t, dev, shifted=True)`: another way to put it there (tests/redzone.py's guard.input, test_gpu_redzone.py)."""
    if place is not None:
        v = place(t, dev, shifted=True)
    else:
        v = torch.empty(t.numel() + 1, device=dev, dtype=t.dtype)[1:].view(t.shape)
        v.copy_(t)
    assert v.is_contiguous() and v.data_ptr() % 16 != 0
    return v


def _aligned(t, dev, place=None):
    v = t.to(dev) if place is None else place(t, dev)
    assert v.data_ptr() % 16 == 0
    return v


# ---- rows 1, 2, 8: DIN attention, the generic H = 16 kernels ------------------------------------------------------------
def _din_inputs(B, T, H, gen):
    q = torch.randn(B, H, generator=gen)
    lens = torch.randint(0, T + 1, (B,), generator=gen)
    lens[0] = 0
    lens[-1] = T
    keys = torch.randn(B, T, H, generator=gen)
    keys = keys * (torch.arange(T).unsqueeze(0) < lens.unsqueeze(1)).unsqueeze(-1)
    ws = [torch.randn(4 * H, 64, generator=gen) / (4 * H) ** 0.5, torch.randn(64, generator=gen) * 0.1,
          torch.randn(64, 32, generator=gen) / 8.0, torch.randn(32, generator=gen) * 0.1,
          torch.randn(32, 1, generator=gen) / 32 ** 0.5, torch.randn(1, generator=gen) * 0.1]
    return q, keys, lens, ws


def _din_vars(ws, dev, flat_grads):
    vs = [Variable(f"v{i}", w.to(dev)) for i, w in enumerate(ws)]
    if flat_grads:
        # the six gradients in one buffer, in the kernel's partial-row order (a model's flat gradient buffer)
        flat = torch.zeros(sum(w.numel() for w in ws), device=dev)
        off = 0
        for v in vs:
            v.grad = flat[off:off + v.data.numel()].view(v.data.shape)
            off += v.data.numel()
    return vs


def _din_oracle(q, keys, lens, ws, g, is_softmax, dtype):
    a = [t.to(dtype, copy=True).requires_grad_(True) for t in [q, keys] + ws]
    r = R.din_attention(a[0], a[1], lens, *a[2:], is_softmax=is_softmax)      # din_attention.py:17-41
    r.backward(g.to(dtype))
    return r.detach(), [t.grad for t in a]


def _din_check(tag, out, dq, dk, vs, ref, a, r32, a32, is_softmax):
    assert_close(out, ref, what=f"{tag} fwd", ref32=r32)
    assert_close(dq, a[0], what=f"{tag} dq", ref32=a32[0])
    assert_close(dk, a[1], what=f"{tag} dkeys", ref32=a32[1])
    for i, nm in enumerate(["f1_w", "f1_b", "f2_w", "f2_b", "f3_w", "f3_b"]):
        if nm == "f3_b" and is_softmax:
            # softmax is shift invariant: the reference value is cancellation noise (test_gpu_din.py)
            assert float((vs[i].grad.cpu().double() - a[7]).abs().max()) <= 1e-5 * max(float(a[6].abs().max()), 1e-30)
            continue
        assert_close(vs[i].grad, a[2 + i], what=f"{tag} d{nm}", reduced=True, ref32=a32[2 + i])


@pytest.mark.parametrize("is_softmax", [False, True])
@pytest.mark.parametrize("B,T,shift,flat_grads", [(37, 50, "query", False), (300, 64, "keys", False), (19, 7, "both", True)])
def test_din_generic_arm(dev, B, T, shift, flat_grads, is_softmax):
    """H = 16 with an unaligned query or keys: din_attention_{fwd,bwd}_kernel<16> instead of din16::*; the same inputs
    aligned take din16::*.  B = 300 > 256 workgroups: a workgroup walks several examples."""
    H = 16
    gen = torch.Generator().manual_seed(B * 3 + T)
    q, keys, lens, ws = _din_inputs(B, T, H, gen)
    g = torch.randn(B, H, generator=gen)
    ref, a = _din_oracle(q, keys, lens, ws, g, is_softmax, torch.float64)
    r32, a32 = _din_oracle(q, keys, lens, ws, g, is_softmax, torch.float32)
    store = VariableStore(dev)
    for arm in ("din16", "generic"):
        if arm == "din16":
            qd, kd = _aligned(q, dev), _aligned(keys, dev)
        else:
            qd = _shifted(q, dev) if shift in ("query", "both") else _aligned(q, dev)
            kd = _shifted(keys, dev) if shift in ("keys", "both") else _aligned(keys, dev)
        qd.requires_grad_(True)
        kd.requires_grad_(True)
        vs = _din_vars(ws, dev, flat_grads)
        out = ops.din_attention(store, qd, kd, lens.to(dev), vs, is_softmax)
        out.backward(g.to(dev))
        _din_check(f"din[{arm}]", out, qd.grad, kd.grad, vs, ref, a, r32, a32, is_softmax)
        # the other layout of the six gradient buffers, same inputs, same kernel arm: the same bits
        qd.grad = kd.grad = None
        vs2 = _din_vars(ws, dev, not flat_grads)
        ops.din_attention(store, qd, kd, lens.to(dev), vs2, is_softmax).backward(g.to(dev))
        for i, nm in enumerate(["f1_w", "f1_b", "f2_w", "f2_b", "f3_w", "f3_b"]):
            assert_bit_exact(vs2[i].grad, vs[i].grad, f"din[{arm}] d{nm}: flat against separate gradient buffers")


@pytest.mark.parametrize("is_softmax", [False, True])
def test_din_generic_arm_joined(dev, is_softmax):
    """DIN's concat (din.py:249-257) with the query's gradient parked in a GradJoin: the attention's g is a column block of
    the [B, 40] concat gradient (ldg = 40 > H) and the parked block is added in the generic backward kernel's epilogue."""
    from recalgorithm_amd import nn
    B, T, H, W0 = 70, 20, 16, 8
    gen = torch.Generator().manual_seed(11 + is_softmax)
    q, keys, lens, ws = _din_inputs(B, T, H, gen)
    side = torch.randn(B, W0, generator=gen)
    G = torch.randn(B, W0 + 2 * H, generator=gen)

    def oracle(dtype):
        a = [t.to(dtype, copy=True).requires_grad_(True) for t in [q, keys] + ws]
        att = R.din_attention(a[0], a[1], lens, *a[2:], is_softmax=is_softmax)
        torch.cat([side.to(dtype), a[0], att], dim=1).backward(G.to(dtype))
        return att.detach(), [t.grad for t in a]
    ref, a = oracle(torch.float64)
    r32, a32 = oracle(torch.float32)
    store = VariableStore(dev)
    for arm in ("din16", "generic"):
        qd = (_aligned(q, dev) if arm == "din16" else _shifted(q, dev)).requires_grad_(True)
        kd = _aligned(keys, dev).requires_grad_(True)
        vs = _din_vars(ws, dev, False)
        join = nn.GradJoin()
        att = ops.din_attention(store, qd, kd, lens.to(dev), vs, is_softmax, query_join=join)
        cat, _ = ops.concat_sumsq([side.to(dev), qd, att], 0.0, joins={1: join})
        cat.backward(G.to(dev))
        assert join.consumer_done and join.pending is None
        _din_check(f"din joined[{arm}]", att, qd.grad, kd.grad, vs, ref, a, r32, a32, is_softmax)


# ---- rows 3, 9: IPNN feature gradient, the general kernel; LDS ceilings ---------------------------------------------------
def _ipnn_oracle(emb, dphi, F, K, dtype):
    """phi[b, t(f, f')] = <e_f, e_f'>, f <= f', row-major upper triangle (pnn.py:152-157 expanded);
    -> (phi, d emb of sum(phi * dphi))."""
    e = emb.to(dtype, copy=True).requires_grad_(True)
    E = e.reshape(-1, F, K)
    iu = torch.triu_indices(F, F)
    phi = (E @ E.transpose(1, 2))[:, iu[0], iu[1]]
    (phi * dphi.to(dtype)).sum().backward()
    return phi.detach(), e.grad


@pytest.mark.parametrize("B,F,K,shift", [
    (37, 6, 5, None), (40, 9, 6, None), (19, 26, 10, None),        # K % 4 != 0
    (33, 26, 16, "emb"), (21, 13, 8, "d_emb"),                     # an unaligned operand
    (9, 100, 16, None), (5, 127, 16, None),                        # bwd4 would need > 160 KiB of LDS
])
def test_ipnn_features_bwd_general_arm(dev, B, F, K, shift):
    lib = _lib.load()
    gen = torch.Generator().manual_seed(B * F + K)
    T = F * (F + 1) // 2
    emb = torch.randn(B, F * K, generator=gen) * 0.5
    dphi = torch.randn(B, T, generator=gen)
    phi_ref, d_ref = _ipnn_oracle(emb, dphi, F, K, torch.float64)
    phi32, d32 = _ipnn_oracle(emb, dphi, F, K, torch.float32)
    eg = _shifted(emb, dev) if shift == "emb" else _aligned(emb, dev)
    phi = torch.empty(B, T, device=dev)
    _lib.check(lib.recalgo_pnn_features_fwd(_p(eg), B, F, K, 0, _p(phi), T, _st()), "ipnn features fwd")
    assert_close(phi, phi_ref, what="ipnn phi", ref32=phi32)
    # dphi with a padded row stride, as ops._PnnProductFn passes it
    ld = (T + 3) // 4 * 4
    dphi_pad = torch.full((B, ld), float("nan"), device=dev)
    dphi_pad[:, :T] = dphi.to(dev)
    d_emb = _shifted(torch.zeros(B, F * K), dev) if shift == "d_emb" else torch.zeros(B, F * K, device=dev)
    _lib.check(lib.recalgo_pnn_features_bwd(_p(eg), _p(dphi_pad), ld, B, F, K, 0, _p(d_emb), 0, _st()), "ipnn features bwd")
    assert_close(d_emb, d_ref, what="ipnn d_emb", reduced=True, ref32=d32)
    d_emb.fill_(0.25)
    _lib.check(lib.recalgo_pnn_features_bwd(_p(eg), _p(dphi_pad), ld, B, F, K, 0, _p(d_emb), 1, _st()), "ipnn features bwd acc")
    assert_close(d_emb - 0.25, d_ref, what="ipnn d_emb (accumulate)", reduced=True)
    if K % 4 == 0 and F <= 90:
        # the same arguments with aligned operands: ipnn_features_bwd4_kernel
        ea, da = _aligned(emb, dev), torch.empty(B, F * K, device=dev)
        _lib.check(lib.recalgo_pnn_features_bwd(_p(ea), _p(dphi_pad), ld, B, F, K, 0, _p(da), 0, _st()), "ipnn features bwd4")
        assert_close(da, d_ref, what="ipnn d_emb [bwd4]", reduced=True, ref32=d32)


def test_ipnn_lds_ceiling(dev):
    """F = 255 is the largest IPNN field count accepted (the triangle table holds 8-bit indices).  At K = 16 the forward
    fits its LDS (100 KiB); neither feature-gradient kernel does (from F = 128 on): a clean RecalgoError, never numbers.
    F = 256 is rejected outright."""
    lib = _lib.load()
    B, F, K = 3, 255, 16
    T = F * (F + 1) // 2
    gen = torch.Generator().manual_seed(255)
    emb = torch.randn(B, F * K, generator=gen) * 0.5
    dphi = torch.randn(B, T, generator=gen)
    phi_ref, _ = _ipnn_oracle(emb, dphi, F, K, torch.float64)
    phi32, _ = _ipnn_oracle(emb, dphi, F, K, torch.float32)
    eg = _aligned(emb, dev)
    phi = torch.empty(B, T, device=dev)
    _lib.check(lib.recalgo_pnn_features_fwd(_p(eg), B, F, K, 0, _p(phi), T, _st()), "ipnn features fwd F=255")
    assert_close(phi, phi_ref, what="ipnn phi F=255", ref32=phi32)
    d_emb = torch.full((B, F * K), 7.0, device=dev)
    dphi_d = dphi.to(dev)
    for f in (128, 255):
        t = f * (f + 1) // 2
        with pytest.raises(_lib.RecalgoError):
            _lib.check(lib.recalgo_pnn_features_bwd(_p(eg), _p(dphi_d), t, B, f, K, 0, _p(d_emb), 0, _st()), "bwd")
    torch.cuda.synchronize()
    assert bool((d_emb == 7.0).all())                           # nothing was launched
    with pytest.raises(_lib.RecalgoError):
        _lib.check(lib.recalgo_pnn_features_fwd(_p(eg), 1, 256, 1, 0, _p(phi), 256 * 257 // 2, _st()), "fwd F=256")


def test_pnn_product_layer_unaligned(dev):
    """ops.pnn_product_layer (IPNN, F = 26, K = 16) on an unaligned embedding row block: the general feature-gradient
    kernel inside the op, against the reference's D-iteration loop (pnn.py:133-181) in float64."""
    B, F, K, D = 45, 26, 16, 24
    gen = torch.Generator().manual_seed(26)
    emb = torch.randn(B, F * K, generator=gen) * 0.5
    lw = torch.randn(F * K, D, generator=gen) * 0.1
    pw = torch.randn(D, F, generator=gen) * 0.3
    bias = torch.randn(D, generator=gen) * 0.1
    g = torch.randn(B, D, generator=gen)

    def oracle(dtype):
        a = [t.to(dtype, copy=True).requires_grad_(True) for t in (emb, lw, pw, bias)]
        _, _, out = R.pnn_product(*a, F, K, "IPNN")
        out.backward(g.to(dtype))
        return out.detach(), [t.grad for t in a]
    ref, a = oracle(torch.float64)
    r32, a32 = oracle(torch.float32)
    store = VariableStore(dev)
    lv, pv, bv = Variable("lw", lw.to(dev)), Variable("pw", pw.to(dev)), Variable("b", bias.to(dev))
    x = _shifted(emb, dev).requires_grad_(True)
    out = ops.pnn_product_layer(store, x, lv, pv, bv, F, K, "IPNN")
    out.backward(g.to(dev))
    ops.flush_dense_splits()
    assert_close(out, ref, what="pnn layer out", ref32=r32)
    assert_close(x.grad, a[0], what="pnn layer d_emb", ref32=a32[0])
    assert_close(lv.grad, a[1], what="pnn layer d linear_w", reduced=True, ref32=a32[1])
    assert_close(pv.grad, a[2], what="pnn layer d product_w", reduced=True, ref32=a32[2])
    assert_close(bv.grad, a[3], what="pnn layer d bias", reduced=True, ref32=a32[3])


def test_bilinear_lds_ceiling(dev):
    """F = 128 is the largest field count recalgo_bilinear_* accept.  K = 4, one set, 'each': the forward needs 32 KiB of
    LDS and gives numbers; K = 64, two sets: 1 MiB > 160 KiB, a clean RecalgoError."""
    lib = _lib.load()
    B, F = 2, 128
    P = (F - 1) * (F - 2) // 2
    gen = torch.Generator().manual_seed(128)
    x = torch.randn(B, F, 4, generator=gen)
    w = torch.randn(F - 1, 4, 4, generator=gen) * 0.3
    ref = R.bilinear_interaction(x.double(), w.double(), "each")
    r32 = R.bilinear_interaction(x, w, "each")
    out = torch.empty(B, P, 4, device=dev)
    xd, wd = x.to(dev), w.to(dev)                      # (held: the launch is asynchronous)
    _lib.check(lib.recalgo_bilinear_fwd(_p(xd), _p(wd), None, None, B, F, 4, 1, _p(out), 4, 0, _st()), "fwd")
    assert_close(out, ref, what="bilinear F=128", ref32=r32)
    x64 = torch.zeros(B, F, 64, device=dev)
    w64 = torch.zeros(64, 64, device=dev)
    big = torch.full((B, P, 128), 7.0, device=dev)
    with pytest.raises(_lib.RecalgoError):
        _lib.check(lib.recalgo_bilinear_fwd(_p(x64), _p(w64), _p(x64), _p(w64), B, F, 64, 0, _p(big), 128, 0, _st()), "fwd")
    torch.cuda.synchronize()
    assert bool((big == 7.0).all())


# ---- row 10: the dynamic-LDS grant of csrc/common.h's launch_lds --------------------------------------------------------
def _bag_mean_bwd_check(dev, K):
    """recalgo_embedding_bag_mean_bwd at B = 8 (bags of one to three ids, a table of 16 rows; agg_smem(K, 256) bytes of
    dynamic LDS whatever B is) against the float64 scatter-mean gradient: d table[id] += g[b] / len(bag b)."""
    lib = _lib.load()
    B, rows = 8, 16
    gen = torch.Generator().manual_seed(K)
    lens = torch.randint(1, 4, (B,), generator=gen)
    offsets = torch.zeros(B + 1, dtype=torch.int64)
    offsets[1:] = lens.cumsum(0)
    values = torch.randint(0, rows, (int(offsets[-1]),), generator=gen)
    g = torch.randn(B, K, generator=gen)
    bag = torch.repeat_interleave(torch.arange(B), lens)
    ref = torch.zeros(rows, K, dtype=torch.float64).index_add(0, values, (g.double() / lens.double().unsqueeze(1))[bag])
    ref32 = torch.zeros(rows, K).index_add(0, values, (g / lens.float().unsqueeze(1))[bag])
    with torch.cuda.device(dev):
        vd, od, gd = values.to(dev), offsets.to(dev), g.to(dev)
        grad = torch.zeros(rows, K, device=dev)
        _lib.check(lib.recalgo_embedding_bag_mean_bwd(_p(vd), _p(od), _p(gd), B, K, K, 0, _p(grad), None, _st()),
                   f"bag mean bwd K={K} on {dev}")
        assert_close(grad, ref, what=f"bag mean bwd K={K} on {dev}", reduced=True, ref32=ref32)


def _lds_grant_sequence():
    """(the child process of test_lds_grant_grows)"""
    for K in (32, 16, 64):
        _bag_mean_bwd_check(torch.device("cuda:0"), K)
    print("lds grant sequence passed")


def test_lds_grant_grows(dev):
    """bag_mean_bwd_kernel<4> at K = 32 (71,696 B: the first grant), K = 16 (38,928 B: below the default allowance, no
    grant) and K = 64 (137,232 B: above what was granted): a grant that is not raised again fails the third launch.  In a
    fresh process, so that no earlier test has launched the kernel at K = 64."""
    env = dict(os.environ, PYTHONPATH=ROOT + os.pathsep + os.environ.get("PYTHONPATH", ""))
    code = "from tests.test_gpu_dispatch_arms import _lds_grant_sequence; _lds_grant_sequence()"
    r = subprocess.run([sys.executable, "-c", code], cwd=ROOT, env=env, capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "lds grant sequence passed" in r.stdout, r.stdout[-3000:] + r.stderr[-3000:]


def test_lds_grant_second_device(dev):
    """The grant belongs to (kernel, device): K = 64 on device 0, then on device 1."""
    if torch.cuda.device_count() < 2:
        pytest.skip("needs two devices")
    for d in (0, 1):
        _bag_mean_bwd_check(torch.device(f"cuda:{d}"), 64)


# ---- rows 4, 5, 6: CIN ----------------------------------------------------------------------------------------------------
def _cin_oracle(x0, xk, w, go, gp, dtype):
    """R.cin_layer (cin_layer.py:17-28) and its autograd in `dtype` -> (out, [dx0, dxk, dW])."""
    a = [t.to(dtype, copy=True).requires_grad_(True) for t in (x0, xk, w)]
    r = R.cin_layer(a[0], a[1], a[2])
    torch.autograd.backward([r, r.sum(-1)], [go.to(dtype), gp.to(dtype)])
    return r.detach(), [t.grad for t in a]


def _cin_run(dev, B, m, Hk, N, D, seed, shift_filter=False):
    gen = torch.Generator().manual_seed(seed)
    x0 = torch.randn(B, m, D, generator=gen)
    xk = torch.randn(B, Hk, D, generator=gen)
    w = torch.randn(1, Hk * m, N, generator=gen) / (Hk * m) ** 0.5
    go, gp = torch.randn(B, N, D, generator=gen), torch.randn(B, N, generator=gen)
    ref, a = _cin_oracle(x0, xk, w, go, gp, torch.float64)
    r32, a32 = _cin_oracle(x0, xk, w, go, gp, torch.float32)
    store = VariableStore(dev)
    wv = Variable("f", _shifted(w, dev) if shift_filter else _aligned(w, dev))
    x0d, xkd = x0.to(dev).requires_grad_(True), xk.to(dev).requires_grad_(True)
    out, pooled = ops.cin_layer(store, x0d, xkd, wv)
    torch.autograd.backward([out, pooled], [go.to(dev), gp.to(dev)])
    tag = f"cin B{B} m{m} Hk{Hk} N{N} D{D}{' shifted W' if shift_filter else ''}"
    assert_close(out, ref, what=f"{tag} fwd", reduced=True, ref32=r32)
    assert_close(pooled, ref.sum(-1), what=f"{tag} pooled", reduced=True, ref32=r32.sum(-1))
    # m > 32: dX^0 and dX^k are each ONE contraction over all Hk * N (i, n) or N * m (n, j) pairs (cin_permute_kernel +
    # launch_contract), where the oracle's autograd sums over n (G W^T) first and then over i or j.  The long flat fp32 sums
    # leave up to 2.4x the oracle's strict misses (measured at m = 39: dX^0 100 vs 58 of 8112, dX^k 66 vs 27 of 4160).  The
    # guard's factor is 2.5 for this arm only; the rtol bound below it is unchanged.
    f = 2.5 if m > 32 else 1.5
    assert_close(x0d.grad, a[0], what=f"{tag} dx0", reduced=True, ref32=a32[0], strict_factor=f)
    assert_close(xkd.grad, a[1], what=f"{tag} dxk", reduced=True, ref32=a32[1], strict_factor=f)
    assert_close(wv.grad, a[2], what=f"{tag} dW", reduced=True, ref32=a32[2])
    return (x0, xk, w, go, gp), (a, a32)


@pytest.mark.parametrize("B,m,Hk,N,D", [(13, 39, 20, 24, 16), (6, 100, 12, 40, 8), (9, 36, 7, 20, 16), (5, 128, 3, 9, 4)])
def test_cin_many_fields(dev, B, m, Hk, N, D):
    """m > 32: the input gradient is two filter permutations and two launch_contract calls (cin.hip, recalgo_cin_layer_bwd).
    (9, 36, 7, 20, 16): the dX^0 contraction (HQ = N = 20, C = m = 36) takes cin_contract2; (5, 128, ...): the most fields.
    Also called with dxk = NULL (the first layer of a stack that needs only dX^0)."""
    (x0, xk, w, go, gp), (a, a32) = _cin_run(dev, B, m, Hk, N, D, seed=B * m + N)
    lib = _lib.load()
    x0d, xkd, wd = x0.to(dev), xk.to(dev), w.to(dev)
    G, GP = go.to(dev), gp.to(dev)
    ws = torch.empty(int(lib.recalgo_cin_layer_bwd_workspace_bytes(B, m, Hk, N, D)), dtype=torch.uint8, device=dev)
    dx0 = torch.full_like(x0d, 0.5)
    dw = torch.empty(1, Hk * m, N, device=dev)
    _lib.check(lib.recalgo_cin_layer_bwd(_p(x0d), _p(xkd), _p(wd), _p(G), _p(GP), N, 0, B, m, Hk, N, D, _p(dx0), 1, None, 0,
                                         _p(dw), _p(ws), _st()), "cin bwd without dxk")
    assert_close(dx0 - 0.5, a[0], what="cin m>32 dx0 (no dxk, accumulate)", reduced=True)
    assert_close(dw, a[2], what="cin m>32 dW (no dxk)", reduced=True, ref32=a32[2])


@pytest.mark.parametrize("B,m,D,Ns", [(11, 39, 16, (24, 16)), (7, 33, 8, (40, 12, 20))])
def test_cin_stack_many_fields(dev, B, m, D, Ns):
    """ops.cin_stack at m > 32 (Criteo: 39 fields): the last layer's backward writes dX^0 (dx0_accumulate 0), the earlier
    ones add to it (dx0_accumulate 1), xdeepfm.py:166-174."""
    gen = torch.Generator().manual_seed(B + m)
    x0 = torch.randn(B, m, D, generator=gen)
    Hs = [m] + list(Ns[:-1])
    ws = [torch.randn(1, h * m, n, generator=gen) / (h * m) ** 0.5 for h, n in zip(Hs, Ns)]
    gp = torch.randn(B, sum(Ns), generator=gen)

    def oracle(dtype):
        a0 = x0.to(dtype, copy=True).requires_grad_(True)
        aw = [w.to(dtype, copy=True).requires_grad_(True) for w in ws]
        _, p_plus = R.cin_stack(a0, aw)
        p_plus.backward(gp.to(dtype))
        return p_plus.detach(), a0.grad, [w.grad for w in aw]
    ref, d0, dws = oracle(torch.float64)
    r32, d032, dws32 = oracle(torch.float32)
    store = VariableStore(dev)
    fv = [Variable(f"f{i}", w.to(dev)) for i, w in enumerate(ws)]
    x0d = x0.to(dev).requires_grad_(True)
    p_plus, _ = ops.cin_stack(store, x0d, fv)
    p_plus.backward(gp.to(dev))
    assert_close(p_plus, ref, what="cin stack p_plus", reduced=True, ref32=r32)
    assert_close(x0d.grad, d0, what="cin stack dx0", reduced=True, ref32=d032, strict_factor=2.0)     # (see _cin_run)
    for i, v in enumerate(fv):
        assert_close(v.grad, dws[i], what=f"cin stack dW{i}", reduced=True, ref32=dws32[i])


@pytest.mark.parametrize("B,m,Hk,N", [(45, 6, 10, 50), (77, 7, 9, 64), (30, 12, 12, 100)])
def test_cin_filter_grad_d32(dev, B, m, Hk, N):
    """D = 32: cin_filter_grad_kernel<32, 2, ...> over two or more column tiles, with a last split holding fewer examples
    than the others (B = 45: 23 splits of 2)."""
    _cin_run(dev, B, m, Hk, N, 32, seed=B + N)


@pytest.mark.parametrize("B,m,Hk,N", [(21, 26, 20, 36), (10, 26, 33, 60), (17, 20, 24, 100), (5, 32, 40, 124)])
def test_cin_contract2_partial_tile(dev, B, m, Hk, N):
    """D = 16, 17..32 fields, N not a multiple of 32: cin_contract2_kernel<16, 2 | 4, 13 | 16> with a partly filled last
    column tile (forward); the backward takes the general fused input gradient and filter gradient (N != 64, 128)."""
    _cin_run(dev, B, m, Hk, N, 16, seed=B * 5 + N)


@pytest.mark.parametrize("B,m,Hk,N", [(40, 26, 26, 128), (12, 20, 50, 64)])
def test_cin_unaligned_filter(dev, B, m, Hk, N):
    """The benchmark shape with a filter that is not 16-byte aligned: the general contraction and the general fused input
    gradient instead of cin_contract2 / cin_input_grad2 (both need float4 filter rows); aligned, the same inputs take them."""
    _cin_run(dev, B, m, Hk, N, 16, seed=B + Hk, shift_filter=True)
    _cin_run(dev, B, m, Hk, N, 16, seed=B + Hk, shift_filter=False)


# ---- row 7: concat + sum of squares --------------------------------------------------------------------------------------
def _cat_ref(parts, scale):
    """din.py:249-257: ev = concat(parts); l2_lambda / 2 / B * sum(ev^2) with the scale folded in."""
    cat = torch.cat([p.double() for p in parts], dim=1)
    return cat, scale * cat.pow(2).sum(), scale * torch.cat(parts, dim=1).pow(2).sum()


@pytest.mark.parametrize("B", [1, 15, 16, 17, 4096, 4097])
@pytest.mark.parametrize("widths,shift", [
    ((16,), ()), ((16, 8, 16), ()),                 # float4 arm throughout
    ((16, 8, 16), (1,)),                            # one unaligned part: that part scalar, the others float4
    ((5, 16), ()),                                  # width % 4: scalar, and the next part at column 5
    ((3, 8, 6, 12), (0, 3)),                        # four parts, odd offsets, two of them unaligned
])
def test_concat_sumsq_arms(dev, B, widths, shift):
    gen = torch.Generator().manual_seed(B + sum(widths))
    parts = [torch.randn(B, w, generator=gen) for w in widths]
    scale = 1e-3 / B
    dparts = [_shifted(p, dev) if i in shift else _aligned(p, dev) for i, p in enumerate(parts)]
    out, val = ops.concat_sumsq(dparts, scale)
    cat, ref, r32 = _cat_ref(parts, scale)
    assert_bit_exact(out, cat.float(), what="concat")
    assert_close(val, ref.reshape(1), what="concat sumsq", reduced=True, ref32=r32.reshape(1))


def test_concat_sumsq_ticket_repeated_calls(dev):
    """The workspace of one batch size is zeroed once and re-used: its ticket must be back at zero after every call.
    20 calls at B = 4097 (257 workgroups) with changing inputs, interleaved with calls at B = 17; every sum against float64,
    and a repeat of the same inputs bit for bit (the partials are added in a fixed order)."""
    gen = torch.Generator().manual_seed(4097)
    vals = {}
    for it in range(20):
        for B in (4097, 17):
            parts = [torch.randn(B, w, generator=gen) * (1 + it % 3) for w in (16, 5, 16)]
            dparts = [p.to(dev) for p in parts]
            _, val = ops.concat_sumsq(dparts, 0.5)
            _, ref, r32 = _cat_ref(parts, 0.5)
            assert_close(val, ref.reshape(1), what=f"ticket call {it} B={B}", reduced=True, ref32=r32.reshape(1))
            _, val2 = ops.concat_sumsq(dparts, 0.5)
            assert_bit_exact(val2, val, what=f"ticket repeat {it} B={B}")
            if it in (0, 19):
                vals.setdefault(B, []).append((dparts, val.clone()))
    for B, runs in vals.items():
        _, again = ops.concat_sumsq(runs[0][0], 0.5)
        assert_bit_exact(again, runs[0][1], what=f"ticket first inputs again B={B}")


def test_concat_sumsq_ticket_graph_replay(dev):
    """Captured in a hipGraph and replayed 10 times with new inputs: the ticket resets itself between replays."""
    B = 4097
    gen = torch.Generator().manual_seed(7)
    static = [torch.zeros(B, w, device=dev) for w in (16, 5, 16)]
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s), torch.no_grad():
        ops.concat_sumsq(static, 0.25)                  # the workspace of this B exists before the capture
    torch.cuda.current_stream().wait_stream(s)
    graph = torch.cuda.CUDAGraph()
    with torch.no_grad(), torch.cuda.graph(graph):
        out, val = ops.concat_sumsq(static, 0.25)
    first = None
    for it in range(10):
        parts = [torch.randn(B, w, generator=gen) * (it + 1) for w in (16, 5, 16)]
        for st_, p in zip(static, parts):
            st_.copy_(p)
        graph.replay()
        torch.cuda.synchronize()
        cat, ref, r32 = _cat_ref(parts, 0.25)
        assert_bit_exact(out, cat.float(), what=f"graph concat {it}")
        assert_close(val, ref.reshape(1), what=f"graph sumsq {it}", reduced=True, ref32=r32.reshape(1))
        if it == 0:
            first = (parts, val.clone())
    for st_, p in zip(static, first[0]):
        st_.copy_(p)
    graph.replay()
    torch.cuda.synchronize()
    assert_bit_exact(val, first[1], what="graph replay of the first inputs")
    # an eager call after the replays sees a clean ticket too
    _, val_e = ops.concat_sumsq(static, 0.25)
    assert_bit_exact(val_e, first[1], what="eager after replays")


def test_concat_sumsq_empty_batch(dev):
    """B = 0: one workgroup, no rows; the sum is exactly 0 and the call returns."""
    parts = [torch.empty(0, w, device=dev) for w in (16, 5)]
    out, val = ops.concat_sumsq(parts, 3.0)
    torch.cuda.synchronize()
    assert tuple(out.shape) == (0, 21)
    assert float(val) == 0.0
    # a following call at B = 1 is unaffected
    p1 = [torch.full((1, 16), 2.0, device=dev), torch.full((1, 5), 1.0, device=dev)]
    _, v1 = ops.concat_sumsq(p1, 3.0)
    assert float(v1) == 3.0 * (16 * 4.0 + 5 * 1.0)
