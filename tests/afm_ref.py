"""AFM's attention network restated from the reference (algorithm/AFM/afm.py:162-188) in torch, differentiated by autograd, in
float64 (the yardstick) or float32 (the reference arithmetic's own rounding).  The reference of tests/test_gpu_afm.py; results
are computed once per case and shared."""
import functools

import torch


def pair_index(F):
    """The pairs (i, j), i < j, in the order of afm.py:162-164 -> two index lists of length F (F - 1) / 2."""
    ii = [i for i in range(F) for j in range(i + 1, F)]
    jj = [j for i in range(F) for j in range(i + 1, F)]
    return ii, jj


def attention(fields, w, bias, h):
    """fields [B, F, K], w [K, t], bias [t], h [t, 1] -> (out [B, K], a [B, P], the scores s [B, P])"""
    ii, jj = pair_index(fields.shape[1])
    pairs = fields[:, ii, :] * fields[:, jj, :]                      # afm.py:162-165  (batch, P, K)
    att = torch.relu(torch.matmul(pairs, w) + bias)                  # afm.py:179-180
    att = torch.matmul(att, h)                                       # afm.py:181      (batch, P, 1)
    score = torch.softmax(att, dim=1)                                # afm.py:182
    return (pairs * score).sum(1), score.squeeze(-1), att.squeeze(-1)    # afm.py:185-186


def inputs(B, F, K, t, seed=0, bias=None, h=None, h_scale=1.0):
    """The float32 inputs of a case on the host: fields, w, bias, h [t, 1] and the output gradient g.  `bias` / `h`: that constant
    in every element; h_scale multiplies a random h."""
    gen = torch.Generator().manual_seed(1000 * F + 10 * K + t + seed)
    rnd = lambda *s: torch.randn(*s, generator=gen)
    x = {"fields": rnd(B, F, K), "w": rnd(K, t) / K ** 0.5, "bias": rnd(t) * 0.3, "h": rnd(t, 1) * (h_scale / t ** 0.5), "g": rnd(B, K)}
    if bias is not None:
        x["bias"] = torch.full((t,), float(bias))
    if h is not None:
        x["h"] = torch.full((t, 1), float(h))
    return x


@functools.lru_cache(maxsize=None)
def case(B, F, K, t, seed=0, bias=None, h=None, h_scale=1.0):
    """-> (inputs, ref64, ref32): each ref a dict out, a, s (the scores), d_fields, dw, dbias, dh.  Cached: treat as read-only."""
    x = inputs(B, F, K, t, seed, bias, h, h_scale)
    refs = []
    for dtype in (torch.float64, torch.float32):
        v = {k: x[k].clone().to(dtype).requires_grad_(k != "g") for k in x}      # (clones: the inputs stay plain tensors)
        out, a, s = attention(v["fields"], v["w"], v["bias"], v["h"])
        out.backward(v["g"])
        refs.append({"out": out.detach(), "a": a.detach(), "s": s.detach(), "d_fields": v["fields"].grad, "dw": v["w"].grad,
                     "dbias": v["bias"].grad, "dh": v["h"].grad})
    return x, refs[0], refs[1]


NAMES = ("out", "d_fields", "dw", "dbias", "dh")
# The two cases of large scores.  One fp32 ulp of a score of 1000 is 6e-5, and the softmax turns an error of a score into a
# relative error of that size in a, out and every gradient: no fp32 arithmetic meets rtol 1e-5 against float64 there, the float32
# restatement included (tests/test_afm_host.py counts what it leaves outside).  They are judged with the floor the protocol
# uses where the reference arithmetic's own fp32 deviation is the yardstick (tests/golden_protocol.py judge_step_against_oracle):
# 4 x max |ref32 - ref64| of the tensor.
LARGE_SCORES = {"bias = 1, h = 5": dict(B=67, F=9, K=16, t=128, bias=1.0, h=5.0),
                "scores beyond +-200": dict(B=33, F=7, K=8, t=12, h_scale=450.0)}


def fp32_floor(r64, r32, k):
    """4 x the largest deviation of the float32 restatement from the float64 one in tensor k"""
    return 4.0 * float((r32[k].double() - r64[k]).abs().max())


def outside_rtol(a, ref, reduced=False, rtol=1e-5):
    """how many elements of a lie outside tests.util.assert_close's bound rtol * (|ref| + rms(ref)) [+ 1e-6 max|ref|]"""
    a, ref = a.double().reshape(-1), ref.double().reshape(-1)
    tol = rtol * (ref.abs() + ref.pow(2).mean().sqrt()) + (1e-6 * ref.abs().max() if reduced else 0.0)
    return int(((a - ref).abs() > tol).sum())
