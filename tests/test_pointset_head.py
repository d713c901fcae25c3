"""Fused point head (csrc/point_head.hip, nova_pointcloud_amd/point_head.py): the reference's
self.output_proj = nn.Linear(embed_dim, 3) (transformer_pointcloud_nova.py :444, :512-515, :611, :778-781) under
GradientGuard(max_grad_norm=15.0) (train_newloss.py :34-43, :681-684, :782) as one HIP forward and one HIP backward that read
x in float32, bfloat16 or float16 as it is.

restate() is the definition of include/nova_hip.h (nova_pointset_head, nova_pointset_head_bwd and the sums over the clouds) in
float64 from the inputs as they are (a 16-bit x is exact in float64), with closed-form gradients. The CPU tests hold it
against literal_form(), the torch ops of the reference (F.linear and a clamp hook), and against torch autograd of it; the
GPU tests hold the kernels against it.

BOUNDS, written before the first GPU run, by count from restate()'s float64 quantities. u = 2^-24; a sum of n terms added in
any order with one rounding each is off by at most n u times the sum of the magnitudes (first order; the counts below
carry the slack for the second).
    out       (E + 2) u (sum_e |x W| + |bias|)    E products and additions in some order, the bias, slack
    gx        (C + 1) u sum_c |g W|               one multiplication and C - 1 fused multiply-adds, slack; for a 16-bit x the
                                                  one rounding to its type on top: half an ulp of that type at gx, and for
                                                  f16 2^-25, half the subnormal spacing. Half an ulp of a format of p
                                                  significant bits at a value in [2^k, 2^(k+1)) is 2^(k-p): 2^(k-8) for bf16
                                                  and 2^(k-11) for f16, between 2^-9 |gx| and 2^-8 |gx| (2^-12 and 2^-11).
                                                  The figures 2^-9 |gx| and 2^-12 |gx| are its lower end only: torch's own
                                                  correctly rounded cast of the float32 gradient reaches 1.61 times them on
                                                  the CPU (test_the_literal_form_in_float32_lies_inside_the_bounds), so the
                                                  bound takes the half ulp of gx's own binade, exactly
    gWs       (N + 2) u sum_i |g x|               per cloud
    gW        sum_s bound(gWs[s]) + S u sum_s sum_i |g x|
    gbs       N u sum_i |g|                       per cloud
    gbias     sum_s bound(gbs[s]) + S u sum_s sum_i |g|
plus 1e-30 times the number of terms (E, C, N, S) for intermediates flushed below 2^-126; g is the gradient after the clamp,
which is exact. The looser check against torch autograd of literal_form() on the GPU in float32 takes 4 times these
bounds: torch's graph is held to the same counts. Where every product and sum is exact in float32 (small integers) every
result is bitwise the float64 one, for a 16-bit x too.

Measured on an MI355X, worst error / bound over all cases: out 0.63, gx 0.68 for a float32 x and 1.00 for bf16 and f16
(C = 1 and 2: the rounding to the 16-bit type lands within 1e-4 of half an ulp, which the bound allows and little more), gWs 0.49,
gW 0.39, gbs 0.49, gbias 0.38; against torch, of the four-fold bound: out 0.063, gx 0 (bitwise torch's in every case), gW 0.14,
gbias 0.10; the docstring of test_random_forward_and_backward and DESIGN.md (fused point head).
"""
import ctypes
import inspect
import math
import os
import re
import subprocess
import sys

import pytest
import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if __name__ == "__main__":  # run as a script by test_abi_rejections_in_a_process_without_a_device
    sys.path.insert(0, ROOT)
from nova_pointcloud_amd import point_head as _point_head  # noqa: E402,F401  every test here is about this module: without it none passes

U = 2.0 ** -24
CHUNK = 128  # == NOVA_HEAD_CHUNK (test_header_constants_and_kernel_shape)
E_CASES = [1, 2, 3, 4, 5, 7, 8, 9, 63, 64, 65, 255, 256, 257, 511, 512, 513, 768, 1024, 4095, 4096]
N_CASES = [1, 2, 3, CHUNK - 1, CHUNK, CHUNK + 1, 2 * CHUNK + 1]
C_CASES = [1, 2, 3, 4, 6, 8]
DTYPES = [torch.float32, torch.bfloat16, torch.float16]
GUARD = 15.0  # the reference's GradientGuard
BITS = {torch.bfloat16: 8, torch.float16: 11}  # significant bits
NAME = {torch.float32: "f32", torch.bfloat16: "bf16", torch.float16: "f16"}


def literal_form(x, W, bias=None, clamp=None):
    """The reference's torch ops: F.linear, with GradientGuard's hook (torch.clamp of the incoming gradient) when clamp is given."""
    out = F.linear(x.to(W.dtype), W, bias)
    if clamp is not None and out.requires_grad:
        out.register_hook(lambda g: torch.clamp(g, -clamp, clamp))
    return out


def restate(x, W, bias=None, g=None, clamp=None):
    """The definition in float64 from the inputs as they are. x [S, N, E] (any dtype), W [C, E], bias [C]. Returns a dict:
    out [S, N, C] and M (its sum of magnitudes); with g [S, N, C] also gx [S, N, E], gWs [S, C, E], gW, gbs [S, C], gbias and
    the sums of magnitudes the bounds need. clamp: g is clamped to [-clamp, clamp] first (exact; NaN stays NaN)."""
    xd, Wd = x.double(), W.double()
    out, M = xd @ Wd.T, xd.abs() @ Wd.abs().T
    if bias is not None:
        out, M = out + bias.double(), M + bias.double().abs()
    res = {"out": out, "M": M}
    if g is None:
        return res
    gd = g.double()
    if clamp is not None:
        gd = torch.clamp(gd, -clamp, clamp)
    res.update(gx=gd @ Wd, m_gx=gd.abs() @ Wd.abs(), gWs=gd.transpose(1, 2) @ xd, m_gWs=gd.abs().transpose(1, 2) @ xd.abs(), gbs=gd.sum(1),
               m_gbs=gd.abs().sum(1))
    res.update(gW=res["gWs"].sum(0), gbias=res["gbs"].sum(0))
    return res


def half_ulp(v, dtype):
    """Half an ulp of `dtype` at each |v| in [2^k, 2^(k+1)): 2^(k - p) for p significant bits; 0 for float32 and at v = 0."""
    if dtype == torch.float32:
        return torch.zeros_like(v)
    exponent = torch.frexp(v.abs())[1]  # |v| = m 2^exponent with m in [0.5, 1): k = exponent - 1
    return torch.where(v == 0, torch.zeros_like(v), torch.ldexp(torch.ones_like(v), exponent - 1 - BITS[dtype]))


def bounds(r, S, N, C, E, dtype=torch.float32):
    """The docstring's bounds for every quantity of restate(); dtype is x's."""
    b = {"out": (E + 2) * U * r["M"] + 1e-30 * (E + 2)}
    if "gx" in r:
        b["gx"] = (C + 1) * U * r["m_gx"] + 1e-30 * C + half_ulp(r["gx"], dtype) + (2.0 ** -25 if dtype == torch.float16 else 0.0)
        b["gWs"] = (N + 2) * U * r["m_gWs"] + 1e-30 * N
        b["gW"] = b["gWs"].sum(0) + S * U * r["m_gWs"].sum(0) + 1e-30 * S
        b["gbs"] = N * U * r["m_gbs"] + 1e-30 * N
        b["gbias"] = b["gbs"].sum(0) + S * U * r["m_gbs"].sum(0) + 1e-30 * S
    return b


def random_case(S, N, C, E, magnitude, seed, dtype=torch.float32, g_scale=1.0):
    """x and bias at `magnitude` (x in `dtype`, kept inside f16's range), W at 1, g at g_scale."""
    gen = torch.Generator().manual_seed(seed)
    rnd = lambda *shape: torch.randn(*shape, generator=gen)
    x = (rnd(S, N, E) * magnitude).clamp(-6e4, 6e4).to(dtype)
    return dict(x=x, W=rnd(C, E), bias=rnd(C) * magnitude, g=rnd(S, N, C) * g_scale)


def integer_case(S, N, C, E, seed, dtype=torch.float32):
    """Small integers: every product, every forward sum and every gradient sum is exact in float32 (|sums| < 2^24), and every
    gx (|gx| <= 8 * 4 * 4 = 128) is exact in bf16 and f16."""
    gen = torch.Generator().manual_seed(seed)
    ints = lambda lo, hi, *shape: torch.randint(lo, hi + 1, shape, generator=gen).float()
    return dict(x=ints(-3, 3, S, N, E).to(dtype), W=ints(-4, 4, C, E), bias=ints(-8, 8, C), g=ints(-4, 4, S, N, C))


# ---- CPU -------------------------------------------------------------------------------------------------------------------


@pytest.mark.parametrize("C,E", [(1, 1), (3, 5), (3, 96), (8, 257)])
def test_restatement_against_float64_autograd_of_the_literal_form(C, E):
    """Values and the three closed-form gradients against autograd of F.linear(x, W, b) in float64, with and without the clamp
    hook (g at 30: about six in ten entries are clamped at 15)."""
    for S, N in ((1, 1), (2, 5), (3, CHUNK + 1)):
        for clamp in (None, GUARD):
            case = {k: v.double() for k, v in random_case(S, N, C, E, 3.0, 100 * N + E, g_scale=30.0).items()}
            leaves = {k: case[k].clone().requires_grad_(True) for k in ("x", "W", "bias")}
            out = literal_form(**leaves, clamp=clamp)
            out.backward(case["g"])
            r = restate(**case, clamp=clamp)
            if clamp is not None:
                assert (case["g"].abs() > clamp).any() and not torch.equal(r["gx"], restate(**case)["gx"])
            for got, want in ((r["out"], out.detach()), (r["gx"], leaves["x"].grad), (r["gW"], leaves["W"].grad), (r["gbias"], leaves["bias"].grad)):
                assert (got - want).abs().max() <= 1e-11 * (1 + want.abs().max()), (C, E, S, N, clamp)


@pytest.mark.parametrize("C,E", [(1, 6), (3, 96), (3, 768), (8, 257), (3, 4096)])
def test_the_literal_form_in_float32_lies_inside_the_bounds(C, E):
    """F.linear and its autograd in float32 on the CPU, with the clamp hook, sit inside every bound around restate(), at both
    magnitudes of the GPU cases; for a bf16 or f16 x the gradient of x is torch's float32 one cast once. The reference alone
    is well inside what the kernel is held to."""
    S, N = 2, 9
    for dtype in DTYPES:
        for magnitude in (1.0, 1e4):
            case = random_case(S, N, C, E, magnitude, 17 + E, dtype, g_scale=10.0)
            r = restate(**case, clamp=GUARD)
            b = bounds(r, S, N, C, E, dtype)
            leaves = {k: case[k].clone().requires_grad_(True) for k in ("x", "W", "bias")}
            out = literal_form(**leaves, clamp=GUARD)
            out.backward(case["g"])
            assert out.dtype == torch.float32 and leaves["x"].grad.dtype == dtype
            for name, got in (("out", out.detach()), ("gx", leaves["x"].grad), ("gW", leaves["W"].grad), ("gbias", leaves["bias"].grad)):
                ratio = ((got.double() - r[name]).abs() / b[name]).max().item()
                assert ratio <= 1.0, (C, E, dtype, magnitude, name, ratio)


def test_restatement_hand_cases():
    x = torch.tensor([[[1.0, 2.0]], [[-3.0, 4.0]]])  # two clouds of one point, E = 2
    W = torch.tensor([[1.0, 0.5], [-2.0, 1.0], [0.0, 4.0]])  # C = 3
    r = restate(x, W)
    assert torch.equal(r["out"], torch.tensor([[[2.0, 0.0, 8.0]], [[-1.0, 10.0, 16.0]]], dtype=torch.float64))
    assert torch.equal(r["M"], torch.tensor([[[2.0, 4.0, 8.0]], [[5.0, 10.0, 16.0]]], dtype=torch.float64))
    bias = torch.tensor([10.0, 20.0, 30.0])
    g = torch.tensor([[[1.0, -20.0, 3.0]], [[0.5, 2.0, 100.0]]])
    r = restate(x, W, bias, g)
    assert torch.equal(r["out"][0, 0], torch.tensor([12.0, 20.0, 38.0], dtype=torch.float64))
    assert torch.equal(r["gx"], torch.tensor([[[41.0, -7.5]], [[-3.5, 402.25]]], dtype=torch.float64))
    assert torch.equal(r["gWs"][0], torch.tensor([[1.0, 2.0], [-20.0, -40.0], [3.0, 6.0]], dtype=torch.float64))
    assert torch.equal(r["gbs"], g[:, 0].double()) and torch.equal(r["gbias"], torch.tensor([1.5, -18.0, 103.0], dtype=torch.float64))
    c = restate(x, W, bias, g, clamp=15.0)  # -20 -> -15, 100 -> 15
    assert torch.equal(c["gbias"], torch.tensor([1.5, -13.0, 18.0], dtype=torch.float64)) and torch.equal(c["out"], r["out"])
    assert torch.equal(c["gx"], torch.tensor([[[31.0, -2.5]], [[-3.5, 62.25]]], dtype=torch.float64))
    assert math.isnan(restate(x, W, bias, torch.full_like(g, math.nan), clamp=15.0)["gbias"][0].item())  # torch.clamp keeps a NaN
    assert torch.equal(restate(x.bfloat16(), W)["out"], r["out"] - bias.double())  # a 16-bit x is taken as it is
    # half an ulp: 8 significant bits for bf16, 11 for f16; constant over a binade, 0 at 0 and for float32
    v = torch.tensor([1.0, 1.99, 2.0, -3.0, 0.0, 0.75], dtype=torch.float64)
    assert torch.equal(half_ulp(v, torch.bfloat16), torch.tensor([2.0 ** -8, 2.0 ** -8, 2.0 ** -7, 2.0 ** -7, 0.0, 2.0 ** -9], dtype=torch.float64))
    assert torch.equal(half_ulp(v, torch.float16), half_ulp(v, torch.bfloat16) / 8) and not half_ulp(v, torch.float32).any()
    assert (torch.tensor([1.0 + 2.0 ** -8]).bfloat16().double() - (1.0 + 2.0 ** -8)).abs().item() == 2.0 ** -8  # a tie: the cast is off by all of it


def test_python_argument_errors_in_the_stated_order():
    from nova_pointcloud_amd import hip, point_head as ph

    fn = ph.point_head
    x, W = torch.zeros(2, 5, 12), torch.zeros(3, 12)
    bad = [
        (dict(x=[1.0], weight=None), "x: expected a tensor"),  # types before anything else, x first
        (dict(x=x, weight=None), "weight: expected a tensor"),
        (dict(x=x.long(), weight=W, bias=3.0), "bias: expected a tensor"),  # types before dtypes
        (dict(x=x.long(), weight=W.reshape(12, 3)), "x: expected a floating dtype"),  # dtypes before shapes
        (dict(x=x, weight=W.int()), "weight: expected a floating dtype"),
        (dict(x=x, weight=W, bias=torch.zeros(3).int()), "bias: expected a floating dtype"),
        (dict(x=torch.zeros(5, 12), weight=W), r"x: expected \[S, N, E\]"),
        (dict(x=x, weight=torch.zeros(3, 11)), r"weight: expected \[C, 12\]"),
        (dict(x=x, weight=torch.zeros(12)), r"weight: expected \[C, 12\]"),
        (dict(x=x, weight=W, bias=torch.zeros(4)), r"bias: expected \[3\]"),
        (dict(x=torch.zeros(2, 0, 5000), weight=torch.zeros(9, 5000)), "1 .. 8 outputs per point"),  # shapes before ranges; C, then E, then N
        (dict(x=torch.zeros(2, 0, 0), weight=torch.zeros(0, 0)), "1 .. 8 outputs per point"),
        (dict(x=torch.zeros(2, 0, ph.HEAD_MAX_DIM + 1), weight=torch.zeros(3, ph.HEAD_MAX_DIM + 1)), "1 .. 4096 channels"),
        (dict(x=torch.zeros(2, 0, 0), weight=torch.zeros(3, 0)), "1 .. 4096 channels"),
        (dict(x=torch.zeros(2, 0, 12), weight=W, grad_clamp=-1.0), "1 .. 65536 points"),  # ranges before grad_clamp
        (dict(x=torch.zeros(1, ph.HEAD_MAX_POINTS + 1, 1), weight=torch.zeros(3, 1), max_clouds_per_launch=0), "1 .. 65536 points"),
        (dict(x=x, weight=W, grad_clamp=0.0, max_clouds_per_launch=0), "grad_clamp must be None or a positive finite number"),  # before max_clouds_per_launch
        (dict(x=x, weight=W, grad_clamp=-15.0), "grad_clamp must be None or a positive finite number"),
        (dict(x=x, weight=W, grad_clamp=math.inf), "grad_clamp must be None or a positive finite number"),
        (dict(x=x, weight=W, grad_clamp=math.nan), "grad_clamp must be None or a positive finite number"),
        (dict(x=x, weight=W, grad_clamp=True), "grad_clamp must be None or a positive finite number"),
        (dict(x=x, weight=W, grad_clamp="15"), "grad_clamp must be None or a positive finite number"),
        (dict(x=x, weight=W, max_clouds_per_launch=0), "max_clouds_per_launch must be an integer >= 1"),
        (dict(x=x, weight=W, max_clouds_per_launch=1.5), "max_clouds_per_launch must be an integer >= 1"),
    ]
    for kwargs, message in bad:
        with pytest.raises(ValueError, match=message):
            fn(**kwargs)
    if torch.cuda.is_available():  # devices come after the ranges and before grad_clamp
        with pytest.raises(ValueError, match="x and weight must be on the same device"):
            fn(x.cuda(), W, grad_clamp=-1.0)
    for kwargs in (dict(x=x, weight=W), dict(x=x.bfloat16(), weight=W, bias=torch.zeros(3), grad_clamp=15.0, max_clouds_per_launch=1),
                   dict(x=x.double(), weight=W.half(), grad_clamp=15)):
        with pytest.raises(hip.NovaHipError, match="runs on the GPU"):  # everything else passed: CPU tensors are refused last
            fn(**kwargs)
    with pytest.raises(hip.NovaHipError, match="runs on the GPU"):
        ph.PointHead(12, 3)(x)
    with pytest.raises(ValueError, match="x: expected a tensor"):
        ph.PointHead(12, 3)(None)
    with pytest.raises(ValueError, match=r"weight: expected \[C, 12\]"):
        ph.PointHead(13, 3)(x)


def abi_checks():
    """Every error of the two entries, in the order include/nova_hip.h states, before any device work. Run by
    test_abi_rejections_in_a_process_without_a_device in a child process that sees no GPU: the calls carry addresses of
    nothing, and a build that lost a check would launch on them; without a device that launch fails with a return code."""
    sys.path.insert(0, ROOT)
    from nova_pointcloud_amd import hip, point_head as ph

    lib = hip.load(check_device=False)
    MB = 1 << 28  # pointers far apart: never dereferenced, rejected first
    x, W, bias, out, g, gx, gWs, gbs, ws = (ctypes.c_void_p(MB * i) for i in range(1, 10))
    fwd = lambda S, N, C, E, dtype=0, x=x, W=W, bias=bias, out=out: lib.nova_pointset_head(x, dtype, W, bias, out, S, N, C, E, None)
    bwd = lambda S, N, C, E, dtype=0, x=x, W=W, g=g, gx=gx, gWs=gWs, gbs=gbs, ws=ws, clamp=0.0: lib.nova_pointset_head_bwd(
        x, dtype, W, g, clamp, gx, gWs, gbs, ws, S, N, C, E, None)
    err = lib.nova_last_error
    SHAPE, ARG = -2, -1
    for fn, who in ((fwd, b"pointset_head: "), (bwd, b"pointset_head_bwd: ")):
        # null pointers first: before the dtype, before every range, also without clouds
        for name in ("x", "W"):
            assert fn(70000, 0, 0, 0, dtype=7, **{name: None}) == ARG and err() == who + b"null pointer " + name.encode(), (name, err())
            assert fn(0, 8, 3, 12, **{name: None}) == ARG and err().endswith(b"null pointer " + name.encode())
        # then the dtype code
        for code in (-1, 3, 7):
            assert fn(70000, 0, 0, 0, dtype=code) == ARG and err().startswith(who + b"unknown dtype code"), (code, err())
        # then the ranges: C, E, N, S
        for dtype in (0, 1, 2):
            for C in (0, -1, ph.HEAD_MAX_OUT + 1):
                assert fn(70000, 0, C, 0, dtype=dtype) == SHAPE and b"NOVA_HEAD_MAX_OUT" in err() and err().startswith(who), C
                assert fn(0, 8, C, 12, dtype=dtype) == SHAPE  # also without clouds
            for E in (0, -1, ph.HEAD_MAX_DIM + 1):
                assert fn(70000, 0, 3, E, dtype=dtype) == SHAPE and b"NOVA_HEAD_MAX_DIM" in err(), E
                assert fn(0, 8, 3, E, dtype=dtype) == SHAPE
            for N in (0, -1, ph.HEAD_MAX_POINTS + 1):
                assert fn(70000, N, 3, 12, dtype=dtype) == SHAPE and b"NOVA_HEAD_MAX_POINTS" in err(), N
                assert fn(0, N, 3, 12, dtype=dtype) == SHAPE
            assert fn(65536, 8, 3, 12, dtype=dtype) == SHAPE and b"65535" in err()
            assert fn(0, 8, 3, 12, dtype=dtype) == 0 and fn(-3, 65536, 8, 4096, dtype=dtype) == 0  # S <= 0 after these
    assert fwd(2, 8, 3, 12, out=None) == ARG and err().endswith(b"null pointer out")
    assert fwd(0, 8, 3, 12, out=None) == ARG and fwd(2, 8, 3, 12, out=None, bias=None) == ARG and err().endswith(b"null pointer out")  # bias may be NULL
    assert fwd(0, 8, 3, 12, bias=None) == 0
    assert bwd(2, 8, 3, 12, g=None) == ARG and err().endswith(b"null pointer g")
    assert bwd(0, 8, 3, 12, gx=None, gWs=None, gbs=None, ws=None) == 0  # S <= 0 returns before the outputs are looked at
    assert bwd(0, 8, 3, 12, x=None, gWs=None) == 0  # x serves gWs alone
    assert bwd(2, 8, 3, 12, x=None) == ARG and err().endswith(b"null pointer x")
    assert bwd(2, 8, 3, 12, gx=None, gWs=None, gbs=None) == ARG and b"no gradient wanted" in err() and b"all NULL" in err()
    assert bwd(2, 8, 3, 12, gx=None, gWs=None, gbs=None, g=None) == ARG and b"null pointer g" in err()  # the null check comes first
    assert bwd(2, 8, 3, 12, ws=None) == ARG and b"workspace ws" in err()
    assert bwd(2, 8, 3, 12, ws=None, gWs=None) == ARG and b"workspace ws" in err()  # gbs alone needs it too
    assert bwd(2, 8, 3, 12, ws=None, gbs=None) == ARG and b"workspace ws" in err()
    assert bwd(2, 8, 3, 12, ws=None, gx=None, gWs=None, gbs=None) == ARG and b"no gradient wanted" in err()  # in that order
    # an output must not overlap an input or another output: checked last (no call here passes every check: what passes
    # them launches, and these pointers are not memory)
    at = lambda p, off: ctypes.c_void_p(p.value + off)
    n_out = 2 * 8 * 3 * 4
    for dtype, es in ((0, 4), (1, 2), (2, 2)):
        for name, p, size in (("x", x, 2 * 8 * 12 * es), ("W", W, 3 * 12 * 4), ("bias", bias, 3 * 4)):
            assert fwd(2, 8, 3, 12, dtype=dtype, out=p) == ARG and err().endswith(b"out overlaps the input " + name.encode()), (name, err())
            assert fwd(2, 8, 3, 12, dtype=dtype, out=at(p, size - 4)) == ARG and err().endswith(b"out overlaps the input " + name.encode())  # its last bytes
            assert fwd(2, 8, 3, 12, dtype=dtype, out=at(p, -n_out + 4)) == ARG and b"overlaps" in err()  # the last float of out on its first
    assert fwd(70000, 8, 3, 12, out=x) == SHAPE  # a shape error still comes first
    for name, p in (("x", x), ("W", W), ("g", g)):
        for oname in ("gx", "gWs", "gbs", "ws"):
            assert bwd(2, 8, 3, 12, **{oname: p}) == ARG and err().endswith(f"{oname} overlaps the input {name}".encode()), (name, oname, err())
    assert bwd(2, 8, 3, 12, gWs=gx) == ARG and err().endswith(b"gx and gWs overlap each other")
    assert bwd(2, 8, 3, 12, gbs=gx) == ARG and err().endswith(b"gx and gbs overlap each other")
    assert bwd(2, 8, 3, 12, ws=gx) == ARG and err().endswith(b"gx and ws overlap each other")
    assert bwd(2, 8, 3, 12, gbs=at(gWs, 2 * 3 * 12 * 4 - 4)) == ARG and err().endswith(b"gWs and gbs overlap each other")  # the last float of gWs
    assert bwd(2, 8, 3, 12, ws=at(gbs, 2 * 3 * 4 - 4)) == ARG and err().endswith(b"gbs and ws overlap each other")
    assert bwd(2, 8, 3, 12, gx=at(ws, 2 * 1 * 3 * 13 * 4 - 4)) == ARG and err().endswith(b"gx and ws overlap each other")  # the last float of the workspace, C (E + 1) per chunk
    assert bwd(2, 8, 3, 12, gbs=gx, ws=None) == ARG and b"workspace" in err()  # before the overlap check
    assert lib.nova_version() == hip.ABI_VERSION  # no version bump
    print("abi checks passed")


def test_abi_rejections_in_a_process_without_a_device():
    env = dict(os.environ, HIP_VISIBLE_DEVICES="-1", CUDA_VISIBLE_DEVICES="-1", ROCR_VISIBLE_DEVICES="-1")
    out = subprocess.run([sys.executable, os.path.abspath(__file__), "--abi-checks"], env=env, capture_output=True, text=True, timeout=300, cwd=ROOT)
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-2000:]
    assert out.stdout.strip().endswith("abi checks passed"), out.stdout[-2000:]


def test_header_constants_and_kernel_shape():
    from nova_pointcloud_amd import hip, point_head as ph

    header = open(os.path.join(ROOT, "include", "nova_hip.h")).read()
    const = lambda name: int(re.search(r"#define " + name + r" (\d+)", header).group(1))
    assert const("NOVA_HEAD_MAX_OUT") == ph.HEAD_MAX_OUT == 8
    assert const("NOVA_HEAD_MAX_DIM") == ph.HEAD_MAX_DIM == 4096
    assert const("NOVA_HEAD_MAX_POINTS") == ph.HEAD_MAX_POINTS == 65536
    assert const("NOVA_HEAD_CHUNK") == ph.HEAD_CHUNK == CHUNK
    assert const("NOVA_HEAD_MAX_DIM") * const("NOVA_HEAD_MAX_OUT") <= const("NOVA_EMBED_MAX_DIM") * const("NOVA_EMBED_MAX_IN")  # the cloud sum's contract fits
    for needle in (":444", ":512-515", ":611", ":778-781", ":34-43", ":681-684", ":782", ":469", "ascending chunk order", "No atomics",
                   "((w0 + w1) + w2) + w3", "512 b + 8 l + j", "round-to-nearest-even", "torch.clamp"):
        assert needle in header, needle
    names = ("nova_pointset_head", "nova_pointset_head_bwd")
    for name in names:
        assert name in hip.SIGNATURES and re.search(r"\bint " + name + r"\(", header), name
    source = open(os.path.join(ROOT, "nova_pointcloud_amd", "csrc", "point_head.hip")).read()
    assert "HD_CHUNK = NOVA_HEAD_CHUNK;" in source and "HD_MAX_E = NOVA_HEAD_MAX_DIM;" in source
    assert "HD_MAX_N = NOVA_HEAD_MAX_POINTS;" in source and "HD_MAX_C = NOVA_HEAD_MAX_OUT;" in source
    assert int(re.search(r"HD_T = (\d+);", source).group(1)) == 256  # the header's four waves per chunk
    assert int(re.search(r"HD_BLOCK = (\d+);", source).group(1)) == 512 and int(re.search(r"HD_LANE = (\d+);", source).group(1)) == 8  # its channel blocks
    assert "#pragma clang fp contract(off)" in source
    for name in names:  # the file defines its own entry points, with their checks
        assert re.search(r"\bint " + name + r"\(", source), name
    # the file defines no summing kernel of its own: the chunk merge is fused_common.h's ordered_sum_kernel, and the sum over
    # the clouds is point_embed.hip's entry point, called from Python
    assert re.findall(r"void (\w+_kernel)\(", source) == ["head_fwd_kernel", "head_bwd_kernel"]
    assert '#include "fused_common.h"' in source and "ordered_sum(st, part, gWs, gbs," in source and "sum_clouds" not in source
    capi = open(os.path.join(ROOT, "nova_pointcloud_amd", "csrc", "capi.hip")).read()
    assert "pointset_head" not in capi
    code = re.sub(r"//.*", "", source)
    assert "atomic" not in code.lower() and "__fdividef" not in code and "__expf" not in code
    makefile = open(os.path.join(ROOT, "nova_pointcloud_amd", "csrc", "Makefile")).read()
    assert "point_head.hip" in re.search(r"^SRCS := (.*)$", makefile, flags=re.M).group(1).split()
    assert "fast-math" not in makefile and "ffast" not in makefile


def test_module_is_the_reference_head():
    from nova_pointcloud_amd import point_head as ph

    cls = ph.PointHead
    params = inspect.signature(cls.__init__).parameters
    assert list(params) == ["self", "embed_dim", "point_dim", "grad_clamp"]
    assert (params["embed_dim"].default, params["point_dim"].default, params["grad_clamp"].default) == (768, 3, None)
    assert list(inspect.signature(cls.forward).parameters) == ["self", "x"]
    assert list(inspect.signature(ph.point_head).parameters) == ["x", "weight", "bias", "grad_clamp", "max_clouds_per_launch"]
    for kwargs, (E, C) in ((dict(), (768, 3)), (dict(embed_dim=96, point_dim=6, grad_clamp=15.0), (96, 6))):
        m = cls(**kwargs)
        sd = m.state_dict()
        assert sorted(sd) == ["output_proj.bias", "output_proj.weight"]  # the reference's names (:444, :611)
        assert sorted(n for n, _ in m.named_parameters()) == ["output_proj.bias", "output_proj.weight"] and not list(m.buffers())
        assert isinstance(m.output_proj, torch.nn.Linear) and m.grad_clamp == kwargs.get("grad_clamp")
        assert sd["output_proj.weight"].shape == (C, E) and sd["output_proj.bias"].shape == (C,)
        assert all(v.dtype == torch.float32 for v in sd.values())
        # a checkpoint of the reference's own layer loads
        ref = {"output_proj.weight": torch.randn(C, E), "output_proj.bias": torch.randn(C)}
        m.load_state_dict(ref)
        assert all(torch.equal(m.state_dict()[k], ref[k]) for k in ref)
    assert "GPU" in cls.__doc__ and ":444" in cls.__doc__ and "GradientGuard" in cls.__doc__


# ---- GPU -------------------------------------------------------------------------------------------------------------------


def nan(*shape, dtype=torch.float32):
    return torch.full(shape, math.nan, dtype=dtype, device="cuda")


def ptr(t):
    return t.data_ptr() if t is not None else None


def guarded(dtype, rows, E, shift=0):
    """A NaN-filled buffer of `dtype` holding rows * E elements between two guard rows, `shift` elements further on: returns
    (the view [rows * E], the whole buffer, the slice bounds)."""
    buf = nan((rows + 2) * E + shift, dtype=dtype)
    lo, hi = E + shift, (rows + 1) * E + shift
    return buf[lo:hi], buf, (lo, hi)


def abi_forward(hip, x, W, bias=None, per=None):
    """nova_pointset_head called directly (x in its own dtype, contiguous). out lies between two guard rows in one NaN-filled
    buffer: returns (out [S, N, C], everything of the buffer outside out)."""
    S, N, E = x.shape
    C = W.shape[0]
    flat, buf, (lo, hi) = guarded(torch.float32, S * N, C)
    out = flat.view(S, N, C)
    per = S if per is None else per
    for s0 in range(0, S, per):
        hip.call("nova_pointset_head", x[s0].data_ptr(), hip.dtype_code(x.dtype), W.data_ptr(), ptr(bias), out[s0].data_ptr(), min(per, S - s0), N, C, E,
                 hip.stream_ptr())
    return out, torch.cat([buf[:lo], buf[hi:]])


def abi_backward(hip, x, W, g, clamp=0.0, want=("gx", "gWs", "gbs"), per=None, shift=0):
    """nova_pointset_head_bwd and the two cloud sums called directly, outputs pre-filled with NaN, gx between two guard rows
    (`shift` elements off): a dict of gx, gWs, gW, gbs, gbias (None where not wanted) and guard (gx's surroundings)."""
    S, N, E = x.shape
    C = W.shape[0]
    chunks = (N + CHUNK - 1) // CHUNK
    gx = guard = None
    if "gx" in want:
        flat, buf, (lo, hi) = guarded(x.dtype, S * N, E, shift)
        gx, guard = flat.view(S, N, E), (buf, lo, hi)
    gWs = nan(S, C, E) if "gWs" in want else None
    gbs = nan(S, C) if "gbs" in want else None
    per = S if per is None else per
    ws = nan(min(per, S) * chunks * C * (E + 1)) if gWs is not None or gbs is not None else None
    at = lambda t, s0: t[s0].data_ptr() if t is not None else None
    stream = hip.stream_ptr()
    for s0 in range(0, S, per):
        hip.call("nova_pointset_head_bwd", x[s0].data_ptr() if gWs is not None else None, hip.dtype_code(x.dtype), W.data_ptr(), g[s0].data_ptr(), clamp,
                 at(gx, s0), at(gWs, s0), at(gbs, s0), ptr(ws), min(per, S - s0), N, C, E, stream)
    gW = gbias = None
    if gWs is not None:
        gW = nan(C, E)
        hip.call("nova_pointset_embed_sum_clouds", gWs.data_ptr(), gW.data_ptr(), S, C * E, stream)
    if gbs is not None:
        gbias = nan(C)
        hip.call("nova_pointset_embed_sum_clouds", gbs.data_ptr(), gbias.data_ptr(), S, C, stream)
    if guard is not None:
        buf, lo, hi = guard
        guard = torch.cat([buf[:lo], buf[hi:]])
    return dict(gx=gx, gWs=gWs, gW=gW, gbs=gbs, gbias=gbias, guard=guard)


GRADS = ("gx", "gWs", "gW", "gbs", "gbias")


def same_bits(a, b):
    if a.dtype != b.dtype or a.shape != b.shape:
        return False
    as_int = torch.int32 if a.dtype == torch.float32 else torch.int16
    return torch.equal(a.contiguous().view(as_int), b.contiguous().view(as_int))


def shapes_of(E):
    """(N, S, C) of one E: every N of N_CASES with S walking 1, 3, 2 and C walking C_CASES at the small E; at the large E the
    chunk boundaries and the single row only (not the full cross product)."""
    ns = N_CASES if E <= 1024 else [1, CHUNK - 1, CHUNK + 1, 2 * CHUNK + 1]
    return [(N, (1, 3, 2)[(n + E) % 3], C_CASES[(n + E) % len(C_CASES)]) for n, N in enumerate(ns)]


def to_gpu(case):
    return {k: v.cuda() for k, v in case.items()}


@pytest.mark.gpu
@pytest.mark.parametrize("E", E_CASES)
def test_exact(hip, E):
    """Small-integer x, W, bias and g (every sum exact in float32, every gx exact in bf16 and f16), x in each dtype: out and all
    gradients bitwise the float64 result, every output pre-filled with NaN and nothing written outside out and gx (guard
    rows). With the bias present the output is bitwise the torch float32 add onto the result without it; through point_head
    the same bits."""
    from nova_pointcloud_amd import point_head as ph

    for n, (N, S, C) in enumerate(shapes_of(E)):
        for dtype in DTYPES:
            case = integer_case(S, N, C, E, 3 * E + N, dtype)
            d = to_gpu(case)
            r = restate(**case)
            where = (E, N, S, C, dtype)
            out, guard = abi_forward(hip, d["x"], d["W"], d["bias"])
            assert torch.isnan(guard).all() and same_bits(out.cpu(), r["out"].float() + 0.0), where  # a zero is +0: every sum starts there
            plain, guard = abi_forward(hip, d["x"], d["W"], per=1)
            assert torch.isnan(guard).all() and same_bits(out, plain + d["bias"]), where
            assert same_bits(ph.point_head(d["x"], d["W"], d["bias"]), out), where
            got = abi_backward(hip, d["x"], d["W"], d["g"])
            assert torch.isnan(got["guard"].float()).all(), where
            assert got["gx"].dtype == dtype and torch.equal(got["gx"].cpu(), r["gx"].to(dtype)), where  # by value: a sum of products may be -0
            for name in GRADS[1:]:
                assert same_bits(got[name].cpu(), r[name].float() + 0.0), (where, name)


WORST = {}


def check(name, got, want, bound, where):
    """Every entry within its bound; the worst error / bound of the quantity is kept for the report."""
    assert torch.isfinite(got.float()).all(), (name, where)
    ratio = ((got.double() - want).abs() / bound.expand_as(want)).max().item()
    WORST[name] = max(WORST.get(name, 0.0), ratio)
    print(f"head {where} {name}: error / bound {ratio:.4g} (worst so far {WORST[name]:.4g})")
    assert ratio <= 1.0, (name, where, ratio)


@pytest.mark.gpu
@pytest.mark.parametrize("E", E_CASES)
def test_random_forward_and_backward(hip, E):
    """Random inputs, x in each dtype, at magnitudes 1 and 1e4 (alternating with the case and the dtype), g at 10 under the
    reference's clamp of 15: out and all five gradients against restate() within bounds() of the module docstring; also
    against torch autograd of literal_form() on the GPU in float32 at 4 times the bounds; each gradient wanted alone is
    bitwise the same as when all are wanted.
    Measured on an MI355X, worst error / bound over all cases: out 0.63, gx 0.66 (float32 x; 0.68 in
    test_both_sides_of_the_grid_size_threshold), 1.00 (bf16) and 1.00 (f16), gWs 0.49, gW 0.39, gbs 0.49, gbias 0.38; against torch,
    of the four-fold bound: out 0.063, gx 0 (bitwise torch's in every case), gW 0.14, gbias 0.10 (fused point head)."""
    for n, (N, S, C) in enumerate(shapes_of(E)):
        for k, dtype in enumerate(DTYPES):
            magnitude = (1.0, 1e4)[(n + k) % 2]
            case = random_case(S, N, C, E, magnitude, 7 * E + 3 * N + k, dtype, g_scale=10.0)
            d = to_gpu(case)
            where = f"E={E} N={N} S={S} C={C} {NAME[dtype]} magnitude={magnitude:g}"
            r = restate(**case, clamp=GUARD)
            b = bounds(r, S, N, C, E, dtype)
            out, _ = abi_forward(hip, d["x"], d["W"], d["bias"])
            check("out", out.cpu(), r["out"], b["out"], where)
            got = abi_backward(hip, d["x"], d["W"], d["g"], clamp=GUARD)
            for name in GRADS:
                check(f"{name} {NAME[dtype]}" if name == "gx" else name, got[name].cpu(), r[name], b[name], where)
            if k == n % 3:
                for alone in ("gx", "gWs", "gbs"):
                    only = abi_backward(hip, d["x"], d["W"], d["g"], clamp=GUARD, want=(alone,), per=1)
                    for name in GRADS:
                        assert (only[name] is None) if name not in (alone, {"gWs": "gW", "gbs": "gbias"}.get(alone)) else same_bits(only[name], got[name]), (where, alone, name)
            leaves = {name: d[name].clone().requires_grad_(True) for name in ("x", "W", "bias")}
            ref = literal_form(**leaves, clamp=GUARD)
            ref.backward(d["g"])
            check("out vs torch", out.cpu(), ref.detach().cpu().double(), 4 * b["out"], where)
            for name, leaf in (("gx", "x"), ("gW", "W"), ("gbias", "bias")):
                check(name + " vs torch", got[name].cpu(), leaves[leaf].grad.cpu().double(), 4 * b[name], where)


def headed(case, per=None, clamp=None, names=("x", "W", "bias")):
    """(out, then the gradients of the tensors in `names`) through point_head under sum(out g)."""
    from nova_pointcloud_amd import point_head as ph

    leaves = {k: (case[k].clone().requires_grad_(True) if k in names else case[k]) for k in ("x", "W", "bias")}
    out = ph.point_head(leaves["x"], leaves["W"], leaves["bias"], grad_clamp=clamp, max_clouds_per_launch=per)
    out.backward(case["g"])
    return [out.detach()] + [leaves[k].grad for k in names]


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16], ids=["bf16", "f16"])
def test_a_sixteen_bit_x_gives_the_bits_of_its_float32_cast(hip, dtype):
    """point_head(x16) is bitwise point_head(x16.float()), its gradient of x is bitwise the float32 one cast once, and the
    gradients of the weight and the bias are bitwise the same: the dtype path changes no sum. E on both sides of a block and
    at the flagship width; g large enough that f16 overflows to infinity where torch's cast does."""
    for (S, N, C, E), g_scale in (((2, CHUNK + 1, 3, 768), 1.0), ((3, 5, 8, 513), 1.0), ((1, 9, 4, 7), 1.0), ((2, 3, 3, 260), 3e4)):
        case = to_gpu(random_case(S, N, C, E, 3.0, 41 + E, dtype, g_scale))
        low = headed(case, clamp=None)
        full = headed(dict(case, x=case["x"].float()))
        assert low[1].dtype == dtype and full[1].dtype == torch.float32
        assert same_bits(low[0], full[0]) and same_bits(low[1], full[1].to(dtype)), (dtype, E)
        assert same_bits(low[2], full[2]) and same_bits(low[3], full[3]), (dtype, E)
        if g_scale > 1.0 and dtype == torch.float16:
            assert torch.isinf(low[1]).any() and not torch.isinf(full[1]).any()  # beyond 65504: inf, as torch's cast


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", DTYPES, ids=["f32", "bf16", "f16"])
def test_the_clamp_is_exact_and_keeps_a_nan(hip, dtype):
    """The clamped backward is bitwise the unclamped backward fed g.clamp(-t, t); a NaN in g stays a NaN in gx, in its cloud's
    gWs and gbs and in the sums over the clouds, and nowhere else; the forward does not depend on the clamp."""
    S, N, C, E = 3, CHUNK + 2, 3, 520
    case = to_gpu(random_case(S, N, C, E, 2.0, 59, dtype, g_scale=20.0))
    x, W, g = case["x"], case["W"], case["g"]
    assert (g.abs() > GUARD).any() and (g.abs() < GUARD).any()
    for t in (GUARD, 0.5):
        got, want = abi_backward(hip, x, W, g, clamp=t), abi_backward(hip, x, W, torch.clamp(g, -t, t))
        for name in GRADS:
            assert same_bits(got[name], want[name]), (t, name)
    plain = abi_backward(hip, x, W, g)
    for t in (0.0, -1.0, math.nan):  # no clamp
        got = abi_backward(hip, x, W, g, clamp=t)
        assert all(same_bits(got[name], plain[name]) for name in GRADS), t
    assert not same_bits(plain["gx"], abi_backward(hip, x, W, g, clamp=GUARD)["gx"])
    a, b = headed(case, clamp=GUARD), headed(dict(case, g=torch.clamp(g, -GUARD, GUARD)))
    assert all(same_bits(p, q) for p, q in zip(a, b))
    bad = g.clone()
    bad[1, 7, 2] = math.nan
    got, want = abi_backward(hip, x, W, bad, clamp=GUARD), abi_backward(hip, x, W, g, clamp=GUARD)
    assert torch.isnan(got["gx"][1, 7].float()).all() and torch.isnan(got["gWs"][1, 2]).all() and torch.isnan(got["gbs"][1, 2])
    assert torch.isnan(got["gW"][2]).all() and torch.isnan(got["gbias"][2])
    keep = torch.ones(S, N, dtype=torch.bool, device="cuda")
    keep[1, 7] = False
    assert same_bits(got["gx"][keep], want["gx"][keep]) and same_bits(got["gWs"][:, :2], want["gWs"][:, :2]) and same_bits(got["gWs"][0], want["gWs"][0])
    assert same_bits(got["gW"][:2], want["gW"][:2]) and same_bits(got["gbias"][:2], want["gbias"][:2]) and same_bits(got["gbs"][[0, 2]], want["gbs"][[0, 2]])


@pytest.mark.gpu
@pytest.mark.parametrize("C,E,dtype", [(3, 7, torch.float32), (8, 516, torch.bfloat16), (3, 768, torch.float16)])
def test_bitwise_reproducible(hip, C, E, dtype):
    """The output and all three gradients bit for bit the same for max_clouds_per_launch 1, 2, S and default, in two runs; per
    cloud for clouds moved to other batch positions and for a cloud run alone (the gradients of W and bias are sums over the
    clouds in their order, so they are compared through their per-cloud parts)."""
    S, N = 5, 2 * CHUNK + 1
    case = to_gpu(random_case(S, N, C, E, 3.0, 23 + E, dtype, g_scale=10.0))
    ref = headed(case, None, GUARD)
    for per in (1, 2, S, None):
        for a, b in zip(ref, headed(case, per, GUARD)):
            assert same_bits(a, b), (E, per)
    raw_out = abi_forward(hip, case["x"], case["W"], case["bias"])[0]
    raw = abi_backward(hip, case["x"], case["W"], case["g"], clamp=GUARD)
    assert same_bits(ref[0], raw_out) and same_bits(ref[1], raw["gx"]) and same_bits(ref[2], raw["gW"]) and same_bits(ref[3], raw["gbias"])
    perm = torch.tensor([3, 0, 4, 1, 2], device="cuda")
    moved_case = dict(case, x=case["x"][perm].contiguous(), g=case["g"][perm].contiguous())
    moved = headed(moved_case, 2, GUARD)
    assert same_bits(ref[0][perm], moved[0]) and same_bits(ref[1][perm], moved[1])
    raw_moved = abi_backward(hip, moved_case["x"], case["W"], moved_case["g"], clamp=GUARD, per=2)
    assert same_bits(raw["gWs"][perm], raw_moved["gWs"]) and same_bits(raw["gbs"][perm], raw_moved["gbs"])
    for s in range(S):
        alone = headed(dict(case, x=case["x"][s:s + 1], g=case["g"][s:s + 1]), None, GUARD)
        assert same_bits(ref[0][s:s + 1], alone[0]) and same_bits(ref[1][s:s + 1], alone[1])
        assert same_bits(alone[2], raw["gWs"][s] + 0.0) and same_bits(alone[3], raw["gbs"][s] + 0.0)  # one cloud: +0 + its part


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", DTYPES, ids=["f32", "bf16", "f16"])
def test_pointers_off_alignment_give_the_same_bits(hip, dtype):
    """x and gx that start one, two, ... elements off a 16-byte boundary, and an odd E, take the narrower accesses (8, 4 and, for
    the 16-bit types, 2 bytes): the same bits as the aligned call, forward and backward, and nothing written outside gx."""
    per16 = 16 // torch.empty(0, dtype=dtype).element_size()
    for C, E in ((3, 520), (6, 263), (3, 768), (2, 5)):
        S, N = 2, CHUNK + 1
        case = to_gpu(random_case(S, N, C, E, 3.0, 31 + E, dtype, g_scale=10.0))
        x, W, g = case["x"], case["W"], case["g"]

        def off(t, elems):  # the same values, `elems` elements further on from a 16-byte boundary
            buf = torch.cat([t.new_zeros(elems), t.flatten()])
            assert buf.data_ptr() % 16 == 0
            return buf[elems:].view(t.shape)

        assert x.data_ptr() % 16 == 0
        want = abi_forward(hip, x, W, case["bias"])[0]
        want_g = abi_backward(hip, x, W, g, clamp=GUARD)
        assert want_g["gx"].data_ptr() % 16 == (E * x.element_size()) % 16
        for elems in (1, 2, 3, per16 // 2, per16 - 1):
            moved = off(x, elems)
            assert moved.data_ptr() % 16 == elems * x.element_size()
            assert same_bits(abi_forward(hip, moved, W, case["bias"])[0], want), (E, elems)
            got = abi_backward(hip, moved, W, g, clamp=GUARD, shift=elems)  # gx shifted as well
            assert torch.isnan(got["guard"].float()).all(), (E, elems)
            for name in GRADS:
                assert same_bits(got[name], want_g[name]), (E, elems, name)
            got = abi_backward(hip, x, W, g, clamp=GUARD, shift=elems, want=("gx",))  # gx alone off the boundary
            assert torch.isnan(got["guard"].float()).all() and same_bits(got["gx"], want_g["gx"]), (E, elems)


@pytest.mark.gpu
def test_both_sides_of_the_grid_size_threshold(hip):
    """A launch of fewer than 512 workgroups takes 16 rows per workgroup in the forward and spreads the channel blocks over
    grid.z in the backward, a larger one 64 rows and walks the blocks inside the workgroup: 520 one-chunk clouds in one
    launch against launches of 100 give the same bits, forward and backward, exact against float64 for small integers and
    within the bounds for random values."""
    S, N, C, E = 520, 20, 3, 1030  # three blocks, the last one partly filled; 20 rows: one workgroup of 64 rows, two of 16
    for dtype in (torch.float32, torch.bfloat16):
        case = integer_case(S, N, C, E, 77, dtype)
        d = to_gpu(case)
        r = restate(**case)
        for per in (S, 100):
            out, guard = abi_forward(hip, d["x"], d["W"], d["bias"], per=per)
            assert torch.isnan(guard).all() and same_bits(out.cpu(), r["out"].float() + 0.0), per
            got = abi_backward(hip, d["x"], d["W"], d["g"], per=per)
            assert torch.isnan(got["guard"].float()).all() and torch.equal(got["gx"].cpu(), r["gx"].to(dtype)), per
            for name in GRADS[1:]:
                assert same_bits(got[name].cpu(), r[name].float() + 0.0), (per, name)
    case = random_case(S, N, C, E, 1.0, 78)
    d = to_gpu(case)
    r = restate(**case)
    b = bounds(r, S, N, C, E)
    whole, _ = abi_forward(hip, d["x"], d["W"], d["bias"])
    parts, _ = abi_forward(hip, d["x"], d["W"], d["bias"], per=100)
    assert same_bits(whole, parts)
    check("out", whole.cpu(), r["out"], b["out"], "grid threshold")
    g_whole = abi_backward(hip, d["x"], d["W"], d["g"])
    g_parts = abi_backward(hip, d["x"], d["W"], d["g"], per=100)
    g_some = abi_backward(hip, d["x"], d["W"], d["g"], want=("gWs", "gbs"), per=100)
    for name in GRADS:
        assert same_bits(g_whole[name], g_parts[name]), name
        assert name == "gx" or same_bits(g_whole[name], g_some[name]), name
        check(f"{name} f32" if name == "gx" else name, g_whole[name].cpu(), r[name], b[name], "grid threshold")


@pytest.mark.gpu
def test_binding_and_stats(hip):
    """Autograd returns the raw ABI results; a non-contiguous g and a strided view of x are accepted, a float64 x is cast by
    torch; what no input needs is not launched and not allocated; no_grad saves nothing and a graph saves x and the weight
    alone; every gradient has its input's dtype."""
    from nova_pointcloud_amd import point_head as ph

    S, N, C, E = 3, CHUNK + 3, 3, 260
    case = to_gpu(random_case(S, N, C, E, 3.0, 5, g_scale=10.0))
    x, W, bias, g = case["x"], case["W"], case["bias"], case["g"]
    delta = lambda before: {k: ph.stats[k] - before[k] for k in before}
    raw_out = abi_forward(hip, x, W, bias)[0]
    raw = abi_backward(hip, x, W, g, clamp=GUARD)
    got = headed(case, 2, GUARD)
    assert same_bits(got[0], raw_out) and same_bits(got[1], raw["gx"]) and same_bits(got[2], raw["gW"]) and same_bits(got[3], raw["gbias"])
    # a non-contiguous g
    wide = torch.randn(S, N, 2 * C, generator=torch.Generator().manual_seed(9)).cuda()
    g_nc = wide[:, :, ::2]
    assert not g_nc.is_contiguous()
    raw_nc = abi_backward(hip, x, W, g_nc.contiguous())
    got = headed(dict(case, g=g_nc))
    assert same_bits(got[1], raw_nc["gx"]) and same_bits(got[2], raw_nc["gW"]) and same_bits(got[3], raw_nc["gbias"])
    # a strided view of wider rows as x: made contiguous by torch, its gradient scattered back by torch
    rows = torch.randn(S, N, 2 * E, generator=torch.Generator().manual_seed(8)).cuda().requires_grad_(True)
    out = ph.point_head(rows[:, :, :E], W)
    out.backward(g)
    view = rows.detach()[:, :, :E].contiguous()
    assert same_bits(out.detach(), abi_forward(hip, view, W)[0])
    assert same_bits(rows.grad[:, :, :E].contiguous(), abi_backward(hip, view, W, g, want=("gx",))["gx"]) and (rows.grad[:, :, E:] == 0).all()
    # a float64 x goes through float32
    xd = x.double().requires_grad_(True)
    out = ph.point_head(xd, W.double(), bias.double())
    out.backward(g)
    assert out.dtype == torch.float32 and xd.grad.dtype == torch.float64 and same_bits(out.detach(), raw_out)
    assert torch.equal(xd.grad, abi_backward(hip, x, W, g, want=("gx",))["gx"].double())
    # stats: every needs_input_grad pattern
    patterns = {("x",): (1, 0), ("W",): (1, 1), ("bias",): (1, 1), ("x", "W"): (1, 1), ("x", "bias"): (1, 1), ("W", "bias"): (1, 2), ("x", "W", "bias"): (1, 2)}
    for names, (backward, sums) in patterns.items():
        before = dict(ph.stats)
        got = headed(case, 2, GUARD, names)
        assert delta(before) == {"forward_launches": 2, "backward_launches": 2 * backward, "cloud_sum_launches": sums}, names
        for k, name in enumerate(names):
            assert same_bits(got[1 + k], raw[{"x": "gx", "W": "gW", "bias": "gbias"}[name]]), (names, name)
    before = dict(ph.stats)
    ph.point_head(x, W, bias)  # nothing requires a gradient
    with torch.no_grad():
        ph.point_head(x.clone().requires_grad_(True), W, bias, max_clouds_per_launch=1)
    assert delta(before) == {"forward_launches": 4, "backward_launches": 0, "cloud_sum_launches": 0}
    # the weight alone on a long cloud: gx (8 MiB here) is not allocated
    big = torch.randn(1, 65536, 32, generator=torch.Generator().manual_seed(3)).cuda()
    W1 = torch.randn(1, 32, generator=torch.Generator().manual_seed(4)).cuda().requires_grad_(True)
    out = ph.point_head(big, W1)
    gb = torch.ones_like(out)
    torch.cuda.synchronize()
    before, allocated = dict(ph.stats), torch.cuda.memory_allocated()
    torch.cuda.reset_peak_memory_stats()
    out.backward(gb)
    torch.cuda.synchronize()
    assert delta(before) == {"forward_launches": 0, "backward_launches": 1, "cloud_sum_launches": 1}
    assert torch.cuda.max_memory_allocated() - allocated < big.numel() * 4 // 2
    # what autograd keeps: nothing without a graph, x and the weight alone with one
    kept = []
    with torch.autograd.graph.saved_tensors_hooks(lambda t: kept.append(tuple(t.shape)) or t, lambda t: t):
        with torch.no_grad():
            ph.point_head(x.clone().requires_grad_(True), W, bias)
        assert kept == []
        ph.point_head(x, W, bias)
        assert kept == []
        ph.point_head(x.clone().requires_grad_(True), W, bias.clone().requires_grad_(True), grad_clamp=GUARD)
    assert sorted(kept) == sorted([(S, N, E), (C, E)]), kept
    # gradient dtypes: each input gets a gradient of its own dtype; x's comes out of the kernel, the others are cast by torch
    for dtype in (torch.bfloat16, torch.float16):
        low = {k: case[k].to(dtype).requires_grad_(True) for k in ("x", "W", "bias")}
        out = ph.point_head(low["x"], low["W"], low["bias"], grad_clamp=GUARD)
        assert out.dtype == torch.float32
        out.backward(g)
        assert all(low[k].grad.dtype == dtype for k in low)
        W32, b32 = low["W"].detach().float(), low["bias"].detach().float()
        raw16 = abi_backward(hip, low["x"].detach(), W32, g, clamp=GUARD)
        assert same_bits(out.detach(), abi_forward(hip, low["x"].detach(), W32, b32)[0])
        assert same_bits(low["x"].grad, raw16["gx"]) and torch.equal(low["W"].grad, raw16["gW"].to(dtype)) and torch.equal(low["bias"].grad, raw16["gbias"].to(dtype))
    with pytest.raises(hip.NovaHipError, match="runs on the GPU"):
        ph.point_head(x.cpu(), W.cpu())


@pytest.mark.gpu
def test_an_empty_cloud_set(hip):
    """S = 0 launches nothing: the output and the gradient of x are empty, and the sums over the clouds (weight, bias) are +0 in
    every element, not what the allocator handed out. The allocator's free blocks of those sizes are filled with NaN first,
    so a gradient that nothing wrote would show."""
    from nova_pointcloud_amd import point_head as ph

    N, C, E = 5, 3, 12
    gen = torch.Generator().manual_seed(11)
    leaf = lambda *shape: torch.randn(*shape, generator=gen).cuda().requires_grad_(True)
    x, W, bias = leaf(0, N, E), leaf(C, E), leaf(C)
    zero_bits = lambda t, shape: t.shape == shape and t.dtype == torch.float32 and (t.view(torch.int32) == 0).all()
    for per in (None, 1):
        for t in (x, W, bias):
            t.grad = None
        dirty = [nan(*shape) for shape in ((C, E), (C,)) for _ in range(4)]
        torch.cuda.synchronize()
        del dirty
        before = dict(ph.stats)
        out = ph.point_head(x, W, bias, grad_clamp=GUARD, max_clouds_per_launch=per)
        assert out.shape == (0, N, C) and out.dtype == torch.float32
        out.backward(torch.empty(0, N, C, device="cuda"))
        assert zero_bits(W.grad, (C, E)) and zero_bits(bias.grad, (C,)) and x.grad.shape == (0, N, E)
        assert ph.stats == before  # no kernel has anything to do
    W.grad = None
    ph.point_head(x.detach().bfloat16(), W).sum().backward()
    assert zero_bits(W.grad, (C, E))
    with torch.no_grad():
        assert ph.point_head(x, W, bias).shape == (0, N, C)


@pytest.mark.gpu
def test_module_in_train_and_eval_mode(hip):
    """The parameters' gradients are the functional's, bitwise; the clamp acts in training mode only (the reference's
    GradientGuard); load_state_dict round-trips; the output is inside the forward bound."""
    from nova_pointcloud_amd import point_head as ph

    for (E, C), dtype in (((768, 3), torch.bfloat16), ((130, 6), torch.float32)):
        S, N = 2, CHUNK + 1
        case = to_gpu(random_case(S, N, C, E, 1.0, E, dtype, g_scale=20.0))
        m = ph.PointHead(E, C, grad_clamp=GUARD).cuda()
        m.load_state_dict({"output_proj.weight": case["W"], "output_proj.bias": case["bias"]})
        assert m.training
        results = {}
        for mode, clamp in (("train", GUARD), ("eval", None)):
            m.train(mode == "train")
            m.zero_grad()
            xl = case["x"].clone().requires_grad_(True)
            out = m(xl)
            out.backward(case["g"])
            want = headed(case, None, clamp)
            assert same_bits(out.detach(), want[0]) and same_bits(xl.grad, want[1]), mode
            assert same_bits(m.output_proj.weight.grad, want[2]) and same_bits(m.output_proj.bias.grad, want[3]), mode
            results[mode] = (out.detach(), xl.grad)
        assert same_bits(results["train"][0], results["eval"][0]) and not same_bits(results["train"][1], results["eval"][1])
        plain = ph.PointHead(E, C).cuda()  # no clamp asked for: training mode changes nothing
        plain.load_state_dict(m.state_dict())
        xl = case["x"].clone().requires_grad_(True)
        plain(xl).backward(case["g"])
        assert same_bits(xl.grad, results["eval"][1])
        cpu = {k: v.cpu() for k, v in case.items()}
        r = restate(**cpu)
        check("module out", results["eval"][0].cpu(), r["out"], bounds(r, S, N, C, E)["out"], f"module E={E}")


if __name__ == "__main__" and sys.argv[1:] == ["--abi-checks"]:
    abi_checks()
