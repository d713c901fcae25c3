"""Fused point embedding (csrc/point_embed.hip, nova_pointcloud_amd/point_embed.py): the reference's
point_embed = nn.Linear(point_cloud_dim, 768) with the broadcast additions that follow it (transformer_pointcloud_nova.py
:562-565, :712-716, :753-760, :772) as one HIP forward and one HIP backward.

restate() is the definition of include/nova_hip.h (nova_pointset_embed, nova_pointset_embed_bwd, _sum_clouds, _pos_bwd) in
float64 from the float32 inputs, with closed-form gradients. The CPU tests hold it against literal_form(), the torch ops of
the reference, and against torch autograd of it; the GPU tests hold the kernels against it.

BOUNDS, written before the first GPU run, by count from restate()'s float64 quantities. u = 2^-24; a sum of n terms added in
any order with one rounding each is off by at most n u times the sum of the magnitudes (first order; the counts below
carry the slack for the second).
    forward   (C + A) u M            A the number of addends present, M = sum_k |x_k W_ek| + |bias| + |pos| + |cond| + |base|:
                                     C roundings for the products, one per addend
    gx        (E + 2) u sum_e |g W|
    gWs       (N + 2) u sum_i |g x|  per cloud
    gW        sum_s bound(gWs[s]) + S u sum_s sum_i |g x|
    gcs       N u sum_i |g|          per cloud
    gbias     sum_s bound(gcs[s]) + S u sum_s sum_i |g|
    gpos      S u sum_s |g|
plus 1e-30 (times N, E or S: the number of terms) for intermediates flushed below 2^-126. The looser check against torch
autograd of literal_form() on the GPU in float32 takes 4 times these bounds: torch's graph is held to the same counts.
Where every product and sum is exact in float32 (small integers) every result is bitwise the float64 one.

Measured on an MI355X, worst error / bound over all cases: forward 0.61 with all addends and 0.98 with some (C = 1 and one
addend: two roundings against a bound of two half ulps), gx 0.44, gWs 0.54, gW 0.39, gcs 0.61, gbias 0.43, gpos 0.66; the
docstring of test_random_forward_and_backward and DESIGN.md (fused point embedding).
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
U = 2.0 ** -24
CHUNK = 128  # == NOVA_EMBED_CHUNK (test_header_constants_and_kernel_shape)
E_CASES = [1, 2, 3, 4, 5, 63, 64, 65, 255, 256, 257, 768, 1024, 4095, 4096]
N_CASES = [1, 2, 3, 4, 5, CHUNK - 1, CHUNK, CHUNK + 1, 2 * CHUNK + 1]
C_CASES = [1, 2, 3, 4, 6, 8]
ADDENDS = ("bias", "pos", "cond", "base")


def literal_form(x, W, bias=None, pos=None, cond=None, base=None):
    """The reference's torch ops: F.linear, then pos[:N], cond[:, None] and base added in that order."""
    out = F.linear(x, W, bias)
    if pos is not None:
        out = out + pos[:x.shape[1]]
    if cond is not None:
        out = out + cond[:, None]
    if base is not None:
        out = out + base
    return out


def restate(x, W, bias=None, pos=None, cond=None, base=None, g=None):
    """The definition in float64 from the inputs as they are. x [S, N, C], W [E, C], bias [E], pos [>= N, E], cond [S, E],
    base [S, N, E]. Returns a dict: out [S, N, E], M (the forward's sum of magnitudes), A (the addends present); with
    g [S, N, E] also gx, gWs [S, E, C], gW, gcs [S, E], gbias, gpos [N, E] and the sums of magnitudes the bounds need."""
    S, N, C = x.shape
    xd, Wd = x.double(), W.double()
    out, M, A = xd @ Wd.T, xd.abs() @ Wd.abs().T, 0
    for t in (bias, pos[:N] if pos is not None else None, cond[:, None] if cond is not None else None, base):
        if t is not None:
            out, M, A = out + t.double(), M + t.double().abs(), A + 1
    res = {"out": out, "M": M, "A": A}
    if g is None:
        return res
    gd = g.double()
    res.update(gx=gd @ Wd, m_gx=gd.abs() @ Wd.abs(), gWs=gd.transpose(1, 2) @ xd, m_gWs=gd.abs().transpose(1, 2) @ xd.abs(),
               gcs=gd.sum(1), m_gcs=gd.abs().sum(1), gpos=gd.sum(0), m_gpos=gd.abs().sum(0))
    res.update(gW=res["gWs"].sum(0), gbias=res["gcs"].sum(0))
    return res


def bounds(r, S, N, C, E):
    """The docstring's bounds for every quantity of restate()."""
    b = {"out": (C + r["A"]) * U * r["M"] + 1e-30 * (C + r["A"])}
    if "gx" in r:
        b["gx"] = (E + 2) * U * r["m_gx"] + 1e-30 * E
        b["gWs"] = (N + 2) * U * r["m_gWs"] + 1e-30 * N
        b["gW"] = b["gWs"].sum(0) + S * U * r["m_gWs"].sum(0)
        b["gcs"] = N * U * r["m_gcs"] + 1e-30 * N
        b["gbias"] = b["gcs"].sum(0) + S * U * r["m_gcs"].sum(0)
        b["gpos"] = S * U * r["m_gpos"] + 1e-30 * S
    return b


def random_case(S, N, C, E, magnitude, seed, rows=None):
    """x, W and the four addends at `magnitude`, g at 1; pos has `rows` >= N rows (default N + 2)."""
    gen = torch.Generator().manual_seed(seed)
    rnd = lambda *shape: torch.randn(*shape, generator=gen)
    return dict(x=rnd(S, N, C) * magnitude, W=rnd(E, C), bias=rnd(E) * magnitude, pos=rnd(N + 2 if rows is None else rows, E) * magnitude,
                cond=rnd(S, E) * magnitude, base=rnd(S, N, E) * magnitude, g=rnd(S, N, E))


def integer_case(S, N, C, E, seed):
    """Small integers: every product, every forward sum and every gradient sum is exact in float32 (|sums| < 2^24)."""
    gen = torch.Generator().manual_seed(seed)
    ints = lambda lo, hi, *shape: torch.randint(lo, hi + 1, shape, generator=gen).float()
    return dict(x=ints(-3, 3, S, N, C), W=ints(-4, 4, E, C), bias=ints(-8, 8, E), pos=ints(-8, 8, N + 1, E), cond=ints(-8, 8, S, E),
                base=ints(-8, 8, S, N, E), g=ints(-4, 4, S, N, E))


def pick(case, names):
    return {k: case[k] for k in names}


# ---- CPU -------------------------------------------------------------------------------------------------------------------


@pytest.mark.parametrize("C,E", [(1, 1), (3, 5), (3, 96), (8, 257)])
def test_restatement_against_float64_autograd_of_the_literal_form(C, E):
    """Values and all six closed-form gradients against autograd of F.linear(x, W, b) + pos[:N] + cond[:, None] + base in float64."""
    for S, N in ((1, 1), (2, 5), (3, CHUNK + 1)):
        case = {k: v.double() for k, v in random_case(S, N, C, E, 3.0, 100 * N + E).items()}
        leaves = {k: case[k].clone().requires_grad_(True) for k in ("x", "W") + ADDENDS}
        out = literal_form(**leaves)
        out.backward(case["g"])
        r = restate(**case)
        gpos = torch.zeros_like(case["pos"])
        gpos[:N] = r["gpos"]  # the rows past N get no gradient
        for got, want in ((r["out"], out.detach()), (r["gx"], leaves["x"].grad), (r["gW"], leaves["W"].grad), (r["gbias"], leaves["bias"].grad),
                          (gpos, leaves["pos"].grad), (r["gcs"], leaves["cond"].grad), (case["g"], leaves["base"].grad)):
            assert (got - want).abs().max() <= 1e-11 * (1 + want.abs().max()), (C, E, S, N)


@pytest.mark.parametrize("C,E", [(1, 6), (3, 96), (3, 768), (8, 257)])
def test_the_literal_form_in_float32_lies_inside_the_forward_bound(C, E):
    """F.linear and the adds in float32 on the CPU sit inside the forward bound around restate(), at both magnitudes of the GPU
    cases and for every subset of addends tried: the reference alone is well inside what the kernel is held to."""
    for magnitude in (1.0, 1e4):
        case = random_case(2, 9, C, E, magnitude, 17 + E)
        for names in ((), ("bias",), ("bias", "pos"), ("cond", "base"), ADDENDS):
            args = pick(case, ("x", "W") + names)
            r = restate(**args)
            ratio = ((literal_form(**args).double() - r["out"]).abs() / bounds(r, 2, 9, C, E)["out"]).max().item()
            assert ratio <= 1.0, (C, E, magnitude, names, ratio)


def test_restatement_hand_cases():
    # C = 1: an outer product; one point; absent addends are no additions
    x = torch.tensor([[[2.0]], [[-3.0]]])
    W = torch.tensor([[1.0], [0.5], [-4.0]])
    r = restate(x, W)
    assert torch.equal(r["out"], torch.tensor([[[2.0, 1.0, -8.0]], [[-3.0, -1.5, 12.0]]], dtype=torch.float64)) and r["A"] == 0
    assert torch.equal(r["M"], r["out"].abs())
    bias, pos, cond, base = torch.tensor([1.0, 1.0, 1.0]), torch.tensor([[10.0, 20.0, 30.0], [7.0, 7.0, 7.0]]), torch.tensor([[100.0] * 3, [200.0] * 3]), torch.ones(2, 1, 3)
    g = torch.tensor([[[1.0, 2.0, 3.0]], [[4.0, 5.0, 6.0]]])
    r = restate(x, W, bias, pos, cond, base, g)
    assert r["A"] == 4 and torch.equal(r["out"][0, 0], torch.tensor([114.0, 123.0, 124.0], dtype=torch.float64))
    assert torch.equal(r["out"][1, 0], torch.tensor([209.0, 220.5, 244.0], dtype=torch.float64))  # pos row 0 for both clouds, row 1 unused
    assert torch.equal(r["gx"], torch.tensor([[[1.0 + 1.0 - 12.0]], [[4.0 + 2.5 - 24.0]]], dtype=torch.float64))
    assert torch.equal(r["gWs"], torch.tensor([[[2.0], [4.0], [6.0]], [[-12.0], [-15.0], [-18.0]]], dtype=torch.float64))
    assert torch.equal(r["gW"][:, 0], torch.tensor([-10.0, -11.0, -12.0], dtype=torch.float64))
    assert torch.equal(r["gcs"], g[:, 0].double()) and torch.equal(r["gbias"], torch.tensor([5.0, 7.0, 9.0], dtype=torch.float64))
    assert torch.equal(r["gpos"], torch.tensor([[5.0, 7.0, 9.0]], dtype=torch.float64))
    only = restate(x, W, cond=cond)
    assert only["A"] == 1 and torch.equal(only["out"], restate(x, W)["out"] + cond.double()[:, None])


def test_python_argument_errors_in_the_stated_order():
    from nova_pointcloud_amd import hip, point_embed as pe

    fn = pe.point_embed
    x, W = torch.zeros(2, 5, 3), torch.zeros(12, 3)
    bad = [
        (dict(points=[1.0], weight=None), "points: expected a tensor"),  # types before anything else, points first
        (dict(points=x, weight=None), "weight: expected a tensor"),
        (dict(points=x, weight=W, bias=3.0), "bias: expected a tensor"),
        (dict(points=x, weight=W, pos=[1.0]), "pos: expected a tensor"),
        (dict(points=x, weight=W, cond=1), "cond: expected a tensor"),
        (dict(points=x.long(), weight=W, base="b"), "base: expected a tensor"),  # types before dtypes
        (dict(points=x.long(), weight=W.reshape(3, 12)), "points: expected a floating dtype"),  # dtypes before shapes
        (dict(points=x, weight=W.int()), "weight: expected a floating dtype"),
        (dict(points=x, weight=W, bias=torch.zeros(12).int()), "bias: expected a floating dtype"),
        (dict(points=x, weight=W, pos=torch.zeros(5, 12).long()), "pos: expected a floating dtype"),
        (dict(points=x, weight=W, cond=torch.zeros(2, 12).bool()), "cond: expected a floating dtype"),
        (dict(points=x, weight=W, base=torch.zeros(2, 5, 12).int()), "base: expected a floating dtype"),
        (dict(points=torch.zeros(5, 3), weight=W), r"points: expected \[S, N, C\]"),
        (dict(points=x, weight=torch.zeros(12, 4)), r"weight: expected \[E, 3\]"),
        (dict(points=x, weight=torch.zeros(12)), r"weight: expected \[E, 3\]"),
        (dict(points=x, weight=W, bias=torch.zeros(11)), r"bias: expected \[12\]"),
        (dict(points=x, weight=W, pos=torch.zeros(4, 12)), r"pos: expected \[P, 12\] or \[1, P, 12\] with P >= 5"),
        (dict(points=x, weight=W, pos=torch.zeros(2, 5, 12)), r"pos: expected \[P, 12\]"),
        (dict(points=x, weight=W, pos=torch.zeros(1, 5, 13)), r"pos: expected \[P, 12\]"),
        (dict(points=x, weight=W, cond=torch.zeros(2, 13)), r"cond: expected \[S, 12\]"),
        (dict(points=x, weight=W, cond=torch.zeros(12)), r"cond: expected \[S, 12\]"),
        (dict(points=x, weight=W, base=torch.zeros(2, 4, 12)), r"base: expected \[S, 5, 12\]"),
        (dict(points=torch.zeros(2, 5, 9), weight=torch.zeros(5000, 9), cond=torch.zeros(3, 5000)), "points and cond must hold the same number of clouds"),  # counts before ranges
        (dict(points=x, weight=W, base=torch.zeros(3, 5, 12)), "points and base must hold the same number of clouds"),
        (dict(points=torch.zeros(2, 0, 9), weight=torch.zeros(5000, 9)), "1 .. 8 inputs per point"),  # C, then E, then N
        (dict(points=torch.zeros(2, 0, 0), weight=torch.zeros(0, 0)), "1 .. 8 inputs per point"),
        (dict(points=torch.zeros(2, 0, 3), weight=torch.zeros(pe.EMBED_MAX_DIM + 1, 3)), "1 .. 4096 channels"),
        (dict(points=torch.zeros(2, 0, 3), weight=torch.zeros(0, 3)), "1 .. 4096 channels"),
        (dict(points=torch.zeros(2, 0, 3), weight=W), "1 .. 65536 points"),
        (dict(points=torch.zeros(1, pe.EMBED_MAX_POINTS + 1, 3), weight=W, max_clouds_per_launch=0), "1 .. 65536 points"),
        (dict(points=x, weight=W, max_clouds_per_launch=0), "max_clouds_per_launch must be an integer >= 1"),
        (dict(points=x, weight=W, max_clouds_per_launch=1.5), "max_clouds_per_launch must be an integer >= 1"),
    ]
    for kwargs, message in bad:
        with pytest.raises(ValueError, match=message):
            fn(**kwargs)
    if torch.cuda.is_available():  # devices come after the ranges and before max_clouds_per_launch
        with pytest.raises(ValueError, match="points and weight must be on the same device"):
            fn(x.cuda(), W, max_clouds_per_launch=0)
    for kwargs in (dict(points=x, weight=W), dict(points=x, weight=W, bias=torch.zeros(12), pos=torch.zeros(1, 9, 12), cond=torch.zeros(2, 12), base=torch.zeros(2, 5, 12))):
        with pytest.raises(hip.NovaHipError, match="runs on the GPU"):  # everything else passed: CPU tensors are refused last
            fn(**kwargs)
    with pytest.raises(hip.NovaHipError, match="runs on the GPU"):
        pe.PointEmbedding(3, 12, 8)(x)
    with pytest.raises(ValueError, match="points: expected a tensor"):
        pe.PointEmbedding(3, 12, 8)(None)
    with pytest.raises(ValueError, match="with P >= 5"):
        pe.PointEmbedding(3, 12, 4)(x)  # more points than max_points


def abi_checks():
    """Every error of the four entries, in the order include/nova_hip.h states, before any device work. Run by
    test_abi_rejections_in_a_process_without_a_device in a child process that sees no GPU: the calls carry addresses of
    nothing, and a build that lost a check would launch on them; without a device that launch fails with a return code."""
    sys.path.insert(0, ROOT)
    from nova_pointcloud_amd import hip, point_embed as pe

    lib = hip.load(check_device=False)
    MB = 1 << 28  # pointers far apart: never dereferenced, rejected first
    x, W, bias, pos, cond, base, out, g, gx, gWs, gcs, ws = (ctypes.c_void_p(MB * i) for i in range(1, 13))
    fwd = lambda S, N, C, E, x=x, W=W, bias=bias, pos=pos, cond=cond, base=base, out=out: lib.nova_pointset_embed(x, W, bias, pos, cond, base, out, S, N, C, E, None)
    bwd = lambda S, N, C, E, x=x, W=W, g=g, gx=gx, gWs=gWs, gcs=gcs, ws=ws: lib.nova_pointset_embed_bwd(x, W, g, gx, gWs, gcs, ws, S, N, C, E, None)
    err = lib.nova_last_error
    SHAPE, ARG = -2, -1
    for fn in (fwd, bwd):
        for C in (0, -1, pe.EMBED_MAX_IN + 1):
            assert fn(70000, 0, C, 0, x=None) == SHAPE and b"NOVA_EMBED_MAX_IN" in err(), C  # C first
            assert fn(0, 8, C, 12) == SHAPE  # also without clouds
        for E in (0, -1, pe.EMBED_MAX_DIM + 1):
            assert fn(70000, 0, 3, E, x=None) == SHAPE and b"NOVA_EMBED_MAX_DIM" in err(), E  # E before N
            assert fn(0, 8, 3, E) == SHAPE
        for N in (0, -1, pe.EMBED_MAX_POINTS + 1):
            assert fn(70000, N, 3, 12, x=None) == SHAPE and b"NOVA_EMBED_MAX_POINTS" in err(), N  # N before the cloud count
            assert fn(0, N, 3, 12) == SHAPE
        assert fn(65536, 8, 3, 12, x=None) == SHAPE and b"65535" in err()  # shape errors before argument errors
        assert fn(0, 8, 3, 12) == 0 and fn(-3, 65536, 8, 4096) == 0
        assert fn(0, 8, 3, 12, x=None, W=None) == 0  # S <= 0 returns before the pointers are looked at
        for name in ("x", "W"):
            assert fn(2, 8, 3, 12, **{name: None}) == ARG and err().endswith(b"null pointer " + name.encode()), (name, err())
    assert fwd(0, 8, 3, 12, out=None) == 0 and bwd(0, 8, 3, 12, g=None, gx=None, gWs=None, gcs=None, ws=None) == 0
    assert fwd(2, 8, 3, 12, out=None) == ARG and err().endswith(b"null pointer out")
    assert fwd(2, 8, 3, 12, out=None, bias=None, pos=None, cond=None, base=None) == ARG and err().endswith(b"null pointer out")  # addends may be NULL
    assert bwd(2, 8, 3, 12, g=None) == ARG and err().endswith(b"null pointer g")
    assert bwd(2, 8, 3, 12, gx=None, gWs=None, gcs=None) == ARG and b"no gradient wanted" in err() and b"all NULL" in err()
    assert bwd(2, 8, 3, 12, gx=None, gWs=None, gcs=None, g=None) == ARG and b"null pointer g" in err()  # the null check comes first
    assert bwd(2, 8, 3, 12, ws=None) == ARG and b"workspace ws" in err()
    assert bwd(2, 8, 3, 12, ws=None, gWs=None) == ARG and b"workspace ws" in err()  # gcs alone needs it too
    assert bwd(2, 8, 3, 12, ws=None, gcs=None) == ARG and b"workspace ws" in err()
    assert bwd(2, 8, 3, 12, ws=None, gx=None, gWs=None, gcs=None) == ARG and b"no gradient wanted" in err()  # in that order
    # an output must not overlap an input or another output: checked last (no call here passes every check: what passes
    # them launches, and these pointers are not memory)
    at = lambda p, off: ctypes.c_void_p(p.value + off)
    n_out = 2 * 8 * 12 * 4
    for name, p, size in (("x", x, 2 * 8 * 3 * 4), ("W", W, 12 * 3 * 4), ("bias", bias, 12 * 4), ("pos", pos, 8 * 12 * 4), ("cond", cond, 2 * 12 * 4),
                          ("base", base, n_out)):
        assert fwd(2, 8, 3, 12, out=p) == ARG and err().endswith(b"out overlaps the input " + name.encode()), (name, err())
        assert fwd(2, 8, 3, 12, out=at(p, size - 4)) == ARG and err().endswith(b"out overlaps the input " + name.encode())  # its last float
        assert fwd(2, 8, 3, 12, out=at(p, -n_out + 4)) == ARG and b"overlaps" in err()  # the last float of out on its first
    assert fwd(70000, 8, 3, 12, out=x) == SHAPE  # a shape error still comes first
    assert fwd(2, 8, 3, 12, out=None, base=x) == ARG and b"null pointer out" in err()
    for name, p in (("x", x), ("W", W), ("g", g)):
        for oname in ("gx", "gWs", "gcs", "ws"):
            assert bwd(2, 8, 3, 12, **{oname: p}) == ARG and err().endswith(f"{oname} overlaps the input {name}".encode()), (name, oname, err())
    assert bwd(2, 8, 3, 12, gWs=gx) == ARG and err().endswith(b"gx and gWs overlap each other")
    assert bwd(2, 8, 3, 12, gcs=gx) == ARG and err().endswith(b"gx and gcs overlap each other")
    assert bwd(2, 8, 3, 12, ws=gx) == ARG and err().endswith(b"gx and ws overlap each other")
    assert bwd(2, 8, 3, 12, gcs=at(gWs, 2 * 12 * 3 * 4 - 4)) == ARG and err().endswith(b"gWs and gcs overlap each other")  # the last float of gWs
    assert bwd(2, 8, 3, 12, ws=at(gcs, 2 * 12 * 4 - 4)) == ARG and err().endswith(b"gcs and ws overlap each other")
    assert bwd(2, 8, 3, 12, gcs=gx, ws=None) == ARG and b"workspace" in err()  # before the overlap check
    # the sum over the clouds
    sc = lambda S, n, a=gWs, o=gx: lib.nova_pointset_embed_sum_clouds(a, o, S, n, None)
    for n in (0, -1, pe.EMBED_MAX_DIM * pe.EMBED_MAX_IN + 1):
        assert sc(2, n, a=None) == SHAPE and b"NOVA_EMBED_MAX_DIM * NOVA_EMBED_MAX_IN" in err(), n
        assert sc(0, n) == SHAPE
    assert sc(0, 36) == 0 and sc(-1, 36, a=None, o=None) == 0
    assert sc(2, 36, a=None) == ARG and err().endswith(b"null pointer per_cloud")
    assert sc(2, 36, o=None) == ARG and err().endswith(b"null pointer out")
    assert sc(2, 36, o=gWs) == ARG and err().endswith(b"out overlaps the input per_cloud")
    assert sc(2, 36, o=at(gWs, 2 * 36 * 4 - 4)) == ARG and b"overlaps" in err()
    # the gradient of pos
    pb = lambda S, N, E, acc=0, g=g, o=gx: lib.nova_pointset_embed_pos_bwd(g, o, S, N, E, acc, None)
    assert pb(70000, 0, 0, g=None) == SHAPE and b"NOVA_EMBED_MAX_DIM" in err()
    assert pb(70000, 0, 12, g=None) == SHAPE and b"NOVA_EMBED_MAX_POINTS" in err()
    assert pb(65536, 8, 12, g=None) == SHAPE and b"65535" in err()
    assert pb(0, 8, 12) == 0 and pb(-1, 8, 12, g=None, o=None) == 0 and pb(0, 0, 12) == SHAPE
    assert pb(2, 8, 12, g=None) == ARG and err().endswith(b"null pointer g")
    assert pb(2, 8, 12, 1, o=None) == ARG and err().endswith(b"null pointer gpos")
    assert pb(2, 8, 12, o=g) == ARG and err().endswith(b"gpos overlaps the input g")
    assert pb(2, 8, 12, 1, o=at(g, 2 * 8 * 12 * 4 - 4)) == ARG and b"overlaps" in err()
    assert lib.nova_version() == hip.ABI_VERSION  # no version bump
    print("abi checks passed")


def test_abi_rejections_in_a_process_without_a_device():
    env = dict(os.environ, HIP_VISIBLE_DEVICES="-1", CUDA_VISIBLE_DEVICES="-1", ROCR_VISIBLE_DEVICES="-1")
    out = subprocess.run([sys.executable, os.path.abspath(__file__), "--abi-checks"], env=env, capture_output=True, text=True, timeout=300, cwd=ROOT)
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-2000:]
    assert out.stdout.strip().endswith("abi checks passed"), out.stdout[-2000:]


def test_header_constants_and_kernel_shape():
    from nova_pointcloud_amd import hip, point_embed as pe

    header = open(os.path.join(ROOT, "include", "nova_hip.h")).read()
    const = lambda name: int(re.search(r"#define " + name + r" (\d+)", header).group(1))
    assert const("NOVA_EMBED_MAX_IN") == pe.EMBED_MAX_IN == 8
    assert const("NOVA_EMBED_MAX_DIM") == pe.EMBED_MAX_DIM == 4096
    assert const("NOVA_EMBED_MAX_POINTS") == pe.EMBED_MAX_POINTS == 65536
    assert const("NOVA_EMBED_CHUNK") == pe.EMBED_CHUNK == CHUNK
    for needle in (":562-565", ":712-716", ":753-756", ":759-760", ":772", ":294", ":297", ":174", ":218-221", ":315-327", ":340-346",
                   "ascending chunk order", "ascending block order", "No atomics", "((w0 + w1) + w2) + w3"):
        assert needle in header, needle
    names = ("nova_pointset_embed", "nova_pointset_embed_bwd", "nova_pointset_embed_sum_clouds", "nova_pointset_embed_pos_bwd")
    for name in names:
        assert name in hip.SIGNATURES and re.search(r"\bint " + name + r"\(", header), name
    source = open(os.path.join(ROOT, "nova_pointcloud_amd", "csrc", "point_embed.hip")).read()
    assert "EM_CHUNK = NOVA_EMBED_CHUNK;" in source and "EM_MAX_E = NOVA_EMBED_MAX_DIM;" in source
    assert "EM_MAX_N = NOVA_EMBED_MAX_POINTS;" in source and "EM_MAX_C = NOVA_EMBED_MAX_IN;" in source
    assert int(re.search(r"EM_T = (\d+);", source).group(1)) == 256  # the header's four waves per chunk
    assert int(re.search(r"EM_BLOCK = (\d+);", source).group(1)) == 256  # the header's channel blocks
    assert "#pragma clang fp contract(off)" in source
    for name in names:  # each file defines its own entry points, with their checks
        assert re.search(r"\bint " + name + r"\(", source), name
    capi = open(os.path.join(ROOT, "nova_pointcloud_amd", "csrc", "capi.hip")).read()
    assert "pointset_embed" not in capi
    code = re.sub(r"//.*", "", source)
    assert "atomic" not in code.lower() and "__fdividef" not in code and "__expf" not in code
    makefile = open(os.path.join(ROOT, "nova_pointcloud_amd", "csrc", "Makefile")).read()
    assert "point_embed.hip" in re.search(r"^SRCS := (.*)$", makefile, flags=re.M).group(1).split()
    assert "fast-math" not in makefile and "ffast" not in makefile


def test_module_is_the_reference_head():
    from nova_pointcloud_amd import point_embed as pe

    cls = pe.PointEmbedding
    params = inspect.signature(cls.__init__).parameters
    assert list(params) == ["self", "point_dim", "embed_dim", "max_points"]
    assert (params["point_dim"].default, params["embed_dim"].default, params["max_points"].default) == (3, 768, 1024)
    assert list(inspect.signature(cls.forward).parameters) == ["self", "points", "cond", "base"]
    for kwargs, (C, E, P) in ((dict(), (3, 768, 1024)), (dict(point_dim=6, embed_dim=96, max_points=50), (6, 96, 50))):
        m = cls(**kwargs)
        sd = m.state_dict()
        assert sorted(sd) == ["point_embed.bias", "point_embed.weight", "pos_embed"]  # the reference's names (:562-565)
        assert sorted(n for n, _ in m.named_parameters()) == ["point_embed.bias", "point_embed.weight", "pos_embed"] and not list(m.buffers())
        assert isinstance(m.point_embed, torch.nn.Linear)
        assert sd["point_embed.weight"].shape == (E, C) and sd["point_embed.bias"].shape == (E,) and sd["pos_embed"].shape == (1, P, E)
        assert all(v.dtype == torch.float32 for v in sd.values())
        assert 0.015 < sd["pos_embed"].std().item() < 0.025  # randn * 0.02
        # a checkpoint of the reference's own layers loads
        ref = {"point_embed.weight": torch.randn(E, C), "point_embed.bias": torch.randn(E), "pos_embed": torch.randn(1, P, E)}
        m.load_state_dict(ref)
        assert all(torch.equal(m.state_dict()[k], ref[k]) for k in ref)
    assert "GPU" in cls.__doc__ and ":562-565" in cls.__doc__


# ---- GPU -------------------------------------------------------------------------------------------------------------------


def nan(*shape):
    return torch.full(shape, math.nan, dtype=torch.float32, device="cuda")


def ptr(t):
    return t.data_ptr() if t is not None else None


def abi_forward(hip, x, W, bias=None, pos=None, cond=None, base=None, per=None, shift=0):
    """nova_pointset_embed called directly on float32 GPU tensors (pos [N, E] contiguous). out lies between two guard rows in one
    NaN-filled buffer, `shift` floats further on: returns (out [S, N, E], everything of the buffer outside out)."""
    S, N, C = x.shape
    E = W.shape[0]
    buf = nan((S * N + 2) * E + shift)
    lo, hi = E + shift, (S * N + 1) * E + shift
    out = buf[lo:hi].view(S, N, E)
    per = S if per is None else per
    for s0 in range(0, S, per):
        hip.call("nova_pointset_embed", x[s0].data_ptr(), W.data_ptr(), ptr(bias), ptr(pos), cond[s0].data_ptr() if cond is not None else None,
                 base[s0].data_ptr() if base is not None else None, out[s0].data_ptr(), min(per, S - s0), N, C, E, hip.stream_ptr())
    return out, torch.cat([buf[:lo], buf[hi:]])


def abi_backward(hip, x, W, g, want=("gx", "gWs", "gcs", "gpos"), per=None):
    """nova_pointset_embed_bwd, the two cloud sums and nova_pointset_embed_pos_bwd called directly, outputs pre-filled with NaN:
    a dict of gx, gWs, gW, gcs, gbias, gpos (None where not wanted)."""
    S, N, C = x.shape
    E = W.shape[0]
    chunks = (N + CHUNK - 1) // CHUNK
    gx = nan(S, N, C) if "gx" in want else None
    gWs = nan(S, E, C) if "gWs" in want else None
    gcs = nan(S, E) if "gcs" in want else None
    gpos = nan(N, E) if "gpos" in want else None
    per = S if per is None else per
    ws = nan(min(per, S) * chunks * E * (C + 1)) if gWs is not None or gcs is not None else None
    at = lambda t, s0: t[s0].data_ptr() if t is not None else None
    stream = hip.stream_ptr()
    for s0 in range(0, S, per):
        if gx is not None or ws is not None:
            hip.call("nova_pointset_embed_bwd", x[s0].data_ptr(), W.data_ptr(), g[s0].data_ptr(), at(gx, s0), at(gWs, s0), at(gcs, s0), ptr(ws),
                     min(per, S - s0), N, C, E, stream)
        if gpos is not None:
            hip.call("nova_pointset_embed_pos_bwd", g[s0].data_ptr(), gpos.data_ptr(), min(per, S - s0), N, E, 1 if s0 else 0, stream)
    gW = gbias = None
    if gWs is not None:
        gW = nan(E, C)
        hip.call("nova_pointset_embed_sum_clouds", gWs.data_ptr(), gW.data_ptr(), S, E * C, stream)
    if gcs is not None:
        gbias = nan(E)
        hip.call("nova_pointset_embed_sum_clouds", gcs.data_ptr(), gbias.data_ptr(), S, E, stream)
    return dict(gx=gx, gWs=gWs, gW=gW, gcs=gcs, gbias=gbias, gpos=gpos)


GRADS = ("gx", "gWs", "gW", "gcs", "gbias", "gpos")


def same_bits(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


def shapes_of(E):
    """(N, S, C) of one E: every N of N_CASES with S alternating 1 and 3 and C walking C_CASES at the small E; at the large E
    the chunk boundaries and the single row only (not the full cross product)."""
    ns = N_CASES if E <= 1024 else [1, CHUNK - 1, CHUNK + 1, 2 * CHUNK + 1]
    return [(N, (1, 3)[(n + E) % 2], C_CASES[(n + E) % len(C_CASES)]) for n, N in enumerate(ns)]


def on_gpu(case, N):
    """The case's tensors on the GPU as the ABI takes them: pos cut to its first N rows."""
    dev = {k: v.cuda() for k, v in case.items()}
    dev["pos"] = dev["pos"][:N].contiguous()
    return dev


@pytest.mark.gpu
@pytest.mark.parametrize("E", E_CASES)
def test_exact(hip, E):
    """Small-integer x, W, addends and g (every sum exact in float32): out and all gradients bitwise the float64 result, every
    output pre-filled with NaN and nothing written outside out (guard rows). Each addend present is bitwise the torch float32
    add onto the result without it, through the ABI and through point_embed."""
    from nova_pointcloud_amd import point_embed as pe

    for N, S, C in shapes_of(E):
        case = integer_case(S, N, C, E, 3 * E + N)
        d = on_gpu(case, N)
        r = restate(**case)
        where = (E, N, S, C)
        out, guard = abi_forward(hip, d["x"], d["W"], d["bias"], d["pos"], d["cond"], d["base"])
        assert torch.isnan(guard).all() and same_bits(out.cpu(), r["out"].float() + 0.0), where  # a zero is +0: -0 + bias
        assert same_bits(abi_forward(hip, d["x"], d["W"], d["bias"], d["pos"], d["cond"], d["base"], per=1)[0], out), where
        assert same_bits(pe.point_embed(d["x"], d["W"], d["bias"], case["pos"].cuda(), d["cond"], d["base"]), out), where  # pos with rows to spare
        # the chain of addends, one more each time: a float32 torch add onto the result without it
        have, prev = {}, abi_forward(hip, d["x"], d["W"])[0]
        assert torch.equal(prev.cpu(), restate(case["x"], case["W"])["out"].float()), where  # by value: with no addend a -0 stays -0
        for name, add in (("bias", d["bias"]), ("pos", d["pos"]), ("cond", d["cond"][:, None]), ("base", d["base"])):
            have[name] = d[name]
            got, guard = abi_forward(hip, d["x"], d["W"], **have)
            assert torch.isnan(guard).all() and same_bits(got, prev + add), (where, name)
            prev = got
        for name, add in (("pos", d["pos"]), ("cond", d["cond"][:, None]), ("base", d["base"])):  # each one alone
            assert same_bits(abi_forward(hip, d["x"], d["W"], **{name: d[name]})[0], abi_forward(hip, d["x"], d["W"])[0] + add), (where, name)
        got = abi_backward(hip, d["x"], d["W"], d["g"])
        for name in GRADS:
            assert same_bits(got[name].cpu(), r[name].float() + 0.0), (where, name)  # a zero is +0: every sum starts there


@pytest.mark.gpu
@pytest.mark.parametrize("C,E", [(3, 12), (6, 260), (3, 768)])
def test_pointers_off_sixteen_and_eight_bytes_give_the_same_bits(hip, C, E):
    """out, base, pos and g that start 8 bytes (E % 4 == 0: the rows would otherwise move 16 bytes per lane) or 4 bytes off a
    16-byte boundary take the narrower accesses: the same bits, forward and backward, and nothing written outside out."""
    S, N = 3, CHUNK + 1
    case = random_case(S, N, C, E, 3.0, 31 + E)
    d = on_gpu(case, N)

    def off(t, floats):  # the same values, `floats` floats further on from a 16-byte boundary
        buf = torch.cat([t.new_zeros(floats), t.flatten()])
        assert buf.data_ptr() % 16 == 0
        return buf[floats:].view(t.shape)

    want, _ = abi_forward(hip, d["x"], d["W"], d["bias"], d["pos"], d["cond"], d["base"])
    want_g = abi_backward(hip, d["x"], d["W"], d["g"])
    assert want.data_ptr() % 16 == (4 * E) % 16 and d["base"].data_ptr() % 16 == 0 and d["g"].data_ptr() % 16 == 0
    for floats in (2, 1, 3):
        assert off(d["base"], floats).data_ptr() % 16 == 4 * floats
        assert same_bits(abi_forward(hip, d["x"], d["W"], d["bias"], d["pos"], d["cond"], off(d["base"], floats))[0], want), floats
        assert same_bits(abi_forward(hip, d["x"], d["W"], d["bias"], off(d["pos"], floats), d["cond"], d["base"])[0], want), floats
        got, guard = abi_forward(hip, d["x"], d["W"], d["bias"], d["pos"], d["cond"], d["base"], shift=floats)
        assert got.data_ptr() % 16 == (4 * E + 4 * floats) % 16 and same_bits(got, want) and torch.isnan(guard).all(), floats
        got_g = abi_backward(hip, d["x"], d["W"], off(d["g"], floats))
        for name in GRADS:
            assert same_bits(got_g[name], want_g[name]), (floats, name)


WORST = {}


def check(name, got, want, bound, where):
    """Every entry within its bound; the worst error / bound of the quantity is kept for the report."""
    assert torch.isfinite(got).all(), (name, where)
    ratio = ((got.double() - want).abs() / bound.expand_as(want)).max().item()
    WORST[name] = max(WORST.get(name, 0.0), ratio)
    print(f"embed {where} {name}: error / bound {ratio:.4g} (worst so far {WORST[name]:.4g})")
    assert ratio <= 1.0, (name, where, ratio)


@pytest.mark.gpu
@pytest.mark.parametrize("E", E_CASES)
def test_random_forward_and_backward(hip, E):
    """Random inputs at magnitudes 1 and 1e4, with all addends and with a varying subset: out and all six gradients against
    restate() within bounds() of the module docstring; also against torch autograd of literal_form() on the GPU in float32 at
    4 times the bounds; each gradient wanted alone is bitwise the same as when all are wanted.
    Measured on an MI355X, worst error / bound over all cases: out 0.61 (0.98 with a subset of the addends, at C = 1 with one
    addend, where the bound is two half ulps for two roundings), gx 0.44, gWs 0.47, gW 0.39, gcs 0.60, gbias 0.43, gpos 0.66
    (gWs 0.54 and gcs 0.61 in test_both_sides_of_the_block_split); against torch, of the four-fold bound: out 0 and gpos 0 (bitwise torch's in every case), gx 0.070, gW 0.155, gbias 0.145,
    gcs 0.042 (fused point embedding)."""
    subsets = ((), ("bias", "pos"), ("cond",), ("base",), ("bias", "cond", "base"))
    for n, (N, S, C) in enumerate(shapes_of(E)):
        for m, magnitude in enumerate((1.0, 1e4)):
            case = random_case(S, N, C, E, magnitude, 7 * E + 3 * N + m)
            d = on_gpu(case, N)
            where = f"E={E} N={N} S={S} C={C} magnitude={magnitude:g}"
            r = restate(**case)
            b = bounds(r, S, N, C, E)
            out, _ = abi_forward(hip, d["x"], d["W"], d["bias"], d["pos"], d["cond"], d["base"])
            check("out", out.cpu(), r["out"], b["out"], where)
            names = subsets[(n + m) % len(subsets)]
            rs = restate(**pick(case, ("x", "W") + names))
            out_s, _ = abi_forward(hip, d["x"], d["W"], **pick(d, names))
            check("out (some addends)", out_s.cpu(), rs["out"], bounds(rs, S, N, C, E)["out"], where)
            got = abi_backward(hip, d["x"], d["W"], d["g"])
            for name in GRADS:
                check(name, got[name].cpu(), r[name], b[name], where)
            if m == 0:
                for alone in ("gx", "gWs", "gcs", "gpos"):
                    only = abi_backward(hip, d["x"], d["W"], d["g"], want=(alone,), per=1)
                    for name in GRADS:
                        assert (only[name] is None) if name not in (alone, {"gWs": "gW", "gcs": "gbias"}.get(alone)) else same_bits(only[name], got[name]), (where, alone, name)
            leaves = {k: d[k].clone().requires_grad_(True) for k in ("x", "W") + ADDENDS}
            ref = literal_form(**leaves)
            ref.backward(d["g"])
            check("out vs torch", out.cpu(), ref.detach().cpu().double(), 4 * b["out"], where)
            for name, leaf in (("gx", "x"), ("gW", "W"), ("gbias", "bias"), ("gpos", "pos"), ("gcs", "cond")):
                check(name + " vs torch", got[name].cpu(), leaves[leaf].grad.cpu().double(), 4 * b[name], where)


def embedded(case, per, names=ADDENDS):
    """(out, then the gradients of x, W and the addends in `names`) through point_embed under sum(out g)."""
    from nova_pointcloud_amd import point_embed as pe

    leaves = {k: case[k].clone().requires_grad_(True) for k in ("x", "W") + tuple(names)}
    out = pe.point_embed(leaves["x"], leaves["W"], **{k: leaves[k] for k in names}, max_clouds_per_launch=per)
    out.backward(case["g"])
    return [out.detach()] + [leaves[k].grad for k in ("x", "W") + tuple(names)]


@pytest.mark.gpu
@pytest.mark.parametrize("C,E", [(3, 7), (8, 132), (3, 768)])
def test_bitwise_reproducible(hip, C, E):
    """The output and all six gradients bit for bit the same for max_clouds_per_launch 1, 2, S and default, in two runs; per
    cloud for clouds moved to other batch positions and for a cloud run alone (the gradients of W, bias and pos are sums over
    the clouds in their order, so they are compared through their per-cloud parts)."""
    S, N = 5, 2 * CHUNK + 1
    case = {k: v.cuda() for k, v in random_case(S, N, C, E, 3.0, 23 + E).items()}
    ref = embedded(case, None)
    for per in (1, 2, S, None):
        for a, b in zip(ref, embedded(case, per)):
            assert same_bits(a, b), (E, per)
    pos = case["pos"][:N].contiguous()
    raw = abi_backward(hip, case["x"], case["W"], case["g"])
    assert same_bits(ref[1], raw["gx"]) and same_bits(ref[2], raw["gW"]) and same_bits(ref[3], raw["gbias"])
    assert same_bits(ref[4][:N], raw["gpos"]) and (ref[4][N:] == 0).all() and same_bits(ref[5], raw["gcs"]) and same_bits(ref[6], case["g"])
    perm = torch.tensor([3, 0, 4, 1, 2], device="cuda")
    moved_case = dict(case, x=case["x"][perm], cond=case["cond"][perm], base=case["base"][perm], g=case["g"][perm])
    moved = embedded(moved_case, 2)
    for k in (0, 1, 5, 6):  # out, the gradients of x, cond and base: per cloud
        assert same_bits(ref[k][perm], moved[k]), k
    raw_moved = abi_backward(hip, moved_case["x"].contiguous(), case["W"], moved_case["g"].contiguous(), per=2)
    assert same_bits(raw["gWs"][perm], raw_moved["gWs"]) and same_bits(raw["gcs"][perm], raw_moved["gcs"])
    for s in range(S):
        one = {k: (v[s:s + 1] if k in ("x", "cond", "base", "g") else v) for k, v in case.items()}
        alone = embedded(one, None)
        assert same_bits(ref[0][s:s + 1], alone[0]) and same_bits(ref[1][s:s + 1], alone[1]) and same_bits(ref[5][s:s + 1], alone[5])
        assert same_bits(alone[2], raw["gWs"][s] + 0.0) and same_bits(alone[3], raw["gcs"][s] + 0.0)  # one cloud: +0 + its part
        assert same_bits(alone[4][:N], case["g"][s] + 0.0)


@pytest.mark.gpu
def test_both_sides_of_the_block_split(hip):
    """A launch of fewer than 512 workgroups spreads the channel blocks over grid.z (the backward only when gx is not wanted), a
    larger one walks them inside the workgroup: 520 one-chunk clouds in one launch (no split) against launches of 100 (split)
    give the same bits, forward and backward, exact against float64 for small integers and within the bounds for random values."""
    S, N, C, E = 520, 3, 3, 600  # three blocks, the last one partly filled
    case = integer_case(S, N, C, E, 77)
    d = on_gpu(case, N)
    r = restate(**case)
    for per in (S, 100):
        out, guard = abi_forward(hip, d["x"], d["W"], d["bias"], d["pos"], d["cond"], d["base"], per=per)
        assert torch.isnan(guard).all() and same_bits(out.cpu(), r["out"].float() + 0.0), per
        got = abi_backward(hip, d["x"], d["W"], d["g"], want=("gWs", "gcs"), per=per)
        for name in ("gWs", "gW", "gcs", "gbias"):
            assert same_bits(got[name].cpu(), r[name].float() + 0.0), (per, name)
    case = random_case(S, N, C, E, 1.0, 78)
    d = on_gpu(case, N)
    r = restate(**case)
    b = bounds(r, S, N, C, E)
    whole, _ = abi_forward(hip, d["x"], d["W"], d["bias"], d["pos"], d["cond"], d["base"])
    parts, _ = abi_forward(hip, d["x"], d["W"], d["bias"], d["pos"], d["cond"], d["base"], per=100)
    assert same_bits(whole, parts)
    check("out", whole.cpu(), r["out"], b["out"], "block split")
    g_whole = abi_backward(hip, d["x"], d["W"], d["g"], want=("gWs", "gcs"))
    g_parts = abi_backward(hip, d["x"], d["W"], d["g"], want=("gWs", "gcs"), per=100)
    g_all = abi_backward(hip, d["x"], d["W"], d["g"], per=100)  # gx wanted: never split
    for name in ("gWs", "gW", "gcs", "gbias"):
        assert same_bits(g_whole[name], g_parts[name]) and same_bits(g_whole[name], g_all[name]), name
        check(name, g_whole[name].cpu(), r[name], b[name], "block split")


@pytest.mark.gpu
def test_binding_and_stats(hip):
    """Autograd returns the raw ABI results; a non-contiguous g and a strided points view are accepted; what no input needs is
    not launched and not allocated; no_grad saves nothing and a graph saves the points and the weight alone; bf16 and f16
    inputs get gradients of their own dtype."""
    from nova_pointcloud_amd import point_embed as pe

    S, N, C, E = 3, CHUNK + 3, 3, 260
    case = {k: v.cuda() for k, v in random_case(S, N, C, E, 3.0, 5).items()}
    x, W, g = case["x"], case["W"], case["g"]
    pos = case["pos"][:N].contiguous()
    delta = lambda before: {k: pe.stats[k] - before[k] for k in before}
    raw_out = abi_forward(hip, x, W, case["bias"], pos, case["cond"], case["base"])[0]
    raw = abi_backward(hip, x, W, g)
    got = embedded(case, 2)
    assert same_bits(got[0], raw_out) and same_bits(got[1], raw["gx"]) and same_bits(got[2], raw["gW"]) and same_bits(got[3], raw["gbias"])
    assert same_bits(got[4][:N], raw["gpos"]) and (got[4][N:] == 0).all() and same_bits(got[5], raw["gcs"]) and same_bits(got[6], g)
    # the reference's [1, P, E] table
    got3 = embedded(dict(case, pos=case["pos"][None]), None)
    assert got3[4].shape == (1, N + 2, E) and same_bits(got3[4][0], got[4]) and same_bits(got3[0], raw_out)
    # a non-contiguous g
    wide = torch.randn(S, N, 2 * E, generator=torch.Generator().manual_seed(9)).cuda()
    g_nc = wide[:, :, ::2]
    assert not g_nc.is_contiguous()
    raw_nc = abi_backward(hip, x, W, g_nc.contiguous())
    got = embedded(dict(case, g=g_nc), None)
    assert same_bits(got[1], raw_nc["gx"]) and same_bits(got[2], raw_nc["gW"]) and same_bits(got[4][:N], raw_nc["gpos"])
    # a strided view of wider rows as the points
    rows = torch.randn(S, N, 2 * C, generator=torch.Generator().manual_seed(8)).cuda().requires_grad_(True)
    out = pe.point_embed(rows[:, :, :C], W)
    out.backward(g)
    view = rows.detach()[:, :, :C].contiguous()
    assert same_bits(out.detach(), abi_forward(hip, view, W)[0])
    assert same_bits(rows.grad[:, :, :C].contiguous(), abi_backward(hip, view, W, g, want=("gx",))["gx"]) and (rows.grad[:, :, C:] == 0).all()
    # stats: only base needs a gradient: no backward kernel at all, and its gradient is g
    bl = case["base"].clone().requires_grad_(True)
    before = dict(pe.stats)
    pe.point_embed(x, W, case["bias"], base=bl, max_clouds_per_launch=2).backward(g)
    assert delta(before) == {"forward_launches": 2, "backward_launches": 0, "pos_grad_launches": 0, "cloud_sum_launches": 0}
    assert same_bits(bl.grad, g)
    # the weight and the bias: one read of g per launch, two cloud sums, no second read of g
    Wl, bias_l = W.clone().requires_grad_(True), case["bias"].clone().requires_grad_(True)
    before = dict(pe.stats)
    pe.point_embed(x, Wl, bias_l, pos=pos, max_clouds_per_launch=2).backward(g)
    assert delta(before) == {"forward_launches": 2, "backward_launches": 2, "pos_grad_launches": 0, "cloud_sum_launches": 2}
    assert same_bits(Wl.grad, raw["gW"]) and same_bits(bias_l.grad, raw["gbias"])
    # pos alone: the second read of g is the only one
    pl = case["pos"].clone().requires_grad_(True)
    before = dict(pe.stats)
    pe.point_embed(x, W, pos=pl, max_clouds_per_launch=1).backward(g)
    assert delta(before) == {"forward_launches": 3, "backward_launches": 0, "pos_grad_launches": 3, "cloud_sum_launches": 0}
    assert same_bits(pl.grad[:N], raw["gpos"])
    # cond alone: no cloud sum; only the points: neither; gx is not allocated unless the points need it
    cl = case["cond"].clone().requires_grad_(True)
    before = dict(pe.stats)
    pe.point_embed(x, W, cond=cl).backward(g)
    assert delta(before) == {"forward_launches": 1, "backward_launches": 1, "pos_grad_launches": 0, "cloud_sum_launches": 0}
    assert same_bits(cl.grad, raw["gcs"])
    big = torch.randn(1, 65536, 8, generator=torch.Generator().manual_seed(3)).cuda()
    W1 = torch.randn(1, 8, generator=torch.Generator().manual_seed(4)).cuda().requires_grad_(True)
    out = pe.point_embed(big, W1)
    gb = torch.ones_like(out)
    torch.cuda.synchronize()
    before, allocated = dict(pe.stats), torch.cuda.memory_allocated()
    torch.cuda.reset_peak_memory_stats()
    out.backward(gb)
    torch.cuda.synchronize()
    assert delta(before) == {"forward_launches": 0, "backward_launches": 1, "pos_grad_launches": 0, "cloud_sum_launches": 1}
    assert torch.cuda.max_memory_allocated() - allocated < big.numel() * 4 // 2  # gx alone would be 2 MiB
    # what autograd keeps: nothing without a graph, the points and the weight alone with one
    kept = []
    with torch.autograd.graph.saved_tensors_hooks(lambda t: kept.append(tuple(t.shape)) or t, lambda t: t):
        with torch.no_grad():
            pe.point_embed(x.clone().requires_grad_(True), W, case["bias"], pos, case["cond"], case["base"])
        assert kept == []
        pe.point_embed(x, W, case["bias"], pos, case["cond"], case["base"])  # nothing requires a gradient
        assert kept == []
        pe.point_embed(x.clone().requires_grad_(True), W, case["bias"], pos, case["cond"], case["base"].clone().requires_grad_(True))
    assert sorted(kept) == sorted([(S, N, C), (E, C)]), kept
    # mixed dtypes
    for dtype in (torch.bfloat16, torch.float16):
        low = {k: case[k].to(dtype).requires_grad_(True) for k in ("x", "W") + ADDENDS}
        out = pe.point_embed(low["x"], low["W"], **{k: low[k] for k in ADDENDS})
        assert out.dtype == torch.float32
        out.backward(g)
        assert all(low[k].grad.dtype == dtype for k in low)
        f32 = {k: v.detach().float() for k, v in low.items()}
        raw16 = abi_backward(hip, f32["x"], f32["W"], g)
        assert same_bits(out.detach(), abi_forward(hip, f32["x"], f32["W"], f32["bias"], f32["pos"][:N].contiguous(), f32["cond"], f32["base"])[0])
        for k, name in (("x", "gx"), ("W", "gW"), ("bias", "gbias"), ("cond", "gcs")):
            assert torch.equal(low[k].grad, raw16[name].to(dtype)), (dtype, k)
        assert torch.equal(low["pos"].grad[:N], raw16["gpos"].to(dtype)) and torch.equal(low["base"].grad, g.to(dtype))
    with pytest.raises(hip.NovaHipError, match="runs on the GPU"):
        pe.point_embed(x.cpu(), W.cpu())


@pytest.mark.gpu
def test_an_empty_cloud_set(hip):
    """S = 0 launches nothing: the output and the per-cloud gradients (points, cond, base) are empty, and the sums over the
    clouds (weight, bias, pos) are +0 in every element, not what the allocator handed out. The allocator's free blocks of
    those sizes are filled with NaN first, so a gradient that nothing wrote would show."""
    from nova_pointcloud_amd import point_embed as pe

    N, C, E, P = 5, 3, 12, 7
    gen = torch.Generator().manual_seed(11)
    leaf = lambda *shape: torch.randn(*shape, generator=gen).cuda().requires_grad_(True)
    x, W, bias, pos, cond, base = leaf(0, N, C), leaf(E, C), leaf(E), leaf(1, P, E), leaf(0, E), leaf(0, N, E)
    zero_bits = lambda t, shape: t.shape == shape and t.dtype == torch.float32 and (t.view(torch.int32) == 0).all()
    for per in (None, 1):
        for t in (x, W, bias, pos, cond, base):
            t.grad = None
        dirty = [nan(*shape) for shape in ((E, C), (E,), (N, E), (P, E), (1, P, E)) for _ in range(4)]
        torch.cuda.synchronize()
        del dirty
        before = dict(pe.stats)
        out = pe.point_embed(x, W, bias, pos=pos, cond=cond, base=base, max_clouds_per_launch=per)
        assert out.shape == (0, N, E) and out.dtype == torch.float32
        out.backward(torch.empty(0, N, E, device="cuda"))
        assert zero_bits(W.grad, (E, C)) and zero_bits(bias.grad, (E,)) and zero_bits(pos.grad, (1, P, E))
        assert x.grad.shape == (0, N, C) and cond.grad.shape == (0, E) and base.grad.shape == (0, N, E)
        assert pe.stats == before  # no kernel has anything to do
    # the weight alone, and under no_grad
    W.grad = None
    pe.point_embed(x.detach(), W).sum().backward()
    assert zero_bits(W.grad, (E, C))
    with torch.no_grad():
        assert pe.point_embed(x, W, bias).shape == (0, N, E)


@pytest.mark.gpu
def test_module_on_the_gpu(hip):
    """The parameters' gradients are the functional's, bitwise; load_state_dict round-trips; the output is inside the forward
    bound."""
    from nova_pointcloud_amd import point_embed as pe

    for C, E, P in ((3, 768, 1024), (6, 130, CHUNK + 9)):
        S, N = 2, CHUNK + 1
        case = {k: v.cuda() for k, v in random_case(S, N, C, E, 1.0, E, rows=P).items()}
        m = pe.PointEmbedding(C, E, P).cuda()
        m.load_state_dict({"point_embed.weight": case["W"], "point_embed.bias": case["bias"], "pos_embed": case["pos"][None]})
        xl, cl, bl = (case[k].clone().requires_grad_(True) for k in ("x", "cond", "base"))
        out = m(xl, cl, bl)
        out.backward(case["g"])
        want = embedded(case, None)
        assert same_bits(out.detach(), want[0]) and same_bits(xl.grad, want[1]) and same_bits(cl.grad, want[5]) and same_bits(bl.grad, want[6])
        assert same_bits(m.point_embed.weight.grad, want[2]) and same_bits(m.point_embed.bias.grad, want[3])
        assert m.pos_embed.grad.shape == (1, P, E) and same_bits(m.pos_embed.grad[0], want[4])
        plain = m(case["x"])
        assert same_bits(plain, abi_forward(hip, case["x"], case["W"], case["bias"], case["pos"][:N].contiguous())[0])
        fresh = pe.PointEmbedding(C, E, P)
        fresh.load_state_dict(m.state_dict())
        assert sorted(fresh.state_dict()) == ["point_embed.bias", "point_embed.weight", "pos_embed"]
        assert same_bits(fresh.cuda()(case["x"], case["cond"], case["base"]), out.detach())
        cpu = {k: v.cpu() for k, v in case.items()}
        r = restate(**cpu)
        check("module out", out.detach().cpu(), r["out"], bounds(r, S, N, C, E)["out"], f"module E={E}")


if __name__ == "__main__" and sys.argv[1:] == ["--abi-checks"]:
    abi_checks()
