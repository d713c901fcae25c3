"""Soft cluster pooling (csrc/soft_cluster.hip, nova_pointcloud_amd/clustering.py): the soft clustering step of the reference's
point-cloud models (transformer_pointcloud_nova.py:465-487, :724-741) as one HIP forward and one HIP backward.

restate() is the definition of include/nova_hip.h (nova_pointset_soft_cluster, nova_pointset_soft_cluster_bwd) in float64,
values and closed-form gradients. The CPU tests hold it against torch autograd of the reference's literal form (cdist,
softmax, the loop over the clusters, + 1e-8); the GPU tests hold the kernels against it.

BOUNDS of the random GPU cases, written before the first GPU run, by count from float64 quantities. u = 2^-24. Per cloud:
    X   = max |x|,  Dm = max(|x|, |c|),  D = max_ik d_ik,  kappa = scale ln 2 = 1 / temperature,  theta = kappa D
    C   = 16 theta + K + 8     relative error of one a_ik in units of u: d_ik and m carry 3 u each (differences, the squares,
                               the square root), so the exponent (m - d) scale ln 2 is off by at most 8 theta u; e_k carries that
                               plus 2 u (v_exp_f32), L the same plus K u, r and the product a = e r one u each
    mass_k        (N + C) u mass_k                                 any-order sum of N terms, each off by C u
    out_kj        B_out = 2 (N + C + 2) u X                        numerator (|x| <= X) and denominator by the line above, 2 u
    delta_h       = U (3 G B_out + 24 u G Dm) + (N + C + 4) u Hd + u H
                               the error of one h_ik computed from the KERNEL's out and mass: U = max u_k, G = max |g|,
                               Hd = max |u_k dot_ik|, H = max |h_ik| over the pairs with a_ik > 0
    one term f_ik e_j (the quotient |e_j| / d_ik <= 1 cancels the distance):
                  kappa a (1 - a) (2 delta_h + 2 C u H) + kappa a (K + 2) u H + (C + 12) u |f e|
                               h_k - hbar = sum_l a_l (h_k - h_l): the errors of h and of a enter with the factor (1 - a_k),
                               the K roundings of the hbar chain with a_k alone
    gc_kj         kappa [(2 delta_h + 2 C u H) sum_i a (1 - a) + (K + 2) u H mass_k] + (N + C + 12) u sum_i |f_ik e_j|
    gx_ij         U G (N + 2 C + 2 K + 4) u + kappa [2 delta_h + 2 C u H + (K + 2) u H] + (C + 2 K + 12) u sum_k |f_ik e_j|
    shared sum    sum_s bound(gc[s]) + S u sum_s |gc[s]|
plus 1e-30 (1 + X) everywhere for weights flushed below 2^-126. The torch float32 form on the CPU sits at under one u against
several hundred u in these bounds, so the reference alone is well inside them.
Measured on an MI355X: see the docstring of test_random_clouds and DESIGN.md.
"""
import ctypes
import functools
import math
import os
import re

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
U = 2.0 ** -24
EPS32 = float(np.float32(1e-8))  # the definition's 1e-8f
CHUNK = 1024  # == NOVA_SOFT_CLUSTER_CHUNK (test_header_constants_and_kernel_shape)
N_CASES = [1, 63, 64, 65, 255, 256, 257, CHUNK - 1, CHUNK, CHUNK + 1, 2 * CHUNK + 1]
K_CASES = [1, 2, 7, 8, 9, 16, 31, 32]
LOG2E = math.log2(math.e)


def scale_of(temperature):
    """log2(e) / temperature, exact in float64 (the kernel's float32 value comes from metrics._interp_scale)."""
    return 0.0 if temperature == math.inf else LOG2E / temperature


def restate(x, c, scale, g=None, gm=None, eps=EPS32):
    """The definition in float64. x [S, N, 3], c [K, 3] or [S, K, 3]. Returns a dict: out, mass, and with g (and optionally
    gm) given gx, gc [S, K, 3] per cloud, gcs [K, 3] their sum over the clouds, and the intermediates the bounds need."""
    x, c = x.double(), c.double()
    S, N = x.shape[:2]
    cc = c if c.dim() == 3 else c.expand(S, *c.shape)
    e = x[:, :, None, :] - cc[:, None, :, :]  # [S, N, K, 3]
    d = e.square().sum(-1).sqrt()
    w = torch.exp2((d.min(-1, keepdim=True).values - d) * scale)
    a = w / w.sum(-1, keepdim=True)
    mass = a.sum(1)
    out = torch.einsum("snk,snj->skj", a, x) / (mass + eps)[..., None]
    res = {"out": out, "mass": mass, "a": a, "d": d, "e": e}
    if g is None:
        return res
    g = g.double()
    gm = torch.zeros_like(mass) if gm is None else gm.double()
    u = 1.0 / (mass + eps)
    ud = u[:, None, :] * torch.einsum("skj,snkj->snk", g, x[:, :, None, :] - out[:, None, :, :])
    h = ud + gm[:, None, :]
    hbar = (a * h).sum(-1, keepdim=True)
    kappa = scale * math.log(2.0)
    f = torch.where(d == 0, torch.zeros_like(d), -kappa * a * (h - hbar) / torch.where(d == 0, torch.ones_like(d), d))
    fe = f[..., None] * e
    res.update(gx=torch.einsum("snk,skj->snj", a * u[:, None, :], g) + fe.sum(2), gc=-fe.sum(1), u=u, ud=ud, h=h, fe=fe, kappa=kappa)
    res["gcs"] = res["gc"].sum(0)
    return res


def literal_form(points, centers, temperature):
    """transformer_pointcloud_nova.py:470-480 as written, the temperature added and the MLP left out. cdist is told not to
    take its matrix-product form, which it would pick by size and which is not the distance of the definition."""
    d = torch.cdist(points, centers, compute_mode="donot_use_mm_for_euclid_dist")
    w = torch.softmax(-d / temperature, dim=-1)
    pooled, masses = [], []
    for k in range(centers.shape[-2]):
        wk = w[:, :, k:k + 1]
        pooled.append((points * wk).sum(dim=1) / (wk.sum(dim=1) + 1e-8))
        masses.append(wk.sum(dim=1)[:, 0])
    return torch.stack(pooled, dim=1), torch.stack(masses, dim=1)


def bounds(r, x, c, g, K):
    """The docstring's bounds from restate()'s float64 quantities: (mass [S, K], out [S, 1, 1], gx [S, N, 3], gc [S, K, 3],
    gcs [K, 3])."""
    S, N = x.shape[:2]
    amax = lambda t: t.abs().reshape(S, -1).max(1).values
    X = amax(x.double())
    Dm = torch.maximum(X, c.double().abs().max() if c.dim() == 2 else amax(c.double()))
    a, d, kappa = r["a"], r["d"], r["kappa"]
    C = 16 * kappa * amax(d) + K + 8
    tiny = 1e-30 * (1 + X)
    b_mass = (N + C)[:, None] * U * r["mass"] + tiny[:, None]
    b_out = 2 * (N + C + 2) * U * X + tiny
    G = amax(g.double())
    H = amax(torch.where(a > 0, r["h"], torch.zeros_like(a)))
    Hd = amax(torch.where(a > 0, r["ud"], torch.zeros_like(a)))
    Umax = amax(r["u"])
    delta_h = Umax * (3 * G * b_out + 24 * U * G * Dm) + (N + C + 4) * U * Hd + U * H
    common = (2 * delta_h + 2 * C * U * H)[:, None, None]
    afe = r["fe"].abs()
    b_gc = kappa * (common * (a * (1 - a)).sum(1)[..., None] + ((K + 2) * U * H)[:, None, None] * r["mass"][..., None]) \
        + (N + C + 12)[:, None, None] * U * afe.sum(1) + tiny[:, None, None]
    b_gx = (Umax * G * (N + 2 * C + 2 * K + 4) * U)[:, None, None] + kappa * (common + ((K + 2) * U * H)[:, None, None]) \
        + (C + 2 * K + 12)[:, None, None] * U * afe.sum(2) + tiny[:, None, None]
    b_gcs = b_gc.sum(0) + S * U * r["gc"].abs().sum(0)
    return b_mass, b_out[:, None, None], b_gx, b_gc, b_gcs


def random_case(S, N, K, shared, seed):
    gen = torch.Generator().manual_seed(seed)
    x = torch.randn(S, N, 3, generator=gen) * 0.5
    c = torch.randn(*(() if shared else (S,)), K, 3, generator=gen) * 0.5
    g = torch.randn(S, K, 3, generator=gen)
    gm = torch.randn(S, K, generator=gen)
    return x, c, g, gm


# ---- CPU -------------------------------------------------------------------------------------------------------------------


@pytest.mark.parametrize("temperature", [1.0, 0.25, 3.0])
@pytest.mark.parametrize("shared", [True, False])
def test_restatement_against_float64_autograd_of_the_reference_form(temperature, shared):
    """Values and closed-form gradients against autograd of the literal loop, four shapes, with a point ON a centre (the
    subgradient convention: torch.cdist's backward gives 0 there, and so does f)."""
    for S, N, K in ((1, 1, 1), (2, 5, 3), (3, 40, 8), (2, 33, 32)):
        x, c, g, gm = (t.double() for t in random_case(S, N, K, shared, 100 * N + K))
        x[0, 0] = c[1 % K] if shared else c[0, 1 % K]  # coincident
        xl, cl = x.clone().requires_grad_(True), c.clone().requires_grad_(True)
        out, mass = literal_form(xl, cl, temperature)
        ((out * g).sum() + (mass * gm).sum()).backward()
        r = restate(x, c, scale_of(temperature), g, gm, eps=1e-8)
        assert (r["d"] == 0).sum() >= 1
        for got, want in ((r["out"], out), (r["mass"], mass), (r["gx"], xl.grad), (r["gcs"] if shared else r["gc"], cl.grad)):
            assert torch.isfinite(got).all()
            assert (got - want.detach()).abs().max() <= 1e-12 * (1 + want.abs().max()), (S, N, K)


def test_restatement_on_hand_cases():
    # N = 1: a point on centre 0, centre 1 at distance ln 2 (temperature 1): a = (2/3, 1/3), mass = a, out = x a / (a + eps)
    x = torch.tensor([[[1.0, 2.0, 3.0]]], dtype=torch.float64)
    c = torch.tensor([[1.0, 2.0, 3.0], [1.0 + math.log(2.0), 2.0, 3.0]], dtype=torch.float64)
    r = restate(x, c, LOG2E, torch.ones(1, 2, 3), torch.ones(1, 2))
    assert torch.allclose(r["mass"], torch.tensor([[2 / 3, 1 / 3]], dtype=torch.float64), rtol=1e-14)
    assert torch.allclose(r["out"], x * (r["mass"] / (r["mass"] + EPS32))[..., None], rtol=1e-14)
    assert r["fe"][0, 0, 0].abs().max() == 0  # the coincident pair carries no gradient through its distance
    # K = 1: a = 1 whatever the temperature: the plain mean, mass = N, and nothing reaches the centre
    x, c, g, gm = random_case(2, 9, 1, False, 3)
    for t in (1.0, 0.01, math.inf):
        r = restate(x, c, scale_of(t), g, gm)
        assert torch.allclose(r["out"], x.double().mean(1, keepdim=True), rtol=1e-8) and (r["mass"] == 9).all()
        assert (r["gc"] == 0).all() and torch.allclose(r["gx"], (g.double() / (9 + EPS32)).expand(2, 9, 3), rtol=1e-14)
    # an empty cluster: at temperature 2^-20 every weight of the far centre underflows: out = +0, mass = 0, finite gradients
    x = torch.tensor([[[0.0, 0.0, 0.0], [1.0, 0.0, 0.0]]], dtype=torch.float64)
    c = torch.tensor([[0.0, 1.0, 0.0], [9.0, 9.0, 9.0]], dtype=torch.float64)
    r = restate(x, c, scale_of(2.0 ** -20), torch.ones(1, 2, 3), torch.ones(1, 2))
    assert (r["mass"][0] == torch.tensor([2.0, 0.0], dtype=torch.float64)).all()
    assert (r["out"][0, 1] == 0).all() and not torch.signbit(r["out"][0, 1]).any()
    assert all(torch.isfinite(r[k]).all() for k in ("gx", "gc", "h", "u"))


def test_python_argument_errors_in_the_stated_order():
    from nova_pointcloud_amd import clustering, hip

    pool = clustering.soft_cluster_pool
    x, c = torch.zeros(2, 5, 3), torch.zeros(4, 3)
    bad = [
        (dict(points=[1.0], centers=None), "points: expected a tensor"),  # types before anything else, points first
        (dict(points=x, centers=None), "centers: expected a tensor"),
        (dict(points=x.long(), centers=c.long().reshape(2, 6)), "points: expected a floating dtype"),  # dtypes before shapes
        (dict(points=x, centers=c.int()), "centers: expected a floating dtype"),
        (dict(points=torch.zeros(2, 5, 4), centers=torch.zeros(4, 2)), r"points: expected \[S, N, 3\]"),
        (dict(points=torch.zeros(5, 3), centers=c), r"points: expected \[S, N, 3\]"),
        (dict(points=x, centers=torch.zeros(3)), r"centers: expected shared \[K, 3\] or per-cloud \[S, K, 3\]"),
        (dict(points=x, centers=torch.zeros(4, 2)), r"centers: expected shared"),
        (dict(points=torch.zeros(2, 0, 3), centers=torch.zeros(3, 4, 3)), "same number of clouds"),  # counts before ranges
        (dict(points=torch.zeros(2, 0, 3), centers=torch.zeros(0, 3)), "1 .. 65536 points"),  # N before K
        (dict(points=torch.zeros(1, clustering.SOFT_CLUSTER_MAX_POINTS + 1, 3), centers=c), "1 .. 65536 points"),
        (dict(points=x, centers=torch.zeros(0, 3)), "1 .. 32 centres"),
        (dict(points=x, centers=torch.zeros(2, 33, 3), temperature=0.0), "1 .. 32 centres"),  # ranges before the temperature
        (dict(points=x, centers=c, temperature=0.0, max_clouds_per_launch=0), "temperature must be"),
        (dict(points=x, centers=c, temperature=-1.0), "temperature must be"),
        (dict(points=x, centers=c, temperature=True), "temperature must be"),
        (dict(points=x, centers=c, temperature=1e-40), "too small"),
        (dict(points=x, centers=c, max_clouds_per_launch=0), "max_clouds_per_launch must be an integer >= 1"),
        (dict(points=x, centers=c, max_clouds_per_launch=1.5), "max_clouds_per_launch must be an integer >= 1"),
    ]
    for kwargs, message in bad:
        with pytest.raises(ValueError, match=message):
            pool(**kwargs)
    if torch.cuda.is_available():  # devices come after the ranges and before the temperature
        with pytest.raises(ValueError, match="same device"):
            pool(x.cuda(), c, temperature=0.0)
    for kwargs in (dict(points=x, centers=c), dict(points=x, centers=torch.zeros(2, 4, 3), return_mass=True)):
        with pytest.raises(hip.NovaHipError, match="runs on the GPU"):  # everything else passed: CPU tensors are refused last
            pool(**kwargs)


def test_abi_rejections_in_the_stated_order():
    """Every error of the three entries, in the order include/nova_hip.h states, before any device work (no GPU needed)."""
    from nova_pointcloud_amd import clustering, hip

    lib = hip.load(check_device=False)
    MB = 1 << 28  # pointers far apart: never dereferenced, rejected first
    x, c, out, mass, ws, g, gm, gx, gc = (ctypes.c_void_p(MB * i) for i in range(1, 10))
    fwd = lambda S, N, K, scale=1.0, shared=1, x=x, c=c, out=out, mass=mass, ws=ws: lib.nova_pointset_soft_cluster(
        x, c, out, mass, ws, S, N, K, shared, scale, None)
    bwd = lambda S, N, K, scale=1.0, shared=1, x=x, c=c, out=out, mass=mass, g=g, gm=gm, gx=gx, gc=gc, ws=ws: lib.nova_pointset_soft_cluster_bwd(
        x, c, out, mass, g, gm, gx, gc, ws, S, N, K, shared, scale, None)
    err = lib.nova_last_error
    big = clustering.SOFT_CLUSTER_MAX_POINTS + 1
    for fn in (fwd, bwd):
        for N in (0, -1, big):
            assert fn(70000, N, 0, -1.0) == -2 and b"NOVA_SOFT_CLUSTER_MAX_POINTS" in err()  # N first
        for K in (0, 33):
            assert fn(70000, 8, K, -1.0) == -2 and b"NOVA_SOFT_CLUSTER_MAX_K" in err()  # K before the cloud count
            assert fn(0, 8, K) == -2  # also without clouds
        assert fn(65536, 8, 8, -1.0) == -2 and b"65535" in err()  # shape errors before argument errors
        for scale in (-1.0, math.nan, math.inf):
            assert fn(2, 8, 8, scale, x=None) == -1 and b"scale" in err()  # before null pointers
            assert fn(0, 8, 8, scale) == -1  # also without clouds
        assert fn(0, 8, 8) == 0 and fn(-3, 8, 32, 0.0) == 0
        assert fn(0, 8, 8, x=None, c=None, out=None, mass=None, ws=None) == 0  # S <= 0 returns before the pointers are looked at
    for name in ("x", "c", "out", "mass", "ws"):
        assert fwd(2, 8, 8, **{name: None}) == -1 and b"null" in err(), name
    for name in ("x", "c", "out", "mass", "g"):
        assert bwd(2, 8, 8, **{name: None}) == -1 and b"null" in err(), name
    # (no call here passes every check: what passes them launches, and these pointers are not memory)
    assert bwd(2, 8, 8, gx=None, gc=None) == -1 and b"both NULL" in err()
    assert bwd(2, 8, 8, gx=None, gc=None, g=None) == -1 and b"null" in err()  # the null check comes first
    assert bwd(2, 8, 8, ws=None) == -1 and b"workspace" in err()
    assert bwd(2, 8, 8, ws=None, gx=None, gc=None) == -1 and b"both NULL" in err()  # in that order
    # outputs must not overlap inputs or each other: checked last
    assert fwd(2, 8, 8, out=x) == -1 and b"overlaps" in err()
    assert fwd(2, 8, 8, out=ctypes.c_void_p(MB + 2 * 8 * 12 - 4)) == -1 and b"overlaps" in err()  # the last float of x
    assert fwd(2, 8, 8, mass=c) == -1 and fwd(2, 8, 8, ws=x) == -1 and b"overlaps" in err()
    assert fwd(2, 8, 8, mass=out) == -1 and fwd(2, 8, 8, ws=out) == -1 and b"overlap each other" in err()
    assert fwd(2, 8, 8, shared=0, out=ctypes.c_void_p(2 * MB + 2 * 8 * 12 - 4)) == -1 and b"overlaps" in err()  # the last float of per-cloud c ..
    assert fwd(70000, 8, 8, out=x) == -2  # .. and a shape error still comes first
    for name in ("x", "c", "out", "mass", "g", "gm"):
        assert bwd(2, 8, 8, gx={"x": x, "c": c, "out": out, "mass": mass, "g": g, "gm": gm}[name]) == -1 and b"overlaps an input" in err(), name
    assert bwd(2, 8, 8, gc=g) == -1 and bwd(2, 8, 8, ws=mass) == -1 and b"overlaps an input" in err()
    assert bwd(2, 8, 8, gc=gx) == -1 and bwd(2, 8, 8, ws=gx) == -1 and b"overlap each other" in err()
    assert bwd(2, 8, 8, gc=gx, ws=None) == -1 and b"workspace" in err()  # before the overlap check
    # the cloud sum
    s = lambda S, K, gc=gc, gcs=gx: lib.nova_pointset_soft_cluster_sum_clouds(gc, gcs, S, K, None)
    assert s(2, 0, gc=None) == -2 and s(2, 33) == -2 and b"NOVA_SOFT_CLUSTER_MAX_K" in err()
    assert s(0, 8, gc=None, gcs=None) == 0 and s(-1, 8) == 0
    assert s(2, 8, gc=None) == -1 and s(2, 8, gcs=None) == -1 and b"null" in err()
    assert s(2, 8, gcs=gc) == -1 and s(2, 8, gcs=ctypes.c_void_p(9 * MB + 2 * 8 * 12 - 4)) == -1 and b"overlaps" in err()
    assert lib.nova_version() == hip.ABI_VERSION  # no version bump


def test_header_constants_and_kernel_shape():
    from nova_pointcloud_amd import clustering, hip

    header = open(os.path.join(ROOT, "include", "nova_hip.h")).read()
    const = lambda name: int(re.search(r"#define " + name + r" (\d+)", header).group(1))
    assert const("NOVA_SOFT_CLUSTER_MAX_POINTS") == clustering.SOFT_CLUSTER_MAX_POINTS == 65536
    assert const("NOVA_SOFT_CLUSTER_MAX_K") == clustering.SOFT_CLUSTER_MAX_K == 32
    assert const("NOVA_SOFT_CLUSTER_CHUNK") == clustering.SOFT_CLUSTER_CHUNK == CHUNK
    for needle in ("nova_pointset_soft_cluster", "nova_pointset_soft_cluster_bwd", "nova_pointset_soft_cluster_sum_clouds", ":465-487",
                   ":724-741", "1e-8f", "ascending chunk order", "ascending s"):
        assert needle in header, needle
    for name in ("nova_pointset_soft_cluster", "nova_pointset_soft_cluster_bwd", "nova_pointset_soft_cluster_sum_clouds"):
        assert name in hip.SIGNATURES
    source = open(os.path.join(ROOT, "nova_pointcloud_amd", "csrc", "soft_cluster.hip")).read()
    assert "SC_CHUNK = NOVA_SOFT_CLUSTER_CHUNK;" in source and "SC_MAX_K = NOVA_SOFT_CLUSTER_MAX_K;" in source
    assert "SC_MAX_N = NOVA_SOFT_CLUSTER_MAX_POINTS;" in source
    assert int(re.search(r"SC_T = (\d+);", source).group(1)) == 256  # the header's 256 threads, 4 points each per chunk
    assert "SC_STEPS = SC_CHUNK / SC_T;" in source
    assert float(re.search(r"SC_EPS = ([0-9e.-]+)f;", source).group(1)) == 1e-8
    assert "atomic" not in source.lower().replace("no atomics", "")
    makefile = open(os.path.join(ROOT, "nova_pointcloud_amd", "csrc", "Makefile")).read()
    assert "soft_cluster.hip" in re.search(r"^SRCS := (.*)$", makefile, flags=re.M).group(1).split()


# ---- GPU -------------------------------------------------------------------------------------------------------------------


def abi(hip, x, c, temperature, g=None, gm=None, want_x=True, want_c=True, per=None):
    """The three entries called directly on float32 tensors, outputs pre-filled with NaN: (out, mass, gx, gc per cloud, gcs)."""
    from nova_pointcloud_amd import metrics

    scale = metrics._interp_scale(temperature)
    S, N = x.shape[:2]
    K, shared = c.shape[-2], c.dim() == 2
    chunks = (N + CHUNK - 1) // CHUNK
    nan = lambda *shape: torch.full(shape, math.nan, dtype=torch.float32, device=x.device)
    out, mass, ws = nan(S, K, 3), nan(S, K), nan(S * chunks * K * 4)
    per = S if per is None else per
    stream = hip.stream_ptr()
    at = lambda t, s0: t[s0].data_ptr() if t is not None else None
    cp = lambda s0: c.data_ptr() if shared else c[s0].data_ptr()
    for s0 in range(0, S, per):
        n = min(per, S - s0)
        hip.call("nova_pointset_soft_cluster", x[s0].data_ptr(), cp(s0), out[s0].data_ptr(), mass[s0].data_ptr(), ws.data_ptr(), n, N, K,
                 1 if shared else 0, scale, stream)
    if g is None:
        return out, mass
    gx = nan(S, N, 3) if want_x else None
    gc = nan(S, K, 3) if want_c else None
    for s0 in range(0, S, per):
        n = min(per, S - s0)
        hip.call("nova_pointset_soft_cluster_bwd", x[s0].data_ptr(), cp(s0), out[s0].data_ptr(), mass[s0].data_ptr(), g[s0].data_ptr(),
                 at(gm, s0), at(gx, s0), at(gc, s0), ws.data_ptr(), n, N, K, 1 if shared else 0, scale, stream)
    gcs = None
    if want_c:
        gcs = nan(K, 3)
        hip.call("nova_pointset_soft_cluster_sum_clouds", gc.data_ptr(), gcs.data_ptr(), S, K, stream)
    return out, mass, gx, gc, gcs


def f32_quotient(num, mass):
    """num / (mass + 1e-8f) in float32 on the CPU: one rounded addition, one IEEE division. The sums start at +0, so a zero
    numerator is +0 (a sum of -0 terms alone would be -0 here)."""
    den = mass.numpy().astype(np.float32) + np.float32(1e-8)
    return torch.from_numpy((num.numpy() + 0.0).astype(np.float32) / den[..., None])


def same_bits(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


@pytest.mark.gpu
@pytest.mark.parametrize("N", N_CASES)
def test_exact_uniform_weights(hip, N):
    """temperature = +inf, K a power of two, small integer coordinates: every a_ik = 1 / K exactly and all sums are exact, so
    mass = N / K and out is the one correctly rounded quotient, in any order of summation: a point dropped or doubled at
    any boundary shows. S cycles 1 .. 5, the centre form alternates."""
    for n, K in enumerate((1, 2, 8, 16, 32)):
        S, shared = (N + n) % 5 + 1, n % 2 == 0
        gen = torch.Generator().manual_seed(N * 37 + K)
        x = torch.randint(-8, 9, (S, N, 3), generator=gen).float()
        x[:, :, 0] += 9  # positive: every point moves the sum
        c = torch.randint(-8, 9, (*(() if shared else (S,)), K, 3), generator=gen).float()
        out, mass = abi(hip, x.cuda(), c.cuda(), math.inf)
        assert same_bits(mass.cpu(), torch.full((S, K), N / K, dtype=torch.float32)), (N, K)
        want = f32_quotient((x.double().sum(1) / K)[:, None, :].expand(S, K, 3), torch.full((S, K), N / K))
        assert same_bits(out.cpu(), want), (N, K)


def lattice_case(S, N, K, shared, seed):
    """Centres on an integer lattice spaced 4 apart, integer points within 1 per axis of a centre other than the last (for
    K > 1): each has one nearest centre, by a gap above 1. Returns x, c and the assignment [S, N]."""
    gen = torch.Generator().manual_seed(seed)
    k = torch.arange(K)
    c = torch.stack([4.0 * (k % 4), 4.0 * ((k // 4) % 4), 4.0 * (k // 16)], dim=-1)
    owner = torch.randint(0, max(1, K - 1), (S, N), generator=gen)
    x = c[owner] + torch.randint(-1, 2, (S, N, 3), generator=gen).float()
    return x, (c if shared else c.expand(S, K, 3).contiguous()), owner


@pytest.mark.gpu
@pytest.mark.parametrize("N", N_CASES)
def test_exact_hard_assignment(hip, N):
    """temperature = 2^-20: every a_ik is exactly 0 or 1, so mass is the counts, out the correctly rounded centroid and the
    cluster no point visits gives +0 (not -0, not NaN)."""
    for n, K in enumerate(K_CASES):
        S, shared = (N + n) % 5 + 1, n % 2 == 1
        x, c, owner = lattice_case(S, N, K, shared, N * 41 + K)
        out, mass = abi(hip, x.cuda(), c.cuda(), 2.0 ** -20)
        onehot = torch.nn.functional.one_hot(owner, K).double()
        counts = onehot.sum(1)
        assert same_bits(mass.cpu(), counts.float()), (N, K)
        want = f32_quotient(torch.einsum("snk,snj->skj", onehot, x.double()), counts)
        assert same_bits(out.cpu(), want), (N, K)
        if K > 1:
            assert same_bits(out.cpu()[:, K - 1], torch.zeros(S, 3)), (N, K)  # +0 bit for bit


@pytest.mark.gpu
@pytest.mark.parametrize("N", [64, 256, 1024, 2048])
def test_exact_backward_uniform_weights(hip, N):
    """temperature = +inf, N >= K powers of two, integer g and gm: u_k = K / N and a_ik = 1 / K are powers of two and kappa = 0,
    so gx[s, i, j] = (sum_k g[s, k, j]) / N exactly for every point and gc == 0 exactly (gm reaches nothing)."""
    for n, K in enumerate((1, 2, 8, 16, 32)):
        S, shared = (N // 64 + n) % 5 + 1, n % 2 == 0
        gen = torch.Generator().manual_seed(N + K)
        x = torch.randint(-8, 9, (S, N, 3), generator=gen).float()
        c = torch.randint(-8, 9, (*(() if shared else (S,)), K, 3), generator=gen).float()
        g = torch.randint(-5, 6, (S, K, 3), generator=gen).float()
        gm = torch.randint(-5, 6, (S, K), generator=gen).float()
        _, _, gx, gc, gcs = abi(hip, x.cuda(), c.cuda(), math.inf, g.cuda(), gm.cuda())
        assert same_bits(gx.cpu(), (g.sum(1, keepdim=True) / N).expand(S, N, 3).contiguous()), (N, K)
        assert (gc.cpu() == 0).all() and (gcs.cpu() == 0).all(), (N, K)


WORST = {}


def check(name, got, want, bound, where):
    """Every entry within its bound; the worst error / bound of the quantity is kept for the report."""
    assert torch.isfinite(got).all(), (name, where)
    ratio = ((got.double() - want).abs() / bound.expand_as(want)).max().item()
    WORST[name] = max(WORST.get(name, 0.0), ratio)
    print(f"soft_cluster {where} {name}: worst error / bound {ratio:.4g}")
    assert ratio <= 1.0, (name, where, ratio)


@pytest.mark.gpu
@pytest.mark.parametrize("N", N_CASES)
def test_random_clouds(hip, N):
    """Gaussian points and centres, every K of K_CASES, S cycling 1 .. 5, both centre forms, temperatures 1, 1/4 and +inf:
    every entry of out, mass, gx, gc and the shared-centre sum against restate() (float64 on the kernel's float32 scale)
    within bounds() of the module docstring; nothing is left out of the comparison. The worst error / bound per quantity is
    printed. Measured on an MI355X, worst over all cases: mass 0.094, out 0.023, gx 0.024, gc 0.0027, the shared-centre sum 0.0013
    (soft cluster pooling)."""
    from nova_pointcloud_amd import metrics

    for n, K in enumerate(K_CASES):
        S, shared, temperature = (N + n) % 5 + 1, (N + n) % 2 == 0, (1.0, 0.25, math.inf)[(N + n) % 3]
        x, c, g, gm = random_case(S, N, K, shared, N * 43 + K)
        out, mass, gx, gc, gcs = (t.cpu() for t in abi(hip, x.cuda(), c.cuda(), temperature, g.cuda(), gm.cuda()))
        r = restate(x, c, metrics._interp_scale(temperature), g, gm)
        b_mass, b_out, b_gx, b_gc, b_gcs = bounds(r, x, c, g, K)
        where = f"N={N} K={K} S={S} {'shared' if shared else 'per-cloud'} T={temperature}"
        check("mass", mass, r["mass"], b_mass, where)
        check("out", out, r["out"], b_out, where)
        check("gx", gx, r["gx"], b_gx, where)
        check("gc", gc, r["gc"], b_gc, where)
        check("gcs", gcs, r["gcs"], b_gcs, where)


# the boundary indices of the reduction over a cloud of 2 CHUNK + 1 points: the first and last lane of a wave, the last thread of
# a step and the first of the next, the last point of a chunk and the first of the next, the lone point of the last chunk
PROBES = [0, 63, 64, 255, 256, CHUNK - 1, CHUNK, 2 * CHUNK - 1, 2 * CHUNK]


@functools.lru_cache(maxsize=None)
def probe_case():
    """One cloud of 2 CHUNK + 1 points per boundary index. Two centres at (-1, 0, 0) and (1, 0, 0), temperature 1/16. The bulk
    of the points lies within 0.02 of one of them: saturated, a (1 - a) below 1e-13, so their f is about 0. Cloud s has ONE
    probe point, at index PROBES[s], near the plane between the centres (a about 1/2 each); g is the same large vector for
    both centroids, so h_0 - h_1 is large there and the probe carries nearly all of its cloud's gc."""
    N, temperature = 2 * CHUNK + 1, 1.0 / 16
    gen = torch.Generator().manual_seed(7)
    c = torch.tensor([[-1.0, 0.0, 0.0], [1.0, 0.0, 0.0]])
    x = c[torch.arange(N) % 2] + (torch.rand(len(PROBES), N, 3, generator=gen) - 0.5) * 0.04
    for s, i in enumerate(PROBES):
        x[s, i] = torch.tensor([0.001 * (s - 4), 0.25 + 0.01 * s, -0.25 + 0.02 * s])
    g = torch.tensor([[1000.0, 0.0, 0.0], [1000.0, 0.0, 0.0]]).expand(len(PROBES), 2, 3).contiguous()
    return x, c, g, temperature


def test_probe_case_is_sensitive_at_every_boundary():
    """On the float64 form alone: removing the probe point of a cloud moves that cloud's gc by at least 64 bounds."""
    from nova_pointcloud_amd import metrics

    x, c, g, temperature = probe_case()
    scale = metrics._interp_scale(temperature)
    r = restate(x, c, scale, g)
    b_gc = bounds(r, x, c, g, 2)[3]
    for s, i in enumerate(PROBES):
        keep = torch.arange(x.shape[1]) != i
        moved = (restate(x[s:s + 1, keep], c, scale, g[s:s + 1])["gc"] - r["gc"][s:s + 1]).abs()
        assert (moved / b_gc[s:s + 1]).max() >= 64, (i, (moved / b_gc[s:s + 1]).max().item())


@pytest.mark.gpu
def test_center_gradient_at_the_reduction_boundaries(hip):
    """The kernel's gc on probe_case() within ONE bound, where a point dropped at any boundary index would move it by 64."""
    from nova_pointcloud_amd import metrics

    x, c, g, temperature = probe_case()
    r = restate(x, c, metrics._interp_scale(temperature), g)
    b_mass, b_out, b_gx, b_gc, b_gcs = bounds(r, x, c, g, 2)
    for cc in (c, c.expand(len(PROBES), 2, 3).contiguous()):
        out, mass, gx, gc, gcs = (t.cpu() for t in abi(hip, x.cuda(), cc.cuda(), temperature, g.cuda()))
        check("gc", gc, r["gc"], b_gc, "probe")
        check("gx", gx, r["gx"], b_gx, "probe")
        check("out", out, r["out"], b_out, "probe")
        check("mass", mass, r["mass"], b_mass, "probe")


def pooled(x, c, g, gm, temperature, per):
    """(out, mass, grad of points, grad of centres) through the module, under sum(out g) + sum(mass gm)."""
    from nova_pointcloud_amd import clustering

    xl, cl = x.clone().requires_grad_(True), c.clone().requires_grad_(True)
    out, mass = clustering.soft_cluster_pool(xl, cl, temperature=temperature, return_mass=True, max_clouds_per_launch=per)
    ((out * g).sum() + (mass * gm).sum()).backward()
    return out.detach(), mass.detach(), xl.grad, cl.grad


@pytest.mark.gpu
@pytest.mark.parametrize("K", [8, 9])
def test_bitwise_reproducible(hip, K):
    """Outputs and gradients bit for bit the same for max_clouds_per_launch 1, 2 and default, in two runs; per cloud for every
    cloud moved to another batch position and for a cloud run alone. The shared-centre gradient is covered over every split."""
    S, N = 5, CHUNK + 1
    for shared in (True, False):
        x, c, g, gm = (t.cuda() for t in random_case(S, N, K, shared, 11 + K))
        base = pooled(x, c, g, gm, 0.5, None)
        for per in (1, 2, None, None):
            for a, b in zip(base, pooled(x, c, g, gm, 0.5, per)):
                assert same_bits(a, b), (K, shared, per)
        perm = torch.tensor([3, 0, 4, 1, 2], device="cuda")
        moved = pooled(x[perm], c if shared else c[perm], g[perm], gm[perm], 0.5, 2)
        for q in range(3 if shared else 4):  # the shared centres' gradient is one sum over the clouds: its order moves with them
            assert same_bits(base[q][perm], moved[q]), (K, shared, q)
        for s in range(S):
            alone = pooled(x[s:s + 1], c if shared else c[s:s + 1], g[s:s + 1], gm[s:s + 1], 0.5, None)
            for q in range(3 if shared else 4):
                assert same_bits(base[q][s:s + 1], alone[q]), (K, shared, s, q)
        # and the raw per-cloud centre gradient of the shared form does not depend on the position either
        raw = abi(hip, x, c, 0.5, g, gm)[3]
        raw_moved = abi(hip, x[perm].contiguous(), c if shared else c[perm].contiguous(), 0.5, g[perm].contiguous(), gm[perm].contiguous(), per=2)[3]
        assert same_bits(raw[perm], raw_moved), (K, shared)


@pytest.mark.gpu
def test_binding(hip):
    """Autograd returns the raw ABI gradients; bf16 and f16 inputs get gradients of their own dtype; a strided x[:, :, :3]
    view works; a backward with no gradient into the centres launches no cloud sum and no centre-gradient kernel."""
    from nova_pointcloud_amd import clustering

    S, N, K = 3, 300, 8
    for shared in (True, False):
        x, c, g, gm = (t.cuda() for t in random_case(S, N, K, shared, 5))
        out, mass, gx, gc, gcs = abi(hip, x, c, 0.5, g, gm)
        got = pooled(x, c, g, gm, 0.5, 2)
        for a, b in zip(got, (out, mass, gx, gcs if shared else gc)):
            assert same_bits(a, b), shared
        # through out alone (gm NULL) and through mass alone (g zero)
        xl, cl = x.clone().requires_grad_(True), c.clone().requires_grad_(True)
        (clustering.soft_cluster_pool(xl, cl, temperature=0.5) * g).sum().backward()
        raw = abi(hip, x, c, 0.5, g, None)
        assert same_bits(xl.grad, raw[2]) and same_bits(cl.grad, raw[4] if shared else raw[3])
        xl, cl = x.clone().requires_grad_(True), c.clone().requires_grad_(True)
        (clustering.soft_cluster_pool(xl, cl, temperature=0.5, return_mass=True)[1] * gm).sum().backward()
        raw = abi(hip, x, c, 0.5, torch.zeros_like(g), gm)
        assert same_bits(xl.grad, raw[2]) and same_bits(cl.grad, raw[4] if shared else raw[3])
    x, c, g, gm = (t.cuda() for t in random_case(S, N, K, True, 6))
    for dtype in (torch.bfloat16, torch.float16):
        xl, cl = x.to(dtype).requires_grad_(True), c.to(dtype).requires_grad_(True)
        out = clustering.soft_cluster_pool(xl, cl)
        assert out.dtype == torch.float32
        (out * g).sum().backward()
        assert xl.grad.dtype == dtype and cl.grad.dtype == dtype
        raw = abi(hip, xl.detach().float(), cl.detach().float(), 1.0, g)
        assert same_bits(out.detach(), raw[0]) and torch.equal(xl.grad, raw[2].to(dtype)) and torch.equal(cl.grad, raw[4].to(dtype))
    wide = torch.randn(S, N, 6, generator=torch.Generator().manual_seed(8)).cuda().requires_grad_(True)
    out = clustering.soft_cluster_pool(wide[:, :, :3], c)
    (out * g).sum().backward()
    raw = abi(hip, wide.detach()[:, :, :3].contiguous(), c, 1.0, g)
    assert same_bits(out.detach(), raw[0]) and same_bits(wide.grad[:, :, :3].contiguous(), raw[2]) and (wide.grad[:, :, 3:] == 0).all()
    # stats: what is not needed is not launched
    xl = x.clone().requires_grad_(True)
    before = dict(clustering.stats)
    (clustering.soft_cluster_pool(xl, c, max_clouds_per_launch=2) * g).sum().backward()
    delta = {k: clustering.stats[k] - before[k] for k in before}
    assert delta == {"forward_launches": 2, "point_grad_launches": 2, "center_grad_launches": 0, "cloud_sum_launches": 0}
    cl = c.clone().requires_grad_(True)
    before = dict(clustering.stats)
    (clustering.soft_cluster_pool(x, cl, max_clouds_per_launch=2) * g).sum().backward()
    delta = {k: clustering.stats[k] - before[k] for k in before}
    assert delta == {"forward_launches": 2, "point_grad_launches": 0, "center_grad_launches": 2, "cloud_sum_launches": 1}
    assert same_bits(cl.grad, abi(hip, x, c, 1.0, g, want_x=False)[4])
    before = dict(clustering.stats)
    clustering.soft_cluster_pool(x, c)
    assert clustering.stats["forward_launches"] == before["forward_launches"] + 1 and clustering.stats["point_grad_launches"] == before["point_grad_launches"]
    with pytest.raises(hip.NovaHipError, match="runs on the GPU"):
        clustering.soft_cluster_pool(x.cpu(), c.cpu())
