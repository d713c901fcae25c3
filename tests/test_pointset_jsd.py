"""The JSD point-set metric (PointFlow's jsd_between_point_cloud_sets on a 28^3 occupancy grid in the ball of radius 0.5):
a float64 restatement of the grid assignment and its properties (CPU), a float32 emulation of the kernel's bounded
slow-path search against the full scan (CPU), jensen_shannon_divergence and normalize_clouds (CPU), the input and C ABI
checks (CPU), and the occupancy kernel (csrc/occupancy.hip) against the restatement (GPU).

The definition restated here (include/nova_hip.h, nova_pointset_occupancy_grid): lattice nodes c(i, j, k) =
(2 (i, j, k) - (R-1)) / (2 (R-1)), flat index (i R + j) R + k; in_sphere keeps the nodes with
(2i-(R-1))^2 + (2j-(R-1))^2 + (2k-(R-1))^2 <= (R-1)^2; a point goes to its nearest grid node, lowest index on ties.
PointFlow's code is restated from the published algorithm, not executed: parity unpinned by execution.

GPU comparisons of per-point nodes leave a point out only when its float64 best and second-best squared distances differ
by less than tau = 5e-7 (d + d^2), d the distance to the second-best node: the float32 node coordinate carries at most
6e-8, so a float32 squared distance carries at most 2 sqrt(3) d 6e-8 + 4 u d^2 (u = 6e-8) and a comparison of two twice
that. At most 0.1 % of the points of a case may be left out (measured with the restatement alone: 0.002 % - 0.022 %)."""
import ctypes
import inspect
import json
import math
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TAU = 5e-7
MAX_LEFT_OUT = 1e-3


# --------------------------------------------------------------------------------------------- restatement
def int_mask(R, in_sphere=True):
    t2 = (2 * np.arange(R, dtype=np.int64) - (R - 1)) ** 2
    m = (t2[:, None, None] + t2[None, :, None] + t2[None, None, :]) <= (R - 1) ** 2
    return m.reshape(-1) if in_sphere else np.ones(R ** 3, dtype=bool)


def float32_pointflow_mask(R):
    """PointFlow's unit_cube_grid_point_cloud membership: float32 grid i * spacing - 0.5, float32 norm <= 0.5."""
    spacing = np.float32(1.0 / float(R - 1))
    c = (np.arange(R, dtype=np.float32) * spacing - np.float32(0.5)).astype(np.float32)
    g = np.stack(np.meshgrid(c, c, c, indexing="ij"), -1).reshape(-1, 3).astype(np.float32)
    return np.linalg.norm(g, axis=1) <= 0.5


def grid_nodes64(R, in_sphere, device="cpu"):
    """(coordinates float64 [G, 3], flat indices int64 [G]) of the grid nodes, in flat order."""
    flat = torch.from_numpy(np.flatnonzero(int_mask(R, in_sphere)))
    ijk = torch.stack([flat // (R * R), (flat // R) % R, flat % R], 1)
    return ((2 * ijk - (R - 1)).double() / (2.0 * (R - 1))).to(device), flat.to(device)


def restated_nodes(x, R=28, in_sphere=True, chunk=4096):
    """Full scan in float64 on x's device: (nearest grid node's flat index [P], leave-out flag [P]) for points x [P, 3]."""
    nodes, flat = grid_nodes64(R, in_sphere, x.device)
    best, near_tie = [], []
    for c in x.double().split(chunk):
        d2 = ((c[:, None, :] - nodes[None]) ** 2).sum(-1)
        v, _ = d2.topk(min(2, d2.shape[1]), dim=1, largest=False)
        idx = torch.arange(d2.shape[1], device=x.device)
        first = torch.where(d2 == v[:, :1], idx, d2.shape[1]).min(dim=1).values  # lowest index at the minimum
        best.append(flat[first])
        d = v[:, -1].sqrt()
        near_tie.append((v[:, -1] - v[:, 0]) < TAU * (d + d * d) if d2.shape[1] > 1 else torch.zeros_like(d, dtype=torch.bool))
    return torch.cat(best), torch.cat(near_tie)


def rounded_nodes32(x, R):
    """The header's float32 rounded node: per axis clamp(rintf((p + 0.5f) * (float)(R-1)), 0, R-1) -> (i, j, k) int64 [P, 3]."""
    x = x.float()
    v = (x + torch.tensor(0.5, dtype=torch.float32, device=x.device)) * torch.tensor(float(R - 1), dtype=torch.float32, device=x.device)
    return torch.round(v).clamp(0, R - 1).long()  # torch.round is round-half-even, as rintf


def rounded_is_member(ijk, R, in_sphere=True):
    if not in_sphere:
        return torch.ones(ijk.shape[0], dtype=torch.bool, device=ijk.device)
    return ((2 * ijk - (R - 1)) ** 2).sum(1) <= (R - 1) ** 2


def ball(S, n, seed, radius, shell=False):
    g = torch.Generator().manual_seed(seed)
    p = torch.randn(S, n, 3, generator=g, dtype=torch.float64)
    r = torch.rand(S, n, 1, generator=g, dtype=torch.float64) ** (1 / 3)
    if shell:
        r = 0.9 + 0.1 * r
    return (p / p.norm(dim=-1, keepdim=True) * r * radius).float()


def restated_histograms(x, R=28, in_sphere=True):
    """(counters, bernoulli) int64 [R^3] of clouds x [S, N, 3] by the restatement."""
    S, N = x.shape[:2]
    nodes, _ = restated_nodes(x.reshape(-1, 3), R, in_sphere)
    nodes = nodes.view(S, N)
    counters = torch.bincount(nodes.reshape(-1), minlength=R ** 3)
    bern = torch.zeros(R ** 3, dtype=torch.int64, device=x.device)
    for s in range(S):
        bern[torch.unique(nodes[s])] += 1
    return counters, bern


def jsd_numpy(P, Q):
    from scipy.stats import entropy

    P, Q = np.asarray(P, dtype=np.float64), np.asarray(Q, dtype=np.float64)
    P_, Q_ = P / P.sum(), Q / Q.sum()
    return entropy((P_ + Q_) / 2, base=2) - (entropy(P_, base=2) + entropy(Q_, base=2)) / 2


def kernel_search_emulated(p, R):
    """The slow-path search of csrc/occupancy.hip for one point p (float32 [3]) whose rounded node is outside the ball, in
    NumPy float32: n0 from the point pulled to radius 0.5 - 0.87 h, the window of columns within D0, one clamped
    candidate per column, minimum of (float32 squared distance, flat index). Returns (flat index, columns visited)."""
    f = np.float32
    rm1 = R - 1
    coord = (2 * np.arange(R) - rm1).astype(f) / f(2 * rm1)
    t2 = (2 * np.arange(R) - rm1) ** 2
    rnd = lambda v: int(min(max(np.rint((f(v) + f(0.5)) * f(rm1)), 0), rm1))
    member = lambda i, j, k: t2[i] + t2[j] + t2[k] <= rm1 * rm1
    inside = (t2[:, None, None] + t2[None, :, None] + t2[None, None, :]) <= rm1 * rm1
    klo = np.where(inside.any(2), inside.argmax(2), -1)  # first k of column (i, j) inside the ball; the last is R - 1 - klo
    sq = lambda c: f(f(p[0] - c[0]) ** 2 + f(p[1] - c[1]) ** 2 + f(p[2] - c[2]) ** 2)
    rin, r = f(0.5) - f(0.87) / f(rm1), np.sqrt(f(p[0] * p[0] + p[1] * p[1] + p[2] * p[2]))
    sc = rin / r if r > rin else f(1)
    n0 = tuple(rnd(p[a] * sc) for a in range(3))
    if not member(*n0):
        n0 = (R // 2,) * 3
    d0 = sq(coord[list(n0)])
    best = (d0, (n0[0] * R + n0[1]) * R + n0[2])
    D0 = np.sqrt(d0) * f(1 + 1e-5) + f(1e-6)
    lo = lambda v: int(min(max(np.floor((v - D0 + f(0.5)) * f(rm1)), 0), rm1))
    hi = lambda v: int(min(max(np.ceil((v + D0 + f(0.5)) * f(rm1)), 0), rm1))
    kr, cols = rnd(p[2]), 0
    for i in range(lo(p[0]), hi(p[0]) + 1):
        for j in range(lo(p[1]), hi(p[1]) + 1):
            cols += 1
            if klo[i, j] < 0:
                continue
            k = min(max(kr, klo[i, j]), rm1 - klo[i, j])
            best = min(best, (sq(coord[[i, j, k]]), (i * R + j) * R + k))
    return best[1], cols


# --------------------------------------------------------------------------------------------- CPU: the definition
def test_integer_mask_equals_float32_mask_for_even_resolutions():
    for R in range(2, 35, 2):
        assert np.array_equal(int_mask(R), float32_pointflow_mask(R)), R
        t2 = (2 * np.arange(R) - (R - 1)) ** 2
        s = (t2[:, None, None] + t2[None, :, None] + t2[None, None, :])
        assert np.abs(s - (R - 1) ** 2).min() >= 2  # no node on the sphere
    assert int(int_mask(28).sum()) == 10144
    assert int(int_mask(2).sum()) == 0
    from nova_pointcloud_amd import metrics

    for R in (3, 8, 27, 28, 32):
        assert np.array_equal(metrics.grid_node_mask(R).numpy(), int_mask(R))
    assert bool(metrics.grid_node_mask(5, in_sphere=False).all())


@pytest.mark.parametrize("R,radius", [(28, 0.5), (28, 0.9), (8, 0.9), (27, 0.7)])
def test_rounded_node_shortcut_agrees_with_the_full_scan(R, radius):
    x = ball(4, 2048, 10 + R, radius).reshape(-1, 3)
    best, near_tie = restated_nodes(x, R)
    ijk = rounded_nodes32(x, R)
    inside = rounded_is_member(ijk, R) & ~near_tie
    flat = (ijk[:, 0] * R + ijk[:, 1]) * R + ijk[:, 2]
    assert int(inside.sum()) > 1000
    assert torch.equal(flat[inside], best[inside])


@pytest.mark.parametrize("R,radius,shell", [(28, 0.6, False), (28, 2.0, True), (8, 0.9, False), (27, 0.9, False), (32, 5.0, True), (3, 1.0, False)])
def test_bounded_search_of_the_kernel_agrees_with_the_full_scan(R, radius, shell):
    """The column + window search (emulated in float32) finds the node of the float64 full scan for points whose rounded
    node is outside the ball, and visits a small window for points just outside."""
    x = ball(1, 4096, 20 + R, radius, shell).reshape(-1, 3)
    slow = ~rounded_is_member(rounded_nodes32(x, R), R)
    x = x[slow][:150]
    assert x.shape[0] >= 100
    best, near_tie = restated_nodes(x, R)
    cols = []
    for p, want, skip in zip(x.numpy(), best.tolist(), near_tie.tolist()):
        got, c = kernel_search_emulated(p, R)
        cols.append(c)
        assert int_mask(R)[got]
        assert skip or got == want, (p, got, want)
    assert int(near_tie.sum()) <= 3
    assert max(cols) <= R * R
    if (R, radius) == (28, 0.6):
        assert np.mean(cols) < 80  # about 5 x 5 to 8 x 8 columns instead of 784


def test_restatement_properties():
    R = 8
    nodes, flat = grid_nodes64(R, True)
    best, near_tie = restated_nodes(nodes, R)  # a point exactly on a node gets that node
    assert torch.equal(best, flat) and not bool(near_tie.any())
    x = ball(5, 300, 3, 0.7)
    counters, bern = restated_histograms(x, R)
    assert int(counters.sum()) == 5 * 300
    assert bool((bern <= 5).all()) and bool((bern <= counters).all())
    assert bool((counters[~torch.from_numpy(int_mask(R))] == 0).all())


# --------------------------------------------------------------------------------------------- CPU: JSD, normalisation
def test_jensen_shannon_divergence():
    from nova_pointcloud_amd.metrics import jensen_shannon_divergence as jsd

    rng = np.random.default_rng(0)
    for n in (2, 17, 10144):
        P, Q = rng.integers(0, 50, n), rng.integers(0, 50, n)
        P[0], Q[-1] = 1, 1
        got = jsd(torch.from_numpy(P), torch.from_numpy(Q))
        assert got.dtype == torch.float64 and got.dim() == 0
        assert abs(float(got) - jsd_numpy(P, Q)) < 1e-12
        assert float(jsd(torch.from_numpy(Q), torch.from_numpy(P))) == pytest.approx(float(got), abs=1e-15)  # symmetric
        assert float(jsd(torch.from_numpy(P), torch.from_numpy(P))) == 0.0
        assert abs(float(jsd(torch.from_numpy(3 * P), torch.from_numpy(P)))) < 1e-12
    assert float(jsd(torch.tensor([1, 2, 0, 0]), torch.tensor([0, 0, 5, 1]))) == pytest.approx(1.0, abs=1e-12)  # disjoint supports
    with pytest.raises(ValueError, match="negative"):
        jsd(torch.tensor([1.0, -1.0]), torch.tensor([1.0, 1.0]))
    with pytest.raises(ValueError, match="unequal"):
        jsd(torch.ones(3), torch.ones(4))
    with pytest.raises(ValueError, match="all-zero"):
        jsd(torch.zeros(3), torch.ones(3))


def test_normalize_clouds():
    from nova_pointcloud_amd.metrics import normalize_clouds

    g = torch.Generator().manual_seed(4)
    x = (torch.randn(3, 200, 3, generator=g, dtype=torch.float64) * torch.tensor([1.0, 2.5, 0.3], dtype=torch.float64) + 4.0)
    s = normalize_clouds(x, "unit_sphere")
    norms = s.norm(dim=-1)
    assert bool((norms <= 0.5 + 1e-12).all()) and torch.allclose(norms.max(dim=1).values, torch.full((3,), 0.5, dtype=torch.float64), atol=1e-12)
    c = normalize_clouds(x, "unit_cube")
    assert bool((c.abs() <= 0.5 + 1e-12).all())
    assert torch.allclose(c.amax(dim=(1, 2)), torch.full((3,), 0.5, dtype=torch.float64), atol=1e-12)
    assert torch.allclose(c.amin(dim=(1, 2)), torch.full((3,), -0.5, dtype=torch.float64), atol=1e-12)
    for mode, ref in (("unit_sphere", s), ("unit_cube", c)):
        moved = normalize_clouds(x * 7.0 + torch.tensor([3.0, -2.0, 11.0], dtype=torch.float64), mode)
        assert torch.allclose(moved, ref, atol=1e-12)  # translation and scale invariance
        flat = normalize_clouds(torch.full((2, 5, 3), 1.25), mode)  # degenerate clouds
        assert torch.equal(flat, torch.zeros(2, 5, 3))
        assert normalize_clouds(x[0].float(), mode).shape == (200, 3)  # a single cloud
    assert normalize_clouds(x, "none") is x
    with pytest.raises(ValueError, match="mode"):
        normalize_clouds(x, "unit_ball")


# --------------------------------------------------------------------------------------------- CPU: checks
def test_occupancy_grid_input_checks():
    from nova_pointcloud_amd import hip, metrics

    with pytest.raises(hip.NovaHipError, match="GPU"):
        metrics.occupancy_grid(torch.zeros(2, 8, 3))
    with pytest.raises(ValueError, match=r"\[S, n, 3\]"):
        metrics.occupancy_grid(torch.zeros(2, 8, 2))
    with pytest.raises(ValueError, match="finite"):
        metrics.occupancy_grid(torch.full((1, 4, 3), float("nan")))
    for bad in (1, 33, 0, -4, 28.0):
        with pytest.raises(ValueError, match="resolution"):
            metrics.occupancy_grid(torch.zeros(2, 8, 3), resolution=bad)
    with pytest.raises(ValueError, match="resolution 2"):
        metrics.occupancy_grid(torch.zeros(2, 8, 3), resolution=2)
    with pytest.raises(ValueError, match="resolution"):
        metrics.compute_all_metrics(torch.zeros(2, 8, 3), torch.zeros(2, 8, 3), jsd=True, jsd_resolution=99)
    assert metrics.OCC_MAX_RESOLUTION == int(
        __import__("re").search(r"#define NOVA_OCC_MAX_RES (\d+)", open(os.path.join(ROOT, "include", "nova_hip.h")).read()).group(1))
    assert metrics.OCC_MAX_RESOLUTION >= 32


def test_occupancy_grid_abi_checks():
    """Argument checks of nova_pointset_occupancy_grid run before any device work (no GPU needed)."""
    from nova_pointcloud_amd import hip

    lib = hip.load(check_device=False)
    fn = lib.nova_pointset_occupancy_grid
    x, cnt, ber = ctypes.c_void_p(4096), ctypes.c_void_p(8192), ctypes.c_void_p(12288)  # never dereferenced: rejected first
    assert fn(x, cnt, ber, None, None, 2, 0, 28, 1, 0, None) == -2            # N = 0
    assert b"empty" in lib.nova_last_error()
    assert fn(x, cnt, ber, None, None, 2, -5, 28, 1, 0, None) == -2
    assert fn(x, cnt, ber, None, None, 2, 1 << 24, 28, 1, 0, None) == -2      # more points than a histogram word counts
    assert fn(x, cnt, ber, None, None, 2, 8, 1, 1, 0, None) == -1             # R below 2
    assert b"resolution" in lib.nova_last_error()
    assert fn(x, cnt, ber, None, None, 2, 8, 33, 0, 0, None) == -1            # R above NOVA_OCC_MAX_RES
    assert b"32" in lib.nova_last_error()
    assert fn(x, cnt, ber, None, None, 2, 8, 2, 1, 0, None) == -1             # no node inside the ball
    assert b"no node" in lib.nova_last_error()
    assert fn(x, cnt, ber, None, None, 2, 8, 28, 1, -1, None) == -1
    assert fn(None, cnt, ber, None, None, 2, 8, 28, 1, 0, None) == -1
    assert b"null" in lib.nova_last_error()
    assert fn(x, None, ber, None, None, 2, 8, 28, 1, 0, None) == -1
    assert b"null" in lib.nova_last_error()
    assert fn(None, None, None, None, None, 0, 8, 28, 1, 0, None) == 0        # S = 0: nothing to do
    assert fn(None, None, None, None, None, 0, 0, 28, 1, 0, None) == -2       # but the shape is still checked


def test_signatures_and_cli_flags():
    from nova_pointcloud_amd import metrics

    sig = inspect.signature(metrics.compute_all_metrics).parameters
    assert sig["jsd"].default is False and sig["jsd_resolution"].default == 28
    assert list(sig)[:4] == ["sample_pcs", "ref_pcs", "batch_size", "emd"]
    assert list(inspect.signature(metrics.jsd_between_point_cloud_sets).parameters) == ["sample_pcs", "ref_pcs", "resolution"]
    assert list(inspect.signature(metrics.entropy_of_occupancy_grid).parameters) == ["pclouds", "grid_resolution", "in_sphere"]
    assert list(inspect.signature(metrics.occupancy_grid).parameters)[:4] == ["pclouds", "resolution", "in_sphere", "return_nodes"]
    out = subprocess.run([sys.executable, os.path.join(ROOT, "scripts", "eval_pointsets.py"), "--help"], check=True,
                         capture_output=True, text=True).stdout
    for flag in ("--jsd", "--jsd-resolution", "--normalize", "unit_sphere", "unit_cube", "--emd"):
        assert flag in out


# --------------------------------------------------------------------------------------------- GPU
def nodes_case(x, R, in_sphere):
    """Kernel nodes of clouds x [S, N, 3] (cuda) against the restatement; returns (result dict, left-out count)."""
    from nova_pointcloud_amd.metrics import occupancy_grid

    S, N = x.shape[:2]
    got = occupancy_grid(x, R, in_sphere, return_nodes=True)
    assert got["nodes"].shape == (S, N) and got["nodes"].dtype == torch.int32
    want, near_tie = restated_nodes(x.reshape(-1, 3), R, in_sphere, chunk=8192)
    nodes = got["nodes"].reshape(-1).long()
    left_out = int(near_tie.sum())
    wrong = int(((nodes != want) & ~near_tie).sum())
    print(f"R {R} in_sphere {in_sphere} points {S * N}: left out {left_out} ({100.0 * left_out / (S * N):.4f} %), "
          f"differing among the left out {int(((nodes != want) & near_tie).sum())}, wrong {wrong}, outside {got['outside']}")
    assert left_out <= MAX_LEFT_OUT * S * N
    assert wrong == 0
    assert bool(torch.from_numpy(int_mask(R, in_sphere)).to(x.device)[nodes].all())  # every node is a grid node
    # the kernel against its own node output: exact
    assert torch.equal(got["counters"], torch.bincount(nodes, minlength=R ** 3))
    bern = torch.zeros(R ** 3, dtype=torch.int64, device=x.device)
    for s in range(S):
        bern[torch.unique(got["nodes"][s].long())] += 1
    assert torch.equal(got["bernoulli"], bern)
    assert got["outside"] == int((~rounded_is_member(rounded_nodes32(x.reshape(-1, 3), R), R, in_sphere)).sum())
    return got, left_out


@pytest.mark.gpu
@pytest.mark.parametrize("name,R,in_sphere", [("ball_0.5", 28, True), ("ball_0.9", 28, True), ("shell_2", 28, True),
                                              ("cube", 28, False), ("ball_0.9", 8, True), ("ball_0.9", 27, True),
                                              ("ball_0.9", 32, True), ("cube", 32, False), ("ball_0.9", 3, True)])
def test_nodes_match_the_restatement(hip, name, R, in_sphere):
    S, N = 64, 2048
    if name == "cube":
        x = torch.rand(S, N, 3, generator=torch.Generator().manual_seed(5)) * 1.4 - 0.7
    else:
        x = ball(S, N, R, {"ball_0.5": 0.5, "ball_0.9": 0.9, "shell_2": 2.0}[name], shell=name == "shell_2")
    got, _ = nodes_case(x.cuda(), R, in_sphere)
    assert int(got["counters"].sum()) == S * N
    if name == "shell_2":
        assert got["outside"] == S * N
    if name == "cube":
        assert got["outside"] == 0


@pytest.mark.gpu
@pytest.mark.parametrize("S,N", [(1, 1), (3, 257), (2, 64), (300, 33)])
def test_nodes_ragged_sizes(hip, S, N):
    nodes_case(ball(S, N, 40 + N, 0.8).cuda(), 28, True)


@pytest.mark.gpu
def test_points_on_nodes_and_far_away(hip):
    from nova_pointcloud_amd.metrics import occupancy_grid

    R = 28
    nodes, flat = grid_nodes64(R, True)
    on = nodes[::5].float().cuda()[None]  # coordinates k / 54: the float32 value is the kernel's node coordinate
    got = occupancy_grid(on, R, True, return_nodes=True)
    assert torch.equal(got["nodes"][0].long().cpu(), flat[::5]) and got["outside"] == 0
    far = torch.tensor([[[1e6, 0.0, 0.0], [0.0, -3e4, 0.0], [0.0, 0.0, 77.0], [-9.0, 0.0, 0.0]]]).cuda()
    got = occupancy_grid(far, R, True, return_nodes=True)
    want, near_tie = restated_nodes(far[0], R)
    assert got["outside"] == 4 and torch.equal(got["nodes"][0].long()[~near_tie], want[~near_tie])
    assert occupancy_grid(torch.zeros(0, 5, 3).cuda())["counters"].sum() == 0


@pytest.mark.gpu
def test_bitwise_reproducible_under_every_split(hip, monkeypatch):
    from nova_pointcloud_amd import metrics

    x = ball(40, 1000, 50, 0.8).cuda()
    keys = ("counters", "bernoulli", "outside")
    one = metrics.occupancy_grid(x, return_nodes=True)
    same = lambda a, b: all(torch.equal(a[k], b[k]) if torch.is_tensor(a[k]) else a[k] == b[k] for k in a)
    assert same(one, metrics.occupancy_grid(x, return_nodes=True))
    for wg in (1, 3, 40, 1000):
        assert same(one, metrics.occupancy_grid(x, return_nodes=True, workgroups=wg)), wg
    for per in (1, 7, 39):
        assert same(one, metrics.occupancy_grid(x, return_nodes=True, max_clouds_per_launch=per)), per
    # 1-cloud and 7-cloud launches accumulated into the same counters through the C ABI
    cnt, ber = torch.zeros(28 ** 3, dtype=torch.int64, device="cuda"), torch.zeros(28 ** 3, dtype=torch.int64, device="cuda")
    out = torch.zeros(1, dtype=torch.int64, device="cuda")
    s0 = 0
    while s0 < 40:
        n = 1 if (s0 // 4) % 2 == 0 else min(7, 40 - s0)
        hip.call("nova_pointset_occupancy_grid", x[s0].data_ptr(), cnt.data_ptr(), ber.data_ptr(), None, out.data_ptr(), n, 1000, 28,
                 1, 0, hip.stream_ptr())
        s0 += n
    assert torch.equal(cnt, one["counters"]) and torch.equal(ber, one["bernoulli"]) and int(out) == one["outside"]
    # a set larger than the host cap
    monkeypatch.setattr(metrics, "_OCC_POINTS_PER_LAUNCH", 4500)
    capped = metrics.occupancy_grid(x, return_nodes=True)
    assert same(one, capped) and all(k in capped for k in keys)
    # more clouds than one workgroup's cloud field holds
    many = ball(600, 16, 51, 0.8).cuda()
    a, b = metrics.occupancy_grid(many, workgroups=1), metrics.occupancy_grid(many, workgroups=600)
    assert same(a, b) and int(a["bernoulli"].max()) <= 600 and int(a["counters"].sum()) == 600 * 16


def entropy_change_bound(moved_fraction, cells):
    """Fannes-Audenaert: two distributions on `cells` outcomes at total-variation distance T differ in base-2 entropy by at
    most T log2(cells - 1) + h2(T)."""
    T = moved_fraction
    if T == 0:
        return 0.0
    return T * math.log2(cells - 1) + (-T * math.log2(T) - (1 - T) * math.log2(1 - T))


@pytest.mark.gpu
@pytest.mark.parametrize("case", ["different", "same"])
def test_jsd_end_to_end(hip, case):
    from nova_pointcloud_amd import metrics

    a = ball(64, 2048, 1, 0.5).cuda()
    b = (ball(64, 2048, 2, 0.5) * torch.tensor([1.0, 0.8, 0.6])).cuda() if case == "different" else ball(64, 2048, 3, 0.5).cuda()
    got = metrics.jsd_between_point_cloud_sets(a, b)
    (Pa, _), (Pb, _) = restated_histograms(a), restated_histograms(b)
    want = jsd_numpy(Pa.cpu().numpy(), Pb.cpu().numpy())
    # Only near-tie points (tau) may sit in a neighbouring cell. With T_a, T_b their shares, P' and Q' move by at most
    # T_a, T_b in total variation and their mean by (T_a + T_b) / 2, so by Fannes-Audenaert on the three entropies
    # |JSD - JSD'| <= F((T_a + T_b) / 2) + (F(T_a) + F(T_b)) / 2, F(T) = T log2(cells - 1) + h2(T), cells = 10144.
    Ta = float(restated_nodes(a.reshape(-1, 3))[1].double().mean())
    Tb = float(restated_nodes(b.reshape(-1, 3))[1].double().mean())
    assert max(Ta, Tb) <= MAX_LEFT_OUT
    bound = entropy_change_bound((Ta + Tb) / 2, 10144) + (entropy_change_bound(Ta, 10144) + entropy_change_bound(Tb, 10144)) / 2
    print(f"{case}: jsd {got:.6f}, restatement {want:.6f}, |difference| {abs(got - want):.3e}, bound {bound:.3e} (T {Ta:.2e}, {Tb:.2e})")
    assert abs(got - want) <= bound + 1e-12
    assert (0.25 < got < 0.40) if case == "different" else (0.01 < got < 0.05)  # 0.311 and 0.029 by the restatement on the CPU
    assert metrics.jsd_between_point_cloud_sets(a, a) == 0.0
    # entropy of the occupancy grid against the restatement's bernoulli (exact when no point is left out)
    ent, counters = metrics.entropy_of_occupancy_grid(a)
    p = restated_histograms(a)[1].double().cpu().numpy() / 64
    p = p[p > 0]
    q = np.where(p < 1, 1 - p, 1.0)
    want_ent = float(-(p * np.log(p) + (1 - p) * np.log(q)).sum() / 10144)
    # a left-out point moves the bernoulli count of at most two nodes by one, and H([p, 1 - p]) moves by at most
    # H([1/64, 63/64]) for a step of 1/64
    step = -(1 / 64) * math.log(1 / 64) - (63 / 64) * math.log(63 / 64)
    assert abs(ent - want_ent) <= 2 * Ta * 64 * 2048 * step / 10144 + 1e-12 and int(counters.sum()) == 64 * 2048
    if case == "different":
        small_a, small_b = a[:12, :256].contiguous(), b[:10, :256].contiguous()
        plain = metrics.compute_all_metrics(small_a, small_b)
        with_jsd = metrics.compute_all_metrics(small_a, small_b, jsd=True)
        assert tuple(plain) == metrics.METRIC_KEYS
        assert tuple(with_jsd) == metrics.METRIC_KEYS + ("jsd", "jsd_outside_fraction")
        assert {k: with_jsd[k] for k in plain} == plain  # bit for bit
        assert with_jsd["jsd"] == metrics.jsd_between_point_cloud_sets(small_a, small_b)
        occ = [metrics.occupancy_grid(s)["outside"] / (s.shape[0] * 256) for s in (small_a, small_b)]
        assert with_jsd["jsd_outside_fraction"] == max(occ) and 0 < max(occ) < 0.1


@pytest.mark.gpu
def test_eval_pointsets_script_jsd_and_normalize(hip, tmp_path, capsys):
    sys.path.insert(0, os.path.join(ROOT, "scripts"))
    import eval_pointsets

    from nova_pointcloud_amd import metrics

    smp = ball(6, 300, 60, 3.0) * torch.tensor([1.0, 0.7, 0.5]) + 2.0
    ref = ball(5, 300, 61, 2.0) - 1.0
    metrics.save_point_clouds(smp, "smp", str(tmp_path / "smp"))
    metrics.save_point_clouds(ref, "ref", str(tmp_path / "ref"))
    args = [str(tmp_path / "smp"), str(tmp_path / "ref")]
    res = eval_pointsets.main(args + ["--jsd", "--normalize", "unit_sphere", "--out", str(tmp_path / "o.json")])
    out = capsys.readouterr()
    assert len(out.out.strip().splitlines()) == 1 and json.loads(out.out) == res and json.loads((tmp_path / "o.json").read_text()) == res
    assert "warning" not in out.err
    ns, nr = metrics.normalize_clouds(smp.cuda(), "unit_sphere"), metrics.normalize_clouds(ref.cuda(), "unit_sphere")
    direct = metrics.compute_all_metrics(ns, nr, jsd=True)
    assert {k: res[k] for k in direct} == direct and res["normalize"] == "unit_sphere"
    assert res["jsd"] == metrics.jsd_between_point_cloud_sets(ns, nr)
    # without the flags the line is what it was; without normalisation these clouds are far outside the ball: one warning
    plain = eval_pointsets.main(args)
    capsys.readouterr()
    assert "jsd" not in plain and "normalize" not in plain
    raw = eval_pointsets.main(args + ["--jsd", "--jsd-resolution", "16"])
    out = capsys.readouterr()
    assert raw["jsd_outside_fraction"] > 0.05 and out.err.count("warning") == 1 and "--normalize" in out.err
    assert len(out.out.strip().splitlines()) == 1
    assert raw["jsd"] == metrics.jsd_between_point_cloud_sets(smp.cuda(), ref.cuda(), 16)
