"""The optimal assignment on the GPU (csrc/assign.hip, metrics.optimal_assignment) and assignment="device" of the EMD metrics.

CPU: the argument checks, and a numpy restatement of the integer scheme of include/nova_hip.h (nova_pointset_assignment)
against scipy on the very inputs the GPU tests use, so the inputs and the bound are shown to belong together before any
GPU sees them. GPU: validity, optimality against scipy, reproducibility, the round cap, the metrics' device path and one
case at the largest capacity form.

Where the bounds come from. The kernel solves, exactly, the assignment problem of the integer costs
Cq(i, j) = rint(c32(i, j) * 2^18), c32 the float32 distance it computes (costs that are multiples of n + 1 and a last
phase at epsilon = 1 leave no room for a non-optimal result). With q = 2^-18 and c the cost a checker uses:
  |Cq q - c| <= q / 2 + |c32 - c|   for every pair (i, j)
so for the kernel's permutation P and any other permutation S (scipy's optimum for c among them)
  mean c(P) <= mean Cq(P) q + q / 2 + d <= mean Cq(S) q + q / 2 + d <= mean c(S) + q + 2 d,     d = max |c32 - c|.
Against scipy on the float32 costs themselves d = 0 (the CPU test); against scipy on float64 distances of the same
float32 points, d is the rounding of the float32 expression: three subtractions, a product, two fused multiply-adds and
a correctly rounded square root perturb the distance by less than 3 ulps of the largest distance (the GPU tests' delta).
From below nothing beats scipy's optimum except by the rounding of the float64 mean itself (1e-9 is far above it)."""
import functools
import os
import time

import numpy as np
import pytest
import torch

Q = 2.0 ** -18
KINDS = ("normal", "ball", "shifted", "lattice", "same", "all_equal")
CLAMPS = {"normal": 2.0, "ball": 0.5, "shifted": 5.0, "lattice": 2.0, "same": 1.0, "all_equal": 0.75}
OPT_SIZES = (7, 65, 257)
GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "pointset_metrics.npz")


@functools.lru_cache(maxsize=None)
def clouds(kind, n, B=2):
    """(x, y) float32 numpy [B, n, 3] of one input kind; made once, never modified."""
    rng = np.random.RandomState(1000 * KINDS.index(kind) + n)
    x, y = rng.randn(B, n, 3), rng.randn(B, n, 3)
    if kind == "normal":
        x, y = np.clip(x, -5, 5), np.clip(y, -5, 5)
    elif kind == "ball":
        x, y = (v / np.linalg.norm(v, axis=-1, keepdims=True) * rng.rand(B, n, 1) ** (1 / 3) for v in (x, y))
    elif kind == "shifted":
        x, y = x + np.array([8.0, -8.0, 8.0]), y + np.array([8.0, -8.0, 8.0]) + 0.25
    elif kind == "lattice":
        x, y = rng.randint(-3, 4, (B, n, 3)), rng.randint(-3, 4, (B, n, 3))
    elif kind == "same":
        y = x
    else:
        x, y = np.broadcast_to(x[:, :1], (B, n, 3)), np.broadcast_to(y[:, :1], (B, n, 3))
    x, y = np.ascontiguousarray(x, dtype=np.float32), np.ascontiguousarray(y, dtype=np.float32)
    x.setflags(write=False)
    y.setflags(write=False)
    return x, y


def clamped(v, clamp):
    return v if clamp is None else np.clip(v, np.float32(-clamp), np.float32(clamp))


def cost64(x, y, clamp):
    """float64 distances [n, n] of one pair's float32 points (after the clamp)."""
    d = clamped(x, clamp).astype(np.float64)[:, None, :] - clamped(y, clamp).astype(np.float64)[None, :, :]
    return np.sqrt((d * d).sum(-1))


def cost32(x, y, clamp):
    """The float32 distances [n, n] as the kernels form them: exact differences, one rounded product, two fused
    multiply-adds (each emulated as a float64 sum of an exact product, rounded to float32), a rounded square root."""
    e = clamped(x, clamp)[:, None, :] - clamped(y, clamp)[None, :, :]
    e64 = e.astype(np.float64)
    d2 = (e[..., 0] * e[..., 0]).astype(np.float64)
    d2 = (e64[..., 1] * e64[..., 1] + d2).astype(np.float32).astype(np.float64)
    d2 = (e64[..., 2] * e64[..., 2] + d2).astype(np.float32)
    return np.sqrt(d2)


@functools.lru_cache(maxsize=None)
def scipy_mean(kind, n, clamp, b, single):
    """scipy's optimal mean matched distance of pair b, on the float64 distances or on the float32 ones (as float64)."""
    from scipy.optimize import linear_sum_assignment

    x, y = clouds(kind, n)
    c = cost32(x[b], y[b], clamp).astype(np.float64) if single else cost64(x[b], y[b], clamp)
    r, col = linear_sum_assignment(c)
    return float(c[r, col].mean()), float(c.max())


def delta(cmax):
    return 3.0 * float(np.spacing(np.float32(cmax)))


def auction_numpy(c32, first_eps=None):
    """The integer scheme of include/nova_hip.h restated: (col_of_row, rounds). c32 float32 [n, n]."""
    n = c32.shape[0]
    C = np.rint(c32.astype(np.float64) * 2.0 ** 18).astype(np.int64) * (n + 1)
    price = np.zeros(n, dtype=np.int64)
    eps = max(1, int(C.max()) // 4) if first_eps is None else first_eps  # "any deterministic function of the inputs"
    rounds = 0
    while True:
        owner = np.full(n, -1, dtype=np.int64)
        col_of_row = np.full(n, -1, dtype=np.int64)
        while True:
            rows = np.nonzero(col_of_row < 0)[0]
            if rows.size == 0:
                break
            a = C[rows] + price[None, :]
            js = a.argmin(axis=1)  # the first minimum: ties to the lowest j
            best = a[np.arange(rows.size), js]
            if n > 1:
                a[np.arange(rows.size), js] = np.iinfo(np.int64).max
                second = a.min(axis=1)
            else:
                second = best
            bid = price[js] + (second - best) + eps
            assert int(bid.max()) < 2 ** 49
            key = np.zeros(n, dtype=np.int64)
            np.maximum.at(key, js, bid * 8192 + (8191 - rows))  # highest bid, then the lowest row
            for j in np.nonzero(key)[0]:
                if owner[j] >= 0:
                    col_of_row[owner[j]] = -1
                owner[j] = 8191 - (key[j] & 8191)
                col_of_row[owner[j]] = j
                price[j] = key[j] >> 13
            rounds += 1
            assert rounds <= 64 * n + 1024
        if eps == 1:
            return col_of_row, rounds
        eps = max(1, eps // 8)


# ------------------------------------------------------------------------------------------------- CPU
def test_argument_errors_on_cpu_tensors():
    from nova_pointcloud_amd import hip, metrics

    x = torch.zeros(2, 8, 3)
    bad = [
        dict(x=torch.zeros(8, 3), y=torch.zeros(8, 3)),
        dict(x=torch.zeros(2, 8, 2), y=torch.zeros(2, 8, 2)),
        dict(x=x, y=torch.zeros(2, 9, 3)),
        dict(x=x, y=torch.zeros(3, 8, 3)),
        dict(x=torch.zeros(1, 0, 3), y=torch.zeros(1, 0, 3)),
        dict(x=torch.zeros(1, 4097, 3), y=torch.zeros(1, 4097, 3)),
        dict(x=torch.full((2, 8, 3), float("nan")), y=x),
        dict(x=x, y=torch.full((2, 8, 3), float("inf"))),
        dict(x=x, y=x, max_rounds=0),
        dict(x=x, y=x, max_rounds=2.5),
        dict(x=x, y=x, rounds_per_launch=0),
        dict(x=x, y=x, rounds_per_launch=True),
        dict(x=x, y=x, clamp=0.0),
        dict(x=x, y=x, clamp=float("inf")),
        dict(x=[[0.0, 0.0, 0.0]], y=x),
    ]
    for kw in bad:
        with pytest.raises(ValueError):
            metrics.optimal_assignment(**kw)
    with pytest.raises(hip.NovaHipError):
        metrics.optimal_assignment(x, x)
    with pytest.raises(hip.NovaHipError):
        metrics.optimal_assignment(x, x, clamp=5.0, max_rounds=10, rounds_per_launch=3)
    for fn in (metrics.compute_emd_distance, metrics.emd_approx, metrics.robust_emd):
        with pytest.raises(ValueError):
            fn(x, x, assignment="gpu")
        with pytest.raises(hip.NovaHipError):
            fn(x, x, assignment="device")


def test_kernel_shape_table_and_state_size():
    from nova_pointcloud_amd import hip, metrics

    assert [metrics.assignment_kernel_shape(n) for n in (1, 64, 65, 256, 257, 1024, 1025, 2048, 2049, 4096)] == [
        (64, 64), (64, 64), (256, 256), (256, 256), (256, 1024), (256, 1024), (512, 2048), (512, 2048), (1024, 4096), (1024, 4096)]
    with pytest.raises(ValueError):
        metrics.assignment_kernel_shape(4097)
    lib = hip.load(check_device=False)
    sizes = [lib.nova_pointset_assignment_state_bytes(n) for n in (0, 1, 2, 1000, 4096, 4097)]
    assert sizes[0] == 0 and sizes[-1] == 0
    for n, b in zip((1, 2, 1000, 4096), sizes[1:-1]):
        assert b % 16 == 0 and b >= 12 * n + 24  # prices and owners, row assignments, epsilon, rounds, done flag
    # the argument errors of the C entry point are decided before anything is launched
    f = lambda n, rounds, ptr: lib.nova_pointset_assignment(ptr, ptr, ptr, ptr, ptr, 1, n, 0.0, 0.0, 0, rounds, 1, ptr, None)
    assert f(0, 1, 16) == -1 and f(4097, 1, 16) == -1 and f(8, 0, 16) == -1 and f(8, 1, None) == -1
    assert b"null" in lib.nova_last_error()


@pytest.mark.parametrize("kind", KINDS)
def test_numpy_restatement_is_within_the_quantum_of_scipy(kind):
    """The integer scheme, restated in numpy, on the GPU tests' own inputs (pair 0, with and without the clamp): its
    float64 mean matched distance, taken like scipy's on the float32 costs the scheme quantises (d = 0 in the module
    docstring), lies in [scipy - 1e-12, scipy + q]."""
    for clamp in (None, CLAMPS[kind]):
        for n in OPT_SIZES:
            x, y = clouds(kind, n)
            c32 = cost32(x[0], y[0], clamp)
            col, rounds = auction_numpy(c32)
            assert sorted(col.tolist()) == list(range(n))
            mean = float(c32.astype(np.float64)[np.arange(n), col].mean())
            ref, _ = scipy_mean(kind, n, clamp, 0, True)
            print(f"{kind} clamp={clamp} n={n}: rounds {rounds}, mean - scipy = {mean - ref:.3e}")
            assert -1e-12 <= mean - ref <= Q, (kind, clamp, n, mean - ref)


def test_numpy_restatement_small_counts():
    for n in (1, 2):
        x, y = clouds("normal", n)
        c32 = cost32(x[0], y[0], None)
        col, _ = auction_numpy(c32)
        from scipy.optimize import linear_sum_assignment

        r, cc = linear_sum_assignment(c32.astype(np.float64))
        assert -1e-12 <= float(c32.astype(np.float64)[np.arange(n), col].mean() - c32.astype(np.float64)[r, cc].mean()) <= Q


# ------------------------------------------------------------------------------------------------- GPU
def run(x, y, **kw):
    from nova_pointcloud_amd import metrics

    idx, cost = metrics.optimal_assignment(torch.from_numpy(x.copy()).cuda(), torch.from_numpy(y.copy()).cuda(), **kw)
    assert idx.is_cuda and idx.dtype == torch.int64 and cost.dtype == torch.float32 and tuple(idx.shape) == x.shape[:2]
    return idx.cpu().numpy(), cost.cpu().numpy()


def check_pair(x, y, clamp, idx, cost):
    """Permutation; the float64 mean recomputed from the indices; the float32 cost against it. The kernel sums at most 4
    terms per thread in turn, 6 pairwise wave steps and at most 16 waves in turn and divides once: at most 27 roundings
    of non-negative partial sums, so |cost - mean32| <= 27 * 2^-24 * mean32 (32 below, for the second-order terms),
    whatever n is; the terms themselves are the float32 distances, each within 3 ulps of the float64 one (3 ulps of the
    bounding box's diagonal covers every term)."""
    n = x.shape[0]
    assert sorted(idx.tolist()) == list(range(n))
    xc, yc = clamped(x, clamp).astype(np.float64), clamped(y, clamp).astype(np.float64)
    mean = float(np.sqrt(((xc - yc[idx]) ** 2).sum(-1)).mean())
    both = np.concatenate([xc, yc])
    diagonal = float(np.linalg.norm(both.max(0) - both.min(0)))
    assert abs(float(cost) - mean) <= 32 * 2.0 ** -24 * mean + delta(diagonal), (float(cost), mean)
    return mean


@pytest.mark.gpu
@pytest.mark.parametrize("n", [1, 2, 63, 64, 65, 255, 256, 257, 511, 512, 513, 1000, 1023, 1024, 1025, 2047, 2048, 2049])
def test_validity_at_every_form_boundary(hip, n):
    """Every row a permutation, at n = 1 and 2, around the wave (64), the workgroup sizes (256, 512, 1024) and the capacity
    forms (64, 256, 1024, 2048; 4096 has its own test), and at an odd size; up to 513 points also optimal against scipy."""
    from scipy.optimize import linear_sum_assignment

    x, y = clouds("normal", n)
    idx, cost = run(x, y)
    for b in range(x.shape[0]):
        mean = check_pair(x[b], y[b], None, idx[b], cost[b])
        if n <= 513:
            c = cost64(x[b], y[b], None)
            r, col = linear_sum_assignment(c)
            assert -1e-9 <= mean - float(c[r, col].mean()) <= Q + 2 * delta(c.max())


@pytest.mark.gpu
@pytest.mark.parametrize("use_clamp", [False, True])
@pytest.mark.parametrize("kind", KINDS)
def test_optimal_against_scipy(hip, kind, use_clamp):
    """mean c64(kernel's permutation) - mean c64(scipy's) in [-1e-9, q + 2 delta] (derivation in the module docstring:
    the kernel's permutation is optimal for the costs quantised to q = 2^-18, each of which is within q / 2 + delta of the
    float64 distance; delta = 3 float32 ulps of the case's largest distance). Indices are not compared: ties abound."""
    clamp = CLAMPS[kind] if use_clamp else None
    for n in OPT_SIZES:
        x, y = clouds(kind, n)
        idx, cost = run(x, y, clamp=clamp)
        for b in range(x.shape[0]):
            mean = check_pair(x[b], y[b], clamp, idx[b], cost[b])
            ref, cmax = scipy_mean(kind, n, clamp, b, False)
            print(f"{kind} clamp={clamp} n={n} b={b}: mean - scipy = {mean - ref:.3e} (bound {Q + 2 * delta(cmax):.3e})")
            assert -1e-9 <= mean - ref <= Q + 2 * delta(cmax), (kind, clamp, n, b, mean - ref)
            if kind == "same":  # x == y: the identity is an optimum and the cost is exactly 0
                assert float(cost[b]) == 0.0 and np.array_equal(clamped(x[b], clamp), clamped(y[b], clamp)[idx[b]])


@pytest.mark.gpu
def test_integer_problem_is_solved_exactly(hip):
    """The header's claim itself: the kernel's cost is bit for bit pairwise_dist's float32 entry, and its permutation is an
    optimum of the integer costs rint(c32 * 2^18) (scipy on those integers, exact in float64, gives the same total)."""
    from scipy.optimize import linear_sum_assignment

    from nova_pointcloud_amd import metrics

    for kind, n, clamp in (("normal", 257, None), ("lattice", 65, 2.0), ("ball", 257, 0.5)):
        x, y = clouds(kind, n)
        idx, _ = run(x, y, clamp=clamp)
        D = metrics.pairwise_dist(torch.from_numpy(x.copy()).cuda(), torch.from_numpy(y.copy()).cuda(), clamp if clamp is not None else 1e30)
        Cq = np.rint(D.cpu().numpy().astype(np.float64) * 2.0 ** 18)
        for b in range(x.shape[0]):
            r, col = linear_sum_assignment(Cq[b])
            assert Cq[b][np.arange(n), idx[b]].sum() == Cq[b][r, col].sum()


@pytest.mark.gpu
def test_bitwise_reproducible(hip):
    """index and cost do not depend on rounds_per_launch (1, 7, default), on the batch around a pair, or on the run."""
    x, y = clouds("normal", 130, 3)
    base = run(x, y)
    for kw in (dict(rounds_per_launch=1), dict(rounds_per_launch=7), dict()):
        again = run(x, y, **kw)
        assert np.array_equal(again[0], base[0]) and np.array_equal(again[1].view(np.uint32), base[1].view(np.uint32))
    for b in range(3):
        alone = run(x[b:b + 1], y[b:b + 1], clamp=None)
        assert np.array_equal(alone[0][0], base[0][b]) and alone[1].view(np.uint32)[0] == base[1].view(np.uint32)[b]


@pytest.mark.gpu
def test_round_cap_raises_and_the_next_call_works(hip):
    from nova_pointcloud_amd import hip as H, metrics

    x, y = clouds("normal", 64)
    xs, ys = torch.from_numpy(x.copy()).cuda(), torch.from_numpy(y.copy()).cuda()
    t0 = time.perf_counter()
    with pytest.raises(H.NovaHipError, match=r"pair\(s\) \[0, 1\] not finished after max_rounds = 1"):
        metrics.optimal_assignment(xs, ys, max_rounds=1)
    assert time.perf_counter() - t0 < 5.0
    idx, cost, rounds = metrics.optimal_assignment(xs, ys, return_rounds=True)
    for b in range(2):
        check_pair(x[b], y[b], None, idx[b].cpu().numpy(), cost[b].cpu().numpy())
    assert rounds.dtype == torch.int64 and bool((rounds > 1).all()) and bool((rounds <= 64 * 64 + 1024).all())
    e = metrics.optimal_assignment(xs[:0], ys[:0])
    assert tuple(e[0].shape) == (0, 64) and tuple(e[1].shape) == (0,) and e[0].is_cuda
    with pytest.raises(H.NovaHipError, match="integer range"):
        metrics.optimal_assignment(xs * 4000.0, ys)


@pytest.mark.gpu
@pytest.mark.parametrize("n", [64, 257])
def test_metrics_device_path_agrees_with_host(hip, n):
    """assignment="device" against "host" per sample: both are means of float32 distances of near-optimal assignments, so
    they differ by at most q + 2 delta (delta: 3 float32 ulps of the largest clamped distance), plus the 1e-8 floor of
    emd_approx applied after instead of before the assignment."""
    from nova_pointcloud_amd import metrics

    x, y = clouds("normal", n, 3)
    xs, ys = torch.from_numpy(x.copy()).cuda(), torch.from_numpy(y.copy()).cuda()
    bound = lambda clamp: Q + 2 * delta(max(cost64(x[b], y[b], clamp).max() for b in range(3)))
    h, d = metrics.emd_approx(xs, ys), metrics.emd_approx(xs, ys, assignment="device")
    assert d.dtype == h.dtype and d.device == h.device and tuple(d.shape) == (3,)
    print(f"emd_approx n={n}: max |host - device| = {float((h.double() - d.double()).abs().max()):.3e} (bound {bound(2.0) + 1e-8:.3e})")
    assert float((h.double() - d.double()).abs().max()) <= bound(2.0) + 1e-8
    h, d = metrics.robust_emd(xs, ys), metrics.robust_emd(xs, ys, assignment="device")
    assert abs(float(h) - float(d)) <= bound(2.0) + 1e-8
    h, d = metrics.compute_emd_distance(xs, ys), metrics.compute_emd_distance(xs, ys, assignment="device")
    print(f"compute_emd_distance n={n}: |host - device| = {abs(float(h) - float(d)):.3e} (bound {bound(5.0):.3e})")
    assert d.is_cuda and abs(float(h) - float(d)) <= bound(5.0)


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["equal", "ragged", "clamped", "large"])
def test_metrics_device_path_on_the_stored_reference_cases(hip, name):
    """The stored outputs of the reference's compute_emd_distance, with the bar of tests/test_metrics.py plus q."""
    from nova_pointcloud_amd import metrics

    z = np.load(GOLD, allow_pickle=False)
    pred, target, want = torch.from_numpy(z[f"{name}/pred"]).cuda(), torch.from_numpy(z[f"{name}/target"]).cuda(), float(z[f"{name}/emd"])
    emd = metrics.compute_emd_distance(pred, target, assignment="device")
    assert emd.is_cuda and abs(float(emd) - want) <= 1e-5 * want + Q


@pytest.mark.gpu
def test_largest_capacity_form(hip):
    """4096 points, once: pair 0 two random clouds (validity and the cost), pair 1 a cloud against a shuffle of itself,
    whose optimum is known without a solver: cost exactly 0 and the inverse of the shuffle."""
    from nova_pointcloud_amd import metrics

    n = 4096
    x, y = (v.copy() for v in clouds("normal", n))
    perm = np.random.RandomState(7).permutation(n)
    y[1] = x[1][perm]
    t0 = time.perf_counter()
    idx, cost, rounds = metrics.optimal_assignment(torch.from_numpy(x.copy()).cuda(), torch.from_numpy(y.copy()).cuda(), return_rounds=True)
    idx, cost = idx.cpu().numpy(), cost.cpu().numpy()
    print(f"n = 4096, B = 2: {time.perf_counter() - t0:.3f} s, rounds {rounds.tolist()}")
    for b in range(2):
        check_pair(x[b], y[b], None, idx[b], cost[b])
    assert float(cost[1]) == 0.0 and np.array_equal(perm[idx[1]], np.arange(n))
