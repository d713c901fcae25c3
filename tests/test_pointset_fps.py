"""Farthest point sampling (csrc/fps.hip, metrics.farthest_point_sample) and resampling clouds to a common point count
(metrics.resample_clouds, scripts/eval_pointsets.py --points): the input, device and C ABI checks and the pure-torch
resampling methods (CPU), and the kernel against a float64 restatement of the definition (GPU).

The definition restated here (include/nova_hip.h, nova_pointset_farthest_point_sample): idx[0] = s0, dist[0] = +inf,
mind = +inf; at step i, mind[j] = min(mind[j], |x[j] - x[idx[i-1]]|^2), idx[i] = the j with the largest mind[j], lowest j on
ties, dist[i] = mind[idx[i]].

Exact cases: integer coordinates make every float32 operation of the kernel exact, so indices and distances must equal the
float64 walk bit for bit, ties included. Random clouds: the kernel's own index sequence is replayed in float64 and every
choice must be a maximum up to REL = 1e-6: a float32 squared distance from float32 inputs carries at most about 8 units of
6e-8 relative error (three differences, three squares, two sums), a comparison of two carries twice that, 16 * 6e-8 = 9.6e-7.
Nothing is left out of the comparison.

Shapes: the ones the issue lists, and one N on each side of every boundary at which the kernel changes the points per
thread or the workgroup size (64 | 128 | 256 | 512 | 1024 | 2048 | 4096 | 8192, fps_config in csrc/fps.hip)."""
import ctypes
import functools
import os
import re
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REL = 1e-6
INF = float("inf")

SHAPES = [(3, 1, 1), (2, 63, 63), (2, 64, 10), (3, 777, 200), (2, 1025, 64), (1, 4099, 300), (1, 16384, 128),
          # both sides of every (P, T) boundary
          (2, 65, 20), (2, 128, 20), (2, 129, 20), (2, 256, 20), (2, 257, 20), (2, 512, 20), (2, 513, 20), (2, 1024, 20),
          (2, 2048, 24), (2, 2049, 24), (2, 4096, 24), (2, 4097, 24), (1, 8192, 24), (1, 8193, 24)]
BOUNDARY_N = (1, 2, 63, 64, 65, 128, 129, 256, 257, 512, 513, 1024, 1025, 2048, 2049, 4096, 4097, 8192, 8193, 16384)


# --------------------------------------------------------------------------------------------- restatement
def restated_fps(x, start, n):
    """The definition in float64 on x's device, all clouds of x [S, N, 3] at once: (idx int64 [S, n], dist float64 [S, n])."""
    x64 = x.double()
    S, N = x64.shape[:2]
    rows, ar = torch.arange(S, device=x.device), torch.arange(N, device=x.device)
    cur = torch.as_tensor(start, device=x.device).long().expand(S).clone()
    idx = torch.zeros(S, n, dtype=torch.int64, device=x.device)
    dist = torch.full((S, n), INF, dtype=torch.float64, device=x.device)
    mind = torch.full((S, N), INF, dtype=torch.float64, device=x.device)
    idx[:, 0] = cur
    for i in range(1, n):
        e = x64 - x64[rows, cur][:, None, :]
        mind = torch.minimum(mind, e[..., 0] * e[..., 0] + e[..., 1] * e[..., 1] + e[..., 2] * e[..., 2])
        m = mind.max(dim=1, keepdim=True).values
        cur = torch.where(mind == m, ar, N).min(dim=1).values  # lowest index at the maximum
        idx[:, i], dist[:, i] = cur, m[:, 0]
    return idx, dist


def lattice(S, N, seed, lo=-8, hi=8):
    return torch.randint(lo, hi + 1, (S, N, 3), generator=torch.Generator().manual_seed(seed)).float()


@functools.lru_cache(maxsize=None)
def lattice_case(S, N, n):
    """(clouds on the GPU, restated idx, restated dist) of the exact test at one shape; computed once, never modified."""
    x = lattice(S, N, 1000 + N).cuda()
    idx, dist = restated_fps(x, 0, n)
    return x, idx, dist


def test_restatement_on_small_cases():
    x = torch.tensor([[[0.0, 0, 0], [1, 0, 0], [5, 0, 0], [5, 0, 0], [-3, 0, 0]]])
    idx, dist = restated_fps(x, 0, 5)
    assert idx.tolist() == [[0, 2, 4, 1, 0]]  # 2 before its twin 3; once every mind is 0 the rule gives index 0
    assert dist.tolist() == [[INF, 25.0, 9.0, 1.0, 0.0]]
    idx, _ = restated_fps(torch.zeros(1, 6, 3), 4, 4)
    assert idx.tolist() == [[4, 0, 0, 0]]
    # the tie rule is exercised: on the (777, 200) lattice cloud most steps have a tied maximum, and float32 agrees
    x = lattice(1, 777, 1000 + 777)
    idx, dist = restated_fps(x, 0, 200)
    x64, mind, tied = x[0].double(), torch.full((777,), INF, dtype=torch.float64), 0
    for i in range(1, 200):
        mind = torch.minimum(mind, ((x64 - x64[idx[0, i - 1]]) ** 2).sum(-1))
        tied += int((mind == mind.max()).sum() > 1)
    assert tied >= 100
    assert bool((dist[0, 1:-1] >= dist[0, 2:]).all())


# --------------------------------------------------------------------------------------------- CPU: checks
def test_input_errors_on_cpu_tensors():
    from nova_pointcloud_amd import hip, metrics

    fps = metrics.farthest_point_sample
    ok = torch.zeros(2, 8, 3)
    with pytest.raises(ValueError, match=r"\[S, N, 3\]"):
        fps(torch.zeros(2, 8, 2), 4)
    with pytest.raises(ValueError, match=r"\[S, N, 3\]"):
        fps(torch.zeros(8, 3), 4)
    with pytest.raises(ValueError, match="points per cloud"):
        fps(torch.zeros(2, 0, 3), 1)
    with pytest.raises(ValueError, match="16384"):
        fps(torch.zeros(1, metrics.FPS_MAX_POINTS + 1, 3), 4)
    for bad in (0, 9, -1, 4.0, True):
        with pytest.raises(ValueError, match="n_samples"):
            fps(ok, bad)
    for bad in (-1, 8, [0, 8], torch.tensor([0, -1]), [0, 1, 2], torch.tensor([0.0, 1.0]), torch.zeros(2, 1, dtype=torch.long)):
        with pytest.raises(ValueError, match="start"):
            fps(ok, 4, start=bad)
    with pytest.raises(ValueError, match="finite"):
        fps(torch.full((1, 4, 3), float("nan")), 2)
    with pytest.raises(ValueError, match="finite"):
        fps(torch.tensor([[[0.0, 0, 0], [INF, 0, 0]]]), 2)
    # a valid CPU tensor: no CPU path
    for start in (0, 3, [1, 2], torch.tensor([7, 0])):
        with pytest.raises(hip.NovaHipError, match="GPU"):
            fps(ok, 4, start=start)
    with pytest.raises(hip.NovaHipError, match="GPU"):
        metrics.resample_clouds(ok, 4, method="fps")
    with pytest.raises(hip.NovaHipError, match="GPU"):
        metrics.resample_clouds(ok, 4)  # fps is the default
    header = open(os.path.join(ROOT, "include", "nova_hip.h")).read()
    assert metrics.FPS_MAX_POINTS == int(re.search(r"#define NOVA_FPS_MAX_POINTS (\d+)", header).group(1)) == 16384
    assert "transformer_pointcloud_nova.py:100-125" in header and "DEVIATION" in header
    for N in BOUNDARY_N:
        P, T = metrics.fps_kernel_shape(N)
        assert P * T >= N and P in (1, 2, 4, 8, 16) and T in (64, 256, 512, 1024)


def test_resample_clouds_on_cpu():
    from nova_pointcloud_amd import metrics

    assert metrics.RESAMPLE_METHODS == ("fps", "first", "random")
    x = torch.randn(3, 50, 3, generator=torch.Generator().manual_seed(0))
    assert torch.equal(metrics.resample_clouds(x, 20, method="first"), x[:, :20])
    for method in metrics.RESAMPLE_METHODS:
        assert metrics.resample_clouds(x, 50, method=method) is x
    a = metrics.resample_clouds(x, 20, method="random", generator=torch.Generator().manual_seed(7))
    b = metrics.resample_clouds(x, 20, method="random", generator=torch.Generator().manual_seed(7))
    c = metrics.resample_clouds(x, 20, method="random", generator=torch.Generator().manual_seed(8))
    assert a.shape == (3, 20, 3) and torch.equal(a, b) and not torch.equal(a, c)
    for s in range(3):
        where = (a[s][:, None, :] == x[s][None, :, :]).all(-1)  # [20, 50]: each row of the result is a row of the cloud
        assert bool((where.sum(1) == 1).all()) and where.any(0).sum() == 20  # and no row is taken twice
    with pytest.raises(ValueError, match="51"):
        metrics.resample_clouds(x, 51, method="first")
    with pytest.raises(ValueError, match="n_points"):
        metrics.resample_clouds(x, 0, method="first")
    with pytest.raises(ValueError, match="method"):
        metrics.resample_clouds(x, 20, method="voxel")
    with pytest.raises(ValueError, match=r"\[S, N, 3\]"):
        metrics.resample_clouds(x[0], 20, method="first")
    assert metrics.resample_clouds(torch.zeros(0, 9, 3), 4, method="random").shape == (0, 4, 3)


def test_abi_rejections():
    """Argument checks of nova_pointset_farthest_point_sample run before any device work (no GPU needed)."""
    from nova_pointcloud_amd import hip, metrics

    lib = hip.load(check_device=False)
    fn = lib.nova_pointset_farthest_point_sample
    x, idx, dist = ctypes.c_void_p(4096), ctypes.c_void_p(8192), ctypes.c_void_p(12288)  # never dereferenced: rejected first
    assert fn(x, None, idx, dist, 2, 0, 1, None) == -2                                  # N = 0
    assert b"NOVA_FPS_MAX_POINTS" in lib.nova_last_error()
    assert fn(x, None, idx, dist, 2, metrics.FPS_MAX_POINTS + 1, 8, None) == -2         # N above the cap
    assert b"16384" in lib.nova_last_error()
    assert fn(x, None, idx, dist, 2, 8, 0, None) == -1                                  # n = 0
    assert fn(x, None, idx, dist, 2, 8, 9, None) == -1                                  # n = N + 1
    assert b"outside 1 .. N" in lib.nova_last_error()
    assert fn(x, None, None, dist, 2, 8, 4, None) == -1                                 # null idx
    assert b"null" in lib.nova_last_error()
    assert fn(None, None, idx, dist, 2, 8, 4, None) == -1                               # null x
    assert fn(None, None, None, None, 0, 8, 4, None) == 0                               # S = 0: nothing to do
    assert fn(None, None, None, None, -3, 8, 4, None) == 0
    assert fn(None, None, None, None, 0, 0, 4, None) == -2                              # but the shape is still checked
    assert lib.nova_version() == 405


def test_script_arguments(tmp_path):
    sys.path.insert(0, os.path.join(ROOT, "scripts"))
    import eval_pointsets

    ns = vars(eval_pointsets.build_parser().parse_args(["a", "b"]))
    assert ns.pop("points") is None and ns.pop("resample") == "fps" and ns.pop("resample_seed") == 0
    assert ns == {"samples": "a", "refs": "b", "out": None, "emd": False, "jsd": False, "jsd_resolution": 28, "normalize": None,
                  "batch_size": None}  # what the script took before --points existed
    ns = eval_pointsets.build_parser().parse_args(["a", "b", "--points", "512", "--resample", "random", "--resample-seed", "3"])
    assert (ns.points, ns.resample, ns.resample_seed) == (512, "random", 3)
    with pytest.raises(SystemExit):
        eval_pointsets.build_parser().parse_args(["a", "b", "--resample", "voxel"])
    np.save(tmp_path / "dense.npy", np.zeros((2, 40, 3), dtype=np.float32))
    np.save(tmp_path / "sparse.npy", np.zeros((2, 30, 3), dtype=np.float32))
    with pytest.raises(ValueError, match=r"refs \(.*sparse\.npy\) has 30 points"):
        eval_pointsets.main([str(tmp_path / "dense.npy"), str(tmp_path / "sparse.npy"), "--points", "32"])
    with pytest.raises(ValueError, match=r"samples \(.*sparse\.npy\) has 30 points"):
        eval_pointsets.main([str(tmp_path / "sparse.npy"), str(tmp_path / "dense.npy"), "--points", "32", "--resample", "first"])
    with pytest.raises(ValueError, match="--points"):
        eval_pointsets.main([str(tmp_path / "dense.npy"), str(tmp_path / "sparse.npy"), "--points", "0"])
    assert "BEFORE --normalize" in eval_pointsets.__doc__


# --------------------------------------------------------------------------------------------- GPU
def kernel(x, n, **kw):
    from nova_pointcloud_amd import metrics

    idx, dist = metrics.farthest_point_sample(x, n, return_distances=True, **kw)
    assert idx.shape == (x.shape[0], n) and idx.dtype == torch.int64 and idx.device == x.device
    assert dist.shape == (x.shape[0], n) and dist.dtype == torch.float32
    return idx, dist


@pytest.mark.gpu
@pytest.mark.parametrize("S,N,n", SHAPES)
def test_exact_with_ties(hip, S, N, n):
    x, want_idx, want_dist = lattice_case(S, N, n)
    idx, dist = kernel(x, n)
    steps = torch.nonzero((idx != want_idx).any(0)).reshape(-1)
    print(f"S {S} N {N} n {n}: first differing step {int(steps[0]) if steps.numel() else None}")
    assert torch.equal(idx, want_idx)
    assert torch.equal(dist.double(), want_dist)  # integers up to 3 * 16^2: exact in both formats


@pytest.mark.gpu
def test_exact_all_zero_tail_and_equal_points(hip):
    from nova_pointcloud_amd import metrics

    x = lattice(2, 63, 5, -1, 1).cuda()  # at most 27 distinct points, n = N: the tail has every mind at 0
    want_idx, want_dist = restated_fps(x, 0, 63)
    idx, dist = kernel(x, 63)
    assert torch.equal(idx, want_idx) and torch.equal(dist.double(), want_dist)
    distinct = [len({tuple(p) for p in c.tolist()}) for c in x.cpu()]
    for s in range(2):
        assert distinct[s] <= 27 and bool((dist[s, distinct[s]:] == 0).all()) and bool((idx[s, distinct[s]:] == 0).all())
        assert bool((dist[s, 1:distinct[s]] > 0).all())
    for N, s0 in ((40, 17), (300, 299), (5000, 4321)):
        same = torch.full((1, N, 3), 2.5).cuda()
        idx, dist = kernel(same, 9, start=s0)
        assert idx.tolist() == [[s0] + [0] * 8] and dist.tolist() == [[INF] + [0.0] * 8]
    assert metrics.farthest_point_sample(torch.zeros(0, 7, 3).cuda(), 3).shape == (0, 3)


@pytest.mark.gpu
@pytest.mark.parametrize("S,N,n", SHAPES)
def test_exact_under_translation(hip, S, N, n):
    x, want_idx, want_dist = lattice_case(S, N, n)
    shifted = x + torch.tensor([4096.0, -4096.0, 4096.0], device=x.device)  # differences stay exact; squared norms do not
    idx, dist = kernel(shifted, n)
    unshifted, _ = kernel(x, n)
    assert torch.equal(idx, unshifted) and torch.equal(idx, want_idx) and torch.equal(dist.double(), want_dist)


@pytest.mark.gpu
@pytest.mark.parametrize("N", BOUNDARY_N)
def test_last_point_and_every_slot_are_reachable(hip, N):
    """Point N - 1 (the last slot that is not padding) far away is chosen first; then, one cloud per probe, a far point at
    index j for j spread over the whole cloud: every register slot and every wave holds a winner once."""
    probes = sorted({0, N - 1, N // 2, N // 3, (2 * N) // 3, max(0, N - 65), min(N - 1, 64), min(N - 1, 255)} | set(range(0, N, max(1, N // 16))))
    x = lattice(len(probes), N, 77, -2, 2)
    for c, j in enumerate(probes):
        x[c, j] = torch.tensor([100.0, -50.0, 25.0])
    n = min(N, 3)
    start = [1 if (j == 0 and N > 1) else 0 for j in probes]
    idx, dist = kernel(x.cuda(), n, start=start)
    want_idx, want_dist = restated_fps(x.cuda(), start, n)
    assert torch.equal(idx, want_idx) and torch.equal(dist.double(), want_dist)
    if N > 1:
        assert idx[:, 1].tolist() == probes


@pytest.mark.gpu
@pytest.mark.parametrize("S,N,n", SHAPES)
def test_random_clouds(hip, S, N, n):
    x = torch.randn(S, N, 3, generator=torch.Generator().manual_seed(2000 + N)).cuda()
    start = [(7 * s + 3) % N for s in range(S)]
    idx, dist = kernel(x, n, start=start)
    assert idx[:, 0].tolist() == start and bool(torch.isinf(dist[:, 0]).all()) and bool((dist[:, 0] > 0).all())
    assert all(len(set(row)) == n for row in idx.tolist())  # distinct: a Gaussian cloud has no repeated point
    assert bool((dist[:, 1:-1] >= dist[:, 2:]).all())  # non-increasing, exactly
    x64, rows = x.double(), torch.arange(S, device=x.device)
    mind = torch.full((S, N), INF, dtype=torch.float64, device=x.device)
    worst_choice, worst_dist = 0.0, 0.0
    for i in range(1, n):
        e = x64 - x64[rows, idx[:, i - 1]][:, None, :]
        mind = torch.minimum(mind, (e * e).sum(-1))
        chosen, best = mind[rows, idx[:, i]], mind.max(dim=1).values
        worst_choice = max(worst_choice, float(((best - chosen) / best).max()))
        worst_dist = max(worst_dist, float(((dist[:, i].double() - chosen).abs() / chosen).max()))
    print(f"S {S} N {N} n {n}: largest relative shortfall of a choice {worst_choice:.3e}, of a distance {worst_dist:.3e} (bound {REL:.0e})")
    assert worst_choice <= REL  # mind64[idx[i]] >= max_j mind64[j] (1 - REL) at every step
    assert worst_dist <= REL


@pytest.mark.gpu
def test_independence_of_batch_split_stream_and_layout(hip):
    from nova_pointcloud_amd import metrics

    S, N, n = 5, 777, 100
    x = torch.randn(S, N, 3, generator=torch.Generator().manual_seed(31)).cuda()
    start = torch.tensor([0, 776, 13, 400, 5])
    idx, dist = kernel(x, n, start=start.cuda())
    same = lambda got: torch.equal(got[0], idx) and torch.equal(got[1], dist)
    assert same(kernel(x, n, start=start)) and same(kernel(x, n, start=start.tolist()))  # device, CPU tensor or list
    for s in range(S):
        one = kernel(x[s:s + 1], n, start=int(start[s]))
        assert torch.equal(one[0][0], idx[s]) and torch.equal(one[1][0], dist[s]), s
    for per in (1, 2, 4):
        assert same(kernel(x, n, start=start, max_clouds_per_launch=per)), per
    assert torch.equal(metrics.farthest_point_sample(x, n, start=start), idx)  # without the distances
    stream = torch.cuda.Stream()
    stream.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(stream):
        on_stream = kernel(x, n, start=start)
    stream.synchronize()
    assert same(on_stream)
    wide = torch.zeros(S, 2 * N, 6, device="cuda")
    wide[:, ::2, 1:4] = x
    view = wide[:, ::2, 1:4]
    assert not view.is_contiguous() and same(kernel(view, n, start=start))
    assert same(kernel(x.double(), n, start=start))  # taken as float32, as every function of the module takes its points
    got = metrics.resample_clouds(x, n, start=start)
    assert torch.equal(got, torch.gather(x, 1, idx[:, :, None].expand(S, n, 3)))
    with pytest.raises(ValueError, match="max_clouds_per_launch"):
        metrics.farthest_point_sample(x, n, max_clouds_per_launch=0)


@pytest.mark.gpu
def test_eval_pointsets_script_points_flag(hip, tmp_path, capsys):
    sys.path.insert(0, os.path.join(ROOT, "scripts"))
    import json

    import eval_pointsets

    from nova_pointcloud_amd import metrics

    g = torch.Generator().manual_seed(90)
    smp = torch.randn(5, 3000, 3, generator=g) * torch.tensor([1.0, 0.7, 0.5]) + 2.0
    ref = torch.randn(4, 2500, 3, generator=g) - 1.0
    np.save(tmp_path / "smp.npy", smp.numpy())
    np.save(tmp_path / "ref.npy", ref.numpy())
    args = [str(tmp_path / "smp.npy"), str(tmp_path / "ref.npy")]
    res = eval_pointsets.main(args + ["--points", "256", "--emd", "--jsd", "--normalize", "unit_sphere"])
    out = capsys.readouterr()
    assert len(out.out.strip().splitlines()) == 1 and json.loads(out.out) == res
    rs, rr = metrics.resample_clouds(smp.cuda(), 256), metrics.resample_clouds(ref.cuda(), 256)
    assert rs.shape == (5, 256, 3) and rr.shape == (4, 256, 3)
    direct = metrics.compute_all_metrics(metrics.normalize_clouds(rs, "unit_sphere"), metrics.normalize_clouds(rr, "unit_sphere"),
                                         emd=True, jsd=True)
    assert {k: res[k] for k in direct} == direct  # the same numbers
    assert set(metrics.METRIC_KEYS + metrics.EMD_METRIC_KEYS + ("jsd",)) <= set(direct)
    assert res["resample"] == "fps" and res["points"] == 256 and res["sample_points"] == 256 and res["ref_points"] == 256
    # the other methods go through the same path
    first = eval_pointsets.main(args + ["--points", "256", "--resample", "first", "--emd"])
    assert {k: first[k] for k in metrics.EMD_METRIC_KEYS} == {
        k: v for k, v in metrics.compute_all_metrics(smp[:, :256].cuda(), ref[:, :256].cuda(), emd=True).items() if k in metrics.EMD_METRIC_KEYS}
    rnd = [eval_pointsets.main(args + ["--points", "256", "--resample", "random", "--resample-seed", str(seed)]) for seed in (1, 1, 2)]
    strip = lambda r: {k: v for k, v in r.items() if k != "seconds"}
    assert strip(rnd[0]) == strip(rnd[1]) != strip(rnd[2]) and rnd[0]["resample"] == "random"
    capsys.readouterr()
    # without --points the script is what it was: no new keys, and the EMD still refuses unequal point counts
    plain = eval_pointsets.main(args)
    assert "resample" not in plain and "points" not in plain and plain["sample_points"] == 3000 and plain["ref_points"] == 2500
    with pytest.raises(ValueError, match="equal point counts"):
        eval_pointsets.main(args + ["--emd"])
