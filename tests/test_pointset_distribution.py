"""Set-level metrics of generated point clouds (MMD, COV, 1-NNA under the Chamfer distance): the matrix logic against a
NumPy restatement of the definitions and hand-built cases (CPU), the C ABI checks and the point-set loader (CPU), and
the all-pairs Chamfer kernel (csrc/chamfer.hip) against float64 (GPU).

Definitions restated here: CD(X, Y) = mean_x min_y |x - y|^2 + mean_y min_x |x - y|^2 (squared, no clamp);
lgan_mmd-CD = mean_r min_s D_rs; lgan_mmd_smp-CD = mean_s min_r D_rs; lgan_cov-CD = |{argmin_r D_rs[r, s]}| / S_r
(ties to the lowest r); 1-NN-CD-acc(_t/_f) = the leave-one-out 1-NN accuracy on the pooled [R; Sm] (diagonal excluded,
ties to the lowest pooled index) over all / reference / sample elements."""
import ctypes
import os

import numpy as np
import pytest
import torch

KEYS = ("lgan_mmd-CD", "lgan_mmd_smp-CD", "lgan_cov-CD", "1-NN-CD-acc", "1-NN-CD-acc_t", "1-NN-CD-acc_f")


# --------------------------------------------------------------------------------------------- float64 restatement
def np_metrics(d_rs, d_rr, d_ss):
    d_rs, d_rr, d_ss = (np.asarray(m, dtype=np.float64) for m in (d_rs, d_rr, d_ss))
    S_r, S_s = d_rs.shape
    out = {"lgan_mmd-CD": float(np.mean(np.min(d_rs, axis=1))), "lgan_mmd_smp-CD": float(np.mean(np.min(d_rs, axis=0)))}
    covered = set()
    for s in range(S_s):
        col = d_rs[:, s]
        covered.add(min(r for r in range(S_r) if col[r] == col.min()))
    out["lgan_cov-CD"] = len(covered) / S_r
    pooled = np.block([[d_rr, d_rs], [d_rs.T, d_ss]])
    n = S_r + S_s
    correct = []
    for i in range(n):
        others = [j for j in range(n) if j != i]
        best = min(pooled[i, j] for j in others)
        nn = min(j for j in others if pooled[i, j] == best)
        correct.append((nn < S_r) == (i < S_r))
    correct = np.array(correct, dtype=np.float64)
    out["1-NN-CD-acc"], out["1-NN-CD-acc_t"], out["1-NN-CD-acc_f"] = correct.mean(), correct[:S_r].mean(), correct[S_r:].mean()
    return out


def cd64(x, y):
    """CD(x[a], y[b]) in float64 on x's device, [A, B]."""
    x, y = x.double(), y.double()
    out = torch.empty(x.shape[0], y.shape[0], dtype=torch.float64)
    for a in range(x.shape[0]):
        for b in range(y.shape[0]):
            d = torch.zeros(x.shape[1], y.shape[1], dtype=torch.float64, device=x.device)
            for k in range(3):
                d += (x[a, :, k, None] - y[b, None, :, k]) ** 2
            out[a, b] = d.min(dim=1).values.mean() + d.min(dim=0).values.mean()
    return out


def metrics_as_floats(m):
    return {k: float(v) for k, v in m.items()}


# --------------------------------------------------------------------------------------------- CPU: matrix logic
@pytest.mark.parametrize("seed,S_r,S_s", [(0, 7, 11), (1, 13, 5), (2, 1, 3)])
def test_matrix_metrics_match_numpy_restatement(seed, S_r, S_s):
    from nova_pointcloud_amd.metrics import distribution_metrics_from_matrices

    g = np.random.default_rng(seed)
    d_rs, d_rr, d_ss = g.random((S_r, S_s)), g.random((S_r, S_r)), g.random((S_s, S_s))
    d_rr, d_ss = d_rr + d_rr.T, d_ss + d_ss.T
    got = distribution_metrics_from_matrices(*(torch.from_numpy(m).float() for m in (d_rs, d_rr, d_ss)))
    assert set(got) == set(KEYS)
    want = np_metrics(*(torch.from_numpy(m).float().numpy() for m in (d_rs, d_rr, d_ss)))
    for k in ("lgan_cov-CD", "1-NN-CD-acc", "1-NN-CD-acc_t", "1-NN-CD-acc_f"):
        assert float(got[k]) == want[k], k
    for k in ("lgan_mmd-CD", "lgan_mmd_smp-CD"):
        assert abs(float(got[k]) - want[k]) <= 1e-6 * abs(want[k]), k


def test_duplicated_samples_are_covered_and_inseparable():
    """Samples that are exact copies of the references: COV = 1 and every 1-NN is the copy across the sets (acc = 0)."""
    from nova_pointcloud_amd.metrics import distribution_metrics_from_matrices

    g = np.random.default_rng(3)
    p = g.random((6, 2)) * 10
    d = ((p[:, None] - p[None]) ** 2).sum(-1) + 1.0  # CD of distinct clouds > 0; of a cloud with its copy 0
    d_rs = d - np.eye(6)
    m = metrics_as_floats(distribution_metrics_from_matrices(*(torch.from_numpy(x) for x in (d_rs, d, d))))
    assert m["lgan_cov-CD"] == 1.0 and m["lgan_mmd-CD"] == 0.0 and m["lgan_mmd_smp-CD"] == 0.0
    assert m["1-NN-CD-acc"] == 0.0 and m["1-NN-CD-acc_t"] == 0.0 and m["1-NN-CD-acc_f"] == 0.0


def test_far_apart_clusters_are_separable():
    from nova_pointcloud_amd.metrics import distribution_metrics_from_matrices

    g = np.random.default_rng(4)
    ref, smp = g.random((5, 3)), g.random((4, 3)) + 100.0
    cd = lambda a, b: ((a[:, None] - b[None]) ** 2).sum(-1)
    m = metrics_as_floats(distribution_metrics_from_matrices(*(torch.from_numpy(x) for x in (cd(ref, smp), cd(ref, ref), cd(smp, smp)))))
    assert m["1-NN-CD-acc"] == 1.0 and m["1-NN-CD-acc_t"] == 1.0 and m["1-NN-CD-acc_f"] == 1.0
    assert m == pytest.approx(np_metrics(cd(ref, smp), cd(ref, ref), cd(smp, smp)), rel=1e-12)


def test_planted_ties_go_to_the_lowest_index():
    from nova_pointcloud_amd.metrics import distribution_metrics_from_matrices

    # COV: every sample is equally near references 1 and 2 (and nearer than to 0): only reference 1 is covered
    d_rs = torch.tensor([[5.0, 5.0], [1.0, 1.0], [1.0, 1.0]])
    d_rr = torch.tensor([[0.0, 9.0, 9.0], [9.0, 0.0, 9.0], [9.0, 9.0, 0.0]])
    d_ss = torch.tensor([[0.0, 9.0], [9.0, 0.0]])
    m = metrics_as_floats(distribution_metrics_from_matrices(d_rs, d_rr, d_ss))
    assert m["lgan_cov-CD"] == 1.0 / 3.0 and m == np_metrics(d_rs, d_rr, d_ss)
    # 1-NN: reference 0 ties between reference 1 (pooled 1) and sample 0 (pooled 2) -> reference 1 -> correct;
    # sample 0 ties between reference 0 (pooled 0) and sample 1 (pooled 3) -> reference 0 -> wrong
    d_rs = torch.tensor([[2.0, 7.0], [8.0, 8.0]])
    d_rr = torch.tensor([[0.0, 2.0], [2.0, 0.0]])
    d_ss = torch.tensor([[0.0, 2.0], [2.0, 0.0]])
    m = metrics_as_floats(distribution_metrics_from_matrices(d_rs, d_rr, d_ss))
    assert m["1-NN-CD-acc_t"] == 1.0 and m["1-NN-CD-acc_f"] == 0.5 and m["1-NN-CD-acc"] == 0.75
    assert m == np_metrics(d_rs, d_rr, d_ss)
    # reference 0 now ties between the two samples (pooled 2 and 3), sample 0 between reference 0 and sample 1, and
    # sample 1 between reference 0 and sample 0: the lower pooled index wins each time, and each choice is wrong
    d_rs = torch.tensor([[2.0, 2.0], [8.0, 8.0]])
    d_rr = torch.tensor([[0.0, 3.0], [3.0, 0.0]])
    m = metrics_as_floats(distribution_metrics_from_matrices(d_rs, d_rr, d_ss))
    assert m["1-NN-CD-acc_t"] == 0.5 and m["1-NN-CD-acc_f"] == 0.0 and m == np_metrics(d_rs, d_rr, d_ss)


def test_matrix_shapes_must_pool():
    from nova_pointcloud_amd.metrics import distribution_metrics_from_matrices

    with pytest.raises(ValueError):
        distribution_metrics_from_matrices(torch.zeros(3, 2), torch.zeros(3, 3), torch.zeros(3, 3))


# --------------------------------------------------------------------------------------------- CPU: input checks
def test_set_metrics_refuse_cpu_tensors_bad_shapes_and_non_finite_points():
    from nova_pointcloud_amd import hip, metrics

    with pytest.raises(hip.NovaHipError):
        metrics.chamfer_matrix(torch.zeros(2, 8, 3))
    with pytest.raises(hip.NovaHipError):
        metrics.chamfer_matrix(torch.zeros(2, 8, 3), torch.zeros(3, 5, 3))
    with pytest.raises(hip.NovaHipError):
        metrics.compute_all_metrics(torch.zeros(2, 8, 3), torch.zeros(3, 8, 3))
    for bad in (torch.zeros(8, 3), torch.zeros(2, 8, 2), torch.zeros(2, 3, 8)):
        with pytest.raises(ValueError):
            metrics.chamfer_matrix(bad)
        with pytest.raises(ValueError):
            metrics.compute_all_metrics(bad, torch.zeros(3, 8, 3))
    for v in (float("nan"), float("inf")):
        x = torch.zeros(2, 8, 3)
        x[1, 3, 2] = v
        with pytest.raises(ValueError, match="finite"):
            metrics.chamfer_matrix(x)
        with pytest.raises(ValueError, match="finite"):
            metrics.compute_all_metrics(torch.zeros(2, 8, 3), x)


def test_chamfer_matrix_abi_checks():
    """Argument checks of nova_pointset_chamfer_matrix run before any device work (no GPU needed)."""
    from nova_pointcloud_amd import hip

    fn = hip.load(check_device=False).nova_pointset_chamfer_matrix
    p, q, c = ctypes.c_void_p(4096), ctypes.c_void_p(8192), ctypes.c_void_p(12288)  # never dereferenced: rejected first
    assert fn(None, q, c, 2, 3, 8, 8, 3, 0, None) == -1          # null x
    assert fn(p, None, c, 2, 3, 8, 8, 3, 0, None) == -1          # null y
    assert fn(p, q, None, 2, 3, 8, 8, 3, 0, None) == -1          # null cd
    assert fn(p, q, c, 2, 3, 8, 8, 2, 0, None) == -1             # ldc < B
    assert fn(p, q, c, 3, 3, 8, 8, 3, 1, None) == -1             # symmetric with x != y
    assert fn(p, p, c, 3, 2, 8, 8, 3, 1, None) == -1             # symmetric with A != B
    assert fn(p, p, c, 3, 3, 8, 9, 3, 1, None) == -1             # symmetric with N != M
    assert b"symmetric" in hip.load(check_device=False).nova_last_error()


# --------------------------------------------------------------------------------------------- CPU: loader
def test_point_set_loader_forms_agree(tmp_path):
    from nova_pointcloud_amd.metrics import load_point_clouds, save_point_clouds

    pts = np.random.default_rng(5).standard_normal((12, 33, 3)).astype(np.float32)
    np.save(tmp_path / "points.npy", pts)
    save_point_clouds(pts, "sample", str(tmp_path / "dir"))  # sample_0 .. sample_11: natural order, not lexical
    a, b = load_point_clouds(str(tmp_path / "points.npy")), load_point_clouds(str(tmp_path / "dir"))
    assert a.dtype == np.float32 and b.dtype == np.float32
    assert np.array_equal(a, pts) and np.array_equal(b, pts)


def test_point_set_loader_rejects_bad_input(tmp_path):
    from nova_pointcloud_amd.metrics import load_point_clouds

    with pytest.raises(FileNotFoundError):
        load_point_clouds(str(tmp_path / "missing.npy"))
    (tmp_path / "empty").mkdir()
    with pytest.raises(FileNotFoundError):
        load_point_clouds(str(tmp_path / "empty"))
    np.save(tmp_path / "flat.npy", np.zeros((10, 3), np.float32))
    with pytest.raises(ValueError):
        load_point_clouds(str(tmp_path / "flat.npy"))
    np.save(tmp_path / "four.npy", np.zeros((2, 10, 4), np.float32))
    with pytest.raises(ValueError):
        load_point_clouds(str(tmp_path / "four.npy"))
    d = tmp_path / "ragged"
    d.mkdir()
    np.save(d / "s_0.npy", np.zeros((10, 3), np.float32))
    np.save(d / "s_1.npy", np.zeros((11, 3), np.float32))
    with pytest.raises(ValueError):
        load_point_clouds(str(d))


# --------------------------------------------------------------------------------------------- GPU
def sphere_clouds(S, n, seed, device="cuda"):
    g = torch.Generator().manual_seed(seed)
    p = torch.randn(S, n, 3, generator=g, dtype=torch.float64)
    p = p / p.norm(dim=-1, keepdim=True) * (1 + 0.02 * torch.randn(S, n, 1, generator=g, dtype=torch.float64))
    return p.float().to(device)


@pytest.mark.gpu
@pytest.mark.parametrize("A,B,N,M", [(1, 1, 1, 1), (3, 5, 257, 1025), (5, 6, 300, 40), (7, 4, 2048, 2048), (2, 3, 4097, 1000),
                                     (2, 2, 2500, 3000)])
def test_chamfer_matrix_matches_float64(hip, A, B, N, M):
    from nova_pointcloud_amd.metrics import chamfer_matrix

    x, y = sphere_clouds(A, N, 10 + N), sphere_clouds(B, M, 20 + M)
    shift = torch.tensor([8.0, -8.0, 8.0], device="cuda")
    for xs, ys in ((x, y), (x + shift, y + shift)):
        got = chamfer_matrix(xs, ys)
        assert got.shape == (A, B) and got.dtype == torch.float32 and got.is_cuda
        want = cd64(xs, ys)
        err = ((got.cpu().double() - want).abs() / want).max().item()
        assert err <= 1e-5, (A, B, N, M, err)


@pytest.mark.gpu
@pytest.mark.parametrize("S,N", [(9, 300), (3, 2500)])
def test_chamfer_matrix_symmetric_mode(hip, S, N):
    from nova_pointcloud_amd.metrics import chamfer_matrix

    x = sphere_clouds(S, N, 30 + N) * torch.linspace(0.5, 1.5, S, device="cuda").view(S, 1, 1)
    sym, full = chamfer_matrix(x), chamfer_matrix(x, x)
    assert torch.equal(sym, sym.t())
    assert ((sym - full).abs() / full.abs().clamp_min(1e-30)).max().item() <= 1e-6
    assert torch.equal(torch.triu(sym), torch.triu(full))  # an entry a <= b is computed the same way in both modes


@pytest.mark.gpu
def test_chamfer_matrix_is_reproducible(hip):
    from nova_pointcloud_amd.metrics import chamfer_matrix

    x, y = sphere_clouds(7, 513, 40), sphere_clouds(5, 700, 41)
    full = chamfer_matrix(x, y)
    assert torch.equal(full, chamfer_matrix(x, y))
    for cap in (1, 3, 8):
        assert torch.equal(full, chamfer_matrix(x, y, max_pairs_per_launch=cap))
    sym = chamfer_matrix(x)
    assert torch.equal(sym, chamfer_matrix(x))
    for cap in (1, 3, 8):
        assert torch.equal(sym, chamfer_matrix(x, max_pairs_per_launch=cap))


@pytest.mark.gpu
def test_compute_all_metrics_end_to_end(hip):
    from nova_pointcloud_amd.metrics import compute_all_metrics

    g = torch.Generator().manual_seed(50)
    centres = torch.rand(24, 1, 3, generator=g) * 3.0  # per-cloud offsets: the CDs between clouds are well separated
    ref = sphere_clouds(24, 2048, 51) + centres.cuda()
    smp = sphere_clouds(20, 2048, 52) + (centres[:20] + 0.3 * torch.rand(20, 1, 3, generator=g)).cuda()
    got = compute_all_metrics(smp, ref, batch_size=64)
    d_rs, d_rr, d_ss = cd64(ref, smp), cd64(ref, ref), cd64(smp, smp)
    # the nearest-neighbour choices are not within float32 error of a tie
    pooled = torch.cat([torch.cat([d_rr, d_rs], 1), torch.cat([d_rs.t(), d_ss], 1)], 0).fill_diagonal_(float("inf"))
    two = pooled.topk(2, dim=1, largest=False).values
    assert ((two[:, 1] - two[:, 0]) / two[:, 0]).min().item() > 1e-4
    two = d_rs.topk(2, dim=0, largest=False).values
    assert ((two[1] - two[0]) / two[0]).min().item() > 1e-4
    want = np_metrics(d_rs.numpy(), d_rr.numpy(), d_ss.numpy())
    assert set(got) == set(KEYS) and all(isinstance(v, float) for v in got.values())
    for k in ("lgan_cov-CD", "1-NN-CD-acc", "1-NN-CD-acc_t", "1-NN-CD-acc_f"):
        assert got[k] == want[k], k
    for k in ("lgan_mmd-CD", "lgan_mmd_smp-CD"):
        assert abs(got[k] - want[k]) <= 1e-5 * want[k], k
