"""Point-set metrics and export for generated point clouds on MI355X.

Same function names, arguments and results as the reference's evaluation code
  compute_chamfer_distance, compute_emd_distance            test_optimize.py:354-415
  distChamfer, emd_approx, robust_chamfer_distance, robust_emd   train_newloss.py:316-385
  GlobalNormalizer                                           test_optimize.py:32-77
  np.save of each generated point cloud                      README.md:108-113
with the O(N M) distance work (torch.cdist + min, the assignment cost matrix) in libnova_hip.so
(csrc/pointset.hip). The optimal assignment itself is scipy's linear_sum_assignment on the host by default, exactly as in
the reference; assignment="device" solves it on the GPU instead (optimal_assignment, csrc/assign.hip: an integer auction
whose mean matched distance is within 2^-18 of the optimum). GPU tensors only: there is no CPU path here (NovaHipError
for CPU tensors or a missing library).

Set-level quality of a generated set against a reference set (MMD, COV, 1-NNA under the Chamfer distance, the numbers
of PointFlow and its successors): chamfer_matrix (csrc/chamfer.hip), distribution_metrics_from_matrices,
compute_all_metrics, and load_point_clouds for what save_point_clouds or `bench.py --dump-outputs` wrote. The same three
metrics under the EMD of that literature (compute_all_metrics(..., emd=True)) run on emd_matrix (csrc/emd.hip): the
approximate matching of Fan et al. ("approxmatch", PointFlow's emd_approx), not the exact assignment of
compute_emd_distance above. It is asymmetric, so the full matrices are computed and oriented as PointFlow orients them.

The seventh column of those tables, the JSD between the two sets' occupancy distributions on a 28^3 grid in the ball of
radius 0.5: occupancy_grid (csrc/occupancy.hip), entropy_of_occupancy_grid, jensen_shannon_divergence,
jsd_between_point_cloud_sets and compute_all_metrics(..., jsd=True). The grid is fixed in space, so the JSD depends on
how the clouds are normalised: normalize_clouds puts each cloud into that ball or cube.

Bringing sets to the point count those metrics need (generated clouds have 2048 points, published reference shapes are
stored denser, and the EMD takes equal counts of at most 4096): farthest_point_sample (csrc/fps.hip) and resample_clouds.

The exact EMD on the GPU: optimal_assignment (csrc/assign.hip), and assignment="device" of compute_emd_distance, emd_approx
and robust_emd.

Local statistics of a cloud: knn_points (csrc/knn.hip), the exact k nearest neighbours of every point with their squared
distances and no [N, M] matrix, and local_density on it, the reference's compute_local_density
(transformer_pointcloud_nova.py:81-89) with the point itself excluded by index rather than by dropping a column.

Thinning a dense cloud without dropping points: kernel_interpolate (csrc/interp.hip), every query the softmax(-distance /
temperature) average of all source values with no [T, N] matrix, and on it the reference's feature_aware_interpolation
(transformer_pointcloud_nova.py:128-152) and adaptive_sampling (:92-97).
"""
import json
import math
import os
import re

import numpy as np
import torch

from . import hip
from ._pointset import (ASSIGNMENT_MODES, INTERP_MAX_CHANNELS, INTERP_MAX_POINTS, _INTERP_PAIRS_PER_LAUNCH,  # noqa: F401  (re-exported)
                        _adaptive_sampling, _assignment_mode, _at, _at_least_one, _check_clamp, _check_clouds, _clouds,
                        _feature_aware_interpolation, _interp_arguments, _interp_scale, _launches, _launching, _points)


def nn_dist(x, y, clamp, unit_norm=False):
    """d[b, i] = min_j ||x[b, i] - y[b, j]|| after clamping coordinates to [-clamp, clamp] (optionally unit-normalised)."""
    x, y = _points(x, "x"), _points(y, "y")
    B, N, M = x.shape[0], x.shape[1], y.shape[1]
    d = torch.empty(B, N, dtype=torch.float32, device=x.device)
    with torch.cuda.device(x.device):
        hip.call("nova_pointset_nn_dist", x.data_ptr(), y.data_ptr(), d.data_ptr(), B, N, M, -float(clamp), float(clamp),
                 1 if unit_norm else 0, hip.stream_ptr())
    return d


def pairwise_dist(x, y, clamp):
    """D[b, i, j] = ||x[b, i] - y[b, j]|| (the `torch.cdist` cost matrix of the EMD assignment)."""
    x, y = _points(x, "x"), _points(y, "y")
    B, N, M = x.shape[0], x.shape[1], y.shape[1]
    D = torch.empty(B, N, M, dtype=torch.float32, device=x.device)
    with torch.cuda.device(x.device):
        hip.call("nova_pointset_pairwise_dist", x.data_ptr(), y.data_ptr(), D.data_ptr(), B, N, M, -float(clamp), float(clamp),
                 hip.stream_ptr())
    return D


# ----------------------------------------------------------------------------------------------------
# test_optimize.py:354-415
# ----------------------------------------------------------------------------------------------------
def compute_chamfer_distance(pred, target):
    """Density-weighted Chamfer distance (test_optimize.py:354-381): coordinates clamped to +-5, both sets cut to the
    smaller point count, nearest-neighbour distances weighted by 1 / (d.detach() + 1e-6), result clamped to [0, 10]."""
    n = min(pred.shape[1], target.shape[1])
    pred, target = pred[:, :n], target[:, :n]
    d_pt, d_tp = nn_dist(pred, target, 5.0), nn_dist(target, pred, 5.0)
    dist1 = (d_pt * (1.0 / (d_pt + 1e-6))).mean(dim=1)
    dist2 = (d_tp * (1.0 / (d_tp + 1e-6))).mean(dim=1)
    return (dist1 + dist2).mean().clamp(0.0, 10.0)


def _assignment_mean(cost):
    from scipy.optimize import linear_sum_assignment

    rows, cols = linear_sum_assignment(cost)
    return cost[rows, cols].mean()


def compute_emd_distance(pred, target, assignment="host"):
    """Earth mover's distance by optimal assignment (test_optimize.py:385-415): clamp +-5, equal point counts, mean
    matched distance per sample, batch mean in [0, 10]. assignment="host" (the default) is scipy linear_sum_assignment on
    the host, as in the reference; "device" is optimal_assignment on the GPU with the same clamp (no cost matrix, no copy;
    each sample's mean within ASSIGN_QUANTUM = 2^-18 of the host's)."""
    device = _assignment_mode(assignment)
    n = min(pred.shape[1], target.shape[1])
    if device:
        emd = optimal_assignment(pred[:, :n], target[:, :n], clamp=5.0)[1]
        return emd.mean().clamp(0.0, 10.0)
    cost = pairwise_dist(pred[:, :n], target[:, :n], 5.0).cpu().numpy()
    emd = torch.tensor([float(_assignment_mean(c)) for c in cost], dtype=torch.float32, device=pred.device)
    return emd.mean().clamp(0.0, 10.0)


# ----------------------------------------------------------------------------------------------------
# train_newloss.py:316-385
# ----------------------------------------------------------------------------------------------------
def distChamfer(a, b):
    """(dl, dr) of train_newloss.py:316-349: points clamped to +-1 and scaled to unit norm, nearest-neighbour distance
    floored at 1e-8, passed through log(d + 1e-8) clamped to [-10, 10] and exp (min and the monotone maps commute)."""
    through_log = lambda d: torch.log(d.clamp_min(1e-8) + 1e-8).clamp(-10, 10).exp().mean()
    return through_log(nn_dist(a, b, 1.0, unit_norm=True)), through_log(nn_dist(b, a, 1.0, unit_norm=True))


def emd_approx(x, y, assignment="host"):
    """Per-sample EMD of train_newloss.py:352-372 (clamp +-2, distances floored at 1e-8): tensor [B]. assignment="host"
    (the default) is scipy on the host, as in the reference; "device" is optimal_assignment on the GPU with the same
    clamp. There the floor of 1e-8 is applied to the matched per-row distances AFTER the assignment, where the reference
    floors the cost matrix BEFORE it: a floored matrix differs from the plain one by at most 1e-8 per entry, so the two
    means can differ only by that same 1e-8 per point (on top of the 2^-18 of the assignment itself)."""
    assert x.size(1) == y.size(1), "EMD only works if two point clouds are equal size"
    if _assignment_mode(assignment):
        idx = optimal_assignment(x, y, clamp=2.0)[0]
        xc, yc = _points(x, "x").clamp(-2.0, 2.0), _points(y, "y").clamp(-2.0, 2.0)
        matched = torch.gather(yc, 1, idx[:, :, None].expand(-1, -1, 3))
        return (xc - matched).square().sum(dim=-1).sqrt().clamp_min(1e-8).mean(dim=1).to(x)
    cost = np.maximum(pairwise_dist(x, y, 2.0).cpu().numpy(), 1e-8)
    return torch.from_numpy(np.stack([_assignment_mean(c) for c in cost]).reshape(-1)).to(x)


def robust_chamfer_distance(pred, gt):
    dl, dr = distChamfer(pred, gt)
    return (dl.mean() + dr.mean()) / 2


def robust_emd(pred, gt, assignment="host"):
    return emd_approx(pred, gt, assignment=assignment).mean()


# ----------------------------------------------------------------------------------------------------
# the optimal assignment itself on the GPU
# ----------------------------------------------------------------------------------------------------
ASSIGN_MAX_POINTS = 4096  # == NOVA_ASSIGN_MAX_POINTS of include/nova_hip.h
ASSIGN_QUANTUM = 2.0 ** -18  # the cost quantum of the integer scheme (include/nova_hip.h, nova_pointset_assignment)
# (row, column) cost evaluations of one bidding wave per launch. A bidding row visits its n columns 64 at a time at ~45 vector
# issues a visit; late in an auction one row bids per round, so a round is ~n / 64 x 45 issues of one latency-bound wave plus
# three barriers, ~2.5 ns per column: 2^22 visits are ~10 ms, and the few early rounds in which every row bids (n / 16 times
# the work, spread over 16 waves) bring a launch to a few tens. Sized from that instruction count, NOT yet from a measured
# round time: tools/assignment_bench.py writes profiles/assignment_bench.json, and this constant is to be re-derived from its
# longest single launch (optimal assignment)
_ASSIGN_COLUMN_VISITS_PER_LAUNCH = 1 << 22


def assignment_kernel_shape(n_points):
    """(workgroup size T, capacity NP) csrc/assign.hip runs a pair of `n_points`-point clouds with."""
    for limit, shape in ((64, (64, 64)), (256, (256, 256)), (1024, (256, 1024)), (2048, (512, 2048)), (ASSIGN_MAX_POINTS, (1024, 4096))):
        if n_points <= limit:
            return shape
    raise ValueError(f"the assignment kernel takes 1 .. {ASSIGN_MAX_POINTS} points per cloud, got {n_points}")


def _assignment_arguments(x, y, clamp, max_rounds, rounds_per_launch):
    """_check_clouds and the operation's own arguments. Returns (max_rounds, rounds_per_launch) with the defaults filled in."""
    _check_clouds(((x, "x"), (y, "y")), letters="B, n", count_range=("assignment", ASSIGN_MAX_POINTS), same_clouds=True,
                  same_points="the assignment")
    n = x.shape[1]
    _check_clamp(clamp)
    max_rounds = 64 * n + 1024 if max_rounds is None else _at_least_one(max_rounds, "max_rounds")
    rounds_per_launch = (max(16, _ASSIGN_COLUMN_VISITS_PER_LAUNCH // n) if rounds_per_launch is None
                         else _at_least_one(rounds_per_launch, "rounds_per_launch"))
    return max_rounds, rounds_per_launch


def optimal_assignment(x, y, clamp=None, max_rounds=None, rounds_per_launch=None, return_rounds=False):
    """The optimal assignment between the clouds x [B, n, 3] and y [B, n, 3] on the GPU, pair by pair (1 <= n <= 4096):
    (index int64 [B, n], cost float32 [B]) on the input's device. index[b] is the permutation that matches x[b, i] to
    y[b, index[b, i]] with the smallest mean Euclidean distance, cost[b] that mean in float32. `clamp` (None: off) clamps
    every coordinate to [-clamp, clamp] first, as pairwise_dist does. This is what scipy's linear_sum_assignment gives on
    the pairwise_dist matrix, up to the cost quantum: costs are rounded to multiples of ASSIGN_QUANTUM = 2^-18 and that
    integer problem is solved exactly (a Jacobi auction with epsilon scaling; the scheme is spelled out in
    include/nova_hip.h at nova_pointset_assignment, the kernel is csrc/assign.hip), so the mean is within 2^-18 of the
    optimal mean, and where several assignments are that close any of them may come back. The result depends on the pair
    alone: bitwise the same for every batch, every rounds_per_launch and every run.

    The auction runs in launches of `rounds_per_launch` bidding rounds (default: _ASSIGN_COLUMN_VISITS_PER_LAUNCH / n)
    until every pair is done. `max_rounds` (default 64 n + 1024, more than ten times what random clouds need) caps the
    rounds of a pair: when it is used up, NovaHipError names the unfinished pairs; the call never loops on. NovaHipError
    also for a pair whose clamped bounding box has a diagonal of 4096 or more (the integer range of the kernel).
    return_rounds=True adds a third result, int64 [B]: the bidding rounds every pair took."""
    max_rounds, per_launch = _assignment_arguments(x, y, clamp, max_rounds, rounds_per_launch)
    x, y = _points(x, "x"), _points(y, "y")
    B, n = x.shape[0], x.shape[1]
    idx = torch.empty(B, n, dtype=torch.int32, device=x.device)
    cost = torch.empty(B, dtype=torch.float32, device=x.device)
    rounds = torch.zeros(B, dtype=torch.int32, device=x.device)
    if B > 0:
        lo, hi = (-float(clamp), float(clamp)) if clamp is not None else (0.0, 0.0)
        with torch.cuda.device(x.device):
            stride = int(hip.load().nova_pointset_assignment_state_bytes(n))
            state = torch.empty(B * stride, dtype=torch.uint8, device=x.device)
            flag = torch.zeros(1, dtype=torch.int32, device=x.device)
            stream, left, restart = hip.stream_ptr(), max_rounds, 1
            while True:
                step = min(per_launch, left)
                hip.call("nova_pointset_assignment", x.data_ptr(), y.data_ptr(), idx.data_ptr(), cost.data_ptr(), state.data_ptr(),
                         B, n, lo, hi, 0 if clamp is None else 1, step, restart, flag.data_ptr(), stream)
                left, restart = left - step, 0
                status = int(flag)
                if status == 1:
                    break
                if status < 0:
                    bad = torch.nonzero(cost == -2.0).flatten().tolist()
                    raise hip.NovaHipError(f"optimal_assignment: pair(s) {bad} outside the kernel's integer range (bounding-box "
                                           "diagonal >= 4096 or a bid >= 2^49); scale the clouds down")
                if left == 0:
                    bad = torch.nonzero(cost < 0).flatten().tolist()
                    raise hip.NovaHipError(f"optimal_assignment: pair(s) {bad} not finished after max_rounds = {max_rounds} bidding rounds")
            if return_rounds:
                hip.call("nova_pointset_assignment_rounds", state.data_ptr(), rounds.data_ptr(), B, n, stream)
    return (idx.long(), cost, rounds.long()) if return_rounds else (idx.long(), cost)


# ----------------------------------------------------------------------------------------------------
# set-level metrics: MMD, COV and 1-NNA under the Chamfer distance
# ----------------------------------------------------------------------------------------------------
METRIC_KEYS = ("lgan_mmd-CD", "lgan_mmd_smp-CD", "lgan_cov-CD", "1-NN-CD-acc", "1-NN-CD-acc_t", "1-NN-CD-acc_f")
_DISTANCES_PER_LAUNCH = 1 << 37  # ~1.4e11 squared distances: tens of milliseconds per launch (profiles/chamfer_matrix_*)
EMD_METRIC_KEYS = ("lgan_mmd-EMD", "lgan_mmd_smp-EMD", "lgan_cov-EMD", "1-NN-EMD-acc", "1-NN-EMD-acc_t", "1-NN-EMD-acc_f")
EMD_MAX_POINTS = 4096  # == NOVA_EMD_MAX_POINTS of include/nova_hip.h
_EMD_EVALUATIONS_PER_LAUNCH = 1 << 36  # (k, l, level) evaluations, ~6.9e10: tens of milliseconds per launch (profiles/emd_matrix_*)


def chamfer_matrix(x, y=None, max_pairs_per_launch=None):
    """cd[a, b] = CD(x[a], y[b]) for clouds x [A, N, 3] and y [B, M, 3] on the GPU: float32 [A, B] on x's device, with

        CD(X, Y) = mean_{p in X} min_{q in Y} |p - q|^2 + mean_{q in Y} min_{p in X} |p - q|^2

    in squared Euclidean distances, no clamp and no normalisation (the convention of PointFlow and its successors; not
    the density-weighted compute_chamfer_distance). y=None is x against itself: only the pairs a <= b are computed and
    the result is exactly symmetric. The pair grid is split into launches of at most `max_pairs_per_launch` cloud pairs
    (default: ~1.4e11 squared distances each); every entry is bitwise the same whatever the split."""
    sym = y is None
    x, y = _clouds([(x, "x")]) * 2 if sym else _clouds([(x, "x"), (y, "y")])
    A, N, B, M = x.shape[0], x.shape[1], y.shape[0], y.shape[1]
    cd = torch.empty(A, B, dtype=torch.float32, device=x.device)
    if A == 0 or B == 0:
        return cd
    if N == 0 or M == 0:
        raise ValueError(f"chamfer_matrix: empty clouds ({N} and {M} points)")
    pairs = max_pairs_per_launch if max_pairs_per_launch is not None else max(1, _DISTANCES_PER_LAUNCH // (N * M))
    if pairs < 1:
        raise ValueError(f"max_pairs_per_launch must be >= 1, got {pairs}")
    bs = max(1, math.isqrt(pairs))  # square blocks; a diagonal block holds bs (bs + 1) / 2 <= pairs pairs
    with torch.cuda.device(x.device):
        st = hip.stream_ptr()

        def launch(a0, a1, b0, b1, symmetric):
            hip.call("nova_pointset_chamfer_matrix", x[a0].data_ptr(), y[b0].data_ptr(), cd[a0, b0:].data_ptr(), a1 - a0, b1 - b0,
                     N, M, B, 1 if symmetric else 0, st)

        if sym:
            for a0 in range(0, A, bs):
                a1 = min(A, a0 + bs)
                launch(a0, a1, a0, a1, True)
                for b0 in range(a1, A, bs):
                    b1 = min(A, b0 + bs)
                    launch(a0, a1, b0, b1, False)
                    cd[b0:b1, a0:a1] = cd[a0:a1, b0:b1].t()
        else:
            bb = min(B, max(bs, pairs // min(A, bs)))  # wide blocks when A is short
            ba = min(A, max(1, pairs // bb))
            for a0 in range(0, A, ba):
                for b0 in range(0, B, bb):
                    launch(a0, min(A, a0 + ba), b0, min(B, b0 + bb), False)
    return cd


def _emd_resident_workgroups(device, N):
    """Workgroups of emd_matrix_kernel resident at once on the device: CUs x what LDS allows per CU (csrc/emd.hip keeps
    36 B per point of capacity - 256, 512, 1024, 2048 or 4096 points - in LDS; the registers allow the same or more)."""
    capacity = next(c for c in (256, 512, 1024, 2048, 4096) if N <= c)
    waves = 8 if capacity == 4096 else 4
    per_cu = max(1, min((160 * 1024) // (36 * capacity + 64), 32 // waves))
    return torch.cuda.get_device_properties(device).multi_processor_count * per_cu


def emd_matrix(x, y=None, max_pairs_per_launch=None):
    """emd[a, b] = EMD(x[a], y[b]) for clouds x [A, N, 3] and y [B, N, 3] on the GPU: float32 [A, B] on x's device. The
    EMD is approxmatch followed by its match cost, divided by n (PointFlow's emd_approx; the algorithm is spelled out
    in include/nova_hip.h at nova_pointset_emd_matrix), on squared Euclidean distances with no clamp and no
    normalisation. It is NOT symmetric: x[a] is the first cloud. It is translation-invariant but not scale-invariant, so
    normalise the points the way the compared work does. Both sets need the same point count N, 1 <= N <= 4096.

    y=None is x against itself: the full matrix is computed (not mirrored). The pair grid is split into launches of at
    most `max_pairs_per_launch` cloud pairs (default: ~6.9e10 (k, l, level) evaluations each, in whole rounds of the
    resident workgroups); every entry is bitwise the same whatever the split."""
    emd_checks = dict(count_range=("EMD", EMD_MAX_POINTS), same_points="the EMD")
    x, y = _clouds([(x, "x")], **emd_checks) * 2 if y is None else _clouds([(x, "x"), (y, "y")], **emd_checks)
    A, N, B = x.shape[0], x.shape[1], y.shape[0]
    emd = torch.empty(A, B, dtype=torch.float32, device=x.device)
    if A == 0 or B == 0:
        return emd
    if max_pairs_per_launch is None:
        res = _emd_resident_workgroups(x.device, N)
        pairs = max(1, _EMD_EVALUATIONS_PER_LAUNCH // (N * N * 10) // res) * res
    else:
        pairs = max_pairs_per_launch
        if pairs < 1:
            raise ValueError(f"max_pairs_per_launch must be >= 1, got {pairs}")
        res = pairs
    bb = min(B, res, pairs)  # column blocks of a round's width; rows fill the launch
    with torch.cuda.device(x.device):
        st = hip.stream_ptr()
        for b0 in range(0, B, bb):
            b1 = min(B, b0 + bb)
            ba = max(1, pairs // (b1 - b0))
            for a0 in range(0, A, ba):
                a1 = min(A, a0 + ba)
                hip.call("nova_pointset_emd_matrix", x[a0].data_ptr(), y[b0].data_ptr(), emd[a0, b0:].data_ptr(), a1 - a0,
                         b1 - b0, N, B, st)
    return emd


def _first_argmin(d, dim):
    """Index of the minimum along `dim`, ties to the lowest index (spelled out rather than relying on a backend)."""
    m = d.min(dim=dim, keepdim=True).values
    idx = torch.arange(d.shape[dim], device=d.device).view([-1 if k == dim else 1 for k in range(d.dim())])
    return torch.where(d == m, idx, d.shape[dim]).min(dim=dim).values


def distribution_metrics_from_matrices(d_rs, d_rr, d_ss, distance="CD"):
    """The six set-level metrics from the Chamfer matrices of a reference set R (S_r clouds) and a sample set Sm (S_s):
    d_rs [S_r, S_s] = CD(R_r, Sm_s), d_rr [S_r, S_r], d_ss [S_s, S_s]. Pure tensor logic (CPU or GPU); 0-dim float64
    tensors on d_rs's device, keyed as PointFlow's evaluation code keys them:

        lgan_mmd-CD      mean_r min_s d_rs[r, s]
        lgan_mmd_smp-CD  mean_s min_r d_rs[r, s]
        lgan_cov-CD      |{argmin_r d_rs[r, s] : s}| / S_r            (argmin ties to the lowest r)
        1-NN-CD-acc      1-NN classifier accuracy on the pooled set [R; Sm] with the matrix [[d_rr, d_rs], [d_rs^T, d_ss]]:
                         each element's nearest other element (diagonal excluded, ties to the lowest pooled index) is
                         correct when it carries the same label; the fraction over all elements
        1-NN-CD-acc_t    the same fraction over the references only
        1-NN-CD-acc_f    the same fraction over the samples only

    `distance` sets only the key suffix ("CD" or "EMD"). For an asymmetric distance pass the matrices oriented as the
    row rule above needs them (compute_all_metrics(..., emd=True) shows how)."""
    if distance not in ("CD", "EMD"):
        raise ValueError(f"distance must be 'CD' or 'EMD', got {distance!r}")
    S_r, S_s = d_rs.shape
    if tuple(d_rr.shape) != (S_r, S_r) or tuple(d_ss.shape) != (S_s, S_s) or S_r == 0 or S_s == 0:
        raise ValueError(f"matrix shapes {tuple(d_rs.shape)}, {tuple(d_rr.shape)}, {tuple(d_ss.shape)} do not form a pooled matrix")
    d_rs, d_rr, d_ss = d_rs.double(), d_rr.to(d_rs.device).double(), d_ss.to(d_rs.device).double()
    out = {f"lgan_mmd-{distance}": d_rs.min(dim=1).values.mean(), f"lgan_mmd_smp-{distance}": d_rs.min(dim=0).values.mean()}
    # the fractions are integer counts divided once in float64 on the host (a device mean may multiply by 1 / n)
    frac = lambda count, total: torch.tensor(int(count) / total, dtype=torch.float64, device=d_rs.device)
    out[f"lgan_cov-{distance}"] = frac(torch.unique(_first_argmin(d_rs, 0)).numel(), S_r)
    pooled = torch.cat([torch.cat([d_rr, d_rs], 1), torch.cat([d_rs.t(), d_ss], 1)], 0)
    pooled.fill_diagonal_(float("inf"))
    is_ref = torch.arange(S_r + S_s, device=d_rs.device) < S_r
    correct = is_ref[_first_argmin(pooled, 1)] == is_ref
    n_t, n_f = int(correct[:S_r].sum()), int(correct[S_r:].sum())
    nn = f"1-NN-{distance}-acc"
    out[nn], out[nn + "_t"], out[nn + "_f"] = frac(n_t + n_f, S_r + S_s), frac(n_t, S_r), frac(n_f, S_s)
    return out


def compute_all_metrics(sample_pcs, ref_pcs, batch_size=None, emd=False, jsd=False, jsd_resolution=28):
    """MMD, COV and 1-NNA under the Chamfer distance (see distribution_metrics_from_matrices) of the generated clouds
    sample_pcs [S_s, N, 3] against the reference clouds ref_pcs [S_r, M, 3], both GPU tensors. `batch_size` caps the
    cloud pairs per kernel launch (chamfer_matrix's and emd_matrix's max_pairs_per_launch). emd=True adds the same six
    metrics under the EMD (emd_matrix; needs N == M <= 4096), keyed `-EMD`. jsd=True adds "jsd"
    (jsd_between_point_cloud_sets at `jsd_resolution`; expects the clouds in the ball of radius 0.5) and
    "jsd_outside_fraction", the larger of the two sets' shares of points outside the grid. Returns a dict of Python floats."""
    if jsd:
        _check_resolution(jsd_resolution, True)
    emd_checks = dict(count_range=("EMD", EMD_MAX_POINTS), same_points="the EMD") if emd else {}
    smp, ref = _clouds([(sample_pcs, "sample_pcs"), (ref_pcs, "ref_pcs")], **emd_checks)
    if smp.shape[0] == 0 or ref.shape[0] == 0:
        raise ValueError("compute_all_metrics: empty set")
    d_rs = chamfer_matrix(ref, smp, batch_size)
    d_rr = chamfer_matrix(ref, None, batch_size)
    d_ss = chamfer_matrix(smp, None, batch_size)
    out = {k: float(v) for k, v in distribution_metrics_from_matrices(d_rs, d_rr, d_ss).items()}
    if emd:
        m_rs = emd_matrix(ref, smp, batch_size)
        m_rr = emd_matrix(ref, None, batch_size)
        m_ss = emd_matrix(smp, None, batch_size)
        # PointFlow's 1-NN classifier takes each element's nearest neighbour along dim 0 of its pooled matrix
        # [[M_rr, M_rs], [M_rs^T, M_ss]] (element j is the second argument of the EMD). The pooled matrix of the
        # transposed blocks is the transpose of that one, so the row rule of distribution_metrics_from_matrices on
        # (M_rs, M_rr^T, M_ss^T) is PointFlow's rule; MMD and COV use M_rs as it stands, as PointFlow does.
        out.update({k: float(v) for k, v in distribution_metrics_from_matrices(m_rs, m_rr.t(), m_ss.t(), distance="EMD").items()})
    if jsd:
        o_s, o_r = occupancy_grid(smp, jsd_resolution, True), occupancy_grid(ref, jsd_resolution, True)
        out["jsd"] = float(jensen_shannon_divergence(o_s["counters"], o_r["counters"]))
        out["jsd_outside_fraction"] = max(o_s["outside"] / (smp.shape[0] * smp.shape[1]), o_r["outside"] / (ref.shape[0] * ref.shape[1]))
    return out


# ----------------------------------------------------------------------------------------------------
# JSD between the occupancy distributions of two sets
# ----------------------------------------------------------------------------------------------------
OCC_MAX_RESOLUTION = 32  # == NOVA_OCC_MAX_RES of include/nova_hip.h
_OCC_POINTS_PER_LAUNCH = 1 << 24  # ~1.7e7 points: 10 ms per launch when every point takes the slow path over the whole grid (profiles/occupancy_grid_*)


def _check_resolution(resolution, in_sphere):
    if not isinstance(resolution, int) or isinstance(resolution, bool) or not 2 <= resolution <= OCC_MAX_RESOLUTION:
        raise ValueError(f"resolution must be an integer in 2 .. {OCC_MAX_RESOLUTION}, got {resolution!r}")
    if in_sphere and resolution == 2:
        raise ValueError("resolution 2 has no node inside the ball of radius 0.5 (in_sphere)")


def grid_node_mask(resolution=28, in_sphere=True):
    """bool [R^3] (CPU): which lattice nodes c(i, j, k) = (i, j, k) / (R - 1) - 0.5, flat index (i R + j) R + k, belong to
    the grid. in_sphere keeps |c| <= 0.5, decided in integers: (2i-(R-1))^2 + (2j-(R-1))^2 + (2k-(R-1))^2 <= (R-1)^2
    (10144 nodes at R = 28; include/nova_hip.h, nova_pointset_occupancy_grid)."""
    _check_resolution(resolution, in_sphere)
    R = resolution
    if not in_sphere:
        return torch.ones(R ** 3, dtype=torch.bool)
    t2 = (2 * torch.arange(R, dtype=torch.int64) - (R - 1)) ** 2
    return ((t2[:, None, None] + t2[None, :, None] + t2[None, None, :]) <= (R - 1) ** 2).reshape(-1)


def occupancy_grid(pclouds, resolution=28, in_sphere=True, return_nodes=False, max_clouds_per_launch=None, workgroups=0):
    """Occupancy of the R^3 lattice over [-0.5, 0.5]^3 (in_sphere: of its nodes inside the ball of radius 0.5) by the
    clouds pclouds [S, N, 3] on the GPU: every point goes to its nearest grid node (a point outside the ball or cube
    too). Returns a dict with

        counters   int64 [R^3] on the input's device: points per node over all clouds (flat index (i R + j) R + k)
        bernoulli  int64 [R^3]: clouds with at least one point on the node
        outside    int: points whose own cell (the per-axis rounded node) is not a grid node, i.e. outside the ball or cube
        nodes      int32 [S, N], each point's node (only with return_nodes=True)

    The definition, the tie rule and the float32 expressions are in include/nova_hip.h at nova_pointset_occupancy_grid.
    The grid is fixed in space: normalise the clouds first (normalize_clouds). All results are integers and are the same
    for every split: the set goes out in launches of at most `max_clouds_per_launch` clouds (default:
    _OCC_POINTS_PER_LAUNCH points each), and `workgroups` (0 = automatic) sets the kernel's grid size."""
    _check_resolution(resolution, in_sphere)
    (x,) = _clouds([(pclouds, "pclouds")])
    S, N, R = x.shape[0], x.shape[1], resolution
    counters = torch.zeros(R ** 3, dtype=torch.int64, device=x.device)
    bernoulli = torch.zeros_like(counters)
    outside = torch.zeros(1, dtype=torch.int64, device=x.device)
    nodes = torch.empty(S, N, dtype=torch.int32, device=x.device) if return_nodes else None
    if S > 0:
        if N == 0:
            raise ValueError("occupancy_grid: empty clouds (0 points)")
        per = max_clouds_per_launch if max_clouds_per_launch is not None else max(1, _OCC_POINTS_PER_LAUNCH // N)
        for stream, s0, count in _launching(x.device, S, per):
            hip.call("nova_pointset_occupancy_grid", _at(x, s0), counters.data_ptr(), bernoulli.data_ptr(), _at(nodes, s0), outside.data_ptr(),
                     count, N, R, 1 if in_sphere else 0, int(workgroups), stream)
    out = {"counters": counters, "bernoulli": bernoulli, "outside": int(outside)}
    if return_nodes:
        out["nodes"] = nodes
    return out


def entropy_of_occupancy_grid(pclouds, grid_resolution=28, in_sphere=True):
    """(acc_entropy, counters) of PointFlow's entropy_of_occupancy_grid, restated from the published algorithm (parity
    unpinned by execution): counters int64 [R^3] as occupancy_grid returns them, and acc_entropy (float) the sum over
    the nodes with bernoulli > 0 of the entropy H([p, 1 - p]) (natural log, p = bernoulli / S), divided by the number of
    grid nodes. Odd resolutions with in_sphere may differ from PointFlow's grid on boundary nodes (its membership test is
    a float32 norm; ours is the integer rule of grid_node_mask); even ones, the default 28 among them, do not."""
    occ = occupancy_grid(pclouds, grid_resolution, in_sphere)
    S = pclouds.shape[0]
    if S == 0:
        raise ValueError("entropy_of_occupancy_grid: empty set")
    p = occ["bernoulli"].double() / S
    p = p[p > 0]
    h = -(torch.xlogy(p, p) + torch.xlogy(1 - p, 1 - p)).sum()
    return float(h) / int(grid_node_mask(grid_resolution, in_sphere).sum()), occ["counters"]


def _entropy_base2(p):
    return -torch.xlogy(p, p).sum() / math.log(2.0)


def jensen_shannon_divergence(P, Q):
    """JSD(P, Q) = H2((P' + Q') / 2) - (H2(P') + H2(Q')) / 2 of two histograms of equal size, P' = P / sum P,
    Q' = Q / sum Q, H2 the base-2 entropy with 0 log 0 = 0 (PointFlow's jensen_shannon_divergence). Pure tensor logic in
    float64, CPU or GPU: a 0-dim float64 tensor in [0, 1] on P's device. ValueError for negative values, unequal sizes or an
    all-zero histogram."""
    P, Q = torch.as_tensor(P), torch.as_tensor(Q)
    if P.numel() != Q.numel():
        raise ValueError(f"histograms of unequal size ({P.numel()} and {Q.numel()})")
    P, Q = P.reshape(-1).double(), Q.to(P.device).reshape(-1).double()
    if bool((P < 0).any()) or bool((Q < 0).any()):
        raise ValueError("negative values")
    if not (float(P.sum()) > 0 and float(Q.sum()) > 0):
        raise ValueError("all-zero histogram")
    P_, Q_ = P / P.sum(), Q / Q.sum()
    res = _entropy_base2((P_ + Q_) / 2) - (_entropy_base2(P_) + _entropy_base2(Q_)) / 2
    return res.clamp(0.0, 1.0)


def jsd_between_point_cloud_sets(sample_pcs, ref_pcs, resolution=28):
    """JSD between the occupancy distributions (the counters of the in-sphere grid at `resolution`) of the generated
    clouds and the reference clouds, both [S, n, 3] GPU tensors expected in the ball of radius 0.5 (normalize_clouds):
    PointFlow's jsd_between_point_cloud_sets, restated from the published algorithm (parity unpinned by execution).
    Returns a Python float in [0, 1]."""
    smp = occupancy_grid(sample_pcs, resolution, True)
    ref = occupancy_grid(ref_pcs, resolution, True)
    return float(jensen_shannon_divergence(smp["counters"], ref["counters"]))


# ----------------------------------------------------------------------------------------------------
# farthest point sampling: sets of different density to a common point count
# ----------------------------------------------------------------------------------------------------
FPS_MAX_POINTS = 16384  # == NOVA_FPS_MAX_POINTS of include/nova_hip.h
RESAMPLE_METHODS = ("fps", "first", "random")
# distance updates (clouds x points x samples) per launch, ~6.9e10. Sized from the kernel's instruction count (7 vector issues
# per update: ~4e12 updates/s on 256 compute units, so ~17 ms per launch), NOT yet from a measured step time: tools/fps_bench.py
# writes profiles/fps_bench.json, and this constant is to be re-derived from it (farthest point sampling)
_FPS_POINT_STEPS_PER_LAUNCH = 1 << 36


def fps_kernel_shape(n_points):
    """(points per thread P, workgroup size T) csrc/fps.hip runs a cloud of `n_points` points with (fps_config there)."""
    for limit, shape in ((64, (1, 64)), (128, (2, 64)), (256, (1, 256)), (512, (2, 256)), (1024, (4, 256)), (2048, (8, 256)),
                         (4096, (16, 256)), (8192, (16, 512)), (FPS_MAX_POINTS, (16, 1024))):
        if n_points <= limit:
            return shape
    raise ValueError(f"the FPS kernel takes 1 .. {FPS_MAX_POINTS} points per cloud, got {n_points}")


def _fps_arguments(points, n_samples, start):
    """_check_clouds and the operation's own arguments. Returns `start` as None (index 0 everywhere) or an int64 CPU tensor [S]."""
    _check_clouds([(points, "points")], letters="S, N", count_range=("FPS", FPS_MAX_POINTS))
    S, N = points.shape[0], points.shape[1]
    if not isinstance(n_samples, int) or isinstance(n_samples, bool) or not 1 <= n_samples <= N:
        raise ValueError(f"n_samples must be an integer in 1 .. {N} (the point count), got {n_samples!r}")
    if isinstance(start, int) and not isinstance(start, bool):
        if not 0 <= start < N:
            raise ValueError(f"start must be in 0 .. {N - 1}, got {start}")
        st = None if start == 0 else torch.full((S,), start, dtype=torch.int64)
    else:
        st = torch.as_tensor(start).detach().cpu()
        if st.dtype.is_floating_point or st.dtype.is_complex or st.dtype == torch.bool or tuple(st.shape) != (S,):
            raise ValueError(f"start: expected an int or {S} integer indices (one per cloud), got {tuple(st.shape)} {st.dtype}")
        st = st.long()
        if S > 0 and not (0 <= int(st.min()) and int(st.max()) < N):
            raise ValueError(f"start must be in 0 .. {N - 1}, got values in {int(st.min())} .. {int(st.max())}")
    return st


def farthest_point_sample(points, n_samples, start=0, return_distances=False, max_clouds_per_launch=None):
    """Farthest point sampling of the clouds points [S, N, 3] on the GPU (1 <= N <= 16384): int64 [S, n_samples] indices on
    the input's device, row s the points of cloud s in the order they were chosen, starting at `start` (an int, or one
    index per cloud as an int tensor or sequence [S]); each further one is the point farthest from all chosen so far,
    lowest index on ties. With return_distances also float32 [S, n_samples]: the squared distance of each chosen point to
    the ones before it (+inf for the first; non-increasing after it). The algorithm and its float32 distance are spelled
    out in include/nova_hip.h at nova_pointset_farthest_point_sample (csrc/fps.hip).

    The set goes out in launches of at most `max_clouds_per_launch` clouds (default: _FPS_POINT_STEPS_PER_LAUNCH distance
    updates each); a cloud's result depends on the cloud and its start only and is bitwise the same for every split."""
    st = _fps_arguments(points, n_samples, start)
    x = _points(points, "points")
    S, N, n = x.shape[0], x.shape[1], n_samples
    per = max_clouds_per_launch if max_clouds_per_launch is not None else max(1, _FPS_POINT_STEPS_PER_LAUNCH // (N * n))
    launches = _launching(x.device, S, per)
    idx = torch.empty(S, n, dtype=torch.int32, device=x.device)
    dist = torch.empty(S, n, dtype=torch.float32, device=x.device) if return_distances else None
    st = st.to(device=x.device, dtype=torch.int32) if st is not None else None
    for stream, s0, count in launches:
        hip.call("nova_pointset_farthest_point_sample", _at(x, s0), st[s0:].data_ptr() if st is not None else None, _at(idx, s0), _at(dist, s0),
                 count, N, n, stream)
    return (idx.long(), dist) if return_distances else idx.long()


def resample_clouds(points, n_points, method="fps", start=0, generator=None):
    """points [S, N, 3] cut to [S, n_points, 3]:
        "fps"     the farthest_point_sample points, in the order chosen (GPU only; `start` as there)
        "first"   points[:, :n_points]
        "random"  a uniformly random subset without repetition: the first n_points of one torch.randperm(N) per cloud,
                  drawn from `generator` (a CPU generator, or None for the global one)
    "first" and "random" are pure torch and work on CPU tensors too. n_points == N returns the input itself; more points
    than the clouds have is a ValueError."""
    if method not in RESAMPLE_METHODS:
        raise ValueError(f"method must be one of {RESAMPLE_METHODS}, got {method!r}")
    _check_clouds([(points, "points")], letters="S, N", finite=False)
    S, N = points.shape[0], points.shape[1]
    _at_least_one(n_points, "n_points")
    if n_points > N:
        raise ValueError(f"cannot resample clouds of {N} points to {n_points}: resampling only removes points")
    if n_points == N:
        return points
    if method == "first":
        return points[:, :n_points]
    if method == "random":
        idx = torch.stack([torch.randperm(N, generator=generator)[:n_points] for _ in range(S)]) if S else torch.empty(0, n_points, dtype=torch.int64)
        idx = idx.to(points.device)
    else:
        idx = farthest_point_sample(points, n_points, start=start)
    return torch.gather(points, 1, idx[:, :, None].expand(S, n_points, 3))


# ----------------------------------------------------------------------------------------------------
# k nearest neighbours and local density
# ----------------------------------------------------------------------------------------------------
KNN_MAX_K = 32  # == NOVA_KNN_MAX_K of include/nova_hip.h
KNN_MAX_POINTS = 65536  # == NOVA_KNN_MAX_POINTS of include/nova_hip.h
# candidate evaluations (clouds x queries x targets) per launch, ~1.7e10. Sized from the kernel's instruction count (about 10
# vector issues per candidate plus 40 per insertion at k = 8: ~4e12 candidates/s on 256 compute units, so ~4 ms per launch;
# at k = 32 nearly every candidate costs a 160-issue insertion, ~5e11/s and ~35 ms), NOT yet from a measured time:
# tools/knn_bench.py writes profiles/knn_bench.json, and this constant is to be re-derived from the longest launch it
# records (k nearest neighbours). A cloud is at most 2^32 candidates, so a launch holds at least four.
_KNN_CANDIDATES_PER_LAUNCH = 1 << 34
_KNN_SPLIT_BELOW = 512  # == KNN_SPLIT_BELOW of csrc/knn.hip


def knn_kernel_shape(n_clouds, n_queries, k):
    """(list rung K, queries per workgroup) csrc/knn.hip runs one launch of `n_clouds` clouds of `n_queries` query points at
    `k` neighbours with (the rung ladder and knn_split there): 256 queries per workgroup, or 64 with the four waves
    sharing the candidates when the launch would have fewer than 512 workgroups."""
    if not 1 <= k <= KNN_MAX_K:
        raise ValueError(f"the kNN kernel takes k in 1 .. {KNN_MAX_K}, got {k}")
    rung = next(r for r in (1, 2, 4, 8, 16, 32) if k <= r)
    return rung, 64 if n_clouds * ((n_queries + 255) // 256) < _KNN_SPLIT_BELOW else 256


def _knn_arguments(x, y, k, exclude_self):
    """_check_clouds and the operation's own arguments. Returns exclude_self resolved to a bool."""
    _check_clouds([(x, "x")] + ([(y, "y")] if y is not None else []), letters="S, N", count_range=("kNN", KNN_MAX_POINTS),
                  same_clouds=True)
    N, M = x.shape[1], (x if y is None else y).shape[1]
    if exclude_self is None:
        exclude_self = y is None
    if not isinstance(exclude_self, bool):
        raise ValueError(f"exclude_self must be a bool or None, got {exclude_self!r}")
    if exclude_self and N != M:
        raise ValueError(f"exclude_self needs equal point counts (query i is target i), got N = {N} and M = {M}")
    k_max = min(KNN_MAX_K, M - (1 if exclude_self else 0))
    if not isinstance(k, int) or isinstance(k, bool) or not 1 <= k <= k_max:
        raise ValueError(f"k must be an integer in 1 .. {k_max} (at most {KNN_MAX_K}, and {M} target points"
                         f"{' without the point itself' if exclude_self else ''}), got {k!r}")
    return exclude_self


def knn_points(x, y=None, k=8, exclude_self=None, return_distances=True, max_clouds_per_launch=None):
    """The exact k nearest neighbours in y [S, M, 3] of every point of x [S, N, 3], cloud by cloud, on the GPU
    (1 <= N, M <= 65536, 1 <= k <= 32): (idx int64 [S, N, k], d2 float32 [S, N, k]) on the input's device, or idx alone
    with return_distances=False. Row (s, i) lists the k targets j with the smallest keys (d2, j) in ascending order, d2 the
    float32 squared distance in exact differences; a distance tie goes to the lowest index, inside the list and at its
    cut-off. No [N, M] matrix is stored. The definition is spelled out in include/nova_hip.h at nova_pointset_knn
    (csrc/knn.hip).

    y=None is the self-query: the targets are x itself, and exclude_self (default True there) skips the query point by its
    index, so k <= N - 1; a duplicate of the point elsewhere in the cloud still comes back, at distance 0. With y given,
    exclude_self defaults to False; True needs N == M (query i is target i).

    The set goes out in launches of at most `max_clouds_per_launch` clouds (default: _KNN_CANDIDATES_PER_LAUNCH candidate
    evaluations each); a cloud's result depends on (x[s], y[s], k, exclude_self) alone and is bitwise the same for every
    split."""
    exclude_self = _knn_arguments(x, y, k, exclude_self)
    xs = _points(x, "x")
    ys = xs if y is None else _points(y, "y")
    S, N, M = xs.shape[0], xs.shape[1], ys.shape[1]
    per = max_clouds_per_launch if max_clouds_per_launch is not None else max(1, _KNN_CANDIDATES_PER_LAUNCH // (N * M))
    launches = _launching(xs.device, S, per)
    idx = torch.empty(S, N, k, dtype=torch.int32, device=xs.device)
    d2 = torch.empty(S, N, k, dtype=torch.float32, device=xs.device) if return_distances else None
    for stream, s0, count in launches:
        hip.call("nova_pointset_knn", _at(xs, s0), _at(ys, s0), _at(idx, s0), _at(d2, s0), count, N, M, k, 1 if exclude_self else 0, stream)
    return (idx.long(), d2) if return_distances else idx.long()


def local_density(points, k_neighbors=8):
    """float32 [S, N]: for every point of points [S, N, 3], the mean Euclidean distance to its k_neighbors nearest other
    points (small where the cloud is dense). The reference's compute_local_density (transformer_pointcloud_nova.py:81-89),
    which takes k_neighbors + 1 columns of torch.cdist and drops the first as the point itself; here the point is excluded
    by index (knn_points), so the distances are the same multiset and a duplicate of the point counts at distance 0."""
    _, d2 = knn_points(points, k=k_neighbors)
    return d2.sqrt().mean(dim=-1)


# ----------------------------------------------------------------------------------------------------
# distance-weighted interpolation and adaptive sampling
# ----------------------------------------------------------------------------------------------------
def kernel_interpolate(queries, points, values=None, temperature=1.0, max_clouds_per_launch=None):
    """Distance-weighted interpolation on the GPU: float32 [S, T, C] on the input's device, row (s, i) the average of
    values[s] [N, C] over ALL source points points[s] [N, 3], weighted by softmax_j(-|queries[s, i] - points[s, j]| /
    temperature) (1 <= T, N <= 65536, 1 <= C <= 8). values=None means the source points themselves (C = 3), which is the
    sum of the reference's feature_aware_interpolation (transformer_pointcloud_nova.py:149-150) without its [T, N] matrix
    and its [S, T, N, 3] product. The point itself is not excluded; the nearest distance is subtracted before the
    exponential, so far queries are served like near ones. temperature=inf is the plain mean. The definition and its
    order of summation are spelled out in include/nova_hip.h at nova_pointset_kernel_interpolate (csrc/interp.hip).

    ValueError for a temperature that is not a real number > 0 or so small that log2(e) / temperature is not finite in
    float32, and for values that are not floating point, not finite or not [S, N, 1 .. 8] on the points' device.

    The set goes out in launches of at most `max_clouds_per_launch` clouds (default: _INTERP_PAIRS_PER_LAUNCH (query,
    source) pairs each); a cloud's result depends on (queries[s], points[s], values[s], temperature) alone and is bitwise
    the same for every split. values=None is bitwise what values=points.clone() gives."""
    C = _interp_arguments(queries, points, values)
    scale = _interp_scale(temperature)
    qs = _points(queries, "queries")
    ps = qs if points is queries else _points(points, "points")
    vs = None
    if values is not None:
        if not values.is_cuda:
            raise hip.NovaHipError("values: point-set metrics run on the GPU (got a CPU tensor)")
        if values.requires_grad and torch.is_grad_enabled():
            raise hip.NovaHipError("values: nova_pointcloud_amd.metrics is evaluation-only (no autograd through the HIP kernels); detach the values")
        vs = values.detach().float().contiguous()
    S, T, N = qs.shape[0], qs.shape[1], ps.shape[1]
    per = max_clouds_per_launch if max_clouds_per_launch is not None else max(1, _INTERP_PAIRS_PER_LAUNCH // (T * N))
    launches = _launching(qs.device, S, per)
    out = torch.empty(S, T, C, dtype=torch.float32, device=qs.device)
    for stream, s0, count in launches:
        hip.call("nova_pointset_kernel_interpolate", _at(qs, s0), _at(ps, s0), _at(vs, s0), _at(out, s0), count, T, N, C, scale, stream)
    return out


def feature_aware_interpolation(points, target_size, temperature=1.0, generator=None):
    """The reference's feature_aware_interpolation (transformer_pointcloud_nova.py:128-152): points [S, N, 3] thinned to
    [S, target_size, 3] without dropping a point's contribution. With N <= target_size the points are repeated cyclically
    and cut to target_size (pure torch; works on CPU tensors). Otherwise target_size of the points are picked by one
    torch.randperm(N, generator=generator) shared by all clouds (a CPU generator, or None for the global one), as in the
    reference, and each becomes kernel_interpolate's softmax(-distance / temperature) average of ALL N points (GPU only;
    float32). The reference's temperature is 1; its topk(8) is dead code and is not reproduced."""
    return _feature_aware_interpolation(kernel_interpolate, points, target_size, temperature, generator)


def adaptive_sampling(subset, target_size, temperature=1.0, generator=None):
    """The reference's adaptive_sampling (transformer_pointcloud_nova.py:92-97): subset [S, N, 3] brought to
    [S, target_size, 3]. N == target_size returns the input itself; N > target_size (a dense subset) returns
    feature_aware_interpolation(subset, target_size, temperature, generator); N < target_size (a sparse one) returns the
    points in farthest-point order (farthest_point_sample(subset, N)), repeated cyclically to target_size, so every prefix
    of the result stays well spread (GPU only).
    DEVIATION, on purpose: the reference sends the sparse case to its farthest_point_sampling with more samples than
    points, which that body cannot deliver (include/nova_hip.h, nova_pointset_kernel_interpolate)."""
    return _adaptive_sampling(kernel_interpolate, farthest_point_sample, subset, target_size, temperature, generator)


NORMALIZE_MODES = ("none", "unit_sphere", "unit_cube")


def normalize_clouds(points, mode):
    """Per-cloud normalisation of points [..., n, 3] (pure torch, CPU or GPU) into the region the occupancy grid covers:
        "unit_sphere"  subtract the centre of the bounding box, divide by twice the largest remaining norm: |p| <= 0.5
        "unit_cube"    subtract the same centre, divide by the longest box side: every coordinate in [-0.5, 0.5]
        "none"         the input itself
    A degenerate cloud (all points equal) maps to the origin."""
    if mode not in NORMALIZE_MODES:
        raise ValueError(f"mode must be one of {NORMALIZE_MODES}, got {mode!r}")
    if mode == "none":
        return points
    if points.dim() < 2 or points.shape[-1] != 3 or points.shape[-2] == 0:
        raise ValueError(f"expected [..., n, 3] points with n >= 1, got {tuple(points.shape)}")
    hi, lo = points.max(dim=-2, keepdim=True).values, points.min(dim=-2, keepdim=True).values
    centred = points - (hi + lo) / 2
    if mode == "unit_sphere":
        scale = 2 * centred.norm(dim=-1, keepdim=True).max(dim=-2, keepdim=True).values
    else:
        scale = (hi - lo).max(dim=-1, keepdim=True).values
    return centred / torch.where(scale > 0, scale, torch.ones_like(scale))


# ----------------------------------------------------------------------------------------------------
# normalisation and export
# ----------------------------------------------------------------------------------------------------
class GlobalNormalizer(object):
    """(x - mean) / std with the training-set statistics of stats.json (test_optimize.py:32-75); identity statistics when
    the file is missing or unreadable, as in the reference."""

    def __init__(self):
        self.global_mean, self.global_std, self.is_fitted = None, None, False

    def load_stats(self, filepath="stats.json"):
        ok = False
        try:
            with open(filepath) as f:
                stats = json.load(f)
            self.global_mean, self.global_std, ok = torch.tensor(stats["mean"]), torch.tensor(stats["std"]), True
        except (OSError, KeyError, ValueError):
            self.global_mean, self.global_std = torch.zeros(3), torch.ones(3)
        self.is_fitted = True
        return ok

    def __call__(self, points, mode="norm"):
        if not self.is_fitted:
            self.load_stats()
        mean, std = self.global_mean.to(points.device), self.global_std.to(points.device)
        return (points - mean) / std if mode == "norm" else points * std + mean


def save_point_clouds(points, prefix, directory="."):
    """One `<prefix>_<i>.npy` file of float32 [N, 3] per generated sample (README.md:108-113). Returns the paths."""
    pts = points.detach().float().cpu().numpy() if torch.is_tensor(points) else np.asarray(points, dtype="float32")
    if pts.ndim != 3 or pts.shape[-1] != 3:
        raise ValueError(f"expected [B, N, 3] points, got {pts.shape}")
    os.makedirs(directory, exist_ok=True)
    paths = []
    for i, pc in enumerate(pts):
        paths.append(os.path.join(directory, f"{prefix}_{i}.npy"))
        np.save(paths[-1], pc)
    return paths


def _natural_key(name):
    return [int(t) if t.isdigit() else t for t in re.split(r"(\d+)", name)]


def load_point_clouds(path):
    """A point set as float32 numpy [S, n, 3] from either a `.npy` file holding [S, n, 3] (what `bench.py --dump-outputs
    DIR` writes as DIR/points.npy) or a directory of per-cloud [n, 3] `.npy` files (what save_point_clouds writes; read
    in natural name order, so `x_2.npy` comes before `x_10.npy`). Raises FileNotFoundError or ValueError."""
    if os.path.isdir(path):
        names = sorted((f for f in os.listdir(path) if f.endswith(".npy")), key=_natural_key)
        if not names:
            raise FileNotFoundError(f"{path}: no .npy files")
        clouds = [np.load(os.path.join(path, f), allow_pickle=False) for f in names]
        for f, c in zip(names, clouds):
            if c.ndim != 2 or c.shape[-1] != 3 or c.shape != clouds[0].shape:
                raise ValueError(f"{os.path.join(path, f)}: expected [{clouds[0].shape[0]}, 3] points like the first file, got {c.shape}")
        pts = np.stack(clouds)
    elif os.path.isfile(path):
        pts = np.load(path, allow_pickle=False)
        if pts.ndim != 3 or pts.shape[-1] != 3:
            raise ValueError(f"{path}: expected [S, n, 3] points, got {pts.shape}")
    else:
        raise FileNotFoundError(path)
    return np.ascontiguousarray(pts, dtype=np.float32)
