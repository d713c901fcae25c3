"""Differentiable kNN neighbourhood feature aggregation on MI355X: the reference's EdgeAligner.extract_edge_features
(transformer_pointcloud_nova.py:176-190: cdist, topk(8), a gather to [B, N, k, C], mean, features - mean), which
EdgeAligner.forward (:192-223) calls for every subset on 768-wide features with the [B, N, N] matrix and the [B, N, k, C]
tensor kept alive for the backward (1.6 GB at 32 x 2048 points), and the aggregation step of every kNN-graph layer
(EdgeConv-style neighbour pooling, PointNet++'s three_interpolate).

One primitive carries the gradient: neighbor_aggregate, the forward of csrc/neighbor.hip and a backward of HIP kernels:
the weight gradient as one dot product per edge, the feature gradient as a GATHER through the inverse neighbour list
(nova_pointset_neighbor_inverse), not torch's index_add with float atomics. The definition, every rounding and the order of
every sum, is in include/nova_hip.h at nova_pointset_neighbor_aggregate. metrics.knn_points feeds it directly; nothing of
size N M or N k C is stored in either pass.
GPU tensors only for the kernels: NovaHipError for CPU tensors or a missing library. Results are bitwise reproducible: the
same for every launch split, every position in the batch and every run, forward and backward."""
import torch
from torch.autograd.function import once_differentiable

from . import hip, metrics
from ._pointset import _at, _at_least_one, _check_clouds, _clouds_per_launch, _launching

NEIGHBOR_MAX_CHANNELS = 4096  # == NOVA_NEIGHBOR_MAX_CHANNELS of include/nova_hip.h
_MAX_CLOUDS_PER_CALL = 65535  # clouds go in grid.y
# Per-launch budgets, ESTIMATED BY COUNT, not yet from a measured time (tools/neighbor_bench.py writes
# profiles/neighbor_bench.json; re-derive both from the longest launch it records). Bytes a launch moves, forward or
# backward, (M + N + N k) C 4 per cloud: 2^34 is a few milliseconds at the HBM rate. Integer compares of the inverse list,
# 3 M N k per cloud: 2^35 is about 10 ms at one compare per lane per cycle on 256 compute units.
_NEIGHBOR_BYTES_PER_LAUNCH = 1 << 34
_NEIGHBOR_COMPARES_PER_LAUNCH = 1 << 35

# launches since import: forward launches of nova_pointset_neighbor_aggregate, builds of the inverse list, and backward
# launches that formed gf (the feature gradient) and gw (the weight gradient); a kernel whose output no input needs is skipped
stats = {"forward_launches": 0, "inverse_launches": 0, "feature_grad_launches": 0, "weight_grad_launches": 0}


def _default_clouds_per_launch(N, M, k, C):
    by_bytes = _NEIGHBOR_BYTES_PER_LAUNCH // ((M + N + N * k) * C * 4)
    by_compares = _NEIGHBOR_COMPARES_PER_LAUNCH // (3 * M * N * k)
    return max(1, min(by_bytes, by_compares, _MAX_CLOUDS_PER_CALL))


def _aggregate_arguments(features, idx, weights):
    """ValueError for everything about the arguments that does not need the GPU (so it holds for CPU tensors too), in one
    order: types, dtypes, shapes, cloud counts, ranges, device."""
    named = [(features, "features"), (idx, "idx")] + ([(weights, "weights")] if weights is not None else [])
    for t, name in named:
        if not torch.is_tensor(t):
            raise ValueError(f"{name}: expected a tensor, got {type(t).__name__}")
    if not features.is_floating_point():
        raise ValueError(f"features: expected a floating dtype, got {features.dtype}")
    if idx.dtype not in (torch.int64, torch.int32):
        raise ValueError(f"idx: expected int64 or int32 indices (as knn_points returns them), got {idx.dtype}")
    if weights is not None and not weights.is_floating_point():
        raise ValueError(f"weights: expected a floating dtype, got {weights.dtype}")
    if features.dim() != 3:
        raise ValueError(f"features: expected [S, M, C], got {tuple(features.shape)}")
    if idx.dim() != 3:
        raise ValueError(f"idx: expected [S, N, k], got {tuple(idx.shape)}")
    if weights is not None and weights.shape != idx.shape:
        raise ValueError(f"weights: expected the shape of idx {tuple(idx.shape)}, got {tuple(weights.shape)}")
    if features.shape[0] != idx.shape[0]:
        raise ValueError(f"features and idx must hold the same number of clouds, got {features.shape[0]} and {idx.shape[0]}")
    (M, C), (N, k) = features.shape[1:], idx.shape[1:]
    for n, name in ((N, "idx"), (M, "features")):
        if not 1 <= n <= metrics.KNN_MAX_POINTS:
            raise ValueError(f"{name}: the neighbour kernels take 1 .. {metrics.KNN_MAX_POINTS} points per cloud, got {n}")
    if not 1 <= k <= metrics.KNN_MAX_K:
        raise ValueError(f"idx: the neighbour kernels take k in 1 .. {metrics.KNN_MAX_K}, got {k}")
    if not 1 <= C <= NEIGHBOR_MAX_CHANNELS:
        raise ValueError(f"features: the neighbour kernels take 1 .. {NEIGHBOR_MAX_CHANNELS} channels, got {C}")
    if len({t.device for t, _ in named}) > 1:
        raise ValueError(f"{' and '.join(n for _, n in named)} must be on the same device, got "
                         f"{' and '.join(str(t.device) for t, _ in named)}")


class _Aggregate(torch.autograd.Function):
    @staticmethod
    def forward(ctx, f, idx, w, per):
        S, M, C = f.shape
        N, k = idx.shape[1], idx.shape[2]
        out = torch.empty(S, N, C, dtype=torch.float32, device=f.device)
        for stream, s0, count in _launching(f.device, S, per):
            hip.call("nova_pointset_neighbor_aggregate", _at(f, s0), _at(idx, s0), _at(w, s0), _at(out, s0), count, N, M, k, C, stream)
            stats["forward_launches"] += 1
        ctx.save_for_backward(f, idx, w)  # [S, M, C], [S, N, k], [S, N, k]: nothing of size N k C
        ctx.per = per
        return out

    @staticmethod
    @once_differentiable
    def backward(ctx, g):
        f, idx, w = ctx.saved_tensors
        per = ctx.per
        S, M, C = f.shape
        N, k = idx.shape[1], idx.shape[2]
        want_f = ctx.needs_input_grad[0]
        want_w = w is not None and ctx.needs_input_grad[2]
        gf = torch.empty_like(f) if want_f else None
        gw = torch.empty_like(w) if want_w else None
        if want_f or want_w:
            g = g.float().contiguous()
            # the inverse neighbour list exists only while the feature gradient is formed
            offsets = torch.empty(S, M + 1, dtype=torch.int32, device=f.device) if want_f else None
            edges = torch.empty(S, N * k, dtype=torch.int32, device=f.device) if want_f else None
            for stream, s0, count in _launching(f.device, S, per):
                if want_f:
                    hip.call("nova_pointset_neighbor_inverse", _at(idx, s0), _at(offsets, s0), _at(edges, s0), count, N, M, k, stream)
                    stats["inverse_launches"] += 1
                hip.call("nova_pointset_neighbor_aggregate_bwd", _at(f, s0), _at(idx, s0), _at(w, s0), _at(g, s0), _at(offsets, s0),
                         _at(edges, s0), _at(gf, s0), _at(gw, s0), count, N, M, k, C, stream)
                stats["feature_grad_launches"] += 1 if want_f else 0
                stats["weight_grad_launches"] += 1 if want_w else 0
        return gf, None, gw, None


def neighbor_aggregate(features, idx, weights=None, max_clouds_per_launch=None):
    """float32 [S, N, C]: row (s, i) the mean over t of features[s, idx[s, i, t]] (weights=None), or the weighted sum
    sum_t weights[s, i, t] * features[s, idx[s, i, t]], summed in the order t = 0 .. k-1 in float32 (include/nova_hip.h,
    nova_pointset_neighbor_aggregate). features [S, M, C] of any floating dtype, idx [S, N, k] int64 or int32 as
    metrics.knn_points returns it, weights [S, N, k] of any floating dtype; 1 <= N, M <= 65536, 1 <= k <= 32,
    1 <= C <= 4096. An index outside 0 .. M-1 is never read and adds +0 (in the mean it still counts in the divisor k);
    duplicate indices in a row are allowed.

    Differentiable in features and, when given, in weights (once; idx carries no gradient). The casts to float32 are torch
    ops, so a bf16 or f16 input gets a gradient of its own dtype, the float32 gradient rounded once. The backward saves the
    inputs alone and runs HIP kernels: the weight gradient is one dot product per edge; the feature gradient is a gather,
    one wave per target row walking the inverse neighbour list (built in the backward, and only when features needs a
    gradient) in increasing edge order, without atomics. So out and both gradients are bitwise the same for every
    `max_clouds_per_launch`, every position in the batch and every run. A kernel whose outputs no input needs is not
    launched (`stats`). Default launch split: _NEIGHBOR_BYTES_PER_LAUNCH and _NEIGHBOR_COMPARES_PER_LAUNCH above."""
    _aggregate_arguments(features, idx, weights)
    (M, C), (N, k) = features.shape[1:], idx.shape[1:]
    per = _clouds_per_launch(max_clouds_per_launch, _default_clouds_per_launch(N, M, k, C), _MAX_CLOUDS_PER_CALL)
    for t, name in [(features, "features"), (idx, "idx")] + ([(weights, "weights")] if weights is not None else []):
        if not t.is_cuda:
            raise hip.NovaHipError(f"{name}: the neighbourhood aggregation runs on the GPU (got a CPU tensor)")
    fs = features.float().contiguous()
    ix = idx.to(torch.int32).contiguous()
    ws = weights.float().contiguous() if weights is not None else None
    return _Aggregate.apply(fs, ix, ws, per)


def neighbor_mean(features, idx):
    """neighbor_aggregate with weights=None: the mean of the k named rows."""
    return neighbor_aggregate(features, idx)


def _feature_rows(points, features, name, what):
    if not torch.is_tensor(features) or not features.is_floating_point() or features.dim() != 3:
        raise ValueError(f"{name}: expected a floating tensor [S, N, C], got "
                         f"{tuple(features.shape) if torch.is_tensor(features) else type(features).__name__}")
    if features.shape[:2] != points.shape[:2]:
        raise ValueError(f"{name}: expected one row per point of {what} {tuple(points.shape[:2])}, got {tuple(features.shape[:2])}")


def edge_features(points, features, k=8, max_clouds_per_launch=None):
    """The reference's extract_edge_features (transformer_pointcloud_nova.py:176-190), float32 [S, N, C]:
    features - neighbor_mean(features, the min(k, N) nearest neighbours of every point of points [S, N, 3] in its own
    cloud). The point itself is among its neighbours (distance 0), as in the reference's topk over cdist(points, points);
    ties go to the lowest index (metrics.knn_points). Differentiable in features, not in points: the reference's topk
    indices carry no gradient either. DEVIATION: the reference's gather does not run as written for [B, N, C] features;
    this is its comment (centre feature minus the mean of the k nearest neighbours' features)."""
    _check_clouds([(points, "points")], letters="S, N", count_range=("kNN", metrics.KNN_MAX_POINTS))
    _feature_rows(points, features, "features", "points")
    _at_least_one(k, "k")
    if max_clouds_per_launch is not None:
        _at_least_one(max_clouds_per_launch, "max_clouds_per_launch")
    pts = points.detach()
    idx = metrics.knn_points(pts, pts, k=min(k, points.shape[1]), exclude_self=False, return_distances=False,
                             max_clouds_per_launch=max_clouds_per_launch)
    return features - neighbor_aggregate(features, idx, max_clouds_per_launch=max_clouds_per_launch)


def knn_interpolate(queries, points, values, k=3, eps=1e-8):
    """PointNet++'s inverse-distance interpolation (three_interpolate at k = 3), float32 [S, T, C]: for every query of
    queries [S, T, 3] the average of values [S, N, C] over its k nearest points of points [S, N, 3], weighted by
    1 / (d2 + eps) normalised over the k neighbours, d2 the squared distance. The neighbours come from metrics.knn_points
    (no [T, N] array); d2 is recomputed in torch from the [S, T, k, 3] gathered neighbour coordinates, so the result is
    differentiable in queries and points through the weight gradient of neighbor_aggregate, and in values through its
    feature gradient. A query coincident with a source has d2 = 0 there and weight 1 / eps before normalisation: finite
    values and gradients for eps > 0."""
    _check_clouds([(queries, "queries"), (points, "points")], letters="S, N", count_range=("kNN", metrics.KNN_MAX_POINTS), same_clouds=True)
    _feature_rows(points, values, "values", "points")
    N = points.shape[1]
    if not isinstance(k, int) or isinstance(k, bool) or not 1 <= k <= min(metrics.KNN_MAX_K, N):
        raise ValueError(f"k must be an integer in 1 .. {min(metrics.KNN_MAX_K, N)} (at most {metrics.KNN_MAX_K}, and {N} points), got {k!r}")
    if not isinstance(eps, (int, float)) or isinstance(eps, bool) or not eps > 0 or eps == float("inf"):
        raise ValueError(f"eps must be a finite number > 0, got {eps!r}")
    idx = metrics.knn_points(queries.detach(), points.detach(), k=k, exclude_self=False, return_distances=False)
    S, T = queries.shape[0], queries.shape[1]
    near = torch.gather(points.float(), 1, idx.reshape(S, T * k, 1).expand(S, T * k, 3)).view(S, T, k, 3)
    d2 = (queries.float()[:, :, None, :] - near).square().sum(dim=-1)
    w = 1.0 / (d2 + eps)
    return neighbor_aggregate(values, idx, w / w.sum(dim=-1, keepdim=True))
