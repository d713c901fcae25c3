"""Differentiable distance-weighted interpolation and adaptive sampling on MI355X: the reference's adaptive_sampling and
feature_aware_interpolation (transformer_pointcloud_nova.py:92-97, 128-152) as they sit in the model's forward, on a
gradient path. generate_pointcloud_autoregressive (:641-700) calls them without no_grad, so with use_autoregressive the
training gradient flows back into the points through softmax(-cdist) and the [S, T, N, 3] product, which PyTorch keeps
alive for the backward (1.3 GB for one 15 000-point cloud at half size).

One primitive carries the gradient: kernel_interpolate, the flash-style forward of csrc/interp.hip with its per-query
statistics (the minimum distance M and the weight sum L) and a backward of two HIP kernels that recompute every pair from
them (csrc/interp_bwd.hip; the definition, every rounding and the order of every sum, is in include/nova_hip.h at
nova_pointset_kernel_interpolate_bwd). Nothing of size T N is stored in either pass. The values are those of
nova_pointcloud_amd.metrics, bit for bit; metrics stays evaluation-only.
GPU tensors only for the kernel: NovaHipError for CPU tensors or a missing library. Results are bitwise reproducible: the
same for every launch split, every position in the batch and every run, forward and backward."""
import torch
from torch.autograd.function import once_differentiable

from . import hip, metrics
from ._pointset import (_INTERP_PAIRS_PER_LAUNCH, _adaptive_sampling, _at, _clouds_per_launch, _feature_aware_interpolation,
                        _interp_arguments, _interp_scale, _launching)

# launches since import: forward launches of nova_pointset_kernel_interpolate_stats, and launches of the two backward
# kernels (query side: gq; source side: gp and gv), which are skipped when no input needs their outputs
stats = {"forward_launches": 0, "query_side_launches": 0, "source_side_launches": 0}


class _Interpolate(torch.autograd.Function):
    @staticmethod
    def forward(ctx, q, p, v, scale, per):
        S, T, N = q.shape[0], q.shape[1], p.shape[1]
        C = 3 if v is None else v.shape[2]
        out = torch.empty(S, T, C, dtype=torch.float32, device=q.device)
        m = torch.empty(S, T, dtype=torch.float32, device=q.device)
        l = torch.empty(S, T, dtype=torch.float32, device=q.device)
        for stream, s0, count in _launching(q.device, S, per):
            hip.call("nova_pointset_kernel_interpolate_stats", _at(q, s0), _at(p, s0), _at(v, s0), _at(out, s0), _at(m, s0), _at(l, s0),
                     count, T, N, C, scale, stream)
            stats["forward_launches"] += 1
        ctx.save_for_backward(q, p, v, out, m, l)  # [S, T | N, 3 | C] and [S, T]: nothing of size T N
        ctx.args = (scale, per)
        return out

    @staticmethod
    @once_differentiable
    def backward(ctx, g):
        q, p, v, out, m, l = ctx.saved_tensors
        scale, per = ctx.args
        S, T, N = q.shape[0], q.shape[1], p.shape[1]
        C = out.shape[2]
        want_q, want_p = ctx.needs_input_grad[0], ctx.needs_input_grad[1]
        want_v = v is not None and ctx.needs_input_grad[2]
        g = g.float().contiguous()
        gq = torch.empty_like(q) if want_q else None
        gp = torch.empty_like(p) if want_p else None
        gv = torch.empty_like(v) if v is not None and (want_p or want_v) else None  # the source-side kernel forms gp and gv together
        if want_q or want_p or want_v:
            for stream, s0, count in _launching(q.device, S, per):
                hip.call("nova_pointset_kernel_interpolate_bwd", _at(q, s0), _at(p, s0), _at(v, s0), _at(out, s0), _at(m, s0), _at(l, s0),
                         _at(g, s0), _at(gq, s0), _at(gp, s0), _at(gv, s0), count, T, N, C, scale, stream)
                stats["query_side_launches"] += 1 if want_q else 0
                stats["source_side_launches"] += 1 if want_p or want_v else 0
        return gq, gp, gv if want_v else None, None, None


def kernel_interpolate(queries, points, values=None, temperature=1.0, max_clouds_per_launch=None):
    """metrics.kernel_interpolate with a gradient: float32 [S, T, C], row (s, i) the average of values[s] [N, C] over ALL
    source points points[s] [N, 3], weighted by softmax_j(-|queries[s, i] - points[s, j]| / temperature); values=None means
    the source points themselves (C = 3). Same arguments, checks and errors, and the same bits; differentiable in queries,
    points and values (not in the temperature, and once only). GPU tensors of any floating dtype: the cast to float32 is a
    torch op, so a bf16 or f16 input gets a gradient of its own dtype, the float32 gradient rounded once.

    Gradient (include/nova_hip.h, nova_pointset_kernel_interpolate_bwd): that of the softmax average, with the derivative
    of the distance at a coincident pair (distance exactly 0) taken as zero: no NaN, as in losses.nearest_match; the
    queries of feature_aware_interpolation are source points, so every query has such a pair. The backward saves the
    inputs, the output and two floats per query, and recomputes every pair in two kernels: one per query over all sources
    (gq), one per source over all queries in increasing index (gp and gv), without atomics, so all three gradients are
    bitwise the same for every `max_clouds_per_launch`, every position in the batch and every run. A kernel whose outputs
    no input needs is not launched (`stats`). Launch splits follow the forward's."""
    _interp_arguments(queries, points, values)
    scale = _interp_scale(temperature)
    named = [(queries, "queries"), (points, "points")] + ([(values, "values")] if values is not None else [])
    for t, name in named:
        if not t.is_cuda:
            raise hip.NovaHipError(f"{name}: the differentiable interpolation runs on the GPU (got a CPU tensor)")
    qs = queries.float().contiguous()
    ps = qs if points is queries else points.float().contiguous()
    vs = values.float().contiguous() if values is not None else None
    per = _clouds_per_launch(max_clouds_per_launch, _INTERP_PAIRS_PER_LAUNCH // (qs.shape[1] * ps.shape[1]))
    return _Interpolate.apply(qs, ps, vs, scale, per)


def feature_aware_interpolation(points, target_size, temperature=1.0, generator=None):
    """metrics.feature_aware_interpolation (the reference's, transformer_pointcloud_nova.py:128-152) with a gradient into
    the points: same signature, same values bit for bit. With N <= target_size the points are repeated cyclically (pure
    torch; works on CPU tensors); otherwise target_size of them, picked by one torch.randperm(N, generator=generator)
    shared by all clouds, become kernel_interpolate's average of ALL N points, and the gradient reaches the points both as
    sources and, through the indexing, as queries."""
    return _feature_aware_interpolation(kernel_interpolate, points, target_size, temperature, generator)


def adaptive_sampling(subset, target_size, temperature=1.0, generator=None):
    """metrics.adaptive_sampling (the reference's, transformer_pointcloud_nova.py:92-97, with the deviation noted there)
    with a gradient into the subset: N == target_size returns the input itself, N > target_size
    feature_aware_interpolation, N < target_size the points in farthest-point order repeated cyclically: the order is
    found on the detached points (indices carry no gradient) and the gather is torch's."""
    detached_order = lambda s, n: metrics.farthest_point_sample(s.detach(), n)  # indices carry no gradient
    return _adaptive_sampling(kernel_interpolate, detached_order, subset, target_size, temperature, generator)
