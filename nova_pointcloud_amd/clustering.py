"""Differentiable soft cluster pooling on MI355X: the soft clustering step both point-cloud models of the reference run in
their forward pass (PointCloudTransformer.forward, transformer_pointcloud_nova.py:465-487, and
NOVAPointCloudTransformer.forward, :724-741: torch.cdist to the learnable cluster_centers [8, 3], softmax(-distances) over
the centres, a Python loop over the 8 clusters forming (points * w).sum(1) / (w.sum(1) + 1e-8)): about 40 launches forward,
with the [B, N, 8] distances and weights and 8 [B, N, 3] products kept alive for the backward.

One primitive carries the gradient: soft_cluster_pool, the forward of csrc/soft_cluster.hip and a backward of HIP kernels
that recompute every weight from the points, the centres and the temperature. The backward saves the inputs, out and mass:
nothing of size N K is stored in either pass. The definition, every rounding and the order of every sum, is in
include/nova_hip.h at nova_pointset_soft_cluster.
GPU tensors only for the kernels: NovaHipError for CPU tensors or a missing library. Results are bitwise reproducible: the
same for every launch split, every position in the batch and every run, forward and backward, the gradient of shared
centres included (the per-cloud gradients are summed in ascending cloud order by a kernel, after every launch)."""
import torch
from torch.autograd.function import once_differentiable

from . import hip
from ._pointset import (MAX_CLOUDS_PER_CALL, _all_floating, _all_tensors, _allocator, _at, _budget_clouds_per_launch, _chunks, _clouds_per_launch,
                        _interp_scale, _launch_stream, _launching, _on_gpu, _same_device, _sum_over)

SOFT_CLUSTER_MAX_POINTS = 65536  # == NOVA_SOFT_CLUSTER_MAX_POINTS of include/nova_hip.h
SOFT_CLUSTER_MAX_K = 32  # == NOVA_SOFT_CLUSTER_MAX_K
SOFT_CLUSTER_CHUNK = 1024  # == NOVA_SOFT_CLUSTER_CHUNK: points per workgroup, the unit of the workspace
# Per-launch budget, ESTIMATED BY COUNT, not from a measured time: (point, centre) pairs a launch forms, about 40 issue slots
# each forward and 80 backward; 2^31 pairs are a few milliseconds on 256 compute units.
_SOFT_CLUSTER_PAIRS_PER_LAUNCH = 1 << 31

# launches since import: forward calls of nova_pointset_soft_cluster, backward calls of nova_pointset_soft_cluster_bwd that
# formed gx (the point gradient) and gc (the per-cloud centre gradient), and sums of gc over the clouds for shared centres;
# a kernel whose output no input needs is skipped
stats = {"forward_launches": 0, "point_grad_launches": 0, "center_grad_launches": 0, "cloud_sum_launches": 0}


def _pool_arguments(points, centers):
    """ValueError for everything about the tensors that does not need the GPU (so it holds for CPU tensors too), in one
    order: types, dtypes, shapes, cloud counts, ranges, device."""
    given = ((points, "points"), (centers, "centers"))
    _all_tensors(given)
    _all_floating(given)
    if points.dim() != 3 or points.shape[-1] != 3:
        raise ValueError(f"points: expected [S, N, 3] clouds, got {tuple(points.shape)}")
    if centers.dim() not in (2, 3) or centers.shape[-1] != 3:
        raise ValueError(f"centers: expected shared [K, 3] or per-cloud [S, K, 3] centres, got {tuple(centers.shape)}")
    if centers.dim() == 3 and centers.shape[0] != points.shape[0]:
        raise ValueError(f"points and centers must hold the same number of clouds, got {points.shape[0]} and {centers.shape[0]}")
    N, K = points.shape[1], centers.shape[-2]
    if not 1 <= N <= SOFT_CLUSTER_MAX_POINTS:
        raise ValueError(f"points: the soft-cluster kernel takes 1 .. {SOFT_CLUSTER_MAX_POINTS} points per cloud, got {N}")
    if not 1 <= K <= SOFT_CLUSTER_MAX_K:
        raise ValueError(f"centers: the soft-cluster kernel takes 1 .. {SOFT_CLUSTER_MAX_K} centres, got {K}")
    _same_device(given)


class _SoftCluster(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, c, scale, per):
        S, N = x.shape[0], x.shape[1]
        K, shared = c.shape[-2], c.dim() == 2
        out = torch.empty(S, K, 3, dtype=torch.float32, device=x.device)
        mass = torch.empty(S, K, dtype=torch.float32, device=x.device)
        ws = torch.empty(min(S, per) * _chunks(N, SOFT_CLUSTER_CHUNK) * K * 4, dtype=torch.float32, device=x.device)  # one launch's chunk partials
        for stream, s0, count in _launching(x.device, S, per):
            hip.call("nova_pointset_soft_cluster", _at(x, s0), c.data_ptr() if shared else _at(c, s0), _at(out, s0), _at(mass, s0),
                     ws.data_ptr(), count, N, K, 1 if shared else 0, scale, stream)
            stats["forward_launches"] += 1
        ctx.save_for_backward(x, c, out, mass)  # [S, N, 3], [K, 3] or [S, K, 3], [S, K, 3], [S, K]: nothing of size N K
        ctx.scale, ctx.per = scale, per
        ctx.set_materialize_grads(False)
        return out, mass

    @staticmethod
    @once_differentiable
    def backward(ctx, g, gm):
        x, c, out, mass = ctx.saved_tensors
        scale, per = ctx.scale, ctx.per
        S, N = x.shape[0], x.shape[1]
        K, shared = c.shape[-2], c.dim() == 2
        want_x, want_c = ctx.needs_input_grad[0], ctx.needs_input_grad[1]
        if (g is None and gm is None) or not (want_x or want_c):
            return None, None, None, None
        g = torch.zeros_like(out) if g is None else g.float().contiguous()
        gm = gm.float().contiguous() if gm is not None else None
        new = _allocator(S, x.device)
        gx = new(S, N, 3) if want_x else None
        gc = new(S, K, 3) if want_c else None  # per cloud in both centre forms
        ws = new(min(S, per) * _chunks(N, SOFT_CLUSTER_CHUNK) * K * 3) if want_c else None
        with _launch_stream(x.device, S, per) as (stream, spans):
            for s0, count in spans:
                hip.call("nova_pointset_soft_cluster_bwd", _at(x, s0), c.data_ptr() if shared else _at(c, s0), _at(out, s0), _at(mass, s0),
                         _at(g, s0), _at(gm, s0), _at(gx, s0), _at(gc, s0), ws.data_ptr() if want_c else None, count, N, K, 1 if shared else 0,
                         scale, stream)
                stats["point_grad_launches"] += 1 if want_x else 0
                stats["center_grad_launches"] += 1 if want_c else 0
            if want_c and shared:  # after every launch has written its clouds: ascending cloud order, whatever the split
                gc = _sum_over("nova_pointset_soft_cluster_sum_clouds", gc, S, (K, 3), K, stream=stream, stats=stats, key="cloud_sum_launches")
        return gx, gc, None, None


def soft_cluster_pool(points, centers, temperature=1.0, return_mass=False, max_clouds_per_launch=None):
    """float32 [S, K, 3]: for every cloud of points [S, N, 3] and every centre, the centroid of the cloud weighted by
    a[i, k] = softmax_k(-|points[s, i] - centre_k| / temperature): out[s, k] = sum_i a[i, k] points[s, i] /
    (sum_i a[i, k] + 1e-8), the reference's weighted_center (transformer_pointcloud_nova.py:465-487 and :724-741, where
    temperature is 1). centers is shared [K, 3] (the reference's cluster_centers parameter) or per cloud [S, K, 3];
    1 <= N <= 65536, 1 <= K <= 32, any floating dtype; points may be a strided view such as x[:, :, :3]. temperature=inf
    gives every centre the plain mean. return_mass=True returns (out, mass), mass [S, K] = sum_i a[i, k] (float32). The
    definition, every rounding and the order of every sum, is in include/nova_hip.h at nova_pointset_soft_cluster. Points
    are not checked for finiteness (a training path: no synchronisation); squared distances must be finite in float32.

    Differentiable once in points and centers, through both outputs. The casts to float32 are torch ops, so a bf16 or f16
    input gets a gradient of its own dtype, the float32 gradient rounded once. The backward saves the inputs, out and mass
    and recomputes every weight in a HIP kernel; a point lying exactly on a centre gets no gradient through that distance
    (torch.cdist's convention). The gradient of shared centres is the sum of the per-cloud gradients in ascending cloud
    order, formed by a kernel after all launches. So both outputs and both gradients are bitwise the same for every
    `max_clouds_per_launch`, every position in the batch and every run. A kernel whose outputs no input needs is not
    launched (`stats`).

    ValueError, in this order: types, dtypes, shapes, cloud counts, point and centre counts, devices, temperature,
    max_clouds_per_launch. NovaHipError for CPU tensors."""
    _pool_arguments(points, centers)
    scale = _interp_scale(temperature)
    per = _clouds_per_launch(max_clouds_per_launch, _budget_clouds_per_launch(_SOFT_CLUSTER_PAIRS_PER_LAUNCH, points.shape[1] * centers.shape[-2]),
                             MAX_CLOUDS_PER_CALL)
    _on_gpu(((points, "points"), (centers, "centers")), "the soft cluster pooling")
    xs = points.float().contiguous()
    cs = centers.float().contiguous()
    out, mass = _SoftCluster.apply(xs, cs, scale, per)
    return (out, mass) if return_mass else out
