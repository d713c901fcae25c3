"""Fused point embedding on MI355X: the step in front of every other point-set operation of the reference's two point-cloud
forwards (transformer_pointcloud_nova.py): point_embed = nn.Linear(point_cloud_dim, 768) followed by
x = x + self.pos_embed[:, :x.shape[1], :] (:562-565, :712-716), the per-cloud rows broadcast over the points (:753-756,
:759-760, :772; AutoregressiveDiffusion.forward :294, :297), EdgeAligner's nn.Linear(3, embed_dim) added onto a per-point base
(:174, :218-221) and PointCloudPatchEmbed / PointCloudPosEmbed at patch size 1 (:315-327, :340-346). In torch that is a GEMM
with K = 3 that writes [S, N, E] once and then one full read-and-write pass per addend; in the backward one read of the
incoming gradient per consumer.

One primitive carries the gradient: point_embed, the forward of csrc/point_embed.hip (one kernel that writes the output
once, every addend included) and a backward HIP kernel that reads the incoming gradient once for the gradients of the
points, the weight, the bias and cond. The gradient of pos is a second read of the incoming gradient, made only when pos
needs one (torch's g.sum(0) is the same read); the gradient of base is the incoming gradient itself. The backward saves
the points and the weight alone: nothing of size N E is stored. The definition, every rounding and the order of every sum,
is in include/nova_hip.h at nova_pointset_embed.
GPU tensors only for the kernels: NovaHipError for CPU tensors or a missing library. Results are bitwise reproducible: the
same for every launch split, every position in the batch and every run, forward and backward (the per-cloud gradients
are summed in ascending cloud order by a kernel, after every launch)."""
import torch
from torch.autograd.function import once_differentiable

from . import hip
from ._pointset import (MAX_CLOUDS_PER_CALL, _all_floating, _all_tensors, _allocator, _at, _budget_clouds_per_launch, _chunks, _clouds_per_launch,
                        _launch_stream, _launching, _on_gpu, _same_device, _sum_over)

EMBED_MAX_IN = 8  # == NOVA_EMBED_MAX_IN of include/nova_hip.h
EMBED_MAX_DIM = 4096  # == NOVA_EMBED_MAX_DIM
EMBED_MAX_POINTS = 65536  # == NOVA_EMBED_MAX_POINTS
EMBED_CHUNK = 128  # == NOVA_EMBED_CHUNK: rows per workgroup of the backward, the unit of its workspace
# Per-launch budget, ESTIMATED BY BYTES, not from a measured time: the output (forward) or the incoming gradient (backward)
# of a launch, 4 N E bytes per cloud. 2 GiB move in about a third of a millisecond at the 6.3e12 B/s a streaming kernel
# reaches on this chip, long against the launch overhead and short enough to leave the queue responsive.
_EMBED_BYTES_PER_LAUNCH = 1 << 31

# launches since import: forward calls of nova_pointset_embed; backward calls of nova_pointset_embed_bwd (the one read of g that
# forms the gradients of the points, the weight, the bias and cond); calls of nova_pointset_embed_pos_bwd (the second read of
# g, for pos alone); sums over the clouds (the weight's and the bias's gradients). A kernel whose output no input needs is
# skipped (a gradient into `base` alone launches nothing: it is the incoming gradient itself)
stats = {"forward_launches": 0, "backward_launches": 0, "pos_grad_launches": 0, "cloud_sum_launches": 0}


def _embed_arguments(points, weight, bias, pos, cond, base):
    """ValueError for everything about the arguments that does not need the GPU (so it holds for CPU tensors too), in one
    order: types, dtypes, shapes, cloud counts, ranges, devices."""
    given = [(points, "points"), (weight, "weight")] + [(t, name) for t, name in ((bias, "bias"), (pos, "pos"), (cond, "cond"), (base, "base"))
                                                        if t is not None]
    _all_tensors(given)
    _all_floating(given)
    if points.dim() != 3:
        raise ValueError(f"points: expected [S, N, C] clouds, got {tuple(points.shape)}")
    S, N, C = points.shape
    if weight.dim() != 2 or weight.shape[1] != C:
        raise ValueError(f"weight: expected [E, {C}] (the layout of nn.Linear.weight), got {tuple(weight.shape)}")
    E = weight.shape[0]
    if bias is not None and tuple(bias.shape) != (E,):
        raise ValueError(f"bias: expected [{E}], got {tuple(bias.shape)}")
    if pos is not None:
        table = pos[0] if pos.dim() == 3 and pos.shape[0] == 1 else pos
        if table.dim() != 2 or table.shape[1] != E or table.shape[0] < N:
            raise ValueError(f"pos: expected [P, {E}] or [1, P, {E}] with P >= {N} (one row per point), got {tuple(pos.shape)}")
    if cond is not None and (cond.dim() != 2 or cond.shape[1] != E):
        raise ValueError(f"cond: expected [S, {E}] (one row per cloud), got {tuple(cond.shape)}")
    if base is not None and (base.dim() != 3 or tuple(base.shape[1:]) != (N, E)):
        raise ValueError(f"base: expected [S, {N}, {E}] (one row of E channels per point), got {tuple(base.shape)}")
    for t, name in ((cond, "cond"), (base, "base")):
        if t is not None and t.shape[0] != S:
            raise ValueError(f"points and {name} must hold the same number of clouds, got {S} and {t.shape[0]}")
    if not 1 <= C <= EMBED_MAX_IN:
        raise ValueError(f"points: the embedding kernel takes 1 .. {EMBED_MAX_IN} inputs per point, got {C}")
    if not 1 <= E <= EMBED_MAX_DIM:
        raise ValueError(f"weight: the embedding kernel takes 1 .. {EMBED_MAX_DIM} channels, got {E}")
    if not 1 <= N <= EMBED_MAX_POINTS:
        raise ValueError(f"points: the embedding kernel takes 1 .. {EMBED_MAX_POINTS} points per cloud, got {N}")
    _same_device(given)


class _PointEmbed(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, W, bias, pos, cond, base, per):
        S, N, C = x.shape
        E = W.shape[0]
        out = torch.empty(S, N, E, dtype=torch.float32, device=x.device)
        ptr = lambda t: t.data_ptr() if t is not None else None
        for stream, s0, count in _launching(x.device, S, per):
            hip.call("nova_pointset_embed", _at(x, s0), W.data_ptr(), ptr(bias), ptr(pos), _at(cond, s0), _at(base, s0), _at(out, s0), count, N, C, E,
                     stream)
            stats["forward_launches"] += 1
        ctx.save_for_backward(x, W)  # [S, N, C], [E, C]: the points and the weight alone, nothing of size N E
        ctx.per = per
        ctx.set_materialize_grads(False)
        return out

    @staticmethod
    @once_differentiable
    def backward(ctx, g):
        x, W = ctx.saved_tensors
        per = ctx.per
        S, N, C = x.shape
        E = W.shape[0]
        want_x, want_w, want_b, want_p, want_c, want_base = ctx.needs_input_grad[:6]
        if g is None:
            return (None,) * 7
        gbase = g if want_base else None  # out = ... + base: the gradient of base is g itself, no kernel
        if not (want_x or want_w or want_b or want_p or want_c):
            return None, None, None, None, None, gbase, None
        g = g.float().contiguous()
        new = _allocator(S, x.device)
        gx = new(S, N, C) if want_x else None
        gWs = new(S, E, C) if want_w else None  # per cloud
        gcs = new(S, E) if want_b or want_c else None  # per cloud: cond's gradient as it stands
        ws = new(min(S, per) * _chunks(N, EMBED_CHUNK) * E * (C + 1)) if want_w or want_b or want_c else None
        gpos = new(N, E) if want_p else None
        gW = gb = None
        with _launch_stream(x.device, S, per) as (stream, spans):
            for n, (s0, count) in enumerate(spans):
                if gx is not None or ws is not None:
                    hip.call("nova_pointset_embed_bwd", _at(x, s0), W.data_ptr(), _at(g, s0), _at(gx, s0), _at(gWs, s0), _at(gcs, s0),
                             ws.data_ptr() if ws is not None else None, count, N, C, E, stream)
                    stats["backward_launches"] += 1
                if want_p:  # ascending launch order, the first one starting from +0: one left-to-right sum over the clouds
                    hip.call("nova_pointset_embed_pos_bwd", _at(g, s0), gpos.data_ptr(), count, N, E, 1 if n > 0 else 0, stream)
                    stats["pos_grad_launches"] += 1
            # after every launch has written its clouds: ascending cloud order, whatever the split
            if want_w:
                gW = _sum_over("nova_pointset_embed_sum_clouds", gWs, S, (E, C), E * C, stream=stream, stats=stats, key="cloud_sum_launches")
            if want_b:
                gb = _sum_over("nova_pointset_embed_sum_clouds", gcs, S, (E,), E, stream=stream, stats=stats, key="cloud_sum_launches")
        return gx, gW, gb, gpos, gcs if want_c else None, gbase, None


def point_embed(points, weight, bias=None, pos=None, cond=None, base=None, max_clouds_per_launch=None):
    """float32 [S, N, E]: F.linear(points, weight, bias) + pos[:N] + cond[:, None] + base in one kernel, every addend optional.
    points [S, N, C] (may be a strided view), weight [E, C] (the layout of nn.Linear.weight), bias [E]; pos [P, E] or the
    reference's [1, P, E] with P >= N, of which the first N rows are used (sliced by a torch op, so its gradient is zero in
    the rest); cond [S, E], one row per cloud broadcast over its points; base [S, N, E]. 1 <= C <= 8, 1 <= E <= 4096,
    1 <= N <= 65536, any floating dtype. The definition, every rounding and the order of every sum, is in include/nova_hip.h
    at nova_pointset_embed: the C products are one multiplication and C - 1 fused multiply-adds in ascending k, then the
    addends given are added in the order bias, pos, cond, base, each rounded once. Inputs are not checked for finiteness (a
    training path: no synchronisation); NaN comes out as in torch.

    Differentiable once in all six tensors. The casts to float32 are torch ops, so a bf16 or f16 input gets a gradient of
    its own dtype, the float32 gradient rounded once. The backward saves the points and the weight alone and reads the
    incoming gradient once for the gradients of points, weight, bias and cond; the gradient of pos reads it a second time
    (as torch's g.sum(0) does), and only when pos needs one; the gradient of base is the incoming gradient itself. The
    gradients of weight and bias are sums of per-cloud gradients in ascending cloud order, formed by a kernel after all
    launches, and the gradient of pos is one left-to-right sum over the clouds. So the output and all gradients are bitwise
    the same for every `max_clouds_per_launch`, every position in the batch and every run. A kernel whose outputs no input
    needs is not launched and its output not allocated (`stats`). An empty cloud set (S = 0) launches nothing: the output
    and the per-cloud gradients are empty, and the gradients of weight, bias and pos, sums over no cloud, are +0.

    ValueError, in this order: types, dtypes, shapes, cloud counts, ranges (inputs per point, channels, points per cloud),
    devices, max_clouds_per_launch. NovaHipError for CPU tensors."""
    _embed_arguments(points, weight, bias, pos, cond, base)
    N, E = points.shape[1], weight.shape[0]
    per = _clouds_per_launch(max_clouds_per_launch, _budget_clouds_per_launch(_EMBED_BYTES_PER_LAUNCH, 4 * N * E), MAX_CLOUDS_PER_CALL)
    _on_gpu(((points, "points"), (weight, "weight"), (bias, "bias"), (pos, "pos"), (cond, "cond"), (base, "base")), "the point embedding")
    f32 = lambda t: t.float().contiguous() if t is not None else None
    table = None
    if pos is not None:
        table = (pos[0] if pos.dim() == 3 else pos)[:N]  # a torch slice: autograd zero-fills the rows past N
    return _PointEmbed.apply(f32(points), f32(weight), f32(bias), f32(table), f32(cond), f32(base), per)


class PointEmbedding(torch.nn.Module):
    """The head of the reference's point-cloud transformers (transformer_pointcloud_nova.py:562-565, applied at :712-716) on
    the HIP kernels: point_embed = nn.Linear(point_dim, embed_dim) and pos_embed = nn.Parameter(randn(1, max_points,
    embed_dim) * 0.02) under the reference's own names, so the matching entries of a reference checkpoint load
    (point_embed.weight, point_embed.bias, pos_embed). forward(points [B, N, point_dim]) returns
    point_embed(points) + pos_embed[:, :N] in float32 from one kernel; forward(points, cond, base) also adds a per-cloud row
    cond [B, embed_dim] (the reference's timestep and text embeddings, :759-760, :772) and a per-point base [B, N, embed_dim]
    (:753-756) in that kernel. N may not exceed max_points. It runs on a GPU."""

    def __init__(self, point_dim=3, embed_dim=768, max_points=1024):
        super().__init__()
        self.point_embed = torch.nn.Linear(point_dim, embed_dim)
        self.pos_embed = torch.nn.Parameter(torch.randn(1, max_points, embed_dim) * 0.02)

    def forward(self, points, cond=None, base=None):
        return point_embed(points, self.point_embed.weight, self.point_embed.bias, pos=self.pos_embed, cond=cond, base=base)
