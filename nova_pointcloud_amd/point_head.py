"""Fused point head on MI355X: the step behind the transformer of the reference's two point-cloud forwards
(transformer_pointcloud_nova.py): self.output_proj = nn.Linear(embed_dim, 3) (:444, :611) applied as
x = self.output_proj(x); x.view(B, -1, 3) (:512-515, :778-781), which train_newloss.py wraps in
GradientGuard(max_grad_norm=15.0) (:34-43, :681-684, :782: an elementwise torch.clamp of the incoming gradient to +-15 through
a tensor hook, in training mode only) and whose result PointCloudLoss consumes (:469). In torch that is a GEMM of output
width 3 over [S, N, E], three more degenerate GEMMs in the backward (g @ W, g^T @ x, g.sum) and one pass for the hook.

It is point_embed transposed. One primitive carries the gradient: point_head, the forward of csrc/point_head.hip (one wave
per row, a fixed-order reduction over the channels) and a backward HIP kernel that reads x at most once and writes the
gradient of x at most once, with the clamp applied to the incoming gradient as it is loaded. x is read, and its gradient
written, in float32, bfloat16 or float16 as it arrives from the transformer: no cast of [S, N, E] is made. The backward saves
x and the weight alone. The definition, every rounding and the order of every sum, is in include/nova_hip.h at
nova_pointset_head.
GPU tensors only for the kernels: NovaHipError for CPU tensors or a missing library. Results are bitwise reproducible: the
same for every launch split, every position in the batch and every run, forward and backward (the per-cloud gradients
are summed in ascending cloud order by a kernel, after every launch)."""
import torch
from torch.autograd.function import once_differentiable

from . import hip
from ._pointset import (MAX_CLOUDS_PER_CALL, _all_floating, _all_tensors, _allocator, _at, _budget_clouds_per_launch, _check_clamp, _chunks,
                        _clouds_per_launch, _launch_stream, _launching, _on_gpu, _same_device, _sum_over)

HEAD_MAX_OUT = 8  # == NOVA_HEAD_MAX_OUT of include/nova_hip.h
HEAD_MAX_DIM = 4096  # == NOVA_HEAD_MAX_DIM
HEAD_MAX_POINTS = 65536  # == NOVA_HEAD_MAX_POINTS
HEAD_CHUNK = 128  # == NOVA_HEAD_CHUNK: rows per workgroup of the backward, the unit of its workspace
_NATIVE = (torch.float32, torch.bfloat16, torch.float16)  # what the kernels read and write as it is
# Per-launch budget, ESTIMATED BY BYTES as in point_embed.py, not from a measured time: the rows of x of a launch (the
# forward's read; the backward moves twice that), N E elements of x's own size per cloud. 2 GiB move in about a third of a
# millisecond at the 6.3e12 B/s a streaming kernel reaches on this chip.
_HEAD_BYTES_PER_LAUNCH = 1 << 31

# launches since import: forward calls of nova_pointset_head; backward calls of nova_pointset_head_bwd (the gradients of x,
# the weight and the bias from one read of x); sums over the clouds (the weight's and the bias's gradients). A kernel whose
# output no input needs is skipped
stats = {"forward_launches": 0, "backward_launches": 0, "cloud_sum_launches": 0}


def _head_arguments(x, weight, bias, grad_clamp):
    """ValueError for everything about the arguments that does not need the GPU (so it holds for CPU tensors too), in one
    order: types, dtypes, shapes, ranges, devices, grad_clamp."""
    given = [(x, "x"), (weight, "weight")] + ([(bias, "bias")] if bias is not None else [])
    _all_tensors(given)
    _all_floating(given)
    if x.dim() != 3:
        raise ValueError(f"x: expected [S, N, E] rows, got {tuple(x.shape)}")
    S, N, E = x.shape
    if weight.dim() != 2 or weight.shape[1] != E:
        raise ValueError(f"weight: expected [C, {E}] (the layout of nn.Linear.weight), got {tuple(weight.shape)}")
    C = weight.shape[0]
    if bias is not None and tuple(bias.shape) != (C,):
        raise ValueError(f"bias: expected [{C}], got {tuple(bias.shape)}")
    if not 1 <= C <= HEAD_MAX_OUT:
        raise ValueError(f"weight: the head kernel takes 1 .. {HEAD_MAX_OUT} outputs per point, got {C}")
    if not 1 <= E <= HEAD_MAX_DIM:
        raise ValueError(f"x: the head kernel takes 1 .. {HEAD_MAX_DIM} channels, got {E}")
    if not 1 <= N <= HEAD_MAX_POINTS:
        raise ValueError(f"x: the head kernel takes 1 .. {HEAD_MAX_POINTS} points per cloud, got {N}")
    _same_device(given)
    _check_clamp(grad_clamp, "grad_clamp")


class _PointHead(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, W, bias, clamp, per):
        S, N, E = x.shape
        C = W.shape[0]
        out = torch.empty(S, N, C, dtype=torch.float32, device=x.device)
        code = hip.dtype_code(x.dtype)
        for stream, s0, count in _launching(x.device, S, per):
            hip.call("nova_pointset_head", _at(x, s0), code, W.data_ptr(), bias.data_ptr() if bias is not None else None, _at(out, s0), count, N, C, E,
                     stream)
            stats["forward_launches"] += 1
        ctx.save_for_backward(x, W)  # the rows and the weight alone
        ctx.clamp, ctx.per = clamp, per
        ctx.set_materialize_grads(False)
        return out

    @staticmethod
    @once_differentiable
    def backward(ctx, g):
        x, W = ctx.saved_tensors
        per = ctx.per
        S, N, E = x.shape
        C = W.shape[0]
        want_x, want_w, want_b = ctx.needs_input_grad[:3]
        if g is None or not (want_x or want_w or want_b):
            return (None,) * 5
        g = g.float().contiguous()
        new = _allocator(S, x.device)
        gx = new(S, N, E, dtype=x.dtype) if want_x else None  # in x's own dtype, rounded once by the kernel
        gWs = new(S, C, E) if want_w else None  # per cloud
        gbs = new(S, C) if want_b else None
        ws = new(min(S, per) * _chunks(N, HEAD_CHUNK) * C * (E + 1)) if want_w or want_b else None
        gW = gb = None
        code = hip.dtype_code(x.dtype)
        with _launch_stream(x.device, S, per) as (stream, spans):
            for s0, count in spans:
                hip.call("nova_pointset_head_bwd", _at(x, s0) if want_w else None, code, W.data_ptr(), _at(g, s0), ctx.clamp, _at(gx, s0), _at(gWs, s0),
                         _at(gbs, s0), ws.data_ptr() if ws is not None else None, count, N, C, E, stream)
                stats["backward_launches"] += 1
            # after every launch has written its clouds: ascending cloud order, whatever the split
            if want_w:
                gW = _sum_over("nova_pointset_embed_sum_clouds", gWs, S, (C, E), C * E, stream=stream, stats=stats, key="cloud_sum_launches")
            if want_b:
                gb = _sum_over("nova_pointset_embed_sum_clouds", gbs, S, (C,), C, stream=stream, stats=stats, key="cloud_sum_launches")
        return gx, gW, gb, None, None


def point_head(x, weight, bias=None, grad_clamp=None, max_clouds_per_launch=None):
    """float32 [S, N, C]: F.linear(x, weight, bias) from one kernel that reads x once. x [S, N, E] in float32, bfloat16 or
    float16 goes to the kernel as it is (any other floating dtype is cast to float32, and a view that is not contiguous made
    contiguous, by a torch op); weight [C, E] (the layout of nn.Linear.weight) and bias [C] are small and are cast to float32
    by torch ops. 1 <= C <= 8, 1 <= E <= 4096, 1 <= N <= 65536. The definition, every rounding and the order of every sum, is
    in include/nova_hip.h at nova_pointset_head: x is converted exactly to float32 on load, a lane sums its channels in
    ascending order, the lanes are added in a fixed tree, and the bias is added once and only when given. Inputs are not
    checked for finiteness (a training path: no synchronisation); NaN comes out as in torch.

    grad_clamp = t (a positive finite number) clamps the incoming gradient elementwise to [-t, t] as the backward loads it
    (the reference's GradientGuard, 15.0 there); None leaves it as it is. The forward does not depend on it.

    Differentiable once in x, weight and bias. The gradient of x comes out of the kernel in x's own dtype (the float32 value
    rounded once); the gradients of weight and bias are float32 sums of per-cloud gradients in ascending cloud order, formed
    by a kernel after all launches and cast back by torch. The backward saves x and the weight alone. So the output and all
    gradients are bitwise the same for every `max_clouds_per_launch`, every position in the batch and every run. A kernel
    whose outputs no input needs is not launched and its output not allocated (`stats`). An empty cloud set (S = 0) launches
    nothing: the output and the gradient of x are empty, and the gradients of weight and bias, sums over no cloud, are +0.

    ValueError, in this order: types, dtypes, shapes, ranges (outputs per point, channels, points per cloud), devices,
    grad_clamp, max_clouds_per_launch. NovaHipError for CPU tensors."""
    _head_arguments(x, weight, bias, grad_clamp)
    N, E = x.shape[1], x.shape[2]
    itemsize = x.element_size() if x.dtype in _NATIVE else 4
    per = _clouds_per_launch(max_clouds_per_launch, _budget_clouds_per_launch(_HEAD_BYTES_PER_LAUNCH, itemsize * N * E), MAX_CLOUDS_PER_CALL)
    _on_gpu(((x, "x"), (weight, "weight"), (bias, "bias")), "the point head")
    f32 = lambda t: t.float().contiguous() if t is not None else None
    rows = (x if x.dtype in _NATIVE else x.float()).contiguous()
    return _PointHead.apply(rows, f32(weight), f32(bias), float(grad_clamp) if grad_clamp is not None else 0.0, per)


class PointHead(torch.nn.Module):
    """The last layer of the reference's point-cloud transformers (transformer_pointcloud_nova.py:444 and :611, applied at
    :512-515 and :778-781) on the HIP kernels: output_proj = nn.Linear(embed_dim, point_dim) under the reference's own name,
    so output_proj.weight and output_proj.bias of a reference checkpoint load. forward(x [B, N, embed_dim]) returns
    output_proj(x) as float32 [B, N, point_dim] from one kernel; x may be float32, bfloat16 or float16. grad_clamp is the
    reference's GradientGuard (train_newloss.py:34-43, 15.0 at :681-684): the incoming gradient is clamped to
    [-grad_clamp, grad_clamp] in training mode only. It runs on a GPU."""

    def __init__(self, embed_dim=768, point_dim=3, grad_clamp=None):
        super().__init__()
        self.output_proj = torch.nn.Linear(embed_dim, point_dim)
        self.grad_clamp = grad_clamp

    def forward(self, x):
        return point_head(x, self.output_proj.weight, self.output_proj.bias, grad_clamp=self.grad_clamp if self.training else None)
