"""Depth-aware 3-D positional encoding on MI355X: the DepthAwarePositionalEncoding of the reference's PointCloudTransformer
(transformer_pointcloud_nova.py:349-389, applied at :456-458 as x = x + depth_pe): every coordinate, times a learnable
scale, through embed_dim // 6 frequencies as (sin, cos) pairs. In torch that is a zeros([B, N, E]), six strided slice
assignments each with its own [B, N, E / 6] division and sine or cosine, and a separate add: about 30 launches, with six
[B, N, E / 6] arguments kept alive for the backward.

One primitive carries the gradient: coordinate_encoding, the forward of csrc/posenc.hip (one kernel that writes the output
once, the add onto `base` included) and a backward HIP kernel that recomputes every argument, sine and cosine from the
points, the scales and the table. The backward saves the inputs alone: nothing of size N E is stored. The definition, every
rounding and the order of every sum, is in include/nova_hip.h at nova_pointset_posenc.
GPU tensors only for the kernels: NovaHipError for CPU tensors or a missing library. Results are bitwise reproducible: the
same for every launch split, every position in the batch and every run, forward and backward, the gradient of the scales
included (the per-cloud gradients are summed in ascending cloud order by a kernel, after every launch)."""
import torch
from torch.autograd.function import once_differentiable

from . import hip
from ._pointset import (MAX_CLOUDS_PER_CALL, _all_floating, _all_tensors, _allocator, _at, _budget_clouds_per_launch, _chunks, _clouds_per_launch,
                        _launch_stream, _launching, _on_gpu, _same_device, _sum_over)

POSENC_MAX_DIM = 4096  # == NOVA_POSENC_MAX_DIM of include/nova_hip.h
POSENC_MAX_POINTS = 65536  # == NOVA_POSENC_MAX_POINTS
POSENC_CHUNK = 32  # == NOVA_POSENC_CHUNK: rows per workgroup, the unit of the backward's workspace
# Per-launch budget, ESTIMATED BY COUNT, not from a measured time: (sin, cos) pairs a launch forms, each one IEEE division
# and one accurate sincosf (about 80 issue slots) and 8 bytes stored (forward) or read (backward); 2^28 pairs are 2 GiB of
# output, under a millisecond of stores and about as much arithmetic on 256 compute units.
_POSENC_PAIRS_PER_LAUNCH = 1 << 28
POSITION_SCALE = 10000.0  # the reference's position_scale (:358)

# launches since import: forward calls of nova_pointset_posenc, backward calls of nova_pointset_posenc_bwd that formed gx (the
# point gradient) and gs (the per-cloud scale gradient), and sums of gs over the clouds; a kernel whose output no input
# needs is skipped (a gradient into `base` alone launches nothing: it is the incoming gradient itself)
stats = {"forward_launches": 0, "point_grad_launches": 0, "scale_grad_launches": 0, "cloud_sum_launches": 0}

_tables = {}  # (embed_dim, device) -> the reference's table on that device


def reference_div_term(embed_dim):
    """The reference's div_term (:359-360), op for op on the CPU: float32 [ceil(embed_dim / 2)]."""
    return POSITION_SCALE ** (torch.arange(0, embed_dim, 2) / embed_dim)


def _reference_table(embed_dim, device):
    key = (embed_dim, torch.device(device))
    if key not in _tables:
        _tables[key] = reference_div_term(embed_dim)[:embed_dim // 6].to(device=device, dtype=torch.float32).contiguous()
    return _tables[key]


def _encoding_arguments(points, scale, embed_dim, base, div_term):
    """ValueError for everything about the arguments that does not need the GPU (so it holds for CPU tensors too), in one
    order: types, dtypes, shapes, cloud counts, ranges, devices."""
    given = [(points, "points"), (scale, "scale")] + [(t, name) for t, name in ((base, "base"), (div_term, "div_term")) if t is not None]
    _all_tensors(given)
    if not isinstance(embed_dim, int) or isinstance(embed_dim, bool):
        raise ValueError(f"embed_dim must be an integer, got {embed_dim!r}")
    _all_floating(given)
    if points.dim() != 3 or points.shape[-1] != 3:
        raise ValueError(f"points: expected [S, N, 3] clouds, got {tuple(points.shape)}")
    if tuple(scale.shape) != (3,):
        raise ValueError(f"scale: expected the three scales [3], got {tuple(scale.shape)}")
    if base is not None and (base.dim() != 3 or tuple(base.shape[1:]) != (points.shape[1], embed_dim)):
        raise ValueError(f"base: expected [S, {points.shape[1]}, {embed_dim}] (one row of embed_dim channels per point), got {tuple(base.shape)}")
    if div_term is not None and (div_term.dim() != 1 or div_term.shape[0] < embed_dim // 6):
        raise ValueError(f"div_term: expected a table of at least embed_dim // 6 = {embed_dim // 6} entries, got {tuple(div_term.shape)}")
    if base is not None and base.shape[0] != points.shape[0]:
        raise ValueError(f"points and base must hold the same number of clouds, got {points.shape[0]} and {base.shape[0]}")
    if not 6 <= embed_dim <= POSENC_MAX_DIM:
        raise ValueError(f"embed_dim: the encoding kernel takes 6 .. {POSENC_MAX_DIM} channels, got {embed_dim}")
    if not 1 <= points.shape[1] <= POSENC_MAX_POINTS:
        raise ValueError(f"points: the encoding kernel takes 1 .. {POSENC_MAX_POINTS} points per cloud, got {points.shape[1]}")
    if div_term is not None:
        used = div_term[:embed_dim // 6]
        if not bool(((used > 0) & torch.isfinite(used)).all()):
            raise ValueError("div_term: the divisors must be positive and finite")
    _same_device(given)


class _Encoding(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, scale, div, base, E, per):
        S, N = x.shape[0], x.shape[1]
        out = torch.empty(S, N, E, dtype=torch.float32, device=x.device)
        for stream, s0, count in _launching(x.device, S, per):
            hip.call("nova_pointset_posenc", _at(x, s0), scale.data_ptr(), div.data_ptr(), _at(base, s0), _at(out, s0), count, N, E, stream)
            stats["forward_launches"] += 1
        ctx.save_for_backward(x, scale, div)  # [S, N, 3], [3], [F]: the inputs alone, nothing of size N E
        ctx.E, ctx.per = E, per
        ctx.set_materialize_grads(False)
        return out

    @staticmethod
    @once_differentiable
    def backward(ctx, g):
        x, scale, div = ctx.saved_tensors
        E, per = ctx.E, ctx.per
        S, N = x.shape[0], x.shape[1]
        want_x, want_s, want_b = ctx.needs_input_grad[0], ctx.needs_input_grad[1], ctx.needs_input_grad[3]
        if g is None:
            return None, None, None, None, None, None
        gb = g if want_b else None  # out = base + pe: the gradient of base is g itself, no kernel
        if not (want_x or want_s):
            return None, None, None, gb, None, None
        g = g.float().contiguous()
        new = _allocator(S, x.device)
        gx = new(S, N, 3) if want_x else None
        gs = new(S, 3) if want_s else None  # per cloud
        ws = new(min(S, per) * _chunks(N, POSENC_CHUNK) * 3) if want_s else None
        with _launch_stream(x.device, S, per) as (stream, spans):
            for s0, count in spans:
                hip.call("nova_pointset_posenc_bwd", _at(x, s0), scale.data_ptr(), div.data_ptr(), _at(g, s0), _at(gx, s0), _at(gs, s0),
                         ws.data_ptr() if want_s else None, count, N, E, stream)
                stats["point_grad_launches"] += 1 if want_x else 0
                stats["scale_grad_launches"] += 1 if want_s else 0
            if want_s:  # after every launch has written its clouds: ascending cloud order, whatever the split
                # the cloud sum of the soft cluster pooling with K = 1: the same contract (include/nova_hip.h)
                gs = _sum_over("nova_pointset_soft_cluster_sum_clouds", gs, S, (3,), 1, stream=stream, stats=stats, key="cloud_sum_launches")
        return gx, gs, None, gb, None, None


def coordinate_encoding(points, scale, embed_dim, base=None, div_term=None, max_clouds_per_launch=None):
    """float32 [S, N, embed_dim]: the reference's depth-aware positional encoding of points [S, N, 3]
    (transformer_pointcloud_nova.py:367-389). With F = embed_dim // 6, for coordinate c and frequency f < F,
    a = points[s, i, c] * scale[c] / div_term[f], channel 6 f + 2 c is sin(a) and channel 6 f + 2 c + 1 is cos(a); the
    channels from 6 F on (where embed_dim % 6 != 0, which the reference cannot take) are zero. With `base`
    [S, N, embed_dim] the result is base + encoding (the reference's x = x + depth_pe, :458), formed in the same kernel.
    scale is a tensor [3] (the reference's scale_x, scale_y, scale_z); it stays on the device, nothing synchronises.
    div_term is None for the reference's table, (10000.0 ** (torch.arange(0, E, 2) / E))[:F] built by those torch ops (bit
    for bit the reference's), or a positive finite float tensor of at least F entries (checking a given table on the GPU
    synchronises). 6 <= embed_dim <= 4096, 1 <= N <= 65536, any floating dtype; points may be a strided view. The
    definition, every rounding and the order of every sum, is in include/nova_hip.h at nova_pointset_posenc. Points are not
    checked for finiteness (a training path: no synchronisation); NaN comes out as in torch.

    Differentiable once in points, scale and base. The casts to float32 are torch ops, so a bf16 or f16 input gets a
    gradient of its own dtype, the float32 gradient rounded once. The backward saves the inputs alone (points, scale, the
    table) and recomputes every sine and cosine in a HIP kernel; the gradient of base is the incoming gradient itself. The
    gradient of scale is the sum of the per-cloud gradients in ascending cloud order, formed by a kernel after all
    launches. So the output and all gradients are bitwise the same for every `max_clouds_per_launch`, every position in the
    batch and every run. A kernel whose outputs no input needs is not launched (`stats`).

    ValueError, in this order: types, dtypes, shapes, cloud counts, ranges (embed_dim, points per cloud, the table's
    values), devices, max_clouds_per_launch. NovaHipError for CPU tensors."""
    _encoding_arguments(points, scale, embed_dim, base, div_term)
    per = _clouds_per_launch(max_clouds_per_launch, _budget_clouds_per_launch(_POSENC_PAIRS_PER_LAUNCH, points.shape[1] * 3 * (embed_dim // 6)),
                             MAX_CLOUDS_PER_CALL)
    _on_gpu(((points, "points"), (scale, "scale"), (base, "base"), (div_term, "div_term")), "the coordinate encoding")
    div = _reference_table(embed_dim, points.device) if div_term is None else div_term.detach().float().contiguous()
    xs = points.float().contiguous()
    sc = scale.float().contiguous()
    bs = base.float().contiguous() if base is not None else None
    return _Encoding.apply(xs, sc, div, bs, embed_dim, per)


class DepthAwarePositionalEncoding(torch.nn.Module):
    """The reference's DepthAwarePositionalEncoding (transformer_pointcloud_nova.py:349-389) on the HIP kernels: the same
    constructor, the same attributes (embed_dim, max_points, position_scale, dim_div, div_term: plain CPU tensors, not
    buffers) and the same three parameters scale_x, scale_y, scale_z, each [1] and initialised to 1, so a state_dict of the
    reference loads. forward(points [B, N, 3]) returns the encoding [B, N, embed_dim] in float32; forward(points, base)
    returns base + encoding in one kernel (the reference's x = x + depth_pe, :458).

    Two differences from the reference, both on purpose:
      - it runs on a GPU: the reference divides a device tensor by its CPU attribute div_term and raises; here the table is
        moved to the input's device once and cached per device;
      - embed_dim % 6 != 0 is accepted (1024 for instance), with zero tail channels from 6 (embed_dim // 6) on; the
        reference raises there, because pe[:, :, 0::6] then has one slot more than div_term[:embed_dim // 6].
    And the scales multiply per coordinate (scale_x the x of every point): the reference stacks them to [3, 1], which
    broadcasts along the point axis and raises unless there are 1 or 3 points (:372).
    The table handed to the kernel is checked like any caller's (positive, finite), which reads one flag back per call."""

    def __init__(self, embed_dim, max_points=2048):
        super().__init__()
        self.embed_dim = embed_dim
        self.max_points = max_points
        self.position_scale = POSITION_SCALE
        self.dim_div = torch.arange(0, embed_dim, 2) / embed_dim
        self.div_term = self.position_scale ** self.dim_div
        self.scale_x = torch.nn.Parameter(torch.ones(1))
        self.scale_y = torch.nn.Parameter(torch.ones(1))
        self.scale_z = torch.nn.Parameter(torch.ones(1))
        self._device_tables = {}

    def _table(self, device):
        if device not in self._device_tables:
            self._device_tables[device] = self.div_term[:self.embed_dim // 6].to(device=device, dtype=torch.float32).contiguous()
        return self._device_tables[device]

    def forward(self, points, base=None):
        scale = torch.cat([self.scale_x, self.scale_y, self.scale_z])  # autograd hands each parameter its entry
        table = self._table(points.device) if torch.is_tensor(points) else None
        return coordinate_encoding(points, scale, self.embed_dim, base=base, div_term=table)
