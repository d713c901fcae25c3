"""Fused bias-dropout-residual on MI355X: the elementwise chains of the transformer body of the reference's point-cloud models
(transformer_pointcloud_nova.py: nn.TransformerEncoderLayer(d_model, nhead, dim_feedforward=4*d_model, dropout=0.1,
batch_first=True, norm_first=True) with the default ReLU, stacked at :433-441 and :590-598, run at :510 and :775; dropout=0.1
from train_newloss.py:652, :673). A training step runs each layer as
    x = x + dropout1(out_proj(attn(norm1(x))))                      bias + dropout + residual on [B, N, E], twice per layer
    x = x + dropout2(linear2(dropout(relu(linear1(norm2(x))))))     bias + ReLU + dropout on [B, N, 4E], once per layer
and in torch each chain reads and writes the activation three or four times and keeps a [rows, D] boolean mask from the device
generator. bias_dropout_add is one kernel of csrc/dropout_add.hip forward and one backward: every operand read once, the
output written once, and the mask Philox4x32-10 keyed on (seed, subsequence, element index), regenerated in the backward and
never stored. The definition, the generator and every rounding, is in include/nova_hip.h at nova_bias_dropout_add.
The seed is a host number: given, or drawn from a CPU torch.Generator (the global one by default), so torch.manual_seed fixes a
training step, activation checkpointing (which restores the CPU generator's state) recomputes the same mask, and nothing here
touches the device generator or synchronises. Not for use inside torch.cuda.graph capture (the seed would be frozen).
GPU tensors only for the kernels: NovaHipError for CPU tensors or a missing library. Results are bitwise reproducible: the
same for every run and every alignment of the storage."""
import numbers
from fractions import Fraction

import numpy as np
import torch
from torch.autograd.function import once_differentiable

from . import hip
from ._pointset import _all_floating, _all_tensors, _chunks, _on_gpu, _same_device, _sum_over

DROPOUT_MAX_DIM = 16384  # == NOVA_DROPOUT_MAX_DIM of include/nova_hip.h
DROPOUT_MAX_ROWS = 1 << 30  # == NOVA_DROPOUT_MAX_ROWS
DROPOUT_CHUNK = 128  # == NOVA_DROPOUT_CHUNK: rows per row of the bias gradient's partial sums
ACT_NONE, ACT_RELU = 0, 1  # NOVA_DROPOUT_ACT_NONE, NOVA_DROPOUT_ACT_RELU
_ACTIVATIONS = {None: ACT_NONE, "relu": ACT_RELU}
_NATIVE = (torch.float32, torch.bfloat16, torch.float16)  # what the kernels read and write as it is
_U64 = (1 << 64) - 1

# launches since import: forward calls of nova_bias_dropout_add; backward calls of nova_bias_dropout_add_bwd (the gradients of
# x and the bias's chunk sums from one read of g); sums over the chunks (the bias's gradient). A kernel whose output no input
# needs is skipped
stats = {"forward_launches": 0, "backward_launches": 0, "bias_sum_launches": 0}


def dropout_threshold(p):
    """(T, scale) as the kernels take them: T = floor(p 2^32) in exact integer arithmetic (an element is kept iff its 32-bit draw
    is >= T: 0 keeps everything, 2^32 nothing), scale = the float32 nearest to the float64 quotient 1 / (1 - p), one division
    and one rounding (1 for p = 0; 0, unused, for p = 1)."""
    T = int((Fraction(p) if isinstance(p, numbers.Rational) else Fraction(float(p))) * (1 << 32))  # p >= 0: truncation is the floor
    scale = float(np.float32(np.float64(1.0) / (np.float64(1.0) - np.float64(p)))) if p < 1 else 0.0
    return T, scale


def draw_seed(generator=None):
    """One seed in 0 .. 2^63 - 1 from a CPU torch.Generator (None: the global one torch.manual_seed sets). No device work."""
    return int(torch.empty((), dtype=torch.int64).random_(generator=generator))


def mask_numbers(p, training=True, seed=None, generator=None):
    """(T, scale, seed) of one call: training=False is p = 0; where nothing is dropped (T == 0) no Philox is evaluated, so no seed
    is drawn and the generator is left alone; otherwise seed=None draws one."""
    T, scale = dropout_threshold(p if training else 0)
    if T == 0:
        return T, scale, 0
    return T, scale, draw_seed(generator) if seed is None else seed


def _dropout_arguments(x, bias, residual, p, activation, seed, subsequence, generator):
    """ValueError for everything about the arguments that does not need the GPU (so it holds for CPU tensors too), in one
    order: types, dtypes, shapes, D range, devices, p, activation (and activation with residual), seed / subsequence range."""
    given = [(x, "x")] + [(t, name) for t, name in ((bias, "bias"), (residual, "residual")) if t is not None]
    _all_tensors(given)
    _all_floating(given)
    if residual is not None and residual.dtype != x.dtype:
        raise ValueError(f"residual: expected x's dtype {x.dtype}, got {residual.dtype}")
    if x.dim() < 1:
        raise ValueError(f"x: expected [..., D] rows, got {tuple(x.shape)}")
    D = x.shape[-1]
    if residual is not None and residual.shape != x.shape:
        raise ValueError(f"residual: expected x's shape {tuple(x.shape)}, got {tuple(residual.shape)}")
    if bias is not None and tuple(bias.shape) != (D,):
        raise ValueError(f"bias: expected [{D}], got {tuple(bias.shape)}")
    if not 1 <= D <= DROPOUT_MAX_DIM:
        raise ValueError(f"x: the dropout kernel takes 1 .. {DROPOUT_MAX_DIM} columns, got {D}")
    if x.numel() // D > DROPOUT_MAX_ROWS:
        raise ValueError(f"x: the dropout kernel takes at most {DROPOUT_MAX_ROWS} rows, got {x.numel() // D}")
    _same_device(given)
    if isinstance(p, bool) or not isinstance(p, numbers.Real) or not 0 <= p <= 1:  # a NaN fails the comparison
        raise ValueError(f"p must be a real number in [0, 1], got {p!r}")
    if activation not in _ACTIVATIONS:
        raise ValueError(f"activation must be None or 'relu', got {activation!r}")
    if activation is not None and residual is not None:
        raise ValueError("activation 'relu' takes no residual (the reference has no such site, and the backward gates on the output)")
    for v, name in ((seed, "seed"), (subsequence, "subsequence")):
        if name == "seed" and v is None:
            continue
        if isinstance(v, bool) or not isinstance(v, int) or not 0 <= v <= _U64:
            raise ValueError(f"{name} must be an integer in 0 .. 2^64 - 1{' or None' if name == 'seed' else ''}, got {v!r}")
    if generator is not None and not (isinstance(generator, torch.Generator) and generator.device.type == "cpu"):
        raise ValueError(f"generator must be None or a CPU torch.Generator, got {generator!r}")


class _BiasDropoutAdd(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, bias, residual, T, scale, seed, subsequence, act):
        D = x.shape[-1]
        rows = x.numel() // D
        out = torch.empty_like(x)
        if rows > 0:
            with torch.cuda.device(x.device):
                hip.call("nova_bias_dropout_add", x.data_ptr(), hip.dtype_code(x.dtype), bias.data_ptr() if bias is not None else None,
                         residual.data_ptr() if residual is not None else None, out.data_ptr(), rows, D, 0, T, scale, seed, subsequence, act,
                         hip.stream_ptr())
            stats["forward_launches"] += 1
        if act == ACT_RELU:
            ctx.save_for_backward(out)  # the next F.linear holds it anyway; without an activation nothing but Python numbers
        ctx.mask = (T, scale, seed, subsequence, act)
        ctx.set_materialize_grads(False)
        return out

    @staticmethod
    @once_differentiable
    def backward(ctx, g):
        T, scale, seed, subsequence, act = ctx.mask
        want_x, want_b, want_r = ctx.needs_input_grad[:3]
        if g is None:
            return (None,) * 8
        gx = gb = None
        if want_x or want_b:
            out = ctx.saved_tensors[0] if act == ACT_RELU else None
            gc = g.contiguous()
            D = g.shape[-1]
            rows = g.numel() // D
            chunks = _chunks(rows, DROPOUT_CHUNK)
            gx = torch.empty_like(gc) if want_x else None  # in the tensor's own dtype, rounded once by the kernel
            parts = torch.empty(chunks, D, dtype=torch.float32, device=g.device) if want_b else None
            with torch.cuda.device(g.device):
                stream = hip.stream_ptr()
                if rows > 0:
                    hip.call("nova_bias_dropout_add_bwd", gc.data_ptr(), out.data_ptr() if out is not None else None, hip.dtype_code(gc.dtype),
                             gx.data_ptr() if want_x else None, parts.data_ptr() if want_b else None, rows, D, 0, T, scale, seed, subsequence, act,
                             stream)
                    stats["backward_launches"] += 1
                if want_b:  # the chunk rows in ascending order; no row: nothing is launched and the sum is +0
                    gb = _sum_over("nova_pointset_embed_sum_clouds", parts, chunks, (D,), D, stream=stream, stats=stats, key="bias_sum_launches")
        return gx, gb, g if want_r else None, None, None, None, None, None


def bias_dropout_add(x, bias=None, residual=None, p=0.1, training=True, activation=None, seed=None, subsequence=0, generator=None):
    """residual + dropout(act(x + bias), p) from one kernel that reads every operand once: x [..., D] in float32, bfloat16 or
    float16 goes to the kernel as it is (any other floating dtype is cast to float32, and a view that is not contiguous made
    contiguous, by a torch op); residual has x's shape and dtype; bias [D] is cast to float32 by a torch op; either may be
    None, and an absent one is no addition. activation is None or "relu" (the feed-forward's first half; it takes no
    residual). 1 <= D <= 16384. The result has x's dtype: the float32 value rounded once.

    p is a Python real in [0, 1]: an element is dropped with probability floor(p 2^32) / 2^32 and a kept one multiplied by the
    float32 nearest to 1 / (1 - p). training=False is p = 0: the same kernel, everything kept. The mask is Philox4x32-10 at
    (seed, subsequence, the element's flat index), the definition in include/nova_hip.h at nova_bias_dropout_add: a dropped
    element is +0 whatever it held (torch makes a dropped infinity a NaN; this does not). seed and subsequence are integers in
    0 .. 2^64 - 1; seed=None draws one from `generator`, a CPU torch.Generator (None: the global one), with no device work and
    no synchronisation, so torch.manual_seed fixes a training step. When p == 0 or training is False no seed is drawn. Give
    the sites of one step different `subsequence`s if they share a seed.

    Differentiable once in x, bias and residual. The gradients of x (in x's dtype, rounded once) and bias (float32: 128-row
    chunk sums in ascending row order, then the chunks in ascending order) come from the HIP backward, which regenerates the
    mask: nothing but Python numbers is saved without an activation, and the output alone with "relu" (torch's convention: the
    gate is out > 0). The gradient of residual is the incoming gradient itself. A kernel whose outputs no input needs is not
    launched (`stats`). No rows (x.numel() == 0) launches nothing: the output and the gradient of x are empty and the gradient
    of bias is +0. Output and gradients are bitwise the same for every run and every alignment of the storage.

    ValueError, in this order: types, dtypes, shapes, D range, devices, p, activation (and activation with residual),
    seed / subsequence range. NovaHipError for CPU tensors."""
    _dropout_arguments(x, bias, residual, p, activation, seed, subsequence, generator)
    _on_gpu(((x, "x"), (bias, "bias"), (residual, "residual")), "the fused dropout")
    T, scale, seed = mask_numbers(p, training, seed, generator)
    native = lambda t: (t if t.dtype in _NATIVE else t.float()).contiguous() if t is not None else None
    return _BiasDropoutAdd.apply(native(x), bias.float().contiguous() if bias is not None else None, native(residual), T, scale, seed, subsequence,
                                 _ACTIVATIONS[activation])


class BiasDropoutAdd(torch.nn.Module):
    """bias_dropout_add as a module: forward(x, bias=None, residual=None) returns residual + dropout(act(x + bias), p) in
    training mode and residual + act(x + bias) in eval() (p = 0, the same kernel). One of these stands behind each GEMM of the
    reference's encoder layer (transformer_pointcloud_nova.py:433-441, :590-598): dropout1 and dropout2 with the residual,
    and activation="relu" for the feed-forward's first half. The seed comes from the global CPU generator. It runs on a GPU."""

    def __init__(self, p=0.1, activation=None):
        super().__init__()
        if isinstance(p, bool) or not isinstance(p, numbers.Real) or not 0 <= p <= 1:
            raise ValueError(f"p must be a real number in [0, 1], got {p!r}")
        if activation not in _ACTIVATIONS:
            raise ValueError(f"activation must be None or 'relu', got {activation!r}")
        self.p, self.activation = p, activation

    def forward(self, x, bias=None, residual=None):
        return bias_dropout_add(x, bias, residual, p=self.p, training=self.training, activation=self.activation)

    def extra_repr(self):
        return f"p={self.p}, activation={self.activation!r}"
