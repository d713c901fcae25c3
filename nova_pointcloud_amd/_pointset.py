"""What the point-set modules (metrics, losses, sampling, neighbors, clustering) share on the host side: the checks of
point tensors and of the arguments several operations take, the split of a cloud set into launches with the one loop
that sends them out, and the body of the two sampling functions that exist with and without a gradient; and what the fused training ops (point_embed, point_head, encoding, clustering,
dropout) share: their argument checks, their sizing and the sums over the clouds that end their backwards. Private to the
package; metrics re-exports the names its tests and tools use."""
import contextlib
import math

import numpy as np
import torch

from . import hip


def _points(t, name):
    if not (torch.is_tensor(t) and t.is_cuda):
        raise hip.NovaHipError(f"{name}: point-set metrics run on the GPU (got {'a CPU tensor' if torch.is_tensor(t) else type(t).__name__})")
    if t.dim() != 3 or t.shape[-1] != 3:
        raise ValueError(f"{name}: expected [B, n, 3] points, got {tuple(t.shape)}")
    if t.requires_grad and torch.is_grad_enabled():
        # evaluation metrics: the HIP distance kernels have no backward, so a loss built on them would silently carry no gradient
        raise hip.NovaHipError(f"{name}: nova_pointcloud_amd.metrics is evaluation-only (no autograd through the HIP kernels); "
                               "detach the points, or build a training loss on nova_pointcloud_amd.losses")
    return t.detach().float().contiguous()


def _check_clouds(named, letters="S, n", count_range=None, same_clouds=False, same_points=None, same_device=True, finite=True):
    """ValueError for everything about the point tensors `named`, a sequence of (tensor, name), that does not need the GPU,
    in one order, each step over all tensors before the next:
      1. type        every entry is a tensor
      2. shape       [<letters>, 3]
      3. counts      same_clouds: equal cloud counts; same_points (what needs them, for the message): equal point counts;
                     count_range = (kernel name, maximum): 1 .. maximum points per cloud
      4. device      same_device: all on one device
      5. finiteness  finite: no NaN and no infinity
    _points refuses CPU tensors only after this, so all of it holds for CPU tensors too."""
    for t, name in named:
        if not torch.is_tensor(t):
            raise ValueError(f"{name}: expected a tensor [{letters}, 3], got {type(t).__name__}")
    for t, name in named:
        if t.dim() != 3 or t.shape[-1] != 3:
            raise ValueError(f"{name}: expected [{letters}, 3] clouds, got {tuple(t.shape)}")
    names = " and ".join(name for _, name in named)
    if same_clouds and len({t.shape[0] for t, _ in named}) > 1:
        raise ValueError(f"{names} must hold the same number of clouds, got {' and '.join(str(t.shape[0]) for t, _ in named)}")
    if same_points and len({t.shape[1] for t, _ in named}) > 1:
        raise ValueError(f"{same_points} needs equal point counts (got {' and '.join(f'{t.shape[1]} ({name})' for t, name in named)})")
    if count_range is not None:
        kernel, most = count_range
        for t, name in named:
            if not 1 <= t.shape[1] <= most:
                raise ValueError(f"{name}: the {kernel} kernel takes 1 .. {most} points per cloud, got {t.shape[1]}")
    if same_device and len({t.device for t, _ in named}) > 1:
        raise ValueError(f"{names} must be on the same device, got {' and '.join(str(t.device) for t, _ in named)}")
    if finite:
        for t, name in named:
            if not bool(torch.isfinite(t).all()):
                raise ValueError(f"{name}: points must be finite")


def _clouds(named, **checks):
    """_check_clouds, then _points for each (tensor, name)."""
    _check_clouds(named, **checks)
    return [_points(t, name) for t, name in named]


def _at_least_one(v, name):
    if not isinstance(v, int) or isinstance(v, bool) or v < 1:
        raise ValueError(f"{name} must be an integer >= 1, got {v!r}")
    return v


def _check_clamp(clamp, name="clamp"):
    if clamp is not None and not (isinstance(clamp, (int, float)) and not isinstance(clamp, bool) and 0 < clamp < math.inf):
        raise ValueError(f"{name} must be None or a positive finite number, got {clamp!r}")
    return (-float(clamp), float(clamp)) if clamp is not None else (-math.inf, math.inf)


ASSIGNMENT_MODES = ("host", "device")


def _assignment_mode(assignment):
    if assignment not in ASSIGNMENT_MODES:
        raise ValueError(f"assignment must be one of {ASSIGNMENT_MODES}, got {assignment!r}")
    return assignment == "device"


def _clouds_per_launch(given, default, most=None):
    """max_clouds_per_launch as given (ValueError unless an integer >= 1), or the operation's default; at most `most`."""
    per = max(1, default) if given is None else _at_least_one(given, "max_clouds_per_launch")
    return per if most is None else min(per, most)


def _launches(n_clouds, per, name="max_clouds_per_launch"):
    """(first cloud, cloud count) of the launches that send `n_clouds` clouds out at most `per` at a time. ValueError, at the
    call and not at the first step, unless per is an integer >= 1."""
    _at_least_one(per, name)
    return [(s0, min(per, n_clouds - s0)) for s0 in range(0, n_clouds, per)]


def _launching(device, n_clouds, per):
    """The launch loop: `for stream, s0, count in _launching(x.device, S, per)` runs its body once per launch of _launches,
    with `device` the current device and `stream` its current stream, read once. Arguments sliced per cloud go in as
    _at(t, s0). The split is made here, at the call (so _launches' ValueError comes before whatever the caller allocates
    between the call and the loop); the device is entered at the first step and left after the last one, or when an
    exception in the body drops the loop."""
    spans = _launches(n_clouds, per)

    def steps():
        with torch.cuda.device(device):
            stream = hip.stream_ptr()
            for s0, count in spans:
                yield stream, s0, count

    return steps()


def _at(t, s0):
    """The device address of cloud s0 of the per-cloud tensor t; NULL for an argument that is not there (None)."""
    return t[s0].data_ptr() if t is not None else None


# ---- the fused training ops (point_embed, point_head, encoding, clustering, dropout): their argument checks, each a step of
# its own over all of `named`, a sequence of (tensor, name), so a module can put a check of its own between two of them

MAX_CLOUDS_PER_CALL = 65535  # clouds go in grid.y


def _all_tensors(named):
    for t, name in named:
        if not torch.is_tensor(t):
            raise ValueError(f"{name}: expected a tensor, got {type(t).__name__}")


def _all_floating(named):
    for t, name in named:
        if not t.is_floating_point():
            raise ValueError(f"{name}: expected a floating dtype, got {t.dtype}")


def _same_device(named):
    """Every entry is on the device of the first."""
    first, lead = named[0]
    for t, name in named[1:]:
        if t.device != first.device:
            raise ValueError(f"{lead} and {name} must be on the same device, got {first.device} and {t.device}")


def _on_gpu(named, what):
    """NovaHipError for a CPU tensor (an entry that is None is skipped); `what` is what runs on the GPU, "the point head"."""
    for t, name in named:
        if t is not None and not t.is_cuda:
            raise hip.NovaHipError(f"{name}: {what} runs on the GPU (got a CPU tensor)")


def _chunks(N, chunk):
    return (N + chunk - 1) // chunk


def _budget_clouds_per_launch(budget, cost):
    """The default clouds per launch: what fits the module's per-launch budget at `cost` per cloud, 1 .. MAX_CLOUDS_PER_CALL."""
    return max(1, min(budget // cost, MAX_CLOUDS_PER_CALL))


def _allocator(n_clouds, device):
    """new(*shape, dtype=torch.float32) for what a backward's launches write. An empty cloud set launches nothing, so nothing
    writes a sum over the clouds: there it starts from +0 and stays there."""
    make = torch.empty if n_clouds > 0 else torch.zeros
    return lambda *shape, dtype=torch.float32: make(*shape, dtype=dtype, device=device)


@contextlib.contextmanager
def _launch_stream(device, n_clouds, per):
    """The launch loop of a backward whose sums over the clouds follow it on the same device and stream (_launching leaves
    the device after the last step): `with _launch_stream(x.device, S, per) as (stream, spans)` holds `device` current, with
    `stream` its current stream, read once, and `spans` what _launches gives."""
    spans = _launches(n_clouds, per)
    with torch.cuda.device(device):
        yield hip.stream_ptr(), spans


def _sum_over(entry, parts, count, out_shape, *extra, stream, stats, key):
    """float32 `out_shape`: the `count` leading slices of `parts` added from +0 in ascending order by the entry point
    `entry`(parts, out, count, *extra, stream), counted in stats[key]. count == 0 launches nothing and gives +0."""
    out = (torch.empty if count > 0 else torch.zeros)(out_shape, dtype=torch.float32, device=parts.device)
    if count > 0:
        hip.call(entry, parts.data_ptr(), out.data_ptr(), count, *extra, stream)
        stats[key] += 1
    return out


INTERP_MAX_POINTS = 65536  # == NOVA_INTERP_MAX_POINTS of include/nova_hip.h
INTERP_MAX_CHANNELS = 8  # == NOVA_INTERP_MAX_CHANNELS of include/nova_hip.h
# (query, source) pairs (clouds x queries x sources) per launch, ~8.6e9. Re-derived from the measured launches of
# tools/interp_bench.py (profiles/interp_bench.json): 32 x 1024 queries on 2048 sources, 512 workgroups, run in 0.21 ms
# (3.1e11 pairs/s) and 7500 queries on 15 000 sources, 118 workgroups on 256 compute units, in 0.58 ms, the longest single
# launch under this cap (1.9e11 pairs/s). Both are too small to fill the chip, so they are far below the instruction-count
# estimate (about 46 vector issue slots per pair: ~1.7e12 pairs/s), and a full launch has not been timed; at the better of
# the two measured rates 2^33 pairs are 28 ms, at the estimate 5 ms. A cloud is at most 2^32 pairs, so a launch holds at
# least two (distance-weighted interpolation).
_INTERP_PAIRS_PER_LAUNCH = 1 << 33


def _interp_scale(temperature):
    """log2(e) / temperature as the float32 the kernel takes. ValueError unless temperature is a real number > 0 (inf
    allowed: the plain mean) and that quotient is finite in float32."""
    if isinstance(temperature, bool) or not isinstance(temperature, (int, float)) or not temperature > 0:
        raise ValueError(f"temperature must be a real number > 0 (inf for the plain mean), got {temperature!r}")
    with np.errstate(over="ignore"):
        scale = float(np.float32(np.float64(math.log2(math.e)) / np.float64(temperature)))  # one division in float64, one rounding
    if not math.isfinite(scale):
        raise ValueError(f"temperature {temperature!r} is too small: log2(e) / temperature is not finite in float32")
    return scale


def _interp_arguments(queries, points, values):
    """_check_clouds and the checks of `values` that do not need the GPU. Returns the channel count C."""
    _check_clouds([(queries, "queries"), (points, "points")], letters="S, N", count_range=("interpolation", INTERP_MAX_POINTS),
                  same_clouds=True)
    if values is None:
        return 3
    if not torch.is_tensor(values):
        raise ValueError(f"values: expected a tensor [S, N, C], got {type(values).__name__}")
    S, N = points.shape[0], points.shape[1]
    if values.dim() != 3 or tuple(values.shape[:2]) != (S, N):
        raise ValueError(f"values: expected [{S}, {N}, C] (one row per source point), got {tuple(values.shape)}")
    if not 1 <= values.shape[2] <= INTERP_MAX_CHANNELS:
        raise ValueError(f"values: the interpolation kernel takes 1 .. {INTERP_MAX_CHANNELS} channels, got {values.shape[2]}")
    if not values.dtype.is_floating_point:
        raise ValueError(f"values: expected a floating-point tensor, got {values.dtype}")
    if values.device != points.device:
        raise ValueError(f"values and points must be on the same device, got {values.device} and {points.device}")
    if not bool(torch.isfinite(values).all()):
        raise ValueError("values: values must be finite")
    return values.shape[2]


def _cyclic(points, target_size):
    """points [S, N, 3] repeated along the point axis and cut to target_size (pure torch)."""
    return points.repeat(1, target_size // points.shape[1] + 1, 1)[:, :target_size]


def _sampling_arguments(points, name, target_size, temperature):
    _check_clouds([(points, name)], letters="S, N", finite=False)
    _at_least_one(target_size, "target_size")
    if points.shape[1] < 1:
        raise ValueError(f"{name}: empty clouds (0 points)")
    _interp_scale(temperature)


def _feature_aware_interpolation(interpolate, points, target_size, temperature, generator):
    """The body of feature_aware_interpolation, on the caller's kernel_interpolate."""
    _sampling_arguments(points, "points", target_size, temperature)
    N = points.shape[1]
    if N <= target_size:
        return _cyclic(points, target_size)
    perm = torch.randperm(N, generator=generator)[:target_size].to(points.device)
    return interpolate(points[:, perm], points, temperature=temperature)


def _adaptive_sampling(interpolate, farthest_point_sample, subset, target_size, temperature, generator):
    """The body of adaptive_sampling, on the caller's kernel_interpolate and farthest_point_sample(subset, N)."""
    _sampling_arguments(subset, "subset", target_size, temperature)
    S, N = subset.shape[0], subset.shape[1]
    if N == target_size:
        return subset
    if N > target_size:
        return _feature_aware_interpolation(interpolate, subset, target_size, temperature, generator)
    order = farthest_point_sample(subset, N)[:, torch.arange(target_size, device=subset.device) % N]
    return torch.gather(subset, 1, order[:, :, None].expand(S, target_size, 3))
