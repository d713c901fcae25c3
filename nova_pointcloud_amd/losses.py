"""Differentiable Chamfer-type and EMD training losses on MI355X: what the reference's PointCloudLoss
(train_newloss.py:395-555) adds to the diffusion loss, without the [B, N, M] torch.cdist matrix that PyTorch keeps alive for
the backward.

One primitive carries the Chamfer-type gradients: nearest_match, the distance from every point of x to its nearest point of y with the
index of that point, and a backward that recomputes the matched pairs and gathers gy in a fixed order (csrc/nearest_match.hip;
the definition, ties and zero distances included, is in include/nova_hip.h at nova_pointset_nearest_match). Everything else is
plain torch on its [B, N] output:
  dist_chamfer, chamfer_loss          distChamfer / robust_chamfer_distance   train_newloss.py:316-349, 381-384
  edge_consistency_loss               _compute_edge_consistency               train_newloss.py:449-457
  autoregressive_consistency_loss                                             train_newloss.py:426-447
  PointCloudLoss                                                              train_newloss.py:395-555
The values are those of nova_pointcloud_amd.metrics (same kernels' expression, bit for bit); metrics stays evaluation-only.
A second primitive carries the EMD's: matched_distance, the distances of the pairs a given permutation matches, with a backward
that gathers both gradients through the permutation and its inverse (csrc/matched.hip; include/nova_hip.h at
nova_pointset_matched_dist). On it
  emd_loss                            emd_approx / robust_emd with a gradient   train_newloss.py:352-377, 418-424
the mean matched distance under the optimal assignment (metrics.optimal_assignment on the GPU, or scipy), differentiated with
the assignment held fixed. The EMD term of PointCloudLoss is a constant by default, as in the reference, whose emd_approx
goes through numpy; PointCloudLoss(emd_gradient=True) puts emd_loss in its place.
GPU tensors only: NovaHipError for CPU tensors or a missing library. Results are bitwise reproducible: the same for every
launch split, every position in the batch and every run, forward and backward."""
import math

import numpy as np
import torch
from torch import nn
from torch.autograd.function import once_differentiable

from . import hip, metrics
from ._pointset import _assignment_mode, _at, _check_clamp, _check_clouds, _clouds_per_launch, _launching

# forward launches of nova_pointset_nearest_match and of nova_pointset_matched_dist since import
stats = {"nearest_match_launches": 0, "matched_dist_launches": 0}

# (query, target) pairs per launch, ~1.7e10: the forward is about 9 vector issues a pair and the backward's gather 7
# (csrc/nearest_match.hip), a few milliseconds a launch by that count; a launch also holds at most 65535 clouds (grid.y)
_PAIRS_PER_LAUNCH = 1 << 34
_MAX_CLOUDS_PER_LAUNCH = 65535


class _NearestMatch(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, y, lo, hi, unit, per):
        B, N, M = x.shape[0], x.shape[1], y.shape[1]
        d = torch.empty(B, N, dtype=torch.float32, device=x.device)
        idx = torch.empty(B, N, dtype=torch.int32, device=x.device)
        if B * N > 0:
            for stream, s0, count in _launching(x.device, B, per):
                hip.call("nova_pointset_nearest_match", _at(x, s0), _at(y, s0), _at(d, s0), _at(idx, s0), count, N, M, lo, hi, unit, stream)
                stats["nearest_match_launches"] += 1
        ctx.save_for_backward(x, y, idx)
        ctx.args = (lo, hi, unit, per)
        ctx.mark_non_differentiable(idx)
        return d, idx

    @staticmethod
    @once_differentiable
    def backward(ctx, g, _):
        x, y, idx = ctx.saved_tensors
        lo, hi, unit, per = ctx.args
        B, N, M = x.shape[0], x.shape[1], y.shape[1]
        g = g.float().contiguous()
        gx = torch.empty_like(x)
        gy = torch.empty_like(y) if B * N > 0 else torch.zeros_like(y)
        if B * N > 0:
            for stream, s0, count in _launching(x.device, B, per):
                hip.call("nova_pointset_nearest_match_bwd", _at(x, s0), _at(y, s0), _at(idx, s0), _at(g, s0), _at(gx, s0), _at(gy, s0),
                         count, N, M, lo, hi, unit, stream)
        return gx, gy, None, None, None, None


def _nearest_match_arguments(x, y, clamp, unit_norm, return_indices, max_clouds_per_launch):
    """_check_clouds and the operation's own arguments; everything here holds for CPU tensors too. Returns
    (lo, hi, clouds per launch)."""
    _check_clouds(((x, "x"), (y, "y")), letters="B, N", same_clouds=True)
    for t, name in ((x, "x"), (y, "y")):
        if not t.is_floating_point():
            raise ValueError(f"{name}: expected floating-point points, got {t.dtype}")
    if y.shape[1] < 1:
        raise ValueError(f"y: every cloud needs at least one point to match to, got {tuple(y.shape)}")
    lo, hi = _check_clamp(clamp)
    for flag, name in ((unit_norm, "unit_norm"), (return_indices, "return_indices")):
        if not isinstance(flag, bool):
            raise ValueError(f"{name} must be a bool, got {flag!r}")
    per = _clouds_per_launch(max_clouds_per_launch, _PAIRS_PER_LAUNCH // max(1, x.shape[1] * y.shape[1]), _MAX_CLOUDS_PER_LAUNCH)
    return lo, hi, per


def nearest_match(x, y, clamp=None, unit_norm=False, return_indices=False, max_clouds_per_launch=None):
    """d float32 [B, N]: the Euclidean distance from every point of x [B, N, 3] to its nearest point of y [B, M, 3], cloud by
    cloud, differentiable in x and in y. return_indices=True adds idx int64 [B, N], the index of that point. GPU tensors of
    any floating dtype: the cast to float32 is a torch op, so a bf16 or f16 input gets a gradient of its own dtype, the
    float32 gradient rounded once.

    `clamp` (None: off) clamps every coordinate to [-clamp, clamp] first; unit_norm=True then scales every point to unit
    length (x / max(|x|, 1e-8)): the point map of metrics.nn_dist, whose output d equals bit for bit. The nearest point is
    the smallest key (float32 squared distance in exact differences, index): a tie goes to the lowest index.

    Gradient (include/nova_hip.h, nova_pointset_nearest_match_bwd): the derivative of |p(x_i) - p(y_idx_i)| with the match
    held fixed, pulled back through the clamp (inclusive bounds, as torch.clamp) and the normalisation (torch's gradient of
    c / clamp_min(|c|, 1e-8)); a coincident pair (distance exactly 0) contributes no gradient and no NaN. y's gradient is
    the sum over the points matched to it, added in increasing i by one thread: no atomics, so d, idx and both gradients are
    bitwise the same for every `max_clouds_per_launch`, every position in the batch and every run. No [N, M] array exists
    in either pass."""
    lo, hi, per = _nearest_match_arguments(x, y, clamp, unit_norm, return_indices, max_clouds_per_launch)
    for t, name in ((x, "x"), (y, "y")):
        if not t.is_cuda:
            raise hip.NovaHipError(f"{name}: the point-set losses run on the GPU (got a CPU tensor)")
    d, idx = _NearestMatch.apply(x.float().contiguous(), y.float().contiguous(), lo, hi, 1 if unit_norm else 0, per)
    return (d, idx.long()) if return_indices else d


# points per launch of the matched-pair kernels: a few dozen bytes a point (csrc/matched.hip), so 2^26 points are ~2.5 GB of
# traffic, about a millisecond a launch by that count; a launch also holds at most 65535 clouds (grid.y)
_MATCHED_POINTS_PER_LAUNCH = 1 << 26


class _MatchedDistance(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, y, idx, inv, lo, hi, floor, per):
        B, n = x.shape[0], x.shape[1]
        d = torch.empty(B, n, dtype=torch.float32, device=x.device)
        if B * n > 0:
            for stream, s0, count in _launching(x.device, B, per):
                hip.call("nova_pointset_matched_dist", _at(x, s0), _at(y, s0), _at(idx, s0), _at(d, s0), count, n, lo, hi, floor, stream)
                stats["matched_dist_launches"] += 1
        ctx.save_for_backward(x, y, idx, inv)
        ctx.args = (lo, hi, floor, per)
        return d

    @staticmethod
    @once_differentiable
    def backward(ctx, g):
        x, y, idx, inv = ctx.saved_tensors
        lo, hi, floor, per = ctx.args
        B, n = x.shape[0], x.shape[1]
        g = g.float().contiguous()
        gx, gy = torch.empty_like(x), torch.empty_like(y)
        if B * n > 0:
            for stream, s0, count in _launching(x.device, B, per):
                hip.call("nova_pointset_matched_dist_bwd", _at(x, s0), _at(y, s0), _at(idx, s0), _at(inv, s0), _at(g, s0), _at(gx, s0),
                         _at(gy, s0), count, n, lo, hi, floor, stream)
        return gx, gy, None, None, None, None, None, None


def _check_pairs(x, y, names, what):
    """_check_clouds for two cloud sets that are matched point to point, and the floating dtype."""
    _check_clouds(((x, names[0]), (y, names[1])), letters="B, n", same_clouds=True, same_points=what)
    for t, name in ((x, names[0]), (y, names[1])):
        if not t.is_floating_point():
            raise ValueError(f"{name}: expected floating-point points, got {t.dtype}")


def _matched_distance_arguments(x, y, index, clamp, floor, max_clouds_per_launch):
    """_check_clouds and the operation's own arguments, the permutation check included; everything here holds for
    CPU tensors too. Returns (lo, hi, floor, clouds per launch)."""
    _check_pairs(x, y, ("x", "y"), "the matched distance")
    B, n = x.shape[0], x.shape[1]
    if not torch.is_tensor(index) or index.dtype != torch.int64 or tuple(index.shape) != (B, n):
        got = f"{index.dtype} {tuple(index.shape)}" if torch.is_tensor(index) else type(index).__name__
        raise ValueError(f"index: expected an int64 tensor [{B}, {n}] (the point of y matched to every point of x), got {got}")
    if index.device != x.device:
        raise ValueError(f"index must be on the device of x and y, got {index.device} and {x.device}")
    lo, hi = _check_clamp(clamp)
    if not (isinstance(floor, (int, float)) and not isinstance(floor, bool) and 0 <= floor < math.inf):
        raise ValueError(f"floor must be a finite number >= 0, got {floor!r}")
    per = _clouds_per_launch(max_clouds_per_launch, _MATCHED_POINTS_PER_LAUNCH // max(1, n), _MAX_CLOUDS_PER_LAUNCH)
    if B * n > 0:  # a permutation sorts to 0 .. n-1; this also covers the range
        bad = (index.sort(dim=1).values != torch.arange(n, device=index.device)).any(dim=1)
        if bool(bad.any()):
            raise ValueError(f"index: every cloud needs a permutation of 0 .. {n - 1}; cloud {int(torch.nonzero(bad)[0])} is the first "
                             "that holds none")
    return lo, hi, float(floor), per


def matched_distance(x, y, index, clamp=None, floor=0.0, max_clouds_per_launch=None):
    """d float32 [B, n]: d[b, i] = max(|c(x[b, i]) - c(y[b, index[b, i]])|, floor), the Euclidean distance of the pairs that the
    permutation `index` (int64 [B, n], a permutation of 0 .. n-1 per cloud; ValueError naming the first cloud where it is
    not) matches between x [B, n, 3] and y [B, n, 3], differentiable in x and in y. GPU tensors of any floating dtype: the cast
    to float32 is a torch op, so a bf16 or f16 input gets a gradient of its own dtype, the float32 gradient rounded once.

    `clamp` (None: off) clamps every coordinate to [-clamp, clamp] first (c above). Before the floor, d[b, i] is bit for bit
    metrics.pairwise_dist(x, y, clamp)[b, i, index[b, i]], the cost the assignment was solved on.

    Gradient (include/nova_hip.h, nova_pointset_matched_dist_bwd): that of the distance with `index` held fixed, through
    clamp_min(floor) (zero below the floor) and the clamp (inclusive bounds, as torch.clamp); a coincident pair (distance
    exactly 0) contributes no gradient and no NaN. x's gradient is read through index and y's through its inverse, which is
    formed here with scatter_ and kept for the backward: both are gathers, one thread per output row, no atomics, so d and
    both gradients are bitwise the same for every `max_clouds_per_launch`, every position in the batch and every run."""
    lo, hi, floor, per = _matched_distance_arguments(x, y, index, clamp, floor, max_clouds_per_launch)
    for t, name in ((x, "x"), (y, "y")):
        if not t.is_cuda:
            raise hip.NovaHipError(f"{name}: the point-set losses run on the GPU (got a CPU tensor)")
    B, n = index.shape
    rows = torch.arange(n, dtype=torch.int32, device=index.device).expand(B, n)
    inv = torch.empty(B, n, dtype=torch.int32, device=index.device).scatter_(1, index, rows)
    return _MatchedDistance.apply(x.float().contiguous(), y.float().contiguous(), index.int().contiguous(), inv, lo, hi, floor, per)


EMD_FLOOR = 1e-8  # the floor of the reference's cost matrix (train_newloss.py:358)


def emd_loss(pred, target, clamp=2.0, assignment="device", max_rounds=None, rounds_per_launch=None, return_assignment=False):
    """The earth mover's distance of every sample as a training loss: tensor float32 [B], per sample the mean over the points
    of matched_distance(pred, target, index, clamp, floor=1e-8), where index is the optimal assignment between the DETACHED
    clouds pred [B, n, 3] and target [B, n, 3] under the same clamp (equal point counts; 2.0 is the clamp of the reference's
    emd_approx, train_newloss.py:352-377). return_assignment=True adds index, int64 [B, n].
      assignment="device"   metrics.optimal_assignment(pred, target, clamp=clamp, max_rounds, rounds_per_launch): the auction
                            kernel, 1 .. 4096 points, its mean within ASSIGN_QUANTUM = 2^-18 of the optimum; its errors
                            (point count, max_rounds used up, the integer range) propagate
      assignment="host"     scipy's linear_sum_assignment on np.maximum(metrics.pairwise_dist(pred, target, clamp), 1e-8),
                            exactly as metrics.emd_approx does; max_rounds and rounds_per_launch are not looked at
    Either way the value and the gradient come from csrc/matched.hip.

    The gradient holds the assignment fixed. The optimal permutation is piecewise constant in the points, so this is the
    gradient of the EMD wherever it has one (the convention of the auction-based EMD losses in the literature): every pred
    point is pulled along the unit vector to its partner, weighted 1 / n, and nothing flows through the choice of partner.

    The value is metrics.emd_approx(pred, target, assignment)'s up to rounding: the matched distances here are the float32
    expression of pairwise_dist (fused multiply-adds, the distances "host" optimises bit for bit), "device" of emd_approx
    squares and sums in plain torch ops (a few ulp per term apart), and the n terms of a sample are summed by torch.mean on
    the GPU here and by numpy on the host there: two float32 summation orders of the same terms."""
    _check_pairs(pred, target, ("pred", "target"), "the EMD")
    if pred.shape[1] < 1:
        raise ValueError(f"pred: every cloud needs at least one point, got {tuple(pred.shape)}")
    _check_clamp(clamp)
    device = _assignment_mode(assignment)
    if not isinstance(return_assignment, bool):
        raise ValueError(f"return_assignment must be a bool, got {return_assignment!r}")
    p, t = pred.detach(), target.detach()
    if device:
        index = metrics.optimal_assignment(p, t, clamp=clamp, max_rounds=max_rounds, rounds_per_launch=rounds_per_launch)[0]
    else:
        from scipy.optimize import linear_sum_assignment

        cost = np.maximum(metrics.pairwise_dist(p, t, math.inf if clamp is None else clamp).cpu().numpy(), EMD_FLOOR)
        index = torch.from_numpy(np.stack([linear_sum_assignment(c)[1] for c in cost]).astype(np.int64)).to(pred.device)
    value = matched_distance(pred, target, index, clamp, floor=EMD_FLOOR).mean(dim=1)
    return (value, index) if return_assignment else value


def _through_log(d):
    return torch.log(d.clamp_min(1e-8) + 1e-8).clamp(-10, 10).exp().mean()


def dist_chamfer(a, b):
    """(dl, dr) of train_newloss.py:316-349 with gradient: points clamped to +-1 and scaled to unit norm, the nearest
    distance of each direction floored at 1e-8 and passed through log(d + 1e-8) clamped to [-10, 10] and exp. Min and the
    monotone maps commute, in value and in which entry receives the gradient, so this is the reference's
    log_dist_matrix.min(...) without the matrix. The values are metrics.distChamfer's, bit for bit."""
    return _through_log(nearest_match(a, b, 1.0, True)), _through_log(nearest_match(b, a, 1.0, True))


def chamfer_loss(pred, target):
    """(dl + dr) / 2 of dist_chamfer: the reference's robust_chamfer_distance (train_newloss.py:381-384, 408-416)."""
    dl, dr = dist_chamfer(pred, target)
    return (dl.mean() + dr.mean()) / 2


def edge_consistency_loss(subset1, subset2):
    """The mean distance from the points of subset1 [B, N, 3] to their nearest points of subset2 [B, M, 3], no clamp and no
    normalisation: for each cloud, torch.cdist(subset1[b], subset2[b]).min(dim=1) averaged (train_newloss.py:449-457)."""
    return nearest_match(subset1, subset2).mean()


def autoregressive_consistency_loss(generated_subsets, target_subsets):
    """The mean of edge_consistency_loss(generated_subsets[i], generated_subsets[j]) over all pairs i < j
    (train_newloss.py:426-447); tensor 0.0 when either list is empty. As in the reference, target_subsets is only looked at
    for that emptiness check: the term measures the generated subsets against each other.

    Pairs with the same point counts (N, M) are stacked along the batch and go out together, so the number of forward
    launches is the number of distinct (N, M) among the pairs, not the number of pairs: twenty subsets of a 2048-point
    cloud, nineteen of 102 points and one of 110, are 190 pairs in two launches."""
    if not generated_subsets or not target_subsets:
        return torch.tensor(0.0, device=generated_subsets[0].device if generated_subsets else torch.device("cpu"))
    subsets = list(generated_subsets)
    _check_clouds([(s, f"generated_subsets[{k}]") for k, s in enumerate(subsets)], letters="B, n", same_clouds=True)
    groups = {}
    for i in range(len(subsets) - 1):
        for j in range(i + 1, len(subsets)):
            groups.setdefault((subsets[i].shape[1], subsets[j].shape[1]), []).append((i, j))
    num_pairs = sum(len(pairs) for pairs in groups.values())
    if num_pairs == 0:
        return torch.tensor(0.0, device=subsets[0].device)
    total = 0.0
    for pairs in groups.values():
        d = nearest_match(torch.cat([subsets[i] for i, _ in pairs], dim=0), torch.cat([subsets[j] for _, j in pairs], dim=0))
        total = total + d.reshape(len(pairs), -1).mean(dim=1).sum()
    return total / num_pairs


class PointCloudLoss(nn.Module):
    """The reference's PointCloudLoss (train_newloss.py:395-555), same constructor and forward signature and the same terms
    in the same order:
      diffusion_weight * mse(noise_pred, noise_target)                     (0.1 in place of a NaN / inf value)
      pred_points / target_points cut to the smaller point count by a random permutation
      + cd_weight * chamfer_loss(pred_points, target_points)               (dropped when NaN / inf)
      + emd_weight * metrics.robust_emd of the DETACHED points             (a constant, as in the reference; dropped when NaN / inf)
        emd_gradient=True: emd_weight * emd_loss(pred_points, target_points).mean() instead, which takes part in the backward
      + autoregressive_weight * autoregressive_consistency_loss(...)       (when both subset lists are given; dropped when NaN / inf)
      the diffusion term alone when the total is NaN / inf
    use_only_diffusion=True, or points not given, returns after the first term. edge_alignment_weight is stored and, as in
    the reference, enters no term. emd_assignment is metrics.robust_emd's `assignment` ("host": scipy, "device": the auction
    kernel); emd_gradient=True uses it for emd_loss's `assignment` and differentiates the term with the assignment held fixed
(emd_loss: the same value up to rounding, and now a gradient that emd_weight scales). emd_gradient=False, the default, is the
reference's behaviour: the optimiser never sees emd_weight. There is no wandb logging: the components of the last call are in self.last_components, a dict of floats.
    DEVIATION, on purpose: the reference swallows every exception of a geometric term and goes on with 0; here an error is
    an error."""

    def __init__(self, scheduler, cd_weight=0.1, emd_weight=0.05, diffusion_weight=1.0, autoregressive_weight=0.2,
                 edge_alignment_weight=0.1, emd_assignment="host", emd_gradient=False):
        super().__init__()
        _assignment_mode(emd_assignment)
        if not isinstance(emd_gradient, bool):
            raise ValueError(f"emd_gradient must be a bool, got {emd_gradient!r}")
        self.scheduler = scheduler
        self.cd_weight = cd_weight
        self.emd_weight = emd_weight
        self.diffusion_weight = diffusion_weight
        self.autoregressive_weight = autoregressive_weight
        self.edge_alignment_weight = edge_alignment_weight
        self.emd_assignment = emd_assignment
        self.emd_gradient = emd_gradient
        self.last_components = {}

    def forward(self, noise_pred, noise_target, pred_points=None, target_points=None, generated_subsets=None, target_subsets=None,
                use_only_diffusion=False):
        finite = lambda t: bool(torch.isfinite(t).all())
        value = lambda t: float(t.detach())
        if not finite(noise_pred):
            noise_pred = torch.clamp(noise_pred, -2.0, 2.0)
        if not finite(noise_target):
            noise_target = torch.clamp(noise_target, -2.0, 2.0)
        diffusion_loss = nn.functional.mse_loss(noise_pred, noise_target, reduction="mean")
        if not finite(diffusion_loss):
            diffusion_loss = torch.tensor(0.1, device=noise_pred.device, dtype=noise_pred.dtype)
        total_loss = self.diffusion_weight * diffusion_loss
        if use_only_diffusion or pred_points is None or target_points is None:
            self.last_components = {"diffusion_loss": value(diffusion_loss), "total_loss": value(total_loss)}
            return total_loss

        if pred_points.shape[1] != target_points.shape[1]:
            min_points = min(pred_points.shape[1], target_points.shape[1])
            if pred_points.shape[1] > min_points:
                pred_points = pred_points[:, torch.randperm(pred_points.shape[1], device=pred_points.device)[:min_points], :]
            if target_points.shape[1] > min_points:
                target_points = target_points[:, torch.randperm(target_points.shape[1], device=target_points.device)[:min_points], :]
        zero = torch.tensor(0.0, device=pred_points.device, dtype=pred_points.dtype)

        cd_loss = chamfer_loss(pred_points, target_points)
        if finite(cd_loss):
            total_loss = total_loss + self.cd_weight * cd_loss
        else:
            cd_loss = zero
        if self.emd_gradient:
            emd = emd_loss(pred_points, target_points, assignment=self.emd_assignment).mean()
        else:
            emd = metrics.robust_emd(pred_points.detach(), target_points.detach(), assignment=self.emd_assignment)
        if finite(emd):
            total_loss = total_loss + self.emd_weight * emd
        else:
            emd = zero
        autoregressive_loss = zero
        if generated_subsets is not None and target_subsets is not None:
            autoregressive_loss = autoregressive_consistency_loss(generated_subsets, target_subsets)
            if finite(autoregressive_loss):
                total_loss = total_loss + self.autoregressive_weight * autoregressive_loss
        if not finite(total_loss):
            total_loss = diffusion_loss
        self.last_components = {"diffusion_loss": value(diffusion_loss), "cd_loss": value(cd_loss), "emd_loss": value(emd),
                                "autoregressive_loss": value(autoregressive_loss), "total_loss": value(total_loss)}
        return total_loss
