"""Farthest point sampling of a chair-sized test set (662 clouds): the HIP kernel (csrc/fps.hip through
metrics.farthest_point_sample) against a batched torch form (the same mind update and argmax as n steps of torch ops over
[S, N]), in one process, at the two shapes of the evaluation path:

    15000 -> 2048    a published reference set (15 000 points per shape) brought to the generated clouds' count
    2048 -> 512      generated clouds brought to a small EMD size

    python3 tools/fps_bench.py [--out FILE]           both paths, one JSON line
    python3 tools/fps_bench.py --hip-only             the HIP launches only, for a kernel-time run:
    rocprofv3 --kernel-trace --stats --output-format csv -d DIR -o fps -- python3 tools/fps_bench.py --hip-only

Both outputs are checked by the validity rule of tests/test_pointset_fps.py: the index sequence is replayed in float64 and
every choice must be a maximum of mind up to 1e-6 relative (the two forms may then still differ where float32 rounds a
near-tie differently; the share of equal indices is reported, not bounded). Both are timed with device events after a
warm-up: the best of --reps repetitions and the spread (max - min) / min. The kernel is latency-bound (n dependent steps
per cloud), so there is no roofline: the figure of merit is the time of one step, reported as nanoseconds per selected
point per cloud = kernel time x resident workgroups / (S x n).
"""
import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from nova_pointcloud_amd import metrics  # noqa: E402
from pointset_bench_common import ball_clouds, timed  # noqa: E402

SHAPES = ((15000, 2048), (2048, 512))
REL = 1e-6


def torch_fps(x, n):
    S, N = x.shape[:2]
    rows = torch.arange(S, device=x.device)
    mind = torch.full((S, N), float("inf"), device=x.device)
    idx = torch.zeros(S, n, dtype=torch.int64, device=x.device)
    cur = idx[:, 0]
    for i in range(1, n):
        mind = torch.minimum(mind, (x - x[rows, cur][:, None, :]).square().sum(-1))
        cur = mind.argmax(dim=1)
        idx[:, i] = cur
    return idx


def worst_shortfall(x, idx, chunk=64):
    """Largest (max_j mind64[j] - mind64[idx[i]]) / max_j mind64[j] over all clouds and steps of the float64 replay."""
    worst = torch.zeros((), dtype=torch.float64, device=x.device)
    for c0 in range(0, x.shape[0], chunk):
        x64, ids = x[c0:c0 + chunk].double(), idx[c0:c0 + chunk]
        rows = torch.arange(x64.shape[0], device=x.device)
        mind = torch.full(x64.shape[:2], float("inf"), dtype=torch.float64, device=x.device)
        for i in range(1, ids.shape[1]):
            mind = torch.minimum(mind, (x64 - x64[rows, ids[:, i - 1]][:, None, :]).square().sum(-1))
            best = mind.max(dim=1).values
            worst = torch.maximum(worst, ((best - mind[rows, ids[:, i]]) / best).max())
    return float(worst)


def resident_workgroups(N, S, device):
    """Workgroups of fps_kernel resident at once: compute units x what the register file allows per unit (the P = 16
    instantiations take 80 VGPRs, 6 waves per SIMD; the others at most 56, the full 8), capped by the set size."""
    P, T = metrics.fps_kernel_shape(N)
    waves_per_cu = 4 * (6 if P == 16 else 8)
    return min(S, torch.cuda.get_device_properties(device).multi_processor_count * min(32, waves_per_cu // (T // 64)))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--S", type=int, default=662)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--hip-only", action="store_true")
    ap.add_argument("--out")
    args = ap.parse_args()
    if args.reps < 5 and not args.hip_only:
        ap.error("--reps must be at least 5")
    S = args.S
    res = {"S": S, "reps": args.reps, "launch_cap_point_steps": metrics._FPS_POINT_STEPS_PER_LAUNCH, "shapes": {}}
    for N, n in SHAPES:
        x = ball_clouds(S, N, N)
        metrics.farthest_point_sample(x[:8], n)  # warm-up (library load, first launch)
        # one launch for the whole set, whatever the cap: the kernel time of the case
        (idx, dist), t, spread = timed(lambda: metrics.farthest_point_sample(x, n, return_distances=True, max_clouds_per_launch=S), args.reps)
        _, t_api, _ = timed(lambda: metrics.farthest_point_sample(x, n), args.reps)  # as a user calls it: capped launches, int64 indices
        P, T = metrics.fps_kernel_shape(N)
        resident = resident_workgroups(N, S, x.device)
        case = {"points_per_thread": P, "workgroup_size": T, "resident_workgroups": resident, "hip_one_launch_s": t, "hip_spread": round(spread, 4),
                "hip_api_s": t_api, "ns_per_selected_point_per_cloud": round(t * resident / (S * n) * 1e9, 1)}
        if not args.hip_only:
            torch_fps(x[:8], 8)
            t_idx, tt, t_spread = timed(lambda: torch_fps(x, n), args.reps)
            case.update({"torch_s": tt, "torch_spread": round(t_spread, 4), "speedup": round(tt / t, 1),
                         "share_of_indices_equal_to_torch": float((idx == t_idx).double().mean()),
                         "hip_worst_relative_shortfall": worst_shortfall(x, idx), "torch_worst_relative_shortfall": worst_shortfall(x, t_idx)})
            assert case["hip_worst_relative_shortfall"] <= REL, case
            assert bool((dist[:, 1:-1] >= dist[:, 2:]).all())
            case["hip_wins_beyond_spread"] = bool(tt > t * (1 + spread + t_spread))
        res["shapes"][f"{N}->{n}"] = case
    line = json.dumps(res)
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
