"""The exact EMD of an evaluation batch: metrics.optimal_assignment (csrc/assign.hip, the auction on the GPU) against the
host path it replaces (metrics.pairwise_dist, .cpu(), scipy's linear_sum_assignment pair after pair), in one process, on
B = 32 and B = 662 pairs of 512- and 2048-point clouds (standard normal, clipped to +-5, clamp 5 as compute_emd_distance).

    python3 tools/assignment_bench.py [--out profiles/assignment_bench.json] [--host-pairs K]

Reported per case, best of --reps (>= 5) with the spread (max - min) / min:
    device_s             optimal_assignment as a user calls it (default rounds_per_launch), device events around the call
    host_s               the host path. scipy solves the pairs one after another on one core, so its time is linear in B:
                         it is MEASURED on the first --host-pairs pairs (default 4; 0 = all B) and scaled to B, and
                         host_pairs_measured says so. pairwise_dist and the copy are part of the measured time.
    rounds               bidding rounds per pair: min, median, max
    longest_launch_s     the longest single kernel launch of one run (the loop of optimal_assignment replayed with an event
                         pair around every launch); metrics._ASSIGN_COLUMN_VISITS_PER_LAUNCH is to be re-derived from it
    mean_minus_host      device cost minus the host's mean on the measured pairs: max and min (within [-1e-6, 2^-18 + 1e-6])
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from nova_pointcloud_amd import hip, metrics  # noqa: E402
from pointset_bench_common import timed  # noqa: E402

CASES = ((32, 512), (662, 512), (32, 2048), (662, 2048))
CLAMP = 5.0


def clouds(B, n, seed):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(B, n, 3, generator=g).clamp(-5, 5).cuda(), torch.randn(B, n, 3, generator=g).clamp(-5, 5).cuda()


def host_path(x, y):
    cost = metrics.pairwise_dist(x, y, CLAMP).cpu().numpy()
    return np.array([float(metrics._assignment_mean(c)) for c in cost])


def wall(fn, reps):
    times = []
    for _ in range(reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = fn()
        times.append(time.perf_counter() - t0)
    return out, min(times), (max(times) - min(times)) / min(times)


def launch_times(x, y):
    """The launch loop of metrics.optimal_assignment with an event pair around every launch: seconds per launch."""
    B, n = x.shape[:2]
    max_rounds, per_launch = metrics._assignment_arguments(x, y, CLAMP, None, None)
    idx = torch.empty(B, n, dtype=torch.int32, device=x.device)
    cost = torch.empty(B, dtype=torch.float32, device=x.device)
    state = torch.empty(B * int(hip.load().nova_pointset_assignment_state_bytes(n)), dtype=torch.uint8, device=x.device)
    flag = torch.zeros(1, dtype=torch.int32, device=x.device)
    out, left, restart = [], max_rounds, 1
    while left > 0:
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        step = min(per_launch, left)
        a.record()
        hip.call("nova_pointset_assignment", x.data_ptr(), y.data_ptr(), idx.data_ptr(), cost.data_ptr(), state.data_ptr(), B, n,
                 -CLAMP, CLAMP, 1, step, restart, flag.data_ptr(), hip.stream_ptr())
        b.record()
        torch.cuda.synchronize()
        out.append(a.elapsed_time(b) / 1e3)
        left, restart = left - step, 0
        if int(flag) != 0:
            break
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--host-reps", type=int, default=5)
    ap.add_argument("--host-pairs", type=int, default=4)
    ap.add_argument("--out")
    args = ap.parse_args()
    if args.reps < 5:
        ap.error("--reps must be at least 5")
    res = {"reps": args.reps, "host_reps": args.host_reps, "column_visits_per_launch": metrics._ASSIGN_COLUMN_VISITS_PER_LAUNCH, "cases": {}}
    xw, yw = clouds(2, 64, 0)
    metrics.optimal_assignment(xw, yw, clamp=CLAMP)  # warm-up (library load, first launch)
    host_path(xw, yw)
    for B, n in CASES:
        x, y = clouds(B, n, 100 * n + B)
        metrics.optimal_assignment(x[:2], y[:2], clamp=CLAMP)
        (idx, cost, rounds), t, spread = timed(lambda: metrics.optimal_assignment(x, y, clamp=CLAMP, return_rounds=True), args.reps)
        assert bool((idx.sort(dim=1).values == torch.arange(n, device=idx.device)).all())
        k = B if args.host_pairs == 0 else min(B, args.host_pairs)
        ref, th, h_spread = wall(lambda: host_path(x[:k], y[:k]), args.host_reps)
        diff = cost[:k].double().cpu().numpy() - ref
        assert -1e-6 <= diff.min() and diff.max() <= 2.0 ** -18 + 1e-6, diff
        launches = launch_times(x, y)
        r = rounds.double()
        res["cases"][f"B{B}_n{n}"] = {
            "workgroup_size": metrics.assignment_kernel_shape(n)[0], "rounds_per_launch": max(16, metrics._ASSIGN_COLUMN_VISITS_PER_LAUNCH // n),
            "device_s": t, "device_spread": round(spread, 4), "host_pairs_measured": k, "host_s": th * B / k, "host_spread": round(h_spread, 4),
            "host_over_device": round(th * B / k / t, 1), "rounds": {"min": int(r.min()), "median": float(r.median()), "max": int(r.max())},
            "launches": len(launches), "longest_launch_s": max(launches), "mean_minus_host": {"min": float(diff.min()), "max": float(diff.max())}}
        print(f"B{B}_n{n}", json.dumps(res["cases"][f"B{B}_n{n}"]), flush=True)
    line = json.dumps(res)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
