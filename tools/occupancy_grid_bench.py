"""Occupancy grid of a chair-sized test set (662 clouds of 2048 points, 28^3 in-sphere grid): the HIP kernel
(csrc/occupancy.hip through metrics.occupancy_grid) against a chunked torch form (torch.cdist to the 10144 grid nodes,
argmin, bincount), in one process, outputs compared, both timed with device events after a warm-up, for three inputs:

    fast     every point's rounded node is a grid node (ball of radius 0.45)
    mixed    ball of radius 0.9: most points outside the grid, at a small distance (a small column window each)
    slow     shell of radius 1.8 - 2.0: every point on the slow path with the whole grid as its window (the worst case)

    python3 tools/occupancy_grid_bench.py [--out FILE]           both paths, one JSON line
    python3 tools/occupancy_grid_bench.py --hip-only             the HIP launches only, for a kernel-time run:
    rocprofv3 --kernel-trace --stats --output-format csv -d DIR -o occ -- python3 tools/occupancy_grid_bench.py --hip-only

The bound is reading 12 bytes per point once at the achievable HBM rate DESIGN.md uses for row_norm (6.3 TB/s). The
torch form differs from the kernel on float32 near-ties only; the share of differing points is reported and bounded.
--workgroups sweeps the kernel's grid size on the fast and mixed inputs.
"""
import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from nova_pointcloud_amd import metrics  # noqa: E402

HBM_BYTES_PER_S = 6.3e12
R = 28


def ball(S, n, seed, radius, shell=False):
    g = torch.Generator().manual_seed(seed)
    p = torch.randn(S, n, 3, generator=g)
    r = torch.rand(S, n, 1, generator=g) ** (1 / 3)
    if shell:
        r = 0.9 + 0.1 * r
    return (p / p.norm(dim=-1, keepdim=True) * r * radius).cuda()


def timed(fn, reps):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    best = float("inf")
    for _ in range(reps):
        torch.cuda.synchronize()
        a.record()
        out = fn()
        b.record()
        torch.cuda.synchronize()
        best = min(best, a.elapsed_time(b) / 1e3)
    return out, best


def torch_nodes(x, nodes, flat, chunk):
    """Each point's nearest grid node by torch.cdist + argmin over chunks of points, and the counters by bincount."""
    pts = x.reshape(-1, 3)
    out = torch.empty(pts.shape[0], dtype=torch.int64, device=x.device)
    for p0 in range(0, pts.shape[0], chunk):
        out[p0:p0 + chunk] = flat[torch.cdist(pts[p0:p0 + chunk], nodes).argmin(dim=1)]
    return out, torch.bincount(out, minlength=R ** 3)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--S", type=int, default=662)
    ap.add_argument("--n", type=int, default=2048)
    ap.add_argument("--chunk", type=int, default=16384, help="points per torch step")
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--workgroups", type=int, nargs="*", default=[], help="also time these grid sizes")
    ap.add_argument("--hip-only", action="store_true")
    ap.add_argument("--out")
    args = ap.parse_args()
    S, n = args.S, args.n
    inputs = {"fast": ball(S, n, 1, 0.45), "mixed": ball(S, n, 2, 0.9), "slow": ball(S, n, 3, 2.0, shell=True)}
    mask = metrics.grid_node_mask(R)
    flat = torch.nonzero(mask).reshape(-1).cuda()
    nodes = ((2 * torch.stack([flat // (R * R), (flat // R) % R, flat % R], 1) - (R - 1)).float() / (2.0 * (R - 1)))
    bound = S * n * 12 / HBM_BYTES_PER_S
    res = {"S": S, "N": n, "R": R, "grid_nodes": int(mask.sum()), "bound": "12 bytes per point once at 6.3 TB/s",
           "bound_s": bound, "launch_cap_points": metrics._OCC_POINTS_PER_LAUNCH}
    for name, x in inputs.items():
        metrics.occupancy_grid(x[:8])  # warm-up (library load, first launch)
        # one launch for the whole set, whatever the cap: the kernel time of the case
        one = lambda wg=0: metrics.occupancy_grid(x, return_nodes=False, max_clouds_per_launch=S, workgroups=wg)
        occ, t = timed(one, args.reps)
        _, t_api = timed(lambda: metrics.occupancy_grid(x), args.reps)  # as a user calls it: capped launches
        res[name] = {"outside_fraction": occ["outside"] / (S * n), "hip_one_launch_s": t, "hip_points_per_s": S * n / t,
                     "hip_api_s": t_api, "times_bound": round(t / bound, 1)}
        for wg in args.workgroups if name != "slow" else []:
            res[name][f"hip_s_workgroups_{wg}"] = timed(lambda: one(wg), args.reps)[1]
        if not args.hip_only:
            torch_nodes(x[:8], nodes, flat, args.chunk)
            (t_nodes, t_counters), tt = timed(lambda: torch_nodes(x, nodes, flat, args.chunk), 3)
            got = metrics.occupancy_grid(x, return_nodes=True)
            differ = int((got["nodes"].reshape(-1).long() != t_nodes).sum())
            res[name].update({"torch_s": tt, "torch_points_per_s": S * n / tt, "speedup": round(tt / t, 1),
                              "points_differing_from_torch": differ})
            assert differ <= 1e-2 * S * n, differ  # float32 near-ties only (cdist expands |p|^2 + |c|^2 - 2 p.c)
            assert int(got["counters"].sum()) == S * n
    # the longest launch a user can meet: a full cap of points, every one on the slow path with the whole grid as its window
    cap_clouds = max(1, metrics._OCC_POINTS_PER_LAUNCH // n)
    worst = ball(cap_clouds, n, 4, 2.0, shell=True)
    _, t_cap = timed(lambda: metrics.occupancy_grid(worst, max_clouds_per_launch=cap_clouds), 5)
    res["worst_case_launch"] = {"clouds": cap_clouds, "points": cap_clouds * n, "seconds": t_cap, "points_per_s": cap_clouds * n / t_cap}
    line = json.dumps(res)
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
