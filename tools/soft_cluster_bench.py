"""Forward + backward of the soft cluster pooling under a scalar loss: clustering.soft_cluster_pool(points, centers).square().sum()
with the gradient taken into the points AND the shared centres (csrc/soft_cluster.hip: nothing of size N K stored, no
atomics) against torch autograd of the reference's literal form on the same GPU (torch.cdist, softmax(-distances), the
Python loop over the clusters, + 1e-8: transformer_pointcloud_nova.py:465-487 and :724-741), at K = 8 centres and

    32 x 2048 points      a training batch of generated clouds
    32 x 15000 points     a batch at the reference's point_cloud_size
    1 x 15000 points      one cloud: a sampling step

    python3 tools/soft_cluster_bench.py [--out profiles/soft_cluster_bench.json]     every case, one JSON line
    python3 tools/soft_cluster_bench.py --case 1x15000 [--hip-only]                   one case in this process, for a kernel-time run:
    rocprofv3 --kernel-trace --stats --output-format csv -d DIR -o soft_cluster -- python3 tools/soft_cluster_bench.py --case 1x15000 --hip-only

Every case runs in a child process of its own under a time limit (--limit seconds); after a case that fails or runs out of
time nothing more is started. One call is the loss forward and backward. After a warm-up, a timed window is as many calls in
a row as last about --window seconds, between two device events; the windows of the two forms alternate, --reps of each (5 by
default): the best time per call and the spread (max - min) / min. The peak of torch.cuda.max_memory_allocated over one
call, above what is allocated before it (the inputs), is recorded for both forms. Values and gradients of the two forms are
compared (largest difference relative to the largest entry). No ratio is fixed in advance: the times are reported, not
asserted. Bytes: one call must read x twice and write gx once, 36 bytes per point; `compulsory_bytes_per_s` is that over the
HIP form's time, an end-to-end rate of the two passes (the kernels are bound by instruction issue, not by memory: DESIGN.md).
"""
import argparse
import json
import os
import subprocess
import sys

from pointset_bench_common import ball_clouds, best_and_spread, calls_per_window, window

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASES = {"32x2048": (32, 2048, 8), "32x15000": (32, 15000, 8), "1x15000": (1, 15000, 8)}  # clouds, points, centres


def torch_soft_cluster(points, centers):
    """The reference's computation, op for op (the cluster MLP left out)."""
    import torch

    w = torch.softmax(-torch.cdist(points, centers), dim=-1)
    pooled = []
    for k in range(centers.shape[0]):
        wk = w[:, :, k:k + 1]
        pooled.append((points * wk).sum(dim=1) / (wk.sum(dim=1) + 1e-8))
    return torch.stack(pooled, dim=1)


def step(form, points, centers):
    points.grad = centers.grad = None
    loss = form(points, centers).square().sum()
    loss.backward()
    return loss.detach(), points.grad, centers.grad


def peak_rise(fn):
    """(result, bytes the peak of one call lies above what was allocated before it)."""
    import torch

    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    before = torch.cuda.memory_allocated()
    out = fn()
    torch.cuda.synchronize()
    return out, torch.cuda.max_memory_allocated() - before


def run_case(name, reps, hip_only, seconds):
    import torch

    sys.path.insert(0, ROOT)
    from nova_pointcloud_amd import clustering

    S, N, K = CASES[name]
    points = ball_clouds(S, N, N + K).requires_grad_(True)
    centers = (torch.randn(K, 3, generator=torch.Generator().manual_seed(K)) * 0.3).cuda().requires_grad_(True)
    forms = {"hip": lambda: step(clustering.soft_cluster_pool, points, centers)}
    if not hip_only:
        forms["torch"] = lambda: step(torch_soft_cluster, points, centers)
    for fn in forms.values():  # warm-up: library load, first launches, the allocator's blocks
        fn()
        fn()
    before = dict(clustering.stats)
    (loss, gp, gc), hip_peak = peak_rise(forms["hip"])
    launches, gp, gc = {key: clustering.stats[key] - before[key] for key in before}, gp.clone(), gc.clone()
    inner = {key: calls_per_window(fn, seconds) for key, fn in forms.items()}
    times = {key: [] for key in forms}
    for _ in range(reps):  # the forms alternate, so drift of the clock or the host meets both alike
        for key, fn in forms.items():
            times[key].append(window(fn, inner[key])[1])
    t, spread = best_and_spread(times["hip"])
    props = torch.cuda.get_device_properties(0)
    compulsory = S * N * 36
    case = {"clouds": S, "points": N, "centers": K, "hip_s": t, "hip_spread": round(spread, 4), "hip_calls_per_window": inner["hip"],
            "hip_launches_per_call": launches, "hip_peak_rise_bytes": hip_peak, "compulsory_bytes": compulsory,
            "compulsory_bytes_per_s": compulsory / t, "pairs_per_s": 2 * S * N * K / t, "device": props.name,
            "compute_units": props.multi_processor_count}
    if not hip_only:
        (t_loss, t_gp, t_gc), torch_peak = peak_rise(forms["torch"])
        tt, t_spread = best_and_spread(times["torch"])
        case.update({"torch_s": tt, "torch_spread": round(t_spread, 4), "torch_calls_per_window": inner["torch"], "torch_peak_rise_bytes": torch_peak,
                     "speedup": round(tt / t, 2), "memory_ratio": round(torch_peak / max(1, hip_peak), 1),
                     "loss_difference_over_loss": float((loss - t_loss).abs() / t_loss.abs()),
                     "point_gradient_difference_over_largest_entry": float((gp - t_gp).abs().max() / t_gp.abs().max()),
                     "center_gradient_difference_over_largest_entry": float((gc - t_gc).abs().max() / t_gc.abs().max()),
                     "hip_wins_beyond_spread": bool(tt > t * (1 + spread + t_spread)),
                     "torch_wins_beyond_spread": bool(t > tt * (1 + spread + t_spread))})
    return case


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--case", choices=sorted(CASES))
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--window", type=float, default=0.2, help="seconds of back-to-back calls one timed window lasts")
    ap.add_argument("--limit", type=int, default=120, help="seconds one case may take")
    ap.add_argument("--hip-only", action="store_true")
    ap.add_argument("--out")
    args = ap.parse_args()
    if args.reps < 5 and not args.hip_only:
        ap.error("--reps must be at least 5")
    if args.case:
        print(json.dumps(run_case(args.case, args.reps, args.hip_only, args.window)))
        return
    res = {"reps": args.reps, "window_s": args.window, "cases": {}}  # no GPU work in this process: the cases run in children
    for name in CASES:
        cmd = [sys.executable, os.path.abspath(__file__), "--case", name, "--reps", str(args.reps), "--window", str(args.window)] + (["--hip-only"] if args.hip_only else [])
        try:
            out = subprocess.run(cmd, capture_output=True, text=True, timeout=args.limit)
        except subprocess.TimeoutExpired:
            sys.exit(f"{name}: no result within {args.limit} s; nothing more is started")
        if out.returncode != 0:
            sys.stderr.write(out.stdout + out.stderr)
            sys.exit(f"{name}: exit status {out.returncode}; nothing more is started")
        res["cases"][name] = json.loads([l for l in out.stdout.splitlines() if l.startswith("{")][-1])
        print(f"{name}: {res['cases'][name]}", file=sys.stderr, flush=True)
    line = json.dumps(res)
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
