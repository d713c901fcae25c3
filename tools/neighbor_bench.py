"""Forward + backward of the kNN neighbourhood aggregation under a loss: neighbors.edge_features(points, features).square().mean()
(csrc/neighbor.hip: no [N, k, C] array, the feature gradient a gather through the inverse neighbour list, no atomics) against
the torch form on the same GPU with the same metrics.knn_points indices (torch.gather to [B, N, k, C], mean over k, autograd:
the reference's extract_edge_features, transformer_pointcloud_nova.py:176-190, with its gather made to run), at

    32 x 2048 points, C = 768, k = 8      a batch of generated clouds at the reference's feature width
    1 x 15000 points, C = 768, k = 8      one published reference shape

    python3 tools/neighbor_bench.py [--out profiles/neighbor_bench.json]     every case, one JSON line
    python3 tools/neighbor_bench.py --case 1x15000 [--hip-only]               one case in this process, for a kernel-time run:
    rocprofv3 --kernel-trace --stats --output-format csv -d DIR -o neighbor -- python3 tools/neighbor_bench.py --case 1x15000 --hip-only

Every case runs in a child process of its own under a time limit (--limit seconds); after a case that fails or runs out of
time nothing more is started. One call is the loss forward and backward into the features; both forms call knn_points inside
(the indices carry no gradient), and its time alone is recorded beside them so that the aggregation's share can be read off.
After a warm-up, a timed window is as many calls in a row as last about --window seconds, between two device events; the
windows of the forms alternate, --reps of each (5 by default): the best time per call and the spread (max - min) / min. The
peak of torch.cuda.max_memory_allocated over one call, above what is allocated before it (the inputs), is recorded for both
forms. Value and gradient of the two forms are compared (largest difference relative to the largest entry). No ratio is fixed
in advance: the times are reported, not asserted. Bytes: the compulsory traffic of one call's aggregation is (M + N) C 4 per
cloud forward and as much backward, the gathered rows N k C 4 each way on top; `compulsory_bytes_per_s` is the first over the
HIP form's time WITHOUT the kNN search, an end-to-end rate of the two passes, not a kernel's share of peak.
"""
import argparse
import json
import os
import subprocess
import sys

from pointset_bench_common import ball_clouds, best_and_spread, calls_per_window, window

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASES = {"32x2048": (32, 2048, 768, 8), "1x15000": (1, 15000, 768, 8)}  # clouds, points, channels, k


def torch_edge_features(points, features, k):
    """The gather / mean form on knn_points' indices."""
    import torch

    from nova_pointcloud_amd import metrics

    S, N, C = features.shape
    idx = metrics.knn_points(points, points, k=min(k, N), exclude_self=False, return_distances=False)
    kk = idx.shape[2]
    near = torch.gather(features[:, :, None, :].expand(S, N, kk, C), 1, idx[:, :, :, None].expand(S, N, kk, C))  # [B, N, k, C]
    return features - near.mean(dim=2)


def step(form, points, features, k):
    features.grad = None
    loss = form(points, features, k).square().mean()
    loss.backward()
    return loss.detach(), features.grad


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
    from nova_pointcloud_amd import metrics, neighbors

    S, N, C, k = CASES[name]
    points = ball_clouds(S, N, N + C)
    features = torch.randn(S, N, C, generator=torch.Generator().manual_seed(N)).cuda().requires_grad_(True)
    hip_step = lambda: step(lambda p, f, kk: neighbors.edge_features(p, f, k=kk), points, features, k)
    knn_only = lambda: metrics.knn_points(points, points, k=k, exclude_self=False, return_distances=False)
    torch_step = lambda: step(torch_edge_features, points, features, k)
    forms = {"hip": hip_step, "knn_only": knn_only}
    if not hip_only:
        forms["torch"] = torch_step
    for fn in forms.values():  # warm-up: library load, first launches, the allocator's blocks
        fn()
        fn()
    before = dict(neighbors.stats)
    (loss, grad), hip_peak = peak_rise(hip_step)
    launches, grad = {key: neighbors.stats[key] - before[key] for key in before}, grad.clone()
    inner = {key: calls_per_window(fn, seconds) for key, fn in forms.items()}
    times = {key: [] for key in forms}
    for _ in range(reps):  # the forms alternate, so drift of the clock or the host meets all of them alike
        for key, fn in forms.items():
            times[key].append(window(fn, inner[key])[1])
    t, spread = best_and_spread(times["hip"])
    t_knn = min(times["knn_only"])
    props = torch.cuda.get_device_properties(0)
    compulsory = 2 * S * (N + N) * C * 4
    case = {"clouds": S, "points": N, "channels": C, "k": k, "hip_s": t, "hip_spread": round(spread, 4), "hip_calls_per_window": inner["hip"],
            "knn_only_s": t_knn, "hip_launches_per_call": launches, "hip_peak_rise_bytes": hip_peak,
            "compulsory_bytes": compulsory, "gathered_bytes": 2 * S * N * k * C * 4,
            "compulsory_bytes_per_s": compulsory / max(t - t_knn, 1e-9), "device": props.name, "compute_units": props.multi_processor_count}
    if not hip_only:
        (t_loss, t_grad), torch_peak = peak_rise(torch_step)
        tt, t_spread = best_and_spread(times["torch"])
        case.update({"torch_s": tt, "torch_spread": round(t_spread, 4), "torch_calls_per_window": inner["torch"], "torch_peak_rise_bytes": torch_peak,
                     "speedup": round(tt / t, 2), "speedup_without_knn": round((tt - t_knn) / max(t - t_knn, 1e-9), 2),
                     "memory_ratio": round(torch_peak / max(1, hip_peak), 1),
                     "loss_difference_over_loss": float((loss - t_loss).abs() / t_loss.abs()),
                     "gradient_difference_over_largest_entry": float((grad - t_grad).abs().max() / t_grad.abs().max()),
                     "hip_wins_beyond_spread": bool(tt > t * (1 + spread + t_spread)),
                     "torch_wins_beyond_spread": bool(t > tt * (1 + spread + t_spread))})
    return case


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--case", choices=sorted(CASES))
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--window", type=float, default=0.2, help="seconds of back-to-back calls one timed window lasts")
    ap.add_argument("--limit", type=int, default=180, help="seconds one case may take")
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
