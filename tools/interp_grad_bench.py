"""Forward + backward of the distance-weighted interpolation with a gradient into the points: sampling.kernel_interpolate
(csrc/interp.hip with statistics, csrc/interp_bwd.hip: nothing of size T N in either pass) against torch autograd of the
reference's literal form (feature_aware_interpolation, transformer_pointcloud_nova.py:145-150: torch.cdist, softmax(-dist),
weights.unsqueeze(-1) * points.unsqueeze(1), sum), on the same GPU, at

    32 x 2048 -> 1024 points      a batch of generated clouds thinned to half
    1 x 15000 -> 7500 points      one published reference shape thinned to half

    python3 tools/interp_grad_bench.py [--out profiles/interp_grad_bench.json]    every case, one JSON line
    python3 tools/interp_grad_bench.py --case 1x15000to7500 [--hip-only]           one case in this process, for a kernel-time run:
    rocprofv3 --kernel-trace --stats --output-format csv -d DIR -o interp_grad -- python3 tools/interp_grad_bench.py --case 1x15000to7500 --hip-only

Every case runs in a child process of its own under a time limit (--limit seconds); after a case that fails or runs out of
time nothing more is started. One call is what feature_aware_interpolation does under a loss: the queries are taken from the
points by one seeded permutation (an indexing op, inside the call), the interpolation runs forward, and a fixed upstream
gradient is sent back into the points, which receive it as sources, as values and, through the indexing, as queries. After
a warm-up, a timed window is as many calls in a row as last about --window seconds, between two device events; the windows
of the forms alternate, --reps of each: the best time per call and the spread (max - min) / min. The peak of
torch.cuda.max_memory_allocated over one call, above what is allocated before it, is recorded for both forms. The two
gradients are compared (largest difference relative to the largest entry; the torch form is float32 with cdist's matmul
mode). No ratio is fixed in advance: the times are reported, not asserted.
"""
import argparse
import json
import os
import subprocess
import sys

from pointset_bench_common import ball_clouds, best_and_spread, calls_per_window, window

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASES = {"32x2048to1024": (32, 2048, 1024), "1x15000to7500": (1, 15000, 7500)}


def torch_interpolate(q, p):
    """The reference's form, statement by statement (its dead topk left out)."""
    import torch

    dist = torch.cdist(q, p)
    weights = torch.softmax(-dist, dim=-1)
    return torch.sum(weights.unsqueeze(-1) * p.unsqueeze(1), dim=2)


def step(form, points, perm, upstream):
    points.grad = None
    out = form(points[:, perm], points)
    out.backward(upstream)
    return out.detach(), points.grad


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
    from nova_pointcloud_amd import metrics, sampling

    S, N, T = CASES[name]
    points = ball_clouds(S, N, N + T).requires_grad_(True)
    perm = torch.randperm(N, generator=torch.Generator().manual_seed(T))[:T].cuda()
    upstream = torch.randn(S, T, 3, generator=torch.Generator().manual_seed(N)).cuda()
    hip_step = lambda: step(sampling.kernel_interpolate, points, perm, upstream)
    hip_forward = lambda: metrics.kernel_interpolate(points.detach()[:, perm], points.detach())
    torch_step = lambda: step(torch_interpolate, points, perm, upstream)
    forms = {"hip": hip_step, "hip_forward_only": hip_forward}
    if not hip_only:
        forms["torch"] = torch_step
    for fn in forms.values():  # warm-up: library load, first launches, the allocator's blocks
        fn()
        fn()
    before = dict(sampling.stats)
    (out, grad), hip_peak = peak_rise(hip_step)
    launches, grad = {k: sampling.stats[k] - before[k] for k in before}, grad.clone()
    inner = {k: calls_per_window(fn, seconds) for k, fn in forms.items()}
    times = {k: [] for k in forms}
    for _ in range(reps):  # the forms alternate, so drift of the clock or the host meets all of them alike
        for k, fn in forms.items():
            times[k].append(window(fn, inner[k])[1])
    t, spread = best_and_spread(times["hip"])
    props = torch.cuda.get_device_properties(0)
    case = {"clouds": S, "points": N, "queries": T, "hip_s": t, "hip_spread": round(spread, 4), "hip_calls_per_window": inner["hip"],
            "hip_forward_only_s": min(times["hip_forward_only"]), "hip_launches_per_call": launches, "hip_peak_rise_bytes": hip_peak,
            "pair_visits_per_s": 3 * S * T * N / t, "device": props.name, "compute_units": props.multi_processor_count}
    if not hip_only:
        (t_out, t_grad), torch_peak = peak_rise(torch_step)
        tt, t_spread = best_and_spread(times["torch"])
        case.update({"torch_s": tt, "torch_spread": round(t_spread, 4), "torch_calls_per_window": inner["torch"], "torch_peak_rise_bytes": torch_peak,
                     "speedup": round(tt / t, 2), "memory_ratio": round(torch_peak / max(1, hip_peak), 1),
                     "largest_output_difference": float((out - t_out).abs().max()),
                     "gradient_difference_over_largest_entry": float((grad - t_grad).abs().max() / t_grad.abs().max()),
                     "hip_wins_beyond_spread": bool(tt > t * (1 + spread + t_spread))})
    return case


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--case", choices=sorted(CASES))
    ap.add_argument("--reps", type=int, default=7)
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
