"""Forward + backward of the depth-aware positional encoding under a scalar loss:
encoding.coordinate_encoding(points, scale, E, base=base).square().mean() with the gradient taken into the points, the
scales AND base (csrc/posenc.hip: one kernel forward, one backward that recomputes every sine and cosine, nothing of size
N E stored) against torch autograd of the reference's literal form on the same GPU (the zeros, the six strided slice
assignments, the separate add: transformer_pointcloud_nova.py:367-389 and :458; the table moved to the device, which the
reference itself omits), at E = 768 and

    32 x 2048 points      a training batch of generated clouds
    1 x 15000 points      one cloud at the reference's point_cloud_size

    python3 tools/posenc_bench.py [--out profiles/posenc_bench.json]     every case, one JSON line
    python3 tools/posenc_bench.py --case 32x2048 [--hip-only]             one case in this process, for a kernel-time run:
    rocprofv3 --kernel-trace --stats --output-format csv -d DIR -o posenc -- python3 tools/posenc_bench.py --case 32x2048 --hip-only

Every case runs in a child process of its own under a time limit (--limit seconds); after a case that fails or runs out of
time nothing more is started. One call is the loss forward and backward. After a warm-up, a timed window is as many calls in
a row as last about --window seconds, between two device events; the windows of the two forms alternate, --reps of each (5 by
default): the best time per call and the spread (max - min) / min. The peak of torch.cuda.max_memory_allocated over one
call, above what is allocated before it (the inputs), is recorded for both forms. The gradients of the two forms are compared
(largest difference relative to the largest entry). No ratio is fixed in advance: the times are reported, not asserted.

The forward kernel alone: `forward_s` is one coordinate_encoding call without base under no_grad (the kernel and the
allocation of its output), timed the same way; its compulsory traffic is the S N E 4 bytes it stores (12 bytes per point
read), and `forward_bytes_per_s` over HBM_BYTES_PER_S is its share of the achievable HBM rate (6.3 TB/s of 8.0 peak). The
same call executes S N 3 (E // 6) IEEE divisions and accurate sincosf: `forward_pairs_per_s`."""
import argparse
import json
import os
import subprocess
import sys

from pointset_bench_common import ball_clouds, best_and_spread, calls_per_window, window

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASES = {"32x2048": (32, 2048, 768), "1x15000": (1, 15000, 768)}  # clouds, points, channels
HBM_BYTES_PER_S = 6.3e12  # achievable (float4 copy); 8.0e12 is the specification


def torch_encoding(points, scale, base, div_term, E):
    """The reference's computation, op for op (scale [3] per coordinate, the table on the device)."""
    import torch

    scaled = points * scale
    pe = torch.zeros(points.shape[0], points.shape[1], E, device=points.device)
    d = div_term[:E // 6]
    pe[:, :, 0::6] = torch.sin(scaled[:, :, 0:1] / d)
    pe[:, :, 1::6] = torch.cos(scaled[:, :, 0:1] / d)
    pe[:, :, 2::6] = torch.sin(scaled[:, :, 1:2] / d)
    pe[:, :, 3::6] = torch.cos(scaled[:, :, 1:2] / d)
    pe[:, :, 4::6] = torch.sin(scaled[:, :, 2:3] / d)
    pe[:, :, 5::6] = torch.cos(scaled[:, :, 2:3] / d)
    return base + pe


def step(form, points, scale, base):
    points.grad = scale.grad = base.grad = None
    loss = form(points, scale, base).square().mean()
    loss.backward()
    return loss.detach(), points.grad, scale.grad, base.grad


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
    from nova_pointcloud_amd import encoding

    S, N, E = CASES[name]
    points = ball_clouds(S, N, N + E).requires_grad_(True)
    scale = torch.tensor([1.0, 1.25, 0.75]).cuda().requires_grad_(True)
    base = (torch.randn(S, N, E, generator=torch.Generator().manual_seed(E)) * 0.02).cuda().requires_grad_(True)
    table = encoding.reference_div_term(E).cuda()
    forms = {"hip": lambda: step(lambda p, s, b: encoding.coordinate_encoding(p, s, E, base=b), points, scale, base)}
    if not hip_only:
        forms["torch"] = lambda: step(lambda p, s, b: torch_encoding(p, s, b, table, E), points, scale, base)
    for fn in forms.values():  # warm-up: library load, first launches, the allocator's blocks
        fn()
        fn()
    before = dict(encoding.stats)
    (loss, gp, gs, gb), hip_peak = peak_rise(forms["hip"])
    launches = {key: encoding.stats[key] - before[key] for key in before}
    gp, gs, gb = gp.clone(), gs.clone(), gb.clone()

    def forward_only():
        with torch.no_grad():
            return encoding.coordinate_encoding(points, scale, E)

    forward_only()
    inner = {key: calls_per_window(fn, seconds) for key, fn in forms.items()}
    inner_f = calls_per_window(forward_only, seconds)
    times, times_f = {key: [] for key in forms}, []
    for _ in range(reps):  # the forms alternate, so drift of the clock or the host meets both alike
        for key, fn in forms.items():
            times[key].append(window(fn, inner[key])[1])
        times_f.append(window(forward_only, inner_f)[1])
    t, spread = best_and_spread(times["hip"])
    tf, spread_f = best_and_spread(times_f)
    props = torch.cuda.get_device_properties(0)
    pairs, stored = S * N * 3 * (E // 6), S * N * E * 4
    case = {"clouds": S, "points": N, "channels": E, "hip_s": t, "hip_spread": round(spread, 4), "hip_calls_per_window": inner["hip"],
            "hip_launches_per_call": launches, "hip_peak_rise_bytes": hip_peak, "forward_s": tf, "forward_spread": round(spread_f, 4),
            "forward_calls_per_window": inner_f, "forward_stored_bytes": stored, "forward_bytes_per_s": (stored + S * N * 12) / tf,
            "forward_share_of_hbm_rate": round((stored + S * N * 12) / tf / HBM_BYTES_PER_S, 4), "hbm_bytes_per_s": HBM_BYTES_PER_S,
            "forward_pairs_per_s": pairs / tf, "device": props.name, "compute_units": props.multi_processor_count}
    if not hip_only:
        (t_loss, t_gp, t_gs, t_gb), torch_peak = peak_rise(forms["torch"])
        tt, t_spread = best_and_spread(times["torch"])
        rel = lambda a, b: float((a - b).abs().max() / b.abs().max())
        case.update({"torch_s": tt, "torch_spread": round(t_spread, 4), "torch_calls_per_window": inner["torch"], "torch_peak_rise_bytes": torch_peak,
                     "speedup": round(tt / t, 2), "memory_ratio": round(torch_peak / max(1, hip_peak), 2),
                     "loss_difference_over_loss": float((loss - t_loss).abs() / t_loss.abs()),
                     "point_gradient_difference_over_largest_entry": rel(gp, t_gp),
                     "scale_gradient_difference_over_largest_entry": rel(gs, t_gs),
                     "base_gradient_difference_over_largest_entry": rel(gb, t_gb),
                     "largest_gradient_difference": max(rel(gp, t_gp), rel(gs, t_gs), rel(gb, t_gb)),
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
