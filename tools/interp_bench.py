"""Distance-weighted interpolation of a dense cloud set down to fewer points (the reference's feature_aware_interpolation,
transformer_pointcloud_nova.py:128-152): the HIP kernel (csrc/interp.hip through metrics.kernel_interpolate) against the
reference's own form in torch on the same GPU - torch.cdist, softmax(-dist), sum(weights.unsqueeze(-1) *
points.unsqueeze(1), dim=2), with its dead topk left out - at

    32 x 2048 -> 1024 points      a batch of generated clouds thinned to half
    1 x 15000 -> 7500 points      one published reference shape thinned to half

    python3 tools/interp_bench.py [--out profiles/interp_bench.json]     every case, one JSON line
    python3 tools/interp_bench.py --case 1x15000to7500 [--hip-only]       one case in this process, for a kernel-time run:
    rocprofv3 --kernel-trace --stats --output-format csv -d DIR -o interp -- python3 tools/interp_bench.py --case 1x15000to7500 --hip-only

Every case runs in a child process of its own under a time limit (--limit seconds); after a case that fails or runs out of
time nothing more is started. The queries are the first T points of one seeded permutation, as in the reference. The
kernel's output is checked against the float64 restatement of tests/test_pointset_interp.py on the first queries of the
first cloud, within that file's bound (N + 512) 2^-24 max |v|. Both forms are timed with device events after a warm-up: the
best of --reps repetitions and the spread (max - min) / min. The torch form holds an [clouds, queries, N, 3] float32 product:
it is chunked over clouds and queries only as far as 16 GiB for that product force. The HIP form is timed as one launch for
the whole set and as a user calls it (launches capped at metrics._INTERP_PAIRS_PER_LAUNCH); each capped launch is also
timed alone, and the longest one is what that constant is re-derived from. No ratio is fixed in advance: the figures are
reported, not asserted.
"""
import argparse
import json
import os
import subprocess
import sys

from pointset_bench_common import ball_clouds, timed

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASES = {"32x2048to1024": (32, 2048, 1024), "1x15000to7500": (1, 15000, 7500)}
PRODUCT_BYTES = 1 << 34  # what the torch form may hold at a time


def torch_interpolate(q, p, clouds, queries):
    """The reference's form, `clouds` clouds and `queries` queries at a time."""
    import torch

    out = torch.empty_like(q)
    for c0 in range(0, p.shape[0], clouds):
        pc = p[c0:c0 + clouds]
        for t0 in range(0, q.shape[1], queries):
            dist = torch.cdist(q[c0:c0 + clouds, t0:t0 + queries], pc)
            weights = torch.softmax(-dist, dim=-1)
            out[c0:c0 + clouds, t0:t0 + queries] = torch.sum(weights.unsqueeze(-1) * pc.unsqueeze(1), dim=2)
    return out


def worst_error_over_bound(q, p, out, n_queries=512):
    """Largest |out - float64 restatement| / ((N + 512) 2^-24 max |p|) over the first queries of the first cloud."""
    import torch

    q64, p64 = q[:1, :n_queries].double(), p[:1].double()
    d = torch.cdist(q64, p64)
    want = torch.softmax(-d, dim=-1) @ p64
    bound = (p.shape[1] + 512) * 2.0 ** -24 * p[:1].abs().amax(dim=1, keepdim=True).double()
    return float(((out[:1, :n_queries].double() - want).abs() / bound).max())


def run_case(name, reps, hip_only):
    import torch

    sys.path.insert(0, ROOT)
    from nova_pointcloud_amd import metrics

    S, N, T = CASES[name]
    p = ball_clouds(S, N, N + T)
    perm = torch.randperm(N, generator=torch.Generator().manual_seed(T))[:T].cuda()
    q = p[:, perm].contiguous()
    metrics.kernel_interpolate(q[:1, :64], p[:1])  # warm-up (library load, first launch)
    out, t, spread = timed(lambda: metrics.kernel_interpolate(q, p, max_clouds_per_launch=S), reps)
    _, t_api, _ = timed(lambda: metrics.kernel_interpolate(q, p), reps)
    per = max(1, metrics._INTERP_PAIRS_PER_LAUNCH // (T * N))
    launches = [timed(lambda: metrics.kernel_interpolate(q[s0:s0 + per], p[s0:s0 + per], max_clouds_per_launch=per), reps)[1]
                for s0 in range(0, S, per)]
    case = {"clouds": S, "points": N, "queries": T, "workgroups": S * ((T + 63) // 64), "hip_one_launch_s": t, "hip_spread": round(spread, 4),
            "hip_api_s": t_api, "clouds_per_capped_launch": min(S, per), "capped_launches": len(launches),
            "longest_capped_launch_s": max(launches), "pairs_per_s": S * T * N / t,
            "hip_worst_error_over_bound": worst_error_over_bound(q, p, out)}
    props = torch.cuda.get_device_properties(0)
    case.update({"device": props.name, "compute_units": props.multi_processor_count, "device_clock_mhz": getattr(props, "clock_rate", 0) / 1e3})
    assert case["hip_worst_error_over_bound"] <= 1, case
    if not hip_only:
        clouds = max(1, min(S, PRODUCT_BYTES // (T * N * 12)))
        queries = T if clouds > 1 or T * N * 12 <= PRODUCT_BYTES else max(1, PRODUCT_BYTES // (N * 12))
        torch_interpolate(q[:1, :64], p[:1], 1, 64)
        t_out, tt, t_spread = timed(lambda: torch_interpolate(q, p, clouds, queries), reps)
        case.update({"torch_s": tt, "torch_spread": round(t_spread, 4), "torch_clouds_per_chunk": clouds, "torch_queries_per_chunk": queries,
                     "speedup": round(tt / t, 2), "largest_difference_to_torch": float((out - t_out).abs().max()),
                     "hip_wins_beyond_spread": bool(tt > t * (1 + spread + t_spread))})
    return case


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--case", choices=sorted(CASES))
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--limit", type=int, default=240, help="seconds one case may take")
    ap.add_argument("--hip-only", action="store_true")
    ap.add_argument("--out")
    args = ap.parse_args()
    if args.reps < 5 and not args.hip_only:
        ap.error("--reps must be at least 5")
    if args.case:
        print(json.dumps(run_case(args.case, args.reps, args.hip_only)))
        return
    sys.path.insert(0, ROOT)
    from nova_pointcloud_amd import metrics  # no GPU work in this process: the cases run in children

    res = {"reps": args.reps, "launch_cap_pairs": metrics._INTERP_PAIRS_PER_LAUNCH, "cases": {}}
    for name in CASES:
        cmd = [sys.executable, os.path.abspath(__file__), "--case", name, "--reps", str(args.reps)] + (["--hip-only"] if args.hip_only else [])
        try:
            out = subprocess.run(cmd, capture_output=True, text=True, timeout=args.limit)
        except subprocess.TimeoutExpired:
            sys.exit(f"{name}: no result within {args.limit} s; nothing more is started")
        if out.returncode != 0:
            sys.stderr.write(out.stdout + out.stderr)
            sys.exit(f"{name}: exit status {out.returncode}; nothing more is started")
        res["cases"][name] = json.loads([l for l in out.stdout.splitlines() if l.startswith("{")][-1])
        print(f"{name}: {res['cases'][name]}", file=sys.stderr, flush=True)
    res["longest_capped_launch_s"] = max(c["longest_capped_launch_s"] for c in res["cases"].values())
    line = json.dumps(res)
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
