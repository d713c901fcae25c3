"""k nearest neighbours of every point of a cloud set among the other points of its cloud (the local-density form): the HIP
kernel (csrc/knn.hip through metrics.knn_points) against the reference's form, torch.cdist + topk(k + 1, largest=False) on
the same GPU (transformer_pointcloud_nova.py:81-89), at

    32 x 2048 points, k = 8        a batch of generated clouds
    1 x 15000 points, k = 8        one published reference shape
    662 x 2048 points, k = 8, 32   a chair-sized test set

    python3 tools/knn_bench.py [--out profiles/knn_bench.json]     every case, one JSON line
    python3 tools/knn_bench.py --case 662x2048k8 [--hip-only]       one case in this process, for a kernel-time run:
    rocprofv3 --kernel-trace --stats --output-format csv -d DIR -o knn -- python3 tools/knn_bench.py --case 662x2048k8 --hip-only

Every case runs in a child process of its own under a time limit (--limit seconds); after a case that fails or runs out of
time nothing more is started. The kernel's output is checked by the validity rule of tests/test_pointset_knn.py on the
first clouds of the set: the indices are replayed in float64 and must be the k nearest up to 1e-6 relative. Both forms are
timed with device events after a warm-up: the best of --reps repetitions and the spread (max - min) / min. The HIP form is
timed as one launch for the whole set and as a user calls it (launches capped at metrics._KNN_CANDIDATES_PER_LAUNCH, int64
indices); each capped launch is also timed alone, and the longest one is what that constant is to be re-derived from.
No ratio is fixed in advance: the figures are reported, not asserted.
"""
import argparse
import json
import os
import subprocess
import sys

from pointset_bench_common import ball_clouds, timed

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASES = {"32x2048k8": (32, 2048, 8), "1x15000k8": (1, 15000, 8), "662x2048k8": (662, 2048, 8), "662x2048k32": (662, 2048, 32)}
REL = 1e-6


def torch_knn(x, k, chunk):
    """The reference's form, `chunk` clouds at a time (the [chunk, N, N] float32 matrix is what it has to hold)."""
    import torch

    idx, d = [], []
    for c0 in range(0, x.shape[0], chunk):
        v, i = torch.cdist(x[c0:c0 + chunk], x[c0:c0 + chunk]).topk(k + 1, dim=-1, largest=False)
        idx.append(i[..., 1:])
        d.append(v[..., 1:])
    return torch.cat(idx), torch.cat(d)


def worst_excess(x, idx, d2, k, n_clouds=4):
    """Over the first clouds: (largest d64[idx] / k-th smallest d64 - 1, largest |d2 - d64[idx]| / d64[idx]) of the float64 replay."""
    import torch

    x64 = x[:n_clouds].double()
    d = torch.zeros(x64.shape[0], x64.shape[1], x64.shape[1], dtype=torch.float64, device=x.device)
    for c in range(3):
        d += (x64[:, :, None, c] - x64[:, None, :, c]) ** 2
    d.diagonal(dim1=1, dim2=2).fill_(float("inf"))
    got = d.gather(-1, idx[:n_clouds])
    kth = d.topk(k, dim=-1, largest=False).values[..., -1:]
    return float((got / kth).max()) - 1, float(((d2[:n_clouds].double() - got).abs() / got).max())


def run_case(name, reps, hip_only):
    import torch

    sys.path.insert(0, ROOT)
    from nova_pointcloud_amd import metrics

    S, N, k = CASES[name]
    x = ball_clouds(S, N, N + k)
    metrics.knn_points(x[:2], k=k)  # warm-up (library load, first launch)
    (idx, d2), t, spread = timed(lambda: metrics.knn_points(x, k=k, max_clouds_per_launch=S), reps)
    _, t_api, _ = timed(lambda: metrics.knn_points(x, k=k), reps)
    per = max(1, metrics._KNN_CANDIDATES_PER_LAUNCH // (N * N))
    launches = [timed(lambda: metrics.knn_points(x[s0:s0 + per], k=k, max_clouds_per_launch=per), reps)[1] for s0 in range(0, S, per)]
    rung, queries = metrics.knn_kernel_shape(min(S, per), N, k)
    case = {"clouds": S, "points": N, "k": k, "list_rung": rung, "queries_per_workgroup": queries, "hip_one_launch_s": t,
            "hip_spread": round(spread, 4), "hip_api_s": t_api, "clouds_per_capped_launch": per, "capped_launches": len(launches),
            "longest_capped_launch_s": max(launches), "candidates_per_s": S * N * N / t}
    excess, d_err = worst_excess(x, idx, d2, k)
    case.update({"hip_worst_excess_over_kth": excess, "hip_worst_distance_error": d_err})
    assert excess <= REL and d_err <= REL, case
    if not hip_only:
        chunk = max(1, (1 << 32) // (N * N))  # 16 GiB of float32 matrix at a time
        torch_knn(x[:2], k, chunk)
        (t_idx, _), tt, t_spread = timed(lambda: torch_knn(x, k, chunk), reps)
        case.update({"torch_s": tt, "torch_spread": round(t_spread, 4), "torch_clouds_per_chunk": min(S, chunk), "speedup": round(tt / t, 2),
                     "share_of_indices_equal_to_torch": float((idx == t_idx).double().mean()),
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

    res = {"reps": args.reps, "launch_cap_candidates": metrics._KNN_CANDIDATES_PER_LAUNCH, "cases": {}}
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
