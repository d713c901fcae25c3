"""Forward + backward of the Chamfer training loss: losses.chamfer_loss (csrc/nearest_match.hip: no [N, M] matrix in either
pass) against the reference's literal form, distChamfer of train_newloss.py:316-349 on torch.cdist under torch autograd, on
the same GPU, at

    32 x 2048 points      a training batch of generated clouds against their targets
    1 x 15000 points      one published reference shape

    python3 tools/chamfer_loss_bench.py [--out profiles/chamfer_loss_bench.json]    every case, one JSON line
    python3 tools/chamfer_loss_bench.py --case 32x2048 [--hip-only]                 one case in this process, for a kernel-time run:
    rocprofv3 --kernel-trace --stats --output-format csv -d DIR -o chamfer -- python3 tools/chamfer_loss_bench.py --case 32x2048 --hip-only

Every case runs in a child process of its own under a time limit (--limit seconds); after a case that fails or runs out of
time nothing more is started. One call is the loss of (pred, target) and its backward into pred. After a warm-up, a timed
window is as many calls in a row as last about --window seconds, between two device events; the windows of the two forms
alternate, --reps of each: the best time per call and the spread (max - min) / min, for both forms. The two losses must
agree within 2e-6 (the bound of tests/test_pointset_losses.py on the value); the largest difference of the two gradients,
relative to the largest entry, is reported. No ratio is fixed in advance: the times are reported, not asserted.
"""
import argparse
import json
import os
import subprocess
import sys

from pointset_bench_common import best_and_spread, calls_per_window, shell_clouds, window

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASES = {"32x2048": (32, 2048), "1x15000": (1, 15000)}


def torch_chamfer_loss(a, b):
    """robust_chamfer_distance on distChamfer, statement by statement (train_newloss.py:316-349, 381-384)."""
    import torch

    x, y = torch.clamp(a, -1.0, 1.0), torch.clamp(b, -1.0, 1.0)
    x = x / torch.clamp(torch.norm(x, dim=-1, keepdim=True), min=1e-8)
    y = y / torch.clamp(torch.norm(y, dim=-1, keepdim=True), min=1e-8)
    dist = torch.clamp(torch.cdist(x, y), min=1e-8)
    log_dist = torch.clamp(torch.log(dist + 1e-8), min=-10, max=10)
    dl, dr = log_dist.min(2)[0].exp().mean(), log_dist.min(1)[0].exp().mean()
    return (dl.mean() + dr.mean()) / 2


def step(loss_fn, pred, target):
    pred.grad = None
    loss = loss_fn(pred, target)
    loss.backward()
    return loss.detach(), pred.grad


def run_case(name, reps, hip_only, seconds):
    import torch

    sys.path.insert(0, ROOT)
    from nova_pointcloud_amd import losses

    B, N = CASES[name]
    pred, target = shell_clouds(B, N, N + 1).requires_grad_(True), shell_clouds(B, N, N + 2)
    hip_step = lambda: step(losses.chamfer_loss, pred, target)
    hip_forward = lambda: losses.chamfer_loss(pred.detach(), target)
    torch_step = lambda: step(torch_chamfer_loss, pred, target)
    forms = {"hip": hip_step, "hip_forward_only": hip_forward} if hip_only else {"hip": hip_step, "hip_forward_only": hip_forward, "torch": torch_step}
    for fn in forms.values():  # warm-up: library load, first launches, the allocator's blocks
        fn()
        fn()
    before = losses.stats["nearest_match_launches"]
    loss, grad = hip_step()
    launches, grad = losses.stats["nearest_match_launches"] - before, grad.clone()
    inner = {k: calls_per_window(fn, seconds) for k, fn in forms.items()}
    times = {k: [] for k in forms}
    for _ in range(reps):  # the forms alternate, so drift of the clock or the host meets all of them alike
        for k, fn in forms.items():
            times[k].append(window(fn, inner[k])[1])
    t, spread = best_and_spread(times["hip"])
    case = {"clouds": B, "points": N, "hip_s": t, "hip_spread": round(spread, 4), "hip_calls_per_window": inner["hip"],
            "hip_forward_only_s": min(times["hip_forward_only"]), "hip_forward_launches_per_call": launches,
            "pair_visits_per_s": 4 * B * N * N / t, "loss": float(loss)}
    if not hip_only:
        torch.cuda.reset_peak_memory_stats()
        t_loss, t_grad = torch_step()
        tt, t_spread = best_and_spread(times["torch"])
        case.update({"torch_s": tt, "torch_spread": round(t_spread, 4), "torch_calls_per_window": inner["torch"],
                     "torch_peak_bytes": torch.cuda.max_memory_allocated(), "speedup": round(tt / t, 2),
                     "loss_difference": abs(float(loss) - float(t_loss)),
                     "gradient_difference_over_largest_entry": float((grad - t_grad).abs().max() / t_grad.abs().max()),
                     "hip_wins_beyond_spread": bool(tt > t * (1 + spread + t_spread))})
        assert case["loss_difference"] <= 2e-6, case
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
