"""Forward + backward of the exact-assignment EMD training loss: losses.emd_loss(...).mean() (the auction of csrc/assign.hip
for the assignment, csrc/matched.hip for the value and the gradient; nothing of size n^2 is stored) against the reference's
form made differentiable on the same GPU, emd_approx of train_newloss.py:352-377 with its numpy tail replaced by a gather:
torch.cdist of the clamped clouds, the cost matrix copied to the host, scipy's linear_sum_assignment sample after sample,
the partners gathered by the result, norm, mean, torch autograd. At

    32 x 2048 points      a training batch of generated clouds against their targets
    8 x 4096 points       the largest clouds the auction takes

    python3 tools/emd_loss_bench.py [--out profiles/emd_loss_bench.json]    every case, one JSON line
    python3 tools/emd_loss_bench.py --case 32x2048 [--hip-only]             one case in this process

Every case runs in a child process of its own under a time limit (--limit seconds); after a case that fails or runs out of
time nothing more is started. One call is the loss of (pred, target) and its backward into pred, between two device events
(a call holds host work on both sides: the auction's launch loop reads a flag, the baseline waits for scipy). After one
warm-up call each, the forms alternate, --reps calls of each: the best time and the spread (max - min) / min. The same way,
on their own: the auction (metrics.optimal_assignment on the detached clouds) and the matched-pair part (matched_distance
under a known assignment, mean, backward); the auction's share is its best time over the whole call's. The two losses are
two optimal means of nearly the same costs (cdist expands |x|^2 + |y|^2 - 2 x.y, the auction quantises to 2^-18): their
difference, the share of points the two assignments give another partner, and the largest difference of the two gradients
relative to the largest entry (a point with another partner is pulled another way) are reported. No ratio is fixed
in advance: the times are reported, not asserted.
"""
import argparse
import json
import os
import subprocess
import sys

from pointset_bench_common import shell_clouds, timed

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASES = {"32x2048": (32, 2048), "8x4096": (8, 4096)}


def torch_emd_loss(pred, target):
    """emd_approx (train_newloss.py:352-377) with the matched distances taken by gather on the device, so that autograd sees them."""
    import numpy as np
    import torch
    from scipy.optimize import linear_sum_assignment

    x, y = torch.clamp(pred, -2.0, 2.0), torch.clamp(target, -2.0, 2.0)
    cost = torch.clamp(torch.cdist(x, y), min=1e-8).detach().cpu().numpy()
    index = torch.from_numpy(np.stack([linear_sum_assignment(c)[1] for c in cost]).astype(np.int64)).to(pred.device)
    torch_emd_loss.index = index  # for the comparison of the two assignments
    matched = torch.gather(y, 1, index[:, :, None].expand(-1, -1, 3))
    return torch.clamp((x - matched).norm(dim=-1), min=1e-8).mean(dim=1).mean()


def step(loss_fn, pred, target):
    pred.grad = None
    loss = loss_fn(pred, target)
    loss.backward()
    return loss.detach(), pred.grad


def run_case(name, reps, hip_only):
    sys.path.insert(0, ROOT)
    from nova_pointcloud_amd import losses, metrics

    B, n = CASES[name]
    pred, target = shell_clouds(B, n, n + 1).requires_grad_(True), shell_clouds(B, n, n + 2)
    index, _, rounds = metrics.optimal_assignment(pred.detach(), target, clamp=2.0, return_rounds=True)
    forms = {"hip": lambda: step(lambda p, t: losses.emd_loss(p, t).mean(), pred, target),
             "auction": lambda: metrics.optimal_assignment(pred.detach(), target, clamp=2.0),
             "matched": lambda: step(lambda p, t: losses.matched_distance(p, t, index, 2.0, 1e-8).mean(), pred, target)}
    if not hip_only:
        forms["torch"] = lambda: step(torch_emd_loss, pred, target)
    for k, fn in forms.items():  # warm-up: library load, first launches, the allocator's blocks
        fn()
        print(f"{name}: {k} warm", file=sys.stderr, flush=True)
    times = {k: [] for k in forms}
    for r in range(reps):  # the forms alternate, so drift of the clock or the host meets all of them alike
        for k, fn in forms.items():
            times[k].append(timed(fn, 1)[1])
        print(f"{name}: rep {r} " + " ".join(f"{k} {times[k][-1]:.4f}" for k in forms), file=sys.stderr, flush=True)
    best = {k: min(v) for k, v in times.items()}
    spread = {k: round((max(v) - min(v)) / min(v), 4) for k, v in times.items()}
    loss, grad = forms["hip"]()
    grad, hip_index = grad.clone(), losses.emd_loss(pred.detach(), target, return_assignment=True)[1]
    case = {"clouds": B, "points": n, "hip_s": best["hip"], "hip_spread": spread["hip"], "auction_s": best["auction"],
            "auction_spread": spread["auction"], "auction_share": round(best["auction"] / best["hip"], 4),
            "matched_fwd_bwd_s": best["matched"], "matched_spread": spread["matched"],
            "auction_rounds_max": int(rounds.max()), "loss": float(loss)}
    if not hip_only:
        t_loss, t_grad = forms["torch"]()
        case.update({"torch_s": best["torch"], "torch_spread": spread["torch"], "speedup": round(best["torch"] / best["hip"], 2),
                     "loss_difference": abs(float(loss) - float(t_loss)),
                     "gradient_difference_over_largest_entry": float((grad - t_grad).abs().max() / t_grad.abs().max()),
                     "share_of_points_with_another_partner": float((hip_index != torch_emd_loss.index).float().mean()),
                     "hip_wins_beyond_spread": bool(best["torch"] > best["hip"] * (1 + spread["hip"] + spread["torch"]))})
    return case


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--case", choices=sorted(CASES))
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--limit", type=int, default=900, help="seconds one case may take")
    ap.add_argument("--hip-only", action="store_true")
    ap.add_argument("--out")
    args = ap.parse_args()
    if args.reps < 5 and not args.hip_only:
        ap.error("--reps must be at least 5")
    if args.case:
        print(json.dumps(run_case(args.case, args.reps, args.hip_only)))
        return
    res = {"reps": args.reps, "cases": {}}  # no GPU work in this process: the cases run in children
    for name in CASES:
        cmd = [sys.executable, os.path.abspath(__file__), "--case", name, "--reps", str(args.reps)] + (["--hip-only"] if args.hip_only else [])
        try:
            out = subprocess.run(cmd, stdout=subprocess.PIPE, text=True, timeout=args.limit)  # the child's progress lines go straight to stderr
        except subprocess.TimeoutExpired:
            sys.exit(f"{name}: no result within {args.limit} s; nothing more is started")
        if out.returncode != 0:
            sys.stderr.write(out.stdout)
            sys.exit(f"{name}: exit status {out.returncode}; nothing more is started")
        res["cases"][name] = json.loads([l for l in out.stdout.splitlines() if l.startswith("{")][-1])
        print(f"{name}: {res['cases'][name]}", file=sys.stderr, flush=True)
        if args.out:  # after every case: a later case that runs out of time leaves the earlier ones on file
            with open(args.out, "w") as f:
                f.write(json.dumps(res) + "\n")
    print(json.dumps(res))


if __name__ == "__main__":
    main()
