"""Forward + backward of the fused point embedding under a scalar loss:
point_embed.point_embed(points, W, b, pos=pos, cond=cond).square().mean() with the gradient taken into W, b, pos and cond
(`params`), and separately also into the points (`params_points`) (csrc/point_embed.hip: one kernel forward, one backward
that reads the incoming gradient once for the points, the weight, the bias and cond, a second read for pos) against torch
autograd of the literal form on the same GPU, F.linear(points, W, b) + pos[:N] + cond[:, None]
(transformer_pointcloud_nova.py:562-565, :712-716, :759-760), at C = 3, E = 768 and

    32 x 2048 points      a training batch of generated clouds
    1 x 15000 points      one cloud at the reference's point_cloud_size

    python3 tools/point_embed_bench.py [--out profiles/point_embed_bench.json]     every case, one JSON line
    python3 tools/point_embed_bench.py --case 32x2048 [--hip-only]                  one case in this process, for a kernel-time run:
    rocprofv3 --kernel-trace --stats --output-format csv -d DIR -o embed -- python3 tools/point_embed_bench.py --case 32x2048 --hip-only

Every case runs in a child process of its own under a time limit (--limit seconds); after a case that fails or runs out of
time nothing more is started. One call is the loss forward and backward. After a warm-up, a timed window is as many calls in
a row as last about --window seconds, between two device events; the windows of the forms alternate, --reps of each (5 by
default): the best time per call and the spread (max - min) / min. The peak of torch.cuda.max_memory_allocated over one
call, above what is allocated before it (the inputs; the gradients of the call before are released first, so no call frees
memory below its own baseline), is recorded for both forms. The gradients of the two forms are compared
(largest difference relative to the largest entry). No ratio is fixed in advance: the times are reported, not asserted.

The forward kernel alone: `forward_s` is one point_embed call with bias, pos and cond under no_grad (the kernel and the
allocation of its output), timed the same way; its compulsory traffic is the S N E 4 bytes it stores plus the N E 4 bytes of
pos it reads once (the other inputs are small), and `forward_bytes_per_s` over HBM_BYTES_PER_S is its share of the
achievable HBM rate (6.3 TB/s of 8.0 peak). The backward kernels alone are timed by the rocprofv3 run above; their
compulsory traffic is `backward_bytes` (one read of g, the partials written and read back) and `pos_backward_bytes` (the
second read of g and the N E 4 bytes stored)."""
import argparse
import json
import os
import subprocess
import sys

from pointset_bench_common import ball_clouds, best_and_spread, calls_per_window, window

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASES = {"32x2048": (32, 2048, 768), "1x15000": (1, 15000, 768)}  # clouds, points, channels
HBM_BYTES_PER_S = 6.3e12  # achievable (float4 copy); 8.0e12 is the specification


def torch_embed(points, W, b, pos, cond):
    """The reference's computation, op for op."""
    import torch.nn.functional as F

    return F.linear(points, W, b) + pos[:points.shape[1]] + cond[:, None]


def step(form, leaves, wanted):
    for t in leaves.values():
        t.grad = None
        t.requires_grad_(False)
    for name in wanted:
        leaves[name].requires_grad_(True)
    loss = form(leaves["points"], leaves["W"], leaves["b"], leaves["pos"], leaves["cond"]).square().mean()
    loss.backward()
    return [loss.detach()] + [leaves[name].grad for name in wanted]


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
    from nova_pointcloud_amd import point_embed as pe

    S, N, E = CASES[name]
    gen = torch.Generator().manual_seed(E + N)
    layer = torch.nn.Linear(3, E)
    leaves = {"points": ball_clouds(S, N, N + E), "W": layer.weight.detach().cuda(), "b": layer.bias.detach().cuda(),
              "pos": (torch.randn(N, E, generator=gen) * 0.02).cuda(), "cond": (torch.randn(S, E, generator=gen) * 0.02).cuda()}
    hip_form = lambda p, W, b, pos, cond: pe.point_embed(p, W, b, pos=pos, cond=cond)
    wanted = {"params": ("W", "b", "pos", "cond"), "params_points": ("W", "b", "pos", "cond", "points")}
    forms = {}
    for mode, names in wanted.items():
        forms["hip_" + mode] = lambda names=names: step(hip_form, leaves, names)
        if not hip_only:
            forms["torch_" + mode] = lambda names=names: step(torch_embed, leaves, names)
    for fn in forms.values():  # warm-up: library load, first launches, the allocator's blocks
        fn()
        fn()

    def forward_only():
        with torch.no_grad():
            return hip_form(*leaves.values())

    forward_only()
    inner = {key: calls_per_window(fn, seconds) for key, fn in forms.items()}
    inner_f = calls_per_window(forward_only, seconds)
    times, times_f = {key: [] for key in forms}, []
    for _ in range(reps):  # the forms alternate, so drift of the clock or the host meets all alike
        for key, fn in forms.items():
            times[key].append(window(fn, inner[key])[1])
        times_f.append(window(forward_only, inner_f)[1])
    tf, spread_f = best_and_spread(times_f)
    props = torch.cuda.get_device_properties(0)
    stored, chunks = S * N * E * 4, (N + pe.EMBED_CHUNK - 1) // pe.EMBED_CHUNK
    partials = S * chunks * E * 4 * 4  # C + 1 = 4 floats per channel and chunk
    case = {"clouds": S, "points": N, "inputs": 3, "channels": E, "forward_s": tf, "forward_spread": round(spread_f, 4),
            "forward_calls_per_window": inner_f, "forward_bytes": stored + N * E * 4 + S * N * 12,
            "forward_bytes_per_s": (stored + N * E * 4 + S * N * 12) / tf,
            "forward_share_of_hbm_rate": round((stored + N * E * 4 + S * N * 12) / tf / HBM_BYTES_PER_S, 4), "hbm_bytes_per_s": HBM_BYTES_PER_S,
            "backward_bytes": stored + 2 * partials + S * N * 12, "backward_partial_bytes": partials, "pos_backward_bytes": stored + N * E * 4,
            "device": props.name, "compute_units": props.multi_processor_count, "modes": {}}
    rel = lambda a, b: float((a - b).abs().max() / b.abs().max())

    def peak_of(fn):
        # The gradients of the call before go first: a call starts by dropping them, and whether that frees memory below
        # the baseline depends on who else still holds them, which is not a property of the form.
        for t in leaves.values():
            t.grad = None
        return peak_rise(fn)

    for mode, names in wanted.items():
        before = dict(pe.stats)
        got, hip_peak = peak_of(forms["hip_" + mode])
        launches = {key: pe.stats[key] - before[key] for key in before}
        got = [t.clone() for t in got]
        t, spread = best_and_spread(times["hip_" + mode])
        m = {"gradients_into": list(names), "hip_s": t, "hip_spread": round(spread, 4), "hip_calls_per_window": inner["hip_" + mode],
             "hip_launches_per_call": launches, "hip_peak_rise_bytes": hip_peak}
        if not hip_only:
            ref, torch_peak = peak_of(forms["torch_" + mode])
            tt, t_spread = best_and_spread(times["torch_" + mode])
            diffs = {n: rel(a, b) for n, a, b in zip(("loss",) + names, got, ref)}
            m.update({"torch_s": tt, "torch_spread": round(t_spread, 4), "torch_calls_per_window": inner["torch_" + mode],
                      "torch_peak_rise_bytes": torch_peak, "speedup": round(tt / t, 2), "memory_ratio": round(torch_peak / max(1, hip_peak), 2),
                      "difference_over_largest_entry": diffs, "largest_gradient_difference": max(diffs.values()),
                      "hip_wins_beyond_spread": bool(tt > t * (1 + spread + t_spread)),
                      "torch_wins_beyond_spread": bool(t > tt * (1 + spread + t_spread))})
        case["modes"][mode] = m
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
