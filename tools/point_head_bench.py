"""Forward + backward of the fused point head under a scalar loss:
point_head.point_head(x, W, b).square().mean() with the gradient taken into x, W and b, with and without grad_clamp=15
(csrc/point_head.hip: one kernel forward, one backward that reads x once and writes its gradient once, the clamp applied
as the incoming gradient is loaded) against torch autograd of the literal form on the same GPU, F.linear(x, W, b) with the
reference's GradientGuard hook (transformer_pointcloud_nova.py:444, :512-515; train_newloss.py:34-43), at C = 3, E = 768, for
x in float32 and in bfloat16 (W and b float32; the torch form casts x to float32 first, as autocast's caller would), and

    32 x 2048 rows        a training batch of generated clouds
    1 x 15000 rows        one cloud at the reference's point_cloud_size

    python3 tools/point_head_bench.py [--out profiles/point_head_bench.json]       every case, one JSON line
    python3 tools/point_head_bench.py --case 32x2048_f32 [--hip-only]               one case in this process, for a kernel-time run:
    rocprofv3 --kernel-trace --stats --output-format csv -d DIR -o head -- python3 tools/point_head_bench.py --case 32x2048_f32 --hip-only

Every case runs in a child process of its own under a time limit (--limit seconds); after a case that fails or runs out of
time nothing more is started. One call is the loss forward and backward. After a warm-up, a timed window is as many calls in
a row as last about --window seconds, between two device events; the windows of the forms alternate, --reps of each (5 by
default): the best time per call and the spread (max - min) / min. The peak of torch.cuda.max_memory_allocated over one
call, above what is allocated before it (the inputs; the gradients of the call before are released first), is recorded for
both forms. The gradients of the two forms are compared (largest difference relative to the largest entry). No ratio is
fixed in advance: the times are reported, not asserted.

The forward kernel alone: `forward_s` is one point_head call under no_grad (the kernel and the allocation of its output),
timed the same way; its compulsory traffic is the S N E elements of x it reads (the output and the weight are small), and
`forward_bytes_per_s` over HBM_BYTES_PER_S is its share of the achievable HBM rate (6.3 TB/s of 8.0 peak). The backward
kernels alone are timed by the rocprofv3 run above; their compulsory traffic is `backward_bytes` (one read of x, one store
of its gradient, the partials written and read back)."""
import argparse
import json
import os
import subprocess
import sys

from pointset_bench_common import best_and_spread, calls_per_window, window

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SHAPES = {"32x2048": (32, 2048, 768), "1x15000": (1, 15000, 768)}  # clouds, rows, channels
CASES = {f"{shape}_{dtype}": (shape, dtype) for shape in SHAPES for dtype in ("f32", "bf16")}
HBM_BYTES_PER_S = 6.3e12  # achievable (float4 copy); 8.0e12 is the specification
GUARD = 15.0  # the reference's GradientGuard(max_grad_norm=15.0)


def torch_head(x, W, b, clamp):
    """The reference's computation, op for op: the linear layer, and GradientGuard's hook on its output."""
    import torch
    import torch.nn.functional as F

    out = F.linear(x.float(), W, b)
    if clamp is not None and out.requires_grad:
        out.register_hook(lambda g: torch.clamp(g, -clamp, clamp))
    return out


def step(form, leaves, clamp):
    for t in leaves.values():
        t.grad = None
    loss = form(leaves["x"], leaves["W"], leaves["b"], clamp).square().mean()
    loss.backward()
    return [loss.detach()] + [t.grad for t in leaves.values()]


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
    from nova_pointcloud_amd import point_head as ph

    shape, dtype_name = CASES[name]
    S, N, E = SHAPES[shape]
    dtype = {"f32": torch.float32, "bf16": torch.bfloat16}[dtype_name]
    gen = torch.Generator().manual_seed(E + N)
    layer = torch.nn.Linear(E, 3)
    leaves = {"x": torch.randn(S, N, E, generator=gen).to(dtype).cuda().requires_grad_(True), "W": layer.weight.detach().cuda().requires_grad_(True),
              "b": layer.bias.detach().cuda().requires_grad_(True)}
    hip_form = lambda x, W, b, clamp: ph.point_head(x, W, b, grad_clamp=clamp)
    modes = {"plain": None, "clamp15": GUARD}
    forms = {}
    for mode, clamp in modes.items():
        forms["hip_" + mode] = lambda clamp=clamp: step(hip_form, leaves, clamp)
        if not hip_only:
            forms["torch_" + mode] = lambda clamp=clamp: step(torch_head, leaves, clamp)
    for fn in forms.values():  # warm-up: library load, first launches, the allocator's blocks
        fn()
        fn()

    def forward_only():
        with torch.no_grad():
            return hip_form(leaves["x"], leaves["W"], leaves["b"], None)

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
    rows_bytes, chunks = S * N * E * leaves["x"].element_size(), (N + ph.HEAD_CHUNK - 1) // ph.HEAD_CHUNK
    partials = S * chunks * 3 * (E + 1) * 4
    small = S * N * 3 * 4  # the output, or the incoming gradient
    case = {"clouds": S, "points": N, "channels": E, "outputs": 3, "x_dtype": dtype_name, "forward_s": tf, "forward_spread": round(spread_f, 4),
            "forward_calls_per_window": inner_f, "forward_bytes": rows_bytes + small, "forward_bytes_per_s": (rows_bytes + small) / tf,
            "forward_share_of_hbm_rate": round((rows_bytes + small) / tf / HBM_BYTES_PER_S, 4), "hbm_bytes_per_s": HBM_BYTES_PER_S,
            "backward_bytes": 2 * rows_bytes + 2 * partials + small, "backward_partial_bytes": partials,
            "device": props.name, "compute_units": props.multi_processor_count, "modes": {}}
    rel = lambda a, b: float((a.float() - b.float()).abs().max() / b.float().abs().max())

    def peak_of(fn):
        for t in leaves.values():  # the gradients of the call before go first (point_embed_bench.py)
            t.grad = None
        return peak_rise(fn)

    for mode in modes:
        before = dict(ph.stats)
        got, hip_peak = peak_of(forms["hip_" + mode])
        launches = {key: ph.stats[key] - before[key] for key in before}
        got = [t.clone() for t in got]
        t, spread = best_and_spread(times["hip_" + mode])
        m = {"grad_clamp": modes[mode], "gradients_into": list(leaves), "hip_s": t, "hip_spread": round(spread, 4), "hip_calls_per_window": inner["hip_" + mode],
             "hip_launches_per_call": launches, "hip_peak_rise_bytes": hip_peak}
        if not hip_only:
            ref, torch_peak = peak_of(forms["torch_" + mode])
            tt, t_spread = best_and_spread(times["torch_" + mode])
            diffs = {n: rel(a, b) for n, a, b in zip(("loss",) + tuple(leaves), got, ref)}
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
