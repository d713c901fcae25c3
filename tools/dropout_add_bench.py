"""Forward + backward of the fused bias-dropout-residual under a scalar loss, both forms of the encoder layer's body:

    residual   dropout.bias_dropout_add(x, b, residual=r, p=0.1).square().mean()          gradients into x, b and r
    relu       dropout.bias_dropout_add(x, b, p=0.1, activation="relu").square().mean()   gradients into x and b

(csrc/dropout_add.hip: one kernel forward, one backward that regenerates the Philox mask or, with "relu", gates on the saved
output, and one sum over the bias gradient's 128-row chunks) against torch autograd of the literal forms on the same GPU,
r + F.dropout(x + b, 0.1) and F.dropout(F.relu(x + b), 0.1) (transformer_pointcloud_nova.py:433-441, :590-598: the
nn.TransformerEncoderLayer with dropout=0.1), for x, r and b in float32 and in bfloat16, at

    32 x 2048 rows        a training batch of generated clouds           D = 768 (d_model) and 3072 (dim_feedforward)
    1 x 15000 rows        one cloud at the reference's point_cloud_size  D = 768 and 3072

    python3 tools/dropout_add_bench.py [--out profiles/dropout_add_bench.json]      every case, one JSON line
    python3 tools/dropout_add_bench.py --case 32x2048x768_f32 [--hip-only]          one case in this process
    rocprofv3 --kernel-trace --stats --output-format csv -d DIR/CASE -o da -- python3 tools/dropout_add_bench.py --case CASE --kernels
                                                                                    a kernel-time run of one case: a few calls, HIP forms only
    python3 tools/dropout_add_bench.py --merge-kernel-stats DIR --out profiles/dropout_add_bench.json --csv profiles/dropout_add_kernel_stats.csv
                                                                                    no GPU: the kernels' rows of DIR/CASE/**kernel_stats.csv into one
                                                                                    CSV, and bytes over time into the JSON's cases

Every case runs in a child process of its own under a time limit (--limit seconds); after a case that fails or runs out of
time nothing more is started. One call is the loss forward and backward. After a warm-up, a timed window is as many calls in
a row as last about --window seconds, between two device events; the windows of the forms alternate, --reps of each (5 by
default): the best time per call and the spread (max - min) / min. The peak of torch.cuda.max_memory_allocated over one
call, above what is allocated before it (the inputs; the gradients of the call before are released first), is recorded for
both forms. The masks of the two forms differ (torch draws from the device generator), so their gradients are not compared
here; tests/test_dropout_add.py holds the kernels to the definition bit for bit. No ratio is fixed in advance: the times are
reported, not asserted.

Kernel times come from the rocprofv3 runs. The compulsory traffic of each kernel, n = rows D elements of the tensor's size:
forward residual 3 n (x, r, out), forward relu 2 n (x, out), backward residual 2 n (g, gx) plus the chunk partials, backward relu
3 n (g, the saved out, gx) plus the partials; over the kernel's average time and HBM_BYTES_PER_S it is the kernel's share of
the achievable streaming rate (6.3 TB/s of 8.0 peak)."""
import argparse
import csv
import glob
import json
import os
import subprocess
import sys

from pointset_bench_common import best_and_spread, calls_per_window, window

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SHAPES = {"32x2048x768": (32, 2048, 768), "32x2048x3072": (32, 2048, 3072), "1x15000x768": (1, 15000, 768), "1x15000x3072": (1, 15000, 3072)}
CASES = {f"{shape}_{dtype}": (shape, dtype) for shape in SHAPES for dtype in ("f32", "bf16")}
HBM_BYTES_PER_S = 6.3e12  # achievable (float4 copy); 8.0e12 is the specification
P = 0.1  # the reference's dropout
CHUNK = 128
ELEMENT_BYTES = {"f32": 4, "bf16": 2}
KERNEL_CALLS = 20


def kernel_bytes(shape, dtype_name):
    """Compulsory bytes of the four kernels of one case, keyed by (backward, relu)."""
    S, N, D = SHAPES[shape]
    n = S * N * D * ELEMENT_BYTES[dtype_name]
    partials = (S * N + CHUNK - 1) // CHUNK * D * 4
    return {(False, False): 3 * n + D * 4, (False, True): 2 * n + D * 4, (True, False): 2 * n + partials, (True, True): 3 * n + partials}


def torch_forms():
    import torch.nn.functional as F

    return {"residual": lambda x, b, r: r + F.dropout(x + b, P), "relu": lambda x, b, r: F.dropout(F.relu(x + b), P)}


def hip_forms():
    sys.path.insert(0, ROOT)
    from nova_pointcloud_amd import dropout

    return {"residual": lambda x, b, r: dropout.bias_dropout_add(x, b, residual=r, p=P),
            "relu": lambda x, b, r: dropout.bias_dropout_add(x, b, p=P, activation="relu")}


def step(form, leaves, into):
    for t in leaves.values():
        t.grad = None
    loss = form(leaves["x"], leaves["b"], leaves["r"]).square().mean()
    loss.backward(inputs=[leaves[k] for k in into])
    return [loss.detach()] + [leaves[k].grad for k in into]


def peak_rise(fn):
    """(result, bytes the peak of one call lies above what was allocated before it)."""
    import torch

    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    before = torch.cuda.memory_allocated()
    out = fn()
    torch.cuda.synchronize()
    return out, torch.cuda.max_memory_allocated() - before


def make_leaves(name):
    import torch

    shape, dtype_name = CASES[name]
    S, N, D = SHAPES[shape]
    dtype = {"f32": torch.float32, "bf16": torch.bfloat16}[dtype_name]
    gen = torch.Generator().manual_seed(D + N)
    new = lambda *s: torch.randn(*s, generator=gen).to(dtype).cuda().requires_grad_(True)
    return {"x": new(S, N, D), "b": new(D), "r": new(S, N, D)}  # the bias in the model's dtype, as an nn.Linear under bf16 holds it


def run_kernels(name):
    """A few calls of the HIP forms alone, for a rocprofv3 run."""
    import torch

    leaves = make_leaves(name)
    for mode, form in hip_forms().items():
        into = ("x", "b", "r") if mode == "residual" else ("x", "b")
        for _ in range(KERNEL_CALLS):
            step(form, leaves, into)
    torch.cuda.synchronize()
    return {"case": name, "calls": KERNEL_CALLS}


def run_case(name, reps, hip_only, seconds):
    import torch

    shape, dtype_name = CASES[name]
    S, N, D = SHAPES[shape]
    leaves = make_leaves(name)
    sys.path.insert(0, ROOT)
    from nova_pointcloud_amd import dropout

    modes = {"residual": ("x", "b", "r"), "relu": ("x", "b")}
    forms = {}
    for mode, into in modes.items():
        forms["hip_" + mode] = lambda f=hip_forms()[mode], into=into: step(f, leaves, into)
        if not hip_only:
            forms["torch_" + mode] = lambda f=torch_forms()[mode], into=into: step(f, leaves, into)
    torch.manual_seed(1)
    for fn in forms.values():  # warm-up: library load, first launches, the allocator's blocks
        fn()
        fn()
    inner = {key: calls_per_window(fn, seconds) for key, fn in forms.items()}
    times = {key: [] for key in forms}
    for _ in range(reps):  # the forms alternate, so drift of the clock or the host meets all alike
        for key, fn in forms.items():
            times[key].append(window(fn, inner[key])[1])
    props = torch.cuda.get_device_properties(0)
    nbytes = kernel_bytes(shape, dtype_name)
    case = {"clouds": S, "points": N, "columns": D, "dtype": dtype_name, "p": P, "tensor_bytes": S * N * D * ELEMENT_BYTES[dtype_name],
            "hbm_bytes_per_s": HBM_BYTES_PER_S, "device": props.name, "compute_units": props.multi_processor_count, "modes": {}}

    def peak_of(fn):
        for t in leaves.values():  # the gradients of the call before go first
            t.grad = None
        return peak_rise(fn)

    for mode, into in modes.items():
        before = dict(dropout.stats)
        got, hip_peak = peak_of(forms["hip_" + mode])
        launches = {key: dropout.stats[key] - before[key] for key in before}
        kept = float((got[1] != 0).float().mean())  # the share of x's gradient that is not zero: about 1 - p (half of that behind the ReLU)
        t, spread = best_and_spread(times["hip_" + mode])
        m = {"gradients_into": list(into), "hip_s": t, "hip_spread": round(spread, 4), "hip_calls_per_window": inner["hip_" + mode],
             "hip_launches_per_call": launches, "hip_peak_rise_bytes": hip_peak, "hip_nonzero_share_of_gx": round(kept, 4),
             "forward_kernel_bytes": nbytes[(False, mode == "relu")], "backward_kernel_bytes": nbytes[(True, mode == "relu")]}
        if not hip_only:
            ref, torch_peak = peak_of(forms["torch_" + mode])
            tt, t_spread = best_and_spread(times["torch_" + mode])
            m.update({"torch_s": tt, "torch_spread": round(t_spread, 4), "torch_calls_per_window": inner["torch_" + mode],
                      "torch_peak_rise_bytes": torch_peak, "torch_nonzero_share_of_gx": round(float((ref[1] != 0).float().mean()), 4),
                      "speedup": round(tt / t, 2), "memory_ratio": round(torch_peak / max(1, hip_peak), 2),
                      "hip_wins_beyond_spread": bool(tt > t * (1 + spread + t_spread)),
                      "torch_wins_beyond_spread": bool(t > tt * (1 + spread + t_spread))})
        case["modes"][mode] = m
    return case


def merge_kernel_stats(root, out_json, out_csv):
    """The rows of this project's kernels from root/CASE/**/*kernel_stats.csv into one CSV with the case in front, and into
    the JSON's cases as `kernels`: average time, compulsory bytes, bytes per second and the share of HBM_BYTES_PER_S."""
    res = json.load(open(out_json)) if out_json and os.path.exists(out_json) else {"cases": {}}
    rows_out = []
    for name, (shape, dtype_name) in CASES.items():
        found = sorted(glob.glob(os.path.join(root, name, "**", "*kernel_stats.csv"), recursive=True))
        if not found:
            continue
        nbytes = kernel_bytes(shape, dtype_name)
        kernels = {}
        for row in csv.DictReader(open(found[0])):
            kname = row["Name"]
            if "nova::" not in kname:
                continue
            rows_out.append([name] + [row[k] for k in ("Name", "Calls", "TotalDurationNs", "AverageNs", "MinNs", "MaxNs", "StdDev")])
            if "dropout_add_kernel" not in kname:
                kernels["bias_chunk_sum"] = {"kernel": kname, "calls": int(row["Calls"]), "average_s": float(row["AverageNs"]) / 1e9}
                continue
            flags = kname[kname.index("<") + 1:kname.index(">")].split(", ")  # T, BWD, RELU, WIDE
            bwd, relu = flags[1] == "true", flags[2] == "true"
            avg = float(row["AverageNs"]) / 1e9
            kernels[("backward_" if bwd else "forward_") + ("relu" if relu else "residual")] = {
                "kernel": kname[:kname.index("(")], "calls": int(row["Calls"]), "average_s": avg, "min_s": float(row["MinNs"]) / 1e9,
                "bytes": nbytes[(bwd, relu)], "bytes_per_s": nbytes[(bwd, relu)] / avg, "share_of_hbm_rate": round(nbytes[(bwd, relu)] / avg / HBM_BYTES_PER_S, 4)}
        res["cases"].setdefault(name, {})["kernels"] = kernels
    if out_csv:
        with open(out_csv, "w", newline="") as f:
            w = csv.writer(f, quoting=csv.QUOTE_NONNUMERIC)
            w.writerow(["Case", "Name", "Calls", "TotalDurationNs", "AverageNs", "MinNs", "MaxNs", "StdDev"])
            w.writerows(rows_out)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--case", choices=sorted(CASES))
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--window", type=float, default=0.2, help="seconds of back-to-back calls one timed window lasts")
    ap.add_argument("--limit", type=int, default=120, help="seconds one case may take")
    ap.add_argument("--hip-only", action="store_true")
    ap.add_argument("--kernels", action="store_true", help="with --case: a few calls of the HIP forms, for a profiler run")
    ap.add_argument("--merge-kernel-stats", metavar="DIR")
    ap.add_argument("--csv")
    ap.add_argument("--out")
    args = ap.parse_args()
    if args.merge_kernel_stats:
        line = json.dumps(merge_kernel_stats(args.merge_kernel_stats, args.out, args.csv))
        print(line)
        if args.out:
            with open(args.out, "w") as f:
                f.write(line + "\n")
        return
    if args.reps < 5 and not args.hip_only:
        ap.error("--reps must be at least 5")
    if args.case:
        print(json.dumps(run_kernels(args.case) if args.kernels else run_case(args.case, args.reps, args.hip_only, args.window)))
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
