"""All-pairs EMD (approxmatch) matrices at a chair-sized test set (S_r = S_s = 662 clouds of 2048 points): the HIP
kernel (csrc/emd.hip through metrics.emd_matrix) timed with device events after a warm-up, and a batched float32 torch
restatement of the same algorithm on the GPU over a subset of the D_rs pairs, outputs compared, in one process.

    python3 tools/emd_matrix_bench.py [--out FILE]            both paths, one JSON line
    python3 tools/emd_matrix_bench.py --hip-only              the HIP matrices only, for a kernel-time run:
    rocprofv3 --kernel-trace --stats --output-format csv -d DIR -o emd -- python3 tools/emd_matrix_bench.py --hip-only

Rates are (k, l, level) evaluations per second: 10 levels x N^2 point pairs per cloud pair. The bound is a
vector-issue bound, not measured: 26 plain f32 operations per evaluation across passes A + B + C at 32 lanes/clk per
SIMD (packed f32) plus 4 transcendentals (3 exp, 1 sqrt) at 8 cycles per wave64 instruction = 1.3125 SIMD-cycles per
evaluation, 1024 SIMDs at 2.4 GHz (1.87e12 evaluations/s).
"""
import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from nova_pointcloud_amd import metrics  # noqa: E402
from pointset_bench_common import shell_clouds, timed_once  # noqa: E402

LEVELS = 10
SIMD_CYCLES_PER_EVAL = 26 / 32 + 4 * 8 / 64
SIMDS, CLOCK = 1024, 2.4e9


def torch_emd(x, y):
    """EMD(x[p], y[p]) for x, y [P, n, 3]: the algorithm of include/nova_hip.h in batched float32 torch."""
    d2 = ((x[:, :, None, :] - y[:, None, :, :]) ** 2).sum(-1)
    dist = d2.sqrt()
    remL = torch.ones(x.shape[:2], device=x.device)
    remR = torch.ones(y.shape[:2], device=x.device)
    cost = torch.zeros(x.shape[0], device=x.device)
    for j in range(7, -3, -1):
        E = torch.exp((-(4.0 ** j) if j > -2 else 0.0) * d2)
        ratioL = remL / (1e-9 + torch.bmm(E, remR[:, :, None])[:, :, 0])
        s = remR * torch.bmm(ratioL[:, None, :], E)[:, 0, :]
        ratioR = torch.clamp(remR / (s + 1e-9), max=1.0) * remR
        remR = torch.clamp(remR - s, min=0.0)
        w = E * ratioL[:, :, None] * ratioR[:, None, :]
        cost = cost + (w * dist).sum((1, 2))
        remL = torch.clamp(remL - w.sum(2), min=0.0)
    return cost / x.shape[1]


def torch_emd_pairs(ref, smp, pairs, chunk):
    out = torch.empty(len(pairs), device=ref.device)
    for i in range(0, len(pairs), chunk):
        a = torch.tensor([p[0] for p in pairs[i:i + chunk]], device=ref.device)
        b = torch.tensor([p[1] for p in pairs[i:i + chunk]], device=ref.device)
        out[i:i + chunk] = torch_emd(ref[a], smp[b])
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--S", type=int, default=662)
    ap.add_argument("--n", type=int, default=2048)
    ap.add_argument("--torch-pairs", type=int, default=64, help="D_rs pairs of the torch comparison")
    ap.add_argument("--chunk", type=int, default=8, help="cloud pairs per torch step")
    ap.add_argument("--hip-only", action="store_true")
    ap.add_argument("--out")
    args = ap.parse_args()
    S, n = args.S, args.n
    ref, smp = shell_clouds(S, n, 1), shell_clouds(S, n, 2)
    metrics.emd_matrix(ref[:32], smp[:32])  # warm-up (library load, first launches)
    torch.cuda.synchronize()
    d_rs, t_rs = timed_once(lambda: metrics.emd_matrix(ref, smp))
    (d_rr, d_ss), t_rr_ss = timed_once(lambda: (metrics.emd_matrix(ref), metrics.emd_matrix(smp)))
    evals_rs = S * S * n * n * LEVELS
    bound = SIMDS * CLOCK / SIMD_CYCLES_PER_EVAL
    t_all = t_rs + t_rr_ss
    res = {"S_r": S, "S_s": S, "N": n, "hip_rs_s": round(t_rs, 4), "hip_rr_ss_s": round(t_rr_ss, 4), "hip_all_s": round(t_all, 4),
           "hip_all_evals_per_s": 3 * evals_rs / t_all,
           "bound": "vector-issue bound (not measured): 26 f32 ops at 32 lanes/clk/SIMD + 4 transcendentals at 8 cyc/wave64 per "
                    "(k, l, level), 1024 SIMDs at 2.4 GHz",
           "bound_evals_per_s": bound, "bound_all_s": round(3 * evals_rs / bound, 2),
           "hip_all_fraction_of_bound": round(3 * evals_rs / t_all / bound, 4),
           "launch_pairs": max(1, metrics._EMD_EVALUATIONS_PER_LAUNCH // (n * n * LEVELS) // metrics._emd_resident_workgroups(ref.device, n))
           * metrics._emd_resident_workgroups(ref.device, n),
           "resident_workgroups": metrics._emd_resident_workgroups(ref.device, n),
           "finite": bool(torch.isfinite(d_rs).all() and torch.isfinite(d_rr).all() and torch.isfinite(d_ss).all())}
    if not args.hip_only:
        g = torch.Generator().manual_seed(3)
        pairs = [(int(a), int(b)) for a, b in zip(torch.randint(S, (args.torch_pairs,), generator=g),
                                                   torch.randint(S, (args.torch_pairs,), generator=g))]
        torch_emd_pairs(ref, smp, pairs[:args.chunk], args.chunk)  # warm-up
        torch.cuda.synchronize()
        d_torch, t_torch = timed_once(lambda: torch_emd_pairs(ref, smp, pairs, args.chunk))
        hip_sub = torch.stack([d_rs[a, b] for a, b in pairs])
        rel = ((d_torch - hip_sub).abs() / hip_sub).max().item()
        per_pair_torch, per_pair_hip = t_torch / len(pairs), t_rs / (S * S)
        res.update({"torch_pairs": len(pairs), "torch_s": round(t_torch, 4), "torch_s_per_pair": per_pair_torch,
                    "hip_s_per_pair": per_pair_hip, "speedup_per_pair": round(per_pair_torch / per_pair_hip, 1),
                    "torch_vs_hip_max_rel": rel})
        assert rel < 1e-3, rel
    line = json.dumps(res)
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
