"""All-pairs Chamfer matrices at a chair-sized test set (S_r = S_s = 662 clouds of 2048 points): the HIP kernel
(csrc/chamfer.hip through metrics.chamfer_matrix) against a chunked torch form (torch.cdist + min over batches of
cloud pairs), in one process, outputs compared, both timed with device events after a warm-up.

    python3 tools/chamfer_matrix_bench.py [--out FILE]            both paths, one JSON line
    python3 tools/chamfer_matrix_bench.py --hip-only              the HIP matrices only, for a kernel-time run:
    rocprofv3 --kernel-trace --stats --output-format csv -d DIR -o cm -- python3 tools/chamfer_matrix_bench.py --hip-only

Rates are squared point distances per second; the bound is the vector-instruction rate for the difference form,
~8 vector operations per distance at 32 lanes/clk per SIMD x 1024 SIMDs (9.8e12 distances/s at 2.4 GHz).
"""
import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from nova_pointcloud_amd import metrics  # noqa: E402
from pointset_bench_common import shell_clouds, timed_once  # noqa: E402

VALU_BOUND = 8.0  # vector operations per distance
LANES_PER_CLK = 32 * 1024


def torch_chamfer(x, y, chunk):
    """The same matrix by torch.cdist + min, `chunk` y-clouds against one x-cloud per step."""
    cd = torch.empty(x.shape[0], y.shape[0], device=x.device)
    for a in range(x.shape[0]):
        for b0 in range(0, y.shape[0], chunk):
            d = torch.cdist(x[a:a + 1], y[b0:b0 + chunk]).square_()  # [chunk, N, M]
            cd[a, b0:b0 + chunk] = d.min(dim=2).values.mean(dim=1) + d.min(dim=1).values.mean(dim=1)
    return cd


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--S", type=int, default=662)
    ap.add_argument("--n", type=int, default=2048)
    ap.add_argument("--chunk", type=int, default=64, help="cloud pairs per torch step")
    ap.add_argument("--hip-only", action="store_true")
    ap.add_argument("--out")
    args = ap.parse_args()
    S, n = args.S, args.n
    ref, smp = shell_clouds(S, n, 1), shell_clouds(S, n, 2)
    metrics.chamfer_matrix(ref[:64], smp[:64])  # warm-up (library load, first launches)
    metrics.chamfer_matrix(ref[:64])
    torch.cuda.synchronize()
    d_rs, t_rs = timed_once(lambda: metrics.chamfer_matrix(ref, smp))
    (d_rr, d_ss), t_sym = timed_once(lambda: (metrics.chamfer_matrix(ref), metrics.chamfer_matrix(smp)))
    pairs_rs, pairs_sym = S * S, S * (S + 1)  # two triangles with their diagonals
    dist_rs, dist_all = pairs_rs * n * n, (pairs_rs + pairs_sym) * n * n
    bound = LANES_PER_CLK * 2.4e9 / VALU_BOUND
    res = {"S_r": S, "S_s": S, "N": n, "M": n, "hip_rs_s": round(t_rs, 4), "hip_rr_ss_s": round(t_sym, 4),
           "hip_all_s": round(t_rs + t_sym, 4), "hip_rs_dist_per_s": dist_rs / t_rs,
           "hip_all_dist_per_s": dist_all / (t_rs + t_sym), "bound": "vector-instruction rate, 8 ops/distance, 2.4 GHz",
           "bound_dist_per_s": bound, "hip_rs_fraction_of_bound": round(dist_rs / t_rs / bound, 4),
           "symmetric_exact": bool(torch.equal(d_rr, d_rr.t()) and torch.equal(d_ss, d_ss.t())),
           "launch_cap_pairs": max(1, metrics._DISTANCES_PER_LAUNCH // (n * n))}
    if not args.hip_only:
        torch_chamfer(ref[:1], smp[:args.chunk], args.chunk)  # warm-up
        torch.cuda.synchronize()
        t_rs_torch = timed_once(lambda: torch_chamfer(ref, smp, args.chunk))
        d_torch, t_torch = t_rs_torch
        rel = ((d_torch - d_rs).abs() / d_rs).max().item()
        res.update({"torch_rs_s": round(t_torch, 4), "torch_rs_dist_per_s": dist_rs / t_torch,
                    "speedup_rs": round(t_torch / t_rs, 2), "torch_vs_hip_max_rel": rel})
        assert rel < 1e-3, rel
    line = json.dumps(res)
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
