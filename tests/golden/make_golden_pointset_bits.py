"""Recorded bits of the point-set kernels, made by RUNNING THE LIBRARY ITSELF on an MI355X at a known commit:

    python tests/golden/make_golden_pointset_bits.py --commit <hash of the commit the library was built from>

tests/test_pointset_bits.py then asks the current build for the same bits. The file holds the inputs themselves (float32
points in the ball of radius 0.5 from a seeded CPU generator), one call per case (function of nova_pointcloud_amd.metrics,
arguments cut out of the stored points, keyword arguments) and every output of that call. The shapes are the smallest that
reach every code path of each kernel: see CASES.

Two things keep the file far below the size limit for committed files without dropping a point count:
  - an output above DIGEST_ABOVE bytes (the [2, 300, 1030] matrix of pairwise_dist alone) is stored as the SHA-256 of its
    bytes, which is the same bitwise test with a poorer failure message;
  - the cross-mode kNN case needs 512 clouds to reach the 256-query workgroup shape: it runs 8 distinct cloud pairs
    repeated 64 times, the 8 distinct results are stored, and the test requires every repetition to equal them.
"""
import argparse
import hashlib
import json
import os
import subprocess
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

DIGEST_ABOVE = 256 * 1024
POOL_POINTS = 18000  # two clouds of 9000, the largest case


def pts(offset, S, N, repeat=1, array="points"):
    """Argument spec: `array`[offset : offset + S N] as [S, N, 3], the S clouds repeated `repeat` times along dim 0."""
    return [array, offset, S, N, repeat]


def _cases():
    c = {}
    x, y = pts(0, 2, 300), pts(9000, 2, 1030)  # ragged 256-block, across the 1024-point tile
    c["nn_dist/clamp5"] = ("nn_dist", [x, y], {"clamp": 5.0})
    c["nn_dist/clamp1_unit"] = ("nn_dist", [x, y], {"clamp": 1.0, "unit_norm": True})
    c["pairwise_dist/clamp5"] = ("pairwise_dist", [x, y], {"clamp": 5.0})
    # register side x, register side y, two passes; symmetric; each whole and in launches of two pairs
    for N, M in ((300, 1030), (2100, 300), (2100, 2100)):
        for split in (None, 2):
            c[f"chamfer_matrix/{N}x{M}/{'whole' if split is None else 'split2'}"] = (
                "chamfer_matrix", [pts(0, 3, N), pts(9000, 2, M)], {"max_pairs_per_launch": split})
    for split in (None, 2):
        c[f"chamfer_matrix/sym300/{'whole' if split is None else 'split2'}"] = ("chamfer_matrix", [pts(0, 3, 300)], {"max_pairs_per_launch": split})
    for N in (200, 300, 600, 1100, 2100):  # the five instantiations
        c[f"emd_matrix/{N}"] = ("emd_matrix", [pts(0, 2, N), pts(9000, 2, N)], {})
    occ = pts(0, 5, 500, array="occ_points")  # about a fifth of the points outside the ball: the slow path
    c["occupancy_grid/sphere28"] = ("occupancy_grid", [occ], {"resolution": 28, "in_sphere": True, "return_nodes": True})
    c["occupancy_grid/cube7"] = ("occupancy_grid", [occ], {"resolution": 7, "in_sphere": False, "return_nodes": True})
    for N in (50, 100, 200, 400, 800, 1600, 3000, 5000, 9000):  # the nine workgroup shapes
        c[f"farthest_point_sample/{N}"] = ("farthest_point_sample", [pts(0, 2, N)], {"n_samples": 32, "return_distances": True})
    c["farthest_point_sample/800_start"] = ("farthest_point_sample", [pts(0, 2, 800)],
                                            {"n_samples": 32, "start": [3, 517], "return_distances": True})
    for k in (1, 3, 8, 17, 32):  # self mode, a list rung each from 1 to 32
        c[f"knn_points/self_k{k}"] = ("knn_points", [pts(0, 2, 300)], {"k": k})
    # 256-query workgroups (512 clouds) across the target tile
    c["knn_points/cross_512x40x1030_k9"] = ("knn_points", [pts(0, 8, 40, 64), pts(9000, 8, 1030, 64)], {"k": 9})
    for n, B in ((50, 2), (200, 2), (600, 2), (1100, 2), (2100, 1)):  # the five capacity forms; state saved and resumed
        c[f"optimal_assignment/{n}"] = ("optimal_assignment", [pts(0, B, n), pts(9000, B, n)],
                                        {"clamp": 2.0, "rounds_per_launch": 16, "return_rounds": True})
    return c


CASES = _cases()


def ball(n, generator, radius=0.5):
    """n points uniform in the ball, float32 [n, 3]."""
    d = torch.randn(n, 3, generator=generator, dtype=torch.float64)
    r = radius * torch.rand(n, 1, generator=generator, dtype=torch.float64) ** (1.0 / 3.0)
    return (d / d.norm(dim=1, keepdim=True) * r).float()


def make_inputs():
    g = torch.Generator().manual_seed(20261018)
    points = ball(POOL_POINTS, g)
    occ = ball(5 * 500, g)
    out = torch.rand(5 * 500, generator=g) < 0.2
    occ = torch.where(out[:, None], occ * (1.0 + 2.0 * torch.rand(5 * 500, 1, generator=g)), occ)
    return {"points": points.numpy(), "occ_points": occ.numpy()}


def argument(arrays, spec, device):
    name, offset, S, N, repeat = spec
    t = torch.from_numpy(arrays[name][offset:offset + S * N]).reshape(S, N, 3)
    return t.repeat(repeat, 1, 1).to(device)


def outputs_of(result):
    """The call's result as a list of (name, numpy array), in a fixed order."""
    if isinstance(result, dict):
        items = sorted(result.items())
    elif isinstance(result, (tuple, list)):
        items = [(str(i), r) for i, r in enumerate(result)]
    else:
        items = [("0", result)]
    return [(k, v.cpu().numpy() if torch.is_tensor(v) else np.asarray(v)) for k, v in items]


def run_case(name, arrays, device="cuda"):
    """Runs case `name` on the GPU. A repeated case is checked for equal repetitions and cut to its distinct clouds."""
    from nova_pointcloud_amd import metrics

    fn, specs, kwargs = CASES[name]
    outs = outputs_of(getattr(metrics, fn)(*(argument(arrays, s, device) for s in specs), **kwargs))
    repeat, distinct = specs[0][4], specs[0][2]
    if repeat > 1:
        for k, v in outs:
            tiled = np.tile(v[:distinct], (repeat,) + (1,) * (v.ndim - 1))
            assert v.tobytes() == tiled.tobytes(), f"{name}/{k}: repeated clouds gave different results"
        outs = [(k, v[:distinct]) for k, v in outs]
    return outs


def digest(a):
    return hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--commit", default=None, help="hash of the commit the loaded library was built from (default: git rev-parse HEAD)")
    ap.add_argument("--out", default=os.path.join(HERE, "pointset_bits.npz"))
    args = ap.parse_args()
    commit = args.commit or subprocess.run(["git", "-C", ROOT, "rev-parse", "HEAD"], check=True, capture_output=True, text=True).stdout.strip()
    arrays = make_inputs()
    meta = {"commit": commit, "device": torch.cuda.get_device_name(0), "outputs": {}}
    for name in CASES:
        recorded = []
        for k, v in run_case(name, arrays):
            entry = {"name": k, "dtype": str(v.dtype), "shape": list(v.shape)}
            if v.nbytes > DIGEST_ABOVE:
                entry["sha256"] = digest(v)
            else:
                arrays[f"{name}/{k}"] = v
            recorded.append(entry)
        meta["outputs"][name] = recorded
        print(name, [(e["name"], e["dtype"], e["shape"], "digest" if "sha256" in e else "") for e in recorded], flush=True)
    arrays["meta"] = np.array(json.dumps(meta))
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    np.savez_compressed(args.out, **arrays)
    print("->", args.out, f"{os.path.getsize(args.out) / 1e3:.1f} kB, commit {commit}")


if __name__ == "__main__":
    main()
