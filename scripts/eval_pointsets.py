"""Set-level quality of generated point clouds against a reference set: MMD, COV and 1-NNA under the Chamfer distance.

    python scripts/eval_pointsets.py SAMPLES REFS [--emd] [--jsd] [--points N [--resample METHOD]] [--normalize MODE] [--out FILE]

SAMPLES and REFS are each a `.npy` holding [S, n, 3] (what `bench.py --dump-outputs DIR` writes as DIR/points.npy) or a
directory of per-cloud [n, 3] `.npy` files (what metrics.save_point_clouds writes). Points are used as given: normalise
both sets the same way first (e.g. metrics.GlobalNormalizer). Prints one JSON line with the six metrics
(metrics.distribution_metrics_from_matrices), the set sizes and the seconds taken; --emd adds the same six metrics under
the EMD (approxmatch, metrics.emd_matrix; equal point counts, at most 4096), keyed `-EMD`; --jsd adds "jsd", the
Jensen-Shannon divergence between the two sets' occupancy distributions on a 28^3 grid (--jsd-resolution R) in the ball of
radius 0.5, and "jsd_outside_fraction"; --normalize unit_sphere / unit_cube (metrics.normalize_clouds) puts every cloud of
both sets into that ball / cube before all metrics; --out writes the same line to FILE.
--points N brings both sets to N points per cloud first: every set with more than N points is resampled
(metrics.resample_clouds; --resample fps, the default, is farthest point sampling, first takes the first N points, random a
random subset drawn with --resample-seed), a set with fewer than N points is an error. Resampling happens BEFORE --normalize,
so the normalisation sees the points the metrics see. With --points the JSON line also carries "resample" and "points".
Runs on the GPU only (the all-pairs Chamfer matrices are HIP kernels) and fails without one.
"""
import argparse
import json
import os
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from nova_pointcloud_amd import hip, metrics  # noqa: E402


def build_parser():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("samples", help="generated clouds: [S, n, 3] .npy or a directory of [n, 3] .npy files")
    ap.add_argument("refs", help="reference clouds: [S, n, 3] .npy or a directory of [n, 3] .npy files")
    ap.add_argument("--out", help="also write the JSON line to this file")
    ap.add_argument("--emd", action="store_true", help="also the six metrics under the EMD (approxmatch)")
    ap.add_argument("--jsd", action="store_true", help="also the JSD between the occupancy distributions of the two sets")
    ap.add_argument("--jsd-resolution", type=int, default=28, metavar="R", help="grid resolution of the JSD (default 28)")
    ap.add_argument("--normalize", choices=metrics.NORMALIZE_MODES, default=None,
                    help="per-cloud normalisation of both sets before all metrics (default: none)")
    ap.add_argument("--batch-size", type=int, default=None, help="cloud pairs per kernel launch (default: the library's cap)")
    ap.add_argument("--points", type=int, default=None, metavar="N",
                    help="resample every set with more than N points per cloud to N, before --normalize (default: use the sets as stored)")
    ap.add_argument("--resample", choices=metrics.RESAMPLE_METHODS, default="fps", help="how --points picks the points (default fps)")
    ap.add_argument("--resample-seed", type=int, default=0, help="seed of --resample random (default 0)")
    return ap


def check_point_counts(named_sets, n_points):
    """ValueError naming the first of the (name, path, points) sets that has fewer than `n_points` points per cloud."""
    if n_points < 1:
        raise ValueError(f"--points must be >= 1, got {n_points}")
    for name, path, pts in named_sets:
        if pts.shape[1] < n_points:
            raise ValueError(f"{name} ({path}) has {pts.shape[1]} points per cloud, fewer than --points {n_points}")


def main(argv=None):
    args = build_parser().parse_args(argv)
    load = lambda path: torch.from_numpy(metrics.load_point_clouds(path))
    if args.points is not None:  # a set too small for --points is reported whether or not a GPU is present
        smp, ref = load(args.samples), load(args.refs)
        check_point_counts([("samples", args.samples, smp), ("refs", args.refs, ref)], args.points)
    if not torch.cuda.is_available():
        raise hip.NovaHipError("eval_pointsets.py needs an MI355X GPU: the Chamfer matrices have no CPU path")
    smp, ref = (smp if args.points is not None else load(args.samples)).cuda(), (ref if args.points is not None else load(args.refs)).cuda()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    if args.points is not None:
        gen = torch.Generator().manual_seed(args.resample_seed)
        smp, ref = (metrics.resample_clouds(pts, args.points, method=args.resample, generator=gen) for pts in (smp, ref))
    if args.normalize is not None:
        smp, ref = metrics.normalize_clouds(smp, args.normalize), metrics.normalize_clouds(ref, args.normalize)
    extra = {"jsd": True, "jsd_resolution": args.jsd_resolution} if args.jsd else {}
    res = metrics.compute_all_metrics(smp, ref, batch_size=args.batch_size, emd=args.emd, **extra)
    if args.normalize is not None:
        res["normalize"] = args.normalize
    if args.points is not None:
        res["resample"], res["points"] = args.resample, args.points
    if res.get("jsd_outside_fraction", 0.0) > 0.05:
        print(f"warning: {100 * res['jsd_outside_fraction']:.1f} % of the points of a set lie outside the JSD grid: the clouds are not "
              "in the unit ball (radius 0.5); normalise them, e.g. with --normalize unit_sphere", file=sys.stderr)
    res.update({"n_samples": smp.shape[0], "n_refs": ref.shape[0], "sample_points": smp.shape[1], "ref_points": ref.shape[1],
                "seconds": round(time.perf_counter() - t0, 4)})
    line = json.dumps(res)
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")
    return res


if __name__ == "__main__":
    main()
