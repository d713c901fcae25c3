"""Record what every nova_pointset_* entry point answers to bad arguments: tests/golden/pointset_errors.json.

    python tests/golden/make_golden_pointset_errors.py path/to/libnova_hip.so <commit the library was built from>
    HIP_VISIBLE_DEVICES=-1 python tests/golden/make_golden_pointset_errors.py --replay    (the test's check of the current build)

One call per argument check of the point-set files (every set_error / NOVA_REQUIRE site) and one per early `return 0`,
each recorded as (entry, arguments, return code, nova_last_error() text). All of them return before any HIP call, so this
runs on a machine without a GPU; pointers that must be non-null are small dummy addresses, never dereferenced on these
paths. For the entry points whose checks once sat in two files, further calls break two checks at once, which pins the
order. tests/test_pointset_abi_errors.py replays the table against the current build and compares code and text exactly:
the table is what the library answered at the commit named in it, and stays that until an entry point's contract changes.

The library is loaded by path with hip.SIGNATURES (as tools/ab_lib.py does), so a build of any commit can be recorded.
"""
import ctypes
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
OUT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "pointset_errors.json")

INF, NAN = float("inf"), float("nan")
IMAX = 2**31 - 1
KNN_MAX, INTERP_MAX, SC_MAX, FPS_MAX, EMD_MAX, ASSIGN_MAX, NB_MAX_C = 65536, 65536, 65536, 16384, 4096, 4096, 4096
OCC_MAX_POINTS = 2**24 - 1


def P(i):
    """Dummy address number i: 1 MiB apart and 16-byte aligned, so no two ranges of a small call overlap by accident."""
    return 0x100000 * i


# entry -> (argument names in ABI order without the trailing stream, a call that passes every check)
ENTRIES = {
    "nn_dist": ("x y d B N M lo hi unit", [P(1), P(2), P(3), 2, 8, 8, -1.0, 1.0, 0]),
    "pairwise_dist": ("x y D B N M lo hi", [P(1), P(2), P(3), 2, 8, 8, -1.0, 1.0]),
    "nearest_match": ("x y d idx B N M lo hi unit", [P(1), P(2), P(3), P(4), 2, 8, 8, -1.0, 1.0, 0]),
    "nearest_match_bwd": ("x y idx g gx gy B N M lo hi unit", [P(1), P(2), P(3), P(4), P(5), P(6), 2, 8, 8, -1.0, 1.0, 0]),
    "matched_dist": ("x y idx d B n lo hi floor", [P(1), P(2), P(3), P(4), 2, 8, -1.0, 1.0, 0.0]),
    "matched_dist_bwd": ("x y idx inv g gx gy B n lo hi floor", [P(1), P(2), P(3), P(4), P(5), P(6), P(7), 2, 8, -1.0, 1.0, 0.0]),
    "chamfer_matrix": ("x y cd A B N M ldc symmetric", [P(1), P(2), P(3), 2, 3, 8, 8, 3, 0]),
    "emd_matrix": ("x y emd A B N ldc", [P(1), P(2), P(3), 2, 3, 8, 3]),
    "occupancy_grid": ("x counters bernoulli node outside S N R in_sphere workgroups", [P(1), P(2), P(3), P(4), P(5), 2, 8, 4, 0, 0]),
    "farthest_point_sample": ("x start idx dist S N n", [P(1), P(2), P(3), P(4), 2, 8, 4]),
    "knn": ("x y idx d2 S N M k exclude_self", [P(1), P(2), P(3), P(4), 2, 8, 8, 4, 0]),
    "neighbor_aggregate": ("f idx w out S N M k C", [P(1), P(2), P(3), P(4), 2, 8, 8, 4, 4]),
    "neighbor_inverse": ("idx offsets edges S N M k", [P(1), P(2), P(3), 2, 8, 8, 4]),
    "neighbor_aggregate_bwd": ("f idx w g offsets edges gf gw S N M k C", [P(1), P(2), P(3), P(4), P(5), P(6), P(7), P(8), 2, 8, 8, 4, 4]),
    "kernel_interpolate": ("q p v out S T N C scale", [P(1), P(2), P(3), P(4), 2, 8, 8, 4, 1.0]),
    "kernel_interpolate_stats": ("q p v out m l S T N C scale", [P(1), P(2), P(3), P(4), P(5), P(6), 2, 8, 8, 4, 1.0]),
    "kernel_interpolate_bwd": ("q p v out m l g gq gp gv S T N C scale",
                               [P(1), P(2), P(3), P(4), P(5), P(6), P(7), P(8), P(9), P(10), 2, 8, 8, 4, 1.0]),
    "soft_cluster": ("x c out mass ws S N K shared_centers scale", [P(1), P(2), P(3), P(4), P(5), 2, 8, 4, 0, 1.0]),
    "soft_cluster_bwd": ("x c out mass g gm gx gc ws S N K shared_centers scale",
                         [P(1), P(2), P(3), P(4), P(5), P(6), P(7), P(8), P(9), 2, 8, 4, 0, 1.0]),
    "soft_cluster_sum_clouds": ("gc gcs S K", [P(1), P(2), 2, 4]),
    "assignment": ("x y col cost state B n lo hi use_clamp rounds restart all_done",
                   [P(1), P(2), P(3), P(4), P(5), 2, 8, -1.0, 1.0, 1, 4, 0, P(6)]),
    "assignment_rounds": ("state rounds_used B n", [P(1), P(2), 2, 8]),
}

NULLS = {
    "nn_dist": "x y d", "pairwise_dist": "x y D", "nearest_match": "x y d idx", "nearest_match_bwd": "x y idx g gx gy",
    "matched_dist": "x y idx d", "matched_dist_bwd": "x y idx inv g gx gy", "chamfer_matrix": "x y cd", "emd_matrix": "x y emd",
    "occupancy_grid": "x counters", "farthest_point_sample": "x idx", "knn": "x y idx", "neighbor_aggregate": "f idx out",
    "neighbor_inverse": "idx offsets edges", "neighbor_aggregate_bwd": "f idx g", "kernel_interpolate": "q p out",
    "kernel_interpolate_stats": "q p out m l", "kernel_interpolate_bwd": "q p out m l g", "soft_cluster": "x c out mass ws",
    "soft_cluster_bwd": "x c out mass g", "soft_cluster_sum_clouds": "gc gcs", "assignment": "x y col cost state all_done",
    "assignment_rounds": "state rounds_used",
}


def cases():
    """[(entry, arguments without the stream)]: every call here returns before any HIP call."""
    out = []

    def bad(entry, **over):
        names, args = ENTRIES[entry]
        names, args = names.split(), list(args)
        for k, v in over.items():
            args[names.index(k)] = v
        out.append((entry, args))

    for entry, names in NULLS.items():  # every pointer that has to be there, one at a time
        for n in names.split():
            bad(entry, **{n: None})

    # ---- pointset.hip, nearest_match.hip: (null, clamp) once in the wrapper, then (nothing to do, M, batch)
    for e in ("nn_dist", "nearest_match", "nearest_match_bwd"):
        bad(e, lo=1.0, hi=-1.0)
        bad(e, lo=NAN)
        bad(e, B=0)
        bad(e, N=0)
        bad(e, B=-1, x=None, y=None)
        bad(e, M=0)
        bad(e, B=65536)
        bad(e, x=None, lo=1.0, hi=-1.0)     # null before clamp
        bad(e, x=None, M=0)                 # wrapper before kernel file: null before the empty target set
        bad(e, lo=1.0, hi=-1.0, M=0)        # clamp before the empty target set
        bad(e, lo=1.0, hi=-1.0, B=65536)    # clamp before the batch limit
        bad(e, M=0, B=65536)                # empty target set before the batch limit
        bad(e, lo=1.0, hi=-1.0, B=0)        # the clamp range is checked even when there is nothing to do
    bad("pairwise_dist", lo=1.0, hi=-1.0)
    bad("pairwise_dist", B=0)
    bad("pairwise_dist", M=0)
    bad("pairwise_dist", N=0, x=None, y=None, D=None)
    bad("pairwise_dist", B=65536)
    bad("pairwise_dist", N=16 * 65535 + 1)
    bad("pairwise_dist", x=None, lo=1.0, hi=-1.0)
    bad("pairwise_dist", x=None, B=65536)           # null before the grid limit
    bad("pairwise_dist", lo=1.0, hi=-1.0, B=65536)  # clamp before the grid limit
    bad("pairwise_dist", lo=1.0, hi=-1.0, M=0)      # clamp even when there is nothing to do
    # ---- matched.hip: (null, clamp, floor), then (nothing to do, batch)
    for e in ("matched_dist", "matched_dist_bwd"):
        bad(e, lo=1.0, hi=-1.0)
        bad(e, floor=-0.5)
        bad(e, floor=NAN)
        bad(e, B=0)
        bad(e, n=0, x=None, idx=None)
        bad(e, B=65536)
        bad(e, x=None, lo=1.0, hi=-1.0)
        bad(e, lo=1.0, hi=-1.0, floor=-0.5)  # clamp before floor
        bad(e, x=None, B=65536)              # wrapper before kernel file: null, clamp and floor before the batch limit
        bad(e, lo=1.0, hi=-1.0, B=65536)
        bad(e, floor=-0.5, B=65536)
        bad(e, floor=-0.5, B=0)              # floor even when there is nothing to do
    # ---- chamfer.hip: (null, ldc, symmetric), then (nothing to do, empty cloud, pair count)
    bad("chamfer_matrix", ldc=2)
    bad("chamfer_matrix", symmetric=1)                                # x != y
    bad("chamfer_matrix", symmetric=1, y=P(1), A=3, B=3, N=8, M=9)     # N != M
    bad("chamfer_matrix", symmetric=1, y=P(1), A=2, B=3)               # A != B
    bad("chamfer_matrix", A=0)
    bad("chamfer_matrix", B=0, x=None, y=None, cd=None)
    bad("chamfer_matrix", N=0)
    bad("chamfer_matrix", M=0)
    bad("chamfer_matrix", A=65536, B=32768, ldc=32768)
    bad("chamfer_matrix", symmetric=1, y=P(1), A=65536, B=65536, ldc=65536)
    bad("chamfer_matrix", x=None, ldc=2)
    bad("chamfer_matrix", ldc=2, symmetric=1)
    bad("chamfer_matrix", x=None, N=0)             # wrapper before kernel file
    bad("chamfer_matrix", ldc=2, N=0)
    bad("chamfer_matrix", symmetric=1, M=0)
    bad("chamfer_matrix", ldc=2, A=65536, B=32768)
    bad("chamfer_matrix", N=0, A=65536, B=32768, ldc=32768)  # empty cloud before the pair count
    bad("chamfer_matrix", A=0, ldc=2)              # ldc even when there is nothing to do
    # ---- emd.hip: (null, ldc, N), then (nothing to do, pair count)
    bad("emd_matrix", ldc=2)
    bad("emd_matrix", N=0)
    bad("emd_matrix", N=EMD_MAX + 1)
    bad("emd_matrix", A=0)
    bad("emd_matrix", B=0, x=None, y=None, emd=None)
    bad("emd_matrix", A=65536, B=32768, ldc=32768)
    bad("emd_matrix", x=None, ldc=2)
    bad("emd_matrix", ldc=2, N=0)
    bad("emd_matrix", x=None, A=65536, B=32768, ldc=32768)  # wrapper before kernel file
    bad("emd_matrix", ldc=2, A=65536, B=32768)
    bad("emd_matrix", N=0, A=65536, B=32768, ldc=32768)
    bad("emd_matrix", N=0, A=0)                    # N even when there is nothing to do
    # ---- occupancy.hip
    bad("occupancy_grid", N=0)
    bad("occupancy_grid", N=OCC_MAX_POINTS + 1)
    bad("occupancy_grid", R=1)
    bad("occupancy_grid", R=33)
    bad("occupancy_grid", R=2, in_sphere=1)
    bad("occupancy_grid", workgroups=-1)
    bad("occupancy_grid", S=0)
    bad("occupancy_grid", S=-2, x=None, counters=None)
    bad("occupancy_grid", S=0, N=0)
    bad("occupancy_grid", S=0, workgroups=-1)
    # ---- fps.hip
    bad("farthest_point_sample", N=0)
    bad("farthest_point_sample", N=FPS_MAX + 1)
    bad("farthest_point_sample", n=0)
    bad("farthest_point_sample", n=9)
    bad("farthest_point_sample", S=0)
    bad("farthest_point_sample", S=0, x=None, idx=None)
    bad("farthest_point_sample", S=0, n=9)
    # ---- knn.hip
    bad("knn", N=0)
    bad("knn", M=0)
    bad("knn", N=KNN_MAX + 1, M=KNN_MAX + 1)
    bad("knn", exclude_self=1, M=9)
    bad("knn", k=0)
    bad("knn", k=33, N=40, M=40)
    bad("knn", k=9)
    bad("knn", k=8, exclude_self=1)
    bad("knn", S=0)
    bad("knn", S=-3, x=None, y=None, idx=None, d2=None)
    bad("knn", S=0, k=9)
    bad("knn", S=IMAX, N=KNN_MAX)   # the launch limit, found after every argument check
    # ---- neighbor.hip
    for e in ("neighbor_aggregate", "neighbor_inverse", "neighbor_aggregate_bwd"):
        bad(e, N=0)
        bad(e, M=KNN_MAX + 1)
        bad(e, k=0)
        bad(e, k=33)
        bad(e, S=65536)
        bad(e, S=0)
        bad(e, S=0, k=0)
        bad(e, S=-1, idx=None)
    for e in ("neighbor_aggregate", "neighbor_aggregate_bwd"):
        bad(e, C=0)
        bad(e, C=NB_MAX_C + 1)
    bad("neighbor_aggregate", out=P(1))
    bad("neighbor_aggregate", out=P(2) + 16)
    bad("neighbor_aggregate", out=P(3))
    bad("neighbor_inverse", offsets=P(1))
    bad("neighbor_inverse", edges=P(1) + 4)
    bad("neighbor_inverse", offsets=P(3))
    bad("neighbor_aggregate_bwd", gw=P(8), w=None)
    bad("neighbor_aggregate_bwd", gf=None, gw=None)
    bad("neighbor_aggregate_bwd", offsets=None)
    bad("neighbor_aggregate_bwd", edges=None)
    bad("neighbor_aggregate_bwd", gf=P(4))
    bad("neighbor_aggregate_bwd", gw=P(1))
    bad("neighbor_aggregate_bwd", gw=P(7))
    bad("neighbor_aggregate_bwd", gf=P(6))
    # ---- interp_common.h, interp.hip, interp_bwd.hip
    for e in ("kernel_interpolate", "kernel_interpolate_stats", "kernel_interpolate_bwd"):
        bad(e, T=0)
        bad(e, N=INTERP_MAX + 1)
        bad(e, C=0)
        bad(e, C=9)
        bad(e, v=None, C=4)
        bad(e, scale=-1.0)
        bad(e, scale=INF)
        bad(e, scale=NAN)
        bad(e, S=0)
        bad(e, S=-1, q=None, p=None, out=None)
        bad(e, S=0, scale=-1.0)
        bad(e, S=IMAX, T=129)   # the launch limit, found after every argument check
    bad("kernel_interpolate_bwd", S=IMAX, T=1, N=513)
    bad("kernel_interpolate_bwd", v=None, C=3)                       # gv given without v
    bad("kernel_interpolate_bwd", gv=None)                           # gp without gv when v is given
    bad("kernel_interpolate_bwd", gq=None, gp=None, gv=None)
    bad("kernel_interpolate_stats", S=0, m=None, l=None)
    bad("kernel_interpolate_bwd", S=0, m=None, g=None)
    # ---- soft_cluster.hip
    for e in ("soft_cluster", "soft_cluster_bwd"):
        bad(e, N=0)
        bad(e, N=SC_MAX + 1)
        bad(e, K=0)
        bad(e, K=33)
        bad(e, S=65536)
        bad(e, scale=-1.0)
        bad(e, scale=INF)
        bad(e, scale=NAN)
        bad(e, K=33, scale=-1.0)
        bad(e, S=0)
        bad(e, S=-1, x=None, c=None)
        bad(e, S=0, scale=NAN)
    bad("soft_cluster", out=P(1))
    bad("soft_cluster", ws=P(2))
    bad("soft_cluster", mass=P(3) + 8)
    bad("soft_cluster", ws=P(4))
    bad("soft_cluster", c=P(3) - 48, shared_centers=0)  # per-cloud centres reach into out
    bad("soft_cluster_bwd", gx=None, gc=None)
    bad("soft_cluster_bwd", ws=None)
    bad("soft_cluster_bwd", gx=P(5))
    bad("soft_cluster_bwd", gc=P(6))
    bad("soft_cluster_bwd", ws=P(1))
    bad("soft_cluster_bwd", gc=P(7))
    bad("soft_cluster_bwd", ws=P(8))
    bad("soft_cluster_sum_clouds", K=0)
    bad("soft_cluster_sum_clouds", K=33)
    bad("soft_cluster_sum_clouds", S=0)
    bad("soft_cluster_sum_clouds", S=0, gc=None, gcs=None)
    bad("soft_cluster_sum_clouds", S=0, K=0)
    bad("soft_cluster_sum_clouds", gcs=P(1) + 48)
    # ---- assign.hip (nova_pointset_assignment has no early return: B <= 0 still sets *all_done on the device)
    bad("assignment", n=0)
    bad("assignment", n=ASSIGN_MAX + 1)
    bad("assignment", rounds=0)
    bad("assignment", lo=1.0, hi=-1.0)
    bad("assignment", lo=NAN)
    bad("assignment", B=0, all_done=None)
    bad("assignment", n=0, rounds=0)
    bad("assignment", rounds=0, lo=1.0, hi=-1.0)
    bad("assignment_rounds", n=0)
    bad("assignment_rounds", n=ASSIGN_MAX + 1)
    bad("assignment_rounds", B=0)
    bad("assignment_rounds", B=-1, state=None, rounds_used=None)
    bad("assignment_rounds", B=0, n=0)
    return out


STATE_BYTES = [0, 1, 8, ASSIGN_MAX, ASSIGN_MAX + 1, -1]  # nova_pointset_assignment_state_bytes: a plain function, no error record


def bind(lib):
    """argtypes / restype of every point-set entry on a ctypes handle (hip.load() has done it for its own handle)."""
    sys.path.insert(0, ROOT)
    from nova_pointcloud_amd import hip

    for name, argtypes in hip.SIGNATURES.items():
        if name.startswith("nova_pointset_"):
            getattr(lib, name).argtypes, getattr(lib, name).restype = argtypes, ctypes.c_int
    res, argtypes = hip.PLAIN["nova_pointset_assignment_state_bytes"]
    lib.nova_pointset_assignment_state_bytes.argtypes, lib.nova_pointset_assignment_state_bytes.restype = argtypes, res
    lib.nova_last_error.restype = ctypes.c_char_p
    return lib


def answer(lib, entry, args):
    """(return code, message or None) of one call; the stream is NULL."""
    rc = getattr(lib, "nova_pointset_" + entry)(*args, None)
    return rc, (lib.nova_last_error().decode() if rc != 0 else None)


def record(lib):
    rows = []
    for entry, args in cases():
        rc, msg = answer(lib, entry, args)
        # -3 would be a launch that failed for want of a device: the call got past the checks, which no case here may
        assert rc in (0, -1, -2), (entry, args, rc, msg)
        rows.append({"entry": entry, "args": args, "rc": rc, "message": msg})
    return rows, [[n, lib.nova_pointset_assignment_state_bytes(n)] for n in STATE_BYTES]


def replay(lib, table):
    """The first call of `table` that `lib` answers otherwise than recorded, as text; None when there is none. Stops at that
    call: past it the arguments are not known to be rejected, and they hold addresses of nothing."""
    for c in table["cases"]:
        got = answer(lib, c["entry"], c["args"])
        if got != (c["rc"], c["message"]):
            return f"{c['entry']}{tuple(c['args'])}: recorded {(c['rc'], c['message'])}, got {got}"
    for n, size in table["state_bytes"]:
        if lib.nova_pointset_assignment_state_bytes(n) != size:
            return f"assignment_state_bytes({n}): recorded {size}, got {lib.nova_pointset_assignment_state_bytes(n)}"
    return None


if __name__ == "__main__":
    if sys.argv[1:] == ["--replay"]:  # the current build against the committed table (tests/test_pointset_abi_errors.py)
        sys.path.insert(0, ROOT)
        from nova_pointcloud_amd import hip

        lib = hip.load(check_device=False)
        # a build that lost a check would launch on the dummy addresses: only where no device can take the launch
        if lib.nova_check_device() == 0:
            sys.exit("a GPU is visible: the replay runs only in a process that sees none (HIP_VISIBLE_DEVICES=-1)")
        with open(OUT) as f:
            table = json.load(f)
        difference = replay(lib, table)
        if difference:
            sys.exit(difference)
        print(f"replayed {len(table['cases'])} cases")
        sys.exit(0)
    path, commit = sys.argv[1], sys.argv[2]
    rows, state_bytes = record(bind(ctypes.CDLL(os.path.abspath(path))))
    with open(OUT, "w") as f:  # one case per line
        f.write('{"commit": %s, "state_bytes": %s, "cases": [\n' % (json.dumps(commit), json.dumps(state_bytes)))
        f.write(",\n".join(json.dumps(r) for r in rows) + "\n]}\n")
    print(f"{len(rows)} cases ({sum(r['rc'] != 0 for r in rows)} errors, {sum(r['rc'] == 0 for r in rows)} early returns) -> {OUT}")
