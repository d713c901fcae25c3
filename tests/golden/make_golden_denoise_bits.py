"""Recorded bits of the denoising loop (csrc/denoise.hip and the kernels it launches), made by RUNNING A LIBRARY on an MI355X:

    python tests/golden/make_golden_denoise_bits.py --lib <libnova_hip.so built at the commit> --commit <its hash>

tests/test_gpu_denoise_bits.py then asks the current build for the same bits. The file denoise_bits.json holds no arrays: per
case the SHA-256 of every input (seeded CPU generators; a drift of the generator then shows as an input mismatch, not as a
kernel failure), of x, the echo energy and the echo rows after the call, and ONE digest over all workspaces after the call
(a, mod, u, h, f, g, v in that order, allocated NaN-filled by denoise_ref.Workspaces, so a row the call never wrote counts too).

A case is one call of nova_decoder_denoise / nova_decoder_denoise_echo on draw 0 of denoise_ref.draw_inputs (the shapes and
sampler branches of test_gpu_denoise_loop.py; no fitness loop: nothing here is compared under a tolerance), with graphs off.
The graph/ cases make the same call twice on a side stream with graphs on and nothing cached: the first captures, the second
replays, each digested on its own; test_gpu_denoise_bits.py also asks both to equal the direct call's recorded digests."""
import argparse
import ctypes
import functools
import hashlib
import json
import os
import subprocess
import sys

import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
for _p in (ROOT, os.path.dirname(HERE)):
    if _p not in sys.path:
        sys.path.insert(0, _p)

import denoise_ref as R  # noqa: E402

DTYPES = {"f32": torch.float32, "bf16": torch.bfloat16, "f16": torch.float16}
STEPS, DEPTH = 4, 3
WORKSPACES = ("a", "mod", "u", "h", "f", "g", "v")


def _cases():
    """name -> (kind, shape, D, branch, dtype, depth, steps, mod_steps (None: steps))"""
    c = {}
    for branch in R.BRANCHES:  # every branch
        for shape, D in (("ragged", 128), ("cross", 768)):
            for dt in DTYPES:
                c[f"branch/{branch}/{shape}{D}/{dt}"] = ("direct", shape, D, branch, dt, DEPTH, STEPS, None)
    for branch in ("euler_trunc", "echo_ne9"):  # the fused-modulate rule flips mid-call where the plan truncates 400 -> 200 rows
        for dt in ("bf16", "f16"):
            c[f"flip/{branch}/cross1024/{dt}"] = ("direct", "cross", 1024, branch, dt, DEPTH, STEPS, None)
    for dt in DTYPES:  # edges: one block, one step, the projection inside every step, the patch embed's limit
        c[f"depth1/euler_trunc/cross768/{dt}"] = ("direct", "cross", 768, "euler_trunc", dt, 1, STEPS, None)
        c[f"steps1/euler_cfg/cross768/{dt}"] = ("direct", "cross", 768, "euler_cfg", dt, DEPTH, 1, 1)
        c[f"mod_steps1/euler_trunc/cross768/{dt}"] = ("direct", "cross", 768, "euler_trunc", dt, DEPTH, STEPS, 1)
        c[f"p64/echo_ne9/p64_128/{dt}"] = ("direct", "p64", 128, "echo_ne9", dt, DEPTH, STEPS, None)
    for branch in R.GRAPH_BRANCHES:  # capture and replay
        c[f"graph/{branch}/ragged128/bf16"] = ("graph", "ragged", 128, branch, "bf16", DEPTH, STEPS, None)
    return c


CASES = _cases()


def direct_case_of(name):
    """The direct call whose recorded digests a graph/ case must reproduce."""
    return "branch/" + name[len("graph/"):]


class Bound(object):
    """The package's binding (structs, dtype codes, current stream) with `call` going to the library at hand."""

    def __init__(self, lib):
        from nova_pointcloud_amd import hip

        self.lib, self.hip = lib, hip

    def __getattr__(self, name):
        return getattr(self.hip, name)

    def call(self, name, *args):
        rc = getattr(self.lib, name)(*args)
        if rc != 0:
            raise self.hip.NovaHipError(f"{name} failed ({rc}): {self.lib.nova_last_error().decode()}")

    def graph_stats(self):
        c, r = ctypes.c_long(0), ctypes.c_long(0)
        self.call("nova_debug_graph_stats", ctypes.byref(c), ctypes.byref(r))
        return c.value, r.value


def bind(path):
    """ctypes handle of the library at `path` with the package's signatures (nova_pointcloud_amd.hip.SIGNATURES)."""
    from nova_pointcloud_amd import hip

    lib = ctypes.CDLL(os.path.abspath(path))
    for name, argtypes in hip.SIGNATURES.items():
        fn = getattr(lib, name)
        fn.argtypes, fn.restype = argtypes, ctypes.c_int
    for name, (res, argtypes) in hip.PLAIN.items():
        fn = getattr(lib, name)
        fn.argtypes, fn.restype = argtypes, res
    assert lib.nova_check_device() == 0, lib.nova_last_error().decode()
    return lib


def digest(*tensors):
    h = hashlib.sha256()
    for t in tensors:
        h.update(t.detach().cpu().contiguous().view(torch.uint8).numpy().tobytes())
    return h.hexdigest()


@functools.lru_cache(maxsize=None)
def weights(D, depth, P):
    return R.make_weights(D, depth, P, R.weights_seed(D, depth, P))


_packs = {}


def pack_for(b, D, depth, P, dtype):
    key = (id(b.lib), D, depth, P, dtype)
    if key not in _packs:
        _packs[key] = R.DecoderPack(b, weights(D, depth, P), dtype, "cuda")
    return _packs[key]


def input_digests(c, w):
    flat = [w[k] for k in ("adaln_w", "adaln_b", "patch_w", "patch_b", "head_w", "head_b")]
    flat += [blk[k] for blk in w["blocks"] for k in ("fc1_w", "fc1_b", "fc2_w", "fc2_b", "norm2_w", "norm2_b")]
    ins = {"weights": digest(*flat), "plan": digest(torch.tensor([list(s) for s in c["plan"]], dtype=torch.float64))}
    for k in ("zc", "temb", "x", "noise", "energy", "echo_rows", "echo_noise"):
        if c[k] is not None:
            ins[k] = digest(c[k])
    return ins


def one_call(b, c, pack, ws, mod_steps, tag, outs):
    x, energy, rows = R.run_hip(b, pack, ws, c["zc"], c["temb"], c["x"], c["plan"], c["noise"], c["renorm"], c["energy"], c["echo_rows"],
                                c["echo_noise"], B=c["B"], n=c["n"], P=c["P"], D=c["D"], mod_steps=mod_steps)
    torch.cuda.synchronize()
    outs[tag + "x"] = digest(x)
    if energy is not None:
        outs[tag + "echo_energy"] = digest(energy)
    if rows is not None:
        outs[tag + "echo_rows"] = digest(rows)
    outs[tag + "workspaces"] = digest(*[getattr(ws, k) for k in WORKSPACES])


def run_case(name, lib):
    """Runs case `name` on `lib`; returns ({input name: sha256}, {output name: sha256})."""
    kind, shape, D, branch, dt, depth, steps, mod_steps = CASES[name]
    b, dtype = Bound(lib), DTYPES[dt]
    c = R.draw_inputs(shape, D, branch, depth, steps, 0)
    pack = pack_for(b, D, depth, c["P"], dtype)
    Ne = 0 if c["echo_rows"] is None else c["echo_rows"].shape[1]
    fresh = lambda: R.Workspaces(dtype, "cuda", steps=steps, S=c["passes"] * c["B"], B=c["B"], n=c["n"], P=c["P"], D=D, depth=depth, Ne=Ne)
    outs = {}
    b.call("nova_debug_set_graphs", 0)  # drops what earlier calls captured: a fresh buffer may land on an old address
    try:
        if kind == "direct":
            one_call(b, c, pack, fresh(), mod_steps, "", outs)
        else:  # the legacy default stream cannot be captured: a stream of its own
            b.call("nova_debug_set_graphs", 1)
            side = torch.cuda.Stream()
            with torch.cuda.stream(side):
                ws = fresh()
                c0, r0 = b.graph_stats()
                one_call(b, c, pack, ws, mod_steps, "capture/", outs)
                assert b.graph_stats() == (c0 + 1, r0), f"{name}: the first call must capture one graph"
                for k in WORKSPACES:  # what the replay does not write itself must not pass for written
                    getattr(ws, k).fill_(float("nan"))
                one_call(b, c, pack, ws, mod_steps, "replay/", outs)
                assert b.graph_stats() == (c0 + 1, r0 + 1), f"{name}: an argument-identical call must replay"
            side.synchronize()
    finally:
        b.call("nova_debug_set_graphs", 1)
    return input_digests(c, weights(D, depth, c["P"])), outs


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--lib", required=True, help="the libnova_hip.so whose bits are recorded")
    ap.add_argument("--commit", default=None, help="hash of the commit that library was built from (default: git rev-parse HEAD)")
    ap.add_argument("--out", default=os.path.join(HERE, "denoise_bits.json"))
    args = ap.parse_args()
    commit = args.commit or subprocess.run(["git", "-C", ROOT, "rev-parse", "HEAD"], check=True, capture_output=True, text=True).stdout.strip()
    lib = bind(args.lib)
    fixture = {"meta": {"commit": commit, "device": torch.cuda.get_device_name(0)}, "cases": {}}
    for name in CASES:
        ins, outs = run_case(name, lib)
        fixture["cases"][name] = {"inputs": ins, "outputs": outs}
    for name in CASES:  # the library recorded from must itself replay what it launches directly
        if name.startswith("graph/"):
            want = fixture["cases"][direct_case_of(name)]["outputs"]
            got = fixture["cases"][name]["outputs"]
            assert all(got[f"{tag}/{k}"] == v for tag in ("capture", "replay") for k, v in want.items()), name
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(fixture, f, indent=0, sort_keys=True)
        f.write("\n")
    print("->", args.out, f"{len(CASES)} cases, {os.path.getsize(args.out) / 1e3:.1f} kB, commit {commit}")


if __name__ == "__main__":
    main()
