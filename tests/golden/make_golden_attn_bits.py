"""Recorded bits of the attention forward kernels (csrc/attn.hip, attn16.hip), made by RUNNING A LIBRARY on an MI355X:

    python tests/golden/make_golden_attn_bits.py --lib <libnova_hip.so built at the commit> --commit <its hash>

tests/test_gpu_attn_bits.py then asks the current build for the same bits. The file attn_fwd_bits.json holds no arrays:
per case the SHA-256 of every input (seeded CPU generators; a drift of the generator then shows as an input mismatch, not
as a kernel failure) and of every output buffer, padding included. Every case is S = 2, and heads = 2 unless it says otherwise;
see CASES for what each one calls. The vit* cases pin whole block stacks (capi.hip: plain, fp8 in both hidden-row modes, KV-cached),
the walk direction of every launch included. Attention shapes: (Lq, Lk) over one exact tile, ragged last tiles, Lk < 64 and Lq across the 128- and 256-row workgroup
edges; for Lk >= 200 two late spike keys make the running max jump after tile 0 (the deferred-rescale branch, which in
variant 5 also rescales the pending P)."""
import argparse
import ctypes
import hashlib
import json
import os
import subprocess
import sys

import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

S, HEADS = 2, 2
LENGTHS = [(1, 1), (17, 64), (33, 63), (128, 129), (129, 31), (257, 200), (300, 769)]
LOG2E = 1.4426950408889634
SCALES = {"at_load": 0.2, "prescaled": 0.6931471805599453}  # the second: scale * log2 e == 1.0f, q counts as pre-scaled
SENTINEL = -3.0
DTYPES = {"bf16": torch.bfloat16, "f16": torch.float16, "f32": torch.float32}


def _cases():
    c = {}
    # nova_attn_fwd: every 16-bit head_dim 64 structure, head_dim 96 and f32 at the default; both scales, packed and cache layout
    kernels = [(dt, 64, av) for dt in ("bf16", "f16") for av in range(6)] + [(dt, 96, -1) for dt in ("bf16", "f16")] + [("f32", hd, -1) for hd in (64, 96)]
    for dt, hd, av in kernels:
        for Lq, Lk in LENGTHS:
            c[f"fwd/{dt}/hd{hd}/v{av}/{Lq}x{Lk}"] = ("fwd", dict(dtype=dt, hd=hd, variant=av, Lq=Lq, Lk=Lk))
    # nova_attn_fwd_lse (bf16): unmasked on three structures, masked (block-causal key limit: prefix, then equal frames)
    for hd in (64, 96):
        for av in (0, 3, 5):
            for L in (63, 200, 333):
                c[f"lse/hd{hd}/v{av}/{L}"] = ("lse", dict(hd=hd, variant=av, L=L, prefix=None, frame=None))
        for L, prefix, frame in ((200, 8, 48), (333, 13, 64)):
            c[f"lse_masked/hd{hd}/{L}"] = ("lse", dict(hd=hd, variant=-1, L=L, prefix=prefix, frame=frame))
    # the reverse walk (rev = 1) of the workgroup decode: the block composite alternates the direction launch by launch
    c["vit_blocks/bf16/D128/L200"] = ("vit", dict(nblocks=2, D=128, L=200))
    # the fp8 stack, delayed and row-scaled hidden rows: 342 rows = two 256-row tiles, the last ragged; 2 x 7 walked launches
    for mode in ("delayed", "rowscaled"):
        c[f"vit_fp8/{mode}/D256/L171"] = ("vit", dict(nblocks=2, D=256, L=171, heads=4, rope_batch=2, mode=f"fp8_{mode}"))
    # the 16-bit KV stack: q pre-scaled by the QKV epilogue, keys read from the cache with its sequence stride, two chunks
    c["vit_kv/bf16/D128"] = ("vit", dict(nblocks=2, D=128, L=0, heads=2, rope_batch=2, mode="kv", chunks=(37, 64), cap=160))
    return c


CASES = _cases()


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


def call(lib, name, *args):
    rc = getattr(lib, name)(*args)
    if rc != 0:
        raise RuntimeError(f"{name} failed ({rc}): {lib.nova_last_error().decode()}")


def digest(t):
    t = t.detach().cpu().contiguous()
    return hashlib.sha256(t.view(torch.uint8).numpy().tobytes()).hexdigest()


def seed_of(name):
    return int.from_bytes(hashlib.sha256(name.encode()).digest()[:4], "little")


def spike(q, k, Lq, Lk, hd):
    """test_attention_structures_16bit's late spikes, sequence 0 / head 0: key Lk - 3 aligned with query 5, key 70 with query 77."""
    if Lk >= 200:
        k[0, Lk - 3, :hd] = (q[0, min(5, Lq - 1), :hd].float() * 4).to(k.dtype)
        k[0, 70, :hd] = (q[0, min(77, Lq - 1), :hd].float() * 3).to(k.dtype)


def stream():
    return torch.cuda.current_stream().cuda_stream


def run_fwd(lib, name, dtype, hd, variant, Lq, Lk):
    from nova_pointcloud_amd import hip

    dt, D = DTYPES[dtype], HEADS * hd
    g = torch.Generator().manual_seed(seed_of(name))
    q = torch.randn(S, Lq, D, generator=g).to(dt)
    k, v = torch.randn(S, Lk, D, generator=g).to(dt), torch.randn(S, Lk, D, generator=g).to(dt)
    spike(q, k, Lq, Lk, hd)
    qpad, self_q = torch.randn(S * Lq, 8, generator=g).to(dt), torch.randn(S, Lk, D, generator=g).to(dt)
    spike(self_q, k, Lk, Lk, hd)
    ins = {"q": q, "k": k, "v": v, "qpad": qpad, "self_q": self_q}
    outs = {}
    call(lib, "nova_debug_set_attn_variant", variant)
    try:
        for sname, scale in SCALES.items():
            f = hd ** -0.5 if sname == "prescaled" else 1.0  # keep the logits of the c == 1 path in the usual range
            # cache layout (test_attention_cross_length): q rows [S*Lq, D + 8], k | v rows [S*Lk, 2D], o [S*Lq + 2, D + 16] with padding
            qbuf = torch.cat([(q.float() * f).to(dt).reshape(S * Lq, D), qpad], 1).contiguous().cuda()
            kv = torch.cat([k.reshape(S * Lk, D), v.reshape(S * Lk, D)], 1).contiguous().cuda()
            o = torch.full((S * Lq + 2, D + 16), SENTINEL, dtype=dt).cuda()
            call(lib, "nova_attn_fwd", qbuf.data_ptr(), kv.data_ptr(), kv.data_ptr() + D * kv.element_size(), o.data_ptr(), S, HEADS, Lq, Lk, hd,
                 D + 8, 2 * D, D + 16, scale, hip.dtype_code(dt), stream())
            outs[f"cache/{sname}"] = o
            # packed QKV [S*Lk, 3D]: self-attention over the Lk rows
            qkv = torch.cat([(self_q.float() * f).to(dt).reshape(S * Lk, D), k.reshape(S * Lk, D), v.reshape(S * Lk, D)], 1).contiguous().cuda()
            o = torch.full((S * Lk, D), SENTINEL, dtype=dt).cuda()
            es = qkv.element_size()
            call(lib, "nova_attn_fwd", qkv.data_ptr(), qkv.data_ptr() + D * es, qkv.data_ptr() + 2 * D * es, o.data_ptr(), S, HEADS, Lk, Lk, hd,
                 3 * D, 3 * D, D, scale, hip.dtype_code(dt), stream())
            outs[f"packed/{sname}"] = o
    finally:
        call(lib, "nova_debug_set_attn_variant", -1)
    return ins, outs


def run_lse(lib, name, hd, variant, L, prefix, frame):
    D = HEADS * hd
    g = torch.Generator().manual_seed(seed_of(name))
    qkv = torch.randn(S, L, 3 * D, generator=g)
    qkv[:, :, :D] *= hd ** -0.5 * LOG2E  # q arrives pre-scaled by scale * log2 e
    qkv = qkv.to(torch.bfloat16)
    spike(qkv[:, :, :D], qkv[:, :, D:2 * D], L, L, hd)
    ins = {"qkv": qkv}
    klim = None
    if prefix is not None:  # token i sees the tokens of frames <= its own; the prefix counts as frame 0
        i = torch.arange(L)
        klim = torch.where(i < prefix, torch.tensor(prefix), prefix + ((i - prefix) // frame + 1) * frame).clamp(max=L).to(torch.int32)
        ins["key_limit"] = klim
        klim = klim.cuda()
    dev = qkv.reshape(S * L, 3 * D).contiguous().cuda()
    o = torch.full((S * L, D), SENTINEL, dtype=torch.bfloat16).cuda()
    lse = torch.full((S, HEADS, L), SENTINEL, dtype=torch.float32).cuda()
    call(lib, "nova_debug_set_attn_variant", variant)
    try:
        call(lib, "nova_attn_fwd_lse", dev.data_ptr(), dev.data_ptr() + 2 * D, dev.data_ptr() + 4 * D, o.data_ptr(), lse.data_ptr(), S, HEADS, L, hd,
             3 * D, D, None if klim is None else klim.data_ptr(), stream())
    finally:
        call(lib, "nova_debug_set_attn_variant", -1)
    return ins, {"o": o, "lse": lse}


BLOCK_KEYS = ("qkv_w", "qkv_b", "proj_w", "proj_b", "norm1_w", "norm1_b", "fc1_w", "fc1_b", "fc2_w", "fc2_b", "norm2_w", "norm2_b")


FP8_KEYS = ("qkv_w", "fc1_w", "fc2_w")  # the three linears nova_vit_blocks_forward_fp8 reads as e4m3 rows


def rope_rows(g, batch, L, hd):
    """A [batch, L, hd/2, 2] (cos, sin) table of seeded angles."""
    a = torch.rand(batch, L, hd // 2, generator=g) * 6.283185307179586
    return torch.stack([a.cos(), a.sin()], -1).contiguous()


def run_vit(lib, name, nblocks, D, L, heads=HEADS, rope_batch=0, mode="plain", chunks=(), cap=0):
    """mode "plain": nova_vit_blocks_forward on L rows; "fp8_delayed" / "fp8_rowscaled": nova_vit_blocks_forward_fp8 on L rows;
    "kv": nova_vit_blocks_forward_kv, one call per entry of `chunks` (rows) over a cache of `cap` rows. rope_batch 0 = no table."""
    from nova_pointcloud_amd import hip

    g = torch.Generator().manual_seed(seed_of(name))
    hidden, dt = 4 * D, torch.bfloat16
    shapes = {"qkv_w": (3 * D, D), "qkv_b": (3 * D,), "proj_w": (D, D), "proj_b": (D,), "norm1_w": (D,), "norm1_b": (D,),
              "fc1_w": (hidden, D), "fc1_b": (hidden,), "fc2_w": (D, hidden), "fc2_b": (D,), "norm2_w": (D,), "norm2_b": (D,)}
    ins, keep = {}, []
    arr = (hip.VitBlock * nblocks)()
    for b in range(nblocks):
        ptrs = []
        for key in BLOCK_KEYS:
            w = torch.randn(*shapes[key], generator=g) * (shapes[key][-1] ** -0.5 if key.endswith("_w") and len(shapes[key]) == 2 else 0.1)
            if key.startswith("norm") and key.endswith("_w"):
                w = w + 1.0
            w = w.to(dt if len(shapes[key]) == 2 else torch.float32)
            ins[f"block{b}/{key}"] = w
            keep.append(w.cuda())
            ptrs.append(keep[-1].data_ptr())
        arr[b] = hip.VitBlock(*ptrs)
    def table(key, rows):
        if not rope_batch:
            return None
        ins[key] = rope_rows(g, rope_batch, rows, D // heads)
        keep.append(ins[key].cuda())
        return keep[-1].data_ptr()

    def filled(*shape, dtype):  # an output buffer whose untouched bytes hash the same
        return torch.full(shape, SENTINEL if dtype.is_floating_point else 0xFD, dtype=dtype, device="cuda")

    if mode == "kv":
        cache = filled(nblocks, S, cap, 2 * D, dtype=dt)
        outs, done = {"cache": cache}, 0
        for c, rows in enumerate(chunks):
            ins[f"x/chunk{c}"] = torch.randn(S * rows, D, generator=g).to(dt)
            xd = ins[f"x/chunk{c}"].cuda()
            ws = [torch.empty(S * rows, n, dtype=dt, device="cuda") for n in (3 * D, D, D, hidden)]
            call(lib, "nova_vit_blocks_forward_kv", arr, nblocks, xd.data_ptr(), S, rows, D, heads, hidden, table(f"rope/chunk{c}", rows), rope_batch or 1,
                 cache.data_ptr(), cap, done, *[w.data_ptr() for w in ws], hip.dtype_code(dt), stream())
            outs[f"x/chunk{c}"] = xd
            done += rows
        return ins, outs
    x = torch.randn(S * L, D, generator=g).to(dt)
    ins["x"] = x
    xd = x.cuda()
    ws = [torch.empty(S * L, n, dtype=dt, device="cuda") for n in (3 * D, D, D, hidden)]
    if mode == "plain":
        call(lib, "nova_vit_blocks_forward", arr, nblocks, xd.data_ptr(), S, L, D, heads, hidden, table("rope", L), rope_batch or 1,
             *[w.data_ptr() for w in ws], hip.dtype_code(dt), stream())
        return ins, {"x": xd}
    # fp8: the weights of the three large linears quantised per output row by the same library, and hashed among the inputs
    arr8 = (hip.VitBlockFp8 * nblocks)()
    for b in range(nblocks):
        ptrs = []
        for key in FP8_KEYS:
            w = keep[b * len(BLOCK_KEYS) + BLOCK_KEYS.index(key)]
            w8, wsc = torch.empty(w.shape, dtype=torch.uint8, device="cuda"), torch.empty(w.shape[0], device="cuda")
            call(lib, "nova_quantize_rows_fp8", w.data_ptr(), w8.data_ptr(), wsc.data_ptr(), w.shape[0], w.shape[1], stream())
            ins[f"block{b}/{key}8"], ins[f"block{b}/{key}s"] = w8, wsc
            ptrs += [w8.data_ptr(), wsc.data_ptr()]
        arr8[b] = hip.VitBlockFp8(*ptrs)
    rope = table("rope", L)
    outs = {"x": xd, "ws_x8": filled(S * L, D, dtype=torch.uint8), "ws_xs": filled(S * L, dtype=torch.float32),
            "ws_h8": filled(S * L, hidden, dtype=torch.uint8), "ws_hs": filled(S * L, dtype=torch.float32)}
    h_scale = h_amax = None
    if mode == "fp8_delayed":  # both are outputs: the scale is read, the amax word recorded per block
        outs["h_scale"] = torch.full((nblocks,), 64.0 / 448.0, dtype=torch.float32, device="cuda")
        outs["h_amax"] = torch.zeros(nblocks, dtype=torch.int32, device="cuda")
        h_scale, h_amax = outs["h_scale"].data_ptr(), outs["h_amax"].data_ptr()
    call(lib, "nova_vit_blocks_forward_fp8", arr, arr8, nblocks, xd.data_ptr(), S, L, D, heads, hidden, rope, rope_batch or 1,
         *[w.data_ptr() for w in ws], *[outs[k].data_ptr() for k in ("ws_x8", "ws_xs", "ws_h8", "ws_hs")], h_scale, h_amax, stream())
    return ins, outs


def run_case(name, lib):
    """Runs case `name` on `lib`; returns ({input name: sha256}, {output name: sha256})."""
    kind, kw = CASES[name]
    ins, outs = {"fwd": run_fwd, "lse": run_lse, "vit": run_vit}[kind](lib, name, **kw)
    torch.cuda.synchronize()
    return {k: digest(v) for k, v in ins.items()}, {k: digest(v) for k, v in outs.items()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--lib", required=True, help="the libnova_hip.so whose bits are recorded")
    ap.add_argument("--commit", default=None, help="hash of the commit that library was built from (default: git rev-parse HEAD)")
    ap.add_argument("--out", default=os.path.join(HERE, "attn_fwd_bits.json"))
    args = ap.parse_args()
    commit = args.commit or subprocess.run(["git", "-C", ROOT, "rev-parse", "HEAD"], check=True, capture_output=True, text=True).stdout.strip()
    lib = bind(args.lib)
    fixture = {"meta": {"commit": commit, "device": torch.cuda.get_device_name(0)}, "cases": {}}
    for name in CASES:
        ins, outs = run_case(name, lib)
        fixture["cases"][name] = {"inputs": ins, "outputs": outs}
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(fixture, f, indent=0, sort_keys=True)
        f.write("\n")
    print("->", args.out, f"{len(CASES)} cases, {os.path.getsize(args.out) / 1e3:.1f} kB, commit {commit}")


if __name__ == "__main__":
    main()
