"""Inputs and float64 references of tests/test_gpu_cross_length.py, and the checks on them that need no GPU.

The GPU file compares nova_attn_fwd at Lq != Lk and the KV-cached block stack with the references built here. Two
properties of those references decide whether the GPU tests can fail at all, and both are checked here on the CPU,
without the library:

  * attention: the last key of every (sequence, head) is aligned with one query, so the float64 reference over Lk - 1
    keys differs from the true one by more than the row-wise bound of the GPU test. A kernel that reads one key too few
    (or masks one too many in a ragged tile) cannot pass.
  * KV-cached stack: the row-wise bound of the GPU test is 3 x the error of a torch emulation of the same stack that
    rounds to the storage type at every launch boundary. The emulation's error is stable over seeds 0 to 4 (every seed
    stays under 2 x the error of seed 0, the seed the GPU test uses), so the bound is not an accident of one draw.
"""
import math

import pytest
import torch

DTYPES = [torch.float32, torch.bfloat16, torch.float16]


def tol(dtype):
    """The project's per-dtype bound (tests/test_gpu_kernels.py)."""
    return {torch.float32: 2e-5, torch.bfloat16: 1.6e-2, torch.float16: 2e-3}[dtype]


def row_err(got, ref):
    """max|got - ref| / max|ref| of every row (float64)."""
    got, ref = got.double(), ref.double()
    return (got - ref).abs().amax(1) / ref.abs().amax(1).clamp_min(1e-6)


# ---------------------------------------------------------------------------------------------
# 1. attention with Lq != Lk
# ---------------------------------------------------------------------------------------------
ATTN_S, ATTN_HEADS = 2, 3
# the smallest pairs that cross a 32- / 64-key tile, a 32- / 64-row wave and a 128- / 256-row workgroup, ragged on either side
ATTN_PAIRS = [(1, 1), (1, 65), (5, 333), (17, 64), (33, 63), (128, 129), (129, 31), (257, 200), (300, 769)]
ATTN_SCALES = ["rsqrt", 0.2]  # head_dim ** -0.5, and a value whose product with log2(e) is no power of two


def attn_scale(scale, hd):
    return float(hd) ** -0.5 if scale == "rsqrt" else float(scale)


def attn_spike_row(Lq):
    return 5 % Lq


def attn_last_key_row(s, h, Lq, Lk):
    """The query row the LAST key of (sequence s, head h) is aligned with: a different row per (s, h), never the spike's."""
    r = (Lq - 1 - 3 * (s * ATTN_HEADS + h)) % Lq
    if Lk >= 200 and h == 0 and Lq > 1 and r == attn_spike_row(Lq):
        r = (r + 1) % Lq
    return r


def attn_case(dtype, hd, Lq, Lk):
    """q [S, Lq, heads, hd], k, v [S, Lk, heads, hd] in `dtype` on the CPU. The last key equals one query row, so its score
    |q|^2 * scale (8 or more) sits at that row's maximum; for Lk >= 200 key Lk - 3 of head 0 is 4 x the spike query, a
    late jump of the running maximum (the deferred-rescale path of the online softmax)."""
    g = torch.Generator().manual_seed(100000 * hd + 1000 * Lq + Lk)
    q = torch.randn(ATTN_S, Lq, ATTN_HEADS, hd, generator=g).to(dtype)
    k = torch.randn(ATTN_S, Lk, ATTN_HEADS, hd, generator=g).to(dtype)
    v = torch.randn(ATTN_S, Lk, ATTN_HEADS, hd, generator=g).to(dtype)
    if Lk >= 200:
        k[:, Lk - 3, 0] = (q[:, attn_spike_row(Lq), 0].float() * 4).to(dtype)
    for s in range(ATTN_S):
        for h in range(ATTN_HEADS):
            k[s, Lk - 1, h] = q[s, attn_last_key_row(s, h, Lq, Lk), h]
    return q, k, v


def attn_ref(q, k, v, scale, nkeys=None):
    """float64 softmax attention on the stored values over the first nkeys keys -> [S*Lq, heads*hd] (no key: zeros)."""
    S, Lq, H, hd = q.shape
    nkeys = k.shape[1] if nkeys is None else nkeys
    if nkeys == 0:
        return torch.zeros(S * Lq, H * hd, dtype=torch.float64)
    q, k, v = q.double(), k.double()[:, :nkeys], v.double()[:, :nkeys]
    p = torch.softmax(torch.einsum("sihc,sjhc->shij", q, k) * scale, -1)
    return torch.einsum("shij,sjhc->sihc", p, v).reshape(S * Lq, H * hd)


def attn_teeth(q, k, v, scale):
    """Per sequence, the largest row-wise distance between the reference and the reference without the last key."""
    S, Lq = q.shape[:2]
    d = row_err(attn_ref(q, k, v, scale, k.shape[1] - 1), attn_ref(q, k, v, scale))
    return d.view(S, Lq).amax(1)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("hd", [64, 96])
@pytest.mark.parametrize("scale", ATTN_SCALES)
@pytest.mark.parametrize("Lq,Lk", ATTN_PAIRS)
def test_attention_inputs_tell_a_dropped_last_key(dtype, hd, scale, Lq, Lk):
    q, k, v = attn_case(dtype, hd, Lq, Lk)
    teeth = attn_teeth(q, k, v, attn_scale(scale, hd))
    # 4 x the bound the GPU test allows: a result within the bound of the true reference is far from the dropped one
    assert teeth.min().item() > 4 * 2.5 * tol(dtype), teeth.tolist()


# ---------------------------------------------------------------------------------------------
# 4. the KV-cached block stack, chunk by chunk
# ---------------------------------------------------------------------------------------------
KV_S, KV_NB, KV_BLOCKS, KV_CAP = 2, 2, 2, 160
KV_CHUNKS = (37, 64, 29)  # cache_len 0, 37, 101; Lk 37, 101, 130
KV_SHAPES = [(128, 2), (384, 4)]  # (D, heads): head_dim 64 and 96
KV_FLOOR = 2e-5  # the float32 tol: the emulation's float32 error (1e-7) says nothing about summation order inside a launch
BLOCK_KEYS = ("qkv_w", "qkv_b", "proj_w", "proj_b", "norm1_w", "norm1_b", "fc1_w", "fc1_b", "fc2_w", "fc2_b", "norm2_w", "norm2_b")


def bf16r(t):
    return t.to(torch.bfloat16).float()


def make_blocks(nblocks, D, hidden, g):
    """Block parameters as float32 tensors holding bfloat16-representable values (GEMM weights scaled by fan_in ** -0.5)."""
    r = lambda *shape, scale=1.0: bf16r(torch.randn(*shape, generator=g) * scale)
    blocks = []
    for _ in range(nblocks):
        blocks.append(dict(
            qkv_w=r(3 * D, D, scale=D ** -0.5), qkv_b=r(3 * D, scale=0.1), proj_w=r(D, D, scale=D ** -0.5), proj_b=r(D, scale=0.1),
            norm1_w=bf16r(1 + 0.1 * torch.randn(D, generator=g)), norm1_b=r(D, scale=0.1),
            fc1_w=r(hidden, D, scale=D ** -0.5), fc1_b=r(hidden, scale=0.1), fc2_w=r(D, hidden, scale=hidden ** -0.5),
            fc2_b=r(D, scale=0.1), norm2_w=bf16r(1 + 0.1 * torch.randn(D, generator=g)), norm2_b=r(D, scale=0.1)))
    return blocks


def make_rope(nb, L, hd, g):
    """[nb, L, hd/2, 2] f32 (cos, sin) of independent random angles: every batch entry and row has its own table."""
    ang = torch.rand(nb, L, hd // 2, generator=g) * (2 * math.pi)
    return torch.stack([ang.cos(), ang.sin()], -1).float().contiguous()


def rotate(t, tab):
    """Pairwise rotation of t [S, L, heads, hd] (float64) by tab [nb, L, hd/2, 2]; sequence s uses tab[s % nb]."""
    S, L, H, hd = t.shape
    tab = tab.double()[torch.arange(S) % tab.shape[0]]  # [S, L, hd/2, 2]
    cos, sin = tab[..., 0][:, :, None], tab[..., 1][:, :, None]
    p = t.reshape(S, L, H, hd // 2, 2)
    x0, x1 = p[..., 0], p[..., 1]
    return torch.stack([cos * x0 - sin * x1, sin * x0 + cos * x1], -1).reshape(S, L, H, hd)


def layer_norm(t, w, b, eps=1e-5):
    mu = t.mean(-1, keepdim=True)
    var = ((t - mu) ** 2).mean(-1, keepdim=True)
    return (t - mu) / torch.sqrt(var + eps) * w.double() + b.double()


def gelu(t):
    return 0.5 * t * (1 + torch.erf(t / math.sqrt(2.0)))


def kv_case(D, heads, seed=0):
    g = torch.Generator().manual_seed(7000 + 10 * D + seed)
    total = sum(KV_CHUNKS)
    return dict(D=D, heads=heads, hidden=4 * D, blocks=make_blocks(KV_BLOCKS, D, 4 * D, g),
                x=bf16r(torch.randn(KV_S, total, D, generator=g)), rope=make_rope(KV_NB, total, D // heads, g))


def kv_stack(case, dtype, chunks, emulate):
    """The KV-cached post-norm stack in float64 torch, fed chunk by chunk (chunk c's queries see the keys of chunks <= c).
    emulate: every launch's output (QKV - q with the softmax scale folded in for the 16-bit types, as the library's QKV
    epilogue does -, attention, each GEMM, each row norm) is rounded to `dtype`. Returns the output rows of every chunk
    [S, L, D] and, per block, the cache rows [S, sum(chunks), 2D] (rotated k | v)."""
    D, H = case["D"], case["heads"]
    hd = D // H
    S = case["x"].shape[0]
    scale = 1.0 / math.sqrt(hd)
    rd = (lambda t: t.to(dtype).double()) if emulate else (lambda t: t)
    fold = scale * 1.4426950408889634 if emulate and dtype != torch.float32 else 1.0
    blocks = [{k: b[k].to(dtype if k.endswith("_w") and not k.startswith("norm") else torch.float32).double() for k in BLOCK_KEYS}
              for b in case["blocks"]]
    caches = [torch.zeros(S, 0, 2 * D, dtype=torch.float64) for _ in blocks]
    outs, pos = [], 0
    for L in chunks:
        x = case["x"][:, pos:pos + L].to(dtype).double()
        tab = case["rope"][:, pos:pos + L]
        for i, b in enumerate(blocks):
            qkv = (x @ b["qkv_w"].T + b["qkv_b"]).view(S, L, 3, H, hd)
            q, k, v = rotate(qkv[:, :, 0], tab), rotate(qkv[:, :, 1], tab), qkv[:, :, 2]
            q, k, v = rd(q * fold) / fold, rd(k), rd(v)
            caches[i] = torch.cat([caches[i], torch.cat([k.reshape(S, L, D), v.reshape(S, L, D)], -1)], 1)
            kk = caches[i][..., :D].reshape(S, -1, H, hd)
            vv = caches[i][..., D:].reshape(S, -1, H, hd)
            p = torch.softmax(torch.einsum("sihc,sjhc->shij", q, kk) * scale, -1)
            a = rd(torch.einsum("shij,sjhc->sihc", p, vv).reshape(S, L, D))
            y = rd(a @ b["proj_w"].T + b["proj_b"])
            x = rd(layer_norm(y, b["norm1_w"], b["norm1_b"]) + x)
            h = rd(gelu(x @ b["fc1_w"].T + b["fc1_b"]))
            y = rd(h @ b["fc2_w"].T + b["fc2_b"])
            x = rd(layer_norm(y, b["norm2_w"], b["norm2_b"]) + x)
        outs.append(x)
        pos += L
    return outs, caches


def kv_emulation_error(case, dtype):
    """(reference outputs, reference caches, the emulation's largest row-wise error against them over all chunks)."""
    ref, ref_caches = kv_stack(case, dtype, KV_CHUNKS, emulate=False)
    emu, _ = kv_stack(case, dtype, KV_CHUNKS, emulate=True)
    err = max(row_err(e.reshape(-1, case["D"]), r.reshape(-1, case["D"])).max().item() for e, r in zip(emu, ref))
    return ref, ref_caches, err


def kv_bound(emu_err):
    return max(3 * emu_err, KV_FLOOR)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("D,heads", KV_SHAPES)
def test_kv_stack_emulation_error_is_stable_over_seeds(dtype, D, heads):
    """Every seed's emulation error stays under the GPU test's bound (3 x the error of seed 0, floored at 2e-5) with a factor
    1.5 to spare. Measured largest row-wise error of the emulation against float64, seed 0 (largest of seeds 0 to 4):
        float32   D 128: 1.70e-07 (1.72e-07)   D 384: 1.45e-07 (1.64e-07)
        bfloat16  D 128: 1.06e-02 (1.20e-02)   D 384: 8.62e-03 (1.40e-02)
        float16   D 128: 1.44e-03 (1.78e-03)   D 384: 1.30e-03 (1.40e-03)"""
    errs = [kv_emulation_error(kv_case(D, heads, seed), dtype)[2] for seed in range(5)]
    bound = kv_bound(errs[0])  # what the GPU test uses
    print(f"emulation row-wise error {dtype} D={D}: " + " ".join(f"{e:.3e}" for e in errs) + f" bound {bound:.3e}")
    assert max(errs) < bound / 1.5, (errs, bound)
