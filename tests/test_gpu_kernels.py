"""Per-kernel numerics of libnova_hip.so against plain PyTorch fp32 math (GPU box only).

Every call goes through the C ABI (ctypes). Tolerances: f32 mode runs on exact-f32 MFMA so only
summation order differs (1e-5 relative to the row scale); bf16 mode is bounded by bf16 storage
rounding of inputs/outputs (2^-8 relative) with f32 accumulation, f16 mode (the reference callers' default precision,
scripts/app_nova_t2i.py:36) likewise by 2^-11.
"""
import math

import pytest
import torch

pytestmark = pytest.mark.gpu

DEV = "cuda"
DTYPES = [torch.float32, torch.bfloat16, torch.float16]
HALF = [torch.bfloat16, torch.float16]  # the two 16-bit storage modes run the same kernels on the bf16 / f16 MFMA forms


def tol(dtype):
    return {torch.float32: 2e-5, torch.bfloat16: 1.6e-2, torch.float16: 2e-3}[dtype]


def relerr(got, ref):
    got, ref = got.float(), ref.float()
    return ((got - ref).abs().max() / ref.abs().max().clamp_min(1e-12)).item()


def rnd(*shape, dtype=torch.float32, scale=1.0, seed=0):
    g = torch.Generator().manual_seed(seed + sum(shape))
    return (torch.randn(*shape, generator=g) * scale).to(DEV).to(dtype)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("M,N,K", [(128, 128, 64), (300, 256, 128), (389, 384, 512), (1, 128, 256), (1024, 1024, 1024)])
@pytest.mark.parametrize("act", [0, 1, 2])
def test_gemm_bias_act(hip, dtype, M, N, K, act):
    a, w = rnd(M, K, dtype=dtype, seed=1), rnd(N, K, dtype=dtype, scale=K ** -0.5, seed=2)
    bias = rnd(N, seed=3)
    out = hip.gemm_bias_act(a, w, bias, act)
    ref = a.float() @ w.float().T + bias
    ref = [lambda x: x, torch.nn.functional.gelu, torch.nn.functional.silu][act](ref)
    assert out.shape == (M, N) and out.dtype == dtype
    assert relerr(out, ref) < tol(dtype)


@pytest.mark.parametrize("tile", [128, 256])
def test_gelu_epilogue_pointwise_accuracy(hip, force_tile, tile):
    """W = I makes the accumulator equal the bf16 input exactly, so the epilogue's GELU is seen pointwise: every bf16
    value in [-16, 16] must come out within 2.6e-5 (the fitted form's bound, csrc/common.h) plus the final bf16
    rounding of the exact erf GELU (reference: nn.GELU() on the fc1 output, vision_transformer.py:36)."""
    vals = torch.arange(0, 65536, dtype=torch.int32).to(torch.int16).view(torch.bfloat16)
    vals = vals[torch.isfinite(vals.float()) & (vals.float().abs() <= 16)]
    K = N = 256
    M = (vals.numel() + K - 1) // K
    a = torch.zeros(M * K, dtype=torch.bfloat16)
    a[: vals.numel()] = vals
    a = a.view(M, K).to(DEV)
    force_tile(tile)
    out = hip.gemm_bias_act(a, torch.eye(K, dtype=torch.bfloat16, device=DEV), None, 1).float().cpu().double()
    x = a.float().cpu().double()
    exact = 0.5 * x * (1 + torch.erf(x / 2 ** 0.5))
    half_ulp = exact.abs().clamp_min(2.0 ** -126) * 2.0 ** -8  # generous half-ulp bound of a bf16 result
    assert ((out - exact).abs() <= 2.6e-5 + half_ulp).all()


def test_gemm_layout_asymmetric(hip):
    """A = I against an asymmetric W catches a transposed C write or a wrong fragment map."""
    K = N = 128
    a = torch.eye(K, device=DEV)
    w = (torch.arange(N * K, device=DEV, dtype=torch.float32).view(N, K) % 251) - 125.0
    for dtype in DTYPES:
        out = hip.gemm_bias_act(a.to(dtype), w.to(dtype), None, 0)
        assert torch.equal(out.float(), w.T.contiguous())


def test_gemm_rejects_bad_shapes(hip):
    a, w = rnd(8, 64), rnd(100, 64)
    with pytest.raises(hip.NovaHipError):
        hip.gemm_bias_act(a, w)


def ref_rope_table(pos, ids, pad, hd, theta=10000.0):
    """embeddings.py:59-67 restated for the test: returns cos, sin [nb, pad + n, hd/2]."""
    if ids is not None:
        pos = pos[ids]  # [nb, n, 3]
    else:
        pos = pos[None]
    pos = torch.nn.functional.pad(pos, (0, 0, pad, 0))
    dims = [hd // 8] + [(hd - hd // 8) // 2] * 2
    ang = []
    for i, rd in enumerate(dims):
        scale = torch.arange(0, rd, 2, device=pos.device).float() / rd
        ang.append(pos[..., i:i + 1] * torch.pow(theta, scale).reciprocal())
    ang = torch.cat(ang, -1)
    return ang.cos(), ang.sin()


def inv_freq(hd, theta=10000.0):
    dims = [hd // 8] + [(hd - hd // 8) // 2] * 2
    return torch.cat([torch.pow(theta, torch.arange(0, rd, 2).float() / rd).reciprocal() for rd in dims]).to(DEV)


def grid_pos(h, w):
    t = torch.zeros(h * w)
    hh = torch.arange(h).repeat_interleave(w).float()
    ww = torch.arange(w).repeat(h).float()
    return torch.stack([t, hh, ww], -1).to(DEV)


@pytest.mark.parametrize("hd", [64, 96])
def test_rope_table(hip, hd):
    pad, nb = 5, 3
    pos = grid_pos(6, 7)
    g = torch.Generator().manual_seed(0)
    ids = torch.stack([torch.randperm(42, generator=g)[:17] for _ in range(nb)]).to(DEV)
    for use_ids in (ids, None):
        tab = hip.rope_table(pos, use_ids, pad, inv_freq(hd), nb, hd)
        cos, sin = ref_rope_table(pos, use_ids, pad, hd)
        cos, sin = cos.expand(nb, -1, -1), sin.expand(nb, -1, -1)
        assert torch.allclose(tab[..., 0], cos, atol=2e-6) and torch.allclose(tab[..., 1], sin, atol=2e-6)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("D,heads", [(128, 2), (384, 4)])
def test_qkv_rope(hip, dtype, D, heads):
    S, L, nb = 4, 37, 2
    hd = D // heads
    x, w, b = rnd(S * L, D, dtype=dtype), rnd(3 * D, D, dtype=dtype, scale=D ** -0.5, seed=5), rnd(3 * D, seed=6)
    pos = grid_pos(8, 8)
    g = torch.Generator().manual_seed(1)
    ids = torch.stack([torch.randperm(64, generator=g)[: L - 7] for _ in range(nb)]).to(DEV)
    tab = hip.rope_table(pos, ids, 7, inv_freq(hd), nb, hd)
    out = hip.qkv_rope(x, w, b, tab, S, L, heads)
    ref = (x.float() @ w.float().T + b).view(S, L, 3, heads, hd)
    cos = tab[..., 0].repeat(S // nb, 1, 1)[:, :, None, None, :]  # sequence s uses table s % nb
    sin = tab[..., 1].repeat(S // nb, 1, 1)[:, :, None, None, :]
    qk = ref[:, :, :2].reshape(S, L, 2, heads, hd // 2, 2)
    x0, x1 = qk[..., 0], qk[..., 1]
    rot = torch.stack([cos * x0 - sin * x1, sin * x0 + cos * x1], -1).view(S, L, 2, heads, hd)
    ref = torch.cat([rot, ref[:, :, 2:]], 2).view(S * L, 3 * D)
    assert relerr(out, ref) < tol(dtype)
    out2 = hip.qkv_rope(x, w, b, None, S, L, heads)
    assert relerr(out2, x.float() @ w.float().T + b) < tol(dtype)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("hd", [64, 96])
@pytest.mark.parametrize("S,heads,L", [(1, 1, 64), (2, 2, 128), (2, 3, 200), (1, 2, 333), (3, 1, 31), (1, 4, 769)])
def test_attention(hip, dtype, hd, S, heads, L):
    D = heads * hd
    qkv = rnd(S * L, 3 * D, dtype=dtype, seed=7)
    out = hip.attn_fwd_packed(qkv, S, L, heads)
    q, k, v = qkv.float().view(S, L, 3, heads, hd).permute(2, 0, 3, 1, 4)
    ref = torch.nn.functional.scaled_dot_product_attention(q, k, v).transpose(1, 2).reshape(S * L, D)
    assert relerr(out, ref) < tol(dtype)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("hd", [64, 96])
def test_attention_spiky_rows(hip, dtype, hd):
    """Force large running-max jumps late in the key stream (online-softmax rescale path)."""
    S, heads, L = 1, 1, 320
    qkv = rnd(S * L, 3 * hd, dtype=dtype, seed=9)
    q = qkv[:, :hd].float()
    qkv[300, hd:2 * hd] = (q[5] * 4).to(dtype)   # key 300 aligned with query 5
    qkv[170, hd:2 * hd] = (q[77] * 3).to(dtype)
    out = hip.attn_fwd_packed(qkv, S, L, heads)
    qq, k, v = qkv.float().view(S, L, 3, heads, hd).permute(2, 0, 3, 1, 4)
    ref = torch.nn.functional.scaled_dot_product_attention(qq, k, v).transpose(1, 2).reshape(S * L, hd)
    assert relerr(out, ref) < tol(dtype)


@pytest.mark.parametrize("dtype", HALF)
@pytest.mark.parametrize("hd", [64, 96])
def test_attention_non_finite_rows_stay_in_their_row(hip, dtype, hd):
    """The contract of nova_attn_fwd for non-finite inputs (include/nova_hip.h; attn16.hip is compiled with -fno-honor-nans, so
    its max / compare instructions are free to ignore a NaN): a query row whose scores are not all finite - a NaN in the query
    (query 37), or scores that overflow to +inf (query 150: 1e30 against a key row of 1e30s) - comes out non-finite in ITS
    output row, as F.scaled_dot_product_attention's would (softmax of a NaN or of inf - inf), and every other output row is
    bit for bit what the clean input gives: nothing a lane decides wave-wide (the deferred-rescale branch) leaks a row's
    NaN or inf into its neighbours."""
    S, heads, L = 2, 2, 333
    D = heads * hd
    clean = rnd(S * L, 3 * D, dtype=dtype, seed=21)
    ref = hip.attn_fwd_packed(clean.clone(), S, L, heads)
    bad = clean.clone()
    bad[37, 5] = float("nan")                      # head 0 of sequence 0, query 37
    bad[150, :hd] = 1e30                           # head 0, query 150 ...
    bad[200, D:D + hd] = 1e30                      # ... against key 200: the score overflows f32
    out = hip.attn_fwd_packed(bad, S, L, heads)
    torch.cuda.synchronize()
    poisoned = torch.zeros(S * L, D, dtype=torch.bool, device=out.device)
    poisoned[37, :hd] = True
    poisoned[150, :hd] = True
    # key 200 of head 0 is huge for EVERY query of sequence 0, head 0: those rows are dominated by (or overflow on) it - finite or
    # not, they differ from the clean run by construction; the contract is about all other (sequence, head) pairs and rows
    touched = torch.zeros_like(poisoned)
    touched[:L, :hd] = True
    assert torch.equal(out[~touched], ref[~touched])
    assert not torch.isfinite(out[37, :hd].float()).any()
    assert not torch.isfinite(out[150, :hd].float()).any()


@pytest.mark.parametrize("dtype", HALF)
@pytest.mark.parametrize("variant", [0, 1, 2, 3, 4, 5])
@pytest.mark.parametrize("S,heads,L", [(1, 1, 64), (2, 3, 200), (1, 2, 333), (3, 1, 31), (1, 4, 769), (2, 2, 2560)])
def test_attention_structures_16bit(hip, dtype, variant, S, heads, L):
    """The three bf16 / head_dim 64 structures (32x32x16; 16x16x32 at 32 and at 64 query rows per wave) against SDPA in f32,
    incl. ragged last tiles and the forced late-max rescale (cdna_hip_programming rule 26)."""
    hd = 64
    D = heads * hd
    qkv = rnd(S * L, 3 * D, dtype=dtype, seed=7)
    if L >= 200:  # spike: key L-3 aligned with query 5, key 70 with query 77 of head 0 -> the running max jumps late in the stream
        q = qkv[:, :hd].float()
        qkv[L - 3, D:D + hd] = (q[5] * 4).to(dtype)
        qkv[70, D:D + hd] = (q[77] * 3).to(dtype)
    q, k, v = qkv.float().view(S, L, 3, heads, hd).permute(2, 0, 3, 1, 4)
    ref = torch.nn.functional.scaled_dot_product_attention(q, k, v).transpose(1, 2).reshape(S * L, D)
    try:
        hip.call("nova_debug_set_attn_variant", variant)
        out = hip.attn_fwd_packed(qkv, S, L, heads)
    finally:
        hip.call("nova_debug_set_attn_variant", -1)
    assert relerr(out, ref) < tol(dtype)
    # row-wise: every query row within bf16 rounding of the reference row (a wrong lane map hides in a global norm)
    row_err = (out.float() - ref).abs().amax(1) / ref.abs().amax(1).clamp_min(1e-6)
    assert row_err.max().item() < 2.5 * tol(dtype), (variant, row_err.argmax().item(), row_err.max().item())


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("D", [128, 768, 1024, 1536])
def test_row_norm_variants(hip, dtype, D):
    rows = 37
    x, res = rnd(rows, D, dtype=dtype, seed=11), rnd(rows, D, dtype=dtype, seed=12)
    gamma, beta = rnd(D, seed=13) + 1, rnd(D, seed=14)
    mod = rnd(rows, 5 * D, dtype=dtype, scale=0.5, seed=15)
    ln = lambda t, eps: torch.nn.functional.layer_norm(t.float(), (D,), None, None, eps)
    # ViT post-norm residual, in place on the residual stream
    r = res.clone()
    hip.row_norm(x, out=r, gamma=gamma, beta=beta, res=r, eps=1e-5)
    assert relerr(r, ln(x, 1e-5) * gamma + beta + res.float()) < tol(dtype)
    # AdaLN-Zero modulate
    o = hip.row_norm(x, mod=mod, scale_off=D, shift_off=2 * D, eps=1e-6)
    assert relerr(o, ln(x, 1e-6) * (1 + mod[:, D:2 * D].float()) + mod[:, 2 * D:3 * D].float()) < tol(dtype)
    # gate * LN_affine + residual
    o = hip.row_norm(x, gamma=gamma, beta=beta, mod=mod, gate_off=4 * D, res=res, eps=1e-5)
    assert relerr(o, (ln(x, 1e-5) * gamma + beta) * mod[:, 4 * D:].float() + res.float()) < tol(dtype)
    # gathered rows
    idx = torch.tensor([5, 0, 36, 36, 7], dtype=torch.int32, device=DEV)
    o = hip.row_norm(x, gamma=gamma, beta=beta, gather=idx, eps=1e-5)
    assert relerr(o, (ln(x, 1e-5) * gamma + beta)[idx.long()]) < tol(dtype)


@pytest.mark.parametrize("dtype", DTYPES)
def test_token_plumbing(hip, dtype):
    B, N, P, D, Lp, S = 2, 24, 3, 128, 5, 4
    canvas, mask = rnd(B, N, P, seed=20), (torch.rand(B, N, device=DEV) > 0.5).float()
    w, b, tok, pe = rnd(D, P, dtype=dtype), rnd(D, seed=21), rnd(1, D, dtype=dtype, seed=22), rnd(N, D, dtype=dtype, seed=23)
    z0 = torch.empty(B, N, D, dtype=dtype, device=DEV)
    c = hip.dtype_code(dtype)
    for pos_embed in (None, pe):
        hip.call("nova_embed_canvas", hip.ptr(canvas), hip.ptr(mask), hip.ptr(w), hip.ptr(b), hip.ptr(tok),
                 hip.ptr(pos_embed), hip.ptr(z0), B, N, P, D, c, hip.stream_ptr())
        e = canvas @ w.float().T + b
        ref = e * (1 - mask[..., None]) + tok.float() * mask[..., None]
        ref = ref + pe.float() if pos_embed is not None else ref
        assert relerr(z0, ref) < tol(dtype)
    prefix = rnd(S, Lp, D, dtype=dtype, seed=24)
    g = torch.Generator().manual_seed(3)
    ids = torch.stack([torch.randperm(N, generator=g)[:9] for _ in range(B)]).to(DEV)
    x1 = torch.empty(S, Lp + 9, D, dtype=dtype, device=DEV)
    hip.call("nova_build_sequence", hip.ptr(prefix), Lp, hip.ptr(z0), N, hip.ptr(ids), hip.ptr(x1), S, B, Lp, 9, D, c,
             hip.stream_ptr())
    zz = torch.cat([z0, z0])
    ref1 = torch.cat([prefix, zz.gather(1, torch.cat([ids, ids])[..., None].expand(-1, -1, D))], 1)
    assert torch.equal(x1, ref1)
    x2 = torch.empty(S, Lp + N, D, dtype=dtype, device=DEV)
    hip.call("nova_build_sequence", hip.ptr(x1), Lp + 9, hip.ptr(z0), N, None, hip.ptr(x2), S, B, Lp, N, D, c,
             hip.stream_ptr())
    x1m = x1 * 2
    hip.call("nova_scatter_tokens", hip.ptr(x1m), hip.ptr(ids), hip.ptr(x2), S, B, Lp, N, 9, D, c, hip.stream_ptr())
    ref2 = torch.cat([x1[:, :Lp], zz.scatter(1, torch.cat([ids, ids])[..., None].expand(-1, -1, D), x1m[:, Lp:])], 1)
    assert torch.equal(x2, ref2)
    # shared token rows (video-encoder bos canvas): tok_batch_rows = 0
    shared = rnd(7, D, dtype=dtype, seed=25)
    xv = torch.empty(S, Lp + 7, D, dtype=dtype, device=DEV)
    hip.call("nova_build_sequence", hip.ptr(prefix), Lp, hip.ptr(shared), 0, None, hip.ptr(xv), S, B, Lp, 7, D, c,
             hip.stream_ptr())
    assert torch.equal(xv, torch.cat([prefix, shared.expand(S, -1, -1)], 1))


@pytest.mark.parametrize("dtype", DTYPES)
def test_decoder_glue(hip, dtype):
    B, n, P, D, S = 3, 5, 3, 256, 6
    c = hip.dtype_code(dtype)
    a, vec = rnd(S * n, D, dtype=dtype, seed=30), rnd(D, dtype=dtype, seed=31)
    out = torch.empty_like(a)
    hip.call("nova_silu_add_rows", hip.ptr(a), hip.ptr(vec), hip.ptr(out), S * n, D, c, hip.stream_ptr())
    assert relerr(out, torch.nn.functional.silu(a.float() + vec.float())) < tol(dtype)
    t = torch.tensor([1000.0, 500.25, 1.0], device=DEV)
    freq = torch.arange(128, dtype=torch.float32, device=DEV).mul(-math.log(10000.0) / 128).exp()
    fe = torch.empty(3, 256, dtype=dtype, device=DEV)
    hip.call("nova_timestep_freq", hip.ptr(t), hip.ptr(freq), hip.ptr(fe), 3, 256, c, hip.stream_ptr())
    emb = t[:, None] * freq[None]
    assert (fe.float() - torch.cat([emb.cos(), emb.sin()], -1)).abs().max() < (1e-4 if dtype == torch.float32 else 8e-3)
    x = rnd(B, n, P, seed=32)
    w, b = rnd(D, P, dtype=dtype, seed=33), rnd(D, seed=34)
    u = torch.empty(S * n, D, dtype=dtype, device=DEV)
    hip.call("nova_patch_embed_rows", hip.ptr(x), hip.ptr(w), hip.ptr(b), hip.ptr(u), S, B, n, P, D, c, hip.stream_ptr())
    assert relerr(u, torch.cat([x, x]).view(S * n, P) @ w.float().T + b) < tol(dtype)
    h = rnd(S * n, D, dtype=dtype, seed=35)
    hw, hb = rnd(P, D, dtype=dtype, scale=D ** -0.5, seed=36), rnd(P, seed=37)
    for cfg, g in ((1, 5.0), (0, 1.0)):
        xx = x.clone()
        hip.call("nova_head_cfg_euler", hip.ptr(h), hip.ptr(hw), hip.ptr(hb), hip.ptr(xx), B, n, P, D, g, cfg, -0.04, c,
                 hip.stream_ptr())
        pred = (h.float() @ hw.float().T + hb).view(S, n, P)
        v = pred[B:] + (pred[:B] - pred[B:]) * g if cfg else pred[:B]
        assert relerr(xx, x + (-0.04) * v) < tol(dtype)


# ---------------------------------------------------------------------------------------------
# the 256x256 ping-pong GEMM (large M) must be bit-identical to the 128x128 structure: same MFMA,
# same k order per output element. Any LDS race (stale or half-landed tile) breaks equality.
# ---------------------------------------------------------------------------------------------
# the two 256x256 structures: one tile per workgroup (2560 + 2: its shipped schedule variant) and the persistent
# one-workgroup-per-CU form (2560 + 20)
TILE256_FORMS = [257, 258, 256]  # one tile per workgroup, persistent with a per-tile prologue (fallback forms), the shipped choice (continuous K-stream where K allows)


@pytest.fixture()
def force_tile(hip):
    def _force(tile):
        hip.call("nova_debug_force_gemm_tile", tile)
    yield _force
    hip.call("nova_debug_force_gemm_tile", 0)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("M,N,K,act", [(256, 256, 64, 0), (300, 256, 128, 2), (1000, 512, 192, 1), (4096, 256, 1024, 0),
                                        (8192 + 77, 1024, 1024, 1), (2560 * 3 + 1, 768, 3072, 0)])
@pytest.mark.parametrize("form", TILE256_FORMS)
def test_gemm_256_tile_bitwise_equals_128_tile(hip, force_tile, form, dtype, M, N, K, act):
    a, w = rnd(M, K, dtype=dtype, seed=41), rnd(N, K, dtype=dtype, scale=K ** -0.5, seed=42)
    bias = rnd(N, seed=43)
    force_tile(128)
    ref = hip.gemm_bias_act(a, w, bias, act)
    force_tile(form)
    out = hip.gemm_bias_act(a, w, bias, act)
    assert torch.equal(out, ref)
    full = a.float() @ w.float().T + bias
    full = [lambda x: x, torch.nn.functional.gelu, torch.nn.functional.silu][act](full)
    assert relerr(out, full) < tol(dtype)


@pytest.mark.parametrize("M,N,K", [(5120, 1024, 1024), (5120, 1024, 4096), (5120, 3072, 1024), (10240, 1024, 1024), (40960, 1024, 1024)])
def test_gemm_automatic_kernel_choice_never_shows_in_the_output(hip, force_tile, M, N, K):
    """The library picks the tile structure by shape (gemm.hip: the persistent 256 kernel from M >= 4096 rows on, unless its tiles
    would cover less than half the CUs - batch 1's out-projection and fc2, 80 tiles - where the 128 tile takes the launch).
    Whatever it picks is bit-identical to both forced structures, so batch size and the rule's threshold never change a result."""
    a, w = rnd(M, K, dtype=torch.bfloat16, seed=51), rnd(N, K, dtype=torch.bfloat16, scale=K ** -0.5, seed=52)
    bias = rnd(N, seed=53)
    auto = hip.gemm_bias_act(a, w, bias, 0)
    force_tile(128)
    t128 = hip.gemm_bias_act(a, w, bias, 0)
    force_tile(256)
    t256 = hip.gemm_bias_act(a, w, bias, 0)
    assert torch.equal(auto, t128) and torch.equal(auto, t256)
    assert relerr(auto, a.float() @ w.float().T + bias) < tol(torch.bfloat16)


@pytest.mark.parametrize("M,N,K,act", [(1, 768, 768, 0), (16, 768, 768, 2), (200, 768, 768, 2), (257, 3072, 768, 1), (999, 1024, 1024, 2),
                                        (130, 4096, 1024, 1), (64, 64, 1024, 0), (1500, 1024, 1024, 2), (3000, 768, 768, 0)])
@pytest.mark.parametrize("dtype", HALF)
def test_small_m_gemm_bitwise_equals_tile_kernels(hip, force_tile, dtype, M, N, K, act):
    """skinny.hip (whole-K workgroups, weights global -> registers) against the 128-tile kernel, bit for bit: the kernel
    picked by the row count must never show in the result (batch / lane splits of the engine rely on it)."""
    a, w = rnd(M, K, dtype=dtype, seed=51), rnd(N, K, dtype=dtype, scale=K ** -0.5, seed=52)
    bias = rnd(N, seed=53)
    force_tile(16)
    out = hip.gemm_bias_act(a, w, bias, act)
    out_nb = hip.gemm_bias_act(a, w, None, act)
    if N % 128 == 0:
        force_tile(128)
        assert torch.equal(out, hip.gemm_bias_act(a, w, bias, act))
        assert torch.equal(out_nb, hip.gemm_bias_act(a, w, None, act))
    full = a.float() @ w.float().T + bias
    full = [lambda x: x, torch.nn.functional.gelu, torch.nn.functional.silu][act](full)
    assert relerr(out, full) < tol(dtype)
    for code in (161, 162, 164):  # 16 / 32 / 64 rows per workgroup: a weight fragment serves 1 / 2 / 4 row blocks
        force_tile(code)
        assert torch.equal(out, hip.gemm_bias_act(a, w, bias, act)), code
    force_tile(0)  # the automatic choice (small-M kernel at these sizes where it pays) gives the same bits again
    assert torch.equal(out, hip.gemm_bias_act(a, w, bias, act))


@pytest.mark.parametrize("M,N,K,act", [(1, 128, 64, 0), (63, 256, 128, 1), (64, 1024, 1024, 2), (65, 768, 768, 0), (400, 1536, 1536, 2), (1152, 1024, 1024, 0),
                                        (1632, 1024, 1024, 2), (1000, 3072, 1024, 0), (2047, 1536, 1536, 1), (3264, 1024, 1024, 0), (517, 1024, 4096, 0)])
@pytest.mark.parametrize("dtype", DTYPES)
def test_gemm_64_tile_bitwise_equals_128_tile(hip, force_tile, dtype, M, N, K, act):
    """gemm.hip's 64 x 64 tile (the launches of the denoising loop, where 128 x 128 tiles would leave CUs idle: forced here, chosen by
    tile count otherwise) against the 128 x 128 tile, bit for bit, with and without bias, ragged last row tile included; the automatic
    choice between the small-M kernel, the 64 tile and the 128 tile gives the same bits again."""
    a, w = rnd(M, K, dtype=dtype, seed=57), rnd(N, K, dtype=dtype, scale=K ** -0.5, seed=58)
    bias = rnd(N, seed=59)
    force_tile(128)
    ref, ref_nb = hip.gemm_bias_act(a, w, bias, act), hip.gemm_bias_act(a, w, None, act)
    force_tile(64)
    pad = torch.full((M + 2, N), 7.0, dtype=dtype, device="cuda")   # rows beyond M stay untouched
    out = hip.gemm_bias_act(a, w, bias, act, out=pad[:M])
    assert torch.equal(out, ref) and torch.equal(hip.gemm_bias_act(a, w, None, act), ref_nb)
    assert bool((pad[M:] == 7.0).all())
    force_tile(0)
    assert torch.equal(hip.gemm_bias_act(a, w, bias, act), ref)
    full = a.float() @ w.float().T + bias
    full = [lambda x: x, torch.nn.functional.gelu, torch.nn.functional.silu][act](full)
    assert relerr(out, full) < tol(dtype)


def test_small_m_gemm_rejects_other_shapes(hip, force_tile):
    force_tile(16)
    a, w = rnd(32, 512, dtype=torch.bfloat16), rnd(128, 512, dtype=torch.bfloat16)
    with pytest.raises(hip.NovaHipError):
        hip.gemm_bias_act(a, w, None, 0)


def _chain_equals_two_row_norms(hip, dtype, D, in_scale=1.0):
    rows = 203
    g, x = rnd(rows, D, dtype=dtype, scale=in_scale, seed=71), rnd(rows, D, dtype=dtype, scale=in_scale, seed=72)
    gamma, beta = rnd(D, seed=73) + 1, rnd(D, seed=74)
    mod = rnd(rows, 5 * D, dtype=dtype, scale=0.5, seed=75)
    x_two = hip.row_norm(g, gamma=gamma, beta=beta, mod=mod, gate_off=4 * D, res=x, eps=1e-5)
    h_two = hip.row_norm(x_two, mod=mod, scale_off=D, shift_off=2 * D, eps=1e-6)
    x_new, h = torch.empty_like(x), torch.empty_like(x)
    hip.call("nova_row_norm_chain", hip.ptr(g), hip.ptr(x), hip.ptr(gamma, torch.float32), hip.ptr(beta, torch.float32), hip.ptr(mod),
             mod.shape[1], 4 * D, D, 2 * D, 1e-5, 1e-6, hip.ptr(x_new), hip.ptr(h), rows, D, hip.dtype_code(dtype), hip.stream_ptr())
    assert torch.equal(x_new, x_two) and torch.equal(h, h_two)
    h2 = torch.empty_like(x)
    hip.call("nova_row_norm_chain", hip.ptr(g), hip.ptr(x), hip.ptr(gamma, torch.float32), hip.ptr(beta, torch.float32), hip.ptr(mod),
             mod.shape[1], 4 * D, D, 2 * D, 1e-5, 1e-6, None, hip.ptr(h2), rows, D, hip.dtype_code(dtype), hip.stream_ptr())
    assert torch.equal(h2, h_two)


CHAIN_WIDTHS = [8, 128, 768, 1024, 1032, 1536, 2048]  # a single lane, one 16-byte chunk over the 2 | 4 chunks-per-lane switch, the full width


@pytest.mark.parametrize("dtype", HALF)
@pytest.mark.parametrize("D", CHAIN_WIDTHS)
def test_row_norm_chain_equals_two_row_norms(hip, dtype, D):
    """Last block's gated norm + residual and the final layer's modulate as one row pass (nova_row_norm_chain) against
    nova_row_norm twice: identical bits for h and for the stored x_new."""
    _chain_equals_two_row_norms(hip, dtype, D)


@pytest.mark.parametrize("dtype", HALF)
@pytest.mark.parametrize("D", CHAIN_WIDTHS)
def test_row_norm_chain_equals_two_row_norms_on_tiny_rows(hip, dtype, D):
    """The same with g and x of 1e-3 N(0,1) (the `tiny` family of tests/test_row_contract_cpu.py): the first norm's variance is about 1e-6,
    so its eps (1e-5, not the second norm's 1e-6) decides rstd, and a chain that hands it the wrong one no longer equals the two launches."""
    _chain_equals_two_row_norms(hip, dtype, D, in_scale=1e-3)


def _adaln_fc1_fused_equals_two_launches(hip, force_tile, dtype, rows, D, N, in_scale=1.0):
    x = rnd(rows, D, dtype=dtype, scale=in_scale, seed=61)
    mod = rnd(rows, 5 * D, dtype=dtype, scale=0.5, seed=62)
    w, bias = rnd(N, D, dtype=dtype, scale=D ** -0.5, seed=63), rnd(N, seed=64)
    force_tile(16)
    fused = hip.adaln_fc1(x, mod, D, 3 * D, w, bias, act=2, eps=1e-6)
    force_tile(128)
    h = hip.row_norm(x, mod=mod, scale_off=D, shift_off=3 * D, eps=1e-6)
    two = hip.gemm_bias_act(h, w, bias, 2)
    assert torch.equal(fused, two)
    assert torch.equal(fused, hip.adaln_fc1(x, mod, D, 3 * D, w, bias, act=2, eps=1e-6))  # forced 128: the two-launch form inside
    ln = torch.nn.functional.layer_norm(x.float(), (D,), None, None, 1e-6)
    hm = (ln * (1 + mod[:, D:2 * D].float()) + mod[:, 3 * D:4 * D].float()).to(dtype).float()
    assert relerr(fused, torch.nn.functional.silu(hm @ w.float().T + bias)) < tol(dtype)
    f32 = [t.float() for t in (x, mod, w)]  # f32 rows always take the two-launch form
    force_tile(0)
    o32 = hip.adaln_fc1(f32[0], f32[1], D, 3 * D, f32[2], bias, act=2, eps=1e-6)
    assert relerr(o32, torch.nn.functional.silu((ln * (1 + f32[1][:, D:2 * D]) + f32[1][:, 3 * D:4 * D]) @ f32[2].T + bias)) < tol(torch.float32)


ADALN_SHAPES = [(1, 768, 768), (37, 768, 768), (256, 768, 768), (300, 1024, 1024), (77, 1024, 2048)]


@pytest.mark.parametrize("rows,D,N", ADALN_SHAPES)
@pytest.mark.parametrize("dtype", HALF)
def test_adaln_fc1_fused_equals_two_launches(hip, force_tile, dtype, rows, D, N):
    """modulate -> fc1 -> SiLU (diffusion_mlp.py:41-47) as ONE launch (LN prologue inside the small-M GEMM) against
    nova_row_norm followed by the GEMM: identical bits, and both close to fp32 math."""
    _adaln_fc1_fused_equals_two_launches(hip, force_tile, dtype, rows, D, N)


@pytest.mark.parametrize("rows,D,N", ADALN_SHAPES)
@pytest.mark.parametrize("dtype", HALF)
def test_adaln_fc1_fused_equals_two_launches_on_tiny_rows(hip, force_tile, dtype, rows, D, N):
    """The same on rows of 1e-3 N(0,1): eps = 1e-6 is as large as the variance, so the LN prologue inside the GEMM and nova_row_norm must
    agree on it to stay bit-identical."""
    _adaln_fc1_fused_equals_two_launches(hip, force_tile, dtype, rows, D, N, in_scale=1e-3)


@pytest.mark.parametrize("form", TILE256_FORMS)
@pytest.mark.parametrize("S,L", [(4, 301), (16, 257), (3, 1400)])
def test_gemm_256_tile_qkv_rope_bitwise(hip, force_tile, form, S, L):
    D, heads, nb = 256, 4, 2
    hd = D // heads
    for dtype in DTYPES:
        x, w, b = rnd(S * L, D, dtype=dtype), rnd(3 * D, D, dtype=dtype, scale=D ** -0.5, seed=5), rnd(3 * D, seed=6)
        side = int((L - 11) ** 0.5) + 1
        pos = grid_pos(side, side)
        g = torch.Generator().manual_seed(1)
        ids = torch.stack([torch.randperm(side * side, generator=g)[: L - 11] for _ in range(nb)]).to(DEV)
        tab = hip.rope_table(pos, ids, 11, inv_freq(hd), nb, hd)
        force_tile(128)
        ref = hip.qkv_rope(x, w, b, tab, S, L, heads)
        force_tile(form)
        out = hip.qkv_rope(x, w, b, tab, S, L, heads)
        assert torch.equal(out, ref)


@pytest.mark.parametrize("form", TILE256_FORMS)
def test_gemm_256_tile_race_screen(hip, force_tile, form):
    """Full-size encoder GEMM shapes, repeated: every launch must reproduce the first bit for bit,
    and match the 128-tile structure (uneven M so that row clamping is exercised)."""
    dtype = torch.bfloat16
    for (M, N, K) in [(64 * 2560, 1024, 1024), (64 * 1347, 3072, 1024), (64 * 2560, 1024, 4096)]:
        a, w = rnd(M, K, dtype=dtype, seed=51), rnd(N, K, dtype=dtype, scale=K ** -0.5, seed=52)
        force_tile(128)
        ref = hip.gemm_bias_act(a, w, None, 0)
        force_tile(form)
        for _ in range(6):
            out = hip.gemm_bias_act(a, w, None, 0)
            assert torch.equal(out, ref)
        del a, w, ref, out


# ---------------------------------------------------------------------------------------------
# MX-fp8 path (BASELINE configs[4]): quantisation + block-scaled MFMA GEMM. The reference has no fp8 path
# (SURVEY section 8d-iv): the kernels are checked against exact arithmetic on the SAME quantised operands, and
# the quantisation error itself is reported against the bf16 GEMM.
# ---------------------------------------------------------------------------------------------
def _dequant(q, scale):
    return q.view(torch.float8_e4m3fn).float() * scale[:, None]


@pytest.mark.parametrize("rows,D", [(1, 128), (37, 1024), (513, 1536), (4096, 4096), (3, 8192), (5, 8)])  # the cap (all 16 chunks live); one lane holds the row
def test_quantize_rows_fp8(hip, rows, D):
    x = rnd(rows, D, dtype=torch.bfloat16, seed=61)
    x[0, :] = 0 if rows > 1 else x[0, :]  # an all-zero row must not divide by zero
    q, scale = hip.quantize_rows_fp8(x)
    amax = x.float().abs().amax(1)
    want_scale = torch.where(amax > 0, amax / 448.0, torch.ones_like(amax))
    assert torch.allclose(scale, want_scale, rtol=1e-6, atol=0)
    want = (x.float() / scale[:, None]).clamp(-448, 448).to(torch.float8_e4m3fn)
    got = q.view(torch.float8_e4m3fn)
    # same OCP e4m3 rounding as torch (round to nearest even), allowing the last bit on ties of the f32 division
    diff = (got.float() - want.float()).abs()
    assert (diff <= want.float().abs() * 2.0 ** -3 + 2.0 ** -9).all()
    assert (got.float() == want.float()).float().mean() > 0.999
    assert relerr(_dequant(q, scale), x.float()) < 0.07


@pytest.mark.parametrize("M,N,K,act", [(256, 256, 128, 0), (300, 512, 384, 1), (5000, 1024, 1024, 2), (4096 + 77, 768, 3072, 0)])
def test_gemm_fp8_exact_on_quantised_operands(hip, M, N, K, act):
    a, w = rnd(M, K, dtype=torch.bfloat16, seed=71), rnd(N, K, dtype=torch.bfloat16, scale=K ** -0.5, seed=72)
    bias = rnd(N, seed=73)
    a8, sa = hip.quantize_rows_fp8(a)
    w8, sw = hip.quantize_rows_fp8(w)
    out = hip.gemm_fp8_bias_act(a8, sa, w8, sw, bias, act)
    assert out.shape == (M, N) and out.dtype == torch.bfloat16
    ref = _dequant(a8, sa).double() @ _dequant(w8, sw).double().T + bias.double()
    ref = [lambda x: x, torch.nn.functional.gelu, torch.nn.functional.silu][act](ref).float()
    assert relerr(out, ref) < tol(torch.bfloat16)          # the kernel: f32 accumulation of exact products
    full = a.float() @ w.float().T + bias
    full = [lambda x: x, torch.nn.functional.gelu, torch.nn.functional.silu][act](full)
    rms = ((out.float() - full).pow(2).mean() / full.pow(2).mean()).sqrt().item()
    assert rms < 0.06, rms                                  # quantisation error of per-row e4m3 against the bf16 layer


def test_gemm_fp8_layout_asymmetric(hip):
    """A = I (exact in e4m3) against an asymmetric integer W: catches a wrong operand byte order or transposed C."""
    K = N = 256
    a = torch.eye(K, device=DEV, dtype=torch.bfloat16)
    w = ((torch.arange(N, device=DEV)[:, None] * 3 + torch.arange(K, device=DEV)[None, :] * 5) % 13 - 6).to(torch.bfloat16)
    a8, sa = hip.quantize_rows_fp8(a)
    w8, sw = hip.quantize_rows_fp8(w)
    out = hip.gemm_fp8_bias_act(a8, sa, w8, sw, None, 0)
    assert relerr(out, _dequant(w8, sw).T.contiguous()) < 1e-2


def test_row_norm_fp8_side_output_equals_quantised_output(hip):
    """The LayerNorm + residual kernel's fp8 side output (the A operand of the next fp8 GEMM) is bit-for-bit what
    nova_quantize_rows_fp8 makes of the bf16 row it stores."""
    import ctypes

    rows, D = 777, 1536
    x, res = rnd(rows, D, dtype=torch.bfloat16, seed=81), rnd(rows, D, dtype=torch.bfloat16, seed=82)
    g, b = 1 + rnd(D, seed=83) * 0.1, rnd(D, seed=84) * 0.1
    plain = hip.row_norm(x, gamma=g, beta=b, res=res)
    out = torch.empty_like(x)
    q = torch.empty(rows, D, dtype=torch.uint8, device=DEV)
    sc = torch.empty(rows, dtype=torch.float32, device=DEV)
    hip.call("nova_row_norm_fp8", x.data_ptr(), out.data_ptr(), g.data_ptr(), b.data_ptr(), res.data_ptr(), q.data_ptr(), sc.data_ptr(),
             rows, D, 1e-5, hip.stream_ptr())
    assert torch.equal(out, plain)
    q2, sc2 = hip.quantize_rows_fp8(out)
    assert torch.equal(sc, sc2) and torch.equal(q, q2)


def test_gemm_fp8_qkv_rope_epilogue(hip):
    """fp8 fused QKV with the RoPE + q-scale epilogue against the same epilogue applied to the dequantised product."""
    S, L, D, heads = 2, 160, 512, 8
    hd = D // heads
    x, w = rnd(S * L, D, dtype=torch.bfloat16, seed=91), rnd(3 * D, D, dtype=torch.bfloat16, scale=D ** -0.5, seed=92)
    bias = rnd(3 * D, seed=93)
    ang = torch.rand(1, L, hd // 2, device=DEV) * 6.28
    rope = torch.stack([ang.cos(), ang.sin()], dim=-1).contiguous()
    x8, xs = hip.quantize_rows_fp8(x)
    w8, ws = hip.quantize_rows_fp8(w)
    out = torch.empty(S * L, 3 * D, dtype=torch.bfloat16, device=DEV)
    hip.call("nova_qkv_rope_fp8", x8.data_ptr(), xs.data_ptr(), w8.data_ptr(), ws.data_ptr(), bias.data_ptr(), rope.data_ptr(),
             out.data_ptr(), S, L, D, heads, 1, 0.5, hip.stream_ptr())
    ref = (_dequant(x8, xs).double() @ _dequant(w8, ws).double().T + bias.double()).view(S, L, 3, heads, hd // 2, 2)
    c, s_ = rope[0, :, None, :, 0].double(), rope[0, :, None, :, 1].double()
    rot = ref.clone()
    for t in (0, 1):  # q and k thirds: adjacent pairs rotated
        a, b = ref[:, :, t, ..., 0], ref[:, :, t, ..., 1]
        rot[:, :, t, ..., 0], rot[:, :, t, ..., 1] = a * c - b * s_, a * s_ + b * c
    rot[:, :, 0] *= 0.5  # q_scale on the q third
    assert relerr(out, rot.reshape(S * L, 3 * D).float()) < tol(torch.bfloat16)


@pytest.mark.parametrize("M,N,K", [(256, 256, 128), (700, 512, 384), (5000, 1536, 1024)])
def test_gemm_fp8_gelu_with_e4m3_output(hip, M, N, K):
    """fc1 of the fp8 stack under delayed scaling: GELU then e4m3 bytes with a static scale straight from the epilogue (4 x 4
    lane-row transpose into 16-byte stores), the running |max| recorded. Against the dequantised product: every element within
    e4m3's half-ulp (2^-4 relative, plus the subnormal step), so a misplaced byte or column would show; saturation at +-448."""
    a, w = rnd(M, K, dtype=torch.bfloat16, seed=101), rnd(N, K, dtype=torch.bfloat16, scale=K ** -0.5, seed=102)
    bias = rnd(N, seed=103)
    a8, sa = hip.quantize_rows_fp8(a)
    w8, sw = hip.quantize_rows_fp8(w)
    ref = torch.nn.functional.gelu(_dequant(a8, sa).double() @ _dequant(w8, sw).double().T + bias.double()).float()
    for scale_val in (float(ref.abs().max()) * 1.5 / 448.0, float(ref.abs().max()) * 0.25 / 448.0):  # in range / saturating
        scale = torch.tensor([scale_val], device=DEV)
        amax = torch.zeros(1, dtype=torch.int32, device=DEV)
        out8 = torch.empty(M, N, dtype=torch.uint8, device=DEV)
        hip.call("nova_gemm_fp8_gelu_q8", a8.data_ptr(), sa.data_ptr(), w8.data_ptr(), sw.data_ptr(), bias.data_ptr(), out8.data_ptr(),
                 M, N, K, scale.data_ptr(), amax.data_ptr(), hip.stream_ptr())
        got = out8.view(torch.float8_e4m3fn).float() * scale_val
        want = ref.clamp(-448 * scale_val, 448 * scale_val)
        err = (got - want).abs()
        assert bool((err <= want.abs() * 2.0 ** -4 + scale_val * 2.0 ** -9 + 1e-4).all()), float((err - want.abs() * 2.0 ** -4).max())
        seen = float(amax.view(torch.float32))
        assert abs(seen - float(ref.abs().max())) <= 1e-3 * float(ref.abs().max())
