"""Direct numerics of the calls only the generation path makes (GPU box only): nova_attn_fwd with Lq != Lk and
independent strides, nova_qkv_rope_cols, nova_modulate_rows, nova_vit_blocks_forward_kv fed chunk by chunk, and the
block-stack composites against the chain of their public parts, bit for bit (which puts the reverse tile walk of every
kernel in a composite under test: the chain always walks forward).

Every reference is float64 torch on the stored values; inputs, references and the two CPU-side self-checks (the attention
inputs tell a dropped last key; the stack bound is stable over seeds) live in tests/test_cross_length_cpu.py.
Bounds are the project's own (tests/test_gpu_kernels.py): tol(dtype) globally, 2.5 x tol(dtype) row-wise.
"""
import pytest
import torch

import test_cross_length_cpu as C
from test_cross_length_cpu import DTYPES, row_err, tol

pytestmark = pytest.mark.gpu

DEV = "cuda"
HALF = [torch.bfloat16, torch.float16]
SENTINEL = -123.25  # exact in all three storage types


def relerr(got, ref):
    got, ref = got.double(), ref.double()
    return ((got - ref).abs().max() / ref.abs().max().clamp_min(1e-12)).item()


def bits(t):
    return t.contiguous().view(torch.int32 if t.dtype == torch.float32 else torch.int16)


def same_bits(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and torch.equal(bits(a), bits(b))


def randn(*shape, seed, scale=1.0):
    return torch.randn(*shape, generator=torch.Generator().manual_seed(seed)) * scale


@pytest.fixture()
def force_tile(hip):
    def _force(tile):
        hip.call("nova_debug_force_gemm_tile", tile)
    yield _force
    hip.call("nova_debug_force_gemm_tile", 0)


# ---------------------------------------------------------------------------------------------
# 1. nova_attn_fwd, Lq != Lk, q / kv / o each with its own row stride
# ---------------------------------------------------------------------------------------------
# (dtype, head_dim, structure): every 16-bit head_dim 64 structure of nova_debug_set_attn_variant, the default elsewhere
ATTN_KERNELS = [(dt, hd, -1) for dt in DTYPES for hd in (64, 96)] + [(dt, 64, av) for dt in HALF for av in range(6)]


@pytest.mark.parametrize("dtype,hd,variant", ATTN_KERNELS)
@pytest.mark.parametrize("Lq,Lk", C.ATTN_PAIRS)
def test_attention_cross_length(hip, dtype, hd, variant, Lq, Lk):
    """q in an [S*Lq, D + 8] buffer, k | v interleaved in [S*Lk, 2D] (the cache layout), o in an [S*Lq + 2, D + 16] buffer
    whose padding must stay untouched; scale head_dim ** -0.5 and 0.2 (the scale-at-load path of the 16-bit kernels).
    The last key carries most of one row's weight per (sequence, head) (asserted: the reference over Lk - 1 keys is
    outside the bound), so one key too few or too many in the ragged tail fails."""
    S, H = C.ATTN_S, C.ATTN_HEADS
    D = H * hd
    q, k, v = C.attn_case(dtype, hd, Lq, Lk)
    qbuf = randn(S * Lq, D + 8, seed=3).to(dtype)
    qbuf[:, :D] = q.reshape(S * Lq, D)
    kv = torch.cat([k.reshape(S * Lk, D), v.reshape(S * Lk, D)], 1).contiguous()
    qd, kvd = qbuf.to(DEV), kv.to(DEV)
    sent = torch.full((S * Lq + 2, D + 16), SENTINEL, dtype=dtype)
    try:
        hip.call("nova_debug_set_attn_variant", variant)
        for scale in C.ATTN_SCALES:
            sc = C.attn_scale(scale, hd)
            ref = C.attn_ref(q, k, v, sc)
            teeth = C.attn_teeth(q, k, v, sc)
            assert teeth.min().item() > 2.5 * tol(dtype), ("the inputs cannot tell a dropped last key", teeth.tolist())
            obuf = sent.to(DEV)
            hip.attn_fwd(qd, kvd, kvd, obuf, S, H, Lq, Lk, hd, D + 8, 2 * D, D + 16, scale=sc, v_off=D)
            obuf = obuf.cpu()
            assert same_bits(obuf[:, D:], sent[:, D:]) and same_bits(obuf[S * Lq:], sent[S * Lq:]), "padding of o was written"
            out = obuf[:S * Lq, :D]
            re, rw = relerr(out, ref), row_err(out, ref)
            print(f"attn {dtype} hd={hd} variant={variant} ({Lq},{Lk}) scale={sc:.4f}: relerr {re:.3e} row {rw.max().item():.3e}")
            assert re < tol(dtype), (scale, re)
            assert rw.max().item() < 2.5 * tol(dtype), (scale, "row", rw.argmax().item(), rw.max().item())
    finally:
        hip.call("nova_debug_set_attn_variant", -1)


# ---------------------------------------------------------------------------------------------
# 2. nova_qkv_rope_cols
# ---------------------------------------------------------------------------------------------
def rope_cols_ref(x, w, b, rope, S, L, heads, rope_cols):
    """float64 x W^T + b with columns [0, rope_cols) rotated by rope[(m // L) % nb, m % L]."""
    ref = x.double() @ w.double().T + b.double()
    hd = rope.shape[2] * 2
    rot = C.rotate(ref[:, :rope_cols].reshape(S, L, rope_cols // hd, hd), rope).reshape(S * L, rope_cols)
    return torch.cat([rot, ref[:, rope_cols:]], 1)


def check_rope_cols(out, ref, rope_cols, dtype):
    out = out.cpu()
    assert relerr(out, ref) < tol(dtype)
    for name, sl in (("rotated", slice(0, rope_cols)), ("unrotated", slice(rope_cols, ref.shape[1]))):
        if sl.start < sl.stop:
            rw = row_err(out[:, sl], ref[:, sl])
            assert rw.max().item() < 2.5 * tol(dtype), (name, "row", rw.argmax().item(), rw.max().item())


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("D,heads", [(128, 2), (384, 4)])
@pytest.mark.parametrize("use", ["kv_all_rows", "q_gathered_rows"])
def test_qkv_rope_cols(hip, dtype, D, heads, use):
    """The two calls of the last encoder block: K | V over all S*L rows (N = 2D, only the K half rotated) and Q over the
    S*n gathered rows (N = D, L = n = 5; S = 3 so that M is no multiple of L * rope_batch). Two batch entries with
    unrelated tables: a wrong (m // L) % rope_batch or m % L shows in the rotated columns, a rotation leaking past
    rope_cols in the others. Without a table (rope_cols = 0) the call is nova_gemm_bias_act, bit for bit."""
    hd = D // heads
    S, L, N = (4, 37, 2 * D) if use == "kv_all_rows" else (3, 5, D)
    M = S * L
    x, w = randn(M, D, seed=51).to(dtype), randn(N, D, seed=52, scale=D ** -0.5).to(dtype)
    b, rope = randn(N, seed=53), C.make_rope(2, L, hd, torch.Generator().manual_seed(54))
    xd, wd, bd = x.to(DEV), w.to(DEV), b.to(DEV)
    out = hip.qkv_rope_cols(xd, wd, bd, rope.to(DEV), L, hd, D)
    check_rope_cols(out, rope_cols_ref(x, w, b, rope, S, L, heads, D), D, dtype)
    plain = hip.qkv_rope_cols(xd, wd, bd, None, L, hd, 0)
    assert same_bits(plain, hip.gemm_bias_act(xd, wd, bd))


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("D,heads", [(256, 4), (768, 8)])
@pytest.mark.parametrize("form", [256, 257, 258])
def test_qkv_rope_cols_large_m_tiles_bitwise(hip, force_tile, dtype, D, heads, form):
    """M = 5 * 821 = 4105 rows (where the 256 x 256 structure takes over), head_dim 64 and 96: the 128 tile and every form
    of the 256 tile (256 the shipped choice, 257 one tile per workgroup, 258 the persistent prologue form) give the same
    bits, and those are right. Head width 96 is where the persistent forms load a second set of table rows."""
    hd = D // heads
    S, L, N = 5, 821, 2 * D
    x, w = randn(S * L, D, seed=61).to(dtype), randn(N, D, seed=62, scale=D ** -0.5).to(dtype)
    b, rope = randn(N, seed=63), C.make_rope(2, L, hd, torch.Generator().manual_seed(64))
    xd, wd, bd, rd = x.to(DEV), w.to(DEV), b.to(DEV), rope.to(DEV)
    force_tile(128)
    o128 = hip.qkv_rope_cols(xd, wd, bd, rd, L, hd, D)
    force_tile(form)
    o256 = hip.qkv_rope_cols(xd, wd, bd, rd, L, hd, D)
    assert same_bits(o128, o256)
    check_rope_cols(o256, rope_cols_ref(x, w, b, rope, S, L, heads, D), D, dtype)


@pytest.mark.parametrize("dtype", DTYPES)
def test_qkv_rope_cols_short_sequence_256_tile_bitwise(hip, force_tile, dtype):
    """A rotated launch with L = 5 < 16 sent to the 256 tile takes its one-tile-per-workgroup kernel (the persistent
    epilogues step through 16-row blocks that cross at most one sequence boundary). M = 61 * 5 = 305: two row tiles, the
    second ragged, M no multiple of L * rope_batch. Same bits as the 128 tile, and those are right."""
    S, L, D, heads = 61, 5, 256, 4
    hd, N = D // heads, 2 * D
    x, w = randn(S * L, D, seed=65).to(dtype), randn(N, D, seed=66, scale=D ** -0.5).to(dtype)
    b, rope = randn(N, seed=67), C.make_rope(2, L, hd, torch.Generator().manual_seed(68))
    xd, wd, bd, rd = x.to(DEV), w.to(DEV), b.to(DEV), rope.to(DEV)
    force_tile(128)
    o128 = hip.qkv_rope_cols(xd, wd, bd, rd, L, hd, D)
    force_tile(256)
    o256 = hip.qkv_rope_cols(xd, wd, bd, rd, L, hd, D)
    assert same_bits(o128, o256)
    check_rope_cols(o256, rope_cols_ref(x, w, b, rope, S, L, heads, D), D, dtype)


# ---------------------------------------------------------------------------------------------
# 3. nova_modulate_rows
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("rows", [1, 37, 4099, 6001])
@pytest.mark.parametrize("D", [128, 768, 1536])
def test_modulate_rows(hip, dtype, rows, D):
    """x * (1 + mod[:, :D]) + mod[:, D:] against float64, and in place == out of place. (6001 x 1536 elements are more
    than the launch's 8192 x 256 x 4: the grid-stride loop takes a second round.)"""
    x = randn(rows, D, seed=71).to(dtype).to(DEV)
    mod = randn(rows, 2 * D, seed=72, scale=0.5).to(dtype).to(DEV)
    out = hip.modulate_rows(x, mod)
    ref = x.double() * (1 + mod[:, :D].double()) + mod[:, D:].double()
    assert out.shape == x.shape and out.dtype == dtype
    assert relerr(out, ref) < tol(dtype)
    inplace = x.clone()
    hip.modulate_rows(inplace, mod, out=inplace)
    assert same_bits(inplace, out)


# ---------------------------------------------------------------------------------------------
# 4. nova_vit_blocks_forward_kv, chunk by chunk
# ---------------------------------------------------------------------------------------------
def pack_blocks(hip, blocks, dtype):
    """nova_vit_block[] of CPU parameter dicts (GEMM weights in dtype, the rest f32); returns (array, device tensors)."""
    arr, dev = (hip.VitBlock * len(blocks))(), []
    for i, b in enumerate(blocks):
        d = {k: b[k].to(dtype if k in ("qkv_w", "proj_w", "fc1_w", "fc2_w") else torch.float32).to(DEV).contiguous()
             for k in C.BLOCK_KEYS}
        dev.append(d)
        arr[i] = hip.VitBlock(*[d[k].data_ptr() for k in C.BLOCK_KEYS])
    return arr, dev


class Workspaces:
    def __init__(self, rows, D, hidden, dtype):
        e = lambda n: torch.empty(rows, n, dtype=dtype, device=DEV)
        self.qkv, self.a, self.b, self.h = e(3 * D), e(D), e(D), e(hidden)


def run_kv_chunks(hip, case, dtype, arr, chunks, cache):
    """Feeds case["x"] in `chunks` through nova_vit_blocks_forward_kv; returns the output rows of every chunk (CPU)."""
    S, D = case["x"].shape[0], case["D"]
    ws = Workspaces(S * max(chunks), D, case["hidden"], dtype)
    outs, pos = [], 0
    for L in chunks:
        x = case["x"][:, pos:pos + L].reshape(S * L, D).to(dtype).to(DEV).contiguous()
        rope = case["rope"][:, pos:pos + L].contiguous().to(DEV)
        hip.vit_blocks_forward_kv(arr, x, S, L, case["heads"], case["hidden"], rope, cache, cache.shape[2], pos,
                                  ws.qkv, ws.a, ws.b, ws.h)
        outs.append(x.cpu())
        pos += L
    return outs


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("D,heads", C.KV_SHAPES)
def test_kv_stack_chunk_by_chunk(hip, dtype, D, heads):
    """Two blocks, S = 2, chunks of 37, 64 and 29 rows into a cache of 160 rows per sequence (kv_ss = 160 * 2D > Lk * 2D),
    against the float64 stack in which chunk c sees the keys of chunks <= c.
    Output rows: row-wise within 3 x the error of the torch emulation that rounds to the storage type at every launch
    boundary (floor 2e-5). That emulation's measured row-wise error, seed 0 (the seed used here):
        float32   D 128: 1.70e-07   D 384: 1.45e-07
        bfloat16  D 128: 1.06e-02   D 384: 8.62e-03
        float16   D 128: 1.44e-03   D 384: 1.30e-03
    Cache rows [0, 130): the reference's rotated k | v within 2.5 x tol row-wise; rows [130, 160) keep the sentinel; a call
    past the capacity is refused and writes nothing; block 0's cache rows do not depend on how the rows were split."""
    case = C.kv_case(D, heads, seed=0)
    S, total, cap = C.KV_S, sum(C.KV_CHUNKS), C.KV_CAP
    ref, ref_caches, emu_err = C.kv_emulation_error(case, dtype)
    bound = C.kv_bound(emu_err)
    arr, keep = pack_blocks(hip, case["blocks"], dtype)
    cache = torch.full((C.KV_BLOCKS, S, cap, 2 * D), SENTINEL, dtype=dtype, device=DEV)
    outs = run_kv_chunks(hip, case, dtype, arr, C.KV_CHUNKS, cache)
    for c, (o, r) in enumerate(zip(outs, ref)):
        rw = row_err(o, r.reshape(-1, D))
        print(f"kv stack {dtype} D={D} chunk {c}: row-wise {rw.max().item():.3e}, bound {bound:.3e} (emulation {emu_err:.3e})")
        assert rw.max().item() < bound, ("chunk", c, "row", rw.argmax().item(), rw.max().item(), "bound", bound, "emulation", emu_err)
    got = cache.cpu()
    for i in range(C.KV_BLOCKS):
        rw = row_err(got[i, :, :total].reshape(S * total, 2 * D), ref_caches[i].reshape(S * total, 2 * D))
        assert rw.max().item() < 2.5 * tol(dtype), ("cache of block", i, "row", rw.argmax().item(), rw.max().item())
    assert same_bits(got[:, :, total:], torch.full_like(got[:, :, total:], SENTINEL)), "free cache rows were written"
    # out of capacity: refused, nothing written
    L = cap - total + 1
    ws = Workspaces(S * L, D, case["hidden"], dtype)
    x = torch.zeros(S * L, D, dtype=dtype, device=DEV)
    rope = C.make_rope(C.KV_NB, L, D // heads, torch.Generator().manual_seed(1)).to(DEV)
    with pytest.raises(hip.NovaHipError):
        hip.vit_blocks_forward_kv(arr, x, S, L, heads, case["hidden"], rope, cache, cap, total, ws.qkv, ws.a, ws.b, ws.h)
    assert same_bits(cache.cpu(), got)
    # one call with all 130 rows: block 0's k | v do not depend on attention, so its cache rows are the same bits
    cache1 = torch.full_like(cache, SENTINEL)
    run_kv_chunks(hip, case, dtype, arr, (total,), cache1)
    assert same_bits(cache1[0, :, :total], cache[0, :, :total])


# ---------------------------------------------------------------------------------------------
# 5. a composite equals the chain of its public parts, bit for bit (float32: nothing is folded into q)
# ---------------------------------------------------------------------------------------------
def chain_block(hip, b, x, S, L, heads, rope, ws, cache=None, cache_len=0):
    """One block through the public entry points, in the composite's launch order, on x [S*L, D] in place.
    cache [cap, 2D] (S = 1): a torch copy of the k | v columns stands in for the append kernel."""
    D = x.shape[1]
    hip.qkv_rope(x, b["qkv_w"], b["qkv_b"], rope, S, L, heads, out=ws.qkv)
    if cache is None:
        hip.attn_fwd_packed(ws.qkv, S, L, heads, out=ws.a)
    else:
        cache[cache_len:cache_len + L] = ws.qkv[:, D:]
        hip.attn_fwd(ws.qkv, cache, cache, ws.a, 1, heads, L, cache_len + L, D // heads, 3 * D, 2 * D, D, v_off=D)
    hip.gemm_bias_act(ws.a, b["proj_w"], b["proj_b"], hip.ACT_NONE, out=ws.b)
    hip.row_norm(ws.b, out=x, gamma=b["norm1_w"], beta=b["norm1_b"], res=x, eps=1e-5)
    hip.gemm_bias_act(x, b["fc1_w"], b["fc1_b"], hip.ACT_GELU_ERF, out=ws.h)
    hip.gemm_bias_act(ws.h, b["fc2_w"], b["fc2_b"], hip.ACT_NONE, out=ws.b)
    hip.row_norm(ws.b, out=x, gamma=b["norm2_w"], beta=b["norm2_b"], res=x, eps=1e-5)


def stack_inputs(hip, S, L, D, heads, nblocks, seed):
    g = torch.Generator().manual_seed(seed)
    arr, dev = pack_blocks(hip, C.make_blocks(nblocks, D, 4 * D, g), torch.float32)
    x = torch.randn(S * L, D, generator=g).to(DEV)
    rope = C.make_rope(2, L, D // heads, g).to(DEV)
    return arr, dev, x, rope


def check_stack_equals_chain(hip, S, L, D, heads):
    nblocks, hidden = 3, 4 * D
    arr, dev, x, rope = stack_inputs(hip, S, L, D, heads, nblocks, seed=81)
    ws = Workspaces(S * L, D, hidden, torch.float32)
    xc = x.clone()
    hip.call("nova_vit_blocks_forward", arr, nblocks, hip.ptr(xc), S, L, D, heads, hidden, hip.ptr(rope), rope.shape[0],
             hip.ptr(ws.qkv), hip.ptr(ws.a), hip.ptr(ws.b), hip.ptr(ws.h), hip.F32, hip.stream_ptr())
    ws2 = Workspaces(S * L, D, hidden, torch.float32)
    xs = x.clone()
    for i, b in enumerate(dev):
        chain_block(hip, b, xs, S, L, heads, rope, ws2)
        if i == 0:  # the stack moves x at all (a no-op on both sides would be "equal" too)
            assert not torch.equal(xs, x)
    assert torch.isfinite(xc).all()
    diff = (xc != xs).any(1).nonzero().flatten()
    assert torch.equal(xc, xs), (f"{diff.numel()} rows differ, first {diff[:8].tolist()}", (xc - xs).abs().max().item())


def test_block_stack_equals_chain_of_parts(hip):
    """nova_vit_blocks_forward walks every second launch's tiles back to front; three blocks of seven launches put every
    kernel on both directions. The walk is a permutation of block ids, so the result is that of the forward-walking
    public calls, bit for bit. 3 x 171 rows: several row tiles, the last one ragged."""
    check_stack_equals_chain(hip, 3, 171, 128, 2)


@pytest.mark.parametrize("tile", [0, 128, 256, 258])
def test_block_stack_equals_chain_of_parts_large(hip, force_tile, tile):
    """2 x 2100 = 4200 rows at D = 256: with the 256 tile forced (256: persistent, 258: its prologue form) the persistent
    GEMM's reversed tile list is what the composite runs."""
    force_tile(tile)
    check_stack_equals_chain(hip, 2, 2100, 256, 4)


def test_kv_block_stack_equals_chain_of_parts(hip):
    """The KV-cached composite, two chunks at S = 1 (where the public attention's key stride is the cache's): x and the
    whole cache, free rows included, equal the chain's."""
    S, D, heads, nblocks, cap = 1, 128, 2, 3, 160
    chunks = (37, 64)
    hidden = 4 * D
    arr, dev, x, rope = stack_inputs(hip, S, sum(chunks), D, heads, nblocks, seed=91)
    cache_c = torch.full((nblocks, S, cap, 2 * D), SENTINEL, device=DEV)
    cache_s = cache_c.clone()
    ws, ws2 = Workspaces(max(chunks), D, hidden, torch.float32), Workspaces(max(chunks), D, hidden, torch.float32)
    pos = 0
    for L in chunks:
        xc = x[pos:pos + L].clone()
        xs = xc.clone()
        tab = rope[:, pos:pos + L].contiguous()
        hip.vit_blocks_forward_kv(arr, xc, S, L, heads, hidden, tab, cache_c, cap, pos, ws.qkv, ws.a, ws.b, ws.h)
        for i, b in enumerate(dev):
            # the chain's workspaces hold exactly L rows, as the composite reads them
            w = Workspaces.__new__(Workspaces)
            w.qkv, w.a, w.b, w.h = ws2.qkv[:L], ws2.a[:L], ws2.b[:L], ws2.h[:L]
            chain_block(hip, b, xs, S, L, heads, tab, w, cache=cache_s[i, 0], cache_len=pos)
        assert torch.equal(xc, xs), ("chunk at", pos, (xc - xs).abs().max().item())
        pos += L
    assert torch.equal(cache_c, cache_s)
    assert not torch.equal(cache_c[:, :, :pos], torch.full_like(cache_c[:, :, :pos], SENTINEL))
