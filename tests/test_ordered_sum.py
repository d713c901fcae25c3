"""ordered_sum_kernel (csrc/fused_common.h), the one kernel behind every ordered float32 sum of the fused training ops, held
directly through the entry points that launch it: nova_pointset_embed_sum_clouds, nova_pointset_soft_cluster_sum_clouds and
the chunk merges of nova_pointset_embed_bwd and nova_pointset_head_bwd (the two-output form).

The contract is an order of additions, so every comparison is BITWISE and no tolerance is involved: the reference is
ordered(), float32 `total = total + v` from +0 in ascending order in a NumPy loop. The inputs are normal draws each scaled by
a random power of two in 2^-20 .. 2^20, and wherever an order exists to get wrong (15 partials or more) the test first
asserts, on the CPU restatement alone, that the descending order gives other bits in at least half of the elements:
otherwise it could not see a wrong order. For the two sum_clouds entries the seed is the first one that has this property;
for the merges the partials are the backward kernel's own (read back from the workspace) and the property is asserted of
them."""
import math

import numpy as np
import pytest
import torch

CHUNK = 128  # == NOVA_EMBED_CHUNK == NOVA_HEAD_CHUNK
COUNTS = [1, 15, 16, 17, 33]  # the group of 16 loads: below it, full, its tail, a second group
ORDERED_FROM = 15  # partial counts from here on carry the order-sensitivity assertion (1 and 2 partials have one order)


def ordered(parts, descending=False):
    """parts [count, ...] float32 (NumPy): the slices added from +0 one by one, float32 throughout."""
    total = np.zeros(parts.shape[1:], dtype=np.float32)
    for k in (range(parts.shape[0] - 1, -1, -1) if descending else range(parts.shape[0])):
        total = total + parts[k]
    assert total.dtype == np.float32
    return total


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.int32)


def order_sensitivity(parts):
    """The fraction of elements whose descending sum has other bits than the ascending one."""
    return float(np.mean(bits(ordered(parts)) != bits(ordered(parts, descending=True))))


def draw(seed, *shape):
    """Normal draws, each scaled by a random power of two in 2^-20 .. 2^20 (exact in float32)."""
    gen = torch.Generator().manual_seed(seed)
    return torch.randn(*shape, generator=gen) * torch.exp2(torch.randint(-20, 21, shape, generator=gen).float())


def order_sensitive_draw(count, n):
    """draw(seed, count, n) for the first seed whose descending sum differs in at least half of the n elements."""
    for seed in range(64):
        parts = draw(seed, count, n)
        if order_sensitivity(parts.numpy()) >= 0.5:
            return parts
    raise AssertionError(f"no seed below 64 makes {count} x {n} partials order-sensitive in half of the elements")


def test_the_restatement_sees_the_order():
    """CPU: the inputs the GPU tests use are order-sensitive in at least half of the elements, for every count with an order
    to get wrong and every width; ordered() starts from +0."""
    for count in COUNTS:
        if count >= ORDERED_FROM:
            for n in (1, 3, 96, 255, 256, 257):
                assert order_sensitivity(order_sensitive_draw(count, n).numpy()) >= 0.5, (count, n)
    lone = ordered(np.full((1, 4), -0.0, dtype=np.float32))
    assert not np.signbit(lone).any()  # +0 + -0 is +0


# ---- GPU -------------------------------------------------------------------------------------------------------------------


def guarded(n, guard=64):
    """A NaN-filled buffer of guard + n + guard floats on the GPU and its middle n."""
    buf = torch.full((n + 2 * guard,), math.nan, dtype=torch.float32, device="cuda")
    return buf, buf[guard:guard + n]


def untouched(buf, lo, hi):
    """Everything of buf outside [lo, hi) is still NaN."""
    return bool(torch.isnan(buf[:lo]).all()) and bool(torch.isnan(buf[hi:]).all())


def same_bits(got, want):
    return np.array_equal(bits(got.detach().cpu().numpy()), bits(want))


SUM_ENTRIES = [
    # entry, widths n, the argument that stands for n
    ("nova_pointset_embed_sum_clouds", [1, 255, 256, 257], lambda n: n),  # the workgroup of 256: below it, full, a second one
    ("nova_pointset_soft_cluster_sum_clouds", [3, 96], lambda n: n // 3),  # K = 1 and K = 32, its limit
]


@pytest.mark.gpu
@pytest.mark.parametrize("entry,widths,arg", SUM_ENTRIES, ids=[e[0] for e in SUM_ENTRIES])
def test_sum_clouds_entries_add_in_ascending_order(hip, entry, widths, arg):
    """Both sum_clouds entries against ordered(), bitwise, for every count in COUNTS and every width; nothing written outside
    the n results; a lone -0 partial comes out as +0."""
    stream = hip.stream_ptr()
    for count in COUNTS:
        for n in widths:
            parts = order_sensitive_draw(count, n) if count >= ORDERED_FROM else draw(count, count, n)
            if count >= ORDERED_FROM:
                assert order_sensitivity(parts.numpy()) >= 0.5
            buf, out = guarded(n)
            hip.call(entry, parts.cuda().data_ptr(), out.data_ptr(), count, arg(n), stream)
            torch.cuda.synchronize()
            assert same_bits(out, ordered(parts.numpy())), (count, n)
            assert untouched(buf, 64, 64 + n), (count, n)
    for n in widths:  # a lone -0: total = +0 + v, never v alone
        buf, out = guarded(n)
        hip.call(entry, torch.full((1, n), -0.0, device="cuda").data_ptr(), out.data_ptr(), 1, arg(n), stream)
        torch.cuda.synchronize()
        assert bool((out == 0).all()) and not bool(torch.signbit(out).any()), n
        assert untouched(buf, 64, 64 + n)


def merge_case(hip, which, S, N, C, E, want, seed):
    """One call of nova_pointset_embed_bwd (which = "embed": the two outputs are gWs [S, E, C] and gcs [S, E]) or of
    nova_pointset_head_bwd ("head": gWs [S, C, E] and gbs [S, C]) on order-sensitive g, with the outputs named in `want`
    and NULL for the other. Returns (first, second, parts): the two outputs as NumPy [S, .] (None where not wanted) and the
    chunk partials the backward kernel left in the workspace, [S, chunks, per]. Asserts that nothing but the wanted outputs
    was written: both lie in one NaN-filled buffer, guards around and between them."""
    chunks = (N + CHUNK - 1) // CHUNK
    split, per = E * C, E * C + (E if which == "embed" else C)
    n1, n2 = S * split, S * (per - split)
    x = draw(seed, S, N, C if which == "embed" else E).cuda()
    g = draw(seed + 1, S, N, E if which == "embed" else C).cuda()
    W = torch.randn(E, C, generator=torch.Generator().manual_seed(seed + 2)).cuda()
    if which == "head":
        W = W.t().contiguous()
    buf = torch.full((64 + n1 + 64 + n2 + 64,), math.nan, dtype=torch.float32, device="cuda")
    first, second = buf[64:64 + n1], buf[128 + n1:128 + n1 + n2]
    ws = torch.full((S * chunks * per,), math.nan, dtype=torch.float32, device="cuda")
    p1 = first.data_ptr() if "first" in want else None
    p2 = second.data_ptr() if "second" in want else None
    if which == "embed":
        hip.call("nova_pointset_embed_bwd", x.data_ptr(), W.data_ptr(), g.data_ptr(), None, p1, p2, ws.data_ptr(), S, N, C, E, hip.stream_ptr())
    else:
        hip.call("nova_pointset_head_bwd", x.data_ptr() if p1 else None, hip.dtype_code(torch.float32), W.data_ptr(), g.data_ptr(), 0.0, None, p1, p2,
                 ws.data_ptr(), S, N, C, E, hip.stream_ptr())
    torch.cuda.synchronize()
    assert bool(torch.isnan(buf[:64]).all()) and bool(torch.isnan(buf[64 + n1:128 + n1]).all()) and bool(torch.isnan(buf[128 + n1 + n2:]).all())
    for name, t in (("first", first), ("second", second)):
        assert bool(torch.isnan(t).all()) == (name not in want), name  # the output that is NULL: nothing written where it would lie
    out = lambda name, t, width: t.cpu().numpy().reshape(S, width) if name in want else None
    return out("first", first, split), out("second", second, per - split), ws.cpu().numpy().reshape(S, chunks, per)


@pytest.mark.gpu
@pytest.mark.parametrize("which", ["embed", "head"])
@pytest.mark.parametrize("E", [5, 256])
def test_chunk_merges_add_in_ascending_order(hip, which, E):
    """The two-output form through embed_bwd (gWs, gcs) and head_bwd (gWs, gbs) at C = 3: 1, 2 and 17 chunks, 1 and 3
    clouds, the first output only, the second only and both. Every wanted output is bitwise ordered() of the partials the
    backward kernel wrote; the unwanted one is NULL and nothing is written for it; at 17 chunks the partials are
    order-sensitive in at least half of the wanted elements."""
    C = 3
    split = E * C
    for N in (CHUNK, CHUNK + 1, CHUNK * 16 + 1):
        for S in (1, 3):
            for want in (("first",), ("second",), ("first", "second")):
                for seed in range(7, 7 + 3 * 8, 3):  # the first seed whose partials are order-sensitive (gbs is 3 elements per cloud)
                    first, second, parts = merge_case(hip, which, S, N, C, E, want, seed)
                    wanted = [(got, parts[:, :, lo:hi]) for got, lo, hi in ((first, 0, split), (second, split, parts.shape[2])) if got is not None]
                    sensitive = all(order_sensitivity(mine.transpose(1, 0, 2)) >= 0.5 for _, mine in wanted)
                    if sensitive or N <= CHUNK * 16:  # 1 and 2 chunks have one order
                        break
                assert sensitive or N <= CHUNK * 16, (N, S, want)
                for got, mine in wanted:
                    assert not np.isnan(mine).any()
                    for s in range(S):
                        assert np.array_equal(bits(got[s]), bits(ordered(mine[s]))), (N, S, want, s)


@pytest.mark.gpu
@pytest.mark.parametrize("which", ["embed", "head"])
def test_a_group_depends_on_its_own_partials_alone(hip, which):
    """More than one group: cloud 2's merged gradients are the same bits whatever cloud 0 holds (S = 3 against the same
    clouds 1 and 2 behind another cloud 0), and the same as alone (S = 1)."""
    C, E, N = 3, 256, CHUNK * 16 + 1
    chunks = (N + CHUNK - 1) // CHUNK
    per = E * C + (E if which == "embed" else C)
    xw, gw = (C, E) if which == "embed" else (E, C)
    x, g = draw(11, 3, N, xw).cuda(), draw(12, 3, N, gw).cuda()
    W = torch.randn(E, C, generator=torch.Generator().manual_seed(13)).cuda()
    W = W if which == "embed" else W.t().contiguous()

    def run(x, g):
        S = x.shape[0]
        first, second = torch.full((S, E * C), math.nan, device="cuda"), torch.full((S, per - E * C), math.nan, device="cuda")
        ws = torch.full((S * chunks * per,), math.nan, device="cuda")
        if which == "embed":
            hip.call("nova_pointset_embed_bwd", x.data_ptr(), W.data_ptr(), g.data_ptr(), None, first.data_ptr(), second.data_ptr(), ws.data_ptr(),
                     S, N, C, E, hip.stream_ptr())
        else:
            hip.call("nova_pointset_head_bwd", x.data_ptr(), hip.dtype_code(torch.float32), W.data_ptr(), g.data_ptr(), 0.0, None, first.data_ptr(),
                     second.data_ptr(), ws.data_ptr(), S, N, C, E, hip.stream_ptr())
        torch.cuda.synchronize()
        return first.cpu().numpy(), second.cpu().numpy()

    base = run(x, g)
    x2, g2 = x.clone(), g.clone()
    x2[0], g2[0] = draw(14, N, xw).cuda(), draw(15, N, gw).cuda() * 1e6
    other = run(x2, g2)
    alone = run(x[2:].contiguous(), g[2:].contiguous())
    for b, o, a in zip(base, other, alone):
        assert not np.isnan(b).any()
        assert np.array_equal(bits(b[2]), bits(o[2])) and np.array_equal(bits(b[2]), bits(a[0]))
        assert np.array_equal(bits(b[1]), bits(o[1])) and not np.array_equal(bits(b[0]), bits(o[0]))
