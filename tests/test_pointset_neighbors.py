"""kNN neighbourhood feature aggregation (nova_pointcloud_amd/neighbors.py on csrc/neighbor.hip): a float32 restatement of the
definition in plain torch, checked on hand cases and against float64 autograd of the reference's gather form, the argument
checks of the Python layer and of the C ABI (CPU); the kernels against that restatement, bit for bit (GPU).

The definition restated here (include/nova_hip.h, nova_pointset_neighbor_aggregate), every operation one float32 rounding:
    forward   term_t = f[idx_t] (mean) or w_t * f[idx_t] (weighted), +0 for an index outside 0 .. M-1; acc = term_0, then
              acc + term_t for t = 1 .. k-1; out = acc / k (mean) or acc (weighted)
    inverse   the stable sort of the in-range edges e = i k + t by target (numpy's stable argsort), as offsets and edges
    gf        per target, over its edges in increasing e: term = w_e * g[e // k] or g[e // k] / k; acc = the first term,
              then acc + term; +0 for a target no edge names
    gw        sum_c g[i, c] * f[idx_t, c] in ONE fixed shape on the GPU; any order satisfies the float64 bound used here

Shapes: the boundaries of the kernels as built (NB_* of csrc/neighbor.hip, see test_header_constants), not the workload.
  channels  one wave walks a row in chunks of 64 lanes x V floats, V = 4 (16-byte loads) when C % 4 == 0, else V = 1:
            C = 1 | 3 (one partial scalar chunk), 4 (one lane of the vector form), 63 | 65 | 255 | 257 (scalar: under one
            chunk, 2, 4 and 5 chunks, the last partial), 64 | 256 (vector: a quarter of a chunk, exactly one), 260 (vector, a
            second chunk with one lane), 768 (vector, three chunks: the workload's width)
  k         1 (no addition), 2, 8, 31, 32 (NOVA_KNN_MAX_K; a row's indices live one per lane)
  N, M      1 | 63 | 64 | 65 | 257 with N != M: 4 rows per workgroup of the row kernels; NB_Q = 64 targets per workgroup of the
            inverse walk (M = 257: five workgroups, scan chunks of 2), whose four waves take a quarter each of the N k edges,
            rounded up to a multiple of 4, NB_TILE / 4 = 1024 indices a turn: N k = 1 (one quarter, three empty), 126 (32, 32, 32,
            30), 2056 and 2080 (one turn), 8224 (quarters of 2056: three turns, the last of 8); the hub has in-degree
            N = 257 > 64, five batches of the gf kernel's edge walk
  S         cycles 1 .. 5 over the cases."""
import ctypes
import os
import re
import types

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
U = 2.0 ** -24
# (C, k, N, M)
CASES = [(1, 1, 1, 1), (3, 2, 63, 64), (4, 8, 64, 63), (63, 31, 65, 257), (64, 32, 257, 65), (65, 8, 257, 257), (255, 2, 64, 65),
         (256, 1, 65, 1), (257, 8, 63, 257), (260, 2, 63, 64), (768, 8, 257, 64), (768, 32, 65, 63), (4, 31, 1, 257), (1, 32, 257, 64)]
SHAPES = [(1 + n % 5,) + case for n, case in enumerate(CASES)]  # (S, C, k, N, M)
PATTERNS = ("knn", "random", "hub", "out_of_range")


# --------------------------------------------------------------------------------------------- restatement
def same_bits(a, b):
    return a.shape == b.shape and torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


def ref_forward(f, idx, w=None):
    """out [S, N, C] float32 of the definition: f [S, M, C] float32, idx [S, N, k] integer, w [S, N, k] float32 or None."""
    S, M, C = f.shape
    N, k = idx.shape[1:]
    idx = idx.long()
    valid = (idx >= 0) & (idx < M)
    safe = idx.clamp(0, M - 1)
    zero = torch.zeros(S, N, C, dtype=torch.float32)
    acc = None
    for t in range(k):
        term = torch.gather(f, 1, safe[:, :, t, None].expand(S, N, C))
        if w is not None:
            term = w[:, :, t, None] * term
        term = torch.where(valid[:, :, t, None], term, zero)
        acc = term if acc is None else acc + term
    return acc if w is not None else acc / torch.full_like(acc, float(k))  # an elementwise IEEE division


def ref_inverse(idx, M):
    """(offsets int32 [S, M + 1], edges: per cloud an int64 array of the in-range edge ids grouped by target)."""
    S, N, k = idx.shape
    offsets, edges = np.zeros((S, M + 1), dtype=np.int32), []
    for s in range(S):
        tgt = idx[s].reshape(-1).numpy().astype(np.int64)
        ids = np.nonzero((tgt >= 0) & (tgt < M))[0]
        edges.append(ids[np.argsort(tgt[ids], kind="stable")])
        offsets[s, 1:] = np.cumsum(np.bincount(tgt[ids], minlength=M))
    return torch.from_numpy(offsets), edges


def ref_gf(g, idx, w, M):
    """gf [S, M, C] float32 of the definition, stepping the rank r within every target's segment."""
    S, N, C = g.shape
    k = idx.shape[2]
    offsets, edges = ref_inverse(idx, M)
    gf = torch.zeros(S, M, C, dtype=torch.float32)
    kf = torch.tensor(float(k), dtype=torch.float32)
    for s in range(S):
        off = offsets[s].long()
        deg = off[1:] - off[:-1]
        ed = torch.from_numpy(edges[s])
        wflat = w[s].reshape(-1) if w is not None else None
        for r in range(int(deg.max()) if M else 0):
            js = torch.nonzero(deg > r)[:, 0]
            e = ed[off[js] + r]
            rows = g[s, e // k]
            term = wflat[e][:, None] * rows if w is not None else rows / kf.expand_as(rows)
            gf[s, js] = term if r == 0 else gf[s, js] + term
    return gf


def gw_float64(f, idx, g):
    """(gw in float64 from the float32 inputs, sum_c |g_c f_c|), both [S, N, k]; 0 for an out-of-range index."""
    S, M, C = f.shape
    N, k = idx.shape[1:]
    idx = idx.long()
    valid = (idx >= 0) & (idx < M)
    safe = idx.clamp(0, M - 1)
    val, mag = torch.zeros(S, N, k, dtype=torch.float64), torch.zeros(S, N, k, dtype=torch.float64)
    for t in range(k):
        prod = g.double() * torch.gather(f.double(), 1, safe[:, :, t, None].expand(S, N, C))
        val[:, :, t], mag[:, :, t] = prod.sum(-1), prod.abs().sum(-1)
    return val * valid, mag * valid


def gw_bound(mag, C):
    """The bound of ANY summation order over C rounded products: (C + 1) u / (1 - (C + 1) u) * sum_c |g_c f_c|."""
    return (C + 1) * U / (1 - (C + 1) * U) * mag


def ref_knn(x, y, k):
    """The k nearest targets by the exact-difference float32 d2, ties to the lowest index (nova_pointset_knn); CPU."""
    e = x[:, :, None, :] - y[:, None, :, :]
    d2 = torch.addcmul(torch.addcmul(e[..., 0] * e[..., 0], e[..., 1], e[..., 1]), e[..., 2], e[..., 2])
    return torch.argsort(d2, dim=-1, stable=True)[..., :k]


def rand(*shape, seed):
    return torch.randn(*shape, generator=torch.Generator().manual_seed(seed))


# --------------------------------------------------------------------------------------------- CPU: hand cases
def test_restatement_k1_is_the_gather():
    f = rand(2, 7, 5, seed=1)
    idx = torch.randint(0, 7, (2, 9, 1), generator=torch.Generator().manual_seed(2))
    want = torch.gather(f, 1, idx.expand(2, 9, 5))
    assert same_bits(ref_forward(f, idx), want)  # x / 1 == x
    w = torch.ones(2, 9, 1)
    assert same_bits(ref_forward(f, idx, w), want)
    g = rand(2, 9, 5, seed=3)
    gf = ref_gf(g, idx, None, 7)
    dense = torch.zeros(2, 7, 5, dtype=torch.float64)
    dense.index_put_((torch.arange(2)[:, None].expand(2, 9), idx[:, :, 0]), g.double(), accumulate=True)
    assert torch.allclose(gf.double(), dense, rtol=0, atol=10 * U * 9 * float(g.abs().max()))  # at most 9 edges per target


def test_restatement_hand_cases():
    f = torch.tensor([[[1.0, 2.0], [10.0, 20.0]]])
    # a duplicate index in a row
    assert ref_forward(f, torch.tensor([[[1, 1]]])).tolist() == [[[10.0, 20.0]]]
    # an out-of-range index adds +0 and still counts in the divisor, on either side and in either position
    for bad in (-1, 2, 2 ** 31 - 1, -2 ** 31):
        assert ref_forward(f, torch.tensor([[[0, bad]]])).tolist() == [[[0.5, 1.0]]]
        assert ref_forward(f, torch.tensor([[[bad, 1]]])).tolist() == [[[5.0, 10.0]]]
        assert ref_forward(f, torch.tensor([[[bad, 1]]]), torch.tensor([[[3.0, 0.5]]])).tolist() == [[[5.0, 10.0]]]
    assert same_bits(ref_forward(-f, torch.tensor([[[5, 5]]])), torch.zeros(1, 1, 2))  # +0, not -0
    # weights with exactly representable values: the closed form
    out = ref_forward(f, torch.tensor([[[0, 1], [1, 0]]]), torch.tensor([[[0.5, 0.25], [2.0, -4.0]]]))
    assert out.tolist() == [[[0.5 + 2.5, 1.0 + 5.0], [20.0 - 4.0, 40.0 - 8.0]]]
    # the inverse list: stable by target, out-of-range edges left out
    idx = torch.tensor([[[1, 0], [1, 7], [0, 1]]])  # edges 0 .. 5
    offsets, edges = ref_inverse(idx, 3)
    assert offsets.tolist() == [[0, 2, 5, 5]] and edges[0].tolist() == [1, 4, 0, 2, 5]
    # gf: a target with no edge gets exactly +0; the others the ordered sum
    g = torch.tensor([[[1.0, -1.0], [2.0, -2.0], [4.0, -4.0]]])
    gf = ref_gf(g, idx, None, 3)
    assert gf.tolist() == [[[0.5 + 2.0, -0.5 - 2.0], [0.5 + 1.0 + 2.0, -0.5 - 1.0 - 2.0], [0.0, 0.0]]]
    assert same_bits(gf[:, 2], torch.zeros(1, 2))
    w = torch.tensor([[[0.5, 0.25], [2.0, 9.0], [-1.0, 4.0]]])
    assert ref_gf(g, idx, w, 3).tolist() == [[[0.25 - 4.0, -0.25 + 4.0], [0.5 + 4.0 + 16.0, -0.5 - 4.0 - 16.0], [0.0, 0.0]]]


def test_restatement_hub():
    """Coincident points under the lowest-index tie rule: every query names the targets 0 .. k-1, in-degree N."""
    N, k, C = 5, 3, 2
    pts = torch.zeros(1, N, 3)
    idx = ref_knn(pts, pts, k)
    assert idx.tolist() == [[[0, 1, 2]] * N]
    offsets, edges = ref_inverse(idx, N)
    assert offsets.tolist() == [[0, 5, 10, 15, 15, 15]] and edges[0].tolist() == [0, 3, 6, 9, 12, 1, 4, 7, 10, 13, 2, 5, 8, 11, 14]
    g = torch.arange(1.0, N * C + 1).view(1, N, C) * 3  # multiples of 3: g / 3 and every partial sum are exact
    gf = ref_gf(g, idx, None, N)
    total = (g / 3).sum(1)
    assert gf[0, :k].tolist() == [total[0].tolist()] * k and same_bits(gf[0, k:], torch.zeros(N - k, C))


@pytest.mark.parametrize("weighted", [False, True])
def test_restatement_against_float64_autograd(weighted):
    """gf and gw of the restatement against float64 autograd of the gather form. Bounds: gf a sum of deg_j terms W g, each one
    rounding, deg_j - 1 additions: (deg_j + 1) u sum |W g|; gw (float32 torch sum here): the any-order bound."""
    S, N, M, k, C = 2, 33, 17, 5, 11
    f, g, w = rand(S, M, C, seed=4), rand(S, N, C, seed=5), rand(S, N, k, seed=6) if weighted else None
    idx = torch.randint(0, M, (S, N, k), generator=torch.Generator().manual_seed(7))
    f64 = f.double().requires_grad_(True)
    w64 = w.double().requires_grad_(True) if weighted else None
    nf = f64[torch.arange(S)[:, None, None], idx]  # [S, N, k, C]
    out64 = (w64[..., None] * nf).sum(2) if weighted else nf.mean(2)
    out64.backward(g.double())
    out = ref_forward(f, idx, w)
    Wabs = w.abs().double() if weighted else torch.full((S, N, k), 1.0 / k, dtype=torch.float64)
    fabs = f.abs().double()[torch.arange(S)[:, None, None], idx]
    assert bool(((out.double() - out64.detach()).abs() <= (k + 1) * U * (Wabs[..., None] * fabs).sum(2)).all())
    mag = torch.zeros(S, M, C, dtype=torch.float64)
    deg = torch.zeros(S, M, dtype=torch.float64)
    sidx = torch.arange(S)[:, None, None].expand(S, N, k)
    mag.index_put_((sidx, idx), Wabs[..., None] * g.abs().double()[:, :, None, :], accumulate=True)
    deg.index_put_((sidx, idx), torch.ones(S, N, k, dtype=torch.float64), accumulate=True)
    gf = ref_gf(g, idx, w, M)
    assert bool(((gf.double() - f64.grad).abs() <= (deg[..., None] + 1) * U * mag).all())
    if weighted:
        val, gmag = gw_float64(f, idx, g)
        assert torch.allclose(val, w64.grad, rtol=1e-12, atol=1e-12)
        gw32 = (g[:, :, None, :] * f[torch.arange(S)[:, None, None], idx]).sum(-1)
        assert bool(((gw32.double() - val).abs() <= gw_bound(gmag, C)).all())


def test_edge_features_restated_against_the_reference_intent():
    """features - mean of the k nearest neighbours' features (the comment of extract_edge_features), the point itself among
    them, at N = 5, C = 4: the reference's cdist + topk in float64 against the restatement on ref_knn's indices."""
    S, N, C, k = 2, 5, 4, 3
    pts, f = rand(S, N, 3, seed=8), rand(S, N, C, seed=9)
    _, nearest = torch.topk(torch.cdist(pts.double(), pts.double()), k=min(k, N), largest=False)
    idx = ref_knn(pts, pts, k)
    assert torch.equal(nearest.sort(-1).values, idx.sort(-1).values) and torch.equal(idx[:, :, 0], torch.arange(N).expand(S, N))
    nf = f.double()[torch.arange(S)[:, None, None], nearest]
    want = f.double() - nf.mean(2)
    got = f - ref_forward(f, idx)
    bound = (k + 1) * U * (f.abs().double() + nf.abs().mean(2))
    assert bool(((got.double() - want).abs() <= bound).all())


# --------------------------------------------------------------------------------------------- CPU: arguments, ABI, constants
def test_python_argument_errors():
    from nova_pointcloud_amd import hip, metrics, neighbors

    f, idx, w = torch.zeros(2, 6, 4), torch.zeros(2, 5, 3, dtype=torch.int64), torch.zeros(2, 5, 3)
    agg = neighbors.neighbor_aggregate
    bad = [((None, idx), "features: expected a tensor"), ((f, [0]), "idx: expected a tensor"), ((f, idx, 1.0), "weights: expected a tensor"),
           ((f.long(), idx), "features: expected a floating"), ((f, idx.float()), "idx: expected int64 or int32"),
           ((f, idx.short()), "idx: expected int64 or int32"), ((f, idx, w.long()), "weights: expected a floating"),
           ((f[0], idx), r"features: expected \[S, M, C\]"), ((f, idx[0]), r"idx: expected \[S, N, k\]"),
           ((f, idx, w[:, :, :2]), "weights: expected the shape of idx"), ((f[:1], idx), "same number of clouds"),
           ((f, torch.zeros(2, 0, 3, dtype=torch.int64)), "idx: the neighbour kernels take 1 .. 65536 points"),
           ((torch.zeros(2, 0, 4), idx), "features: the neighbour kernels take 1 .. 65536 points"),
           ((f, torch.zeros(2, 5, 0, dtype=torch.int64)), "k in 1 .. 32"), ((f, torch.zeros(2, 5, 33, dtype=torch.int64)), "k in 1 .. 32"),
           ((torch.zeros(2, 6, 0), idx), "1 .. 4096 channels"), ((torch.zeros(2, 6, 4097), idx), "1 .. 4096 channels")]
    for args, message in bad:
        with pytest.raises(ValueError, match=message):
            agg(*args)
    for per in (0, -1, 1.5, True, "2"):
        with pytest.raises(ValueError, match="max_clouds_per_launch must be an integer >= 1"):
            agg(f, idx, max_clouds_per_launch=per)
        with pytest.raises(ValueError, match="max_clouds_per_launch must be an integer >= 1"):
            neighbors.edge_features(torch.zeros(2, 6, 3), f, max_clouds_per_launch=per)
    # valid arguments on the CPU: no fallback
    for call in (lambda: agg(f, idx), lambda: agg(f, idx.int(), w), lambda: neighbors.neighbor_mean(f, idx)):
        with pytest.raises(hip.NovaHipError, match="runs on the GPU"):
            call()
    pts = torch.zeros(2, 6, 3)
    edge, interp = neighbors.edge_features, neighbors.knn_interpolate
    with pytest.raises(ValueError, match=r"points: expected \[S, N, 3\]"):
        edge(torch.zeros(2, 6, 2), f)
    with pytest.raises(ValueError, match="points: points must be finite"):
        edge(torch.full((2, 6, 3), float("nan")), f)
    with pytest.raises(ValueError, match="features: expected a floating tensor"):
        edge(pts, f.long())
    with pytest.raises(ValueError, match="features: expected one row per point"):
        edge(pts, torch.zeros(2, 5, 4))
    for k in (0, -1, 2.0, True):
        with pytest.raises(ValueError, match="k must be an integer >= 1"):
            edge(pts, f, k=k)
    with pytest.raises(hip.NovaHipError):
        edge(pts, f)
    q = torch.zeros(2, 9, 3)
    with pytest.raises(ValueError, match="same number of clouds"):
        interp(q[:1], pts, f)
    with pytest.raises(ValueError, match="values: expected one row per point"):
        interp(q, pts, torch.zeros(2, 9, 4))
    for k in (0, 7, 33, 1.0, True):
        with pytest.raises(ValueError, match="k must be an integer in 1 .. 6"):
            interp(q, pts, f, k=k)
    for eps in (0, -1e-8, float("inf"), float("nan"), "1", True):
        with pytest.raises(ValueError, match="eps must be a finite number > 0"):
            interp(q, pts, f, eps=eps)
    with pytest.raises(hip.NovaHipError):
        interp(q, pts, f)
    assert set(neighbors.stats) == {"forward_launches", "inverse_launches", "feature_grad_launches", "weight_grad_launches"}
    assert neighbors._default_clouds_per_launch(2048, 2048, 8, 768) >= 32 and neighbors._default_clouds_per_launch(65536, 65536, 32, 4096) == 1
    assert metrics.KNN_MAX_K == 32


def test_abi_rejections_in_the_stated_order():
    """Every error of the three entries, in the order include/nova_hip.h states, before any device work (no GPU needed)."""
    from nova_pointcloud_amd import hip, metrics, neighbors

    lib = hip.load(check_device=False)
    MB = 1 << 28  # pointers far apart: never dereferenced, rejected first
    f, idx, w, out, g, offsets, edges, gf, gw = (ctypes.c_void_p(MB * i) for i in range(1, 10))
    big, wide = metrics.KNN_MAX_POINTS + 1, neighbors.NEIGHBOR_MAX_CHANNELS + 1
    fwd = lambda S, N, M, k, C, f=f, idx=idx, w=w, out=out: lib.nova_pointset_neighbor_aggregate(f, idx, w, out, S, N, M, k, C, None)
    inv = lambda S, N, M, k, C=None, idx=idx, offsets=offsets, edges=edges: lib.nova_pointset_neighbor_inverse(idx, offsets, edges, S, N, M, k, None)
    bwd = lambda S, N, M, k, C, f=f, idx=idx, w=w, g=g, offsets=offsets, edges=edges, gf=gf, gw=gw: lib.nova_pointset_neighbor_aggregate_bwd(
        f, idx, w, g, offsets, edges, gf, gw, S, N, M, k, C, None)
    err = lib.nova_last_error
    for fn in (fwd, inv, bwd):
        for N, M in ((0, 8), (8, 0), (big, 8), (8, big)):
            assert fn(2, N, M, 0, 0) == -2 and b"NOVA_KNN_MAX_POINTS" in err()  # before C and k
        for k in (0, 33):
            assert fn(70000, 8, 8, k, 4) == -1 and b"NOVA_KNN_MAX_K" in err()  # before the cloud count
            assert fn(0, 8, 8, k, 4) == -1  # also without clouds
        assert fn(65536, 8, 8, 8, 4) == -2 and b"65535" in err()
        assert fn(0, 8, 8, 8, 4) == 0 and fn(-3, 8, 8, 32, 4) == 0 and fn(0, 0, 8, 8, 4) == -2
    for fn in (fwd, bwd):
        for C in (0, wide):
            assert fn(2, 8, 8, 0, C) == -2 and b"NOVA_NEIGHBOR_MAX_CHANNELS" in err()  # before k
    for name in ("f", "idx", "out"):
        assert fwd(2, 8, 8, 8, 4, **{name: None}) == -1 and b"null" in err(), name
    for name in ("idx", "offsets", "edges"):
        assert inv(2, 8, 8, 8, **{name: None}) == -1 and b"null" in err(), name
    for name in ("f", "idx", "g"):
        assert bwd(2, 8, 8, 8, 4, **{name: None}) == -1 and b"null" in err(), name
    assert bwd(2, 8, 8, 8, 4, w=None) == -1 and b"gw given without w" in err()
    assert bwd(2, 8, 8, 8, 4, w=None, f=None) == -1 and b"null" in err()  # the null check comes first
    assert bwd(2, 8, 8, 8, 4, gf=None, gw=None) == -1 and b"both NULL" in err()
    assert bwd(2, 8, 8, 8, 4, w=None, gf=None, gw=None) == -1 and b"both NULL" in err()
    for name in ("offsets", "edges"):
        assert bwd(2, 8, 8, 8, 4, **{name: None}) == -1 and b"inverse list" in err(), name
    # outputs must not overlap inputs (or each other): checked last
    assert fwd(2, 8, 8, 8, 4, out=f) == -1 and b"overlaps" in err()
    assert fwd(2, 8, 8, 8, 4, out=ctypes.c_void_p(MB + 2 * 8 * 4 * 4 - 4)) == -1 and b"overlaps" in err()  # the last float of f
    assert fwd(2, 8, 8, 8, 4, out=idx) == -1 and fwd(2, 8, 8, 8, 4, out=w) == -1
    assert inv(2, 8, 8, 8, offsets=idx) == -1 and inv(2, 8, 8, 8, edges=idx) == -1 and inv(2, 8, 8, 8, edges=offsets) == -1 and b"overlap" in err()
    assert bwd(2, 8, 8, 8, 4, gf=g) == -1 and bwd(2, 8, 8, 8, 4, gw=w) == -1 and bwd(2, 8, 8, 8, 4, gw=gf) == -1 and b"overlaps" in err()
    assert bwd(2, 8, 8, 8, 4, gf=g, offsets=None) == -1 and b"inverse list" in err()  # before the overlap check
    assert bwd(0, 8, 8, 8, 4, f=None, idx=None, w=None, g=None, offsets=None, edges=None, gf=None, gw=None) == 0
    assert lib.nova_version() == hip.ABI_VERSION


def test_header_constants():
    from nova_pointcloud_amd import hip, metrics, neighbors

    header = open(os.path.join(ROOT, "include", "nova_hip.h")).read()
    const = lambda name: int(re.search(r"#define " + name + r" (\d+)", header).group(1))
    assert const("NOVA_NEIGHBOR_MAX_CHANNELS") == neighbors.NEIGHBOR_MAX_CHANNELS >= 2048
    assert const("NOVA_KNN_MAX_K") == metrics.KNN_MAX_K and const("NOVA_KNN_MAX_POINTS") == metrics.KNN_MAX_POINTS
    for needle in ("nova_pointset_neighbor_aggregate", "nova_pointset_neighbor_inverse", "nova_pointset_neighbor_aggregate_bwd",
                   ":176-190", ":192-223", ":286-290", "DEVIATION", "does not run as written"):
        assert needle in header, needle
    for name in ("nova_pointset_neighbor_aggregate", "nova_pointset_neighbor_inverse", "nova_pointset_neighbor_aggregate_bwd"):
        assert name in hip.SIGNATURES
    source = open(os.path.join(ROOT, "nova_pointcloud_amd", "csrc", "neighbor.hip")).read()
    kconst = lambda name: int(re.search(name + r" = (\d+);", source).group(1))
    assert (kconst("NB_T"), kconst("NB_TILE"), kconst("NB_Q")) == (256, 4096, 64)  # the shapes of this file are built around them
    assert "atomic" not in re.sub(r"//.*", "", source)  # no atomics anywhere: one order of summation
    assert "neighbor.hip" in open(os.path.join(ROOT, "nova_pointcloud_amd", "csrc", "Makefile")).read()
    assert {s for s, *_ in SHAPES} == {1, 2, 3, 4, 5}
    assert {c for _, c, *_ in SHAPES} >= {1, 3, 4, 63, 64, 65, 255, 256, 257, 768} and {k for _, _, k, _, _ in SHAPES} == {1, 2, 8, 31, 32}
    assert {n for *_, n, _ in SHAPES} == {m for *_, m in SHAPES} == {1, 63, 64, 65, 257} and any(n != m for *_, n, m in SHAPES)


# --------------------------------------------------------------------------------------------- GPU
NAN = float("nan")
SENTINEL = -77


def run_abi(hip, f, idx, w, g, per=None, want_gf=True, want_gw=None):
    """The three raw entries on GPU copies of the CPU tensors, every output pre-filled (NaN, or SENTINEL for the integer
    lists) so that an unwritten element shows; clouds go out `per` at a time. Returns CPU tensors."""
    dev = torch.device("cuda")
    S, M, C = f.shape
    N, k = idx.shape[1:]
    want_gw = w is not None if want_gw is None else want_gw
    fd, gd = f.to(dev).contiguous(), g.to(dev).contiguous()
    ix = idx.to(dev).to(torch.int32).contiguous()
    wd = w.to(dev).contiguous() if w is not None else None
    out = torch.full((S, N, C), NAN, device=dev)
    gf = torch.full((S, M, C), NAN, device=dev) if want_gf else None
    gw = torch.full((S, N, k), NAN, device=dev) if want_gw else None
    offsets = torch.full((S, M + 1), SENTINEL, dtype=torch.int32, device=dev)
    edges = torch.full((S, N * k), SENTINEL, dtype=torch.int32, device=dev)
    at = lambda t, s0: t[s0].data_ptr() if t is not None else None
    per = S if per is None else per
    stream = hip.stream_ptr()
    for s0 in range(0, S, per):
        n = min(per, S - s0)
        hip.call("nova_pointset_neighbor_aggregate", at(fd, s0), at(ix, s0), at(wd, s0), at(out, s0), n, N, M, k, C, stream)
        hip.call("nova_pointset_neighbor_inverse", at(ix, s0), at(offsets, s0), at(edges, s0), n, N, M, k, stream)
        if want_gf or want_gw:
            hip.call("nova_pointset_neighbor_aggregate_bwd", at(fd, s0), at(ix, s0), at(wd, s0), at(gd, s0), at(offsets, s0), at(edges, s0),
                     at(gf, s0), at(gw, s0), n, N, M, k, C, stream)
    torch.cuda.synchronize()
    cpu = lambda t: t.cpu() if t is not None else None
    return dict(out=cpu(out), offsets=cpu(offsets), edges=cpu(edges), gf=cpu(gf), gw=cpu(gw))


def make_indices(pattern, S, N, M, k, seed):
    """idx [S, N, k] int64 on the CPU, or None where the pattern needs k <= M and the case has fewer targets."""
    from nova_pointcloud_amd import metrics

    gen = torch.Generator().manual_seed(seed)
    if pattern in ("knn", "hub"):
        if k > M:
            return None
        x, y = (torch.randn(S, N, 3, generator=gen), torch.randn(S, M, 3, generator=gen)) if pattern == "knn" else (torch.zeros(S, N, 3), torch.zeros(S, M, 3))
        idx = metrics.knn_points(x.cuda(), y.cuda(), k=k, exclude_self=False, return_distances=False).cpu()
        if pattern == "hub":  # the lowest-index tie rule: every query names the targets 0 .. k-1
            assert torch.equal(idx, torch.arange(k).expand(S, N, k))
        return idx
    idx = torch.randint(0, M, (S, N, k), generator=gen)  # uniformly random, with duplicates inside rows
    if pattern == "out_of_range":
        outside = torch.tensor([-1, M, M + 5, -2 ** 31, 2 ** 31 - 1, -M - 1])
        idx[:, N // 2, :] = outside[torch.arange(k) % 6]  # a whole row, in every cloud
        idx[:, 0, 0] = M  # and the first term of the first row
        idx[:, -1, -1] = -1
    return idx


@pytest.mark.gpu
@pytest.mark.parametrize("S,C,k,N,M", SHAPES)
def test_kernels_bitwise_against_the_restatement(hip, S, C, k, N, M):
    """out, the inverse list and gf are bitwise the restatement's, mean and weighted form, on every index pattern; gw is within
    the any-order bound of its float64 value and bitwise the same in one launch and cloud by cloud."""
    ran = 0
    for p, pattern in enumerate(PATTERNS):
        idx = make_indices(pattern, S, N, M, k, seed=100 + p)
        if idx is None:
            continue
        f, g, w = rand(S, M, C, seed=200 + p), rand(S, N, C, seed=300 + p), rand(S, N, k, seed=400 + p)
        offsets, edges = ref_inverse(idx, M)
        val, mag = gw_float64(f, idx, g)
        for weights in (None, w):
            got = run_abi(hip, f, idx, weights, g)
            tag = (pattern, weights is not None)
            assert same_bits(got["out"], ref_forward(f, idx, weights)), tag
            assert torch.equal(got["offsets"], offsets), tag
            for s in range(S):
                total = int(offsets[s, M])
                assert got["edges"][s, :total].tolist() == edges[s].tolist(), tag
                assert bool((got["edges"][s, total:] == SENTINEL).all()), tag  # slots past offsets[s, M] are not written
            assert same_bits(got["gf"], ref_gf(g, idx, weights, M)), tag
            if weights is not None:
                assert not bool(torch.isnan(got["gw"]).any()), tag
                err = (got["gw"].double() - val).abs()
                print(f"{tag}: gw max error / bound = {float((err / gw_bound(mag, C).clamp_min(1e-300)).max()):.3g}")
                assert bool((err <= gw_bound(mag, C)).all()), tag
                assert bool((got["gw"][mag == 0] == 0).all()), tag
                split = run_abi(hip, f, idx, weights, g, per=1, want_gf=False)
                assert same_bits(split["gw"], got["gw"]) and same_bits(split["out"], got["out"]), tag
        ran += 1
    assert ran >= 2


def api_gradients(f, idx, w, g, wanted=(True, True), **kw):
    """(out, gf, gw) of neighbors.neighbor_aggregate under the upstream gradient g, on the GPU."""
    from nova_pointcloud_amd import neighbors

    fl = f.detach().clone().cuda().requires_grad_(wanted[0])
    wl = w.detach().clone().cuda().requires_grad_(wanted[1]) if w is not None else None
    out = neighbors.neighbor_aggregate(fl, idx.cuda(), wl, **kw)
    assert out.dtype == torch.float32 and out.shape == (f.shape[0], idx.shape[1], f.shape[2])
    if fl.requires_grad or (wl is not None and wl.requires_grad):
        out.backward(g.cuda())
    return out.detach(), fl.grad, wl.grad if wl is not None else None


@pytest.mark.gpu
@pytest.mark.parametrize("C", [65, 260])
def test_bitwise_reproducible_across_splits_positions_and_runs(hip, C):
    S, N, M, k = 5, 65, 63, 8
    f, g, w = rand(S, M, C, seed=11), rand(S, N, C, seed=12), rand(S, N, k, seed=13)
    idx = make_indices("out_of_range", S, N, M, k, seed=14)
    base = api_gradients(f, idx, w, g)
    for per in (1, 2, None, None):  # None twice: two runs
        again = api_gradients(f, idx, w, g, max_clouds_per_launch=per)
        assert all(same_bits(a, b) for a, b in zip(again, base)), per
    roll = [1, 2, 3, 4, 0]  # every cloud at another batch position
    moved = api_gradients(f[roll], idx[roll], w[roll], g[roll])
    assert all(same_bits(a, b[roll]) for a, b in zip(moved, base))
    alone = api_gradients(f[3:4], idx[3:4], w[3:4], g[3:4])
    assert all(same_bits(a, b[3:4]) for a, b in zip(alone, base))
    mean = api_gradients(f, idx, None, g)
    for per in (1, 2):
        again = api_gradients(f, idx, None, g, max_clouds_per_launch=per)
        assert same_bits(again[0], mean[0]) and same_bits(again[1], mean[1]) and again[2] is None


@pytest.mark.gpu
def test_binding_returns_the_raw_abi_gradients(hip):
    """The autograd binding checked by comparison: backward() returns exactly what the raw entries give, nothing for idx, a bf16
    gradient for a bf16 input, and the inverse list and the gf kernel are skipped when only the weights need a gradient."""
    from nova_pointcloud_amd import neighbors

    S, N, M, k, C = 3, 65, 33, 8, 20
    f, g, w = rand(S, M, C, seed=21), rand(S, N, C, seed=22), rand(S, N, k, seed=23)
    idx = make_indices("random", S, N, M, k, seed=24)
    raw = run_abi(hip, f, idx, w, g)
    for index in (idx, idx.int()):
        out, gf, gw = api_gradients(f, index, w, g)
        assert same_bits(out.cpu(), raw["out"]) and same_bits(gf.cpu(), raw["gf"]) and same_bits(gw.cpu(), raw["gw"])
    raw_mean = run_abi(hip, f, idx, None, g)
    out, gf, gw = api_gradients(f, idx, None, g)
    assert same_bits(out.cpu(), raw_mean["out"]) and same_bits(gf.cpu(), raw_mean["gf"]) and gw is None
    assert same_bits(neighbors.neighbor_mean(f.cuda(), idx.cuda()).cpu(), raw_mean["out"])
    # backward called as autograd calls it: one entry per forward argument, None for idx and for the launch split
    ctx = types.SimpleNamespace(saved_tensors=(f.cuda(), idx.int().cuda(), w.cuda()), per=S, needs_input_grad=(True, False, True, False))
    grads = neighbors._Aggregate.backward(ctx, g.cuda())
    assert len(grads) == 4 and grads[1] is None and grads[3] is None
    assert same_bits(grads[0].cpu(), raw["gf"]) and same_bits(grads[2].cpu(), raw["gw"])
    # only the weights need a gradient: no inverse list, no gf kernel
    before = dict(neighbors.stats)
    out, gf, gw = api_gradients(f, idx, w, g, wanted=(False, True))
    delta = {name: neighbors.stats[name] - before[name] for name in before}
    assert delta == {"forward_launches": 1, "inverse_launches": 0, "feature_grad_launches": 0, "weight_grad_launches": 1}
    assert gf is None and same_bits(gw.cpu(), raw["gw"])
    before = dict(neighbors.stats)
    out, gf, gw = api_gradients(f, idx, w, g, wanted=(True, False), max_clouds_per_launch=2)
    delta = {name: neighbors.stats[name] - before[name] for name in before}
    assert delta == {"forward_launches": 2, "inverse_launches": 2, "feature_grad_launches": 2, "weight_grad_launches": 0}
    assert gw is None and same_bits(gf.cpu(), raw["gf"])
    before = dict(neighbors.stats)
    api_gradients(f, idx, w, g, wanted=(False, False))
    assert neighbors.stats["forward_launches"] == before["forward_launches"] + 1 and neighbors.stats["inverse_launches"] == before["inverse_launches"]
    # bf16 inputs: the kernels see the float32 casts, the gradients come back in bf16, the float32 gradient rounded once
    fb, wb = f.bfloat16(), w.bfloat16()
    raw16 = run_abi(hip, fb.float(), idx, wb.float(), g)
    out, gf, gw = api_gradients(fb, idx, wb, g)
    assert gf.dtype == torch.bfloat16 and gw.dtype == torch.bfloat16 and same_bits(out.cpu(), raw16["out"])
    assert torch.equal(gf.cpu(), raw16["gf"].bfloat16()) and torch.equal(gw.cpu(), raw16["gw"].bfloat16())


@pytest.mark.gpu
@pytest.mark.parametrize("N,C,k", [(257, 65, 8), (5, 4, 8)])
def test_edge_features_against_the_gather_form(hip, N, C, k):
    """edge_features against torch's gather / mean form on the same GPU with the same indices. Value: both sides sum k terms
    (k - 1 roundings), divide and subtract: (k + 1) u (|f_i| + mean_t |f_jt|). Feature gradient under the upstream G:
    gf_j = G_j - sum over the deg_j edges naming j of G_i / k, each term one rounding, deg_j additions:
    (deg_j + 1) u (|G_j| + sum |G_i| / k), the in-degree-scaled analogue."""
    from nova_pointcloud_amd import metrics, neighbors

    S = 2
    pts, f, G = rand(S, N, 3, seed=31).cuda(), rand(S, N, C, seed=32).cuda(), rand(S, N, C, seed=33).cuda()
    kk = min(k, N)
    idx = metrics.knn_points(pts, pts, k=kk, exclude_self=False, return_distances=False)
    assert idx.shape == (S, N, kk) and torch.equal(idx[:, :, 0], torch.arange(N, device="cuda").expand(S, N))  # the point itself
    sidx = torch.arange(S, device="cuda")[:, None, None]
    fl = f.clone().requires_grad_(True)
    pl = pts.clone().requires_grad_(True)
    got = neighbors.edge_features(pl, fl, k=k)
    got.backward(G)
    assert pl.grad is None  # not differentiable in the points
    ft = f.clone().requires_grad_(True)
    want = ft - ft[sidx, idx].mean(2)
    want.backward(G)
    bound = (kk + 1) * U * (f.abs().double() + f.abs().double()[sidx, idx].mean(2))
    err = (got.detach().double() - want.detach().double()).abs()
    print(f"value: max error / bound = {float((err / bound).max()):.3g}")
    assert bool((err <= bound).all())
    mag, deg = torch.zeros(S, N, C, dtype=torch.float64, device="cuda"), torch.zeros(S, N, dtype=torch.float64, device="cuda")
    mag.index_put_((sidx.expand(S, N, kk), idx), (G.abs().double() / kk)[:, :, None, :].expand(S, N, kk, C), accumulate=True)
    deg.index_put_((sidx.expand(S, N, kk), idx), torch.ones(S, N, kk, dtype=torch.float64, device="cuda"), accumulate=True)
    gbound = (deg[..., None] + 1) * U * (G.abs().double() + mag)
    gerr = (fl.grad.double() - ft.grad.double()).abs()
    print(f"gradient: max error / bound = {float((gerr / gbound).max()):.3g}")
    assert bool((gerr <= gbound).all())
    assert same_bits(neighbors.edge_features(pts, f, k=k, max_clouds_per_launch=1), got.detach())


def dense_interpolate(q, p, v, k, eps):
    """The dense float64 form: cdist, topk, gather, inverse-distance weights."""
    S = q.shape[0]
    d2 = torch.cdist(q, p).square()
    near, idx = torch.topk(d2, k=k, largest=False)
    a = 1.0 / (near + eps)
    w = a / a.sum(-1, keepdim=True)
    return (w[..., None] * v[torch.arange(S, device=q.device)[:, None, None], idx]).sum(2), idx


@pytest.mark.gpu
def test_knn_interpolate(hip):
    """k = 1 returns the nearest point's value exactly (a / a == 1). k = 3, N = 65, T = 130 against float64 autograd of the dense
    form, on random points (no distance ties). Tolerances, counting float32 roundings at relative size u each, to first order:
    d2 = sum of three squared differences: 4; a = 1 / (d2 + eps): + 2 = 6; w = a / sum_3 a: + 6 (the other a) + 3 = 15, taken as 16.
      value     w v rounded and k - 1 additions:                  (16 + k) u sum_t w_t |v_t|
      d values  per target, deg_j terms w g and deg_j additions:  (16 + 1 + deg_j) u sum_e w_e |g_i|
      d queries the weight gradient gw_t carries (C + 1) u of sum_c |g_c v_c| =: m_t (the any-order bound); the chain back through
                w = a / A, a = 1 / (d2 + eps), d2 = |q - p|^2 is under 16 products, quotients and sums on values that carry at
                most 16 u themselves, and k + 3 additions join the terms: (C + 1 + 32 + k + 3) u, taken as (C + 64) u, times the
                sum of absolute terms  T_i = sum_t a_t^2 ((m_t + sum_s m_s w_s) / A) 2 |q_i - p_t|  per axis
      d points  the same terms gathered per source, deg_j more additions: (C + 64 + deg_j) u sum_e (the term of edge e)."""
    from nova_pointcloud_amd import metrics, neighbors

    S, T, N, C, eps = 2, 130, 65, 5, 1e-8
    q, p, v, G = rand(S, T, 3, seed=41).cuda(), rand(S, N, 3, seed=42).cuda(), rand(S, N, C, seed=43).cuda(), rand(S, T, C, seed=44).cuda()
    sidx = torch.arange(S, device="cuda")[:, None, None]
    idx1 = metrics.knn_points(q, p, k=1, exclude_self=False, return_distances=False)
    assert same_bits(neighbors.knn_interpolate(q, p, v, k=1), v[sidx, idx1][:, :, 0])

    k = 3
    leaves = [t.clone().requires_grad_(True) for t in (q, p, v)]
    out = neighbors.knn_interpolate(*leaves, k=k, eps=eps)
    out.backward(G)
    leaves64 = [t.double().requires_grad_(True) for t in (q, p, v)]
    out64, idx64 = dense_interpolate(*leaves64, k, eps)
    out64.backward(G.double())
    idx = metrics.knn_points(q, p, k=k, exclude_self=False, return_distances=False)
    assert torch.equal(idx, idx64)  # the same neighbours in the same order: no ties
    q64, p64, v64, G64 = q.double(), p.double(), v.double(), G.double()
    near = p64[sidx, idx]  # [S, T, k, 3]
    diff = (q64[:, :, None, :] - near).abs()
    a = 1.0 / ((q64[:, :, None, :] - near).square().sum(-1) + eps)
    A = a.sum(-1, keepdim=True)
    w = a / A
    vn = v64[sidx, idx]  # [S, T, k, C]
    ratio = lambda err, bound: float((err / bound.clamp_min(1e-300)).max())
    vbound = (16 + k) * U * (w[..., None] * vn.abs()).sum(2)
    verr = (out.detach().double() - out64.detach()).abs()
    edge = sidx.expand(S, T, k)
    deg = torch.zeros(S, N, dtype=torch.float64, device="cuda").index_put_((edge, idx), torch.ones(S, T, k, dtype=torch.float64, device="cuda"), accumulate=True)
    gvmag = torch.zeros(S, N, C, dtype=torch.float64, device="cuda").index_put_((edge, idx), w[..., None] * G64.abs()[:, :, None, :], accumulate=True)
    gvbound = (17 + deg[..., None]) * U * gvmag
    gverr = (leaves[2].grad.double() - leaves64[2].grad).abs()
    m = (G64.abs()[:, :, None, :] * vn.abs()).sum(-1)  # [S, T, k]
    term = (a.square() * (m + (m * w).sum(-1, keepdim=True)) / A)[..., None] * 2 * diff  # [S, T, k, 3]
    gqbound = (C + 64) * U * term.sum(2)
    gqerr = (leaves[0].grad.double() - leaves64[0].grad).abs()
    gpmag = torch.zeros(S, N, 3, dtype=torch.float64, device="cuda").index_put_((edge, idx), term, accumulate=True)
    gpbound = (C + 64 + deg[..., None]) * U * gpmag
    gperr = (leaves[1].grad.double() - leaves64[1].grad).abs()
    print(f"error / bound: value {ratio(verr, vbound):.3g}, d values {ratio(gverr, gvbound):.3g}, d queries {ratio(gqerr, gqbound):.3g}, "
          f"d points {ratio(gperr, gpbound):.3g}")
    assert bool((verr <= vbound).all()) and bool((gverr <= gvbound).all())
    assert bool((gqerr <= gqbound).all()) and bool((gperr <= gpbound).all())

    # a query coincident with a source: d2 = 0 there, weight 1 / eps before normalisation; finite values and gradients
    qc = q.clone()
    qc[0, 0], qc[1, 5] = p[0, 3], p[1, 64]
    leaves = [t.clone().requires_grad_(True) for t in (qc, p, v)]
    out = neighbors.knn_interpolate(*leaves, k=k, eps=eps)
    out.backward(G)
    assert bool(torch.isfinite(out).all()) and all(bool(torch.isfinite(t.grad).all()) for t in leaves)
    assert torch.allclose(out[0, 0], v[0, 3], rtol=1e-5, atol=1e-5)  # the coincident source carries almost all the weight
