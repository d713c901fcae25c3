"""Distance-weighted interpolation (csrc/interp.hip, metrics.kernel_interpolate) and the two functions of the reference on
it (metrics.feature_aware_interpolation, metrics.adaptive_sampling): the input, device and C ABI checks and the pure-torch
branches (CPU), and the kernel against a float64 restatement of the definition (GPU).

The definition restated here (include/nova_hip.h, nova_pointset_kernel_interpolate): out[s, i] = softmax_j(-d(i, j) / tau) @ v[s]
with d the Euclidean distance, computed in float64 from the float32 inputs; tau = inf is the plain mean.

Exact cases: on integer lattice coordinates every squared distance is an exact small integer, equal squared distances have
equal square roots and different ones differ by more than 0.018 (sqrt(768) - sqrt(767)), so
  tau = inf     every weight is exp2(+-0) = 1: the output is sum_j v_j / N, the sums exact integers below 2^24
  tau = 2^-20   scale = log2(e) 2^20: a tied-nearest source has weight exp2(0) = 1, every other one exp2(< -27000) = 0: the
                output is the sum of the tied nearest sources' values divided by their count
and the kernel must give the correctly rounded float32 quotient bit for bit, for every query. One source dropped, doubled or
misplaced at a tile, chunk or wave boundary changes it (value channel 0 is the source index).

Shapes: the boundaries of the kernel as built, not the workload. T = 1 | 63 | 64 | 65 | 130 across the 64 queries of a
workgroup; N = 1 | 63 | 64 | 65 (one wave's chunk; waves 1 .. 3 without a source), 255 | 256 | 257 (one round of the four
waves), 1023 | 1024 | 1025 and 2049 (the 1024-source tile): every N at T = 65 and every T at N = 257. Every shape runs all
channel forms C = 1, 3 (values=None), 3 (explicit), 4, 5, 8 (the template rungs 4 and 8 and the form without a value tile);
the cloud count S = 1 .. 5 cycles over the shapes."""
import ctypes
import functools
import math
import os
import re

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INF = float("inf")
N_ALL = (1, 63, 64, 65, 255, 256, 257, 1023, 1024, 1025, 2049)
T_ALL = (1, 63, 64, 65, 130)
TN = [(65, n) for n in N_ALL] + [(t, 257) for t in T_ALL if t != 65]
SHAPES = [(1 + k % 5, t, n) for k, (t, n) in enumerate(TN)]  # (S, T, N)
CHANNELS = (1, None, 3, 4, 5, 8)  # None: values=None, the source points themselves
TEMPERATURES = (1.0, 0.25, 1.0 / 16)
U = 2.0 ** -24


# --------------------------------------------------------------------------------------------- restatement
def restated(q, p, v, tau):
    """softmax(-d / tau) @ v in float64, d from the float32 inputs: [S, T, C] float64 on q's device."""
    q64, p64 = q.double(), p.double()
    d2 = torch.zeros(q.shape[0], q.shape[1], p.shape[1], dtype=torch.float64, device=q.device)
    for c in range(3):
        d2 += (q64[:, :, None, c] - p64[:, None, :, c]) ** 2
    return torch.softmax(-d2.sqrt() / tau, dim=-1) @ v.double()


def test_restatement_on_hand_cases():
    # sources at distance 0 and ln 2 of the query: weights 1 and 1/2, normalised 2/3 and 1/3
    q = torch.zeros(1, 1, 3, dtype=torch.float64)
    p = torch.tensor([[[0.0, 0, 0], [0, math.log(2.0), 0]]], dtype=torch.float64)
    v = torch.tensor([[[0.0, 6.0], [3.0, 0.0]]], dtype=torch.float64)
    assert torch.allclose(restated(q, p, v, 1.0), torch.tensor([[[1.0, 4.0]]], dtype=torch.float64), rtol=0, atol=1e-15)
    # half the temperature squares the weight ratio: 1 and 1/4, normalised 4/5 and 1/5
    assert torch.allclose(restated(q, p, v, 0.5), torch.tensor([[[0.6, 4.8]]], dtype=torch.float64), rtol=0, atol=1e-15)
    # tau = inf: the plain mean, whatever the distances
    far = torch.tensor([[[7.0, -2, 1]]])
    pts = torch.tensor([[[0.0, 0, 0], [1, 0, 0], [0, 5, 0], [3, 3, 3]]])
    assert restated(far, pts, pts, INF).tolist() == [[[1.0, 2.0, 0.75]]]
    # a vanishing temperature picks the nearest source: squared distances 54, 41, 99, 45, so (1, 0, 0)
    assert restated(far, pts, pts, 2.0 ** -20).tolist() == [[[1.0, 0.0, 0.0]]]


def lattice(S, N, seed, half=8):
    return torch.randint(-half, half + 1, (S, N, 3), generator=torch.Generator().manual_seed(seed)).float()


def lattice_values(S, N, C, seed):
    """[S, N, C] integer values: channel 0 the source index j, channel 1 j mod 7, the others random in -8 .. 8."""
    v = torch.randint(-8, 9, (S, N, C), generator=torch.Generator().manual_seed(seed)).float()
    j = torch.arange(N, dtype=torch.float32)
    v[..., 0] = j
    if C > 1:
        v[..., 1] = j % 7
    return v


def quotient32(num, den):
    """The correctly rounded float32 quotient of two tensors of float32-representable values, on num's device: one IEEE
    division of two float64 tensors on the host (a device division by a scalar may multiply by the reciprocal instead),
    rounded once more to float32, which for a quotient of two float32 values is the same as rounding it once."""
    return (num.double().cpu() / den.double().cpu().expand_as(num)).float().to(num.device)


def values_of(form, p, seed):
    """(the `values` argument, the values it stands for) of one channel form on lattice data."""
    if form is None:
        return None, p
    v = lattice_values(p.shape[0], p.shape[1], form, seed).to(p.device)
    return v, v


# --------------------------------------------------------------------------------------------- CPU: checks
def test_input_errors_on_cpu_tensors():
    from nova_pointcloud_amd import hip, metrics

    interp = metrics.kernel_interpolate
    q, p = torch.zeros(2, 5, 3), torch.zeros(2, 8, 3)
    for bad in (torch.zeros(2, 8, 2), torch.zeros(8, 3), torch.zeros(2, 8, 3, 1)):
        with pytest.raises(ValueError, match=r"\[S, N, 3\]"):
            interp(bad, p)
        with pytest.raises(ValueError, match=r"\[S, N, 3\]"):
            interp(q, bad)
        with pytest.raises(ValueError, match=r"\[S, N, 3\]"):
            metrics.feature_aware_interpolation(bad, 4)
        with pytest.raises(ValueError, match=r"\[S, N, 3\]"):
            metrics.adaptive_sampling(bad, 4)
    with pytest.raises(ValueError, match="expected a tensor"):
        interp(q, [[0.0, 0, 0]])
    with pytest.raises(ValueError, match="same number of clouds"):
        interp(torch.zeros(3, 5, 3), p)
    with pytest.raises(ValueError, match="points per cloud"):
        interp(torch.zeros(2, 0, 3), p)
    with pytest.raises(ValueError, match="points per cloud"):
        interp(q, torch.zeros(2, 0, 3))
    with pytest.raises(ValueError, match="65536"):
        interp(q[:1], torch.zeros(1, metrics.INTERP_MAX_POINTS + 1, 3))
    with pytest.raises(ValueError, match="65536"):
        interp(torch.zeros(1, metrics.INTERP_MAX_POINTS + 1, 3), p[:1])
    with pytest.raises(ValueError, match="finite"):
        interp(torch.full((2, 5, 3), float("nan")), p)
    with pytest.raises(ValueError, match="finite"):
        interp(q, torch.tensor([[[0.0, 0, 0], [INF, 0, 0]]] * 2))
    # values
    for C in (0, 9):
        with pytest.raises(ValueError, match="channels"):
            interp(q, p, torch.zeros(2, 8, C))
    for bad in (torch.zeros(2, 7, 3), torch.zeros(3, 8, 3), torch.zeros(2, 8), torch.zeros(2, 8, 3, 1)):
        with pytest.raises(ValueError, match="values: expected"):
            interp(q, p, bad)
    with pytest.raises(ValueError, match="values: expected a tensor"):
        interp(q, p, [[1.0]])
    with pytest.raises(ValueError, match="floating-point"):
        interp(q, p, torch.zeros(2, 8, 2, dtype=torch.int64))
    for bad in (float("nan"), INF, -INF):
        with pytest.raises(ValueError, match="values must be finite"):
            interp(q, p, torch.full((2, 8, 2), bad))
    # temperature, in all three functions
    for bad in (0, 0.0, -1.0, float("nan"), -INF, 1e-39, 1e-300, True, "1", None, torch.tensor(1.0)):
        with pytest.raises(ValueError, match="temperature"):
            interp(q, p, temperature=bad)
        with pytest.raises(ValueError, match="temperature"):
            metrics.feature_aware_interpolation(p, 4, temperature=bad)
        with pytest.raises(ValueError, match="temperature"):
            metrics.adaptive_sampling(p, 4, temperature=bad)
    with pytest.raises(ValueError, match="too small"):
        interp(q, p, temperature=1e-39)
    assert metrics._interp_scale(INF) == 0.0 and metrics._interp_scale(1e300) == 0.0  # the plain mean
    assert metrics._interp_scale(1.0) == float(torch.tensor(math.log2(math.e), dtype=torch.float32))
    assert metrics._interp_scale(2.0 ** -20) == metrics._interp_scale(1) * 2.0 ** 20
    # target_size and empty clouds
    for fn in (metrics.feature_aware_interpolation, metrics.adaptive_sampling):
        for bad in (0, -1, 2.0, True):
            with pytest.raises(ValueError, match="target_size"):
                fn(p, bad)
        with pytest.raises(ValueError, match="empty"):
            fn(torch.zeros(2, 0, 3), 4)
    # valid CPU tensors: no CPU path for the kernel
    with pytest.raises(hip.NovaHipError, match="GPU"):
        interp(q, p)
    with pytest.raises(hip.NovaHipError, match="GPU"):
        interp(q, p, torch.zeros(2, 8, 8), temperature=INF)
    with pytest.raises(hip.NovaHipError, match="GPU"):
        metrics.feature_aware_interpolation(p, 4)
    with pytest.raises(hip.NovaHipError, match="GPU"):
        metrics.adaptive_sampling(p, 4)
    with pytest.raises(hip.NovaHipError, match="GPU"):
        metrics.adaptive_sampling(p, 9)  # the farthest-point order needs the GPU too


def test_pure_torch_branches():
    from nova_pointcloud_amd import metrics

    p = torch.arange(2 * 5 * 3, dtype=torch.float64).reshape(2, 5, 3)  # any dtype: nothing is computed
    assert metrics.adaptive_sampling(p, 5) is p and torch.equal(metrics.feature_aware_interpolation(p, 5), p)
    for target in (5, 6, 10, 13):
        got = metrics.feature_aware_interpolation(p, target, temperature=0.5)
        assert got.shape == (2, target, 3) and got.dtype == p.dtype
        assert torch.equal(got, p[:, torch.arange(target) % 5])
    one = torch.tensor([[[1.0, 2.0, 3.0]]])
    assert torch.equal(metrics.feature_aware_interpolation(one, 4), one.expand(1, 4, 3))
    assert metrics.feature_aware_interpolation(torch.zeros(0, 5, 3), 7).shape == (0, 7, 3)
    assert metrics.adaptive_sampling(torch.zeros(0, 5, 3), 5).shape == (0, 5, 3)
    nan = torch.full((1, 3, 3), float("nan"))  # like resample_clouds, the pure-torch branches do not look at the values
    assert metrics.adaptive_sampling(nan, 3) is nan and metrics.feature_aware_interpolation(nan, 5).shape == (1, 5, 3)


def test_header_constants_and_kernel_shape():
    from nova_pointcloud_amd import hip, metrics

    header = open(os.path.join(ROOT, "include", "nova_hip.h")).read()
    assert metrics.INTERP_MAX_POINTS == int(re.search(r"#define NOVA_INTERP_MAX_POINTS (\d+)", header).group(1)) == 65536
    assert metrics.INTERP_MAX_CHANNELS == int(re.search(r"#define NOVA_INTERP_MAX_CHANNELS (\d+)", header).group(1)) == 8
    assert "transformer_pointcloud_nova.py:128-152" in header and "dead code" in header and ":92-97" in header
    assert hip.SIGNATURES["nova_pointset_kernel_interpolate"][8] is ctypes.c_float
    source = open(os.path.join(ROOT, "nova_pointcloud_amd", "csrc", "interp.hip")).read()
    const = lambda name: int(re.search(name + r" = (\d+);", source).group(1))
    # the one workgroup shape the shapes of this file are built around
    assert (const("INTERP_T"), const("INTERP_Q"), const("INTERP_TILE"), const("INTERP_CHUNK")) == (256, 64, 1024, 64)
    assert isinstance(metrics._INTERP_PAIRS_PER_LAUNCH, int) and metrics._INTERP_PAIRS_PER_LAUNCH >= 1 << 32  # a whole cloud fits a launch
    assert {n for _, t, n in SHAPES if t == 65} == set(N_ALL) and {t for _, t, n in SHAPES if n == 257} == set(T_ALL)
    assert {s for s, _, _ in SHAPES} == {1, 2, 3, 4, 5}


def test_abi_rejections():
    """Argument checks of nova_pointset_kernel_interpolate run before any device work (no GPU needed)."""
    from nova_pointcloud_amd import hip, metrics

    lib = hip.load(check_device=False)
    fn = lib.nova_pointset_kernel_interpolate
    q, p, v, out = (ctypes.c_void_p(4096 * i) for i in (1, 2, 3, 4))  # never dereferenced: rejected first
    assert fn(q, p, v, out, 2, 0, 8, 3, 1.0, None) == -2                                   # T = 0
    assert b"NOVA_INTERP_MAX_POINTS" in lib.nova_last_error()
    assert fn(q, p, v, out, 2, 8, 0, 3, 1.0, None) == -2                                   # N = 0
    assert fn(q, p, v, out, 2, metrics.INTERP_MAX_POINTS + 1, 8, 3, 1.0, None) == -2       # T above the cap
    assert fn(q, p, v, out, 2, 8, metrics.INTERP_MAX_POINTS + 1, 3, 1.0, None) == -2       # N above the cap
    assert b"65536" in lib.nova_last_error()
    assert fn(q, p, v, out, 2, 8, 8, 0, 1.0, None) == -2                                   # C = 0
    assert fn(q, p, v, out, 2, 8, 8, 9, 1.0, None) == -2                                   # C = 9
    assert b"NOVA_INTERP_MAX_CHANNELS" in lib.nova_last_error()
    assert fn(q, p, None, out, 2, 8, 8, 9, 1.0, None) == -2                                # the shape comes first
    for C in (1, 2, 4, 8):
        assert fn(q, p, None, out, 2, 8, 8, C, 1.0, None) == -1                            # v == NULL needs C == 3
    assert b"C == 3" in lib.nova_last_error()
    for bad in (-1.0, -1e-30, float("nan"), INF, -INF):
        assert fn(q, p, v, out, 2, 8, 8, 3, bad, None) == -1                               # scale
        assert b"scale" in lib.nova_last_error()
        assert fn(None, None, None, None, 0, 8, 8, 3, bad, None) == -1                     # also without clouds
    assert fn(None, p, v, out, 2, 8, 8, 3, 1.0, None) == -1 and fn(q, None, v, out, 2, 8, 8, 3, 1.0, None) == -1
    assert fn(q, p, v, None, 2, 8, 8, 3, 1.0, None) == -1                                  # null out
    assert b"null" in lib.nova_last_error()
    assert fn(q, q, None, None, 1, 8, 8, 3, 0.0, None) == -1
    assert fn(None, None, None, None, 0, 8, 8, 3, 0.0, None) == 0                          # S = 0: nothing to do
    assert fn(None, None, None, None, -3, 8, 8, 8, 1.0, None) == -1                        # v == NULL with C = 8 still counts
    assert fn(None, None, v, None, -3, 8, 8, 8, 1.0, None) == 0
    assert fn(None, None, None, None, 0, 0, 8, 3, 1.0, None) == -2                         # and the shape
    assert lib.nova_version() == 405


# --------------------------------------------------------------------------------------------- GPU
def kernel(q, p, v=None, **kw):
    from nova_pointcloud_amd import metrics

    out = metrics.kernel_interpolate(q, p, v, **kw)
    C = 3 if v is None else v.shape[2]
    assert out.shape == (q.shape[0], q.shape[1], C) and out.dtype == torch.float32 and out.device == q.device
    return out


def same_bits(a, b):
    return a.shape == b.shape and torch.equal(a.view(torch.int32), b.view(torch.int32))


@functools.lru_cache(maxsize=None)
def lattice_case(S, T, N, half):
    """(queries, points) on the integer lattice -half .. half, on the GPU; computed once, never modified."""
    return lattice(S, T, 5000 + 7 * T + N, half).cuda(), lattice(S, N, 6000 + N, half).cuda()


@pytest.mark.gpu
@pytest.mark.parametrize("S,T,N", SHAPES + [(1, 65, 4096)])  # 4096: the largest cloud whose index sum is exact
def test_exact_count(hip, S, T, N):
    """tau = inf: every query is sum_j v_j / N in float32, bit for bit."""
    q, p = lattice_case(S, T, N, 8)
    for form in CHANNELS:
        arg, v = values_of(form, p, 7000 + N)
        want = quotient32(v.sum(1), torch.full((1, 1), float(N)))[:, None, :].expand(S, T, v.shape[2])
        assert float(v.abs().sum(1).max()) < 2 ** 24  # every partial sum is an exact float32
        got = kernel(q, p, arg, temperature=INF)
        bad = torch.nonzero((got != want).any(-1).reshape(-1)).reshape(-1)
        print(f"count S {S} T {T} N {N} C {form}: first differing query {int(bad[0]) if bad.numel() else None}")
        assert same_bits(got, want.contiguous()), form


def selection_half(N):
    """Half-width of the lattice of the selection test: about N / 2 cells, so that ties are common (within -8 .. 8)."""
    return min(8, max(1, round(N ** (1 / 3) / 2)))


def restated_selection(q, p, v):
    """(float32 [S, T, C] quotient of the integer sum of the tied nearest sources' values by their count, share of queries with a tie)."""
    d2 = ((q.long()[:, :, None, :] - p.long()[:, None, :, :]) ** 2).sum(-1)  # exact integers
    tied = (d2 == d2.min(dim=-1, keepdim=True).values).double()
    sums, count = tied @ v.double(), tied.sum(-1, keepdim=True)
    assert float(sums.abs().max()) < 2 ** 24
    return quotient32(sums, count), float((count > 1).double().mean())


@pytest.mark.gpu
@pytest.mark.parametrize("S,T,N", SHAPES)
def test_exact_selection(hip, S, T, N):
    """tau = 2^-20: every query is the mean of its tied nearest sources, bit for bit; at least a quarter of the queries of
    every case with N >= 63 have a tie (N = 1 cannot have one)."""
    q, p = lattice_case(S, T, N, selection_half(N))
    for form in CHANNELS:
        arg, v = values_of(form, p, 8000 + N)
        want, ties = restated_selection(q, p, v)
        got = kernel(q, p, arg, temperature=2.0 ** -20)
        bad = torch.nonzero((got != want).any(-1).reshape(-1)).reshape(-1)
        print(f"selection S {S} T {T} N {N} C {form}: first differing query {int(bad[0]) if bad.numel() else None}, "
              f"share of queries with a tie {ties:.2f}")
        assert same_bits(got, want), form
        assert ties >= 0.25 or N == 1


def ball(S, N, seed):
    """Points in the unit ball, denser towards the centre."""
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(S, N, 3, generator=g)
    return x / x.norm(dim=-1, keepdim=True) * torch.rand(S, N, 1, generator=g)


@functools.lru_cache(maxsize=None)
def random_case(S, T, N):
    """(queries, points, {channel form: values argument}) of the random test, on the GPU; computed once, never modified."""
    q, p = ball(S, T, 100 + 3 * T + N).cuda(), ball(S, N, 200 + N).cuda()
    vals = {C: None if C is None else torch.randn(S, N, C, generator=torch.Generator().manual_seed(300 + N + C)).cuda() for C in CHANNELS}
    vals[3] = p.clone() * 3 - 1  # the explicit three-channel form on values of its own
    return q, p, vals


@pytest.mark.gpu
@pytest.mark.parametrize("S,T,N", SHAPES)
def test_random_clouds(hip, S, T, N):
    """Points and queries in the unit ball, tau = 1, 1/4, 1/16, every entry against the float64 restatement within

        (N + 512) * 2^-24 * max_j |v[s, j, c]|

    in three parts, with u = 2^-24 (one float32 rounding, relative):
      N u     the numerator and the denominator are sequential float32 sums of N terms of one sign pattern per weight, each
              addition one rounding: N u relative to max |v| for the quotient (the four-way merge and the division add 6 u,
              which the slack of the next part covers);
      460 u   the argument of exp2 is (m - d) scale with |m - d| <= 2 in the unit ball and scale <= 16 log2(e): |argument|
              <= 46. The two distances, their difference and the product carry about 5 roundings that reach the argument in
              full, an absolute error of 5 * 46 u = 230 u, which is the relative error e of the weight (times ln 2 < 1). The
              output is a ratio of sums weighted by them, which a relative error e of the weights moves by at most
              2 e max |v|: 460 u;
      52 u    exp2 itself (v_exp_f32: 1 ulp = 2 u) and the float32 rounding of scale (46 u / 2), doubled as above: 50 u.
    Nothing is left out of the comparison. Measured on an MI355X: the worst error / bound over all cases is 0.021 (DESIGN.md,
    distance-weighted interpolation)."""
    q, p, vals = random_case(S, T, N)
    worst = 0.0
    for tau in TEMPERATURES:
        for form in CHANNELS:
            v = p if form is None else vals[form]
            got = kernel(q, p, vals[form], temperature=tau)
            want = restated(q, p, v, tau)
            bound = (N + 512) * U * v.abs().amax(dim=1, keepdim=True).double()  # [S, 1, C]
            ratio = float(((got.double() - want).abs() / bound).max())
            worst = max(worst, ratio)
            print(f"random S {S} T {T} N {N} C {form} tau {tau}: worst error / bound {ratio:.4f}")
            assert bool(torch.isfinite(got).all())
            assert bool(((got.double() - want).abs() <= bound).all()), (form, tau, ratio)
    print(f"random S {S} T {T} N {N}: worst error / bound over all forms {worst:.4f}")


@pytest.mark.gpu
def test_bitwise_invariance(hip):
    S, T, N = 5, 130, 1025
    q, p = ball(S, T, 51).cuda(), ball(S, N, 52).cuda()
    for C in (None, 5):
        v = None if C is None else torch.randn(S, N, C, generator=torch.Generator().manual_seed(53)).cuda()
        for tau in (0.25, INF):
            whole = kernel(q, p, v, temperature=tau)
            for per in (1, 2, S):
                assert same_bits(kernel(q, p, v, temperature=tau, max_clouds_per_launch=per), whole), (C, tau, per)
            for s in range(S):  # alone and inside the batch
                one = kernel(q[s:s + 1], p[s:s + 1], None if v is None else v[s:s + 1], temperature=tau)
                assert same_bits(one[0], whole[s]), (C, tau, s)
    for tau in TEMPERATURES + (INF, 2.0 ** -20):  # values=None against a copy of the points as values
        assert same_bits(kernel(q, p, None, temperature=tau), kernel(q, p, p.clone(), temperature=tau)), tau
        # queries aliasing the points against a copy, in both channel forms
        assert same_bits(kernel(p, p, None, temperature=tau), kernel(p.clone(), p, None, temperature=tau)), tau
        assert same_bits(kernel(p, p, p, temperature=tau), kernel(p.clone(), p, p.clone(), temperature=tau)), tau
    # a channel's result does not depend on the other channels or on the rung they put it on
    v8 = torch.randn(S, N, 8, generator=torch.Generator().manual_seed(54)).cuda()
    out8 = kernel(q, p, v8, temperature=0.25)
    for C in (1, 3, 4, 5):
        assert same_bits(kernel(q, p, v8[..., :C].contiguous(), temperature=0.25), out8[..., :C].contiguous()), C
    # other dtypes are converted, as for the points
    assert same_bits(kernel(q.double(), p.double(), v8.double(), temperature=0.25), out8)
    assert kernel(q[:0], p[:0], temperature=1.0).shape == (0, T, 3)
    with pytest.raises(ValueError, match="max_clouds_per_launch"):
        kernel(q, p, max_clouds_per_launch=0)


@pytest.mark.gpu
def test_composites(hip):
    from nova_pointcloud_amd import metrics

    S, N, target = 3, 700, 257
    p = ball(S, N, 61).cuda()
    got = metrics.feature_aware_interpolation(p, target, temperature=0.25, generator=torch.Generator().manual_seed(9))
    perm = torch.randperm(N, generator=torch.Generator().manual_seed(9))[:target].cuda()
    assert same_bits(got, kernel(p[:, perm], p, temperature=0.25))
    # the reference's own form at its temperature of 1 (transformer_pointcloud_nova.py:145-150), in float64
    ref = metrics.feature_aware_interpolation(p, target, generator=torch.Generator().manual_seed(9)).double()
    dist = torch.cdist(p[:, perm].double(), p.double())
    want = torch.sum(torch.softmax(-dist, dim=-1).unsqueeze(-1) * p.double().unsqueeze(1), dim=2)
    assert bool(((ref - want).abs() <= (N + 512) * U * p.abs().amax(dim=1, keepdim=True).double()).all())
    # adaptive_sampling: the three regimes
    assert metrics.adaptive_sampling(p, N) is p
    dense = metrics.adaptive_sampling(p, target, temperature=0.25, generator=torch.Generator().manual_seed(9))
    assert same_bits(dense, got)
    for up in (N + 1, 2 * N, 2 * N + 5):
        sparse = metrics.adaptive_sampling(p, up)
        order = metrics.farthest_point_sample(p, N)[:, torch.arange(up, device="cuda") % N]
        assert sparse.shape == (S, up, 3) and torch.equal(sparse, torch.gather(p, 1, order[:, :, None].expand(S, up, 3)))
        assert torch.equal(sparse[:, :N].sort(dim=1).values, p.sort(dim=1).values)  # every point once before any comes twice
    # the cyclic branch on the GPU
    assert torch.equal(metrics.feature_aware_interpolation(p, N + 3), p[:, torch.arange(N + 3, device="cuda") % N])
    # queries far from every source: exp2 of the raw distances would be 0 / 0
    far = ball(S, 65, 62).cuda() + 1e3
    for v in (None, torch.randn(S, N, 8, generator=torch.Generator().manual_seed(63)).cuda()):
        out = kernel(far, p, v, temperature=1.0)
        vv = p if v is None else v
        lo, hi = vv.amin(dim=1, keepdim=True), vv.amax(dim=1, keepdim=True)
        assert bool(torch.isfinite(out).all())
        slack = (N + 512) * U * vv.abs().amax(dim=1, keepdim=True)  # a weighted average stays inside the values' range
        assert bool((out >= lo - slack).all()) and bool((out <= hi + slack).all())
