"""Depth-aware 3-D positional encoding (csrc/posenc.hip, nova_pointcloud_amd/encoding.py): the reference's
DepthAwarePositionalEncoding (transformer_pointcloud_nova.py:349-389, applied at :456-458) as one HIP forward and one HIP
backward.

restate() is the definition of include/nova_hip.h (nova_pointset_posenc, nova_pointset_posenc_bwd): the arguments
a = (x * scale) / div formed in float32 (IEEE, so bitwise the kernel's), their sines and cosines in float64, and closed-form
gradients in float64. The CPU tests hold it against literal_form(), the reference's forward in this project's own code, and
against torch autograd of it; the GPU tests hold the kernels against it.

TOLERANCE of the forward, written before the first GPU run: against restate(), 4 ulp of the exact value's float32 spacing,
the spacing floored at the one of the smallest normal (2^-149): the OpenCL full-profile limit for sin and cos, which the
device math library is written to. With base, half a spacing of the sum on top (the one rounded addition).

BOUNDS of the backward, written before the first GPU run, by count from restate()'s float64 quantities. u = 2^-24, F = E // 6.
    M_cf  = (|g[6f+2c] cos a_cf| + |g[6f+2c+1] sin a_cf|) / div[f],   T_ic = sum_f M_cf,   A_sc = sum_{i in cloud s} |x_ic| T_ic
    one term: sine and cosine 4 ulp = 8 u each, the product u, the fused sum u, the division u: at most 11 u M_cf
    t_ic      (F + 12) u T_ic                   the terms, plus F u T_ic for a sum of F terms in any order, one u of slack
    gx[i, c]  |scale_c| (F + 13) u T_ic         one more rounding for the product with the scale
    gs[s, c]  (F + N + 13) u A_sc               every t off as above, N fused accumulations in any order
    scale gradient   sum_s bound(gs[s]) + S u sum_s A_sc
plus 1e-30 (1 + |scale_c|), 1e-30 N (1 + max |x|) for intermediates flushed below 2^-126 (fewer than 3000 per row, each
below 1.2e-38). The looser check against torch autograd of literal_form() on the GPU in float32 takes 4 times these bounds
plus 4 u max |a| sum_f (|g[6f+2c]| + |g[6f+2c+1]|) / div[f] (times |scale_c|, or summed with |x_ic|): torch's graph is held
to the same count, and an argument it rounds one ulp apart (2 u |a|) moves its sine and cosine by as much. It is made at
|x scale| about 1 and 100, not at 2^20.

Measured on an MI355X, worst error / bound over all cases: forward 0.38 (0.9994 with base: the addition's half ulp), gx 0.20,
gs 0.13, scale gradient 0.094; the docstrings of test_random_forward and test_random_backward and DESIGN.md.
"""
import ctypes
import functools
import inspect
import math
import os
import re
import subprocess
import sys

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
U = 2.0 ** -24
CHUNK = 32  # == NOVA_POSENC_CHUNK (test_header_constants_and_kernel_shape)
E_CASES = [6, 7, 11, 12, 126, 131, 132, 384, 390, 768, 1024, 1536, 4095, 4096]
N_CASES = [1, 2, 3, 4, 5, CHUNK - 1, CHUNK, CHUNK + 1, 2 * CHUNK + 1]
MAGNITUDES = [1.0, 100.0, 2.0 ** 20]


def reference_table(E):
    """The reference's div_term (:359-360), op for op."""
    return 10000.0 ** (torch.arange(0, E, 2) / E)


def restate(x, scale, div, E, base=None, g=None, arg_dtype=torch.float32):
    """The definition. x [S, N, 3], scale [3], div [>= F]; the arguments are formed in arg_dtype (float32: bitwise the
    kernel's), everything after them in float64. Returns a dict: out [S, N, E]; with g [S, N, E] also gx [S, N, 3], gs [S, 3]
    per cloud, gsum [3] and the sums of magnitudes T [S, N, 3] and A [S, 3] the bounds need."""
    S, N = x.shape[:2]
    F = E // 6
    xs, sc, dv = x.to(arg_dtype), scale.to(arg_dtype), div[:F].to(arg_dtype)
    s = xs * sc  # rounded once
    a = (s[:, :, None, :] / dv[None, None, :, None]).double()  # [S, N, F, 3], rounded once
    sn, cs = a.sin(), a.cos()
    pe = torch.zeros(S, N, E, dtype=torch.float64)
    pe[:, :, :6 * F] = torch.stack([sn, cs], dim=-1).reshape(S, N, 6 * F)  # channel 6 f + 2 c (+ 1)
    res = {"pe": pe, "out": pe if base is None else base.double() + pe, "a": a}
    if g is None:
        return res
    gg = g.double()[:, :, :6 * F].reshape(S, N, F, 3, 2)  # the tail channels of g are not read
    dv64 = dv.double()[None, None, :, None]
    t = ((gg[..., 0] * cs - gg[..., 1] * sn) / dv64).sum(2)
    T = (((gg[..., 0] * cs).abs() + (gg[..., 1] * sn).abs()) / dv64).sum(2)
    G = ((gg[..., 0].abs() + gg[..., 1].abs()) / dv64).sum(2)
    gs = (xs.double() * t).sum(1)
    res.update(gx=sc.double() * t, gs=gs, gsum=gs.sum(0), t=t, T=T, G=G, A=(xs.double().abs() * T).sum(1))
    return res


def literal_form(points, scale, div_term, E):
    """transformer_pointcloud_nova.py:367-389 in this project's words: the zeros, the six strided slice assignments, each with
    its own division. scale is [3], one factor per coordinate. Defined, like the reference, for E % 6 == 0 only."""
    scaled = points * scale
    pe = torch.zeros(points.shape[0], points.shape[1], E, dtype=points.dtype, device=points.device)
    d = div_term[:E // 6]
    for c in range(3):
        pe[:, :, 2 * c::6] = torch.sin(scaled[:, :, c:c + 1] / d)
        pe[:, :, 2 * c + 1::6] = torch.cos(scaled[:, :, c:c + 1] / d)
    return pe


def spacing32(v):
    """The float32 spacing at |v| (float64 tensor), floored at the spacing of the smallest normal, 2^-149."""
    m = v.abs().clamp_min(2.0 ** -126).clamp_max(3.0e38)
    return 2.0 ** (torch.frexp(m).exponent - 24).double()  # m = q 2^e with q in [0.5, 1): spacing 2^(e - 24)


def forward_cap(r, base=None):
    """The docstring's tolerance for every entry of out."""
    cap = 4 * spacing32(r["pe"])
    return cap if base is None else cap + 0.5 * spacing32(r["out"].abs() + cap)


def backward_bounds(r, x, scale, E):
    """The docstring's bounds: (gx [S, N, 3], gs [S, 3], gsum [3])."""
    S, N = x.shape[:2]
    F = E // 6
    sa = scale.double().abs()
    b_gx = sa * (F + 13) * U * r["T"] + 1e-30 * (1 + sa)
    b_gs = (F + N + 13) * U * r["A"] + 1e-30 * N * (1 + x.double().abs().max())
    b_gsum = b_gs.sum(0) + S * U * r["A"].sum(0)
    return b_gx, b_gs, b_gsum


def loose_bounds(r, x, scale, E):
    """4 times backward_bounds plus the allowance for an argument rounded one ulp apart (module docstring)."""
    b_gx, b_gs, b_gsum = backward_bounds(r, x, scale, E)
    slip = 4 * U * r["a"].abs().max() * r["G"]  # [S, N, 3]
    l_gs = 4 * b_gs + (x.double().abs() * slip).sum(1)
    return 4 * b_gx + scale.double().abs() * slip, l_gs, 4 * b_gsum + (l_gs - 4 * b_gs).sum(0)


def random_case(S, N, E, magnitude, seed, custom_table=False):
    """x with |x scale| about `magnitude`; the scales negative and of mixed magnitude; base and g with non-zero tails."""
    gen = torch.Generator().manual_seed(seed)
    scale = torch.tensor([-1.5, 0.03125, 7.0]) * (1 + 0.1 * torch.rand(3, generator=gen))
    x = torch.randn(S, N, 3, generator=gen) * magnitude / scale.abs()
    div = torch.rand(E // 6 + 2, generator=gen) * 50 + 0.01 if custom_table else reference_table(E)
    base = torch.randn(S, N, E, generator=gen)
    g = torch.randn(S, N, E, generator=gen)
    return x, scale, div.float(), base, g


# ---- CPU -------------------------------------------------------------------------------------------------------------------


@pytest.mark.parametrize("E", [6, 96, 768, 1536])
def test_restatement_against_the_reference_form_in_float32(E):
    """literal_form in float32 on the CPU sits inside the forward's cap around restate(), at every magnitude of the GPU cases:
    the reference alone is well inside the tolerance the kernel is held to."""
    for magnitude in MAGNITUDES:
        x, scale, div, base, g = random_case(2, 9, E, magnitude, 17 + E)
        r = restate(x, scale, div, E)
        got = literal_form(x, scale, div, E)
        ratio = ((got.double() - r["out"]).abs() / forward_cap(r)).max().item()
        assert ratio <= 1.0, (E, magnitude, ratio)


@pytest.mark.parametrize("E", [6, 12, 96, 390])
def test_restatement_against_float64_autograd_of_the_reference_form(E):
    """Values and all three closed-form gradients (points, scales, base) against autograd of the literal form in float64."""
    for S, N in ((1, 1), (2, 5), (3, CHUNK + 1)):
        x, scale, div, base, g = (t.double() for t in random_case(S, N, E, 3.0, 100 * N + E))
        xl, sl, bl = (t.clone().requires_grad_(True) for t in (x, scale, base))
        out = bl + literal_form(xl, sl, div, E)
        (out * g).sum().backward()
        r = restate(x, scale, div, E, base, g, arg_dtype=torch.float64)
        for got, want in ((r["out"], out.detach()), (r["gx"], xl.grad), (r["gsum"], sl.grad), (g, bl.grad)):
            assert (got - want).abs().max() <= 1e-11 * (1 + want.abs().max()), (E, S, N)
        assert (r["gs"].sum(0) - r["gsum"]).abs().max() == 0


def test_restatement_tail_channels_and_hand_cases():
    # E % 6 != 0 (the extension): the first 6 F channels are those of E' = 6 F, the tail is +0, g's tail reaches nothing
    for E in (7, 11, 131, 1024):
        F = E // 6
        x, scale, div, base, g = random_case(2, 3, E, 3.0, E)
        r = restate(x, scale, div, E, None, g)
        r6 = restate(x, scale, div, 6 * F, None, g[:, :, :6 * F])
        assert torch.equal(r["out"][:, :, :6 * F], r6["out"]) and (r["out"][:, :, 6 * F:] == 0).all()
        assert not torch.signbit(r["out"][:, :, 6 * F:]).any()
        assert torch.equal(r["gx"], r6["gx"]) and torch.equal(r["gs"], r6["gs"])
    # x = 0: sine channels +0, cosine channels 1, and the gradient is g_sin / div through the sine alone
    E = 12
    div = torch.tensor([2.0, 4.0])
    g = torch.arange(12.0).reshape(1, 1, 12) + 1
    r = restate(torch.zeros(1, 1, 3), torch.tensor([1.0, 2.0, 3.0]), div, E, None, g)
    assert torch.equal(r["out"][0, 0], torch.tensor([0.0, 1.0] * 6, dtype=torch.float64))
    want_t = torch.tensor([1 / 2 + 7 / 4, 3 / 2 + 9 / 4, 5 / 2 + 11 / 4], dtype=torch.float64)
    assert torch.allclose(r["t"][0, 0], want_t, rtol=1e-15) and torch.allclose(r["gx"][0, 0], want_t * torch.tensor([1.0, 2.0, 3.0]))
    assert (r["gs"] == 0).all()


def test_forward_cap_is_four_ulp_floored_at_the_smallest_normal():
    v = torch.tensor([1.0, 1.5, 0.75, 2.0 ** -126, 2.0 ** -140, 0.0, -3.0], dtype=torch.float64)
    want = torch.tensor([2.0 ** -23, 2.0 ** -23, 2.0 ** -24, 2.0 ** -149, 2.0 ** -149, 2.0 ** -149, 2.0 ** -22], dtype=torch.float64)
    assert torch.equal(spacing32(v), want)


def test_python_argument_errors_in_the_stated_order():
    from nova_pointcloud_amd import encoding, hip

    enc = encoding.coordinate_encoding
    x, s = torch.zeros(2, 5, 3), torch.ones(3)
    bad = [
        (dict(points=[1.0], scale=None, embed_dim=12), "points: expected a tensor"),  # types before anything else, points first
        (dict(points=x, scale=None, embed_dim=12), "scale: expected a tensor"),
        (dict(points=x, scale=s, embed_dim=12, base=3.0), "base: expected a tensor"),
        (dict(points=x, scale=s, embed_dim=12, div_term=[1.0, 2.0]), "div_term: expected a tensor"),
        (dict(points=x.long(), scale=s, embed_dim=12.0), "embed_dim must be an integer"),  # types before dtypes
        (dict(points=x, scale=s, embed_dim=True), "embed_dim must be an integer"),
        (dict(points=x.long(), scale=s.reshape(1, 3), embed_dim=12), "points: expected a floating dtype"),  # dtypes before shapes
        (dict(points=x, scale=s.int(), embed_dim=12), "scale: expected a floating dtype"),
        (dict(points=x, scale=s, embed_dim=12, base=torch.zeros(2, 5, 12).int()), "base: expected a floating dtype"),
        (dict(points=x, scale=s, embed_dim=12, div_term=torch.ones(2).long()), "div_term: expected a floating dtype"),
        (dict(points=torch.zeros(2, 5, 4), scale=torch.ones(4), embed_dim=12), r"points: expected \[S, N, 3\]"),
        (dict(points=torch.zeros(5, 3), scale=s, embed_dim=12), r"points: expected \[S, N, 3\]"),
        (dict(points=x, scale=torch.ones(1, 3), embed_dim=12), r"scale: expected the three scales \[3\]"),
        (dict(points=x, scale=s, embed_dim=12, base=torch.zeros(2, 5, 13)), r"base: expected \[S, 5, 12\]"),
        (dict(points=x, scale=s, embed_dim=12, base=torch.zeros(2, 4, 12)), r"base: expected \[S, 5, 12\]"),
        (dict(points=x, scale=s, embed_dim=12, div_term=torch.ones(1)), "div_term: expected a table of at least"),
        (dict(points=x, scale=s, embed_dim=12, div_term=torch.ones(2, 2)), "div_term: expected a table of at least"),
        (dict(points=x, scale=s, embed_dim=5000, base=torch.zeros(3, 5, 5000)), "same number of clouds"),  # counts before ranges
        (dict(points=torch.zeros(2, 0, 3), scale=s, embed_dim=5), "6 .. 4096 channels"),  # embed_dim before the point count
        (dict(points=x, scale=s, embed_dim=encoding.POSENC_MAX_DIM + 1), "6 .. 4096 channels"),
        (dict(points=torch.zeros(2, 0, 3), scale=s, embed_dim=12), "1 .. 65536 points"),
        (dict(points=torch.zeros(1, encoding.POSENC_MAX_POINTS + 1, 3), scale=s, embed_dim=12, div_term=torch.zeros(2)), "1 .. 65536 points"),
        (dict(points=x, scale=s, embed_dim=12, div_term=torch.tensor([1.0, 0.0])), "positive and finite"),
        (dict(points=x, scale=s, embed_dim=12, div_term=torch.tensor([1.0, -2.0, 1.0])), "positive and finite"),
        (dict(points=x, scale=s, embed_dim=12, div_term=torch.tensor([math.inf, 1.0])), "positive and finite"),
        (dict(points=x, scale=s, embed_dim=12, div_term=torch.tensor([1.0, math.nan]), max_clouds_per_launch=0), "positive and finite"),
        (dict(points=x, scale=s, embed_dim=12, max_clouds_per_launch=0), "max_clouds_per_launch must be an integer >= 1"),
        (dict(points=x, scale=s, embed_dim=12, max_clouds_per_launch=1.5), "max_clouds_per_launch must be an integer >= 1"),
    ]
    for kwargs, message in bad:
        with pytest.raises(ValueError, match=message):
            enc(**kwargs)
    enc_ok = dict(points=x, scale=s, embed_dim=12, div_term=torch.tensor([1.0, 2.0, -1.0]))  # entries past embed_dim // 6 are not looked at
    if torch.cuda.is_available():  # devices come after the ranges and before max_clouds_per_launch
        with pytest.raises(ValueError, match="same device"):
            enc(x.cuda(), s, 12, max_clouds_per_launch=0)
    for kwargs in (dict(points=x, scale=s, embed_dim=12), dict(points=x, scale=s, embed_dim=7, base=torch.zeros(2, 5, 7)), enc_ok):
        with pytest.raises(hip.NovaHipError, match="runs on the GPU"):  # everything else passed: CPU tensors are refused last
            enc(**kwargs)
    with pytest.raises(hip.NovaHipError, match="runs on the GPU"):
        encoding.DepthAwarePositionalEncoding(12)(x)
    with pytest.raises(ValueError, match="points: expected a tensor"):
        encoding.DepthAwarePositionalEncoding(12)(None)


def abi_checks():
    """Every error of the two entries, in the order include/nova_hip.h states, before any device work. Run by
    test_abi_rejections_in_a_process_without_a_device in a child process that sees no GPU: the calls carry addresses of
    nothing, and a build that lost a check would launch on them; without a device that launch fails with a return code."""
    sys.path.insert(0, ROOT)
    from nova_pointcloud_amd import encoding, hip

    lib = hip.load(check_device=False)
    MB = 1 << 28  # pointers far apart: never dereferenced, rejected first
    x, scale, div, base, out, g, gx, gs, ws = (ctypes.c_void_p(MB * i) for i in range(1, 10))
    fwd = lambda S, N, E, x=x, scale=scale, div=div, base=base, out=out: lib.nova_pointset_posenc(x, scale, div, base, out, S, N, E, None)
    bwd = lambda S, N, E, x=x, scale=scale, div=div, g=g, gx=gx, gs=gs, ws=ws: lib.nova_pointset_posenc_bwd(x, scale, div, g, gx, gs, ws, S, N, E, None)
    err = lib.nova_last_error
    SHAPE, ARG = -2, -1
    for fn in (fwd, bwd):
        for E in (5, 0, -1, encoding.POSENC_MAX_DIM + 1):
            assert fn(70000, 0, E, x=None) == SHAPE and b"NOVA_POSENC_MAX_DIM" in err(), E  # E first
            assert fn(0, 8, E) == SHAPE  # also without clouds
        for N in (0, -1, encoding.POSENC_MAX_POINTS + 1):
            assert fn(70000, N, 12, x=None) == SHAPE and b"NOVA_POSENC_MAX_POINTS" in err(), N  # N before the cloud count
            assert fn(0, N, 12) == SHAPE
        assert fn(65536, 8, 12, x=None) == SHAPE and b"65535" in err()  # shape errors before argument errors
        assert fn(0, 8, 12) == 0 and fn(-3, 65536, 4096) == 0
        assert fn(0, 8, 12, x=None, scale=None, div=None) == 0  # S <= 0 returns before the pointers are looked at
        for name in ("x", "scale", "div"):
            assert fn(2, 8, 12, **{name: None}) == ARG and err().endswith(b"null pointer " + name.encode()), (name, err())
    assert fwd(0, 8, 12, out=None, base=None) == 0 and bwd(0, 8, 12, g=None, gx=None, gs=None, ws=None) == 0
    assert fwd(2, 8, 12, out=None) == ARG and err().endswith(b"null pointer out")
    assert bwd(2, 8, 12, g=None) == ARG and err().endswith(b"null pointer g")
    assert bwd(2, 8, 12, gx=None, gs=None) == ARG and b"both NULL" in err() and b"gx and gs" in err()
    assert bwd(2, 8, 12, gx=None, gs=None, g=None) == ARG and b"null pointer g" in err()  # the null check comes first
    assert bwd(2, 8, 12, ws=None) == ARG and b"workspace ws" in err()
    assert bwd(2, 8, 12, ws=None, gx=None, gs=None) == ARG and b"both NULL" in err()  # in that order
    # an output must not overlap an input or another output: checked last (no call here passes every check: what passes
    # them launches, and these pointers are not memory)
    at = lambda p, off: ctypes.c_void_p(p.value + off)
    for name, p, size in (("x", x, 2 * 8 * 12), ("scale", scale, 12), ("div", div, 2 * 4), ("base", base, 2 * 8 * 12 * 4)):
        assert fwd(2, 8, 12, out=p) == ARG and err().endswith(b"out overlaps the input " + name.encode()), (name, err())
        assert fwd(2, 8, 12, out=at(p, size - 4)) == ARG and err().endswith(b"out overlaps the input " + name.encode())  # its last float
        assert fwd(2, 8, 12, out=at(p, -2 * 8 * 12 * 4 + 4)) == ARG and b"overlaps" in err()  # the last float of out on its first
    assert fwd(70000, 8, 12, out=x) == SHAPE  # a shape error still comes first
    assert fwd(2, 8, 12, out=None, base=x) == ARG and b"null pointer out" in err()
    for name, p in (("x", x), ("scale", scale), ("div", div), ("g", g)):
        assert bwd(2, 8, 12, gx=p) == ARG and err().endswith(b"gx overlaps the input " + name.encode()), (name, err())
        assert bwd(2, 8, 12, gs=p) == ARG and err().endswith(b"gs overlaps the input " + name.encode())
        assert bwd(2, 8, 12, ws=p) == ARG and err().endswith(b"ws overlaps the input " + name.encode())
    assert bwd(2, 8, 12, gs=gx) == ARG and err().endswith(b"gx and gs overlap each other")
    assert bwd(2, 8, 12, ws=gx) == ARG and err().endswith(b"gx and ws overlap each other")
    assert bwd(2, 8, 12, ws=at(gs, 2 * 12 - 4)) == ARG and err().endswith(b"gs and ws overlap each other")  # the last float of gs
    assert bwd(2, 8, 12, gs=gx, ws=None) == ARG and b"workspace" in err()  # before the overlap check
    assert lib.nova_version() == hip.ABI_VERSION  # no version bump
    print("abi checks passed")


def test_abi_rejections_in_a_process_without_a_device():
    env = dict(os.environ, HIP_VISIBLE_DEVICES="-1", CUDA_VISIBLE_DEVICES="-1", ROCR_VISIBLE_DEVICES="-1")
    out = subprocess.run([sys.executable, os.path.abspath(__file__), "--abi-checks"], env=env, capture_output=True, text=True, timeout=300, cwd=ROOT)
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-2000:]
    assert out.stdout.strip().endswith("abi checks passed"), out.stdout[-2000:]


def test_header_constants_and_kernel_shape():
    from nova_pointcloud_amd import encoding, hip

    header = open(os.path.join(ROOT, "include", "nova_hip.h")).read()
    const = lambda name: int(re.search(r"#define " + name + r" (\d+)", header).group(1))
    assert const("NOVA_POSENC_MAX_DIM") == encoding.POSENC_MAX_DIM == 4096
    assert const("NOVA_POSENC_MAX_POINTS") == encoding.POSENC_MAX_POINTS == 65536
    assert const("NOVA_POSENC_CHUNK") == encoding.POSENC_CHUNK == CHUNK
    for needle in ("nova_pointset_posenc", "nova_pointset_posenc_bwd", ":349-389", ":456-458", "EXTENSION", "ascending chunk order",
                   "nova_pointset_soft_cluster_sum_clouds(gs, out3, S, K = 1, stream)", "No atomics"):
        assert needle in header, needle
    for name in ("nova_pointset_posenc", "nova_pointset_posenc_bwd"):
        assert name in hip.SIGNATURES
    source = open(os.path.join(ROOT, "nova_pointcloud_amd", "csrc", "posenc.hip")).read()
    assert "PE_CHUNK = NOVA_POSENC_CHUNK;" in source and "PE_MAX_E = NOVA_POSENC_MAX_DIM;" in source
    assert "PE_MAX_N = NOVA_POSENC_MAX_POINTS;" in source
    assert int(re.search(r"PE_T = (\d+);", source).group(1)) == 256  # the header's four waves per chunk
    assert "#pragma clang fp contract(off)" in source
    code = re.sub(r"//.*", "", source)
    assert "atomic" not in code.lower() and "__sinf" not in code and "__cosf" not in code and "__sincosf" not in code
    # the file defines no summing kernel of its own: the chunk merge is fused_common.h's ordered_sum_kernel, and the cloud sum
    # is the soft cluster pooling's entry point, called from Python
    assert re.findall(r"void (\w+_kernel)\(", code) == ["posenc_fwd_kernel", "posenc_bwd_kernel"]
    assert '#include "fused_common.h"' in code and "ordered_sum(st, ws, gs," in code and code.count("sum_clouds") == 0
    makefile = open(os.path.join(ROOT, "nova_pointcloud_amd", "csrc", "Makefile")).read()
    assert "posenc.hip" in re.search(r"^SRCS := (.*)$", makefile, flags=re.M).group(1).split()
    assert "fast-math" not in makefile and "ffast" not in makefile


def test_module_is_the_reference_module():
    from nova_pointcloud_amd import encoding

    cls = encoding.DepthAwarePositionalEncoding
    params = inspect.signature(cls.__init__).parameters
    assert list(params) == ["self", "embed_dim", "max_points"] and params["max_points"].default == 2048
    assert params["embed_dim"].default is inspect.Parameter.empty
    assert list(inspect.signature(cls.forward).parameters) == ["self", "points", "base"]
    for E in (6, 96, 768, 1024):
        m = cls(E) if E != 96 else cls(E, max_points=4096)
        assert m.embed_dim == E and m.max_points == (4096 if E == 96 else 2048) and m.position_scale == 10000.0
        assert torch.equal(m.dim_div, torch.arange(0, E, 2) / E)
        want = 10000.0 ** (torch.arange(0, E, 2) / E)
        assert m.div_term.dtype == torch.float32 and m.div_term.shape == want.shape
        assert torch.equal(m.div_term.view(torch.int32), want.view(torch.int32))  # bitwise
        assert torch.equal(encoding.reference_div_term(E).view(torch.int32), want.view(torch.int32))
        sd = m.state_dict()
        assert list(sd) == ["scale_x", "scale_y", "scale_z"]
        for key in sd:
            assert sd[key].shape == (1,) and sd[key].dtype == torch.float32 and sd[key].item() == 1.0
        assert [n for n, _ in m.named_parameters()] == ["scale_x", "scale_y", "scale_z"] and not list(m.buffers())
    assert "GPU" in cls.__doc__ and "embed_dim % 6 != 0" in cls.__doc__


# ---- GPU -------------------------------------------------------------------------------------------------------------------


def nan(*shape):
    return torch.full(shape, math.nan, dtype=torch.float32, device="cuda")


def abi_forward(hip, x, scale, div, E, base=None, per=None):
    """nova_pointset_posenc called directly on float32 GPU tensors. out lies between two guard rows in one NaN-filled
    buffer: returns (out [S, N, E], the two guard rows)."""
    S, N = x.shape[:2]
    buf = nan((S * N + 2) * E)
    out = buf[E:(S * N + 1) * E].view(S, N, E)
    per = S if per is None else per
    for s0 in range(0, S, per):
        hip.call("nova_pointset_posenc", x[s0].data_ptr(), scale.data_ptr(), div.data_ptr(), base[s0].data_ptr() if base is not None else None,
                 out[s0].data_ptr(), min(per, S - s0), N, E, hip.stream_ptr())
    return out, torch.cat([buf[:E], buf[(S * N + 1) * E:]])


def abi_backward(hip, x, scale, div, E, g, want_x=True, want_s=True, per=None):
    """nova_pointset_posenc_bwd and the cloud sum called directly, outputs pre-filled with NaN: (gx, gs per cloud, gsum)."""
    S, N = x.shape[:2]
    chunks = (N + CHUNK - 1) // CHUNK
    gx = nan(S, N, 3) if want_x else None
    gs = nan(S, 3) if want_s else None
    ws = nan(S * chunks * 3) if want_s else None
    at = lambda t, s0: t[s0].data_ptr() if t is not None else None
    per = S if per is None else per
    for s0 in range(0, S, per):
        hip.call("nova_pointset_posenc_bwd", x[s0].data_ptr(), scale.data_ptr(), div.data_ptr(), g[s0].data_ptr(), at(gx, s0), at(gs, s0),
                 ws.data_ptr() if want_s else None, min(per, S - s0), N, E, hip.stream_ptr())
    gsum = None
    if want_s:
        gsum = nan(3)
        hip.call("nova_pointset_soft_cluster_sum_clouds", gs.data_ptr(), gsum.data_ptr(), S, 1, hip.stream_ptr())
    return gx, gs, gsum


def same_bits(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


def shapes_of(E):
    """(N, S) of one E: every N of N_CASES with S alternating 1 and 3 at the small E; at the large E the chunk boundaries and
    the single row only (not the full cross product)."""
    ns = N_CASES if E <= 1024 else [1, CHUNK - 1, CHUNK + 1, 2 * CHUNK + 1]
    return [(N, (1, 3)[(n + E) % 2]) for n, N in enumerate(ns)]


@pytest.mark.gpu
@pytest.mark.parametrize("E", E_CASES)
def test_exact_forward(hip, E):
    """Points equal to 0: exactly +0 in the sine channels (scales >= 0) and 1 in the cosine channels, +0 in the tail channels
    (out pre-filled with NaN), nothing written past [S, N, E] (guard rows). With base: bitwise base + encoding formed by a torch float32 add,
    through the ABI and through coordinate_encoding, for random points too."""
    from nova_pointcloud_amd import encoding

    F = E // 6
    want0 = torch.zeros(E)
    want0[1:6 * F:2] = 1.0
    for N, S in shapes_of(E):
        x, scale, div, base, g = (t.cuda() for t in random_case(S, N, E, 100.0, E + N))
        out, guard = abi_forward(hip, torch.zeros_like(x), scale.abs(), div, E)
        assert same_bits(out.cpu(), want0.expand(S, N, E).contiguous()), (E, N, S)
        assert torch.isnan(guard).all(), (E, N, S)
        # a negative scale makes the argument 0 * scale = -0 and its sine -0, as IEEE and torch have it: x's channels here
        signed = abi_forward(hip, torch.zeros_like(x), scale, div, E)[0].cpu()
        assert torch.equal(signed, out.cpu()) and same_bits(signed[:, :, 0:6 * F:6], torch.full((S, N, F), -0.0)), (E, N, S)
        assert same_bits(signed[:, :, 2:6 * F:6], torch.zeros(S, N, F)) and same_bits(signed[:, :, 6 * F:], torch.zeros(S, N, E - 6 * F))
        plain, guard = abi_forward(hip, x, scale, div, E)
        assert torch.isnan(guard).all() and not torch.isnan(plain).any()
        assert same_bits(plain[:, :, 6 * F:].cpu(), torch.zeros(S, N, E - 6 * F)), (E, N, S)  # +0 bit for bit
        based, guard = abi_forward(hip, x, scale, div, E, base)
        assert torch.isnan(guard).all() and same_bits(based, base + plain), (E, N, S)
        assert same_bits(abi_forward(hip, x, scale, div, E, base, per=1)[0], based)  # a second run, one cloud per launch
        fn = encoding.coordinate_encoding(x, scale, E, div_term=div)
        assert same_bits(fn, plain) and same_bits(encoding.coordinate_encoding(x, scale, E, base=base, div_term=div), base + fn), (E, N, S)


@pytest.mark.gpu
@pytest.mark.parametrize("E", [12, 390])
def test_rows_off_eight_bytes_give_the_same_bits(hip, E):
    """out, base and g that start 4 bytes off an 8-byte boundary (E even: the rows would otherwise move as 8-byte pairs) take
    the 4-byte accesses: the same bits, and nothing written outside out."""
    S, N = 3, CHUNK + 1
    x, scale, div, base, g = (t.cuda() for t in random_case(S, N, E, 100.0, 31 + E))
    off = lambda t: torch.cat([t.new_zeros(1), t.flatten()])[1:].view(t.shape)  # the same values, 4 bytes further on
    assert off(base).data_ptr() % 8 == 4 and base.data_ptr() % 8 == 0
    want = abi_forward(hip, x, scale, div, E, base)[0]
    assert same_bits(abi_forward(hip, x, scale, div, E, off(base))[0], want)
    buf = nan((S * N + 2) * E + 1)
    out = buf[E + 1:(S * N + 1) * E + 1].view(S, N, E)
    hip.call("nova_pointset_posenc", x.data_ptr(), scale.data_ptr(), div.data_ptr(), base.data_ptr(), out.data_ptr(), S, N, E, hip.stream_ptr())
    assert out.data_ptr() % 8 == 4 and same_bits(out, want)
    assert torch.isnan(buf[:E + 1]).all() and torch.isnan(buf[(S * N + 1) * E + 1:]).all()
    for a, b in zip(abi_backward(hip, x, scale, div, E, off(g)), abi_backward(hip, x, scale, div, E, g)):
        assert same_bits(a, b)


WORST = {}


def check(name, got, want, bound, where):
    """Every entry within its bound; the worst error / bound of the quantity is kept for the report."""
    assert torch.isfinite(got).all(), (name, where)
    ratio = ((got.double() - want).abs() / bound.expand_as(want)).max().item()
    WORST[name] = max(WORST.get(name, 0.0), ratio)
    print(f"posenc {where} {name}: error / bound {ratio:.4g} (worst so far {WORST[name]:.4g})")
    assert ratio <= 1.0, (name, where, ratio)


@pytest.mark.gpu
@pytest.mark.parametrize("E", E_CASES)
def test_random_forward(hip, E):
    """Random points with |x scale| about 1, 100 and 2^20 (the last catches a native sine), negative and mixed-magnitude
    scales, the reference's table and a custom one, with and without base: every entry of out against restate() within the
    module docstring's cap of 4 ulp (plus half an ulp of the sum with base). Measured on an MI355X, worst error / cap over all
    cases: 0.38 without base (about 1.5 ulp, at |x scale| about 2^20); 0.9994 with base, where the half ulp of the one addition
    is nearly all of the cap (depth-aware positional encoding)."""
    for n, (N, S) in enumerate(shapes_of(E)):
        for m, magnitude in enumerate(MAGNITUDES):
            custom = (n + m) % 3 == 0
            x, scale, div, base, g = random_case(S, N, E, magnitude, 7 * E + 3 * N + m, custom)
            where = f"E={E} N={N} S={S} |x scale|={magnitude:g} {'custom' if custom else 'reference'} table"
            r = restate(x, scale, div, E)
            out, _ = abi_forward(hip, x.cuda(), scale.cuda(), div.cuda(), E)
            check("out", out.cpu(), r["out"], forward_cap(r), where)
            if (n + m) % 2 == 0:
                rb = restate(x, scale, div, E, base)
                out, _ = abi_forward(hip, x.cuda(), scale.cuda(), div.cuda(), E, base.cuda())
                check("out+base", out.cpu(), rb["out"], forward_cap(rb, base), where)


@pytest.mark.gpu
@pytest.mark.parametrize("E", E_CASES)
def test_random_backward(hip, E):
    """gx, the per-cloud gs and the scale gradient against restate() within backward_bounds() of the module docstring, at all
    three magnitudes; at |x scale| about 1 and 100 also against torch autograd of literal_form() on the GPU in float32
    (E % 6 == 0) within loose_bounds(). g is non-zero in the tail channels throughout, and zeroing them changes no bit; gx
    alone and gs alone are bitwise the pair's. Measured on an MI355X, worst error / bound over all cases: gx 0.20, gs 0.13, the
    scale gradient 0.094; against torch, gx 0.046 and the scale gradient 0.022 of the looser bound."""
    F = E // 6
    for n, (N, S) in enumerate(shapes_of(E)):
        for m, magnitude in enumerate(MAGNITUDES):
            custom = (n + m) % 3 == 1
            x, scale, div, base, g = random_case(S, N, E, magnitude, 11 * E + 5 * N + m, custom)
            where = f"E={E} N={N} S={S} |x scale|={magnitude:g} {'custom' if custom else 'reference'} table"
            r = restate(x, scale, div, E, None, g)
            b_gx, b_gs, b_gsum = backward_bounds(r, x, scale, E)
            xc, sc, dc, gc = x.cuda(), scale.cuda(), div.cuda(), g.cuda()
            gx, gs, gsum = abi_backward(hip, xc, sc, dc, E, gc)
            check("gx", gx.cpu(), r["gx"], b_gx, where)
            check("gs", gs.cpu(), r["gs"], b_gs, where)
            check("gsum", gsum.cpu(), r["gsum"], b_gsum, where)
            if m == 0:
                g0 = gc.clone()
                g0[:, :, 6 * F:] = 0
                for a, b in zip((gx, gs, gsum), abi_backward(hip, xc, sc, dc, E, g0, per=1)):
                    assert same_bits(a, b), where  # the tail of g is not read (and the launch split changes nothing)
                assert same_bits(abi_backward(hip, xc, sc, dc, E, gc, want_s=False)[0], gx), where
                only = abi_backward(hip, xc, sc, dc, E, gc, want_x=False)
                assert only[0] is None and same_bits(only[1], gs) and same_bits(only[2], gsum), where
            if E % 6 == 0 and magnitude <= 100.0:
                xl, sl = xc.clone().requires_grad_(True), sc.clone().requires_grad_(True)
                (literal_form(xl, sl, dc, E) * gc).sum().backward()
                l_gx, l_gs, l_gsum = loose_bounds(r, x, scale, E)
                check("gx vs torch", gx.cpu(), xl.grad.cpu().double(), l_gx, where)
                check("gsum vs torch", gsum.cpu(), sl.grad.cpu().double(), l_gsum, where)


def encoded(x, scale, E, base, g, per, div=None):
    """(out, grad of points, grad of scale, grad of base) through coordinate_encoding under sum(out g)."""
    from nova_pointcloud_amd import encoding

    xl, sl, bl = (t.clone().requires_grad_(True) for t in (x, scale, base))
    out = encoding.coordinate_encoding(xl, sl, E, base=bl, div_term=div, max_clouds_per_launch=per)
    out.backward(g)
    return out.detach(), xl.grad, sl.grad, bl.grad


@pytest.mark.gpu
@pytest.mark.parametrize("E", [7, 132, 768])
def test_bitwise_reproducible(hip, E):
    """The output and all gradients bit for bit the same for max_clouds_per_launch 1, 2, S and default, in two runs; per
    cloud for clouds moved to other batch positions and for a cloud run alone (the scale gradient is one sum over the clouds
    in their order, so it is compared through its per-cloud parts)."""
    S, N = 5, 2 * CHUNK + 1
    x, scale, div, base, g = (t.cuda() for t in random_case(S, N, E, 100.0, 23 + E))
    ref = encoded(x, scale, E, base, g, None)
    for per in (1, 2, S, None):
        for a, b in zip(ref, encoded(x, scale, E, base, g, per)):
            assert same_bits(a, b), (E, per)
    raw = abi_backward(hip, x, scale, div, E, g)
    assert same_bits(ref[1], raw[0]) and same_bits(ref[2], raw[2]) and same_bits(ref[3], g)
    perm = torch.tensor([3, 0, 4, 1, 2], device="cuda")
    moved = encoded(x[perm], scale, E, base[perm], g[perm], 2)
    assert same_bits(ref[0][perm], moved[0]) and same_bits(ref[1][perm], moved[1]) and same_bits(ref[3][perm], moved[3])
    raw_moved = abi_backward(hip, x[perm].contiguous(), scale, div, E, g[perm].contiguous(), per=2)
    assert same_bits(raw[1][perm], raw_moved[1]) and same_bits(raw[0][perm], raw_moved[0])
    for s in range(S):
        alone = encoded(x[s:s + 1], scale, E, base[s:s + 1], g[s:s + 1], None)
        assert same_bits(ref[0][s:s + 1], alone[0]) and same_bits(ref[1][s:s + 1], alone[1])
        assert same_bits(alone[2], raw[1][s] + 0.0)  # one cloud: the sum over the clouds is +0 + gs[s]


@pytest.mark.gpu
def test_binding_and_stats(hip):
    """Autograd returns the raw ABI results; a non-contiguous g and a strided points view are accepted; what no input needs is
    not launched and not allocated; no_grad saves nothing and a graph saves the inputs alone; bf16 and f16 inputs get
    gradients of their own dtype."""
    from nova_pointcloud_amd import encoding

    S, N, E = 3, CHUNK + 3, 131
    x, scale, div, base, g = (t.cuda() for t in random_case(S, N, E, 3.0, 5))
    fwd = lambda **kw: encoding.coordinate_encoding(kw.pop("x", x), kw.pop("scale", scale), E, div_term=div, **kw)
    delta = lambda before: {k: encoding.stats[k] - before[k] for k in before}
    raw_out = abi_forward(hip, x, scale, div, E, base)[0]
    raw = abi_backward(hip, x, scale, div, E, g)
    got = encoded(x, scale, E, base, g, 2, div)
    assert same_bits(got[0], raw_out) and same_bits(got[1], raw[0]) and same_bits(got[2], raw[2]) and same_bits(got[3], g)
    # a non-contiguous g
    wide = torch.randn(S, N, 2 * E, generator=torch.Generator().manual_seed(9)).cuda()
    g_nc = wide[:, :, ::2]
    assert not g_nc.is_contiguous()
    raw_nc = abi_backward(hip, x, scale, div, E, g_nc.contiguous())
    got = encoded(x, scale, E, base, g_nc, None, div)
    assert same_bits(got[1], raw_nc[0]) and same_bits(got[2], raw_nc[2])
    # a strided view of wider rows as the points
    rows = torch.randn(S, N, 6, generator=torch.Generator().manual_seed(8)).cuda().requires_grad_(True)
    out = fwd(x=rows[:, :, :3])
    out.backward(g)
    raw_v = abi_backward(hip, rows.detach()[:, :, :3].contiguous(), scale, div, E, g)
    assert same_bits(out.detach(), abi_forward(hip, rows.detach()[:, :, :3].contiguous(), scale, div, E)[0])
    assert same_bits(rows.grad[:, :, :3].contiguous(), raw_v[0]) and (rows.grad[:, :, 3:] == 0).all()
    # stats: only base needs a gradient: no backward kernel at all, and its gradient is g
    bl = base.clone().requires_grad_(True)
    before = dict(encoding.stats)
    fwd(base=bl, max_clouds_per_launch=2).backward(g)
    assert delta(before) == {"forward_launches": 2, "point_grad_launches": 0, "scale_grad_launches": 0, "cloud_sum_launches": 0}
    assert same_bits(bl.grad, g)
    # only scale needs one: the gx stores are skipped (gx is not allocated: the backward's allocations stay far below its size)
    big = torch.randn(1, 65536, 3, generator=torch.Generator().manual_seed(3)).cuda()
    sl = scale.clone().requires_grad_(True)
    out = encoding.coordinate_encoding(big, sl, 6, max_clouds_per_launch=1)
    gb = torch.ones_like(out)
    torch.cuda.synchronize()
    before, allocated = dict(encoding.stats), torch.cuda.memory_allocated()
    torch.cuda.reset_peak_memory_stats()
    out.backward(gb)
    torch.cuda.synchronize()
    assert delta(before) == {"forward_launches": 0, "point_grad_launches": 0, "scale_grad_launches": 1, "cloud_sum_launches": 1}
    assert torch.cuda.max_memory_allocated() - allocated < big.numel() * 4 // 2  # gx alone would be 768 KiB
    assert same_bits(sl.grad, abi_backward(hip, big, scale, encoding._reference_table(6, big.device), 6, gb, want_x=False)[2])
    # only the points need one: no scale gradient, no cloud sum
    xl = x.clone().requires_grad_(True)
    before = dict(encoding.stats)
    fwd(x=xl, max_clouds_per_launch=2).backward(g)
    assert delta(before) == {"forward_launches": 2, "point_grad_launches": 2, "scale_grad_launches": 0, "cloud_sum_launches": 0}
    assert same_bits(xl.grad, raw[0])
    # what autograd keeps: nothing without a graph, the inputs alone with one
    kept = []
    with torch.autograd.graph.saved_tensors_hooks(lambda t: kept.append(tuple(t.shape)) or t, lambda t: t):
        with torch.no_grad():
            fwd(x=x.clone().requires_grad_(True), base=base)
        assert kept == []
        fwd(base=base)  # nothing requires a gradient
        assert kept == []
        fwd(x=x.clone().requires_grad_(True), base=base)
    assert sorted(kept) == sorted([(S, N, 3), (3,), tuple(div.shape)]), kept
    # mixed dtypes
    for dtype in (torch.bfloat16, torch.float16):
        xl, sl, bl = x.to(dtype).requires_grad_(True), scale.to(dtype).requires_grad_(True), base.to(dtype).requires_grad_(True)
        out = encoding.coordinate_encoding(xl, sl, E, base=bl, div_term=div)
        assert out.dtype == torch.float32
        out.backward(g)
        assert xl.grad.dtype == dtype and sl.grad.dtype == dtype and bl.grad.dtype == dtype
        x32, s32, b32 = xl.detach().float(), sl.detach().float(), bl.detach().float()
        raw16 = abi_backward(hip, x32, s32, div, E, g)
        assert same_bits(out.detach(), abi_forward(hip, x32, s32, div, E, b32)[0])
        assert torch.equal(xl.grad, raw16[0].to(dtype)) and torch.equal(sl.grad, raw16[2].to(dtype)) and torch.equal(bl.grad, g.to(dtype))
    with pytest.raises(hip.NovaHipError, match="runs on the GPU"):
        encoding.coordinate_encoding(x.cpu(), scale.cpu(), E)


@pytest.mark.gpu
def test_module_on_the_gpu(hip):
    """Each of scale_x / y / z.grad is the matching entry of the functional's scale gradient, bitwise; load_state_dict
    round-trips; E = 1024 (not a multiple of 6) runs with zero tail channels; the table is cached per device."""
    from nova_pointcloud_amd import encoding

    for E in (768, 1024):
        S, N = 2, CHUNK + 1
        x, scale, div, base, g = (t.cuda() for t in random_case(S, N, E, 3.0, E))
        m = encoding.DepthAwarePositionalEncoding(E).cuda()
        with torch.no_grad():
            for p, v in zip((m.scale_x, m.scale_y, m.scale_z), scale):
                p.fill_(v)
        xl, bl = x.clone().requires_grad_(True), base.clone().requires_grad_(True)
        out = m(xl, bl)
        out.backward(g)
        want = encoded(x, scale, E, base, g, None)
        assert same_bits(out.detach(), want[0]) and same_bits(xl.grad, want[1]) and same_bits(bl.grad, want[3])
        for c, p in enumerate((m.scale_x, m.scale_y, m.scale_z)):
            assert p.grad.shape == (1,) and same_bits(p.grad, want[2][c:c + 1]), (E, c)
        assert same_bits(m(x), abi_forward(hip, x, scale, reference_table(E)[:E // 6].cuda(), E)[0])
        assert (m(x)[:, :, 6 * (E // 6):] == 0).all() and m.div_term.device.type == "cpu"
        assert m._table(x.device) is m._table(x.device) and list(m._device_tables) == [x.device]
        fresh = encoding.DepthAwarePositionalEncoding(E)
        fresh.load_state_dict(m.state_dict())
        assert list(fresh.state_dict()) == ["scale_x", "scale_y", "scale_z"]
        assert same_bits(fresh.cuda()(x, base), out.detach())
    r = restate(x.cpu(), scale.cpu(), reference_table(1024), 1024, base.cpu())
    check("module out", out.detach().cpu(), r["out"], forward_cap(r, base.cpu()), "E=1024 module")


if __name__ == "__main__" and sys.argv[1:] == ["--abi-checks"]:
    abi_checks()
