"""Cases, float64 restatements and bounds of tests/test_gpu_row_contract.py, and the checks on them that need no GPU.

The GPU file holds `nova_row_norm` (csrc/rownorm.h, csrc/rowops.hip), `nova_row_norm_bwd` (csrc/rownorm_bwd.hip) and the
glue kernels around them to ELEMENTWISE bounds against float64 on the stored values. What decides whether those tests can
fail at all is checked here, on the CPU and without the library:

  * the bounds come from the kernels' stated arithmetic, not from running them: a numpy float32 restatement of the same
    operation order (per-lane sums in chunk order, a pairwise tree over the 64 lanes) stays under half of them;
  * the inputs have teeth: a forward that ignores or swaps `eps`, drops the last 16-byte chunk of a row from the
    statistics, or exchanges scale and shift lands more than 4 bounds from the reference on the family built for it;
  * the argument checks of the forward refuse bad calls before any launch (fake pointers, no GPU).

Notation. u_T is the unit roundoff of the storage type - 2^-24 (f32), 2^-8 (bf16), 2^-11 (f16): rounding to nearest is within
u_T of a value at the BOTTOM of its binade, half of that at the top. G = gamma (1 + scale) gate. A_y is y with every factor
and term replaced by its absolute value, (((|x| + |mean|) rstd |gamma| + |beta|)(1 + |scale|) + |shift|) |gate| + |res|.

Forward:   |y - ref| <= u_T |ref| + (D/64 + 8) 2^-24 mean|x| rstd |G| + 8 2^-24 A_y
  the middle term is the f32 mean (each lane adds up to D/64 chunk sums, then six wave steps and the division), the last one
  the half dozen f32 operations per element and rsqrtf.
Backward:  |dx - ref| <= u_T |ref| + (D/64 + 8) 2^-23 A_dx,  A_dx = rstd (|dn| + mean|dn| + |n| mean(|dn| |n|))
           d_scale, d_shift, d_gate: u_T |ref| + 8 2^-24 A

Row families (fixed seeds, stored in the dtype under test; the reference is float64 on the stored values):
  unit    N(0,1)
  offset  |x - mean| << |mean|. f32: 100 + 0.01 N(0,1). bf16 / f16: the storage type keeps 8 / 11 significand bits, so the
          ratio spread / offset cannot go below 7 ulps / 1 for 8 distinct values whatever the offset: what was chosen is the
          f32 offset, 100, with a spread of two ulps of the storage type there (ulp = 0.5 for bf16, 0.0625 for f16) -
          x = 100 + ulp * round(2 N(0,1)) - and the first 8 elements of every row a ladder of 8 adjacent storage values,
          100 + ulp * (-4 .. 3), so that every row has its 8 distinct values at any width.
  tiny    1e-3 N(0,1): the variance is about 1e-6 and `eps` decides rstd
  const   one repeated value per row (0.3 + 0.1 (row mod 7), not exact in binary): variance 0, the output is the beta / shift /
          res path alone, and what an inexact f32 mean leaves of x - mean is multiplied by eps^-1/2
  spike   0.01 N(0,1) with the last element 1000: the row's last chunk carries the statistics
  scales  row i scaled by 10^(i mod 7 - 3): small rows next to large ones, which a global norm hides

u_T |ref| is `rounding` below: in f16 it stops shrinking at 2^-25 under the smallest normal 2^-14, where the values are 2^-24 apart (the
missing term the GPU runs found: outputs and gradients of a few 1e-6 on `scales` rows, 9 x the bound without it; bf16 and f32 underflow
near 1e-38, out of reach).

The margin of the restatement, as measured here (worst over all widths, families and both eps; per kind in the `[contract-cpu]` lines):
  forward, f32: 0.499 (kind `everything`, the spike element itself, D 1028: 4.4 of the 9 f32 ulps the bound gives it; 0.27 to 0.36 for the
      other kinds). For f32 rows this is the assertion the bound was given with, <= 0.5 of the whole bound.
  forward, bf16 | f16: 0.996 | 0.998 of the whole bound after rounding to the storage type, 0.31 | 0.36 before it against the bound of f32
      rows. A 16-bit result cannot stay under half of its WHOLE bound: the first term, u_T |ref|, IS the rounding to the storage type, so
      the correctly rounded exact result already sits at up to u_T |ref| / (u_T |ref| + rest) of it - about 1/2 at the top of a binade,
      towards 1 at the bottom - and among a few thousand elements one always lies near a bottom. No choice of inputs changes that. So the
      half-bound margin is asserted where it says something, in all three dtypes: the UNROUNDED f32 restatement against the bound of f32
      rows (2^-24 |ref| + the same other terms) <= 0.5; and the rounded result against its whole bound <= 1 (<= 0.5 for f32, where the
      two statements coincide). Together: a 16-bit result is within u_T |ref| of an f32 value that uses half of the remaining terms.
  backward, the same split: dx 0.17 (f32), 0.15 | 0.15 unrounded; d_gate 0.48, d_scale 0.45, d_shift 0.11 (f32: one or two f32 products
      of n against 8 ulps; exact for d_shift without a gate).
"""
import ctypes

import numpy as np
import pytest
import torch

F64 = torch.float64
DTYPES = [torch.float32, torch.bfloat16, torch.float16]
U_T = {torch.float32: 2.0 ** -24, torch.bfloat16: 2.0 ** -8, torch.float16: 2.0 ** -11}
VEC = {torch.float32: 4, torch.bfloat16: 8, torch.float16: 8}  # values per 16-byte chunk
WIDTHS = {torch.float32: [4, 132, 1024, 1028, 1536, 2048], torch.bfloat16: [8, 136, 1024, 1032, 1536, 2048],
          torch.float16: [8, 136, 1024, 1032, 1536, 2048]}
FAMILIES = ["unit", "offset", "tiny", "const", "spike", "scales"]
BWD_FAMILIES = ["unit", "offset", "tiny", "scales"]
EPS = [1e-5, 1e-6]
ROWS = 37
ROW_COUNTS = [1, 3, 4, 5, 37]   # around the four-rows-per-workgroup edge
BIG_ROWS, BIG_WIDTHS = 1025, [1024, 2048]  # one width per NIT form: 2 | 4 chunks per lane (16-bit), 4 | 8 (f32)
GATHER = [5, 0, 36, 36, 7]
CANARY = -1536.0  # exact in f32, bf16 and f16
SUBNORMAL = {torch.float32: 0.0, torch.bfloat16: 0.0, torch.float16: 2.0 ** -25}  # half the spacing below f16's smallest normal 2^-14
OFFSET, OFFSET_ULP = 100.0, {torch.bfloat16: 0.5, torch.float16: 0.0625}
NORM_KINDS = {  # tests/test_gpu_train_kernels.py (compared below)
    "vit_post_norm": dict(affine=True, ss=False, gate=False, res=True),
    "adaln_modulate": dict(affine=False, ss=True, gate=False, res=False),
    "gated_norm": dict(affine=True, ss=False, gate=True, res=True),
    "plain": dict(affine=False, ss=False, gate=False, res=False),
    "everything": dict(affine=True, ss=True, gate=True, res=True),
}


def rounding(ref, dtype):
    """The first term of every bound, u_T |ref|: rounding to nearest in the storage type. It is u_T |ref| in the type's normal range; below
    f16's smallest normal, 2^-14, the values are 2^-24 apart whatever their size, so the term stops shrinking at 2^-25 there (which is
    u_T * 2^-14: the two expressions meet). bf16 and f32 underflow near 1e-38, out of every case's reach."""
    return (U_T[dtype] * ref.abs()).clamp_min(SUBNORMAL[dtype])


def mod_layout(D, dtype):
    """[pad | shift | gate | pad | scale]: shift comes before scale, the stride exceeds the columns used."""
    vec = VEC[dtype]
    return dict(mod_ld=5 * D + vec, shift_off=vec, gate_off=vec + D, scale_off=vec + 4 * D)


def family_rows(family, dtype, rows, D):
    g = torch.Generator().manual_seed(100003 * FAMILIES.index(family) + 17 * D + DTYPES.index(dtype))
    z = torch.randn(rows, D, generator=g, dtype=F64)
    i = torch.arange(rows, dtype=F64)[:, None]
    if family == "unit":
        x = z
    elif family == "offset":
        if dtype == torch.float32:
            x = OFFSET + 0.01 * z
        else:
            ulp = OFFSET_ULP[dtype]
            x = OFFSET + ulp * torch.round(2 * z)
            x[:, :8] = OFFSET + ulp * (torch.arange(8, dtype=F64) - 4)
    elif family == "tiny":
        x = 1e-3 * z
    elif family == "const":
        x = (0.3 + 0.1 * (i % 7)).expand(rows, D).clone()
    elif family == "spike":
        x = 0.01 * z
        x[:, -1] = 1000.0
    elif family == "scales":
        x = z * 10.0 ** (i % 7 - 3)
    else:
        raise KeyError(family)
    return x.to(dtype)


def make_case(dtype, kind, D, family, rows=ROWS):
    """Everything one call reads, on the CPU in the storage types the kernel gets (gamma / beta are f32 in every mode)."""
    x = family_rows(family, dtype, rows, D)
    g = torch.Generator().manual_seed(7 + 31 * D + DTYPES.index(dtype))
    lay = mod_layout(D, dtype)
    c = dict(dtype=dtype, kind=kind, D=D, family=family, rows=rows, x=x, has=NORM_KINDS[kind], **lay)
    c["gamma"] = (1 + 0.2 * torch.randn(D, generator=g)).float()
    c["beta"] = (0.2 * torch.randn(D, generator=g)).float()
    c["mod"] = (0.5 * torch.randn(rows, lay["mod_ld"], generator=g)).to(dtype)
    c["res"] = torch.randn(rows, D, generator=g).to(dtype)
    c["dy"] = torch.randn(rows, D, generator=g).to(dtype)
    return c


def _terms(c, rows, swap=False):
    """float64 gamma, beta, scale, shift, gate, res of the first `rows` OUTPUT rows (None where the kind has none)."""
    D = c["D"]
    col = lambda off: c["mod"][:rows, off:off + D].to(F64)
    so, bo = (c["shift_off"], c["scale_off"]) if swap else (c["scale_off"], c["shift_off"])
    has = c["has"]
    return (c["gamma"].to(F64) if has["affine"] else None, c["beta"].to(F64) if has["affine"] else None,
            col(so) if has["ss"] else None, col(bo) if has["ss"] else None, col(c["gate_off"]) if has["gate"] else None,
            c["res"][:rows].to(F64) if has["res"] else None)


def _stats(x, D, eps, drop=0):
    """mean, rstd of float64 rows; drop: the last `drop` elements contribute nothing to either sum (a load that never came)."""
    keep = torch.ones(D, dtype=F64)
    if drop:
        keep[D - drop:] = 0
    mean = (x * keep).sum(1, keepdim=True) / D
    var = (((x - mean) ** 2) * keep).sum(1, keepdim=True) / D
    return mean, 1.0 / torch.sqrt(var + eps)


def forward_ref(c, eps, rows=None, src=None, swap=False, drop_last_chunk=False, x=None):
    """float64 y of nova_row_norm on the stored values, its bound, and n. rows: the first `rows` rows; src: gathered source rows
    (res and mod stay indexed by OUTPUT row); swap: scale and shift exchanged; drop_last_chunk: statistics without the last chunk."""
    D, dtype = c["D"], c["dtype"]
    x = (c["x"] if x is None else x).to(F64)
    x = x[src] if src is not None else x[: (c["rows"] if rows is None else rows)]
    R = x.shape[0]
    gamma, beta, scale, shift, gate, res = _terms(c, R, swap)
    mean, rstd = _stats(x, D, eps, VEC[dtype] if drop_last_chunk else 0)
    n = (x - mean) * rstd
    y, A, G = n, (x.abs() + mean.abs()) * rstd, torch.ones_like(x)
    if gamma is not None:
        y, A, G = y * gamma + beta, A * gamma.abs() + beta.abs(), G * gamma
    if scale is not None:
        y, A, G = y * (1 + scale) + shift, A * (1 + scale.abs()) + shift.abs(), G * (1 + scale)
    if gate is not None:
        y, A, G = y * gate, A * gate.abs(), G * gate
    if res is not None:
        y, A = y + res, A + res.abs()
    arith = (D / 64 + 8) * 2.0 ** -24 * x.abs().mean(1, keepdim=True) * rstd * G.abs() + 8 * 2.0 ** -24 * A
    return dict(y=y, bound=rounding(y, dtype) + arith, f32=2.0 ** -24 * y.abs() + arith, n=n)


def backward_ref(c, eps, rows=None):
    """float64 restatement of the formulas at the head of csrc/rownorm_bwd.hip: dx and the modulation gradients with their bounds."""
    D, dtype = c["D"], c["dtype"]
    R = c["rows"] if rows is None else rows
    x, dy = c["x"][:R].to(F64), c["dy"][:R].to(F64)
    gamma, beta, scale, shift, gate, _ = _terms(c, R)
    mean, rstd = _stats(x, D, eps)
    n = (x - mean) * rstd
    u1, A_u1 = (n * gamma + beta, n.abs() * gamma.abs() + beta.abs()) if gamma is not None else (n, n.abs())
    small = 8 * 2.0 ** -24
    out, g = {}, dy
    if gate is not None:
        u2, A_u2 = (u1 * (1 + scale) + shift, A_u1 * (1 + scale.abs()) + shift.abs()) if scale is not None else (u1, A_u1)
        out["d_gate"] = (dy * u2, dy.abs() * A_u2)
        g = g * gate
    if scale is not None:
        out["d_shift"] = (g, g.abs())
        out["d_scale"] = (g * u1, g.abs() * A_u1)
        g = g * (1 + scale)
    dn = g * gamma if gamma is not None else g
    dx = rstd * (dn - dn.mean(1, keepdim=True) - n * (dn * n).mean(1, keepdim=True))
    A_dx = rstd * (dn.abs() + dn.abs().mean(1, keepdim=True) + n.abs() * (dn.abs() * n.abs()).mean(1, keepdim=True))
    r = {k: dict(y=v, f32=2.0 ** -24 * v.abs() + small * A, bound=rounding(v, dtype) + small * A) for k, (v, A) in out.items()}
    arith = (D / 64 + 8) * 2.0 ** -23 * A_dx
    r["dx"] = dict(y=dx, f32=2.0 ** -24 * dx.abs() + arith, bound=rounding(dx, dtype) + arith)
    r["n"] = n
    return r


def worst(got, ref, key="bound"):
    """max |got - ref| / bound over all elements; anything not finite counts as infinitely far."""
    diff = (got.to(F64) - ref["y"]).abs()
    ratio = torch.where(diff == 0, torch.zeros_like(diff), diff / ref[key])  # an exact result meets a bound of zero
    return float(torch.nan_to_num(ratio, nan=float("inf")).max())


def apart(a, b, bound):
    """Per row the largest |a - b| / bound, and of those the smallest: every row tells the two apart by that much."""
    return float(((a - b).abs() / bound).amax(1).min())


# ---------------------------------------------------------------------------------------------------------------------
# the float32 restatement: one wave per row, lane l holds chunks l, 64 + l, ..., NIT chunks per lane
# ---------------------------------------------------------------------------------------------------------------------
f32 = np.float32


def _lanes(a, D, vec):
    """[rows, D] -> [rows, NIT, 64, vec] in the kernel's lane <-> element mapping, and the mask of real elements."""
    rows = a.shape[0]
    nit = -(-(D // vec) // 64)
    pad = np.zeros((rows, nit * 64 * vec), dtype=a.dtype)
    pad[:, :D] = a
    real = np.zeros(nit * 64 * vec, dtype=bool)
    real[:D] = True
    return pad.reshape(rows, nit, 64, vec), real.reshape(nit, 64, vec)


def _tree(s):
    while s.shape[1] > 1:
        s = s[:, 0::2] + s[:, 1::2]
    return s  # [rows, 1]


def _lane_sum4(values):
    """sum += (v0 + v1) + (v2 + v3) for every group of four, chunk by chunk, then the wave tree."""
    rows, nit, _, vec = values.shape
    s = np.zeros((rows, 64), dtype=f32)
    for it in range(nit):
        for k in range(vec // 4):
            v = values[:, it, :, 4 * k:4 * k + 4]
            s = s + ((v[..., 0] + v[..., 1]) + (v[..., 2] + v[..., 3]))
    return _tree(s)


def _np32(t):
    return None if t is None else t.to(F64).numpy().astype(f32)


def emulate_forward(c, eps):
    """csrc/rownorm.h in numpy float32: the unrounded f32 result as float64 [rows, D]."""
    D, vec, rows = c["D"], VEC[c["dtype"]], c["rows"]
    gamma, beta, scale, shift, gate, res = (_np32(t) for t in _terms(c, rows))
    x = _np32(c["x"])
    xl, real = _lanes(x, D, vec)
    mean = _lane_sum4(xl) / f32(D)
    sq = np.zeros((rows, 64), dtype=f32)
    for it in range(xl.shape[1]):
        for j in range(vec):
            d = xl[:, it, :, j] - mean
            sq = sq + np.where(real[it, :, j], d * d, f32(0))
    rstd = (1.0 / np.sqrt((_tree(sq) / f32(D) + f32(eps)).astype(np.float64))).astype(f32)  # rsqrtf: correctly rounded here
    v = (x - mean) * rstd
    if gamma is not None:
        v = v * gamma + beta
    if scale is not None:
        v = v * (f32(1) + scale) + shift
    if gate is not None:
        v = v * gate
    if res is not None:
        v = v + res
    assert v.dtype == f32
    return torch.from_numpy(v.astype(np.float64))


def emulate_backward(c, eps):
    """csrc/rownorm_bwd.hip in numpy: f64 statistics, n rounded to f32 once, everything after it in f32, in the kernel's order."""
    D, vec, rows = c["D"], VEC[c["dtype"]], c["rows"]
    gamma, beta, scale, shift, gate, _ = (_np32(t) for t in _terms(c, rows))
    x64 = c["x"].to(F64)
    mean, rstd64 = _stats(x64, D, eps)
    n = ((x64 - mean) * rstd64).numpy().astype(f32)
    rstd = rstd64.numpy().astype(f32)
    g = _np32(c["dy"])
    u1 = n * gamma + beta if gamma is not None else n
    out = {}
    if gate is not None:
        u2 = u1 * (f32(1) + scale) + shift if scale is not None else u1
        out["d_gate"] = g * u2
        g = g * gate
    if scale is not None:
        out["d_shift"] = g
        out["d_scale"] = g * u1
        g = g * (f32(1) + scale)
    dn = g * gamma if gamma is not None else g
    dl, _ = _lanes(dn, D, vec)
    nl, _ = _lanes(n, D, vec)
    inv_d = f32(1.0 / D)
    m1, m2 = _lane_sum4(dl) * inv_d, _lane_sum4(dl * nl) * inv_d
    out["dx"] = (dn - m1 - n * m2) * rstd
    assert all(v.dtype == f32 for v in out.values())
    return {k: torch.from_numpy(v.astype(np.float64)) for k, v in out.items()}


def stored(t, dtype):
    return t.to(dtype).to(F64)


def margins(emu, ref, dtype):
    """(rounded to the storage type against the bound, unrounded against the bound of f32 rows: u_T = 2^-24, the same other terms)."""
    return worst(stored(emu, dtype), ref), worst(emu, ref, "f32")


def assert_margins(emu, ref, dtype, what):
    whole, as_f32 = margins(emu, ref, dtype)
    assert as_f32 <= 0.5, (what, "unrounded, against the f32 bound", as_f32)
    assert whole <= (0.5 if dtype == torch.float32 else 1.0), (what, "rounded, against the bound", whole)
    return whole, as_f32


# ---------------------------------------------------------------------------------------------------------------------
# the CPU tests
# ---------------------------------------------------------------------------------------------------------------------
def test_kinds_are_the_training_tests_kinds():
    import test_gpu_train_kernels as T

    assert NORM_KINDS == T.NORM_KINDS


@pytest.mark.parametrize("dtype", DTYPES)
def test_families_are_what_they_say(dtype):
    for D in WIDTHS[dtype]:
        for family in FAMILIES:
            x = family_rows(family, dtype, ROWS, D)
            assert x.dtype == dtype and x.shape == (ROWS, D) and torch.isfinite(x.float()).all()
            assert torch.equal(x, family_rows(family, dtype, ROWS, D))  # fixed seed
            x64 = x.to(F64)
            if family == "offset" and D >= 8:
                assert min(len(torch.unique(r)) for r in x64) >= 8
                assert float(((x64 - x64.mean(1, keepdim=True)).abs().amax(1) / x64.mean(1).abs()).max()) < 0.05
            if family == "tiny" and D >= 132:
                assert 0.5e-6 < float(x64.var(1, unbiased=False).mean()) < 2e-6
            if family == "const":
                assert all(len(torch.unique(r)) == 1 for r in x64)
            if family == "spike":
                assert bool((x64[:, -1] == 1000).all())
    assert float(torch.tensor(CANARY).to(dtype)) == CANARY


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("kind", sorted(NORM_KINDS))
def test_forward_restatement_in_f32_stays_under_half_the_bound(dtype, kind):
    top = [0.0, 0.0]
    for D in WIDTHS[dtype]:
        for family in FAMILIES:
            c = make_case(dtype, kind, D, family)
            for eps in EPS:
                m = assert_margins(emulate_forward(c, eps), forward_ref(c, eps), dtype, (D, family, eps))
                top = [max(a, b) for a, b in zip(top, m)]
    print(f"\n[contract-cpu] forward restatement {dtype} {kind}: rounded {top[0]:.3f}, unrounded against the f32 bound {top[1]:.3f}")


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("kind", sorted(NORM_KINDS))
def test_backward_restatement_in_f32_stays_under_half_the_bounds(dtype, kind):
    top = {}
    for D in WIDTHS[dtype]:
        for family in BWD_FAMILIES:
            c = make_case(dtype, kind, D, family)
            eps = eps_of(kind)
            ref, emu = backward_ref(c, eps), emulate_backward(c, eps)
            assert set(emu) == set(ref) - {"n"}
            for name, e in emu.items():
                m = assert_margins(e, ref[name], dtype, (name, D, family))
                top[name] = [max(a, b) for a, b in zip(top.get(name, [0.0, 0.0]), m)]
    print(f"\n[contract-cpu] backward restatement {dtype} {kind}: " + ", ".join(f"{k} {v[0]:.3f} / {v[1]:.3f}" for k, v in sorted(top.items())))


def eps_of(kind):
    """The engine's: 1e-6 for the AdaLN modulate, 1e-5 for the norms with an affine."""
    return 1e-6 if kind == "adaln_modulate" else 1e-5


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("kind", sorted(NORM_KINDS))
def test_tiny_rows_tell_the_two_eps_apart(dtype, kind):
    """A forward that ignores eps, or takes the engine's other one, is more than 4 bounds away on every `tiny` row (on `unit`
    rows it would pass most 16-bit bounds: rstd moves by 5e-6 relative)."""
    for D in WIDTHS[dtype]:
        c = make_case(dtype, kind, D, "tiny")
        a, b = forward_ref(c, 1e-5), forward_ref(c, 1e-6)
        assert apart(a["y"], b["y"], torch.maximum(a["bound"], b["bound"])) > 4, D


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("kind", sorted(NORM_KINDS))
def test_spike_rows_tell_a_dropped_last_chunk(dtype, kind):
    for D in WIDTHS[dtype]:
        c = make_case(dtype, kind, D, "spike")
        for eps in EPS:
            a, b = forward_ref(c, eps), forward_ref(c, eps, drop_last_chunk=True)
            assert apart(a["y"], b["y"], torch.maximum(a["bound"], b["bound"])) > 4, (D, eps)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("kind", ["adaln_modulate", "everything"])
@pytest.mark.parametrize("family", FAMILIES)
def test_every_family_tells_scale_and_shift_exchanged(dtype, kind, family):
    for D in WIDTHS[dtype]:
        c = make_case(dtype, kind, D, family)
        for eps in EPS:
            a, b = forward_ref(c, eps), forward_ref(c, eps, swap=True)
            assert apart(a["y"], b["y"], torch.maximum(a["bound"], b["bound"])) > 4, (D, eps)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("kind", ["vit_post_norm", "gated_norm", "everything", "adaln_modulate"])
def test_gather_case_tells_res_and_mod_indexed_by_source_row(dtype, kind):
    """`in` is indexed by source row, `res` and `mod` by output row: a reference that gathers them too is far away."""
    for D in WIDTHS[dtype]:
        c = make_case(dtype, kind, D, "unit")
        a = forward_ref(c, 1e-5, src=GATHER)
        wrong = dict(c, mod=c["mod"][GATHER], res=c["res"][GATHER])
        b = forward_ref(wrong, 1e-5, src=GATHER)
        assert apart(a["y"], b["y"], torch.maximum(a["bound"], b["bound"])) > 4, D


# ---------------------------------------------------------------------------------------------------------------------
# refusals: the argument checks run before any device work, so fake pointers do and no GPU is needed
# ---------------------------------------------------------------------------------------------------------------------
def _lib():
    from nova_pointcloud_amd import hip

    return hip, hip.load(check_device=False)


P = [ctypes.c_void_p(4096 * (i + 1)) for i in range(8)]  # never dereferenced


def _row_norm(lib, *, D=128, dtype, gamma=None, beta=None, mod=None, mod_ld=0, scale_off=-1, shift_off=-1, gate_off=-1, rows=5):
    return lib.nova_row_norm(P[0], P[1], gamma, beta, mod, mod_ld, scale_off, shift_off, gate_off, None, None, rows, D, 1e-5, dtype, None)


def test_row_norm_refuses_bad_arguments_before_any_launch():
    hip, lib = _lib()
    err = lambda: lib.nova_last_error().decode()
    SHAPE, ARG = -2, -1
    for dtype in (hip.F32, hip.BF16, hip.F16):
        vec = 4 if dtype == hip.F32 else 8
        assert _row_norm(lib, D=2056, dtype=dtype) == SHAPE and "D=2056 unsupported" in err()
        assert _row_norm(lib, gamma=P[2], dtype=dtype) == ARG and "gamma/beta must come together" in err()
        assert _row_norm(lib, beta=P[3], dtype=dtype) == ARG and "gamma/beta must come together" in err()
        for bad in (dict(scale_off=vec // 2, shift_off=128), dict(scale_off=0, shift_off=128 + vec // 2), dict(gate_off=vec + 1)):
            assert _row_norm(lib, mod=P[4], mod_ld=512, dtype=dtype, **bad) == SHAPE, bad
            assert f"modulation offsets must be multiples of {vec}" in err()
        assert _row_norm(lib, mod=P[4], mod_ld=512 + vec // 2, scale_off=0, shift_off=128, dtype=dtype) == SHAPE
        assert "multiples of" in err()
    for dtype in (hip.BF16, hip.F16):
        assert _row_norm(lib, D=12, dtype=dtype) == SHAPE and "D=12 unsupported (need D % 8 == 0" in err()
    assert _row_norm(lib, D=12, dtype=hip.F32, rows=0) == 0  # nothing to do is not an error


def test_row_norm_refuses_a_modulation_term_past_the_row_stride():
    """off + D > mod_ld would read past the modulation row (into the next row, or past the buffer on the last one). The backward
    always refused it; the forward, the chain and the two-launch form of nova_adaln_fc1 refuse it with the same message."""
    hip, lib = _lib()
    err = lambda: lib.nova_last_error().decode()
    D = 128
    for dtype in (hip.F32, hip.BF16, hip.F16):
        vec = 4 if dtype == hip.F32 else 8
        ld = 3 * D
        ok_off = ld - D
        for name in ("scale_off", "shift_off", "gate_off"):
            args = dict(scale_off=0, shift_off=D, gate_off=ok_off)
            args[name] = ok_off + vec
            assert _row_norm(lib, mod=P[4], mod_ld=ld, dtype=dtype, **args) == -2, (name, dtype)
            assert f"row_norm: modulation offset {ok_off + vec} + D {D} exceeds the row stride {ld}" in err()
        # the same sentence as the backward's
        bwd = lib.nova_row_norm_bwd(P[0], P[1], None, None, P[4], ld, 0, D, ok_off + vec, P[2], P[5], None, None, 4, 5, D, 1e-5, dtype, None)
        assert bwd == -2 and f"row_norm_bwd: modulation offset {ok_off + vec} + D {D} exceeds the row stride {ld}" in err()
    for dtype in (hip.BF16, hip.F16):
        chain = lambda gate, scale, shift, ld: lib.nova_row_norm_chain(P[0], P[1], P[2], P[3], P[4], ld, gate, scale, shift, 1e-5, 1e-6, None,
                                                                      P[5], 5, D, dtype, None)
        for offs in ((3 * D - 120, 0, D), (0, 3 * D - 120, D), (0, D, 3 * D - 120)):
            assert chain(*offs, 3 * D) == -2, offs
            assert f"row_norm_chain: modulation offset {3 * D - 120} + D {D} exceeds the row stride {3 * D}" in err()
    # nova_adaln_fc1 on f32 rows always takes the two-launch form: row_norm's check answers
    rc = lib.nova_adaln_fc1(P[0], P[4], 2 * D, 0, D + 4, 1e-6, P[2], None, P[5], P[6], 5, D, D, 2, hip.F32, None)
    assert rc == -2 and f"row_norm: modulation offset {D + 4} + D {D} exceeds the row stride {2 * D}" in err()


def test_patch_vector_lengths_0_and_65_are_refused_before_any_launch():
    hip, lib = _lib()
    for dtype in (hip.F32, hip.BF16, hip.F16):
        for bad in (0, 65, -1):
            assert lib.nova_embed_canvas(P[0], P[1], P[2], P[3], P[4], None, P[5], 2, 3, bad, 8, dtype, None) == -2, bad
            assert f"embed_canvas: patch vector length {bad} unsupported (1..64)".encode() in lib.nova_last_error()
            assert lib.nova_patch_embed_rows(P[0], P[2], P[3], P[5], 2, 2, 3, bad, 8, dtype, None) == -2, bad
            assert f"patch_embed_rows: patch vector length {bad} unsupported".encode() in lib.nova_last_error()
