"""The row kernels held to an elementwise contract on hard rows (GPU box only).

`nova_row_norm` (csrc/rownorm.h, csrc/rowops.hip), its fp8 side output, `nova_row_norm_bwd` (csrc/rownorm_bwd.hip) and the glue
kernels around them are called through the C ABI and every output element is compared in float64 with a restatement of the
operation on the stored inputs. Cases, restatements and bounds live in tests/test_row_contract_cpu.py, which also shows on the
CPU that the bounds leave a float32 restatement of the kernels' operation order a factor two, and that the inputs tell the
wrong kernels named below apart from the right one by more than four bounds. Bounds: forward u_T |ref| + (D/64 + 8) 2^-24 mean|x| rstd |G|
+ 8 2^-24 A_y; dx u_T |ref| + (D/64 + 8) 2^-23 A_dx; modulation gradients u_T |ref| + 8 2^-24 A; glue u_T |ref| + 4 2^-24 A.

Every output lives in a buffer prefilled with a canary (-1536, exact in f32, bf16 and f16) with padding behind it: an element
nobody wrote fails its bound (the caching allocator would otherwise hand back the previous call's correct result), and the
padding must keep its bits.

What each family or shape is there to catch:
  tiny rows                      `eps` ignored, or the engine's 1e-5 and 1e-6 exchanged (CPU teeth: > 4 bounds on every row)
  spike rows                     the last 16-byte chunk dropped from the statistics (a wrong `d < D`, a wrong NIT at 1032 / 1028)
  offset / const rows            statistics that lose |x - mean| << |mean| beyond what an f32 mean must; nothing else states how
                                 far the forward (f32 statistics) and the backward (f64 statistics) normalise one row apart
  scales rows                    a small row next to a large one: an error a global max|err| / max|ref| hides
  shift before scale, mod_ld > columns used   scale and shift exchanged; a modulation row addressed by 5 D instead of mod_ld
  rows 1, 3, 4, 5, 37, 1025      the four-rows-per-workgroup edge, the XCD remap of row blocks
  widths 8 / 4, 1032 / 1028, 2048   a single lane, one chunk over the NIT switch, every lane's last chunk
  gather with res and mod        res / mod indexed by SOURCE row (they belong to the output row)
  out == res, out == in          a store issued before the row's last load
  NaN / inf in one row           a row's statistics leaking into its workgroup neighbours
  past-the-cap glue launches     a grid-stride increment off by one block, a 32-bit element index, a tail never written
  P = 1, 64 and D = 8, 264       the patch loops at both ends, a D loop that assumes whole 256-column trips

Measured worst error / bound on an MI355X (`[contract]` lines of a `-s` run of this file), f32 | bf16 | f16. A 16-bit figure near 1 is
the rounding to the storage type itself (u_T |ref| is reached at the bottom of a binade; the CPU file says why no margin can be asked
of it); the f32 column is the one that measures the kernels' arithmetic:
  nova_row_norm, rows 1 to 37, every kind, width, family, eps      0.369 | 0.996 | 0.998
      by family (f16): unit 0.997, offset 0.958, tiny 0.998, const 0.976, spike 0.998, scales 0.997
  nova_row_norm, 1025 rows                                         0.321 | 0.996 | 0.998
  nova_row_norm with gather, res and mod                           0.196 | 0.996 | 0.995
  nova_row_norm_fp8 (bf16): bits equal nova_quantize_rows_fp8; scale 0.80 of 2^-23 relative (1.14 ulps of the scale itself, which is why
      "one ulp" is taken at the bottom of the binade: see the test); dequantised values 1.000 half steps (exact ties occur)
  nova_row_norm_bwd  dx 0.173 | 0.995 | 0.990   d_scale 0.362 | 0.996 | 0.998   d_shift 0.111 | 0.988 | 0.999   d_gate 0.370 | 0.996 | 0.999
  nova_silu_add_rows 0.584 | 0.996 | 1.000 (rounded: the assertion is <= 1)   silu_add_steps 0.591 | 0.996 | 0.998
  nova_modulate_rows 0.394 | 0.996 | 0.999
  nova_act_fwd / nova_act_bwd   gelu 0.418 / 0.372 (f32), 0.975 / 0.996 (bf16)   silu 0.394 / 0.474 (f32), 0.996 / 0.996 (bf16)
  rope_table 0.032 of atol 2e-6, with and without ids
  nova_embed_canvas, nova_patch_embed_rows (P 1 and 64, D 8 and 264)   0.907 | 0.996 | 0.995   (f32: P = 64, D = 264; 0.30 at P = 1)
  nova_head_cfg_euler 0.189 | 0.157 | 0.149
The first run found no kernel outside a bound in f32 or bf16. In f16 four tests missed - 1025-row forward 1.04 and 1.01, silu_add_rows 409,
modulate_rows 1.55 - all on outputs below f16's smallest normal 2^-14, where the values are 2^-24 apart and u_T |ref| asks for more than
the format has: the rounding term is now floored at 2^-25 for f16 (`rounding` in the CPU file), which no correctly rounded result can miss.

Forward and backward on the same row. The forward keeps f32 statistics (csrc/rownorm.h: tests/golden/denoise_bits.json and the other
recorded bits pin its arithmetic), the backward recomputes them in f64 (csrc/rownorm_bwd.hip). On f32 `offset` rows (100 + 0.01 N(0,1),
n of order 1) each stays within its own bound of the float64 n - forward 0.03 to 0.09 of its bound, backward 0.11 to 0.24 of an ulp-sized
one - and the two differ by up to 1.3e-3 ABSOLUTE in n (D 132; 5.9e-4 to 1.1e-3 at the other widths), 0.03 to 0.09 forward bounds: the
rounding of the f32 mean, 2^-24 * 100, times rstd = 100. That gap is what the forward's middle term allows and what the backward no longer has.

Each test fails for a named wrong kernel. Built and run once against this file (wrong results only, every access in bounds):
  eps fixed at 1e-5 in the forward              forward (all 90), 1025 rows, gather and non-finite of the AdaLN kind
  res indexed by source row under gather        gather tests of the three kinds with a residual
  last chunk dropped from the statistics        forward (all 90), 1025 rows, gather, non-finite, fp8 side output, forward / backward consistency
  scale and shift exchanged                     every forward test of the two kinds with scale / shift
  grid-stride increment one block too far       silu_add_rows, silu_add_steps, modulate_rows, activations, rope_table (canary left in the tail)
  backward: eps fixed at 1e-5, d_scale / d_shift stored at each other's offsets   backward tests of the two kinds with scale / shift
  last patch element dropped; D loops of patch_embed_rows and the head that stop after one 256-column trip   patch embeddings (all 12), head D 260 / 2048
"""
import math

import pytest
import torch

import test_row_contract_cpu as C
from test_row_contract_cpu import CANARY, DTYPES, F64, NORM_KINDS, U_T, VEC, WIDTHS

pytestmark = pytest.mark.gpu
DEV = "cuda"
KINDS = sorted(NORM_KINDS)
NAME = {torch.float32: "f32", torch.bfloat16: "bf16", torch.float16: "f16"}


def canary(*shape, dtype):
    return torch.full(shape, CANARY, dtype=dtype, device=DEV)


def keeps_canary(t):
    return bool((t == CANARY).all())


def upload(c):
    return {k: c[k].to(DEV).contiguous() for k in ("x", "mod", "res", "gamma", "beta", "dy")}


def rows_of(ref, r):
    return {k: v[:r] for k, v in ref.items()}


def forward(hip, c, d, eps, rows, buf, *, inp=None, res=None, gather=None):
    """nova_row_norm on the first `rows` rows of the case into buf[:rows]; inp / res override the input / residual pointers."""
    has = c["has"]
    mod = d["mod"] if (has["ss"] or has["gate"]) else None
    res = (d["res"] if res is None else res) if has["res"] else None
    hip.call("nova_row_norm", hip.ptr(d["x"] if inp is None else inp), hip.ptr(buf), hip.ptr(d["gamma"]) if has["affine"] else None,
             hip.ptr(d["beta"]) if has["affine"] else None, hip.ptr(mod), c["mod_ld"] if mod is not None else 0,
             c["scale_off"] if has["ss"] else -1, c["shift_off"] if has["ss"] else -1, c["gate_off"] if has["gate"] else -1, hip.ptr(res),
             hip.ptr(gather), rows, c["D"], float(eps), hip.dtype_code(c["dtype"]), hip.stream_ptr())
    torch.cuda.synchronize()
    return buf.cpu()


def check_rows(got, ref, rows, what):
    assert keeps_canary(got[rows:]), (what, "the two rows behind the output changed")
    w = C.worst(got[:rows], ref)
    assert w <= 1.0, (what, w)
    return w


# ---------------------------------------------------------------------------------------------------------------------
# 3. forward
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES, ids=NAME.get)
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("wi", range(6))
def test_row_norm_forward_every_element_within_its_bound(hip, dtype, kind, wi):
    D = WIDTHS[dtype][wi]
    for family in C.FAMILIES:
        c = C.make_case(dtype, kind, D, family)
        d = upload(c)
        for eps in C.EPS:
            ref = C.forward_ref(c, eps)
            top = 0.0
            for rows in C.ROW_COUNTS:
                what = (NAME[dtype], kind, D, family, eps, rows)
                r = rows_of(ref, rows)
                plain = forward(hip, c, d, eps, rows, canary(rows + 2, D, dtype=dtype))
                top = max(top, check_rows(plain, r, rows, what))
                if rows not in (5, 37):
                    continue
                if c["has"]["res"]:  # in place on the residual stream, as the engine's post-norm calls
                    buf = canary(rows + 2, D, dtype=dtype)
                    buf[:rows] = d["res"][:rows]
                    got = forward(hip, c, d, eps, rows, buf, res=buf)
                    check_rows(got, r, rows, what + ("out == res",))
                    assert torch.equal(got, plain), what + ("out == res",)
                buf = canary(rows + 2, D, dtype=dtype)
                buf[:rows] = d["x"][:rows]
                got = forward(hip, c, d, eps, rows, buf, inp=buf)
                check_rows(got, r, rows, what + ("out == in",))
                assert torch.equal(got, plain), what + ("out == in",)
            print(f"\n[contract] row_norm fwd {NAME[dtype]} {kind} D={D} {family} eps={eps:g}: {top:.3f}", end="")


@pytest.mark.parametrize("dtype", DTYPES, ids=NAME.get)
@pytest.mark.parametrize("D", C.BIG_WIDTHS)
def test_row_norm_forward_1025_rows(hip, dtype, D):
    for family, kind in (("unit", "everything"), ("scales", "everything"), ("tiny", "adaln_modulate"), ("spike", "vit_post_norm")):
        c = C.make_case(dtype, kind, D, family, rows=C.BIG_ROWS)
        eps = C.eps_of(kind)
        got = forward(hip, c, upload(c), eps, C.BIG_ROWS, canary(C.BIG_ROWS + 2, D, dtype=dtype))
        w = check_rows(got, C.forward_ref(c, eps), C.BIG_ROWS, (NAME[dtype], kind, D, family))
        print(f"\n[contract] row_norm fwd {NAME[dtype]} {kind} D={D} {family} rows=1025: {w:.3f}", end="")


@pytest.mark.parametrize("dtype", DTYPES, ids=NAME.get)
@pytest.mark.parametrize("kind", KINDS)
def test_row_norm_gather_with_res_and_mod(hip, dtype, kind):
    """5 output rows out of 37 sources, with repeats: `in` by source row, `res` and `mod` by output row."""
    idx = torch.tensor(C.GATHER, dtype=torch.int32, device=DEV)
    for D in WIDTHS[dtype]:
        for family in ("unit", "scales"):
            c = C.make_case(dtype, kind, D, family)
            eps = C.eps_of(kind)
            got = forward(hip, c, upload(c), eps, len(C.GATHER), canary(len(C.GATHER) + 2, D, dtype=dtype), gather=idx)
            w = check_rows(got, C.forward_ref(c, eps, src=C.GATHER), len(C.GATHER), (NAME[dtype], kind, D, family, "gather"))
            print(f"\n[contract] row_norm fwd gather {NAME[dtype]} {kind} D={D} {family}: {w:.3f}", end="")


@pytest.mark.parametrize("dtype", DTYPES, ids=NAME.get)
@pytest.mark.parametrize("kind", KINDS)
def test_row_norm_non_finite_row_stays_in_its_row(hip, dtype, kind):
    """One NaN and one inf in row 2 of 5 (rows 0 to 3 share a workgroup): every other row passes its bound, row 2 is not finite."""
    for D in WIDTHS[dtype]:
        c = C.make_case(dtype, kind, D, "unit", rows=5)
        c["x"][2, 1] = float("nan")
        c["x"][2, D - 1] = float("inf")
        eps = C.eps_of(kind)
        got = forward(hip, c, upload(c), eps, 5, canary(7, D, dtype=dtype))
        assert keeps_canary(got[5:])
        ref = C.forward_ref(c, eps)
        for r in (0, 1, 3, 4):
            assert C.worst(got[r:r + 1], {k: v[r:r + 1] for k, v in ref.items()}) <= 1.0, (NAME[dtype], kind, D, r)
        assert not torch.isfinite(got[2].float()).any(), (NAME[dtype], kind, D)


def _e4m3_half_step(v):
    """Half the e4m3 spacing at |v|: 3 mantissa bits, smallest normal 2^-6 (below it the subnormal step 2^-9), top binade 256."""
    e = torch.floor(torch.log2(v.abs().clamp_min(2.0 ** -6))).clamp_max(8)
    return torch.exp2(e - 4)


@pytest.mark.parametrize("D", [8, 1032, 2048])
def test_row_norm_fp8_side_output(hip, D):
    """nova_row_norm_fp8: the e4m3 bytes and scales equal nova_quantize_rows_fp8 of the stored bf16 row bit for bit, and against float64
    on that row: scale == amax / 448 within one ulp - taken as 2^-23 relative, an ulp at the bottom of a binade: the kernel multiplies by
    the rounded 1 / 448 (off by 0.75 * 2^-24) and rounds once more (2^-24), 0.875 * 2^-23 in all; in ulps of the scale itself that is up to
    1.25 where amax / 448 lies high in its binade, so the count in ulps is printed, not asserted -, every dequantised value within half an
    e4m3 step of x / scale (plus 2^-22 |x / scale| for the two f32 roundings of x * (1 / scale))."""
    dtype = torch.bfloat16
    tops = [0.0, 0.0, 0.0]
    for family in ("unit", "scales", "zero"):
        c = C.make_case(dtype, "vit_post_norm", D, "const" if family == "zero" else family)
        if family == "zero":  # a value whose f32 row sum is exact: x - mean = 0, and with beta = 0 and res = 0 the output is all zero
            c["x"] = torch.full_like(c["x"], 0.75)
            c["beta"], c["res"] = torch.zeros_like(c["beta"]), torch.zeros_like(c["res"])
        d = upload(c)
        rows = c["rows"]
        out = canary(rows + 2, D, dtype=dtype)
        q = torch.full((rows + 2, D), 0xA5, dtype=torch.uint8, device=DEV)
        sc = torch.full((rows + 2,), CANARY, dtype=torch.float32, device=DEV)
        hip.call("nova_row_norm_fp8", hip.ptr(d["x"]), hip.ptr(out), hip.ptr(d["gamma"]), hip.ptr(d["beta"]), hip.ptr(d["res"]), hip.ptr(q),
                 hip.ptr(sc), rows, D, 1e-5, hip.stream_ptr())
        torch.cuda.synchronize()
        assert keeps_canary(out[rows:]) and keeps_canary(sc[rows:]) and bool((q[rows:] == 0xA5).all())
        check_rows(out.cpu(), C.forward_ref(c, 1e-5), rows, ("fp8", D, family))
        q2, sc2 = hip.quantize_rows_fp8(out[:rows].contiguous())
        assert torch.equal(q[:rows], q2) and torch.equal(sc[:rows], sc2), (D, family)
        x = out[:rows].cpu().to(F64)
        s = sc[:rows].cpu().to(F64)
        if family == "zero":
            assert bool((x == 0).all()) and bool((s == 1).all()) and bool(((q[:rows].cpu() & 0x7F) == 0).all())
            continue
        want = x.abs().amax(1) / 448.0
        assert bool((want > 0).all())
        rel = ((s - want).abs() / want).max().item() / 2.0 ** -23
        ulps = ((s - want).abs() / torch.exp2(torch.floor(torch.log2(want)) - 23)).max().item()
        assert rel <= 1.0, (D, family, rel)
        v = x / s[:, None]
        deq = q[:rows].cpu().view(torch.float8_e4m3fn).float().to(F64)
        step = ((deq - v).abs() / (_e4m3_half_step(v) + 2.0 ** -22 * v.abs())).max().item()
        assert step <= 1.0, (D, family, step)
        tops = [max(a, b) for a, b in zip(tops, (rel, ulps, step))]
    print(f"\n[contract] row_norm_fp8 D={D}: scale error {tops[0]:.3f} of 2^-23 relative ({tops[1]:.3f} ulps), dequantised error {tops[2]:.3f} half steps", end="")


# ---------------------------------------------------------------------------------------------------------------------
# 4. backward
# ---------------------------------------------------------------------------------------------------------------------
def backward(hip, c, d, eps, rows, parts, *, mod=None, lay=None, dy=None, affine=None):
    """nova_row_norm_bwd on the first `rows` rows -> (dx buffer [rows + 2, D], dmod [rows, mod_ld] or None), on the CPU."""
    has, D, dtype = c["has"], c["D"], c["dtype"]
    if lay is None:  # the case's own modulation row; lay / mod: another layout (the consistency test's gate-only row)
        lay = dict(mod_ld=c["mod_ld"], scale_off=c["scale_off"] if has["ss"] else -1, shift_off=c["shift_off"] if has["ss"] else -1,
                   gate_off=c["gate_off"] if has["gate"] else -1)
        mod = d["mod"] if (has["ss"] or has["gate"]) else None
    affine = has["affine"] if affine is None else affine
    dx = canary(rows + 2, D, dtype=dtype)
    dmod = canary(rows, lay["mod_ld"], dtype=dtype) if mod is not None else None
    dg = torch.full((parts, D), float("nan"), dtype=torch.float32, device=DEV) if affine else None
    db = torch.full((parts, D), float("nan"), dtype=torch.float32, device=DEV) if affine else None
    hip.call("nova_row_norm_bwd", hip.ptr(d["x"]), hip.ptr(d["dy"] if dy is None else dy), hip.ptr(d["gamma"]) if affine else None,
             hip.ptr(d["beta"]) if affine else None, hip.ptr(mod), lay["mod_ld"] if mod is not None else 0, lay["scale_off"], lay["shift_off"],
             lay["gate_off"], hip.ptr(dx), hip.ptr(dmod), hip.ptr(dg), hip.ptr(db), parts, rows, D, float(eps), hip.dtype_code(dtype),
             hip.stream_ptr())
    torch.cuda.synchronize()
    return dx.cpu(), None if dmod is None else dmod.cpu()


@pytest.mark.parametrize("dtype", DTYPES, ids=NAME.get)
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("wi", range(6))
def test_row_norm_backward_every_element_within_its_bound(hip, dtype, kind, wi):
    D = WIDTHS[dtype][wi]
    eps = C.eps_of(kind)
    cols = dict(d_scale="scale_off", d_shift="shift_off", d_gate="gate_off")
    for family in C.BWD_FAMILIES:
        c = C.make_case(dtype, kind, D, family)
        d = upload(c)
        top = {}
        for rows in (1, 5, 37):
            ref = C.backward_ref(c, eps, rows)
            first = None
            for parts in (4, min(1024, (rows + 3) // 4 * 4)):
                what = (NAME[dtype], kind, D, family, rows, parts)
                dx, dmod = backward(hip, c, d, eps, rows, parts)
                assert keeps_canary(dx[rows:]), what
                top["dx"] = max(top.get("dx", 0.0), C.worst(dx[:rows], ref["dx"]))
                written = torch.zeros(c["mod_ld"], dtype=torch.bool)
                for name, off in cols.items():
                    if name in ref:
                        o = c[off]
                        written[o:o + D] = True
                        top[name] = max(top.get(name, 0.0), C.worst(dmod[:, o:o + D], ref[name]))
                assert (dmod is None) == (not written.any())
                if dmod is not None:
                    assert keeps_canary(dmod[:, ~written]), what + ("a column of dmod outside the terms changed",)
                assert max(top.values()) <= 1.0, (what, top)
                if first is None:
                    first = (dx, dmod)
                else:  # one wave per row whatever the grid: dx and dmod do not depend on parts
                    assert torch.equal(dx, first[0]) and (dmod is None or torch.equal(dmod, first[1])), what
        print(f"\n[contract] row_norm bwd {NAME[dtype]} {kind} D={D} {family}: " + " ".join(f"{k} {v:.3f}" for k, v in sorted(top.items())), end="")


def test_forward_and_backward_normalise_offset_rows_within_their_bounds_of_each_other(hip):
    """f32 `offset` rows: the forward's n (plain kind, read from `out`) and the backward's n (d_gate of a gate-only call with dy = 1:
    d_gate = dy * u2 = n) against the float64 n. The forward keeps f32 statistics, the backward takes them in f64; each stays within
    its own bound, and the gap between them is printed."""
    dtype = torch.float32
    for D in WIDTHS[dtype]:
        c = C.make_case(dtype, "plain", D, "offset")
        d = upload(c)
        rows = c["rows"]
        ref = C.forward_ref(c, 1e-5)
        n_fwd = forward(hip, c, d, 1e-5, rows, canary(rows + 2, D, dtype=dtype))[:rows].to(F64)
        gate = torch.randn(rows, D, device=DEV)
        _, dmod = backward(hip, c, d, 1e-5, rows, 4, mod=gate, lay=dict(mod_ld=D, scale_off=-1, shift_off=-1, gate_off=0),
                           dy=torch.ones(rows, D, device=DEV), affine=False)
        n_bwd = dmod.to(F64)
        n = ref["n"]
        w_fwd = C.worst(n_fwd, ref)
        w_bwd = C.worst(n_bwd, dict(y=n, bound=U_T[dtype] * n.abs() + 8 * 2.0 ** -24 * n.abs()))
        assert w_fwd <= 1.0 and w_bwd <= 1.0, (D, w_fwd, w_bwd)
        gap = (n_fwd - n_bwd).abs()
        print(f"\n[contract] n forward vs backward f32 offset D={D}: forward {w_fwd:.3f} of its bound, backward {w_bwd:.3f} of its bound, "
              f"largest gap {gap.max().item():.3e} absolute = {(gap / ref['bound']).max().item():.3f} forward bounds", end="")


# ---------------------------------------------------------------------------------------------------------------------
# 5. glue kernels past their block caps and at their P / D edges
# ---------------------------------------------------------------------------------------------------------------------
def check_glue(got, ref, A, dtype, what, marks=None, atol=None):
    """|got - ref| <= u_T |ref| (C.rounding) + 4 * 2^-24 * A (or atol) for every element, on the device in float64; `marks` names flat indices."""
    got, ref = got.reshape(-1).to(F64), ref.reshape(-1).to(F64)
    bound = torch.full_like(ref, atol) if atol is not None else C.rounding(ref, dtype) + 4 * 2.0 ** -24 * A.reshape(-1).to(F64)
    diff = (got - ref).abs()
    ratio = torch.nan_to_num(torch.where(diff == 0, torch.zeros_like(diff), diff / bound), nan=float("inf"))
    w = ratio.max().item()
    named = dict(marks or {}, worst=int(ratio.argmax()))
    assert w <= 1.0, f"{what}: worst error / bound {w:.3f}; " + "; ".join(
        f"{k} element [{i}] got {got[i].item():.9g} ref {ref[i].item():.9g} error / bound {ratio[i].item():.3f}" for k, i in named.items())
    return w


def randn_dev(*shape, seed, dtype, scale=1.0):
    g = torch.Generator(device=DEV).manual_seed(seed)
    return (torch.randn(*shape, device=DEV, generator=g) * scale).to(dtype)


ROW_CAP = 8192 * 256 * 4      # elements one trip of silu_add_rows / modulate_rows covers (8192 blocks, 4 values per thread)
PAST_ROWS, PAST_D = 4097, 2048  # rows * D / 4 = 2 097 664 > 2 097 152


@pytest.mark.parametrize("dtype", DTYPES, ids=NAME.get)
@pytest.mark.parametrize("rowvec", [True, False])
def test_silu_add_rows_takes_a_second_trip(hip, dtype, rowvec):
    """A = |a| + |vec|: the fast exponential inside silu rounds its argument x log2 e in f32, an error that grows with |x|, so the
    companion of silu(z) is |z|'s terms, not |silu(z)|."""
    rows, D = PAST_ROWS, PAST_D
    assert rows * D > ROW_CAP
    a = randn_dev(rows, D, seed=1, dtype=dtype)
    vec = randn_dev(D, seed=2, dtype=dtype) if rowvec else None
    out = canary(rows + 1, D, dtype=dtype)
    hip.call("nova_silu_add_rows", hip.ptr(a), hip.ptr(vec), hip.ptr(out), rows, D, hip.dtype_code(dtype), hip.stream_ptr())
    z = a.to(F64) + (vec.to(F64) if rowvec else 0)
    A = a.to(F64).abs() + (vec.to(F64).abs() if rowvec else 0)
    w = check_glue(out[:rows], z * torch.sigmoid(z), A, dtype, ("silu_add_rows", NAME[dtype], rowvec),
                   {"first past the cap": ROW_CAP, "last": rows * D - 1})
    assert keeps_canary(out[rows:])
    print(f"\n[contract] silu_add_rows {NAME[dtype]} rowvec={rowvec}: {w:.3f}", end="")


@pytest.mark.parametrize("dtype", DTYPES, ids=NAME.get)
def test_modulate_rows_takes_a_second_trip(hip, dtype):
    rows, D = PAST_ROWS, PAST_D
    x, mod = randn_dev(rows, D, seed=3, dtype=dtype), randn_dev(rows, 2 * D, seed=4, dtype=dtype, scale=0.5)
    out = canary(rows + 1, D, dtype=dtype)
    hip.call("nova_modulate_rows", hip.ptr(x), hip.ptr(mod), hip.ptr(out), rows, D, hip.dtype_code(dtype), hip.stream_ptr())
    x64, sc, sh = x.to(F64), mod[:, :D].to(F64), mod[:, D:].to(F64)
    w = check_glue(out[:rows], x64 * (1 + sc) + sh, x64.abs() * (1 + sc.abs()) + sh.abs(), dtype, ("modulate_rows", NAME[dtype]),
                   {"first past the cap": ROW_CAP, "last": rows * D - 1})
    assert keeps_canary(out[rows:])
    print(f"\n[contract] modulate_rows {NAME[dtype]}: {w:.3f}", end="")


@pytest.mark.parametrize("dtype", DTYPES, ids=NAME.get)
def test_silu_add_steps_takes_a_second_trip_inside_the_denoising_loop(hip, dtype):
    """silu_add_steps has no entry of its own: nova_decoder_denoise with the AdaLN projections of all steps hoisted (mod_steps == steps)
    calls it on steps * rows rows and leaves its output in the caller's workspace `ws_a`. 16 steps x 8193 rows x 128 columns / 4 =
    4 195 328 > 16384 blocks x 256."""
    import ctypes

    import denoise_ref as R

    D, depth, P, B, n, steps = 128, 1, 3, 1, 8193, 16
    cap = 16384 * 256 * 4
    assert steps * B * n * D > cap
    _, pack, ws = R.make_decoder(D, depth, P, dtype, R.weights_seed(D, depth, P), hip=hip, steps=steps, S=B, B=B, n=n)
    ws.a = canary(steps * B * n + 1, D, dtype=dtype)
    ws.zc.copy_(randn_dev(B * n, D, seed=5, dtype=dtype))
    ws.temb.copy_(randn_dev(steps, D, seed=6, dtype=dtype))
    ws.x.copy_(randn_dev(B, n, P, seed=7, dtype=torch.float32))
    plan = R.plan_struct(hip, [R.Step(1.0, 0.0, 1.0, 0.0, -1.0 / steps, 1.0, 0.0, 0.0, 0)] * steps)
    hip.set_graphs(False)
    try:
        hip.call("nova_decoder_denoise", ctypes.byref(pack.struct), ws.zc.data_ptr(), ws.temb.data_ptr(), ws.x.data_ptr(), plan, None, 1.0,
                 None, steps, B, B, n, P, D, ws.a.data_ptr(), ws.u.data_ptr(), ws.h.data_ptr(), ws.f.data_ptr(), ws.g.data_ptr(),
                 ws.mod.data_ptr(), ws.v.data_ptr(), steps, hip.dtype_code(dtype), hip.stream_ptr())
        torch.cuda.synchronize()
    finally:
        hip.set_graphs(True)
    zc, temb = ws.zc.to(F64), ws.temb.to(F64)
    z = zc[None] + temb[:, None]  # [steps, rows, D]
    A = zc.abs()[None] + temb.abs()[:, None]
    w = check_glue(ws.a[:steps * B * n], z * torch.sigmoid(z), A, dtype, ("silu_add_steps", NAME[dtype]),
                   {"first past the cap": cap, "last": steps * B * n * D - 1})
    assert keeps_canary(ws.a[steps * B * n:]) and bool(torch.isfinite(ws.x).all())
    print(f"\n[contract] silu_add_steps {NAME[dtype]}: {w:.3f}", end="")


def _act_ref(kind, x, dy):
    """float64 value or dy * slope, and the companion: |x| for the value, |dy| (1 + |x|) for the slope (the exponential's and erf's
    argument errors grow with |x|; csrc/rownorm_bwd.hip spells the formulas)."""
    if kind == "gelu":
        cdf = 0.5 * (1 + torch.erf(x / math.sqrt(2.0)))
        val, slope = x * cdf, cdf + x * torch.exp(-0.5 * x * x) / math.sqrt(2 * math.pi)
    else:
        s = torch.sigmoid(x)
        val, slope = x * s, s * (1 + x * (1 - s))
    return (val, x.abs()) if dy is None else (dy * slope, dy.abs() * (1 + x.abs()))


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float32], ids=NAME.get)
@pytest.mark.parametrize("kind", ["gelu", "silu"])
def test_activations_take_a_second_trip(hip, dtype, kind):
    vec = VEC[dtype]
    cap = 16384 * 256 * vec  # elements of one trip: 16384 blocks, one 16-byte chunk per thread
    n = cap + 257 * vec
    x, dy = randn_dev(n, seed=8, dtype=dtype, scale=2.5), randn_dev(n, seed=9, dtype=dtype)
    marks = {"first past the cap": cap, "last": n - 1}
    code, k = hip.dtype_code(dtype), 1 if kind == "gelu" else 2
    y = canary(n + vec, dtype=dtype)
    hip.call("nova_act_fwd", hip.ptr(x), hip.ptr(y), n, k, code, hip.stream_ptr())
    ref, A = _act_ref(kind, x.to(F64), None)
    w_f = check_glue(y[:n], ref, A, dtype, ("act_fwd", kind, NAME[dtype]), marks)
    dx = canary(n + vec, dtype=dtype)
    hip.call("nova_act_bwd", hip.ptr(x), hip.ptr(dy), hip.ptr(dx), n, k, code, hip.stream_ptr())
    ref, A = _act_ref(kind, x.to(F64), dy.to(F64))
    w_b = check_glue(dx[:n], ref, A, dtype, ("act_bwd", kind, NAME[dtype]), marks)
    assert keeps_canary(y[n:]) and keeps_canary(dx[n:])
    print(f"\n[contract] act {kind} {NAME[dtype]}: fwd {w_f:.3f} bwd {w_b:.3f}", end="")


@pytest.mark.parametrize("use_ids", [True, False])
def test_rope_table_takes_a_second_trip(hip, use_ids):
    """nb * (pad + n) * hd / 2 = 3 * 10924 * 32 = 1 048 704 > 4096 blocks x 256. Reference: the f32 angle pos * inv_freq (one rounding, as
    the kernel forms it) through float64 cos / sin; atol 2e-6 as tests/test_gpu_kernels.py::test_rope_table."""
    from test_gpu_kernels import grid_pos, inv_freq

    hd, nb, pad = 64, 3, 5
    pos = grid_pos(61, 179)  # 10919 positions
    n_pos = pos.shape[0]
    g = torch.Generator().manual_seed(0)
    ids = torch.stack([torch.randperm(n_pos, generator=g) for _ in range(nb)]).to(DEV) if use_ids else None
    total = nb * (pad + n_pos) * (hd // 2)
    cap = 4096 * 256
    assert cap < total < cap + 4096
    freq = inv_freq(hd)
    buf = canary(total * 2 + 64, dtype=torch.float32)
    tab = hip.rope_table(pos, ids, pad, freq, nb, hd, out=buf)
    n0, n1 = (hd // 8) // 2, ((hd - hd // 8) // 2) // 2
    axis = torch.tensor([0] * n0 + [1] * n1 + [2] * (hd // 2 - n0 - n1), device=DEV)
    p = pos[ids] if use_ids else pos[None].expand(nb, -1, -1)          # [nb, n, 3]
    p = torch.nn.functional.pad(p, (0, 0, pad, 0))                      # rows l < pad are position 0
    ang = (p[..., axis] * freq).to(F64)                                 # the f32 product, then float64
    ref = torch.stack([ang.cos(), ang.sin()], -1)
    w = check_glue(tab, ref, None, torch.float32, ("rope_table", use_ids), {"first past the cap": 2 * cap, "last": 2 * total - 1}, atol=2e-6)
    assert keeps_canary(buf[2 * total:])
    print(f"\n[contract] rope_table ids={use_ids}: {w:.3f} of atol 2e-6", end="")


@pytest.mark.parametrize("dtype", DTYPES, ids=NAME.get)
@pytest.mark.parametrize("P", [1, 64])
@pytest.mark.parametrize("D", [8, 264])
def test_patch_embeddings_at_their_p_and_d_edges(hip, dtype, P, D):
    B, N, S, n = 2, 5, 4, 3
    code = hip.dtype_code(dtype)
    canvas, mask = randn_dev(B, N, P, seed=10, dtype=torch.float32), (torch.arange(B * N, device=DEV).view(B, N) % 3 == 1).float()
    w, bias = randn_dev(D, P, seed=11, dtype=dtype, scale=P ** -0.5), randn_dev(D, seed=12, dtype=torch.float32)
    tok, pe = randn_dev(1, D, seed=13, dtype=dtype), randn_dev(N, D, seed=14, dtype=dtype)
    w64, m = w.to(F64), mask.to(F64)[..., None]
    e, Ae = canvas.to(F64) @ w64.T + bias.to(F64), canvas.to(F64).abs() @ w64.abs().T + bias.to(F64).abs()
    tops = []
    for pos_embed in (None, pe):
        z0 = canary(B * N + 1, D, dtype=dtype)
        hip.call("nova_embed_canvas", hip.ptr(canvas), hip.ptr(mask), hip.ptr(w), hip.ptr(bias), hip.ptr(tok), hip.ptr(pos_embed), hip.ptr(z0),
                 B, N, P, D, code, hip.stream_ptr())
        ref, A = e * (1 - m) + tok.to(F64) * m, Ae * (1 - m) + tok.to(F64).abs() * m
        if pos_embed is not None:
            ref, A = ref + pe.to(F64), A + pe.to(F64).abs()
        tops.append(check_glue(z0[:B * N], ref, A, dtype, ("embed_canvas", NAME[dtype], P, D, pos_embed is not None)))
        assert keeps_canary(z0[B * N:])
    x = randn_dev(B, n, P, seed=15, dtype=torch.float32)
    u = canary(S * n + 1, D, dtype=dtype)
    hip.call("nova_patch_embed_rows", hip.ptr(x), hip.ptr(w), hip.ptr(bias), hip.ptr(u), S, B, n, P, D, code, hip.stream_ptr())
    xs = torch.cat([x] * (S // B)).to(F64)  # sequence s reads batch entry s % B
    tops.append(check_glue(u[:S * n], xs @ w64.T + bias.to(F64), xs.abs() @ w64.abs().T + bias.to(F64).abs(), dtype,
                           ("patch_embed_rows", NAME[dtype], P, D)))
    assert keeps_canary(u[S * n:])
    print(f"\n[contract] embed_canvas | +pos_embed | patch_embed_rows {NAME[dtype]} P={P} D={D}: " + " | ".join(f"{t:.3f}" for t in tops), end="")


@pytest.mark.parametrize("dtype", DTYPES, ids=NAME.get)
@pytest.mark.parametrize("D", [4, 260, 2048])
@pytest.mark.parametrize("cfg", [1, 0])
def test_head_cfg_euler_per_element_on_nearly_cancelling_predictions(hip, dtype, D, cfg):
    """The unconditional rows are the conditional ones with every seventh column moved by about 1 %: pc - pu is small against either,
    which a global norm of x hides. x is f32 in every mode (u_T = 2^-24)."""
    B, n, P, g, dt = 3, 5, 3, 5.0, -0.04
    hc = randn_dev(B * n, D, seed=16, dtype=dtype)
    hu = hc.clone()
    hu[:, ::7] = (hc[:, ::7].float() * 1.01).to(dtype)
    h = torch.cat([hc, hu]).contiguous()
    w, bias = randn_dev(P, D, seed=17, dtype=dtype, scale=D ** -0.5), randn_dev(P, seed=18, dtype=torch.float32)
    x = randn_dev(B * n * P, seed=19, dtype=torch.float32)
    buf = canary(B * n * P + 8, dtype=torch.float32)
    buf[:B * n * P] = x
    hip.call("nova_head_cfg_euler", hip.ptr(h), hip.ptr(w), hip.ptr(bias), hip.ptr(buf), B, n, P, D, g if cfg else 1.0, cfg, dt,
             hip.dtype_code(dtype), hip.stream_ptr())
    w64, b64 = w.to(F64), bias.to(F64)
    pc, pu = hc.to(F64) @ w64.T + b64, hu.to(F64) @ w64.T + b64
    Ac, Au = hc.to(F64).abs() @ w64.abs().T + b64.abs(), hu.to(F64).abs() @ w64.abs().T + b64.abs()
    v, Av = (pu + g * (pc - pu), Au + g * (Ac + Au)) if cfg else (pc, Ac)
    x64 = x.to(F64).view(B * n, P)
    top = check_glue(buf[:B * n * P], x64 + dt * v, x64.abs() + abs(dt) * Av, torch.float32, ("head_cfg_euler", NAME[dtype], D, cfg))
    assert keeps_canary(buf[B * n * P:])
    if cfg:
        assert float((pc - pu).abs().max() / pc.abs().max()) < 0.05
    print(f"\n[contract] head_cfg_euler {NAME[dtype]} D={D} cfg={cfg}: {top:.3f}", end="")
