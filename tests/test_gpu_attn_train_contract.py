"""The training attention and the LayerNorm backward held to their C contract (include/nova_hip.h), element by element.

`nova_attn_fwd_lse` (the LSE / MASK forms of csrc/attn16.hip) and `nova_attn_bwd` (`attn_delta_kernel`, `attn_bwd_dq`,
`attn_bwd_dkv` of csrc/attn_bwd.hip) are called with raw pointers, in a contiguous layout and in the packed strided layout
of the fused QKV projection, and every output - o, lse, delta, dq, dk, dv - is compared ELEMENTWISE in float64 with a
restatement of the header's formulas on the bf16 values the kernels receive (`restate`). The restatement itself is pinned to
torch autograd of F.scaled_dot_product_attention in float64 by a CPU test first, with the factor conventions `scale` and
`ln 2`. The CPU tests (the restatement, the ABI refusals) carry no mark; each GPU test carries `pytest.mark.gpu` of its own,
because one module-wide mark would take the CPU tests with it.

Bounds (from the kernels' stated arithmetic, not from running them); `A_x` is the product that yields x with every factor
replaced by its absolute value:
  lse    |lse - ref| <= 1.5 * 2^-9 + LSE_BINADE + hd * 2^-23 * max_j |s2_ij|, LSE_BINADE = log2(e) * 2^-9. The LSE forms
         (`attn_bf16_m16<E, HD, 2, true, SUMM = true>`, masked or not, head_dim 64 and 96) take `l_tot = lacc[qb][0]`: the row
         sum of the bf16-ROUNDED P, accumulated in f32 by an MFMA against an all-ones block - not the f32 sum of the unrounded
         exponentials (`l_run`, the SUMM = false forms, which no training call reaches). The scores are f32 sums of hd exact
         products. The first term is the derivation this file started from: "a rounded P is within 2^-9 relative, so is the
         sum, 1.44 * 2^-9 in the log2 domain". The unchanged kernel exceeded it, by up to 1.52x, in rows of 127 keys and
         more and nowhere else, and the reason is a term that derivation leaves out: bf16 keeps 8 significand bits, so
         rounding to nearest is within 2^-9 of the TOP of a value's binade but 2^-8 of its bottom - the unit roundoff is
         2^-8. A peaked row is one P; with a single 64-key tile the row maximum is subtracted exactly and that P is 1.0,
         which rounds without error, but from the second tile on the maximum is only refreshed when it grows by more than
         2^8 (the deferred rescale), the dominant P = 2^(s - m_run) falls anywhere in its binade and carries up to 2^-8.
         LSE_BINADE is that second half, log2(1 + 2^-8) - log2(1 + 2^-9) rounded up. (The gradient bound below already
         counts "the lse error carried into P" as 2^-8 relative.)
  delta  |delta - sum_c dO * o_kernel| <= hd * 2^-23 * sum_c |dO| |o|    (o_kernel: the forward's own bf16 output)
  o      |o - ref| <= 2^-7 A_o + 2^-9 |ref|
  dq dk dv  |g - ref| <= 2^-7 A_g + 2^-9 |ref|; 2^-7: bf16 rounding of P / dS (2^-9), the lse error carried into P
         (<= 2^-8 relative) and the hardware exp2, roughly doubled. dq and dk add the f32 cancellation of dP - delta,
         E_ij = P_ij * hd * 2^-23 * (sum_c |dO_ic| |v_jc| + sum_c |dO_ic| |o_ic|), carried through the same absolute
         product (scale * E |K|, ln 2 * E^T |q~|).
  d_gamma / d_beta of nova_row_norm_bwd: |sum over parts - float64| <= rows * 2^-23 * sum_rows |term|.

Measured worst error / bound on an MI355X (this file's own cases; `[contract]` lines of a `-s` run):
  unmasked, head_dim 64:  lse 0.79  delta 0.01  o 0.59  dq 0.78  dk 0.78  dv 0.76
  unmasked, head_dim 96:  lse 0.80  delta 0.01  o 0.69  dq 0.75  dk 0.71  dv 0.72
  masked,   head_dim 64:  lse 0.71  delta 0.01  o 0.45  dq 0.61  dk 0.63  dv 0.63
  masked,   head_dim 96:  lse 0.65  delta 0.01  o 0.47  dq 0.61  dk 0.66  dv 0.72
  (lse against its first term alone: up to 1.52, in rows of 127 keys and more; 0.64 at most below that.)
  nova_row_norm_bwd, d_gamma | d_beta at most: one row 0.87 | 0 (exact), 5 rows 0.15 | 0.07, 1025 rows 0.001 | 0.001. With one
  row the bound is one f32 ulp of dy * n. The kernel as this file found it missed it there - 5.2 (f32, D 128), 1.2 (bf16, D 128),
  1842 (f32, D 1536), 540 (bf16, D 1536) times, the same for every `parts`, worst in the columns of smallest |n| - because
  n = (x - mean) * rstd cannot be had to an ulp from f32 statistics where |x - mean| is far below |mean|: the rounding of
  the mean alone (2^-24 |mean|) is then many ulps of x - mean. The backward now takes mean, variance and n in f64 and rounds
  n to f32 once (csrc/rownorm_bwd.hip); the bound is the one this test was given.
"""
import ctypes
import math

import pytest
import torch

gpu = pytest.mark.gpu
LOG2E = 1.4426950408889634
LN2 = math.log(2.0)
LSE_BINADE = LOG2E * 2.0 ** -9  # the half of bf16's unit roundoff 2^-8 that "2^-9 relative" leaves out (module docstring)
FILL = 0x7FA5  # bf16 bit pattern of the canaries, held as int16 (a NaN: any read of it poisons the result)
S_, H_ = 2, 3
F64 = torch.float64
DEV = "cuda"


# ---------------------------------------------------------------------------------------------------------------------
# 1. the float64 restatement of include/nova_hip.h
# ---------------------------------------------------------------------------------------------------------------------
def restate(qs, k, v, d_o, klim, scale, o_for_delta=None):
    """Everything the two entry points promise, in float64, from q~ (= q * scale * log2 e), k, v, dO [S, h, L, hd] and the
    key limit [L] (None: no mask). delta is sum_c dO * o_for_delta (the header's definition on the forward's own o) or, when
    that is None, on the exact o. Returns a dict with o, lse, delta, dq, dk, dv, the absolute companions A_* and the f32
    cancellation terms C_dq / C_dk."""
    qs, k, v, d_o = (t.to(F64) for t in (qs, k, v, d_o))
    L, hd = qs.shape[-2], qs.shape[-1]
    s2 = qs @ k.transpose(-1, -2)
    vis = torch.ones(L, L, dtype=torch.bool) if klim is None else torch.arange(L)[None, :] < klim.to(torch.int64)[:, None]
    s2m = torch.where(vis, s2, torch.full_like(s2, float("-inf")))
    lse = torch.logsumexp(s2m * LN2, dim=-1) * LOG2E  # log2 sum_visible 2^s2
    p = torch.where(vis, torch.exp2(s2 - lse[..., None]), torch.zeros_like(s2))
    o = p @ v
    od = o if o_for_delta is None else o_for_delta.to(F64)
    delta = (d_o * od).sum(-1)
    dp = d_o @ v.transpose(-1, -2)
    ds = p * (dp - delta[..., None])
    r = dict(o=o, lse=lse, delta=delta, p=p, dv=p.transpose(-1, -2) @ d_o, dq=scale * (ds @ k), dk=LN2 * (ds.transpose(-1, -2) @ qs))
    r["smax"] = torch.where(vis, s2.abs(), torch.zeros_like(s2)).amax(-1)
    r["A_o"] = p @ v.abs()
    r["A_dv"] = p.transpose(-1, -2) @ d_o.abs()
    r["A_dq"] = scale * (ds.abs() @ k.abs())
    r["A_dk"] = LN2 * (ds.abs().transpose(-1, -2) @ qs.abs())
    e = p * (hd * 2.0 ** -23) * (d_o.abs() @ v.abs().transpose(-1, -2) + (d_o.abs() * od.abs()).sum(-1)[..., None])
    r["C_dq"] = scale * (e @ k.abs())
    r["C_dk"] = LN2 * (e.transpose(-1, -2) @ qs.abs())
    return r


def make_inputs(L, hd, spread, seed, S=S_, h=H_, spiky=False):
    """bf16 q~, k, v, dO [S, h, L, hd] on the host. spread > 1: peaked rows. spiky: keys planted late in the stream that align
    with two queries (the online-softmax rescale path, as tests/test_gpu_kernels.py::test_attention_spiky_rows)."""
    g = torch.Generator().manual_seed(seed)
    mk = lambda s: torch.randn(S, h, L, hd, generator=g) * s
    q, k, v, d_o = mk(spread), mk(1.0), mk(1.0), mk(1.0)
    if spiky:
        k[:, :, L - 7] = q[:, :, 5] * 4
        k[:, :, 170] = q[:, :, 77] * 3
    scale = hd ** -0.5
    qs = (q * (scale * LOG2E)).bfloat16()
    return qs, k.bfloat16(), v.bfloat16(), d_o.bfloat16(), scale


def staircase(L, cap=None):
    """Key limits with steps at rows and values off every multiple of 4, several inside one 32-row block / one 64-key tile; ends at L
    (or, capped, at `cap`: the keys past it are seen by nobody)."""
    rows = [0, 3, 5, 8, 21, 45, 70, 101, 130, 161, 199, 230]
    lims = [1, 1 + 4, 37, 70, 93, 121, 130, 150, 197, 203, 230, L]
    kl = torch.empty(L, dtype=torch.int32)
    for r0, lim in zip(rows, lims):
        kl[r0:] = min(lim, L)
    kl[L - 3:] = L
    return kl if cap is None else kl.clamp(max=cap)


def key_limits(L, kind):
    if kind == "all_L":
        return torch.full((L,), L, dtype=torch.int32)
    if kind == "all_1":
        return torch.ones(L, dtype=torch.int32)
    if kind == "staircase":
        return staircase(L)
    if kind == "staircase_capped":
        return staircase(L, cap=L - 9)
    assert kind == "late_jump" and L == 257
    kl = torch.full((L,), 100, dtype=torch.int32)
    kl[200:] = L
    return kl


@pytest.mark.parametrize("hd", [64, 96])
@pytest.mark.parametrize("L", [5, 70])
def test_restatement_matches_float64_autograd_of_sdpa(L, hd):
    """`restate` against torch autograd of F.scaled_dot_product_attention in float64, differentiated w.r.t. the UNSCALED
    q = q~ / (scale * log2 e): no mask, a staircase ending at L and one whose last limit is below L. 1e-10 of each tensor's largest entry;
    dk / dv rows of unseen keys exactly 0 in both."""
    qs, k, v, d_o, scale = make_inputs(L, hd, 2.0, seed=L + hd, S=2, h=2)
    cap = L - 2
    for klim in (None, staircase(L), staircase(L, cap=cap)):
        r = restate(qs, k, v, d_o, klim, scale)
        q64 = (qs.to(F64) / (scale * LOG2E)).requires_grad_(True)
        k64, v64 = k.to(F64).requires_grad_(True), v.to(F64).requires_grad_(True)
        mask = None if klim is None else torch.arange(L)[None, :] < klim.to(torch.int64)[:, None]
        out = torch.nn.functional.scaled_dot_product_attention(q64, k64, v64, attn_mask=mask)
        out.backward(d_o.to(F64))
        for name, got, ref in (("o", r["o"], out.detach()), ("dq", r["dq"], q64.grad), ("dk", r["dk"], k64.grad), ("dv", r["dv"], v64.grad)):
            err = (got - ref).abs().max().item()
            assert err <= 1e-10 * ref.abs().max().item(), (name, L, hd, klim is not None, err)
        # lse in the log2 domain against the natural-log one of the scaled scores
        s = (q64.detach() @ k64.detach().transpose(-1, -2)) * scale
        if mask is not None:
            s = s.masked_fill(~mask, float("-inf"))
        assert (r["lse"] - torch.logsumexp(s, -1) * LOG2E).abs().max().item() <= 1e-10 * r["lse"].abs().max().item()
        if klim is not None and int(klim[-1]) < L:
            assert int(klim[-1]) == cap
            for t in (r["dk"], r["dv"], k64.grad, v64.grad):
                assert (t[:, :, cap:] == 0).all()
            assert r["dk"][:, :, :cap].abs().max() > 0


# ---------------------------------------------------------------------------------------------------------------------
# 2. layouts: buffers of int16 (bf16 bit patterns) pre-filled with FILL, two spare rows, gap columns
# ---------------------------------------------------------------------------------------------------------------------
class _Buf:
    def __init__(self, rows, stride):
        self.t = torch.full((rows + 2, stride), FILL, dtype=torch.int16, device=DEV)
        self.rows, self.stride = rows, stride
        self.used = torch.zeros(rows + 2, stride, dtype=torch.bool)

    def put(self, col, x):  # x: bf16 host [S, h, L, hd] -> token-major rows [S L, h hd] at column `col`
        S, h, L, hd = x.shape
        rows = x.transpose(1, 2).reshape(S * L, h * hd).contiguous().view(torch.int16)
        self.t[: self.rows, col:col + h * hd] = rows.to(DEV)
        self.claim(col, h * hd)

    def claim(self, col, width):
        self.used[: self.rows, col:col + width] = True

    def ptr(self, hip, col=0):
        return hip.ptr(self.t) + 2 * col

    def get(self, col, S, h, L, hd):  # -> int16 host [S, h, L, hd]
        return self.t[: self.rows, col:col + h * hd].cpu().view(S, L, h, hd).transpose(1, 2).contiguous()

    def untouched(self):
        return bool((self.t.cpu()[~self.used] == FILL).all())


def run_kernels(hip, qs, k, v, d_o, klim, scale, layout, forward_of=None):
    """Forward with lse, then backward, through the C ABI with raw pointers. layout "A": eight contiguous buffers, every stride h * hd.
    layout "B": q~ | k | v thirds of one [S L + 2, 3 D] buffer, o at row stride D + 64, dO at D + 128, dq | dk | dv thirds of one
    [S L + 2, 3 D] buffer. Every buffer has two spare rows and is pre-filled with FILL; lse / delta with NaN. Asserts the canaries and
    that lse / delta were written. forward_of: an earlier result whose o and lse are handed to the backward instead of running the forward
    (the backward kernels alone). Returns host tensors: o, dq, dk, dv as int16 bit patterns [S, h, L, hd], lse / delta f32 [S, h, L]."""
    S, h, L, hd = qs.shape
    D, n = h * hd, S * L
    if layout == "A":
        bq, bk, bv, bo, bdo, bdq, bdk, bdv = (_Buf(n, D) for _ in range(8))
        cq = ck = cv = cdq = cdk = cdv = 0
        qkv_rs = o_rs = do_rs = dqkv_rs = D
    else:
        bq = bk = bv = _Buf(n, 3 * D)
        bdq = bdk = bdv = _Buf(n, 3 * D)
        bo, bdo = _Buf(n, D + 64), _Buf(n, D + 128)
        cq, ck, cv = 0, D, 2 * D
        cdq, cdk, cdv = 0, D, 2 * D
        qkv_rs, o_rs, do_rs, dqkv_rs = 3 * D, D + 64, D + 128, 3 * D
    bq.put(cq, qs), bk.put(ck, k), bv.put(cv, v), bdo.put(0, d_o)
    bo.claim(0, D), bdq.claim(cdq, D), bdk.claim(cdk, D), bdv.claim(cdv, D)
    lse = torch.full((S, h, L), float("nan"), dtype=torch.float32, device=DEV)
    delta = torch.full((S, h, L), float("nan"), dtype=torch.float32, device=DEV)
    kl = None if klim is None else klim.to(torch.int32).cuda()
    if forward_of is None:
        hip.call("nova_attn_fwd_lse", bq.ptr(hip, cq), bk.ptr(hip, ck), bv.ptr(hip, cv), bo.ptr(hip), hip.ptr(lse), S, h, L, hd, qkv_rs, o_rs,
                 hip.ptr(kl), hip.stream_ptr())
    else:
        bo.put(0, forward_of["o"].view(torch.bfloat16))
        lse.copy_(forward_of["lse"])
    hip.call("nova_attn_bwd", bq.ptr(hip, cq), bk.ptr(hip, ck), bv.ptr(hip, cv), bo.ptr(hip), bdo.ptr(hip), hip.ptr(lse), hip.ptr(delta),
             bdq.ptr(hip, cdq), bdk.ptr(hip, cdk), bdv.ptr(hip, cdv), S, h, L, hd, qkv_rs, o_rs, do_rs, dqkv_rs, float(scale), hip.ptr(kl),
             hip.stream_ptr())
    torch.cuda.synchronize()
    for name, b in (("qkv", bq), ("o", bo), ("dO", bdo), ("dq", bdq), ("dk", bdk), ("dv", bdv)):
        assert b.untouched(), f"layout {layout}: a gap column or spare row of the {name} buffer lost its fill pattern"
    out = dict(o=bo.get(0, S, h, L, hd), dq=bdq.get(cdq, S, h, L, hd), dk=bdk.get(cdk, S, h, L, hd), dv=bdv.get(cdv, S, h, L, hd),
               lse=lse.cpu(), delta=delta.cpu())
    assert torch.isfinite(out["lse"]).all(), f"layout {layout}: an lse entry was not written"
    assert torch.isfinite(out["delta"]).all(), f"layout {layout}: a delta entry was not written"
    return out


def _f64(bits):
    return bits.view(torch.bfloat16).to(F64)


def _worst(err, bound):
    """max of err / bound over the tensor and its (sequence, head, row); an error where the bound is 0 counts as infinite."""
    ratio = torch.where(bound > 0, err / bound.clamp_min(1e-300), torch.where(err > 0, torch.full_like(err, float("inf")), torch.zeros_like(err)))
    per_row = ratio if ratio.dim() == 3 else ratio.amax(-1)
    i = int(per_row.argmax())
    S, h, L = per_row.shape
    return float(per_row.flatten()[i]), (i // (h * L), (i // L) % h, i % L)


def check_case(hip, L, hd, spread, klim, seed, spiky=False, tag=""):
    """Both layouts (same bits), the canaries, single (sequence, head) pairs alone, and every elementwise bound of the module docstring."""
    qs, k, v, d_o, scale = make_inputs(L, hd, spread, seed, spiky=spiky)
    a = run_kernels(hip, qs, k, v, d_o, klim, scale, "A")
    b = run_kernels(hip, qs, k, v, d_o, klim, scale, "B")
    for name in ("o", "lse", "delta", "dq", "dk", "dv"):
        assert torch.equal(a[name].view(torch.int16 if name in ("o", "dq", "dk", "dv") else torch.int32),
                           b[name].view(torch.int16 if name in ("o", "dq", "dk", "dv") else torch.int32)), f"{name}: the strided layout differs from the contiguous one"
    for s, hh in ((0, 1), (1, 2)):  # a pair alone, from copies of its slices, gives the bits it has inside the S = 2, heads = 3 call
        one = run_kernels(hip, *(t[s:s + 1, hh:hh + 1].clone() for t in (qs, k, v, d_o)), klim, scale, "B")
        for name in ("o", "lse", "delta", "dq", "dk", "dv"):
            x, y = one[name][0, 0], a[name][s, hh]
            assert torch.equal(x.view(torch.int16 if x.dtype == torch.int16 else torch.int32), y.view(torch.int16 if y.dtype == torch.int16 else torch.int32)), \
                f"{name} of (sequence {s}, head {hh}) alone differs from the same pair inside the batched call"
    o_k = _f64(a["o"])
    r = restate(qs, k, v, d_o, klim, scale, o_for_delta=o_k)
    eps = 2.0 ** -7
    checks = {
        "lse": ((a["lse"].to(F64) - r["lse"]).abs(), 1.5 * 2.0 ** -9 + LSE_BINADE + hd * 2.0 ** -23 * r["smax"]),
        "delta": ((a["delta"].to(F64) - r["delta"]).abs(), hd * 2.0 ** -23 * (d_o.to(F64).abs() * o_k.abs()).sum(-1)),
        "o": ((o_k - r["o"]).abs(), eps * r["A_o"] + 2.0 ** -9 * r["o"].abs()),
        "dq": ((_f64(a["dq"]) - r["dq"]).abs(), eps * r["A_dq"] + 2.0 ** -9 * r["dq"].abs() + r["C_dq"]),
        "dk": ((_f64(a["dk"]) - r["dk"]).abs(), eps * r["A_dk"] + 2.0 ** -9 * r["dk"].abs() + r["C_dk"]),
        "dv": ((_f64(a["dv"]) - r["dv"]).abs(), eps * r["A_dv"] + 2.0 ** -9 * r["dv"].abs()),
    }
    worst = {name: _worst(err, bound) for name, (err, bound) in checks.items()}
    print(f"\n[contract] hd={hd} masked={int(klim is not None)} L={L} {tag} " + " ".join(f"{n}={w[0]:.3f}@{w[1]}" for n, w in worst.items()))
    bad = {n: w for n, w in worst.items() if not w[0] <= 1.0}
    assert not bad, f"error / bound above 1 at (sequence, head, row): {bad} (all: {worst})"
    return a, (qs, k, v, d_o, scale)


@gpu
@pytest.mark.parametrize("spread", [1.0, 4.0])
@pytest.mark.parametrize("hd", [64, 96])
@pytest.mark.parametrize("L", [1, 31, 33, 63, 64, 65, 127, 128, 129, 193, 257])
def test_unmasked_rows_meet_their_bounds_in_both_layouts(hip, L, hd, spread):
    """The 32-row wave, the 64-row streamed tile and the 128-row workgroup at -1, 0, +1, and a third workgroup; flat and peaked rows."""
    check_case(hip, L, hd, spread, None, seed=1000 * hd + 10 * L + int(spread), tag=f"spread={spread}")


@gpu
@pytest.mark.parametrize("hd", [64, 96])
def test_unmasked_spiky_rows_meet_their_bounds(hip, hd):
    """Late keys aligned with queries 5 and 77: the running max jumps by far more than 2^8 after most of the row sum was taken."""
    check_case(hip, 257, hd, 1.0, None, seed=9 + hd, spiky=True, tag="spiky")


KINDS = ["all_L", "all_1", "staircase", "staircase_capped"]


@gpu
@pytest.mark.parametrize("hd", [64, 96])
@pytest.mark.parametrize("L,kind", [(L, kd) for L in (40, 129, 257) for kd in KINDS] + [(257, "late_jump")])
def test_key_limits_meet_their_bounds_in_both_layouts(hip, L, kind, hd):
    """Limits the header allows: all L, all 1, a staircase off every multiple of 4 (steps inside a 32-row block and a 64-key tile), the
    same capped at L - 9 (keys nobody sees: dk = dv = 0 WRITTEN over the whole width), and for L = 257 limit 100 below row 200 (a
    128-key workgroup skips its leading query tiles, the dq workgroups stop early). Then the backward counterpart of the forward's
    independence check: dq and delta of the queries below the first step keep their bits when the keys and values they cannot see, and the
    dO rows of the other queries, are perturbed. The backward kernels are what is under test, so they get the first run's o and lse: the
    FORWARD's bits of such a row are not independent of unseen data (found here with the late jump, rows 192..199: the deferred rescale
    is decided per wave, so a row whose wave-mates see a perturbed key can be re-based by 2^-delta at another tile - the same value
    within every bound above, other bits), and through lse that would move dq as well."""
    klim = key_limits(L, kind)
    a, (qs, k, v, d_o, scale) = check_case(hip, L, hd, 2.0, klim, seed=77 * hd + L + len(kind), tag=kind)
    if kind == "staircase_capped":
        for name in ("dk", "dv"):
            assert (_f64(a[name])[:, :, L - 9:] == 0).all(), f"{name} rows of keys that no query sees are not 0"
    first_limit = int(klim[0])
    first_step = int((klim != klim[0]).nonzero()[0]) if bool((klim != klim[0]).any()) else L
    k2, v2, do2 = k.clone(), v.clone(), d_o.clone()
    k2[:, :, first_limit:] = (k2[:, :, first_limit:].float() + 1.0).bfloat16()
    v2[:, :, first_limit:] = (v2[:, :, first_limit:].float() - 1.0).bfloat16()
    do2[:, :, first_step:] = (do2[:, :, first_step:].float() * 1.5 + 0.25).bfloat16()
    if first_limit < L or first_step < L:
        again = run_kernels(hip, qs, k2, v2, do2, klim, scale, "A", forward_of=a)
        for name in ("delta", "dq"):
            x, y = again[name][:, :, :first_step], a[name][:, :, :first_step]
            bits = torch.int16 if x.dtype == torch.int16 else torch.int32
            assert torch.equal(x.contiguous().view(bits), y.contiguous().view(bits)), f"{name} of the queries below the first step moved with data they cannot see"


# ---------------------------------------------------------------------------------------------------------------------
# 6. `parts` of nova_row_norm_bwd
# ---------------------------------------------------------------------------------------------------------------------
def test_row_norm_bwd_refuses_bad_parts_before_any_launch():
    """parts must be a positive multiple of 4 (one partial row per wave, four waves per workgroup): 6 and 0 are refused by the argument
    checks, which run before any device work (no GPU needed; the pointers are never dereferenced)."""
    from nova_pointcloud_amd import hip

    lib = hip.load(check_device=False)
    fn = lib.nova_row_norm_bwd
    p = [ctypes.c_void_p(4096 * (i + 1)) for i in range(7)]  # x, dy, gamma, beta, dx, dgamma_part, dbeta_part
    args = lambda parts, dtype: (p[0], p[1], p[2], p[3], None, 0, -1, -1, -1, p[4], None, p[5], p[6], parts, 5, 128, 1e-5, dtype, None)
    for dtype in (hip.F32, hip.BF16):
        for parts in (6, 0, -4, 1023):
            assert fn(*args(parts, dtype)) == -1, (parts, dtype)
            assert b"parts" in lib.nova_last_error()


def _norm_bwd(hip, x, dy, gamma, beta, parts):
    rows, D = x.shape
    dx = torch.empty_like(x)
    dg = torch.full((parts, D), float("nan"), dtype=torch.float32, device=DEV)
    db = torch.full((parts, D), float("nan"), dtype=torch.float32, device=DEV)
    hip.call("nova_row_norm_bwd", hip.ptr(x), hip.ptr(dy), hip.ptr(gamma), hip.ptr(beta), None, 0, -1, -1, -1, hip.ptr(dx), None, hip.ptr(dg),
             hip.ptr(db), parts, rows, D, 1e-5, hip.dtype_code(x.dtype), hip.stream_ptr())
    torch.cuda.synchronize()
    return dx.cpu(), dg.cpu(), db.cpu()


@gpu
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("D", [128, 1536])
@pytest.mark.parametrize("rows", [1, 5, 1025])
def test_row_norm_bwd_partial_rows_for_any_parts(hip, rows, D, dtype):
    """parts in {4, 64, 1024} (autograd.py only ever passes min(1024, rows rounded up to 4)): every partial row is written and finite -
    the waves that own no row write zeros -, their sum over dim 0 is the float64 d_gamma = sum_rows dy * n and d_beta = sum_rows dy
    (on the stored values of x and dy) within rows * 2^-23 * sum_rows |term|, dx does not depend on parts bit for bit, and a second
    identical call returns identical bits."""
    g = torch.Generator().manual_seed(rows + D)
    x = (torch.randn(rows, D, generator=g) * 1.5 + 0.3).to(dtype)
    dy = torch.randn(rows, D, generator=g).to(dtype)
    gamma, beta = 1 + 0.2 * torch.randn(D, generator=g), 0.2 * torch.randn(D, generator=g)
    x64, dy64 = x.to(F64), dy.to(F64)
    mu = x64.mean(-1, keepdim=True)
    n = (x64 - mu) / torch.sqrt(((x64 - mu) ** 2).mean(-1, keepdim=True) + 1e-5)
    ref = {"d_gamma": (dy64 * n).sum(0), "d_beta": dy64.sum(0)}
    bound = {"d_gamma": rows * 2.0 ** -23 * (dy64 * n).abs().sum(0), "d_beta": rows * 2.0 ** -23 * dy64.abs().sum(0)}
    xd, dyd, gd, bd = x.cuda(), dy.cuda(), gamma.cuda(), beta.cuda()
    dx0, worst = None, {}
    for parts in (4, 64, 1024):
        dx, dg, db = _norm_bwd(hip, xd, dyd, gd, bd, parts)
        dx_again, dg_again, db_again = _norm_bwd(hip, xd, dyd, gd, bd, parts)
        bits = torch.int32 if dtype == torch.float32 else torch.int16
        assert torch.equal(dx.view(bits), dx_again.view(bits)) and torch.equal(dg.view(torch.int32), dg_again.view(torch.int32)) \
            and torch.equal(db.view(torch.int32), db_again.view(torch.int32)), f"parts={parts}: two identical calls differ"
        assert torch.isfinite(dg).all() and torch.isfinite(db).all(), f"parts={parts}: a partial row was not written"
        if parts > rows:
            assert (dg[rows:] == 0).all() and (db[rows:] == 0).all(), f"parts={parts}: a wave that owns no row wrote something other than 0"
        if dx0 is None:
            dx0 = dx
        assert torch.equal(dx.view(bits), dx0.view(bits)), f"dx depends on parts ({parts} against 4)"
        for name, part in (("d_gamma", dg), ("d_beta", db)):
            err = (part.to(F64).sum(0) - ref[name]).abs()
            ratio = torch.where(bound[name] > 0, err / bound[name].clamp_min(1e-300), torch.where(err > 0, torch.full_like(err, float("inf")), torch.zeros_like(err)))
            worst[(name, parts)] = (float(ratio.max()), int(ratio.argmax()))
    print(f"\n[contract] row_norm_bwd rows={rows} D={D} {dtype} " + " ".join(f"{n}/{p}={w[0]:.3f}@{w[1]}" for (n, p), w in worst.items()))
    bad = {kp: w for kp, w in worst.items() if not w[0] <= 1.0}
    assert not bad, f"error / bound above 1 at (column): {bad}"
