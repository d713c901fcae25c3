"""Cross-length training attention on the GPU: `nova_attn_cross_fwd_lse` / `nova_attn_cross_bwd` (the (Lq, Lk) forms of
`attn_delta_kernel`, `attn_bwd_dq`, `attn_bwd_dkv` of csrc/attn_bwd.hip and the LSE / MASK forwards of csrc/attn16.hip) held
to their C contract with raw pointers, then `autograd.attention`, `attention.MultiheadAttention` and `attention.EdgeAligner`.

Every output of the two entry points - o, lse, delta, dq, dk, dv - is compared ELEMENTWISE in float64 with
`restate_cross` (tests/test_attn_cross_cpu.py, pinned there to float64 autograd of F.scaled_dot_product_attention) under the
bounds of the module docstring of tests/test_gpu_attn_train_contract.py, unchanged: they come from the kernels' arithmetic,
which has no notion of which of the two lengths a loop bound came from. At Lq == Lk with equal strides the six outputs are
bit for bit those of `nova_attn_fwd_lse` / `nova_attn_bwd`.

Measured worst error / bound on an MI355X (this file's own cases; `[cross]` lines of a `-s` run):
  unmasked, head_dim 64:  lse 0.79  delta 0.01  o 0.60  dq 0.69  dk 0.81  dv 0.80
  unmasked, head_dim 96:  lse 0.80  delta 0.01  o 0.56  dq 0.79  dk 0.76  dv 0.80
  masked,   head_dim 64:  lse 0.63  delta 0.01  o 0.49  dq 0.58  dk 0.70  dv 0.71
  masked,   head_dim 96:  lse 0.66  delta 0.01  o 0.45  dq 0.67  dk 0.72  dv 0.70
  EdgeAligner(256, 4), bf16 against the literal float32 form, error / largest entry: output 0.003, feature gradients 0.005 .. 0.010,
  parameter gradients 0.003 .. 0.008 (bound 3e-2).
"""
import pytest
import torch

from test_attn_cross_cpu import make_cross_inputs, restate_cross, staircase_cross
from test_gpu_attn_train_contract import F64, LSE_BINADE, _Buf, _f64, _worst, staircase

pytestmark = pytest.mark.gpu
DEV = "cuda"
NAMES = ("o", "lse", "delta", "dq", "dk", "dv")


def _bits(t):
    return t.contiguous().view(torch.int16 if t.dtype == torch.int16 else torch.int32)


def run_cross(hip, qs, k, v, d_o, klim, scale, layout, api="cross"):
    """Forward with lse, then backward, with raw pointers. layout "A": eight contiguous buffers, every stride h * hd. layout "P": q~ at row
    stride D + 64, k | v halves of one [S Lk + 2, 2 D] buffer, o at D + 64, dO at D + 128, dq at D + 192, dk | dv halves of one
    [S Lk + 2, 2 D] buffer. layout "QKV" (Lq == Lk only): q~ | k | v thirds of one [S L + 2, 3 D] buffer, o at D + 64, dO at D + 128,
    dq | dk | dv thirds of one buffer - the packed layout of the self-attention entry points, equal strides on both sides. Every buffer has
    two spare rows and is pre-filled with the NaN canary, lse / delta with NaN. api "cross": the two new entry points; "self": nova_attn_fwd_lse /
    nova_attn_bwd (Lq == Lk, equal strides). Returns host tensors: o, dq, dk, dv as int16 bit patterns, lse / delta f32 [S, h, Lq]."""
    S, h, Lq, hd = qs.shape
    Lk = k.shape[2]
    D, nq, nk = h * hd, S * Lq, S * Lk
    if layout == "A":
        bq, bo, bdo, bdq = (_Buf(nq, D) for _ in range(4))
        bk, bv, bdk, bdv = (_Buf(nk, D) for _ in range(4))
        ck = cv = cdk = cdv = cq = cdq = 0
        q_rs = kv_rs = o_rs = do_rs = dq_rs = dkv_rs = D
    elif layout == "P":
        bq, bo, bdo, bdq = _Buf(nq, D + 64), _Buf(nq, D + 64), _Buf(nq, D + 128), _Buf(nq, D + 192)
        bk = bv = _Buf(nk, 2 * D)
        bdk = bdv = _Buf(nk, 2 * D)
        cq = cdq = 0
        ck, cv, cdk, cdv = 0, D, 0, D
        q_rs, kv_rs, o_rs, do_rs, dq_rs, dkv_rs = D + 64, 2 * D, D + 64, D + 128, D + 192, 2 * D
    else:
        assert layout == "QKV" and Lq == Lk
        bq = bk = bv = _Buf(nq, 3 * D)
        bdq = bdk = bdv = _Buf(nq, 3 * D)
        bo, bdo = _Buf(nq, D + 64), _Buf(nq, D + 128)
        cq, ck, cv, cdq, cdk, cdv = 0, D, 2 * D, 0, D, 2 * D
        q_rs = kv_rs = dq_rs = dkv_rs = 3 * D
        o_rs, do_rs = D + 64, D + 128
    bq.put(cq, qs), bk.put(ck, k), bv.put(cv, v), bdo.put(0, d_o)
    bo.claim(0, D), bdq.claim(cdq, D), bdk.claim(cdk, D), bdv.claim(cdv, D)
    lse = torch.full((S, h, Lq), float("nan"), dtype=torch.float32, device=DEV)
    delta = torch.full((S, h, Lq), float("nan"), dtype=torch.float32, device=DEV)
    kl = None if klim is None else klim.to(torch.int32).cuda()
    ptrs = (bq.ptr(hip, cq), bk.ptr(hip, ck), bv.ptr(hip, cv), bo.ptr(hip))
    grads = (bdq.ptr(hip, cdq), bdk.ptr(hip, cdk), bdv.ptr(hip, cdv))
    if api == "cross":
        hip.call("nova_attn_cross_fwd_lse", *ptrs, hip.ptr(lse), S, h, Lq, Lk, hd, q_rs, kv_rs, o_rs, hip.ptr(kl), hip.stream_ptr())
        hip.call("nova_attn_cross_bwd", *ptrs, bdo.ptr(hip), hip.ptr(lse), hip.ptr(delta), *grads, S, h, Lq, Lk, hd, q_rs, kv_rs, o_rs, do_rs,
                 dq_rs, dkv_rs, float(scale), hip.ptr(kl), hip.stream_ptr())
    else:
        assert api == "self" and Lq == Lk and q_rs == kv_rs and dq_rs == dkv_rs
        hip.call("nova_attn_fwd_lse", *ptrs, hip.ptr(lse), S, h, Lq, hd, q_rs, o_rs, hip.ptr(kl), hip.stream_ptr())
        hip.call("nova_attn_bwd", *ptrs, bdo.ptr(hip), hip.ptr(lse), hip.ptr(delta), *grads, S, h, Lq, hd, q_rs, o_rs, do_rs, dq_rs, float(scale),
                 hip.ptr(kl), hip.stream_ptr())
    torch.cuda.synchronize()
    for name, b in (("q", bq), ("k | v", bk), ("o", bo), ("dO", bdo), ("dq", bdq), ("dk | dv", bdk)):
        assert b.untouched(), f"layout {layout}: a gap column or spare row of the {name} buffer lost its fill pattern"
    out = dict(o=bo.get(0, S, h, Lq, hd), dq=bdq.get(cdq, S, h, Lq, hd), dk=bdk.get(cdk, S, h, Lk, hd), dv=bdv.get(cdv, S, h, Lk, hd),
               lse=lse.cpu(), delta=delta.cpu())
    assert torch.isfinite(out["lse"]).all(), f"layout {layout}: an lse entry was not written"
    assert torch.isfinite(out["delta"]).all(), f"layout {layout}: a delta entry was not written"
    for name in ("o", "dq", "dk", "dv"):
        assert torch.isfinite(_f64(out[name])).all(), f"layout {layout}: an entry of {name} was not written (or is not finite)"
    return out


def check_cross_case(hip, Lq, Lk, hd, spread, klim, seed, tag=""):
    """Both layouts (same bits), the canaries, single (sequence, head) pairs alone, and every elementwise bound of the contract."""
    qs, k, v, d_o, scale = make_cross_inputs(Lq, Lk, hd, spread, seed)
    a = run_cross(hip, qs, k, v, d_o, klim, scale, "A")
    b = run_cross(hip, qs, k, v, d_o, klim, scale, "P")
    for name in NAMES:
        assert torch.equal(_bits(a[name]), _bits(b[name])), f"{name}: the packed layout differs from the contiguous one"
    for s, hh in ((0, 1), (1, 2)):  # a pair alone, from copies of its slices, gives the bits it has inside the S = 2, heads = 3 call
        one = run_cross(hip, *(t[s:s + 1, hh:hh + 1].clone() for t in (qs, k, v, d_o)), klim, scale, "P")
        for name in NAMES:
            assert torch.equal(_bits(one[name][0, 0]), _bits(a[name][s, hh])), \
                f"{name} of (sequence {s}, head {hh}) alone differs from the same pair inside the batched call"
    o_k = _f64(a["o"])
    r = restate_cross(qs, k, v, d_o, klim, scale, o_for_delta=o_k)
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
    print(f"\n[cross] hd={hd} masked={int(klim is not None)} Lq={Lq} Lk={Lk} {tag} " + " ".join(f"{n}={w[0]:.3f}@{w[1]}" for n, w in worst.items()))
    bad = {n: w for n, w in worst.items() if not w[0] <= 1.0}
    assert not bad, f"error / bound above 1 at (sequence, head, row): {bad} (all: {worst})"
    return a


# ---------------------------------------------------------------------------------------------------------------------
# e. contract at cross lengths
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("spread", [1.0, 4.0])
@pytest.mark.parametrize("hd", [64, 96])
@pytest.mark.parametrize("Lq,Lk", [(1, 129), (129, 1), (31, 65), (65, 31), (64, 128), (128, 64), (127, 257), (257, 127), (102, 306)])
def test_cross_rows_meet_their_bounds_in_both_layouts(hip, Lq, Lk, hd, spread):
    """One query against a third key workgroup's first row and the reverse; the 32-row wave, the 64-row streamed tile and the 128-row
    workgroup at -1, 0, +1 on either side with the other side on the other side of it; 102 queries against three subsets' keys. Flat
    and peaked rows. With Lk = 1 P is 1, dq and dk are 0 up to the f32 cancellation term, which the bound carries."""
    check_cross_case(hip, Lq, Lk, hd, spread, None, seed=100000 * hd + 300 * Lq + Lk + int(spread), tag=f"spread={spread}")


# ---------------------------------------------------------------------------------------------------------------------
# f. equal lengths: the bits of the self-attention entry points
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("masked", [False, True])
@pytest.mark.parametrize("hd", [64, 96])
@pytest.mark.parametrize("L", [33, 129, 257])
def test_cross_entry_points_at_equal_lengths_return_the_self_attention_bits(hip, L, hd, masked):
    """Lq = Lk = L, q~ | k | v thirds of one buffer (equal strides on both sides): o, lse, delta, dq, dk, dv of the cross entry points
    are bit for bit those of nova_attn_fwd_lse + nova_attn_bwd."""
    qs, k, v, d_o, scale = make_cross_inputs(L, L, hd, 2.0, seed=31 * L + hd + int(masked))
    klim = staircase(L) if masked else None
    new = run_cross(hip, qs, k, v, d_o, klim, scale, "QKV", api="cross")
    old = run_cross(hip, qs, k, v, d_o, klim, scale, "QKV", api="self")
    for name in NAMES:
        assert torch.equal(_bits(new[name]), _bits(old[name])), f"{name}: the cross entry points moved a bit at Lq == Lk == {L}"


# ---------------------------------------------------------------------------------------------------------------------
# g. key limits at cross lengths
# ---------------------------------------------------------------------------------------------------------------------
def cross_key_limits(Lq, Lk, kind):
    if kind == "all_Lk":
        return torch.full((Lq,), Lk, dtype=torch.int32)
    if kind == "all_1":
        return torch.ones(Lq, dtype=torch.int32)
    if kind == "staircase":
        return staircase_cross(Lq, Lk)
    assert kind == "staircase_capped"
    return staircase_cross(Lq, Lk, cap=Lk - 9)


@pytest.mark.parametrize("hd", [64, 96])
@pytest.mark.parametrize("kind", ["all_Lk", "all_1", "staircase", "staircase_capped"])
@pytest.mark.parametrize("Lq,Lk", [(40, 129), (257, 100)])
def test_cross_key_limits_meet_their_bounds_in_both_layouts(hip, Lq, Lk, kind, hd):
    """Limits the header allows at Lq != Lk: all Lk, all 1, a staircase with steps off every multiple of 4, the same capped at Lk - 9 (keys
    nobody sees: dk = dv = 0 WRITTEN over the whole width; the canary check of run_cross shows they were written at all)."""
    klim = cross_key_limits(Lq, Lk, kind)
    assert int(klim.min()) >= 1 and int(klim.max()) <= Lk and bool((klim[1:] >= klim[:-1]).all())
    a = check_cross_case(hip, Lq, Lk, hd, 2.0, klim, seed=77 * hd + 1000 * Lq + Lk + len(kind), tag=kind)
    unseen = int(klim.max())
    if unseen < Lk:
        for name in ("dk", "dv"):
            assert (_f64(a[name])[:, :, unseen:] == 0).all(), f"{name} rows of keys that no query sees are not 0"
    if kind == "staircase_capped":
        assert unseen == Lk - 9


# ---------------------------------------------------------------------------------------------------------------------
# d (device part). key_limit_of_mask on rectangular masks
# ---------------------------------------------------------------------------------------------------------------------
def test_key_limit_of_mask_takes_rectangular_staircases_only(hip):
    from nova_pointcloud_amd import autograd as A

    Lq, Lk = 40, 129
    klim = staircase_cross(Lq, Lk)
    vis = torch.arange(Lk)[None, :] < klim.to(torch.int64)[:, None]
    for mask in (vis.cuda(), torch.zeros(Lq, Lk).masked_fill(~vis, float("-inf")).cuda()):
        got = A.key_limit_of_mask(mask)
        assert got is not None and got.dtype == torch.int32 and torch.equal(got.cpu(), klim)
        q, k = (torch.zeros(1, 1, n, 64, dtype=torch.bfloat16, device=DEV) for n in (Lq, Lk))
        assert A.attention_supported(q, mask, k) and not A.attention_supported(q, mask) and not A.attention_supported(k, mask, q)
    down = klim.clone()
    down[10] = down[9] - 1  # a decreasing step
    assert A.key_limit_of_mask((torch.arange(Lk)[None, :] < down.to(torch.int64)[:, None]).cuda()) is None
    holes = vis.clone()
    holes[20, 2] = False  # not a prefix
    assert A.key_limit_of_mask(holes.cuda()) is None
    none = vis.clone()
    none[0, :] = False  # a limit of 0
    assert A.key_limit_of_mask(none.cuda()) is None
    # limits above Lk cannot be written as an [Lq, Lk] mask; the attention refuses a mask made for more keys than it is given
    wide = (torch.arange(Lk + 5)[None, :] < (klim.to(torch.int64) + 5)[:, None]).cuda()
    q, k = (torch.zeros(1, 1, n, 64, dtype=torch.bfloat16, device=DEV) for n in (Lq, Lk))
    assert not A.attention_supported(q, wide, k)
    with pytest.raises(ValueError):
        A.attention(q, k, k, attn_mask=wide)


# ---------------------------------------------------------------------------------------------------------------------
# h. autograd
# ---------------------------------------------------------------------------------------------------------------------
def _rel(got, ref):
    return ((got.float() - ref.float()).abs().max() / ref.float().abs().max().clamp_min(1e-12)).item()


@pytest.mark.parametrize("S,h,Lq,Lk", [(1, 1, 64, 200), (2, 3, 102, 306), (1, 2, 333, 31), (3, 2, 31, 1031)])
@pytest.mark.parametrize("spread", [1.0, 4.0])
@pytest.mark.parametrize("hd", [64, 96])
def test_cross_attention_forward_backward_match_autograd(hip, S, h, Lq, Lk, spread, hd, monkeypatch):
    """autograd.attention(q, k, v) with Lk != Lq against F.scaled_dot_product_attention differentiated in float32 on the same bf16
    values, under the bounds of tests/test_gpu_train_kernels.py; it goes through the cross entry points and counts as a call."""
    from nova_pointcloud_amd import autograd as A

    g = torch.Generator().manual_seed(S * 1000 + h * 100 + Lq + 7 * Lk + hd)
    mk = lambda L, s: (torch.randn(S, h, L, hd, generator=g) * s).bfloat16().cuda()
    q, k, v, d_out = mk(Lq, spread), mk(Lk, 1.0), mk(Lk, 1.0), mk(Lq, 1.0)
    q, k, v = (t.requires_grad_(True) for t in (q, k, v))
    assert A.attention_supported(q, None, k)
    names, real = [], hip.call
    monkeypatch.setattr(hip, "call", lambda name, *a: (names.append(name), real(name, *a))[1])
    before = A.stats["attention_calls"]
    out = A.attention(q, k, v)
    out.backward(d_out)
    assert A.stats["attention_calls"] == before + 1 and names == ["nova_attn_cross_fwd_lse", "nova_attn_cross_bwd"]
    qf, kf, vf = (t.detach().float().requires_grad_(True) for t in (q, k, v))
    ref = torch.nn.functional.scaled_dot_product_attention(qf, kf, vf)
    ref.backward(d_out.float())
    assert out.shape == (S, h, Lq, hd) and q.grad.shape == q.shape and k.grad.shape == k.shape and v.grad.shape == v.shape
    assert _rel(out, ref.detach()) < 1.6e-2
    for name, got, want in (("dq", q.grad, qf.grad), ("dk", k.grad, kf.grad), ("dv", v.grad, vf.grad)):
        assert torch.isfinite(got.float()).all(), name
        assert _rel(got, want) < 2e-2, (name, _rel(got, want))


def test_equal_lengths_still_take_the_self_attention_entry_points(hip, monkeypatch):
    from nova_pointcloud_amd import autograd as A

    g = torch.Generator().manual_seed(4)
    q, k, v = ((torch.randn(2, 3, 70, 64, generator=g)).bfloat16().cuda().requires_grad_(True) for _ in range(3))
    names, real = [], hip.call
    monkeypatch.setattr(hip, "call", lambda name, *a: (names.append(name), real(name, *a))[1])
    A.attention(q, k, v).float().square().mean().backward()
    assert names == ["nova_attn_fwd_lse", "nova_attn_bwd"]


def test_cross_attention_with_a_rectangular_mask_matches_autograd(hip):
    """The [Lq, Lk] key-limit mask through autograd.attention against SDPA with the same boolean mask (bounds as above)."""
    from nova_pointcloud_amd import autograd as A

    S, h, Lq, Lk, hd = 2, 3, 102, 306, 64
    g = torch.Generator().manual_seed(12)
    mk = lambda L: torch.randn(S, h, L, hd, generator=g).bfloat16().cuda()
    q, k, v, d_out = mk(Lq), mk(Lk), mk(Lk), mk(Lq)
    q, k, v = (t.requires_grad_(True) for t in (q, k, v))
    mask = (torch.arange(Lk)[None, :] < staircase_cross(Lq, Lk, cap=Lk - 9).to(torch.int64)[:, None]).cuda()
    assert A.attention_supported(q, mask, k)
    out = A.attention(q, k, v, attn_mask=mask)
    out.backward(d_out)
    qf, kf, vf = (t.detach().float().requires_grad_(True) for t in (q, k, v))
    ref = torch.nn.functional.scaled_dot_product_attention(qf, kf, vf, attn_mask=mask)
    ref.backward(d_out.float())
    assert _rel(out, ref.detach()) < 1.6e-2
    for name, got, want in (("dq", q.grad, qf.grad), ("dk", k.grad, kf.grad), ("dv", v.grad, vf.grad)):
        assert _rel(got, want) < 2e-2, (name, _rel(got, want))
    assert (k.grad[:, :, Lk - 9:] == 0).all() and (v.grad[:, :, Lk - 9:] == 0).all()


# ---------------------------------------------------------------------------------------------------------------------
# i. MultiheadAttention
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("m", [410, None], ids=["cross", "self"])
def test_multihead_attention_trains_through_hip_kernels(hip, m):
    """MultiheadAttention(256, 4) in bf16, cross (n = 150, m = 410) and self, against torch.nn.MultiheadAttention(256, 4,
    batch_first=True) in float32 with the same state_dict: output, input gradients and every parameter gradient within 3e-2 of the
    largest entry (the bound of test_attention_module_trains_through_hip_kernels), and the HIP attention was reached."""
    from nova_pointcloud_amd import autograd as A
    from nova_pointcloud_amd.attention import MultiheadAttention

    torch.manual_seed(5)
    mod = MultiheadAttention(256, 4).cuda().bfloat16()
    with torch.no_grad():
        mod.in_proj_bias.copy_(torch.randn(768) * 0.1), mod.out_proj.bias.copy_(torch.randn(256) * 0.1)
    n = 150
    x = (torch.randn(2, n, 256) * 0.7).bfloat16().cuda()
    y = None if m is None else (torch.randn(2, m, 256) * 0.7).bfloat16().cuda()
    before = A.stats["attention_calls"]
    xa = x.clone().requires_grad_(True)
    ya = xa if m is None else y.clone().requires_grad_(True)
    out, weights = mod(xa, ya, ya)
    assert weights is None and out.dtype == torch.bfloat16 and out.shape == (2, n, 256)
    out.float().square().mean().backward()
    assert A.stats["attention_calls"] == before + 1, "the training forward did not reach the HIP attention"
    got = {name: p.grad.float().clone() for name, p in mod.named_parameters()}
    ref_mod = torch.nn.MultiheadAttention(256, 4, batch_first=True).cuda().float()
    ref_mod.load_state_dict({name: t.float() for name, t in mod.state_dict().items()}, strict=True)
    xb = x.float().requires_grad_(True)
    yb = xb if m is None else y.float().requires_grad_(True)
    ref, _ = ref_mod(xb, yb, yb, need_weights=False)
    ref.square().mean().backward()
    assert _rel(out.detach(), ref.detach()) < 3e-2
    assert _rel(xa.grad, xb.grad) < 3e-2
    if m is not None:
        assert _rel(ya.grad, yb.grad) < 3e-2
    for name, p in ref_mod.named_parameters():
        assert _rel(got[name], p.grad) < 3e-2, (name, _rel(got[name], p.grad))


# ---------------------------------------------------------------------------------------------------------------------
# j. EdgeAligner
# ---------------------------------------------------------------------------------------------------------------------
class _LiteralEdgeAligner(torch.nn.Module):
    """The literal torch form: cdist, topk, gather, mean, nn.MultiheadAttention, nn.Linear (what the reference's comments describe)."""

    def __init__(self, embed_dim, num_heads):
        super().__init__()
        self.biattn = torch.nn.MultiheadAttention(embed_dim, num_heads, batch_first=True)
        self.edge_mlp = torch.nn.Sequential(torch.nn.Linear(embed_dim, embed_dim // 2), torch.nn.ReLU(), torch.nn.Linear(embed_dim // 2, embed_dim))
        self.spatial_embed = torch.nn.Linear(3, embed_dim)

    @staticmethod
    def edge(points, features):
        idx = torch.topk(torch.cdist(points.float(), points.float()), k=min(8, points.shape[1]), dim=-1, largest=False).indices  # [B, N, k]
        B, N, C = features.shape
        nb = torch.gather(features[:, None].expand(B, N, N, C), 2, idx[..., None].expand(B, N, idx.shape[-1], C))
        return features - nb.mean(dim=2)

    def forward(self, cp, cf, nps, nfs):
        cur = self.edge(cp, cf)
        others = [self.edge(p, f) for p, f in zip(nps, nfs)]
        everything = torch.cat(others, dim=1) if others else cur
        aligned, _ = self.biattn(cur, everything, everything, need_weights=False)
        return aligned + self.spatial_embed(cp.to(aligned.dtype))


def _aligner_run(mod, dtype, cp, cf, nps, nfs, w):
    cfa = cf.to(dtype).clone().requires_grad_(True)
    nfa = [f.to(dtype).clone().requires_grad_(True) for f in nfs]
    out = mod(cp, cfa, nps, nfa)
    (out.float() * w).sum().backward()
    res = {"out": out.detach().float(), "d_current": cfa.grad.float()}
    for i, f in enumerate(nfa):
        res[f"d_neighbor{i}"] = f.grad.float()
    for name, p in mod.named_parameters():
        if p.grad is not None:
            res[name] = p.grad.float().clone()
    mod.zero_grad()
    return res


def test_edge_aligner_matches_the_literal_torch_form(hip):
    """EdgeAligner(256, 4) in bf16, a current subset of 102 points and three neighbour subsets, against the literal float32 torch form
    with the same state_dict: output, feature gradients and parameter gradients within 3e-2 of the largest entry; edge_mlp gets no
    gradient in either. An empty neighbour list attends over the current edge features."""
    from nova_pointcloud_amd import autograd as A
    from nova_pointcloud_amd.attention import EdgeAligner

    torch.manual_seed(21)
    ours = EdgeAligner(256, 4).cuda().bfloat16()
    with torch.no_grad():
        ours.biattn.in_proj_bias.copy_(torch.randn(768) * 0.1), ours.biattn.out_proj.bias.copy_(torch.randn(256) * 0.1)
    ref = _LiteralEdgeAligner(256, 4).cuda().float()
    ref.load_state_dict({name: t.float() for name, t in ours.state_dict().items()}, strict=True)
    B, n = 2, 102
    cp, cf = torch.rand(B, n, 3).cuda(), (torch.randn(B, n, 256) * 0.7).cuda()
    nps = [torch.rand(B, m, 3).cuda() for m in (102, 102, 103)]
    nfs = [(torch.randn(B, p.shape[1], 256) * 0.7).cuda() for p in nps]
    # the features both forms see are the bf16-rounded ones
    cf, nfs = cf.bfloat16().float(), [f.bfloat16().float() for f in nfs]
    w = torch.randn(B, n, 256).cuda()
    before = A.stats["attention_calls"]
    got = _aligner_run(ours, torch.bfloat16, cp, cf, nps, nfs, w)
    assert A.stats["attention_calls"] == before + 1, "the aligner did not reach the HIP attention"
    want = _aligner_run(ref, torch.float32, cp, cf, nps, nfs, w)
    assert got.keys() == want.keys() and not any(name.startswith("edge_mlp") for name in got)
    worst = {name: _rel(got[name], want[name]) for name in want}
    print("\n[cross] EdgeAligner bf16 against the literal float32 form: " + " ".join(f"{k_}={v_:.4f}" for k_, v_ in worst.items()))
    bad = {k_: v_ for k_, v_ in worst.items() if not v_ < 3e-2}
    assert not bad, (bad, worst)
    # no neighbours yet: query = key = value = the current edge features (equal lengths: the self-attention entry points)
    alone = ours(cp, cf.bfloat16(), [], [])
    alone_ref = ref(cp, cf, [], [])
    assert alone.dtype == torch.bfloat16 and alone.shape == (B, n, 256)
    assert _rel(alone, alone_ref.detach()) < 3e-2
