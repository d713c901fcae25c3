"""Cross-length training attention, the part that needs no GPU: the float64 restatement of include/nova_hip.h for
(Lq, Lk), pinned to torch autograd of F.scaled_dot_product_attention; the refusals of `nova_attn_cross_fwd_lse` /
`nova_attn_cross_bwd`, all decided before any launch; `attention.MultiheadAttention` against torch.nn.MultiheadAttention
in float64; the parameter names of `attention.EdgeAligner`. tests/test_gpu_attn_cross.py holds the kernels to the same
restatement on the GPU."""
import ctypes
import math

import pytest
import torch

LOG2E = 1.4426950408889634
LN2 = math.log(2.0)
F64 = torch.float64


# ---------------------------------------------------------------------------------------------------------------------
# a. the restatement for (Lq, Lk): `restate` of tests/test_gpu_attn_train_contract.py with the two lengths apart
# ---------------------------------------------------------------------------------------------------------------------
def restate_cross(qs, k, v, d_o, klim, scale, o_for_delta=None):
    """Everything the two cross entry points promise, in float64, from q~ (= q * scale * log2 e) and dO [S, h, Lq, hd], k and
    v [S, h, Lk, hd] and the key limit [Lq] (None: no mask). Factor conventions as in the header: dq = scale * dS K (the
    gradient of the UNSCALED q), dk = ln 2 * dS^T q~. delta is sum_c dO * o_for_delta (the forward's own o) or, when that is
    None, on the exact o. Returns o, lse, delta, dq, dk, dv, the absolute companions A_* and the f32 cancellation terms
    C_dq / C_dk, all as `restate` names them."""
    qs, k, v, d_o = (t.to(F64) for t in (qs, k, v, d_o))
    Lq, Lk, hd = qs.shape[-2], k.shape[-2], qs.shape[-1]
    s2 = qs @ k.transpose(-1, -2)
    vis = torch.ones(Lq, Lk, dtype=torch.bool) if klim is None else torch.arange(Lk)[None, :] < klim.to(torch.int64)[:, None]
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


def make_cross_inputs(Lq, Lk, hd, spread, seed, S=2, h=3):
    """bf16 q~ and dO [S, h, Lq, hd], k and v [S, h, Lk, hd] on the host; spread > 1: peaked rows."""
    g = torch.Generator().manual_seed(seed)
    mk = lambda L, s: torch.randn(S, h, L, hd, generator=g) * s
    q, k, v, d_o = mk(Lq, spread), mk(Lk, 1.0), mk(Lk, 1.0), mk(Lq, 1.0)
    scale = hd ** -0.5
    return (q * (scale * LOG2E)).bfloat16(), k.bfloat16(), v.bfloat16(), d_o.bfloat16(), scale


def staircase_cross(Lq, Lk, cap=None):
    """Key limits [Lq] in [1, Lk], non-decreasing, with steps at rows and values off every multiple of 4 (the rows and values of
    `staircase` in tests/test_gpu_attn_train_contract.py, the values cut at Lk); the last three rows see all Lk keys, or,
    capped, `cap` of them (the keys past it are seen by nobody)."""
    rows = [0, 3, 5, 8, 21, 45, 70, 101, 130, 161, 199, 230]
    lims = [1, 1 + 4, 37, 70, 93, 121, 130, 150, 197, 203, 230, Lk]
    kl = torch.empty(Lq, dtype=torch.int32)
    for r0, lim in zip(rows, lims):
        kl[r0:] = min(lim, Lk)
    kl[max(Lq - 3, 0):] = Lk
    return kl if cap is None else kl.clamp(max=cap)


@pytest.mark.parametrize("hd", [64, 96])
@pytest.mark.parametrize("Lq,Lk", [(5, 70), (70, 5), (1, 9), (9, 1)])
def test_cross_restatement_matches_float64_autograd_of_sdpa(Lq, Lk, hd):
    """`restate_cross` against torch autograd of F.scaled_dot_product_attention in float64, differentiated w.r.t. the UNSCALED
    q = q~ / (scale * log2 e): no mask, a staircase ending at Lk and one capped below Lk (at Lk - 2; with a single key no limit
    below Lk exists and the capped staircase is the uncapped one). 1e-10 of each tensor's largest entry (where autograd's dq / dk
    are identically 0 - one visible key - of the largest entry of the cancelling terms, see below); dk / dv rows of unseen keys
    exactly 0 in both."""
    qs, k, v, d_o, scale = make_cross_inputs(Lq, Lk, hd, 2.0, seed=1000 * Lq + Lk + hd, S=2, h=2)
    cap = max(1, Lk - 2)
    for klim in (None, staircase_cross(Lq, Lk), staircase_cross(Lq, Lk, cap=cap)):
        if klim is not None:
            assert klim.shape == (Lq,) and int(klim.min()) >= 1 and int(klim.max()) <= Lk and bool((klim[1:] >= klim[:-1]).all())
        r = restate_cross(qs, k, v, d_o, klim, scale)
        q64 = (qs.to(F64) / (scale * LOG2E)).requires_grad_(True)
        k64, v64 = k.to(F64).requires_grad_(True), v.to(F64).requires_grad_(True)
        mask = None if klim is None else torch.arange(Lk)[None, :] < klim.to(torch.int64)[:, None]
        out = torch.nn.functional.scaled_dot_product_attention(q64, k64, v64, attn_mask=mask)
        out.backward(d_o.to(F64))
        assert r["o"].shape == (2, 2, Lq, hd) and r["dk"].shape == (2, 2, Lk, hd) and r["lse"].shape == (2, 2, Lq)
        # Lk = 1 (or every limit 1): softmax over one key is constant, so autograd's dq and dk are identically 0 and "the largest
        # entry" gives no scale. The restatement forms them as dS = P (dP - delta) with dP = delta up to float64 rounding; there
        # the scale is that of the two terms that cancel, P (|dP| + |delta|), carried through the same product.
        unc = r["p"] * ((d_o.to(F64) @ v.to(F64).transpose(-1, -2)).abs() + r["delta"].abs()[..., None])
        floor = {"dq": scale * (unc @ k.to(F64).abs()), "dk": LN2 * (unc.transpose(-1, -2) @ qs.to(F64).abs())}
        for name, got, ref in (("o", r["o"], out.detach()), ("dq", r["dq"], q64.grad), ("dk", r["dk"], k64.grad), ("dv", r["dv"], v64.grad)):
            err = (got - ref).abs().max().item()
            largest = ref.abs().max().item()
            if largest == 0.0 and name in floor:
                assert Lk == 1 or (klim is not None and int(klim.max()) == 1), (name, Lq, Lk)
                largest = floor[name].max().item()
            assert err <= 1e-10 * largest, (name, Lq, Lk, hd, klim is not None, err)
        s = (q64.detach() @ k64.detach().transpose(-1, -2)) * scale
        if mask is not None:
            s = s.masked_fill(~mask, float("-inf"))
        assert (r["lse"] - torch.logsumexp(s, -1) * LOG2E).abs().max().item() <= 1e-10 * r["lse"].abs().max().item()
        if klim is not None and int(klim[-1]) < Lk:
            assert int(klim[-1]) == cap
            for t in (r["dk"], r["dv"], k64.grad, v64.grad):
                assert (t[:, :, cap:] == 0).all()
            assert r["dv"][:, :, :cap].abs().max() > 0


def test_cross_restatement_is_restate_at_equal_lengths():
    """With Lq == Lk the restatement is the one the self-attention contract test uses, entry by entry."""
    from test_gpu_attn_train_contract import restate, staircase

    qs, k, v, d_o, scale = make_cross_inputs(37, 37, 64, 2.0, seed=3, S=1, h=2)
    for klim in (None, staircase(37)):
        a, b = restate(qs, k, v, d_o, klim, scale), restate_cross(qs, k, v, d_o, klim, scale)
        assert a.keys() == b.keys()
        for name in a:
            assert torch.equal(a[name], b[name]), name


# ---------------------------------------------------------------------------------------------------------------------
# b. the refusals of the two entry points: before any launch (no GPU: the pointers are never dereferenced)
# ---------------------------------------------------------------------------------------------------------------------
ERR_ARG, ERR_SHAPE = -1, -2
P = [ctypes.c_void_p(4096 * (i + 1)) for i in range(10)]  # q, k, v, o, d_o, lse, delta, dq, dk, dv


def _fwd_args(ptrs=None, S=2, heads=3, Lq=5, Lk=9, hd=64, q_rs=192, kv_rs=192, o_rs=192, klim=None):
    p = list(P[:4]) + [P[5]] if ptrs is None else ptrs
    return (*p, S, heads, Lq, Lk, hd, q_rs, kv_rs, o_rs, klim, None)


def _bwd_args(ptrs=None, S=2, heads=3, Lq=5, Lk=9, hd=64, q_rs=192, kv_rs=192, o_rs=192, do_rs=192, dq_rs=192, dkv_rs=192, klim=None):
    p = list(P) if ptrs is None else ptrs
    return (*p, S, heads, Lq, Lk, hd, q_rs, kv_rs, o_rs, do_rs, dq_rs, dkv_rs, 0.125, klim, None)


def test_cross_entry_points_are_bound_and_refuse_bad_arguments_before_any_launch():
    from nova_pointcloud_amd import hip

    assert "nova_attn_cross_fwd_lse" in hip.SIGNATURES and "nova_attn_cross_bwd" in hip.SIGNATURES
    assert len(hip.SIGNATURES["nova_attn_cross_fwd_lse"]) == 15 and len(hip.SIGNATURES["nova_attn_cross_bwd"]) == 24
    lib = hip.load(check_device=False)
    fwd, bwd = lib.nova_attn_cross_fwd_lse, lib.nova_attn_cross_bwd
    assert fwd.argtypes == hip.SIGNATURES["nova_attn_cross_fwd_lse"] and bwd.argtypes == hip.SIGNATURES["nova_attn_cross_bwd"]

    def refused(fn, args, code, word):
        assert fn(*args) == code, (fn.__name__, args)
        assert word in lib.nova_last_error(), (lib.nova_last_error(), word)

    # null pointers, one at a time
    for i in range(5):
        p = list(P[:4]) + [P[5]]
        p[i] = None
        refused(fwd, _fwd_args(ptrs=p), ERR_ARG, b"null pointer")
    for i in range(10):
        p = list(P)
        p[i] = None
        refused(bwd, _bwd_args(ptrs=p), ERR_ARG, b"null pointer")
    # head dimensions that are not built
    for hd in (32, 128, 0):
        refused(fwd, _fwd_args(hd=hd), ERR_SHAPE, b"head_dim")
        refused(bwd, _bwd_args(hd=hd), ERR_SHAPE, b"head_dim")
    # strides that are not 16-byte multiples, each stride on its own
    for name in ("q_rs", "kv_rs", "o_rs"):
        refused(fwd, _fwd_args(**{name: 196}), ERR_SHAPE, b"16-byte")
    for name in ("q_rs", "kv_rs", "o_rs", "do_rs", "dq_rs", "dkv_rs"):
        refused(bwd, _bwd_args(**{name: 196}), ERR_SHAPE, b"16-byte")
    # no keys for some queries
    for Lk in (0, -3):
        refused(fwd, _fwd_args(Lk=Lk), ERR_SHAPE, b"Lk")
        refused(bwd, _bwd_args(Lk=Lk), ERR_SHAPE, b"Lk")
    # a side whose rows span 2 GiB or more: Lq * q_rs, Lq * do_rs (o_rs in the forward), Lk * kv_rs, in bytes
    big = 1 << 20  # rows; with a stride of 1024 elements that is 2 GiB
    refused(fwd, _fwd_args(Lq=big, q_rs=1024), ERR_SHAPE, b"2 GiB")
    refused(fwd, _fwd_args(Lq=big, o_rs=1024), ERR_SHAPE, b"2 GiB")
    refused(fwd, _fwd_args(Lk=big, kv_rs=1024), ERR_SHAPE, b"2 GiB")
    refused(bwd, _bwd_args(Lq=big, q_rs=1024), ERR_SHAPE, b"2 GiB")
    refused(bwd, _bwd_args(Lq=big, do_rs=1024), ERR_SHAPE, b"2 GiB")
    refused(bwd, _bwd_args(Lk=big, kv_rs=1024), ERR_SHAPE, b"2 GiB")
    # an oversize grid: more than 2^31 - 1 workgroups on the query side, and on the key side alone
    refused(fwd, _fwd_args(S=60000, heads=60000, Lq=200), ERR_SHAPE, b"grid")
    refused(bwd, _bwd_args(S=60000, heads=60000, Lq=200), ERR_SHAPE, b"grid")
    refused(bwd, _bwd_args(S=40000, heads=40000, Lq=1, Lk=200), ERR_SHAPE, b"grid")
    # nothing to do: no launch, 0
    for kw in (dict(S=0), dict(Lq=0), dict(S=0, Lk=0), dict(Lq=0, Lk=0)):
        assert fwd(*_fwd_args(**kw)) == 0 and bwd(*_bwd_args(**kw)) == 0, kw


# ---------------------------------------------------------------------------------------------------------------------
# c. MultiheadAttention against torch.nn.MultiheadAttention
# ---------------------------------------------------------------------------------------------------------------------
def _rel(got, ref):
    return ((got - ref).abs().max() / ref.abs().max().clamp_min(1e-300)).item()


@pytest.mark.parametrize("m", [None, 19], ids=["self", "cross"])
def test_multihead_attention_is_torch_multihead_attention_in_float64(m):
    """Same state_dict keys and shapes, load_state_dict(strict=True) both ways, and in float64 the output and every parameter
    and input gradient within 1e-12 of the tensor's largest entry: self (n = 7) and cross (n = 7, m = 19), E = 128, 2 heads."""
    from nova_pointcloud_amd.attention import MultiheadAttention

    torch.manual_seed(11)
    ref = torch.nn.MultiheadAttention(128, 2, batch_first=True).double()
    ours = MultiheadAttention(128, 2).double()
    sd_r, sd_o = ref.state_dict(), ours.state_dict()
    assert list(sd_r) == list(sd_o) == ["in_proj_weight", "in_proj_bias", "out_proj.weight", "out_proj.bias"]
    assert {n: tuple(t.shape) for n, t in sd_r.items()} == {n: tuple(t.shape) for n, t in sd_o.items()}
    with torch.no_grad():  # biases start at 0 in both: give every parameter a value that matters
        for p in ours.parameters():
            p.copy_(torch.randn_like(p) * 0.2)
    ref.load_state_dict(ours.state_dict(), strict=True)
    ours.load_state_dict(ref.state_dict(), strict=True)
    n = 7
    x = torch.randn(3, n, 128, dtype=F64)
    y = x if m is None else torch.randn(3, m, 128, dtype=F64)
    w = torch.randn(3, n, 128, dtype=F64)
    got, want = {}, {}
    for mod, store in ((ours, got), (ref, want)):
        a = x.clone().requires_grad_(True)
        b = a if m is None else y.clone().requires_grad_(True)
        out, none = mod(a, b, b, need_weights=False)
        assert none is None and out.shape == (3, n, 128)
        (out * w).sum().backward()
        store["out"], store["d_query"] = out.detach(), a.grad
        if m is not None:
            store["d_key_value"] = b.grad
        for name, p in mod.named_parameters():
            store[name] = p.grad.clone()
        mod.zero_grad()
    assert got.keys() == want.keys()
    for name in want:
        assert _rel(got[name], want[name]) <= 1e-12, (name, _rel(got[name], want[name]))
    with pytest.raises(ValueError, match="need_weights"):
        ours(x, y, y, need_weights=True)


def test_multihead_attention_without_bias_and_with_dropout_keeps_torchs_names():
    from nova_pointcloud_amd.attention import MultiheadAttention

    ours, ref = MultiheadAttention(64, 2, dropout=0.1, bias=False), torch.nn.MultiheadAttention(64, 2, dropout=0.1, bias=False, batch_first=True)
    assert list(ours.state_dict()) == list(ref.state_dict()) == ["in_proj_weight", "out_proj.weight"]
    x, y = torch.randn(2, 5, 64), torch.randn(2, 9, 64)
    ours.eval(), ref.eval()
    ref.load_state_dict(ours.state_dict(), strict=True)
    assert _rel(ours(x, y, y)[0], ref(x, y, y, need_weights=False)[0]) < 1e-5
    ours.train()
    out, _ = ours(x, y, y)  # dropout in training mode: torch's SDPA
    assert out.shape == (2, 5, 64) and torch.isfinite(out).all()


# ---------------------------------------------------------------------------------------------------------------------
# d. EdgeAligner's names
# ---------------------------------------------------------------------------------------------------------------------
def test_edge_aligner_has_the_reference_modules_parameter_names():
    """The key set of the reference's EdgeAligner(128, 2).state_dict() (transformer_pointcloud_nova.py:158-174), listed here."""
    from nova_pointcloud_amd.attention import EdgeAligner

    want = {"biattn.in_proj_weight": (384, 128), "biattn.in_proj_bias": (384,), "biattn.out_proj.weight": (128, 128),
            "biattn.out_proj.bias": (128,), "edge_mlp.0.weight": (64, 128), "edge_mlp.0.bias": (64,), "edge_mlp.2.weight": (128, 64),
            "edge_mlp.2.bias": (128,), "spatial_embed.weight": (128, 3), "spatial_embed.bias": (128,)}
    assert {n: tuple(t.shape) for n, t in EdgeAligner(128, 2).state_dict().items()} == want


def test_attention_supported_answers_as_before_without_a_key_tensor():
    """`attention_supported(q, attn_mask, k)`: k=None is the self-attention question; a key tensor is checked without a device through
    the same stand-in tests/test_mirror_cpu.py uses."""
    from nova_pointcloud_amd import autograd as A

    class FakeCuda(object):
        is_cuda = True

        def __init__(self, shape, dtype):
            self.shape, self.dtype = shape, dtype

        def dim(self):
            return len(self.shape)

    q = FakeCuda((2, 3, 16, 64), torch.bfloat16)
    assert A.attention_supported(q) == A._ENABLED
    assert A.attention_supported(q, None, FakeCuda((2, 3, 40, 64), torch.bfloat16)) == A._ENABLED
    assert not A.attention_supported(q, None, FakeCuda((2, 3, 40, 96), torch.bfloat16))   # another head dimension
    assert not A.attention_supported(q, None, FakeCuda((2, 4, 40, 64), torch.bfloat16))   # another head count
    assert not A.attention_supported(q, None, FakeCuda((2, 3, 40, 64), torch.float32))
    assert not A.attention_supported(q, None, FakeCuda((2, 3, 0, 64), torch.bfloat16))    # no keys
    assert not A.attention_supported(q, torch.zeros(16, 40), FakeCuda((2, 3, 40, 64), torch.bfloat16))  # a CPU mask
    assert not A.attention_supported(torch.zeros(2, 3, 16, 64, dtype=torch.bfloat16), None, torch.zeros(2, 3, 40, 64, dtype=torch.bfloat16))
