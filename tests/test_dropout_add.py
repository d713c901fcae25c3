"""Fused bias-dropout-residual (nova_pointcloud_amd.dropout, csrc/dropout_add.hip) against a restatement of its definition.

restate() below is include/nova_hip.h at nova_bias_dropout_add in numpy / torch on the CPU: Philox4x32-10 in uint64 arithmetic,
the per-element chain in float32 with the stated roundings, the 128-row chunk sums of the bias gradient in ascending row order
and the chunks in ascending order. The kernels are held BITWISE to it, forward and gx; the bias gradient bitwise too, and within
    (rows + 2) u sum_rows |gx| + 1e-30 rows,  u = 2^-24
of the float64 sum (a float32 sum of `rows` terms in any order errs by at most (rows - 1) u sum |terms| to first order; the
chunk merge adds less than one more step per chunk; + 2 covers the second-order terms at these row counts). The mask's
statistics are required of the restated mask, which the kernel must then equal bit for bit.
"""
import ctypes
import math
import os
import re
import subprocess
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if __name__ == "__main__":  # run as a script by test_abi_rejections_in_a_process_without_a_device
    sys.path.insert(0, ROOT)
from nova_pointcloud_amd import dropout as _dropout  # noqa: E402  every test here is about this module: without it none passes

U = 2.0 ** -24
CHUNK = 128  # == NOVA_DROPOUT_CHUNK (test_header_constants)
MAX_D = 16384  # == NOVA_DROPOUT_MAX_DIM
M0, M1, W0, W1 = 0xD2511F53, 0xCD9E8D57, 0x9E3779B9, 0xBB67AE85
MASK32 = np.uint64(0xFFFFFFFF)
DTYPES = [torch.float32, torch.bfloat16, torch.float16]
NAME = {torch.float32: "f32", torch.bfloat16: "bf16", torch.float16: "f16"}
NONE, RELU = 0, 1


# ---- the definition, restated -------------------------------------------------------------------------------------------

def philox4x32_10(counter, key):
    """counter: four uint64 arrays holding 32-bit words, key: two ints. Returns the four output words (uint64 arrays < 2^32)."""
    c0, c1, c2, c3 = (np.asarray(c, dtype=np.uint64) & MASK32 for c in counter)
    k0, k1 = int(key[0]) & 0xFFFFFFFF, int(key[1]) & 0xFFFFFFFF
    for _ in range(10):
        p0, p1 = np.uint64(M0) * c0, np.uint64(M1) * c2  # 32 x 32 -> 64 bits: no overflow in uint64
        c0, c1, c2, c3 = (p1 >> np.uint64(32)) ^ c1 ^ np.uint64(k0), p1 & MASK32, (p0 >> np.uint64(32)) ^ c3 ^ np.uint64(k1), p0 & MASK32
        k0, k1 = (k0 + W0) & 0xFFFFFFFF, (k1 + W1) & 0xFFFFFFFF  # the key is bumped after every round
    return c0, c1, c2, c3


def draws(first, count, seed, subsequence):
    """w(i) for the flat indices first .. first + count - 1 (uint64 array of 32-bit values): word i & 3 at counter i >> 2."""
    q0, q1 = first >> 2, (first + count - 1) >> 2
    q = np.arange(q1 - q0 + 1, dtype=np.uint64) + np.uint64(q0)
    sub = np.full_like(q, subsequence & 0xFFFFFFFF), np.full_like(q, subsequence >> 32)
    words = np.stack(philox4x32_10((q & MASK32, q >> np.uint64(32), *sub), (seed & 0xFFFFFFFF, seed >> 32)), axis=1).reshape(-1)
    return words[first - 4 * q0: first - 4 * q0 + count]


def keep_mask(rows, D, T, seed, subsequence, first_row=0):
    """bool [rows, D]: kept iff (uint64) w(i) >= T, i = (first_row + row) * D + col."""
    if rows * D == 0:
        return torch.zeros(rows, D, dtype=torch.bool)
    return torch.from_numpy(draws(first_row * D, rows * D, seed, subsequence) >= np.uint64(T)).view(rows, D)


def restate(x, bias=None, residual=None, g=None, p=0.1, seed=0, subsequence=0, act=NONE, first_row=0, out_for_gate=None):
    """The definition on CPU tensors. x, residual, g [rows, D] in one dtype, bias float32 [D]. Returns a dict: keep, out (x's
    dtype), and with g: v (the float32 gx before the store rounding), gx (x's dtype), parts [chunks, D] and gbias [D] (float32)."""
    rows, D = x.shape
    T, scale = _dropout.dropout_threshold(p)
    s = torch.tensor(scale, dtype=torch.float32)
    zero = torch.zeros((), dtype=torch.float32)
    keep = keep_mask(rows, D, T, seed, subsequence, first_row)
    t = x.float()  # exact
    if bias is not None:
        t = t + bias.float()
    if act == RELU:
        t = torch.where(t > 0, t, torch.where(t != t, t, zero))
    d = torch.where(keep, t * s, zero)  # a dropped element is +0 whatever t is
    o = residual.float() + d if residual is not None else d
    res = {"keep": keep, "out": o.to(x.dtype)}  # one round-to-nearest-even
    if g is not None:
        gate = (res["out"] if out_for_gate is None else out_for_gate).float() > 0 if act == RELU else keep
        v = torch.where(gate, g.float() * s, zero)
        chunks = (rows + CHUNK - 1) // CHUNK
        parts = np.zeros((chunks, D), dtype=np.float32)
        vn = v.numpy()
        for r in range(rows):  # ascending rows, one float32 addition each, from +0
            parts[r // CHUNK] = parts[r // CHUNK] + vn[r]
        gbias = np.zeros(D, dtype=np.float32)
        for c in range(chunks):  # ascending chunks, from +0
            gbias = gbias + parts[c]
        res.update(v=v, gx=v.to(x.dtype), parts=torch.from_numpy(parts), gbias=torch.from_numpy(gbias))
    return res


def bits(t):
    return t.contiguous().view(torch.int32 if t.element_size() == 4 else torch.int16)


def same_bits(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and torch.equal(bits(a.cpu()), bits(b.cpu()))


def make(rows, D, dtype, seed, with_bias=True, with_res=True):
    gen = torch.Generator().manual_seed(seed)
    x = torch.randn(rows, D, generator=gen).to(dtype)
    b = torch.randn(D, generator=gen) if with_bias else None
    r = torch.randn(rows, D, generator=gen).to(dtype) if with_res else None
    g = torch.randn(rows, D, generator=gen).to(dtype)
    return x, b, r, g


# ---- CPU ----------------------------------------------------------------------------------------------------------------

def test_philox_known_answers():
    cases = [((0, 0, 0, 0), (0, 0), "6627e8d5 e169c58d bc57ac4c 9b00dbd8"),
             ((0xFFFFFFFF,) * 4, (0xFFFFFFFF,) * 2, "408f276d 41c83b0e a20bc7c6 6d5451fd"),
             ((0x243F6A88, 0x85A308D3, 0x13198A2E, 0x03707344), (0xA4093822, 0x299F31D0), "d16cfe09 94fdcceb 5001e420 24126ea1")]
    for counter, key, want in cases:
        got = philox4x32_10([np.array([c], dtype=np.uint64) for c in counter], key)
        assert " ".join(f"{int(w[0]):08x}" for w in got) == want
    # the draw of element i is word i & 3 at counter (i >> 2, subsequence), key seed: the third vector read that way
    seed, sub = (0x299F31D0 << 32) | 0xA4093822, (0x03707344 << 32) | 0x13198A2E
    first = ((0x85A308D3 << 32) | 0x243F6A88) << 2
    assert [f"{int(w):08x}" for w in draws(first, 4, seed, sub)] == "d16cfe09 94fdcceb 5001e420 24126ea1".split()
    assert [f"{int(w):08x}" for w in draws(first + 1, 2, seed, sub)] == ["94fdcceb", "5001e420"]


def test_header_constants():
    header = open(os.path.join(ROOT, "include", "nova_hip.h")).read()
    const = lambda name: int(re.search(r"#define " + name + r" (\d+)", header).group(1))
    assert const("NOVA_DROPOUT_CHUNK") == CHUNK == _dropout.DROPOUT_CHUNK
    assert const("NOVA_DROPOUT_MAX_DIM") == MAX_D == _dropout.DROPOUT_MAX_DIM
    assert const("NOVA_DROPOUT_MAX_ROWS") == _dropout.DROPOUT_MAX_ROWS
    assert (const("NOVA_DROPOUT_ACT_NONE"), const("NOVA_DROPOUT_ACT_RELU")) == (NONE, RELU) == (_dropout.ACT_NONE, _dropout.ACT_RELU)
    text = header[header.index("Fused bias-dropout-residual"):header.index("#define NOVA_DROPOUT_MAX_DIM")]
    for word in (f"0x{M0:08X}", f"0x{M1:08X}", f"0x{W0:08X}", f"0x{W1:08X}", "Philox4x32-10", "transformer_pointcloud_nova.py", ":433-441", ":590-598",
                 ":510", ":775", "train_newloss.py", "6627e8d5 e169c58d bc57ac4c 9b00dbd8", "408f276d 41c83b0e a20bc7c6 6d5451fd",
                 "d16cfe09 94fdcceb 5001e420 24126ea1"):
        assert word in text, word
    assert text.rstrip().endswith("fails to bind, loudly). */") and "Added without a version bump" in text


def test_threshold_and_scale():
    T = _dropout.dropout_threshold
    assert T(0) == (0, 1.0) and T(0.0) == (0, 1.0) and T(1) == (1 << 32, 0.0) and T(1.0) == (1 << 32, 0.0)
    assert T(0.5) == (1 << 31, 2.0)
    assert T(0.1) == (int(0.1 * 2 ** 32), float(np.float32(1 / 0.9)))  # p 2^32 is exact in float64: a power-of-two scaling
    assert T(0.1)[0] == 429496729 and T(0.9)[0] == 3865470566
    assert T(2.0 ** -33) == (0, float(np.float32(1 / (1 - 2.0 ** -33))))  # below one draw in 2^32: nothing is dropped
    assert T(np.float32(0.25)) == (1 << 30, float(np.float32(4 / 3)))


@pytest.mark.parametrize("p", [0.1, 0.5, 0.9])
@pytest.mark.parametrize("seed", [0, 1])
def test_mask_kept_share(p, seed):
    n = 1 << 20
    T, _ = _dropout.dropout_threshold(p)
    share = float((draws(0, n, seed, 0) >= np.uint64(T)).mean())
    sigma = math.sqrt(p * (1 - p) / n)
    print(f"p {p} seed {seed}: kept {share:.6f}, {(share - (1 - p)) / sigma:+.2f} sigma")
    assert abs(share - (1 - p)) <= 5 * sigma


def test_mask_rows_columns_and_subsequences():
    rows, D, p = 1024, 768, 0.1
    T, _ = _dropout.dropout_threshold(p)
    keep = keep_mask(rows, D, T, 1, 0).double()
    for name, share, count in (("column", keep.mean(0), rows), ("row", keep.mean(1), D)):
        sigma = math.sqrt(p * (1 - p) / count)
        worst = float((share - (1 - p)).abs().max()) / sigma
        print(f"{name} shares {float(share.min()):.3f} .. {float(share.max()):.3f}, worst {worst:.2f} sigma")
        assert worst <= 5
    n = rows * D
    T5, _ = _dropout.dropout_threshold(0.5)
    agree = float((keep_mask(rows, D, T5, 1, 0) == keep_mask(rows, D, T5, 1, 1)).double().mean())
    print(f"subsequences 0 and 1 agree on {agree:.4f}")
    assert abs(agree - 0.5) <= 5 * math.sqrt(0.25 / n)
    assert not torch.equal(keep_mask(rows, D, T5, 1, 0), keep_mask(rows, D, T5, 2, 0))
    # a slice sees the mask of its place
    assert torch.equal(keep_mask(rows, D, T, 1, 0)[128:256], keep_mask(128, D, T, 1, 0, first_row=128))
    assert keep_mask(4, 5, 0, 3, 0).all() and not keep_mask(4, 5, 1 << 32, 3, 0).any()  # T = 0 keeps all, T = 2^32 none


@pytest.mark.parametrize("rows,D,act", [(129, 12, NONE), (257, 5, NONE), (130, 9, RELU)])
def test_restatement_equals_the_literal_forms(rows, D, act):
    p, seed = 0.3, 11
    x, b, r, g = make(rows, D, torch.float32, 5, with_res=act == NONE)
    res = restate(x, b, r, g, p=p, seed=seed, act=act)
    _, scale = _dropout.dropout_threshold(p)
    mask, s = res["keep"], torch.tensor(scale, dtype=torch.float32)
    xa, ba = x.clone().requires_grad_(), b.clone().requires_grad_()
    if act == NONE:
        ra = r.clone().requires_grad_()
        lit = ra + torch.where(mask, (xa + ba) * s, torch.zeros(()))
    else:
        lit = torch.where(mask, torch.relu(xa + ba) * s, torch.zeros(()))
    assert torch.equal(res["out"], lit.detach())
    lit.backward(g)
    assert torch.equal(res["gx"], xa.grad)
    if act == NONE:
        assert torch.equal(ra.grad, g)
    exact = res["v"].double().sum(0)
    bound = (rows + 2) * U * res["v"].double().abs().sum(0) + 1e-30 * rows
    for name, got in (("restated", res["gbias"]), ("autograd", ba.grad)):
        ratio = float(((got.double() - exact).abs() / bound).max())
        print(f"{name} bias gradient: worst error / bound {ratio:.3f}")
        assert ratio <= 1
    assert res["parts"].shape == ((rows + CHUNK - 1) // CHUNK, D)


def test_restatement_special_values():
    inf, nan = math.inf, math.nan
    x = torch.tensor([[inf, -inf, nan, 1.0, -2.0, -0.0, inf, nan]])
    T, scale = _dropout.dropout_threshold(0.5)
    wanted = lambda k: k[:4] == [True, False, False, True] and k[6:] == [False, True]  # inf and a NaN kept, -inf, a NaN and inf dropped
    seed = next(s for s in range(4096) if wanted(keep_mask(1, 8, T, s, 0)[0].tolist()))
    keep = keep_mask(1, 8, T, seed, 0)[0]
    out = restate(x, p=0.5, seed=seed)["out"][0]
    for j in range(8):
        if not keep[j]:
            assert out[j].item() == 0 and not math.copysign(1, out[j].item()) < 0  # +0 for a dropped inf or NaN
    assert out[0].item() == inf and out[3].item() == 2.0 and math.isnan(out[7].item())
    relu = restate(x, p=0.0, act=RELU)["out"][0]
    assert relu[0].item() == inf and math.isnan(relu[2].item()) and math.isnan(relu[7].item())
    assert all(relu[j].item() == 0 and math.copysign(1, relu[j].item()) > 0 for j in (1, 4, 5))


def test_python_argument_errors_in_the_stated_order():
    from nova_pointcloud_amd import hip

    f = _dropout.bias_dropout_add
    x, b, r = torch.zeros(4, 6), torch.zeros(6), torch.zeros(4, 6)
    bad_all = dict(p=2, activation="gelu", seed=-1)
    # 1. types, before everything else
    for kw in (dict(x=None), dict(bias=3.0), dict(residual=[1])):
        args = dict(x=x.long(), bias=b, residual=r.half())
        args.update(kw)
        with pytest.raises(ValueError, match="expected a tensor"):
            f(**args, **bad_all)
    # 2. dtypes
    with pytest.raises(ValueError, match="x: expected a floating dtype"):
        f(x.long(), b, torch.zeros(3), **bad_all)
    with pytest.raises(ValueError, match="bias: expected a floating dtype"):
        f(x, b.long(), torch.zeros(3), **bad_all)
    with pytest.raises(ValueError, match="residual: expected x's dtype"):
        f(x, b, torch.zeros(3).half(), **bad_all)
    # 3. shapes
    with pytest.raises(ValueError, match=r"x: expected \[\.\.\., D\]"):
        f(torch.zeros(()), **bad_all)
    with pytest.raises(ValueError, match="residual: expected x's shape"):
        f(x, torch.zeros(7), torch.zeros(6, 4), **bad_all)
    with pytest.raises(ValueError, match=r"bias: expected \[6\]"):
        f(torch.zeros(0, 6), torch.zeros(7), **bad_all)
    # 4. D range
    for D in (0, MAX_D + 1):
        with pytest.raises(ValueError, match=f"takes 1 .. {MAX_D} columns"):
            f(torch.zeros(1, D), torch.zeros(D, device="meta"), **bad_all)
    # 5. devices
    with pytest.raises(ValueError, match="same device"):
        f(x, b.to("meta"), r, **bad_all)
    with pytest.raises(ValueError, match="x and residual must be on the same device"):
        f(x, b, r.to("meta"), **bad_all)
    # 6. p
    for p in (-0.1, 1.5, math.nan, True, "0.1", None, 1 + 0j):
        with pytest.raises(ValueError, match="p must be a real number"):
            f(x, b, r, p=p, activation="gelu", seed=-1)
    # 7. activation, then activation with residual
    with pytest.raises(ValueError, match="activation must be None or 'relu'"):
        f(x, b, r, activation="gelu", seed=-1)
    with pytest.raises(ValueError, match="takes no residual"):
        f(x, b, r, activation="relu", seed=-1)
    # 8. seed / subsequence range
    for kw in (dict(seed=-1), dict(seed=1 << 64), dict(seed=1.0), dict(seed=True), dict(subsequence=-1), dict(subsequence=1 << 64),
               dict(subsequence=None)):
        with pytest.raises(ValueError, match="must be an integer in 0 .. 2\\^64 - 1"):
            f(x, b, r, **kw)
    with pytest.raises(ValueError, match="generator must be"):
        f(x, b, r, generator=7)
    # what passes all of that meets the device check: CPU tensors are refused, with every training / p setting, and no seed is drawn
    state = torch.get_rng_state()
    for kw in (dict(), dict(p=0), dict(p=1), dict(training=False), dict(seed=(1 << 64) - 1, subsequence=(1 << 64) - 1), dict(residual=None, activation="relu")):
        args = dict(x=x, bias=b, residual=r)
        args.update(kw)
        with pytest.raises(hip.NovaHipError, match="runs on the GPU"):
            f(**args)
    assert torch.equal(torch.get_rng_state(), state)
    with pytest.raises(ValueError, match="p must be"):
        _dropout.BiasDropoutAdd(p=1.5)
    with pytest.raises(ValueError, match="activation must be"):
        _dropout.BiasDropoutAdd(activation="gelu")


def test_seed_drawing():
    torch.manual_seed(1234)
    a, b = _dropout.draw_seed(), _dropout.draw_seed()
    torch.manual_seed(1234)
    assert (_dropout.draw_seed(), _dropout.draw_seed()) == (a, b) and a != b  # manual_seed fixes the step; consecutive sites differ
    assert isinstance(a, int) and 0 <= a < 1 << 63
    gen = torch.Generator().manual_seed(7)
    state = torch.get_rng_state()
    c = _dropout.draw_seed(gen)
    assert torch.equal(torch.get_rng_state(), state)  # a generator of one's own leaves the global one alone
    assert _dropout.draw_seed(torch.Generator().manual_seed(7)) == c and _dropout.draw_seed(gen) != c
    # checkpointing restores the CPU generator's state and so recomputes the same seed
    torch.set_rng_state(state)
    d = _dropout.draw_seed()
    torch.set_rng_state(state)
    assert _dropout.draw_seed() == d


def test_no_seed_is_drawn_when_nothing_is_dropped():
    """p = 0 and training=False take seed 0 and leave the generator untouched; p > 0 draws exactly one seed, a given one none."""
    numbers = _dropout.mask_numbers
    torch.manual_seed(99)
    state = torch.get_rng_state()
    gen = torch.Generator().manual_seed(3)
    gstate = gen.get_state()
    assert numbers(0) == numbers(0.0, seed=5) == numbers(0.7, training=False) == numbers(2.0 ** -40) == (0, 1.0, 0)
    assert numbers(0, generator=gen) == (0, 1.0, 0) and numbers(0.5, seed=17, generator=gen) == (1 << 31, 2.0, 17)
    assert numbers(1, seed=(1 << 64) - 1) == (1 << 32, 0.0, (1 << 64) - 1)
    assert torch.equal(torch.get_rng_state(), state) and torch.equal(gen.get_state(), gstate)
    got = numbers(0.5)
    assert not torch.equal(torch.get_rng_state(), state)
    torch.manual_seed(99)
    assert got == (1 << 31, 2.0, _dropout.draw_seed())
    state = torch.get_rng_state()
    assert numbers(0.5, generator=gen) == (1 << 31, 2.0, _dropout.draw_seed(torch.Generator().manual_seed(3)))
    assert torch.equal(torch.get_rng_state(), state) and not torch.equal(gen.get_state(), gstate)


def abi_checks():
    """Every error of the two entries, in the order include/nova_hip.h states, before any device work, and the rows <= 0
    return. Run by test_abi_rejections_in_a_process_without_a_device in a child process that sees no GPU: the calls carry
    addresses of nothing, and a build that lost a check would launch on them; without a device that launch fails with a
    return code."""
    sys.path.insert(0, ROOT)
    from nova_pointcloud_amd import hip

    lib = hip.load(check_device=False)
    MB = 1 << 28  # pointers far apart: never dereferenced, rejected first
    x, bias, res, out, g, gx, parts = (ctypes.c_void_p(MB * i) for i in range(1, 8))
    T1 = 429496729

    def fwd(rows=4, D=8, dtype=0, x=x, bias=bias, residual=res, out=out, first_row=0, T=T1, act=NONE):
        return lib.nova_bias_dropout_add(x, dtype, bias, residual, out, rows, D, first_row, T, 1.0, 1, 0, act, None)

    def bwd(rows=4, D=8, dtype=0, g=g, out=None, gx=gx, parts=parts, first_row=0, T=T1, act=NONE):
        return lib.nova_bias_dropout_add_bwd(g, out, dtype, gx, parts, rows, D, first_row, T, 1.0, 1, 0, act, None)

    err = lib.nova_last_error
    SHAPE, ARG = -2, -1
    worst = dict(dtype=7, D=0, T=(1 << 32) + 1, first_row=-1)  # everything later in the order is wrong too
    # 1. null pointers
    for name in ("x", "out"):
        assert fwd(**worst, act=9, **{name: None}) == ARG and err() == b"bias_dropout_add: null pointer " + name.encode(), err()
        assert fwd(rows=0, **{name: None}) == ARG
    assert bwd(**worst, act=9, g=None) == ARG and err() == b"bias_dropout_add_bwd: null pointer g", err()
    assert bwd(rows=0, g=None) == ARG
    for fn, who in ((fwd, b"bias_dropout_add: "), (bwd, b"bias_dropout_add_bwd: ")):
        # 2. dtype
        for code in (-1, 3, 7):
            assert fn(**dict(worst, dtype=code), act=9) == ARG and err().startswith(who + b"unknown dtype code"), err()
        # 3. act
        for act in (-1, 2, 9):
            assert fn(**dict(worst, dtype=1), act=act) == ARG and err().startswith(who + b"unknown act code"), err()
        for dtype in (0, 1, 2):
            # 5. D range, then rows
            for D in (0, -1, MAX_D + 1):
                assert fn(**dict(worst, dtype=dtype, D=D)) == SHAPE and b"NOVA_DROPOUT_MAX_DIM" in err() and err().startswith(who), err()
                assert fn(rows=0, D=D, dtype=dtype) == SHAPE
            assert fn(rows=(1 << 30) + 1, dtype=dtype, T=1 << 33) == SHAPE and b"NOVA_DROPOUT_MAX_ROWS" in err()
            # 6. T
            assert fn(dtype=dtype, T=(1 << 32) + 1, first_row=-1) == ARG and b"exceeds 2^32" in err(), err()
            assert fn(rows=0, dtype=dtype, T=1 << 63) == ARG
            # 7. first_row
            assert fn(dtype=dtype, first_row=-1) == ARG and b"is negative" in err()
            assert fn(dtype=dtype, first_row=-128, T=1 << 32) == ARG and b"is negative" in err()
            assert fn(dtype=dtype, first_row=(1 << 48) - 3) == ARG and b"exceeds 2^48" in err()
            # rows <= 0 returns 0 after these and writes nothing, whatever T in range
            for T in (0, T1, 1 << 32):
                assert fn(rows=0, dtype=dtype, T=T) == 0 and fn(rows=-5, D=MAX_D, dtype=dtype, T=T, first_row=1 << 40) == 0
    # 3. RELU with a residual (forward); 4. RELU without the saved out (backward): before the ranges
    assert fwd(**dict(worst, dtype=0), act=RELU) == ARG and err().endswith(b"takes no residual"), err()
    assert fwd(rows=0, act=RELU) == ARG and fwd(rows=0, act=RELU, residual=None) == 0
    assert fwd(rows=0, bias=None, residual=None) == 0  # bias and residual may be NULL
    assert bwd(**dict(worst, dtype=0), act=RELU) == ARG and b"needs the saved out" in err(), err()
    assert bwd(rows=0, act=RELU) == ARG and bwd(rows=0, act=RELU, out=out) == 0
    assert bwd(**dict(worst, dtype=0), act=RELU, out=out) == SHAPE
    # 8. first_row off the chunks with gbias_parts; 9. nothing wanted: both before the rows <= 0 return
    for first_row in (1, 127, 129, (1 << 33) + 64):
        assert bwd(first_row=first_row, gx=None, parts=None) == ARG and b"no gradient wanted" in err()
        assert bwd(first_row=first_row) == ARG and b"not a multiple of 128" in err(), err()
        assert bwd(rows=0, first_row=first_row) == ARG and bwd(rows=0, first_row=first_row, parts=None) == 0
    assert bwd(gx=None, parts=None) == ARG and err().endswith(b"no gradient wanted (gx and gbias_parts are both NULL)")
    assert bwd(rows=0, gx=None, parts=None) == ARG and bwd(rows=0, gx=None) == 0 and bwd(rows=0, parts=None) == 0
    assert bwd(first_row=-1, gx=None, parts=None) == ARG and b"is negative" in err()  # in that order
    # 10. an output must not overlap an input or another output: checked last (no call here passes every check: what passes
    # them launches, and these pointers are not memory)
    at = lambda p, off: ctypes.c_void_p(p.value + off)
    for dtype, es in ((0, 4), (1, 2), (2, 2)):
        n = 4 * 8 * es
        for name, p, size in (("x", x, n), ("bias", bias, 8 * 4), ("residual", res, n)):
            assert fwd(dtype=dtype, out=p) == ARG and err().endswith(b"out overlaps the input " + name.encode()), (name, err())
            assert fwd(dtype=dtype, out=at(p, size - 2)) == ARG and err().endswith(b"out overlaps the input " + name.encode())  # its last bytes
            assert fwd(dtype=dtype, out=at(p, -n + 2)) == ARG and b"overlaps" in err()  # the last bytes of out on its first
        assert fwd(dtype=dtype, out=x, rows=0) == 0 and fwd(dtype=dtype, out=x, D=0) == SHAPE  # a shape error still comes first
        assert bwd(dtype=dtype, gx=g) == ARG and err().endswith(b"gx overlaps the input g")
        assert bwd(dtype=dtype, parts=at(g, n - 4)) == ARG and err().endswith(b"gbias_parts overlaps the input g")
        assert bwd(dtype=dtype, gx=out, out=out, act=RELU) == ARG and err().endswith(b"gx overlaps the input out")
        assert bwd(dtype=dtype, parts=at(out, -8 * 4 + 4), out=out, act=RELU) == ARG and err().endswith(b"gbias_parts overlaps the input out")
        assert bwd(dtype=dtype, parts=at(gx, n - 4)) == ARG and err().endswith(b"gx and gbias_parts overlap each other")
        assert bwd(dtype=dtype, gx=at(parts, 8 * 4 - 2)) == ARG and err().endswith(b"gx and gbias_parts overlap each other")  # one chunk row of D floats
    assert lib.nova_version() == hip.ABI_VERSION  # no version bump
    print("abi checks passed")


def test_abi_rejections_in_a_process_without_a_device():
    env = dict(os.environ, HIP_VISIBLE_DEVICES="-1", CUDA_VISIBLE_DEVICES="-1", ROCR_VISIBLE_DEVICES="-1")
    out = subprocess.run([sys.executable, os.path.abspath(__file__), "--abi-checks"], env=env, capture_output=True, text=True, timeout=300, cwd=ROOT)
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-2000:]
    assert out.stdout.strip().endswith("abi checks passed"), out.stdout[-2000:]


# ---- GPU ----------------------------------------------------------------------------------------------------------------

def run_gpu(x, b, r, g, p, seed, subsequence=0, activation=None, training=True):
    """Forward and backward through the public function on the GPU: out, gx, gbias (None where there is no bias), gres."""
    dev = "cuda"
    xa = x.to(dev).requires_grad_()
    ba = b.to(dev).requires_grad_() if b is not None else None
    ra = r.to(dev).requires_grad_() if r is not None else None
    out = _dropout.bias_dropout_add(xa, ba, ra, p=p, training=training, activation=activation, seed=seed, subsequence=subsequence)
    out.backward(g.to(dev))
    return out.detach(), xa.grad, ba.grad if b is not None else None, ra.grad if r is not None else None


def check_against_restatement(rows, D, dtype, p, with_bias, with_res, act, seed=20261021, subsequence=0):
    x, b, r, g = make(rows, D, dtype, rows * 100003 + D, with_bias, with_res)
    want = restate(x, b, r, g, p=p, seed=seed, subsequence=subsequence, act=act)
    out, gx, gb, gr = run_gpu(x, b, r, g, p, seed, subsequence, "relu" if act == RELU else None)
    assert same_bits(out, want["out"]), f"out differs in {int((bits(out.cpu()) != bits(want['out'])).sum())} of {rows * D} elements"
    assert same_bits(gx, want["gx"]), f"gx differs in {int((bits(gx.cpu()) != bits(want['gx'])).sum())} of {rows * D} elements"
    if with_res:
        assert same_bits(gr, g)
    if with_bias:
        assert same_bits(gb, want["gbias"])
        exact = want["v"].double().sum(0)
        bound = (rows + 2) * U * want["v"].double().abs().sum(0) + 1e-30 * rows
        ratio = float(((gb.cpu().double() - exact).abs() / bound).max())
        print(f"rows {rows} D {D} {NAME[dtype]} p {p}: bias gradient worst error / bound {ratio:.3f}")
        assert ratio <= 1
    return want


F32, BF16, F16 = DTYPES
# the vector tail (D % 4, D % 8), the row straddle of a Philox group (D % 4 != 0), the chunk edge (127, 128, 129, 257 rows), more
# than one workgroup, the widest row; every D and row count the definition names, every dtype, every p, with and without each addend
CASES = [(1, 1, F32, 0.1, True, True), (2, 3, BF16, 0.5, True, True), (127, 4, F32, 0.9, False, True), (128, 5, F16, 0.1, True, False),
         (129, 8, BF16, 0.1, True, True), (257, 9, F32, 0.5, True, True), (129, 64, F16, 0.9, False, False), (257, 767, BF16, 0.1, True, True),
         (257, 768, F32, 0.1, True, True), (129, 768, BF16, 0.1, True, True), (128, 769, F16, 0.5, True, True), (129, 3072, F16, 0.1, True, True),
         (2, 16384, BF16, 0.1, True, True), (129, 16384, F32, 0.5, True, False), (257, 768, BF16, 0, True, True), (257, 768, F16, 1, True, True),
         (129, 9, F32, 0, True, True), (129, 9, BF16, 1, False, True)]
RELU_CASES = [(257, 3072, BF16, 0.1, True), (129, 3072, F32, 0.1, True), (127, 5, F16, 0.5, True), (128, 769, BF16, 0.9, False),
              (129, 768, F32, 0.5, False), (2, 16384, F16, 0.1, True), (129, 8, BF16, 0, True), (129, 9, F32, 1, True)]


@pytest.mark.gpu
@pytest.mark.parametrize("rows,D,dtype,p,with_bias,with_res", CASES, ids=lambda v: NAME.get(v, str(v)))
def test_forward_and_backward_bitwise(hip, rows, D, dtype, p, with_bias, with_res):
    check_against_restatement(rows, D, dtype, p, with_bias, with_res, NONE)


@pytest.mark.gpu
@pytest.mark.parametrize("rows,D,dtype,p,with_bias", RELU_CASES, ids=lambda v: NAME.get(v, str(v)))
def test_relu_form_bitwise(hip, rows, D, dtype, p, with_bias):
    check_against_restatement(rows, D, dtype, p, with_bias, False, RELU, subsequence=(1 << 40) + 7)


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", DTYPES, ids=lambda v: NAME[v])
def test_storage_off_alignment_gives_the_same_bits(hip, dtype):
    """One element off a 16-byte boundary (4 bytes for float32, 2 for the 16-bit types), and a D that is no multiple of the
    vector: the element-by-element path, the same bits as the aligned 16-byte path and as the restatement."""
    vec = 16 // torch.empty((), dtype=dtype).element_size()
    for rows, D in ((129, 8 * vec), (130, 8 * vec + vec // 2), (3, 8 * vec + 1)):
        x, b, r, g = make(rows, D, dtype, 77)
        n = rows * D

        def shifted(t):
            buf = torch.empty(n + vec, dtype=dtype, device="cuda")
            assert buf.data_ptr() % 16 == 0
            v = buf[1:1 + n].view(rows, D)
            v.copy_(t)
            assert v.is_contiguous() and v.data_ptr() % 16 == t.element_size()
            return v

        aligned = run_gpu(x, b, r, g, 0.3, 9)
        xs, rs = shifted(x).requires_grad_(), shifted(r).requires_grad_()
        bs = b.cuda().requires_grad_()
        out = _dropout.bias_dropout_add(xs, bs, rs, p=0.3, seed=9)
        out.backward(shifted(g))
        want = restate(x, b, r, g, p=0.3, seed=9)
        for got, ref, name in ((out.detach(), aligned[0], "out"), (xs.grad, aligned[1], "gx"), (bs.grad, aligned[2], "gbias")):
            assert same_bits(got, ref), (name, rows, D)
        assert same_bits(out.detach(), want["out"]) and same_bits(xs.grad, want["gx"]) and same_bits(bs.grad, want["gbias"])
        # the saved output of the ReLU form off alignment too
        xs2 = shifted(x).requires_grad_()
        o2 = _dropout.bias_dropout_add(xs2, bs, p=0.3, seed=9, activation="relu")
        o2.backward(shifted(g))
        w2 = restate(x, b, None, g, p=0.3, seed=9, act=RELU)
        assert same_bits(o2.detach(), w2["out"]) and same_bits(xs2.grad, w2["gx"])


def abi_forward(hip, x, b, r, first_row, T, scale, seed, sub, act=NONE):
    out = torch.empty_like(x)
    hip.call("nova_bias_dropout_add", x.data_ptr(), hip.dtype_code(x.dtype), b.data_ptr() if b is not None else None,
             r.data_ptr() if r is not None else None, out.data_ptr(), x.shape[0], x.shape[1], first_row, T, scale, seed, sub, act, hip.stream_ptr())
    return out


def abi_backward(hip, g, out, first_row, T, scale, seed, sub, act=NONE):
    rows, D = g.shape
    gx = torch.empty_like(g)
    parts = torch.empty((rows + CHUNK - 1) // CHUNK, D, dtype=torch.float32, device=g.device)
    hip.call("nova_bias_dropout_add_bwd", g.data_ptr(), out.data_ptr() if out is not None else None, hip.dtype_code(g.dtype), gx.data_ptr(),
             parts.data_ptr(), rows, D, first_row, T, scale, seed, sub, act, hip.stream_ptr())
    return gx, parts


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", [F32, BF16], ids=lambda v: NAME[v])
def test_a_slice_sees_the_mask_of_its_place(hip, dtype):
    rows, D, seed, sub = 384, 768, 31, 2
    T, scale = _dropout.dropout_threshold(0.1)
    x, b, r, g = (t.cuda() for t in make(rows, D, dtype, 3))
    whole = abi_forward(hip, x, b, r, 0, T, scale, seed, sub)
    part = abi_forward(hip, x[128:256], b, r[128:256], 128, T, scale, seed, sub)
    assert same_bits(part, whole[128:256])
    assert not same_bits(abi_forward(hip, x[128:256], b, r[128:256], 0, T, scale, seed, sub), whole[128:256])  # the place matters
    gx, parts = abi_backward(hip, g, None, 0, T, scale, seed, sub)
    gx1, parts1 = abi_backward(hip, g[128:256], None, 128, T, scale, seed, sub)
    assert same_bits(gx1, gx[128:256]) and same_bits(parts1, parts[1:2])
    want = restate(x.cpu(), b.cpu(), r.cpu(), g.cpu(), p=0.1, seed=seed, subsequence=sub)
    assert same_bits(whole, want["out"]) and same_bits(gx, want["gx"]) and same_bits(parts, want["parts"])


@pytest.mark.gpu
@pytest.mark.parametrize("D,dtype", [(768, F32), (768, BF16), (5, F16)], ids=lambda v: NAME.get(v, str(v)))
def test_first_row_past_two_to_the_32_quads(hip, D, dtype):
    """first_row = 2^33, a multiple of 128: i >> 2 passes 2^32, so the counter's high word is live."""
    rows, first, seed, sub = 4, 1 << 33, (1 << 63) + 5, (1 << 64) - 1
    assert first % CHUNK == 0 and (first * D) >> 2 >= 1 << 32
    T, scale = _dropout.dropout_threshold(0.5)
    x, b, r, g = make(rows, D, dtype, 8)
    want = restate(x, b, r, g, p=0.5, seed=seed, subsequence=sub, first_row=first)
    assert not torch.equal(want["keep"], keep_mask(rows, D, T, seed, sub, first_row=0))
    xc, bc, rc, gc = (t.cuda() for t in (x, b, r, g))
    assert same_bits(abi_forward(hip, xc, bc, rc, first, T, scale, seed, sub), want["out"])
    gx, parts = abi_backward(hip, gc, None, first, T, scale, seed, sub)
    assert same_bits(gx, want["gx"]) and same_bits(parts, want["parts"])


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", DTYPES, ids=lambda v: NAME[v])
def test_nothing_dropped_and_everything_dropped(hip, dtype):
    rows, D = 130, 72
    x, b, r, g = make(rows, D, dtype, 4)
    plain = (r.float() + (x.float() + b)).to(dtype)
    for kw in (dict(p=0), dict(p=0.0), dict(p=0.7, training=False)):
        out, gx, gb, gr = run_gpu(x, b, r, g, seed=None, **kw)
        assert torch.equal(out.cpu(), plain) and torch.equal(gx.cpu(), g) and same_bits(gr, g)
        assert same_bits(gb, restate(x, b, r, g, p=0)["gbias"])
    out, gx, gb, gr = run_gpu(x, b, r, g, p=1, seed=3)
    zero = torch.zeros(rows, D, dtype=dtype)
    assert same_bits(out, r) and same_bits(gx, zero) and same_bits(gb, torch.zeros(D)) and same_bits(gr, g)  # +0, not -0
    out, gx, gb, _ = run_gpu(x, b, None, g, p=1.0, seed=3)
    assert same_bits(out, zero) and same_bits(gx, zero) and same_bits(gb, torch.zeros(D))
    out, gx, gb, _ = run_gpu(x, b, None, g, p=1, seed=3, activation="relu")
    assert same_bits(out, zero) and same_bits(gx, zero) and same_bits(gb, torch.zeros(D))


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", DTYPES, ids=lambda v: NAME[v])
def test_special_values(hip, dtype):
    """A dropped inf or NaN gives +0, a kept one propagates, relu(NaN) stays NaN: bit for bit the restatement (NaN payloads aside)."""
    inf, nan = math.inf, math.nan
    rows, D = 8, 16
    x = torch.tensor([inf, -inf, nan, 1.0, -2.0, -0.0, 0.0, 3.0] * (rows * D // 8)).view(rows, D).to(dtype)
    r = torch.ones(rows, D, dtype=dtype)
    for act, res in ((NONE, r), (NONE, None), (RELU, None)):
        want = restate(x, None, res, p=0.5, seed=21, act=act)
        out = _dropout.bias_dropout_add(x.cuda(), None, res.cuda() if res is not None else None, p=0.5, seed=21,
                                        activation="relu" if act == RELU else None).cpu()
        keep, xf = want["keep"], x.float()
        assert keep.any() and not keep.all()
        assert torch.equal(out.isnan(), want["out"].isnan())
        assert same_bits(out.nan_to_num(nan=7.0), want["out"].nan_to_num(nan=7.0))
        base = 1.0 if res is not None else 0.0
        dropped = out[~keep]
        assert torch.equal(dropped.float(), torch.full_like(dropped.float(), base)) and not torch.signbit(dropped).any()
        nonfinite = keep & ~xf.isfinite()
        if act == RELU:
            assert out[keep & xf.isnan()].isnan().all() and (out[keep & (xf == inf)] == inf).all()
            assert (out[keep & (xf <= 0)] == 0).all() and not torch.signbit(out[keep & (xf <= 0)]).any()
        else:
            assert nonfinite.any() and not out[nonfinite].isfinite().any()


@pytest.mark.gpu
def test_saved_tensors_stats_and_the_residual_gradient(hip):
    st = _dropout.stats
    x, b, r, g = (t.cuda() for t in make(130, 24, BF16, 6))
    xa, ba, ra = x.clone().requires_grad_(), b.clone().requires_grad_(), r.clone().requires_grad_()
    before = dict(st)
    out = _dropout.bias_dropout_add(xa, ba, ra, p=0.2, seed=1)
    assert out.grad_fn.saved_tensors == () and st["forward_launches"] == before["forward_launches"] + 1
    out.backward(g)
    assert (st["backward_launches"], st["bias_sum_launches"]) == (before["backward_launches"] + 1, before["bias_sum_launches"] + 1)
    o2 = _dropout.bias_dropout_add(xa, ba, p=0.2, seed=1, activation="relu")
    saved = o2.grad_fn.saved_tensors
    assert len(saved) == 1 and saved[0].data_ptr() == o2.data_ptr()  # out alone
    # only x: no chunk sums; only the bias: no gx; only the residual: no launch at all
    before = dict(st)
    _dropout.bias_dropout_add(xa, b, r, p=0.2, seed=1).backward(g)
    assert (st["backward_launches"], st["bias_sum_launches"]) == (before["backward_launches"] + 1, before["bias_sum_launches"])
    ba.grad = None
    _dropout.bias_dropout_add(x, ba, r, p=0.2, seed=1).backward(g)
    assert (st["backward_launches"], st["bias_sum_launches"]) == (before["backward_launches"] + 2, before["bias_sum_launches"] + 1)
    want = restate(x.cpu(), b.cpu(), r.cpu(), g.cpu(), p=0.2, seed=1)
    assert same_bits(ba.grad, want["gbias"]) and same_bits(xa.grad, (2 * want["v"]).to(BF16))  # xa took the same gradient twice
    before = dict(st)
    ra.grad = None
    _dropout.bias_dropout_add(x, b, ra, p=0.2, seed=1).backward(g)
    assert (st["backward_launches"], st["bias_sum_launches"]) == (before["backward_launches"], before["bias_sum_launches"])
    assert same_bits(ra.grad, g)
    assert not _dropout.bias_dropout_add(x, b, r, p=0.2, seed=1).requires_grad
    # the gradient of the residual is the incoming gradient itself: the same tensor object comes back from the backward
    class Ctx:
        mask = (*_dropout.dropout_threshold(0.2), 1, 0, NONE)
        needs_input_grad = (False, False, True, False, False, False, False, False)
        saved_tensors = ()

    before = dict(st)
    with torch.no_grad():
        grads = _dropout._BiasDropoutAdd.backward(Ctx, g)
    assert grads[2] is g and grads[0] is None and grads[1] is None and st == before
    Ctx.needs_input_grad = (True, True, True) + (False,) * 5
    with torch.no_grad():
        grads = _dropout._BiasDropoutAdd.backward(Ctx, g)
    assert grads[2] is g and same_bits(grads[0], want["gx"]) and same_bits(grads[1], want["gbias"])


@pytest.mark.gpu
def test_reproducible_and_seeded(hip):
    x, b, r, g = make(257, 768, BF16, 12)
    a1, a2 = run_gpu(x, b, r, g, 0.1, 5), run_gpu(x, b, r, g, 0.1, 5)
    assert all(same_bits(u, v) for u, v in zip(a1, a2))
    other = run_gpu(x, b, r, g, 0.1, 5, subsequence=1)
    assert not same_bits(other[0], a1[0]) and not same_bits(other[1], a1[1])
    assert not same_bits(run_gpu(x, b, r, g, 0.1, 6)[0], a1[0])
    # seed=None: the global CPU generator; torch.manual_seed fixes the step, and the next site draws another seed
    torch.manual_seed(4321)
    s1, s2 = run_gpu(x, b, r, g, 0.1, None), run_gpu(x, b, r, g, 0.1, None)
    torch.manual_seed(4321)
    t1 = run_gpu(x, b, r, g, 0.1, None)
    assert all(same_bits(u, v) for u, v in zip(s1, t1)) and not same_bits(s1[0], s2[0])
    torch.manual_seed(4321)
    assert same_bits(run_gpu(x, b, r, g, 0.1, _dropout.draw_seed())[0], s1[0])
    own = torch.Generator().manual_seed(4321)
    xc = x.cuda()
    assert same_bits(_dropout.bias_dropout_add(xc, b.cuda(), r.cuda(), p=0.1, generator=own), s1[0])
    # leading dimensions are rows; a view that is not contiguous and a float64 x go through torch ops
    o3 = _dropout.bias_dropout_add(xc.view(1, 257, 768), b.cuda(), r.cuda().view(1, 257, 768), p=0.1, seed=5)
    assert o3.shape == (1, 257, 768) and same_bits(o3.view(257, 768), a1[0])
    xt = xc.t().contiguous().t()
    assert not xt.is_contiguous() and same_bits(_dropout.bias_dropout_add(xt, b.cuda(), r.cuda(), p=0.1, seed=5), a1[0])
    o64 = _dropout.bias_dropout_add(xc.double(), b.cuda().double(), r.cuda().double(), p=0.1, seed=5)
    assert o64.dtype == torch.float32 and same_bits(o64, restate(x.float(), b, r.float(), p=0.1, seed=5)["out"])


@pytest.mark.gpu
def test_no_rows_launch_nothing(hip):
    before = dict(_dropout.stats)
    x = torch.zeros(0, 12, device="cuda", requires_grad=True)
    b = torch.ones(12, device="cuda", requires_grad=True)
    r = torch.zeros(0, 12, device="cuda", requires_grad=True)
    out = _dropout.bias_dropout_add(x, b, r, p=0.5, seed=1)
    out.sum().backward()
    assert out.shape == (0, 12) and x.grad.shape == (0, 12) and r.grad.shape == (0, 12)
    assert same_bits(b.grad, torch.zeros(12)) and _dropout.stats == before
    out = _dropout.bias_dropout_add(torch.zeros(3, 0, 12, device="cuda"), b, activation="relu")
    assert out.shape == (3, 0, 12) and _dropout.stats == before


@pytest.mark.gpu
def test_module_in_train_and_eval_mode(hip):
    x, b, r, g = make(129, 40, F16, 2)
    m = _dropout.BiasDropoutAdd(p=0.4)
    assert m.training and "p=0.4" in repr(m)
    torch.manual_seed(8)
    got = m(x.cuda(), b.cuda(), r.cuda())
    torch.manual_seed(8)
    assert same_bits(got, restate(x, b, r, p=0.4, seed=_dropout.draw_seed())["out"])
    m.eval()
    state = torch.get_rng_state()
    assert same_bits(m(x.cuda(), b.cuda(), r.cuda()), restate(x, b, r, p=0)["out"])
    assert same_bits(m(x.cuda(), b.cuda(), r.cuda()), _dropout.bias_dropout_add(x.cuda(), b.cuda(), r.cuda(), p=0))
    assert torch.equal(torch.get_rng_state(), state)
    relu = _dropout.BiasDropoutAdd(p=0.4, activation="relu").eval()
    assert same_bits(relu(x.cuda(), b.cuda()), torch.relu(x.float() + b).to(F16))


if __name__ == "__main__":
    if sys.argv[1:] == ["--abi-checks"]:
        abi_checks()
