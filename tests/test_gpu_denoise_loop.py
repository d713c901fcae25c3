"""Direct numerics of the denoising loop (GPU box only): nova_decoder_denoise and nova_decoder_denoise_echo called at the
ABI on freshly allocated buffers, every sampler branch, against the float64 restatement of tests/denoise_ref.py (pinned
against the project's PyTorch modules in tests/test_denoise_restatement_cpu.py). No pipeline, no encoder.

Shapes (B, n, P), the smallest at which each mechanism changes:
  ragged 3, 7, 3     B n = 21 is no multiple of the head kernel's 4 rows per workgroup; n P = 21 < one 256-thread pass of the
                     renorm kernels
  cross  2, 100, 3   n P = 300 crosses 256; 2-pass rows = 400 > 320, 1-pass rows = 200 <= 320: a truncated plan flips the
                     fused-m1 rule in the middle of one call at D = 768 / 1024
  wide-P 2, 5, 12 and 1, 3, 64 (the patch embed's limit; 65 is refused)
D 128 and 1536 never take the small-M kernel (1536: six passes of the head kernel's lane loop; 128: half a wave idle there);
depth 3 = first / middle / last block; steps 4.

Bounds.
  f32: max-abs error over max-abs of the reference < 1e-4, the bound the project holds whole f32 pipelines to; the same for
  the echo energy and the echo rows. Inputs are drawn so that a plain float32 run of the restatement itself stays within a
  third of that bound (case_is_fit: decided on the reference alone). The first choice of the clip cases (guidance 4) did not:
  with the DDPM epsilon step (kx = 17.4 at the first of 4 steps) plain CPU float32 measured 1.04e-4 on cross / D = 768 and the
  library 1.06e-4; the clip cases now run at guidance 1.5.
  16-bit: the yardstick is e_store, the error of denoise_ref(store=dtype) against denoise_ref(store=None): the reference
  measured against itself. The library must stay within FACTOR x e_store in max-abs and in rms (its f32 accumulation and
  16-bit output roundings are independent draws of the size of the emulation's, compounded over steps x depth). For the echo
  energy and the echo rows e_store is pooled over POOL input draws (pooled_echo_yardstick says why: a single draw of it is a
  handful of samples; against single draws the library measured up to 3.7 x on cases where e_store happened to come out low).
  The sampler arithmetic is f32 in every mode, so no quantity is asked to be better than the f32 bound (where e_store is 0 -
  a ratio clamped in every step makes the echo rows independent of the network - the f32 bound is what holds).

Measured on the MI355X: library error / e_store, the largest over the branches of a row, max-abs | rms, and the branch with
the largest; outputs whose bound is the f32 floor left out. Several are above 1.5, so FACTOR stays 3.
  dtype     shape          output  ratio
  bfloat16  ragged D=128   x     1.43 | 1.11   (ddpm_sample_clip)
  bfloat16  ragged D=128   echo  1.46 | 1.26   (renorm_above)
  bfloat16  cross D=768    x     1.47 | 1.13   (image_renorm)
  bfloat16  cross D=768    echo  1.67 | 1.59   (echo_ne100)
  bfloat16  cross D=1024   x     1.01 | 1.00   (euler_trunc)
  bfloat16  cross D=1024   echo  0.42 | 0.44   (echo_ne9)
  bfloat16  cross D=1536   x     0.98 | 0.99   (euler_trunc)
  bfloat16  cross D=1536   echo  0.21 | 0.27   (echo_ne9)
  bfloat16  p12 D=128      x     1.00 | 1.00   (euler_trunc)
  bfloat16  p12 D=128      echo  1.23 | 1.13   (echo_ne9)
  bfloat16  p64 D=128      x     1.08 | 1.00   (echo_ne9)
  bfloat16  p64 D=128      echo  0.51 | 0.53   (echo_ne9)
  float16   ragged D=128   x     2.08 | 1.30   (ddpm_sample)
  float16   ragged D=128   echo  1.80 | 2.02   (renorm_above)
  float16   cross D=768    x     1.85 | 1.08   (ddpm_sample)
  float16   cross D=768    echo  1.20 | 1.50   (spatiotemporal_renorm)
  float16   cross D=1024   x     1.65 | 1.07   (euler_trunc)
  float16   cross D=1024   echo  1.39 | 1.41   (echo_ne9)
  float16   cross D=1536   x     0.97 | 1.02   (echo_ne9)
  float16   cross D=1536   echo  0.33 | 0.32   (echo_ne9)
  float16   p12 D=128      x     1.00 | 1.00   (euler_trunc)
  float16   p12 D=128      echo  0.45 | 0.54   (echo_ne9)
  float16   p64 D=128      x     1.00 | 1.02   (echo_ne9)
  float16   p64 D=128      echo  1.47 | 1.49   (echo_ne9)
f32, largest max-abs error: 4.1e-5 (echo_ne0_clip, cross D=768; plain CPU float32 on the same case: 2.8e-5).
"""
import ctypes
import functools

import pytest
import torch

import denoise_ref as R

pytestmark = pytest.mark.gpu

DEV = "cuda"
DTYPES = [torch.float32, torch.bfloat16, torch.float16]
F32_BOUND = 1e-4
FACTOR = 3.0
STEPS, DEPTH = 4, 3
MAX_DRAWS = 16  # inputs are redrawn until case_is_fit() holds on the float64 reference alone
POOL = 4  # input draws behind the 16-bit yardstick of the echo outputs (pooled_echo_yardstick)
NOVA_ERR_ARG, NOVA_ERR_SHAPE = -1, -2

SHAPES, BRANCHES = R.SHAPES, R.BRANCHES  # one definition with the recorded bits (test_gpu_denoise_bits.py)
RENORM_BRANCHES = [k for k, v in BRANCHES.items() if v.get("renorm", 1.0) < 1]
GRAPH_BRANCHES = R.GRAPH_BRANCHES  # what may be captured


def bits(t):
    return t.contiguous().view(torch.int32)


def same_bits(a, b):
    return a.shape == b.shape and torch.equal(bits(a), bits(b))


def errs(got, ref):
    """(max-abs, rms) error over the max-abs of the reference."""
    d, scale = (got.double() - ref.double()).abs(), ref.double().abs().max().clamp_min(1e-30)
    return (d.max() / scale).item(), (d.pow(2).mean().sqrt() / scale).item()


@functools.lru_cache(maxsize=None)
def weights(D, depth, P):
    return R.make_decoder(D, depth, P, None, seed=R.weights_seed(D, depth, P))[0]


_packs = {}


def pack_for(hip, D, depth, P, dtype):
    key = (D, depth, P, dtype)
    if key not in _packs:
        _packs[key] = R.make_decoder(D, depth, P, dtype, seed=R.weights_seed(D, depth, P), hip=hip, device=DEV)[1]
    return _packs[key]


@functools.lru_cache(maxsize=None)
def case(shape, D, branch, depth=DEPTH, steps=STEPS):
    """Inputs, plan and the float64 reference of one case (CPU only; shared by every test and dtype that uses it)."""
    for draw in range(MAX_DRAWS):
        c = draw_case(shape, D, branch, depth, steps, draw)
        if case_is_fit(c):
            return c
    raise AssertionError(f"no fit inputs for {shape}/{D}/{branch} in {MAX_DRAWS} draws")


def draw_case(shape, D, branch, depth, steps, draw):
    c = R.draw_inputs(shape, D, branch, depth, steps, draw)
    c["ref"] = reference(c, None)
    return c


def outputs(res):
    out = [("x", res.x)]
    if res.echo_energy is not None:
        out.append(("echo energy", res.echo_energy))
    if res.echo_rows is not None and res.echo_rows.numel():
        out.append(("echo rows", res.echo_rows))
    return out


def case_is_fit(c):
    """Decided on the reference alone. (1) The case exercises what it is for (check_reference_regime). (2) It is conditioned well
    enough for the f32 bound to say something: a plain float32 run of the restatement (arith=float32: torch's CPU float32, nothing
    of the library) must itself stay within F32_BOUND / 3 of the float64 run. The library's f32 error is another draw of that
    size, and the largest of a few hundred such errors easily differs by 2 between draws; where plain float32 is itself at the
    bound (the DDPM epsilon step has kx = 17.4, kv = -17.4 at the first of 4 steps, and guidance extrapolation multiplies the gain
    every later step applies to what the clamp let through) the bound could only be met by luck."""
    try:
        check_reference_regime(c)
    except AssertionError:
        return False
    plain = reference(c, None, arith=torch.float32)
    c["plain_f32"] = max(errs(got, ref)[0] for (_, got), (_, ref) in zip(outputs(plain), outputs(c["ref"])))
    return 3 * c["plain_f32"] <= F32_BOUND


def reference(c, store, arith=torch.float64):
    return R.denoise_ref(weights(c["D"], c["depth"], c["P"]), c["zc"], c["temb"], c["x"], c["plan"], c["noise"], c["renorm"], c["energy"],
                         c["echo_rows"], c["echo_noise"], B=c["B"], n=c["n"], P=c["P"], D=c["D"], store=store, arith=arith)


@functools.lru_cache(maxsize=None)
def stored_reference(shape, D, branch, depth, steps, dtype):
    return reference(case(shape, D, branch, depth, steps), dtype)


@functools.lru_cache(maxsize=None)
def pooled_echo_yardstick(shape, D, branch, depth, steps, dtype):
    """e_store of the echo energy / echo rows as {name: (max-abs, rms)}, each the root mean square over POOL input draws of the
    case's branch and shape. These outputs depend on the network through ONE scalar (the renorm ratio) per (step, sample) - 4 to
    12 numbers a case - so a single draw's e_store is a handful of samples: over 8 draws of one case it ranges over a factor 5
    (3e-4 .. 1.5e-3 for the bf16 echo rows of echo_spatiotemporal / ragged) while that of x, hundreds of values, moves by less
    than 2. A ratio of two such draws says nothing; the pool estimates the size the emulation's error has on this case."""
    acc = {}
    for draw in range(POOL):
        c = draw_case(shape, D, branch, depth, steps, draw)
        for (name, s), (_, r) in list(zip(outputs(reference(c, dtype)), outputs(c["ref"])))[1:]:
            acc.setdefault(name, []).append(errs(s, r))
    rms = lambda v: (sum(t * t for t in v) / len(v)) ** 0.5
    return {name: (rms([e[0] for e in v]), rms([e[1] for e in v])) for name, v in acc.items()}


def fresh_ws(c, dtype, **over):
    Ne = 0 if c["echo_rows"] is None else c["echo_rows"].shape[1]
    kw = dict(steps=c["steps"], S=c["passes"] * c["B"], B=c["B"], n=c["n"], P=c["P"], D=c["D"], depth=c["depth"], Ne=Ne)
    kw.update(over)
    return R.Workspaces(dtype, DEV, **kw)


def run(hip, c, dtype, ws=None, **kw):
    pack = pack_for(hip, c["D"], c["depth"], c["P"], dtype)
    ws = fresh_ws(c, dtype) if ws is None else ws
    args = dict(B=c["B"], n=c["n"], P=c["P"], D=c["D"])
    args.update(kw)
    return R.run_hip(hip, pack, ws, c["zc"], c["temb"], c["x"], c["plan"], c["noise"], c["renorm"], c["energy"], c["echo_rows"],
                     c["echo_noise"], **args)


def assert_same(a, b, what):
    for name, u, v in zip(("x", "echo energy", "echo rows"), a, b):
        assert (u is None) == (v is None)
        if u is not None:
            assert same_bits(u, v), (what, name, (u.double() - v.double()).abs().max().item())


def check_reference_regime(c):
    """What the case is meant to exercise, asserted on the float64 reference alone."""
    ratio = c["ref"].ratio
    if c["regime"] == "below":
        assert (ratio < c["renorm"]).any(), ratio
    elif c["regime"] == "inside":
        assert ((ratio > c["renorm"]) & (ratio < 1)).any(), ratio
    elif c["regime"] == "above":
        assert (ratio > 1.01).any(), ratio  # far enough above 1 that a missing upper clamp shows
    if c["clip"] > 0:
        changed, met = c["ref"].clipped
        assert 0.05 <= changed / met <= 0.95, (changed, met)


def check_against_reference(got, c, dtype):
    ref = c["ref"]
    pairs = [("x", got[0], ref.x)]
    if got[1] is not None:
        pairs.append(("echo energy", got[1], ref.echo_energy))
    if got[2] is not None and got[2].numel():
        pairs.append(("echo rows", got[2], ref.echo_rows))
    st = None if dtype == torch.float32 else stored_reference(c["shape"], c["D"], c["branch"], c["depth"], c["steps"], dtype)
    for name, g, r in pairs:
        assert torch.isfinite(g).all(), name
        e_max, e_rms = errs(g, r)
        if st is None:
            print(f"denoise {c['branch']} {c['shape']} D={c['D']} f32 {name}: max {e_max:.3e} rms {e_rms:.3e}")
            assert e_max < F32_BOUND, (name, e_max)
            continue
        if name == "x":
            s_max, s_rms = errs(st.x, r)
        else:
            s_max, s_rms = pooled_echo_yardstick(c["shape"], c["D"], c["branch"], c["depth"], c["steps"], dtype)[name]
        print(f"denoise {c['branch']} {c['shape']} D={c['D']} {dtype} {name}: max {e_max:.3e} rms {e_rms:.3e}; e_store max {s_max:.3e} "
              f"rms {s_rms:.3e}; ratio max {e_max / max(s_max, 1e-30):.2f} rms {e_rms / max(s_rms, 1e-30):.2f}")
        assert e_max <= max(FACTOR * s_max, F32_BOUND), (name, "max", e_max, s_max)
        assert e_rms <= max(FACTOR * s_rms, F32_BOUND), (name, "rms", e_rms, s_rms)


def check_case(hip, c, dtype):
    check_reference_regime(c)
    got = run(hip, c, dtype)
    check_against_reference(got, c, dtype)
    if c["steps"] > 1:
        assert_same(run(hip, c, dtype, mod_steps=1), got, "mod_steps = 1 vs steps")
    try:
        hip.call("nova_debug_force_gemm_tile", 128)
        assert_same(run(hip, c, dtype), got, "128-tile GEMMs (separate modulate launch) vs automatic")
    finally:
        hip.call("nova_debug_force_gemm_tile", 0)
    return got


# ---------------------------------------------------------------------------------------------
# every sampler branch, against the reference and against itself
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("shape,D", [("ragged", 128), ("cross", 768)])
@pytest.mark.parametrize("branch", list(BRANCHES))
def test_sampler_branch(hip, branch, shape, D, dtype):
    check_case(hip, case(shape, D, branch), dtype)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("shape,D", [("cross", 1024), ("cross", 1536), ("p12", 128), ("p64", 128)])
@pytest.mark.parametrize("branch", ["euler_trunc", "echo_ne9"])
def test_wide_rows_and_patches(hip, branch, shape, D, dtype):
    """D = 1024 flips the fused-m1 rule where the plan truncates (400 -> 200 rows), D = 1536 never takes the small-M kernel;
    P = 12 and P = 64 (the limit of the patch embed)."""
    check_case(hip, case(shape, D, branch), dtype)


@pytest.mark.parametrize("dtype", DTYPES)
def test_depth_one(hip, dtype):
    """One block: it is the first and the last at once (its chain launch carries the final modulate)."""
    check_case(hip, case("cross", 768, "euler_trunc", 1, STEPS), dtype)


@pytest.mark.parametrize("dtype", DTYPES)
def test_single_step(hip, dtype):
    """steps = 1 with mod_steps = 1 = steps: the direct path, no hoisted projection."""
    c = case("cross", 768, "euler_cfg", DEPTH, 1)
    got = run(hip, c, dtype, mod_steps=1)
    check_against_reference(got, c, dtype)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("shape,D", [("ragged", 128), ("cross", 768)])
@pytest.mark.parametrize("branch", RENORM_BRANCHES)
def test_renorm_sample_alone_equals_sample_in_batch(hip, branch, shape, D, dtype):
    """The per-sample sums must not depend on B: the last sample run alone (B = 1, fresh buffers) gives the bits it has inside
    the batch."""
    c = case(shape, D, branch)
    B, n, b = c["B"], c["n"], c["B"] - 1
    got = run(hip, c, dtype)
    one = dict(c, B=1, zc=torch.cat([c["zc"][(q * B + b) * n:(q * B + b + 1) * n] for q in range(c["passes"])]), x=c["x"][b:b + 1],
               noise=None if c["noise"] is None else c["noise"][:, b:b + 1].contiguous(),
               energy=None if c["energy"] is None else c["energy"][b:b + 1],
               echo_rows=None if c["echo_rows"] is None else c["echo_rows"][b:b + 1],
               echo_noise=None if c["echo_noise"] is None else c["echo_noise"][:, b:b + 1].contiguous())
    alone = run(hip, one, dtype)
    assert_same(alone, tuple(None if t is None else t[b:b + 1] for t in got), "sample alone vs in the batch")


# ---------------------------------------------------------------------------------------------
# hipGraph replay and its cache key
# ---------------------------------------------------------------------------------------------
@pytest.fixture()
def side_stream():
    """The legacy default stream cannot be captured: the graph tests run on a stream of their own."""
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        yield s
    s.synchronize()


@pytest.fixture()
def graphs(hip):
    hip.set_graphs(False)  # drops what earlier tests captured: a fresh buffer may land on an old address
    hip.set_graphs(True)
    yield hip
    hip.set_graphs(True)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("shape,D", [("ragged", 128), ("cross", 768)])
@pytest.mark.parametrize("branch", GRAPH_BRANCHES)
def test_graph_replay_equals_direct_launches(graphs, side_stream, branch, shape, D, dtype):
    hip = graphs
    c = case(shape, D, branch)
    ws = fresh_ws(c, dtype)
    try:
        c0, r0 = hip.graph_stats()
        captured = run(hip, c, dtype, ws=ws)
        assert hip.graph_stats() == (c0 + 1, r0), "the first call must capture (and launch) one graph"
        replayed = run(hip, c, dtype, ws=ws)  # run_hip restores x in the same buffers
        assert hip.graph_stats() == (c0 + 1, r0 + 1), "an argument-identical call must replay"
        hip.set_graphs(False)
        direct = run(hip, c, dtype, ws=ws)
        assert hip.graph_stats()[1] == r0 + 1
    finally:
        hip.set_graphs(True)
    assert_same(captured, direct, "capture call vs direct launches")
    assert_same(replayed, direct, "replay vs direct launches")


def test_graph_cache_key(graphs, side_stream):
    """One capture per distinct argument set; a plan that differs in one c0 is a different set; the 4 bytes of padding
    between nova_decoder's `depth` and `blocks` are not an argument."""
    hip = graphs
    dtype = torch.float32
    c = case("ragged", 128, "euler_cfg")
    ws = fresh_ws(c, dtype)
    pack = pack_for(hip, c["D"], c["depth"], c["P"], dtype)
    c0, r0 = hip.graph_stats()
    first = run(hip, c, dtype, ws=ws)
    second = run(hip, c, dtype, ws=ws)
    assert hip.graph_stats() == (c0 + 1, r0 + 1)
    assert_same(first, second, "replay")
    assert hip.Decoder.blocks.offset == 8 and ctypes.sizeof(ctypes.c_int) == 4  # the hole is bytes 4 .. 7
    copy = hip.Decoder.from_buffer_copy(pack.struct)
    ctypes.memset(ctypes.addressof(copy) + 4, 0xA5, 4)
    third = run(hip, c, dtype, ws=ws, struct=copy)
    assert hip.graph_stats() == (c0 + 1, r0 + 2), "the struct's padding bytes entered the graph key"
    assert_same(third, first, "struct copy with other padding bytes")
    plan = list(c["plan"])
    plan[1] = plan[1]._replace(c0=R.f32(plan[1].c0 * 1.5))
    other = dict(c, plan=plan)
    fourth = run(hip, other, dtype, ws=ws)
    assert hip.graph_stats() == (c0 + 2, r0 + 2), "a plan with another c0 must capture anew"
    assert not same_bits(fourth[0], first[0])
    e_max, _ = errs(fourth[0], reference(other, None).x)
    assert e_max < F32_BOUND, e_max


# ---------------------------------------------------------------------------------------------
# refusals: the documented error code, nothing launched, x untouched
# ---------------------------------------------------------------------------------------------
def refused(hip, c, dtype, code, ws=None, **kw):
    ws = fresh_ws(c, dtype, S=3 * c["B"]) if ws is None else ws
    with pytest.raises(hip.NovaHipError) as e:
        run(hip, c, dtype, ws=ws, **kw)
    torch.cuda.synchronize()
    assert R.error_code(e.value) == code, str(e.value)
    assert same_bits(ws.x.view(-1)[: c["x"].numel()].cpu(), c["x"].reshape(-1)), "a refused call changed x"
    for name in ("a", "mod", "u", "h", "f", "g", "v"):
        assert torch.isnan(getattr(ws, name)).all(), f"a refused call wrote workspace {name}"
    return ws


def with_step(c, i, **fields):
    plan = list(c["plan"])
    plan[i] = plan[i]._replace(**fields)
    return dict(c, plan=plan)


def test_refusals(hip):
    dtype = torch.float32
    c = case("ragged", 128, "euler_cfg")
    hip.set_graphs(False)
    try:
        refused(hip, c, dtype, NOVA_ERR_ARG, mod_steps=2)
        refused(hip, c, dtype, NOVA_ERR_SHAPE, S=2 * c["B"] + 1)
        refused(hip, c, dtype, NOVA_ERR_SHAPE, S=4 * c["B"])
        refused(hip, with_step(c, 1, extra_kind=3), dtype, NOVA_ERR_ARG)
        refused(hip, with_step(c, 2, extra_kind=1), dtype, NOVA_ERR_SHAPE)  # on the direct path: steps 0 and 1 must not have run
        refused(hip, dict(c, P=65), dtype, NOVA_ERR_SHAPE)
        # guidance renorm on the scalar echo energy with a step that is not the Euler step, with and without guidance on that step
        r = case("ragged", 128, "renorm_inside")
        ddpm = R.make_plan(R.ddpm_coefs(STEPS, "epsilon"), 4.0)[2]
        refused(hip, with_step(r, 2, **ddpm._asdict()), dtype, NOVA_ERR_ARG)
        refused(hip, with_step(r, 2, **ddpm._replace(guidance=1.0)._asdict()), dtype, NOVA_ERR_ARG)
        # the echo entry: renorm >= 1, and no echo rows
        e = case("ragged", 128, "echo_ne9")
        refused(hip, dict(e, renorm=1.0), dtype, NOVA_ERR_ARG)
        refused(hip, e, dtype, NOVA_ERR_ARG, null_echo=True)
        # n = 0: nothing to do, success
        ws = fresh_ws(c, dtype)
        run(hip, c, dtype, ws=ws, n=0, S=2 * c["B"])
        assert same_bits(ws.x.cpu(), c["x"]) and torch.isnan(ws.u).all()
    finally:
        hip.set_graphs(True)


def test_refusal_during_capture_leaves_the_stream_usable(graphs, side_stream):
    """Step 2 needs three passes but S = 2B: the plan is refused while the stream is capturing. The capture must be closed, x
    untouched, and the next valid call on the same stream must run and be right."""
    hip = graphs
    dtype = torch.float32
    c = case("ragged", 128, "euler_cfg")
    ws = refused(hip, with_step(c, 2, extra_kind=1, extra_scale=1.5), dtype, NOVA_ERR_SHAPE, ws=fresh_ws(c, dtype))
    got = run(hip, c, dtype, ws=ws)
    e_max, _ = errs(got[0], c["ref"].x)
    assert e_max < F32_BOUND, e_max
