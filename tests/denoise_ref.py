"""A float64 restatement of the denoising loop (`nova_decoder_denoise`, `nova_decoder_denoise_echo`) and the plumbing to
call the two entry points directly. A plain helper module (like golden_util.py), shared by test_denoise_restatement_cpu.py,
which pins the restatement against the project's PyTorch modules without a GPU, test_gpu_denoise_loop.py and the recorded
bits (golden/make_golden_denoise_bits.py); the last two build their cases from SHAPES, BRANCHES and draw_inputs below.

`denoise_ref` is written from the definitions in include/nova_hip.h (`nova_sampler_step`, `nova_decoder_denoise`,
`nova_decoder_denoise_echo`) and diffnext/models/diffusion_mlp.py, not from the kernels: one plain loop, all arithmetic in
float64, one code path for every shape. The sampler step's `clip` is a number in the plan like the other coefficients.
"""
import collections
import ctypes
import re
import zlib

import numpy as np
import torch

Step = collections.namedtuple("Step", "guidance kx kv clip c0 cx sigma extra_scale extra_kind")
Result = collections.namedtuple("Result", "x echo_energy echo_rows ratio clipped")
# ratio   [steps, B] float64: the guidance-renorm factor BEFORE clamping to [renorm, 1]; NaN where a step does not renormalise
# clipped (values of x0 the clamp changed, values of x0 that met a clamp) over predicted and echo rows, all steps


def f32(v):
    return float(np.float32(v))


def step(guidance=1.0, kx=0.0, kv=1.0, clip=0.0, c0=0.0, cx=1.0, sigma=0.0, extra_scale=0.0, extra_kind=0, exact=False):
    """One plan entry; the coefficients rounded to float32 (what `nova_sampler_step` holds) unless `exact`."""
    r = (lambda v: float(v)) if exact else f32
    return Step(r(guidance), r(kx), r(kv), r(clip), r(c0), r(cx), r(sigma), r(extra_scale), int(extra_kind))


def make_plan(coefs, guidance, extra_scale=0.0, extra_kind=0, clip=None, exact=False):
    """`coefs` as engine.sampler_plan returns them ((kx, kv, clip, c0, cx, sigma) per step), `guidance` one value or one per step."""
    g = list(guidance) if isinstance(guidance, (list, tuple)) else [guidance] * len(coefs)
    return [step(g[i], c[0], c[1], c[2] if clip is None else clip, c[3], c[4], c[5], extra_scale, extra_kind, exact=exact)
            for i, c in enumerate(coefs)]


def _stored(t, store):
    return t if store is None else t.to(store).to(t.dtype)


def _ln(x, eps):
    mu = x.mean(-1, keepdim=True)
    var = ((x - mu) ** 2).mean(-1, keepdim=True)
    return (x - mu) / torch.sqrt(var + eps)


def _silu(x):
    return x / (1 + torch.exp(-x))


def denoise_ref(dec, zc, temb, x, sched, noise, renorm, echo_energy=None, echo_rows=None, echo_noise=None, *, B, n, P, D,
                store=None, arith=torch.float64):
    """dec: dict of CPU tensors (adaln_w [(3 depth + 2) D, D], adaln_b, patch_w [D, P], patch_b, head_w [P, D], head_b and
    blocks: list of dicts fc1_w, fc1_b, fc2_w, fc2_b, norm2_w, norm2_b); zc [S n, D]; temb [steps, D]; x [B, n, P];
    sched: list of Step; noise [steps, B, n, P] or None; echo_energy [B] (the scalar form of nova_decoder_denoise) or
    echo_rows [B, Ne, P] with echo_noise [steps, B, Ne, P] or None (nova_decoder_denoise_echo).
    `store`: the library's storage dtype; what it keeps in that dtype is rounded to it where it is stored.
    `arith`: float64, always, for a reference. float32 turns the same lines into a plain float32 implementation, whose error against
    the float64 run tells how well conditioned a case is (what ANY float32 implementation can be asked to reach on it)."""
    A = arith
    q = lambda t: _stored(t.to(A), store)
    depth = len(dec["blocks"])
    aw, pw, hw = q(dec["adaln_w"]), q(dec["patch_w"]), q(dec["head_w"])
    ab, pb, hb = dec["adaln_b"].to(A), dec["patch_b"].to(A), dec["head_b"].to(A)
    blocks = [{k: (q(v) if k in ("fc1_w", "fc2_w") else v.to(A)) for k, v in blk.items()} for blk in dec["blocks"]]
    zc, temb = q(zc).view(-1, n, D), q(temb)
    x = x.to(A).clone().view(B, n, P)
    E = None if echo_energy is None else echo_energy.to(A).clone()
    rows_e = None if echo_rows is None else echo_rows.to(A).clone()
    do_renorm = renorm < 1
    ratios = torch.full((len(sched), B), float("nan"), dtype=A)
    changed = met = 0

    def sampler(sp, xo, v, nz):
        nonlocal changed, met
        x0 = sp.kx * xo + sp.kv * v
        if sp.clip > 0:
            lim = x0.clamp(-sp.clip, sp.clip)
            changed, met = changed + int((lim != x0).sum()), met + x0.numel()
            x0 = lim
        xn = sp.c0 * x0 + sp.cx * xo
        if nz is not None and sp.sigma != 0:
            xn = xn + sp.sigma * nz.to(A)
        return xn

    for i, sp in enumerate(sched):
        cfg = sp.guidance > 1
        passes = (3 if sp.extra_kind else 2) if cfg else 1
        z = zc[: passes * B]                                                     # [passes B, n, D]
        a = _stored(_silu(z + temb[i]), store)                                    # ws_a
        mod = _stored(a @ aw.T + ab, store)                                       # ws_mod
        u = _stored(x.repeat(passes, 1, 1) @ pw.T + pb, store)                    # ws_u: every pass embeds the same x
        for b, blk in enumerate(blocks):
            scale, shift, gate = (mod[..., (3 * b + k) * D:(3 * b + k + 1) * D] for k in range(3))
            h = _stored(_ln(u, 1e-6) * (1 + scale) + shift, store)                # ws_h
            f = _stored(_silu(h @ blk["fc1_w"].T + blk["fc1_b"]), store)          # ws_f
            g = _stored(f @ blk["fc2_w"].T + blk["fc2_b"], store)                 # ws_g
            u = _stored((_ln(g, 1e-5) * blk["norm2_w"] + blk["norm2_b"]) * gate + u, store)
        scale, shift = mod[..., 3 * depth * D:(3 * depth + 1) * D], mod[..., (3 * depth + 1) * D:(3 * depth + 2) * D]
        h = _stored(_ln(u, 1e-6) * (1 + scale) + shift, store)
        out = (h @ hw.T + hb).view(passes, B, n, P)
        ratio = torch.ones(B, dtype=A)
        if not cfg:
            v = out[0]
        else:
            c, un = out[0], out[1]
            if sp.extra_kind == 1:
                vhat, extra = un + (c - out[2]) * sp.guidance, (out[2] - un) * sp.extra_scale
            elif sp.extra_kind == 2:
                vhat, extra = un + (c - un) * sp.guidance, (c - out[2]) * sp.extra_scale
            else:
                vhat, extra = un + (c - un) * sp.guidance, 0.0
            if do_renorm:
                # the norms run over ALL rows of a sample; on a row that is not predicted every pass returns x_t
                e2 = rows_e.pow(2).sum((1, 2)) if rows_e is not None else E
                raw = torch.sqrt((c.pow(2).sum((1, 2)) + e2) / (vhat.pow(2).sum((1, 2)) + e2))
                ratios[i] = raw
                ratio = raw.clamp(renorm, 1.0)
            v = ratio.view(B, 1, 1) * vhat + extra
        x = sampler(sp, x, v, None if noise is None else noise[i].view(B, n, P))
        if do_renorm and rows_e is not None:
            rows_e = sampler(sp, rows_e, ratio.view(B, 1, 1) * rows_e, None if echo_noise is None else echo_noise[i])
        elif do_renorm and E is not None:
            # the Euler step x <- x + c0 v on rows with v = ratio x: their squared norm takes the factor squared
            E = E * (1 + sp.c0 * ratio) ** 2
    return Result(x, E, rows_e, ratios, (changed, met))


# ---------------------------------------------------------------------------------------------
# weights, ctypes structs, workspaces
# ---------------------------------------------------------------------------------------------
def bf16_round(t):
    return t.to(torch.bfloat16).float()


def make_weights(D, depth, P, seed):
    """Decoder weights drawn in f32 and rounded to bf16 once, so that f32, bf16 and f16 runs share them (f16 rounds the
    bf16 values again where they leave its range; `denoise_ref(store=float16)` does the same)."""
    g = torch.Generator().manual_seed(seed)
    rn = lambda *s, scale=1.0: torch.randn(*s, generator=g) * scale
    w = {"adaln_w": bf16_round(rn((3 * depth + 2) * D, D, scale=0.5 / D ** 0.5)), "adaln_b": rn((3 * depth + 2) * D, scale=0.1),
         "patch_w": bf16_round(rn(D, P, scale=1.0 / P ** 0.5)), "patch_b": rn(D, scale=0.1),
         "head_w": bf16_round(rn(P, D, scale=1.0 / D ** 0.5)), "head_b": rn(P, scale=0.1), "blocks": []}
    for _ in range(depth):
        w["blocks"].append({"fc1_w": bf16_round(rn(D, D, scale=1.0 / D ** 0.5)), "fc1_b": rn(D, scale=0.1),
                            "fc2_w": bf16_round(rn(D, D, scale=1.0 / D ** 0.5)), "fc2_b": rn(D, scale=0.1),
                            "norm2_w": 1 + rn(D, scale=0.1), "norm2_b": rn(D, scale=0.1)})
    return w


class DecoderPack(object):
    """The weights (`w`, CPU), their device copies (kept alive here) and the `hip.Decoder` / `hip.MlpBlock` structs."""

    def __init__(self, hip, w, dtype, device):
        self.w, self.dtype, self.keep = w, dtype, []
        dev = lambda t, dt: self.keep.append(t.to(device=device, dtype=dt).contiguous()) or self.keep[-1].data_ptr()
        depth = len(w["blocks"])
        self.blocks = (hip.MlpBlock * depth)()
        for i, b in enumerate(w["blocks"]):
            self.blocks[i] = hip.MlpBlock(dev(b["fc1_w"], dtype), dev(b["fc1_b"], torch.float32), dev(b["fc2_w"], dtype),
                                          dev(b["fc2_b"], torch.float32), dev(b["norm2_w"], torch.float32), dev(b["norm2_b"], torch.float32))
        self.struct = hip.Decoder(depth, ctypes.cast(self.blocks, ctypes.POINTER(hip.MlpBlock)), dev(w["adaln_w"], dtype),
                                  dev(w["adaln_b"], torch.float32), dev(w["patch_w"], dtype), dev(w["patch_b"], torch.float32),
                                  dev(w["head_w"], dtype), dev(w["head_b"], torch.float32))


class Workspaces(object):
    """Freshly allocated buffers of one call shape, filled with NaN: a kernel that reads a row nobody wrote shows."""

    def __init__(self, dtype, device, *, steps, S, B, n, P, D, depth, Ne=0):
        e = lambda *s: torch.full(s, float("nan"), dtype=dtype, device=device)
        rows = S * n
        self.a, self.mod = e(steps * rows, D), e(steps * rows, (3 * depth + 2) * D)
        self.u, self.h, self.f, self.g = e(rows, D), e(rows, D), e(rows, D), e(rows, D)
        f = lambda *s: torch.full(s, float("nan"), dtype=torch.float32, device=device)
        self.v = f(3 * B * n * P)
        self.x, self.energy = f(B, n, P), f(B)
        self.echo = f(B, max(Ne, 1), P)  # never a null pointer, also for Ne = 0
        self.noise, self.echo_noise = f(steps, B, n, P), f(steps, B, max(Ne, 1), P)
        self.zc, self.temb = e(rows, D), e(steps, D)


def make_decoder(D, depth, P, dtype, seed, hip=None, device="cuda", **shape):
    """(weights, DecoderPack or None, Workspaces or None). Without `hip` only the weights are made (CPU tests);
    `shape` (steps, S, B, n and optionally Ne) asks for the workspaces too."""
    w = make_weights(D, depth, P, seed)
    pack = None if hip is None else DecoderPack(hip, w, dtype, device)
    ws = Workspaces(dtype, device, P=P, D=D, depth=depth, **shape) if (hip is not None and shape) else None
    return w, pack, ws


def plan_struct(hip, sched):
    plan = (hip.SamplerStep * len(sched))()
    for i, s in enumerate(sched):
        plan[i] = hip.SamplerStep(*s)
    return plan


def error_code(exc):
    """The nova_status inside the message of a NovaHipError raised by hip.call."""
    m = re.search(r"failed \((-?\d+)\)", str(exc))
    return int(m.group(1)) if m else None


def run_hip(hip, pack, ws, zc, temb, x, sched, noise, renorm, echo_energy=None, echo_rows=None, echo_noise=None, *, B, n, P, D,
            mod_steps=None, S=None, Ne=None, steps=None, struct=None, echo_entry=None, null_echo=False):
    """One call of nova_decoder_denoise (or, with `echo_rows` / `echo_entry`, nova_decoder_denoise_echo) through hip.call on
    the current stream: the inputs are copied into the buffers of `ws` (same addresses call after call), the call is made,
    and (x, echo energy or None, echo rows or None) come back as CPU tensors. Raises NovaHipError on a refusal."""
    dtype = pack.dtype
    steps = len(sched) if steps is None else steps
    S = zc.shape[0] // n if S is None else S
    use_echo = (echo_rows is not None) if echo_entry is None else echo_entry
    ne = (echo_rows.shape[1] if echo_rows is not None else 0) if Ne is None else Ne
    up = lambda buf, t: buf.view(-1)[: t.numel()].copy_(t.reshape(-1).to(buf.dtype), non_blocking=False)
    up(ws.zc, zc), up(ws.temb, temb), up(ws.x, x)
    if noise is not None:
        up(ws.noise, noise)
    if echo_energy is not None:
        up(ws.energy, echo_energy)
    if echo_rows is not None and echo_rows.numel():
        up(ws.echo, echo_rows)
    if echo_noise is not None and echo_noise.numel():
        up(ws.echo_noise, echo_noise)
    plan = plan_struct(hip, sched)
    dec = ctypes.byref(pack.struct if struct is None else struct)
    tail = (steps, S, B, n, P, D, ws.a.data_ptr(), ws.u.data_ptr(), ws.h.data_ptr(), ws.f.data_ptr(), ws.g.data_ptr(),
            ws.mod.data_ptr(), ws.v.data_ptr(), steps if mod_steps is None else mod_steps, hip.dtype_code(dtype), hip.stream_ptr())
    nz = None if noise is None else ws.noise.data_ptr()
    if use_echo:
        hip.call("nova_decoder_denoise_echo", dec, ws.zc.data_ptr(), ws.temb.data_ptr(), ws.x.data_ptr(), plan, nz, renorm,
                 None if null_echo else ws.echo.data_ptr(), None if echo_noise is None else ws.echo_noise.data_ptr(), ne, *tail)
    else:
        hip.call("nova_decoder_denoise", dec, ws.zc.data_ptr(), ws.temb.data_ptr(), ws.x.data_ptr(), plan, nz, renorm,
                 None if echo_energy is None else ws.energy.data_ptr(), *tail)
    torch.cuda.current_stream().synchronize()
    xo = ws.x.view(-1)[: x.numel()].view(x.shape).cpu()
    eo = None if echo_energy is None else ws.energy[:B].cpu()
    ro = None if echo_rows is None else ws.echo.view(-1)[: echo_rows.numel()].view(echo_rows.shape).cpu()
    return xo, eo, ro


# ---------------------------------------------------------------------------------------------
# inputs and plans shared by the CPU and the GPU tests
# ---------------------------------------------------------------------------------------------
def make_inputs(B, n, P, D, passes, steps, seed, Ne=0):
    """zc / temb already rounded to bf16 (exact in f32 and bf16; f16 rounds again, as `denoise_ref(store=float16)` does)."""
    g = torch.Generator().manual_seed(seed)
    rn = lambda *s: torch.randn(*s, generator=g)
    return {"zc": bf16_round(rn(passes * B * n, D)), "temb": bf16_round(rn(steps, D)), "x": rn(B, n, P), "noise": rn(steps, B, n, P),
            "echo_rows": rn(B, Ne, P), "echo_noise": rn(steps, B, Ne, P)}


def euler_coefs(steps):
    from nova_pointcloud_amd import engine
    from nova_pointcloud_amd.diffnext.schedulers import FlowMatchEulerDiscreteScheduler

    return engine.sampler_plan(FlowMatchEulerDiscreteScheduler(), steps)[1]


def ddpm_coefs(steps, prediction_type):
    from nova_pointcloud_amd import engine
    from nova_pointcloud_amd.diffnext.schedulers import DDPMScheduler

    return engine.sampler_plan(DDPMScheduler(prediction_type=prediction_type), steps)[1]


# ---------------------------------------------------------------------------------------------
# the cases of the GPU tests: shapes, sampler branches and the inputs / plan of one draw. One definition for the numerics
# (test_gpu_denoise_loop.py) and the recorded bits (golden/make_golden_denoise_bits.py, test_gpu_denoise_bits.py)
# ---------------------------------------------------------------------------------------------
SHAPES = {"ragged": (3, 7, 3), "cross": (2, 100, 3), "p12": (2, 5, 12), "p64": (1, 3, 64)}  # (B, n, P): test_gpu_denoise_loop.py says why

# name -> sampler ("euler" or a DDPM prediction type), guidance, and what differs from the plain 2-pass call
#   trunc: the last two steps run at guidance 1; extra: (extra_kind, extra_scale); energy: echo energy per predicted value
#   (the scalar entry); Ne: echo rows (the echo entry); regime: where the UNCLAMPED ratio of the reference must lie at least once
BRANCHES = {
    "euler_nocfg": dict(sampler="euler", g=1.0, passes=1),
    "euler_cfg": dict(sampler="euler", g=4.0),
    "euler_trunc": dict(sampler="euler", g=4.0, trunc=True),
    "renorm_floor_zero_energy": dict(sampler="euler", g=8.0, renorm=0.3, energy=0.0, regime="below"),
    "renorm_inside": dict(sampler="euler", g=4.0, trunc=True, renorm=0.3, energy=1.0, regime="inside"),
    "renorm_above": dict(sampler="euler", g=3.0, extra=(1, 1.5), third_is_cond=True, renorm=0.3, energy=0.1, regime="above"),
    "image": dict(sampler="euler", g=3.0, trunc=True, extra=(1, 1.5)),
    "image_renorm": dict(sampler="euler", g=3.0, trunc=True, extra=(1, 1.5), renorm=0.3, energy=1.0),
    "spatiotemporal": dict(sampler="euler", g=3.0, trunc=True, extra=(2, 1.5)),
    "spatiotemporal_renorm": dict(sampler="euler", g=3.0, trunc=True, extra=(2, 1.5), renorm=0.3, energy=1.0),
    "ddpm_epsilon": dict(sampler="epsilon", g=4.0, noise=True),
    "ddpm_v": dict(sampler="v_prediction", g=4.0, noise=True),
    "ddpm_sample": dict(sampler="sample", g=4.0, noise=True),
    "echo_ne0": dict(sampler="epsilon", g=4.0, noise=True, trunc=True, renorm=0.3, Ne=0),
    "echo_ne9": dict(sampler="epsilon", g=4.0, noise=True, trunc=True, renorm=0.3, Ne=9),
    "echo_ne100": dict(sampler="v_prediction", g=4.0, noise=True, trunc=True, renorm=0.3, Ne=100),
    "echo_spatiotemporal": dict(sampler="sample", g=3.0, noise=True, trunc=True, extra=(2, 1.5), renorm=0.3, Ne=9),
}
for _name in ("ddpm_epsilon", "ddpm_v", "ddpm_sample", "echo_ne0", "echo_ne9", "echo_ne100"):
    # g = 1.5: at g = 4 the clamp's survivors of the first DDPM steps carry errors no float32 run keeps below the f32 bound (case_is_fit)
    BRANCHES[_name + "_clip"] = dict(BRANCHES[_name], clip=1.0, g=1.5)
GRAPH_BRANCHES = [k for k, v in BRANCHES.items() if not v.get("noise") and v.get("renorm", 1.0) >= 1]  # what may be captured



def weights_seed(D, depth, P):
    """The seed of a case's decoder weights (make_weights / make_decoder)."""
    return 1000 + D + depth + P


def draw_inputs(shape, D, branch, depth, steps, draw):
    """Inputs and plan of one case (CPU tensors; no reference): draw `draw` of the seeded generator."""
    B, n, P = SHAPES[shape]
    spec = BRANCHES[branch]
    extra_kind, extra_scale = spec.get("extra", (0, 0.0))
    passes = spec.get("passes", 3 if extra_kind else 2)
    Ne = spec.get("Ne")
    inp = make_inputs(B, n, P, D, passes, steps, seed=zlib.crc32(f"{shape}/{D}/{branch}/{draw}".encode()), Ne=Ne or 0)
    if spec.get("third_is_cond"):  # image guidance with the third pass equal to the cond pass: v-hat = u exactly, ratio |c| / |u|
        inp["zc"] = torch.cat([inp["zc"][: 2 * B * n], inp["zc"][: B * n]])
    coefs = euler_coefs(steps) if spec["sampler"] == "euler" else ddpm_coefs(steps, spec["sampler"])
    g = [spec["g"]] * steps
    if spec.get("trunc"):
        g[-2:] = [1.0] * len(g[-2:])
    plan = make_plan(coefs, g, extra_scale, extra_kind, clip=spec.get("clip"))
    renorm = spec.get("renorm", 1.0)
    energy = None if "energy" not in spec else torch.full((B,), spec["energy"] * n * P) * (1 + 0.25 * torch.arange(B))
    c = dict(shape=shape, D=D, branch=branch, depth=depth, steps=steps, B=B, n=n, P=P, passes=passes, plan=plan, renorm=renorm,
             zc=inp["zc"], temb=inp["temb"], x=inp["x"], noise=inp["noise"] if spec.get("noise") else None, energy=energy,
             echo_rows=inp["echo_rows"] if Ne is not None else None, echo_noise=inp["echo_noise"] if Ne is not None else None,
             regime=spec.get("regime"), clip=spec.get("clip", 0.0), draw=draw)
    return c
