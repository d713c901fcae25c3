"""Pins tests/denoise_ref.py (the float64 restatement the GPU tests of the denoising loop compare with) against the
project's own PyTorch modules, in float64, without a GPU: `DiffusionMLP`, `GuidanceScaler`, `FlowMatchEulerDiscreteScheduler`
and `DDPMScheduler`, with the plan coefficients from `engine.sampler_plan`.

The comparison is the full-canvas form of `Transformer3DModel.denoise` (transformer_3d.py): ALL N rows of a sample go
through `GuidanceScaler.scale` and `scheduler.step`; the decoder is applied to the `pred_ids` rows and the other rows echo
x_t. The restatement sees only the predicted rows plus either the echo rows or, for the Euler step, their squared norm.
"""
import math

import pytest
import torch

import denoise_ref as R
from nova_pointcloud_amd import engine
from nova_pointcloud_amd.diffnext.models.diffusion_mlp import DiffusionMLP
from nova_pointcloud_amd.diffnext.models.guidance_scaler import GuidanceScaler
from nova_pointcloud_amd.diffnext.schedulers import DDPMScheduler, FlowMatchEulerDiscreteScheduler

F64 = torch.float64
B, N, n, P, D, DEPTH, STEPS = 2, 7, 3, 3, 16, 2, 4
TOL = 1e-12


def rel(a, b):
    return ((a.double() - b.double()).abs().max() / b.double().abs().max().clamp_min(1e-300)).item()


def build_module(seed):
    """A float64 DiffusionMLP (patch 1 x 1 over a [P, N, 1] image: a token's patch vector is its P channels) with random
    parameters, and the same parameters as the restatement's weight dict."""
    torch.manual_seed(seed)
    m = DiffusionMLP(DEPTH, D, D, patch_size=1, image_dim=P).double()
    with torch.no_grad():
        for p in m.parameters():
            p.copy_(torch.randn(p.shape, dtype=F64) * (0.3 if p.dim() > 1 else 0.1))
        for blk in m.blocks:
            blk.norm2.weight.add_(1.0)
    w = {"adaln_w": torch.cat([b.norm1.proj.weight for b in m.blocks] + [m.norm.proj.weight]).detach(),
         "adaln_b": torch.cat([b.norm1.proj.bias for b in m.blocks] + [m.norm.proj.bias]).detach(),
         "patch_w": engine.patch_weight(m.patch_embed.proj), "patch_b": m.patch_embed.proj.bias.detach(),
         "head_w": m.head.weight.detach(), "head_b": m.head.bias.detach(),
         "blocks": [{"fc1_w": b.proj.fc1.weight.detach(), "fc1_b": b.proj.fc1.bias.detach(), "fc2_w": b.proj.fc2.weight.detach(),
                     "fc2_b": b.proj.fc2.bias.detach(), "norm2_w": b.norm2.weight.detach(), "norm2_b": b.norm2.bias.detach()}
                    for b in m.blocks]}
    return m.eval(), w


def to_image(rows):  # [B, N, P] -> [B, P, N, 1]
    return rows.transpose(1, 2).unsqueeze(-1).contiguous()


def to_rows(img):
    return img.squeeze(-1).transpose(1, 2).contiguous()


def full_canvas(m, scheduler, scaler, z, canvas, pred_ids, seed):
    """Transformer3DModel.denoise, line by line, on a canvas of N rows. Returns the final rows [B, N, P]."""
    pe = m.patch_embed
    gen = torch.Generator().manual_seed(seed)
    x, ids = to_image(canvas), pred_ids
    scheduler._step_index = None
    with torch.no_grad():
        for t in scheduler.timesteps:
            z, ids = scaler.maybe_disable(t, z, ids)
            timestep = torch.as_tensor(t).expand(z.shape[0])
            pred = m(scaler.expand(x), timestep, z, ids)
            pred = pe.unpatchify(scaler.scale(pred))
            x = scheduler.step(pred, t, x, generator=gen).prev_sample
    return pe.patchify(x)


def scheduler_for(kind):
    if kind == "euler":
        s = FlowMatchEulerDiscreteScheduler()
    else:
        s = DDPMScheduler(prediction_type=kind)
        # its tables are float32 tensors; as float64 (same values) every coefficient of its step is a float64 expression
        # of them, which is what engine.sampler_plan computes from float(alphas_cumprod[t])
        s.alphas_cumprod, s.one = s.alphas_cumprod.double(), s.one.double()
    coefs = engine.sampler_plan(s, STEPS)[1]
    return s, coefs


def ddpm_noise(scheduler, seed):
    """The gaussians scheduler.step will draw from a generator with this seed: one [B, P, N, 1] float64 draw per step with t > 0."""
    gen = torch.Generator().manual_seed(seed)
    out = []
    for t in scheduler.timesteps:
        out.append(to_rows(torch.randn(B, P, N, 1, generator=gen, dtype=F64)) if t > 0 else torch.zeros(B, N, P, dtype=F64))
    return torch.stack(out)


def take(t, ids):
    """Rows `ids` [Bx, k] of t [Bx, N, F] or [steps, Bx, N, F]."""
    if t.dim() == 4:
        return torch.stack([take(s, ids) for s in t])
    return t.gather(1, ids.unsqueeze(-1).expand(-1, -1, t.shape[-1]))


def run_case(kind, guidance, *, trunc=False, renorm=1.0, image=0.0, spatiotemporal=0.0, seed=0):
    m, w = build_module(seed)
    scheduler, coefs = scheduler_for(kind)
    ts = [float(t) for t in scheduler.timesteps]
    g_trunc = (ts[1] + ts[2]) / 2 if trunc else 0
    scaler = GuidanceScaler(guidance_scale=guidance, guidance_trunc=g_trunc, guidance_renorm=renorm, image_guidance_scale=image,
                            spatiotemporal_guidance_scale=spatiotemporal)
    passes = scaler.num_passes
    g = torch.Generator().manual_seed(100 + seed)
    z = torch.randn(passes * B, N, D, generator=g, dtype=F64)
    canvas = torch.randn(B, N, P, generator=g, dtype=F64)
    order = torch.stack([torch.randperm(N, generator=g) for _ in range(B)])
    pred_ids = order[:, :n].sort(1).values
    rest_ids = order[:, n:].sort(1).values
    noise_all = ddpm_noise(scheduler, 7) if kind != "euler" else None
    full = full_canvas(m, scheduler, scaler.clone(), z, canvas, pred_ids.repeat(passes, 1).unsqueeze(-1), 7)

    tce = m.time_cond_embed
    with torch.no_grad():
        zc = tce.condition_proj(take(z, pred_ids.repeat(passes, 1))).reshape(passes * B * n, D)
        temb = torch.stack([tce.timestep_proj(tce.get_freq_embed(torch.as_tensor(t).view(1), F64))[0] for t in scheduler.timesteps])
    gs = [1.0 if (trunc and t < g_trunc) else guidance for t in ts]
    kind_x, scale_x = (1, image) if image else ((2, spatiotemporal) if spatiotemporal else (0, 0.0))
    plan = R.make_plan(coefs, gs, scale_x, kind_x, exact=True)
    x = take(canvas, pred_ids)
    echo = take(canvas, rest_ids)
    nz = None if noise_all is None else take(noise_all, pred_ids)
    enz = None if noise_all is None else take(noise_all, rest_ids)
    kw = dict(B=B, n=n, P=P, D=D)
    by_rows = R.denoise_ref(w, zc, temb, x, plan, nz, renorm, None, echo, enz, **kw)
    want_x, want_echo = take(full, pred_ids), take(full, rest_ids)
    return dict(by_rows=by_rows, want_x=want_x, want_echo=want_echo, args=(w, zc, temb, x, plan, nz), echo=echo, kw=kw, renorm=renorm)


def check_rows(c):
    assert rel(c["by_rows"].x, c["want_x"]) < TOL
    if c["renorm"] < 1:
        assert rel(c["by_rows"].echo_rows, c["want_echo"]) < TOL


def test_euler_two_pass():
    c = run_case("euler", 4.0)
    check_rows(c)
    assert torch.isnan(c["by_rows"].ratio).all()  # no renorm: no ratio reported


def test_euler_trunc_renorm_scalar_energy_stands_in_for_the_echo_rows():
    c = run_case("euler", 4.0, trunc=True, renorm=0.3)
    check_rows(c)
    ratio = c["by_rows"].ratio
    assert torch.isfinite(ratio[:2]).all() and torch.isnan(ratio[2:]).all()  # the last two steps run without guidance
    w, zc, temb, x, plan, nz = c["args"]
    by_energy = R.denoise_ref(w, zc, temb, x, plan, nz, 0.3, c["echo"].pow(2).sum((1, 2)), **c["kw"])
    assert rel(by_energy.x, c["want_x"]) < TOL
    assert rel(by_energy.echo_energy, c["want_echo"].pow(2).sum((1, 2))) < TOL
    assert torch.equal(torch.isnan(by_energy.ratio), torch.isnan(ratio)) and rel(by_energy.ratio[:2], ratio[:2]) < TOL


@pytest.mark.parametrize("which", ["image", "spatiotemporal"])
@pytest.mark.parametrize("renorm", [1.0, 0.3])
def test_three_pass_guidance(which, renorm):
    c = run_case("euler", 3.0, trunc=True, renorm=renorm, **{which: 1.5})
    check_rows(c)
    if renorm < 1:
        w, zc, temb, x, plan, nz = c["args"]
        by_energy = R.denoise_ref(w, zc, temb, x, plan, nz, renorm, c["echo"].pow(2).sum((1, 2)), **c["kw"])
        assert rel(by_energy.x, c["want_x"]) < TOL


@pytest.mark.parametrize("kind", ["epsilon", "v_prediction", "sample"])
@pytest.mark.parametrize("renorm", [1.0, 0.3])
def test_ddpm_with_injected_noise(kind, renorm):
    c = run_case(kind, 4.0, renorm=renorm)
    check_rows(c)
    if renorm >= 1:  # without renorm the predicted rows do not depend on the others: nova_decoder_denoise's form
        w, zc, temb, x, plan, nz = c["args"]
        assert rel(R.denoise_ref(w, zc, temb, x, plan, nz, 1.0, **c["kw"]).x, c["want_x"]) < TOL


# ---------------------------------------------------------------------------------------------
# hand cases
# ---------------------------------------------------------------------------------------------
def hand_decoder():
    """D = 8, one block, the AdaLN projection all zero: scale = shift = gate = 0, so the block returns its input and the
    final layer is a plain LayerNorm. patch embed: u = (x0, -x0, x1, -x1, 0, 0, 0, 0); head: v = (LN(u)[0], LN(u)[2])."""
    Dh, Ph = 8, 2
    z = lambda *s: torch.zeros(*s, dtype=F64)
    pw, hw = z(Dh, Ph), z(Ph, Dh)
    pw[0, 0], pw[1, 0], pw[2, 1], pw[3, 1] = 1, -1, 1, -1
    hw[0, 0], hw[1, 2] = 1, 1
    blk = {"fc1_w": torch.eye(Dh, dtype=F64), "fc1_b": z(Dh), "fc2_w": torch.eye(Dh, dtype=F64), "fc2_b": z(Dh),
           "norm2_w": torch.ones(Dh, dtype=F64), "norm2_b": z(Dh)}
    return {"adaln_w": z(5 * Dh, Dh), "adaln_b": z(5 * Dh), "patch_w": pw, "patch_b": z(Dh), "head_w": hw, "head_b": z(Ph), "blocks": [blk]}


@pytest.mark.parametrize("clip,x0_want", [(4.5, (3.9, 4.5)), (10.0, (3.9, 5.2)), (0.0, (3.9, 5.2))])
def test_hand_case_one_row(clip, x0_want):
    """x = (3, 4): u = (3, -3, 4, -4, 0, 0, 0, 0), mean 0, variance 50 / 8 = 6.25, so LN(u) = u / 2.5 up to eps and
    v = (1.2, 1.6) r with r = 2.5 / sqrt(6.25 + 1e-6). kx = 0.5, kv = 2: x0 = (1.5 + 2.4 r, 2 + 3.2 r) ~ (3.9, 5.2); a clip of 4.5
    clamps the second value only, a clip of 10 neither. c0 = 0.25, cx = 0.5, sigma = 0.1, noise (1, -2):
    x <- 0.25 x0 + (1.5, 2) + (0.1, -0.2)."""
    r = 2.5 / math.sqrt(6.25 + 1e-6)
    x0 = [1.5 + 2.4 * r, 2.0 + 3.2 * r]
    assert abs(x0[0] - x0_want[0]) < 1e-5 and abs(min(x0[1], clip or 99) - x0_want[1]) < 1e-5  # the docstring's round figures
    if clip > 0:
        x0 = [min(max(v, -clip), clip) for v in x0]
    want = torch.tensor([[[0.25 * x0[0] + 1.5 + 0.1, 0.25 * x0[1] + 2.0 - 0.2]]], dtype=F64)
    plan = [R.step(1.0, 0.5, 2.0, clip, 0.25, 0.5, 0.1, exact=True)]
    res = R.denoise_ref(hand_decoder(), torch.zeros(1, 8, dtype=F64), torch.zeros(1, 8, dtype=F64), torch.tensor([[[3.0, 4.0]]], dtype=F64),
                        plan, torch.tensor([[[[1.0, -2.0]]]], dtype=F64), 1.0, B=1, n=1, P=2, D=8)
    assert rel(res.x, want) < TOL
    assert res.clipped == ((1, 2) if clip == 4.5 else ((0, 2) if clip else (0, 0)))


def test_hand_case_no_echo_rows():
    """Ne = 0: the norms run over the predicted rows alone. Same decoder; cond and uncond rows are the same network on the
    same x, so c = u = v-hat = (1.2, 1.6) r for any guidance and the unclamped ratio is exactly 1; with an echo energy E the
    ratio stays 1 and E takes (1 + dt)^2. An empty echo-row tensor and a zero energy give the same x."""
    r = 2.5 / math.sqrt(6.25 + 1e-6)
    plan = [R.step(4.0, c0=-0.25, exact=True)]
    args = (hand_decoder(), torch.zeros(2, 8, dtype=F64), torch.zeros(1, 8, dtype=F64), torch.tensor([[[3.0, 4.0]]], dtype=F64), plan, None, 0.3)
    kw = dict(B=1, n=1, P=2, D=8)
    rows = R.denoise_ref(*args, None, torch.zeros(1, 0, 2, dtype=F64), None, **kw)
    energy = R.denoise_ref(*args, torch.tensor([2.0], dtype=F64), **kw)
    want = torch.tensor([[[3.0 - 0.25 * 1.2 * r, 4.0 - 0.25 * 1.6 * r]]], dtype=F64)
    assert rel(rows.x, want) < TOL and rel(energy.x, want) < TOL
    assert abs(rows.ratio.item() - 1.0) < TOL and rows.echo_rows.shape == (1, 0, 2)
    assert abs(energy.echo_energy.item() - 2.0 * 0.75 ** 2) < TOL


def test_ratio_is_reported_before_clamping():
    """With no echo rows and a large guidance the factor falls below the floor: the reported value is the raw one, the
    applied one the floor (x moves by floor * v-hat)."""
    w = R.make_weights(16, 1, 3, seed=5)
    inp = R.make_inputs(2, 4, 3, 16, 2, 1, seed=6)
    plan = [R.step(9.0, c0=-0.5)]
    res = R.denoise_ref(w, inp["zc"], inp["temb"], inp["x"], plan, None, 0.9, torch.zeros(2), B=2, n=4, P=3, D=16)
    assert (res.ratio < 0.9).all() and (res.ratio > 0).all()
    free = R.denoise_ref(w, inp["zc"], inp["temb"], inp["x"], plan, None, 1.0, B=2, n=4, P=3, D=16)
    assert rel(res.x - inp["x"].double(), 0.9 * (free.x - inp["x"].double())) < 1e-12
