"""Training kernels of libnova_hip.so against torch autograd (GPU box only).

Attention backward (csrc/attn_bwd.hip): forward output and dq / dk / dv of `nova_pointcloud_amd.autograd.attention` against
F.scaled_dot_product_attention differentiated in float32 on the same bf16-valued inputs. Tolerance: P and dS pass
through bf16 on their way into the MFMAs (2^-8 relative per element), gradients are sums of such terms - 2e-2 of the
tensor's largest magnitude.
"""
import os
import sys

import pytest
import torch

pytestmark = pytest.mark.gpu
PKG = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "nova_pointcloud_amd")
if PKG not in sys.path:
    sys.path.insert(0, PKG)  # the drop-in `diffnext` package


def _ref(q, k, v, d_out):
    qf, kf, vf = (t.detach().float().requires_grad_(True) for t in (q, k, v))
    out = torch.nn.functional.scaled_dot_product_attention(qf, kf, vf)
    out.backward(d_out.float())
    return out.detach(), qf.grad, kf.grad, vf.grad


def _rel(got, ref):
    return ((got.float() - ref).abs().max() / ref.abs().max().clamp_min(1e-12)).item()


@pytest.mark.parametrize("S,h,L", [(1, 1, 64), (2, 3, 128), (1, 2, 200), (2, 1, 333), (1, 4, 1031), (3, 2, 31)])
@pytest.mark.parametrize("spread", [1.0, 4.0])
@pytest.mark.parametrize("hd", [64, 96])
def test_attention_forward_backward_match_autograd(hip, S, h, L, spread, hd):
    from nova_pointcloud_amd import autograd as A

    g = torch.Generator().manual_seed(S * 1000 + h * 100 + L + hd)
    mk = lambda s: (torch.randn(S, h, L, hd, generator=g) * s).bfloat16().cuda()
    q, k, v, d_out = mk(spread), mk(1.0), mk(1.0), mk(1.0)  # spread > 1: peaked rows (large score range)
    q, k, v = (t.requires_grad_(True) for t in (q, k, v))
    assert A.attention_supported(q)
    out = A.attention(q, k, v)
    out.backward(d_out)
    o_ref, dq_ref, dk_ref, dv_ref = _ref(q, k, v, d_out)
    assert out.shape == (S, h, L, hd) and q.grad.shape == q.shape
    assert _rel(out, o_ref) < 1.6e-2
    for name, got, ref in (("dq", q.grad, dq_ref), ("dk", k.grad, dk_ref), ("dv", v.grad, dv_ref)):
        assert torch.isfinite(got.float()).all(), name
        assert _rel(got, ref) < 2e-2, (name, _rel(got, ref))


def test_attention_module_trains_through_hip_kernels(hip):
    """`Attention.forward` with autograd on (the training forward) takes the HIP attention for bf16 / head_dim 64 and its
    parameter gradients match the PyTorch definition of the same module."""
    from diffnext.models.vision_transformer import Attention
    from nova_pointcloud_amd import autograd as A

    torch.manual_seed(5)
    attn = Attention(256, 4).cuda().bfloat16()
    x = (torch.randn(2, 150, 256) * 0.7).bfloat16().cuda()
    before = A.stats["attention_calls"]
    xa = x.clone().requires_grad_(True)
    attn(xa).float().square().mean().backward()
    calls = A.stats["attention_calls"] - before
    assert calls, "training forward did not reach the HIP attention"
    got = {n: p.grad.float().clone() for n, p in attn.named_parameters()}
    gx = xa.grad.float().clone()
    attn.zero_grad()
    ref_mod = Attention(256, 4).cuda().float()
    ref_mod.load_state_dict({k_: v_.float() for k_, v_ in attn.state_dict().items()})
    xb = x.float().requires_grad_(True)
    ref_mod(xb).square().mean().backward()
    assert _rel(gx, xb.grad) < 3e-2
    for n, p in ref_mod.named_parameters():
        assert _rel(got[n], p.grad) < 3e-2, n


def test_bf16_training_step_with_hip_attention_matches_torch_attention(hip):
    """One `train_video` step (transformer_3d.py:79-100) of the golden model in bf16 on the GPU, all draws injected: with
    the HIP attention forward + backward inside every ViT block against the same step on torch's SDPA. Loss and every
    parameter gradient agree to bf16 accuracy (both paths round activations to bf16; they differ in where)."""
    import numpy as np

    from diffnext.schedulers import FlowMatchEulerDiscreteScheduler
    from golden_util import Golden
    from nova_pointcloud_amd import autograd as A
    from test_mirror_cpu import build_from_golden

    gold = Golden("tiny_rope")

    def step(use_hip_attention):
        model = build_from_golden(gold, torch.bfloat16, "cuda")
        model.noise_scheduler = FlowMatchEulerDiscreteScheduler()
        model.train()
        g = torch.Generator().manual_seed(5)
        real_rand, real_randn, real_normal = torch.rand, torch.randn, torch.normal
        torch.rand = lambda *a, **k: real_rand(*a, generator=g).to(k.get("device", "cpu"))
        torch.randn = lambda *a, **k: real_randn(*a, generator=g).to(device=k.get("device", "cpu"), dtype=k.get("dtype", None))
        torch.normal = lambda m_, s_, size, **k: real_normal(m_, s_, size, generator=g).to(k.get("device", "cpu"))
        np.random.seed(11)
        keep, before = A._ENABLED, A.stats["attention_calls"]
        A._ENABLED = use_hip_attention
        try:
            out = model({"x": gold.t["train/x"].clone().cuda().bfloat16(), "prompt": [p.clone().cuda().bfloat16() for p in gold.prompt_embeds]})
            out["loss"].backward()
        finally:
            torch.rand, torch.randn, torch.normal = real_rand, real_randn, real_normal
            A._ENABLED = keep
        calls = A.stats["attention_calls"] - before
        grads = {k: v.grad.detach().float() for k, v in model.named_parameters() if v.grad is not None}
        return float(out["loss"].detach()), grads, calls

    loss_hip, g_hip, n_hip = step(True)
    loss_pt, g_pt, n_pt = step(False)
    assert n_hip > 0 and n_pt == 0
    assert abs(loss_hip - loss_pt) <= 2e-2 * abs(loss_pt)
    assert g_hip.keys() == g_pt.keys() and len(g_hip) > 20
    worst = 0.0
    for name, ref in g_pt.items():
        got = g_hip[name]
        assert torch.isfinite(got).all(), name
        if float(ref.abs().max()) == 0.0:  # not on the T = 1 path (frame patch embedding): zero on both
            assert float(got.abs().max()) == 0.0, name
            continue
        cos = torch.nn.functional.cosine_similarity(got.flatten(), ref.flatten(), dim=0).item()
        assert cos > 0.98, (name, cos)
        worst = max(worst, 1 - cos)
    print(f"\n[train-attn] loss hip {loss_hip:.5f} torch {loss_pt:.5f}; worst 1 - cos over {len(g_pt)} gradients {worst:.2e}")


def test_f32_training_step_with_hip_norms_and_activations_matches_the_torch_composition(hip):
    """One `train_video` step (transformer_3d.py:79-100) of the golden model in f32 on the GPU, all draws injected: the LayerNorm family
    and the GELU / SiLU activations on the HIP kernels (forward + backward) against the same step on their torch composition (the attention
    is torch's in both: the HIP attention is a bf16 kernel). Everything is f32, so the two steps agree closely: loss to 1e-5 relative,
    every parameter gradient to 2e-4 of its largest entry."""
    import numpy as np

    from diffnext.schedulers import FlowMatchEulerDiscreteScheduler
    from golden_util import Golden
    from nova_pointcloud_amd import autograd as A
    from test_mirror_cpu import build_from_golden

    gold = Golden("tiny_rope")

    def step(use_hip):
        model = build_from_golden(gold, torch.float32, "cuda")
        model.noise_scheduler = FlowMatchEulerDiscreteScheduler()
        model.train()
        g = torch.Generator().manual_seed(5)
        real_rand, real_randn, real_normal = torch.rand, torch.randn, torch.normal
        torch.rand = lambda *a, **k: real_rand(*a, generator=g).to(k.get("device", "cpu"))
        torch.randn = lambda *a, **k: real_randn(*a, generator=g).to(device=k.get("device", "cpu"), dtype=k.get("dtype", None))
        torch.normal = lambda m_, s_, size, **k: real_normal(m_, s_, size, generator=g).to(k.get("device", "cpu"))
        np.random.seed(11)
        keep = (A._NORM_ENABLED, A._ACT_ENABLED)
        before = (A.stats["norm_calls"], A.stats["act_calls"])
        A._NORM_ENABLED = A._ACT_ENABLED = use_hip
        try:
            out = model({"x": gold.t["train/x"].clone().cuda(), "prompt": [p.clone().cuda() for p in gold.prompt_embeds]})
            out["loss"].backward()
        finally:
            torch.rand, torch.randn, torch.normal = real_rand, real_randn, real_normal
            A._NORM_ENABLED, A._ACT_ENABLED = keep
        calls = (A.stats["norm_calls"] - before[0], A.stats["act_calls"] - before[1])
        grads = {k: v.grad.detach().clone() for k, v in model.named_parameters() if v.grad is not None}
        return float(out["loss"].detach()), grads, calls

    loss_hip, g_hip, n_hip = step(True)
    loss_pt, g_pt, n_pt = step(False)
    assert n_hip[0] > 0 and n_hip[1] > 0 and n_pt == (0, 0), (n_hip, n_pt)
    assert abs(loss_hip - loss_pt) <= 1e-5 * abs(loss_pt), (loss_hip, loss_pt)
    assert g_hip.keys() == g_pt.keys() and len(g_hip) > 20
    worst = 0.0
    for name, ref in g_pt.items():
        got = g_hip[name]
        assert torch.isfinite(got).all(), name
        scale = float(ref.abs().max())
        if scale == 0.0:
            assert float(got.abs().max()) == 0.0, name
            continue
        err = float((got - ref).abs().max()) / scale
        assert err < 2e-4, (name, err)
        worst = max(worst, err)
    print(f"\n[train-f32] loss hip {loss_hip:.7f} torch {loss_pt:.7f}; worst relative gradient error over {len(g_pt)} tensors {worst:.2e}; "
          f"HIP norm / activation calls {n_hip}")


def test_train_script_one_rank_under_torchrun_bf16_on_rccl(hip, tmp_path):
    """`scripts/train.py` as the reference launches it - one process per GPU under torchrun - on this box's one GPU:
    NOVA-d48w768 random-init (the config's architecture), bf16, 64-point synthetic samples, 3 steps. The process group is
    RCCL ("nccl"), so the weight broadcast, the bucketed gradient all_reduce and the loss all_reduce run on the device;
    the ViT blocks take the HIP attention forward + backward (bf16, head_dim 64). Checks the loss log and the checkpoint."""
    import json
    import subprocess

    root = os.path.dirname(PKG)
    env = dict(os.environ, PYTHONPATH=os.pathsep.join([PKG, root, os.environ.get("PYTHONPATH", "")]), HSA_ENABLE_IPC_MODE_LEGACY="0",
               NOVA_TRAIN_LOG_JSON=str(tmp_path / "history.json"))
    cmd = [sys.executable, "-m", "torch.distributed.run", "--standalone", "--nnodes=1", "--nproc-per-node=1", "--local-addr", "127.0.0.1",
           os.path.join(root, "scripts", "train.py"), "--config", os.path.join(root, "configs", "train_pointcloud_tiny.yaml"),
           f"experiment.output_dir={tmp_path}", "training.max_train_steps=3", "training.mixed_precision=bf16", "train_dataloader.batch_size=4"]
    out = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=900)
    assert out.returncode == 0, out.stderr[-3000:]
    history = json.load(open(tmp_path / "history.json"))
    assert history["world"] == 1 and history["backend"] == "nccl" and history["dtype"] == "torch.bfloat16"
    assert len(history["loss"]) == 3 and all(0 < v < 10 for v in history["loss"])
    assert history["hip_attention_calls"] > 0
    assert os.path.isdir(os.path.join(str(tmp_path), "checkpoints", "checkpoint-3", "transformer"))


def test_bench_launch_contract_one_rank_on_rccl(hip):
    """The driver's N > 1 launch line (`python -m torch.distributed.run --nnodes=1 --nproc-per-node N --master-addr
    127.0.0.1 --master-port P bench.py --gpus N ...`) with N = 1 on this box's GPU: RCCL process group, barrier-bracketed
    timing, all_gather of the generated point sets, max-over-ranks time, ONE JSON line from rank 0 (reduced AR / diffusion
    step counts; the contract, not the number, is under test). `--full`: the roofline of the serialised kernel pass is checked too."""
    import json
    import subprocess

    root = os.path.dirname(PKG)
    env = dict(os.environ, HSA_ENABLE_IPC_MODE_LEGACY="0")
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "1", "--master-addr", "127.0.0.1",
           "--master-port", "29641", os.path.join(root, "bench.py"), "--gpus", "1", "--steps", "1", "--warmup", "1",
           "--workload", "d48w768_1024pts_b8", "--ar-steps", "6", "--diffusion-steps", "3", "--full", "--no-cpu-baseline"]
    out = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=900, cwd=root)
    assert out.returncode == 0, out.stderr[-3000:]
    lines = [l for l in out.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1
    rec = json.loads(lines[0])
    assert rec["n_gpus"] == 1 and rec["steps"] == 1 and rec["value"] > 0 and rec["scaling"] == "weak"
    assert rec["config"]["global_batch"] == 8 and "roofline" in rec


# ---------------------------------------------------------------------------------------------------------------------
# LayerNorm family backward (csrc/rownorm_bwd.hip) behind autograd.fused_norm, against PyTorch autograd in float32
# ---------------------------------------------------------------------------------------------------------------------
def _norm_ref(x, gamma, beta, scale, shift, gate, res, eps):
    """The composition the modules spell out (vision_transformer.py:78-82, normalization.py:34-36, diffusion_mlp.py:52-53)."""
    y = torch.nn.functional.layer_norm(x, (x.shape[-1],), gamma, beta, eps)
    if scale is not None:
        y = y * (1 + scale) + shift
    if gate is not None:
        y = y * gate
    return y + res if res is not None else y


NORM_KINDS = {  # which terms are present: the three uses in the model + the bare and the full combination
    "vit_post_norm": dict(affine=True, ss=False, gate=False, res=True),
    "adaln_modulate": dict(affine=False, ss=True, gate=False, res=False),
    "gated_norm": dict(affine=True, ss=False, gate=True, res=True),
    "plain": dict(affine=False, ss=False, gate=False, res=False),
    "everything": dict(affine=True, ss=True, gate=True, res=True),
}


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16, torch.float16])
@pytest.mark.parametrize("kind", sorted(NORM_KINDS))
@pytest.mark.parametrize("shape", [(3, 37, 128), (2, 300, 768), (5000, 1024), (1, 7, 1536)])
def test_fused_norm_forward_backward_match_autograd(hip, dtype, kind, shape):
    from nova_pointcloud_amd import autograd as A

    k = NORM_KINDS[kind]
    D = shape[-1]
    g = torch.Generator().manual_seed(D + len(shape))
    r = lambda *s, sc=1.0: (torch.randn(*s, generator=g) * sc).to(dtype).cuda()
    x, dy = r(*shape), r(*shape)
    gamma = (1 + r(D, sc=0.2)).float() if k["affine"] else None
    beta = r(D, sc=0.2).float() if k["affine"] else None
    n_mod = (2 if k["ss"] else 0) + (1 if k["gate"] else 0)
    mod = r(*shape[:-1], max(n_mod, 1) * D, sc=0.5)  # what `proj(SiLU(z))` yields; the terms are chunk views of it
    res = r(*shape) if k["res"] else None
    leaves = [t for t in (x, gamma, beta, mod if n_mod else None, res) if t is not None]
    for t in leaves:
        t.requires_grad_(True)
    chunks = list(mod.chunk(max(n_mod, 1), dim=-1))
    scale, shift = (chunks[0], chunks[1]) if k["ss"] else (None, None)
    gate = chunks[-1] if k["gate"] else None
    assert A.fused_norm_supported(x, gamma=gamma, scale=scale, shift=shift, gate=gate, res=res)
    eps = 1e-6 if kind == "adaln_modulate" else 1e-5
    out = A.fused_norm(x, gamma, beta, scale, shift, gate, res, eps)
    out.backward(dy)
    got = [t.grad.clone() for t in leaves]
    # reference: the same values in float32 through PyTorch's own autograd
    ref_leaves = [t.detach().float().requires_grad_(True) for t in leaves]
    it = iter(ref_leaves)
    xr = next(it)
    gr, br = (next(it), next(it)) if k["affine"] else (None, None)
    modr = next(it) if n_mod else mod.detach().float()
    rc = list(modr.chunk(max(n_mod, 1), dim=-1))
    ref = _norm_ref(xr, gr, br, rc[0] if k["ss"] else None, rc[1] if k["ss"] else None, rc[-1] if k["gate"] else None,
                    next(it) if k["res"] else None, eps)
    ref.backward(dy.float())
    tol = {torch.float32: 2e-5, torch.bfloat16: 1.6e-2, torch.float16: 2e-3}[dtype]
    assert out.shape == x.shape and out.dtype == dtype and _rel(out, ref.detach()) < tol
    names = ["x"] + (["gamma", "beta"] if k["affine"] else []) + (["mod"] if n_mod else []) + (["res"] if k["res"] else [])
    for name, gt, rl in zip(names, got, ref_leaves):
        assert torch.isfinite(gt.float()).all(), name
        # parameter gradients are sums over all rows of 16-bit-rounded terms: a few ulps of the storage type at the sum's scale
        assert _rel(gt, rl.grad) < (4 * tol if name in ("gamma", "beta") else 2 * tol), (name, _rel(gt, rl.grad))


def test_training_modules_take_the_fused_norm_and_match_the_torch_definition(hip):
    """Block (post-norm residual x2), AdaLayerNormZero and DiffusionBlock with autograd on, on the GPU: the fused HIP norm is
    what runs (call counter), and outputs + every parameter gradient match the same modules with it switched off."""
    from diffnext.models.diffusion_mlp import DiffusionBlock
    from diffnext.models.vision_transformer import Block
    from nova_pointcloud_amd import autograd as A

    torch.manual_seed(9)
    for make, args in ((lambda: Block(256, 4), lambda: (torch.randn(2, 70, 256) * 0.7,)),
                       (lambda: DiffusionBlock(256), lambda: (torch.randn(2, 70, 256) * 0.7, torch.randn(2, 70, 256) * 0.7))):
        mod = make().cuda().float()
        with torch.no_grad():
            for p in mod.parameters():
                p.add_(torch.randn_like(p) * 0.02)
        ins = [t.cuda().requires_grad_(True) for t in args()]
        before = A.stats["norm_calls"]
        out = mod(*ins)
        out.square().mean().backward()
        assert A.stats["norm_calls"] > before
        grads = {n: p.grad.clone() for n, p in mod.named_parameters()}
        gin = [t.grad.clone() for t in ins]
        mod.zero_grad()
        for t in ins:
            t.grad = None
        A._NORM_ENABLED = False
        try:
            ref = mod(*ins)
            ref.square().mean().backward()
        finally:
            A._NORM_ENABLED = True
        assert _rel(out.detach(), ref.detach()) < 1e-4
        for t, gi in zip(ins, gin):
            assert _rel(gi, t.grad) < 1e-3
        for n, p in mod.named_parameters():
            assert _rel(grads[n], p.grad) < 1e-3, n


@pytest.mark.parametrize("amp", [torch.float16, torch.bfloat16])
def test_block_under_autocast_with_f32_parameters_matches_the_torch_composition(hip, amp):
    """The reference trainer runs the model under torch.cuda.amp.autocast() with f32 parameters (train_newloss.py:1049): inside a
    Block the branch output (a Linear under autocast) is 16-bit while the residual stream (LayerNorm outputs, f32 input) stays f32.
    The fused norm + residual kernel takes ONE storage type, so that pair must go the torch way - not read the f32 residual as
    halves (round-3 defect: the support check compared x with itself). Same loss and gradients as with the fused norms disabled,
    and the autograd function itself refuses mismatched operand types."""
    from diffnext.models.vision_transformer import Block
    from nova_pointcloud_amd import autograd as A

    torch.manual_seed(13)
    mod = Block(256, 4).cuda().float()
    x = (torch.randn(2, 70, 256) * 0.7).cuda().requires_grad_(True)

    def step():
        mod.zero_grad()
        x.grad = None
        with torch.autocast("cuda", dtype=amp):
            out = mod(x)
        out.float().square().mean().backward()
        return out.detach().float(), x.grad.clone(), {n: p.grad.clone() for n, p in mod.named_parameters()}

    out, gx, gp = step()
    A._NORM_ENABLED = False
    try:
        ref, rgx, rgp = step()
    finally:
        A._NORM_ENABLED = True
    assert out.dtype == ref.dtype and torch.isfinite(out).all()
    assert _rel(out, ref) < 1e-5 and _rel(gx, rgx) < 1e-4
    for n in gp:
        assert _rel(gp[n], rgp[n]) < 1e-4, n
    y16, res32 = torch.randn(8, 256, device="cuda", dtype=amp), torch.randn(8, 256, device="cuda")
    assert not A.fused_norm_supported(y16, gamma=mod.norm1.weight, res=res32)
    with pytest.raises(TypeError):
        A.fused_norm(y16, gamma=mod.norm1.weight, beta=mod.norm1.bias, res=res32)


# ---------------------------------------------------------------------------------------------------------------------
# Pointwise activations of the MLPs, forward and backward (csrc/rownorm_bwd.hip act_kernel; reference vision_transformer.py:35,38
# nn.GELU(), diffusion_mlp.py:33,36 and normalization.py:32,35 nn.SiLU())
# ---------------------------------------------------------------------------------------------------------------------
# elementwise bound |got - ref| <= rtol |ref| + atol against PyTorch's f32 result on the same (storage-rounded) inputs:
# f32: a few ulp of erff / expf; 16-bit: half an ulp of the storage type (2^-9 bf16, 2^-12 f16) on the rounded result, doubled
ACT_TOL = {torch.float32: (2e-6, 2e-6), torch.bfloat16: (2 ** -8, 1e-6), torch.float16: (2 ** -11, 1e-6)}


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16, torch.float16])
@pytest.mark.parametrize("kind", ["gelu", "silu"])
@pytest.mark.parametrize("shape", [(8,), (3, 37, 128), (2, 300, 3072), (5000, 1024)])
def test_activation_forward_backward_match_autograd(hip, dtype, kind, shape):
    from nova_pointcloud_amd import autograd as A

    g = torch.Generator().manual_seed(100 * len(shape) + shape[-1] % 97 + (0 if kind == "gelu" else 7))
    x = torch.randn(*shape, generator=g) * 2.5
    flat = x.view(-1)
    flat[:8] = torch.tensor([0.0, -0.0, 8.0, -8.0, 30.0, -30.0, -0.7518, 1e-4])[: flat.numel()]  # zeros, both tails, gelu' = 0, tiny
    dy = torch.randn(*shape, generator=g)
    x, dy = x.to(dtype).cuda(), dy.to(dtype).cuda()
    fn = (lambda t: torch.nn.functional.gelu(t)) if kind == "gelu" else torch.nn.functional.silu
    xr = x.detach().float().clone().requires_grad_(True)  # (.float() of an f32 tensor is the tensor itself: clone before requires_grad_)
    ref = fn(xr)
    ref.backward(dy.float())
    assert A.activation_supported(x)
    xa = x.detach().clone().requires_grad_(True)
    y = A.activation(xa, A.ACT_GELU if kind == "gelu" else A.ACT_SILU)
    y.backward(dy)
    assert y.dtype == dtype and xa.grad.dtype == dtype and y.shape == x.shape
    rtol, atol = ACT_TOL[dtype]
    torch.testing.assert_close(y.float(), ref.detach(), rtol=rtol, atol=atol)
    torch.testing.assert_close(xa.grad.float(), xr.grad, rtol=rtol, atol=atol * max(1.0, dy.float().abs().max().item()))


def test_activation_refuses_ragged_sizes_and_unknown_kinds(hip):
    """Whole 16-byte chunks only: the predicate says no (the modules then take the torch op), the C entry point says why."""
    from nova_pointcloud_amd import autograd as A

    x = torch.randn(13, device="cuda", dtype=torch.bfloat16)
    assert not A.activation_supported(x)
    assert not A.activation_supported(torch.randn(16))  # host tensor
    y = torch.empty_like(x)
    with pytest.raises(hip.NovaHipError, match="multiple"):
        hip.call("nova_act_fwd", x.data_ptr(), y.data_ptr(), x.numel(), 1, hip.dtype_code(x.dtype), hip.stream_ptr())
    x16 = torch.randn(16, device="cuda", dtype=torch.bfloat16)
    with pytest.raises(hip.NovaHipError, match="kind"):
        hip.call("nova_act_fwd", x16.data_ptr(), torch.empty_like(x16).data_ptr(), 16, 7, hip.dtype_code(x16.dtype), hip.stream_ptr())


def test_training_modules_take_the_hip_activation_and_match_the_torch_definition(hip):
    """MLP (GELU), the decoder's MLP and AdaLayerNormZero (SiLU) with autograd on, on the GPU: the HIP activation is what runs
    (call counter), outputs and every gradient match the same modules with it switched off; under no_grad it is not taken."""
    from diffnext.models.diffusion_mlp import DiffusionBlock
    from diffnext.models.vision_transformer import Block
    from nova_pointcloud_amd import autograd as A

    torch.manual_seed(11)
    for make, args in ((lambda: Block(256, 4), lambda: (torch.randn(2, 70, 256) * 0.7,)),
                       (lambda: DiffusionBlock(256), lambda: (torch.randn(2, 70, 256) * 0.7, torch.randn(2, 70, 256) * 0.7))):
        mod = make().cuda().float()
        with torch.no_grad():
            for p in mod.parameters():
                p.add_(torch.randn_like(p) * 0.02)
        ins = [t.cuda().requires_grad_(True) for t in args()]
        before = A.stats["act_calls"]
        out = mod(*ins)
        out.square().mean().backward()
        assert A.stats["act_calls"] > before, type(mod).__name__
        grads = {n: p.grad.clone() for n, p in mod.named_parameters()}
        gin = [t.grad.clone() for t in ins]
        mod.zero_grad()
        for t in ins:
            t.grad = None
        A._ACT_ENABLED = False
        try:
            ref = mod(*ins)
            ref.square().mean().backward()
        finally:
            A._ACT_ENABLED = True
        assert _rel(out.detach(), ref.detach()) < 1e-5
        for t, gi in zip(ins, gin):
            assert _rel(gi, t.grad) < 1e-4
        for n, p in mod.named_parameters():
            assert _rel(grads[n], p.grad) < 1e-4, n


# ---------------------------------------------------------------------------------------------------------------------
# Block-causal frame mask of multi-frame training (reference embeddings.py:247-260, transformer_3d.py:176-177) as a per-query key limit
# ---------------------------------------------------------------------------------------------------------------------
def _frame_mask(prefix, frames, per_frame, device="cuda", dtype=torch.bfloat16):
    """What MaskEmbed.get_attn_mask builds: token i sees token j iff frame(i) >= frame(j), the prefix counting as frame 0."""
    d = torch.cat([torch.zeros(prefix), torch.arange(frames).repeat_interleave(per_frame)])
    return torch.where(d[:, None] >= d[None, :], 0.0, float("-inf")).to(device=device, dtype=dtype)


@pytest.mark.parametrize("hd", [64, 96])
@pytest.mark.parametrize("S,h,prefix,frames,per_frame", [(2, 2, 8, 3, 40), (1, 3, 37, 4, 100), (2, 1, 0, 5, 64), (1, 2, 300, 2, 333)])
def test_masked_attention_forward_backward_match_autograd(hip, S, h, prefix, frames, per_frame, hd):
    from nova_pointcloud_amd import autograd as A

    L = prefix + frames * per_frame
    g = torch.Generator().manual_seed(L + hd)
    mk = lambda s: (torch.randn(S, h, L, hd, generator=g) * s).bfloat16().cuda()
    q, k, v, d_out = mk(2.0), mk(1.0), mk(1.0), mk(1.0)
    q, k, v = (t.requires_grad_(True) for t in (q, k, v))
    mask = _frame_mask(prefix, frames, per_frame)
    limit = A.key_limit_of_mask(mask)
    assert limit is not None and limit.dtype == torch.int32 and int(limit[0]) == prefix + per_frame and int(limit[-1]) == L
    assert A.key_limit_of_mask(mask) is limit  # cached per mask tensor
    assert A.attention_supported(q, mask)
    out = A.attention(q, k, v, mask)
    out.backward(d_out)
    qf, kf, vf = (t.detach().float().requires_grad_(True) for t in (q, k, v))
    ref = torch.nn.functional.scaled_dot_product_attention(qf, kf, vf, attn_mask=mask.float())
    ref.backward(d_out.float())
    assert _rel(out, ref.detach()) < 1.6e-2
    for name, got, want in (("dq", q.grad, qf.grad), ("dk", k.grad, kf.grad), ("dv", v.grad, vf.grad)):
        assert torch.isfinite(got.float()).all(), name
        assert _rel(got, want) < 2e-2, (name, _rel(got, want))
    # rows of the first frame must not depend on later frames at all: perturbing the last frame's keys / values leaves them bit-identical
    with torch.no_grad():
        k2, v2 = k.detach().clone(), v.detach().clone()
        k2[:, :, -per_frame:] += 1.0
        v2[:, :, -per_frame:] -= 1.0
        again = A.attention(q.detach(), k2, v2, mask)
    first = prefix + per_frame
    assert torch.equal(again[:, :, :first], out.detach()[:, :, :first])


def test_masks_that_are_not_key_limits_are_refused(hip):
    from nova_pointcloud_amd import autograd as A

    L = 64
    q = torch.zeros(1, 1, L, 64, dtype=torch.bfloat16, device="cuda")
    band = torch.full((L, L), float("-inf"), device="cuda").triu(5).tril(-1) * 0  # zeros: everything visible -> a valid (trivial) limit
    assert A.attention_supported(q, band.bfloat16())
    anti = torch.where(torch.arange(L)[:, None] <= torch.arange(L)[None, :], 0.0, float("-inf")).cuda()  # sees only LATER keys: no prefix form
    assert A.key_limit_of_mask(anti) is None and not A.attention_supported(q, anti)
    bias = torch.randn(L, L, device="cuda")  # finite biases are not a visibility mask
    assert not A.attention_supported(q, bias)
