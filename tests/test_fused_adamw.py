"""The fused AdamW step with in-kernel gradient clipping (nova_pointcloud_amd/optim.py on csrc/adamw.hip).

CPU: restate(), the definition of include/nova_hip.h at nova_adamw_step in numpy float32 (the step, and the sum of squares in
its stated chunk and merge order), is pinned to torch.optim.AdamW and clip_grad_norm_ before any kernel is involved; then
every ValueError of the constructor and of step, the state_dict format, the header's constants, the Trainer's wiring and the
argument checks of the two entry points (validation-only calls: nothing is launched).
GPU: the kernels are held BITWISE to restate() for the parameter, both moments, the master copy and the sum of squares."""
import copy
import ctypes
import functools
import math
import os
import re
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "nova_pointcloud_amd")
for p in (ROOT, PKG, os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)

from nova_pointcloud_amd import hip as H  # noqa: E402
from nova_pointcloud_amd import optim as M  # noqa: E402
from nova_pointcloud_amd.optim import FusedAdamW  # noqa: E402

HEADER = os.path.join(ROOT, "include", "nova_hip.h")
F = np.float32
CHUNK, COLUMNS, BLOCK = 8192, 256, 32  # as the header states them (test_header_constants compares)
U = 2.0 ** -24  # unit roundoff of float32
HALF = {torch.bfloat16, torch.float16}


# ---- restate(): the header's text in numpy float32 -----------------------------------------------------------------------

def widen(t):
    """A torch tensor of float32 / bfloat16 / float16 as float32 numpy (exact)."""
    return t.detach().cpu().float().numpy().reshape(-1).copy()


def narrow(a, dtype):
    """float32 numpy to a CPU torch tensor of `dtype`, ONE round-to-nearest-even (float32: as it is)."""
    return torch.from_numpy(np.ascontiguousarray(a)).to(dtype)


def tree(a):
    """s[t] = s[t] + s[t + h] for h = 128, 64, .. 1: s[0]"""
    assert a.dtype == np.float32 and a.size == 256
    while a.size > 1:
        h = a.size // 2
        a = a[:h] + a[h:]
    return a[0]


def restate_sumsq(grads):
    """The float32 sum of squares of a list of float32 arrays (already widened) in the header's order."""
    parts = []
    for g in grads:
        for c0 in range(0, g.size, CHUNK):
            x = np.zeros(CHUNK, F)  # an element past n - 1 is not added; adding its +0 to a sum that is >= +0 is the same
            x[:min(CHUNK, g.size - c0)] = g[c0:c0 + CHUNK]
            sq = (x * x).reshape(CHUNK // (256 * 8), 256, 8)  # [unit row j, thread t, element k]: unit u = 256 j + t
            acc = np.zeros(256, F)
            for j in range(sq.shape[0]):
                for k in range(8):
                    acc = acc + sq[j, :, k]
            parts.append(tree(acc))
    if not parts:
        return F(0)
    rows = -(-len(parts) // COLUMNS)
    table = np.zeros(rows * COLUMNS, F)
    table[:len(parts)] = np.array(parts, F)
    cols = np.zeros(COLUMNS, F)
    for row in table.reshape(rows, COLUMNS):
        cols = cols + row
    return tree(cols)


def numbers(lr, betas, eps, wd, t):
    """The seven float32 numbers, each formed in float64 and rounded once."""
    d = np.float64
    lr, b1, b2, eps, wd, t = d(lr), d(betas[0]), d(betas[1]), d(eps), d(wd), d(t)
    return tuple(F(v) for v in (1 - lr * wd, 1 - b1, b2, 1 - b2, np.sqrt(1 - b2 ** t), lr / (1 - b1 ** t), eps))


def clip_coefficient(sumsq, max_norm):
    with np.errstate(all="ignore"):
        c = F(max_norm) / (np.sqrt(F(sumsq)) + F(1e-6))
    return F(1) if c > 1 else c


def restate_step(p0, g, m, v, nums, s=None):
    """(p', m', v') as float32 arrays from float32 arrays; p0 is the master copy or the widened parameter, s the clip
    coefficient or None for "no multiplication"."""
    decay, w1, b2, w2, q, a, eps = nums
    assert all(x.dtype == np.float32 for x in (p0, g, m, v, decay, w1, b2, w2, q, a, eps))
    with np.errstate(all="ignore"):
        if s is not None:
            g = g * F(s)
        p1 = p0 * decay
        m2 = m + w1 * (g - m)
        v2 = v * b2 + w2 * (g * g)
        d = np.sqrt(v2) / q + eps
        p2 = p1 - a * (m2 / d)
    assert p2.dtype == np.float32 and m2.dtype == np.float32 and v2.dtype == np.float32
    return p2, m2, v2


class Restated(object):
    """restate() as an optimizer over CPU copies: tensors [(values, dtype, group index)], groups [dict(lr, betas, eps, wd)]."""

    def __init__(self, values, dtypes, group_of, groups, master_weights=True):
        self.dtypes, self.group_of, self.groups = dtypes, group_of, groups
        self.p = [narrow(widen(x), dt) for x, dt in zip(values, dtypes)]  # the stored parameter
        self.master = [widen(x) if (dt in HALF and master_weights) else None for x, dt in zip(self.p, dtypes)]
        self.m = [np.zeros(x.numel(), F) for x in self.p]
        self.v = [np.zeros(x.numel(), F) for x in self.p]
        self.t = [0] * len(values)
        self.sumsq = None

    def step(self, grads, max_grad_norm=None):
        """grads: a tensor (of the parameter's dtype) or None per parameter."""
        present = [i for i, g in enumerate(grads) if g is not None]
        s = None
        if max_grad_norm is not None:
            self.sumsq = restate_sumsq([widen(grads[i]) for i in present])
            s = clip_coefficient(self.sumsq, max_grad_norm)
        for i in present:
            self.t[i] += 1
            gr = self.groups[self.group_of[i]]
            nums = numbers(gr["lr"], gr["betas"], gr["eps"], gr["wd"], self.t[i])
            p0 = self.master[i] if self.master[i] is not None else widen(self.p[i])
            p2, self.m[i], self.v[i] = restate_step(p0, widen(grads[i]), self.m[i], self.v[i], nums, s)
            if self.master[i] is not None:
                self.master[i] = p2
            self.p[i] = narrow(p2, self.dtypes[i])


def bits(t):
    """The raw bits of a tensor (on the CPU), so that NaN payloads and the sign of zero count."""
    t = t.detach().cpu().contiguous().reshape(-1)
    return t.view(torch.int32) if t.dtype == torch.float32 else t.view(torch.int16)


def same_bits(a, b):
    a = torch.from_numpy(a) if isinstance(a, np.ndarray) else a
    b = torch.from_numpy(b) if isinstance(b, np.ndarray) else b
    return a.dtype == b.dtype and a.numel() == b.numel() and torch.equal(bits(a), bits(b))


# ---- CPU: restate() against torch ----------------------------------------------------------------------------------------

SIZES3 = (1, 7, 1000)
GROUPS2 = [dict(lr=1e-2, betas=(0.9, 0.999), eps=1e-8, wd=1e-2), dict(lr=3e-3, betas=(0.9, 0.999), eps=1e-8, wd=0.1)]
GROUP_OF3 = (0, 1, 1)


def scenario3(steps, seed=5):
    """Start values and `steps` gradient lists for the three tensors, float32 on the CPU."""
    g = torch.Generator().manual_seed(seed)
    values = [torch.randn(n, generator=g) for n in SIZES3]
    grads = [[torch.randn(n, generator=g) * 0.5 for n in SIZES3] for _ in range(steps)]
    return values, grads


def torch_groups(params, groups=GROUPS2, group_of=GROUP_OF3):
    return [dict(params=[p for p, gi in zip(params, group_of) if gi == k], lr=gr["lr"], betas=gr["betas"], eps=gr["eps"], weight_decay=gr["wd"])
            for k, gr in enumerate(groups)]


def torch_run(values, grads, dtype, clip):
    """torch.optim.AdamW(foreach=False) on the CPU in `dtype`, clip_grad_norm_ first when clip is given: p, m, v after every
    step, as float64."""
    params = [torch.nn.Parameter(x.to(dtype).clone()) for x in values]
    opt = torch.optim.AdamW(torch_groups(params), foreach=False)
    out = []
    for step in grads:
        for p, g in zip(params, step):
            p.grad = g.to(dtype).clone()
        if clip is not None:
            torch.nn.utils.clip_grad_norm_(params, clip)
        opt.step()
        out.append(([p.detach().double().clone() for p in params], [opt.state[p]["exp_avg"].double().clone() for p in params],
                    [opt.state[p]["exp_avg_sq"].double().clone() for p in params]))
    return out


def restate_run(values, grads, clip):
    r = Restated(values, [torch.float32] * 3, GROUP_OF3, GROUPS2)
    out = []
    for step in grads:
        r.step(step, clip)
        out.append(([torch.from_numpy(widen(p)).double() for p in r.p], [torch.from_numpy(m.copy()).double() for m in r.m],
                    [torch.from_numpy(v.copy()).double() for v in r.v]))
    return out


def deviation(run, ref):
    """The largest absolute deviation per quantity (p, m, v) over all steps and tensors."""
    return tuple(max(float((a - b).abs().max()) for sa, sb in zip(run, ref) for a, b in zip(sa[q], sb[q])) for q in range(3))


@functools.lru_cache(maxsize=None)
def yardstick(clip):
    """(float32 torch's deviation from float64 torch, restate()'s deviation from float64 torch), each (p, m, v), over 10
    steps of the scenario. Computed once per clip setting and shared by the tests that need it."""
    values, grads = scenario3(10)
    ref = torch_run(values, grads, torch.float64, clip)
    return deviation(torch_run(values, grads, torch.float32, clip), ref), deviation(restate_run(values, grads, clip), ref)


@pytest.mark.parametrize("clip", [None, 1.0])
def test_restate_against_torch(clip):
    """10 steps on 3 tensors (1, 7, 1000 elements) in two groups of different lr and weight decay, from the same float32 inputs:
    torch.optim.AdamW(foreach=False) in float32, the same in float64, and restate(); with clip = 1.0 the torch runs call
    clip_grad_norm_ first (the norm is about 16, so the coefficient is about 0.06). The yardstick is the float32 torch run's
    largest deviation from the float64 run per quantity; restate() is another, equally valid, rounding order of the same
    formula and must stay within 2 x that.
    Measured (p, m, v):   float32 torch vs float64       restate() vs float64
      no clipping         (1.07e-06, 3.18e-08, 1.39e-09)  (1.07e-06, 2.50e-08, 1.83e-09)
      clip = 1.0          (1.26e-06, 1.92e-09, 7.48e-12)  (1.26e-06, 3.48e-09, 1.11e-11)
    (With clipping the coefficient itself differs in its last bit between torch's order of the norm and the stated one, which
    moves every m and v together: 1.8 x and 1.5 x the yardstick, inside the factor 2.)"""
    f32, mine = yardstick(clip)
    print("float32 torch vs float64 (p, m, v):", f32, " restate vs float64:", mine)
    assert all(y > 0 for y in f32)
    for q, name in enumerate(("p", "m", "v")):
        assert mine[q] <= 2 * f32[q], (name, mine[q], f32[q])


def test_restate_sumsq_against_float64():
    """The stated order on 2 CHUNK + 17 elements and on a short tensor: within n u of the float64 sum (each square and each of
    at most n - 1 additions of non-negative terms carries one rounding, see test_gpu_grad_norm_bound)."""
    g = torch.Generator().manual_seed(9)
    grads = [torch.randn(2 * CHUNK + 17, generator=g).numpy(), torch.randn(5, generator=g).numpy()]
    want = sum(float((x.astype(np.float64) ** 2).sum()) for x in grads)
    n = sum(x.size for x in grads)
    assert abs(float(restate_sumsq(grads)) - want) <= (n + 1) * U * want
    assert restate_sumsq([]) == 0 and restate_sumsq([np.zeros(0, F)]) == 0


# ---- CPU: every ValueError ------------------------------------------------------------------------------------------------

def cpu_param(n=4, dtype=torch.float32, grad=True):
    p = torch.nn.Parameter(torch.zeros(n, dtype=dtype))
    if grad:
        p.grad = torch.ones(n, dtype=dtype)
    return p


@pytest.mark.parametrize("kwargs, text", [
    (dict(lr=-1e-3), "lr must be"), (dict(lr=float("nan")), "lr must be"), (dict(eps=-1e-8), "eps must be"),
    (dict(weight_decay=-0.1), "weight_decay must be"), (dict(betas=(1.0, 0.999)), "betas must be"), (dict(betas=(0.9, -0.1)), "betas must be"),
    (dict(betas=(0.9,)), "betas must be"), (dict(betas=(0.9, 1.0)), "betas must be"), (dict(master_weights=1), "master_weights must be")])
def test_constructor_value_errors(kwargs, text):
    with pytest.raises(ValueError, match=text):
        FusedAdamW([cpu_param()], **kwargs)


def test_step_value_errors_on_cpu_tensors():
    """Everything about the arguments that does not need the GPU is a ValueError raised before any launch, so it holds for CPU
    tensors; what is left for CPU tensors is the NovaHipError. (Mixed devices cannot be built without a GPU.)"""
    before = dict(M.stats)
    for bad in (0, -1.0, float("nan"), True, "1"):
        with pytest.raises(ValueError, match="max_grad_norm must be"):
            FusedAdamW([cpu_param()]).step(max_grad_norm=bad)
    p = cpu_param(dtype=torch.bfloat16)
    p.data = p.data.float()  # the gradient stays bfloat16
    with pytest.raises(ValueError, match="gradient: expected its parameter's dtype torch.float32, got torch.bfloat16"):
        FusedAdamW([p]).step()
    with pytest.raises(ValueError, match="parameter: expected float32, bfloat16 or float16, got torch.float64"):
        FusedAdamW([cpu_param(dtype=torch.float64)]).step()
    t = torch.nn.Parameter(torch.zeros(4, 3).t())
    t.grad = torch.ones(3, 4)
    assert not t.is_contiguous()
    with pytest.raises(ValueError, match="parameter: expected a contiguous tensor"):
        FusedAdamW([t]).step()
    c = cpu_param(12)
    c.grad = torch.ones(24)[::2]
    with pytest.raises(ValueError, match="gradient: expected a contiguous tensor"):
        FusedAdamW([c]).step()
    s = cpu_param(4, grad=False)
    s.grad = torch.sparse_coo_tensor(torch.tensor([[1]]), torch.tensor([1.0]), (4,))
    with pytest.raises(ValueError, match="takes dense tensors"):
        FusedAdamW([s]).step()
    opt = FusedAdamW([cpu_param()])
    opt.param_groups[0]["lr"] = -1.0  # what a scheduler may write
    with pytest.raises(ValueError, match="lr must be"):
        opt.step()
    opt = FusedAdamW([cpu_param()])
    opt.param_groups[0]["amsgrad"] = True
    with pytest.raises(ValueError, match="no amsgrad mode"):
        opt.step()
    # the order: max_grad_norm comes before the tensors, the parameter's dtype before the gradient's contiguity
    with pytest.raises(ValueError, match="max_grad_norm must be"):
        FusedAdamW([cpu_param(dtype=torch.float64)]).step(max_grad_norm=0)
    with pytest.raises(ValueError, match="parameter: expected float32"):
        FusedAdamW([c, cpu_param(dtype=torch.float64)]).step()
    ok = FusedAdamW([cpu_param()])
    with pytest.raises(H.NovaHipError, match="runs on the GPU"):
        ok.step()
    assert ok.state_dict()["state"] == {}  # refused before any state was made or any step counted
    FusedAdamW([cpu_param(grad=False)]).step(max_grad_norm=1.0)  # nothing has a gradient: nothing to do, even on the CPU
    assert M.stats == before


# ---- CPU: state_dict ------------------------------------------------------------------------------------------------------

def test_state_dict_format_matches_torch():
    a, b = cpu_param(3), cpu_param(5, dtype=torch.bfloat16)
    mine = FusedAdamW([dict(params=[a], lr=1e-2), dict(params=[b], weight_decay=0.3)]).state_dict()
    theirs = torch.optim.AdamW([dict(params=[a], lr=1e-2), dict(params=[b], weight_decay=0.3)]).state_dict()
    assert mine["state"] == theirs["state"] == {}
    assert [sorted(g) for g in mine["param_groups"]] == [sorted(g) for g in theirs["param_groups"]]
    assert mine["param_groups"] == theirs["param_groups"]  # the same values too: it loads into torch.optim.AdamW as it is
    torch.optim.AdamW([a, b]).load_state_dict(FusedAdamW([a, b]).state_dict())


def test_load_state_dict_keeps_float32_state_for_a_bfloat16_parameter():
    """A hand-built state in torch's format: the float32 moments hold values no bfloat16 has. torch's own loader casts them to
    the parameter's dtype; this one keeps them."""
    p = cpu_param(3, dtype=torch.bfloat16)
    fine = torch.tensor([1.0 + 2.0 ** -20, -3.0 - 2.0 ** -18, 2.0 ** -30])
    state = {"state": {0: {"step": torch.tensor(4.0), "exp_avg": fine.clone(), "exp_avg_sq": fine.abs()}},
             "param_groups": [dict(torch.optim.AdamW([p]).state_dict()["param_groups"][0], lr=0.5)]}
    theirs = torch.optim.AdamW([p])
    theirs.load_state_dict(state)
    assert theirs.state[p]["exp_avg"].dtype == torch.bfloat16  # the trap
    opt = FusedAdamW([p])
    opt.load_state_dict(state)
    st = opt.state[p]
    assert st["exp_avg"].dtype == st["exp_avg_sq"].dtype == torch.float32
    assert same_bits(st["exp_avg"], fine) and same_bits(st["exp_avg_sq"], fine.abs())
    assert st["exp_avg"].data_ptr() != state["state"][0]["exp_avg"].data_ptr()  # a copy, as torch's loader makes
    assert st["step"].dtype == torch.float32 and st["step"].device.type == "cpu" and float(st["step"]) == 4.0
    assert "master" not in st and opt.param_groups[0]["lr"] == 0.5
    out = opt.state_dict()["state"][0]
    assert sorted(out) == ["exp_avg", "exp_avg_sq", "step"] and out["exp_avg"].dtype == torch.float32
    state["state"][0]["master"] = fine.clone()  # a state of this class: the master copy stays float32 too
    opt.load_state_dict(state)
    assert same_bits(opt.state[p]["master"], fine)


# ---- CPU: header, table, Trainer -------------------------------------------------------------------------------------------

def test_header_constants_and_signatures():
    text = open(HEADER).read()
    const = lambda name: int(re.search(rf"#define {name} (\d+)", text).group(1))
    assert const("NOVA_ADAMW_CHUNK") == M.ADAMW_CHUNK == CHUNK
    assert const("NOVA_ADAMW_SUM_COLUMNS") == M.ADAMW_SUM_COLUMNS == COLUMNS
    assert const("NOVA_ADAMW_BLOCK") == M.ADAMW_BLOCK == BLOCK
    assert const("NOVA_ADAMW_MAX_N") == M.ADAMW_MAX_N == 2 ** 31 - 1
    assert CHUNK % (256 * 8) == 0
    assert "nova_adamw_sumsq" in H.SIGNATURES and "nova_adamw_step" in H.SIGNATURES
    body = re.search(r"typedef struct nova_adamw_tensor \{(.*?)\} nova_adamw_tensor;", text, re.S).group(1)
    assert re.findall(r"(\w+)\s*[,;]", body) == [k for k, _ in H.AdamWTensor._fields_]  # the names in front of a comma or semicolon
    assert ctypes.sizeof(H.AdamWTensor) == 80


def test_step_numbers_are_rounded_once():
    for t in (1, 2, 1000):
        want = numbers(3e-3, (0.9, 0.999), 1e-8, 0.1, t)
        got = M.step_numbers(3e-3, (0.9, 0.999), 1e-8, 0.1, float(t))
        assert [F(g) for g in got] == list(want) and all(float(F(g)) == g for g in got)


class _OneBatch(object):
    def next(self):
        return [None]


class _Quadratic(torch.nn.Module):
    """What Trainer needs of a model: blocks to configure, the modules it freezes, a loss."""

    def __init__(self):
        super().__init__()
        empty = lambda: torch.nn.Module()
        self.video_encoder, self.image_encoder, self.image_decoder = empty(), empty(), empty()
        for m in (self.video_encoder, self.image_encoder, self.image_decoder):
            m.blocks = torch.nn.ModuleList()
        self.video_encoder.patch_embed = torch.nn.Linear(2, 2)
        self.text_embed = empty()
        self.text_embed.norm = torch.nn.LayerNorm(2)
        self.video_pos_embed = torch.nn.Linear(2, 2)
        self.motion_embed = None
        self.w = torch.nn.Parameter(torch.tensor([1.0, -2.0, 3.0]))

    def forward(self, inputs):
        return {"loss": (self.w * self.w).sum()}


def trainer_with(target, monkeypatch, clip=0.5):
    from diffnext.engine.train_engine import Trainer

    calls = {"fused": [], "clip": []}
    monkeypatch.setattr(FusedAdamW, "step", lambda self, closure=None, max_grad_norm=None: calls["fused"].append((closure, max_grad_norm)))
    real = torch.nn.utils.clip_grad_norm_
    monkeypatch.setattr(torch.nn.utils, "clip_grad_norm_", lambda params, c, *a, **k: (calls["clip"].append(c), real(params, c, *a, **k))[1])
    training = {"max_grad_norm": clip} if clip is not None else {}
    config = {"training": training, "optimizer": {"target": target, "params": {"lr": 0.1}},
              "lr_scheduler": {"target": "ConstantLR", "params": {"lr_max": 0.1}}}
    return Trainer(config, _Quadratic(), _OneBatch()), calls


def test_trainer_passes_the_clip_to_the_fused_step(monkeypatch):
    for target in ("FusedAdamW", "nova_pointcloud_amd.optim.FusedAdamW"):
        trainer, calls = trainer_with(target, monkeypatch)
        assert type(trainer.optimizer) is FusedAdamW
        trainer.optimizer.param_groups[0]["lr_scale"] = 0.5
        stats = trainer.run_step()
        assert calls == {"fused": [(None, 0.5)], "clip": []}
        assert trainer.optimizer.param_groups[0]["lr"] == 0.05 and stats["lr"] == 0.1  # lr_scale only writes group["lr"]
        assert trainer.model.w.grad is None  # zero_grad(set_to_none=True) as before
        monkeypatch.undo()
    trainer, calls = trainer_with("FusedAdamW", monkeypatch, clip=None)
    trainer.run_step()
    assert calls == {"fused": [(None, None)], "clip": []}


def test_trainer_keeps_the_torch_path_for_other_targets(monkeypatch):
    trainer, calls = trainer_with("torch.optim.AdamW", monkeypatch)
    assert type(trainer.optimizer) is torch.optim.AdamW
    w0 = trainer.model.w.detach().clone()
    trainer.run_step()
    assert calls == {"fused": [], "clip": [0.5]} and not torch.equal(trainer.model.w.detach(), w0)
    monkeypatch.undo()
    trainer, calls = trainer_with("SGD", monkeypatch, clip=None)
    assert type(trainer.optimizer) is torch.optim.SGD
    trainer.run_step()
    assert calls == {"fused": [], "clip": []}


# ---- the entry points' argument checks: validation-only calls, rejected before any launch ---------------------------------

def abi_rejections(lib):
    ARG = -1
    err = lambda: lib.nova_last_error().decode()
    keep = (ctypes.c_float * 8)()
    there = ctypes.addressof(keep)  # never dereferenced: every call below is refused by the checks

    def table(n=4, dtype=0, **fields):
        t = (H.AdamWTensor * 1)()
        t[0].param = t[0].grad = t[0].exp_avg = t[0].exp_avg_sq = there
        t[0].n, t[0].dtype = n, dtype
        for k, v in fields.items():
            setattr(t[0], k, v)
        return t

    step = lambda t, count=1, sumsq=None, max_norm=0.0: lib.nova_adamw_step(t, count, sumsq, max_norm, None)
    sumsq = lambda t, count=1, ws=there, floats=8, out=there + 16, norm=None: lib.nova_adamw_sumsq(t, count, ws, floats, out, norm, None)
    for call, who in ((step, "adamw_step"), (sumsq, "adamw_sumsq")):
        assert call(table(), count=-1) == ARG and err() == f"{who}: count -1 is negative"
        assert call(None) == ARG and err() == f"{who}: null pointer tensors"
        assert call(table(n=-1)) == ARG and err() == f"{who}: tensor 0: n -1 outside 0 .. 2^31 - 1"
        assert call(table(n=2 ** 31)) == ARG and err() == f"{who}: tensor 0: n 2147483648 outside 0 .. 2^31 - 1"
        assert call(table(dtype=7)) == ARG and err() == f"{who}: tensor 0: unknown dtype code 7 (NOVA_F32, NOVA_BF16, NOVA_F16)"
        assert call(table(n=-1, dtype=7, grad=None)) == ARG and "n -1 outside" in err()  # the order: n, dtype, pointers
        assert call(table(dtype=7, grad=None)) == ARG and "unknown dtype code 7" in err()
        assert call(table(grad=None)) == ARG and err() == f"{who}: tensor 0: null pointer grad"
        assert call(table(n=0, grad=None, param=None, exp_avg=None, exp_avg_sq=None)) == 0  # nothing to touch, nothing launched
        assert call(None, count=0) == 0
    for field in ("param", "exp_avg", "exp_avg_sq"):
        assert step(table(**{field: None})) == ARG and err() == f"adamw_step: tensor 0: null pointer {field}"
        assert sumsq(table(n=0, **{field: None})) == 0  # the sum reads the gradient alone
    assert step(table(param=None, grad=None)) == ARG and err().endswith("null pointer param")
    for bad, shown in ((0.0, "0"), (-2.0, "-2"), (float("nan"), "nan")):
        assert step(table(), sumsq=there, max_norm=bad) == ARG and err() == f"adamw_step: max_norm {shown} must be > 0 when sumsq is given"
    assert step(table(grad=None), sumsq=there, max_norm=0.0) == ARG and err().endswith("null pointer grad")  # the list comes first
    assert sumsq(table(), ws=None) == ARG and err() == "adamw_sumsq: null pointer workspace"
    assert sumsq(table(n=CHUNK + 1), floats=1) == ARG and err() == f"adamw_sumsq: the workspace holds 1 floats, the list has 2 chunks of {CHUNK}"
    assert sumsq(table(), out=None) == ARG and err() == "adamw_sumsq: null pointer sumsq"
    assert sumsq(table(), out=there) == ARG and err() == "adamw_sumsq: sumsq overlaps the workspace"
    assert sumsq(table(), norm=there) == ARG and err() == "adamw_sumsq: norm overlaps the workspace"
    assert sumsq(table(), norm=there + 16) == ARG and err() == "adamw_sumsq: norm and sumsq overlap each other"


def test_abi_rejections_without_a_device():
    abi_rejections(H.load(check_device=False))


# ---- GPU -------------------------------------------------------------------------------------------------------------------

DEV = "cuda:0"
SIZES = (0, 1, 3, 4, 5, CHUNK - 1, CHUNK, CHUNK + 1, 2 * CHUNK + 17)
GROUP = dict(lr=1e-2, betas=(0.9, 0.999), eps=1e-8, wd=1e-2)
DTYPES = [torch.float32, torch.bfloat16, torch.float16]


def inputs(sizes, dtype, steps, seed=3):
    """Start values and `steps` gradient lists (CPU tensors of `dtype`) for tensors of `sizes`; a few exact zeros among them."""
    g = torch.Generator().manual_seed(seed)
    values = [torch.randn(n, generator=g).to(dtype) for n in sizes]
    grads = []
    for _ in range(steps):
        step = [(torch.randn(n, generator=g) * 0.5).to(dtype) for n in sizes]
        for x in step:
            x[::7] = 0
        grads.append(step)
    return values, grads


def placed(x, off, dtype=None):
    """A copy of the flat CPU tensor x on the GPU as a view that starts `off` elements into a larger storage."""
    big = torch.zeros(x.numel() + off + 8, dtype=dtype or x.dtype, device=DEV)
    view = big[off:off + x.numel()]
    view.copy_(x.to(DEV))
    assert view.is_contiguous() and (x.numel() == 0 or view.data_ptr() == big.data_ptr() + off * big.element_size())
    return view


class Fused(object):
    """FusedAdamW on GPU copies of `values`, each tensor's parameter, gradient, moments and master copy starting offs(i, which)
    elements into their storages (0: the allocator's alignment)."""

    def __init__(self, values, groups, group_of, master_weights=True, offs=lambda i, which: 0):
        self.offs = offs
        self.params = [torch.nn.Parameter(placed(x, offs(i, 0))) for i, x in enumerate(values)]
        self.opt = FusedAdamW([dict(params=[p for p, gi in zip(self.params, group_of) if gi == k], lr=gr["lr"], betas=gr["betas"], eps=gr["eps"],
                                    weight_decay=gr["wd"]) for k, gr in enumerate(groups)], master_weights=master_weights)
        if any(offs(i, w) for i in range(len(values)) for w in range(5)):
            for i, (p, x) in enumerate(zip(self.params, values)):  # the state torch would make, placed by hand
                zero = torch.zeros(x.numel())
                st = {"step": torch.tensor(0.0), "exp_avg": placed(zero, offs(i, 2)), "exp_avg_sq": placed(zero, offs(i, 3))}
                if master_weights and x.dtype in HALF:
                    st["master"] = placed(x.float(), offs(i, 4))
                self.opt.state[p] = st

    def step(self, grads, max_grad_norm=None):
        for i, (p, g) in enumerate(zip(self.params, grads)):
            p.grad = placed(g, self.offs(i, 1)) if g is not None else None
        self.opt.step(max_grad_norm=max_grad_norm)

    def state(self, i, key):
        return self.opt.state[self.params[i]].get(key)

    def sumsq(self):
        """nova_adamw_sumsq itself over the gradients present, as the step just called it: the float32 before the square root."""
        grads = [p.grad for p in self.params if p.grad is not None]
        table = (H.AdamWTensor * max(len(grads), 1))()
        for e, g in zip(table, grads):
            e.grad, e.n, e.dtype = g.data_ptr(), g.numel(), H.dtype_code(g.dtype)
        chunks = sum(-(-g.numel() // CHUNK) for g in grads)
        ws, out = torch.empty(max(chunks, 1), device=DEV), torch.full((), -1.0, device=DEV)
        H.call("nova_adamw_sumsq", table, len(grads), ws.data_ptr(), ws.numel(), out.data_ptr(), None, H.stream_ptr())
        return out


def norm_of(sumsq):
    """The correctly rounded float32 square root of the float32 sum of squares, as the kernel stores the norm."""
    return torch.tensor(float(np.sqrt(F(sumsq))), dtype=torch.float32)


def check_against(fused, ref, clip, what=""):
    for i in range(len(ref.p)):
        assert same_bits(fused.params[i], ref.p[i]), (what, "p", i)
        if ref.t[i] == 0:
            continue
        assert same_bits(fused.state(i, "exp_avg"), ref.m[i]), (what, "m", i)
        assert same_bits(fused.state(i, "exp_avg_sq"), ref.v[i]), (what, "v", i)
        assert (fused.state(i, "master") is None) == (ref.master[i] is None)
        if ref.master[i] is not None:
            assert same_bits(fused.state(i, "master"), ref.master[i]), (what, "master", i)
        assert float(fused.state(i, "step")) == ref.t[i]
    if clip is not None:
        assert same_bits(fused.sumsq(), torch.tensor(float(ref.sumsq))), (what, float(fused.sumsq()), float(ref.sumsq))
        assert same_bits(fused.opt.grad_norm, norm_of(ref.sumsq)), (what, float(fused.opt.grad_norm), float(norm_of(ref.sumsq)))
    else:
        assert fused.opt.grad_norm is None


@functools.lru_cache(maxsize=None)
def restated_sizes(dtype, clip):
    """restate() over SIZES for 3 steps, computed once per (dtype, clip): the snapshots after every step."""
    values, grads = inputs(SIZES, dtype, 3)
    ref = Restated(values, [dtype] * len(SIZES), [0] * len(SIZES), [GROUP])
    shots = []
    for step in grads:
        ref.step(step, clip)
        shots.append(copy.deepcopy(ref))
    return shots


@pytest.mark.gpu
@pytest.mark.parametrize("clip", [None, 2.0], ids=["noclip", "clip"])
@pytest.mark.parametrize("dtype", DTYPES, ids=["f32", "bf16", "f16"])
def test_gpu_sizes_bitwise(hip, dtype, clip):
    """Sizes 0, 1, 3, 4, 5, CHUNK - 1, CHUNK, CHUNK + 1 and 2 CHUNK + 17 in one list, 3 consecutive steps (t = 1 and t > 1), with
    and without clipping (the norm is about 90, so max_grad_norm = 2 scales): p, m, v, master and the norm are restate()'s bits."""
    values, grads = inputs(SIZES, dtype, 3)
    fused = Fused(values, [GROUP], [0] * len(SIZES))
    for k, step in enumerate(grads):
        fused.step(step, clip)
        check_against(fused, restated_sizes(dtype, clip)[k], clip, f"step {k + 1}")
    if clip is not None:
        assert clip_coefficient(restated_sizes(dtype, clip)[0].sumsq, clip) < 0.1


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", DTYPES, ids=["f32", "bf16", "f16"])
def test_gpu_alignment(hip, dtype):
    """The same tensors as views starting 1, 2 and 3 elements into a larger storage, parameter, gradient, moments and master
    copy offset independently: identical to the aligned run (which is restate()'s)."""
    values, grads = inputs(SIZES, dtype, 3)
    offs = lambda i, which: (1 + i + 2 * which + (i * which) % 3) % 4  # every tensor mixes offsets; some pointers stay aligned
    assert {offs(i, w) for i in range(len(SIZES)) for w in range(5)} == {0, 1, 2, 3}
    assert any(len({offs(i, w) for w in range(5)}) > 2 for i in range(len(SIZES)))
    aligned, shifted = Fused(values, [GROUP], [0] * len(SIZES)), Fused(values, [GROUP], [0] * len(SIZES), offs=offs)
    for k, step in enumerate(grads):
        aligned.step(step, 2.0), shifted.step(step, 2.0)
        for i in range(len(SIZES)):
            assert same_bits(aligned.params[i], shifted.params[i]), (k, i)
            for key in ("exp_avg", "exp_avg_sq", "master"):
                a, b = aligned.state(i, key), shifted.state(i, key)
                assert (a is None and b is None) or same_bits(a, b), (k, i, key)
        assert same_bits(aligned.opt.grad_norm, shifted.opt.grad_norm)
        check_against(shifted, restated_sizes(dtype, 2.0)[k], 2.0, f"step {k + 1}")
    assert any(p.data_ptr() % 16 for p in shifted.params) and any(p.grad.data_ptr() % 16 for p in shifted.params)


@pytest.mark.gpu
def test_gpu_list_longer_than_one_launch(hip):
    """BLOCK + 1 tensors of 5 elements: the same results as the first BLOCK and the last one stepped in two separate optimizers.
    The sum of squares depends on the list by definition, so it is compared within the long list only, and the long list is
    clipped with a max_grad_norm above the norm: s = 1, and the multiplication by 1 is exact."""
    sizes = (5,) * (BLOCK + 1)
    values, grads = inputs(sizes, torch.float32, 2, seed=11)
    whole = Fused(values, [GROUP], [0] * len(sizes))
    head, tail = Fused(values[:BLOCK], [GROUP], [0] * BLOCK), Fused(values[BLOCK:], [GROUP], [0])
    ref = Restated(values, [torch.float32] * len(sizes), [0] * len(sizes), [GROUP])
    before = dict(M.stats)
    for step in grads:
        whole.step(step, 1e6)
        head.step(step[:BLOCK]), tail.step(step[BLOCK:])
        ref.step(step, 1e6)
        assert clip_coefficient(ref.sumsq, 1e6) == 1
        check_against(whole, ref, 1e6)
        for i in range(len(sizes)):
            other, j = (head, i) if i < BLOCK else (tail, i - BLOCK)
            assert same_bits(whole.params[i], other.params[j]) and same_bits(whole.state(i, "exp_avg_sq"), other.state(j, "exp_avg_sq"))
    made = {k: M.stats[k] - before[k] for k in before}
    assert made == {"sumsq_calls": 2, "sumsq_launches": 2 * 3, "step_calls": 6, "step_launches": 2 * (2 + 1 + 1)}


@pytest.mark.gpu
def test_gpu_clipping(hip):
    """max_grad_norm above the norm is bitwise the unclipped result (s = 1: the multiplication is exact); below it, it scales,
    as restate() does; two runs give the same bits."""
    sizes = (3, CHUNK + 1, 700)
    values, grads = inputs(sizes, torch.float32, 1, seed=21)
    runs = {}
    for name, clip in (("none", None), ("above", 1e4), ("below", 0.25), ("again", 0.25)):
        runs[name] = Fused(values, [GROUP], [0] * 3)
        runs[name].step(grads[0], clip)
        ref = Restated(values, [torch.float32] * 3, [0] * 3, [GROUP])
        ref.step(grads[0], clip)
        check_against(runs[name], ref, clip, name)
    for i in range(3):
        assert same_bits(runs["none"].params[i], runs["above"].params[i]) and same_bits(runs["none"].state(i, "exp_avg"), runs["above"].state(i, "exp_avg"))
        assert same_bits(runs["below"].params[i], runs["again"].params[i]) and same_bits(runs["below"].state(i, "exp_avg_sq"), runs["again"].state(i, "exp_avg_sq"))
        assert not same_bits(runs["none"].state(i, "exp_avg"), runs["below"].state(i, "exp_avg"))
    assert same_bits(runs["below"].opt.grad_norm, runs["again"].opt.grad_norm) and same_bits(runs["below"].opt.grad_norm, runs["above"].opt.grad_norm)
    norm = float(runs["below"].opt.grad_norm)
    # the first moment after one step from zero is w1 (g s): the scale shows in it. From the float32 norm on, five roundings
    # (the sum with 1e-6, the quotient, g s, w1 itself, the product): 5 u per element, asserted at 6 u for the float64 side's own
    s = 0.25 / (norm + 1e-6)
    m, g = runs["below"].state(1, "exp_avg").cpu().double(), grads[0][1].double()
    assert s < 0.01 and bool(((m - 0.1 * s * g).abs() <= 6 * U * (0.1 * s * g).abs()).all())


@pytest.mark.gpu
def test_gpu_grad_norm_bound(hip):
    """grad_norm against the float64 norm. With u = 2^-24 and n elements: every square is rounded once, and every partial sum
    an element enters is rounded once, in ANY order at most n - 1 of them, so the float32 sum of squares is
    S' = sum g_i^2 (1 + d_i) with |d_i| <= (1 + u)^n - 1, i.e. |S' - S| <= n u S (1 + O(n u)) since all terms are >= 0 (no
    cancellation). The norm is sqrt(S') rounded once: sqrt(S') = sqrt(S) sqrt(1 + d), |sqrt(1 + d) - 1| <= |d| / 2 ... so
    |grad_norm - sqrt(S)| <= (n u / 2 + u) sqrt(S) (1 + O(n u)) <= (n + 2) u sqrt(S) / 2 (1 + O(n u)). Asserted with the
    second-order factor 1 + n u written out. (The kernel's order is far shallower than n: 32 + 8 + ceil(P / 256) + 8
    additions on any path, so the figure printed is much smaller.)"""
    sizes = (2 * CHUNK + 17, 5, CHUNK)
    n = sum(sizes)
    for dtype in DTYPES:
        values, grads = inputs(sizes, dtype, 1, seed=31)
        fused = Fused(values, [GROUP], [0] * 3)
        fused.step(grads[0], 1.0)
        want = math.sqrt(sum(float((g.double() ** 2).sum()) for g in grads[0]))
        got = float(fused.opt.grad_norm)
        assert fused.opt.grad_norm.dim() == 0 and fused.opt.grad_norm.dtype == torch.float32 and fused.opt.grad_norm.is_cuda
        print(dtype, "grad_norm", got, "float64", want, "relative", abs(got - want) / want, "bound", (n + 2) * U / 2)
        assert abs(got - want) <= (n + 2) * U / 2 * (1 + n * U) * want


@pytest.mark.gpu
def test_gpu_master_weights(hip):
    """A bfloat16 parameter at 1.0 stepped 50 times with lr = 1e-4 and a constant gradient: every update is about lr, far below
    half a bfloat16 ulp (2^-9 below 1.0). With master weights the float32 copy moves every step and the parameter flips once
    the sum passes 2^-9 (about 20 steps); without them the parameter never moves. Both are restate()'s bits."""
    group = dict(lr=1e-4, betas=(0.9, 0.999), eps=1e-8, wd=0.0)
    values = [torch.ones(19, dtype=torch.bfloat16)]
    grad = [torch.full((19,), 0.5, dtype=torch.bfloat16)]
    with_master, without = Fused(values, [group], [0], master_weights=True), Fused(values, [group], [0], master_weights=False)
    ref_with, ref_without = Restated(values, [torch.bfloat16], [0], [group], True), Restated(values, [torch.bfloat16], [0], [group], False)
    masters, flipped_at = [], None
    for k in range(50):
        for run in (with_master, without, ref_with, ref_without):
            run.step(grad)
        masters.append(float(with_master.state(0, "master")[0]))
        if flipped_at is None and float(with_master.params[0].detach()[0]) != 1.0:
            flipped_at = k + 1
        assert float(without.params[0].detach().float().min()) == 1.0 and without.state(0, "master") is None
    assert all(b < a for a, b in zip([1.0] + masters, masters))  # the master copy moves every step
    assert flipped_at is not None and 10 < flipped_at < 40 and float(with_master.params[0].detach()[0]) == 1.0 - 2.0 ** -8
    check_against(with_master, ref_with, None)
    check_against(without, ref_without, None)
    assert with_master.state(0, "master").dtype == torch.float32
    assert same_bits(with_master.params[0], with_master.state(0, "master").to(torch.bfloat16))  # the parameter is the master rounded once


@pytest.mark.gpu
def test_gpu_skipped_work(hip):
    """A parameter without a gradient is untouched and its step count not advanced; a list without any gradient launches
    nothing; the gradients are bit-identical before and after a step."""
    sizes = (5, CHUNK + 3, 9)
    values, grads = inputs(sizes, torch.bfloat16, 2, seed=41)
    fused = Fused(values, [GROUP], [0] * 3)
    ref = Restated(values, [torch.bfloat16] * 3, [0] * 3, [GROUP])
    first = [grads[0][0], None, grads[0][2]]
    fused.step(first, 1.5), ref.step(first, 1.5)
    assert "step" not in fused.opt.state[fused.params[1]] and same_bits(fused.params[1], values[1])
    check_against(fused, ref, 1.5)
    fused.step(grads[1], 1.5), ref.step(grads[1], 1.5)
    assert [float(fused.state(i, "step")) for i in range(3)] == [2.0, 1.0, 2.0]
    check_against(fused, ref, 1.5)
    kept = [p.grad for p in fused.params]
    for p, g in zip(fused.params, grads[1]):
        assert same_bits(p.grad, g)  # the step that just ran did not write them
    before, params_before = dict(M.stats), [p.detach().clone() for p in fused.params]
    fused.step([None, None, None], 1.5)
    fused.step([None, None, None])
    assert M.stats == before and fused.opt.grad_norm is None
    assert all(same_bits(a, b) for a, b in zip(params_before, fused.params)) and [float(fused.state(i, "step")) for i in range(3)] == [2.0, 1.0, 2.0]
    del kept
    empty = Fused([torch.zeros(0)], [GROUP], [0])  # only an empty tensor: nothing to launch, the norm is +0
    empty.step([torch.zeros(0)], 1.0)
    assert M.stats["sumsq_launches"] == before["sumsq_launches"] and M.stats["step_launches"] == before["step_launches"]
    assert same_bits(empty.opt.grad_norm, torch.zeros(()))


@pytest.mark.gpu
@pytest.mark.parametrize("direction", ["fused_to_torch", "torch_to_fused"])
def test_gpu_state_dict_interchange(hip, direction):
    """Five steps of one optimizer, its state_dict into the other class on the same float32 parameters, then one more step of
    each from that state: the two agree within 2 x the CPU test's yardstick (float32 torch against float64 torch on the same
    scenario, per quantity), the two being equally valid rounding orders of the same formula."""
    values, grads = scenario3(6)
    make_params = lambda: [torch.nn.Parameter(x.to(DEV)) for x in values]

    def build(kind, params):
        groups = torch_groups(params)
        return FusedAdamW(groups) if kind == "fused" else torch.optim.AdamW(groups, foreach=False)

    def step(opt, params, step_grads):
        for p, g in zip(params, step_grads):
            p.grad = g.to(DEV)
        opt.step()

    first_kind, second_kind = ("fused", "torch") if direction == "fused_to_torch" else ("torch", "fused")
    pa = make_params()
    a = build(first_kind, pa)
    for k in range(5):
        step(a, pa, grads[k])
    pb = [torch.nn.Parameter(p.detach().clone()) for p in pa]
    b = build(second_kind, pb)
    b.load_state_dict(copy.deepcopy(a.state_dict()))  # as a checkpoint holds it: torch's loader shares `step` with its source
    for p in pb:
        st = b.state[p]
        assert float(st["step"]) == 5.0 and st["exp_avg"].dtype == torch.float32 and st["exp_avg"].device == p.device and "master" not in st
    step(a, pa, grads[5]), step(b, pb, grads[5])
    (yp, ym, yv), _ = yardstick(None)
    for p, q in zip(pa, pb):
        assert float(a.state[p]["step"]) == float(b.state[q]["step"]) == 6.0
        assert float((p.detach() - q.detach()).abs().max()) <= 2 * yp
        assert float((a.state[p]["exp_avg"] - b.state[q]["exp_avg"]).abs().max()) <= 2 * ym
        assert float((a.state[p]["exp_avg_sq"] - b.state[q]["exp_avg_sq"]).abs().max()) <= 2 * yv


@pytest.mark.gpu
def test_gpu_abi_rejections(hip):
    abi_rejections(hip.load())
