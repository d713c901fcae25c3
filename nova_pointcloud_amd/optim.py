"""Fused AdamW with in-kernel gradient clipping on MI355X: what the reference's trainer does after the backward,
torch.nn.utils.clip_grad_norm_ and then torch.optim.AdamW with betas (0.9, 0.999) (train_newloss.py:827-841, :1060-1082), as
the two entry points of csrc/adamw.hip over the whole parameter list: nova_adamw_sumsq (the float32 sum of squares of every
gradient, in a fixed order, left on the device beside its square root, the norm) and nova_adamw_step (the update, with
torch's clip coefficient formed in the kernel from that sum). Each gradient is read twice and never written, each parameter
and each moment is read and written once, and the host never waits for the device. The definition, every rounding and the order of the sum, is in
include/nova_hip.h at nova_adamw_step.
bfloat16 / float16 parameters keep a float32 master copy that the same kernel updates (master_weights=True): the 16-bit
parameter is the master rounded once, so an update below half a 16-bit ulp is not lost.
GPU tensors only: NovaHipError for CPU parameters or a missing library. Results are bitwise reproducible: the same for every
run, every alignment of the storage and every split of the list over launches."""
import math
import numbers
from itertools import chain

import numpy as np
import torch

from . import hip
from ._pointset import _chunks

ADAMW_CHUNK = 8192  # == NOVA_ADAMW_CHUNK of include/nova_hip.h: elements per partial of the sum of squares
ADAMW_SUM_COLUMNS = 256  # == NOVA_ADAMW_SUM_COLUMNS: columns of the partials' last sum
ADAMW_BLOCK = 32  # == NOVA_ADAMW_BLOCK: tensors per launch
ADAMW_MAX_N = (1 << 31) - 1  # == NOVA_ADAMW_MAX_N: elements per tensor
_NATIVE = (torch.float32, torch.bfloat16, torch.float16)  # what the kernels read and write as it is
_FLOAT32_STATE = ("exp_avg", "exp_avg_sq", "master")  # float32 whatever the parameter's dtype

# since import: calls of nova_adamw_sumsq / nova_adamw_step and the kernel launches they made (one per block of ADAMW_BLOCK
# tensors with elements, plus the last sum of nova_adamw_sumsq). A step with no gradient, or only empty ones, makes none
stats = {"sumsq_calls": 0, "sumsq_launches": 0, "step_calls": 0, "step_launches": 0}


def _torch_group_defaults():
    """The keys torch.optim.AdamW keeps in a parameter group beside ours, at their defaults (amsgrad, maximize, foreach,
    capturable, differentiable, fused, ...): a state_dict of FusedAdamW carries them, so it loads into torch.optim.AdamW."""
    return {k: v for k, v in torch.optim.AdamW([torch.zeros(1)]).defaults.items() if k not in ("lr", "betas", "eps", "weight_decay")}


def _check_hyper(lr, betas, eps, weight_decay):
    """ValueError, in this order: lr, eps, betas, weight_decay (torch.optim.AdamW's order and ranges; a NaN fails)."""
    real = lambda v: isinstance(v, numbers.Real) and not isinstance(v, bool)
    if not (real(lr) and lr >= 0):
        raise ValueError(f"lr must be a real number >= 0, got {lr!r}")
    if not (real(eps) and eps >= 0):
        raise ValueError(f"eps must be a real number >= 0, got {eps!r}")
    if not (isinstance(betas, (tuple, list)) and len(betas) == 2 and all(real(b) and 0 <= b < 1 for b in betas)):
        raise ValueError(f"betas must be two real numbers in [0, 1), got {betas!r}")
    if not (real(weight_decay) and weight_decay >= 0):
        raise ValueError(f"weight_decay must be a real number >= 0, got {weight_decay!r}")


def step_numbers(lr, betas, eps, weight_decay, t):
    """(decay, w1, b2, w2, q, a, eps) of nova_adamw_tensor for step count t >= 1: each formed in float64 and rounded once to
    float32 (returned as Python floats that hold float32 values)."""
    f = lambda v: float(np.float32(v))
    lr, b1, b2, t = float(lr), float(betas[0]), float(betas[1]), float(t)
    return (f(1.0 - lr * float(weight_decay)), f(1.0 - b1), f(b2), f(1.0 - b2), f(math.sqrt(1.0 - b2 ** t)), f(lr / (1.0 - b1 ** t)), f(float(eps)))


class FusedAdamW(torch.optim.Optimizer):
    """AdamW (decoupled weight decay, torch.optim.AdamW's formula) whose step is one HIP pass over the parameter list, with
    torch's clip_grad_norm_ folded in: step(max_grad_norm=c) clips by the total 2-norm of all gradients without writing them.

    Parameter groups behave as in torch (per-group lr, betas, eps, weight_decay). State per parameter, under torch's names:
    `step` (a float32 CPU scalar tensor), `exp_avg` and `exp_avg_sq` (float32 whatever the parameter's dtype), and `master`
    (float32) for bfloat16 / float16 parameters when master_weights is on, made from the parameter at first use.
    state_dict() / load_state_dict() interchange with torch.optim.AdamW; a state loaded into this class keeps its float32
    tensors float32 (torch's loader would cast them to the parameter's dtype).

    `stats` (module level) counts calls and launches; `grad_norm` holds the last step's pre-clip norm."""

    def __init__(self, params, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=1e-2, master_weights=True):
        _check_hyper(lr, betas, eps, weight_decay)
        if not isinstance(master_weights, bool):
            raise ValueError(f"master_weights must be a bool, got {master_weights!r}")
        super().__init__(params, dict(lr=lr, betas=tuple(betas), eps=eps, weight_decay=weight_decay, **_torch_group_defaults()))
        self.master_weights = master_weights
        self.grad_norm = None  # after step(max_grad_norm=c): the total norm before clipping, a 0-dim device tensor
        self._workspace = None  # the partials of the sum of squares; grown as needed, nothing of a gradient is kept

    def _step_arguments(self, max_grad_norm):
        """ValueError for everything that does not need the GPU (so it holds for CPU tensors too), in one order, each check over
        the whole list before the next: max_grad_norm; the groups' numbers (lr, eps, betas, weight_decay, then the torch modes
        this class does not have); sparse tensors; the parameter's dtype; the gradient's dtype; contiguity (parameter, then
        gradient); size; devices. Returns [(group, parameter)] for the parameters that have a gradient."""
        if max_grad_norm is not None and not (isinstance(max_grad_norm, numbers.Real) and not isinstance(max_grad_norm, bool) and max_grad_norm > 0):
            raise ValueError(f"max_grad_norm must be None or a real number > 0, got {max_grad_norm!r}")
        for group in self.param_groups:
            _check_hyper(group["lr"], group["betas"], group["eps"], group["weight_decay"])
            for mode in ("amsgrad", "maximize", "capturable", "differentiable"):
                if group.get(mode):
                    raise ValueError(f"FusedAdamW has no {mode} mode (the group sets {mode}={group[mode]!r})")
        work = [(group, p) for group in self.param_groups for p in group["params"] if p.grad is not None]
        for _, p in work:
            if p.layout != torch.strided or p.grad.layout != torch.strided:
                raise ValueError(f"FusedAdamW takes dense tensors, got a {p.layout} parameter with a {p.grad.layout} gradient")
        for _, p in work:
            if p.dtype not in _NATIVE:
                raise ValueError(f"parameter: expected float32, bfloat16 or float16, got {p.dtype}")
        for _, p in work:
            if p.grad.dtype != p.dtype:
                raise ValueError(f"gradient: expected its parameter's dtype {p.dtype}, got {p.grad.dtype}")
        for _, p in work:
            if not p.is_contiguous():
                raise ValueError(f"parameter: expected a contiguous tensor, got shape {tuple(p.shape)} with strides {p.stride()}")
            if not p.grad.is_contiguous():
                raise ValueError(f"gradient: expected a contiguous tensor, got shape {tuple(p.grad.shape)} with strides {p.grad.stride()}")
        for _, p in work:
            if p.numel() > ADAMW_MAX_N:
                raise ValueError(f"parameter: the AdamW kernel takes at most {ADAMW_MAX_N} elements per tensor, got {p.numel()}")
        for _, p in work:
            for t, name in ((p, "parameter"), (p.grad, "gradient")):
                if t.device != work[0][1].device:
                    raise ValueError(f"all parameters and gradients must be on one device, got {work[0][1].device} and {t.device} ({name})")
        return work

    def _state_of(self, p):
        """The parameter's state, made at first use and repaired after a load: float32 moments and master on the parameter's
        device, the step count a float32 CPU scalar tensor."""
        st = self.state[p]
        if "step" not in st:
            st["step"] = torch.tensor(0.0, dtype=torch.float32)
        for key in ("exp_avg", "exp_avg_sq"):
            if key not in st:
                st[key] = torch.zeros(p.shape, dtype=torch.float32, device=p.device)
        if self.master_weights and p.dtype != torch.float32 and "master" not in st:
            st["master"] = p.detach().float().contiguous()  # exact: every 16-bit value is a float32
        for key in _FLOAT32_STATE:
            t = st.get(key)
            if t is not None and not (t.dtype == torch.float32 and t.device == p.device and t.is_contiguous() and t.numel() == p.numel()):
                if t.numel() != p.numel():
                    raise ValueError(f"state {key}: expected {p.numel()} elements (its parameter's), got {t.numel()}")
                st[key] = t.to(device=p.device, dtype=torch.float32).contiguous()
        return st

    @torch.no_grad()
    def step(self, closure=None, max_grad_norm=None):
        """One AdamW step of every parameter that has a gradient; a parameter whose .grad is None is skipped and its step count
        not advanced. max_grad_norm=c > 0: the gradients of ALL groups are clipped to the total 2-norm c first, as
        torch.nn.utils.clip_grad_norm_(parameters, c) does (coefficient min(1, c / (norm + 1e-6))), inside the update: the
        gradients themselves are not written. self.grad_norm is then the norm before clipping as a 0-dim float32 device tensor
        (no .item(), no synchronisation); without max_grad_norm it is None. A closure, if given, is evaluated with gradients
        enabled first. Returns nothing.

        All tensors dense, contiguous and on one GPU; a gradient has its parameter's dtype, float32, bfloat16 or float16.
        ValueError, before any launch, in the order of _step_arguments; NovaHipError for CPU parameters."""
        if closure is not None:
            with torch.enable_grad():
                closure()
        work = self._step_arguments(max_grad_norm)
        self.grad_norm = None
        if not work:
            return
        device = work[0][1].device
        if device.type != "cuda":
            raise hip.NovaHipError("parameter: the fused AdamW runs on the GPU (got a CPU tensor)")
        states = [self._state_of(p) for _, p in work]
        torch._foreach_add_([st["step"] for st in states], 1.0)
        table = (hip.AdamWTensor * len(work))()
        numbers_of = {}
        nonempty = chunks = 0
        for e, (group, p), st in zip(table, work, states):
            key = (id(group), float(st["step"]))  # a CPU scalar: no device work
            if key not in numbers_of:
                numbers_of[key] = step_numbers(group["lr"], group["betas"], group["eps"], group["weight_decay"], key[1])
            master = st.get("master")
            e.param, e.grad, e.exp_avg, e.exp_avg_sq = p.data_ptr(), p.grad.data_ptr(), st["exp_avg"].data_ptr(), st["exp_avg_sq"].data_ptr()
            e.master = master.data_ptr() if master is not None else None
            e.n, e.dtype = p.numel(), hip.dtype_code(p.dtype)
            e.decay, e.w1, e.b2, e.w2, e.q, e.a, e.eps = numbers_of[key]
            nonempty += p.numel() > 0
            chunks += _chunks(p.numel(), ADAMW_CHUNK)
        blocks = _chunks(nonempty, ADAMW_BLOCK)
        with torch.cuda.device(device):
            stream = hip.stream_ptr()
            sumsq = None
            if max_grad_norm is not None:
                # the sum and its square root, both written by the kernel; no chunk: nothing is launched and both are +0
                sumsq, norm = (torch.empty if chunks else torch.zeros)(2, dtype=torch.float32, device=device).unbind(0)
                if self._workspace is None or self._workspace.numel() < chunks or self._workspace.device != device:
                    self._workspace = torch.empty(max(chunks, 1), dtype=torch.float32, device=device)
                hip.call("nova_adamw_sumsq", table, len(work), self._workspace.data_ptr(), self._workspace.numel(), sumsq.data_ptr(), norm.data_ptr(),
                         stream)
                stats["sumsq_calls"] += 1
                stats["sumsq_launches"] += blocks + 1 if chunks else 0
                self.grad_norm = norm
            hip.call("nova_adamw_step", table, len(work), sumsq.data_ptr() if sumsq is not None else None,
                     float(max_grad_norm) if max_grad_norm is not None else 0.0, stream)
            stats["step_calls"] += 1
            stats["step_launches"] += blocks

    def load_state_dict(self, state_dict):
        """torch's loader, then the float32 state (exp_avg, exp_avg_sq, master) taken again from `state_dict` as float32: the
        loader casts every floating state tensor to its parameter's dtype, which for a bfloat16 / float16 parameter would
        round the moments and the master copy. `step` becomes a float32 CPU scalar tensor wherever it was kept. A state
        without `master` (one of torch.optim.AdamW) gets it from the parameter at the next step."""
        super().load_state_dict(state_dict)
        saved_ids = chain.from_iterable(g["params"] for g in state_dict["param_groups"])
        params = chain.from_iterable(g["params"] for g in self.param_groups)
        for k, p in zip(saved_ids, params):
            saved = state_dict["state"].get(k)
            if saved is None:
                continue
            st = self.state[p]
            for key in _FLOAT32_STATE:
                if torch.is_tensor(saved.get(key)):
                    st[key] = saved[key].detach().to(device=p.device, dtype=torch.float32, copy=True).contiguous()
            if "step" in saved:
                st["step"] = torch.as_tensor(saved["step"]).detach().to(device="cpu", dtype=torch.float32, copy=True).reshape(())
