"""The optimizer step on HIP kernels: SGD / Adam / AdamW whose step() never reads the device, with the reference's learning-rate rule evaluated on the device.

    opt = optim.SGD(params, lr=0.01, momentum=0.9, weight_decay=1e-4, lr_schedule=optim.TrainPyLR(0.01))
    scaler.scale(loss).backward(); scaler.step(opt); scaler.update()          # train.py:180-182 unchanged; or opt.step()

Each class subclasses the torch optimizer of its name and overrides step() only: constructor arguments, param_groups, the per-parameter state keys and the
state-dict format are the parent's, so checkpoints move both ways.  One step() is one fd_optim_begin launch (global step, skip flag from GradScaler's found_inf,
the step's learning rates, Adam's bias corrections -- all in the optimizer's own state block on the device) and one update launch per 64 tensors, whose pointers
travel by value in the kernel arguments (include/fcosdet.h "Optimizer step").  Every pointer a launch receives is read from the live tensors inside that step():
gradients are re-allocated by every backward and live elsewhere during a graph capture, so nothing about them is cached.  The step is therefore capture-safe as it
is (train_graph.GraphedStep); run one eager step first, because the state tensors are created by the first step that sees a gradient.

Clipping the global gradient norm is a constructor argument, max_grad_norm=35.0: step() then first enqueues one sum-of-squares launch per 64 gradients and one
finish launch that turns them into the clip coefficient, and the update launches divide every gradient by scale / coefficient instead of by the scale -- one
more read of the gradients, no write to them, no host read.  p.grad is NOT modified: the one difference from torch.nn.utils.clip_grad_norm_.

Averaging the weights (SWA / EMA) is optim.AveragedModel at the end of this file: torch.optim.swa_utils.AveragedModel on the same terms -- no host read, the
optimizer's skip flag honoured, capture-safe.  optim.update_bn(loader, avg) then recomputes the running statistics of the averaged copy's
batch-statistics BatchNorms on the HIP kernels, leaving the frozen ones alone.

What stays stock: torch.amp.GradScaler's own inf check and update().  Moving an optimizer goes through state_dict() / load_state_dict() and
global_step / set_global_step(); pickling or deep-copying the optimizer object itself is not supported (torch's __getstate__ drops the state block).
"""
from __future__ import annotations

import ctypes as C
import math
from typing import NamedTuple, Tuple

import torch
import torch.optim.swa_utils

from . import _lib, ops
from ._lib import FdError


class TrainPyLR(NamedTuple):
    """train.py:160-173 as it is written: while G < warmup_steps the rate is G / warmup_steps * lr_init; at G == a drop step it becomes lr_init * factor; any other
    step keeps the rate of the step before (so steps 501 .. 20000 run at 500/501 * lr_init).  G starts at 1."""
    lr_init: float
    warmup_steps: int = 501
    drops: Tuple[Tuple[int, float], ...] = ((20001, 0.1), (50001, 0.01))
    first_step = 1

    def at(self, step: int, before: float) -> float:
        """The rate the reference's loop holds after the lines of step `step` have run for every G in first_step .. step (closed form; `before`: the rate
        the optimizer was built with).  Used to seed the device scalar when a run resumes at a step (set_global_step)."""
        when, lr = 0, float(before)
        if step >= 1 and self.warmup_steps > 1:
            when = min(step, self.warmup_steps - 1)
            lr = float(when / self.warmup_steps * self.lr_init)
        for at_step, factor in self.drops:
            if at_step <= step and at_step >= max(when, 1):
                when, lr = at_step, self.lr_init * factor
        return lr


class TrainNewLR(NamedTuple):
    """train_new.py:79-90: a function of the step alone.  Below warmup_steps a linear blend from warmup_factor to 1 times lr_init; from there lr_init multiplied
    by gamma once per milestone reached (repeated multiplication, as there).  G starts at 0."""
    lr_init: float
    warmup_steps: int = 500
    warmup_factor: float = 1.0 / 3.0
    milestones: Tuple[int, ...] = (120000, 160000)
    gamma: float = 0.1
    first_step = 0

    def at(self, step: int, before: float) -> float:
        if step < self.first_step:
            return float(before)
        lr = self.lr_init
        if step < self.warmup_steps:
            alpha = float(step) / self.warmup_steps
            lr = lr * (self.warmup_factor * (1.0 - alpha) + alpha)
        else:
            for m in self.milestones:
                if step < m:
                    break
                lr *= self.gamma
        return float(lr)


_WORDS = C.sizeof(_lib.OptimState) // 8
_F = _lib.OptimState
_CLIP = _lib.GradClip


def _word(field) -> int:
    return field.offset // 8


class _HipStep:
    """What the three classes share: the state block, the begin launch, the chunked update launches.  A mixin placed BEFORE the torch optimizer in the bases.

    max_grad_norm (keyword of the three constructors, default None = the step as it is without it): clip the global 2-norm of all gradients of all param groups
    to this value, with torch.nn.utils.clip_grad_norm_'s coefficient min(1, max_norm / (norm + 1e-6)), inside step().  It is an attribute of the optimizer, not
    a param-group key and not part of the state dict.  The gradients themselves are never written (p.grad still holds the unclipped, still scaled values after
    the step); a step whose gradients hold an inf or a NaN is skipped like one GradScaler flags, with or without a scaler.  opt.grad_norm is the unscaled norm of
    the last step as a device scalar.  The value travels by value in the finish launch: changing opt.max_grad_norm after a graph capture does not reach the
    replays -- capture again."""
    _step_supports_amp_scaling = True      # torch.amp.GradScaler then leaves grad_scale / found_inf on the optimizer as device tensors and does not read them
    _ADAM = False

    def _fd_init(self, lr_schedule, max_grad_norm=None) -> None:
        if lr_schedule is not None and not isinstance(lr_schedule, (TrainPyLR, TrainNewLR)):
            raise ValueError("lr_schedule must be an optim.TrainPyLR, an optim.TrainNewLR or None")
        if len(self.param_groups) > _lib.OPTIM_MAX_GROUPS:
            raise ValueError(f"param_groups: {len(self.param_groups)} groups (the device state block holds {_lib.OPTIM_MAX_GROUPS})")
        for name in ("maximize", "differentiable", "amsgrad"):
            if any(g.get(name) for g in self.param_groups):
                raise ValueError(f"{name}=True is not implemented by the HIP optimizer step")
        if any(g.get("dampening", 0) != 0 for g in self.param_groups):
            raise ValueError("dampening != 0 is not implemented by the HIP optimizer step")
        if lr_schedule is not None:
            drops = lr_schedule.drops if isinstance(lr_schedule, TrainPyLR) else lr_schedule.milestones
            if len(drops) > _lib.OPTIM_MAX_DROPS or lr_schedule.warmup_steps < 1:
                raise ValueError(f"lr_schedule: at most {_lib.OPTIM_MAX_DROPS} drops / milestones, warmup_steps >= 1")
        params = [p for g in self.param_groups for p in g["params"]]
        for p in params:
            if p.dtype != torch.float32:
                raise ValueError(f"params: the HIP optimizer step updates fp32 parameters (got {p.dtype}); AMP keeps its parameters in fp32")
            if p.device != params[0].device:
                raise ValueError(f"params: all parameters of one optimizer must live on one device (got {params[0].device} and {p.device})")
            if not p.is_contiguous() and not p.is_contiguous(memory_format=torch.channels_last):
                raise ValueError("params: parameters must be dense (contiguous or channels_last)")
        self._fd_schedule = lr_schedule
        self._fd_device = params[0].device
        # The state block (fd_optim_state): allocated once, so its address is the same in a capture and in its replays.  Viewed as int64 for the counters.
        self._fd_state = torch.zeros(_WORDS, dtype=torch.float64, device=self._fd_device)
        self._fd_state_i = self._fd_state.view(torch.int64)
        first = lr_schedule.first_step if lr_schedule is not None else 1
        self._fd_state_i[_word(_F.global_step)] = first - 1
        self._fd_lr0 = [g["lr"] for g in self.param_groups]
        if lr_schedule is not None:
            for i, g in enumerate(self.param_groups):
                w = _word(_F.lr) + i
                self._fd_state[w] = float(g["lr"])
                g["lr"] = self._fd_state[w]            # 0-dim fp64 view: fd_optim_begin overwrites it, logging reads it with .item()
        self.launches = 0                              # launches of the last step(): begin + updates (+ sum-of-squares + finish with max_grad_norm)
        self._fd_order = {}                            # id(param group) -> its parameters' indices, largest first
        # Clipping: the value travels BY VALUE in the finish launch, so a change after a graph capture does not reach the replays.
        self._fd_clip = None
        if max_grad_norm is not None:
            if isinstance(max_grad_norm, bool) or not isinstance(max_grad_norm, (int, float)) or not math.isfinite(max_grad_norm) or max_grad_norm <= 0:
                raise ValueError(f"max_grad_norm must be a positive finite number or None (got {max_grad_norm!r})")
            max_grad_norm = float(max_grad_norm)
            # The clip block (fd_grad_clip) and the partials for the largest possible chunk count, both allocated once: same addresses in a capture and its replays.
            self._fd_clip = torch.zeros(C.sizeof(_CLIP) // 8, dtype=torch.float64, device=self._fd_device)
            self._fd_clip_f = self._fd_clip.view(torch.float32)
            chunks = -(-len(params) // _lib.OPTIM_MAX_TENSORS)
            self._fd_partials = torch.empty(_lib.lib().fd_grad_norm_workspace_bytes(chunks) // 8, dtype=torch.float64, device=self._fd_device)
        self.max_grad_norm = max_grad_norm

    # ------------------------------------------------------------------ counters
    @property
    def global_step(self) -> torch.Tensor:
        """0-dim int64 device tensor: the step fd_optim_begin evaluated last (the reference's GLOBAL_STEPS)."""
        return self._fd_state_i[_word(_F.global_step)]

    def set_global_step(self, n: int) -> None:
        """The next step() evaluates the learning-rate rule at n + 1 (resuming a run; tests).  With a schedule the rate scalars get what the reference's loop
        would hold after step n, because train.py's rule keeps the previous rate on most steps."""
        self._fd_state_i[_word(_F.global_step)] = int(n)
        if self._fd_schedule is not None:
            for i, lr0 in enumerate(self._fd_lr0):
                self._fd_state[_word(_F.lr) + i] = self._fd_schedule.at(int(n), float(lr0))

    @property
    def grad_norm(self) -> torch.Tensor:
        """0-dim fp32 device tensor, a view of the clip block: the global 2-norm of the UNSCALED gradients of the last step(), before clipping (inf / nan on a
        step that was skipped for a non-finite gradient).  Only with max_grad_norm."""
        if self.max_grad_norm is None:
            raise AttributeError("grad_norm: the optimizer was built without max_grad_norm, its step() does not compute the norm")
        return self._fd_clip_f[_CLIP.total_norm_f32.offset // 4]

    def _applied(self, i: int) -> torch.Tensor:
        return self._fd_state_i[_word(_F.applied) + i]

    # ------------------------------------------------------------------ the step
    def _begin_params(self, active) -> _lib.OptimBeginParams:
        bp = _lib.OptimBeginParams()
        bp.n_groups, bp.adam = len(self.param_groups), int(self._ADAM)
        s = self._fd_schedule
        if isinstance(s, TrainPyLR):
            bp.rule, bp.lr_init, bp.warmup_steps, bp.n_drops = _lib.OPTIM_LR_TRAIN_PY, float(s.lr_init), int(s.warmup_steps), len(s.drops)
            for i, (at_step, factor) in enumerate(s.drops):
                bp.drop_step[i], bp.drop_factor[i] = int(at_step), float(factor)
        elif isinstance(s, TrainNewLR):
            bp.rule, bp.lr_init, bp.warmup_steps, bp.n_drops = _lib.OPTIM_LR_TRAIN_NEW, float(s.lr_init), int(s.warmup_steps), len(s.milestones)
            bp.warmup_factor, bp.gamma = float(s.warmup_factor), float(s.gamma)
            for i, m in enumerate(s.milestones):
                bp.drop_step[i] = int(m)
        else:
            bp.rule = _lib.OPTIM_LR_NONE
        for i, g in enumerate(self.param_groups):
            bp.active[i] = int(active[i])
            lr = g["lr"]
            if s is None:
                if isinstance(lr, torch.Tensor):
                    if lr.device != self._fd_device or lr.numel() != 1 or lr.dtype not in (torch.float32, torch.float64):
                        raise FdError(f"lr: a tensor lr must be one fp32 / fp64 element on {self._fd_device}")
                    bp.lr_ptr[i], bp.lr_ptr_f64[i] = lr.data_ptr(), int(lr.dtype == torch.float64)
                else:
                    bp.lr_value[i] = float(lr)
            if self._ADAM:
                b1, b2 = g["betas"]
                if isinstance(b1, torch.Tensor) or isinstance(b2, torch.Tensor):
                    raise FdError("betas: tensor betas are not implemented by the HIP optimizer step")
                bp.beta1[i], bp.beta2[i] = float(b1), float(b2)
        return bp

    def _state_names(self, group) -> Tuple[str, ...]:
        raise NotImplementedError

    def _hyper(self, i: int, group) -> _lib.OptimHyper:
        raise NotImplementedError

    def _gather(self, group):
        """The live tensors of one group: (params, p / g / state address lists, numels).  Parameters without a gradient are left out and their state is
        not touched; state tensors are created (zeros) for a parameter the first time it arrives with a gradient, as the parent does."""
        names = self._state_names(group)
        ps, pp, gp, sp, ne = [], [], [], [[] for _ in names], []
        # Largest first, so that the tensors of a chunk are of similar size: a launch's grid follows its largest tensor, and a block past a shorter
        # tensor's end only exits.  The ORDER is remembered (shapes do not change); every address below is read now.
        order = self._fd_order.get(id(group))
        if order is None or len(order) != len(group["params"]):
            order = self._fd_order[id(group)] = sorted(range(len(group["params"])), key=lambda k: -group["params"][k].numel())
        for k in order:
            p = group["params"][k]
            g = p.grad
            if g is None:
                continue
            if not p.is_cuda:
                raise FdError("pytorch_object_detection_amd runs on the GPU only (got a CPU parameter); there is no CPU fallback")
            if g.is_sparse or g.layout != torch.strided:
                raise FdError("grad: sparse gradients are not implemented by the HIP optimizer step")
            if g.dtype != torch.float32 or g.device != p.device:
                raise FdError(f"grad: the HIP optimizer step takes fp32 gradients on the parameter's device (got {g.dtype} on {g.device})")
            if g.stride() != p.stride() or not (g.is_contiguous() or g.is_contiguous(memory_format=torch.channels_last)):
                raise FdError(f"grad: a gradient must be dense in its parameter's layout (shape {tuple(g.shape)}, strides {g.stride()} against {p.stride()})")
            st = self.state[p]
            for k, name in enumerate(names):
                s = st.get(name)
                if s is None:
                    if torch.cuda.is_current_stream_capturing():
                        raise FdError(f"{name}: the optimizer state would be created inside a graph capture and zeroed by every replay; run one eager step first")
                    s = st[name] = torch.zeros_like(p, memory_format=torch.preserve_format)
                elif s.dtype != torch.float32 or s.device != p.device or s.stride() != p.stride():
                    raise FdError(f"{name}: state must be fp32 on the parameter's device and in its layout")
                sp[k].append(s.data_ptr())
            ps.append(p)
            pp.append(p.data_ptr())
            gp.append(g.data_ptr())
            ne.append(p.numel())
        return ps, pp, gp, sp, ne

    @torch.no_grad()
    def step(self, closure=None):
        loss = None
        if self._fd_device.type != "cuda":
            raise FdError("pytorch_object_detection_amd runs on the GPU only (got CPU parameters); there is no CPU fallback")
        if closure is not None:
            with torch.enable_grad():
                loss = closure()
        grad_scale, found_inf = getattr(self, "grad_scale", None), getattr(self, "found_inf", None)
        gathered = [self._gather(g) for g in self.param_groups]
        with torch.cuda.device(self._fd_device):
            launches = 0
            if self.max_grad_norm is not None:
                if self._fd_clip is None:
                    raise FdError("max_grad_norm: the optimizer was built without it; pass it to the constructor, which allocates the clip block")
                # one global norm over every group's live gradients; from here on the step's scale and skip flag are the clip block's
                n, slots = ops.grad_sumsq([a for t in gathered for a in t[2]], [k for t in gathered for k in t[4]], self._fd_partials)
                ops.grad_clip_finish(self._fd_partials, slots, grad_scale, found_inf, self.max_grad_norm, self._fd_clip)
                launches = n + 1
                grad_scale, found_inf = self._fd_clip_f[_CLIP.eff_scale.offset // 4], self._fd_clip_f[_CLIP.found.offset // 4]
            ops.optim_begin(self._fd_state, found_inf, self._begin_params([bool(t[0]) for t in gathered]))
            launches, touched = launches + 1, []
            for i, (group, (ps, pp, gp, sp, ne)) in enumerate(zip(self.param_groups, gathered)):
                if not ps:
                    continue
                launches += ops.optim_update(self._ADAM, pp, gp, sp[0] if len(sp) > 0 else None, sp[1] if len(sp) > 1 else None, ne,
                                             self._hyper(i, group), self._fd_state, grad_scale)
                touched += ps
        self.launches = launches
        if touched:
            torch.autograd.graph.increment_version(touched)      # host only: code that keys on _version sees the update
        return loss


class SGD(_HipStep, torch.optim.SGD):
    """torch.optim.SGD (dampening 0) on fd_optim_sgd_f32.  State key: momentum_buffer (only with momentum != 0), starting as zeros -- with dampening 0 that is
    torch's 'the first step copies the gradient'."""

    def __init__(self, params, *args, lr_schedule=None, max_grad_norm=None, **kwargs):
        super().__init__(params, *args, **kwargs)
        self._fd_init(lr_schedule, max_grad_norm)

    def _state_names(self, group):
        return ("momentum_buffer",) if group["momentum"] != 0 else ()

    def _hyper(self, i, group):
        h = _lib.OptimHyper()
        h.group, h.nesterov, h.momentum, h.weight_decay = i, int(bool(group["nesterov"])), float(group["momentum"]), float(group["weight_decay"])
        return h

    def load_state_dict(self, state_dict):
        super().load_state_dict(state_dict)
        _rebind_lr(self)
        for st in self.state.values():                     # torch.optim.SGD keeps None for a parameter it has not stepped yet
            if st.get("momentum_buffer", 0) is None:
                del st["momentum_buffer"]

    def state_dict(self):
        return _detached_lr(self, super().state_dict())


class Adam(_HipStep, torch.optim.Adam):
    """torch.optim.Adam (no AMSGrad) on fd_optim_adam_f32.  State keys: exp_avg, exp_avg_sq and, in state_dict() only, step: the applied-step count lives once
    per param group on the device (it does not advance on a step GradScaler skips, as in torch's fused Adam); state_dict() reads it and writes it into every
    parameter's entry, load_state_dict() takes it back and refuses a group whose entries disagree."""
    _ADAM = True

    def __init__(self, params, *args, lr_schedule=None, max_grad_norm=None, **kwargs):
        super().__init__(params, *args, **kwargs)
        self._fd_init(lr_schedule, max_grad_norm)

    def _state_names(self, group):
        return ("exp_avg", "exp_avg_sq")

    def _hyper(self, i, group):
        h = _lib.OptimHyper()
        h.group, h.decoupled_wd, h.weight_decay, h.eps = i, int(bool(group.get("decoupled_weight_decay", False))), float(group["weight_decay"]), float(group["eps"])
        h.beta1, h.beta2 = float(group["betas"][0]), float(group["betas"][1])
        return h

    def state_dict(self):
        sd = _detached_lr(self, super().state_dict())
        counts = self._fd_state_i[_word(_F.applied):_word(_F.applied) + len(self.param_groups)].tolist()       # the one host read
        for gi, g in enumerate(sd["param_groups"]):
            for idx in g["params"]:
                if idx in sd["state"]:
                    sd["state"][idx] = dict(sd["state"][idx], step=torch.tensor(float(counts[gi]), dtype=torch.float32))
        return sd

    def load_state_dict(self, state_dict):
        super().load_state_dict(state_dict)
        _rebind_lr(self)
        for gi, g in enumerate(self.param_groups):
            steps = set()
            for p in g["params"]:
                st = self.state.get(p)
                if st and "step" in st:
                    steps.add(float(st.pop("step")))
            if len(steps) > 1:
                raise ValueError(f"step: the parameters of param group {gi} carry different step counts {sorted(steps)}; the HIP Adam keeps one per group")
            self._fd_state_i[_word(_F.applied) + gi] = int(steps.pop()) if steps else 0


class AdamW(Adam, torch.optim.AdamW):
    """torch.optim.AdamW: Adam with decoupled weight decay (p *= 1 - lr * wd before the update)."""


def _detached_lr(opt: _HipStep, sd: dict) -> dict:
    """A scheduled lr is a view of the state block: a state dict gets its value as a tensor of its own."""
    if opt._fd_schedule is not None:
        sd["param_groups"] = [dict(g, lr=g["lr"].clone()) if isinstance(g["lr"], torch.Tensor) else g for g in sd["param_groups"]]
    return sd


def _rebind_lr(opt: _HipStep) -> None:
    """After a load: a scheduled lr is again the view fd_optim_begin writes, holding the loaded value."""
    if opt._fd_schedule is None:
        return
    for i, g in enumerate(opt.param_groups):
        w = _word(_F.lr) + i
        view = opt._fd_state[w]
        if g["lr"] is not view:
            view.copy_(torch.as_tensor(g["lr"], dtype=torch.float64))
            g["lr"] = view


_AVG_WORDS = C.sizeof(_lib.AvgState) // 8


def _dense(t: torch.Tensor) -> bool:
    return t.layout == torch.strided and (t.is_contiguous() or (t.dim() == 4 and t.is_contiguous(memory_format=torch.channels_last)))


class AveragedModel(torch.optim.swa_utils.AveragedModel):
    """torch.optim.swa_utils.AveragedModel whose update_parameters() never reads the device (include/fcosdet.h "Averaging the model's weights").

        avg = optim.AveragedModel(model, decay=0.999, optimizer=opt)            # EMA; decay=None: SWA, the equal average of the parent's default
        scaler.step(opt); scaler.update(); avg.update_parameters(model)         # after the optimizer's step; evaluate avg.module

    .module (a deep copy of the model), .n_averaged (registered 0-dim int64 buffer), .use_buffers, forward and the state-dict keys (n_averaged + module.*) are
    the parent's, so checkpoints move both ways.  One difference: n_averaged is created on the device of the copy's parameters (the parent leaves it on the CPU
    unless device= is given), because the begin launch increments it.

    One update is one fd_avg_begin launch (the gate, this call's blend factor, n_averaged += 1), one fd_avg_update_f32 launch per 64 averaged fp32 tensors
    (avg = avg + (p - avg) * w in fp32; the first applied update copies) and one fd_avg_copy_bytes launch per 64 copied buffers; every address is read from the
    live tensors inside the call and travels by value in the kernel arguments, so the call can be recorded into a HIP graph with the optimizer's step.

    decay=None: weight 1 / (n_averaged + 1) (get_swa_multi_avg_fn); decay=d in [0, 1]: weight 1 - d (get_ema_multi_avg_fn(d)).  A callable avg_fn / multi_avg_fn
    is refused: Python cannot run inside the launch.
    optimizer=: one of this module's SGD / Adam / AdamW.  The begin launch then reads that optimizer's skip flag and global step on the device: a step that
    GradScaler or clipping skipped leaves the average and n_averaged untouched, and start_step / every gate the update (it applies when
    global_step >= start_step and (global_step - start_step) % every == 0 -- SWA from step N, every k steps).  The gate compares against the step the optimizer
    evaluated LAST, so call update_parameters() after opt.step() / scaler.step(opt).  Without optimizer every call averages, as in the parent.
    decay, start_step and every travel by value in the begin launch: changing them after a graph capture does not reach the replays -- capture again.

    Buffers: use_buffers=False (default) copies every buffer from the model on every applied call; use_buffers=True averages the floating buffers with the
    parameters and COPIES the integer ones (BatchNorm's num_batches_tracked).  The parent pushes integer buffers through a truncating blend, an accident of
    its non-floating fallback branch; that is not followed.

    Refused: non-fp32 floating tensors, pairs whose shapes / strides / devices differ, non-dense tensors, CPU tensors (there is no CPU fallback), a model with
    more tensors than the copy.  The copy's batch-statistics BatchNorms get statistics that belong to the averaged weights from update_bn(loader, avg) below.
    Not here: SWALR, a decay warm-up, averaging in fp64.  Moving an averaged model goes through state_dict() /
    load_state_dict(); with optimizer= the object itself can be neither pickled nor deep-copied, as the optimizer cannot."""

    def __init__(self, model, device=None, avg_fn=None, multi_avg_fn=None, use_buffers=False, *, decay=None, optimizer=None, start_step=0, every=1):
        for name, fn in (("avg_fn", avg_fn), ("multi_avg_fn", multi_avg_fn)):
            if fn is not None:
                raise ValueError(f"{name}: a Python callable cannot run inside the launch; pass decay= (EMA) or leave it None (SWA, the equal average)")
        if decay is not None:
            if isinstance(decay, bool) or not isinstance(decay, (int, float)) or not math.isfinite(decay) or not 0.0 <= decay <= 1.0:
                raise ValueError(f"decay must be a number in [0, 1] or None (got {decay!r})")
            decay = float(decay)
        if optimizer is not None and not isinstance(optimizer, _HipStep):
            raise ValueError(f"optimizer must be one of this module's SGD / Adam / AdamW (got {type(optimizer).__name__}): the gate reads its device state block")
        for name, v, lo in (("start_step", start_step, None), ("every", every, 1)):
            if isinstance(v, bool) or not isinstance(v, int) or (lo is not None and v < lo):
                raise ValueError(f"{name} must be an integer" + (f" >= {lo}" if lo is not None else "") + f" (got {v!r})")
        if optimizer is None and (start_step != 0 or every != 1):
            raise ValueError("start_step / every gate on an optimizer's global step: pass optimizer= as well")
        super().__init__(model, device, None, None, use_buffers)
        self.decay, self.start_step, self.every = decay, int(start_step), int(every)
        self._fd_opt = [optimizer]                         # in a list: not a sub-module, not part of the state dict
        first = next(iter(self.module.parameters()), None)
        if device is None and first is not None:
            self.n_averaged = self.n_averaged.to(first.device)
        self._fd_state = None                              # fd_avg_state on n_averaged's device, allocated by the first update
        self._fd_order = None
        self.launches = 0                                  # launches of the last update_parameters(): begin + updates + copies

    def _begin_params(self) -> _lib.AvgBeginParams:
        bp = _lib.AvgBeginParams()
        bp.mode, bp.decay = (_lib.AVG_SWA, 0.0) if self.decay is None else (_lib.AVG_EMA, float(self.decay))
        bp.start_step, bp.every = int(self.start_step), int(self.every)
        return bp

    def _pairs(self, model):
        """The live tensors of one update: (averaged pairs, copied pairs), each a list of (copy's tensor, model's tensor) in the parent's pairing."""
        mine_p, theirs_p = list(self.module.parameters()), list(model.parameters())
        mine_b, theirs_b = list(self.module.buffers()), list(model.buffers())
        if len(theirs_p) > len(mine_p) or len(theirs_b) != len(mine_b):
            raise ValueError(f"model: {len(theirs_p)} parameters / {len(theirs_b)} buffers against {len(mine_p)} / {len(mine_b)} on the averaged copy")
        averaged, copied = list(zip(mine_p, theirs_p)), []
        for a, b in zip(mine_b, theirs_b):
            (averaged if self.use_buffers and a.is_floating_point() else copied).append((a, b))
        dev = self.n_averaged.device
        for kind, pairs in (("averaged", averaged), ("copied", copied)):
            for a, b in pairs:
                if not a.is_cuda or not b.is_cuda:
                    raise FdError("model: pytorch_object_detection_amd runs on the GPU only (got a CPU tensor); there is no CPU fallback")
                if a.device != dev or b.device != dev:
                    raise ValueError(f"model: every tensor must live on n_averaged's device {dev} (got {a.device} and {b.device})")
                if kind == "averaged" and (a.dtype != torch.float32 or b.dtype != torch.float32):
                    raise ValueError(f"model: the averaging kernel takes fp32 tensors (got {a.dtype} and {b.dtype}, shape {tuple(a.shape)})")
                if a.dtype != b.dtype or a.shape != b.shape or a.stride() != b.stride():
                    raise ValueError(f"model: a pair differs in dtype / shape / strides ({a.dtype} {tuple(a.shape)} {a.stride()} against "
                                     f"{b.dtype} {tuple(b.shape)} {b.stride()})")
                if not _dense(a) or not _dense(b):
                    raise ValueError(f"model: tensors must be dense (contiguous or channels_last; shape {tuple(a.shape)}, strides {a.stride()})")
        return averaged, copied

    @torch.no_grad()
    def update_parameters(self, model) -> None:
        n = self.n_averaged                                # the live buffer: .to() / load_state_dict may have moved it
        averaged, copied = self._pairs(model)
        if not n.is_cuda:
            raise FdError("n_averaged: pytorch_object_detection_amd runs on the GPU only (the averaged model is on the CPU); there is no CPU fallback")
        if self._fd_state is None or self._fd_state.device != n.device:
            if torch.cuda.is_current_stream_capturing():
                raise FdError("update_parameters: the state block would be allocated inside a graph capture; run one eager update first")
            self._fd_state = torch.zeros(_AVG_WORDS, dtype=torch.float64, device=n.device)
        # Largest first, so that the tensors of a launch are of similar size (its grid follows the largest).  The ORDER is remembered; every address is read now.
        sig = (len(averaged), len(copied))
        if self._fd_order is None or self._fd_order[0] != sig:
            self._fd_order = (sig, sorted(range(len(averaged)), key=lambda k: -averaged[k][0].numel()),
                              sorted(range(len(copied)), key=lambda k: -copied[k][0].numel() * copied[k][0].element_size()))
        averaged, copied = [averaged[k] for k in self._fd_order[1]], [copied[k] for k in self._fd_order[2]]
        opt = self._fd_opt[0]
        skip = opt._fd_state_i[_word(_F.skip)] if opt is not None else None
        step = opt._fd_state_i[_word(_F.global_step)] if opt is not None else None
        with torch.cuda.device(n.device):
            ops.avg_begin(self._fd_state, n, skip, step, self._begin_params())
            launches = 1
            if averaged:
                launches += ops.avg_update([a.data_ptr() for a, _ in averaged], [b.data_ptr() for _, b in averaged], [a.numel() for a, _ in averaged],
                                           self._fd_state)
            if copied:
                launches += ops.avg_copy([a.data_ptr() for a, _ in copied], [b.data_ptr() for _, b in copied],
                                         [a.numel() * a.element_size() for a, _ in copied], self._fd_state)
        self.launches = launches
        # host only: the averaged module's plans and folded BatchNorms key on _version and re-pack on its next forward
        torch.autograd.graph.increment_version([n] + [a for a, _ in averaged] + [a for a, _ in copied])


def update_bn(loader, model, device=None) -> None:
    """torch.optim.swa_utils.update_bn for this project's models: recompute the running statistics of the BatchNorms that run on BATCH statistics as the equal
    average over `loader`.  Same signature and batch conventions: a batch is a tensor, or a list / tuple whose first element is the input, moved
    to `device` when one is given.  The main use is the averaged copy, whose weights are averaged but whose running statistics are only copied:

        optim.update_bn(loader, avg)                  # avg = optim.AveragedModel(...); also a bare detector or a DistributedDataParallel wrapper

    It runs under torch.no_grad() in fp32 and never reads the device.  Three differences from the stock function:
      * it records model.training, calls model.train(), and THEN resets (device fills) and sets momentum = None on only the BatchNorms for which
        `training and track_running_stats` holds -- the set that will run on batch statistics.  What train() keeps in eval mode (the backbone the constructor
        froze, everything under freeze_all_bn, a stem enable_training() froze) keeps its statistics bit for bit; the stock function resets those to 0 / 1
        and never recomputes them.  An empty set returns with the mode restored.
      * momentum = None stays on the HIP batch-statistics kernels: they read num_batches_tracked on the device and blend with 1 / n (the `_cma` entry
        points), at the launches of an ordinary train-mode forward, and the forward can be captured.
      * momenta and model.train(was_training) are restored in a finally:, and every running tensor it wrote has its version counter bumped (HIP launches do
        not bump them), so folded BatchNorms and plans re-pack on the next eval forward.
    Under nn.SyncBatchNorm on more than one rank every rank passes its own shard: the statistics are global and all ranks end with identical buffers."""
    with torch.no_grad():
        was_training = model.training
        model.train()
        momenta = {}
        try:
            # (a trunk names the layers it keeps on their running statistics whatever .training says: the EfficientNet stem without train_stem)
            kept = {id(b) for m in model.modules() if hasattr(m, "bn_on_running_stats") for b in m.bn_on_running_stats()}
            for m in model.modules():
                if isinstance(m, torch.nn.modules.batchnorm._BatchNorm) and m.training and m.track_running_stats and id(m) not in kept:
                    momenta[m] = m.momentum
            if not momenta:
                return
            for m in momenta:
                m.running_mean.zero_()
                m.running_var.fill_(1)
                if m.num_batches_tracked is not None:
                    m.num_batches_tracked.zero_()
                m.momentum = None
            for batch in loader:
                if isinstance(batch, (list, tuple)):
                    batch = batch[0]
                if device is not None:
                    batch = batch.to(device)
                model(batch)
        finally:
            for m, momentum in momenta.items():
                m.momentum = momentum
            model.train(was_training)
            written = [t for m in momenta for t in (m.running_mean, m.running_var, m.num_batches_tracked) if t is not None]
            if written:
                torch.autograd.graph.increment_version(written)
