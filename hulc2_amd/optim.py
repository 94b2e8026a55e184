"""hulc2_amd.optim.Adam / AdamW / SGD — torch.optim's classes for a model whose parameters live in the fp32 arena of hulc2_amd's weight keeper.

reference: hulc2/models/hulc2.py:185-198 (`configure_optimizers` instantiates `optimizer._target_`, conf/model/optimizer/adam.yaml:
`torch.optim.Adam`, lr 2e-4; adamw.yaml: `torch.optim.AdamW`, weight_decay 1e-6; sgd.yaml: `torch.optim.SGD`, momentum 0.9).  Swapping that
one class path keeps the update rule, the hyper-parameters and the `state_dict()` layout
(per parameter `step` / `exp_avg` / `exp_avg_sq`, or `momentum_buffer`: a Lightning checkpoint of either optimizer loads into the other) and replaces the step
itself: torch's multi-tensor Adam walks 212 tensors (~1.5 ms of host time per step, the largest single item of the eager loop's host
budget, tools/eager_profile.py) and leaves the kernel-side weight copies stale, so the keeper re-derives them before the next forward
(five launches over the whole arena); here ONE launch of the arena kernel of the rule (hulc_adam_step* / hulc_adamw_step / hulc_sgd_step)
updates parameters and optimizer state and writes the bf16 shadow
and the split operands' remainders, two more derive the transposed / repacked copies — exactly what ArenaTrainer.optimizer_step launches.
The gradients are read where the step node left them (hulc2_amd/stepnode.py: the keeper's gradient arena, `p.grad` = its views); a
gradient that lives elsewhere is copied into its slice first (one `_foreach_copy_`).

Under `torch.amp.GradScaler` (the reference trains with `precision: 16`, conf/trainer/play_trainer.yaml:3) the optimizer declares
`_step_supports_amp_scaling`: `scaler.step(optimizer)` then hands over its device scalars (`grad_scale`, `found_inf`) instead of
synchronising on `found_inf.item()`, and the kernel applies them itself — gradients multiplied by 1 / scale, the whole step skipped
(parameters, state, step count) when an inf / NaN was found, as torch's fused Adam does.  The host never waits for the GPU inside a step.

Whenever the fused form does not apply — parameters not (yet) in an arena, a parameter that has state and no gradient, a parameter whose
FIRST gradient arrives after the others have stepped (torch starts its step count at 1 then), amsgrad / maximize / Adam's decoupled weight
decay / `fused=True`, several parameter groups, CPU — `step()` is the torch parent's step(), on the same state tensors.  Parameters that
have NEVER had a gradient are left alone by AdamW and SGD through the kernels' skip ranges (torch skips them, decay included); Adam, whose
kernel has none, takes torch's step when such parameters meet a weight decay.

Gradient clipping (`max_grad_norm=` / `clip_grad_value=` at construction, `set_grad_clip()` later, Lightning's `gradient_clip_val` through
Hulc2.configure_gradient_clipping) happens INSIDE the fused step: one norm pass over the gradient arena (hulc_grad_norm_clip, under a
GradScaler with its scale as the pass's loss scale), then the step kernel multiplies — or, by value, clamps — every gradient in registers.
The clipped gradient exists only there: `.grad` is left UNCLIPPED (and, under a GradScaler, still scaled) after a fused `step()`, where
`clip_grad_norm_` would have rewritten it.  A step that falls back to torch's path clips with torch's own functions, `.grad` included."""
import importlib
from typing import Callable, Optional, Tuple

import torch

from . import kernels as kn
from .arena import MAX_KERNEL_RANGES, arena_of
from .compat import instantiate

CONSTANT_SCHEDULE = "transformers.get_constant_schedule"


def resolve_warmup(num_training_steps: int, num_warmup_steps, inferred_steps: Callable[[], int]) -> Tuple[int, int]:
    """Hulc2.compute_warmup's rule (reference: hulc2/models/hulc2.py:164-183) for any caller that knows the length of the run: a negative
    num_training_steps is replaced by inferred_steps(), a float num_warmup_steps is a fraction of the training steps, cut to an int."""
    if num_training_steps < 0:
        num_training_steps = int(inferred_steps())
    if isinstance(num_warmup_steps, float):
        num_warmup_steps = num_warmup_steps * num_training_steps
    return num_training_steps, int(num_warmup_steps)


def make_lr_scheduler(cfg, optimizer):
    """The configured `lr_scheduler._target_` on `optimizer` (reference: hulc2.py:194, conf/model/lr_scheduler/*.yaml: three
    transformers.get_*_schedule* functions, each a LambdaLR).  Without an importable target only the constant schedule has a stand-in
    (LambdaLR with factor 1.0, the same numbers); any other target raises — a warm-up / decay config never trains at a constant rate."""
    tgt = cfg.get("_target_") if hasattr(cfg, "get") else None
    if not tgt:
        raise ValueError("lr_scheduler config without a _target_")
    try:
        importlib.import_module(tgt.rpartition(".")[0])
    except ImportError as e:
        if tgt == CONSTANT_SCHEDULE:
            return torch.optim.lr_scheduler.LambdaLR(optimizer, lambda _: 1.0)
        raise ImportError(f"lr_scheduler target {tgt!r} cannot be imported ({e}); only {CONSTANT_SCHEDULE} has a built-in stand-in") from e
    return instantiate(cfg, optimizer)


def lr_lambda_from_config(cfg, num_training_steps: Optional[int] = None) -> Callable[[int], float]:
    """The factor function of an `lr_scheduler` config for ArenaTrainer.set_lr_schedule: the configured target is instantiated on a
    throw-away one-parameter optimizer and its `lr_lambdas[0]` handed back — the reference's own Python function, not a copy of it.
    num_training_steps: the length of the run, used where the config says -1 (Lightning's estimated_stepping_batches in the reference)."""
    cfg = dict(cfg)
    if "num_warmup_steps" in cfg:
        def inferred():
            if num_training_steps is None:
                raise ValueError("lr_scheduler.num_training_steps < 0 needs num_training_steps")
            return num_training_steps
        cfg["num_training_steps"], cfg["num_warmup_steps"] = resolve_warmup(cfg["num_training_steps"], cfg["num_warmup_steps"], inferred)
    sched = make_lr_scheduler(cfg, torch.optim.SGD([torch.nn.Parameter(torch.zeros(1))], lr=1.0))
    lambdas = getattr(sched, "lr_lambdas", None)
    if not lambdas:
        raise TypeError(f"lr_scheduler target {cfg.get('_target_')!r} is not a LambdaLR: no lr_lambdas to take the factor from")
    return lambdas[0]


def trainer_kwargs_from_config(cfg) -> dict:
    """ArenaTrainer keyword arguments for an `optimizer` config (conf/model/optimizer/{adam,adamw,sgd}.yaml: `_target_` torch.optim.Adam,
    AdamW or SGD), torch's defaults filled in for the keys the config leaves out (AdamW's weight_decay is 1e-2, Adam's and SGD's 0)."""
    cfg = dict(cfg)
    tgt = cfg.pop("_target_", None)
    kinds = {"torch.optim.Adam": "adam", "torch.optim.AdamW": "adamw", "torch.optim.SGD": "sgd"}
    if tgt not in kinds:
        raise NotImplementedError(f"optimizer target {tgt!r}: the arena trainer has torch.optim.Adam, AdamW and SGD")
    kind = kinds[tgt]
    cfg = {k: v for k, v in cfg.items() if not str(k).startswith("_")}
    if cfg.pop("amsgrad", False) or cfg.pop("maximize", False):
        raise NotImplementedError("amsgrad / maximize are not built into the arena optimizer kernels")
    for k in ("foreach", "fused", "capturable", "differentiable"):       # (how torch runs its own step: nothing of the update rule)
        cfg.pop(k, None)
    out = {"optimizer": kind, "lr": float(cfg.pop("lr", 1e-3))}
    if kind == "sgd":
        out.update(momentum=float(cfg.pop("momentum", 0.0)), dampening=float(cfg.pop("dampening", 0.0)),
                   nesterov=bool(cfg.pop("nesterov", False)), weight_decay=float(cfg.pop("weight_decay", 0.0)))
    else:
        if kind == "adam" and cfg.pop("decoupled_weight_decay", False):
            out["optimizer"] = kind = "adamw"                            # (torch.optim.AdamW IS Adam with this flag)
        cfg.pop("decoupled_weight_decay", None)
        out.update(betas=tuple(float(b) for b in cfg.pop("betas", (0.9, 0.999))), eps=float(cfg.pop("eps", 1e-8)),
                   weight_decay=float(cfg.pop("weight_decay", 1e-2 if kind == "adamw" else 0.0)))
    # the drop-in optimizers' clipping keys (hulc2_amd.optim.Adam(max_grad_norm=... / clip_grad_value=...)) are the trainer's two arguments
    norm, value = cfg.pop("max_grad_norm", None), cfg.pop("clip_grad_value", None)
    if norm and value:
        raise ValueError("optimizer config: max_grad_norm and clip_grad_value exclude each other")
    if norm or value:
        out.update(gradient_clip_val=float(norm or value), gradient_clip_algorithm="norm" if norm else "value")
    if cfg:
        raise NotImplementedError(f"optimizer config keys {sorted(cfg)} are not known to the arena trainer")
    return out


class _ArenaStep:
    """What the drop-in optimizers share, mixed in IN FRONT of the torch class: the arena binding (state tensors re-homed into flat arenas
    at the parameters' offsets), the gradient-arena views, the one-fill zero_grad, the GradScaler device scalars, the device step count and
    every rule by which a step goes to the torch parent instead.  A subclass names its arena-resident state (_state_names), says which group
    flags it does not cover (_uncovered), whether torch keeps a per-parameter `step` (_counts_steps), whether its kernel takes skip ranges
    (_skips) and launches the pass (_launch)."""
    _counts_steps = True
    _skips = False

    def _arena_init(self) -> None:
        self._arena = None           # (tr, flat_g, grad views, *state arenas) once the parameters are found in a keeper's arena
        self._live, self._mv = set(), ()
        self._bound_names = None
        self._fused_steps = 0        # the step count of the fused path as the HOST knows it (a GradScaler may skip steps on the device: _steps())
        self._dev_steps = None       # device words {unused, step count}: the kernel's bias correction reads the count from here
        self._skippable = False      # a GradScaler's found_inf has been handed in since the host count was last read back
        self.fused_launches = 0      # (tests / logging: steps taken by the fused path)
        self._clip_out = None        # device {gradient norm, clip coefficient} of the fused path's last norm pass
        # torch.amp.GradScaler.step: hand `grad_scale` / `found_inf` over as attributes instead of unscaling and synchronising itself
        self._step_supports_amp_scaling = True

    def _state_names(self, g) -> tuple:
        raise NotImplementedError

    def _uncovered(self, g) -> bool:
        raise NotImplementedError

    # ---- gradient clipping -------------------------------------------------------------------------------------------------------------
    @staticmethod
    def _clip_defaults(kw: dict) -> Tuple[Optional[float], Optional[float]]:
        """take max_grad_norm / clip_grad_value out of a constructor's keyword arguments (torch's __init__ knows neither)"""
        return kw.pop("max_grad_norm", None), kw.pop("clip_grad_value", None)

    def set_grad_clip(self, max_norm: Optional[float] = None, value: Optional[float] = None) -> None:
        """Clip the gradients of every following step: by their global L2 norm (torch.nn.utils.clip_grad_norm_(params, max_norm)) or by value
        (clip_grad_value_(params, value)); None / 0 for both switches clipping off.  Stored as `max_grad_norm` / `clip_grad_value` in every
        param group (the key is absent while that form is off: the groups of an unclipped optimizer are torch's own), so the setting travels in
        state_dict()["param_groups"] and comes back with load_state_dict().  One threshold for all parameters: the norm is global."""
        for name, x in (("max_norm", max_norm), ("value", value)):
            if x is not None and not (0.0 <= float(x) < float("inf")):
                raise ValueError(f"set_grad_clip: {name} must be finite and >= 0 (0 / None: off), got {x!r}")
        if max_norm and value:
            raise ValueError("set_grad_clip: clip by norm or by value, not both")
        for g in self.param_groups:
            for key, x in (("max_grad_norm", max_norm), ("clip_grad_value", value)):
                if x:
                    g[key] = float(x)
                else:
                    g.pop(key, None)

    def _clip_kwargs(self, tr, flat_g, g, grad_scale) -> dict:
        """the fused step's clipping: the norm pass (by norm) and the step kernel's clipping arguments"""
        if g.get("clip_grad_value"):
            return {"clip_value": float(g["clip_grad_value"])}
        if not g.get("max_grad_norm"):
            return {}
        if self._clip_out is None or self._clip_out.device != tr.dev:
            self._clip_out = torch.zeros(2, dtype=torch.float32, device=tr.dev)     # {norm of the unscaled gradients, clip coefficient}
        kn.grad_norm_clip(flat_g, tr.total, 1.0, grad_scale, float(g["max_grad_norm"]), self._clip_out)
        return {"clip_coef_dev": self._clip_out[1:2]}

    def _torch_clip(self) -> None:
        """the same clipping on torch's path, by torch's own functions on the (unscaled) `.grad`s"""
        g0 = self.param_groups[0]
        ps = [p for g in self.param_groups for p in g["params"] if p.grad is not None]
        if ps and g0.get("max_grad_norm"):
            torch.nn.utils.clip_grad_norm_(ps, float(g0["max_grad_norm"]))
        elif ps and g0.get("clip_grad_value"):
            torch.nn.utils.clip_grad_value_(ps, float(g0["clip_grad_value"]))

    def _launch(self, tr, flat_g, arenas, g, grad_scale, found_inf, skip_ranges, clip) -> None:
        raise NotImplementedError

    # ---- arena binding -----------------------------------------------------------------------------------------------------------------
    def _release(self) -> None:
        """leave the arenas: the fused step count goes back into the per-parameter `step` tensors FIRST (torch's path and a later re-bind
        read them), the moments stay where they are (state entries hold the views)"""
        if self._arena is not None:
            self._sync_steps()
            self._arena = None

    def _bind(self) -> Optional[tuple]:
        if len(self.param_groups) != 1:
            self._release()
            return None
        g = self.param_groups[0]
        if g.get("maximize") or g.get("differentiable") or g.get("fused") or self._uncovered(g):
            self._release()
            return None
        params = [p for p in g["params"] if p.requires_grad]     # (frozen parameters never get a gradient: torch skips them, the arena does not hold them)
        tr = arena_of(params)
        if tr is None:
            self._release()
            return None
        names = self._state_names(g)
        if self._arena is not None and self._arena[0] is tr and self._bound_names == names:
            return self._arena
        self._release()                                           # (another arena took the parameters over: the old one's step count is written back)
        mark = names[0] if names else None                        # the state entry that says "this parameter has stepped"
        steps = []
        for p in tr.params:
            st = self.state.get(p)
            if st is not None and mark in st:
                steps.append(int(float(st["step"])) if self._counts_steps else 1)
        if steps and min(steps) != max(steps):
            # parameters with different histories: torch's per-tensor path.  Remembered by the histories themselves, so that the (arena-sized)
            # re-homing below is not attempted again on every step while nothing has changed
            return None
        dev, total = tr.dev, tr.total
        # gradients: the keeper's own gradient arena when it has one (the step node writes them there: no copy), else a buffer of this optimizer
        flat_g = tr.flat_g if tr.flat_g.numel() == total else torch.zeros(total, dtype=torch.float32, device=dev)
        arenas = [torch.zeros(total, dtype=torch.float32, device=dev) for _ in names]
        views, sviews = [], [[] for _ in names]
        self._live = set()                                        # indices (arena order) of the parameters that have had a gradient = have state, as in torch
        with torch.no_grad():
            for i, (p, off) in enumerate(zip(tr.params, tr.offsets)):
                n = p.numel()
                mine = [a[off:off + n].view(p.shape) for a in arenas]
                st = self.state.get(p)
                if st is not None and mark in st:                 # state made by torch's path / a loaded checkpoint moves into the arenas
                    for name, view in zip(names, mine):
                        view.copy_(st[name])
                        st[name] = view
                    self._live.add(i)
                views.append(flat_g[off:off + n].view(p.shape))
                for k, view in enumerate(mine):
                    sviews[k].append(view)
        self._mv = tuple(sviews)
        self._bound_names = names
        self._fused_steps = steps[0] if steps else 0
        self._dev_steps = torch.tensor([0, self._fused_steps], dtype=torch.int64, device=dev)
        self._skippable = False
        self._arena = (tr, flat_g, views, *arenas)
        return self._arena

    def _steps(self) -> int:
        """the fused path's step count; read back from the device when a GradScaler may have skipped steps there (one synchronisation, only
        where somebody asks: state_dict(), leaving the fused path)"""
        if self._skippable and self._dev_steps is not None:
            self._fused_steps = int(self._dev_steps[1].item())
            self._skippable = False
        return self._fused_steps

    def _sync_steps(self) -> None:
        if self._arena is not None and self._counts_steps:
            ps = self._arena[0].params
            n = self._steps()
            for i in self._live:
                self.state[ps[i]]["step"] = torch.tensor(float(n))

    def _skip_ranges(self, tr, idx) -> Optional[list]:
        """arena ranges of the parameters WITHOUT a gradient (all of them have never had one when this is called), neighbours merged; None
        when they do not fit the kernel's 8 ranges or start off a multiple of 4"""
        have = set(idx)
        ranges = tr.span_ranges(i for i in range(len(tr.params)) if i not in have)
        return None if len(ranges) > MAX_KERNEL_RANGES or any(a % 4 for a, _ in ranges) else ranges

    # ---- torch.optim.Optimizer interface --------------------------------------------------------------------------------------------------
    def _torch_step(self):
        """The torch parent's step() on the same state.  A GradScaler's device scalars (handed over because this class supports them) are applied
        the way the scaler itself would have: unscale + inf check over the gradients, one synchronisation, skip on inf."""
        found_inf, grad_scale = getattr(self, "found_inf", None), getattr(self, "grad_scale", None)
        if any(g.get("fused") for g in self.param_groups):       # torch's own fused kernels take the scaler's scalars themselves
            if any(g.get("max_grad_norm") or g.get("clip_grad_value") for g in self.param_groups):
                raise NotImplementedError("gradient clipping with torch's fused=True step: its kernel unscales the gradients itself, after any clip")
            return super().step()
        if found_inf is not None or grad_scale is not None:
            grads = [p.grad for g in self.param_groups for p in g["params"] if p.grad is not None]
            if grad_scale is not None and grads:
                inv = grad_scale.double().reciprocal().float()
                fi = found_inf if found_inf is not None else torch.zeros(1, dtype=torch.float32, device=inv.device)
                by_dev = {}
                for t in grads:
                    by_dev.setdefault((t.device, t.dtype), []).append(t)
                for (d, _), ts in by_dev.items():
                    torch._amp_foreach_non_finite_check_and_unscale_(ts, fi.to(d), inv.to(d))
            self.found_inf = self.grad_scale = None             # (torch's foreach path refuses the attributes; GradScaler deletes them afterwards)
            if found_inf is not None and float(found_inf.item()) != 0.0:
                return
        self._torch_clip()                                       # (after the unscale, as scaler.unscale_ + clip_grad_norm_ in a torch loop)
        super().step()

    @torch.no_grad()
    def step(self, closure=None):
        loss = None
        if closure is not None:
            with torch.enable_grad():
                loss = closure()
        arena = self._bind()
        grads = None
        idx = None
        skip = []
        if arena is not None:
            tr = arena[0]
            idx = [i for i, p in enumerate(tr.params) if p.grad is not None]
            grads = [tr.params[i].grad for i in idx]
            # torch SKIPS a parameter without a gradient (no state, no update).  The arena launch gives the same result for a parameter that has
            # never had one — its gradient slice and its moments are zero, the update is 0 / (0 + eps) — as long as there is no weight decay; a
            # parameter that HAS moments and misses a gradient would get an update from them here and none from torch, and one whose FIRST
            # gradient arrives after the others have stepped starts at step 1 in torch (its own bias correction): the per-tensor path then
            late = self._fused_steps > 0 and any(i not in self._live for i in idx)
            if late or any(g.is_sparse or g.dtype != torch.float32 or g.device != tr.dev for g in grads):
                arena = None
            elif len(idx) < len(tr.params):
                if not self._live.issubset(idx):
                    arena = None
                elif self._skips:
                    # a kernel with skip ranges leaves the never-reached parameters alone, whatever the decay; without decay the plain pass
                    # does too, so ranges that do not fit the kernel's eight only matter when there is one
                    skip = self._skip_ranges(tr, idx)
                    if skip is None:
                        skip = []
                        if float(self.param_groups[0]["weight_decay"]) != 0.0:
                            arena = None
                elif float(self.param_groups[0]["weight_decay"]) != 0.0:
                    arena = None
        if arena is None:
            self._release()
            self._torch_step()
            # torch's path may have made state of its own (a parameter's first gradient) and has moved the step counters: the next fused step
            # re-homes whatever the state holds now into fresh arenas (_bind)
            return loss
        tr, flat_g, views = arena[:3]
        g = self.param_groups[0]
        base = flat_g.data_ptr()
        away = [k for k, i in enumerate(idx) if grads[k].data_ptr() != base + 4 * tr.offsets[i] or not grads[k].is_contiguous()]
        if away:                                                  # gradients that are not already views of the gradient arena
            torch._foreach_copy_([views[idx[k]] for k in away], [grads[k] for k in away])
        if len(idx) < len(views) and flat_g is tr.flat_g:         # (a shared arena may hold an older pass's values in a slice nobody wrote this time)
            have = set(idx)
            for i in range(len(views)):
                if i not in have:
                    views[i].zero_()
        for i in idx:
            if i not in self._live:                               # first gradient of this parameter: it gets its state entry, as torch would make it
                self._live.add(i)
                if self._bound_names:
                    st = self.state[tr.params[i]]
                    if self._counts_steps:
                        st["step"] = torch.tensor(float(self._fused_steps))
                    for name, sv in zip(self._bound_names, self._mv):
                        st[name] = sv[i]
        found_inf, grad_scale = getattr(self, "found_inf", None), getattr(self, "grad_scale", None)
        if found_inf is not None:
            found_inf = found_inf.reshape(1).to(device=tr.dev, dtype=torch.float32)
            self._skippable = True
        if grad_scale is not None:
            grad_scale = grad_scale.reshape(1).to(device=tr.dev, dtype=torch.float32)
        self._fused_steps += 1
        kn.step_count_advance_if(self._dev_steps, found_inf)
        self._launch(tr, flat_g, arena[3:], g, grad_scale, found_inf, skip, self._clip_kwargs(tr, flat_g, g, grad_scale))
        tr.derive_after_step()
        # the kernel wrote the arena directly: the parameters' version counters did not move, so the keeper's staleness check (sum of the
        # versions) sees nothing to refresh — which is right, its copies came out of the same launches
        self.fused_launches += 1
        return loss

    def zero_grad(self, set_to_none: bool = True) -> None:
        """torch.optim.Optimizer.zero_grad.  `set_to_none=False` — the default of the torch 1.12 the reference pins, and what its Lightning calls
        between training_step and backward — is one launch per gradient in torch (106 launches, 0.38 ms of GPU time and 0.47 ms of host time
        per step, tools/study/zero_in_place_cost.py); when the gradients are the views of the keeper's gradient arena it is ONE fill of the
        arena here.  The keeper is told which version of the arena is known to be all zeros: the step node's backward then has nothing to keep
        and add back (stepnode._take_live_grads) as long as no torch operation has written the arena in between."""
        arena = self._arena
        if set_to_none or arena is None or arena[1] is not arena[0].flat_g:
            return super().zero_grad(set_to_none=set_to_none)
        tr, flat_g = arena[0], arena[1]
        lo = flat_g.data_ptr()
        hi = lo + 4 * flat_g.numel()
        inside = False
        for grp in self.param_groups:
            for p in grp["params"]:
                g = p.grad
                if g is None:
                    continue
                if g.grad_fn is not None:
                    g.detach_()
                else:
                    g.requires_grad_(False)
                if not g.is_sparse and lo <= g.data_ptr() < hi:
                    inside = True
                else:
                    g.zero_()                                     # a gradient that lives elsewhere (DDP's bucket views, a user's tensor): as torch does
        if inside:
            flat_g.zero_()                                        # (slices nobody's `.grad` points at are scratch: step() fills or zeroes them itself)
            tr.grads_zeroed_at = flat_g._version                  # views share the arena's version counter: any in-place torch op on one moves it

    def state_dict(self):
        self._sync_steps()
        return super().state_dict()

    def load_state_dict(self, state_dict):
        g0 = self.param_groups[0]
        mine = (g0.get("max_grad_norm"), g0.get("clip_grad_value"))
        super().load_state_dict(state_dict)
        if not any("max_grad_norm" in g or "clip_grad_value" in g for g in state_dict["param_groups"]):
            self.set_grad_clip(*mine)                             # (a state written without clipping keys, e.g. torch's own: this optimizer's setting stays)
        self._arena = None                                        # the loaded tensors are re-homed into the arenas by the next step()


class Adam(_ArenaStep, torch.optim.Adam):
    def __init__(self, params, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.0, amsgrad=False, **kw):
        clip = self._clip_defaults(kw)
        super().__init__(params, lr=lr, betas=betas, eps=eps, weight_decay=weight_decay, amsgrad=amsgrad, **kw)
        self._arena_init()
        self.set_grad_clip(*clip)

    def _state_names(self, g) -> tuple:
        return ("exp_avg", "exp_avg_sq")

    def _uncovered(self, g) -> bool:
        return bool(g.get("amsgrad") or g.get("capturable") or g.get("decoupled_weight_decay"))

    def _launch(self, tr, flat_g, arenas, g, grad_scale, found_inf, skip_ranges, clip) -> None:
        m, v = arenas
        kn.adam_step(tr.flat_p, flat_g, m, v, tr.flat_bf16, tr.total, float(g["lr"]), float(g["betas"][0]), float(g["betas"][1]),
                     float(g["eps"]), float(g["weight_decay"]), self._fused_steps, grad_scale=1.0, step_state_dev=self._dev_steps,
                     lo=tr.flat_lo, lo_ranges=tr.lo_ranges, loss_scale_dev=grad_scale, found_inf_dev=found_inf, **clip)


class AdamW(_ArenaStep, torch.optim.AdamW):
    """torch.optim.AdamW (conf/model/optimizer/adamw.yaml) whose step is the arena launch hulc_adamw_step.  Parameters that have never had a
    gradient are passed to the kernel as skip ranges, so the decoupled decay leaves them alone as torch does."""
    _skips = True

    def __init__(self, params, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=1e-2, amsgrad=False, **kw):
        clip = self._clip_defaults(kw)
        super().__init__(params, lr=lr, betas=betas, eps=eps, weight_decay=weight_decay, amsgrad=amsgrad, **kw)
        self._arena_init()
        self.set_grad_clip(*clip)

    def _state_names(self, g) -> tuple:
        return ("exp_avg", "exp_avg_sq")

    def _uncovered(self, g) -> bool:
        return bool(g.get("amsgrad") or g.get("capturable") or not g.get("decoupled_weight_decay"))

    def _launch(self, tr, flat_g, arenas, g, grad_scale, found_inf, skip_ranges, clip) -> None:
        m, v = arenas
        kn.adamw_step(tr.flat_p, flat_g, m, v, tr.flat_bf16, tr.total, float(g["lr"]), float(g["betas"][0]), float(g["betas"][1]),
                      float(g["eps"]), float(g["weight_decay"]), self._fused_steps, grad_scale=1.0, step_state_dev=self._dev_steps,
                      lo=tr.flat_lo, lo_ranges=tr.lo_ranges, loss_scale_dev=grad_scale, found_inf_dev=found_inf, skip_ranges=skip_ranges, **clip)


class SGD(_ArenaStep, torch.optim.SGD):
    """torch.optim.SGD (conf/model/optimizer/sgd.yaml) whose step is the arena launch hulc_sgd_step.  torch keeps no step count for SGD: a
    parameter is live once it has a `momentum_buffer` (with momentum == 0: once it has stepped here), and the device count only says
    whether a step is the first — the one that copies the gradient into the buffer."""
    _skips = True
    _counts_steps = False

    def __init__(self, params, lr=1e-3, momentum=0, dampening=0, weight_decay=0, nesterov=False, **kw):
        clip = self._clip_defaults(kw)
        super().__init__(params, lr=lr, momentum=momentum, dampening=dampening, weight_decay=weight_decay, nesterov=nesterov, **kw)
        self._arena_init()
        self.set_grad_clip(*clip)

    def _state_names(self, g) -> tuple:
        return ("momentum_buffer",) if g["momentum"] != 0 else ()

    def _uncovered(self, g) -> bool:
        return False

    def _launch(self, tr, flat_g, arenas, g, grad_scale, found_inf, skip_ranges, clip) -> None:
        kn.sgd_step(tr.flat_p, flat_g, arenas[0] if arenas else None, tr.flat_bf16, tr.total, float(g["lr"]), float(g["momentum"]),
                    float(g["dampening"]), bool(g["nesterov"]), float(g["weight_decay"]), self._fused_steps, grad_scale=1.0,
                    step_state_dev=self._dev_steps, lo=tr.flat_lo, lo_ranges=tr.lo_ranges, loss_scale_dev=grad_scale, found_inf_dev=found_inf,
                    skip_ranges=skip_ranges, **clip)
