"""FusedAdam: torch.optim.Adam semantics, one HIP launch for up to 8 tensors.

The reference builds torch.optim.Adam over five parameter groups
(src/core/optimizer.py:100-113); torch's fused Adam then launches once per
group.  This optimizer keeps the same per-group hyper-parameters and state
layout ('step', 'exp_avg', 'exp_avg_sq' per parameter) but updates every
tensor in a single gs_adam_step launch.
Parameters without .grad are skipped, as torch does.

Visibility-gated step (gsplat's visible_adam / SelectiveAdam, the sparse Adam
of Taming 3DGS): step(visible=mask) updates the rows mask marks and leaves the
parameters and both moments of every other row bit for bit, whatever their
gradients hold -- one gs_adam_step_rows launch.  The step counts (and so the
bias corrections) advance as without the mask: they are per tensor, not per
row.
"""
from __future__ import annotations

import ctypes as C
import itertools

import torch
from torch.optim import optimizer as _OPT

from . import _native as N


class FusedAdam(torch.optim.Optimizer):
    def __init__(self, params, lr=1e-3, betas=(0.9, 0.999), eps=1e-8):
        super().__init__(params, dict(lr=lr, betas=betas, eps=eps))
        # parameter -> tensor the updated value is written to instead of the
        # parameter (gs_adam_tensor.param_out); empty: in place, as torch
        self.param_out = {}

    def set_output(self, param: torch.Tensor, out: torch.Tensor) -> None:
        """Write param's updates to `out` (same shape, contiguous fp32, no
        overlap) and leave param unchanged: the in-place step's reads and
        writes, for a benchmark that renders one fixed scene every step."""
        if out.shape != param.shape or out.dtype != torch.float32 or not out.is_contiguous() or \
                out.device != param.device or out.data_ptr() == param.data_ptr():
            raise ValueError("param_out must be a separate contiguous fp32 tensor shaped like the parameter")
        self.param_out[param] = out

    def _begin(self):
        """Advance every parameter with a gradient by one step: the descriptors
        (param, moments, grad, row count, lr, bias corrections) of this step,
        grouped by (beta1, beta2, eps)."""
        batches = {}
        for group in self.param_groups:
            b1, b2 = group["betas"]
            for p in group["params"]:
                if p.grad is None:
                    continue
                if not (p.is_cuda and p.dtype == torch.float32 and p.is_contiguous() and p.grad.is_contiguous()):
                    raise RuntimeError("FusedAdam needs contiguous fp32 HIP tensors")
                st = self.state[p]
                if not st:
                    st["step"] = 0
                    st["exp_avg"] = torch.zeros_like(p)
                    st["exp_avg_sq"] = torch.zeros_like(p)
                st["step"] += 1
                t = st["step"]
                rows = p.shape[0] if p.dim() else 1
                batches.setdefault((float(b1), float(b2), float(group["eps"])), []).append(
                    (p, st["exp_avg"], st["exp_avg_sq"], p.grad, rows, float(group["lr"]), 1.0 - b1 ** t,
                     (1.0 - b2 ** t) ** 0.5, self.param_out.get(p)))
        return batches

    @staticmethod
    def _launch(batches, lo=None, hi=None):
        """One gs_adam_step per (betas, eps) batch of <= 8 tensors, over rows
        [lo, hi) of each (dim 0; all rows when lo is None)."""
        if not batches:
            return
        lib = N.load()
        stream = N.stream_ptr()
        for (b1, b2, eps), ds in batches.items():
            for i in range(0, len(ds), N.GS_ADAM_MAX_TENSORS):
                chunk = ds[i:i + N.GS_ADAM_MAX_TENSORS]
                a = N.GsAdamArgs()
                a.num_tensors, a.beta1, a.beta2, a.eps = len(chunk), b1, b2, eps
                a.one_minus_beta1, a.one_minus_beta2 = 1.0 - b1, 1.0 - b2  # (in double, rounded once)
                for k, (p, m, v, g, rows, lr, bc1, bc2s, out) in enumerate(chunk):
                    if lo is None:
                        off, num = 0, p.numel()
                    else:
                        cols = p.numel() // max(rows, 1)
                        r0, r1 = min(lo, rows), min(hi, rows)
                        off, num = r0 * cols, (r1 - r0) * cols
                    a.t[k] = N.GsAdamTensor(N.ptr(p) + 4 * off, N.ptr(m) + 4 * off, N.ptr(v) + 4 * off,
                                            N.ptr(g) + 4 * off, num, lr, bc1, bc2s,
                                            N.ptr(out) + 4 * off if out is not None else None)
                N.check(lib.gs_adam_step(C.byref(a), stream), "gs_adam_step")

    def _check_visible(self, visible) -> None:
        """ValueError unless `visible` is a contiguous [N] bool / uint8 tensor
        on the parameters' device with N = dim 0 of every parameter that has
        a gradient, and no such parameter has a set_output (before anything
        is launched or counted)."""
        if not isinstance(visible, torch.Tensor) or visible.dtype not in (torch.bool, torch.uint8):
            raise ValueError("visible must be a bool or uint8 tensor, got "
                             f"{getattr(visible, 'dtype', type(visible).__name__)}")
        if visible.dim() != 1 or not visible.is_contiguous():
            raise ValueError(f"visible must be a contiguous [N] mask, got shape {tuple(visible.shape)} "
                             f"stride {tuple(visible.stride())}")
        n = visible.shape[0]
        for group in self.param_groups:
            for p in group["params"]:
                if p.grad is None:
                    continue
                if p.device != visible.device:
                    raise ValueError(f"visible is on {visible.device}, a parameter on {p.device}")
                if p.dim() < 1 or p.shape[0] != n:
                    raise ValueError(f"visible marks {n} rows, a parameter with a gradient has shape "
                                     f"{tuple(p.shape)}")
                if p in self.param_out:
                    raise ValueError("visible does not combine with set_output parameters (gs_adam_step_rows "
                                     "updates in place)")

    @staticmethod
    def _launch_rows(batches, visible, lo=None, hi=None):
        """_launch through gs_adam_step_rows: rows [lo, hi) (all when lo is
        None) of every tensor, the mask offset by lo."""
        if not batches:
            return
        lib = N.load()
        stream = N.stream_ptr()
        n = visible.shape[0]
        r0, r1 = (0, n) if lo is None else (min(lo, n), min(hi, n))
        for (b1, b2, eps), ds in batches.items():
            for i in range(0, len(ds), N.GS_ADAM_MAX_TENSORS):
                chunk = ds[i:i + N.GS_ADAM_MAX_TENSORS]
                a = N.GsAdamRowsArgs()
                a.rows, a.row_mask = r1 - r0, N.ptr(visible) + r0
                ad = a.adam
                ad.num_tensors, ad.beta1, ad.beta2, ad.eps = len(chunk), b1, b2, eps
                ad.one_minus_beta1, ad.one_minus_beta2 = 1.0 - b1, 1.0 - b2  # (in double, rounded once)
                for k, (p, m, v, g, rows, lr, bc1, bc2s, _) in enumerate(chunk):
                    cols = p.numel() // max(rows, 1)
                    off = r0 * cols
                    a.cols[k] = max(cols, 1)
                    ad.t[k] = N.GsAdamTensor(N.ptr(p) + 4 * off, N.ptr(m) + 4 * off, N.ptr(v) + 4 * off,
                                             N.ptr(g) + 4 * off, (r1 - r0) * cols, lr, bc1, bc2s, None)
                N.check(lib.gs_adam_step_rows(C.byref(a), stream), "gs_adam_step_rows")

    def zero_grad(self, set_to_none: bool = True) -> None:
        """Optimizer.zero_grad without its profiler annotation (host time
        the small configurations are bound by); same semantics."""
        for group in self.param_groups:
            for p in group["params"]:
                if p.grad is not None:
                    if set_to_none:
                        p.grad = None
                    else:
                        if p.grad.grad_fn is not None:
                            p.grad.detach_()
                        else:
                            p.grad.requires_grad_(False)
                        p.grad.zero_()

    def _hooks_registered(self) -> bool:
        return bool(self._optimizer_step_pre_hooks or self._optimizer_step_post_hooks
                    or _OPT._global_optimizer_pre_hooks or _OPT._global_optimizer_post_hooks)

    def _hooked(self, fn, args, kwargs):
        """fn(*args, **kwargs) between the registered step pre / post hooks,
        in torch.optim.Optimizer's order and with its argument rewriting
        (torch's profile_hook_step wrapper, which `step.hooked` skips)."""
        for hook in itertools.chain(_OPT._global_optimizer_pre_hooks.values(),
                                    self._optimizer_step_pre_hooks.values()):
            res = hook(self, args, kwargs)
            if res is not None:
                if isinstance(res, tuple) and len(res) == 2:
                    args, kwargs = res
                else:
                    raise RuntimeError(f"{hook} must return None or a tuple of (new_args, new_kwargs), "
                                       f"but got {res}.")
        out = fn(*args, **kwargs)
        for hook in itertools.chain(self._optimizer_step_post_hooks.values(),
                                    _OPT._global_optimizer_post_hooks.values()):
            hook(self, args, kwargs)
        return out

    @torch.no_grad()
    def step(self, closure=None, visible=None):
        """One Adam step over every parameter with a gradient.  visible: a [N]
        bool / uint8 mask on the parameters' device -- only the rows it marks
        are updated (every parameter with a gradient must have N rows); None:
        the dense step, as follows.  The launch
        descriptors are kept between steps and only the per-step fields
        (gradient address, lr, bias corrections) rewritten while the
        parameters, moments and outputs stay where they were.  torch's
        profiler annotation is not run (step is marked hooked, see below);
        registered step pre / post hooks (per optimizer or global) are, when
        there are any (checking costs two dict tests)."""
        if visible is not None:
            if self._hooks_registered():
                return self._hooked(self._step_visible, (closure,), {"visible": visible})
            return self._step_visible(closure, visible=visible)
        if self._hooks_registered():
            return self._hooked(self._step, (closure,), {})
        return self._step(closure)

    def _step_visible(self, closure=None, visible=None):
        loss = None
        if closure is not None:
            with torch.enable_grad():
                loss = closure()
        self._check_visible(visible)
        self._launch_rows(self._begin(), visible)
        return loss

    def _step(self, closure=None):
        loss = None
        if closure is not None:
            with torch.enable_grad():
                loss = closure()
        plan, per_step = [], []
        for group in self.param_groups:
            b1, b2 = group["betas"]
            eps, lr = group["eps"], group["lr"]
            for p in group["params"]:
                g = p.grad
                if g is None:
                    continue
                if not g.is_contiguous():
                    raise RuntimeError("FusedAdam needs contiguous gradients")
                st = self.state[p]
                if not st:
                    if not (p.is_cuda and p.dtype == torch.float32 and p.is_contiguous()):
                        raise RuntimeError("FusedAdam needs contiguous fp32 HIP tensors")
                    st["step"] = 0
                    st["exp_avg"] = torch.zeros_like(p)
                    st["exp_avg_sq"] = torch.zeros_like(p)
                st["step"] += 1
                t = st["step"]
                out = self.param_out.get(p)
                plan.append((p.data_ptr(), st["exp_avg"].data_ptr(), st["exp_avg_sq"].data_ptr(),
                             out.data_ptr() if out is not None else 0, p.numel(), float(b1), float(b2), float(eps)))
                per_step.append((g, float(lr), 1.0 - b1 ** t, (1.0 - b2 ** t) ** 0.5))
        if not plan:
            return loss  # (no parameter has a gradient: nothing to launch)
        key = tuple(plan)
        cached = getattr(self, "_plan_cache", None)
        if cached is None or cached[0] != key:
            launches = []
            by_betas = {}
            for i, d in enumerate(plan):
                by_betas.setdefault(d[5:8], []).append(i)
            for (b1, b2, eps), idx in by_betas.items():
                for j in range(0, len(idx), N.GS_ADAM_MAX_TENSORS):
                    chunk = idx[j:j + N.GS_ADAM_MAX_TENSORS]
                    a = N.GsAdamArgs()
                    a.num_tensors, a.beta1, a.beta2, a.eps = len(chunk), b1, b2, eps
                    a.one_minus_beta1, a.one_minus_beta2 = 1.0 - b1, 1.0 - b2  # (in double, rounded once)
                    for k, i in enumerate(chunk):
                        pp, m, v, o, num = plan[i][:5]
                        a.t[k] = N.GsAdamTensor(pp, m, v, None, num, 0.0, 1.0, 1.0, o or None)
                    launches.append((a, chunk))
            cached = self._plan_cache = (key, launches)
        lib = N.load()
        stream = N.stream_ptr()
        for a, chunk in cached[1]:
            for k, i in enumerate(chunk):
                g, lr, bc1, bc2s = per_step[i]
                tk = a.t[k]
                tk.grad, tk.lr, tk.bias_correction1, tk.bias_correction2_sqrt = g.data_ptr(), lr, bc1, bc2s
            N.check(lib.gs_adam_step(C.byref(a), stream), "gs_adam_step")
        return loss

    # torch.optim.Optimizer wraps step with its hook / profiler dispatch unless
    # the function says it is hooked already: ~40 us of host time per step,
    # which the small configurations are bound by
    step.hooked = True

    @torch.no_grad()
    def step_ranges(self, ranges, before=None, visible=None):
        """The same update as step() (Adam is elementwise: bit-identical),
        launched over row ranges [lo, hi) of every parameter in turn; before(k),
        when given, runs before range k is queued -- the data-parallel
        reducer makes the stream wait for range k's all-reduce there, so
        range k's update overlaps the reductions of the ranges after it.
        visible: as step(); range k reads the mask from row lo on (the ranges
        are arbitrary, nothing is rounded to the kernel's row blocks)."""
        if visible is not None:
            self._check_visible(visible)
        if self._hooks_registered():
            return self._hooked(self._step_ranges, (ranges, before), {} if visible is None else {"visible": visible})
        return self._step_ranges(ranges, before, visible=visible)

    def _step_ranges(self, ranges, before=None, visible=None):
        batches = self._begin()
        for k, (lo, hi) in enumerate(ranges):
            if before is not None:
                before(k)
            if visible is None:
                self._launch(batches, lo, hi)
            else:
                self._launch_rows(batches, visible, lo, hi)


# --------------------------------------------------------------------------
# Schedules and density control (reference src/core/optimizer.py:7-141)
# --------------------------------------------------------------------------
import math  # noqa: E402


class LearningRateScheduler:
    """optimizer.py:7-32: cosine from lr_init to lr_final over max_steps,
    times the delay ramp lr_delay_mult -> 1 over lr_delay_steps."""

    def __init__(self, lr_init: float, lr_final: float, lr_delay_steps: int, lr_delay_mult: float, max_steps: int):
        self.lr_init, self.lr_final = lr_init, lr_final
        self.lr_delay_steps, self.lr_delay_mult, self.max_steps = lr_delay_steps, lr_delay_mult, max_steps

    def get_lr(self, step: int) -> float:
        if self.max_steps <= 0:
            return self.lr_final
        t = min(step, self.max_steps) / self.max_steps
        lr = self.lr_final + (self.lr_init - self.lr_final) * 0.5 * (1 + math.cos(math.pi * t))
        if self.lr_delay_steps > 0:
            lr *= self.lr_delay_mult + (1 - self.lr_delay_mult) * min(step / self.lr_delay_steps, 1)
        return float(lr)


class DensityController:
    """optimizer.py:34-88: densify in [densify_from_iter, densify_until_iter]
    every densify_interval iterations; split / clone by |dL/dxyz| and prune
    opacity <= min_opacity in one GPU pass (GaussianModel.densify_and_prune),
    the Adam state following the Gaussians.  With config.densify_criterion
    "screen" the gradient test reads the model's accumulated screen-space
    statistics (gaussians.density_stats) and config.prune_screen_radius joins
    the prune.  dist: the trainer's process group module when data parallel:
    every rank has seen other views, so the statistics are all-reduced right
    before (SUM of grad_accum and denom, MAX of max_radii) and every rank
    takes the same decisions.  With config.densify_absgrad the split test
    reads the statistics' absolute gradient (abs_accum, all-reduced with SUM
    beside the others) against config.densify_abs_grad_threshold."""

    def __init__(self, config):
        self.config = config

    def should_densify(self, iteration: int) -> bool:
        c = self.config
        return c.densify_from_iter <= iteration <= c.densify_until_iter and iteration % c.densify_interval == 0

    @torch.no_grad()
    def densify_and_prune(self, gaussians, optimizer, iteration: int, scene_extent: float, dist=None) -> dict:
        c = self.config
        kw = {}
        if getattr(c, "densify_criterion", "xyz_grad") == "screen":
            stats = gaussians.density_stats
            if dist is not None and stats.n:
                dist.all_reduce(stats.grad_accum, op=dist.ReduceOp.SUM)
                dist.all_reduce(stats.denom, op=dist.ReduceOp.SUM)
                dist.all_reduce(stats.max_radii, op=dist.ReduceOp.MAX)
                if stats.abs_accum is not None:
                    dist.all_reduce(stats.abs_accum, op=dist.ReduceOp.SUM)
            kw = {"stats": stats, "max_screen_radius": float(getattr(c, "prune_screen_radius", 0.0))}
            if getattr(c, "densify_absgrad", False):
                kw["abs_grad_threshold"] = float(c.densify_abs_grad_threshold)
        return gaussians.densify_and_prune(c.densify_grad_threshold, scene_extent,
                                           getattr(c, "min_opacity", 0.01), optimizer=optimizer,
                                           seed=0x5EED0000 + iteration, **kw)


class GaussianOptimizer:
    """optimizer.py:90-141 with FusedAdam over the reference's five groups.
    After densification the Adam moments are remapped, kept Gaussians
    carrying theirs; with config.reset_adam_on_densify a fresh optimizer is
    built instead, as the reference's setup_optimizer() does
    (optimizer.py:133-137: every moment and step count dropped)."""

    def __init__(self, gaussians, config):
        self.gaussians, self.config = gaussians, config
        self.optimizer = None
        self.lr_scheduler = LearningRateScheduler(config.position_lr_init, config.position_lr_final, 0, 1.0,
                                                  config.iterations)
        self.density_controller = DensityController(config)

    def setup_optimizer(self) -> None:
        g, c = self.gaussians, self.config
        self.optimizer = FusedAdam([
            {"params": [g._xyz], "lr": c.position_lr_init},
            {"params": [g._features_dc, g._features_rest], "lr": c.feature_lr},
            {"params": [g._opacity], "lr": c.opacity_lr},
            {"params": [g._scaling], "lr": c.scaling_lr},
            {"params": [g._rotation], "lr": c.rotation_lr},
        ])  # torch.optim.Adam defaults, as optimizer.py:109

    def step(self, visible=None) -> None:
        """The Adam step; visible: the [N] mask of the rows to update
        (FusedAdam.step), None: every row."""
        if visible is None:
            self.optimizer.step()
        else:
            self.optimizer.step(visible=visible)

    def zero_grad(self) -> None:
        self.optimizer.zero_grad(set_to_none=True)

    def update_learning_rate(self, iteration: int) -> None:
        """optimizer.py:120-129: every group follows the position schedule's ratio."""
        base, c = self.lr_scheduler.get_lr(iteration), self.config
        pg = self.optimizer.param_groups
        pg[0]["lr"] = base
        pg[1]["lr"] = base * (c.feature_lr / c.position_lr_init)
        pg[2]["lr"] = base * (c.opacity_lr / c.position_lr_init)
        pg[3]["lr"] = base * (c.scaling_lr / c.position_lr_init)
        pg[4]["lr"] = base * (c.rotation_lr / c.position_lr_init)

    def densify_and_prune(self, iteration: int, scene_extent: float, dist=None):
        if self.density_controller.should_densify(iteration):
            info = self.density_controller.densify_and_prune(self.gaussians, self.optimizer, iteration, scene_extent,
                                                             dist=dist)
            if getattr(self.config, "reset_adam_on_densify", False):
                self.setup_optimizer()
            return info
        return None

    # -- densify_criterion "mcmc" (3DGS-MCMC) -------------------------------------
    def mcmc_regularize(self) -> None:
        """Add the gradients of mcmc_opacity_reg * mean(opacity) + mcmc_scale_reg *
        mean(scale) to _opacity.grad and _scaling.grad (one launch, before the
        Adam step; a parameter without a gradient is skipped)."""
        from . import mcmc
        g, c = self.gaussians, self.config
        mcmc.mcmc_regularize(g._opacity.data, g._scaling.data, g._opacity.grad, g._scaling.grad,
                             c.mcmc_opacity_reg, c.mcmc_scale_reg)

    def relocate_and_grow(self, iteration: int):
        """On a refinement iteration (the densification schedule),
        GaussianModel.relocate_and_grow seeded by the iteration; else None."""
        if not self.density_controller.should_densify(iteration):
            return None
        c = self.config
        return self.gaussians.relocate_and_grow(c.mcmc_cap_max, c.mcmc_min_opacity, 0x3C3C0000 + 2 * iteration,
                                                optimizer=self.optimizer, grow_factor=c.mcmc_grow_factor)

    def mcmc_noise(self, iteration: int) -> None:
        """The iteration's position noise (one launch, after the Adam step and
        the refinement): mcmc_noise_lr * the xyz group's current learning
        rate, seeded by the iteration."""
        from . import mcmc
        g = self.gaussians
        scale = float(self.config.mcmc_noise_lr) * float(self.optimizer.param_groups[0]["lr"])
        mcmc.mcmc_noise(g._xyz.data, g._scaling.data, g._rotation.data, g._opacity.data, scale,
                        0x401E0000 + iteration)

    def reset_opacity(self) -> None:
        self.gaussians.reset_opacity()

    @torch.no_grad()
    def prune_by_contribution(self, stats, threshold: float) -> dict:
        """Drop every Gaussian whose largest blend weight over the views in
        `stats` (ContributionStats.weight_max) is not above `threshold` (>= 0;
        0 keeps exactly what contributed somewhere), the Adam moments of the
        kept ones following them.  The criterion reads weight_max only, which
        no summation order touches: every data-parallel rank and a single
        process decide the same.  Returns {"n_before", "n_after"}."""
        threshold = float(threshold)
        if not threshold >= 0.0:
            raise ValueError(f"the contribution threshold must be >= 0, got {threshold!r}")
        g = self.gaussians
        n = g.get_num_points()
        if stats.n != n or stats.device != g._xyz.device:
            raise ValueError(f"stats holds {stats.n} Gaussians on {stats.device}, the model {n} on {g._xyz.device}")
        keep = stats.weight_max > threshold
        g.prune_points(keep, self.optimizer)
        return {"n_before": n, "n_after": g.get_num_points()}

    @torch.no_grad()
    def cap_opacity(self, max_opacity: float = 0.01) -> None:
        """The 3DGS opacity reset: every opacity above max_opacity comes down to
        it -- _opacity.data = minimum(_opacity, logit(max_opacity)), the logit
        rounded to fp32 once -- and the opacity parameter's Adam moments start
        over from zero (its step count stays; no other state is touched).
        reset_opacity keeps the reference's own semantics (every opacity set)."""
        p = self.gaussians._opacity
        cap = torch.tensor(math.log(max_opacity / (1.0 - max_opacity)), dtype=torch.float32, device=p.device)
        torch.minimum(p.data, cap, out=p.data)  # (in place: the address other launches hold stays)
        st = self.optimizer.state.get(p) if self.optimizer is not None else None
        if st:
            st["exp_avg"].zero_()
            st["exp_avg_sq"].zero_()
