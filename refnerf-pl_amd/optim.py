"""ClippedAdam: the optimiser step of the reference's training loop as one torch.optim.Optimizer.

The reference runs, after every backward (internal/nerf_system.py:205-217, internal/train_utils.py:448-467):
clip_grad_value_(grad_max_val), clip_grad_norm_(grad_max_norm) over all of the model's parameters, Adam.step(), and
per-parameter weights_l2s / grad_norms / grad_maxes.  Here that is 2 k + 1 launches for k tensors (3 for the flat blob of
Config.hip_flat_grads) of the kernels in csrc/refnerf_optim.h, with no host synchronisation.  The state keys are
torch.optim.Adam's (step / exp_avg / exp_avg_sq), so the `optimizer_states` of a reference checkpoint load and continue,
and `param_groups[i]['lr']` is driven by a stock LambdaLR.

CUDA float32 contiguous tensors take the kernels (anything else on a device is an error, never an eager fall-back); CPU
tensors take `_cpu_step`, a torch restatement of the same operation order."""
import math

import torch

from . import _hip


class _Plan:
    """The per-tensor device buffers of the kernels: the work-item workspace and the [n_seg, 3] statistics."""

    def __init__(self, p, seg_off):
        self.device = p.device
        self.n_seg = len(seg_off) - 1
        self.workspace, self.seg_stats, self.n_items = _hip.optim_plan(p.numel(), seg_off, p.device)


class ClippedAdam(torch.optim.Optimizer):
    """Adam (no AMSGrad, no weight decay) behind clip_grad_value_(grad_max_val) and clip_grad_norm_(grad_max_norm).

    params: tensors or param-group dicts.  `segments`: {id(tensor) or tensor: (names, offsets)} cuts a tensor into named
    runs of elements (offsets has len(names) + 1 entries, 0 .. numel) for stats(); a tensor without an entry is one segment
    named by `names` ({tensor: name}) or its index.  The global norm runs over every parameter of the optimiser that has a
    gradient, as clip_grad_norm_(model.parameters()) does; grad_max_norm must therefore be the same in every group."""

    def __init__(self, params, lr=2e-3, betas=(0.9, 0.999), eps=1e-6, grad_max_val=0.0, grad_max_norm=0.0, segments=None,
                 names=None):
        if lr < 0.0 or eps < 0.0 or not 0.0 <= betas[0] < 1.0 or not 0.0 <= betas[1] < 1.0:
            raise ValueError(f"ClippedAdam: invalid hyper-parameters lr={lr} betas={betas} eps={eps}")
        self._segments, self._plans, self._dev_state, self._last = {}, {}, None, None
        self._given = ({(k if isinstance(k, int) else id(k)): v for k, v in (segments or {}).items()},
                       {(k if isinstance(k, int) else id(k)): v for k, v in (names or {}).items()})
        super().__init__(params, dict(lr=lr, betas=tuple(betas), eps=eps, grad_max_val=grad_max_val, grad_max_norm=grad_max_norm))

    def add_param_group(self, param_group):
        """torch's, plus the segment table of every new tensor (one segment named by its index unless the constructor was
        told otherwise)."""
        super().add_param_group(param_group)
        by_id, name_of = self._given
        for i, p in enumerate(q for g in self.param_groups for q in g["params"]):
            if id(p) in self._segments:
                continue
            seg_names, off = by_id.get(id(p), ([name_of.get(id(p), str(i))], [0, p.numel()]))
            off = [int(o) for o in off]
            if len(off) != len(seg_names) + 1 or off[0] != 0 or off[-1] != p.numel() or any(b <= a for a, b in zip(off, off[1:])):
                raise ValueError(f"ClippedAdam: the segments of parameter {i} do not tile [0, {p.numel()})")
            self._segments[id(p)] = (list(seg_names), off)

    # ---- torch.optim.Adam compatibility ----------------------------------------------------------------------------
    def load_state_dict(self, state_dict):
        super().load_state_dict(state_dict)
        for g in self.param_groups:             # a torch.optim.Adam checkpoint carries no clip settings: keep the constructor's
            for k, v in self.defaults.items():
                g.setdefault(k, v)
        for st in self.state.values():          # `step` is host arithmetic here (Adam(fused / capturable) keeps it on the device),
            if torch.is_tensor(st.get("step")):  # and its own tensor (torch hands over the checkpoint's object, not a copy)
                st["step"] = st["step"].detach().to("cpu", torch.float32).clone()

    def _init_state(self, p):
        st = self.state[p]
        if len(st) == 0:
            st["step"] = torch.tensor(0.0, dtype=torch.float32)
            st["exp_avg"] = torch.zeros_like(p, memory_format=torch.preserve_format)
            st["exp_avg_sq"] = torch.zeros_like(p, memory_format=torch.preserve_format)
        return st

    def _active(self):
        out = [(g, p) for g in self.param_groups for p in g["params"] if p.grad is not None]
        norms = {float(g["grad_max_norm"]) for g in self.param_groups}
        if len(norms) > 1:
            raise ValueError("ClippedAdam: grad_max_norm is a global-norm clip and must be the same in every param group")
        for _, p in out:
            if p.grad.is_sparse:
                raise RuntimeError("ClippedAdam does not support sparse gradients")
        return out, norms.pop()

    # ---- the step --------------------------------------------------------------------------------------------------
    @torch.no_grad()
    def step(self, closure=None):
        loss = None
        if closure is not None:
            with torch.enable_grad():
                loss = closure()
        self._run(clip_only=False)
        return loss

    @torch.no_grad()
    def clip_gradients(self):
        """The two clips alone, written back into the .grad tensors (for callers who keep their own optimiser step)."""
        self._run(clip_only=True)

    def _run(self, clip_only):
        active, max_norm = self._active()
        if not active:
            return
        devices = {p.device for _, p in active}
        if len(devices) != 1:
            raise ValueError("ClippedAdam: all parameters must live on one device")
        if next(iter(devices)).type == "cuda":
            self._hip_step(active, max_norm, clip_only)
        else:
            self._cpu_step(active, max_norm, clip_only)

    @staticmethod
    def _scalars(group, st, clip_only):
        """lr, bias_correction1, sqrt(bias_correction2) of this step, in double; advances `step`."""
        if clip_only:
            return float(group["lr"]), 1.0, 1.0
        st["step"] += 1
        t = float(st["step"])
        b1, b2 = group["betas"]
        return float(group["lr"]), 1.0 - b1 ** t, math.sqrt(1.0 - b2 ** t)

    def _hip_step(self, active, max_norm, clip_only):
        dev = active[0][1].device
        for _, p in active:
            g = p.grad
            if not (p.dtype == torch.float32 and g.dtype == torch.float32 and p.is_contiguous() and g.is_contiguous() and g.device == dev):
                raise ValueError("ClippedAdam: the HIP step takes contiguous float32 parameters and gradients on one device "
                                 "(there is no eager fall-back on a device)")
        n_all = sum(len(g["params"]) for g in self.param_groups)
        with torch.cuda.device(dev):
            if self._dev_state is None or self._dev_state.device != dev or self._dev_state.numel() < _hip.optim_state_bytes(n_all):
                self._dev_state = _hip.optim_state(n_all, dev)        # (first step, or add_param_group since the last one)
            state = self._dev_state
            plans = []
            for _, p in active:
                plan = self._plans.get(id(p))
                if plan is None or plan.device != dev:
                    plan = self._plans[id(p)] = _Plan(p, self._segments[id(p)][1])
                plans.append(plan)
            for slot, ((group, p), plan) in enumerate(zip(active, plans)):
                _hip.optim_stats(p.grad, p, plan.n_seg, plan.n_items, group["grad_max_val"], plan.workspace, plan.seg_stats, state, slot)
            _hip.optim_finalize(state, len(active), max_norm)
            for group, p in active:
                st = None if clip_only else self._init_state(p)
                lr, bc1, sbc2 = self._scalars(group, st, clip_only)
                cfg = _hip.AdamCfg(lr=lr, beta1=group["betas"][0], beta2=group["betas"][1], eps=group["eps"], bias_correction1=bc1,
                                   sqrt_bias_correction2=sbc2, grad_max_val=float(group["grad_max_val"]),
                                   write_grad=int(clip_only), no_step=int(clip_only))
                if clip_only:
                    _hip.optim_adam_step(None, p.grad, None, None, cfg, state)
                else:
                    _hip.optim_adam_step(p, p.grad, st["exp_avg"], st["exp_avg_sq"], cfg, state)
        hdr = state[:8].view(torch.float32)
        self._last = dict(total_norm=hdr[0], clip_coef=hdr[1], seg={id(p): plan.seg_stats for (_, p), plan in zip(active, plans)})

    def _cpu_step(self, active, max_norm, clip_only):
        """The same operations in the same order with torch on the host (tests, callers without a device)."""
        seg_stats, clipped, c2 = {}, [], torch.zeros((), dtype=torch.float64)
        for group, p in active:
            g, val = p.grad, float(group["grad_max_val"])
            _, off = self._segments[id(p)]
            gf, wf = g.reshape(-1), p.detach().reshape(-1)
            rows = [(torch.linalg.vector_norm(gf[a:b].double()).to(g.dtype), gf[a:b].abs().max(), (wf[a:b].double() ** 2).sum().to(p.dtype))
                    for a, b in zip(off, off[1:])]
            seg_stats[id(p)] = torch.stack([torch.stack(r) for r in rows])
            c = g.clamp(min=-val, max=val) if val > 0 else g
            c2 = c2 + (c.double() ** 2).sum()
            clipped.append(c)
        total_norm = c2.sqrt()
        coef = torch.clamp(max_norm / (total_norm + 1e-6), max=1.0) if max_norm > 0 else torch.ones((), dtype=torch.float64)
        for (group, p), c in zip(active, clipped):
            g = c * coef.to(c.dtype)
            if clip_only:
                p.grad.copy_(g)
                continue
            st = self._init_state(p)
            lr, bc1, sbc2 = self._scalars(group, st, clip_only)
            b1, b2 = group["betas"]
            st["exp_avg"].lerp_(g, 1.0 - b1)
            st["exp_avg_sq"].mul_(b2).addcmul_(g, g, value=1.0 - b2)
            denom = (st["exp_avg_sq"].sqrt() / sbc2).add_(group["eps"])
            p.addcdiv_(st["exp_avg"], denom, value=-(lr / bc1))
        self._last = dict(total_norm=total_norm.to(torch.float32), clip_coef=coef.to(torch.float32), seg=seg_stats)

    # ---- statistics --------------------------------------------------------------------------------------------------
    def stats(self):
        """The last step's statistics as tensors on the parameters' device (no synchronisation): total_norm (of the
        value-clipped gradients, what clip_grad_norm_ returns), clip_coef, and {segment name: 0-d tensor} dicts grad_norms,
        grad_maxes (raw gradient) and weights_l2s (squared, before the step) -- nerf_system.on_after_backward's.
        On a device the tensors are VIEWS of the buffers the kernels write: the next step() or clip_gradients() overwrites
        them in place.  `.clone()` what has to outlive the step (a logger that gathers once per epoch), or read it first."""
        if self._last is None:
            raise RuntimeError("ClippedAdam.stats(): no step has run yet")
        out = dict(total_norm=self._last["total_norm"], clip_coef=self._last["clip_coef"], grad_norms={}, grad_maxes={}, weights_l2s={})
        for pid, tab in self._last["seg"].items():
            for i, name in enumerate(self._segments[pid][0]):
                out["grad_norms"][name], out["grad_maxes"][name], out["weights_l2s"][name] = tab[i, 0], tab[i, 1], tab[i, 2]
        return out
