"""LAMB (You et al., ICLR 2020, Alg. 2) with clipping of the global gradient norm: the large-batch optimizer of the Adam family, as
LARS is of SGD (`optimizer.optimizer=[LAMB, {...}]`).  torch ships none; this one steps through the fused launch group of
csrc/lamb.hip (vipant_lamb_step) and carries a plain torch implementation of the same rule for what the kernels do not cover.

Per `step()`, over the parameters that have a gradient (all groups together for G):

    G   = sqrt(sum over all tensors of sum g^2)       c = max_grad_norm > 0 ? min(1, max_grad_norm / (G + 1e-6)) : 1        g' = c g
    m   = m + (1 - beta1)(g' - m)                      v = beta2 v + (1 - beta2) g' g'
    u   = (m / bc1) / (sqrt(v / bc2) + eps) + wd p     phi = adapt and |p| > 0 and |u| > 0 ? |p| / |u| : 1 (per tensor)     p = p - lr phi u

With `exclude_bias_and_norm` a tensor with ndim < 2 has wd = 0 and no adaptation (the rule `Monitor.build_optimizer` gives LARS through
`exclude_bias_or_norm`).  Gradients are not modified.  The state per parameter is Adam's -- `step` (torch's host scalar tensor),
`exp_avg`, `exp_avg_sq` (fp32, laid out like the parameter) -- so an Adam / AdamW checkpoint's state loads into LAMB and back."""
from __future__ import annotations

import torch
from torch.optim.optimizer import _get_scalar_dtype

from .. import ops
from ..errors import VipantError
from .adam import _state_fits

__all__ = ["LAMB"]

F32 = torch.float32


class LAMB(torch.optim.Optimizer):
    """`fused=True`: one vipant_lamb_step launch group per step (no host round trip: the clip factor and the trust ratios stay on
    the device).  The plain torch step runs instead for `fused=False` and for whatever the kernels do not cover -- CPU parameters,
    non-fp32 or non-contiguous parameters, sparse or non-fp32 gradients, groups with different betas, a closure, a state that does not
    fit; the decision is taken before any step count or value is touched.  `max_grad_norm` is one value per optimizer (0 = no clipping)."""

    def __init__(self, params, lr=1e-3, betas=(0.9, 0.999), eps=1e-6, weight_decay=0.01, max_grad_norm=0.0,
                 exclude_bias_and_norm=True, fused=True):
        if lr < 0.0 or eps < 0.0 or weight_decay < 0.0 or not (0.0 <= betas[0] < 1.0 and 0.0 <= betas[1] < 1.0):
            raise VipantError(f"LAMB: need lr, eps, weight_decay >= 0 and betas in [0, 1), got {lr}, {eps}, {weight_decay}, {betas}")
        self.fused = bool(fused)          # (not a group key: torch's load_state_dict moves `step` to the device in groups that carry `fused`)
        super().__init__(params, dict(lr=lr, betas=tuple(betas), eps=eps, weight_decay=weight_decay, max_grad_norm=max_grad_norm,
                                      exclude_bias_and_norm=exclude_bias_and_norm))

    def add_param_group(self, param_group):
        super().add_param_group(param_group)
        norms = {float(g["max_grad_norm"]) for g in self.param_groups}
        if len(norms) > 1 or min(norms) < 0.0:
            raise VipantError(f"LAMB: max_grad_norm is one non-negative value per optimizer (the norm is global), the groups say {sorted(norms)}")

    def _gather(self):
        """-> [(parameter, gradient, state, (lr, weight_decay, eps, beta1, beta2, adapt))] over every parameter with a gradient; creates
        missing state."""
        todo = []
        for group in self.param_groups:
            beta1, beta2 = group["betas"]
            for p in group["params"]:
                if p.grad is None:
                    continue                # keeps its step count and its moments
                st = self.state[p]
                if len(st) == 0:
                    dtype = torch.float64 if p.dtype == torch.float64 else F32
                    st["step"] = torch.tensor(0.0, dtype=_get_scalar_dtype())
                    st["exp_avg"] = torch.zeros_like(p, dtype=dtype, memory_format=torch.preserve_format)
                    st["exp_avg_sq"] = torch.zeros_like(p, dtype=dtype, memory_format=torch.preserve_format)
                adapt = not (group["exclude_bias_and_norm"] and p.ndim < 2)
                hyper = (float(group["lr"]), float(group["weight_decay"]) if adapt else 0.0, float(group["eps"]), float(beta1), float(beta2), adapt)
                todo.append((p, p.grad, st, hyper))
        return todo

    @staticmethod
    def _kernel_covers(todo):
        dev = todo[0][0].device
        for p, g, st, hyper in todo:
            if not p.is_cuda or p.device != dev or p.dtype != F32 or not p.is_contiguous() or g.is_sparse or g.dtype != F32 or g.device != dev:
                return False
            if hyper[3:5] != todo[0][3][3:5]:
                return False
        return True

    @torch.no_grad()
    def step(self, closure=None):
        loss = None
        if closure is not None:
            with torch.enable_grad():
                loss = closure()
        todo = self._gather()
        if not todo:
            return loss
        max_grad_norm = float(self.param_groups[0]["max_grad_norm"])
        if not self.fused or closure is not None or not self._kernel_covers(todo):
            self._plain_step(todo, max_grad_norm)
            return loss
        plist, slist = [p for p, _, _, _ in todo], [st for _, _, st, _ in todo]
        glist = [g if g.is_contiguous() else g.contiguous() for _, g, _, _ in todo]
        mlist, vlist = [st["exp_avg"] for st in slist], [st["exp_avg_sq"] for st in slist]
        # the tables hold raw pointers: (re)built when the list changes (module/adam.py)
        key = tuple([p.data_ptr() for p in plist] + [m.data_ptr() for m in mlist] + [v.data_ptr() for v in vlist])
        cached = self.__dict__.get("_vipant_fused")
        if cached is None or cached[0] != key:
            if not _state_fits(plist, slist):
                self._plain_step(todo, max_grad_norm)
                return loss
            cached = self.__dict__["_vipant_fused"] = (key, ops.LambState([p.data for p in plist], mlist, vlist))
        steps = [st["step"] for st in slist]
        torch._foreach_add_(steps, 1)
        memo, recs = {}, []
        for (_, _, _, hyper), count in zip(todo, torch.stack(steps).tolist()):        # lr / weight_decay / eps as the groups hold them NOW
            k = (hyper, count)
            if k not in memo:
                lr, wd, eps, beta1, beta2, adapt = hyper
                memo[k] = ops.LambState.record(lr, wd, eps, beta1, beta2, count, adapt)
            recs.append(memo[k])
        beta1, beta2 = todo[0][3][3:5]
        cached[1].step(glist, recs, beta1, beta2, max_grad_norm, checked=all(g.shape == p.shape for g, p in zip(glist, plist)))
        # the kernels wrote the parameters through raw pointers: tell torch (module/lars.py: the bf16 weight cache of no-grad forwards
        # is keyed on a tensor's version)
        torch.autograd.graph.increment_version(plist)
        return loss

    @staticmethod
    def _plain_step(todo, max_grad_norm):
        """The rule in torch operations, tensor by tensor, in the precision of the moments (fp32; float64 for float64 parameters)."""
        grads = [(g.to_dense() if g.is_sparse else g).to(st["exp_avg"].dtype) for _, g, st, _ in todo]
        clip = None
        if max_grad_norm > 0:
            norms = torch.stack([torch.linalg.vector_norm(g).to(grads[0].device) for g in grads])
            clip = torch.clamp(max_grad_norm / (torch.linalg.vector_norm(norms) + 1e-6), max=1.0)
        for (p, _, st, (lr, wd, eps, beta1, beta2, adapt)), g in zip(todo, grads):
            if clip is not None:
                g = g * clip.to(g.device)
            st["step"] += 1
            count = float(st["step"])
            m, v = st["exp_avg"], st["exp_avg_sq"]
            w = p.detach().to(m.dtype)
            m.add_(g - m, alpha=1.0 - beta1)
            v.mul_(beta2).addcmul_(g, g, value=1.0 - beta2)
            u = (m / (1.0 - beta1 ** count)) / ((v / (1.0 - beta2 ** count)).sqrt() + eps)
            if wd != 0:
                u = u + wd * w
            if adapt:
                pn, un = torch.linalg.vector_norm(w), torch.linalg.vector_norm(u)
                u = u * torch.where((pn > 0) & (un > 0), pn / un, torch.ones_like(pn))
            p.copy_(w - lr * u)
