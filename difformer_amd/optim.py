"""The optimiser of the reference's drivers with the update on the device in one launch.

    optimizer = difformer_amd.Adam(model.parameters(), lr=args.lr, weight_decay=args.weight_decay)     # was: torch.optim.Adam(...)

`node classification/main.py:111`, `image and text/main.py:95`, `spatial-temporal/main.py:83` and `physical particle/main.py:77`
all build `torch.optim.Adam(model.parameters(), lr=..., weight_decay=...)`, whose default foreach path is seven multi-tensor
launches per step.  `Adam` here is a subclass: `param_groups`, `zero_grad`, `add_param_group`, `state_dict` and
`load_state_dict` are torch's, and `step()` hands every float32 parameter of a group that has a gradient to csrc/adam.hip
(C ABI include/difformer_adam.h) in one launch per 48 tensors.

Semantics are torch.optim.Adam's with amsgrad=False, maximize=False and the L2 weight decay `g + wd p` (not AdamW).  Every
element is evaluated in float64 from the unrounded moments and p, exp_avg and exp_avg_sq are rounded once to float32; there is
no floating-point atomic, so two steps from bitwise-equal state give bitwise-equal state.  Gradients are read, never written.

State per parameter is torch's: `step` (a 0-d float32 tensor on the parameter's device, as with capturable=True), `exp_avg`,
`exp_avg_sq`.  The kernel increments `step`; the host never reads it and nothing synchronises, so a step can be captured as
it is -- `GraphedTrainStep(model, difformer_amd.Adam(...), ...)` needs no flag.  A device group reports capturable=True in its
`param_groups` entry, so that `state_dict()` loads into `torch.optim.Adam(..., capturable=True)` and back.  Hyper-parameters
are read from `param_groups` at every eager step; a captured step has them baked in, as torch with a float lr.

The kernels of this package write parameters through raw pointers and key every packed-weight memo on
`(data_ptr, _version)`; `step()` therefore bumps the version counter of every parameter it updated
(`torch.autograd.graph.increment_version`, no kernel launched), or the next forward would serve stale weights.

A group of CPU parameters takes torch's own step, unchanged.  Anything else raises ValueError before the device is touched:
bfloat16, float16 or float64 parameters on the device, a group that mixes placements, sparse gradients, amsgrad, maximize,
differentiable, decoupled weight decay, a tensor lr.
"""
from __future__ import annotations

import torch

from . import ops

__all__ = ["Adam"]


def _on_device(t):
    """Does this tensor go through the kernel (True) or through torch's step (False: a CPU tensor)?"""
    return t.device.type != "cpu"


def _check_group(group):
    """The options the kernel does not implement; at construction and again at every step (param_groups is the user's)."""
    for flag in ("amsgrad", "maximize", "differentiable", "decoupled_weight_decay"):
        if group.get(flag):
            raise ValueError(f"difformer_amd.Adam: {flag}=True is not implemented (torch.optim.Adam has it)")
    if torch.is_tensor(group["lr"]):
        raise ValueError("difformer_amd.Adam: lr must be a Python float, not a tensor")


class Adam(torch.optim.Adam):
    def __init__(self, params, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=0, amsgrad=False, *, maximize=False,
                 differentiable=False):
        _check_group(dict(lr=lr, amsgrad=amsgrad, maximize=maximize, differentiable=differentiable))
        super().__init__(params, lr=lr, betas=betas, eps=eps, weight_decay=weight_decay, foreach=None, fused=None)

    def add_param_group(self, param_group):
        """torch's, then the placement of the group decides `capturable`: True for device parameters (step counters on the
        device), False for CPU parameters (torch's step, bitwise)."""
        super().add_param_group(param_group)
        group = self.param_groups[-1]
        try:
            _check_group(group)
            group["capturable"] = self._placement(group)
        except ValueError:
            del self.param_groups[-1]
            raise

    def load_state_dict(self, state_dict):
        """torch's, then device groups get their step counters back on the device (a state_dict of a torch.optim.Adam without
        capturable keeps them on the host)."""
        super().load_state_dict(state_dict)
        for group in self.param_groups:
            _check_group(group)
            group["capturable"] = self._placement(group)
            if group["capturable"]:
                for p in group["params"]:
                    st = self.state.get(p)
                    if st and torch.is_tensor(st.get("step")) and (st["step"].device != p.device or st["step"].dtype != torch.float32):
                        st["step"] = st["step"].to(device=p.device, dtype=torch.float32)

    @staticmethod
    def _placement(group):
        """True: every parameter is a float32 device tensor; False: every one is on the CPU; else ValueError."""
        where = {_on_device(p) for p in group["params"]}
        if len(where) > 1:
            raise ValueError("difformer_amd.Adam: a parameter group mixes CPU and device parameters")
        if where == {True}:
            for p in group["params"]:
                if p.dtype != torch.float32:
                    raise ValueError(f"difformer_amd.Adam: device parameters must be float32 (got {p.dtype}, {tuple(p.shape)}); "
                                     "bfloat16, float16 and float64 parameters are not updated by the kernel")
            return True
        return False

    def _collect(self, group):
        """The group's parameters that have a gradient and those gradients, dense; every check, no device work."""
        params, grads = [], []
        dev = None
        for p in group["params"]:
            g = p.grad
            if g is None:
                continue
            if not _on_device(p):
                raise ValueError("difformer_amd.Adam: a parameter group mixes CPU and device parameters")
            if p.dtype != torch.float32:
                raise ValueError(f"difformer_amd.Adam: device parameters must be float32 (got {p.dtype}, {tuple(p.shape)}); "
                                 "bfloat16, float16 and float64 parameters are not updated by the kernel")
            if g.is_sparse or g.layout != torch.strided:
                raise ValueError("difformer_amd.Adam: sparse gradients are not supported")
            if dev is None:
                dev = p.device
            elif p.device != dev:
                raise ValueError(f"difformer_amd.Adam: a parameter group spans {dev} and {p.device}")
            if not p.is_contiguous():
                raise ValueError(f"difformer_amd.Adam: parameters must be contiguous (got shape {tuple(p.shape)}, strides {p.stride()})")
            params.append(p)
            grads.append(g)
        return params, grads

    def _moments(self, params):
        """exp_avg, exp_avg_sq and step of every parameter, made on first use."""
        exp_avgs, exp_avg_sqs, steps = [], [], []
        for p in params:
            st = self.state[p]
            if not st:
                st["step"] = torch.zeros((), dtype=torch.float32, device=p.device)
                st["exp_avg"] = torch.zeros_like(p, memory_format=torch.contiguous_format)
                st["exp_avg_sq"] = torch.zeros_like(p, memory_format=torch.contiguous_format)
            exp_avgs.append(st["exp_avg"])
            exp_avg_sqs.append(st["exp_avg_sq"])
            steps.append(st["step"])
        return exp_avgs, exp_avg_sqs, steps

    @torch.no_grad()
    def step(self, closure=None):
        loss = None
        if closure is not None:
            with torch.enable_grad():
                loss = closure()
        host, work = [], []
        for group in self.param_groups:                      # every error before the first launch
            _check_group(group)
            if not group["params"]:
                continue
            on = _on_device(group["params"][0])              # placement as it is NOW: model.to() after construction moves it
            if group.get("capturable") != on:
                group["capturable"] = self._placement(group)
            if on:
                work.append((group, self._collect(group)))
            else:
                if any(_on_device(p) for p in group["params"]):
                    raise ValueError("difformer_amd.Adam: a parameter group mixes CPU and device parameters")
                host.append(group)
        if host:                                             # torch's own step over the CPU groups alone
            every = self.param_groups
            self.param_groups = host
            try:
                super().step()
            finally:
                self.param_groups = every
        be = ops.get_backend() if work else None
        for group, (params, grads) in work:                  # every check of every group has passed
            if not params:
                continue
            grads = [g if g.is_contiguous() else g.contiguous() for g in grads]
            exp_avgs, exp_avg_sqs, steps = self._moments(params)
            beta1, beta2 = group["betas"]
            be.adam_step(params, grads, exp_avgs, exp_avg_sqs, steps, float(group["lr"]), float(beta1), float(beta2),
                         float(group["eps"]), float(group["weight_decay"]))
            torch.autograd.graph.increment_version(params)     # the (data_ptr, _version) memos of the forward see the update
        return loss
