"""The flat-buffer SGD mechanism every trainer shares (:class:`~.training.DecoderTrainer`,
:class:`~.cl_training.ClassifierTrainer`, :class:`~.vgg_training.VGG16ClassifierTrainer`):
the trained Parameters view one flat fp32 buffer, their gradients a second one whose tail
slots carry the step's loss (the gate) and AMP's ``found_inf`` through the DDP all-reduce,
and ``tcam_sgd_step_gated`` / ``tcam_sgd_step_amp`` update each parameter group in one launch
(torch.optim.SGD + the reference's skip of a non-finite loss, train_wsol.py:1181; AMP:
``scaler.step`` + ``scaler.update`` on the device).
"""
from __future__ import annotations

from typing import Dict, List, Optional, Sequence

import torch
import torch.distributed as dist
import torch.nn as nn

from . import _lib
from ._lib import check


def _stream() -> int:
    return torch.cuda.current_stream().cuda_stream


class FlatSGD:
    """``params`` (in order) re-pointed into ``flat``; ``bounds``: the element offsets where a
    new parameter group starts (none: one group).  Allocates on the parameters' device.

    A trainer sets, besides: ``model``, ``lrs`` (one rate per group), ``momentum``,
    ``dampening``, ``weight_decay``, ``nesterov``, ``scaler_cfg`` (growth factor, backoff
    factor, growth interval), ``bns`` (the BatchNorms it trains, if any) and ``repack()``."""

    PLANS: Sequence[str] = ()   # the model's eval plans that fold the trained weights
    bns: Sequence[nn.BatchNorm2d] = ()

    def __init__(self, params: Sequence[nn.Parameter], bounds: Sequence[int] = (),
                 amp: bool = False, init_scale: float = 2.0 ** 16):
        self.params: List[nn.Parameter] = list(params)
        self.amp = bool(amp)
        self.dev = dev = self.params[0].device
        n = sum(p.numel() for p in self.params)
        self.bounds = [int(b) for b in bounds]
        if sorted(self.bounds) != self.bounds or any(b < 0 or b > n for b in self.bounds):
            raise ValueError(f"parameter group boundaries {self.bounds} of {n} elements")
        self.flat = torch.empty(n, device=dev, dtype=torch.float32)
        # gradient + one slot for the step's total loss: the DDP all-reduce carries the loss
        # with the gradient, and the SGD kernel skips the step on the device when the summed
        # loss is not finite — every rank sees the same sum (AMP: one more slot, the
        # GradScaler found_inf flag, summed over the ranks too)
        self._gbuf = torch.zeros(n + (2 if self.amp else 1), device=dev, dtype=torch.float32)
        self.grad = self._gbuf[:n]
        self.loss_gate = self._gbuf[n:n + 1]
        self.found_inf = self._gbuf[n + 1:n + 2] if self.amp else None
        # GradScaler state on the device (torch.cuda.amp.GradScaler: _scale, _growth_tracker)
        self.scale = torch.full((1,), float(init_scale), device=dev, dtype=torch.float32)
        self.growth_tracker = torch.zeros(1, device=dev, dtype=torch.int32)
        self.mom = torch.zeros(n, device=dev, dtype=torch.float32)
        # device counters: [applied steps, skipped (non-finite) steps]
        self.step_counts = torch.zeros(2, device=dev, dtype=torch.int32)
        # per group (scale, growth tracker, counters): the tail group carries the real ones,
        # a group before it shadows (scaler.update() runs in every group's launch, once per
        # step each)
        self._group_state = [(self.scale.clone(), self.growth_tracker.clone(),
                              torch.zeros_like(self.step_counts)) for _ in self.bounds]
        self._group_state.append((self.scale, self.growth_tracker, self.step_counts))
        self.views: Dict[int, torch.Tensor] = {}
        off = 0
        for p in self.params:
            k = p.numel()
            self.flat[off:off + k].copy_(p.detach().reshape(-1))
            p.data = self.flat[off:off + k].view(p.shape)
            self.views[id(p)] = self.grad[off:off + k].view(p.shape)
            off += k
        self.zero_bias: Dict[int, torch.Tensor] = {}
        self.steps = 0

    # ------------------------------------------------------------ helpers
    def g(self, p: torch.Tensor) -> torch.Tensor:
        """The gradient of Parameter ``p``: its view of the flat gradient buffer."""
        return self.views[id(p)]

    def _zeros(self, n: int) -> torch.Tensor:
        z = self.zero_bias.get(n)
        if z is None:
            z = torch.zeros(n, device=self.dev, dtype=torch.float32)
            self.zero_bias[n] = z
        return z

    def views_intact(self) -> bool:
        """True while every trained Parameter still views this trainer's flat buffer
        (another trainer or a load that replaced ``.data`` breaks the aliasing)."""
        off, base = 0, self.flat.data_ptr()
        for p in self.params:
            if p.data_ptr() != base + 4 * off:
                return False
            off += p.numel()
        return True

    def param_version(self) -> int:
        return sum(p._version for p in self.params)

    @property
    def bn_flat(self) -> torch.Tensor:
        """A copy of every trained BN's running mean / var, concatenated (empty without
        one)."""
        return torch.cat([self.flat[:0]] + [t.reshape(-1) for bn in self.bns
                                            for t in (bn.running_mean, bn.running_var)])

    def set_bn_flat(self, flat: torch.Tensor) -> None:
        off = 0
        for bn in self.bns:
            for t in (bn.running_mean, bn.running_var):
                k = t.numel()
                t.copy_(flat[off:off + k].view_as(t))
                off += k

    @property
    def applied_steps(self) -> int:
        """SGD steps applied (steps whose all-reduced loss was finite); a host sync."""
        return int(self.step_counts[0].item())

    @property
    def skipped_steps(self) -> int:
        return int(self.step_counts[1].item())

    def _side(self, fn, *tensors) -> None:
        """Runs ``fn`` (a weight-gradient launch) on the side stream after everything queued
        so far on the current stream (``wgrad_side`` off: inline); the tensors it reads are
        marked in use by that stream so the allocator does not hand their memory out before
        it is done.  :meth:`_join_side` ends the backward that used it."""
        if not self.wgrad_side:
            fn()
            return
        if self._wg_stream is None:
            self._wg_stream = torch.cuda.Stream(device=self.dev)
        side = self._wg_stream
        side.wait_stream(torch.cuda.current_stream(self.dev))
        for t in tensors:
            if t is not None:
                t.record_stream(side)
        with torch.cuda.stream(side):
            fn()

    def _join_side(self) -> None:
        if self._wg_stream is not None:
            torch.cuda.current_stream(self.dev).wait_stream(self._wg_stream)

    # ------------------------------------------------------------- the step
    def _sgd_step(self, dist_scale: float, gate: torch.Tensor) -> None:
        """The update of every non-empty group: gradient times ``dist_scale``, skipped on the
        device when ``gate`` is not finite (AMP: when the loss slot is not finite or
        ``found_inf`` is set; scaler.step(optimizer) + scaler.update())."""
        lib = _lib.load()
        edges = [0] + self.bounds + [self.flat.numel()]
        for a, e, lr, (sc, tr, cnt) in zip(edges, edges[1:], self.lrs, self._group_state):
            if e <= a:
                continue
            args = (self.flat[a:e].data_ptr(), self.grad[a:e].data_ptr(),
                    self.mom[a:e].data_ptr(), e - a, lr, self.momentum, self.dampening,
                    self.weight_decay, 1 if self.nesterov else 0, dist_scale)
            if self.amp:
                check(lib.tcam_sgd_step_amp(*args, self._gbuf[-2:].data_ptr(), cnt.data_ptr(),
                                            cnt.data_ptr() + 4, sc.data_ptr(), tr.data_ptr(),
                                            *self.scaler_cfg, _stream()), "tcam_sgd_step_amp")
            else:
                check(lib.tcam_sgd_step_gated(*args, gate.data_ptr(), cnt.data_ptr(),
                                              cnt.data_ptr() + 4, _stream()),
                      "tcam_sgd_step_gated")

    def all_reduce_and_step(self, gate: Optional[torch.Tensor] = None) -> None:
        """DDP average (RCCL all-reduce of the flat gradient with its loss / found_inf
        slots), rank 0's BN statistics broadcast (DDP broadcast_buffers), the gated SGD step
        of every parameter group, repack; the model's eval plans are dropped (the kernels
        write the weights without a version bump).  ``gate``: a gate other than the loss
        slot; the gradient alone is then all-reduced."""
        dist_scale = 1.0
        if dist.is_available() and dist.is_initialized():
            dist.all_reduce(self._gbuf if gate is None else self.grad, op=dist.ReduceOp.SUM)
            if self.bns:
                bn = self.bn_flat
                dist.broadcast(bn, src=0)
                self.set_bn_flat(bn)
            dist_scale = 1.0 / dist.get_world_size()
        self._sgd_step(dist_scale, self.loss_gate if gate is None else gate)
        if self.bns:   # one multi-tensor launch for every BN's counter
            torch._foreach_add_([bn.num_batches_tracked for bn in self.bns], 1)
        self.repack()
        self.model.invalidate_plans(self.PLANS)
