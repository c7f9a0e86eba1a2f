"""ClippedSGD -- the optimizer tail of the reference's training step (train_fast.py:165-166: clip_grad_norm(max_norm=35), then the
step of torch.optim.SGD(lr, momentum=0.9, weight_decay=1e-4)) as ONE native call over all parameters (dtc_sgd_step: two kernel
nodes, detectorch_amd/csrc/optim/clipped_sgd.hip) instead of a chain of foreach kernels that each stream the whole parameter set.

Differences from clip_grad_norm_ + torch.optim.SGD that a caller can observe (include/detectorch_optim_hip.h has the contract):
  * GPU only: step() raises on CPU parameters; dense contiguous float32 parameters and gradients only;
  * gradients are NOT written: .grad stays unclipped, the clip factor is applied on the fly;
  * momentum buffers start as zeros and the first step uses the general formula (torch clones the first update): equal values,
    only a -0.0 of the update becomes +0.0 in the buffer;
  * the norm is accumulated in double: denormal gradients give a non-zero norm where float32 squaring underflows (the clip factor
    is 1 either way);
  * skip_nonfinite=True: a step whose gradient norm is NaN or inf leaves every parameter and buffer untouched and sets stats[2];
    False applies the formula as written (what torch does): inf gives a clip factor of 0, NaN propagates;
  * no dampening, no Nesterov momentum, one momentum and one max_norm for all groups; lr and weight_decay may differ per group;
  * `stats`: float32 [4] on the device = (total_norm, coef, nonfinite, 0) of the last step.  step() never syncs with the host.
state_dict() / load_state_dict() have torch.optim.SGD's layout (state[p]['momentum_buffer'], SGD's group keys), so a checkpoint of
the reference (train_fast.py:177-183) loads here and one of ours loads there; a missing buffer means zeros.
"""
import torch

from . import hip_optim


class ClippedSGD(torch.optim.Optimizer):
    def __init__(self, params, lr, momentum=0.9, weight_decay=1e-4, max_norm=35.0, skip_nonfinite=False, capturable=False):
        """capturable=True: step() uploads nothing, so that it can be captured in a graph after prepare(); lr and weight_decay then
        reach the kernels through set_lr_(lr) or by writing `hyper` (float32 [groups, 2] = (lr, wd) on the device) in place, outside
        the graph."""
        if not lr >= 0.0 or not weight_decay >= 0.0:
            raise ValueError("lr and weight_decay must be >= 0")
        if not 0.0 <= momentum < 1.0:
            raise ValueError("momentum must be in [0, 1)")
        if not max_norm > 0.0:
            raise ValueError("max_norm must be > 0 (float('inf'): no clipping)")
        # torch.optim.SGD's group keys, so that either optimizer loads the other's state_dict
        defaults = dict(lr=lr, momentum=momentum, dampening=0, weight_decay=weight_decay, nesterov=False, maximize=False,
                        foreach=None, differentiable=False, fused=None)
        super().__init__(params, defaults)
        if len(self.param_groups) > hip_optim.MAX_GROUPS:
            raise ValueError("at most %d parameter groups" % hip_optim.MAX_GROUPS)
        self.max_norm, self.skip_nonfinite, self.capturable = float(max_norm), bool(skip_nonfinite), bool(capturable)
        self.stats = self.hyper = None
        self._key = self._plan = None

    def _momentum(self):
        m = {float(g['momentum']) for g in self.param_groups}
        if len(m) != 1 or any(g.get('dampening', 0) or g.get('nesterov', False) or g.get('maximize', False) for g in self.param_groups):
            raise NotImplementedError("ClippedSGD: one momentum for all groups; no dampening, Nesterov momentum or maximize")
        return m.pop()

    def _hyper_rows(self):
        return [[float(g['lr']), float(g['weight_decay'])] for g in self.param_groups]

    def _gather(self):
        """(params, grads, bufs, group indices) of the parameters that have a gradient; creates the missing momentum buffers"""
        params, grads, bufs, groups = [], [], [], []
        for k, group in enumerate(self.param_groups):
            for p in group['params']:
                if p.grad is None:
                    continue
                if not p.is_cuda or not p.grad.is_cuda:
                    raise RuntimeError("detectorch_amd.optim.ClippedSGD runs on the GPU only (got a CPU parameter); there is no CPU "
                                       "fallback")
                if p.grad.is_sparse:
                    raise RuntimeError("ClippedSGD does not support sparse gradients")
                state = self.state[p]
                if state.get('momentum_buffer') is None:                 # a missing buffer means zeros
                    state['momentum_buffer'] = torch.zeros_like(p, memory_format=torch.contiguous_format)
                params.append(p); grads.append(p.grad); bufs.append(state['momentum_buffer']); groups.append(k)
        return params, grads, bufs, groups

    @torch.no_grad()
    def prepare(self):
        """What a step needs beside the arithmetic, without taking one: momentum buffers, the device table of the (parameter,
        gradient, buffer) addresses, the device copy of (lr, wd).  The table is cached and rebuilt, in memory of its own, when an
        address changes (zero_grad(set_to_none=True), load_state_dict).  step() calls it; call it yourself, with the gradients in
        place, before capturing step() in a graph.  -> False when no parameter has a gradient."""
        params, grads, bufs, groups = self._gather()
        if not params:
            return False
        key = (tuple((p.data_ptr(), g.data_ptr(), b.data_ptr(), p.numel(), k) for p, g, b, k in zip(params, grads, bufs, groups)),
               len(self.param_groups))
        dev, n_groups = params[0].device, len(self.param_groups)
        stale = self.stats is None or self.stats.device != dev or self.hyper.shape[0] != n_groups
        if (stale or key != self._key) and torch.cuda.is_current_stream_capturing():
            raise RuntimeError("ClippedSGD: the parameter, gradient or buffer addresses changed; call prepare() before the capture")
        if key != self._key:
            self._plan, self._key = hip_optim.make_plan(params, grads, bufs, groups, n_groups), key
        if stale:
            self.stats = torch.zeros(4, dtype=torch.float32, device=dev)
            self.hyper = torch.tensor(self._hyper_rows(), dtype=torch.float32, pin_memory=True).to(dev, non_blocking=True)
        return True

    @torch.no_grad()
    def step(self, closure=None):
        """One dtc_sgd_step over the parameters of all groups that have a gradient.  Not capturable: (lr, wd) go up from
        param_groups through a pinned staging copy on the current stream, every call.  No host sync."""
        loss = None
        if closure is not None:
            with torch.enable_grad():
                loss = closure()
        momentum = self._momentum()
        if not self.prepare():
            return loss
        if not self.capturable:
            # a fresh pinned block per step: the copy of an earlier step may still be reading the last one
            self.hyper.copy_(torch.tensor(self._hyper_rows(), dtype=torch.float32, pin_memory=True), non_blocking=True)
        hip_optim.sgd_step(self._plan, self.hyper, momentum, self.max_norm, self.stats, self.skip_nonfinite)
        return loss

    def load_state_dict(self, state_dict):
        """torch.optim.SGD's layout (its own state_dict loads); the device copies follow the loaded groups at the next step."""
        super().load_state_dict(state_dict)
        self._key = self._plan = self.stats = self.hyper = None

    def set_lr_(self, lr):
        """adjust_learning_rate for every group, param_groups and the device copy both (in place, on the current stream): the way
        to change the rate of a capturable optimizer between replays."""
        for g in self.param_groups:
            g['lr'] = lr
        if self.hyper is not None:
            self.hyper[:, 0].fill_(float(lr))
        return self
