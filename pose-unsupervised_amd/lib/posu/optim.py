"""Adam on the HIP kernel (posu_adam_step, include/posu.h): a drop-in for the reference's
optimizer, torch.optim.Adam (utils/utils.py:79-83, stepped by core/function.py:366), for f32
parameters on the GPU.

Same hyper-parameters, state layout ('step', 'exp_avg', 'exp_avg_sq' per parameter, so
state_dict / load_state_dict and a switch to or from torch.optim.Adam keep working) and update
rule; the arithmetic is f32 and agrees with torch's kernels within rounding, not bit for bit.
Every parameter of a group with the same step count goes to one call (a few launches for the
whole network).  amsgrad / maximize / complex parameters are refused.

``capturable=True`` (posu_adam_step_dev) keeps the step counts on the device (f32 0-dim tensors,
torch's capturable convention) and computes the bias corrections there: step() never reads the
device back, can be captured in a graph, and honours a loss scaler's ``grad_scale`` /
``found_inf`` attributes (the convention of torch.amp.GradScaler for optimizers that set
``_step_supports_amp_scaling``; posu.amp.LossScaler uses the same): an overflowed step changes
neither the parameters nor the state.  ``max_grad_norm`` (capturable only) clips the gradients to
that global norm inside the update, as torch.nn.utils.clip_grad_norm_ before step() would.
"""
import ctypes

import numpy as np
import torch

from . import _native as nat

_REC = np.dtype([('p', '<u8'), ('g', '<u8'), ('m', '<u8'), ('v', '<u8'), ('n', '<i8')])
assert _REC.itemsize == 40   # sizeof(posu_adam_tensor)
_REC_DEV = np.dtype([('p', '<u8'), ('g', '<u8'), ('m', '<u8'), ('v', '<u8'), ('step', '<u8'), ('n', '<i8')])
assert _REC_DEV.itemsize == 48   # sizeof(posu_adam_dev_tensor)
_REC_GRAD = np.dtype([('g', '<u8'), ('n', '<i8')])
assert _REC_GRAD.itemsize == 16   # sizeof(posu_grad_tensor)


class GradStats:
    """posu_grad_stats over a list of f32 gradients of one device: the overflow flag and the sum of
    squares in device scalars that live as long as this object (found_inf f32, sumsq f64; the
    workspace grows when a larger table comes)."""

    def __init__(self, device):
        self.device = device
        self.found_inf = torch.zeros((), dtype=torch.float32, device=device)
        self.sumsq = torch.zeros((), dtype=torch.float64, device=device)
        self.workspace = None

    def run(self, grads, scale=None, unscale=False):
        rec = np.zeros(len(grads), dtype=_REC_GRAD)
        for i, g in enumerate(grads):
            if g.dtype != torch.float32 or g.is_sparse or not g.is_contiguous() or g.device != self.device:
                raise NotImplementedError('gradient statistics: dense contiguous f32 gradients of one device only')
            rec[i] = (g.data_ptr(), g.numel())
        table = rec.ctypes.data_as(ctypes.c_void_p)
        need = nat.load().posu_grad_stats_workspace(table, len(grads))
        if self.workspace is None or self.workspace.numel() < need:
            self.workspace = torch.empty(need, dtype=torch.uint8, device=self.device)
        with torch.cuda.device(self.device):
            nat.call('posu_grad_stats', table, len(grads), nat.ptr(scale), int(bool(unscale)), nat.ptr(self.found_inf),
                     nat.ptr(self.sumsq), nat.ptr(self.workspace), self.workspace.numel(), nat.stream_of(self.device))


class Adam(torch.optim.Adam):
    _step_supports_amp_scaling = False

    def __init__(self, params, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.0, capturable=False,
                 max_grad_norm=None):
        if capturable:
            super().__init__(params, lr=lr, betas=betas, eps=eps, weight_decay=weight_decay, capturable=True)
            # the scaler hands grad_scale / found_inf to step() instead of unscaling and skipping itself
            self._step_supports_amp_scaling = True
        else:
            if max_grad_norm is not None:
                raise ValueError('posu.optim.Adam: max_grad_norm needs capturable=True')
            super().__init__(params, lr=lr, betas=betas, eps=eps, weight_decay=weight_decay)
        self.capturable = bool(capturable)
        self.max_grad_norm = None if max_grad_norm is None else float(max_grad_norm)
        self._stats = {}   # device -> GradStats, for max_grad_norm without a scaler's sum of squares

    @staticmethod
    def _checked_params(group, state):
        """The group's parameters that have a gradient; every one is checked before any state
        changes: a refusal leaves the optimizer as it was."""
        if group.get('amsgrad') or group.get('maximize') or group.get('differentiable'):
            raise NotImplementedError('posu.optim.Adam: amsgrad / maximize / differentiable are not supported')
        params = [p for p in group['params'] if p.grad is not None]
        for p in params:
            if p.grad.is_sparse or p.is_complex() or p.dtype != torch.float32:
                raise NotImplementedError('posu.optim.Adam: dense f32 parameters only')
            nat.require_cuda(p, p.grad)
            st = state[p]
            if not p.is_contiguous() or (len(st) and not (st['exp_avg'].is_contiguous() and
                                                          st['exp_avg_sq'].is_contiguous())):
                raise NotImplementedError('posu.optim.Adam: contiguous parameters and state only')
        return params

    @torch.no_grad()
    def step(self, closure=None):
        loss = None
        if closure is not None:
            with torch.enable_grad():
                loss = closure()
        if self.capturable:
            self._step_dev()
            return loss
        for group in self.param_groups:
            params = self._checked_params(group, self.state)
            by_step = {}
            for p in params:
                st = self.state[p]
                if len(st) == 0:   # torch.optim.Adam's state (step on the host, as its non-fused form)
                    st['step'] = torch.tensor(0.0)
                    st['exp_avg'] = torch.zeros_like(p, memory_format=torch.contiguous_format)
                    st['exp_avg_sq'] = torch.zeros_like(p, memory_format=torch.contiguous_format)
                st['step'] += 1
                g = p.grad if p.grad.is_contiguous() else p.grad.contiguous()
                by_step.setdefault((int(st['step'].item()), p.device), []).append((p, g, st))
            beta1, beta2 = group['betas']
            for (step, dev), items in by_step.items():
                rec = np.zeros(len(items), dtype=_REC)
                for i, (p, g, st) in enumerate(items):
                    rec[i] = (p.data_ptr(), g.data_ptr(), st['exp_avg'].data_ptr(), st['exp_avg_sq'].data_ptr(),
                              p.numel())
                with torch.cuda.device(dev):
                    nat.call('posu_adam_step', rec.ctypes.data_as(ctypes.c_void_p), len(items), float(group['lr']),
                             float(beta1), float(beta2), float(group['eps']), float(group['weight_decay']), step,
                             nat.stream_of(dev))
        return loss

    def _step_dev(self):
        """The capturable step: nothing here reads the device."""
        grad_scale = getattr(self, 'grad_scale', None)
        found_inf = getattr(self, 'found_inf', None)
        sumsq = getattr(self, 'grad_sumsq', None)   # posu.amp.LossScaler's, of the gradients as stored
        work = []   # (group, device, [(p, g, state)])
        for group in self.param_groups:
            by_dev = {}
            for p in self._checked_params(group, self.state):
                st = self.state[p]
                if len(st) and not (torch.is_tensor(st['step']) and st['step'].is_cuda and
                                    st['step'].dtype == torch.float32 and st['step'].numel() == 1):
                    raise RuntimeError('posu.optim.Adam(capturable=True): the step counts are f32 tensors on the '
                                       "parameters' device")
                g = p.grad if p.grad.is_contiguous() else p.grad.contiguous()
                by_dev.setdefault(p.device, []).append((p, g, st))
            work += [(group, dev, items) for dev, items in by_dev.items()]
        for t in (grad_scale, found_inf, sumsq):
            if t is not None and any(t.device != dev for _, dev, _ in work):
                raise RuntimeError('posu.optim.Adam: grad_scale / found_inf are on another device than the parameters')
        max_norm = self.max_grad_norm or 0.0
        if max_norm > 0.0 and sumsq is None and work:
            # no scaler gave the sum of squares: one statistics pass over every group's gradients
            if len({dev for _, dev, _ in work}) > 1:
                raise NotImplementedError('posu.optim.Adam: max_grad_norm over several devices')
            dev = work[0][1]
            if dev not in self._stats:
                self._stats[dev] = GradStats(dev)
            self._stats[dev].run([g for _, _, items in work for _, g, _ in items])
            sumsq = self._stats[dev].sumsq
        for group, dev, items in work:
            fresh = [st for _, _, st in items if len(st) == 0]
            if fresh:   # the new step counts as views of one buffer
                steps = torch.zeros(len(fresh), dtype=torch.float32, device=dev)
                for k, st in enumerate(fresh):
                    st['step'] = steps[k]
            rec = np.zeros(len(items), dtype=_REC_DEV)
            for i, (p, g, st) in enumerate(items):
                if 'exp_avg' not in st:
                    st['exp_avg'] = torch.zeros_like(p, memory_format=torch.contiguous_format)
                    st['exp_avg_sq'] = torch.zeros_like(p, memory_format=torch.contiguous_format)
                rec[i] = (p.data_ptr(), g.data_ptr(), st['exp_avg'].data_ptr(), st['exp_avg_sq'].data_ptr(),
                          st['step'].data_ptr(), p.numel())
            beta1, beta2 = group['betas']
            with torch.cuda.device(dev):
                nat.call('posu_adam_step_dev', rec.ctypes.data_as(ctypes.c_void_p), len(items), float(group['lr']),
                         float(beta1), float(beta2), float(group['eps']), float(group['weight_decay']),
                         nat.ptr(found_inf), nat.ptr(grad_scale), nat.ptr(sumsq), float(max_norm), nat.stream_of(dev))
