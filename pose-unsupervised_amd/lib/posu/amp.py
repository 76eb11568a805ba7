"""Dynamic loss scaling for fp16 training, with all of its state on the device.

fp16 storage needs the loss scaled up before the backward (with N(0, 1e-3) initial weights and an
MSE averaged over the heatmap pixels, the activation gradients lie below fp16's normal range), the
gradients scaled back down before the update, and a step that overflowed skipped.  torch's
GradScaler does this for its own optimizers; its unfused path reads ``found_inf`` back every step,
which stops the host from running ahead of the GPU-bound training step.  LossScaler keeps the same
interface and semantics and never reads the device in the training loop:

    scaler = LossScaler()
    net = get_pose_net(cfg, True, precision='fp16', loss_scaler=scaler)
    opt = posu.optim.Adam(net.parameters(), lr, capturable=True)
    ...
    scaler.scale(loss).backward()
    scaler.step(opt)
    scaler.update()

``step`` runs one pass over the gradients (posu_grad_stats: the overflow flag and the sum of
squares) and hands ``grad_scale`` / ``found_inf`` to the capturable posu.optim.Adam, whose kernels
divide by the scale and return before any store when the flag is set (posu_adam_step_dev);
``update`` is torch's ``_amp_update_scale_`` as a one-thread kernel (posu_loss_scale_update).  Only
``get_scale()``, ``found_inf()`` and ``state_dict()`` synchronise.  ``step(opt); update()`` can be
captured in a graph.

Under DistributedDataParallel the gradients a rank sees are the all-reduced ones: a non-finite
value on one rank is non-finite on all of them after the all-reduce, so every rank sets its flag
and skips the same step without a further collective.
"""
import torch

from . import _native as nat
from . import optim

_READY, _UNSCALED, _STEPPED = 'ready', 'unscaled', 'stepped'


class LossScaler:
    def __init__(self, init_scale=2. ** 16, growth_factor=2., backoff_factor=.5, growth_interval=2000, enabled=True):
        if enabled:
            if not growth_factor >= 1.0:
                raise ValueError('The growth factor must be >= 1.0.')
            if not 0.0 < backoff_factor <= 1.0:
                raise ValueError('The backoff factor must be in (0, 1].')
            if int(growth_interval) < 1:
                raise ValueError('The growth interval must be >= 1.')
        self._enabled = bool(enabled)
        self._init_scale = float(init_scale)
        self._init_tracker = 0
        self._growth_factor = float(growth_factor)
        self._backoff_factor = float(backoff_factor)
        self._growth_interval = int(growth_interval)
        self._scale = None      # f32 0-dim, on the device of the first loss / gradient
        self._tracker = None    # i32 0-dim: clean steps since the scale last changed
        self._per_optimizer = {}   # id(optimizer) -> {'stage', 'stats': optim.GradStats}
        self._last_found = None

    def is_enabled(self):
        return self._enabled

    def _state(self, device):
        if self._scale is None:
            self._scale = torch.full((), self._init_scale, dtype=torch.float32, device=device)
            self._tracker = torch.full((), self._init_tracker, dtype=torch.int32, device=device)
        elif self._scale.device != device:
            raise RuntimeError('LossScaler: its state is on %s, got a tensor on %s' % (self._scale.device, device))
        return self._scale

    def _of(self, optimizer):
        st = self._per_optimizer.get(id(optimizer))
        if st is None:
            st = self._per_optimizer[id(optimizer)] = {'stage': _READY, 'stats': None}
        return st

    @staticmethod
    def _grads(optimizer):
        return [p.grad for group in optimizer.param_groups for p in group['params'] if p.grad is not None]

    def _run_stats(self, optimizer, st, unscale):
        grads = self._grads(optimizer)
        if not grads:
            raise RuntimeError('LossScaler: the optimizer has no gradients')
        nat.require_cuda(*grads)
        scale = self._state(grads[0].device)
        if st['stats'] is None:
            st['stats'] = optim.GradStats(grads[0].device)
        st['stats'].run(grads, scale=scale if unscale else None, unscale=unscale)

    # ------------------------------------------------------------------ the training loop
    def scale(self, loss):
        """loss * scale, a device scalar product (autograd scales every gradient by it)."""
        if not self._enabled:
            return loss
        nat.require_cuda(loss)
        return loss * self._state(loss.device)

    def unscale_(self, optimizer):
        """Divide the optimizer's gradients by the scale in place (and record whether any was
        non-finite), for callers that look at the gradients before step()."""
        if not self._enabled:
            return
        st = self._of(optimizer)
        if st['stage'] != _READY:
            raise RuntimeError('unscale_() has already been called on this optimizer since the last update().'
                               if st['stage'] == _UNSCALED else 'unscale_() is being called after step().')
        with torch.no_grad():
            self._run_stats(optimizer, st, unscale=True)
        st['stage'] = _UNSCALED

    def step(self, optimizer, *args, **kwargs):
        """optimizer.step() on the unscaled gradients, skipped on the device when a gradient is
        non-finite.  Only a capturable posu.optim.Adam can do that without reading the flag back."""
        if not (isinstance(optimizer, optim.Adam) and optimizer.capturable):
            raise TypeError('LossScaler.step: needs a posu.optim.Adam(capturable=True), got %s'
                            % type(optimizer).__name__)
        if not self._enabled:
            return optimizer.step(*args, **kwargs)
        if 'closure' in kwargs or args:
            raise RuntimeError('Closure use is not supported with a loss scaler.')
        st = self._of(optimizer)
        if st['stage'] == _STEPPED:
            raise RuntimeError('step() has already been called since the last update().')
        if st['stage'] == _READY:
            with torch.no_grad():
                self._run_stats(optimizer, st, unscale=False)
        stats = st['stats']
        optimizer.grad_scale = self._scale if st['stage'] == _READY else None
        optimizer.found_inf = stats.found_inf
        optimizer.grad_sumsq = stats.sumsq
        try:
            out = optimizer.step()
        finally:
            del optimizer.grad_scale, optimizer.found_inf, optimizer.grad_sumsq
        st['stage'] = _STEPPED
        return out

    def update(self):
        """Halve the scale after an overflowed step, double it after growth_interval clean ones."""
        if not self._enabled:
            return
        found = [st['stats'].found_inf for st in self._per_optimizer.values() if st['stage'] != _READY]
        if not found:
            raise RuntimeError('No inf checks were recorded prior to update.')
        flag = found[0] if len(found) == 1 else torch.stack(found).sum()
        with torch.cuda.device(flag.device):
            nat.call('posu_loss_scale_update', nat.ptr(self._scale), nat.ptr(self._tracker), nat.ptr(flag),
                     self._growth_factor, self._backoff_factor, self._growth_interval, nat.stream_of(flag.device))
        self._last_found = flag
        for st in self._per_optimizer.values():
            st['stage'] = _READY

    # ------------------------------------------------------------------ these synchronise
    def get_scale(self):
        if not self._enabled:
            return 1.0
        return self._init_scale if self._scale is None else float(self._scale.item())

    def found_inf(self):
        """Whether the last inspected gradients (unscale_ / step) held an inf or a nan."""
        live = [st['stats'].found_inf for st in self._per_optimizer.values() if st['stage'] != _READY]
        flags = live or ([self._last_found] if self._last_found is not None else [])
        return any(float(f.item()) != 0.0 for f in flags)

    def state_dict(self):
        if not self._enabled:
            return {}
        return {'scale': self.get_scale(), 'growth_factor': self._growth_factor,
                'backoff_factor': self._backoff_factor, 'growth_interval': self._growth_interval,
                '_growth_tracker': self._init_tracker if self._tracker is None else int(self._tracker.item())}

    def load_state_dict(self, state_dict):
        if not self._enabled:
            return
        if len(state_dict) == 0:
            raise RuntimeError('The source state dict is empty, possibly because it was saved from a disabled '
                               'instance of LossScaler.')
        self._init_scale = float(state_dict['scale'])
        self._growth_factor = float(state_dict['growth_factor'])
        self._backoff_factor = float(state_dict['backoff_factor'])
        self._growth_interval = int(state_dict['growth_interval'])
        self._init_tracker = int(state_dict['_growth_tracker'])
        if self._scale is not None:
            self._scale.fill_(self._init_scale)
            self._tracker.fill_(self._init_tracker)
