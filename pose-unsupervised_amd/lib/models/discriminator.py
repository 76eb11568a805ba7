"""The heatmap discriminator of the mutual-information loss (reference
lib/models/discriminator.py:225-242) on HIP kernels.

The module holds the reference's parameters and buffers under the reference's names
(``block_nonlinear.0.weight`` ... ``block_nonlinear.6.bias``), so its checkpoints load; the
layers themselves never run as torch modules.  Two entry points, both differentiable and both
honouring ``train()`` / ``eval()``:

* ``pair_scores(low_features, heatmaps, indices, joint_idx, nseg=1)``: the fused path of
  HeatmapMILoss -- the scores of all Q x Q (feature row, heatmap value) pairs per image without
  the [N Q Q, C + 1] pair tensor (csrc/heatmap_mi.hip);
* ``forward(embd)`` on a plain [R, c_in] tensor: the reference's signature, the same kernels at
  Q = 1, N = R (column 0 is the heatmap value, the rest one feature row per sample).

The other discriminators of the reference's file (LocalDiscriminator, GlobalDiscriminator,
ViewDiscriminator, JointsDiscriminator, DomainDiscriminator) are not part of this build.
"""
import torch
import torch.nn as nn

from posu import ops


def _not_built(name):
    def ctor(*args, **kwargs):
        raise NotImplementedError('%s is not part of this build (HeatmapDiscriminator is)' % name)
    ctor.__name__ = name
    return ctor


LocalDiscriminator = _not_built('LocalDiscriminator')
DomainDiscriminator = _not_built('DomainDiscriminator')
ViewDiscriminator = _not_built('ViewDiscriminator')
JointsDiscriminator = _not_built('JointsDiscriminator')


class HeatmapDiscriminator(nn.Module):
    def __init__(self, cfg):
        super(HeatmapDiscriminator, self).__init__()
        c_in = cfg.HEATMAP_DISCRIMINATOR.INPUT_CHANNELS
        c_m = cfg.HEATMAP_DISCRIMINATOR.INTER_CHANNELS
        if c_m not in (32, 64, 128):
            raise NotImplementedError('HEATMAP_DISCRIMINATOR.INTER_CHANNELS must be 32, 64 or 128, got %d' % c_m)
        if (c_in - 1) % 8 or c_in - 1 > 512 or c_in < 9:
            raise NotImplementedError('HEATMAP_DISCRIMINATOR.INPUT_CHANNELS - 1 must be a multiple of 8, at most '
                                      '512; got %d' % c_in)
        self.c_in, self.c_m = c_in, c_m
        # parameter holders only (names and shapes of the reference's nn.Sequential)
        self.block_nonlinear = nn.Sequential(
            nn.Linear(c_in, c_m, bias=False),
            nn.BatchNorm1d(c_m),
            nn.LeakyReLU(0.2),
            nn.Linear(c_m, c_m // 4),
            nn.BatchNorm1d(c_m // 4),
            nn.LeakyReLU(0.2),
            nn.Linear(c_m // 4, 1),
        )

    def _params(self):
        b = self.block_nonlinear
        return {'W1': b[0].weight, 'g1': b[1].weight, 'be1': b[1].bias, 'rm1': b[1].running_mean,
                'rv1': b[1].running_var, 'W2': b[3].weight, 'b2': b[3].bias, 'g2': b[4].weight, 'be2': b[4].bias,
                'rm2': b[4].running_mean, 'rv2': b[4].running_var, 'w3': b[6].weight, 'b3': b[6].bias}

    def _track(self, stats, nseg):
        """The running buffers after `nseg` successive train-mode calls (one per segment, in order):
        running = (1 - momentum) running + momentum batch, the unbiased variance into running_var."""
        c_m = self.c_m
        with torch.no_grad():
            for s in range(nseg):
                for bn, sl in ((self.block_nonlinear[1], slice(0, c_m)),
                               (self.block_nonlinear[4], slice(c_m, c_m + c_m // 4))):
                    bn.num_batches_tracked += 1
                    m = bn.momentum if bn.momentum is not None else 1.0 / float(bn.num_batches_tracked)
                    bn.running_mean.mul_(1.0 - m).add_(stats[s, 0, sl], alpha=m)
                    bn.running_var.mul_(1.0 - m).add_(stats[s, 2, sl], alpha=m)

    def pair_scores(self, low_features, heatmaps, indices, joint_idx, nseg=1):
        """u [B, Q, Q]: u[n, i, j] scores (feature row indices[n, i], heatmap value indices[n, j]) of
        image n -- the reference's row order (n, i, j).  B = nseg * N; BatchNorm statistics (and, in
        train mode, the running-buffer updates) are per segment, as nseg separate calls would be."""
        if low_features.shape[1] != self.c_in - 1:
            raise ValueError('HeatmapDiscriminator takes %d feature channels, got %d'
                             % (self.c_in - 1, low_features.shape[1]))
        bn1 = self.block_nonlinear[1]
        u, stats = ops.heatmap_pair_scores(low_features, heatmaps, indices, joint_idx, self._params(), nseg=nseg,
                                           training=self.training, eps=bn1.eps)
        if self.training:
            self._track(stats, nseg)
        return u

    def forward(self, embd):
        """[R, c_in] -> [R, 1] (reference discriminator.py:241-242)."""
        if embd.dim() != 2 or embd.shape[1] != self.c_in:
            raise ValueError('HeatmapDiscriminator.forward takes [R, %d], got %s' % (self.c_in, tuple(embd.shape)))
        r = embd.shape[0]
        feat = embd[:, 1:].reshape(r, self.c_in - 1, 1, 1)
        hm = embd[:, :1].reshape(r, 1, 1, 1)
        idx = torch.zeros((r, 1), dtype=torch.int32)
        return self.pair_scores(feat, hm, idx, 0, nseg=1).reshape(r, 1)
