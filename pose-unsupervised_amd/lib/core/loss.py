"""Hot-path losses (reference lib/core/loss.py) on HIP kernels.

* JointsMSELoss (loss.py:64-86): weighted per-joint heatmap MSE, one fused
  reduction kernel + its backward.
* MeanMSELoss: nn.MSELoss(reduction='mean') on the same kernels, differentiable in both arguments
  (what the training loop's consistent loss needs: both of its inputs carry gradients).
* FundamentalLoss (loss.py:89-133): epipolar residual |x_j^T F_{s,i,j} x_i| over the
  V(V-1) ordered view pairs, one kernel for the whole batch (the reference issues
  B x 12 small matmuls from a Python loop) + its backward.  The fundamental matrices
  are read from ``<DATASET.ROOT>/testdata/fundamental_matrix.pkl`` like the reference
  ({(subject, i, j): 3x3}), or given directly as a dict.
* ReprojectionLoss (no reference counterpart): its n-view sibling.  All views are triangulated (fp64 DLT,
  optionally confidence-weighted), the point is projected back into every view and the pixel distance to
  the predictions is the loss; the backward goes through the projection, the smallest singular vector and
  the undistortion (csrc/triangulate_grad.hip).

* HeatmapMILoss (loss.py:636-781): the mutual information (JSD or InfoNCE) between the
  sampled heatmap values of one joint and the backbone's low-level feature rows, scored by
  HeatmapDiscriminator over all Q x Q pairs per image.  The reference materialises the pairs as
  a [N Q Q, C + 1] tensor; here the pair scores, their backward and the measures are kernels
  that never form it (csrc/heatmap_mi.hip), and ``views`` runs the reference's per-view calls
  (function.py:266-267 / 276-277) as one call with per-view BatchNorm statistics.

The reference's other discriminator losses -- MILoss (its gradient penalty needs a double
backward through the kernels), ViewMILoss, JointsMILoss and the domain loss -- are outside this
build and raise if asked for.
"""
import itertools
import os
import pickle

import numpy as np
import torch

from posu import ops


class JointsMSELoss(torch.nn.Module):
    def __init__(self, use_target_weight):
        super(JointsMSELoss, self).__init__()
        self.use_target_weight = use_target_weight

    def forward(self, output, target, target_weight):
        w = target_weight if self.use_target_weight else None
        return ops.joints_mse(output, target, w)


class MeanMSELoss(torch.nn.Module):
    """torch.nn.MSELoss(reduction='mean') of two [N, J, ...] f32 cuda tensors on the JointsMSE kernels, with
    a gradient for both arguments: a drop-in for the ``criterion_dict['mse']`` that the training loop's
    consistent loss calls (function.py:294)."""

    def forward(self, input, target):
        return ops.mse_mean(input, target)


class FundamentalLoss:
    def __init__(self, cfg, fundamental_matrix_dict=None, device=None):
        self.use_target_weight = cfg.LOSS.USE_TARGET_WEIGHT_FUND
        if fundamental_matrix_dict is None:
            path = os.path.join(cfg.DATASET.ROOT, 'testdata', 'fundamental_matrix.pkl')
            with open(path, 'rb') as f:  # the user's own data file, as in the reference
                fundamental_matrix_dict = pickle.load(f)
        if device is None:
            if torch.distributed.is_available() and torch.distributed.is_initialized():
                device = torch.device('cuda', torch.distributed.get_rank() % max(torch.cuda.device_count(), 1))
            else:
                device = torch.device('cuda', torch.cuda.current_device())
        self.device = device
        self.fundamental_matrix_dict = fundamental_matrix_dict
        keys = list(fundamental_matrix_dict.keys())
        self.subjects = sorted({k[0] for k in keys})
        self.nviews = 1 + max(max(k[1], k[2]) for k in keys)
        self.pairs = list(itertools.permutations(range(self.nviews), 2))
        table = np.zeros((len(self.subjects), len(self.pairs), 3, 3), dtype=np.float32)
        self._missing = {}  # subject -> first (subject, i, j) key absent from the dict
        for si, s in enumerate(self.subjects):
            for pi, (i, j) in enumerate(self.pairs):
                if (s, i, j) in fundamental_matrix_dict:
                    table[si, pi] = np.asarray(fundamental_matrix_dict[(s, i, j)], dtype=np.float32)
                else:
                    self._missing.setdefault(s, (s, i, j))
        self.F = torch.from_numpy(table).to(device)
        self._subj_index = {s: i for i, s in enumerate(self.subjects)}

    def subject_indices(self, subjects):
        """Rows of the F table; a subject without an entry, or with a (subject, i, j) pair
        missing from the dict, raises KeyError like the reference's dict lookup
        (loss.py:127) -- never a silent zero matrix."""
        subjects = np.asarray(subjects).tolist()
        for s in subjects:
            if s in self._missing:
                raise KeyError(self._missing[s])
        idx = np.array([self._subj_index[s] for s in subjects], dtype=np.int32)
        return torch.from_numpy(idx).to(self.device)

    def __call__(self, joints_2d_list, target_weight, meta):
        """joints_2d_list: V x [K, J, 2] image px (cuda); target_weight: V x [K, J, 1]; meta: V dicts."""
        assert isinstance(joints_2d_list[0], torch.Tensor)
        batch_size = joints_2d_list[0].shape[0]
        subject = meta[0]['subject']
        subject = subject.numpy() if isinstance(subject, torch.Tensor) else np.asarray(subject)
        assert batch_size == len(subject)
        assert len(joints_2d_list) == self.nviews
        x = torch.stack(joints_2d_list, dim=0)
        w = None
        if self.use_target_weight:
            w = torch.stack([t.reshape(batch_size, -1) for t in target_weight], dim=0)
        return ops.epipolar_loss(x, w, self.F, self.subject_indices(subject))


class ReprojectionLoss:
    """The n-view counterpart of FundamentalLoss (no reference counterpart: the quantity the pseudo-label
    round computes offline as its reprojected labels, as a loss): the predictions of all views are
    triangulated, the point is projected back into every view with the lens model, and the pixel distance
    to the predictions is averaged (ops.reprojection_loss; 2 to 4 views).

    camera_dict: {(subject, view): camera dict in the H36M layout}; it becomes the [S, V, 3, 4] / [S, V, 9]
    device tables of multiviews.triangulate.camera_table (DATASET.NO_DISTORTION honoured), gathered per
    sample by meta[0]['subject'] on the device."""

    def __init__(self, cfg, camera_dict, device=None):
        from multiviews.triangulate import camera_table
        self.use_target_weight = getattr(cfg.LOSS, 'USE_TARGET_WEIGHT_REPROJ', True)
        self.no_distortion = bool(getattr(cfg.DATASET, 'NO_DISTORTION', False))
        if device is None:
            if torch.distributed.is_available() and torch.distributed.is_initialized():
                device = torch.device('cuda', torch.distributed.get_rank() % max(torch.cuda.device_count(), 1))
            else:
                device = torch.device('cuda', torch.cuda.current_device())
        self.device = device
        keys = list(camera_dict.keys())
        self.subjects = sorted({k[0] for k in keys})
        self.nviews = 1 + max(k[1] for k in keys)
        M = np.zeros((len(self.subjects), self.nviews, 3, 4))
        intr = np.zeros((len(self.subjects), self.nviews, 9))
        self._missing = {}  # subject -> first (subject, view) key absent from the dict
        for si, s in enumerate(self.subjects):
            for v in range(self.nviews):
                if (s, v) in camera_dict:
                    M[si, v], intr[si, v] = camera_table(camera_dict[(s, v)], self.no_distortion)
                else:
                    self._missing.setdefault(s, (s, v))
        self.M = torch.from_numpy(M).to(device)
        self.intr = torch.from_numpy(intr).to(device)
        self._subj_index = {s: i for i, s in enumerate(self.subjects)}

    def subject_indices(self, subjects):
        """Rows of the camera tables; a subject without cameras, or with a (subject, view) missing from the
        dict, raises KeyError like FundamentalLoss.subject_indices -- never a silent zero camera."""
        subjects = np.asarray(subjects).tolist()
        for s in subjects:
            if s in self._missing:
                raise KeyError(self._missing[s])
            if s not in self._subj_index:
                raise KeyError((s, 0))
        idx = np.array([self._subj_index[s] for s in subjects], dtype=np.int64)
        return torch.from_numpy(idx).to(self.device)

    def __call__(self, joints_2d_list, target_weight, meta, confidence=None, detach_point=False):
        """joints_2d_list: V x [K, J, 2] image px (cuda); target_weight: V x [K, J, 1]; meta: V dicts -- what
        the training loop hands to criterion_dict['fundamental'].  confidence: None or V x [K, J] (or
        [K, J, 1]) weights of each view's DLT rows, differentiable.  detach_point: the triangulated point is
        a constant and only the direct term reaches the predictions."""
        assert isinstance(joints_2d_list[0], torch.Tensor)
        ops.require_cuda(*joints_2d_list)
        batch_size = joints_2d_list[0].shape[0]
        subject = meta[0]['subject']
        subject = subject.cpu().numpy() if isinstance(subject, torch.Tensor) else np.asarray(subject)
        assert batch_size == len(subject)
        assert len(joints_2d_list) == self.nviews
        idx = self.subject_indices(subject)
        x = torch.stack(joints_2d_list, dim=0)                    # view-major [V, K, J, 2], as the kernels read it
        w = None
        if self.use_target_weight and target_weight is not None:
            w = torch.stack([t.reshape(batch_size, -1) for t in target_weight], dim=1)
        c = None
        if confidence is not None:
            c = torch.stack([t.reshape(batch_size, -1) for t in confidence], dim=1)
        return ops.reprojection_loss(self.M.index_select(0, idx), self.intr.index_select(0, idx), x, None, c, w,
                                     undistort=not self.no_distortion, view_major=True,
                                     detach_point=detach_point)


def _not_built(name, why):
    def ctor(*args, **kwargs):
        raise NotImplementedError('%s is not part of this build: %s' % (name, why))
    ctor.__name__ = name
    return ctor


MILoss = _not_built('MILoss', 'its gradient penalty needs a double backward through the kernels')
ViewMILoss = _not_built('ViewMILoss', 'only HeatmapMILoss is built')
JointsMILoss = _not_built('JointsMILoss', 'only HeatmapMILoss is built')


class HeatmapMILoss:
    """Reference lib/core/loss.py:636-781.  Constructor and ``__call__`` are the reference's (one
    view in, the scalar loss out); ``sample_indices`` exposes the position sampling, ``indices=``
    takes positions drawn elsewhere, and ``views`` sums the loss over a list of views in one call.

    sampler='host' (the default) draws the positions with torch on the host, like the reference; it reads
    the two meta entries, which is a synchronisation when they live on the device.  sampler='device'
    draws them with a counter-based kernel (``sample_indices_device``) from `seed` (None: one value from
    torch's default generator at construction) and the number of draws made so far, and nothing between
    the metadata and the loss touches the host.  ``sampler_state`` / ``load_sampler_state`` carry
    {'seed', 'calls'} through a checkpoint.  DDP ranks need different seeds (a caller who passes `seed`
    adds the rank).  The sampling is not graph-capturable: the call number is a by-value argument."""

    MAP = 64   # the reference asserts 64 x 64 low-level and heatmap maps (loss.py:686, 714-716)

    def __init__(self, cfg, discriminator_dict, sampler='host', seed=None):
        if sampler not in ('host', 'device'):
            raise ValueError("HeatmapMILoss sampler must be 'host' or 'device', got %r" % (sampler,))
        self.sampler = sampler
        self._seed, self._calls = None, 0
        if sampler == 'device':
            # one 63-bit value from torch's default host generator, so torch.manual_seed repeats a run
            self._seed = int(seed) if seed is not None else int(torch.randint(0, 2 ** 63 - 1, (1,)).item())
        self.use_target_weight = cfg.LOSS.USE_TARGET_WEIGHT
        self.measure = cfg.LOSS.HEATMAP_MI_MEASURE
        if self.measure not in ops.MI_MEASURES:
            raise NotImplementedError('LOSS.HEATMAP_MI_MEASURE %r (JSD and NCE are built)' % (self.measure,))
        self.sigma = cfg.NETWORK.SIGMA
        # image px per heatmap px, (w, h)
        self.feat = torch.as_tensor(np.asarray(cfg.NETWORK.IMAGE_SIZE, dtype=np.float64)
                                    / np.asarray(cfg.NETWORK.HEATMAP_SIZE, dtype=np.float64))
        self.heatmap_d = discriminator_dict['heatmap_discriminator']

    # -- sampling (host-side torch, as in the reference: loss.py:646-672, 691-703)
    def window(self, loc):
        """The (2r + 1)^2 linear positions around `loc` [N], r = 3 sigma + 2, clamped to the map
        (the linear index is clamped, like the reference's, so a window at the border repeats
        positions): [N, P]."""
        r = int(self.sigma * 3 + 2)
        off = torch.arange(-r, r + 1)
        grid = (off[:, None] * self.MAP + off[None, :]).reshape(-1)
        return (loc.reshape(-1, 1).long() + grid[None, :]).clamp(0, self.MAP * self.MAP - 1)

    def locations(self, meta, joint_idx, generator=None):
        """Per image the window centre: the ground-truth joint (joints_2d_transformed / feat + 0.5,
        truncated, clamped to the map) when it is visible, a uniformly random position otherwise.
        Image n keeps slot n (the reference moves the invisible joints' random draws to the end of
        the batch, loss.py:697-699; which image a random centre lands on does not matter to it)."""
        m = self.MAP
        j2d = torch.as_tensor(meta['joints_2d_transformed']).double().cpu()
        gt = (j2d / self.feat + 0.5).long().clamp(0, m - 1)
        gt = (gt[:, :, 1] * m + gt[:, :, 0])[:, joint_idx]
        vis = torch.as_tensor(meta['joints_vis']).cpu()[:, joint_idx, 0] != 0
        rnd = torch.randint(0, m * m, gt.shape, generator=generator)
        return torch.where(vis, gt, rnd)

    def sample_indices(self, meta, joint_idx, generator=None, return_locations=False):
        """[N, P // 2 + P // 4] positions: half of the window's P entries without replacement, then a
        quarter as many distinct positions from outside the window."""
        m = self.MAP
        loc = self.locations(meta, joint_idx, generator)
        win = self.window(loc)
        n, p = win.shape
        pick = torch.rand(n, p, generator=generator).argsort(dim=1)[:, :p // 2]
        inside = win.gather(1, pick)
        score = torch.rand(n, m * m, generator=generator)
        score.scatter_(1, win, -1.0)
        outside = score.topk(p // 4, dim=1).indices
        idx = torch.cat([inside, outside], dim=1)
        return (idx, loc) if return_locations else idx

    # -- sampling on the device (posu_heatmap_mi_sample, include/posu.h)
    def sample_indices_device(self, meta, joint_idx, return_locations=False):
        """sample_indices on the device, for one meta dict ([N, Q] int32 cuda) or a list of them (one launch
        over the concatenated rows, view-major: [V N, Q], row k = v N + n).  The metadata may live on the
        host or on the device; it is uploaded, never read back.  Every launch uses call number
        ``self._calls`` and then increments it, and row k's draw depends on (seed, call, k) alone, so a
        seed and a call count name the whole sequence (``sampler_state``).  Under DDP every rank needs its
        own seed: ``seed=None`` draws it from the rank's torch generator, a caller who passes ``seed`` adds
        the rank.  The call number is a by-value kernel argument, so the sampling cannot be captured in a
        graph (a replay would repeat one draw)."""
        if self.sampler != 'device':
            raise RuntimeError("sample_indices_device needs HeatmapMILoss(..., sampler='device')")
        metas = [meta] if isinstance(meta, dict) else list(meta)
        joints = [torch.as_tensor(m['joints_2d_transformed']) for m in metas]
        vis = [torch.as_tensor(m['joints_vis']) for m in metas]
        dev = next((t.device for t in joints + vis if t.is_cuda), None)
        if dev is None:
            if not torch.cuda.is_available():
                ops.require_cuda(*joints)    # no GPU: the library's refusal, never a host fallback
            dev = torch.device('cuda', torch.cuda.current_device())
        vis = [v[:, :, 0] if v.dim() == 3 else v for v in vis]
        joints = torch.cat([t.to(device=dev, dtype=torch.float64) for t in joints], dim=0)
        vis = torch.cat([t.to(device=dev, dtype=torch.float64) for t in vis], dim=0)
        idx, loc = ops.heatmap_mi_sample(joints, vis, joint_idx, (float(self.feat[0]), float(self.feat[1])),
                                         (self.MAP, self.MAP), int(self.sigma * 3 + 2), self._seed, self._calls)
        self._calls += 1
        return (idx, loc) if return_locations else idx

    def sampler_state(self):
        """{'seed', 'calls'} of the device sampler, for a checkpoint."""
        return {'seed': self._seed, 'calls': self._calls}

    def load_sampler_state(self, state):
        if self.sampler != 'device':
            raise RuntimeError("load_sampler_state needs HeatmapMILoss(..., sampler='device')")
        self._seed, self._calls = int(state['seed']), int(state['calls'])

    def _check_maps(self, low_features, high_features):
        if tuple(low_features.shape[2:]) != (self.MAP, self.MAP) or tuple(high_features.shape[2:]) != (self.MAP,
                                                                                                      self.MAP):
            raise NotImplementedError('HeatmapMILoss takes 64 x 64 maps (like the reference), got low %s, high %s'
                                      % (tuple(low_features.shape[2:]), tuple(high_features.shape[2:])))

    def __call__(self, low_features, high_features, target_weight, meta, joint_idx, indices=None):
        """low_features [N, C, 64, 64], high_features [N, J, 64, 64] (cuda), meta on the host (with
        sampler='device': on the host or on the device, and `indices` may be a cuda tensor)."""
        self._check_maps(low_features, high_features)
        if indices is None:
            indices = (self.sample_indices_device(meta, joint_idx) if self.sampler == 'device'
                       else self.sample_indices(meta, joint_idx))
        u = self.heatmap_d.pair_scores(low_features, high_features, indices, joint_idx, nseg=1)
        return ops.pair_mi_loss(u, self.measure, 1)[0]

    def views(self, low_list, out_list, weight_list, meta_list, joint_idx, indices=None):
        """sum over views of __call__ (function.py:266-267 / 276-277) as one call: the views are
        the segments of the kernels, each with its own BatchNorm statistics, and the running
        buffers end as after the per-view calls in order.  indices: None or one [N, Q] per view; with
        sampler='device' the positions of all views are drawn in one launch, and `indices` may also be
        cuda tensors (one [N, Q] per view or one [V N, Q]), which never leave the device."""
        nseg = len(low_list)
        for l, o in zip(low_list, out_list):
            self._check_maps(l, o)
        if indices is None and self.sampler == 'device':
            indices = self.sample_indices_device(list(meta_list), joint_idx)   # all views in one launch
        elif indices is None:
            indices = [self.sample_indices(m, joint_idx) for m in meta_list]
        low = low_list[0] if nseg == 1 else torch.cat(list(low_list), dim=0)
        out = out_list[0] if nseg == 1 else torch.cat(list(out_list), dim=0)
        if self.sampler == 'device' and isinstance(indices, torch.Tensor):
            idx = indices                                          # one [V N, Q], host or device
        elif self.sampler == 'device' and all(isinstance(i, torch.Tensor) and i.is_cuda for i in indices):
            idx = torch.cat(list(indices), dim=0)                  # stays on the device
        else:
            idx = torch.cat([torch.as_tensor(i).cpu() for i in indices], dim=0)
        u = self.heatmap_d.pair_scores(low, out, idx, joint_idx, nseg=nseg)
        return ops.pair_mi_loss(u, self.measure, nseg).sum()
