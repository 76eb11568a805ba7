"""The 3-D estimation protocol of the reference's run/pose3d/estimate.py on the GPU.

The reference's driver loops over the 4-view groups on the host: triangulate, test the skeleton
against the expected limb lengths (``break_limb_length``, estimate.py:84-96), send the groups that
break them through the pictorial structure model with the grid centred on the triangulated root
(``--Mode combination``, estimate.py:227-246; ``pict_struct`` sends every group), and score the
result in every camera's frame, optionally after Procrustes alignment (``error_computing_3d``,
estimate.py:110-123), into mean / joint-wise / action-wise / before-after MPJPE (estimate.py:248-277).

Here every step is one launch per batch: ``estimate_poses`` joins posu_triangulate_dlt,
posu_limb_break and posu_rpsm_run; ``pose3d_errors`` is posu_pose3d_errors (csrc/pose3d.hip) and
``Pose3DMeter`` keeps the sums of the report on the device.  ``break_limb_length`` and
``error_computing_3d`` keep the reference's signatures for one pose.  The reference's pickle / h5
loaders and its argparse driver are not built.  There is no CPU path.
"""
import numpy as np
import torch

from posu import ops
from multiviews import pictorial, triangulate
from multiviews.body import HumanBody

MODES = ('triangulation', 'pict_struct', 'combination')


def _device():
    if not torch.cuda.is_available():
        raise RuntimeError('pose-unsupervised_amd runs the 3-D estimation protocol on the GPU; '
                           'no cuda device is visible')
    return torch.device('cuda', torch.cuda.current_device())


def _to_device(a, dev=None):
    """-> (f64 device tensor, was it a tensor).  A CPU tensor is refused like everywhere else."""
    if isinstance(a, torch.Tensor):
        ops.require_cuda(a)
        return a, True
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float64)).to(dev or _device()), False


# ------------------------------------------------------------------ limb check
def break_limb_length_batch(poses, limb_lengths, thres=0.4, body=None):
    """poses [G, J, 3]; limb_lengths as rpsm_batch takes them (a dict keyed (parent, child), a list of G
    dicts, [J] or [G, J] by child joint) -> flag [G]: some limb is off its expected length by more than
    thres * length.  numpy in, numpy bool out; a cuda tensor in, a uint8 device tensor out."""
    x, on_device = _to_device(poses)
    tree = pictorial._tree(body or HumanBody())
    # one dict: a single shared row; every other form as a row per group
    rows = (tree.by_child(limb_lengths) if isinstance(limb_lengths, dict)
            else pictorial._limb_rows(limb_lengths, tree, x.shape[0]))
    flag = ops.limb_break(x, torch.from_numpy(tree.parent).to(x.device), pictorial._dev_f64(rows, x.device), thres)
    return flag if on_device else flag.cpu().numpy().astype(bool)


def break_limb_length(skel, pred, limb_length, thres=0.4):
    """The reference's signature for one pose (estimate.py:84-96): skel a list of {'idx', 'children'}
    nodes, pred [J, 3], limb_length keyed (parent, child) -> bool."""
    x, _ = _to_device(pred)
    tree = pictorial._skeleton_tree(skel)
    limb = pictorial._dev_f64(tree.by_child(limb_length), x.device)
    flag = ops.limb_break(x.reshape(1, -1, 3), torch.from_numpy(tree.parent).to(x.device), limb, thres)
    return bool(flag.cpu().numpy()[0])


# ---------------------------------------------------------------------- errors
def pose3d_errors(poses, j3d_gt, R, T, procrustes=False, return_aligned=False):
    """poses [G, J, 3] world frame, j3d_gt [G, V, J, 3] camera frames, R [G, V, 3, 3], T [G, V, 3] ->
    err [G, V, J] (with return_aligned also the predictions in the camera frames, aligned onto the
    ground truth when procrustes is set).  numpy in, numpy out; cuda tensors stay on the device."""
    x, on_device = _to_device(poses)
    gt, R, T = (_to_device(a, x.device)[0] for a in (j3d_gt, R, T))
    out = ops.pose3d_errors(x, gt, R, T, procrustes=procrustes, return_aligned=return_aligned)
    if on_device:
        return out
    return tuple(o.cpu().numpy() for o in out) if return_aligned else out.cpu().numpy()


def error_computing_3d(point3d, j3d_set, R_set, T_set, Procrustes):
    """The reference's signature for one group (estimate.py:110-123): point3d [J, 3], V ground truths
    [J, 3], V rotations, V camera centres ([3, 1] or [3]), 'Yes' / 'No' -> list of V arrays [J]."""
    gt = np.stack([np.asarray(g, dtype=np.float64) for g in j3d_set])[None]
    R = np.stack([np.asarray(r, dtype=np.float64) for r in R_set])[None]
    T = np.stack([np.asarray(t, dtype=np.float64).reshape(3) for t in T_set])[None]
    err = pose3d_errors(np.asarray(point3d, dtype=np.float64)[None], gt, R, T, procrustes=(Procrustes == 'Yes'))
    return list(err[0])


# ----------------------------------------------------------------------- modes
def estimate_poses(camera_params, poses2d, heatmaps, boxes, limb_lengths, pairwise_constraint, config,
                   mode='combination', joints_vis=None, thres=0.4, root_idx=None):
    """camera_params / boxes: G*4 dicts (group-major, view-minor); poses2d [G*4, J, 2]; heatmaps
    [G*4, J, h, w]; limb_lengths / pairwise_constraint as rpsm_batch takes them -> (poses [G, J, 3]
    float64 on the device, info).

    'triangulation'  triangulate_poses alone (heatmaps, boxes, pairwise_constraint may be None);
    'pict_struct'    every group through rpsm_batch, the grid centred on its triangulated root;
    'combination'    the limb check on the triangulated poses, rpsm_batch on the groups it flags,
                     their results scattered back.  The flag vector is read once (G bytes), the only
                     device read; with no group flagged nothing more is launched.
    info = {'triangulated': the triangulated poses, 'refined': bool [G] on the host, 'count': int}.
    A joint seen by fewer than two views triangulates to zeros and will normally flag its group, as
    the reference's arithmetic has it."""
    if mode not in MODES:
        raise ValueError('estimate_poses: mode must be one of %s, got %r' % (', '.join(MODES), mode))
    dev = poses2d.device if isinstance(poses2d, torch.Tensor) else _device()
    if isinstance(poses2d, torch.Tensor):
        ops.require_cuda(poses2d)
        xy = poses2d
    else:
        xy = np.asarray(poses2d)
        xy = torch.from_numpy(np.ascontiguousarray(xy if xy.dtype == np.float32 else xy.astype(np.float64))).to(dev)
    dataset = getattr(config, 'DATASET', None)
    x0 = triangulate.triangulate_poses(camera_params, xy, joints_vis,
                                       no_distortion=bool(getattr(dataset, 'NO_DISTORTION', False)))
    groups, views = x0.shape[0], triangulate.NVIEWS
    info = {'triangulated': x0, 'refined': np.zeros(groups, dtype=bool), 'count': 0}
    if mode == 'triangulation' or groups == 0:
        return x0, info
    body = HumanBody()
    if root_idx is None:
        root_idx = getattr(dataset, 'ROOTIDX', None)
        root_idx = body.root_idx if root_idx is None else int(root_idx)
    tree = pictorial._tree(body)
    limbs = pictorial._limb_rows(limb_lengths, tree, groups)
    hm = heatmaps if isinstance(heatmaps, torch.Tensor) else torch.from_numpy(
        np.ascontiguousarray(heatmaps, dtype=np.float32)).to(dev)
    ops.require_cuda(hm)
    camera_params, boxes = list(camera_params)[:groups * views], list(boxes)[:groups * views]
    if mode == 'pict_struct':
        poses = pictorial.rpsm_batch(camera_params, hm, boxes, x0[:, root_idx], limbs, pairwise_constraint, config)
        info['refined'][:] = True
        info['count'] = groups
        return poses, info
    flag = ops.limb_break(x0, torch.from_numpy(tree.parent).to(dev), pictorial._dev_f64(limbs, dev), thres)
    refined = flag.cpu().numpy().astype(bool)          # the one device read of the mode
    idx = np.flatnonzero(refined)
    info['refined'], info['count'] = refined, int(idx.size)
    if idx.size == 0:
        return x0, info
    didx = torch.from_numpy(idx).to(dev)
    sub = [i * views + v for i in idx for v in range(views)]
    hm = hm.reshape((groups, views) + tuple(hm.shape[-3:]))[didx]
    fixed = pictorial.rpsm_batch([camera_params[i] for i in sub], hm, [boxes[i] for i in sub], x0[didx, root_idx],
                                 limbs[idx], pairwise_constraint, config)
    poses = x0.clone()
    poses[didx] = fixed
    return poses, info


# ----------------------------------------------------------------------- report
class Pose3DMeter:
    """The report of estimate.py:215-277 as sums on the device.  ``update`` only enqueues; ``summary``
    reads the sums once."""

    def __init__(self, num_joints, num_actions, device=None):
        self.J, self.A = int(num_joints), int(num_actions)
        self.device = device or _device()
        # [joint sums J | sum m, sum m^2 | action sums A | action hits A | before, after, refined]
        self.sums = torch.zeros(self.J + 2 + 2 * self.A + 3, dtype=torch.float64, device=self.device)
        self.samples = 0     # (group, camera) pairs seen: known from the shapes, never read back
        self.groups = 0
        self._before = False

    def update(self, err, actions, refined=None, err_before=None):
        """err [G, V, J] cuda (pose3d_errors of the final poses); actions [G] indices < num_actions;
        refined [G] booleans (info['refined']) and err_before [G, V, J] (the errors of
        info['triangulated']; only the refined groups' rows count) feed the before / after comparison."""
        ops.require_cuda(err, err_before)
        g, v, j = err.shape
        if j != self.J:
            raise ValueError('Pose3DMeter: errors of %d joints, the meter has %d' % (j, self.J))
        err = err.detach().to(torch.float64)
        s, J, A = self.sums, self.J, self.A
        per_sample = err.mean(dim=2)                    # np.mean(errors, 0) of the [J, samples] table
        per_group = err.mean(dim=(1, 2))                # np.mean(errs) of one group
        act = torch.as_tensor(actions, device=err.device).to(torch.int64).reshape(g)
        s[:J] += err.sum(dim=(0, 1))
        s[J] += per_sample.sum()
        s[J + 1] += (per_sample * per_sample).sum()
        # one-hot sums: an action outside [0, A) adds to no slot (an indexed add would fault on it)
        onehot = (act[:, None] == torch.arange(A, device=err.device)[None, :]).to(torch.float64)
        s[J + 2:J + 2 + A] += (onehot * per_group[:, None]).sum(dim=0)
        s[J + 2 + A:J + 2 + 2 * A] += onehot.sum(dim=0)
        if refined is not None:
            mask = torch.as_tensor(refined, device=err.device).reshape(g).to(torch.float64)
            if err_before is not None:
                self._before = True
                s[-3] += (err_before.detach().to(torch.float64).mean(dim=(1, 2)) * mask).sum()
            s[-2] += (per_group * mask).sum()
            s[-1] += mask.sum()
        self.samples += g * v
        self.groups += g

    def summary(self):
        """-> dict(mpjpe, joint_wise [J], variance (np.var of the per-sample means), action_wise
        {action: mean of its groups' means}, compare {'before', 'after'} or None when no group was
        refined, pict_struct_count, groups)."""
        s = self.sums.cpu().numpy()
        J, A, n = self.J, self.A, max(self.samples, 1)
        joint_wise = s[:J] / n
        mean_m = s[J] / n
        hits = s[J + 2 + A:J + 2 + 2 * A]
        count = int(round(s[-1]))
        return {'mpjpe': float(s[:J].sum() / (n * J)), 'joint_wise': joint_wise,
                'variance': float(s[J + 1] / n - mean_m * mean_m),
                'action_wise': {a: float(s[J + 2 + a] / hits[a]) for a in range(A) if hits[a] > 0},
                'compare': {'before': float(s[-3] / count) if self._before else float('nan'),
                            'after': float(s[-2] / count)} if count else None,
                'pict_struct_count': count, 'groups': self.groups}
