"""Fundamental matrices from 2-D joints on the device: the producer of the {(subject, i, j): 3x3} table that
FundamentalLoss reads (core/loss.py), which the reference makes with cv2.findFundamentalMat(pts_i, pts_j,
cv2.FM_LMEDS) in run/test/generate_fundamental_matirx.py:36-103 and checks by the mean and max of
|x_j^T F x_i| (there and in run/test/test_fund_mtx.py:56-71).

estimate_fundamental is the estimator (posu_fundamental_lmeds: least median of squares over the normalised
8-point algorithm, include/posu.h); fundamental_matrix_dict lays a set of multi-view poses out as one
problem per subject and view pair, runs them in one call and reads the result back once;
epipolar_residuals is the generator's printed check.  The joints may be ground truth or the predictions
validate_device leaves on the device (result.locations, with their confidences as the validity).

There is no CPU path: CPU tensors given to the estimator and a machine without a device raise RuntimeError.
"""
import itertools
import os
import pickle

import numpy as np
import torch

from posu import ops
from posu._native import require_cuda

MIN_INLIERS = 8     # the reference's assert np.sum(mask) >= 8


def _device():
    if not torch.cuda.is_available():
        raise RuntimeError('pose-unsupervised_amd estimates fundamental matrices on the GPU; no cuda device is visible')
    return torch.device('cuda', torch.cuda.current_device())


def estimate_fundamental(pts_i, pts_j, valid=None, hypotheses=512, seed=0, refit=True):
    """P independent problems in one call: pts_i, pts_j [P, N, 2] cuda (f32 is promoted to f64), valid [P, N] or
    None -> (F [P, 3, 3] f64 with x_j^T F x_i = 0 and F[2][2] = 1, mask [P, N] uint8, info), all on the device.
    info: sample [P, 8] int32 (the winning rows), median, sigma [P] f64, n_inliers, best [P] int64.  A problem
    that kept fewer than 8 inliers has a zero matrix and n_inliers = 0."""
    require_cuda(pts_i, pts_j, valid)
    if pts_i.dim() != 3 or pts_i.shape[2] != 2 or tuple(pts_j.shape) != tuple(pts_i.shape):
        raise ValueError('estimate_fundamental: pts_i and pts_j must both be [P, N, 2], got %s and %s'
                         % (tuple(pts_i.shape), tuple(pts_j.shape)))
    pts = torch.cat([pts_i.detach().to(torch.float64), pts_j.detach().to(torch.float64)], dim=2)
    F, mask, sample, stats = ops.fundamental_lmeds(pts, valid, hypotheses, seed, refit)
    info = {'sample': sample, 'median': stats[:, 0], 'sigma': stats[:, 1], 'n_inliers': stats[:, 2].to(torch.int64),
            'best': stats[:, 3].to(torch.int64)}
    return F, mask, info


def _problems(poses, subjects, valid, min_confidence, frames, ordered=False):
    """poses [G, V, J, 2 or 3] (a tensor, on the device it is to stay on) -> (keys, pts_i, pts_j, valid): one
    problem per subject and view pair i < j (every ordered pair with `ordered`), its rows the joints of the
    subject's groups (frames='all') or of its first group ('first'), padded to the longest with valid = 0."""
    if frames not in ('all', 'first'):
        raise ValueError("fundamental_matrix_dict: frames must be 'all' or 'first', got %r" % (frames,))
    if poses.dim() != 4 or poses.shape[3] not in (2, 3):
        raise ValueError('fundamental_matrix_dict: poses2d must be [G, V, J, 2 or 3], got %s' % (tuple(poses.shape),))
    g, v, j, c = poses.shape
    subjects = [int(s) for s in np.asarray(subjects).reshape(-1)]
    if len(subjects) != g:
        raise ValueError('fundamental_matrix_dict: %d subjects for %d groups' % (len(subjects), g))
    if min_confidence is not None and c != 3:
        raise ValueError('fundamental_matrix_dict: min_confidence needs [G, V, J, 3] poses (x, y, confidence)')
    groups = {}
    for k, s in enumerate(subjects):
        if frames == 'all' or s not in groups:
            groups.setdefault(s, []).append(k)
    pairs = list(itertools.permutations(range(v), 2) if ordered else itertools.combinations(range(v), 2))
    n = max(len(ks) for ks in groups.values()) * j
    keys = [(s, a, b) for s in groups for a, b in pairs]
    grp = np.zeros((len(keys), n), dtype=np.int64)
    pad = np.zeros((len(keys), n), dtype=bool)
    for k, (s, _, _) in enumerate(keys):
        rows = np.repeat(np.asarray(groups[s], dtype=np.int64), j)
        grp[k, :len(rows)], pad[k, :len(rows)] = rows, True
    dev = poses.device
    # one upload: the group and joint of every row, the two views of every problem, the padding
    table = np.concatenate([grp.reshape(-1), np.tile(np.arange(n) % j, len(keys)),
                            np.array([k[1] for k in keys] + [k[2] for k in keys], dtype=np.int64),
                            pad.reshape(-1).astype(np.int64)])
    table = torch.from_numpy(table).to(dev)
    pn = len(keys) * n
    grp_d, jt_d = table[:pn].view(len(keys), n), table[pn:2 * pn].view(len(keys), n)
    vi_d, vj_d = table[2 * pn:2 * pn + len(keys)], table[2 * pn + len(keys):2 * pn + 2 * len(keys)]
    ok = table[2 * pn + 2 * len(keys):].view(len(keys), n).ne(0)
    xi, xj = poses[grp_d, vi_d[:, None], jt_d], poses[grp_d, vj_d[:, None], jt_d]
    if valid is not None:
        if tuple(valid.shape) != (g, v, j):
            raise ValueError('fundamental_matrix_dict: valid must be [G, V, J], got %s' % (tuple(valid.shape),))
        valid = valid.to(dev).ne(0)
        ok = ok & valid[grp_d, vi_d[:, None], jt_d] & valid[grp_d, vj_d[:, None], jt_d]
    if min_confidence is not None:
        ok = ok & (xi[:, :, 2] > min_confidence) & (xj[:, :, 2] > min_confidence)
    return keys, xi[:, :, :2], xj[:, :, :2], ok.to(torch.uint8)


def _on_device(poses2d, valid):
    if isinstance(poses2d, torch.Tensor) and poses2d.is_cuda:
        dev = poses2d.device
    else:
        dev = _device()
    poses = torch.as_tensor(poses2d).detach().to(dev)
    if valid is not None:
        valid = torch.as_tensor(np.asarray(valid) if not isinstance(valid, torch.Tensor) else valid).to(dev)
    return poses, valid


def fundamental_matrix_dict(poses2d, subjects, valid=None, min_confidence=None, frames='all', hypotheses=512, seed=0):
    """{(subject, i, j): float64 3x3} for every subject and ordered view pair, as FundamentalLoss takes it.

    poses2d [G, V, J, 2 or 3], host or device, group-major like the datasets' grouping (result.locations of
    validate_device reshaped to [G, V, J, 3] stays on the device); subjects [G] on the host; valid [G, V, J] or
    None.  With 3 channels and min_confidence a correspondence counts when both views' third channel exceeds
    it.  frames='all' uses every group of a subject, 'first' the subject's first group only (the reference's
    choice).  One problem per subject and pair i < j; the (s, j, i) entry is the transpose, which has the same
    scale (the reference estimates both orders on their own).  One read-back at the end.  ValueError names the
    key of a problem that kept fewer than 8 inliers (the reference asserts np.sum(mask) >= 8)."""
    poses, valid = _on_device(poses2d, valid)
    keys, xi, xj, ok = _problems(poses, subjects, valid, min_confidence, frames)
    F, _, info = estimate_fundamental(xi, xj, ok, hypotheses=hypotheses, seed=seed)
    back = torch.cat([F.reshape(len(keys), 9), info['n_inliers'].to(torch.float64)[:, None]], dim=1).cpu().numpy()
    out = {}
    for k, (s, a, b) in enumerate(keys):
        if back[k, 9] < MIN_INLIERS:
            raise ValueError('fundamental_matrix_dict: the problem of key %r kept fewer than %d inliers'
                             % ((s, a, b), MIN_INLIERS))
        out[(s, a, b)] = back[k, :9].reshape(3, 3).copy()
        out[(s, b, a)] = out[(s, a, b)].T.copy()
    return out


def fundamental_from_db(db, grouping, **kw):
    """The generator script's own input: the reference's records (db[k]['joints_2d'] [J, 2], db[k]['subject'])
    and grouping lists (one list of V record indices per group) -> fundamental_matrix_dict's result.  The
    reference reads the no_distortion annotation set here; so should the caller."""
    poses = np.stack([np.stack([np.asarray(db[k]['joints_2d'], dtype=np.float64)[:, :2] for k in items])
                      for items in grouping])
    subjects = [int(db[items[0]]['subject']) for items in grouping]
    return fundamental_matrix_dict(poses, subjects, **kw)


def epipolar_residuals(F_dict, poses2d, subjects, valid=None):
    """The check the generator prints: |x_j^T F x_i| over every group and joint of every key's subject and pair.
    -> {'mean', 'max'} over all of them and 'per_key': {key: (mean, max)}.  One read-back."""
    poses, valid = _on_device(poses2d, valid)
    keys, xi, xj, ok = _problems(poses, subjects, valid, None, 'all', ordered=True)
    missing = [k for k in keys if k not in F_dict]
    if missing:
        raise KeyError(missing[0])
    F = torch.from_numpy(np.stack([np.asarray(F_dict[k], dtype=np.float64) for k in keys])).to(poses.device)
    pts = torch.cat([xi.to(torch.float64), xj.to(torch.float64)], dim=2)
    stats = ops.epipolar_residual_stats(F, pts, ok)
    back = torch.cat([stats, ok.sum(dim=1, dtype=torch.float64)[:, None]], dim=1).cpu().numpy()
    total = back[:, 2].sum()
    return {'mean': float((back[:, 0] * back[:, 2]).sum() / total) if total else 0.0,
            'max': float(back[:, 1].max()),
            'per_key': {k: (float(back[i, 0]), float(back[i, 1])) for i, k in enumerate(keys)}}


def save_fundamental_dict(path, d):
    """Write the pickle FundamentalLoss(cfg) opens: <DATASET.ROOT>/testdata/fundamental_matrix.pkl."""
    folder = os.path.dirname(str(path))
    if folder:
        os.makedirs(folder, exist_ok=True)
    with open(path, 'wb') as f:
        pickle.dump({(int(s), int(a), int(b)): np.asarray(m, dtype=np.float64) for (s, a, b), m in d.items()}, f)
