"""MPJPE, as the reference's evaluation harness computes it (run/test/test_triangulate.py:84-102).

The harness maps both joint sets into one order (``u2a_mapping``: union index u ->
dataset index a, entries marked '*' dropped, sorted by u; test_triangulate.py:84-88),
selects ``pred3d[:, u]`` only when the 2-D inputs were the dataset's own (GT) joints
(:90-93, predictions read from the h5 file are already in union order) and
``gt3d[:, a]`` (:96), then reports the per-joint Euclidean error's mean, std, max and the
share of joints beyond mean + std (:98-102).

``mpjpe_stats`` is that arithmetic on host arrays (numpy, fp64); ``mpjpe_sums`` is the
device form used by the multi-rank evaluation: per-rank (error sum, squared-error sum,
count, max) that one small all-reduce combines (posu.dist.sum_over_ranks).

``evaluate_h36m`` / ``evaluate_mpii`` are the joint detection rates the reference's validation ends with
(``dataset.evaluate``: lib/dataset/multiview_h36m_compatible.py:184-234, lib/dataset/mpii_compatible.py:139-193)
for predictions that are on the device: one posu_detection_counts launch, one read-back of the integer
counts, and the reference's divisions on them."""
from collections import OrderedDict

import numpy as np
import torch


def u2a_indices(u2a_mapping):
    """(u, a) index arrays of test_triangulate.py:84-88 from a dataset's u2a mapping
    ({union index: dataset index or '*'})."""
    items = sorted(((k, v) for k, v in u2a_mapping.items() if v != '*'), key=lambda kv: kv[0])
    return np.array([k for k, _ in items]), np.array([v for _, v in items])


def mpjpe_stats(pred3d, gt3d, u=None, a=None, pred_in_union_order=True):
    """pred3d [N, J, 3], gt3d [N, Jd, 3] (mm) -> dict(mean, std, max, frac_above_mean_std,
    per_joint [N, J]).  u / a: the u2a index arrays (None: identity, same joint order)."""
    pred3d = np.asarray(pred3d, dtype=np.float64)
    gt3d = np.asarray(gt3d, dtype=np.float64)
    assert len(pred3d) == len(gt3d)
    pred = pred3d if (u is None or pred_in_union_order) else pred3d[:, u, :]
    gt = gt3d if a is None else gt3d[:, a, :]
    norm = np.linalg.norm(pred - gt, axis=2)
    mean, std = float(np.mean(norm)), float(np.std(norm))
    return {'mean': mean, 'std': std, 'max': float(np.amax(norm)),
            'frac_above_mean_std': float(np.sum(norm > mean + std) / norm.size), 'per_joint': norm}


def mpjpe_sums(pred3d, gt3d):
    """Device tensors [N, J, 3] -> [sum |e|, sum |e|^2, count, max |e|] (f64) for a
    multi-rank mean / std / max (combine the sums with a SUM and the max with a MAX)."""
    e = torch.linalg.norm(pred3d.double() - gt3d.double(), dim=2)
    return torch.stack([e.sum(), (e * e).sum(), torch.tensor(float(e.numel()), dtype=torch.float64,
                                                             device=e.device), e.max()])


def stats_from_sums(s, sq, count, mx):
    mean = s / count
    return {'mean': mean, 'std': float(np.sqrt(max(sq / count - mean * mean, 0.0))), 'max': mx}


# ------------------------------------------------------- joint detection rates
H36M_THRESHOLDS = (0.5, 0.4, 0.3, 0.2, 0.1)   # multiview_h36m_compatible.py:188 and :229
MPII_THRESHOLD = 0.5                          # mpii_compatible.py:143


def _cuda(x, dtype, device):
    if isinstance(x, torch.Tensor):
        return x.detach().to(device=device, dtype=dtype)
    return torch.from_numpy(np.ascontiguousarray(x)).to(device=device, dtype=dtype)


def _eval_device(*arrays):
    for x in arrays:
        if isinstance(x, torch.Tensor) and x.is_cuda:
            return x.device
    if not torch.cuda.is_available():
        raise RuntimeError('pose-unsupervised_amd evaluates on the GPU; no cuda device is visible')
    return torch.device('cuda', torch.cuda.current_device())


def _union_rows(x, u, k):
    """The dataset's array in union order -> the annotated joints ``[:, u]``; an array that already has the
    K annotated joints is taken as it is."""
    return x if x.shape[1] == k else x[:, torch.as_tensor(u, dtype=torch.long, device=x.device)]


def _counts(pred, gt, head, vis, thresholds, form, u):
    from . import ops
    dev = _eval_device(pred, gt, head, vis)
    pred = _cuda(pred, torch.float32, dev)
    if pred.dim() != 3 or pred.shape[1] != len(u) or pred.shape[2] < 2:
        raise ValueError('evaluate: pred must be [N, %d, 2 or 3] (the annotated union joints), got %s'
                         % (len(u), tuple(pred.shape)))
    gt = _union_rows(_cuda(gt, torch.float64, dev), u, len(u))[:, :, :2]
    if vis is not None:
        vis = _cuda(vis, torch.float64, dev)
        vis = _union_rows(vis[:, :, 0] if vis.dim() == 3 else vis, u, len(u))
    counts = ops.detection_counts(pred[:, :, :3].contiguous(), gt, _cuda(head, torch.float64, dev).reshape(-1),
                                  thresholds, form=form, vis=vis)
    return counts.cpu().numpy().astype(np.int64), pred.shape[0]   # the one read-back


def h36m_name_values(counts, nrows, u2a_mapping, actual_joints):
    """The table of multiview_h36m_compatible.py:217-234 from integer counts [5, 2, K] (or [5, K]: detected rows
    per joint at H36M_THRESHOLDS) over ``nrows`` frames: per joint name (``head`` left out) the rate at 0.5, then
    ``mean(15j)`` and ``mean@0.4`` .. ``mean@0.1`` -> (OrderedDict, mean(15j))."""
    _, a = u2a_indices(u2a_mapping)
    counts = np.asarray(counts).astype(np.int64)
    detected = counts[:, 0, :] if counts.ndim == 3 else counts
    if detected.shape != (len(H36M_THRESHOLDS), len(a)):
        raise ValueError('h36m_name_values: counts for %d thresholds and %d joints expected, got %s'
                         % (len(H36M_THRESHOLDS), len(a), detected.shape))
    rates = detected / float(nrows)                         # np.sum(detected, axis=0) / np.float(gt.shape[0])
    names = [actual_joints[k] for k in a]
    if 'head' not in names:
        raise ValueError("h36m_name_values: the mapping has no 'head' joint (the reference leaves it out of the mean)")
    head_idx = len(names) - 1 - names[::-1].index('head')
    name_values = OrderedDict()
    for i, name in enumerate(names):
        if name != 'head':
            name_values[name] = rates[0, i]
    name_values['mean(15j)'] = np.mean(np.delete(rates[0], head_idx))
    for t, thr in enumerate(H36M_THRESHOLDS[1:], start=1):
        name_values['mean@{:.1f}'.format(thr)] = np.mean(np.delete(rates[t], head_idx))
    return name_values, name_values['mean(15j)']


def mpii_name_values(counts, u2a_mapping, actual_joints):
    """The table of mpii_compatible.py:184-193 from integer counts [1, 2, K] (or [2, K]): detected-and-visible and
    visible rows per joint -> (OrderedDict, mean).  The divisors are float32, as the reference has them; a joint
    that is never visible gives nan, and so does the mean then."""
    _, a = u2a_indices(u2a_mapping)
    counts = np.asarray(counts).astype(np.int64).reshape(-1, 2, len(a))[0]
    detected, visible = counts[0].astype(np.float64), counts[1].astype(np.float64)
    with np.errstate(invalid='ignore', divide='ignore'):
        rate = detected / visible.astype(np.float32)
        ratio = visible / np.sum(visible).astype(np.float32)
        name_values = OrderedDict((actual_joints[k], rate[i]) for i, k in enumerate(a))
        name_values['mean'] = np.sum(ratio * rate)
    return name_values, name_values['mean']


def evaluate_h36m(pred, gt, scales, u2a_mapping, actual_joints):
    """MultiViewH36MCompatible.evaluate (multiview_h36m_compatible.py:184-234) on the device.

    pred [N, K, 2 or 3]: the K annotated union joints in order (``all_preds[:, u]``); gt [N, Junion, >= 2]: the
    frames' ``joints_2d`` (or [N, K, 2], selected already); scales [N, 2]: the frames' ``scale``; cuda tensors or
    numpy.  A joint is detected at threshold t when || gt - pred || <= max(scale) * 200 / 10 * t in f64.
    Returns (OrderedDict name_values, perf_indicator) of ``h36m_name_values``; the indicator is ``mean(15j)``."""
    u, _ = u2a_indices(u2a_mapping)
    dev = _eval_device(pred, gt, scales)
    head = _cuda(scales, torch.float64, dev).amax(dim=1) * 200 / 10.0
    counts, n = _counts(pred, gt, head, None, H36M_THRESHOLDS, 0, u)
    return h36m_name_values(counts, n, u2a_mapping, actual_joints)


def evaluate_mpii(pred, gt, joints_vis, headsizes, u2a_mapping, actual_joints):
    """MPIIDatasetCompatible.evaluate (mpii_compatible.py:139-193) on the device.

    pred [N, K, 2 or 3]; gt [N, Junion, >= 2] (or [N, K, 2]); joints_vis [N, Junion, 3] as the dataset keeps it
    (column 0 is read), or [N, Junion] / [N, K], holding 0 and 1; headsizes [N]: the frames' head-box norms times
    the reference's 0.6; cuda tensors or numpy.  Detected: || gt - pred || / headsize <= 0.5 in f64.
    Returns (OrderedDict name_values, perf_indicator) of ``mpii_name_values``: per joint name
    detected-and-visible / visible, then ``mean``, the visibility-weighted sum, which is also the indicator."""
    u, _ = u2a_indices(u2a_mapping)
    counts, _ = _counts(pred, gt, headsizes, joints_vis, (MPII_THRESHOLD,), 1, u)
    return mpii_name_values(counts, u2a_mapping, actual_joints)
