"""Generate tests/golden/validate_eval.npz by running the REFERENCE's own dataset evaluations,
MultiViewH36MCompatible.evaluate (lib/dataset/multiview_h36m_compatible.py:184-234) and
MPIIDatasetCompatible.evaluate (lib/dataset/mpii_compatible.py:139-193), on the CPU.  Run once, where the
reference is checked out (not on the GPU box):

    python tests/golden/make_validate_golden.py

The two modules are loaded by file path (make_golden's REF_LIB) with stand-ins for what they import but
``evaluate`` does not need (h5py, cv2, json_tricks, dataset.joints_dataset_compatible, utils.vis), with
``np.float = float`` for current numpy, and ``loadmat`` replaced by seeded head boxes.  ``evaluate`` is called
unbound on a stand-in ``self`` that carries what it reads: u2a_mapping (two '*' entries, out of order, 'head'
mapped), grouping, db, actual_joints.  The file holds data only: the inputs and the returned tables, plus the
integer counts behind them taken with the fp64 numpy expression of each form.

h36m.*  N = 24 frames (6 groups x 4), 19 union joints of which 17 are annotated; pred float32 [N, 17, 3];
        thresholds 0.5 .. 0.1, form d <= head * thr.  Rows on the boundary: frame 0 has scale 0.5 (head 10),
        gt (0, 0) and pred (3, 4) for joint 0 (d = 5 = head * 0.5) and pred (0, 4) for joint 1 (d = 4 =
        head * 0.4); frame 1, joint 0 holds a (d, head, thr) found by a small search on which d <= head * thr
        and d / head <= thr disagree (h36m.forms_disagree says whether the search found one).
mpii.*  N = 20 frames (5 groups x 4), 18 union joints of which 16 are annotated; joints_vis 0 / 1 with union
        joint 4 never visible (its rate is nan, and so is the mean); form d / head <= 0.5.  Frame 0, joint 0:
        d = head / 2 exactly.
"""
import collections
import importlib.util
import os
import sys
import types

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import make_golden as mg  # noqa: E402  (REF_LIB)

H36M_JOINTS = ['root', 'rhip', 'rkne', 'rank', 'lhip', 'lkne', 'lank', 'belly', 'neck', 'nose', 'head', 'lsho',
               'lelb', 'lwri', 'rsho', 'relb', 'rwri']
MPII_JOINTS = ['rank', 'rkne', 'rhip', 'lhip', 'lkne', 'lank', 'root', 'thorax', 'upper neck', 'head top', 'rwri',
               'relb', 'rsho', 'lsho', 'lelb', 'lwri']
THRESHOLDS = (0.5, 0.4, 0.3, 0.2, 0.1)


def _load_reference():
    if not hasattr(np, 'float'):
        np.float = float
    for name in ('h5py', 'cv2', 'json_tricks'):
        sys.modules.setdefault(name, types.ModuleType(name))
    base = types.ModuleType('dataset.joints_dataset_compatible')
    base.JointsDatasetCompatible = type('JointsDatasetCompatible', (object,), {})
    vis = types.ModuleType('utils.vis')
    vis.save_all_preds = lambda *a, **k: None
    for name, mod in (('dataset', types.ModuleType('dataset')), ('dataset.joints_dataset_compatible', base),
                      ('utils', types.ModuleType('utils')), ('utils.vis', vis)):
        sys.modules[name] = mod
    out = []
    for fname in ('multiview_h36m_compatible.py', 'mpii_compatible.py'):
        spec = importlib.util.spec_from_file_location('ref_' + fname[:-3], os.path.join(mg.REF_LIB, 'dataset', fname))
        mod = importlib.util.module_from_spec(spec)
        spec.loader.exec_module(mod)
        out.append(mod)
    return out


def _mapping(r, nunion, nactual):
    """{union index: dataset index or '*'}: a seeded assignment with nunion - nactual '*' entries, inserted out
    of key order (the reference sorts by key)."""
    slots = list(r.permutation(nunion))
    stars = sorted(slots[nactual:])
    pairs = dict(zip(slots[:nactual], r.permutation(nactual)))
    keys = list(r.permutation(nunion))
    return collections.OrderedDict((int(k), '*' if k in stars else int(pairs[k])) for k in keys)


def _u_a(mapping):
    items = sorted(((k, v) for k, v in mapping.items() if v != '*'), key=lambda kv: kv[0])
    return np.array([k for k, _ in items]), np.array([v for _, v in items])


def _counts(pred, gt, head, vis, form):
    """[T, 2, K] int64 with the fp64 numpy expression of each form."""
    d = np.sqrt(np.sum((gt - pred[:, :, :2]) ** 2, axis=2))
    h = head[:, None]
    vis = np.ones(d.shape, bool) if vis is None else vis != 0
    out = np.zeros((len(THRESHOLDS), 2, d.shape[1]), np.int64)
    for t, thr in enumerate(THRESHOLDS):
        det = (d <= h * thr) if form == 0 else (np.divide(d, h) <= thr)
        out[t, 0] = np.sum(det & vis, axis=0)
        out[t, 1] = np.sum(vis, axis=0)
    return out


def _find_disagreement(r):
    """(scale, d, thr) with (d <= head * thr) != (d / head <= thr), head = scale * 200 / 10.0; None if a few
    thousand draws find none."""
    for _ in range(20000):
        s = float(r.uniform(0.5, 3.0))
        h = s * 200 / 10.0
        for thr in THRESHOLDS[1:]:
            for d in (h * thr, np.nextafter(h * thr, np.inf), np.nextafter(h * thr, 0.0)):
                if np.sqrt(d * d) == d and (d <= h * thr) != (d / h <= thr):
                    return s, float(d), thr
    return None


def _table(name_values):
    return np.array(list(name_values.keys())), np.array([float(v) for v in name_values.values()], dtype=np.float64)


def h36m_case(ref, r):
    n, nunion, k = 24, 19, len(H36M_JOINTS)
    mapping = _mapping(r, nunion, k)
    u, _ = _u_a(mapping)
    gt = r.uniform(100.0, 900.0, size=(n, nunion, 2))
    scales = r.uniform(0.8, 2.5, size=(n, 2))
    head = np.amax(scales, axis=1) * 200 / 10.0
    # offsets from 0 to 0.7 head sizes: rates strictly between 0 and 1 at every threshold
    ang = r.uniform(0, 2 * np.pi, size=(n, k))
    rad = r.uniform(0.0, 0.7, size=(n, k)) * head[:, None]
    pred = np.zeros((n, k, 3), np.float32)
    pred[:, :, 0] = gt[:, u, 0] + rad * np.cos(ang)
    pred[:, :, 1] = gt[:, u, 1] + rad * np.sin(ang)
    pred[:, :, 2] = r.uniform(0.1, 1.0, size=(n, k))
    # the boundary rows
    scales[0] = (0.5, 0.25)
    gt[0, u[0]] = (0.0, 0.0)
    pred[0, 0, :2] = (3.0, 4.0)
    gt[0, u[1]] = (0.0, 0.0)
    pred[0, 1, :2] = (0.0, 4.0)
    found = _find_disagreement(r)
    if found is not None:
        s, d, _ = found
        scales[1] = (s, s / 2)
        gt[1, u[0]] = (d, 0.0)
        pred[1, 0, :2] = (0.0, 0.0)
    fake = types.SimpleNamespace(
        u2a_mapping=mapping, actual_joints=dict(enumerate(H36M_JOINTS)),
        grouping=[[4 * g + c for c in range(4)] for g in range(n // 4)],
        db=[{'joints_2d': gt[i], 'scale': scales[i], 'image': 'f%d' % i} for i in range(n)])
    name_values, perf = ref.MultiViewH36MCompatible.evaluate(fake, pred, None)
    names, values = _table(name_values)
    head = np.amax(scales, axis=1) * 200 / 10.0
    c0, c1 = _counts(pred, gt[:, u], head, None, 0), _counts(pred, gt[:, u], head, None, 1)
    return {'pred': pred, 'gt': gt, 'scales': scales, 'u2a_keys': np.array(list(mapping.keys())),
            'u2a_values': np.array([-1 if v == '*' else v for v in mapping.values()]),
            'joint_names': np.array(H36M_JOINTS), 'names': names, 'values': values, 'perf': np.float64(perf),
            'counts_form0': c0, 'counts_form1': c1, 'forms_disagree': np.array(bool((c0 != c1).any()))}


def mpii_case(ref, r):
    n, nunion, k = 20, 18, len(MPII_JOINTS)
    mapping = _mapping(r, nunion, k)
    u, _ = _u_a(mapping)
    gt = r.uniform(50.0, 600.0, size=(n, nunion, 2))
    boxes = np.zeros((2, 2, n))
    boxes[0] = r.uniform(10.0, 300.0, size=(2, n))
    boxes[1] = boxes[0] + r.uniform(20.0, 120.0, size=(2, n))
    headsizes = np.linalg.norm(boxes[1, :, :] - boxes[0, :, :], axis=0) * 0.6
    vis = np.zeros((n, nunion, 3))
    vis[:, :, 0] = vis[:, :, 1] = (r.uniform(size=(n, nunion)) > 0.25)
    vis[:, u[4], :] = 0.0                       # a joint that is never visible
    ang = r.uniform(0, 2 * np.pi, size=(n, k))
    rad = r.uniform(0.0, 1.0, size=(n, k)) * headsizes[:, None]
    pred = np.zeros((n, k, 3), np.float32)
    pred[:, :, 0] = gt[:, u, 0] + rad * np.cos(ang)
    pred[:, :, 1] = gt[:, u, 1] + rad * np.sin(ang)
    pred[:, :, 2] = r.uniform(0.1, 1.0, size=(n, k))
    gt[0, u[0]] = (headsizes[0] / 2, 0.0)       # d / head = 0.5 exactly
    pred[0, 0, :2] = (0.0, 0.0)
    vis[0, u[0], :2] = 1.0
    ref.loadmat = lambda path: {'headboxes_src': boxes}
    fake = types.SimpleNamespace(
        u2a_mapping=mapping, actual_joints=dict(enumerate(MPII_JOINTS)), root='', subset='valid',
        grouping=[[4 * g + c for c in range(4)] for g in range(n // 4)],
        db=[{'joints_2d': gt[i], 'joints_vis': vis[i], 'image': 'f%d' % i} for i in range(n)])
    name_values, perf = ref.MPIIDatasetCompatible.evaluate(fake, pred, None)
    names, values = _table(name_values)
    v = vis[:, u, 0]
    return {'pred': pred, 'gt': gt, 'joints_vis': vis, 'headsizes': headsizes,
            'u2a_keys': np.array(list(mapping.keys())),
            'u2a_values': np.array([-1 if x == '*' else x for x in mapping.values()]),
            'joint_names': np.array(MPII_JOINTS), 'names': names, 'values': values, 'perf': np.float64(perf),
            'counts_form0': _counts(pred, gt[:, u], headsizes, v, 0),
            'counts_form1': _counts(pred, gt[:, u], headsizes, v, 1)}


def main():
    ref_h36m, ref_mpii = _load_reference()
    r = np.random.default_rng(20260)
    out = {}
    for prefix, case in (('h36m', h36m_case(ref_h36m, r)), ('mpii', mpii_case(ref_mpii, r))):
        for key, value in case.items():
            out['%s.%s' % (prefix, key)] = value
    out['thresholds'] = np.array(THRESHOLDS)
    path = os.path.join(HERE, 'validate_eval.npz')
    np.savez_compressed(path, **out)
    print('wrote', path, os.path.getsize(path), 'bytes; forms disagree:', bool(out['h36m.forms_disagree']))
    for prefix in ('h36m', 'mpii'):
        print(prefix, dict(zip(out[prefix + '.names'].tolist(), np.round(out[prefix + '.values'], 4).tolist())))


if __name__ == '__main__':
    main()
