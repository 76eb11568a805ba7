"""Generate tests/golden/pose3d.npz from the REFERENCE's 3-D evaluation code (/root/reference).
Run once, not on the GPU box:

    python tests/golden/make_pose3d_golden.py

utils.pose_utils.PoseUtils imports as it is (numpy and sklearn).  run/pose3d/estimate.py cannot be
imported (multiviews.tool and pict_struct do not exist), so the file is parsed here and only its
two self-contained functions, break_limb_length and error_computing_3d, are compiled from the parse
tree and executed, with `procrustes` bound to PoseUtils().procrustes.  Nothing of the reference's
text is written anywhere: only arrays go into the file.

Every float result is stored as the 50-digit mpmath evaluation of the same formulas (the yardstick,
rounded to fp64) together with the reference's own largest distance from it (ref_err_*), which is
what the tests' tolerances are built from.  Inputs follow tests/pose3d_restatement.py's seeded
recipes (no reference code):

  procrustes   per J in (4, 16, 17, 65) two pairs, the second mirrored, each under the six
               (scaling, reflection) settings of pose3d_restatement.SETTINGS
               -> pa_J{J}_{A,B} [2, J, 3]; pa_J{J}_{Z [6, 2, J, 3], d [6, 2], R, scale, t};
                  pa_J{J}_ref_err_{Z, d} [6, 2]
  errors       per J in (16, 17) five groups of four cameras, Procrustes 'No' / 'Yes'
               -> er_J{J}_{X, gt, R, T}; er_J{J}_err [2, 5, 4, J]; er_J{J}_ref_err [2, 5, 4]
  limb check   70 groups from make_limb_cases (regenerated from the seed by the tests; a checksum is
               stored), shared and per-group limbs, and the hand-built ties
               -> lb_{shared, group}_{flag [70], sum}; lb_tie_{poses, limb, thres, flag}
"""
import ast
import os
import sys

import mpmath as mp
import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
REF = '/root/reference'
sys.path.insert(0, os.path.dirname(HERE))
import pose3d_restatement as rs  # noqa: E402  -- recipes only; imports neither lib

mp.mp.dps = 50


def _import_reference():
    sys.path.insert(0, os.path.join(REF, 'lib'))
    from utils.pose_utils import PoseUtils
    tree = ast.parse(open(os.path.join(REF, 'run', 'pose3d', 'estimate.py')).read())
    wanted = [n for n in tree.body if isinstance(n, ast.FunctionDef)
              and n.name in ('break_limb_length', 'error_computing_3d')]
    assert len(wanted) == 2
    ns = {'np': np, 'procrustes': PoseUtils().procrustes}
    exec(compile(ast.Module(body=wanted, type_ignores=[]), 'estimate_functions', 'exec'), ns)
    return PoseUtils(), ns['break_limb_length'], ns['error_computing_3d']


# ---------------------------------------------------------------- 50-digit yardstick
def _mat(a):
    return mp.matrix(np.asarray(a, dtype=np.float64).tolist())


def _np(m):
    return np.array([[float(m[i, j]) for j in range(m.cols)] for i in range(m.rows)])


def mp_procrustes(A, B, scaling=True, reflection='best'):
    A, B = (m if isinstance(m, mp.matrix) else _mat(m) for m in (A, B))    # fp64 arrays or 50-digit matrices
    n = A.rows
    ones = mp.matrix([[1] * n])
    a_bar, b_bar = ones * A / n, ones * B / n
    A0 = A - mp.matrix([[a_bar[0, c] for c in range(3)] for _ in range(n)])
    B0 = B - mp.matrix([[b_bar[0, c] for c in range(3)] for _ in range(n)])
    ssx = sum(A0[i, c] ** 2 for i in range(n) for c in range(3))
    ssy = sum(B0[i, c] ** 2 for i in range(n) for c in range(3))
    a_norm, b_norm = mp.sqrt(ssx), mp.sqrt(ssy)
    A0, B0 = A0 / a_norm, B0 / b_norm
    U, S, Vt = mp.svd_r(A0.T * B0)
    s = [S[i] for i in range(3)]
    assert s[0] >= s[1] >= s[2] > 0
    V = Vt.T
    R = V * U.T
    if reflection != 'best' and bool(reflection) != (mp.det(R) < 0):
        for r in range(3):
            V[r, 2] = -V[r, 2]
        s[2] = -s[2]
        R = V * U.T
    trace = s[0] + s[1] + s[2]
    rows = lambda row: mp.matrix([[row[0, c] for c in range(3)] for _ in range(n)])   # noqa: E731
    if scaling:
        scale, d = trace * a_norm / b_norm, 1 - trace ** 2
        Z = a_norm * trace * (B0 * R) + rows(a_bar)
    else:
        scale, d = mp.mpf(1), 1 + ssy / ssx - 2 * trace * b_norm / a_norm
        Z = b_norm * (B0 * R) + rows(a_bar)
    t = a_bar - scale * (b_bar * R)
    return d, Z, R, scale, t


def mp_errors(X, gt, R, T, yes):
    """One (group, camera) -> err [J] as mpf."""
    X, gt, R = _mat(X), _mat(gt), _mat(R)
    n = X.rows
    Tm = mp.matrix([[mp.mpf(float(T[c])) for c in range(3)] for _ in range(n)])
    pred = (R * (X - Tm).T).T
    if yes:
        pred = mp_procrustes(gt, pred)[1]
    return [mp.sqrt(sum((gt[i, c] - pred[i, c]) ** 2 for c in range(3))) for i in range(n)]


def _dist(mp_vals, ref):
    """Largest |reference - yardstick| over an array, in fp64 (the subtraction at 50 digits)."""
    ref = np.asarray(ref, dtype=np.float64).reshape(-1)
    return max(float(abs(mp.mpf(float(r)) - m)) for r, m in zip(ref, mp_vals))


def _flat(m):
    return [m[i, j] for i in range(m.rows) for j in range(m.cols)]


# ----------------------------------------------------------------------------- cases
def procrustes_cases(pu, data):
    for J in (4, 16, 17, 65):
        rng = np.random.RandomState(100 + J)
        pairs = [rs.make_pair(rng, J, mirrored=m) for m in (False, True)]
        A, B = np.stack([p[0] for p in pairs]), np.stack([p[1] for p in pairs])
        out = {k: [] for k in ('Z', 'd', 'R', 'scale', 't', 'ref_err_Z', 'ref_err_d')}
        for scaling, reflection in rs.SETTINGS:
            row = {k: [] for k in out}
            for a, b in zip(A, B):
                d_ref, z_ref, tf = pu.procrustes(a.copy(), b.copy(), scaling=scaling, reflection=reflection)
                d, Z, R, scale, t = mp_procrustes(a, b, scaling, reflection)
                det = np.linalg.det(tf['rotation'])
                assert reflection == 'best' or (det < 0) == bool(reflection)
                # the restatement states the same formulas: it must sit where the reference sits
                d_rs, z_rs = rs.procrustes(a, b, scaling, reflection)[:2]
                assert np.abs(z_rs - z_ref).max() <= 1e-10 and abs(d_rs - d_ref) <= 1e-13
                row['Z'].append(_np(Z))
                row['d'].append(float(d))
                row['R'].append(_np(R))
                row['scale'].append(float(scale))
                row['t'].append(_np(t)[0])
                row['ref_err_Z'].append(_dist(_flat(Z), z_ref))
                row['ref_err_d'].append(float(abs(mp.mpf(float(d_ref)) - d)))
            for k in out:
                out[k].append(np.array(row[k]))
        data['pa_J%d_A' % J], data['pa_J%d_B' % J] = A, B
        for k in out:
            data['pa_J%d_%s' % (J, k)] = np.stack(out[k])
        print('procrustes J=%d: ref_err Z max %.2e mm (coordinates to %.0f), d max %.2e; det(best) %s'
              % (J, np.max(out['ref_err_Z']), np.abs(A).max(), np.max(out['ref_err_d']),
                 [round(float(np.linalg.det(r)), 3) for r in out['R'][0]]))


def error_cases(error_computing_3d, data):
    for J in (16, 17):
        X, gt, R, T = rs.make_groups(np.random.RandomState(200 + J), 5, 4, J)
        err = np.empty((2, 5, 4, J))
        ref_err = np.empty((2, 5, 4))
        for k, yes in enumerate(('No', 'Yes')):
            for g in range(5):
                ref = error_computing_3d(X[g], list(gt[g]), list(R[g]), [t.reshape(3, 1) for t in T[g]], yes)
                for v in range(4):
                    m = mp_errors(X[g], gt[g, v], R[g, v], T[g, v], yes == 'Yes')
                    err[k, g, v] = [float(x) for x in m]
                    ref_err[k, g, v] = _dist(m, ref[v])
            e_rs = rs.pose3d_errors(X, gt, R, T, yes == 'Yes')[0]
            assert np.abs(e_rs - err[k]).max() <= 1e-9
        data.update({'er_J%d_X' % J: X, 'er_J%d_gt' % J: gt, 'er_J%d_R' % J: R, 'er_J%d_T' % J: T,
                     'er_J%d_err' % J: err, 'er_J%d_ref_err' % J: ref_err})
        print('errors J=%d: MPJPE %.1f mm, PA-MPJPE %.1f mm; ref_err max %.2e / %.2e'
              % (J, err[0].mean(), err[1].mean(), ref_err[0].max(), ref_err[1].max()))


def _skeleton():
    kids = [[] for _ in rs.PARENT]
    for c, p in enumerate(rs.PARENT):
        if p >= 0:
            kids[p].append(c)
    return [{'idx': i, 'children': k} for i, k in enumerate(kids)]


def tie_cases():
    """Two joints (parent 0 -> child 1) on the x axis: two exact ties, a neighbour just past one, and a
    pose holding a NaN -> (poses [4, 2, 3], limb [4, 2], thres [4])."""
    poses = np.zeros((4, 2, 3))
    poses[0, 1, 0] = 15.0          # |10 - 15| = 5 = 0.5 * 10: a tie
    poses[1, 1, 0] = 14.0          # |10 - 14| = 4 = 0.4 * 10 in fp64: a tie
    poses[2, 1, 0] = 15.000001     # just past the first tie
    poses[3, 1] = [np.nan, 3.0, 4.0]
    limb = np.tile([0.0, 10.0], (4, 1))
    return poses, limb, np.array([0.5, 0.4, 0.5, 0.4])


def limb_cases(break_limb_length, data):
    skel = _skeleton()
    for name, per_group in (('shared', False), ('group', True)):
        poses, limb, moved = rs.make_limb_cases(300 + per_group, 70, per_group)
        rows = np.broadcast_to(limb, (70, 16))
        flag = np.zeros(70, dtype=np.uint8)
        for g in range(70):
            table = {(int(rs.PARENT[c]), c): rows[g, c] for c in range(16) if rs.PARENT[c] >= 0}
            flag[g] = break_limb_length(skel, poses[g], table)
            for (p, c), L in table.items():       # far from the threshold: flags are safe to compare exactly
                off = abs(L - np.linalg.norm(poses[g, p] - poses[g, c]))
                assert abs(off - 0.4 * L) >= 1e-6 * L
        assert np.array_equal(flag.astype(bool), moved) and 20 < flag.sum() < 50
        assert np.array_equal(rs.limb_break(poses, rs.PARENT, limb)[0], moved)
        data['lb_%s_flag' % name] = flag
        data['lb_%s_sum' % name] = np.array(poses.sum())
        print('limb check (%s limbs): %d of 70 flag' % (name, flag.sum()))
    poses, limb, thres = tie_cases()
    assert 0.4 * 10 == 4.0 and 0.5 * 10 == 5.0
    two = [{'idx': 0, 'children': [1]}, {'idx': 1, 'children': []}]
    with np.errstate(invalid='ignore'):
        flag = np.array([break_limb_length(two, poses[i], {(0, 1): limb[i, 1]}, thres[i]) for i in range(4)])
    assert flag.tolist() == [False, False, True, False]
    data.update(lb_tie_poses=poses, lb_tie_limb=limb, lb_tie_thres=thres, lb_tie_flag=flag.astype(np.uint8))


def main():
    pu, break_limb_length, error_computing_3d = _import_reference()
    data = {}
    procrustes_cases(pu, data)
    error_cases(error_computing_3d, data)
    limb_cases(break_limb_length, data)
    path = os.path.join(HERE, 'pose3d.npz')
    np.savez_compressed(path, **data)
    print('pose3d.npz', os.path.getsize(path), 'bytes')


if __name__ == '__main__':
    main()
