"""The 3-D evaluation protocol, host side: the three posu_* entry points are declared, exported and
bound, their argument checks run before any launch, the Python layers refuse CPU tensors, and the
numpy restatement (tests/pose3d_restatement.py) is pinned to the reference's recorded results
(tests/golden/pose3d.npz, made by make_pose3d_golden.py).  No kernel is launched here.

Tolerances: every float in the golden is a 50-digit evaluation (the yardstick) with the
reference's own distance from it, ref_err; the restatement states the same fp64 formulas, so it
has to sit within 8 x that distance (never less than 8 ulp of the largest coordinate, or of 1 for
the normalised residual d)."""
import ctypes
import os
import re
import types

import numpy as np
import pytest
import torch

import pose3d_restatement as rs
from posu import _native

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ('posu_procrustes', 'posu_pose3d_errors', 'posu_limb_break')


def z_gate(ref_err, coords):
    return 8 * max(float(np.max(ref_err)), float(np.spacing(np.abs(coords).max())))


def d_gate(ref_err):
    return 8 * max(float(np.max(ref_err)), 2.2e-16)


def test_pose3d_symbols_are_declared_listed_and_exported():
    src = open(os.path.join(REPO, 'include', 'posu.h')).read()
    src = re.sub(r'/\*.*?\*/', '', src, flags=re.S)
    declared = set(re.findall(r'\b(posu_\w+)\s*\(', src))
    lib = _native.load()
    for name in SYMBOLS:
        assert name in declared, name
        assert name in _native.exported_symbols(), name
        assert hasattr(lib, name), name
    assert lib.posu_abi_version() == _native.ABI_VERSION == 16   # additive: the revision does not move


def test_pose3d_argument_errors_are_reported_without_a_gpu():
    lib = _native.load()
    p = ctypes.c_void_p(256)

    def err(st, text):
        assert st == 1, st
        assert text in _native.last_error(), _native.last_error()

    def pa(A=p, B=p, N=2, J=16, refl=0, outs=(p, p, p, p, p)):
        return lib.posu_procrustes(A, B, N, J, 1, refl, *outs, None)
    err(pa(A=None), 'null pointer')
    err(pa(B=None), 'null pointer')
    err(pa(outs=(None,) * 5), 'null pointer')
    err(pa(N=0), 'bad shape')
    err(pa(J=0), 'bad shape')
    err(pa(refl=3), 'reflection')

    def er(X=p, gt=p, R=p, T=p, G=2, V=4, J=16, out=p):
        return lib.posu_pose3d_errors(X, gt, R, T, G, V, J, 1, out, None, None)
    for kw in ({'X': None}, {'gt': None}, {'R': None}, {'T': None}, {'out': None}):
        err(er(**kw), 'null pointer')
    err(er(G=0), 'bad shape')
    err(er(V=0), 'bad shape')
    err(er(J=0), 'bad shape')
    err(er(G=1 << 20, V=1 << 12), 'too large')

    def lb(X=p, parent=p, limb=p, stride=16, G=2, J=16, flag=p):
        return lib.posu_limb_break(X, parent, limb, stride, G, J, 0.4, flag, None, None)
    for kw in ({'X': None}, {'parent': None}, {'limb': None}, {'flag': None}):
        err(lb(**kw), 'null pointer')
    err(lb(G=0), 'bad shape')
    err(lb(J=0), 'bad shape')
    err(lb(stride=8), 'limb_stride')


def test_python_layers_refuse_cpu_tensors_and_unbuilt_parts():
    from multiviews import estimate
    from posu import ops
    from utils.pose_utils import PoseUtils
    a = torch.zeros(2, 16, 3, dtype=torch.float64)
    with pytest.raises(RuntimeError, match='cuda'):
        ops.procrustes(a, a)
    with pytest.raises(RuntimeError, match='cuda'):
        ops.pose3d_errors(a, torch.zeros(2, 4, 16, 3), torch.zeros(2, 4, 3, 3), torch.zeros(2, 4, 3))
    with pytest.raises(RuntimeError, match='cuda'):
        ops.limb_break(a, torch.zeros(16, dtype=torch.int32), torch.ones(16))
    with pytest.raises(RuntimeError, match='cuda'):
        PoseUtils().procrustes(a, a)
    with pytest.raises(RuntimeError, match='cuda'):
        PoseUtils().procrustes(a[0], a[0])
    with pytest.raises(RuntimeError, match='cuda'):
        estimate.break_limb_length_batch(a, np.ones(16))
    with pytest.raises(RuntimeError, match='cuda'):
        estimate.pose3d_errors(a, torch.zeros(2, 4, 16, 3), torch.zeros(2, 4, 3, 3), torch.zeros(2, 4, 3))
    with pytest.raises(RuntimeError, match='cuda'):
        estimate.Pose3DMeter(16, 3, device=torch.device('cpu')).update(torch.zeros(2, 4, 16), [0, 1])
    with pytest.raises(NotImplementedError):
        PoseUtils().estimate_camera(np.zeros((16, 2)), np.zeros((16, 3)))
    with pytest.raises(NotImplementedError):
        PoseUtils().align_3d_to_2d(np.zeros((16, 2)), np.zeros((16, 3)), {}, 0)


def test_estimate_poses_refuses_an_unknown_mode_and_runs_nowhere_without_a_device(monkeypatch):
    from multiviews import estimate
    cfg = types.SimpleNamespace()
    with pytest.raises(ValueError, match='mode'):
        estimate.estimate_poses([], np.zeros((0, 16, 2)), None, None, None, None, cfg, mode='ransac')
    monkeypatch.setattr(torch.cuda, 'is_available', lambda: False)
    with pytest.raises(RuntimeError, match='cuda'):
        estimate.estimate_poses([], np.zeros((0, 16, 2)), None, None, None, None, cfg, mode='triangulation')
    with pytest.raises(RuntimeError, match='cuda'):
        estimate.error_computing_3d(np.zeros((16, 3)), [np.zeros((16, 3))], [np.eye(3)], [np.zeros((3, 1))], 'No')
    with pytest.raises(RuntimeError, match='cuda'):
        estimate.break_limb_length([{'idx': 0, 'children': [1]}, {'idx': 1, 'children': []}], np.zeros((2, 3)),
                                   {(0, 1): 10.0})


# ------------------------------------------------------ the restatement against the golden
@pytest.mark.parametrize('J', [4, 16, 17, 65])
@pytest.mark.parametrize('fn', ['procrustes', 'procrustes_jacobi'])
def test_restated_procrustes_sits_where_the_reference_sits(golden, J, fn):
    g = golden('pose3d.npz')
    A, B = g['pa_J%d_A' % J], g['pa_J%d_B' % J]
    for k, (scaling, reflection) in enumerate(rs.SETTINGS):
        for n in range(A.shape[0]):
            d, Z, R, scale, t = getattr(rs, fn)(A[n], B[n], scaling, reflection)
            gz = z_gate(g['pa_J%d_ref_err_Z' % J][k, n], A[n])
            ez = float(np.abs(Z - g['pa_J%d_Z' % J][k, n]).max())
            ed = abs(d - g['pa_J%d_d' % J][k, n])
            print('%s J=%d %s/%s pair %d: Z %.2e (gate %.2e), d %.2e' % (fn, J, scaling, reflection, n, ez, gz, ed))
            assert ez <= gz
            assert ed <= d_gate(g['pa_J%d_ref_err_d' % J][k, n])
            assert float(np.abs(R - g['pa_J%d_R' % J][k, n]).max()) <= 1e-13
            assert abs(scale - g['pa_J%d_scale' % J][k, n]) <= 1e-14
            assert float(np.abs(t - g['pa_J%d_t' % J][k, n]).max()) <= gz
            assert reflection == 'best' or (np.linalg.det(R) < 0) == reflection
    # the second pair is mirrored: its best fit is a reflection, the first's a rotation
    dets = [np.linalg.det(r) for r in g['pa_J%d_R' % J][0]]
    assert dets[0] > 0.99 and dets[1] < -0.99


@pytest.mark.parametrize('J', [16, 17])
def test_restated_errors_equal_the_reference(golden, J):
    g = golden('pose3d.npz')
    X, gt, R, T = (g['er_J%d_%s' % (J, k)] for k in ('X', 'gt', 'R', 'T'))
    for k, yes in enumerate((False, True)):
        err, pred = rs.pose3d_errors(X, gt, R, T, yes)
        gate = z_gate(g['er_J%d_ref_err' % J][k], gt)
        assert float(np.abs(err - g['er_J%d_err' % J][k]).max()) <= gate
        assert np.array_equal(err, np.linalg.norm(gt - pred, axis=3))
    assert g['er_J%d_err' % J][1].mean() < 0.5 * g['er_J%d_err' % J][0].mean()    # alignment matters here


def test_restated_limb_check_equals_the_reference_exactly(golden):
    g = golden('pose3d.npz')
    for name, per_group in (('shared', False), ('group', True)):
        poses, limb, moved = rs.make_limb_cases(300 + per_group, 70, per_group)
        assert float(poses.sum()) == float(g['lb_%s_sum' % name])      # the seeded recipe drew the same poses
        flag, worst = rs.limb_break(poses, rs.PARENT, limb)
        assert np.array_equal(flag, g['lb_%s_flag' % name].astype(bool)) and np.array_equal(flag, moved)
        assert np.all(worst[moved] > 0.59) and np.all(worst[~moved] < 0.11)
    flags = [rs.limb_break(g['lb_tie_poses'][i:i + 1], [-1, 0], g['lb_tie_limb'][i:i + 1], g['lb_tie_thres'][i])[0][0]
             for i in range(4)]
    assert flags == g['lb_tie_flag'].astype(bool).tolist() == [False, False, True, False]


def test_restated_summary_on_a_hand_checked_table():
    err = np.arange(2 * 2 * 3, dtype=np.float64).reshape(2, 2, 3)          # two groups, two cameras, three joints
    s = rs.summary([err], [[1, 1]], [[False, True]], [err + 1.0])
    assert s['mpjpe'] == 5.5 and s['joint_wise'].tolist() == [4.5, 5.5, 6.5]
    assert s['variance'] == np.var([1.0, 4.0, 7.0, 10.0])
    assert s['action_wise'] == {1: 5.5} and s['compare'] == {'before': 9.5, 'after': 8.5}
    assert s['pict_struct_count'] == 1 and s['groups'] == 2
