"""Differentiable triangulation and the reprojection loss, host side.  No kernel is launched here.

The restatement (tests/triangulation_grad_restatement.py), which the GPU tests hold the kernels to, is itself held
to oracle.geometry_ref.triangulate_poses / reproject_poses (pinned by the reference's goldens) with unit weights,
and the closed-form backward of the smallest singular vector that the kernel uses is held to autograd through
torch.linalg.svd.  The entry points are declared, exported and bound, and answer their argument errors before any
launch; the Python layers refuse CPU tensors and a missing camera."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

import triangulation_grad_restatement as rs
from oracle import geometry_ref as G
from posu import _native
from posu import synthetic as syn

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ('posu_triangulate_dlt_w', 'posu_triangulate_dlt_bwd', 'posu_reprojection_loss_workspace',
           'posu_reprojection_loss_fwd', 'posu_reprojection_loss_bwd')


def _rel(a, b):
    return float((a - b).abs().max() / b.abs().max())


# ------------------------------------------------------------------ the restatement against the oracle
@pytest.mark.parametrize('distortion', [True, False], ids=['distorted', 'pinhole'])
def test_restatement_equals_the_oracle_with_unit_weights(distortion):
    c = rs.case(3, 4, 5, distortion, seed=2)
    p2d = c['xy'].reshape(12, 5, 2).numpy()
    vis = np.ones((12, 5))
    vis[0:2, 1] = 0                                       # joint 1 of group 0: two views
    vis[5:8, 2] = 0                                       # joint 2 of group 1: one view
    tv = torch.from_numpy(vis.reshape(3, 4, 5))
    for v, t in ((None, None), (vis, tv)):
        Xo = G.triangulate_poses(c['cams'], p2d, v, no_distortion=not distortion)
        proj_o, res_o = G.reproject_poses(p2d, c['cams'], np.ones((12, 5)) if v is None else v,
                                          no_distortion=not distortion)
        for route in ('svd', 'eigh'):
            X = rs.triangulate(c['M'], c['intr'], c['xy'], t, None, True, route)
            dx = np.abs(X.numpy() - Xo).max() / np.abs(Xo).max()
            proj = rs.project(c['M'], c['intr'], X).reshape(12, 5, 2).numpy()
            solved = res_o.astype(bool)
            dp = np.abs(proj - proj_o)[solved].max() / np.abs(proj_o).max()
            print('%s, %s, vis %s: X %.2e, projections %.2e relative to the oracle' % (
                'distorted' if distortion else 'pinhole', route, v is not None, dx, dp))
            # svd is numpy's own route (LAPACK gesdd on both sides); eigh squares the condition number
            assert dx < (1e-12 if route == 'svd' else 1e-8)
            assert dp < (1e-12 if route == 'svd' else 1e-8)
        if v is not None:
            assert (X[1, 2] == 0).all() and (Xo[1, 2] == 0).all()
            e = rs.residuals(c['M'], c['intr'], c['xy'], X, t)
            eo = np.linalg.norm(proj_o - p2d, axis=-1).reshape(3, 4, 5)
            assert (e[1, :, 2] == 0).all()
            assert np.abs(e.numpy() - eo)[solved.reshape(3, 4, 5)].max() < 1e-6


def test_undistortion_is_the_identity_without_coefficients():
    c = rs.case(2, 4, 3, False, seed=3)
    assert torch.equal(rs.undistort(c['intr'], c['xy']), c['xy'])
    d = rs.case(2, 4, 3, True, seed=3)
    moved = (rs.undistort(d['intr'], d['xy']) - d['xy']).abs().max()
    assert 0.01 < float(moved) < 100.0


# ------------------------------------------------------------------ the closed form the kernel computes
@pytest.mark.parametrize('V', [2, 3, 4])
def test_closed_form_gA_equals_autograd(V):
    c = rs.case(3, V, 5, True, seed=4)
    und = rs.undistort(c['intr'], c['xy'])
    A = rs.rows(c['M'], und, torch.ones(3, V, 5, dtype=torch.bool), c['w']).clone().requires_grad_(True)
    gX = torch.from_numpy(np.random.default_rng(6).normal(size=(3, 5, 3)))
    ref, = torch.autograd.grad((rs.point(A, 'svd') * gX).sum(), A)
    via_eigh, = torch.autograd.grad((rs.point(A, 'eigh') * gX).sum(), A)
    got = rs.closed_form_gA(A.detach(), gX)
    print('V = %d: closed form against autograd through svd %.2e (autograd through eigh: %.2e)' % (
        V, _rel(got, ref), _rel(via_eigh, ref)))
    # the closed form is built on eigh, so it can be no closer to the svd route than autograd through eigh is:
    # 8 x that disagreement, and in any case inside the cap the GPU tests hold their bounds to
    assert _rel(got, ref) <= max(8 * _rel(via_eigh, ref), 1e-12)
    assert _rel(got, ref) < 1e-6


def test_detached_loss_has_only_the_direct_term():
    c = rs.case(3, 4, 5, True, seed=5)
    r = rs.reference(c, None, c['w'], c['omega'], True, True)
    X = rs.triangulate(c['M'], c['intr'], c['xy'], None, c['w'])
    d = rs.project(c['M'], c['intr'], X) - c['xy']
    direct = -c['omega'][..., None] * d / d.norm(dim=-1, keepdim=True) / 60
    assert _rel(r['gxy'], direct) < 1e-12
    assert (r['gw'] == 0).all()
    full = rs.reference(c, None, c['w'], c['omega'], True, False)
    assert float(full['loss']) == float(r['loss'])
    assert _rel(full['gxy'], direct) > 1e-3 and float(full['gw'].abs().max()) > 0


# ------------------------------------------------------------------ symbols and argument errors
def test_symbols_are_declared_listed_and_exported():
    src = open(os.path.join(REPO, 'include', 'posu.h')).read()
    src = re.sub(r'/\*.*?\*/', '', src, flags=re.S)
    declared = set(re.findall(r'\b(posu_\w+)\s*\(', src))
    lib = _native.load()
    for name in SYMBOLS:
        assert name in declared, name
        assert name in _native.exported_symbols(), name
        assert hasattr(lib, name), name
    assert lib.posu_abi_version() == _native.ABI_VERSION == 16   # additive: the revision does not move


def test_workspace_query_answers_on_the_host():
    ws = _native.load().posu_reprojection_loss_workspace
    assert ws(1, 1) == 8 and ws(32, 16) == 16 and ws(1, 257) == 16 and ws(0, 16) == 8
    for bad in ((-1, 16), (1, 0), (1 << 20, 1 << 10)):
        assert ws(*bad) == -1, bad


def test_argument_errors_are_reported_before_any_launch():
    lib = _native.load()
    p = ctypes.c_void_p(256)

    def err(st, text):
        assert st == 1, st
        assert text in _native.last_error(), _native.last_error()

    def fwd(M=p, intr=p, xy=p, dtype=_native.F64, V=4, X=p, w=p):
        return lib.posu_triangulate_dlt_w(M, intr, xy, dtype, 40, 10, None, w, 3, V, 5, 1, X, None)

    def bwd(M=p, intr=p, xy=p, dtype=_native.F64, V=4, gX=p, gxy=p):
        return lib.posu_triangulate_dlt_bwd(M, intr, xy, dtype, 40, 10, None, None, 3, V, 5, 1, gX, gxy, None, None)

    def lfwd(M=p, intr=p, xy=p, dtype=_native.F64, V=4, loss=p, ws=p, nbytes=8):
        return lib.posu_reprojection_loss_fwd(M, intr, xy, dtype, 40, 10, None, None, None, 3, V, 5, 1, loss, None,
                                              None, ws, nbytes, None)

    def lbwd(M=p, intr=p, xy=p, dtype=_native.F64, V=4, gloss=p, gxy=p):
        return lib.posu_reprojection_loss_bwd(M, intr, xy, dtype, 40, 10, None, None, None, 3, V, 5, 1, 0, gloss,
                                              gxy, None, None)
    for fn, required in ((fwd, ('M', 'intr', 'xy', 'X')), (bwd, ('M', 'intr', 'xy', 'gX', 'gxy')),
                         (lfwd, ('M', 'intr', 'xy', 'loss', 'ws')), (lbwd, ('M', 'intr', 'xy', 'gloss', 'gxy'))):
        for name in required:
            err(fn(**{name: None}), 'null pointer')
        for V in (1, 5):
            err(fn(V=V), '2 <= V <= 4')
        for dtype in (_native.BF16, _native.F16, 7):
            err(fn(dtype=dtype), 'dtype')
    err(fwd(V=5, w=None), '2 <= V <= 4')                 # also without weights, where posu_triangulate_dlt takes 16
    err(lfwd(nbytes=7), 'workspace too small')
    err(lfwd(ws=ctypes.c_void_p(260)), 'aligned')
    # G == 0: nothing to do, no launch (the pointers above are not memory)
    assert lib.posu_triangulate_dlt_w(p, p, p, _native.F64, 40, 10, None, p, 0, 4, 5, 1, p, None) == 0
    assert lib.posu_triangulate_dlt_bwd(p, p, p, _native.F64, 40, 10, None, None, 0, 4, 5, 1, p, p, None, None) == 0
    assert lib.posu_reprojection_loss_fwd(p, p, p, _native.F64, 40, 10, None, None, None, 0, 4, 5, 1, p, None, None,
                                          p, 8, None) == 0
    assert lib.posu_reprojection_loss_bwd(p, p, p, _native.F64, 40, 10, None, None, None, 0, 4, 5, 1, 0, p, p, None,
                                          None) == 0


# ------------------------------------------------------------------ the Python layers
def _camera_dict():
    return {(s, v): cam for s in syn.SUBJECTS for v, cam in enumerate(syn.h36m_like_cameras(s))}


def test_python_layers_refuse_cpu_tensors():
    from core.loss import ReprojectionLoss
    from posu import ops
    c = rs.case(2, 4, 3, True, seed=7)
    with pytest.raises(RuntimeError, match='cuda'):
        ops.triangulate_points(c['M'], c['intr'], c['xy'])
    with pytest.raises(RuntimeError, match='cuda'):
        ops.reprojection_loss(c['M'], c['intr'], c['xy'], weights=c['w'], target_weight=c['omega'])
    with pytest.raises(RuntimeError, match='cuda'):
        ops.reprojection_residuals(c['M'], c['intr'], c['xy'])
    crit = ReprojectionLoss(syn.make_cfg(), _camera_dict(), device=torch.device('cpu'))
    assert tuple(crit.M.shape) == (2, 4, 3, 4) and tuple(crit.intr.shape) == (2, 4, 9)
    views = [c['xy'][:, v].float() for v in range(4)]
    weights = [torch.ones(2, 3, 1) for _ in range(4)]
    with pytest.raises(RuntimeError, match='cuda'):
        crit(views, weights, [{'subject': torch.tensor([9, 11])}] * 4)


def test_camera_tables_and_missing_cameras():
    from core.loss import ReprojectionLoss
    from multiviews.triangulate import camera_table
    cams = _camera_dict()
    cfg = syn.make_cfg()
    crit = ReprojectionLoss(cfg, cams, device=torch.device('cpu'))
    M, intr = camera_table(cams[(11, 2)])
    assert np.array_equal(crit.M[1, 2].numpy(), M) and np.array_equal(crit.intr[1, 2].numpy(), intr)
    assert crit.subject_indices([11, 9, 11]).tolist() == [1, 0, 1]
    assert crit.use_target_weight is True and float(crit.intr[:, :, 4:].abs().max()) > 0
    cfg.DATASET.NO_DISTORTION = True
    cfg.LOSS.USE_TARGET_WEIGHT_REPROJ = False
    plain = ReprojectionLoss(cfg, cams, device=torch.device('cpu'))
    assert plain.use_target_weight is False and float(plain.intr[:, :, 4:].abs().max()) == 0
    del cams[(11, 3)]
    holed = ReprojectionLoss(cfg, cams, device=torch.device('cpu'))
    assert holed.subject_indices([9, 9]).tolist() == [0, 0]
    with pytest.raises(KeyError, match=r'\(11, 3\)'):
        holed.subject_indices([9, 11])
    with pytest.raises(KeyError):
        holed.subject_indices([1])
