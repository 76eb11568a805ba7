"""posu_triangulate_dlt_w / _bwd and posu_reprojection_loss_fwd / _bwd on the device, through ops.triangulate_points,
ops.reprojection_loss and core.loss.ReprojectionLoss, against the torch restatement
(tests/triangulation_grad_restatement.py; test_triangulation_grad_host.py holds it to the oracle).

Yardstick.  Every kernel output is compared with the restatement's SVD route (values from torch.linalg.svd,
gradients from autograd through it), relative to the largest reference entry of that quantity.  The bound is the
disagreement of the restatement's second route (torch.linalg.eigh of A^T A) with the SVD route on the same inputs,
measured here and printed; an f32 output adds one f32 ulp of that largest entry.  No bound may exceed 1e-6
(asserted: a condition on the inputs, not a measurement of the kernel).  A quantity whose reference is zero
everywhere (gw with the point detached) must be exactly zero.  DESIGN.md section 5 records what was measured."""
import functools

import numpy as np
import pytest
import torch

import triangulation_grad_restatement as rs
from posu import synthetic as syn

pytestmark = pytest.mark.gpu
CAP = 1e-6


def _check(tag, got, svd, eigh, f32=False):
    got, svd, eigh = [torch.as_tensor(t).detach().cpu().double() for t in (got, svd, eigh)]
    assert got.shape == svd.shape, (tag, got.shape, svd.shape)
    assert torch.isfinite(got).all(), tag
    top = float(svd.abs().max())
    if top == 0.0:
        print('%-28s reference is zero everywhere: exact' % tag)
        assert float(got.abs().max()) == 0.0, tag
        return
    bound = float((eigh - svd).abs().max()) / top
    assert bound <= CAP, (tag, bound)                     # the two routes of the reference alone stay inside the cap
    if f32:
        bound += float(np.spacing(np.float32(top))) / top
    err = float((got - svd).abs().max()) / top
    print('%-28s kernel against svd %.3e, bound (eigh against svd%s) %.3e' % (tag, err, ' + f32 ulp' if f32 else '',
                                                                              bound))
    assert err <= bound, (tag, err, bound)


@functools.lru_cache(maxsize=None)
def _case(G=3, V=4, J=5, distortion=True, noise=2.0):
    return rs.case(G, V, J, distortion, seed=11, noise=noise)


def _gX(c):
    G, _, J = c['xy'].shape[:3]
    return torch.from_numpy(np.random.default_rng(12).normal(size=(G, J, 3)))


@functools.lru_cache(maxsize=None)
def _refs(key, use_w=True, use_omega=True, detach=False, undistort=True, vis_key=None, f32=False):
    """Both routes of the restatement on one case, computed once and shared."""
    c = dict(_case(*key))
    if f32:
        c['xy'] = c['xy'].float().double()               # the reference sees what the kernel reads
    vis = _vis(c) if vis_key else None
    w = c['w'] if use_w else None
    om = c['omega'] if use_omega else None
    if vis_key == 'zeros':
        vis, om = None, _omega_with_zeros(c)
    return tuple(rs.reference(c, vis, w, om, undistort, detach, route, _gX(c)) for route in ('svd', 'eigh'))


def _vis(c):
    vis = torch.ones(c['xy'].shape[:3], dtype=torch.uint8)
    vis[0, :2, 1] = 0                                    # joint 1 of group 0: exactly two views
    vis[1, 1:, 2] = 0                                    # joint 2 of group 1: one view
    vis[2, 3, 0] = 0                                     # joint 0 of group 2: three views
    return vis


def _omega_with_zeros(c):
    om = c['omega'].clone()
    om[0, 1, :] = 0
    om[2, :, 3] = 0
    return om


def _run(cuda, c, vis=None, w=None, omega=None, undistort=True, detach=False, dtype=torch.float64, view_major=False):
    """Every output of the Python layer on one case: X and the triangulation's gradients for gX, the loss, its X,
    e and gradients (xy's gradients come back in xy's own layout)."""
    from posu import ops
    M, intr = c['M'].to(cuda), c['intr'].to(cuda)
    xy0 = c['xy'].permute(1, 0, 2, 3).contiguous() if view_major else c['xy']
    visd = None if vis is None else vis.to(cuda)
    omd = None if omega is None else omega.to(cuda)
    out = {}
    xy = xy0.to(device=cuda, dtype=dtype).requires_grad_(True)
    wd = None if w is None else w.to(cuda).requires_grad_(True)
    X = ops.triangulate_points(M, intr, xy, visd, wd, undistort, view_major)
    (X * _gX(c).to(cuda)).sum().backward()
    out['X'], out['tri_gxy'], out['tri_gw'] = X.detach(), xy.grad, None if wd is None else wd.grad
    xy = xy0.to(device=cuda, dtype=dtype).requires_grad_(True)
    wd = None if w is None else w.to(cuda).requires_grad_(True)
    loss, LX = ops.reprojection_loss(M, intr, xy, visd, wd, omd, undistort, view_major, detach, return_points=True)
    assert not LX.requires_grad and loss.dtype == torch.float64 and loss.dim() == 0
    loss.backward()
    out['loss'], out['loss_X'], out['gxy'], out['gw'] = loss.detach(), LX, xy.grad, None if wd is None else wd.grad
    out['e'], _ = ops.reprojection_residuals(M, intr, xy.detach(), visd, wd, undistort, view_major)
    for k in ('tri_gxy', 'gxy'):
        assert out[k].dtype == dtype and out[k].shape == xy0.shape
        if view_major:
            out[k] = out[k].permute(1, 0, 2, 3)
    return out


def _compare(tag, out, svd, eigh, f32=False, weights=True):
    _check(tag + ' X', out['X'], svd['X'], eigh['X'])
    _check(tag + ' loss X', out['loss_X'], svd['X'], eigh['X'])
    _check(tag + ' e', out['e'], svd['e'], eigh['e'])
    _check(tag + ' loss', out['loss'], svd['loss'], eigh['loss'])
    _check(tag + ' tri gxy', out['tri_gxy'], svd['tri_gxy'], eigh['tri_gxy'], f32)
    _check(tag + ' gxy', out['gxy'], svd['gxy'], eigh['gxy'], f32)
    if weights:
        _check(tag + ' tri gw', out['tri_gw'], svd['tri_gw'], eigh['tri_gw'])
        _check(tag + ' gw', out['gw'], svd['gw'], eigh['gw'])


# ------------------------------------------------------------------ the cases
@pytest.mark.parametrize('detach', [False, True], ids=['through_point', 'detached'])
def test_f64_weighted_distorted(cuda, detach):
    c = _case()
    svd, eigh = _refs((3, 4, 5, True, 2.0), detach=detach)
    out = _run(cuda, c, None, c['w'], c['omega'], detach=detach)
    _compare('G3 V4 J5 f64' + (' detached' if detach else ''), out, svd, eigh)


@pytest.mark.parametrize('dtype', [torch.float64, torch.float32], ids=['f64', 'f32'])
@pytest.mark.parametrize('view_major', [False, True], ids=['group_major', 'view_major'])
def test_without_weights_the_point_is_triangulate_dlt_bit_for_bit(cuda, view_major, dtype):
    from posu import ops
    c = _case()
    M, intr = c['M'].to(cuda), c['intr'].to(cuda)
    xy = (c['xy'].permute(1, 0, 2, 3).contiguous() if view_major else c['xy']).to(device=cuda, dtype=dtype)
    vis = _vis(c).to(cuda)
    for v in (None, vis):
        want = ops.triangulate_dlt(M, intr, xy, v, True, view_major)
        got = ops.triangulate_points(M, intr, xy, v, None, True, view_major)
        assert torch.equal(got, want)
    svd, eigh = _refs((3, 4, 5, True, 2.0), use_w=False, use_omega=False, f32=dtype == torch.float32)
    out = _run(cuda, c, None, None, None, dtype=dtype, view_major=view_major)
    _compare('no weights %s %s' % ('view-major' if view_major else 'group-major', str(dtype).split('.')[1]), out, svd,
             eigh, f32=dtype == torch.float32, weights=False)


def test_f32_view_major_the_pipeline_layout(cuda):
    c = _case()
    svd, eigh = _refs((3, 4, 5, True, 2.0), f32=True)
    out = _run(cuda, c, None, c['w'], c['omega'], dtype=torch.float32, view_major=True)
    _compare('f32 view-major', out, svd, eigh, f32=True)


def test_pinhole_cameras_without_undistortion(cuda):
    key = (3, 4, 5, False, 2.0)
    c = _case(*key)
    assert float(c['intr'][:, :, 4:].abs().max()) == 0.0
    svd, eigh = _refs(key, undistort=False)
    out = _run(cuda, c, None, c['w'], c['omega'], undistort=False)
    _compare('pinhole undistort=0', out, svd, eigh)
    # the identity path of the undistortion: asking for it on these cameras changes no bit
    same = _run(cuda, c, None, c['w'], c['omega'], undistort=True)
    for k in out:
        assert torch.equal(out[k], same[k]), k


@pytest.mark.parametrize('V', [2, 3])
def test_two_and_three_view_rigs(cuda, V):
    key = (3, V, 5, True, 2.0)
    c = _case(*key)
    svd, eigh = _refs(key)
    _compare('V = %d' % V, _run(cuda, c, None, c['w'], c['omega']), svd, eigh)


def test_visibility_mask(cuda):
    c = _case()
    vis = _vis(c)
    svd, eigh = _refs((3, 4, 5, True, 2.0), vis_key='vis')
    out = _run(cuda, c, vis, c['w'], c['omega'])
    _compare('vis mask', out, svd, eigh)
    # the joint seen in one view: no point, no gradient, no loss contribution
    assert float(out['X'][1, 2].abs().max()) == 0.0 and float(out['loss_X'][1, 2].abs().max()) == 0.0
    assert float(out['e'][1, :, 2].abs().max()) == 0.0
    for k in ('tri_gxy', 'gxy', 'tri_gw', 'gw'):
        assert float(out[k][1, :, 2].abs().max()) == 0.0, k
    # views that are off get nothing; the two that remain of joint 1 of group 0 do
    off = vis == 0
    for k in ('tri_gxy', 'gxy', 'tri_gw', 'gw'):
        assert float(out[k][off.to(out[k].device)].abs().max()) == 0.0, k
    assert float(out['gxy'][0, 2:, 1].abs().min()) > 0.0


def test_target_weight_zeros_with_the_point_detached(cuda):
    c = _case()
    om = _omega_with_zeros(c)
    svd, eigh = _refs((3, 4, 5, True, 2.0), detach=True, vis_key='zeros')
    out = _run(cuda, c, None, c['w'], om, detach=True)
    _compare('omega zeros, detached', out, svd, eigh)
    assert float(out['gxy'][(om == 0).to(out['gxy'].device)].abs().max()) == 0.0
    assert float(out['gxy'][(om != 0).to(out['gxy'].device)].abs().min()) > 0.0
    assert float(out['gw'].abs().max()) == 0.0


def test_exact_projections_give_a_finite_loss_and_finite_gradients(cuda):
    c = _case(3, 4, 5, False, 0.0)                       # noise-free, no distortion: every residual is rounding noise
    for detach in (False, True):
        out = _run(cuda, c, None, c['w'], c['omega'], detach=detach)
        print('exact projections: loss %.3e px' % float(out['loss']))
        assert 0.0 <= float(out['loss']) < 1e-6
        for k in ('X', 'tri_gxy', 'tri_gw', 'gxy', 'gw', 'e'):
            assert torch.isfinite(out[k]).all(), k
        assert float((out['X'].cpu() - c['poses']).abs().max()) < 1e-5   # mm


@pytest.mark.parametrize('G,J', [(1, 1), (13, 5), (257, 1)], ids=['1', '65', '257'])
def test_loss_reduction_across_a_wave_and_a_block(cuda, G, J):
    from posu import ops
    key = (G, 4, J, True, 2.0)
    c = _case(*key)
    svd, eigh = _refs(key)
    loss = ops.reprojection_loss(c['M'].to(cuda), c['intr'].to(cuda), c['xy'].to(cuda), None, c['w'].to(cuda),
                                 c['omega'].to(cuda))
    _check('G J = %d loss' % (G * J), loss, svd['loss'], eigh['loss'])


def test_two_runs_give_the_same_bits(cuda):
    c = _case(13, 4, 5, True, 2.0)
    a = _run(cuda, c, _vis(c), c['w'], c['omega'])
    b = _run(cuda, c, _vis(c), c['w'], c['omega'])
    for k in a:
        assert torch.equal(a[k], b[k]), k
    a = _run(cuda, c, None, c['w'], None, dtype=torch.float32, view_major=True)
    b = _run(cuda, c, None, c['w'], None, dtype=torch.float32, view_major=True)
    for k in a:
        assert torch.equal(a[k], b[k]), k


def test_reprojection_loss_module_end_to_end(cuda):
    from core.loss import ReprojectionLoss
    from posu import ops
    N, V, J = 5, 4, 16
    cams = {(s, v): cam for s in syn.SUBJECTS for v, cam in enumerate(syn.h36m_like_cameras(s))}
    cfg = syn.make_cfg()
    crit = ReprojectionLoss(cfg, cams, device=cuda)
    c = _case(N, V, J, True, 2.0)                        # group g's rig is subject SUBJECTS[g % 2]: group_subjects
    subject = torch.from_numpy(syn.group_subjects(N))
    views = [c['xy'][:, v].float().to(cuda).requires_grad_(True) for v in range(V)]
    r = np.random.default_rng(13)
    tw = [torch.from_numpy((r.uniform(size=(N, J, 1)) > 0.2).astype(np.float32)).to(cuda) for _ in range(V)]
    conf = [torch.from_numpy(r.uniform(0.3, 1.0, size=(N, J))).to(cuda).requires_grad_(True) for _ in range(V)]
    meta = [{'subject': subject} for _ in range(V)]
    loss = crit(views, tw, meta, confidence=conf)
    loss.backward()
    # the same through ops on the gathered tables
    idx = crit.subject_indices(subject.numpy())
    assert torch.equal(crit.M[idx].cpu(), c['M']) and torch.equal(crit.intr[idx].cpu(), c['intr'])
    x = torch.stack([v.detach() for v in views], dim=0).requires_grad_(True)
    w = torch.stack([t.detach() for t in conf], dim=1).requires_grad_(True)
    want = ops.reprojection_loss(crit.M[idx], crit.intr[idx], x, None, w, torch.stack([t[..., 0] for t in tw], dim=1),
                                 view_major=True)
    want.backward()
    assert torch.equal(loss, want) and float(loss.detach()) > 0
    for v in range(V):
        assert views[v].grad is not None and views[v].grad.dtype == torch.float32
        assert torch.equal(views[v].grad, x.grad[v]) and float(views[v].grad.abs().max()) > 0
        assert torch.equal(conf[v].grad, w.grad[:, v]) and float(conf[v].grad.abs().max()) > 0
    # detached: the direct term only, nothing for the confidences; without target weights the loss changes
    views2 = [v.detach().clone().requires_grad_(True) for v in views]
    crit(views2, tw, meta, detach_point=True).backward()
    assert float((views2[0].grad - views[0].grad).abs().max()) > 0
    cfg.LOSS.USE_TARGET_WEIGHT_REPROJ = False
    plain = ReprojectionLoss(cfg, cams, device=cuda)(views, tw, meta)
    assert float(plain.detach()) != float(loss.detach())
    # and against the restatement, as everything else here
    ref = [rs.loss(c['M'], c['intr'], c['xy'].float().double(), None, w.detach().cpu(),
                   torch.stack([t[..., 0] for t in tw], dim=1).double().cpu(), route=route)[0] for route in ('svd', 'eigh')]
    _check('ReprojectionLoss', loss, ref[0], ref[1])
