"""posu_fundamental_lmeds and posu_epipolar_residual_stats on the device against the numpy restatement
(tests/fundamental_restatement.py), and the Python layers above them end to end.

cv2 is not installed, so the restatement is the reference; test_fundamental_host.py holds it to the analytic
matrices and shows that no case below has a near-tie between winners or at the inlier threshold.  `sample`,
`best` and `mask` must therefore be equal, bit for bit.  `F` (scaled to F[2][2] = 1) may differ by 16 x the
spread between the Jacobi and the numpy.linalg restatement, floored at 1e-12: hipcc contracts to FMA, numpy
does not, and the refit's sums are taken in another order."""
import math

import numpy as np
import pytest
import torch

import fundamental_cases as fc
import fundamental_restatement as rs
from posu import synthetic as syn

pytestmark = pytest.mark.gpu
CASES = list(fc.gpu_cases())


def _run(cuda, name, seed_offset=0, refit=True):
    from posu import ops
    c = fc.gpu_cases()[name]
    pts = torch.from_numpy(c['pts']).to(cuda)
    valid = None if c['valid'] is None else torch.from_numpy(c['valid']).to(cuda)
    out = ops.fundamental_lmeds(pts, valid, c['H'], c['seed'] + seed_offset, refit)
    return [t.cpu().numpy() for t in out]


@pytest.mark.parametrize('name', CASES)
def test_lmeds_equals_the_restatement(cuda, name):
    F, mask, sample, stats = _run(cuda, name)
    r = fc.restated(name)
    assert np.array_equal(sample, r['sample'])
    assert np.array_equal(stats[:, 3].astype(np.int64), r['best'])
    assert np.array_equal(mask, r['mask'])
    assert np.array_equal(stats[:, 2].astype(np.int64), r['n_inliers'])
    tol = max(16 * fc.spread(name), 1e-12)
    diff = np.abs(fc.unit22(F) - fc.unit22(r['F'])).max()
    print('%s: |F - restatement| %.3e (tolerance %.3e), median rel %.3e' % (
        name, diff, tol, np.abs(stats[:, 0] / r['median'] - 1).max()))
    assert diff <= tol
    # as distances: on exact data the winning median is rounding noise (1e-13 px), below the 1e-9 px the data
    # gate asks for and with no digits to compare
    np.testing.assert_allclose(np.sqrt(stats[:, 0]), np.sqrt(r['median']), rtol=1e-9, atol=1e-9)
    np.testing.assert_allclose(stats[:, 1], r['sigma'], rtol=1e-9, atol=1e-8)
    # the same seed: the same bits
    again = _run(cuda, name)
    for a, b in zip((F, mask, sample, stats), again):
        assert np.array_equal(a, b)
    # another seed: another sample, where there are more samples than hypotheses.  With n = 9 valid rows there
    # are 9 and the best of them wins under every seed, but as another hypothesis; with N = 8, H = 1 there is one
    c = fc.gpu_cases()[name]
    n = c['pts'].shape[1] if c['valid'] is None else int(c['valid'].sum(axis=1).min())
    other = _run(cuda, name, seed_offset=1000)
    if math.comb(n, 8) > c['H']:
        assert not np.array_equal(other[2], sample)
    elif c['H'] > 1:
        assert not np.array_equal(other[3][:, 3], stats[:, 3])


def test_the_unrefitted_winner_is_returned_with_refit_off(cuda):
    name = '2x65x64'
    F, mask, sample, stats = _run(cuda, name, refit=False)
    r = fc.restated(name)
    assert np.array_equal(sample, r['sample']) and np.array_equal(mask, r['mask'])
    assert np.abs(F - fc.unit22(r['winner_F'])).max() <= 1e-12


def test_degenerate_problems_give_a_zero_matrix_and_leave_the_others_alone(cuda):
    from multiviews import fundamental as fm
    from posu import ops
    good = fc.gpu_cases()['2x65x64']['pts'][0, :32]
    pts = np.stack([good, good, np.broadcast_to(good[5], good.shape)]).copy()
    valid = np.ones((3, 32), dtype=np.uint8)
    valid[1, 7:] = 0                                   # 7 valid rows
    F, mask, sample, stats = [t.cpu().numpy() for t in ops.fundamental_lmeds(
        torch.from_numpy(pts).to(cuda), torch.from_numpy(valid).to(cuda), 32, 3)]
    r = rs.lmeds(pts, valid, 32, 3)
    assert stats[0, 2] >= 8 and np.abs(F[0] - r['F'][0]).max() <= 1e-12 and np.array_equal(mask[0], r['mask'][0])
    for p in (1, 2):
        assert stats[p, 2] == 0 and not F[p].any() and not mask[p].any()
        assert r['n_inliers'][p] == 0
    assert (sample[1] == -1).all() and stats[1, 3] == -1 and np.isinf(stats[1, 0])
    # the device is healthy: the next call is the first one again
    F2 = ops.fundamental_lmeds(torch.from_numpy(pts).to(cuda), torch.from_numpy(valid).to(cuda), 32, 3)[0]
    assert np.array_equal(F2.cpu().numpy(), F)
    poses = fc.projections(9, 1, seed=3)
    few = np.zeros((1, 4, 16), dtype=np.uint8)
    few[:, :, :7] = 1
    with pytest.raises(ValueError, match=r'\(9, 0, 1\)'):
        fm.fundamental_matrix_dict(poses, [9], valid=few, hypotheses=16)
    with pytest.raises(ValueError, match=r'\(9, 0, 1\)'):
        fm.fundamental_matrix_dict(np.broadcast_to(poses[:, :, :1], poses.shape).copy(), [9], hypotheses=16)


@pytest.mark.parametrize('name', ['3x16x65', '12x128x256 outliers'])
def test_residual_stats_equal_numpy(cuda, name):
    from posu import ops
    c, r = fc.gpu_cases()[name], fc.restated(name)
    valid = None if c['valid'] is None else torch.from_numpy(c['valid']).to(cuda)
    got = ops.epipolar_residual_stats(torch.from_numpy(r['F']).to(cuda), torch.from_numpy(c['pts']).to(cuda), valid)
    want = rs.residual_stats(r['F'], c['pts'], c['valid'])
    print('%s: residual stats rel %.3e' % (name, np.abs(got.cpu().numpy() / want - 1).max()))
    np.testing.assert_allclose(got.cpu().numpy(), want, rtol=1e-12, atol=0)


def _two_subjects():
    poses = np.concatenate([fc.projections(s, 6, seed=40 + s) for s in syn.SUBJECTS])      # [12, 4, 16, 2]
    subjects = np.repeat(np.asarray(syn.SUBJECTS), 6)
    return poses, subjects


def test_end_to_end_dict_feeds_the_fundamental_loss(cuda, tmp_path):
    from core.loss import FundamentalLoss
    from multiviews import fundamental as fm
    poses, subjects = _two_subjects()
    d = fm.fundamental_matrix_dict(poses, subjects, hypotheses=64, seed=1)
    assert len(d) == 24 and all(np.array_equal(d[(s, j, i)], d[(s, i, j)].T) for s, i, j in d)
    for s in syn.SUBJECTS:
        cams = syn.h36m_like_cameras(s, distortion=False)
        for i, j in fc.PAIRS:
            assert np.abs(d[(s, i, j)] - syn.fundamental(cams[i], cams[j])).max() < 1e-9
    res = fm.epipolar_residuals(d, poses, subjects)
    assert len(res['per_key']) == 24 and res['mean'] <= res['max'] < 1e-6
    cfg = syn.make_cfg(data_root=str(tmp_path))
    joints = [torch.from_numpy(poses[:, v]).float().to(cuda) for v in range(4)]
    weight = [torch.ones(12, 16, 1, device=cuda) for _ in range(4)]
    meta = [{'subject': torch.from_numpy(subjects)} for _ in range(4)]
    ours = FundamentalLoss(cfg, fundamental_matrix_dict=d, device=cuda)(joints, weight, meta).item()
    ref = FundamentalLoss(cfg, fundamental_matrix_dict=syn.fundamental_dict(distortion=False), device=cuda)(
        joints, weight, meta).item()
    print('loss from the estimated table %.3e, from the analytic table %.3e' % (ours, ref))
    assert abs(ours - ref) < 1e-6
    fm.save_fundamental_dict(str(tmp_path / 'testdata' / 'fundamental_matrix.pkl'), d)
    from_file = FundamentalLoss(cfg, device=cuda)
    assert torch.equal(from_file.F, FundamentalLoss(cfg, fundamental_matrix_dict=d, device=cuda).F)


def test_device_locations_give_the_host_result(cuda):
    from multiviews import fundamental as fm
    poses, subjects = _two_subjects()
    r = np.random.default_rng(5)
    conf = r.uniform(0.3, 1.0, size=poses.shape[:3] + (1,))
    noisy = np.where(conf < 0.5, poses + 80.0, poses)                   # what a low confidence is a sign of
    loc = np.concatenate([noisy, conf], axis=3).astype(np.float32).reshape(48, 16, 3)
    on_device = torch.from_numpy(loc).to(cuda)                           # [G V, J, 3], as validate_device leaves it
    a = fm.fundamental_matrix_dict(on_device.view(12, 4, 16, 3), subjects, min_confidence=0.5, hypotheses=64, seed=2)
    b = fm.fundamental_matrix_dict(loc.reshape(12, 4, 16, 3), subjects, min_confidence=0.5, hypotheses=64, seed=2)
    assert sorted(a) == sorted(b) and len(a) == 24 and all(np.array_equal(a[k], b[k]) for k in a)
