"""Fundamental-matrix estimation, host side.  No kernel is launched here.

The three posu_* entry points are declared, exported and bound and answer their argument errors before any
launch; the Python layers refuse CPU tensors; fundamental_matrix_dict's layout of problems is checked with a
fake estimator.  The restatement (tests/fundamental_restatement.py), which the GPU test holds the kernel to,
is itself held to the analytic matrices of the synthetic rigs:

  clean projections, all 12 pairs, N = 16, 32, 128: the largest point-to-epipolar-line distance on the data
  must stay below 1e-9 px.  Measured with the Jacobi form: 3.3e-12, 3.3e-12 and 7.2e-12 px (numpy.linalg
  form: 2.2e-12, 3.4e-12, 7.6e-12), all below the 1e-10 the plain numpy pipeline suggested.
  30 % of the rows displaced by 30 to 200 px, H = 256: no displaced row in the mask, the refit within
  1e-9 px on the clean rows (measured 1.2e-11 px).

Jacobi against numpy.linalg on the GPU test's cases: the same sample, winner and mask, and matrices
(F[2][2] = 1) that differ by at most 2.7e-16 element-wise (3.0e-14 on the noise-free 1 x 8 x 1 case): the
GPU tolerance, 16 x that spread, therefore sits on its floor of 1e-12.  On the GPU the matrices came within
2.0e-15 of the restatement's (1 x 8 x 1), 8.1e-16 (3 x 16 x 65) and 3.2e-17 or less on the other cases.

The GPU test demands equal samples, winners and masks.  So that this cannot hide a near-tie, the restatement
must show on every case that (a) the winning median and the smallest median of a hypothesis with OTHER rows
differ by more than 1e-6 relative, and (b) no row's error is within 1e-6 relative of sigma^2.  Hypotheses
that drew the same 8 rows are sorted into the same hypothesis, bit for bit, on both sides (with n = 9 and
H = 65 there are only 9 distinct ones), so they tie exactly and the lowest h wins: that is no near-tie."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

import fundamental_cases as fc
import fundamental_restatement as rs
from posu import _native

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(REPO, 'pose-unsupervised_amd', 'csrc')
SYMBOLS = ('posu_fundamental_lmeds', 'posu_fundamental_workspace', 'posu_epipolar_residual_stats')
CASES = list(fc.gpu_cases())


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


def test_philox_has_one_home():
    holders = [f for f in sorted(os.listdir(CSRC)) if '0xD2511F53' in open(os.path.join(CSRC, f)).read()]
    assert holders == ['philox_common.h']
    for user in ('mi_sample.hip', 'fundamental.hip'):
        assert '#include "philox_common.h"' in open(os.path.join(CSRC, user)).read()


def test_workspace_query_answers_on_the_host():
    ws = _native.load().posu_fundamental_workspace
    assert ws(42, 8192, 512) == 42 * 512 * (9 * 8 + 8 + 8 * 4)
    assert ws(1, 8, 1) == 112
    for bad in ((0, 16, 4), (-1, 16, 4), (1, 7, 4), (1, 16, 0), (65536, 16, 4), (1, (1 << 26) + 1, 4),
                (1, 16, (1 << 20) + 1)):
        assert ws(*bad) == -1, bad
    from posu import ops
    assert ops.fundamental_workspace(3, 16, 65) == ws(3, 16, 65)
    with pytest.raises(ValueError, match='N'):
        ops.fundamental_workspace(1, 7, 4)


def test_argument_errors_are_reported_before_any_launch():
    lib = _native.load()
    p = ctypes.c_void_p(256)

    def err(st, text):
        assert st == 1, st
        assert text in _native.last_error(), _native.last_error()

    def lmeds(pts=p, valid=None, P=2, N=16, H=4, F=p, mask=p, sample=p, stats=p, ws=p, nbytes=1 << 20):
        return lib.posu_fundamental_lmeds(pts, valid, P, N, H, 0, 1, F, mask, sample, stats, ws, nbytes, None)
    for kw in ({'pts': None}, {'F': None}, {'mask': None}, {'sample': None}, {'stats': None}, {'ws': None}):
        err(lmeds(**kw), 'null pointer')
    err(lmeds(N=7), 'N must be at least 8')
    err(lmeds(H=0), 'H must be at least 1')
    err(lmeds(P=0), 'P')
    err(lmeds(nbytes=2 * 4 * 112 - 1), 'workspace too small')
    err(lmeds(ws=ctypes.c_void_p(260)), 'aligned')

    def stats(F=p, pts=p, P=2, N=16, out=p):
        return lib.posu_epipolar_residual_stats(F, pts, None, P, N, out, None)
    for kw in ({'F': None}, {'pts': None}, {'out': None}):
        err(stats(**kw), 'null pointer')
    for kw in ({'P': 0}, {'N': 0}):
        err(stats(**kw), 'bad shape')


def test_python_layers_refuse_cpu_tensors(monkeypatch):
    from multiviews import fundamental as fm
    from posu import ops
    pts = torch.zeros(2, 16, 4, dtype=torch.float64)
    with pytest.raises(RuntimeError, match='cuda'):
        ops.fundamental_lmeds(pts)
    with pytest.raises(RuntimeError, match='cuda'):
        ops.epipolar_residual_stats(torch.zeros(2, 3, 3, dtype=torch.float64), pts)
    with pytest.raises(RuntimeError, match='cuda'):
        fm.estimate_fundamental(pts[:, :, :2], pts[:, :, 2:])
    monkeypatch.setattr(torch.cuda, 'is_available', lambda: False)
    with pytest.raises(RuntimeError, match='cuda'):
        fm.fundamental_matrix_dict(np.zeros((2, 4, 16, 2)), [9, 11])
    with pytest.raises(RuntimeError, match='cuda'):
        fm.epipolar_residuals({}, np.zeros((2, 4, 16, 2)), [9, 11])


# ------------------------------------------------------------------ the restatement against the analytic matrix
def test_draws_are_distinct_valid_sorted_and_bounded():
    valid = np.zeros(40, dtype=bool)
    valid[::3] = True                                   # 14 valid rows
    for h in range(20):
        rows = rs.draw(40, valid, 77, 3, h)
        assert rows is not None and rows == sorted(set(rows)) and len(rows) == 8 and valid[rows].all()
        assert rows == rs.draw(40, valid, 77, 3, h)
    assert len({tuple(rs.draw(40, valid, 77, 3, h)) for h in range(20)}) > 1
    valid[21:] = False                                  # 7 valid rows: the 64th rejection gives up
    assert all(rs.draw(40, valid, 77, 3, h) is None for h in range(8))


@pytest.mark.parametrize('groups', [1, 2, 8])
@pytest.mark.parametrize('linalg', [False, True], ids=['jacobi', 'linalg'])
def test_restatement_recovers_the_analytic_matrix_on_clean_data(groups, linalg):
    pts = fc.pair_points(fc.projections(9, groups, seed=20 + groups), fc.PAIRS)
    r = rs.lmeds(pts, None, 64, 3, linalg=linalg)
    assert (r['n_inliers'] == 16 * groups).all()
    worst = max(rs.epipolar_distance(r['F'][p], pts[p]).max() for p in range(len(fc.PAIRS)))
    print('N = %d, %s: largest point-to-line distance %.3e px, |F - analytic| %.3e'
          % (16 * groups, 'linalg' if linalg else 'jacobi', worst, np.abs(r['F'] - fc.analytic(9, fc.PAIRS)).max()))
    assert worst < 1e-9
    # the convention: x_j^T F x_i = 0, F[2][2] = 1, as posu.synthetic.fundamental has it
    assert np.abs(r['F'][:, 2, 2] - 1.0).max() == 0.0
    assert rs.residual_stats(r['F'], pts)[:, 1].max() < 1e-9


def test_restatement_rejects_displaced_rows():
    pts, moved = fc.displace(fc.pair_points(fc.projections(9, 8, seed=30), fc.PAIRS), 0.3, 31)
    r = rs.lmeds(pts, None, 256, 4)
    assert not (r['mask'].astype(bool) & moved).any()
    assert (r['n_inliers'] >= 8).all()
    worst = max(rs.epipolar_distance(r['F'][p], pts[p][~moved[p]]).max() for p in range(len(fc.PAIRS)))
    print('refit on the clean rows: %.3e px' % worst)
    assert worst < 1e-9


# ------------------------------------------------------------------ what the GPU test relies on
@pytest.mark.parametrize('name', CASES)
def test_jacobi_and_linalg_restatements_agree(name):
    a, b = fc.restated(name, False), fc.restated(name, True)
    for key in ('sample', 'best', 'mask', 'n_inliers'):
        assert np.array_equal(a[key], b[key]), key
    assert (a['n_inliers'] >= 8).all()                  # every case is solvable: the degenerate ones are apart
    print('%s: Jacobi against numpy.linalg, largest element-wise difference %.3e' % (name, fc.spread(name)))
    assert fc.spread(name) < 1e-12 / 16                 # the GPU tolerance is its floor on every case


@pytest.mark.parametrize('name', CASES)
def test_no_near_ties_in_the_gpu_cases(name):
    c, r = fc.gpu_cases()[name], fc.restated(name)
    for p in range(c['pts'].shape[0]):
        med, rows, hb = r['medians'][p], r['samples'][p], r['best'][p]
        assert med[hb] == med.min() and hb == int(np.argmin(med))
        others = [med[h] for h in range(c['H']) if not np.array_equal(rows[h], rows[hb])]
        same = [med[h] for h in range(c['H']) if np.array_equal(rows[h], rows[hb])]
        assert all(m == med[hb] for m in same)          # the same rows: the same bits
        if others:
            assert min(others) - med[hb] > 1e-6 * med[hb], (p, med[hb], min(others))
        e = r['errors'][p]
        e = e[np.isfinite(e)]
        assert np.abs(e / r['sigma'][p] ** 2 - 1.0).min() > 1e-6, p


# ------------------------------------------------------------------ fundamental_matrix_dict's plumbing
class _Fake:
    """estimate_fundamental's stand-in: records its inputs, returns matrix k = [[k, 1, 2], [3, 4, 5], [6, 7, 1]]."""

    def __init__(self, few=None):
        self.calls, self.few = [], few

    def __call__(self, pts_i, pts_j, valid=None, hypotheses=512, seed=0, refit=True):
        self.calls.append((pts_i, pts_j, valid, hypotheses, seed))
        n = pts_i.shape[0]
        F = torch.tensor([[0., 1, 2], [3, 4, 5], [6, 7, 1]], dtype=torch.float64).repeat(n, 1, 1)
        F[:, 0, 0] = torch.arange(n, dtype=torch.float64)
        inl = torch.full((n,), 16, dtype=torch.int64)
        if self.few is not None:
            inl[self.few] = 7
        return F, torch.ones(pts_i.shape[:2], dtype=torch.uint8), {'n_inliers': inl}


def _plumbing(monkeypatch, few=None):
    from multiviews import fundamental as fm
    fake = _Fake(few)
    monkeypatch.setattr(fm, '_device', lambda: torch.device('cpu'))
    monkeypatch.setattr(fm, 'estimate_fundamental', fake)
    return fm, fake


def test_dict_keys_transposes_rows_and_padding(monkeypatch):
    fm, fake = _plumbing(monkeypatch)
    subjects = [9, 11, 9, 9, 11]
    poses = np.random.default_rng(0).uniform(0, 1000, size=(5, 4, 16, 2))
    d = fm.fundamental_matrix_dict(poses, subjects, hypotheses=33, seed=5)
    assert sorted(d) == sorted((s, i, j) for s in (9, 11) for i, j in fc.PAIRS) and len(d) == 24
    for (s, i, j), F in d.items():
        assert F.dtype == np.float64 and F.shape == (3, 3)
        assert np.array_equal(d[(s, j, i)], F.T)
    assert d[(9, 0, 1)][0, 0] == 0 and d[(9, 2, 3)][0, 0] == 5 and d[(11, 0, 1)][0, 0] == 6
    (xi, xj, valid, hyp, seed), = fake.calls
    assert (hyp, seed) == (33, 5) and tuple(xi.shape) == (12, 48, 2) and tuple(valid.shape) == (12, 48)
    # problem 1 is (9, 0, 2): the subject's groups 0, 2, 3, joint-minor; problem 8 is (11, 0, 3), padded
    assert np.array_equal(xi[1].numpy(), poses[[0, 2, 3], 0].reshape(48, 2))
    assert np.array_equal(xj[1].numpy(), poses[[0, 2, 3], 2].reshape(48, 2))
    assert valid[1].all()
    assert np.array_equal(xj[8, :32].numpy(), poses[[1, 4], 3].reshape(32, 2))
    assert valid[8, :32].all() and not valid[8, 32:].any()


def test_dict_first_frames_validity_and_confidence(monkeypatch):
    fm, fake = _plumbing(monkeypatch)
    subjects = [11, 9, 11]
    poses = np.random.default_rng(1).uniform(0, 1000, size=(3, 4, 16, 3))
    poses[:, :, :, 2] = 0.9
    poses[2, 1, 5, 2] = 0.1                              # not the first group of subject 11: ignored by 'first'
    poses[0, 1, 4, 2] = 0.1
    valid = np.ones((3, 4, 16), dtype=np.uint8)
    valid[1, 3, 7] = 0
    fm.fundamental_matrix_dict(torch.from_numpy(poses), subjects, valid=valid, min_confidence=0.5, frames='first')
    xi, xj, ok, _, _ = fake.calls[0]
    assert tuple(xi.shape) == (12, 16, 2)
    assert np.array_equal(xi[0].numpy(), poses[0, 0, :, :2]) and np.array_equal(xj[0].numpy(), poses[0, 1, :, :2])
    assert np.array_equal(xi[6].numpy(), poses[1, 0, :, :2])             # subject 9 comes second: its group 1
    expect = np.ones((12, 16), dtype=np.uint8)
    pairs = [(i, j) for i in range(4) for j in range(i + 1, 4)]
    for k, (i, j) in enumerate(pairs):
        if 1 in (i, j):
            expect[k, 4] = 0                             # subject 11, view 1, joint 4: low confidence
        if 3 in (i, j):
            expect[6 + k, 7] = 0                         # subject 9, view 3, joint 7: invalid
    assert np.array_equal(ok.numpy(), expect)
    with pytest.raises(ValueError, match='min_confidence'):
        fm.fundamental_matrix_dict(poses[..., :2], subjects, min_confidence=0.5)
    with pytest.raises(ValueError, match='frames'):
        fm.fundamental_matrix_dict(poses, subjects, frames='some')


def test_dict_names_the_key_that_kept_too_few_inliers(monkeypatch):
    fm, _ = _plumbing(monkeypatch, few=7)
    with pytest.raises(ValueError, match=r'\(11, 0, 2\)'):
        fm.fundamental_matrix_dict(np.zeros((2, 4, 16, 2)), [9, 11])


def test_from_db_and_saved_pickle(monkeypatch, tmp_path):
    fm, fake = _plumbing(monkeypatch)
    r = np.random.default_rng(2)
    db = [{'joints_2d': r.uniform(0, 1000, size=(16, 2)), 'subject': 9 if k < 8 else 11} for k in range(16)]
    grouping = [[0, 1, 2, 3], [4, 5, 6, 7], [8, 9, 10, 11], [12, 13, 14, 15]]
    d = fm.fundamental_from_db(db, grouping, frames='first')
    xi = fake.calls[0][0]
    assert np.array_equal(xi[0].numpy(), db[0]['joints_2d']) and np.array_equal(xi[6].numpy(), db[8]['joints_2d'])
    path = tmp_path / 'testdata' / 'fundamental_matrix.pkl'
    fm.save_fundamental_dict(str(path), d)
    import pickle
    with open(path, 'rb') as f:
        back = pickle.load(f)
    assert sorted(back) == sorted(d) and all(np.array_equal(back[k], d[k]) for k in d)
