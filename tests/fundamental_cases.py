"""The inputs of the fundamental-matrix tests, shared by test_fundamental_host.py (which asserts on the
restatement the conditions the GPU comparison relies on) and test_gpu_fundamental.py (which holds the kernel
to the restatement), and the restatement's results on them, computed once per process.

Synthetic H36M-like rigs without distortion, random 3-D poses, their projections.  The cases that are
compared bit for bit carry pixel noise: on exact projections every all-inlier hypothesis has a median of
rounding noise, and which of them wins is decided by the last bit."""
import functools
import itertools

import numpy as np

import fundamental_restatement as rs
from multiviews.cameras import project_pose
from posu import synthetic as syn

PAIRS = list(itertools.permutations(range(4), 2))


def projections(subject, groups, seed=0):
    """[G, 4, 16, 2] px of `groups` random poses in the subject's four views."""
    cams = syn.h36m_like_cameras(subject, distortion=False)
    X = syn.synthetic_poses3d(groups, 16, seed)
    return np.stack([np.stack([np.asarray(project_pose(X[g], cams[v]), dtype=np.float64) for v in range(4)])
                     for g in range(groups)])


def pair_points(poses, pairs):
    """poses [G, V, J, 2] -> [len(pairs), G * J, 4]: (x_i, y_i, x_j, y_j) of every group and joint."""
    return np.stack([np.concatenate([poses[:, i].reshape(-1, 2), poses[:, j].reshape(-1, 2)], axis=1)
                     for i, j in pairs])


def analytic(subject, pairs):
    cams = syn.h36m_like_cameras(subject, distortion=False)
    return np.stack([syn.fundamental(cams[i], cams[j]) for i, j in pairs])


def displace(pts, share, seed):
    """`share` of every problem's rows moved by 30 to 200 px in image j -> (pts, moved [P, N] bool)."""
    r = np.random.default_rng(seed)
    pts = pts.copy()
    P, N, _ = pts.shape
    moved = np.zeros((P, N), dtype=bool)
    for p in range(P):
        rows = r.choice(N, size=int(round(share * N)), replace=False)
        moved[p, rows] = True
        ang, dist = r.uniform(0, 2 * np.pi, len(rows)), r.uniform(30.0, 200.0, len(rows))
        pts[p, rows, 2] += dist * np.cos(ang)
        pts[p, rows, 3] += dist * np.sin(ang)
    return pts, moved


def _noisy(pts, sigma, seed):
    return pts + np.random.default_rng(seed).normal(0.0, sigma, size=pts.shape)


@functools.lru_cache(maxsize=None)
def gpu_cases():
    """name -> dict(pts [P, N, 4], valid [P, N] uint8 or None, H, seed): the P x N x H cases of the GPU test."""
    cases = {}
    one = pair_points(projections(9, 1, seed=1), [(0, 1)])
    cases['1x8x1'] = dict(pts=one[:, :8].copy(), valid=None, H=1, seed=11)
    odd = _noisy(pair_points(projections(9, 1, seed=2), [(0, 1), (1, 3), (2, 0)]), 0.3, 3)
    valid = np.ones((3, 16), dtype=np.uint8)
    for p, off in enumerate(([0, 3, 4, 7, 9, 12, 15], [1, 2, 5, 6, 8, 10, 11], [0, 1, 2, 13, 14, 15, 7])):
        valid[p, off] = 0
    cases['3x16x65'] = dict(pts=odd, valid=valid, H=65, seed=5)
    wide = _noisy(pair_points(projections(11, 9, seed=4), [(0, 2), (3, 1)]), 1.0, 6)
    cases['2x65x64'] = dict(pts=wide[:, :65].copy(), valid=None, H=64, seed=7)
    cases['2x129x64'] = dict(pts=wide[:, :129].copy(), valid=None, H=64, seed=8)
    half = _noisy(pair_points(projections(9, 2, seed=5), [(1, 2), (0, 3)]), 1.0, 9)
    cases['2x64x64 duplicated rows'] = dict(pts=np.concatenate([half, half], axis=1), valid=None, H=64, seed=10)
    out, _ = displace(_noisy(pair_points(projections(11, 8, seed=6), PAIRS), 0.3, 12), 0.3, 13)
    cases['12x128x256 outliers'] = dict(pts=out, valid=None, H=256, seed=14)
    return cases


@functools.lru_cache(maxsize=None)
def restated(name, linalg=False, seed_offset=0):
    c = gpu_cases()[name]
    return rs.lmeds(c['pts'], c['valid'], c['H'], c['seed'] + seed_offset, linalg=linalg)


def unit22(F):
    return F / F[..., 2:3, 2:3]


@functools.lru_cache(maxsize=None)
def spread(name):
    """The largest element-wise difference between the Jacobi and the numpy.linalg restatement's matrices
    (F[2][2] = 1): what the conditioning allows two correct fp64 solvers to differ by."""
    a, b = restated(name, False), restated(name, True)
    return float(np.abs(a['F'] - b['F']).max())
