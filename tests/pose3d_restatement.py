"""numpy fp64 restatement of the 3-D evaluation protocol (run/pose3d/estimate.py and
PoseUtils.procrustes, written out from their formulas) and the seeded input recipes shared by
tests/golden/make_pose3d_golden.py, the tests and tools/pose3d_micro.py.  Host only, not product
code: the package never imports it.

``procrustes`` uses numpy's SVD; ``procrustes_jacobi`` is the same arithmetic with the kernel's
one-sided Jacobi SVD (csrc/pose3d.hip) in place of LAPACK, for the summation-order-free part of
the kernel's error.
"""
import numpy as np

# the MPII tree of multiviews.body (joint -> parent)
PARENT = np.array([1, 2, 6, 6, 3, 4, -1, 6, 7, 8, 11, 12, 7, 7, 13, 14], dtype=np.int32)
LEAVES = (0, 5, 9, 10, 15)
REFLECTIONS = ('best', True, False)
SETTINGS = [(sc, rf) for sc in (True, False) for rf in REFLECTIONS]   # order of the golden's case axis


# ------------------------------------------------------------------ input recipes
def random_rotation(rng):
    """A proper rotation from a QR factorisation of a Gaussian matrix."""
    q, r = np.linalg.qr(rng.randn(3, 3))
    q = q * np.sign(np.diag(r))
    if np.linalg.det(q) < 0:
        q[:, 2] = -q[:, 2]
    return q


def make_pose(rng, joints):
    return rng.randn(joints, 3) * 400 + rng.randn(3) * 3000


def make_pair(rng, joints, mirrored=False):
    """(A, B): A a random pose (mm), B = A + 30 mm noise under a rotation, a 1 +- 0.1 scale and a shift;
    mirrored: the x axis of B flipped first, so the best fit is a reflection."""
    A = make_pose(rng, joints)
    B = A + rng.randn(joints, 3) * 30
    if mirrored:
        B = B * np.array([-1.0, 1.0, 1.0])
    B = (1 + rng.uniform(-0.1, 0.1)) * B.dot(random_rotation(rng)) + rng.randn(3) * 500
    return A, B


def make_groups(rng, groups, views, joints):
    """World poses and cameras for pose3d_errors: X [G, J, 3], gt [G, V, J, 3] (the pose in each camera's
    frame plus 30 mm noise and a 1 +- 0.05 scale about the camera), R [G, V, 3, 3], T [G, V, 3]."""
    X = np.stack([make_pose(rng, joints) for _ in range(groups)])
    R = np.stack([[random_rotation(rng) for _ in range(views)] for _ in range(groups)])
    T = rng.randn(groups, views, 3) * 2000 + np.array([0.0, 0.0, 4500.0])
    gt = np.empty((groups, views, joints, 3))
    for g in range(groups):
        for v in range(views):
            cam = R[g, v].dot(X[g].T - T[g, v].reshape(3, 1)).T
            gt[g, v] = (1 + rng.uniform(-0.05, 0.05)) * cam + rng.randn(joints, 3) * 30
    return X, gt, R, T


def make_limb_cases(seed, groups, per_group):
    """Poses for the limb check by a random walk over the MPII tree (only +, *, /, sqrt of a seeded
    RandomState stream, so every host draws the same bits): -> (poses [G, 16, 3], limb [16] or [G, 16],
    moved [G] bool).  In every group one leaf joint is moved along its limb, by 0.6 limb in the groups
    marked `moved` (about half) and by 0.1 limb in the others."""
    rng = np.random.RandomState(seed)
    base = rng.uniform(150, 450, 16)
    base[6] = 0.0
    limb = np.tile(base, (groups, 1)) * (rng.uniform(0.5, 2.0, (groups, 1)) if per_group else 1.0)
    poses = np.zeros((groups, 16, 3))
    moved = rng.uniform(size=groups) < 0.5
    order = [6, 2, 3, 7, 1, 4, 8, 12, 13, 0, 5, 9, 11, 14, 10, 15]       # parents before children
    for g in range(groups):
        poses[g, 6] = rng.randn(3) * 3000
        for c in order[1:]:
            d = rng.randn(3)
            poses[g, c] = poses[g, PARENT[c]] + d / np.sqrt((d * d).sum()) * limb[g, c]
        c = LEAVES[rng.randint(len(LEAVES))]
        step = (0.6 if moved[g] else 0.1) * (1.0 if rng.uniform() < 0.5 else -1.0)
        poses[g, c] = poses[g, c] + (poses[g, c] - poses[g, PARENT[c]]) * step
    return poses, (limb if per_group else base), moved


# --------------------------------------------------------------------- procrustes
def _finish(A, B, s, U, V, scaling, reflection, stats):
    a_bar, b_bar, ssx, ssy, a_norm, b_norm, B0 = stats
    R = V.dot(U.T)
    if reflection != 'best':
        if bool(reflection) != (np.linalg.det(R) < 0):
            V = V.copy()
            s = s.copy()
            V[:, -1] *= -1
            s[-1] *= -1
            R = V.dot(U.T)
    trace = s.sum()
    if scaling:
        scale = trace * a_norm / b_norm
        d = 1 - trace ** 2
        Z = a_norm * trace * B0.dot(R) + a_bar
    else:
        scale = 1.0
        d = 1 + ssy / ssx - 2 * trace * b_norm / a_norm
        Z = b_norm * B0.dot(R) + a_bar
    return d, Z, R, scale, a_bar - scale * b_bar.dot(R)


def _normalise(A, B):
    A, B = np.asarray(A, dtype=np.float64), np.asarray(B, dtype=np.float64)
    a_bar, b_bar = A.mean(0), B.mean(0)
    A0, B0 = A - a_bar, B - b_bar
    ssx, ssy = (A0 ** 2).sum(), (B0 ** 2).sum()
    a_norm, b_norm = np.sqrt(ssx), np.sqrt(ssy)
    A0, B0 = A0 / a_norm, B0 / b_norm
    return A0.T.dot(B0), (a_bar, b_bar, ssx, ssy, a_norm, b_norm, B0)


def procrustes(A, B, scaling=True, reflection='best'):
    """-> (d, Z [J, 3], R [3, 3], scale, t [3]) with Z = scale * B R + t."""
    with np.errstate(all='ignore'):
        M, stats = _normalise(A, B)
        if not np.isfinite(M).all():
            nan = np.full(3, np.nan)
            return np.nan, np.full(np.shape(A), np.nan), np.full((3, 3), np.nan), np.nan, nan
        U, s, Vt = np.linalg.svd(M)
        return _finish(A, B, s, U, Vt.T, scaling, reflection, stats)


def jacobi_svd3(M, sweeps=30):
    """One-sided Jacobi as the kernel runs it -> (U, s descending, V) with M = U diag(s) V^T."""
    W, V = np.array(M, dtype=np.float64), np.eye(3)
    for _ in range(sweeps):
        rotated = False
        for p in range(2):
            for q in range(p + 1, 3):
                alpha, beta, gamma = W[:, p].dot(W[:, p]), W[:, q].dot(W[:, q]), W[:, p].dot(W[:, q])
                if gamma != 0.0 and abs(gamma) > 1e-15 * np.sqrt(alpha * beta):
                    rotated = True
                    zeta = (beta - alpha) / (2.0 * gamma)
                    t = (1.0 if zeta >= 0 else -1.0) / (abs(zeta) + np.sqrt(1.0 + zeta * zeta))
                    cs = 1.0 / np.sqrt(1.0 + t * t)
                    sn = cs * t
                    for X in (W, V):
                        xp, xq = X[:, p].copy(), X[:, q].copy()
                        X[:, p], X[:, q] = cs * xp - sn * xq, sn * xp + cs * xq
        if not rotated:
            break
    s = np.sqrt((W * W).sum(0))
    U = W / s
    k = int(np.argmin(s))
    if not s[k] > 1e-14 * s.max():                       # rank 2: complete U, as the kernel does
        U[:, k] = np.cross(U[:, (k + 1) % 3], U[:, (k + 2) % 3])
    order = np.argsort(-s, kind='stable')
    return U[:, order], s[order], V[:, order]


def procrustes_jacobi(A, B, scaling=True, reflection='best'):
    with np.errstate(all='ignore'):
        M, stats = _normalise(A, B)
        U, s, V = jacobi_svd3(M)
        return _finish(A, B, s, U, V, scaling, reflection, stats)


# ------------------------------------------------------------------------- errors
def pose3d_errors(X, gt, R, T, use_procrustes=False):
    """X [G, J, 3], gt [G, V, J, 3], R [G, V, 3, 3], T [G, V, 3] -> (err [G, V, J], pred [G, V, J, 3])."""
    X, gt, R, T = (np.asarray(a, dtype=np.float64) for a in (X, gt, R, T))
    err, pred = np.empty(gt.shape[:3]), np.empty(gt.shape)
    for g in range(gt.shape[0]):
        for v in range(gt.shape[1]):
            p = R[g, v].dot(X[g].T - T[g, v].reshape(3, 1)).T
            if use_procrustes:
                p = procrustes(gt[g, v], p)[1]
            pred[g, v] = p
            err[g, v] = np.linalg.norm(gt[g, v] - p, axis=1)
    return err, pred


# --------------------------------------------------------------------- limb check
def limb_break(poses, parent, limb, thres=0.4):
    """poses [G, J, 3]; limb [J] or [G, J] by child -> (flag [G] bool, worst [G])."""
    poses = np.asarray(poses, dtype=np.float64)
    limb = np.broadcast_to(np.asarray(limb, dtype=np.float64), poses.shape[:2])
    kids = np.flatnonzero(np.asarray(parent) >= 0)
    with np.errstate(all='ignore'):
        actual = np.linalg.norm(poses[:, np.asarray(parent)[kids]] - poses[:, kids], axis=2)
        offset = np.abs(limb[:, kids] - actual)
        rel = offset / limb[:, kids]
        return (offset > thres * limb[:, kids]).any(1), np.where(np.isnan(rel), 0.0, rel).max(1, initial=0.0)


# ------------------------------------------------------------------------- report
def summary(err_batches, action_batches, refined_batches=None, before_batches=None):
    """estimate.py:215-277 over batches of err [G, V, J]: every (group, camera) is one sample."""
    errors, action_sum, action_hits, before, after = [], {}, {}, [], []
    for b, (err, actions) in enumerate(zip(err_batches, action_batches)):
        for g in range(err.shape[0]):
            errs = [err[g, v] for v in range(err.shape[1])]
            if refined_batches is not None and refined_batches[b][g]:
                after.append(np.mean(errs))
                if before_batches is not None:
                    before.append(np.mean(before_batches[b][g]))
            errors += errs
            a = int(actions[g])
            action_sum[a] = action_sum.get(a, 0.0) + np.mean(errs)
            action_hits[a] = action_hits.get(a, 0) + 1
    table = np.array(errors).T                                           # [J, samples]
    return {'mpjpe': float(np.mean(table)), 'joint_wise': np.mean(table, 1),
            'variance': float(np.var(np.mean(table, 0))),
            'action_wise': {a: action_sum[a] / action_hits[a] for a in action_sum},
            'compare': {'before': float(np.mean(before)) if before else float('nan'),
                        'after': float(np.mean(after))} if after else None,
            'pict_struct_count': len(after), 'groups': sum(e.shape[0] for e in err_batches)}
