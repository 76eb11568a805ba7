"""posu_fundamental_lmeds restated in numpy fp64 (include/posu.h has the definition): the Philox draws, the
sorted sample, the Hartley normalisation, the 8 x 9 system, the one-sided Jacobi of csrc/geometry_common.h
in the kernel's pair order, rank 2, the symmetric epipolar error, the rank-n/2 element, the sigma rule, the
inlier mask, the refit on the 9 x 9 Gram matrix and the scaling.  cv2 is not installed, so this is what the
kernel is held to: `sample`, `best` and `mask` bit for bit, `F` to a tolerance (numpy rounds every product
and sum on its own, hipcc contracts to FMA, and the refit's sums are taken in another order).

linalg=True replaces the two decompositions (the null vector and the 3 x 3 SVD) by numpy.linalg's: the
difference between the two forms is the spread the conditioning allows.

Everything is batched over a leading axis, so that a case of a few thousand hypotheses takes a second."""
import numpy as np

from heatmap_mi_sampler_restatement import bounded, philox4x32_10

SAMPLE = 8
MAX_REJECTS = 64
SIGMA_FLOOR = 1e-3
MASK32 = 0xFFFFFFFF


# ------------------------------------------------------------------ draws
def draw(n_rows, valid, seed, p, h):
    """The 8 sorted rows of hypothesis h of problem p, or None when 64 candidates were rejected."""
    key = (seed & MASK32, (seed >> 32) & MASK32)
    rows, rejected, b = [], 0, 0
    while len(rows) < SAMPLE and rejected < MAX_REJECTS:
        for w in philox4x32_10((b, h, p, 0), key):
            if len(rows) == SAMPLE or rejected == MAX_REJECTS:
                break
            cand = bounded(w, n_rows)
            if (valid is not None and not valid[cand]) or cand in rows:
                rejected += 1
            else:
                rows.append(cand)
        b += 1
    return sorted(rows) if len(rows) == SAMPLE else None


# ------------------------------------------------------------------ the Jacobi of geometry_common.h, batched
def jacobi_columns(A):
    """A [B, R, N] -> (A V, V): column pairs (p, q), p < q, in the kernel's order, at most 30 sweeps; a matrix
    whose sweep rotated nothing is finished (further sweeps would not touch it either)."""
    A = np.array(A, dtype=np.float64)
    B, R, N = A.shape
    V = np.broadcast_to(np.eye(N), (B, N, N)).copy()
    with np.errstate(all='ignore'):
        for _ in range(30):
            rotated = np.zeros(B, dtype=bool)
            for p in range(N - 1):
                for q in range(p + 1, N):
                    alpha, beta, gamma = np.zeros(B), np.zeros(B), np.zeros(B)
                    for r in range(R):
                        alpha = alpha + A[:, r, p] * A[:, r, p]
                        beta = beta + A[:, r, q] * A[:, r, q]
                        gamma = gamma + A[:, r, p] * A[:, r, q]
                    go = (gamma != 0.0) & (np.abs(gamma) > 1e-15 * np.sqrt(alpha * beta))
                    if not go.any():
                        continue
                    rotated |= go
                    zeta = (beta - alpha) / (2.0 * gamma)
                    tt = np.where(zeta >= 0, 1.0, -1.0) / (np.abs(zeta) + np.sqrt(1.0 + zeta * zeta))
                    cs = 1.0 / np.sqrt(1.0 + tt * tt)
                    sn = cs * tt
                    for M in (A, V):
                        mp, mq = M[:, :, p].copy(), M[:, :, q].copy()
                        g = go[:, None]
                        M[:, :, p] = np.where(g, cs[:, None] * mp - sn[:, None] * mq, mp)
                        M[:, :, q] = np.where(g, sn[:, None] * mp + cs[:, None] * mq, mq)
            if not rotated.any():
                break
    return A, V


def _first_smallest_column(A):
    """Index of the column of the smallest squared norm, the first of equals; comparisons with NaN are false."""
    B, R, N = A.shape
    best, col = None, np.zeros(B, dtype=np.int64)
    with np.errstate(all='ignore'):
        for c in range(N):
            n = np.zeros(B)
            for r in range(R):
                n = n + A[:, r, c] * A[:, r, c]
            if c == 0:
                best = n
            else:
                less = n < best
                best = np.where(less, n, best)
                col = np.where(less, c, col)
    return col


def null_vector(A, linalg=False):
    """A [B, R, 9] -> the right singular vector of the smallest singular value, [B, 9]."""
    B = A.shape[0]
    if linalg:
        out = np.full((B, 9), np.nan)
        for b in range(B):
            if np.isfinite(A[b]).all():
                out[b] = np.linalg.svd(A[b], full_matrices=True)[2][-1]
        return out
    AV, V = jacobi_columns(A)
    col = _first_smallest_column(AV)
    return V[np.arange(B), :, col]


def system_rows(xi, yi, xj, yj):
    one = np.ones_like(xi)
    return np.stack([xj * xi, xj * yi, xj, yj * xi, yj * yi, yj, xi, yi, one], axis=-1)


def finish_matrix(f, hi, hj, linalg=False):
    """f [B, 9], hi / hj = (cx, cy, s) each [B] -> F [B, 3, 3]: rank 2, then T_j^T F^ T_i."""
    B = f.shape[0]
    Fh = f.reshape(B, 3, 3)
    with np.errstate(all='ignore'):
        if linalg:
            R = np.full((B, 3, 3), np.nan)
            for b in range(B):
                if np.isfinite(Fh[b]).all():
                    u, s, vt = np.linalg.svd(Fh[b])
                    s[2] = 0.0
                    R[b] = (u * s) @ vt
        else:
            A, V = jacobi_columns(Fh)
            n = [A[:, 0, c] * A[:, 0, c] + A[:, 1, c] * A[:, 1, c] + A[:, 2, c] * A[:, 2, c] for c in range(3)]
            drop = np.zeros(B, dtype=np.int64)
            drop = np.where(n[1] < n[0], 1, drop)
            drop = np.where(n[2] < np.where(drop == 1, n[1], n[0]), 2, drop)
            R = np.zeros((B, 3, 3))
            for r in range(3):
                for k in range(3):
                    s = np.zeros(B)
                    for c in range(3):
                        s = s + np.where(drop == c, 0.0, A[:, r, c] * V[:, k, c])
                    R[:, r, k] = s
        (cxi, cyi, si), (cxj, cyj, sj) = hi, hj
        M = np.zeros((B, 3, 3))
        M[:, :, 0] = R[:, :, 0] * si[:, None]
        M[:, :, 1] = R[:, :, 1] * si[:, None]
        M[:, :, 2] = R[:, :, 2] - si[:, None] * (cxi[:, None] * R[:, :, 0] + cyi[:, None] * R[:, :, 1])
        F = np.zeros((B, 3, 3))
        F[:, 0, :] = sj[:, None] * M[:, 0, :]
        F[:, 1, :] = sj[:, None] * M[:, 1, :]
        F[:, 2, :] = M[:, 2, :] - sj[:, None] * (cxj[:, None] * M[:, 0, :] + cyj[:, None] * M[:, 1, :])
    return F


def solve_samples(x, linalg=False):
    """x [B, 8, 4] -> F [B, 3, 3]: the normalised 8-point algorithm on 8 rows."""
    with np.errstate(all='ignore'):
        s = np.zeros((x.shape[0], 4))
        for k in range(SAMPLE):
            s = s + x[:, k, :]
        c = s / SAMPLE
        di, dj = np.zeros(x.shape[0]), np.zeros(x.shape[0])
        for k in range(SAMPLE):
            d = x[:, k, :] - c
            di = di + np.sqrt(d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1])
            dj = dj + np.sqrt(d[:, 2] * d[:, 2] + d[:, 3] * d[:, 3])
        si, sj = np.sqrt(2.0) / (di / SAMPLE), np.sqrt(2.0) / (dj / SAMPLE)
        d = x - c[:, None, :]
        A = system_rows(si[:, None] * d[:, :, 0], si[:, None] * d[:, :, 1], sj[:, None] * d[:, :, 2],
                        sj[:, None] * d[:, :, 3])
        f = null_vector(A, linalg)
    return finish_matrix(f, (c[:, 0], c[:, 1], si), (c[:, 2], c[:, 3], sj), linalg)


# ------------------------------------------------------------------ errors
def epipolar_errors(F, x):
    """F [..., 3, 3], x [N, 4] -> max(d_i^2, d_j^2) [..., N]; NaN -> +inf."""
    F = np.asarray(F)[..., None, :, :]
    xi, yi, xj, yj = x[:, 0], x[:, 1], x[:, 2], x[:, 3]
    with np.errstate(all='ignore'):
        a = F[..., 0, 0] * xi + F[..., 0, 1] * yi + F[..., 0, 2]
        b = F[..., 1, 0] * xi + F[..., 1, 1] * yi + F[..., 1, 2]
        c = F[..., 2, 0] * xi + F[..., 2, 1] * yi + F[..., 2, 2]
        s = xj * a + yj * b + c
        s2 = s * s
        at = F[..., 0, 0] * xj + F[..., 1, 0] * yj + F[..., 2, 0]
        bt = F[..., 0, 1] * xj + F[..., 1, 1] * yj + F[..., 2, 1]
        e = np.fmax(s2 / (at * at + bt * bt), s2 / (a * a + b * b))
    return np.where(np.isnan(e), np.inf, e)


def epipolar_distance(F, x):
    """The larger of the two point-to-line distances, px: sqrt of the error above."""
    return np.sqrt(epipolar_errors(F, x))


def scale_matrix(F):
    """F[2][2] = 1, or Frobenius norm 1 when |F[2][2]| <= 1e-7 max|F|; None for a zero or non-finite matrix."""
    mx = np.abs(F).max()
    if not np.isfinite(F).all() or not mx > 0.0:
        return None
    fro = 0.0
    for v in F.reshape(-1):
        fro = fro + v * v
    return F / (np.sqrt(fro) if abs(F[2, 2]) <= 1e-7 * mx else F[2, 2])


def refit(x, linalg=False):
    """The normalised 8-point solve over the rows x [n, 4] on their 9 x 9 Gram matrix."""
    n = x.shape[0]
    with np.errstate(all='ignore'):
        c = x.sum(axis=0) / n
        d = x - c
        si = np.sqrt(2.0) / (np.sqrt(d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]).sum() / n)
        sj = np.sqrt(2.0) / (np.sqrt(d[:, 2] * d[:, 2] + d[:, 3] * d[:, 3]).sum() / n)
        A = system_rows(si * d[:, 0], si * d[:, 1], sj * d[:, 2], sj * d[:, 3])
        G = np.zeros((9, 9))
        for u in range(9):
            for v in range(u, 9):
                G[u, v] = G[v, u] = (A[:, u] * A[:, v]).sum()
        if linalg:
            f = np.linalg.eigh(G)[1][:, 0][None] if np.isfinite(G).all() else np.full((1, 9), np.nan)
        else:
            f = null_vector(G[None], False)
    one = np.ones(1)
    return finish_matrix(f, (c[0] * one, c[1] * one, si * one), (c[2] * one, c[3] * one, sj * one), linalg)[0]


# ------------------------------------------------------------------ the estimator
def lmeds(pts, valid=None, hypotheses=512, seed=0, do_refit=True, linalg=False):
    """pts [P, N, 4], valid [P, N] or None -> dict of F [P, 3, 3], mask [P, N] uint8, sample [P, 8] int32,
    median, sigma, n_inliers, best [P], and for the tests medians [P, H], samples [P, H, 8], errors [P, N]
    (the winner's) and winner_F [P, 3, 3] (unscaled)."""
    pts = np.asarray(pts, dtype=np.float64)
    P, N, _ = pts.shape
    H = int(hypotheses)
    valid = None if valid is None else np.asarray(valid).astype(bool)
    out = {'F': np.zeros((P, 3, 3)), 'mask': np.zeros((P, N), np.uint8), 'sample': np.full((P, 8), -1, np.int32),
           'median': np.full(P, np.inf), 'sigma': np.zeros(P), 'n_inliers': np.zeros(P, np.int64),
           'best': np.full(P, -1, np.int64), 'medians': np.full((P, H), np.inf),
           'samples': np.full((P, H, 8), -1, np.int32), 'errors': np.full((P, N), np.inf),
           'winner_F': np.zeros((P, 3, 3))}
    for p in range(P):
        ok = np.ones(N, dtype=bool) if valid is None else valid[p]
        n = int(ok.sum())
        usable = []
        for h in range(H):
            rows = draw(N, None if valid is None else ok, seed, p, h)
            if rows is not None:
                out['samples'][p, h] = rows
                usable.append(h)
        if not usable:
            continue
        Fh = solve_samples(pts[p][out['samples'][p, usable]], linalg)
        err = epipolar_errors(Fh, pts[p][ok])
        med = np.sort(err, axis=1)[:, n // 2]
        med = np.where(np.isfinite(Fh).all(axis=(1, 2)), med, np.inf)
        out['medians'][p, usable] = med
        if not (med < np.inf).any():
            continue
        k = int(np.argmin(med))                      # the first of equals: the lowest h
        hb, m = usable[k], med[k]
        small = 5.0 / (n - 8) if n > 8 else 0.0
        sigma = max(2.5 * 1.4826 * (1.0 + small) * np.sqrt(m), SIGMA_FLOOR)
        e = epipolar_errors(Fh[k], pts[p])
        mask = ok & (e <= sigma * sigma)
        out['median'][p], out['sigma'][p], out['best'][p] = m, sigma, hb
        out['sample'][p] = out['samples'][p, hb]
        out['errors'][p] = np.where(ok, e, np.inf)
        out['winner_F'][p] = Fh[k]
        F = Fh[k]
        if mask.sum() >= SAMPLE and do_refit:
            F = refit(pts[p][mask], linalg)
        F = scale_matrix(F) if mask.sum() >= SAMPLE else None
        if F is not None:
            out['F'][p], out['mask'][p], out['n_inliers'][p] = F, mask, int(mask.sum())
    return out


def residual_stats(F, pts, valid=None):
    """Per problem (mean, max) over the valid rows of |x_j^T F x_i| -> [P, 2]."""
    pts = np.asarray(pts, dtype=np.float64)
    out = np.zeros((pts.shape[0], 2))
    for p in range(pts.shape[0]):
        x = pts[p] if valid is None else pts[p][np.asarray(valid[p]).astype(bool)]
        if len(x) == 0:
            continue
        hi = np.concatenate([x[:, :2], np.ones((len(x), 1))], axis=1)
        hj = np.concatenate([x[:, 2:], np.ones((len(x), 1))], axis=1)
        r = np.abs(np.sum((hj @ F[p]) * hi, axis=1))
        out[p] = r.mean(), r.max()
    return out
