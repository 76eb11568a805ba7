"""Plain-torch fp64 restatement of the differentiable triangulation and the reprojection loss, written from the
formulas of DESIGN.md section 4 (f14); torch autograd supplies its gradients.  Test infrastructure only.

  undistort    the OpenCV fixed point, five iterations, the identity for a camera without coefficients
  rows         A [G, J, 2 V, 4]: the rows w (u m2 - m0), w (v m2 - m1) of every view, zero for a view that is off
  point        the smallest right singular vector of A, dehomogenised, by two routes:
                 'svd'   torch.linalg.svd(A)        -- the reference route (values and, by autograd, gradients)
                 'eigh'  torch.linalg.eigh(A^T A)   -- the second opinion: its disagreement with 'svd' on the same
                                                      inputs is the yardstick of the GPU tests
  project      [R | t] = K^-1 M, plumb-bob distortion, back through K
  loss         sum omega ||project(X) - xy|| / (G V J), omega forced to 0 for a view that is off or a joint seen in
               fewer than two views; detach_point cuts the path through X

Tensors are group-major: M [G, V, 3, 4], intr [G, V, 9], xy [G, V, J, 2], vis / w / omega [G, V, J]."""
import numpy as np
import torch

from multiviews.triangulate import camera_tables
from posu import synthetic as syn


def undistort(intr, xy):
    """intr [G, V, 9], xy [G, V, J, 2] -> the undistorted pixels, as the function is computed."""
    c = intr[:, :, None, :]
    fx, fy, cx, cy, k1, k2, p1, p2, k3 = [c[..., i] for i in range(9)]
    xd, yd = (xy[..., 0] - cx) / fx, (xy[..., 1] - cy) / fy
    x, y = xd, yd
    for _ in range(5):
        r2 = x * x + y * y
        icdist = 1.0 / (1.0 + ((k3 * r2 + k2) * r2 + k1) * r2)
        dx = 2.0 * p1 * x * y + p2 * (r2 + 2.0 * x * x)
        dy = p1 * (r2 + 2.0 * y * y) + 2.0 * p2 * x * y
        x, y = (xd - dx) * icdist, (yd - dy) * icdist
    out = torch.stack([x * fx + cx, y * fy + cy], dim=-1)
    plain = (intr[..., 4:].abs().sum(dim=-1) == 0)[:, :, None, None]
    return torch.where(plain, xy, out)


def rows(M, und, on, w=None):
    """-> A [G, J, 2 V, 4]; on [G, V, J] bool."""
    m0, m1, m2 = M[:, :, None, 0, :], M[:, :, None, 1, :], M[:, :, None, 2, :]     # [G, V, 1, 4]
    a0 = und[..., 0:1] * m2 - m0
    a1 = und[..., 1:2] * m2 - m1
    A = torch.stack([a0, a1], dim=2)                                               # [G, V, 2, J, 4]
    scale = on.to(A.dtype) if w is None else on.to(A.dtype) * w
    A = A * scale[:, :, None, :, None]
    g, v, _, j, _ = A.shape
    return A.permute(0, 3, 1, 2, 4).reshape(g, j, 2 * v, 4)


def smallest_vector(A, route):
    if route == 'svd':
        return torch.linalg.svd(A, full_matrices=False).Vh[..., -1, :]
    if route == 'eigh':
        return torch.linalg.eigh(A.transpose(-1, -2) @ A).eigenvectors[..., :, 0]
    raise ValueError(route)


def point(A, route='svd'):
    h = smallest_vector(A, route)
    return h[..., :3] / h[..., 3:4]


def project(M, intr, X):
    """X [G, J, 3] -> [G, V, J, 2]."""
    Xh = torch.cat([X, torch.ones_like(X[..., :1])], dim=-1)
    P = torch.einsum('gvrc,gjc->gvjr', M, Xh)
    c = intr[:, :, None, :]
    fx, fy, cx, cy, k1, k2, p1, p2, k3 = [c[..., i] for i in range(9)]
    zc = P[..., 2]
    x = (P[..., 0] - cx * zc) / fx / zc
    y = (P[..., 1] - cy * zc) / fy / zc
    r2 = x * x + y * y
    radial = 1.0 + ((k3 * r2 + k2) * r2 + k1) * r2
    xd = x * radial + 2.0 * p1 * x * y + p2 * (r2 + 2.0 * x * x)
    yd = y * radial + p1 * (r2 + 2.0 * y * y) + 2.0 * p2 * x * y
    return torch.stack([fx * xd + cx, fy * yd + cy], dim=-1)


def _on(xy, vis):
    return torch.ones(xy.shape[:3], dtype=torch.bool, device=xy.device) if vis is None else vis.bool()


def triangulate(M, intr, xy, vis=None, w=None, undistort_points=True, route='svd'):
    """-> X [G, J, 3]; (0, 0, 0) for a joint seen in fewer than two views."""
    on = _on(xy, vis)
    solved = on.sum(dim=1) >= 2                                                    # [G, J]
    und = undistort(intr, xy) if undistort_points else xy
    A = rows(M, und, on, w)
    # a joint that is not solved gets a harmless full-rank system, so that no NaN reaches the gradients
    A = torch.where(solved[:, :, None, None], A, rows(M, und.detach(), torch.ones_like(on), None))
    return torch.where(solved[:, :, None], point(A, route), torch.zeros((), dtype=A.dtype))


def residuals(M, intr, xy, X, vis=None):
    """e [G, V, J] = ||project(X) - xy||, 0 for a joint that was not solved."""
    solved = (_on(xy, vis).sum(dim=1) >= 2)[:, None, :]
    d = project(M, intr, torch.where(solved[:, 0, :, None], X, torch.ones((), dtype=X.dtype))) - xy
    d = torch.where(solved[..., None], d, torch.ones((), dtype=X.dtype))
    return torch.where(solved, d.norm(dim=-1), torch.zeros((), dtype=X.dtype))


def loss(M, intr, xy, vis=None, w=None, omega=None, undistort_points=True, detach_point=False, route='svd'):
    """-> (loss, X, e)."""
    on = _on(xy, vis)
    X = triangulate(M, intr, xy, vis, w, undistort_points, route)
    Xl = X.detach() if detach_point else X
    e = residuals(M, intr, xy, Xl, vis)
    om = (on & (on.sum(dim=1) >= 2)[:, None, :]).to(xy.dtype)
    if omega is not None:
        om = om * omega
    g, v, j = on.shape
    return (om * e).sum() / (g * v * j), X, e


def closed_form_gA(A, gX):
    """The backward of `point` in A, as the kernel computes it: with B = A^T A = sum lam_i q_i q_i^T, h = q_min,
    gh = (gX / h3, -(gX . X) / h3), z = sum_{i != min} q_i (q_i . gh) / (lam_min - lam_i),
    gA = (A z) h^T + (A h) z^T."""
    lam, Q = torch.linalg.eigh(A.transpose(-1, -2) @ A)
    h = Q[..., :, 0]
    X = h[..., :3] / h[..., 3:4]
    gh = torch.cat([gX / h[..., 3:4], -(gX * X).sum(dim=-1, keepdim=True) / h[..., 3:4]], dim=-1)
    coef = (Q[..., :, 1:] * gh[..., :, None]).sum(dim=-2) / (lam[..., 0:1] - lam[..., 1:])
    z = (Q[..., :, 1:] * coef[..., None, :]).sum(dim=-1)
    Az, Ah = (A @ z[..., None])[..., 0], (A @ h[..., None])[..., 0]
    return Az[..., :, None] * h[..., None, :] + Ah[..., :, None] * z[..., None, :]


# ------------------------------------------------------------------ inputs
def case(G=3, V=4, J=5, distortion=True, seed=0, noise=2.0, weights=True):
    """Synthetic rigs (posu.synthetic.group_cameras, the first V cameras of each), synthetic_poses3d projected
    into them plus seeded N(0, noise px): lam_min > 0 and no residual is exactly zero when noise > 0.
    -> dict of float64 torch tensors M, intr, xy, w (uniform in [0.3, 1]), omega (uniform in [0.5, 1.5]), and
    the camera dicts and poses they came from."""
    cams = syn.group_cameras(G, distortion)
    M, intr = camera_tables(cams, 4, no_distortion=not distortion)
    M, intr = torch.from_numpy(M[:, :V].copy()), torch.from_numpy(intr[:, :V].copy())
    X = torch.from_numpy(syn.synthetic_poses3d(G, J, seed=seed))
    r = np.random.default_rng([seed, G, V, J])
    xy = project(M, intr, X) + torch.from_numpy(r.normal(0.0, 1.0, size=(G, V, J, 2))) * noise
    out = {'M': M, 'intr': intr, 'xy': xy, 'cams': cams, 'poses': X,
           'w': torch.from_numpy(r.uniform(0.3, 1.0, size=(G, V, J))) if weights else None,
           'omega': torch.from_numpy(r.uniform(0.5, 1.5, size=(G, V, J)))}
    return out


def reference(c, vis=None, w=None, omega=None, undistort_points=True, detach_point=False, route='svd', gX=None):
    """Values and autograd gradients of one case by `route`: X, gxy / gw of sum(X * gX) (the triangulation's
    backward), and the loss with its e, gxy and gw.  w / omega: tensors or None."""
    out = {}
    xy = c['xy'].clone().requires_grad_(True)
    ww = None if w is None else w.clone().requires_grad_(True)
    X = triangulate(c['M'], c['intr'], xy, vis, ww, undistort_points, route)
    out['X'] = X.detach()
    if gX is not None:
        g = torch.autograd.grad((X * gX).sum(), [xy] + ([ww] if ww is not None else []))
        out['tri_gxy'] = g[0]
        out['tri_gw'] = g[1] if ww is not None else None
    xy = c['xy'].clone().requires_grad_(True)
    ww = None if w is None else w.clone().requires_grad_(True)
    val, _, e = loss(c['M'], c['intr'], xy, vis, ww, omega, undistort_points, detach_point, route)
    out['loss'], out['e'] = val.detach(), e.detach()
    g = torch.autograd.grad(val, [xy] + ([ww] if ww is not None else []), allow_unused=True)
    out['gxy'] = g[0]
    out['gw'] = (torch.zeros_like(ww) if g[1] is None else g[1]) if ww is not None else None
    return out
