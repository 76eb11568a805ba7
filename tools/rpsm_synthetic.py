"""Synthetic RPSM inputs -- the one recipe behind tests/golden/make_rpsm_golden.py (which runs it
with the reference's functions), tests/test_gpu_rpsm.py and tools/rpsm_micro.py -- and a plain
numpy restatement of the model.  Host only, not product code: the package never imports it.

Recipe: four cameras on a 4.5 m circle at 1.5 m height looking at (0, 0, 900) with radial and
tangential distortion, a random-walk pose over the MPII tree from a root near
(+-300, +-300, 950), per-view boxes = the projected joints' bounding square x 1.3, heatmaps =
Gaussian (sigma 1.5 px) at the projected joints + N(0, 0.02) noise (so ~45 % of the values
are negative, like network output).
"""
import types

import numpy as np

IMAGE = 256


def _lib():
    """(HumanBody, project_pose, get_affine_transform, affine_transform) of this repository's lib/,
    imported on first use: the golden generator passes the reference's instead."""
    from multiviews.body import HumanBody
    from multiviews.cameras import project_pose
    from utils.transforms import affine_transform, get_affine_transform
    return HumanBody, project_pose, get_affine_transform, affine_transform


def edges_of(body):
    return [(n['idx'], c) for n in body.skeleton for c in n['children']]


def make_cameras(rng):
    cams = []
    for v in range(4):
        th = 2 * np.pi * v / 4 + rng.uniform(-0.2, 0.2)
        T = np.array([4500 * np.cos(th), 4500 * np.sin(th), 1500.0])
        z = np.array([0.0, 0.0, 900.0]) - T
        z /= np.linalg.norm(z)
        right = np.cross(z, [0.0, 0.0, 1.0])
        right /= np.linalg.norm(right)
        cams.append({'R': np.stack([right, np.cross(z, right), z]), 'T': T.reshape(3, 1),
                     'fx': np.array([1145.0 + rng.uniform(-1, 1)]), 'fy': np.array([1144.0 + rng.uniform(-1, 1)]),
                     'cx': np.array([512.0 + rng.uniform(-3, 3)]), 'cy': np.array([515.0 + rng.uniform(-3, 3)]),
                     'k': np.array([[-0.2], [0.25], [-0.01]]), 'p': np.array([[-0.001], [0.002]])})
    return cams


def make_pose(rng, body, limbs, half):
    """Random walk from the root, redrawn until every joint is within `half` of it per axis."""
    for _ in range(200000):
        root = np.array([rng.choice([-300.0, 300.0]), rng.choice([-300.0, 300.0]), 950.0]) + rng.uniform(-20, 20, 3)
        pose = np.zeros((len(body.skeleton), 3))
        pose[body.root_idx] = root
        queue = [body.root_idx]
        while queue:
            n = queue.pop(0)
            for c in body.skeleton[n]['children']:
                d = rng.normal(size=3)
                pose[c] = pose[n] + d / np.linalg.norm(d) * rng.uniform(*limbs)
                queue.append(c)
        if np.abs(pose - root).max() < half:
            return pose
    raise RuntimeError('no pose fits the box')


def make_config(first_nbins, grid_size, depth, hm, recur_nbins=2, tolerance=150):
    ns = types.SimpleNamespace
    return ns(NETWORK=ns(IMAGE_SIZE=np.array([IMAGE, IMAGE]), HEATMAP_SIZE=np.array([hm, hm])),
              PICT_STRUCT=ns(FIRST_NBINS=first_nbins, RECUR_NBINS=recur_nbins, RECUR_DEPTH=depth,
                             GRID_SIZE=grid_size, LIMB_LENGTH_TOLERANCE=tolerance))


def make_group(rng, grid_size, limbs, hm, fns=None):
    """One 4-view group -> dict(cams, heatmaps [4, J, hm, hm] f32, boxes, center [3], limb_length, pose).
    fns: (HumanBody, project_pose, get_affine_transform, affine_transform), default this lib's."""
    HumanBody, project_pose, get_affine_transform, affine_transform = fns or _lib()
    body = HumanBody()
    cams = make_cameras(rng)
    pose = make_pose(rng, body, limbs, grid_size / 2 - 10)
    center = pose[body.root_idx] + rng.uniform(-8, 8, 3)
    limb_length = {(p, c): float(np.linalg.norm(pose[p] - pose[c])) for p, c in edges_of(body)}
    nj = len(body.skeleton)
    boxes, heat = [], np.zeros((4, nj, hm, hm), dtype=np.float32)
    yy, xx = np.mgrid[0:hm, 0:hm]
    for v, cam in enumerate(cams):
        xy = project_pose(pose, cam)
        lo, hi = xy.min(0), xy.max(0)
        side = float((hi - lo).max()) * 1.3
        boxes.append({'center': (lo + hi) / 2, 'scale': np.array([side / 200.0, side / 200.0])})
        trans = get_affine_transform(boxes[v]['center'], boxes[v]['scale'], 0, np.array([IMAGE, IMAGE]))
        uv = affine_transform(xy, trans) * hm / IMAGE
        for j in range(nj):
            g = np.exp(-((xx - uv[j, 0]) ** 2 + (yy - uv[j, 1]) ** 2) / (2 * 1.5 ** 2))
            heat[v, j] = (g + rng.normal(0, 0.02, (hm, hm))).astype(np.float32)
    return dict(cams=cams, heatmaps=heat, boxes=boxes, center=center, limb_length=limb_length, pose=pose)


# ------------------------------------------------------------ numpy restatement
def grid_numpy(size, center, n):
    g1 = np.linspace(-size / 2, size / 2, n)
    gx, gy, gz = np.meshgrid(g1 + center[0], g1 + center[1], g1 + center[2])
    return np.stack([gx.reshape(-1), gy.reshape(-1), gz.reshape(-1)], axis=1)


def unary_numpy(heatmaps, grids, boxes, cams, image_size):
    """[V, J, h, h] f32, 1 or J grids [N, 3] -> [J, N]: bilinear samples of the projected grid, 0 outside."""
    _, project_pose, get_affine_transform, affine_transform = _lib()
    nv, nj, h, _ = heatmaps.shape
    out = np.zeros((nj, grids[0].shape[0]))
    for j in range(nj):
        grid = grids[0 if len(grids) == 1 else j]
        for v in range(nv):
            trans = get_affine_transform(boxes[v]['center'], boxes[v]['scale'], 0, image_size)
            xy = affine_transform(project_pose(grid, cams[v]), trans) * np.array([h, h]) / np.asarray(image_size)
            inside = (xy >= 0).all(1) & (xy <= h - 1).all(1)
            i = np.clip(np.floor(xy), 0, h - 2).astype(np.int64)
            t = xy - i
            m = heatmaps[v, j].astype(np.float64)
            val = (m[i[:, 1], i[:, 0]] * ((1 - t[:, 0]) * (1 - t[:, 1])) + m[i[:, 1] + 1, i[:, 0]] * ((1 - t[:, 0]) * t[:, 1])
                   + m[i[:, 1], i[:, 0] + 1] * (t[:, 0] * (1 - t[:, 1])) + m[i[:, 1] + 1, i[:, 0] + 1] * (t[:, 0] * t[:, 1]))
            out[j] = out[j] + np.where(inside, val, 0.0)
    return out


def pairwise_numpy(grid_p, grid_c, limb, thr, strict):
    d = np.sqrt(((grid_p[:, None, :] - grid_c[None, :, :]) ** 2).sum(-1))
    off = np.abs(d - limb)
    return off < thr if strict else off <= thr


def infer_numpy(unary, pairwise, body, chunk=512):
    """Max-product, leaves first: v = P * e (a disallowed pair is a zero), first argmax; -> bins [J]."""
    energy, state = {}, {}
    for node in body.skeleton_sorted_by_level:
        p = node['idx']
        e = np.array(unary[p], dtype=np.float64)
        for c in node['children']:
            P, ec = pairwise[(p, c)], energy[c]
            m, s = np.empty(len(e)), np.empty(len(e), dtype=np.int64)
            for i in range(0, len(e), chunk):
                v = P[i:i + chunk] * ec
                s[i:i + chunk] = np.argmax(v, axis=1)
                m[i:i + chunk] = np.max(v, axis=1)
            e = e * m
            state[c] = s
        energy[p] = e
    bins = np.zeros(len(body.skeleton), dtype=np.int64)
    bins[body.root_idx] = np.argmax(energy[body.root_idx])
    for node in body.skeleton_sorted_by_level[::-1]:
        for c in node['children']:
            bins[c] = state[c][bins[node['idx']]]
    return bins


def rpsm_numpy(group, pairwise, config):
    """The whole model for one group on the host -> pose [J, 3]."""
    body = _lib()[0]()
    ps, size = config.PICT_STRUCT, config.NETWORK.IMAGE_SIZE
    grid = grid_numpy(ps.GRID_SIZE, group['center'], ps.FIRST_NBINS)
    unary = unary_numpy(group['heatmaps'], [grid], group['boxes'], group['cams'], size)
    pose = grid[infer_numpy(unary, pairwise, body)]
    cur = ps.GRID_SIZE / ps.FIRST_NBINS
    for _ in range(ps.RECUR_DEPTH):
        grids = [grid_numpy(cur, p, ps.RECUR_NBINS) for p in pose]
        unary = unary_numpy(group['heatmaps'], grids, group['boxes'], group['cams'], size)
        pw = {(p, c): pairwise_numpy(grids[p], grids[c], group['limb_length'][(p, c)], ps.LIMB_LENGTH_TOLERANCE, False)
              for p, c in edges_of(body)}
        bins = infer_numpy(unary, pw, body)
        pose = np.stack([grids[j][bins[j]] for j in range(len(pose))])
        cur = cur / ps.RECUR_NBINS
    return pose
