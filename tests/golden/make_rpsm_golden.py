"""Generate the RPSM fixtures tests/golden/rpsm_{a,b,c}.npz by importing the REFERENCE's
multiviews.pictorial (/root/reference/lib) in this container.  Run once, not on the GPU box:

    python tests/golden/make_rpsm_golden.py

The reference is imported as it is, with real scipy and the cv2 stand-in of make_golden.py (only
cv2.getAffineTransform).  Everything stored under ref_* is what the reference's own functions
returned (compute_grid, compute_unary_term, infer, get_loc_from_cube_idx, recursive_infer, rpsm,
HumanBody); infer's per-joint energies are read from its local table when it returns.  The
inputs follow the fixed recipe of tools/rpsm_synthetic.py (seeded RandomState, no reference code):

  cameras   four on a 4.5 m circle at 1.5 m height looking at (0, 0, 900); fx ~ 1145, fy ~ 1144,
            c ~ (512, 515), k = (-0.2, 0.25, -0.01), p = (-0.001, 0.002); fx / fy / cx / cy as
            1-element arrays
  pose      a random walk over the tree from a root near (+-300, +-300, 950), limb lengths
            uniform in the case's range, redrawn until every joint lies inside the level-1 box
  boxes     the joints' projected bounding square x 1.3; the level-1 box is larger than the
            pose, so in every view part of its grid projects outside the heatmap (printed)
  heatmaps  Gaussian (sigma 1.5 px) at the projected joints + N(0, 0.02) noise, float32
  pairwise  level 1: | norm(xyz[i] - xyz[j]) - L | < 0.4 L on the centred grid, L the pose's own
            limb lengths (also the recursion's limb_length), stored as packed bits

Cases: A  FIRST_NBINS 5, GRID_SIZE 600, limbs 160-260, 24x24, depth 3, 3 groups of 4 views
       B  FIRST_NBINS 8, GRID_SIZE 1000, limbs 150-300, 32x32, depth 4, 1 group
       C  A's first group seen by views 0 and 2 only (outputs only; inputs are A's)
all with RECUR_NBINS 2 and tolerance 150.
"""
import os
import sys
import types

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(os.path.dirname(HERE))
REF_LIB = '/root/reference/lib'


def _load_recipe():
    # by file path: this repository's lib/ must not shadow the reference's packages here
    import importlib.util
    spec = importlib.util.spec_from_file_location('rpsm_synthetic', os.path.join(REPO, 'tools', 'rpsm_synthetic.py'))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


recipe = _load_recipe()   # the input recipe; imports nothing of either lib until given functions
IMAGE = recipe.IMAGE


def _import_reference():
    m = types.ModuleType('cv2')

    def getAffineTransform(src, dst):
        a = np.zeros((6, 6))
        b = np.zeros(6)
        src = np.asarray(src, np.float64)
        dst = np.asarray(dst, np.float64)
        for i in range(3):
            a[2 * i, :3] = [src[i, 0], src[i, 1], 1]
            a[2 * i + 1, 3:] = [src[i, 0], src[i, 1], 1]
            b[2 * i:2 * i + 2] = dst[i]
        return np.linalg.solve(a, b).reshape(2, 3)

    m.getAffineTransform = getAffineTransform
    m.INTER_LINEAR = 1
    sys.modules['cv2'] = m
    if REF_LIB not in sys.path:
        sys.path.insert(0, REF_LIB)
    import multiviews.pictorial as pict
    import multiviews.cameras as cams
    import utils.transforms as tf
    from multiviews.body import HumanBody
    return pict, cams, tf, HumanBody


def level1_pairwise(body, limb_length, size, nbins):
    g1 = np.linspace(-size / 2, size / 2, nbins)
    gx, gy, gz = np.meshgrid(g1, g1, g1)
    xyz = np.stack([gx.reshape(-1), gy.reshape(-1), gz.reshape(-1)], axis=1)
    d = np.sqrt(((xyz[:, None, :] - xyz[None, :, :]) ** 2).sum(-1))
    return {e: (np.abs(d - L) < 0.4 * L).astype(np.int8) for e, L in limb_length.items()}


def pack(pairwise, edges):
    return np.stack([np.packbits(pairwise[e] != 0, axis=1, bitorder='little') for e in edges])


class _InferEnergies:
    """Reads the reference infer()'s states_of_all_joints when the function returns."""

    def __init__(self, pict):
        self.code = pict.infer.__code__
        self.energy = None

    def __call__(self, frame, event, arg):
        if event == 'return' and frame.f_code is self.code:
            st = frame.f_locals['states_of_all_joints']
            self.energy = np.stack([np.asarray(st[j]['Energy'], dtype=np.float64).reshape(-1) for j in range(len(st))])


def run_group(ref, cfg, cams, heatmaps, boxes, center, limb_length, pairwise):
    """The reference's rpsm, level by level, with every intermediate."""
    pict, _, _, HumanBody = ref
    body = HumanBody()
    ps = cfg.PICT_STRUCT
    grid = pict.compute_grid(ps.GRID_SIZE, center, ps.FIRST_NBINS)
    unary = pict.compute_unary_term(heatmaps, [grid], boxes, cams, cfg.NETWORK.IMAGE_SIZE)
    outside = []
    for cam, box in zip(cams, boxes):
        trans = ref[2].get_affine_transform(box['center'], box['scale'], 0, cfg.NETWORK.IMAGE_SIZE)
        uv = ref[2].affine_transform(ref[1].project_pose(grid, cam), trans) * heatmaps.shape[-1] / IMAGE
        outside.append(float(np.mean((uv < 0).any(1) | (uv > heatmaps.shape[-1] - 1).any(1))))
    print('   level-1 grid outside the heatmap per view:', ' '.join('%.0f%%' % (100 * o) for o in outside))
    assert max(outside) > 0.02
    probe = _InferEnergies(pict)
    sys.setprofile(probe)
    try:
        cube = pict.infer(unary, pairwise, body, cfg)
    finally:
        sys.setprofile(None)
    pose = pict.get_loc_from_cube_idx([grid], cube)
    levels = [pose]
    cur = ps.GRID_SIZE / ps.FIRST_NBINS
    for _ in range(ps.RECUR_DEPTH):
        pose = pict.recursive_infer(pose, cams, heatmaps, boxes, cfg.NETWORK.IMAGE_SIZE, cfg.NETWORK.HEATMAP_SIZE,
                                    body, limb_length, cur, ps.RECUR_NBINS, ps.LIMB_LENGTH_TOLERANCE, cfg)
        levels.append(pose)
        cur = cur / ps.RECUR_NBINS
    final = pict.rpsm(cams, heatmaps, boxes, center, limb_length, pairwise, cfg)
    assert np.array_equal(final, levels[-1])
    # no near-ties: the result must not move under 1e-12 relative perturbations of the heatmaps
    prng = np.random.RandomState(5)
    for _ in range(3):
        hp = heatmaps.astype(np.float64) * (1 + 1e-12 * prng.standard_normal(heatmaps.shape))
        assert np.array_equal(pict.rpsm(cams, hp, boxes, center, limb_length, pairwise, cfg), final), 'near-tie'
    return dict(grid=grid, unary=np.stack(unary), bins=np.array([b for _, b in cube], dtype=np.int32),
                energy=probe.energy, levels=np.stack(levels), final=final)


def make_group(ref, rng, cfg, limbs, hm):
    """The shared recipe (tools/rpsm_synthetic.py), evaluated with the reference's functions."""
    pict, rcams, tf, HumanBody = ref
    g = recipe.make_group(rng, cfg.PICT_STRUCT.GRID_SIZE, limbs, hm,
                          fns=(HumanBody, rcams.project_pose, tf.get_affine_transform, tf.affine_transform))
    return g['cams'], g['heatmaps'], g['boxes'], g['center'], g['limb_length'], g['pose']


def cams_arrays(groups):
    keys = ('R', 'T', 'fx', 'fy', 'cx', 'cy', 'k', 'p')
    return {'cam_' + k: np.stack([np.stack([np.asarray(c[k], dtype=np.float64) for c in cams]) for cams in groups])
            for k in keys}


def make_case(ref, name, seed, first_nbins, grid_size, limbs, hm, depth, ngroups):
    _, _, _, HumanBody = ref
    body = HumanBody()
    edges = [(n['idx'], c) for n in body.skeleton for c in n['children']]
    rng = np.random.RandomState(seed)
    cfg = recipe.make_config(first_nbins, grid_size, depth, hm)
    groups, outs = [], []
    for _ in range(ngroups):
        cams, heat, boxes, center, limb_length, pose = make_group(ref, rng, cfg, limbs, hm)
        pairwise = level1_pairwise(body, limb_length, grid_size, first_nbins)
        out = run_group(ref, cfg, cams, heat, boxes, center, limb_length, pairwise)
        err = np.linalg.norm(out['final'] - pose, axis=1)
        outside = float(np.mean(out['unary'] == 0))
        print('%s: recovered to %.1f mm (mean %.1f), %.0f%% negative heatmap values, %.1f%% zero unary, '
              '%.1f%% pairs allowed' % (name, err.max(), err.mean(), 100 * np.mean(heat < 0), 100 * outside,
                                        100 * np.mean([m.mean() for m in pairwise.values()])))
        groups.append(dict(cams=cams, heat=heat, boxes=boxes, center=center, limb_length=limb_length, pose=pose,
                           pairwise=pairwise))
        outs.append(out)
    data = dict(first_nbins=first_nbins, recur_nbins=2, recur_depth=depth, grid_size=float(grid_size),
                tolerance=150.0, image_size=np.array([IMAGE, IMAGE]), edges=np.array(edges, dtype=np.int32),
                heatmaps=np.stack([g['heat'] for g in groups]),
                box_center=np.stack([np.stack([b['center'] for b in g['boxes']]) for g in groups]),
                box_scale=np.stack([np.stack([b['scale'] for b in g['boxes']]) for g in groups]),
                grid_center=np.stack([g['center'] for g in groups]),
                limb_length=np.stack([[g['limb_length'][e] for e in edges] for g in groups]),
                pairwise_bits=np.stack([pack(g['pairwise'], edges) for g in groups]),
                true_pose=np.stack([g['pose'] for g in groups]),
                ref_grid=np.stack([o['grid'] for o in outs]), ref_unary=np.stack([o['unary'] for o in outs]),
                ref_bins=np.stack([o['bins'] for o in outs]), ref_energy=np.stack([o['energy'] for o in outs]),
                ref_levels=np.stack([o['levels'] for o in outs]), ref_final=np.stack([o['final'] for o in outs]),
                body_children=np.array([n['children'] + [-1] * (3 - len(n['children'])) for n in body.skeleton],
                                       dtype=np.int32),
                body_level_order=np.array([n['idx'] for n in body.skeleton_sorted_by_level], dtype=np.int32),
                body_parent=np.array([n.get('parent', -1) for n in body.skeleton], dtype=np.int32),
                body_root=body.root_idx, **cams_arrays([g['cams'] for g in groups]))
    np.savez_compressed(os.path.join(HERE, name + '.npz'), **data)
    return cfg, groups


def main():
    ref = _import_reference()
    cfg, groups = make_case(ref, 'rpsm_a', 11, 5, 600, (160, 260), 24, 3, 3)
    make_case(ref, 'rpsm_b', 12, 8, 1000, (150, 300), 32, 4, 1)
    # C: A's first group through views 0 and 2 only
    g, views = groups[0], [0, 2]
    out = run_group(ref, cfg, [g['cams'][v] for v in views], g['heat'][views], [g['boxes'][v] for v in views],
                    g['center'], g['limb_length'], g['pairwise'])
    err = np.linalg.norm(out['final'] - g['pose'], axis=1)
    print('rpsm_c: recovered to %.1f mm (mean %.1f)' % (err.max(), err.mean()))
    np.savez_compressed(os.path.join(HERE, 'rpsm_c.npz'), views=np.array(views), ref_unary=out['unary'],
                        ref_bins=out['bins'], ref_energy=out['energy'], ref_levels=out['levels'],
                        ref_final=out['final'])
    for n in ('rpsm_a', 'rpsm_b', 'rpsm_c'):
        print(n, os.path.getsize(os.path.join(HERE, n + '.npz')), 'bytes')


if __name__ == '__main__':
    main()
