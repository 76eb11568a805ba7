"""RPSM on the GPU (csrc/rpsm.hip behind multiviews.pictorial) against the reference's recorded
results (tests/golden/rpsm_*.npz, made by make_rpsm_golden.py) and against numpy restatements
written out here.

Gates.  The unary term is ~30 fp64 operations on pixel coordinates of order 1e3 feeding a heatmap
slope <= 1 per pixel: a few 1e-12, gated at 1e-10.  Everything after it is products, comparisons
and look-ups of identical inputs, so bins are exact and energies bit-identical -- up to the sign
of a zero: IEEE comparison does not order -0.0 and +0.0 (the reference's tie-break treats them as
equal) and numpy's SIMD max returns either, so energies are compared bit for bit after x + 0.0,
which maps both zeros to +0.0 and changes nothing else.  Poses are grid coordinates
centre + offset of the same bins: 1e-9 mm per level, 1e-6 mm end to end.
"""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'tools'))
import rpsm_synthetic as rs  # noqa: E402  -- the input recipe and numpy restatements (not product code)

pytestmark = pytest.mark.gpu

CAM_KEYS = ('R', 'T', 'fx', 'fy', 'cx', 'cy', 'k', 'p')


def _bits_equal(a, b):
    a, b = np.asarray(a, dtype=np.float64) + 0.0, np.asarray(b, dtype=np.float64) + 0.0
    return a.shape == b.shape and np.array_equal(a.view(np.int64), b.view(np.int64))


class Case:
    """One golden file as the reference's call arguments."""

    def __init__(self, g, views=None):
        self.g = g
        self.views = list(range(g['heatmaps'].shape[1])) if views is None else list(views)
        self.edges = [tuple(e) for e in g['edges'].tolist()]
        self.nbins = int(g['first_nbins'])
        self.N = self.nbins ** 3
        self.G = g['heatmaps'].shape[0]
        self.config = rs.make_config(self.nbins, float(g['grid_size']), int(g['recur_depth']), g['heatmaps'].shape[-1],
                                  recur_nbins=int(g['recur_nbins']), tolerance=float(g['tolerance']))

    def cams(self, gi):
        return [{k: self.g['cam_' + k][gi, v] for k in CAM_KEYS} for v in self.views]

    def boxes(self, gi):
        return [{'center': self.g['box_center'][gi, v], 'scale': self.g['box_scale'][gi, v]} for v in self.views]

    def heatmaps(self, gi):
        return self.g['heatmaps'][gi][self.views]

    def limbs(self, gi):
        return {e: float(self.g['limb_length'][gi, i]) for i, e in enumerate(self.edges)}

    def pairwise(self, gi):
        bits = np.unpackbits(self.g['pairwise_bits'][gi], axis=-1, bitorder='little')[:, :, :self.N]
        return {e: bits[i] for i, e in enumerate(self.edges)}


@pytest.fixture(scope='module')
def cases(golden, cuda):
    a, b, c = golden('rpsm_a.npz'), golden('rpsm_b.npz'), golden('rpsm_c.npz')
    return {'a': Case(a), 'b': Case(b), 'c': (Case(a, views=c['views']), c)}


# ------------------------------------------------------------------ 1. unary
@pytest.mark.parametrize('name', ['a', 'b'])
def test_unary_level1_matches_the_reference(cases, name):
    from multiviews.pictorial import compute_unary_term
    case = cases[name]
    for gi in range(case.G):
        ref = case.g['ref_unary'][gi]
        got = np.stack(compute_unary_term(case.heatmaps(gi), [case.g['ref_grid'][gi]], case.boxes(gi), case.cams(gi),
                                          case.config.NETWORK.IMAGE_SIZE))
        err = float(np.abs(got - ref).max())
        print('unary %s[%d]: max abs err %.3e, %d exact zeros' % (name, gi, err, int((ref == 0).sum())))
        assert err <= 1e-10
        assert np.array_equal(got == 0, ref == 0)


def test_unary_per_joint_grids_and_two_views(cases):
    """The recursion's form (a grid per joint) and V = 2, against the numpy restatement."""
    from multiviews.pictorial import compute_grid, compute_unary_term
    case, c = cases['c']
    grids = [compute_grid(60.0, p, 2) for p in c['ref_levels'][0]]
    size = case.config.NETWORK.IMAGE_SIZE
    got = np.stack(compute_unary_term(case.heatmaps(0), grids, case.boxes(0), case.cams(0), size))
    ref = rs.unary_numpy(case.heatmaps(0), grids, case.boxes(0), case.cams(0), size)
    assert got.shape == (16, 8) and float(np.abs(got - ref).max()) <= 1e-10
    lvl1 = np.stack(compute_unary_term(case.heatmaps(0), [case.g['ref_grid'][0]], case.boxes(0), case.cams(0), size))
    assert float(np.abs(lvl1 - c['ref_unary']).max()) <= 1e-10 and np.array_equal(lvl1 == 0, c['ref_unary'] == 0)


# ------------------------------------------------- 2. one level of inference
@pytest.mark.parametrize('name', ['a', 'b'])
def test_infer_from_the_reference_unary_is_exact(cases, cuda, name):
    from multiviews.body import HumanBody
    from multiviews.pictorial import infer, pack_pairwise, _tree
    from posu import ops
    case, body = cases[name], HumanBody()
    for gi in range(case.G):
        unary, ref_bins = case.g['ref_unary'][gi], case.g['ref_bins'][gi]
        cube = infer(list(unary), case.pairwise(gi), body, case.config)
        assert [j for j, _ in cube] == list(range(16))
        assert [b for _, b in cube] == ref_bins.tolist()
        packed = pack_pairwise(case.pairwise(gi))
        bins, pose, energy, _, _ = ops.rpsm_infer(torch.from_numpy(unary[None]).to(cuda), _tree(body),
                                                  mask=packed.mask(cuda),
                                                  pose_grid=torch.from_numpy(case.g['ref_grid'][gi][None, None]).to(cuda))
        assert bins[0].cpu().tolist() == ref_bins.tolist()
        assert _bits_equal(energy[0, body.root_idx].cpu().numpy(), case.g['ref_energy'][gi, body.root_idx])
        assert _bits_equal(energy[0].cpu().numpy(), case.g['ref_energy'][gi])
        assert np.array_equal(pose[0].cpu().numpy(), case.g['ref_levels'][gi, 0])


# ------------------------------------------------------------ 3. semantics
def _maxprod_numpy(unary, pairwise, children, order, chunk=512):
    """infer written out: leaves first, v = P * e (a disallowed pair is a zero, not -inf), first
    argmax, E = ((u * m1) * m2) ... in children order; then the root's first argmax and the states
    walked down.  `order`: deepest first, the root last.  Parent rows in chunks to bound memory."""
    energy, maxv, state = {}, {}, {}
    for p in order:
        e = np.array(unary[p], dtype=np.float64)
        for c in children[p]:
            state[c], maxv[c] = np.empty(len(e), dtype=np.int64), np.empty(len(e))
            for i in range(0, len(e), chunk):
                v = pairwise[(p, c)][i:i + chunk] * energy[c][None, :]
                state[c][i:i + chunk], maxv[c][i:i + chunk] = np.argmax(v, axis=1), np.max(v, axis=1)
            e = e * maxv[c]
        energy[p] = e
    root = order[-1]
    bins = {root: int(np.argmax(energy[root]))}
    for p in order[::-1]:
        for c in children[p]:
            bins[c] = int(state[c][bins[p]])
    return energy, maxv, state, bins


def _body_infer_numpy(unary, pairwise, body):
    order = [n['idx'] for n in body.skeleton_sorted_by_level]
    assert order[-1] == body.root_idx
    bins = _maxprod_numpy(unary, pairwise, {n['idx']: n['children'] for n in body.skeleton}, order)[3]
    return np.array([bins[j] for j in range(len(order))])


def test_max_product_semantics_on_a_hand_built_chain(cuda):
    """J = 3 chain 0 -> 1 -> 2, N = 40 (two mask words, the second partial): parent rows with no
    allowed child, rows whose allowed children are all negative, rows where every pair is allowed and
    negative, +-0.0 mixed into the energies, and duplicate maxima (first index must win)."""
    from posu import ops
    n = 40
    rng = np.random.RandomState(7)
    u = rng.uniform(-1, 1, (3, n))
    u[2, [3, 17, 33]] = 0.75            # duplicate maxima in the leaf
    u[2, [5, 36]] = 0.0, -0.0           # signed zeros
    u[2, 20:30] = -np.abs(u[2, 20:30])
    u[1, [4, 9]] = u[1, 4]
    u[0, [11, 30]] = 50.0               # with P01[11] == P01[30] below: a duplicate maximum at the root
    P12 = (rng.rand(n, n) < 0.3).astype(np.int8)
    P12[0] = 0                          # no allowed child
    P12[1] = 0
    P12[1, 20:30] = 1                   # only negative children allowed -> a disallowed zero wins
    P12[2] = 1
    P12[3] = 0
    P12[3, [3, 17, 33]] = 1             # duplicate positive maxima
    P12[6] = 0
    P12[6, [5, 36]] = 1                 # only signed zeros allowed
    P01 = (rng.rand(n, n) < 0.3).astype(np.int8)
    P01[7] = 0
    P01[8] = 1
    P01[11] = P01[30]                   # identical rows under identical unaries: a root tie
    uneg = u.copy()
    uneg[2] = -np.abs(u[2]) - 0.1       # every leaf energy negative
    children, order = {0: [1], 1: [2], 2: []}, [2, 1, 0]
    tree = ops.RpsmTree([-1, 0, 1], [[1], [2], []])
    for unary in (u, uneg):
        pw = {(0, 1): P01, (1, 2): P12}
        energy, maxv, state, bins = _maxprod_numpy(unary, pw, children, order)
        bits = np.zeros((2, 2, n), dtype=np.uint32)       # [edge][word j / 32][parent bin i]
        for e, P in enumerate((P01, P12)):
            by = np.zeros((n, 8), dtype=np.uint8)
            by[:, :5] = np.packbits(P != 0, axis=1, bitorder='little')
            bits[e] = by.view('<u4').T
        got_bins, _, got_e, got_m, got_s = ops.rpsm_infer(torch.from_numpy(unary[None]).to(cuda), tree,
                                                          mask=torch.from_numpy(bits.view(np.int32)).to(cuda))
        for c in (1, 2):
            assert np.array_equal(got_s[0, c].cpu().numpy(), state[c]), c
            assert _bits_equal(got_m[0, c].cpu().numpy(), maxv[c]), c
        for j in range(3):
            assert _bits_equal(got_e[0, j].cpu().numpy(), energy[j]), j
        assert got_bins[0].cpu().tolist() == [bins[0], bins[1], bins[2]]
    # what the rows were built to show (on the mixed-sign unary)
    energy, maxv, state, bins = _maxprod_numpy(u, {(0, 1): P01, (1, 2): P12}, children, order)
    assert maxv[2][0] == 0 and state[2][0] == 0          # nothing allowed: zero at the first index
    assert maxv[2][1] == 0 and state[2][1] == 0          # allowed ones negative: the first disallowed zero wins
    assert state[2][3] == 3                              # duplicate maxima: first index
    assert state[2][6] == 0 and maxv[2][6] == 0          # signed zeros never beat the first zero
    assert energy[0][11] == energy[0][30] == energy[0].max() and bins[0] == 11   # root tie: first index


# ----------------------------------------------------------- 4. recursion
@pytest.mark.parametrize('name', ['a', 'b'])
def test_recursion_levels_follow_the_reference(cases, name):
    from multiviews.body import HumanBody
    from multiviews.pictorial import recursive_infer
    case, body = cases[name], HumanBody()
    ps = case.config.PICT_STRUCT
    for gi in range(case.G):
        pose, cur = case.g['ref_levels'][gi, 0], ps.GRID_SIZE / ps.FIRST_NBINS
        for level in range(1, ps.RECUR_DEPTH + 1):
            pose = recursive_infer(pose, case.cams(gi), case.heatmaps(gi), case.boxes(gi), case.config.NETWORK.IMAGE_SIZE,
                                   case.config.NETWORK.HEATMAP_SIZE, body, case.limbs(gi), cur, ps.RECUR_NBINS,
                                   ps.LIMB_LENGTH_TOLERANCE, case.config)
            err = float(np.abs(pose - case.g['ref_levels'][gi, level]).max())
            print('recursion %s[%d] level %d: %.3e mm' % (name, gi, level, err))
            assert err <= 1e-9
            cur = cur / ps.RECUR_NBINS


def test_on_the_fly_constraint_is_the_reference_rule(cases):
    """compute_pairwise_constrain (<= tolerance) from per-joint grids against numpy."""
    from multiviews.body import HumanBody
    from multiviews.pictorial import compute_grid, compute_pairwise_constrain
    case, body = cases['a'], HumanBody()
    grids = [compute_grid(120.0, p, 2) for p in case.g['ref_levels'][0, 0]]
    got = compute_pairwise_constrain(body.skeleton, case.limbs(0), grids, 150)
    assert list(got) == body.edges()
    allowed = 0
    for (p, c), m in got.items():
        ref = rs.pairwise_numpy(grids[p], grids[c], case.limbs(0)[(p, c)], 150, strict=False)
        assert m.shape == (8, 8) and np.array_equal(m != 0, ref)
        allowed += int(ref.sum())
    assert 0 < allowed < 15 * 64


# ---------------------------------------------------------- 5. end to end
def test_rpsm_end_to_end(cases, cuda):
    from multiviews.pictorial import pack_pairwise, rpsm, rpsm_batch
    for name in ('a', 'b'):
        case = cases[name]
        for gi in range(case.G):
            pose = rpsm(case.cams(gi), case.heatmaps(gi), case.boxes(gi), case.g['grid_center'][gi], case.limbs(gi),
                        case.pairwise(gi), case.config)
            assert isinstance(pose, np.ndarray) and pose.shape == (16, 3) and pose.dtype == np.float64
            err = float(np.abs(pose - case.g['ref_final'][gi]).max())
            print('rpsm %s[%d]: %.3e mm' % (name, gi, err))
            assert err <= 1e-6
    case, c = cases['c']
    pose = rpsm(case.cams(0), case.heatmaps(0), case.boxes(0), case.g['grid_center'][0], case.limbs(0),
                case.pairwise(0), case.config)
    assert float(np.abs(pose - c['ref_final']).max()) <= 1e-6
    # a dict and a PackedPairwise give the same result; per-level poses
    packed = pack_pairwise(case.pairwise(0))
    final, levels = rpsm_batch(case.cams(0), case.heatmaps(0), case.boxes(0), case.g['grid_center'][:1], case.limbs(0),
                               packed, case.config, return_levels=True)
    assert np.array_equal(final[0], pose) and np.array_equal(levels[-1], final)
    assert float(np.abs(levels[:, 0] - c['ref_levels']).max()) <= 1e-9


def test_rpsm_batch_equals_single_calls_and_keeps_cuda_tensors(cases, cuda):
    """Every group refines with its OWN limb lengths (run/test/test_rpsm.py computes them per group); the
    level-1 constraint is the one table a batch shares (group 0's here), so groups 1 and 2 differ from
    their goldens at level 1 and the batch is pinned to the single calls, group 0 also to its golden."""
    from multiviews.pictorial import pack_pairwise, rpsm, rpsm_batch
    case = cases['a']
    packed = pack_pairwise(case.pairwise(0))
    limbs = [case.limbs(gi) for gi in range(case.G)]
    assert limbs[0] != limbs[1] != limbs[2]
    singles = np.stack([rpsm(case.cams(gi), case.heatmaps(gi), case.boxes(gi), case.g['grid_center'][gi], limbs[gi],
                             packed, case.config) for gi in range(case.G)])
    assert float(np.abs(singles[0] - case.g['ref_final'][0]).max()) <= 1e-6
    cams = [c for gi in range(case.G) for c in case.cams(gi)]
    boxes = [b for gi in range(case.G) for b in case.boxes(gi)]
    hm = case.g['heatmaps'].reshape(case.G * 4, 16, 24, 24)
    batch = rpsm_batch(cams, hm, boxes, case.g['grid_center'], limbs, packed, case.config)
    assert batch.shape == (3, 16, 3) and batch.dtype == np.float64
    assert np.array_equal(batch, singles)
    # the same as a [G, J] array by child joint; one shared dict is a different (broadcast) table
    from multiviews.pictorial import _limb_rows, _tree
    from multiviews.body import HumanBody
    table = _limb_rows(limbs, _tree(HumanBody()), case.G)
    assert np.array_equal(rpsm_batch(cams, hm, boxes, case.g['grid_center'], table, packed, case.config), batch)
    shared = rpsm_batch(cams, hm, boxes, case.g['grid_center'], limbs[0], packed, case.config)
    assert np.array_equal(shared[0], batch[0])
    assert np.array_equal(shared[1], rpsm(case.cams(1), case.heatmaps(1), case.boxes(1), case.g['grid_center'][1],
                                          limbs[0], packed, case.config))
    on_dev = rpsm_batch(cams, torch.from_numpy(hm).to(cuda), boxes, case.g['grid_center'], limbs, packed, case.config)
    assert isinstance(on_dev, torch.Tensor) and on_dev.is_cuda and on_dev.dtype == torch.float64
    assert np.array_equal(on_dev.cpu().numpy(), batch)
    with pytest.raises(ValueError, match='square'):
        rpsm_batch(cams, np.zeros((12, 16, 24, 32), dtype=np.float32), boxes, case.g['grid_center'], limbs, packed,
                   case.config)
    with pytest.raises(ValueError):
        rpsm_batch(cams, hm, boxes, case.g['grid_center'], limbs[:2], packed, case.config)


def test_batched_refinement_with_per_group_limbs_follows_the_reference(cases, cuda):
    """All three groups of A refined in ONE batched call per level, each with its own limb lengths, from the
    golden's pose of the level before: every group's pose equals the golden's next level (1e-9 mm)."""
    from multiviews.body import HumanBody
    from multiviews.pictorial import _affines, _camera_rows, _dev_f64, _limb_rows, _tree
    from posu import ops
    case, tree = cases['a'], _tree(HumanBody())
    ps, size = case.config.PICT_STRUCT, case.config.NETWORK.IMAGE_SIZE
    hm = torch.from_numpy(case.g['heatmaps']).to(cuda)
    rows = _dev_f64(_camera_rows([c for gi in range(case.G) for c in case.cams(gi)]), cuda).reshape(case.G, 4, 20)
    aff = _dev_f64(_affines([b for gi in range(case.G) for b in case.boxes(gi)], size), cuda).reshape(case.G, 4, 2, 3)
    limb = _dev_f64(_limb_rows([case.limbs(gi) for gi in range(case.G)], tree, case.G), cuda)
    cur = ps.GRID_SIZE / ps.FIRST_NBINS
    for level in range(1, ps.RECUR_DEPTH + 1):
        grids = ops.rpsm_grid(_dev_f64(case.g['ref_levels'][:, level - 1], cuda), cur, ps.RECUR_NBINS)
        unary = ops.rpsm_unary(hm, rows, aff, grids, size)
        pose = ops.rpsm_infer(unary, tree, grid=grids, limb=limb, tolerance=float(ps.LIMB_LENGTH_TOLERANCE))[1]
        err = np.abs(pose.cpu().numpy() - case.g['ref_levels'][:, level]).max(axis=(1, 2))
        print('batched refinement level %d: per-group err %s mm' % (level, err))
        assert float(err.max()) <= 1e-9
        cur = cur / ps.RECUR_NBINS
    # the limbs matter: group 1 refined with group 0's lengths allows other pairs
    from multiviews.pictorial import compute_grid
    g1 = [compute_grid(120.0, p, 2) for p in case.g['ref_levels'][1, 0]]
    differs = any(not np.array_equal(rs.pairwise_numpy(g1[p], g1[c], case.limbs(0)[(p, c)], 150, False),
                                     rs.pairwise_numpy(g1[p], g1[c], case.limbs(1)[(p, c)], 150, False))
                  for p, c in case.edges)
    assert differs


# --------------------------------------------------- 6. the mask builder
@pytest.mark.parametrize('name', ['a', 'b'])
def test_pairwise_constraint_builder_is_bit_identical_to_numpy(cases, name):
    from multiviews.pictorial import compute_pairwise_constraint
    case = cases[name]
    size, limbs = float(case.g['grid_size']), case.limbs(0)
    packed = compute_pairwise_constraint(size, limbs, case.nbins)
    g1 = np.linspace(-size / 2, size / 2, case.nbins)
    gx, gy, gz = np.meshgrid(g1, g1, g1)
    xyz = np.stack([gx.reshape(-1), gy.reshape(-1), gz.reshape(-1)], axis=1)
    d = np.sqrt(((xyz[:, None, :] - xyz[None, :, :]) ** 2).sum(-1))
    dense = packed.dense()
    assert packed.N == case.N and packed.bits.shape == (15, (case.N + 31) // 32, case.N)
    for e in case.edges:
        assert np.array_equal(dense[e] != 0, np.abs(d - limbs[e]) < 0.4 * limbs[e]), e
    # ... which is the golden's level-1 constraint, padding bits zero
    rows = np.ascontiguousarray(np.transpose(packed.bits, (0, 2, 1)))      # [E, N, words]: numpy.packbits rows
    raw = rows.view(np.uint8)[:, :, :case.g['pairwise_bits'].shape[-1]]
    assert np.array_equal(raw, case.g['pairwise_bits'][0])


# ------------------------------------------------------- 7. production size
def test_production_grid_16_bins(cuda):
    """FIRST_NBINS = 16: N = 4096, full-length LDS rows, 128 mask words per row, 24-bit flat pair
    indices.  GRID_SIZE 2000, limbs 150-450, depth 2, 32 x 32 heatmaps; the mask from the GPU builder;
    level-1 bins and every level's pose against the numpy restatement of infer (chunked)."""
    from multiviews.body import HumanBody
    from multiviews.pictorial import (compute_grid, compute_pairwise_constraint, compute_unary_term, infer,
                                      rpsm_batch)
    body = HumanBody()
    cfg = rs.make_config(16, 2000.0, 2, 32)
    ps, size = cfg.PICT_STRUCT, cfg.NETWORK.IMAGE_SIZE
    grp = rs.make_group(np.random.RandomState(21), 2000.0, (150, 450), 32)
    packed = compute_pairwise_constraint(2000.0, grp['limb_length'], 16)
    assert packed.bits.shape == (15, 128, 4096)
    dense = packed.dense()
    frac = float(np.mean([m.mean() for m in dense.values()]))
    assert 0.001 < frac < 0.2, frac
    grid = compute_grid(2000.0, grp['center'], 16)
    unary = np.stack(compute_unary_term(grp['heatmaps'], [grid], grp['boxes'], grp['cams'], size))
    assert float(np.abs(unary - rs.unary_numpy(grp['heatmaps'], [grid], grp['boxes'], grp['cams'], size)).max()) <= 1e-10
    ref_bins = _body_infer_numpy(unary, dense, body)
    assert len(set(ref_bins.tolist())) > 4                  # not collapsed onto one bin
    assert [b for _, b in infer(list(unary), packed, body, cfg)] == ref_bins.tolist()
    final, levels = rpsm_batch(grp['cams'], grp['heatmaps'], grp['boxes'], grp['center'][None], grp['limb_length'],
                               packed, cfg, return_levels=True)
    pose = grid[ref_bins]
    assert np.array_equal(levels[0, 0], pose)
    cur = ps.GRID_SIZE / ps.FIRST_NBINS
    for level in range(1, ps.RECUR_DEPTH + 1):
        grids = [compute_grid(cur, p, ps.RECUR_NBINS) for p in pose]
        u = np.stack(compute_unary_term(grp['heatmaps'], grids, grp['boxes'], grp['cams'], size))
        pw = {(p, c): rs.pairwise_numpy(grids[p], grids[c], grp['limb_length'][(p, c)], ps.LIMB_LENGTH_TOLERANCE, False)
              for p, c in body.edges()}
        bins = _body_infer_numpy(u, pw, body)
        pose = np.stack([grids[j][bins[j]] for j in range(16)])
        assert float(np.abs(levels[level, 0] - pose).max()) <= 1e-9, level
        cur = cur / ps.RECUR_NBINS
    assert float(np.abs(final[0] - pose).max()) <= 1e-9
