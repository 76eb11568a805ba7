"""The 3-D evaluation protocol on the GPU (csrc/pose3d.hip behind posu.ops, utils.pose_utils and
multiviews.estimate) against the reference's recorded results (tests/golden/pose3d.npz, made by
make_pose3d_golden.py) and the numpy restatement (tests/pose3d_restatement.py).

Gates.  Every float of the golden is a 50-digit evaluation (the yardstick) stored with the
reference's own distance from it (ref_err).  Coordinates (Z, the errors, the translation):
|kernel - yardstick| <= 8 * max(ref_err, ulp(largest |coordinate|)); the normalised residual d:
8 * max(ref_err_d, 2.2e-16).  On the CPU the reference and a numpy restatement of the kernel's
Jacobi algorithm both sit at 2-6 ulp; the factor 8 covers the wave reduction's summation order and
FMA contraction.  Rotations: 1e-13 (at most 90 plane rotations accumulated in two 3 x 3 factors of
entries <= 1).  Flags, modes and the degenerate batch are exact.  The meter: 1e-9 relative (sums of
at most 128 values of one sign; E[x^2] - E[x]^2 on means that spread by >= 1 mm loses < 1e-12).
Each case prints its figures before it asserts.
"""
import numpy as np
import pytest
import torch

import pose3d_restatement as rs

pytestmark = pytest.mark.gpu

CAM_KEYS = ('R', 'T', 'fx', 'fy', 'cx', 'cy', 'k', 'p')


def z_gate(ref_err, coords):
    return 8 * max(float(np.max(ref_err)), float(np.spacing(np.abs(coords).max())))


def d_gate(ref_err):
    return 8 * max(float(np.max(ref_err)), 2.2e-16)


def _dev(a, cuda):
    return torch.from_numpy(np.ascontiguousarray(a)).to(cuda)


def _host(outs):
    return [o.cpu().numpy() for o in outs]


# ------------------------------------------------------------ 1, 2. procrustes
@pytest.mark.parametrize('J', [4, 16, 17, 65])
def test_procrustes_against_the_golden_and_its_invariants(golden, cuda, J):
    from posu import ops
    g = golden('pose3d.npz')
    A, B = g['pa_J%d_A' % J], g['pa_J%d_B' % J]
    worst_z = worst_d = worst_r = 0.0
    for N in (1, 3, 67):                                   # 67: 17 blocks of four waves, the last one partial
        pick = np.arange(N) % A.shape[0]
        a, b = _dev(A[pick], cuda), _dev(B[pick], cuda)
        for k, (scaling, reflection) in enumerate(rs.SETTINGS):
            d, Z, R, scale, t = _host(ops.procrustes(a, b, scaling, reflection))
            assert Z.shape == (N, J, 3) and R.shape == (N, 3, 3) and t.shape == (N, 3) and d.shape == scale.shape == (N,)
            for n, src in enumerate(pick):
                gz = z_gate(g['pa_J%d_ref_err_Z' % J][k, src], A[src])
                gd = d_gate(g['pa_J%d_ref_err_d' % J][k, src])
                ez = float(np.abs(Z[n] - g['pa_J%d_Z' % J][k, src]).max())
                ed = float(abs(d[n] - g['pa_J%d_d' % J][k, src]))
                er = float(np.abs(R[n] - g['pa_J%d_R' % J][k, src]).max())
                orth = float(np.abs(R[n].T.dot(R[n]) - np.eye(3)).max())
                ld = np.longdouble                    # the test's own rounding kept out of the invariant
                form = float(np.abs(ld(scale[n]) * B[src].astype(ld).dot(R[n].astype(ld)) + t[n].astype(ld)
                                    - Z[n].astype(ld)).max())
                if n < 2:
                    print('procrustes J=%d N=%d scaling=%s reflection=%s pair %d: Z %.2e (gate %.2e) d %.2e (gate %.2e) '
                          'R %.2e RtR-I %.2e scale*B*R+t %.2e' % (J, N, scaling, reflection, src, ez, gz, ed, gd, er, orth,
                                                                 form))
                worst_z, worst_d, worst_r = max(worst_z, ez / gz), max(worst_d, ed / gd), max(worst_r, er, orth)
                assert ez <= gz and ed <= gd
                assert er <= 1e-13 and orth <= 1e-13
                assert form <= gz
                assert abs(scale[n] - g['pa_J%d_scale' % J][k, src]) <= 1e-14 * max(1.0, scale[n])
                assert float(np.abs(t[n] - g['pa_J%d_t' % J][k, src]).max()) <= gz
                det = np.linalg.det(R[n])
                assert reflection == 'best' or (det < 0) == reflection
                assert reflection != 'best' or (det < 0) == bool(src)     # pair 1 is mirrored
                assert scaling or scale[n] == 1.0
    print('procrustes J=%d: worst Z / gate %.3f, d / gate %.3f, rotation %.2e' % (J, worst_z, worst_d, worst_r))


def _restatement_err(A, B, scaling, reflection, ref):
    """The numpy restatement's distance from the 50-digit evaluation of the same formulas (mp_procrustes of
    tests/golden/make_pose3d_golden.py, the golden's yardstick; mpmath comes with torch's sympy) for Z, d and
    t: the ref_err of the gates."""
    import os
    import sys
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden'))
    import make_pose3d_golden as mk
    md, mZ, _, _, mt = mk.mp_procrustes(A, B, scaling, reflection)
    return mk._dist(mk._flat(mZ), ref[1]), float(abs(mk.mp.mpf(float(ref[0])) - md)), mk._dist(mk._flat(mt), ref[4])


def _numpy_references(A, B, scaling, reflection, rank2):
    """rs.procrustes, and at rank 2 with reflection 'best' also the same numpy SVD with the third column of U
    negated: LAPACK completes that column with a sign of its choice, the kernel with a cross product, and with
    'best' nothing fixes the sign afterwards (a forced reflection does, through the determinant)."""
    refs = [rs.procrustes(A, B, scaling, reflection)]
    if rank2 and reflection == 'best':
        M, stats = rs._normalise(A, B)
        U, s, Vt = np.linalg.svd(M)
        U[:, 2] = -U[:, 2]
        refs.append(rs._finish(A, B, s, U, Vt.T, scaling, reflection, stats))
    return refs


@pytest.mark.parametrize('J', [3, 65])
def test_procrustes_five_poses_against_the_numpy_restatement(cuda, J):
    """N = 5 leaves three waves of the second block idle; J = 3 is the smallest J with a rank-2 M (three
    centred points span a plane), J = 65 wraps the lane stride once.  Against rs.procrustes (numpy's SVD) at
    the gates of the golden test: 8 * max(ref_err, ulp of the largest coordinate) for Z and for t, each with
    its own ref_err, 8 * max(ref_err_d, 2.2e-16) for d, 1e-13 for the rotation, 1e-14 for the scale, and the
    kernel's own Z = scale * B R + t at the Z gate.  ref_err is, as in the golden, the reference's own
    distance from the 50-digit evaluation of the same formulas -- here the numpy restatement's, evaluated in
    the test by the golden maker's mp_procrustes.  (With ref_err left at 0 the J = 65 case measured Z 5.7e-12
    mm against a gate of 3.6e-12 on an MI355X: 6 ulp of coordinates that passed 4096 mm where the gate
    counted ulps of an A below it; every other figure was inside.)
    At J = 3 M has rank 2 exactly, the 50-digit SVD has no third singular value to order by, and ref_err
    stays 0: every gate is the plain 8 ulp.  What ref_err absorbs at J = 65, the conditioning of the pose,
    is therefore bounded on the inputs instead: R is the orthogonal polar factor of M and moves by about
    eps / (s1 - |s2|) per unit rounding (s2 = 0 here), and t = a_bar - scale * b_bar R multiplies that by a
    centroid as large as the coordinates, so 8 ulp for t needs s1 of a few tenths.  Pairs are drawn from the
    seeded stream until five have s1 >= 0.25; three joints nearer a line approach the rank-1 case that has no
    defined result (csrc/pose3d.hip).  The first pair dropped has s1 = 0.0026; there numpy itself is 114 ulp
    from the 50-digit t.  With reflection 'best' the kernel's R and t must match one of numpy's two
    completions of U; both poses lie in planes, so Z, d and the scale do not see the sign."""
    from posu import ops
    rng = np.random.RandomState(17)
    pairs = []
    while len(pairs) < 5:
        pa, pb = rs.make_pair(rng, J, mirrored=bool(len(pairs) & 1))
        s1 = np.linalg.svd(rs._normalise(pa, pb)[0], compute_uv=False)[1]
        if J > 3 or s1 >= 0.25:
            pairs.append((pa, pb))
    A, B = np.stack([p[0] for p in pairs]), np.stack([p[1] for p in pairs])
    a, b = _dev(A, cuda), _dev(B, cuda)
    for scaling, reflection in rs.SETTINGS:
        d, Z, R, scale, t = _host(ops.procrustes(a, b, scaling, reflection))
        assert Z.shape == (5, J, 3) and R.shape == (5, 3, 3) and t.shape == (5, 3) and d.shape == scale.shape == (5,)
        for n in range(5):
            refs = _numpy_references(A[n], B[n], scaling, reflection, J == 3)
            rd, rZ, _, rscale, _ = refs[0]
            ref_z, ref_d, ref_t = _restatement_err(A[n], B[n], scaling, reflection, refs[0]) if J > 3 else (0.0, 0.0, 0.0)
            gz, gd, gt = z_gate(ref_z, A[n]), d_gate(ref_d), z_gate(ref_t, A[n])
            ez, ed = float(np.abs(Z[n] - rZ).max()), float(abs(d[n] - rd))
            # R and t against the completion they are nearer to (one reference unless rank 2 and 'best')
            er, et = min((float(np.abs(R[n] - r[2]).max()), float(np.abs(t[n] - r[4]).max())) for r in refs)
            orth = float(np.abs(R[n].T.dot(R[n]) - np.eye(3)).max())
            ld = np.longdouble
            form = float(np.abs(ld(scale[n]) * B[n].astype(ld).dot(R[n].astype(ld)) + t[n].astype(ld)
                                - Z[n].astype(ld)).max())
            print('procrustes J=%d scaling=%s reflection=%s pose %d: Z %.2e scale*B*R+t %.2e (gate %.2e) t %.2e (gate '
                  '%.2e) d %.2e (gate %.2e) R %.2e RtR-I %.2e' % (J, scaling, reflection, n, ez, form, gz, et, gt, ed, gd,
                                                                  er, orth))
            assert ez <= gz and ed <= gd and form <= gz and et <= gt
            assert er <= 1e-13 and orth <= 1e-13
            assert abs(scale[n] - rscale) <= 1e-14 * max(1.0, scale[n])
            assert reflection == 'best' or (np.linalg.det(R[n]) < 0) == reflection
            assert scaling or scale[n] == 1.0


def test_pose_utils_procrustes_keeps_the_reference_interface(golden, cuda):
    from posu import ops
    from utils.pose_utils import PoseUtils
    g = golden('pose3d.npz')
    A, B = g['pa_J16_A'], g['pa_J16_B']
    want = _host(ops.procrustes(_dev(A, cuda), _dev(B, cuda), False, True))
    d, Z, tform = PoseUtils().procrustes(A[1], B[1], scaling=False, reflection=True)        # numpy in, numpy out
    assert isinstance(d, float) and isinstance(Z, np.ndarray) and Z.shape == (16, 3) and set(tform) == {
        'rotation', 'scale', 'translation'}
    assert d == want[0][1] and np.array_equal(Z, want[1][1]) and np.array_equal(tform['rotation'], want[2][1])
    assert tform['scale'] == 1.0 and np.array_equal(tform['translation'], want[4][1])
    d, Z, tform = PoseUtils().procrustes(_dev(A, cuda).float(), _dev(B, cuda).float())      # batched, on the device
    assert all(x.is_cuda and x.dtype == torch.float64 for x in (d, Z, tform['rotation'], tform['scale'],
                                                                tform['translation']))
    assert Z.shape == (2, 16, 3) and tform['rotation'].shape == (2, 3, 3) and d.shape == (2,)
    ref = rs.procrustes(A[0].astype(np.float32).astype(np.float64), B[0].astype(np.float32).astype(np.float64))
    assert float(np.abs(Z[0].cpu().numpy() - ref[1]).max()) <= z_gate(1e-11, A)
    with pytest.raises(ValueError):
        PoseUtils().procrustes(A[0], B[0], reflection='worst')
    with pytest.raises(ValueError):
        PoseUtils().procrustes(A[0], B[0, :8])


# ------------------------------------------------------------- 3. pose3d_errors
@pytest.mark.parametrize('J', [16, 17])
def test_pose3d_errors_against_the_golden(golden, cuda, J):
    from multiviews import estimate
    from posu import ops
    g = golden('pose3d.npz')
    X, gt, R, T = (g['er_J%d_%s' % (J, k)] for k in ('X', 'gt', 'R', 'T'))
    for k, name in enumerate(('No', 'Yes')):
        for G in (1, 5):
            for V in (1, 4):
                args = [_dev(a, cuda) for a in (X[:G], gt[:G, :V], R[:G, :V], T[:G, :V])]
                err, aligned = _host(ops.pose3d_errors(*args, procrustes=(name == 'Yes'), return_aligned=True))
                gate = z_gate(g['er_J%d_ref_err' % J][k, :G, :V], gt[:G, :V])
                e = float(np.abs(err - g['er_J%d_err' % J][k, :G, :V]).max())
                print('pose3d_errors J=%d Procrustes=%s G=%d V=%d: %.2e (gate %.2e)' % (J, name, G, V, e, gate))
                assert err.shape == (G, V, J) and e <= gate
                assert float(np.abs(np.linalg.norm(gt[:G, :V] - aligned, axis=3) - err).max()) <= gate
                assert np.array_equal(_host([ops.pose3d_errors(*args, procrustes=(name == 'Yes'))])[0], err)
        # the reference's signature, one group: V arrays [J]
        errs = estimate.error_computing_3d(X[2], list(gt[2]), list(R[2]), [t.reshape(3, 1) for t in T[2]], name)
        assert isinstance(errs, list) and len(errs) == 4 and errs[0].shape == (J,)
        assert float(np.abs(np.stack(errs) - g['er_J%d_err' % J][k, 2]).max()) <= z_gate(g['er_J%d_ref_err' % J][k, 2], gt[2])
    # batched, numpy in -> numpy out; cuda in -> cuda out
    out = estimate.pose3d_errors(X, gt, R, T, procrustes=True)
    assert isinstance(out, np.ndarray) and float(np.abs(out - g['er_J%d_err' % J][1]).max()) <= z_gate(
        g['er_J%d_ref_err' % J][1], gt)
    assert estimate.pose3d_errors(*[_dev(a, cuda) for a in (X, gt, R, T)]).is_cuda


# ---------------------------------------------------------------- 4. limb_break
@pytest.mark.parametrize('per_group', [False, True])
def test_limb_break_against_the_golden(golden, cuda, per_group):
    from multiviews import estimate
    from multiviews.body import HumanBody
    from posu import ops
    g = golden('pose3d.npz')
    name = 'group' if per_group else 'shared'
    poses, limb, moved = rs.make_limb_cases(300 + per_group, 70, per_group)
    assert float(poses.sum()) == float(g['lb_%s_sum' % name])
    want = g['lb_%s_flag' % name]
    assert np.array_equal(want.astype(bool), moved) and 20 < want.sum() < 50
    parent = _dev(rs.PARENT, cuda)
    assert np.array_equal(HumanBody().parents(), rs.PARENT)
    for G in (1, 70):
        lg = limb[:G] if per_group else limb
        flag, worst = ops.limb_break(_dev(poses[:G], cuda), parent, _dev(lg, cuda), 0.4, return_worst=True)
        assert flag.dtype == torch.uint8 and np.array_equal(flag.cpu().numpy(), want[:G])
        ref_worst = rs.limb_break(poses[:G], rs.PARENT, lg)[1]
        assert float(np.abs(worst.cpu().numpy() - ref_worst).max()) <= 1e-12
    # the batched form of multiviews.estimate takes the forms rpsm_batch takes
    edges = HumanBody().edges()
    rows = np.broadcast_to(limb, (70, 16))
    forms = [[{e: rows[i, e[1]] for e in edges} for i in range(70)], np.ascontiguousarray(rows)]
    if not per_group:
        forms += [{e: limb[e[1]] for e in edges}, limb]
    for form in forms:
        out = estimate.break_limb_length_batch(poses, form)
        assert out.dtype == bool and np.array_equal(out, moved)
    assert np.array_equal(estimate.break_limb_length_batch(_dev(poses, cuda), forms[1]).cpu().numpy(), want)
    skel = HumanBody().skeleton
    assert [estimate.break_limb_length(skel, poses[i], forms[0][i]) for i in range(4)] == moved[:4].tolist()


def test_limb_break_ties_do_not_flag_and_a_nan_never_does(golden, cuda):
    from multiviews import estimate
    from posu import ops
    g = golden('pose3d.npz')
    poses, limb, thres = g['lb_tie_poses'], g['lb_tie_limb'], g['lb_tie_thres']
    assert poses[0, 1, 0] == 15.0 and poses[1, 1, 0] == 14.0 and poses[2, 1, 0] == 15.000001 and np.isnan(poses[3]).any()
    assert 0.4 * 10 == 4.0 and 0.5 * 10 == 5.0
    assert g['lb_tie_flag'].tolist() == [0, 0, 1, 0]
    parent = _dev(np.array([-1, 0], dtype=np.int32), cuda)
    two = [{'idx': 0, 'children': [1]}, {'idx': 1, 'children': []}]
    for i in range(4):
        flag = ops.limb_break(_dev(poses[i:i + 1], cuda), parent, _dev(limb[i:i + 1], cuda), float(thres[i]))
        assert flag.cpu().tolist() == [int(g['lb_tie_flag'][i])], i
        assert estimate.break_limb_length(two, poses[i], {(0, 1): 10.0}, thres[i]) == bool(g['lb_tie_flag'][i])
    # the NaN pose inside a batch leaves its neighbours alone
    flag = ops.limb_break(_dev(poses[[2, 3, 0]], cuda), parent, _dev(limb[0], cuda), 0.5)
    assert flag.cpu().tolist() == [1, 0, 0]


# --------------------------------------------------------------------- 5. modes
class _RpsmCase:
    """tests/golden/rpsm_a.npz (3 groups, 4 views, 24 x 24 heatmaps, 5^3 bins) as estimate_poses' arguments."""

    def __init__(self, g):
        import sys
        import os
        sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'tools'))
        import rpsm_synthetic
        self.g, self.G = g, g['heatmaps'].shape[0]
        self.edges = [tuple(e) for e in g['edges'].tolist()]
        self.config = rpsm_synthetic.make_config(int(g['first_nbins']), float(g['grid_size']), int(g['recur_depth']),
                                                 g['heatmaps'].shape[-1], recur_nbins=int(g['recur_nbins']),
                                                 tolerance=float(g['tolerance']))
        self.cams = [{k: g['cam_' + k][gi, v] for k in CAM_KEYS} for gi in range(self.G) for v in range(4)]
        self.boxes = [{'center': g['box_center'][gi, v], 'scale': g['box_scale'][gi, v]}
                      for gi in range(self.G) for v in range(4)]
        self.hm = g['heatmaps'].reshape(self.G * 4, 16, 24, 24)
        self.limbs = [{e: float(g['limb_length'][gi, i]) for i, e in enumerate(self.edges)} for gi in range(self.G)]
        bits = np.unpackbits(g['pairwise_bits'][0], axis=-1, bitorder='little')[:, :, :int(g['first_nbins']) ** 3]
        self.pairwise = {e: bits[i] for i, e in enumerate(self.edges)}

    def poses2d(self, pose3d):
        from multiviews.cameras import project_pose
        return np.stack([project_pose(pose3d[i // 4], cam) for i, cam in enumerate(self.cams)])


@pytest.fixture(scope='module')
def rpsm_case(golden, cuda):
    return _RpsmCase(golden('rpsm_a.npz'))


def test_estimate_poses_modes(rpsm_case, cuda):
    from multiviews import estimate
    from multiviews.pictorial import pack_pairwise, rpsm_batch
    from multiviews.triangulate import triangulate_poses
    c = rpsm_case
    true = c.g['true_pose']
    for gi in range(c.G):                                # the golden's limb lengths are true_pose's own
        for (p, ch), L in c.limbs[gi].items():
            assert abs(np.linalg.norm(true[gi, p] - true[gi, ch]) - L) <= 3e-14
    moved = true.copy()
    moved[1, 0] = moved[1, 0] + (moved[1, 0] - moved[1, 1]) * 0.6       # joint 0 hangs on joint 1
    packed = pack_pairwise(c.pairwise)
    clean2d, moved2d = c.poses2d(true), c.poses2d(moved)

    def run(p2d, mode):
        poses, info = estimate.estimate_poses(c.cams, p2d, c.hm, c.boxes, c.limbs, packed, c.config, mode=mode)
        assert poses.is_cuda and poses.dtype == torch.float64 and tuple(poses.shape) == (3, 16, 3)
        assert info['refined'].dtype == bool and isinstance(info['count'], int) and info['triangulated'].is_cuda
        return poses.cpu().numpy(), info

    x0 = triangulate_poses(c.cams, moved2d)
    rows = np.stack([[c.limbs[gi].get((int(rs.PARENT[j]), j), 0.0) for j in range(16)] for gi in range(3)])
    flags, worst = rs.limb_break(x0, rs.PARENT, rows)
    print('modes: worst offset / limb per group %s' % np.round(worst, 4))
    assert flags.tolist() == [False, True, False]        # exactly the moved group breaks its limb lengths

    tri, info = run(moved2d, 'triangulation')
    assert np.array_equal(tri, x0) and info['count'] == 0 and not info['refined'].any()
    alone, _ = estimate.estimate_poses(c.cams, moved2d, None, None, None, None, c.config, mode='triangulation')
    assert np.array_equal(alone.cpu().numpy(), x0)

    ps, info = run(moved2d, 'pict_struct')
    assert np.array_equal(ps, rpsm_batch(c.cams, c.hm, c.boxes, x0[:, 6], c.limbs, packed, c.config))
    assert info['count'] == 3 and info['refined'].all() and np.array_equal(info['triangulated'].cpu().numpy(), x0)

    comb, info = run(moved2d, 'combination')
    assert np.array_equal(comb[[0, 2]], x0[[0, 2]])
    assert np.array_equal(comb[1], rpsm_batch(c.cams[4:8], c.hm[4:8], c.boxes[4:8], x0[1:2, 6], c.limbs[1], packed,
                                              c.config)[0])
    assert not np.array_equal(comb[1], x0[1])
    assert info['refined'].tolist() == [False, True, False] and info['count'] == 1
    assert np.array_equal(info['triangulated'].cpu().numpy(), x0)
    on_dev, info = estimate.estimate_poses(c.cams, _dev(moved2d, cuda), _dev(c.hm, cuda), c.boxes, rows, packed,
                                           c.config)    # device inputs, limbs as [G, J], the default mode
    assert np.array_equal(on_dev.cpu().numpy(), comb) and info['count'] == 1

    same, info = run(clean2d, 'combination')             # nothing moved: no group goes through RPSM
    assert np.array_equal(same, run(clean2d, 'triangulation')[0]) and info['count'] == 0


# ----------------------------------------------------------- 6. degenerate pose
def test_a_degenerate_pose_ends_in_nan_and_leaves_its_neighbours_alone(cuda):
    """Termination on legitimate input: a pose whose joints all coincide normalises to 0 / 0; the
    bounded, NaN-false Jacobi test ends its wave, and the other waves' results do not change."""
    from posu import ops
    rng = np.random.RandomState(7)
    pairs = [rs.make_pair(rng, 16) for _ in range(5)]
    A, B = np.stack([p[0] for p in pairs]), np.stack([p[1] for p in pairs])
    B[2] = B[2, 0]
    keep = [0, 1, 3, 4]
    for scaling, reflection in rs.SETTINGS:
        full = _host(ops.procrustes(_dev(A, cuda), _dev(B, cuda), scaling, reflection))
        part = _host(ops.procrustes(_dev(A[keep], cuda), _dev(B[keep], cuda), scaling, reflection))
        for f, p in zip(full, part):
            assert np.array_equal(f[keep], p) and np.isfinite(p).all()
        d, Z, R, scale, t = full
        assert np.isnan(Z[2]).all() and np.isnan(R[2]).all() and np.isnan(t[2]).all() and np.isnan(d[2])
    X, gt, Rc, T = rs.make_groups(rng, 2, 4, 16)
    gt[1, 2] = gt[1, 2, 0]
    err = ops.pose3d_errors(*[_dev(a, cuda) for a in (X, gt, Rc, T)], procrustes=True).cpu().numpy()
    assert np.isnan(err[1, 2]).all() and np.isfinite(np.delete(err.reshape(8, 16), 6, axis=0)).all()


def test_coplanar_joints_align_like_the_reference(cuda):
    """Rank-2 M: the kernel completes U with a cross product where LAPACK picks a sign.  With B in a
    plane (alone or with A) that sign does not reach Z, d, scale or t; with only A in a plane it flips Z
    about that plane, so Z is compared inside the plane and by its distance from it.  Bound: the kernel
    and the numpy restatement each sit within 8 ulp of the largest coordinate of the exact result (the
    gate of the golden cases), so they differ by at most 16."""
    from posu import ops
    rng = np.random.RandomState(13)
    for J in (5, 16):
        A, B = rs.make_pair(rng, J)
        cases = {'both': (A * [1, 1, 0] + [0, 0, 700.0], B * [1, 1, 0] + [0, 0, -300.0]),
                 'B': (A, B * [1, 1, 0] + [0, 0, 250.0]),
                 'A': (A * [1, 1, 0] + [0, 0, 700.0], B)}
        for name, (a, b) in cases.items():
            tol = 16 * float(np.spacing(np.abs(a).max()))
            for scaling, reflection in rs.SETTINGS:
                d, Z, R, scale, t = [o[0] for o in _host(ops.procrustes(_dev(a[None], cuda), _dev(b[None], cuda),
                                                                        scaling, reflection))]
                rd, rZ, rR, rscale, rt = rs.procrustes(a, b, scaling, reflection)
                assert np.isfinite(Z).all() and float(np.abs(R.T.dot(R) - np.eye(3)).max()) <= 1e-13
                assert reflection == 'best' or (np.linalg.det(R) < 0) == reflection
                ez = float(np.abs(Z[:, :2] - rZ[:, :2]).max())
                eh = float(np.abs(np.abs(Z[:, 2] - 700.0) - np.abs(rZ[:, 2] - 700.0)).max()) if name == 'A' else \
                    float(np.abs(Z[:, 2] - rZ[:, 2]).max())
                print('coplanar %s J=%d %s/%s: Z %.2e / %.2e (bound %.2e) d %.2e' % (name, J, scaling, reflection, ez, eh,
                                                                                   tol, abs(d - rd)))
                assert ez <= tol and eh <= tol
                assert abs(d - rd) <= 16 * 2.2e-16 and abs(scale - rscale) <= 1e-14 * rscale
                if name != 'A':
                    assert float(np.abs(t - rt).max()) <= tol


# ------------------------------------------------------------------- 7. the meter
def test_pose3d_meter_reports_like_the_reference(cuda):
    from multiviews.estimate import Pose3DMeter
    rng = np.random.RandomState(11)
    errs, befores, actions, refined = [], [], [[0, 2, 2, 1, 0], [1, 2, 1]], [np.zeros(5, bool), np.zeros(3, bool)]
    refined[0][3] = refined[1][0] = True
    for G in (5, 3):
        level = rng.uniform(20, 120, (G, 4, 1))           # per-sample means spread by far more than 1 mm
        errs.append(level + rng.uniform(0, 30, (G, 4, 16)))
        befores.append(errs[-1] + rng.uniform(0, 50, (G, 4, 16)))
    means = np.concatenate([e.mean(2).reshape(-1) for e in errs])
    assert np.ptp(means) >= 1.0
    meter = Pose3DMeter(16, 3)
    for e, b, a, r in zip(errs, befores, actions, refined):
        meter.update(_dev(e, cuda), a, refined=r, err_before=_dev(b, cuda))
    got, want = meter.summary(), rs.summary(errs, actions, refined, befores)
    print('meter: mpjpe %.6f variance %.6f compare %s' % (got['mpjpe'], got['variance'], got['compare']))
    assert set(got) == set(want) and got['pict_struct_count'] == 2 and got['groups'] == 8
    np.testing.assert_allclose(got['mpjpe'], want['mpjpe'], rtol=1e-9)
    np.testing.assert_allclose(got['joint_wise'], want['joint_wise'], rtol=1e-9)
    np.testing.assert_allclose(got['variance'], want['variance'], rtol=1e-9)
    assert sorted(got['action_wise']) == sorted(want['action_wise']) == [0, 1, 2]
    for a in want['action_wise']:
        np.testing.assert_allclose(got['action_wise'][a], want['action_wise'][a], rtol=1e-9)
    for k in ('before', 'after'):
        np.testing.assert_allclose(got['compare'][k], want['compare'][k], rtol=1e-9)
    assert got['compare']['before'] > got['compare']['after']
    plain = Pose3DMeter(16, 3)                            # no refinement recorded: nothing to compare
    plain.update(_dev(errs[0], cuda), actions[0])
    assert plain.summary()['compare'] is None and plain.summary()['pict_struct_count'] == 0
