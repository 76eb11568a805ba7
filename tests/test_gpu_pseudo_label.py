"""The pseudo-label round on the device against the oracle's geometry (oracle.geometry_ref through
tests/pseudo_label_restatement.py) and the reference's recorded PCKh values (tests/golden/pseudo_label.npz).

Masks and counts are compared exactly.  That is safe because the inputs keep every decision away from its
threshold, which each test asserts on the CPU through the oracle before it looks at a device result: no
reprojection error within 1e-6 px of REPROJ_THRE, no two pairs of a joint with equal inlier counts and mean
errors within 1e-9 px, no detection distance within 1e-3 px of half the head size -- all far above the
1e-9 px or so by which two fp64 evaluations of this geometry differ -- and every joint visible in every set
(a finite PCKh).  The seeds that meet them were found by make_pseudo_label_golden.py --search; nothing is
masked out.  Against the oracle, projections carry posu_reproject's bar in test_gpu_kernels.py, 1e-4 px;
against posu_reproject itself they are compared exactly: the sweep and that entry point inline one function
(solve_project, csrc/geometry_common.h)."""
import functools
import os

import numpy as np
import pytest
import torch

import pseudo_label_restatement as rs
from posu import _native, ops
from posu import synthetic as syn

pytestmark = pytest.mark.gpu
J = 16


@functools.lru_cache(maxsize=None)
def case_inputs(name):
    ngroups, distortion, thresholds = rs.CASES[name]
    inp = rs.make_inputs(rs.SEEDS[name], ngroups, distortion)
    inp['err'] = rs.pair_table(inp['locations'][:, :, :2].astype(np.float64), inp['cams'], not distortion)
    return inp


@functools.lru_cache(maxsize=None)
def case_stages(name, inliers, use_ransac):
    """The oracle's stages of one case (computed once, shared, never modified) with the conditions asserted."""
    ngroups, distortion, thresholds = rs.CASES[name]
    inp = case_inputs(name)
    masks, proj = rs.stages(inp['locations'], inp['cams'], thresholds, not distortion, rs.REPROJ_THRE, inliers,
                            use_ransac)
    # every joint stays visible where the golden's PCKh is compared; other settings only compare masks
    golden_setting = inliers == rs.GOLDEN_INLIERS and use_ransac
    bad = rs.conditions(inp['locations'], inp['gt2d'], inp['headsizes'], inp['err'], masks, proj, rs.REPROJ_THRE,
                        all_visible=golden_setting)
    assert not bad, bad
    masks.setflags(write=False)
    proj.setflags(write=False)
    return masks, proj


def device_tables(inp, cuda, nviews, no_distortion):
    from multiviews.triangulate import camera_tables
    M, intr = camera_tables(inp['cams'], nviews, no_distortion=no_distortion)
    loc = torch.from_numpy(inp['locations']).to(cuda)
    g = len(inp['cams']) // nviews
    xy = loc[:, :, :2].double().reshape(g, nviews, -1, 2).contiguous()
    conf = loc[:, :, 2].reshape(g, nviews, -1).contiguous()
    return torch.from_numpy(M).to(cuda), torch.from_numpy(intr).to(cuda), xy, conf


def check_sweep(cuda, inp, masks, proj, thresholds, nviews, no_distortion, inliers, use_ransac):
    M, intr, xy, conf = device_tables(inp, cuda, nviews, no_distortion)
    g, _, nj, _ = xy.shape
    got_m, got_p = ops.pseudo_label_sweep(M, intr, xy, conf, thresholds, rs.REPROJ_THRE, inliers, use_ransac,
                                          undistort=not no_distortion)
    assert got_m.shape == (len(thresholds), 3, g, nviews, nj) and got_m.dtype == torch.uint8
    assert got_p.shape == (len(thresholds), g, nviews, nj, 2) and got_p.dtype == torch.float64
    gm = got_m.cpu().numpy().reshape(len(thresholds), 3, g * nviews, nj)
    gp = got_p.cpu().numpy().reshape(len(thresholds), g * nviews, nj, 2)
    assert set(np.unique(gm)) <= {0, 1}
    for t, thre in enumerate(thresholds):
        for s in range(3):
            np.testing.assert_array_equal(gm[t, s].astype(bool), masks[t, s], err_msg='thre %s stage %d' % (thre, s))
        perr = float(np.abs(gp[t] - proj[t]).max())
        print('thre %s: projections within %.2e px of the oracle' % (thre, perr))
        assert perr <= 1e-4
        # the existing entry points, called per threshold on the same masks
        vis0 = got_m[t, 0]
        np.testing.assert_array_equal(
            ops.ransac_inliers(M, intr, xy, vis0, float(rs.REPROJ_THRE), inliers, undistort=not no_distortion)
            .cpu().numpy(), got_m[t, 1].cpu().numpy())
        p1, v1 = ops.reproject(M, intr, xy, got_m[t, 1] if use_ransac else vis0, undistort=not no_distortion)
        np.testing.assert_array_equal(v1.cpu().numpy(), got_m[t, 2].cpu().numpy())
        print('thre %s: posu_reproject and the sweep differ by %.2e px' % (thre, float((p1 - got_p[t]).abs().max())))
        assert torch.equal(p1, got_p[t])
    return got_m, got_p


@pytest.mark.parametrize('inliers', rs.INLIERS)
@pytest.mark.parametrize('use_ransac', [True, False])
@pytest.mark.parametrize('name', list(rs.CASES))
def test_sweep_masks_and_projections_match_oracle_and_existing_ops(cuda, golden, name, use_ransac, inliers):
    """G = 5 (80 threads: two blocks) with and without distortion, and G = 8 with T = 8 and two equal
    thresholds in a row (the n-view solve is reused)."""
    ngroups, distortion, thresholds = rs.CASES[name]
    masks, proj = case_stages(name, inliers, use_ransac)
    if inliers == rs.GOLDEN_INLIERS and use_ransac:       # the stored stages are these
        g = golden('pseudo_label.npz')
        assert np.array_equal(masks, g[name + '_masks']) and np.array_equal(proj, g[name + '_proj'])
    assert masks[:, 1].any() and not masks[:, 1].all()
    check_sweep(cuda, case_inputs(name), masks, proj, thresholds, 4, not distortion, inliers, use_ransac)


@pytest.mark.parametrize('inliers', rs.INLIERS)
@pytest.mark.parametrize('use_ransac', [True, False])
def test_sweep_three_views_five_joints_one_threshold(cuda, use_ransac, inliers):
    inp = rs.make_v3_inputs()
    masks, proj, err = rs.stages_views(inp['locations'], inp['cams'], [0.6], False, rs.REPROJ_THRE, inliers,
                                       use_ransac, 3)
    bad = rs.conditions(inp['locations'], inp['gt2d'], inp['headsizes'], err, masks, proj, rs.REPROJ_THRE,
                        all_visible=inliers <= 3)          # four inliers of three views: RANSAC keeps nothing
    assert not bad, bad
    assert masks[:, 1].any() == (inliers <= 3)
    check_sweep(cuda, inp, masks, proj, [0.6], 3, False, inliers, use_ransac)


def test_no_groups_launch_nothing_and_return_empty(cuda):
    M = torch.zeros(0, 4, 3, 4, dtype=torch.float64, device=cuda)
    intr = torch.zeros(0, 4, 9, dtype=torch.float64, device=cuda)
    xy = torch.zeros(0, 4, J, 2, dtype=torch.float64, device=cuda)
    conf = torch.zeros(0, 4, J, device=cuda)
    m, p = ops.pseudo_label_sweep(M, intr, xy, conf, [0.6, 0.7])
    assert m.shape == (2, 3, 0, 4, J) and p.shape == (2, 0, 4, J, 2)
    out = torch.full((3, 2 * J + 5), 7, dtype=torch.int32, device=cuda)
    c = ops.pckh_counts(torch.zeros(0, J, 2, device=cuda), torch.zeros(3, 0, J, dtype=torch.uint8, device=cuda),
                        torch.zeros(0, J, 2, device=cuda), torch.zeros(0, 1, device=cuda), 4, out=out)
    assert c.data_ptr() == out.data_ptr() and not c.cpu().numpy().any()


@pytest.mark.parametrize('name', list(rs.CASES))
def test_counts_equal_numpy_and_my_eval_equals_the_reference(cuda, golden, name):
    from multiviews import pseudo_label as pl
    ngroups, distortion, thresholds = rs.CASES[name]
    g = golden('pseudo_label.npz')
    inp = case_inputs(name)
    masks, proj = case_stages(name, rs.GOLDEN_INLIERS, True)
    got_m, got_p = check_sweep(cuda, inp, masks, proj, thresholds, 4, not distortion, rs.GOLDEN_INLIERS, True)
    t, n = len(thresholds), ngroups * 4
    pred = torch.from_numpy(inp['locations'][:, :, :2]).to(cuda)
    gt, head = torch.from_numpy(inp['gt2d']).to(cuda), torch.from_numpy(inp['headsizes']).to(cuda)
    counts = ops.pckh_counts(pred, got_m.reshape(t * 3, n, J), gt, head, 4, 0.5, pred_sets=got_p.reshape(t, n, J, 2),
                             set_pred=[s for i in range(t) for s in (-1, -1, i)]).cpu().numpy().reshape(t, 3, -1)
    assert counts.dtype == np.int32 and counts.shape[2] == 2 * J + 5
    gp = got_p.cpu().numpy().reshape(t, n, J, 2)
    p64 = inp['locations'][:, :, :2].astype(np.float64)
    for i in range(t):
        for s in range(3):
            want = rs.counts(gp[i] if s == 2 else p64, inp['gt2d'], masks[i, s], inp['headsizes'])
            np.testing.assert_array_equal(counts[i, s], want, err_msg='threshold %d stage %d' % (i, s))
            assert pl.pckh_from_counts(counts[i, s, :J], counts[i, s, J:2 * J]) == g[name + '_pckh'][i, s]
    assert 0 < counts[:, :, :J].sum() < counts[:, :, J:2 * J].sum()       # detection is neither all nor nothing
    # no ground truth: no detections, the visibility counts stand
    blind = ops.pckh_counts(None, got_m.reshape(t * 3, n, J), None, None, 4).cpu().numpy().reshape(t, 3, -1)
    assert not blind[:, :, :J].any() and np.array_equal(blind[:, :, J:], counts[:, :, J:])
    # my_eval on device tensors and on numpy arrays: the reference's value, bit for bit
    for i in (0, t - 1):
        for s in range(3):
            p = torch.from_numpy(proj[i].copy()).to(cuda) if s == 2 else pred
            got = pl.my_eval(p, gt, torch.from_numpy(masks[i, s].copy()).to(cuda), head)
            assert got == g[name + '_pckh'][i, s], (i, s, got)
    assert pl.my_eval(inp['locations'][:, :, :2], inp['gt2d'], masks[0, 0], inp['headsizes']) == g[name + '_pckh'][0, 0]
    if name == 'g5_dist':               # one joint never visible: nan, as in the reference
        vis = masks[0, 0].copy()
        vis[:, 3] = False
        assert np.isnan(pl.my_eval(pred, gt, torch.from_numpy(vis).to(cuda), head)) and np.isnan(g['nan_pckh'])


def round_cfg(distortion, use_ransac=True, use_reproj=True, loop=False, inliers=rs.GOLDEN_INLIERS):
    cfg = syn.make_cfg()
    cfg.DATASET.NO_DISTORTION = not distortion
    cfg.PSEUDO_LABEL.NUM_INLIERS, cfg.PSEUDO_LABEL.REPROJ_THRE = inliers, rs.REPROJ_THRE
    cfg.PSEUDO_LABEL.IF_RANSAC, cfg.PSEUDO_LABEL.USE_REPROJ = use_ransac, use_reproj
    cfg.PSEUDO_LABEL.IF_LOOP, cfg.PSEUDO_LABEL.CONFIDENCE_THRE = loop, 0.6
    return cfg


def check_records(records, want, pckh_rows, locations):
    assert [r['name'] for r in records] == [w['name'] for w in want]
    for r, w, pk in zip(records, want, pckh_rows):
        assert sorted(r) == ['joints_at', 'joints_vis', 'name', 'pckh', 'pseudo_2d', 'ransac', 'vis_share']
        assert r['joints_vis'].dtype == bool and np.array_equal(r['joints_vis'], w['joints_vis'])
        assert np.array_equal(r['joints_at'], w['joints_at']) and r['joints_at'].shape == (5,)
        assert r['vis_share'] == w['vis_share']
        if pk is not None:
            assert r['pckh'] == pk[w['stage']], r['name']
        if w['stage'] == 0:
            assert r['pseudo_2d'].dtype == np.float32 and np.array_equal(r['pseudo_2d'], locations[:, :, :2])
        else:
            assert float(np.abs(r['pseudo_2d'] - w['pseudo_2d']).max()) <= 1e-4
        assert (r['ransac'] is None) == (w['ransac'] is None)
        if w['ransac'] is not None:
            assert np.array_equal(r['ransac']['joints_vis'], w['ransac']['joints_vis'])
            assert np.array_equal(r['ransac']['joints_at'], w['ransac']['joints_at'])
            assert r['ransac']['vis_share'] == w['ransac']['vis_share']
            if pk is not None:
                assert r['ransac']['pckh'] == pk[1]


def test_round_default_sweep_equals_restatement_and_golden(cuda, golden, monkeypatch):
    """The reference's default sweep (0.6 .. 0.9) on the eight-group inputs: records, one sweep and one counts
    call, the same from a cuda tensor, and the loop-training form."""
    from multiviews import pseudo_label as pl
    g = golden('pseudo_label.npz')
    inp = case_inputs('g8_t8')
    masks, proj = case_stages('g8_t8', rs.GOLDEN_INLIERS, True)
    rows = rs.DEFAULT_ROWS
    masks, proj, pckh = masks[rows], proj[rows], g['g8_t8_pckh'][rows]
    thresholds = [0.6, 0.7, 0.8, 0.9]
    want = rs.round_records(inp['locations'], thresholds, masks, proj, True, True)
    calls = []
    real = _native.call
    monkeypatch.setattr(_native, 'call', lambda name, *a: (calls.append(name), real(name, *a))[1])
    records = pl.pseudo_label_round(inp['locations'], inp['cams'], inp['gt2d'], inp['headsizes'], round_cfg(True))
    assert calls == ['posu_pseudo_label_sweep', 'posu_pckh_counts']
    assert [r['name'] for r in records] == ['0.6_0', '0.6_1', '0.7_0', '0.7_1', '0.8_0', '0.8_1', '0.9_0', '0.9_1']
    check_records(records, want, [pckh[i // 2] for i in range(8)], inp['locations'])
    # a cuda locations tensor gives the same records
    del calls[:]
    again = pl.pseudo_label_round(torch.from_numpy(inp['locations']).to(cuda), inp['cams'], inp['gt2d'],
                                  inp['headsizes'], round_cfg(True))
    assert calls == ['posu_pseudo_label_sweep', 'posu_pckh_counts']
    for a, b in zip(again, records):
        assert a['name'] == b['name'] and a['pckh'] == b['pckh'] and a['vis_share'] == b['vis_share']
        assert np.array_equal(a['joints_vis'], b['joints_vis']) and np.array_equal(a['pseudo_2d'], b['pseudo_2d'])
    # without USE_REPROJ only the '_0' records; without ground truth the coverage stands and PCKh is nan
    cfg = round_cfg(True, use_reproj=False)
    plain = pl.pseudo_label_round(inp['locations'], inp['cams'], None, None, cfg)
    check_records(plain, rs.round_records(inp['locations'], thresholds, masks, proj, True, False), [None] * 4,
                  inp['locations'])
    assert all(np.isnan(r['pckh']) and np.isnan(r['ransac']['pckh']) for r in plain)
    # loop training: the single configured threshold
    loop = pl.pseudo_label_round(inp['locations'], inp['cams'], inp['gt2d'], inp['headsizes'],
                                 round_cfg(True, loop=True))
    check_records(loop, rs.round_records(inp['locations'], [0.6], masks[:1], proj[:1], True, True), [pckh[0]] * 2,
                  inp['locations'])


@pytest.mark.parametrize('name', ['g5_dist', 'g5_pin'])
@pytest.mark.parametrize('use_ransac', [True, False])
def test_round_with_given_thresholds_honours_the_config(cuda, golden, tmp_path, name, use_ransac):
    """Five groups with and without distortion (DATASET.NO_DISTORTION), IF_RANSAC on and off, and write_round."""
    from multiviews import pseudo_label as pl
    g = golden('pseudo_label.npz')
    ngroups, distortion, thresholds = rs.CASES[name]
    inp = case_inputs(name)
    masks, proj = case_stages(name, rs.GOLDEN_INLIERS, use_ransac)
    cfg = round_cfg(distortion, use_ransac=use_ransac)
    records = pl.pseudo_label_round(inp['locations'], inp['cams'], inp['gt2d'], inp['headsizes'], cfg,
                                    thresholds=thresholds)
    want = rs.round_records(inp['locations'], thresholds, masks, proj, use_ransac, True)
    pckh = [g[name + '_pckh'][i // 2] if use_ransac else None for i in range(2 * len(thresholds))]
    check_records(records, want, pckh, inp['locations'])
    if not use_ransac:      # stage 0 does not depend on RANSAC: its golden value holds here too
        assert [r['pckh'] for r in records[::2]] == g[name + '_pckh'][:, 0].tolist()
    names = [r['name'] for r in records]
    out = str(tmp_path)
    for loop in (False, True):
        cfg.PSEUDO_LABEL.IF_LOOP = loop
        seen = {}
        written, selected, deleted = pl.write_round(records, out, cfg, writer=seen.__setitem__)
        assert written == list(seen) == rs.files_written(names, out, loop, use_ransac)
        for r in records:
            p = pl.label_path(out, r['name'])
            if p in seen:
                assert seen[p]['pseudo_2d'] is r['pseudo_2d'] and seen[p]['joints_vis'] is r['joints_vis']
        if loop:
            assert selected is None and deleted is None
            continue
        sel, dele = pl.select_pseudo_labels(names, [r['pckh'] for r in records], [r['vis_share'] for r in records])
        assert sel and sorted(sel + dele) == sorted(names)
        assert open(os.path.join(out, 'select.txt')).read().split() == rs.files_written(sel, out, False, False)
        assert open(os.path.join(out, 'delete.txt')).read().split() == rs.files_written(dele, out, False, False)
        assert selected == rs.files_written(sel, out, False, False)


def test_round_refuses_what_it_cannot_compare(cuda):
    from multiviews import pseudo_label as pl
    inp = case_inputs('g5_dist')
    cfg = round_cfg(True)
    with pytest.raises(TypeError, match='float32'):
        pl.pseudo_label_round(inp['locations'].astype(np.float64), inp['cams'], inp['gt2d'], inp['headsizes'], cfg)
    with pytest.raises(ValueError, match='T'):
        pl.pseudo_label_round(inp['locations'], inp['cams'], inp['gt2d'], inp['headsizes'], cfg,
                              thresholds=[0.1 * i for i in range(9)])
    with pytest.raises(ValueError, match='groups'):
        pl.pseudo_label_round(inp['locations'][:-1], inp['cams'], inp['gt2d'], inp['headsizes'], cfg)
