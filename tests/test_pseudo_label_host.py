"""The pseudo-label round, host side: the three posu_* entry points are declared, exported and bound, the
workspace query and the argument checks answer before any launch, the Python layers refuse CPU tensors, and
the host parts (dominance filter, thresholds, file writing) equal the reference's recorded results
(tests/golden/pseudo_label.npz, made by make_pseudo_label_golden.py).  No kernel is launched here."""
import ctypes
import os
import re
import sys

import numpy as np
import pytest
import torch

import pseudo_label_restatement as rs
from oracle import geometry_ref as G
from posu import _native
from posu import synthetic as syn

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ('posu_pseudo_label_workspace', 'posu_pseudo_label_sweep', 'posu_pckh_counts')


def test_pseudo_label_symbols_are_declared_listed_and_exported():
    src = open(os.path.join(REPO, 'include', 'posu.h')).read()
    src = re.sub(r'/\*.*?\*/', '', src, flags=re.S)
    declared = set(re.findall(r'\b(posu_\w+)\s*\(', src))
    lib = _native.load()
    for name in SYMBOLS:
        assert name in declared, name
        assert name in _native.exported_symbols(), name
        assert hasattr(lib, name), name
    assert lib.posu_abi_version() == _native.ABI_VERSION == 16   # additive: the revision does not move


def test_workspace_query_answers_on_the_host():
    lib = _native.load()
    ws = lib.posu_pseudo_label_workspace
    t, g, v, j = 4, 2215, 4, 16
    proj, counts, masks = t * g * v * j * 2 * 8, t * 3 * (2 * j + v + 1) * 4, t * 3 * g * v * j
    assert ws(t, g, v, j) == proj + (counts + 7) // 8 * 8 + masks
    assert ws(1, 0, 2, 1) == (3 * 5 * 4 + 7) // 8 * 8           # no groups: the counts table alone
    assert ws(8, 1, 4, 1) > 0 and ws(1, 1, 3, 5) > 0
    for bad in ((0, 1, 4, 16), (9, 1, 4, 16), (4, 1, 1, 16), (4, 1, 5, 16), (4, 1, 4, 0), (4, -1, 4, 16)):
        assert ws(*bad) == -1, bad
    from posu import ops
    assert ops.pseudo_label_workspace(t, g, v, j) == ws(t, g, v, j)
    with pytest.raises(ValueError, match='T'):
        ops.pseudo_label_workspace(9, 1, 4, 16)


def test_argument_errors_are_reported_before_any_launch():
    lib = _native.load()
    p = ctypes.c_void_p(256)
    thre = (ctypes.c_float * 8)(*[0.6] * 8)
    host = ctypes.cast(thre, ctypes.c_void_p)

    def err(st, text):
        assert st == 1, st
        assert text in _native.last_error(), _native.last_error()

    def sweep(M=p, intr=p, xy=p, conf=p, th=host, T=4, G=2, V=4, J=16, inl=3, vis=p, proj=p):
        return lib.posu_pseudo_label_sweep(M, intr, xy, conf, th, T, G, V, J, 1, 10.0, inl, 1, vis, proj, None)
    for kw in ({'M': None}, {'intr': None}, {'xy': None}, {'conf': None}, {'th': None}, {'vis': None}, {'proj': None}):
        err(sweep(**kw), 'null pointer')
    for kw in ({'T': 0}, {'T': 9}, {'V': 1}, {'V': 5}, {'J': 0}, {'G': -1}):
        err(sweep(**kw), 'bad shape')
    err(sweep(inl=0), 'min_inliers')
    err(sweep(G=1 << 30, J=16), 'too large')
    assert sweep(G=0, M=None, xy=None, vis=None, proj=None) == 0          # no groups: OK, nothing launched

    sel = (ctypes.c_int * 4)(-1, -1, 0, 5)
    hsel = ctypes.cast(sel, ctypes.c_void_p)

    def cnt(pred=p, sets=None, sp=None, vis=p, gt=p, head=p, B=4, N=8, J=16, V=4, out=p):
        return lib.posu_pckh_counts(pred, sets, sp, vis, gt, head, B, N, J, V, 0.5, out, None)
    for kw in ({'out': None}, {'vis': None}, {'head': None}, {'pred': None}, {'sp': hsel}):
        err(cnt(**kw), 'null pointer')
    for kw in ({'B': 0}, {'B': 33}, {'N': -4}, {'N': 6}, {'J': 0}, {'V': 0}, {'V': 9}):
        err(cnt(**kw), 'bad shape')
    err(cnt(N=1 << 30, J=16), 'too large')


def test_python_layers_refuse_cpu_tensors():
    from multiviews import pseudo_label as pl
    from posu import ops
    g, v, j = 2, 4, 16
    M, intr = torch.zeros(g, v, 3, 4, dtype=torch.float64), torch.zeros(g, v, 9, dtype=torch.float64)
    xy, conf = torch.zeros(g, v, j, 2, dtype=torch.float64), torch.zeros(g, v, j)
    with pytest.raises(RuntimeError, match='cuda'):
        ops.pseudo_label_sweep(M, intr, xy, conf, [0.6])
    pred, vis, head = torch.zeros(g * v, j, 2), torch.ones(1, g * v, j, dtype=torch.uint8), torch.ones(g * v, 1)
    with pytest.raises(RuntimeError, match='cuda'):
        ops.pckh_counts(pred, vis, pred, head, v)
    with pytest.raises(RuntimeError, match='cuda'):
        pl.my_eval(pred, pred, vis[0], head)
    cfg = syn.make_cfg()
    with pytest.raises(RuntimeError, match='cuda'):
        pl.pseudo_label_round(torch.zeros(g * v, j, 3), syn.group_cameras(g), pred.numpy(), head.numpy(), cfg)


def test_round_runs_nowhere_without_a_device(monkeypatch):
    from multiviews import pseudo_label as pl
    monkeypatch.setattr(torch.cuda, 'is_available', lambda: False)
    with pytest.raises(RuntimeError, match='cuda'):
        pl.pseudo_label_round(np.zeros((8, 16, 3), np.float32), syn.group_cameras(2), np.zeros((8, 16, 2)),
                              np.ones((8, 1)), syn.make_cfg())
    with pytest.raises(RuntimeError, match='cuda'):
        pl.my_eval(np.zeros((8, 16, 2)), np.zeros((8, 16, 2)), np.ones((8, 16), bool), np.ones((8, 1)))


def test_thresholds_default_as_in_the_reference():
    from multiviews import pseudo_label as pl
    cfg = syn.make_cfg()
    assert pl.default_thresholds(cfg) == [0.6, 0.7, 0.8, 0.9]            # no IF_LOOP field: the config default
    cfg.PSEUDO_LABEL.IF_LOOP = False
    assert pl.default_thresholds(cfg) == [0.6, 0.7, 0.8, 0.9]
    cfg.PSEUDO_LABEL.IF_LOOP, cfg.PSEUDO_LABEL.CONFIDENCE_THRE = True, 0.75
    assert pl.default_thresholds(cfg) == [0.75]
    scales = np.array([[1.0, 1.5], [2.0, 0.5]])
    assert pl.headsizes_from_scales(scales).tolist() == [[30.0], [40.0]]


def test_selection_equals_the_reference(golden):
    from multiviews import pseudo_label as pl
    g = golden('pseudo_label.npz')
    for i, (acc, num) in enumerate(rs.SELECT_CASES):
        names = ['%s_%d' % (0.6 + 0.1 * (k // 2), k % 2) for k in range(len(acc))]
        final = g['sel_%d_final' % i].tolist()
        selected, deleted = pl.select_pseudo_labels(names, acc, num)
        assert selected == [names[k] for k in final], i
        assert deleted == [names[k] for k in range(len(names)) if k not in final], i
    assert g['sel_0_final'].tolist() == [3, 2, 1, 0]     # nothing dominates on a Pareto front
    assert g['sel_1_final'].tolist() == [3]              # a chain: the last set dominates the rest
    assert len(g['sel_2_final']) == 3                    # ties drop with their equals


def test_pckh_expression_on_counts_equals_the_reference(golden):
    """The host half of my_eval: the reference's expression on the integer sums the counts kernel produces
    (here taken in numpy from the golden's masks) gives the reference's value bit for bit, nan included."""
    from multiviews import pseudo_label as pl
    g = golden('pseudo_label.npz')
    for name, (ngroups, distortion, thresholds) in rs.CASES.items():
        inp = rs.make_inputs(rs.SEEDS[name], ngroups, distortion)
        assert float(inp['locations'].astype(np.float64).sum() + inp['gt2d'].sum()) == float(g[name + '_sum'])
        pred = inp['locations'][:, :, :2].astype(np.float64)
        for t in range(len(thresholds)):
            for s in range(3):
                c = rs.counts(g[name + '_proj'][t] if s == 2 else pred, inp['gt2d'], g[name + '_masks'][t, s],
                              inp['headsizes'])
                got = pl.pckh_from_counts(c[:16], c[16:32])
                assert got == g[name + '_pckh'][t, s] and type(got) is np.float64
    assert np.isnan(pl.pckh_from_counts([3, 0, 2], [4, 0, 5])) and np.isnan(g['nan_pckh'])


def test_general_view_ransac_of_the_restatement_is_the_oracles():
    ngroups, distortion, thresholds = rs.CASES['g5_dist']
    inp = rs.make_inputs(rs.SEEDS['g5_dist'], ngroups, distortion)
    p2d = inp['locations'][:, :, :2].astype(np.float64)
    err = rs.pair_table(p2d, inp['cams'], False)
    m0 = inp['locations'][:, :, 2] > 0.6
    for inl in rs.INLIERS:
        assert np.array_equal(rs.ransac_from_table(err, m0, rs.REPROJ_THRE, inl),
                              G.ransac(p2d, inp['cams'], m0, rs.REPROJ_THRE, inl, False))
    proj, res = rs.reproject_views(p2d, inp['cams'], m0, False, 4)
    ref_proj, ref_res = G.reproject_poses(p2d, inp['cams'], m0, False)
    assert np.array_equal(proj, ref_proj) and np.array_equal(res, ref_res)
    # the pinned confidences: float32(0.6) is above 0.6 in f64 and not in f32, where numpy compares
    conf = inp['locations'][:, :, 2]
    assert (conf == rs.F06).sum() == 4 and not (conf > 0.6)[conf == rs.F06].any()
    assert (conf.astype(np.float64) > 0.6)[conf == rs.F06].all()


def test_save_pseudo_label_needs_h5py_or_a_writer(tmp_path, monkeypatch):
    from multiviews import pseudo_label as pl
    monkeypatch.setitem(sys.modules, 'h5py', None)                # importing it raises ImportError
    with pytest.raises(ImportError, match='h5py'):
        pl.save_pseudo_label(str(tmp_path / 'x_pseudo_label.h5'), np.zeros((4, 16, 2)), np.ones((4, 16), bool))
    seen = []
    pl.save_pseudo_label('p', np.zeros((4, 16, 2)), np.ones((4, 16), bool), writer=lambda p, d: seen.append((p, d)))
    assert seen[0][0] == 'p' and sorted(seen[0][1]) == ['joints_vis', 'pseudo_2d']


def test_write_round_writes_the_references_files(tmp_path):
    from multiviews import pseudo_label as pl
    acc, num = rs.SELECT_CASES[2]
    names = ['0.6_0', '0.6_1', '0.7_0', '0.7_1', '0.8_0']
    records = [{'name': n, 'pckh': a, 'vis_share': s, 'pseudo_2d': np.zeros((4, 16, 2)),
                'joints_vis': np.ones((4, 16), bool)} for n, a, s in zip(names, acc, num)]
    cfg = syn.make_cfg()
    out = str(tmp_path)
    for loop, ransac in ((False, True), (True, True), (True, False)):
        cfg.PSEUDO_LABEL.IF_LOOP, cfg.PSEUDO_LABEL.IF_RANSAC = loop, ransac
        seen = []
        for f in ('select.txt', 'delete.txt'):
            if os.path.exists(os.path.join(out, f)):
                os.remove(os.path.join(out, f))
        written, selected, deleted = pl.write_round(records, out, cfg, writer=lambda p, d: seen.append(p))
        assert written == seen == rs.files_written(names, out, loop, ransac)
        if loop:
            assert selected is None and deleted is None and not os.path.exists(os.path.join(out, 'select.txt'))
            continue
        sel, dele = pl.select_pseudo_labels(names, acc, num)
        assert selected == rs.files_written(sel, out, False, False)
        assert open(os.path.join(out, 'select.txt')).read() == ''.join(p + '\n' for p in selected)
        assert open(os.path.join(out, 'delete.txt')).read() == ''.join(
            p + '\n' for p in rs.files_written(dele, out, False, False))
