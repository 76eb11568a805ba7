"""The device-resident validation epoch on the MI355X (csrc/validate.hip, core.function.validate_device):

* posu_decode_views against the reference goldens (flip.npz, decode.npz, train_loop.npz) and, bit for bit,
  against the unchanged chain ops.flip_back + ops.argmax2d + ops.pck_accuracy on seeded shapes and edge maps;
* posu_detection_counts against the fp64 numpy expression of each form on validate_eval.npz's inputs, and the
  two evaluations against the reference's tables;
* validate_batch_device / validate_device against validate_batch / validate: equal, not close (the same
  kernels in the same order), and no device read or synchronisation between two log lines.
"""
import itertools
import sys

import numpy as np
import pytest
import torch

from posu import metrics, ops, synthetic as syn
from test_gpu_train_loop import ACC_CASES, _Data, _ReadCounters, _offset_view
from test_gpu_validate import _FakeDataset, _FakeH5, _perm
from test_validate_device_host import assert_table, mapping_of

pytestmark = pytest.mark.gpu

SHAPES = [(4, 3, 16, 16, 16), (1, 1, 17, 12, 10), (8, 2, 5, 3, 5), (2, 2, 16, 96, 96)]   # (V, N, J, H, W)


def _host(t):
    return None if t is None else t.cpu().numpy()


# ------------------------------------------------------------------ the existing chain
def _chain(outs, flips, perm, shift, tgts, aff, post, thr=0.5):
    """What validate_batch does per view with the existing ops -> (merged [V*N, J, H, W], preds [V*N, J, 3],
    pck results or None), rows interleaved view-minor (preds[k::V] = view k)."""
    v, n = len(outs), outs[0].shape[0]
    merged = outs if flips is None else [ops.flip_back(f, perm, hm=o, shift=shift) for o, f in zip(outs, flips)]
    hm = torch.empty((v * n,) + tuple(outs[0].shape[1:]), dtype=torch.float32, device=outs[0].device)
    preds = torch.empty((v * n, outs[0].shape[1], 3), dtype=torch.float32, device=outs[0].device)
    for k, m in enumerate(merged):
        p, mv = ops.argmax2d(m, post_process=post, affine64=None if aff is None else aff[k * n:(k + 1) * n])
        hm[k::v] = m
        preds[k::v, :, :2] = p
        preds[k::v, :, 2:] = mv
    pck = None if tgts is None else ops.pck_accuracy(merged, tgts, thr)
    return hm, preds, pck


def _assert_same_as_chain(outs, flips, perm, shift, tgts, aff, post, with_merged, what):
    hm, preds, pck = _chain(outs, flips, perm, shift, tgts, aff, post)
    merged_out = torch.full_like(hm, 777.0) if with_merged else None
    p, m, acc, avg, cnt, step = ops.decode_views(outs, flipped=flips, perm=perm, shift=shift, targets=tgts,
                                                 affine64=aff, post_process=post, merged_out=merged_out)
    np.testing.assert_array_equal(_host(p), _host(preds), err_msg=what)
    if with_merged:
        assert m is merged_out
        np.testing.assert_array_equal(_host(m), _host(hm), err_msg=what)
    else:
        assert m is None
    if tgts is None:
        assert acc is None and avg is None and cnt is None and step is None
    else:
        for got, ref in zip((acc, avg, cnt, step), (pck[0], pck[1], pck[2], pck[4])):
            assert _host(got).tobytes() == _host(ref).tobytes(), what


@pytest.fixture(scope='module')
def seeded(cuda):
    """Per shape: outputs, mirrored outputs and targets (V lists), a joint permutation and affines, made once."""
    cases = {}
    for shape in SHAPES:
        v, n, j, h, w = shape
        g = torch.Generator().manual_seed(sum(shape))
        outs = [torch.randn(n, j, h, w, generator=g).to(cuda) for _ in range(v)]
        flips = [torch.randn(n, j, h, w, generator=g).to(cuda) for _ in range(v)]
        # targets: the output's own peak moved by up to one pixel, so that valid pairs, hits and misses occur
        tgts = []
        for o in outs:
            t = torch.rand(n, j, h, w, generator=g) * 0.5
            idx = o.flatten(2).argmax(dim=2).cpu()
            moved = (idx + torch.randint(0, 3, idx.shape, generator=g) - 1).clamp(0, h * w - 1)
            t.flatten(2).scatter_(2, moved.unsqueeze(2), 1.0)
            tgts.append(t.to(cuda))
        perm = torch.randperm(j, generator=g).to(torch.int32).to(cuda)
        aff = (torch.randn(v * n, 2, 3, generator=g, dtype=torch.float64) * 3).to(cuda)
        cases[shape] = (outs, flips, tgts, perm, aff)
    torch.cuda.synchronize()
    return cases


@pytest.mark.parametrize('shape', SHAPES, ids=lambda s: 'x'.join(map(str, s)))
def test_decode_views_equals_the_existing_chain(seeded, shape):
    outs, flips, tgts, perm, aff = seeded[shape]
    for use_flip, shift, use_tgt, with_merged in itertools.product((False, True), repeat=4):
        if shift and not use_flip:
            continue
        what = 'flip %s shift %s targets %s merged %s' % (use_flip, shift, use_tgt, with_merged)
        _assert_same_as_chain(outs, flips if use_flip else None, perm if use_flip else None, shift,
                              tgts if use_tgt else None, aff, True, with_merged, what)
    # no post-process, no affine: the plain argmax coordinates
    _assert_same_as_chain(outs, flips, perm, True, tgts, None, False, True, 'raw coordinates')


# ------------------------------------------------------------------ reference goldens
def test_flip_merge_matches_the_reference_golden(cuda, golden):
    """12 x 10 maps: W is not a multiple of 4, the 4-byte path."""
    g = golden('flip.npz')
    hm, hmf = torch.from_numpy(g['hm']).to(cuda), torch.from_numpy(g['hm_flipped']).to(cuda)
    perm = _perm(g['pairs'])
    for shift, key in ((True, 'avg_shift'), (False, 'avg_noshift')):
        # one view of three samples, then three views of one sample: the rows are n * V + v either way
        for outs, flips in (([hm], [hmf]), ([hm[k:k + 1] for k in range(3)], [hmf[k:k + 1] for k in range(3)])):
            merged = torch.empty_like(hm)
            ops.decode_views(outs, flipped=flips, perm=perm, shift=shift, merged_out=merged)
            np.testing.assert_array_equal(_host(merged), g[key])


def test_decode_matches_the_reference_golden_and_interleaves_the_views(cuda, golden):
    """decode.npz's six maps as V = 3 views of N = 2: row n * V + v of preds_out is map v * N + n.  Equal to the
    existing decode (ops.argmax2d) and to the golden."""
    g = golden('decode.npz')
    hm = torch.from_numpy(g['heatmaps']).to(cuda)
    T = torch.from_numpy(g['inv_affines']).to(cuda)
    views = [hm[2 * v:2 * v + 2] for v in range(3)]
    order = np.array([v * 2 + n for n in range(2) for v in range(3)])      # row n * 3 + v -> map v * 2 + n
    for post, key in ((True, 'final_preds'), (False, 'final_preds_nopost')):
        p, _, _, _, _, _ = ops.decode_views(views, affine64=T, post_process=post)
        p = _host(p)
        ref_p, ref_v = ops.argmax2d(hm, post_process=post, affine64=T)
        np.testing.assert_array_equal(p[:, :, :2], _host(ref_p)[order])
        np.testing.assert_array_equal(p[:, :, 2:], _host(ref_v)[order])
        print(key, 'max |diff| vs golden', np.abs(p[:, :, :2] - g[key][order]).max())
        np.testing.assert_array_equal(p[:, :, :2], g[key][order])
        np.testing.assert_array_equal(p[:, :, 2:], g['final_vals'][order])
    raw, _, _, _, _, _ = ops.decode_views(views, post_process=False)
    np.testing.assert_array_equal(_host(raw)[:, :, :2], g['max_preds'][order])


@pytest.mark.parametrize('name', ACC_CASES)
def test_accuracy_matches_the_reference_golden(cuda, golden, name):
    g = golden('train_loop.npz')
    out = torch.from_numpy(g['acc.%s.output' % name]).to(cuda)
    tgt = torch.from_numpy(g['acc.%s.target' % name]).to(cuda)
    p, _, acc, avg, cnt, step = [_host(x) for x in ops.decode_views([out], targets=[tgt], post_process=False)]
    assert np.array_equal(acc[0], g['acc.%s.acc' % name])
    assert avg[0] == float(g['acc.%s.avg' % name]) and cnt[0] == int(g['acc.%s.cnt' % name])
    assert np.array_equal(p[:, :, :2], g['acc.%s.pred' % name])
    assert step[0] == avg[0] and step[1] == float(cnt[0])


def test_accuracy_cases_as_views_of_one_call(cuda, golden):
    """The cases of one shape as the views of one call: every view is its own row."""
    g = golden('train_loop.npz')
    names = [n for n in ACC_CASES if g['acc.%s.output' % n].shape == g['acc.d.output'].shape]
    assert len(names) >= 1
    names = (names * 3)[:3]
    outs = [torch.from_numpy(g['acc.%s.output' % n]).to(cuda) for n in names]
    tgts = [torch.from_numpy(g['acc.%s.target' % n]).to(cuda) for n in names]
    _, _, acc, avg, cnt, step = [_host(x) for x in ops.decode_views(outs, targets=tgts)]
    for k, n in enumerate(names):
        assert np.array_equal(acc[k], g['acc.%s.acc' % n]) and avg[k] == float(g['acc.%s.avg' % n])
        assert cnt[k] == int(g['acc.%s.cnt' % n])
    assert step[0] == np.mean(avg) and step[1] == np.mean(cnt.astype(np.float64))


# ------------------------------------------------------------------ edge maps
def _edge_maps(h, w):
    """[1, 9, h, w]: constant, all-negative, a maximum on each border, all -inf, column 0 next to the border
    (the merged maximum of the shifted flip test), an interior maximum."""
    r = np.random.default_rng(5)
    m = (r.random((1, 9, h, w)) * 0.1).astype(np.float32)
    m[0, 0] = 0.5
    m[0, 1] = -1.0 - r.random((h, w))
    m[0, 2, 0, 3] = 2.0            # top
    m[0, 3, h - 1, 4] = 2.0        # bottom
    m[0, 4, 3, 0] = 2.0            # left
    m[0, 5, 2, w - 1] = 2.0        # right
    m[0, 6] = -np.inf
    m[0, 7, 4, 1] = 2.0            # ix = 1: no quarter-pixel shift
    m[0, 8, 3, 4] = 2.0
    m[0, 8, 3, 5] = 1.0            # interior: +0.25 in x
    m[0, 8, 2, 4] = 1.5            # and -0.25 in y
    return m


@pytest.mark.parametrize('h,w', [(8, 8), (7, 9)])
def test_edge_maps(cuda, h, w):
    maps = _edge_maps(h, w)
    o = torch.from_numpy(maps).to(cuda)
    off = _offset_view(o)                       # a view whose storage starts 1 float past a 16-byte boundary
    p, m, _, _, _, _ = ops.decode_views([o, off], post_process=True,
                                        merged_out=torch.empty(2, 9, h, w, device=cuda))
    p, m = _host(p), _host(m)
    np.testing.assert_array_equal(p[0], p[1])   # the aligned and the offset view agree
    np.testing.assert_array_equal(m[0], maps[0])
    np.testing.assert_array_equal(m[1], maps[0])
    want = {0: (0, 0, 0.5), 1: (0, 0, maps[0, 1].max()), 2: (3, 0, 2.0), 3: (4, h - 1, 2.0), 4: (0, 3, 2.0),
            5: (w - 1, 2, 2.0), 6: (0, 0, -np.inf), 7: (1, 4, 2.0), 8: (4.25, 2.75, 2.0)}
    for j, (x, y, v) in want.items():
        assert tuple(p[0, j]) == (np.float32(x), np.float32(y), np.float32(v)), (j, p[0, j])
    # the same maps through the flip test (mirrored inputs with their own edge maps), shift on and off, with and
    # without targets, aligned and offset: equal to the chain
    f = torch.from_numpy(np.ascontiguousarray(maps[:, ::-1, :, ::-1])).to(cuda)
    t = torch.from_numpy(np.ascontiguousarray(maps[:, :, ::-1])).to(cuda)
    perm = torch.tensor([8, 7, 6, 5, 4, 3, 2, 1, 0], dtype=torch.int32, device=cuda)
    for shift, use_tgt, with_merged in itertools.product((False, True), repeat=3):
        _assert_same_as_chain([o, off], [f, _offset_view(f)], perm, shift, [t, _offset_view(t)] if use_tgt else None,
                              None, True, with_merged, 'edge maps shift %s' % shift)
    # column 0 with shift: flipped column W - 1 lands on column 0 twice (x = 0 and x = 1 read the same source)
    z = torch.zeros(1, 1, h, w, device=cuda)
    fl = torch.zeros(1, 1, h, w, device=cuda)
    fl[0, 0, 3, w - 1] = 4.0
    p, _, _, _, _, _ = ops.decode_views([z], flipped=[fl], shift=True)
    assert tuple(_host(p)[0, 0]) == (0.0, 3.0, 2.0)


def test_an_empty_batch_launches_nothing(cuda):
    buf = torch.full((3, 4, 3), 777.0, device=cuda)
    p, m, acc, _, _, _ = ops.decode_views([torch.zeros(0, 4, 8, 8, device=cuda)] * 2, preds_out=buf, row0=3)
    assert p is buf and m is None and acc is None
    assert bool((_host(buf) == 777.0).all())
    p, _, _, _, _, _ = ops.decode_views([torch.zeros(0, 4, 8, 8, device=cuda)])
    assert tuple(p.shape) == (0, 4, 3)


@pytest.mark.parametrize('shape', [(4, 3, 16, 16, 16), (1, 1, 17, 12, 10)], ids=lambda s: 'x'.join(map(str, s)))
def test_row0_writes_its_rows_and_no_other(cuda, seeded, shape):
    outs, flips, tgts, perm, aff = seeded[shape]
    v, n, j, h, w = shape
    hm, preds, _ = _chain(outs, flips, perm, True, None, aff, True)
    rows, row0 = v * n + 5, 3
    pbuf = torch.full((rows, j, 3), 777.0, device=cuda)
    mbuf = torch.full((rows, j, h, w), 777.0, device=cuda)
    ops.decode_views(outs, flipped=flips, perm=perm, shift=True, affine64=aff, preds_out=pbuf, merged_out=mbuf,
                     row0=row0)
    pbuf, mbuf = _host(pbuf), _host(mbuf)
    np.testing.assert_array_equal(pbuf[row0:row0 + v * n], _host(preds))
    np.testing.assert_array_equal(mbuf[row0:row0 + v * n], _host(hm))
    for buf in (pbuf, mbuf):
        assert bool((buf[:row0] == 777.0).all()) and bool((buf[row0 + v * n:] == 777.0).all())
    # rows that do not fit are refused before the launch
    with pytest.raises(RuntimeError, match='do not fit'):
        ops.decode_views(outs, preds_out=torch.empty((rows, j, 3), device=cuda), row0=6)
    with pytest.raises(RuntimeError, match='do not fit'):
        ops.decode_views(outs, preds_out=torch.empty((rows, j, 3), device=cuda),
                         merged_out=torch.empty((v * n, j, h, w), device=cuda), row0=1)


# ------------------------------------------------------------------ detection counts and the evaluations
def _golden_inputs(g, prefix):
    u2a, joints = mapping_of(g, prefix)
    u, _ = metrics.u2a_indices(u2a)
    head = np.amax(g['h36m.scales'], axis=1) * 200 / 10.0 if prefix == 'h36m' else g['mpii.headsizes']
    vis = None if prefix == 'h36m' else g['mpii.joints_vis'][:, u, 0]
    return u2a, joints, g[prefix + '.pred'], g[prefix + '.gt'][:, u], head, vis


@pytest.mark.parametrize('prefix', ['h36m', 'mpii'])
@pytest.mark.parametrize('form', [0, 1])
def test_detection_counts_equal_the_numpy_expression(cuda, golden, prefix, form):
    g = golden('validate_eval.npz')
    _, _, pred, gt, head, vis = _golden_inputs(g, prefix)
    want = g['%s.counts_form%d' % (prefix, form)]
    dev = [None if x is None else torch.from_numpy(np.ascontiguousarray(x)).to(cuda) for x in (pred, gt, head, vis)]
    five = _host(ops.detection_counts(dev[0], dev[1], dev[2], g['thresholds'], form=form, vis=dev[3]))
    print(prefix, form, five[:, 0].tolist())
    assert five.dtype == np.int32 and np.array_equal(five, want)
    one = _host(ops.detection_counts(dev[0], dev[1], dev[2], [0.5], form=form, vis=dev[3]))
    assert np.array_equal(one, want[:1])
    # [N, J, 2] predictions read the same x and y
    two = _host(ops.detection_counts(dev[0][:, :, :2].contiguous(), dev[1], dev[2], g['thresholds'], form=form,
                                     vis=dev[3]))
    assert np.array_equal(two, want)
    empty = _host(ops.detection_counts(dev[0][:0], dev[1][:0], dev[2][:0], [0.5, 0.4], form=form))
    assert empty.shape == (2, 2, pred.shape[1]) and not empty.any()


def test_the_evaluations_are_the_reference_tables(cuda, golden):
    g = golden('validate_eval.npz')
    u2a, joints = mapping_of(g, 'h36m')
    for to in (lambda x: x, lambda x: torch.from_numpy(x).to(cuda)):           # numpy in, cuda in
        name_values, perf = metrics.evaluate_h36m(to(g['h36m.pred']), to(g['h36m.gt']), to(g['h36m.scales']), u2a,
                                                  joints)
        assert_table(name_values, perf, g, 'h36m')
    u2a, joints = mapping_of(g, 'mpii')
    for to in (lambda x: x, lambda x: torch.from_numpy(x).to(cuda)):
        name_values, perf = metrics.evaluate_mpii(to(g['mpii.pred']), to(g['mpii.gt']), to(g['mpii.joints_vis']),
                                                  to(g['mpii.headsizes']), u2a, joints)
        assert_table(name_values, perf, g, 'mpii')


# ------------------------------------------------------------------ the loop
def _r18(cuda, cfg, seed):
    from models.multiview_pose_resnet import get_multiview_pose_net
    from models.pose_resnet import get_pose_net
    net = get_pose_net(cfg, is_train=False, precision='fp32')
    net.load_state_dict(syn.synthetic_state_dict(net.state_dict(), seed=seed))
    return get_multiview_pose_net(net.to(cuda).eval(), cfg).to(cuda)


def _batch(rng, nb, sources=None):
    views = [torch.from_numpy(rng.standard_normal((nb, 3, 64, 64)).astype(np.float32)) for _ in range(4)]
    target = [torch.from_numpy(rng.random((nb, 16, 16, 16)).astype(np.float32)) for _ in range(4)]
    weight = [torch.from_numpy((rng.random((nb, 16, 1)) > 0.2).astype(np.float32)) for _ in range(4)]
    meta = [{'center': torch.from_numpy(rng.uniform(100, 900, (nb, 2))),
             'scale': torch.from_numpy(rng.uniform(1, 3, (nb, 2))), 'source': list(sources or ['h36m'] * nb)}
            for _ in range(4)]
    return views, target, weight, meta


def _criteria():
    from core.loss import JointsMSELoss
    return {'mse_weights': JointsMSELoss(use_target_weight=True)}


def _compare_batch(cuda, cfg, model, batch, flip_pairs):
    from core.function import validate_batch, validate_batch_device
    views, target, weight, meta = batch
    views = [v.to(cuda) for v in views]
    n = views[0].shape[0]
    ref = validate_batch(cfg, model, views, target, weight, meta, flip_pairs=flip_pairs, criterion_dict=_criteria())
    preds = torch.full((4 * n + 2, 16, 3), 777.0, device=cuda)
    hms = torch.full((4 * n + 2, 16, 16, 16), 777.0, device=cuda)
    got = validate_batch_device(cfg, model, views, target, weight, meta, flip_pairs, _criteria(), preds, hms, 1)
    assert got['rows'] == 4 * n
    assert all(isinstance(got[k], torch.Tensor) and got[k].is_cuda for k in ('loss', 'acc', 'cnt', 'acc_table'))
    assert got['loss'].dim() == 0 and got['acc'].dim() == 0 and got['cnt'].dim() == 0
    np.testing.assert_array_equal(_host(preds)[1:1 + 4 * n], ref['preds'])
    np.testing.assert_array_equal(_host(hms)[1:1 + 4 * n], ref['heatmaps'])
    assert bool((_host(preds)[[0, -1]] == 777.0).all()) and bool((_host(hms)[[0, -1]] == 777.0).all())
    print('loss', float(got['loss']), ref['loss'], 'acc', float(got['acc']), ref['acc'], 'cnt', float(got['cnt']))
    assert float(got['loss']) == ref['loss']
    assert float(got['acc']) == ref['acc'] and float(got['cnt']) == ref['cnt']
    return got, ref


@pytest.mark.parametrize('flip', [False, True])
def test_validate_batch_device_equals_validate_batch(cuda, flip):
    cfg = syn.make_cfg(num_layers=18, image_size=64, flip_test=flip, shift_heatmap=flip)
    model = _r18(cuda, cfg, seed=4)
    _compare_batch(cuda, cfg, model, _batch(np.random.default_rng(1), 2), _FakeDataset.flip_pairs)


def test_validate_batch_device_aggre_loss_terms(cuda):
    """AGGRE + FUSE_OUTPUT + the consistent loss + the pseudo-label loss (test_gpu_validate.py's case), N = 3 with
    one 'mpii' sample: the H36M rows chosen on the host give the loss of the boolean-mask selection."""
    cfg = syn.make_cfg(num_layers=18, image_size=64)
    cfg.NETWORK.AGGRE = True
    cfg.TEST.FUSE_OUTPUT = True
    cfg.LOSS.USE_CONSISTENT_LOSS = True
    cfg.LOSS.MSE_LOSS_WEIGHT = 0.7
    cfg.DATASET.PSEUDO_LABEL_PATH = 'pseudo.pkl'
    torch.manual_seed(3)   # the Aggregation weights are drawn from torch's generator
    model = _r18(cuda, cfg, seed=2)
    got, ref = _compare_batch(cuda, cfg, model, _batch(np.random.default_rng(2), 3, ['h36m', 'mpii', 'h36m']), None)
    assert np.isfinite(ref['loss'])


@pytest.fixture(scope='module')
def epoch(cuda):
    """validate() once over the two-batch loader (3 then 2 groups) of test_gpu_validate.py, flip test on: what it
    hands to the h5 writer and to dataset.evaluate, shared by the tests below and left unchanged."""
    from core import function as fn
    cfg = syn.make_cfg(num_layers=18, image_size=64, flip_test=True, shift_heatmap=True)
    cfg.PRINT_FREQ = 100
    model = _r18(cuda, cfg, seed=4)
    rng = np.random.default_rng(0)
    loader = [_batch(rng, nb) for nb in (3, 2)]
    fake, ds = _FakeH5(), _FakeDataset(ngroups=5)
    saved = sys.modules.get('h5py')
    sys.modules['h5py'] = fake
    try:
        perf = fn.validate(cfg, loader, ds, {'base_model': model}, _criteria(), 'out', None, 0)
    finally:
        if saved is None:
            del sys.modules['h5py']
        else:
            sys.modules['h5py'] = saved
    (name, rec), = fake.files.items()
    return {'cfg': cfg, 'model': model, 'loader': loader, 'perf': perf, 'file': name, 'rec': rec,
            'evaluated': ds.evaluated}


def test_validate_device_hands_over_what_validate_does(cuda, monkeypatch, epoch):
    from core import function as fn
    fake, ds = _FakeH5(), _FakeDataset(ngroups=5)
    monkeypatch.setitem(sys.modules, 'h5py', fake)
    res = fn.validate_device(epoch['cfg'], epoch['loader'], ds, {'base_model': epoch['model']}, _criteria(), 'out',
                             None, 0)
    assert res.perf_indicator == epoch['perf'] == 0.5 and res.name_values == {'mpjpe': 1.0}
    (name, rec), = fake.files.items()
    assert name == epoch['file'] and rec['mode'] == 'w'
    for key in ('heatmaps', 'locations', 'joint_names_order'):
        np.testing.assert_array_equal(rec[key], epoch['rec'][key], err_msg=key)
    np.testing.assert_array_equal(ds.evaluated, epoch['evaluated'])
    np.testing.assert_array_equal(res.u, epoch['rec']['joint_names_order'])
    assert res.locations.is_cuda and tuple(res.locations.shape) == (20, 16, 3)
    assert res.heatmaps.is_cuda and tuple(res.heatmaps.shape) == (20, 16, 16, 16)
    np.testing.assert_array_equal(_host(res.locations)[:, res.u], epoch['rec']['locations'])
    np.testing.assert_array_equal(_host(res.heatmaps)[:, res.u], epoch['rec']['heatmaps'])
    assert res.meters['loss']['count'] == 20 and 0.0 <= res.meters['acc']['avg'] <= 1.0


def test_validate_device_without_heatmaps_feeds_the_pseudo_label_round(cuda, monkeypatch, epoch):
    from core import function as fn
    from multiviews import pseudo_label as pl
    fake, ds = _FakeH5(), _FakeDataset(ngroups=5)
    monkeypatch.setitem(sys.modules, 'h5py', fake)
    res = fn.validate_device(epoch['cfg'], epoch['loader'], ds, {'base_model': epoch['model']}, _criteria(), 'out',
                             None, 0, keep_heatmaps=False)
    assert fake.files == {} and res.heatmaps is None and res.perf_indicator == 0.5
    np.testing.assert_array_equal(ds.evaluated, epoch['evaluated'])
    locations = res.locations[:, res.u]
    assert locations.is_cuda and locations.dtype == torch.float32
    host = np.ascontiguousarray(epoch['evaluated'])          # the host path's all_preds[:, u]
    cfg = syn.make_cfg()
    cfg.PSEUDO_LABEL.USE_REPROJ = True
    cfg.PSEUDO_LABEL.NUM_INLIERS, cfg.PSEUDO_LABEL.REPROJ_THRE = 2, 1e4
    cfg.PSEUDO_LABEL.IF_LOOP = False
    cams = syn.group_cameras(5)
    thresholds = [float(q) for q in np.quantile(host[:, :, 2], [0.25, 0.5, 0.75])]   # some joints on, some off
    got = pl.pseudo_label_round(locations, cams, None, None, cfg, thresholds=thresholds)
    want = pl.pseudo_label_round(host, cams, None, None, cfg, thresholds=thresholds)
    assert [r['name'] for r in got] == [r['name'] for r in want] and len(got) == 6
    masks = [r['joints_vis'].mean() for r in want]
    assert 0.0 < min(masks[0::2]) and max(masks[0::2]) < 1.0
    for a, b in zip(got, want):
        assert np.array_equal(a['joints_vis'], b['joints_vis']) and np.array_equal(a['pseudo_2d'], b['pseudo_2d'])
        assert np.array_equal(a['joints_at'], b['joints_at']) and a['vis_share'] == b['vis_share']


def test_validate_device_reads_nothing_between_log_lines(cuda, monkeypatch, epoch):
    """Three batches with PRINT_FREQ larger than the loader; the counters are armed from batch 1 until the loader
    is exhausted (before the final read of the meters and of the results)."""
    from core import function as fn
    fake, ds = _FakeH5(), _FakeDataset(ngroups=8)
    monkeypatch.setitem(sys.modules, 'h5py', fake)
    counters = _ReadCounters(monkeypatch)
    rng = np.random.default_rng(7)
    data = _Data(list(epoch['loader']) + [_batch(rng, 3)], counters)
    res = fn.validate_device(epoch['cfg'], data, ds, {'base_model': epoch['model']}, _criteria(), 'out', None, 0)
    torch.cuda.synchronize()
    assert counters.calls == []
    assert res.meters['loss']['count'] == 32


def test_validate_batch_device_reads_nothing(cuda, monkeypatch, epoch):
    from core.function import validate_batch_device
    views, target, weight, meta = epoch['loader'][0]
    views = [v.to(cuda) for v in views]
    preds = torch.zeros((12, 16, 3), device=cuda)
    hms = torch.zeros((12, 16, 16, 16), device=cuda)
    args = (epoch['cfg'], epoch['model'], views, target, weight, meta, _FakeDataset.flip_pairs, _criteria())
    validate_batch_device(*args, preds, hms, 0)      # the first call builds what later calls reuse
    counters = _ReadCounters(monkeypatch)
    counters.armed = True
    got = validate_batch_device(*args, preds, None, 0)
    counters.armed = False
    assert counters.calls == []
    assert float(got['loss']) > 0.0
