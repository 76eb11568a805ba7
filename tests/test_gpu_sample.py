"""The training sample on the device (csrc/sample.hip): posu_sample_images against the restatement
(tests/sample_restatement.py, pinned against PIL and the reference by tests/test_sample_host.py) exactly,
posu_sample_joints_targets and BatchMaker.multiview against the reference's recorded __getitem__ results
(tests/golden/sample_batch.npz) bit for bit, and one core.function.train step on such a batch."""
import itertools

import numpy as np
import pytest
import torch

import sample_restatement as rs
from oracle import geometry_ref as G
from posu import datapath, optim, synthetic as syn

pytestmark = pytest.mark.gpu

SIZE = (32, 24)     # (w, h): a non-square crop


def _img(h, w, seed):
    return np.random.default_rng(seed).integers(0, 256, (h, w, 3), dtype=np.uint8)


def _trans(center, scale, rot, size=SIZE):
    from utils.transforms import get_affine_transform
    return get_affine_transform(np.array(center, dtype=np.float64), np.array([scale, scale]), rot, list(size))


def _jit(order, b, c, s, shift, active=True):
    return {'order': list(order), 'brightness': b, 'contrast': c, 'saturation': s, 'hue_shift': shift,
            'active': active}


def _records_of(jitters):
    rec = datapath.jitter_records(len(jitters))
    for k, j in enumerate(jitters):
        rec['order'][k] = j['order']
        rec['brightness'][k], rec['contrast'][k], rec['saturation'][k] = j['brightness'], j['contrast'], j['saturation']
        rec['hue_shift'][k], rec['active'][k] = j['hue_shift'], j['active']
    return rec


@pytest.fixture(scope='module')
def image_case():
    """Eight records over two sources of different sizes and a constant one; the restatement's crops, computed
    once.  Flip on and off, rotated and not, a crop partly and one wholly outside its source, the grey branch of
    the hue, contrast factors inside [0, 1] and above 1, hue shifts > 0, 0 and < 0 (231), jitter inactive next
    to active."""
    a, b = _img(37, 53, 1), _img(64, 48, 2)
    grey = np.full((40, 40, 3), 90, dtype=np.uint8)
    cases = [
        (a, False, _trans((26, 18), 0.2, 0.0), _jit((0, 1, 2, 3), 1.4, 0.6, 1.5, 30)),
        (a, True, _trans((20, 20), 0.15, 25.0), _jit((3, 2, 1, 0), 0.8, 1.7, 0.7, 0)),
        (b, True, _trans((24, 30), 0.3, 0.0), _jit((0, 1, 2, 3), 2.0, 2.0, 2.0, 9, active=False)),
        (b, False, _trans((30, 40), 0.25, -40.0), _jit((1, 3, 0, 2), 2.9, 1.0, 0.5, 231)),
        (a, False, _trans((50, 2), 0.2, 10.0), _jit((2, 0, 3, 1), 0.7, 0.5, 2.0, 206)),       # partly outside
        (b, True, _trans((400, -300), 0.2, 0.0), _jit((1, 0, 2, 3), 1.2, 1.5, 1.1, 3)),       # wholly outside
        (grey, False, _trans((20, 20), 0.1, 15.0), _jit((3, 1, 2, 0), 1.1, 0.9, 1.8, 128)),   # H = S = 0
        (a, True, _trans((0, 36), 0.25, 0.0), _jit((0, 1, 2, 3), 1.0, 1.0, 1.0, 0, active=False)),
    ]
    ref = [rs.sample_image_u8(img, flip, trans, SIZE, jit if jit['active'] else None) for img, flip, trans, jit in cases]
    plain = [G.warp_affine_linear(cases[k][0], cases[k][2], SIZE) for k in (4, 5)]
    assert plain[0].any() and (plain[0] == 0).all(-1).any() and not plain[1].any()
    return {'images': [c[0] for c in cases], 'flip': np.array([c[1] for c in cases]),
            'trans': np.stack([c[2] for c in cases]), 'jitter': _records_of([c[3] for c in cases]),
            'u8': np.stack([r[0] for r in ref]), 'l_sum': [r[1] for r in ref]}


@pytest.mark.parametrize('out', ['u8', 'f32'])
def test_sample_images_equals_the_restatement(cuda, image_case, out):
    c = image_case
    got, ws = datapath.sample_images(c['images'], c['trans'], SIZE, cuda, flip=c['flip'], jitter=c['jitter'], out=out,
                                     return_workspace=True)
    got = got.cpu().numpy()
    for k in range(len(c['images'])):
        if out == 'u8':
            np.testing.assert_array_equal(got[k], c['u8'][k], err_msg='record %d' % k)
        else:
            ref = G.to_tensor_normalize(c['u8'][k], datapath.IMAGENET_MEAN, datapath.IMAGENET_STD)
            assert got[k].tobytes() == ref.tobytes(), k
    # the contrast pre-pass: every active record's exact integer sum of L, 0 for the inactive ones
    assert ws.cpu().tolist() == [0 if s is None else s for s in c['l_sum']]


def test_sample_images_without_jitter_is_the_flipped_crop(cuda, image_case):
    c = image_case
    got = datapath.sample_images(c['images'], c['trans'], SIZE, cuda, flip=c['flip'], out='u8').cpu().numpy()
    for k, (img, flip, trans) in enumerate(zip(c['images'], c['flip'], c['trans'])):
        np.testing.assert_array_equal(got[k], rs.sample_image_u8(img, flip, trans, SIZE)[0], err_msg='record %d' % k)
    # no flip array at all, and RGB sources (the jitter is not symmetric in the channels)
    rgb = datapath.sample_images(c['images'][:2], c['trans'][:2], SIZE, cuda, jitter=c['jitter'][:2], bgr=False,
                                 out='u8').cpu().numpy()
    for k in range(2):
        j = c['jitter'][k]
        jit = _jit(j['order'].tolist(), float(j['brightness']), float(j['contrast']), float(j['saturation']),
                   int(j['hue_shift']))
        np.testing.assert_array_equal(rgb[k], rs.sample_image_u8(c['images'][k], False, c['trans'][k], SIZE, jit,
                                                                 bgr=False)[0])
    assert not np.array_equal(rgb[0], c['u8'][0])


def test_all_24_orders_in_one_call(cuda):
    """24 records of 16 x 12 crops, one per order of the four operations: the order is per record."""
    orders = list(itertools.permutations(range(4)))
    imgs = [_img(37, 53, 40), _img(64, 48, 41)]
    images = [imgs[k % 2] for k in range(24)]
    r = np.random.default_rng(42)
    trans = np.stack([_trans((r.uniform(10, 40), r.uniform(10, 30)), r.uniform(0.1, 0.3), r.uniform(-30, 30), (16, 12))
                      for _ in range(24)])
    flip = r.uniform(size=24) < 0.5
    jit = [_jit(o, float(np.float32(r.uniform(0.7, 3.0))), float(np.float32(r.uniform(0.5, 2.0))),
                float(np.float32(r.uniform(0.5, 2.0))), int(r.integers(0, 256))) for o in orders]
    got, ws = datapath.sample_images(images, trans, (16, 12), cuda, flip=flip, jitter=_records_of(jit), out='u8',
                                     return_workspace=True)
    got, ws = got.cpu().numpy(), ws.cpu().tolist()
    results = set()
    for k in range(24):
        ref, l_sum = rs.sample_image_u8(images[k], flip[k], trans[k], (16, 12), jit[k])
        np.testing.assert_array_equal(got[k], ref, err_msg='order %s' % (orders[k],))
        assert ws[k] == l_sum
        results.add(ref.tobytes())
    assert len(results) == 24


def test_contrast_sum_over_several_blocks(cuda):
    """A 64 x 48 crop is 12 blocks: the workspace holds the restatement's integer sum of L, taken after the
    brightness and hue steps that precede the contrast step."""
    img = _img(64, 48, 50)
    trans = _trans((24, 32), 0.3, 5.0, (64, 48))[None]
    jit = _jit((0, 3, 1, 2), 1.3, 1.6, 0.9, 77)
    got, ws = datapath.sample_images([img], trans, (64, 48), cuda, jitter=_records_of([jit]), out='u8',
                                     return_workspace=True)
    ref, l_sum = rs.sample_image_u8(img, False, trans[0], (64, 48), jit)
    assert ws.dtype == torch.int64 and ws.cpu().tolist() == [l_sum] and l_sum > 64 * 48
    np.testing.assert_array_equal(got.cpu().numpy()[0], ref)


@pytest.mark.parametrize('out', ['u8', 'f32'])
def test_crop_warp_is_unchanged_on_the_same_inputs(cuda, image_case, out):
    """posu_crop_warp shares the warp's device function with posu_sample_images: still the oracle's crop."""
    c = image_case
    got = datapath.crop_warp(c['images'], c['trans'], SIZE, cuda, out=out).cpu().numpy()
    for k, (img, trans) in enumerate(zip(c['images'], c['trans'])):
        ref = G.warp_affine_linear(img, trans, SIZE)
        if out == 'f32':
            ref = G.to_tensor_normalize(ref, datapath.IMAGENET_MEAN, datapath.IMAGENET_STD)
        assert got[k].tobytes() == ref.tobytes(), k


# ------------------------------------------------------------------ joints / targets
def test_joints_and_targets_equal_the_reference(cuda, golden):
    """The golden's label cases (J = 16, the union flip pairs, maps 24 x 32): flipped and rotated records, exactly
    one visible joint (the reference's .squeeze() case) with and without a flip, none visible, a joint whose
    joint / stride + 0.5 is below an integer in f64 and on it in f32, patches touching and missing each border,
    zero_weight."""
    from utils.transforms import flip_pair_order
    g = golden('sample_batch.npz')
    n = len(g['lab.db_source'])
    trans = np.stack([rs.golden_trans(g, 'lab', k, int(g['lab.width'][k]), rs.LAB['image_size'])[2] for k in range(n)])
    joints = torch.from_numpy(g['lab.db_joints_2d']).to(cuda)
    vis = torch.from_numpy(g['lab.db_joints_vis']).to(cuda)
    j2d, jvis, target, weight = datapath.sample_joints_targets(
        joints, vis, trans, rs.LAB['image_size'], rs.LAB['heatmap_size'], rs.LAB['sigma'], flip=g['lab.flip'],
        widths=g['lab.width'], flip_order=flip_pair_order(16, rs.UNION_FLIP_PAIRS),
        zero_weight=g['lab.db_source'] == 'h36m')
    assert j2d.dtype == jvis.dtype == torch.float64 and target.dtype == weight.dtype == torch.float32
    assert target.shape == (n, 16, 32, 24) and weight.shape == (n, 16, 1)
    j2d, jvis = j2d.cpu().numpy(), jvis.cpu().numpy()
    for k in range(n):
        bad = np.flatnonzero((j2d[k] != g['lab.joints_2d_transformed'][k]).any(-1))
        assert bad.size == 0, (k, bad, j2d[k][bad], g['lab.joints_2d_transformed'][k][bad])
        assert np.array_equal(jvis[k], g['lab.joints_vis'][k]), k
    assert target.cpu().numpy().tobytes() == g['lab.target'].tobytes()
    assert weight.cpu().numpy().tobytes() == g['lab.weight'].tobytes()
    # without a flip array nothing is mirrored: the unflipped records give the same rows
    keep = np.flatnonzero(~g['lab.flip'])
    j2, _, t2, w2 = datapath.sample_joints_targets(joints[keep], vis[keep], trans[keep], rs.LAB['image_size'],
                                                   rs.LAB['heatmap_size'], rs.LAB['sigma'],
                                                   zero_weight=(g['lab.db_source'] == 'h36m')[keep])
    assert np.array_equal(j2.cpu().numpy(), j2d[keep]) and torch.equal(t2, target[keep]) and torch.equal(w2, weight[keep])


# ------------------------------------------------------------------ BatchMaker
def _golden_batch(g):
    records = rs.golden_records(g, 'mv')
    images = [g['mv.image_%d' % k] for k in range(8)]
    jitter = _records_of([dict(j, active=True) for j in rs.golden_jitter(g)])
    aug = {'scale_factor': g['mv.scale_factor'], 'rotation': rs.golden_rotation(g, 'mv'), 'flip': g['mv.flip'],
           'jitter': jitter}
    groups = [[records[b * 4 + v] for v in range(4)] for b in range(2)]
    return groups, [[images[b * 4 + v] for v in range(4)] for b in range(2)], aug


def _cfg():
    cfg = syn.train_loop_cfg(num_layers=18, image_size=64, fundamental=True, watch_grad_norm=True, print_freq=100,
                             sigma=rs.MV['sigma'])
    cfg.DATASET.COLOR_JITTER = True
    return cfg


@pytest.fixture(scope='module')
def made_batch(cuda, golden):
    g = golden('sample_batch.npz')
    maker = datapath.BatchMaker(_cfg(), True, rs.AUG_PARAMS, rs.UNION_FLIP_PAIRS, device=cuda)
    groups, images, aug = _golden_batch(g)
    return maker.multiview(groups, images, aug)


def test_multiview_returns_the_references_collated_batch(cuda, golden, made_batch):
    g = golden('sample_batch.npz')
    inp, target, weight, meta = made_batch
    assert len(inp) == len(target) == len(weight) == len(meta) == 4
    for v in range(4):
        assert inp[v].is_cuda and target[v].is_cuda and weight[v].is_cuda
        for name, got in (('input', inp[v]), ('target', target[v]), ('weight', weight[v])):
            ref = g['mv.%s_%d' % (name, v)]
            assert tuple(got.shape) == ref.shape and got.cpu().numpy().tobytes() == ref.tobytes(), (name, v)
        assert tuple(meta[v]) == rs.META_KEYS
        assert meta[v]['source'] == g['mv.meta_%d.source' % v].tolist()
        for key in rs.META_KEYS:
            if key == 'source':
                continue
            ref = torch.from_numpy(g['mv.meta_%d.%s' % (v, key)])
            got = meta[v][key]
            assert got.dtype == ref.dtype and got.shape == ref.shape, (v, key, got.dtype, ref.dtype)
            assert torch.equal(got.cpu(), ref), (v, key)
        assert meta[v]['joints_2d_transformed'].is_cuda and not meta[v]['center'].is_cuda
    assert meta[0]['rotation'].dtype == torch.float64 and meta[1]['rotation'].dtype == torch.int64


def test_single_view_call_equals_the_multiview_rows(cuda, golden, made_batch):
    g = golden('sample_batch.npz')
    maker = datapath.BatchMaker(_cfg(), True, rs.AUG_PARAMS, rs.UNION_FLIP_PAIRS, device=cuda)
    groups, images, aug = _golden_batch(g)
    rows = [4, 5, 6, 7]
    sub = {'scale_factor': aug['scale_factor'][rows], 'rotation': [aug['rotation'][k] for k in rows],
           'flip': aug['flip'][rows], 'jitter': aug['jitter'][rows]}
    inp, target, weight, meta = maker(groups[1], images[1], sub)
    for v in range(4):
        assert torch.equal(inp[v], made_batch[0][v][1]) and torch.equal(target[v], made_batch[1][v][1])
        assert torch.equal(weight[v], made_batch[2][v][1])
        assert torch.equal(meta['joints_2d_transformed'][v], made_batch[3][v]['joints_2d_transformed'][1])
    assert meta['source'] == ['mpii'] * 4 and meta['subject'].tolist() == [-1] * 4
    # drawn here when no aug is given: an evaluation maker draws nothing and jitters nothing
    cfg = _cfg()
    cfg.DATASET.COLOR_JITTER = False
    plain = datapath.BatchMaker(cfg, False, rs.AUG_PARAMS, rs.UNION_FLIP_PAIRS, device=cuda)
    x, _, w, m = plain(groups[1], images[1])
    assert m['rotation'].dtype == torch.int64 and torch.equal(m['scale'], torch.from_numpy(g['mv.db_scale'][4:]))
    from utils.transforms import get_affine_transform
    t0 = get_affine_transform(g['mv.db_center'][4], g['mv.db_scale'][4], 0, [64, 64])
    ref = G.to_tensor_normalize(G.warp_affine_linear(images[1][0], t0, (64, 64)), datapath.IMAGENET_MEAN,
                                datapath.IMAGENET_STD)
    assert x[0].cpu().numpy().tobytes() == ref.tobytes()


def _r18(cuda, cfg, state=None):
    from models.multiview_pose_resnet import get_multiview_pose_net
    from models.pose_resnet import get_pose_net
    net = get_pose_net(cfg, is_train=False, precision='fp32')
    net.load_state_dict(syn.synthetic_state_dict(net.state_dict(), seed=7))
    model = get_multiview_pose_net(net, cfg).to(cuda)
    if state is not None:
        model.load_state_dict(state)
    return model


def test_train_takes_the_batch_as_made(cuda, golden, made_batch):
    """One core.function.train step (R18 at 64 x 64, MSE + fundamental + the gradient watch) on the batch as
    BatchMaker made it and on the same tensors copied to the host, as a loader would hand them: the same
    meters and the same parameters, bit for bit.  The batch is the golden's with pseudo labels (the records'
    own joints), so that the H36M samples keep their weights and the fundamental loss has something to weigh."""
    import copy
    from core.function import train
    from core.loss import FundamentalLoss, JointsMSELoss
    cfg = _cfg()
    groups, images, aug = _golden_batch(golden('sample_batch.npz'))
    groups = [[dict(r, joints_2d_pseudo=r['joints_2d'], joints_vis_pseudo=r['joints_vis']) for r in g] for g in groups]
    maker = datapath.BatchMaker(cfg, True, rs.AUG_PARAMS, rs.UNION_FLIP_PAIRS, pseudo_label=True, device=cuda)
    pseudo_batch = maker.multiview(groups, images, aug)
    inp, target, weight, meta = pseudo_batch
    for v in range(4):      # the same sample; only the H36M rows' weights differ: kept, not zeroed
        assert torch.equal(inp[v], made_batch[0][v]) and torch.equal(target[v], made_batch[1][v])
        assert torch.equal(weight[v][1], made_batch[2][v][1]) and not made_batch[2][v][0].any()
        assert weight[v][0].any()
    host_meta = [{k: (v.cpu() if torch.is_tensor(v) else v) for k, v in m.items()} for m in meta]
    host = ([t.cpu() for t in inp], [t.cpu() for t in target], [t.cpu() for t in weight], host_meta)
    fl = FundamentalLoss(cfg, fundamental_matrix_dict=syn.fundamental_dict(), device=cuda)
    finals, params = [], []
    state = None
    for batch in (pseudo_batch, host):
        model = _r18(cuda, cfg, state)
        if state is None:
            state = copy.deepcopy(model.state_dict())
        opt = optim.Adam(model.parameters(), lr=1e-3)
        finals.append(train(cfg, [batch], {'base_model': model},
                            {'mse_weights': JointsMSELoss(use_target_weight=True), 'fundamental': fl},
                            {'base_model': opt}, 1, '', None, 0))
        params.append([p.detach().clone() for p in model.parameters()])
    for name in ('loss', 'mse', 'fund', 'acc', 'mse_grad', 'fund_grad'):
        a, b = finals[0][name], finals[1][name]
        print('%-10s val %.9g count %g' % (name, a['val'], a['count']))
        assert (a['val'], a['avg'], a['count']) == (b['val'], b['avg'], b['count']), name
    assert np.isfinite(finals[0]['loss']['val']) and finals[0]['mse']['val'] > 0 and finals[0]['fund']['val'] > 0
    for k, (a, b) in enumerate(zip(*params)):
        assert torch.equal(a, b), 'parameter %d' % k
