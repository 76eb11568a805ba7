"""The training sample, host side (no kernel is launched here):

* the numpy restatement (tests/sample_restatement.py) of PIL's point operations equals the installed PIL,
  exhaustively: RGB -> HSV and HSV -> RGB over all 2^24 triples, the ImageEnhance blend over all 256 x 256
  (degenerate, value) pairs, L over all triples;
* the restatement of the whole sample equals the reference's own __getitem__ as recorded in
  tests/golden/sample_batch.npz (make_sample_batch_golden.py), bit for bit;
* utils.transforms.fliplr_joints, posu.datapath.draw_augmentation, the three posu_sample_* symbols and their
  argument checks, and the wrappers' refusal of CPU tensors.
"""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

import sample_restatement as rs
from oracle import geometry_ref as G
from posu import _native, datapath

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ('posu_sample_workspace', 'posu_sample_images', 'posu_sample_joints_targets')


# ------------------------------------------------------------------ the restatement equals PIL
@pytest.fixture(scope='module')
def triples():
    """All 2^24 byte triples as a 4096 x 4096 x 3 image."""
    v = np.arange(1 << 24, dtype=np.int64)
    return np.stack([(v >> 16) & 255, (v >> 8) & 255, v & 255], axis=1).astype(np.uint8).reshape(4096, 4096, 3)


def test_rgb_to_hsv_equals_pil_over_all_triples(triples):
    Image = pytest.importorskip('PIL.Image')
    ref = np.asarray(Image.fromarray(triples, 'RGB').convert('HSV'))
    got = np.stack(rs.rgb_to_hsv(triples[..., 0], triples[..., 1], triples[..., 2]), axis=-1)
    assert int((got != ref).any(-1).sum()) == 0
    l_ref = np.asarray(Image.fromarray(triples, 'RGB').convert('L'))
    assert np.array_equal(rs.pil_l(triples[..., 0], triples[..., 1], triples[..., 2]), l_ref)


def test_hsv_to_rgb_equals_pil_over_all_triples(triples):
    Image = pytest.importorskip('PIL.Image')
    ref = np.asarray(Image.fromarray(triples, 'HSV').convert('RGB'))
    got = np.stack(rs.hsv_to_rgb(triples[..., 0], triples[..., 1], triples[..., 2]), axis=-1)
    assert int((got != ref).any(-1).sum()) == 0
    # the round trip the hue step makes for a shift of 0 is lossy: up to 7 grey levels
    sub = triples[::17, ::13]
    back = np.stack(rs.hsv_to_rgb(*rs.rgb_to_hsv(sub[..., 0], sub[..., 1], sub[..., 2])), axis=-1)
    assert 0 < np.abs(back - sub.astype(np.int64)).max() <= 7


@pytest.mark.parametrize('factor', [0, 0.5, 1, 1.3, 3.0, 0.7, 2.0, float(np.float32(0.9999)), 1.0001, 0.123456])
def test_blend_equals_pil_over_all_pairs(factor):
    """The factors of the three ImageEnhance steps: 0, 1 and the ends of ColorJitter's ranges (0.7 / 3.0,
    0.5 / 2.0) among them."""
    Image = pytest.importorskip('PIL.Image')
    d, x = np.meshgrid(np.arange(256), np.arange(256), indexing='ij')
    ref = np.asarray(Image.blend(Image.fromarray(d.astype(np.uint8), 'L'), Image.fromarray(x.astype(np.uint8), 'L'),
                                 factor))
    assert np.array_equal(rs.blend(d, x, factor), ref)


def test_color_jitter_equals_image_enhance_on_an_image(golden):
    """The composition on a real image, every order: ImageEnhance's three classes and the HSV round trip
    against the restatement's color_jitter (the contrast grey from the image's own mean L)."""
    Image = pytest.importorskip('PIL.Image')
    from PIL import ImageEnhance
    import itertools
    img = golden('sample_batch.npz')['mv.image_0'][:, :, ::-1]
    b, c, s, shift = 1.7, 0.6, 1.9, 231
    for order in itertools.permutations(range(4)):
        pil = Image.fromarray(np.ascontiguousarray(img), 'RGB')
        for op in order:
            if op == rs.BRIGHTNESS:
                pil = ImageEnhance.Brightness(pil).enhance(b)
            elif op == rs.CONTRAST:
                pil = ImageEnhance.Contrast(pil).enhance(c)
            elif op == rs.SATURATION:
                pil = ImageEnhance.Color(pil).enhance(s)
            else:
                h, sat, v = pil.convert('HSV').split()
                h = Image.fromarray(((np.asarray(h).astype(np.int64) + shift) % 256).astype(np.uint8), 'L')
                pil = Image.merge('HSV', (h, sat, v)).convert('RGB')
        got, l_sum = rs.color_jitter(img, order, b, c, s, shift)
        assert np.array_equal(got, np.asarray(pil)), order
        assert l_sum is not None and l_sum > 0


# ------------------------------------------------------------------ the restatement equals the reference
def _mv_sample(g, k, jitter):
    img = g['mv.image_%d' % k]
    _, _, trans = rs.golden_trans(g, 'mv', k, img.shape[1], rs.MV['image_size'])
    return rs.sample(img, g['mv.db_joints_2d'][k], g['mv.db_joints_vis'][k], bool(g['mv.flip'][k]), trans,
                     rs.MV['image_size'], rs.MV['heatmap_size'], rs.MV['sigma'], g['mv.db_source'][k] == 'h36m',
                     jitter[k], rs.MEAN, rs.STD)


def test_restatement_equals_the_references_multiview_batch(golden):
    g = golden('sample_batch.npz')
    jitter = rs.golden_jitter(g)
    assert [j['hue_shift'] for j in jitter].count(0) == 2 and any(j['hue_shift'] > 200 for j in jitter)
    for v in range(4):
        for b in range(2):
            k = b * 4 + v
            inp, tgt, wgt, j2d, vis = _mv_sample(g, k, jitter)
            assert inp.dtype == np.float32 and inp.tobytes() == g['mv.input_%d' % v][b].tobytes(), k
            assert tgt.tobytes() == g['mv.target_%d' % v][b].tobytes(), k
            assert wgt.tobytes() == g['mv.weight_%d' % v][b].tobytes(), k
            assert np.array_equal(j2d, g['mv.meta_%d.joints_2d_transformed' % v][b]), k
            assert np.array_equal(vis, g['mv.meta_%d.joints_vis' % v][b]), k
            center, scale, _ = rs.golden_trans(g, 'mv', k, g['mv.image_%d' % k].shape[1], rs.MV['image_size'])
            assert np.array_equal(center, g['mv.meta_%d.center' % v][b]), k
            assert np.array_equal(scale, g['mv.meta_%d.scale' % v][b]), k
    # the batch holds what it was built to hold: flips, rotations, both clip bounds of the scale, a grey image
    assert g['mv.flip'].sum() == 2 and (g['mv.rotation'] != 0).sum() == 3
    assert set(g['mv.scale_factor'][4:]) >= {0.75, 1.25}
    assert not g['mv.weight_0'][0].any() and g['mv.weight_0'][1].any()      # h36m zeroed, mpii kept


def test_restatement_equals_the_references_label_cases(golden):
    g = golden('sample_batch.npz')
    for k in range(len(g['lab.db_source'])):
        _, _, trans = rs.golden_trans(g, 'lab', k, int(g['lab.width'][k]), rs.LAB['image_size'])
        j2d, vis, tgt, wgt = rs.sample_joints_targets(
            g['lab.db_joints_2d'][k], g['lab.db_joints_vis'][k], bool(g['lab.flip'][k]), int(g['lab.width'][k]),
            rs.UNION_FLIP_PAIRS, trans, g['lab.db_source'][k] == 'h36m', rs.LAB['image_size'],
            rs.LAB['heatmap_size'], rs.LAB['sigma'])
        assert np.array_equal(j2d, g['lab.joints_2d_transformed'][k]), k
        assert np.array_equal(vis, g['lab.joints_vis'][k]), k
        assert tgt.tobytes() == g['lab.target'][k].tobytes(), k
        assert wgt.tobytes() == g['lab.weight'][k].tobytes(), k


def test_fliplr_joints_equals_the_reference(golden):
    from utils.transforms import fliplr_joints
    g = golden('sample_batch.npz')
    joints, vis = g['lab.db_joints_2d'][0].copy(), g['lab.db_joints_vis'][0][:, :2].copy()
    j, v = fliplr_joints(joints, vis, 96, rs.UNION_FLIP_PAIRS)
    assert np.array_equal(j, g['lab.fliplr_joints']) and np.array_equal(v, g['lab.fliplr_vis'])
    assert v is vis and np.array_equal(joints[:, 0] * vis[:, 0], j[:, 0])     # in place, like the reference
    rj, rv = rs.fliplr_joints(g['lab.db_joints_2d'][0], g['lab.db_joints_vis'][0][:, :2], 96, rs.UNION_FLIP_PAIRS)
    assert np.array_equal(rj, j) and np.array_equal(rv, v)


# ------------------------------------------------------------------ draw_augmentation
def _records(sources):
    return [{'source': s} for s in sources]


def test_nothing_is_drawn_for_h36m_or_outside_training():
    for is_train, sources in ((True, ['h36m'] * 5), (False, ['mpii', 'h36m', 'mpii'])):
        rng = np.random.default_rng(5)
        state = rng.bit_generator.state
        aug = datapath.draw_augmentation(_records(sources), rs.AUG_PARAMS, is_train, False, rng)
        assert rng.bit_generator.state == state                       # not one draw
        assert np.array_equal(aug['scale_factor'], np.ones(len(sources))) and not aug['flip'].any()
        assert aug['rotation'] == [0] * len(sources) and all(type(r) is int for r in aug['rotation'])
        assert aug['jitter'] is None


def test_draws_follow_the_references_distributions():
    n = 4000
    aug = datapath.draw_augmentation(_records(['mpii'] * n), rs.AUG_PARAMS, True, True, np.random.default_rng(1))
    sf, rot, flip, jit = aug['scale_factor'], np.array(aug['rotation'], dtype=np.float64), aug['flip'], aug['jitter']
    assert sf.min() == 0.75 and sf.max() == 1.25                      # both clip bounds are hit
    assert rot.min() == -60.0 and rot.max() == 60.0
    assert 0.35 < (rot == 0).mean() < 0.45 and 0.45 < flip.mean() < 0.55
    assert jit.dtype == datapath.JITTER_DTYPE and jit.dtype.itemsize == 20 and jit['active'].all()
    assert all(sorted(o) == [0, 1, 2, 3] for o in jit['order'].tolist())        # a permutation
    assert len({tuple(o) for o in jit['order'].tolist()}) == 24
    assert 0.7 <= jit['brightness'].min() and jit['brightness'].max() <= 3.0 and jit['brightness'].max() > 2.9
    for name in ('contrast', 'saturation'):
        assert 0.5 <= jit[name].min() < 0.51 and 1.99 < jit[name].max() <= 2.0
    shift = jit['hue_shift'].astype(int)
    assert set(np.unique(shift)) == set(range(0, 51)) | set(range(206, 256))     # trunc(hue * 255) mod 256
    # a source whose 'flip' is off never flips; the jitter is drawn for h36m too
    params = {'mpii': dict(rs.AUG_PARAMS['mpii'], flip=False), 'h36m': rs.AUG_PARAMS['h36m']}
    aug = datapath.draw_augmentation(_records(['mpii', 'h36m'] * 50), params, True, True, np.random.default_rng(2))
    assert not aug['flip'].any() and aug['jitter']['active'].all()
    assert np.all(aug['scale_factor'][1::2] == 1.0) and np.any(aug['scale_factor'][0::2] != 1.0)


def test_a_negative_hue_wraps():
    assert datapath.hue_shift_of(-0.1) == 231 and datapath.hue_shift_of(-0.003) == 0
    assert datapath.hue_shift_of(0.1) == 25 and datapath.hue_shift_of(-0.2) == rs.hue_shift_of(-0.2)
    for hue in np.linspace(-0.2, 0.2, 41):
        assert datapath.hue_shift_of(hue) == rs.hue_shift_of(hue)


# ------------------------------------------------------------------ the C ABI
def test_sample_symbols_are_declared_listed_and_exported():
    src = open(os.path.join(REPO, 'include', 'posu.h')).read()
    src = re.sub(r'/\*.*?\*/', '', src, flags=re.S)
    declared = set(re.findall(r'\b(posu_\w+)\s*\(', src))
    lib = _native.load()
    for name in SYMBOLS:
        assert name in declared, name
        assert name in _native.exported_symbols(), name
        assert hasattr(lib, name), name
    assert lib.posu_abi_version() == _native.ABI_VERSION == 16   # additive: the revision does not move
    assert lib.posu_sample_workspace(0) == 0 and lib.posu_sample_workspace(128) == 1024
    assert lib.posu_sample_workspace(-1) == -1


def test_argument_errors_are_reported_before_any_launch():
    lib = _native.load()
    p = ctypes.c_void_p(256)

    def err(st, text):
        assert st == 1, st
        assert text in _native.last_error(), _native.last_error()

    def images(src=p, off=p, hw=p, C=3, M=p, jit=None, contrast=0, N=2, dh=8, dw=8, mode=0, mean=None, std=None,
               ws=None, ws_bytes=0, out=p):
        return lib.posu_sample_images(src, off, hw, C, M, None, jit, contrast, 1, N, dh, dw, mode, mean, std, ws,
                                      ws_bytes, out, None)
    for kw in ({'src': None}, {'off': None}, {'hw': None}, {'M': None}, {'out': None}, {'contrast': 1}):
        err(images(**kw), 'null pointer')
    for kw in ({'C': 1}, {'C': 4}, {'N': -1}, {'N': 65536}, {'dh': 0}, {'dw': 0}, {'dh': 1 << 16, 'dw': 1 << 16}):
        err(images(**kw), 'bad shape')
    err(images(mode=2), 'mode must be')
    err(images(mode=1), 'mean and std')
    err(images(jit=p), 'workspace')
    err(images(jit=p, ws=p, ws_bytes=8), 'workspace')
    assert images(N=0) == 0                                            # no records: OK, nothing launched

    def labels(j=p, v=p, flip=None, hw=None, perm=None, M=p, N=2, J=16, iw=64, ih=64, mw=16, mh=16, sigma=1.0,
               jo=p, vo=p, t=p, w=p):
        return lib.posu_sample_joints_targets(j, v, flip, hw, perm, M, None, N, J, iw, ih, mw, mh, sigma, jo, vo, t,
                                              w, None)
    for kw in ({'j': None}, {'v': None}, {'M': None}, {'jo': None}, {'vo': None}, {'t': None}, {'w': None},
               {'flip': p}, {'flip': p, 'hw': p}, {'flip': p, 'perm': p}):
        err(labels(**kw), 'null pointer')
    for kw in ({'N': -1}, {'J': 0}, {'iw': 0}, {'ih': 0}, {'mw': 0}, {'mh': 0}, {'sigma': 0.0},
               {'mw': 1 << 16, 'mh': 1 << 16}):
        err(labels(**kw), 'bad shape')
    err(labels(N=1 << 28, J=16), 'too large')
    assert labels(N=0) == 0


def test_the_wrappers_refuse_cpu_tensors():
    img = [np.zeros((8, 8, 3), dtype=np.uint8)]
    eye = np.array([[[1.0, 0, 0], [0, 1.0, 0]]])
    with pytest.raises(RuntimeError, match='cuda'):
        datapath.sample_images(img, eye, (8, 8), torch.device('cpu'))
    with pytest.raises(RuntimeError, match='cuda'):
        datapath.sample_images([torch.zeros(8, 8, 3, dtype=torch.uint8)], eye, (8, 8), 'cpu',
                               jitter=datapath.jitter_records(1))
    with pytest.raises(RuntimeError, match='cuda'):
        datapath.sample_joints_targets(torch.zeros(1, 16, 2, dtype=torch.float64),
                                       torch.ones(1, 16, 2, dtype=torch.float64), eye, (8, 8), (2, 2))
    from posu import synthetic as syn
    with pytest.raises(RuntimeError, match='cuda'):
        datapath.BatchMaker(syn.train_loop_cfg(sigma=1), True, rs.AUG_PARAMS, rs.UNION_FLIP_PAIRS, device='cpu')


def test_jitter_record_layout_is_the_headers():
    """JITTER_DTYPE is posu_jitter of include/posu.h field by field: 3 f32, order[4], hue_shift, active, pad."""
    src = open(os.path.join(REPO, 'include', 'posu.h')).read()
    body = re.search(r'typedef struct posu_jitter \{(.*?)\} posu_jitter;', src, flags=re.S).group(1)
    fields = re.findall(r'(\w+)(?:\[(\d+)\])?\s*[,;]', body)
    assert [f for f, _ in fields] == ['brightness', 'contrast', 'saturation', 'order', 'hue_shift', 'active',
                                      'reserved']
    dt = datapath.JITTER_DTYPE
    assert list(dt.names) == [f for f, _ in fields]
    assert [dt.fields[n][1] for n in dt.names] == [0, 4, 8, 12, 16, 17, 18] and dt.itemsize == 20
    rec = datapath.jitter_records(3)
    assert not rec['active'].any() and rec['order'].tolist() == [[0, 1, 2, 3]] * 3
