"""Golden for the training sample (posu_sample_images / posu_sample_joints_targets / BatchMaker): the
REFERENCE's JointsDatasetCompatible.__getitem__ (lib/dataset/joints_dataset_compatible.py:111-201, with its
own __init__, fliplr_joints, get_affine_transform, affine_transform and generate_heatmap), imported
in-process and called per record, then torch's default_collate -- what the training loader hands
core.function.train.  cv2 and torchvision are not installed; their stand-ins are

  cv2          imread returns the seeded image of that file name; warpAffine is the oracle's restatement
               (oracle.geometry_ref.warp_affine_linear: PARITY UNPINNED against cv2 itself);
               getAffineTransform is the oracle's 6x6 solve;
  torchvision  Compose / ToPILImage / ColorJitter / ToTensor / Normalize on the installed PIL: ColorJitter is
               torchvision's composition restated (the four operations in the drawn order, each PIL's
               ImageEnhance or, for the hue, the HSV round trip with the uint8 add), the arithmetic is PIL's.

random.random, np.random.randn and ColorJitter's draws are scripted, so every drawn parameter is recorded.
MultiViewH36MCompatible.__getitem__ (multiview_h36m_compatible.py:165-174) is the loop over a group's four
records written out below (its module needs h5py and the annotation files).  Run once in this container:

    python tests/golden/make_sample_batch_golden.py

Two sections in sample_batch.npz: 'mv.' 2 groups x 4 views at 64 x 64 (maps 16 x 16) with colour jitter and
ToTensor + Normalize, collated per view; 'lab.' label edge cases at 96 x 128 (maps 24 x 32), no transform.
"""
import os
import random
import sys
import types

import numpy as np
import torch
from PIL import Image, ImageEnhance

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, REPO)
from oracle import geometry_ref as G  # noqa: E402

MEAN, STD = (0.485, 0.456, 0.406), (0.229, 0.224, 0.225)
AUG = {'mpii': {'scale_factor': 0.25, 'rotation_factor': 30, 'flip': True},
       'h36m': {'scale_factor': 0.25, 'rotation_factor': 30, 'flip': False}}
IMAGES = {}          # file name -> seeded image, what the cv2 stand-in's imread returns
SCRIPT = {'random': [], 'randn': [], 'jitter': []}


# ---------------------------------------------------------------- stand-ins
def _cv2():
    cv2 = types.ModuleType('cv2')
    cv2.IMREAD_COLOR, cv2.IMREAD_IGNORE_ORIENTATION, cv2.INTER_LINEAR = 1, 128, 1
    cv2.imread = lambda path, flags=None: IMAGES[os.path.basename(path)].copy()
    cv2.warpAffine = lambda img, trans, dsize, flags=None: G.warp_affine_linear(np.ascontiguousarray(img), trans, dsize)
    cv2.getAffineTransform = lambda src, dst: G._solve_affine(src, dst)
    return cv2


class Compose:
    def __init__(self, transforms):
        self.transforms = transforms

    def __call__(self, x):
        for t in self.transforms:
            x = t(x)
        return x


class ToPILImage:
    def __call__(self, arr):
        return Image.fromarray(np.ascontiguousarray(arr), 'RGB')


class ColorJitter:
    """torchvision.transforms.ColorJitter.forward on a PIL image; the draws of get_params are scripted."""

    def __init__(self, brightness, contrast, saturation, hue):
        self.ranges = (brightness, contrast, saturation, (-hue, hue))

    def __call__(self, img):
        order, b, c, s, h = SCRIPT['jitter'].pop(0)
        for lo_hi, val in zip(self.ranges, (b, c, s, h)):
            assert lo_hi[0] <= val <= lo_hi[1]
        for fn_id in order:
            if fn_id == 0:
                img = ImageEnhance.Brightness(img).enhance(b)
            elif fn_id == 1:
                img = ImageEnhance.Contrast(img).enhance(c)
            elif fn_id == 2:
                img = ImageEnhance.Color(img).enhance(s)
            else:                                  # torchvision _functional_pil.adjust_hue
                hh, ss, vv = img.convert('HSV').split()
                np_h = np.array(hh, dtype=np.uint8)
                np_h = (np_h.astype(np.int64) + np.int64(np.trunc(h * 255))).astype(np.uint8)   # the uint8 add wraps
                img = Image.merge('HSV', (Image.fromarray(np_h, 'L'), ss, vv)).convert('RGB')
        return img


class ToTensor:
    def __call__(self, pic):
        return torch.from_numpy(np.array(pic)).permute(2, 0, 1).contiguous().to(torch.float32).div(255)


class Normalize:
    def __init__(self, mean, std):
        self.mean, self.std = torch.tensor(mean, dtype=torch.float32), torch.tensor(std, dtype=torch.float32)

    def __call__(self, t):
        return (t - self.mean.view(-1, 1, 1)) / self.std.view(-1, 1, 1)


def _reference_dataset_class():
    sys.path.insert(0, '/root/reference/lib')
    sys.modules['cv2'] = _cv2()
    tv = types.ModuleType('torchvision')
    tv.transforms = types.ModuleType('torchvision.transforms')
    for cls in (Compose, ToPILImage, ColorJitter, ToTensor, Normalize):
        setattr(tv.transforms, cls.__name__, cls)
    sys.modules['torchvision'], sys.modules['torchvision.transforms'] = tv, tv.transforms
    import importlib.util
    spec = importlib.util.spec_from_file_location(
        'ref_joints_dataset_compatible', '/root/reference/lib/dataset/joints_dataset_compatible.py')
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod.JointsDatasetCompatible


def _dataset(cls, image_size, heatmap_size, sigma, color_jitter, transform, db):
    ns = types.SimpleNamespace
    cfg = ns(DATASET=ns(ROOT='', DATA_FORMAT='jpg', COLOR_JITTER=color_jitter),
             NETWORK=ns(IMAGE_SIZE=np.array(image_size), HEATMAP_SIZE=np.array(heatmap_size), SIGMA=sigma))
    ds = cls(cfg, 'train', True, transform)
    ds.db, ds.no_distortion, ds.pseudo_label, ds.aug_param_dict = db, False, False, AUG
    return ds


# ---------------------------------------------------------------- seeded inputs
def _image(name, h, w, seed, constant=None):
    r = np.random.default_rng(seed)
    if constant is not None:
        img = np.empty((h, w, 3), dtype=np.uint8)
        img[:] = constant
    else:
        # smooth colour ramps plus noise: every hue sector and a wide range of saturations
        yy, xx = np.meshgrid(np.arange(h), np.arange(w), indexing='ij')
        img = np.stack([(xx * 255 // max(w - 1, 1)), (yy * 255 // max(h - 1, 1)), ((xx + yy) * 3) % 256], axis=2)
        img = np.clip(img + r.integers(-40, 41, img.shape), 0, 255).astype(np.uint8)
    IMAGES[name] = img
    return img


def _record(name, source, subject, center, scale, joints, vis):
    vis3 = np.concatenate([vis, vis[:, :1]], axis=1)
    return {'image': name, 'source': source, 'subject': subject, 'center': np.asarray(center, dtype=np.float64),
            'scale': np.asarray(scale, dtype=np.float64), 'joints_2d': np.asarray(joints, dtype=np.float64),
            'joints_vis': vis3.astype(np.float64)}


def _scale_factor(randn, sf=0.25):
    return float(np.clip(randn * sf + 1, 1 - sf, 1 + sf))     # :151


def _script_aug(randn_scale, rot_u, randn_rot, flip_u):
    """One augmented record's draws in the order __getitem__ makes them (:151-155)."""
    SCRIPT['randn'].append(randn_scale)
    SCRIPT['random'].append(rot_u)
    if rot_u <= 0.6:
        SCRIPT['randn'].append(randn_rot)
    SCRIPT['random'].append(flip_u)


def mv_records():
    """2 groups x 4 views: group 0 'h36m' (no augmentation, weights zeroed), group 1 'mpii' (augmented)."""
    r = np.random.default_rng(2024)
    sizes = [(37, 53), (64, 48), (50, 50), (41, 67), (64, 48), (37, 53), (48, 64), (30, 30)]
    db, jit = [], []
    for k, (h, w) in enumerate(sizes):
        name = 'mv_%d.jpg' % k
        _image(name, h, w, 500 + k, constant=(90, 90, 90) if k == 2 else None)
        joints = r.uniform(-0.1, 1.1, (16, 2)) * np.array([w, h])
        vis = (r.uniform(size=(16, 1)) > 0.25).astype(np.float64).repeat(2, axis=1)
        center = np.array([w * r.uniform(0.3, 0.7), h * r.uniform(0.3, 0.7)])
        scale = np.array([1.0, 1.0]) * max(h, w) / 200.0 * r.uniform(0.7, 1.3)
        group = k // 4
        db.append(_record(name, 'h36m' if group == 0 else 'mpii', 9 if group == 0 else 11, center, scale, joints, vis))
        order = [int(v) for v in r.permutation(4)]
        hue = (0.0, -0.13, 0.2, -0.2, 0.07, 0.0, -0.004, 0.15)[k]
        jit.append((order, float(np.float32(r.uniform(0.7, 3.0))), float(np.float32(r.uniform(0.5, 2.0))),
                    float(np.float32(r.uniform(0.5, 2.0))), hue))
    draws = [(0.9, 0.3, 0.8, 0.2), (-5.0, 0.9, 0.0, 0.7), (5.0, 0.5, 4.0, 0.5), (0.1, 0.6, -0.5, 0.51)]
    return db, jit, draws


def _joint_at(mu, stride):
    """A coordinate whose int(v / stride + 0.5) is mu, a quarter cell from either boundary."""
    return stride * (mu + 0.25) if mu >= 0 else stride * (mu - 0.75)


def lab_records():
    """Label edge cases at 96 x 128 -> 24 x 32, sigma 1 (stride 4, tmp 3); all 'mpii' but record 4."""
    r = np.random.default_rng(77)
    h, w = 128, 96
    db, draws = [], []
    unit = (np.array([48.0, 64.0]), np.array([0.48, 0.48]))      # centre and scale of the identity crop
    for k in range(6):
        name = 'lab_%d.jpg' % k
        _image(name, h, w, 700 + k)
        joints = r.uniform(-0.1, 1.1, (16, 2)) * np.array([w, h])
        vis = (r.uniform(size=(16, 1)) > 0.25).astype(np.float64).repeat(2, axis=1)
        center, scale = np.array([w * r.uniform(0.4, 0.6), h * r.uniform(0.4, 0.6)]), np.array([0.6, 0.6])
        source = 'mpii'
        if k == 0:                        # flip + rotation, one joint visible in x only
            vis[3] = (1.0, 0.0)
            draws.append((0.4, 0.1, 0.6, 0.1))
        elif k == 1:                      # exactly one visible joint: affine_transform's .squeeze() case
            vis[:] = 0.0
            vis[7] = 1.0
            draws.append((-0.3, 0.2, -0.7, 0.9))
        elif k == 2:                      # none visible, flipped
            vis[:] = 0.0
            draws.append((0.0, 0.9, 0.0, 0.3))
        elif k == 3:                      # the identity crop: joints placed in map cells
            center, scale = unit
            vis[:] = 1.0
            mid = (_joint_at(12, 4.0), _joint_at(16, 4.0))
            xs = [_joint_at(m, 4.0) for m in (26, 27, -4, -5)] + [-0.4 * 4, -1.6 * 4]   # ul = 23 | 24, br = 0 | -1
            ys = [_joint_at(m, 4.0) for m in (34, 35, -4, -5)]
            for i, x in enumerate(xs):
                joints[i] = (x, mid[1])
            for i, y in enumerate(ys):
                joints[6 + i] = (mid[0], y)
            joints[10] = (22.0 - 2.0 ** -30, mid[1])      # x / 4 + 0.5 just below 6 in f64, 6 in f32
            joints[11] = (mid[0], 4 * 7.5)                # exactly on a .5 boundary
            vis[12], vis[13] = (0.5, 0.5), (0.0, 0.0)     # keeps its weight and paints nothing | off
            draws.append((0.0, 0.9, 0.0, 0.9))            # scale x 1, no rotation, no flip
        elif k == 4:                      # h36m without pseudo labels: weights zeroed, nothing drawn
            source = 'h36m'
        else:                             # one visible joint, flipped
            vis[:] = 0.0
            vis[12] = 1.0
            draws.append((0.2, 0.7, 0.0, 0.4))
        db.append(_record(name, source, 9 if source == 'h36m' else 1, center, scale, joints, vis))
    return db, draws


# ---------------------------------------------------------------- recording
def main():
    cls = _reference_dataset_class()
    random.random = lambda: SCRIPT['random'].pop(0)
    np.random.randn = lambda: SCRIPT['randn'].pop(0)
    out = {}

    # ---- mv: the multi-view batch
    db, jit, draws = mv_records()
    ds = _dataset(cls, (64, 64), (16, 16), 1, True, Compose([ToTensor(), Normalize(MEAN, STD)]), db)
    assert ds.flip_pairs == [[0, 5], [1, 4], [2, 3], [10, 15], [11, 14], [12, 13]]
    for d in draws:
        _script_aug(*d)
    SCRIPT['jitter'].extend(jit)
    grouping = [[0, 1, 2, 3], [4, 5, 6, 7]]
    groups = []
    for items in grouping:                      # MultiViewH36MCompatible.__getitem__
        inp, tgt, wgt, meta = [], [], [], []
        for item in items:
            i, t, w, m = ds[item]
            inp.append(i), tgt.append(t), wgt.append(w), meta.append(m)
        groups.append((inp, tgt, wgt, meta))
    assert not SCRIPT['random'] and not SCRIPT['randn'] and not SCRIPT['jitter']
    inp, tgt, wgt, meta = torch.utils.data.default_collate(groups)
    for v in range(4):
        out['mv.input_%d' % v], out['mv.target_%d' % v] = inp[v].numpy(), tgt[v].numpy()
        out['mv.weight_%d' % v] = wgt[v].numpy()
        for key, val in meta[v].items():
            out['mv.meta_%d.%s' % (v, key)] = np.array(val) if key == 'source' else val.numpy()
    for k, rec in enumerate(db):
        out['mv.image_%d' % k] = IMAGES[rec['image']]
    _save_db(out, 'mv', db)
    out['mv.jitter_order'] = np.array([j[0] for j in jit], dtype=np.uint8)
    out['mv.jitter_factors'] = np.array([j[1:4] for j in jit], dtype=np.float32)
    out['mv.jitter_hue'] = np.array([j[4] for j in jit], dtype=np.float64)
    # what was drawn, per record: meta's scale / rotation / the flip (the centre moved)
    flat_meta = [groups[g][3][v] for g in range(2) for v in range(4)]
    out['mv.scale_factor'] = np.array([1.0] * 4 + [_scale_factor(d[0]) for d in draws])
    out['mv.rotation'] = np.array([float(m['rotation']) for m in flat_meta])
    out['mv.flip'] = np.array([m['center'][0] != rec['center'][0] for m, rec in zip(flat_meta, db)])

    # ---- lab: label edge cases
    db, draws = lab_records()
    ds = _dataset(cls, (96, 128), (24, 32), 1, False, None, db)
    for d in draws:
        _script_aug(*d)
    samples = [ds[i] for i in range(len(db))]
    assert not SCRIPT['random'] and not SCRIPT['randn']
    out['lab.target'] = np.stack([s[1].numpy() for s in samples])
    out['lab.weight'] = np.stack([s[2].numpy() for s in samples])
    out['lab.joints_2d_transformed'] = np.stack([s[3]['joints_2d_transformed'] for s in samples])
    out['lab.joints_vis'] = np.stack([s[3]['joints_vis'] for s in samples])
    out['lab.center'] = np.stack([s[3]['center'] for s in samples])
    out['lab.scale'] = np.stack([s[3]['scale'] for s in samples])
    out['lab.rotation'] = np.array([float(s[3]['rotation']) for s in samples])
    factors = iter(_scale_factor(d[0]) for d in draws)
    out['lab.scale_factor'] = np.array([next(factors) if rec['source'] != 'h36m' else 1.0 for rec in db])
    out['lab.flip'] = np.array([s[3]['center'][0] != rec['center'][0] for s, rec in zip(samples, db)])
    out['lab.width'] = np.array([IMAGES[rec['image']].shape[1] for rec in db], dtype=np.int32)
    _save_db(out, 'lab', db)
    # fliplr_joints on its own, as the reference returns it (the product, the swapped vis)
    sys.path.insert(0, '/root/reference/lib')
    from utils.transforms import fliplr_joints
    j, v = fliplr_joints(db[0]['joints_2d'].copy(), db[0]['joints_vis'].copy()[:, :2], 96, ds.flip_pairs)
    out['lab.fliplr_joints'], out['lab.fliplr_vis'] = j, v
    # the checks the cases were built for
    jt = out['lab.joints_2d_transformed']
    x = jt[3, 10, 0]
    assert int(x / 4.0 + 0.5) == 5 and int(float(np.float32(x)) / 4.0 + 0.5) == 6, x
    w3 = out['lab.weight'][3, :, 0]
    assert w3[:10].tolist() == [1, 0, 1, 0, 1, 1, 1, 0, 1, 0], w3
    assert out['lab.flip'].tolist() == [True, False, True, False, False, True]
    assert (out['lab.joints_vis'][1, :, 0] > 0).sum() == 1 and (out['lab.joints_vis'][5, :, 0] > 0).sum() == 1
    assert not out['lab.weight'][4].any() and out['lab.target'][4].any()
    assert out['mv.flip'].tolist() == [False] * 4 + [True, False, True, False], out['mv.flip']
    np.savez_compressed(os.path.join(HERE, 'sample_batch.npz'), **out)
    print('sample batch golden written: %d arrays, rotations %s / %s' % (len(out), out['mv.rotation'], out['lab.rotation']))


def _save_db(out, prefix, db):
    for key in ('center', 'scale', 'joints_2d', 'joints_vis'):
        out['%s.db_%s' % (prefix, key)] = np.stack([rec[key] for rec in db])
    out['%s.db_source' % prefix] = np.array([rec['source'] for rec in db])
    out['%s.db_subject' % prefix] = np.array([rec['subject'] for rec in db], dtype=np.int64)


if __name__ == '__main__':
    main()
