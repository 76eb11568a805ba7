"""Batch data-path kernels: the crop of
JointsDatasetCompatible.__getitem__ (cv2.warpAffine INTER_LINEAR, optionally fused with
ToTensor + Normalize; lib/dataset/joints_dataset_compatible.py:161-172) for a whole batch in one
launch, Gaussian target heatmaps (JointsDatasetCompatible.generate_heatmap,
joints_dataset_compatible.py:215-253) in one launch, and the sum-normalised integral decode of
run/test/test_integral.py:63-70.  cuda tensors only.

The training half of __getitem__ (joints_dataset_compatible.py:111-201) for a whole batch: sample_images
(flip, warp, ColorJitter, ToTensor + Normalize), sample_joints_targets (fliplr_joints, the joints' affine,
the targets, in f64 where the reference is), draw_augmentation (the reference's draws, on the host) and
BatchMaker, which joins them into the batch core.function.train takes.
"""
import numpy as np
import torch

from ._native import call, ptr, stream_of, require_cuda

# run/pose2d/train.py:322-323 (transforms.Normalize after ToTensor)
IMAGENET_MEAN = (0.485, 0.456, 0.406)
IMAGENET_STD = (0.229, 0.224, 0.225)


def _flatten_images(images):
    """N uint8 [H, W, C] arrays or tensors -> (flat uint8 tensors, element offsets [N + 1], shapes)."""
    shapes = [tuple(im.shape) for im in images]
    if any(len(sh) != 3 for sh in shapes) or len({sh[2] for sh in shapes}) > 1:
        raise ValueError('images must be [H, W, C] with one channel count')
    offs = np.cumsum([0] + [int(np.prod(sh)) for sh in shapes])
    flat = [im.reshape(-1) if torch.is_tensor(im) else torch.from_numpy(np.ascontiguousarray(im).reshape(-1))
            for im in images]
    if any(f.dtype != torch.uint8 for f in flat):
        raise TypeError('uint8 images expected (cv2.imread)')
    return flat, offs, shapes


def _upload_images(images, device):
    """The concatenated sources on `device` with their offsets and [H, W] table, and the channel count."""
    flat, offs, shapes = _flatten_images(images)
    c = shapes[0][2] if shapes else 3
    src = torch.cat([f.to(device) for f in flat]) if flat else torch.empty(0, dtype=torch.uint8, device=device)
    off = torch.tensor(offs[:-1], dtype=torch.int64, device=device)
    hw = torch.tensor([[sh[0], sh[1]] for sh in shapes], dtype=torch.int32, device=device).reshape(-1)
    return src, off, hw, c


def crop_warp(images, trans, image_size, device, out='f32', mean=IMAGENET_MEAN, std=IMAGENET_STD):
    """images: N uint8 [H, W, C] arrays (numpy or cuda tensors, sizes may differ); trans: [N, 2, 3]
    src -> dst affines (utils.transforms.get_affine_transform(center, scale, rot, image_size));
    image_size (w, h).  out='u8': cv2.warpAffine's uint8 [N, h, w, C]; out='f32': the network input
    ToTensor + Normalize would give, f32 [N, C, h, w]."""
    if out not in ('u8', 'f32'):
        raise ValueError("out must be 'u8' or 'f32'")
    n = len(images)
    dw, dh = int(image_size[0]), int(image_size[1])
    src, off, hw, c = _upload_images(images, device)
    M = torch.as_tensor(np.asarray(trans, dtype=np.float64).reshape(n, 6), device=device).contiguous()
    require_cuda(src)
    if out == 'u8':
        res = torch.empty((n, dh, dw, c), dtype=torch.uint8, device=device)
        m = s = None
    else:
        res = torch.empty((n, c, dh, dw), dtype=torch.float32, device=device)
        m = torch.tensor(mean, dtype=torch.float32, device=device)
        s = torch.tensor(std, dtype=torch.float32, device=device)
        if m.numel() != c or s.numel() != c:
            raise ValueError('mean / std need one value per channel')
    call('posu_crop_warp', ptr(src), ptr(off), ptr(hw), c, ptr(M), n, dh, dw, 0 if out == 'u8' else 1, ptr(m), ptr(s),
         ptr(res), stream_of(device))
    return res


def crop_batch(images, centers, scales, rotations, image_size, device, out='f32'):
    """The crops of a batch as __getitem__ makes them: trans = get_affine_transform(center,
    scale, rotation, image_size) per sample (host, float64), then crop_warp."""
    from utils.transforms import get_affine_transform
    trans = np.stack([get_affine_transform(np.asarray(c, dtype=np.float64), np.asarray(s, dtype=np.float64), r,
                                           image_size) for c, s, r in zip(centers, scales, rotations)])
    return crop_warp(images, trans, image_size, device, out=out), trans


def generate_heatmaps(joints, joints_vis, image_size, heatmap_size, sigma=2, zero_weight=None):
    """joints [N, J, 2] (crop px), joints_vis [N, J] or [N, J, k] (column 0 used) ->
    (target [N, J, hm_h, hm_w] f32, target_weight [N, J, 1] f32).  zero_weight: optional
    [N] bool, samples whose weights are zeroed (H36M without pseudo labels)."""
    require_cuda(joints)
    j = joints.float().contiguous()
    v = joints_vis.to(device=j.device, dtype=torch.float32)
    if v.dim() == 3:
        v = v[..., 0]
    v = v.contiguous()
    n, nj, _ = j.shape
    hw, hh = int(heatmap_size[0]), int(heatmap_size[1])
    target = torch.empty((n, nj, hh, hw), dtype=torch.float32, device=j.device)
    weight = torch.empty((n, nj, 1), dtype=torch.float32, device=j.device)
    zw = None
    if zero_weight is not None:
        zw = torch.as_tensor(zero_weight, device=j.device).to(torch.uint8).contiguous()
    call('posu_gaussian_targets', ptr(j), ptr(v), n, nj, int(image_size[0]), int(image_size[1]), hw, hh,
         float(sigma), ptr(zw), ptr(target), ptr(weight), stream_of(j.device))
    return target, weight


def integral_preds(heatmaps):
    """[N, J, H, W] -> [N, J, 2] (x, y) sum-normalised integral coordinates."""
    require_cuda(heatmaps)
    h = heatmaps.float().contiguous()
    n, nj, hh, ww = h.shape
    out = torch.empty((n, nj, 2), dtype=torch.float32, device=h.device)
    call('posu_integral2d_fwd', ptr(h), n, nj, hh, ww, ptr(out), stream_of(h.device))
    return out


# ------------------------------------------------------------------ the training sample
# torchvision ColorJitter's fn_ids, the values of a jitter record's `order`
BRIGHTNESS, CONTRAST, SATURATION, HUE = 0, 1, 2, 3

# include/posu.h: posu_jitter (20 bytes, packed)
JITTER_DTYPE = np.dtype([('brightness', '<f4'), ('contrast', '<f4'), ('saturation', '<f4'), ('order', 'u1', (4,)),
                         ('hue_shift', 'u1'), ('active', 'u1'), ('reserved', 'u1', (2,))])

# joints_dataset_compatible.py:69-70
JITTER_BRIGHTNESS, JITTER_CONTRAST, JITTER_SATURATION, JITTER_HUE = (0.7, 3.0), (0.5, 2.0), (0.5, 2.0), 0.2


def jitter_records(n):
    """n inactive jitter records (JITTER_DTYPE): the identity order, factors 1, no hue shift."""
    rec = np.zeros(n, dtype=JITTER_DTYPE)
    rec['brightness'] = rec['contrast'] = rec['saturation'] = 1.0
    rec['order'] = np.arange(4, dtype=np.uint8)
    return rec


def _has_contrast(jitter):
    return bool(np.any((jitter['active'] != 0) & np.any(jitter['order'] == CONTRAST, axis=1)))


def _sample_images_dev(src, off, hw, M, flip, jitter, contrast, bgr, n, dh, dw, out, mean, std):
    """posu_sample_images on device tensors; returns (crops, workspace or None)."""
    require_cuda(src, off, hw, M, flip, jitter, mean, std)
    dev = src.device
    if out == 'u8':
        res = torch.empty((n, dh, dw, 3), dtype=torch.uint8, device=dev)
    else:
        res = torch.empty((n, 3, dh, dw), dtype=torch.float32, device=dev)
    ws = torch.empty(n, dtype=torch.int64, device=dev) if jitter is not None else None
    call('posu_sample_images', ptr(src), ptr(off), ptr(hw), 3, ptr(M), ptr(flip), ptr(jitter), int(contrast),
         int(bool(bgr)), n, dh, dw, 0 if out == 'u8' else 1, ptr(mean), ptr(std), ptr(ws),
         0 if ws is None else ws.numel() * 8, ptr(res), stream_of(dev))
    return res, ws


def sample_images(images, trans, image_size, device, flip=None, jitter=None, bgr=True, out='f32',
                  mean=IMAGENET_MEAN, std=IMAGENET_STD, return_workspace=False):
    """The input crops of N training records in one enqueue (JointsDatasetCompatible.__getitem__,
    joints_dataset_compatible.py:156-173): flip, cv2.warpAffine, ColorJitter, ToTensor + Normalize.

    images, trans, image_size, out, mean, std: as crop_warp's, three channels.  flip: None or [N] bool, the
    records whose source is mirrored before the warp (trans is then built from the mirrored centre).  jitter:
    None or [N] JITTER_DTYPE records (jitter_records / draw_augmentation).  bgr: the sources are cv2's BGR;
    the jitter works on RGB and the result is in the source's order again.  return_workspace: also return
    the [N] int64 sums of L that the contrast steps averaged (0 for records without one)."""
    if out not in ('u8', 'f32'):
        raise ValueError("out must be 'u8' or 'f32'")
    n = len(images)
    dw, dh = int(image_size[0]), int(image_size[1])
    src, off, hw, c = _upload_images(images, device)
    if c != 3:
        raise ValueError('sample_images expects three channels')
    require_cuda(src)
    M = torch.as_tensor(np.asarray(trans, dtype=np.float64).reshape(n, 6), device=device).contiguous()
    fl = None if flip is None else torch.as_tensor(np.asarray(flip).astype(np.uint8).reshape(n), device=device)
    jt, contrast = None, False
    if jitter is not None:
        jitter = np.ascontiguousarray(jitter, dtype=JITTER_DTYPE).reshape(n)
        contrast = _has_contrast(jitter)
        jt = torch.from_numpy(jitter.view(np.uint8).copy()).to(device)
    m = s = None
    if out == 'f32':
        m = torch.tensor(mean, dtype=torch.float32, device=device)
        s = torch.tensor(std, dtype=torch.float32, device=device)
        if m.numel() != 3 or s.numel() != 3:
            raise ValueError('mean / std need one value per channel')
    res, ws = _sample_images_dev(src, off, hw, M, fl, jt, contrast, bgr, n, dh, dw, out, m, s)
    if not contrast and ws is not None:
        ws.zero_()
    return (res, ws) if return_workspace else res


def sample_joints_targets(joints, joints_vis, trans, image_size, heatmap_size, sigma=2, flip=None, widths=None,
                          flip_order=None, zero_weight=None):
    """The label half of N training records in one launch (joints_dataset_compatible.py:157-158, :175-186):
    fliplr_joints, the crop affine for the visible joints, generate_heatmap; f64 where the reference is.

    joints [N, J, 2] and joints_vis [N, J, >= 2] (the first two columns are used): f64 cuda tensors in source
    px; trans [N, 2, 3]; flip None or [N] bool with widths [N] (the sources' widths) and flip_order [J]
    (utils.transforms.flip_pair_order); zero_weight None or [N] bool (H36M without pseudo labels).
    Returns (joints_2d_transformed [N, J, 2] f64, joints_vis [N, J, 2] f64, target [N, J, h, w] f32,
    target_weight [N, J, 1] f32)."""
    require_cuda(joints, joints_vis)
    dev = joints.device
    if joints.dtype != torch.float64 or joints_vis.dtype != torch.float64:
        raise TypeError('sample_joints_targets expects float64 joints and joints_vis (the db records)')
    n, nj, _ = joints.shape
    j = joints.contiguous()
    v = joints_vis[..., :2].contiguous()
    M = torch.as_tensor(np.asarray(trans, dtype=np.float64).reshape(n, 6) if not torch.is_tensor(trans) else trans,
                        device=dev).reshape(n, 6).contiguous()
    fl = hw = perm = None
    if flip is not None:
        if widths is None or flip_order is None:
            raise ValueError('flip needs the source widths and the flip order')
        order = [int(k) for k in flip_order]
        if sorted(order) != list(range(nj)):
            raise ValueError('flip_order must be a permutation of the %d joints' % nj)
        fl = torch.as_tensor(np.asarray(flip).astype(np.uint8).reshape(n), device=dev)
        w = np.asarray(widths, dtype=np.int32).reshape(n)
        hw = torch.as_tensor(np.stack([np.zeros_like(w), w], axis=1).reshape(-1), device=dev)
        perm = torch.tensor(order, dtype=torch.int32, device=dev)
    zw = None
    if zero_weight is not None:
        zw = torch.as_tensor(np.asarray(zero_weight).astype(np.uint8).reshape(n), device=dev)
    return _sample_joints_targets_dev(j, v, fl, hw, perm, M, zw, n, nj, image_size, heatmap_size, sigma)


def _sample_joints_targets_dev(j, v, fl, hw, perm, M, zw, n, nj, image_size, heatmap_size, sigma):
    require_cuda(j, v, fl, hw, perm, M, zw)
    dev = j.device
    hm_w, hm_h = int(heatmap_size[0]), int(heatmap_size[1])
    jout = torch.empty((n, nj, 2), dtype=torch.float64, device=dev)
    vout = torch.empty((n, nj, 2), dtype=torch.float64, device=dev)
    target = torch.empty((n, nj, hm_h, hm_w), dtype=torch.float32, device=dev)
    weight = torch.empty((n, nj, 1), dtype=torch.float32, device=dev)
    call('posu_sample_joints_targets', ptr(j), ptr(v), ptr(fl), ptr(hw), ptr(perm), ptr(M), ptr(zw), n, nj,
         int(image_size[0]), int(image_size[1]), hm_w, hm_h, float(sigma), ptr(jout), ptr(vout), ptr(target),
         ptr(weight), stream_of(dev))
    return jout, vout, target, weight


def draw_augmentation(records, aug_param_dict, is_train, color_jitter, rng):
    """The random draws of __getitem__ (joints_dataset_compatible.py:148-159, :67-71) for a list of db
    records, on the host from a numpy.random.Generator.  The draws follow the reference's distributions, not
    its random streams (np.random / random / torch): a seed gives other values than the reference's.

    Drawn only when is_train and the record's source is not 'h36m': the scale factor
    clip(randn * sf + 1, 1 - sf, 1 + sf), the rotation clip(randn * rf, -2 rf, 2 rf) with probability 0.6
    (else 0), the flip with probability 0.5 where the source's 'flip' is set.  With color_jitter, for every
    record: a uniformly random order of the four operations, brightness from U(0.7, 3.0), contrast and
    saturation from U(0.5, 2.0), hue from U(-0.2, 0.2) stored as hue_shift = trunc(hue * 255) mod 256.

    Returns {'scale_factor': [N] f64, 'rotation': N numbers (the int 0 where none was drawn), 'flip': [N]
    bool, 'jitter': None or [N] JITTER_DTYPE}."""
    n = len(records)
    scale_factor, rotation, flip = np.ones(n), [0] * n, np.zeros(n, dtype=bool)
    for k, rec in enumerate(records):
        if not (is_train and rec['source'] != 'h36m'):
            continue
        par = aug_param_dict[rec['source']]
        sf, rf = par['scale_factor'], par['rotation_factor']
        scale_factor[k] = np.clip(rng.standard_normal() * sf + 1, 1 - sf, 1 + sf)
        if rng.random() <= 0.6:
            rotation[k] = float(np.clip(rng.standard_normal() * rf, -rf * 2, rf * 2))
        flip[k] = bool(par['flip']) and rng.random() <= 0.5
    jitter = None
    if color_jitter:
        jitter = jitter_records(n)
        jitter['active'] = 1
        for k in range(n):
            jitter['order'][k] = rng.permutation(4)
            jitter['brightness'][k] = rng.uniform(*JITTER_BRIGHTNESS)
            jitter['contrast'][k] = rng.uniform(*JITTER_CONTRAST)
            jitter['saturation'][k] = rng.uniform(*JITTER_SATURATION)
            jitter['hue_shift'][k] = hue_shift_of(rng.uniform(-JITTER_HUE, JITTER_HUE))
    return {'scale_factor': scale_factor, 'rotation': rotation, 'flip': flip, 'jitter': jitter}


def hue_shift_of(hue):
    """adjust_hue's uint8 add of hue * 255: truncated toward zero, then mod 256 (-0.1 -> 231)."""
    return int(np.trunc(hue * 255)) % 256


def _align8(k):
    return (k + 7) // 8 * 8


class BatchMaker:
    """Training batches on the device: what JointsDatasetCompatible.__getitem__ (per sample) and the
    DataLoader's collate give, made by two enqueues for the whole batch.

    cfg: NETWORK.IMAGE_SIZE / HEATMAP_SIZE / SIGMA, DATASET.COLOR_JITTER (absent = off); aug_param_dict:
    per source {'scale_factor', 'rotation_factor', 'flip'}; flip_pairs: the dataset's left / right pairs;
    pseudo_label: H36M records carry joints_2d_pseudo / joints_vis_pseudo and keep their weights.  Image
    decoding, the db and its grouping stay with the caller."""

    def __init__(self, cfg, is_train, aug_param_dict, flip_pairs, pseudo_label=False, device='cuda', rng=None,
                 mean=IMAGENET_MEAN, std=IMAGENET_STD, bgr=True):
        from utils.transforms import flip_pair_order
        self.image_size = [int(v) for v in cfg.NETWORK.IMAGE_SIZE]
        self.heatmap_size = [int(v) for v in cfg.NETWORK.HEATMAP_SIZE]
        self.sigma = cfg.NETWORK.SIGMA
        self.num_joints = 16
        self.is_train, self.aug_param_dict, self.pseudo_label = is_train, aug_param_dict, pseudo_label
        self.color_jitter = bool(getattr(cfg.DATASET, 'COLOR_JITTER', False))
        self.flip_order = flip_pair_order(self.num_joints, flip_pairs)
        self.device = torch.device(device)
        if self.device.type != 'cuda':
            raise RuntimeError('BatchMaker runs only on the MI355X HIP path; got a CPU device (use a cuda device)')
        self.rng = rng if rng is not None else np.random.default_rng()
        self.bgr = bgr
        self._mean = torch.tensor(mean, dtype=torch.float32, device=self.device)
        self._std = torch.tensor(std, dtype=torch.float32, device=self.device)
        self._perm = torch.tensor(self.flip_order, dtype=torch.int32, device=self.device)

    def draw(self, records):
        return draw_augmentation(records, self.aug_param_dict, self.is_train, self.color_jitter, self.rng)

    def _host_half(self, records, images, aug):
        """Per record on the host, f64: the mirrored centre, the drawn scale, the crop affine and the label
        source (joints_dataset_compatible.py:134-161)."""
        from utils.transforms import get_affine_transform
        n = len(records)
        nj = self.num_joints
        joints, vis = np.empty((n, nj, 2)), np.empty((n, nj, 2))
        centers, scales, trans = np.empty((n, 2)), np.empty((n, 2)), np.empty((n, 6))
        zero_w = np.zeros(n, dtype=np.uint8)
        for k, rec in enumerate(records):
            pseudo = rec['source'] == 'h36m' and self.pseudo_label
            j = np.asarray(rec['joints_2d_pseudo' if pseudo else 'joints_2d'], dtype=np.float64)
            v = np.asarray(rec['joints_vis_pseudo' if pseudo else 'joints_vis'], dtype=np.float64)
            assert len(j) == nj and len(v) == nj
            joints[k], vis[k] = j[:, :2], v[:, :2]
            center = np.array(rec['center'], dtype=np.float64)
            scale = np.array(rec['scale'], dtype=np.float64) * aug['scale_factor'][k]
            if aug['flip'][k]:
                center[0] = images[k].shape[1] - center[0] - 1
            centers[k], scales[k] = center, scale
            trans[k] = get_affine_transform(center, scale, aug['rotation'][k], self.image_size).reshape(6)
            zero_w[k] = rec['source'] == 'h36m' and not self.pseudo_label
        return joints, vis, centers, scales, trans, zero_w

    def _enqueue(self, records, images, aug):
        """One upload of the small tables, one of the sources, the two calls -> device tensors of the whole
        list of records."""
        n = len(records)
        if len(images) != n:
            raise ValueError('one image per record')
        joints, vis, centers, scales, trans, zero_w = self._host_half(records, images, aug)
        flat, offs, shapes = _flatten_images(images)
        if any(sh[2] != 3 for sh in shapes):
            raise ValueError('BatchMaker expects three-channel images')
        jitter = aug['jitter']
        parts = [trans, joints.reshape(-1), vis.reshape(-1), np.asarray(offs[:-1], dtype=np.int64),
                 np.array([[sh[0], sh[1]] for sh in shapes], dtype=np.int32).reshape(-1),
                 np.asarray(aug['flip']).astype(np.uint8), zero_w]
        if jitter is not None:
            parts.append(np.ascontiguousarray(jitter, dtype=JITTER_DTYPE).reshape(n).view(np.uint8))
        starts = np.cumsum([0] + [_align8(p.nbytes) for p in parts])
        host = np.zeros(int(starts[-1]), dtype=np.uint8)
        for p, s in zip(parts, starts):
            host[s:s + p.nbytes] = np.ascontiguousarray(p).reshape(-1).view(np.uint8)
        table = torch.from_numpy(host).to(self.device)
        dev = [table[s:s + p.nbytes] for p, s in zip(parts, starts)]
        M, j, v = (d.view(torch.float64) for d in dev[:3])
        off, hw, fl, zw = dev[3].view(torch.int64), dev[4].view(torch.int32), dev[5], dev[6]
        jt = dev[7] if jitter is not None else None
        if all(torch.is_tensor(f) and f.is_cuda for f in flat):
            src = torch.cat(flat)
        else:
            src = torch.cat([f.cpu() for f in flat]).to(self.device)
        dw, dh = self.image_size
        contrast = jitter is not None and _has_contrast(jitter)
        inp, _ = _sample_images_dev(src, off, hw, M.view(n, 6), fl, jt, contrast, self.bgr, n, dh, dw, 'f32',
                                    self._mean, self._std)
        jout, vout, target, weight = _sample_joints_targets_dev(
            j.view(n, -1, 2), v.view(n, -1, 2), fl, hw, self._perm, M.view(n, 6), zw, n, self.num_joints,
            self.image_size, self.heatmap_size, self.sigma)
        return inp, target, weight, jout, vout, centers, scales

    @staticmethod
    def _meta(records, aug, rows, centers, scales, jout, vout):
        """default_collate of the per-sample meta dicts (joints_dataset_compatible.py:191-200) for the records
        `rows`: f64 tensors, the rotation int64 while nothing was drawn, source a list, subject int64.
        joints_2d_transformed and joints_vis stay on the device that computed them."""
        recs = [records[k] for k in rows]
        rot = [aug['rotation'][k] for k in rows]
        return {
            'scale': torch.from_numpy(scales[rows]),
            'center': torch.from_numpy(centers[rows]),
            'rotation': torch.tensor(rot, dtype=torch.int64 if all(isinstance(r, int) for r in rot)
                                     else torch.float64),
            'joints_2d': torch.from_numpy(np.stack([np.asarray(r['joints_2d'], dtype=np.float64) for r in recs])),
            'joints_2d_transformed': jout[rows[0]:rows[-1] + 1],
            'joints_vis': vout[rows[0]:rows[-1] + 1],
            'source': [r['source'] for r in recs],
            'subject': torch.tensor([int(r['subject']) if r['source'] == 'h36m' else -1 for r in recs],
                                    dtype=torch.int64),
        }

    def __call__(self, records, images, aug=None):
        """records: N db records (center, scale, joints_2d, joints_vis, source, subject; with pseudo_label
        also joints_2d_pseudo / joints_vis_pseudo); images: their decoded uint8 [H, W, 3] images (numpy or
        cuda tensors); aug: draw_augmentation's result (drawn here when None).
        Returns (input [N, 3, h, w], target [N, J, hh, hw], target_weight [N, J, 1], meta)."""
        aug = self.draw(records) if aug is None else aug
        inp, target, weight, jout, vout, centers, scales = self._enqueue(records, images, aug)
        rows = list(range(len(records)))
        return inp, target, weight, self._meta(records, aug, rows, centers, scales, jout, vout)

    def multiview(self, groups, images, aug=None):
        """groups: [B][V] records, images: [B][V] images (aug over the B * V records group by group) -> the
        four lists over the V views that MultiViewH36MCompatible.__getitem__ plus the collate give: input[v]
        [B, 3, h, w], target[v], weight[v], meta[v] -- core.function.train's batch, from one enqueue of
        V * B frames."""
        nb, nv = len(groups), len(groups[0])
        if any(len(g) != nv for g in groups):
            raise ValueError('every group needs the same number of views')
        # view-major, so that every view's rows are one contiguous block of the outputs
        order = [(b, v) for v in range(nv) for b in range(nb)]
        records = [groups[b][v] for b, v in order]
        imgs = [images[b][v] for b, v in order]
        if aug is None:
            aug = self.draw(records)
        else:
            pick = [b * nv + v for b, v in order]
            aug = {'scale_factor': np.asarray(aug['scale_factor'])[pick], 'rotation': [aug['rotation'][k] for k in pick],
                   'flip': np.asarray(aug['flip'])[pick],
                   'jitter': None if aug['jitter'] is None else aug['jitter'][pick]}
        inp, target, weight, jout, vout, centers, scales = self._enqueue(records, imgs, aug)
        views = [list(range(v * nb, (v + 1) * nb)) for v in range(nv)]
        return ([inp[r[0]:r[-1] + 1] for r in views], [target[r[0]:r[-1] + 1] for r in views],
                [weight[r[0]:r[-1] + 1] for r in views],
                [self._meta(records, aug, r, centers, scales, jout, vout) for r in views])
