"""Time a training batch made on the device (posu.datapath.BatchMaker.multiview: host affines, one upload of
the tables, posu_sample_images + posu_sample_joints_targets) with and without the colour jitter, against the
plain crop and targets this build had before (posu.datapath.crop_warp + generate_heatmaps on the same crops:
no flip, no jitter, joints in f32).  Default: 32 groups x 4 views, 1000 x 1000 sources -> 256 x 256.

    python tools/sample_batch_micro.py [--groups 32] [--src 1000] [--size 256] [--reps 20] [--out FILE]

Three numbers per variant, each the median of the repeats after warm-up: the whole call from host images
(wall clock to a device synchronise: the 3 MB-per-frame upload is part of it), the whole call from sources
already on the device, and the kernels alone (device events around the enqueues on prepared tensors).
Prints JSON lines and writes them to --out.
"""
import argparse
import json
import os
import statistics
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(REPO, 'pose-unsupervised_amd', 'lib'), REPO]

import numpy as np  # noqa: E402
import torch  # noqa: E402

from posu import datapath  # noqa: E402
from posu import synthetic as syn  # noqa: E402

AUG = {'mpii': {'scale_factor': 0.25, 'rotation_factor': 30, 'flip': True}}
FLIP_PAIRS = [[0, 5], [1, 4], [2, 3], [10, 15], [11, 14], [12, 13]]


def make_groups(ngroups, src, seed=0):
    r = np.random.default_rng(seed)
    groups, images = [], []
    for _ in range(ngroups):
        recs, imgs = [], []
        for _ in range(4):
            recs.append({'center': r.uniform(0.4, 0.6, 2) * src, 'scale': np.full(2, src / 200.0 * r.uniform(0.8, 1.1)),
                         'joints_2d': r.uniform(0.1, 0.9, (16, 2)) * src,
                         'joints_vis': (r.uniform(size=(16, 1)) > 0.1).astype(np.float64).repeat(3, axis=1),
                         'source': 'mpii', 'subject': 0})
            imgs.append(r.integers(0, 256, (src, src, 3), dtype=np.uint8))
        groups.append(recs)
        images.append(imgs)
    return groups, images


def wall(fn, reps):
    fn()
    torch.cuda.synchronize()
    times = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        times.append((time.perf_counter() - t0) * 1e3)
    return statistics.median(times), min(times), max(times)


def events(fn, reps):
    fn()
    torch.cuda.synchronize()
    times = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        times.append(a.elapsed_time(b))
    return statistics.median(times), min(times), max(times)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--groups', type=int, default=32)
    ap.add_argument('--src', type=int, default=1000)
    ap.add_argument('--size', type=int, default=256)
    ap.add_argument('--reps', type=int, default=20)
    ap.add_argument('--out', default='')
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('sample_batch_micro needs the GPU: nothing is measured without one')
    dev = torch.device('cuda', 0)
    cfg = syn.train_loop_cfg(image_size=args.size, sigma=2)
    size, hm = [args.size] * 2, [int(v) for v in cfg.NETWORK.HEATMAP_SIZE]
    groups, images = make_groups(args.groups, args.src)
    dev_images = [[torch.from_numpy(im).to(dev) for im in g] for g in images]
    lines = []

    def report(name, **kw):
        line = dict(name=name, groups=args.groups, frames=args.groups * 4, src=args.src, size=args.size, **kw)
        lines.append(json.dumps(line))
        print(lines[-1], flush=True)

    for jitter in (True, False):
        cfg.DATASET.COLOR_JITTER = jitter
        maker = datapath.BatchMaker(cfg, True, AUG, FLIP_PAIRS, device=dev, rng=np.random.default_rng(1))
        aug = maker.draw([r for g in groups for r in g])
        name = 'multiview_jitter' if jitter else 'multiview_plain'
        report(name + '.host_images', ms=wall(lambda: maker.multiview(groups, images, aug), max(3, args.reps // 4)))
        report(name + '.device_images', ms=wall(lambda: maker.multiview(groups, dev_images, aug), args.reps))
        # the two enqueues alone, on the tensors multiview prepares
        order = [(b, v) for v in range(4) for b in range(args.groups)]
        records = [groups[b][v] for b, v in order]
        imgs = [dev_images[b][v] for b, v in order]
        pick = [b * 4 + v for b, v in order]
        sub = {'scale_factor': aug['scale_factor'][pick], 'rotation': [aug['rotation'][k] for k in pick],
               'flip': aug['flip'][pick], 'jitter': None if aug['jitter'] is None else aug['jitter'][pick]}
        n = len(records)
        joints, vis, _, _, trans, zero_w = maker._host_half(records, imgs, sub)
        src, off, hw, _ = datapath._upload_images(imgs, dev)
        M = torch.from_numpy(trans).to(dev)
        fl = torch.from_numpy(sub['flip'].astype(np.uint8)).to(dev)
        jt = None if sub['jitter'] is None else torch.from_numpy(sub['jitter'].view(np.uint8).copy()).to(dev)
        j, v = torch.from_numpy(joints).to(dev), torch.from_numpy(vis).to(dev)
        zw = torch.from_numpy(zero_w).to(dev)
        report(name + '.images_kernels', ms=events(lambda: datapath._sample_images_dev(
            src, off, hw, M, fl, jt, jt is not None, True, n, args.size, args.size, 'f32', maker._mean, maker._std),
            args.reps))
        report(name + '.labels_kernel', ms=events(lambda: datapath._sample_joints_targets_dev(
            j, v, fl, hw, maker._perm, M, zw, n, 16, size, hm, 2), args.reps))

    # the baseline: the plain crop and the f32 targets on the same crops
    flat = [im for g in dev_images for im in g]
    recs = [r for g in groups for r in g]
    from utils.transforms import get_affine_transform
    trans = np.stack([get_affine_transform(r['center'], r['scale'], 0, size) for r in recs])
    jc = torch.from_numpy(np.stack([r['joints_2d'] for r in recs])).to(dev)
    jv = torch.from_numpy(np.stack([r['joints_vis'] for r in recs])).to(dev)

    def baseline():
        x = datapath.crop_warp(flat, trans, size, dev)
        return x, datapath.generate_heatmaps(jc, jv, size, hm, sigma=2)
    report('baseline_crop_warp_heatmaps.device_images', ms=wall(baseline, args.reps))
    report('baseline_crop_warp_heatmaps.events', ms=events(baseline, args.reps))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, 'w') as f:
            f.write('\n'.join(lines) + '\n')


if __name__ == '__main__':
    main()
