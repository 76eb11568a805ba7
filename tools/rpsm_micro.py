"""Micro-benchmark of the RPSM 3-D lifter (multiviews.pictorial.rpsm_batch, csrc/rpsm.hip) at the
reference's production grid: FIRST_NBINS 16 (N = 4096), RECUR_NBINS 2, RECUR_DEPTH 10, 32 x 32
heatmaps, G groups of 4 views per call.  HIP events around the enqueue (posu_rpsm_run on
prepared device tensors), after warm-up, median of the repeats; level 1 is the same call with
RECUR_DEPTH 0, the recursion is the difference.  `call_ms` is rpsm_batch as a user calls it
(host camera / affine tables, upload, launch, wait).  Beside it the numpy restatement
(tools/rpsm_synthetic.py rpsm_numpy) of one group on the host.

    python tools/rpsm_micro.py [--groups 1,32,128] [--first-nbins 16] [--depth 10] [--reps 7] [--no-cpu]

Prints one JSON line per batch size.
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

from multiviews import pictorial as P  # noqa: E402
from multiviews.body import HumanBody  # noqa: E402
from posu import ops  # noqa: E402

sys.path.insert(0, os.path.join(REPO, 'tools'))
import rpsm_synthetic as rs  # noqa: E402


def event_ms(fn, warmup, reps):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    out = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        out.append(a.elapsed_time(b))
    return statistics.median(out)


def wall_ms(fn, warmup, reps):
    for _ in range(warmup):
        fn()
    out = []
    for _ in range(reps):
        torch.cuda.synchronize()
        t = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        out.append((time.perf_counter() - t) * 1e3)
    return statistics.median(out)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--groups', default='1,32,128')
    ap.add_argument('--first-nbins', type=int, default=16)
    ap.add_argument('--grid-size', type=float, default=2000.0)
    ap.add_argument('--depth', type=int, default=10)
    ap.add_argument('--heatmap', type=int, default=32)
    ap.add_argument('--distinct', type=int, default=4, help='distinct synthetic groups, tiled to the batch')
    ap.add_argument('--warmup', type=int, default=2)
    ap.add_argument('--reps', type=int, default=7)
    ap.add_argument('--no-cpu', action='store_true')
    args = ap.parse_args()
    dev = torch.device('cuda', 0)
    torch.set_num_threads(min(16, os.cpu_count() or 1))
    body = HumanBody()
    tree = P._tree(body)
    rng = np.random.RandomState(3)
    base = [rs.make_group(rng, args.grid_size, (150, 450), args.heatmap) for _ in range(args.distinct)]
    limbs = base[0]['limb_length']          # the level-1 constraint's; every group refines with its own
    t = time.perf_counter()
    packed = P.compute_pairwise_constraint(args.grid_size, limbs, args.first_nbins)
    mask = packed.mask(dev)
    torch.cuda.synchronize()
    mask_ms = (time.perf_counter() - t) * 1e3
    cpu_ms = None
    if not args.no_cpu:
        cfg = rs.make_config(args.first_nbins, args.grid_size, args.depth, args.heatmap)
        dense = packed.dense()
        t = time.perf_counter()
        ref = rs.rpsm_numpy(base[0], dense, cfg)
        cpu_ms = (time.perf_counter() - t) * 1e3
        got = P.rpsm(base[0]['cams'], base[0]['heatmaps'], base[0]['boxes'], base[0]['center'], limbs, packed, cfg)
        assert float(np.abs(got - ref).max()) <= 1e-6, 'GPU and numpy poses differ'
    for g in [int(x) for x in args.groups.split(',')]:
        grp = [base[i % len(base)] for i in range(g)]
        cams = [c for x in grp for c in x['cams']]
        boxes = [b for x in grp for b in x['boxes']]
        hm = torch.from_numpy(np.stack([x['heatmaps'] for x in grp])).to(dev)
        centers = np.stack([x['center'] for x in grp])
        rows = P._dev_f64(P._camera_rows(cams), dev)
        aff = P._dev_f64(P._affines(boxes, [rs.IMAGE, rs.IMAGE]), dev)
        cdev = P._dev_f64(centers, dev)
        group_limbs = [x['limb_length'] for x in grp]
        limb = P._dev_f64(P._limb_rows(group_limbs, tree, g), dev)

        def run(depth):
            return ops.rpsm_run(hm, rows, aff, [rs.IMAGE, rs.IMAGE], cdev, args.grid_size, args.first_nbins, 2, depth,
                                150.0, limb, mask, tree)

        full = event_ms(lambda: run(args.depth), args.warmup, args.reps)
        level1 = event_ms(lambda: run(0), args.warmup, args.reps)
        cfg = rs.make_config(args.first_nbins, args.grid_size, args.depth, args.heatmap)
        call = wall_ms(lambda: P.rpsm_batch(cams, hm, boxes, centers, group_limbs, packed, cfg), 1, max(3, args.reps // 2))
        print(json.dumps({'tool': 'rpsm_micro', 'groups': g, 'first_nbins': args.first_nbins, 'depth': args.depth,
                          'gpu_ms': round(full, 4), 'level1_ms': round(level1, 4),
                          'recursion_ms': round(full - level1, 4), 'gpu_ms_per_group': round(full / g, 4),
                          'call_ms': round(call, 3), 'mask_build_ms': round(mask_ms, 2),
                          'cpu_numpy_ms_one_group': None if cpu_ms is None else round(cpu_ms, 1)}), flush=True)


if __name__ == '__main__':
    main()
