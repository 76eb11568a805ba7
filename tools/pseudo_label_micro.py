"""Time one pseudo-label round (multiviews.pseudo_label.pseudo_label_round: one upload, one
posu_pseudo_label_sweep, one posu_pckh_counts, one read-back) against the same sweep done the way the
reference's script does it on this build's drop-in functions: per threshold one multiviews.triangulate.ransac
and one reproject_poses call (each uploads its inputs and reads its result back) with the scoring in numpy
on the host.  H36M training-set size by default: 2215 groups x 4 views x 16 joints, T = 4 thresholds.

    python tools/pseudo_label_micro.py [--groups 2215] [--reps 20] [--out profiles/r11/pseudo_label_micro.txt]

Wall clock around whole calls (host work is part of both), after warm-up, median of the repeats; the two
kernels alone are also event-timed on prepared device tensors.  Prints JSON lines and writes them to --out.

    python tools/pseudo_label_micro.py --digest

No timing: the fp64 geometry entry points (posu_triangulate_dlt, posu_ransac_inliers, posu_reproject,
posu_pseudo_label_sweep, posu_pckh_counts) on small seeded inputs that reach every branch, one sha1 per output
tensor.  Two builds (tools/with_lib.py) compute the same bits when their listings are equal line for line.
"""
import argparse
import hashlib
import json
import os
import statistics
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(REPO, 'pose-unsupervised_amd', 'lib'), REPO, os.path.join(REPO, 'tests')]

import numpy as np  # noqa: E402
import torch  # noqa: E402

from multiviews import pseudo_label as pl  # noqa: E402
from multiviews.triangulate import camera_tables, ransac, reproject_poses  # noqa: E402
from posu import ops  # noqa: E402
from posu import synthetic as syn  # noqa: E402


def make_inputs(ngroups, seed=3):
    """Cameras of the synthetic rigs, noisy projections with gross outliers, confidences, ground truth, heads."""
    cams = syn.group_cameras(ngroups, distortion=True)
    M, intr = camera_tables(cams, 4, no_distortion=True)
    poses = syn.synthetic_poses3d(ngroups)
    X = np.concatenate([poses, np.ones(poses.shape[:2] + (1,))], axis=2)
    P = np.einsum('gvrc,gjc->gvjr', M, X)                               # pinhole ground truth: inputs only
    gt2d = (P[..., :2] / P[..., 2:]).reshape(ngroups * 4, -1, 2)
    r = np.random.default_rng(seed)
    p2d = gt2d + r.normal(0, 1.5, size=gt2d.shape)
    bad = r.uniform(size=p2d.shape[:2]) < 0.15
    p2d[bad] += r.choice([-1, 1], size=(bad.sum(), 2)) * r.uniform(60, 120, size=(bad.sum(), 2))
    conf = r.uniform(0.3, 1.1, size=p2d.shape[:2])
    loc = np.concatenate([p2d, conf[:, :, None]], axis=2).astype(np.float32)
    head = pl.headsizes_from_scales(r.uniform(0.1, 0.4, size=(ngroups * 4, 2)))
    return cams, loc, gt2d, head


def numpy_eval(pred2d, gt2d, joints_vis, headsizes, threshold=0.5):
    """my_eval's arithmetic and the script's coverage lines, on the host."""
    d = np.sqrt(np.sum((gt2d - pred2d) ** 2, axis=2)) / headsizes
    det = (d <= threshold) * joints_vis
    with np.errstate(invalid='ignore', divide='ignore'):
        rate = np.sum(det, axis=0) / np.sum(joints_vis, axis=0).astype(np.float32)
        ratio = np.sum(joints_vis, axis=0) / np.sum(joints_vis).astype(np.float32)
    per = np.sum(np.reshape(joints_vis, (-1, 4, joints_vis.shape[1])), axis=1)
    return np.sum(ratio * rate), np.sum(joints_vis) / joints_vis.size, [np.sum(per == c) / per.size for c in range(5)]


def per_threshold_round(loc, cams, gt2d, head, cfg, thresholds):
    """The script's loop on the per-call functions: what a user of this build wrote before the round existed."""
    pred2d, conf = loc[:, :, :2], loc[:, :, 2]
    out = []
    for thre in thresholds:
        vis = conf > thre
        out.append(numpy_eval(pred2d, gt2d, vis, head))
        vis = ransac(pred2d, cams, vis, cfg)
        out.append(numpy_eval(pred2d, gt2d, vis, head))
        proj, vis = reproject_poses(pred2d, cams, vis, cfg.DATASET.NO_DISTORTION)
        out.append(numpy_eval(proj, gt2d, vis, head))
    return out


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
    return statistics.median(out), min(out), max(out)


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
    return statistics.median(out), min(out), max(out)


def sha(t):
    return hashlib.sha1(t.contiguous().view(torch.uint8).cpu().numpy().tobytes()).hexdigest()[:12]


def digest():
    import pseudo_label_restatement as rs
    dev = torch.device('cuda', 0)

    def line(tag, *outs):
        torch.cuda.synchronize()
        print('%-66s %s' % (tag, ' '.join(sha(o) for o in outs)), flush=True)

    def up(a):
        return torch.from_numpy(np.ascontiguousarray(a)).to(dev)

    # triangulation: V = 2, 3, 4 take the register kernel, 5 and 16 the folded one.  Seven groups of 16 joints
    # are two blocks.  View v of group g is camera v % 4 of rig g + v // 4; the pixels are the pinhole
    # projections plus noise; the mask hides views at random and leaves joints 3 (one view) and 7 (none).
    G, J = 7, 16
    poses = syn.synthetic_poses3d(G)
    X1 = np.concatenate([poses, np.ones((G, J, 1))], axis=2)
    for distortion in (True, False):
        M4, I4 = camera_tables(syn.group_cameras(G, distortion=distortion), 4, no_distortion=not distortion)
        for V in (2, 3, 4, 5, 16):
            pick = [[((g + v // 4) % G, v % 4) for v in range(V)] for g in range(G)]
            M = np.stack([[M4[a, b] for a, b in row] for row in pick])
            intr = np.stack([[I4[a, b] for a, b in row] for row in pick])
            P = np.einsum('gvrc,gjc->gvjr', M, X1)
            r = np.random.default_rng(100 + V)
            xy = P[..., :2] / P[..., 2:] + r.normal(0, 1.5, size=(G, V, J, 2))
            vis = (r.uniform(size=(G, V, J)) < 0.7).astype(np.uint8)
            vis[:, 1:, 3] = 0
            vis[:, 0, 3] = 1
            vis[:, :, 7] = 0
            Md, Id, visd = up(M), up(intr), up(vis)
            for dt in (torch.float32, torch.float64):
                xyd = up(xy).to(dt)
                tag = 'triangulate_dlt V=%d %s %s' % (V, str(dt).split('.')[1], 'distorted' if distortion else 'pinhole')
                line(tag, ops.triangulate_dlt(Md, Id, xyd, None, undistort=distortion),
                     ops.triangulate_dlt(Md, Id, xyd, visd, undistort=distortion))
            if V == 4:
                xv = up(np.ascontiguousarray(xy.transpose(1, 0, 2, 3)))
                line('triangulate_dlt V=4 float64 view-major', ops.triangulate_dlt(Md, Id, xv, visd, distortion, True))

    # the per-threshold entry points and the sweep at the GPU tests' cases (tests/pseudo_label_restatement.py)
    cases = [(name, rs.make_inputs(rs.SEEDS[name], rs.CASES[name][0], rs.CASES[name][1]), 4, rs.CASES[name][1],
              rs.CASES[name][2]) for name in rs.CASES]
    cases.append(('v3', rs.make_v3_inputs(), 3, True, [0.6]))
    for name, inp, V, distortion, thresholds in cases:
        M, intr = (up(a) for a in camera_tables(inp['cams'], V, no_distortion=not distortion))
        loc = up(inp['locations'])
        g = len(inp['cams']) // V
        xy = loc[:, :, :2].double().reshape(g, V, -1, 2).contiguous()
        conf = loc[:, :, 2].reshape(g, V, -1).contiguous()
        hide = conf > 0.6                                  # a mask that hides views
        for inliers in rs.INLIERS:
            line('%s ransac_inliers INLIERS=%d' % (name, inliers),
                 ops.ransac_inliers(M, intr, xy, None, rs.REPROJ_THRE, inliers, undistort=distortion),
                 ops.ransac_inliers(M, intr, xy, hide, rs.REPROJ_THRE, inliers, undistort=distortion))
        line('%s reproject' % name, *(ops.reproject(M, intr, xy, None, undistort=distortion) +
                                      ops.reproject(M, intr, xy, hide, undistort=distortion)))
        for use_ransac in (True, False):
            for inliers in rs.INLIERS:
                masks, proj = ops.pseudo_label_sweep(M, intr, xy, conf, thresholds, rs.REPROJ_THRE, inliers, use_ransac,
                                                     undistort=distortion)
                line('%s pseudo_label_sweep ransac=%d INLIERS=%d' % (name, use_ransac, inliers), masks, proj)
                if inliers != rs.GOLDEN_INLIERS or not use_ransac:
                    continue
                t, n, nj = len(thresholds), g * V, xy.shape[2]
                gt, head = up(inp['gt2d']), up(inp['headsizes'])
                sel = [s for i in range(t) for s in (-1, -1, i)]
                line('%s pckh_counts' % name,
                     ops.pckh_counts(xy.reshape(n, nj, 2), masks.reshape(t * 3, n, nj), gt, head, V, 0.5,
                                     pred_sets=proj.reshape(t, n, nj, 2), set_pred=sel),
                     ops.pckh_counts(None, masks.reshape(t * 3, n, nj), None, None, V))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--digest', action='store_true', help='no timing: one sha1 per output tensor at small shapes')
    ap.add_argument('--groups', type=int, default=2215)
    ap.add_argument('--warmup', type=int, default=3)
    ap.add_argument('--reps', type=int, default=20)
    ap.add_argument('--out', default=os.path.join(REPO, 'profiles', 'r11', 'pseudo_label_micro.txt'))
    args = ap.parse_args()
    if args.digest:
        return digest()
    if args.reps < 20:
        ap.error('--reps must be at least 20')
    dev = torch.device('cuda', 0)
    G, J, thresholds = args.groups, 16, [0.6, 0.7, 0.8, 0.9]
    cams, loc, gt2d, head = make_inputs(G)
    cfg = syn.make_cfg()
    cfg.PSEUDO_LABEL.NUM_INLIERS, cfg.PSEUDO_LABEL.REPROJ_THRE = 3, 10
    cfg.PSEUDO_LABEL.IF_RANSAC, cfg.PSEUDO_LABEL.USE_REPROJ, cfg.PSEUDO_LABEL.IF_LOOP = True, True, False

    # the two ways agree before either is timed
    records = pl.pseudo_label_round(loc, cams, gt2d, head, cfg)
    old = per_threshold_round(loc, cams, gt2d, head, cfg, thresholds)
    for i in range(len(thresholds)):
        r0, r1 = records[2 * i], records[2 * i + 1]
        # reproject_poses hands its projections back in the predictions' float32: a detection a hair from its
        # threshold may fall the other way there, so the last stage's PCKh is compared loosely
        for got, want, tol in ((r0, old[3 * i], 1e-12), (r0['ransac'], old[3 * i + 1], 1e-12),
                               (r1, old[3 * i + 2], 1e-3)):
            assert got['vis_share'] == want[1] and np.array_equal(got['joints_at'], want[2])
            assert abs(got['pckh'] - want[0]) <= tol, (got['pckh'], want[0])

    lines = []

    def report(what, ms, how):
        lines.append(json.dumps({'tool': 'pseudo_label_micro', 'what': what, 'groups': G, 'views': 4, 'joints': J,
                                 'thresholds': len(thresholds), 'reps': args.reps, 'ms_median': round(ms[0], 3),
                                 'ms_min': round(ms[1], 3), 'ms_max': round(ms[2], 3), 'timed': how}))
        print(lines[-1], flush=True)

    report('pseudo_label_round', wall_ms(lambda: pl.pseudo_label_round(loc, cams, gt2d, head, cfg),
                                         args.warmup, args.reps),
           'wall clock: camera tables, one upload, two launches, one read-back, records')
    report('per-threshold ransac + reproject_poses + numpy scoring',
           wall_ms(lambda: per_threshold_round(loc, cams, gt2d, head, cfg, thresholds), args.warmup, args.reps),
           'wall clock: per call camera tables, upload, launch, read-back; scoring on the host')
    M, intr = (torch.from_numpy(a).to(dev) for a in camera_tables(cams, 4, False))
    locd = torch.from_numpy(loc).to(dev)
    xy = locd[:, :, :2].double().reshape(G, 4, J, 2).contiguous()
    conf = locd[:, :, 2].reshape(G, 4, J).contiguous()
    masks, proj = ops.pseudo_label_sweep(M, intr, xy, conf, thresholds, 10.0, 3, True)
    report('posu_pseudo_label_sweep', event_ms(
        lambda: ops.pseudo_label_sweep(M, intr, xy, conf, thresholds, 10.0, 3, True, vis_out=masks, proj_out=proj),
        args.warmup, args.reps), 'HIP events around the wrapper, outputs preallocated')
    vis0 = masks[0, 0].contiguous()
    report('posu_ransac_inliers + posu_reproject, one threshold', event_ms(
        lambda: ops.reproject(M, intr, xy, ops.ransac_inliers(M, intr, xy, vis0, 10.0, 3)), args.warmup, args.reps),
        'HIP events around the two wrappers')
    gt, hd = torch.from_numpy(gt2d).to(dev), torch.from_numpy(head).to(dev)
    sel = [s for i in range(len(thresholds)) for s in (-1, -1, i)]
    pred = xy.reshape(G * 4, J, 2)
    report('posu_pckh_counts, 12 sets', event_ms(
        lambda: ops.pckh_counts(pred, masks.reshape(12, G * 4, J), gt, hd, 4, 0.5, pred_sets=proj.reshape(4, -1, J, 2),
                                set_pred=sel), args.warmup, args.reps), 'HIP events around the wrapper')
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, 'w') as f:
        f.write('\n'.join(lines) + '\n')


if __name__ == '__main__':
    main()
