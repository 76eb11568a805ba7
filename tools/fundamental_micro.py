"""Time the H36M-sized fundamental-matrix call (7 subjects x 6 view pairs = 42 problems, 8192 correspondences
each, 512 hypotheses) on the device against the numpy restatement (tests/fundamental_restatement.py) on the
host, and print a digest of the outputs.

    python tools/fundamental_micro.py [--problems 42] [--rows 8192] [--hypotheses 512] [--reps 20]
                                      [--host-problems 2] [--out profiles/r13/fundamental_micro.txt]

The device call is event-timed as a whole (three launches) after warm-up, median of the repeats.  The
restatement is timed once on --host-problems problems and scaled to all of them: it is a test aid, not a fast
host implementation, so the ratio says only that the estimate no longer needs the host.  Before anything is
timed the two are compared on those problems: the same sample, winner and mask.  Not a gate: the workload is
light; what matters is the capability and that the data stay on the device.
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

import fundamental_restatement as rs  # noqa: E402
from multiviews.cameras import project_pose  # noqa: E402
from posu import ops  # noqa: E402
from posu import synthetic as syn  # noqa: E402


def make_inputs(problems, rows, seed=3):
    """Noisy projections (1 px) of random poses in the synthetic rigs' view pairs, 15 % of the rows gross outliers."""
    r = np.random.default_rng(seed)
    pairs = [(i, j) for i in range(4) for j in range(i + 1, 4)]
    X = syn.synthetic_poses3d((rows + 15) // 16, 16, seed).reshape(-1, 3)[:rows]
    pts = np.zeros((problems, rows, 4))
    for p in range(problems):
        cams = syn.h36m_like_cameras(p // len(pairs) + 1, distortion=False)
        i, j = pairs[p % len(pairs)]
        pts[p, :, :2], pts[p, :, 2:] = project_pose(X, cams[i]), project_pose(X, cams[j])
    pts += r.normal(0, 1.0, size=pts.shape)
    bad = r.uniform(size=pts.shape[:2]) < 0.15
    pts[bad, 2:] += r.choice([-1, 1], size=(bad.sum(), 2)) * r.uniform(30, 200, size=(bad.sum(), 2))
    return pts


def sha(t):
    return hashlib.sha1(t.contiguous().view(torch.uint8).cpu().numpy().tobytes()).hexdigest()[:12]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--problems', type=int, default=42)
    ap.add_argument('--rows', type=int, default=8192)
    ap.add_argument('--hypotheses', type=int, default=512)
    ap.add_argument('--seed', type=int, default=1)
    ap.add_argument('--warmup', type=int, default=3)
    ap.add_argument('--reps', type=int, default=20)
    ap.add_argument('--host-problems', type=int, default=2)
    ap.add_argument('--out', default=os.path.join(REPO, 'profiles', 'r13', 'fundamental_micro.txt'))
    args = ap.parse_args()
    dev = torch.device('cuda', 0)
    P, N, H = args.problems, args.rows, args.hypotheses
    pts = make_inputs(P, N)
    pts_d = torch.from_numpy(pts).to(dev)

    F, mask, sample, stats = ops.fundamental_lmeds(pts_d, None, H, args.seed)
    torch.cuda.synchronize()
    k = min(args.host_problems, P)
    t = time.perf_counter()
    host = rs.lmeds(pts[:k], None, H, args.seed)
    host_s = (time.perf_counter() - t) * P / k
    assert np.array_equal(sample[:k].cpu().numpy(), host['sample'])
    assert np.array_equal(stats[:k, 3].cpu().numpy().astype(np.int64), host['best'])
    assert np.array_equal(mask[:k].cpu().numpy(), host['mask'])
    fdiff = float(np.abs(F[:k].cpu().numpy() - host['F']).max())

    for _ in range(args.warmup):
        ops.fundamental_lmeds(pts_d, None, H, args.seed)
    torch.cuda.synchronize()
    ms = []
    for _ in range(args.reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        ops.fundamental_lmeds(pts_d, None, H, args.seed)
        b.record()
        b.synchronize()
        ms.append(a.elapsed_time(b))
    resid = ops.epipolar_residual_stats(F, pts_d, mask)
    lines = [json.dumps({'tool': 'fundamental_micro', 'problems': P, 'rows': N, 'hypotheses': H, 'reps': args.reps,
                         'device_ms_median': round(statistics.median(ms), 3), 'device_ms_min': round(min(ms), 3),
                         'device_ms_max': round(max(ms), 3), 'host_restatement_s_scaled': round(host_s, 2),
                         'host_problems_timed': k, 'max_abs_F_diff_vs_restatement': fdiff,
                         'inliers_min': int(stats[:, 2].min().item()), 'inliers_max': int(stats[:, 2].max().item()),
                         'inlier_residual_mean_max': round(float(resid[:, 0].max().item()), 6),
                         'timed': 'HIP events around the wrapper (workspace and outputs allocated inside)'}),
             json.dumps({'tool': 'fundamental_micro', 'digest': {'F': sha(F), 'mask': sha(mask), 'sample': sha(sample),
                                                                 'stats': sha(stats)}})]
    for line in lines:
        print(line, flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, 'w') as f:
        f.write('\n'.join(lines) + '\n')


if __name__ == '__main__':
    main()
