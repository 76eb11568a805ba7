"""Micro-benchmark of the 3-D evaluation kernels (csrc/pose3d.hip: posu_procrustes,
posu_pose3d_errors, posu_limb_break) at the reference's evaluation size: G = 2048 groups, V = 4
cameras, J = 16 joints.  HIP events around each enqueue on prepared device tensors, after warm-up,
median of the repeats.  Beside them the reference-style numpy loop (tests/pose3d_restatement.py:
one procrustes / one error_computing_3d / one break_limb_length per pose) on the same data on the
host, wall clock, once.

    python tools/pose3d_micro.py [--groups 2048] [--reps 25] [--out profiles/r10/pose3d_micro.txt]

Prints one JSON line per kernel and writes the same lines to --out.

    python tools/pose3d_micro.py --digest

No timing: the three entry points on small seeded inputs that reach every branch (J = 3, 16 and 65, every
reflection / scaling setting, a coplanar pose and one whose joints all coincide; limbs shared and per group,
a NaN pose) and one sha1 per output tensor over its raw bytes, so NaN payloads count.  Two builds
(tools/with_lib.py) compute the same bits when their listings are equal line for line.
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

import pose3d_restatement as rs  # noqa: E402
from posu import ops  # noqa: E402


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
    dev = torch.device('cuda', 0)

    def line(tag, *outs):
        torch.cuda.synchronize()
        print('%-58s %s' % (tag, ' '.join(sha(o) for o in outs)), flush=True)

    def up(a):
        return torch.from_numpy(np.ascontiguousarray(a)).to(dev)

    rng = np.random.RandomState(21)
    for J in (3, 16, 65):
        pairs = [rs.make_pair(rng, J, mirrored=bool(n & 1)) for n in range(7)]   # seven poses: two blocks
        A, B = np.stack([p[0] for p in pairs]), np.stack([p[1] for p in pairs])
        A[2], B[2] = A[2] * [1, 1, 0] + [0, 0, 700.0], B[2] * [1, 1, 0] + [0, 0, -300.0]   # coplanar: rank-2 M
        B[4] = B[4, 0]                                                              # all joints equal: 0 / 0
        for scaling, reflection in rs.SETTINGS:
            line('procrustes J=%d scaling=%d reflection=%s' % (J, scaling, reflection),
                 *ops.procrustes(up(A), up(B), scaling, reflection))
    for J in (16, 65):
        X, gt, R, T = rs.make_groups(rng, 3, 4, J)
        gt[1, 2] = gt[1, 2, 0]
        args = [up(a) for a in (X, gt, R, T)]
        for yes in (False, True):
            line('pose3d_errors J=%d procrustes=%d' % (J, yes), *ops.pose3d_errors(*args, procrustes=yes,
                                                                                  return_aligned=True))
    for per_group in (False, True):
        poses, limb, _ = rs.make_limb_cases(300 + per_group, 70, per_group)
        poses[5, 9] = np.nan
        line('limb_break per_group=%d' % per_group,
             *ops.limb_break(up(poses), up(rs.PARENT), up(limb), 0.4, return_worst=True))
    chain = np.arange(-1, 64, dtype=np.int32)                                        # 65 joints: the stride wraps
    poses = rng.randn(5, 65, 3) * 300
    line('limb_break J=65', *ops.limb_break(up(poses), up(chain), up(np.full(65, 420.0)), 0.4, return_worst=True))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--digest', action='store_true', help='no timing: one sha1 per output tensor at small shapes')
    ap.add_argument('--groups', type=int, default=2048)
    ap.add_argument('--views', type=int, default=4)
    ap.add_argument('--joints', type=int, default=16)
    ap.add_argument('--warmup', type=int, default=5)
    ap.add_argument('--reps', type=int, default=25)
    ap.add_argument('--out', default=os.path.join(REPO, 'profiles', 'r10', 'pose3d_micro.txt'))
    args = ap.parse_args()
    if args.digest:
        return digest()
    if args.reps < 20:
        ap.error('--reps must be at least 20')
    dev = torch.device('cuda', 0)
    G, V, J = args.groups, args.views, args.joints
    rng = np.random.RandomState(5)
    X, gt, R, T = rs.make_groups(rng, G, V, J)
    limb = np.linalg.norm(X[0][np.maximum(rs.PARENT, 0)] - X[0], axis=1) if J == 16 else np.ones(J)
    parent = rs.PARENT if J == 16 else np.arange(-1, J - 1, dtype=np.int32)
    pred = rs.pose3d_errors(X, gt, R, T, False)[1]                  # the predictions in the camera frames
    d = {k: torch.from_numpy(np.ascontiguousarray(v)).to(dev) for k, v in
         dict(X=X, gt=gt, R=R, T=T, A=gt.reshape(G * V, J, 3), B=pred.reshape(G * V, J, 3), limb=limb,
              parent=parent).items()}
    runs = {
        'posu_procrustes': (lambda: ops.procrustes(d['A'], d['B']), G * V),
        'posu_pose3d_errors (Procrustes)': (lambda: ops.pose3d_errors(d['X'], d['gt'], d['R'], d['T'], True), G * V),
        'posu_pose3d_errors (plain)': (lambda: ops.pose3d_errors(d['X'], d['gt'], d['R'], d['T'], False), G * V),
        'posu_limb_break': (lambda: ops.limb_break(d['X'], d['parent'], d['limb']), G),
    }
    cpu = {}
    t = time.perf_counter()
    for a, b in zip(gt.reshape(G * V, J, 3), pred.reshape(G * V, J, 3)):
        rs.procrustes(a, b)
    cpu['posu_procrustes'] = (time.perf_counter() - t) * 1e3
    for name, yes in (('posu_pose3d_errors (Procrustes)', True), ('posu_pose3d_errors (plain)', False)):
        t = time.perf_counter()
        ref = rs.pose3d_errors(X, gt, R, T, yes)[0]
        cpu[name] = (time.perf_counter() - t) * 1e3
        got = ops.pose3d_errors(d['X'], d['gt'], d['R'], d['T'], yes).cpu().numpy()
        assert float(np.abs(got - ref).max()) <= 1e-9, 'GPU and numpy errors differ'
    t = time.perf_counter()
    for g in range(G):
        rs.limb_break(X[g:g + 1], parent, limb)
    cpu['posu_limb_break'] = (time.perf_counter() - t) * 1e3
    lines = []
    for name, (fn, poses) in runs.items():
        med, lo, hi = event_ms(fn, args.warmup, args.reps)
        lines.append(json.dumps({'tool': 'pose3d_micro', 'kernel': name, 'groups': G, 'views': V, 'joints': J,
                                 'poses': poses, 'reps': args.reps, 'gpu_ms_median': round(med, 4),
                                 'gpu_ms_min': round(lo, 4), 'gpu_ms_max': round(hi, 4),
                                 'gpu_includes': 'f64 casts, output allocation and the launch (events around the wrapper)',
                                 'cpu_numpy_loop_ms': round(cpu[name], 1)}))
        print(lines[-1], flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, 'w') as f:
        f.write('\n'.join(lines) + '\n')


if __name__ == '__main__':
    main()
