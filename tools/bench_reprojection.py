"""Time the reprojection-consistency loss at the workload shape (32 groups, 4 views, 16 joints, H36M-like
distorted rigs, f32 view-major predictions, confidences and target weights): forward + backward to the
predictions and the confidences, for

  * fused: ops.reprojection_loss (csrc/triangulate_grad.hip: two launches forward, one backward), and
  * torch: the plain-torch fp64 restatement (tests/triangulation_grad_restatement.py, the SVD route, autograd),

on the same device, in the same process, alternating the two.  Prints one JSON line: milliseconds per step
(median and spread over the repeats, host clock around a device synchronise), each side's loss and the largest
difference of the two sides' gradients relative to the largest entry.  Needs a GPU; there is no CPU path.

    python tools/bench_reprojection.py [--groups 32 --views 4 --joints 16 --repeats 5 --iters 20] [--lib PATH]

--lib PATH loads another build of libposeu.so.
"""
import argparse
import json
import os
import statistics
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (os.path.join(REPO, 'pose-unsupervised_amd', 'lib'), os.path.join(REPO, 'tests'), REPO):
    if p not in sys.path:
        sys.path.insert(0, p)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--lib', default=None, help='another build of libposeu.so')
    ap.add_argument('--groups', type=int, default=32)
    ap.add_argument('--views', type=int, default=4)
    ap.add_argument('--joints', type=int, default=16)
    ap.add_argument('--detach-point', action='store_true')
    ap.add_argument('--repeats', type=int, default=5)
    ap.add_argument('--iters', type=int, default=20)
    ap.add_argument('--warmup', type=int, default=3)
    args = ap.parse_args()
    if args.lib:
        from posu import _native
        _native._LIB_PATH = os.path.abspath(args.lib)

    import torch
    import triangulation_grad_restatement as R
    from posu import ops

    if not torch.cuda.is_available():
        raise SystemExit('bench_reprojection needs a GPU')
    dev = torch.device('cuda', 0)
    c = R.case(args.groups, args.views, args.joints, True, seed=21)
    M, intr = c['M'].to(dev), c['intr'].to(dev)
    xy_vm = c['xy'].permute(1, 0, 2, 3).contiguous().float().to(dev)        # [V, G, J, 2] f32: the pipeline's layout
    xy_gm = xy_vm.double().permute(1, 0, 2, 3).contiguous()                  # the same numbers for the restatement
    conf, omega = c['w'].to(dev), c['omega'].to(dev)

    def fused():
        x = xy_vm.detach().requires_grad_(True)
        w = conf.detach().requires_grad_(True)
        loss = ops.reprojection_loss(M, intr, x, None, w, omega, view_major=True, detach_point=args.detach_point)
        loss.backward()
        return loss, x.grad.permute(1, 0, 2, 3).double(), w.grad

    def restated():
        x = xy_gm.detach().requires_grad_(True)
        w = conf.detach().requires_grad_(True)
        loss = R.loss(M, intr, x, None, w, omega, True, args.detach_point, 'svd')[0]
        loss.backward()
        return loss, x.grad, w.grad if w.grad is not None else torch.zeros_like(w)

    def timed(fn):
        for _ in range(args.warmup):
            fn()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(args.iters):
            out = fn()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3 / args.iters, out

    rows = {'fused': [], 'torch': []}
    for _ in range(args.repeats):              # alternate the two sides
        rows['fused'].append(timed(fused))
        rows['torch'].append(timed(restated))
    result = {'shape': dict(groups=args.groups, views=args.views, joints=args.joints, xy='f32 view-major',
                            detach_point=bool(args.detach_point)), 'iters': args.iters, 'repeats': args.repeats}
    for name, r in rows.items():
        ms = [x[0] for x in r]
        result[name] = {'ms_median': round(statistics.median(ms), 4), 'ms_min': round(min(ms), 4),
                        'ms_max': round(max(ms), 4), 'loss': float(r[-1][1][0].detach())}
    result['speedup'] = round(result['torch']['ms_median'] / result['fused']['ms_median'], 2)
    (_, gx_f, gw_f), (_, gx_t, gw_t) = rows['fused'][-1][1], rows['torch'][-1][1]
    result['gxy_rel_diff'] = float((gx_f - gx_t).abs().max() / gx_t.abs().max())
    if float(gw_t.abs().max()) > 0:
        result['gw_rel_diff'] = float((gw_f - gw_t).abs().max() / gw_t.abs().max())
    print(json.dumps(result))


if __name__ == '__main__':
    main()
