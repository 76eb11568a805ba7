"""Time core.function.train against the loop a user of this build has today, at the bench's
training workload (R50 at 256 x 256, 4 views x 32, bf16, JointsMSE + FundamentalLoss, posu.optim.Adam):

  * train:    core.function.train -- PCK accuracy, the running meters and the H36M selection stay on
              the device, nothing is read back between two log lines;
  * baseline: the reference's step (lib/core/function.py:148-469) written here from the same public
              functions the way the reference writes it: loss.item() / mse_loss.item() / fund_loss.item()
              every step and accuracy(o.detach().cpu().numpy(), t.detach().cpu().numpy()) per view.

Both run in one process on one model and optimiser, alternating `--repeats` times; each leg is
`--steps` steps between two device synchronisations on the host clock, after one autotuning step and
`--warmup` steps of each loop.  The batches are placed on the device beforehand (both loops' .to(device)
is then free), so the difference between the legs is what the loops themselves do.  Prints one JSON
line: ms per step of every leg, the medians, and each side's spread (max - min over its legs).

    python tools/bench_train_loop.py [--groups 32 --steps 60 --warmup 5 --repeats 3 --precision bf16]
"""
import argparse
import json
import logging
import os
import statistics
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (os.path.join(REPO, 'pose-unsupervised_amd', 'lib'), REPO):
    if p not in sys.path:
        sys.path.insert(0, p)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--layers', type=int, default=50)
    ap.add_argument('--size', type=int, default=256)
    ap.add_argument('--groups', type=int, default=32, help='samples per view')
    ap.add_argument('--precision', default='bf16', choices=['bf16', 'fp32'])
    ap.add_argument('--steps', type=int, default=60, help='steps per timed leg (60 x ~21 ms: over a second)')
    ap.add_argument('--warmup', type=int, default=5)
    ap.add_argument('--repeats', type=int, default=3)
    ap.add_argument('--watch', action='store_true', help='LOSS.WATCH_GRAD_NORM in both loops')
    args = ap.parse_args()

    import numpy as np
    import torch
    from core.evaluate import accuracy
    from core.function import AverageMeter, train
    from core.loss import FundamentalLoss, JointsMSELoss
    from models.multiview_pose_resnet import get_multiview_pose_net
    from models.pose_resnet import get_pose_net
    from posu import optim, plan as pplan, synthetic as syn
    from utils.gradients import check_grad_norm
    from utils.transforms import generate_integral_preds_2d_th, transform_back_th

    if not torch.cuda.is_available():
        raise SystemExit('bench_train_loop needs a GPU')
    logging.disable(logging.CRITICAL)    # train()'s log line at step 0 of every leg
    dev = torch.device('cuda', 0)
    cfg = syn.train_loop_cfg(num_layers=args.layers, image_size=args.size, fundamental=True,
                             watch_grad_norm=args.watch, print_freq=10 ** 9)
    net = get_pose_net(cfg, is_train=False, precision=args.precision)
    net.load_state_dict(syn.synthetic_state_dict(net.state_dict(), seed=syn.calibrated_seed(args.layers, args.size),
                                                 bn_stats=syn.load_bn_stats(args.layers, args.size)))
    model = get_multiview_pose_net(net.to(dev), cfg).train()
    opt = optim.Adam(net.parameters(), lr=1e-3)
    crit = JointsMSELoss(use_target_weight=True)
    fl = FundamentalLoss(cfg, fundamental_matrix_dict=syn.fundamental_dict(), device=dev)
    L = cfg.LOSS

    distinct = []
    for inp, tgt, wgt, meta in syn.train_loop_batches(2, nviews=4, batch=args.groups, image_size=args.size, seed=1,
                                                      target_sigma=2.0):
        distinct.append(([v.to(dev) for v in inp], [t.to(dev) for t in tgt], [w.to(dev) for w in wgt], meta))

    def batches(n):
        return [distinct[k % len(distinct)] for k in range(n)]

    def baseline(data):
        losses, mse_losses, fund_losses, avg_acc = AverageMeter(), AverageMeter(), AverageMeter(), AverageMeter()
        for input, target, weight, meta in data:
            input = [v.to(dev, non_blocking=False) for v in input]
            raw, _, _, _ = model(input)
            output = raw
            loss, mse_loss = 0, 0
            target_cuda, weight_cuda = [], []
            for t, w, r in zip(target, weight, raw):
                t, w = t.to(dev, non_blocking=False), w.to(dev, non_blocking=False)
                target_cuda.append(t)
                weight_cuda.append(w)
                mse_loss = mse_loss + crit(r, t, w) * L.MSE_LOSS_WEIGHT
            loss = loss + mse_loss
            joints = transform_back_th(cfg, [generate_integral_preds_2d_th(o) for o in output], meta)
            fund_loss = fl(joints, weight_cuda, meta) * L.FUNDAMENTAL_LOSS_WEIGHT
            loss = loss + fund_loss
            if args.watch:
                grad_dict = check_grad_norm({'mse': mse_loss, 'fund': fund_loss}, raw, norm=1)
            opt.zero_grad()
            loss.backward()
            opt.step()
            n = len(input) * input[0].size(0)
            losses.update(loss.item(), n)
            mse_losses.update(mse_loss.item(), n)
            fund_losses.update(fund_loss.item(), 1)
            if args.watch:
                [v.item() for v in grad_dict.values()]
            acc, cnt = [], []
            for o, t in zip(output, target_cuda):
                _, a, c, _ = accuracy(o.detach().cpu().numpy(), t.detach().cpu().numpy())
                acc.append(a)
                cnt.append(c)
            avg_acc.update(np.mean(acc), np.mean(cnt))
        return losses.avg

    def ours(data):
        return train(cfg, data, {'base_model': model}, {'mse_weights': crit, 'fundamental': fl}, {'base_model': opt},
                     1, '', None, 0)['loss']['avg']

    def timed(fn, n):
        data = batches(n)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        loss = fn(data)
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) / n * 1e3, loss

    # the first step times every admissible conv tile: the switch bench.py --mode train sets (posu/train_plan.py)
    pplan._Tuner.active, pplan._Tuner.reps = True, 3
    try:
        ours(batches(1))
    finally:
        pplan._Tuner.active = False
    for fn in (ours, baseline):
        fn(batches(max(1, args.warmup)))
    legs = {'train': [], 'baseline': []}
    loss = {}
    for _ in range(args.repeats):
        for name, fn in (('baseline', baseline), ('train', ours)):
            ms, loss[name] = timed(fn, args.steps)
            legs[name].append(round(ms, 4))
    out = {'metric': 'train_loop_ms_per_step', 'unit': 'ms', 'higher_is_better': False,
           'workload': 'R%d at %d, %d x 4, %s, JointsMSE + FundamentalLoss%s, posu.optim.Adam'
                       % (args.layers, args.size, args.groups, args.precision, ' + grad-norm watch' if args.watch else ''),
           'steps': args.steps, 'warmup': args.warmup, 'repeats': args.repeats}
    for name, ms in legs.items():
        out[name] = {'ms_per_step': ms, 'median': round(statistics.median(ms), 4),
                     'spread': round(max(ms) - min(ms), 4), 'last_avg_loss': float(loss[name])}
    out['train_over_baseline'] = round(out['train']['median'] / out['baseline']['median'], 4)
    print(json.dumps(out))


if __name__ == '__main__':
    main()
