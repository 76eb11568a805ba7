"""Micro-benchmark of fp16 training (posu.amp.LossScaler + posu.optim.Adam(capturable=True)) beside
the bf16 step: bench.py's configs[3] training step (R50@256, 32 groups x 4 views, JointsMSE +
FundamentalLoss, backward, Adam; bench.train_batch) with tuned tiles, HIP events around one whole
step, median of the repeats after warm-up --

  bf16   loss.backward(); opt.step()                      posu.optim.Adam (host step count)
  fp16   scaler.scale(loss).backward(); scaler.step(opt); scaler.update()

and the optimizer alone on the same network's gradients: posu_adam_step (one pass) against the
posu_grad_stats + posu_adam_step_dev pair the scaler runs (two passes over the gradients).

    python tools/train_fp16_micro.py [--groups 32] [--reps 7] [--warmup 3]

Prints one JSON line.
"""
import argparse
import json
import os
import statistics
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(REPO, 'pose-unsupervised_amd', 'lib'), REPO]

import torch  # noqa: E402

import bench  # noqa: E402
from posu import amp, optim, plan as pplan  # noqa: E402


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


def captured(fn):
    """fn's launches as a graph (one stream: a linear graph)."""
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        fn()
    return graph


def bench_args(precision, groups):
    argv, sys.argv = sys.argv, ['bench.py', '--mode', 'train', '--precision', precision, '--groups', str(groups)]
    try:
        return bench.parse()
    finally:
        sys.argv = argv


def training_step(precision, groups, dev):
    """-> (step function, network, optimizer, scaler or None) of bench.py's training batch."""
    tb = bench.train_batch(bench_args(precision, groups), dev)
    net = tb['net']
    scaler = None
    if precision == 'fp16':
        scaler = net.loss_scaler = amp.LossScaler()
    opt = optim.Adam(net.parameters(), lr=1e-3, capturable=scaler is not None)

    def step():
        loss = tb['loss']()
        opt.zero_grad(set_to_none=True)
        if scaler is None:
            loss.backward()
            opt.step()
        else:
            scaler.scale(loss).backward()
            scaler.step(opt)
            scaler.update()

    pplan._Tuner.active, pplan._Tuner.reps = True, 3   # the first step times the tiles, as bench.py's does
    try:
        step()
    finally:
        pplan._Tuner.active = False
    return step, net, opt, scaler


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--groups', type=int, default=32)
    ap.add_argument('--reps', type=int, default=7)
    ap.add_argument('--warmup', type=int, default=3)
    args = ap.parse_args()
    dev = torch.device('cuda', 0)
    out = {'tool': 'train_fp16_micro', 'layers': 50, 'size': 256, 'groups': args.groups, 'views': 4,
           'reps': args.reps}
    for precision in ('bf16', 'fp16'):
        step, net, opt, scaler = training_step(precision, args.groups, dev)
        if scaler is not None:   # let the scale settle below the overflow before timing
            for _ in range(20):
                step()
            out['fp16_loss_scale'] = scaler.get_scale()
        out['%s_step_ms' % precision] = round(event_ms(step, args.warmup, args.reps), 3)
        if scaler is not None:
            # the optimizer alone, on this network's last gradients (left in .grad, still scaled)
            params = [p for p in net.parameters() if p.grad is not None]
            host = optim.Adam(params, lr=1e-3)

            def pair():
                scaler.step(opt)
                scaler.update()
            # as called (the host builds the launch tables: these are enqueue-bound) and as replays of
            # a captured graph (the device time of the launches alone)
            out['adam_step_ms'] = round(event_ms(host.step, args.warmup, args.reps), 4)
            out['stats_plus_adam_dev_ms'] = round(event_ms(pair, args.warmup, args.reps), 4)
            out['adam_step_replay_ms'] = round(event_ms(captured(host.step).replay, args.warmup, args.reps), 4)
            out['stats_plus_adam_dev_replay_ms'] = round(event_ms(captured(pair).replay, args.warmup, args.reps), 4)
            out['found_inf_in_timed_pair'] = scaler.found_inf()
            out['parameters'] = sum(p.numel() for p in params)
        del step, net, opt, scaler
        torch.cuda.empty_cache()
    print(json.dumps(out))


if __name__ == '__main__':
    main()
