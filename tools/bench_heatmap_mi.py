"""Time the heatmap mutual-information loss at the workload shape (4 views, N = 8 per view,
C = 256, sigma = 2 -> Q = 216, c_m = 64, JSD): a discriminator step (features and heatmaps
detached: forward, backward to the parameters) and the generator-side forward + backward
(gradients to the features and the heatmaps too), for

  * fused: HeatmapMILoss.views over HeatmapDiscriminator.pair_scores (csrc/heatmap_mi.hip), and
  * torch: the materialising plain-torch restatement in fp32 (tests/heatmap_mi_restatement.py),
    one call per view like the reference's loop,

on the same device, in the same process, alternating the two.  Prints one JSON line: milliseconds
per step (median and spread over the repeats, host clock around a device synchronise) and
torch.cuda.max_memory_allocated of each side's step.  Needs a GPU; there is no CPU path.

    python tools/bench_heatmap_mi.py [--views 4 --batch 8 --repeats 5 --iters 10 --features bf16] [--lib PATH]

--lib PATH loads another build of libposeu.so (two builds, alternated by the caller, are how a change
to the kernels is timed against its parent).

    python tools/bench_heatmap_mi.py --digest [--lib PATH]

No timing: ops.heatmap_pair_scores and both measures at small fixed shapes (DIGEST_SHAPES: one and
two segments, every c_m, every j-slab count of the pair passes, a block that walks two chunks,
Q = 1), seeded inputs and indices with a repeated position per image; f32 / bf16 / f16 features,
train and eval, inputs attached and detached, the discriminator frozen; one sha1 per output tensor.
Two builds compute the same bits when their listings are equal line for line.
"""
import argparse
import hashlib
import json
import os
import statistics
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (os.path.join(REPO, 'pose-unsupervised_amd', 'lib'), os.path.join(REPO, 'tests'), REPO):
    if p not in sys.path:
        sys.path.insert(0, p)


# (S, N, Q, C, c_m): what each reaches is in DESIGN.md section 4 (JS = max(1, min(4, Q / 8)) j slabs,
# k_b3 the largest JS3 <= JS with JS3 c_m <= 2 Q; 64 rows per chunk, at most 32 blocks per slab)
DIGEST_SHAPES = [(1, 3, 18, 32, 32), (2, 3, 18, 32, 32), (1, 2, 216, 256, 64), (1, 2, 18, 16, 128),
                 (1, 1, 128, 8, 128), (1, 1, 192, 8, 128), (1, 129, 16, 8, 32), (1, 5, 7, 8, 64),
                 (1, 37, 1, 32, 32)]


def digest_indices(seed, rows, q):
    """Seeded positions [rows, q] of a 64 x 64 map; position 0 of every image repeats at the end."""
    import numpy as np
    idx = np.random.default_rng(seed).integers(0, 64 * 64, (rows, q)).astype(np.int32)
    if q > 1:
        idx[:, -1] = idx[:, 0]
    return idx


def digest():
    import torch
    from models.discriminator import HeatmapDiscriminator
    from posu import ops
    from posu import synthetic as syn

    dev = torch.device('cuda', 0)

    def sha(t):
        return hashlib.sha1(t.detach().contiguous().view(torch.uint8).cpu().numpy().tobytes()).hexdigest()[:12]

    for s, n, q, c, cm in DIGEST_SHAPES:
        joint = 1
        case = syn.heatmap_mi_case(500 + q + cm, s * n, c, cm, joint_idx=joint)
        idx = torch.as_tensor(digest_indices(600 + q + cm, s * n, q))
        disc = HeatmapDiscriminator(syn.heatmap_mi_cfg(channels=c, inter_channels=cm, joint_idx=joint))
        disc.load_state_dict({k: torch.as_tensor(v) for k, v in case['state'].items()})
        disc = disc.to(dev)
        low32 = torch.as_tensor(case['low_features']).to(dev).float()
        heat0 = torch.as_tensor(case['heatmaps']).to(dev).float()
        runs = [(dt, training, attach, False) for dt in (torch.float32, torch.bfloat16, torch.float16)
                for training in (True, False) for attach in (True, False)]
        runs.append((torch.float32, True, True, True))     # dparams null: k_b2 without the d W2 sums
        for dt, training, attach, frozen in runs:
            low = low32.to(dt).permute(0, 2, 3, 1).contiguous().permute(0, 3, 1, 2).requires_grad_(attach)
            heat = heat0.clone().requires_grad_(attach)
            params = {k: (v.detach().clone() if frozen else v.detach().clone().requires_grad_(
                v.is_floating_point() and k not in ('rm1', 'rv1', 'rm2', 'rv2'))) for k, v in disc._params().items()}
            u, stats = ops.heatmap_pair_scores(low, heat, idx, joint, params, nseg=s, training=training)
            nce = ops.pair_mi_loss(u, 'NCE', s)
            jsd = ops.pair_mi_loss(u, 'JSD', s) if q > 1 else None    # JSD has no off-diagonal pair at Q = 1
            (nce.sum() if jsd is None else nce.sum() + jsd.sum()).backward()
            torch.cuda.synchronize()
            outs = [('u', u), ('jsd', jsd), ('nce', nce), ('stats', stats if training else None),
                    ('dlow', low.grad), ('dheat', heat.grad)]
            outs += [('d' + k, p.grad) for k, p in params.items()]
            tag = 'S%d N%d Q%d C%d cm%d %s %s %s%s' % (s, n, q, c, cm, str(dt).split('.')[1],
                                                      'train' if training else 'eval',
                                                      'attached' if attach else 'detached', ' frozen' if frozen else '')
            print('%-52s %s' % (tag, ' '.join('%s=%s' % (k, sha(t)) for k, t in outs if t is not None)))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--lib', default=None, help='another build of libposeu.so')
    ap.add_argument('--digest', action='store_true', help='no timing: one sha1 per output tensor at small shapes')
    ap.add_argument('--views', type=int, default=4)
    ap.add_argument('--batch', type=int, default=8)
    ap.add_argument('--channels', type=int, default=256)
    ap.add_argument('--inter', type=int, default=64)
    ap.add_argument('--sigma', type=int, default=2)
    ap.add_argument('--features', choices=['f32', 'bf16'], default='f32',
                    help='feature storage of the fused path (the restatement always computes in fp32)')
    ap.add_argument('--repeats', type=int, default=5)
    ap.add_argument('--iters', type=int, default=10)
    ap.add_argument('--warmup', type=int, default=3)
    args = ap.parse_args()
    if args.lib:
        from posu import _native
        _native._LIB_PATH = os.path.abspath(args.lib)
    if args.digest:
        return digest()

    import torch
    import heatmap_mi_restatement as R
    from core.loss import HeatmapMILoss
    from models.discriminator import HeatmapDiscriminator
    from posu import synthetic as syn

    if not torch.cuda.is_available():
        raise SystemExit('bench_heatmap_mi needs a GPU')
    dev = torch.device('cuda', 0)
    joint = 3
    cfg = syn.heatmap_mi_cfg(sigma=args.sigma, channels=args.channels, inter_channels=args.inter, joint_idx=joint)
    cases = [syn.heatmap_mi_case(100 + v, args.batch, args.channels, args.inter, joint_idx=joint)
             for v in range(args.views)]
    disc = HeatmapDiscriminator(cfg)
    disc.load_state_dict({k: torch.as_tensor(v) for k, v in cases[0]['state'].items()})
    disc = disc.to(dev).train()
    crit = HeatmapMILoss(cfg, {'heatmap_discriminator': disc})
    metas = [{'joints_2d_transformed': torch.as_tensor(c['joints_2d_transformed']),
              'joints_vis': torch.as_tensor(c['joints_vis'])} for c in cases]
    gen = torch.Generator().manual_seed(1)
    indices = [crit.sample_indices(m, joint, generator=gen) for m in metas]
    fdt = torch.bfloat16 if args.features == 'bf16' else torch.float32
    # one stacked channels-last tensor per side, the views its slices (what a stacked backbone call hands over)
    stacked = torch.cat([torch.as_tensor(c['low_features']) for c in cases]).to(dev).float()
    low_fused = stacked.to(fdt).permute(0, 2, 3, 1).contiguous().permute(0, 3, 1, 2)
    low_torch = stacked.clone()
    heat = torch.cat([torch.as_tensor(c['heatmaps']) for c in cases]).to(dev).float()
    del stacked
    n = args.batch
    state = {k: v.detach().clone().requires_grad_(v.is_floating_point() and 'running' not in k)
             for k, v in disc.state_dict().items() if 'num_batches' not in k}
    buffers = {k: state[k].detach().clone() for k in R.BUFFER_KEYS}
    idx_dev = [i.to(dev) for i in indices]

    def fused(generator_side):
        lo = low_fused.detach().requires_grad_(generator_side)
        hm = heat.detach().requires_grad_(generator_side)
        for p in disc.parameters():
            p.grad = None
        loss = crit.views([lo[v * n:(v + 1) * n] for v in range(args.views)],
                          [hm[v * n:(v + 1) * n] for v in range(args.views)], [None] * args.views, metas, joint,
                          indices=indices)
        loss.backward()
        return loss

    def restated(generator_side):
        lo = low_torch.detach().requires_grad_(generator_side)
        hm = heat.detach().requires_grad_(generator_side)
        for k in R.PARAM_KEYS:
            state[k].grad = None
        loss = 0
        for v in range(args.views):
            loss = loss + R.loss(lo[v * n:(v + 1) * n], hm[v * n:(v + 1) * n], idx_dev[v], joint, state, 'JSD', True,
                                 buffers)
        loss.backward()
        return loss

    def timed(fn, side):
        for _ in range(args.warmup):
            fn(side)
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats()
        base = torch.cuda.memory_allocated()
        t0 = time.perf_counter()
        for _ in range(args.iters):
            loss = fn(side)
        torch.cuda.synchronize()
        ms = (time.perf_counter() - t0) * 1e3 / args.iters
        return ms, torch.cuda.max_memory_allocated() - base, float(loss)

    result = {'shape': dict(views=args.views, batch=n, channels=args.channels, inter=args.inter, sigma=args.sigma,
                            q=int(indices[0].shape[1]), features=args.features, measure='JSD'),
              'iters': args.iters, 'repeats': args.repeats}
    for side, label in ((False, 'discriminator_step'), (True, 'generator_fwd_bwd')):
        rows = {'fused': [], 'torch': []}
        for _ in range(args.repeats):          # alternate the two sides
            rows['fused'].append(timed(fused, side))
            rows['torch'].append(timed(restated, side))
        entry = {}
        for name, r in rows.items():
            ms = [x[0] for x in r]
            entry[name] = {'ms_median': round(statistics.median(ms), 4), 'ms_min': round(min(ms), 4),
                           'ms_max': round(max(ms), 4), 'peak_extra_bytes': max(x[1] for x in r),
                           'loss': r[-1][2]}
        entry['speedup'] = round(entry['torch']['ms_median'] / entry['fused']['ms_median'], 2)
        result[label] = entry
    print(json.dumps(result))


if __name__ == '__main__':
    main()
