"""Generate tests/golden/heatmap_mi.npz by running the REFERENCE's own HeatmapMILoss over its
HeatmapDiscriminator (lib/core/loss.py:636-781, lib/models/discriminator.py:225-242) on the CPU in
float64.  Run once, where the reference is checked out (not on the GPU box):

    python tests/golden/make_heatmap_mi_golden.py

The reference is imported in-process the way make_golden.py does it (core.loss imports OpenCV,
which is not installed: the same stand-in module).  Inputs come from posu.synthetic.heatmap_mi_case
(a seeded numpy Generator: features, heatmaps, joints, the discriminator's parameters and
non-trivial BatchNorm weights / running statistics), so the file stores only the seeds, the
positions the reference drew, and the reference's results:

  A  N = 3, sigma = 0 (Q = 18), C = 32, c_m = 32, JSD and NCE, train mode; joint at (0, 0), joint at
     the far corner, one invisible joint (clamped windows: repeated positions);
  B  N = 2, sigma = 2 (Q = 216), C = 256, c_m = 64, JSD, train mode (the workload's widths);
  C  case A in eval() with the given running statistics.

Per case and measure: indices, loss, every parameter gradient, the BatchNorm buffers after the call,
and the feature / heatmap gradients at the sampled positions (float64; float32 casts for case B).
"""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import make_golden as mg  # noqa: E402  (the cv2 stand-in and the by-path loader of posu.synthetic)

syn = mg.syn

CASES = {
    # name: (seed, n, channels, c_m, sigma, joint_idx, corners, training, measures, torch seed)
    'A': (11, 3, 32, 32, 0, 5, True, True, ('JSD', 'NCE'), 101),
    'B': (12, 2, 256, 64, 2, 3, False, True, ('JSD',), 102),
    'C': (11, 3, 32, 32, 0, 5, True, False, ('JSD', 'NCE'), 103),
}


def _import_reference():
    mg._install_cv2_standin()
    for p in (mg.REF_LIB, os.path.join(mg.REF_LIB, 'core')):
        if p not in sys.path:
            sys.path.insert(0, p)
    import core.loss as ref_loss
    import models.discriminator as ref_disc
    return ref_loss, ref_disc


def run_case(ref_loss, ref_disc, name, measure):
    seed, n, c, cm, sigma, joint, corners, training, _, tseed = CASES[name]
    cfg = syn.heatmap_mi_cfg(sigma=sigma, channels=c, inter_channels=cm, measure=measure, joint_idx=joint)
    case = syn.heatmap_mi_case(seed, n, c, cm, joint_idx=joint, corners=corners)
    disc = ref_disc.HeatmapDiscriminator(cfg).double()
    disc.load_state_dict({k: torch.as_tensor(v) for k, v in case['state'].items()})
    disc.train(training)
    crit = ref_loss.HeatmapMILoss(cfg, {'heatmap_discriminator': disc})
    drawn = []
    sample = crit._sample_some_indices

    def recording(loc, max_len=64):
        idx = sample(loc, max_len=max_len)
        drawn.append(idx.clone())
        return idx
    crit._sample_some_indices = recording
    low = torch.as_tensor(case['low_features']).requires_grad_(True)
    heat = torch.as_tensor(case['heatmaps']).requires_grad_(True)
    meta = {'joints_2d_transformed': torch.as_tensor(case['joints_2d_transformed']),
            'joints_vis': torch.as_tensor(case['joints_vis'])}
    torch.manual_seed(tseed)
    loss = crit(low, heat, None, meta, joint)
    loss.backward()
    idx = drawn[0]
    q = idx.shape[1]
    big = name == 'B'
    cast = (lambda a: a.astype(np.float32)) if big else (lambda a: a)
    dlow = low.grad.permute(0, 2, 3, 1).reshape(n, -1, c)
    dheat = heat.grad[:, joint].reshape(n, -1)
    # the gradients are zero off the sampled positions (and off the joint's map)
    mask = torch.zeros(n, 64 * 64, dtype=torch.bool)
    mask.scatter_(1, idx, True)
    assert float(dlow[~mask].abs().max()) == 0.0 and float(dheat[~mask].abs().max()) == 0.0
    others = [j for j in range(heat.shape[1]) if j != joint]
    assert float(heat.grad[:, others].abs().max()) == 0.0
    out = {'indices': idx.numpy().astype(np.int32), 'loss': np.float64(loss.item()),
           'dlow_at': cast(dlow.gather(1, idx[:, :, None].expand(n, q, c)).numpy()),
           'dheat_at': cast(dheat.gather(1, idx).numpy())}
    for k, p in disc.named_parameters():
        out['grad.' + k] = p.grad.numpy()
    for k, b in disc.named_buffers():
        out['buffer.' + k] = b.numpy()
    return out


def main():
    ref_loss, ref_disc = _import_reference()
    blob = {}
    for name, spec in CASES.items():
        blob['%s.spec' % name] = np.array(spec[:6] + (int(spec[6]), int(spec[7])), dtype=np.int64)
        for measure in spec[8]:
            res = run_case(ref_loss, ref_disc, name, measure)
            dup = sum(len(r) - len(set(r.tolist())) for r in res['indices'])
            print('%s %s: loss %.12g, Q = %d, repeated positions %d' % (name, measure, res['loss'],
                                                                      res['indices'].shape[1], dup))
            for k, v in res.items():
                blob['%s.%s.%s' % (name, measure, k)] = v
    path = os.path.join(HERE, 'heatmap_mi.npz')
    np.savez(path, **blob)
    print('wrote', path, os.path.getsize(path), 'bytes')


if __name__ == '__main__':
    main()
