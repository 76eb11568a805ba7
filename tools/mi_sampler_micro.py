"""The positions of one heatmap-MI step, 4 views x 32 images, sigma 2 (Q = 216): the device sampler
(HeatmapMILoss(sampler='device').sample_indices_device, one launch for the four views; device events
over 2000 back-to-back calls, and the entry point alone on concatenated inputs) against the host
sample_indices per view + concatenation + upload (wall clock to a synchronise), with the metadata on the
host and on the device as BatchMaker leaves it.  The legs alternate; medians of nine windows.

    python tools/mi_sampler_micro.py"""
import os
import statistics
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(REPO, 'pose-unsupervised_amd', 'lib'), REPO]
import numpy as np
import torch
from core.loss import HeatmapMILoss
from posu import ops, synthetic as syn

cuda = torch.device('cuda', 0)
V, N, J, joint = 4, 32, 16, 0
cfg = syn.heatmap_mi_cfg(sigma=2, channels=256, inter_channels=64)
rng = np.random.default_rng(0)
host_meta = [{'joints_2d_transformed': torch.as_tensor(rng.uniform(0.0, 256.0, (N, J, 2))),
              'joints_vis': torch.as_tensor((rng.uniform(size=(N, J, 3)) > 0.1).astype(np.float64))} for _ in range(V)]
dev_meta = [{k: t.to(cuda) for k, t in m.items()} for m in host_meta]
host = HeatmapMILoss(cfg, {'heatmap_discriminator': None})
dev = HeatmapMILoss(cfg, {'heatmap_discriminator': None}, sampler='device', seed=1)


def host_path(meta):
    idx = torch.cat([host.sample_indices(m, joint) for m in meta], dim=0)
    return torch.from_numpy(np.ascontiguousarray(idx.numpy().astype(np.int32))).to(cuda)


def wall(fn, reps):
    torch.cuda.synchronize()
    t = time.perf_counter()
    for _ in range(reps):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t) / reps * 1e6


def events(fn, reps):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    a.record()
    for _ in range(reps):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / reps * 1e3


for _ in range(20):
    host_path(host_meta), host_path(dev_meta), dev.sample_indices_device(dev_meta, joint)
cat_j = torch.cat([m['joints_2d_transformed'] for m in dev_meta]).contiguous()
cat_v = torch.cat([m['joints_vis'][:, :, 0] for m in dev_meta]).contiguous()
res = {'kernel_launch_only_events': [], 'host_meta_host_sampler': [], 'device_meta_host_sampler': [],
       'device_sampler_events': [], 'device_sampler_wall': []}
for _ in range(9):
    res['host_meta_host_sampler'].append(wall(lambda: host_path(host_meta), 20))
    res['device_sampler_events'].append(events(lambda: dev.sample_indices_device(dev_meta, joint), 2000))
    res['kernel_launch_only_events'].append(
        events(lambda: ops.heatmap_mi_sample(cat_j, cat_v, joint, (4.0, 4.0), (64, 64), 8, 1, 5), 2000))
    res['device_meta_host_sampler'].append(wall(lambda: host_path(dev_meta), 20))
    res['device_sampler_wall'].append(wall(lambda: dev.sample_indices_device(dev_meta, joint), 2000))
for k, v in res.items():
    print('%-28s median %10.1f us  min %10.1f  max %10.1f  (per step: %d views x %d images, Q = 216)'
          % (k, statistics.median(v), min(v), max(v), V, N))
