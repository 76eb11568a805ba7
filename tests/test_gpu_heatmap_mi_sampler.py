"""The device sampler of the heatmap mutual-information loss on the GPU: posu_heatmap_mi_sample
against its numpy restatement (tests/heatmap_mi_sampler_restatement.py) bit for bit, its centres
against HeatmapMILoss.locations, the structure of a draw at the workload's Q, the loss through
HeatmapMILoss(sampler='device') against the host path on the same positions, and a training loop
with heatmap MI on and device-resident metadata that reads nothing between its log lines."""
from collections import Counter

import numpy as np
import pytest
import torch

import heatmap_mi_sampler_restatement as S
from posu import ops, optim, synthetic as syn

pytestmark = pytest.mark.gpu

SEED = (0x9e3779b9 << 32) | 0x5eed0001      # a non-zero high half
J = 16


def edge_rows(feat, joint_idx, seed=0):
    """B = 12 rows of [J, 2] crop px for a 64 x 64 map at `feat` px per map px, the tested joint at: the
    four corners, an edge, the interior, three invisible rows, and coordinates that are negative, at or
    beyond the crop size, exactly on a rounding boundary (v / feat + 0.5 an integer) and just below one."""
    crop = 64.0 * feat
    on = feat * 10.5                                # on / feat + 0.5 == 11 exactly
    below = float(np.nextafter(feat * 20.5, 0.0))   # just below the boundary to 21
    rng = np.random.default_rng(100 + seed)
    joints = rng.uniform(0.0, crop, (12, J, 2))
    vis = np.ones((12, J, 3))
    vis[:, (joint_idx + 1) % J] = 0.0               # a neighbour's flag must not matter
    joints[:9, joint_idx] = [(0.0, 0.0), (crop - 1.0, 0.0), (0.0, crop - 1.0), (crop - 1.0, crop - 1.0),
                             (0.0, 0.43 * crop), (0.37 * crop, 0.61 * crop),
                             (0.5 * crop, 0.5 * crop), (0.0, 0.0), (crop - 1.0, crop - 1.0)]
    vis[6:9, joint_idx] = 0.0
    joints[9:, joint_idx] = [(-7.3, on), (crop, crop + 50.0), (below, -1e-9)]
    return joints, vis


def restated(joints, vis, joint_idx, feat, radius, seed, call):
    return S.sample(joints, vis[:, :, 0], joint_idx, feat, feat, 64, 64, radius, seed, call)


def on_device(joints, vis, joint_idx, feat, radius, seed, call, cuda):
    idx, loc = ops.heatmap_mi_sample(torch.as_tensor(joints).to(cuda), torch.as_tensor(vis).to(cuda), joint_idx,
                                     (feat, feat), (64, 64), radius, seed, call)
    assert idx.is_cuda and loc.is_cuda and idx.dtype == torch.int32 and loc.dtype == torch.int32
    return idx.cpu().numpy(), loc.cpu().numpy()


# ------------------------------------------------------------------ 1. bits
@pytest.mark.parametrize('joint_idx', [0, 15])
@pytest.mark.parametrize('feat', [4.0, 5.0])
@pytest.mark.parametrize('radius', [2, 5, 8])
def test_bits_equal_the_restatement(cuda, radius, feat, joint_idx):
    joints, vis = edge_rows(feat, joint_idx)
    call = 3 + (1 << 33)
    want_idx, want_loc = restated(joints, vis, joint_idx, feat, radius, SEED, call)
    p, n_in, n_out = S.sizes(radius)
    assert want_idx.shape == (12, n_in + n_out) and n_in + n_out == {2: 18, 5: 90, 8: 216}[radius]
    assert want_loc[:6].tolist() == [0, 63, 63 * 64, 64 * 64 - 1, int(0.43 * 64 + 0.5) * 64,
                                     int(0.61 * 64 + 0.5) * 64 + int(0.37 * 64 + 0.5)]
    assert want_loc[9] == 11 * 64 and want_loc[10] == 64 * 64 - 1 and want_loc[11] in (20, 21)
    idx, loc = on_device(joints, vis, joint_idx, feat, radius, SEED, call, cuda)
    assert np.array_equal(loc, want_loc), (loc, want_loc)
    bad = np.nonzero((idx != want_idx).any(axis=1))[0]
    assert bad.size == 0, 'rows %s differ, first: %s vs %s' % (bad.tolist(), idx[bad[0]], want_idx[bad[0]])
    # one row alone, host inputs in f32 (any float dtype is brought to f64 on the device)
    one_j, one_v = joints[5:6].astype(np.float32), vis[5:6].astype(np.float32)
    w_idx, w_loc = restated(one_j.astype(np.float64), one_v, joint_idx, feat, radius, SEED, call)
    g_idx, g_loc = ops.heatmap_mi_sample(torch.as_tensor(one_j), torch.as_tensor(one_v), joint_idx, (feat, feat),
                                         (64, 64), radius, SEED, call)
    assert g_idx.is_cuda and np.array_equal(g_idx.cpu().numpy(), w_idx) and np.array_equal(g_loc.cpu().numpy(), w_loc)


# ------------------------------------------------------------------ 2. row independence
def test_rows_do_not_depend_on_the_batch_and_calls_differ(cuda):
    rng = np.random.default_rng(7)
    joints = rng.uniform(-16.0, 272.0, (130, J, 2))
    vis = (rng.uniform(size=(130, J, 3)) > 0.3).astype(np.float64)
    big, big_loc = on_device(joints, vis, 4, 4.0, 5, SEED, 11, cuda)
    small, small_loc = on_device(joints[:3], vis[:3], 4, 4.0, 5, SEED, 11, cuda)
    assert np.array_equal(big[:3], small) and np.array_equal(big_loc[:3], small_loc)
    again, again_loc = on_device(joints, vis, 4, 4.0, 5, SEED, 11, cuda)
    assert np.array_equal(big, again) and np.array_equal(big_loc, again_loc)
    other, _ = on_device(joints, vis, 4, 4.0, 5, SEED, 12, cuda)
    assert all(not np.array_equal(a, b) for a, b in zip(big, other))
    want, want_loc = restated(joints[120:], vis[120:], 4, 4.0, 5, SEED, 11)
    ref, ref_loc = S.sample(joints[120:], vis[120:, :, 0], 4, 4.0, 4.0, 64, 64, 5, SEED, 11, first_row=120)
    assert np.array_equal(big[120:], ref) and np.array_equal(big_loc[120:], ref_loc)      # beyond one block of rows
    assert not np.array_equal(want, ref)


# ------------------------------------------------------------------ 3. centres against the host
def _crit(cuda, sigma, image_size, **kw):
    from core.loss import HeatmapMILoss
    cfg = syn.heatmap_mi_cfg(sigma=sigma, channels=32, inter_channels=32, image_size=image_size)
    return HeatmapMILoss(cfg, {'heatmap_discriminator': None}, **kw)


@pytest.mark.parametrize('image_size,joint_idx', [(256, 0), (320, 15)])
def test_centres_equal_the_host_locations(cuda, image_size, joint_idx):
    feat = image_size / 64.0
    joints, vis = edge_rows(feat, joint_idx, seed=1)
    meta = {'joints_2d_transformed': torch.as_tensor(joints), 'joints_vis': torch.as_tensor(vis)}
    host = _crit(cuda, 1, image_size).locations(meta, joint_idx)
    dev = _crit(cuda, 1, image_size, sampler='device', seed=SEED)
    on_dev = {k: v.to(cuda) for k, v in meta.items()}
    idx, loc = dev.sample_indices_device(on_dev, joint_idx, return_locations=True)
    visible = vis[:, joint_idx, 0] != 0
    assert visible.sum() == 9
    assert torch.equal(loc.cpu().long()[visible], host[visible])
    assert idx.shape == (12, 90) and dev.sampler_state() == {'seed': SEED, 'calls': 1}
    # the wrapper's draw is the entry point's with (seed, calls); host metadata gives the same bits
    want, _ = restated(joints, vis, joint_idx, feat, 5, SEED, 0)
    assert np.array_equal(idx.cpu().numpy(), want)
    dev.load_sampler_state({'seed': SEED, 'calls': 0})
    assert torch.equal(dev.sample_indices_device(meta, joint_idx), idx)


# ------------------------------------------------------------------ 4. structure at the workload's Q
def test_structure_of_a_draw_at_sigma_2(cuda):
    rng = np.random.default_rng(12)
    b, radius = 256, 8
    joints = rng.uniform(-8.0, 264.0, (b, J, 2))
    joints[:4, 2] = [(0.0, 0.0), (255.0, 0.0), (0.0, 255.0), (255.0, 255.0)]
    vis = (rng.uniform(size=(b, J, 3)) > 0.2).astype(np.float64)
    vis[:4, 2] = 1.0
    meta = {'joints_2d_transformed': torch.as_tensor(joints).to(cuda), 'joints_vis': torch.as_tensor(vis).to(cuda)}
    crit = _crit(cuda, 2, 256, sampler='device', seed=SEED + 1)
    idx, loc = crit.sample_indices_device(meta, 2, return_locations=True)
    p, n_in, n_out = S.sizes(radius)
    assert idx.shape == (b, 216) and n_in == 144 and n_out == 72
    assert int(idx.min()) >= 0 and int(idx.max()) < 4096 and int(loc.min()) >= 0 and int(loc.max()) < 4096
    windows = crit.window(loc.cpu()).tolist()
    rows = idx.cpu().tolist()
    repeated = 0
    for k in range(b):
        win = Counter(windows[k])
        inside, outside = Counter(rows[k][:n_in]), rows[k][n_in:]
        assert all(inside[pos] <= win[pos] for pos in inside), k     # also: inside is a subset of the window
        repeated += max(inside.values()) > 1
        assert len(set(outside)) == n_out and not set(outside) & set(win), k
    assert repeated >= 2          # the corner windows repeat positions


# ------------------------------------------------------------------ 5. the same loss either way
@pytest.mark.parametrize('measure', ['JSD', 'NCE'])
def test_device_and_host_paths_give_the_same_loss_and_gradients(cuda, measure):
    from core.loss import HeatmapMILoss
    from models.discriminator import HeatmapDiscriminator
    n, joint = 4, 3
    cases = [syn.heatmap_mi_case(40 + v, n, 32, 32, joint_idx=joint, corners=(v == 1)) for v in range(2)]
    cfg = syn.heatmap_mi_cfg(sigma=1, channels=32, inter_channels=32, measure=measure, joint_idx=joint)
    metas = [{'joints_2d_transformed': torch.as_tensor(c['joints_2d_transformed']).to(cuda),
              'joints_vis': torch.as_tensor(c['joints_vis']).to(cuda)} for c in cases]

    def run(sampler, indices):
        disc = HeatmapDiscriminator(cfg)
        disc.load_state_dict({k: torch.as_tensor(v) for k, v in cases[0]['state'].items()})
        disc = disc.to(cuda).train()
        crit = HeatmapMILoss(cfg, {'heatmap_discriminator': disc}, sampler=sampler, seed=SEED)
        lows = [torch.as_tensor(c['low_features']).float().to(cuda).requires_grad_(True) for c in cases]
        heats = [torch.as_tensor(c['heatmaps']).float().to(cuda).requires_grad_(True) for c in cases]
        loss = crit.views(lows, heats, None, metas, joint, indices=indices)
        loss.backward()
        out = {'loss': loss.detach()}
        for v in range(2):
            out['dlow%d' % v], out['dheat%d' % v] = lows[v].grad, heats[v].grad
        for k, prm in disc.named_parameters():
            out['grad.' + k] = prm.grad
        for k, buf in disc.named_buffers():
            out['buffer.' + k] = buf.detach().clone()
        return out, crit

    probe = HeatmapMILoss(cfg, {'heatmap_discriminator': None}, sampler='device', seed=SEED)
    drawn = probe.sample_indices_device(metas, joint)               # [2 N, Q], view-major
    assert drawn.shape == (2 * n, 90)
    host_copies = [drawn[v * n:(v + 1) * n].cpu().long() for v in range(2)]
    dev, crit = run('device', None)
    assert crit.sampler_state()['calls'] == 1                       # both views in one launch
    host, _ = run('host', host_copies)
    assert sorted(dev) == sorted(host) and len(dev) == 1 + 4 + 9 + 6
    assert np.isfinite(float(dev['loss']))
    for k in dev:
        assert torch.equal(dev[k], host[k]), k
    assert float(dev['dlow1'].abs().max()) > 0 and float(dev['dheat0'].abs().max()) > 0
    # device indices handed in: per view and as one tensor, the same bits again
    for given in ([drawn[:n], drawn[n:]], drawn, drawn.long()):
        again, _ = run('device', given)
        for k in dev:
            assert torch.equal(dev[k], again[k]), k


# ------------------------------------------------------------------ 6. no reads in the loop
def _loop(cuda, monkeypatch, epoch, sampler):
    from core.function import train
    from core.loss import HeatmapMILoss, JointsMSELoss
    from models.discriminator import HeatmapDiscriminator
    from test_gpu_train_loop import _Data, _ReadCounters, _Stub
    cfg = syn.train_loop_cfg(image_size=256, fundamental=False, watch_grad_norm=False, heatmap_mi=True, sigma=0,
                             mi_channels=32, mi_inter_channels=32)
    batches = syn.train_loop_batches(3, nviews=4, batch=2, image_size=256, seed=5, target_sigma=2.0)
    for _, _, _, meta in batches:       # as posu.datapath.BatchMaker returns them: f64 on the device
        for m in meta:
            for key in ('joints_2d_transformed', 'joints_vis'):
                m[key] = m[key].to(device=cuda, dtype=torch.float64)
    stub = _Stub(2).to(cuda)
    torch.manual_seed(9)
    disc = HeatmapDiscriminator(cfg).to(cuda)
    opts = {'base_model': optim.Adam(stub.parameters(), lr=1e-2),
            'heatmap_discriminator': optim.Adam(disc.parameters(), lr=1e-2)}
    crits = {'mse_weights': JointsMSELoss(use_target_weight=True),
             'heatmap_mi': HeatmapMILoss(cfg, {'heatmap_discriminator': disc}, sampler=sampler)}
    with monkeypatch.context() as mp:
        counters = _ReadCounters(mp)
        final = train(cfg, _Data(batches, counters), {'base_model': stub, 'heatmap_discriminator': disc}, crits, opts,
                      epoch, '', None, 0)
        torch.cuda.synchronize()
    return final, list(counters.calls), crits['heatmap_mi']


def test_train_with_heatmap_mi_reads_nothing_between_log_lines(cuda, monkeypatch):
    for epoch, meter, other in ((0, 'hmi_d', 'hmi_g'), (1, 'hmi_g', 'hmi_d')):
        final, calls, crit = _loop(cuda, monkeypatch, epoch, 'device')
        assert calls == [], (epoch, calls)
        assert final[meter]['count'] == 3 and final[other]['count'] == 0
        assert np.isfinite(final[meter]['avg']) and np.isfinite(final[meter]['val'])
        assert crit.sampler_state()['calls'] == 3       # one launch per step for the four views
    # the control: the host sampler on the same batches reads the metadata back, and the counters see it
    final, calls, _ = _loop(cuda, monkeypatch, 0, 'host')
    assert 'cpu' in calls, calls
    assert final['hmi_d']['count'] == 3 and np.isfinite(final['hmi_d']['avg'])
