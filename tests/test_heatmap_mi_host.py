"""Heatmap mutual-information loss, the checks that need no GPU: the plain-torch restatement
against the reference's golden numbers in fp64, the position sampling, the host-side refusals of
the entry points, the module's state_dict and the workspace bound."""
import ctypes

import numpy as np
import pytest
import torch

import heatmap_mi_restatement as R
from posu import _native, ops, synthetic as syn

GOLDEN_CASES = [('A', 'JSD'), ('A', 'NCE'), ('B', 'JSD'), ('C', 'JSD'), ('C', 'NCE')]


def case_of(g, name):
    seed, n, c, cm, sigma, joint, corners, training = [int(v) for v in g['%s.spec' % name]]
    case = syn.heatmap_mi_case(seed, n, c, cm, joint_idx=joint, corners=bool(corners))
    return case, dict(n=n, c=c, cm=cm, sigma=sigma, joint=joint, training=bool(training))


def golden_quantities(g, name, measure):
    pre = '%s.%s.' % (name, measure)
    return {k[len(pre):]: v for k, v in g.items() if k.startswith(pre) and not k.endswith('indices')}


@pytest.fixture(scope='module')
def mi_golden(golden):
    return golden('heatmap_mi.npz')


@pytest.mark.parametrize('name,measure', GOLDEN_CASES)
def test_restatement_reproduces_the_reference_in_fp64(mi_golden, name, measure):
    """Every golden quantity to 1e-12 of its largest magnitude: pins the row order (n, i, j), both
    measures, the buffer updates and the accumulation at repeated positions."""
    case, spec = case_of(mi_golden, name)
    idx = mi_golden['%s.%s.indices' % (name, measure)]
    assert any(len(set(r.tolist())) < len(r) for r in idx), 'the case is meant to repeat positions'
    got = R.evaluate(case, idx, spec['joint'], measure, spec['training'], torch.float64, 'cpu')
    want = golden_quantities(mi_golden, name, measure)
    assert {'loss', 'dlow_at', 'dheat_at'} <= set(want) and len(want) == 3 + 9 + 6
    for k, ref in want.items():
        if k.endswith('num_batches_tracked'):
            assert int(ref) == 3 + int(spec['training'])
            continue
        have = got[k].detach().numpy()
        tol = 1e-12 if ref.dtype == np.float64 else 2.0 ** -23   # case B's input gradients are f32 casts
        scale = max(float(np.abs(ref).max()), 1e-300)
        assert float(np.abs(have.reshape(ref.shape) - ref).max()) <= tol * scale, k
    # dense gradients: nothing off the sampled positions or off the joint's map
    mask = torch.zeros(spec['n'], 64 * 64, dtype=torch.bool)
    mask.scatter_(1, torch.as_tensor(idx).long(), True)
    dl = got['dlow'].permute(0, 2, 3, 1).reshape(spec['n'], -1, spec['c'])
    assert float(dl[~mask].abs().max()) == 0.0
    dh = got['dheat'].clone()
    assert float(dh[:, spec['joint']].reshape(spec['n'], -1)[~mask].abs().max()) == 0.0
    dh[:, spec['joint']] = 0
    assert float(dh.abs().max()) == 0.0


@pytest.mark.parametrize('sigma', [0, 1, 2])
def test_sample_indices_properties(sigma):
    from core.loss import HeatmapMILoss
    joint, n = 4, 6
    cfg = syn.heatmap_mi_cfg(sigma=sigma, channels=32, inter_channels=32, joint_idx=joint)
    crit = HeatmapMILoss(cfg, {'heatmap_discriminator': None})
    case = syn.heatmap_mi_case(21 + sigma, n, 8, 32, joint_idx=joint, corners=True)
    meta = {'joints_2d_transformed': torch.as_tensor(case['joints_2d_transformed']),
            'joints_vis': torch.as_tensor(case['joints_vis'])}
    gen = torch.Generator().manual_seed(5)
    p = (2 * (3 * sigma + 2) + 1) ** 2
    seen_other_window = False
    for _ in range(4):
        idx, loc = crit.sample_indices(meta, joint, generator=gen, return_locations=True)
        assert idx.shape == (n, p // 2 + p // 4) and idx.dtype == torch.int64
        assert int(idx.min()) >= 0 and int(idx.max()) < 64 * 64
        win = crit.window(loc)
        assert win.shape == (n, p)
        gt = (torch.as_tensor(case['joints_2d_transformed'][:, joint]) / 4.0 + 0.5).long().clamp(0, 63)
        gt = gt[:, 1] * 64 + gt[:, 0]
        for k in range(n):
            inside, outside = idx[k, :p // 2].tolist(), idx[k, p // 2:].tolist()
            w = set(win[k].tolist())
            assert set(inside) <= w
            assert not (set(outside) & w) and len(set(outside)) == len(outside)
            if k != 2:
                assert int(loc[k]) == int(gt[k])    # visible joints: the ground-truth location
        assert int(loc[0]) == 0 and int(loc[1]) == 64 * 64 - 1   # the corners
        seen_other_window |= int(loc[2]) != int(gt[2])
    assert seen_other_window   # the invisible joint's window is a random one, not the ground truth's


def _table(n=13, value=16):
    tab = (ctypes.c_void_p * n)()
    for k in range(n):
        tab[k] = value
    return tab


def test_pair_score_limits_are_refused_without_a_gpu():
    """Each limit returns POSU_ERR_ARG with its message before anything is launched."""
    lib = _native.load()
    p = ctypes.c_void_p(16)
    tab = _table()
    good_idx = np.zeros(2 * 18, dtype=np.int32)

    def fwd(dtype=_native.F32, S=1, N=2, H=64, W=64, C=32, J=16, joint=0, idx_host=good_idx, Q=18, cm=32, params=tab,
            feat=p, ws=p, ws_bytes=1 << 40):
        return lib.posu_heatmap_pair_scores_fwd(dtype, feat, p, S, N, H, W, C, J, joint, p, idx_host.ctypes.data, Q,
                                                cm, params, 1, 1e-5, p, p, ws, ws_bytes, None)

    def bwd(**kw):
        a = dict(dtype=_native.F32, S=1, N=2, H=64, W=64, C=32, J=16, joint=0, Q=18, cm=32)
        a.update(kw)
        return lib.posu_heatmap_pair_scores_bwd(a['dtype'], p, p, a['S'], a['N'], a['H'], a['W'], a['C'], a['J'],
                                                a['joint'], p, good_idx.ctypes.data, a['Q'], a['cm'], tab, 1, 1e-5, p,
                                                p, p, p, p, p, 1 << 40, None)
    bad = good_idx.copy()
    bad[7] = 64 * 64
    neg = good_idx.copy()
    neg[0] = -1
    null_w2 = _table()
    null_w2[5] = None
    cases = [
        (dict(cm=48), 'c_m must be 32, 64 or 128'), (dict(cm=256), 'c_m must be 32, 64 or 128'),
        (dict(C=36), 'multiple of 8'), (dict(C=520), 'at most 512'),
        (dict(Q=257), 'Q must be in 1..256'),
        (dict(idx_host=bad), 'index outside'), (dict(idx_host=neg), 'index outside'),
        (dict(joint=16), 'joint_idx out of range'), (dict(joint=-1), 'joint_idx out of range'),
        (dict(N=4000, Q=256, cm=128, idx_host=np.zeros(4000 * 256, dtype=np.int32)), 'below 2^31'),
        (dict(feat=None), 'null pointer'), (dict(params=null_w2), 'null pointer'),
        (dict(dtype=_native.F16X3), 'POSU_F32, POSU_BF16 or POSU_F16'),
        (dict(ws_bytes=1024), 'workspace too small'),
    ]
    for kw, msg in cases:
        assert fwd(**kw) == 1, kw
        assert msg in _native.last_error(), (kw, _native.last_error())
    for kw, msg in [(dict(cm=48), 'c_m must be'), (dict(C=36), 'multiple of 8'), (dict(Q=300), 'Q must be'),
                    (dict(joint=99), 'joint_idx out of range')]:
        assert bwd(**kw) == 1 and msg in _native.last_error(), kw
    assert lib.posu_heatmap_mi_workspace(1, 2, 257, 32, None) == -1
    assert lib.posu_heatmap_mi_workspace(1, 2, 18, 48, None) == -1
    # the measures
    assert lib.posu_pair_mi_loss_fwd(p, 1, 2, 18, 2, p, p, 1 << 20, None) == 1 and 'measure' in _native.last_error()
    assert lib.posu_pair_mi_loss_fwd(None, 1, 2, 18, 0, p, p, 1 << 20, None) == 1
    assert 'null pointer' in _native.last_error()
    assert lib.posu_pair_mi_loss_fwd(p, 1, 2, 1, 0, p, p, 1 << 20, None) == 1 and 'Q >= 2' in _native.last_error()
    assert lib.posu_pair_mi_loss_bwd(p, 1, 2, 18, 0, None, p, None) == 1 and 'null pointer' in _native.last_error()


def test_workspace_stays_within_the_stated_bound():
    """At the workload shape (4 views, N = 8, sigma = 2, c_m = 64): at most S N Q^2 * 4 +
    S N Q (c_m + 4) floats plus the reductions' own bytes, which depend on the grid, not on the
    pairs.  Arithmetic only."""
    S, N, Q, cm = 4, 8, 216, 64
    total, red = ops.heatmap_mi_workspace(S, N, Q, cm)
    assert 0 < red < total
    assert total - red <= 4 * (S * N * Q * Q * 4 + S * N * Q * (cm + 4))
    # nothing 16 or 64 wide per pair: one scalar per pair and at most two floats per pair of dA slab buffers
    assert total - red <= 4 * (S * N * Q * (cm + 4) + 3 * S * N * Q * Q)
    # the grid is capped, and the partial count with it: more images, the same reduction bytes
    _, red_cap = ops.heatmap_mi_workspace(1, 2 * N, Q, cm)
    _, red_cap2 = ops.heatmap_mi_workspace(1, 8 * N, Q, cm)
    assert red_cap == red_cap2


def test_state_dict_is_the_reference_modules():
    from models.discriminator import HeatmapDiscriminator
    for channels, cm in ((256, 64), (32, 32)):
        d = HeatmapDiscriminator(syn.heatmap_mi_cfg(channels=channels, inter_channels=cm))
        sd = d.state_dict()
        assert list(sd) == [k for k, _ in R.STATE_LAYOUT]
        for k, shape in R.STATE_LAYOUT:
            assert tuple(sd[k].shape) == shape(channels + 1, cm), k
        case = syn.heatmap_mi_case(1, 1, channels, cm)
        d.load_state_dict({k: torch.as_tensor(v) for k, v in case['state'].items()})


def test_cpu_tensors_and_unbuilt_losses_raise():
    from core import loss as L
    from models import discriminator as D
    cfg = syn.heatmap_mi_cfg(channels=32, inter_channels=32, sigma=0)
    d = D.HeatmapDiscriminator(cfg)
    with pytest.raises(RuntimeError, match='cuda'):
        d(torch.zeros(5, 33))
    with pytest.raises(RuntimeError, match='cuda'):
        d.pair_scores(torch.zeros(1, 32, 64, 64), torch.zeros(1, 16, 64, 64), torch.zeros(1, 18, dtype=torch.long), 0)
    with pytest.raises(RuntimeError, match='cuda'):
        ops.pair_mi_loss(torch.zeros(2, 3, 3), 'JSD')
    crit = L.HeatmapMILoss(cfg, {'heatmap_discriminator': d})
    with pytest.raises(NotImplementedError, match='64 x 64'):
        crit(torch.zeros(1, 32, 32, 32), torch.zeros(1, 16, 32, 32), None, {}, 0, indices=torch.zeros(1, 18))
    for ctor in (L.MILoss, L.ViewMILoss, L.JointsMILoss, D.LocalDiscriminator, D.DomainDiscriminator):
        with pytest.raises(NotImplementedError):
            ctor(cfg)
    with pytest.raises(NotImplementedError):
        D.HeatmapDiscriminator(syn.heatmap_mi_cfg(channels=32, inter_channels=48))
