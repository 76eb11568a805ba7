"""The device sampler of the heatmap mutual-information loss, what can be checked without a GPU:
Philox4x32-10's known answers, the entry point's refusals, the Python switch, and the distribution
of the numpy restatement (tests/heatmap_mi_sampler_restatement.py), which the kernel is held to bit
for bit on the GPU (tests/test_gpu_heatmap_mi_sampler.py).

The distribution bounds are 5 standard deviations of the exact law of each statistic, not
measurements.  With the seed and inputs used here the definition gives: worst inclusion-count
deviation 77 (bound 160), outside chi-square 4117 (bound 4521), invisible-centre chi-squares 92.8
(rows) and 61.1 (columns) (bound 119), at most 8 outside draws for 6 positions."""
import ctypes
import math
import os
import re

import numpy as np
import pytest
import torch

import heatmap_mi_sampler_restatement as S
from posu import _native, ops, synthetic as syn

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SEED, ROWS, RADIUS, CENTRE = 0x5eed0001, 4096, 2, 32 * 64 + 32
P, N_IN, N_OUT = 25, 12, 6


def test_philox_known_answers():
    kat = [((0, 0, 0, 0), (0, 0), '6627e8d5 e169c58d bc57ac4c 9b00dbd8'),
           ((0xffffffff,) * 4, (0xffffffff,) * 2, '408f276d 41c83b0e a20bc7c6 6d5451fd'),
           ((0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344), (0xa4093822, 0x299f31d0),
            'd16cfe09 94fdcceb 5001e420 24126ea1')]
    for counter, key, want in kat:
        assert ' '.join('%08x' % w for w in S.philox4x32_10(counter, key)) == want
    assert S.bounded(0xffffffff, 4096) == 4095 and S.bounded(0, 4096) == 0 and S.bounded(1 << 31, 25) == 12
    assert S.sizes(2) == (P, N_IN, N_OUT) and S.sizes(5) == (121, 60, 30) and S.sizes(8) == (289, 144, 72)


def test_the_symbol_is_declared_and_bound():
    src = re.sub(r'/\*.*?\*/', '', open(os.path.join(REPO, 'include', 'posu.h')).read(), flags=re.S)
    lib = _native.load()
    assert re.search(r'\bposu_heatmap_mi_sample\s*\(', src)
    assert 'posu_heatmap_mi_sample' in _native.exported_symbols() and hasattr(lib, 'posu_heatmap_mi_sample')
    assert lib.posu_abi_version() == _native.ABI_VERSION == 16


def test_argument_limits_are_refused_without_a_gpu():
    """Each limit returns POSU_ERR_ARG with its message before anything is launched; B = 0 succeeds."""
    lib = _native.load()
    p = ctypes.c_void_p(16)

    def run(joints=p, vis=p, B=2, J=16, joint=0, fw=4.0, fh=4.0, H=64, W=64, radius=2, idx=p, loc=p):
        return lib.posu_heatmap_mi_sample(joints, vis, B, J, joint, fw, fh, H, W, radius, 1, 0, idx, loc, None)

    cases = [
        (dict(joints=None), 'null pointer'), (dict(vis=None), 'null pointer'), (dict(idx=None), 'null pointer'),
        (dict(joint=16), 'joint_idx out of range'), (dict(joint=-1), 'joint_idx out of range'),
        (dict(radius=0), 'radius'), (dict(radius=-3), 'radius'),
        (dict(radius=16, H=256, W=256), 'at most 1024 entries'),      # P = 1089
        (dict(H=256, W=257), 'at most 65536 positions'),
        (dict(radius=8, H=26, W=26), 'window too large'),             # P + P / 4 = 361 > 676 / 2
        (dict(radius=2, H=7, W=8), 'window too large'),               # 31 > 28
        (dict(fw=0.0), 'finite and positive'), (dict(fh=-4.0), 'finite and positive'),
        (dict(fw=float('nan')), 'finite and positive'), (dict(fh=float('inf')), 'finite and positive'),
    ]
    for kw, msg in cases:
        assert run(**kw) == 1, kw
        assert 'posu_heatmap_mi_sample' in _native.last_error() and msg in _native.last_error(), \
            (kw, _native.last_error())
    assert run(B=0) == 0
    assert run(B=0, loc=None) == 0
    assert run(B=0, radius=15, H=256, W=256) == 0       # P = 961: the largest window
    assert run(B=0, radius=2, H=8, W=8) == 0            # 31 <= 32: the smallest map for it


def _crit(**kw):
    from core.loss import HeatmapMILoss
    cfg = syn.heatmap_mi_cfg(sigma=0, channels=32, inter_channels=32)
    return HeatmapMILoss(cfg, {'heatmap_discriminator': None}, **kw)


def test_python_refusals_and_sampler_state():
    with pytest.raises(ValueError, match='bogus'):
        _crit(sampler='bogus')
    # the default draws nothing from torch's generator at construction and has no device state
    torch.manual_seed(4)
    want = torch.rand(3)
    torch.manual_seed(4)
    host = _crit()
    assert torch.equal(torch.rand(3), want)
    assert host.sampler == 'host' and host.sampler_state() == {'seed': None, 'calls': 0}
    with pytest.raises(RuntimeError, match="sampler='device'"):
        host.sample_indices_device({}, 0)
    # seed=None: one 63-bit value from the default generator, repeatable under torch.manual_seed
    torch.manual_seed(4)
    a = _crit(sampler='device')
    torch.manual_seed(4)
    b = _crit(sampler='device')
    torch.manual_seed(5)
    c = _crit(sampler='device')
    assert a.sampler_state() == b.sampler_state() and a.sampler_state()['calls'] == 0
    assert 0 <= a.sampler_state()['seed'] < 2 ** 63 and c.sampler_state()['seed'] != a.sampler_state()['seed']
    d = _crit(sampler='device', seed=(7 << 40) + 3)
    assert d.sampler_state() == {'seed': (7 << 40) + 3, 'calls': 0}
    d.load_sampler_state({'seed': 11, 'calls': 5})
    assert d.sampler_state() == {'seed': 11, 'calls': 5}


def test_device_sampler_without_a_gpu_is_refused_not_run_on_the_host(monkeypatch):
    monkeypatch.setattr(torch.cuda, 'is_available', lambda: False)
    case = syn.heatmap_mi_case(3, 2, 8, 32)
    meta = {'joints_2d_transformed': torch.as_tensor(case['joints_2d_transformed']),
            'joints_vis': torch.as_tensor(case['joints_vis'])}
    crit = _crit(sampler='device', seed=1)
    with pytest.raises(RuntimeError, match='cuda'):
        crit.sample_indices_device(meta, 0)
    with pytest.raises(RuntimeError, match='cuda'):
        crit.sample_indices_device([meta, meta], 0)
    with pytest.raises(RuntimeError, match='cuda'):
        ops.heatmap_mi_sample(meta['joints_2d_transformed'], meta['joints_vis'], 0, (4.0, 4.0), (64, 64), 2, 1, 0)
    assert crit.sampler_state()['calls'] == 0      # a refused draw does not advance the stream


@pytest.fixture(scope='module')
def trial():
    """4096 rows of the restatement at the centre of the map: visible (call 0) and invisible (call 1)."""
    joints = np.zeros((ROWS, 1, 2))
    joints[:, 0] = (32 * 4.0, 32 * 4.0)
    stats = []
    idx, loc = S.sample(joints, np.ones((ROWS, 1)), 0, 4.0, 4.0, 64, 64, RADIUS, SEED, 0, stats=stats)
    _, loc_inv = S.sample(joints, np.zeros((ROWS, 1)), 0, 4.0, 4.0, 64, 64, RADIUS, SEED, 1)
    return {'idx': idx, 'loc': loc, 'loc_inv': loc_inv, 'stats': stats}


def test_inside_is_a_uniform_subset_of_the_window_entries(trial):
    idx, window = trial['idx'], S.window_of(CENTRE, RADIUS, 64, 64)
    assert (trial['loc'] == CENTRE).all() and len(set(window)) == P
    for row in idx:
        assert len(set(row[:N_IN].tolist())) == N_IN and set(row[:N_IN].tolist()) <= set(window)
    counts = np.array([(idx[:, :N_IN] == w).sum() for w in window])
    worst = float(np.abs(counts - ROWS * N_IN / P).max())
    bound = 5 * math.sqrt(ROWS * (N_IN / P) * (1 - N_IN / P))
    print('inclusion counts: worst deviation %.2f, bound %.1f' % (worst, bound))
    assert round(bound) == 160 and worst <= 160
    # and in random order: every entry appears in slot 0 about equally often (the same law with 1 / P)
    first = np.array([(idx[:, 0] == w).sum() for w in window])
    assert float(np.abs(first - ROWS / P).max()) <= 5 * math.sqrt(ROWS * (1 / P) * (1 - 1 / P))


def test_outside_positions_are_distinct_uniform_and_off_the_window(trial):
    idx, window = trial['idx'], S.window_of(CENTRE, RADIUS, 64, 64)
    out = idx[:, N_IN:]
    for row in out:
        assert len(set(row.tolist())) == N_OUT and not set(row.tolist()) & set(window)
    counts = np.bincount(out.ravel(), minlength=64 * 64)
    free = np.ones(64 * 64, dtype=bool)
    free[window] = False
    assert counts[~free].sum() == 0 and int(free.sum()) == 4071
    expect = N_OUT * ROWS / 4071.0
    chi2 = float(((counts[free] - expect) ** 2 / expect).sum())
    bound = 4070 + 5 * math.sqrt(2 * 4070)
    print('outside chi-square %.1f, bound %.1f' % (chi2, bound))
    assert math.floor(bound) == 4521 and chi2 <= 4521
    draws = [s['draws'] for s in trial['stats']]
    print('outside draws per row: worst %d for %d positions' % (max(draws), N_OUT))
    assert max(draws) <= 64 * N_OUT and all(s['filled'] == 0 for s in trial['stats'])


def test_invisible_centres_are_uniform_over_the_map(trial):
    loc = trial['loc_inv']
    assert loc.min() >= 0 and loc.max() < 64 * 64
    bound = 63 + 5 * math.sqrt(126)
    assert math.floor(bound) == 119
    for name, bins in (('rows', loc // 64), ('columns', loc % 64)):
        chi2 = float(((np.bincount(bins, minlength=64) - ROWS / 64.0) ** 2 / (ROWS / 64.0)).sum())
        print('invisible centres, %s: chi-square %.2f, bound %.1f' % (name, chi2, bound))
        assert chi2 <= 119


def test_rows_are_independent_of_the_batch():
    """Row k of a batch is row k of the stream: a function of (seed, call, k) and its own inputs."""
    rng = np.random.default_rng(2)
    joints = rng.uniform(-20.0, 280.0, (5, 3, 2))
    vis = (rng.uniform(size=(5, 3)) > 0.4).astype(np.float64)
    idx, loc = S.sample(joints, vis, 1, 4.0, 4.0, 64, 64, 5, (9 << 32) + 1, 3)
    sub, sub_loc = S.sample(joints[2:4], vis[2:4], 1, 4.0, 4.0, 64, 64, 5, (9 << 32) + 1, 3, first_row=2)
    assert np.array_equal(idx[2:4], sub) and np.array_equal(loc[2:4], sub_loc)
    other, _ = S.sample(joints, vis, 1, 4.0, 4.0, 64, 64, 5, (9 << 32) + 1, 4)
    assert all(not np.array_equal(a, b) for a, b in zip(idx, other))


def test_corner_window_repeats_positions_within_the_windows_multiplicities():
    joints = np.zeros((64, 1, 2))
    idx, loc = S.sample(joints, np.ones((64, 1)), 0, 4.0, 4.0, 64, 64, RADIUS, SEED, 2)
    window = S.window_of(0, RADIUS, 64, 64)
    assert (loc == 0).all() and window.count(0) == 13     # the entries before the centre all clamp to 0
    most = 0
    for row in idx:
        inside = row[:N_IN].tolist()
        for pos in set(inside):
            assert inside.count(pos) <= window.count(pos)
        most = max(most, inside.count(0))
        assert len(set(row[N_IN:].tolist())) == N_OUT and not set(row[N_IN:].tolist()) & set(window)
    assert most >= 2


def test_the_bounded_loop_falls_back_to_the_lowest_free_positions(monkeypatch):
    """With the draw limit forced to zero the outside slots are the lowest positions off the window,
    ascending: the branch that bounds the loop, unreachable at the real limit."""
    monkeypatch.setattr(S, 'MAX_DRAWS_PER_SLOT', 0)
    st = {}
    idx, _ = S.sample_row((0.0, 0.0), True, 0, 4.0, 4.0, 64, 64, RADIUS, SEED, 0, stats=st)
    window = set(S.window_of(0, RADIUS, 64, 64))
    assert idx[N_IN:] == [q for q in range(64 * 64) if q not in window][:N_OUT]
    assert st == {'draws': 0, 'filled': N_OUT}
