"""Heatmap mutual-information loss on the GPU: the fused pair-score / measure kernels against the
materialising plain-torch restatement (tests/heatmap_mi_restatement.py) run in fp64 on the same
device with the golden's positions.

Tolerance, per quantity: the restatement is also run in fp32 and its error against fp64, normalised
by the fp64 maximum, is the yardstick; the kernels must be within max(4 x that, 2^-20).  Both are
fp32 evaluations that differ in summation order.  Every test prints the ratios it measured."""
import numpy as np
import pytest
import torch

import heatmap_mi_restatement as R
from posu import synthetic as syn

pytestmark = pytest.mark.gpu

FLOOR = 2.0 ** -20


def _spec(g, name):
    seed, n, c, cm, sigma, joint, corners, training = [int(v) for v in g['%s.spec' % name]]
    case = syn.heatmap_mi_case(seed, n, c, cm, joint_idx=joint, corners=bool(corners))
    return case, dict(n=n, c=c, cm=cm, sigma=sigma, joint=joint, training=bool(training))


@pytest.fixture(scope='module')
def mi_golden(golden):
    return golden('heatmap_mi.npz')


def build(case, spec, measure, cuda, training=True):
    from core.loss import HeatmapMILoss
    from models.discriminator import HeatmapDiscriminator
    cfg = syn.heatmap_mi_cfg(sigma=spec['sigma'], channels=spec['c'], inter_channels=spec['cm'], measure=measure,
                             joint_idx=spec['joint'])
    disc = HeatmapDiscriminator(cfg)
    disc.load_state_dict({k: torch.as_tensor(v) for k, v in case['state'].items()})
    disc = disc.to(cuda).train(training)
    return HeatmapMILoss(cfg, {'heatmap_discriminator': disc}), disc


def channels_last(a, cuda, dtype=torch.float32):
    """[N, C, H, W] logical over [N, H, W, C] memory: what the backbone hands over."""
    t = torch.as_tensor(a).to(cuda).to(dtype)
    return t.permute(0, 2, 3, 1).contiguous().permute(0, 3, 1, 2)


def run_fused(case, spec, idx, measure, cuda, training=True, feature_dtype=torch.float32, detach=False):
    crit, disc = build(case, spec, measure, cuda, training)
    low = channels_last(case['low_features'], cuda, feature_dtype)
    heat = torch.as_tensor(case['heatmaps']).to(cuda).float()
    if not detach:
        low.requires_grad_(True)
        heat.requires_grad_(True)
    u = disc.pair_scores(low, heat, torch.as_tensor(idx), spec['joint'])
    from posu import ops
    val = ops.pair_mi_loss(u, measure, 1)[0]
    val.backward()
    torch.cuda.synchronize()
    out = {'loss': val.detach(), 'u': u.detach()}
    if not detach:
        n, q, c = spec['n'], idx.shape[1], spec['c']
        ix = torch.as_tensor(idx).long().to(cuda)
        out['dlow'], out['dheat'] = low.grad, heat.grad
        out['dlow_at'] = low.grad.permute(0, 2, 3, 1).reshape(n, -1, c).gather(1, ix[:, :, None].expand(n, q, c))
        out['dheat_at'] = heat.grad[:, spec['joint']].reshape(n, -1).gather(1, ix)
    else:
        assert low.grad is None and heat.grad is None
    sd = disc.state_dict()
    for k, p in disc.named_parameters():
        out['grad.' + k] = p.grad
    for k in R.BUFFER_KEYS:
        out['buffer.' + k] = sd[k]
    out['tracked'] = (int(sd['block_nonlinear.1.num_batches_tracked']), int(sd['block_nonlinear.4.num_batches_tracked']))
    return out


def compare(got, ref64, ref32, keys, label, special=None):
    """max |got - ref64| / max |ref64| against max(4 x the fp32 restatement's, 2^-20), per quantity."""
    bad = []
    for k in keys:
        r64 = ref64[k].double()
        scale = max(float(r64.abs().max()), 1e-300)
        e32 = float((ref32[k].double() - r64).abs().max()) / scale
        err = float((got[k].double().reshape(r64.shape) - r64).abs().max()) / scale
        bound = (special or {}).get(k, max(4.0 * e32, FLOOR))
        print('%s %-40s kernel %.3e  fp32 restatement %.3e  ratio %.2f  bound %.3e'
              % (label, k, err, e32, err / max(e32, 1e-300), bound))
        if not err <= bound:
            bad.append((k, err, bound))
    assert not bad, bad


def all_keys(with_inputs=True, training=True):
    keys = ['loss', 'u'] + ['grad.' + k for k in R.PARAM_KEYS]
    if with_inputs:
        keys += ['dlow_at', 'dheat_at']
    if training:
        keys += ['buffer.' + k for k in R.BUFFER_KEYS]
    return keys


_REF = {}


def references(case, spec, idx, measure, cuda, training, feature_dtype=None):
    """fp64 and fp32 restatement of one case, computed once and shared."""
    key = (id(case), measure, training, feature_dtype)
    if key not in _REF:
        _REF[key] = tuple(R.evaluate(case, idx, spec['joint'], measure, training, dt, cuda, feature_dtype)
                          for dt in (torch.float64, torch.float32))
    return _REF[key]


def off_sample_zero(got, idx, spec, cuda):
    n, c = spec['n'], spec['c']
    mask = torch.zeros(n, 64 * 64, dtype=torch.bool, device=cuda)
    mask.scatter_(1, torch.as_tensor(idx).long().to(cuda), True)
    dl = got['dlow'].permute(0, 2, 3, 1).reshape(n, -1, c)
    assert float(dl[~mask].float().abs().max()) == 0.0
    dh = got['dheat'].clone()
    assert float(dh[:, spec['joint']].reshape(n, -1)[~mask].abs().max()) == 0.0
    dh[:, spec['joint']] = 0
    assert float(dh.abs().max()) == 0.0


@pytest.fixture(scope='module')
def case_a(mi_golden):
    return _spec(mi_golden, 'A')


@pytest.mark.parametrize('measure', ['JSD', 'NCE'])
def test_case_a_train(mi_golden, case_a, cuda, measure):
    case, spec = case_a
    idx = mi_golden['A.%s.indices' % measure]
    ref64, ref32 = references(case, spec, idx, measure, cuda, True)
    # the fp64 restatement on the device is the golden's (the CPU test pins it to 1e-12)
    assert abs(float(ref64['loss']) - float(mi_golden['A.%s.loss' % measure])) <= 1e-11 * abs(float(ref64['loss']))
    got = run_fused(case, spec, idx, measure, cuda)
    compare(got, ref64, ref32, all_keys(), 'A/' + measure)
    off_sample_zero(got, idx, spec, cuda)
    # repeated positions hold the sum over their occurrences: equal values at equal positions
    dup = 0
    for n in range(spec['n']):
        row = idx[n].tolist()
        for i, pos in enumerate(row):
            j = row.index(pos)
            if j != i:
                dup += 1
                assert torch.equal(got['dlow_at'][n, i], got['dlow_at'][n, j])
                assert torch.equal(got['dheat_at'][n, i], got['dheat_at'][n, j])
    assert dup > 0
    assert got['tracked'] == (4, 4)


def test_case_b_workload_widths(mi_golden, cuda):
    case, spec = _spec(mi_golden, 'B')
    idx = mi_golden['B.JSD.indices']
    ref64, ref32 = references(case, spec, idx, 'JSD', cuda, True)
    got = run_fused(case, spec, idx, 'JSD', cuda)
    compare(got, ref64, ref32, all_keys(), 'B/JSD')
    off_sample_zero(got, idx, spec, cuda)


@pytest.mark.parametrize('measure', ['JSD', 'NCE'])
def test_case_c_eval(mi_golden, cuda, measure):
    case, spec = _spec(mi_golden, 'C')
    idx = mi_golden['C.%s.indices' % measure]
    ref64, ref32 = references(case, spec, idx, measure, cuda, False)
    got = run_fused(case, spec, idx, measure, cuda, training=False)
    compare(got, ref64, ref32, all_keys(training=False), 'C/' + measure)
    for k in R.BUFFER_KEYS:   # eval() leaves the buffers alone
        assert torch.equal(got['buffer.' + k].cpu(), torch.as_tensor(case['state'][k]).float())
    assert got['tracked'] == (3, 3)


def test_two_segments_equal_two_calls(mi_golden, case_a, cuda):
    """views() over two different views = the two per-view calls summed; the buffers = two
    sequential updates."""
    case0, spec = case_a
    case1 = syn.heatmap_mi_case(77, spec['n'], spec['c'], spec['cm'], joint_idx=spec['joint'], corners=True)
    idx0, idx1 = mi_golden['A.JSD.indices'], mi_golden['A.NCE.indices']

    def inputs(case):
        low = channels_last(case['low_features'], cuda).requires_grad_(True)
        heat = torch.as_tensor(case['heatmaps']).to(cuda).float().requires_grad_(True)
        return low, heat
    crit, disc = build(case0, spec, 'JSD', cuda)
    (l0, h0), (l1, h1) = inputs(case0), inputs(case1)
    total = crit.views([l0, l1], [h0, h1], [None, None], [None, None], spec['joint'],
                       indices=[torch.as_tensor(idx0), torch.as_tensor(idx1)])
    total.backward()
    crit2, disc2 = build(case0, spec, 'JSD', cuda)
    (m0, g0), (m1, g1) = inputs(case0), inputs(case1)
    seq = crit2(m0, g0, None, None, spec['joint'], indices=torch.as_tensor(idx0)) \
        + crit2(m1, g1, None, None, spec['joint'], indices=torch.as_tensor(idx1))
    seq.backward()
    torch.cuda.synchronize()
    assert abs(float(total.detach()) - float(seq.detach())) <= 2.0 ** -22 * abs(float(seq.detach()))
    for a, b in ((l0, m0), (l1, m1), (h0, g0), (h1, g1)):
        assert torch.equal(a.grad, b.grad)     # per-segment work is the same arithmetic
    for (k, p), (_, p2) in zip(disc.named_parameters(), disc2.named_parameters()):
        scale = float(p2.grad.abs().max())
        assert float((p.grad - p2.grad).abs().max()) <= 2.0 ** -20 * scale, k   # summed in another order
    for (k, b), (_, b2) in zip(disc.named_buffers(), disc2.named_buffers()):
        assert torch.equal(b, b2), k
    assert int(disc.block_nonlinear[1].num_batches_tracked) == 5


def test_forward_on_plain_rows(cuda):
    """forward(embd) on [37, c_in] = the restatement's plain MLP; gradients via a random cotangent."""
    spec = dict(n=1, c=32, cm=32, sigma=0, joint=0)
    case = syn.heatmap_mi_case(5, 1, 32, 32)
    rng = np.random.default_rng(9)
    embd = rng.standard_normal((37, 33))
    cot = rng.standard_normal((37, 1))
    _, disc = build(case, spec, 'JSD', cuda)

    def restated(dtype):
        x = torch.as_tensor(embd).to(cuda, dtype).requires_grad_(True)
        state = {k: torch.as_tensor(v).to(cuda, dtype) for k, v in case['state'].items() if 'num_batches' not in k}
        for k in R.PARAM_KEYS:
            state[k].requires_grad_(True)
        buffers = {k: state[k].clone() for k in R.BUFFER_KEYS}
        y = R.discriminator(x, state, True, buffers)
        grads = torch.autograd.grad(y, [x] + [state[k] for k in R.PARAM_KEYS], torch.as_tensor(cot).to(cuda, dtype))
        out = {'y': y.detach(), 'dx': grads[0]}
        out.update({'grad.' + k: g for k, g in zip(R.PARAM_KEYS, grads[1:])})
        out.update({'buffer.' + k: buffers[k] for k in R.BUFFER_KEYS})
        return out
    ref64, ref32 = restated(torch.float64), restated(torch.float32)
    x = torch.as_tensor(embd).to(cuda).float().requires_grad_(True)
    y = disc(x)
    assert y.shape == (37, 1)
    y.backward(torch.as_tensor(cot).to(cuda).float())
    torch.cuda.synchronize()
    got = {'y': y.detach(), 'dx': x.grad}
    got.update({'grad.' + k: p.grad for k, p in disc.named_parameters()})
    sd = disc.state_dict()
    got.update({'buffer.' + k: sd[k] for k in R.BUFFER_KEYS})
    compare(got, ref64, ref32, list(ref64), 'rows')


def test_bf16_features(mi_golden, case_a, cuda):
    """bf16 feature storage against the restatement fed the same rounded features: the same bound
    for the loss and the parameter gradients, one bf16 rounding (2^-8 of the maximum) for the
    feature gradient."""
    case, spec = case_a
    idx = mi_golden['A.JSD.indices']
    ref64, ref32 = references(case, spec, idx, 'JSD', cuda, True, torch.bfloat16)
    got = run_fused(case, spec, idx, 'JSD', cuda, feature_dtype=torch.bfloat16)
    assert got['dlow'].dtype == torch.bfloat16
    compare(got, ref64, ref32, all_keys(), 'A/bf16', special={'dlow_at': 2.0 ** -8})
    off_sample_zero(got, idx, spec, cuda)


def test_discriminator_step_skips_input_gradients(mi_golden, case_a, cuda):
    case, spec = case_a
    idx = mi_golden['A.JSD.indices']
    full = run_fused(case, spec, idx, 'JSD', cuda)
    det = run_fused(case, spec, idx, 'JSD', cuda, detach=True)   # asserts the inputs got no gradient
    for k in R.PARAM_KEYS:
        assert torch.equal(full['grad.' + k], det['grad.' + k]), k


def test_two_identical_calls_are_bit_identical(mi_golden, cuda):
    case, spec = _spec(mi_golden, 'B')
    idx = mi_golden['B.JSD.indices']
    a = run_fused(case, spec, idx, 'JSD', cuda)
    b = run_fused(case, spec, idx, 'JSD', cuda)
    for k in a:
        if k != 'tracked':
            assert torch.equal(a[k], b[k]), k


def test_wide_discriminator_c_m_128(cuda):
    """c_m = 128 takes the two-wave blocks of the pair passes: a small shape against the restatement."""
    spec = dict(n=2, c=16, cm=128, sigma=0, joint=1)
    case = syn.heatmap_mi_case(31, 2, 16, 128, joint_idx=1)
    from core.loss import HeatmapMILoss
    crit = HeatmapMILoss(syn.heatmap_mi_cfg(sigma=0, channels=16, inter_channels=128), {'heatmap_discriminator': None})
    meta = {'joints_2d_transformed': case['joints_2d_transformed'], 'joints_vis': case['joints_vis']}
    idx = crit.sample_indices(meta, 1, generator=torch.Generator().manual_seed(2)).numpy()
    ref64, ref32 = references(case, spec, idx, 'JSD', cuda, True)
    got = run_fused(case, spec, idx, 'JSD', cuda)
    compare(got, ref64, ref32, all_keys(), 'cm128')


@pytest.mark.parametrize('n,q,c,cm', [(1, 192, 8, 128), (129, 16, 8, 32), (5, 7, 8, 64)],
                         ids=['three_b3_slabs', 'two_chunks_per_block', 'one_slab_ragged_waves'])
def test_pair_walk_edges(cuda, n, q, c, cm):
    """Walks of the pair passes no other case takes, against the restatement (JSD, training):
    1 x 192, c_m 128: four j slabs, three in k_b3 (its dA buffers summed by k_sum_slabs);
    129 x 16, c_m 32: 33 chunks over 32 blocks, block 0 walks two (k_b2 / k_b3 re-zero their per-chunk
    state, k_b3 overwrites A in place between them);
    5 x 7, c_m 64: one slab whose 7 values of j are no multiple of the four waves.
    Positions are seeded draws with one repeated per image."""
    spec = dict(n=n, c=c, cm=cm, sigma=0, joint=1)
    case = syn.heatmap_mi_case(900 + q, n, c, cm, joint_idx=1)
    idx = np.random.default_rng(q).integers(0, 64 * 64, (n, q)).astype(np.int32)
    idx[:, -1] = idx[:, 0]
    # one use each: not through references(), whose cache is keyed on the identity of a case that lives on
    ref64, ref32 = (R.evaluate(case, idx, 1, 'JSD', True, dt, cuda, None) for dt in (torch.float64, torch.float32))
    got = run_fused(case, spec, idx, 'JSD', cuda)
    compare(got, ref64, ref32, all_keys(), 'walk %dx%d cm%d' % (n, q, cm))


def test_micro_step_moves_the_discriminator(cuda):
    """views() over four synthetic 64 x 64 views, backward, one posu.optim.Adam step on the
    discriminator (no backbone of the suite has 64 x 64 maps at a size it trains cheaply)."""
    from posu.optim import Adam
    spec = dict(n=2, c=32, cm=32, sigma=1, joint=2)
    cases = [syn.heatmap_mi_case(40 + v, 2, 32, 32, joint_idx=2) for v in range(4)]
    crit, disc = build(cases[0], spec, 'JSD', cuda)
    before = [p.detach().clone() for p in disc.parameters()]
    opt = Adam(disc.parameters(), lr=1e-3)
    lows = [channels_last(c['low_features'], cuda, torch.bfloat16) for c in cases]
    heats = [torch.as_tensor(c['heatmaps']).to(cuda).float() for c in cases]
    metas = [{'joints_2d_transformed': torch.as_tensor(c['joints_2d_transformed']),
              'joints_vis': torch.as_tensor(c['joints_vis'])} for c in cases]
    loss = crit.views(lows, heats, [None] * 4, metas, spec['joint'])
    opt.zero_grad()
    loss.backward()
    opt.step()
    torch.cuda.synchronize()
    assert np.isfinite(float(loss.detach()))
    for b, p in zip(before, disc.parameters()):
        assert bool(torch.isfinite(p).all()) and not torch.equal(b, p.detach())
    assert int(disc.block_nonlinear[4].num_batches_tracked) == 3 + 4
