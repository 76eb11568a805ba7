"""Loss scaling on the device (fp16 training): the gradient statistics pass (posu_grad_stats),
Adam with its step counts, the scale and the overflow flag in device memory (posu_adam_step_dev)
against the host-stepped kernel, the scale's update (posu_loss_scale_update), and
posu.amp.LossScaler over them: no host synchronisation, graph capture, torch's own GradScaler."""
import numpy as np
import pytest
import torch

from posu import amp, optim

pytestmark = pytest.mark.gpu

# empty, below / at / above a float4, a ragged tail, one chunk -1 / exact / +1, several chunks + tail
SIZES = [0, 1, 3, 4, 7, 2047, 2048, 2049, 3 * 4096 + 5]
NTENSORS = 130        # three launches of <= 64 tensors
UNALIGNED = 16        # this tensor (2049 elements) is a view one float into its storage


def _tensors(cuda, seed):
    g = torch.Generator(device=cuda).manual_seed(seed)
    out = []
    for i in range(NTENSORS):
        n = SIZES[i % len(SIZES)]
        t = torch.randn(n + 1, device=cuda, generator=g) * (10.0 ** (i % 5 - 2))
        out.append(t[1:] if i == UNALIGNED else t[:n].clone())
    assert out[UNALIGNED].data_ptr() % 16 == 4 and out[UNALIGNED].numel() == 2049
    return out


@pytest.fixture(scope='module')
def grads(cuda):
    return _tensors(cuda, 7)


def _stats(cuda, ts, **kw):
    st = optim.GradStats(cuda)
    st.run(ts, **kw)
    return float(st.found_inf.item()), st.sumsq.item()


def test_stats_sum_of_squares_matches_fp64_and_repeats_bit_for_bit(cuda, grads):
    ref = sum(float((t.cpu().numpy().astype(np.float64) ** 2).sum()) for t in grads)
    found, ss = _stats(cuda, grads)
    found2, ss2 = _stats(cuda, grads)
    print('sumsq %.17g, numpy fp64 %.17g, rel %.3g' % (ss, ref, abs(ss / ref - 1)))
    assert found == 0.0 and found2 == 0.0
    np.testing.assert_allclose(ss, ref, rtol=1e-12)
    assert np.float64(ss).tobytes() == np.float64(ss2).tobytes()


# (tensor, element, value): element 0 of the first tensor that has one; the last element of the
# 3 * 4096 + 5 tensor's ragged tail; a tensor of the third launch (tensors 128 and 129)
@pytest.mark.parametrize('which,where,value', [(1, 0, float('inf')), (8, 3 * 4096 + 4, float('nan')),
                                               (129, 2, float('-inf'))],
                         ids=['inf-first-element', 'nan-end-of-ragged-tail', 'neg-inf-third-launch'])
def test_stats_finds_a_non_finite_value(cuda, grads, which, where, value):
    ts = list(grads)
    assert ts[0].numel() == 0 and where < ts[which].numel()
    ts[which] = ts[which].clone()
    ts[which][where] = value
    found, _ = _stats(cuda, ts)
    assert found == 1.0


def test_stats_square_overflowing_f32_is_not_an_overflow(cuda, grads):
    ts = list(grads)
    ts[3] = torch.full((4,), 3e38, device=cuda)
    found, ss = _stats(cuda, ts)
    assert found == 0.0 and np.isfinite(ss) and ss > 4 * 8.9e76


def test_stats_unscale_in_place_is_exact(cuda, grads):
    ts = _tensors(cuda, 7)
    want = [t * 2.0 ** -16 for t in grads]
    scale = torch.full((), 2.0 ** 16, device=cuda)
    st = optim.GradStats(cuda)
    st.run(ts, scale=scale, unscale=True)
    assert float(st.found_inf.item()) == 0.0
    for i, (a, b) in enumerate(zip(ts, want)):
        assert torch.equal(a, b), i
    # the sum of squares is of the gradients as the call leaves them
    ref = sum(float((t.cpu().numpy().astype(np.float64) ** 2).sum()) for t in want)
    np.testing.assert_allclose(st.sumsq.item(), ref, rtol=1e-12)


# ------------------------------------------------------------------ Adam with the step on the device
def _params(cuda, seed=21):
    return [torch.nn.Parameter(t) for t in _tensors(cuda, seed)]


def _step_grads(cuda, it):
    return _tensors(cuda, 100 + it)


def _run(cuda, opt, params, steps=5, mul=1.0, before_step=None):
    for it in range(steps):
        for p, g in zip(params, _step_grads(cuda, it)):
            p.grad = g * mul
        if before_step is not None:
            before_step(it)
        opt.step()
    torch.cuda.synchronize()


def _state_of(opt, params):
    return [(p.detach().clone(), opt.state[p]['exp_avg'].clone(), opt.state[p]['exp_avg_sq'].clone(),
             opt.state[p]['step'].clone()) for p in params]


@pytest.fixture(scope='module', params=[0.0, 1e-2], ids=['wd0', 'wd1e-2'])
def host_stepped(request, cuda):
    """Five steps of the host-stepped posu.optim.Adam: the reference of the device-stepped runs."""
    wd = request.param
    params = _params(cuda)
    opt = optim.Adam(params, lr=1e-3, weight_decay=wd)
    _run(cuda, opt, params)
    return wd, _state_of(opt, params)


def test_adam_dev_is_bit_identical_to_the_host_stepped_kernel(cuda, host_stepped):
    """Same arithmetic, bias corrections from the same doubles (the device's pow against the
    host's: equal after the rounding to f32 on these five steps)."""
    wd, ref = host_stepped
    params = _params(cuda)
    opt = optim.Adam(params, lr=1e-3, weight_decay=wd, capturable=True)
    _run(cuda, opt, params)
    steps = {opt.state[p]['step'].untyped_storage().data_ptr() for p in params}
    assert len(steps) == 1   # the step counts are views of one buffer
    for i, (got, want) in enumerate(zip(_state_of(opt, params), ref)):
        for a, b, what in zip(got[:3], want[:3], ('param', 'exp_avg', 'exp_avg_sq')):
            assert torch.equal(a, b), (what, i, float((a - b).abs().max()))
        assert got[3].is_cuda and got[3].dtype == torch.float32 and float(got[3]) == 5.0 == float(want[3])
    sd = opt.state_dict()
    o2 = optim.Adam(params, lr=1e-3, weight_decay=wd, capturable=True)
    o2.load_state_dict(sd)
    st = o2.state[params[1]]['step']
    assert st.is_cuda and float(st) == 5.0


@pytest.mark.parametrize('k', [16, -3])
def test_adam_dev_power_of_two_grad_scale_is_exact(cuda, host_stepped, k):
    wd, ref = host_stepped
    params = _params(cuda)
    opt = optim.Adam(params, lr=1e-3, weight_decay=wd, capturable=True)
    opt.grad_scale = torch.full((), 2.0 ** k, device=cuda)
    opt.found_inf = torch.zeros((), device=cuda)
    _run(cuda, opt, params, mul=2.0 ** k)
    for i, (got, want) in enumerate(zip(_state_of(opt, params), ref)):
        for a, b in zip(got, want[:3] + (want[3].to(cuda),)):
            assert torch.equal(a, b), i


def test_adam_dev_found_inf_changes_nothing(cuda):
    params = _params(cuda)
    opt = optim.Adam(params, lr=1e-3, weight_decay=1e-2, capturable=True)
    _run(cuda, opt, params, steps=2)
    before = _state_of(opt, params)
    opt.found_inf = torch.ones((), device=cuda)
    opt.grad_scale = torch.full((), 4.0, device=cuda)
    for p, g in zip(params, _step_grads(cuda, 2)):
        p.grad = g
    opt.step()
    torch.cuda.synchronize()
    for i, (got, want) in enumerate(zip(_state_of(opt, params), before)):
        for a, b in zip(got, want):
            assert torch.equal(a, b), i
    assert float(opt.state[params[1]]['step']) == 2.0


@pytest.mark.parametrize('wd', [0.0, 1e-2])
def test_adam_dev_max_grad_norm_matches_clip_grad_norm(cuda, wd):
    """max_grad_norm inside the update = torch.nn.utils.clip_grad_norm_ before the plain step, within
    tests/test_optim.py's tolerances (one product g * (1 / scale * clip) against two roundings)."""
    max_norm = 5.0
    ref = _params(cuda)
    o_ref = optim.Adam(ref, lr=1e-3, weight_decay=wd)
    norms = []
    _run(cuda, o_ref, ref, before_step=lambda it: norms.append(
        float(torch.nn.utils.clip_grad_norm_(ref, max_norm))))
    assert min(norms) > 10 * max_norm   # the clip is active in every step
    ours = _params(cuda)
    o_ours = optim.Adam(ours, lr=1e-3, weight_decay=wd, capturable=True, max_grad_norm=max_norm)
    _run(cuda, o_ours, ours)
    for i, (a, b) in enumerate(zip(ref, ours)):
        torch.testing.assert_close(b, a, rtol=1e-5, atol=1e-7, msg=lambda m: 'param %d: %s' % (i, m))
        for key in ('exp_avg', 'exp_avg_sq'):
            r = o_ref.state[a][key]
            torch.testing.assert_close(o_ours.state[b][key], r, rtol=1e-5,
                                       atol=1e-6 * float(r.abs().max()) if r.numel() else 0.0,
                                       msg=lambda m: '%s %d: %s' % (key, i, m))


# ------------------------------------------------------------------ the scaler
def _small(cuda, n=10, seed=3):
    g = torch.Generator(device=cuda).manual_seed(seed)
    return [torch.nn.Parameter(torch.randn(5 + 300 * i, device=cuda, generator=g)) for i in range(n)]


def _small_grads(cuda, params, it, scale, bad=False):
    g = torch.Generator(device=cuda).manual_seed(50 + it)
    out = [torch.randn(p.shape, device=cuda, generator=g) * scale for p in params]
    if bad:
        out[4][7] = float('inf')
    return out


def test_scaler_dynamics(cuda):
    """growth_interval 2: clean, clean, inf, clean, clean -> S, 2S, S, S, 2S; the overflowed step
    changes nothing but the scale."""
    S = 2.0 ** 10
    params = _small(cuda)
    opt = optim.Adam(params, lr=1e-3, capturable=True)
    scaler = amp.LossScaler(init_scale=S, growth_interval=2)
    scales = []
    for it, bad in enumerate([False, False, True, False, False]):
        before = [p.detach().clone() for p in params]
        for p, g in zip(params, _small_grads(cuda, params, it, scaler.get_scale(), bad)):
            p.grad = g
        scaler.step(opt)
        assert scaler.found_inf() == bad
        scaler.update()
        scales.append(scaler.get_scale())
        same = all(torch.equal(a, p.detach()) for a, p in zip(before, params))
        assert same == bad
    assert scales == [S, 2 * S, S, S, 2 * S]
    assert float(opt.state[params[0]]['step']) == 4.0
    sd = scaler.state_dict()
    assert sd['scale'] == 2 * S and sd['_growth_tracker'] == 0
    other = amp.LossScaler()
    other.load_state_dict(sd)
    assert other.get_scale() == 2 * S
    # the scale does not grow to inf
    top = amp.LossScaler(init_scale=2.0 ** 127, growth_interval=1)
    for p, g in zip(params, _small_grads(cuda, params, 9, 1.0)):
        p.grad = g
    top.step(opt)
    top.update()
    assert top.get_scale() == 2.0 ** 127


def test_training_loop_calls_do_not_synchronise(cuda):
    params = _small(cuda)
    opt = optim.Adam(params, lr=1e-3, capturable=True, max_grad_norm=1.0)
    scaler = amp.LossScaler()
    x = torch.randn(params[0].shape, device=cuda)

    def iteration():
        loss = (params[0] * x).sum()
        scaled = scaler.scale(loss)
        for p, g in zip(params, _small_grads(cuda, params, 0, 1.0)):
            p.grad = g
        scaler.step(opt)
        scaler.update()
        opt.step()   # the capturable step on its own
        return scaled

    iteration()   # allocates the state
    torch.cuda.synchronize()
    saved = torch.cuda.get_sync_debug_mode()
    torch.cuda.set_sync_debug_mode('error')
    try:
        try:
            x.sum().item()
            detects = False
        except RuntimeError:
            detects = True
        if detects:
            iteration()
    finally:
        torch.cuda.set_sync_debug_mode(saved)
    if not detects:
        pytest.skip('this build does not raise on a synchronising .item() under set_sync_debug_mode')


def _three_steps(cuda, use_graph):
    params = _small(cuda)
    opt = optim.Adam(params, lr=1e-3, weight_decay=1e-2, capturable=True)
    scaler = amp.LossScaler(init_scale=256., growth_interval=2)
    static = [torch.zeros_like(p) for p in params]
    for p, s in zip(params, static):
        p.grad = s

    def feed(it, bad=False):
        for s, g in zip(static, _small_grads(cuda, params, it, 256., bad)):
            s.copy_(g)

    feed(0)
    scaler.step(opt)   # eager first step: allocates the state
    scaler.update()
    graph = None
    if use_graph:
        torch.cuda.synchronize()
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):   # one stream: a linear graph
            scaler.step(opt)
            scaler.update()
    for it, bad in ((1, False), (2, True), (3, False)):
        feed(it, bad)
        if graph is not None:
            graph.replay()
        else:
            scaler.step(opt)
            scaler.update()
    torch.cuda.synchronize()
    return ([p.detach().clone() for p in params] + [opt.state[p][k].clone() for p in params
                                                    for k in ('exp_avg', 'exp_avg_sq', 'step')],
            scaler.get_scale())


def test_step_and_update_replay_from_a_graph_bit_for_bit(cuda):
    eager, s_eager = _three_steps(cuda, False)
    replayed, s_graph = _three_steps(cuda, True)
    assert s_eager == s_graph == 256.   # grown after two clean steps, halved by the inf
    for i, (a, b) in enumerate(zip(eager, replayed)):
        assert torch.equal(a, b), i
    assert float(eager[-1]) == 3.0   # four steps, one skipped


def test_torch_grad_scaler_drives_the_capturable_adam(cuda):
    def run(scaler):
        params = _small(cuda)
        opt = optim.Adam(params, lr=1e-3, capturable=True)
        scaler.scale(torch.zeros((), device=cuda))   # torch's scaler makes its state here
        for it, bad in enumerate([False, True, False]):
            for p, g in zip(params, _small_grads(cuda, params, it, scaler.get_scale(), bad)):
                p.grad = g
            scaler.step(opt)
            scaler.update()
        torch.cuda.synchronize()
        return [p.detach().clone() for p in params], scaler.get_scale(), float(opt.state[params[0]]['step'])

    ours, s_ours, n_ours = run(amp.LossScaler())
    theirs, s_theirs, n_theirs = run(torch.amp.GradScaler('cuda'))
    assert s_ours == s_theirs == 2.0 ** 15 and n_ours == n_theirs == 2.0
    for i, (a, b) in enumerate(zip(ours, theirs)):
        assert torch.equal(a, b), i
