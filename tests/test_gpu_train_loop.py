"""core.function.train and the three device metrics behind it (csrc/train_metrics.hip):

* posu_pck_accuracy against the reference's accuracy (tests/golden/train_loop.npz) -- equal, not
  close: the counts are integers, each accuracy one f64 division, the average summed in the
  reference's order -- and against this build's core.evaluate.accuracy on random maps;
* posu_grad_row_norms against the reference's check_grad_norm (golden, f64) and against torch
  norms of the same gradients on real losses, to L * 2^-52 relative (f64 sums of L exact terms in
  another order);
* train() against a loop written here from the same public pieces with explicit .item() reads:
  same parameters, Adam moments, BatchNorm buffers and meters, and no device read or
  synchronisation between two log lines; the heatmap-MI alternation; fp16 through a LossScaler.
"""
import copy
from collections import OrderedDict

import numpy as np
import pytest
import torch
import torch.nn as nn

from posu import amp, ops, optim, synthetic as syn

pytestmark = pytest.mark.gpu

ACC_CASES = ('a', 'b', 'c', 'c24', 'd', 'd0', 'e3x5', 'e4x4', 'f')


# ------------------------------------------------------------------ accuracy
def _offset_view(t):
    """The same values in a tensor whose storage starts one float past a 16-byte boundary."""
    buf = torch.empty(t.numel() + 1, dtype=t.dtype, device=t.device)
    v = buf[1:].view(t.shape)
    v.copy_(t)
    assert v.data_ptr() % 16 == 4 and v.is_contiguous()
    return v


def _host(res):
    return [r.cpu().numpy() for r in res]


@pytest.mark.parametrize('name', ACC_CASES)
def test_pck_accuracy_equals_the_reference(cuda, golden, name):
    g = golden('train_loop.npz')
    out = torch.from_numpy(g['acc.%s.output' % name]).to(cuda)
    tgt = torch.from_numpy(g['acc.%s.target' % name]).to(cuda)
    thr = 0.5
    acc, avg, cnt, pred, step = _host(ops.pck_accuracy([out], [tgt], thr))
    print(name, 'acc', acc[0], 'ref', g['acc.%s.acc' % name], 'avg', avg[0], 'cnt', cnt[0])
    assert np.array_equal(acc[0], g['acc.%s.acc' % name])
    assert avg[0] == float(g['acc.%s.avg' % name]) and cnt[0] == int(g['acc.%s.cnt' % name])
    assert np.array_equal(pred[0], g['acc.%s.pred' % name])
    assert step[0] == avg[0] and step[1] == float(cnt[0])
    # views whose storage is offset by one float (the 4-byte loads) give the same results
    off = _host(ops.pck_accuracy([_offset_view(out)], [_offset_view(tgt)], thr))
    again = _host(ops.pck_accuracy([out], [tgt], thr))
    for a, b, c in zip((acc, avg, cnt, pred, step), off, again):
        assert a.tobytes() == b.tobytes() == c.tobytes()


def test_pck_accuracy_views_are_independent_rows(cuda, golden):
    """Three views in one call (two cases of one shape, one of them twice, one offset): every row is
    its own single-view result and step is np.mean over the rows."""
    g = golden('train_loop.npz')
    a = [torch.from_numpy(g['acc.a.%s' % k]).to(cuda) for k in ('output', 'target')]
    b = [a[0].flip(0).contiguous(), a[1].flip(0).contiguous()]
    outs, tgts = [a[0], b[0], _offset_view(a[0])], [a[1], b[1], a[1]]
    acc, avg, cnt, pred, step = _host(ops.pck_accuracy(outs, tgts))
    for v, (o, t) in enumerate(zip(outs, tgts)):
        acc1, avg1, cnt1, pred1, _ = _host(ops.pck_accuracy([o], [t]))
        assert np.array_equal(acc[v], acc1[0]) and avg[v] == avg1[0] and cnt[v] == cnt1[0]
        assert np.array_equal(pred[v], pred1[0])
    assert np.array_equal(acc[0], g['acc.a.acc']) and np.array_equal(acc[2], g['acc.a.acc'])
    assert step[0] == np.mean(list(avg)) and step[1] == np.mean(list(cnt))


def test_accuracy_device_equals_accuracy_view_by_view(cuda):
    from core.evaluate import accuracy, accuracy_device
    gen = torch.Generator().manual_seed(77)
    outs = [torch.rand(4, 16, 64, 64, generator=gen) for _ in range(4)]
    # the largest of 4096 uniform values lie about 2.4e-4 apart: noise a few times that moves about
    # half of the targets' maxima somewhere else (a miss) and leaves the others in place (a hit)
    tgts = [o + 1e-3 * torch.rand(o.shape, generator=gen) for o in outs]
    outs, tgts = [o.to(cuda) for o in outs], [t.to(cuda) for t in tgts]
    acc, avg, cnt, pred, step = accuracy_device(outs, tgts)
    assert acc.is_cuda and acc.dtype == torch.float64 and cnt.dtype == torch.int32 and pred.dtype == torch.float32
    acc, avg, cnt, pred, step = _host((acc, avg, cnt, pred, step))
    ref_avg, ref_cnt = [], []
    for v in range(4):
        a, m, c, p = accuracy(outs[v], tgts[v])
        assert np.array_equal(acc[v], a) and avg[v] == m and cnt[v] == c
        assert np.array_equal(pred[v], p)      # accuracy returns its predictions on the host
        ref_avg.append(m)
        ref_cnt.append(c)
    print('accuracy_device: avg per view %s, cnt %s' % (avg, cnt))
    assert 0.1 < min(ref_avg) and max(ref_avg) < 0.9      # hits and misses are both there
    assert step[0] == np.mean(ref_avg) and step[1] == np.mean(ref_cnt)


@pytest.mark.parametrize('thr', [0.3, 1.3])
def test_accuracy_device_applies_its_threshold(cuda, golden, thr):
    """At 8 x 24 the normalised distances of a one-px offset are 1 / 2.4 = 0.42 (y), 1 / 0.8 = 1.25 (x) and
    1.32 (both): thr 0.3 keeps only the exact hits, thr 1.3 adds both single offsets.  Against this build's
    accuracy(), which applies thr too (the reference's ignores it)."""
    from core.evaluate import accuracy, accuracy_device
    g = golden('train_loop.npz')
    out = torch.from_numpy(g['acc.c24.output']).to(cuda)
    tgt = torch.from_numpy(g['acc.c24.target']).to(cuda)
    acc, avg, cnt, _, _ = _host(accuracy_device([out], [tgt], thr=thr))
    a, m, c, _ = accuracy(out, tgt, thr=thr)
    print('thr %g: acc %s (thr 0.5: %s)' % (thr, acc[0], g['acc.c24.acc']))
    assert np.array_equal(acc[0], a) and avg[0] == m and cnt[0] == c
    at_half = g['acc.c24.acc'][1:]
    assert np.all(acc[0][1:] <= at_half) if thr < 0.5 else np.all(acc[0][1:] >= at_half)
    assert not np.array_equal(acc[0][1:], at_half)


# ------------------------------------------------------------------ the consistent loss's criterion
@pytest.mark.parametrize('shape', [(3, 5, 8, 8), (2, 16, 16, 16), (2, 3, 5, 7)])
def test_mse_mean_matches_torch_mse_loss_in_value_and_both_gradients(cuda, shape):
    """ops.mse_mean / core.loss.MeanMSELoss against torch.nn.functional.mse_loss evaluated in f64 on the
    same f32 values.  Bounds from the f32 operations: the value is a sum of n = numel f32 terms (n 2^-24
    relative at worst); a gradient element 2 g (a - b) / n goes through one f32 subtraction, the scale's
    two divisions and two products: 8 x 2^-24 relative per element, no absolute term."""
    import torch.nn.functional as F
    from core.loss import MeanMSELoss
    gen = torch.Generator().manual_seed(31)
    a0, b0 = torch.randn(shape, generator=gen), torch.randn(shape, generator=gen)
    n = a0.numel()

    def reference(grad_a, grad_b):
        a = a0.double().requires_grad_(grad_a)
        b = b0.double().requires_grad_(grad_b)
        loss = F.mse_loss(a, b)
        (loss * 0.7).backward()
        return loss.item(), a.grad, b.grad

    for grad_a, grad_b in ((True, True), (True, False), (False, True)):
        a = a0.to(cuda).requires_grad_(grad_a)
        b = b0.to(cuda).requires_grad_(grad_b)
        loss = MeanMSELoss()(a, b)
        assert loss.dim() == 0 and loss.dtype == torch.float32
        (loss * 0.7).backward()
        ref, ga, gb = reference(grad_a, grad_b)
        assert abs(loss.item() - ref) <= n * 2.0 ** -24 * abs(ref)
        for got, want, needed in ((a.grad, ga, grad_a), (b.grad, gb, grad_b)):
            if not needed:
                assert got is None
                continue
            err = (got.double().cpu() - want).abs()
            worst = float((err / want.abs().clamp_min(1e-300)).max())
            print('%s grads (%s, %s): value rel %.3g, gradient rel max %.3g' % (shape, grad_a, grad_b,
                                                                               abs(loss.item() - ref) / abs(ref), worst))
            assert bool((err <= 8 * 2.0 ** -24 * want.abs()).all())
    # d/db = -d/da exactly
    a, b = a0.to(cuda).requires_grad_(True), b0.to(cuda).requires_grad_(True)
    ops.mse_mean(a, b).backward()
    assert torch.equal(a.grad, -b.grad) and float(a.grad.abs().max()) > 0


# ------------------------------------------------------------------ gradient norms
def _assert_rel(got, ref, length, what):
    bound = length * 2.0 ** -52
    rel = abs(got - ref) / abs(ref)
    print('%s: got %.17g ref %.17g rel %.3g (bound %.3g)' % (what, got, ref, rel, bound))
    assert rel <= bound, what


@pytest.mark.parametrize('p', [1, 2])
def test_grad_row_norms_match_the_reference(cuda, golden, p):
    g = golden('train_loop.npz')
    grads = g['gn.grads'].astype(np.float32)
    assert np.array_equal(grads.astype(np.float64), g['gn.grads'])
    length = grads.shape[2]
    for k, name in enumerate(g['gn.losses']):
        views = [None if g['gn.unused'][k, v] else torch.from_numpy(grads[v]).to(cuda).view(3, 2, 4, 4)
                 for v in range(4)]
        got = ops.grad_row_norms(views, p)
        assert got.dtype == torch.float64 and got.dim() == 0
        again = ops.grad_row_norms(views, p)
        assert got.cpu().numpy().tobytes() == again.cpu().numpy().tobytes()
        ref = float(g['gn.p%d' % p][k])
        if np.isnan(ref):
            assert np.isnan(got.item()), name
        else:
            _assert_rel(got.item(), ref, length, '%s p=%d' % (name, p))
    with pytest.raises(ValueError):
        ops.grad_row_norms([None, None], p)


def _real_losses(cuda, seed=5):
    """Weighted MSE and FundamentalLoss on 4 views of [2, 16, 16, 16] heatmaps (leaves)."""
    from core.loss import FundamentalLoss
    from utils.transforms import generate_integral_preds_2d_th, transform_back_th
    cfg = syn.train_loop_cfg(image_size=64)
    (_, target, weight, meta), = syn.train_loop_batches(1, image_size=64, seed=seed)
    gen = torch.Generator().manual_seed(seed)
    x = [(t + 0.1 * torch.randn(t.shape, generator=gen)).to(cuda).requires_grad_(True) for t in target]
    target, weight = [t.to(cuda) for t in target], [w.to(cuda) for w in weight]
    mse = sum(ops.joints_mse(a, t, w) for a, t, w in zip(x, target, weight))
    fl = FundamentalLoss(cfg, fundamental_matrix_dict=syn.fundamental_dict(), device=cuda)
    joints = transform_back_th(cfg, [generate_integral_preds_2d_th(a) for a in x], meta)
    fund = fl(joints, weight, meta) * cfg.LOSS.FUNDAMENTAL_LOSS_WEIGHT
    return x, OrderedDict([('mse', mse), ('fund', fund)])


@pytest.mark.parametrize('p', [1, 2])
def test_check_grad_norm_on_real_losses(cuda, p):
    from utils.gradients import check_grad_norm
    x, losses = _real_losses(cuda)
    res = check_grad_norm(losses, x, norm=p)
    assert list(res) == ['mse', 'fund']
    for name, loss in losses.items():
        grads = torch.autograd.grad(loss, x, retain_graph=True)
        ref = 0.0
        for gr in grads:
            rn = gr.double().view(gr.shape[0], -1).norm(p=p, dim=1)
            ref = ref + (rn.sum() / rn.ne(0).double().sum()).item()
        _assert_rel(res[name].item(), ref, x[0][0].numel(), '%s p=%d' % (name, p))
    # the watch leaves the graph as it was: .grad after it equals .grad without it
    sum(losses.values()).backward()
    x2, losses2 = _real_losses(cuda)
    sum(losses2.values()).backward()
    for a, b in zip(x, x2):
        assert torch.equal(a.grad, b.grad)


def test_check_grad_norm_reports_views_without_a_gradient(cuda, capsys):
    from utils.gradients import check_grad_norm
    x = [torch.rand(2, 3, 4, 4, device=cuda).requires_grad_(True) for _ in range(3)]
    res = check_grad_norm({'two': (x[0] ** 2).sum() + (x[2] ** 2).sum()}, x, norm=2)
    assert 'grad of two (view 1) is None' in capsys.readouterr().out
    ref = sum(float((2 * x[v].detach().double()).view(2, -1).norm(dim=1).mean()) for v in (0, 2))
    _assert_rel(res['two'].item(), ref, 48, 'two views of three')
    free = torch.rand(2, 3, device=cuda).requires_grad_(True)
    with pytest.raises(ValueError, match='nothing'):
        check_grad_norm({'nothing': (free ** 2).sum()}, x)


def test_meters_update_is_the_average_meter(cuda):
    from core.function import AverageMeter
    r = np.random.default_rng(4)
    table = torch.zeros((5, 3), dtype=torch.float64, device=cuda)
    host = [AverageMeter() for _ in range(5)]
    for step in range(7):
        v, w = r.standard_normal(5).astype(np.float32).astype(np.float64), r.integers(1, 9, 5).astype(np.float64)
        active = [1, step % 2, 1, 0, step != 3]
        ops.meters_update(table, torch.from_numpy(v).to(cuda), torch.from_numpy(w).to(cuda), active)
        for m in range(5):
            if active[m]:
                host[m].update(float(v[m]), float(w[m]))
    got = table.cpu().numpy()
    for m in range(5):
        assert (got[m, 0], got[m, 1], got[m, 2]) == (host[m].val, host[m].sum, host[m].count), m


# ------------------------------------------------------------------ the loop
class _ReadCounters:
    """Counts device reads and synchronisations while armed (calls on cuda tensors / streams / events)."""
    # besides the explicit reads, the conversions that read one element (bool / float / int / index of a
    # cuda tensor) and what a boolean-mask selection is made of (nonzero, masked_select, x[mask])
    TENSOR = ('item', 'cpu', 'numpy', 'tolist', '__bool__', '__float__', '__int__', '__index__', 'nonzero',
              'masked_select')

    def __init__(self, monkeypatch):
        self.armed = False
        self.calls = []
        for name in self.TENSOR:
            monkeypatch.setattr(torch.Tensor, name, self._wrap(getattr(torch.Tensor, name), name, tensor=True))
        for name in ('nonzero', 'masked_select'):
            monkeypatch.setattr(torch, name, self._wrap(getattr(torch, name), 'torch.' + name, tensor=True))
        getitem = torch.Tensor.__getitem__

        def counted_getitem(t, index):
            if self.armed and t.is_cuda:
                for k in (index if isinstance(index, tuple) else (index,)):
                    if isinstance(k, torch.Tensor) and k.dtype in (torch.bool, torch.uint8):
                        self.calls.append('__getitem__[mask]')
            return getitem(t, index)
        monkeypatch.setattr(torch.Tensor, '__getitem__', counted_getitem)
        monkeypatch.setattr(torch.cuda, 'synchronize', self._wrap(torch.cuda.synchronize, 'cuda.synchronize'))
        for cls in (torch.cuda.Stream, torch.cuda.Event):
            monkeypatch.setattr(cls, 'synchronize', self._wrap(cls.synchronize, cls.__name__ + '.synchronize'))

    def _wrap(self, fn, name, tensor=False):
        def counted(*args, **kwargs):
            if self.armed and (not tensor or (args and getattr(args[0], 'is_cuda', False))):
                self.calls.append(name)
            return fn(*args, **kwargs)
        return counted


def test_the_counters_see_hidden_reads(cuda, monkeypatch):
    """The control for the zero-reads assertions below: each kind of read is counted, host tensors and
    index_select are not."""
    counters = _ReadCounters(monkeypatch)
    x = torch.arange(6., device=cuda).view(3, 2)
    mask = torch.tensor([True, False, True], device=cuda)
    counters.armed = True
    x[mask], x[:, 0][mask], bool(x[0, 0] > 1), float(x[0, 1]), int(x[1, 0]), x.sum().item(), x.nonzero()
    torch.nonzero(x), x.cpu(), x.tolist(), torch.cuda.synchronize()
    seen = list(counters.calls)
    counters.calls.clear()
    x.index_select(0, torch.tensor([0, 2], device=cuda)), x[0], x[:, 1], x.cpu  # no read
    torch.ones(3).numpy(), bool(torch.ones(1)), torch.ones(3)[torch.tensor([True, False, True])]   # host tensors
    counters.armed = False
    for name in ('__getitem__[mask]', '__bool__', '__float__', '__int__', 'item', 'nonzero', 'torch.nonzero', 'cpu',
                 'tolist', 'cuda.synchronize'):
        assert name in seen, (name, seen)
    assert seen.count('__getitem__[mask]') == 2
    assert counters.calls == []


class _Data:
    """A loader over prepared batches that arms the counters when it hands out batch 1 and disarms
    them when it is exhausted (before train() reads its final meters)."""

    def __init__(self, batches, counters):
        self.batches, self.counters = batches, counters

    def __len__(self):
        return len(self.batches)

    def __iter__(self):
        for k, b in enumerate(self.batches):
            if k == 1:
                self.counters.armed = True
            yield b
        self.counters.armed = False


def _r18(cuda, cfg, state=None, precision='fp32', scaler=None, init='he'):
    from models.multiview_pose_resnet import get_multiview_pose_net
    from models.pose_resnet import get_pose_net
    net = get_pose_net(cfg, is_train=False, precision=precision, loss_scaler=scaler)
    make = syn.synthetic_state_dict if init == 'he' else syn.reference_init_state_dict
    net.load_state_dict(make(net.state_dict(), seed=7))
    model = get_multiview_pose_net(net, cfg).to(cuda)
    if state is not None:
        model.load_state_dict(state)
    return model


def _snapshot(model, opt):
    params = [p.detach().clone() for p in model.parameters()]
    moments = [(opt.state[p]['exp_avg'].clone(), opt.state[p]['exp_avg_sq'].clone()) for p in model.parameters()]
    return params, moments, [b.detach().clone() for b in model.buffers()]


def _hand_loop(cuda, cfg, batches, model, opt, fl, cons_crit):
    """The reference's step (function.py:148-469) for MSE + consistent + fundamental + watch, from the
    public pieces, the way a user writes it today: boolean-mask selection, .item() per scalar, host
    accuracy per view."""
    from core.evaluate import accuracy
    from core.function import AverageMeter, fuse_routing, select_out_h36m, select_out_h36m_meta
    from core.loss import JointsMSELoss
    from utils.gradients import check_grad_norm
    from utils.transforms import generate_integral_preds_2d_th, transform_back_th
    L = cfg.LOSS
    crit = JointsMSELoss(use_target_weight=True)
    aggre = bool(cfg.NETWORK.AGGRE)
    meters = {k: AverageMeter() for k in ('loss', 'mse', 'acc', 'consistent', 'fund', 'mse_grad', 'fund_grad')}
    model.train()
    for input, target, weight, meta in batches:
        input = [v.to(cuda) for v in input]
        n = len(input) * input[0].size(0)
        raw, agg, _, _ = model(input)
        output = fuse_routing(raw, agg, aggre, meta) if aggre and cfg.TEST.FUSE_OUTPUT else raw
        target_cuda, weight_cuda = [t.to(cuda) for t in target], [w.to(cuda) for w in weight]
        loss, mse_loss = 0, 0
        for t, w, r in zip(target_cuda, weight_cuda, raw):
            mse_loss = mse_loss + crit(r, t, w) * L.MSE_LOSS_WEIGHT
        loss = loss + mse_loss
        if aggre:
            for t, w, o in zip(target_cuda, weight_cuda, output):
                mse_loss = mse_loss + crit(o, t, w) * L.MSE_LOSS_WEIGHT
            loss = loss + mse_loss
        consistent_loss, fund_loss = 0, 0
        s_raw, _ = select_out_h36m(raw, raw, meta)
        assert len(s_raw[0]) != 0
        s_weight, s_output = select_out_h36m(weight_cuda, output, meta)
        s_meta = select_out_h36m_meta(meta, ['center', 'scale', 'subject'])
        if aggre and L.USE_CONSISTENT_LOSS:
            s_agg, _ = select_out_h36m(agg, agg, meta)
            cal_loss = cons_crit(torch.cat(s_raw, dim=0), torch.cat(s_agg, dim=0))
            loss = loss + cal_loss * L.CONSISTENT_LOSS_WEIGHT
            consistent_loss = cal_loss.item() * L.CONSISTENT_LOSS_WEIGHT
        joints = transform_back_th(cfg, [generate_integral_preds_2d_th(o) for o in s_output], s_meta)
        fund_loss = fl(joints, s_weight, s_meta) * L.FUNDAMENTAL_LOSS_WEIGHT
        loss = loss + fund_loss
        grad_dict = check_grad_norm(OrderedDict([('mse', mse_loss), ('fund', fund_loss)]), raw, norm=1)
        opt.zero_grad()
        loss.backward()
        opt.step()
        meters['loss'].update(loss.item(), n)
        meters['mse'].update(mse_loss.item(), n)
        if L.USE_CONSISTENT_LOSS:
            meters['consistent'].update(consistent_loss, n)
        meters['fund'].update(fund_loss.item(), 1)
        meters['mse_grad'].update(grad_dict['mse'].item(), 1)
        meters['fund_grad'].update(grad_dict['fund'].item(), 1)
        accs, cnts = [], []
        for o, t in zip(output, target_cuda):
            _, a, c, _ = accuracy(o.detach().cpu().numpy(), t.detach().cpu().numpy())
            accs.append(a)
            cnts.append(c)
        meters['acc'].update(np.mean(accs), np.mean(cnts))
    return meters


@pytest.fixture(params=['raw', 'aggre'])
def loop_run(request, cuda, monkeypatch):
    """train() and the hand-written loop from the same state on the same 3 batches (R18 at 64 x 64,
    fp32, 4 views x 2, the second sample of every batch from 'mpii')."""
    from core.function import train
    from core.loss import FundamentalLoss, JointsMSELoss
    aggre = request.param == 'aggre'
    cfg = syn.train_loop_cfg(num_layers=18, image_size=64, aggre=aggre, fuse_output=aggre, consistent=aggre,
                             fundamental=True, watch_grad_norm=True, print_freq=100)
    batches = syn.train_loop_batches(3, nviews=4, batch=2, image_size=64, seed=11, sources=['h36m', 'mpii'])
    fl = FundamentalLoss(cfg, fundamental_matrix_dict=syn.fundamental_dict(), device=cuda)
    torch.manual_seed(3)   # the Aggregation weights are drawn from torch's generator
    hand_model = _r18(cuda, cfg)
    state = copy.deepcopy(hand_model.state_dict())
    hand_opt = optim.Adam(hand_model.parameters(), lr=1e-3)
    cons_crit = torch.nn.MSELoss(reduction='mean')   # the reference's criterion_dict['mse'] (its own torch form)
    hand_meters = _hand_loop(cuda, cfg, batches, hand_model, hand_opt, fl, cons_crit)

    model = _r18(cuda, cfg, state=state)
    opt = optim.Adam(model.parameters(), lr=1e-3)
    counters = _ReadCounters(monkeypatch)
    final = train(cfg, _Data(batches, counters), {'base_model': model},
                  {'mse_weights': JointsMSELoss(use_target_weight=True), 'fundamental': fl, 'mse': cons_crit},
                  {'base_model': opt},
                  1, '', None, 0)
    torch.cuda.synchronize()
    return {'hand': _snapshot(hand_model, hand_opt), 'hand_meters': hand_meters, 'train': _snapshot(model, opt),
            'final': final, 'calls': list(counters.calls), 'consistent': aggre}


def test_train_equals_the_hand_written_loop_and_reads_nothing_between_log_lines(loop_run):
    (hp, hm, hb), (tp, tm, tb) = loop_run['hand'], loop_run['train']
    assert len(hp) == len(tp) > 60 and len(hb) == len(tb) > 0
    for k, (a, b) in enumerate(zip(hp, tp)):
        assert torch.equal(a, b), 'parameter %d' % k
    for k, ((a1, a2), (b1, b2)) in enumerate(zip(hm, tm)):
        assert torch.equal(a1, b1) and torch.equal(a2, b2), 'Adam moments %d' % k
    for k, (a, b) in enumerate(zip(hb, tb)):
        assert torch.equal(a, b), 'buffer %d' % k
    final = loop_run['final']
    names = ['loss', 'mse', 'acc', 'fund', 'mse_grad', 'fund_grad'] + (['consistent'] if loop_run['consistent'] else [])
    for name in names:
        ref, got = loop_run['hand_meters'][name], final[name]
        print('%-10s val %.9g avg %.9g count %g' % (name, got['val'], got['avg'], got['count']))
        assert (got['val'], got['avg'], got['count']) == (float(ref.val), float(ref.avg), float(ref.count)), name
    assert final['loss']['count'] == 3 * 8 and final['fund']['count'] == 3
    assert final['hmi_g']['count'] == 0 and final['hmi_d']['count'] == 0
    # batches 1 and 2 (i % PRINT_FREQ != 0): no .item / .cpu / .numpy / .tolist on a cuda tensor, no
    # device, stream or event synchronisation
    assert loop_run['calls'] == []


# ------------------------------------------------------------------ heatmap-MI alternation
class _Stub(nn.Module):
    """A base model that returns its parameters: 4 views of heatmaps [N, 16, 64, 64] and low-level
    features [N, 32, 64, 64]."""

    def __init__(self, n):
        super().__init__()
        gen = torch.Generator().manual_seed(21)
        self.hm = nn.Parameter(0.1 * torch.randn(4, n, 16, 64, 64, generator=gen))
        self.low = nn.Parameter(torch.randn(4, n, 32, 64, 64, generator=gen))

    def forward(self, views):
        hm = [self.hm[v] * 1.0 for v in range(4)]
        low = [self.low[v] * 1.0 for v in range(4)]
        return hm, [], low, low


def _stub_run(cuda, epoch, heatmap_mi):
    from core.function import train
    from core.loss import HeatmapMILoss, JointsMSELoss
    from models.discriminator import HeatmapDiscriminator
    cfg = syn.train_loop_cfg(image_size=256, fundamental=False, watch_grad_norm=False, heatmap_mi=heatmap_mi,
                             sigma=0, mi_channels=32, mi_inter_channels=32)
    batches = syn.train_loop_batches(2, nviews=4, batch=2, image_size=256, seed=5, target_sigma=2.0)
    stub = _Stub(2).to(cuda)
    torch.manual_seed(9)
    disc = HeatmapDiscriminator(cfg).to(cuda)
    before = copy.deepcopy(disc.state_dict())
    opts = {'base_model': optim.Adam(stub.parameters(), lr=1e-2),
            'heatmap_discriminator': optim.Adam(disc.parameters(), lr=1e-2)}
    crits = {'mse_weights': JointsMSELoss(use_target_weight=True),
             'heatmap_mi': HeatmapMILoss(cfg, {'heatmap_discriminator': disc})}
    final = train(cfg, batches, {'base_model': stub, 'heatmap_discriminator': disc}, crits, opts, epoch, '', None, 0)
    torch.cuda.synchronize()
    return stub, disc, before, opts, final


def test_heatmap_mi_alternates_between_discriminator_and_generator(cuda):
    plain, _, _, _, _ = _stub_run(cuda, 0, heatmap_mi=False)
    # even epoch: a discriminator step on detached inputs
    stub, disc, before, opts, final = _stub_run(cuda, 0, heatmap_mi=True)
    after = disc.state_dict()
    changed = [k for k in before if k.endswith('weight') and not torch.equal(before[k], after[k])]
    assert len(changed) == 5, changed     # three Linear and two BatchNorm weights
    for bn in ('1', '4'):
        key = 'block_nonlinear.%s.num_batches_tracked' % bn
        assert int(after[key]) - int(before[key]) == 4 * 2      # 4 views per step, 2 steps
    assert torch.equal(stub.hm, plain.hm) and torch.equal(stub.low, plain.low)   # the MSE-only update
    assert final['hmi_d']['count'] == 2 and final['hmi_g']['count'] == 0 and np.isfinite(final['hmi_d']['avg'])
    # odd epoch: the weighted generator term; the discriminator's parameters and optimiser untouched
    stub, disc, before, opts, final = _stub_run(cuda, 1, heatmap_mi=True)
    after = disc.state_dict()
    for k in before:
        if not k.endswith('num_batches_tracked') and 'running' not in k:
            assert torch.equal(before[k], after[k]), k
    assert len(opts['heatmap_discriminator'].state) == 0
    assert not torch.equal(stub.hm, plain.hm) and not torch.equal(stub.low, plain.low)
    assert final['hmi_g']['count'] == 2 and final['hmi_d']['count'] == 0 and np.isfinite(final['hmi_g']['avg'])


# ------------------------------------------------------------------ fp16 through the loss scaler
def test_fp16_train_equals_the_three_line_amp_loop(cuda, monkeypatch):
    from core.function import train
    from core.loss import JointsMSELoss
    cfg = syn.train_loop_cfg(num_layers=18, image_size=64, fundamental=False, watch_grad_norm=False)
    batches = syn.train_loop_batches(2, nviews=4, batch=2, image_size=64, seed=13)
    crit = JointsMSELoss(use_target_weight=True)

    hand_scaler = amp.LossScaler()
    hand = _r18(cuda, cfg, precision='fp16', scaler=hand_scaler, init='reference')
    state = copy.deepcopy(hand.state_dict())
    hand_opt = optim.Adam(hand.parameters(), lr=1e-3, capturable=True)
    hand.train()
    for input, target, weight, _ in batches:
        raw, _, _, _ = hand([v.to(cuda) for v in input])
        loss = 0
        for t, w, r in zip(target, weight, raw):
            loss = loss + crit(r, t.to(cuda), w.to(cuda)) * cfg.LOSS.MSE_LOSS_WEIGHT
        hand_opt.zero_grad()
        hand_scaler.scale(loss).backward()
        hand_scaler.step(hand_opt)
        hand_scaler.update()

    scaler = amp.LossScaler()
    model = _r18(cuda, cfg, state=state, precision='fp16', scaler=scaler, init='reference')
    opt = optim.Adam(model.parameters(), lr=1e-3, capturable=True)
    initial = [p.detach().clone() for p in model.parameters()]
    counters = _ReadCounters(monkeypatch)
    final = train(cfg, _Data(batches, counters), {'base_model': model}, {'mse_weights': crit}, {'base_model': opt},
                  0, '', None, 0)
    torch.cuda.synchronize()
    assert counters.calls == []
    (hp, hm, hb), (tp, tm, tb) = _snapshot(hand, hand_opt), _snapshot(model, opt)
    assert any(not torch.equal(a, b) for a, b in zip(tp, initial))     # the steps were applied
    for k, (a, b) in enumerate(zip(hp, tp)):
        assert torch.equal(a, b), 'parameter %d' % k
    for k, ((a1, a2), (b1, b2)) in enumerate(zip(hm, tm)):
        assert torch.equal(a1, b1) and torch.equal(a2, b2), 'Adam moments %d' % k
    for k, (a, b) in enumerate(zip(hb, tb)):
        assert torch.equal(a, b), 'buffer %d' % k
    assert scaler.state_dict()['_growth_tracker'] == 2 and scaler.get_scale() == hand_scaler.get_scale()
    assert final['loss']['count'] == 2 * 8 and np.isfinite(final['loss']['avg'])
