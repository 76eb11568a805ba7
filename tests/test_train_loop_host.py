"""core.function.train and its device metrics, what can be checked without a GPU: the entry points
exist and are declared and bound, the losses this build lacks are refused before the first batch,
CPU tensors are refused, and the host helpers compute what the reference's do."""
import os
import re

import numpy as np
import pytest
import torch

from posu import _native, ops, synthetic as syn

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRY_POINTS = ('posu_pck_accuracy', 'posu_grad_row_norms', 'posu_meters_update')
UNBUILT = ('USE_GLOBAL_MI_LOSS', 'USE_LOCAL_MI_LOSS', 'USE_DOMAIN_TRANSFER_LOSS', 'USE_VIEW_MI_LOSS',
           'USE_JOINTS_MI_LOSS')


def test_the_training_loop_entry_points_import():
    from core.evaluate import accuracy_device
    from core.function import AverageMeter, percent_of_datasource, select_out_h36m_meta, train
    from core.loss import MeanMSELoss
    from utils.gradients import check_grad_norm
    assert all(callable(f) for f in (train, accuracy_device, check_grad_norm, AverageMeter, percent_of_datasource,
                                     select_out_h36m_meta, MeanMSELoss))


def test_new_symbols_are_declared_and_bound():
    src = open(os.path.join(REPO, 'include', 'posu.h')).read()
    src = re.sub(r'/\*.*?\*/', '', src, flags=re.S)
    lib = _native.load()
    for name in ENTRY_POINTS + ('posu_pck_accuracy_workspace', 'posu_grad_row_norms_workspace'):
        assert re.search(r'\b%s\s*\(' % name, src), name
        assert name in _native.exported_symbols() and hasattr(lib, name), name
    assert lib.posu_abi_version() == _native.ABI_VERSION == 16
    # the workspace queries answer on the host: V outside 1..8 and empty shapes are refused
    assert lib.posu_pck_accuracy_workspace(4, 2, 16) == 4 * 2 * 16 * 4
    assert lib.posu_pck_accuracy_workspace(9, 2, 16) == -1 and lib.posu_pck_accuracy_workspace(0, 2, 16) == -1
    assert lib.posu_grad_row_norms_workspace(4, 3) == 4 * 3 * 8
    assert lib.posu_grad_row_norms_workspace(9, 3) == -1 and lib.posu_grad_row_norms_workspace(4, 0) == -1
    # argument errors come back before any launch
    assert lib.posu_pck_accuracy(None, None, 4, 2, 16, 8, 8, 0.5, None, None, None, None, None, None, 0, None) == 1
    assert 'null pointer' in _native.last_error()
    assert lib.posu_grad_row_norms(None, 4, 3, 32, 1, None, None, 0, None) == 1
    assert lib.posu_meters_update(None, 3, None, None, None, None) == 1


class _Untouchable:
    """A data source that fails the test when train() looks at it."""

    def __iter__(self):
        pytest.fail('train() advanced its data iterator before refusing the configuration')

    def __len__(self):
        pytest.fail('train() asked for the length of its data before refusing the configuration')


@pytest.mark.parametrize('flag', UNBUILT)
def test_unbuilt_losses_are_refused_before_the_first_batch(flag):
    from core.function import train
    cfg = syn.train_loop_cfg()
    setattr(cfg.LOSS, flag, True)
    with pytest.raises(NotImplementedError, match=flag):
        train(cfg, _Untouchable(), {}, {}, {}, 0, '', None, 0)


def test_absent_loss_flags_read_as_off():
    """A config without the flags at all gets past the refusal (and then fails on the empty dicts)."""
    from core.function import train
    cfg = syn.train_loop_cfg()
    for flag in UNBUILT:
        delattr(cfg.LOSS, flag)
    with pytest.raises(KeyError):
        train(cfg, _Untouchable(), {}, {}, {}, 0, '', None, 0)


def test_cpu_tensors_are_refused():
    from core.evaluate import accuracy_device
    from utils.gradients import check_grad_norm
    hm = [torch.rand(1, 2, 4, 4) for _ in range(2)]
    with pytest.raises(RuntimeError, match='cuda'):
        accuracy_device(hm, hm)
    with pytest.raises(RuntimeError, match='cuda'):
        ops.pck_accuracy(hm, hm)
    with pytest.raises(RuntimeError, match='cuda'):
        ops.grad_row_norms([torch.rand(2, 8), None])
    with pytest.raises(RuntimeError, match='cuda'):
        ops.mse_mean(torch.rand(2, 3, 4, 4), torch.rand(2, 3, 4, 4))
    with pytest.raises(RuntimeError, match='cuda'):
        ops.meters_update(torch.zeros(2, 3, dtype=torch.float64), torch.zeros(2, dtype=torch.float64),
                          torch.ones(2, dtype=torch.float64), [1, 1])
    x = torch.rand(2, 8, requires_grad=True)
    with pytest.raises(RuntimeError, match='cuda'):
        check_grad_norm({'sq': (x ** 2).sum()}, [x])


def test_percent_of_datasource():
    from core.function import percent_of_datasource
    meta = [{'source': ['h36m', 'h36m', 'mpii', 'h36m']}, {'source': ['mpii'] * 4}]
    assert percent_of_datasource(meta) == 'h36m 75.0%\tmpii 25.0%\t'


def test_select_out_h36m_meta():
    from core.function import select_out_h36m_meta
    meta = [{'source': ['h36m', 'mpii', 'h36m'], 'center': torch.arange(6.).reshape(3, 2) + 10 * v,
             'scale': np.arange(6.).reshape(3, 2) - v, 'subject': torch.tensor([9, 0, 11]), 'other': None}
            for v in range(4)]
    out = select_out_h36m_meta(meta, ['center', 'scale', 'subject'])
    assert len(out) == 4
    for v, m in enumerate(out):
        assert sorted(m) == ['center', 'scale', 'subject']
        assert torch.equal(m['center'], meta[v]['center'][[0, 2]])
        assert np.array_equal(m['scale'], meta[v]['scale'][[0, 2]])
        assert m['subject'].tolist() == [9, 11]
    assert select_out_h36m_meta([{'source': ['mpii', 'mpii'], 'center': torch.zeros(2, 2)}] * 4, ['center']) == []


def test_average_meter_arithmetic():
    from core.function import AverageMeter
    m = AverageMeter()
    assert (m.val, m.avg, m.sum, m.count) == (0, 0, 0, 0)
    m.update(0.5, 8)
    m.update(0.25, 4)
    assert m.val == 0.25 and m.sum == 0.5 * 8 + 0.25 * 4 and m.count == 12 and m.avg == 5.0 / 12
    m.update(3.0)
    assert m.val == 3.0 and m.count == 13 and m.avg == 8.0 / 13
    m.reset()
    assert (m.val, m.avg, m.sum, m.count) == (0, 0, 0, 0)


def test_train_loop_batches_are_seeded_and_shaped_like_the_loader():
    a = syn.train_loop_batches(2, nviews=4, batch=2, image_size=64, seed=3, sources=['h36m', 'mpii'])
    b = syn.train_loop_batches(2, nviews=4, batch=2, image_size=64, seed=3, sources=['h36m', 'mpii'])
    assert len(a) == 2
    for (ia, ta, wa, ma), (ib, tb, wb, mb) in zip(a, b):
        assert len(ia) == len(ta) == len(wa) == len(ma) == 4
        assert ia[0].shape == (2, 3, 64, 64) and ta[0].shape == (2, 16, 16, 16) and wa[0].shape == (2, 16, 1)
        assert all(torch.equal(x, y) for x, y in zip(ia + ta + wa, ib + tb + wb))
        assert ma[0]['source'] == ['h36m', 'mpii']
        assert sorted(ma[0]) == ['center', 'joints_2d_transformed', 'joints_vis', 'scale', 'source', 'subject']
        assert float(ta[0].max()) <= 1.0 and float(ta[0].amax(dim=(2, 3)).min()) > 0.5
    assert not torch.equal(a[0][0][0], a[1][0][0])
