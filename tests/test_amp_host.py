"""fp16 training's loss-scaling entry points (posu_grad_stats, posu_adam_step_dev,
posu_loss_scale_update; additive to ABI 16) and their Python side (posu.amp.LossScaler,
posu.optim.Adam(capturable=True), PoseResNet.loss_scaler) as far as the host goes: exports,
argument refusals before the GPU is touched, type refusals, the model's precision switch."""
import ctypes

import numpy as np
import pytest
import torch

from posu import _native as nat
from posu import amp, optim, synthetic as syn

ENTRY_POINTS = ['posu_grad_stats_workspace', 'posu_grad_stats', 'posu_adam_step_dev', 'posu_loss_scale_update']
FAKE = 0x1000   # a non-null pointer no refused call dereferences


def _refused(name, *args):
    status = getattr(nat.load(), name)(*args)
    assert status != 0, name
    msg = nat.last_error()
    assert msg, name
    return msg


def test_library_exports_the_entry_points_at_abi_16():
    lib = nat.load()
    for name in ENTRY_POINTS:
        assert name in nat.exported_symbols()
        assert hasattr(lib, name)
    assert lib.posu_abi_version() == 16 == nat.ABI_VERSION


def _grad_table(sizes):
    rec = np.zeros(len(sizes), dtype=optim._REC_GRAD)
    for i, n in enumerate(sizes):
        rec[i] = (FAKE, n)
    return rec


def test_grad_stats_refuses_bad_arguments():
    rec = _grad_table([5, 2049])
    tab = rec.ctypes.data_as(ctypes.c_void_p)
    need = nat.load().posu_grad_stats_workspace(tab, 2)
    assert need == 8 * 3   # one double per 2048-element chunk
    assert 'null tensor table' in _refused('posu_grad_stats', None, 2, None, 0, FAKE, None, None, 0, None)
    assert 'found_inf' in _refused('posu_grad_stats', tab, 2, None, 0, None, None, None, 0, None)
    assert 'workspace' in _refused('posu_grad_stats', tab, 2, None, 0, FAKE, FAKE, FAKE, need - 1, None)
    assert 'scale' in _refused('posu_grad_stats', tab, 2, None, 1, FAKE, None, None, 0, None)
    neg = _grad_table([5, -1])
    ntab = neg.ctypes.data_as(ctypes.c_void_p)
    assert 'negative size' in _refused('posu_grad_stats', ntab, 2, None, 0, FAKE, None, None, 0, None)
    assert nat.load().posu_grad_stats_workspace(ntab, 2) == -1
    assert nat.load().posu_grad_stats_workspace(None, 2) == -1


def test_adam_step_dev_refuses_bad_arguments():
    rec = np.zeros(1, dtype=optim._REC_DEV)
    rec[0] = (FAKE, FAKE, FAKE, FAKE, FAKE, 8)
    tab = rec.ctypes.data_as(ctypes.c_void_p)
    hyper = (1e-3, 0.9, 0.999, 1e-8, 0.0)
    assert 'null tensor table' in _refused('posu_adam_step_dev', None, 1, *hyper, None, None, None, 0.0, None)
    rec[0]['n'] = -8
    assert 'negative size' in _refused('posu_adam_step_dev', tab, 1, *hyper, None, None, None, 0.0, None)
    rec[0]['n'] = 8
    rec[0]['step'] = 0
    assert 'null pointer' in _refused('posu_adam_step_dev', tab, 1, *hyper, None, None, None, 0.0, None)
    rec[0]['step'] = FAKE
    assert 'sum of squares' in _refused('posu_adam_step_dev', tab, 1, *hyper, None, None, None, 1.0, None)
    assert 'hyper' in _refused('posu_adam_step_dev', tab, 1, 1e-3, 1.0, 0.999, 1e-8, 0.0, None, None, None, 0.0, None)


def test_loss_scale_update_refuses_bad_arguments():
    assert 'found_inf' in _refused('posu_loss_scale_update', FAKE, FAKE, None, 2.0, 0.5, 2000, None)
    assert 'null scale' in _refused('posu_loss_scale_update', None, FAKE, FAKE, 2.0, 0.5, 2000, None)
    assert 'growth_interval' in _refused('posu_loss_scale_update', FAKE, FAKE, FAKE, 2.0, 0.5, 0, None)
    with pytest.raises(ValueError):
        amp.LossScaler(growth_interval=0)


def test_loss_scaler_steps_only_a_capturable_posu_adam():
    p = torch.nn.Parameter(torch.zeros(8))
    p.grad = torch.ones(8)
    scaler = amp.LossScaler()
    with pytest.raises(TypeError, match='capturable'):
        scaler.step(torch.optim.Adam([p]))
    with pytest.raises(TypeError, match='capturable'):
        scaler.step(optim.Adam([p]))
    assert torch.equal(p.detach(), torch.zeros(8))
    with pytest.raises(ValueError):
        optim.Adam([p], max_grad_norm=1.0)   # clipping lives in the capturable step


def test_capturable_adam_refuses_cpu_parameters():
    p = torch.nn.Parameter(torch.zeros(8))
    p.grad = torch.ones(8)
    opt = optim.Adam([p], capturable=True)
    assert opt._step_supports_amp_scaling and not optim.Adam([p])._step_supports_amp_scaling
    with pytest.raises(RuntimeError, match='MI355X HIP path'):
        opt.step()
    assert len(opt.state[p]) == 0   # refused before any state was made
    with pytest.raises(RuntimeError, match='MI355X HIP path'):
        amp.LossScaler().step(opt)


def test_loss_scaler_state_dict_round_trip_on_the_host():
    a = amp.LossScaler(init_scale=1024., growth_interval=7)
    sd = a.state_dict()
    assert sd == {'scale': 1024., 'growth_factor': 2., 'backoff_factor': .5, 'growth_interval': 7,
                  '_growth_tracker': 0}
    b = amp.LossScaler()
    b.load_state_dict(sd)
    assert b.state_dict() == sd and b.get_scale() == 1024.
    assert amp.LossScaler(enabled=False).state_dict() == {}


def test_fp16_trains_only_with_a_loss_scaler_attached():
    from models.pose_resnet import get_pose_net
    cfg = syn.make_cfg(num_layers=18, image_size=64)
    net = get_pose_net(cfg, is_train=False, precision='fp16').train()
    assert net.loss_scaler is None
    with pytest.raises(NotImplementedError, match='loss scaling'):
        net.train_plan()
    net = get_pose_net(cfg, is_train=False, precision='fp16', loss_scaler=amp.LossScaler()).train()
    assert net.train_plan().code == nat.F16
    with pytest.raises(RuntimeError, match='cuda'):   # past the precision check, refused as a CPU input
        net(torch.zeros(1, 3, 64, 64))
    net.precision = 'fp16x3'   # the split dtype still does not train
    with pytest.raises(NotImplementedError):
        net.train_plan()
    net.precision, net.loss_scaler = 'fp16', object()   # not a LossScaler
    with pytest.raises(NotImplementedError):
        net.train_plan()
