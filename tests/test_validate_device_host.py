"""The device-resident validation epoch (core.function.validate_device, csrc/validate.hip), what can be
checked without a GPU: the entry points exist and are declared and bound, argument errors come back before
any launch, CPU tensors are refused, and the evaluation tables computed from integer counts are the
reference's (tests/golden/validate_eval.npz, made by tests/golden/make_validate_golden.py from
MultiViewH36MCompatible.evaluate and MPIIDatasetCompatible.evaluate)."""
import os
import re

import numpy as np
import pytest
import torch

from posu import _native, metrics, ops

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ('posu_decode_views_workspace', 'posu_decode_views', 'posu_detection_counts')


def mapping_of(g, prefix):
    """(u2a_mapping, actual_joints) of a golden case, the mapping in the stored (unsorted) key order."""
    u2a = {int(k): ('*' if v < 0 else int(v)) for k, v in zip(g[prefix + '.u2a_keys'], g[prefix + '.u2a_values'])}
    return u2a, dict(enumerate(g[prefix + '.joint_names'].tolist()))


def assert_table(name_values, perf, g, prefix):
    assert list(name_values.keys()) == g[prefix + '.names'].tolist()
    got = np.array([float(v) for v in name_values.values()])
    print(prefix, got, g[prefix + '.values'])
    assert np.array_equal(got, g[prefix + '.values'], equal_nan=True)
    assert np.array_equal(np.float64(perf), g[prefix + '.perf'], equal_nan=True)


def test_the_validation_entry_points_import():
    from core.function import ValidationResult, validate_batch_device, validate_device
    assert all(callable(f) for f in (validate_device, validate_batch_device, ValidationResult, ops.decode_views,
                                     ops.detection_counts, metrics.evaluate_h36m, metrics.evaluate_mpii))


def test_new_symbols_are_declared_and_bound():
    src = open(os.path.join(REPO, 'include', 'posu.h')).read()
    src = re.sub(r'/\*.*?\*/', '', src, flags=re.S)
    lib = _native.load()
    for name in SYMBOLS:
        assert re.search(r'\b%s\s*\(' % name, src), name
        assert name in _native.exported_symbols() and hasattr(lib, name), name
    assert lib.posu_abi_version() == _native.ABI_VERSION == 16


def test_the_workspace_query_answers_on_the_host():
    lib = _native.load()
    assert lib.posu_decode_views_workspace(4, 2, 16) == 4 * 2 * 16 * 4
    assert lib.posu_decode_views_workspace(8, 1, 1) == 8 * 4 and lib.posu_decode_views_workspace(1, 3, 5) == 60
    assert lib.posu_decode_views_workspace(3, 0, 16) == 0          # an empty batch needs nothing
    for v in (0, 9, -1):
        assert lib.posu_decode_views_workspace(v, 2, 16) == -1
    assert lib.posu_decode_views_workspace(4, -1, 16) == -1 and lib.posu_decode_views_workspace(4, 2, 0) == -1
    assert lib.posu_decode_views_workspace(8, 1 << 20, 1 << 8) == -1   # 2^31 maps


def _decode(lib, v=4, n=2, j=16, h=8, w=8, row0=0, rows=8, outputs=None, preds=None):
    return lib.posu_decode_views(outputs, None, None, 0, None, None, v, n, j, h, w, 1, 0.5, None, preds, row0, rows,
                                 None, None, None, None, None, 0, None)


def test_argument_errors_come_back_before_any_launch():
    """Every call here would fault if it reached a kernel: the pointers are null or made up."""
    import ctypes
    lib = _native.load()
    assert _decode(lib) == 1 and 'null pointer' in _native.last_error()
    assert _decode(lib, v=0) == 1 and '1 to 8 views' in _native.last_error()
    assert _decode(lib, v=9) == 1 and '1 to 8 views' in _native.last_error()
    for bad in ({'n': -1}, {'j': 0}, {'h': 0}, {'w': -3}, {'h': 1 << 16, 'w': 1 << 15}):
        assert _decode(lib, **bad) == 1 and 'bad shape' in _native.last_error(), bad
    # rows [row0, row0 + V * N) must lie inside the buffers
    for bad in ({'row0': -1}, {'row0': 1}, {'rows': 7}, {'row0': 8, 'rows': 8}):
        assert _decode(lib, **bad) == 1 and 'do not fit' in _native.last_error(), bad
    # a table with a null view
    table = (ctypes.c_void_p * 4)(None, None, None, None)
    fake = ctypes.c_void_p(4096)
    assert _decode(lib, outputs=ctypes.cast(table, ctypes.c_void_p), preds=fake) == 1
    assert 'null view pointer' in _native.last_error()
    # N = 0 launches nothing and needs no pointer
    assert _decode(lib, n=0, rows=0) == 0

    def counts(pred=None, stride=2, t=1, form=0, n=4, j=3, thr=True, out=True):
        th = (ctypes.c_double * 8)(0.5)
        return lib.posu_detection_counts(pred, stride, None, None, None, ctypes.cast(th, ctypes.c_void_p) if thr else
                                         None, t, form, n, j, fake if out else None, None)
    assert counts(out=False) == 1 and 'null pointer' in _native.last_error()
    assert counts(thr=False) == 1 and 'null pointer' in _native.last_error()
    assert counts(t=0) == 1 and counts(t=9) == 1 and '1 to 8 thresholds' in _native.last_error()
    assert counts(n=-1) == 1 and counts(j=0) == 1 and 'bad shape' in _native.last_error()
    assert counts(stride=4) == 1 and '[N, J, 2] or [N, J, 3]' in _native.last_error()
    assert counts(form=2) == 1 and 'form 0' in _native.last_error()
    assert counts() == 1 and 'null pointer' in _native.last_error()     # pred, gt, head with N > 0


def test_cpu_tensors_are_refused():
    hm = [torch.rand(1, 2, 4, 4) for _ in range(2)]
    with pytest.raises(RuntimeError, match='cuda'):
        ops.decode_views(hm)
    with pytest.raises(RuntimeError, match='cuda'):
        ops.decode_views(hm, flipped=hm, targets=hm, affine64=torch.zeros(2, 2, 3, dtype=torch.float64))
    with pytest.raises(RuntimeError, match='cuda'):
        ops.detection_counts(torch.rand(4, 3, 2), torch.rand(4, 3, 2, dtype=torch.float64),
                             torch.ones(4, dtype=torch.float64), [0.5])


def test_device_meters_take_their_names():
    """train()'s table keeps its ten slots; validate_device asks for two."""
    from core.function import METERS, VALID_METERS
    assert len(METERS) == 10 and METERS[:3] == ('loss', 'mse', 'acc')
    assert VALID_METERS == ('loss', 'acc')


def test_h36m_table_from_counts_is_the_reference(golden):
    g = golden('validate_eval.npz')
    u2a, joints = mapping_of(g, 'h36m')
    n = g['h36m.pred'].shape[0]
    name_values, perf = metrics.h36m_name_values(g['h36m.counts_form0'], n, u2a, joints)
    assert_table(name_values, perf, g, 'h36m')
    assert 'head' not in name_values and list(name_values)[-5:] == ['mean(15j)', 'mean@0.4', 'mean@0.3', 'mean@0.2',
                                                                    'mean@0.1']
    assert len(name_values) == 16 + 5
    # the detected counts alone ([T, K]) are enough
    again, _ = metrics.h36m_name_values(g['h36m.counts_form0'][:, 0], n, u2a, joints)
    assert list(again.items()) == list(name_values.items())
    with pytest.raises(ValueError, match='head'):
        metrics.h36m_name_values(g['h36m.counts_form0'], n, u2a, {k: 'j%d' % k for k in joints})


def test_mpii_table_from_counts_is_the_reference(golden):
    g = golden('validate_eval.npz')
    u2a, joints = mapping_of(g, 'mpii')
    name_values, perf = metrics.mpii_name_values(g['mpii.counts_form1'][:1], u2a, joints)
    assert_table(name_values, perf, g, 'mpii')
    assert list(name_values)[-1] == 'mean' and len(name_values) == 16 + 1
    # the joint that is never visible: 0 / 0
    assert g['mpii.counts_form1'][0, 1].min() == 0 and np.isnan(perf)
    assert sum(np.isnan(v) for v in name_values.values()) == 2


def test_the_golden_holds_the_boundary_rows(golden):
    """d == head * thr exactly (detected by <=), a row on which the two forms disagree, d / head == 0.5."""
    g = golden('validate_eval.npz')
    u2a, _ = mapping_of(g, 'h36m')
    u, _ = metrics.u2a_indices(u2a)
    pred, gt = g['h36m.pred'].astype(np.float64), g['h36m.gt'][:, u]
    head = np.amax(g['h36m.scales'], axis=1) * 200 / 10.0
    d = np.sqrt(np.sum((gt - pred[:, :, :2]) ** 2, axis=2))
    assert head[0] == 10.0 and d[0, 0] == 5.0 == head[0] * 0.5 and d[0, 1] == 4.0 == head[0] * 0.4
    assert bool(g['h36m.forms_disagree'])
    diff = g['h36m.counts_form0'] != g['h36m.counts_form1']
    assert diff.any() and not diff[0].any()            # never at 0.5: a product with 0.5 is exact
    u2a, _ = mapping_of(g, 'mpii')
    u, _ = metrics.u2a_indices(u2a)
    d = np.sqrt(np.sum((g['mpii.gt'][:, u] - g['mpii.pred'][:, :, :2].astype(np.float64)) ** 2, axis=2))
    assert d[0, 0] / g['mpii.headsizes'][0] == 0.5 and g['mpii.joints_vis'][0, u[0], 0] == 1
