"""CPU-side pieces of bench.py's default line: the CPU baseline leg (the oracle chain on the host
cores) returns plain JSON values -- a leaked numpy meta dict once made the whole default line fail
at json.dumps on the GPU box -- and the line's serializer handles numpy scalars."""
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import bench  # noqa: E402


def test_cpu_baseline_entry_is_plain_json():
    cpu, ref = bench.cpu_baseline(18, 128, 1, 0.0)
    s = json.dumps(cpu)       # no default= hook: every value must already be a JSON type
    d = json.loads(s)
    assert d['kind'] == 'port' and d['cores'] >= 1 and isinstance(d['host_cpus'], int)
    assert d['value'] > 0 and d['batch1_forward_ms'] > 0
    assert 'X' in ref and 'host' in ref


def test_dump_outputs_dtypes_and_budget(tmp_path, monkeypatch):
    """--dump-outputs: float64 stays, everything else becomes float32; small arrays are written whole;
    over the byte budget the largest array is cut to a seeded sample, the same on every call."""
    big = np.arange(40000, dtype=np.int32).reshape(100, 400)
    arrays = {'big': big, 'x': np.ones((4, 3)), 'loss': np.array(1.5, np.float32)}
    bench.dump_outputs(str(tmp_path / 'a'), arrays)
    got = {f: np.load(tmp_path / 'a' / f) for f in sorted(os.listdir(tmp_path / 'a'))}
    assert list(got) == ['big.npy', 'loss.npy', 'x.npy']
    assert got['big.npy'].dtype == np.float32 and np.array_equal(got['big.npy'], big.astype(np.float32))
    assert got['x.npy'].dtype == np.float64 and got['loss.npy'].dtype == np.float32 and got['loss.npy'] == 1.5
    monkeypatch.setattr(bench, 'DUMP_BYTES', 64000)
    for d in ('b', 'c'):
        bench.dump_outputs(str(tmp_path / d), arrays)
    b, c = np.load(tmp_path / 'b' / 'big.npy'), np.load(tmp_path / 'c' / 'big.npy')
    assert np.array_equal(b, c) and b.ndim == 1 and 10000 < b.size < 40000
    assert np.all(np.diff(b) > 0) and np.all(np.isin(b, big.astype(np.float32)))   # elements of big, in order
    assert np.array_equal(np.load(tmp_path / 'b' / 'x.npy'), arrays['x'])
    assert sum(os.path.getsize(tmp_path / 'b' / f) for f in os.listdir(tmp_path / 'b')) <= 64000


def test_plain_run_is_the_default(monkeypatch):
    monkeypatch.setattr(sys, 'argv', ['bench.py', '--gpus', '1', '--steps', '7', '--warmup', '2'])
    a = bench.parse()
    assert (a.full, a.dump_outputs, a.steps, a.warmup) == (False, '', 7, 2)
    monkeypatch.setattr(sys, 'argv', ['bench.py', '--full', '--dump-outputs', 'out'])
    a = bench.parse()
    assert a.full and a.dump_outputs == 'out'


def test_line_serializer_converts_numpy_values():
    line = {'a': np.float32(1.5), 'b': np.int64(3), 'c': np.arange(3)}
    d = json.loads(json.dumps(line, default=bench._json_default))
    assert d == {'a': 1.5, 'b': 3, 'c': [0, 1, 2]}
