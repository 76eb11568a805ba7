"""The launch sequence of PoseResNetPlan.run(), read off on the CPU and compared with tests/plan_traces.json.

posu.ops.call is replaced by a recorder and ops.ptr by (storage bytes, byte offset), so a plan built
on CPU tensors "runs" without libposeu.so: a trace fixes the entry points and their order, every
integer argument (N, H, W, C, P, the weight stream's size, tile, relu) and which slice of which buffer
each launch reads and writes.  The geometry keys handed to plan._tuned (tune files persist them) and
the autotuner's candidate lists are pinned beside the traces.

    python tests/test_plan_trace.py --write

rewrites the fixture from the code as it stands; a refactor of the plan records it before and must
reproduce it unchanged after.
"""
import json
import os
import sys

import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
LIB = os.path.join(os.path.dirname(HERE), 'pose-unsupervised_amd', 'lib')
if LIB not in sys.path:
    sys.path.insert(0, LIB)

FIXTURE = os.path.join(HERE, 'plan_traces.json')

# name -> (ResNet depth, compute dtype, (H, W), frames per view, run(chunks=), switches set before the plan
# is built, switches set for the run)
CONFIGS = {}


def _cfg(name, depth, dtype, hw, n=2, chunks=None, build=(), run=()):
    CONFIGS[name] = (depth, dtype, hw, n, chunks, dict(build), dict(run))


_cfg('r50_bf16', 50, 'bf16', (256, 256))
_cfg('r50_bf16_chunks2', 50, 'bf16', (256, 256), chunks=2)
for _sw in ('FUSED_BOTTLENECK', 'S2_TAIL', 'S2_CHAIN', 'CHAINED_TAILS', 'TAIL_W24', 'STEM_VIEWS'):
    _cfg('r50_bf16_%s_off' % _sw, 50, 'bf16', (256, 256), run={_sw: False})
_cfg('r50_bf16_CHAIN_LAYERS_2B_on', 50, 'bf16', (256, 256), build={'CHAIN_LAYERS_2B': True})
_cfg('r50_bf16_fused_max_1mib', 50, 'bf16', (256, 256), run={'_FUSED_MAX_BYTES': 1 << 20})
_cfg('r50_fp16x3', 50, 'fp16x3', (256, 256))
_cfg('r50_fp16x3_chunks1', 50, 'fp16x3', (256, 256), chunks=1)
for _el in (1, 3):
    _cfg('r50_fp16x3_EARLY_LAYERS_%d' % _el, 50, 'fp16x3', (256, 256), run={'EARLY_LAYERS': _el})
_cfg('r50_fp16x3_SPLIT_TAILS_off', 50, 'fp16x3', (256, 256), build={'SPLIT_TAILS': False})
for _sw in ('CHAINED_TAILS', 'CHAIN_LAYERS'):
    _cfg('r50_fp16x3_%s_off' % _sw, 50, 'fp16x3', (256, 256), run={_sw: False})
_cfg('r50_fp16x3_n3', 50, 'fp16x3', (256, 256), n=3)
_cfg('r50_fp32', 50, 'fp32', (256, 256))
_cfg('r18_fp32_128', 18, 'fp32', (128, 128))
_cfg('r152_fp16_384', 152, 'fp16', (384, 384))
_cfg('r152_fp16_384_TAIL_W96_off', 152, 'fp16', (384, 384), build={'TAIL_W96': False})
# rows 50 / 25 / 13: the strided tail, the layer2 tail and the layer3 tail all fall back to conv launches
_cfg('r50_bf16_200x256', 50, 'bf16', (200, 256))
_cfg('r50_fp16x3_200x256', 50, 'fp16x3', (200, 256))
# rows 56 / 28 / 14: only layer3 falls back
_cfg('r50_bf16_224x256', 50, 'bf16', (224, 256))
# the direct stem: pack, conv, max-pool
_cfg('r50_bf16_255', 50, 'bf16', (255, 255))

# the documented single-block entry (_Block.__call__): every block of a plan called unchained, in order
BLOCK_CONFIGS = {'blocks_r50_bf16': (50, 'bf16', 64), 'blocks_r50_fp16x3': (50, 'fp16x3', 64),
                 'blocks_r152_fp16_384': (152, 'fp16', 96), 'blocks_r18_fp32_128': (18, 'fp32', 32)}

CAND_COUTS = (17, 64, 128, 256, 512, 2048)
CAND_SWITCHES = ('default', 'TILES_128X8', 'TILES_SPLIT_SG')

_NETS = {}
_PLANS = {}


def _patch_ops(mp, log):
    """posu.ops with every touch of the library or the GPU replaced; launches go to `log`."""
    from posu import ops, plan as P

    def fake_ptr(t):
        return None if t is None else [t.untyped_storage().nbytes(), t.storage_offset() * t.element_size()]

    def fake_stem_pool_views(views, wpk, scale, shift, code, out=None, hflip=False):
        n, _, h, w = views[0].shape
        log.append(['stem_pool_views', len(views), n, h, w, bool(hflip)])
        return torch.empty((n * len(views), h // 4, w // 4, 64 * ops.cmul(code)), dtype=ops.torch_dtype(code))

    def fake_stem_pool(x, wpk, scale, shift, code, out=None, hflip=False):
        n, _, h, w = x.shape
        log.append(['stem_pool', 1, n, h, w, bool(hflip), fake_ptr(out)])
        return out if out is not None else torch.empty((n, h // 4, w // 4, 64 * ops.cmul(code)),
                                                       dtype=ops.torch_dtype(code))

    mp.setattr(ops, 'call', lambda name, *args: log.append([name] + list(args)))
    mp.setattr(ops, 'ptr', fake_ptr)
    mp.setattr(ops, 'stream_of', lambda device: None)
    mp.setattr(ops, 'require_cuda', lambda *ts: None)
    mp.setattr(ops, 'conv_bk', lambda code: 32 if code == ops.F32 else 64)   # bk_of, csrc/conv_igemm.hip
    mp.setattr(ops, 'stem_pool_views', fake_stem_pool_views)
    mp.setattr(ops, 'stem_pool', fake_stem_pool)
    mp.setattr(P, '_TUNE_CACHE', {})


def _net(depth):
    if depth not in _NETS:
        from models.pose_resnet import get_pose_net
        from posu import synthetic as syn
        torch.manual_seed(depth)
        _NETS[depth] = get_pose_net(syn.make_cfg(num_layers=depth), is_train=False).eval()
    return _NETS[depth]


def _plan(mp, depth, dtype, build):
    """One plan per (net, dtype, construction switches), shared by the configurations that differ only in
    run-time switches."""
    from posu import ops, plan as P
    key = (depth, dtype, tuple(sorted(build.items())))
    if key not in _PLANS:
        with mp.context() as m:
            for k, v in build.items():
                m.setattr(P, k, v)
            with torch.no_grad():
                _PLANS[key] = P.PoseResNetPlan(_net(depth), ops.dtype_code(dtype))
    return _PLANS[key]


def _wrap_tuned(mp, keys):
    from posu import plan as P
    inner = P._tuned

    def tuned(key, cout, launch):
        keys.append(key)
        return inner(key, cout, launch)
    mp.setattr(P, '_tuned', tuned)


def _plain(obj):
    """Tuples as lists, as the fixture's JSON holds them."""
    return json.loads(json.dumps(obj))


def record_run(mp, name):
    from posu import plan as P
    depth, dtype, (h, w), n, chunks, build, run = CONFIGS[name]
    launches, keys = [], []
    with mp.context() as m:
        _patch_ops(m, launches)
        plan = _plan(m, depth, dtype, build)
        _wrap_tuned(m, keys)
        for k, v in run.items():
            m.setattr(P, k, v)
        views = [torch.zeros(n, 3, h, w) for _ in range(2)]
        with torch.no_grad():
            plan.run(plan.pack_input(views), chunks=chunks)
    return _plain({'launches': launches, 'tuned': keys})


def record_blocks(mp, name):
    from posu import ops
    depth, dtype, side = BLOCK_CONFIGS[name]
    launches, keys = [], []
    with mp.context() as m:
        _patch_ops(m, launches)
        plan = _plan(m, depth, dtype, {})
        _wrap_tuned(m, keys)
        x = torch.zeros((2, side, side, 64 * ops.cmul(plan.code)), dtype=ops.torch_dtype(plan.code))
        with torch.no_grad():
            for layer in plan.layers:
                for blk in layer:
                    x = blk(x, plan.code)
    return _plain({'launches': launches, 'tuned': keys})


def record_candidates(mp, switch):
    from posu import ops, plan as P
    with mp.context() as m:
        if switch != 'default':
            m.setattr(P, switch, False)
        return _plain([[cout, code, ksplit, P._tile_candidates(cout, code, ksplit=ksplit)]
                       for cout in CAND_COUTS for code in (None, ops.F32, ops.BF16, ops.F16, ops.F16X3)
                       for ksplit in (False, True)])


def _fixture():
    with open(FIXTURE) as f:
        return json.load(f)


def _first_difference(got, want):
    for i, (g, w) in enumerate(zip(got, want)):
        if g != w:
            return 'entry %d: got %r, recorded %r' % (i, g, w)
    return 'length: got %d, recorded %d' % (len(got), len(want))


@pytest.mark.parametrize('name', list(CONFIGS) + list(BLOCK_CONFIGS))
def test_plan_launches_match_recorded_trace(monkeypatch, name):
    """Every launch (entry point, integer arguments, buffer slices) and every _tuned geometry key of the
    configuration equals the recorded one, element for element."""
    got = (record_run if name in CONFIGS else record_blocks)(monkeypatch, name)
    want = _fixture()['traces'][name]
    for part in ('launches', 'tuned'):
        assert got[part] == want[part], '%s %s: %s' % (name, part, _first_difference(got[part], want[part]))


def test_fixture_holds_exactly_these_configurations():
    fx = _fixture()
    assert sorted(fx['traces']) == sorted(list(CONFIGS) + list(BLOCK_CONFIGS))
    assert sorted(fx['candidates']) == sorted(CAND_SWITCHES)


@pytest.mark.parametrize('switch', CAND_SWITCHES)
def test_tile_candidates_match_recorded_lists(monkeypatch, switch):
    """_tile_candidates for every output width class, dtype and ksplit, under the default switches and
    with TILES_128X8 / TILES_SPLIT_SG off."""
    assert record_candidates(monkeypatch, switch) == _fixture()['candidates'][switch]


def _write():
    mp = pytest.MonkeyPatch()
    traces = {name: record_run(mp, name) for name in CONFIGS}
    traces.update({name: record_blocks(mp, name) for name in BLOCK_CONFIGS})
    cands = {sw: record_candidates(mp, sw) for sw in CAND_SWITCHES}
    dumps = lambda o: json.dumps(o, separators=(',', ':'))
    out = ['{"traces":{']
    for i, (name, tr) in enumerate(traces.items()):
        out.append('%s:{' % dumps(name))
        for j, part in enumerate(('launches', 'tuned')):
            out.append('%s:[' % dumps(part))
            out.append(',\n'.join(dumps(e) for e in tr[part]))
            out.append(']' if j else '],')
        out.append('}' if i == len(traces) - 1 else '},')
    out.append('},"candidates":{')
    for i, (sw, rows) in enumerate(cands.items()):
        out.append('%s:[' % dumps(sw))
        out.append(',\n'.join(dumps(r) for r in rows))
        out.append(']' if i == len(cands) - 1 else '],')
    out.append('}}')
    with open(FIXTURE, 'w') as f:
        f.write('\n'.join(out) + '\n')
    print('wrote %s: %d traces, %d launches' % (FIXTURE, len(traces), sum(len(t['launches']) for t in traces.values())))


if __name__ == '__main__':
    if sys.argv[1:] != ['--write']:
        raise SystemExit('usage: python tests/test_plan_trace.py --write')
    _write()
