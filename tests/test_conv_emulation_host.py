"""The derived bound of tests/conv_emulation.py on the CPU, for every case geometry of
tests/test_gpu_conv_edges.py: a CORRECT implementation with another summation order (torch CPU
fp32 on the dtype-rounded operands, result rounded RNE to the dtype) lies inside the bound, and
each of a list of wrong implementations -- a zeroed weight tap, the last K mod BK products dropped,
the input shifted by a column, the residual of the neighbouring pixel, no ReLU, one channel's scale
replaced by 1, an output channel never stored, a store into a guard band, an untouched pixel of
the in-place data gradient off by one ulp, the weight gradient's last pixel stage dropped -- lies
outside it.  The results go through the same sentinel allocator and checks as the kernels'."""
import pytest
import torch

import conv_emulation as ce

KEYS = ['f32', 'bf16', 'f16']


def _stored(c, key, ref):
    """ref (emulation layout) stored into a sentinel-guarded buffer in the kernel's layout."""
    out = ce.from_layout(c, ref, key)
    g = ce.Guarded(out.shape, out.dtype, 'cpu')
    g.out.copy_(out)
    return g


def _bits(t):
    return t.view(torch.int16 if t.element_size() == 2 else torch.int32)


def _run(c, key, inp, emul, mutant=None):
    buffer_level = mutant in ('sentinel_channel', 'band', 'ulp')
    g = _stored(c, key, ce.restate(c, inp, key, None if buffer_level else mutant))
    if mutant == 'sentinel_channel':     # one output channel (a weight gradient's row) left unwritten
        if ce.is_nhwc(c):
            _bits(g.out)[..., -1] = g.pattern
        elif c['kind'] == 'head':
            _bits(g.out)[:, -1] = g.pattern
        elif c['kind'] == 'gemm':
            _bits(g.out)[-1, :, -1] = g.pattern
        else:
            _bits(g.out)[-1] = g.pattern
    elif mutant == 'band':
        g.buf[g.nb + g.n] = 0
    elif mutant == 'ulp':                # pixel (0, 1) is not one the in-place kernel writes
        _bits(g.out)[0, 0, 1, 0] += 1
    if c.get('inplace'):
        return ce.verify_inplace(c, g, emul, inp['res'])
    return ce.verify(c, g, emul)


@pytest.mark.parametrize('key', KEYS)
@pytest.mark.parametrize('group', list(ce.GROUPS))
def test_fp32_restatement_inside_the_bound_and_mutants_outside(group, key):
    worst, survived, tried = 0.0, [], set()
    for c in ce.GROUPS[group](key):
        inp = ce.make_inputs(c, key)
        emul = ce.emulate(c, inp, key)
        worst = max(worst, _run(c, key, inp, emul))
        for m in ce.mutants(c, key):
            tried.add(m)
            try:
                _run(c, key, inp, emul, m)
            except AssertionError:
                continue
            survived.append((c['id'], m))
    print('%s %s: fp32 restatement worst deviation / bound %.3g over %d cases; mutants %s'
          % (group, key, worst, len(ce.GROUPS[group](key)), sorted(tried)))
    assert not survived, survived


def test_every_mutant_kind_is_exercised():
    tried = {m for key in KEYS for group in ce.GROUPS for c in ce.GROUPS[group](key) for m in ce.mutants(c, key)}
    assert tried == {'tap', 'ktail', 'xshift', 'resshift', 'norelu', 'scale1', 'sentinel_channel', 'band', 'ulp',
                     'last_stage'}


@pytest.mark.parametrize('key', KEYS)
def test_ragged_split_follows_the_split_rule(key):
    """The weight-gradient case built from the launcher's rule: splits of several stages, the last
    one holding a single pixel."""
    bp = ce.WGRAD_BP[key]
    tiles = ce.wgrad_tiles(136 if key != 'f32' else 132, 576)
    p = ce.wgrad_ragged_p(tiles, bp)
    pps, splits = ce.wgrad_split_rule(p, tiles, bp)
    assert tiles == 10 and pps % bp == 0 and pps > bp and splits > 1 and p - pps * (splits - 1) == 1
    assert splits <= -(-ce.WGRAD_BLOCKS // tiles) + 1


def test_sentinel_allocator():
    for dt in (torch.float32, torch.bfloat16, torch.float16):
        g = ce.Guarded((3, 5, 8), dt, 'cpu')
        assert g.out.data_ptr() % 16 == 0 and g.out.shape == (3, 5, 8)
        assert bool(torch.isnan(g.buf.float()).all())
        with pytest.raises(AssertionError, match='never written'):
            g.check()
        g.out.zero_()
        g.check()
        g.buf[g.nb - 1] = 1
        with pytest.raises(AssertionError, match='guard band'):
            g.check()
