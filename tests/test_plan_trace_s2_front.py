"""plan.S2_FRONT on changes exactly one thing in the launch sequence tests/plan_traces.json records: layer2
block 0's conv1 launch and the strided tail reading its output become the one front-fused launch -- every
other launch, every argument and every other _tuned key as recorded.  And a plan that was never tuned does
not take the one-launch form on its own (S2_FRONT_TUNE only follows a tuned table).  CPU only (the recorder
of test_plan_trace)."""
import pytest

import test_plan_trace as T

FRONT = {'posu_bottleneck_s2_tail_fwd': 'posu_bottleneck_s2_front_tail_fwd',
         'posu_bottleneck_s2_tail_next_fwd': 'posu_bottleneck_s2_front_tail_next_fwd'}
W1_BYTES = 4 * 8 * 2 * 1024   # conv1's 8 k-steps in front of the stream: 4 waves x 2 KB each


def _one_launch(conv1, tail):
    """The recorded conv1 launch and the tail launch reading its output -> the front-fused launch."""
    name, code, t1, x, n, h, w, c, p, ws, nbytes = tail[:11]
    assert conv1[0] == 'posu_conv2d_fwd' and conv1[2] == x and conv1[8] == p and conv1[17] == t1
    s1, b1 = conv1[13], conv1[14]
    return [FRONT[name], code, x, n, h, w, c, p, s1, b1, [ws[0] + W1_BYTES, ws[1]], nbytes + W1_BYTES] + tail[11:]


@pytest.mark.parametrize('name', ['r50_bf16', 'r50_bf16_chunks2', 'r50_bf16_S2_CHAIN_off', 'r50_bf16_224x256'])
def test_s2_front_on_is_the_recorded_plan_with_conv1_inside_the_tail(monkeypatch, name):
    from posu import plan as P
    want = T._fixture()['traces'][name]
    tails = [i for i, e in enumerate(want['launches']) if e[0] in FRONT]
    assert tails, 'the recorded plan runs layer2 block 0 as conv1 + the strided tail'
    expect = []
    for i, e in enumerate(want['launches']):
        if i + 1 in tails:
            continue                                  # the conv1 launch: folded into the next entry
        expect.append(_one_launch(want['launches'][i - 1], e) if i in tails else e)
    monkeypatch.setattr(P, 'S2_FRONT', True)
    got = T.record_run(monkeypatch, name)
    assert len(got['launches']) == len(want['launches']) - len(tails)
    assert got['launches'] == expect, T._first_difference(got['launches'], expect)
    # conv1 no longer goes through the tile table
    gone = [k for k in want['tuned'] if k not in got['tuned']]
    assert len(got['tuned']) == len(want['tuned']) - len(tails)
    assert gone and all(k[0] == 'conv' and k[3] == 128 and k[2][2:] == [64, 256] for k in gone)


def test_untuned_plan_keeps_the_two_launches(monkeypatch):
    """The defaults: S2_FRONT off, S2_FRONT_TUNE on.  With an empty tile table and no tuner running the block
    launches what the fixture records; a stored choice for its geometry switches the form."""
    from posu import ops, plan as P
    assert P.S2_FRONT is False and P.S2_FRONT_TUNE is True
    want = T._fixture()['traces']['r50_bf16']['launches']
    assert T.record_run(monkeypatch, 'r50_bf16')['launches'] == want
    tail = next(e for e in want if e[0] in FRONT)
    key = ('s2_front', ops.BF16, (tail[4], tail[5], tail[6], tail[7]), True)
    with monkeypatch.context() as m:
        launches = []
        T._patch_ops(m, launches)
        m.setitem(P._TUNE_CACHE, key, 1)   # (_patch_ops installs an empty table)
        plan = T._plan(m, 50, 'bf16', {})
        import torch
        with torch.no_grad():
            plan.run(plan.pack_input([torch.zeros(2, 3, 256, 256) for _ in range(2)]))
    names = [e[0] for e in launches]
    assert 'posu_bottleneck_s2_front_tail_next_fwd' in names and len(names) == len(want) - 1
