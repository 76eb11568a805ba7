"""Layer2's first Bottleneck as one launch (posu_bottleneck_s2_front_tail[_next]_fwd, csrc/tail_s2.hip):
the strided tail computing the block's own conv1 + BN1 + ReLU on each tile's 9 x 33 window from x,
against the conv1 launch followed by the tail that reads its output -- bit for bit -- and against
torch fp32; the padding of the window, the refusals, the plan switch S2_FRONT, and (on the CPU) the
layout of the stream with conv1's k-steps in front."""
import pytest
import torch
import torch.nn.functional as F

from posu import ops, packing, synthetic as syn
from posu._native import BF16, F16

gpu = pytest.mark.gpu


def _sentinel(like, shape):
    """Output pre-filled with a quiet-NaN pattern no kernel produces."""
    out = torch.empty(shape, dtype=like.dtype, device=like.device)
    out.view(torch.int16).fill_(0x7fc1 if like.dtype == torch.bfloat16 else 0x7e01)
    return out


def _bn(g, ch):
    return (torch.rand(ch, generator=g) + 0.5, torch.randn(ch, generator=g) * 0.1)


def _operands(g, cuda, code):
    """Weights and BNs of the block (and of the next block's conv1), built as
    test_layer2_first_block_strided_tail_matches_two_launches_and_torch builds them: host f32 tensors
    and the device packs.  BN1's shifts are of both signs, so relu(b1) != 0 on about half the channels."""
    w1 = torch.randn(128, 256, 1, 1, generator=g) * (2.0 / 256) ** 0.5
    bn1 = _bn(g, 128)
    w2 = torch.randn(128, 128, 3, 3, generator=g) * (2.0 / (9 * 128)) ** 0.5
    bn2 = _bn(g, 128)
    w3 = torch.randn(512, 128, 1, 1, generator=g) * (2.0 / 128) ** 0.5 * 0.3
    bn3 = _bn(g, 512)
    wd = torch.randn(512, 256, 1, 1, generator=g) * (2.0 / 256) ** 0.5 * 0.3
    bnd = _bn(g, 512)
    w1n = torch.randn(128, 512, 1, 1, generator=g) * (2.0 / 512) ** 0.5
    bn1n = _bn(g, 128)
    assert bool((bn1[1] > 0).any()) and bool((bn1[1] < 0).any())
    dt = ops.torch_dtype(code)
    bk = ops.conv_bk(code)
    host = dict(w1=w1, bn1=bn1, w2=w2, bn2=bn2, w3=w3, bn3=bn3, wd=wd, bnd=bnd)
    dev = dict(p1=packing.pack_conv_weight(w1.to(cuda), 256, bk, dt),
               p2=packing.pack_conv_weight(w2.to(cuda), 128, bk, dt),
               p1n=packing.pack_conv_weight(w1n.to(cuda), 512, bk, dt),
               pdual=packing.pack_dual_1x1_weight(w3.to(cuda), bn3[0].to(cuda), wd.to(cuda), bnd[0].to(cuda), dt),
               shift=(bn3[1].double() + bnd[1].double()).float().to(cuda),
               s=[t.to(cuda) for t in (bn1[0], bn1[1], bn2[0], bn2[1], bn1n[0], bn1n[1])])
    return host, dev


def _two_step(xd, d, code, nxt):
    s = d['s']
    t1 = ops.conv2d_nhwc(xd, d['p1'], 128, 1, 1, 1, 0, s[0], s[1], None, True, code)
    if nxt:
        return ops.bottleneck_s2_tail_next_nhwc(t1, xd, packing.pack_s2_tail_stream(d['p2'], d['pdual'], d['p1n']),
                                                s[2], s[3], d['shift'], s[4], s[5], code)
    return ops.bottleneck_s2_tail_nhwc(t1, xd, packing.pack_s2_tail_stream(d['p2'], d['pdual']), s[2], s[3],
                                       d['shift'], code), None


def _front(xd, d, code, nxt):
    s = d['s']
    n, h = xd.shape[:2]
    y = _sentinel(xd, (n, h // 2, 32, 512))
    if nxt:
        ws = packing.pack_s2_tail_stream(d['p2'], d['pdual'], d['p1n'], w1=d['p1'])
        return ops.bottleneck_s2_front_tail_next_nhwc(xd, s[0], s[1], ws, s[2], s[3], d['shift'], s[4], s[5], code,
                                                      out=y, t1n=_sentinel(xd, (n, h // 2, 32, 128)))
    ws = packing.pack_s2_tail_stream(d['p2'], d['pdual'], w1=d['p1'])
    return ops.bottleneck_s2_front_tail_nhwc(xd, s[0], s[1], ws, s[2], s[3], d['shift'], code, out=y), None


def _differing(a, b):
    return int((a.view(torch.int16) != b.view(torch.int16)).sum())


@gpu
@pytest.mark.parametrize('code', [BF16, F16])
@pytest.mark.parametrize('n,h', [(1, 8), (2, 16), (3, 24), (1, 64)])
def test_front_tail_matches_conv1_launch_then_tail_and_torch(cuda, code, n, h):
    """y (and, chained, y and t1n) of the one-launch block equals, bit for bit, the conv1 launch followed by
    posu_bottleneck_s2_tail[_next]_fwd; every output element is written (NaN sentinels); y is within the
    dtype's tolerance of torch fp32.  h = 8: one tile row, every tile has the top padding row; (2, 16):
    interior tile rows and the image-to-image boundary; (3, 24): an odd image count; (1, 64): the full map
    height.  Both column tiles occur everywhere, only the left one has a padding column."""
    g = torch.Generator().manual_seed(291 + h + n)
    hw, d = _operands(g, cuda, code)
    dt = ops.torch_dtype(code)
    xq = torch.randn(n, 256, h, 64, generator=g).abs().to(dt).float()
    xd = xq.permute(0, 2, 3, 1).contiguous().to(cuda, dt)
    y_ref, _ = _two_step(xd, d, code, False)
    yn_ref, t1n_ref = _two_step(xd, d, code, True)
    y, _ = _front(xd, d, code, False)
    yn, t1n = _front(xd, d, code, True)
    torch.cuda.synchronize()
    dy, dyn, dt1 = _differing(y, y_ref), _differing(yn, yn_ref), _differing(t1n, t1n_ref)
    print('front tail n=%d h=%d: y differing %d; chained: y %d, t1n %d' % (n, h, dy, dyn, dt1))
    assert dy == 0 and dyn == 0 and dt1 == 0
    bn1, bn2, bn3, bnd = hw['bn1'], hw['bn2'], hw['bn3'], hw['bnd']
    t1r = F.relu(F.conv2d(xq, hw['w1']) * bn1[0].view(1, -1, 1, 1) + bn1[1].view(1, -1, 1, 1))
    t2r = F.relu(F.conv2d(t1r, hw['w2'], stride=2, padding=1) * bn2[0].view(1, -1, 1, 1) + bn2[1].view(1, -1, 1, 1))
    ref = F.relu(F.conv2d(t2r, hw['w3']) * bn3[0].view(1, -1, 1, 1) + bn3[1].view(1, -1, 1, 1) +
                 F.conv2d(xq, hw['wd'], stride=2) * bnd[0].view(1, -1, 1, 1) + bnd[1].view(1, -1, 1, 1))
    err = (y.float().cpu().permute(0, 3, 1, 2) - ref).abs()
    tol = 0.05 if code == BF16 else 0.01
    print('front tail vs torch fp32: max err %.4g (max |ref| %.4g)' % (float(err.max()), float(ref.abs().max())))
    assert float(err.max()) <= tol * float(ref.abs().max()) + tol, float(err.max())


@gpu
@pytest.mark.parametrize('code', [BF16, F16])
def test_front_tail_window_padding_is_zero_not_relu_b1(cuda, code):
    """x = 0 and b1 = +1 on every channel: t1 is 1 inside the image, and conv2's padding must still be 0.
    A window whose out-of-image pixels held relu(b1) = 1 would differ from the two-step path along the
    top row and the left column of every image."""
    g = torch.Generator().manual_seed(5)
    _, d = _operands(g, cuda, code)
    d['s'][1] = torch.ones(128, device=cuda)
    xd = torch.zeros(2, 16, 64, 256, device=cuda, dtype=ops.torch_dtype(code))
    y_ref, _ = _two_step(xd, d, code, False)
    y, _ = _front(xd, d, code, False)
    torch.cuda.synchronize()
    assert float(y_ref.float().abs().max()) > 0
    # the border outputs do see the padding: they differ from the interior ones of the reference
    assert not torch.equal(y_ref[:, 0, 5], y_ref[:, 2, 5]) and not torch.equal(y_ref[:, 2, 0], y_ref[:, 2, 5])
    assert _differing(y, y_ref) == 0


@gpu
def test_front_tail_refusals_name_the_entry_point(cuda):
    x = torch.zeros(1, 8, 64, 256, device=cuda, dtype=torch.bfloat16)
    w1 = torch.zeros(128, 256, device=cuda, dtype=torch.bfloat16)
    w2 = torch.zeros(128, 1152, device=cuda, dtype=torch.bfloat16)
    wdual = torch.zeros(512, 384, device=cuda, dtype=torch.bfloat16)
    w1n = torch.zeros(128, 512, device=cuda, dtype=torch.bfloat16)
    ws = packing.pack_s2_tail_stream(w2, wdual, w1=w1)
    wsn = packing.pack_s2_tail_stream(w2, wdual, w1n, w1=w1)
    s = torch.ones(128, device=cuda)
    sh = torch.ones(512, device=cuda)
    name = 'posu_bottleneck_s2_front_tail_fwd'
    with pytest.raises(RuntimeError, match=name + ': null pointer'):
        ops.bottleneck_s2_front_tail_nhwc(x, None, s, ws, s, s, sh, BF16)
    with pytest.raises(RuntimeError, match=name + '.*multiple of 8'):
        ops.bottleneck_s2_front_tail_nhwc(x[:, :4], s, s, ws, s, s, sh, BF16)
    with pytest.raises(RuntimeError, match=name + '.*input W = 64'):
        ops.bottleneck_s2_front_tail_nhwc(x[:, :, :32].contiguous(), s, s, ws, s, s, sh, BF16)
    # the plain tail's stream (no conv1 in front) and the chained front stream are both the wrong size
    with pytest.raises(RuntimeError, match=name + ': wstream holds'):
        ops.bottleneck_s2_front_tail_nhwc(x, s, s, packing.pack_s2_tail_stream(w2, wdual), s, s, sh, BF16)
    with pytest.raises(RuntimeError, match=name + ': wstream holds'):
        ops.bottleneck_s2_front_tail_nhwc(x, s, s, wsn, s, s, sh, BF16)
    with pytest.raises(RuntimeError, match=name + '.*alias'):
        ops.bottleneck_s2_front_tail_nhwc(x, s, s, ws, s, s, sh, BF16, out=x)
    namen = 'posu_bottleneck_s2_front_tail_next_fwd'
    with pytest.raises(RuntimeError, match=namen + ': wstream holds'):
        ops.bottleneck_s2_front_tail_next_nhwc(x, s, s, ws, s, s, sh, s, s, BF16)
    with pytest.raises(RuntimeError, match=namen + '.*alias'):
        ops.bottleneck_s2_front_tail_next_nhwc(x, s, s, wsn, s, s, sh, s, s, BF16, t1n=x)


@gpu
@pytest.mark.parametrize('precision', ['bf16', 'fp16'])
def test_plan_front_tail_is_bit_identical_and_one_launch_fewer(cuda, precision, monkeypatch):
    """The R50@256 plan at one frame per view, heuristic tiles (an empty tuning table): heatmaps and
    features with S2_FRONT on equal those with it off, and the forward makes exactly one library call
    fewer -- layer2 block 0's conv1."""
    import posu.plan as P
    from models.pose_resnet import get_pose_net
    net = get_pose_net(syn.make_cfg(num_layers=50, image_size=256), is_train=False, precision=precision)
    net.load_state_dict(syn.synthetic_state_dict(net.state_dict(), seed=0, bn_stats=syn.load_bn_stats(50, 256)))
    net = net.to(cuda).eval()
    monkeypatch.setattr(P, '_TUNE_CACHE', {})
    plan = net.plan(cuda)
    blk = plan.layers[1][0]
    assert 's2_front' in blk.packs and 's2_front_next' in blk.packs
    views = [v.to(cuda) for v in syn.synthetic_views(4, 1, 256, seed=13)]
    calls = []
    inner = ops.call
    monkeypatch.setattr(ops, 'call', lambda name, *a: (calls.append(name), inner(name, *a))[1])
    saved = P.S2_FRONT
    monkeypatch.setattr(P, 'S2_FRONT_TUNE', False)
    try:
        with torch.no_grad():
            P.S2_FRONT = True
            assert blk.select(views[0].new_zeros((4, 64, 64, 256)))[0] == 's2_tail'
            hm1, _, f1 = plan.run(plan.pack_input(views))
            on, calls[:] = list(calls), []
            P.S2_FRONT = False
            hm0, _, f0 = plan.run(plan.pack_input(views))
            off = list(calls)
    finally:
        P.S2_FRONT = saved
    torch.cuda.synchronize()
    assert torch.equal(hm1, hm0) and torch.equal(f1, f0)
    assert len(on) == len(off) - 1
    assert 'posu_bottleneck_s2_front_tail_next_fwd' in on and 'posu_bottleneck_s2_front_tail_next_fwd' not in off
    assert on.count('posu_conv2d_fwd') == off.count('posu_conv2d_fwd') - 1


@gpu
def test_tuner_chooses_between_the_two_forms_and_untuned_plans_keep_two_launches(cuda, monkeypatch):
    """S2_FRONT off (the default), S2_FRONT_TUNE on: a plan that was never tuned runs the conv1 launch and
    the tail; while the tuner is active the block times both forms and stores 1 / 0 under its 's2_front'
    key; the stored choice then decides, and S2_FRONT_TUNE off ignores it.  y is the same bit for bit."""
    import posu.plan as P
    from models.pose_resnet import get_pose_net
    net = get_pose_net(syn.make_cfg(num_layers=50, image_size=256), is_train=False, precision='bf16')
    net.load_state_dict(syn.synthetic_state_dict(net.state_dict(), seed=0, bn_stats=syn.load_bn_stats(50, 256)))
    net = net.to(cuda).eval()
    monkeypatch.setattr(P, '_TUNE_CACHE', {})
    monkeypatch.setattr(P, '_TUNE_TIMES', {})
    monkeypatch.setattr(P, 'S2_FRONT', False)
    monkeypatch.setattr(P, 'S2_FRONT_TUNE', True)
    blk = net.plan(cuda).layers[1][0]
    x = torch.randn(2, 64, 64, 256, generator=torch.Generator().manual_seed(3)).abs().to(cuda, torch.bfloat16)
    calls = []
    inner = ops.call
    monkeypatch.setattr(ops, 'call', lambda name, *a: (calls.append(name), inner(name, *a))[1])

    def launches():
        calls[:] = []
        with torch.no_grad():
            y, t1n = blk.run(x, BF16)
        torch.cuda.synchronize()
        return list(calls), y, t1n

    two = ['posu_conv2d_fwd', 'posu_bottleneck_s2_tail_next_fwd']
    one = ['posu_bottleneck_s2_front_tail_next_fwd']
    names, y0, t0 = launches()
    assert names == two and not P._TUNE_CACHE
    monkeypatch.setattr(P._Tuner, 'active', True)
    monkeypatch.setattr(P._Tuner, 'reps', 2)
    monkeypatch.setattr(P._Tuner, 'seen', [])
    names, y1, t1 = launches()
    monkeypatch.setattr(P._Tuner, 'active', False)
    key = ('s2_front', BF16, (2, 64, 64, 256), True)
    assert P._TUNE_CACHE[key] in (0, 1) and set(P._TUNE_TIMES[key]) == {0, 1}
    print('tuned s2_front at 2 frames:', P._TUNE_CACHE[key], P._TUNE_TIMES[key])
    assert names.count(one[0]) >= 3 and names.count(two[1]) >= 3     # both forms were timed
    # conv1's tile: the heuristic's before the tuning; the two-K-group tile 39 sums in another order
    same = P._TUNE_CACHE.get(('conv', BF16, (2, 64, 64, 256), 128, 1, 1, 0, False)) != 39
    for choice, want in ((1, one), (0, two)):
        P._TUNE_CACHE[key] = choice
        names, y, t = launches()
        assert names == want
        if same or choice:
            assert torch.equal(y, y0) and torch.equal(t, t0)
    P._TUNE_CACHE[key] = 1
    monkeypatch.setattr(P, 'S2_FRONT_TUNE', False)
    assert launches()[0] == two
    monkeypatch.setattr(P, 'S2_FRONT', True)
    assert launches()[0] == one


def test_front_stream_layout_and_refusals():
    """CPU: pack_s2_tail_stream(.., w1=) puts conv1's 8 k-steps in front of the unchanged stream, group cq's
    k-step p / n-tile j / lane 16 q + r holding w1[32 cq + 16 j + r][32 p + 8 q .. + 7]."""
    w2 = torch.arange(128 * 1152, dtype=torch.float32).reshape(128, 1152)
    wdual = -torch.arange(512 * 384, dtype=torch.float32).reshape(512, 384)
    w1n = torch.arange(128 * 512, dtype=torch.float32).reshape(128, 512) + 0.5
    w1 = (1000 * torch.arange(128).view(128, 1) + torch.arange(256).view(1, 256)).float()   # 1000 row + column
    for nxt, steps in ((None, 84), (w1n, 100)):
        base = packing.pack_s2_tail_stream(w2, wdual, nxt)
        ws = packing.pack_s2_tail_stream(w2, wdual, nxt, w1=w1)
        assert tuple(base.shape) == (4, steps, 2, 64, 8) and tuple(ws.shape) == (4, steps + 8, 2, 64, 8)
        assert ws.is_contiguous() and ws.numel() * 2 == 4 * (steps + 8) * 2048   # bytes in a 2-byte dtype
        assert torch.equal(ws[:, 8:], base)
        for cq, p, j, q, r in ((0, 0, 0, 0, 0), (3, 7, 1, 3, 15), (2, 5, 0, 1, 9), (1, 2, 1, 2, 4)):
            want = 1000.0 * (32 * cq + 16 * j + r) + 32 * p + 8 * q + torch.arange(8)
            assert torch.equal(ws[cq, p, j, 16 * q + r], want), (cq, p, j, q, r)
    with pytest.raises(ValueError, match='conv1 pack must be \\[128\\]\\[256\\]'):
        packing.pack_s2_tail_stream(w2, wdual, w1=w1[:, :128])
    with pytest.raises(ValueError, match='conv1 pack must be \\[128\\]\\[256\\]'):
        packing.pack_s2_tail_stream(w2, wdual, w1=w1n)
    with pytest.raises(ValueError, match='conv1 pack is'):
        packing.pack_s2_tail_stream(w2, wdual, w1=w1.to(torch.bfloat16))
    with pytest.raises(ValueError, match='conv2 pack \\[128\\]\\[1152\\]'):
        packing.pack_s2_tail_stream(w2[:64], wdual, w1=w1)
