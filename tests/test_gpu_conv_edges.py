"""Edge shapes of the conv kernel family on the MI355X against the fp64 emulation and the derived
per-element bound of tests/conv_emulation.py (its docstring states the bound; its case lists are
the ones tests/test_conv_emulation_host.py validates the bound on): windows larger than the image,
the generic and row-uniform gathers away from the stem (also under the data gradient's
zero-upsampling), ragged Cout against every tile id and epilogue, the dual 1x1, the sub-pixel
deconv, the NCHW head, the row GEMM, the data gradient out of place and in place, and the split-K
weight gradient below one pixel stage, with a ragged last split, K below the n-tile and ragged
m-tiles.  Every output lies in a sentinel-filled buffer between two guard bands: every element must
be written, inside its bound (exact where the bound is zero), and the bands untouched.  Each test
prints its worst deviation / bound."""
import pytest
import torch
import torch.nn.functional as F

import conv_emulation as ce
from posu import aggregate, ops, packing, train_ops as T
from posu._native import BF16, F16, F32

pytestmark = pytest.mark.gpu

KEYS = ['f32', 'bf16', 'f16']
CODE = {'f32': F32, 'bf16': BF16, 'f16': F16}


def _nhwc(t, cuda, dt):
    return t.float().permute(0, 2, 3, 1).contiguous().to(cuda, dt)


def _par(v, cuda):
    return v.to(cuda) if v is not None else None


def _out_shape(c, inp):
    kind = c['kind']
    if kind == 'conv':
        return (c['n'],) + ce.out_grid(c) + (c['cout'],)
    if kind == 'dual':
        return (c['n'], c['h'], c['w'], c['cout'])
    if kind == 'deconv':
        return (c['n'], 2 * c['h'], 2 * c['w'], c['cout'])
    if kind == 'head':
        return (c['n'], c['j'], c['h'], c['w'])
    if kind == 'gemm':
        return (c['ncol'] // c['vblk'], c['m'], c['vblk'])
    if kind == 'dgrad':
        return (c['n'], c['h'], c['w'], c['cin'])
    if kind == 'wgrad':
        return (c['cout'], c['creal'], c['k'], c['k'])
    return (c['cin'], c['cout'], 4, 4)


def _launch(c, inp, key, cuda, tile=-1, out=None):
    """Case c on the GPU into a sentinel-guarded output (or `out`) -> the Guarded buffer."""
    code, dt, bk = CODE[key], ce.DTYPES[key], ce.BK[key]
    kind = c['kind']
    g = ce.Guarded(_out_shape(c, inp), ce.out_dtype(c, key), cuda) if out is None else out
    wf = inp['w'].float().to(cuda) if 'w' in inp else None
    if kind == 'conv':
        ops.conv2d_nhwc(_nhwc(inp['x'], cuda, dt), packing.pack_conv_weight(wf, c['c'], bk, dt), c['cout'], c['k'],
                        c['k'], c['s'], c['p'], _par(inp['scale'], cuda), _par(inp['shift'], cuda),
                        _nhwc(inp['res'], cuda, dt) if inp['res'] is not None else None, c['relu'], code, out=g.out,
                        out_hw=ce.out_grid(c) if c['crop'] else None, tile=tile)
    elif kind == 'dual':
        ones = torch.ones(c['cout'], device=cuda)
        wpk = packing.pack_dual_1x1_weight(wf, ones, inp['w2'].float().to(cuda), ones, dt)   # weights as they are
        ops.conv1x1_dual_nhwc(_nhwc(inp['x'], cuda, dt), _nhwc(inp['x2'], cuda, dt), c['s2'], wpk, c['cout'],
                              _par(inp['shift'], cuda), True, code, out=g.out, tile=tile,
                              scale=_par(inp['scale'], cuda))
    elif kind == 'deconv':
        ops.deconv4x4s2_nhwc(_nhwc(inp['x'], cuda, dt), packing.pack_deconv4x4_weight(wf, bk, dt), c['cout'],
                             _par(inp['scale'], cuda), _par(inp['shift'], cuda), bool(c['affine']), code, out=g.out,
                             tile=tile)
    elif kind == 'head':
        ops.head1x1_nchw(_nhwc(inp['x'], cuda, dt), packing.pack_conv_weight(wf, c['c'], bk, dt), c['j'],
                         _par(inp['shift'], cuda), code, out=g.out)
    elif kind == 'gemm':
        wt = torch.zeros(packing.round_up(c['ncol'], packing.COUT_ALIGN), c['k'], device=cuda)
        wt[:c['ncol']] = wf
        aggregate.gemm_rows(inp['x'].float().to(cuda, dt), wt.to(dt), c['ncol'], c['vblk'], code, out=g.out)
    elif kind == 'dgrad':
        res = _nhwc(inp['res'], cuda, dt) if inp['res'] is not None else None
        T.conv2d_dgrad(_nhwc(inp['dy'], cuda, dt), packing.pack_conv_dgrad_weight(wf, bk, dt), c['cin'], c['k'],
                       c['k'], c['s'], c['p'], (c['h'], c['w']), code, residual=res, out=g.out,
                       tile=None if tile == -1 else tile)
    elif kind == 'wgrad':
        T.conv2d_wgrad(_nhwc(inp['dy'], cuda, dt), _nhwc(inp['x'], cuda, dt), c['creal'], c['k'], c['k'], c['s'],
                       c['p'], code, out=g.out)
    else:
        T.deconv4x4s2_wgrad(_nhwc(inp['x'], cuda, dt), _nhwc(inp['dy'], cuda, dt), code, out=g.out)
    torch.cuda.synchronize()
    return g


def _sweep(group, key, cases, cuda):
    """Every case launched and verified; the cases outside their bound are reported together (an
    error of the runtime ends the sweep at once) -> worst deviation / bound."""
    worst, failed, exact, total = 0.0, [], 0, 0
    for c in cases:
        inp = ce.make_inputs(c, key)
        emul = ce.emulate(c, inp, key)
        exact, total = exact + int((emul.d == 0).sum()), total + emul.d.numel()
        g = _launch(c, inp, key, cuda)
        try:
            worst = max(worst, ce.verify(c, g, emul))
        except AssertionError as e:
            failed.append('%s: %s' % (c['id'], str(e).splitlines()[0]))
    print('%s %s: worst deviation / bound %.3g over %d cases (%d outputs, %.1f %% of them bound to be exact)'
          % (group, key, worst, len(cases), total, 100.0 * exact / total))
    assert not failed, '\n'.join(failed)


@pytest.mark.parametrize('key', KEYS)
def test_forward_edge_shapes(cuda, key):
    _sweep('forward', key, ce.forward_cases(key), cuda)


@pytest.mark.parametrize('key', KEYS)
def test_every_tile_id_on_ragged_cout(cuda, key):
    """Each tile id of the table on Cout 72 / 68, the 128- and 256-wide ones also on 200 / 132: inside
    the bound, and bit-identical to the heuristic's result -- every loop but the two-K-group tile (39,
    2-byte dtypes) walks K in one order."""
    worst, failed = 0.0, []
    for c in ce.tile_cases(key):
        inp = ce.make_inputs(c, key)
        emul = ce.emulate(c, inp, key)
        ref = _launch(c, inp, key, cuda).out
        for t in ce.tile_ids(key):
            if c['cout'] > 128 and ce.tile_bn(t) < 128:
                continue
            g = _launch(c, inp, key, cuda, tile=t)
            try:
                worst = max(worst, ce.verify(c, g, emul))
                if t != 39 or key == 'f32':
                    assert torch.equal(g.out, ref), 'differs from the heuristic tile by %.3g' % float(
                        (g.out.float() - ref.float()).abs().max())
            except AssertionError as e:
                failed.append('%s tile %d: %s' % (c['id'], t, str(e).splitlines()[0]))
    print('forward tiles %s: worst deviation / bound %.3g' % (key, worst))
    assert not failed, '\n'.join(failed)


@pytest.mark.parametrize('key', KEYS)
def test_dual_1x1_edge_shapes(cuda, key):
    _sweep('dual', key, ce.dual_cases(key), cuda)


@pytest.mark.parametrize('key', KEYS)
def test_deconv_edge_shapes(cuda, key):
    _sweep('deconv', key, ce.deconv_cases(key), cuda)


@pytest.mark.parametrize('key', KEYS)
def test_head_and_row_gemm_edge_shapes(cuda, key):
    _sweep('head / GEMM', key, ce.head_cases(key) + ce.gemm_cases(key), cuda)


@pytest.mark.parametrize('k', [1, 3])
@pytest.mark.parametrize('cin', [32, 64])
def test_split_fp16_ragged_cout(cuda, cin, k):
    """The split dtype on Cout 96 / 160 (ragged against the 128-wide tiles) with tests/test_gpu_split.py's
    gate: rel_err < 2e-6 of the magnitude sum; sentinel-guarded outputs."""
    S = ops.F16X3
    g0 = torch.Generator().manual_seed(7 * cin + k)
    n, h, w, pad = 1, 5, 7, k // 2
    worst = 0.0
    for cout in (96, 160):
        x = torch.randn(n, cin, h, w, generator=g0, dtype=torch.float64)
        wt = torch.randn(cout, cin, k, k, generator=g0, dtype=torch.float64) * 0.05
        scale = torch.rand(cout, generator=g0) + 0.5
        shift = torch.randn(cout, generator=g0) * 0.1
        res = torch.randn(n, cout, h, w, generator=g0, dtype=torch.float64)
        xs = packing.to_split(x.permute(0, 2, 3, 1).contiguous()).to(cuda)
        rs = packing.to_split(res.permute(0, 2, 3, 1).contiguous()).to(cuda)
        pk = packing.pack_conv_weight(wt.float(), cin, 32, torch.float32)
        e = packing.split_exponent(pk)
        ws = packing.to_split(pk, e).to(cuda)
        xq = ops.widen(xs, S).permute(0, 3, 1, 2).double().cpu()
        rq = ops.widen(rs, S).permute(0, 3, 1, 2).double().cpu()
        wq = wt.float().double()
        col = lambda v: v.double()[None, :, None, None]   # noqa: E731
        ref = F.relu(F.conv2d(xq, wq, padding=pad) * col(scale) + col(shift) + rq)
        mag = F.conv2d(xq.abs(), wq.abs(), padding=pad) * col(scale) + 1.0
        for tile in (-1, 0, 3, 7, 31):
            g = ce.Guarded((n, h, w, 2 * cout), torch.float16, cuda)
            ops.conv2d_nhwc(xs, ws, cout, k, k, 1, pad, (scale.double() * 2.0 ** -e).float().to(cuda),
                            shift.to(cuda), rs, True, S, out=g.out, tile=tile)
            torch.cuda.synchronize()
            g.check()
            got = ops.widen(g.out, S).permute(0, 3, 1, 2).double().cpu()
            rel = float(((got - ref).abs() / (mag + 1e-30)).max())
            worst = max(worst, rel)
            assert rel < 2e-6, (cout, tile, rel)
    print('split fp16 C %d %dx%d: worst rel_err %.3g' % (cin, k, k, worst))


@pytest.mark.parametrize('key', KEYS)
def test_data_gradient_edge_shapes(cuda, key):
    _sweep('data gradient', key, ce.dgrad_cases(key), cuda)


@pytest.mark.parametrize('key', KEYS)
def test_data_gradient_in_place(cuda, key):
    """The in-place 1x1 / stride-2 data gradient (inplace=True with a residual) that every downsample
    branch of the training step runs: the result IS the residual's storage, pixels (2i, 2j) satisfy
    the bound, every other pixel keeps the residual bit for bit, and the out-of-place launch on the
    same operands gives the same bits."""
    code, dt, bk = CODE[key], ce.DTYPES[key], ce.BK[key]
    worst = 0.0
    for c in ce.inplace_cases(key):
        inp = ce.make_inputs(c, key)
        emul = ce.emulate(c, inp, key)
        dy = _nhwc(inp['dy'], cuda, dt)
        wpk = packing.pack_conv_dgrad_weight(inp['w'].float().to(cuda), bk, dt)
        res = ce.Guarded(_out_shape(c, inp), dt, cuda, fill=_nhwc(inp['res'], cuda, dt))
        dx = T.conv2d_dgrad(dy, wpk, c['cin'], 1, 1, 2, 0, (c['h'], c['w']), code, residual=res.out, inplace=True)
        torch.cuda.synchronize()
        assert dx.data_ptr() == res.out.data_ptr() and dx.shape == res.out.shape, c['id']
        worst = max(worst, ce.verify_inplace(c, res, emul, inp['res']))
        ref = _launch(dict(c, inplace=False), inp, key, cuda)
        ce.verify(c, ref, emul)
        assert torch.equal(ref.out, dx), c['id']
    print('data gradient in place %s: worst deviation / bound %.3g' % (key, worst))


@pytest.mark.parametrize('key', KEYS)
def test_data_gradient_tile_candidates_on_ragged_cin(cuda, key):
    """Cin 72 and 200: every tile the autotuner may pick (plan._tile_candidates) gives the heuristic's
    dx bit for bit, as tests/test_gpu_train_kernels.py asserts for 64 / 128 / 256; the heuristic's dx
    inside the bound."""
    from posu import plan as pl
    worst, failed = 0.0, []
    for c in ce.dgrad_tile_cases(key):
        inp = ce.make_inputs(c, key)
        ref = _launch(c, inp, key, cuda)
        worst = max(worst, ce.verify(c, ref, ce.emulate(c, inp, key)))
        for t in pl._tile_candidates(c['cin'], CODE[key]):
            g = _launch(c, inp, key, cuda, tile=t)
            g.check()
            if not torch.equal(g.out, ref.out):
                failed.append('%s tile %d' % (c['id'], t))
    print('data gradient tiles %s: worst deviation / bound %.3g' % (key, worst))
    assert not failed, failed


@pytest.mark.parametrize('key', KEYS)
def test_weight_gradient_edge_shapes(cuda, key):
    """dW starts as the f32 sentinel: every element must be written, exact zeros included (the 3x3
    window over a 1x1 image has eight of nine taps zero)."""
    _sweep('weight gradient', key, ce.wgrad_cases(key) + ce.deconv_wgrad_cases(key), cuda)
    c = ce.wgrad_cases(key)[0]
    inp = ce.make_inputs(c, key)
    dw = _launch(c, inp, key, cuda).out.cpu()
    centre = torch.zeros(3, 3, dtype=torch.bool)
    centre[1, 1] = True
    assert bool((dw[:, :, ~centre] == 0).all()) and bool((dw[:, :, centre] != 0).any())
