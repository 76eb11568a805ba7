"""fp64 emulation of the conv kernel family with a DERIVED per-element bound, the sentinel output
allocator, and the edge-shape case lists shared by tests/test_gpu_conv_edges.py (the kernels) and
tests/test_conv_emulation_host.py (the bound itself, on the CPU).

The kernels' stated arithmetic (csrc/conv_igemm.hip, csrc/conv_wgrad.hip): operands already rounded
to the compute dtype, EXACT products (bf16 x bf16 and fp16 x fp16 fit an f32 mantissa; an f32
product is fused into its addition by the f32 MFMA), f32 accumulation of K terms in any order, the
affine (scale, shift), the residual add and ReLU in f32, one rounding on store.  So against the
fp64 value v of the same operands

    |pre-rounding kernel value - v| <= dv,   dv = ACC |s| gamma_K S + R u (|v| + dv),

gamma_K = K u / (1 - K u), u = 2^-24, S = conv(|x|, |w|) the magnitude sum, K the number of
accumulated products INCLUDING padding (the kernels add the zeros too), R the f32 roundings after
the accumulation: 2 for the NHWC epilogue (affine, residual add), 1 for the NCHW head's bias add,
0 for the row GEMM.  The stored value is the dtype rounding (after ReLU) of something in
[v - dv, v + dv]; rounding is monotone, so it lies between the roundings of the interval's ends
(`_store`) -- and must be EXACT where the interval holds no rounding boundary.  An f32 output is
its own rounding, the same statement with the f32 format.

ACC is the accumulation factor: 1 is the standard bound for K additions each rounded to nearest,
in any order and any grouping -- which covers a 16x16x32 MFMA adding its 32 products (the f32
16x16x4 one: 4) to an accumulator element inside the matrix core, as long as no step there loses
more than a round-to-nearest addition would.  Raising it (to at most 2: every step truncating
instead of rounding) would need that argument made from the hardware's documentation; the kernels
sit inside ACC = 1 at every shape here, so it is not made.

The weight gradient sums P pixel products per element through the block's pixel stages, its two
stage groups and the split-K reduction: gamma_(P + splits) S + u |dW| with `splits` the
launcher's upper limit ceil(128 / tiles) + 1.
"""
import math

import torch
import torch.nn.functional as F

U32 = 2.0 ** -24
ACC = 1
DTYPES = {'f32': torch.float32, 'bf16': torch.bfloat16, 'f16': torch.float16}
BK = {'f32': 32, 'bf16': 64, 'f16': 64}           # K-tile of the implicit GEMM (128-byte rows)
WGRAD_BP = {'f32': 32, 'bf16': 64, 'f16': 64}     # pixels per stage of the weight-gradient kernel
WGRAD_BLOCKS = 128                                # its blocks per launch (tiles x pixel splits)
# quiet-NaN patterns no kernel produces (tests/test_gpu_bottleneck.py::_sentinel; f32: 0x7fc00001)
SENTINEL = {torch.bfloat16: 0x7fc1, torch.float16: 0x7e01, torch.float32: 0x7fc00001}
BAND = 4096                                       # guard band bytes on each side of an output


def _q(t, dt=torch.bfloat16):
    """Round an fp64 tensor to dt (RNE) and back, as a kernel store does."""
    if dt == torch.float32:
        return t.float().double()
    return t.float().to(dt).double()


def _col(v):
    return v.double().view(1, -1, 1, 1)


def _gamma(k):
    return k * U32 / (1 - k * U32)


class _E:
    """An emulated stored tensor (fp64 values, exactly representable in the dtype) and its
    per-element bound d on the kernel's deviation from it."""

    def __init__(self, v, d=None):
        self.v, self.d = v, torch.zeros_like(v) if d is None else d


def _store(v, dv, relu=True, dt=torch.bfloat16):
    """Round (after ReLU) a pre-rounding value v known to within dv: -> _E."""
    act = F.relu if relu else (lambda t: t)
    r = _q(act(v), dt)
    d = torch.maximum((_q(act(v + dv), dt) - r).abs(), (_q(act(v - dv), dt) - r).abs())
    return _E(r, d)


def _conv(srcs, scale, shift, residual=None, relu=True, dt=torch.bfloat16, out_hw=None, rounds=2):
    """sum over the sources of their convolutions, * scale + shift (+ residual): the emulated stored
    output and its bound.  A source is (E input, fp64 weight already rounded as packed, stride,
    padding) for a Conv2d weight [Cout, C, KH, KW], or (E, weight, 2, 1, 'deconv') for a
    ConvTranspose2d(4, s2, p1) weight [C, Cout, 4, 4] (2 x 2 taps per output).  scale / shift may be
    None; out_hw crops the output grid; rounds = the f32 roundings after the accumulation."""
    v = S = P = 0
    k = 0
    for a, w, stride, pad, *kind in srcs:
        if kind and kind[0] == 'deconv':
            op = lambda t, wt: F.conv_transpose2d(t, wt, stride=2, padding=1)   # noqa: E731
            k += w.shape[0] * 4
        else:
            op = lambda t, wt: F.conv2d(t, wt, stride=stride, padding=pad)      # noqa: E731
            k += w.shape[1] * w.shape[2] * w.shape[3]
        v = v + op(a.v, w)
        S = S + op(a.v.abs(), w.abs())
        P = P + op(a.d, w.abs())
    if out_hw is not None:
        v, S, P = (t[:, :, :out_hw[0], :out_hw[1]] for t in (v, S, P))
    sc = _col(scale) if scale is not None else 1.0
    v = v * sc
    if shift is not None:
        v = v + _col(shift)
    dv = abs(sc) * (P + ACC * _gamma(k) * S)
    if residual is not None:
        v = v + residual.v
        dv = dv + residual.d
    dv = dv + rounds * U32 * (v.abs() + dv)
    return _store(v, dv, relu, dt)


def _dgrad(dy, w, stride, pad, hw, residual=None, dt=torch.bfloat16):
    """Data gradient of a Conv2d weight w [Cout, Cin, KH, KW]: dx = conv_transpose(dy, w) over the
    input grid hw (+ residual); K = KH KW Cout products per element, the upsampling zeros included."""
    kh, kw = w.shape[2], w.shape[3]
    op_h = hw[0] - ((dy.v.shape[2] - 1) * stride - 2 * pad + kh)
    op_w = hw[1] - ((dy.v.shape[3] - 1) * stride - 2 * pad + kw)
    op = lambda t, wt: F.conv_transpose2d(t, wt, stride=stride, padding=pad, output_padding=(op_h, op_w))  # noqa: E731
    v = op(dy.v, w)
    dv = op(dy.d, w.abs()) + ACC * _gamma(kh * kw * w.shape[0]) * op(dy.v.abs(), w.abs())
    if residual is not None:
        v = v + residual.v
        dv = dv + residual.d
    dv = dv + 2 * U32 * (v.abs() + dv)
    return _store(v, dv, False, dt)


def wgrad_tiles(cout, k):
    """Tiles of the weight-gradient launch: 64- or 128-row m-tiles, 128-wide n-tiles."""
    bm = 64 if cout <= 64 else 128
    return -(-cout // bm) * -(-k // 128)


def wgrad_split_rule(p, tiles, bp):
    """The launcher's documented pixel split (csrc/conv_wgrad.hip, launch_wgrad): as many splits as
    give WGRAD_BLOCKS blocks, at most one per pixel stage; whole stages per split -> (pps, splits)."""
    pst = -(-p // bp)
    splits = max(1, min(-(-WGRAD_BLOCKS // tiles), pst))
    pps = -(-pst // splits) * bp
    return pps, -(-p // pps)


def wgrad_ragged_p(tiles, bp):
    """The smallest P whose last split holds ONE pixel (P = pps (splits - 1) + 1) with splits of
    more than one stage, under wgrad_split_rule."""
    for p in range(bp + 1, 1 << 16):
        pps, splits = wgrad_split_rule(p, tiles, bp)
        if pps > bp and splits > 1 and p == pps * (splits - 1) + 1:
            return p
    raise AssertionError('no ragged split found')


def _wgrad(dy, x, wshape, stride, pad):
    """dW [Cout, Creal, KH, KW] (f32 output) of a conv over x [N, C >= Creal, H, W] with output
    gradient dy: fp64 value and the bound gamma_(P + splits) S + u |dW|."""
    cout, creal, kh, kw = wshape
    xr = x[:, :creal]
    v = torch.nn.grad.conv2d_weight(xr, wshape, dy, stride=stride, padding=pad)
    S = torch.nn.grad.conv2d_weight(xr.abs(), wshape, dy.abs(), stride=stride, padding=pad)
    p = dy.shape[0] * dy.shape[2] * dy.shape[3]
    splits = -(-WGRAD_BLOCKS // wgrad_tiles(cout, kh * kw * x.shape[1])) + 1
    return _E(v, ACC * _gamma(p + splits) * S + U32 * v.abs())


# ---------------------------------------------------------------- the sentinel allocator
class Guarded:
    """An output carved out of a larger buffer with a BAND-byte guard band on each side, bands and
    interior pre-filled with the dtype's sentinel pattern (fill: the interior's initial values
    instead, for an operand the kernel updates in place)."""

    def __init__(self, shape, dtype, device, fill=None):
        es = torch.empty((), dtype=dtype).element_size()
        self.nb, self.n = BAND // es, int(math.prod(shape))
        self.pattern = SENTINEL[dtype]
        self.buf = torch.empty(self.n + 2 * self.nb, dtype=dtype, device=device)
        self.bits = self.buf.view(torch.int16 if es == 2 else torch.int32)
        self.bits.fill_(self.pattern)
        self.out = self.buf[self.nb:self.nb + self.n].view(shape)
        if fill is not None:
            self.out.copy_(fill)

    def check(self, written=True):
        """The bands bit-for-bit untouched and (written) no interior element still the pattern."""
        bits = self.bits.cpu()
        lo, hi = bits[:self.nb], bits[self.nb + self.n:]
        assert bool((lo == self.pattern).all()) and bool((hi == self.pattern).all()), \
            'guard band touched at %d elements' % int((lo != self.pattern).sum() + (hi != self.pattern).sum())
        if written:
            left = int((bits[self.nb:self.nb + self.n] == self.pattern).sum())
            assert left == 0, '%d output elements never written' % left


def check_bound(name, got, emul):
    """got (fp64, emul's layout) within emul's bound at EVERY element -> the worst deviation / bound."""
    assert got.shape == emul.v.shape, (name, got.shape, emul.v.shape)
    dev = (got - emul.v).abs()
    worst = float((dev / emul.d.clamp_min(1e-300)).max())
    assert bool(torch.isfinite(got).all()), '%s: non-finite outputs' % name
    bad = dev > emul.d
    assert not bool(bad.any()), '%s: deviation beyond the derived bound at %d of %d elements (worst %.3g x)' % (
        name, int(bad.sum()), bad.numel(), worst)
    return worst


def _check(name, got_nhwc, emul):
    """The fused-block gate of tests/test_gpu_rounding_emulation.py (bf16)."""
    got = got_nhwc.float().cpu().permute(0, 3, 1, 2).double()
    dev = (got - emul.v).abs()
    ulp = 2.0 ** -7 * emul.v.abs().clamp_min(2.0 ** -4)
    r = dev / ulp
    off = float((r > 0.5).double().mean())
    exact_req = emul.d == 0
    print('%s vs bf16-rounding emulation: exact %.4f, >1/2 ulp %.5f, max %.3g ulp; derived bound: %.3f of the '
          'outputs must be exact, bound max %.3g ulp, largest deviation / bound %.3g'
          % (name, float((r == 0).double().mean()), off, float(r.max()), float(exact_req.double().mean()),
             float((emul.d / ulp).max()), float((dev / emul.d.clamp_min(1e-30)).max())))
    assert torch.isfinite(got).all()
    assert bool((dev <= emul.d).all()), 'deviation beyond the derived bound at %d elements' % int((dev > emul.d).sum())
    assert off < 5e-3, off


# ---------------------------------------------------------------- the edge-shape cases
def _case(kind, cid, **kw):
    return dict(kind=kind, id=cid, **kw)


def _fwd(cid, n, h, w, c, cout, k, s, p, scale=True, shift=True, res=False, relu=True, crop=False):
    return _case('conv', cid, n=n, h=h, w=w, c=c, cout=cout, k=k, s=s, p=p, scale=scale, shift=shift, res=res,
                 relu=relu, crop=crop)


def forward_cases(key):
    """ops.conv2d_nhwc: windows larger than the image, the generic and row-uniform gathers away
    from the stem, ragged Cout, every epilogue combination."""
    two = key != 'f32'
    out = []
    for n, h, w in [(3, 1, 1), (1, 1, 5), (2, 2, 3)]:
        out.append(_fwd('window>image 3x3 s1 %dx%dx%d' % (n, h, w), n, h, w, 64, 64, 3, 1, 1, res=True))
    for n, h, w in [(1, 2, 2), (2, 5, 4)]:
        out.append(_fwd('window>image 3x3 s2 %dx%dx%d' % (n, h, w), n, h, w, 64, 64, 3, 2, 1, res=True))
    out.append(_fwd('generic C16 3x3 (K 144)', 2, 5, 7, 16, 64, 3, 1, 1, res=True))
    out.append(_fwd('C32 3x3 s2', 2, 7, 5, 32, 64, 3, 2, 1))
    out.append(_fwd('generic C8 5x5', 1, 6, 6, 8, 64, 5, 1, 2))
    cr = 16 if two else 8   # KW * C == BK: one kernel row per K-tile
    out.append(_fwd('row-uniform C%d 4x4 s2' % cr, 2, 6, 8, cr, 64, 4, 2, 1))
    out.append(_fwd('row-uniform C%d 4x4 s1 p2 cropped' % cr, 2, 6, 8, cr, 64, 4, 1, 2, res=True, crop=True))
    for cout in ([8, 24, 72, 136, 200] if two else [4, 12, 68, 132]):
        out.append(_fwd('ragged Cout %d 1x1' % cout, 1, 5, 7, 64, cout, 1, 1, 0, res=True))
    rc = 72 if two else 68
    out.append(_fwd('ragged Cout %d 3x3' % rc, 1, 5, 7, 64, rc, 3, 1, 1, res=True))
    for sc, sh in [(True, True), (False, True), (False, False)]:
        for res in (True, False):
            for relu in (True, False):
                out.append(_fwd('epilogue scale %d shift %d res %d relu %d' % (sc, sh, res, relu), 2, 5, 7, 64, rc,
                                3, 1, 1, scale=sc, shift=sh, res=res, relu=relu))
    return out


# tests/test_gpu_kernels.py::test_every_tile_configuration_matches_torch's ids
TILE_IDS = [0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11, 12, 15, 16, 17, 18, 19, 20, 22, 23, 31, 33, 37, 39]
# bn of the id's tile shape (csrc/conv_igemm.hip kTiles; id & 7 names the shape below 32, 7 / 15 /
# 39 are the eight-wave 128 x 128 tiles)
_TILE_BN = {0: 64, 1: 64, 2: 64, 3: 128, 4: 128, 5: 256, 6: 128, 7: 128}


def tile_bn(tile):
    return 128 if tile in (7, 15, 39) else _TILE_BN[tile & 7]


def tile_ids(key):
    return TILE_IDS + ([t + 32 for t in range(7)] if key != 'f32' else [])


def tile_cases(key):
    """The ragged-Cout geometries of the tile sweep: 72 / 68 for every id, 200 / 132 for ids whose
    tile is 128 or 256 wide."""
    two = key != 'f32'
    return [_fwd('tiles Cout %d' % cout, 1, 5, 7, 64, cout, 3, 1, 1, res=True)
            for cout in ([72, 200] if two else [68, 132])]


def dual_cases(key):
    rc = 72 if key != 'f32' else 68
    out = []
    for c, c2 in [(64, 64), (128, 64)]:
        for cout in (rc, 256):
            for s2 in (1, 2):
                for scale in (True, False):
                    out.append(_case('dual', 'dual C %d C2 %d Cout %d stride2 %d scale %d' % (c, c2, cout, s2, scale),
                                     n=3, h=3, w=5, c=c, c2=c2, cout=cout, s2=s2, scale=scale))
    return out


def deconv_cases(key):
    two = key != 'f32'
    shapes = [(n, h, w, 64, cout) for n, h, w in [(2, 1, 1), (1, 1, 3), (2, 3, 2)]
              for cout in (64, 40, 72 if two else 68)]
    shapes.append((2, 3, 2, 32 if two else 16, 64))   # KW * C == BK with KW = 2: row-uniform
    return [_case('deconv', 'deconv %dx%dx%d C %d Cout %d affine %d' % (n, h, w, c, cout, aff), n=n, h=h, w=w, c=c,
                  cout=cout, affine=aff) for n, h, w, c, cout in shapes for aff in (True, False)]


def head_cases(key):
    return [_case('head', 'head J %d C %d' % (j, c), n=3, h=5, w=7, c=c, j=j) for j in (1, 16, 17, 20)
            for c in (64, 256)]


def gemm_cases(key):
    return [_case('gemm', 'gemm K %d Ncol %d vblk %d' % (k, ncol, vblk), m=70, k=k, ncol=ncol, vblk=vblk)
            for k in (64, 256) for ncol, vblk in [(216, 72), (64, 8), (40, 40)]]


def _dg(cid, h, w, cin, cout, k, s, p, res, inplace=False, n=2):
    return _case('dgrad', cid, n=n, h=h, w=w, cin=cin, cout=cout, k=k, s=s, p=p, res=res, inplace=inplace)


_DGRAD_GRIDS = [(3, 1, 1, 1, 1), (3, 1, 1, 2, 3), (3, 2, 1, 5, 4), (3, 2, 1, 6, 7), (4, 2, 1, 6, 8), (1, 2, 0, 5, 7),
                (1, 2, 0, 6, 4)]   # k, stride, pad, H, W of the input grid


def dgrad_cases(key):
    """T.conv2d_dgrad: small grids x (Cin = dx channels, dy channels) x residual.  dy channels 16 / 32
    at stride 2 reach the generic gather with `up`, 16 at 4x4 / s2 in the 2-byte dtypes row-uniform
    with `up`."""
    two = key != 'f32'
    sm, md, rg = (8, 24, 72) if two else (4, 12, 68)
    pairs = [(64, 64), (sm, 16), (md, 32), (rg, 8), (64, 16), (rg, 32), (sm, 8)]
    return [_dg('dgrad %dx%d s%d p%d %dx%d Cin %d dyC %d res %d' % (k, k, s, p, h, w, cin, cout, res), h, w, cin,
                cout, k, s, p, res) for k, s, p, h, w in _DGRAD_GRIDS for cin, cout in pairs for res in (True, False)]


def inplace_cases(key):
    rg = 72 if key != 'f32' else 68
    return [_dg('in-place 1x1 s2 %dx%d Cin %d dyC %d' % (h, w, cin, cout), h, w, cin, cout, 1, 2, 0, True, True)
            for h, w in [(5, 7), (6, 4)] for cin, cout in [(64, 64), (rg, 16), (rg, 64)]]


def dgrad_tile_cases(key):
    """Ragged Cin under every tile candidate: 3x3, strided 3x3 and 1x1 over a 5 x 7 input grid."""
    return [_dg('dgrad tiles %dx%d s%d Cin %d res %d' % (k, k, s, cin, res), 5, 7, cin, 64, k, s, p, res)
            for cin in (72, 200) for k, s, p in [(3, 1, 1), (3, 2, 1), (1, 1, 0)] for res in (True, False)]


def _wg(cid, n, h, w, c, creal, cout, k, s, p):
    return _case('wgrad', cid, n=n, h=h, w=w, c=c, creal=creal, cout=cout, k=k, s=s, p=p)


def wgrad_cases(key):
    two = key != 'f32'
    out = [_wg('3x3 over a 1x1 image (centre tap only)', 1, 1, 1, 64, 64, 64, 3, 1, 1)]
    for n, h, w in [(1, 1, 1), (1, 1, 3), (1, 3, 11), (1, 5, 13), (3, 1, 43)]:
        out.append(_wg('P %d' % (n * h * w), n, h, w, 16, 16, 64, 3, 1, 1))
    # the launcher's documented split rule (wgrad_split_rule) run here for Cout 136 / 132, K 576
    # (10 tiles): the smallest P whose last split holds one pixel
    rc = 136 if two else 132
    pr = wgrad_ragged_p(wgrad_tiles(rc, 576), WGRAD_BP[key])
    out.append(_wg('P %d: one pixel in the last split' % pr, 1, 1, pr, 64, 64, rc, 3, 1, 1))
    for cout in ([8, 24, 64, 72, 136] if two else [4, 12, 64, 68, 132]):
        out.append(_wg('Cout %d' % cout, 2, 5, 7, 16, 16, cout, 3, 1, 1))
    out.append(_wg('K 8', 2, 5, 7, 8, 8, 64, 1, 1, 0))
    out.append(_wg('K 392 (7x7, C 8, Creal 3)', 2, 9, 8, 8, 3, 64, 7, 2, 3))
    out.append(_wg('K 576', 2, 5, 7, 64, 64, 72 if two else 68, 3, 1, 1))
    out.append(_wg('1x1 C 64 Creal 40', 2, 5, 7, 64, 40, 64, 1, 1, 0))
    sm = 24 if two else 12
    for h, w in [(5, 7), (6, 4)]:
        out.append(_wg('3x3 s2 %dx%d' % (h, w), 2, h, w, 16, 16, sm, 3, 2, 1))
        out.append(_wg('1x1 s2 %dx%d' % (h, w), 2, h, w, 16, 16, sm, 1, 2, 0))
    return out


def deconv_wgrad_cases(key):
    return [_case('dwgrad', 'deconv wgrad %dx%dx%d' % (n, h, w), n=n, h=h, w=w, cin=64, cout=16)
            for n, h, w in [(2, 1, 1), (2, 2, 3)]]


GROUPS = {
    'forward': lambda key: forward_cases(key) + tile_cases(key),
    'dual': dual_cases,
    'deconv': deconv_cases,
    'head / GEMM': lambda key: head_cases(key) + gemm_cases(key),
    'data gradient': lambda key: dgrad_cases(key) + inplace_cases(key) + dgrad_tile_cases(key),
    'weight gradient': lambda key: wgrad_cases(key) + deconv_wgrad_cases(key),
}


# ---------------------------------------------------------------- inputs, emulation, restatement
def out_grid(c):
    """Output grid of a conv case (the crop: one row and one column less than the window allows)."""
    ho = (c['h'] + 2 * c['p'] - c['k']) // c['s'] + 1
    wo = (c['w'] + 2 * c['p'] - c['k']) // c['s'] + 1
    return (ho - 1, wo - 1) if c.get('crop') else (ho, wo)


def make_inputs(c, key, seed=0):
    """Seeded CPU operands of case c as fp64 tensors already rounded to the compute dtype (NCHW
    activations, torch-layout weights); per-channel parameters in f32."""
    dt = DTYPES[key]
    g = torch.Generator().manual_seed(1000 + seed)

    def rn(*shape, scale=1.0):
        return _q(torch.randn(*shape, generator=g).double() * scale, dt)

    def par(n):
        return torch.rand(n, generator=g) + 0.5, torch.randn(n, generator=g) * 0.1

    kind = c['kind']
    i = {}
    if kind == 'conv':
        i['x'] = rn(c['n'], c['c'], c['h'], c['w'])
        i['w'] = rn(c['cout'], c['c'], c['k'], c['k'], scale=(2.0 / (c['c'] * c['k'] ** 2)) ** 0.5)
        sc, sh = par(c['cout'])
        i['scale'], i['shift'] = (sc if c['scale'] else None), (sh if c['shift'] else None)
        i['res'] = rn(c['n'], c['cout'], *out_grid(c)) if c['res'] else None
    elif kind == 'dual':
        h2, w2 = (c['h'] - 1) * c['s2'] + 1, (c['w'] - 1) * c['s2'] + 1
        i['x'] = _q(F.relu(torch.randn(c['n'], c['c'], c['h'], c['w'], generator=g)).double(), dt)
        i['x2'] = rn(c['n'], c['c2'], h2, w2)
        i['w'] = rn(c['cout'], c['c'], 1, 1, scale=0.1)
        i['w2'] = rn(c['cout'], c['c2'], 1, 1, scale=0.1)
        sc, sh = par(c['cout'])
        i['scale'], i['shift'] = (sc if c['scale'] else None), sh
    elif kind == 'deconv':
        i['x'] = rn(c['n'], c['c'], c['h'], c['w'])
        i['w'] = rn(c['c'], c['cout'], 4, 4, scale=(2.0 / (4 * c['c'])) ** 0.5)
        sc, sh = par(c['cout'])
        i['scale'], i['shift'] = (sc, sh) if c['affine'] else (None, None)
    elif kind == 'head':
        i['x'] = rn(c['n'], c['c'], c['h'], c['w'])
        i['w'] = rn(c['j'], c['c'], 1, 1, scale=0.06)
        i['shift'] = torch.randn(c['j'], generator=g)
    elif kind == 'gemm':
        i['x'] = rn(c['m'], c['k'])
        i['w'] = rn(c['ncol'], c['k'], scale=c['k'] ** -0.5)
    elif kind == 'dgrad':
        ho, wo = (c['h'] + 2 * c['p'] - c['k']) // c['s'] + 1, (c['w'] + 2 * c['p'] - c['k']) // c['s'] + 1
        i['dy'] = rn(c['n'], c['cout'], ho, wo)
        i['w'] = rn(c['cout'], c['cin'], c['k'], c['k'], scale=(2.0 / (c['cin'] * c['k'] ** 2)) ** 0.5)
        i['res'] = rn(c['n'], c['cin'], c['h'], c['w']) if c['res'] else None
    elif kind == 'wgrad':
        ho, wo = (c['h'] + 2 * c['p'] - c['k']) // c['s'] + 1, (c['w'] + 2 * c['p'] - c['k']) // c['s'] + 1
        i['x'] = rn(c['n'], c['c'], c['h'], c['w'])   # channels past Creal hold values too: never read out
        i['dy'] = rn(c['n'], c['cout'], ho, wo)
    elif kind == 'dwgrad':
        i['x'] = rn(c['n'], c['cin'], c['h'], c['w'])
        i['dy'] = rn(c['n'], c['cout'], 2 * c['h'], 2 * c['w'])
    else:
        raise ValueError(kind)
    return i


def emulate(c, i, key):
    """The emulated output of case c and its bound, in the layout `to_layout` gives."""
    dt = DTYPES[key]
    kind = c['kind']
    if kind == 'conv':
        res = _E(i['res']) if i['res'] is not None else None
        return _conv([(_E(i['x']), i['w'], c['s'], c['p'])], i['scale'], i['shift'], res, c['relu'], dt,
                     out_grid(c) if c['crop'] else None)
    if kind == 'dual':
        return _conv([(_E(i['x']), i['w'], 1, 0), (_E(i['x2']), i['w2'], c['s2'], 0)], i['scale'], i['shift'], None,
                     True, dt)
    if kind == 'deconv':
        return _conv([(_E(i['x']), i['w'], 2, 1, 'deconv')], i['scale'], i['shift'], None, c['affine'], dt)
    if kind == 'head':
        return _conv([(_E(i['x']), i['w'], 1, 0)], None, i['shift'], None, False, torch.float32, rounds=1)
    if kind == 'gemm':
        x = i['x'].view(c['m'], c['k'], 1, 1)
        e = _conv([(_E(x), i['w'].view(c['ncol'], c['k'], 1, 1), 1, 0)], None, None, None, False, torch.float32,
                  rounds=0)
        rows = lambda t: t.view(c['m'], c['ncol'] // c['vblk'], c['vblk']).permute(1, 0, 2).contiguous()  # noqa: E731
        return _E(rows(e.v), rows(e.d))
    if kind == 'dgrad':
        res = _E(i['res']) if i['res'] is not None else None
        return _dgrad(_E(i['dy']), i['w'], c['s'], c['p'], (c['h'], c['w']), res, dt)
    if kind == 'wgrad':
        return _wgrad(i['dy'], i['x'], (c['cout'], c['creal'], c['k'], c['k']), c['s'], c['p'])
    if kind == 'dwgrad':
        # ConvTranspose2d(4, s2, p1): x plays the output gradient, dy the input of a 4x4 / s2 / p1 conv
        return _wgrad(i['x'], i['dy'], (c['cin'], c['cout'], 4, 4), 2, 1)
    raise ValueError(kind)


def out_dtype(c, key):
    return torch.float32 if c['kind'] in ('head', 'gemm', 'wgrad', 'dwgrad') else DTYPES[key]


def is_nhwc(c):
    return c['kind'] in ('conv', 'dual', 'deconv', 'dgrad')


def to_layout(c, out):
    """A kernel output (device layout) -> fp64 CPU tensor in the emulation's layout."""
    t = out.detach().cpu()
    return (t.float().permute(0, 3, 1, 2) if is_nhwc(c) else t).double().contiguous()


def from_layout(c, ref, key):
    """The inverse: an fp64 tensor in the emulation's layout -> the device layout and dtype."""
    t = ref.permute(0, 2, 3, 1) if is_nhwc(c) else ref
    return t.contiguous().float().to(out_dtype(c, key))


def verify(c, guarded, emul):
    """Guard bands untouched, every element written, every element within its bound."""
    guarded.check()
    return check_bound(c['id'], to_layout(c, guarded.out), emul)


def verify_inplace(c, guarded, emul, res):
    """The in-place 1x1 / s2 data gradient: pixels (2i, 2j) within the bound, every other pixel the
    original residual bit for bit, the guard bands untouched."""
    guarded.check(written=False)
    got = to_layout(c, guarded.out)
    worst = check_bound(c['id'], got[:, :, ::2, ::2], _E(emul.v[:, :, ::2, ::2], emul.d[:, :, ::2, ::2]))
    keep = torch.ones_like(got, dtype=torch.bool)
    keep[:, :, ::2, ::2] = False
    assert torch.equal(got[keep], res[keep]), '%s: %d untouched elements changed' % (
        c['id'], int((got[keep] != res[keep]).sum()))
    return worst


# ---- a plain fp32 statement of each op (torch CPU, its own summation order) and its mutants
def k_tail(c, key):
    """K mod BK of a case whose K axis the kernel pads to whole K-tiles (0: no tail)."""
    kind = c['kind']
    if kind == 'conv':
        return (c['k'] * c['k'] * c['c']) % BK[key]
    if kind == 'dgrad':
        return (c['k'] * c['k'] * c['cout']) % BK[key]
    if kind == 'deconv':
        return (4 * c['c']) % BK[key]
    return 0


_SHIFTED = {'dual': 'x2', 'dgrad': 'dy', 'dwgrad': 'dy'}   # the operand 'xshift' moves ('x' otherwise)


def _shift_extent(c):
    """Extent of the axis 'xshift' rolls: the shifted operand's width (the row GEMM: its rows)."""
    kind = c['kind']
    if kind == 'gemm':
        return c['m']
    if kind == 'dual':
        return (c['w'] - 1) * c['s2'] + 1
    if kind == 'dgrad':
        return (c['w'] + 2 * c['p'] - c['k']) // c['s'] + 1
    return 2 * c['w'] if kind == 'dwgrad' else c['w']


def mutants(c, key):
    """The wrong implementations that apply to case c (the host test: each must fail `verify`)."""
    kind = c['kind']
    m = ['sentinel_channel', 'band']
    if _shift_extent(c) > 1:
        m.append('xshift')
    if kind in ('wgrad', 'dwgrad'):
        return m + ['last_stage']
    m.append('tap')
    # (a 3x3 data gradient over a 1 x 1 grid reads its centre tap only: the K tail multiplies zeros)
    if k_tail(c, key) and not (kind == 'dgrad' and c['h'] * c['w'] == 1):
        m.append('ktail')
    if c.get('res') and (kind == 'dgrad' or c['n'] * math.prod(out_grid(c)) > 1):   # a neighbouring pixel exists
        m.append('resshift')
    if c.get('relu') or kind == 'dual' or (kind == 'deconv' and c['affine']):
        m.append('norelu')
    if (kind in ('conv', 'dual') and c['scale']) or (kind == 'deconv' and c['affine']):
        m.append('scale1')
    if c.get('inplace'):
        m.append('ulp')
    return m


def _zero_tap(w, transposed=False):
    """One window tap zeroed (the centre one; a 1x1 window: its last input channel instead)."""
    w = w.clone()
    kh, kw = w.shape[2], w.shape[3]
    if kh * kw > 1:
        w[:, :, kh // 2, kw // 2] = 0
    elif transposed:
        w[-1] = 0
    else:
        w[:, -1] = 0
    return w


def _drop_k_tail(w, r, order):
    """The last r products of the kernel's K order dropped: `order` permutes w to [rows, kh, kw, ci]."""
    wp = w.permute(*order).clone(memory_format=torch.contiguous_format)
    flat = wp.view(wp.shape[0], -1)
    flat[:, flat.shape[1] - r:] = 0
    inv = [order.index(d) for d in range(4)]
    return wp.permute(*inv).contiguous()


def restate(c, i, key, mutant=None):
    """Case c in torch CPU fp32 on the rounded operands, the result rounded RNE to the output dtype
    (fp64 tensor, emulation layout).  mutant: one of `mutants(c, key)` applied to the computation
    ('sentinel_channel', 'band' and 'ulp' act on the stored buffer: the host test applies them)."""
    kind = c['kind']
    i = dict(i)
    relu = True
    if mutant == 'tap':
        if kind == 'dual':
            i['w2'] = _zero_tap(i['w2'])
        elif kind == 'gemm':
            i['w'] = i['w'].clone()
            i['w'][:, -1] = 0
        else:
            # (a dgrad / deconv weight is [reduced channels][output channels]: a 1x1's last dy channel)
            i['w'] = _zero_tap(i['w'], transposed=kind in ('dgrad', 'deconv'))
    elif mutant == 'ktail':
        r = k_tail(c, key)
        if kind == 'conv':
            i['w'] = _drop_k_tail(i['w'], r, (0, 2, 3, 1))
        elif kind == 'dgrad':
            # the kernel's K order runs over the FLIPPED window, dy channel fastest
            wf = _drop_k_tail(i['w'].flip(2, 3), r, (1, 2, 3, 0))
            i['w'] = wf.flip(2, 3)
        else:
            raise ValueError('no K tail in ' + kind)
    elif mutant == 'xshift':
        name = _SHIFTED.get(kind, 'x')
        i[name] = torch.roll(i[name], 1, dims=0 if kind == 'gemm' else 3)
    elif mutant == 'resshift':
        r = i['res'].permute(1, 0, 2, 3)
        i['res'] = torch.roll(r.reshape(r.shape[0], -1), 1, dims=1).view(r.shape).permute(1, 0, 2, 3)
    elif mutant == 'norelu':
        relu = False
    elif mutant == 'scale1':
        i['scale'] = i['scale'].clone()
        i['scale'][-1] = 1.0
    elif mutant == 'last_stage':
        # the pixels of the last stage of the pixel-major reduction axis never summed
        g = 'dy' if kind == 'wgrad' else 'x'
        t = i[g].permute(1, 0, 2, 3).clone(memory_format=torch.contiguous_format)
        flat = t.view(t.shape[0], -1)
        flat[:, (flat.shape[1] - 1) // WGRAD_BP[key] * WGRAD_BP[key]:] = 0
        i[g] = t.permute(1, 0, 2, 3)
    f = {k: (v.float() if v is not None else None) for k, v in i.items()}
    col = lambda v: v.view(1, -1, 1, 1)   # noqa: E731

    def epilogue(y, act):
        if f.get('scale') is not None:
            y = y * col(f['scale'])
        if f.get('shift') is not None:
            y = y + col(f['shift'])
        if f.get('res') is not None:
            y = y + f['res']
        return F.relu(y) if act and relu else y

    if kind == 'conv':
        y = F.conv2d(f['x'], f['w'], stride=c['s'], padding=c['p'])
        ho, wo = out_grid(c)
        y = epilogue(y[:, :, :ho, :wo], c['relu'])
    elif kind == 'dual':
        y = epilogue(F.conv2d(f['x'], f['w']) + F.conv2d(f['x2'], f['w2'], stride=c['s2']), True)
    elif kind == 'deconv':
        y = epilogue(F.conv_transpose2d(f['x'], f['w'], stride=2, padding=1), c['affine'])
    elif kind == 'head':
        y = F.conv2d(f['x'], f['w'], f['shift'])
    elif kind == 'gemm':
        y = (f['x'] @ f['w'].t()).view(c['m'], c['ncol'] // c['vblk'], c['vblk']).permute(1, 0, 2)
    elif kind == 'dgrad':
        ho, wo = f['dy'].shape[2], f['dy'].shape[3]
        op = (c['h'] - ((ho - 1) * c['s'] - 2 * c['p'] + c['k']), c['w'] - ((wo - 1) * c['s'] - 2 * c['p'] + c['k']))
        y = epilogue(F.conv_transpose2d(f['dy'], f['w'], stride=c['s'], padding=c['p'], output_padding=op), False)
    elif kind == 'wgrad':
        y = torch.nn.grad.conv2d_weight(f['x'][:, :c['creal']].contiguous(), (c['cout'], c['creal'], c['k'], c['k']),
                                        f['dy'], stride=c['s'], padding=c['p'])
    elif kind == 'dwgrad':
        y = torch.nn.grad.conv2d_weight(f['dy'], (c['cin'], c['cout'], 4, 4), f['x'], stride=2, padding=1)
    else:
        raise ValueError(kind)
    return _q(y.double(), out_dtype(c, key)).contiguous()
