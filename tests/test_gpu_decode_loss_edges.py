"""Edge shapes of the small kernels around the network (csrc/heatmap.hip, csrc/datapath.hip and the
epipolar / affine parts of csrc/geometry.hip) against plain float64 restatements on the CPU: maps
with H != W, the scalar fallbacks of the float4 paths, views whose storage is not 16-byte aligned,
partial waves and blocks, the second trip of the grid-stride loops, every view count's pair
enumeration and the Gaussian-target truncation rules (tests/golden/datapath_edges.npz, recorded from
the reference by tests/golden/make_datapath_golden.py edges).

Tolerances.  Identical fp32 operations are compared exactly (arg-max, flip_back, target weights,
zero gradients, misaligned against aligned).  Every other bound is 8 x the deviation of the
project's fp32 CPU oracle (G.softargmax2d, G.joints_mse, G.fundamental_loss with torch fp32 autograd)
from the float64 reference on the test's own inputs, the largest over the case's shapes, taken
relative to max|reference| (the factor covers the kernels' fixed but different summation order and
__expf); it is computed when the test runs and never replaces the older golden tests' bounds, which
are asserted as well.  The deviations measured on the CPU that wrote this file stand next to each
bound.

Not reached here: the 64-bit index branch of mse_bwd_kernel (it needs 2^31 elements), NaN / inf
inputs, and V > 4 for RANSAC and reprojection."""
import functools
import itertools
import math

import numpy as np
import pytest
import torch

from oracle import geometry_ref as G
from posu import datapath, ops, synthetic as syn
from tests.golden.make_datapath_golden import EDGE_CASES

pytestmark = pytest.mark.gpu

# (N, J, H, W)
SHAPES = [(3, 5, 16, 12),    # vector path, H > W
          (2, 3, 7, 9),      # HW = 63 < 64, W odd: scalar path, idle lanes
          (1, 5, 5, 6),      # HW = 30, NJ = 5: partial block
          (3, 7, 24, 18),    # W % 4 != 0 but HW % 4 == 0: must take the scalar path
          (2, 3, 13, 10),    # HW % 4 != 0
          (2, 4, 12, 20)]    # vector path, W > H
BIG = (9, 16, 128, 128)      # 2,359,296 elements: the second trip of the 8192 x 256 grid-stride loops
MPII_FLIP_PAIRS = [[0, 5], [1, 4], [2, 3], [10, 15], [11, 14], [12, 13]]


def _ids(shapes):
    return ['x'.join(str(v) for v in s) for s in shapes]


def _peaked(n, j, h, w, seed):
    """tests/golden/make_golden.py peaked_heatmaps: a sigma-2 Gaussian on 0.02 noise per map."""
    r = np.random.default_rng(seed)
    hm = 0.02 * r.standard_normal((n, j, h, w)).astype(np.float32)
    ys, xs = np.mgrid[0:h, 0:w]
    for a in range(n):
        for b in range(j):
            cy, cx = r.uniform(2, h - 3), r.uniform(2, w - 3)
            hm[a, b] += np.exp(-((ys - cy) ** 2 + (xs - cx) ** 2) / (2 * 2.0 ** 2)).astype(np.float32)
    return hm


def _rel_dev(oracle, ref):
    """max|oracle - ref| / max|ref| of two CPU tensors / arrays."""
    oracle, ref = np.asarray(oracle, dtype=np.float64), np.asarray(ref, dtype=np.float64)
    return float(np.abs(oracle - ref).max() / np.abs(ref).max())


def _check(what, got, ref, dev, old_atol=None, old_rtol=0.0):
    """got within 8 x dev x max|ref| of ref (dev: the fp32 oracle's own relative deviation), and
    within the older golden test's bound when there is one.  Prints the figures first."""
    got, ref = np.asarray(got, dtype=np.float64), np.asarray(ref, dtype=np.float64)
    scale = float(np.abs(ref).max())
    err = float(np.abs(got - ref).max())
    bound = 8.0 * dev * scale
    print('%s: kernel err %.3g, bound %.3g (8 x oracle dev %.3g x max|ref| %.3g), ratio %.2f'
          % (what, err, bound, dev, scale, err / bound if bound > 0 else float('inf')))
    if old_atol is not None:
        np.testing.assert_allclose(got, ref, atol=old_atol, rtol=old_rtol, err_msg=what + ' (the older bound)')
    assert err <= bound, '%s: err %.3g > 8 x the fp32 oracle deviation = %.3g' % (what, err, bound)


# ------------------------------------------------------------------------------ soft-argmax
def _softargmax(hm, beta, T=None):
    """Softmax expectation in hm's dtype (G.softargmax2d's operations with beta for its 100), then
    the per-sample affine [x, y, 1] @ T^T."""
    n, j, h, w = hm.shape
    p = torch.softmax((hm * beta).reshape(n, j, -1), dim=-1).reshape(n, j, h, w)
    xs = torch.sum(p.sum(dim=2) * torch.arange(w, dtype=hm.dtype).view(1, 1, -1), dim=2)
    ys = torch.sum(p.sum(dim=3) * torch.arange(h, dtype=hm.dtype).view(1, 1, -1), dim=2)
    out = torch.stack([xs, ys], dim=2)
    if T is not None:
        out = torch.einsum('njc,nkc->njk', torch.cat([out, torch.ones(n, j, 1, dtype=hm.dtype)], 2), T.to(hm.dtype))
    return out


def _softargmax_oracle32(hm, beta, T=None):
    """The fp32 oracle: G.softargmax2d where it applies (beta = 100), its restatement with another
    beta otherwise; the affine as test_softargmax_backward_matches_autograd applies it."""
    n, j = hm.shape[:2]
    out = G.softargmax2d(hm) if beta == 100.0 else _softargmax(hm, beta)
    if T is not None:
        out = torch.einsum('njc,nkc->njk', torch.cat([out, torch.ones(n, j, 1)], 2), T)
    return out


@functools.lru_cache(maxsize=None)
def _sa_inputs(shape):
    """Peaked maps; map [0, 0]: the peak in the last row and last column (a row / column swap
    cannot cancel); [0, 1]: constant; [0, 2] and the whole last sample (N > 1): flat low contrast."""
    n, j, h, w = shape
    seed = 1000 + 100 * h + w
    r = np.random.default_rng(seed)
    hm = _peaked(n, j, h, w, seed)
    hm[0, 0] = 0.02 * r.standard_normal((h, w))
    hm[0, 0, h - 1, w - 1] += 1.0
    hm[0, 1] = 0.37
    hm[0, 2] = 0.03 * r.standard_normal((h, w))
    if n > 1:
        hm[n - 1] = 0.03 * r.standard_normal((j, h, w))
    T = r.uniform(-2, 2, size=(n, 2, 3)).astype(np.float32)
    gout = r.standard_normal((n, j, 2)).astype(np.float32)
    return torch.from_numpy(hm), torch.from_numpy(T), torch.from_numpy(gout)


@functools.lru_cache(maxsize=None)
def _sa_fwd_dev(beta, affine):
    """The fp32 oracle's deviation from float64 over the shape set.  Measured: beta 100 1.6e-07 plain and
    2.9e-07 after the affine, beta 1 2.0e-07 and 2.0e-07, all relative to max|ref| (23, 51, 12 and 26 px);
    in pixels at most 3.6e-06 plain (24x18) and 7.4e-06 after the affine.  The bounds run from 4e-06 px
    (5x6, beta 1) to 1.2e-04 px (12x20 after the affine), against the golden test's 2e-4 and 5e-3 px."""
    devs = []
    for shape in SHAPES:
        hm, T, _ = _sa_inputs(shape)
        T = T if affine else None
        devs.append(_rel_dev(_softargmax_oracle32(hm, beta, T), _softargmax(hm.double(), beta, T)))
    return max(devs)


@pytest.mark.parametrize('affine', [False, True], ids=['plain', 'affine'])
@pytest.mark.parametrize('beta', [100.0, 1.0])
@pytest.mark.parametrize('shape', SHAPES, ids=_ids(SHAPES))
def test_softargmax_forward_matches_fp64(cuda, shape, beta, affine):
    hm, T, _ = _sa_inputs(shape)
    T = T if affine else None
    ref = _softargmax(hm.double(), beta, T)
    got = ops.softargmax2d(hm.to(cuda), beta=beta, affine=None if T is None else T.to(cuda)).cpu()
    dev = _sa_fwd_dev(beta, affine)
    _check('softargmax fwd %s beta %g affine %d' % (shape, beta, affine), got, ref, dev,
           old_atol=5e-3 if affine else 2e-4)
    if not affine:
        h, w = shape[2:]
        centre = np.array([(w - 1) / 2.0, (h - 1) / 2.0])
        assert np.abs(got[0, 1].double().numpy() - centre).max() <= 8.0 * dev * float(ref.abs().max())
        if beta == 100.0:   # the corner peak decodes next to (W - 1, H - 1)
            assert np.abs(got[0, 0].double().numpy() - np.array([w - 1.0, h - 1.0])).max() < 0.5


@functools.lru_cache(maxsize=None)
def _sa_bwd_refs(shape):
    hm, T, gout = _sa_inputs(shape)
    a = hm.double().requires_grad_(True)
    (_softargmax(a, 100.0, T) * gout.double()).sum().backward()
    b = hm.clone().requires_grad_(True)
    (_softargmax_oracle32(b, 100.0, T) * gout).sum().backward()
    return a.grad, b.grad


@functools.lru_cache(maxsize=None)
def _sa_bwd_dev():
    """fp32 autograd of G.softargmax2d against float64 autograd.  Measured: 1.3e-06 of max|grad| (the
    largest gradient entry is 393) over the shape set."""
    return max(_rel_dev(b, a) for a, b in (_sa_bwd_refs(s) for s in SHAPES))


@pytest.mark.parametrize('shape', SHAPES, ids=_ids(SHAPES))
def test_softargmax_backward_matches_fp64_autograd(cuda, shape):
    """Every shape: the float4 store loop (16x12, 12x20) and the scalar one (the rest)."""
    hm, T, gout = _sa_inputs(shape)
    ref, _ = _sa_bwd_refs(shape)
    b = hm.to(cuda).requires_grad_(True)
    (ops.softargmax2d(b, beta=100.0, affine=T.to(cuda)) * gout.to(cuda)).sum().backward()
    _check('softargmax bwd %s' % (shape,), b.grad.cpu(), ref, _sa_bwd_dev(), old_atol=1e-4, old_rtol=1e-3)


def _offset_view(t, k, cuda):
    """t's values in a contiguous cuda view whose storage starts k floats into a 16-B aligned buffer."""
    buf = torch.zeros(t.numel() + 4, dtype=torch.float32, device=cuda)
    assert buf.data_ptr() % 16 == 0
    view = buf[k:k + t.numel()].view(t.shape)
    view.copy_(t)
    assert view.is_contiguous() and view.data_ptr() % 16 == 4 * k
    return view


@pytest.mark.parametrize('k', [1, 2, 3])
def test_softargmax_and_mse_on_a_misaligned_view_equal_the_aligned_call(cuda, k):
    """A contiguous view keeps its storage offset through .contiguous(): the kernels must not take
    16-B loads from it, and must give the very bits they give on an aligned copy."""
    shape = SHAPES[0]
    hm, T, gout = _sa_inputs(shape)
    T, gout = T.to(cuda), gout.to(cuda)
    for affine in (None, T):
        a = hm.to(cuda).requires_grad_(True)
        b = _offset_view(hm, k, cuda).requires_grad_(True)
        oa, ob = ops.softargmax2d(a, affine=affine), ops.softargmax2d(b, affine=affine)
        assert torch.equal(oa, ob)
        (oa * gout).sum().backward()
        (ob * gout).sum().backward()
        assert torch.equal(a.grad, b.grad)
    r = np.random.default_rng(50 + k)
    pred = torch.from_numpy(r.standard_normal(shape).astype(np.float32))
    gt = torch.from_numpy(r.standard_normal(shape).astype(np.float32))
    w = torch.from_numpy(r.uniform(size=shape[:2] + (1,)).astype(np.float32)).to(cuda)
    for wt in (w, None):
        for gt_k in (k, 0):   # both maps off the boundary, and the prediction alone
            a = pred.to(cuda).requires_grad_(True)
            b = _offset_view(pred, k, cuda).requires_grad_(True)
            la, lb = ops.joints_mse(a, gt.to(cuda), wt), ops.joints_mse(b, _offset_view(gt, gt_k, cuda), wt)
            assert torch.equal(la, lb)
            la.backward()
            lb.backward()
            assert torch.equal(a.grad, b.grad)


# ---------------------------------------------------------------------------------- arg-max
def _planted_maps(h, w, seed):
    """The maps the decode can get wrong, each [h, w] f32."""
    r = np.random.default_rng(seed)
    hw = h * w
    maps = [-1.0 - np.abs(r.standard_normal((h, w))),        # all negative: coordinates zeroed
            np.zeros((h, w))]                                 # all zero: max 0 is not > 0
    ties = [(3, 10)]                                          # two lanes of the first trip
    if hw > 67:
        ties += [(10, 67),                                    # the first index in a higher lane than the second
                 (5, 69)]                                     # the same lane, 64 apart
    for i0, i1 in ties:
        m = 0.1 * r.uniform(size=hw)
        m[i0] = m[i1] = 2.0
        maps.append(m.reshape(h, w))
    for py, px in ((0, w - 1), (h - 1, 0), (1, 1), (h - 2, w - 2), (2, 2)):   # strict 1 < p < size - 1, per axis
        m = 0.1 * r.uniform(size=(h, w))
        m[py, px] = 1.0
        maps.append(m)
    py, px = h - 3, w - 3                                     # an interior peak for every shape of the set
    for horizontal in (True, False):                          # dx == 0 with dy != 0, then the reverse
        m = np.zeros((h, w))
        m[py, px] = 1.0
        m[py, px - 1], m[py, px + 1] = (0.5, 0.5) if horizontal else (0.25, 0.5)
        m[py - 1, px], m[py + 1, px] = (0.5, 0.25) if horizontal else (0.5, 0.5)
        maps.append(m)
    return [np.asarray(m, dtype=np.float32) for m in maps]


@functools.lru_cache(maxsize=None)
def _argmax_batches(shape):
    """The planted maps in as many [N, J, H, W] batches as they need, peaked maps in the free slots."""
    n, j, h, w = shape
    planted = _planted_maps(h, w, seed=7 * h + w)
    out = []
    for k in range(0, len(planted), n * j):
        hm = _peaked(n, j, h, w, seed=300 + k + h).reshape(n * j, h, w)
        part = planted[k:k + n * j]
        hm[:len(part)] = np.stack(part)
        out.append(hm.reshape(n, j, h, w))
    return out


def _post_process(hm, coords):
    """get_final_preds' quarter-pixel shift (oracle.geometry_ref.get_final_preds before its affine)."""
    coords = coords.copy()
    h, w = hm.shape[2:]
    for n in range(hm.shape[0]):
        for p in range(hm.shape[1]):
            m = hm[n][p]
            px = int(math.floor(coords[n][p][0] + 0.5))
            py = int(math.floor(coords[n][p][1] + 0.5))
            if 1 < px < w - 1 and 1 < py < h - 1:
                diff = np.array([m[py][px + 1] - m[py][px - 1], m[py + 1][px] - m[py - 1][px]])
                coords[n][p] += np.sign(diff) * .25
    return coords


@pytest.mark.parametrize('post', [False, True], ids=['nopost', 'post'])
@pytest.mark.parametrize('shape', SHAPES, ids=_ids(SHAPES))
def test_argmax_decode_matches_get_final_preds(cuda, shape, post):
    n, _, h, w = shape
    r = np.random.default_rng(6)
    centers, scales = r.uniform(300, 700, size=(n, 2)), r.uniform(3.5, 6.0, size=(n, 2))
    T = np.stack([G.crop_affine(centers[i], scales[i], [w, h]) for i in range(n)])
    for hm in _argmax_batches(shape):
        coords, maxvals = G.get_max_preds(hm)
        if post:
            coords = _post_process(hm, coords)
        d = torch.from_numpy(hm).to(cuda)
        p, v = ops.argmax2d(d, post_process=post)
        np.testing.assert_array_equal(p.cpu().numpy(), coords)
        np.testing.assert_array_equal(v.cpu().numpy(), maxvals)
        pa, va = ops.argmax2d(d, post_process=post, affine64=torch.from_numpy(T).to(cuda))
        final, _ = G.get_final_preds(hm, centers, scales, post_process=post)
        np.testing.assert_allclose(pa.cpu().numpy(), final, atol=1e-4, rtol=0)
        np.testing.assert_array_equal(va.cpu().numpy(), maxvals)


# ------------------------------------------------------------------------- integral decode
def _integral(hm):
    """run/test/test_integral.py:63-70 as tests/golden/make_datapath_golden.py restates it, in hm's dtype."""
    h, w = hm.shape[2:]
    hn = hm / np.sum(hm, axis=(2, 3), keepdims=True)
    accu_w = np.sum(hn, axis=2)
    accu_h = np.sum(hn, axis=3)
    return np.stack((np.sum(accu_w * np.arange(w).reshape((1, 1, w)), axis=2),
                     np.sum(accu_h * np.arange(h).reshape((1, 1, h)), axis=2)), axis=2)


@functools.lru_cache(maxsize=None)
def _integral_inputs(shape):
    return np.abs(np.random.default_rng(sum(shape)).standard_normal(shape)).astype(np.float32)


@functools.lru_cache(maxsize=None)
def _integral_dev():
    """The restatement on the f32 maps (what the golden recorded) against float64.  Measured: 1.7e-07 of
    max|ref| (12.0 px) over the shape set."""
    return max(_rel_dev(_integral(_integral_inputs(s)), _integral(_integral_inputs(s).astype(np.float64)))
               for s in SHAPES)


@pytest.mark.parametrize('shape', SHAPES, ids=_ids(SHAPES))
def test_integral_decode_matches_fp64(cuda, shape):
    hm = _integral_inputs(shape)
    got = datapath.integral_preds(torch.from_numpy(hm).to(cuda)).cpu().numpy()
    _check('integral %s' % (shape,), got, _integral(hm.astype(np.float64)), _integral_dev(),
           old_atol=1e-4, old_rtol=1e-5)


# -------------------------------------------------------------------------------- affine2d
def _affine(pts, T):
    return torch.einsum('njc,nkc->njk', torch.cat([pts, torch.ones_like(pts[..., :1])], 2), T)


@functools.lru_cache(maxsize=None)
def _affine_refs(nj):
    """(inputs, float64 value and gradient, fp32 autograd value and gradient)."""
    n, j = nj
    r = np.random.default_rng(n * 100 + j)
    pts = torch.from_numpy(r.uniform(0, 64, size=(n, j, 2)).astype(np.float32))
    T = torch.from_numpy(r.uniform(-2, 2, size=(n, 2, 3)).astype(np.float32))
    g = torch.from_numpy(r.standard_normal((n, j, 2)).astype(np.float32))
    out = []
    for dt in (torch.float64, torch.float32):
        a = pts.to(dt).clone().requires_grad_(True)
        o = _affine(a, T.to(dt))
        (o * g.to(dt)).sum().backward()
        out.append((o.detach(), a.grad))
    return (pts, T, g), out[0], out[1]


AFFINE_NJ = [(3, 5), (40, 17)]    # 15 points; 680: above one 256-thread block and no multiple of it


@functools.lru_cache(maxsize=None)
def _affine_dev():
    """Measured: value 9.3e-08 of max|ref| (about 220), gradient 5.7e-08 of max|grad| (about 7.8)."""
    vals = [_affine_refs(nj) for nj in AFFINE_NJ]
    return max(_rel_dev(v[2][0], v[1][0]) for v in vals), max(_rel_dev(v[2][1], v[1][1]) for v in vals)


@pytest.mark.parametrize('nj', AFFINE_NJ, ids=['3x5', '40x17'])
def test_affine2d_forward_and_backward_match_fp64_autograd(cuda, nj):
    (pts, T, g), (ref, gref), _ = _affine_refs(nj)
    a = pts.to(cuda).requires_grad_(True)
    out = ops.affine2d(a, T.to(cuda))
    (out * g.to(cuda)).sum().backward()
    dev_o, dev_g = _affine_dev()
    _check('affine2d fwd %s' % (nj,), out.detach().cpu(), ref, dev_o, old_atol=5e-3)
    _check('affine2d bwd (transpose) %s' % (nj,), a.grad.cpu(), gref, dev_g)


# ------------------------------------------------------------------------------- flip_back
def _flip_back(hf, perm, hm, shift):
    """Mirror W, out joint j from flipped joint perm[j], the optional one-column shift with column 0
    duplicated (function.py:579-582), the optional average; float32 as the kernel."""
    f = hf if perm is None else hf[:, perm]
    f = f[..., ::-1].copy()
    if shift:
        s = f.copy()
        s[..., 1:] = f[..., :-1]
        f = s
    return f if hm is None else (hm + f) * np.float32(0.5)


FLIP_CASES = [((2, 6, 5, 9), [1, 0, 2, 5, 4, 3]), ((3, 4, 12, 7), [0, 3, 2, 1])]   # some pairs swapped, some fixed


@pytest.mark.parametrize('shift', [False, True], ids=['noshift', 'shift'])
@pytest.mark.parametrize('shape,perm', FLIP_CASES, ids=_ids([c[0] for c in FLIP_CASES]))
def test_flip_back_bit_exact(cuda, shape, perm, shift):
    r = np.random.default_rng(sum(shape))
    hf, hm = r.standard_normal(shape).astype(np.float32), r.standard_normal(shape).astype(np.float32)
    for use_perm, use_hm in itertools.product((False, True), repeat=2):
        got = ops.flip_back(torch.from_numpy(hf).to(cuda), perm=perm if use_perm else None,
                            hm=torch.from_numpy(hm).to(cuda) if use_hm else None, shift=shift)
        ref = _flip_back(hf, perm if use_perm else None, hm if use_hm else None, shift)
        np.testing.assert_array_equal(got.cpu().numpy(), ref)


def test_flip_back_grid_stride(cuda):
    r = np.random.default_rng(31)
    hf, hm = r.standard_normal(BIG).astype(np.float32), r.standard_normal(BIG).astype(np.float32)
    perm = list(range(16))
    for a, b in MPII_FLIP_PAIRS:
        perm[a], perm[b] = b, a
    got = ops.flip_back(torch.from_numpy(hf).to(cuda), perm=perm, hm=torch.from_numpy(hm).to(cuda), shift=True)
    np.testing.assert_array_equal(got.cpu().numpy(), _flip_back(hf, perm, hm, True))


# ------------------------------------------------------------------------------- JointsMSE
MSE_HW = [(5, 6), (7, 9), (16, 12), (24, 18)]     # HW 30, 63 (scalar loop), 192, 432 (16-B loads)
MSE_NJ = [(2, 3), (20, 17)]                       # NJ = 340 > 256: the loop of mse_final_kernel


@functools.lru_cache(maxsize=None)
def _mse_refs(shape, weighted):
    """(inputs, float64 loss and gradient, G.joints_mse fp32 loss and gradient)."""
    n, j = shape[:2]
    r = np.random.default_rng(sum(shape) + 1000 * weighted)
    pred = torch.from_numpy(r.standard_normal(shape).astype(np.float32))
    gt = torch.from_numpy(r.standard_normal(shape).astype(np.float32))
    w = None
    if weighted:
        w = r.uniform(size=(n, j, 1)).astype(np.float32)
        w[:, 1] = 0.0          # a joint without a label anywhere
        w[0, 0] = 0.0
        w = torch.from_numpy(w)
    out = []
    for dt in (torch.float64, torch.float32):
        a = pred.to(dt).clone().requires_grad_(True)
        loss = G.joints_mse(a, gt.to(dt), None if w is None else w.to(dt))
        loss.backward()
        out.append((loss.detach(), a.grad))
    return (pred, gt, w), out[0], out[1]


@functools.lru_cache(maxsize=None)
def _mse_dev(shapes, weighted):
    """Measured over the small shapes: loss 1.0e-07 (weighted) and 5.5e-08 of the loss, gradient 1.3e-07
    and 1.2e-07 of max|grad|; at the grid-stride shape the gradient 1.1e-07."""
    vals = [_mse_refs(s, weighted) for s in shapes]
    return max(_rel_dev(v[2][0], v[1][0]) for v in vals), max(_rel_dev(v[2][1], v[1][1]) for v in vals)


MSE_SHAPES = tuple(nj + hw for nj in MSE_NJ for hw in MSE_HW)


@pytest.mark.parametrize('weighted', [True, False], ids=['w', 'nw'])
@pytest.mark.parametrize('shape', MSE_SHAPES, ids=_ids(MSE_SHAPES))
def test_joints_mse_forward_and_backward_match_fp64(cuda, shape, weighted):
    (pred, gt, w), (loss_ref, grad_ref), _ = _mse_refs(shape, weighted)
    a = pred.to(cuda).requires_grad_(True)
    loss = ops.joints_mse(a, gt.to(cuda), None if w is None else w.to(cuda))
    loss.backward()
    dev_l, dev_g = _mse_dev(MSE_SHAPES, weighted)
    _check('joints_mse loss %s w %d' % (shape, weighted), loss.detach().cpu(), loss_ref, dev_l,
           old_atol=0.0, old_rtol=1e-5)
    grad = a.grad.cpu()
    _check('joints_mse grad %s w %d' % (shape, weighted), grad, grad_ref, dev_g)
    if weighted:
        assert not grad[:, 1].any() and not grad[0, 0].any()    # weight 0: the gradient is exactly 0


def test_joints_mse_backward_grid_stride(cuda):
    # the 64-bit index branch of mse_bwd_kernel needs N * J * HW >= 2^31 elements (8 GiB per tensor): left out
    (pred, gt, w), (_, grad_ref), _ = _mse_refs(BIG, True)
    a = pred.to(cuda).requires_grad_(True)
    ops.joints_mse(a, gt.to(cuda), w.to(cuda)).backward()
    grad = a.grad.cpu()
    _check('joints_mse grad %s' % (BIG,), grad, grad_ref, _mse_dev((BIG,), True)[1])
    assert not grad[:, 1].any() and not grad[0, 0].any()


# -------------------------------------------------------------------------------- epipolar
def _epipolar(x, w, F, subj):
    """FundamentalLoss.__call__ (lib/core/loss.py:101-133) in x's dtype: pairs in
    itertools.permutations order, |h_j^T F h_i|, weights w_i * w_j, mean over N * P * J.
    x [V, N, J, 2], w [V, N, J] or None, F [S, P, 3, 3] -> (loss, residuals [N, P, J])."""
    v, n, j, _ = x.shape
    pairs = list(itertools.permutations(range(v), 2))
    homo = torch.cat([x, torch.ones(v, n, j, 1, dtype=x.dtype)], dim=3)
    resid = []
    for b in range(n):
        row = []
        for p, (pi, pj) in enumerate(pairs):
            r = torch.abs(torch.sum(torch.mm(homo[pj][b], F[int(subj[b]), p]) * homo[pi][b], dim=1))
            if w is not None:
                r = r * (w[pj][b] * w[pi][b])
            row.append(r)
        resid.append(torch.stack(row))
    resid = torch.stack(resid)
    return resid.sum() / (n * len(pairs) * j), resid


EPI_CASES = tuple((v, nj) for v in (2, 3, 4) for nj in ((1, 3), (5, 16)))   # N * P * J: 6 ... 960


@functools.lru_cache(maxsize=None)
def _epi_refs(v, nj, weighted):
    n, j = nj
    s, p = 3, v * (v - 1)
    r = np.random.default_rng(1000 * v + 10 * n + weighted)
    x = torch.from_numpy(r.uniform(100, 900, size=(v, n, j, 2)).astype(np.float32))
    w = torch.from_numpy((r.uniform(size=(v, n, j)) > 0.2).astype(np.float32)) if weighted else None
    scale = np.abs(np.stack(list(syn.fundamental_dict().values()))).mean(axis=0)   # the magnitude per entry
    F = (r.standard_normal((s, p, 3, 3)) * scale).astype(np.float32)
    F[0] = 0.0                                  # subject 0: every residual and gradient exactly 0
    F = torch.from_numpy(F)
    subj = np.array([2, 0, 1, 0, 2][:n] if n > 1 else [2], dtype=np.int32)   # all three, not sorted
    a = x.double().requires_grad_(True)
    loss64, resid64 = _epipolar(a, None if w is None else w.double(), F.double(), subj)
    loss64.backward()
    # the fp32 oracle: G.fundamental_loss with torch fp32 autograd (per element: the restatement in fp32)
    joints = [x[k].clone().requires_grad_(True) for k in range(v)]
    F_dict = {(int(sb), pi, pj): F[sb, q].numpy() for sb in range(s)
              for q, (pi, pj) in enumerate(itertools.permutations(range(v), 2))}
    weights = [(w[k] if weighted else torch.ones(n, j)).unsqueeze(2) for k in range(v)]
    loss32 = G.fundamental_loss(joints, weights, subj, F_dict, use_target_weight=weighted)
    loss32.backward()
    grad32 = torch.stack([t.grad for t in joints])
    resid32 = _epipolar(x, w, F, subj)[1]
    return (x, w, F, subj), (loss64.detach(), resid64.detach(), a.grad), (loss32.detach(), resid32, grad32)


@functools.lru_cache(maxsize=None)
def _epi_dev(weighted):
    """Measured over the six cases, weighted / unweighted: loss 8.2e-08 / 1.0e-07 of the loss, residuals
    8.5e-08 / 1.4e-07 of the largest residual, gradient 9.5e-08 / 1.3e-07 of max|grad|."""
    vals = [_epi_refs(v, nj, weighted) for v, nj in EPI_CASES]
    return tuple(max(_rel_dev(c[2][k], c[1][k]) for c in vals) for k in range(3))


@pytest.mark.parametrize('weighted', [True, False], ids=['w', 'nw'])
@pytest.mark.parametrize('v,nj', EPI_CASES, ids=['V%d-%dx%d' % (v, nj[0], nj[1]) for v, nj in EPI_CASES])
def test_epipolar_loss_residuals_and_gradient_match_fp64(cuda, v, nj, weighted):
    (x, w, F, subj), (loss_ref, resid_ref, grad_ref), _ = _epi_refs(v, nj, weighted)
    dev_l, dev_r, dev_g = _epi_dev(weighted)
    wd = None if w is None else w.to(cuda)
    Fd, sd = F.to(cuda), torch.from_numpy(subj).to(cuda)
    a = x.to(cuda).requires_grad_(True)
    loss = ops.epipolar_loss(a, wd, Fd, sd)
    loss.backward()
    resid, loss2 = ops.epipolar_residuals(x.to(cuda), wd, Fd, sd)
    what = 'epipolar V %d N x J %s w %d' % (v, nj, weighted)
    _check(what + ' loss', loss.detach().cpu(), loss_ref, dev_l, old_atol=0.0, old_rtol=1e-5)
    _check(what + ' residuals', resid.cpu(), resid_ref, dev_r)
    _check(what + ' gradient', a.grad.cpu(), grad_ref, dev_g)
    assert torch.equal(loss2, loss.detach())
    zero = torch.from_numpy(subj == 0)
    assert not resid.cpu()[zero].any()              # F = 0: the residuals are exactly 0 ...
    assert not a.grad.cpu()[:, zero].any()          # ... and so is the gradient (sign(0) = 0, as torch.abs)


# ------------------------------------------------------------------------ Gaussian targets
def _painted_boxes(t):
    """Per map the bounding box (x0, x1, y0, y1) of its positive pixels, -1s for an empty map."""
    n, j = t.shape[:2]
    out = np.full((n, j, 4), -1, dtype=np.int64)
    for a in range(n):
        for b in range(j):
            ys, xs = np.nonzero(t[a, b] > 0)
            if len(ys):
                out[a, b] = [xs.min(), xs.max(), ys.min(), ys.max()]
    return out


@pytest.mark.parametrize('case', range(len(EDGE_CASES)),
                         ids=['%dx%d-to-%dx%d-sigma%g' % (i + h + (s,)) for i, h, s in EDGE_CASES])
def test_gaussian_targets_match_reference_at_the_edges(cuda, golden, case):
    g = golden('datapath_edges.npz')
    image, heatmap, sigma = EDGE_CASES[case]
    want_t, want_w = g['targets_%d' % case], g['weights_%d' % case]
    t, w = datapath.generate_heatmaps(torch.from_numpy(g['joints_%d' % case]).to(cuda),
                                      torch.from_numpy(g['vis_%d' % case]).to(cuda), image, heatmap, sigma=sigma)
    t, w = t.cpu().numpy(), w.cpu().numpy()
    np.testing.assert_array_equal(w, want_w)
    np.testing.assert_allclose(t, want_t, rtol=1e-6, atol=1e-7)
    assert (t > 0).sum() == (want_t > 0).sum()
    np.testing.assert_array_equal(_painted_boxes(t), _painted_boxes(want_t))


def _gaussian_targets(joints, vis, image, heatmap, sigma):
    """generate_heatmap (lib/dataset/joints_dataset_compatible.py:215-253) for a batch in float64;
    Python's int() is np.trunc."""
    n, j = vis.shape
    hw, hh = heatmap
    tmp = 3.0 * sigma
    mu_x = np.trunc(joints[..., 0].astype(np.float64) / (image[0] / hw) + 0.5)
    mu_y = np.trunc(joints[..., 1].astype(np.float64) / (image[1] / hh) + 0.5)
    ul_x, ul_y = np.trunc(mu_x - tmp), np.trunc(mu_y - tmp)
    br_x, br_y = np.trunc(mu_x + tmp + 1), np.trunc(mu_y + tmp + 1)
    outside = (ul_x >= hw) | (ul_y >= hh) | (br_x < 0) | (br_y < 0)
    weight = np.where(outside, 0.0, vis).astype(np.float32)
    c0 = (2 * tmp + 1) // 2
    xs = np.arange(hw).reshape(1, 1, 1, hw)
    ys = np.arange(hh).reshape(1, 1, hh, 1)
    ux, uy, bx, by = (a.reshape(n, j, 1, 1) for a in (ul_x, ul_y, br_x, br_y))
    g = np.exp(-((xs - ux - c0) ** 2 + (ys - uy - c0) ** 2) / (2.0 * sigma ** 2))
    paint = (weight.reshape(n, j, 1, 1) > 0.5) & (xs >= ux) & (xs < bx) & (ys >= uy) & (ys < by)
    return np.where(paint, g, 0.0), weight.reshape(n, j, 1)


def test_gaussian_targets_grid_stride(cuda):
    n, j = BIG[:2]
    r = np.random.default_rng(41)
    joints = (r.uniform(-0.1, 1.1, size=(n, j, 2)) * 512).astype(np.float32)
    vis = r.choice(np.array([0.0, 1.0, 1.0, 1.0, 0.5], dtype=np.float32), size=(n, j))
    want_t, want_w = _gaussian_targets(joints, vis, (512, 512), (128, 128), 2)
    t, w = datapath.generate_heatmaps(torch.from_numpy(joints).to(cuda), torch.from_numpy(vis).to(cuda),
                                      (512, 512), (128, 128), sigma=2)
    t = t.cpu().numpy()
    np.testing.assert_array_equal(w.cpu().numpy(), want_w)
    np.testing.assert_allclose(t, want_t, rtol=1e-6, atol=1e-7)
    assert (t > 0).sum() == (want_t > 0).sum()
    np.testing.assert_array_equal(_painted_boxes(t), _painted_boxes(want_t))
