"""Training in fp16 (precision 'fp16' with a posu.amp.LossScaler attached): the training kernels
in F16 storage against autograd (the cases and the bf16 tolerances of
tests/test_gpu_train_kernels.py, which runs them in F32 / BF16), the training step against the
reference golden and against the fp32 step on the GPU beside the bf16 step (the measurement fp16
training exists for), an Adam trajectory through overflow-skipped steps, determinism."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

from posu import amp, ops, optim, packing, synthetic as syn, train_ops as T
from posu._native import F16

pytestmark = pytest.mark.gpu

DT = torch.float16


# ------------------------------------------------------------------ the kernels in F16
def _nhwc(t, cuda, cpad=None):
    t = t.permute(0, 2, 3, 1)
    if cpad is not None and cpad > t.shape[-1]:
        t = F.pad(t, (0, cpad - t.shape[-1]))
    return t.contiguous().to(cuda, DT)


def _nchw(t):
    return t.float().cpu().permute(0, 3, 1, 2)


def _close_lowp(got, ref, frac=0.02):   # test_gpu_train_kernels.py's bf16 gate (fp16 rounds 8 x finer)
    err = (got - ref).abs().max().item()
    scale = ref.abs().max().item()
    assert err <= frac * scale + 1e-3, (err, scale)


DGRAD_CASES = [
    # n, cin, h, w, cout, k, stride, pad
    (2, 64, 16, 16, 64, 3, 1, 1),
    (2, 64, 17, 15, 128, 3, 2, 1),    # strided 3x3, odd input
    (2, 128, 16, 16, 256, 1, 2, 0),   # downsample 1x1 / s2 (with residual: in place over dy's pixels)
    (2, 64, 15, 17, 128, 1, 2, 0),    # the same, odd input
    (3, 256, 8, 8, 64, 1, 1, 0),
    (2, 128, 8, 8, 64, 4, 2, 1),      # the deconv's data gradient is this forward conv's shape
]


@pytest.mark.parametrize('case', DGRAD_CASES)
def test_conv_dgrad_matches_autograd(cuda, case):
    n, cin, h, w, cout, k, s, p = case
    g = torch.Generator().manual_seed(11)
    x = torch.randn(n, cin, h, w, generator=g, requires_grad=True)
    wt = torch.randn(cout, cin, k, k, generator=g) * (2.0 / (cin * k * k)) ** 0.5
    y = F.conv2d(x, wt, stride=s, padding=p)
    dy = torch.randn_like(y)
    (dx_ref,) = torch.autograd.grad(y, x, dy)
    res = torch.randn_like(dx_ref)
    wpk = packing.pack_conv_dgrad_weight(wt.to(cuda), ops.conv_bk(F16), DT)
    dx = T.conv2d_dgrad(_nhwc(dy, cuda), wpk, cin, k, k, s, p, (h, w), F16)
    dx_r = T.conv2d_dgrad(_nhwc(dy, cuda), wpk, cin, k, k, s, p, (h, w), F16, residual=_nhwc(res, cuda))
    torch.cuda.synchronize()
    _close_lowp(_nchw(dx), dx_ref)
    _close_lowp(_nchw(dx_r), dx_ref + res.to(DT).float())


@pytest.mark.parametrize('case', [DGRAD_CASES[0], DGRAD_CASES[1], DGRAD_CASES[4], (2, 64, 16, 16, 256, 1, 1, 0)])
def test_conv_dgrad_every_tile_equals_the_heuristic(cuda, case):
    from posu import plan as pl
    n, cin, h, w, cout, k, s, p = case
    g = torch.Generator().manual_seed(12)
    wt = torch.randn(cout, cin, k, k, generator=g) * (2.0 / (cin * k * k)) ** 0.5
    ho, wo = (h + 2 * p - k) // s + 1, (w + 2 * p - k) // s + 1
    dy = torch.randn(n, ho, wo, cout, generator=g).to(cuda, DT)
    res = torch.randn(n, h, w, cin, generator=g).to(cuda, DT)
    wpk = packing.pack_conv_dgrad_weight(wt.to(cuda), ops.conv_bk(F16), DT)
    for r in (None, res):
        ref = T.conv2d_dgrad(dy, wpk, cin, k, k, s, p, (h, w), F16, residual=r)
        for t in pl._tile_candidates(cin, F16):
            got = T.conv2d_dgrad(dy, wpk, cin, k, k, s, p, (h, w), F16, residual=r, tile=t)
            assert torch.equal(got, ref), (t, r is None)


@pytest.mark.parametrize('n,cin,h,w,cout', [(2, 64, 16, 16, 128), (2, 128, 8, 12, 256), (1, 40, 6, 10, 64)])
def test_s2_conv_data_gradient_as_subpixel_deconv(cuda, n, cin, h, w, cout):
    g = torch.Generator().manual_seed(17)
    x = torch.randn(n, cin, h, w, generator=g, requires_grad=True)
    wt = torch.randn(cout, cin, 3, 3, generator=g) * (2.0 / (cin * 9)) ** 0.5
    y = F.conv2d(x, wt, stride=2, padding=1)
    dy = torch.randn_like(y)
    (dx_ref,) = torch.autograd.grad(y, x, dy)
    wdc = packing.pack_deconv4x4_weight(wt.to(cuda), ops.conv_bk(F16), DT)
    dx = ops.deconv4x4s2_nhwc(_nhwc(dy, cuda), wdc, cin, None, None, False, F16)
    wpk = packing.pack_conv_dgrad_weight(wt.to(cuda), ops.conv_bk(F16), DT)
    dx_up = T.conv2d_dgrad(_nhwc(dy, cuda), wpk, cin, 3, 3, 2, 1, (h, w), F16)
    torch.cuda.synchronize()
    assert dx.shape == dx_up.shape == (n, h, w, cin)
    _close_lowp(_nchw(dx), dx_ref)
    _close_lowp(_nchw(dx), _nchw(dx_up), 0.01)


def test_deconv_weight_and_data_gradients(cuda):
    g = torch.Generator().manual_seed(13)
    n, cin, h, w, cout = 2, 128, 6, 5, 64
    x = torch.randn(n, cin, h, w, generator=g, requires_grad=True)
    wt = (torch.randn(cin, cout, 4, 4, generator=g) * 0.05).requires_grad_(True)
    y = F.conv_transpose2d(x, wt, stride=2, padding=1)
    dy = torch.randn_like(y)
    dx_ref, dw_ref = torch.autograd.grad(y, (x, wt), dy)
    dyd = _nhwc(dy, cuda)
    dw = T.deconv4x4s2_wgrad(_nhwc(x.detach(), cuda), dyd, F16)
    wpk = packing.pack_conv_weight(wt.detach().to(cuda), cout, ops.conv_bk(F16), DT)
    dx = ops.conv2d_nhwc(dyd, wpk, cin, 4, 4, 2, 1, None, None, None, False, F16)
    torch.cuda.synchronize()
    _close_lowp(dw.cpu(), dw_ref)
    _close_lowp(_nchw(dx), dx_ref)


def _bn_ref(z, nseg, gamma, beta, rm, rv, res, relu):
    outs = []
    for zs, rs in zip(z.chunk(nseg), (res.chunk(nseg) if res is not None else [None] * nseg)):
        o = F.batch_norm(zs, rm, rv, gamma, beta, training=True, momentum=0.1, eps=1e-5)
        if rs is not None:
            o = o + rs
        outs.append(F.relu(o) if relu else o)
    return torch.cat(outs)


@pytest.mark.parametrize('c,nseg,residual,relu', [(64, 4, False, True), (256, 2, True, True),
                                                  (2048, 1, False, False), (128, 4, True, True),
                                                  (64, 6, True, True)])  # 6 segments: two finalize passes
@pytest.mark.parametrize('size', [(2, 9, 7), (3, 24, 20)])  # the larger one runs the unrolled loops
def test_bn_train_forward_and_backward_match_autograd(cuda, c, nseg, residual, relu, size):
    g = torch.Generator().manual_seed(14)
    b, h, w = size
    z = (torch.randn(nseg * b, c, h, w, generator=g) * 2 + 0.5).to(DT).float().requires_grad_(True)
    gamma = (torch.rand(c, generator=g) + 0.5).requires_grad_(True)
    beta = (torch.randn(c, generator=g) * 0.1).requires_grad_(True)
    res = torch.randn(nseg * b, c, h, w, generator=g).to(DT).float().requires_grad_(True) if residual else None
    rm0, rv0 = torch.randn(c, generator=g) * 0.1, torch.rand(c, generator=g) + 0.5
    rm, rv = rm0.clone(), rv0.clone()
    y = _bn_ref(z, nseg, gamma, beta, rm, rv, res, relu)
    gy = torch.randn(y.shape, generator=g).to(DT).float()
    grads = torch.autograd.grad(y, [z, gamma, beta] + ([res] if residual else []), gy)
    zd = _nhwc(z.detach(), cuda)
    rmd, rvd = rm0.clone().to(cuda), rv0.clone().to(cuda)
    mean, rstd, sc, sh = T.bn_train_fwd(zd, nseg, gamma.detach().to(cuda), beta.detach().to(cuda), 1e-5, 0.1,
                                        rmd, rvd)
    rd = _nhwc(res.detach(), cuda) if residual else None
    yd = T.bn_apply(zd, nseg, sc, sh, rd, relu)
    dz, gres, dgam, dbet = T.bn_train_bwd(_nhwc(gy, cuda), yd if relu else None, zd, nseg, mean, rstd,
                                          gamma.detach().to(cuda), want_gres=residual)
    if relu and not residual:  # mask recomputed from z instead of read from y: same result
        dz2, _, dg2, db2 = T.bn_train_bwd(_nhwc(gy, cuda), None, zd, nseg, mean, rstd, gamma.detach().to(cuda),
                                          relu_from=(sc, sh))
        torch.testing.assert_close(dz2, dz, atol=0, rtol=0)
        torch.testing.assert_close(dg2, dgam, atol=0, rtol=0)
        torch.testing.assert_close(db2, dbet, atol=0, rtol=0)
    torch.cuda.synchronize()
    torch.testing.assert_close(rmd.cpu(), rm, atol=1e-2, rtol=1e-2)
    _close_lowp(_nchw(yd), y.detach())
    _close_lowp(_nchw(dz), grads[0], 0.03)
    _close_lowp(dgam.cpu(), grads[1], 0.03)
    _close_lowp(dbet.cpu(), grads[2], 0.03)


@pytest.mark.parametrize('shape', [(4, 17, 16, 64), (2, 32, 30, 64), (2, 9, 9, 128)])
def test_fused_stem_bn_relu_maxpool_equals_the_two_pass_path(cuda, shape):
    g = torch.Generator().manual_seed(42)
    n, h, w, c = shape
    nseg = 2
    z = (torch.randint(-3, 4, shape, generator=g).float() * 0.5).to(cuda, DT)   # ties in every window
    gamma = (torch.rand(c, generator=g) + 0.5).to(cuda)
    beta = (torch.randn(c, generator=g) * 0.1).to(cuda)
    _, _, sc, sh = T.bn_train_fwd(z, nseg, gamma, beta, 1e-5, 0.1)
    a = T.bn_apply(z, nseg, sc, sh, None, True)
    ref = ops.maxpool3x3s2_nhwc(a, F16)
    y, idx = T.bn_relu_maxpool(z, nseg, sc, sh)
    gy = torch.randint(-4, 5, ref.shape, generator=g).float().to(cuda, DT)
    gx_ref = T.maxpool3x3s2_bwd(a, gy)
    gx = T.maxpool3x3s2_bwd_idx(idx, gy, (h, w))
    torch.cuda.synchronize()
    assert torch.equal(y, ref)
    assert torch.equal(gx, gx_ref)


def test_maxpool_backward_with_ties_matches_autograd(cuda):
    g = torch.Generator().manual_seed(16)
    x = torch.randint(-2, 3, (2, 64, 17, 16), generator=g).float().requires_grad_(True)  # many ties
    y = F.max_pool2d(x, 3, stride=2, padding=1)
    gy = torch.randint(-4, 5, y.shape, generator=g).float()  # exact in fp16
    (gx_ref,) = torch.autograd.grad(y, x, gy)
    gx = T.maxpool3x3s2_bwd(_nhwc(x.detach(), cuda), _nhwc(gy, cuda))
    torch.testing.assert_close(_nchw(gx), gx_ref, atol=0, rtol=0)


# ------------------------------------------------------------------ the training step
# the bf16 gates of tests/test_gpu_train.py (TRAIN_256_BANDS['bf16'], ['bf16-mse'], ADAM_BANDS['bf16'])
BANDS = {'hm': 0.3, 'loss': 1e-3, 'fund': 1e-2, 'norm_rel_max': 0.9, 'norm_rel_median': 0.6, 'cos': 0.15}
BANDS_MSE = {'hm': 0.3, 'loss': 1e-3, 'norm_rel_max': 0.25, 'norm_rel_median': 0.02, 'cos': 0.995}
ADAM_BANDS = {'loss': 3e-2, 'norm_median': 1e-2, 'norm_max': 0.3}
MAX_BACKOFFS = 17   # 2^16 halves to 1 in sixteen


def _golden_net(cuda, g, precision='fp32'):
    from models.pose_resnet import get_pose_net
    cfg = syn.make_cfg(num_layers=int(g['num_layers']), image_size=int(g['image_size']))
    net = get_pose_net(cfg, is_train=False, precision=precision)
    net.load_state_dict(syn.synthetic_state_dict(net.state_dict(), seed=int(g['seed'])))
    return net.to(cuda)


def _step(cuda, g, precision, net, scaler=None):
    """tests/test_gpu_train.py::_step (one reference-style training step, no optimizer) on `net`;
    with a scaler the backward runs on scaler.scale(loss)."""
    from core.loss import FundamentalLoss, JointsMSELoss
    from models.multiview_pose_resnet import get_multiview_pose_net
    from utils.transforms import generate_integral_preds_2d_th, transform_back_th
    nl, size, nv, b, seed = (int(g[k]) for k in ('num_layers', 'image_size', 'nviews', 'batch', 'seed'))
    cfg = syn.make_cfg(num_layers=nl, image_size=size)
    net.precision = precision
    net.loss_scaler = scaler
    net = net.train()
    net.zero_grad(set_to_none=True)
    model = get_multiview_pose_net(net, cfg)
    views = [v.to(cuda) for v in syn.synthetic_views(nv, b, size, seed=seed + 1)]
    meta = [{'center': torch.from_numpy(g['centers'][v]), 'scale': torch.from_numpy(g['scales'][v]),
             'subject': torch.from_numpy(g['subjects'])} for v in range(nv)]
    target = [torch.from_numpy(g['targets'][v]).to(cuda) for v in range(nv)]
    weight = [torch.from_numpy(g['target_weight'][v]).to(cuda) for v in range(nv)]
    raw_features, _, _, _ = model(views)
    crit = JointsMSELoss(use_target_weight=True)
    mse = 0
    for t, w, r in zip(target, weight, raw_features):
        mse = mse + crit(r, t, w)
    joints2d = transform_back_th(cfg, [generate_integral_preds_2d_th(o) for o in raw_features], meta)
    fl = FundamentalLoss(cfg, fundamental_matrix_dict=syn.fundamental_dict(), device=cuda)
    fl.use_target_weight = True
    fund = fl(joints2d, weight, meta) * float(g['fund_weight'])
    loss = mse + fund
    (loss if scaler is None else scaler.scale(loss)).backward()
    return net, raw_features, joints2d, mse, fund


def _clean_step(cuda, g, precision, net=None, scaler=None):
    """A step whose gradients did not overflow, through public calls only: forward,
    scaler.scale(loss).backward(), unscale_, update(); again while found_inf() is set (the scale
    halves each time).  The gradients left in .grad are the unscaled ones.  fp32 / bf16: the
    plain step.  -> (net, heatmaps, joints, mse, fund, scaler, optimizer)."""
    net = _golden_net(cuda, g) if net is None else net
    if precision != 'fp16':
        out = _step(cuda, g, precision, net)
        torch.cuda.synchronize()
        return out + (None, None)
    scaler = amp.LossScaler() if scaler is None else scaler
    opt = optim.Adam(net.parameters(), lr=1e-3, capturable=True)
    for _ in range(MAX_BACKOFFS):
        out = _step(cuda, g, precision, net, scaler)
        scaler.unscale_(opt)
        scaler.update()
        if not scaler.found_inf():
            torch.cuda.synchronize()
            return out + (scaler, opt)
    raise AssertionError('the fp16 gradients still overflow at scale %g' % scaler.get_scale())


def test_fp16_train_step_meets_the_bf16_gates_of_the_reference_golden(cuda, golden):
    g = golden('train_step_r50_128.npz')
    net, hm, joints, mse, fund, scaler, _ = _clean_step(cuda, g, 'fp16')
    hm_err = float(np.abs(torch.stack(hm).detach().cpu().numpy() - g['heatmaps']).max())
    named = dict(net.named_parameters())
    assert list(named) == list(g['grad_names']) and len(named) == 170
    norms = np.array([named[n].grad.norm().item() for n in g['grad_names']])
    rel = np.abs(norms / g['grad_norms'] - 1)
    print('fp16 R50@128 step at scale %g: heatmaps max %.3g, mse %.6g vs %.6g, fund %.6g vs %.6g, grad-norm rel '
          'median %.3g max %.3g, all-zero gradients %d'
          % (scaler.get_scale(), hm_err, mse.item(), g['loss_mse'], fund.item(), g['loss_fund'], np.median(rel),
             rel.max(), int((norms == 0).sum())))
    assert hm_err < BANDS['hm']
    np.testing.assert_allclose(mse.item(), g['loss_mse'], rtol=BANDS['loss'])
    np.testing.assert_allclose(fund.item(), g['loss_fund'], rtol=BANDS['fund'])
    assert np.all(np.isfinite(norms))
    for n, got, ref in zip(g['grad_names'], norms, g['grad_norms']):
        assert torch.isfinite(named[n].grad).all(), n
        assert got > 0 or ref == 0, n


def _inputs_r50_256(groups=2, seed=3):
    """tests/test_gpu_train.py's configs[3]-shaped batch (R50@256, 4 views x `groups`)."""
    from posu.pipeline import synthetic_meta
    _, host = synthetic_meta(groups, 'cpu', image_size=256)
    r = np.random.default_rng(seed)
    c = r.uniform(4, 60, size=(4, groups, 16, 2))
    ys, xs = np.meshgrid(np.arange(64), np.arange(64), indexing='ij')
    tgt = np.exp(-((xs - c[..., 0, None, None]) ** 2 + (ys - c[..., 1, None, None]) ** 2) / 8.0).astype(np.float32)
    tw = (r.uniform(size=(4, groups, 16, 1)) > 0.1).astype(np.float32)
    return {'num_layers': 50, 'image_size': 256, 'nviews': 4, 'batch': groups, 'seed': seed, 'fund_weight': 10.0,
            'targets': tgt, 'target_weight': tw, 'centers': host['centers'], 'scales': host['scales'],
            'subjects': host['subjects']}


@pytest.fixture(scope='module')
def against_fp32(cuda):
    """R50@256, 4 views x 2, fund_weight 10 and 0: the bf16 and the fp16 step against the fp32 step
    on the GPU, same weights and batch.  {fund_weight: {precision: metrics}}."""
    g = _inputs_r50_256()
    net = _golden_net(cuda, g)
    out = {}
    for fw in (10.0, 0.0):
        g['fund_weight'] = fw
        runs = {}
        for precision in ('fp32', 'bf16', 'fp16'):
            _, hm, _, mse, fund, scaler, _ = _clean_step(cuda, g, precision, net)
            runs[precision] = {'hm': torch.stack(hm).detach().clone(), 'mse': mse.item(), 'fund': float(fund.detach()),
                               'grads': [p.grad.detach().double().ravel().clone() for p in net.parameters()],
                               'scale': None if scaler is None else scaler.get_scale()}
        ref = runs['fp32']
        gr = torch.cat(ref['grads'])
        nr = np.array([float(t.norm()) for t in ref['grads']])
        out[fw] = {}
        for precision in ('bf16', 'fp16'):
            r = runs[precision]
            ga = torch.cat(r['grads'])
            rel = np.abs(np.array([float(t.norm()) for t in r['grads']]) / nr - 1)
            m = {'hm': float((r['hm'] - ref['hm']).abs().max()), 'mse': r['mse'], 'mse_ref': ref['mse'],
                 'fund': r['fund'], 'fund_ref': ref['fund'], 'cos': float(ga @ gr / (ga.norm() * gr.norm())),
                 'norm_rel_median': float(np.median(rel)), 'norm_rel_max': float(rel.max()),
                 'finite': bool(torch.isfinite(ga).all()), 'scale': r['scale']}
            out[fw][precision] = m
            print('R50@256 4x2 fund_weight %g, %s against the fp32 GPU step: heatmaps max %.4g, mse %.6g vs %.6g, '
                  'fund %.6g vs %.6g, grad-norm rel median %.4g max %.4g, whole-gradient cosine %.6f%s'
                  % (fw, precision, m['hm'], m['mse'], m['mse_ref'], m['fund'], m['fund_ref'], m['norm_rel_median'],
                     m['norm_rel_max'], m['cos'], '' if m['scale'] is None else ' (loss scale %g)' % m['scale']))
    return out


@pytest.mark.parametrize('fund_weight', [10.0, 0.0])
def test_fp16_step_is_closer_to_fp32_than_the_bf16_step(against_fp32, fund_weight):
    """The measurement fp16 training exists for (DESIGN.md section 5 records the printed values)."""
    bf, fp = against_fp32[fund_weight]['bf16'], against_fp32[fund_weight]['fp16']
    assert fp['finite']
    assert fp['hm'] < bf['hm'], (fp['hm'], bf['hm'])
    assert fp['cos'] > bf['cos'], (fp['cos'], bf['cos'])


@pytest.mark.parametrize('fund_weight', [10.0, 0.0])
def test_fp16_step_passes_the_bf16_bands(against_fp32, fund_weight):
    m = against_fp32[fund_weight]['fp16']
    b = BANDS if fund_weight else BANDS_MSE
    assert m['hm'] < b['hm']
    np.testing.assert_allclose(m['mse'], m['mse_ref'], rtol=b['loss'])
    if fund_weight:
        np.testing.assert_allclose(m['fund'], m['fund_ref'], rtol=b['fund'])
    assert m['norm_rel_max'] < b['norm_rel_max']
    assert m['norm_rel_median'] < b['norm_rel_median']
    assert m['cos'] > b['cos']


def _adam_run(cuda, g, scaler, max_iters):
    """tests/test_gpu_train.py's Adam trajectory in fp16 through `scaler` and the capturable
    posu.optim.Adam: iterate until len(g['losses']) steps were applied.  -> losses and parameter
    norms of the applied steps, iterations used, all-zero gradient tensors per applied step."""
    from core.loss import JointsMSELoss
    from models.multiview_pose_resnet import get_multiview_pose_net
    from models.pose_resnet import get_pose_net
    nl, size, nv, b, seed = (int(g[k]) for k in ('num_layers', 'image_size', 'nviews', 'batch', 'init_seed'))
    cfg = syn.make_cfg(num_layers=nl, image_size=size)
    net = get_pose_net(cfg, is_train=False, precision='fp16', loss_scaler=scaler)
    net.load_state_dict(syn.reference_init_state_dict(net.state_dict(), seed=seed))
    net = net.to(cuda).train()
    model = get_multiview_pose_net(net, cfg)
    views = [v.to(cuda) for v in syn.synthetic_views(nv, b, size, seed=seed + 1)]
    tgt = torch.from_numpy(g['targets']).to(cuda)
    tw = torch.from_numpy(g['target_weight']).to(cuda)
    opt = optim.Adam(net.parameters(), lr=float(g['lr']), capturable=True)
    crit = JointsMSELoss(use_target_weight=True)
    params = list(net.parameters())
    losses, norms, zeros = [], [], []
    iters = 0
    while len(losses) < len(g['losses']) and iters < max_iters:
        iters += 1
        before = [p.detach().clone() for p in params]
        out, _, _, _ = model(views)
        loss = sum(crit(o, tgt[v], tw[v]) for v, o in enumerate(out))
        opt.zero_grad()
        scaler.scale(loss).backward()
        scaler.step(opt)
        skipped = scaler.found_inf()
        scaler.update()
        if skipped:   # an overflowed step changes nothing but the scale
            assert all(torch.equal(a, p.detach()) for a, p in zip(before, params))
            continue
        assert not all(torch.equal(a, p.detach()) for a, p in zip(before, params))
        losses.append(loss.item())
        norms.append([float(p.detach().norm()) for p in params])
        zeros.append(sum(int(not bool(p.grad.any())) for p in params))
    return np.array(losses), np.array(norms), iters, zeros


def test_fp16_adam_trajectory_skips_overflows_and_matches_reference(cuda, golden):
    g = golden('adam_r18_128.npz')
    scaler = amp.LossScaler()
    losses, norms, iters, zeros = _adam_run(cuda, g, scaler, 22)
    print('fp16 Adam trajectory: %d iterations for %d applied steps, final scale %g, all-zero gradient tensors per '
          'step %s\n  losses %s\n  ref fp64 %s' % (iters, len(losses), scaler.get_scale(), zeros, np.round(losses, 6),
                                                   np.round(g['losses_f64'], 6)))
    assert len(losses) == len(g['losses']) == 6
    rel = np.abs(losses / g['losses_f64'] - 1)
    nrel = np.abs(norms / g['param_norms_f64'] - 1)
    print('  loss rel vs fp64 %s, param-norm rel median %s max %s' % (rel, np.median(nrel, axis=1), nrel.max(axis=1)))
    assert np.all(np.isfinite(losses))
    assert rel.max() < ADAM_BANDS['loss'], rel
    assert np.median(nrel, axis=1).max() < ADAM_BANDS['norm_median']
    assert nrel.max() < ADAM_BANDS['norm_max']
    # for the record (no gate): the same run without loss scaling -- scale 1, growth off
    plain = amp.LossScaler(init_scale=1.0, growth_factor=1.0)
    l1, _, it1, z1 = _adam_run(cuda, g, plain, 6)
    print('  unscaled (scale 1): %d iterations, all-zero gradient tensors per step %s of %d, losses %s'
          % (it1, z1, norms.shape[1], np.round(l1, 6)))


def test_fp16_step_is_deterministic(cuda, golden):
    g = golden('train_step_r50_128.npz')
    net = _golden_net(cuda, g)
    state = {k: v.detach().clone() for k, v in net.state_dict().items()}
    _, _, _, _, _, scaler, _ = _clean_step(cuda, g, 'fp16', net)
    fixed = scaler.get_scale()   # a scale that does not overflow: both runs take one pass at it
    runs = []
    for _ in range(2):
        net.load_state_dict(state)
        _clean_step(cuda, g, 'fp16', net, amp.LossScaler(init_scale=fixed))
        grads = [p.grad.detach().clone() for p in net.parameters()]
        st = optim.GradStats(cuda)
        st.run(grads)
        runs.append((grads, st.sumsq.item(), float(st.found_inf.item())))
    (ga, sa, fa), (gb, sb, fb) = runs
    assert fa == fb == 0.0 and np.float64(sa).tobytes() == np.float64(sb).tobytes()
    for i, (a, b) in enumerate(zip(ga, gb)):
        assert torch.equal(a, b), i
