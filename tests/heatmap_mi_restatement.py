"""A plain-torch, materialising statement of the heatmap mutual-information loss: the dense
[N Q Q, C + 1] pair tensor, the three-layer discriminator with batch statistics, and the JSD /
InfoNCE measures, in whatever dtype and on whatever device its inputs have.  The golden tests
hold it to the reference's numbers in fp64; the GPU tests compare the kernels against it.

Parameters are a dict keyed like the module's state_dict ('block_nonlinear.0.weight', ...).
"""
import math

import torch
import torch.nn.functional as F

EPS = 1e-5
MOMENTUM = 0.1
PARAM_KEYS = ('block_nonlinear.0.weight', 'block_nonlinear.1.weight', 'block_nonlinear.1.bias',
              'block_nonlinear.3.weight', 'block_nonlinear.3.bias', 'block_nonlinear.4.weight',
              'block_nonlinear.4.bias', 'block_nonlinear.6.weight', 'block_nonlinear.6.bias')
BUFFER_KEYS = ('block_nonlinear.1.running_mean', 'block_nonlinear.1.running_var',
               'block_nonlinear.4.running_mean', 'block_nonlinear.4.running_var')
# the reference module's state_dict: (key, shape as a function of c_in and c_m)
STATE_LAYOUT = (
    ('block_nonlinear.0.weight', lambda ci, cm: (cm, ci)),
    ('block_nonlinear.1.weight', lambda ci, cm: (cm,)),
    ('block_nonlinear.1.bias', lambda ci, cm: (cm,)),
    ('block_nonlinear.1.running_mean', lambda ci, cm: (cm,)),
    ('block_nonlinear.1.running_var', lambda ci, cm: (cm,)),
    ('block_nonlinear.1.num_batches_tracked', lambda ci, cm: ()),
    ('block_nonlinear.3.weight', lambda ci, cm: (cm // 4, cm)),
    ('block_nonlinear.3.bias', lambda ci, cm: (cm // 4,)),
    ('block_nonlinear.4.weight', lambda ci, cm: (cm // 4,)),
    ('block_nonlinear.4.bias', lambda ci, cm: (cm // 4,)),
    ('block_nonlinear.4.running_mean', lambda ci, cm: (cm // 4,)),
    ('block_nonlinear.4.running_var', lambda ci, cm: (cm // 4,)),
    ('block_nonlinear.4.num_batches_tracked', lambda ci, cm: ()),
    ('block_nonlinear.6.weight', lambda ci, cm: (1, cm // 4)),
    ('block_nonlinear.6.bias', lambda ci, cm: (1,)),
)


def pair_tensor(low_features, heatmaps, indices, joint_idx):
    """[N, C, H, W], [N, J, H, W], [N, Q] -> [N Q Q, 1 + C]; row (n, i, j) = [h[n, idx[n, j]] | f[n, idx[n, i], :]]."""
    n, c = low_features.shape[:2]
    q = indices.shape[1]
    rows = low_features.permute(0, 2, 3, 1).reshape(n, -1, c)
    f = rows.gather(1, indices[:, :, None].expand(n, q, c))
    h = heatmaps[:, joint_idx].reshape(n, -1).gather(1, indices)
    return torch.cat([h[:, None, :, None].expand(n, q, q, 1), f[:, :, None, :].expand(n, q, q, c)], dim=3).reshape(
        n * q * q, c + 1)


def discriminator(x, state, training, buffers=None):
    """The three Linear layers with BatchNorm1d + LeakyReLU(0.2) between them on rows x [R, c_in].
    training: batch statistics, and `buffers` (a dict of the four running tensors) is updated in
    place the way BatchNorm1d does; otherwise the running statistics in `state` normalise."""
    def bn(z, name):
        rm = (buffers if training else state)['block_nonlinear.%s.running_mean' % name]
        rv = (buffers if training else state)['block_nonlinear.%s.running_var' % name]
        return F.batch_norm(z, rm, rv, state['block_nonlinear.%s.weight' % name],
                            state['block_nonlinear.%s.bias' % name], training, MOMENTUM, EPS)
    z = x @ state['block_nonlinear.0.weight'].t()
    z = F.leaky_relu(bn(z, '1'), 0.2)
    z = z @ state['block_nonlinear.3.weight'].t() + state['block_nonlinear.3.bias']
    z = F.leaky_relu(bn(z, '4'), 0.2)
    return z @ state['block_nonlinear.6.weight'].t() + state['block_nonlinear.6.bias']


def jsd(u):
    """u [N, Q, Q]: mean off the diagonal of softplus(-u) + u - log 2, minus the mean on it of log 2 - softplus(-u)."""
    q = u.shape[1]
    eye = torch.eye(q, dtype=torch.bool, device=u.device)[None].expand_as(u)
    sp = F.softplus(-u)
    return (sp + u - math.log(2.0))[~eye].mean() - (math.log(2.0) - sp)[eye].mean()


def nce(u):
    """u [N, Q, Q]: mean over (n, i) of -log_softmax([u_ii, u_i0 .. u_iQ-1 with -10 at j = i])[0]."""
    q = u.shape[1]
    eye = torch.eye(q, dtype=torch.bool, device=u.device)[None]
    diag = torch.diagonal(u, dim1=1, dim2=2)
    logits = torch.cat([diag[:, :, None], torch.where(eye, torch.full_like(u, -10.0), u)], dim=2)
    return -(F.log_softmax(logits, dim=2)[:, :, 0]).mean()


MEASURES = {'JSD': jsd, 'NCE': nce}


def scores(low_features, heatmaps, indices, joint_idx, state, training=True, buffers=None):
    """u [N, Q, Q] of one view."""
    n, q = indices.shape
    x = pair_tensor(low_features, heatmaps, indices, joint_idx)
    return discriminator(x, state, training, buffers).reshape(n, q, q)


def loss(low_features, heatmaps, indices, joint_idx, state, measure, training=True, buffers=None):
    return MEASURES[measure](scores(low_features, heatmaps, indices, joint_idx, state, training, buffers))


def evaluate(case, indices, joint_idx, measure, training, dtype, device, feature_dtype=None):
    """Loss, scores, every gradient and the updated buffers of one view, from a
    posu.synthetic.heatmap_mi_case dict (numpy float64), computed in `dtype` on `device`.
    feature_dtype: the features are rounded to it first (then computed in `dtype`).
    Gradients of the inputs come back dense ('dlow', 'dheat') and gathered at the sampled
    positions ('dlow_at' [N, Q, C], 'dheat_at' [N, Q])."""
    t = lambda a: torch.as_tensor(a).to(device=device, dtype=dtype)  # noqa: E731
    low = torch.as_tensor(case['low_features']).to(device)
    if feature_dtype is not None:
        low = low.to(feature_dtype)
    low = low.to(dtype).requires_grad_(True)
    heat = t(case['heatmaps']).requires_grad_(True)
    idx = torch.as_tensor(indices).long().to(device)
    state = {k: t(v) for k, v in case['state'].items() if 'num_batches' not in k}
    for k in PARAM_KEYS:
        state[k].requires_grad_(True)
    buffers = {k: state[k].clone() for k in BUFFER_KEYS}
    u = scores(low, heat, idx, joint_idx, state, training, buffers)
    val = MEASURES[measure](u)
    grads = torch.autograd.grad(val, [low, heat] + [state[k] for k in PARAM_KEYS])
    n, q = idx.shape
    c = low.shape[1]
    out = {'loss': val.detach(), 'u': u.detach(), 'dlow': grads[0], 'dheat': grads[1]}
    out['dlow_at'] = grads[0].permute(0, 2, 3, 1).reshape(n, -1, c).gather(1, idx[:, :, None].expand(n, q, c))
    out['dheat_at'] = grads[1][:, joint_idx].reshape(n, -1).gather(1, idx)
    for k, g in zip(PARAM_KEYS, grads[2:]):
        out['grad.' + k] = g
    for k in BUFFER_KEYS:
        out['buffer.' + k] = buffers[k]
    return out
