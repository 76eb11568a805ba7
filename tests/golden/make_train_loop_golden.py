"""Generate tests/golden/train_loop.npz by running the REFERENCE's own core.evaluate.accuracy
(lib/core/evaluate.py:42-73) and utils.gradients.check_grad_norm (lib/utils/gradients.py:16-40) on
the CPU.  Run once, where the reference is checked out (not on the GPU box):

    python tests/golden/make_train_loop_golden.py

The reference is imported in-process the way make_heatmap_mi_golden.py does it (make_golden's cv2
stand-in and REF_LIB).  The file holds data only: the small inputs and the reference's results.
The reference's train() itself needs a cuda device, a process group and h5py, so the loop is
checked on the GPU against a hand-written sequence of pieces that are pinned elsewhere.

Accuracy cases (output / target [N, J, H, W] f32 -> acc [J + 1], avg, cnt, pred [N, J, 2]):
  a  N = 3, J = 5, 16 x 16 peaked maps;
  b  N = 1, J = 4, 40 x 40 one-hot maps on the threshold: d exactly 0.5 (no hit at thr 0.5), d = 0.25
     (a hit), an invalid target (1, 7), an all-zero output against target (9, 9);
  c  N = 4, J = 6, 8 x 12 maps (non-square);
  c24  N = 4, J = 6, 8 x 24 maps: the H / W pairing of the normalisation decides the hits (a target one px
     off along x is a miss, 1 / 0.8, and one px off along y a hit, 1 / 2.4; the other pairing gives the opposite);
  d  N = 2, J = 4, 8 x 8: two equal maxima, an all-negative map, a joint whose targets are all invalid;
  d0 N = 1, J = 2, 8 x 8: every joint invalid (cnt 0, avg 0);
  e3x5 / e4x4  N = 2, J = 3 maps smaller than a wave, H W not a multiple of 4;
  f  N = 1, J = 5, 16 x 16.

Gradient-norm cases: V = 4 tensors [3, 2 * 4 * 4] in float64 on float32-representable values, the
losses sums of squares: view 3 unused by 'plain' (no gradient), view 1 with a zero row; 'nan' adds
view 3 at zero (all its gradient rows zero: 0 / 0); norm orders 1 and 2.
"""
import os
import sys
from collections import OrderedDict

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import make_golden as mg  # noqa: E402  (the cv2 stand-in and REF_LIB)


def _import_reference():
    mg._install_cv2_standin()
    for p in (mg.REF_LIB, os.path.join(mg.REF_LIB, 'core')):
        if p not in sys.path:
            sys.path.insert(0, p)
    import core.evaluate as ref_eval
    import utils.gradients as ref_grad
    return ref_eval, ref_grad


OFFSETS = ((0, 0), (0, 0), (0, 0), (1, 0), (0, 1), (-1, 0), (0, -1), (1, 1))   # (dx, dy) of target - output


def _peaked(r, n, j, h, w):
    """Noise in [0, 0.5) plus one peak per output map; the target's peak sits on it or one px away."""
    out = r.uniform(0.0, 0.5, size=(n, j, h, w))
    tgt = np.zeros((n, j, h, w))
    for a in range(n):
        for b in range(j):
            y, x = int(r.integers(0, h)), int(r.integers(0, w))
            out[a, b, y, x] = 1.0 + r.uniform()
            dx, dy = OFFSETS[int(r.integers(0, len(OFFSETS)))]
            tgt[a, b, int(np.clip(y + dy, 0, h - 1)), int(np.clip(x + dx, 0, w - 1))] = 1.0
    return out.astype(np.float32), tgt.astype(np.float32)


def _onehot(shape, points):
    m = np.zeros(shape, dtype=np.float32)
    for (a, b), xy in points.items():
        if xy is not None:
            m[a, b, xy[1], xy[0]] = 1.0
    return m


def accuracy_cases():
    r = np.random.default_rng(20240)
    cases = OrderedDict()
    cases['a'] = _peaked(r, 3, 5, 16, 16)
    cases['b'] = (_onehot((1, 4, 40, 40), {(0, 0): (12, 10), (0, 1): (11, 10), (0, 2): (5, 5), (0, 3): None}),
                  _onehot((1, 4, 40, 40), {(0, 0): (10, 10), (0, 1): (10, 10), (0, 2): (1, 7), (0, 3): (9, 9)}))
    cases['c'] = _peaked(r, 4, 6, 8, 12)
    cases['c24'] = _peaked(r, 4, 6, 8, 24)
    out, tgt = _peaked(r, 2, 4, 8, 8)
    out[0, 0] = 0.0
    out[0, 0, 2, 5] = out[0, 0, 6, 1] = 0.75         # two equal maxima: the first wins
    out[:, 1] = -1.0 - np.abs(out[:, 1])             # all negative: coordinates (0, 0)
    tgt[:, 2] = 0.0
    tgt[0, 2, 4, 1] = tgt[1, 2, 0, 6] = 1.0          # x <= 1 / y <= 1: every target of joint 2 invalid
    cases['d'] = (out, tgt)
    cases['d0'] = (_peaked(r, 1, 2, 8, 8)[0], np.zeros((1, 2, 8, 8), dtype=np.float32))
    cases['e3x5'] = _peaked(r, 2, 3, 3, 5)
    cases['e4x4'] = _peaked(r, 2, 3, 4, 4)
    cases['f'] = _peaked(r, 1, 5, 16, 16)
    return cases


def gradient_case():
    r = np.random.default_rng(20241)
    x = r.standard_normal((4, 3, 2 * 4 * 4)).astype(np.float32).astype(np.float64)
    x[1, 1] = 0.0     # one zero row
    x[3] = 0.0        # a view at zero: its gradient rows are all zero
    return x, np.array([1.0, 0.5, 2.0, 4.0])   # loss weights (powers of two: the gradients stay f32 values)


def main():
    ref_eval, ref_grad = _import_reference()
    blob = {}
    for name, (out, tgt) in accuracy_cases().items():
        # at thr 0.5 only: the reference's accuracy() does not pass its thr argument on to dist_acc
        acc, avg, cnt, pred = ref_eval.accuracy(out, tgt)
        print('accuracy %-5s %s: acc %s avg %r cnt %d' % (name, out.shape, np.round(acc, 4), avg, cnt))
        blob.update({'acc.%s.output' % name: out, 'acc.%s.target' % name: tgt,
                     'acc.%s.acc' % name: np.asarray(acc, dtype=np.float64),
                     'acc.%s.avg' % name: np.float64(avg), 'acc.%s.cnt' % name: np.int64(cnt),
                     'acc.%s.pred' % name: np.asarray(pred, dtype=np.float32)})
    assert np.array_equal(blob['acc.b.acc'], np.array([1 / 3, 0, 1, -1, 0])) and blob['acc.b.cnt'] == 3
    assert blob['acc.d0.cnt'] == 0 and blob['acc.d0.avg'] == 0

    x, k = gradient_case()
    views = [torch.from_numpy(x[v]).reshape(3, 2, 4, 4).requires_grad_(True) for v in range(4)]
    plain = sum(k[v] * (views[v] ** 2).sum() for v in range(3))
    losses = OrderedDict([('plain', plain), ('nan', plain + k[3] * (views[3] ** 2).sum())])
    grads = np.stack([2.0 * k[v] * x[v] for v in range(4)])
    assert np.array_equal(grads, grads.astype(np.float32).astype(np.float64))
    blob['gn.grads'] = grads
    blob['gn.unused'] = np.array([[0, 0, 0, 1], [0, 0, 0, 0]], dtype=np.uint8)   # per loss, per view
    blob['gn.losses'] = np.array(list(losses))
    for p in (1, 2):
        res = ref_grad.check_grad_norm(losses, views, norm=p)
        blob['gn.p%d' % p] = np.array([float(res[name]) for name in losses], dtype=np.float64)
        print('grad norm p=%d: %s' % (p, blob['gn.p%d' % p]))
        assert np.isfinite(blob['gn.p%d' % p][0]) and np.isnan(blob['gn.p%d' % p][1])
    path = os.path.join(HERE, 'train_loop.npz')
    np.savez(path, **blob)
    print('wrote', path, os.path.getsize(path), 'bytes')


if __name__ == '__main__':
    main()
