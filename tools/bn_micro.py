"""Micro-benchmark of the training BatchNorm passes (posu_bn_train_fwd / posu_bn_apply /
posu_bn_train_bwd) at the R50@256 training-step shapes (128 frames = 4 view segments),
HIP events, one process, min over rounds.  Reports algorithmic HBM bytes / time.

    python tools/bn_micro.py [--reps 20] [--rounds 3]

Run under `rocprofv3 --kernel-trace --stats` for the per-kernel split.

    python tools/bn_micro.py --digest [--lib PATH]

No timing: every entry point of csrc/bn_train.hip at small fixed shapes (the GPU tests' shapes;
bf16 / f16 / f32; per-channel parameters 16-byte aligned and 4 bytes off, which takes the generic
kernels; odd H and W for the pool) and one sha1 per output tensor.  Two builds compute the same
bits when their listings are equal line for line.
"""
import argparse
import hashlib
import os
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(REPO, 'pose-unsupervised_amd', 'lib'), REPO]

import torch  # noqa: E402

from posu import train_ops as T  # noqa: E402

SHAPES = [(128, 64, 64, 256), (128, 64, 64, 64), (128, 32, 32, 512), (128, 16, 16, 1024), (128, 8, 8, 2048)]
NSEG = 4


def timeit(fn, reps, rounds):
    best = 1e9
    for _ in range(rounds):
        fn()
        torch.cuda.synchronize()
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(reps):
            fn()
        b.record()
        b.synchronize()
        best = min(best, a.elapsed_time(b) * 1e3 / reps)
    return best


# (C, nseg, (images per segment, H, W)): the BatchNorm tests' shapes; 128 x 128 pixels per segment
# are 256 / 128 partial blocks per segment (four / two trips of the finalize)
DIGEST_BN = [(64, 1, (1, 128, 128)), (64, 2, (1, 128, 128)), (256, 2, (3, 24, 20)), (64, 4, (2, 9, 7)),
             (64, 4, (3, 24, 20)), (256, 2, (2, 9, 7)), (128, 4, (3, 24, 20)), (64, 6, (2, 9, 7)),
             (2048, 1, (2, 9, 7)), (2048, 1, (2, 5, 3))]
DIGEST_POOL = [(4, 17, 16, 64), (2, 32, 30, 64), (2, 9, 9, 128), (2, 17, 16, 64), (2, 7, 5, 8)]


def sha(t):
    return hashlib.sha1(t.contiguous().view(torch.uint8).cpu().numpy().tobytes()).hexdigest()[:12]


def off4(t):
    """t's values in a contiguous view that starts 4 bytes into a larger (aligned) buffer."""
    buf = torch.empty(t.numel() + 1, dtype=t.dtype, device=t.device)
    buf[1:].copy_(t.reshape(-1))
    return buf[1:].view(t.shape)


def digest():
    dev = torch.device('cuda', 0)

    def line(tag, *outs):
        torch.cuda.synchronize()
        print('%-58s %s' % (tag, ' '.join(sha(o) for o in outs if o is not None)))

    for dt in (torch.bfloat16, torch.float16, torch.float32):
        name = str(dt).split('.')[1]
        for c, nseg, (b, h, w) in DIGEST_BN:
            g = torch.Generator().manual_seed(1000 + c + 7 * nseg + h)
            shp = (nseg * b, h, w, c)
            z = (torch.randn(shp, generator=g) * 2 + 0.4).to(dev, dt)
            r = torch.randn(shp, generator=g).to(dev, dt)
            gy = torch.randn(shp, generator=g).to(dev, dt)
            gamma = (torch.rand(c, generator=g) + 0.5).to(dev)
            beta = (torch.randn(c, generator=g) * 0.1).to(dev)
            rm, rv = (torch.randn(c, generator=g) * 0.1).to(dev), (torch.rand(c, generator=g) + 0.5).to(dev)
            tag = '%s C%d nseg%d %dx%dx%d ' % (name, c, nseg, b, h, w)
            mean, rstd, sc, sh = T.bn_train_fwd(z, nseg, gamma, beta, 1e-5, 0.1, rm, rv)
            line(tag + 'bn_train_fwd', mean, rstd, sc, sh, rm, rv)
            line(tag + 'channel_sum', T.channel_sum(z))
            for al, f in (('aligned', lambda t: t), ('off4', off4)):
                m_, r_, sc_, sh_ = f(mean), f(rstd), f(sc), f(sh)
                y = T.bn_apply(z, nseg, sc_, sh_, r, True)
                y0 = T.bn_apply(z, nseg, sc_, sh_, None, True)
                line(tag + al + ' bn_apply(res,relu)', y)
                line(tag + al + ' bn_apply(relu)', y0)
                line(tag + al + ' bn_apply()', T.bn_apply(z, nseg, sc_, sh_, None, False))
                y2, mask = T.bn_apply_mask(z, nseg, sc_, sh_, r)
                line(tag + al + ' bn_apply_mask', y2, mask)
                line(tag + al + ' bn_train_bwd(y)', *T.bn_train_bwd(gy, y, z, nseg, m_, r_, gamma, want_gres=True))
                line(tag + al + ' bn_train_bwd_mask', *T.bn_train_bwd(gy, None, z, nseg, m_, r_, gamma, want_gres=True,
                                                                      mask=mask))
                line(tag + al + ' bn_train_bwd(relu_from)', *T.bn_train_bwd(gy, None, z, nseg, m_, r_, gamma,
                                                                            relu_from=(sc_, sh_)))
                line(tag + al + ' bn_train_bwd()', *T.bn_train_bwd(gy, None, z, nseg, m_, r_, gamma))
        for shp in DIGEST_POOL:
            n, h, w, c = shp
            g = torch.Generator().manual_seed(2000 + h + w)
            zf = torch.randint(-3, 4, shp, generator=g).float() * 0.5   # ties in every window
            x = zf.clone()
            x[0, h // 2, w // 2, :] = float('nan')                       # a NaN is taken
            z, x = zf.to(dev, dt), x.to(dev, dt)
            ho, wo = (h - 1) // 2 + 1, (w - 1) // 2 + 1
            gy = torch.randint(-4, 5, (n, ho, wo, c), generator=g).float().to(dev, dt)
            gamma = (torch.rand(c, generator=g) + 0.5).to(dev)
            beta = (torch.randn(c, generator=g) * 0.1).to(dev)
            tag = '%s pool %dx%dx%dx%d ' % ((name,) + shp)
            _, _, sc, sh = T.bn_train_fwd(z, 2, gamma, beta, 1e-5, 0.1)
            line(tag + 'maxpool3x3s2_bwd', T.maxpool3x3s2_bwd(x, gy))
            for al, f in (('aligned', lambda t: t), ('off4', off4)):
                y, idx = T.bn_relu_maxpool(z, 2, f(sc), f(sh))
                line(tag + al + ' bn_relu_maxpool3x3s2_fwd', y, idx)
            line(tag + 'maxpool3x3s2_bwd_idx', T.maxpool3x3s2_bwd_idx(idx, gy, (h, w)))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=20)
    ap.add_argument('--rounds', type=int, default=3)
    ap.add_argument('--lib', default=None, help='another build of libposeu.so (experiments)')
    ap.add_argument('--frames', type=int, default=128, help='batch of the shapes (32: one view of the 4)')
    ap.add_argument('--nseg', type=int, default=NSEG)
    ap.add_argument('--digest', action='store_true', help='no timing: one sha1 per output tensor at small shapes')
    args = ap.parse_args()
    if args.lib:
        from posu import _native
        _native._LIB_PATH = os.path.abspath(args.lib)
    if args.digest:
        return digest()
    dev = torch.device('cuda', 0)
    g = torch.Generator(device=dev).manual_seed(0)
    total = 0.0
    for shp in SHAPES:
        shp = (args.frames,) + tuple(shp[1:])
        c = shp[-1]
        z = torch.randn(shp, device=dev, generator=g).to(torch.bfloat16)
        r = torch.randn(shp, device=dev, generator=g).to(torch.bfloat16)
        gy = torch.randn(shp, device=dev, generator=g).to(torch.bfloat16)
        gamma = torch.rand(c, device=dev) + 0.5
        beta = torch.randn(c, device=dev)
        nb = z.numel() * 2
        mean, rstd, sc, sh = T.bn_train_fwd(z, args.nseg, gamma, beta, 1e-5, 0.1)
        y = T.bn_apply(z, args.nseg, sc, sh, r, True)
        _, mask = T.bn_apply_mask(z, args.nseg, sc, sh, r)
        out = torch.empty_like(z)
        cases = [
            ('stats', lambda: T.bn_train_fwd(z, args.nseg, gamma, beta, 1e-5, 0.1), 1),
            ('apply', lambda: T.bn_apply(z, args.nseg, sc, sh, None, True, out=out), 2),
            ('apply+res', lambda: T.bn_apply(z, args.nseg, sc, sh, r, True, out=out), 3),
            ('bwd(y,gres)', lambda: T.bn_train_bwd(gy, y, z, args.nseg, mean, rstd, gamma, want_gres=True), 8),
            ('bwd(mask,gres)', lambda: T.bn_train_bwd(gy, None, z, args.nseg, mean, rstd, gamma, want_gres=True,
                                                      mask=mask), 6),
            ('bwd(relu_from)', lambda: T.bn_train_bwd(gy, None, z, args.nseg, mean, rstd, gamma, relu_from=(sc, sh)), 5),
        ]
        for name, fn, passes in cases:
            us = timeit(fn, args.reps, args.rounds)
            total += us
            print('%-22s %-14s %8.1f us  %5.2f TB/s' % (str(shp), name, us, passes * nb / us / 1e6))
    print('TOTAL %.1f us' % total)


if __name__ == '__main__':
    main()
