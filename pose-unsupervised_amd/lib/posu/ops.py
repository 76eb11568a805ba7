"""Tensor-level wrappers over libposeu.so entry points.

Every function here takes/returns torch tensors on a cuda (HIP) device, launches on
PyTorch's current stream, and raises if given CPU tensors: there is no fallback
path.  Autograd Functions wrap the kernels that the training step differentiates
through (soft-argmax, crop affine, epipolar loss, heatmap MSE, the heatmap
mutual-information pair scores and measures).
"""
import numpy as np
import torch

from . import _native as nat
from ._native import F32, BF16, F64, F16, F16X3, ptr, call, stream_of, require_cuda

_TORCH_OF = {F32: torch.float32, BF16: torch.bfloat16, F16: torch.float16, F16X3: torch.float16}


def dtype_code(dtype):
    if dtype in ('bf16', torch.bfloat16, BF16):
        return BF16
    if dtype in ('fp32', 'f32', torch.float32, F32):
        return F32
    if dtype in ('fp16', 'f16', torch.float16, F16):
        return F16
    if dtype in ('fp16x3', F16X3):
        return F16X3
    raise ValueError('unsupported compute dtype %r (bf16 | fp16 | fp16x3 | fp32)' % (dtype,))


def torch_dtype(code):
    return _TORCH_OF[code]


def cmul(code):
    """Stored elements per logical channel: 2 for the split dtype (a (hi, lo) fp16 pair,
    [hi 32 | lo 32] per 32-channel block, include/posu.h), else 1."""
    return 2 if code == F16X3 else 1


def channels(x, code):
    """Logical channel count of an NHWC activation tensor."""
    return x.shape[3] // cmul(code)


def widen(x, code):
    """NHWC activations -> f32 values (the split dtype's pairs summed: hi + lo is exact in f32)."""
    if code != F16X3:
        return x.float()
    n, h, w, c2 = x.shape
    t = x.view(n, h, w, c2 // 64, 2, 32).float()
    return (t[..., 0, :] + t[..., 1, :]).reshape(n, h, w, c2 // 2)


def conv_bk(code):
    return nat.load().posu_conv_bk(code)


# ---------------------------------------------------------------- layout ops
def pack_nchw_to_nhwc(x, code, cpad, out=None, hflip=False):
    """[N, C, H, W] f32 -> [N, H, W, cpad] (zero channels above C); hflip mirrors W."""
    require_cuda(x)
    x = x.contiguous().float()
    n, c, h, w = x.shape
    if out is None:
        out = torch.empty((n, h, w, cpad * cmul(code)), dtype=torch_dtype(code), device=x.device)
    call('posu_pack_nchw_to_nhwc', code, ptr(x), n, c, h, w, ptr(out), cpad, int(hflip), stream_of(x.device))
    return out


def pack_s2d_nchw(x, code, cpad, out=None, hflip=False):
    """[N, C, H, W] f32 -> space-to-depth [N, H/2, W/2, cpad] (channel (dy*2+dx)*C + c); hflip mirrors W."""
    require_cuda(x)
    x = x.contiguous().float()
    n, c, h, w = x.shape
    if out is None:
        out = torch.empty((n, h // 2, w // 2, cpad * cmul(code)), dtype=torch_dtype(code), device=x.device)
    call('posu_pack_s2d_nchw', code, ptr(x), n, c, h, w, ptr(out), cpad, int(hflip), stream_of(x.device))
    return out


def nhwc_to_nchw_f32(x, code):
    require_cuda(x)
    n, h, w, c = x.shape
    c //= cmul(code)
    out = torch.empty((n, c, h, w), dtype=torch.float32, device=x.device)
    call('posu_nhwc_to_nchw_f32', code, ptr(x), n, h, w, c, ptr(out), stream_of(x.device))
    return out


# ------------------------------------------------------------------ conv ops
def conv2d_nhwc(x, wpk, cout, kh, kw, stride, pad, scale, shift, residual, relu, code, out=None, out_hw=None,
                tile=-1):
    n, h, w, c = x.shape
    c //= cmul(code)
    ho = (h + 2 * pad - kh) // stride + 1
    wo = (w + 2 * pad - kw) // stride + 1
    if out_hw is not None:
        ho, wo = out_hw
    if out is None:
        out = torch.empty((n, ho, wo, cout * cmul(code)), dtype=x.dtype, device=x.device)
    call('posu_conv2d_fwd', code, ptr(x), n, h, w, c, ptr(wpk), cout, kh, kw, stride, pad,
         ptr(scale), ptr(shift), ptr(residual), int(relu), ptr(out), ho, wo, int(tile), stream_of(x.device))
    return out


def conv1x1_dual_nhwc(x, x2, stride2, wpk, cout, shift, relu, code, out=None, tile=-1, scale=None):  # noqa: D401
    """act((W[:, :C] x + W[:, C:] x2[::stride2, ::stride2]) * scale + shift) (two 1x1 sources, one
    output; scale None = 1)."""
    n, h, w, c = x.shape
    _, h2, w2, c2 = x2.shape
    c //= cmul(code)
    c2 //= cmul(code)
    if out is None:
        out = torch.empty((n, h, w, cout * cmul(code)), dtype=x.dtype, device=x.device)
    call('posu_conv1x1_dual_fwd', code, ptr(x), n, h, w, c, ptr(x2), h2, w2, c2, int(stride2), ptr(wpk), cout,
         ptr(scale), ptr(shift), int(relu), ptr(out), int(tile), stream_of(x.device))
    return out


def bottleneck_nhwc(x, w1, s1, b1, w2, s2, b2, w3, s3, b3, code, out=None):
    """Fused identity-residual Bottleneck (posu_bottleneck_fwd): x [N, H, W, C] -> y."""
    n, h, w, c = x.shape
    if out is None:
        out = torch.empty_like(x)
    call('posu_bottleneck_fwd', code, ptr(x), n, h, w, c, w1.shape[0], ptr(w1), ptr(s1), ptr(b1), ptr(w2), ptr(s2),
         ptr(b2), ptr(w3), ptr(s3), ptr(b3), ptr(out), stream_of(x.device))
    return out


def bottleneck_tail_stream_nhwc(t1, x, wstream, s2, b2, s3, b3, code, out=None):
    """conv2 + conv3 (+ residual) of a layer2 / layer3 identity Bottleneck with the weights
    streamed into registers (posu_bottleneck_tail_stream_fwd, csrc/tail_stream.hip; the split dtype
    also at layer1's shape); wstream = packing.pack_tail_stream(conv2 pack, conv3 pack)."""
    n, h, w, c = x.shape
    if out is None:
        out = torch.empty_like(x)
    call('posu_bottleneck_tail_stream_fwd', code, ptr(t1), ptr(x), n, h, w, c // cmul(code), t1.shape[3] // cmul(code),
         ptr(wstream),
         wstream.numel() * wstream.element_size(), ptr(s2), ptr(b2), ptr(s3), ptr(b3), ptr(out), stream_of(x.device))
    return out


def bottleneck_s2_tail_nhwc(t1, x, wstream, s2, b2, shift, code, out=None):
    """conv2 (3x3 / stride 2) + the conv3 | downsample dual GEMM of layer2's first Bottleneck in one
    launch (posu_bottleneck_s2_tail_fwd, csrc/tail_s2.hip): t1 [N, H, 64, 128], x [N, H, 64, 256] ->
    y [N, H/2, 32, 512]; wstream = packing.pack_s2_tail_stream(conv2 pack, dual pack)."""
    n, h, w, c = x.shape
    if out is None:
        out = torch.empty((n, h // 2, w // 2, shift.numel()), dtype=x.dtype, device=x.device)
    call('posu_bottleneck_s2_tail_fwd', code, ptr(t1), ptr(x), n, h, w, c, t1.shape[3], ptr(wstream),
         wstream.numel() * wstream.element_size(), ptr(s2), ptr(b2), ptr(shift), shift.numel(), ptr(out),
         stream_of(x.device))
    return out


def bottleneck_s2_tail_next_nhwc(t1, x, wstream, s2, b2, shift, s1n, b1n, code, out=None, t1n=None):
    """The strided tail chained with the next identity block's conv1 + BN1 + ReLU over y
    (posu_bottleneck_s2_tail_next_fwd); wstream = packing.pack_s2_tail_stream(conv2 pack, dual pack,
    next conv1 pack).  Returns (y, t1n) with t1n [N, H/2, 32, 128] bit-identical to a conv launch of
    the next conv1 over y."""
    n, h, w, c = x.shape
    if out is None:
        out = torch.empty((n, h // 2, w // 2, shift.numel()), dtype=x.dtype, device=x.device)
    if t1n is None:
        t1n = torch.empty((n, h // 2, w // 2, s1n.numel()), dtype=x.dtype, device=x.device)
    call('posu_bottleneck_s2_tail_next_fwd', code, ptr(t1), ptr(x), n, h, w, c, t1.shape[3], ptr(wstream),
         wstream.numel() * wstream.element_size(), ptr(s2), ptr(b2), ptr(shift), shift.numel(), ptr(out), ptr(s1n),
         ptr(b1n), ptr(t1n), stream_of(x.device))
    return out, t1n


def bottleneck_s2_front_tail_nhwc(x, s1, b1, wstream, s2, b2, shift, code, out=None):
    """The whole first Bottleneck of layer2 in one launch (posu_bottleneck_s2_front_tail_fwd): conv1 + BN1
    (s1, b1) + ReLU computed on each tile's window from x [N, H, 64, 256], then the strided tail -> y
    [N, H/2, 32, 512]; wstream = packing.pack_s2_tail_stream(conv2 pack, dual pack, w1=conv1 pack)."""
    n, h, w, c = x.shape
    if out is None:
        out = torch.empty((n, h // 2, w // 2, shift.numel()), dtype=x.dtype, device=x.device)
    call('posu_bottleneck_s2_front_tail_fwd', code, ptr(x), n, h, w, c, s2.numel(), ptr(s1), ptr(b1), ptr(wstream),
         wstream.numel() * wstream.element_size(), ptr(s2), ptr(b2), ptr(shift), shift.numel(), ptr(out),
         stream_of(x.device))
    return out


def bottleneck_s2_front_tail_next_nhwc(x, s1, b1, wstream, s2, b2, shift, s1n, b1n, code, out=None, t1n=None):
    """The same, chained with the next identity block's conv1 (posu_bottleneck_s2_front_tail_next_fwd;
    wstream = packing.pack_s2_tail_stream(conv2 pack, dual pack, next conv1 pack, w1=conv1 pack)).
    Returns (y, t1n) as bottleneck_s2_tail_next_nhwc."""
    n, h, w, c = x.shape
    if out is None:
        out = torch.empty((n, h // 2, w // 2, shift.numel()), dtype=x.dtype, device=x.device)
    if t1n is None:
        t1n = torch.empty((n, h // 2, w // 2, s1n.numel()), dtype=x.dtype, device=x.device)
    call('posu_bottleneck_s2_front_tail_next_fwd', code, ptr(x), n, h, w, c, s2.numel(), ptr(s1), ptr(b1),
         ptr(wstream), wstream.numel() * wstream.element_size(), ptr(s2), ptr(b2), ptr(shift), shift.numel(),
         ptr(out), ptr(s1n), ptr(b1n), ptr(t1n), stream_of(x.device))
    return out, t1n


def bottleneck_tail_stream_next_nhwc(t1, x, wstream, s2, b2, s3, b3, s1n, b1n, code, out=None, t1n=None):
    """The tail above chained with the NEXT identity block's conv1 + BN1 + ReLU over its output
    (posu_bottleneck_tail_stream_next_fwd); wstream = packing.pack_tail_stream(conv2 pack, conv3
    pack, next conv1 pack).  Returns (y, t1n): t1n is what a conv launch of the next conv1 over y
    would produce, bit for bit."""
    n, h, w, c = x.shape
    p = t1.shape[3]
    if out is None:
        out = torch.empty_like(x)
    if t1n is None:
        t1n = torch.empty((n, h, w, p), dtype=x.dtype, device=x.device)
    cm = cmul(code)
    call('posu_bottleneck_tail_stream_next_fwd', code, ptr(t1), ptr(x), n, h, w, c // cm, p // cm, ptr(wstream),
         wstream.numel() * wstream.element_size(), ptr(s2), ptr(b2), ptr(s3), ptr(b3), ptr(out), ptr(s1n), ptr(b1n),
         ptr(t1n), stream_of(x.device))
    return out, t1n


def bottleneck_tail_stream_chain_nhwc(t1, x, wstream, s2, b2, s3, b3, s1n, b1n, code, out=None, t1n=None):
    """The last identity block's tail of a layer chained with the NEXT layer's first conv1 + BN1 + ReLU
    (C -> Pn = s1n.numel() = 2 P; posu_bottleneck_tail_stream_chain_fwd, split fp16): (y, t1n [N, H, W, Pn])."""
    n, h, w, c = x.shape
    cm = cmul(code)
    p, pn = t1.shape[3] // cm, s1n.numel()
    if out is None:
        out = torch.empty_like(x)
    if t1n is None:
        t1n = torch.empty((n, h, w, pn * cm), dtype=x.dtype, device=x.device)
    call('posu_bottleneck_tail_stream_chain_fwd', code, ptr(t1), ptr(x), n, h, w, c // cm, p, pn, ptr(wstream),
         wstream.numel() * wstream.element_size(), ptr(s2), ptr(b2), ptr(s3), ptr(b3), ptr(out), ptr(s1n), ptr(b1n),
         ptr(t1n), stream_of(x.device))
    return out, t1n


def bottleneck_down_tail_stream_nhwc(t1, x, wstream, s2, b2, s3, b3, code, s1n=None, b1n=None, out=None, t1n=None):
    """Layer1's first Bottleneck after its conv1 in split fp16 (posu_bottleneck_down_tail_stream_fwd):
    conv2 + the [conv3 | downsample] dual GEMM (scale s3, shift b3) + ReLU in one launch, t1 / x
    [N, H, 64, 64] -> y [N, H, 64, 256] (logical channels); with s1n / b1n also the next identity block's
    conv1 + BN1 + ReLU over y.  Returns (y, t1n or None)."""
    n, h, w, _ = x.shape
    cm = cmul(code)
    c = s3.numel()
    if out is None:
        out = torch.empty((n, h, w, c * cm), dtype=x.dtype, device=x.device)
    if s1n is not None and t1n is None:
        t1n = torch.empty_like(t1)
    call('posu_bottleneck_down_tail_stream_fwd', code, ptr(t1), ptr(x), n, h, w, c, t1.shape[3] // cm, ptr(wstream),
         wstream.numel() * wstream.element_size(), ptr(s2), ptr(b2), ptr(s3), ptr(b3), ptr(out), ptr(s1n), ptr(b1n),
         ptr(t1n if s1n is not None else None), stream_of(x.device))
    return out, (t1n if s1n is not None else None)


def bottleneck_down_nhwc(x, w1, s1, b1, w2, s2, b2, w3d, shift3, code, out=None):
    """Fused first Bottleneck of layer1 with its downsample (posu_bottleneck_down_fwd):
    x [N, H, W, C] -> y [N, H, W, w3d.shape[0]]."""
    n, h, w, c = x.shape
    if out is None:
        out = torch.empty((n, h, w, w3d.shape[0]), dtype=x.dtype, device=x.device)
    call('posu_bottleneck_down_fwd', code, ptr(x), n, h, w, c, w1.shape[0], ptr(w1), ptr(s1), ptr(b1), ptr(w2),
         ptr(s2), ptr(b2), ptr(w3d), ptr(shift3), ptr(out), stream_of(x.device))
    return out


def deconv4x4s2_nhwc(x, wpk, cout, scale, shift, relu, code, out=None, tile=-1):
    n, h, w, c = x.shape
    c //= cmul(code)
    if out is None:
        out = torch.empty((n, 2 * h, 2 * w, cout * cmul(code)), dtype=x.dtype, device=x.device)
    call('posu_deconv4x4s2_fwd', code, ptr(x), n, h, w, c, ptr(wpk), cout, ptr(scale), ptr(shift),
         int(relu), ptr(out), int(tile), stream_of(x.device))
    return out


def deconv4x4s2_head(x, wpk, cout, scale, shift, head_w, njoints, head_b, code, keep_f=True, hm_out=None,
                     f_out=None, head_w_lo=None):
    """Last deconv + BN + ReLU fused with the 1x1 head: returns (heatmaps NCHW f32, f NHWC or None).
    head_w_lo (2-byte dtypes): the head weight's rounding residual -> the split-precision head."""
    n, h, w, c = x.shape
    c //= cmul(code)
    if hm_out is None:
        hm_out = torch.empty((n, njoints, 2 * h, 2 * w), dtype=torch.float32, device=x.device)
    if keep_f and f_out is None:
        f_out = torch.empty((n, 2 * h, 2 * w, cout * cmul(code)), dtype=x.dtype, device=x.device)
    call('posu_deconv4x4s2_head_fwd', code, ptr(x), n, h, w, c, ptr(wpk), cout, ptr(scale), ptr(shift),
         ptr(f_out if keep_f else None), ptr(head_w), ptr(head_w_lo), njoints, ptr(head_b), ptr(hm_out),
         stream_of(x.device))
    return hm_out, (f_out if keep_f else None)


def head1x1_nchw(x, wpk, cout, bias, code, out=None):
    n, h, w, c = x.shape
    c //= cmul(code)
    if out is None:
        out = torch.empty((n, cout, h, w), dtype=torch.float32, device=x.device)
    call('posu_head1x1_nchw_fwd', code, ptr(x), n, h, w, c, ptr(wpk), cout, ptr(bias), ptr(out),
         stream_of(x.device))
    return out


def stem_pool_views(views, wpk, scale, shift, code, out=None, hflip=False):
    """stem_pool over the views of one forward in ONE launch (posu_stem_pool_views_fwd): a list of
    NCHW f32 [Nv, 3, H, W] tensors (same shape) -> NHWC [V * Nv, H/4, W/4, 64], view-major."""
    import ctypes
    if not views or not all(v.is_cuda for v in views):
        raise RuntimeError('stem_pool_views: HIP op needs GPU tensors')
    n, c, h, w = views[0].shape
    if c != 3 or any(tuple(v.shape) != (n, c, h, w) for v in views):
        raise ValueError('stem_pool_views: views of one shape [N, 3, H, W] expected')
    views = [v.contiguous().float() for v in views]
    if out is None:
        out = torch.empty((n * len(views), h // 4, w // 4, 64 * cmul(code)), dtype=torch_dtype(code),
                          device=views[0].device)
    arr = (ctypes.c_void_p * len(views))(*[v.data_ptr() for v in views])
    call('posu_stem_pool_views_fwd', code, ctypes.cast(arr, ctypes.c_void_p), len(views), n, h, w, int(bool(hflip)),
         ptr(wpk), ptr(scale), ptr(shift), ptr(out), stream_of(views[0].device))
    return out


def stem_pool(x, wpk, scale, shift, code, out=None, hflip=False):
    """Fused input pack + 7x7/s2 stem + BN + ReLU + 3x3/s2 max-pool: NCHW f32 [N, 3, H, W]
    -> NHWC [N, H/4, W/4, 64] (compute dtype)."""
    if not x.is_cuda:
        raise RuntimeError('stem_pool: HIP op needs a GPU tensor')
    n, c, h, w = x.shape
    if c != 3:
        raise ValueError('stem_pool: 3 input channels expected')
    x = x.contiguous().float()
    if out is None:
        out = torch.empty((n, h // 4, w // 4, 64 * cmul(code)), dtype=torch_dtype(code), device=x.device)
    call('posu_stem_pool_fwd', code, ptr(x), n, h, w, int(bool(hflip)), ptr(wpk), ptr(scale), ptr(shift), ptr(out),
         stream_of(x.device))
    return out


def maxpool3x3s2_nhwc(x, code, out=None):
    n, h, w, c = x.shape
    ho, wo = (h - 1) // 2 + 1, (w - 1) // 2 + 1
    if out is None:
        out = torch.empty((n, ho, wo, c), dtype=x.dtype, device=x.device)
    call('posu_maxpool3x3s2_fwd', code, ptr(x), n, h, w, c // cmul(code), ptr(out), stream_of(x.device))
    return out


# ------------------------------------------------------------ heatmap decode
class _SoftArgmax(torch.autograd.Function):
    @staticmethod
    def forward(ctx, hm, beta, affine):
        hm = hm.contiguous()
        n, j, h, w = hm.shape
        out = torch.empty((n, j, 2), dtype=torch.float32, device=hm.device)
        stats = torch.empty((n, j, 4), dtype=torch.float32, device=hm.device)
        call('posu_softargmax2d_fwd', ptr(hm), n, j, h, w, float(beta), ptr(affine), ptr(out), ptr(stats),
             stream_of(hm.device))
        ctx.save_for_backward(hm, stats, affine)
        ctx.beta = beta
        return out

    @staticmethod
    def backward(ctx, gout):
        hm, stats, affine = ctx.saved_tensors
        n, j, h, w = hm.shape
        gout = gout.contiguous().float()
        ghm = torch.empty_like(hm)
        call('posu_softargmax2d_bwd', ptr(hm), ptr(stats), n, j, h, w, float(ctx.beta), ptr(affine), ptr(gout),
             ptr(ghm), stream_of(hm.device))
        return ghm, None, None


def softargmax2d(hm, beta=100.0, affine=None):
    """[N, J, H, W] f32 heatmaps -> [N, J, 2] (x=col, y=row); affine [N, 2, 3] maps to image px."""
    require_cuda(hm, affine)
    if hm.dtype != torch.float32:
        raise TypeError('soft-argmax expects float32 heatmaps (got %s)' % hm.dtype)
    if affine is not None:
        affine = affine.to(device=hm.device, dtype=torch.float32).contiguous()
    return _SoftArgmax.apply(hm, beta, affine)


class _Affine2d(torch.autograd.Function):
    @staticmethod
    def forward(ctx, pts, T):
        pts = pts.contiguous().float()
        n, j, _ = pts.shape
        out = torch.empty_like(pts)
        call('posu_affine2d_apply', ptr(pts), ptr(T), n, j, 0, ptr(out), stream_of(pts.device))
        ctx.save_for_backward(T)
        return out

    @staticmethod
    def backward(ctx, g):
        (T,) = ctx.saved_tensors
        g = g.contiguous().float()
        n, j, _ = g.shape
        gin = torch.empty_like(g)
        call('posu_affine2d_apply', ptr(g), ptr(T), n, j, 1, ptr(gin), stream_of(g.device))
        return gin, None


def affine2d(pts, T):
    """[N, J, 2] @ per-sample [N, 2, 3] affine (homogeneous)."""
    require_cuda(pts)
    T = T.to(device=pts.device, dtype=torch.float32).contiguous()
    return _Affine2d.apply(pts, T)


def argmax2d(hm, post_process=True, affine64=None):
    """get_final_preds on device: returns (preds [N, J, 2] f32, maxvals [N, J, 1] f32)."""
    require_cuda(hm)
    hm = hm.contiguous().float()
    n, j, h, w = hm.shape
    if affine64 is not None:
        affine64 = affine64.to(device=hm.device, dtype=torch.float64).contiguous()
    preds = torch.empty((n, j, 2), dtype=torch.float32, device=hm.device)
    maxv = torch.empty((n, j, 1), dtype=torch.float32, device=hm.device)
    call('posu_argmax2d_fwd', ptr(hm), n, j, h, w, int(bool(post_process)), ptr(affine64), ptr(preds), ptr(maxv),
         stream_of(hm.device))
    return preds, maxv


def flip_back(hm_flipped, perm=None, hm=None, shift=False, out=None):
    """Flip-test heatmaps back (mirror W, permute joints by `perm`, optional one-column
    shift) and, with `hm`, average: 0.5 * (hm + flip_back(hm_flipped))."""
    require_cuda(hm_flipped)
    hf = hm_flipped.contiguous().float()
    n, j, h, w = hf.shape
    if perm is not None and not isinstance(perm, torch.Tensor):
        perm = torch.tensor(list(perm), dtype=torch.int32)
    if perm is not None:
        perm = perm.to(device=hf.device, dtype=torch.int32).contiguous()
    if hm is not None:
        hm = hm.contiguous().float()
    if out is None:
        out = torch.empty_like(hf)
    call('posu_flip_back', ptr(hf), ptr(perm), ptr(hm), n, j, h, w, int(bool(shift)), ptr(out), stream_of(hf.device))
    return out


# ----------------------------------------------------------------- losses
class _Epipolar(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, w, F, subj):
        x = x.contiguous().float()
        v, n, j, _ = x.shape
        s = F.shape[0]
        loss = torch.empty((), dtype=torch.float32, device=x.device)
        call('posu_epipolar_loss_fwd', ptr(x), ptr(w), ptr(F), ptr(subj), v, n, j, s, ptr(loss), None,
             stream_of(x.device))
        ctx.save_for_backward(x, w, F, subj)
        return loss

    @staticmethod
    def backward(ctx, gloss):
        x, w, F, subj = ctx.saved_tensors
        v, n, j, _ = x.shape
        gloss = gloss.contiguous().float().reshape(1)
        gx = torch.empty_like(x)
        call('posu_epipolar_loss_bwd', ptr(x), ptr(w), ptr(F), ptr(subj), v, n, j, F.shape[0], ptr(gloss),
             ptr(gx), stream_of(x.device))
        return gx, None, None, None


def epipolar_loss(x, w, F, subj):
    """x [V, N, J, 2] image px; w [V, N, J] or None; F [S, V(V-1), 3, 3]; subj [N] int32."""
    require_cuda(x, w, F, subj)
    if w is not None:
        w = w.contiguous().float()
    return _Epipolar.apply(x, w, F.contiguous().float(), subj.contiguous().int())


def epipolar_residuals(x, w, F, subj):
    """Per (sample, pair, joint) weighted |x_j^T F x_i| [N, P, J] (no autograd)."""
    require_cuda(x, w, F, subj)
    x = x.contiguous().float()
    v, n, j, _ = x.shape
    p = v * (v - 1)
    loss = torch.empty((), dtype=torch.float32, device=x.device)
    resid = torch.empty((n, p, j), dtype=torch.float32, device=x.device)
    call('posu_epipolar_loss_fwd', ptr(x), ptr(None if w is None else w.contiguous().float()),
         ptr(F.contiguous().float()), ptr(subj.contiguous().int()), v, n, j, F.shape[0], ptr(loss), ptr(resid),
         stream_of(x.device))
    return resid, loss


class _JointsMSE(torch.autograd.Function):
    @staticmethod
    def forward(ctx, pred, gt, w):
        n, j = pred.shape[:2]
        hw = pred[0, 0].numel()
        pred = pred.contiguous().float()
        gt = gt.contiguous().float()
        ws = torch.empty((n * j,), dtype=torch.float32, device=pred.device)
        loss = torch.empty((), dtype=torch.float32, device=pred.device)
        call('posu_joints_mse_fwd', ptr(pred), ptr(gt), ptr(w), n, j, hw, ptr(ws), ptr(loss), stream_of(pred.device))
        ctx.save_for_backward(pred, gt, w)
        return loss

    @staticmethod
    def backward(ctx, gloss):
        pred, gt, w = ctx.saved_tensors
        n, j = pred.shape[:2]
        hw = pred[0, 0].numel()
        gloss = gloss.contiguous().float().reshape(1)
        gpred = torch.empty_like(pred)
        call('posu_joints_mse_bwd', ptr(pred), ptr(gt), ptr(w), n, j, hw, ptr(gloss), ptr(gpred),
             stream_of(pred.device))
        return gpred, None, None


def joints_mse(pred, gt, w=None):
    require_cuda(pred, gt, w)
    if w is not None:
        w = w.reshape(pred.shape[0], pred.shape[1]).contiguous().float()
    return _JointsMSE.apply(pred, gt, w)


class _MSEMean(torch.autograd.Function):
    """mean((a - b)^2) with a gradient for both arguments (the JointsMSE kernels, unweighted: a sum of
    per-joint means / J; d/db = -d/da)."""

    @staticmethod
    def forward(ctx, a, b):
        n, j = a.shape[:2]
        hw = a[0, 0].numel()
        a = a.contiguous().float()
        b = b.contiguous().float()
        ws = torch.empty((n * j,), dtype=torch.float32, device=a.device)
        loss = torch.empty((), dtype=torch.float32, device=a.device)
        call('posu_joints_mse_fwd', ptr(a), ptr(b), None, n, j, hw, ptr(ws), ptr(loss), stream_of(a.device))
        ctx.save_for_backward(a, b)
        return loss / j

    @staticmethod
    def backward(ctx, gloss):
        a, b = ctx.saved_tensors
        n, j = a.shape[:2]
        hw = a[0, 0].numel()
        gloss = (gloss.contiguous().float() / j).reshape(1)
        ga = torch.empty_like(a)
        call('posu_joints_mse_bwd', ptr(a), ptr(b), None, n, j, hw, ptr(gloss), ptr(ga), stream_of(a.device))
        return (ga if ctx.needs_input_grad[0] else None), (-ga if ctx.needs_input_grad[1] else None)


def mse_mean(a, b):
    """torch.nn.MSELoss(reduction='mean') of two [N, J, ...] f32 cuda tensors on the JointsMSE kernels,
    differentiable in both (the training loop's consistent loss, function.py:291-296)."""
    require_cuda(a, b)
    if a.shape != b.shape or a.dim() < 3:
        raise ValueError('mse_mean: two [N, J, ...] tensors of one shape expected')
    return _MSEMean.apply(a, b)


# -------------------------------------------------------------- triangulation
def triangulate_dlt(M, intr, xy, vis=None, undistort=True, view_major=False):
    """M [G, V, 3, 4] f64, intr [G, V, 9] f64, xy [G, V, J, 2] (or [V, G, J, 2] with view_major) f32|f64,
    vis [G, V, J] u8 -> X [G, J, 3] f64."""
    require_cuda(M, intr, xy, vis)
    if view_major:
        v, g, j, _ = xy.shape
        sg, sv = j * 2, g * j * 2
    else:
        g, v, j, _ = xy.shape
        sg, sv = v * j * 2, j * 2
    M = M.contiguous().double()
    intr = intr.contiguous().double()
    xy = xy.contiguous()
    if xy.dtype == torch.float64:
        code = F64
    else:
        xy = xy.float()
        code = F32
    if vis is not None:
        vis = vis.contiguous().to(torch.uint8)
    X = torch.empty((g, j, 3), dtype=torch.float64, device=xy.device)
    call('posu_triangulate_dlt', ptr(M), ptr(intr), ptr(xy), code, sg, sv, ptr(vis), g, v, j, int(bool(undistort)),
         ptr(X), stream_of(xy.device))
    return X


def ransac_inliers(M, intr, xy, vis=None, reproj_thre=20.0, min_inliers=2, undistort=True):
    """multiviews.triangulate.ransac on device: M [G, V, 3, 4] f64, intr [G, V, 9] f64,
    xy [G, V, J, 2], vis [G, V, J] -> res_vis [G, V, J] uint8."""
    require_cuda(M, intr, xy)
    g, v, j, _ = xy.shape
    xy = xy.to(torch.float64).contiguous()
    if vis is not None:
        vis = vis.to(device=xy.device, dtype=torch.uint8).contiguous()
    out = torch.empty((g, v, j), dtype=torch.uint8, device=xy.device)
    call('posu_ransac_inliers', ptr(M.contiguous()), ptr(intr.contiguous()), ptr(xy), ptr(vis), g, v, j,
         int(bool(undistort)), float(reproj_thre), int(min_inliers), ptr(out), stream_of(xy.device))
    return out


def reproject(M, intr, xy, vis=None, undistort=True):
    """multiviews.triangulate.reproject_poses on device -> (proj [G, V, J, 2] f64, res_vis [G, V, J] uint8)."""
    require_cuda(M, intr, xy)
    g, v, j, _ = xy.shape
    xy = xy.to(torch.float64).contiguous()
    if vis is not None:
        vis = vis.to(device=xy.device, dtype=torch.uint8).contiguous()
    proj = torch.empty((g, v, j, 2), dtype=torch.float64, device=xy.device)
    res = torch.empty((g, v, j), dtype=torch.uint8, device=xy.device)
    call('posu_reproject', ptr(M.contiguous()), ptr(intr.contiguous()), ptr(xy), ptr(vis), g, v, j,
         int(bool(undistort)), ptr(proj), ptr(res), stream_of(xy.device))
    return proj, res


# ------------------------------------- differentiable triangulation, reprojection loss
def _tri_args(M, intr, xy, vis, weights, target_weight, view_major):
    """The tensors of the differentiable entry points in the layouts include/posu.h asks for: xy keeps its
    layout (f64 stays, everything else is read as f32), the [G, V, J] tables are group-major f64."""
    require_cuda(M, intr, xy, vis, weights, target_weight)
    if view_major:
        v, g, j, _ = xy.shape
        sg, sv = j * 2, g * j * 2
    else:
        g, v, j, _ = xy.shape
        sg, sv = v * j * 2, j * 2
    if not 2 <= v <= 4:
        raise ValueError('the differentiable triangulation takes 2 to 4 views, got %d' % v)
    M = M.detach().contiguous().double()
    intr = intr.detach().contiguous().double()
    if vis is not None:
        vis = vis.reshape(g, v, j).ne(0).to(torch.uint8).contiguous()
    if weights is not None:
        weights = weights.reshape(g, v, j)
    if target_weight is not None:
        target_weight = target_weight.detach().reshape(g, v, j).contiguous().double()
    return M, intr, vis, weights, target_weight, (g, v, j, sg, sv)


def _xy_storage(xy):
    xy = xy.detach().contiguous()
    return (xy, F64) if xy.dtype == torch.float64 else (xy.float(), F32)


class _TriangulatePoints(torch.autograd.Function):
    @staticmethod
    def forward(ctx, xy, w, M, intr, vis, dims, undistort):
        g, v, j, sg, sv = dims
        xs, code = _xy_storage(xy)
        ws = None if w is None else w.detach().contiguous().double()
        X = torch.empty((g, j, 3), dtype=torch.float64, device=xy.device)
        call('posu_triangulate_dlt_w', ptr(M), ptr(intr), ptr(xs), code, sg, sv, ptr(vis), ptr(ws), g, v, j,
             undistort, ptr(X), stream_of(xy.device))
        ctx.save_for_backward(xs, ws, M, intr, vis)
        ctx.args = (code, dims, undistort, xy.dtype, None if w is None else w.dtype)
        return X

    @staticmethod
    def backward(ctx, gX):
        xs, ws, M, intr, vis = ctx.saved_tensors
        code, (g, v, j, sg, sv), undistort, xy_dtype, w_dtype = ctx.args
        gX = gX.contiguous().double()
        gxy = torch.empty_like(xs)
        gw = None if ws is None else torch.empty_like(ws)
        call('posu_triangulate_dlt_bwd', ptr(M), ptr(intr), ptr(xs), code, sg, sv, ptr(vis), ptr(ws), g, v, j,
             undistort, ptr(gX), ptr(gxy), ptr(gw), stream_of(xs.device))
        return (gxy.to(xy_dtype), None if gw is None else gw.to(w_dtype), None, None, None, None, None)


def triangulate_points(M, intr, xy, vis=None, weights=None, undistort=True, view_major=False):
    """triangulate_dlt for 2 to 4 views with a gradient: differentiable in xy and in weights, the optional
    [G, V, J] confidence that multiplies the two DLT rows of a view.  M [G, V, 3, 4], intr [G, V, 9],
    xy [G, V, J, 2] (or [V, G, J, 2] with view_major) f32|f64, vis [G, V, J] -> X [G, J, 3] f64."""
    M, intr, vis, weights, _, dims = _tri_args(M, intr, xy, vis, weights, None, view_major)
    return _TriangulatePoints.apply(xy, weights, M, intr, vis, dims, int(bool(undistort)))


class _ReprojectionLoss(torch.autograd.Function):
    @staticmethod
    def forward(ctx, xy, w, M, intr, vis, omega, dims, undistort, detach_point):
        g, v, j, sg, sv = dims
        if g == 0:
            raise ValueError('reprojection_loss: empty batch (the mean over G V J residuals is undefined)')
        dev = xy.device
        xs, code = _xy_storage(xy)
        ws = None if w is None else w.detach().contiguous().double()
        loss = torch.empty((), dtype=torch.float64, device=dev)
        X = torch.empty((g, j, 3), dtype=torch.float64, device=dev)
        nbytes = nat.load().posu_reprojection_loss_workspace(g, j)
        if nbytes < 0:
            raise ValueError('reprojection_loss: bad shape G = %d, J = %d' % (g, j))
        workspace = torch.empty((nbytes // 8,), dtype=torch.float64, device=dev)
        call('posu_reprojection_loss_fwd', ptr(M), ptr(intr), ptr(xs), code, sg, sv, ptr(vis), ptr(ws), ptr(omega),
             g, v, j, undistort, ptr(loss), ptr(X), None, ptr(workspace), nbytes, stream_of(dev))
        ctx.save_for_backward(xs, ws, M, intr, vis, omega)
        ctx.args = (code, dims, undistort, detach_point, xy.dtype, None if w is None else w.dtype)
        ctx.mark_non_differentiable(X)
        return loss, X

    @staticmethod
    def backward(ctx, gloss, _gX):
        xs, ws, M, intr, vis, omega = ctx.saved_tensors
        code, (g, v, j, sg, sv), undistort, detach_point, xy_dtype, w_dtype = ctx.args
        gloss = gloss.contiguous().double().reshape(1)
        gxy = torch.empty_like(xs)
        gw = None if ws is None else torch.empty_like(ws)
        call('posu_reprojection_loss_bwd', ptr(M), ptr(intr), ptr(xs), code, sg, sv, ptr(vis), ptr(ws), ptr(omega),
             g, v, j, undistort, detach_point, ptr(gloss), ptr(gxy), ptr(gw), stream_of(xs.device))
        return (gxy.to(xy_dtype), None if gw is None else gw.to(w_dtype)) + (None,) * 7


def reprojection_loss(M, intr, xy, vis=None, weights=None, target_weight=None, undistort=True, view_major=False,
                      detach_point=False, return_points=False):
    """The n-view reprojection-consistency loss (2 to 4 views): triangulate the predictions of all views (row
    weights `weights`, as triangulate_points), project the point into every view with the lens model and average
    the pixel distance to the predictions, weighted by `target_weight` [G, V, J]: sum / (G V J), an f64 scalar.
    Differentiable in xy and weights; with detach_point the point is a constant (the online pseudo-label reading)
    and only the direct term reaches xy.  return_points: -> (loss, X [G, J, 3] f64, no gradient)."""
    M, intr, vis, weights, omega, dims = _tri_args(M, intr, xy, vis, weights, target_weight, view_major)
    loss, X = _ReprojectionLoss.apply(xy, weights, M, intr, vis, omega, dims, int(bool(undistort)),
                                      int(bool(detach_point)))
    return (loss, X) if return_points else loss


def reprojection_residuals(M, intr, xy, vis=None, weights=None, undistort=True, view_major=False):
    """The loss's per-view pixel distances e [G, V, J] f64 and its points X [G, J, 3] f64 (no autograd)."""
    M, intr, vis, weights, _, (g, v, j, sg, sv) = _tri_args(M, intr, xy, vis, weights, None, view_major)
    dev = xy.device
    xs, code = _xy_storage(xy)
    ws = None if weights is None else weights.detach().contiguous().double()
    loss = torch.empty((), dtype=torch.float64, device=dev)
    X = torch.empty((g, j, 3), dtype=torch.float64, device=dev)
    e = torch.empty((g, v, j), dtype=torch.float64, device=dev)
    nbytes = nat.load().posu_reprojection_loss_workspace(g, j)
    workspace = torch.empty((max(nbytes, 8) // 8,), dtype=torch.float64, device=dev)
    call('posu_reprojection_loss_fwd', ptr(M), ptr(intr), ptr(xs), code, sg, sv, ptr(vis), ptr(ws), None, g, v, j,
         int(bool(undistort)), ptr(loss), ptr(X), ptr(e), ptr(workspace), nbytes, stream_of(dev))
    return e, X


# ----------------------------------------------------------------------- RPSM
RPSM_MAX_BINS = 4096


class RpsmTree:
    """The skeleton tree as the three host int arrays the RPSM entry points read
    (include/posu.h): parent [J] (root = -1), child_ptr [J + 1], child_idx [J - 1]."""

    def __init__(self, parents, children):
        import numpy as np
        self.parent = np.ascontiguousarray(parents, dtype=np.int32)
        self.njoints = len(self.parent)
        self.child_ptr = np.zeros(self.njoints + 1, dtype=np.int32)
        self.child_ptr[1:] = np.cumsum([len(c) for c in children])
        self.child_idx = np.ascontiguousarray([c for cs in children for c in cs] + [0], dtype=np.int32)
        self.edges = [(j, c) for j, cs in enumerate(children) for c in cs]   # mask row e <-> edges[e]

    def args(self):
        return _host(self.parent), _host(self.child_ptr), _host(self.child_idx)

    def by_child(self, values, what='limb_length'):
        """dict keyed (parent, child) -> host f64 [J] indexed by the child joint; an array [J] is
        taken as already in that form."""
        import numpy as np
        if not isinstance(values, dict):
            out = np.ascontiguousarray(values, dtype=np.float64)
            if out.shape != (self.njoints,):
                raise ValueError('%s must be a dict keyed (parent, child) or [J] by child joint' % what)
            return out
        out = np.zeros(self.njoints, dtype=np.float64)
        for p, c in self.edges:
            if (p, c) not in values:
                raise KeyError('%s has no entry for edge %r' % (what, (p, c)))
            out[c] = float(values[(p, c)])
        return out


def _host(a):
    import ctypes
    return ctypes.c_void_p(a.ctypes.data)


def _cube(nbins):
    nbins = int(nbins)
    return nbins, nbins * nbins * nbins


def rpsm_grid(centers, size, nbins):
    """compute_grid for a batch of boxes: centers [..., 3] f64 -> grid [..., nbins^3, 3] f64."""
    require_cuda(centers)
    nbins, n = _cube(nbins)
    centers = centers.contiguous().double()
    lead = tuple(centers.shape[:-1])
    grid = torch.empty(lead + (n, 3), dtype=torch.float64, device=centers.device)
    call('posu_rpsm_grid', ptr(centers), centers.numel() // 3, float(size), nbins, ptr(grid), stream_of(centers.device))
    return grid


def rpsm_unary(heatmaps, cams, affine, grid, image_size):
    """heatmaps [G, V, J, H, W] f32, cams [G, V, 20] f64, affine [G, V, 2, 3] f64, grid [G, 1 | J, N, 3] f64,
    image_size (w, h) -> unary [G, J, N] f64."""
    require_cuda(heatmaps, cams, affine, grid)
    g, v, j, h, w = heatmaps.shape
    heatmaps = heatmaps.contiguous().float()
    ng, n = grid.shape[1], grid.shape[2]
    unary = torch.empty((g, j, n), dtype=torch.float64, device=heatmaps.device)
    call('posu_rpsm_unary', ptr(heatmaps), ptr(cams.contiguous().double()), ptr(affine.contiguous().double()),
         g, v, j, h, w, float(image_size[0]), float(image_size[1]), ptr(grid.contiguous().double()), ng, n,
         ptr(unary), stream_of(heatmaps.device))
    return unary


def rpsm_infer(unary, tree, mask=None, grid=None, limb=None, tolerance=0.0, pose_grid=None):
    """One grid level of max-product inference.  unary [G, J, N] f64; the pairwise term is either
    mask [J - 1, ceil(N / 32), N] int32 (packed bits) or computed from grid [G, 1 | J, N, 3], limb (f64 [G, J]
    on the device, by child joint, a row per group) and tolerance.  -> (bins [G, J] int32, pose [G, J, 3] f64 or None, energy [G, J, N],
    maxv [G, J, N], state [G, J, N] int32).  pose needs a grid (pose_grid, default grid)."""
    require_cuda(unary, mask, grid, pose_grid, limb)
    unary = unary.contiguous().double()
    g, j, n = unary.shape
    dev = unary.device
    energy, maxv = torch.empty_like(unary), torch.zeros_like(unary)
    state = torch.zeros((g, j, n), dtype=torch.int32, device=dev)
    if mask is not None:
        mask = mask.contiguous()
        if mask.dtype != torch.int32 or tuple(mask.shape) != (j - 1, (n + 31) // 32, n):
            raise ValueError('mask must be int32 [J - 1, ceil(N / 32), N], got %s %s' % (mask.dtype, tuple(mask.shape)))
    if grid is not None:
        grid = grid.contiguous().double()
    if limb is not None:
        limb = _limb_table(limb, g, j)
    call('posu_rpsm_infer', ptr(unary), *tree.args(), ptr(mask), ptr(grid), 1 if grid is None else grid.shape[1],
         ptr(limb), float(tolerance), g, j, n, ptr(energy), ptr(maxv), ptr(state),
         stream_of(dev))
    pg = grid if pose_grid is None else pose_grid.contiguous().double()
    bins = torch.empty((g, j), dtype=torch.int32, device=dev)
    pose = None if pg is None else torch.empty((g, j, 3), dtype=torch.float64, device=dev)
    pg_ptr, ngp = ptr(pg), (1 if pg is None else pg.shape[1])
    call('posu_rpsm_backtrack', ptr(energy), ptr(state), *tree.args(), pg_ptr, ngp, g, j, n, ptr(bins), ptr(pose),
         stream_of(dev))
    return bins, pose, energy, maxv, state


def _limb_table(limb, g, j):
    limb = limb.contiguous().double()
    if tuple(limb.shape) != (g, j):
        raise ValueError('limb lengths must be [G, J] = [%d, %d] (a row per group, by child joint), got %s'
                         % (g, j, tuple(limb.shape)))
    return limb


def rpsm_pairwise_mask(grid, tree, limb, thr, strict):
    """grid [1 | J, N, 3] f64 -> packed constraint [J - 1, ceil(N / 32), N] int32 of every edge:
    |norm(g_p[i] - g_c[j]) - limb[c]| < thr[c] (strict) or <= thr[c]; limb, thr host f64 [J] by child."""
    require_cuda(grid)
    grid = grid.contiguous().double()
    ng, n = grid.shape[0], grid.shape[1]
    mask = torch.empty((tree.njoints - 1, (n + 31) // 32, n), dtype=torch.int32, device=grid.device)
    call('posu_rpsm_pairwise_mask', ptr(grid), ng, n, *tree.args(), tree.njoints, _host(limb), _host(thr),
         int(bool(strict)), ptr(mask), stream_of(grid.device))
    return mask


def rpsm_run(heatmaps, cams, affine, image_size, grid_centers, grid_size, first_nbins, recur_nbins, recur_depth,
             tolerance, limb, mask, tree, return_levels=False):
    """The whole recursion for G groups in one enqueue (posu_rpsm_run) -> pose [G, J, 3] f64 (and, with
    return_levels, [recur_depth + 1, G, J, 3]: the pose after level 1 and after every refinement).
    limb: f64 [G, J] on the device, every group's limb lengths by child joint."""
    require_cuda(heatmaps, cams, affine, grid_centers, mask, limb)
    g, v, j, h, w = heatmaps.shape
    dev = heatmaps.device
    heatmaps = heatmaps.contiguous().float()
    first_nbins, n1 = _cube(first_nbins)
    recur_nbins, _ = _cube(recur_nbins)
    mask = mask.contiguous()
    if mask.dtype != torch.int32 or tuple(mask.shape) != (j - 1, (n1 + 31) // 32, n1):
        raise ValueError('the level-1 constraint must be int32 [J - 1, ceil(N / 32), N] for N = %d bins, got %s %s'
                         % (n1, mask.dtype, tuple(mask.shape)))
    limb = _limb_table(limb, g, j)
    nbytes = nat.load().posu_rpsm_workspace_bytes(g, j, first_nbins, recur_nbins)
    work = torch.empty((max(int(nbytes), 0) + 8,), dtype=torch.uint8, device=dev)
    pose = torch.empty((g, j, 3), dtype=torch.float64, device=dev)
    levels = torch.empty((int(recur_depth) + 1, g, j, 3), dtype=torch.float64, device=dev) if return_levels else None
    call('posu_rpsm_run', ptr(heatmaps), ptr(cams.contiguous().double()), ptr(affine.contiguous().double()), g, v, j,
         h, w, float(image_size[0]), float(image_size[1]), ptr(grid_centers.contiguous().double()), float(grid_size),
         first_nbins, recur_nbins, int(recur_depth), float(tolerance), ptr(limb), ptr(mask), *tree.args(),
         ptr(work), int(nbytes), ptr(pose), ptr(levels), stream_of(dev))
    return (pose, levels) if return_levels else pose


# ------------------------------------------------------- heatmap mutual-information loss
MI_MEASURES = {'JSD': 0, 'NCE': 1}
# order of the parameter table of posu_heatmap_pair_scores_* (include/posu.h)
_MI_PARAMS = ('W1', 'g1', 'be1', 'rm1', 'rv1', 'W2', 'b2', 'g2', 'be2', 'rm2', 'rv2', 'w3', 'b3')
_MI_GRADS = ('W1', 'g1', 'be1', 'W2', 'b2', 'g2', 'be2', 'w3', 'b3')   # dparams order


def heatmap_mi_workspace(nseg, n, q, cm):
    """(bytes, bytes of it that do not grow with the pairs) of the pair-score workspace."""
    import ctypes
    red = ctypes.c_longlong(0)
    total = nat.load().posu_heatmap_mi_workspace(nseg, n, q, cm, ctypes.byref(red))
    if total < 0:
        raise ValueError('heatmap MI: unsupported shape S=%d N=%d Q=%d c_m=%d' % (nseg, n, q, cm))
    return int(total), int(red.value)


def _mi_param_table(p, training):
    import ctypes
    tab = (ctypes.c_void_p * len(_MI_PARAMS))()
    for k, name in enumerate(_MI_PARAMS):
        t = p[name]
        if t is None:
            if not (training and name in ('rm1', 'rv1', 'rm2', 'rv2')):
                raise ValueError('heatmap MI: parameter %s is missing' % name)
            tab[k] = None
        else:
            tab[k] = t.data_ptr()
    return tab


def _mi_geometry(feat, hm, idx, p):
    b, h, w, c = feat.shape
    q = idx.shape[1]
    cm = p['W1'].shape[0]
    if hm.shape[0] != b or tuple(hm.shape[2:]) != (h, w) or idx.shape[0] != b:
        raise ValueError('heatmap MI: features %s, heatmaps %s and indices %s disagree'
                         % (tuple(feat.shape), tuple(hm.shape), tuple(idx.shape)))
    if p['W1'].shape[1] != c + 1:
        raise ValueError('heatmap MI: the discriminator takes %d inputs, the features have %d channels (+ 1)'
                         % (p['W1'].shape[1], c))
    return b, h, w, c, hm.shape[1], q, cm


def _host_ptr(a):
    return None if a is None else a.ctypes.data


class _HeatmapPairScores(torch.autograd.Function):
    """u[n, i, j] of the discriminator over (feature row idx[n, i], heatmap value idx[n, j]).
    feat: [B, H, W, C] contiguous (f32 / bf16 / f16); hm: [B, J, H, W] f32; idx: [B, Q] int32 on the
    device, idx_host its host copy (checked by the library) or None (indices made on the device: the range
    is then the caller's contract and the kernels clamp).  Returns (u, stats)."""

    @staticmethod
    def forward(ctx, feat, hm, idx, idx_host, joint_idx, nseg, training, eps, *params):
        p = dict(zip(_MI_PARAMS, params))
        b, h, w, c, j, q, cm = _mi_geometry(feat, hm, idx, p)
        n = b // nseg
        ws_bytes, _ = heatmap_mi_workspace(nseg, n, q, cm)
        ws = torch.empty(ws_bytes, dtype=torch.uint8, device=feat.device)
        k2 = cm // 4
        stats = torch.empty((nseg, 3, cm + k2), dtype=torch.float32, device=feat.device)
        u = torch.empty((b, q, q), dtype=torch.float32, device=feat.device)
        tab = _mi_param_table(p, training)
        call('posu_heatmap_pair_scores_fwd', nat.dtype_code_of(feat), ptr(feat), ptr(hm), nseg, n, h, w, c, j,
             int(joint_idx), ptr(idx), _host_ptr(idx_host), q, cm, tab, int(training), float(eps), ptr(stats), ptr(u),
             ptr(ws), ws_bytes, stream_of(feat.device))
        # training mode normalises with batch statistics: the running buffers (updated in place by
        # the module after this call) are not part of the backward
        saved = [None if (training and name in ('rm1', 'rv1', 'rm2', 'rv2')) else p[name] for name in _MI_PARAMS]
        ctx.save_for_backward(feat, hm, idx, *[t for t in saved if t is not None])
        ctx.saved_names = [name for name, t in zip(_MI_PARAMS, saved) if t is not None]
        ctx.idx_host, ctx.joint_idx, ctx.nseg, ctx.training, ctx.eps = idx_host, int(joint_idx), nseg, training, eps
        ctx.mark_non_differentiable(stats)
        return u, stats

    @staticmethod
    def backward(ctx, du, _dstats):
        feat, hm, idx = ctx.saved_tensors[:3]
        p = dict.fromkeys(_MI_PARAMS)
        p.update(zip(ctx.saved_names, ctx.saved_tensors[3:]))
        b, h, w, c, j, q, cm = _mi_geometry(feat, hm, idx, p)
        nseg, n, k2 = ctx.nseg, b // ctx.nseg, cm // 4
        need = ctx.needs_input_grad
        want_feat, want_hm = need[0], need[1]
        grad_pos = {name: 8 + _MI_PARAMS.index(name) for name in _MI_GRADS}
        want_params = any(need[k] for k in grad_pos.values())
        out = [None] * (8 + len(_MI_PARAMS))
        if not (want_feat or want_hm or want_params):
            return tuple(out)
        dev = feat.device
        ws_bytes, _ = heatmap_mi_workspace(nseg, n, q, cm)
        ws = torch.empty(ws_bytes, dtype=torch.uint8, device=dev)
        stats = torch.empty((nseg, 3, cm + k2), dtype=torch.float32, device=dev)
        dparams = torch.empty(nat.load().posu_heatmap_dparams_floats(c, cm), dtype=torch.float32,
                              device=dev) if want_params else None
        dfeat = torch.empty_like(feat) if want_feat else None
        dhm = torch.empty_like(hm) if want_hm else None
        du = du.contiguous().float()
        tab = _mi_param_table(p, ctx.training)
        call('posu_heatmap_pair_scores_bwd', nat.dtype_code_of(feat), ptr(feat), ptr(hm), nseg, n, h, w, c, j,
             ctx.joint_idx, ptr(idx), _host_ptr(ctx.idx_host), q, cm, tab, int(ctx.training), float(ctx.eps),
             ptr(stats), ptr(du), ptr(dparams), ptr(dfeat), ptr(dhm), ptr(ws), ws_bytes, stream_of(dev))
        out[0], out[1] = dfeat, dhm
        if want_params:
            sizes = {'W1': cm * (c + 1), 'g1': cm, 'be1': cm, 'W2': k2 * cm, 'b2': k2, 'g2': k2, 'be2': k2, 'w3': k2,
                     'b3': 1}
            off = 0
            for name in _MI_GRADS:
                if need[grad_pos[name]]:
                    out[grad_pos[name]] = dparams[off:off + sizes[name]].view(p[name].shape)
                off += sizes[name]
        return tuple(out)


def heatmap_pair_scores(low_features, heatmaps, indices, joint_idx, params, nseg=1, training=True, eps=1e-5):
    """Scores u [B, Q, Q] of the heatmap discriminator over every (feature row, heatmap value) pair
    of each image (reference core/loss.py:674-717 + models/discriminator.py:225-242), and the batch
    statistics [nseg, 3, c_m + c_m // 4] (mean, biased, unbiased variance) of the two BatchNorms.

    low_features [B, C, H, W] (f32 / bf16 / f16): a tensor whose channel stride is 1 (the backbone's
    x1.permute(0, 3, 1, 2)) is read in place, anything else is made channels-last once.
    heatmaps [B, J, H, W]; indices [B, Q] integer; B = nseg * N, statistics per segment.  Host indices are
    range-checked by the library; an int32 / int64 cuda tensor is used in place (converted to int32 on the
    device if need be) with no copy to the host: its range is the caller's contract, the kernels clamp.
    params: dict of W1, g1, be1, rm1, rv1, W2, b2, g2, be2, rm2, rv2, w3, b3 (f32)."""
    require_cuda(low_features, heatmaps, *[t for t in params.values() if t is not None])
    if low_features.dtype not in (torch.float32, torch.bfloat16, torch.float16):
        low_features = low_features.float()
    feat = low_features.permute(0, 2, 3, 1)
    if not feat.is_contiguous():
        feat = feat.contiguous()
    if feat.shape[0] % nseg:
        raise ValueError('heatmap MI: %d images do not split into %d segments' % (feat.shape[0], nseg))
    hm = heatmaps.contiguous().float()
    if isinstance(indices, torch.Tensor) and indices.is_cuda and indices.dtype in (torch.int32, torch.int64):
        # made on the device (heatmap_mi_sample): used in place, never copied to the host to be checked
        idx_host = None
        idx = indices.detach().to(device=feat.device, dtype=torch.int32).contiguous()
    else:
        idx_host = np.ascontiguousarray(indices.detach().cpu().numpy().astype(np.int32))
        idx = torch.from_numpy(idx_host).to(feat.device)
    plist = []
    for name in _MI_PARAMS:
        t = params[name]
        plist.append(None if t is None else t.contiguous().float())
    return _HeatmapPairScores.apply(feat, hm, idx, idx_host, joint_idx, nseg, bool(training), eps, *plist)


def heatmap_mi_sample(joints, vis, joint_idx, feat, map_hw, radius, seed, call):
    """The positions HeatmapMILoss scores, drawn on the device (posu_heatmap_mi_sample; include/posu.h
    defines the stream): (idx [B, Q] int32, loc [B] int32, the window centres), Q = P // 2 + P // 4 for
    P = (2 radius + 1)^2.  Row k depends on (seed, call, k) and on its own inputs only.

    joints [B, J, 2] crop px and vis [B, J] or [B, J, k] (column 0 is used): host or device tensors of any
    float dtype, brought to f64 on the device (an upload, never a read).  feat: crop px per map px (w, h);
    map_hw: (H, W).  `call` is passed by value, so a captured graph would replay one draw."""
    joints, vis = torch.as_tensor(joints), torch.as_tensor(vis)
    dev = joints.device if joints.is_cuda else (vis.device if vis.is_cuda else None)
    if dev is None:
        if not torch.cuda.is_available():
            require_cuda(joints, vis)
        dev = torch.device('cuda', torch.cuda.current_device())
    if vis.dim() == 3:
        vis = vis[:, :, 0]
    if joints.dim() != 3 or joints.shape[2] != 2 or tuple(vis.shape) != tuple(joints.shape[:2]):
        raise ValueError('heatmap_mi_sample: joints [B, J, 2] and vis [B, J] or [B, J, k] expected, got %s and %s'
                         % (tuple(joints.shape), tuple(vis.shape)))
    joints = joints.detach().to(device=dev, dtype=torch.float64).contiguous()
    vis = vis.detach().to(device=dev, dtype=torch.float64).contiguous()
    b, j = vis.shape
    p = (2 * int(radius) + 1) ** 2
    idx = torch.empty((b, p // 2 + p // 4), dtype=torch.int32, device=dev)
    loc = torch.empty((b,), dtype=torch.int32, device=dev)
    if b:   # (`call` the argument shadows the binding's call here)
        nat.call('posu_heatmap_mi_sample', ptr(joints), ptr(vis), b, j, int(joint_idx), float(feat[0]),
                 float(feat[1]), int(map_hw[0]), int(map_hw[1]), int(radius), int(seed), int(call), ptr(idx),
                 ptr(loc), stream_of(dev))
    return idx, loc


class _PairMILoss(torch.autograd.Function):
    @staticmethod
    def forward(ctx, u, measure, nseg):
        b, q, _ = u.shape
        ws_bytes = nat.load().posu_pair_mi_workspace(nseg)
        ws = torch.empty(ws_bytes, dtype=torch.uint8, device=u.device)
        loss = torch.empty((nseg,), dtype=torch.float32, device=u.device)
        call('posu_pair_mi_loss_fwd', ptr(u), nseg, b // nseg, q, measure, ptr(loss), ptr(ws), ws_bytes,
             stream_of(u.device))
        ctx.save_for_backward(u)
        ctx.measure, ctx.nseg = measure, nseg
        return loss

    @staticmethod
    def backward(ctx, gloss):
        u, = ctx.saved_tensors
        b, q, _ = u.shape
        gloss = gloss.contiguous().float()
        du = torch.empty_like(u)
        call('posu_pair_mi_loss_bwd', ptr(u), ctx.nseg, b // ctx.nseg, q, ctx.measure, ptr(gloss), ptr(du),
             stream_of(u.device))
        return du, None, None


def pair_mi_loss(u, measure, nseg=1):
    """The mutual-information measure ('JSD' or 'NCE', reference core/loss.py:719-757) on pair scores
    u [nseg * N, Q, Q]: one loss per segment, [nseg]."""
    require_cuda(u)
    if measure not in MI_MEASURES:
        raise NotImplementedError('heatmap MI measure %r (JSD and NCE are built)' % (measure,))
    if u.dim() != 3 or u.shape[1] != u.shape[2] or u.shape[0] % nseg:
        raise ValueError('pair_mi_loss: u must be [nseg * N, Q, Q], got %s' % (tuple(u.shape),))
    return _PairMILoss.apply(u.contiguous().float(), MI_MEASURES[measure], nseg)


# ------------------------------------------------------------ training-loop metrics
def _view_pointers(tensors):
    import ctypes
    return (ctypes.c_void_p * len(tensors))(*[None if t is None else t.data_ptr() for t in tensors])


def _same_maps(views, what):
    views = [v.detach() for v in views]
    require_cuda(*views)
    shape = tuple(views[0].shape)
    for v in views:
        if v.dtype != torch.float32 or tuple(v.shape) != shape:
            raise ValueError('%s: float32 tensors of one shape expected, got %s %s' % (what, v.dtype, tuple(v.shape)))
    return [v.contiguous() for v in views]


def pck_accuracy(outputs, targets, thr=0.5):
    """PCK accuracy of V views (posu_pck_accuracy): lists of [N, J, H, W] f32 cuda heatmaps ->
    (acc [V, J + 1] f64, avg [V] f64, cnt [V] int32, pred [V, N, J, 2] f32, step [2] f64 = the means
    over the views of avg and cnt), all on the device; nothing is read back."""
    import ctypes
    if not outputs or len(outputs) != len(targets):
        raise ValueError('pck_accuracy: one target per output view expected')
    outs, tgts = _same_maps(outputs, 'pck_accuracy'), _same_maps(targets, 'pck_accuracy')
    if outs[0].dim() != 4 or tgts[0].shape != outs[0].shape:
        raise ValueError('pck_accuracy: [N, J, H, W] outputs and targets of one shape expected')
    v = len(outs)
    n, j, h, w = outs[0].shape
    dev = outs[0].device
    ws_bytes = nat.load().posu_pck_accuracy_workspace(v, n, j)
    if ws_bytes < 0:
        raise ValueError('pck_accuracy: unsupported shape V=%d N=%d J=%d (1 to 8 views)' % (v, n, j))
    ws = torch.empty(ws_bytes, dtype=torch.uint8, device=dev)
    acc = torch.empty((v, j + 1), dtype=torch.float64, device=dev)
    avg = torch.empty((v,), dtype=torch.float64, device=dev)
    cnt = torch.empty((v,), dtype=torch.int32, device=dev)
    pred = torch.empty((v, n, j, 2), dtype=torch.float32, device=dev)
    step = torch.empty((2,), dtype=torch.float64, device=dev)
    po, pt = _view_pointers(outs), _view_pointers(tgts)
    call('posu_pck_accuracy', ctypes.cast(po, ctypes.c_void_p), ctypes.cast(pt, ctypes.c_void_p), v, n, j, h, w,
         float(thr), ptr(acc), ptr(avg), ptr(cnt), ptr(pred), ptr(step), ptr(ws), ws_bytes, stream_of(dev))
    return acc, avg, cnt, pred, step


def grad_row_norms(grads, p=1):
    """sum over the views of (sum of the rows' p-norms / rows with a norm != 0) in f64
    (posu_grad_row_norms): grads a list of [N, ...] f32 cuda tensors of one shape, None = a view
    without a gradient (skipped; at least one must be there).  -> 0-dim f64 cuda tensor."""
    import ctypes
    have = [g for g in grads if g is not None]
    if not have:
        raise ValueError('grad_row_norms: no view has a gradient')
    if p not in (1, 2):
        raise ValueError('grad_row_norms: norm order 1 or 2, got %r' % (p,))
    have = _same_maps(have, 'grad_row_norms')
    it = iter(have)
    rows = [None if g is None else next(it) for g in grads]
    n = have[0].shape[0]
    length = have[0][0].numel()
    dev = have[0].device
    ws_bytes = nat.load().posu_grad_row_norms_workspace(len(rows), n)
    if ws_bytes < 0:
        raise ValueError('grad_row_norms: unsupported shape V=%d N=%d (1 to 8 views)' % (len(rows), n))
    ws = torch.empty(ws_bytes // 8, dtype=torch.float64, device=dev)
    out = torch.empty((), dtype=torch.float64, device=dev)
    tab = _view_pointers(rows)
    call('posu_grad_row_norms', ctypes.cast(tab, ctypes.c_void_p), len(rows), n, length, int(p), ptr(out), ptr(ws),
         ws_bytes, stream_of(dev))
    return out


def meters_update(table, values, weights, active):
    """AverageMeter.update of every active slot in one launch (posu_meters_update): table [M, 3] f64
    (val, sum, count) updated in place; values, weights [M] f64 cuda; active: M host booleans."""
    require_cuda(table, values, weights)
    m = table.shape[0]
    for t, shape in ((table, (m, 3)), (values, (m,)), (weights, (m,))):
        if t.dtype != torch.float64 or tuple(t.shape) != shape or not t.is_contiguous():
            raise ValueError('meters_update: contiguous float64 table [M, 3], values [M] and weights [M] expected')
    mask = np.ascontiguousarray(np.asarray(active, dtype=np.uint8))
    if mask.shape != (m,):
        raise ValueError('meters_update: one active flag per meter expected')
    call('posu_meters_update', ptr(table), m, ptr(values), ptr(weights), mask.ctypes.data, stream_of(table.device))
    return table


# ------------------------------------------------------ 3-D evaluation protocol
_REFLECTION = {'best': 0, True: 1, False: 2}   # posu_procrustes' reflection codes (include/posu.h)


def _f64(t):
    return t.detach().to(torch.float64).contiguous()


def procrustes(A, B, scaling=True, reflection='best'):
    """PoseUtils.procrustes for a batch (posu_procrustes): A (target), B [N, J, 3] cuda, any float dtype
    -> (d [N], Z [N, J, 3], R [N, 3, 3], scale [N], t [N, 3]) f64 on the device, Z = scale * B R + t."""
    require_cuda(A, B)
    if A.dim() != 3 or A.shape[2] != 3 or A.shape != B.shape or A.shape[0] < 1 or A.shape[1] < 1:
        raise ValueError('procrustes: two [N, J, 3] tensors of one shape expected, got %s and %s'
                         % (tuple(A.shape), tuple(B.shape)))
    if isinstance(reflection, str) and reflection != 'best' or reflection not in _REFLECTION:
        raise ValueError("procrustes: reflection must be 'best', True or False, got %r" % (reflection,))
    A, B = _f64(A), _f64(B)
    n, j, _ = A.shape
    dev = A.device
    d = torch.empty((n,), dtype=torch.float64, device=dev)
    Z = torch.empty((n, j, 3), dtype=torch.float64, device=dev)
    R = torch.empty((n, 3, 3), dtype=torch.float64, device=dev)
    scale = torch.empty((n,), dtype=torch.float64, device=dev)
    t = torch.empty((n, 3), dtype=torch.float64, device=dev)
    call('posu_procrustes', ptr(A), ptr(B), n, j, int(bool(scaling)), _REFLECTION[reflection], ptr(d), ptr(Z), ptr(R),
         ptr(scale), ptr(t), stream_of(dev))
    return d, Z, R, scale, t


def pose3d_errors(X, gt, R, T, procrustes=False, return_aligned=False):
    """error_computing_3d for a batch (posu_pose3d_errors): X [G, J, 3] world frame, gt [G, V, J, 3] camera
    frames, R [G, V, 3, 3], T [G, V, 3] (or [G, V, 3, 1]) cuda -> err [G, V, J] f64 (with return_aligned
    also pred [G, V, J, 3], Procrustes-aligned onto gt when procrustes is set)."""
    require_cuda(X, gt, R, T)
    if gt.dim() != 4 or gt.shape[3] != 3 or gt.shape[0] < 1 or gt.shape[1] < 1 or gt.shape[2] < 1:
        raise ValueError('pose3d_errors: gt must be [G, V, J, 3], got %s' % (tuple(gt.shape),))
    g, v, j, _ = gt.shape
    if tuple(X.shape) != (g, j, 3) or tuple(R.shape) != (g, v, 3, 3) or T.numel() != g * v * 3:
        raise ValueError('pose3d_errors: X [G, J, 3], R [G, V, 3, 3], T [G, V, 3] expected for gt %s; got %s, %s, %s'
                         % (tuple(gt.shape), tuple(X.shape), tuple(R.shape), tuple(T.shape)))
    X, gt, R, T = _f64(X), _f64(gt), _f64(R), _f64(T.reshape(g, v, 3))
    dev = gt.device
    err = torch.empty((g, v, j), dtype=torch.float64, device=dev)
    aligned = torch.empty((g, v, j, 3), dtype=torch.float64, device=dev) if return_aligned else None
    call('posu_pose3d_errors', ptr(X), ptr(gt), ptr(R), ptr(T), g, v, j, int(bool(procrustes)), ptr(err), ptr(aligned),
         stream_of(dev))
    return (err, aligned) if return_aligned else err


def limb_break(X, parent, limb, thres=0.4, return_worst=False):
    """break_limb_length for a batch (posu_limb_break): X [G, J, 3], parent [J] (-1 at the root), limb [G, J]
    or one shared [J] by child joint, all cuda -> flag [G] uint8 (with return_worst also the largest
    offset / limb [G] f64)."""
    require_cuda(X, parent, limb)
    if X.dim() != 3 or X.shape[2] != 3 or X.shape[0] < 1 or X.shape[1] < 1:
        raise ValueError('limb_break: X must be [G, J, 3], got %s' % (tuple(X.shape),))
    g, j, _ = X.shape
    if tuple(parent.shape) != (j,) or tuple(limb.shape) not in ((j,), (g, j)):
        raise ValueError('limb_break: parent [J] and limb [J] or [G, J] expected for X %s; got %s, %s'
                         % (tuple(X.shape), tuple(parent.shape), tuple(limb.shape)))
    X, limb = _f64(X), _f64(limb)
    parent = parent.to(torch.int32).contiguous()
    dev = X.device
    flag = torch.empty((g,), dtype=torch.uint8, device=dev)
    worst = torch.empty((g,), dtype=torch.float64, device=dev) if return_worst else None
    call('posu_limb_break', ptr(X), ptr(parent), ptr(limb), j if limb.dim() == 2 else 0, g, j, float(thres), ptr(flag),
         ptr(worst), stream_of(dev))
    return (flag, worst) if return_worst else flag


# ----------------------------------------------------------- pseudo-label round
def pseudo_label_workspace(t, g, v, j):
    """Bytes of one round's device results (posu_pseudo_label_workspace: projections, counts, masks); raises
    outside 1 <= T <= 8, 2 <= V <= 4, J > 0, G >= 0."""
    n = nat.load().posu_pseudo_label_workspace(int(t), int(g), int(v), int(j))
    if n < 0:
        raise ValueError('pseudo_label_workspace: 1 <= T <= 8, 2 <= V <= 4, J > 0, G >= 0 expected, got T=%d G=%d '
                         'V=%d J=%d' % (t, g, v, j))
    return n


def pseudo_label_sweep(M, intr, xy, conf, thresholds, reproj_thre=20.0, min_inliers=2, use_ransac=True,
                       undistort=True, vis_out=None, proj_out=None):
    """The threshold / RANSAC / reprojection stages of test_pseudo_label.py's loop for every threshold in one
    launch (posu_pseudo_label_sweep): M [G, V, 3, 4] f64, intr [G, V, 9] f64, xy [G, V, J, 2], conf [G, V, J] f32,
    all cuda; thresholds: up to 8 numbers, compared in f32 -> (masks [T, 3, G, V, J] uint8 of the stages
    threshold / RANSAC / reprojection, proj [T, G, V, J, 2] f64)."""
    require_cuda(M, intr, xy, conf, vis_out, proj_out)
    if xy.dim() != 4 or xy.shape[3] != 2:
        raise ValueError('pseudo_label_sweep: xy must be [G, V, J, 2], got %s' % (tuple(xy.shape),))
    g, v, j, _ = xy.shape
    if tuple(conf.shape) != (g, v, j) or M.numel() != g * v * 12 or intr.numel() != g * v * 9:
        raise ValueError('pseudo_label_sweep: conf [G, V, J], M [G, V, 3, 4], intr [G, V, 9] expected for xy %s; '
                         'got %s, %s, %s' % (tuple(xy.shape), tuple(conf.shape), tuple(M.shape), tuple(intr.shape)))
    if conf.dtype != torch.float32:
        raise TypeError('pseudo_label_sweep: conf must be float32 (the thresholds are compared in f32), got %s'
                        % conf.dtype)
    thre = np.ascontiguousarray(thresholds, dtype=np.float32).reshape(-1)
    t = int(thre.size)
    dev = xy.device
    xy, conf = _f64(xy), conf.detach().contiguous()
    if vis_out is None:
        vis_out = torch.empty((t, 3, g, v, j), dtype=torch.uint8, device=dev)
    if proj_out is None:
        proj_out = torch.empty((t, g, v, j, 2), dtype=torch.float64, device=dev)
    if (vis_out.dtype, proj_out.dtype) != (torch.uint8, torch.float64) or vis_out.numel() != t * 3 * g * v * j \
            or proj_out.numel() != t * g * v * j * 2 or not (vis_out.is_contiguous() and proj_out.is_contiguous()):
        raise ValueError('pseudo_label_sweep: vis_out [T, 3, G, V, J] uint8 and proj_out [T, G, V, J, 2] f64, '
                         'contiguous, expected')
    nat.call('posu_pseudo_label_sweep', ptr(_f64(M)), ptr(_f64(intr)), ptr(xy), ptr(conf), _host(thre), t, g, v, j,
         int(bool(undistort)), float(reproj_thre), int(min_inliers), int(bool(use_ransac)), ptr(vis_out),
         ptr(proj_out), stream_of(dev))
    return vis_out.view(t, 3, g, v, j), proj_out.view(t, g, v, j, 2)


def pckh_counts(pred, vis, gt, head, nviews=1, threshold=0.5, pred_sets=None, set_pred=None, out=None):
    """Integer counts behind my_eval and the Joints@k lines for B label sets (posu_pckh_counts): vis [B, N, J]
    (non-zero = visible), pred [N, J, 2] shared by the sets, gt [N, J, 2] or None, head [N] (or [N, 1]), all
    cuda; pred_sets [S, N, J, 2] with set_pred (B ints: -1 = pred, s = pred_sets[s]) gives sets predictions of
    their own -> counts [B, 2J + nviews + 1] int32: detected-and-visible per joint, visible per joint, and the
    histogram of visible views per (group, joint) for N = G * nviews group-major frames."""
    require_cuda(pred, vis, gt, head, pred_sets, out)
    if vis.dim() != 3:
        raise ValueError('pckh_counts: vis must be [B, N, J], got %s' % (tuple(vis.shape),))
    b, n, j = vis.shape
    if gt is not None and (pred is None or head is None or tuple(gt.shape) != (n, j, 2) or head.numel() != n):
        raise ValueError('pckh_counts: gt [N, J, 2] needs pred and head [N]')
    if pred is not None and tuple(pred.shape) != (n, j, 2):
        raise ValueError('pckh_counts: pred must be [N, J, 2] for vis %s, got %s' % (tuple(vis.shape), tuple(pred.shape)))
    sel = None
    if set_pred is not None:
        sel = np.ascontiguousarray(set_pred, dtype=np.int32).reshape(-1)
        nsets = 0 if pred_sets is None else pred_sets.numel() // max(n * j * 2, 1)
        if sel.size != b or (sel >= nsets).any():
            raise ValueError('pckh_counts: set_pred needs B entries below the number of pred_sets')
        if pred_sets is not None and (pred_sets.dtype != torch.float64 or not pred_sets.is_contiguous()):
            raise ValueError('pckh_counts: pred_sets must be contiguous float64')
    dev = vis.device
    vis = vis.detach()
    if vis.dtype != torch.uint8:
        vis = vis.ne(0).to(torch.uint8)
    vis = vis.contiguous()
    w = 2 * j + int(nviews) + 1
    if out is None:
        out = torch.empty((b, w), dtype=torch.int32, device=dev)
    elif out.dtype != torch.int32 or out.numel() != b * w or not out.is_contiguous():
        raise ValueError('pckh_counts: out must be contiguous int32 [B, 2J + nviews + 1]')
    nat.call('posu_pckh_counts', ptr(None if pred is None else _f64(pred)), ptr(pred_sets),
         None if sel is None else _host(sel), ptr(vis), ptr(None if gt is None else _f64(gt)),
         ptr(None if head is None else _f64(head.reshape(-1))), b, n, j, int(nviews), float(threshold), ptr(out),
         stream_of(dev))
    return out.view(b, w)


# ------------------------------------------------------------ validation epoch
def decode_views(outputs, flipped=None, perm=None, shift=False, targets=None, affine64=None, post_process=True,
                 thr=0.5, preds_out=None, merged_out=None, row0=0):
    """The validation batch body after the forwards for all V views in one launch (posu_decode_views): the
    flip-test merge 0.5 * (o + flip_back(flipped)) (``perm``: [J] ints, ``shift``: SHIFT_HEATMAP),
    get_final_preds (``affine64`` [V * N, 2, 3] f64 view-major, ``post_process``) and, with ``targets``, the
    PCK accuracy of the merged maps.  outputs / flipped / targets: lists of V [N, J, H, W] f32 cuda tensors.

    ``preds_out`` [R, J, 3] f32 (x, y, maxval; allocated at R = V * N when None) and ``merged_out`` [R, J, H, W]
    f32 (None: the merged maps are not stored) are written at rows row0 + n * V + v, the reference's
    preds[k::nviews] order; the other rows are left alone.  Returns (preds_out, merged_out, acc [V, J + 1] f64,
    avg [V] f64, cnt [V] int32, step [2] f64 = the views' mean avg and cnt), the last four None without
    targets; everything stays on the device and nothing is read back."""
    import ctypes
    if not outputs:
        raise ValueError('decode_views: at least one view expected')
    outs = _same_maps(outputs, 'decode_views')
    if outs[0].dim() != 4:
        raise ValueError('decode_views: [N, J, H, W] outputs expected, got %s' % (tuple(outs[0].shape),))
    v = len(outs)
    n, j, h, w = outs[0].shape
    dev = outs[0].device
    flips = tgts = None
    for name, views in (('flipped', flipped), ('targets', targets)):
        if views is None:
            continue
        views = _same_maps(views, 'decode_views')
        if len(views) != v or views[0].shape != outs[0].shape:
            raise ValueError('decode_views: one %s tensor of the outputs\' shape per view expected' % name)
        if name == 'flipped':
            flips = views
        else:
            tgts = views
    if perm is not None:
        if flips is None:
            raise ValueError('decode_views: perm goes with flipped')
        if not isinstance(perm, torch.Tensor):
            host = [int(p) for p in perm]
            if len(host) != j or min(host) < 0 or max(host) >= j:
                raise ValueError('decode_views: perm must hold J joint indices')
            perm = torch.tensor(host, dtype=torch.int32)
        if perm.numel() != j:
            raise ValueError('decode_views: perm must hold J joint indices')
        perm = perm.to(device=dev, dtype=torch.int32).contiguous()
    require_cuda(affine64, preds_out, merged_out)
    if affine64 is not None:
        if affine64.numel() != v * n * 6:
            raise ValueError('decode_views: affine64 must be [V * N, 2, 3], got %s' % (tuple(affine64.shape),))
        affine64 = affine64.to(device=dev, dtype=torch.float64).contiguous()
    row0 = int(row0)
    if preds_out is None:
        if row0 != 0:
            raise ValueError('decode_views: row0 needs preds_out')
        preds_out = torch.empty((v * n, j, 3), dtype=torch.float32, device=dev)
    rows = preds_out.shape[0]
    if preds_out.dtype != torch.float32 or tuple(preds_out.shape[1:]) != (j, 3) or not preds_out.is_contiguous():
        raise ValueError('decode_views: preds_out must be contiguous float32 [R, J, 3]')
    if merged_out is not None:
        if merged_out.dtype != torch.float32 or tuple(merged_out.shape[1:]) != (j, h, w) \
                or not merged_out.is_contiguous():
            raise ValueError('decode_views: merged_out must be contiguous float32 [R, J, H, W]')
        rows = min(rows, merged_out.shape[0])
    ws_bytes = nat.load().posu_decode_views_workspace(v, n, j)
    if ws_bytes < 0:
        raise ValueError('decode_views: unsupported shape V=%d N=%d J=%d (1 to 8 views)' % (v, n, j))
    acc = avg = cnt = step = ws = None
    if tgts is not None:
        ws = torch.empty(max(ws_bytes, 4), dtype=torch.uint8, device=dev)
        acc = torch.empty((v, j + 1), dtype=torch.float64, device=dev)
        avg = torch.empty((v,), dtype=torch.float64, device=dev)
        cnt = torch.empty((v,), dtype=torch.int32, device=dev)
        step = torch.empty((2,), dtype=torch.float64, device=dev)
    tables = [None if t is None else _view_pointers(t) for t in (outs, flips, tgts)]
    po, pf, pt = [None if t is None else ctypes.cast(t, ctypes.c_void_p) for t in tables]
    call('posu_decode_views', po, pf, ptr(perm), int(bool(shift)), pt, ptr(affine64), v, n, j, h, w,
         int(bool(post_process)), float(thr), ptr(merged_out), ptr(preds_out), row0, rows, ptr(acc), ptr(avg),
         ptr(cnt), ptr(step), ptr(ws), ws_bytes, stream_of(dev))
    return preds_out, merged_out, acc, avg, cnt, step


def detection_counts(pred, gt, head, thresholds, form=0, vis=None, out=None):
    """Per threshold and joint, the rows whose prediction lies within that threshold's head-size distance of the
    ground truth (posu_detection_counts): pred [N, J, 2] or [N, J, 3] f32 (x, y), gt [N, J, 2], head [N] (or
    [N, 1]), vis [N, J] (non-zero = counted) or None, all cuda; thresholds: 1 to 8 numbers; form 0: d <= head * thr
    (the H36M evaluation), form 1: d / head <= thr (the MPII one), in f64 -> counts [T, 2, J] int32 on the device:
    detected-and-visible and visible."""
    require_cuda(pred, gt, head, vis, out)
    if pred.dim() != 3 or pred.shape[2] not in (2, 3):
        raise ValueError('detection_counts: pred must be [N, J, 2] or [N, J, 3], got %s' % (tuple(pred.shape),))
    n, j, c = pred.shape
    if tuple(gt.shape) != (n, j, 2) or head.numel() != n:
        raise ValueError('detection_counts: gt [N, J, 2] and head [N] expected for pred %s, got %s and %s'
                         % (tuple(pred.shape), tuple(gt.shape), tuple(head.shape)))
    if form not in (0, 1):
        raise ValueError('detection_counts: form 0 (d <= head * thr) or 1 (d / head <= thr), got %r' % (form,))
    thre = np.ascontiguousarray(thresholds, dtype=np.float64).reshape(-1)
    t = int(thre.size)
    dev = pred.device
    pred = pred.detach().to(torch.float32).contiguous()
    if vis is not None:
        if tuple(vis.shape) != (n, j):
            raise ValueError('detection_counts: vis must be [N, J], got %s' % (tuple(vis.shape),))
        vis = vis.detach()
        if vis.dtype != torch.uint8:
            vis = vis.ne(0).to(torch.uint8)
        vis = vis.contiguous()
    if out is None:
        out = torch.empty((max(t, 1), 2, j), dtype=torch.int32, device=dev)
    elif out.dtype != torch.int32 or out.numel() != t * 2 * j or not out.is_contiguous():
        raise ValueError('detection_counts: out must be contiguous int32 [T, 2, J]')
    nat.call('posu_detection_counts', ptr(pred), c, ptr(_f64(gt)), ptr(_f64(head.reshape(-1))), ptr(vis), _host(thre),
             t, int(form), n, j, ptr(out), stream_of(dev))
    return out.view(t, 2, j)


def _valid_u8(valid, shape, what):
    if valid is None:
        return None
    if tuple(valid.shape) != tuple(shape):
        raise ValueError('%s: valid must be %s, got %s' % (what, list(shape), tuple(valid.shape)))
    valid = valid.detach()
    if valid.dtype != torch.uint8:
        valid = valid.ne(0).to(torch.uint8)
    return valid.contiguous()


def fundamental_workspace(p, n, h):
    """Bytes of posu_fundamental_lmeds' device workspace; raises ValueError for shapes it refuses."""
    nbytes = nat.load().posu_fundamental_workspace(int(p), int(n), int(h))
    if nbytes < 0:
        raise ValueError('fundamental_workspace: 1 <= P <= 65535, 8 <= N <= 2^26, 1 <= H <= 2^20 expected, got P=%d '
                         'N=%d H=%d' % (p, n, h))
    return nbytes


def fundamental_lmeds(pts, valid=None, hypotheses=512, seed=0, refit=True):
    """Least-median-of-squares fundamental matrices of P problems in one call (posu_fundamental_lmeds;
    include/posu.h defines the estimator): pts [P, N, 4] (x_i, y_i, x_j, y_j) px, valid [P, N] or None, cuda ->
    (F [P, 3, 3] f64, mask [P, N] uint8, sample [P, 8] int32, stats [P, 4] f64: median, sigma, n_inliers, the
    winning hypothesis), all on the device."""
    require_cuda(pts, valid)
    if pts.dim() != 3 or pts.shape[2] != 4:
        raise ValueError('fundamental_lmeds: pts must be [P, N, 4], got %s' % (tuple(pts.shape),))
    p, n, _ = pts.shape
    nbytes = fundamental_workspace(p, n, hypotheses)
    dev = pts.device
    pts = _f64(pts)
    valid = _valid_u8(valid, (p, n), 'fundamental_lmeds')
    ws = torch.empty((nbytes // 8,), dtype=torch.float64, device=dev)
    F = torch.empty((p, 3, 3), dtype=torch.float64, device=dev)
    mask = torch.empty((p, n), dtype=torch.uint8, device=dev)
    sample = torch.empty((p, 8), dtype=torch.int32, device=dev)
    stats = torch.empty((p, 4), dtype=torch.float64, device=dev)
    nat.call('posu_fundamental_lmeds', ptr(pts), ptr(valid), p, n, int(hypotheses), int(seed) & (2 ** 64 - 1),
             int(bool(refit)), ptr(F), ptr(mask), ptr(sample), ptr(stats), ptr(ws), nbytes, stream_of(dev))
    return F, mask, sample, stats


def epipolar_residual_stats(F, pts, valid=None):
    """Per problem the mean and the max over the valid rows of |x_j^T F x_i| (posu_epipolar_residual_stats):
    F [P, 3, 3], pts [P, N, 4], valid [P, N] or None, cuda -> [P, 2] f64 on the device."""
    require_cuda(F, pts, valid)
    if pts.dim() != 3 or pts.shape[2] != 4 or tuple(F.shape) != (pts.shape[0], 3, 3):
        raise ValueError('epipolar_residual_stats: F [P, 3, 3] and pts [P, N, 4] expected, got %s and %s'
                         % (tuple(F.shape), tuple(pts.shape)))
    p, n, _ = pts.shape
    valid = _valid_u8(valid, (p, n), 'epipolar_residual_stats')
    out = torch.empty((p, 2), dtype=torch.float64, device=pts.device)
    nat.call('posu_epipolar_residual_stats', ptr(_f64(F)), ptr(_f64(pts)), ptr(valid), p, n, ptr(out),
             stream_of(pts.device))
    return out
