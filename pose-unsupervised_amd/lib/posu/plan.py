"""Inference plan for PoseResNet on the HIP kernels.

A plan is the packed, device-resident form of a PoseResNet (NHWC weights, folded BN)
plus the ordered list of kernel launches of one forward pass
(lib/models/pose_resnet.py:191-205 of the reference):

    pack(NCHW f32 -> NHWC, C 3 -> 8)
    stem conv 7x7/s2 + BN + ReLU          -> maxpool 3x3/s2
    layer1..4: per block conv/BN/ReLU chain, residual (+ downsample conv/BN) fused
               into the last conv's epilogue
    3 x (deconv 4x4/s2 + BN + ReLU)       (sub-pixel, one launch each)
    final 1x1 conv + bias                 -> NCHW f32 heatmaps

All launches go to PyTorch's current stream, so a forward can be captured in a
torch.cuda.CUDAGraph (hipGraph) by the caller.
"""
from collections import namedtuple

import torch

from . import ops
from .packing import (fold_bn, pack_bottleneck_conv1_weight, pack_bottleneck_conv3_weight, pack_bottleneck_down_weight,
                      pack_conv_weight, pack_deconv4x4_weight, pack_down_tail_stream,
                      pack_dual_1x1_weight, pack_s2_tail_stream, pack_stem_fused_weight, pack_stem_s2d_weight,
                      pack_tail_stream, split_exponent, to_split)

STEM_CIN_PAD = 8      # direct 7x7 stem (odd input sizes)
STEM_S2D_PAD = 16     # space-to-depth stem: 4 sub-pixels x 3 channels, padded
SPLIT_PAD = 32        # the split dtype's channel granule (the stem pads to it)


def _stem_pads(code):
    """(direct-stem Cin pad, space-to-depth pad) in logical channels (distinct: run_stem tells the
    two packed inputs apart by their channel count; the split dtype's direct stem, for odd input
    sizes only, pads to 2 granules)."""
    return (2 * SPLIT_PAD, SPLIT_PAD) if code == ops.F16X3 else (STEM_CIN_PAD, STEM_S2D_PAD)


def _pack(pk32, code):
    """An f32 / f64 pack in the logical K order -> (pack in the compute dtype, power-of-two weight
    exponent e the epilogue scale must undo: 2^-e; 0 except for the split dtype)."""
    if code == ops.F16X3:
        e = split_exponent(pk32)
        return to_split(pk32, e), e
    return pk32.to(ops.torch_dtype(code)).contiguous(), 0


def _unscale(scale, e):
    return scale if e == 0 else (scale.double() * 2.0 ** -e).float().contiguous()

# fused pack + stem + max-pool kernel (posu_stem_pool_fwd) for bf16 / fp16 plans
FUSED_STEM = True
# bf16 / fp16 plans: the fused deconv+head sums the head in split precision (the deconv output and
# the head weights as hi + lo pairs of the dtype): the rounding of the deconv output to the dtype
# was the largest single term of the 2-byte chains' joint error (tools/precision_attribution.py)
PRECISE_HEAD = True
# the fused stem over all views of a forward in one launch (posu_stem_pool_views_fwd); False: one
# launch per view
STEM_VIEWS = True


class RawViews:
    """pack_input's result when the fused stem applies: the caller's NCHW f32 views
    (stacked on N in order), consumed directly by posu_stem_pool_fwd.  .packed() gives the
    space-to-depth pack of the two-launch path (chunked runs, tools)."""

    def __init__(self, plan, views, hflip):
        self.plan, self.views, self.hflip = plan, views, hflip
        _, _, self.h, self.w = views[0].shape
        self.shape = (sum(v.shape[0] for v in views), self.h, self.w, 3)
        self.device = views[0].device

    def packed(self):
        return self.plan.pack_input(self.views, hflip=self.hflip, fused=False)

    def __getitem__(self, sl):
        """Batch slice (chunked runs): the views' rows [start, stop) of the stacked batch."""
        if not isinstance(sl, slice) or sl.step not in (None, 1):
            raise TypeError('RawViews supports contiguous batch slices only')
        start, stop, _ = sl.indices(self.shape[0])
        out, base = [], 0
        for v in self.views:
            a, b = max(start - base, 0), min(stop - base, v.shape[0])
            if a < b:
                out.append(v[a:b])
            base += v.shape[0]
        return RawViews(self.plan, out, self.hflip)

# the 128x128 eight-wave staggered conv tiles (7 / 15, round 4) among the autotuner's candidates
TILES_128X8 = True
# the 128x128 tile with two K groups of four waves (39, round 5; inference plans only: its K order
# differs from the other tiles', and the training plan relies on every candidate summing alike).
# bf16 / fp16 plans: on again at the end of round 6 -- with this round's plan the headline and configs[1]
# measured 1 % faster with it (2.237 / 2.250 vs 2.267 / 2.270 ms; 1.331 / 1.327 vs 1.345 / 1.342 ms,
# profiles/r06/ksplit_bf16_ab_r6ah.txt; round 5's plan showed no gain), and the line's `control` leg times
# the plan without it.  Where the tuner picks it, the 2-byte plans' last bits depend on the tuned table
# (reproducible under a fixed --tune-file).  The split dtype never gets tile 39: every candidate tile of
# the parity mode sums alike, so its results do not depend on the tuning (and the A/B was at noise level:
# 5.689 / 5.603 vs 5.675 / 5.704 ms, profiles/r06/ksplit_bf16_ab_r6ah.txt)
TILES_KSPLIT = True
# the split dtype's staggered eight-wave tiles (31, 47 / 55; round 6) among its autotuner candidates
TILES_SPLIT_SG = True

# ---- per-layer tile autotuning: geometry key -> conv tile configuration (process-wide,
# shared by every plan, so a re-packed plan does not re-tune)
_TUNE_CACHE = {}
_TUNE_TIMES = {}   # geometry key -> {tile: best ms of the reps}, the last tuning's measurements
_REFINE_TIMES = {}  # geometry key -> {tile: ms per whole forward}, the in-context stage's measurements
# the in-context second tuning stage (PoseResNetPlan._refine_in_context)
REFINE_IN_CONTEXT = True


class _Tuner:
    active = False
    reps = 3
    seen = []   # geometry keys met by the current tuning run, in launch order
    probe = None      # in-context stage: the geometry whose launches are bracketed by HIP events
    probe_events = []


def _tile_candidates(cout, code=None, ksplit=False):
    """Tile ids (include/posu.h): cfg 0..6, cfg + 8 = single-slot ring (four-wave tiles;
    short-K layers: more blocks per CU), cfg + 16 = three-slot ring (two K-tiles in flight),
    cfg + 32 = persistent K-tile stream (epilogue stores overlap the next tile's fetch),
    23 / 31 = 256x256 / 256x128 with waves 4-7 staggered by half a K-tile, 7 / 15 = 128x128 with
    eight waves (staggered in bf16 / f16, unstaggered in split fp16, whose staggered twins are
    47 / 55), 39 = 128x128 with two K groups.  The library's table (kTiles, csrc/conv_igemm.hip)
    says what every id runs per dtype; an id it has no kernel for in a dtype (the + 32 bit and
    7 / 15 / 23 / 31 / 39 in f32) runs the id without the bit or the heuristic's tile, which the
    f32 lists below rely on."""
    cpad = (cout + 63) // 64 * 64
    c = [0, 1, 2]
    if cpad % 128 == 0:
        c += [3, 4, 6]
    if cpad % 256 == 0:
        c.append(5)
    # + 32: the persistent K-tile stream (2-byte dtypes; others ignore the bit);
    # 23 / 31: the eight-wave tiles with waves 4-7 staggered by half a K-tile; 7 / 15: 128x128 with
    # eight staggered waves (2x4 / 4x2 wave grids)
    sg = [23 + 8 * (t == 6) for t in c if t in (5, 6)] + ([7, 15] if cpad % 128 == 0 and TILES_128X8 else [])
    rings = c + [t + 8 for t in c if t <= 4] + [t + 16 for t in c if t != 5]
    if code == ops.F16X3:   # the split dtype: plain rings (no persistent stream), the unstaggered (7 / 15)
        # and (round 6) staggered (47 / 55) eight-wave 128x128 tiles and the staggered 256x128 tile (31); never
        # the two-K-group tile (39, TILES_KSPLIT above)
        return rings + ([7, 15] + ([47, 55, 31] if TILES_SPLIT_SG else []) if cpad % 128 == 0 else [])
    if ksplit and code in (ops.BF16, ops.F16) and cpad % 128 == 0:
        sg = sg + [39]
    # (tile 32, the persistent 256x64 four-wave instance, is left out: it spills 928 B per lane to
    # scratch and took ~1.2 ms per launch in the tuning trials, 10x the other tiles)
    return rings + [t + 32 for t in c if t != 0] + sg


def _tuned(key, cout, launch):
    """launch(tile) -> output.  While tuning, time every admissible tile once on the real
    operands (HIP events) and keep the fastest for this geometry."""
    cands = _tile_candidates(cout, key[1], ksplit=TILES_KSPLIT and key[0] in ('conv', 'dual', 'deconv'))
    if _Tuner.active and key not in _Tuner.seen:
        _Tuner.seen.append(key)
    # (re)tune a geometry not in the table, or whose tuned tile is no longer a candidate (a plan
    # switch such as TILES_128X8 turned off for a control run)
    if _Tuner.active and (key not in _TUNE_CACHE or _TUNE_CACHE[key] not in cands):
        # two passes over the candidates, the second in reverse order, each tile's best of the two:
        # one pass let the clock ramp and the neighbours' cache state pick tiles that run 20-25 %
        # slower in the graph (layer4 3x3: 75 vs 60 us, profiles/r04/replay_breakdown_r4l.txt)
        times = {}
        for order in (cands, cands[::-1]):
            for t in order:
                launch(t)
                a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                a.record()
                for _ in range(_Tuner.reps):
                    launch(t)
                b.record()
                b.synchronize()
                ms = a.elapsed_time(b)
                times[t] = min(ms, times.get(t, ms))
        _TUNE_CACHE[key] = min(cands, key=lambda t: (times[t], cands.index(t)))
        _TUNE_TIMES[key] = times
    t = _TUNE_CACHE.get(key, -1)
    if _Tuner.probe is not None and key == _Tuner.probe:
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        out = launch(t if t in cands else -1)
        b.record()
        _Tuner.probe_events.append((a, b))
        return out
    return launch(t if t in cands else -1)


def tuned_tiles():
    """The autotuned table (geometry key -> tile), e.g. for logging."""
    return dict(_TUNE_CACHE)


def tuning_times():
    """The last tuning's per-tile times (geometry key -> {tile: ms for the reps}), for diagnostics."""
    return {k: dict(v) for k, v in _TUNE_TIMES.items()}


def refine_times():
    """The in-context stage's times (geometry key -> {tile: median ms of its launches inside a forward})."""
    return {k: dict(v) for k, v in _REFINE_TIMES.items()}


class _Conv:
    __slots__ = ('w', 'scale', 'shift', 'cout', 'k', 'stride', 'pad', 'relu')

    def __init__(self, conv, bn, relu, code, bk, cin_pad=None):
        cin = conv.weight.shape[1]
        # (the split dtype packs 32 logical k per K-tile)
        self.w, e = _pack(pack_conv_weight(conv.weight, cin_pad or cin, 32 if code == ops.F16X3 else bk,
                                           torch.float32), code)
        self.scale, self.shift = fold_bn(bn, conv.bias)
        self.scale = _unscale(self.scale, e)
        self.cout = conv.weight.shape[0]
        self.k = conv.kernel_size[0]
        if conv.kernel_size[0] != conv.kernel_size[1]:
            raise NotImplementedError('square kernels only')
        self.stride = conv.stride[0]
        self.pad = conv.padding[0]
        self.relu = relu

    def __call__(self, x, code, residual=None, out=None):
        if out is None:
            ho = (x.shape[1] + 2 * self.pad - self.k) // self.stride + 1
            wo = (x.shape[2] + 2 * self.pad - self.k) // self.stride + 1
            out = torch.empty((x.shape[0], ho, wo, self.cout * ops.cmul(code)), dtype=x.dtype, device=x.device)
        key = ('conv', code, tuple(x.shape), self.cout, self.k, self.stride, self.pad, residual is not None)
        return _tuned(key, self.cout, lambda t: ops.conv2d_nhwc(
            x, self.w, self.cout, self.k, self.k, self.stride, self.pad, self.scale, self.shift, residual, self.relu,
            code, out=out, tile=t))


class _DualTail:
    """Bottleneck conv3/bn3 + downsample conv/bn as one two-source 1x1 GEMM."""
    __slots__ = ('w', 'scale', 'shift', 'cout', 'stride2')

    def __init__(self, conv3, bn3, dconv, dbn, code):
        s3, b3 = fold_bn(bn3, conv3.bias)
        sd, bd = fold_bn(dbn, dconv.bias)
        self.w, e = _pack(pack_dual_1x1_weight(conv3.weight, s3, dconv.weight, sd, torch.float64), code)
        self.shift = (b3.double() + bd.double()).float().contiguous()
        self.cout = conv3.weight.shape[0]
        self.scale = None if e == 0 else torch.full((self.cout,), 2.0 ** -e, device=self.shift.device)
        self.stride2 = dconv.stride[0]

    def __call__(self, mid, x, code, out=None):
        if out is None:
            out = torch.empty(tuple(mid.shape[:3]) + (self.cout * ops.cmul(code),), dtype=mid.dtype, device=mid.device)
        key = ('dual', code, tuple(mid.shape), tuple(x.shape), self.cout)
        return _tuned(key, self.cout, lambda t: ops.conv1x1_dual_nhwc(
            mid, x, self.stride2, self.w, self.cout, self.shift, True, code, out=out, tile=t, scale=self.scale))


# Bottlenecks of layer1 (planes 64, 64x64 maps) as ONE fused launch each in bf16 / fp16 plans
# (posu_bottleneck_fwd; the first block, with its downsample, posu_bottleneck_down_fwd), and the
# identity Bottlenecks of layer2 / layer3 as conv1 (a conv launch) + the register-streamed
# conv2 + conv3 + residual tail (posu_bottleneck_tail_stream_fwd); False runs the convolutions.
# (The round-2 LDS-ring layer2 block / layer3 tail kernels, slower than the streamed tail, were
# removed from the library in round 4.)
FUSED_BOTTLENECK = True
# layer2's first Bottleneck: conv2 (3x3 / stride 2) and the conv3 | downsample dual GEMM as ONE
# launch (posu_bottleneck_s2_tail_fwd) after the conv1 launch; False: two launches
S2_TAIL = True
# consecutive streamed identity tails chained: block i's tail also computes block i+1's conv1
# over its output (posu_bottleneck_tail_stream_next_fwd), so block i+1 has no conv1 launch and y
# is not re-read for it (tools/chain_micro.py: layer2 105.0 vs 130.0 us, layer3 76.3 vs 85.0 us
# for a tail + the next conv1 launch; bit-identical)
CHAINED_TAILS = True
# layer2's strided tail chained with block 1's conv1 (posu_bottleneck_s2_tail_next_fwd, round 4;
# under CHAINED_TAILS too)
S2_CHAIN = True
# layer2's first Bottleneck as ONE launch: its conv1 folded into the strided tail, which computes
# relu(bn1(conv1(x))) on each tile's window instead of reading t1 (posu_bottleneck_s2_front_tail[_next]_fwd,
# bit-identical).  True: always; False: where the autotuner measured it faster (S2_FRONT_TUNE), else the
# conv1 launch, then the tail reading its output.  Off by default like every untuned choice: a plan that
# was never tuned launches what it always launched (tests/test_plan_trace.py pins that sequence)
S2_FRONT = False
# the autotuner times both forms of that block on its real operands and keeps the faster in the tile table
# (key ('s2_front', dtype, x shape, chained) -> 1 / 0, persisted with the tiles by bench.py --tune-file);
# False: never the one-launch form unless S2_FRONT forces it (bench.py --plan-flag S2_FRONT_TUNE=0 is the
# A/B handle; the headline measured 2.255 vs 2.308 ms with the one-launch form, profiles/r10)
S2_FRONT_TUNE = True
# the identity Bottlenecks at 384x384 (R152, BASELINE configs[4]) as conv1 + the streamed tail
# (round 5): layer3 at W = 24 (not chained), layer2 at W = 48 (chained).  Chaining layer3's W = 24 tails
# like the 256x256 ones (2-row tiles, three m-tiles per wave, round 6) measured even with each conv1 a
# launch of its own after the plain 6-row tail (configs[4] 9.82 / 10.01 vs 9.97 / 9.97 k frames/s,
# profiles/r06/w24_chain_ab_r6l.txt) -- the 2-row tiles' weight stream (a third of the MFMAs per fragment)
# costs what the conv1 launches cost -- so the plan has no such variant
TAIL_W24 = True
# the split dtype's identity Bottlenecks of layer1 / layer2 / layer3 as conv1 + the streamed tail
# (chained), layer1's first block as conv1 + the down tail (chained), round 6; False: the conv launches
SPLIT_TAILS = True
# layer1 at 384x384 (96-wide maps, R152 configs[4]) in bf16 / fp16 plans on the streamed tails (round 6):
# the first block as conv1 + the down tail, the identity blocks as the (chained) tail; False: three
# conv launches per block (the fused layer1 kernel is built for 64-wide maps)
TAIL_W96 = True
# split fp16: the last identity block of layers 1-3 chains the NEXT layer's first conv1 too (C -> 2 P,
# posu_bottleneck_tail_stream_chain_fwd, round 6), so that block's conv1 is no launch of its own
CHAIN_LAYERS = True
# the same layer chain in bf16 / fp16 plans (layers 2-3, NX = 2 tails): bit-identical, but measured
# 0.6 % slower on the headline (call r6m: 2.279 vs 2.264 ms; the 2-row NX = 2 tiles halve the layer's
# last tail's rows per workgroup, which costs what the saved conv1 launch gains), so off
CHAIN_LAYERS_2B = False
# round 6: the split dtype's forward runs stem..layer2 and deconv2..head depth-first over two halves
# of the batch by default (run(chunks=None)): its activations are twice the 2-byte ones, so a half
# batch's layer1 / layer2 tensors stay in the 256 MiB Infinity Cache between launches; the layers stay
# chained (layer1 -> layer2 inside a half, layer2 -> layer3 through a whole-batch buffer) -- 5.47-5.64
# vs 5.60-5.75 ms per forward at 32 x 4 (profiles/r06/chunks_ab_r6vwx.txt; 4 chunks slower: the halved
# grids cost more).  The bf16 headline measured slower chunked (2.376 / 2.378 vs 2.325 / 2.346 ms) and
# keeps 1.  Both ends are sliced, the late stage like the early one: a late stage in quarters or eighths
# measured no better than in halves (5.619 / 5.784, 5.727 / 5.714 vs 5.639 / 5.661 ms, same file).
CHUNKS_F16X3 = 2
EARLY_LAYERS = 2     # layers in the chunked early stage (1 .. 3): stem..layer2 (1: stem..layer1)
_FUSED_MAX_BYTES = (1 << 31) - 256   # the fused kernels address x / y with 32-bit byte offsets


def _fused_fits(x, cout):
    """Input and output of a fused Bottleneck kernel inside its 32-bit addressing range (larger
    batches run the convolutions, which use 64-bit addressing)."""
    px = x.shape[0] * x.shape[1] * x.shape[2]
    es = x.element_size()
    return px * max(x.shape[3], cout) * es < _FUSED_MAX_BYTES


_2B = (ops.BF16, ops.F16)
_SPLIT = (ops.F16X3,)
# Where a fused kernel runs: the dtypes, the map width, the multiple its rows must be of (its row tile), the
# chained entry points it has there ('next': + the next block's conv1, 'layer': + the next layer's first
# conv1), and its switches -- built: read when a plan is constructed (off: the packs are not made), live:
# read at every call.
_At = namedtuple('_At', 'codes width rows chains built live', defaults=((), None, None))
# What a fused kernel is built for: the (Cout, K) pack shapes of conv1, conv2 and conv3, or of the
# conv3 | downsample dual pack, in logical k (a pack row holds cmul(code) stored halves per k), conv2's
# stride, and where it runs.
_Kernel = namedtuple('_Kernel', 'conv1 conv2 conv3 dual stride at')
_GEOMETRY = {
    # layer1 at 64-wide maps, one launch per block: the identity blocks, the first block with its downsample
    'fused': _Kernel((64, 256), (64, 576), (256, 64), None, 1, (_At(_2B, 64, 1),)),
    'fused_down': _Kernel((64, 64), (64, 576), None, (256, 128), 1, (_At(_2B, 64, 1),)),
    # conv1 (a conv launch), then conv2 + the dual GEMM in one: layer1's first block (2-row tiles) and
    # layer2's, strided
    'down_tail': _Kernel((64, 64), (64, 576), None, (256, 128), 1,
                         (_At(_SPLIT, 64, 2, ('next',), 'SPLIT_TAILS', 'SPLIT_TAILS'),
                          _At(_2B, 96, 2, ('next',), 'TAIL_W96', 'TAIL_W96'))),
    's2_tail': _Kernel((128, 256), (128, 1152), None, (512, 384), 2, (_At(_2B, 64, 8, ('next',), live='S2_TAIL'),)),
    # conv1, then the register-streamed conv2 + conv3 + residual tail: the identity blocks of layers 1-3
    # (the split dtype at 256x256 only; 2-byte layer1 at 64-wide maps runs 'fused'; W = 48 / 24: R152 at
    # 384x384, BASELINE configs[4])
    'l1': _Kernel((64, 256), (64, 576), (256, 64), None, 1,
                  (_At(_SPLIT, 64, 2, ('next', 'layer'), 'SPLIT_TAILS'), _At(_2B, 96, 2, ('next',), 'TAIL_W96'))),
    'l2': _Kernel((128, 512), (128, 1152), (512, 128), None, 1,
                  (_At(_2B, 32, 4, ('next', 'layer')), _At(_SPLIT, 32, 4, ('next', 'layer'), 'SPLIT_TAILS'),
                   _At(_2B, 48, 2, ('next',), live='TAIL_W24'))),
    'l3': _Kernel((256, 1024), (256, 2304), (1024, 256), None, 1,
                  (_At(_2B, 16, 8, ('next', 'layer')), _At(_SPLIT, 16, 8, ('next', 'layer'), 'SPLIT_TAILS'),
                   _At(_2B, 24, 6, (), live='TAIL_W24'))),
}


def _on(switch):
    return switch is None or bool(globals()[switch])


class _Block:
    """One residual block: its packs and the launches it makes.  select() names the variant
    that runs on an input, run() executes it:

        'fused' / 'fused_down'   posu_bottleneck_fwd / posu_bottleneck_down_fwd
        'down_tail'              conv1, posu_bottleneck_down_tail_stream_fwd (chained: with s1n / b1n)
        's2_tail'                conv1, posu_bottleneck_s2_tail_fwd (chained: .._s2_tail_next_fwd); S2_FRONT, or
                                 tuned so (S2_FRONT_TUNE): posu_bottleneck_s2_front_tail_fwd (.._next_fwd)
                                 alone, conv1 inside it
        'tail'                   conv1 (unless handed in), posu_bottleneck_tail_stream_fwd (chained 'next':
                                 .._stream_next_fwd, 'layer': .._stream_chain_fwd)
        'dual'                   conv1 (unless handed in), conv2, the conv3 | downsample dual GEMM
        'convs'                  the plain conv launches, the residual in the last one's epilogue
    """
    __slots__ = ('convs', 'down', 'dual', 'code', 'kind', 'packs', 'chain', 'xchain', 'dscale')

    def __init__(self, blk, code, bk):
        names = ['conv1', 'conv2', 'conv3'] if hasattr(blk, 'conv3') else ['conv1', 'conv2']
        self.convs = []
        self.down = None
        self.dual = None
        self.code = code
        self.kind = None     # 'l1' / 'l2' / 'l3': the identity block of that layer the streamed tail is built for
        # the fused kernels' packs by variant: 'fused' (conv1, conv3 with permuted K), 'fused_down' ([w3*s3 |
        # wd*sd], permuted conv3 K), 'tail' / 'down_tail' / 's2_tail' (the per-wave weight streams),
        # '.._next' / 'tail_layer' (the streams with the chained conv1 appended) and 's2_front' / 's2_front_next'
        # (the strided tail's streams with the block's own conv1 in front, S2_FRONT)
        self.packs = {}
        self.chain = None    # the next block's conv1 (_Conv) where this block's tail can chain it
        self.xchain = None   # the next layer's first conv1 (_Conv), chained by this layer's last tail
        self.dscale = None   # the down tail's dual-GEMM epilogue scale (2^-e; ones in 2-byte plans)
        ds = blk.downsample
        if ds is not None and len(names) == 3 and ds[0].kernel_size == (1, 1) and \
                blk.conv3.weight.shape[1] % bk == 0 and ds[0].weight.shape[1] % bk == 0:
            for nm in names[:2]:
                self.convs.append(_Conv(getattr(blk, nm), getattr(blk, 'bn' + nm[-1]), True, code, bk))
            self.dual = _DualTail(blk.conv3, blk.bn3, ds[0], ds[1], code)
            c2 = self.convs[1]
            if self._built_for('fused_down'):
                self.packs['fused_down'] = pack_bottleneck_down_weight(self.dual.w, 64)
            if self._built_for('down_tail'):
                self.packs['down_tail'] = pack_down_tail_stream(c2.w, self.dual.w)
                self.dscale = (self.dual.scale if self.dual.scale is not None else
                               torch.ones(self.dual.cout, device=self.dual.shift.device))
            if self._built_for('s2_tail'):
                self.packs['s2_tail'] = pack_s2_tail_stream(c2.w, self.dual.w)
                self.packs['s2_front'] = pack_s2_tail_stream(c2.w, self.dual.w, w1=self.convs[0].w)
            return
        for nm in names:
            self.convs.append(_Conv(getattr(blk, nm), getattr(blk, 'bn' + nm[-1]), True, code, bk))
        if ds is not None:
            self.down = _Conv(ds[0], ds[1], False, code, bk)
        if self._built_for('fused'):
            self.packs['fused'] = (pack_bottleneck_conv1_weight(blk.conv1.weight, ops.torch_dtype(code)),
                                   pack_bottleneck_conv3_weight(blk.conv3.weight, ops.torch_dtype(code)))
        self.kind = next((k for k in ('l1', 'l2', 'l3') if self._built_for(k)), None)
        if self.kind is not None:
            self.packs['tail'] = pack_tail_stream(self.convs[1].w, self.convs[2].w)

    def _built_for(self, kernel):
        """This block's convolutions are the ones `kernel` is built for (_GEOMETRY), in a dtype it has,
        that row's construction switch on."""
        g = _GEOMETRY[kernel]
        if self.down is not None or (self.dual is None) != (g.dual is None) or len(self.convs) != (2 if g.dual else 3):
            return False
        c1, c2 = self.convs[:2]
        last, shape = (self.dual, g.dual) if g.dual else (self.convs[2], g.conv3)
        cm = ops.cmul(self.code)
        return (c1.k == 1 and c1.stride == 1 and c2.k == 3 and c2.stride == g.stride and c2.pad == 1 and
                (last.stride2 == g.stride if g.dual else last.k == 1 and last.stride == 1) and
                all(c.cout == co and tuple(c.w.shape) == (co, k * cm)
                    for c, (co, k) in ((c1, g.conv1), (c2, g.conv2), (last, shape))) and
                any(self.code in a.codes and _on(a.built) for a in g.at))

    def _chains(self, how):
        """The streamed tail of this block's kind has the `how`-chained entry point in this dtype."""
        return self.kind is not None and any(self.code in a.codes and how in a.chains
                                             for a in _GEOMETRY[self.kind].at)

    def link_next(self, nxt):
        """Chain this block's tail with the next block's conv1: identity tails of one kind, the down tail
        and layer1's block 1, the strided tail and layer2's block 1."""
        c2 = self.convs[1]
        if self.kind is not None and self.kind == nxt.kind:
            self.chain = nxt.convs[0]
            self.packs['tail_next'] = pack_tail_stream(c2.w, self.convs[2].w, self.chain.w)
        elif 'down_tail' in self.packs and nxt.kind == 'l1':
            self.chain = nxt.convs[0]
            self.packs['down_tail_next'] = pack_down_tail_stream(c2.w, self.dual.w, self.chain.w)
        elif 's2_tail' in self.packs and nxt.kind == 'l2':
            self.chain = nxt.convs[0]
            self.packs['s2_tail_next'] = pack_s2_tail_stream(c2.w, self.dual.w, self.chain.w)
            self.packs['s2_front_next'] = pack_s2_tail_stream(c2.w, self.dual.w, self.chain.w, w1=self.convs[0].w)

    def link_layer(self, first):
        """Chain this last identity block's tail with the next layer's first block's conv1 (1x1 / stride 1,
        C -> 2 P: posu_bottleneck_tail_stream_chain_fwd): split fp16 layers 1-3, bf16 / fp16 layers 2-3
        (CHAIN_LAYERS_2B)."""
        if not (self._chains('layer') and (self.code in _SPLIT or CHAIN_LAYERS_2B) and first.dual is not None):
            return
        c1n = first.convs[0]
        planes = self.convs[1].cout
        if c1n.k == 1 and c1n.stride == 1 and c1n.cout == 2 * planes and tuple(c1n.w.shape)[1] == self.convs[0].w.shape[1]:
            self.xchain = c1n
            self.packs['tail_layer'] = pack_tail_stream(self.convs[1].w, self.convs[2].w, c1n.w)

    @property
    def cout(self):
        return self.dual.cout if self.dual is not None else self.convs[-1].cout

    def _at(self, kernel, x):
        """The _GEOMETRY row under which this block runs `kernel` on x [N, H, W, C], or None: the block has
        the kernel's packs, the fused kernels are on (FUSED_BOTTLENECK) and address x and y, and a row of
        this dtype, its per-call switch on, has x's width and divides its rows."""
        g = _GEOMETRY[kernel]
        if not (kernel == self.kind or kernel in self.packs) or not FUSED_BOTTLENECK or \
                x.shape[3] != g.conv1[1] * ops.cmul(self.code) or not _fused_fits(x, self.cout):
            return None
        return next((a for a in g.at if self.code in a.codes and x.shape[2] == a.width and
                     x.shape[1] % a.rows == 0 and _on(a.live)), None)

    def select(self, x, t1=False, chain_out=False, chain=True):
        """-> (variant, chained): the launches run() makes for the input x (only its shape and dtype are
        read; nothing is launched or allocated).  t1: this block's conv1 output is handed in (the previous
        tail chained it); chain_out: this is a layer's last block, asked for the next layer's first conv1;
        chain = False suppresses chaining.  chained: None, 'next' or 'layer' -- the extra output."""
        chain = chain and CHAINED_TAILS
        at = self._at(self.kind, x) if self.kind is not None else None
        if at is not None:
            if chain and chain_out and CHAIN_LAYERS and self.xchain is not None and 'layer' in at.chains:
                return 'tail', 'layer'
            return 'tail', ('next' if chain and self.chain is not None and 'next' in at.chains else None)
        if t1:
            if self.dual is None:
                raise RuntimeError('a chained conv1 output handed to a block without a streamed tail')
            return 'dual', None   # the first block of a layer whose conv1 the previous layer's last tail computed
        for variant in ('fused_down', 'down_tail', 's2_tail'):
            at = self._at(variant, x)
            if at is not None:
                nxt = (chain and variant + '_next' in self.packs and 'next' in at.chains and
                       (S2_CHAIN or variant != 's2_tail'))
                return variant, ('next' if nxt else None)
        if self.dual is not None:
            return 'dual', None
        return ('fused' if self._at('fused', x) is not None else 'convs'), None

    def run(self, x, code, out=None, t1=None, chain_out=False, t1n_out=None, chain=True):
        """-> (y, t1n): t1n = the conv1 output this block's tail computed for the next block (CHAINED_TAILS)
        or, chain_out, for the next layer's first block (CHAIN_LAYERS; into t1n_out), else None; t1 = this
        block's conv1 output from the previous block's chained tail (None: computed here)."""
        variant, chained = self.select(x, t1 is not None, chain_out, chain)
        cs = self.convs
        if variant == 'tail':
            c2, c3 = cs[1:]
            if t1 is None:
                t1 = cs[0](x, code)
            if chained == 'layer':
                n1 = self.xchain
                return ops.bottleneck_tail_stream_chain_nhwc(t1, x, self.packs['tail_layer'], c2.scale, c2.shift,
                                                             c3.scale, c3.shift, n1.scale, n1.shift, code, out=out,
                                                             t1n=t1n_out)
            if chained == 'next':
                n1 = self.chain
                return ops.bottleneck_tail_stream_next_nhwc(t1, x, self.packs['tail_next'], c2.scale, c2.shift,
                                                            c3.scale, c3.shift, n1.scale, n1.shift, code, out=out)
            return ops.bottleneck_tail_stream_nhwc(t1, x, self.packs['tail'], c2.scale, c2.shift, c3.scale, c3.shift,
                                                   code, out=out), None
        if variant == 'fused':
            c1, c2, c3 = cs
            w1f, w3f = self.packs['fused']
            return ops.bottleneck_nhwc(x, w1f, c1.scale, c1.shift, c2.w, c2.scale, c2.shift, w3f, c3.scale, c3.shift,
                                       code, out=out), None
        if variant == 'fused_down':
            c1, c2 = cs
            return ops.bottleneck_down_nhwc(x, c1.w, c1.scale, c1.shift, c2.w, c2.scale, c2.shift,
                                            self.packs['fused_down'], self.dual.shift, code, out=out), None
        if variant == 'down_tail':
            c1, c2 = cs
            s1n, b1n = (self.chain.scale, self.chain.shift) if chained else (None, None)
            return ops.bottleneck_down_tail_stream_nhwc(
                c1(x, code), x, self.packs['down_tail_next' if chained else 'down_tail'], c2.scale, c2.shift,
                self.dscale, self.dual.shift, code, s1n=s1n, b1n=b1n, out=out)
        if variant == 's2_tail':
            front = S2_FRONT or (S2_FRONT_TUNE and self._front_tuned(x, code, chained, out))
            return self._s2_tail(x, code, chained, out, front)
        if variant == 'dual':
            return self.dual(cs[1](cs[0](x, code) if t1 is None else t1, code), x, code, out=out), None
        res = self.down(x, code) if self.down is not None else x
        y = x
        for c in cs[:-1]:
            y = c(y, code)
        return cs[-1](y, code, residual=res, out=out), None

    def _s2_tail(self, x, code, chained, out, front):
        """The 's2_tail' variant's launches: front -- the block's conv1 inside the strided tail, one launch --
        or the conv1 launch and the tail reading its output.  Bit-identical (the same K order per accumulator)
        unless conv1's tuned tile is the two-K-group one."""
        c1, c2 = self.convs
        n1 = self.chain
        if front:
            if chained:
                return ops.bottleneck_s2_front_tail_next_nhwc(
                    x, c1.scale, c1.shift, self.packs['s2_front_next'], c2.scale, c2.shift, self.dual.shift,
                    n1.scale, n1.shift, code, out=out)
            return ops.bottleneck_s2_front_tail_nhwc(x, c1.scale, c1.shift, self.packs['s2_front'], c2.scale,
                                                     c2.shift, self.dual.shift, code, out=out), None
        if chained:
            return ops.bottleneck_s2_tail_next_nhwc(c1(x, code), x, self.packs['s2_tail_next'], c2.scale, c2.shift,
                                                    self.dual.shift, n1.scale, n1.shift, code, out=out)
        return ops.bottleneck_s2_tail_nhwc(c1(x, code), x, self.packs['s2_tail'], c2.scale, c2.shift,
                                           self.dual.shift, code, out=out), None

    def _front_tuned(self, x, code, chained, out):
        """The tuned choice between the two forms of _s2_tail for this input (S2_FRONT_TUNE): while the
        autotuner runs, both are timed on the real operands like the tiles of _tuned (two passes, the second
        in reverse order, each form's best) and the faster is kept in the tile table; otherwise the stored
        choice, or -- a plan that was never tuned -- the two launches."""
        key = ('s2_front', code, tuple(x.shape), bool(chained))
        if _Tuner.active and key not in _TUNE_CACHE:
            seen = list(_Tuner.seen)
            times = {}
            for order in ((0, 1), (1, 0)):
                for f in order:
                    self._s2_tail(x, code, chained, out, bool(f))   # (the first call tunes conv1's tile)
                    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    a.record()
                    for _ in range(_Tuner.reps):
                        self._s2_tail(x, code, chained, out, bool(f))
                    b.record()
                    b.synchronize()
                    ms = a.elapsed_time(b)
                    times[f] = min(ms, times.get(f, ms))
            _TUNE_CACHE[key] = int(times[1] < times[0])
            _TUNE_TIMES[key] = times
            if _TUNE_CACHE[key]:
                _Tuner.seen[:] = seen   # conv1 is no launch of this forward: nothing for the in-context stage
        return bool(_TUNE_CACHE.get(key, 0))

    def __call__(self, x, code, out=None):
        """The block alone, unchained: y."""
        return self.run(x, code, out=out, chain=False)[0]


class _Deconv:
    __slots__ = ('w', 'scale', 'shift', 'cout')

    def __init__(self, dc, bn, code, bk):
        if dc.stride != (2, 2) or dc.padding != (1, 1) or dc.output_padding != (0, 0):
            raise NotImplementedError('deconv supported for kernel 4, stride 2, padding 1')
        self.w, e = _pack(pack_deconv4x4_weight(dc.weight, 32 if code == ops.F16X3 else bk, torch.float32), code)
        self.scale, self.shift = fold_bn(bn, dc.bias)
        self.scale = _unscale(self.scale, e)
        self.cout = dc.weight.shape[1]

    def __call__(self, x, code, out=None):
        if out is None:
            out = torch.empty((x.shape[0], 2 * x.shape[1], 2 * x.shape[2], self.cout * ops.cmul(code)), dtype=x.dtype,
                              device=x.device)
        key = ('deconv', code, tuple(x.shape), self.cout)
        return _tuned(key, self.cout, lambda t: ops.deconv4x4s2_nhwc(
            x, self.w, self.cout, self.scale, self.shift, True, code, out=out, tile=t))


class PoseResNetPlan:
    """Packed weights + forward launch sequence of one PoseResNet in one compute dtype."""

    def __init__(self, net, code):
        self.code = code
        bk = ops.conv_bk(code)
        self.cin_pad, self.s2d_pad = _stem_pads(code)
        self.stem = _Conv(net.conv1, net.bn1, True, code, bk, cin_pad=self.cin_pad)
        # the same stem as a 4x4/s1 conv over the 2x2 space-to-depth input (even sizes); the same
        # weights, so the same split exponent (the stem's scale is shared)
        if code == ops.F16X3:
            self.stem_s2d_w = to_split(pack_stem_s2d_weight(net.conv1.weight, self.s2d_pad, 32, torch.float32),
                                       split_exponent(net.conv1.weight.float()))
        else:
            self.stem_s2d_w = pack_stem_s2d_weight(net.conv1.weight, self.s2d_pad, bk, ops.torch_dtype(code))
        self.layers = [[_Block(b, code, bk) for b in layer] for layer in
                       (net.layer1, net.layer2, net.layer3, net.layer4)]
        for layer in self.layers:
            for b0, b1 in zip(layer, layer[1:]):
                b0.link_next(b1)
        for la, lb in zip(self.layers, self.layers[1:]):
            la[-1].link_layer(lb[0])
        mods = list(net.deconv_layers)
        self.deconvs = []
        for i in range(0, len(mods), 3):
            self.deconvs.append(_Deconv(mods[i], mods[i + 1], code, bk))
        fl = net.final_layer
        if fl.kernel_size != (1, 1):
            raise NotImplementedError('final layer supported for FINAL_CONV_KERNEL = 1')
        # the fused head reads hi / lo weight halves in the logical channel order (the split dtype
        # too); a separate head launch of the split dtype reads a split pack (head_w_split)
        self.head_w = pack_conv_weight(fl.weight, fl.weight.shape[1], bk, ops.torch_dtype(code))
        self.head_w_lo = None   # the split-precision head's residual weights (2-byte dtypes)
        self.head_w_split = None
        if code in (ops.BF16, ops.F16, ops.F16X3):
            w32 = pack_conv_weight(fl.weight, fl.weight.shape[1], bk, torch.float32)
            self.head_w_lo = (w32 - self.head_w.float()).to(ops.torch_dtype(code)).contiguous()
        if code == ops.F16X3:
            self.head_w_split = to_split(pack_conv_weight(fl.weight, fl.weight.shape[1], 32, torch.float32))
        self.head_b = (fl.bias.detach().float().contiguous() if fl.bias is not None
                       else torch.zeros(fl.weight.shape[0], device=fl.weight.device))
        self.njoints = fl.weight.shape[0]
        last = self.deconvs[-1] if self.deconvs else None
        self.fuse_head = last is not None and last.cout == 256 and self.njoints <= 16
        self.stem_fused_w = None
        if (FUSED_STEM and code in (ops.BF16, ops.F16, ops.F16X3) and tuple(net.conv1.weight.shape) == (64, 3, 7, 7)
                and net.conv1.stride == (2, 2) and net.conv1.padding == (3, 3)):
            if code == ops.F16X3:   # hi plane, then lo plane (posu_stem_pool_fwd); the stem conv's exponent
                v = pack_stem_fused_weight(net.conv1.weight, torch.float64) * 2.0 ** split_exponent(net.conv1.weight)
                hi = v.to(torch.float16)
                self.stem_fused_w = torch.cat([hi, (v - hi.double()).to(torch.float16)], dim=0).contiguous()
            else:
                self.stem_fused_w = pack_stem_fused_weight(net.conv1.weight, ops.torch_dtype(code))

    def pack_input(self, views, hflip=False, fused=True):
        """List of NCHW f32 tensors (same shape) -> one NHWC batch (views stacked on N):
        space-to-depth [N, H/2, W/2, 16] for even H, W, else [N, H, W, 8]; hflip mirrors
        every image along W (flip test).  Where the fused stem applies (bf16 / fp16,
        H % 8 == 0, W in {256, 384}) the views are handed over as they are (RawViews)."""
        n, _, h, w = views[0].shape
        if fused and self.stem_fused_w is not None and h % 8 == 0 and w in ((256,) if self.code == ops.F16X3 else
                                                                             (256, 384)) and views[0].shape[1] == 3:
            return RawViews(self, list(views), hflip)
        s2d = h % 2 == 0 and w % 2 == 0
        cm = ops.cmul(self.code)
        shape = ((n * len(views), h // 2, w // 2, self.s2d_pad * cm) if s2d else
                 (n * len(views), h, w, self.cin_pad * cm))
        x = torch.empty(shape, dtype=ops.torch_dtype(self.code), device=views[0].device)
        for i, v in enumerate(views):
            if s2d:
                ops.pack_s2d_nchw(v, self.code, self.s2d_pad, out=x[i * n:(i + 1) * n], hflip=hflip)
            else:
                ops.pack_nchw_to_nhwc(v, self.code, self.cin_pad, out=x[i * n:(i + 1) * n], hflip=hflip)
        return x

    def stem_pool(self, x):
        """stem + max-pool: one fused launch over the views for RawViews, else two launches."""
        code = self.code
        if isinstance(x, RawViews):
            if STEM_VIEWS and len({tuple(v.shape) for v in x.views}) == 1 and len(x.views) <= 8:
                return ops.stem_pool_views(x.views, self.stem_fused_w, self.stem.scale, self.stem.shift, code,
                                           hflip=x.hflip)
            out = torch.empty((x.shape[0], x.h // 4, x.w // 4, self.stem.cout * ops.cmul(code)),
                              dtype=ops.torch_dtype(code), device=x.device)
            base = 0
            for v in x.views:
                ops.stem_pool(v, self.stem_fused_w, self.stem.scale, self.stem.shift, code,
                              out=out[base:base + v.shape[0]], hflip=x.hflip)
                base += v.shape[0]
            return out
        return ops.maxpool3x3s2_nhwc(self.run_stem(x), code)

    def run_stem(self, x):
        code = self.code
        if isinstance(x, RawViews):
            x = x.packed()
        if x.shape[3] == self.s2d_pad * ops.cmul(code):
            st = self.stem
            out = torch.empty(tuple(x.shape[:3]) + (st.cout * ops.cmul(code),), dtype=x.dtype, device=x.device)
            key = ('stem_s2d', code, tuple(x.shape), st.cout)
            return _tuned(key, st.cout, lambda t: ops.conv2d_nhwc(
                x, self.stem_s2d_w, st.cout, 4, 4, 1, 2, st.scale, st.shift, None, True, code,
                out=out, out_hw=(x.shape[1], x.shape[2]), tile=t))
        return self.stem(x, code)

    def _run_layers(self, x, lo, hi, t1=None, out=None, keep=None, t1_out=None):
        """Layers lo .. hi - 1 block by block -> (the last one's output, layer1's or None, t1).  A chained
        tail hands the next block its conv1 output (CHAINED_TAILS), a layer's last tail the next layer's
        first block (CHAIN_LAYERS): t1 is the first block's, from the walk before, and the returned t1 the
        one the walk's last tail put into t1_out (the slice of a whole-batch buffer the next walk takes; given
        only where that tail chains), else None.  out / keep: the slices the last layer's / layer1's output
        go to."""
        x1 = None
        for li in range(lo, hi):
            layer = self.layers[li]
            final = li == hi - 1
            for bi, blk in enumerate(layer):
                last = bi == len(layer) - 1
                dst = (out if final else keep if li == 0 else None) if last else None
                x, t1 = blk.run(x, self.code, out=dst, t1=t1, chain_out=last and (not final or t1_out is not None),
                                t1n_out=t1_out if last and final else None)
            if li == 0:
                x1 = x
        return x, x1, t1

    def _stage_early(self, x, out=None, keep=None, t1_out=None, nl=2):
        """stem -> maxpool -> layer1 [-> layer2] (nl layers; out: the last one's output slice, keep: layer1
        output slice to fill when nl = 2).  Returns whether the last tail filled t1_out."""
        return self._run_layers(self.stem_pool(x), 0, nl, out=out, keep=keep, t1_out=t1_out)[2] is not None

    def _last_deconv_head(self, x, keep_f, hm_out=None, f_out=None):
        """Last deconv (+BN+ReLU) and the 1x1 head, fused into one launch when possible."""
        code = self.code
        dc = self.deconvs[-1]
        if self.fuse_head:
            return ops.deconv4x4s2_head(x, dc.w, dc.cout, dc.scale, dc.shift, self.head_w, self.njoints, self.head_b,
                                        code, keep_f=keep_f, hm_out=hm_out, f_out=f_out,
                                        head_w_lo=self.head_w_lo if PRECISE_HEAD else None)
        f = dc(x, code, out=f_out)
        hw = self.head_w_split if code == ops.F16X3 else self.head_w
        return ops.head1x1_nchw(f, hw, self.njoints, self.head_b, code, out=hm_out), f

    def _stage_late(self, x, hm_out=None, f_out=None, keep_f=True):
        """deconv2 .. last deconv -> head."""
        code = self.code
        for dc in self.deconvs[1:-1]:
            x = dc(x, code)
        return self._last_deconv_head(x, keep_f, hm_out=hm_out, f_out=f_out)

    def default_chunks(self):
        """The depth-first slices run(chunks=None) takes: CHUNKS_F16X3 for the split dtype, else 1."""
        return CHUNKS_F16X3 if self.code == ops.F16X3 else 1

    def autotune(self, x, chunks=None, keep_features=True, reps=3):
        """Time every admissible tile configuration of every conv launch of this forward
        (on the packed input x) and keep the fastest per layer geometry; later runs (and
        hipGraph captures) use the tuned tiles."""
        _Tuner.active, _Tuner.reps, _Tuner.seen = True, reps, []
        try:
            with torch.no_grad():
                out = self.run(x, chunks=chunks, keep_features=keep_features)
        finally:
            _Tuner.active = False
        if REFINE_IN_CONTEXT:
            with torch.no_grad():
                self._refine_in_context(x, chunks, keep_features)
        return out

    def _refine_in_context(self, x, chunks, keep_features, within=0.25, top=3, forwards=6):
        """Second tuning stage: for every geometry of this forward whose best per-launch
        candidates lie within 25 % of each other, run the whole forward with each of its top
        three and keep the one whose launches of that geometry took least INSIDE the forward
        (HIP events around exactly those launches, median over two rounds of `forwards`
        forwards).  The per-launch trials run one launch back to back; inside the network a
        launch follows other kernels at sustained clocks, and the ranking can differ: layer4's
        3x3 took 53 us on two tiles in isolation and 62 vs 75 us on them in the graph
        (profiles/r04/replay_breakdown*.txt).  (Round 4 compared whole-forward times, whose
        run-to-run spread -- ~0.5 % of 2.5 ms -- is as large as the differences it had to
        resolve: deconv1 went to a tile 15 us slower in one tuning, profiles/r05.)  within / top: the
        candidate window; a wider one measured no gain (2.329 / 2.335 vs 2.325 / 2.317 ms, call r6ak)."""
        def forward_ms(key):
            self.run(x, chunks=chunks, keep_features=keep_features)
            torch.cuda.synchronize()
            _Tuner.probe, _Tuner.probe_events = key, []
            try:
                for _ in range(forwards):
                    self.run(x, chunks=chunks, keep_features=keep_features)
                torch.cuda.synchronize()
                ms = sorted(a.elapsed_time(b) for a, b in _Tuner.probe_events)
            finally:
                _Tuner.probe, _Tuner.probe_events = None, []
            return ms[len(ms) // 2] if ms else float('inf')
        for key in list(_Tuner.seen):
            times = _TUNE_TIMES.get(key)
            if not times or key not in _TUNE_CACHE:
                continue
            best = min(times.values())
            cands = sorted((t for t in times if times[t] <= best * (1 + within)), key=lambda t: times[t])[:top]
            if len(cands) < 2:
                continue
            res = {}
            for order in (cands, cands[::-1]):
                for t in order:
                    _TUNE_CACHE[key] = t
                    ms = forward_ms(key)
                    res[t] = min(ms, res.get(t, ms))
            _TUNE_CACHE[key] = min(cands, key=lambda t: (res[t], cands.index(t)))
            _REFINE_TIMES[key] = res

    def run(self, x, chunks=None, keep_features=True):
        """Packed input -> (heatmaps NCHW f32, layer1 out NHWC, deconv out NHWC).

        chunks > 1 runs the HBM-bound ends of the network (stem..layer2 and
        deconv2..head) depth-first over `chunks` slices of the batch, so their
        activations stay resident in the 256 MiB Infinity Cache between producer and
        consumer; layer3..deconv1 run on the whole batch (None: default_chunks()).
        keep_features=False skips materialising the full layer1 / deconv outputs
        (returned as None)."""
        code = self.code
        if chunks is None:
            chunks = self.default_chunks()
        n = x.shape[0]
        if chunks <= 1 or n % chunks or len(self.deconvs) < 2:
            x, x1, t1 = self._run_layers(self.stem_pool(x), 0, len(self.layers))
            if t1 is not None:
                raise RuntimeError('the last layer produced a chained conv1 output')
            for dc in self.deconvs[:-1]:
                x = dc(x, code)
            hm, f = self._last_deconv_head(x, keep_features)
            return hm, (x1 if keep_features else None), f
        c = n // chunks
        dt = ops.torch_dtype(code)
        dev = x.device
        if x.shape[3] == self.s2d_pad * ops.cmul(code):
            hs, ws = x.shape[1], x.shape[2]
        else:
            hs, ws = (x.shape[1] - 1) // 2 + 1, (x.shape[2] - 1) // 2 + 1
        hp, wp = (hs - 1) // 2 + 1, (ws - 1) // 2 + 1          # after maxpool = layer1 grid
        cm = ops.cmul(code)
        el = max(1, min(EARLY_LAYERS, len(self.layers) - 1))   # layers in the chunked early stage
        he, we = hp, wp
        for _ in range(el - 1):                                  # layers 2.. halve the grid
            he, we = (he - 1) // 2 + 1, (we - 1) // 2 + 1
        tail = self.layers[el - 1][-1]   # the last early block
        x2 = torch.empty((n, he, we, tail.cout * cm), dtype=dt, device=dev)
        x1 = x2 if el == 1 else (torch.empty((n, hp, wp, self.layers[0][-1].cout * cm), dtype=dt,
                                             device=dev) if keep_features else None)
        # the next layer's first conv1 over the whole batch, where the last early tail computes it chunk by
        # chunk (CHAIN_LAYERS; only an identity block chains, so its input has the shape of its output, a
        # chunk of x2), else None
        t1 = (torch.empty((n, he, we, tail.xchain.cout * cm), dtype=dt, device=dev)
              if tail.select(x2[:c], chain_out=True) == ('tail', 'layer') else None)
        chained = []
        for k in range(chunks):
            sl = slice(k * c, (k + 1) * c)
            chained.append(self._stage_early(x[sl], out=x2[sl], keep=None if (x1 is None or el == 1) else x1[sl],
                                             t1_out=None if t1 is None else t1[sl], nl=el))
        if any(chained) != all(chained):
            raise RuntimeError('the chunks of one batch took different tails')
        y, _, t1 = self._run_layers(x2, el, len(self.layers), t1=t1 if all(chained) else None)
        if t1 is not None:
            raise RuntimeError('the last layer produced a chained conv1 output')
        y = self.deconvs[0](y, code)
        hf, wf = y.shape[1] * 2 ** (len(self.deconvs) - 1), y.shape[2] * 2 ** (len(self.deconvs) - 1)
        hm = torch.empty((n, self.njoints, hf, wf), dtype=torch.float32, device=dev)
        f = (torch.empty((n, hf, wf, self.deconvs[-1].cout * cm), dtype=dt, device=dev) if keep_features else None)
        for k in range(chunks):
            sl = slice(k * c, (k + 1) * c)
            self._stage_late(y[sl], hm_out=hm[sl], f_out=None if f is None else f[sl], keep_f=f is not None)
        return hm, (x1 if keep_features else None), f
