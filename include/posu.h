/*
 * posu.h — C ABI of libposeu.so, the MI355X (gfx950) kernels behind the
 * pose-unsupervised hot path:
 *
 *   PoseResNet forward (ResNet-18..152 backbone + 3x ConvTranspose head)
 *     -> heatmap soft-argmax / argmax decoding (+ crop affine back to image px)
 *     -> epipolar (fundamental-matrix) consistency loss
 *     -> multi-view DLT triangulation.
 *
 * The reference (LouisNUST/pose-unsupervised) is pure Python/PyTorch; these
 * entry points replace the framework ops its Python functions call.  Each
 * declaration cites the reference interface it replaces (file:line relative to
 * the reference repo root).
 *
 * Conventions (all entry points):
 *   - Every tensor argument is a caller-owned DEVICE pointer (e.g. from
 *     torch.Tensor.data_ptr()).  Shapes are explicit ints; layouts are stated.
 *   - `stream` is a hipStream_t passed as void* (PyTorch's current stream).
 *     Calls only enqueue work; none synchronises, allocates or frees, so every
 *     call is hipGraph-capturable.
 *   - Return value: 0 (POSU_OK) or a POSU_ERR_* code; posu_last_error() then
 *     returns a thread-local message.
 *   - dtype codes: POSU_F32 (fp32 operands, exact-f32 MFMA, the parity mode)
 *                  POSU_BF16 (bf16 operands, f32 accumulate, the fast mode),
 *                  POSU_F16  (IEEE fp16 operands, f32 accumulate: BASELINE configs[4]'s
 *                             fp16 backbone; same kernels and speed as bf16),
 *                  POSU_F16X3 (ABI 13, split fp16: the parity-bearing fast mode).  Every value
 *                             is stored as a pair hi = fp16(v), lo = fp16(v - hi) -- v to ~22
 *                             mantissa bits -- and every product is summed as hi.hi + lo.hi +
 *                             hi.lo (three fp16 MFMAs, f32 accumulate; the lo.lo term dropped).
 *                             Split layout of a tensor of C logical channels (C % 32 == 0): 2C
 *                             fp16 per pixel, logical channel c's hi at (c / 32) * 64 + c % 32
 *                             and its lo 32 elements later ([hi 32 | lo 32] per 32-channel
 *                             block).  Entry points that accept it take LOGICAL channel counts;
 *                             packed weights use the same interleave along K (k = tap * C + ci
 *                             logical, then split per 32-block), so posu_conv_bk = 64 halves =
 *                             32 logical k per K-tile.
 */
#ifndef POSU_H_
#define POSU_H_

#ifdef __cplusplus
extern "C" {
#endif

#define POSU_OK 0
#define POSU_ERR_ARG 1          /* invalid shape / pointer / unsupported config */
#define POSU_ERR_HIP 2          /* a HIP launch failed */

#define POSU_F32 0
#define POSU_BF16 1
#define POSU_F64 2
#define POSU_F16 3
#define POSU_F16X3 4

/* ---------------------------------------------------------------- runtime */
const char* posu_last_error(void);
/* ABI revision: 4 stateless conv knobs; 5 the fused layer1 Bottleneck kernels and batched
 * weight packing; 6 the LDS-tiled packing; 7 the layer3 Bottleneck tail; 8 the crop warp
 * (posu_crop_warp); 9 the chained streamed tail (posu_bottleneck_tail_stream_next_fwd); 10 the
 * BatchNorm statistics in the conv epilogue (measured slower, removed in 11); 11 the streamed
 * tails take their weight stream's byte size, the round-2 LDS-ring layer2 block / layer3 tail
 * kernels removed, the strided tail of layer2's first block (posu_bottleneck_s2_tail_fwd) the
 * one-launch multi-view stem (posu_stem_pool_views_fwd) added, the fused deconv+head takes an
 * optional split-precision head (hw_lo); 12 the chained strided tail
 * (posu_bottleneck_s2_tail_next_fwd); 13 the split-fp16 dtype POSU_F16X3 (conv / dual / deconv /
 * deconv+head / head / pack / s2d pack / max-pool / unpack entry points); 14 (training) the ReLU
 * bit mask (posu_bn_apply_mask / posu_bn_train_bwd_mask) and the fused stem BN + ReLU + max-pool
 * with stored argmax taps (posu_bn_relu_maxpool3x3s2_fwd / posu_maxpool3x3s2_bwd_idx), the training
 * stem's convolution and weight gradient from the NCHW f32 views (posu_stem_conv_views_fwd /
 * posu_stem_wgrad_views); 15 (training) the data gradient on a chosen tile
 * (posu_conv2d_dgrad_tile: the training step autotunes it like the forward convolutions), 3x3
 * sources of the batched deconv packing (the strided 3x3 convs' sub-pixel data gradient), the
 * Adam step (posu_adam_step); 16 (round 6) the split-fp16 dtype in the streamed Bottleneck tails
 * (posu_bottleneck_tail_stream_fwd / _next_fwd, layer1 / layer2 / layer3 at 256x256) and the
 * downsampling first-block tail (posu_bottleneck_down_tail_stream_fwd).  The RPSM entry points
 * (posu_rpsm_*) and fp16 training's loss-scaling ones (posu_grad_stats, posu_grad_stats_workspace,
 * posu_adam_step_dev, posu_loss_scale_update) are additive to 16: new symbols only, the revision
 * does not move; so are the heatmap mutual-information ones and the training loop's metrics
 * (posu_pck_accuracy, posu_grad_row_norms, posu_meters_update and their workspace queries) and the
 * 3-D evaluation protocol (posu_procrustes, posu_pose3d_errors, posu_limb_break) and the
 * pseudo-label round (posu_pseudo_label_workspace, posu_pseudo_label_sweep, posu_pckh_counts) and the
 * training sample (posu_sample_workspace, posu_sample_images, posu_sample_joints_targets) and the
 * validation epoch (posu_decode_views_workspace, posu_decode_views, posu_detection_counts).  The
 * ctypes binding refuses a library of another revision. */
int posu_abi_version(void);

/* ------------------------------------------------------------ input prep */
/* NCHW fp32 image batch -> NHWC activations with Cpad (>= C) channels,
 * zero-filled above C.  Replaces the implicit layout of the first
 * nn.Conv2d call in PoseResNet.forward (lib/models/pose_resnet.py:192).
 * x: [N, C, H, W] f32.  y: [N, H, W, Cpad] of `dtype`.  hflip != 0 reads the
 * image mirrored along W (the flip test's torch.flip(view, dims=[3]),
 * lib/core/function.py:569). */
int posu_pack_nchw_to_nhwc(int dtype, const float* x, int N, int C, int H, int W,
                           void* y, int Cpad, int hflip, void* stream);

/* NCHW fp32 -> space-to-depth NHWC for the stem: y[n][i][j][(dy*2+dx)*C + c] =
 * x[n][c][2i+dy][2j+dx], zero above 4C.  The 7x7/s2/p3 stem conv then runs as a
 * 4x4/s1 conv with top/left padding 2 over this grid (K = 16 * Cpad instead of
 * 49 * Cpad taps of a Cin-padded 7x7 window).  H, W even; y: [N, H/2, W/2, Cpad];
 * hflip as above. */
int posu_pack_s2d_nchw(int dtype, const float* x, int N, int C, int H, int W,
                       void* y, int Cpad, int hflip, void* stream);

/* Batched weight packing (training: the parameters change every optimizer step).  One
 * launch packs every job of a device-resident table: fp32 PyTorch weights -> the layouts the
 * conv kernels read, in `dtype` (replaces per-layer torch packing; the modes restate
 * lib/posu/packing.py):
 *   POSU_PACK_CONV:   Conv2d [cout][cin][kh][kw] -> [rows][kpad], k = tap * pitch + ci
 *                     (posu_conv2d_fwd's w; pitch = the channel stride of the packed K);
 *   POSU_PACK_DGRAD:  the same weight flipped and transposed -> [rows >= cin][kpad],
 *                     k = tap * pitch + co, value w[co][ci][kh-1-th][kw-1-tw] (co < cout only;
 *                     posu_conv2d_dgrad's weight);
 *   POSU_PACK_DECONV: ConvTranspose2d [cin][cout][4][4] -> [4 classes][rows][kpad],
 *                     k = (ty*2 + tx) * cin + ci (posu_deconv4x4s2_fwd's w).  ABI 15: also a
 *                     [cin][cout][3][3] source (kh = kw = 3), read as its 4x4 zero-padding (tap
 *                     index 3 = 0) -- a Conv2d(3, s2, p1) weight [co][ci][3][3] packed this way
 *                     makes posu_deconv4x4s2_fwd the conv's data gradient (even H, W).
 * Zero outside the source.  block_start: the job's first block; blocks per job =
 * posu_pack_job_blocks(the job's mode .. kpad fields) (-1: kpad not a multiple of 8, a
 * deconv other than 4x4 / 3x3, or a non-positive size); total_blocks = their sum. */
#define POSU_PACK_CONV 0
#define POSU_PACK_DGRAD 1
#define POSU_PACK_DECONV 2
typedef struct posu_pack_job {
  const float* src;
  void* dst;
  long long block_start;
  int mode, cout, cin, kh, kw, pitch, rows, kpad;
} posu_pack_job;
long long posu_pack_job_blocks(int mode, int cout, int cin, int kh, int kw, int pitch, int rows, int kpad);
int posu_pack_weights(int dtype, const posu_pack_job* jobs, int njobs, long long total_blocks, void* stream);

/* NHWC activations -> NCHW fp32 (for returning x1 / f in the reference
 * layout: lib/models/pose_resnet.py:205). */
int posu_nhwc_to_nchw_f32(int dtype, const void* x, int N, int H, int W, int C,
                          float* y, void* stream);

/* ---------------------------------------------------------- convolutions */
/* Implicit-GEMM convolution on MFMA (NHWC), fused eval-mode BatchNorm
 * (per-channel scale/shift), optional residual add and ReLU:
 *     y = act( conv(x, w) * scale[co] + shift[co] + residual )
 * Replaces nn.Conv2d + nn.BatchNorm2d (+ `out += residual`) + nn.ReLU in
 * Bottleneck.forward / BasicBlock.forward (lib/models/pose_resnet.py:42-58,
 * 79-99), the stem (pose_resnet.py:192-194) and the downsample branch
 * (pose_resnet.py:136-141).
 *   x: [N, H, W, C] dtype, C % 8 == 0.
 *   w: packed [CoutPad][Kpad] dtype, k = (kh*KW + kw)*C + ci, zero padded;
 *      CoutPad = round_up(Cout, 64), Kpad = round_up(KH*KW*C, posu_conv_bk(dtype)).
 *   scale/shift: [Cout] f32 (may be NULL: scale 1, shift 0), 16-byte aligned (here and
 *   in posu_conv1x1_dual_fwd / posu_deconv4x4s2_fwd / posu_deconv4x4s2_head_fwd).
 *   residual: NULL or [N, Ho, Wo, Cout] dtype.
 *   y: [N, Ho, Wo, Cout] dtype.  `pad` is the top/left padding; Ho/Wo may be
 *   smaller than (H + 2 pad - KH) / stride + 1 (bottom/right padding implied).
 *   tile (here and in posu_conv1x1_dual_fwd / posu_deconv4x4s2_fwd): -1 = the
 *   built-in heuristic, else a fixed tile configuration cfg + 8 * variant:
 *     cfg 0: 256x64, 1: 128x64, 2: 64x64, 3: 128x128, 4: 64x128 (four waves),
 *         5: 256x256, 6: 256x128 (eight waves);
 *     variant 1: single-slot LDS ring (cfg 0-4), 2: three-slot ring (cfg != 5);
 *     + 32 (bf16 / f16): the persistent K-tile stream (cfg 0 has none and runs its plain ring);
 *        the other dtypes, and outputs of 2 GiB or more, ignore the bit;
 *     23 / 31 (bf16 / f16): 256x256 / 256x128 with waves 4-7 staggered by half a K-tile;
 *     7 / 15 (bf16 / f16, ABI 11): 128x128 with eight staggered waves (2x4 / 4x2 wave grids);
 *     39 (2-byte dtypes, ABI 13, NHWC outputs): 128x128 with two K groups of four waves (each group
 *        sums every other K-tile over the whole tile, the halves added in LDS at the end: a
 *        different K order, so not bit-identical to the other tiles);
 *     split fp16 (POSU_F16X3): 7 / 15 unstaggered; 31 (ABI 16) staggered, the lagging waves holding a
 *        K-tile's third product hi(w).lo(x) across the barrier; 47 / 55 (ABI 16, this dtype only) the
 *        staggered 128x128 eight-wave tiles (2x4 / 4x2 wave grids).
 *   An id that exists but has no kernel for the launch runs the heuristic's tile instead: a tile
 *   wider than CoutPad divides into (128 for cfg 3 / 4 / 6 and 7 / 15 / 31 / 39 / 47 / 55, 256 for
 *   cfg 5 and 23), 7 / 15 / 23 / 31 / 39 in f32, 23 in split fp16.  Refused ("tile must be"): every
 *   other id, 47 / 55 outside split fp16 among them.  The one table behind all of this is kTiles
 *   in csrc/conv_igemm.hip.
 *   The tile only changes speed (every configuration but 39 computes the same sums in the same
 *   K order); the Python plan picks it per layer by timing every admissible
 *   configuration once (PoseResNetPlan.autotune).  The library keeps no mutable state:
 *   every knob is an argument. */
int posu_conv_bk(int dtype);
/* Fused stem (replaces lib/models/pose_resnet.py:192-195, conv1 -> bn1 -> relu ->
 * maxpool, and the input pack): x NCHW f32 [N, 3, H, W] (the reference's input tensor,
 * mirrored along W when hflip), w packed [64][224] dtype (k = kh*32 + kw*4 + c, zero for
 * kw = 7 / c = 3; posu/packing.py:pack_stem_fused_weight), BN scale/shift [64] f32,
 * y NHWC [N, H/4, W/4, 64] dtype.  BF16 / F16, H % 8 == 0, W in {256, 384}; F16X3 (ABI 13, W = 256):
 * w = the hi plane [64][224] followed by the lo plane [64][224] of the weights (scaled by the
 * caller's power of two, undone in `scale`), the input split into (hi, lo) fp16 as it is staged,
 * three MFMAs per kernel row, y split [N, H/4, W/4, 128]. */
int posu_stem_pool_fwd(int dtype, const float* x, int N, int H, int W, int hflip, const void* w,
                       const float* scale, const float* shift, void* y, void* stream);
/* posu_stem_pool_fwd over the views of one forward in ONE launch (lib/models/multiview_pose_resnet.py
 * runs the backbone per view; the stem needs no per-view statistics in eval mode): views = host
 * array of nviews (1..8) device pointers to [Nv, 3, H, W] f32, y = [nviews * Nv, H/4, W/4, 64]
 * view-major.  Same values as nviews posu_stem_pool_fwd launches. */
int posu_stem_pool_views_fwd(int dtype, const float* const* views, int nviews, int Nv, int H, int W, int hflip,
                             const void* w, const float* scale, const float* shift, void* y, void* stream);
int posu_conv2d_fwd(int dtype, const void* x, int N, int H, int W, int C,
                    const void* w, int Cout, int KH, int KW, int stride, int pad,
                    const float* scale, const float* shift, const void* residual,
                    int relu, void* y, int Ho, int Wo, int tile, void* stream);

/* Two 1x1 convolutions summed into one output (Bottleneck conv3/bn3 + the
 * downsample conv/bn residual branch, lib/models/pose_resnet.py:90-99, 136-141):
 *   y[n,i,j,:] = act( W[:, :C] x[n,i,j,:] + W[:, C:] x2[n, i*stride2, j*stride2, :]
 *                     * scale + shift )
 * with the two BN scales pre-multiplied into W by the caller.
 *   x: [N, H, W, C]; x2: [N, H2, W2, C2]; C, C2 multiples of posu_conv_bk(dtype);
 *   w: [CoutPad][C + C2]; y: [N, H, W, Cout], Cout a multiple of 16 bytes (as in
 *   posu_conv2d_fwd: the epilogues store whole 16-byte channel chunks). */
int posu_conv1x1_dual_fwd(int dtype, const void* x, int N, int H, int W, int C,
                          const void* x2, int H2, int W2, int C2, int stride2,
                          const void* w, int Cout, const float* scale, const float* shift,
                          int relu, void* y, int tile, void* stream);

/* ConvTranspose2d(kernel 4, stride 2, padding 1, output_padding 0) as four
 * stride-1 2x2 sub-pixel convolutions (one per output parity class) in one
 * launch, + fused BN + ReLU.  Replaces _make_deconv_layer's
 * ConvTranspose2d/BatchNorm2d/ReLU triples (lib/models/pose_resnet.py:164-189).
 *   x: [N, H, W, C] dtype.
 *   w: packed [4 classes][CoutPad][Kpad] dtype (see posu_pack_deconv4x4 in
 *      the Python layer), class = py*2 + px, k = (ty*2 + tx)*C + ci.
 *   y: [N, 2H, 2W, Cout] dtype. */
int posu_deconv4x4s2_fwd(int dtype, const void* x, int N, int H, int W, int C,
                         const void* w, int Cout, const float* scale,
                         const float* shift, int relu, void* y, int tile, void* stream);

/* Fused Bottleneck block, eval mode (lib/models/pose_resnet.py:61-99 with the BNs folded):
 *   y = relu( conv3(relu(conv2_3x3(relu(conv1(x) * s1 + b1)) * s2 + b2)) * s3 + b3 + x )
 * in one launch that streams each image's rows once: the two planes-wide intermediates stay
 * in LDS / registers, x is read from HBM once (conv1 input and residual) and y written
 * once.  Identity residual (no downsample), stride 1.  Built for layer1 of PoseResNet at
 * 256x256: W = 64, C = 256, P = 64; dtype BF16 / F16.
 *   x, y: [N, H, W, C] (y must not alias x);
 *   w1: [P][C] with the input channels permuted: column 32 s + 8 q + e holds channel
 *       32 s + 16 (q & 1) + 8 (q >> 1) + e, s1/b1 [P] f32;
 *   w2: [P][9 * P] (posu_conv2d_fwd packing of conv2, k = (kh * 3 + kw) * P + ci), s2/b2 [P];
 *   w3: [C][P] with the input channels of every 32-block permuted: column 32 b + 8 q + e
 *       holds input channel 32 b + 16 (e >> 2) + 4 q + (e & 3) (the order in which conv2's
 *       accumulators become conv3's MFMA operand), s3/b3 [C]. */
int posu_bottleneck_fwd(int dtype, const void* x, int N, int H, int W, int C, int P, const void* w1,
                        const float* s1, const float* b1, const void* w2, const float* s2,
                        const float* b2, const void* w3, const float* s3, const float* b3, void* y,
                        void* stream);

/* The tail of an identity Bottleneck of layer2 (W = 32, C = 512, P = 128) or layer3 (W = 16,
 * C = 1024, P = 256) (lib/models/pose_resnet.py:79-99) with the weights streamed from L2
 * straight into registers (each wave loads its own 2 n-tiles' MFMA fragments a few k-steps
 * ahead; no LDS weight ring): conv2 3x3 + BN2 + ReLU -> conv3 1x1 + BN3 + residual + ReLU.
 * t1 [N, H, W, P] (conv1 output), x [N, H, W, C], y [N, H, W, C], H a multiple of 8.
 * wstream: packing.pack_tail_stream of the conv2 [P][9P] and conv3 [C][P] posu_conv2d_fwd packs,
 * [P/32][9 P/32 + C/32][2][64][8] elements of dtype; wstream_bytes = its size in bytes (checked
 * against what the kernel reads: a pack for another layer or the chained variant's pack is
 * refused, never read past).  Bit-identical to posu_conv2d_fwd(conv2) followed by
 * posu_conv2d_fwd(conv3, residual). */
int posu_bottleneck_tail_stream_fwd(int dtype, const void* t1, const void* x, int N, int H, int W, int C,
                                    int P, const void* wstream, long long wstream_bytes, const float* s2,
                                    const float* b2, const float* s3, const float* b3, void* y, void* stream);

/* posu_bottleneck_tail_stream_fwd chained with the NEXT identity Bottleneck's conv1 (1x1, C -> P)
 * + BN1 + ReLU over this block's output y (lib/models/pose_resnet.py:79-84 of block i+1; the
 * reference runs it as a separate conv over y): each y chunk of P channels is staged in LDS as
 * it is produced and multiplied into the next conv1's accumulators, so y is not re-read and the
 * next block's conv1 launch disappears.  wstream: packing.pack_tail_stream(conv2, conv3, next
 * conv1 [P][C] pack) -- [P/32][9 P/32 + 2 C/32][2][64][8]; s1n/b1n [P] the next conv1's folded
 * BN; t1n [N, H, W, P] out (aliasing no other operand).  y and t1n are bit-identical to this
 * tail followed by posu_conv2d_fwd(next conv1, ReLU) over y. */
int posu_bottleneck_tail_stream_next_fwd(int dtype, const void* t1, const void* x, int N, int H, int W, int C,
                                         int P, const void* wstream, long long wstream_bytes, const float* s2,
                                         const float* b2, const float* s3, const float* b3, void* y,
                                         const float* s1n, const float* b1n, void* t1n, void* stream);

/* (ABI 16) Both tails above also take POSU_F16X3 (split fp16 pairs, [N, H, W, 2 C] storage, C and P
 * logical), at layer1 (W = 64, C = 256, P = 64; 2-row tiles), layer2 (W = 32; 2-row tiles) and
 * layer3 (W = 16; 4-row tiles) of PoseResNet at 256x256: every k-step pair multiplied as hi.hi +
 * lo(w).hi(x) + hi(w).lo(x), bit-identical to the split posu_conv2d_fwd launches they replace;
 * wstream = packing.pack_tail_stream of the split packs (K' = 2 K).
 *
 * The FIRST Bottleneck of layer1 (lib/models/pose_resnet.py:61-99 with its stride-1 downsample,
 * pose_resnet.py:136-141; eval BN folded), split fp16 only: conv2 + the [conv3 | downsample] dual
 * GEMM + ReLU in one launch,
 *   y = relu( [w3*s3 | wd*sd] . [ relu(bn2(conv2_3x3(t1))) ; x ] * s3 + b3 ),
 * = posu_conv2d_fwd(conv2) then posu_conv1x1_dual_fwd(t2, x, stride 1), bit for bit.  t1 [N, H, 64, P]
 * (conv1's output), x [N, H, 64, P] (the block input), y [N, H, 64, C] with C = 256, P = 64
 * (logical channels), H even.  s3 / b3: the dual GEMM's scale (the split weight exponent's 2^-e) and
 * shift (b3 + bd).  s1n / b1n / t1n: optional (all null, or all given) -- the next identity block's
 * conv1 + BN1 + ReLU over y, as posu_bottleneck_tail_stream_next_fwd.  wstream =
 * packing.pack_down_tail_stream(conv2 pack, dual pack[, next conv1 pack]). */
/* (ABI 16) The LAST identity block of a layer chained with the NEXT layer's first conv1 + BN1 + ReLU
 * (1x1 / stride 1 over y, C -> Pn = 2 P at this map size: layer2 / 3 / 4 block 0's conv1,
 * lib/models/pose_resnet.py:79-81) at 256x256: the split fp16 tails of layers 1-3 and the bf16 / fp16 tails of
 * layers 2-3 (their 4-m-tile variants: layer2 2-row, layer3 4-row tiles); Pn = P is
 * posu_bottleneck_tail_stream_next_fwd.  Each y chunk's next-conv1 k-steps run twice, once per half
 * of the Pn outputs (two accumulator sets); t1n [N, H, W, Pn] (logical), s1n / b1n [Pn] f32, wstream =
 * packing.pack_tail_stream(conv2, conv3, next conv1 [Pn][C']).  Bit-identical to the tail followed by
 * posu_conv2d_fwd(next conv1) over y. */
int posu_bottleneck_tail_stream_chain_fwd(int dtype, const void* t1, const void* x, int N, int H, int W, int C,
                                          int P, int Pn, const void* wstream, long long wstream_bytes,
                                          const float* s2, const float* b2, const float* s3, const float* b3,
                                          void* y, const float* s1n, const float* b1n, void* t1n, void* stream);
int posu_bottleneck_down_tail_stream_fwd(int dtype, const void* t1, const void* x, int N, int H, int W, int C,
                                         int P, const void* wstream, long long wstream_bytes, const float* s2,
                                         const float* b2, const float* s3, const float* b3, void* y,
                                         const float* s1n, const float* b1n, void* t1n, void* stream);

/* The tail of the FIRST Bottleneck of layer2 (lib/models/pose_resnet.py:61-99 with the downsample
 * branch, pose_resnet.py:136-141; eval BN folded) of PoseResNet at 256x256, in one launch:
 *   y = relu( [w3*s3 | wd*sd] . [ relu(bn2(conv2_3x3_stride2(t1))) ; x(2 oy, 2 ox) ] + shift ),
 * i.e. posu_conv2d_fwd(conv2, stride 2) followed by posu_conv1x1_dual_fwd(t2, x, stride 2) with t2
 * kept on chip.  t1 [N, H, 64, 128] (conv1's output), x [N, H, 64, 256] (the block input),
 * y [N, H/2, 32, 512]; H a multiple of 8; BF16 / F16.  s2 / b2: conv2's folded BN [128] f32;
 * shift = b3 + bd [512] f32 (16-B aligned).  wstream: packing.pack_s2_tail_stream of the conv2
 * [128][1152] and dual [512][384] posu_conv2d_fwd / posu_conv1x1_dual_fwd packs,
 * [4][84][2][64][8] elements of dtype; wstream_bytes its size (checked).  Bit-identical to the two
 * launches (same MFMA sequence per accumulator). */
int posu_bottleneck_s2_tail_fwd(int dtype, const void* t1, const void* x, int N, int H, int W, int C, int P,
                                const void* wstream, long long wstream_bytes, const float* s2, const float* b2,
                                const float* shift, int Cout, void* y, void* stream);

/* The same, chained with the next (identity) Bottleneck's conv1 + BN1 + ReLU (ABI 12), as
 * posu_bottleneck_tail_stream_next_fwd chains the identity tails: while each 128-channel chunk of
 * y is produced, the tail also runs the next block's conv1 over it, and writes
 * t1n = relu(conv1n(y) * s1n + b1n) [N, H/2, 32, 128] -- bit-identical to posu_conv2d_fwd over y
 * (lib/models/pose_resnet.py:79-81 of layer2's block 1), which then has no conv1 launch and y is
 * not re-read for it.  wstream: packing.pack_s2_tail_stream(conv2 pack, dual pack, next conv1
 * pack [128][512]), [4][100][2][64][8]; s1n / b1n the next conv1's folded BN [128] f32 (16-B
 * aligned); t1n must alias no other operand. */
int posu_bottleneck_s2_tail_next_fwd(int dtype, const void* t1, const void* x, int N, int H, int W, int C, int P,
                                     const void* wstream, long long wstream_bytes, const float* s2, const float* b2,
                                     const float* shift, int Cout, void* y, const float* s1n, const float* b1n,
                                     void* t1n, void* stream);

/* The two tails above with the block's own conv1 folded in (additive, ABI 16): each tile computes
 *   t1 = relu(conv1_1x1(x) * s1 + b1)
 * on its 9 x 33 window from x (zeros outside the image: conv2's padding) instead of reading it, so
 * the block is ONE launch and t1 never exists in memory.  Arguments as above without t1, plus
 * s1 / b1: conv1's folded BN [128] f32 (16-B aligned).  wstream:
 * packing.pack_s2_tail_stream(conv2 pack, dual pack[, next conv1 pack], w1=conv1 pack [128][256]):
 * conv1's 8 k-steps in front, [4][92][2][64][8] (chained: [4][108]...).  y (and t1n) are
 * bit-identical to posu_conv2d_fwd(conv1) followed by posu_bottleneck_s2_tail[_next]_fwd. */
int posu_bottleneck_s2_front_tail_fwd(int dtype, const void* x, int N, int H, int W, int C, int P, const float* s1,
                                      const float* b1, const void* wstream, long long wstream_bytes,
                                      const float* s2, const float* b2, const float* shift, int Cout, void* y,
                                      void* stream);
int posu_bottleneck_s2_front_tail_next_fwd(int dtype, const void* x, int N, int H, int W, int C, int P,
                                           const float* s1, const float* b1, const void* wstream,
                                           long long wstream_bytes, const float* s2, const float* b2,
                                           const float* shift, int Cout, void* y, const float* s1n,
                                           const float* b1n, void* t1n, void* stream);

/* The same fused block for the first Bottleneck of layer1 (lib/models/pose_resnet.py:61-99
 * with the downsample branch, pose_resnet.py:136-141): conv3/bn3 and the 1x1 downsample/bn
 * share one accumulator (as in posu_conv1x1_dual_fwd),
 *   y = relu( [w3*s3 | wd*sd] . [t2 ; x] + shift3 ),  t2 = conv2 output as above,
 * x read once (conv1 input and downsample input), y written once.  W = 64, C = P = 64,
 * 4P = 256 output channels; dtype BF16 / F16.
 *   x: [N, H, W, C]; y: [N, H, W, 4P] (must not alias x);
 *   w1: [P][C] (natural channel order), s1/b1 [P]; w2, s2, b2 as posu_bottleneck_fwd;
 *   w3d: [4P][2P]: columns 0..P-1 = conv3 weight * s3 with the posu_bottleneck_fwd column
 *        permutation of w3, columns P..2P-1 = downsample weight * sd (natural order);
 *   shift3: [4P] f32 = b3 + bd. */
int posu_bottleneck_down_fwd(int dtype, const void* x, int N, int H, int W, int C, int P,
                             const void* w1, const float* s1, const float* b1, const void* w2,
                             const float* s2, const float* b2, const void* w3d, const float* shift3,
                             void* y, void* stream);

/* Cross-view Aggregation (multiview_pose_resnet.py:16-58, ChannelWiseFC / Aggregation,
 * NETWORK.AGGRE): the V(V-1) per-pair [HW x HW] matrices form one block matrix with
 * zero diagonal blocks (scaled by 1/(V-1)), so all V aggregated views are ONE GEMM:
 *   posu_pack_view_rows: x[m][o*HW + q] = src[o][m][q]   (src f32 [V][M][HW], M = N*J)
 *   posu_gemm_rows_f32:  out[blk][m][j] = sum_k x[m][k] * wt[blk*vblk + j][k]  (f32,
 *                        view-major output, vblk = HW; wt packed [round_up(Ncol,64)][K])
 * K must be a power of two and a multiple of the K-tile. */
int posu_pack_view_rows(int dtype, const float* src, int V, int M, int HW, void* dst, void* stream);
int posu_gemm_rows_f32(int dtype, const void* x, int M, int K, const void* wt, int Ncol, int vblk,
                       float* out, void* stream);

/* The last deconv stage fused with the final 1x1 head: deconv + BN + ReLU as
 * posu_deconv4x4s2_fwd, then per output pixel hm[n][j][pix] = bias[j] +
 * sum_c hw[j][c] f[c] (lib/models/pose_resnet.py:202-203) from the tile still in LDS,
 * so the 256-channel deconv output need not round-trip through HBM.
 *   y: NULL (do not store f) or [N, 2H, 2W, Cout] dtype; Cout == 256;
 *   hw: packed head weight [>= 16][round_up(Cout, posu_conv_bk)] dtype (rows >= J zero);
 *   hw_lo (ABI 11): NULL, or (BF16 / F16) the head weight's rounding residual w - hw rounded to
 *   the dtype, same layout: the split-precision head -- the deconv output f enters as
 *   round(f) + round(f - round(f)) and the head sums hi.hi + lo.hi + hi.lo products (three MFMAs
 *   per fragment), so the heatmaps carry about twice the dtype's mantissa instead of f's
 *   rounding to the dtype (the largest single source of the 2-byte chains' joint error,
 *   DESIGN.md section 5); f itself is still stored rounded;
 *   hbias: [J] f32; hm: [N, J, 2H, 2W] f32; J <= 16. */
int posu_deconv4x4s2_head_fwd(int dtype, const void* x, int N, int H, int W, int C,
                              const void* w, int Cout, const float* scale, const float* shift,
                              void* y, const void* hw, const void* hw_lo, int J, const float* hbias,
                              float* hm, void* stream);

/* 1x1 convolution (+bias) writing NCHW fp32 heatmaps: PoseResNet.final_layer
 * (lib/models/pose_resnet.py:126-132, 203).
 *   x: [N, H, W, C] dtype; w: packed [CoutPad][Kpad]; bias: [Cout] f32;
 *   y: [N, Cout, H, W] f32. */
int posu_head1x1_nchw_fwd(int dtype, const void* x, int N, int H, int W, int C,
                          const void* w, int Cout, const float* bias, float* y,
                          void* stream);

/* MaxPool2d(3, stride 2, padding 1) on NHWC (lib/models/pose_resnet.py:113,195).
 * y: [N, Ho, Wo, C], Ho = (H - 1) / 2 + 1. */
int posu_maxpool3x3s2_fwd(int dtype, const void* x, int N, int H, int W, int C,
                          void* y, void* stream);

/* ---------------------------------------------------- heatmap -> coords */
/* Soft-argmax (generate_integral_preds_2d_th, lib/utils/transforms.py:149-171):
 *   p = softmax(beta * h) over H*W (beta = 100 in the reference),
 *   x = sum p * col, y = sum p * row,
 * optionally followed by the per-sample crop affine of transform_back_th
 * (lib/utils/transforms.py:174-198): [x, y, 1] @ T^T.
 *   hm: [N, J, H, W] f32 contiguous; affine: NULL or [N, 2, 3] f32;
 *   out: [N, J, 2] f32.  stats: NULL or [N, J, 4] f32 = (max of beta*h,
 *   sum of exp, x, y in heatmap px) kept for the backward pass. */
int posu_softargmax2d_fwd(const float* hm, int N, int J, int H, int W, float beta,
                          const float* affine, float* out, float* stats, void* stream);

/* Gradient of posu_softargmax2d_fwd w.r.t. hm, given gout [N, J, 2]:
 *   dh = beta * p * ((col - x) * gx' + (row - y) * gy'), g' = T_lin^T g.
 * ghm: [N, J, H, W] f32 (overwritten). */
int posu_softargmax2d_bwd(const float* hm, const float* stats, int N, int J, int H, int W,
                          float beta, const float* affine, const float* gout, float* ghm,
                          void* stream);

/* Argmax decoding + quarter-pixel post-process + crop affine back
 * (get_max_preds / get_final_preds, lib/core/inference.py:19-75).
 *   First maximum wins (np.argmax); coords zeroed when maxval <= 0;
 *   post_process != 0 applies the +-0.25 px shift (inference.py:57-66);
 *   affine: NULL or [N, 2, 3] f64 (transform_preds, transforms.py:67-73, which
 *   applies the cv2 float64 matrix in float64 before storing float32).
 *   preds: [N, J, 2] f32; maxvals: [N, J] f32. */
int posu_argmax2d_fwd(const float* hm, int N, int J, int H, int W, int post_process,
                      const double* affine, float* preds, float* maxvals, void* stream);

/* Per-sample 2-D affine of joint coordinates (transform_back_th's
 * `[x, y, 1] @ T^T`, lib/utils/transforms.py:190-195):
 *   transpose == 0: out = [x, y, 1] @ T^T            (forward)
 *   transpose == 1: out = g @ T[:, :, 0:2]            (its gradient w.r.t. pts)
 *   pts: [N, J, 2] f32; T: [N, 2, 3] f32; out: [N, J, 2] f32. */
int posu_affine2d_apply(const float* pts, const float* T, int N, int J, int transpose,
                        float* out, void* stream);

/* Weighted heatmap MSE (JointsMSELoss.forward, lib/core/loss.py:70-86):
 *   loss = sum_j mean_{n,p} (pred*w_nj - gt*w_nj)^2 = sum_{n,j,p} (w (pred-gt))^2 / (N*HW)
 *   pred, gt: [N, J, HW] f32; w: NULL (use_target_weight False) or [N, J] f32;
 *   ws: workspace [N*J] f32 (per-map partial sums, fixed-order final sum);
 *   loss: [1] f32. */
int posu_joints_mse_fwd(const float* pred, const float* gt, const float* w, int N, int J, int HW,
                        float* ws, float* loss, void* stream);

/* Gradient of posu_joints_mse_fwd w.r.t. pred given gloss [1] (device):
 *   gpred = gloss * 2 w^2 (pred - gt) / (N*HW).  gpred: [N, J, HW] f32. */
int posu_joints_mse_bwd(const float* pred, const float* gt, const float* w, int N, int J, int HW,
                        const float* gloss, float* gpred, void* stream);

/* Flip test (lib/core/function.py:566-583): heatmaps of the mirrored input brought
 * back -- W mirrored, joint channels permuted by the dataset's flip pairs
 * (flip_back_th, lib/utils/transforms.py:33-47), optionally shifted right by one
 * column (SHIFT_HEATMAP, function.py:579-582) -- and, when hm is non-NULL, averaged
 * with the plain heatmaps: out = 0.5 * (hm + flip_back(hm_flipped)).
 *   hm_flipped, hm, out: [N, J, H, W] f32 (out may alias hm); perm: NULL or [J] int32
 *   device array, perm[j] = the joint whose flipped map becomes joint j. */
int posu_flip_back(const float* hm_flipped, const int* perm, const float* hm, int N, int J,
                   int H, int W, int shift, float* out, void* stream);

/* ------------------------------------------------------------ data path */
/* The crop of JointsDatasetCompatible.__getitem__ (lib/dataset/joints_dataset_compatible.py
 * :161-172): per sample, cv2.warpAffine(img, trans, (dw, dh), flags=INTER_LINEAR) with the
 * default constant-0 border, computed as OpenCV 3.4 does (the matrix inverted in double,
 * coordinates in 1/1024-px fixed point rounded half to even, 1/32-px bilinear weights, 15-bit
 * fixed-point sum); mode 1 fuses torchvision ToTensor + Normalize (the network input).
 *   src: uint8 HWC images, sample n at byte offset src_off[n] with height / width
 *        src_hw[2n], src_hw[2n + 1], C channels (all device arrays);
 *   M:   [N][2][3] f64 src -> dst matrices (get_affine_transform, not inverted);
 *   mode 0: out uint8 [N, dh, dw, C] (cv2.warpAffine's result);
 *   mode 1: out f32 [N, C, dh, dw] = (v / 255 - mean[c]) / std[c] (mean, std: [C] f32). */
int posu_crop_warp(const unsigned char* src, const long long* src_off, const int* src_hw, int C,
                   const double* M, int N, int dh, int dw, int mode, const float* mean, const float* std,
                   void* out, void* stream);

/* Gaussian target heatmaps of a batch (JointsDatasetCompatible.generate_heatmap,
 * lib/dataset/joints_dataset_compatible.py:215-253): joints [N, J, 2] f32 in crop px,
 * vis [N, J] f32 (joints_vis[:, 0]); target [N, J, hm_h, hm_w] f32, weight [N, J] f32;
 * zero_weight: NULL or [N] uint8 (1 = weights zeroed: H36M samples without pseudo labels). */
int posu_gaussian_targets(const float* joints, const float* vis, int N, int J, int image_w,
                          int image_h, int hm_w, int hm_h, double sigma,
                          const unsigned char* zero_weight, float* target, float* weight,
                          void* stream);

/* The training sample of JointsDatasetCompatible.__getitem__ (lib/dataset/joints_dataset_compatible.py
 * :111-201) for N records per enqueue, in two calls: the images and the labels.
 *
 * One record's colour jitter: torchvision ColorJitter (joints_dataset_compatible.py:67-71) with its drawn
 * parameters.  order: the four operations by torchvision's fn_id (0 brightness, 1 contrast, 2 saturation,
 * 3 hue) in the order they run; any other value is skipped.  hue_shift: trunc(hue * 255) mod 256 (adjust_hue's
 * uint8 add).  active = 0: the record is not jittered. */
typedef struct posu_jitter {
  float brightness, contrast, saturation;
  unsigned char order[4];
  unsigned char hue_shift;
  unsigned char active;
  unsigned char reserved[2];
} posu_jitter;

/* Bytes of posu_sample_images' workspace for N records (one 64-bit sum each); -1 for N < 0. */
long long posu_sample_workspace(int N);

/* The input crops: per record
 *   flip    flip[n] != 0: data_numpy[:, ::-1, :] before the warp (:156) -- a source tap at column tx reads
 *           column W - 1 - tx, the border test stays on tx (exact; the matrix is not touched);
 *   warp    posu_crop_warp's arithmetic (:162-165);
 *   jitter  on the uint8 RGB triple (:168-172; bgr != 0: the source is cv2's BGR, reversed before and after),
 *           PIL's arithmetic: ImageEnhance's blends d + f * (x - d) in f32 (truncated for 0 <= f <= 1, else
 *           clipped to [0, 255] and truncated) against black (brightness), the pixel's own
 *           L = (19595 R + 38470 G + 7471 B + 0x8000) >> 16 (saturation) and one grey per image,
 *           int(mean(L) + 0.5) (contrast); the hue as Convert.c's RGB -> HSV, H += hue_shift mod 256,
 *           HSV -> RGB, done for a shift of 0 too (the round trip is lossy);
 *   output  mode 0: uint8 [N, dh, dw, 3]; mode 1: ToTensor + Normalize (:173), f32 [N, 3, dh, dw].
 * src, src_off, src_hw, M, mode, mean, std: as posu_crop_warp's, C == 3.  flip: NULL or [N] uint8;
 * jitter: NULL or [N] records (device).  contrast != 0 when some active record has a contrast step: a first
 * pass then recomputes the warp and the operations before that step and sums L exactly (integers, one
 * 64-bit atomic per block) into the workspace, which is zeroed on the stream first; without it the
 * contrast step must not occur.  workspace: posu_sample_workspace(N) bytes, needed with jitter records;
 * after the call it holds the records' L sums ([N] uint64, 0 for records without a contrast step).
 * Nothing is allocated and nothing synchronises: the call can be captured. */
int posu_sample_images(const unsigned char* src, const long long* src_off, const int* src_hw, int C,
                       const double* M, const unsigned char* flip, const posu_jitter* jitter, int contrast,
                       int bgr, int N, int dh, int dw, int mode, const float* mean, const float* std,
                       void* workspace, long long workspace_bytes, void* out, void* stream);

/* The labels, in one launch and in f64 where the reference is f64: per record
 *   flip    fliplr_joints (lib/utils/transforms.py:50-64): x = W - x - 1 with W = src_hw[2n + 1], the pair
 *           swap of joints and vis (joint j reads joint perm[j]), joints * vis;
 *   affine  [x, y, 1] . trans^T for the joints with vis[:, 0] > 0 (:175-177, transforms.py:112-120).  numpy
 *           hands the product to BLAS, whose kernels fuse one multiply-add; its two forms are reproduced:
 *           fma(y, t1, x * t0) + t2 with two or more visible joints, fma(x, t0, y * t1) + t2 with one;
 *   target  generate_heatmap (:207-253): mu = int(joint / stride + 0.5) in f64, the Gaussian in f32 with
 *           numpy's own float32 exp (its AVX2 / AVX512F kernel: faithful, not correctly rounded) restated.
 * joints, vis: [N, J, 2] f64 (vis: the first two columns of joints_vis); flip: NULL or [N] uint8 (then
 * src_hw [N][2] int32 and perm [J] int32 are needed); M: [N][2][3] f64; zero_weight: NULL or [N] uint8.
 * joints_out, vis_out: [N, J, 2] f64 (meta's joints_2d_transformed / joints_vis); target [N, J, hm_h, hm_w]
 * f32; weight [N, J] f32. */
int posu_sample_joints_targets(const double* joints, const double* vis, const unsigned char* flip,
                               const int* src_hw, const int* perm, const double* M,
                               const unsigned char* zero_weight, int N, int J, int image_w, int image_h,
                               int hm_w, int hm_h, double sigma, double* joints_out, double* vis_out,
                               float* target, float* weight, void* stream);
/* Sum-normalised integral coordinates (run/test/test_integral.py:63-70):
 * out[n][j] = (sum x h, sum y h) / sum h  over hm [N, J, H, W] f32 -> [N, J, 2] f32. */
int posu_integral2d_fwd(const float* hm, int N, int J, int H, int W, float* out, void* stream);

/* ------------------------------------------------------------- geometry */
/* Epipolar consistency loss (FundamentalLoss.__call__, lib/core/loss.py:101-133):
 *   loss = sum_{b, (i,j) in permutations(V,2), k} |x~_j^T F_{s(b),i,j} x~_i| * w_i w_j
 *          / (N * V*(V-1) * J)
 *   x: [V, N, J, 2] f32 (image px); w: NULL or [V, N, J] f32 (target weights,
 *   used when non-NULL, i.e. USE_TARGET_WEIGHT_FUND);
 *   F: [S, V*(V-1), 3, 3] f32, pair index p enumerates itertools.permutations
 *   order; subj: [N] int32 in [0, S).
 *   loss: [1] f32 (written, not accumulated); resid: NULL or [N, P, J] f32. */
int posu_epipolar_loss_fwd(const float* x, const float* w, const float* F,
                           const int* subj, int V, int N, int J, int S,
                           float* loss, float* resid, void* stream);

/* d loss / d x given the scalar upstream gradient gloss [1] (device).
 * gx: [V, N, J, 2] f32 (overwritten). */
int posu_epipolar_loss_bwd(const float* x, const float* w, const float* F,
                           const int* subj, int V, int N, int J, int S,
                           const float* gloss, float* gx, void* stream);

/* Multi-view linear triangulation (triangulate_poses / pymvg
 * MultiCameraSystem.find3d, lib/multiviews/triangulate.py:43-99): per
 * (group, joint), undistort each visible view's point with the OpenCV
 * fixed-point model (5 iterations), build 2 DLT rows per view
 * (x*M[2]-M[0], y*M[2]-M[1]) and take the right singular vector of the
 * smallest singular value (one-sided Jacobi SVD, fp64).  Joints seen in < 2
 * views give (0,0,0) (triangulate.py:95-96).
 *   M:    [G, V, 3, 4] f64 projection matrices K[R | -R C];
 *   intr: [G, V, 9] f64 = fx, fy, cx, cy, k1, k2, p1, p2, k3;
 *   xy:   pixel coords in xy_dtype (POSU_F32 or POSU_F64); joint k of view v of
 *         group g at xy[g*xy_stride_g + v*xy_stride_v + 2k] (elements):
 *         [G, V, J, 2] -> (V*J*2, J*2); view-major [V, G, J, 2] -> (J*2, G*J*2);
 *   vis:  NULL (all visible) or [G, V, J] uint8;
 *   undistort: 0 = no_distortion cameras (distortion ignored);
 *   X:    [G, J, 3] f64. */
int posu_triangulate_dlt(const double* M, const double* intr, const void* xy, int xy_dtype,
                         int xy_stride_g, int xy_stride_v, const unsigned char* vis, int G,
                         int V, int J, int undistort, double* X, void* stream);

/* Pseudo-label RANSAC (multiviews/triangulate.py:102-165, ransac): per (group, joint),
 * every pair of visible views (itertools.combinations order) is triangulated (DLT on
 * undistorted points), re-projected into all V views (pymvg find2d: [R|t] = K^-1 M,
 * OpenCV plumb-bob distortion of intr), and views with error < reproj_thre are that
 * pair's inliers; pairs with fewer than min_inliers (>= 1) are skipped; the best pair has
 * the most inliers, ties broken by the smaller mean error.  res_vis[g][v][k] = 1 for the
 * best pair's inliers, else 0.  xy: [G, V, J, 2] f64 (all views, visible or not);
 * vis: NULL or [G, V, J] uint8; 2 <= V <= 4. */
int posu_ransac_inliers(const double* M, const double* intr, const double* xy,
                        const unsigned char* vis, int G, int V, int J, int undistort,
                        double reproj_thre, int min_inliers, unsigned char* res_vis, void* stream);
/* reproject_poses (triangulate.py:168-213): triangulate each joint from its visible
 * views and project into every view: proj [G, V, J, 2] f64 and res_vis = 1 where the
 * joint has >= 2 visible views (zeros otherwise). */
int posu_reproject(const double* M, const double* intr, const double* xy, const unsigned char* vis,
                   int G, int V, int J, int undistort, double* proj, unsigned char* res_vis,
                   void* stream);

/* Differentiable triangulation and the reprojection-consistency loss (additive to ABI 16; csrc/
 * triangulate_grad.hip).  One thread per (group, joint), fp64, 2 <= V <= 4, no atomics: the same inputs give
 * the same bits.  M, intr, xy (with xy_dtype and the two strides, view-major included), vis and undistort are
 * posu_triangulate_dlt's.  All of them return POSU_ERR_ARG before any launch for a null required pointer, V
 * outside 2..4 or another xy dtype, and succeed without a launch when G == 0.
 *
 * posu_triangulate_dlt_w: posu_triangulate_dlt with w: NULL (then it IS posu_triangulate_dlt, bit for bit) or
 * [G, V, J] f64 row weights: the two DLT rows of view v are multiplied by w[g][v][k] (a confidence).
 *   X: [G, J, 3] f64; (0, 0, 0) for a joint seen in fewer than two views. */
int posu_triangulate_dlt_w(const double* M, const double* intr, const void* xy, int xy_dtype,
                           int xy_stride_g, int xy_stride_v, const unsigned char* vis, const double* w,
                           int G, int V, int J, int undistort, double* X, void* stream);
/* Its backward from gX [G, J, 3] f64; the forward is recomputed from the same inputs.  With A the weighted
 * 2V x 4 system, A^T A = sum lam_i q_i q_i^T, h = q_min, X = h[:3] / h[3]:
 *   gh = (gX / h3, -(gX . X) / h3),  z = sum_{i != min} q_i (q_i . gh) / (lam_min - lam_i),
 *   gA = (A z) h^T + (A h) z^T;  the row w (u m2 - m0) gives g_u = w (gA_row . m2), g_w += gA_row . (u m2 - m0);
 * g_u, g_v then go through the 2 x 2 Jacobian of the five undistortion iterations as they are computed.
 *   gxy: xy's dtype and layout (every entry of the V views is written: zero for a view that is off and for a
 *        joint seen in fewer than two views);  gw: NULL or [G, V, J] f64 (written likewise). */
int posu_triangulate_dlt_bwd(const double* M, const double* intr, const void* xy, int xy_dtype,
                             int xy_stride_g, int xy_stride_v, const unsigned char* vis, const double* w,
                             int G, int V, int J, int undistort, const double* gX, void* gxy, double* gw,
                             void* stream);
/* Reprojection loss: per (g, k) the point X of posu_triangulate_dlt_w is projected into every view with the
 * lens model of intr (as posu_reproject does), e[g][v][k] = ||proj - xy[g][v][k]|| in px, and
 *   loss = sum omega e / (G V J)         (the constant divisor, as posu_epipolar_loss_fwd has it)
 * with omega NULL (1) or [G, V, J] f64 residual weights, forced to 0 where the view is off or the joint is seen
 * in fewer than two views.  loss: [1] f64 (written, not accumulated; untouched when G == 0).
 * X: NULL or [G, J, 3] f64; e: NULL or [G, V, J] f64 (0 for a joint seen in fewer than two views).
 * workspace: posu_reprojection_loss_workspace(G, J) bytes (-1: bad shape), 8-byte aligned: one partial sum per
 * 256 (group, joint)s, summed in a fixed order by a second launch. */
long long posu_reprojection_loss_workspace(int G, int J);
int posu_reprojection_loss_fwd(const double* M, const double* intr, const void* xy, int xy_dtype,
                               int xy_stride_g, int xy_stride_v, const unsigned char* vis, const double* w,
                               const double* omega, int G, int V, int J, int undistort, double* loss,
                               double* X, double* e, void* workspace, long long workspace_bytes, void* stream);
/* d loss / d xy and d loss / d w from the device scalar gloss [1] f64.  detach_point == 0: the gradient reaches
 * xy directly (-omega r / ||r||, r = proj - xy) and through X (the projection's Jacobian, then
 * posu_triangulate_dlt_bwd's path), and reaches w through X.  detach_point != 0: X is a constant (the online
 * pseudo-label reading), only the direct term remains and gw is zero.  r = 0 contributes zero, never NaN.
 *   gxy: xy's dtype and layout;  gw: NULL or [G, V, J] f64. */
int posu_reprojection_loss_bwd(const double* M, const double* intr, const void* xy, int xy_dtype,
                               int xy_stride_g, int xy_stride_v, const unsigned char* vis, const double* w,
                               const double* omega, int G, int V, int J, int undistort, int detach_point,
                               const double* gloss, void* gxy, double* gw, void* stream);

/* ------------------------------------------------------------------- RPSM */
/* The recursive pictorial structure model (lib/multiviews/pictorial.py, driven by
 * run/test/test_rpsm.py): multi-view heatmaps -> 3-D pose by max-product inference over the
 * skeleton tree on a grid of N = nbins^3 bins, refined RECUR_DEPTH times on a small grid around
 * every joint.  These entry points are additive to ABI 16 (nothing older changes).  fp64
 * throughout, in the reference's operation order, compiled without fused multiply-adds: the
 * results are discrete decisions.  Limits: 1 <= V <= 8, 2 <= J <= 32, 2 <= nbins, N <= 4096,
 * H == W (the reference's interpolator only works for square heatmaps).
 *
 * The tree (multiviews/body.py) is three HOST int arrays, read during the call: parent [J]
 * (root = -1), child_ptr [J + 1] and child_idx [J - 1] -- node n's children, in the order of
 * its 'children' list, are child_idx[child_ptr[n] .. child_ptr[n + 1]).  Edge e (a row of the
 * packed constraint) is the edge into child_idx[e].  Limb lengths are indexed by the child joint
 * (the root's entry is ignored): a DEVICE f64 table [G, J], one row per group, where groups are
 * inferred (posu_rpsm_infer, posu_rpsm_run); HOST double [J] for the mask builder.
 * The packed constraint is uint32 [J - 1, ceil(N / 32), N]: bit (j & 31) of word [e][j / 32][i]
 * allows child bin j under parent bin i (numpy.packbits, bitorder 'little', of row i; the word
 * index outside the parent bin so that consecutive lanes read consecutive words).
 * Bin order (compute_grid, pictorial.py:108-119; numpy meshgrid 'xy'): flat bin
 * b = (a * nbins + bx) * nbins + c has coordinates (x[bx], y[a], z[c]). */

/* Bytes posu_rpsm_run needs for G groups (-1: a shape outside the limits). */
long long posu_rpsm_workspace_bytes(int G, int J, int first_nbins, int recur_nbins);
/* compute_grid (pictorial.py:108-119) for `count` boxes: centers [count, 3] f64 ->
 * grid [count, nbins^3, 3] f64, axis = linspace(-size/2, size/2, nbins) + center. */
int posu_rpsm_grid(const double* centers, int count, double size, int nbins, double* grid, void* stream);
/* compute_unary_term (pictorial.py:146-190): unary [G, J, N] f64 = sum over views of the bilinear
 * sample (scipy RegularGridInterpolator on hmap.T, linear, 0 outside [0, H-1]) of heatmaps
 * [G, V, J, H, W] f32 at the grid point projected by cameras.project_pose (cameras.py:25-54,
 * avg_f), the crop affine and * [W, H] / (img_w, img_h).
 *   cams:   [G, V, 20] f64 = R row-major [9], T [3], f = (fx + fy) / 2, cx, cy, k [3], p [2];
 *   affine: [G, V, 2, 3] f64 = get_affine_transform(center, scale, 0, image_size);
 *   grid:   [G, NG, N, 3] f64, NG = 1 (shared by the joints) or J. */
int posu_rpsm_unary(const float* heatmaps, const double* cams, const double* affine, int G, int V,
                    int J, int H, int W, double img_w, double img_h, const double* grid, int NG,
                    int N, double* unary, void* stream);
/* infer's forward pass (pictorial.py:36-65) on one grid level, one max-product launch per tree
 * depth, deepest first.  For edge (p, c) and parent bin i: v_j = P[i, j] * energy[c][j] (a
 * disallowed pair is a zero, not -inf), maxv[c][i] = max_j v_j, state[c][i] = the first j
 * attaining it; energy[p] = ((unary[p] * maxv[c1]) * maxv[c2]) ... in children order.
 *   P: mask != NULL: the packed constraint (above), shared by the groups;
 *      mask == NULL: |norm(grid[p][i] - grid[c][j]) - limb[g][c]| <= tolerance
 *      (compute_pairwise_constrain, pictorial.py:122-143), grid [G, NG, N, 3], limb DEVICE f64
 *      [G, J] (every group its own limb lengths, as run/test/test_rpsm.py:123 computes them);
 *   unary [G, J, N] f64 in; energy, maxv [G, J, N] f64 and state [G, J, N] int32 out (the root's
 *   maxv / state rows are not written). */
int posu_rpsm_infer(const double* unary, const int* parent, const int* child_ptr, const int* child_idx,
                    const unsigned int* mask, const double* grid, int NG, const double* limb,
                    double tolerance, int G, int J, int N, double* energy, double* maxv, int* state,
                    void* stream);
/* infer's back-tracking and get_loc_from_cube_idx (pictorial.py:68-105): the root takes the first
 * argmax of its energy, every other joint state[joint][its parent's bin]; bins [G, J] int32 and
 * pose [G, J, 3] f64 = the bins' grid coordinates (either may be NULL). */
int posu_rpsm_backtrack(const double* energy, const int* state, const int* parent, const int* child_ptr,
                        const int* child_idx, const double* grid, int NG, int G, int J, int N, int* bins,
                        double* pose, void* stream);
/* The packed constraint of every edge from grid [NG, N, 3] (NG = 1 or J): bit = |norm(g_p[i] -
 * g_c[j]) - limb[c]| < thr[c] (strict != 0: compute_pairwise_constraint of
 * run/test/generate_pairwise_constraints.py:60-95 on a centred grid, thr = 0.4 limb) or <= thr[c]
 * (strict == 0: pictorial.py:122-143).  limb, thr: HOST double [J] by child joint.
 * mask: the packed constraint [J - 1, ceil(N / 32), N] uint32. */
int posu_rpsm_pairwise_mask(const double* grid, int NG, int N, const int* parent, const int* child_ptr,
                            const int* child_idx, int J, const double* limb, const double* thr, int strict,
                            unsigned int* mask, void* stream);
/* rpsm (pictorial.py:214-250) for G groups, enqueued without a host synchronisation: level 1 on
 * the grid_size box of first_nbins^3 bins at grid_centers [G, 3] with the packed constraint, then
 * recur_depth refinements of recur_nbins^3 bins per joint on boxes of grid_size / first_nbins /
 * recur_nbins^level with the on-the-fly constraint from limb (DEVICE f64 [G, J], a row per
 * group).  G * J <= 65535 per call.  pose: [G, J, 3] f64; level_poses: NULL or
 * [recur_depth + 1, G, J, 3] f64 (the pose after level 1 and after every refinement);
 * workspace >= posu_rpsm_workspace_bytes(G, J, first_nbins, recur_nbins) bytes. */
int posu_rpsm_run(const float* heatmaps, const double* cams, const double* affine, int G, int V, int J,
                  int H, int W, double img_w, double img_h, const double* grid_centers, double grid_size,
                  int first_nbins, int recur_nbins, int recur_depth, double tolerance, const double* limb,
                  const unsigned int* mask, const int* parent, const int* child_ptr, const int* child_idx,
                  void* workspace, long long workspace_bytes, double* pose, double* level_poses,
                  void* stream);

/* ----------------------------------------------------------- training path */
/* BASELINE configs[3]: the data-parallel training step (run/pose2d/train.py +
 * core/function.py:91-366: per-view backbone forward in train mode, JointsMSELoss,
 * FundamentalLoss, loss.backward(), optimizer step).  Replaces the autograd of
 * torch.nn.Conv2d / ConvTranspose2d / BatchNorm2d / ReLU / MaxPool2d for the
 * PoseResNet modules (lib/models/pose_resnet.py:21-205). */

/* Data gradient of conv2d x[N,H,W,Cin] -> y[N,Ho,Wo,Cout] (KHxKW, stride 1|2, pad):
 *   dy: [N,Ho,Wo,Cout] dtype; wt: weights flipped + transposed, packed
 *   [round_up(Cin,64)][round_up(KH*KW*Cout, BK)] (K order (kh, kw, co)), i.e. the
 *   forward packing of W[:, :, ::-1, ::-1].transpose(0, 1);
 *   residual: NULL or [N,H,W,Cin] added to dx; dx: [N,H,W,Cin] dtype.
 *   Cout must be a power of two >= 8 (it is the GEMM's reduction channel count).
 *   1x1 / stride 2 / pad 0 with residual == dx: accumulated in place, dx[2i][2j] += dy[i][j] W^T,
 *   a GEMM over dy's pixels (the other pixels keep dx) instead of over the zero-upsampled grid. */
int posu_conv2d_dgrad(int dtype, const void* dy, int N, int Ho, int Wo, int Cout, const void* wt,
                      int Cin, int KH, int KW, int stride, int pad, const void* residual,
                      void* dx, int H, int W, void* stream);
/* ABI 15: the same on tile configuration `tile` (posu_conv2d_fwd's table; -1 = the built-in
 * heuristic, which posu_conv2d_dgrad runs).  Every tile except 39 accumulates in the same K order,
 * so the choice changes speed, not results.  Refused: an unknown tile. */
int posu_conv2d_dgrad_tile(int dtype, const void* dy, int N, int Ho, int Wo, int Cout, const void* wt,
                           int Cin, int KH, int KW, int stride, int pad, const void* residual,
                           void* dx, int H, int W, int tile, void* stream);

/* ABI 15: the Adam step (torch.optim.Adam, utils/utils.py:79-83; core/function.py:366) over a
 * table of f32 parameter tensors: per element g' = g (+ weight_decay p), m = b1 m + (1-b1) g',
 * v = b2 v + (1-b2) g'^2, p -= lr / (1 - b1^step) * m / (sqrt(v) / sqrt(1 - b2^step) + eps),
 * in f32 (within rounding of torch's kernels).  p, m, v updated in place; `step` = the step being
 * taken (>= 1).  The table is host memory, read during the call (the launches carry it). */
typedef struct posu_adam_tensor {
  float* p;
  const float* g;
  float* m;
  float* v;
  long long n;
} posu_adam_tensor;
int posu_adam_step(const posu_adam_tensor* tensors, int ntensors, double lr, double beta1, double beta2,
                   double eps, double weight_decay, long long step, void* stream);

/* fp16 training (additive to ABI 16): loss scaling without a host synchronisation.  The three
 * entry points below only enqueue on `stream`, allocate nothing and read whatever decides the
 * step from device memory, so a training loop keeps its run-ahead and the calls can be captured
 * in a hipGraph.  Tables are host memory, read during the call (the launches carry them).
 *
 * posu_grad_stats: one pass over a table of f32 gradient tensors.
 *   found_inf (device float[1], required): zeroed by the call (hipMemsetAsync on the stream), then
 *     1.0f if any element is inf or nan.
 *   unscale != 0: g *= 1 / *scale in place (scale: device float[1], the loss scale; required then,
 *     otherwise not read).
 *   sumsq (device double[1], or NULL): the sum of squares of the gradients as the call leaves
 *     them (after the in-place unscale, if any), squared and accumulated in double: per-block
 *     partials in `workspace` (>= posu_grad_stats_workspace bytes, needed only with sumsq) summed
 *     in a fixed order, the same bits on every run.
 * posu_grad_stats_workspace: -1 for a null table or a negative size. */
typedef struct posu_grad_tensor {
  float* g;
  long long n;
} posu_grad_tensor;
long long posu_grad_stats_workspace(const posu_grad_tensor* tensors, int ntensors);
int posu_grad_stats(const posu_grad_tensor* tensors, int ntensors, const float* scale, int unscale,
                    float* found_inf, double* sumsq, void* workspace, long long workspace_bytes,
                    void* stream);

/* posu_adam_step_dev: the update of posu_adam_step (same arithmetic) with the step count of every
 * tensor in device memory (`step`, a float holding the number of steps taken; torch's
 * capturable convention) and the bias corrections computed from it on the device, in double.
 *   found_inf (device float[1], or NULL): when non-zero the call changes nothing: p, m, v and
 *     step keep their bits.  Otherwise step += 1 first.
 *   scale (device float[1], or NULL): the gradients are read as g / *scale.
 *   sumsq (device double[1], or NULL) with max_norm > 0: the gradients are clipped to the global
 *     norm max_norm, g * min(1, max_norm / (sqrt(*sumsq) / *scale + 1e-6)), where *sumsq is the
 *     sum of squares of the gradients as stored (torch.nn.utils.clip_grad_norm_).  max_norm <= 0:
 *     no clipping.
 * With all three NULL this is a capturable plain Adam. */
typedef struct posu_adam_dev_tensor {
  float* p;
  const float* g;
  float* m;
  float* v;
  float* step;
  long long n;
} posu_adam_dev_tensor;
int posu_adam_step_dev(const posu_adam_dev_tensor* tensors, int ntensors, double lr, double beta1, double beta2,
                       double eps, double weight_decay, const float* found_inf, const float* scale,
                       const double* sumsq, double max_norm, void* stream);

/* posu_loss_scale_update: torch's _amp_update_scale_ on device scalars (one thread).  *found_inf
 * != 0: *scale *= backoff, *growth_tracker = 0; else ++*growth_tracker, and when it reaches
 * growth_interval (>= 1): *scale *= growth unless that is not finite, *growth_tracker = 0. */
int posu_loss_scale_update(float* scale, int* growth_tracker, const float* found_inf, double growth,
                           double backoff, int growth_interval, void* stream);

/* Weight gradient dW[Cout][Creal][KH][KW] (f32, the nn.Conv2d weight layout) of a
 * conv over x[N,H,W,C] (C >= Creal, padded channels ignored) with output gradient
 * dy[N,Ho,Wo,Cout].  Also ConvTranspose2d(4, s2, p1): pass x = the transposed
 * conv's output gradient (as a [N,2H,2W,Cout_t] input), dy = its input
 * [N,H,W,Cin_t], KH=KW=4, stride 2, pad 1 -> dW[Cin_t][Cout_t][4][4].
 * workspace >= posu_conv2d_wgrad_workspace(...) bytes (split-K partials). */
long long posu_conv2d_wgrad_workspace(int dtype, int N, int H, int W, int C, int Cout, int KH,
                                      int KW, int stride, int pad);
int posu_conv2d_wgrad(int dtype, const void* dy, const void* x, int N, int H, int W, int C,
                      int Creal, int Cout, int KH, int KW, int stride, int pad, float* dw,
                      void* workspace, long long workspace_bytes, void* stream);

/* Training-mode BatchNorm2d over z[nseg*Pseg, C] (NHWC, nseg batch segments = camera
 * views with separate statistics, torch.nn.functional.batch_norm(training=True)
 * per segment): mean/rstd/scale/shift [nseg, C] f32 out; running_mean/var
 * (optional) updated once per segment in order, unbiased variance. */
long long posu_bn_workspace(int nseg, int C);
int posu_bn_train_fwd(int dtype, const void* z, int nseg, int Pseg, int C, const float* gamma,
                      const float* beta, float eps, float momentum, float* running_mean,
                      float* running_var, float* mean, float* rstd, float* scale, float* shift,
                      void* workspace, long long workspace_bytes, void* stream);
/* y = act(z * scale[seg] + shift[seg] (+ residual)) */
int posu_bn_apply(int dtype, const void* z, int nseg, int Pseg, int C, const float* scale,
                  const float* shift, const void* residual, int relu, void* y, void* stream);
/* Backward of y = relu?(bn(z) (+ r)):  g' = gy * [y > 0]; without a residual the mask
 * can instead be recomputed from z with the forward's per-segment relu_scale/relu_shift
 * ([nseg, C], posu_bn_train_fwd's scale/shift: y > 0 <=> z*scale + shift > 0), which
 * saves reading y; y = relu_scale = NULL: no ReLU.
 * dz = gamma*rstd*(g' - mean(g') - xhat*mean(g'*xhat)) per segment; dgamma/dbeta
 * [C] f32 written (summed over segments); gres (optional) = g'. */
int posu_bn_train_bwd(int dtype, const void* gy, const void* y, const float* relu_scale,
                      const float* relu_shift, const void* z, int nseg, int Pseg,
                      int C, const float* mean, const float* rstd, const float* gamma,
                      float* dgamma, float* dbeta, void* dz, void* gres, void* workspace,
                      long long workspace_bytes, void* stream);
/* ABI 14: the residual Bottleneck output's ReLU mask as bits.  posu_bn_apply_mask = posu_bn_apply
 * with relu = 1 that also writes mask [nseg*Pseg*C/E] bytes (E = 8 for BF16 / F16, 4 for F32:
 * one byte per 16-B chunk, bit e = [y_e > 0] of the stored y); posu_bn_train_bwd_mask =
 * posu_bn_train_bwd reading that mask instead of y (16x fewer bytes than y, read twice per
 * backward).  Replaces the reference's autograd ReLU / BatchNorm2d backward
 * (lib/models/pose_resnet.py:92-97), results identical to the y-masked path. */
int posu_bn_apply_mask(int dtype, const void* z, int nseg, int Pseg, int C, const float* scale,
                       const float* shift, const void* residual, void* y, void* mask, void* stream);
int posu_bn_train_bwd_mask(int dtype, const void* gy, const void* mask, const void* z, int nseg,
                           int Pseg, int C, const float* mean, const float* rstd,
                           const float* gamma, float* dgamma, float* dbeta, void* dz, void* gres,
                           void* workspace, long long workspace_bytes, void* stream);
/* out[c] = sum_p x[p][c] (f32), e.g. the final layer's bias gradient;
 * workspace >= posu_bn_workspace(1, C). */
int posu_channel_sum(int dtype, const void* x, int P, int C, float* out, void* workspace,
                     long long workspace_bytes, void* stream);
/* MaxPool2d(3, 2, 1) backward (PyTorch's first-maximum tie rule), x the forward
 * input [N,H,W,C], gy [N,Ho,Wo,C] -> gx [N,H,W,C]; workspace: argmax taps. */
long long posu_maxpool3x3s2_bwd_workspace(int N, int H, int W, int C);
int posu_maxpool3x3s2_bwd(int dtype, const void* x, int N, int H, int W, int C, const void* gy,
                          void* gx, void* workspace, long long workspace_bytes, void* stream);
/* ABI 14, the training stem (lib/models/pose_resnet.py:192-195: bn1, relu, maxpool): from the
 * raw conv output z [N,H,W,C] (N = nseg equal segments) and posu_bn_train_fwd's scale/shift,
 * y [N,Ho,Wo,C] = maxpool3x3s2(relu(z*scale[seg] + shift[seg]) rounded to dtype) and idx
 * [N,Ho,Wo,C] bytes = the argmax tap 0..8 (first maximum in window order) -- the activation
 * itself is never written.  posu_maxpool3x3s2_bwd_idx: gx [N,H,W,C] from those taps and gy
 * [N,Ho,Wo,C]; identical to posu_maxpool3x3s2_bwd over the activation. */
int posu_bn_relu_maxpool3x3s2_fwd(int dtype, const void* z, int nseg, int N, int H, int W, int C,
                                  const float* scale, const float* shift, void* y, void* idx,
                                  void* stream);
int posu_maxpool3x3s2_bwd_idx(int dtype, const void* idx, const void* gy, int N, int H, int W,
                              int C, void* gx, void* stream);
/* ABI 14, the training stem's convolution (lib/models/pose_resnet.py:192, nn.Conv2d(3, 64, 7, 2, 3,
 * bias=False)) straight from the caller's NCHW f32 views (views[v] = [Nv, 3, H, W], a host array of
 * device pointers, stacked view-major like posu_stem_pool_views_fwd): z [nviews*Nv, H/2, W/2, 64]
 * of dtype (BF16 / F16) from the parameter's own f32 weight w [64][3][7][7]; and its weight
 * gradient dw [64][3][7][7] f32 from dz [nviews*Nv, H/2, W/2, 64] (workspace:
 * posu_stem_wgrad_workspace bytes of per-block partials, summed in a fixed order).  W = 256,
 * H % 8 == 0. */
int posu_stem_conv_views_fwd(int dtype, const float* const* views, int nviews, int Nv, int H, int W,
                             const float* w, void* z, void* stream);
long long posu_stem_wgrad_workspace(int N, int H, int W);
int posu_stem_wgrad_views(int dtype, const float* const* views, int nviews, int Nv, int H, int W,
                          const void* dz, float* dw, void* workspace, long long workspace_bytes,
                          void* stream);

/* ------------------------------------------------- heatmap mutual-information loss */
/* HeatmapMILoss over HeatmapDiscriminator (lib/core/loss.py:636-781, lib/models/discriminator.py
 * :225-242; called per view from lib/core/function.py:259-278).  Additive to ABI 16.  The reference
 * builds all Q x Q (feature row, heatmap value) pairs of an image as a dense [N Q Q, C + 1] tensor
 * (loss.py:705-713) and runs Linear(C + 1 -> cm, no bias) -> BatchNorm1d -> LeakyReLU(0.2) ->
 * Linear(cm -> cm / 4) -> BatchNorm1d -> LeakyReLU(0.2) -> Linear(cm / 4 -> 1) over it.  Here the
 * first Linear splits into A[n, i, :] + h[n, j] w_h with A = F_s W_f^T (W1 = [w_h | W_f]) and every
 * pass over the pairs recomputes the rest from A and h; nothing per pair is stored but the score.
 *
 *   feat:  channels-last features [S N, H, W, C] of `dtype` (POSU_F32 / POSU_BF16 / POSU_F16);
 *   hm:    heatmaps [S N, J, H, W] f32, of which joint `joint_idx` is used;
 *   idx:   DEVICE int32 [S N, Q], sampled positions in [0, H W); idx_host: NULL, or a host copy,
 *          which is then checked (an index outside the map is refused).  Without a host copy the
 *          range is the caller's contract; the kernels clamp a stray index into the map;
 *   S segments (the reference's views) of N images: BatchNorm statistics per segment over its
 *          N Q^2 rows, like posu_bn_train_fwd's nseg;
 *   params: HOST array of 13 device pointers, read during the call: W1 [cm, C + 1], gamma1, beta1,
 *          running_mean1, running_var1 [cm], W2 [cm / 4, cm], b2, gamma2, beta2, running_mean2,
 *          running_var2 [cm / 4], w3 [cm / 4], b3 [1]  (the running statistics may be NULL when
 *          training != 0; they are never written);
 *   training != 0: batch statistics; stats [S, 3, cm + cm / 4] f32 out = per segment the batch
 *          mean, the biased and the unbiased variance of BN1's cm then BN2's cm / 4 channels (the
 *          caller updates its running buffers from them, segment by segment);
 *          training == 0: the running statistics, one pass, stats not written (may be NULL);
 *   u:     [S N, Q, Q] f32 out, u[n, i, j] = the score of (feature row idx[n, i], heatmap value
 *          idx[n, j]): the reference's row order.
 * Limits (POSU_ERR_ARG before any launch): cm in {32, 64, 128}; C a multiple of 8, at most 512;
 * Q <= 256; joint_idx in [0, J); S N Q^2 cm < 2^31; non-null required pointers.
 * workspace: >= posu_heatmap_mi_workspace(S, N, Q, cm) bytes, 16-byte aligned: S N Q (cm + 2) + S N Q^2
 * floats (A, h, dh and one scalar per pair), up to 2 S N Q^2 more for the backward's dA buffers (one
 * per j slab, as many slabs as fit), plus what does not grow with the pairs (derived per-segment
 * values and the f64 partials of the reductions: *reduction_bytes, optional out).  No activation
 * 16 or 64 wide is stored per pair. */
long long posu_heatmap_mi_workspace(int S, int N, int Q, int cm, long long* reduction_bytes);
int posu_heatmap_pair_scores_fwd(int dtype, const void* feat, const float* hm, int S, int N, int H, int W,
                                 int C, int J, int joint_idx, const int* idx, const int* idx_host, int Q,
                                 int cm, const float* const* params, int training, float eps, float* stats,
                                 float* u, void* workspace, long long workspace_bytes, void* stream);
/* Its backward (the autograd of loss.py:770-773 through the discriminator) from du [S N, Q, Q],
 * recomputing the forward from the same inputs (stats: scratch of the forward's size when
 * training != 0).  Three optional outputs, NULL = not computed:
 *   dparams: f32 [posu_heatmap_dparams_floats(C, cm)] = dW1 [cm (C + 1)] | dgamma1 | dbeta1 [cm] |
 *            dW2 [cm / 4 * cm] | db2 | dgamma2 | dbeta2 | dw3 [cm / 4] | db3 [1];
 *   dfeat:   [S N, H, W, C] of `dtype`, zero outside the sampled positions;
 *   dhm:     [S N, J, H, W] f32, zero outside joint_idx and the sampled positions.
 * A position sampled more than once receives the sum over its occurrences, added in index order.
 * No floating-point atomics: two calls on the same inputs give the same bits. */
long long posu_heatmap_dparams_floats(int C, int cm);
int posu_heatmap_pair_scores_bwd(int dtype, const void* feat, const float* hm, int S, int N, int H, int W,
                                 int C, int J, int joint_idx, const int* idx, const int* idx_host, int Q,
                                 int cm, const float* const* params, int training, float eps, float* stats,
                                 const float* du, float* dparams, void* dfeat, float* dhm, void* workspace,
                                 long long workspace_bytes, void* stream);
/* The mutual-information measures on u [S N, Q, Q] (loss.py:719-757), one loss per segment:
 *   measure 0, JSD (get_jsd_loss): mean over the off-diagonal of softplus(-u) + u - log 2 minus
 *     the mean over the diagonal of log 2 - softplus(-u)  (Q >= 2);
 *   measure 1, NCE (get_infonce_loss): per (n, i) -log_softmax of [u_ii, u_i0 .. u_i,Q-1 with -10
 *     at j = i] at position 0, averaged.
 * loss: [S] f32; workspace >= posu_pair_mi_workspace(S) bytes.  Backward: du [S N, Q, Q] from
 * gloss [S] (device). */
long long posu_pair_mi_workspace(int S);
int posu_pair_mi_loss_fwd(const float* u, int S, int N, int Q, int measure, float* loss, void* workspace,
                          long long workspace_bytes, void* stream);
int posu_pair_mi_loss_bwd(const float* u, int S, int N, int Q, int measure, const float* gloss, float* du,
                          void* stream);
/* The positions HeatmapMILoss scores, drawn on the device (the reference draws them on the host,
 * lib/core/loss.py:646-703): per image the window centre, half of the window's entries without
 * replacement and a quarter as many distinct positions outside it.  Additive to ABI 16.
 *
 *   joints: DEVICE f64 [B, J, 2], (x, y) in crop px (meta['joints_2d_transformed']);
 *   vis:    DEVICE f64 [B, J], joint visible when != 0 (column 0 of meta['joints_vis']);
 *   feat_w, feat_h: crop px per map px; the map is H x W; the window is (2 radius + 1)^2;
 *   idx:    DEVICE int32 [B, Q] out; loc: DEVICE int32 [B] out, the window centres, may be NULL.
 * With P = (2 radius + 1)^2, n_in = P / 2, n_out = P / 4 (integer divisions), Q = n_in + n_out.
 *
 * The stream.  Row k's draw is a function of (seed, call, k) and of row k's inputs only: not of B,
 * of the launch geometry or of other rows, so a batch may be drawn in one launch or in pieces.  Its
 * random words are the outputs of Philox4x32-10 (multipliers 0xD2511F53, 0xCD9E8D57, Weyl constants
 * 0x9E3779B9, 0xBB67AE85) with key (seed low 32 bits, seed high 32 bits) and counter (b, k, call
 * low, call high) for b = 0, 1, 2, ..., consumed in output order.  bounded(w, n) = (w * n) >> 32 on
 * the 64-bit product maps a word to [0, n); the relative bias of an outcome is at most n / 2^32:
 * below 2.5e-7 for the window draws (n <= 1024) and for the 64 x 64 map (none at all when n is a
 * power of two), at most 1.6e-5 for the largest map allowed here.
 *   centre: gx = trunc(joints[k, joint_idx, 0] / feat_w + 0.5) in f64 (IEEE division, truncation
 *     toward zero) clamped to [0, W - 1] (NaN gives 0), gy likewise with feat_h and H, gt = gy W +
 *     gx: HeatmapMILoss.locations' integers for finite coordinates below 2^31.  Word 0 is always
 *     consumed: centre = visible ? gt : bounded(w0, H W) (the reference's uniform centre for an
 *     invisible joint, loss.py:698; image k keeps slot k);
 *   window: entry e = (dy + radius)(2 radius + 1) + (dx + radius) holds clamp(centre + dy W + dx, 0,
 *     H W - 1): the LINEAR index is clamped (loss.py:654-657), so a window at a border repeats
 *     positions;
 *   inside: a partial Fisher-Yates over the P entries: perm = identity; for t = 0 .. n_in - 1:
 *     j = t + bounded(next word, P - t), swap perm[t] and perm[j], idx[k, t] = window[perm[t]];
 *   outside: p = bounded(next word, H W) repeatedly, accepted when it is neither a window position
 *     nor already accepted; idx[k, n_in + a] = the a-th accepted p.  After 64 n_out draws the
 *     remaining slots take the lowest free positions in ascending order (the limits keep the
 *     acceptance above 1/2, so this is unreachable in practice; it bounds the loop);
 *   loc[k] = centre.
 * Limits (POSU_ERR_ARG before any launch): non-null joints, vis, idx; joint_idx in [0, J);
 * radius >= 1; P <= 1024; H W <= 65536; P + P / 4 <= H W / 2; feat_w, feat_h finite and positive.
 * B == 0 succeeds without a launch.  `call` is a by-value argument: a captured graph would replay
 * one draw. */
int posu_heatmap_mi_sample(const double* joints, const double* vis, int B, int J, int joint_idx, double feat_w,
                           double feat_h, int H, int W, int radius, unsigned long long seed,
                           unsigned long long call, int* idx, int* loc, void* stream);

/* ------------------------------------------------- training-loop metrics */
/* What lib/core/function.py:91-527 (train) computes about a step besides the losses, without a
 * read-back.  Additive to ABI 16.  Stream-ordered, no allocation, no atomics, f64 partials in a
 * fixed order: two calls on the same inputs give the same bits.
 *
 * PCK accuracy of V (1..8) views (accuracy, lib/core/evaluate.py:42-73, with calc_dists / dist_acc
 * :17-39 over get_max_preds, lib/core/inference.py:19-47; called per view on host copies at
 * function.py:463-466).  outputs / targets: HOST arrays of V device pointers to [N, J, H, W] f32
 * (any 4-byte alignment; 16-byte aligned maps are read with 16-byte loads).  Per map pair the
 * argmaxes are posu_argmax2d_fwd's at post_process = 0 (first maximum, (0, 0) when maxval <= 0);
 * then in f64 valid = tx > 1 && ty > 1, d = sqrt((px / (H/10) - tx / (H/10))^2 + (py / (W/10) -
 * ty / (W/10))^2) -- x over H and y over W is the reference's pairing -- and hit = valid && d < thr.
 *   acc  [V, J + 1] f64: acc[j + 1] = hits / valid over n, -1 without a valid target; acc[0] = avg;
 *   avg  [V] f64: the accuracies >= 0 added joint by joint in index order / cnt (0 when cnt == 0);
 *   cnt  [V] int32: joints with a valid target;
 *   pred [V, N, J, 2] f32: the outputs' argmax coordinates;
 *   step [2] f64: the means over the views of avg and of cnt, added as np.mean adds them
 *        (function.py:467-468);
 *   workspace >= posu_pck_accuracy_workspace(V, N, J) bytes (-1: V outside 1..8, a non-positive
 *        size, or 2^31 map pairs and more). */
long long posu_pck_accuracy_workspace(int V, int N, int J);
int posu_pck_accuracy(const float* const* outputs, const float* const* targets, int V, int N, int J, int H,
                      int W, double thr, double* acc, double* avg, int* cnt, float* pred, double* step,
                      void* workspace, long long workspace_bytes, void* stream);

/* The gradient-norm watch (check_grad_norm, lib/utils/gradients.py:31-39; function.py:352-362).
 * grads: HOST array of V (1..8) device pointers to [N, L] f32, NULL = a view without a gradient
 * (skipped).  Per row the p-norm (p = 1 or 2) accumulated in f64;
 *   out[0] = sum over the views of (sum of row norms / number of rows whose norm != 0), f64
 * (a view whose rows are all zero adds 0 / 0 = NaN, as the reference's does; 0 when every pointer
 * is NULL).  workspace >= posu_grad_row_norms_workspace(V, N) bytes, 8-byte aligned. */
long long posu_grad_row_norms_workspace(int V, int N);
int posu_grad_row_norms(const float* const* grads, int V, int N, long long L, int p, double* out,
                        void* workspace, long long workspace_bytes, void* stream);

/* AverageMeter.update (function.py:693-709) for every meter of the loop in one launch.
 * table [M, 3] f64 device (val, sum, count), M <= 64; v, w [M] f64 device; active [M] u8 HOST mask,
 * read during the call (it becomes a launch argument, so a captured launch keeps it).  Per active
 * slot m: val = v[m]; sum += v[m] * w[m]; count += w[m], each operation rounded on its own like
 * the host's float arithmetic; avg = sum / count is left to the reader. */
int posu_meters_update(double* table, int M, const double* v, const double* w, const unsigned char* active,
                       void* stream);

/* ------------------------------------------------- 3-D evaluation protocol */
/* run/pose3d/estimate.py's arithmetic in fp64 (csrc/pose3d.hip), additive to ABI 16.  One wave per
 * pose, lanes stride over the joints (any J >= 1); every pointer is a device pointer.
 *
 * PoseUtils.procrustes (lib/utils/pose_utils.py:61-143) for N pose pairs: B is moved onto the
 * target A.  In the reference's order: subtract the means, ssX / ssY and the norms, divide by them,
 * M = A0^T B0, SVD (one-sided Jacobi, at most 30 sweeps), R = V U^T, S_trace = sum s; with scaling
 * scale = S_trace * normA / normB, d = 1 - S_trace^2, Z = normA * S_trace * B0 R + meanA, without it
 * scale = 1, d = 1 + ssY / ssX - 2 S_trace normB / normA, Z = normB * B0 R + meanA;
 * t = meanA - scale * meanB R, so Z = scale * B R + t.
 *   A, B:  [N, J, 3] f64;
 *   scaling: 0 / 1;
 *   reflection: 0 = 'best' (R as it comes), 1 = force a reflection (det R < 0), 2 = forbid one; the
 *          forced fix negates the column of V and the singular value that belong to the smallest
 *          singular value, then R = V U^T again (pose_utils.py:111-119);
 *   d [N], Z [N, J, 3], R [N, 3, 3], scale [N], t [N, 3] f64: each may be NULL, not all of them.
 * A pose whose joints all coincide (ssX or ssY = 0) gives NaN, as the reference's 0 / 0 does.  With
 * coplanar joints (M of rank 2) U is completed by a cross product where LAPACK picks a sign: the
 * sign reaches Z only when the target alone is planar, as it does in the reference; collinear joints
 * (rank 1) have no defined result. */
int posu_procrustes(const double* A, const double* B, int N, int J, int scaling, int reflection, double* d,
                    double* Z, double* R, double* scale, double* t, void* stream);

/* error_computing_3d (estimate.py:110-123) for G groups x V cameras: per (group, camera)
 * pred = (R (X^T - T))^T; with procrustes != 0, pred <- Z of procrustes(gt, pred) (scaling on,
 * reflection 'best'); err[g][v][j] = || gt - pred ||.
 *   X:   [G, J, 3] f64, world frame;
 *   gt:  [G, V, J, 3] f64, every camera's frame;
 *   R:   [G, V, 3, 3] f64;  T: [G, V, 3] f64 (the camera centre, world frame);
 *   err: [G, V, J] f64;  aligned: NULL or [G, V, J, 3] f64, receives pred. */
int posu_pose3d_errors(const double* X, const double* gt, const double* R, const double* T, int G, int V,
                       int J, int procrustes, double* err, double* aligned, void* stream);

/* break_limb_length (estimate.py:84-96) for G poses: flag[g] = 1 iff some edge (parent[c], c) has
 * | limb[c] - || X_p - X_c || | > thres * limb[c] (strict; a NaN never flags, as in numpy), else 0.
 *   X:      [G, J, 3] f64;
 *   parent: [J] int32, -1 at the root (an entry outside [0, J) is no edge);
 *   limb:   expected lengths by child joint: [G, J] with limb_stride = J, or one shared [J] with
 *           limb_stride = 0;
 *   flag:   [G] uint8;  worst: NULL or [G] f64, the largest offset / limb over the edges (NaN
 *           ratios are passed over; 0 without edges). */
int posu_limb_break(const double* X, const int* parent, const double* limb, int limb_stride, int G, int J,
                    double thres, unsigned char* flag, double* worst, void* stream);

/* ------------------------------------------------------ pseudo-label round */
/* The loop of run/test/test_pseudo_label.py:193-259 for a sweep of T (1..8) confidence thresholds in
 * one launch, one thread per (group, joint).  The pair triangulations of ransac (triangulate.py:142-155)
 * and their reprojection errors do not depend on the confidence threshold: they are solved once and
 * every threshold reuses them.  Per threshold t:
 *   stage 0  conf > thre[t], compared in f32 as numpy compares an f32 array with a Python float
 *            (test_pseudo_label.py:194);
 *   stage 1  ransac (triangulate.py:102-165) on the stage-0 mask: posu_ransac_inliers' result;
 *   stage 2  reproject_poses (triangulate.py:169-213) on the stage-1 mask when use_ransac is set, on
 *            the stage-0 mask otherwise: posu_reproject's result.  The n-view solve is repeated only
 *            when the mask differs from the one last solved.
 *   M: [G, V, 3, 4] f64;  intr: [G, V, 9] f64;  xy: [G, V, J, 2] f64;  conf: [G, V, J] f32;
 *   thre: HOST array of T floats;  2 <= V <= 4;  min_inliers >= 1;
 *   vis_out:  [T, 3, G, V, J] uint8, the three stages' masks;
 *   proj_out: [T, G, V, J, 2] f64, stage 2's projections (zeros where fewer than 2 views were on).
 * G == 0 returns POSU_OK without a launch.
 *
 * posu_pseudo_label_workspace answers on the host: the bytes of one round's device results laid out as
 * proj_out, then the posu_pckh_counts table of the T * 3 sets ([T * 3, 2J + V + 1] int32, padded to a
 * multiple of 8 bytes), then vis_out -- one allocation, one read-back.  -1 outside 1 <= T <= 8,
 * 2 <= V <= 4, J > 0, G >= 0. */
long long posu_pseudo_label_workspace(int T, int G, int V, int J);
int posu_pseudo_label_sweep(const double* M, const double* intr, const double* xy, const float* conf,
                            const float* thre, int T, int G, int V, int J, int undistort,
                            double reproj_thre, int min_inliers, int use_ransac, unsigned char* vis_out,
                            double* proj_out, void* stream);

/* The reductions behind my_eval (test_pseudo_label.py:89-105), np.sum(joints_vis) (:196) and the
 * Joints@k lines (:197-205) for B (1..32) label sets of N = G * V frames (group-major) at once.
 *   vis:  [B, N, J] uint8;  gt: NULL or [N, J, 2] f64;  head: [N] f64 (the frames' head sizes);
 *   pred: [N, J, 2] f64, the predictions shared by the sets;  pred_sets: NULL or [S, N, J, 2] f64;
 *   set_pred: NULL (every set reads pred) or a HOST array of B ints: set b reads pred when
 *             set_pred[b] < 0 and pred_sets[set_pred[b]] otherwise;
 *   counts: [B, 2J + V + 1] int32, zeroed here on the stream: [j] frames with joint j visible and
 *           sqrt((gt - pred)^2 summed over x, y) / head <= threshold (f64, :96-98), [J + j] frames with
 *           joint j visible, [2J + k] the (group, joint)s visible in exactly k of the V (1..8) views.
 * gt == NULL leaves the detection counts zero (loop training without ground truth).  Integer
 * atomics: the result does not depend on the order.  N == 0 zeroes counts and launches nothing. */
int posu_pckh_counts(const double* pred, const double* pred_sets, const int* set_pred,
                     const unsigned char* vis, const double* gt, const double* head, int B, int N, int J,
                     int V, double threshold, int* counts, void* stream);

/* ---------------------------------------------------- fundamental matrices */
/* The table FundamentalLoss reads, estimated from 2-D correspondences (the reference makes it with
 * cv2.findFundamentalMat(pts_i, pts_j, cv2.FM_LMEDS), run/test/generate_fundamental_matirx.py:36-103): a
 * least-median-of-squares estimator over the normalised 8-point algorithm for P independent problems
 * (one per subject and view pair) in one call (csrc/fundamental.hip).  Additive to ABI 16.  fp64,
 * stream-ordered, no allocation, no host read; the same inputs and seed give the same bits.
 *   pts:   [P, N, 4] f64, (x_i, y_i, x_j, y_j) in pixels;  valid: NULL (every row) or [P, N] uint8;
 *   H hypotheses per problem;  n = the problem's valid rows.
 * Hypothesis h of problem p:
 *   sample  8 distinct valid rows.  The words are those of the Philox4x32-10 blocks (see
 *           posu_heatmap_mi_sample) with key (seed low, seed high) and counter (b, h, p, 0), b = 0, 1, ...,
 *           consumed in output order; a word gives the candidate row (word * N) >> 32, rejected when the
 *           row is invalid or already taken.  The 64th rejection ends the hypothesis: it is unusable and
 *           its median is +inf.  The 8 rows are then sorted ascending, so that two hypotheses with the
 *           same rows are the same hypothesis bit for bit.
 *   solve   Hartley normalisation of each image's 8 points (centroid to the origin, mean distance
 *           sqrt 2); the 8 x 9 system with rows [xj xi, xj yi, xj, yj xi, yj yi, yj, xi, yi, 1], i.e.
 *           x_j^T F x_i = 0; the right singular vector of the smallest singular value by one-sided Jacobi;
 *           rank 2 by a 3 x 3 Jacobi SVD with the smallest singular value set to zero; F = T_j^T F^ T_i.
 *   score   a valid row's error is max(d_i^2, d_j^2), the squared distances of x_i to the line F^T x_j
 *           and of x_j to the line F x_i; a NaN counts as +inf.  The hypothesis's median is the exact
 *           element of rank n / 2 (0-based, integer division) of these errors.  N has no cap.
 * Per problem: the winner is the smallest median (ties to the lowest h);
 *   sigma = 2.5 * 1.4826 * (1 + 5 / (n - 8)) * sqrt(median), the 5 / (n - 8) taken as 0 for n = 8,
 *   floored at 1e-3 px; the inliers are the valid rows with error <= sigma^2; with refit != 0 the
 *   normalised 8-point solve is repeated over all inliers on the 9 x 9 Gram matrix of their rows, else
 *   the winner itself is kept; the result is scaled to F[2][2] = 1, or to Frobenius norm 1 when
 *   |F[2][2]| <= 1e-7 max|F|.  A problem with n < 8, without a usable hypothesis, with fewer than 8
 *   inliers or with a non-finite result writes a zero matrix, a zero mask and n_inliers = 0.
 *   F: [P, 3, 3] f64;  mask: [P, N] uint8;  sample: [P, 8] int32, the winner's rows (-1 without one);
 *   stats: [P, 4] f64: the winning median (+inf without a winner), sigma, n_inliers, the winning h (-1);
 *   workspace: DEVICE, 8-byte aligned, at least posu_fundamental_workspace(P, N, H) bytes, which answers
 *   on the host (-1 outside 1 <= P <= 65535, 8 <= N <= 2^26, 1 <= H <= 2^20).
 * POSU_ERR_ARG before any launch: a null pointer (valid excepted), P < 1, N < 8, H < 1, a workspace that
 * is too small. */
long long posu_fundamental_workspace(int P, int N, int H);
int posu_fundamental_lmeds(const double* pts, const unsigned char* valid, int P, int N, int H,
                           unsigned long long seed, int refit, double* F, unsigned char* mask, int* sample,
                           double* stats, void* workspace, long long workspace_bytes, void* stream);
/* The check the generator prints (:54-63): per problem the mean and the max over the valid rows of
 * |x_j^T F x_i|.  F: [P, 3, 3] f64; pts, valid as above (N >= 1); out: [P, 2] f64 (mean, max; zeros
 * without a valid row). */
int posu_epipolar_residual_stats(const double* F, const double* pts, const unsigned char* valid, int P, int N,
                                 double* out, void* stream);

/* ------------------------------------------------------- validation epoch */
/* The batch body of validate (lib/core/function.py:529-690) after the forwards, for all V (1..8) views
 * in one launch (csrc/validate.hip), additive to ABI 16.  One wave per map (v, n, j).  Stream-ordered,
 * no allocation, no synchronisation, no atomics.
 *   outputs:  HOST array of V device pointers to the plain outputs [N, J, H, W] f32 (any 4-byte
 *             alignment; rows of whole float4s in 16-byte aligned maps are moved with 16-byte accesses);
 *   flipped:  NULL, or a HOST array of V device pointers to the outputs of the mirrored input, raw
 *             (function.py:570-576).  The merged map is the reference's flip_back_th
 *             (lib/utils/transforms.py:33-47), SHIFT_HEATMAP (function.py:579-582) and average (:583)
 *             in posu_flip_back's expression: m = 0.5f * (o + F), F = flipped[n][perm[j]][y][W - 1 - xs],
 *             xs = shift ? max(x - 1, 0) : x.  Without flipped, m = o;
 *   perm:     NULL (identity) or [J] int32 DEVICE: the joint each joint swaps with (an entry outside
 *             [0, J) reads the joint itself);
 *   targets:  NULL, or a HOST array of V device pointers to the target heatmaps: then accuracy
 *             (lib/core/evaluate.py:42-73, called per view at function.py:618-624) of the merged maps in
 *             posu_pck_accuracy's arithmetic and layout: acc [V, J + 1] f64, avg [V] f64, cnt [V] int32,
 *             step [2] f64, with workspace >= posu_decode_views_workspace(V, N, J) bytes, 4-byte aligned
 *             (-1: V outside 1..8, N < 0, J < 1, or 2^31 maps and more).  Without targets these five may
 *             be NULL and are not written;
 *   affine64: NULL or [V * N, 2, 3] f64, view-major: the inverse crop affines of get_final_preds
 *             (lib/core/inference.py:50-75);
 *   decode:   posu_argmax2d_fwd's: the first maximum of m, coordinates zeroed when it is <= 0, with
 *             post_process the +-0.25 px shift toward the larger neighbour when 1 < ix < W - 1 and
 *             1 < iy < H - 1 (neighbours recomputed from the inputs), the f64 affine, the f32 store;
 *   preds_out:  [rows, J, 3] f32, (x, y, maxval);  merged_out: NULL or [rows, J, H, W] f32, receives m.
 *             Both are addressed by row = row0 + n * V + v, the reference's preds[k::nviews] order
 *             (function.py:632-644): the pointers are the bases of the epoch's buffers, and
 *             0 <= row0, row0 + V * N <= rows is required.  Rows outside that range are not touched.
 * N == 0 returns POSU_OK without a launch. */
long long posu_decode_views_workspace(int V, int N, int J);
int posu_decode_views(const float* const* outputs, const float* const* flipped, const int* perm, int shift,
                      const float* const* targets, const double* affine64, int V, int N, int J, int H, int W,
                      int post_process, double thr, float* merged_out, float* preds_out, long long row0,
                      long long rows, double* acc, double* avg, int* cnt, double* step, void* workspace,
                      long long workspace_bytes, void* stream);

/* The counts behind the evaluations validate ends with (function.py:678), for T (1..8) thresholds at once.
 *   pred: [N, J, pred_stride] f32, pred_stride 2 or 3: x and y are read and widened to f64;
 *   gt:   [N, J, 2] f64;  head: [N] f64;  vis: NULL (every joint counts) or [N, J] uint8;
 *   thresholds: HOST array of T doubles;
 *   d = sqrt(dx * dx + dy * dy) in f64, each operation rounded on its own, and a row is detected when
 *     form 0: d <= head * thr   (MultiViewH36MCompatible.evaluate, lib/dataset/multiview_h36m_compatible.py:205-208)
 *     form 1: d / head <= thr   (MPIIDatasetCompatible.evaluate, lib/dataset/mpii_compatible.py:173-175);
 *   counts: [T, 2, J] int32, zeroed here on the stream: [t][0][j] rows with joint j visible and detected
 *           at thresholds[t], [t][1][j] rows with joint j visible.
 * Integer atomics: the result does not depend on the order.  N == 0 zeroes counts and launches nothing. */
int posu_detection_counts(const float* pred, int pred_stride, const double* gt, const double* head,
                          const unsigned char* vis, const double* thresholds, int T, int form, int N, int J,
                          int* counts, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* POSU_H_ */
