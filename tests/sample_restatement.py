"""CPU restatement (test infrastructure only) of the training sample of
JointsDatasetCompatible.__getitem__ (reference lib/dataset/joints_dataset_compatible.py:111-201):

  flip             data_numpy[:, ::-1, :] before the warp (:156)
  warp             cv2.warpAffine as oracle.geometry_ref.warp_affine_linear restates it (:162-165)
  colour jitter    torchvision ColorJitter on a PIL image (:67-71, :168-172): PIL's ImageEnhance blends
                   and mode conversions (Blend.c, Convert.c) written out in numpy
  ToTensor + Normalize   oracle.geometry_ref.to_tensor_normalize (:173)
  joints           fliplr_joints (lib/utils/transforms.py:50-64), affine_transform (:112-120) for the
                   visible joints (:175-177), generate_heatmap (:207-253)

The PIL pieces are pinned against the installed PIL by tests/test_sample_host.py (exhaustively), the whole
sample against the reference's own __getitem__ by tests/golden/sample_batch.npz.
"""
from fractions import Fraction

import numpy as np

from oracle import geometry_ref as G

# the ColorJitter operations by torchvision's fn_id
BRIGHTNESS, CONTRAST, SATURATION, HUE = 0, 1, 2, 3

UNION_FLIP_PAIRS = [[0, 5], [1, 4], [2, 3], [10, 15], [11, 14], [12, 13]]


# ---------------------------------------------------------------- PIL point operations
def pil_l(r, g, b):
    """Image.convert('L') of an RGB image (Convert.c, L24 with rounding)."""
    r, g, b = (np.asarray(v).astype(np.int64) for v in (r, g, b))
    return (19595 * r + 38470 * g + 7471 * b + 0x8000) >> 16


def blend(d, x, f):
    """Image.blend(degenerate, image, f) per byte (Blend.c): d + f * (x - d) in f32; truncated for
    0 <= f <= 1, otherwise clipped to [0, 255] and truncated."""
    f = np.float32(f)
    d = np.asarray(d).astype(np.int64)
    x = np.asarray(x).astype(np.int64)
    t = d.astype(np.float32) + f * (x - d).astype(np.float32)
    assert t.dtype == np.float32
    if 0 <= f <= 1:
        return t.astype(np.int64)
    return np.clip(t, np.float32(0), np.float32(255)).astype(np.int64)


def rgb_to_hsv(r, g, b):
    """Image.convert('HSV') of RGB (Convert.c rgb2hsv_row): f32 quotients, the sum with the constant and
    the fmod in double, each rounded to f32."""
    r, g, b = (np.asarray(v).astype(np.int64) for v in (r, g, b))
    maxc = np.maximum(r, np.maximum(g, b))
    minc = np.minimum(r, np.minimum(g, b))
    grey = maxc == minc
    cr = np.where(grey, 1, maxc - minc).astype(np.float32)
    mx = np.where(grey, 1, maxc).astype(np.float32)
    s = cr / mx
    rc = (maxc - r).astype(np.float32) / cr
    gc = (maxc - g).astype(np.float32) / cr
    bc = (maxc - b).astype(np.float32) / cr
    h_r = bc - gc
    h_g = (2.0 + rc.astype(np.float64) - bc.astype(np.float64)).astype(np.float32)
    h_b = (4.0 + gc.astype(np.float64) - rc.astype(np.float64)).astype(np.float32)
    h = np.where(r == maxc, h_r, np.where(g == maxc, h_g, h_b))
    assert h.dtype == np.float32 and s.dtype == np.float32
    h = np.fmod(h.astype(np.float64) / 6.0 + 1.0, 1.0).astype(np.float32)
    H = (h.astype(np.float64) * 255.0).astype(np.int64)
    S = (s.astype(np.float64) * 255.0).astype(np.int64)
    return np.where(grey, 0, H), np.where(grey, 0, S), maxc


def _round_half_away(x):
    """C round() on non-negative doubles."""
    fl = np.floor(x)
    return (fl + (x - fl >= 0.5)).astype(np.int64)


def hsv_to_rgb(h, s, v):
    """Image.convert('RGB') of HSV (Convert.c hsv2rgb): the sector and its remainder from h * 6.0 / 255.0
    in double (the remainder rounded to f32), fs = s / 255.0 rounded to f32, fs * f in f32, the three
    products in double, C round()."""
    h, s, v = (np.asarray(a).astype(np.int64) for a in (h, s, v))
    h6 = h.astype(np.float32).astype(np.float64) * 6.0 / 255.0
    i = np.floor(h6)
    f = (h6 - i.astype(np.float32).astype(np.float64)).astype(np.float32)
    fs = (s.astype(np.float32).astype(np.float64) / 255.0).astype(np.float32)
    vd = v.astype(np.float64)
    fsf = fs * f
    assert fsf.dtype == np.float32
    p = np.clip(_round_half_away(vd * (1.0 - fs.astype(np.float64))), 0, 255)
    q = np.clip(_round_half_away(vd * (1.0 - fsf.astype(np.float64))), 0, 255)
    t = np.clip(_round_half_away(vd * (1.0 - fs.astype(np.float64) * (1.0 - f.astype(np.float64)))), 0, 255)
    k = i.astype(np.int64) % 6
    r = np.choose(k, [v, q, p, p, t, v])
    g = np.choose(k, [t, v, v, q, p, p])
    b = np.choose(k, [p, p, t, v, v, q])
    grey = s == 0
    return np.where(grey, v, r), np.where(grey, v, g), np.where(grey, v, b)


def contrast_grey(l_sum, count):
    """ImageEnhance.Contrast's degenerate grey: int(ImageStat.Stat(L).mean[0] + 0.5)."""
    return int(int(l_sum) / int(count) + 0.5)


def color_jitter(rgb, order, brightness, contrast, saturation, hue_shift):
    """torchvision ColorJitter.forward on a PIL RGB image with the drawn parameters: the four operations in
    `order` (fn_ids).  rgb uint8 [h, w, 3] -> (uint8 [h, w, 3], the integer sum of L that the contrast
    step averaged, or None without a contrast step)."""
    x = np.asarray(rgb).astype(np.int64)
    l_sum = None
    for op in order:
        if op == BRIGHTNESS:
            x = blend(0, x, brightness)
        elif op == CONTRAST:
            l_sum = int(pil_l(x[..., 0], x[..., 1], x[..., 2]).sum())
            x = blend(contrast_grey(l_sum, x.shape[0] * x.shape[1]), x, contrast)
        elif op == SATURATION:
            x = blend(pil_l(x[..., 0], x[..., 1], x[..., 2])[..., None], x, saturation)
        elif op == HUE:
            h, s, v = rgb_to_hsv(x[..., 0], x[..., 1], x[..., 2])
            x = np.stack(hsv_to_rgb((h + int(hue_shift)) % 256, s, v), axis=-1)
    return x.astype(np.uint8), l_sum


def hue_shift_of(hue):
    """adjust_hue's np.uint8(hue_factor * 255): truncation toward zero, then mod 256."""
    return int(np.trunc(hue * 255)) % 256


# ---------------------------------------------------------------- the image half
def sample_image_u8(img, flip, trans, image_size, jitter=None, bgr=True):
    """The uint8 crop before ToTensor: flip, warp, jitter.  jitter: None or a dict with order, brightness,
    contrast, saturation, hue_shift.  Returns (uint8 [h, w, 3] in the source's channel order, L sum)."""
    img = np.asarray(img)
    if flip:
        img = img[:, ::-1, :]
    out = G.warp_affine_linear(np.ascontiguousarray(img), trans, (int(image_size[0]), int(image_size[1])))
    if jitter is None:
        return out, None
    rgb = out[:, :, ::-1] if bgr else out
    jit, l_sum = color_jitter(rgb, jitter['order'], jitter['brightness'], jitter['contrast'], jitter['saturation'],
                              jitter['hue_shift'])
    return np.ascontiguousarray(jit[:, :, ::-1] if bgr else jit), l_sum


# ---------------------------------------------------------------- the label half
def _fma(a, b, c):
    """round(a * b + c) with one rounding."""
    return float(Fraction(float(a)) * Fraction(float(b)) + Fraction(float(c)))


def affine_visible(joints, vis0, trans):
    """joints[visible] = affine_transform(joints[visible], trans) (:175-177).  np.dot hands the
    [K, 3] x [3, 2] product to BLAS, whose kernels fuse one multiply-add: with K >= 2 rows (gemm)
    fma(y, t1, x * t0) + t2, with one row (gemv) fma(x, t0, y * t1) + t2 -- written out here so the
    restatement does not depend on the BLAS it runs with."""
    joints = np.array(joints, dtype=np.float64)
    rows = np.flatnonzero(np.asarray(vis0) > 0)
    for j in rows:
        x, y = joints[j]
        for c in range(2):
            t0, t1, t2 = (float(v) for v in trans[c])
            acc = _fma(y, t1, x * t0) if len(rows) >= 2 else _fma(x, t0, y * t1)
            joints[j, c] = acc + t2
    return joints


def fliplr_joints(joints, joints_vis, width, matched_parts):
    joints = np.array(joints, dtype=np.float64)
    joints_vis = np.array(joints_vis, dtype=np.float64)
    joints[:, 0] = width - joints[:, 0] - 1
    perm = list(range(len(joints)))
    for a, b in matched_parts:
        perm[a], perm[b] = b, a
    joints, joints_vis = joints[perm], joints_vis[perm]
    return joints * joints_vis, joints_vis


def _f32(fr):
    """The float32 nearest a Fraction, ties to even."""
    d = float(fr)                                   # correctly rounded to double
    r = np.float32(d)
    if Fraction(d) != fr:                           # rounded twice: repair a double that sits on an f32 tie
        for a, b in ((np.nextafter(r, np.float32(-np.inf)), r), (r, np.nextafter(r, np.float32(np.inf)))):
            mid = (Fraction(float(a)) + Fraction(float(b))) / 2
            if Fraction(d) == mid:
                r = b if fr > mid else a
    return r


def _fmaf(a, b, c):
    return _f32(Fraction(float(a)) * Fraction(float(b)) + Fraction(float(c)))


_EXP_P = [np.float32(v) for v in (9.999999999980870924916e-01, 7.257664613233124478488e-01,
                                  2.473615434895520810817e-01, 5.114512081637298353406e-02,
                                  6.757896990527504603057e-03, 5.082762527590693718096e-04)]
_EXP_Q = [np.float32(v) for v in (1.0, -2.742335390411667452936e-01, 2.159509375685829852307e-02)]


def numpy_exp_f32(x):
    """np.exp of one float32 as numpy's AVX2 / AVX512F kernels compute it (simd_exp_FLOAT: faithful, not
    correctly rounded), written out with exact fused multiply-adds so that the restatement gives the same
    bits on any host.  For arguments in [-9, 0]."""
    x = np.float32(x)
    magic = np.float32(12582912.0)
    q = np.float32(x * np.float32(1.44269504088896341))
    q = np.float32(np.float32(q + magic) - magic)
    r = _fmaf(q, np.float32(-6.93145752e-1), x)
    r = _fmaf(q, np.float32(-1.42860677e-6), r)
    num = _fmaf(_EXP_P[5], r, _EXP_P[4])
    for k in (3, 2, 1, 0):
        num = _fmaf(num, r, _EXP_P[k])
    den = _fmaf(_fmaf(_EXP_Q[2], r, _EXP_Q[1]), r, _EXP_Q[0])
    return np.float32(np.ldexp(np.float32(num / den), int(q)))


def generate_heatmap(joints, joints_vis, image_size, heatmap_size, sigma, zero_weight):
    """generate_heatmap (:207-253): mu in f64, the Gaussian in f32 through numpy's float32 exp."""
    nj = len(joints)
    hw, hh = int(heatmap_size[0]), int(heatmap_size[1])
    target = np.zeros((nj, hh, hw), dtype=np.float32)
    weight = np.asarray(joints_vis)[:, :1].astype(np.float32)
    tmp = sigma * 3
    stride = np.asarray(image_size, dtype=np.float64) / np.asarray(heatmap_size, dtype=np.float64)
    size = 2 * tmp + 1
    ax = np.arange(0, size, 1, np.float32)
    arg = -((ax - size // 2) ** 2 + (ax[:, None] - size // 2) ** 2) / (2 * sigma ** 2)
    assert arg.dtype == np.float32
    table = {a: numpy_exp_f32(a) for a in np.unique(arg).tolist()}
    g = np.array([[table[a] for a in row] for row in arg.tolist()], dtype=np.float32)
    for j in range(nj):
        mu_x = int(joints[j][0] / stride[0] + 0.5)
        mu_y = int(joints[j][1] / stride[1] + 0.5)
        ul = [int(mu_x - tmp), int(mu_y - tmp)]
        br = [int(mu_x + tmp + 1), int(mu_y + tmp + 1)]
        if ul[0] >= hw or ul[1] >= hh or br[0] < 0 or br[1] < 0:
            weight[j] = 0
            continue
        if weight[j] > 0.5:
            gx = max(0, -ul[0]), min(br[0], hw) - ul[0]
            gy = max(0, -ul[1]), min(br[1], hh) - ul[1]
            ix = max(0, ul[0]), min(br[0], hw)
            iy = max(0, ul[1]), min(br[1], hh)
            target[j][iy[0]:iy[1], ix[0]:ix[1]] = g[gy[0]:gy[1], gx[0]:gx[1]]
    if zero_weight:
        weight = np.zeros((nj, 1), dtype=np.float32)
    return target, weight


def sample_joints_targets(joints, joints_vis, flip, width, flip_pairs, trans, zero_weight, image_size, heatmap_size,
                          sigma):
    """One record's label half -> (joints_2d_transformed [J, 2] f64, joints_vis [J, 2] f64, target, weight)."""
    joints = np.array(joints, dtype=np.float64)
    vis = np.array(joints_vis, dtype=np.float64)[:, :2]
    if flip:
        joints, vis = fliplr_joints(joints, vis, width, flip_pairs)
    joints = affine_visible(joints, vis[:, 0], trans)
    target, weight = generate_heatmap(joints, vis, image_size, heatmap_size, sigma, zero_weight)
    return joints, vis, target, weight


def sample(img, joints, joints_vis, flip, trans, image_size, heatmap_size, sigma, zero_weight, jitter, mean, std,
           flip_pairs=UNION_FLIP_PAIRS):
    """The whole sample: (input f32 [3, h, w], target, weight, joints_2d_transformed, joints_vis)."""
    u8, _ = sample_image_u8(img, flip, trans, image_size, jitter)
    j, v, t, w = sample_joints_targets(joints, joints_vis, flip, np.asarray(img).shape[1], flip_pairs, trans,
                                       zero_weight, image_size, heatmap_size, sigma)
    return G.to_tensor_normalize(u8, mean, std), t, w, j, v


# ---------------------------------------------------------------- the golden's records (sample_batch.npz)
MEAN, STD = (0.485, 0.456, 0.406), (0.229, 0.224, 0.225)
AUG_PARAMS = {'mpii': {'scale_factor': 0.25, 'rotation_factor': 30, 'flip': True},
              'h36m': {'scale_factor': 0.25, 'rotation_factor': 30, 'flip': False}}
MV = {'image_size': (64, 64), 'heatmap_size': (16, 16), 'sigma': 1}
LAB = {'image_size': (96, 128), 'heatmap_size': (24, 32), 'sigma': 1}
META_KEYS = ('scale', 'center', 'rotation', 'joints_2d', 'joints_2d_transformed', 'joints_vis', 'source', 'subject')


def golden_records(g, prefix):
    """The db records of a golden section, as the reference's dataset holds them."""
    n = len(g[prefix + '.db_source'])
    return [{'center': g[prefix + '.db_center'][k], 'scale': g[prefix + '.db_scale'][k],
             'joints_2d': g[prefix + '.db_joints_2d'][k], 'joints_vis': g[prefix + '.db_joints_vis'][k],
             'source': str(g[prefix + '.db_source'][k]), 'subject': int(g[prefix + '.db_subject'][k])}
            for k in range(n)]


def golden_rotation(g, prefix):
    """The recorded rotations as __getitem__ left them: the int 0 where none was drawn."""
    return [float(r) if r != 0 else 0 for r in g[prefix + '.rotation']]


def golden_jitter(g):
    """The 'mv' section's scripted ColorJitter draws as restatement dicts."""
    return [{'order': [int(v) for v in o], 'brightness': float(f[0]), 'contrast': float(f[1]),
             'saturation': float(f[2]), 'hue_shift': hue_shift_of(float(h))}
            for o, f, h in zip(g['mv.jitter_order'], g['mv.jitter_factors'], g['mv.jitter_hue'])]


def golden_trans(g, prefix, k, width, image_size):
    """Record k's crop affine as __getitem__ builds it: the mirrored centre, the drawn scale and rotation."""
    from utils.transforms import get_affine_transform
    center = np.array(g[prefix + '.db_center'][k], dtype=np.float64)
    scale = np.array(g[prefix + '.db_scale'][k], dtype=np.float64) * g[prefix + '.scale_factor'][k]
    if g[prefix + '.flip'][k]:
        center[0] = width - center[0] - 1
    return center, scale, get_affine_transform(center, scale, golden_rotation(g, prefix)[k], list(image_size))
