"""Recursive pictorial structure model (reference lib/multiviews/pictorial.py) on the HIP
fp64 RPSM kernels (libposeu.so posu_rpsm_*, csrc/rpsm.hip).

The reference walks a 3-D bin grid per 4-view group in numpy: a scipy interpolator per
(view, joint) for the unary term, a dense [N, N] multiply + argmax per limb for the
max-product, and a Python double loop for the recursion's limb-length constraint.  Here the
same names and signatures run on the GPU -- ``rpsm`` / ``rpsm_batch`` enqueue the whole
recursion of every group in one call (posu_rpsm_run) and only the pose comes back -- and the
pieces (``compute_unary_term``, ``infer``, ``compute_pairwise_constrain``,
``recursive_infer``) call the single kernels.  ``compute_grid`` and
``get_loc_from_cube_idx`` are host numpy (tiny).  There is no CPU path: without a visible
device every GPU function raises RuntimeError.

The level-1 pairwise constraint is the reference's dict keyed (parent, child) of dense arrays
or scipy sparse matrices, or a ``PackedPairwise`` (bit-packed once, uploaded once, reused
across calls): ``pack_pairwise(dict)`` or, built on the GPU,
``compute_pairwise_constraint(box_size, limb_length, nbins)``.
"""
import numpy as np
import torch

from posu import ops
from multiviews.body import HumanBody
from multiviews.cameras import unfold_camera_param
from utils.transforms import get_affine_transform

try:
    import scipy.sparse as _sparse
except ImportError:  # dense constraints only
    _sparse = None


def _device(device=None):
    if not torch.cuda.is_available():
        raise RuntimeError('pose-unsupervised_amd runs the pictorial structure model on the GPU; '
                           'no cuda device is visible')
    return device or torch.device('cuda', torch.cuda.current_device())


def _tree(body):
    return ops.RpsmTree(body.parents(), body.children())


def _skeleton_tree(skeleton):
    parents = np.full(len(skeleton), -1, dtype=np.int32)
    for node in skeleton:
        for c in node['children']:
            parents[c] = node['idx']
    return ops.RpsmTree(parents, [list(node['children']) for node in skeleton])


def _dev_f64(a, dev):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float64)).to(dev)


# ---------------------------------------------------------------- host pieces
def compute_grid(boxSize, boxCenter, nBins):
    """[nBins^3, 3] grid of bin centres (pictorial.py:108-119): every axis is
    linspace(-boxSize/2, boxSize/2, nBins) + centre, flat bin (a*n + bx)*n + c at
    (x[bx], y[a], z[c]) -- numpy's 'xy' meshgrid order."""
    g1 = np.linspace(-boxSize / 2, boxSize / 2, nBins)
    x, y, z = g1 + boxCenter[0], g1 + boxCenter[1], g1 + boxCenter[2]
    grid = np.empty((nBins, nBins, nBins, 3))
    grid[..., 0] = x[None, :, None]
    grid[..., 1] = y[:, None, None]
    grid[..., 2] = z[None, None, :]
    return grid.reshape(-1, 3)


def get_loc_from_cube_idx(grid, pose3d_as_cube_idx):
    """[(joint, bin)] -> [J, 3] grid coordinates; one shared grid or one per joint."""
    pose3d = np.zeros((len(pose3d_as_cube_idx), 3))
    for joint_idx, cube_idx in pose3d_as_cube_idx:
        pose3d[joint_idx] = grid[0 if len(grid) == 1 else joint_idx][cube_idx]
    return pose3d


# ------------------------------------------------------- packed pairwise term
class PackedPairwise:
    """The level-1 constraint of every edge as bits: ``bits`` uint32 [E, ceil(N/32), N], bit j & 31
    of word [e][j / 32][i] allows child bin j under parent bin i (numpy.packbits of row i, little
    bit order; the word index outside the parent bin, the layout the kernel reads coalesced);
    edge e = ``edges[e]`` = (parent, child)."""

    def __init__(self, edges, nbins_total, bits=None, device_mask=None):
        self.edges = list(edges)
        self.N = int(nbins_total)
        self._bits = bits
        self._dev = {}
        if device_mask is not None:
            self._dev[device_mask.device] = device_mask

    @property
    def bits(self):
        if self._bits is None:
            m = next(iter(self._dev.values()))
            self._bits = m.cpu().numpy().view(np.uint32)
        return self._bits

    def mask(self, device):
        """int32 device tensor [E, ceil(N/32), N], uploaded on first use."""
        if device not in self._dev:
            self._dev[device] = torch.from_numpy(self.bits.view(np.int32)).to(device)
        return self._dev[device]

    def dense(self):
        """dict (parent, child) -> uint8 [N, N]."""
        rows = np.ascontiguousarray(np.transpose(self.bits, (0, 2, 1)))       # [E, N, words]
        b = np.unpackbits(rows.view(np.uint8), axis=-1, bitorder='little')
        return {e: b[i, :, :self.N] for i, e in enumerate(self.edges)}


def pack_pairwise(pairwise, body=None):
    """dict (parent, child) -> dense [N, N] array or scipy sparse matrix  =>  PackedPairwise
    (rows in the body's edge order).  Any non-zero entry allows the pair."""
    edges = (body or HumanBody()).edges()
    rows, n = [], None
    for e in edges:
        m = pairwise[e]
        if _sparse is not None and _sparse.issparse(m):
            m = m.toarray()
        m = np.asarray(m)
        if m.ndim != 2 or m.shape[0] != m.shape[1] or (n is not None and m.shape[0] != n):
            raise ValueError('pairwise constraint %r must be [N, N] with one N for all edges, got %s'
                             % (e, m.shape))
        n = m.shape[0]
        words = (n + 31) // 32
        by = np.zeros((n, words * 4), dtype=np.uint8)
        by[:, :(n + 7) // 8] = np.packbits(m != 0, axis=1, bitorder='little')
        rows.append(by.view('<u4').T)
    if n > ops.RPSM_MAX_BINS:
        raise ValueError('N = %d bins: the RPSM kernels take at most %d' % (n, ops.RPSM_MAX_BINS))
    return PackedPairwise(edges, n, bits=np.ascontiguousarray(np.stack(rows), dtype=np.uint32))


def compute_pairwise_constraint(box_size, limb_length, nbins, rel=0.4, body=None, device=None):
    """run/test/generate_pairwise_constraints.py:60-95 on the GPU: on the centred nbins^3 grid of
    a box_size box, pair (i, j) of edge (p, c) is allowed when
    | norm(xyz[i] - xyz[j]) - limb_length[(p, c)] | < rel * limb_length[(p, c)]  ->  PackedPairwise."""
    dev = _device(device)
    body = body or HumanBody()
    tree = _tree(body)
    limb = tree.by_child(limb_length)
    grid = ops.rpsm_grid(torch.zeros((1, 3), dtype=torch.float64, device=dev), float(box_size), int(nbins))
    mask = ops.rpsm_pairwise_mask(grid, tree, limb, rel * limb, strict=True)
    return PackedPairwise(body.edges(), int(nbins) ** 3, device_mask=mask)


def _packed(pairwise, body):
    return pairwise if isinstance(pairwise, PackedPairwise) else pack_pairwise(pairwise, body)


# ------------------------------------------------------------------ GPU pieces
def _camera_rows(cams):
    """camera dicts -> [len, 20] f64: R [9], T [3], f = (fx + fy) / 2, cx, cy, k [3], p [2]
    (cameras.unfold_camera_param with avg_f, what project_pose uses)."""
    rows = np.zeros((len(cams), 20))
    for i, cam in enumerate(cams):
        R, T, f, c, k, p = unfold_camera_param(cam)
        rows[i, 0:9] = np.asarray(R, dtype=np.float64).reshape(9)
        rows[i, 9:12] = np.asarray(T, dtype=np.float64).reshape(3)
        rows[i, 12] = np.ravel(np.asarray(f, dtype=np.float64))[0]
        rows[i, 13:15] = np.asarray(c, dtype=np.float64).reshape(2)
        rows[i, 15:18] = np.asarray(k, dtype=np.float64).reshape(3)
        rows[i, 18:20] = np.asarray(p, dtype=np.float64).reshape(2)
    return rows


def _limb_rows(limb_lengths, tree, groups):
    """-> host f64 [G, J] by child joint: a dict or [J] for all groups, or G dicts / [G, J]."""
    if isinstance(limb_lengths, dict):
        return np.tile(tree.by_child(limb_lengths), (groups, 1))
    if isinstance(limb_lengths, (list, tuple)) and len(limb_lengths) and isinstance(limb_lengths[0], dict):
        if len(limb_lengths) != groups:
            raise ValueError('%d limb-length tables for %d groups' % (len(limb_lengths), groups))
        return np.stack([tree.by_child(d) for d in limb_lengths])
    arr = np.asarray(limb_lengths, dtype=np.float64)
    if arr.shape == (tree.njoints,):
        return np.tile(arr, (groups, 1))
    if arr.shape != (groups, tree.njoints):
        raise ValueError('limb_lengths must be a dict, G dicts, [J] or [G, J] by child joint; got shape %s'
                         % (arr.shape,))
    return arr


def _affines(boxes, image_size):
    return np.stack([get_affine_transform(b['center'], b['scale'], 0, image_size) for b in boxes])


def _heatmaps(heatmaps, dev, groups, views):
    if isinstance(heatmaps, torch.Tensor):
        ops.require_cuda(heatmaps)
        hm = heatmaps
    else:
        hm = torch.from_numpy(np.ascontiguousarray(heatmaps, dtype=np.float32)).to(dev)
    if hm.shape[-1] != hm.shape[-2]:
        raise ValueError('RPSM needs square heatmaps (H == W): the reference builds its interpolator axes '
                         'from the swapped sizes; got %d x %d' % (hm.shape[-2], hm.shape[-1]))
    return hm.reshape(groups, views, hm.shape[-3], hm.shape[-2], hm.shape[-1])


def compute_unary_term(heatmap, grid, bbox2D, cam, imgSize):
    """heatmap [n views, k joints, h, w]; grid: list of 1 (shared) or k arrays [nbins, 3];
    bbox2D / cam: n dicts -> list of k arrays [nbins] (pictorial.py:146-190)."""
    dev = heatmap.device if isinstance(heatmap, torch.Tensor) else _device()
    n = heatmap.shape[0]
    hm = _heatmaps(heatmap, dev, 1, n)
    g = _dev_f64(np.stack([np.asarray(x) for x in grid]), dev)[None]
    unary = ops.rpsm_unary(hm, _dev_f64(_camera_rows(cam), dev)[None], _dev_f64(_affines(bbox2D, imgSize), dev)[None],
                           g, imgSize)
    return list(unary[0].cpu().numpy())


def compute_pairwise_constrain(skeleton, limb_length, grid, tolerance):
    """dict (parent, child) -> [nbins, nbins] of 0 / 1: | norm(grid[p][i] - grid[c][j]) - limb | <= tolerance
    (pictorial.py:122-143), from the GPU mask builder."""
    dev = _device()
    tree = _skeleton_tree(skeleton)
    limb = tree.by_child(limb_length)
    g = _dev_f64(np.stack([np.asarray(x) for x in grid]), dev)
    mask = ops.rpsm_pairwise_mask(g, tree, limb, np.full(len(limb), float(tolerance)), strict=False)
    packed = PackedPairwise(tree.edges, g.shape[1], device_mask=mask)
    return {e: m.astype(np.float64) for e, m in packed.dense().items()}


def infer(unary, pairwise, body, config=None):
    """Max-product over the tree (pictorial.py:19-86): unary list of J arrays [nbins], pairwise dict
    (or PackedPairwise) -> sorted [[joint, bin]]."""
    dev = _device()
    u = _dev_f64(np.stack([np.asarray(x, dtype=np.float64).reshape(-1) for x in unary]), dev)[None]
    bins = ops.rpsm_infer(u, _tree(body), mask=_packed(pairwise, body).mask(dev))[0]
    return [[j, int(b)] for j, b in enumerate(bins[0].cpu().numpy())]


def recursive_infer(initpose, cams, heatmaps, boxes, img_size, heatmap_size, body, limb_length, grid_size, nbins,
                    tolerance, config=None):
    """One refinement (pictorial.py:193-211): a grid of nbins^3 bins around every joint of initpose
    [J, 3], unary, limb-length constraint from the grids, inference -> pose [J, 3]."""
    dev = heatmaps.device if isinstance(heatmaps, torch.Tensor) else _device()
    tree = _tree(body)
    hm = _heatmaps(heatmaps, dev, 1, heatmaps.shape[0])
    grids = ops.rpsm_grid(_dev_f64(initpose, dev)[None], float(grid_size), int(nbins))
    unary = ops.rpsm_unary(hm, _dev_f64(_camera_rows(cams), dev)[None], _dev_f64(_affines(boxes, img_size), dev)[None],
                           grids, img_size)
    pose = ops.rpsm_infer(unary, tree, grid=grids, limb=_dev_f64(tree.by_child(limb_length), dev)[None],
                          tolerance=float(tolerance))[1]
    return pose[0].cpu().numpy()


def rpsm_batch(camera_params, heatmaps, boxes, grid_centers, limb_lengths, pairwise_constraint, config,
               return_levels=False):
    """rpsm for G groups in one enqueue.  camera_params / boxes: G*V dicts (group-major, view-minor);
    heatmaps [G*V, J, h, w] (or [G, V, J, h, w]); grid_centers [G, 3]; limb_lengths: one dict keyed
    (parent, child) per group (a list of G, as run/test/test_rpsm.py computes them per group; or an array
    [G, J] by child joint), or a single dict / [J] shared by all groups; pairwise_constraint, shared by the
    groups: the reference's dict or a PackedPairwise -> poses [G, J, 3] float64 (with
    return_levels also [RECUR_DEPTH + 1, G, J, 3]: the pose after level 1 and every refinement).
    A cuda heatmaps tensor is read in place and the result stays on its device; numpy in, numpy out.
    grid_centers given as a cuda tensor are used where they are (no read-back)."""
    on_device = isinstance(heatmaps, torch.Tensor)
    dev = heatmaps.device if on_device else _device()
    if isinstance(grid_centers, torch.Tensor) and grid_centers.is_cuda:   # used in place: no read-back
        cdev = grid_centers.to(device=dev, dtype=torch.float64).reshape(-1, 3).contiguous()
    else:
        cdev = _dev_f64(np.asarray(grid_centers.cpu() if isinstance(grid_centers, torch.Tensor) else grid_centers,
                                   dtype=np.float64).reshape(-1, 3), dev)
    groups = cdev.shape[0]
    if groups == 0 or len(camera_params) % groups or len(boxes) != len(camera_params):
        raise ValueError('%d cameras and %d boxes do not split into %d groups' % (len(camera_params), len(boxes),
                                                                                 groups))
    views = len(camera_params) // groups
    body = HumanBody()
    tree = _tree(body)
    image_size = config.NETWORK.IMAGE_SIZE
    ps = config.PICT_STRUCT
    hm = _heatmaps(heatmaps, dev, groups, views)
    if hm.shape[2] != tree.njoints:
        raise ValueError('heatmaps of %d joints, the body has %d' % (hm.shape[2], tree.njoints))
    packed = _packed(pairwise_constraint, body)
    if packed.N != int(ps.FIRST_NBINS) ** 3:
        raise ValueError('the pairwise constraint has %d bins, FIRST_NBINS^3 = %d' % (packed.N, int(ps.FIRST_NBINS) ** 3))
    limbs = _dev_f64(_limb_rows(limb_lengths, tree, groups), dev)
    rows = _dev_f64(_camera_rows(camera_params), dev).reshape(groups, views, 20)
    aff = _dev_f64(_affines(boxes, image_size), dev).reshape(groups, views, 2, 3)
    step = 65535 // tree.njoints          # groups per enqueue (the launch grid's extent)
    outs = [ops.rpsm_run(hm[a:a + step], rows[a:a + step], aff[a:a + step], image_size, cdev[a:a + step],
                         float(ps.GRID_SIZE), int(ps.FIRST_NBINS), int(ps.RECUR_NBINS), int(ps.RECUR_DEPTH),
                         float(ps.LIMB_LENGTH_TOLERANCE), limbs[a:a + step], packed.mask(dev), tree,
                         return_levels=return_levels) for a in range(0, groups, step)]
    if len(outs) == 1:
        out = outs[0]
    elif return_levels:
        out = (torch.cat([o[0] for o in outs], 0), torch.cat([o[1] for o in outs], 1))
    else:
        out = torch.cat(outs, 0)
    if on_device:
        return out
    return tuple(o.cpu().numpy() for o in out) if return_levels else out.cpu().numpy()


def rpsm(cams, heatmaps, boxes, grid_center, limb_length, pairwise_constraint, config):
    """cams / boxes: one dict per view, heatmaps [views, J, h, w], grid_center [3] -> pose [J, 3]
    (pictorial.py:214-250): rpsm_batch for one group."""
    center = grid_center.cpu().numpy() if isinstance(grid_center, torch.Tensor) else np.asarray(grid_center)
    return rpsm_batch(cams, heatmaps, boxes, center.reshape(1, 3), limb_length, pairwise_constraint, config)[0]
