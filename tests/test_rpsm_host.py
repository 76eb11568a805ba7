"""RPSM, host side: the body tables, the grid, constraint packing and the argument checks of the
posu_rpsm_* entry points.  No kernel is launched here."""
import ctypes
import os
import re

import numpy as np
import pytest

from posu import _native

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RPSM_SYMBOLS = ('posu_rpsm_workspace_bytes', 'posu_rpsm_grid', 'posu_rpsm_unary', 'posu_rpsm_infer',
                'posu_rpsm_backtrack', 'posu_rpsm_pairwise_mask', 'posu_rpsm_run')


def test_rpsm_symbols_are_declared_listed_and_exported():
    src = open(os.path.join(REPO, 'include', 'posu.h')).read()
    src = re.sub(r'/\*.*?\*/', '', src, flags=re.S)
    declared = set(re.findall(r'\b(posu_\w+)\s*\(', src))
    lib = _native.load()
    for name in RPSM_SYMBOLS:
        assert name in declared, name
        assert name in _native.exported_symbols(), name
        assert hasattr(lib, name), name
    assert lib.posu_abi_version() == 16   # additive: the revision does not move


def test_human_body_tables_equal_the_reference(golden):
    from multiviews.body import HumanBody
    g = golden('rpsm_a.npz')
    body = HumanBody()
    assert body.root_idx == int(g['body_root']) == 6
    assert len(body.skeleton) == 16
    for node, kids in zip(body.skeleton, g['body_children']):
        assert node['children'] == [int(c) for c in kids if c >= 0]
        assert set(node) >= {'idx', 'name', 'children'}
    assert [n['idx'] for n in body.skeleton_sorted_by_level] == g['body_level_order'].tolist()
    np.testing.assert_array_equal(body.parents(), g['body_parent'])
    assert body.children() == [n['children'] for n in body.skeleton]
    assert body.edges() == [tuple(e) for e in g['edges'].tolist()]
    for n in body.skeleton:
        if n['idx'] != 6:
            assert body.skeleton[n['parent']]['level'] + 1 == n['level']


@pytest.mark.parametrize('case', ['rpsm_a.npz', 'rpsm_b.npz'])
def test_compute_grid_equals_the_reference_exactly(golden, case):
    from multiviews.pictorial import compute_grid, get_loc_from_cube_idx
    g = golden(case)
    for center, ref in zip(g['grid_center'], g['ref_grid']):
        grid = compute_grid(float(g['grid_size']), center, int(g['first_nbins']))
        assert grid.shape == ref.shape and np.array_equal(grid, ref)
    cube = [[j, int(b)] for j, b in enumerate(g['ref_bins'][0])]
    assert np.array_equal(get_loc_from_cube_idx([g['ref_grid'][0]], cube), g['ref_levels'][0, 0])


@pytest.mark.parametrize('n', [125, 64, 33])
def test_pack_pairwise_round_trips_dense_and_sparse(n):
    from multiviews.body import HumanBody
    from multiviews.pictorial import pack_pairwise
    try:
        import scipy.sparse as sparse
    except ImportError:   # then only dense input is accepted
        sparse = None
    rng = np.random.RandomState(n)
    edges = HumanBody().edges()
    dense = {e: (rng.rand(n, n) < 0.2).astype(np.int8) for e in edges}
    mixed = {e: (sparse.lil_matrix(m) if sparse and i % 2 else m) for i, (e, m) in enumerate(dense.items())}
    for src in (dense, mixed):
        packed = pack_pairwise(src)
        assert packed.N == n and packed.edges == edges
        assert packed.bits.dtype == np.uint32 and packed.bits.shape == (15, (n + 31) // 32, n)
        back = packed.dense()
        for e in edges:
            assert np.array_equal(back[e], dense[e])
        # bit j & 31 of word [edge][j / 32][i], and zero padding past N
        e0 = edges[3]
        i, j = np.argwhere(dense[e0])[5]
        assert (int(packed.bits[3, j // 32, i]) >> (j % 32)) & 1
        if n % 32:
            assert not (packed.bits[:, -1, :] >> (n % 32)).any()
    with pytest.raises(ValueError):
        pack_pairwise({e: np.zeros((n, n + 1)) for e in edges})


def test_packed_golden_constraint_is_numpy_packbits(golden):
    from multiviews.pictorial import pack_pairwise
    g = golden('rpsm_a.npz')
    n = int(g['first_nbins']) ** 3
    bits = np.unpackbits(g['pairwise_bits'][0], axis=-1, bitorder='little')[:, :, :n]
    packed = pack_pairwise({tuple(e): bits[i] for i, e in enumerate(g['edges'].tolist())})
    rows = np.ascontiguousarray(np.transpose(packed.bits, (0, 2, 1)))       # [E, N, words]: numpy.packbits rows
    raw = rows.view(np.uint8)[:, :, :g['pairwise_bits'].shape[-1]]
    assert np.array_equal(raw, g['pairwise_bits'][0])


def _tree():
    from multiviews.body import HumanBody
    from posu.ops import RpsmTree
    body = HumanBody()
    return RpsmTree(body.parents(), body.children())


def test_rpsm_argument_errors_are_reported_without_a_gpu():
    """Every entry point validates on the host before any launch: null pointer, N > 4096, H != W,
    V = 0, J = 33 (and a bad tree)."""
    lib = _native.load()
    p = ctypes.c_void_p(256)
    tree = _tree()
    t = tree.args()
    host = np.ones(40)
    hp = ctypes.c_void_p(host.ctypes.data)

    def err(st, text):
        assert st == 1, st
        assert text in _native.last_error(), _native.last_error()

    assert lib.posu_rpsm_workspace_bytes(1, 16, 16, 2) > 0
    assert lib.posu_rpsm_workspace_bytes(1, 16, 17, 2) == -1
    assert lib.posu_rpsm_workspace_bytes(1, 33, 16, 2) == -1
    assert lib.posu_rpsm_workspace_bytes(1, 16, 16, 1) == -1

    err(lib.posu_rpsm_grid(None, 1, 100.0, 4, p, None), 'null pointer')
    err(lib.posu_rpsm_grid(p, 1, 100.0, 17, p, None), '4096')
    err(lib.posu_rpsm_grid(p, 1, 100.0, 1, p, None), 'nbins >= 2')

    def unary(hm=p, V=4, J=16, H=24, W=24, N=125):
        return lib.posu_rpsm_unary(hm, p, p, 1, V, J, H, W, 256.0, 256.0, p, 1, N, p, None)
    err(unary(hm=None), 'null pointer')
    err(unary(N=4097), '4096')
    err(unary(W=32), 'H == W')
    err(unary(V=0), '1 <= V <= 8')
    err(unary(V=9), '1 <= V <= 8')
    err(unary(J=33), '2 <= J <= 32')

    def infer(u=p, J=16, N=125, mask=p, tr=t):
        return lib.posu_rpsm_infer(u, *tr, mask, None, 1, None, 0.0, 1, J, N, p, p, p, None)
    err(infer(u=None), 'null pointer')
    err(infer(mask=None), 'null pointer')
    err(infer(N=4097), '4096')
    err(infer(J=33), '2 <= J <= 32')
    two_roots = tree.parent.copy()
    two_roots[0] = -1
    err(infer(tr=(ctypes.c_void_p(two_roots.ctypes.data),) + t[1:]), 'bad tree')
    cyc = tree.parent.copy()
    cyc[[6, 2]] = 2, 6
    err(infer(tr=(ctypes.c_void_p(cyc.ctypes.data),) + t[1:]), 'bad tree')

    def back(e=p, J=16, N=125):
        return lib.posu_rpsm_backtrack(e, p, *t, p, 1, 1, J, N, p, p, None)
    err(back(e=None), 'null pointer')
    err(back(N=4097), '4096')
    err(back(J=33), '2 <= J <= 32')

    def pmask(gr=p, J=16, N=125):
        return lib.posu_rpsm_pairwise_mask(gr, 1, N, *t, J, hp, hp, 1, p, None)
    err(pmask(gr=None), 'null pointer')
    err(pmask(N=4097), '4096')
    err(pmask(J=33), '2 <= J <= 32')

    def run(hm=p, V=4, J=16, H=24, W=24, nb=5, rb=2, ws=1 << 30):
        return lib.posu_rpsm_run(hm, p, p, 1, V, J, H, W, 256.0, 256.0, p, 600.0, nb, rb, 3, 150.0, hp, p, *t, p,
                                 ws, p, None, None)
    err(run(hm=None), 'null pointer')
    err(run(nb=17), '4096')
    err(run(rb=1), 'nbins >= 2')
    err(run(W=32), 'H == W')
    err(run(V=0), '1 <= V <= 8')
    err(run(J=33), '2 <= J <= 32')
    err(run(ws=16), 'workspace')


def test_limb_length_tables_per_group_or_shared():
    """rpsm_batch's limb_lengths: one dict per group (or [G, J]), or one dict / [J] for all groups."""
    from multiviews.pictorial import _limb_rows
    tree = _tree()
    rng = np.random.RandomState(0)
    dicts = [{e: float(rng.uniform(100, 400)) for e in tree.edges} for _ in range(3)]
    rows = _limb_rows(dicts, tree, 3)
    assert rows.shape == (3, 16) and rows.dtype == np.float64
    for g, d in enumerate(dicts):
        for (p, c), v in d.items():
            assert rows[g, c] == v
        assert rows[g, 6] == 0                      # the root has no limb
    assert np.array_equal(_limb_rows(dicts[1], tree, 3), np.tile(rows[1], (3, 1)))
    assert np.array_equal(_limb_rows(rows, tree, 3), rows)
    assert np.array_equal(_limb_rows(rows[2], tree, 2), np.tile(rows[2], (2, 1)))
    with pytest.raises(ValueError):
        _limb_rows(dicts[:2], tree, 3)
    with pytest.raises(ValueError):
        _limb_rows(np.zeros((3, 15)), tree, 3)
    broken = dict(dicts[0])
    del broken[tree.edges[4]]
    with pytest.raises(KeyError):
        _limb_rows([broken, dicts[1], dicts[2]], tree, 3)


def test_rpsm_refuses_to_run_without_a_device_or_on_bad_input(monkeypatch):
    import torch
    from multiviews import pictorial
    with pytest.raises(ValueError, match='square'):
        pictorial._heatmaps(np.zeros((4, 16, 24, 32), dtype=np.float32), torch.device('cpu'), 1, 4)
    monkeypatch.setattr(torch.cuda, 'is_available', lambda: False)
    with pytest.raises(RuntimeError, match='cuda'):
        pictorial.rpsm([], np.zeros((4, 16, 24, 24), dtype=np.float32), [], np.zeros(3), {}, {}, None)
    with pytest.raises(RuntimeError, match='cuda'):
        pictorial.infer([np.zeros(8)] * 16, {}, None)
    with pytest.raises(RuntimeError, match='cuda'):
        pictorial.compute_pairwise_constraint(600.0, {}, 5)
