"""Golden for the data-path kernels: the REFERENCE's
JointsDatasetCompatible.generate_heatmap (lib/dataset/joints_dataset_compatible.py,
imported in-process with stand-ins for cv2 / torchvision, which are not installed and
which generate_heatmap does not use) called per sample on seeded joints, and the
integral decode of run/test/test_integral.py:63-70 (a script: its lines are restated
here as numpy on seeded heatmaps).  Run once in this container:

    python tests/golden/make_datapath_golden.py

A second, separate recorder writes datapath_edges.npz: generate_heatmap on non-square maps,
anisotropic strides, a non-integer 3 * sigma and patches that just touch or just miss an edge:

    python tests/golden/make_datapath_golden.py edges
"""
import os
import sys
import types

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))


def datapath_inputs(seed=0):
    r = np.random.default_rng(seed)
    n, j = 6, 16
    joints = r.uniform(-20, 276, size=(n, j, 2)).astype(np.float32)
    joints[0, :4] = [[0.0, 0.0], [255.9, 255.9], [-13.0, 100.0], [270.0, 5.0]]   # corners / just outside
    joints[1, :3] = [[-2.1, -1.7], [1.9, 2.2], [258.0, 258.0]]                    # int() truncation at < 0
    vis = (r.uniform(size=(n, j)) > 0.2).astype(np.float32)
    sources = np.array(['mpii', 'h36m', 'mpii', 'h36m', 'mpii', 'mpii'])
    hm = np.abs(r.standard_normal((4, j, 64, 64))).astype(np.float32)
    return joints, vis, sources, hm


# (image (w, h), heatmap (w, h), sigma) of the edge-case golden, datapath_edges.npz
EDGE_CASES = [((96, 128), (24, 32), 1), ((96, 72), (32, 18), 2), ((128, 128), (32, 32), 3),
              ((128, 128), (32, 32), 1.5)]


def _joint_at(mu, stride):
    """A joint coordinate whose int(joint / stride + 0.5) is mu, a quarter cell from either boundary."""
    return stride * (mu + 0.25) if mu >= 0 else stride * (mu - 0.75)


def datapath_edge_inputs(case, seed=100):
    """joints [2, 16, 2] f32 and vis [2, 16] f32 of edge case `case`: rows 0-7 of each sample are
    placed from the case's strides and tmp = 3 * sigma (sample 0 works the x axis, sample 1 the y
    axis), the rest are seeded uniform over [-0.1, 1.1] x the image size."""
    (iw, ih), (hw, hh), sigma = EDGE_CASES[case]
    r = np.random.default_rng(seed + case)
    n, j = 2, 16
    joints = (r.uniform(-0.1, 1.1, size=(n, j, 2)) * np.array([iw, ih])).astype(np.float32)
    vis = r.choice(np.array([0.0, 1.0, 1.0, 1.0, 0.5], dtype=np.float32), size=(n, j))
    vis[:, :8] = 1.0
    tmp = 3 * sigma
    stride = (iw / hw, ih / hh)
    size = (hw, hh)
    for a in (0, 1):          # the axis under test; the other coordinate sits mid-map
        b = 1 - a
        ul_last = int(np.ceil(size[a] - 1 + tmp))      # int(mu - tmp) == size - 1: one column / row painted
        ul_out = int(np.ceil(size[a] + tmp))           # int(mu - tmp) == size: outside, weight 0
        br_zero = int(np.floor(-tmp - 2)) + 1          # int(mu + tmp + 1) == 0: touching, nothing painted
        br_out = br_zero - 1                           # int(mu + tmp + 1) == -1: outside, weight 0
        assert int(ul_last - tmp) == size[a] - 1 and int(ul_out - tmp) == size[a]
        assert int(br_zero + tmp + 1) == 0 and int(br_out + tmp + 1) == -1
        along = [-0.4 * stride[a], -0.6 * stride[a], -1.6 * stride[a]]           # int() truncates, floor differs
        along += [_joint_at(m, stride[a]) for m in (ul_last, ul_out, br_zero, br_out)]
        mid = stride[b] * (size[b] // 2 + 0.25)
        for k, v in enumerate(along):
            joints[a, k, a] = v
            joints[a, k, b] = mid
    joints[0, 7] = [stride[0] * (5 + 0.5), stride[1] * (7 + 0.5)]               # mu exactly on a .5 boundary
    joints[1, 7] = [stride[0] * (hw // 2 + 0.25), stride[1] * (hh // 2 + 0.25)]
    vis[1, 7] = 0.5                                                             # keeps its weight, paints nothing
    vis[0, 8], vis[0, 9], vis[0, 10] = 0.0, 0.5, 1.0
    return joints, vis


def _reference_dataset_class():
    sys.path.insert(0, '/root/reference/lib')
    sys.modules.setdefault('cv2', types.ModuleType('cv2'))
    tv = types.ModuleType('torchvision')
    tv.transforms = types.ModuleType('torchvision.transforms')
    sys.modules.setdefault('torchvision', tv)
    sys.modules.setdefault('torchvision.transforms', tv.transforms)
    import importlib.util
    spec = importlib.util.spec_from_file_location(
        'ref_joints_dataset_compatible', '/root/reference/lib/dataset/joints_dataset_compatible.py')
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod.JointsDatasetCompatible


def edges_main():
    """The second recorder: generate_heatmap on the edge cases -> datapath_edges.npz (datapath.npz is
    not touched).  python tests/golden/make_datapath_golden.py edges"""
    JointsDatasetCompatible = _reference_dataset_class()
    out = {}
    for case, (image, heatmap, sigma) in enumerate(EDGE_CASES):
        joints, vis = datapath_edge_inputs(case)
        stub = types.SimpleNamespace(num_joints=16, heatmap_size=np.array(heatmap), image_size=np.array(image),
                                     sigma=sigma, pseudo_label=False)
        targets, weights = [], []
        for n in range(joints.shape[0]):
            jv = np.stack([vis[n], vis[n]], axis=1)
            t, w = JointsDatasetCompatible.generate_heatmap(stub, joints[n].copy(), jv, 'mpii')
            targets.append(t)
            weights.append(w)
        out['joints_%d' % case], out['vis_%d' % case] = joints, vis
        out['targets_%d' % case], out['weights_%d' % case] = np.stack(targets), np.stack(weights)
        print('case %d: weights sum %g, painted maps %d' % (case, np.stack(weights).sum(),
                                                            int((np.stack(targets).max(axis=(2, 3)) > 0).sum())))
    np.savez_compressed(os.path.join(HERE, 'datapath_edges.npz'), **out)
    print('datapath edges golden written')


def main():
    sys.path.insert(0, '/root/reference/lib')
    sys.modules.setdefault('cv2', types.ModuleType('cv2'))
    tv = types.ModuleType('torchvision')
    tv.transforms = types.ModuleType('torchvision.transforms')
    sys.modules.setdefault('torchvision', tv)
    sys.modules.setdefault('torchvision.transforms', tv.transforms)
    # the module file itself (the dataset package __init__ pulls in json_tricks etc.)
    import importlib.util
    spec = importlib.util.spec_from_file_location(
        'ref_joints_dataset_compatible', '/root/reference/lib/dataset/joints_dataset_compatible.py')
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    JointsDatasetCompatible = mod.JointsDatasetCompatible
    joints, vis, sources, hm = datapath_inputs()
    stub = types.SimpleNamespace(num_joints=16, heatmap_size=np.array([64, 64]), image_size=np.array([256, 256]),
                                 sigma=2, pseudo_label=False)
    targets, weights = [], []
    for n in range(joints.shape[0]):
        jv = np.stack([vis[n], vis[n]], axis=1)
        t, w = JointsDatasetCompatible.generate_heatmap(stub, joints[n].copy(), jv, sources[n])
        targets.append(t)
        weights.append(w)
    # test_integral.py:63-70
    h = hm / np.sum(hm, axis=(2, 3), keepdims=True)
    coordinates = np.arange(64).reshape((1, 1, 64))
    accu_w = np.sum(h, axis=2)
    accu_h = np.sum(h, axis=3)
    integral = np.stack((np.sum(accu_w * coordinates, axis=2), np.sum(accu_h * coordinates, axis=2)), axis=2)
    np.savez_compressed(os.path.join(HERE, 'datapath.npz'), targets=np.stack(targets), weights=np.stack(weights),
                        integral=integral)
    print('datapath golden written', np.stack(weights).sum())


if __name__ == '__main__':
    edges_main() if sys.argv[1:] == ['edges'] else main()
