"""The 16-joint MPII skeleton tree of the pictorial structure model (reference
lib/multiviews/body.py): ``skeleton`` (one dict per joint: idx, name, children, and after the
level sort parent / level), ``skeleton_sorted_by_level`` (deepest first, the order infer walks)
and ``root_idx``.  ``parents()`` / ``children()`` give the same tree as the arrays the RPSM
kernels take (posu.ops.RpsmTree).
"""
import numpy as np

JOINT_NAMES = ('rank', 'rkne', 'rhip', 'lhip', 'lkne', 'lank', 'root', 'thorax', 'upper neck', 'head top',
               'rwri', 'relb', 'rsho', 'lsho', 'lelb', 'lwri')
# joint -> its parent (mpii order); every children list is its joints in ascending order
# (root: [2, 3, 7], thorax: [8, 12, 13]), which is also the order infer multiplies them in
PARENT = (1, 2, 6, 6, 3, 4, -1, 6, 7, 8, 11, 12, 7, 7, 13, 14)
ROOT = 6


class HumanBody(object):

    def __init__(self):
        self.root_idx = ROOT
        self.skeleton = self.get_skeleton()
        self.skeleton_sorted_by_level = self.sort_skeleton_by_level(self.skeleton)

    def get_skeleton(self):
        kids = [[] for _ in JOINT_NAMES]
        for j, p in enumerate(PARENT):
            if p >= 0:
                kids[p].append(j)
        return [{'idx': i, 'name': n, 'children': kids[i]} for i, n in enumerate(JOINT_NAMES)]

    def sort_skeleton_by_level(self, skeleton):
        """Breadth-first levels from the root, then descending by numpy's default argsort
        reversed -- the reference's order, ties included (body.py:39-57)."""
        level = np.zeros(len(skeleton))
        queue = [ROOT]
        while queue:
            cur = queue.pop(0)
            for child in skeleton[cur]['children']:
                skeleton[child]['parent'] = cur
                level[child] = level[cur] + 1
                queue.append(child)
        out = []
        for i in np.argsort(level)[::-1]:
            skeleton[i]['level'] = level[i]
            out.append(skeleton[i])
        return out

    def parents(self):
        """int32 [J]: every joint's parent, -1 for the root."""
        return np.array([n.get('parent', -1) for n in self.skeleton], dtype=np.int32)

    def children(self):
        """Every joint's ordered children (list of lists)."""
        return [list(n['children']) for n in self.skeleton]

    def edges(self):
        """(parent, child) in skeleton order: the rows of a packed pairwise constraint."""
        return [(n['idx'], c) for n in self.skeleton for c in n['children']]
