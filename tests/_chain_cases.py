"""The lists the cluster-chain tests share (tests/test_cluster_chain_host.py asserts the coverage of exactly what
tests/test_cluster_chain_gpu.py runs): toy events with slabs knocked out of every track, hand-built scenes, the ring, the line and the
lattice.  Everything is made once per key and handed out read-only."""
import numpy as np

from uresnet_amd import synthetic_io as sio
from uresnet_amd.clusters import ClusterSpec, cluster_numpy

SPEC = ClusterSpec(None, (1, 2), True)           # 26 neighbours in 3-D, 8 in 2-D
# name -> (shape, entries, slabs (axis, period, first, width), max_gap, min_cos): a voxel survives when on every slab's axis its
# coordinate % period lies outside [first, first + width)
FIXTURES = {
    "angles": ((32, 32, 32), (0, 1, 2), ((0, 6, 2, 2), (1, 7, 3, 2)), 12, 0.7),
    "long": ((32, 32, 32), (0, 1), ((0, 8, 3, 2), (2, 10, 3, 2)), 12, 0.8),
    "value": ((32, 32, 32), (0, 1), ((0, 12, 5, 2), (2, 10, 3, 2)), 6, 0.9),
    "flat": ((24, 20), (0, 1), ((0, 7, 3, 2),), 6, 0.8),
}
_made = {}


def ids_of(off, index, cls, shape, spec):
    """cluster_numpy per event: (ids, table offsets, the table's cls)."""
    ids, counts, tcls = [], [], []
    for e in range(len(off) - 1):
        c, first, _, k = cluster_numpy(index[off[e]:off[e + 1]], cls[off[e]:off[e + 1]], shape, spec)
        ids.append(c), counts.append(first.size), tcls.append(k)
    return np.concatenate(ids), np.concatenate([[0], np.cumsum(counts)]).astype(np.int64), np.concatenate(tcls)


def _frozen(*arrays):
    for a in arrays:
        a.setflags(write=False)
    return arrays


def fixture(name):
    """(off, index, value, cluster, toff, tcls, truth, truth_toff): the surviving voxels of the named events, their true classes
    clustered under SPEC, and as ``truth`` the clusters of the unbroken lists restricted to the survivors."""
    if name not in _made:
        shape, entries, slabs, _, _ = FIXTURES[name]
        lists, classes, values, truths, tcounts = [], [], [], [], []
        for e in entries:
            vb = sio.dense_to_voxels(*sio.lartpc_sparse(list(shape) + [1], 3, e))
            index, label = np.asarray(vb.index, np.int64), np.asarray(vb.label).astype(np.uint8)
            whole, first, _, _ = cluster_numpy(index, label, shape, SPEC)
            coords = np.unravel_index(index, shape)
            keep = np.ones(index.size, bool)
            for axis, period, k0, w in slabs:
                keep &= ~((coords[axis] % period >= k0) & (coords[axis] % period < k0 + w))
            left = whole[keep]
            alive = np.unique(left[left >= 0])                 # a truth row that lost every voxel is renumbered away
            renumber = np.full(first.size + 1, -1, np.int64)
            renumber[alive] = np.arange(alive.size)
            lists.append(index[keep]), classes.append(label[keep]), values.append(np.asarray(vb.value, np.float32)[keep])
            truths.append(renumber[left]), tcounts.append(alive.size)
        off = np.concatenate([[0], np.cumsum([a.size for a in lists])]).astype(np.int64)
        index, cls, value = np.concatenate(lists), np.concatenate(classes), np.concatenate(values)
        cluster, toff, tcls = ids_of(off, index, cls, shape, SPEC)
        truth_toff = np.concatenate([[0], np.cumsum(tcounts)]).astype(np.int64)
        _made[name] = _frozen(off, index, value, cluster, toff, tcls, np.concatenate(truths), truth_toff)
    return _made[name]


def scene(shape, events, spec):
    """``events``: per event a list of (points, class).  The lists sorted by index, clustered by cluster_numpy under ``spec``.
    Returns (off, index, ids, toff, tcls) and ``at(event, point)`` = the global list position of a point."""
    off, index, cls, where = [0], [], [], {}
    for e, segs in enumerate(events):
        pts = [(tuple(p), c) for points, c in segs for p in points]
        flat = np.array([np.ravel_multi_index(p, shape) for p, _ in pts], np.int64)
        order = np.argsort(flat)
        for k, o in enumerate(order):
            where[(e, pts[o][0])] = off[-1] + k
        index.append(flat[order]), cls.append(np.array([pts[o][1] for o in order], np.uint8))
        off.append(off[-1] + flat.size)
    off, index, cls = np.array(off, np.int64), np.concatenate(index), np.concatenate(cls)
    ids, toff, tcls = ids_of(off, index, cls, shape, spec)
    return (off, index, ids, toff, tcls), lambda e, p: where[(e, tuple(p))]


def ring():
    """An octagon of eight 3-voxel fragments in the plane x0 = 8 of (16, 32, 32): four axis-parallel sides and four diagonal ones,
    every corner a gap of (0, 2, 2) or so.  At min_cos 0.7 every end joins its neighbour's: a ring."""
    sides = [[(8, 6, c) for c in (13, 14, 15)], [(8, 8 + k, 18 + k) for k in range(3)], [(8, r, 22) for r in (13, 14, 15)],
             [(8, 18 + k, 20 - k) for k in range(3)], [(8, 22, c) for c in (15, 14, 13)], [(8, 20 - k, 10 - k) for k in range(3)],
             [(8, r, 6) for r in (15, 14, 13)], [(8, 10 - k, 8 + k) for k in range(3)]]
    return scene((16, 32, 32), [[(pts, 1) for pts in sides]], ClusterSpec(26, (1,), False))


def line(fragments=10):
    """``fragments`` 3-voxel fragments along the last axis of (8, 8, 64) with holes of 3 voxels, in two events."""
    segs = [([(3, 4, 6 * k + c) for c in range(3)], 1) for k in range(fragments)]
    return scene((8, 8, 6 * fragments + 4), [segs, segs[:3]], ClusterSpec(26, (1,), False))


def lattice(rows=2100, filler=60000):
    """``rows`` 3-voxel fragments along the last axis, ten to a line (holes of 2 voxels, pitch 5), the lines on a pitch of 4 in
    both other axes of a volume (planes, 32, 52); behind them ``filler`` entries without a cluster, so that the list is longer
    than one chunk of every scan.  One event.  Returns (shape, index, ids, rows)."""
    key = ("lattice", rows, filler)
    if key not in _made:
        lines = -(-rows // 10)
        planes = -(-lines // 8)
        pts = []
        for r in range(rows):
            ln, k = divmod(r, 10)
            pts += [(4 * (ln // 8), 4 * (ln % 8), 5 * k + c) for c in range(3)]
        shape = (4 * planes + 1 + -(-filler // (32 * 52)), 32, 52)
        index = np.ravel_multi_index(np.array(pts).T, shape)
        order = np.argsort(index, kind="stable")
        ids_sorted = np.repeat(np.arange(rows), 3)[order]
        # ids numbered by lowest position, as ursn_cluster_voxels numbers them
        _, firsts = np.unique(ids_sorted, return_index=True)
        rank = np.empty(rows, np.int64)
        rank[ids_sorted[np.sort(firsts)]] = np.arange(rows)
        start = (4 * planes + 1) * 32 * 52
        index = np.concatenate([index[order], start + np.arange(filler)])
        ids = np.concatenate([rank[ids_sorted], np.full(filler, -1)])
        assert (np.diff(index) > 0).all() and index[-1] < np.prod(shape)
        _made[key] = (shape,) + _frozen(index, ids) + (rows,)
    return _made[key]
