"""The lists the cluster-cone tests share (tests/test_cluster_cone_host.py asserts the coverage of exactly what
tests/test_cluster_cone_gpu.py runs): hand-built scenes around one or two stems, the far scene whose apexes lie more than 63 planes
away on both sides, the lattice that is longer than one chunk of every scan, and the toy showers.  Everything is made once per key
and handed out read-only."""
import numpy as np

from _chain_cases import _frozen, ids_of, scene
from uresnet_amd.clusters import ClusterConeSpec, ClusterSpec

ONE = ClusterSpec(26, (1, 2, 3), True)            # 26 neighbours; voxels of different class never share a cluster
FLAT = ClusterSpec(8, (1, 2, 3), True)
_made = {}


def stem(a, b, c0, n, cls=1):
    """``n`` voxels along the last axis from (a, b, c0)."""
    return ([(a, b, c0 + k) for k in range(n)], cls)


def dot(p, cls=1):
    return ([tuple(p)], cls)


def _boundary():
    """A stem of 8 with apexes A = (20, 10, 4) and B = (20, 10, 11).  From A: (3, 0, 4) away, cos exactly 0.8; (0, 4, 3) away, cos
    0.6; (0, 0, 13) away, beyond reach 12 on one axis only; (4, 3, 12) away, inside the box but dist2 = 169 > 144."""
    segs = [stem(20, 10, 4, 8), dot((23, 10, 8)), dot((20, 14, 7)), dot((20, 10, 17)), dot((24, 13, 16))]
    return (48, 32, 32), [segs], ClusterConeSpec(12, 0.8, 8, 1)


def _tie():
    """Two stems of 8, a voxel (0, +-5, 5) from the first apex of each: dist2 50 twice, cos 0.707 at min_cos 0.7."""
    segs = [stem(10, 10, 4, 8), stem(10, 20, 4, 8), dot((10, 15, 9))]
    return (32, 32, 32), [segs], ClusterConeSpec(12, 0.7, 8, 1)


def _rank():
    """Two collinear stems of 8: equal n, so the lower row is the parent of the other, never the reverse."""
    return (32, 32, 32), [[stem(10, 10, 2, 8), stem(10, 10, 14, 8)]], ClusterConeSpec(24, 0.8, 8, 1)


def _misaligned():
    """A stem of 9 and, on its line, a bar of 8 across it: aligned in the cone, square to the axis.  At seed_size 9 the bar has no
    axis to speak of and the cone alone decides."""
    return (32, 32, 32), [[stem(10, 10, 2, 9), ([(10, 6 + k, 16) for k in range(8)], 1)]], ClusterConeSpec(24, 0.8, 8, 1)


MISALIGNED_LOOSE = ClusterConeSpec(24, 0.8, 9, 1)


def _tree():
    """A primary of 10, a fragment of 4 on its line (itself a parent at seed_size 4), a voxel behind that (depth 2), and a voxel in
    the primary's cone that comes earlier in the list than the primary."""
    segs = [stem(20, 10, 10, 10), stem(20, 10, 24, 4), dot((20, 10, 30)), dot((18, 10, 14))]
    return (48, 32, 40), [segs], ClusterConeSpec(24, 0.8, 4, 1)


def _sides():
    """A stem of 10 at (20, 10, 10..19) with children beyond both of its ends, five events: more members on one side (and the
    mirror), equal members but more children on one side (and the mirror), equal both."""
    p = stem(20, 10, 10, 10)
    events = [[p, dot((20, 10, 23)), stem(20, 10, 4, 3)], [p, stem(20, 10, 23, 3), dot((20, 10, 6))],
              [p, stem(20, 10, 23, 2), dot((20, 10, 6)), dot((20, 12, 4))], [p, dot((20, 10, 23)), dot((20, 12, 25)), stem(20, 10, 5, 2)],
              [p, dot((20, 10, 23)), dot((20, 10, 6))]]
    return (48, 32, 40), events, ClusterConeSpec(24, 0.8, 8, 1)


def _classes():
    """A stem of class 1 with a voxel of class 1 and a voxel of class 2 on its cone's boundary."""
    segs = [stem(20, 10, 4, 8), dot((23, 10, 8)), dot((20, 13, 8), 2)]
    return (48, 32, 32), [segs], ClusterConeSpec(12, 0.8, 8, 1)


def _coincide():
    """A stem of 9 (class 1) and a ring of 8 (class 2) around its first voxel: the ring's anchor IS that apex voxel, dist2 = 0."""
    ring = [(19 + i, 9 + j, 4) for i in range(3) for j in range(3) if (i, j) != (1, 1)]
    return (48, 32, 32), [[stem(20, 10, 4, 9), (ring, 2)]], ClusterConeSpec(12, 0.8, 9, 1, None, False)


def _empty_mid():
    """An empty event between two full ones."""
    return (48, 32, 32), [_boundary()[1][0], [], _tie()[1][0]], ClusterConeSpec(12, 0.7, 8, 1)


def _flat():
    """2-D: a stem of 8 along the last axis, a voxel (3, 4) from its first end (cos exactly 0.8) and one (-4, 3) from it."""
    segs = [([(10, 4 + k) for k in range(8)], 1), ([(13, 8)], 1), ([(6, 7)], 1)]
    return (40, 40), [segs], ClusterConeSpec(12, 0.8, 8, 1)


def _far():
    """reach 127: stems along the FIRST axis, so their apexes lie in other planes than the child at (100, 8, 8): 80 planes below
    and 80 above (the wave's trips 0 and 3), 20 below and 17 above (trips 1 and 2)."""
    along = lambda x0, n, b, c: ([(x0 + k, b, c) for k in range(n)], 1)
    segs = [along(20, 10, 8, 8), along(171, 10, 8, 8), along(80, 8, 8, 12), along(110, 8, 8, 4), dot((100, 8, 8))]
    return (200, 16, 16), [segs], ClusterConeSpec(127, 0.8, 8, 1)


SCENES = {"boundary": _boundary, "tie": _tie, "rank": _rank, "misaligned": _misaligned, "tree": _tree, "sides": _sides,
          "classes": _classes, "coincide": _coincide, "empty_mid": _empty_mid, "flat": _flat, "far": _far}


def named(name):
    """(shape, (off, index, ids, toff, tcls), at, spec) of a hand-built scene."""
    if name not in _made:
        shape, events, spec = SCENES[name]()
        lists, at = scene(shape, events, ONE if len(shape) == 3 else FLAT)
        _made[name] = (shape, _frozen(*lists), at, spec)
    return _made[name]


def lattice(stems=2100, filler=60000):
    """``stems`` three-voxel stems along the last axis on a pitch of 4 in both other axes of (planes, 32, 8), each with one voxel
    two beyond its far end (its only child at reach 5, seed_size 3), and behind them ``filler`` entries without a cluster: more
    rows, apexes and tiles than one chunk of any scan.  One event.  Returns (shape, index, ids, rows)."""
    key = ("lattice", stems, filler)
    if key not in _made:
        planes = 4 * -(-stems // 8)
        pts, owner = [], []
        for s in range(stems):
            a, b = 4 * (s // 8), 4 * (s % 8)
            pts += [(a, b, 0), (a, b, 1), (a, b, 2), (a, b, 4)]
            owner += [2 * s, 2 * s, 2 * s, 2 * s + 1]
        shape = (planes + 1 + -(-filler // (32 * 8)), 32, 8)
        index = np.ravel_multi_index(np.array(pts).T, shape)
        order = np.argsort(index, kind="stable")
        own = np.array(owner)[order]
        _, firsts = np.unique(own, return_index=True)         # ids numbered by lowest position, as ursn_cluster_voxels numbers them
        rank = np.empty(2 * stems, np.int64)
        rank[own[np.sort(firsts)]] = np.arange(2 * stems)
        start = (planes + 1) * 32 * 8
        index = np.concatenate([index[order], start + np.arange(filler)])
        ids = np.concatenate([rank[own], np.full(filler, -1)])
        assert (np.diff(index) > 0).all() and index[-1] < np.prod(shape)
        _made[key] = (shape,) + _frozen(index, ids) + (2 * stems,)
    return _made[key]


LATTICE_SPEC = ClusterConeSpec(5, 0.8, 3, 1, None, False)

# ---- the toy showers -------------------------------------------------------------------------------------------------------------
TOY_SHAPE = (96, 64, 64)
TOY_SEEDS = (1, 2, 3, 4, 5, 6)
TOY_SPEC = ClusterConeSpec(48, 0.7, 8, 1, None, False)
TOY_STARTS = ((10, 16, 16), (10, 47, 47))        # the two cones open along the first axis and stay 15.6 voxels wide: they do not cross


def _toy_event(seed):
    """Two showers: a 12-voxel stem along the first axis and 25 fragments of 1 to 5 voxels (short lines along the first axis) whose
    first voxel lies 16 to 46 voxels from the stem's start inside a half-angle of 18 degrees.  Returns (index, truth) sorted."""
    rng = np.random.default_rng(seed)
    voxels = {}
    for s, (a, b, c) in enumerate(TOY_STARTS):
        for k in range(12):
            voxels[(a + k, b, c)] = s
        for _ in range(25):
            r, theta, phi = rng.uniform(16.0, 46.0), np.radians(rng.uniform(0.0, 18.0)), rng.uniform(0.0, 2.0 * np.pi)
            p = (a + r * np.cos(theta), b + r * np.sin(theta) * np.cos(phi), c + r * np.sin(theta) * np.sin(phi))
            p = [int(round(x)) for x in p]
            for k in range(int(rng.integers(1, 6))):
                q = (p[0] + k, p[1], p[2])
                if all(0 <= x < d for x, d in zip(q, TOY_SHAPE)):
                    voxels.setdefault(q, s)
    pts = sorted(voxels, key=lambda q: np.ravel_multi_index(q, TOY_SHAPE))
    return np.array([np.ravel_multi_index(q, TOY_SHAPE) for q in pts], np.int64), np.array([voxels[q] for q in pts], np.int64)


def toys():
    """(off, index, cluster, toff, tcls, truth, truth_toff): one event per seed, every voxel of class 1, clustered with 26
    neighbours; ``truth`` is the shower a voxel was generated for."""
    if "toys" not in _made:
        made = [_toy_event(seed) for seed in TOY_SEEDS]
        off = np.concatenate([[0], np.cumsum([m[0].size for m in made])]).astype(np.int64)
        index, truth = np.concatenate([m[0] for m in made]), np.concatenate([m[1] for m in made])
        cluster, toff, tcls = ids_of(off, index, np.ones(index.size, np.uint8), TOY_SHAPE, ClusterSpec(26, (1,), False))
        truth_toff = 2 * np.arange(len(TOY_SEEDS) + 1, dtype=np.int64)
        _made["toys"] = _frozen(off, index, cluster, toff, tcls, truth, truth_toff)
    return _made["toys"]
