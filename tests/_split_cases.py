"""Small lists for the cluster split (tests/test_cluster_split_host.py asserts what they cover, tests/test_cluster_split_gpu.py runs
them on the device).  Plain helper module (not a conftest).  A case is a dict: ``shape``, ``off``, ``index``, ``cluster``, ``toff``,
``size``, ``cls`` -- concatenated per-event lists with a clustering in the format ursn_cluster_voxels writes (ids numbered by the
lowest position of a row).  The rows are GIVEN, not computed: a case may put two separate limbs into one row."""
import numpy as np

_cache = {}


def segment(p, q):
    """The voxels of the straight line from p to q: every step moves by at most 1 on every axis."""
    p, q = np.array(p, np.int64), np.array(q, np.int64)
    steps = int(np.abs(q - p).max())
    if steps == 0:
        return {tuple(int(x) for x in p)}
    return {tuple(int(x) for x in np.rint(p + (q - p) * (t / steps)).astype(np.int64)) for t in range(steps + 1)}


def path(*points):
    out = set()
    for a, b in zip(points[:-1], points[1:]):
        out |= segment(a, b)
    return out


def shifted(cells, d):
    return {tuple(c[a] + d[a] for a in range(len(d))) for c in cells}


def event(shape, rows, noise=()):
    """One event: ``rows`` = [(cells, cls)], disjoint sets of coordinates, each ONE cluster row; ``noise`` cells get the id -1.
    Returns (index, ids, first, size, cls), ids numbered by the lowest position."""
    owner = {}
    for k, (cells, _) in enumerate(rows):
        for c in cells:
            assert c not in owner and all(0 <= c[a] < shape[a] for a in range(len(shape))), (c, shape)
            owner[c] = k
    for c in noise:
        assert c not in owner
        owner[c] = -1
    cells = sorted(owner, key=lambda c: int(np.ravel_multi_index(c, shape)))
    index = np.array([int(np.ravel_multi_index(c, shape)) for c in cells], np.int64)
    number, first, size = {}, [], []
    ids = np.full(index.size, -1, np.int64)
    for j, c in enumerate(cells):
        k = owner[c]
        if k < 0:
            continue
        if k not in number:
            number[k] = len(number)
            first.append(j)
            size.append(0)
        ids[j] = number[k]
        size[number[k]] += 1
    order = sorted(number, key=number.get)
    return index, ids, np.array(first, np.int32), np.array(size, np.int32), np.array([rows[k][1] for k in order], np.uint8)


def batch(shape, events):
    """``events``: a list of (rows, noise) -> a case."""
    made = [event(shape, rows, noise) for rows, noise in events]
    cat = lambda k, dt: np.concatenate([m[k] for m in made]).astype(dt) if made else np.zeros(0, dt)
    return {"shape": tuple(shape), "off": np.concatenate([[0], np.cumsum([m[0].size for m in made])]).astype(np.int64),
            "index": cat(0, np.int64), "cluster": cat(1, np.int64),
            "toff": np.concatenate([[0], np.cumsum([m[2].size for m in made])]).astype(np.int64),
            "first": cat(2, np.int32), "size": cat(3, np.int32), "cls": cat(4, np.uint8)}


def _ring(c, radius, n=96):
    return {(c[0], int(round(c[1] + radius * np.cos(2 * np.pi * t / n))), int(round(c[2] + radius * np.sin(2 * np.pi * t / n))))
            for t in range(n)}


def jack(c, arm):
    """Six arms of ``arm`` voxels from one centre: with radius == arm every voxel sees three arms or more."""
    out = {tuple(c)}
    for a in range(3):
        for s in (-1, 1):
            for k in range(1, arm + 1):
                out.add(tuple(c[b] + (s * k if b == a else 0) for b in range(3)))
    return out


S3 = (24, 24, 24)
Y3 = path((2, 3, 12), (12, 12, 12)) | path((22, 4, 10), (12, 12, 12)) | path((12, 22, 14), (12, 12, 12))
X3 = path((2, 2, 5), (21, 21, 5)) | path((2, 21, 6), (21, 2, 6))
V3 = path((3, 3, 3), (12, 12, 12), (20, 3, 12))
LINE3 = path((1, 2, 3), (22, 20, 15))
THICK3 = path((2, 4, 6), (20, 18, 9)) | shifted(path((2, 4, 6), (20, 18, 9)), (0, 1, 0))
RING3 = _ring((11, 12, 12), 8)
# a U-turn whose limbs are one empty row apart: inside one ball of radius 2 or 3, joined only at the far end
UTURN3 = path((6, 5, 3), (6, 5, 18)) | path((6, 7, 3), (6, 7, 18)) | {(6, 6, 18)}
BLOB3 = {(a, b, c) for a in range(8, 14) for b in range(8, 14) for c in range(8, 14)}
STUB3 = path((20, 20, 20), (20, 20, 22))


def shapes3d():
    """One shape per event; a stub too small to be eligible, a noise voxel with the id -1 and an empty event."""
    ev = [([(Y3, 1)], [(0, 0, 0)]), ([(X3, 1)], []), ([], []), ([(V3, 2)], []), ([(LINE3, 1), (STUB3, 1)], []), ([(THICK3, 1)], []),
          ([(RING3, 2)], []), ([(UTURN3, 1)], [(23, 23, 23)]), ([(BLOB3, 1)], [])]
    return batch(S3, ev)


def jacks():
    """Six arms from one centre: five arms and more.  At radius 3 the jack with arms of 5 has a junction of 13 entries: ``grow`` 6
    hands all of them to the arms, ``grow`` 1 only the outer six, and the seven left are a piece of kind 2; so is every junction
    with ``grow`` 0.  The jacks with arms of 2 are stubs at radius 3: no arm at the centre."""
    return batch(S3, [([(jack((6, 6, 6), 2), 1), (jack((16, 16, 16), 5), 1)], []), ([(jack((6, 6, 6), 2), 1)], [])])


S2 = (48, 40)
Y2 = path((3, 4), (20, 20)) | path((40, 6), (20, 20)) | path((22, 38), (20, 20))
X2 = path((2, 2), (39, 39)) | path((2, 39), (39, 2))
V2 = path((4, 4), (30, 20), (6, 36))
UTURN2 = path((5, 3), (30, 3)) | path((5, 5), (30, 5)) | {(30, 4)}
BLOB2 = {(a, b) for a in range(10, 20) for b in range(10, 20)}


def shapes2d():
    ev = [([(Y2, 1)], []), ([(X2, 1)], [(47, 39)]), ([(V2, 1)], []), ([], []), ([(path((1, 1), (46, 30)), 1)], []), ([(UTURN2, 2)], []),
          ([(BLOB2, 1)], []), ([(Y2, 1)], [])]                                       # the last: the first event's indices again
    return batch(S2, ev)


def frame3d():
    """The twelve edges of the volume: every ball is clipped, by every face somewhere, and the corners are junctions."""
    s = (9, 10, 11)
    cells = set()
    for a in range(3):
        for u in (0, s[(a + 1) % 3] - 1):
            for v in (0, s[(a + 2) % 3] - 1):
                for t in range(s[a]):
                    c = [0, 0, 0]
                    c[a], c[(a + 1) % 3], c[(a + 2) % 3] = t, u, v
                    cells.add(tuple(c))
    return batch(s, [([(cells, 1)], [])])


def frame2d():
    s = (12, 9)
    cells = {(a, b) for a in range(s[0]) for b in range(s[1]) if a in (0, s[0] - 1) or b in (0, s[1] - 1)} | path((0, 4), (11, 4))
    return batch(s, [([(cells, 1)], [])])


def wrap3d():
    """One row of two limbs: the first ends at the end of the list row (4, 4, .), the second begins the list row (4, 5, .), and their
    indices are consecutive.  Coordinates say they are 11 apart; index arithmetic alone would join them."""
    s = (8, 8, 12)
    a, b = path((4, 4, 3), (4, 4, 11)), {(4, 5, 0)} | path((5, 6, 1), (5, 7, 9))
    return batch(s, [([(a | b, 1)], [])])


def wrap2d():
    s = (10, 12)
    a, b = path((4, 2), (4, 11)), {(5, 0)} | path((6, 1), (9, 1))
    return batch(s, [([(a | b, 1)], [])])


def mixed():
    """Rows that are not eligible beside rows that are: a row of class 3 (classes (1, 2)), a row of two separate limbs below min_size
    that must stay whole, the same indices in neighbouring events, empty events first and last."""
    far = path((2, 2, 2), (2, 2, 5)) | path((20, 20, 20), (20, 20, 22))              # 7 voxels, two limbs, one row
    ev = [([], []), ([(Y3, 1), (far, 1)], [(0, 23, 0)]), ([(Y3, 3), (far, 2)], []), ([(Y3, 2), (shifted(LINE3, (1, 0, 2)), 3)], []), ([], [])]
    return batch(S3, ev)


def many():
    """1,117 entries in fifteen events: no multiple of 256 (a workgroup of the per-entry launches), of 64 (a tile) or of 4 (a
    workgroup of the wave form); five workgroups of the per-entry launches, 280 of the wave form."""
    ev = []
    for k in range(14):
        d = (k % 2, (k // 2) % 2, k % 3)
        ev.append(([(shifted(Y3, d), 1), (shifted(UTURN3, (12 - 2 * (k % 2), 8, 2)), 2)], []))
    ev.append(([(BLOB3, 1), (STUB3, 1)], [(0, 0, 1), (0, 2, 1)]))
    return batch(S3, ev)


CASES = {"shapes3d": shapes3d, "shapes2d": shapes2d, "jacks": jacks, "frame3d": frame3d, "frame2d": frame2d, "wrap3d": wrap3d,
         "wrap2d": wrap2d, "mixed": mixed, "many": many}


def case(name):
    if name not in _cache:
        c = CASES[name]()
        for v in c.values():
            if isinstance(v, np.ndarray):
                v.setflags(write=False)
        _cache[name] = c
    return _cache[name]


def statement(name, spec):
    """cluster_split_numpy of a case, computed once per (case, spec) and shared."""
    from uresnet_amd.clusters import cluster_split_numpy
    key = (name, repr(spec))
    if key not in _cache:
        c = case(name)
        _cache[key] = cluster_split_numpy(c["off"], c["index"], c["cluster"], c["toff"], c["size"], c["shape"], spec, c["cls"])
    return _cache[key]


def replicate(c, want, R):
    """The case R times over (R n events, every list unchanged) and its expected tables: positions (``key``, ``first_pos``) move
    with their replica, everything else is event-local."""
    tile = lambda a: np.tile(a, (R,) + (1,) * (a.ndim - 1))
    cum = lambda o: np.concatenate([[0], np.cumsum(np.tile(np.diff(o), R))]).astype(np.int64)
    m = int(c["off"][-1])
    big = {"shape": c["shape"], "off": cum(c["off"]), "toff": cum(c["toff"])}
    for k in ("index", "cluster", "first", "size", "cls"):
        big[k] = tile(c[k])
    out = {"split": tile(want["split"]), "mark": tile(want["mark"]), "piece_offsets": cum(want["piece_offsets"]),
           "junction_offsets": cum(want["junction_offsets"]), "rows": tile(want["rows"]), "events": tile(want["events"]),
           "table": {k: tile(v) for k, v in want["table"].items()},
           "pieces": {k: tile(v) for k, v in want["pieces"].items()}, "junctions": {k: tile(v) for k, v in want["junctions"].items()}}
    out["pieces"]["key"] = out["pieces"]["key"] + np.repeat(np.arange(R, dtype=np.int64) * m, want["pieces"]["key"].size)
    out["junctions"]["first_pos"] = out["junctions"]["first_pos"] + np.repeat(np.arange(R, dtype=np.int64) * m,
                                                                              want["junctions"]["first_pos"].size)
    return big, out
