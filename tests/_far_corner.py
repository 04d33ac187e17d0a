"""Voxel lists at the largest extents the voxel-list calls accept.  Plain helper module, not a conftest; importable
without a GPU.

Every call states "extents in [1, 32768], prod(spatial) < 2^31, indices are int32", and every kernel behind it turns an index into
coordinates and back.  The lists here are the case sets whose coverage the host tests of each call already assert, cropped to their
bounding box and moved, event by event, to where that arithmetic is at its bounds: against the far faces of a shape that has one
quantity at its cap (FAR), at the origin (ORIGIN), or across index 2^30 (MIDDLE).  Row-major order is lexicographic, so a
translation keeps every per-event list sorted and every event-local id what it was; the pure-Python statements are dict-based and
cost the same in any volume.  tests/test_far_corner_host.py proves that the statements are translation-equivariant outside
COORD_COLUMNS and that every batch reaches what it is named for; the GPU modules run the batches through their own _check."""
import collections
import functools

import numpy as np

import _chain_cases as chain_cases
import _cone_cases as cone_cases
import _split_cases as split_cases
from uresnet_amd import clusters as C

# ---- the shapes: each has one quantity at its bound ----------------------------------------------------------------------------
LARGEST_VOLUME = (2047, 1024, 1024)          # V = 2^31 - 2^20: the largest index is 2,146,435,071
AXIS0_CAP = (32768, 256, 255)                # axis 0 at its cap
AXIS1_CAP = (40, 32768, 1638)                # axis 1 at its cap
AXIS2_CAP = (255, 256, 32768)                # axis 2 at its cap: x-runs and % D2
LARGEST_PLANE = (2, 32768, 32767)            # D1 * D2 = 2^30 - 32768
SHAPES_3D = (LARGEST_VOLUME, AXIS0_CAP, AXIS1_CAP, AXIS2_CAP, LARGEST_PLANE)
CAPPED_2D = (32768, 32768)                   # the calls that cap extents
WIDEST_2D = (46340, 46340)                   # V = 2,147,395,600: the calls that only require V < 2^31
SHAPES_CAPPED = SHAPES_3D + (CAPPED_2D,)
SHAPES_VOLUME = SHAPES_3D + (CAPPED_2D, WIDEST_2D)           # ursn_cluster_voxels, the crop calls
CUBE = (1290, 1290, 1290)                    # V = 2,146,689,000: a cube, whose axes the symmetry remap may permute
MAX_EXTENT, MAX_VOLUME = 32768, 2 ** 31
LONG_TRACK = {0: AXIS0_CAP, 1: AXIS1_CAP, 2: AXIS2_CAP}      # the capped axis -> its shape

FAR, ORIGIN, MIDDLE = "far", "origin", "middle"
PLACEMENTS = (FAR, ORIGIN, MIDDLE)


def shape_id(shape):
    return "x".join(str(s) for s in shape)


def volume(shape):
    return int(np.prod(np.array(shape, np.int64)))


def pivot(shape):
    """The index a MIDDLE event straddles: 2^30 where the volume has indices on both sides of it, else the middle of the volume
    ((32768, 32768) ends at 2^30 - 1)."""
    V = volume(shape)
    return 2 ** 30 if V > 2 ** 30 + 2 ** 20 else V // 2


def coords(index, shape):
    """[m, ndim] int64 coordinates of a list."""
    index = np.asarray(index, np.int64)
    return np.stack(np.unravel_index(index, shape), axis=1).astype(np.int64).reshape(index.size, len(shape))


def ravel(x, shape):
    x = np.asarray(x, np.int64).reshape(-1, len(shape))
    assert x.size == 0 or ((x >= 0).all() and (x < np.array(shape, np.int64)).all()), "a coordinate outside the shape"
    out = np.zeros(x.shape[0], np.int64)
    for a, s in enumerate(shape):
        out = out * int(s) + x[:, a]
    return out


def crop(index, shape):
    """The list re-indexed into its bounding box: (index, box shape, the box's low corner)."""
    x = coords(index, shape)
    lo, hi = x.min(axis=0), x.max(axis=0)
    box = tuple(int(s) for s in hi - lo + 1)
    return ravel(x - lo, box), box, lo


def translate(off, index, small_shape, big_shape, shifts):
    """The batch re-indexed into ``big_shape``, event e moved by ``shifts[e]`` (one integer per axis)."""
    off = np.asarray(off, np.int64)
    shifts = np.asarray(shifts, np.int64).reshape(off.size - 1, len(small_shape))
    x = coords(index, small_shape) + np.repeat(shifts, np.diff(off), axis=0)
    out = ravel(x, big_shape)
    for e in range(off.size - 1):
        assert (np.diff(out[off[e]:off[e + 1]]) > 0).all()
    return out


def shift_for(placement, x, big_shape):
    """The shift that puts an event with coordinates ``x`` where ``placement`` says.  FAR: its bounding box against every far face,
    max(x_a) = S_a - 1.  ORIGIN: as it is.  MIDDLE: some entry as close to pivot(big_shape) as the faces allow, so that the event
    has entries below the pivot and entries at or above it; None where no shift does that."""
    big = np.array(big_shape, np.int64)
    lo, hi = x.min(axis=0), x.max(axis=0)
    assert (lo >= 0).all() and (hi < big).all(), "the event does not fit"
    if placement == ORIGIN:
        return np.zeros(len(big_shape), np.int64)
    if placement == FAR:
        return big - 1 - hi
    target = coords([pivot(big_shape)], big_shape)[0]
    for j in list(range(x.shape[0] // 2, x.shape[0])) + list(range(x.shape[0] // 2)):
        shift = np.clip(target - x[j], -lo, big - 1 - hi)
        index = ravel(x + shift, big_shape)
        if index.min() < pivot(big_shape) <= index.max():
            return shift
    return None                    # an event in one plane cannot straddle a pivot that lies on the edge of a plane


# ---- sources: lists with a clustering, in the frame they were made in ----------------------------------------------------------
# cls: per entry or None; tcls / size: per row of the cluster table
Source = collections.namedtuple("Source", "name shape off index value cls cluster toff size tcls")
SPEC_3D = C.ClusterSpec(26, (0, 1, 2), True, 2)       # the random lists: per class, class 0 included, pairs and more
SPEC_2D = C.ClusterSpec(8, (0, 1, 2), True, 2)


def _sizes(off, cluster, toff):
    ev = np.repeat(np.arange(off.size - 1), np.diff(off))
    row = np.where(cluster >= 0, cluster + toff[ev], -1)
    return np.bincount(row[row >= 0], minlength=int(toff[-1])).astype(np.int32)


def _source(name, shape, off, index, value, cls, cluster, toff, tcls, size=None, seed=0):
    off, toff, index, cluster = (np.asarray(a, np.int64) for a in (off, toff, index, cluster))
    if value is None:
        value = np.random.default_rng(1000 + seed).uniform(-3.0, 40.0, index.size)
    size = _sizes(off, cluster, toff) if size is None else np.asarray(size, np.int32)
    return Source(name, tuple(shape), off, index, np.asarray(value, np.float32), None if cls is None else np.asarray(cls, np.uint8),
                  cluster, toff, size, np.asarray(tcls, np.uint8))


def random_source(seed, shape, occupancy):
    """The recipe of the graph / vertex / profile modules' random lists: three events with an empty one between them, three
    classes, clustered per class."""
    rng = np.random.default_rng(seed)
    V = volume(shape)
    lists = [np.flatnonzero(rng.uniform(size=V) < p) for p in (occupancy, 2.0, occupancy / 2, occupancy)]
    lists[1] = np.zeros(0, np.int64)
    off = np.concatenate([[0], np.cumsum([a.size for a in lists])]).astype(np.int64)
    index = np.concatenate(lists)
    cls = rng.integers(0, 3, index.size).astype(np.uint8)
    value = rng.uniform(-3.0, 40.0, index.size).astype(np.float32)
    cluster, toff, tcls = chain_cases.ids_of(off, index, cls, shape, SPEC_3D if len(shape) == 3 else SPEC_2D)
    return _source("random%r" % (shape,), shape, off, index, value, cls, cluster, toff, tcls)


def _lift(s):
    """A 2-D source as one plane of a 3-D volume: the indices are the same numbers."""
    return s._replace(name=s.name + "_plane", shape=(1,) + s.shape)


def _chain_source(name):
    off, index, value, cluster, toff, tcls = chain_cases.fixture(name)[:6]
    return _source("chain_" + name, chain_cases.FIXTURES[name][0], off, index, value, None, cluster, toff, tcls)


def _scene_source(name, shape, lists, seed):
    off, index, ids, toff, tcls = lists
    return _source(name, shape, off, index, None, None, ids, toff, tcls, seed=seed)


def _cone_source(name, seed):
    shape, lists, _, _ = cone_cases.named(name)
    return _scene_source("cone_" + name, shape, lists, seed)


def _split_source(name):
    c = split_cases.case(name)
    return _source("split_" + name, c["shape"], c["off"], c["index"], None, None, c["cluster"], c["toff"], c["cls"], c["size"])


@functools.lru_cache(maxsize=None)
def sources(family, ndim):
    """The sources of a family of calls: 'random' (clusters, features, graph, profile, vertices), 'chain', 'cone', 'split'."""
    if family == "random":
        if ndim == 2:
            return (random_source(11, (20, 24), 0.3),)
        return (random_source(9, (24, 20, 28), 0.04), random_source(10, (2, 24, 28), 0.2))
    if family == "chain":
        if ndim == 2:
            return (_chain_source("flat"),)
        return tuple(_chain_source(k) for k in ("angles", "long", "value")) + (
            _scene_source("chain_ring", (16, 32, 32), chain_cases.ring()[0], 1), _scene_source("chain_line", (8, 8, 64), chain_cases.line()[0], 2),
            _lift(_chain_source("flat")))
    if family == "cone":
        flat = _cone_source("flat", 3)
        if ndim == 2:
            return (flat,)
        off, index, cluster, toff, tcls = cone_cases.toys()[:5]
        toys = _source("cone_toys", cone_cases.TOY_SHAPE, off, index, None, None, cluster, toff, tcls, seed=4)
        return tuple(_cone_source(k, 10 + i) for i, k in enumerate(sorted(cone_cases.SCENES)) if k != "flat") + (toys, _lift(flat))
    assert family == "split", family
    if ndim == 2:
        return tuple(_split_source(k) for k in ("shapes2d", "frame2d", "wrap2d"))
    # every 3-D case but 'many', which is there for the launch multiples of its 1,117 entries (DESIGN.md 1d's axis, not this one)
    return tuple(_split_source(k) for k in ("shapes3d", "jacks", "frame3d", "wrap3d", "mixed")) + (_lift(_split_source("shapes2d")),)


# ---- batches -------------------------------------------------------------------------------------------------------------------
# small / big: Source in the small frame (every source cropped to its bounding box, at the origin of a shape that holds them all)
# and in the big shape; shifts [n, ndim]: big coordinates minus small coordinates per event; placement: per event, None = empty
FarBatch = collections.namedtuple("FarBatch", "small big shifts placement")


def fits(s, big_shape):
    return len(s.shape) == len(big_shape) and all(b <= S for b, S in zip(crop(s.index, s.shape)[1], big_shape))


@functools.lru_cache(maxsize=None)
def far_batch(family, big_shape, rotate=0):
    """Every source of the family whose bounding box fits ``big_shape``, concatenated into one batch; the non-empty events of every
    source take FAR, ORIGIN, MIDDLE in turn (started ``rotate`` further on), so event bits and large indices meet in one packed key
    and every source has an event in the far corner."""
    used = [s for s in sources(family, len(big_shape)) if fits(s, big_shape)]
    assert used, (family, big_shape)
    boxes = [crop(s.index, s.shape) for s in used]
    small_shape = tuple(int(max(b[1][a] for b in boxes)) for a in range(len(big_shape)))
    small_index, big_index, shifts, placement = [], [], [], []
    for s, (index, box, _) in zip(used, boxes):
        x = coords(index, box)
        k = rotate
        for e in range(s.off.size - 1):
            xe = x[s.off[e]:s.off[e + 1]]
            if xe.shape[0] == 0:
                shifts.append(np.zeros(len(big_shape), np.int64)), placement.append(None)
                continue
            where = PLACEMENTS[k % 3] if xe.shape[0] > 1 else FAR
            k += 1
            shift = shift_for(where, xe, big_shape)
            if shift is None:
                where, shift = FAR, shift_for(FAR, xe, big_shape)
            shifts.append(shift), placement.append(where)
            small_index.append(ravel(xe, small_shape)), big_index.append(ravel(xe + shifts[-1], big_shape))
    cat = lambda parts: np.concatenate(parts)
    cum = lambda parts: np.concatenate([[0], np.cumsum(cat([np.diff(p) for p in parts]))]).astype(np.int64)
    cls = None if used[0].cls is None else cat([s.cls for s in used])
    made = dict(name="%s@%s" % (family, shape_id(big_shape)), off=cum([s.off for s in used]), value=cat([s.value for s in used]), cls=cls,
                cluster=cat([s.cluster for s in used]), toff=cum([s.toff for s in used]), size=cat([s.size for s in used]),
                tcls=cat([s.tcls for s in used]))
    small = Source(shape=small_shape, index=cat(small_index), **made)
    big = Source(shape=tuple(big_shape), index=cat(big_index), **made)
    for a in small + big:
        if isinstance(a, np.ndarray):
            a.setflags(write=False)
    return FarBatch(small, big, np.array(shifts, np.int64), tuple(placement))


@functools.lru_cache(maxsize=None)
def clustered(family, big_shape, connectivity, same_class, min_size=1):
    """Another clustering of a batch's lists (they need per-entry classes: the 'random' family): (cluster, toff, tcls), computed in
    the small frame -- ids are event-local and translation keeps them, which tests/test_far_corner_host.py proves."""
    s = far_batch(family, big_shape).small
    return chain_cases.ids_of(s.off, s.index, s.cls, s.shape, C.ClusterSpec(connectivity, (0, 1, 2), same_class, min_size))


def split_case(s):
    """A Source as the dict tests/_split_cases.py hands out."""
    return {"shape": s.shape, "off": s.off, "index": s.index, "cluster": s.cluster, "toff": s.toff, "size": s.size, "cls": s.tcls}


# ---- the long track --------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def long_track(shape, drift=None):
    """One 26-connected staircase of 32,768 entries spanning the capped axis of ``shape`` end to end, drifting across the other two
    axes and ending in the far corner: coordinate t on the capped axis, S_b - 1 - drift_b + (t * drift_b) // 32767 on the others,
    drift_b = S_b - 1 (it starts in the origin corner) or the given ``drift``.  One event, every entry of class 1, one cluster.
    Returns a Source."""
    axis = [a for a, s in enumerate(shape) if s == MAX_EXTENT]
    assert len(axis) == 1 and len(shape) == 3, shape
    t = np.arange(MAX_EXTENT, dtype=np.int64)
    by = [shape[a] - 1 if drift is None else min(int(drift), shape[a] - 1) for a in range(3)]
    x = np.stack([t if a == axis[0] else shape[a] - 1 - by[a] + (t * by[a]) // (MAX_EXTENT - 1) for a in range(3)], axis=1)
    assert (np.abs(np.diff(x, axis=0)) <= 1).all() and (x[-1] == np.array(shape) - 1).all() and (drift is not None or (x[0] == 0).all())
    index = np.sort(ravel(x, shape))
    M = index.size
    s = _source("long_track@%s" % shape_id(shape), shape, [0, M], index, None, np.ones(M, np.uint8), np.zeros(M, np.int64), [0, 1], [1],
                seed=axis[0])
    for a in s:
        if isinstance(a, np.ndarray):
            a.setflags(write=False)
    return s


# ---- the statements, flattened to {"table.column": array} ------------------------------------------------------------------------
_NAMES = {"graph": {"edges": C.GRAPH_EDGE, "rows": C.GRAPH_ROW, "groups": C.GRAPH_GROUP, "events": C.GRAPH_EVENT},
          "vertex": {"incidence": C.VERTEX_INCIDENCE, "events": C.VERTEX_EVENT}, "chain": {"events": C.CHAIN_EVENT},
          "cone": {"events": C.CONE_EVENT}, "split": {"rows": C.SPLIT_ROW, "events": C.SPLIT_EVENT}}

WIDEST = {"graph": C.ClusterGraphSpec(3), "profile": C.ClusterProfileSpec(0.5, 16, 65536), "vertex": C.ClusterVertexSpec(3, 2),
          "chain": C.ClusterChainSpec(31, 0.7, 2, None, True), "cone": C.ClusterConeSpec(127, 0.7, 8, 1, None, True),
          "split": C.ClusterSplitSpec(3, -0.7, 8)}


def statement(family, s, spec=None):
    """The statement of a family on a Source, as its own (nested) result."""
    spec = WIDEST.get(family) if spec is None else spec
    if family == "cluster":
        from _long_lists import Batch, cluster_statement
        return cluster_statement(Batch(s.shape, s.off, s.index, s.cls, s.value), spec)
    if family == "features":
        return C.cluster_features_numpy(s.off, s.index, s.value, s.cluster, s.toff, s.shape)
    if family == "graph":
        return C.cluster_graph_numpy(s.off, s.index, s.cluster, s.toff, s.shape, spec, s.value, s.tcls)
    if family == "profile":
        return C.cluster_profile_numpy(s.off, s.index, s.value, s.cluster, s.toff, s.shape, spec)
    if family == "vertex":
        return C.cluster_vertices_numpy(s.off, s.index, s.value, s.cluster, s.toff, s.shape, spec, s.tcls)
    if family == "chain":
        return C.cluster_chains_numpy(s.off, s.index, s.value, s.cluster, s.toff, s.shape, spec, s.tcls)
    if family == "cone":
        return C.cluster_cones_numpy(s.off, s.index, s.value, s.cluster, s.toff, s.shape, spec, s.tcls)
    assert family == "split", family
    return C.cluster_split_numpy(s.off, s.index, s.cluster, s.toff, s.size, s.shape, spec, s.tcls)


def flatten(family, want):
    """{"table.column": array}: nested tables by their keys, the 2-D integer tables by their column names."""
    out = {}
    for k, v in want.items():
        if isinstance(v, dict):
            for name, a in v.items():
                out["%s.%s" % (k, name)] = a
        elif k in _NAMES.get(family, {}):
            for c, name in enumerate(_NAMES[family][k]):
                out["%s.%s" % (k, name)] = v[:, c]
        else:
            out[k] = v
    return out


# ---- the columns that are positions ------------------------------------------------------------------------------------------------
# column -> (kind, what its rows are counted by): kind 'pos' = moves by the event's shift on its axis (the column's last digit, or
# its position in a [K, 3] column); 'sum' = by the shift times the named count column; 'real' = an fp64 / fp32 position, equal to
# within rounding of anchor + sum / n; 'free' = the three fp64 profile columns that are formed from such positions and round with
# them.  The rows of a table belong to events through the named offsets array: per event ([n + 1]) or per cluster row ([K + 1]).
_OBJECT = {"s": ("sum", "n"), "lo": ("pos", None), "hi": ("pos", None), "m": ("pos", None), "centroid": ("real", None)}
_BOX = {"%s%d" % (k, a): ("pos", None) for k in ("lo", "hi") for a in range(3)}
_SUMS = lambda n: {"s%d" % a: ("sum", n) for a in range(3)}
_REAL = {"c%d" % a: ("real", None) for a in range(3)}


def _table(prefix, columns):
    return {prefix + k: v for k, v in columns.items()}


COORD_COLUMNS = {
    "cluster": {},
    "features": dict(_OBJECT),
    "graph": _table("groups.", _BOX),
    "profile": dict(_table("objects.", _OBJECT), **_table("bins.", _REAL),
                    **{"rows.path": ("free", None), "rows.min_cos": ("free", None), "rows.straightness": ("free", None)}),
    "vertex": dict(_table("objects.", _OBJECT), **_table("vertices.", dict(_BOX, **_SUMS("ends"), **_REAL))),
    "chain": dict(_table("objects.", _OBJECT), **_table("chains.", _BOX)),
    "cone": dict(_table("objects.", _OBJECT), **_table("showers.", _BOX)),
    "split": _table("junctions.", dict(_BOX, **_SUMS("entries"), **_REAL)),
}
# table prefix -> (offsets key, 'event' or 'row'); '' = the tables of the features statement itself
ROW_EVENTS = {
    "features": {"": ("toff", "event")},
    "graph": {"groups": ("group_offsets", "event")},
    "profile": {"objects": ("toff", "event"), "bins": ("bin_offsets", "row"), "rows": ("toff", "event")},
    "vertex": {"objects": ("toff", "event"), "vertices": ("vertex_offsets", "event")},
    "chain": {"objects": ("toff", "event"), "chains": ("chain_offsets", "event")},
    "cone": {"objects": ("toff", "event"), "showers": ("shower_offsets", "event")},
    "split": {"junctions": ("junction_offsets", "event")},
}


def event_of_rows(family, column, want, toff):
    """The event of every row of the table ``column`` lives in."""
    prefix = column.rsplit(".", 1)[0] if "." in column else ""
    key, per = ROW_EVENTS[family][prefix]
    offsets = np.asarray(toff if key == "toff" else want[key], np.int64)
    owner = np.repeat(np.arange(offsets.size - 1), np.diff(offsets))
    if per == "row":
        owner = np.repeat(np.arange(toff.size - 1), np.diff(toff))[owner]
    return owner


# ---- the symmetry remap in closed form ---------------------------------------------------------------------------------------------
def remap_closed_form(index, shape, perm, flip):
    """o[a] = f_a(i[perm[a]]) with f_a(x) = S_a - 1 - x where flip[a], in Python integers: where the voxel with this index goes
    when the volume is transposed by ``perm`` and then flipped on the axes ``flip``.  Indices outside the volume pass through."""
    nd = len(shape)
    out = []
    V = volume(shape)
    for i in (int(v) for v in index):
        if not 0 <= i < V:
            out.append(i)
            continue
        x, r = [0] * nd, i
        for a in range(nd - 1, -1, -1):
            r, x[a] = divmod(r, int(shape[a]))
        o = [x[perm[a]] for a in range(nd)]
        o = [int(shape[a]) - 1 - o[a] if flip[a] else o[a] for a in range(nd)]
        k = 0
        for a in range(nd):
            k = k * int(shape[a]) + o[a]
        out.append(k)
    return np.array(out, np.int64)
