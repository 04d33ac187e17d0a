"""Tiled inference and crop training for volumes larger than the network, host side: the box grid, pseudo-random training crops,
and the numpy statement of the three device passes of csrc/tiling.hip (``ursn_crop_count`` / ``ursn_crop_write`` /
``ursn_scores_scatter``, include/uresnet_hip.h) -- the definition the device is tested against.

A box covers ``0 <= x[a] - origin[a] < tile[a]`` of one large event; its core, ``core_lo[a] <= x[a] - origin[a] < core_hi[a]`` in
box-local coordinates, is the part whose voxels the box owns.  Not in the reference, whose network and events share one size."""
import numpy as np


class Boxes(object):
    """B boxes of one tile size: ``event`` int32 [B], ``origin`` int32 [B, ndim], ``core_lo`` / ``core_hi`` int32 [B, ndim] in
    box-local coordinates or both None (every box owns all of itself).  Mirrors the box arrays of ``ursn_crop_desc``."""

    __slots__ = ('event', 'origin', 'core_lo', 'core_hi')

    def __init__(self, event, origin, core_lo=None, core_hi=None):
        self.event = np.ascontiguousarray(event, dtype=np.int32).reshape(-1)
        self.origin = np.ascontiguousarray(origin, dtype=np.int32).reshape(self.event.shape[0], -1)
        if (core_lo is None) != (core_hi is None):
            raise ValueError('Boxes: core_lo and core_hi must be given together')
        self.core_lo = None if core_lo is None else np.ascontiguousarray(core_lo, dtype=np.int32).reshape(self.origin.shape)
        self.core_hi = None if core_hi is None else np.ascontiguousarray(core_hi, dtype=np.int32).reshape(self.origin.shape)

    def __len__(self):
        return int(self.event.shape[0])

    @property
    def ndim(self):
        return int(self.origin.shape[1])

    def select(self, keep):
        """The boxes ``keep`` names (an index array, a boolean mask or a slice), in that order."""
        return Boxes(self.event[keep], self.origin[keep], None if self.core_lo is None else self.core_lo[keep],
                     None if self.core_hi is None else self.core_hi[keep])


def _shapes(big, tile):
    big, tile = tuple(int(s) for s in big), tuple(int(t) for t in tile)
    if len(big) not in (2, 3) or len(tile) != len(big):
        raise ValueError('tiling: big = %r and tile = %r must both have 2 or 3 axes' % (big, tile))
    if min(big) < 1 or min(tile) < 1:
        raise ValueError('tiling: big = %r / tile = %r: every extent must be >= 1' % (big, tile))
    if int(np.prod(big, dtype=np.int64)) >= 2 ** 31 or int(np.prod(tile, dtype=np.int64)) >= 2 ** 31:
        raise ValueError('tiling: prod(big) and prod(tile) must stay below 2^31 (indices are int32)')
    return big, tile


def axis_grid(S, T, halo):
    """One axis of ``grid``: (origins, core_lo, core_hi), the cores in GLOBAL coordinates."""
    S, T, halo = int(S), int(T), int(halo)
    if halo < 0 or T - 2 * halo < 1:
        raise ValueError('tiling.grid: halo = %d leaves no stride in a tile of %d' % (halo, T))
    if S <= T:
        return [0], [0], [S]
    s = T - 2 * halo
    origins = list(range(0, S - T, s)) + [S - T]
    cuts = [0] + [(b + a + T) // 2 for a, b in zip(origins[:-1], origins[1:])] + [S]   # midpoint of the overlap [b, a + T)
    return origins, cuts[:-1], cuts[1:]


def grid(big, tile, halo, n=1):
    """The boxes of a tiled analysis of ``n`` events of shape ``big`` with a network of shape ``tile``.  Per axis the origins are
    ``0, s, 2 s, ... < S - T`` followed by ``S - T`` with the stride ``s = T - 2 * halo`` (``S <= T``: the single origin 0).  The
    core boundaries lie at the midpoint of the overlap of neighbouring boxes, 0 at the first box and ``S`` at the last, so the cores
    partition the volume and each lies inside its box.  Boxes come event by event, in row-major order of the grid."""
    big, tile = _shapes(big, tile)
    halos = [int(halo)] * len(big) if np.isscalar(halo) else [int(h) for h in halo]
    axes = [axis_grid(S, T, h) for S, T, h in zip(big, tile, halos)]
    mesh = np.meshgrid(*[np.arange(len(a[0])) for a in axes], indexing='ij')
    pick = [m.reshape(-1) for m in mesh]
    origin = np.stack([np.asarray(a[0], np.int64)[p] for a, p in zip(axes, pick)], axis=1)
    lo = np.stack([np.asarray(a[1], np.int64)[p] for a, p in zip(axes, pick)], axis=1) - origin
    hi = np.stack([np.asarray(a[2], np.int64)[p] for a, p in zip(axes, pick)], axis=1) - origin
    n, per = int(n), origin.shape[0]
    return Boxes(np.repeat(np.arange(n), per), np.tile(origin, (n, 1)), np.tile(lo, (n, 1)), np.tile(hi, (n, 1)))


def random_boxes(seed, vb, big, tile):
    """Training crops: one box per event of ``vb`` (a VoxelBatch at ``prod(big)``), centred on a pseudo-randomly chosen listed
    voxel with a jitter of up to a quarter tile per axis, then moved back inside the volume where the volume is at least a tile
    wide (origin 0 where it is not).  A pure function of its arguments (numpy's PCG64 seeded with ``(seed, event)``; ``seed`` is a
    non-negative integer or a sequence of them); an event
    with no voxels gets origin 0.  The boxes have no cores: a crop owns all of itself."""
    big, tile = _shapes(big, tile)
    origin = np.zeros((vb.n, len(big)), np.int64)
    seeds = [int(seed)] if np.isscalar(seed) else [int(x) for x in seed]
    for e in range(vb.n):
        a, b = int(vb.offsets[e]), int(vb.offsets[e + 1])
        if b <= a:
            continue
        rng = np.random.default_rng(seeds + [e])
        centre = np.unravel_index(int(vb.index[a + int(rng.integers(b - a))]), big)
        for ax, (S, T) in enumerate(zip(big, tile)):
            o = int(centre[ax]) - T // 2 + int(rng.integers(-(T // 4), T // 4 + 1))
            origin[e, ax] = min(max(o, 0), S - T) if S >= T else 0
    return Boxes(np.arange(vb.n), origin)


def crop_numpy(vb, big, tile, boxes):
    """The count and write passes: ``(crop, src, owned, count, owned_count)``.  ``crop`` is a VoxelBatch at ``prod(tile)`` voxels
    with one event per box: the entries of event ``boxes.event[b]`` that lie inside box b, in list order, with box-local row-major
    indices (subtracting the origin keeps the order, so they are strictly increasing); value / label / weight gathered where
    ``vb`` has them, ``bg_weight[b] = vb.bg_weight[event]``.  ``src`` int32 [m]: the position of each entry in ``vb``'s list;
    ``owned`` uint8 [m]: 1 inside the box's core; ``count`` / ``owned_count`` int64 [B].  A box of an event outside [0, n) is
    empty and gets bg_weight 0."""
    from .ssnet import VoxelBatch
    big, tile = _shapes(big, tile)
    nd = len(big)
    if boxes.ndim != nd:
        raise ValueError('crop_numpy: boxes of %d axes for a volume of %d' % (boxes.ndim, nd))
    B = len(boxes)
    T = np.asarray(tile, np.int64)
    srcs, owns, idxs = [], [], []
    count, owned_count = np.zeros(B, np.int64), np.zeros(B, np.int64)
    bg = None if vb.bg_weight is None else np.zeros(B, np.float32)
    for b in range(B):
        e = int(boxes.event[b])
        if not 0 <= e < vb.n:
            continue
        lo, hi = int(vb.offsets[e]), int(vb.offsets[e + 1])
        if bg is not None:
            bg[b] = vb.bg_weight[e]
        coords = np.stack(np.unravel_index(vb.index[lo:hi].astype(np.int64), big), axis=1) if hi > lo else np.zeros((0, nd), np.int64)
        local = coords - boxes.origin[b].astype(np.int64)
        inside = np.all((local >= 0) & (local < T), axis=1)
        core = inside if boxes.core_lo is None else \
            inside & np.all((local >= boxes.core_lo[b]) & (local < boxes.core_hi[b]), axis=1)
        keep = np.flatnonzero(inside)
        srcs.append(lo + keep)
        owns.append(core[keep].astype(np.uint8))
        idxs.append(np.ravel_multi_index(tuple(local[keep].T), tile) if keep.size else np.zeros(0, np.int64))
        count[b], owned_count[b] = keep.size, int(core.sum())
    src = np.concatenate(srcs).astype(np.int32) if srcs else np.zeros(0, np.int32)
    owned = np.concatenate(owns).astype(np.uint8) if owns else np.zeros(0, np.uint8)
    index = np.concatenate(idxs).astype(np.int32) if idxs else np.zeros(0, np.int32)
    offsets = np.zeros(B + 1, np.int64)
    np.cumsum(count, out=offsets[1:])
    take = lambda a: None if a is None else a[src]
    crop = VoxelBatch(offsets, index, vb.value[src], take(vb.label), take(vb.weight), bg if vb.weight is not None else None,
                      int(np.prod(tile)))
    return crop, src, owned, count, owned_count


def stitch_numpy(out, src, owned, **rows):
    """The scatter: for every named array of ``rows`` (the gather head's ``scores`` [m, C], ``pred`` [m], ``ana`` [m] of one crop
    batch), ``out[name][src[j]] = rows[name][j]`` for the rows with ``owned[j] == 1``; every other row of ``out`` (arrays laid out
    in the large batch's list order) stays as it is.  Returns ``out``."""
    src, sel = np.asarray(src), np.asarray(owned) == 1
    for name, a in rows.items():
        if a is not None:
            out[name][src[sel]] = np.asarray(a)[sel]
    return out
