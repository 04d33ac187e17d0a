"""Voxel clusters: connected components of the predicted voxels of an event's list (csrc/cluster.hip does it on the device; this
file holds the specification and its numpy / pure-Python statement, the yardstick of the tests).

An entry of a sorted per-event index list PARTICIPATES when its index lies in ``[0, prod(spatial))`` and its class is one of
``spec.classes`` (None: every class but 0).  Two participating entries are joined when their coordinates differ by at most 1 on
every axis and in at most 1 / 2 / 3 axes -- connectivity 6 / 18 / 26 in 3-D, 1 / 2 axes = 4 / 8 in 2-D -- and, with
``same_class``, have equal class.  Clusters are the connected components with at least ``min_size`` entries, numbered in the order
of their lowest list position (``scipy.ndimage.label``'s numbering for a raster-ordered list); every other entry gets -1."""
import numpy as np

CONNECTIVITY = {2: (4, 8), 3: (6, 18, 26)}
_ON = ('pred', 'ana')


class ClusterSpec(object):
    """``connectivity`` None = 26 in 3-D and 8 in 2-D (resolved against the shape by ``axes``); ``classes`` None = every class but
    0, else an iterable of class numbers in [0, 32); ``same_class`` True = only entries of equal class join; ``min_size`` >= 1 =
    smaller components are dropped and not numbered; ``on`` = which class array of the inference calls is clustered."""

    def __init__(self, connectivity=None, classes=None, same_class=True, min_size=1, on='pred'):
        if connectivity is not None and (type(connectivity) is not int or connectivity not in (4, 8, 6, 18, 26)):
            raise ValueError('ClusterSpec: connectivity = %r, expected None, 4 or 8 (2-D), 6, 18 or 26 (3-D)' % (connectivity,))
        if classes is not None:
            classes = tuple(classes)
            if any(type(c) is not int or not 0 <= c < 32 for c in classes) or len(set(classes)) != len(classes):
                raise ValueError('ClusterSpec: classes = %r, expected None or distinct integers in [0, 32)' % (classes,))
        if type(same_class) is not bool:
            raise ValueError('ClusterSpec: same_class = %r, expected a bool' % (same_class,))
        if type(min_size) is not int or not 1 <= min_size < 2 ** 31:
            raise ValueError('ClusterSpec: min_size = %r, expected an integer >= 1' % (min_size,))
        if on not in _ON:
            raise ValueError("ClusterSpec: on = %r, expected 'pred' or 'ana'" % (on,))
        self.connectivity, self.classes, self.same_class, self.min_size, self.on = connectivity, classes, same_class, min_size, on

    def axes(self, ndim):
        """(connectivity, axes in which two joined entries may differ) for a shape of ``ndim`` axes."""
        if ndim not in CONNECTIVITY:
            raise ValueError('ClusterSpec: %d spatial axes, expected 2 or 3' % ndim)
        c = CONNECTIVITY[ndim][-1] if self.connectivity is None else self.connectivity
        if c not in CONNECTIVITY[ndim]:
            raise ValueError('ClusterSpec: connectivity %d is not one of %r for %d spatial axes' % (c, CONNECTIVITY[ndim], ndim))
        return c, CONNECTIVITY[ndim].index(c) + 1

    def class_mask(self):
        """Bit k set = class k participates."""
        if self.classes is None:
            return 0xFFFFFFFE
        m = 0
        for c in self.classes:
            m |= 1 << c
        return m

    def __repr__(self):
        return 'ClusterSpec(connectivity=%r, classes=%r, same_class=%r, min_size=%r, on=%r)' % (
            self.connectivity, self.classes, self.same_class, self.min_size, self.on)


def cluster_numpy(index, cls, spatial, spec):
    """The statement: a union-find over a position dict (coordinates -> list position), links to the lower position, ids by lowest
    position.  ``index`` int [m] sorted, ``cls`` int [m].  Returns ``(cluster int32 [m], first int32 [K], size int32 [K],
    cls uint8 [K])``; ``first`` is a list position."""
    index = np.asarray(index, np.int64).reshape(-1)
    cls = np.asarray(cls).reshape(-1)
    spatial = tuple(int(s) for s in spatial)
    if index.shape != cls.shape:
        raise ValueError('cluster_numpy: %d indices, %d classes' % (index.size, cls.size))
    _, axes = spec.axes(len(spatial))
    mask, vox, m = spec.class_mask(), int(np.prod(spatial, dtype=np.int64)), index.size
    part = (index >= 0) & (index < vox) & np.array([0 <= int(c) < 32 and (mask >> int(c)) & 1 == 1 for c in cls], bool)
    coords = np.stack(np.unravel_index(np.where(part, index, 0), spatial), axis=1) if m else np.zeros((0, len(spatial)), np.int64)
    where = {tuple(int(x) for x in coords[j]): j for j in range(m) if part[j]}
    steps = [d for d in np.ndindex(*([3] * len(spatial))) if 0 < sum(1 for x in d if x != 1) <= axes]
    parent = list(range(m))

    def find(x):
        while parent[x] != x:
            parent[x] = parent[parent[x]]
            x = parent[x]
        return x

    for j in range(m):
        if not part[j]:
            continue
        for d in steps:
            q = where.get(tuple(int(coords[j][a]) + d[a] - 1 for a in range(len(spatial))))
            if q is None or q > j or (spec.same_class and cls[q] != cls[j]):
                continue
            a, b = find(j), find(q)
            if a != b:
                parent[max(a, b)] = min(a, b)
    root = np.array([find(j) if part[j] else -1 for j in range(m)], np.int64)
    sizes = np.bincount(root[root >= 0], minlength=max(m, 1))
    first = np.array([j for j in range(m) if part[j] and root[j] == j and sizes[j] >= spec.min_size], np.int64)
    ids = np.full(max(m, 1), -1, np.int64)
    ids[first] = np.arange(first.size)
    cluster = np.where(root >= 0, ids[np.maximum(root, 0)], -1).astype(np.int32) if m else np.zeros(0, np.int32)
    return cluster, first.astype(np.int32), sizes[first].astype(np.int32), cls[first].astype(np.uint8)
