"""Loss weights as a function of the label alone (not in the reference, which reads them as a stored larcv product,
config/input_train3d.cfg: Tensor3DProducer "weight"): per-event class balance plus a category of its own for the voxels where two
foreground classes meet.  ``WeightSpec`` names the variant, ``make_weights_numpy`` is the numpy statement of the definition that
``ursn_make_weights`` (include/uresnet_hip.h, csrc/make_weights.hip) computes on the device, bit for bit.

For voxel v of event e, with ``ncls`` classes, radius r, ``scale[ncls + 1]``:

* class: ``c(v) = int(label[v])`` (truncation, like the loss head) if ``-1 < label[v] < ncls``, else none (NaN included);
* boundary: r >= 1, c(v) >= 1 and some u != v inside the event's volume with ``max_i |u_i - v_i| <= r``, c(u) >= 1, c(u) != c(v);
* category: ``k(v) = ncls`` for a boundary voxel, else c(v); ``counts[e, k]`` = voxels of event e in category k;
* weight: ``'class'``: ``scale[k(v)]``; ``'invfreq'``: ``float32(float64(scale[k(v)]) / float64(counts[e, k(v)]))``; none voxels 0.

With r = 0, ``'invfreq'`` and all-ones scale this is what ``synthetic_io.lartpc_sparse`` computes with ``np.bincount``.
"""
import itertools
import math

import numpy as np

MODES = ('class', 'invfreq')      # the library's URSN_WEIGHTS_CLASS = 0, URSN_WEIGHTS_INVFREQ = 1
MAX_RADIUS = 3
MAX_CLASSES = 8


class WeightSpec(object):
    """``mode`` 'class' | 'invfreq'; ``radius`` 0..3 (0: no boundary category); ``scale`` None (all ones) or ``num_class + 1``
    finite numbers: one per class, then the boundary category's."""

    __slots__ = ('mode', 'radius', 'scale')

    def __init__(self, mode='invfreq', radius=0, scale=None):
        if mode not in MODES:
            raise ValueError('WeightSpec: mode = %r, expected one of %r' % (mode, MODES))
        if isinstance(radius, bool) or not isinstance(radius, (int, np.integer)) or not 0 <= int(radius) <= MAX_RADIUS:
            raise ValueError('WeightSpec: radius = %r, expected an integer in [0, %d]' % (radius, MAX_RADIUS))
        if scale is not None:
            try:
                scale = tuple(float(s) for s in scale)
            except (TypeError, ValueError):
                raise ValueError('WeightSpec: scale = %r, expected None or a sequence of numbers' % (scale,))
            if not 2 <= len(scale) <= MAX_CLASSES + 1:
                raise ValueError('WeightSpec: scale has %d entries, expected num_class + 1 in [2, %d]' % (len(scale), MAX_CLASSES + 1))
            if not all(math.isfinite(s) for s in scale):
                raise ValueError('WeightSpec: scale = %r holds a non-finite value' % (scale,))
        self.mode, self.radius, self.scale = mode, int(radius), scale

    def mode_code(self):
        return MODES.index(self.mode)

    def scales(self, num_class):
        """The ``num_class + 1`` scales as float32 (what the device reads)."""
        if not 1 <= int(num_class) <= MAX_CLASSES:
            raise ValueError('WeightSpec: num_class = %r outside [1, %d]' % (num_class, MAX_CLASSES))
        if self.scale is None:
            return np.ones(int(num_class) + 1, np.float32)
        if len(self.scale) != int(num_class) + 1:
            raise ValueError('WeightSpec: scale has %d entries for %d classes (num_class + 1 expected)' % (len(self.scale), num_class))
        with np.errstate(over='ignore'):
            s = np.asarray(self.scale, np.float64).astype(np.float32)
        if not np.all(np.isfinite(s)):
            raise ValueError('WeightSpec: scale = %r is not finite in float32' % (self.scale,))
        return s

    def __repr__(self):
        return 'WeightSpec(mode=%r, radius=%d, scale=%r)' % (self.mode, self.radius, self.scale)


def make_weights_numpy(label, spatial, num_class, spec):
    """``label`` [n, voxels] (or [n, *spatial]) -> (weight float32 [n, voxels], counts int64 [n, num_class + 1])."""
    sp = tuple(int(s) for s in spatial)
    nd, ncls, r = len(sp), int(num_class), spec.radius
    if nd not in (2, 3):
        raise ValueError('make_weights_numpy: %d spatial extents, expected 2 or 3' % nd)
    V = int(np.prod(sp))
    L = np.asarray(label, np.float32).reshape((-1,) + sp)
    n = L.shape[0]
    scale = spec.scales(ncls)
    with np.errstate(invalid='ignore'):
        ok = (L > -1) & (L < ncls)
    c = np.where(ok, np.where(ok, L, 0).astype(np.int64), -1)      # astype truncates toward zero; -1 = none
    fg = c >= 1
    bnd = np.zeros(c.shape, bool)
    if r >= 1:
        pad = np.pad(c, [(0, 0)] + [(r, r)] * nd, constant_values=-1)      # outside the volume: never a neighbour
        for off in itertools.product(range(2 * r + 1), repeat=nd):
            if all(o == r for o in off):
                continue
            u = pad[(slice(None),) + tuple(slice(o, o + s) for o, s in zip(off, sp))]
            bnd |= fg & (u >= 1) & (u != c)
    k = np.where(bnd, ncls, c).reshape(n, V)
    counts = np.zeros((n, ncls + 1), np.int64)
    weight = np.zeros((n, V), np.float32)
    for e in range(n):
        has = k[e] >= 0
        counts[e] = np.bincount(k[e][has], minlength=ncls + 1)
        if spec.mode == 'class':
            table = scale
        else:
            table = np.zeros(ncls + 1, np.float32)
            some = counts[e] > 0
            table[some] = (scale[some].astype(np.float64) / counts[e][some].astype(np.float64)).astype(np.float32)
        weight[e][has] = table[k[e][has]]
    return weight, counts
