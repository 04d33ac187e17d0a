"""The cube-symmetry codes of include/uresnet_hip.h ("cube-symmetry augmentation and test-time averaging") in pure numpy: the
definition every device pass is checked against, the group arithmetic, and the per-minibatch draw of the driver's AUGMENT flag.

An operation is a small integer code.  For one event ``x`` of shape ``[*spatial, C]``::

    out = np.flip(np.transpose(x, P[code >> ndim] + (ndim,)), axis=[a for a in range(ndim) if (code >> a) & 1])

with ``P`` the axis permutations in lexicographic order: 48 codes in 3-D, 8 in 2-D, code 0 the identity, bit ``a`` flips OUTPUT
axis ``a``.  Equivalently input voxel ``i`` lands at output voxel ``o`` with ``o[a] = f_a(i[P[a]])``, ``f_a(t) = spatial[a]-1-t``
if bit ``a`` is set, else ``t``.  A code is valid for a shape iff ``spatial[P[a]] == spatial[a]`` for every ``a``.
"""
import itertools

import numpy as np


def perms(ndim):
    """The axis permutations of ``ndim`` axes in lexicographic order."""
    if ndim not in (2, 3):
        raise ValueError('symmetry: ndim = %r not in (2, 3)' % (ndim,))
    return list(itertools.permutations(range(ndim)))


def count(ndim):
    return len(perms(ndim)) << ndim


def _split(ndim, code):
    code = int(code)
    if not 0 <= code < count(ndim):
        raise ValueError('symmetry: code %d outside [0, %d) for %d-D' % (code, count(ndim), ndim))
    return perms(ndim)[code >> ndim], [(code >> a) & 1 for a in range(ndim)]


def _join(ndim, p, flips):
    return (perms(ndim).index(tuple(p)) << ndim) | sum(int(f) << a for a, f in enumerate(flips))


def valid(spatial, code):
    """Whether ``code`` keeps the shape ``spatial`` (it only permutes axes of equal size)."""
    spatial = tuple(int(s) for s in spatial)
    if not 0 <= int(code) < count(len(spatial)):
        return False
    p, _ = _split(len(spatial), code)
    return all(spatial[p[a]] == spatial[a] for a in range(len(spatial)))


def inverse(ndim, code):
    """i[P[a]] = f_a(o[a]): the inverse permutes by P^-1 and flips axis k iff the code flips axis P^-1[k]."""
    p, f = _split(ndim, code)
    inv = [p.index(k) for k in range(ndim)]
    return _join(ndim, inv, [f[inv[k]] for k in range(ndim)])


def compose(ndim, a, b):
    """The code of "b after a": o[y] = fb_y(m[Pb[y]]) with m[x] = fa_x(i[Pa[x]])."""
    pa, fa = _split(ndim, a)
    pb, fb = _split(ndim, b)
    return _join(ndim, [pa[pb[y]] for y in range(ndim)], [fb[y] ^ fa[pb[y]] for y in range(ndim)])


def apply_numpy(x, spatial, code):
    """The definition: ``x`` is one event ``[*spatial]`` or ``[*spatial, C]`` (or anything that reshapes to it); a contiguous
    array of the same shape comes back."""
    spatial = tuple(int(s) for s in spatial)
    ndim = len(spatial)
    if not valid(spatial, code):
        raise ValueError('symmetry: code %d is not valid for the shape %s' % (code, spatial))
    x = np.asarray(x)
    shape = x.shape
    v = x.reshape(spatial + (-1,))
    p, f = _split(ndim, code)
    out = np.flip(np.transpose(v, p + (ndim,)), axis=[a for a in range(ndim) if f[a]])
    return np.ascontiguousarray(out).reshape(shape)


def apply_batch(x, spatial, codes):
    """``apply_numpy`` per event of ``x`` [N, ...] with one code per event."""
    x = np.asarray(x)
    if len(codes) != x.shape[0]:
        raise ValueError('symmetry: %d codes for %d events' % (len(codes), x.shape[0]))
    return np.stack([apply_numpy(x[i], spatial, c) for i, c in enumerate(codes)])


def group(name, spatial):
    """The codes of a named group that are valid for ``spatial``: '' -> [0], 'flip' -> the flips, 'cube' -> every valid code."""
    ndim = len(tuple(spatial))
    if name == '':
        return [0]
    if name == 'flip':
        return list(range(1 << ndim))
    if name == 'cube':
        return [c for c in range(count(ndim)) if valid(spatial, c)]
    raise ValueError("symmetry: group %r not in ('', 'flip', 'cube')" % (name,))


def draw(seed, iteration, minibatch, rank, n, codes):
    """``n`` codes drawn uniformly from ``codes`` by a counter-based generator keyed by (seed, iteration, minibatch, rank) and
    nothing else: the same tuple gives the same ops, so a resumed run repeats them, and ranks differ."""
    words = [int(seed) & 0xFFFFFFFF, int(iteration) & 0xFFFFFFFF, int(minibatch) & 0xFFFFFFFF, int(rank) & 0xFFFFFFFF]
    key = np.array([words[0] | (words[1] << 32), words[2] | (words[3] << 32)], dtype=np.uint64)
    rng = np.random.Generator(np.random.Philox(key=key))
    codes = np.asarray(list(codes), dtype=np.int32)
    return [int(c) for c in codes[rng.integers(0, len(codes), size=int(n))]]
