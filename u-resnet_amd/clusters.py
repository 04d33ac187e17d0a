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


# ---- per-cluster object records (csrc/cluster_features.hip does it on the device; this is the statement) --------------------------
FIX_SHIFT = 16                      # charge is summed in fixed point: rint(value * 2^16) as an integer
FIX_LIMIT = 2.0 ** 15               # |value| at or beyond it (or not finite): no charge, bit 0 of flags
MAX_EXTENT = 32768
JACOBI_SWEEPS = 8
JACOBI_PAIRS = ((0, 1), (0, 2), (1, 2))
PAIRS = ((0, 0), (1, 1), (2, 2), (0, 1), (0, 2), (1, 2))       # the order of dd and cov
_PAIR_AT = {(0, 0): 0, (1, 1): 1, (2, 2): 2, (0, 1): 3, (1, 0): 3, (0, 2): 4, (2, 0): 4, (1, 2): 5, (2, 1): 5}


def jacobi_eigen3(cov):
    """Eigenvalues and the leading eigenvector of the symmetric 3 x 3 matrix ``cov`` (six fp64 numbers in the order of PAIRS) by
    cyclic Jacobi on a FIXED schedule: JACOBI_SWEEPS sweeps over the pairs (0,1), (0,2), (1,2); nothing is tested for convergence.
    Every line below is one fp64 operation rounded on its own; the device kernel follows it operation for operation.

    The matrix is held as its six elements a[00, 11, 22, 01, 02, 12], the vectors as v[row][column], the identity at the start.
    One rotation of the pair (p, q), with r the third index, is skipped when a_pq == 0 exactly (either sign of zero); otherwise
        theta = (a_qq - a_pp) / (2 * a_pq)
        t     = sign(theta) / (|theta| + sqrt(theta * theta + 1))        sign(theta) = +1 for theta >= 0, else -1
        c     = 1 / sqrt(t * t + 1)
        s     = t * c
        tau   = s / (1 + c)
        h     = t * a_pq
    and then, in this order, every right-hand side reading the values from BEFORE the rotation,
        a_pp = a_pp - h
        a_qq = a_qq + h
        a_pq = 0
        a_rp = a_rp - s * (a_rq + tau * a_rp)
        a_rq = a_rq + s * (a_rp - tau * a_rq)
        for k = 0, 1, 2:   v_kp = v_kp - s * (v_kq + tau * v_kp)
                           v_kq = v_kq + s * (v_kp - tau * v_kq)
    (a theta too large to square gives t = 0, c = 1, s = 0: the element is dropped and nothing else moves).
    ``eval`` = the diagonal in descending order, ties keeping the lower column first; ``axis`` = the column of the first, negated as
    a whole (unary minus) when its component of largest magnitude -- the lowest axis among equals -- is negative."""
    a = [np.float64(x) for x in cov]
    one, two, zero = np.float64(1.0), np.float64(2.0), np.float64(0.0)
    v = [[one if i == k else zero for i in range(3)] for k in range(3)]
    for p, q in JACOBI_PAIRS * JACOBI_SWEEPS:
        with np.errstate(over='ignore'):                       # theta may overflow by design: t = 0 then
            r = 3 - p - q
            pq, rp, rq = _PAIR_AT[(p, q)], _PAIR_AT[(r, p)], _PAIR_AT[(r, q)]
            apq = a[pq]
            if apq == zero:
                continue
            theta = (a[q] - a[p]) / (two * apq)
            root = np.sqrt(theta * theta + one)
            t = (one if theta >= zero else -one) / (np.abs(theta) + root)
            c = one / np.sqrt(t * t + one)
            s = t * c
            tau = s / (one + c)
            h = t * apq
            a[p] = a[p] - h
            a[q] = a[q] + h
            a[pq] = zero
            g, f = a[rp], a[rq]
            a[rp] = g - s * (f + tau * g)
            a[rq] = f + s * (g - tau * f)
            for k in range(3):
                g, f = v[k][p], v[k][q]
                v[k][p] = g - s * (f + tau * g)
                v[k][q] = f + s * (g - tau * f)
    order = sorted(range(3), key=lambda i: -a[i])              # stable: equal values keep the lower column first
    ev = np.array([a[i] for i in order], np.float64)
    ax = [v[k][order[0]] for k in range(3)]
    big = 0
    for k in (1, 2):
        if np.abs(ax[k]) > np.abs(ax[big]):
            big = k
    if ax[big] < zero:
        ax = [-x for x in ax]
    return ev, np.array(ax, np.float64)


def cluster_features_numpy(offsets, index, value, cluster, table_offsets, spatial):
    """The statement of the per-cluster object records: for every cluster (global row = ``table_offsets[event]`` + event-local id)
    the reductions over its members, the entries j of that event with ``cluster[j] == id``.  Slow on purpose: Python integers
    wherever 64 bits could overflow, scalar fp64 operations in one fixed order, one member at a time.

    Coordinates x are those of ``np.unravel_index(index, spatial)``; in 2-D the third coordinate is 0.  Integers, exact:
    ``n`` members, ``lo`` / ``hi`` [3] bounding box, ``s`` [3] coordinate sums, ``charge`` = sum of rint(float64(value) * 2^16) (a
    member with |value| >= 2^15 or a value that is not finite adds nothing and sets bit 0 of ``flags``; no values: 0), anchor
    ``m`` = floor((2 s + n) / (2 n)) (the centroid rounded to a voxel), ``d`` [3] = sum (x - m), ``dd`` [6] = sum (x_a - m_a)(x_b -
    m_b) over PAIRS.  Bounds, with every extent <= 32768 and fewer than 2^31 entries: |s| < 2^15 * 2^31 = 2^46 and 2 s + n < 2^48;
    |x - m| < 2^15, so |d| < 2^46 and |dd| < 2^30 * 2^31 = 2^61; |rint(value * 2^16)| <= 2^31, so |charge| <= 2^62: all inside
    int64.  fp64, one rounded operation each: ``centroid`` = s / n; ``cov[ab]`` = dd[ab] / n - (d[a] / n) * (d[b] / n), where the
    anchor keeps |d / n| <= 0.5, so nothing cancels; ``eval`` / ``axis`` = ``jacobi_eigen3(cov)``.  Ends: for every member
    t = (axis[0] * (x_0 - m_0) + axis[1] * (x_1 - m_1)) + axis[2] * (x_2 - m_2) in fp64, rounded once to fp32 (a zero of either
    sign counts as +0); ``end_lo`` / ``end_hi`` = the list position, global across the batch, of the smallest / largest fp32 t,
    the LOWER position among equals in both; ``t_lo`` / ``t_hi`` those fp32 values; ``length`` = float64(t_hi) - float64(t_lo).

    Returns a dict of arrays with one row per cluster: int64 ``n, charge, s, lo, hi, m, d, dd, flags, end_lo, end_hi``; float64
    ``centroid, cov, eval, axis, length``; float32 ``t_lo, t_hi``."""
    offsets = [int(x) for x in np.asarray(offsets).reshape(-1)]
    table_offsets = [int(x) for x in np.asarray(table_offsets).reshape(-1)]
    index = np.asarray(index, np.int64).reshape(-1)
    cluster = np.asarray(cluster, np.int64).reshape(-1)
    spatial = tuple(int(s) for s in spatial)
    nev, ndim = len(offsets) - 1, len(spatial)
    if ndim not in (2, 3) or any(not 1 <= s <= MAX_EXTENT for s in spatial):
        raise ValueError('cluster_features_numpy: spatial = %r, expected 2 or 3 extents in [1, %d]' % (spatial, MAX_EXTENT))
    if len(table_offsets) != nev + 1 or index.size != cluster.size or (nev >= 0 and offsets[-1] != index.size):
        raise ValueError('cluster_features_numpy: offsets, table_offsets and the lists disagree')
    if value is not None:
        value = np.asarray(value, np.float32).reshape(-1)
        if value.size != index.size:
            raise ValueError('cluster_features_numpy: %d values for %d entries' % (value.size, index.size))
    K = table_offsets[-1]
    rows = [None] * K
    for e in range(nev):
        members = [[] for _ in range(table_offsets[e + 1] - table_offsets[e])]
        for j in range(offsets[e], offsets[e + 1]):
            if cluster[j] >= 0:
                members[int(cluster[j])].append(j)
        for i, mem in enumerate(members):
            rows[table_offsets[e] + i] = mem
    out = {k: np.zeros((K,) + shp, dt) for k, shp, dt in (
        ('n', (), np.int64), ('charge', (), np.int64), ('s', (3,), np.int64), ('lo', (3,), np.int64), ('hi', (3,), np.int64),
        ('m', (3,), np.int64), ('d', (3,), np.int64), ('dd', (6,), np.int64), ('flags', (), np.int64), ('end_lo', (), np.int64),
        ('end_hi', (), np.int64), ('centroid', (3,), np.float64), ('cov', (6,), np.float64), ('eval', (3,), np.float64),
        ('axis', (3,), np.float64), ('length', (), np.float64), ('t_lo', (), np.float32), ('t_hi', (), np.float32))}
    for row, mem in enumerate(rows):
        if not mem:
            raise ValueError('cluster_features_numpy: cluster row %d has no member' % row)
        xs = []
        for j in mem:
            c = np.unravel_index(int(index[j]), spatial)
            xs.append(tuple(int(c[a]) if a < ndim else 0 for a in range(3)))
        n = len(mem)
        s = [sum(x[a] for x in xs) for a in range(3)]
        charge, flags = 0, 0
        if value is not None:
            for j in mem:
                val = np.float64(value[j])
                if not np.isfinite(val) or abs(val) >= FIX_LIMIT:
                    flags |= 1
                else:
                    charge += int(np.rint(val * np.float64(2.0 ** FIX_SHIFT)))
        m = [(2 * s[a] + n) // (2 * n) for a in range(3)]
        d = [sum(x[a] - m[a] for x in xs) for a in range(3)]
        dd = [sum((x[a] - m[a]) * (x[b] - m[b]) for x in xs) for a, b in PAIRS]
        fn = np.float64(n)
        mean = [np.float64(d[a]) / fn for a in range(3)]
        cov = [np.float64(dd[k]) / fn - mean[a] * mean[b] for k, (a, b) in enumerate(PAIRS)]
        ev, ax = jacobi_eigen3(cov)
        best_lo = best_hi = None
        for j, x in zip(mem, xs):
            t = (ax[0] * np.float64(x[0] - m[0]) + ax[1] * np.float64(x[1] - m[1])) + ax[2] * np.float64(x[2] - m[2])
            t = np.float32(t)
            if t == np.float32(0.0):
                t = np.float32(0.0)
            if best_lo is None or t < best_lo[0]:            # members come in list order: strict comparisons keep the lower position
                best_lo = (t, j)
            if best_hi is None or t > best_hi[0]:
                best_hi = (t, j)
        out['n'][row], out['charge'][row], out['flags'][row] = n, charge, flags
        out['s'][row], out['m'][row], out['d'][row], out['dd'][row] = s, m, d, dd
        out['lo'][row] = [min(x[a] for x in xs) for a in range(3)]
        out['hi'][row] = [max(x[a] for x in xs) for a in range(3)]
        out['centroid'][row] = [np.float64(s[a]) / fn for a in range(3)]
        out['cov'][row], out['eval'][row], out['axis'][row] = cov, ev, ax
        out['end_lo'][row], out['end_hi'][row] = best_lo[1], best_hi[1]
        out['t_lo'][row], out['t_hi'][row] = best_lo[0], best_hi[0]
        out['length'][row] = np.float64(best_hi[0]) - np.float64(best_lo[0])
    return out


# ---- cluster matching (csrc/cluster_match.hip does it on the device; this is the statement) ---------------------------------------
MATCH_ROW_INT = ('n', 'charge', 'matched', 'partners', 'best', 'overlap', 'overlap_charge', 'flags')
MATCH_ROW_REAL = ('purity', 'efficiency', 'iou', 'matched_fraction')
MATCH_EVENT_INT = ('n_both', 'pairs', 'pairs_a', 'pairs_b', 'cells', 'rows_a', 'rows_b', 'mutual', 'overlap_a', 'members_a',
                   'overlap_b', 'members_b')
MATCH_EVENT_REAL = ('ari', 'purity', 'efficiency', 'mutual_fraction')


def cluster_match_numpy(offsets, cluster_a, table_offsets_a, cluster_b, table_offsets_b, value=None):
    """The statement of the match of two clusterings of the same concatenated per-event lists: ``cluster_a`` / ``cluster_b`` hold
    event-local ids or -1 as ``ursn_cluster_voxels`` writes them, each with its ``table_offsets`` [n+1] (global row =
    ``table_offsets[event]`` + id).  A is "predicted" and B "true" by convention; the definition is symmetric.  Slow on purpose:
    Python integers wherever 64 bits could overflow, scalar fp64 operations in one fixed order, one entry at a time.

    A CELL is a pair (A row, B row) of one event with at least one common entry: ``c`` = the number of common entries, ``q`` = the
    sum of rint(float64(value) * 2^16) over them (an entry with |value| >= 2^15 or a value that is not finite adds nothing and sets
    bit 0 of the flags of BOTH its rows; no values: 0).

    Row record of a row of side X (Y the other side), MATCH_ROW_INT: ``n`` members whatever their Y id, ``charge`` the fixed-point
    sum over them, ``matched`` members whose Y id is >= 0, ``partners`` cells of the row, ``best`` the event-local Y id of the cell
    with the largest c (the lowest id among equals; -1 without a cell), ``overlap`` / ``overlap_charge`` that cell's c / q (0
    without one), ``flags`` bit 0 = a charge was dropped, bit 1 = mutual (the best row's own best is this row).  MATCH_ROW_REAL,
    each ONE division of integers converted to fp64: ``purity`` = overlap / n, ``efficiency`` = overlap / n_Y(best), ``iou`` =
    overlap / (n + n_Y(best) - overlap), ``matched_fraction`` = matched / n (efficiency and iou are 0.0 without a cell).

    Event record, MATCH_EVENT_INT: [0] N = entries with both ids >= 0, [1] S = sum over cells of c (c - 1) / 2, [2] SA = sum over A
    rows of matched (matched - 1) / 2, [3] SB the same over B rows, [4] cells, [5] KA, [6] KB, [7] mutual pairs, [8] / [9] sums over
    A rows of overlap / n, [10] / [11] the same over B rows.  Bounds with fewer than 2^31 entries: N, KA, KB, cells, mutual and the
    sums of overlap and n are below 2^31; S, SA, SB <= N (N - 1) / 2 < 2^61; |charge|, |q| <= 2^31 * 2^31 = 2^62 in a row record
    and every event integer is below 2^62: all inside int64.  MATCH_EVENT_REAL: [0] the adjusted Rand index, in this order: P =
    N (N - 1) / 2 as an integer, 1.0 if P == 0; E = (f(SA) * f(SB)) / f(P); mean = (f(SA) + f(SB)) * 0.5; den = mean - E, 1.0 if
    den == 0; else (f(S) - E) / den, with f the int64 -> fp64 conversion and every operation rounded on its own; [1] = [8] / [9]
    (0.0 when [9] == 0), [2] = [10] / [11] (0.0 when [11] == 0), [3] = f(2 mutual) / f(KA + KB) (0.0 without rows).

    Cell list, CSR by global A row: ``pair_offsets`` [KA_total + 1], ``pair_b`` (event-local B id, ascending inside a row),
    ``pair_n``, ``pair_q``.  An id outside [-1, K_e) of its event and a row without a member raise ValueError.

    Returns a dict: ``a_int`` / ``b_int`` int64 [K, 8], ``a_real`` / ``b_real`` float64 [K, 4], ``event_int`` int64 [n, 12],
    ``event_real`` float64 [n, 4], ``pair_offsets`` int64, ``pair_b`` int32, ``pair_n`` / ``pair_q`` int64."""
    offsets = [int(x) for x in np.asarray(offsets).reshape(-1)]
    toff = [[int(x) for x in np.asarray(t).reshape(-1)] for t in (table_offsets_a, table_offsets_b)]
    ids = [np.asarray(c, np.int64).reshape(-1) for c in (cluster_a, cluster_b)]
    nev = len(offsets) - 1
    if nev < 1 or any(len(t) != nev + 1 for t in toff) or ids[0].size != ids[1].size or offsets[0] != 0 or offsets[-1] != ids[0].size \
            or any(t[0] != 0 or any(t[e + 1] < t[e] for e in range(nev)) for t in toff) \
            or any(offsets[e + 1] < offsets[e] for e in range(nev)):
        raise ValueError('cluster_match_numpy: offsets, table offsets and the id lists disagree')
    if value is not None:
        value = np.asarray(value, np.float32).reshape(-1)
        if value.size != ids[0].size:
            raise ValueError('cluster_match_numpy: %d values for %d entries' % (value.size, ids[0].size))
    K = [t[-1] for t in toff]
    rows = [[{'n': 0, 'charge': 0, 'matched': 0, 'flags': 0, 'cells': {}} for _ in range(K[x])] for x in (0, 1)]
    for e in range(nev):
        for j in range(offsets[e], offsets[e + 1]):
            local = [int(ids[x][j]) for x in (0, 1)]
            for x in (0, 1):
                if not -1 <= local[x] < toff[x][e + 1] - toff[x][e]:
                    raise ValueError('cluster_match_numpy: entry %d has id %d outside [-1, %d)' % (j, local[x], toff[x][e + 1] - toff[x][e]))
            q, dropped = 0, False
            if value is not None:
                val = np.float64(value[j])
                if not np.isfinite(val) or abs(val) >= FIX_LIMIT:
                    dropped = True
                else:
                    q = int(np.rint(val * np.float64(2.0 ** FIX_SHIFT)))
            for x in (0, 1):
                if local[x] < 0:
                    continue
                row = rows[x][toff[x][e] + local[x]]
                row['n'] += 1
                row['charge'] += q
                if dropped:
                    row['flags'] |= 1
                if local[1 - x] >= 0:
                    row['matched'] += 1
                    cell = row['cells'].setdefault(local[1 - x], [0, 0])
                    cell[0] += 1
                    cell[1] += q
    event_of = [[e for e in range(nev) for _ in range(toff[x][e + 1] - toff[x][e])] for x in (0, 1)]
    for x in (0, 1):
        for r, row in enumerate(rows[x]):
            if row['n'] == 0:
                raise ValueError('cluster_match_numpy: row %d of side %s has no member' % (r, 'AB'[x]))
            row['best'], row['overlap'], row['overlap_charge'] = -1, 0, 0
            for other in sorted(row['cells']):                  # ascending id: a strict comparison keeps the lowest among equals
                if row['cells'][other][0] > row['overlap']:
                    row['best'], (row['overlap'], row['overlap_charge']) = other, row['cells'][other]
    out = {'a_int': np.zeros((K[0], 8), np.int64), 'b_int': np.zeros((K[1], 8), np.int64),
           'a_real': np.zeros((K[0], 4), np.float64), 'b_real': np.zeros((K[1], 4), np.float64),
           'event_int': np.zeros((nev, 12), np.int64), 'event_real': np.zeros((nev, 4), np.float64)}
    ev = [[0] * 12 for _ in range(nev)]
    zero = np.float64(0.0)
    for x in (0, 1):
        for r, row in enumerate(rows[x]):
            e = event_of[x][r]
            n, matched, overlap = row['n'], row['matched'], row['overlap']
            n_other, mutual = 0, False
            if row['best'] >= 0:
                other = rows[1 - x][toff[1 - x][e] + row['best']]
                n_other = other['n']
                mutual = other['best'] == r - toff[x][e]
            flags = row['flags'] | (2 if mutual else 0)
            out['ab'[x] + '_int'][r] = [n, row['charge'], matched, len(row['cells']), row['best'], overlap, row['overlap_charge'], flags]
            fn = np.float64(n)
            out['ab'[x] + '_real'][r] = [np.float64(overlap) / fn,
                                         np.float64(overlap) / np.float64(n_other) if row['best'] >= 0 else zero,
                                         np.float64(overlap) / np.float64(n + n_other - overlap) if row['best'] >= 0 else zero,
                                         np.float64(matched) / fn]
            if x == 0:
                ev[e][0] += matched
                ev[e][1] += sum(c * (c - 1) // 2 for c, _ in row['cells'].values())
                ev[e][2] += matched * (matched - 1) // 2
                ev[e][4] += len(row['cells'])
                ev[e][7] += 1 if mutual else 0
                ev[e][8] += overlap
                ev[e][9] += n
            else:
                ev[e][3] += matched * (matched - 1) // 2
                ev[e][10] += overlap
                ev[e][11] += n
    half = np.float64(0.5)
    for e in range(nev):
        ev[e][5], ev[e][6] = toff[0][e + 1] - toff[0][e], toff[1][e + 1] - toff[1][e]
        assert all(0 <= v < 2 ** 62 for v in ev[e])
        N, S, SA, SB = ev[e][:4]
        P = N * (N - 1) // 2
        ari = np.float64(1.0)
        if P != 0:
            E = (np.float64(SA) * np.float64(SB)) / np.float64(P)
            mean = (np.float64(SA) + np.float64(SB)) * half
            den = mean - E
            if den != zero:
                ari = (np.float64(S) - E) / den
        out['event_int'][e] = ev[e]
        out['event_real'][e] = [ari, np.float64(ev[e][8]) / np.float64(ev[e][9]) if ev[e][9] else zero,
                                np.float64(ev[e][10]) / np.float64(ev[e][11]) if ev[e][11] else zero,
                                np.float64(2 * ev[e][7]) / np.float64(ev[e][5] + ev[e][6]) if ev[e][5] + ev[e][6] else zero]
    pair_offsets, pb, pn, pq = [0], [], [], []
    for row in rows[0]:
        for other in sorted(row['cells']):
            pb.append(other), pn.append(row['cells'][other][0]), pq.append(row['cells'][other][1])
        pair_offsets.append(len(pb))
    out['pair_offsets'] = np.array(pair_offsets, np.int64)
    out['pair_b'], out['pair_n'], out['pair_q'] = np.array(pb, np.int32), np.array(pn, np.int64), np.array(pq, np.int64)
    return out


# ---- cluster contact graph (csrc/cluster_graph.hip does it on the device; this is the statement) ----------------------------------
GRAPH_EDGE = ('b', 'pairs', 'touch', 'dist2', 'pos_a', 'pos_b')
GRAPH_ROW = ('degree', 'group', 'nearest', 'nearest_dist2', 'pairs', 'touching')
GRAPH_GROUP = ('rows', 'edges', 'n', 'charge', 'lo0', 'lo1', 'lo2', 'hi0', 'hi1', 'hi2', 'first_row', 'mask_flags')
GRAPH_EVENT = ('groups', 'edges', 'isolated', 'largest')
GRAPH_MAX_GAP = 3


class ClusterGraphSpec(object):
    """``gap`` in [1, 3]: two entries of different clusters are near when their coordinates differ by at most ``gap`` on every
    axis."""

    def __init__(self, gap=1):
        if type(gap) is not int or not 1 <= gap <= GRAPH_MAX_GAP:
            raise ValueError('ClusterGraphSpec: gap = %r, expected an integer in [1, %d]' % (gap, GRAPH_MAX_GAP))
        self.gap = gap

    def __repr__(self):
        return 'ClusterGraphSpec(gap=%r)' % (self.gap,)


def cluster_graph_numpy(offsets, index, cluster, table_offsets, spatial, spec=None, value=None, cls=None):
    """The statement of the contact graph of the clusters of concatenated per-event lists: ``index`` sorted per event, row-major in
    ``spatial`` (2 or 3 extents <= 32768), ``cluster`` the event-local ids or -1 and ``table_offsets`` [n+1] as
    ``ursn_cluster_voxels`` writes them (global row = ``table_offsets[event]`` + id), optionally ``value`` [m] and the cluster
    table's ``cls`` [K_total].  Slow on purpose: Python integers, one entry and one offset at a time.

    Coordinates are ``np.unravel_index(index, spatial)``, with x[2] = 0 in 2-D.  Two entries of one event are NEAR when each has an
    id >= 0, the ids differ and the coordinates differ by at most ``spec.gap`` on every axis (Chebyshev distance, decided on
    coordinates, never on indices).  An EDGE is an unordered pair of rows a < b of one event with at least one near pair of entries,
    one in a and one in b.

    GRAPH_EDGE: ``b`` (event-local), ``pairs`` the unordered near pairs between the two rows, ``touch`` those at Chebyshev distance
    1, ``dist2`` the smallest squared Euclidean distance over them, ``pos_a`` / ``pos_b`` the positions in the concatenated list of
    the near pair smallest in (dist2, position in a, position in b).  Stored as CSR by global row a, ascending b, with
    ``edge_offsets`` [K_total + 1].  GRAPH_ROW: ``degree`` (edges on either side), ``group`` (event-local), ``nearest`` the
    event-local id of the partner smallest in (dist2, id) or -1, ``nearest_dist2`` (0 without an edge), ``pairs`` summed over the
    row's edges, ``touching`` its edges with touch > 0.  GROUPS are the connected components of an event's rows under its edges,
    numbered per event in the order of their lowest row.  GRAPH_GROUP: ``rows``, ``edges``, ``n`` member entries, ``charge`` = sum of
    rint(float64(value) * 2^16) (|value| >= 2^15 or a non-finite value adds nothing and sets bit 0 of the flags; 0 without values),
    the coordinate box ``lo`` / ``hi`` (0 for the missing 2-D axis), ``first_row``, ``mask_flags`` = class_mask | flags << 32 with
    bit ``cls`` of every member row (0 without ``cls``); with ``group_offsets`` [n+1].  GRAPH_EVENT: ``groups``, ``edges``,
    ``isolated`` (rows of degree 0), ``largest`` (the largest group's n).  Per entry ``group``: the group of its row, -1 for id -1.

    Bounds: an entry has at most 7^3 - 1 = 342 neighbours and every pair is counted once, so pairs < m * 171 < 2^39; dist2 <= 27;
    the box is within 2^15; |charge| <= 2^31 * 2^31 = 2^62.

    An id outside [-1, K_e), a row without a member, an index outside the volume at an entry with an id and a cls >= 32 raise
    ValueError.  Returns a dict: ``edge_offsets`` int64 [K+1], ``edges`` int64 [E, 6], ``rows`` int64 [K, 6], ``group_offsets``
    int64 [n+1], ``groups`` int64 [G, 12], ``events`` int64 [n, 4], ``group`` int32 [m]."""
    spec = ClusterGraphSpec() if spec is None else spec
    if not isinstance(spec, ClusterGraphSpec):
        raise ValueError('cluster_graph_numpy: spec = %r, expected a ClusterGraphSpec' % (spec,))
    gap = spec.gap
    spatial = tuple(int(s) for s in spatial)
    if len(spatial) not in (2, 3) or any(not 1 <= s <= MAX_EXTENT for s in spatial):
        raise ValueError('cluster_graph_numpy: spatial = %r, expected 2 or 3 extents in [1, %d]' % (spatial, MAX_EXTENT))
    offsets = [int(x) for x in np.asarray(offsets).reshape(-1)]
    toff = [int(x) for x in np.asarray(table_offsets).reshape(-1)]
    index = [int(x) for x in np.asarray(index).reshape(-1)]
    ids = [int(x) for x in np.asarray(cluster).reshape(-1)]
    nev, m = len(offsets) - 1, len(index)
    if nev < 1 or len(toff) != nev + 1 or len(ids) != m or offsets[0] != 0 or offsets[-1] != m or toff[0] != 0 \
            or any(offsets[e + 1] < offsets[e] or toff[e + 1] < toff[e] for e in range(nev)):
        raise ValueError('cluster_graph_numpy: offsets, table offsets and the lists disagree')
    K = toff[-1]
    if value is not None:
        value = np.asarray(value, np.float32).reshape(-1)
        if value.size != m:
            raise ValueError('cluster_graph_numpy: %d values for %d entries' % (value.size, m))
    if cls is not None:
        cls = [int(c) for c in np.asarray(cls).reshape(-1)]
        if len(cls) != K or any(not 0 <= c < 32 for c in cls):
            raise ValueError('cluster_graph_numpy: cls must hold %d classes in [0, 32)' % K)
    vox = 1
    for s in spatial:
        vox *= s
    steps = [d for d in np.ndindex(*([2 * gap + 1] * len(spatial))) if any(x != gap for x in d)]
    edges = {}                                   # (global a, global b) -> [pairs, touch, (dist2, pos_a, pos_b)]
    members = [0] * K
    coords = [None] * m
    for e in range(nev):
        ke = toff[e + 1] - toff[e]
        where = {}
        for j in range(offsets[e], offsets[e + 1]):
            if not -1 <= ids[j] < ke:
                raise ValueError('cluster_graph_numpy: entry %d has id %d outside [-1, %d)' % (j, ids[j], ke))
            if ids[j] < 0:
                continue
            if not 0 <= index[j] < vox:
                raise ValueError('cluster_graph_numpy: entry %d has index %d outside the volume %r' % (j, index[j], spatial))
            x = tuple(int(c) for c in np.unravel_index(index[j], spatial))
            coords[j] = x + (0,) * (3 - len(x))
            where[x] = j
            members[toff[e] + ids[j]] += 1
        for x, j in where.items():
            for d in steps:
                y = tuple(x[k] + d[k] - gap for k in range(len(x)))
                q = where.get(y)
                if q is None or q > j or ids[q] == ids[j]:    # every unordered pair once, from its higher position
                    continue
                (ra, pa), (rb, pb) = sorted(((ids[j], j), (ids[q], q)))
                delta = [abs(d[k] - gap) for k in range(len(x))]
                cell = edges.setdefault((toff[e] + ra, toff[e] + rb), [0, 0, None])
                cell[0] += 1
                cell[1] += 1 if max(delta) == 1 else 0
                rank = (sum(v * v for v in delta), pa, pb)
                if cell[2] is None or rank < cell[2]:
                    cell[2] = rank
    for r in range(K):
        if members[r] == 0:
            raise ValueError('cluster_graph_numpy: row %d has no member' % r)
    event_of = [e for e in range(nev) for _ in range(toff[e + 1] - toff[e])]
    rows = [[0, -1, -1, 0, 0, 0] for _ in range(K)]
    nearest = [None] * K
    parent = list(range(K))

    def find(x):
        while parent[x] != x:
            parent[x] = parent[parent[x]]
            x = parent[x]
        return x

    edge_offsets, table = [0], []
    by_row = [[] for _ in range(K)]
    for (a, b) in sorted(edges):
        by_row[a].append(b)
    for a in range(K):
        for b in by_row[a]:
            pairs, touch, (dist2, pa, pb) = edges[(a, b)]
            assert pairs < max(m, 1) * 171 and dist2 <= 27
            table.append([b - toff[event_of[a]], pairs, touch, dist2, pa, pb])
            for x, y in ((a, b), (b, a)):
                rows[x][0] += 1
                rows[x][4] += pairs
                rows[x][5] += 1 if touch > 0 else 0
                if nearest[x] is None or (dist2, y) < nearest[x]:
                    nearest[x] = (dist2, y)
            ra, rb = find(a), find(b)
            if ra != rb:
                parent[max(ra, rb)] = min(ra, rb)
        edge_offsets.append(len(table))
    roots = [find(r) for r in range(K)]
    group_of, group_offsets, groups = [0] * K, [0], []
    events = [[0, 0, 0, 0] for _ in range(nev)]
    for e in range(nev):
        local = {}
        for r in range(toff[e], toff[e + 1]):
            if roots[r] == r:
                local[r] = len(local)
                groups.append([0, 0, 0, 0, MAX_EXTENT, MAX_EXTENT, MAX_EXTENT, -1, -1, -1, r - toff[e], 0])
            g = group_offsets[e] + local[roots[r]]              # a root is the lowest row of its group: it came first
            group_of[r] = g
            rows[r][1] = local[roots[r]]
            if nearest[r] is not None:
                rows[r][2], rows[r][3] = nearest[r][1] - toff[e], nearest[r][0]
            groups[g][0] += 1
            groups[g][1] += len(by_row[r])
            if cls is not None:
                groups[g][11] |= 1 << cls[r]
            events[e][1] += len(by_row[r])
            events[e][2] += 1 if rows[r][0] == 0 else 0
        group_offsets.append(len(groups))
        events[e][0] = len(local)
    group = np.full(m, -1, np.int32)
    for e in range(nev):
        for j in range(offsets[e], offsets[e + 1]):
            if ids[j] < 0:
                continue
            g = group_of[toff[e] + ids[j]]
            rec = groups[g]
            group[j] = g - group_offsets[e]
            rec[2] += 1
            if value is not None:
                val = np.float64(value[j])
                if not np.isfinite(val) or abs(val) >= FIX_LIMIT:
                    rec[11] |= 1 << 32
                else:
                    rec[3] += int(np.rint(val * np.float64(2.0 ** FIX_SHIFT)))
            for k in range(3):
                rec[4 + k], rec[7 + k] = min(rec[4 + k], coords[j][k]), max(rec[7 + k], coords[j][k])
    for e in range(nev):
        for g in range(group_offsets[e], group_offsets[e + 1]):
            assert abs(groups[g][3]) <= 2 ** 62
            events[e][3] = max(events[e][3], groups[g][2])
    return {'edge_offsets': np.array(edge_offsets, np.int64), 'edges': np.array(table, np.int64).reshape(-1, 6),
            'rows': np.array(rows, np.int64).reshape(-1, 6), 'group_offsets': np.array(group_offsets, np.int64),
            'groups': np.array(groups, np.int64).reshape(-1, 12), 'events': np.array(events, np.int64).reshape(-1, 4), 'group': group}


# ---- per-cluster charge profiles along the principal axis (csrc/cluster_profile.hip does it on the device; this is the statement) --
PROFILE_BIN_INT = ('n', 'charge', 'd0', 'd1', 'd2', 'flags')
PROFILE_BIN_REAL = ('c0', 'c1', 'c2', 'dqdx')
PROFILE_ROW_INT = ('bins', 'filled', 'gaps', 'longest_gap', 'peak_bin', 'h', 'head_n', 'head_charge', 'tail_n', 'tail_charge',
                   'direction', 'flags')
PROFILE_ROW_REAL = ('path', 'min_cos', 'kink_bin', 'head_dqdx', 'tail_dqdx', 'straightness')
PROFILE_MIN_STEP, PROFILE_MAX_STEP = 0.5, 4096.0
PROFILE_MAX_END_BINS = 16
PROFILE_MAX_BINS = 65536


class ClusterProfileSpec(object):
    """``step``: the segment length along the principal axis in voxels, a finite float in [0.5, 4096]; ``end_bins`` in [1, 16]: the
    segments at either end whose charge is compared; ``max_bins`` in [1, 65536]: a longer profile is truncated into its last bin."""

    def __init__(self, step=1.0, end_bins=3, max_bins=4096):
        if type(step) not in (int, float) or not np.isfinite(step) or not PROFILE_MIN_STEP <= step <= PROFILE_MAX_STEP:
            raise ValueError('ClusterProfileSpec: step = %r, expected a finite float in [%g, %g]'
                             % (step, PROFILE_MIN_STEP, PROFILE_MAX_STEP))
        if type(end_bins) is not int or not 1 <= end_bins <= PROFILE_MAX_END_BINS:
            raise ValueError('ClusterProfileSpec: end_bins = %r, expected an integer in [1, %d]' % (end_bins, PROFILE_MAX_END_BINS))
        if type(max_bins) is not int or not 1 <= max_bins <= PROFILE_MAX_BINS:
            raise ValueError('ClusterProfileSpec: max_bins = %r, expected an integer in [1, %d]' % (max_bins, PROFILE_MAX_BINS))
        self.step, self.end_bins, self.max_bins = float(step), end_bins, max_bins

    def __repr__(self):
        return 'ClusterProfileSpec(step=%r, end_bins=%r, max_bins=%r)' % (self.step, self.end_bins, self.max_bins)


def profile_bin_count(length, step, max_bins):
    """(nb, nb_true, pad) of a cluster of this ``length``: three fp64 operations, each rounded on its own.  The host sizes the bin
    table with it, the device follows it."""
    length, step = np.float64(length), np.float64(step)
    nb_true = int(np.floor(length / step)) + 1
    pad = (np.float64(nb_true) * step - length) / np.float64(2.0)
    return min(nb_true, int(max_bins)), nb_true, pad


def cluster_profile_numpy(offsets, index, value, cluster, table_offsets, spatial, spec):
    """The statement of the per-cluster charge profiles: every cluster's members are sorted into segments of ``spec.step`` voxels
    along the principal axis of its object record, and each segment (bin) gets a count, a charge and a centroid.  Slow on purpose,
    in the style of ``cluster_features_numpy``, which it calls first: Python integers, scalar fp64 operations each rounded on its
    own, one member at a time.  From the object record of row r it takes ``n``, the anchor ``m``, ``axis``, ``t_lo`` and ``length``.

    Segment count, in fp64: ``nb_true`` = floor(length / step) + 1, ``nb`` = min(nb_true, max_bins), ``pad`` = (float64(nb_true) *
    step - length) / 2 (the slack of the last segment, split evenly between the two ends, so that head and tail are comparable).
    Segment of a member: t = (axis[0] * (x_0 - m_0) + axis[1] * (x_1 - m_1)) + axis[2] * (x_2 - m_2) in fp64, rounded once to fp32
    (a zero of either sign counts as +0): the object record's own expression; u = ((float64(t) - float64(t_lo)) + pad) / step;
    b = min(max(floor(u), 0), nb - 1).

    Bins, CSR by global row (``bin_offsets`` [K_total + 1]).  int64 ``n`` members, ``charge`` = sum of rint(float64(value) * 2^16),
    ``d`` [3] = sum (x - m), ``flags``: a member with a value that is not finite or with |value| >= 2^15 adds to n and d, adds
    nothing to charge and sets bit 0 (the object record's rule; no values: charge 0).  fp64 ``c`` [3] = float64(m) + float64(d) /
    float64(n) and ``dqdx`` = (float64(charge) / 2^16) / step; an empty bin holds +0.0 in all four.
    Bounds, with every extent <= 32768 and fewer than 2^31 entries: bin n < 2^31, |d| < 2^15 * 2^31 = 2^46, |charge| <= 2^31 *
    2^31 = 2^62 (any sum over bins of one row obeys the same bound), nb <= 65536.

    Rows.  int64 ``bins`` = nb, ``filled`` bins with n > 0, ``gaps`` maximal runs of empty bins between filled ones and
    ``longest_gap`` the longest, ``peak_bin`` the bin of the largest charge (lowest among equals), ``h`` = min(end_bins, nb // 2),
    ``head_n`` / ``head_charge`` over bins [0, h), ``tail_n`` / ``tail_charge`` over bins [nb - h, nb), ``direction`` = +1 if
    tail_charge > head_charge, -1 if smaller, 0 if equal or h == 0, ``flags``: bit 0 some bin is flagged, bit 1 nb_true > max_bins
    (truncated into the last bin).  ``direction`` is the sign of a charge asymmetry between the two ends and NOTHING MORE: whether
    the particle stopped there is the consumer's judgement.
    fp64 ``path`` = the length of the polyline through the centroids of the filled bins in ascending order, each segment
    sqrt((dx * dx + dy * dy) + dz * dz), added one after another; ``min_cos`` = the smallest dot / (s1 * s2) over consecutive
    pairs of polyline segments (dot in the same association; a pair with s1 * s2 == 0 is skipped; 1.0 without a pair) and
    ``kink_bin`` the bin of that pair's middle point as a float (lowest among equals, -1.0 without one); ``head_dqdx`` =
    (float64(head_charge) / 2^16) / (float64(h) * step), ``tail_dqdx`` likewise (both 0.0 when h == 0); ``straightness`` = length
    / path, or 1.0 when path == 0.

    An id outside its event's rows, a row without a member and an index outside the volume at an entry with an id raise, as in
    ``cluster_features_numpy``.  Returns ``{'objects': that function's dict, 'bin_offsets': int64 [K + 1], 'bins': {name: [B]},
    'rows': {name: [K]}}`` with the names of PROFILE_BIN_INT / _REAL and PROFILE_ROW_INT / _REAL."""
    if not isinstance(spec, ClusterProfileSpec):
        raise ValueError('cluster_profile_numpy: spec = %r, expected a ClusterProfileSpec' % (spec,))
    spatial = tuple(int(s) for s in spatial)
    off = [int(x) for x in np.asarray(offsets).reshape(-1)]
    toff = [int(x) for x in np.asarray(table_offsets).reshape(-1)]
    index = np.asarray(index, np.int64).reshape(-1)
    cluster = np.asarray(cluster, np.int64).reshape(-1)
    vox = int(np.prod(spatial, dtype=np.int64)) if spatial else 0
    for e in range(min(len(off), len(toff)) - 1):
        for j in range(off[e], min(off[e + 1], cluster.size, index.size)):
            if cluster[j] >= 0 and not cluster[j] < toff[e + 1] - toff[e]:
                raise ValueError('cluster_profile_numpy: entry %d has id %d, its event has %d clusters'
                                 % (j, cluster[j], toff[e + 1] - toff[e]))
            if cluster[j] >= 0 and not 0 <= index[j] < vox:
                raise ValueError('cluster_profile_numpy: entry %d has index %d outside the volume' % (j, index[j]))
    f = cluster_features_numpy(offsets, index, value, cluster, table_offsets, spatial)
    if value is not None:
        value = np.asarray(value, np.float32).reshape(-1)
    ndim, K = len(spatial), toff[-1]
    step, two16 = np.float64(spec.step), np.float64(2.0 ** FIX_SHIFT)
    members = [[] for _ in range(K)]
    for e in range(len(off) - 1):
        for j in range(off[e], off[e + 1]):
            if cluster[j] >= 0:
                members[toff[e] + int(cluster[j])].append(j)
    bin_offsets = [0]
    bins = {k: [] for k in PROFILE_BIN_INT + PROFILE_BIN_REAL}
    rows = {k: [] for k in PROFILE_ROW_INT + PROFILE_ROW_REAL}
    zero, one = np.float64(0.0), np.float64(1.0)
    for r in range(K):
        m, ax = [int(x) for x in f['m'][r]], [np.float64(x) for x in f['axis'][r]]
        t_lo, length = np.float64(f['t_lo'][r]), np.float64(f['length'][r])
        nb, nb_true, pad = profile_bin_count(length, step, spec.max_bins)
        bn, bq, bf = [0] * nb, [0] * nb, [0] * nb
        bd = [[0, 0, 0] for _ in range(nb)]
        for j in members[r]:
            c = np.unravel_index(int(index[j]), spatial)
            x = [int(c[a]) if a < ndim else 0 for a in range(3)]
            t = (ax[0] * np.float64(x[0] - m[0]) + ax[1] * np.float64(x[1] - m[1])) + ax[2] * np.float64(x[2] - m[2])
            t = np.float32(t)
            if t == np.float32(0.0):
                t = np.float32(0.0)
            u = ((np.float64(t) - t_lo) + pad) / step
            b = min(max(int(np.floor(u)), 0), nb - 1)
            bn[b] += 1
            for a in range(3):
                bd[b][a] += x[a] - m[a]
            if value is not None:
                val = np.float64(value[j])
                if not np.isfinite(val) or abs(val) >= FIX_LIMIT:
                    bf[b] |= 1
                else:
                    bq[b] += int(np.rint(val * two16))
        cents = []
        for b in range(nb):
            assert bn[b] < 2 ** 31 and all(abs(v) < 2 ** 46 for v in bd[b]) and abs(bq[b]) <= 2 ** 62
            if bn[b] > 0:
                c = [np.float64(m[a]) + np.float64(bd[b][a]) / np.float64(bn[b]) for a in range(3)]
                dq = (np.float64(bq[b]) / two16) / step
                cents.append((b, c))
            else:
                c, dq = [zero, zero, zero], zero
            for k, v in zip(PROFILE_BIN_INT, (bn[b], bq[b], bd[b][0], bd[b][1], bd[b][2], bf[b])):
                bins[k].append(v)
            for k, v in zip(PROFILE_BIN_REAL, (c[0], c[1], c[2], dq)):
                bins[k].append(v)
        bin_offsets.append(bin_offsets[-1] + nb)
        filled = len(cents)
        gaps = longest = run = 0
        seen = False
        for b in range(nb):
            if bn[b] > 0:
                if seen and run > 0:
                    gaps, longest = gaps + 1, max(longest, run)
                seen, run = True, 0
            else:
                run += 1
        peak = 0
        for b in range(1, nb):
            if bq[b] > bq[peak]:
                peak = b
        h = min(spec.end_bins, nb // 2)
        head_n, head_q = sum(bn[:h]), sum(bq[:h])
        tail_n, tail_q = sum(bn[nb - h:nb]), sum(bq[nb - h:nb])
        direction = 0 if h == 0 else (1 if tail_q > head_q else -1 if tail_q < head_q else 0)
        flags = (1 if any(bf) else 0) | (2 if nb_true > spec.max_bins else 0)
        path, best, kink = zero, None, np.float64(-1.0)
        prev = None                                               # the segment before: (dx, dy, dz, s)
        for k in range(1, len(cents)):
            d = [cents[k][1][a] - cents[k - 1][1][a] for a in range(3)]
            s = np.sqrt((d[0] * d[0] + d[1] * d[1]) + d[2] * d[2])
            path = path + s
            if prev is not None:
                den = prev[3] * s
                if den != zero:
                    cos = ((prev[0] * d[0] + prev[1] * d[1]) + prev[2] * d[2]) / den
                    if best is None or cos < best:
                        best, kink = cos, np.float64(cents[k - 1][0])
            prev = (d[0], d[1], d[2], s)
        if h > 0:
            head_dqdx = (np.float64(head_q) / two16) / (np.float64(h) * step)
            tail_dqdx = (np.float64(tail_q) / two16) / (np.float64(h) * step)
        else:
            head_dqdx = tail_dqdx = zero
        straight = length / path if path != zero else one
        for k, v in zip(PROFILE_ROW_INT, (nb, filled, gaps, longest, peak, h, head_n, head_q, tail_n, tail_q, direction, flags)):
            rows[k].append(v)
        for k, v in zip(PROFILE_ROW_REAL, (path, one if best is None else best, kink, head_dqdx, tail_dqdx, straight)):
            rows[k].append(v)
    out_bins = {k: np.array(bins[k], np.int64 if k in PROFILE_BIN_INT else np.float64).reshape(-1) for k in bins}
    out_rows = {k: np.array(rows[k], np.int64 if k in PROFILE_ROW_INT else np.float64).reshape(-1) for k in rows}
    return {'objects': f, 'bin_offsets': np.array(bin_offsets, np.int64), 'bins': out_bins, 'rows': out_rows}


# ---- vertex candidates: where cluster end points meet (csrc/cluster_vertex.hip does it on the device; this is the statement) ------
VERTEX_INT = ('ends', 'rows', 'bodies', 'near', 'n', 'charge', 's0', 's1', 's2', 'lo0', 'lo1', 'lo2', 'hi0', 'hi1', 'hi2', 'first_pos',
              'mask_flags')
VERTEX_REAL = ('c0', 'c1', 'c2', 'min_cos', 'max_cos')
VERTEX_INCIDENCE = ('row', 'kind', 'near', 'dist2', 'pos')
VERTEX_EVENT = ('vertices', 'junctions', 'free', 'primary')
VERTEX_MAX_RADIUS = 3
VERTEX_MAX_DIRECTIONS = 16


class ClusterVertexSpec(object):
    """``radius`` in [1, 3]: two end points, or an end point and an entry, are near when their coordinates differ by at most
    ``radius`` on every axis; ``min_size`` >= 1: clusters with fewer members have no end points; ``classes`` None = clusters of
    every class, else distinct class numbers in [0, 32): only clusters of these classes have end points (needs the table's cls)."""

    def __init__(self, radius=2, min_size=3, classes=None):
        if type(radius) is not int or not 1 <= radius <= VERTEX_MAX_RADIUS:
            raise ValueError('ClusterVertexSpec: radius = %r, expected an integer in [1, %d]' % (radius, VERTEX_MAX_RADIUS))
        if type(min_size) is not int or not 1 <= min_size < 2 ** 31:
            raise ValueError('ClusterVertexSpec: min_size = %r, expected an integer >= 1' % (min_size,))
        if classes is not None:
            given = classes
            try:
                classes = tuple(classes)
            except TypeError:
                classes = ()
            if not classes or any(type(c) is not int or not 0 <= c < 32 for c in classes) or len(set(classes)) != len(classes):
                raise ValueError('ClusterVertexSpec: classes = %r, expected None or distinct integers in [0, 32)' % (given,))
        self.radius, self.min_size, self.classes = radius, min_size, classes

    def class_mask(self):
        """Bit k set = clusters of class k have end points; 0 = every class."""
        m = 0
        for c in self.classes or ():
            m |= 1 << c
        return m

    def __repr__(self):
        return 'ClusterVertexSpec(radius=%r, min_size=%r, classes=%r)' % (self.radius, self.min_size, self.classes)


def cluster_vertices_numpy(offsets, index, value, cluster, table_offsets, spatial, spec, cls=None):
    """The statement of the vertex candidates of concatenated per-event lists: which cluster end points meet at one point, how many
    objects leave that point and at what angles, and which clusters pass it with their body.  Slow on purpose, in the style of
    ``cluster_features_numpy``, which it calls first (its result is returned under ``objects``): Python integers, scalar fp64
    operations each rounded on its own, one entry at a time.

    END POINTS.  A global row r is ELIGIBLE when its object record has n >= ``spec.min_size`` and, with ``spec.classes``,
    ``cls[r]`` is one of them.  An eligible row has end points at the list positions ``end_lo[r]`` and ``end_hi[r]`` of its object
    record -- one end point when the two are equal.  The KEY of an end point is 2 r + side, side 0 for end_lo and 1 for end_hi (a
    single end point has side 0); its DIRECTION is u = +axis[r] at the lo end and -axis[r] (unary minus) at the hi end: it points
    from the end into its cluster.  Coordinates are ``np.unravel_index(index, spatial)`` with x[2] = 0 in 2-D; NEAR means a
    difference of at most ``spec.radius`` on every axis (Chebyshev distance, decided on coordinates, never on indices: never across
    a row end, a plane end or an event boundary).

    VERTICES.  Two end points of one event and of DIFFERENT rows are linked when they are near.  A vertex is a connected component
    of end points under links (a lone end point is a vertex with ends = 1); vertices are numbered per event in the order of their
    lowest key, ``vertex_offsets`` [n + 1].

    INCIDENCES.  For every end point p of vertex v and every entry j of the same event with ``cluster[j] >= 0`` near p (j = p
    included) the pair (p, j) counts towards the incidence (v, row of j).  VERTEX_INCIDENCE: ``row`` (event-local); ``kind`` bit
    0 / bit 1 set by the pair (p, p) alone according to p's side -- the set of that row's own ends inside v, 0 = the row passes v
    with its body, 3 = both of its ends are in v; ``near`` the number of such pairs; ``dist2`` / ``pos`` the squared Euclidean
    distance and the list position of j of the pair smallest in (dist2, position of j), dist2 <= 27.  Stored CSR by global vertex,
    ascending row, ``inc_offsets`` [V + 1].

    VERTEX_INT: ``ends``; ``rows`` its incidences; ``bodies`` those of kind 0; ``near`` summed over them; ``n`` / ``charge`` the
    object records' n and fixed-point charge summed over the incident rows; ``s0..2`` the sum of the end-point coordinates;
    ``lo0..2`` / ``hi0..2`` their box; ``first_pos`` the list position of the lowest-key end point; ``mask_flags`` = the class mask
    of the incident rows (bit ``cls``; 0 without ``cls``) | flags << 32, flag bit 0: more than 16 ends, the cosines use the first 16;
    flag bit 1: an incident row with length == 0.  VERTEX_REAL: ``c0..2`` = float64(s[a]) / float64(ends); ``min_cos`` / ``max_cos``
    over the pairs i < k of the first min(ends, 16) end directions in ascending key order, cos = (u_i[0] * u_k[0] + u_i[1] *
    u_k[1]) + u_i[2] * u_k[2], the first pair's value kept unless a later one is strictly smaller / larger; both +0.0 with fewer
    than two ends.

    What the record does NOT decide: two ends with min_cos near -1 and no body are what a track broken in two looks like, three
    ends at right angles what an interaction looks like, one end on a body what a delta ray or a decay looks like -- which of them
    it is, is the consumer's judgement.  Nothing here orders the incidences into parent and child, and ``rows['direction']`` of the
    charge profile says nothing more than it did.

    Per row ``row_vertex`` int32 [K, 2]: the event-local vertex of the lo and the hi end, -1 for a row that is not eligible, both
    equal for a single end point.  VERTEX_EVENT: ``vertices``; ``junctions`` (ends >= 2 or bodies >= 1); ``free`` (the others);
    ``primary`` the vertex largest in (rows, n), the lowest id among equals, -1 without a vertex.

    Bounds, with every extent <= 32768, fewer than 2^30 entries (so that every key is an int32) and K rows: a vertex has at most 2 K
    end points, each with at most
    7^3 = 343 near entries, so near < 2 K * 343 < 2^41; the incident rows of a vertex are distinct rows of one event, so n < 2^31
    and |charge| <= 2^62; |s| < 2^15 * 2^32 = 2^47; dist2 <= 27.

    An id outside its event's rows, a row without a member, an index outside the volume at an entry with an id, an end position
    that is not a member of its row and a cls >= 32 raise ValueError.  Returns a dict: ``objects``; ``vertex_offsets`` int64
    [n + 1]; ``vertices`` {name: [V]} over VERTEX_INT (int64) and VERTEX_REAL (float64); ``inc_offsets`` int64 [V + 1];
    ``incidence`` int64 [I, 5]; ``row_vertex`` int32 [K, 2]; ``events`` int64 [n, 4]."""
    if not isinstance(spec, ClusterVertexSpec):
        raise ValueError('cluster_vertices_numpy: spec = %r, expected a ClusterVertexSpec' % (spec,))
    spatial = tuple(int(s) for s in spatial)
    if len(spatial) not in (2, 3) or any(not 1 <= s <= MAX_EXTENT for s in spatial):
        raise ValueError('cluster_vertices_numpy: spatial = %r, expected 2 or 3 extents in [1, %d]' % (spatial, MAX_EXTENT))
    off = [int(x) for x in np.asarray(offsets).reshape(-1)]
    toff = [int(x) for x in np.asarray(table_offsets).reshape(-1)]
    idx = [int(x) for x in np.asarray(index).reshape(-1)]
    ids = [int(x) for x in np.asarray(cluster).reshape(-1)]
    nev, m, ndim, g = len(off) - 1, len(idx), len(spatial), spec.radius
    if nev < 1 or len(toff) != nev + 1 or len(ids) != m or off[0] != 0 or off[-1] != m or toff[0] != 0 \
            or any(off[e + 1] < off[e] or toff[e + 1] < toff[e] for e in range(nev)):
        raise ValueError('cluster_vertices_numpy: offsets, table offsets and the lists disagree')
    K = toff[-1]
    if cls is not None:
        cls = [int(c) for c in np.asarray(cls).reshape(-1)]
        if len(cls) != K or any(not 0 <= c < 32 for c in cls):
            raise ValueError('cluster_vertices_numpy: cls must hold %d classes in [0, 32)' % K)
    if spec.classes is not None and cls is None:
        raise ValueError('cluster_vertices_numpy: spec.classes = %r needs the cluster table\'s cls' % (spec.classes,))
    vox = 1
    for s in spatial:
        vox *= s
    coords, where = [None] * m, [dict() for _ in range(nev)]
    for e in range(nev):
        for j in range(off[e], off[e + 1]):
            if ids[j] < 0:
                continue
            if not ids[j] < toff[e + 1] - toff[e]:
                raise ValueError('cluster_vertices_numpy: entry %d has id %d, its event has %d clusters' % (j, ids[j], toff[e + 1] - toff[e]))
            if not 0 <= idx[j] < vox:
                raise ValueError('cluster_vertices_numpy: entry %d has index %d outside the volume %r' % (j, idx[j], spatial))
            x = tuple(int(c) for c in np.unravel_index(idx[j], spatial))
            coords[j] = x + (0,) * (3 - ndim)
            where[e][coords[j]] = j
    f = cluster_features_numpy(offsets, index, value, cluster, table_offsets, spatial)    # raises on a row without a member
    event_of = [e for e in range(nev) for _ in range(toff[e + 1] - toff[e])]
    mask = spec.class_mask()
    ends = {}                                             # key -> list position
    for r in range(K):
        if int(f['n'][r]) < spec.min_size or (mask and not (mask >> cls[r]) & 1):
            continue
        e = event_of[r]
        for side, p in ((0, int(f['end_lo'][r])), (1, int(f['end_hi'][r]))):
            if not off[e] <= p < off[e + 1] or ids[p] != r - toff[e]:
                raise ValueError('cluster_vertices_numpy: the end position %d of row %d is not a member of it' % (p, r))
            if side == 0 or p != int(f['end_lo'][r]):
                ends[2 * r + side] = p
    key_at = {p: k for k, p in ends.items()}              # a position is the end of one row only
    steps = [tuple(d[a] - g if a < ndim else 0 for a in range(3)) for d in np.ndindex(*([2 * g + 1] * ndim))]

    entry_event = [e for e in range(nev) for _ in range(off[e], off[e + 1])]

    def near(p):
        """(position, dist2) of every entry with an id near the entry at position p, itself included."""
        for d in steps:
            q = where[entry_event[p]].get(tuple(coords[p][a] + d[a] for a in range(3)))
            if q is not None:
                yield q, d[0] * d[0] + d[1] * d[1] + d[2] * d[2]

    parent = {k: k for k in ends}

    def find(x):
        while parent[x] != x:
            parent[x] = parent[parent[x]]
            x = parent[x]
        return x

    for k in sorted(ends):
        for q, _ in near(ends[k]):
            other = key_at.get(q)
            if other is None or other >> 1 == k >> 1:
                continue
            a, b = find(k), find(other)
            if a != b:
                parent[max(a, b)] = min(a, b)
    vertex_of, vertex_offsets, members = {}, [0], []      # members[v]: the keys of global vertex v, ascending
    for e in range(nev):
        for k in sorted(ends):
            if event_of[k >> 1] != e:
                continue
            root = find(k)
            if root == k:
                vertex_of[k] = len(members)
                members.append([])
            vertex_of[k] = vertex_of[root]                # a root is the lowest key of its vertex: it came first
            members[vertex_of[k]].append(k)
        vertex_offsets.append(len(members))
    V = len(members)
    row_vertex = np.full((K, 2), -1, np.int32)
    for k, v in vertex_of.items():
        r, local = k >> 1, v - vertex_offsets[event_of[k >> 1]]
        row_vertex[r][k & 1] = local
        if int(f['end_lo'][r]) == int(f['end_hi'][r]):
            row_vertex[r][1] = local
    vert = {name: [] for name in VERTEX_INT + VERTEX_REAL}
    inc_offsets, incidence = [0], []
    events = [[vertex_offsets[e + 1] - vertex_offsets[e], 0, 0, -1] for e in range(nev)]
    best = [None] * nev
    zero = np.float64(0.0)
    for v in range(V):
        e = event_of[members[v][0] >> 1]
        cells = {}                                        # global row -> [kind, near, (dist2, pos)]
        for k in members[v]:
            p = ends[k]
            for q, d2 in near(p):
                cell = cells.setdefault(toff[e] + ids[q], [0, 0, None])
                cell[1] += 1
                if q == p:
                    cell[0] |= 1 << (k & 1)
                if cell[2] is None or (d2, q) < cell[2]:
                    cell[2] = (d2, q)
        n_sum = q_sum = near_sum = bodies = cmask = flags = 0
        for r in sorted(cells):
            kind, cnt, (d2, pos) = cells[r]
            assert d2 <= 27 and cnt < 2 * max(K, 1) * 343
            incidence.append([r - toff[e], kind, cnt, d2, pos])
            near_sum, bodies = near_sum + cnt, bodies + (1 if kind == 0 else 0)
            n_sum, q_sum = n_sum + int(f['n'][r]), q_sum + int(f['charge'][r])
            if cls is not None:
                cmask |= 1 << cls[r]
            if f['length'][r] == zero:
                flags |= 2
        inc_offsets.append(len(incidence))
        xs = [coords[ends[k]] for k in members[v]]
        s = [sum(x[a] for x in xs) for a in range(3)]
        assert n_sum < 2 ** 31 and abs(q_sum) <= 2 ** 62 and all(abs(t) < 2 ** 47 for t in s)
        if len(members[v]) > VERTEX_MAX_DIRECTIONS:
            flags |= 1
        us = []
        for k in members[v][:VERTEX_MAX_DIRECTIONS]:
            ax = [np.float64(t) for t in f['axis'][k >> 1]]
            us.append(ax if k & 1 == 0 else [-t for t in ax])
        lo_cos = hi_cos = None
        for i in range(len(us)):
            for k in range(i + 1, len(us)):
                cos = (us[i][0] * us[k][0] + us[i][1] * us[k][1]) + us[i][2] * us[k][2]
                if lo_cos is None:
                    lo_cos = hi_cos = cos
                if cos < lo_cos:
                    lo_cos = cos
                if cos > hi_cos:
                    hi_cos = cos
        fe = np.float64(len(xs))
        ints = [len(xs), len(cells), bodies, near_sum, n_sum, q_sum] + s + [min(x[a] for x in xs) for a in range(3)] + \
            [max(x[a] for x in xs) for a in range(3)] + [ends[members[v][0]], cmask | flags << 32]
        reals = [np.float64(s[a]) / fe for a in range(3)] + [zero if lo_cos is None else lo_cos, zero if hi_cos is None else hi_cos]
        for name, val in zip(VERTEX_INT + VERTEX_REAL, ints + reals):
            vert[name].append(val)
        junction = len(xs) >= 2 or bodies >= 1
        events[e][1] += 1 if junction else 0
        events[e][2] += 0 if junction else 1
        if best[e] is None or (len(cells), n_sum) > best[e]:          # ascending id: a strict comparison keeps the lowest
            best[e], events[e][3] = (len(cells), n_sum), v - vertex_offsets[e]
    vertices = {k: np.array(vert[k], np.int64 if k in VERTEX_INT else np.float64).reshape(-1) for k in vert}
    return {'objects': f, 'vertex_offsets': np.array(vertex_offsets, np.int64), 'vertices': vertices,
            'inc_offsets': np.array(inc_offsets, np.int64), 'incidence': np.array(incidence, np.int64).reshape(-1, 5),
            'row_vertex': row_vertex, 'events': np.array(events, np.int64).reshape(-1, 4)}


# ---- cluster chains: broken track fragments joined end to end (csrc/cluster_chain.hip does it on the device; this is the statement) --
CHAIN_INT = ('rows', 'joins', 'n', 'charge', 'lo0', 'lo1', 'lo2', 'hi0', 'hi1', 'hi2', 'first_row', 'end_a', 'end_b', 'gap2_sum',
             'gap2_max', 'mask_flags')
CHAIN_REAL = ('path', 'gaps', 'span', 'straightness', 'min_cos')
JOIN_INT = ('key_a', 'key_b', 'dist2', 'pos_a', 'pos_b', 'chain')
JOIN_REAL = ('c_ax', 'c_lo', 'c_hi', 'gap')
CHAIN_EVENT = ('chains', 'joins', 'joined', 'longest')
CHAIN_MAX_GAP = 31


class ClusterChainSpec(object):
    """``max_gap`` in [1, 31]: two end points can be joined when their coordinates differ by at most ``max_gap`` on every axis;
    ``min_cos`` a finite float in [0, 1]: the three cosines of a join (axis against axis, gap against either axis) must reach it;
    ``min_size`` >= 1: clusters with fewer members are not joined; ``classes`` None = clusters of every class, else distinct class
    numbers in [0, 32): only clusters of these classes are joined (needs the table's cls); ``same_class`` True = only clusters of
    equal class are joined (needs the table's cls)."""

    def __init__(self, max_gap=6, min_cos=0.9, min_size=3, classes=None, same_class=True):
        if type(max_gap) is not int or not 1 <= max_gap <= CHAIN_MAX_GAP:
            raise ValueError('ClusterChainSpec: max_gap = %r, expected an integer in [1, %d]' % (max_gap, CHAIN_MAX_GAP))
        if type(min_cos) not in (int, float) or not np.isfinite(min_cos) or not 0.0 <= min_cos <= 1.0:
            raise ValueError('ClusterChainSpec: min_cos = %r, expected a finite float in [0, 1]' % (min_cos,))
        if type(min_size) is not int or not 1 <= min_size < 2 ** 31:
            raise ValueError('ClusterChainSpec: min_size = %r, expected an integer >= 1' % (min_size,))
        if classes is not None:
            given = classes
            try:
                classes = tuple(classes)
            except TypeError:
                classes = ()
            if not classes or any(type(c) is not int or not 0 <= c < 32 for c in classes) or len(set(classes)) != len(classes):
                raise ValueError('ClusterChainSpec: classes = %r, expected None or distinct integers in [0, 32)' % (given,))
        if type(same_class) is not bool:
            raise ValueError('ClusterChainSpec: same_class = %r, expected a bool' % (same_class,))
        self.max_gap, self.min_cos, self.min_size, self.classes, self.same_class = max_gap, float(min_cos), min_size, classes, same_class

    def class_mask(self):
        """Bit k set = clusters of class k can be joined; 0 = every class."""
        m = 0
        for c in self.classes or ():
            m |= 1 << c
        return m

    def __repr__(self):
        return 'ClusterChainSpec(max_gap=%r, min_cos=%r, min_size=%r, classes=%r, same_class=%r)' % (
            self.max_gap, self.min_cos, self.min_size, self.classes, self.same_class)


def chain_cosines(u_p, u_q, d):
    """(dist2, c_ax, c_lo, c_hi) of a candidate: ``u_p`` / ``u_q`` the directions of the end points with the lower / higher key,
    ``d`` = x(q) - x(p) as integers.  Every line is one fp64 operation rounded on its own; the device follows it."""
    dist2 = d[0] * d[0] + d[1] * d[1] + d[2] * d[2]
    with np.errstate(divide='ignore', invalid='ignore'):
        s = np.sqrt(np.float64(dist2))
        f = [np.float64(x) for x in d]
        c_ax = -((u_p[0] * u_q[0] + u_p[1] * u_q[1]) + u_p[2] * u_q[2])
        c_lo = (-((u_p[0] * f[0] + u_p[1] * f[1]) + u_p[2] * f[2])) / s
        c_hi = ((u_q[0] * f[0] + u_q[1] * f[1]) + u_q[2] * f[2]) / s
    return dist2, c_ax, c_lo, c_hi


def cluster_chains_numpy(offsets, index, value, cluster, table_offsets, spatial, spec, cls=None):
    """The statement of the cluster chains of concatenated per-event lists: which clusters are fragments of one broken track, joined
    end to end across a gap.  Slow on purpose, in the style of ``cluster_features_numpy``, which it calls first (its result is
    returned under ``objects``): Python integers, scalar fp64 operations each rounded on its own.

    END POINTS.  A global row r is ELIGIBLE when its object record has n >= ``spec.min_size`` and end_lo != end_hi and, with
    ``spec.classes``, ``cls[r]`` is one of them.  An eligible row has two end points, at the list positions ``end_lo[r]`` and
    ``end_hi[r]``; the KEY of an end point is 2 r + side (side 0 = end_lo); its DIRECTION is u = +axis[r] at the lo end and
    -axis[r] (unary minus) at the hi end: it points from the end into its cluster.  Coordinates are ``np.unravel_index(index,
    spatial)`` with x[2] = 0 in 2-D.

    CANDIDATES.  Two end points p < q (by key) of one event and of DIFFERENT rows whose coordinates differ by at most
    ``spec.max_gap`` on every axis and, with ``spec.same_class``, whose rows have equal ``cls``.  Evaluated once, p the lower key
    (``chain_cosines``): d = x(q) - x(p); dist2 = d . d (1 .. 3 * 31^2 = 2883); s = sqrt(float64(dist2));
    c_ax = -((u_p[0] * u_q[0] + u_p[1] * u_q[1]) + u_p[2] * u_q[2]); c_lo = (-((u_p[0] * d0 + u_p[1] * d1) + u_p[2] * d2)) / s;
    c_hi = ((u_q[0] * d0 + u_q[1] * d1) + u_q[2] * d2) / s.  ACCEPTED when c_ax >= min_cos and c_lo >= min_cos and c_hi >= min_cos
    (a NaN rejects): the two bodies point away from each other and the gap vector leaves p's body and enters q's.

    JOINS.  Every end point counts its accepted candidates (``row_candidates``) and picks as BEST the one smallest in (dist2,
    partner key); {p, q} is a JOIN when each is the other's best.  An end point is in at most one join, a row in at most two.

    CHAINS.  Rows linked by joins are unioned; a chain is a component, numbered per event by its lowest row, ``chain_offsets``
    [n + 1]; every row is in exactly one chain (a row without a join is a chain of one).  ``merged[j]`` is the event-local chain
    of ``cluster[j]``'s row, -1 where ``cluster[j]`` is -1.  ``table``: ``first`` int32 = the lowest event-local list position of a
    member, ``size`` int32 = members, ``cls`` uint8 = ``cls`` of the lowest row (0 without ``cls``): with ids numbered by lowest
    position, as ``ursn_cluster_voxels`` numbers them, ``first`` is strictly increasing per event and (merged, chain_offsets,
    table) is a clustering in that call's format.

    CHAIN_INT: ``rows``; ``joins``; ``n`` / ``charge`` summed over the object records; ``lo0..2`` / ``hi0..2`` the union of their
    boxes; ``first_row`` (event-local); ``end_a`` / ``end_b`` list positions (the walk); ``gap2_sum`` / ``gap2_max`` over the
    joins' dist2; ``mask_flags`` = the class mask of the rows (0 without ``cls``) | flags << 32, flag bit 0: a ring (no free end),
    flag bit 1: a member row whose object record has flags != 0.  CHAIN_REAL: ``path``, ``gaps``, ``span``, ``straightness``,
    ``min_cos``.  THE WALK fixes the order of the fp64 sums.  START is the chain's free end point (an end of a member row that is
    in no join; a row that is not eligible counts as having two free ends) with the lowest key; a ring starts at the lo side of
    ``first_row``.  ``end_a`` is START's position.  Enter the start row at that side, then ``rows`` times: path = path +
    length[row]; leave at the other side; if that side is in a join and fewer than ``joins`` joins were taken: g =
    sqrt(float64(dist2)), path = path + g, gaps = gaps + g, min_cos takes the join's c_ax if it is the first or strictly smaller,
    enter the partner row at the partner's side.  ``end_b`` is the position of the end at which the walk leaves its last row;
    span = sqrt(float64(squared distance between the coordinates of end_a and end_b)); straightness = span / path, +0.0 when
    path == 0.0; min_cos and gaps are +0.0 without joins.

    JOINS LIST, CSR by event (``join_offsets`` [n + 1]), ascending key_a.  JOIN_INT: ``key_a`` < ``key_b`` (event-local keys),
    ``dist2``, ``pos_a``, ``pos_b`` (list positions), ``chain`` (event-local).  JOIN_REAL: ``c_ax``, ``c_lo``, ``c_hi``, ``gap`` =
    sqrt(float64(dist2)).  Per row: ``row_chain`` int32 [K]; ``row_join`` int32 [K, 2] the partner's event-local key at the lo /
    hi side, -1 for none; ``row_candidates`` int32 [K, 2].  CHAIN_EVENT: ``chains``, ``joins``, ``joined`` (chains with rows >=
    2), ``longest`` = the chain largest in (rows, n), the lowest id among equals, -1 without chains.

    Bounds, with every extent <= 32768, fewer than 2^30 entries (m_total < 2^30, so that every key is an int32 below 2^31 and
    dist2 << 32 | key fits a 64-bit word) and K rows: at most K joins (an end point is in at most one, and a join takes two);
    n < 2^31 and |charge| <= 2^62 (the rows of a chain are distinct rows of one event); gap2_sum <= 2883 K.

    An id outside its event's rows, a row without a member, an index outside the volume at an entry with an id, an end position
    of an eligible row that is not a member of it and a cls >= 32 raise ValueError.  Returns a dict: ``objects``;
    ``chain_offsets`` int64 [n + 1]; ``merged`` int32 [m]; ``table`` {first, size, cls}; ``chains`` {name: [C]} over CHAIN_INT
    (int64) and CHAIN_REAL (float64); ``join_offsets`` int64 [n + 1]; ``joins`` {name: [J]} over JOIN_INT / JOIN_REAL;
    ``row_chain``; ``row_join``; ``row_candidates``; ``events`` int64 [n, 4]."""
    if not isinstance(spec, ClusterChainSpec):
        raise ValueError('cluster_chains_numpy: spec = %r, expected a ClusterChainSpec' % (spec,))
    spatial = tuple(int(s) for s in spatial)
    if len(spatial) not in (2, 3) or any(not 1 <= s <= MAX_EXTENT for s in spatial):
        raise ValueError('cluster_chains_numpy: spatial = %r, expected 2 or 3 extents in [1, %d]' % (spatial, MAX_EXTENT))
    off = [int(x) for x in np.asarray(offsets).reshape(-1)]
    toff = [int(x) for x in np.asarray(table_offsets).reshape(-1)]
    idx = [int(x) for x in np.asarray(index).reshape(-1)]
    ids = [int(x) for x in np.asarray(cluster).reshape(-1)]
    nev, m, ndim, g = len(off) - 1, len(idx), len(spatial), spec.max_gap
    if nev < 1 or len(toff) != nev + 1 or len(ids) != m or off[0] != 0 or off[-1] != m or toff[0] != 0 \
            or any(off[e + 1] < off[e] or toff[e + 1] < toff[e] for e in range(nev)):
        raise ValueError('cluster_chains_numpy: offsets, table offsets and the lists disagree')
    K = toff[-1]
    if cls is not None:
        cls = [int(c) for c in np.asarray(cls).reshape(-1)]
        if len(cls) != K or any(not 0 <= c < 32 for c in cls):
            raise ValueError('cluster_chains_numpy: cls must hold %d classes in [0, 32)' % K)
    if spec.classes is not None and cls is None:
        raise ValueError('cluster_chains_numpy: spec.classes = %r needs the cluster table\'s cls' % (spec.classes,))
    if spec.same_class and cls is None:
        raise ValueError('cluster_chains_numpy: spec.same_class needs the cluster table\'s cls')
    vox = 1
    for s in spatial:
        vox *= s

    def coords_of(j):
        x = tuple(int(c) for c in np.unravel_index(idx[j], spatial))
        return x + (0,) * (3 - ndim)

    first_pos = [None] * K                                # the lowest event-local position of a member
    for e in range(nev):
        for j in range(off[e], off[e + 1]):
            if ids[j] < 0:
                continue
            if not ids[j] < toff[e + 1] - toff[e]:
                raise ValueError('cluster_chains_numpy: entry %d has id %d, its event has %d clusters' % (j, ids[j], toff[e + 1] - toff[e]))
            if not 0 <= idx[j] < vox:
                raise ValueError('cluster_chains_numpy: entry %d has index %d outside the volume %r' % (j, idx[j], spatial))
            r = toff[e] + ids[j]
            if first_pos[r] is None:
                first_pos[r] = j - off[e]
    f = cluster_features_numpy(offsets, index, value, cluster, table_offsets, spatial)    # raises on a row without a member
    event_of = [e for e in range(nev) for _ in range(toff[e + 1] - toff[e])]
    mask, min_cos = spec.class_mask(), np.float64(spec.min_cos)
    ends, xs, us = {}, {}, {}                             # key -> list position, coordinates, direction
    for r in range(K):
        lo, hi = int(f['end_lo'][r]), int(f['end_hi'][r])
        if int(f['n'][r]) < spec.min_size or lo == hi or (mask and not (mask >> cls[r]) & 1):
            continue
        e = event_of[r]
        ax = [np.float64(t) for t in f['axis'][r]]
        for side, p in ((0, lo), (1, hi)):
            if not off[e] <= p < off[e + 1] or ids[p] != r - toff[e]:
                raise ValueError('cluster_chains_numpy: the end position %d of row %d is not a member of it' % (p, r))
            ends[2 * r + side], xs[2 * r + side], us[2 * r + side] = p, coords_of(p), (ax if side == 0 else [-t for t in ax])
    by_event = [[] for _ in range(nev)]
    for k in sorted(ends):
        by_event[event_of[k >> 1]].append(k)
    accepted = {}                                         # (p, q), p < q -> (dist2, c_ax, c_lo, c_hi)
    ncand = {k: 0 for k in ends}
    best = {}                                             # key -> (dist2, partner key)

    def consider(p, q):
        if p >> 1 == q >> 1 or (spec.same_class and cls[p >> 1] != cls[q >> 1]):
            return
        d = [xs[q][a] - xs[p][a] for a in range(3)]
        if any(abs(t) > g for t in d):
            return
        dist2, c_ax, c_lo, c_hi = chain_cosines(us[p], us[q], d)
        assert 1 <= dist2 <= 3 * CHAIN_MAX_GAP ** 2
        if c_ax >= min_cos and c_lo >= min_cos and c_hi >= min_cos:
            accepted[(p, q)] = (dist2, c_ax, c_lo, c_hi)
            for a, b in ((p, q), (q, p)):
                ncand[a] += 1
                if a not in best or (dist2, b) < best[a]:
                    best[a] = (dist2, b)

    for keys in by_event:
        if len(keys) <= (2 * g + 1) ** 2:                 # few end points: every pair
            for i, p in enumerate(keys):
                for q in keys[i + 1:]:
                    consider(p, q)
        else:                                             # many: by column (x0, x1)
            cols = {}
            for k in keys:
                cols.setdefault(xs[k][:2], []).append(k)
            for p in keys:
                for d0 in range(-g, g + 1):
                    for d1 in range(-g, g + 1):
                        for q in cols.get((xs[p][0] + d0, xs[p][1] + d1), ()):
                            if q > p:
                                consider(p, q)
    partner = {k: best[k][1] for k in best if best.get(best[k][1], (0, -1))[1] == k}
    assert len(partner) <= 2 * K and len(partner) % 2 == 0
    parent = list(range(K))

    def find(x):
        while parent[x] != x:
            parent[x] = parent[parent[x]]
            x = parent[x]
        return x

    for k in sorted(partner):
        if k < partner[k]:
            a, b = find(k >> 1), find(partner[k] >> 1)
            if a != b:
                parent[max(a, b)] = min(a, b)
    chain_of, chain_offsets, members = [0] * K, [0], []   # members[c]: the rows of global chain c, ascending
    for e in range(nev):
        for r in range(toff[e], toff[e + 1]):
            root = find(r)
            if root == r:
                chain_of[r] = len(members)
                members.append([])
            chain_of[r] = chain_of[root]                  # a root is the lowest row of its chain: it came first
            members[chain_of[r]].append(r)
        chain_offsets.append(len(members))
    C = len(members)
    merged = np.full(m, -1, np.int32)
    for e in range(nev):
        for j in range(off[e], off[e + 1]):
            if ids[j] >= 0:
                merged[j] = chain_of[toff[e] + ids[j]] - chain_offsets[e]
    row_chain = np.array([chain_of[r] - chain_offsets[event_of[r]] for r in range(K)], np.int32).reshape(K)
    row_join, row_candidates = np.full((K, 2), -1, np.int32), np.zeros((K, 2), np.int32)
    for k in ends:
        row_candidates[k >> 1][k & 1] = ncand[k]
        if k in partner:
            row_join[k >> 1][k & 1] = partner[k] - 2 * toff[event_of[k >> 1]]
    chains = {name: [] for name in CHAIN_INT + CHAIN_REAL}
    table = {'first': [], 'size': [], 'cls': []}
    events = [[chain_offsets[e + 1] - chain_offsets[e], 0, 0, -1] for e in range(nev)]
    longest = [None] * nev
    zero = np.float64(0.0)

    def cand(a, b):
        return accepted[(min(a, b), max(a, b))]

    for c in range(C):
        rows = members[c]
        e = event_of[rows[0]]
        n_sum = sum(int(f['n'][r]) for r in rows)
        q_sum = sum(int(f['charge'][r]) for r in rows)
        joined = [k for r in rows for k in (2 * r, 2 * r + 1) if k in partner]
        free = [k for r in rows for k in (2 * r, 2 * r + 1) if k not in partner]
        njoin = len(joined) // 2
        d2s = [cand(k, partner[k])[0] for k in joined if k < partner[k]]
        cmask = flags = 0
        for r in rows:
            if cls is not None:
                cmask |= 1 << cls[r]
            if int(f['flags'][r]) != 0:
                flags |= 2
        if not free:
            flags |= 1
        start = min(free) if free else 2 * rows[0]
        pos = lambda k: int(f['end_hi' if k & 1 else 'end_lo'][k >> 1])
        path = gaps = zero
        lowest, taken = None, 0
        row, side = start >> 1, start & 1
        out = start
        for _ in range(len(rows)):
            path = path + np.float64(f['length'][row])
            out = 2 * row + (1 - side)
            if out in partner and taken < njoin:
                dist2, c_ax, _, _ = cand(out, partner[out])
                gap = np.sqrt(np.float64(dist2))
                path = path + gap
                gaps = gaps + gap
                if lowest is None or c_ax < lowest:
                    lowest = c_ax
                taken += 1
                row, side = partner[out] >> 1, partner[out] & 1
        end_a, end_b = pos(start), pos(out)
        xa, xb = coords_of(end_a), coords_of(end_b)
        span = np.sqrt(np.float64(sum((xa[a] - xb[a]) ** 2 for a in range(3))))
        assert n_sum < 2 ** 31 and abs(q_sum) <= 2 ** 62 and taken == njoin <= len(rows)
        ints = [len(rows), njoin, n_sum, q_sum] + [min(int(f['lo'][r][a]) for r in rows) for a in range(3)] + \
            [max(int(f['hi'][r][a]) for r in rows) for a in range(3)] + [rows[0] - toff[e], end_a, end_b, sum(d2s), max(d2s + [0]),
                                                                        cmask | flags << 32]
        reals = [path, gaps, span, span / path if path != zero else zero, zero if lowest is None else lowest]
        for name, val in zip(CHAIN_INT + CHAIN_REAL, ints + reals):
            chains[name].append(val)
        table['first'].append(min(first_pos[r] for r in rows))
        table['size'].append(n_sum)
        table['cls'].append(cls[rows[0]] if cls is not None else 0)
        events[e][1] += njoin
        events[e][2] += 1 if len(rows) >= 2 else 0
        if longest[e] is None or (len(rows), n_sum) > longest[e]:             # ascending id: a strict comparison keeps the lowest
            longest[e], events[e][3] = (len(rows), n_sum), c - chain_offsets[e]
    joins = {name: [] for name in JOIN_INT + JOIN_REAL}
    join_offsets = [0]
    for e in range(nev):
        for k in by_event[e]:                             # ascending key
            if k in partner and k < partner[k]:
                q = partner[k]
                dist2, c_ax, c_lo, c_hi = accepted[(k, q)]
                vals = [k - 2 * toff[e], q - 2 * toff[e], dist2, ends[k], ends[q], chain_of[k >> 1] - chain_offsets[e], c_ax, c_lo, c_hi,
                        np.sqrt(np.float64(dist2))]
                for name, val in zip(JOIN_INT + JOIN_REAL, vals):
                    joins[name].append(val)
        join_offsets.append(len(joins['key_a']))
    assert join_offsets[-1] <= K
    return {'objects': f, 'chain_offsets': np.array(chain_offsets, np.int64), 'merged': merged,
            'table': {'first': np.array(table['first'], np.int32).reshape(-1), 'size': np.array(table['size'], np.int32).reshape(-1),
                      'cls': np.array(table['cls'], np.uint8).reshape(-1)},
            'chains': {k: np.array(chains[k], np.int64 if k in CHAIN_INT else np.float64).reshape(-1) for k in chains},
            'join_offsets': np.array(join_offsets, np.int64),
            'joins': {k: np.array(joins[k], np.int64 if k in JOIN_INT else np.float64).reshape(-1) for k in joins},
            'row_chain': row_chain, 'row_join': row_join, 'row_candidates': row_candidates,
            'events': np.array(events, np.int64).reshape(-1, 4)}


# ---- cluster cones: shower fragments gathered to their primary (csrc/cluster_cone.hip does it on the device; this is the statement) --
CONE_INT = ('rows', 'n', 'charge', 'lo0', 'lo1', 'lo2', 'hi0', 'hi1', 'hi2', 'first_row', 'primary', 'start', 'depth', 'dist2_max',
            'primary_n', 'mask_flags')
CONE_REAL = ('primary_fraction', 'min_cos', 't_max', 'r_max')
LINK_INT = ('child', 'apex', 'dist2', 'pos', 'shower', 'depth')
LINK_REAL = ('c_cone', 't', 'r', 'c_ax')
CONE_EVENT = ('showers', 'links', 'grouped', 'largest')
CONE_MAX_REACH = 127


class ClusterConeSpec(object):
    """``reach`` in [1, 127]: the largest distance from an apex to a child's anchor (per axis and Euclidean); ``min_cos`` a finite
    float in (0, 1]: the smallest accepted cosine, of the cone and, for a child with an axis of its own, of the two axes;
    ``seed_size`` >= 2: rows with fewer members are no parent; ``min_size`` >= 1: rows with fewer members are no child;
    ``classes`` None = rows of every class, else distinct class numbers in [0, 32): only rows of these classes take part (needs the
    table's cls); ``same_class`` True = only rows of equal class are linked (needs the table's cls)."""

    def __init__(self, reach=48, min_cos=0.8, seed_size=8, min_size=1, classes=None, same_class=True):
        if type(reach) is not int or not 1 <= reach <= CONE_MAX_REACH:
            raise ValueError('ClusterConeSpec: reach = %r, expected an integer in [1, %d]' % (reach, CONE_MAX_REACH))
        if type(min_cos) not in (int, float) or not np.isfinite(min_cos) or not 0.0 < min_cos <= 1.0:
            raise ValueError('ClusterConeSpec: min_cos = %r, expected a finite float in (0, 1]' % (min_cos,))
        if type(seed_size) is not int or not 2 <= seed_size < 2 ** 31:
            raise ValueError('ClusterConeSpec: seed_size = %r, expected an integer >= 2' % (seed_size,))
        if type(min_size) is not int or not 1 <= min_size < 2 ** 31:
            raise ValueError('ClusterConeSpec: min_size = %r, expected an integer >= 1' % (min_size,))
        if classes is not None:
            given = classes
            try:
                classes = tuple(classes)
            except TypeError:
                classes = ()
            if not classes or any(type(c) is not int or not 0 <= c < 32 for c in classes) or len(set(classes)) != len(classes):
                raise ValueError('ClusterConeSpec: classes = %r, expected None or distinct integers in [0, 32)' % (given,))
        if type(same_class) is not bool:
            raise ValueError('ClusterConeSpec: same_class = %r, expected a bool' % (same_class,))
        self.reach, self.min_cos, self.seed_size, self.min_size = reach, float(min_cos), seed_size, min_size
        self.classes, self.same_class = classes, same_class

    def class_mask(self):
        """Bit k set = rows of class k take part; 0 = every class."""
        m = 0
        for c in self.classes or ():
            m |= 1 << c
        return m

    def __repr__(self):
        return 'ClusterConeSpec(reach=%r, min_cos=%r, seed_size=%r, min_size=%r, classes=%r, same_class=%r)' % (
            self.reach, self.min_cos, self.seed_size, self.min_size, self.classes, self.same_class)


def cone_link(u, a, d):
    """(t, c_cone, c_ax) of a candidate: ``u`` the direction of the apex, ``a`` the axis of the child or None when the child has
    none to speak of (c_ax is then +0.0), ``d`` = anchor(child) - x(apex) as integers.  Every line is one fp64 operation rounded on
    its own; the device follows it."""
    dist2 = d[0] * d[0] + d[1] * d[1] + d[2] * d[2]
    with np.errstate(divide='ignore', invalid='ignore'):
        s = np.sqrt(np.float64(dist2))
        f = [np.float64(x) for x in d]
        t = (u[0] * f[0] + u[1] * f[1]) + u[2] * f[2]
        c_cone = t / s
        c_ax = np.float64(0.0) if a is None else np.fabs((u[0] * a[0] + u[1] * a[1]) + u[2] * a[2])
    return t, c_cone, c_ax


def cluster_cones_numpy(offsets, index, value, cluster, table_offsets, spatial, spec, cls=None):
    """The statement of the shower cones of concatenated per-event lists: which clusters are fragments of one electromagnetic
    shower, gathered to the cluster they came from.  Slow on purpose, in the style of ``cluster_chains_numpy``: it calls
    ``cluster_features_numpy`` first (returned under ``objects``); Python integers, scalar fp64 operations each rounded on its own.

    ELIGIBILITY.  A global row C is CHILD-eligible when its object record has n >= ``spec.min_size`` and, with ``spec.classes``,
    ``cls[C]`` is one of them.  A global row P is PARENT-eligible when n >= ``spec.seed_size`` and end_lo != end_hi under the same
    class condition.  A parent has two APEXES, at the list positions ``end_lo[P]`` and ``end_hi[P]``, with the KEY 2 P + side (side
    0 = end_lo) and the DIRECTION u = +axis[P] at the lo end, -axis[P] (unary minus) at the hi end: from the end into the row.  A
    child is represented by its anchor ``m[C]``.  Coordinates are ``np.unravel_index(index, spatial)`` with x[2] = 0 in 2-D.

    RANK.  P OUTRANKS C when n_P > n_C, or n_P == n_C and P < C: a strict total order, so links never form a cycle.

    CANDIDATES.  A child C and an apex (P, side) of different rows of one event, P outranking C and, with ``spec.same_class``, of
    equal ``cls``; d = m[C] - x(apex) as integers with |d_a| <= reach on every axis and 1 <= dist2 = d . d <= reach^2.
    ``cone_link``: s = sqrt(float64(dist2)); t = (u[0] * d0 + u[1] * d1) + u[2] * d2; c_cone = t / s; c_ax = fabs((u[0] * a0 +
    u[1] * a1) + u[2] * a2) with a = axis[C], formed only when C is itself PARENT-eligible.  ACCEPTED when c_cone >= min_cos and,
    where c_ax is formed, c_ax >= min_cos (a NaN rejects).

    LINKS.  Every child counts its accepted candidates (``row_candidates``) and takes as its PARENT apex the accepted candidate
    smallest in (dist2, apex key): a LINK.  No mutual test: a parent may have many children; a row has at most one parent.

    SHOWERS.  The links form a forest; a SHOWER is a tree, its PRIMARY the root, a row's ``depth`` its links to the root.  Showers
    are numbered per event by their lowest row, ``shower_offsets`` [n + 1]; a row with no link at all is a shower of one.
    ``merged[j]`` is the event-local shower of ``cluster[j]``'s row, -1 where ``cluster[j]`` is -1.  ``table``: ``first`` int32 =
    the lowest event-local list position of a member, ``size`` int32 = members, ``cls`` uint8 = ``cls`` of the PRIMARY (0 without
    ``cls``): (merged, shower_offsets, table) is a clustering in the format ``ursn_cluster_voxels`` writes.

    CONE_INT: ``rows``; ``n`` / ``charge`` summed over the object records; ``lo0..2`` / ``hi0..2`` the union of their boxes;
    ``first_row`` (event-local lowest row); ``primary`` (event-local); ``start`` = the list position of the primary's apex on the
    START side: the side with the larger summed n of its DIRECT children, among equals the side with more direct children, then
    side 0 (a primary that is not parent-eligible: end_lo); ``depth`` the largest of a row; ``dist2_max`` over the links;
    ``primary_n``; ``mask_flags`` = the class mask of the rows (0 without ``cls``) | flags << 32, flag bit 0: the primary has direct
    children at both apexes, flag bit 1: a member row whose object record has flags != 0.  CONE_REAL: ``primary_fraction`` =
    float64(primary_n) / float64(n); ``min_cos`` the smallest c_cone and ``t_max`` the largest t over the links, +0.0 without;
    ``r_max`` = sqrt(float64(dist2_max)).

    LINK LIST, CSR by event (``link_offsets`` [n + 1]), ascending child row.  LINK_INT: ``child`` (event-local row), ``apex``
    (event-local key), ``dist2``, ``pos`` (list position of the apex), ``shower`` (event-local), ``depth`` (of the child).
    LINK_REAL: ``c_cone``, ``t``, ``r`` = s, ``c_ax`` (+0.0 where it was not formed).  Per row: ``row_shower`` int32 [K];
    ``row_parent`` int32 [K] the event-local apex key, -1 for none; ``row_candidates`` int32 [K]; ``row_children`` int32 [K, 2]
    direct children at the lo / hi apex; ``row_depth`` int32 [K].  CONE_EVENT: ``showers``, ``links``, ``grouped`` (showers with
    rows >= 2), ``largest`` = the shower largest in (rows, n), the lowest id among equals, -1 without showers.

    Bounds, with K rows: at most K links (a row has at most one parent); dist2 <= 127^2 = 16129; fewer than 2^30 entries so that
    dist2 << 32 | apex key fits a 64-bit word with keys below 2^31; n < 2^31 and |charge| <= 2^62.

    An id outside its event's rows, a row without a member, an index outside the volume at an entry with an id, an end position of
    a parent-eligible row that is not a member of it and a cls >= 32 raise ValueError.  Returns a dict: ``objects``;
    ``shower_offsets`` int64 [n + 1]; ``merged`` int32 [m]; ``table`` {first, size, cls}; ``showers`` {name: [S]} over CONE_INT
    (int64) and CONE_REAL (float64); ``link_offsets`` int64 [n + 1]; ``links`` {name: [L]} over LINK_INT / LINK_REAL;
    ``row_shower``; ``row_parent``; ``row_candidates``; ``row_children``; ``row_depth``; ``events`` int64 [n, 4]."""
    if not isinstance(spec, ClusterConeSpec):
        raise ValueError('cluster_cones_numpy: spec = %r, expected a ClusterConeSpec' % (spec,))
    spatial = tuple(int(s) for s in spatial)
    if len(spatial) not in (2, 3) or any(not 1 <= s <= MAX_EXTENT for s in spatial):
        raise ValueError('cluster_cones_numpy: spatial = %r, expected 2 or 3 extents in [1, %d]' % (spatial, MAX_EXTENT))
    off = [int(x) for x in np.asarray(offsets).reshape(-1)]
    toff = [int(x) for x in np.asarray(table_offsets).reshape(-1)]
    idx = [int(x) for x in np.asarray(index).reshape(-1)]
    ids = [int(x) for x in np.asarray(cluster).reshape(-1)]
    nev, m, ndim, reach = len(off) - 1, len(idx), len(spatial), spec.reach
    if nev < 1 or len(toff) != nev + 1 or len(ids) != m or off[0] != 0 or off[-1] != m or toff[0] != 0 \
            or any(off[e + 1] < off[e] or toff[e + 1] < toff[e] for e in range(nev)):
        raise ValueError('cluster_cones_numpy: offsets, table offsets and the lists disagree')
    K = toff[-1]
    if cls is not None:
        cls = [int(c) for c in np.asarray(cls).reshape(-1)]
        if len(cls) != K or any(not 0 <= c < 32 for c in cls):
            raise ValueError('cluster_cones_numpy: cls must hold %d classes in [0, 32)' % K)
    if spec.classes is not None and cls is None:
        raise ValueError('cluster_cones_numpy: spec.classes = %r needs the cluster table\'s cls' % (spec.classes,))
    if spec.same_class and cls is None:
        raise ValueError('cluster_cones_numpy: spec.same_class needs the cluster table\'s cls')
    vox = 1
    for s in spatial:
        vox *= s

    def coords_of(j):
        x = tuple(int(c) for c in np.unravel_index(idx[j], spatial))
        return x + (0,) * (3 - ndim)

    first_pos = [None] * K                                # the lowest event-local position of a member
    for e in range(nev):
        for j in range(off[e], off[e + 1]):
            if ids[j] < 0:
                continue
            if not ids[j] < toff[e + 1] - toff[e]:
                raise ValueError('cluster_cones_numpy: entry %d has id %d, its event has %d clusters' % (j, ids[j], toff[e + 1] - toff[e]))
            if not 0 <= idx[j] < vox:
                raise ValueError('cluster_cones_numpy: entry %d has index %d outside the volume %r' % (j, idx[j], spatial))
            r = toff[e] + ids[j]
            if first_pos[r] is None:
                first_pos[r] = j - off[e]
    f = cluster_features_numpy(offsets, index, value, cluster, table_offsets, spatial)    # raises on a row without a member
    event_of = [e for e in range(nev) for _ in range(toff[e + 1] - toff[e])]
    mask, min_cos = spec.class_mask(), np.float64(spec.min_cos)
    size = [int(f['n'][r]) for r in range(K)]
    anchor = [tuple(int(t) for t in f['m'][r]) for r in range(K)]
    in_class = [not mask or bool((mask >> cls[r]) & 1) for r in range(K)]
    child_ok = [size[r] >= spec.min_size and in_class[r] for r in range(K)]
    parent_ok = [size[r] >= spec.seed_size and int(f['end_lo'][r]) != int(f['end_hi'][r]) and in_class[r] for r in range(K)]
    axis = [[np.float64(t) for t in f['axis'][r]] for r in range(K)]
    pos_of, xs, us = {}, {}, {}                           # apex key -> list position, coordinates, direction
    cells = [{} for _ in range(nev)]                      # per event: (x // reach on every axis) -> apex keys, ascending
    for r in range(K):
        if not parent_ok[r]:
            continue
        e = event_of[r]
        for side, p in ((0, int(f['end_lo'][r])), (1, int(f['end_hi'][r]))):
            if not off[e] <= p < off[e + 1] or ids[p] != r - toff[e]:
                raise ValueError('cluster_cones_numpy: the end position %d of row %d is not a member of it' % (p, r))
            k = 2 * r + side
            pos_of[k], xs[k], us[k] = p, coords_of(p), (axis[r] if side == 0 else [-t for t in axis[r]])
            cells[e].setdefault(tuple(c // reach for c in xs[k]), []).append(k)
    ncand = [0] * K
    link = [None] * K                                     # child row -> (dist2, apex key, t, c_cone, c_ax)
    for c in range(K):
        if not child_ok[c]:
            continue
        e, mc = event_of[c], anchor[c]
        home = tuple(t // reach for t in mc)
        for g0 in (home[0] - 1, home[0], home[0] + 1):
            for g1 in (home[1] - 1, home[1], home[1] + 1):
                for g2 in (home[2] - 1, home[2], home[2] + 1):
                    for k in cells[e].get((g0, g1, g2), ()):
                        p = k >> 1
                        if p == c or not (size[p] > size[c] or (size[p] == size[c] and p < c)):
                            continue
                        if spec.same_class and cls[p] != cls[c]:
                            continue
                        d = [mc[a] - xs[k][a] for a in range(3)]
                        dist2 = d[0] * d[0] + d[1] * d[1] + d[2] * d[2]
                        if any(abs(t) > reach for t in d) or not 1 <= dist2 <= reach * reach:
                            continue
                        t, c_cone, c_ax = cone_link(us[k], axis[c] if parent_ok[c] else None, d)
                        if not c_cone >= min_cos or (parent_ok[c] and not c_ax >= min_cos):
                            continue
                        ncand[c] += 1
                        if link[c] is None or (dist2, k) < link[c][:2]:
                            link[c] = (dist2, k, t, c_cone, c_ax)
    assert all(lk is None or 1 <= lk[0] <= CONE_MAX_REACH ** 2 for lk in link)
    root, depth = [0] * K, [0] * K
    for r in range(K):
        x, h = r, 0
        while link[x] is not None:                        # rank strictly rises: the walk ends
            x, h = link[x][1] >> 1, h + 1
            assert h <= K
        root[r], depth[r] = x, h
    lowest = {}                                           # root -> the lowest row of its tree
    for r in range(K):
        lowest.setdefault(root[r], r)
    shower_of, shower_offsets, members = [0] * K, [0], []  # members[s]: the rows of global shower s, ascending
    for e in range(nev):
        for r in range(toff[e], toff[e + 1]):
            if lowest[root[r]] == r:
                lowest[root[r]] = -1 - len(members)       # from now on: the shower's number
                members.append([])
            shower_of[r] = -1 - lowest[root[r]]
            members[shower_of[r]].append(r)
        shower_offsets.append(len(members))
    S = len(members)
    merged = np.full(m, -1, np.int32)
    for e in range(nev):
        for j in range(off[e], off[e + 1]):
            if ids[j] >= 0:
                merged[j] = shower_of[toff[e] + ids[j]] - shower_offsets[e]
    row_shower = np.array([shower_of[r] - shower_offsets[event_of[r]] for r in range(K)], np.int32).reshape(K)
    row_parent = np.array([-1 if link[r] is None else link[r][1] - 2 * toff[event_of[r]] for r in range(K)], np.int32).reshape(K)
    row_candidates = np.array(ncand, np.int32).reshape(K)
    row_depth = np.array(depth, np.int32).reshape(K)
    row_children = np.zeros((K, 2), np.int32)
    child_n = [[0, 0] for _ in range(K)]                  # summed n of the direct children at the lo / hi apex
    for r in range(K):
        if link[r] is not None:
            k = link[r][1]
            row_children[k >> 1][k & 1] += 1
            child_n[k >> 1][k & 1] += size[r]
    showers = {name: [] for name in CONE_INT + CONE_REAL}
    table = {'first': [], 'size': [], 'cls': []}
    events = [[shower_offsets[e + 1] - shower_offsets[e], 0, 0, -1] for e in range(nev)]
    largest = [None] * nev
    zero = np.float64(0.0)
    for s in range(S):
        rows = members[s]
        e, prim = event_of[rows[0]], root[rows[0]]
        n_sum = sum(size[r] for r in rows)
        q_sum = sum(int(f['charge'][r]) for r in rows)
        links = [link[r] for r in rows if link[r] is not None]
        cmask = flags = 0
        for r in rows:
            if cls is not None:
                cmask |= 1 << cls[r]
            if int(f['flags'][r]) != 0:
                flags |= 2
        kids = row_children[prim]
        if kids[0] > 0 and kids[1] > 0:
            flags |= 1
        side = 0
        if parent_ok[prim]:
            if child_n[prim][1] > child_n[prim][0] or (child_n[prim][1] == child_n[prim][0] and kids[1] > kids[0]):
                side = 1
        start = int(f['end_hi' if side else 'end_lo'][prim])
        d2max = max([lk[0] for lk in links] + [0])
        assert n_sum < 2 ** 31 and abs(q_sum) <= 2 ** 62 and len(links) == len(rows) - 1
        ints = [len(rows), n_sum, q_sum] + [min(int(f['lo'][r][a]) for r in rows) for a in range(3)] + \
            [max(int(f['hi'][r][a]) for r in rows) for a in range(3)] + \
            [rows[0] - toff[e], prim - toff[e], start, max(depth[r] for r in rows), d2max, size[prim], cmask | flags << 32]
        reals = [np.float64(size[prim]) / np.float64(n_sum), min([lk[3] for lk in links]) if links else zero,
                 max([lk[2] for lk in links]) if links else zero, np.sqrt(np.float64(d2max))]
        for name, val in zip(CONE_INT + CONE_REAL, ints + reals):
            showers[name].append(val)
        table['first'].append(min(first_pos[r] for r in rows))
        table['size'].append(n_sum)
        table['cls'].append(cls[prim] if cls is not None else 0)
        events[e][1] += len(links)
        events[e][2] += 1 if len(rows) >= 2 else 0
        if largest[e] is None or (len(rows), n_sum) > largest[e]:             # ascending id: a strict comparison keeps the lowest
            largest[e], events[e][3] = (len(rows), n_sum), s - shower_offsets[e]
    links = {name: [] for name in LINK_INT + LINK_REAL}
    link_offsets = [0]
    for e in range(nev):
        for r in range(toff[e], toff[e + 1]):             # ascending child row
            if link[r] is not None:
                dist2, k, t, c_cone, c_ax = link[r]
                vals = [r - toff[e], k - 2 * toff[e], dist2, pos_of[k], shower_of[r] - shower_offsets[e], depth[r], c_cone, t,
                        np.sqrt(np.float64(dist2)), c_ax]
                for name, val in zip(LINK_INT + LINK_REAL, vals):
                    links[name].append(val)
        link_offsets.append(len(links['child']))
    assert link_offsets[-1] <= K
    return {'objects': f, 'shower_offsets': np.array(shower_offsets, np.int64), 'merged': merged,
            'table': {'first': np.array(table['first'], np.int32).reshape(-1), 'size': np.array(table['size'], np.int32).reshape(-1),
                      'cls': np.array(table['cls'], np.uint8).reshape(-1)},
            'showers': {k: np.array(showers[k], np.int64 if k in CONE_INT else np.float64).reshape(-1) for k in showers},
            'link_offsets': np.array(link_offsets, np.int64),
            'links': {k: np.array(links[k], np.int64 if k in LINK_INT else np.float64).reshape(-1) for k in links},
            'row_shower': row_shower, 'row_parent': row_parent, 'row_candidates': row_candidates, 'row_children': row_children,
            'row_depth': row_depth, 'events': np.array(events, np.int64).reshape(-1, 4)}


# ---- cluster splits: a component of several particles cut at its junctions and kinks (csrc/cluster_split.hip does it on the
# device; this is the statement) --------------------------------------------------------------------------------------------------
SPLIT_PIECE = ('row', 'n', 'attached', 'kind', 'key', 'contacts', 'junction_lo', 'junction_hi')
SPLIT_JUNCTION_INT = ('row', 'entries', 'attached', 'arms_max', 'kinks', 's0', 's1', 's2', 'lo0', 'lo1', 'lo2', 'hi0', 'hi1', 'hi2',
                      'first_pos', 'contacts', 'piece_lo', 'piece_hi')
SPLIT_JUNCTION_REAL = ('c0', 'c1', 'c2')
SPLIT_ROW = ('pieces', 'junctions', 'cut')
SPLIT_EVENT = ('pieces', 'junctions', 'rows_cut', 'cut')
SPLIT_MAX_RADIUS = 3
SPLIT_MAX_GROW = 8
SPLIT_MAX_ARMS = 15
_SPLIT_NEIGHBOURS = tuple((a, b, c) for a in (-1, 0, 1) for b in (-1, 0, 1) for c in (-1, 0, 1) if (a, b, c) != (0, 0, 0))


class ClusterSplitSpec(object):
    """``radius`` in [1, 3]: the Chebyshev radius of the ball in which the arms of a voxel are counted; ``kink_cos`` a float in
    [-1, 1]: a voxel with exactly two arms is cut when the cosine between them exceeds it (straight is -1), a value >= 1 switches
    kinks off; ``min_size`` >= 1: rows whose table ``size`` is smaller stay whole; ``classes`` None = rows of every class, else
    distinct class numbers in [0, 32): only rows of these classes are split (needs the table's cls); ``grow`` in [0, 8]: the
    rounds in which the cut voxels are handed back to the pieces that touch them, None = 2 * radius."""

    def __init__(self, radius=2, kink_cos=-0.7, min_size=8, classes=None, grow=None):
        if type(radius) is not int or not 1 <= radius <= SPLIT_MAX_RADIUS:
            raise ValueError('ClusterSplitSpec: radius = %r, expected an integer in [1, %d]' % (radius, SPLIT_MAX_RADIUS))
        if type(kink_cos) not in (int, float) or not np.isfinite(kink_cos) or not -1.0 <= kink_cos <= 1.0:
            raise ValueError('ClusterSplitSpec: kink_cos = %r, expected a finite float in [-1, 1]' % (kink_cos,))
        if type(min_size) is not int or not 1 <= min_size < 2 ** 31:
            raise ValueError('ClusterSplitSpec: min_size = %r, expected an integer >= 1' % (min_size,))
        if classes is not None:
            given = classes
            try:
                classes = tuple(classes)
            except TypeError:
                classes = ()
            if not classes or any(type(c) is not int or not 0 <= c < 32 for c in classes) or len(set(classes)) != len(classes):
                raise ValueError('ClusterSplitSpec: classes = %r, expected None or distinct integers in [0, 32)' % (given,))
        if grow is None:
            grow = 2 * radius
        if type(grow) is not int or not 0 <= grow <= SPLIT_MAX_GROW:
            raise ValueError('ClusterSplitSpec: grow = %r, expected None or an integer in [0, %d]' % (grow, SPLIT_MAX_GROW))
        self.radius, self.kink_cos, self.min_size, self.classes, self.grow = radius, float(kink_cos), min_size, classes, grow

    def class_mask(self):
        """Bit k set = rows of class k are split; 0 = every class."""
        m = 0
        for c in self.classes or ():
            m |= 1 << c
        return m

    def __repr__(self):
        return 'ClusterSplitSpec(radius=%r, kink_cos=%r, min_size=%r, classes=%r, grow=%r)' % (
            self.radius, self.kink_cos, self.min_size, self.classes, self.grow)


def cluster_split_numpy(offsets, index, cluster, table_offsets, size, spatial, spec, cls=None):
    """The statement of the cluster split of concatenated per-event lists: a connected component that holds several particles
    (prongs of one vertex, crossing tracks, a kinked track) is cut where it branches or bends, and the pieces come back as one more
    clustering of the same lists.  Slow on purpose, in the style of ``cluster_chains_numpy``: Python integers, scalar fp64
    operations each rounded on its own.  Lists are row-major in ``spatial`` and strictly increasing per event; coordinates are
    ``np.unravel_index(index, spatial)`` with x[2] = 0 in 2-D.  A POSITION is a place in the concatenated list.

    ADJACENT.  Two different entries of one event whose coordinates differ by at most 1 on every axis: full adjacency, whatever
    connectivity made the clustering, decided on coordinates (never on linear indices: the last voxel of a row and the first of
    the next are not adjacent); cells outside the volume are empty.

    ELIGIBLE.  A global row r with ``size[r] >= spec.min_size`` and, with ``spec.classes``, ``cls[r]`` one of them.

    ARMS, for every member j of an eligible row R.  BALL(j): the members of R within Chebyshev distance ``radius`` of x(j).
    REACH(j): the entries of BALL(j) joined to j by a path of adjacent entries inside BALL(j) (a parallel limb of R that merely
    passes within ``radius`` is not reached).  SHELL(j): the entries of REACH(j) at Chebyshev distance exactly ``radius``.  The
    ARMS are the connected components of SHELL(j) under adjacency among shell entries; arms(j) = min(their number, 15).  An end
    sees 1 arm, a body 2, a junction 3 or more; a stub shorter than ``radius`` reaches no shell and makes no arm.

    KINK, evaluated only with exactly 2 arms and kink_cos < 1.  s_a = the integer sum of x(q) - x(j) over arm a; dot = s_1 . s_2,
    q_a = s_a . s_a; with both q_a > 0: c = float64(dot) / (sqrt(float64(q_1)) * sqrt(float64(q_2))) and KINK iff c > kink_cos (the
    product of the two roots commutes, so the order of the arms does not matter).

    CUT.  j is cut when arms(j) >= 3 or KINK.

    PIECES AND JUNCTIONS.  Among the entries of eligible rows, adjacent entries of the same row with the same cut status are
    joined.  Uncut components are PIECES of kind 1, cut components are JUNCTIONS.  A row that is not eligible is ONE piece of kind
    0, whole, connected or not.  An eligible row that is itself disconnected (a chain of ``cluster_chains``, say) falls into its
    components: the split belongs BEFORE the chains and cones.

    ATTACHMENT, in rounds t = 1 .. ``grow``.  A cut entry that has no piece yet looks at its adjacent entries of the same row that
    are uncut or were attached in a round before t; if there are any it takes the piece of the one at the lowest position.  Round t
    reads only what earlier rounds wrote.  What a junction still holds after the last round is one piece of kind 2 (connected or
    not).

    NUMBERING.  Pieces are numbered per event in ascending KEY: for kinds 0 and 1 the lowest position of the original members (for
    kind 1 the uncut component), for kind 2 the lowest position of the junction's entries before attachment.  Junctions are
    numbered per event by their lowest position.  With attachment a piece's ``first`` need not ascend with its id.

    CONTACT.  An ordered pair (cut entry, adjacent uncut entry of its row), taken before attachment.

    Outputs.  ``split`` int32 [m]: the event-local piece, -1 where ``cluster`` is -1.  ``piece_offsets`` / ``junction_offsets``
    int64 [n + 1].  ``table``: ``first`` int32 = the lowest event-local position of the final members, ``size`` int32 = the final
    members, ``cls`` uint8 = the row's cls (0 without cls).  ``mark`` uint8 [m] = arms | junction << 4 | kink << 5 | attached << 6,
    0 for entries that were not evaluated (junction: the entry is cut).  SPLIT_PIECE int64: ``row`` (event-local), ``n`` (final
    members), ``attached`` (of them, attached cut entries), ``kind``, ``key`` (a position), ``contacts`` (contacts whose uncut
    entry is an original member), ``junction_lo`` / ``junction_hi`` the smallest / largest event-local junction among those
    contacts, -1 for none; a piece of kind 2 has contacts 0 and names its own junction in both.  SPLIT_JUNCTION_INT int64: ``row``,
    ``entries``, ``attached`` (entries handed to pieces), ``arms_max``, ``kinks`` (entries with KINK), ``s0..2`` the coordinate
    sums, ``lo0..2`` / ``hi0..2`` the box, ``first_pos`` (its lowest position), ``contacts``, ``piece_lo`` / ``piece_hi`` the
    smallest / largest event-local piece among its contacts' uncut entries, -1 for none.  SPLIT_JUNCTION_REAL: ``c0..2`` =
    float64(s) / float64(entries): the vertex position that ``cluster_vertices`` cannot see.  ``rows`` int32 [K, 3] over
    SPLIT_ROW: pieces, junctions, cut entries.  ``events`` int64 [n, 4] over SPLIT_EVENT: pieces, junctions, rows with a junction,
    cut entries.

    An id outside its event's rows, an index outside the volume at an entry with an id, a list that does not increase strictly
    inside an event and a cls >= 32 raise ValueError."""
    if not isinstance(spec, ClusterSplitSpec):
        raise ValueError('cluster_split_numpy: spec = %r, expected a ClusterSplitSpec' % (spec,))
    spatial = tuple(int(s) for s in spatial)
    if len(spatial) not in (2, 3) or any(not 1 <= s <= MAX_EXTENT for s in spatial):
        raise ValueError('cluster_split_numpy: spatial = %r, expected 2 or 3 extents in [1, %d]' % (spatial, MAX_EXTENT))
    off = [int(x) for x in np.asarray(offsets).reshape(-1)]
    toff = [int(x) for x in np.asarray(table_offsets).reshape(-1)]
    idx = [int(x) for x in np.asarray(index).reshape(-1)]
    ids = [int(x) for x in np.asarray(cluster).reshape(-1)]
    sizes = [int(x) for x in np.asarray(size).reshape(-1)]
    nev, m, ndim, rad = len(off) - 1, len(idx), len(spatial), spec.radius
    if nev < 1 or len(toff) != nev + 1 or len(ids) != m or off[0] != 0 or off[-1] != m or toff[0] != 0 \
            or any(off[e + 1] < off[e] or toff[e + 1] < toff[e] for e in range(nev)):
        raise ValueError('cluster_split_numpy: offsets, table offsets and the lists disagree')
    K = toff[-1]
    if len(sizes) != K:
        raise ValueError('cluster_split_numpy: size must hold %d rows' % K)
    if cls is not None:
        cls = [int(c) for c in np.asarray(cls).reshape(-1)]
        if len(cls) != K or any(not 0 <= c < 32 for c in cls):
            raise ValueError('cluster_split_numpy: cls must hold %d classes in [0, 32)' % K)
    if spec.classes is not None and cls is None:
        raise ValueError('cluster_split_numpy: spec.classes = %r needs the cluster table\'s cls' % (spec.classes,))
    vox = 1
    for s in spatial:
        vox *= s
    ext = spatial + (1,) * (3 - ndim)
    mask, kink_cos = spec.class_mask(), np.float64(spec.kink_cos)
    eligible = [sizes[r] >= spec.min_size and (not mask or bool((mask >> cls[r]) & 1)) for r in range(K)]
    event_of_row = [e for e in range(nev) for _ in range(toff[e + 1] - toff[e])]
    row_of, xs, event_of = [-1] * m, [None] * m, [0] * m
    at = [{} for _ in range(nev)]                         # per event: coordinates -> position, entries with an id only
    for e in range(nev):
        for j in range(off[e], off[e + 1]):
            event_of[j] = e
            if j > off[e] and idx[j] <= idx[j - 1]:
                raise ValueError('cluster_split_numpy: entry %d does not increase the list of event %d' % (j, e))
            if ids[j] < 0:
                continue
            if not ids[j] < toff[e + 1] - toff[e]:
                raise ValueError('cluster_split_numpy: entry %d has id %d, its event has %d clusters' % (j, ids[j], toff[e + 1] - toff[e]))
            if not 0 <= idx[j] < vox:
                raise ValueError('cluster_split_numpy: entry %d has index %d outside the volume %r' % (j, idx[j], spatial))
            row_of[j] = toff[e] + ids[j]
            x = tuple(int(c) for c in np.unravel_index(idx[j], spatial)) + (0,) * (3 - ndim)
            xs[j] = x
            at[e][x] = j

    def neighbours(j):
        """The adjacent entries of j's row, ascending position (= ascending coordinates, the lists being sorted)."""
        x, out = xs[j], []
        for d in _SPLIT_NEIGHBOURS:
            y = (x[0] + d[0], x[1] + d[1], x[2] + d[2])
            if all(0 <= y[a] < ext[a] for a in range(3)):
                q = at[event_of[j]].get(y)
                if q is not None and row_of[q] == row_of[j]:
                    out.append(q)
        return sorted(out)

    def flood(seed, allowed):
        """The offsets of ``allowed`` joined to ``seed`` by steps of adjacency inside ``allowed``."""
        seen, todo = {seed}, [seed]
        while todo:
            d = todo.pop()
            for s in _SPLIT_NEIGHBOURS:
                y = (d[0] + s[0], d[1] + s[1], d[2] + s[2])
                if y in allowed and y not in seen:
                    seen.add(y)
                    todo.append(y)
        return seen

    mark = np.zeros(m, np.uint8)
    arms_of, cut, kink = [0] * m, [False] * m, [False] * m
    for j in range(m):
        r = row_of[j]
        if r < 0 or not eligible[r]:
            continue
        x, e = xs[j], event_of[j]
        # REACH by a search from j that never leaves the ball: the same set as the flood of BALL(j) from j
        reach, todo = {(0, 0, 0)}, [(0, 0, 0)]
        while todo:
            d = todo.pop()
            for s in _SPLIT_NEIGHBOURS:
                y = (d[0] + s[0], d[1] + s[1], d[2] + s[2])
                if y in reach or max(abs(y[0]), abs(y[1]), abs(y[2])) > rad:
                    continue
                c = (x[0] + y[0], x[1] + y[1], x[2] + y[2])
                if not all(0 <= c[a] < ext[a] for a in range(3)):
                    continue
                q = at[e].get(c)
                if q is not None and row_of[q] == r:
                    reach.add(y)
                    todo.append(y)
        shell = set(d for d in reach if max(abs(d[0]), abs(d[1]), abs(d[2])) == rad)
        arms = []
        while shell:
            arm = flood(min(shell), shell)
            arms.append(arm)
            shell -= arm
        arms_of[j] = min(len(arms), SPLIT_MAX_ARMS)
        if len(arms) == 2 and spec.kink_cos < 1.0:
            s1 = [sum(d[a] for d in arms[0]) for a in range(3)]
            s2 = [sum(d[a] for d in arms[1]) for a in range(3)]
            dot = s1[0] * s2[0] + s1[1] * s2[1] + s1[2] * s2[2]
            q1 = s1[0] * s1[0] + s1[1] * s1[1] + s1[2] * s1[2]
            q2 = s2[0] * s2[0] + s2[1] * s2[1] + s2[2] * s2[2]
            if q1 > 0 and q2 > 0:
                c = np.float64(dot) / (np.sqrt(np.float64(q1)) * np.sqrt(np.float64(q2)))
                kink[j] = bool(c > kink_cos)
        cut[j] = arms_of[j] >= 3 or kink[j]
    # components of equal cut status inside the eligible rows; the root of a component is its lowest position
    parent = list(range(m))

    def find(x):
        while parent[x] != x:
            parent[x] = parent[parent[x]]
            x = parent[x]
        return x

    nbrs = [None] * m
    for j in range(m):
        if row_of[j] >= 0 and eligible[row_of[j]]:
            nbrs[j] = neighbours(j)
            for q in nbrs[j]:
                if q < j and cut[q] == cut[j]:
                    a, b = find(j), find(q)
                    if a != b:
                        parent[max(a, b)] = min(a, b)
    row_first = [None] * K
    for j in range(m):
        if row_of[j] >= 0 and row_first[row_of[j]] is None:
            row_first[row_of[j]] = j
    root = [find(j) if nbrs[j] is not None else -1 for j in range(m)]
    # attachment
    piece_key, stamp = [-1] * m, [0] * m                   # the key of the piece an entry ends in; the round that attached it
    for j in range(m):
        r = row_of[j]
        if r >= 0:
            piece_key[j] = row_first[r] if not eligible[r] else root[j] if not cut[j] else -1
    for t in range(1, spec.grow + 1):
        taken = []
        for j in range(m):
            if nbrs[j] is not None and cut[j] and stamp[j] == 0:
                for q in nbrs[j]:                         # ascending position
                    if not cut[q] or 0 < stamp[q] < t:
                        taken.append((j, piece_key[q]))
                        break
        for j, key in taken:                              # written after the round has read
            piece_key[j], stamp[j] = key, t
    for j in range(m):
        if nbrs[j] is not None and cut[j] and stamp[j] == 0:
            piece_key[j] = root[j]                        # the remainder of its junction: kind 2
    # numbering
    piece_id, junction_id = {}, {}                        # key -> global number
    piece_offsets, junction_offsets = [0], [0]
    for e in range(nev):
        for key in sorted(set(piece_key[j] for j in range(off[e], off[e + 1]) if piece_key[j] >= 0)):
            piece_id[key] = len(piece_id)
        for key in sorted(set(root[j] for j in range(off[e], off[e + 1]) if root[j] >= 0 and cut[j])):
            junction_id[key] = len(junction_id)
        piece_offsets.append(len(piece_id))
        junction_offsets.append(len(junction_id))
    P, J = len(piece_id), len(junction_id)
    split = np.full(m, -1, np.int32)
    pieces = [[0] * len(SPLIT_PIECE) for _ in range(P)]
    junctions = [[0] * len(SPLIT_JUNCTION_INT) for _ in range(J)]
    first = [None] * P
    rows = np.zeros((K, 3), np.int32)
    events = [[piece_offsets[e + 1] - piece_offsets[e], junction_offsets[e + 1] - junction_offsets[e], 0, 0] for e in range(nev)]
    for key, g in piece_id.items():
        r = row_of[key]
        e = event_of_row[r]
        pieces[g][0], pieces[g][3], pieces[g][4] = r - toff[e], 0 if not eligible[r] else 2 if cut[key] else 1, key
        pieces[g][6] = pieces[g][7] = junction_id[key] - junction_offsets[e] if eligible[r] and cut[key] else -1
        rows[r][0] += 1
    for key, g in junction_id.items():
        r = row_of[key]
        e = event_of_row[r]
        t = junctions[g]
        t[0], t[14], t[16], t[17] = r - toff[e], key, -1, -1
        t[8:11], t[11:14] = list(xs[key]), list(xs[key])
        rows[r][1] += 1
        if rows[r][1] == 1:
            events[e][2] += 1
    for j in range(m):
        if row_of[j] < 0:
            continue
        e, r = event_of[j], row_of[j]
        g = piece_id[piece_key[j]]
        split[j] = g - piece_offsets[e]
        pieces[g][1] += 1
        pieces[g][2] += 1 if stamp[j] > 0 else 0
        if first[g] is None:
            first[g] = j - off[e]
        mark[j] = arms_of[j] | (16 if cut[j] else 0) | (32 if kink[j] else 0) | (64 if stamp[j] > 0 else 0)
        if not cut[j]:
            continue
        jg = junction_id[root[j]]
        t = junctions[jg]
        t[1] += 1
        t[2] += 1 if stamp[j] > 0 else 0
        t[3] = max(t[3], arms_of[j])
        t[4] += 1 if kink[j] else 0
        for a in range(3):
            t[5 + a] += xs[j][a]
            t[8 + a], t[11 + a] = min(t[8 + a], xs[j][a]), max(t[11 + a], xs[j][a])
        rows[r][2] += 1
        events[e][3] += 1
        for q in nbrs[j]:
            if cut[q]:
                continue
            pg = piece_id[root[q]]                        # the piece q was a member of before attachment
            pl, jl = pg - piece_offsets[e], jg - junction_offsets[e]
            t[15] += 1
            t[16], t[17] = pl if t[16] < 0 else min(t[16], pl), max(t[17], pl)
            u = pieces[pg]
            u[5] += 1
            u[6], u[7] = jl if u[6] < 0 else min(u[6], jl), max(u[7], jl)
    centroid = [[np.float64(t[5 + a]) / np.float64(t[1]) for a in range(3)] for t in junctions]
    prow = [toff[event_of[p[4]]] + p[0] for p in pieces]
    return {'split': split, 'mark': mark, 'piece_offsets': np.array(piece_offsets, np.int64),
            'junction_offsets': np.array(junction_offsets, np.int64),
            'table': {'first': np.array(first, np.int32).reshape(-1), 'size': np.array([p[1] for p in pieces], np.int32).reshape(-1),
                      'cls': np.array([cls[r] if cls is not None else 0 for r in prow], np.uint8).reshape(-1)},
            'pieces': {k: np.array([p[c] for p in pieces], np.int64).reshape(-1) for c, k in enumerate(SPLIT_PIECE)},
            'junctions': dict([(k, np.array([t[c] for t in junctions], np.int64).reshape(-1)) for c, k in enumerate(SPLIT_JUNCTION_INT)] +
                              [(k, np.array([c3[a] for c3 in centroid], np.float64).reshape(-1)) for a, k in enumerate(SPLIT_JUNCTION_REAL)]),
            'rows': rows, 'events': np.array(events, np.int64).reshape(-1, 4)}
