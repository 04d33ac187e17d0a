"""Expected results for voxel lists longer than the pure-Python statements can reach.  Plain helper module, not a
conftest; importable without a GPU.

Two constructions.  REPLICATED EVENTS: events are independent and every id is event-local, so the statement is run once on a base
batch of a few thousand entries and the result of the batch repeated R times is formed with numpy alone -- per-event tables tile,
offsets arrays are cumulative sums, and only the columns the definitions state as positions in the whole batch (``end_lo`` /
``end_hi`` of the object records, ``pos_a`` / ``pos_b`` of the edges) move by the replica's list offset.  RUN LATTICE: one long
event of x-runs that touch nothing, whose clustering is a cumulative sum over run starts.  tests/test_long_lists_host.py proves
both against the statements at sizes those can reach, and that every case of CASES crosses the threshold it is named for."""
import collections

import numpy as np

from uresnet_amd import _lib
from uresnet_amd.clusters import (ClusterGraphSpec, ClusterSpec, cluster_features_numpy, cluster_graph_numpy, cluster_match_numpy,
                                  cluster_numpy)

# ---- the thresholds, as the sources state them (tests/test_long_lists_host.py reads the sources and compares) ------------------
VOX_ITER = 8                       # voxel_io.hip:125  #define VOX_ITER 8
VOX_SPAN = 256 * VOX_ITER          # voxel_io.hip:126  voxels per workgroup of the count / write passes
CL_ITER = 8                        # cluster.hip:39    #define CL_ITER 8
CL_SPAN = 256 * CL_ITER            # cluster.hip:40    list positions per workgroup of the count / rank passes
VOXEL_SCAN_THREADS = 1024          # voxel_io.hip:251  voxel_scan_kernel <<<dim3(1), dim3(1024)>>>, chunk = ceil(B / 1024)
CLUSTER_SCAN_THREADS = 1024        # cluster.hip:414   cluster_scan_kernel <<<dim3(1), dim3(1024)>>>
CROP_SCAN_THREADS = 1024           # tiling.hip:306    crop_scan_kernel <<<dim3(1), dim3(1024)>>>, chunk = ceil(boxes / 1024)
CG_SCAN_THREADS = 1024             # cluster_graph.hip:49   per = ceil(K / CG_SCAN_THREADS) rows per thread of clgraph_scan
CM_SCAN_THREADS = 1024             # cluster_match.hip:39   per = ceil(rows / CM_SCAN_THREADS) of clmatch_scan
CF_ROW_BLOCKS = 1024               # cluster_features.hip:36  workgroup cap of the per-row kernels
CF_I = _lib.CLFEAT_I               # cluster_features.hip:32  int64 cells per row that clfeat_init clears
CF_INIT_THREADS = 4 * CF_ROW_BLOCKS * 256      # cluster_features.hip:495  clfeat_init: at most 4 * CF_ROW_BLOCKS workgroups of 256
CF_ROW256_THREADS = CF_ROW_BLOCKS * 256        # cluster_features.hip:491  clfeat_anchor / clfeat_ends: CF_ROW_BLOCKS x 256
CF_ROW64_THREADS = 4 * CF_ROW_BLOCKS * 64      # cluster_features.hip:492  clfeat_axis: 4 * CF_ROW_BLOCKS x 64
CM_GRID_CAP = 16384                # cluster_match.hip:38   cm_grid(items) = min(ceil(items / 256), CM_GRID_CAP)
CG_GRID_CAP = 16384                # cluster_graph.hip:48   cg_grid(items) = min(ceil(items / 256), CG_GRID_CAP)
CM_STRIDE = CM_GRID_CAP * 256      # items one trip of a striding match kernel covers
CG_STRIDE = CG_GRID_CAP * 256      # ... and of a graph kernel
EVENT_BLOCK = 256                  # cluster_match.hip:529  clmatch_event: one thread per event, ceil(n / 256) workgroups


def cdiv(a, b):
    return -(-int(a) // int(b))


def pow2_at_least(x):
    t = 2
    while t < x:
        t <<= 1
    return t


def match_slots(m_total):
    """cm_slots (cluster_match.hip:433): the power of two at or above 2 * max(m_total, 1)."""
    return pow2_at_least(2 * max(int(m_total), 1))


def graph_slots(edge_cap):
    """cg_slots (cluster_graph.hip:667): the power of two at or above 2 * edge_cap + 2."""
    return pow2_at_least(2 * int(edge_cap) + 2)


def scan_chunks(items, threads=1024):
    """The one-workgroup scans: (chunk, [lo, hi) of the last thread that owns something, [lo, hi) of the last thread)."""
    chunk = cdiv(items, threads)
    span = lambda t: (min(t * chunk, items), min(t * chunk + chunk, items))
    last_owner = cdiv(items, chunk) - 1 if items else 0
    return chunk, span(last_owner), span(threads - 1)


# ---- lists -----------------------------------------------------------------------------------------------------------------------
Batch = collections.namedtuple("Batch", "shape off index cls value")


def _batch(shape, lists, classes, seed):
    off = np.concatenate([[0], np.cumsum([x.size for x in lists])]).astype(np.int64)
    index = np.concatenate(lists).astype(np.int64) if lists else np.zeros(0, np.int64)
    cls = np.concatenate(classes).astype(np.uint8) if classes else np.zeros(0, np.uint8)
    value = np.random.default_rng(seed).uniform(-3.0, 40.0, index.size).astype(np.float32)
    return Batch(tuple(shape), off, index, cls, value)


def repeat(b, R):
    """The batch R times over: R * n events, every list unchanged."""
    off = np.concatenate([[0], np.cumsum(np.tile(np.diff(b.off), R))]).astype(np.int64)
    return Batch(b.shape, off, np.tile(b.index, R), np.tile(b.cls, R), np.tile(b.value, R))


def random_base(seed=0, shape=(20, 16, 22), occupancy=0.5):
    """List (a): three events, the middle one empty, random occupancy and three classes."""
    rng = np.random.default_rng(seed)
    V = int(np.prod(shape))
    lists = [np.flatnonzero(rng.uniform(size=V) < occupancy) if e != 1 else np.zeros(0, np.int64) for e in range(3)]
    return _batch(shape, lists, [rng.integers(0, 3, x.size) for x in lists], seed + 100)


SPEC_PER_CLASS = ClusterSpec(26, (0, 1, 2), True, 2)       # list (a)'s ids; side B of its match
SPEC_ANY_CLASS = ClusterSpec(26, (0, 1, 2), False, 1)      # side A of its match
SPEC_ROWS = ClusterSpec(26, None, True, 1)                 # the own-rows and small-event batches


def own_rows_base(seed=1, pairs_join=False, shape=(16, 16, 16), pairs=5):
    """Three events of isolated voxels on the stride-2 lattice (classes 1 and 2): every entry a cluster of its own.  Each event
    also has `pairs` voxels at an odd last coordinate next to a lattice voxel, the lattice site beyond them cleared: of the other
    class (two rows that touch: an edge and a group of two) or, with pairs_join, of the same class (one two-voxel cluster)."""
    rng = np.random.default_rng(seed)
    sites = np.stack(np.meshgrid(*[np.arange(0, s, 2) for s in shape], indexing="ij"), -1).reshape(-1, 3)
    lists, classes = [], []
    for e, keep in enumerate((0.8, 0.6, 0.7)):
        occ = {tuple(int(c) for c in x): int(rng.integers(1, 3)) for x in sites[rng.uniform(size=sites.shape[0]) < keep]}
        chosen = [x for x in sorted(occ) if x[2] + 1 < shape[2]]
        for k in rng.choice(len(chosen), pairs, replace=False):
            a, b, c = chosen[int(k)]
            if (a, b, c - 1) in occ:                      # a pair voxel of the site before: leave this site alone
                continue
            occ.pop((a, b, c + 2), None)
            occ[(a, b, c + 1)] = occ[(a, b, c)] if pairs_join else 3 - occ[(a, b, c)]
        idx = np.ravel_multi_index(np.array(sorted(occ)).T, shape)
        order = np.argsort(idx)
        lists.append(idx[order]), classes.append(np.array([occ[x] for x in sorted(occ)])[order])
    return _batch(shape, lists, classes, seed + 100)


def small_events(n, m_total, seed, shape=(6, 6, 6), empty_runs=((40, 340), (2000, 2350))):
    """n events of 0 to 6 entries: the first and the last empty, runs of consecutive empty events (the [first, last) ranges of
    empty_runs, clipped to n), some events whose entries are all of class 0 (ids all -1).  The sizes are drawn, then
    trimmed from the back until they sum to m_total."""
    rng = np.random.default_rng(seed)
    V = int(np.prod(shape))
    sizes = rng.integers(0, 7, n)
    sizes[0] = sizes[-1] = 0
    for a, b in empty_runs:
        sizes[min(a, n):min(b, n)] = 0
    e = n - 2
    while sizes.sum() > m_total:                           # trim: more events than entries when m_total < n
        sizes[e] = max(0, sizes[e] - (int(sizes.sum()) - m_total))
        e -= 1
    assert sizes.sum() == m_total, (int(sizes.sum()), m_total)
    lists = [np.sort(rng.choice(V, int(s), replace=False)) for s in sizes]
    classes = [rng.integers(0, 3, int(s)) for s in sizes]
    for e in np.flatnonzero(sizes)[::9]:
        classes[e][:] = 0                                  # every entry of the event gets id -1
    return _batch(shape, lists, classes, seed + 100)


# ---- the statements on a batch ---------------------------------------------------------------------------------------------------
def cluster_statement(b, spec):
    """cluster_numpy per event: ids [M], counts [n], the table back to back (``first`` is a position inside its event), offsets."""
    ids, first, size, tcls, counts = [], [], [], [], []
    for e in range(b.off.size - 1):
        lo, hi = int(b.off[e]), int(b.off[e + 1])
        c, f, s, t = cluster_numpy(b.index[lo:hi], b.cls[lo:hi], b.shape, spec)
        ids.append(c), first.append(f), size.append(s), tcls.append(t), counts.append(f.size)
    cat = lambda parts, dt: np.concatenate(parts).astype(dt)
    return {"cluster": cat(ids, np.int32), "count": np.array(counts, np.int32), "first": cat(first, np.int32),
            "size": cat(size, np.int32), "cls": cat(tcls, np.uint8),
            "table_offsets": np.concatenate([[0], np.cumsum(counts)]).astype(np.int64)}


def reversed_ids(cl, off):
    """The same rows numbered from the back of their event (side B of the own-rows match): every row keeps its members."""
    K = np.diff(cl["table_offsets"])
    ev = np.repeat(np.arange(K.size), np.diff(off))
    out = dict(cl)
    out["cluster"] = np.where(cl["cluster"] >= 0, K[ev] - 1 - cl["cluster"], -1).astype(np.int32)
    return out


def features_statement(b, cl):
    return cluster_features_numpy(b.off, b.index, b.value, cl["cluster"], cl["table_offsets"], b.shape)


def match_statement(b, cl_a, cl_b):
    return cluster_match_numpy(b.off, cl_a["cluster"], cl_a["table_offsets"], cl_b["cluster"], cl_b["table_offsets"], b.value)


def graph_statement(b, cl, gap=1):
    return cluster_graph_numpy(b.off, b.index, cl["cluster"], cl["table_offsets"], b.shape, ClusterGraphSpec(gap), b.value, cl["cls"])


# ---- the result of the batch repeated R times, from the result of the batch -------------------------------------------------------
def _tile(a, R):
    return np.tile(a, (R,) + (1,) * (a.ndim - 1))


def _cum(offsets, R):
    return np.concatenate([[0], np.cumsum(np.tile(np.diff(offsets), R))]).astype(np.int64)


def _shifts(per_replica_rows, R, m_base):
    """The list offset of its replica for every row of a table of `per_replica_rows` rows per replica."""
    return np.repeat(np.arange(R, dtype=np.int64) * int(m_base), per_replica_rows)


def tile_cluster(w, R):
    """Every column is event-local (``first`` counts from its event's first entry, cluster.hip:317 `j - lo`)."""
    out = {k: _tile(w[k], R) for k in ("cluster", "count", "first", "size", "cls")}
    out["table_offsets"] = _cum(w["table_offsets"], R)
    return out


def tile_features(w, R, m_base):
    """``end_lo`` / ``end_hi`` are list positions 'global across the batch' (clusters.py, cluster_features_numpy): they move."""
    out = {k: _tile(v, R) for k, v in w.items()}
    K = w["n"].shape[0]
    for k in ("end_lo", "end_hi"):
        out[k] = out[k] + _shifts(K, R, m_base)
    return out


def tile_match(w, R):
    """No column is a list position: ``best`` and ``pair_b`` are event-local ids; ``pair_offsets`` is CSR over all A rows."""
    out = {k: _tile(w[k], R) for k in ("a_int", "b_int", "a_real", "b_real", "event_int", "event_real", "pair_b", "pair_n", "pair_q")}
    out["pair_offsets"] = _cum(w["pair_offsets"], R)
    return out


def tile_graph(w, R, m_base):
    """``pos_a`` / ``pos_b`` (columns 4, 5 of the edges) are 'positions in the concatenated list' (clusters.py, GRAPH_EDGE): they
    move.  ``b``, ``group``, ``nearest`` and ``first_row`` are event-local; the two offsets arrays are cumulative."""
    out = {k: _tile(w[k], R) for k in ("edges", "rows", "groups", "events", "group")}
    out["edges"][:, 4:6] += _shifts(w["edges"].shape[0], R, m_base)[:, None]
    out["edge_offsets"], out["group_offsets"] = _cum(w["edge_offsets"], R), _cum(w["group_offsets"], R)
    return out


# ---- the run lattice -------------------------------------------------------------------------------------------------------------
_PATTERN = np.array([1, 0, 1, 1, 0, 1, 1, 1, 0, 0, 1, 1, 1, 1, 0], bool)       # runs of 1, 2, 3, 4 with gaps 1, 1, 2, 1


def run_lattice(shape, min_size=1):
    """One event in `shape` (3 extents): x-runs of length 1 to 4 along the last axis (the pattern above, started at another phase
    in every row, cut off by the row end), on every second row of every second plane, so no two runs touch under connectivity 26.
    Run k has class 1 + k % 3.  Returns (Batch, expected) with the expected clustering of ClusterSpec(26, None, True, min_size):
    ids are a cumulative sum over run starts; runs shorter than min_size are dropped and the rest renumbered."""
    D0, D1, S = (int(s) for s in shape)
    rows = np.arange(D0 * D1)
    used = ((rows // D1) % 2 == 0) & ((rows % D1) % 2 == 0)
    phase = (rows * 7) % _PATTERN.size
    mask = _PATTERN[(np.arange(S)[None, :] + phase[:, None]) % _PATTERN.size] & used[:, None]
    index = np.flatnonzero(mask.reshape(-1))
    start = np.ones(index.size, bool)
    start[1:] = (index[1:] != index[:-1] + 1) | (index[1:] % S == 0)
    run = np.cumsum(start) - 1
    size = np.bincount(run)
    first = np.flatnonzero(start)
    run_cls = (1 + np.arange(size.size) % 3).astype(np.uint8)
    keep = size >= min_size
    new_id = np.where(keep, np.cumsum(keep) - 1, -1)
    K = int(keep.sum())
    want = {"cluster": new_id[run].astype(np.int32), "count": np.array([K], np.int32), "first": first[keep].astype(np.int32),
            "size": size[keep].astype(np.int32), "cls": run_cls[keep], "table_offsets": np.array([0, K], np.int64)}
    value = np.random.default_rng(7).uniform(-3.0, 40.0, index.size).astype(np.float32)
    return Batch((D0, D1, S), np.array([0, index.size], np.int64), index, run_cls[run], value), want


# ---- the GPU cases ------------------------------------------------------------------------------------------------------------------
# name: the test case; crosses: the threshold(s) it is named for (keys of tests/test_long_lists_host.CROSSES); n events, m_total
# entries (labels_*: voxels per event), rows (cluster table rows; match: of either side), boxes, edge_cap.  tests/test_long_lists_gpu
# asserts that what it builds has exactly these numbers; the host test does the arithmetic.
Case = collections.namedtuple("Case", "name crosses n m_total rows boxes edge_cap")

LABELS_3D = (132, 128, 129)
LABELS_2D = (1112, 1888)                        # 2^21 + 2048 + 256 pixels
LATTICE = (209, 200, 301)
LATTICE_SMALL = [(5, 6, 301), (7, 9, 47), (3, 4, 600)]      # 301, 47: no multiple of the pattern's 15: runs end at the row end
CROP_BIG, CROP_TILE, CROP_HALO = (100, 124), (8, 8), 1
R_RANDOM = 299
R_ROWS_40K, R_ROWS_262K, R_ROWS_4M = 38, 246, 3928

CASES = [
    Case("labels_3d", ("voxel_scan",), 2, 132 * 128 * 129, 0, 0, 0),
    Case("labels_2d", ("voxel_scan",), 2, 2 ** 21 + 2048 + 256, 0, 0, 0),
    Case("labels_many_events", ("event_blocks",), 700, 2048 + 300, 0, 0, 0),
    Case("random_replicated", ("cluster_scan", "match_slots", "entry_blocks", "event_blocks"), 897, 2100176, 34086, 0, 0),
    Case("lattice", ("cluster_scan",), 1, 2107000, 632100, 0, 0),
    Case("rows_40k", ("clfeat_init",), 114, 41154, 40584, 0, 0),
    Case("rows_262k", ("clfeat_rows",), 738, 266418, 262728, 0, 0),
    Case("rows_4m", ("match_rows", "graph_rows", "event_blocks"), 11784, 4254024, 4254024, 0, 58920),
    Case("checkerboard_3x8", ("graph_scan",), 3, 1536, 1536, 0, 0),
    Case("checkerboard_12", ("graph_scan",), 1, 1728, 1728, 0, 0),
    Case("checkerboard_wide_table", ("graph_slots",), 3, 1536, 1536, 0, 2 ** 21 + 5),
    Case("crop_boxes", ("crop_scan",), 3, 0, 0, 1071, 0),
    Case("small_events_5000", ("event_blocks",), 5000, 12800, 0, 0, 0),
    Case("small_events_700", ("event_blocks", "events_over_entries"), 700, 300, 0, 0, 0),
]
BY_NAME = {c.name: c for c in CASES}
