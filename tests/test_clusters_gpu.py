"""Voxel clusters on the device (csrc/cluster.hip) against the numpy statement (uresnet_amd.clusters.cluster_numpy).  Every comparison
is exact.  Op level: the list and every output sit between 0xFF guard bands (tests/_guard.py) at exact sizes; each case runs three
times -- scratch filled 0xFF, filled 0x00, and as the second call left it -- and all three must give the statement's bits with
status 0.  Net level: 'cluster' in want of the voxel-score calls, cluster_voxels, and the driver's fourth record."""
import ctypes
import io
from contextlib import redirect_stdout

import numpy as np
import pytest

import _far_corner as far
from _guard import Guarded
from uresnet_amd import _lib, tiling, uresnet
from uresnet_amd import synthetic_io as sio
from uresnet_amd.clusters import ClusterSpec, cluster_numpy
from uresnet_amd.ssnet import VoxelBatch

pytestmark = pytest.mark.gpu


# ---- op level ------------------------------------------------------------------------------------------------------------------
def _want(off, index, cls, shape, spec):
    """The statement per event: ids [M], counts [n], the table back to back, its offsets [n + 1]."""
    ids, first, size, tcls, counts = [], [], [], [], []
    for e in range(len(off) - 1):
        a, b = int(off[e]), int(off[e + 1])
        c, f, s, t = cluster_numpy(index[a:b], cls[a:b], shape, spec)
        ids.append(c), first.append(f), size.append(s), tcls.append(t), counts.append(f.size)
    cat = lambda parts, dt: np.concatenate(parts).astype(dt) if parts else np.zeros(0, dt)
    return {"cluster": cat(ids, np.int32), "count": np.array(counts, np.int32), "first": cat(first, np.int32),
            "size": cat(size, np.int32), "cls": cat(tcls, np.uint8),
            "table_offsets": np.concatenate([[0], np.cumsum(counts)]).astype(np.int64)}


FILLS = (0xFF, 0x00, None)


def _run(lib, off, index, cls, shape, spec, cap=None, table=True, fills=FILLS):
    """Three calls of ursn_cluster_voxels on guarded operands; returns the three results as host arrays (`fills`: the scratch fill
    before each call, None = as the call before left it; tests/test_long_lists_gpu.py runs two)."""
    import torch
    off = np.asarray(off, np.int64)
    index, cls = np.asarray(index, np.int32), np.asarray(cls, np.uint8)
    n, M = off.size - 1, int(off[-1])
    assert index.size == M and cls.size == M
    cap = M if cap is None else cap
    g_off = Guarded(n + 1, torch.int64, off)
    g_idx = Guarded(max(M, 1), torch.int32)
    g_cls = Guarded(max(M, 1), torch.uint8)
    if M:
        g_idx.set(index), g_cls.set(cls)
    need = int(lib.ursn_cluster_scratch_bytes(n, M))
    assert need >= 8 and need % 8 == 0
    scratch = Guarded(need, torch.uint8)
    d = _lib.ursn_cluster_desc()
    d.ndim, d.n, d.m_total = len(shape), n, M
    for i, s in enumerate(shape):
        d.spatial[i] = s
    d.offsets, d.index, d.cls = g_off.ptr, g_idx.ptr, g_cls.ptr
    conn, _ = spec.axes(len(shape))
    d.connectivity, d.class_mask, d.same_class, d.min_size = conn, spec.class_mask(), int(spec.same_class), spec.min_size
    results = []
    for fill in fills:
        if fill is not None:
            scratch.fill(fill)
        outs = {"cluster": Guarded(max(M, 1), torch.int32), "count": Guarded(n, torch.int32), "status": Guarded(1, torch.int32),
                "table_offsets": Guarded(n + 1, torch.int64)}
        if table:
            outs.update(first=Guarded(max(cap, 1), torch.int32), size=Guarded(max(cap, 1), torch.int32),
                        cls=Guarded(max(cap, 1), torch.uint8))
        o = _lib.ursn_cluster_out()
        for name, g in outs.items():
            setattr(o, name, g.ptr)
        if not table:
            o.table_offsets = None
        o.cap = cap
        _lib.check(lib.ursn_cluster_voxels(ctypes.byref(d), ctypes.byref(o), ctypes.c_void_p(scratch.ptr), need, None))
        torch.cuda.synchronize()
        for name, g in list(outs.items()) + [("offsets", g_off), ("index", g_idx), ("cls_in", g_cls), ("scratch", scratch)]:
            g.check(name)
        results.append({name: g.numpy() for name, g in outs.items()})
    return results


def _check(lib, off, index, cls, shape, spec, cap=None):
    """Runs the case and compares all three calls with the statement; returns the statement."""
    off = np.asarray(off, np.int64)
    index, cls = np.asarray(index, np.int64), np.asarray(cls, np.uint8)
    n, M = off.size - 1, int(off[-1])
    want = _want(off, index, cls, shape, spec)
    total = int(want["table_offsets"][-1])
    rows = total if cap is None else min(cap, total)
    for k, got in enumerate(_run(lib, off, index, cls, shape, spec, cap)):
        what = "call %d" % k
        assert int(got["status"][0]) == 0, what
        assert np.array_equal(got["cluster"][:M], want["cluster"]), what
        assert np.array_equal(got["count"], want["count"]) and np.array_equal(got["table_offsets"], want["table_offsets"]), what
        for name in ("first", "size", "cls"):
            assert np.array_equal(got[name][:rows], want[name][:rows]), (what, name)
            rest = got[name][rows:]
            assert (rest.view(np.uint8) == 0xFF).all(), (what, name, "rows at or beyond the count or cap were written")
    return want


def _list(shape, coords):
    idx = np.sort(np.ravel_multi_index(np.array(coords, np.int64).T, shape)) if len(coords) else np.zeros(0, np.int64)
    assert np.unique(idx).size == idx.size
    return idx


@pytest.mark.parametrize("conn", [6, 18, 26])
def test_adjacent_indices_across_a_row_or_plane_end_do_not_join(lib, conn):
    shape = (4, 5, 6)
    # x = 5 of one row | x = 0 of the next; last row of a plane | first row of the next, one index and one row apart
    index = _list(shape, [(0, 0, 5), (0, 1, 0), (1, 4, 2), (1, 4, 5), (2, 0, 0), (2, 0, 2)])
    assert list(index) == [5, 6, 56, 59, 60, 62]
    want = _check(lib, [0, 6], index, np.ones(6, np.uint8), shape, ClusterSpec(conn))
    assert list(want["cluster"]) == [0, 1, 2, 3, 4, 5]


def test_pairs_that_tell_the_connectivities_apart(lib):
    shape = (6, 6, 6)
    pairs = [(0, 0, 0), (0, 0, 1), (0, 3, 0), (0, 4, 1), (3, 0, 0), (4, 1, 1),      # face, edge, corner, later entry at +x
             (3, 3, 1), (3, 4, 0), (3, 3, 4), (4, 4, 3)]                              # edge and corner, later entry at -x
    index = _list(shape, pairs)
    for conn, clusters in ((6, 9), (18, 7), (26, 5)):
        want = _check(lib, [0, 10], index, np.ones(10, np.uint8), shape, ClusterSpec(conn))
        assert int(want["count"][0]) == clusters, conn
    flat = _list((6, 6), [(0, 0), (0, 1), (3, 0), (4, 1), (3, 4), (4, 3)])
    for conn, clusters in ((4, 5), (8, 3)):
        want = _check(lib, [0, 6], flat, np.ones(6, np.uint8), (6, 6), ClusterSpec(conn))
        assert int(want["count"][0]) == clusters, conn


def test_comb_whose_teeth_meet_only_in_the_last_plane(lib):
    shape = (16, 16, 16)
    teeth = [(a, b, c) for a in range(15) for b in range(0, 16, 2) for c in range(0, 16, 2)]
    spine = [(15, b, c) for b in range(16) for c in range(16)]
    index = _list(shape, teeth + spine)
    want = _check(lib, [0, index.size], index, np.full(index.size, 2, np.uint8), shape, ClusterSpec(6))
    assert int(want["count"][0]) == 1 and int(want["size"][0]) == 64 * 15 + 256
    # without the spine every tooth is a cluster of its own
    index = _list(shape, teeth)
    want = _check(lib, [0, index.size], index, np.full(index.size, 2, np.uint8), shape, ClusterSpec(6))
    assert int(want["count"][0]) == 64 and (want["size"] == 15).all()


def _thin_snake(S=16, planes=8):
    """One voxel wide at connectivity 6 in S^3: every other row of the first `planes` even planes, rows joined at alternating ends,
    planes joined by one voxel at the end of their last row and at the start of their first row in turn, so the whole is ONE path."""
    pts = []
    for k in range(planes):
        a = 2 * k
        for r, b in enumerate(range(0, S, 2)):
            pts += [(a, b, c) for c in range(S)]
            if b < S - 2:
                pts.append((a, b + 1, S - 1 if r % 2 == 0 else 0))
        if k < planes - 1:
            pts.append((a + 1, S - 2, S - 1) if k % 2 == 0 else (a + 1, 0, 0))
    return pts


def test_snakes(lib):
    """A one-voxel-wide snake fills at most about a quarter of a volume at connectivity 6: 1087 entries in 16^3.  The ~3000-entry
    snake therefore runs through 24^3 (2999 entries): the chain is long and its halves meet only at the very last links."""
    shape = (24, 24, 24)
    index = _list(shape, _thin_snake(24, 10))
    assert index.size == 10 * (12 * 24 + 11) + 9 == 2999
    want = _check(lib, [0, index.size], index, np.ones(index.size, np.uint8), shape, ClusterSpec(6))
    assert int(want["count"][0]) == 1 and int(want["size"][0]) == 2999
    cut = np.delete(index, np.flatnonzero(index == np.ravel_multi_index((10, 12, 7), shape)))      # cut near the middle: two halves
    want = _check(lib, [0, cut.size], cut, np.ones(cut.size, np.uint8), shape, ClusterSpec(6))
    assert int(want["count"][0]) == 2 and min(want["size"]) > 1000
    shape = (16, 16, 16)
    index = _list(shape, _thin_snake())
    assert index.size == 8 * (8 * 16 + 7) + 7
    want = _check(lib, [0, index.size], index, np.ones(index.size, np.uint8), shape, ClusterSpec(6))
    assert int(want["count"][0]) == 1 and int(want["size"][0]) == index.size
    # cut in the middle of the first plane's third row it is two clusters
    cut = np.delete(index, np.flatnonzero(index == np.ravel_multi_index((0, 4, 7), shape)))
    want = _check(lib, [0, cut.size], cut, np.ones(cut.size, np.uint8), shape, ClusterSpec(6))
    assert int(want["count"][0]) == 2


def test_full_block_and_checkerboard(lib):
    shape = (12, 12, 12)
    full = np.arange(1728)
    want = _check(lib, [0, 1728], full, np.ones(1728, np.uint8), shape, ClusterSpec(26))
    assert int(want["count"][0]) == 1 and int(want["size"][0]) == 1728
    x = np.stack(np.unravel_index(full, shape), axis=1)
    board = full[x.sum(axis=1) % 2 == 0]
    want = _check(lib, [0, board.size], board, np.ones(board.size, np.uint8), shape, ClusterSpec(26))
    assert int(want["count"][0]) == 1 and int(want["size"][0]) == 864
    want = _check(lib, [0, board.size], board, np.ones(board.size, np.uint8), shape, ClusterSpec(6))
    assert int(want["count"][0]) == 864 and (want["size"] == 1).all() and np.array_equal(want["cluster"], np.arange(864))


def _random_list(seed, shape, occupancy, classes=3):
    rng = np.random.default_rng(seed)
    index = np.flatnonzero(rng.uniform(size=int(np.prod(shape))) < occupancy)
    return index, rng.integers(0, classes, index.size).astype(np.uint8)


@pytest.mark.parametrize("occupancy", [0.05, 0.3, 0.6])
def test_random_lists_with_three_classes(lib, occupancy):
    shape = (24, 20, 28)
    index, cls = _random_list(int(occupancy * 100), shape, occupancy)
    assert 600 <= index.size <= 8200
    for same_class in (True, False):
        for classes in ((0, 1, 2), None, ()):
            want = _check(lib, [0, index.size], index, cls, shape, ClusterSpec(26, classes, same_class))
            if classes == ():
                assert (want["cluster"] == -1).all() and int(want["count"][0]) == 0
            if classes is None:
                assert (want["cluster"][cls == 0] == -1).all() and (want["cluster"][cls != 0] >= 0).all()
    _check(lib, [0, index.size], index, cls, shape, ClusterSpec(6))
    _check(lib, [0, index.size], index, cls, shape, ClusterSpec(18, min_size=4))


def test_min_size_drops_and_renumbers(lib):
    shape = (8, 8, 8)
    lengths = [4, 2, 3, 1, 5, 2, 3]
    pts = [(2 * (i // 4), 2 * (i % 4), c) for i, n in enumerate(lengths) for c in range(1, 1 + n)]
    index = _list(shape, pts)
    want = _check(lib, [0, index.size], index, np.ones(index.size, np.uint8), shape, ClusterSpec(26, min_size=3))
    assert list(want["size"]) == [4, 3, 5, 3] and list(want["first"]) == [0, 6, 10, 17]
    assert list(want["cluster"]) == [0] * 4 + [-1] * 2 + [1] * 3 + [-1] + [2] * 5 + [-1] * 2 + [3] * 3
    want = _check(lib, [0, index.size], index, np.ones(index.size, np.uint8), shape, ClusterSpec(26, min_size=6))
    assert int(want["count"][0]) == 0 and (want["cluster"] == -1).all()


def test_events_do_not_join_and_may_be_empty(lib):
    shape = (6, 6, 6)
    p, pc = _random_list(3, shape, 0.3, classes=2)
    pc += 1
    spec = ClusterSpec(26)
    # empty first, in the middle and last; the same pattern in the two events between them
    off = np.cumsum([0, 0, p.size, 0, p.size, 0])
    want = _check(lib, off, np.concatenate([p, p]), np.concatenate([pc, pc]), shape, spec)
    assert list(want["count"][[0, 2, 4]]) == [0, 0, 0] and want["count"][1] == want["count"][3] > 0
    assert np.array_equal(want["cluster"][:p.size], want["cluster"][p.size:])
    # single-entry events, identical neighbours, and a long event: boundaries inside a workgroup's 256 entries and several workgroups
    big_shape = (24, 20, 28)
    q, qc = _random_list(4, big_shape, 0.05, classes=3)
    one = np.array([7])
    lists = [one, q[:100], q[:100], one, q]
    classes = [np.array([1], np.uint8), qc[:100] | 1, qc[:100] | 1, np.array([2], np.uint8), qc]
    off = np.concatenate([[0], np.cumsum([a.size for a in lists])])
    want = _check(lib, off, np.concatenate(lists), np.concatenate(classes), big_shape, spec)
    assert want["count"][0] == want["count"][3] == 1 and want["count"][1] == want["count"][2]
    # all events empty: nothing that reads the list is launched
    want = _check(lib, [0, 0, 0], np.zeros(0, np.int64), np.zeros(0, np.uint8), shape, spec)
    assert list(want["count"]) == [0, 0]


def test_indices_outside_the_volume_take_no_part(lib):
    shape = (4, 5, 6)
    index = np.array([-1, 0, 1, 118, 119, 120, 121])
    want = _check(lib, [0, 7], index, np.ones(7, np.uint8), shape, ClusterSpec(26))
    assert list(want["cluster"]) == [-1, 0, 0, 1, 1, -1, -1]


def test_a_short_cap_bounds_the_table_and_nothing_else(lib):
    shape = (24, 20, 28)
    index, cls = _random_list(9, shape, 0.05)
    off = [0, 300, index.size]
    full = _want(np.array(off), index, cls, shape, ClusterSpec(26, (0, 1, 2)))
    total = int(full["table_offsets"][-1])
    assert total > 40
    for cap in (total // 2, 1, 0):
        _check(lib, off, index, cls, shape, ClusterSpec(26, (0, 1, 2)), cap=cap)
    # no table at all: ids and counts only
    got = _run(lib, off, index, cls, shape, ClusterSpec(26, (0, 1, 2)), table=False)[0]
    assert np.array_equal(got["cluster"], full["cluster"]) and np.array_equal(got["count"], full["count"])


@pytest.mark.parametrize("conn", [4, 8])
def test_two_dimensional_lists(lib, conn):
    shape = (20, 24)
    a, ac = _random_list(11, shape, 0.3)
    b, bc = _random_list(12, shape, 0.6)
    off = [0, a.size, a.size + b.size]
    for same_class in (True, False):
        _check(lib, off, np.concatenate([a, b]), np.concatenate([ac, bc]), shape, ClusterSpec(conn, None, same_class, 2))
    # x = 23 of one row and x = 0 of the next
    want = _check(lib, [0, 2], [23, 24], [1, 1], shape, ClusterSpec(conn))
    assert list(want["cluster"]) == [0, 1]


# ---- the largest legal extents (tests/_far_corner.py) ---------------------------------------------------------------
@pytest.mark.parametrize("shape", far.SHAPES_VOLUME, ids=far.shape_id)
def test_far_corner(lib, shape):
    """The random lists against the far faces, at the origin and across index 2^30 of a shape that has one quantity at its cap
    (what the batch reaches is asserted in tests/test_far_corner_host.py)."""
    b = far.far_batch("random", shape).big
    assert int(b.index.max()) >= far.volume(shape) - far.volume(shape[1:]) and far.FAR in far.far_batch("random", shape).placement
    wide, narrow = (26, 6) if len(shape) == 3 else (8, 4)
    for conn, same_class, min_size in ((wide, True, 2), (wide, False, 1), (narrow, True, 1), (narrow, False, 3)):
        want = _check(lib, b.off, b.index, b.cls, shape, ClusterSpec(conn, (0, 1, 2), same_class, min_size))
        assert want["table_offsets"][-1] > 0
        if (conn, same_class, min_size) == (wide, True, 2):                 # the ids the other calls' far-corner tests are given
            assert np.array_equal(want["cluster"], b.cluster) and np.array_equal(want["table_offsets"], b.toff)


@pytest.mark.parametrize("axis", sorted(far.LONG_TRACK))
def test_a_track_across_the_longest_axis(lib, axis):
    """32,768 entries, one 26-connected staircase from the origin corner to the far corner along the capped axis; along axis 2 of
    (255, 256, 32768) the same list is also clustered as runs: at connectivity 6 every step aside ends a cluster."""
    s = far.long_track(far.LONG_TRACK[axis])
    want = _check(lib, s.off, s.index, s.cls, s.shape, ClusterSpec(26))
    assert want["count"].tolist() == [1] and want["size"].tolist() == [32768]
    if axis == 2:
        want = _check(lib, s.off, s.index, s.cls, s.shape, ClusterSpec(6))
        assert int(want["count"][0]) > 1 and int(want["size"].max()) >= 64
        x = np.zeros(32768, np.int64)                      # one x-run of 32,768: the last row of the volume
        x[:] = far.volume(s.shape) - 32768 + np.arange(32768)
        want = _check(lib, [0, 32768], x, s.cls, s.shape, ClusterSpec(6))
        assert want["count"].tolist() == [1] and want["size"].tolist() == [32768]


# ---- net level -----------------------------------------------------------------------------------------------------------------
DIMS = (32, 32, 32, 1)
_cache = {}


def _net(prec):
    net = uresnet(dims=list(DIMS), num_class=3, base_num_outputs=8, num_strides=2)
    net.construct(trainable=False, use_weight=False, seed=7, precision=prec)
    return net


def _events(n=2):
    if "vb" not in _cache:
        _cache["vb"] = VoxelBatch.concat([sio.dense_to_voxels(*sio.lartpc_sparse(list(DIMS), 3, e)) for e in range(n)]).validate()
    return _cache["vb"]


def _same_clusters(r, classes, shape, spec):
    """r['cluster'] / r['clusters'] equal the statement on the given per-event classes."""
    for i in range(len(r["index"])):
        c, first, size, tcls = cluster_numpy(r["index"][i], classes[i], shape, spec)
        assert r["cluster"][i].dtype == np.int32 and np.array_equal(r["cluster"][i], c), i
        t = r["clusters"][i]
        assert np.array_equal(t["first"], first) and np.array_equal(t["size"], size) and np.array_equal(t["cls"], tcls), i


@pytest.mark.parametrize("prec", ["fp32", "bf16"])
def test_inference_voxel_scores_with_clusters(prec):
    net, vb = _net(prec), _events()
    plain = net.inference_voxel_scores(None, vb, with_labels=False, want=("pred", "ana"))
    assert sorted(plain) == ["ana", "index", "pred"]
    spec = ClusterSpec(classes=(0, 1, 2), min_size=2)
    net.set_clustering(spec)
    r = net.inference_voxel_scores(None, vb, with_labels=False, want=("pred", "cluster"))
    assert sorted(r) == ["cluster", "clusters", "index", "pred"]
    assert all(np.array_equal(a, b) for a, b in zip(r["pred"], plain["pred"]))
    _same_clusters(r, r["pred"], DIMS[:-1], spec)
    assert sum(t["first"].size for t in r["clusters"]) > 0
    alone = net.inference_voxel_scores(None, vb, with_labels=False, want=("cluster",))
    assert sorted(alone) == ["cluster", "clusters", "index"]
    assert all(np.array_equal(a, b) for a, b in zip(alone["cluster"], r["cluster"]))
    assert sorted(net.inference_voxel_scores(None, vb, with_labels=False)) == ["ana", "index", "pred", "scores"]   # defaults unchanged
    on_ana = ClusterSpec(connectivity=18, on="ana")
    net.set_clustering(on_ana)
    r = net.inference_voxel_scores(None, vb, with_labels=True, want=("scores", "cluster"))
    assert sorted(r) == ["acc_all", "acc_nonzero", "cluster", "clusters", "index", "scores"]
    _same_clusters(r, plain["ana"], DIMS[:-1], on_ana)
    assert sum(t["first"].size for t in r["clusters"]) > 0


@pytest.mark.parametrize("prec", ["fp32", "bf16"])
def test_tiled_clusters_are_in_the_large_shape_and_cross_tiles(prec):
    big, halo = (48, 40, 56), 4
    vb = VoxelBatch.concat([sio.dense_to_voxels(*sio.lartpc_sparse(list(big) + [1], 3, e)) for e in range(2)]).validate()
    net = _net(prec)
    for spec in (ClusterSpec(classes=(0, 1, 2), same_class=False), ClusterSpec(classes=(0, 1, 2), min_size=3)):
        net.set_clustering(spec)
        r = net.inference_tiled_voxel_scores(None, vb, big, halo=halo, want=("pred", "cluster"))
        _same_clusters(r, r["pred"], big, spec)
    # from the numpy side: with every listed voxel joined to its neighbours, some cluster has entries in two boxes' cores
    spec = ClusterSpec(classes=(0, 1, 2), same_class=False)
    boxes = tiling.grid(big, DIMS[:-1], halo)
    spans = 0
    for i in range(2):
        c, first, _, _ = cluster_numpy(r["index"][i], r["pred"][i], big, spec)
        x = np.stack(np.unravel_index(r["index"][i], big), axis=1)
        owner = np.full(c.size, -1)
        for b in range(len(boxes)):
            lo, hi = boxes.origin[b] + boxes.core_lo[b], boxes.origin[b] + boxes.core_hi[b]
            owner[np.all((x >= lo) & (x < hi), axis=1)] = b
        assert (owner >= 0).all()
        spans += sum(1 for k in range(first.size) if np.unique(owner[c == k]).size > 1)
    assert spans >= 1


@pytest.mark.parametrize("prec", ["fp32", "bf16"])
def test_cluster_voxels_on_tta_results_and_on_true_labels(prec):
    net, vb = _net(prec), _events()
    spec = ClusterSpec(18, min_size=2)
    tta = net.inference_voxel_scores_tta(None, vb, [0, 1])
    r = net.cluster_voxels(None, vb, tta["pred"], spec)
    r["index"] = tta["index"]
    _same_clusters(r, tta["pred"], DIMS[:-1], spec)
    off = vb.offsets
    truth = [vb.label[off[i]:off[i + 1]].astype(np.uint8) for i in range(vb.n)]
    r = net.cluster_voxels(None, tta["index"], truth, ClusterSpec())
    r["index"] = tta["index"]
    _same_clusters(r, truth, DIMS[:-1], ClusterSpec())
    assert sum(t["first"].size for t in r["clusters"]) > 0
    # another shape than the network's, a flat class array
    flat = net.cluster_voxels(None, [np.array([23, 24, 25])], np.array([1, 1, 1]), ClusterSpec(4), shape=(20, 24))
    assert list(flat["cluster"][0]) == [0, 1, 1] and list(flat["clusters"][0]["size"]) == [1, 2]


# ---- driver --------------------------------------------------------------------------------------------------------------------
def _ana_cfg(tmp_path, tag, extra):
    inp = tmp_path / "input.cfg"
    inp.write_text("Dims [32, 32, 32, 1]\nNumClass 3\nGenerator 'lartpc_sparse'\nNumEntries 64\n"
                   "Keys {'data': 'data', 'label': 'label', 'weight': 'weight'}\n")
    out = tmp_path / ("ssnet_%s.npy" % tag)
    ana = tmp_path / ("ana_%s.cfg" % tag)
    ana.write_text("NUM_CLASS 3\nBASE_NUM_FILTERS 4\nMAIN_INPUT_CONFIG '%s'\nANA_OUTPUT_CONFIG '%s'\nLOGDIR ''\nSAVE_FILE ''\n"
                   "ITERATIONS 1\nMINIBATCH_SIZE 2\nTRAIN False\nUSE_WEIGHTS False\nSUMMARY_STEPS 0\nCHECKPOINT_STEPS 0\n"
                   "SPARSE_IO True\nSPARSE_SCORES True\n%s" % (inp, out, extra))
    return ana, out


def _drive(tmp_path, tag, extra, interactive=False):
    from uresnet_amd.ssnet_trainval import ssnet_trainval
    cfg, out = _ana_cfg(tmp_path, tag, extra)
    t = ssnet_trainval()
    with redirect_stdout(io.StringIO()):
        t.override_config(str(cfg))
        t.initialize()
        res = t.ana_step() if interactive else t.batch_process()
        t.reset()
    with open(str(out), "rb") as f:
        return f.read(), res


def _records(blob):
    f, recs = io.BytesIO(blob), []
    while f.tell() < len(blob):
        a = f.tell()
        arr = np.load(f)
        recs.append((arr, blob[a:f.tell()]))
    return recs


def test_driver_appends_the_cluster_record(tmp_path):
    without, _ = _drive(tmp_path, "plain", "")
    off, _ = _drive(tmp_path, "off", "ANA_CLUSTER ''\nCLUSTER_MIN_SIZE 3\n")
    assert off == without and len(_records(without)) == 6                     # default '': byte for byte the file without the key
    on, _ = _drive(tmp_path, "on", "ANA_CLUSTER 'ana'\nCLUSTER_CONNECTIVITY 18\nCLUSTER_MIN_SIZE 2\n")
    old, new = _records(without), _records(on)
    assert len(new) == 8
    spec = ClusterSpec(18, min_size=2, on="ana")
    for e in range(2):
        for k in range(3):
            assert new[4 * e + k][1] == old[3 * e + k][1], (e, k)               # the first three records, header included
        index, ana, cluster = new[4 * e][0], new[4 * e + 1][0], new[4 * e + 3][0]
        assert cluster.dtype == np.int32 and np.array_equal(cluster, cluster_numpy(index, ana, (32, 32, 32), spec)[0])
        assert (cluster >= 0).any()
    _, res = _drive(tmp_path, "inter", "ANA_CLUSTER 'pred'\n", interactive=True)
    _, ref = _drive(tmp_path, "inter0", "", interactive=True)
    assert sorted(res) == sorted(ref)
    for ev, ev0 in zip(res["voxels"], ref["voxels"]):
        assert sorted(ev) == sorted(list(ev0) + ["cluster", "clusters"])
        c, first, size, tcls = cluster_numpy(ev["index"], ev["pred"], (32, 32, 32), ClusterSpec())
        assert np.array_equal(ev["cluster"], c) and np.array_equal(ev["clusters"]["first"], first)
        assert np.array_equal(ev["clusters"]["size"], size) and np.array_equal(ev["clusters"]["cls"], tcls)
