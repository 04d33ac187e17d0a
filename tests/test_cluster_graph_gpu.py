"""Cluster contact graph on the device (csrc/cluster_graph.hip) against the pure-Python statement
(uresnet_amd.clusters.cluster_graph_numpy).  Every comparison is np.array_equal on every table.  Op level: the lists and every
output sit between 0xFF guard bands (tests/_guard.py) and the scratch has exactly the stated size; each case runs four times --
scratch filled 0xFF, filled 0x00, as the second call left it (the same arguments again), and with one table insertion per near pair
instead of one per distinct edge of a workgroup (URSN_CLGRAPH_WAVE=0) -- and all four must give the statement's bits with status 0.
Net level: set_cluster_graph with the voxel-score calls, cluster_graph, and the driver's ANA_GRAPH file."""
import ctypes
import io
import os
from contextlib import redirect_stdout

import numpy as np
import pytest

import _far_corner as far
from _guard import Guarded
from uresnet_amd import _lib, uresnet
from uresnet_amd import synthetic_io as sio
from uresnet_amd.clusters import (GRAPH_EDGE, GRAPH_EVENT, GRAPH_GROUP, GRAPH_ROW, ClusterGraphSpec, ClusterSpec, cluster_graph_numpy,
                                  cluster_numpy)
from uresnet_amd.ssnet import VoxelBatch, graph_csv_header

pytestmark = pytest.mark.gpu

E, I, G, EV = _lib.CLGRAPH_E, _lib.CLGRAPH_I, _lib.CLGRAPH_G, _lib.CLGRAPH_EV
OVERFLOW = _lib.CLGRAPH_EDGE_OVERFLOW
ROUTES = ((0xFF, True), (0x00, True), (None, True), (0xFF, False))


def _untouched(a):
    return bool((np.ascontiguousarray(a).view(np.uint8) == 0xFF).all())


def _run(lib, off, index, ids, toff, spatial, gap, value, cls, cap_rows, cap_groups, edge_out_cap, edge_cap, rows, groups, edges,
         with_edges=True, short_scratch=False, routes=ROUTES):
    """Four calls of ursn_cluster_graph on guarded operands.  The tables hold rows / groups / edges records whatever the caps are, so
    what lies at or beyond a cap can be seen to be untouched.  Returns per call a dict of host arrays."""
    import torch
    n, M, K = off.size - 1, int(off[-1]), int(toff[-1])
    g_off, g_toff = Guarded(n + 1, torch.int64, off), Guarded(n + 1, torch.int64, toff)
    g_index, g_ids = Guarded(max(M, 1), torch.int32), Guarded(max(M, 1), torch.int32)
    g_val = None if value is None else Guarded(max(M, 1), torch.float32)
    g_cls = None if cls is None else Guarded(max(K, 1), torch.uint8)
    if M:
        g_index.set(index.astype(np.int32)), g_ids.set(ids.astype(np.int32))
        if g_val is not None:
            g_val.set(value)
    if K and g_cls is not None:
        g_cls.set(cls.astype(np.uint8))
    need = int(lib.ursn_cluster_graph_scratch_bytes(n, M, cap_rows, cap_groups, edge_cap))
    assert need >= 8 and need % 8 == 0
    scratch = Guarded(need, torch.uint8)
    d = _lib.ursn_cluster_graph_desc()
    d.ndim, d.n, d.gap, d.m_total, d.edge_cap = len(spatial), n, gap, M, edge_cap
    for i, s in enumerate(spatial):
        d.spatial[i] = s
    d.offsets, d.index, d.cluster, d.table_offsets = g_off.ptr, g_index.ptr, g_ids.ptr, g_toff.ptr
    d.value, d.cls = None if g_val is None else g_val.ptr, None if g_cls is None else g_cls.ptr
    inputs = [("offsets", g_off), ("table_offsets", g_toff), ("index", g_index), ("cluster", g_ids), ("scratch", scratch)] + \
        ([] if g_val is None else [("value", g_val)]) + ([] if g_cls is None else [("cls", g_cls)])
    results = []
    for fill, wave in routes:
        if fill is not None:
            scratch.fill(fill)
        out = {"rows": Guarded((max(rows, 1), I), torch.int64), "groups": Guarded((max(groups, 1), G), torch.int64),
               "group_offsets": Guarded(n + 1, torch.int64), "event": Guarded((n, EV), torch.int64),
               "group": Guarded(max(M, 1), torch.int32), "status": Guarded(1, torch.int32)}
        if with_edges:
            out.update({"edge_offsets": Guarded(max(rows, cap_rows) + 1, torch.int64), "edges": Guarded((max(edges, 1), E), torch.int64)})
        o = _lib.ursn_cluster_graph_out()
        for name, g in out.items():
            setattr(o, name, g.ptr)
        o.cap_rows, o.cap_groups, o.edge_out_cap = cap_rows, cap_groups, edge_out_cap if with_edges else 0
        if not wave:
            os.environ["URSN_CLGRAPH_WAVE"] = "0"
        try:
            rc = lib.ursn_cluster_graph(ctypes.byref(d), ctypes.byref(o), ctypes.c_void_p(scratch.ptr), need - 8 if short_scratch else need,
                                        None)
        finally:
            os.environ.pop("URSN_CLGRAPH_WAVE", None)
        torch.cuda.synchronize()
        if short_scratch:                                  # refused before any launch: nothing was written anywhere
            assert rc != 0 and b"cluster_graph: scratch of %d bytes is too small" % (need - 8) in lib.ursn_last_error()
            assert all(_untouched(g.numpy()) for g in out.values())
        else:
            _lib.check(rc)
        for name, g in inputs + list(out.items()):
            g.check(name)
        results.append({name: g.numpy() for name, g in out.items()})
    return results


def _check(lib, off, index, ids, toff, spatial, gap, value=None, cls=None, cap_rows=None, cap_groups=None, edge_out_cap=None,
           edge_cap=None, with_edges=True):
    """Runs the case and compares all four calls with the statement; returns the statement."""
    off, toff, index, ids = (np.asarray(x, np.int64) for x in (off, toff, index, ids))
    value = None if value is None else np.asarray(value, np.float32)
    cls = None if cls is None else np.asarray(cls, np.uint8)
    want = cluster_graph_numpy(off, index, ids, toff, spatial, ClusterGraphSpec(gap), value, cls)
    K, NG, NE = int(toff[-1]), int(want["group_offsets"][-1]), int(want["edge_offsets"][-1])
    cap_rows, cap_groups = (K if cap_rows is None else cap_rows), (NG if cap_groups is None else cap_groups)
    edge_out_cap, edge_cap = (NE if edge_out_cap is None else edge_out_cap), (NE if edge_cap is None else edge_cap)
    kr, kg, ke = min(cap_rows, K), min(cap_groups, NG), min(edge_out_cap, NE)
    for k, got in enumerate(_run(lib, off, index, ids, toff, spatial, gap, value, cls, cap_rows, cap_groups, edge_out_cap, edge_cap,
                                 K, NG, NE, with_edges)):
        what = "call %d" % k
        assert int(got["status"][0]) == 0, (what, int(got["status"][0]))
        assert np.array_equal(got["rows"][:kr], want["rows"][:kr]), what
        assert _untouched(got["rows"][kr:]), (what, "rows at or beyond the count or cap were written")
        assert np.array_equal(got["groups"][:kg], want["groups"][:kg]), what
        assert _untouched(got["groups"][kg:]), (what, "groups at or beyond the count or cap were written")
        assert np.array_equal(got["group_offsets"], want["group_offsets"]), what                    # the TRUE counts
        assert np.array_equal(got["event"], want["events"]), what
        assert np.array_equal(got["group"][:off[-1]], want["group"]) and got["group"].dtype == np.int32, what
        if with_edges:
            assert np.array_equal(got["edge_offsets"][:kr + 1], want["edge_offsets"][:kr + 1]), what   # the TRUE counts
            assert _untouched(got["edge_offsets"][kr + 1:]), what
            assert np.array_equal(got["edges"][:ke], want["edges"][:ke]), what
            assert _untouched(got["edges"][ke:]), (what, "edges at or beyond the count or cap were written")
    return want


def _ravel(coords, spatial):
    return np.ravel_multi_index(np.asarray(coords, np.int64).T, spatial)


def _lists(events, spatial):
    """Per event a dict {coordinate tuple: id} -> sorted lists, ids and the table offsets (every id 0..K_e-1 must occur)."""
    off, index, ids, counts = [0], [], [], []
    for ev in events:
        items = sorted((int(_ravel([c], spatial)[0]), i) for c, i in ev.items())
        index += [x for x, _ in items]
        ids += [i for _, i in items]
        off.append(len(index))
        used = sorted(set(i for _, i in items if i >= 0))
        assert used == list(range(len(used)))
        counts.append(len(used))
    return np.array(off, np.int64), np.array(index, np.int64), np.array(ids, np.int64), np.concatenate([[0], np.cumsum(counts)])


def _clustered(off, index, cls, shape, spec):
    ids, counts, tcls = [], [], []
    for e in range(len(off) - 1):
        c, first, _, kc = cluster_numpy(index[off[e]:off[e + 1]], cls[off[e]:off[e + 1]], shape, spec)
        ids.append(c), counts.append(first.size), tcls.append(kc)
    return np.concatenate(ids).astype(np.int64), np.concatenate([[0], np.cumsum(counts)]).astype(np.int64), np.concatenate(tcls)


# ---- boundaries --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("gap", [1, 2, 3])
@pytest.mark.parametrize("spatial", [(7, 9, 11), (10, 13)], ids=["3d", "2d"])
def test_exactly_gap_and_one_more(lib, spatial, gap):
    """Two one-voxel clusters exactly `gap` and `gap + 1` apart along each axis and along the full diagonal: an edge, and none.
    Event 1 is empty; event 2 holds the first voxel's coordinates again and a far corner: no edge crosses an event."""
    nd = len(spatial)
    p = (1,) * nd
    steps = [tuple(1 if k == a else 0 for k in range(nd)) for a in range(nd)] + [(1,) * nd]
    for step in steps:
        for dist, edges in ((gap, 1), (gap + 1, 0)):
            q = tuple(p[k] + dist * step[k] for k in range(nd))
            far = tuple(s - 1 for s in spatial)
            for flip in (0, 1):                               # the lower row at the lower and at the higher list position
                lists = _lists([{p: flip, q: 1 - flip}, {}, {q: 0, far: 1}], spatial)
                want = _check(lib, *lists, spatial, gap, value=np.arange(4, dtype=np.float32), cls=[1, 2, 1, 1])
                assert want["events"][:, 1].tolist() == [edges, 0, 0] and want["events"][:, 0].tolist() == [2 - edges, 0, 2]
                if edges:
                    assert want["edges"][0].tolist() == [1, 1, int(dist == 1), dist * dist * sum(step), flip, 1 - flip]


@pytest.mark.parametrize("gap", [1, 2, 3])
def test_index_neighbours_that_are_not_coordinate_neighbours(lib, gap):
    """Indices that follow each other across a row end and across a plane end; and entries with id -1 between two clusters."""
    s3, s2 = (7, 9, 11), (10, 13)
    want = _check(lib, *_lists([{(0, 0, 10): 0, (0, 1, 0): 1}, {}, {(0, 8, 10): 0, (1, 0, 0): 1}], s3), s3, gap)
    assert want["edge_offsets"][-1] == 0 and want["events"][:, 0].tolist() == [2, 0, 2]
    assert np.diff(_lists([{(0, 0, 10): 0, (0, 1, 0): 1}], s3)[1]).tolist() == [1]
    want = _check(lib, *_lists([{(0, 12): 0, (1, 0): 1}, {}, {(9, 12): 0, (0, 0): 1}], s2), s2, gap)
    assert want["edge_offsets"][-1] == 0
    want = _check(lib, *_lists([{(3, 4, 2): 0, (3, 4, 3): -1, (3, 4, 4): 1, (3, 5, 3): -1}, {}, {(3, 4, 3): -1}], s3), s3, gap)
    assert want["edge_offsets"][-1] == (0 if gap == 1 else 1) and want["group"].tolist() == [0, -1, 0 if gap > 1 else 1, -1, -1]
    if gap > 1:
        assert want["edges"][0].tolist() == [1, 1, 0, 4, 0, 2]


# ---- ties ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("flip", [0, 1])
def test_ties_fall_to_the_lowest_positions_and_the_lowest_id(lib, flip):
    s3 = (7, 9, 11)
    ev = {(2, 2, z): flip for z in (2, 3, 4)}
    ev.update({(2, 3, z): 1 - flip for z in (2, 3, 4)})          # three pairs at dist2 1, four at dist2 2
    ev.update({(4, 4, 8): 4, (4, 4, 9): 3, (4, 5, 8): 2})        # row 4 has two partners at dist2 1: the lower id, at the higher position
    want = _check(lib, *_lists([ev, {}, {(0, 0, 0): 0}], s3), s3, 1, cls=[1, 1, 2, 3, 4, 5])
    first = want["edges"][0].tolist()
    assert first[:4] == [1, 7, 7, 1] and first[4:] == ([0, 3] if flip == 0 else [3, 0])
    assert want["rows"][4].tolist()[:4] == [2, 1, 2, 1] and want["rows"][2, 2] == 4 and want["rows"][3, 2] == 4
    for gap in (2, 3):
        _check(lib, *_lists([ev, {}, {(0, 0, 0): 0}], s3), s3, gap)


# ---- groups --------------------------------------------------------------------------------------------------------------------------
def test_chains_numbering_and_isolated_rows(lib):
    """A chain of 7 clusters whose lowest row is in its middle; two chains that join only through the LAST row; rows of degree 0."""
    s3 = (7, 9, 11)
    ev = {(1, 1, z): i for z, i in enumerate([3, 2, 1, 0, 4, 5, 6])}
    ev.update({(3, 3, z): 7 + z for z in range(3)})
    ev.update({(5, 3, z): 10 + z for z in range(3)})
    ev.update({(4, 3, 3): 15, (4, 6, 3): 15})                    # the last row touches the ends of both chains
    ev.update({(6, 8, 10): 13, (0, 8, 10): 14})                  # isolated
    value = np.linspace(-2.0, 30.0, len(ev) + 2).astype(np.float32)
    want = _check(lib, *_lists([ev, {}, {(1, 1, 1): 0, (5, 5, 5): 1}], s3), s3, 1, value=value, cls=np.arange(18) % 5)
    assert want["rows"][:16, 1].tolist() == [0] * 7 + [1] * 6 + [2, 3, 1]
    assert want["groups"][:4, [0, 1, 10]].tolist() == [[7, 6, 0], [7, 6, 7], [1, 0, 13], [1, 0, 14]]
    assert want["events"].tolist() == [[4, 12, 2, 8], [0, 0, 0, 0], [2, 0, 2, 1]]
    _check(lib, *_lists([ev, {}, {(1, 1, 1): 0, (5, 5, 5): 1}], s3), s3, 3, value=value)


# ---- more than 256 edges in a workgroup, and edge_cap -----------------------------------------------------------------------------------
def _checkerboard(n=1):
    shape = (8, 8, 8)
    x = np.stack(np.unravel_index(np.arange(512), shape), 1)
    cls = (1 + x.sum(1) % 2).astype(np.uint8)
    off = np.arange(n + 1, dtype=np.int64) * 512
    index, cls = np.tile(np.arange(512, dtype=np.int64), n), np.tile(cls, n)
    ids, toff, tcls = _clustered(off, index, cls, shape, ClusterSpec(6, (1, 2), True, 1))
    assert toff[-1] == 512 * n                                   # every voxel its own cluster
    return shape, off, index, cls, ids, toff, tcls


def test_every_voxel_its_own_cluster(lib):
    shape, off, index, _, ids, toff, tcls = _checkerboard()
    want = _check(lib, off, index, ids, toff, shape, 1, value=np.ones(512, np.float32), cls=tcls)
    NE = int(want["edge_offsets"][-1])
    assert NE == 3 * 7 * 64 + 6 * 49 * 8 + 4 * 343 and want["events"].tolist() == [[1, NE, 0, 512]]
    for edge_cap, bit in ((NE - 1, OVERFLOW), (NE, 0), (NE // 3, OVERFLOW), (0, OVERFLOW)):
        for k, got in enumerate(_run(lib, off, index, ids, toff, shape, 1, None, None, 512, 512, NE, edge_cap, 512, 1, NE)):
            assert int(got["status"][0]) == bit, (edge_cap, k, int(got["status"][0]))


def test_cluster_graph_grows_its_edge_table():
    net = _net("fp32")
    shape, off, index, cls, ids, toff, tcls = _checkerboard()
    lists = [index]
    clusters = net.cluster_voxels(None, lists, cls, ClusterSpec(6, (1, 2), True, 1), shape=shape)
    want = cluster_graph_numpy(off, index, ids, toff, shape, ClusterGraphSpec(1), None, tcls)
    assert int(want["edge_offsets"][-1]) > 4 * int(toff[-1]) + 1024          # the precondition: the default table is too small
    got = net.cluster_graph(None, lists, clusters, ClusterGraphSpec(1), shape=shape)
    _same_graph(got, want, off, toff)


# ---- contention, several workgroups ---------------------------------------------------------------------------------------------------
_dense = {}


def _dense_case():
    if not _dense:
        shape = (16, 16, 12)
        rng = np.random.default_rng(11)
        index = np.arange(3072, dtype=np.int64)
        cls = rng.integers(0, 3, 3072).astype(np.uint8)
        off = np.array([0, 3072], np.int64)
        ids, toff, tcls = _clustered(off, index, cls, shape, ClusterSpec(26, (0, 1, 2), True, 1))
        _dense["case"] = (shape, off, index, ids, toff, tcls, rng.uniform(-3.0, 40.0, 3072).astype(np.float32))
    return _dense["case"]


@pytest.mark.parametrize("gap", [1, 2])
def test_giant_rows_that_alternate_from_lane_to_lane(lib, gap):
    shape, off, index, ids, toff, tcls, value = _dense_case()
    assert np.bincount(ids).max() > 800 and (ids[1:] != ids[:-1]).mean() > 0.5
    want = _check(lib, off, index, ids, toff, shape, gap, value=value, cls=tcls)
    assert want["edges"][:, 1].max() > 3000 and want["groups"][0, 2] > 3000


# ---- caps ------------------------------------------------------------------------------------------------------------------------------
def test_short_caps_bound_what_is_written(lib):
    rng = np.random.default_rng(9)
    shape = (20, 24)
    lists = [np.flatnonzero(rng.uniform(size=480) < 0.3) if e != 1 else np.zeros(0, np.int64) for e in range(3)]
    off = np.concatenate([[0], np.cumsum([x.size for x in lists])])
    index = np.concatenate(lists)
    cls = rng.integers(1, 4, index.size).astype(np.uint8)
    ids, toff, tcls = _clustered(off, index, cls, shape, ClusterSpec(4, None, True, 1))
    value = rng.uniform(-3.0, 40.0, index.size).astype(np.float32)
    want = cluster_graph_numpy(off, index, ids, toff, shape, ClusterGraphSpec(1))
    K, NG, NE = int(toff[-1]), int(want["group_offsets"][-1]), int(want["edge_offsets"][-1])
    assert K > 60 and 5 < NG < K and NE > 60
    for caps in ((0, None, None), (K - 1, None, None), (None, 0, None), (None, NG - 1, None), (None, None, 0), (None, None, NE - 1),
                 (K - 1, NG - 1, NE - 1), (0, 0, 0), (K + 5, NG + 5, NE + 5)):
        _check(lib, off, index, ids, toff, shape, 1, value, tcls, *caps)
    _check(lib, off, index, ids, toff, shape, 2, value, tcls, with_edges=False)
    _check(lib, off, index, ids, toff, shape, 1, value, tcls, edge_cap=NE + 1000)


def test_no_entries_and_no_rows(lib):
    z = np.zeros(0, np.int64)
    want = _check(lib, [0, 0, 0], z, z, [0, 0, 0], (7, 9, 11), 1, value=z.astype(np.float32), cls=z)
    assert want["events"].tolist() == [[0, 0, 0, 0]] * 2
    _check(lib, [0, 0], z, z, [0, 0], (10, 13), 3, cap_rows=5, cap_groups=3, edge_out_cap=4, edge_cap=7)
    _check(lib, [0, 4, 6], [1, 2, 3, 4, 0, 5], np.full(6, -1), [0, 0, 0], (10, 13), 2, value=np.ones(6, np.float32), edge_cap=0)
    _check(lib, [0, 1], [5], [0], [0, 1], (10, 13), 2, value=[np.inf], cls=[31], edge_cap=0)


# ---- guards --------------------------------------------------------------------------------------------------------------------------
def test_scratch_one_word_short_is_refused_before_any_launch(lib):
    lists = _lists([{(1, 1, 1): 0, (1, 1, 2): 1}], (7, 9, 11))
    _run(lib, *lists, (7, 9, 11), 1, None, None, 2, 2, 1, 1, 2, 2, 1, short_scratch=True)


def test_an_id_outside_its_events_rows_sets_status(lib):
    """The argument check's positive control: an id equal to K_e is never used as an index; the entry is skipped, *status is non-zero
    and no border is touched (checked inside _run).  Likewise an index outside the volume, and a row without a member."""
    s2 = (10, 13)
    off, index, ids, toff = _lists([{(1, 1): 0, (1, 2): 1, (2, 2): 0, (5, 5): 1}, {(1, 1): 0}], s2)
    for bad, bit in ((np.array([0, 2, 0, 1, 0]), 1), (np.array([0, -2, 0, 1, 0]), 1), (np.array([0, 0, 0, 0, 0]), 2)):
        for got in _run(lib, off, index, bad, toff, s2, 1, None, None, 3, 3, 3, 8, 3, 3, 3):
            assert int(got["status"][0]) & bit and not int(got["status"][0]) & OVERFLOW
    outside = index.copy()
    outside[3] = 130
    for got in _run(lib, off, outside, ids, toff, s2, 1, None, None, 3, 3, 3, 8, 3, 3, 3):
        assert int(got["status"][0]) & 4
    net = _net("fp32")
    lists = [index[:4], index[4:]]
    tables = [{"first": np.zeros(k, np.int32), "size": np.ones(k, np.int32), "cls": np.ones(k, np.uint8)} for k in (2, 1)]
    good = {"cluster": [ids[:4].astype(np.int32), ids[4:].astype(np.int32)], "clusters": tables}
    assert net.cluster_graph(None, lists, good, ClusterGraphSpec(1), shape=s2)[0]["event"]["edges"] == 1
    broken = {"cluster": [np.array([0, 2, 0, 1], np.int32), ids[4:].astype(np.int32)], "clusters": tables}
    with pytest.raises(_lib.UrsnError) as e:
        net.cluster_graph(None, lists, broken, ClusterGraphSpec(1), shape=s2)
    assert "cluster_graph" in str(e.value)


# ---- the largest legal extents (tests/_far_corner.py) ---------------------------------------------------------------
@pytest.mark.parametrize("shape", far.SHAPES_CAPPED, ids=far.shape_id)
def test_far_corner(lib, shape):
    """The random lists against the far faces, at the origin and across index 2^30 (tests/test_far_corner_host.py asserts what the
    batch reaches): every box of the search is clipped by a far face somewhere, and the group boxes carry the largest coordinates."""
    b = far.far_batch("random", shape).big
    for gap in (3, 1):
        want = _check(lib, b.off, b.index, b.cluster, b.toff, shape, gap, value=b.value, cls=b.tcls)
        assert want["edge_offsets"][-1] > 0
    hi = want["groups"][:, 7:7 + len(shape)]
    assert (hi.max(axis=0) == np.array(shape) - 1).all()
    cluster, toff, tcls = far.clustered("random", shape, 6 if len(shape) == 3 else 4, False)
    _check(lib, b.off, b.index, cluster, toff, shape, 3, value=None, cls=tcls)


# ---- net level -----------------------------------------------------------------------------------------------------------------
DIMS = (16, 16, 16, 1)
_cache = {}


def _net(prec):
    net = uresnet(dims=list(DIMS), num_class=3, base_num_outputs=4 if prec == "fp32" else 8, num_strides=2)
    net.construct(trainable=False, use_weight=False, seed=7, precision=prec)
    return net


def _events(shape=DIMS[:-1], n=2):
    if shape not in _cache:
        _cache[shape] = VoxelBatch.concat([sio.dense_to_voxels(*sio.lartpc_sparse(list(shape) + [1], 3, e)) for e in range(n)]).validate()
    return _cache[shape]


def _toff(tables):
    return np.concatenate([[0], np.cumsum([t["first"].size for t in tables])]).astype(np.int64)


def _same_graph(got, want, off, toff, edges=True):
    """A graph as the Python surface returns it equals the statement's tables, column by column."""
    assert len(got) == len(off) - 1
    eo, go = want["edge_offsets"], want["group_offsets"]
    for e, ev in enumerate(got):
        assert sorted(ev) == sorted(["rows", "groups", "group", "event"] + (["edge_offsets", "edges"] if edges else []))
        for c, name in enumerate(GRAPH_ROW):
            assert ev["rows"][name].dtype == np.int64 and np.array_equal(ev["rows"][name], want["rows"][toff[e]:toff[e + 1], c]), (e, name)
        for c, name in enumerate(GRAPH_GROUP):
            assert np.array_equal(ev["groups"][name], want["groups"][go[e]:go[e + 1], c]), (e, name)
        assert ev["group"].dtype == np.int32 and np.array_equal(ev["group"], want["group"][off[e]:off[e + 1]]), e
        assert ev["event"] == {name: int(want["events"][e, c]) for c, name in enumerate(GRAPH_EVENT)}, e
        if edges:
            assert np.array_equal(ev["edge_offsets"], eo[toff[e]:toff[e + 1] + 1] - eo[toff[e]]), e
            for c, name in enumerate(GRAPH_EDGE):
                assert np.array_equal(ev["edges"][name], want["edges"][eo[toff[e]]:eo[toff[e + 1]], c]), (e, name)


def _result_graph(net, r, vb, shape, gap):
    """r['graph'] equals the statement on the returned ids, and cluster_graph on the returned ids."""
    toff = _toff(r["clusters"])
    assert toff[-1] > 1
    want = cluster_graph_numpy(vb.offsets, vb.index, np.concatenate(r["cluster"]), toff, shape, ClusterGraphSpec(gap), vb.value,
                               np.concatenate([t["cls"] for t in r["clusters"]]))
    _same_graph(r["graph"], want, vb.offsets, toff)
    again = net.cluster_graph(None, vb, r, ClusterGraphSpec(gap), shape=shape)
    _same_graph(again, want, vb.offsets, toff)
    _same_graph(net.cluster_graph(None, vb, r, ClusterGraphSpec(gap), shape=shape, edges=False), want, vb.offsets, toff, edges=False)
    return want


def _same_result(x, y):
    assert sorted(x) == sorted(y)
    for key in x:
        if key == "clusters":
            assert all(np.array_equal(p[k], q[k]) and p[k].dtype == q[k].dtype for p, q in zip(x[key], y[key]) for k in p)
        elif isinstance(x[key], list):
            assert all(np.array_equal(p, q) and p.dtype == q.dtype for p, q in zip(x[key], y[key])), key
        else:
            assert x[key] == y[key], key


def test_inference_voxel_scores_with_graph():
    net, vb = _net("fp32"), _events()
    net.set_clustering(ClusterSpec(classes=(0, 1, 2), min_size=1))
    before = net.inference_voxel_scores(None, vb, want=("pred", "cluster"))          # the setter never called: today's keys
    assert sorted(before) == ["acc_all", "acc_nonzero", "cluster", "clusters", "index", "pred"]
    net.set_cluster_graph(ClusterGraphSpec(1))
    r = net.inference_voxel_scores(None, vb, want=("pred", "cluster"))
    assert sorted(r) == sorted(list(before) + ["graph"])
    want = _result_graph(net, r, vb, DIMS[:-1], 1)
    assert want["edge_offsets"][-1] > 0
    assert sorted(net.inference_voxel_scores(None, vb, want=("pred",))) == ["acc_all", "acc_nonzero", "index", "pred"]
    # two calls with different lists in between give the first call's bits again
    other = _events((16, 16, 16), 2)
    half = VoxelBatch.concat([sio.dense_to_voxels(*sio.lartpc_sparse(list(DIMS), 3, e)) for e in (5, 6, 7)]).validate()
    net.inference_voxel_scores(None, half, want=("pred", "cluster"))
    r2 = net.inference_voxel_scores(None, other, want=("pred", "cluster"))
    _same_graph(r2["graph"], want, vb.offsets, _toff(r["clusters"]))
    net.set_cluster_graph(None)
    _same_result(before, net.inference_voxel_scores(None, vb, want=("pred", "cluster")))
    r.pop("graph")
    _same_result(before, r)


def test_tiled_graph_is_in_the_large_shape():
    big = (32, 32, 32)
    vb = _events(big)
    net = _net("fp32")
    net.set_clustering(ClusterSpec(classes=(0, 1, 2), same_class=True))
    before = net.inference_tiled_voxel_scores(None, vb, big, want=("pred", "cluster"))
    net.set_cluster_graph(ClusterGraphSpec(2))
    r = net.inference_tiled_voxel_scores(None, vb, big, want=("pred", "cluster"))
    assert sorted(r) == sorted(list(before) + ["graph"]) and r["tiles_run"] > 1
    want = _result_graph(net, r, vb, big, 2)
    g = want["groups"]
    crossing = (g[:, 0] > 1) & ((g[:, 4:7] < 16) & (g[:, 7:10] >= 16)).any(1)       # rows of both sides of a tile border, one group
    assert crossing.any()
    net.set_cluster_graph(None)
    _same_result(before, net.inference_tiled_voxel_scores(None, vb, big, want=("pred", "cluster")))


# ---- driver --------------------------------------------------------------------------------------------------------------------
def _drive(tmp_path, tag, extra):
    from uresnet_amd.ssnet_trainval import ssnet_trainval
    inp = tmp_path / "input.cfg"
    inp.write_text("Dims [32, 32, 32, 1]\nNumClass 3\nGenerator 'lartpc_sparse'\nNumEntries 64\n"      # the driver's net has 5 strides
                   "Keys {'data': 'data', 'label': 'label', 'weight': 'weight'}\n")
    out = tmp_path / ("ssnet_%s.npy" % tag)
    ana = tmp_path / ("ana_%s.cfg" % tag)
    ana.write_text("NUM_CLASS 3\nBASE_NUM_FILTERS 4\nMAIN_INPUT_CONFIG '%s'\nANA_OUTPUT_CONFIG '%s'\nLOGDIR ''\nSAVE_FILE ''\n"
                   "ITERATIONS 1\nMINIBATCH_SIZE 2\nTRAIN False\nUSE_WEIGHTS False\nSUMMARY_STEPS 0\nCHECKPOINT_STEPS 0\n"
                   "SPARSE_IO True\nSPARSE_SCORES True\nANA_CLUSTER 'pred'\n%s" % (inp, out, extra))
    t = ssnet_trainval()
    with redirect_stdout(io.StringIO()):
        t.override_config(str(ana))
        t.initialize()
        res = t.ana_step()
        t.reset()
    with open(str(out), "rb") as f:
        return f.read(), res


def test_driver_writes_one_row_per_group(tmp_path):
    """The CSV's integers are the returned graph's; the driver's own records are byte for byte those of a run without the key."""
    csv = tmp_path / "graph.csv"
    plain, ref = _drive(tmp_path, "plain", "")
    with_key, res = _drive(tmp_path, "graph", "ANA_GRAPH '%s'\nGRAPH_GAP 2\n" % csv)
    assert with_key == plain and "graph" not in ref and sorted(res) == sorted(list(ref) + ["graph"])
    lines = csv.read_text().split("\n")
    total = sum(ev["event"]["groups"] for ev in res["graph"])
    assert lines[0] + "\n" == graph_csv_header() and lines[-1] == "" and len(lines) == 2 + total and total > 0
    at = 1
    for e, ev in enumerate(res["graph"]):
        for g in range(ev["event"]["groups"]):
            row = [int(x) for x in lines[at].split(",")]
            assert row == [int(res["entries"][e]), g] + [int(ev["groups"][name][g]) for name in GRAPH_GROUP], (e, g)
            at += 1
