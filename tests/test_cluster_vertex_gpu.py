"""Vertex candidates on the device (csrc/cluster_vertex.hip) against the numpy statement (uresnet_amd.clusters.cluster_vertices_numpy).
Every comparison is np.array_equal on every column, fp64 columns by their bits.  Op level: the lists, the object tables and every
output sit between 0xFF guard bands (tests/_guard.py); each case runs four times -- scratch filled 0xFF, filled 0x00, as the second
call left it (the same arguments again), and in the plain form (URSN_CLVTX_WAVE=0: one thread per end point, one insertion per pair)
-- and all four must give the statement's bits; everything at or beyond a count or a cap must be left untouched.  The object tables
the call reads are the statement's own (cluster_features_numpy, laid out as the device lays them out;
tests/test_cluster_features_gpu.py holds the device to those bits).  Net level: set_cluster_vertices with the voxel-score calls,
cluster_vertices, and the driver's ANA_VERTICES file."""
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
from uresnet_amd.clusters import (VERTEX_EVENT, VERTEX_INCIDENCE, VERTEX_INT, VERTEX_REAL, ClusterSpec, ClusterVertexSpec, cluster_numpy,
                                  cluster_vertices_numpy)
from uresnet_amd.ssnet import VoxelBatch, vertices_csv_header

pytestmark = pytest.mark.gpu

FI, FR = _lib.CLFEAT_I, _lib.CLFEAT_R
VI, VR, IN, EV = _lib.CLVTX_VI, _lib.CLVTX_VR, _lib.CLVTX_IN, _lib.CLVTX_EV
FEAT_INT = (("n", 0, 1), ("charge", 1, 1), ("s", 2, 3), ("lo", 5, 3), ("hi", 8, 3), ("m", 11, 3), ("d", 14, 3), ("dd", 17, 6),
            ("flags", 23, 1), ("end_lo", 24, 1), ("end_hi", 25, 1))
FEAT_REAL = (("centroid", 0, 3), ("cov", 3, 6), ("eval", 9, 3), ("axis", 12, 3), ("length", 15, 1), ("t_lo", 16, 1), ("t_hi", 17, 1))
ROUTES = ((0xFF, True), (0x00, True), (None, True), (0xFF, False))


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint64)


def _feature_tables(f):
    K = f["n"].shape[0]
    it, rt = np.zeros((K, FI), np.int64), np.zeros((K, FR), np.float64)
    for name, at, w in FEAT_INT:
        it[:, at:at + w] = f[name].reshape(K, w)
    for name, at, w in FEAT_REAL:
        rt[:, at:at + w] = f[name].astype(np.float64).reshape(K, w)
    return it, rt


def _untouched(a):
    return bool((np.ascontiguousarray(a).view(np.uint8) == 0xFF).all())


def _check(lib, off, index, value, cluster, toff, shape, spec, cls=None, cap_rows=None, cap_vertices=None, inc_cap=None, inc_out_cap=None,
           tamper=None, status=0):
    """Runs the case four times on guarded operands and compares every call with the statement; returns the statement.  With
    ``tamper(index, cluster, itab, rtab, cls)`` the device's copies are changed in place first: the four calls must then all report
    exactly ``status`` and agree with each other byte for byte; returns the first call's row_vertex."""
    import torch
    off, toff = np.asarray(off, np.int64), np.asarray(toff, np.int64)
    index, cluster = np.asarray(index, np.int64), np.asarray(cluster, np.int64)
    want = cluster_vertices_numpy(off, index, value, cluster, toff, shape, spec, cls)
    wvi = np.stack([want["vertices"][k] for k in VERTEX_INT], 1)
    wvr = np.stack([want["vertices"][k] for k in VERTEX_REAL], 1)
    fit, frt = _feature_tables(want["objects"])
    n, M, K = off.size - 1, int(off[-1]), int(toff[-1])
    V, I = int(want["vertex_offsets"][-1]), int(want["inc_offsets"][-1])
    index, cluster, cls = index.astype(np.int32), cluster.astype(np.int32), None if cls is None else np.array(cls, np.uint8)
    first = None
    if tamper is not None:
        tamper(index, cluster, fit, frt, cls)
    cap_rows = K if cap_rows is None else cap_rows
    slack = 0 if tamper is None else 64                                  # a skipped row can split a vertex or add a body
    cap_vertices = V + slack if cap_vertices is None else cap_vertices
    inc_cap = I + slack if inc_cap is None else inc_cap
    inc_out_cap = I + slack if inc_out_cap is None else inc_out_cap
    rows, verts, incs = min(cap_rows, K), min(cap_vertices, V), min(inc_out_cap, I)
    g_off, g_toff = Guarded(n + 1, torch.int64, off), Guarded(n + 1, torch.int64, toff)
    g_idx, g_cl = Guarded(max(M, 1), torch.int32), Guarded(max(M, 1), torch.int32)
    if M:
        g_idx.set(index), g_cl.set(cluster)
    g_it, g_rt = Guarded((max(K, 1), FI), torch.int64), Guarded((max(K, 1), FR), torch.float64)
    g_cls = None if cls is None else Guarded(max(K, 1), torch.uint8)
    if K:
        g_it.set(fit), g_rt.set(frt)
        if g_cls is not None:
            g_cls.set(cls)
    need = int(lib.ursn_cluster_vertices_scratch_bytes(n, M, inc_cap))
    assert need >= 8 and need % 8 == 0
    scratch = Guarded(need, torch.uint8)
    d = _lib.ursn_cluster_vtx_desc()
    d.ndim, d.n, d.m_total, d.radius, d.inc_cap = len(shape), n, M, spec.radius, inc_cap
    for i, s in enumerate(shape):
        d.spatial[i] = s
    d.offsets, d.index, d.cluster, d.table_offsets = g_off.ptr, g_idx.ptr, g_cl.ptr, g_toff.ptr
    d.itab, d.rtab, d.feat_cap = g_it.ptr, g_rt.ptr, K
    d.cls = None if g_cls is None else g_cls.ptr
    d.min_size, d.class_mask = spec.min_size, spec.class_mask()
    for k, (fill, wave) in enumerate(ROUTES):
        what = "call %d" % k
        if fill is not None:
            scratch.fill(fill)
        voff, ioff = Guarded(n + 1, torch.int64), Guarded(cap_vertices + 1, torch.int64)
        vi, vr = Guarded((max(cap_vertices, 1), VI), torch.int64), Guarded((max(cap_vertices, 1), VR), torch.float64)
        inc = Guarded((max(inc_out_cap, 1), IN), torch.int64)
        rv, ev = Guarded((max(cap_rows, 1), 2), torch.int32), Guarded((n, EV), torch.int64)
        status_out = Guarded(1, torch.int32)
        o = _lib.ursn_cluster_vtx_out()
        o.vertex_offsets, o.vtx_itab, o.vtx_rtab, o.cap_vertices = voff.ptr, vi.ptr, vr.ptr, cap_vertices
        o.inc_offsets, o.incidence, o.inc_out_cap = ioff.ptr, inc.ptr, inc_out_cap
        o.row_vertex, o.cap_rows, o.event, o.status = rv.ptr, cap_rows, ev.ptr, status_out.ptr
        if not wave:
            os.environ["URSN_CLVTX_WAVE"] = "0"
        try:
            _lib.check(lib.ursn_cluster_vertices(ctypes.byref(d), ctypes.byref(o), ctypes.c_void_p(scratch.ptr), need, None))
        finally:
            os.environ.pop("URSN_CLVTX_WAVE", None)
        torch.cuda.synchronize()
        named = [("vertex_offsets", voff), ("inc_offsets", ioff), ("vtx_itab", vi), ("vtx_rtab", vr), ("incidence", inc),
                 ("row_vertex", rv), ("event", ev), ("status", status_out), ("offsets", g_off), ("table_offsets", g_toff), ("index", g_idx),
                 ("cluster", g_cl), ("itab", g_it), ("rtab", g_rt), ("scratch", scratch)] + ([] if g_cls is None else [("cls", g_cls)])
        for name, g in named:
            g.check(name)
        code = int(status_out.numpy()[0])
        if tamper is not None:
            assert code == status, (what, code)
            outs = [g.numpy().copy() for _, g in named[:7]]
            first = outs if first is None else first
            for (name, _), a, b in zip(named, outs, first):
                assert np.array_equal(a.view(np.uint8), b.view(np.uint8)), (what, name, "differs from the first call")
            continue
        assert np.array_equal(voff.numpy(), want["vertex_offsets"]), what               # the true counts, whatever the caps are
        if I > inc_cap:
            assert code == _lib.CLVTX_INC_OVERFLOW, (what, code)
            for name, g in named[1:7]:
                assert _untouched(g.numpy()), (what, name, "written after an overflow")
            continue
        assert code == 0, (what, code)
        got_ioff, gvi, gvr, ginc, grv = ioff.numpy(), vi.numpy(), vr.numpy(), inc.numpy(), rv.numpy()
        assert np.array_equal(got_ioff[:verts + 1], want["inc_offsets"][:verts + 1]), what
        assert _untouched(got_ioff[verts + 1:]), (what, "inc_offsets beyond the vertices")
        for c, name in enumerate(VERTEX_INT):
            assert np.array_equal(gvi[:verts, c], wvi[:verts, c]), (what, "vertex", name)
        for c, name in enumerate(VERTEX_REAL):
            assert np.array_equal(_bits(gvr[:verts, c]), _bits(wvr[:verts, c])), (what, "vertex", name)
        for c, name in enumerate(VERTEX_INCIDENCE):
            assert np.array_equal(ginc[:incs, c], want["incidence"][:incs, c]), (what, "incidence", name)
        assert np.array_equal(grv[:rows], want["row_vertex"][:rows]), (what, "row_vertex")
        assert np.array_equal(ev.numpy(), want["events"]), (what, "events")
        assert _untouched(gvi[verts:]) and _untouched(gvr[verts:]), (what, "vertices at or beyond the count or cap were written")
        assert _untouched(ginc[incs:]), (what, "incidences at or beyond the count or cap were written")
        assert _untouched(grv[rows:]), (what, "rows at or beyond the count or cap were written")
    return want if tamper is None else first[5]


def _ids(off, index, cls, shape, spec):
    ids, counts, tcls = [], [], []
    for e in range(len(off) - 1):
        c, first, _, k = cluster_numpy(index[off[e]:off[e + 1]], cls[off[e]:off[e + 1]], shape, spec)
        ids.append(c), counts.append(first.size), tcls.append(k)
    return np.concatenate(ids), np.concatenate([[0], np.cumsum(counts)]).astype(np.int64), np.concatenate(tcls)


_made = {}


def _case(shape, same_class):
    """The four events of the profile test -- random, empty, random without a cluster (class 0 only), random -- with values holding
    an Inf, a NaN and 2^15; ids under ClusterSpec(26 | 8, (1, 2), same_class).  Made once per key and shared read-only."""
    key = (shape, same_class)
    if key not in _made:
        rng = np.random.default_rng(len(shape))
        vox, occ = int(np.prod(shape)), (0.1 if len(shape) == 3 else 0.45)
        lists = [np.flatnonzero(rng.uniform(size=vox) < occ), np.zeros(0, np.int64), np.flatnonzero(rng.uniform(size=vox) < occ / 2),
                 np.flatnonzero(rng.uniform(size=vox) < occ)]
        cls = [rng.integers(0, 3, a.size).astype(np.uint8) for a in lists]
        cls[2][:] = 0
        off = np.concatenate([[0], np.cumsum([a.size for a in lists])])
        index, cls = np.concatenate(lists), np.concatenate(cls)
        cluster, toff, tcls = _ids(off, index, cls, shape, ClusterSpec(26 if len(shape) == 3 else 8, (1, 2), same_class))
        value = rng.uniform(-3.0, 40.0, index.size).astype(np.float32)
        inside = np.flatnonzero(cluster >= 0)
        value[inside[3]], value[inside[40]], value[inside[-2]] = np.float32(np.inf), np.float32(np.nan), np.float32(2.0 ** 15)
        assert toff[1] > 2 and toff[2] == toff[1] == toff[3] and toff[4] > toff[3] and (cluster == -1).sum() > 10
        for a in (off, index, value, cluster, toff, tcls):
            a.setflags(write=False)
        _made[key] = (off, index, value, cluster, toff, tcls)
    return _made[key]


@pytest.mark.parametrize("min_size", [1, 3])
@pytest.mark.parametrize("radius", [1, 2, 3])
@pytest.mark.parametrize("same_class", [False, True], ids=["joined", "by_class"])
@pytest.mark.parametrize("shape", [(16, 16, 16), (12, 10)], ids=["3d", "2d"])
def test_random_lists(lib, shape, same_class, radius, min_size):
    """Under the joined spec nothing within distance 1 is another cluster, so radius 1 finds its links under the by-class spec."""
    off, index, value, cluster, toff, tcls = _case(shape, same_class)
    want = _check(lib, off, index, value, cluster, toff, shape, ClusterVertexSpec(radius, min_size), cls=tcls)
    v = want["vertices"]
    assert v["ends"].size > 0 and (radius == 1 and not same_class or (v["ends"] >= 2).any())
    if len(shape) == 3 and radius == 3:
        assert (v["mask_flags"] >> 32 & 1).any() and v["ends"].max() > 16      # the cosines stop at 16 directions


@pytest.mark.parametrize("shape", [(16, 16, 16), (12, 10)], ids=["3d", "2d"])
def test_without_values_without_cls_and_with_classes(lib, shape):
    off, index, value, cluster, toff, tcls = _case(shape, True)
    none = _check(lib, off, index, None, cluster, toff, shape, ClusterVertexSpec(2, 3), cls=tcls)
    assert (none["vertices"]["charge"] == 0).all() and (none["vertices"]["mask_flags"] & 6 != 0).all()
    bare = _check(lib, off, index, value, cluster, toff, shape, ClusterVertexSpec(2, 3), cls=None)
    assert (bare["vertices"]["mask_flags"] & 0xFFFFFFFF == 0).all() and (bare["vertices"]["charge"] != 0).any()
    only = _check(lib, off, index, value, cluster, toff, shape, ClusterVertexSpec(2, 2, (1,)), cls=tcls)
    assert (only["row_vertex"][tcls != 1] == -1).all() and (only["row_vertex"][tcls == 1] >= 0).any()
    assert (only["vertices"]["mask_flags"] & 2 != 0).all() and (only["incidence"][:, 1] == 0).any()


def test_every_voxel_its_own_cluster(lib):
    """Hundreds of distinct (vertex, row) keys in a workgroup, so its 256-slot table falls through to direct insertions, and one
    vertex with every end.  In 2-D every other column is filled: at radius 1 each column is a vertex, at radius 2 each event."""
    shape = (12, 10)
    index = np.arange(0, 120, 2)
    ids, toff = np.concatenate([np.arange(20), np.arange(40)]), [0, 20, 60]
    one = _check(lib, [0, 20, 60], index, None, ids, toff, shape, ClusterVertexSpec(1, 1))
    assert one["vertices"]["ends"].tolist() == [4] * 5 + [8] * 5 and one["events"].tolist() == [[5, 5, 0, 0], [5, 5, 0, 0]]
    big = _check(lib, [0, 20, 60], index, None, ids, toff, shape, ClusterVertexSpec(2, 1))
    assert big["events"][:, 0].tolist() == [1, 1] and big["vertices"]["ends"].tolist() == [20, 40]
    assert (big["vertices"]["mask_flags"] >> 32).tolist() == [3, 3] and (big["incidence"][:, 1] == 1).all()
    shape = (16, 16, 16)
    index = np.arange(0, 4096, 3)
    all3 = _check(lib, [0, index.size], index, None, np.arange(index.size), [0, index.size], shape, ClusterVertexSpec(3, 1))
    assert all3["vertices"]["ends"].tolist() == [index.size] and all3["inc_offsets"][-1] == index.size > 1024


def lattice(clusters):
    """Two-voxel clusters along the last axis on a lattice of pitch (2, 2, 4) in (2 * planes, 16, 16): at radius 1 no end point
    reaches another row, so there are 2 * clusters vertices with one incidence each."""
    pts = [(2 * (r // 32), 2 * ((r // 4) % 8), 4 * (r % 4) + k) for r in range(clusters) for k in range(2)]
    shape = (2 * ((clusters + 31) // 32), 16, 16)
    index = np.ravel_multi_index(np.array(pts).T, shape)
    assert (np.diff(index) > 0).all()
    return shape, index, np.repeat(np.arange(clusters), 2)


def test_more_keys_than_one_step_of_the_scan_and_one_sweep_of_the_walk(lib):
    """2,100 rows = 4,200 keys and 4,200 vertices: the one-workgroup scans of 1,024 threads take chunks of five (the last threads
    none), the walk kernels' 1,024 workgroups of four end points sweep twice (the second sweep ragged), and every striding kernel
    runs more than one workgroup.  tests/test_cluster_vertex_host.py derives these numbers from the source."""
    shape, index, ids = lattice(2100)
    want = _check(lib, [0, index.size], index, None, ids, [0, 2100], shape, ClusterVertexSpec(1, 2))
    assert want["vertex_offsets"].tolist() == [0, 4200] and (want["vertices"]["rows"] == 1).all()
    assert (want["incidence"][:, 2] == 2).all() and sorted(set(want["incidence"][:, 1])) == [1, 2]


def test_caps_and_overflow(lib):
    shape = (16, 16, 16)
    off, index, value, cluster, toff, tcls = _case(shape, False)
    spec = ClusterVertexSpec(2, 3)
    want = cluster_vertices_numpy(off, index, value, cluster, toff, shape, spec, tcls)
    K, V, I = int(toff[-1]), int(want["vertex_offsets"][-1]), int(want["inc_offsets"][-1])
    for cap_rows in (K + 3, K // 2, 0):
        _check(lib, off, index, value, cluster, toff, shape, spec, cls=tcls, cap_rows=cap_rows)
    for cap_vertices in (V + 2, V // 2, 1, 0):
        _check(lib, off, index, value, cluster, toff, shape, spec, cls=tcls, cap_vertices=cap_vertices)
    for inc_out_cap in (I + 2, I // 2, 0):
        _check(lib, off, index, value, cluster, toff, shape, spec, cls=tcls, inc_out_cap=inc_out_cap)
    _check(lib, off, index, value, cluster, toff, shape, spec, cls=tcls, inc_cap=I + 7)
    _check(lib, off, index, value, cluster, toff, shape, spec, cls=tcls, inc_cap=I - 1)     # overflow: vertex_offsets and status only
    _check(lib, off, index, value, cluster, toff, shape, spec, cls=tcls, inc_cap=0)


def test_inconsistent_tables_set_their_status_bit(lib):
    """One inconsistency at a time, each reported as its own bit by all four calls (the bits that the first launch finds reach the
    status word through a later launch, so none is lost to the store that starts the word), and the row is skipped."""
    shape = (16, 16, 16)
    off, index, value, cluster, toff, tcls = _case(shape, False)
    spec = ClusterVertexSpec(2, 3)
    f = cluster_vertices_numpy(off, index, value, cluster, toff, shape, spec, tcls)["objects"]
    big = np.flatnonzero(f["n"][:toff[1]] >= 5)
    r0, r1 = int(big[0]), int(big[1])                                      # two eligible rows of the first event
    inner = [int(j) for j in np.flatnonzero(cluster[:off[1]] == r0) if j not in (f["end_lo"][r0], f["end_hi"][r0])][0]

    def other_row(index, cluster, itab, rtab, cls):
        itab[r0, 25] = f["end_lo"][r1]                                    # end_hi: a member of another row
    def no_member(index, cluster, itab, rtab, cls):
        itab[r0, 0] = 0
    def bad_class(index, cluster, itab, rtab, cls):
        cls[r0] = 32
    def bad_id(index, cluster, itab, rtab, cls):
        cluster[inner] = int(toff[1]) + 3                                 # beyond its event's rows
    def bad_index(index, cluster, itab, rtab, cls):
        index[off[1] - 1] = 16 ** 3 + 5                                   # the event's last entry: the list stays sorted
    assert cluster[off[1] - 1] >= 0
    for tamper, bit, skipped in ((other_row, 32, True), (no_member, 2, True), (bad_class, 16, True), (bad_id, 1, False),
                                 (bad_index, 4, None)):
        rv = _check(lib, off, index, value, cluster, toff, shape, spec, cls=tcls, tamper=tamper, status=bit)
        if skipped is not None:
            assert (rv[r0].tolist() == [-1, -1]) == skipped and rv[r1].min() >= 0, (tamper.__name__, rv[r0], rv[r1])


def test_no_entries_and_no_clusters(lib):
    shape = (6, 7, 8)
    z = np.zeros(0, np.int64)
    spec = ClusterVertexSpec()
    _check(lib, [0, 0, 0], z, None, z, [0, 0, 0], shape, spec)
    _check(lib, [0, 0], z, None, z, [0, 0], shape, spec, cap_rows=5, cap_vertices=4, inc_cap=7, inc_out_cap=3)
    want = _check(lib, [0, 4, 6], np.array([1, 5, 9, 200, 3, 4]), None, np.full(6, -1), [0, 0, 0], shape, spec, cap_rows=6, cap_vertices=6,
                  inc_cap=6, inc_out_cap=6)
    assert want["events"].tolist() == [[0, 0, 0, -1], [0, 0, 0, -1]]


# ---- the largest legal extents (tests/_far_corner.py) ---------------------------------------------------------------
@pytest.mark.parametrize("shape", far.SHAPES_CAPPED, ids=far.shape_id)
def test_far_corner(lib, shape):
    """The random lists against the far faces, at the origin and across index 2^30 (tests/test_far_corner_host.py asserts what the
    batch reaches): the end points' neighbourhoods are clipped by the far faces and the vertex records carry the largest positions."""
    b = far.far_batch("random", shape).big
    want = _check(lib, b.off, b.index, b.value, b.cluster, b.toff, shape, far.WIDEST["vertex"], cls=b.tcls)
    v = want["vertices"]
    assert v["n"].size > 0 and all(v["hi%d" % a].max() == shape[a] - 1 for a in range(len(shape)))
    cluster, toff, tcls = far.clustered("random", shape, 6 if len(shape) == 3 else 4, False)
    _check(lib, b.off, b.index, None, cluster, toff, shape, ClusterVertexSpec(3, 1, (1, 2)), cls=tcls)
    _check(lib, b.off, b.index, b.value, b.cluster, b.toff, shape, ClusterVertexSpec(1, 3), cls=None)


@pytest.mark.parametrize("axis", sorted(far.LONG_TRACK))
def test_a_track_across_the_longest_axis(lib, axis):
    """One cluster of 32,768 members whose two end points are the origin corner and the far corner: two free ends."""
    s = far.long_track(far.LONG_TRACK[axis])
    want = _check(lib, s.off, s.index, s.value, s.cluster, s.toff, s.shape, far.WIDEST["vertex"], cls=s.tcls)
    assert want["events"][0, 0] == 2 and sorted(want["vertices"]["hi%d" % axis].tolist())[-1] == 32767


# ---- net level -----------------------------------------------------------------------------------------------------------------
DIMS = (32, 32, 32, 1)
_cache = {}


def _net(prec="fp32"):
    net = uresnet(dims=list(DIMS), num_class=3, base_num_outputs=8, num_strides=2)
    net.construct(trainable=False, use_weight=False, seed=7, precision=prec)
    return net


def _events(n=2):
    if "vb" not in _cache:
        _cache["vb"] = VoxelBatch.concat([sio.dense_to_voxels(*sio.lartpc_sparse(list(DIMS), 3, e)) for e in range(n)]).validate()
    return _cache["vb"]


def _same_vertices(r, vb, shape, spec):
    """r['vertices'] equals the statement evaluated on r['index'], the batch's values, r['cluster'] and the table's cls."""
    counts = [t["first"].size for t in r["clusters"]]
    toff = np.concatenate([[0], np.cumsum(counts)])
    cls = np.concatenate([t["cls"] for t in r["clusters"]])
    want = cluster_vertices_numpy(vb.offsets, np.concatenate(r["index"]), vb.value, np.concatenate(r["cluster"]), toff, shape, spec, cls)
    assert len(r["vertices"]) == len(counts) and toff[-1] > 0 and want["vertex_offsets"][-1] > 0
    voff, ioff = want["vertex_offsets"], want["inc_offsets"]
    for i, got in enumerate(r["vertices"]):
        assert sorted(got) == ["event", "inc_offsets", "incidence", "objects", "row_vertex", "vertices"]
        lo, hi = voff[i], voff[i + 1]
        assert sorted(got["vertices"]) == sorted(VERTEX_INT + VERTEX_REAL)
        for name in VERTEX_INT + VERTEX_REAL:
            w = want["vertices"][name][lo:hi]
            assert got["vertices"][name].dtype == w.dtype and np.array_equal(_bits(got["vertices"][name]), _bits(w)), (i, name)
        assert np.array_equal(got["inc_offsets"], ioff[lo:hi + 1] - ioff[lo]), i
        assert np.array_equal(got["incidence"], want["incidence"][ioff[lo]:ioff[hi]]), i
        assert np.array_equal(got["row_vertex"], want["row_vertex"][toff[i]:toff[i + 1]]), i
        assert got["event"] == dict(zip(VERTEX_EVENT, (int(x) for x in want["events"][i]))), i
        for name in ("end_lo", "end_hi", "axis", "n"):
            assert np.array_equal(got["objects"][name], want["objects"][name][toff[i]:toff[i + 1]]), (i, name)
    return want


def test_inference_voxel_scores_with_vertices():
    net, vb = _net(), _events()
    net.set_clustering(ClusterSpec(classes=(0, 1, 2), min_size=2))
    before = net.inference_voxel_scores(None, vb, with_labels=False, want=("pred", "cluster"))
    assert sorted(before) == ["cluster", "clusters", "index", "pred"]                 # the setter never called: the parent's keys
    spec = ClusterVertexSpec(2, 3)
    net.set_cluster_vertices(spec)
    r = net.inference_voxel_scores(None, vb, with_labels=False, want=("pred", "cluster"))
    assert sorted(r) == ["cluster", "clusters", "index", "pred", "vertices"]          # the object records ran, and are not a key
    assert all(np.array_equal(a, b) for a, b in zip(r["cluster"], before["cluster"]))
    want = _same_vertices(r, vb, DIMS[:-1], spec)
    assert sorted(net.inference_voxel_scores(None, vb, with_labels=False, want=("pred",))) == ["index", "pred"]
    # the stand-alone call on the same lists gives the same records
    again = net.cluster_vertices(None, vb, None, {"cluster": r["cluster"], "clusters": r["clusters"]}, spec)
    _same_vertices(dict(r, vertices=again), vb, DIMS[:-1], spec)
    # an incidence table that is too small is made again through the doubling path
    assert want["inc_offsets"][-1] > 3
    net._vertex_inc_cap = lambda K: 3
    _same_vertices(net.inference_voxel_scores(None, vb, with_labels=False, want=("pred", "cluster")), vb, DIMS[:-1], spec)
    del net._vertex_inc_cap
    other = ClusterVertexSpec(3, 1, (1, 2))
    net.set_cluster_vertices(other)
    _same_vertices(net.inference_voxel_scores(None, vb, with_labels=False, want=("pred", "cluster")), vb, DIMS[:-1], other)
    net.set_cluster_vertices(None)
    assert sorted(net.inference_voxel_scores(None, vb, with_labels=False, want=("pred", "cluster"))) == \
        ["cluster", "clusters", "index", "pred"]


def test_tiled_vertices_are_in_the_large_shape():
    big, halo = (48, 40, 56), 4                                                       # two tiles per axis
    vb = VoxelBatch.concat([sio.dense_to_voxels(*sio.lartpc_sparse(list(big) + [1], 3, e)) for e in range(2)]).validate()
    net = _net()
    net.set_clustering(ClusterSpec(classes=(0, 1, 2), same_class=True))
    spec = ClusterVertexSpec(2, 3)
    net.set_cluster_vertices(spec)
    r = net.inference_tiled_voxel_scores(None, vb, big, halo=halo, want=("pred", "cluster"))
    assert "vertices" in r and "objects" not in r
    _same_vertices(r, vb, big, spec)


# ---- driver --------------------------------------------------------------------------------------------------------------------
def _drive(tmp_path, tag, extra):
    from uresnet_amd.ssnet_trainval import ssnet_trainval
    inp = tmp_path / "input.cfg"
    inp.write_text("Dims [32, 32, 32, 1]\nNumClass 3\nGenerator 'lartpc_sparse'\nNumEntries 64\n"
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


def test_driver_writes_one_row_per_vertex(tmp_path):
    """The CSV parses back to the returned records; the driver's own records are byte for byte those of a run without the key."""
    csv = tmp_path / "vertices.csv"
    plain, ref = _drive(tmp_path, "plain", "")
    with_key, res = _drive(tmp_path, "vertices", "ANA_VERTICES '%s'\nVERTEX_RADIUS 3\nVERTEX_MIN_SIZE 2\n" % csv)
    assert with_key == plain                                                          # the records do not change
    lines = csv.read_text().split("\n")
    assert lines[0] + "\n" == vertices_csv_header() and lines[-1] == ""
    names = lines[0].split(",")
    rows = [dict(zip(names, line.split(","))) for line in lines[1:-1]]
    at = 0
    for e, (ev, ev0) in enumerate(zip(res["voxels"], ref["voxels"])):
        assert sorted(ev) == sorted(list(ev0) + ["vertices"])
        got = ev["vertices"]["vertices"]
        assert got["ends"].size == ev["vertices"]["event"]["vertices"] > 0
        for k in range(got["ends"].size):
            row = rows[at]
            at += 1
            assert (int(row["entry"]), int(row["vertex"])) == (int(res["entries"][e]), k)
            for name in VERTEX_INT:
                assert int(row[name]) == int(got[name][k]), (e, k, name)
            for name in VERTEX_REAL:
                assert float(row[name]) == got[name][k], (e, k, name)
    assert at == len(rows)
