"""Cluster splits on the device (csrc/cluster_split.hip) against the numpy statement (uresnet_amd.clusters.cluster_split_numpy).
Every comparison is np.array_equal on every column, fp64 columns by their bits.  Op level: the lists, the cluster table and every
output sit between 0xFF guard bands (tests/_guard.py); each case runs four times -- scratch filled 0xFF, filled 0x00, as the second
call left it (the same arguments again), and in the other form (URSN_CLSPLIT_WAVE=1: one wave64 per entry; the plain form, one
thread per entry, is the default because it measured faster) -- and all four must give the statement's bits; everything at or beyond a count or a cap must be left untouched.  The lists are those of
tests/_split_cases.py, whose coverage tests/test_cluster_split_host.py asserts.  Net level: cluster_split on the clusters a
voxel-score call returned and the pieces as the clustering of another call; set_cluster_split with the plain and the tiled
voxel-score calls, downstream=True against the stand-alone calls made on the pieces, the feature off byte for byte as before; the
driver's ANA_SPLIT file."""
import ctypes
import os

import numpy as np
import pytest

import _far_corner as far
import _split_cases as cases
from _guard import Guarded
from uresnet_amd import _lib, uresnet
from uresnet_amd import synthetic_io as sio
from uresnet_amd.clusters import (SPLIT_EVENT, SPLIT_JUNCTION_INT, SPLIT_JUNCTION_REAL, SPLIT_PIECE, SPLIT_ROW, ClusterSpec,
                                  ClusterSplitSpec, cluster_features_numpy, cluster_split_numpy)
from uresnet_amd.ssnet import VoxelBatch

pytestmark = pytest.mark.gpu

PI, JI, JR, ROW, EV = _lib.CLSPLIT_PI, _lib.CLSPLIT_JI, _lib.CLSPLIT_JR, _lib.CLSPLIT_ROW, _lib.CLSPLIT_EV
ROUTES = ((0xFF, None), (0x00, None), (None, "0"), (0xFF, "1"))      # (scratch fill, URSN_CLSPLIT_WAVE)


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint64)


def _untouched(a):
    return bool((np.ascontiguousarray(a).view(np.uint8) == 0xFF).all())


def _check(lib, c, spec, want=None, use_cls=True, cap_pieces=None, cap_junctions=None, cap_rows=None, tamper=None, status=0):
    """Runs the case four times on guarded operands and compares every call with the statement ``want`` (computed here when not
    given); returns it.  With ``tamper(index, cluster, size, cls)`` the device's copies are changed in place first: the four calls
    must then all report exactly ``status`` and agree with each other byte for byte; returns the first call's outputs by name."""
    import torch
    off, toff, shape = np.asarray(c["off"], np.int64), np.asarray(c["toff"], np.int64), c["shape"]
    cls = np.array(c["cls"], np.uint8) if use_cls else None
    if want is None:
        want = cluster_split_numpy(off, c["index"], c["cluster"], toff, c["size"], shape, spec, cls)
    wpi = np.stack([want["pieces"][k] for k in SPLIT_PIECE], 1).reshape(-1, PI)
    wji = np.stack([want["junctions"][k] for k in SPLIT_JUNCTION_INT], 1).reshape(-1, JI)
    wjr = np.stack([want["junctions"][k] for k in SPLIT_JUNCTION_REAL], 1).reshape(-1, JR)
    n, M, K = off.size - 1, int(off[-1]), int(toff[-1])
    P, J = int(want["piece_offsets"][-1]), int(want["junction_offsets"][-1])
    index, cluster, size = np.array(c["index"], np.int32), np.array(c["cluster"], np.int32), np.array(c["size"], np.int32)
    first = None
    if tamper is not None:
        tamper(index, cluster, size, cls)
    cap_pieces = (P if tamper is None else M) if cap_pieces is None else cap_pieces
    cap_junctions = (J if tamper is None else M) if cap_junctions is None else cap_junctions
    cap_rows = K if cap_rows is None else cap_rows
    pieces, junctions, rows = min(cap_pieces, P), min(cap_junctions, J), min(cap_rows, K)
    g_off, g_toff = Guarded(n + 1, torch.int64, off), Guarded(n + 1, torch.int64, toff)
    g_idx, g_cl = Guarded(max(M, 1), torch.int32), Guarded(max(M, 1), torch.int32)
    g_size, g_cls = Guarded(max(K, 1), torch.int32), None if cls is None else Guarded(max(K, 1), torch.uint8)
    if M:
        g_idx.set(index), g_cl.set(cluster)
    if K:
        g_size.set(size)
        if g_cls is not None:
            g_cls.set(cls)
    need = int(lib.ursn_cluster_split_scratch_bytes(n, M))
    assert need >= 8 and need % 8 == 0
    scratch = Guarded(need, torch.uint8)
    d = _lib.ursn_cluster_split_desc()
    d.ndim, d.n, d.m_total, d.radius = len(shape), n, M, spec.radius
    for i, s in enumerate(shape):
        d.spatial[i] = s
    d.offsets, d.index, d.cluster, d.table_offsets, d.size = g_off.ptr, g_idx.ptr, g_cl.ptr, g_toff.ptr, g_size.ptr
    d.cls = None if g_cls is None else g_cls.ptr
    d.kink_cos, d.min_size, d.class_mask, d.grow = spec.kink_cos, spec.min_size, spec.class_mask(), spec.grow
    for k, (fill, wave) in enumerate(ROUTES):
        what = "call %d" % k
        if fill is not None:
            scratch.fill(fill)
        split, mark = Guarded(max(M, 1), torch.int32), Guarded(max(M, 1), torch.uint8)
        poff, joff = Guarded(n + 1, torch.int64), Guarded(n + 1, torch.int64)
        t_first, t_size, t_cls = (Guarded(max(cap_pieces, 1), dt) for dt in (torch.int32, torch.int32, torch.uint8))
        pi = Guarded((max(cap_pieces, 1), PI), torch.int64)
        ji, jr = Guarded((max(cap_junctions, 1), JI), torch.int64), Guarded((max(cap_junctions, 1), JR), torch.float64)
        rw, ev, status_out = Guarded((max(cap_rows, 1), ROW), torch.int32), Guarded((n, EV), torch.int64), Guarded(1, torch.int32)
        o = _lib.ursn_cluster_split_out()
        o.split, o.mark, o.piece_offsets, o.first, o.size, o.cls = split.ptr, mark.ptr, poff.ptr, t_first.ptr, t_size.ptr, t_cls.ptr
        o.piece_itab, o.cap_pieces = pi.ptr, cap_pieces
        o.junction_offsets, o.junction_itab, o.junction_rtab, o.cap_junctions = joff.ptr, ji.ptr, jr.ptr, cap_junctions
        o.rows, o.cap_rows, o.event, o.status = rw.ptr, cap_rows, ev.ptr, status_out.ptr
        if wave is not None:
            os.environ["URSN_CLSPLIT_WAVE"] = wave
        try:
            _lib.check(lib.ursn_cluster_split(ctypes.byref(d), ctypes.byref(o), ctypes.c_void_p(scratch.ptr), need, None))
        finally:
            os.environ.pop("URSN_CLSPLIT_WAVE", None)
        torch.cuda.synchronize()
        named = [("split", split), ("mark", mark), ("piece_offsets", poff), ("junction_offsets", joff), ("first", t_first),
                 ("size", t_size), ("table cls", t_cls), ("piece_itab", pi), ("junction_itab", ji), ("junction_rtab", jr), ("rows", rw),
                 ("event", ev), ("status", status_out), ("offsets", g_off), ("table_offsets", g_toff), ("index", g_idx),
                 ("cluster", g_cl), ("table size", g_size), ("scratch", scratch)] + ([] if g_cls is None else [("cls", g_cls)])
        for name, g in named:
            g.check(name)
        code = int(status_out.numpy()[0])
        if tamper is not None:
            assert code == status, (what, code)
            outs = {name: g.numpy().copy() for name, g in named[:12]}
            first = outs if first is None else first
            for name in outs:
                assert np.array_equal(outs[name].view(np.uint8), first[name].view(np.uint8)), (what, name, "differs from the first call")
            continue
        assert code == 0, (what, code)
        assert np.array_equal(poff.numpy(), want["piece_offsets"]) and np.array_equal(joff.numpy(), want["junction_offsets"]), what
        assert np.array_equal(ev.numpy(), want["events"]), (what, "events")                  # the true counts, whatever the caps are
        if M:
            assert np.array_equal(mark.numpy(), want["mark"]), (what, "mark", np.flatnonzero(mark.numpy() != want["mark"])[:8])
            assert np.array_equal(split.numpy(), want["split"]), (what, "split", np.flatnonzero(split.numpy() != want["split"])[:8])
        else:
            assert _untouched(split.numpy()) and _untouched(mark.numpy()), (what, "split / mark of an empty list")
        gpi, gji, gjr = pi.numpy(), ji.numpy(), jr.numpy()
        for col, name in enumerate(SPLIT_PIECE):
            assert np.array_equal(gpi[:pieces, col], wpi[:pieces, col]), (what, "piece", name)
        for col, name in enumerate(SPLIT_JUNCTION_INT):
            assert np.array_equal(gji[:junctions, col], wji[:junctions, col]), (what, "junction", name)
        for col, name in enumerate(SPLIT_JUNCTION_REAL):
            assert np.array_equal(_bits(gjr[:junctions, col]), _bits(wjr[:junctions, col])), (what, "junction", name)
        for name, g in (("first", t_first), ("size", t_size), ("cls", t_cls)):
            assert g.numpy().dtype == want["table"][name].dtype and np.array_equal(g.numpy()[:pieces], want["table"][name][:pieces]), (what, name)
            assert _untouched(g.numpy()[pieces:]), (what, name, "beyond the count or cap")
        assert np.array_equal(rw.numpy()[:rows], want["rows"][:rows]), (what, "rows")
        assert _untouched(gpi[pieces:]), (what, "pieces at or beyond the count or cap were written")
        assert _untouched(gji[junctions:]) and _untouched(gjr[junctions:]), (what, "junctions at or beyond the count or cap were written")
        assert _untouched(rw.numpy()[rows:]), (what, "rows beyond")
    return want if tamper is None else first


@pytest.mark.parametrize("radius", [1, 2, 3])
@pytest.mark.parametrize("name", sorted(cases.CASES))
def test_the_cases_at_every_radius(lib, name, radius):
    spec = ClusterSplitSpec(radius)
    _check(lib, cases.case(name), spec, cases.statement(name, spec))


@pytest.mark.parametrize("name,spec", [
    ("jacks", ClusterSplitSpec(3, -0.7, 8, None, 1)),            # the junction of 13 keeps seven: a piece of kind 2
    ("jacks", ClusterSplitSpec(3, -0.7, 8, None, 0)),
    ("shapes3d", ClusterSplitSpec(2, 1.0, 8, None, 0)),          # kinks off, nothing attached
    ("shapes3d", ClusterSplitSpec(2, -0.95, 4, None, 1)),        # nearly every bend a kink
    ("shapes2d", ClusterSplitSpec(3, -1.0, 1, None, 8)),
    ("mixed", ClusterSplitSpec(2, -0.7, 8, (1, 2), None)),       # a row of class 3 stays whole
    ("mixed", ClusterSplitSpec(1, 0.0, 3, (2,), 2)),
], ids=lambda v: v if isinstance(v, str) else repr(v)[17:-1])
def test_other_settings(lib, name, spec):
    want = _check(lib, cases.case(name), spec, cases.statement(name, spec))
    assert want["piece_offsets"][-1] > 0


def test_without_cls(lib):
    spec = ClusterSplitSpec(2)
    want = _check(lib, cases.case("mixed"), spec, use_cls=False)
    assert (want["table"]["cls"] == 0).all() and want["junction_offsets"][-1] > 0


def test_replicated_events_cross_the_one_step_scan(lib):
    """The one-workgroup scans take one tile of 64 entries per thread up to 65,536 entries; 59 copies of the 1,117 entries of `many`
    are 65,903 entries = 1,030 tiles, two per thread.  The expected tables are the statement's on the base, replicated."""
    spec = ClusterSplitSpec(2)
    big, want = cases.replicate(cases.case("many"), cases.statement("many", spec), 59)
    assert big["off"][-1] == 65903 and -(-65903 // 64) > 1024
    _check(lib, big, spec, want)


def test_caps(lib):
    spec = ClusterSplitSpec(2)
    c, want = cases.case("shapes3d"), cases.statement("shapes3d", spec)
    K, P, J = int(c["toff"][-1]), int(want["piece_offsets"][-1]), int(want["junction_offsets"][-1])
    assert P >= 4 and J >= 4
    for cap in (K + 3, K // 2, 0):
        _check(lib, c, spec, want, cap_rows=cap)
    for cap in (P + 2, P // 2, 0):
        _check(lib, c, spec, want, cap_pieces=cap)
    for cap in (J + 2, J // 2, 0):
        _check(lib, c, spec, want, cap_junctions=cap)


def test_inconsistent_lists_set_their_status_bit(lib):
    """One inconsistency at a time, each reported as its own bit by all four calls, which agree byte for byte."""
    spec = ClusterSplitSpec(2)
    c, want = cases.case("shapes3d"), cases.statement("shapes3d", spec)
    off, toff = c["off"], c["toff"]
    inner = int(off[0]) + 7
    last = int(off[1]) - 1
    assert c["cluster"][inner] >= 0 and c["cluster"][last] >= 0

    def bad_id(index, cluster, size, cls):
        cluster[inner] = int(toff[1] - toff[0]) + 3                       # beyond its event's rows
    def bad_index(index, cluster, size, cls):
        index[last] = int(np.prod(c["shape"])) + 5                        # the event's last entry: the list stays sorted
    def bad_order(index, cluster, size, cls):
        index[inner] = index[inner - 1]
    def bad_class(index, cluster, size, cls):
        cls[0] = 32
    for tamper, bit in ((bad_id, 1), (bad_index, 4), (bad_order, 2), (bad_class, 16)):
        got = _check(lib, c, spec, want, tamper=tamper, status=bit)
        if tamper is bad_id:
            assert got["split"][inner] == -1 and got["mark"][inner] == 0
        if tamper is bad_class:
            assert (got["split"][off[0]:off[1]][c["cluster"][off[0]:off[1]] == 0] == -1).all()


def test_no_entries_and_no_clusters(lib):
    z, z32 = np.zeros(0, np.int64), np.zeros(0, np.int32)
    spec = ClusterSplitSpec()
    empty = lambda off, toff, index=z, cluster=z: {"shape": (6, 7, 8), "off": np.array(off), "toff": np.array(toff), "index": index,
                                                   "cluster": cluster, "size": z32, "cls": np.zeros(0, np.uint8)}
    _check(lib, empty([0, 0, 0], [0, 0, 0]), spec)
    _check(lib, empty([0, 0], [0, 0]), spec, cap_rows=5, cap_pieces=4, cap_junctions=3)
    want = _check(lib, empty([0, 4, 6], [0, 0, 0], np.array([1, 5, 9, 200, 3, 4]), np.full(6, -1)), spec, cap_rows=6, cap_pieces=6,
                  cap_junctions=6)
    assert want["events"].tolist() == [[0, 0, 0, 0], [0, 0, 0, 0]] and want["split"].tolist() == [-1] * 6


# ---- the largest legal extents (tests/_far_corner.py) ---------------------------------------------------------------
@pytest.mark.parametrize("shape", far.SHAPES_CAPPED, ids=far.shape_id)
def test_far_corner(lib, shape):
    """The cases against the far faces, at the origin and across index 2^30, at radius 3: balls that a far face clips around
    junctions (tests/test_far_corner_host.py asserts that a junction lies within the radius of a far face)."""
    b = far.far_batch("split", shape).big
    want = _check(lib, far.split_case(b), far.WIDEST["split"])
    j = want["junctions"]
    assert j["row"].size > 0 and any(j["hi%d" % a].max() >= shape[a] - 4 for a in range(len(shape)))
    _check(lib, far.split_case(b), ClusterSplitSpec(1, -0.95, 4, None, 1), use_cls=False)


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


def _same_split(got, vb, index, clusters, shape, spec):
    """``got`` (what cluster_split returns) equals the statement on the lists and the clustering ``clusters``."""
    counts = [t["first"].size for t in clusters["clusters"]]
    toff = np.concatenate([[0], np.cumsum(counts)])
    cls = np.concatenate([t["cls"] for t in clusters["clusters"]])
    size = np.concatenate([t["size"] for t in clusters["clusters"]])
    want = cluster_split_numpy(vb.offsets, index, np.concatenate(clusters["cluster"]), toff, size, shape, spec, cls)
    assert sorted(got) == ["cluster", "clusters", "events"] and len(got["events"]) == len(counts) and toff[-1] > 0
    poff, joff, off = want["piece_offsets"], want["junction_offsets"], vb.offsets
    for i, ev in enumerate(got["events"]):
        assert sorted(ev) == ["event", "junctions", "mark", "pieces", "rows"]
        for name in SPLIT_PIECE:
            w = want["pieces"][name][poff[i]:poff[i + 1]]
            assert ev["pieces"][name].dtype == w.dtype and np.array_equal(ev["pieces"][name], w), (i, name)
        for name in SPLIT_JUNCTION_INT + SPLIT_JUNCTION_REAL:
            w = want["junctions"][name][joff[i]:joff[i + 1]]
            assert ev["junctions"][name].dtype == w.dtype and np.array_equal(_bits(ev["junctions"][name]), _bits(w)), (i, name)
        for col, name in enumerate(SPLIT_ROW):
            assert np.array_equal(ev["rows"][name], want["rows"][toff[i]:toff[i + 1], col]), (i, name)
        assert ev["mark"].dtype == np.uint8 and np.array_equal(ev["mark"], want["mark"][off[i]:off[i + 1]]), i
        assert ev["event"] == dict(zip(SPLIT_EVENT, (int(x) for x in want["events"][i]))), i
        assert got["cluster"][i].dtype == np.int32 and np.array_equal(got["cluster"][i], want["split"][off[i]:off[i + 1]]), i
        for name in ("first", "size", "cls"):
            w = want["table"][name][poff[i]:poff[i + 1]]
            assert got["clusters"][i][name].dtype == w.dtype and np.array_equal(got["clusters"][i][name], w), (i, name)
    return want


def test_cluster_split_of_a_voxel_score_result():
    net, vb = _net(), _events()
    net.set_clustering(ClusterSpec(classes=(0, 1, 2), min_size=2))
    r = net.inference_voxel_scores(None, vb, with_labels=False, want=("pred", "cluster"))
    assert sorted(r) == ["cluster", "clusters", "index", "pred"]
    index = np.concatenate(r["index"])
    for spec in (ClusterSplitSpec(2, -0.7, 4), ClusterSplitSpec(1, -0.5, 2, (1, 2), 0), ClusterSplitSpec(3, 1.0, 6, None, 8)):
        got = net.cluster_split(None, vb, {"cluster": r["cluster"], "clusters": r["clusters"]}, spec)
        want = _same_split(got, vb, index, r, DIMS[:-1], spec)
    assert want["piece_offsets"][-1] >= want["piece_offsets"].size - 1
    # the pieces are themselves a clustering: the object records of the pieces
    spec = ClusterSplitSpec(2, -0.7, 4)
    got = net.cluster_split(None, vb, r, spec)
    pieces = net.cluster_features(None, vb, None, got)
    ptoff = np.concatenate([[0], np.cumsum([t["first"].size for t in got["clusters"]])])
    want = cluster_features_numpy(vb.offsets, index, vb.value, np.concatenate(got["cluster"]), ptoff, DIMS[:-1])
    for i, ev in enumerate(pieces):
        for name in ("n", "charge", "end_lo", "end_hi", "axis", "length"):
            assert np.array_equal(_bits(ev[name].astype(np.float64)), _bits(want[name][ptoff[i]:ptoff[i + 1]].astype(np.float64))), (i, name)
    # too small an estimate (here: one piece, no junction): the call runs once more from the true counts, with the same result
    net._cluster_split_estimate = (0, 1, 0, 0)
    again = net.cluster_split(None, vb, r, spec)
    _same_split(again, vb, index, r, DIMS[:-1], spec)


def _same_arrays(a, b, path="result"):
    """Two results of a voxel-score call are equal byte for byte, key by key."""
    assert type(a) is type(b), path
    if isinstance(a, dict):
        assert sorted(a) == sorted(b), path
        for k in a:
            _same_arrays(a[k], b[k], "%s[%r]" % (path, k))
    elif isinstance(a, (list, tuple)):
        assert len(a) == len(b), path
        for i, (x, y) in enumerate(zip(a, b)):
            _same_arrays(x, y, "%s[%d]" % (path, i))
    elif isinstance(a, np.ndarray):
        assert a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes(), path
    else:
        assert a == b or (a != a and b != b), path


def _everything_on(net):
    from uresnet_amd.clusters import ClusterChainSpec, ClusterConeSpec, ClusterGraphSpec, ClusterProfileSpec, ClusterVertexSpec
    net.set_cluster_features(True)
    net.set_cluster_profiles(ClusterProfileSpec())
    net.set_cluster_vertices(ClusterVertexSpec())
    net.set_cluster_chains(ClusterChainSpec(12, 0.7, 2))
    net.set_cluster_cones(ClusterConeSpec())
    net.set_cluster_graph(ClusterGraphSpec(1))


def test_inference_voxel_scores_with_the_split():
    from uresnet_amd.clusters import ClusterChainSpec, ClusterConeSpec, ClusterGraphSpec, ClusterProfileSpec, ClusterVertexSpec
    net, vb = _net(), _events()
    net.set_clustering(ClusterSpec(classes=(0, 1, 2), min_size=2))
    _everything_on(net)
    want = ("pred", "cluster")
    before = net.inference_voxel_scores(None, vb, with_labels=False, want=want)
    assert "split" not in before                                                        # the setter never called: the parent's keys
    spec = ClusterSplitSpec(2, -0.7, 4)
    net.set_cluster_split(spec)
    r = net.inference_voxel_scores(None, vb, with_labels=False, want=want)
    assert sorted(r) == sorted(list(before) + ["split"])
    index = np.concatenate(r["index"])
    _same_split(r["split"], vb, index, r, DIMS[:-1], spec)
    _same_arrays({k: v for k, v in r.items() if k != "split"}, before)                  # downstream off: every other record as it was
    _same_arrays(net.cluster_split(None, vb, r, spec), r["split"])                      # the stand-alone call: the same records
    # downstream: the records describe the pieces, and equal the stand-alone calls made on the pieces
    net.set_cluster_split(spec, downstream=True)
    d = net.inference_voxel_scores(None, vb, with_labels=False, want=want)
    assert sorted(d) == sorted(r)
    _same_arrays({k: d[k] for k in ("index", "pred", "cluster", "clusters", "split")}, {k: r[k] for k in ("index", "pred", "cluster", "clusters", "split")})
    pieces = d["split"]
    _same_arrays(d["objects"], net.cluster_features(None, vb, None, pieces))
    _same_arrays(d["profiles"], net.cluster_profiles(None, vb, None, pieces, ClusterProfileSpec()))
    _same_arrays(d["vertices"], net.cluster_vertices(None, vb, None, pieces, ClusterVertexSpec()))
    _same_arrays(d["chains"], net.cluster_chains(None, vb, None, pieces, ClusterChainSpec(12, 0.7, 2)))
    _same_arrays(d["cones"], net.cluster_cones(None, vb, None, pieces, ClusterConeSpec()))
    _same_arrays(d["graph"], net.cluster_graph(None, vb, pieces, ClusterGraphSpec(1)))
    assert sum(t["first"].size for t in pieces["clusters"]) > sum(t["first"].size for t in d["clusters"])   # something was split
    # off again: byte for byte what it was
    net.set_cluster_split(None)
    _same_arrays(net.inference_voxel_scores(None, vb, with_labels=False, want=want), before)
    assert sorted(net.inference_voxel_scores(None, vb, with_labels=False, want=("pred",))) == ["index", "pred"]


def test_tiled_split_is_in_the_large_shape():
    big, halo = (48, 40, 56), 4                                                       # two tiles per axis
    vb = VoxelBatch.concat([sio.dense_to_voxels(*sio.lartpc_sparse(list(big) + [1], 3, e)) for e in range(2)]).validate()
    net = _net()
    net.set_clustering(ClusterSpec(classes=(0, 1, 2), same_class=True))
    net.set_cluster_features(True)
    before = net.inference_tiled_voxel_scores(None, vb, big, halo=halo, want=("pred", "cluster"))
    spec = ClusterSplitSpec(2, -0.7, 4)
    net.set_cluster_split(spec)
    r = net.inference_tiled_voxel_scores(None, vb, big, halo=halo, want=("pred", "cluster"))
    assert sorted(r) == sorted(list(before) + ["split"])
    _same_arrays({k: v for k, v in r.items() if k != "split"}, before)
    _same_split(r["split"], vb, np.concatenate(r["index"]), r, big, spec)
    net.set_cluster_split(spec, downstream=True)
    d = net.inference_tiled_voxel_scores(None, vb, big, halo=halo, want=("pred", "cluster"))
    _same_arrays(d["split"], r["split"])
    _same_arrays(d["objects"], net.cluster_features(None, vb, None, d["split"], shape=big))


# ---- driver --------------------------------------------------------------------------------------------------------------------
def _drive(tmp_path, tag, extra):
    import io
    from contextlib import redirect_stdout
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


def test_driver_writes_one_row_per_junction(tmp_path):
    """The CSV parses back to the returned records; the driver's own records are byte for byte those of a run without the key."""
    from uresnet_amd.ssnet import split_csv_header
    csv = tmp_path / "split.csv"
    plain, ref = _drive(tmp_path, "plain", "")
    with_key, res = _drive(tmp_path, "split", "ANA_SPLIT '%s'\nSPLIT_RADIUS 2\nSPLIT_KINK_COS -0.9\nSPLIT_MIN_SIZE 4\nSPLIT_GROW 2\n" % csv)
    assert with_key == plain                                                          # the records do not change
    lines = csv.read_text().split("\n")
    assert lines[0] + "\n" == split_csv_header() and lines[-1] == ""
    names = lines[0].split(",")
    rows = [dict(zip(names, line.split(","))) for line in lines[1:-1]]
    at = 0
    for e, (ev, ev0) in enumerate(zip(res["voxels"], ref["voxels"])):
        assert sorted(ev) == sorted(list(ev0) + ["split"])
        got = ev["split"]["junctions"]
        assert got["row"].size == ev["split"]["event"]["junctions"] and ev["split"]["split"].shape == ev["cluster"].shape
        for k in range(got["row"].size):
            row = rows[at]
            at += 1
            assert (int(row["entry"]), int(row["junction"])) == (int(res["entries"][e]), k)
            for name in SPLIT_JUNCTION_INT:
                assert int(row[name]) == int(got[name][k]), (e, k, name)
            for name in SPLIT_JUNCTION_REAL:
                assert float(row[name]) == got[name][k], (e, k, name)
    assert at == len(rows) > 0
