"""Cluster cones on the device (csrc/cluster_cone.hip) against the numpy statement (uresnet_amd.clusters.cluster_cones_numpy).
Every comparison is np.array_equal on every column, fp64 columns by their bits.  Op level: the lists, the object tables and every
output sit between 0xFF guard bands (tests/_guard.py); each case runs four times -- scratch filled 0xFF, filled 0x00, as the second
call left it (the same arguments again), and in the plain form (URSN_CLCONE_WAVE=0: one thread per child row) -- and all four must
give the statement's bits; everything at or beyond a count or a cap must be left untouched.  The object tables the call reads are
the statement's own (cluster_features_numpy, laid out as the device lays them out; tests/test_cluster_features_gpu.py holds the
device to those bits).  The lists are those of tests/_cone_cases.py, whose coverage tests/test_cluster_cone_host.py asserts.  Net
level: set_cluster_cones with the voxel-score calls, cluster_cones (on clusters and on chains), and the driver's ANA_CONES file."""
import ctypes
import io
import os
from contextlib import redirect_stdout

import numpy as np
import pytest

import _chain_cases as chain_cases
import _cone_cases as cases
import _far_corner as far
from _guard import Guarded
from uresnet_amd import _lib, uresnet
from uresnet_amd import synthetic_io as sio
from uresnet_amd.clusters import (CONE_EVENT, CONE_INT, CONE_REAL, LINK_INT, LINK_REAL, ClusterChainSpec, ClusterConeSpec, ClusterSpec,
                                  cluster_cones_numpy, cluster_features_numpy)
from uresnet_amd.ssnet import VoxelBatch, cones_csv_header

pytestmark = pytest.mark.gpu

FI, FR = _lib.CLFEAT_I, _lib.CLFEAT_R
SI, SR, LI, LR, EV = _lib.CLCONE_SI, _lib.CLCONE_SR, _lib.CLCONE_LI, _lib.CLCONE_LR, _lib.CLCONE_EV
FEAT_INT = (("n", 0, 1), ("charge", 1, 1), ("s", 2, 3), ("lo", 5, 3), ("hi", 8, 3), ("m", 11, 3), ("d", 14, 3), ("dd", 17, 6),
            ("flags", 23, 1), ("end_lo", 24, 1), ("end_hi", 25, 1))
FEAT_REAL = (("centroid", 0, 3), ("cov", 3, 6), ("eval", 9, 3), ("axis", 12, 3), ("length", 15, 1), ("t_lo", 16, 1), ("t_hi", 17, 1))
ROUTES = ((0xFF, True), (0x00, True), (None, True), (0xFF, False))
ROW_NAMES = ("row_shower", "row_parent", "row_candidates", "row_children", "row_depth")


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


def _check(lib, off, index, value, cluster, toff, shape, spec, cls=None, cap_rows=None, cap_showers=None, cap_links=None, tamper=None,
           status=0):
    """Runs the case four times on guarded operands and compares every call with the statement; returns the statement.  With
    ``tamper(index, cluster, itab, rtab, cls)`` the device's copies are changed in place first: the four calls must then all report
    exactly ``status`` and agree with each other byte for byte; returns the first call's row_parent."""
    import torch
    off, toff = np.asarray(off, np.int64), np.asarray(toff, np.int64)
    index, cluster = np.asarray(index, np.int64), np.asarray(cluster, np.int64)
    want = cluster_cones_numpy(off, index, value, cluster, toff, shape, spec, cls)
    wsi = np.stack([want["showers"][k] for k in CONE_INT], 1)
    wsr = np.stack([want["showers"][k] for k in CONE_REAL], 1)
    wli = np.stack([want["links"][k] for k in LINK_INT], 1)
    wlr = np.stack([want["links"][k] for k in LINK_REAL], 1)
    fit, frt = _feature_tables(want["objects"])
    n, M, K = off.size - 1, int(off[-1]), int(toff[-1])
    S, L = int(want["shower_offsets"][-1]), int(want["link_offsets"][-1])
    index, cluster, cls = index.astype(np.int32), cluster.astype(np.int32), None if cls is None else np.array(cls, np.uint8)
    first = None
    if tamper is not None:
        tamper(index, cluster, fit, frt, cls)
    cap_rows = K if cap_rows is None else cap_rows
    cap_showers = (S if tamper is None else K) if cap_showers is None else cap_showers       # a skipped row can split a shower
    cap_links = (L if tamper is None else K) if cap_links is None else cap_links
    rows, showers, links = min(cap_rows, K), min(cap_showers, S), min(cap_links, L)
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
    need = int(lib.ursn_cluster_cones_scratch_bytes(n, M))
    assert need >= 8 and need % 8 == 0
    scratch = Guarded(need, torch.uint8)
    d = _lib.ursn_cluster_cone_desc()
    d.ndim, d.n, d.m_total, d.reach = len(shape), n, M, spec.reach
    for i, s in enumerate(shape):
        d.spatial[i] = s
    d.offsets, d.index, d.cluster, d.table_offsets = g_off.ptr, g_idx.ptr, g_cl.ptr, g_toff.ptr
    d.itab, d.rtab, d.feat_cap = g_it.ptr, g_rt.ptr, K
    d.cls = None if g_cls is None else g_cls.ptr
    d.min_cos, d.min_size, d.class_mask, d.same_class = spec.min_cos, spec.min_size, spec.class_mask(), int(spec.same_class)
    d.seed_size = spec.seed_size
    for k, (fill, wave) in enumerate(ROUTES):
        what = "call %d" % k
        if fill is not None:
            scratch.fill(fill)
        merged, soff, loff = Guarded(max(M, 1), torch.int32), Guarded(n + 1, torch.int64), Guarded(n + 1, torch.int64)
        t_first, t_size, t_cls = (Guarded(max(cap_showers, 1), dt) for dt in (torch.int32, torch.int32, torch.uint8))
        si, sr = Guarded((max(cap_showers, 1), SI), torch.int64), Guarded((max(cap_showers, 1), SR), torch.float64)
        li, lr = Guarded((max(cap_links, 1), LI), torch.int64), Guarded((max(cap_links, 1), LR), torch.float64)
        cr = max(cap_rows, 1)
        rs, rp, rn, rk, rd = Guarded(cr, torch.int32), Guarded(cr, torch.int32), Guarded(cr, torch.int32), Guarded((cr, 2), torch.int32), \
            Guarded(cr, torch.int32)
        ev, status_out = Guarded((n, EV), torch.int64), Guarded(1, torch.int32)
        o = _lib.ursn_cluster_cone_out()
        o.merged, o.shower_offsets, o.first, o.size, o.cls = merged.ptr, soff.ptr, t_first.ptr, t_size.ptr, t_cls.ptr
        o.shower_itab, o.shower_rtab, o.cap_showers = si.ptr, sr.ptr, cap_showers
        o.link_offsets, o.link_itab, o.link_rtab, o.cap_links = loff.ptr, li.ptr, lr.ptr, cap_links
        o.row_shower, o.row_parent, o.row_candidates, o.row_children, o.row_depth, o.cap_rows = rs.ptr, rp.ptr, rn.ptr, rk.ptr, rd.ptr, \
            cap_rows
        o.event, o.status = ev.ptr, status_out.ptr
        if not wave:
            os.environ["URSN_CLCONE_WAVE"] = "0"
        try:
            _lib.check(lib.ursn_cluster_cones(ctypes.byref(d), ctypes.byref(o), ctypes.c_void_p(scratch.ptr), need, None))
        finally:
            os.environ.pop("URSN_CLCONE_WAVE", None)
        torch.cuda.synchronize()
        named = [("merged", merged), ("shower_offsets", soff), ("link_offsets", loff), ("first", t_first), ("size", t_size),
                 ("table cls", t_cls), ("shower_itab", si), ("shower_rtab", sr), ("link_itab", li), ("link_rtab", lr), ("row_shower", rs),
                 ("row_parent", rp), ("row_candidates", rn), ("row_children", rk), ("row_depth", rd), ("event", ev),
                 ("status", status_out), ("offsets", g_off), ("table_offsets", g_toff), ("index", g_idx), ("cluster", g_cl),
                 ("itab", g_it), ("rtab", g_rt), ("scratch", scratch)] + ([] if g_cls is None else [("cls", g_cls)])
        for name, g in named:
            g.check(name)
        code = int(status_out.numpy()[0])
        if tamper is not None:
            assert code == status, (what, code)
            outs = [g.numpy().copy() for _, g in named[:16]]
            first = outs if first is None else first
            for (name, _), a, b in zip(named, outs, first):
                assert np.array_equal(a.view(np.uint8), b.view(np.uint8)), (what, name, "differs from the first call")
            continue
        assert code == 0, (what, code)
        assert np.array_equal(soff.numpy(), want["shower_offsets"]) and np.array_equal(loff.numpy(), want["link_offsets"]), what
        assert np.array_equal(ev.numpy(), want["events"]), (what, "events")                  # the true counts, whatever the caps are
        if M:
            assert np.array_equal(merged.numpy(), want["merged"]), (what, "merged")
        else:
            assert _untouched(merged.numpy()), (what, "merged of an empty list")
        gsi, gsr, gli, glr = si.numpy(), sr.numpy(), li.numpy(), lr.numpy()
        for c, name in enumerate(CONE_INT):
            assert np.array_equal(gsi[:showers, c], wsi[:showers, c]), (what, "shower", name)
        for c, name in enumerate(CONE_REAL):
            assert np.array_equal(_bits(gsr[:showers, c]), _bits(wsr[:showers, c])), (what, "shower", name)
        for c, name in enumerate(LINK_INT):
            assert np.array_equal(gli[:links, c], wli[:links, c]), (what, "link", name)
        for c, name in enumerate(LINK_REAL):
            assert np.array_equal(_bits(glr[:links, c]), _bits(wlr[:links, c])), (what, "link", name)
        for name, g in (("first", t_first), ("size", t_size), ("cls", t_cls)):
            assert g.numpy().dtype == want["table"][name].dtype and np.array_equal(g.numpy()[:showers], want["table"][name][:showers]), (what, name)
            assert _untouched(g.numpy()[showers:]), (what, name, "beyond the count or cap")
        for name, g in zip(ROW_NAMES, (rs, rp, rn, rk, rd)):
            assert np.array_equal(g.numpy()[:rows], want[name][:rows]), (what, name)
            assert _untouched(g.numpy()[rows:]), (what, name, "rows beyond")
        assert _untouched(gsi[showers:]) and _untouched(gsr[showers:]), (what, "showers at or beyond the count or cap were written")
        assert _untouched(gli[links:]) and _untouched(glr[links:]), (what, "links at or beyond the count or cap were written")
    return want if tamper is None else first[11]


@pytest.mark.parametrize("name", sorted(cases.SCENES))
def test_the_named_scenes(lib, name):
    """Every hand-built scene at its own settings, without cls where the settings allow it, and at a second setting that moves a
    decision (tests/test_cluster_cone_host.py holds the statement's answers)."""
    shape, (off, index, ids, toff, tcls), _, spec = cases.named(name)
    value = (np.arange(index.size) % 7 + 0.25).astype(np.float32)
    want = _check(lib, off, index, value, ids, toff, shape, spec, cls=tcls)
    other = {"misaligned": cases.MISALIGNED_LOOSE, "boundary": ClusterConeSpec(13, 0.6, 8, 1), "tree": ClusterConeSpec(24, 0.8, 5, 1),
             "classes": ClusterConeSpec(12, 0.8, 8, 1, None, False), "far": ClusterConeSpec(16, 0.8, 8, 1)}.get(name)
    if other is not None:
        moved = _check(lib, off, index, value, ids, toff, shape, other, cls=tcls)
        assert not np.array_equal(moved["row_parent"], want["row_parent"])
        want = want if want["link_offsets"][-1] else moved
    assert want["link_offsets"][-1] >= 1 and (want["showers"]["charge"] != 0).all()
    free = ClusterConeSpec(spec.reach, spec.min_cos, spec.seed_size, spec.min_size, None, False)
    bare = _check(lib, off, index, None, ids, toff, shape, free, cls=None)
    assert (bare["showers"]["mask_flags"] & 0xFFFFFFFF == 0).all() and (bare["showers"]["charge"] == 0).all() and (bare["table"]["cls"] == 0).all()


def test_the_far_scene_at_every_reach(lib):
    """The child at (100, 8, 8) accepts apexes 20 planes below and 17, 80 above and 80 below: reach 16 sees none, 48 two, 127 four
    (the wave's four trips over the planes)."""
    shape, (off, index, ids, toff, tcls), at, _ = cases.named("far")
    child = int(ids[at(0, (100, 8, 8))])
    for reach, count in ((16, 0), (19, 1), (48, 2), (64, 2), (80, 4), (127, 4)):
        want = _check(lib, off, index, None, ids, toff, shape, ClusterConeSpec(reach, 0.8, 8, 1), cls=tcls)
        assert want["row_candidates"][child] == count, (reach, want["row_candidates"])


@pytest.mark.parametrize("same_class", [True, False], ids=["by_class", "any_class"])
@pytest.mark.parametrize("reach", [3, 12, 31, 48])
@pytest.mark.parametrize("name", ["angles", "flat"])
def test_knocked_out_events(lib, name, reach, same_class):
    """The chain tests' toy events (tracks and shower blobs with slabs knocked out): many rows of every size, three classes, values."""
    shape = chain_cases.FIXTURES[name][0]
    off, index, value, cluster, toff, tcls = chain_cases.fixture(name)[:6]
    want = _check(lib, off, index, value, cluster, toff, shape, ClusterConeSpec(reach, 0.7, 4, 1, None, same_class), cls=tcls)
    assert want["shower_offsets"][-1] > 0 and (reach < 12 or want["link_offsets"][-1] > 0)


def test_the_toy_showers(lib):
    off, index, cluster, toff, tcls = cases.toys()[:5]
    want = _check(lib, off, index, None, cluster, toff, cases.TOY_SHAPE, cases.TOY_SPEC, cls=tcls)
    assert (want["events"][:, 2] >= 2).all() and want["showers"]["depth"].max() >= 1
    _check(lib, off, index, None, cluster, toff, cases.TOY_SHAPE, ClusterConeSpec(127, 0.5, 3, 1, None, False), cls=tcls)   # deeper trees


def test_every_voxel_its_own_cluster(lib):
    """end_lo == end_hi everywhere: nothing is a parent, no apex exists, every row is a shower of its own."""
    shape = (12, 10)
    index = np.arange(0, 120, 2)
    ids, toff = np.concatenate([np.arange(20), np.arange(40)]), [0, 20, 60]
    want = _check(lib, [0, 20, 60], index, None, ids, toff, shape, ClusterConeSpec(127, 0.5, 2, 1, None, False))
    assert want["shower_offsets"].tolist() == toff and want["link_offsets"].tolist() == [0, 0, 0] and (want["row_candidates"] == 0).all()
    assert np.array_equal(want["merged"], ids) and (want["showers"]["primary_fraction"] == 1.0).all()


def test_the_lattice_crosses_every_one_step_threshold(lib):
    """4,200 rows (2,100 stems = 4,200 apexes, 2,100 links) in a list of 68,400 entries: the one-workgroup scans of 1,024 threads
    take chunks of two (1,069 tiles) and five (rows), and the search's 1,024 workgroups of four child rows sweep twice.
    tests/test_cluster_cone_host.py derives these numbers from the source."""
    shape, index, ids, rows = cases.lattice()
    want = _check(lib, [0, index.size], index, None, ids, [0, rows], shape, cases.LATTICE_SPEC)
    assert want["events"].tolist() == [[2100, 2100, 2100, 0]] and (want["showers"]["rows"] == 2).all()
    want = _check(lib, [0, index.size], index, None, ids, [0, rows], shape, ClusterConeSpec(3, 0.8, 3, 1, None, False))
    assert want["events"].tolist() == [[4200, 0, 0, 0]]


def test_caps(lib):
    shape, (off, index, ids, toff, tcls), _, spec = cases.named("sides")
    want = cluster_cones_numpy(off, index, None, ids, toff, shape, spec, tcls)
    K, S, L = int(toff[-1]), int(want["shower_offsets"][-1]), int(want["link_offsets"][-1])
    assert L >= 4 and S >= 4
    for cap_rows in (K + 3, K // 2, 0):
        _check(lib, off, index, None, ids, toff, shape, spec, cls=tcls, cap_rows=cap_rows)
    for cap_showers in (S + 2, S // 2, 0):
        _check(lib, off, index, None, ids, toff, shape, spec, cls=tcls, cap_showers=cap_showers)
    for cap_links in (L + 2, L // 2, 0):
        _check(lib, off, index, None, ids, toff, shape, spec, cls=tcls, cap_links=cap_links)


def test_inconsistent_tables_set_their_status_bit(lib):
    """One inconsistency at a time, each reported as its own bit by all four calls (the bits that the first launch finds reach the
    status word through a later launch, so none is lost to the store that starts the word), and the row takes no part."""
    shape, (off, index, ids, toff, tcls), at, spec = cases.named("tree")
    want = cluster_cones_numpy(off, index, None, ids, toff, shape, spec, tcls)
    f = want["objects"]
    r0, r1 = int(ids[at(0, (20, 10, 24))]), int(ids[at(0, (20, 10, 10))])       # the fragment of 4: a child and a parent; the primary
    assert want["row_parent"][r0] >= 0 and want["row_children"][r0].sum() == 1
    inner, last = at(0, (20, 10, 25)), int(off[1] - 1)
    assert inner not in (f["end_lo"][r0], f["end_hi"][r0]) and ids[last] >= 0

    def other_row(index, cluster, itab, rtab, cls):
        itab[r0, 25] = f["end_lo"][r1]                                    # end_hi: a member of another row
    def bad_anchor(index, cluster, itab, rtab, cls):
        itab[r0, 13] = shape[2]                                           # the anchor: outside the volume
    def no_member(index, cluster, itab, rtab, cls):
        itab[r0, 0] = 0
    def bad_class(index, cluster, itab, rtab, cls):
        cls[r0] = 32
    def bad_id(index, cluster, itab, rtab, cls):
        cluster[inner] = int(toff[1]) + 3                                 # beyond its event's rows
    def bad_index(index, cluster, itab, rtab, cls):
        index[last] = int(np.prod(shape)) + 5                             # the event's last entry: the list stays sorted
    for tamper, bit, skipped in ((other_row, 32, True), (bad_anchor, 32, True), (no_member, 2, True), (bad_class, 16, True),
                                 (bad_id, 1, False), (bad_index, 4, None)):
        rp = _check(lib, off, index, None, ids, toff, shape, spec, cls=tcls, tamper=tamper, status=bit)
        if skipped is not None:
            assert (rp[r0] == -1) == skipped, (tamper.__name__, rp)


def test_no_entries_and_no_clusters(lib):
    shape = (6, 7, 8)
    z = np.zeros(0, np.int64)
    spec = ClusterConeSpec(same_class=False)
    _check(lib, [0, 0, 0], z, None, z, [0, 0, 0], shape, spec)
    _check(lib, [0, 0], z, None, z, [0, 0], shape, spec, cap_rows=5, cap_showers=4, cap_links=3)
    want = _check(lib, [0, 4, 6], np.array([1, 5, 9, 200, 3, 4]), None, np.full(6, -1), [0, 0, 0], shape, spec, cap_rows=6, cap_showers=6,
                  cap_links=6)
    assert want["events"].tolist() == [[0, 0, 0, -1], [0, 0, 0, -1]] and want["merged"].tolist() == [-1] * 6


# ---- the largest legal extents (tests/_far_corner.py) ---------------------------------------------------------------
@pytest.mark.parametrize("shape", far.SHAPES_CAPPED, ids=far.shape_id)
def test_far_corner(lib, shape):
    """The scenes and the toy showers against the far faces, at the origin and across index 2^30, at reach 127: search windows that
    a far face clips (tests/test_far_corner_host.py asserts that links are accepted through such windows)."""
    b = far.far_batch("cone", shape).big
    for same_class in (True, False):
        want = _check(lib, b.off, b.index, b.value, b.cluster, b.toff, shape, ClusterConeSpec(127, 0.7, 8, 1, None, same_class), cls=b.tcls)
        assert want["link_offsets"][-1] > 0
        assert all(want["showers"]["hi%d" % a].max() == shape[a] - 1 for a in range(len(shape)))
    _check(lib, b.off, b.index, None, b.cluster, b.toff, shape, ClusterConeSpec(12, 0.8, 4, 1, None, False), cls=None)


@pytest.mark.parametrize("axis", sorted(far.LONG_TRACK))
def test_a_track_across_the_longest_axis(lib, axis):
    """One cluster of 32,768 members from corner to corner: a primary without a child, whose two apexes are the two corners."""
    s = far.long_track(far.LONG_TRACK[axis])
    want = _check(lib, s.off, s.index, s.value, s.cluster, s.toff, s.shape, far.WIDEST["cone"], cls=s.tcls)
    assert want["events"][0, :2].tolist() == [1, 0] and want["showers"]["hi%d" % axis].tolist() == [32767]


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


def _same_cones(clustering, index, vb, shape, spec, got):
    """``got`` equals the statement evaluated on the lists, the batch's values and the clustering's ids and table cls."""
    counts = [t["first"].size for t in clustering["clusters"]]
    toff = np.concatenate([[0], np.cumsum(counts)])
    cls = np.concatenate([t["cls"] for t in clustering["clusters"]])
    want = cluster_cones_numpy(vb.offsets, np.concatenate(index), vb.value, np.concatenate(clustering["cluster"]), toff, shape, spec, cls)
    assert sorted(got) == ["cluster", "clusters", "events"] and len(got["events"]) == len(counts) and toff[-1] > 0
    soff, loff, off = want["shower_offsets"], want["link_offsets"], vb.offsets
    for i, ev in enumerate(got["events"]):
        assert sorted(ev) == sorted(("event", "links", "objects", "showers") + ROW_NAMES)
        lo, hi = soff[i], soff[i + 1]
        for name in CONE_INT + CONE_REAL:
            w = want["showers"][name][lo:hi]
            assert ev["showers"][name].dtype == w.dtype and np.array_equal(_bits(ev["showers"][name]), _bits(w)), (i, name)
        for name in LINK_INT + LINK_REAL:
            w = want["links"][name][loff[i]:loff[i + 1]]
            assert ev["links"][name].dtype == w.dtype and np.array_equal(_bits(ev["links"][name]), _bits(w)), (i, name)
        for name in ROW_NAMES:
            assert ev[name].dtype == np.int32 and np.array_equal(ev[name], want[name][toff[i]:toff[i + 1]]), (i, name)
        assert ev["event"] == dict(zip(CONE_EVENT, (int(x) for x in want["events"][i]))), i
        for name in ("end_lo", "end_hi", "axis", "n", "m"):
            assert np.array_equal(ev["objects"][name], want["objects"][name][toff[i]:toff[i + 1]]), (i, name)
        assert got["cluster"][i].dtype == np.int32 and np.array_equal(got["cluster"][i], want["merged"][off[i]:off[i + 1]]), i
        for name in ("first", "size", "cls"):
            w = want["table"][name][lo:hi]
            assert got["clusters"][i][name].dtype == w.dtype and np.array_equal(got["clusters"][i][name], w), (i, name)
    return want


def test_inference_voxel_scores_with_cones():
    net, vb = _net(), _events()
    net.set_clustering(ClusterSpec(classes=(0, 1, 2), min_size=2))
    before = net.inference_voxel_scores(None, vb, with_labels=False, want=("pred", "cluster"))
    assert sorted(before) == ["cluster", "clusters", "index", "pred"]                 # the setter never called: the parent's keys
    spec = ClusterConeSpec(24, 0.6, 4, 1)
    net.set_cluster_cones(spec)
    r = net.inference_voxel_scores(None, vb, with_labels=False, want=("pred", "cluster"))
    assert sorted(r) == ["cluster", "clusters", "cones", "index", "pred"]             # the object records ran, and are not a key
    assert all(np.array_equal(a, b) for a, b in zip(r["cluster"], before["cluster"]))
    _same_cones(r, r["index"], vb, DIMS[:-1], spec, r["cones"])
    assert sorted(net.inference_voxel_scores(None, vb, with_labels=False, want=("pred",))) == ["index", "pred"]
    # the stand-alone call on the same lists gives the same records
    again = net.cluster_cones(None, vb, None, {"cluster": r["cluster"], "clusters": r["clusters"]}, spec)
    _same_cones(r, r["index"], vb, DIMS[:-1], spec, again)
    # the result is itself a clustering: the object records of the showers
    merged = net.cluster_features(None, vb, None, r["cones"])
    mtoff = np.concatenate([[0], np.cumsum([t["first"].size for t in r["cones"]["clusters"]])])
    want = cluster_features_numpy(vb.offsets, np.concatenate(r["index"]), vb.value, np.concatenate(r["cones"]["cluster"]), mtoff, DIMS[:-1])
    for i, ev in enumerate(merged):
        for name in ("n", "charge", "end_lo", "end_hi", "axis", "length"):
            assert np.array_equal(_bits(ev[name].astype(np.float64)), _bits(want[name][mtoff[i]:mtoff[i + 1]].astype(np.float64))), (i, name)
    # cones on chains: the dict cluster_chains returns is a legal clusters argument; both setters at once
    net.set_cluster_chains(ClusterChainSpec(12, 0.7, 2))
    both = net.inference_voxel_scores(None, vb, with_labels=False, want=("pred", "cluster"))
    assert sorted(both) == ["chains", "cluster", "clusters", "cones", "index", "pred"]
    _same_cones(both, both["index"], vb, DIMS[:-1], spec, both["cones"])
    on_chains = net.cluster_cones(None, vb, None, both["chains"], spec)
    _same_cones(both["chains"], both["index"], vb, DIMS[:-1], spec, on_chains)
    net.set_cluster_chains(None)
    other = ClusterConeSpec(127, 0.5, 2, 1, (1, 2), False)
    net.set_cluster_cones(other)
    again = net.inference_voxel_scores(None, vb, with_labels=False, want=("pred", "cluster"))
    _same_cones(again, again["index"], vb, DIMS[:-1], other, again["cones"])
    net.set_cluster_cones(None)
    assert sorted(net.inference_voxel_scores(None, vb, with_labels=False, want=("pred", "cluster"))) == \
        ["cluster", "clusters", "index", "pred"]


def test_tiled_cones_are_in_the_large_shape():
    big, halo = (48, 40, 56), 4                                                       # two tiles per axis
    vb = VoxelBatch.concat([sio.dense_to_voxels(*sio.lartpc_sparse(list(big) + [1], 3, e)) for e in range(2)]).validate()
    net = _net()
    net.set_clustering(ClusterSpec(classes=(0, 1, 2), same_class=True))
    spec = ClusterConeSpec(40, 0.6, 4, 1)
    net.set_cluster_cones(spec)
    r = net.inference_tiled_voxel_scores(None, vb, big, halo=halo, want=("pred", "cluster"))
    assert "cones" in r and "objects" not in r
    _same_cones(r, r["index"], vb, big, spec, r["cones"])


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


def test_driver_writes_one_row_per_shower(tmp_path):
    """The CSV parses back to the returned records; the driver's own records are byte for byte those of a run without the key."""
    csv = tmp_path / "cones.csv"
    plain, ref = _drive(tmp_path, "plain", "")
    with_key, res = _drive(tmp_path, "cones", "ANA_CONES '%s'\nCONE_REACH 24\nCONE_MIN_COS 0.6\nCONE_SEED_SIZE 4\n" % csv)
    assert with_key == plain                                                          # the records do not change
    lines = csv.read_text().split("\n")
    assert lines[0] + "\n" == cones_csv_header() and lines[-1] == ""
    names = lines[0].split(",")
    rows = [dict(zip(names, line.split(","))) for line in lines[1:-1]]
    at = 0
    for e, (ev, ev0) in enumerate(zip(res["voxels"], ref["voxels"])):
        assert sorted(ev) == sorted(list(ev0) + ["cones"])
        got = ev["cones"]["showers"]
        assert got["rows"].size == ev["cones"]["event"]["showers"] > 0 and ev["cones"]["merged"].shape == ev["cluster"].shape
        for k in range(got["rows"].size):
            row = rows[at]
            at += 1
            assert (int(row["entry"]), int(row["shower"])) == (int(res["entries"][e]), k)
            for name in CONE_INT:
                assert int(row[name]) == int(got[name][k]), (e, k, name)
            for name in CONE_REAL:
                assert float(row[name]) == got[name][k], (e, k, name)
    assert at == len(rows)
