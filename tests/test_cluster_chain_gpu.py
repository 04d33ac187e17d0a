"""Cluster chains on the device (csrc/cluster_chain.hip) against the numpy statement (uresnet_amd.clusters.cluster_chains_numpy).
Every comparison is np.array_equal on every column, fp64 columns by their bits.  Op level: the lists, the object tables and every
output sit between 0xFF guard bands (tests/_guard.py); each case runs four times -- scratch filled 0xFF, filled 0x00, as the second
call left it (the same arguments again), and in the plain form (URSN_CLCHAIN_WAVE=0: one thread per end point) -- and all four must
give the statement's bits; everything at or beyond a count or a cap must be left untouched.  The object tables the call reads are
the statement's own (cluster_features_numpy, laid out as the device lays them out; tests/test_cluster_features_gpu.py holds the
device to those bits).  The lists are those of tests/_chain_cases.py, whose coverage tests/test_cluster_chain_host.py asserts.  Net
level: set_cluster_chains with the voxel-score calls, cluster_chains, and the driver's ANA_CHAINS file."""
import ctypes
import io
import os
from contextlib import redirect_stdout

import numpy as np
import pytest

import _chain_cases as cases
import _far_corner as far
from _guard import Guarded
from uresnet_amd import _lib, uresnet
from uresnet_amd import synthetic_io as sio
from uresnet_amd.clusters import (CHAIN_EVENT, CHAIN_INT, CHAIN_REAL, JOIN_INT, JOIN_REAL, ClusterChainSpec, ClusterSpec,
                                  cluster_chains_numpy, cluster_features_numpy)
from uresnet_amd.ssnet import VoxelBatch, chains_csv_header

pytestmark = pytest.mark.gpu

FI, FR = _lib.CLFEAT_I, _lib.CLFEAT_R
CI, CR, JI, JR, EV = _lib.CLCHAIN_CI, _lib.CLCHAIN_CR, _lib.CLCHAIN_JI, _lib.CLCHAIN_JR, _lib.CLCHAIN_EV
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


def _check(lib, off, index, value, cluster, toff, shape, spec, cls=None, cap_rows=None, cap_chains=None, cap_joins=None, tamper=None,
           status=0):
    """Runs the case four times on guarded operands and compares every call with the statement; returns the statement.  With
    ``tamper(index, cluster, itab, rtab, cls)`` the device's copies are changed in place first: the four calls must then all report
    exactly ``status`` and agree with each other byte for byte; returns the first call's row_join."""
    import torch
    off, toff = np.asarray(off, np.int64), np.asarray(toff, np.int64)
    index, cluster = np.asarray(index, np.int64), np.asarray(cluster, np.int64)
    want = cluster_chains_numpy(off, index, value, cluster, toff, shape, spec, cls)
    wci = np.stack([want["chains"][k] for k in CHAIN_INT], 1)
    wcr = np.stack([want["chains"][k] for k in CHAIN_REAL], 1)
    wji = np.stack([want["joins"][k] for k in JOIN_INT], 1)
    wjr = np.stack([want["joins"][k] for k in JOIN_REAL], 1)
    fit, frt = _feature_tables(want["objects"])
    n, M, K = off.size - 1, int(off[-1]), int(toff[-1])
    C, J = int(want["chain_offsets"][-1]), int(want["join_offsets"][-1])
    index, cluster, cls = index.astype(np.int32), cluster.astype(np.int32), None if cls is None else np.array(cls, np.uint8)
    first = None
    if tamper is not None:
        tamper(index, cluster, fit, frt, cls)
    cap_rows = K if cap_rows is None else cap_rows
    cap_chains = (C if tamper is None else K) if cap_chains is None else cap_chains       # a skipped row can split a chain
    cap_joins = (J if tamper is None else K) if cap_joins is None else cap_joins
    rows, chains, joins = min(cap_rows, K), min(cap_chains, C), min(cap_joins, J)
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
    need = int(lib.ursn_cluster_chains_scratch_bytes(n, M))
    assert need >= 8 and need % 8 == 0
    scratch = Guarded(need, torch.uint8)
    d = _lib.ursn_cluster_chain_desc()
    d.ndim, d.n, d.m_total, d.max_gap = len(shape), n, M, spec.max_gap
    for i, s in enumerate(shape):
        d.spatial[i] = s
    d.offsets, d.index, d.cluster, d.table_offsets = g_off.ptr, g_idx.ptr, g_cl.ptr, g_toff.ptr
    d.itab, d.rtab, d.feat_cap = g_it.ptr, g_rt.ptr, K
    d.cls = None if g_cls is None else g_cls.ptr
    d.min_cos, d.min_size, d.class_mask, d.same_class = spec.min_cos, spec.min_size, spec.class_mask(), int(spec.same_class)
    for k, (fill, wave) in enumerate(ROUTES):
        what = "call %d" % k
        if fill is not None:
            scratch.fill(fill)
        merged, coff, joff = Guarded(max(M, 1), torch.int32), Guarded(n + 1, torch.int64), Guarded(n + 1, torch.int64)
        t_first, t_size, t_cls = (Guarded(max(cap_chains, 1), dt) for dt in (torch.int32, torch.int32, torch.uint8))
        ci, cr = Guarded((max(cap_chains, 1), CI), torch.int64), Guarded((max(cap_chains, 1), CR), torch.float64)
        ji, jr = Guarded((max(cap_joins, 1), JI), torch.int64), Guarded((max(cap_joins, 1), JR), torch.float64)
        rc, rj, rn = Guarded(max(cap_rows, 1), torch.int32), Guarded((max(cap_rows, 1), 2), torch.int32), \
            Guarded((max(cap_rows, 1), 2), torch.int32)
        ev, status_out = Guarded((n, EV), torch.int64), Guarded(1, torch.int32)
        o = _lib.ursn_cluster_chain_out()
        o.merged, o.chain_offsets, o.first, o.size, o.cls = merged.ptr, coff.ptr, t_first.ptr, t_size.ptr, t_cls.ptr
        o.chain_itab, o.chain_rtab, o.cap_chains = ci.ptr, cr.ptr, cap_chains
        o.join_offsets, o.join_itab, o.join_rtab, o.cap_joins = joff.ptr, ji.ptr, jr.ptr, cap_joins
        o.row_chain, o.row_join, o.row_candidates, o.cap_rows = rc.ptr, rj.ptr, rn.ptr, cap_rows
        o.event, o.status = ev.ptr, status_out.ptr
        if not wave:
            os.environ["URSN_CLCHAIN_WAVE"] = "0"
        try:
            _lib.check(lib.ursn_cluster_chains(ctypes.byref(d), ctypes.byref(o), ctypes.c_void_p(scratch.ptr), need, None))
        finally:
            os.environ.pop("URSN_CLCHAIN_WAVE", None)
        torch.cuda.synchronize()
        named = [("merged", merged), ("chain_offsets", coff), ("join_offsets", joff), ("first", t_first), ("size", t_size),
                 ("table cls", t_cls), ("chain_itab", ci), ("chain_rtab", cr), ("join_itab", ji), ("join_rtab", jr), ("row_chain", rc),
                 ("row_join", rj), ("row_candidates", rn), ("event", ev), ("status", status_out), ("offsets", g_off),
                 ("table_offsets", g_toff), ("index", g_idx), ("cluster", g_cl), ("itab", g_it), ("rtab", g_rt), ("scratch", scratch)] + \
            ([] if g_cls is None else [("cls", g_cls)])
        for name, g in named:
            g.check(name)
        code = int(status_out.numpy()[0])
        if tamper is not None:
            assert code == status, (what, code)
            outs = [g.numpy().copy() for _, g in named[:14]]
            first = outs if first is None else first
            for (name, _), a, b in zip(named, outs, first):
                assert np.array_equal(a.view(np.uint8), b.view(np.uint8)), (what, name, "differs from the first call")
            continue
        assert code == 0, (what, code)
        assert np.array_equal(coff.numpy(), want["chain_offsets"]) and np.array_equal(joff.numpy(), want["join_offsets"]), what
        assert np.array_equal(ev.numpy(), want["events"]), (what, "events")                  # the true counts, whatever the caps are
        if M:
            assert np.array_equal(merged.numpy(), want["merged"]), (what, "merged")
        else:
            assert _untouched(merged.numpy()), (what, "merged of an empty list")
        gci, gcr, gji, gjr = ci.numpy(), cr.numpy(), ji.numpy(), jr.numpy()
        for c, name in enumerate(CHAIN_INT):
            assert np.array_equal(gci[:chains, c], wci[:chains, c]), (what, "chain", name)
        for c, name in enumerate(CHAIN_REAL):
            assert np.array_equal(_bits(gcr[:chains, c]), _bits(wcr[:chains, c])), (what, "chain", name)
        for c, name in enumerate(JOIN_INT):
            assert np.array_equal(gji[:joins, c], wji[:joins, c]), (what, "join", name)
        for c, name in enumerate(JOIN_REAL):
            assert np.array_equal(_bits(gjr[:joins, c]), _bits(wjr[:joins, c])), (what, "join", name)
        for name, g in (("first", t_first), ("size", t_size), ("cls", t_cls)):
            assert g.numpy().dtype == want["table"][name].dtype and np.array_equal(g.numpy()[:chains], want["table"][name][:chains]), (what, name)
            assert _untouched(g.numpy()[chains:]), (what, name, "beyond the count or cap")
        assert np.array_equal(rc.numpy()[:rows], want["row_chain"][:rows]), (what, "row_chain")
        assert np.array_equal(rj.numpy()[:rows], want["row_join"][:rows]), (what, "row_join")
        assert np.array_equal(rn.numpy()[:rows], want["row_candidates"][:rows]), (what, "row_candidates")
        assert _untouched(gci[chains:]) and _untouched(gcr[chains:]), (what, "chains at or beyond the count or cap were written")
        assert _untouched(gji[joins:]) and _untouched(gjr[joins:]), (what, "joins at or beyond the count or cap were written")
        assert _untouched(rc.numpy()[rows:]) and _untouched(rj.numpy()[rows:]) and _untouched(rn.numpy()[rows:]), (what, "rows beyond")
    return want if tamper is None else first[11]


@pytest.mark.parametrize("min_size", [1, 3])
@pytest.mark.parametrize("same_class", [True, False], ids=["by_class", "any_class"])
@pytest.mark.parametrize("min_cos", [0.7, 0.9])
@pytest.mark.parametrize("max_gap", [3, 6, 12, 31])
@pytest.mark.parametrize("name", ["angles", "long", "flat"])
def test_knocked_out_events(lib, name, max_gap, min_cos, same_class, min_size):
    shape = cases.FIXTURES[name][0]
    off, index, value, cluster, toff, tcls = cases.fixture(name)[:6]
    want = _check(lib, off, index, value, cluster, toff, shape, ClusterChainSpec(max_gap, min_cos, min_size, None, same_class), cls=tcls)
    assert want["chain_offsets"][-1] > 0                 # what the lists cover is asserted in tests/test_cluster_chain_host.py


@pytest.mark.parametrize("name", sorted(cases.FIXTURES))
def test_the_fixtures_at_their_own_settings(lib, name):
    """The settings tests/test_cluster_chain_host.py asserts the coverage of (min_size 2, both values of same_class), without cls and
    with classes."""
    shape, _, _, gap, min_cos = cases.FIXTURES[name]
    off, index, value, cluster, toff, tcls = cases.fixture(name)[:6]
    for same in (True, False):
        _check(lib, off, index, value, cluster, toff, shape, ClusterChainSpec(gap, min_cos, 2, None, same), cls=tcls)
    bare = _check(lib, off, index, None, cluster, toff, shape, ClusterChainSpec(gap, min_cos, 2, None, False), cls=None)
    assert (bare["chains"]["mask_flags"] & 0xFFFFFFFF == 0).all() and (bare["chains"]["charge"] == 0).all() and (bare["table"]["cls"] == 0).all()
    only = _check(lib, off, index, value, cluster, toff, shape, ClusterChainSpec(gap, min_cos, 2, (2,), True), cls=tcls)
    assert (only["row_join"][tcls != 2] == -1).all() and (only["chains"]["charge"] != 0).any()


def test_the_ring_and_the_line(lib):
    (off, index, ids, toff, tcls), _ = cases.ring()
    want = _check(lib, off, index, None, ids, toff, (16, 32, 32), ClusterChainSpec(4, 0.7, 3, None, False), cls=tcls)
    assert want["chains"]["rows"].tolist() == [8] and want["chains"]["joins"].tolist() == [8] and want["chains"]["mask_flags"][0] >> 32 == 1
    (off, index, ids, toff, tcls), _ = cases.line()
    want = _check(lib, off, index, None, ids, toff, (8, 8, 64), ClusterChainSpec(4, 0.9, 3), cls=tcls)
    assert want["chains"]["rows"].tolist() == [10, 3] and want["chains"]["path"].tolist() == [56.0, 14.0]


def test_every_voxel_its_own_cluster(lib):
    """end_lo == end_hi everywhere: nothing is eligible, no end point exists, every row is a chain of its own."""
    shape = (12, 10)
    index = np.arange(0, 120, 2)
    ids, toff = np.concatenate([np.arange(20), np.arange(40)]), [0, 20, 60]
    want = _check(lib, [0, 20, 60], index, None, ids, toff, shape, ClusterChainSpec(31, 0.0, 1, None, False))
    assert want["chain_offsets"].tolist() == toff and want["join_offsets"].tolist() == [0, 0, 0] and (want["row_candidates"] == 0).all()
    assert np.array_equal(want["merged"], ids) and (want["chains"]["path"] == 0.0).all()
    shape = (16, 16, 16)
    index = np.arange(0, 4096, 3)
    _check(lib, [0, index.size], index, None, np.arange(index.size), [0, index.size], shape, ClusterChainSpec(2, 0.5, 1, None, False))


def test_the_lattice_crosses_every_one_step_threshold(lib):
    """2,100 rows = 4,200 end points in a list of 66,300 entries: the three one-workgroup scans of 1,024 threads (1,036 tiles, 2,100
    rows, 4,200 keys) take chunks of two, three and five, the search's 1,024 workgroups of four end points sweep twice, and with
    max_gap 2 the chain walk's 32 workgroups of 64 chains sweep twice; with max_gap 3 every line is a chain of ten rows.
    tests/test_cluster_chain_host.py derives these numbers from the source."""
    shape, index, ids, rows = cases.lattice()
    want = _check(lib, [0, index.size], index, None, ids, [0, rows], shape, ClusterChainSpec(3, 0.9, 3, None, False))
    assert want["events"].tolist() == [[210, 1890, 210, 0]] and (want["chains"]["rows"] == 10).all()
    assert (want["chains"]["path"] == 47.0).all() and (want["row_candidates"] <= 1).all()      # 10 * 2 + 9 * 3
    want = _check(lib, [0, index.size], index, None, ids, [0, rows], shape, ClusterChainSpec(2, 0.9, 3, None, False))
    assert want["events"].tolist() == [[2100, 0, 0, 0]]


def test_caps(lib):
    shape, _, _, gap, min_cos = cases.FIXTURES["long"]
    off, index, value, cluster, toff, tcls = cases.fixture("long")[:6]
    spec = ClusterChainSpec(gap, min_cos, 2)
    want = cluster_chains_numpy(off, index, value, cluster, toff, shape, spec, tcls)
    K, C, J = int(toff[-1]), int(want["chain_offsets"][-1]), int(want["join_offsets"][-1])
    assert J >= 4 and C >= 4
    for cap_rows in (K + 3, K // 2, 0):
        _check(lib, off, index, value, cluster, toff, shape, spec, cls=tcls, cap_rows=cap_rows)
    for cap_chains in (C + 2, C // 2, 0):
        _check(lib, off, index, value, cluster, toff, shape, spec, cls=tcls, cap_chains=cap_chains)
    for cap_joins in (J + 2, J // 2, 0):
        _check(lib, off, index, value, cluster, toff, shape, spec, cls=tcls, cap_joins=cap_joins)


def test_inconsistent_tables_set_their_status_bit(lib):
    """One inconsistency at a time, each reported as its own bit by all four calls (the bits that the first launch finds reach the
    status word through a later launch, so none is lost to the store that starts the word), and the row is not joined."""
    shape, _, _, gap, min_cos = cases.FIXTURES["long"]
    off, index, value, cluster, toff, tcls = cases.fixture("long")[:6]
    spec = ClusterChainSpec(gap, min_cos, 2)
    want = cluster_chains_numpy(off, index, value, cluster, toff, shape, spec, tcls)
    f = want["objects"]
    joined = np.flatnonzero((want["row_join"][:toff[1]] >= 0).any(axis=1) & (f["n"][:toff[1]] >= 4))
    r0 = int(joined[0])                                                     # a joined row of the first event
    r1 = int([r for r in range(toff[1]) if r != r0][0])
    inner = [int(j) for j in np.flatnonzero(cluster[:off[1]] == r0) if j not in (f["end_lo"][r0], f["end_hi"][r0])][0]
    last = int(off[1] - 1)
    assert cluster[last] >= 0

    def other_row(index, cluster, itab, rtab, cls):
        itab[r0, 25] = f["end_lo"][r1]                                    # end_hi: a member of another row
    def no_member(index, cluster, itab, rtab, cls):
        itab[r0, 0] = 0
    def bad_class(index, cluster, itab, rtab, cls):
        cls[r0] = 32
    def bad_id(index, cluster, itab, rtab, cls):
        cluster[inner] = int(toff[1]) + 3                                 # beyond its event's rows
    def bad_index(index, cluster, itab, rtab, cls):
        index[last] = int(np.prod(shape)) + 5                             # the event's last entry: the list stays sorted
    for tamper, bit, skipped in ((other_row, 32, True), (no_member, 2, True), (bad_class, 16, True), (bad_id, 1, False),
                                 (bad_index, 4, None)):
        rj = _check(lib, off, index, value, cluster, toff, shape, spec, cls=tcls, tamper=tamper, status=bit)
        if skipped is not None:
            assert (rj[r0].tolist() == [-1, -1]) == skipped, (tamper.__name__, rj[r0])


def test_no_entries_and_no_clusters(lib):
    shape = (6, 7, 8)
    z = np.zeros(0, np.int64)
    spec = ClusterChainSpec(same_class=False)
    _check(lib, [0, 0, 0], z, None, z, [0, 0, 0], shape, spec)
    _check(lib, [0, 0], z, None, z, [0, 0], shape, spec, cap_rows=5, cap_chains=4, cap_joins=3)
    want = _check(lib, [0, 4, 6], np.array([1, 5, 9, 200, 3, 4]), None, np.full(6, -1), [0, 0, 0], shape, spec, cap_rows=6, cap_chains=6,
                  cap_joins=6)
    assert want["events"].tolist() == [[0, 0, 0, -1], [0, 0, 0, -1]] and want["merged"].tolist() == [-1] * 6


# ---- the largest legal extents (tests/_far_corner.py) ---------------------------------------------------------------
@pytest.mark.parametrize("shape", far.SHAPES_CAPPED, ids=far.shape_id)
def test_far_corner(lib, shape):
    """The fixtures, the ring and the line against the far faces, at the origin and across index 2^30, at max_gap 31: search windows
    that a far face clips (tests/test_far_corner_host.py asserts that joins are accepted through such windows)."""
    b = far.far_batch("chain", shape).big
    for same_class in (True, False):
        want = _check(lib, b.off, b.index, b.value, b.cluster, b.toff, shape, ClusterChainSpec(31, 0.7, 2, None, same_class), cls=b.tcls)
        assert want["join_offsets"][-1] > 0
        assert all(want["chains"]["hi%d" % a].max() == shape[a] - 1 for a in range(len(shape)))
    _check(lib, b.off, b.index, None, b.cluster, b.toff, shape, ClusterChainSpec(3, 0.9, 3, None, False), cls=None)


@pytest.mark.parametrize("axis", sorted(far.LONG_TRACK))
def test_a_track_across_the_longest_axis(lib, axis):
    """One cluster of 32,768 members from corner to corner: one chain of one row, whose end points have nothing to search."""
    s = far.long_track(far.LONG_TRACK[axis])
    want = _check(lib, s.off, s.index, s.value, s.cluster, s.toff, s.shape, far.WIDEST["chain"], cls=s.tcls)
    assert want["events"][0, :2].tolist() == [1, 0] and want["chains"]["hi%d" % axis].tolist() == [32767]


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


def _same_chains(r, vb, shape, spec, got=None):
    """r['chains'] equals the statement evaluated on r['index'], the batch's values, r['cluster'] and the table's cls."""
    got = r["chains"] if got is None else got
    counts = [t["first"].size for t in r["clusters"]]
    toff = np.concatenate([[0], np.cumsum(counts)])
    cls = np.concatenate([t["cls"] for t in r["clusters"]])
    want = cluster_chains_numpy(vb.offsets, np.concatenate(r["index"]), vb.value, np.concatenate(r["cluster"]), toff, shape, spec, cls)
    assert sorted(got) == ["cluster", "clusters", "events"] and len(got["events"]) == len(counts) and toff[-1] > 0
    coff, joff, off = want["chain_offsets"], want["join_offsets"], vb.offsets
    for i, ev in enumerate(got["events"]):
        assert sorted(ev) == ["chains", "event", "joins", "objects", "row_candidates", "row_chain", "row_join"]
        lo, hi = coff[i], coff[i + 1]
        for name in CHAIN_INT + CHAIN_REAL:
            w = want["chains"][name][lo:hi]
            assert ev["chains"][name].dtype == w.dtype and np.array_equal(_bits(ev["chains"][name]), _bits(w)), (i, name)
        for name in JOIN_INT + JOIN_REAL:
            w = want["joins"][name][joff[i]:joff[i + 1]]
            assert ev["joins"][name].dtype == w.dtype and np.array_equal(_bits(ev["joins"][name]), _bits(w)), (i, name)
        for name in ("row_chain", "row_join", "row_candidates"):
            assert ev[name].dtype == np.int32 and np.array_equal(ev[name], want[name][toff[i]:toff[i + 1]]), (i, name)
        assert ev["event"] == dict(zip(CHAIN_EVENT, (int(x) for x in want["events"][i]))), i
        for name in ("end_lo", "end_hi", "axis", "n"):
            assert np.array_equal(ev["objects"][name], want["objects"][name][toff[i]:toff[i + 1]]), (i, name)
        assert got["cluster"][i].dtype == np.int32 and np.array_equal(got["cluster"][i], want["merged"][off[i]:off[i + 1]]), i
        for name in ("first", "size", "cls"):
            w = want["table"][name][lo:hi]
            assert got["clusters"][i][name].dtype == w.dtype and np.array_equal(got["clusters"][i][name], w), (i, name)
    return want


def test_inference_voxel_scores_with_chains():
    net, vb = _net(), _events()
    net.set_clustering(ClusterSpec(classes=(0, 1, 2), min_size=2))
    before = net.inference_voxel_scores(None, vb, with_labels=False, want=("pred", "cluster"))
    assert sorted(before) == ["cluster", "clusters", "index", "pred"]                 # the setter never called: the parent's keys
    spec = ClusterChainSpec(12, 0.7, 2)
    net.set_cluster_chains(spec)
    r = net.inference_voxel_scores(None, vb, with_labels=False, want=("pred", "cluster"))
    assert sorted(r) == ["chains", "cluster", "clusters", "index", "pred"]            # the object records ran, and are not a key
    assert all(np.array_equal(a, b) for a, b in zip(r["cluster"], before["cluster"]))
    _same_chains(r, vb, DIMS[:-1], spec)
    assert sorted(net.inference_voxel_scores(None, vb, with_labels=False, want=("pred",))) == ["index", "pred"]
    # the stand-alone call on the same lists gives the same records
    again = net.cluster_chains(None, vb, None, {"cluster": r["cluster"], "clusters": r["clusters"]}, spec)
    _same_chains(r, vb, DIMS[:-1], spec, got=again)
    # the result is itself a clustering: the object records of the merged objects
    merged = net.cluster_features(None, vb, None, r["chains"])
    mtoff = np.concatenate([[0], np.cumsum([t["first"].size for t in r["chains"]["clusters"]])])
    want = cluster_features_numpy(vb.offsets, np.concatenate(r["index"]), vb.value, np.concatenate(r["chains"]["cluster"]), mtoff, DIMS[:-1])
    for i, ev in enumerate(merged):
        for name in ("n", "charge", "end_lo", "end_hi", "axis", "length"):
            assert np.array_equal(_bits(ev[name].astype(np.float64)), _bits(want[name][mtoff[i]:mtoff[i + 1]].astype(np.float64))), (i, name)
    other = ClusterChainSpec(31, 0.5, 1, (1, 2), False)
    net.set_cluster_chains(other)
    _same_chains(net.inference_voxel_scores(None, vb, with_labels=False, want=("pred", "cluster")), vb, DIMS[:-1], other)
    net.set_cluster_chains(None)
    assert sorted(net.inference_voxel_scores(None, vb, with_labels=False, want=("pred", "cluster"))) == \
        ["cluster", "clusters", "index", "pred"]


def test_tiled_chains_are_in_the_large_shape():
    big, halo = (48, 40, 56), 4                                                       # two tiles per axis
    vb = VoxelBatch.concat([sio.dense_to_voxels(*sio.lartpc_sparse(list(big) + [1], 3, e)) for e in range(2)]).validate()
    net = _net()
    net.set_clustering(ClusterSpec(classes=(0, 1, 2), same_class=True))
    spec = ClusterChainSpec(12, 0.7, 2)
    net.set_cluster_chains(spec)
    r = net.inference_tiled_voxel_scores(None, vb, big, halo=halo, want=("pred", "cluster"))
    assert "chains" in r and "objects" not in r
    _same_chains(r, vb, big, spec)


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


def test_driver_writes_one_row_per_chain(tmp_path):
    """The CSV parses back to the returned records; the driver's own records are byte for byte those of a run without the key."""
    csv = tmp_path / "chains.csv"
    plain, ref = _drive(tmp_path, "plain", "")
    with_key, res = _drive(tmp_path, "chains", "ANA_CHAINS '%s'\nCHAIN_GAP 12\nCHAIN_MIN_COS 0.7\nCHAIN_MIN_SIZE 2\n" % csv)
    assert with_key == plain                                                          # the records do not change
    lines = csv.read_text().split("\n")
    assert lines[0] + "\n" == chains_csv_header() and lines[-1] == ""
    names = lines[0].split(",")
    rows = [dict(zip(names, line.split(","))) for line in lines[1:-1]]
    at = 0
    for e, (ev, ev0) in enumerate(zip(res["voxels"], ref["voxels"])):
        assert sorted(ev) == sorted(list(ev0) + ["chains"])
        got = ev["chains"]["chains"]
        assert got["rows"].size == ev["chains"]["event"]["chains"] > 0 and ev["chains"]["merged"].shape == ev["cluster"].shape
        for k in range(got["rows"].size):
            row = rows[at]
            at += 1
            assert (int(row["entry"]), int(row["chain"])) == (int(res["entries"][e]), k)
            for name in CHAIN_INT:
                assert int(row[name]) == int(got[name][k]), (e, k, name)
            for name in CHAIN_REAL:
                assert float(row[name]) == got[name][k], (e, k, name)
    assert at == len(rows)
