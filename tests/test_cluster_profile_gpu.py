"""Per-cluster charge profiles on the device (csrc/cluster_profile.hip) against the numpy statement
(uresnet_amd.clusters.cluster_profile_numpy).  Every comparison is np.array_equal on every field, fp64 fields by their bits.  Op
level: the lists, the object tables and every output sit between 0xFF guard bands (tests/_guard.py); each case runs four times --
scratch filled 0xFF, filled 0x00, as the second call left it (the same arguments again), and with one atomic set per entry
(URSN_CLPROF_WAVE=0) -- and all four must give the statement's bits.  The object tables the profile reads are the statement's own
(cluster_features_numpy, laid out as the device lays them out; tests/test_cluster_features_gpu.py holds the device to those bits).
Net level: set_cluster_profiles with the voxel-score calls, cluster_profiles, and the driver's ANA_PROFILES file."""
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
from uresnet_amd.clusters import (PROFILE_BIN_INT, PROFILE_BIN_REAL, PROFILE_ROW_INT, PROFILE_ROW_REAL, ClusterProfileSpec, ClusterSpec,
                                  cluster_numpy, cluster_profile_numpy)
from uresnet_amd.ssnet import VoxelBatch, profiles_csv_header

pytestmark = pytest.mark.gpu

FI, FR = _lib.CLFEAT_I, _lib.CLFEAT_R
BI, BR, RI, RR = _lib.CLPROF_BI, _lib.CLPROF_BR, _lib.CLPROF_RI, _lib.CLPROF_RR
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


def _want_tables(p):
    B, K = p["bins"]["n"].size, p["rows"]["bins"].size
    bi = np.stack([p["bins"][k] for k in PROFILE_BIN_INT], 1) if B else np.zeros((0, BI), np.int64)
    br = np.stack([p["bins"][k] for k in PROFILE_BIN_REAL], 1) if B else np.zeros((0, BR), np.float64)
    ri = np.stack([p["rows"][k] for k in PROFILE_ROW_INT], 1) if K else np.zeros((0, RI), np.int64)
    rr = np.stack([p["rows"][k] for k in PROFILE_ROW_REAL], 1) if K else np.zeros((0, RR), np.float64)
    return bi, br, ri, rr


def _untouched(a):
    return bool((np.ascontiguousarray(a).view(np.uint8) == 0xFF).all())


def _check(lib, off, index, value, cluster, toff, shape, spec, cap_rows=None, bin_cap=None, feat_cap=None):
    """Runs the case four times on guarded operands and compares every call with the statement; returns the statement."""
    import torch
    off, toff = np.asarray(off, np.int64), np.asarray(toff, np.int64)
    index, cluster = np.asarray(index, np.int64), np.asarray(cluster, np.int64)
    value = None if value is None else np.asarray(value, np.float32)
    want = cluster_profile_numpy(off, index, value, cluster, toff, shape, spec)
    wbi, wbr, wri, wrr = _want_tables(want)
    fit, frt = _feature_tables(want["objects"])
    n, M, K = off.size - 1, int(off[-1]), int(toff[-1])
    cap_rows = K if cap_rows is None else cap_rows
    feat_cap = K if feat_cap is None else feat_cap
    rows = min(cap_rows, feat_cap, K, M)
    total = int(want["bin_offsets"][rows])
    bin_cap = total if bin_cap is None else bin_cap
    g_off, g_toff = Guarded(n + 1, torch.int64, off), Guarded(n + 1, torch.int64, toff)
    g_idx, g_cl = Guarded(max(M, 1), torch.int32), Guarded(max(M, 1), torch.int32)
    g_val = None if value is None else Guarded(max(M, 1), torch.float32)
    if M:
        g_idx.set(index.astype(np.int32)), g_cl.set(cluster.astype(np.int32))
        if g_val is not None:
            g_val.set(value)
    g_it, g_rt = Guarded((max(feat_cap, 1), FI), torch.int64), Guarded((max(feat_cap, 1), FR), torch.float64)
    if min(feat_cap, K):
        g_it.tensor[:min(feat_cap, K)].copy_(torch.from_numpy(fit[:feat_cap].copy()))
        g_rt.tensor[:min(feat_cap, K)].copy_(torch.from_numpy(frt[:feat_cap].copy()))
    need = int(lib.ursn_cluster_profile_scratch_bytes(n, M, cap_rows, bin_cap))
    assert need >= 8 and need % 8 == 0
    scratch = Guarded(need, torch.uint8)
    d = _lib.ursn_cluster_prof_desc()
    d.ndim, d.n, d.m_total = len(shape), n, M
    for i, s in enumerate(shape):
        d.spatial[i] = s
    d.offsets, d.index, d.cluster, d.table_offsets = g_off.ptr, g_idx.ptr, g_cl.ptr, g_toff.ptr
    d.value = None if g_val is None else g_val.ptr
    d.itab, d.rtab, d.feat_cap = g_it.ptr, g_rt.ptr, feat_cap
    d.step, d.end_bins, d.max_bins = spec.step, spec.end_bins, spec.max_bins
    for k, (fill, wave) in enumerate(ROUTES):
        what = "call %d" % k
        if fill is not None:
            scratch.fill(fill)
        boff = Guarded(cap_rows + 1, torch.int64)
        bi, br = Guarded((max(bin_cap, 1), BI), torch.int64), Guarded((max(bin_cap, 1), BR), torch.float64)
        ri, rr = Guarded((max(cap_rows, 1), RI), torch.int64), Guarded((max(cap_rows, 1), RR), torch.float64)
        status = Guarded(1, torch.int32)
        o = _lib.ursn_cluster_prof_out()
        o.bin_offsets, o.bin_itab, o.bin_rtab, o.row_itab, o.row_rtab = boff.ptr, bi.ptr, br.ptr, ri.ptr, rr.ptr
        o.cap_rows, o.bin_cap, o.status = cap_rows, bin_cap, status.ptr
        if not wave:
            os.environ["URSN_CLPROF_WAVE"] = "0"
        try:
            _lib.check(lib.ursn_cluster_profile(ctypes.byref(d), ctypes.byref(o), ctypes.c_void_p(scratch.ptr), need, None))
        finally:
            os.environ.pop("URSN_CLPROF_WAVE", None)
        torch.cuda.synchronize()
        named = [("bin_offsets", boff), ("bin_itab", bi), ("bin_rtab", br), ("row_itab", ri), ("row_rtab", rr), ("status", status),
                 ("offsets", g_off), ("table_offsets", g_toff), ("index", g_idx), ("cluster", g_cl), ("itab", g_it), ("rtab", g_rt),
                 ("scratch", scratch)] + ([] if g_val is None else [("value", g_val)])
        for name, g in named:
            g.check(name)
        got_off, code = boff.numpy(), int(status.numpy()[0])
        assert np.array_equal(got_off[:rows + 1], want["bin_offsets"][:rows + 1]), what      # the true counts, whatever bin_cap is
        assert _untouched(got_off[rows + 1:]), (what, "bin_offsets beyond the rows")
        if total > bin_cap:
            assert code == _lib.CLPROF_BIN_OVERFLOW, (what, code)
            assert _untouched(bi.numpy()[bin_cap:]) and _untouched(br.numpy()[bin_cap:]), (what, "bins beyond bin_cap")
            assert _untouched(ri.numpy()[rows:]) and _untouched(rr.numpy()[rows:]), (what, "rows beyond the cap")
            continue
        assert code == 0, (what, code)
        gbi, gbr, gri, grr = bi.numpy(), br.numpy(), ri.numpy(), rr.numpy()
        for c, name in enumerate(PROFILE_BIN_INT):
            assert np.array_equal(gbi[:total, c], wbi[:total, c]), (what, "bin", name)
        for c, name in enumerate(PROFILE_BIN_REAL):
            assert np.array_equal(_bits(gbr[:total, c]), _bits(wbr[:total, c])), (what, "bin", name)
        for c, name in enumerate(PROFILE_ROW_INT):
            assert np.array_equal(gri[:rows, c], wri[:rows, c]), (what, "row", name)
        for c, name in enumerate(PROFILE_ROW_REAL):
            assert np.array_equal(_bits(grr[:rows, c]), _bits(wrr[:rows, c])), (what, "row", name)
        assert _untouched(gbi[total:]) and _untouched(gbr[total:]), (what, "bins at or beyond the total were written")
        assert _untouched(gri[rows:]) and _untouched(grr[rows:]), (what, "rows at or beyond the count or cap were written")
    return want


def _ids(off, index, cls, shape, spec):
    ids, counts = [], []
    for e in range(len(off) - 1):
        c, first, _, _ = cluster_numpy(index[off[e]:off[e + 1]], cls[off[e]:off[e + 1]], shape, spec)
        ids.append(c), counts.append(first.size)
    return np.concatenate(ids) if ids else np.zeros(0, np.int32), np.concatenate([[0], np.cumsum(counts)]).astype(np.int64)


_made = {}


def _case(shape):
    """Four events -- random, empty, random without a cluster (class 0 only), random -- with ids of -1 in the others; values with an
    Inf, a NaN and 2^15.  Made once per shape and shared read-only."""
    if shape not in _made:
        rng = np.random.default_rng(len(shape))
        vox, occ = int(np.prod(shape)), (0.1 if len(shape) == 3 else 0.45)
        lists = [np.flatnonzero(rng.uniform(size=vox) < occ), np.zeros(0, np.int64), np.flatnonzero(rng.uniform(size=vox) < occ / 2),
                 np.flatnonzero(rng.uniform(size=vox) < occ)]
        cls = [rng.integers(0, 3, a.size).astype(np.uint8) for a in lists]
        cls[2][:] = 0
        off = np.concatenate([[0], np.cumsum([a.size for a in lists])])
        index, cls = np.concatenate(lists), np.concatenate(cls)
        cluster, toff = _ids(off, index, cls, shape, ClusterSpec(26 if len(shape) == 3 else 8, (1, 2), False))
        value = rng.uniform(-3.0, 40.0, index.size).astype(np.float32)
        inside = np.flatnonzero(cluster >= 0)
        value[inside[3]], value[inside[40]], value[inside[-2]] = np.float32(np.inf), np.float32(np.nan), np.float32(2.0 ** 15)
        assert toff[1] > 2 and toff[2] == toff[1] == toff[3] and toff[4] > toff[3] and (cluster == -1).sum() > 10
        for a in (off, index, value, cluster, toff):
            a.setflags(write=False)
        _made[shape] = (off, index, value, cluster, toff)
    return _made[shape]


@pytest.mark.parametrize("step", [0.5, 0.7, 1.0, 3.3])
@pytest.mark.parametrize("shape", [(16, 16, 16), (12, 10)], ids=["3d", "2d"])
def test_random_lists(lib, shape, step):
    off, index, value, cluster, toff = _case(shape)
    want = _check(lib, off, index, value, cluster, toff, shape, ClusterProfileSpec(step, 3, 4096))
    assert (want["rows"]["flags"] & 1).sum() >= 1 and (want["rows"]["bins"] > 1).any()


@pytest.mark.parametrize("shape", [(16, 16, 16), (12, 10)], ids=["3d", "2d"])
def test_no_values_end_bins_and_truncation(lib, shape):
    off, index, value, cluster, toff = _case(shape)
    none = _check(lib, off, index, None, cluster, toff, shape, ClusterProfileSpec(1.0, 1, 4096))
    assert (none["bins"]["charge"] == 0).all() and (none["rows"]["flags"] == 0).all() and (none["rows"]["direction"] == 0).all()
    cut = _check(lib, off, index, value, cluster, toff, shape, ClusterProfileSpec(0.5, 16, 3))
    assert (cut["rows"]["flags"] & 2).any() and cut["rows"]["bins"].max() == 3


def test_every_voxel_its_own_cluster(lib):
    shape = (12, 10)
    index = np.arange(0, 120, 2)
    want = _check(lib, [0, 20, 60], index, np.linspace(0.5, 30.0, 60).astype(np.float32), np.concatenate([np.arange(20), np.arange(40)]),
                  [0, 20, 60], shape, ClusterProfileSpec(0.7, 2, 8))
    assert (want["rows"]["bins"] == 1).all() and (want["rows"]["h"] == 0).all() and (want["bins"]["n"] == 1).all()


def test_a_workgroup_with_more_keys_than_its_table(lib):
    """The first 512 entries (one workgroup's two rounds) are 512 one-voxel clusters: 512 distinct bins for a 256-slot table, so half
    of them take the direct route; behind them one long track shares its bins among many lanes."""
    shape = (16, 16, 16)
    singles = np.arange(512)
    track = np.ravel_multi_index(np.array([(8 + a, b, c) for a in range(2) for b in range(16) for c in range(16)]).T, shape)
    index = np.concatenate([singles, track])
    cluster = np.concatenate([np.arange(512), np.full(track.size, 512)])
    value = np.random.default_rng(5).uniform(0.0, 9.0, index.size).astype(np.float32)
    want = _check(lib, [0, index.size], index, value, cluster, [0, 513], shape, ClusterProfileSpec(1.0, 3, 4096))
    assert (want["rows"]["bins"][:512] == 1).all() and want["rows"]["bins"][512] >= 16 and want["bins"]["n"].max() >= 16


def test_more_rows_than_scan_threads(lib):
    """2,500 rows of ragged length: the one-workgroup scan of 1,024 threads takes chunks of three rows."""
    shape = (64, 8, 40)
    rng = np.random.default_rng(8)
    pts, ids = [], []
    for r in range(2500):
        a, b, c0 = r // 40, (r // 5) % 8, (r % 5) * 8
        for c in range(c0, c0 + int(rng.integers(1, 8))):      # 1 .. 7 voxels, then at least one free
            pts.append((a, b, c)), ids.append(r)
    index = np.ravel_multi_index(np.array(pts).T, shape)
    assert (np.diff(index) > 0).all()
    want = _check(lib, [0, index.size], index, rng.uniform(0.0, 5.0, index.size).astype(np.float32), ids, [0, 2500], shape,
                  ClusterProfileSpec(1.0, 2, 4096))
    assert sorted(set(want["rows"]["bins"])) == [1, 2, 3, 4, 5, 6, 7]


def test_caps(lib):
    """Fewer rows than clusters, fewer object records than rows, and a bin table one short of the total."""
    shape = (16, 16, 16)
    off, index, value, cluster, toff = _case(shape)
    spec = ClusterProfileSpec(1.0, 3, 4096)
    K = int(toff[-1])
    for cap_rows in (K + 3, K // 2, 1, 0):
        _check(lib, off, index, value, cluster, toff, shape, spec, cap_rows=cap_rows)
    _check(lib, off, index, value, cluster, toff, shape, spec, feat_cap=K // 3)
    total = int(cluster_profile_numpy(off, index, value, cluster, toff, shape, spec)["bin_offsets"][-1])
    _check(lib, off, index, value, cluster, toff, shape, spec, bin_cap=total + 5)
    _check(lib, off, index, value, cluster, toff, shape, spec, bin_cap=total - 1)        # overflow: offsets and status only
    _check(lib, off, index, value, cluster, toff, shape, spec, bin_cap=0)


def test_no_entries_and_no_clusters(lib):
    shape = (6, 7, 8)
    z = np.zeros(0, np.int64)
    spec = ClusterProfileSpec()
    _check(lib, [0, 0, 0], z, z.astype(np.float32), z, [0, 0, 0], shape, spec)
    _check(lib, [0, 0], z, None, z, [0, 0], shape, spec, cap_rows=5, bin_cap=7, feat_cap=5)
    _check(lib, [0, 4, 6], np.array([1, 5, 9, 200, 3, 4]), np.ones(6, np.float32), np.full(6, -1), [0, 0, 0], shape, spec, cap_rows=6,
           bin_cap=6, feat_cap=6)


# ---- the largest legal extents (tests/_far_corner.py) ---------------------------------------------------------------
@pytest.mark.parametrize("shape", far.SHAPES_CAPPED, ids=far.shape_id)
def test_far_corner(lib, shape):
    """The random lists against the far faces, at the origin and across index 2^30 (tests/test_far_corner_host.py asserts what the
    batch reaches): the bin centroids are positions in the large shape."""
    b = far.far_batch("random", shape).big
    want = _check(lib, b.off, b.index, b.value, b.cluster, b.toff, shape, far.WIDEST["profile"])
    top = max(want["bins"]["c%d" % a].max() / (shape[a] - 1) for a in range(len(shape)))
    assert top > 0.999 and want["rows"]["bins"].max() >= 8
    cluster, toff, _ = far.clustered("random", shape, 6 if len(shape) == 3 else 4, False)
    _check(lib, b.off, b.index, None, cluster, toff, shape, ClusterProfileSpec(1.0, 3, 4096))


@pytest.mark.parametrize("axis", sorted(far.LONG_TRACK))
def test_a_track_across_the_longest_axis(lib, axis):
    """One cluster of 32,768 members from corner to corner, length 32768.98 along axis 0: at step 0.5 that is 65,538 segments, cut
    to the record's stated maximum of 65,536 with bit 1 of the flags.  The track that drifts by 150 only has a length in
    [32767.5, 32768): exactly 65,536 segments and no flag; max_bins 65535 cuts that one too."""
    s = far.long_track(far.LONG_TRACK[axis])
    want = _check(lib, s.off, s.index, s.value, s.cluster, s.toff, s.shape, ClusterProfileSpec(0.5, 16, 65536))
    assert want["rows"]["bins"].tolist() == [65536] and want["rows"]["flags"].tolist() == [2]
    if axis == 0:
        s = far.long_track(far.LONG_TRACK[axis], 150)
        want = _check(lib, s.off, s.index, s.value, s.cluster, s.toff, s.shape, ClusterProfileSpec(0.5, 16, 65536))
        assert 32767.5 <= want["objects"]["length"][0] < 32768 and want["rows"]["bins"].tolist() == [65536] and want["rows"]["flags"].tolist() == [0]
        cut = _check(lib, s.off, s.index, s.value, s.cluster, s.toff, s.shape, ClusterProfileSpec(0.5, 16, 65535))
        assert cut["rows"]["bins"].tolist() == [65535] and cut["rows"]["flags"].tolist() == [2]


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


def _same_profiles(r, vb, shape, spec):
    """r['profiles'] equals the statement evaluated on r['index'], the batch's values and r['cluster']."""
    counts = [t["first"].size for t in r["clusters"]]
    toff = np.concatenate([[0], np.cumsum(counts)])
    want = cluster_profile_numpy(vb.offsets, np.concatenate(r["index"]), vb.value, np.concatenate(r["cluster"]), toff, shape, spec)
    assert len(r["profiles"]) == len(counts) and toff[-1] > 0
    boff = want["bin_offsets"]
    for i, got in enumerate(r["profiles"]):
        assert sorted(got) == ["bin_offsets", "bins", "objects", "rows"]
        lo, hi = boff[toff[i]], boff[toff[i + 1]]
        assert np.array_equal(got["bin_offsets"], boff[toff[i]:toff[i + 1] + 1] - lo), i
        assert sorted(got["rows"]) == sorted(PROFILE_ROW_INT + PROFILE_ROW_REAL)
        assert sorted(got["bins"]) == sorted(PROFILE_BIN_INT + PROFILE_BIN_REAL)
        for name in PROFILE_ROW_INT + PROFILE_ROW_REAL:
            w = want["rows"][name][toff[i]:toff[i + 1]]
            assert got["rows"][name].dtype == w.dtype and np.array_equal(_bits(got["rows"][name]), _bits(w)), (i, name)
        for name in PROFILE_BIN_INT + PROFILE_BIN_REAL:
            w = want["bins"][name][lo:hi]
            assert got["bins"][name].dtype == w.dtype and np.array_equal(_bits(got["bins"][name]), _bits(w)), (i, name)
        for name in ("length", "axis", "m", "n"):
            assert np.array_equal(got["objects"][name], want["objects"][name][toff[i]:toff[i + 1]]), (i, name)


def test_inference_voxel_scores_with_profiles():
    net, vb = _net(), _events()
    net.set_clustering(ClusterSpec(classes=(0, 1, 2), min_size=2))
    before = net.inference_voxel_scores(None, vb, with_labels=False, want=("pred", "cluster"))
    assert sorted(before) == ["cluster", "clusters", "index", "pred"]                 # the setter never called: the parent's keys
    spec = ClusterProfileSpec(1.0, 3, 4096)
    net.set_cluster_profiles(spec)
    r = net.inference_voxel_scores(None, vb, with_labels=False, want=("pred", "cluster"))
    assert sorted(r) == ["cluster", "clusters", "index", "pred", "profiles"]          # the object records ran, and are not a key
    assert all(np.array_equal(a, b) for a, b in zip(r["cluster"], before["cluster"]))
    _same_profiles(r, vb, DIMS[:-1], spec)
    assert sorted(net.inference_voxel_scores(None, vb, with_labels=False, want=("pred",))) == ["index", "pred"]
    net.set_cluster_features(True)
    both = net.inference_voxel_scores(None, vb, with_labels=False, want=("pred", "cluster"))
    assert sorted(both) == ["cluster", "clusters", "index", "objects", "pred", "profiles"]
    _same_profiles(both, vb, DIMS[:-1], spec)
    net.set_cluster_features(False)
    # the stand-alone call on the same lists gives the same records
    again = net.cluster_profiles(None, vb, None, {"cluster": r["cluster"], "clusters": r["clusters"]}, spec)
    _same_profiles(dict(r, profiles=again), vb, DIMS[:-1], spec)
    # a bin table that is too small is made again through the exact path
    net._profile_bin_cap = lambda M, s: 3
    _same_profiles(net.inference_voxel_scores(None, vb, with_labels=False, want=("pred", "cluster")), vb, DIMS[:-1], spec)
    del net._profile_bin_cap
    net.set_cluster_profiles(None)
    assert sorted(net.inference_voxel_scores(None, vb, with_labels=False, want=("pred", "cluster"))) == \
        ["cluster", "clusters", "index", "pred"]


def test_tiled_profiles_are_in_the_large_shape():
    big, halo = (48, 40, 56), 4                                                       # two tiles per axis
    vb = VoxelBatch.concat([sio.dense_to_voxels(*sio.lartpc_sparse(list(big) + [1], 3, e)) for e in range(2)]).validate()
    net = _net()
    net.set_clustering(ClusterSpec(classes=(0, 1, 2), same_class=False))
    spec = ClusterProfileSpec(2.0, 2, 4096)
    net.set_cluster_profiles(spec)
    r = net.inference_tiled_voxel_scores(None, vb, big, halo=halo, want=("pred", "cluster"))
    assert "profiles" in r and "objects" not in r
    _same_profiles(r, vb, big, spec)


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


def test_driver_writes_one_row_per_cluster(tmp_path):
    """The CSV parses back to the returned records; the driver's own records are byte for byte those of a run without the key."""
    csv = tmp_path / "profiles.csv"
    plain, ref = _drive(tmp_path, "plain", "")
    with_key, res = _drive(tmp_path, "profiles", "ANA_PROFILES '%s'\nPROFILE_STEP 2.0\nPROFILE_END_BINS 2\n" % csv)
    assert with_key == plain                                                          # the records do not change
    lines = csv.read_text().split("\n")
    assert lines[0] + "\n" == profiles_csv_header() and lines[-1] == ""
    names = lines[0].split(",")
    rows = [dict(zip(names, line.split(","))) for line in lines[1:-1]]
    at = 0
    for e, (ev, ev0) in enumerate(zip(res["voxels"], ref["voxels"])):
        assert sorted(ev) == sorted(list(ev0) + ["profiles"])
        got = ev["profiles"]["rows"]
        assert got["bins"].size == ev["clusters"]["first"].size > 0
        for k in range(got["bins"].size):
            row = rows[at]
            at += 1
            assert (int(row["entry"]), int(row["cluster"])) == (int(res["entries"][e]), k)
            for name in PROFILE_ROW_INT:
                assert int(row[name]) == int(got[name][k]), (e, k, name)
            for name in PROFILE_ROW_REAL:
                assert float(row[name]) == got[name][k], (e, k, name)
            assert int(row["h"]) == min(2, int(row["bins"]) // 2)
    assert at == len(rows)
