"""Per-cluster object records on the device (csrc/cluster_features.hip) against the numpy statement
(uresnet_amd.clusters.cluster_features_numpy).  Every comparison is np.array_equal on every field, fp64 and fp32 fields by their
bits.  Op level: the lists and both tables sit between 0xFF guard bands (tests/_guard.py); each case runs four times -- scratch
filled 0xFF, filled 0x00, as the second call left it (the same arguments again), and with one atomic per entry instead of one per
row of a workgroup (URSN_CLFEAT_WAVE=0) -- and all four must give the statement's bits with status 0.  Net level: set_cluster_features with
the voxel-score calls, cluster_features, and the driver's ANA_OBJECTS file."""
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
from uresnet_amd.clusters import ClusterSpec, cluster_features_numpy, cluster_numpy
from uresnet_amd.ssnet import VoxelBatch, objects_csv_header

pytestmark = pytest.mark.gpu

I, R = _lib.CLFEAT_I, _lib.CLFEAT_R
INT_FIELDS = (("n", 0, 1), ("charge", 1, 1), ("s", 2, 3), ("lo", 5, 3), ("hi", 8, 3), ("m", 11, 3), ("d", 14, 3), ("dd", 17, 6),
              ("flags", 23, 1), ("end_lo", 24, 1), ("end_hi", 25, 1))
REAL_FIELDS = (("centroid", 0, 3), ("cov", 3, 6), ("eval", 9, 3), ("axis", 12, 3), ("length", 15, 1), ("t_lo", 16, 1), ("t_hi", 17, 1))


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view({4: np.uint32, 8: np.uint64}[a.dtype.itemsize])


def _tables(f):
    """The statement's dict as the two device tables (t_lo / t_hi widened, as the device stores them)."""
    K = f["n"].shape[0]
    it, rt = np.zeros((K, I), np.int64), np.zeros((K, R), np.float64)
    for name, at, w in INT_FIELDS:
        it[:, at:at + w] = f[name].reshape(K, w)
    for name, at, w in REAL_FIELDS:
        rt[:, at:at + w] = f[name].astype(np.float64).reshape(K, w)
    return it, rt


ROUTES = ((0xFF, True), (0x00, True), (None, True), (0xFF, False))


def _run(lib, off, index, value, cluster, toff, shape, cap, routes=ROUTES):
    """Four calls of ursn_cluster_features on guarded operands; returns per call (itab, rtab, status) as host arrays (`routes`:
    the scratch fill and the URSN_CLFEAT_WAVE route of each call; tests/test_long_lists_gpu.py runs two)."""
    import torch
    n, M = off.size - 1, int(off[-1])
    g_off, g_toff = Guarded(n + 1, torch.int64, off), Guarded(n + 1, torch.int64, toff)
    g_idx, g_cl = Guarded(max(M, 1), torch.int32), Guarded(max(M, 1), torch.int32)
    g_val = None if value is None else Guarded(max(M, 1), torch.float32)
    if M:
        g_idx.set(index.astype(np.int32)), g_cl.set(cluster.astype(np.int32))
        if g_val is not None:
            g_val.set(value)
    need = int(lib.ursn_cluster_features_scratch_bytes(n, M, cap))
    assert need >= 8 and need % 8 == 0
    scratch = Guarded(need, torch.uint8)
    d = _lib.ursn_cluster_feat_desc()
    d.ndim, d.n, d.m_total = len(shape), n, M
    for i, s in enumerate(shape):
        d.spatial[i] = s
    d.offsets, d.index, d.cluster, d.table_offsets = g_off.ptr, g_idx.ptr, g_cl.ptr, g_toff.ptr
    d.value = None if g_val is None else g_val.ptr
    results = []
    for fill, wave in routes:
        if fill is not None:
            scratch.fill(fill)
        itab, rtab = Guarded((max(cap, 1), I), torch.int64), Guarded((max(cap, 1), R), torch.float64)
        status = Guarded(1, torch.int32)
        o = _lib.ursn_cluster_feat_out()
        o.itab, o.rtab, o.cap, o.status = itab.ptr, rtab.ptr, cap, status.ptr
        if not wave:
            os.environ["URSN_CLFEAT_WAVE"] = "0"
        try:
            _lib.check(lib.ursn_cluster_features(ctypes.byref(d), ctypes.byref(o), ctypes.c_void_p(scratch.ptr), need, None))
        finally:
            os.environ.pop("URSN_CLFEAT_WAVE", None)
        torch.cuda.synchronize()
        named = [("itab", itab), ("rtab", rtab), ("status", status), ("offsets", g_off), ("table_offsets", g_toff), ("index", g_idx),
                 ("cluster", g_cl), ("scratch", scratch)] + ([] if g_val is None else [("value", g_val)])
        for name, g in named:
            g.check(name)
        results.append((itab.numpy(), _bits(rtab.numpy()), int(status.numpy()[0])))
    return results


def _check(lib, off, index, value, cluster, toff, shape, cap=None):
    """Runs the case and compares all four calls with the statement; returns the statement."""
    off, toff = np.asarray(off, np.int64), np.asarray(toff, np.int64)
    index, cluster = np.asarray(index, np.int64), np.asarray(cluster, np.int64)
    value = None if value is None else np.asarray(value, np.float32)
    want = cluster_features_numpy(off, index, value, cluster, toff, shape)
    wi, wr = _tables(want)
    total = int(toff[-1])
    cap = total if cap is None else cap
    rows = min(cap, total)
    for k, (it, rt, status) in enumerate(_run(lib, off, index, value, cluster, toff, shape, cap)):
        what = "call %d" % k
        assert status == 0, what
        for name, at, w in INT_FIELDS:
            assert np.array_equal(it[:rows, at:at + w], wi[:rows, at:at + w]), (what, name)
        for name, at, w in REAL_FIELDS:
            assert np.array_equal(rt[:rows, at:at + w], _bits(wr[:rows, at:at + w])), (what, name)
        assert (it[rows:].view(np.uint8) == 0xFF).all() and (rt[rows:].view(np.uint8) == 0xFF).all(), \
            (what, "rows at or beyond the count or cap were written")
    return want


def _ids(off, index, cls, shape, spec):
    """cluster_numpy per event: the flat ids and the table offsets."""
    ids, counts = [], []
    for e in range(len(off) - 1):
        c, first, _, _ = cluster_numpy(index[off[e]:off[e + 1]], cls[off[e]:off[e + 1]], shape, spec)
        ids.append(c), counts.append(first.size)
    return np.concatenate(ids) if ids else np.zeros(0, np.int32), np.concatenate([[0], np.cumsum(counts)]).astype(np.int64)


def _event(shape, parts, holes=()):
    """Sorted index list of the union of `parts` (class 1) and `holes` (class 0: they get id -1), with the classes."""
    pts = [p for part in parts for p in part]
    idx = np.ravel_multi_index(np.array(pts + list(holes), np.int64).T, shape)
    cls = np.array([1] * len(pts) + [0] * len(holes), np.uint8)
    order = np.argsort(idx)
    assert np.unique(idx).size == idx.size
    return idx[order], cls[order]


def _values(rng, m):
    return rng.uniform(-3.0, 40.0, m).astype(np.float32)


def test_hand_made_shapes_3d(lib):
    shape = (16, 12, 20)
    first = [[(0, 0, 0)],                                                     # a single voxel
             [(2, 2, c) for c in range(3, 12)],                               # lines along each axis: two zero eigenvalues
             [(4, b, 1) for b in range(1, 10)],
             [(a, 10, 18) for a in range(0, 9)],
             [(8 + i, i, 5 + i) for i in range(6)]]                           # ... and along a diagonal
    third = [[(3, b, c) for b in range(2, 7) for c in range(4, 11)],          # a flat plate
             [(a, b, c) for a in range(8, 12) for b in range(2, 6) for c in range(2, 6)],     # a filled cube: three equal eigenvalues
             [(14, 2, c) for c in range(8, 16)] + [(14, b, 15) for b in range(3, 8)],         # an L-shaped track
             [(6, b, 14) for b in range(8)], [(6, b, 16) for b in range(8)],  # two clusters interleaved in list order
             [(1, b, c) for b in range(2) for c in range(7)]]                 # 2 x 7: two members tie in t at either end
    holes = [(6, b, 15) for b in range(8)] + [(14, 3, 14), (0, 5, 5)]         # class 0 between members: id -1
    a, ac = _event(shape, first)
    c, cc = _event(shape, third, holes)
    off = np.array([0, a.size, a.size, a.size + c.size])
    index, cls = np.concatenate([a, c]), np.concatenate([ac, cc])
    cluster, toff = _ids(off, index, cls, shape, ClusterSpec(26))
    assert list(toff) == [0, 5, 5, 11] and (cluster == -1).sum() == len(holes)
    # rows in the order of their lowest list position: single, line 0, line 2, line 1, diagonal | 2 x 7, plate, the pair, cube, L
    row = np.where(cluster >= 0, cluster + toff[np.searchsorted(off, np.arange(index.size), side="right") - 1], -1)
    pair = row[(row == 7) | (row == 8)]
    assert pair.size == 16 and list(pair[:4]) == [7, 8, 7, 8]
    rng = np.random.default_rng(1)
    value = _values(rng, index.size)
    want = _check(lib, off, index, value, cluster, toff, shape)
    assert list(want["axis"][0]) == [1.0, 0.0, 0.0] and want["length"][0] == 0 and want["end_lo"][0] == want["end_hi"][0] == 0
    assert [list(want["axis"][k]) for k in (1, 2, 3)] == [[1, 0, 0], [0, 0, 1], [0, 1, 0]] and (want["eval"][0:4, 1:] == 0).all()
    assert (np.abs(want["eval"][4, 1:]) < 1e-14).all() and np.abs(want["axis"][4] - 3 ** -0.5).max() < 1e-15     # the diagonal
    assert want["eval"][9][0] == want["eval"][9][1] == want["eval"][9][2] == 1.25 and list(want["axis"][9]) == [1.0, 0.0, 0.0]
    tie = 5                                                                   # the 2 x 7 block: axis 2, rows b = 0 and b = 1 tie
    p0 = int(a.size + np.flatnonzero(c == np.ravel_multi_index((1, 0, 0), shape))[0])
    assert list(want["axis"][tie]) == [0.0, 0.0, 1.0] and (want["end_lo"][tie], want["end_hi"][tie]) == (p0, p0 + 6)
    # no values; a value of 2^15 and a NaN: flag bit 0, the charge as without them
    none = _check(lib, off, index, None, cluster, toff, shape)
    assert (none["charge"] == 0).all() and (none["flags"] == 0).all()
    odd = value.copy()
    j, k = int(np.flatnonzero(row == 2)[2]), int(np.flatnonzero(row == 9)[0])
    odd[j], odd[k] = np.float32(2.0 ** 15), np.float32(np.nan)
    zero = value.copy()
    zero[j] = zero[k] = 0
    flagged = _check(lib, off, index, odd, cluster, toff, shape)
    assert list(np.flatnonzero(flagged["flags"])) == [2, 9]
    assert np.array_equal(flagged["charge"], cluster_features_numpy(off, index, zero, cluster, toff, shape)["charge"])


def test_hand_made_shapes_2d(lib):
    shape = (24, 40)
    one = [[(0, 0)], [(2, c) for c in range(3, 30)], [(b, 38) for b in range(4, 20)], [(5 + i, 2 + i) for i in range(9)],
           [(b, c) for b in range(18, 22) for c in range(10, 21)]]
    two = [[(3, c) for c in range(5, 25)] + [(b, 24) for b in range(4, 15)], [(20, 1)], [(10, c) for c in range(2, 9)],
           [(12, c) for c in range(2, 9)]]
    a, ac = _event(shape, one, [(23, 39)])
    b, bc = _event(shape, two, [(11, c) for c in range(2, 9)])
    off = np.array([0, a.size, a.size + b.size])
    index, cls = np.concatenate([a, b]), np.concatenate([ac, bc])
    for conn in (4, 8):
        cluster, toff = _ids(off, index, cls, shape, ClusterSpec(conn))
        assert toff[-1] == (9 if conn == 8 else 17)                          # the diagonal falls apart at connectivity 4
        want = _check(lib, off, index, _values(np.random.default_rng(conn), index.size), cluster, toff, shape)
        assert all((want[name][:, 2] == 0).all() for name in ("s", "lo", "hi", "m", "d", "centroid", "axis"))


def test_no_entries_and_no_clusters(lib):
    shape = (6, 7, 8)
    z = np.zeros(0, np.int64)
    _check(lib, [0, 0, 0], z, z.astype(np.float32), z, [0, 0, 0], shape)
    _check(lib, [0, 0], z, None, z, [0, 0], shape, cap=5)
    index = np.array([1, 5, 9, 200, 3, 4])
    _check(lib, [0, 4, 6], index, np.ones(6, np.float32), np.full(6, -1), [0, 0, 0], shape, cap=6)     # entries, none in a cluster


def test_cross_block_accumulation(lib):
    """One cluster over a whole dense 40^3 event -- 64,000 entries, 250 workgroups adding to one row -- beside an event of 3,200
    two-voxel clusters.  The ids are written down, not computed: a full block is one component, and the pairs touch nothing."""
    shape = (40, 40, 40)
    dense = np.arange(64000)
    pairs = np.ravel_multi_index(np.array([(a, b, c + k) for a in range(0, 40, 2) for b in range(0, 40, 2) for c in range(0, 40, 5)
                                           for k in (0, 1)]).T, shape)
    assert (np.diff(pairs) > 0).all() and pairs.size == 6400
    off = np.array([0, dense.size, dense.size + pairs.size])
    cluster = np.concatenate([np.zeros(dense.size, np.int64), np.arange(pairs.size) // 2])
    value = _values(np.random.default_rng(2), int(off[-1]))
    want = _check(lib, off, np.concatenate([dense, pairs]), value, cluster, [0, 1, 3201], shape)
    assert want["n"][0] == 64000 and list(want["m"][0]) == [20, 20, 20] and (want["n"][1:] == 2).all()


def test_extreme_coordinates(lib):
    shape = (32768, 2, 2)
    index = np.ravel_multi_index(np.array([(0, 0, 0), (0, 0, 1), (32767, 1, 0), (32767, 1, 1)]).T, shape)
    want = _check(lib, [0, 4], index, np.array([1, 2, 3, 4], np.float32), [0, 0, 1, 1], [0, 2], shape)
    assert list(want["s"][1]) == [65534, 2, 1] and list(want["hi"][1]) == [32767, 1, 1]
    # ... and one cluster from end to end: the largest |x - m| and second moment the extents allow
    want = _check(lib, [0, 4], index, None, [0, 0, 0, 0], [0, 1], shape)
    assert want["dd"][0][0] == 2 * 16384 ** 2 + 2 * 16383 ** 2 and want["length"][0] >= 32767


def _random_list(seed, shape, occupancy, classes=3):
    rng = np.random.default_rng(seed)
    index = np.flatnonzero(rng.uniform(size=int(np.prod(shape))) < occupancy)
    return index, rng.integers(0, classes, index.size).astype(np.uint8), _values(rng, index.size)


def test_a_short_cap_bounds_the_tables(lib):
    shape = (24, 20, 28)
    index, cls, value = _random_list(9, shape, 0.05)
    off = np.array([0, 300, index.size])
    cluster, toff = _ids(off, index, cls, shape, ClusterSpec(26, (0, 1, 2)))
    total = int(toff[-1])
    assert total > 40
    for cap in (total + 3, total // 2, 1, 0):
        _check(lib, off, index, value, cluster, toff, shape, cap=cap)


@pytest.mark.parametrize("conn", [6, 26])
def test_random_lists(lib, conn):
    shape = (24, 20, 28)
    a, ac, av = _random_list(conn, shape, 0.05)
    b, bc, bv = _random_list(conn + 1, shape, 0.2 if conn == 6 else 0.1)
    off = np.array([0, a.size, a.size + b.size])
    index, cls, value = np.concatenate([a, b]), np.concatenate([ac, bc]), np.concatenate([av, bv])
    for same_class in (True, False):
        for min_size in (1, 3):
            cluster, toff = _ids(off, index, cls, shape, ClusterSpec(conn, None, same_class, min_size))
            assert toff[-1] > 20
            _check(lib, off, index, value, cluster, toff, shape)


# ---- the largest legal extents (tests/_far_corner.py) ---------------------------------------------------------------
@pytest.mark.parametrize("shape", far.SHAPES_CAPPED, ids=far.shape_id)
def test_far_corner(lib, shape):
    """The random lists against the far faces, at the origin and across index 2^30 (tests/test_far_corner_host.py asserts what the
    batch reaches), under the clustering they come with and under the narrowest one."""
    b = far.far_batch("random", shape).big
    want = _check(lib, b.off, b.index, b.value, b.cluster, b.toff, shape)
    top = np.array(shape + (1,) * (3 - len(shape))) - 1
    assert (want["hi"].max(axis=0) == top).all()
    cluster, toff, _ = far.clustered("random", shape, 6 if len(shape) == 3 else 4, False)
    assert toff[-1] > b.toff[-1]
    _check(lib, b.off, b.index, None, cluster, toff, shape)


@pytest.mark.parametrize("axis", sorted(far.LONG_TRACK))
def test_a_track_across_the_longest_axis(lib, axis):
    """One cluster of 32,768 members from the origin corner to the far corner: the largest sums and second moments a row takes."""
    s = far.long_track(far.LONG_TRACK[axis])
    want = _check(lib, s.off, s.index, s.value, s.cluster, s.toff, s.shape)
    assert want["n"].tolist() == [32768] and want["lo"][0].tolist() == [0, 0, 0] and want["hi"][0].tolist() == [d - 1 for d in s.shape]
    assert want["dd"][0][axis] > 2.9e12 and want["length"][0] > 32767


# ---- net level -----------------------------------------------------------------------------------------------------------------
DIMS = (32, 32, 32, 1)
FIELDS = [name for name, _, _ in INT_FIELDS + REAL_FIELDS]
_cache = {}


def _net(prec):
    net = uresnet(dims=list(DIMS), num_class=3, base_num_outputs=8, num_strides=2)
    net.construct(trainable=False, use_weight=False, seed=7, precision=prec)
    return net


def _events(n=2):
    if "vb" not in _cache:
        _cache["vb"] = VoxelBatch.concat([sio.dense_to_voxels(*sio.lartpc_sparse(list(DIMS), 3, e)) for e in range(n)]).validate()
    return _cache["vb"]


def _same_objects(r, vb, shape):
    """r['objects'] equals the statement evaluated on r['index'], the batch's values and r['cluster'], joined with r['clusters']."""
    counts = [t["first"].size for t in r["clusters"]]
    toff = np.concatenate([[0], np.cumsum(counts)])
    want = cluster_features_numpy(vb.offsets, np.concatenate(r["index"]), vb.value, np.concatenate(r["cluster"]), toff, shape)
    assert len(r["objects"]) == len(counts) and toff[-1] > 0
    for i, got in enumerate(r["objects"]):
        assert sorted(got) == sorted(FIELDS + ["first", "size", "cls"])
        for name in FIELDS:
            w = want[name][toff[i]:toff[i + 1]]
            assert got[name].dtype == w.dtype and got[name].shape == w.shape and np.array_equal(_bits(got[name]), _bits(w)), (i, name)
        for name in ("first", "size", "cls"):
            assert np.array_equal(got[name], r["clusters"][i][name]), (i, name)


@pytest.mark.parametrize("prec", ["fp32", "bf16"])
def test_inference_voxel_scores_with_objects(prec):
    net, vb = _net(prec), _events()
    spec = ClusterSpec(classes=(0, 1, 2), min_size=2)
    net.set_clustering(spec)
    off_r = net.inference_voxel_scores(None, vb, with_labels=False, want=("pred", "cluster"))
    assert sorted(off_r) == ["cluster", "clusters", "index", "pred"]                  # the setter never called: today's keys
    net.set_cluster_features(True)
    r = net.inference_voxel_scores(None, vb, with_labels=False, want=("pred", "cluster"))
    assert sorted(r) == ["cluster", "clusters", "index", "objects", "pred"]
    assert all(np.array_equal(a, b) for a, b in zip(r["cluster"], off_r["cluster"]))
    _same_objects(r, vb, DIMS[:-1])
    assert sorted(net.inference_voxel_scores(None, vb, with_labels=False, want=("pred",))) == ["index", "pred"]     # no 'cluster': none
    # the stand-alone call on the same lists gives the same records
    again = net.cluster_features(None, vb, None, {"cluster": r["cluster"], "clusters": r["clusters"]})
    for a, b in zip(again, r["objects"]):
        assert all(np.array_equal(_bits(a[name]), _bits(b[name])) for name in FIELDS)
    net.set_cluster_features(False)
    assert sorted(net.inference_voxel_scores(None, vb, with_labels=False, want=("pred", "cluster"))) == \
        ["cluster", "clusters", "index", "pred"]


@pytest.mark.parametrize("prec", ["fp32", "bf16"])
def test_tiled_objects_are_in_the_large_shape(prec):
    big, halo = (48, 40, 56), 4                                                       # two tiles per axis
    vb = VoxelBatch.concat([sio.dense_to_voxels(*sio.lartpc_sparse(list(big) + [1], 3, e)) for e in range(2)]).validate()
    net = _net(prec)
    net.set_clustering(ClusterSpec(classes=(0, 1, 2), same_class=False))
    net.set_cluster_features(True)
    r = net.inference_tiled_voxel_scores(None, vb, big, halo=halo, want=("pred", "cluster"))
    assert "objects" in r
    _same_objects(r, vb, big)


# ---- driver --------------------------------------------------------------------------------------------------------------------
def _drive(tmp_path, tag, extra, interactive=False):
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
        res = t.ana_step() if interactive else t.batch_process()
        t.reset()
    with open(str(out), "rb") as f:
        return f.read(), res


@pytest.mark.parametrize("tile", ["", "ANA_TILE [48, 40, 56]\nANA_TILE_HALO 4\n"], ids=["plain", "tiled"])
def test_driver_writes_one_row_per_cluster(tmp_path, tile):
    """The CSV parses back to the returned records; the driver's own records are byte for byte those of a run without the key."""
    shape = (48, 40, 56) if tile else (32, 32, 32)
    csv = tmp_path / "objects.csv"
    plain, ref = _drive(tmp_path, "plain", tile, interactive=True)
    with_key, res = _drive(tmp_path, "objects", tile + "ANA_OBJECTS '%s'\n" % csv, interactive=True)
    assert with_key == plain                                                          # the records do not change
    lines = csv.read_text().split("\n")
    assert lines[0] + "\n" == objects_csv_header() and lines[-1] == ""
    rows = [line.split(",") for line in lines[1:-1]]
    names = lines[0].split(",")
    at = 0
    for e, (ev, ev0) in enumerate(zip(res["voxels"], ref["voxels"])):
        assert sorted(ev) == sorted(list(ev0) + ["objects"])
        o = ev["objects"]
        assert o["n"].size == ev["clusters"]["first"].size > 0
        start = sum(v["index"].size for v in res["voxels"][:e])
        for k in range(o["n"].size):
            row = dict(zip(names, rows[at]))
            at += 1
            assert (int(row["entry"]), int(row["cluster"]), int(row["class"]), int(row["size"])) == \
                (int(res["entries"][e]), k, int(o["cls"][k]), int(o["size"][k]))
            assert float(row["charge"]) * 65536.0 == float(o["charge"][k]) and float(row["length"]) == o["length"][k]
            for name in ("centroid", "eval", "axis"):
                assert [float(row["%s_%d" % (name, a)]) for a in range(3)] == list(o[name][k]), (e, k, name)
            for name in ("end_lo", "end_hi"):
                x = np.unravel_index(int(ev["index"][int(o[name][k]) - start]), shape)
                assert [int(row["%s_%d" % (name, a)]) for a in range(3)] == [int(c) for c in x], (e, k, name)
    assert at == len(rows)
