"""Voxel clusters, host side (no GPU): the appended symbols under an unchanged ABI 9, the scratch query, every argument refusal of
ursn_cluster_voxels (include/uresnet_hip.h), ClusterSpec, the config keys and the driver's refusals, and the numpy statement
(uresnet_amd.clusters.cluster_numpy) against scipy.ndimage.label.  Every library call below is refused on its arguments before any
device access, so the fake pointers are never dereferenced."""
import ctypes
import io
import os
from contextlib import redirect_stdout

import numpy as np
import pytest

import uresnet_amd  # noqa: F401
from uresnet_amd import _lib, ssnet_config, uresnet
from uresnet_amd.clusters import ClusterSpec, cluster_numpy
from uresnet_amd.ssnet import VoxelBatch

FAKE = 0x10000
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _p(a):
    return ctypes.c_void_p(a)


def test_symbols_appended_under_abi_9(lib):
    assert _lib.ABI_VERSION == 9 and lib.ursn_abi_version() == 9
    with open(os.path.join(ROOT, "include", "uresnet_hip.h")) as f:
        hdr = f.read()
    for name in ("ursn_cluster_scratch_bytes", "ursn_cluster_voxels"):
        assert name in _lib.EXPORTS and hasattr(lib, name) and (name + "(") in hdr, name
    assert "#define URSN_ABI_VERSION 9" in hdr and "typedef struct ursn_cluster_desc" in hdr and "} ursn_cluster_out;" in hdr
    assert ctypes.sizeof(_lib.ursn_cluster_desc) == 72 and ctypes.sizeof(_lib.ursn_cluster_out) == 64


def test_scratch_query(lib):
    """The domain only: at least 8 bytes, 8-byte granular and growing with the list inside it, 0 outside; no layout is pinned."""
    q = lib.ursn_cluster_scratch_bytes
    for n in (1, 5, 65535):
        sizes = [q(n, m) for m in (0, 1, 2047, 2048, 2049, 8000, 10 ** 6, 2 ** 31 - 1)]
        assert all(b >= 8 and b % 8 == 0 for b in sizes) and sizes == sorted(sizes) and sizes[0] < sizes[-1], (n, sizes)
        assert q(n, 8000) >= 4 * 8000                                           # at least a word per entry: it scales with the list
    for n, m in ((0, 10), (-1, 10), (65536, 10), (1, -1), (1, 2 ** 31), (1, 2 ** 40)):
        assert q(n, m) == 0, (n, m)


def _desc(ndim=3, spatial=(8, 8, 8), n=2, m_total=10, offsets=FAKE, index=FAKE + 0x1000, cls=FAKE + 0x2001, connectivity=26,
          class_mask=0xFFFFFFFE, same_class=1, min_size=1):
    d = _lib.ursn_cluster_desc()
    d.ndim, d.n, d.m_total = ndim, n, m_total
    for i in range(3):
        d.spatial[i] = spatial[i] if i < len(spatial) else 0
    d.offsets, d.index, d.cls = offsets, index, cls
    d.connectivity, d.class_mask, d.same_class, d.min_size = connectivity, class_mask, same_class, min_size
    return d


def _out(cluster=FAKE + 0x10000, count=FAKE + 0x11000, first=FAKE + 0x12000, size=FAKE + 0x13000, cls=FAKE + 0x14001,
         table_offsets=FAKE + 0x15000, cap=10, status=FAKE + 0x16000):
    o = _lib.ursn_cluster_out()
    for name in ("cluster", "count", "first", "size", "cls", "table_offsets", "status"):
        setattr(o, name, locals()[name])
    o.cap = cap
    return o


SCRATCH = FAKE + 0x20000


def _refused(lib, text, desc=None, out=None, scratch=SCRATCH, sbytes=1 << 20, okw=None, **kw):
    d = _desc(**kw) if desc is None else desc
    o = _out(**(okw or {})) if out is None else out
    rc = lib.ursn_cluster_voxels(ctypes.byref(d) if d != "null" else None, ctypes.byref(o) if o != "null" else None, _p(scratch),
                                 sbytes, None)
    msg = lib.ursn_last_error()
    assert rc != 0 and text in msg, (rc, msg)


def test_cluster_voxels_refusals(lib):
    who = b"cluster_voxels"
    r = lambda text, **kw: _refused(lib, who + text, **kw)
    r(b": null desc / out", desc="null")
    r(b": null desc / out", out="null")
    r(b": ndim = 1, must be 2 or 3", ndim=1)
    r(b": ndim = 4, must be 2 or 3", ndim=4)
    r(b": spatial[0] = 0 < 1", spatial=(0, 8, 8))
    r(b": spatial[2] = -3 < 1", spatial=(8, 8, -3))
    r(b": prod(spatial) >= 2^31", spatial=(2048, 1024, 1024))
    r(b": prod(spatial) >= 2^31", ndim=2, spatial=(65536, 32768), connectivity=8)
    for c in (5, 0, 27, 4, 8, -6):
        r(b": connectivity = %d, must be 6, 18 or 26 in 3-D and 4 or 8 in 2-D" % c, connectivity=c)
    for c in (18, 6, 26, 5):
        r(b": connectivity = %d, must be 6, 18 or 26 in 3-D and 4 or 8 in 2-D" % c, ndim=2, spatial=(8, 8), connectivity=c)
    r(b": same_class = 2, must be 0 or 1", same_class=2)
    r(b": min_size = 0 < 1", min_size=0)
    r(b": min_size = -4 < 1", min_size=-4)
    r(b": n = 0 outside [1, 65535]", n=0)
    r(b": n = 65536 outside [1, 65535]", n=65536)
    r(b": m_total = -1 outside [0, 2^31)", m_total=-1)
    r(b": m_total = 2147483648 outside [0, 2^31)", m_total=2 ** 31)
    r(b": null offsets", offsets=None)
    r(b": null index / cls", index=None)
    r(b": null index / cls", cls=None)
    r(b": null out->cluster", okw=dict(cluster=None))
    r(b": null out->count / out->status", okw=dict(count=None))
    r(b": null out->count / out->status", okw=dict(status=None))
    r(b": cap = -1 < 0", okw=dict(cap=-1))
    for name in ("first", "size", "cls"):
        keep = dict(first=None, size=None, cls=None, table_offsets=None)
        del keep[name]
        r(b": a table array needs table_offsets", okw=keep)
    r(b": null scratch", scratch=None)
    r(b": offsets / table_offsets / scratch must be 8-byte aligned", offsets=FAKE + 4)
    r(b": offsets / table_offsets / scratch must be 8-byte aligned", okw=dict(table_offsets=FAKE + 0x15004))
    r(b": offsets / table_offsets / scratch must be 8-byte aligned", scratch=SCRATCH + 4)
    r(b": index / cluster / count / first / size / status must be 4-byte aligned", index=FAKE + 0x1002)
    for name in ("cluster", "count", "first", "size", "status"):
        r(b": index / cluster / count / first / size / status must be 4-byte aligned", okw={name: FAKE + 0x1A002})
    need = lib.ursn_cluster_scratch_bytes(2, 10)
    assert need >= 8
    r(b": scratch of %d bytes is too small, %d needed" % (need - 8, need), sbytes=need - 8)
    r(b": scratch of 0 bytes is too small", sbytes=0)
    big = lib.ursn_cluster_scratch_bytes(2, 2 ** 31 - 1)
    r(b": scratch of %d bytes is too small, %d needed" % (big - 8, big), m_total=2 ** 31 - 1, sbytes=big - 8)


# ---- ClusterSpec ---------------------------------------------------------------------------------------------------------------
def test_cluster_spec_validation():
    s = ClusterSpec()
    assert (s.connectivity, s.classes, s.same_class, s.min_size, s.on) == (None, None, True, 1, "pred")
    assert s.axes(3) == (26, 3) and s.axes(2) == (8, 2) and s.class_mask() == 0xFFFFFFFE
    assert ClusterSpec(6).axes(3) == (6, 1) and ClusterSpec(18).axes(3) == (18, 2) and ClusterSpec(4).axes(2) == (4, 1)
    assert ClusterSpec(classes=[0, 2, 31]).class_mask() == (1 | 4 | 1 << 31) and ClusterSpec(classes=()).class_mask() == 0
    for ndim, c in ((2, 6), (2, 18), (2, 26), (3, 4), (3, 8)):
        with pytest.raises(ValueError):
            ClusterSpec(c).axes(ndim)
    with pytest.raises(ValueError):
        ClusterSpec().axes(4)
    for kw in (dict(connectivity=5), dict(connectivity=27), dict(connectivity=6.0), dict(connectivity="26"), dict(classes=[1, 1]),
               dict(classes=[-1]), dict(classes=[32]), dict(classes=[1.0]), dict(same_class=1), dict(min_size=0),
               dict(min_size=2.0), dict(min_size=2 ** 31), dict(on="scores"), dict(on=None)):
        with pytest.raises(ValueError):
            ClusterSpec(**kw)


# ---- config keys and the driver ------------------------------------------------------------------------------------------------
def test_config_keys_default_off_and_validated(tmp_path):
    c = ssnet_config()
    assert (c.ANA_CLUSTER, c.CLUSTER_CONNECTIVITY, c.CLUSTER_CLASSES, c.CLUSTER_MIN_SIZE) == ("", 0, [], 1)
    assert c.cluster_spec() is None
    out = io.StringIO()
    with redirect_stdout(out):
        c.dump()
    for key in ("ANA_CLUSTER", "CLUSTER_CONNECTIVITY", "CLUSTER_CLASSES", "CLUSTER_MIN_SIZE"):
        assert any(line.startswith(key + ".") or line.startswith(key + " ") for line in out.getvalue().split("\n")), key
    p = tmp_path / "a.cfg"
    p.write_text("ANA_CLUSTER 'ana'\nCLUSTER_CONNECTIVITY 18\nCLUSTER_CLASSES [1, 2]\nCLUSTER_MIN_SIZE 5\n")
    with redirect_stdout(io.StringIO()):
        c.override(str(p))
    assert (c.ANA_CLUSTER, c.CLUSTER_CONNECTIVITY, c.CLUSTER_CLASSES, c.CLUSTER_MIN_SIZE) == ("ana", 18, [1, 2], 5)
    s = c.cluster_spec()
    assert (s.connectivity, s.classes, s.same_class, s.min_size, s.on) == (18, (1, 2), True, 5, "ana")
    assert ssnet_config().ANA_CLUSTER == "" and ssnet_config().CLUSTER_CLASSES == []
    for text in ("ANA_CLUSTER True\n", "ANA_CLUSTER 'scores'\n", "ANA_CLUSTER 1\n", "CLUSTER_CONNECTIVITY 5\n",
                 "CLUSTER_CONNECTIVITY 26.0\n", "CLUSTER_CONNECTIVITY '26'\n", "CLUSTER_CLASSES (1, 2)\n", "CLUSTER_CLASSES [1.0]\n",
                 "CLUSTER_CLASSES [1, 1]\n", "CLUSTER_CLASSES [32]\n", "CLUSTER_CLASSES 1\n", "CLUSTER_MIN_SIZE 0\n",
                 "CLUSTER_MIN_SIZE 2.0\n", "CLUSTER_MIN_SIZE [2]\n"):
        bad = tmp_path / "b.cfg"
        bad.write_text(text)
        with redirect_stdout(io.StringIO()), pytest.raises(TypeError):
            ssnet_config().override(str(bad))


def _driver(tmp_path, text):
    from uresnet_amd.ssnet_trainval import ssnet_trainval
    inp = tmp_path / "in.cfg"
    inp.write_text("Dims [16, 16, 16, 1]\nNumClass 3\nGenerator 'lartpc_sparse'\nNumEntries 4\n")
    cfg = tmp_path / "net.cfg"
    cfg.write_text("MAIN_INPUT_CONFIG '%s'\nLOGDIR ''\nSAVE_FILE ''\nMINIBATCH_SIZE 1\n%s" % (inp, text))
    t = ssnet_trainval()
    with redirect_stdout(io.StringIO()):
        t.override_config(str(cfg))
    return t


def test_driver_refuses_ana_cluster_without_its_companions(tmp_path):
    """Every refusal comes before a stream is opened or a device is touched."""
    csv = tmp_path / "a.csv"
    for text, words in (("TRAIN False\nANA_CLUSTER 'pred'\n", ("ANA_CLUSTER", "SPARSE_IO")),
                        ("TRAIN False\nSPARSE_IO True\nANA_CLUSTER 'pred'\n", ("ANA_CLUSTER", "SPARSE_SCORES", "ANA_TILE")),
                        ("TRAIN False\nSPARSE_SCORES True\nANA_CLUSTER 'ana'\n", ("ANA_CLUSTER", "SPARSE_IO")),
                        ("TRAIN False\nSPARSE_IO True\nANA_CLUSTER 'ana'\nANA_CSV '%s'\n" % csv, ("ANA_CLUSTER", "ANA_CSV")),
                        ("TRAIN False\nANA_CLUSTER 'ana'\nANA_CSV '%s'\n" % csv, ("ANA_CLUSTER", "ANA_CSV")),
                        ("TRAIN False\nSPARSE_IO True\nSPARSE_SCORES True\nANA_CLUSTER 'pred'\nANA_TTA [0, 1]\n",
                         ("ANA_CLUSTER", "ANA_TTA", "cluster_voxels"))):
        with pytest.raises(ValueError) as e:
            _driver(tmp_path, text).initialize()
        for w in words:
            assert w in str(e.value), (text, str(e.value))
    assert not csv.exists()


def test_cluster_wanted_without_a_spec_is_an_unknown_name():
    """construct(allocate=False) never touches a device: whatever came after the refusal would raise something else."""
    net = uresnet(dims=[16, 16, 16, 1], num_class=3, base_num_outputs=4, num_strides=2)
    net.construct(trainable=False, use_weight=False, allocate=False)
    vb = VoxelBatch([0, 1], [5], [2.0], [1.0], None, None, 16 ** 3)
    for call in (lambda: net.inference_voxel_scores(None, vb, want=("cluster",)),
                 lambda: net.inference_voxel_scores(None, vb, want=("pred", "cluster")),
                 lambda: net.inference_tiled_voxel_scores(None, vb, (16, 16, 16), want=("cluster",))):
        with pytest.raises(ValueError, match="non-empty subset"):
            call()
    net.set_clustering(ClusterSpec())
    with pytest.raises(ValueError, match=r"\('scores', 'pred', 'ana', 'cluster'\)"):
        net.inference_voxel_scores(None, vb, want=("softmax",))
    for call in (lambda: net.inference_voxel_scores(None, vb, want=("cluster", "softmax")),
                 lambda: net.inference_voxel_scores(None, vb, want=()),
                 lambda: net.inference_tiled_voxel_scores(None, vb, (16, 16, 16), want=("clusters",))):
        with pytest.raises(ValueError, match="non-empty subset"):
            call()
    net.set_clustering(None)
    with pytest.raises(ValueError, match="non-empty subset"):
        net.inference_voxel_scores(None, vb, want=("cluster",))
    for bad in ("pred", 26, ClusterSpec(connectivity=8)):
        with pytest.raises(ValueError):
            net.set_clustering(bad)
    two = uresnet(dims=[16, 16, 16, 1], num_class=2, base_num_outputs=4, num_strides=2)
    two.construct(trainable=False, use_weight=False, allocate=False)
    with pytest.raises(ValueError, match="ana"):
        two.set_clustering(ClusterSpec(on="ana"))
    two.set_clustering(ClusterSpec(on="pred"))


# ---- the statement against scipy -----------------------------------------------------------------------------------------------
def _structure(ndim, axes):
    grid = np.stack(np.meshgrid(*[np.arange(-1, 2)] * ndim, indexing="ij"), axis=-1)
    return (np.abs(grid).sum(axis=-1) <= axes)


def _scipy_ids(dense, ndim, axes, min_size=1):
    """scipy's labels per voxel, components below min_size dropped and the rest renumbered in scipy's own order."""
    ndi = pytest.importorskip("scipy.ndimage")
    lab, k = ndi.label(dense, structure=_structure(ndim, axes))
    sizes = np.bincount(lab.reshape(-1), minlength=k + 1)
    keep = np.flatnonzero(sizes[1:] >= min_size) + 1
    remap = np.full(k + 1, -1, np.int64)
    remap[keep] = np.arange(keep.size)
    return remap[lab], keep.size


@pytest.mark.parametrize("shape,conns", [((12, 10, 14), (6, 18, 26)), ((20, 24), (4, 8))], ids=["3d", "2d"])
@pytest.mark.parametrize("occupancy", [0.05, 0.12, 0.3, 0.6])
def test_cluster_numpy_is_scipy_label(shape, conns, occupancy):
    pytest.importorskip("scipy.ndimage")
    rng = np.random.default_rng(int(occupancy * 100) + len(shape))
    vox = int(np.prod(shape))
    index = np.flatnonzero(rng.uniform(size=vox) < occupancy).astype(np.int32)
    cls = rng.integers(1, 4, index.size).astype(np.uint8)
    counts = []
    for c in conns:
        axes = conns.index(c) + 1
        # one class: every listed voxel takes part, classes ignored
        spec = ClusterSpec(c, classes=[1, 2, 3], same_class=False)
        cluster, first, size, tcls = cluster_numpy(index, cls, shape, spec)
        dense = np.zeros(vox, bool)
        dense[index] = True
        want, k = _scipy_ids(dense.reshape(shape), len(shape), axes)
        assert np.array_equal(cluster, want.reshape(-1)[index]) and first.size == k, (c, occupancy)
        assert np.array_equal(size, np.bincount(cluster, minlength=k)) and np.array_equal(tcls, cls[first])
        assert np.array_equal(first, [np.flatnonzero(cluster == i)[0] for i in range(k)])
        counts.append((k, int(size.max()) if k else 0))
        # per class with same_class: scipy once per class, the ids merged in the order of their lowest list position
        for min_size in (1, 3):
            spec = ClusterSpec(c, classes=[1, 3], same_class=True, min_size=min_size)
            cluster, first, size, tcls = cluster_numpy(index, cls, shape, spec)
            tag = np.full(index.size, -1, np.int64)
            base = 0
            for k_cls in (1, 3):
                dense = np.zeros(vox, bool)
                dense[index[cls == k_cls]] = True
                want, k = _scipy_ids(dense.reshape(shape), len(shape), axes, min_size)
                got = want.reshape(-1)[index]
                sel = (cls == k_cls) & (got >= 0)
                tag[sel] = got[sel] + base
                base += k
            # renumber the per-class tags by lowest list position
            order, seen = {}, 0
            want_ids = np.full(index.size, -1, np.int32)
            for j in range(index.size):
                if tag[j] >= 0:
                    if tag[j] not in order:
                        order[tag[j]] = seen
                        seen += 1
                    want_ids[j] = order[tag[j]]
            assert np.array_equal(cluster, want_ids) and first.size == seen, (c, occupancy, min_size)
            assert (cluster[cls == 2] == -1).all() and np.array_equal(tcls, cls[first])
            assert np.array_equal(size, np.bincount(cluster[cluster >= 0], minlength=seen)) and (size >= min_size).all()
    if len(shape) == 3 and occupancy == 0.05:
        assert counts[0][0] >= 60 and counts[0][1] <= 4          # many small clusters at connectivity 6
    if len(shape) == 3 and occupancy == 0.6:
        assert counts[-1][0] <= 3 and counts[-1][1] >= 900       # one giant cluster at connectivity 26


def test_cluster_numpy_edges():
    spec = ClusterSpec()
    cluster, first, size, tcls = cluster_numpy(np.zeros(0, np.int32), np.zeros(0, np.uint8), (4, 5, 6), spec)
    assert cluster.shape == (0,) and cluster.dtype == np.int32 and first.size == size.size == tcls.size == 0
    # x = 5 of one row and x = 0 of the next; the last row of a plane and the first row of the next: adjacent indices, no neighbours
    index = np.array([5, 6, 59, 60, 120], np.int64)
    cls = np.array([1, 1, 1, 1, 1], np.uint8)
    for c in (6, 18, 26):
        cluster, first, _, _ = cluster_numpy(np.append(index, [-1]), np.append(cls, [1]), (4, 5, 6), ClusterSpec(c))
        assert list(cluster[:2]) == [0, 1] and cluster[4] == -1 and cluster[5] == -1, c      # 120 == prod(spatial), -1: no part
        assert list(cluster[2:4]) == [2, 3] and first.size == 4, c
    with pytest.raises(ValueError):
        cluster_numpy([1, 2], [1], (4, 5, 6), spec)
