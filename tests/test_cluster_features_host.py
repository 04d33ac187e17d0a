"""Per-cluster object records, host side (no GPU): the appended symbols under an unchanged ABI 9, the scratch query, every argument
refusal of ursn_cluster_features (include/uresnet_hip.h), the ANA_OBJECTS key and the driver's refusal, and the numpy statement
(uresnet_amd.clusters.cluster_features_numpy) against independent numpy.  Every library call below is refused on its arguments before
any device access, so the fake pointers are never dereferenced."""
import ctypes
import io
import os
from contextlib import redirect_stdout

import numpy as np
import pytest

import uresnet_amd  # noqa: F401
from uresnet_amd import _lib, ssnet_config, uresnet
from uresnet_amd.clusters import PAIRS, ClusterSpec, cluster_features_numpy, cluster_numpy, jacobi_eigen3
from uresnet_amd.ssnet import VoxelBatch, objects_csv_header

FAKE = 0x10000
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _p(a):
    return ctypes.c_void_p(a)


def test_symbols_appended_under_abi_9(lib):
    assert _lib.ABI_VERSION == 9 and lib.ursn_abi_version() == 9
    with open(os.path.join(ROOT, "include", "uresnet_hip.h")) as f:
        hdr = f.read()
    for name in ("ursn_cluster_features_scratch_bytes", "ursn_cluster_features"):
        assert name in _lib.EXPORTS and hasattr(lib, name) and (name + "(") in hdr, name
    assert "#define URSN_ABI_VERSION 9" in hdr and "} ursn_cluster_feat_desc;" in hdr and "} ursn_cluster_feat_out;" in hdr
    assert "#define URSN_CLFEAT_I %d " % _lib.CLFEAT_I in hdr and "#define URSN_CLFEAT_R %d " % _lib.CLFEAT_R in hdr
    assert (_lib.CLFEAT_I * 8) % 16 == 0 and (_lib.CLFEAT_R * 8) % 16 == 0
    assert ctypes.sizeof(_lib.ursn_cluster_feat_desc) == 72 and ctypes.sizeof(_lib.ursn_cluster_feat_out) == 32


def test_scratch_query(lib):
    """The domain only: at least 8 bytes, 8-byte granular, monotone in every argument inside it, 0 outside; no layout is pinned."""
    q = lib.ursn_cluster_features_scratch_bytes
    ms = (0, 1, 2047, 2048, 2049, 8000, 10 ** 6, 2 ** 31 - 1)
    for n in (1, 5, 65535):
        for cap in (0, 1, 8000, 2 ** 31):
            sizes = [q(n, m, cap) for m in ms]
            assert all(b >= 8 and b % 8 == 0 for b in sizes) and sizes == sorted(sizes) and sizes[0] < sizes[-1], (n, cap, sizes)
    for m in ms:
        by_cap = [q(5, m, cap) for cap in (0, 1, 100, 10 ** 6, 2 ** 31)]
        by_n = [q(n, m, 100) for n in (1, 2, 100, 65535)]
        assert by_cap == sorted(by_cap) and by_n == sorted(by_n), m
    for n, m, cap in ((0, 10, 10), (-1, 10, 10), (65536, 10, 10), (1, -1, 10), (1, 2 ** 31, 10), (1, 2 ** 40, 10), (1, 10, -1)):
        assert q(n, m, cap) == 0, (n, m, cap)


def _desc(ndim=3, spatial=(8, 8, 8), n=2, m_total=10, offsets=FAKE, index=FAKE + 0x1000, value=FAKE + 0x2000, cluster=FAKE + 0x3000,
          table_offsets=FAKE + 0x4000):
    d = _lib.ursn_cluster_feat_desc()
    d.ndim, d.n, d.m_total = ndim, n, m_total
    for i in range(3):
        d.spatial[i] = spatial[i] if i < len(spatial) else 0
    d.offsets, d.index, d.value, d.cluster, d.table_offsets = offsets, index, value, cluster, table_offsets
    return d


def _out(itab=FAKE + 0x10000, rtab=FAKE + 0x20000, cap=10, status=FAKE + 0x30000):
    o = _lib.ursn_cluster_feat_out()
    o.itab, o.rtab, o.cap, o.status = itab, rtab, cap, status
    return o


SCRATCH = FAKE + 0x40000


def _refused(lib, text, desc=None, out=None, scratch=SCRATCH, sbytes=1 << 20, okw=None, **kw):
    d = _desc(**kw) if desc is None else desc
    o = _out(**(okw or {})) if out is None else out
    rc = lib.ursn_cluster_features(ctypes.byref(d) if d != "null" else None, ctypes.byref(o) if o != "null" else None, _p(scratch),
                                   sbytes, None)
    msg = lib.ursn_last_error()
    assert rc != 0 and text in msg, (rc, msg)


def test_cluster_features_refusals(lib):
    """Null streams and fake device pointers: a call that got past its checks would fault here, not return."""
    who = b"cluster_features"
    r = lambda text, **kw: _refused(lib, who + text, **kw)
    r(b": null desc / out", desc="null")
    r(b": null desc / out", out="null")
    r(b": ndim = 1, must be 2 or 3", ndim=1)
    r(b": ndim = 4, must be 2 or 3", ndim=4)
    r(b": spatial[0] = 0 outside [1, 32768]", spatial=(0, 8, 8))
    r(b": spatial[2] = -3 outside [1, 32768]", spatial=(8, 8, -3))
    r(b": spatial[0] = 32769 outside [1, 32768]", spatial=(32769, 2, 2))
    r(b": spatial[1] = 32769 outside [1, 32768]", ndim=2, spatial=(2, 32769))
    r(b": prod(spatial) >= 2^31", spatial=(2048, 1024, 1024))
    r(b": prod(spatial) >= 2^31", spatial=(32768, 32768, 2))
    r(b": n = 0 outside [1, 65535]", n=0)
    r(b": n = 65536 outside [1, 65535]", n=65536)
    r(b": m_total = -1 outside [0, 2^31)", m_total=-1)
    r(b": m_total = 2147483648 outside [0, 2^31)", m_total=2 ** 31)
    r(b": cap = -1 < 0", okw=dict(cap=-1))
    r(b": null offsets / table_offsets", offsets=None)
    r(b": null offsets / table_offsets", table_offsets=None)
    r(b": null index / cluster", index=None)
    r(b": null index / cluster", cluster=None)
    r(b": null out->status", okw=dict(status=None))
    r(b": null out->itab / out->rtab", okw=dict(itab=None))
    r(b": null out->itab / out->rtab", okw=dict(rtab=None))
    r(b": null scratch", scratch=None)
    for kw in (dict(offsets=FAKE + 4), dict(table_offsets=FAKE + 0x4004), dict(okw=dict(itab=FAKE + 0x10004)),
               dict(okw=dict(rtab=FAKE + 0x20004)), dict(scratch=SCRATCH + 4)):
        r(b": offsets / table_offsets / itab / rtab / scratch must be 8-byte aligned", **kw)
    for kw in (dict(index=FAKE + 0x1002), dict(value=FAKE + 0x2002), dict(cluster=FAKE + 0x3001), dict(okw=dict(status=FAKE + 0x30002))):
        r(b": index / value / cluster / status must be 4-byte aligned", **kw)
    need = lib.ursn_cluster_features_scratch_bytes(2, 10, 10)
    assert need >= 8
    r(b": scratch of %d bytes is too small, %d needed" % (need - 8, need), sbytes=need - 8)
    r(b": scratch of 0 bytes is too small", sbytes=0)
    big = lib.ursn_cluster_features_scratch_bytes(2, 2 ** 31 - 1, 10)
    r(b": scratch of %d bytes is too small, %d needed" % (big - 8, big), m_total=2 ** 31 - 1, sbytes=big - 8)
    # the largest legal extent passes the argument checks: the refusal that comes is the LAST check's, the scratch size
    r(b": scratch of 0 bytes is too small", spatial=(32768, 2, 2), sbytes=0)
    r(b": scratch of 0 bytes is too small", ndim=2, spatial=(32768, 32768), sbytes=0)
    r(b": scratch of 0 bytes is too small", value=None, sbytes=0)                 # a null value list is legal


# ---- config key, driver, Python surface ----------------------------------------------------------------------------------------
def test_config_key_default_off_and_validated(tmp_path):
    c = ssnet_config()
    assert c.ANA_OBJECTS == ""
    out = io.StringIO()
    with redirect_stdout(out):
        c.dump()
    assert any(line.startswith("ANA_OBJECTS.") or line.startswith("ANA_OBJECTS ") for line in out.getvalue().split("\n"))
    p = tmp_path / "a.cfg"
    p.write_text("ANA_OBJECTS '/tmp/objects.csv'\n")
    with redirect_stdout(io.StringIO()):
        c.override(str(p))
    assert c.ANA_OBJECTS == "/tmp/objects.csv" and ssnet_config().ANA_OBJECTS == ""
    for text in ("ANA_OBJECTS True\n", "ANA_OBJECTS 1\n", "ANA_OBJECTS ['a.csv']\n", "ANA_OBJECTS None\n"):
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


def test_driver_refuses_ana_objects_without_ana_cluster(tmp_path):
    """Before a stream is opened or a device is touched; the file is not created."""
    csv = tmp_path / "objects.csv"
    for text in ("TRAIN False\nANA_OBJECTS '%s'\n" % csv,
                 "TRAIN False\nSPARSE_IO True\nSPARSE_SCORES True\nANA_OBJECTS '%s'\n" % csv):
        with pytest.raises(ValueError) as e:
            _driver(tmp_path, text).initialize()
        assert "ANA_OBJECTS" in str(e.value) and "ANA_CLUSTER" in str(e.value), str(e.value)
    assert not csv.exists()
    head = objects_csv_header()
    assert head.endswith("\n") and head.split(",")[:5] == ["entry", "cluster", "class", "size", "charge"] and len(head.split(",")) == 21


def test_set_cluster_features_leaves_want_as_it_was():
    """construct(allocate=False) never touches a device."""
    net = uresnet(dims=[16, 16, 16, 1], num_class=3, base_num_outputs=4, num_strides=2)
    net.construct(trainable=False, use_weight=False, allocate=False)
    vb = VoxelBatch([0, 1], [5], [2.0], [1.0], None, None, 16 ** 3)
    net.set_cluster_features(True)
    for want in (("cluster",), ("objects",), ("pred", "objects")):             # no spec: 'cluster' is unknown, 'objects' always is
        with pytest.raises(ValueError, match=r"non-empty subset of \('scores', 'pred', 'ana'\)"):
            net.inference_voxel_scores(None, vb, want=want)
    net.set_clustering(ClusterSpec())
    for call in (lambda: net.inference_voxel_scores(None, vb, want=("softmax",)),
                 lambda: net.inference_voxel_scores(None, vb, want=("cluster", "objects")),
                 lambda: net.inference_tiled_voxel_scores(None, vb, (16, 16, 16), want=("clusters",)),
                 lambda: net.inference_tiled_voxel_scores(None, vb, (16, 16, 16), want=("objects",))):
        with pytest.raises(ValueError, match=r"non-empty subset of \('scores', 'pred', 'ana', 'cluster'\)"):
            call()
    for bad in (1, None, "on"):
        with pytest.raises(ValueError):
            net.set_cluster_features(bad)
    net.set_cluster_features(False)


# ---- the statement against independent numpy -----------------------------------------------------------------------------------
CASES = [((12, 10, 14), 6, 0.25, 1), ((12, 10, 14), 26, 0.06, 2), ((9, 16, 11), 18, 0.1, 3), ((20, 24), 4, 0.45, 4),
         ((20, 24), 8, 0.2, 5)]
_stat = {}


def _case(k):
    """One random list, clustered by cluster_numpy, and the statement on it (computed once, shared, never changed)."""
    if k not in _stat:
        shape, conn, occupancy, seed = CASES[k]
        rng = np.random.default_rng(seed)
        index = np.flatnonzero(rng.uniform(size=int(np.prod(shape))) < occupancy)
        value = rng.uniform(0.0, 50.0, index.size).astype(np.float32)
        cluster, first, size, _ = cluster_numpy(index, np.ones(index.size, np.uint8), shape, ClusterSpec(conn))
        f = cluster_features_numpy([0, index.size], index, value, cluster, [0, first.size], shape)
        x = np.stack(np.unravel_index(index, shape), axis=1)
        if len(shape) == 2:
            x = np.concatenate([x, np.zeros((index.size, 1), np.int64)], axis=1)
        for a in f.values():
            a.flags.writeable = False
        _stat[k] = (shape, index, value, cluster, first, size, f, x)
    return _stat[k]


@pytest.mark.parametrize("k", range(len(CASES)))
def test_first_order_fields_against_bincount(k):
    shape, index, value, cluster, first, size, f, x = _case(k)
    K = first.size
    assert K > 5 and f["n"].dtype == np.int64 and np.array_equal(f["n"], size) and np.array_equal(f["n"], np.bincount(cluster, minlength=K))
    lo, hi = np.full((K, 3), 1 << 40), np.full((K, 3), -1)
    np.minimum.at(lo, cluster, x)
    np.maximum.at(hi, cluster, x)
    assert np.array_equal(f["lo"], lo) and np.array_equal(f["hi"], hi)
    for a in range(3):
        s = np.bincount(cluster, weights=x[:, a], minlength=K).astype(np.int64)       # exact: small integers in fp64
        assert np.array_equal(f["s"][:, a], s)
        assert np.array_equal(f["centroid"][:, a], s / f["n"])
    assert np.array_equal(f["m"], np.floor(f["centroid"] + 0.5).astype(np.int64))     # the centroid rounded to a voxel
    assert (np.abs(f["d"]) * 2 <= f["n"][:, None]).all()                               # |d / n| <= 0.5
    q = np.rint(value.astype(np.float64) * 65536.0).astype(np.int64)
    assert np.array_equal(f["charge"], np.bincount(cluster, weights=q, minlength=K).astype(np.int64)) and (f["flags"] == 0).all()
    if len(shape) == 2:
        assert all((f[name][:, 2] == 0).all() for name in ("lo", "hi", "s", "m", "d", "centroid", "axis"))
        assert (f["dd"][:, [2, 4, 5]] == 0).all() and (f["cov"][:, [2, 4, 5]] == 0).all()


def _full(c):
    return np.array([[c[0], c[3], c[4]], [c[3], c[1], c[5]], [c[4], c[5], c[2]]])


def test_second_order_fields_against_numpy_cov_and_eigh():
    """cov within 1e-12 max(1, trace) of np.cov(bias=True): the anchor bounds the correction term by 0.25 and every other step is
    one rounding.  eval within 1e-10 max(trace, 1) of eigvalsh.  |axis . v| >= 1 - 1e-9 where the leading gap is at least 1e-3 of the
    trace (perturbation theory: angle error ~ eps trace / gap ~ 1e-13); the filter may leave out at most 10 % of the clusters of
    size >= 3."""
    seen = kept = 0
    for k in range(len(CASES)):
        shape, index, value, cluster, first, size, f, x = _case(k)
        for row in range(first.size):
            pts = x[cluster == row].astype(np.float64)
            ref = np.cov(pts.T, bias=True).reshape(3, 3) if pts.shape[0] > 1 else np.zeros((3, 3))
            trace = float(np.trace(ref))
            cov = _full(f["cov"][row])
            assert np.abs(cov - ref).max() <= 1e-12 * max(1.0, trace), (k, row)
            w, v = np.linalg.eigh(ref)
            assert np.abs(f["eval"][row] - w[::-1]).max() <= 1e-10 * max(trace, 1.0), (k, row)
            assert f["eval"][row][0] >= f["eval"][row][1] >= f["eval"][row][2]
            ax = f["axis"][row]
            assert abs(float(ax @ ax) - 1.0) < 1e-12 and ax[np.argmax(np.abs(ax))] > 0
            if size[row] >= 3:
                seen += 1
                if w[2] - w[1] >= 1e-3 * trace:
                    kept += 1
                    assert abs(float(ax @ v[:, 2])) >= 1 - 1e-9, (k, row)
    assert seen >= 80 and kept >= 0.9 * seen, (seen, kept)


@pytest.mark.parametrize("k", range(len(CASES)))
def test_end_points_against_brute_force(k):
    shape, index, value, cluster, first, size, f, x = _case(k)
    for row in range(first.size):
        mem = np.flatnonzero(cluster == row)
        dx = (x[mem] - f["m"][row]).astype(np.float64)
        ax = f["axis"][row]
        t = ((ax[0] * dx[:, 0] + ax[1] * dx[:, 1]) + ax[2] * dx[:, 2]).astype(np.float32) + np.float32(0.0)
        lo, hi = mem[np.argmin(t)], mem[np.argmax(t)]                 # argmin / argmax return the FIRST extreme: the lower position
        assert (f["end_lo"][row], f["end_hi"][row]) == (lo, hi), (k, row)
        assert f["t_lo"][row] == t.min() and f["t_hi"][row] == t.max() and f["t_lo"].dtype == np.float32
        assert f["length"][row] == np.float64(t.max()) - np.float64(t.min())
        if size[row] == 1:
            assert lo == hi == first[row] and f["length"][row] == 0 and list(ax) == [1.0, 0.0, 0.0]


def test_statement_edges():
    shape = (6, 7, 8)
    # a symmetric line along axis 2 around its anchor: both ends tie in |t|, not in t; a 2 x 2 square: t ties at both ends
    line = np.ravel_multi_index(np.array([(1, 1, c) for c in range(1, 6)]).T, shape)
    square = np.ravel_multi_index(np.array([(4, 4, 4), (4, 4, 5), (4, 5, 4), (4, 5, 5)]).T, shape)
    index = np.concatenate([line, square])
    cluster = np.array([0] * 5 + [1] * 4)
    value = np.array([1.5, 2.0 ** 15, np.nan, -2.25, np.inf, 0.5, 0.25, -(2.0 ** 15), 2.0 ** -17], np.float32)
    f = cluster_features_numpy([0, 9], index, value, cluster, [0, 2], shape)
    assert list(f["flags"]) == [1, 1] and list(f["charge"]) == [int((1.5 - 2.25) * 65536), int(0.75 * 65536)]   # 2^-17 rounds to even: 0
    assert list(f["axis"][0]) == [0.0, 0.0, 1.0] and list(f["eval"][0]) == [2.0, 0.0, 0.0] and f["length"][0] == 4.0
    assert (f["end_lo"][0], f["end_hi"][0]) == (0, 4)
    assert list(f["eval"][1]) == [0.25, 0.25, 0.0] and list(f["m"][1]) == [4, 5, 5]
    # equal eigenvalues keep the lower column first: the axis is coordinate axis 1, and two members tie at each end
    assert list(f["axis"][1]) == [0.0, 1.0, 0.0] and f["length"][1] == 1.0
    assert (f["end_lo"][1], f["end_hi"][1]) == (5, 7)                            # the LOWER position of each tied pair
    none = cluster_features_numpy([0, 9], index, None, cluster, [0, 2], shape)
    assert list(none["charge"]) == [0, 0] and list(none["flags"]) == [0, 0] and np.array_equal(none["dd"], f["dd"])
    empty = cluster_features_numpy([0, 0, 0], np.zeros(0, np.int64), None, np.zeros(0, np.int64), [0, 0, 0], shape)
    assert empty["n"].shape == (0,) and empty["dd"].shape == (0, 6) and empty["t_lo"].dtype == np.float32
    ev, ax = jacobi_eigen3([1.0, 1.0, 1.0, 0.0, 0.0, 0.0])                      # three equal eigenvalues: every rotation skipped
    assert list(ev) == [1.0, 1.0, 1.0] and list(ax) == [1.0, 0.0, 0.0] and len(PAIRS) == 6
    with pytest.raises(ValueError):
        cluster_features_numpy([0, 9], index, value, cluster, [0, 2], (6, 7, 32769))
    with pytest.raises(ValueError):
        cluster_features_numpy([0, 9], index, value, cluster, [0, 3], shape)    # a row without members
