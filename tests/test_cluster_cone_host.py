"""Cluster cones, host side (no GPU): the appended symbols under an unchanged ABI 9, the scratch query, every argument refusal of
ursn_cluster_cones (include/uresnet_hip.h), ClusterConeSpec, the ANA_CONES / CONE_* keys and the driver's refusal,
set_cluster_cones, the arithmetic that puts the GPU test's lattice and far scene past the one-step thresholds of
csrc/cluster_cone.hip, and the pure-Python statement (uresnet_amd.clusters.cluster_cones_numpy): hand-built scenes with hand-checked
answers, invariants, the coverage of exactly the lists tests/test_cluster_cone_gpu.py runs (tests/_cone_cases.py makes them for both
files), and the value of the feature on the toy showers.  Every library call below is refused on its arguments before any device
access, so the fake pointers are never dereferenced."""
import ctypes
import io
import os
import re
from contextlib import redirect_stdout

import numpy as np
import pytest

import _cone_cases as cases
import uresnet_amd  # noqa: F401
from uresnet_amd import _lib, ssnet_config, uresnet
from uresnet_amd.clusters import (CONE_EVENT, CONE_INT, CONE_MAX_REACH, CONE_REAL, LINK_INT, LINK_REAL, ClusterConeSpec, ClusterSpec,
                                  cluster_cones_numpy, cluster_features_numpy, cluster_match_numpy, cone_link)
from uresnet_amd.ssnet import chains_csv_header, cones_csv_header, cones_csv_row

FAKE = 0x10000
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _p(a):
    return ctypes.c_void_p(a)


def _bits(x):
    return int(np.float64(x).view(np.uint64))


def test_symbols_appended_under_abi_9(lib):
    assert _lib.ABI_VERSION == 9 and lib.ursn_abi_version() == 9
    with open(os.path.join(ROOT, "include", "uresnet_hip.h")) as f:
        hdr = f.read()
    for name in ("ursn_cluster_cones_scratch_bytes", "ursn_cluster_cones"):
        assert name in _lib.EXPORTS and hasattr(lib, name) and (name + "(") in hdr, name
    assert "#define URSN_ABI_VERSION 9" in hdr and "} ursn_cluster_cone_desc;" in hdr and "} ursn_cluster_cone_out;" in hdr
    for name in ("SI", "SR", "LI", "LR", "EV"):
        assert "#define URSN_CLCONE_%s %d " % (name, getattr(_lib, "CLCONE_" + name)) in hdr, name
    assert (_lib.CLCONE_SI, _lib.CLCONE_SR, _lib.CLCONE_LI, _lib.CLCONE_LR, _lib.CLCONE_EV) == \
        (len(CONE_INT), len(CONE_REAL), len(LINK_INT), len(LINK_REAL), len(CONE_EVENT)) == (16, 4, 6, 4, 4)
    assert ctypes.sizeof(_lib.ursn_cluster_cone_desc) == 120 and ctypes.sizeof(_lib.ursn_cluster_cone_out) == 160
    assert CONE_MAX_REACH == 127
    # the section stands between the chains' and the vertices': nothing that other tests pin moved
    assert hdr.index("ursn_cluster_chains(") < hdr.index("ursn_cluster_cones_scratch_bytes(") < hdr.index("ursn_cluster_cones(") < \
        hdr.index("ursn_cluster_vertices_scratch_bytes(")
    assert hdr.rindex("\nint ursn_") == hdr.index("\nint ursn_cluster_vertices(")
    section = hdr.split("cluster cones: shower fragments")[1].split("ursn_cluster_vertices_scratch_bytes(")[0]
    for text in ("at most K links", "dist2 <= 127^2 = 16129", "dist2 << 32 | apex key", "hence m_total < 2^30", "|charge| <= 2^62",
                 "c_ax = fabs((u[0] * a0 + u[1] * a1) + u[2] * a2)", "consumer's judgement", "URSN_CLCONE_WAVE=0", "\"cluster_cones:\""):
        assert text in section, text
    with open(os.path.join(ROOT, "u-resnet_amd", "build.py")) as f:
        assert '"cluster_cone.hip"' in f.read()


def test_scratch_query(lib):
    """The domain only: at least 8 bytes, 8-byte granular, monotone in the list length, 0 outside; no layout is pinned."""
    q = lib.ursn_cluster_cones_scratch_bytes
    ms = (0, 1, 63, 64, 65, 2047, 2048, 2049, 8000, 10 ** 6, 2 ** 30 - 1)
    for n in (1, 5, 65535):
        sizes = [q(n, m) for m in ms]
        assert all(b >= 8 and b % 8 == 0 for b in sizes) and sizes == sorted(sizes) and sizes[0] < sizes[-1], (n, sizes)
    assert q(1, 1000) <= q(5, 1000) <= q(65535, 1000)
    for args in ((0, 10), (-1, 10), (65536, 10), (1, -1), (1, 2 ** 30), (1, 2 ** 40), (1, -2 ** 62)):
        assert q(*args) == 0, args


DESC = dict(ndim=3, n=2, reach=48, m_total=10, offsets=FAKE, index=FAKE + 0x1000, cluster=FAKE + 0x2000, table_offsets=FAKE + 0x3000,
            itab=FAKE + 0x5000, rtab=FAKE + 0x6000, feat_cap=10, cls=FAKE + 0x7000, min_cos=0.8, min_size=1, class_mask=6, same_class=1,
            seed_size=8)
OUT = dict(merged=FAKE + 0x10000, shower_offsets=FAKE + 0x11000, first=FAKE + 0x12000, size=FAKE + 0x13000, cls=FAKE + 0x14000,
           shower_itab=FAKE + 0x15000, shower_rtab=FAKE + 0x16000, cap_showers=10, link_offsets=FAKE + 0x17000, link_itab=FAKE + 0x18000,
           link_rtab=FAKE + 0x19000, cap_links=10, row_shower=FAKE + 0x1a000, row_parent=FAKE + 0x1b000, row_candidates=FAKE + 0x1c000,
           row_children=FAKE + 0x1d000, row_depth=FAKE + 0x1e000, cap_rows=10, event=FAKE + 0x1f000, status=FAKE + 0x20000)
SCRATCH = FAKE + 0x40000
ROW_KEYS = ("row_shower", "row_parent", "row_candidates", "row_children", "row_depth")


def _refused(lib, text, scratch=SCRATCH, sbytes=1 << 20, null=None, spatial=(7, 9, 11), out=None, **kw):
    d, o = _lib.ursn_cluster_cone_desc(), _lib.ursn_cluster_cone_out()
    for k, v in DESC.items():
        setattr(d, k, kw.pop(k, v))
    for i, s in enumerate(spatial):
        d.spatial[i] = s
    for k, v in dict(OUT, **(out or {})).items():
        setattr(o, k, v)
    assert not kw, kw
    rc = lib.ursn_cluster_cones(None if null == "desc" else ctypes.byref(d), None if null == "out" else ctypes.byref(o), _p(scratch),
                                sbytes, None)
    msg = lib.ursn_last_error()
    assert rc != 0 and msg.startswith(b"cluster_cones:") and text in msg, (rc, msg)


def test_cluster_cones_refusals(lib):
    """Null streams and fake device pointers: a call that got past its checks would fault here, not return."""
    who = b"cluster_cones"
    r = lambda text, **kw: _refused(lib, who + text, **kw)
    ro = lambda text, **out: _refused(lib, who + text, out=out)
    r(b": null desc / out", null="desc")
    r(b": null desc / out", null="out")
    r(b": n = 0 outside [1, 65535]", n=0)
    r(b": n = 65536 outside [1, 65535]", n=65536)
    r(b": m_total = -1 outside [0, 2^30)", m_total=-1)
    r(b": m_total = 1073741824 outside [0, 2^30)", m_total=2 ** 30)
    r(b": ndim = 1, expected 2 or 3", ndim=1)
    r(b": ndim = 4, expected 2 or 3", ndim=4)
    r(b": spatial[0] = 0 outside [1, 32768]", spatial=(0, 9, 11))
    r(b": spatial[1] = 32769 outside [1, 32768]", spatial=(7, 32769, 11))
    r(b": spatial[2] = -1 outside [1, 32768]", spatial=(7, 9, -1))
    r(b": 2147483648 voxels, expected fewer than 2^31", spatial=(2048, 1024, 1024))
    r(b": reach = 0 outside [1, 127]", reach=0)
    r(b": reach = 128 outside [1, 127]", reach=128)
    r(b": reach = -2147483648 outside [1, 127]", reach=-2 ** 31)
    r(b": min_cos = 0 outside (0, 1]", min_cos=0.0)
    r(b": min_cos = nan outside (0, 1]", min_cos=float("nan"))
    r(b": min_cos = -0.1 outside (0, 1]", min_cos=-0.1)
    r(b": min_cos = 1.5 outside (0, 1]", min_cos=1.5)
    r(b": min_cos = inf outside (0, 1]", min_cos=float("inf"))
    r(b": seed_size = 1 < 2", seed_size=1)
    r(b": seed_size = -7 < 2", seed_size=-7)
    r(b": min_size = 0 < 1", min_size=0)
    r(b": min_size = -5 < 1", min_size=-5)
    r(b": same_class = 2, expected 0 or 1", same_class=2)
    r(b": same_class = -1, expected 0 or 1", same_class=-1)
    r(b": feat_cap = -1 < 0", feat_cap=-1)
    ro(b": cap_rows = -1 < 0", cap_rows=-1)
    ro(b": cap_rows = -9223372036854775808 < 0", cap_rows=-2 ** 63)
    ro(b": cap_showers = -1 < 0", cap_showers=-1)
    ro(b": cap_links = -1 < 0", cap_links=-1)
    r(b": null offsets / table_offsets", offsets=None)
    r(b": null offsets / table_offsets", table_offsets=None)
    r(b": null index / cluster", index=None)
    r(b": null index / cluster", cluster=None)
    r(b": null itab / rtab", itab=None)
    r(b": null itab / rtab", rtab=None)
    r(b": class_mask = 0x6 needs cls", cls=None)
    r(b": same_class needs cls", cls=None, class_mask=0)
    ro(b": null out->status", status=None)
    for key in ("shower_offsets", "link_offsets", "event"):
        ro(b": null out->shower_offsets / out->link_offsets / out->event", **{key: None})
    ro(b": null out->merged", merged=None)
    for key in ("shower_itab", "shower_rtab", "first", "size", "cls"):
        ro(b": null out->shower_itab / out->shower_rtab / out->first / out->size / out->cls", **{key: None})
    for key in ("link_itab", "link_rtab"):
        ro(b": null out->link_itab / out->link_rtab", **{key: None})
    for key in ROW_KEYS:
        ro(b": null out->row_shower / out->row_parent / out->row_candidates / out->row_children / out->row_depth", **{key: None})
    r(b": null scratch", scratch=None)
    aligned8 = b": offsets / table_offsets / itab / rtab / the out tables / scratch must be 8-byte aligned"
    for key in ("offsets", "table_offsets", "itab", "rtab"):
        r(aligned8, **{key: DESC[key] + 4})
    for key in ("shower_offsets", "shower_itab", "shower_rtab", "link_offsets", "link_itab", "link_rtab", "event"):
        ro(aligned8, **{key: OUT[key] + 4})
    r(aligned8, scratch=SCRATCH + 4)
    aligned4 = b": index / cluster / merged / first / size / the row arrays / status must be 4-byte aligned"
    for key in ("index", "cluster"):
        r(aligned4, **{key: DESC[key] + 2})
    for key in ("merged", "first", "size") + ROW_KEYS:
        ro(aligned4, **{key: OUT[key] + 2})
    ro(aligned4, status=OUT["status"] + 1)
    need = lib.ursn_cluster_cones_scratch_bytes(2, 10)
    r(b": scratch of %d bytes is too small, %d needed" % (need - 8, need), sbytes=need - 8)
    # legal shapes of a call get as far as the scratch size: no cls; 2-D; the ends of the ranges; no rows / showers / links / records /
    # entries
    small = b": scratch of 0 bytes is too small"
    r(small, cls=None, class_mask=0, same_class=0, sbytes=0)
    r(small, cls=FAKE + 0x7001, class_mask=0xFFFFFFFF, sbytes=0)                                       # bytes: no alignment asked
    _refused(lib, who + small, out=dict(cls=OUT["cls"] + 1), sbytes=0)
    r(small, ndim=2, spatial=(32768, 32768, -5), sbytes=0)
    r(small, reach=1, min_cos=5e-324, min_size=1, seed_size=2, sbytes=0)
    r(small, reach=127, min_cos=1.0, min_size=2 ** 31 - 1, seed_size=2 ** 31 - 1, sbytes=0)
    _refused(lib, who + small, out=dict({k: None for k in ROW_KEYS}, cap_rows=0), sbytes=0)
    _refused(lib, who + small, out=dict(cap_showers=0, shower_itab=None, shower_rtab=None, first=None, size=None, cls=None), sbytes=0)
    _refused(lib, who + small, out=dict(cap_links=0, link_itab=None, link_rtab=None), sbytes=0)
    r(small, feat_cap=0, itab=None, rtab=None, sbytes=0)
    _refused(lib, who + small, out=dict(merged=None), m_total=0, index=None, cluster=None, sbytes=0)


def test_cluster_cone_spec_refusals():
    s = ClusterConeSpec()
    assert (s.reach, s.min_cos, s.seed_size, s.min_size, s.classes, s.same_class) == (48, 0.8, 8, 1, None, True) and s.class_mask() == 0
    assert repr(s) == "ClusterConeSpec(reach=48, min_cos=0.8, seed_size=8, min_size=1, classes=None, same_class=True)"
    s = ClusterConeSpec(127, 1, 2, 1, {1, 4}, False)
    assert (s.reach, s.min_cos, type(s.min_cos), sorted(s.classes), s.class_mask(), s.same_class) == (127, 1.0, float, [1, 4], 18, False)
    assert ClusterConeSpec(1, 1e-300, 2 ** 31 - 1, 2 ** 31 - 1, [0, 31]).class_mask() == 0x80000001
    for bad in (0, 128, -1, 48.0, True, "48", None):
        with pytest.raises(ValueError) as e:
            ClusterConeSpec(reach=bad)
        assert "reach" in str(e.value) and repr(bad) in str(e.value), str(e.value)
    for bad in (0, 0.0, -0.1, 1.5, float("nan"), float("inf"), True, "0.9", None):
        with pytest.raises(ValueError) as e:
            ClusterConeSpec(min_cos=bad)
        assert "min_cos" in str(e.value) and repr(bad) in str(e.value), str(e.value)
    for bad in (1, 0, -3, 2 ** 31, 8.0, True, "8", None):
        with pytest.raises(ValueError) as e:
            ClusterConeSpec(seed_size=bad)
        assert "seed_size" in str(e.value) and repr(bad) in str(e.value), str(e.value)
    for bad in (0, -3, 2 ** 31, 3.0, True, "3", None):
        with pytest.raises(ValueError) as e:
            ClusterConeSpec(min_size=bad)
        assert "min_size" in str(e.value) and repr(bad) in str(e.value), str(e.value)
    for bad in ((), [32], [-1], [1, 1], [1.0], ["1"], [True], 3):
        with pytest.raises(ValueError) as e:
            ClusterConeSpec(classes=bad)
        assert "classes" in str(e.value) and repr(bad) in str(e.value), str(e.value)
    for bad in (0, 1, None, "True"):
        with pytest.raises(ValueError) as e:
            ClusterConeSpec(same_class=bad)
        assert "same_class" in str(e.value) and repr(bad) in str(e.value), str(e.value)
    with pytest.raises(ValueError):
        cluster_cones_numpy([0, 0], [], None, [], [0, 0], (4, 4), 2)
    with pytest.raises(ValueError):
        cluster_cones_numpy([0, 0], [], None, [], [0, 0], (4, 4), ClusterConeSpec(classes=(1,), same_class=False))   # classes need cls
    with pytest.raises(ValueError):
        cluster_cones_numpy([0, 0], [], None, [], [0, 0], (4, 4), ClusterConeSpec())                                 # same_class too
    assert cluster_cones_numpy([0, 0], [], None, [], [0, 0], (4, 4), ClusterConeSpec(same_class=False))["events"].tolist() == [[0, 0, 0, -1]]


# ---- config keys, driver, Python surface ---------------------------------------------------------------------------------------
KEYS = ("ANA_CONES", "CONE_REACH", "CONE_MIN_COS", "CONE_SEED_SIZE", "CONE_MIN_SIZE", "CONE_CLASSES", "CONE_SAME_CLASS")


def test_config_keys_default_off_and_validated(tmp_path):
    c = ssnet_config()
    assert [getattr(c, k) for k in KEYS] == ["", 48, 0.8, 8, 1, [], True]
    out = io.StringIO()
    with redirect_stdout(out):
        c.dump()
    for key in KEYS:
        assert any(line.startswith(key + ".") or line.startswith(key + " ") for line in out.getvalue().split("\n")), key
    p = tmp_path / "a.cfg"
    p.write_text("ANA_CONES '/tmp/cones.csv'\nCONE_REACH 127\nCONE_MIN_COS 0.75\nCONE_SEED_SIZE 12\nCONE_MIN_SIZE 2\nCONE_CLASSES [1, 2]\n"
                 "CONE_SAME_CLASS False\n")
    with redirect_stdout(io.StringIO()):
        c.override(str(p))
    assert [getattr(c, k) for k in KEYS] == ["/tmp/cones.csv", 127, 0.75, 12, 2, [1, 2], False]
    assert [getattr(ssnet_config(), k) for k in KEYS] == ["", 48, 0.8, 8, 1, [], True]
    for text in ("ANA_CONES True\n", "ANA_CONES 1\n", "ANA_CONES ['a.csv']\n", "ANA_CONES None\n", "CONE_REACH 0\n", "CONE_REACH 128\n",
                 "CONE_REACH 48.0\n", "CONE_REACH '48'\n", "CONE_MIN_COS 0.0\n", "CONE_MIN_COS -0.1\n", "CONE_MIN_COS 1.5\n",
                 "CONE_MIN_COS '0.9'\n", "CONE_MIN_COS float('nan')\n", "CONE_SEED_SIZE 1\n", "CONE_SEED_SIZE 8.0\n", "CONE_MIN_SIZE 0\n",
                 "CONE_MIN_SIZE 3.0\n", "CONE_MIN_SIZE '3'\n", "CONE_CLASSES [32]\n", "CONE_CLASSES [1, 1]\n", "CONE_CLASSES [1.0]\n",
                 "CONE_CLASSES 1\n", "CONE_SAME_CLASS 1\n", "CONE_SAME_CLASS 'yes'\n"):
        bad = tmp_path / "b.cfg"
        bad.write_text(text)
        with redirect_stdout(io.StringIO()), pytest.raises(Exception) as e:
            ssnet_config().override(str(bad))
        assert isinstance(e.value, (TypeError, ValueError, SyntaxError, NameError)), (text, e.value)


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


def test_driver_refuses_ana_cones_without_ana_cluster(tmp_path):
    """Before a stream is opened or a device is touched; the file is not created."""
    csv = tmp_path / "cones.csv"
    for text in ("TRAIN False\nANA_CONES '%s'\n" % csv,
                 "TRAIN False\nSPARSE_IO True\nSPARSE_SCORES True\nCONE_REACH 12\nANA_CONES '%s'\n" % csv):
        with pytest.raises(ValueError) as e:
            _driver(tmp_path, text).initialize()
        assert "ANA_CONES" in str(e.value) and "ANA_CLUSTER" in str(e.value), str(e.value)
    assert not csv.exists()
    head = cones_csv_header()
    assert head.endswith("\n") and head[:-1].split(",") == ["entry", "shower"] + list(CONE_INT) + list(CONE_REAL)
    cols = {name: np.array([3 + c, -(7 + c)], np.int64) for c, name in enumerate(CONE_INT)}
    cols.update({name: np.array([0.5, 1.0 / 3.0 + c]) for c, name in enumerate(CONE_REAL)})
    cells = cones_csv_row(5, 1, cols)[:-1].split(",")
    assert cells[:18] == ["5", "1"] + [str(-(7 + c)) for c in range(16)]
    assert [float(x) for x in cells[18:]] == [1.0 / 3.0 + c for c in range(4)]
    assert len(chains_csv_header().split(",")) == 23                                  # the chains file is as it was


def test_set_cluster_cones_leaves_want_as_it_was():
    """construct(allocate=False) never touches a device."""
    net = uresnet(dims=[16, 16, 16, 1], num_class=3, base_num_outputs=4, num_strides=2)
    assert net._want_names() == ("scores", "pred", "ana")
    net.set_cluster_cones(ClusterConeSpec(12))
    assert net._want_names() == ("scores", "pred", "ana")
    net.set_clustering(ClusterSpec())
    assert net._want_names() == ("scores", "pred", "ana", "cluster")
    net.set_cluster_cones(None)
    for bad in (True, 1, 2.0, "2", ClusterSpec()):
        with pytest.raises(ValueError) as e:
            net.set_cluster_cones(bad)
        assert "set_cluster_cones" in str(e.value)
    with pytest.raises(ValueError) as e:
        net.cluster_cones(None, [np.arange(3)], None, {"cluster": [np.zeros(3)], "clusters": [{"first": np.zeros(1)}]}, 5)
    assert "cluster_cones" in str(e.value)


# ---- the statement: hand-built scenes ----------------------------------------------------------------------------------------------
def _run(name, spec=None, with_cls=True):
    shape, (off, index, ids, toff, tcls), at, own = cases.named(name)
    w = cluster_cones_numpy(off, index, None, ids, toff, shape, own if spec is None else spec, tcls if with_cls else None)
    _invariants(w, off, index, ids, toff, shape)
    return w, ids, toff, at


def _coords(index, shape):
    return tuple(int(c) for c in np.unravel_index(int(index), shape)) + (0,) * (3 - len(shape))


def _invariants(w, off, index, ids, toff, shape):
    """The clustering contract and the forest: every row in one shower, first strictly increasing, sizes adding up, a parent that
    outranks its child, depths along the links, the records of a link recomputed from the object records, cluster_features_numpy
    accepting the result."""
    K, soff, loff = int(toff[-1]), w["shower_offsets"], w["link_offsets"]
    sh, ln, f = w["showers"], w["links"], w["objects"]
    rs, rp, rd, rk = w["row_shower"], w["row_parent"], w["row_depth"], w["row_children"]
    assert sorted(sh) == sorted(CONE_INT + CONE_REAL) and sorted(ln) == sorted(LINK_INT + LINK_REAL)
    assert all(v.shape == (soff[-1],) for v in sh.values()) and all(v.shape == (loff[-1],) for v in ln.values())
    assert rs.shape == rp.shape == rd.shape == w["row_candidates"].shape == (K,) and rk.shape == (K, 2) and w["merged"].shape == ids.shape
    assert ((rp >= 0) == (w["row_candidates"] >= 1)).all() and loff[-1] <= K and loff[-1] == (rp >= 0).sum() == rk.sum()
    for e in range(len(off) - 1):
        k0, k1, s0, s1 = int(toff[e]), int(toff[e + 1]), int(soff[e]), int(soff[e + 1])
        rows = np.bincount(rs[k0:k1], minlength=s1 - s0)
        assert rs[k0:k1].min(initial=0) >= 0 and np.array_equal(rows, sh["rows"][s0:s1]) and (rows >= 1).all()
        mine, them = ids[off[e]:off[e + 1]], w["merged"][off[e]:off[e + 1]]
        assert ((mine < 0) == (them < 0)).all() and np.array_equal(them[mine >= 0], rs[k0:k1][mine[mine >= 0]])
        t = w["table"]
        assert (np.diff(t["first"][s0:s1]) > 0).all() and t["size"][s0:s1].sum() == (mine >= 0).sum()
        assert np.array_equal(np.bincount(them[them >= 0], minlength=s1 - s0), t["size"][s0:s1])
        for s in range(s0, s1):
            members = k0 + np.flatnonzero(rs[k0:k1] == s - s0)
            prim = k0 + int(sh["primary"][s])
            assert t["first"][s] == np.flatnonzero(them == s - s0)[0] and sh["n"][s] == t["size"][s] == f["n"][members].sum()
            assert sh["first_row"][s] == members[0] - k0 and rp[prim] == -1 and rd[prim] == 0 and prim in members
            assert (rp[members] == -1).sum() == 1 and sh["depth"][s] == rd[members].max() and sh["primary_n"][s] == f["n"][prim]
            assert sh["primary_fraction"][s] == float(f["n"][prim]) / float(sh["n"][s]) and sh["r_max"][s] == np.sqrt(float(sh["dist2_max"][s]))
            assert sh["start"][s] in (f["end_lo"][prim], f["end_hi"][prim])
            assert (sh["mask_flags"][s] >> 32 & 1) == int(rk[prim, 0] > 0 and rk[prim, 1] > 0)
            if members.size == 1:
                assert _bits(sh["min_cos"][s]) == _bits(sh["t_max"][s]) == 0 and sh["dist2_max"][s] == 0
        children = k0 + np.flatnonzero(rp[k0:k1] >= 0)
        assert np.array_equal(ln["child"][loff[e]:loff[e + 1]], children - k0)
        for j, c in zip(range(loff[e], loff[e + 1]), children):
            key = int(rp[c])
            p = k0 + (key >> 1)
            assert ln["apex"][j] == key and (f["n"][p] > f["n"][c] or (f["n"][p] == f["n"][c] and p < c)) and rd[c] == rd[p] + 1
            assert rs[c] == rs[p] == ln["shower"][j] and ln["depth"][j] == rd[c] and ln["pos"][j] == f["end_hi" if key & 1 else "end_lo"][p]
            d = [int(a) - b for a, b in zip(f["m"][c], _coords(index[ln["pos"][j]], shape))]
            assert ln["dist2"][j] == sum(x * x for x in d) >= 1 and ln["r"][j] == np.sqrt(float(ln["dist2"][j]))
            u = [np.float64(-x if key & 1 else x) for x in f["axis"][p]]
            tt, c_cone, _ = cone_link(u, None, d)
            assert _bits(tt) == _bits(ln["t"][j]) and _bits(c_cone) == _bits(ln["c_cone"][j]) and tt > 0 and c_cone > 0
            s = s0 + int(rs[c])
            assert sh["min_cos"][s] <= c_cone and sh["t_max"][s] >= tt and sh["dist2_max"][s] >= ln["dist2"][j]
        ev = w["events"][e]
        assert ev[0] == s1 - s0 and ev[1] == loff[e + 1] - loff[e] == (sh["rows"][s0:s1] - 1).sum() and ev[2] == (sh["rows"][s0:s1] >= 2).sum()
        if s1 > s0:
            pairs = list(zip(sh["rows"][s0:s1], sh["n"][s0:s1]))
            assert pairs.index(max(pairs)) == ev[3]
        else:
            assert ev[3] == -1
    # the result is a clustering: the object records of the showers
    g = cluster_features_numpy(off, index, None, w["merged"], soff, shape)
    assert np.array_equal(g["n"], sh["n"]) and np.array_equal(g["lo"], np.stack([sh["lo%d" % a] for a in range(3)], 1)) and \
        np.array_equal(g["hi"], np.stack([sh["hi%d" % a] for a in range(3)], 1))


def test_the_cone_boundary_the_box_and_the_ball():
    w, ids, toff, at = _run("boundary")
    stem, inside, wide, beyond, corner = (int(ids[at(0, p)]) for p in ((20, 10, 4), (23, 10, 8), (20, 14, 7), (20, 10, 17), (24, 13, 16)))
    f = w["objects"]
    key = 2 * stem + int(f["end_hi"][stem] == at(0, (20, 10, 4)))                # the apex at the stem's first voxel
    assert w["row_parent"].tolist() == [key if r == inside else -1 for r in range(5)] and w["row_candidates"][inside] == 1
    ln = w["links"]
    assert (ln["dist2"][0], ln["t"][0], ln["r"][0], ln["pos"][0]) == (25, 4.0, 5.0, at(0, (20, 10, 4)))
    assert _bits(ln["c_cone"][0]) == _bits(0.8) == _bits(np.float64(4.0) / np.float64(5.0)) and _bits(ln["c_ax"][0]) == 0
    assert _bits(w["showers"]["min_cos"][0]) == _bits(0.8) and w["showers"]["t_max"][0] == 4.0 and w["showers"]["rows"].tolist() == [2, 1, 1, 1]
    # one step of the last place up, and the voxel on the boundary is outside
    tight = _run("boundary", ClusterConeSpec(12, float(np.nextafter(0.8, 1.0)), 8, 1))[0]
    assert tight["link_offsets"].tolist() == [0, 0] and tight["shower_offsets"].tolist() == [0, 5]
    # cos 0.6 comes in at 0.6; 13 voxels along one axis come in at reach 13, and so does dist2 169
    assert _run("boundary", ClusterConeSpec(12, 0.6, 8, 1))[0]["row_parent"][wide] == key
    more = _run("boundary", ClusterConeSpec(13, 0.8, 8, 1))[0]
    assert more["row_parent"][beyond] == key and more["row_parent"][corner] == key and more["showers"]["dist2_max"][0] == 169
    assert w["row_candidates"][beyond] == 0 and w["row_candidates"][corner] == 0
    t, c, _ = cone_link([0.0, 0.0, 1.0], None, [4, 3, 12])
    assert c > 0.9 and 4 * 4 + 3 * 3 + 12 * 12 > 12 * 12                        # refused by the ball alone


def test_equal_distances_take_the_lower_key_and_equal_sizes_the_lower_row():
    w, ids, toff, at = _run("tie")
    a, b, c = (int(ids[at(0, p)]) for p in ((10, 10, 4), (10, 20, 4), (10, 15, 9)))
    f = w["objects"]
    ka, kb = (2 * r + int(f["end_hi"][r] == at(0, p)) for r, p in ((a, (10, 10, 4)), (b, (10, 20, 4))))
    assert a < b and w["row_candidates"][c] == 2 and w["row_parent"][c] == min(ka, kb) and w["links"]["dist2"].tolist() == [50]
    w, ids, toff, at = _run("rank")
    assert w["objects"]["n"].tolist() == [8, 8] and w["row_parent"][0] == -1 and w["row_parent"][1] >> 1 == 0 and w["row_depth"].tolist() == [0, 1]
    assert w["links"]["c_ax"].tolist() == [1.0] and w["links"]["t"].tolist() == [16.0] and w["showers"]["primary"].tolist() == [0]


def test_a_large_child_needs_its_axis_in_line():
    w = _run("misaligned")[0]
    assert w["link_offsets"].tolist() == [0, 0] and w["row_candidates"].tolist() == [0, 0]
    # the same bar below seed_size has no axis to speak of: the cone alone decides
    loose = _run("misaligned", cases.MISALIGNED_LOOSE)[0]
    assert loose["link_offsets"].tolist() == [0, 1] and loose["links"]["dist2"].tolist() == [196] and _bits(loose["links"]["c_ax"][0]) == 0
    t, c_cone, c_ax = cone_link([0.0, 0.0, 1.0], [0.0, 1.0, 0.0], [0, 0, 14])
    assert (t, c_cone, c_ax) == (14.0, 1.0, 0.0)
    assert _run("rank")[0]["link_offsets"].tolist() == [0, 1]                    # the same child aligned is accepted


def test_a_tree_of_depth_two_whose_first_row_is_not_its_primary():
    w, ids, toff, at = _run("tree")
    early, prim, mid, leaf = (int(ids[at(0, p)]) for p in ((18, 10, 14), (20, 10, 10), (20, 10, 24), (20, 10, 30)))
    assert (early, prim) == (0, 1) and w["shower_offsets"].tolist() == [0, 1] and w["row_depth"].tolist() == [1, 0, 1, 2]
    sh = w["showers"]
    assert (sh["rows"][0], sh["first_row"][0], sh["primary"][0], sh["depth"][0], sh["n"][0], sh["primary_n"][0]) == (4, 0, 1, 2, 16, 10)
    assert w["row_parent"][leaf] >> 1 == mid and w["row_parent"][mid] >> 1 == prim and w["row_parent"][early] >> 1 == prim
    assert w["row_children"][prim].sum() == 2 and w["row_children"][mid].sum() == 1 and sh["primary_fraction"][0] == 10.0 / 16.0
    assert w["table"]["first"].tolist() == [0] and w["table"]["size"].tolist() == [16] and sh["dist2_max"][0] == 256


def test_the_start_side_by_each_rule_in_turn():
    w, ids, toff, at = _run("sides")
    f, rk, sh = w["objects"], w["row_children"], w["showers"]
    used = set()
    for e in range(5):
        k0 = int(toff[e])
        prim = k0 + int(sh["primary"][e])
        kids = [[r for r in range(k0, int(toff[e + 1])) if w["row_parent"][r] == 2 * (prim - k0) + side] for side in (0, 1)]
        sums = [int(f["n"][k].sum()) for k in kids]
        assert sh["rows"][e] == toff[e + 1] - k0 and sh["mask_flags"][e] >> 32 == 1 and [len(k) for k in kids] == rk[prim].tolist()
        if sums[0] != sums[1]:
            rule, side = 1, int(sums[1] > sums[0])
        elif len(kids[0]) != len(kids[1]):
            rule, side = 2, int(len(kids[1]) > len(kids[0]))
        else:
            rule, side = 3, 0
        used.add((rule, side))
        assert sh["start"][e] == f["end_hi" if side else "end_lo"][prim], (e, rule, side)
    assert used == {(1, 0), (1, 1), (2, 0), (2, 1), (3, 0)}                     # every rule decided, towards either side
    # a primary that is no parent starts at its end_lo
    lone = _run("boundary")[0]
    assert lone["showers"]["start"][1:].tolist() == lone["objects"]["end_lo"][[1, 2, 4]].tolist()


def test_classes_and_same_class():
    w, ids, toff, at = _run("classes")
    stem, same, other = (int(ids[at(0, p)]) for p in ((20, 10, 4), (23, 10, 8), (20, 13, 8)))
    assert w["row_parent"][same] >= 0 and w["row_parent"][other] == -1 and w["showers"]["mask_flags"].tolist() == [2, 4]
    both = _run("classes", ClusterConeSpec(12, 0.8, 8, 1, None, False))[0]
    assert (both["row_parent"][[same, other]] >= 0).all() and both["showers"]["mask_flags"].tolist() == [6] and both["table"]["cls"].tolist() == [1]
    bare = _run("classes", ClusterConeSpec(12, 0.8, 8, 1, None, False), with_cls=False)[0]
    assert bare["link_offsets"].tolist() == [0, 2] and bare["showers"]["mask_flags"].tolist() == [0] and bare["table"]["cls"].tolist() == [0]
    only = _run("classes", ClusterConeSpec(12, 0.8, 8, 1, (1,), False))[0]
    assert only["row_parent"][same] >= 0 and only["row_parent"][other] == -1
    assert _run("classes", ClusterConeSpec(12, 0.8, 8, 1, (2,), False))[0]["link_offsets"].tolist() == [0, 0]
    assert _run("classes", ClusterConeSpec(12, 0.8, 8, 2, None, False))[0]["link_offsets"].tolist() == [0, 0]      # min_size
    assert _run("classes", ClusterConeSpec(12, 0.8, 9, 1, None, False))[0]["link_offsets"].tolist() == [0, 0]      # seed_size


def test_an_anchor_on_the_apex_an_empty_event_and_two_dimensions():
    w, ids, toff, at = _run("coincide")
    ring, stem = int(ids[at(0, (19, 9, 4))]), int(ids[at(0, (20, 10, 4))])
    f = w["objects"]
    assert f["m"][ring].tolist() == [20, 10, 4] and f["n"].tolist() == [8, 9] and (ring, stem) == (0, 1)
    far_key = 2 * stem + int(f["end_hi"][stem] == at(0, (20, 10, 12)))
    assert w["row_candidates"][ring] == 1 and w["row_parent"][ring] == far_key and w["links"]["dist2"].tolist() == [64]   # dist2 = 0: refused
    w, ids, toff, at = _run("empty_mid")
    assert toff.tolist() == [0, 5, 5, 8] and w["events"][1].tolist() == [0, 0, 0, -1] and w["shower_offsets"][1] == w["shower_offsets"][2]
    assert w["link_offsets"].tolist() == [0, 2, 2, 3] and w["links"]["child"].tolist()[2] == 1                            # event-local
    w, ids, toff, at = _run("flat")
    assert w["links"]["dist2"].tolist() == [25] and _bits(w["links"]["c_cone"][0]) == _bits(0.8) and w["links"]["pos"][0] == at(0, (10, 4))
    assert w["showers"]["lo2"].tolist() == [0, 0] and w["showers"]["hi2"].tolist() == [0, 0] and w["row_parent"][int(ids[at(0, (6, 7))])] == -1


def test_the_statement_raises_on_inconsistent_input(monkeypatch):
    from uresnet_amd import clusters
    shape, spec = (12, 10), ClusterConeSpec(6, 0.5, 2, 1)
    ok = dict(offsets=[0, 4], index=[1, 2, 35, 36], value=None, cluster=[0, 0, 1, 1], table_offsets=[0, 2], spatial=shape, spec=spec,
              cls=[1, 1])
    assert cluster_cones_numpy(**ok)["shower_offsets"].tolist() == [0, 1]   # (3, 5) from the first row's apex: cos 0.857
    for change in (dict(cluster=[0, 0, 2, 2]), dict(table_offsets=[0, 3], cls=[1, 2, 1]), dict(index=[1, 2, 35, 120]),
                   dict(index=[-1, 2, 35, 36]), dict(cls=[1, 32]), dict(cls=[1]), dict(spatial=(12, 10, 4, 4)), dict(offsets=[0, 2])):
        with pytest.raises(ValueError):
            cluster_cones_numpy(**dict(ok, **change))
    real = clusters.cluster_features_numpy

    def moved(*a, **kw):
        f = real(*a, **kw)
        f["end_hi"][0] = 2                                               # a member of the other row
        return f
    monkeypatch.setattr(clusters, "cluster_features_numpy", moved)
    with pytest.raises(ValueError) as e:
        cluster_cones_numpy(**ok)
    assert "not a member" in str(e.value)


# ---- the statement on the lists of the GPU test -------------------------------------------------------------------------------------
def test_every_named_scene_links_and_the_far_scene_takes_four_trips():
    """What tests/test_cluster_cone_gpu.py runs cannot pass on empty tables: every scene has a link at its own settings (the
    misaligned one at the settings the GPU test adds), and the far scene has links across more than 63 planes, towards both sides
    of one child, so that a wave striding the planes 64 at a time needs its first and its fourth trip."""
    with open(os.path.join(ROOT, "u-resnet_amd", "csrc", "cluster_cone.hip")) as f:
        src = f.read()
    const = {name: int(value) for name, value in re.findall(r"#define (CN_[A-Z_]+) (\d+)\b", src)}
    assert const["CN_PLANE_TRIPS"] == 4 == -(-(2 * CONE_MAX_REACH + 1) // 64) and "const int p = trip * 64 + lane;" in src
    for name in cases.SCENES:
        spec = cases.MISALIGNED_LOOSE if name == "misaligned" else None
        assert _run(name, spec)[0]["link_offsets"][-1] >= 1, name
    shape, (off, index, ids, toff, tcls), at, spec = cases.named("far")
    w = _run("far")[0]
    f, child = w["objects"], int(ids[at(0, (100, 8, 8))])
    assert spec.reach == 127 and w["row_candidates"][child] == 4
    planes = []                                                                 # of every apex the child accepts
    for r in range(int(toff[-1])):
        for side, pos in ((0, f["end_lo"][r]), (1, f["end_hi"][r])):
            if r == child or f["n"][r] < spec.seed_size:
                continue
            x = _coords(index[pos], shape)
            d = [int(a) - b for a, b in zip(f["m"][child], x)]
            u = [np.float64(-v if side else v) for v in f["axis"][r]]
            if cone_link(u, None, d)[1] >= spec.min_cos and sum(v * v for v in d) <= 127 ** 2:
                planes.append(x[0] - int(f["m"][child][0]))
    trips = sorted((p + spec.reach) // 64 for p in planes)
    assert sorted(planes) == [-80, -20, 17, 80] and trips == [0, 1, 2, 3] and min(planes) < -63 and max(planes) > 63
    d0 = [abs(int(f["m"][int(c)][0]) - _coords(index[p], shape)[0]) for c, p in zip(w["links"]["child"], w["links"]["pos"])]
    assert max(d0) > 63, d0


def test_the_lattice_case_crosses_the_one_step_thresholds():
    """The GPU test test_the_lattice_crosses_every_one_step_threshold runs 2,100 three-voxel stems, each with one voxel behind it,
    followed by 60,000 entries without a cluster.  With the constants of the source as they are now:"""
    with open(os.path.join(ROOT, "u-resnet_amd", "csrc", "cluster_cone.hip")) as f:
        src = f.read()
    const = {name: int(value) for name, value in re.findall(r"#define (CN_[A-Z_]+) (\d+)\b", src)}
    scan, wave_cap, grid_cap, tile = (const[k] for k in ("CN_SCAN_THREADS", "CN_WAVE_GRID_CAP", "CN_GRID_CAP", "CN_TILE"))
    assert "const int64_t first = WAVE ? (int64_t)blockIdx.x * 4 : (int64_t)blockIdx.x * 256" in src           # 4 child rows per workgroup
    assert "const int64_t N = mode == 0 ? a.tiles : cn_rows(a);" in src                                        # what the scans run over
    shape, index, ids, rows = cases.lattice()
    entries = index.size
    assert (rows, entries, (ids >= 0).sum()) == (4200, 68400, 8400)
    w = cluster_cones_numpy([0, entries], index, None, ids, [0, rows], shape, cases.LATTICE_SPEC)
    _invariants(w, np.array([0, entries]), index, ids, np.array([0, rows]), shape)
    assert w["events"].tolist() == [[2100, 2100, 2100, 0]] and (w["showers"]["rows"] == 2).all() and (w["links"]["dist2"] == 16).all()
    apexes = 2 * int((w["objects"]["n"] >= cases.LATTICE_SPEC.seed_size).sum())
    # the one-workgroup scans: tiles, rows (twice) -- each takes a second chunk, and the last threads take none; the apexes and the
    # links they count are more than one chunk's worth too
    tiles = -(-entries // tile)
    for items, per, busy in ((tiles, 2, 535), (rows, 5, 840)):
        assert items > scan and -(-items // scan) == per and -(-items // per) == busy < scan, (items, per, busy)
    assert apexes == 4200 > scan and w["link_offsets"][-1] == 2100 > scan and entries % tile == 48             # the last tile is ragged
    # the search: 4 rows per workgroup in the wave form: a second sweep
    sweep = 4 * wave_cap
    assert sweep < rows < 2 * sweep and -(-(rows - sweep) // 4) == 26 < wave_cap
    assert -(-rows // 256) == 17 < wave_cap                                                                    # the plain form: one sweep
    assert 1 < -(-entries // 256) == 268 < grid_cap


def test_showers_are_closer_to_the_truth_than_the_fragments():
    """Six toy events of two cone showers in (96, 64, 64): a 12-voxel stem and 25 fragments of 1 to 5 voxels inside an 18 degree
    half-angle each; reach 48, min_cos 0.7, seed_size 8, min_size 1.  In every event the adjusted Rand index against the two true
    showers is strictly greater for the showers than for the fragments.  Measured (seeds 1 to 6): 0.0587 -> 1.0, 0.0844 -> 0.7796,
    0.0836 -> 1.0, 0.0557 -> 1.0, 0.0550 -> 1.0, 0.0673 -> 1.0."""
    off, index, cluster, toff, tcls, truth, truth_toff = cases.toys()
    w = cluster_cones_numpy(off, index, None, cluster, toff, cases.TOY_SHAPE, cases.TOY_SPEC, tcls)
    _invariants(w, off, index, cluster, toff, cases.TOY_SHAPE)
    before = cluster_match_numpy(off, cluster, toff, truth, truth_toff)
    after = cluster_match_numpy(off, w["merged"], w["shower_offsets"], truth, truth_toff)
    assert len(off) - 1 == len(cases.TOY_SEEDS) == 6
    for e in range(6):
        print("seed %d: ARI %.6f -> %.6f" % (cases.TOY_SEEDS[e], before["event_real"][e, 0], after["event_real"][e, 0]))
        assert after["event_real"][e, 0] > before["event_real"][e, 0]
        assert toff[e + 1] - toff[e] >= 30 and w["events"][e][2] >= 2             # tens of fragments; both showers gathered
    # the two cones do not cross: no shower mixes the two truths
    for e in range(6):
        mine, them = w["merged"][off[e]:off[e + 1]], truth[off[e]:off[e + 1]]
        assert all(np.unique(them[mine == s]).size == 1 for s in np.unique(mine))
