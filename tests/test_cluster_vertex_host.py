"""Vertex candidates, host side (no GPU): the appended symbols under an unchanged ABI 9, the scratch query, every argument refusal of
ursn_cluster_vertices (include/uresnet_hip.h), ClusterVertexSpec, the ANA_VERTICES / VERTEX_* keys and the driver's refusal,
set_cluster_vertices, the arithmetic that puts the GPU test's lattice past the one-step thresholds of csrc/cluster_vertex.hip, and
the pure-Python statement (uresnet_amd.clusters.cluster_vertices_numpy): invariants and a coverage condition on random lists, and
hand-built shapes with hand-checked answers.  Every library call below is refused on its arguments before any device access, so the
fake pointers are never dereferenced."""
import ctypes
import io
import os
import re
from contextlib import redirect_stdout

import numpy as np
import pytest

import uresnet_amd  # noqa: F401
from uresnet_amd import _lib, clusters, ssnet_config, uresnet
from uresnet_amd.clusters import (VERTEX_EVENT, VERTEX_INCIDENCE, VERTEX_INT, VERTEX_REAL, ClusterSpec, ClusterVertexSpec, cluster_numpy,
                                  cluster_vertices_numpy)
from uresnet_amd.ssnet import objects_csv_header, vertices_csv_header, vertices_csv_row

FAKE = 0x10000
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _p(a):
    return ctypes.c_void_p(a)


def test_symbols_appended_under_abi_9(lib):
    assert _lib.ABI_VERSION == 9 and lib.ursn_abi_version() == 9
    with open(os.path.join(ROOT, "include", "uresnet_hip.h")) as f:
        hdr = f.read()
    for name in ("ursn_cluster_vertices_scratch_bytes", "ursn_cluster_vertices"):
        assert name in _lib.EXPORTS and hasattr(lib, name) and (name + "(") in hdr, name
    assert "#define URSN_ABI_VERSION 9" in hdr and "} ursn_cluster_vtx_desc;" in hdr and "} ursn_cluster_vtx_out;" in hdr
    for name in ("VI", "VR", "IN", "EV"):
        assert "#define URSN_CLVTX_%s %d " % (name, getattr(_lib, "CLVTX_" + name)) in hdr, name
    assert "#define URSN_CLVTX_INC_OVERFLOW %d " % _lib.CLVTX_INC_OVERFLOW in hdr
    assert (_lib.CLVTX_VI, _lib.CLVTX_VR, _lib.CLVTX_IN, _lib.CLVTX_EV) == \
        (len(VERTEX_INT), len(VERTEX_REAL), len(VERTEX_INCIDENCE), len(VERTEX_EVENT)) == (17, 5, 5, 4)
    assert ctypes.sizeof(_lib.ursn_cluster_vtx_desc) == 112 and ctypes.sizeof(_lib.ursn_cluster_vtx_out) == 88
    # the header ends with this section: nothing before it moved
    assert hdr.index("ursn_cluster_profile(") < hdr.index("ursn_cluster_vertices_scratch_bytes(")
    assert hdr.rindex("\nint ursn_") == hdr.index("\nint ursn_cluster_vertices(")
    section = hdr.split("vertex candidates")[1]
    for text in ("near < 2 K * 343", "|charge| <= 2^62", "|s| < 2^15 * 2^32", "dist2 <= 27", "consumer's judgement", "packed words fit"):
        assert text in section, text


def test_scratch_query(lib):
    """The domain only: at least 8 bytes, 8-byte granular, monotone in the list length and the incidence cap, 0 outside; no layout
    is pinned."""
    q = lib.ursn_cluster_vertices_scratch_bytes
    ms = (0, 1, 2047, 2048, 2049, 8000, 10 ** 6, 2 ** 30 - 1)
    for n in (1, 5, 65535):
        for inc in (0, 1, 10 ** 6, 2 ** 30 - 1):
            sizes = [q(n, m, inc) for m in ms]
            assert all(b >= 8 and b % 8 == 0 for b in sizes) and sizes == sorted(sizes) and sizes[0] < sizes[-1], (n, inc, sizes)
        by_cap = [q(n, 8000, inc) for inc in (0, 1, 100, 8000, 2 ** 20, 2 ** 30 - 1)]
        assert by_cap == sorted(by_cap) and by_cap[0] >= 8 and by_cap[0] < by_cap[-1], (n, by_cap)
    for args in ((0, 10, 1), (-1, 10, 1), (65536, 10, 1), (1, -1, 1), (1, 2 ** 30, 1), (1, 2 ** 40, 1), (1, 10, -1), (1, 10, 2 ** 30),
                 (1, 10, 2 ** 62)):
        assert q(*args) == 0, args


DESC = dict(ndim=3, n=2, radius=2, m_total=10, inc_cap=64, offsets=FAKE, index=FAKE + 0x1000, cluster=FAKE + 0x2000,
            table_offsets=FAKE + 0x3000, itab=FAKE + 0x5000, rtab=FAKE + 0x6000, feat_cap=10, cls=FAKE + 0x7000, min_size=3, class_mask=6)
OUT = dict(vertex_offsets=FAKE + 0x10000, vtx_itab=FAKE + 0x11000, vtx_rtab=FAKE + 0x12000, cap_vertices=20, inc_offsets=FAKE + 0x13000,
           incidence=FAKE + 0x14000, inc_out_cap=64, row_vertex=FAKE + 0x15000, cap_rows=10, event=FAKE + 0x16000, status=FAKE + 0x17000)
SCRATCH = FAKE + 0x40000


def _refused(lib, text, scratch=SCRATCH, sbytes=1 << 20, null=None, spatial=(7, 9, 11), **kw):
    d, o = _lib.ursn_cluster_vtx_desc(), _lib.ursn_cluster_vtx_out()
    for k, v in DESC.items():
        setattr(d, k, kw.pop(k, v))
    for i, s in enumerate(spatial):
        d.spatial[i] = s
    for k, v in OUT.items():
        setattr(o, k, kw.pop(k, v))
    assert not kw, kw
    rc = lib.ursn_cluster_vertices(None if null == "desc" else ctypes.byref(d), None if null == "out" else ctypes.byref(o), _p(scratch),
                                   sbytes, None)
    msg = lib.ursn_last_error()
    assert rc != 0 and msg.startswith(b"cluster_vertices:") and text in msg, (rc, msg)


def test_cluster_vertices_refusals(lib):
    """Null streams and fake device pointers: a call that got past its checks would fault here, not return."""
    who = b"cluster_vertices"
    r = lambda text, **kw: _refused(lib, who + text, **kw)
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
    r(b": radius = 0 outside [1, 3]", radius=0)
    r(b": radius = 4 outside [1, 3]", radius=4)
    r(b": radius = -2147483648 outside [1, 3]", radius=-2 ** 31)
    r(b": min_size = 0 < 1", min_size=0)
    r(b": min_size = -5 < 1", min_size=-5)
    r(b": inc_cap = -1 outside [0, 2^30)", inc_cap=-1)
    r(b": inc_cap = 1073741824 outside [0, 2^30)", inc_cap=2 ** 30)
    r(b": inc_cap = 9223372036854775807 outside [0, 2^30)", inc_cap=2 ** 63 - 1)
    r(b": feat_cap = -1 < 0", feat_cap=-1)
    r(b": cap_rows = -1 < 0", cap_rows=-1)
    r(b": cap_rows = -9223372036854775808 < 0", cap_rows=-2 ** 63)
    r(b": cap_vertices = -1 < 0", cap_vertices=-1)
    r(b": inc_out_cap = -1 < 0", inc_out_cap=-1)
    r(b": null offsets / table_offsets", offsets=None)
    r(b": null offsets / table_offsets", table_offsets=None)
    r(b": null index / cluster", index=None)
    r(b": null index / cluster", cluster=None)
    r(b": null itab / rtab", itab=None)
    r(b": null itab / rtab", rtab=None)
    r(b": class_mask = 0x6 needs cls", cls=None)
    r(b": null out->status", status=None)
    for key in ("vertex_offsets", "inc_offsets", "event"):
        r(b": null out->vertex_offsets / out->inc_offsets / out->event", **{key: None})
    r(b": null out->vtx_itab / out->vtx_rtab", vtx_itab=None)
    r(b": null out->vtx_itab / out->vtx_rtab", vtx_rtab=None)
    r(b": null out->incidence", incidence=None)
    r(b": null out->row_vertex", row_vertex=None)
    r(b": null scratch", scratch=None)
    for key in ("offsets", "table_offsets", "itab", "rtab"):
        r(b": offsets / table_offsets / itab / rtab / the out tables / scratch must be 8-byte aligned", **{key: DESC[key] + 4})
    for key in ("vertex_offsets", "vtx_itab", "vtx_rtab", "inc_offsets", "incidence", "event"):
        r(b": offsets / table_offsets / itab / rtab / the out tables / scratch must be 8-byte aligned", **{key: OUT[key] + 4})
    r(b": offsets / table_offsets / itab / rtab / the out tables / scratch must be 8-byte aligned", scratch=SCRATCH + 4)
    for key in ("index", "cluster"):
        r(b": index / cluster / row_vertex / status must be 4-byte aligned", **{key: DESC[key] + 2})
    r(b": index / cluster / row_vertex / status must be 4-byte aligned", row_vertex=OUT["row_vertex"] + 2)
    r(b": index / cluster / row_vertex / status must be 4-byte aligned", status=OUT["status"] + 1)
    need = lib.ursn_cluster_vertices_scratch_bytes(2, 10, 64)
    r(b": scratch of %d bytes is too small, %d needed" % (need - 8, need), sbytes=need - 8)
    # legal shapes of a call get as far as the scratch size: no cls; 2-D; the ends of the ranges; no rows / vertices / incidences /
    # records / entries
    r(b": scratch of 0 bytes is too small", cls=None, class_mask=0, sbytes=0)
    r(b": scratch of 0 bytes is too small", cls=FAKE + 0x7001, class_mask=0xFFFFFFFF, sbytes=0)       # bytes: no alignment asked
    r(b": scratch of 0 bytes is too small", ndim=2, spatial=(32768, 32768, -5), sbytes=0)
    r(b": scratch of 0 bytes is too small", radius=1, min_size=1, sbytes=0)
    r(b": scratch of 0 bytes is too small", radius=3, min_size=2 ** 31 - 1, sbytes=0)
    r(b": scratch of 0 bytes is too small", cap_rows=0, row_vertex=None, sbytes=0)
    r(b": scratch of 0 bytes is too small", cap_vertices=0, vtx_itab=None, vtx_rtab=None, sbytes=0)
    r(b": scratch of 0 bytes is too small", inc_out_cap=0, incidence=None, sbytes=0)
    r(b": scratch of 0 bytes is too small", inc_cap=0, sbytes=0)
    r(b": scratch of 0 bytes is too small", feat_cap=0, itab=None, rtab=None, sbytes=0)
    r(b": scratch of 0 bytes is too small", m_total=0, index=None, cluster=None, sbytes=0)


def test_cluster_vertex_spec_refusals():
    s = ClusterVertexSpec()
    assert (s.radius, s.min_size, s.classes) == (2, 3, None) and s.class_mask() == 0
    assert repr(s) == "ClusterVertexSpec(radius=2, min_size=3, classes=None)"
    s = ClusterVertexSpec(3, 1, {1, 4})
    assert (s.radius, s.min_size, sorted(s.classes), s.class_mask()) == (3, 1, [1, 4], 18)
    assert ClusterVertexSpec(1, 2 ** 31 - 1, [0, 31]).class_mask() == 0x80000001
    for bad in (0, 4, -1, 2.0, True, "2", None):
        with pytest.raises(ValueError) as e:
            ClusterVertexSpec(radius=bad)
        assert "radius" in str(e.value) and repr(bad) in str(e.value), str(e.value)
    for bad in (0, -3, 2 ** 31, 3.0, True, "3", None):
        with pytest.raises(ValueError) as e:
            ClusterVertexSpec(min_size=bad)
        assert "min_size" in str(e.value) and repr(bad) in str(e.value), str(e.value)
    for bad in ((), [32], [-1], [1, 1], [1.0], ["1"], [True], 3):
        with pytest.raises(ValueError) as e:
            ClusterVertexSpec(classes=bad)
        assert "classes" in str(e.value) and repr(bad) in str(e.value), str(e.value)
    with pytest.raises(ValueError):
        cluster_vertices_numpy([0, 0], [], None, [], [0, 0], (4, 4), 2)
    with pytest.raises(ValueError):
        cluster_vertices_numpy([0, 0], [], None, [], [0, 0], (4, 4), ClusterVertexSpec(classes=(1,)))     # classes need cls


# ---- config keys, driver, Python surface ---------------------------------------------------------------------------------------
def test_config_keys_default_off_and_validated(tmp_path):
    c = ssnet_config()
    assert c.ANA_VERTICES == "" and c.VERTEX_RADIUS == 2 and c.VERTEX_MIN_SIZE == 3 and c.VERTEX_CLASSES == []
    out = io.StringIO()
    with redirect_stdout(out):
        c.dump()
    for key in ("ANA_VERTICES", "VERTEX_RADIUS", "VERTEX_MIN_SIZE", "VERTEX_CLASSES"):
        assert any(line.startswith(key + ".") or line.startswith(key + " ") for line in out.getvalue().split("\n")), key
    p = tmp_path / "a.cfg"
    p.write_text("ANA_VERTICES '/tmp/vertices.csv'\nVERTEX_RADIUS 3\nVERTEX_MIN_SIZE 5\nVERTEX_CLASSES [1, 2]\n")
    with redirect_stdout(io.StringIO()):
        c.override(str(p))
    assert (c.ANA_VERTICES, c.VERTEX_RADIUS, c.VERTEX_MIN_SIZE, c.VERTEX_CLASSES) == ("/tmp/vertices.csv", 3, 5, [1, 2])
    fresh = ssnet_config()
    assert (fresh.ANA_VERTICES, fresh.VERTEX_RADIUS, fresh.VERTEX_MIN_SIZE, fresh.VERTEX_CLASSES) == ("", 2, 3, [])
    for text in ("ANA_VERTICES True\n", "ANA_VERTICES 1\n", "ANA_VERTICES ['a.csv']\n", "ANA_VERTICES None\n", "VERTEX_RADIUS 0\n",
                 "VERTEX_RADIUS 4\n", "VERTEX_RADIUS 2.0\n", "VERTEX_RADIUS '2'\n", "VERTEX_MIN_SIZE 0\n", "VERTEX_MIN_SIZE 3.0\n",
                 "VERTEX_MIN_SIZE '3'\n", "VERTEX_CLASSES [32]\n", "VERTEX_CLASSES [1, 1]\n", "VERTEX_CLASSES [1.0]\n",
                 "VERTEX_CLASSES 1\n"):
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


def test_driver_refuses_ana_vertices_without_ana_cluster(tmp_path):
    """Before a stream is opened or a device is touched; the file is not created."""
    csv = tmp_path / "vertices.csv"
    for text in ("TRAIN False\nANA_VERTICES '%s'\n" % csv,
                 "TRAIN False\nSPARSE_IO True\nSPARSE_SCORES True\nVERTEX_RADIUS 3\nANA_VERTICES '%s'\n" % csv):
        with pytest.raises(ValueError) as e:
            _driver(tmp_path, text).initialize()
        assert "ANA_VERTICES" in str(e.value) and "ANA_CLUSTER" in str(e.value), str(e.value)
    assert not csv.exists()
    head = vertices_csv_header()
    assert head.endswith("\n") and head[:-1].split(",") == ["entry", "vertex"] + list(VERTEX_INT) + list(VERTEX_REAL)
    cols = {name: np.array([3 + c, -(7 + c)], np.int64) for c, name in enumerate(VERTEX_INT)}
    cols.update({name: np.array([0.5, 1.0 / 3.0 + c]) for c, name in enumerate(VERTEX_REAL)})
    line = vertices_csv_row(5, 1, cols)
    cells = line[:-1].split(",")
    assert cells[:19] == ["5", "1"] + [str(-(7 + c)) for c in range(17)]
    assert [float(x) for x in cells[19:]] == [1.0 / 3.0 + c for c in range(5)]
    assert len(objects_csv_header().split(",")) == 21                                 # the objects file is as it was


def test_set_cluster_vertices_leaves_want_as_it_was():
    """construct(allocate=False) never touches a device."""
    net = uresnet(dims=[16, 16, 16, 1], num_class=3, base_num_outputs=4, num_strides=2)
    assert net._want_names() == ("scores", "pred", "ana")
    net.set_cluster_vertices(ClusterVertexSpec(3))
    assert net._want_names() == ("scores", "pred", "ana")
    net.set_clustering(ClusterSpec())
    assert net._want_names() == ("scores", "pred", "ana", "cluster")
    net.set_cluster_vertices(None)
    for bad in (True, 1, 2.0, "2", ClusterSpec()):
        with pytest.raises(ValueError) as e:
            net.set_cluster_vertices(bad)
        assert "set_cluster_vertices" in str(e.value)
    assert net._vertex_inc_cap(0) == 1024 and net._vertex_inc_cap(1000) == 5024 and net._vertex_inc_cap(2 ** 40) == 2 ** 30 - 1


def test_the_lattice_case_crosses_the_one_step_thresholds():
    """The GPU test test_more_keys_than_one_step_of_the_scan_and_one_sweep_of_the_walk runs 2,100 two-voxel clusters.  With the
    constants of the source as they are now: 4,200 keys and 4,200 vertices."""
    with open(os.path.join(ROOT, "u-resnet_amd", "csrc", "cluster_vertex.hip")) as f:
        src = f.read()
    const = {name: int(value) for name, value in re.findall(r"#define (VX_[A-Z_]+) (\d+)\b", src)}
    scan, wave_cap, grid_cap, dirs = const["VX_SCAN_THREADS"], const["VX_WAVE_GRID_CAP"], const["VX_GRID_CAP"], const["VX_DIRS"]
    assert dirs == clusters.VERTEX_MAX_DIRECTIONS == 16
    assert "vx_first_key() { return WAVE ? (int64_t)blockIdx.x * 4 : (int64_t)blockIdx.x * 256; }" in src     # 4 end points per workgroup
    rows = 2100
    keys = vertices = 2 * rows
    per = -(-keys // scan)                        # the chunk of one scan thread
    assert keys > scan and per == 5 and keys % per == 0 and keys // per == 840 < scan        # 840 threads take 5, the others none
    sweep = 4 * wave_cap                           # keys one sweep of the wave form covers
    assert sweep < keys < 2 * sweep and (keys - sweep) % 4 == 0 and (keys - sweep) // 4 == 26 < wave_cap   # the second sweep: 26 workgroups
    assert keys > 256 and -(-keys // 256) == 17 < wave_cap                                   # the plain form: 17 workgroups, one sweep
    assert vertices > 256 and -(-vertices // 64) == 66 and -(-vertices // 256) == 17 < grid_cap   # the vertex kernel runs 64 threads
    assert "dim3(vx_grid(keys, 64, VX_GRID_CAP)), dim3(64)" in src


# ---- the statement ---------------------------------------------------------------------------------------------------------------
def _ids(off, index, cls, shape, spec):
    ids, counts, tcls = [], [], []
    for e in range(len(off) - 1):
        c, first, _, k = cluster_numpy(index[off[e]:off[e + 1]], cls[off[e]:off[e + 1]], shape, spec)
        ids.append(c), counts.append(first.size), tcls.append(k)
    return np.concatenate(ids), np.concatenate([[0], np.cumsum(counts)]).astype(np.int64), np.concatenate(tcls)


_made = {}


def _case(shape, same_class):
    """The lists of tests/test_cluster_vertex_gpu.py's random case (default_rng(len(shape)): 3 in 3-D), made the same way."""
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
        _made[key] = (off, index, value, cluster, toff, tcls)
    return _made[key]


def test_the_random_case_covers_every_kind_of_record():
    """The coverage condition of the GPU test's random lists, on the statement: it cannot pass on empty tables.  The statement's own
    counts: 3-D, radius 2, min_size 3: 73 vertices, 16 with two or more ends, 180 body incidences, 8 incidences of kind 3; radius 3:
    a vertex with 50 ends; 2-D, radius 2, min_size 3: 17 vertices, 3 with two ends, 12 body incidences."""
    off, index, value, cluster, toff, tcls = _case((16, 16, 16), False)
    w = cluster_vertices_numpy(off, index, value, cluster, toff, (16, 16, 16), ClusterVertexSpec(2, 3), tcls)
    v, inc = w["vertices"], w["incidence"]
    counts = (v["ends"].size, int((v["ends"] >= 2).sum()), int((inc[:, 1] == 0).sum()), int((inc[:, 1] == 3).sum()))
    assert counts == (73, 16, 180, 8)
    assert counts[1] >= 10 and counts[2] >= 100 and counts[3] >= 1
    w3 = cluster_vertices_numpy(off, index, value, cluster, toff, (16, 16, 16), ClusterVertexSpec(3, 3), tcls)["vertices"]
    assert w3["ends"].max() == 50 > 16 and (w3["mask_flags"][w3["ends"] > 16] >> 32 & 1).all()
    assert not (w3["mask_flags"][w3["ends"] <= 16] >> 32 & 1).any()
    off, index, value, cluster, toff, tcls = _case((12, 10), False)
    w = cluster_vertices_numpy(off, index, value, cluster, toff, (12, 10), ClusterVertexSpec(2, 3), tcls)
    two, bodies = int((w["vertices"]["ends"] == 2).sum()), int((w["incidence"][:, 1] == 0).sum())
    assert (w["vertices"]["ends"].size, two, bodies) == (17, 3, 12) and two >= 2 and bodies >= 5
    # under the joined spec nothing within distance 1 is another cluster: radius 1 finds its links under the by-class spec
    off, index, value, cluster, toff, tcls = _case((16, 16, 16), True)
    w1 = cluster_vertices_numpy(off, index, value, cluster, toff, (16, 16, 16), ClusterVertexSpec(1, 3), tcls)
    assert (w1["vertices"]["ends"] >= 2).sum() >= 5 and (w1["incidence"][:, 1] == 0).sum() >= 20


@pytest.mark.parametrize("shape,radius,min_size,same_class", [((16, 16, 16), 2, 3, False), ((16, 16, 16), 1, 1, True),
                                                               ((16, 16, 16), 3, 2, True), ((12, 10), 2, 1, False), ((12, 10), 3, 3, True)])
def test_statement_invariants(shape, radius, min_size, same_class):
    off, index, value, cluster, toff, tcls = _case(shape, same_class)
    w = cluster_vertices_numpy(off, index, value, cluster, toff, shape, ClusterVertexSpec(radius, min_size), tcls)
    f, v, inc, ioff, voff, rv = w["objects"], w["vertices"], w["incidence"], w["inc_offsets"], w["vertex_offsets"], w["row_vertex"]
    K, V = int(toff[-1]), int(voff[-1])
    assert sorted(v) == sorted(VERTEX_INT + VERTEX_REAL) and all(x.shape == (V,) for x in v.values()) and V > 3
    assert ioff.shape == (V + 1,) and ioff[0] == 0 and inc.shape == (ioff[-1], 5) and rv.shape == (K, 2) and rv.dtype == np.int32
    assert np.array_equal(np.diff(ioff), v["rows"]) and np.array_equal(w["events"][:, 0], np.diff(voff))
    eligible = f["n"] >= min_size
    assert ((rv >= 0).all(axis=1) == eligible).all() and ((rv == -1).all(axis=1) == ~eligible).all()
    single = f["end_lo"] == f["end_hi"]
    assert (rv[single & eligible, 0] == rv[single & eligible, 1]).all()
    ends_seen = np.zeros(V, np.int64)
    for e in range(len(off) - 1):
        for r in range(toff[e], toff[e + 1]):
            if eligible[r]:
                for side in range(1 if single[r] else 2):               # every end belongs to exactly one vertex of its event
                    assert 0 <= rv[r, side] < voff[e + 1] - voff[e]
                    ends_seen[voff[e] + rv[r, side]] += 1
        for g in range(voff[e], voff[e + 1]):
            rows = inc[ioff[g]:ioff[g + 1]]
            assert (np.diff(rows[:, 0]) > 0).all() and (rows[:, 0] < toff[e + 1] - toff[e]).all() and (rows[:, 2] >= 1).all()
            assert (rows[:, 3] <= (27 if len(shape) == 3 else 18)).all()
            for local, kind, near, dist2, pos in rows:                   # row_vertex agrees with the incidences' kind
                r = toff[e] + local
                mine = {0: rv[r, 0] == g - voff[e], 1: rv[r, 1] == g - voff[e] and not single[r]}
                assert kind == (1 if mine[0] else 0) + (2 if mine[1] else 0), (g, r, kind, rv[r])
                assert off[e] <= pos < off[e + 1] and cluster[pos] == local and (dist2 == 0) == (kind != 0)
            with_ends = int((rows[:, 1] != 0).sum())
            assert v["rows"][g] == with_ends + v["bodies"][g] and v["bodies"][g] == (rows[:, 1] == 0).sum()
            assert v["ends"][g] == (rows[:, 1] & 1).sum() + (rows[:, 1] >> 1).sum() and v["near"][g] == rows[:, 2].sum()
            assert v["n"][g] == f["n"][toff[e] + rows[:, 0]].sum() and v["charge"][g] == f["charge"][toff[e] + rows[:, 0]].sum()
            assert v["mask_flags"][g] & 0xFFFFFFFF == np.bitwise_or.reduce(1 << tcls[toff[e] + rows[:, 0]].astype(np.int64))
            for a in range(3):
                assert v["lo%d" % a][g] * v["ends"][g] <= v["s%d" % a][g] <= v["hi%d" % a][g] * v["ends"][g]
                assert v["c%d" % a][g] == v["s%d" % a][g] / v["ends"][g]
            assert -1.0 - 1e-12 <= v["min_cos"][g] <= v["max_cos"][g] <= 1.0 + 1e-12
            if v["ends"][g] < 2:
                assert _bits(v["min_cos"][g]) == _bits(v["max_cos"][g]) == 0     # +0.0
        ev = w["events"][e]
        sl = slice(voff[e], voff[e + 1])
        junction = (v["ends"][sl] >= 2) | (v["bodies"][sl] >= 1)
        assert ev[1] == junction.sum() and ev[2] == (~junction).sum() and ev[1] + ev[2] == ev[0]
        if ev[0]:
            best = max(zip(v["rows"][sl], v["n"][sl]))
            assert (v["rows"][sl][ev[3]], v["n"][sl][ev[3]]) == best and list(zip(v["rows"][sl], v["n"][sl])).index(best) == ev[3]
        else:
            assert ev[3] == -1
    assert np.array_equal(ends_seen, v["ends"])


def _bits(x):
    return int(np.float64(x).view(np.uint64))


def test_the_statement_is_symmetric_under_event_order():
    shape = (16, 16, 16)
    off, index, value, cluster, toff, tcls = _case(shape, True)
    spec = ClusterVertexSpec(2, 2, (1,))
    w = cluster_vertices_numpy(off, index, value, cluster, toff, shape, spec, tcls)
    order = [3, 2, 1, 0]
    pick = lambda a, o: np.concatenate([a[o[e]:o[e + 1]] for e in order])
    off2 = np.concatenate([[0], np.cumsum([off[e + 1] - off[e] for e in order])])
    toff2 = np.concatenate([[0], np.cumsum([toff[e + 1] - toff[e] for e in order])])
    w2 = cluster_vertices_numpy(off2, pick(index, off), pick(value, off), pick(cluster, off), toff2, shape, spec, pick(tcls, toff))
    for new, old in enumerate(order):
        a, b = slice(w["vertex_offsets"][old], w["vertex_offsets"][old + 1]), slice(w2["vertex_offsets"][new], w2["vertex_offsets"][new + 1])
        shift = off2[new] - off[old]
        for name in VERTEX_INT + VERTEX_REAL:
            moved = shift if name == "first_pos" else 0
            assert np.array_equal((w["vertices"][name][a] + moved).view(np.uint64), w2["vertices"][name][b].view(np.uint64)), (old, name)
        ia = w["incidence"][w["inc_offsets"][a.start]:w["inc_offsets"][a.stop]]
        ib = w2["incidence"][w2["inc_offsets"][b.start]:w2["inc_offsets"][b.stop]]
        assert np.array_equal(ia + [0, 0, 0, 0, shift], ib) and np.array_equal(w["events"][old], w2["events"][new])
        assert np.array_equal(w["row_vertex"][toff[old]:toff[old + 1]], w2["row_vertex"][toff2[new]:toff2[new + 1]])


def _scene(shape, events, spec):
    """``events``: per event a list of (points, class).  The lists sorted by index, clustered by cluster_numpy under ``spec``.
    Returns the statement's arguments and ``at(event, point)`` = the global list position of a point."""
    off, index, cls, where = [0], [], [], {}
    for e, segs in enumerate(events):
        pts = [(tuple(p), c) for points, c in segs for p in points]
        flat = np.array([np.ravel_multi_index(p, shape) for p, _ in pts], np.int64)
        order = np.argsort(flat)
        for k, o in enumerate(order):
            where[(e, pts[o][0])] = off[-1] + k
        index.append(flat[order]), cls.append(np.array([pts[o][1] for o in order], np.uint8))
        off.append(off[-1] + flat.size)
    off, index, cls = np.array(off), np.concatenate(index), np.concatenate(cls)
    ids, toff, tcls = _ids(off, index, cls, shape, spec)
    return (off, index, None, ids, toff, shape), tcls, ids, toff, lambda e, p: where[(e, tuple(p))]


def _vertex_of(w, ids, toff, at, e, p, side):
    """The global vertex of the end of the given side of the row the point belongs to."""
    r = toff[e] + ids[at(e, p)]
    assert w["objects"]["end_hi" if side else "end_lo"][r] == at(e, p)
    return int(w["vertex_offsets"][e] + w["row_vertex"][r][side])


def test_a_y_vertex_has_three_ends_at_right_angles():
    shape = (16, 16, 16)
    arms = [([(6 + k, 5, 5) for k in range(5)], 1), ([(5, 6 + k, 5) for k in range(5)], 2), ([(5, 5, 6 + k) for k in range(5)], 3)]
    args, tcls, ids, toff, at = _scene(shape, [arms], ClusterSpec(26, (1, 2, 3), True))
    assert toff.tolist() == [0, 3]
    w = cluster_vertices_numpy(*args, ClusterVertexSpec(1, 3), tcls)
    v = w["vertices"]
    assert w["vertex_offsets"].tolist() == [0, 4] and sorted(v["ends"]) == [1, 1, 1, 3]
    y = _vertex_of(w, ids, toff, at, 0, (6, 5, 5), 0)
    assert y == _vertex_of(w, ids, toff, at, 0, (5, 6, 5), 0) == _vertex_of(w, ids, toff, at, 0, (5, 5, 6), 0)
    assert (v["ends"][y], v["rows"][y], v["bodies"][y], v["n"][y]) == (3, 3, 0, 15)
    assert v["min_cos"][y] == 0.0 and v["max_cos"][y] == 0.0
    assert (v["s0"][y], v["s1"][y], v["s2"][y]) == (16, 16, 16) and v["c0"][y] == 16.0 / 3.0
    assert (v["lo0"][y], v["hi0"][y]) == (5, 6) and v["mask_flags"][y] == 0b1110
    inc = w["incidence"][w["inc_offsets"][y]:w["inc_offsets"][y + 1]]
    assert inc[:, 1].tolist() == [1, 1, 1] and inc[:, 3].tolist() == [0, 0, 0] and inc[:, 2].tolist() == [4, 4, 4]
    assert w["events"].tolist() == [[4, 1, 3, y]]                       # the junction is the primary vertex


def test_a_broken_track_has_two_ends_back_to_back():
    shape = (16, 16, 16)
    segs = [([(4, 4, c) for c in range(1, 6)], 1), ([(4, 4, c) for c in range(8, 13)], 1)]
    args, tcls, ids, toff, at = _scene(shape, [segs], ClusterSpec(26, (1,), False))
    assert toff.tolist() == [0, 2]
    assert cluster_vertices_numpy(*args, ClusterVertexSpec(2, 3), tcls)["vertex_offsets"].tolist() == [0, 4]     # a hole of two: 3 apart
    w = cluster_vertices_numpy(*args, ClusterVertexSpec(3, 3), tcls)
    v = w["vertices"]
    assert w["vertex_offsets"].tolist() == [0, 3]
    g = _vertex_of(w, ids, toff, at, 0, (4, 4, 5), 1)
    assert g == _vertex_of(w, ids, toff, at, 0, (4, 4, 8), 0)
    assert (v["ends"][g], v["bodies"][g], v["rows"][g]) == (2, 0, 2)
    assert v["min_cos"][g] == -1.0 and v["max_cos"][g] == -1.0          # exactly: a straight axis-parallel segment has a unit axis
    assert (v["c0"][g], v["c1"][g], v["c2"][g]) == (4.0, 4.0, 6.5) and v["first_pos"][g] == at(0, (4, 4, 5))
    inc = w["incidence"][w["inc_offsets"][g]:w["inc_offsets"][g + 1]]
    assert inc.tolist() == [[0, 2, 5, 0, at(0, (4, 4, 5))], [1, 1, 5, 0, at(0, (4, 4, 8))]]   # 4 of its own row and 1 of the other


def test_a_t_junction_is_one_end_on_a_body():
    shape = (16, 16, 16)
    segs = [([(4, 4, c) for c in range(11)], 1), ([(4, b, 5) for b in (6, 7, 8)], 2)]
    args, tcls, ids, toff, at = _scene(shape, [segs], ClusterSpec(26, (1, 2), True))
    w = cluster_vertices_numpy(*args, ClusterVertexSpec(2, 3), tcls)
    v = w["vertices"]
    g = _vertex_of(w, ids, toff, at, 0, (4, 6, 5), 0)
    assert (v["ends"][g], v["bodies"][g], v["rows"][g], v["n"][g]) == (1, 1, 2, 14)
    assert _bits(v["min_cos"][g]) == 0 and _bits(v["max_cos"][g]) == 0
    inc = w["incidence"][w["inc_offsets"][g]:w["inc_offsets"][g + 1]]
    long_row, short_row = ids[at(0, (4, 4, 0))], ids[at(0, (4, 6, 5))]
    assert inc[inc[:, 0] == long_row].tolist() == [[long_row, 0, 5, 4, at(0, (4, 4, 5))]]      # (4, 4, 3..7); the closest is 2 away
    assert inc[inc[:, 0] == short_row].tolist() == [[short_row, 1, 3, 0, at(0, (4, 6, 5))]]
    assert w["events"][0].tolist()[:3] == [4, 1, 3] and w["events"][0][3] == g


def test_both_ends_of_one_row_in_one_vertex_are_kind_3():
    shape = (16, 16, 16)
    segs = [([(4, b, 4) for b in (3, 4, 5)], 1), ([(4, 4, c) for c in (6, 7, 8)], 2)]
    args, tcls, ids, toff, at = _scene(shape, [segs], ClusterSpec(26, (1, 2), True))
    w = cluster_vertices_numpy(*args, ClusterVertexSpec(2, 3), tcls)
    v = w["vertices"]
    g = _vertex_of(w, ids, toff, at, 0, (4, 4, 6), 0)
    assert g == _vertex_of(w, ids, toff, at, 0, (4, 3, 4), 0) == _vertex_of(w, ids, toff, at, 0, (4, 5, 4), 1)
    assert v["ends"][g] == 3 and v["bodies"][g] == 0 and w["vertex_offsets"].tolist() == [0, 2]
    inc = w["incidence"][w["inc_offsets"][g]:w["inc_offsets"][g + 1]]
    bent = ids[at(0, (4, 3, 4))]
    assert inc[inc[:, 0] == bent][0].tolist()[:2] == [bent, 3] and inc[inc[:, 0] != bent][0][1] == 1
    assert inc[inc[:, 0] == bent][0][4] == at(0, (4, 3, 4))              # dist2 0 at both ends: the lower position
    assert v["min_cos"][g] == -1.0 and _bits(v["max_cos"][g]) in (0, 1 << 63)     # its two ends face each other; the third is square


def test_no_link_across_a_row_end_or_an_event_boundary():
    shape = (12, 10)
    segs = [([(3, 7), (3, 8), (3, 9)], 1), ([(4, 0), (4, 1), (4, 2)], 1)]
    args, tcls, ids, toff, at = _scene(shape, [segs, segs], ClusterSpec(8, (1,), False))
    assert at(0, (4, 0)) == at(0, (3, 9)) + 1 and toff.tolist() == [0, 2, 4]          # neighbours in the list, 9 columns apart
    w = cluster_vertices_numpy(*args, ClusterVertexSpec(3, 3), tcls)
    assert w["vertex_offsets"].tolist() == [0, 4, 8] and (w["vertices"]["ends"] == 1).all() and (w["vertices"]["rows"] == 1).all()
    assert (w["incidence"][:, 2] == 3).all() and w["events"].tolist() == [[4, 0, 4, 0], [4, 0, 4, 0]]
    assert w["row_vertex"].tolist() == [[0, 1], [2, 3], [0, 1], [2, 3]]


def test_rows_that_are_not_eligible():
    shape = (12, 10)
    segs = [([(2, 2)], 1), ([(2, 5), (2, 6), (2, 7)], 2), ([(8, 1), (8, 2)], 1)]
    args, tcls, ids, toff, at = _scene(shape, [segs], ClusterSpec(8, (1, 2), True))
    one = cluster_vertices_numpy(*args, ClusterVertexSpec(1, 1), tcls)
    assert one["row_vertex"].tolist() == [[0, 0], [1, 2], [3, 4]] and one["vertices"]["ends"].tolist() == [1] * 5
    assert one["vertices"]["mask_flags"].tolist() == [2 | 2 << 32, 4, 4, 2, 2]      # the single voxel has length 0
    three = cluster_vertices_numpy(*args, ClusterVertexSpec(1, 3), tcls)
    assert three["row_vertex"].tolist() == [[-1, -1], [0, 1], [-1, -1]]
    only = cluster_vertices_numpy(*args, ClusterVertexSpec(3, 1, (1,)), tcls)
    assert only["row_vertex"].tolist() == [[0, 0], [-1, -1], [1, 2]]
    inc = only["incidence"][only["inc_offsets"][0]:only["inc_offsets"][1]]
    assert inc.tolist() == [[0, 1, 1, 0, at(0, (2, 2))], [1, 0, 1, 9, at(0, (2, 5))]]       # the other class passes as a body
    assert only["vertices"]["mask_flags"][0] == 6 | 2 << 32


def test_the_statement_raises_on_inconsistent_input(monkeypatch):
    shape, spec = (12, 10), ClusterVertexSpec(2, 1)
    ok = dict(offsets=[0, 3], index=[1, 2, 35], value=None, cluster=[0, 0, 1], table_offsets=[0, 2], spatial=shape, spec=spec, cls=[1, 2])
    assert cluster_vertices_numpy(**ok)["vertex_offsets"].tolist() == [0, 3]
    for change in (dict(cluster=[0, 0, 2]), dict(table_offsets=[0, 3], cls=[1, 2, 1]), dict(index=[1, 2, 120]), dict(index=[1, 2, -1]),
                   dict(cls=[1, 32]), dict(cls=[1]), dict(spatial=(12, 10, 4, 4)), dict(offsets=[0, 2])):
        with pytest.raises(ValueError):
            cluster_vertices_numpy(**dict(ok, **change))
    real = clusters.cluster_features_numpy

    def moved(*a, **kw):
        f = real(*a, **kw)
        f["end_hi"][0] = 2                                               # a member of the other row
        return f
    monkeypatch.setattr(clusters, "cluster_features_numpy", moved)
    with pytest.raises(ValueError) as e:
        cluster_vertices_numpy(**ok)
    assert "not a member" in str(e.value)
