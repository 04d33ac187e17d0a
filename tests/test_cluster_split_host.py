"""Cluster splits, host side (no GPU): the appended symbols under an unchanged ABI 9, the scratch query, every argument refusal of
ursn_cluster_split (include/uresnet_hip.h), ClusterSplitSpec, the ANA_SPLIT / SPLIT_* keys and the driver's refusal,
set_cluster_split, and the pure-Python statement (uresnet_amd.clusters.cluster_split_numpy): hand-built shapes with hand-checked
answers, invariants, the coverage of exactly the lists tests/test_cluster_split_gpu.py runs (tests/_split_cases.py makes them for
both files), and the purpose of the feature against the true particles of toy events.  Every library call below is refused on its
arguments before any device access, so the fake pointers are never dereferenced."""
import ctypes
import io
import os
from contextlib import redirect_stdout

import numpy as np
import pytest

import _split_cases as cases
import uresnet_amd  # noqa: F401
from uresnet_amd import _lib, ssnet_config, uresnet
from uresnet_amd.clusters import (SPLIT_EVENT, SPLIT_JUNCTION_INT, SPLIT_JUNCTION_REAL, SPLIT_PIECE, SPLIT_ROW, ClusterChainSpec,
                                  ClusterSpec, ClusterSplitSpec, cluster_chains_numpy, cluster_split_numpy)
from uresnet_amd.ssnet import chains_csv_header, split_csv_header, split_csv_row

FAKE = 0x10000
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _p(a):
    return ctypes.c_void_p(a)


def test_symbols_appended_under_abi_9(lib):
    assert _lib.ABI_VERSION == 9 and lib.ursn_abi_version() == 9
    with open(os.path.join(ROOT, "include", "uresnet_hip.h")) as f:
        hdr = f.read()
    for name in ("ursn_cluster_split_scratch_bytes", "ursn_cluster_split"):
        assert name in _lib.EXPORTS and hasattr(lib, name) and (name + "(") in hdr, name
    assert "#define URSN_ABI_VERSION 9" in hdr and "} ursn_cluster_split_desc;" in hdr and "} ursn_cluster_split_out;" in hdr
    for name in ("PI", "JI", "JR", "ROW", "EV"):
        assert "#define URSN_CLSPLIT_%s %d " % (name, getattr(_lib, "CLSPLIT_" + name)) in hdr, name
    assert (_lib.CLSPLIT_PI, _lib.CLSPLIT_JI, _lib.CLSPLIT_JR, _lib.CLSPLIT_ROW, _lib.CLSPLIT_EV) == \
        (len(SPLIT_PIECE), len(SPLIT_JUNCTION_INT), len(SPLIT_JUNCTION_REAL), len(SPLIT_ROW), len(SPLIT_EVENT)) == (8, 18, 3, 3, 4)
    assert ctypes.sizeof(_lib.ursn_cluster_split_desc) == 104 and ctypes.sizeof(_lib.ursn_cluster_split_out) == 128
    # the section stands between the cones' and the vertices': nothing that other tests pin moved
    assert hdr.index("ursn_cluster_cones(") < hdr.index("ursn_cluster_split_scratch_bytes(") < hdr.index("ursn_cluster_split(") < \
        hdr.index("ursn_cluster_vertices_scratch_bytes(")
    assert hdr.rindex("\nint ursn_") == hdr.index("\nint ursn_cluster_vertices(")
    for title in ("cluster chains: broken track fragments", "cluster cones: shower fragments", "per-cluster charge profiles"):
        assert hdr.count(title) == 1, title
    section = hdr.split("cluster splits: a component of several particles")[1].split("ursn_cluster_vertices_scratch_bytes(")[0]
    for text in ("min(their number, 15)", "c = (double)dot / (sqrt((double)q_1) * sqrt((double)q_2))", "URSN_CLSPLIT_WAVE=0",
                 "`first` need not ascend", "\"cluster_split:\"", "components -> split -> chains -> cones"):
        assert text in section, text
    with open(os.path.join(ROOT, "u-resnet_amd", "build.py")) as f:
        assert '"cluster_split.hip"' in f.read()


def test_scratch_query(lib):
    """The domain only: at least 8 bytes, 8-byte granular, monotone in the list length, 0 outside; no layout is pinned."""
    q = lib.ursn_cluster_split_scratch_bytes
    ms = (0, 1, 63, 64, 65, 2047, 2048, 2049, 8000, 10 ** 6, 2 ** 30 - 1)
    for n in (1, 5, 65535):
        sizes = [q(n, m) for m in ms]
        assert all(b >= 8 and b % 8 == 0 for b in sizes) and sizes == sorted(sizes) and sizes[0] < sizes[-1], (n, sizes)
    assert q(1, 1000) <= q(5, 1000) <= q(65535, 1000)
    for args in ((0, 10), (-1, 10), (65536, 10), (1, -1), (1, 2 ** 30), (1, 2 ** 40), (1, -2 ** 62)):
        assert q(*args) == 0, args


DESC = dict(ndim=3, n=2, radius=2, m_total=10, offsets=FAKE, index=FAKE + 0x1000, cluster=FAKE + 0x2000, table_offsets=FAKE + 0x3000,
            size=FAKE + 0x5000, cls=FAKE + 0x7000, kink_cos=-0.7, min_size=8, class_mask=6, grow=4, reserved=0)
OUT = dict(split=FAKE + 0x10000, mark=FAKE + 0x11000, piece_offsets=FAKE + 0x12000, first=FAKE + 0x13000, size=FAKE + 0x14000,
           cls=FAKE + 0x15000, piece_itab=FAKE + 0x16000, cap_pieces=10, junction_offsets=FAKE + 0x17000, junction_itab=FAKE + 0x18000,
           junction_rtab=FAKE + 0x19000, cap_junctions=10, rows=FAKE + 0x1a000, cap_rows=10, event=FAKE + 0x1d000, status=FAKE + 0x1e000)
SCRATCH = FAKE + 0x40000


def _refused(lib, text, scratch=SCRATCH, sbytes=1 << 20, null=None, spatial=(7, 9, 11), out=None, **kw):
    d, o = _lib.ursn_cluster_split_desc(), _lib.ursn_cluster_split_out()
    for k, v in DESC.items():
        setattr(d, k, kw.pop(k, v))
    for i, s in enumerate(spatial):
        d.spatial[i] = s
    for k, v in dict(OUT, **(out or {})).items():
        setattr(o, k, v)
    assert not kw, kw
    rc = lib.ursn_cluster_split(None if null == "desc" else ctypes.byref(d), None if null == "out" else ctypes.byref(o), _p(scratch),
                                sbytes, None)
    msg = lib.ursn_last_error()
    assert rc != 0 and msg.startswith(b"cluster_split:") and text in msg, (rc, msg)


def test_cluster_split_refusals(lib):
    """Null streams and fake device pointers: a call that got past its checks would fault here, not return."""
    who = b"cluster_split"
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
    r(b": radius = 0 outside [1, 3]", radius=0)
    r(b": radius = 4 outside [1, 3]", radius=4)
    r(b": radius = -2147483648 outside [1, 3]", radius=-2 ** 31)
    r(b": kink_cos = nan outside [-1, 1]", kink_cos=float("nan"))
    r(b": kink_cos = -1.1 outside [-1, 1]", kink_cos=-1.1)
    r(b": kink_cos = 1.5 outside [-1, 1]", kink_cos=1.5)
    r(b": kink_cos = inf outside [-1, 1]", kink_cos=float("inf"))
    r(b": min_size = 0 < 1", min_size=0)
    r(b": min_size = -5 < 1", min_size=-5)
    r(b": grow = -1 outside [0, 8]", grow=-1)
    r(b": grow = 9 outside [0, 8]", grow=9)
    r(b": reserved = 1, expected 0", reserved=1)
    ro(b": cap_pieces = -1 < 0", cap_pieces=-1)
    ro(b": cap_junctions = -1 < 0", cap_junctions=-1)
    ro(b": cap_rows = -1 < 0", cap_rows=-1)
    ro(b": cap_rows = -9223372036854775808 < 0", cap_rows=-2 ** 63)
    r(b": null offsets / table_offsets", offsets=None)
    r(b": null offsets / table_offsets", table_offsets=None)
    for key in ("index", "cluster", "size"):
        r(b": null index / cluster / size", **{key: None})
    r(b": class_mask = 0x6 needs cls", cls=None)
    ro(b": null out->status", status=None)
    for key in ("piece_offsets", "junction_offsets", "event"):
        ro(b": null out->piece_offsets / out->junction_offsets / out->event", **{key: None})
    for key in ("split", "mark"):
        ro(b": null out->split / out->mark", **{key: None})
    for key in ("piece_itab", "first", "size", "cls"):
        ro(b": null out->piece_itab / out->first / out->size / out->cls", **{key: None})
    for key in ("junction_itab", "junction_rtab"):
        ro(b": null out->junction_itab / out->junction_rtab", **{key: None})
    ro(b": null out->rows", rows=None)
    r(b": null scratch", scratch=None)
    aligned8 = b": offsets / table_offsets / the out tables / scratch must be 8-byte aligned"
    for key in ("offsets", "table_offsets"):
        r(aligned8, **{key: DESC[key] + 4})
    for key in ("piece_offsets", "piece_itab", "junction_offsets", "junction_itab", "junction_rtab", "event"):
        ro(aligned8, **{key: OUT[key] + 4})
    r(aligned8, scratch=SCRATCH + 4)
    aligned4 = b": index / cluster / size / split / first / the row array / status must be 4-byte aligned"
    for key in ("index", "cluster", "size"):
        r(aligned4, **{key: DESC[key] + 2})
    for key in ("split", "first", "size", "rows"):
        ro(aligned4, **{key: OUT[key] + 2})
    ro(aligned4, status=OUT["status"] + 1)
    need = lib.ursn_cluster_split_scratch_bytes(2, 10)
    r(b": scratch of %d bytes is too small, %d needed" % (need - 8, need), sbytes=need - 8)
    # legal shapes of a call get as far as the scratch size: no cls; 2-D; the ends of the ranges; no rows / pieces / junctions / entries
    small = b": scratch of 0 bytes is too small"
    r(small, cls=None, class_mask=0, sbytes=0)
    r(small, cls=FAKE + 0x7001, class_mask=0xFFFFFFFF, sbytes=0)                                       # bytes: no alignment asked
    _refused(lib, who + small, out=dict(cls=OUT["cls"] + 1, mark=OUT["mark"] + 1), sbytes=0)
    r(small, ndim=2, spatial=(32768, 32768, -5), sbytes=0)
    r(small, radius=1, kink_cos=-1.0, min_size=1, grow=0, sbytes=0)
    r(small, radius=3, kink_cos=1.0, min_size=2 ** 31 - 1, grow=8, sbytes=0)
    _refused(lib, who + small, out=dict(cap_rows=0, rows=None), sbytes=0)
    _refused(lib, who + small, out=dict(cap_pieces=0, piece_itab=None, first=None, size=None, cls=None), sbytes=0)
    _refused(lib, who + small, out=dict(cap_junctions=0, junction_itab=None, junction_rtab=None), sbytes=0)
    _refused(lib, who + small, out=dict(split=None, mark=None), m_total=0, index=None, cluster=None, size=None, sbytes=0)


def test_cluster_split_spec_refusals():
    s = ClusterSplitSpec()
    assert (s.radius, s.kink_cos, s.min_size, s.classes, s.grow) == (2, -0.7, 8, None, 4) and s.class_mask() == 0
    assert repr(s) == "ClusterSplitSpec(radius=2, kink_cos=-0.7, min_size=8, classes=None, grow=4)"
    s = ClusterSplitSpec(3, 1, 1, {1, 4}, 0)
    assert (s.radius, s.kink_cos, type(s.kink_cos), sorted(s.classes), s.class_mask(), s.grow) == (3, 1.0, float, [1, 4], 18, 0)
    assert ClusterSplitSpec(1).grow == 2 and ClusterSplitSpec(3).grow == 6 and ClusterSplitSpec(3, grow=8).grow == 8
    assert ClusterSplitSpec(1, -1.0, 2 ** 31 - 1, [0, 31]).class_mask() == 0x80000001
    for bad in (0, 4, -1, 2.0, True, "2", None):
        with pytest.raises(ValueError) as e:
            ClusterSplitSpec(radius=bad)
        assert "radius" in str(e.value) and repr(bad) in str(e.value), str(e.value)
    for bad in (-1.1, 1.5, float("nan"), float("inf"), True, "0.9", None):
        with pytest.raises(ValueError) as e:
            ClusterSplitSpec(kink_cos=bad)
        assert "kink_cos" in str(e.value) and repr(bad) in str(e.value), str(e.value)
    for bad in (0, -3, 2 ** 31, 3.0, True, "3", None):
        with pytest.raises(ValueError) as e:
            ClusterSplitSpec(min_size=bad)
        assert "min_size" in str(e.value) and repr(bad) in str(e.value), str(e.value)
    for bad in ((), [32], [-1], [1, 1], [1.0], ["1"], [True], 3):
        with pytest.raises(ValueError) as e:
            ClusterSplitSpec(classes=bad)
        assert "classes" in str(e.value) and repr(bad) in str(e.value), str(e.value)
    for bad in (-1, 9, 2.0, True, "2"):
        with pytest.raises(ValueError) as e:
            ClusterSplitSpec(grow=bad)
        assert "grow" in str(e.value) and repr(bad) in str(e.value), str(e.value)
    with pytest.raises(ValueError):
        cluster_split_numpy([0, 0], [], [], [0, 0], [], (4, 4), 2)
    with pytest.raises(ValueError):
        cluster_split_numpy([0, 0], [], [], [0, 0], [], (4, 4), ClusterSplitSpec(classes=(1,)))                 # classes need cls
    assert cluster_split_numpy([0, 0], [], [], [0, 0], [], (4, 4), ClusterSplitSpec())["events"].tolist() == [[0, 0, 0, 0]]
    line = dict(offsets=[0, 3], index=[0, 1, 2], cluster=[0, 0, 0], table_offsets=[0, 1], size=[3], spatial=(4, 4), spec=ClusterSplitSpec(1, 1.0, 1))
    assert cluster_split_numpy(**line)["split"].tolist() == [0, 0, 0]
    for change in (dict(index=[0, 2, 2]), dict(index=[0, 1, 16]), dict(cluster=[0, 1, 0]), dict(cls=[32]), dict(size=[3, 1])):
        with pytest.raises(ValueError):
            cluster_split_numpy(**dict(line, **change))


# ---- config keys, driver, Python surface ---------------------------------------------------------------------------------------
def test_config_keys_default_off_and_validated(tmp_path):
    c = ssnet_config()
    keys = ("ANA_SPLIT", "SPLIT_RADIUS", "SPLIT_KINK_COS", "SPLIT_MIN_SIZE", "SPLIT_CLASSES", "SPLIT_GROW", "SPLIT_DOWNSTREAM")
    assert [getattr(c, k) for k in keys] == ["", 2, -0.7, 8, [], -1, False]
    out = io.StringIO()
    with redirect_stdout(out):
        c.dump()
    for key in keys:
        assert any(line.startswith(key + ".") or line.startswith(key + " ") for line in out.getvalue().split("\n")), key
    p = tmp_path / "a.cfg"
    p.write_text("ANA_SPLIT '/tmp/split.csv'\nSPLIT_RADIUS 3\nSPLIT_KINK_COS -0.25\nSPLIT_MIN_SIZE 5\nSPLIT_CLASSES [1, 2]\n"
                 "SPLIT_GROW 0\nSPLIT_DOWNSTREAM True\n")
    with redirect_stdout(io.StringIO()):
        c.override(str(p))
    assert [getattr(c, k) for k in keys] == ["/tmp/split.csv", 3, -0.25, 5, [1, 2], 0, True]
    assert [getattr(ssnet_config(), k) for k in keys] == ["", 2, -0.7, 8, [], -1, False]
    for text in ("ANA_SPLIT True\n", "ANA_SPLIT 1\n", "ANA_SPLIT ['a.csv']\n", "ANA_SPLIT None\n", "SPLIT_RADIUS 0\n", "SPLIT_RADIUS 4\n",
                 "SPLIT_RADIUS 2.0\n", "SPLIT_RADIUS '2'\n", "SPLIT_KINK_COS -1.1\n", "SPLIT_KINK_COS 1.5\n", "SPLIT_KINK_COS '0.9'\n",
                 "SPLIT_KINK_COS float('nan')\n", "SPLIT_MIN_SIZE 0\n", "SPLIT_MIN_SIZE 3.0\n", "SPLIT_MIN_SIZE '3'\n", "SPLIT_CLASSES [32]\n",
                 "SPLIT_CLASSES [1, 1]\n", "SPLIT_CLASSES [1.0]\n", "SPLIT_CLASSES 1\n", "SPLIT_GROW -2\n", "SPLIT_GROW 9\n", "SPLIT_GROW 2.0\n",
                 "SPLIT_DOWNSTREAM 1\n", "SPLIT_DOWNSTREAM 'yes'\n"):
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


def test_driver_refuses_ana_split_without_ana_cluster(tmp_path):
    """Before a stream is opened or a device is touched; the file is not created."""
    csv = tmp_path / "split.csv"
    for text in ("TRAIN False\nANA_SPLIT '%s'\n" % csv,
                 "TRAIN False\nSPARSE_IO True\nSPARSE_SCORES True\nSPLIT_RADIUS 3\nANA_SPLIT '%s'\n" % csv):
        with pytest.raises(ValueError) as e:
            _driver(tmp_path, text).initialize()
        assert "ANA_SPLIT" in str(e.value) and "ANA_CLUSTER" in str(e.value), str(e.value)
    assert not csv.exists()
    head = split_csv_header()
    assert head.endswith("\n") and head[:-1].split(",") == ["entry", "junction"] + list(SPLIT_JUNCTION_INT) + list(SPLIT_JUNCTION_REAL)
    cols = {name: np.array([3 + c, -(7 + c)], np.int64) for c, name in enumerate(SPLIT_JUNCTION_INT)}
    cols.update({name: np.array([0.5, 1.0 / 3.0 + c]) for c, name in enumerate(SPLIT_JUNCTION_REAL)})
    cells = split_csv_row(5, 1, cols)[:-1].split(",")
    assert cells[:20] == ["5", "1"] + [str(-(7 + c)) for c in range(18)]
    assert [float(x) for x in cells[20:]] == [1.0 / 3.0 + c for c in range(3)]
    assert len(chains_csv_header().split(",")) == 23                                  # the chains file is as it was


def test_set_cluster_split_leaves_want_as_it_was():
    """construct(allocate=False) never touches a device."""
    net = uresnet(dims=[16, 16, 16, 1], num_class=3, base_num_outputs=4, num_strides=2)
    assert net._want_names() == ("scores", "pred", "ana")
    net.set_cluster_split(ClusterSplitSpec(3), downstream=True)
    assert net._want_names() == ("scores", "pred", "ana") and net._cluster_split_downstream is True
    net.set_clustering(ClusterSpec())
    assert net._want_names() == ("scores", "pred", "ana", "cluster")
    net.set_cluster_split(None, downstream=True)
    assert net._cluster_split_spec is None and net._cluster_split_downstream is False
    for bad in (True, 1, 2.0, "2", ClusterSpec()):
        with pytest.raises(ValueError) as e:
            net.set_cluster_split(bad)
        assert "set_cluster_split" in str(e.value)
    with pytest.raises(ValueError) as e:
        net.set_cluster_split(ClusterSplitSpec(), downstream=1)
    assert "downstream" in str(e.value)
    with pytest.raises(ValueError) as e:
        net.cluster_split(None, [np.arange(3)], {"cluster": [np.zeros(3)], "clusters": [{"first": np.zeros(1)}]}, 5)
    assert "cluster_split" in str(e.value)


# ---- the statement ---------------------------------------------------------------------------------------------------------------
def _one(shape, cells, spec, cls=1):
    c = cases.batch(shape, [([(cells, cls)], [])])
    w = cluster_split_numpy(c["off"], c["index"], c["cluster"], c["toff"], c["size"], shape, spec, c["cls"])
    at = {cell: j for j, cell in enumerate(sorted(cells, key=lambda x: int(np.ravel_multi_index(x, shape))))}
    return c, w, at


def test_hand_checked_shapes():
    # a straight line along the last axis: the two ends see one arm, the bodies two, the stubs next to the ends one; nothing is cut
    c, w, at = _one((5, 5, 12), cases.path((2, 2, 1), (2, 2, 10)), ClusterSplitSpec(2, -0.7, 1))
    assert (w["mark"] & 15).tolist() == [1, 1, 2, 2, 2, 2, 2, 2, 1, 1] and w["split"].tolist() == [0] * 10
    assert w["events"].tolist() == [[1, 0, 0, 0]] and w["rows"].tolist() == [[1, 0, 0]]
    assert {k: v.tolist() for k, v in w["pieces"].items()} == dict(row=[0], n=[10], attached=[0], kind=[1], key=[0], contacts=[0],
                                                                  junction_lo=[-1], junction_hi=[-1])
    # a plus in 2-D with arms of 5: at radius 2 the centre and its four neighbours see four arms (the next ones out two, opposite); with grow 0 that junction of
    # five is a piece of kind 2 between four arms of four
    plus = cases.path((1, 6), (11, 6)) | cases.path((6, 1), (6, 11))
    c, w, at = _one((13, 13), plus, ClusterSplitSpec(2, 1.0, 1, None, 0))
    centre = at[(6, 6)]
    assert w["mark"][centre] == (4 | 16) and sorted(w["mark"][at[x]] for x in ((5, 6), (7, 6), (6, 5), (6, 7))) == [4 | 16] * 4
    assert int((w["mark"] & 16 > 0).sum()) == 5 and w["events"].tolist() == [[5, 1, 1, 5]]
    assert sorted(w["pieces"]["kind"].tolist()) == [1, 1, 1, 1, 2] and sorted(w["pieces"]["n"].tolist()) == [4, 4, 4, 4, 5]
    j = {k: v.tolist() for k, v in w["junctions"].items()}
    assert (j["entries"], j["attached"], j["arms_max"], j["kinks"], j["contacts"]) == ([5], [0], [4], [0], [4])
    assert (j["s0"], j["s1"], j["lo0"], j["hi0"], j["lo1"], j["hi1"], j["c0"], j["c1"], j["c2"]) == ([30], [30], [5], [7], [5], [7], [6.0], [6.0], [0.0])
    assert j["first_pos"] == [at[(5, 6)]] and (j["piece_lo"], j["piece_hi"]) == ([0], [4])
    k2 = w["pieces"]["kind"].tolist().index(2)
    assert w["pieces"]["junction_lo"].tolist() == [0] * 5 and w["pieces"]["contacts"].tolist() == [1 if k != k2 else 0 for k in range(5)]
    # the same with grow 1: the four neighbours go to their arms, the centre stays
    c, w1, at = _one((13, 13), plus, ClusterSplitSpec(2, 1.0, 1, None, 1))
    assert sorted(w1["pieces"]["n"].tolist()) == [1, 5, 5, 5, 5] and int((w1["mark"] & 64 > 0).sum()) == 4
    assert w1["junctions"]["attached"].tolist() == [4] and np.array_equal(w1["mark"] & 63, w["mark"])
    # grow 2: the centre takes the piece of its neighbour at the lowest position, (5, 5) does not exist, so (5, 6)'s
    c, w2, at = _one((13, 13), plus, ClusterSplitSpec(2, 1.0, 1, None, 2))
    assert w2["split"][centre] == w2["split"][at[(5, 6)]] == w2["split"][at[(1, 6)]] and sorted(w2["pieces"]["kind"].tolist()) == [1] * 4
    assert sorted(w2["pieces"]["n"].tolist()) == [5, 5, 5, 6] and w2["junctions"]["attached"].tolist() == [5]
    # a right angle: kink_cos -0.7 cuts the corner (cosine 0 > -0.7), kinks off leaves the L whole
    ell = cases.path((2, 2), (2, 10), (10, 10))
    c, w, at = _one((13, 13), ell, ClusterSplitSpec(2, -0.7, 1, None, 0))
    assert w["mark"][at[(2, 10)]] == (2 | 16 | 32) and w["events"][0, 1] == 1 and w["junctions"]["kinks"][0] == w["junctions"]["entries"][0]
    c, w, at = _one((13, 13), ell, ClusterSplitSpec(2, 1.0, 1, None, 0))
    assert w["events"].tolist() == [[1, 0, 0, 0]]


def _invariants(c, w, spec):
    off, toff = c["off"], c["toff"]
    n = off.size - 1
    assert w["split"].dtype == np.int32 and w["mark"].dtype == np.uint8 and w["rows"].dtype == np.int32
    assert np.array_equal(w["split"] < 0, np.asarray(c["cluster"]) < 0)
    assert np.array_equal(w["events"][:, 0], np.diff(w["piece_offsets"])) and np.array_equal(w["events"][:, 1], np.diff(w["junction_offsets"]))
    for e in range(n):
        ids = w["split"][off[e]:off[e + 1]]
        lo, hi = w["piece_offsets"][e], w["piece_offsets"][e + 1]
        members = ids[ids >= 0]
        assert np.array_equal(np.unique(members), np.arange(hi - lo))                      # every piece has a member, no id is skipped
        assert np.array_equal(np.bincount(members, minlength=hi - lo), w["table"]["size"][lo:hi])
        for k in range(hi - lo):
            where = np.flatnonzero(ids == k)
            assert w["table"]["first"][lo + k] == where[0]
            rows = np.unique(np.asarray(c["cluster"])[off[e]:off[e + 1]][where])
            assert rows.tolist() == [w["pieces"]["row"][lo + k]]                            # a piece never crosses its row
        assert np.all(np.diff(w["pieces"]["key"][lo:hi]) > 0)                                # numbered by ascending key
        assert w["events"][e, 3] == int((w["mark"][off[e]:off[e + 1]] & 16 > 0).sum())
    assert np.array_equal(w["pieces"]["n"], w["table"]["size"]) and w["pieces"]["attached"].sum() == int((w["mark"] & 64 > 0).sum())
    assert w["pieces"]["contacts"].sum() == w["junctions"]["contacts"].sum()
    assert np.array_equal(w["rows"][:, 0], np.bincount(np.repeat(toff[:-1], np.diff(w["piece_offsets"])) + w["pieces"]["row"], minlength=toff[-1]))
    assert w["rows"][:, 2].sum() == w["junctions"]["entries"].sum() == int((w["mark"] & 16 > 0).sum())
    assert ((w["mark"] & 64 > 0) <= (w["mark"] & 16 > 0)).all() and ((w["mark"] & 32 > 0) <= (w["mark"] & 16 > 0)).all()
    if spec.grow == 0:
        assert not (w["mark"] & 64).any() and (w["pieces"]["kind"] == 2).sum() == w["junction_offsets"][-1]


@pytest.mark.parametrize("radius", [1, 2, 3])
@pytest.mark.parametrize("name", sorted(cases.CASES))
def test_invariants_of_the_cases(name, radius):
    spec = ClusterSplitSpec(radius)
    _invariants(cases.case(name), cases.statement(name, spec), spec)


def test_invariants_at_other_settings():
    for name, spec in (("jacks", ClusterSplitSpec(3, -0.7, 8, None, 1)), ("jacks", ClusterSplitSpec(3, -0.7, 8, None, 0)),
                       ("shapes3d", ClusterSplitSpec(2, 1.0, 8, None, 0)), ("mixed", ClusterSplitSpec(2, -0.7, 8, (1, 2), None))):
        _invariants(cases.case(name), cases.statement(name, spec), spec)


def test_what_the_cases_cover():
    """Arms 0, 1, 2, 3 and 4 or more, a kink, an attached entry, a remainder of kind 2, a clipped ball, a dropped limb, a wrap that
    index arithmetic alone would make, rows that are not eligible by size and by class, entries without an id, empty events."""
    arms = set()
    for name in cases.CASES:
        for radius in (1, 2, 3):
            arms |= set((cases.statement(name, ClusterSplitSpec(radius))["mark"] & 15).tolist())
    assert {0, 1, 2, 3, 4, 5, 6} <= arms
    w = cases.statement("shapes3d", ClusterSplitSpec(2))
    assert (w["mark"] & 32).any() and (w["mark"] & 64).any() and w["junctions"]["kinks"].max() > 0
    c = cases.case("shapes3d")
    ev = lambda e: slice(int(c["off"][e]), int(c["off"][e + 1]))
    assert c["off"][3] == c["off"][2] and (c["cluster"] < 0).sum() == 2                                    # an empty event, two noise voxels
    assert w["events"][0, 1] >= 1 and (w["mark"][ev(0)] & 15).max() == 3                                   # the Y: a junction of three arms
    assert (w["mark"][ev(1)] & 15).max() == 4                                                              # the X: four
    assert (w["mark"][ev(3)] & 32).any() and (w["mark"][ev(3)] & 15).max() == 2                            # the V: a kink and no junction
    assert w["events"][4].tolist() == [2, 0, 0, 0] and set((w["mark"][ev(4)] & 15).tolist()) == {0, 1, 2}   # the line whole; the stub not evaluated
    assert w["pieces"]["kind"][w["piece_offsets"][4]:w["piece_offsets"][5]].tolist() in ([1, 0], [0, 1])
    assert w["events"][6].tolist() == [1, 0, 0, 0] and set((w["mark"][ev(6)] & 15).tolist()) == {2}            # the ring: every entry a body
    assert w["events"][5, 0] == 1 and (w["mark"][ev(5)] & 15).max() == 2          # the thick track: steps read as kinks, all handed back
    assert w["events"][8].tolist() == [1, 0, 0, 0] and set((w["mark"][ev(8)] & 15).tolist()) == {1}          # a solid blob: its shell is one arm
    # the U-turn: both limbs lie inside one ball, REACH drops the other limb: bodies see two arms, not four, and nothing is cut there
    for radius in (2, 3):
        u = cases.statement("shapes3d", ClusterSplitSpec(radius, 1.0))
        body = [j for j in range(int(c["off"][7]), int(c["off"][8])) if c["cluster"][j] >= 0 and 8 <= c["index"][j] % 24 <= 12]
        assert len(body) == 10 and set((u["mark"][body] & 15).tolist()) == {2}
    for name in ("shapes2d",):
        u, c2 = cases.statement(name, ClusterSplitSpec(2, 1.0)), cases.case(name)
        body = [j for j in range(int(c2["off"][5]), int(c2["off"][6])) if 10 <= c2["index"][j] // 40 <= 20]
        assert len(body) == 22 and set((u["mark"][body] & 15).tolist()) == {2}
    # a remainder of kind 2 with grow > 0, and every junction one with grow 0
    w = cases.statement("jacks", ClusterSplitSpec(3, -0.7, 8, None, 1))
    assert (w["pieces"]["kind"] == 2).sum() == 1 and w["pieces"]["n"][w["pieces"]["kind"] == 2].tolist() == [7] and (w["mark"] & 15).max() == 6
    assert (w["table"]["first"][w["pieces"]["kind"] == 2] != w["pieces"]["key"][w["pieces"]["kind"] == 2]).all()   # its key entry went away
    assert (cases.statement("jacks", ClusterSplitSpec(3, -0.7, 8, None, 0))["pieces"]["kind"] == 2).sum() == 1
    # clipped balls: every entry of the frames is within the radius of a face, the corners are junctions of three
    for name, shape in (("frame3d", (9, 10, 11)), ("frame2d", (12, 9))):
        w, c = cases.statement(name, ClusterSplitSpec(3)), cases.case(name)
        x = np.stack(np.unravel_index(c["index"], shape), 1)
        clipped = ((x < 3) | (x >= np.array(shape) - 3)).any(axis=1)
        assert (clipped.all() if name == "frame3d" else clipped.sum() >= 36) and w["junction_offsets"][-1] >= 2
        for a in range(len(shape)):
            assert (x[:, a] == 0).any() and (x[:, a] == shape[a] - 1).any()
    assert cases.statement("frame3d", ClusterSplitSpec(2))["junction_offsets"][-1] == 8 and \
        cases.statement("frame3d", ClusterSplitSpec(2))["junctions"]["arms_max"].tolist() == [3] * 8
    # the wrap: consecutive indices across a row end, one row, two pieces at every radius
    for name, shape in (("wrap3d", (8, 8, 12)), ("wrap2d", (10, 12))):
        c = cases.case(name)
        assert (np.diff(c["index"]) == 1).any() and c["toff"].tolist() == [0, 1]
        j = int(np.flatnonzero((np.diff(c["index"]) == 1) & (c["index"][:-1] % shape[-1] == shape[-1] - 1))[0])
        for radius in (1, 2, 3):
            w = cases.statement(name, ClusterSplitSpec(radius, 1.0))
            assert w["split"][j] != w["split"][j + 1] and w["events"][0, 0] == 2 and (w["mark"][[j, j + 1]] & 15).tolist() == [1, 1]
    # rows that are not eligible: by size (a row of two limbs stays ONE piece of kind 0), by class
    c, w = cases.case("mixed"), cases.statement("mixed", ClusterSplitSpec(2, -0.7, 8, (1, 2), None))
    assert c["off"][0] == c["off"][1] and c["off"][-1] == c["off"][-2]
    assert (w["pieces"]["kind"] == 0).sum() == 4 and w["rows"][:, 0].tolist() == [1, 3, 1, 1, 1, 3]
    far = w["pieces"]["n"][(w["pieces"]["kind"] == 0)]
    assert sorted(far.tolist()) == [7, 7, 22, 31]                                  # two limbs far apart stay one piece; class 3 stays whole
    assert np.array_equal(c["index"][c["off"][1]:c["off"][2]][1:], c["index"][c["off"][2]:c["off"][3]])     # the same indices in neighbouring events
    # the long case and its replica
    m = int(cases.case("many")["off"][-1])
    assert m == 1117 and m % 256 and m % 64 and m % 4 and -(-59 * m // 64) > 1024 >= -(-58 * m // 64)
    big, want = cases.replicate(cases.case("jacks"), cases.statement("jacks", ClusterSplitSpec(3)), 3)
    again = cluster_split_numpy(big["off"], big["index"], big["cluster"], big["toff"], big["size"], big["shape"], ClusterSplitSpec(3), big["cls"])
    for k in ("split", "mark", "piece_offsets", "junction_offsets", "rows", "events"):
        assert np.array_equal(want[k], again[k]), k
    for group in ("table", "pieces", "junctions"):
        for k in want[group]:
            assert np.array_equal(want[group][k], again[group][k]), (group, k)


# ---- the purpose: pieces against the true particles ------------------------------------------------------------------------------
def _ari(a, b):
    """The adjusted Rand index of two labelings of the same entries."""
    a, b = np.unique(a, return_inverse=True)[1], np.unique(b, return_inverse=True)[1]
    table = np.zeros((a.max() + 1, b.max() + 1), np.int64)
    np.add.at(table, (a, b), 1)
    pairs = lambda x: (x * (x - 1) // 2).sum()
    both, ra, rb, total = pairs(table), pairs(table.sum(1)), pairs(table.sum(0)), a.size * (a.size - 1) // 2
    expected = ra * rb / total
    return float((both - expected) / (0.5 * (ra + rb) - expected)) if 0.5 * (ra + rb) != expected else 0.0


TOY = (40, 40, 40)


def _connected(cells):
    todo, seen = [cells[0]], {cells[0]}
    have = set(cells)
    while todo:
        x = todo.pop()
        for d in np.ndindex(3, 3, 3):
            y = (x[0] + d[0] - 1, x[1] + d[1] - 1, x[2] + d[2] - 1)
            if y in have and y not in seen:
                seen.add(y)
                todo.append(y)
    return len(seen) == len(have)


def _direction(rng):
    v = rng.normal(size=3)
    return v / np.linalg.norm(v)


def toy_event(kind, seed):
    """One component of several true particles: ``prongs`` (three tracks from one vertex), ``kink`` (two tracks end to end at an
    angle), ``cross`` (two tracks through one point).  Returns (cells in list order, true particle of each)."""
    rng = np.random.default_rng(seed)
    centre = rng.integers(16, 24, size=3).astype(np.float64)
    while True:
        dirs = [_direction(rng) for _ in range(3)]
        cosines = [abs(float(dirs[i] @ dirs[k])) if kind == "cross" else float(dirs[i] @ dirs[k]) for i in range(3) for k in range(i)]
        if max(cosines) < 0.5:
            break
    tip = lambda d, length: tuple(int(x) for x in np.rint(centre + d * length))
    c0 = tuple(int(x) for x in centre)
    if kind == "prongs":
        tracks = [cases.segment(c0, tip(d, rng.integers(11, 15))) for d in dirs]
    elif kind == "kink":
        tracks = [cases.segment(c0, tip(d, rng.integers(11, 15))) for d in dirs[:2]]
    else:
        tracks = [cases.segment(tip(-d, rng.integers(11, 15)), c0) | cases.segment(c0, tip(d, rng.integers(11, 15))) for d in dirs[:2]]
    owner = {}
    for k, t in enumerate(tracks):
        for cell in t:
            owner.setdefault(cell, k)
    cells = sorted(owner, key=lambda x: int(np.ravel_multi_index(x, TOY)))
    return cells, np.array([owner[x] for x in cells])


def _toy_scores(kind, seed, radius):
    cells, truth = toy_event(kind, seed)
    index = np.array([int(np.ravel_multi_index(x, TOY)) for x in cells])
    m = index.size
    ids = np.zeros(m, np.int64)                                                        # ONE component: every track touches the others
    spec = ClusterSplitSpec(radius, -0.7, 8, None, 2 * radius)
    w = cluster_split_numpy([0, m], index, ids, [0, 1], [m], TOY, spec)
    whole = cluster_split_numpy([0, m], index, ids, [0, 1], [m], TOY, ClusterSplitSpec(radius, 1.0, m + 1))
    assert whole["events"].tolist() == [[1, 0, 0, 0]]
    assert _connected(cells)
    ch = cluster_chains_numpy([0, m], index, None, w["split"], w["piece_offsets"], TOY,
                              ClusterChainSpec(2 * radius + 2, 0.9, 3, None, False))
    return _ari(ids, truth), _ari(w["split"], truth), _ari(ch["merged"], truth)


TOY_SEEDS = (0, 1, 2)


@pytest.mark.parametrize("radius", [2, 3])
@pytest.mark.parametrize("kind", ["prongs", "kink", "cross"])
def test_the_pieces_are_closer_to_the_particles_than_the_component(kind, radius):
    """Fixed-seed toy events in 40^3, each ONE connected component of two or three true particles, so the adjusted Rand index of
    the component against the truth is exactly 0.  kink_cos -0.7, grow 2 radius.  Measured (seeds 0, 1, 2):
        prongs  radius 2: 0.896 0.895 0.879   radius 3: 0.896 0.895 0.770
        kink    radius 2: 0.800 1.000 0.809   radius 3: 0.800 0.809 0.809
        cross   radius 2: 0.388 0.439 0.485   radius 3: 0.388 0.439 0.485   (four half tracks)
        cross, then cluster_chains_numpy on the pieces (max_gap 2 radius + 2, min_cos 0.9): 0.679 0.729 1.000 at either radius
    Asserted as inequalities only; no threshold is fixed.  (Not every seed holds: a kink flatter than kink_cos is not cut, and the
    chains can also join two prongs of a vertex -- seed 1 of the prongs falls to 0.494 with them.)"""
    for seed in TOY_SEEDS:
        before, pieces, chained = _toy_scores(kind, seed, radius)
        print("%s radius %d seed %d: component %.3f, pieces %.3f, chained %.3f" % (kind, radius, seed, before, pieces, chained))
        assert before == 0.0 and pieces > before, (seed, before, pieces)
        if kind == "cross":
            assert chained > pieces, (seed, pieces, chained)
