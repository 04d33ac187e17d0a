"""Cluster chains, host side (no GPU): the appended symbols under an unchanged ABI 9, the scratch query, every argument refusal of
ursn_cluster_chains (include/uresnet_hip.h), ClusterChainSpec, the ANA_CHAINS / CHAIN_* keys and the driver's refusal,
set_cluster_chains, the arithmetic that puts the GPU test's lattice past the one-step thresholds of csrc/cluster_chain.hip, and the
pure-Python statement (uresnet_amd.clusters.cluster_chains_numpy): hand-built shapes with hand-checked answers, invariants, the
coverage of exactly the lists tests/test_cluster_chain_gpu.py runs (tests/_chain_cases.py makes them for both files), and the value
of the feature against the unbroken truth.  Every library call below is refused on its arguments before any device access, so the
fake pointers are never dereferenced."""
import ctypes
import io
import os
import re
from contextlib import redirect_stdout

import numpy as np
import pytest

import _chain_cases as cases
import uresnet_amd  # noqa: F401
from uresnet_amd import _lib, ssnet_config, uresnet
from uresnet_amd.clusters import (CHAIN_EVENT, CHAIN_INT, CHAIN_REAL, JOIN_INT, JOIN_REAL, ClusterChainSpec, ClusterSpec, chain_cosines,
                                  cluster_chains_numpy, cluster_match_numpy, cluster_numpy)
from uresnet_amd.ssnet import chains_csv_header, chains_csv_row, vertices_csv_header

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
    for name in ("ursn_cluster_chains_scratch_bytes", "ursn_cluster_chains"):
        assert name in _lib.EXPORTS and hasattr(lib, name) and (name + "(") in hdr, name
    assert "#define URSN_ABI_VERSION 9" in hdr and "} ursn_cluster_chain_desc;" in hdr and "} ursn_cluster_chain_out;" in hdr
    for name in ("CI", "CR", "JI", "JR", "EV"):
        assert "#define URSN_CLCHAIN_%s %d " % (name, getattr(_lib, "CLCHAIN_" + name)) in hdr, name
    assert (_lib.CLCHAIN_CI, _lib.CLCHAIN_CR, _lib.CLCHAIN_JI, _lib.CLCHAIN_JR, _lib.CLCHAIN_EV) == \
        (len(CHAIN_INT), len(CHAIN_REAL), len(JOIN_INT), len(JOIN_REAL), len(CHAIN_EVENT)) == (16, 5, 6, 4, 4)
    assert ctypes.sizeof(_lib.ursn_cluster_chain_desc) == 120 and ctypes.sizeof(_lib.ursn_cluster_chain_out) == 144
    # the section stands between the profile's and the vertices': nothing that other tests pin moved
    assert hdr.index("ursn_cluster_profile(") < hdr.index("ursn_cluster_chains_scratch_bytes(") < hdr.index("ursn_cluster_chains(") < \
        hdr.index("ursn_cluster_vertices_scratch_bytes(")
    section = hdr.split("cluster chains: broken track fragments")[1].split("ursn_cluster_vertices_scratch_bytes(")[0]
    for text in ("at most K joins", "|charge| <= 2^62", "dist2 << 32 | key", "m_total is bounded by 2^30", "c_ax = -((u_p[0] * u_q[0]",
                 "consumer's judgement", "URSN_CLCHAIN_WAVE=0", "\"cluster_chains:\""):
        assert text in section, text
    with open(os.path.join(ROOT, "u-resnet_amd", "build.py")) as f:
        assert '"cluster_chain.hip"' in f.read()


def test_scratch_query(lib):
    """The domain only: at least 8 bytes, 8-byte granular, monotone in the list length, 0 outside; no layout is pinned."""
    q = lib.ursn_cluster_chains_scratch_bytes
    ms = (0, 1, 63, 64, 65, 2047, 2048, 2049, 8000, 10 ** 6, 2 ** 30 - 1)
    for n in (1, 5, 65535):
        sizes = [q(n, m) for m in ms]
        assert all(b >= 8 and b % 8 == 0 for b in sizes) and sizes == sorted(sizes) and sizes[0] < sizes[-1], (n, sizes)
    assert q(1, 1000) <= q(5, 1000) <= q(65535, 1000)
    for args in ((0, 10), (-1, 10), (65536, 10), (1, -1), (1, 2 ** 30), (1, 2 ** 40), (1, -2 ** 62)):
        assert q(*args) == 0, args


DESC = dict(ndim=3, n=2, max_gap=6, m_total=10, offsets=FAKE, index=FAKE + 0x1000, cluster=FAKE + 0x2000, table_offsets=FAKE + 0x3000,
            itab=FAKE + 0x5000, rtab=FAKE + 0x6000, feat_cap=10, cls=FAKE + 0x7000, min_cos=0.9, min_size=3, class_mask=6, same_class=1,
            reserved=0)
OUT = dict(merged=FAKE + 0x10000, chain_offsets=FAKE + 0x11000, first=FAKE + 0x12000, size=FAKE + 0x13000, cls=FAKE + 0x14000,
           chain_itab=FAKE + 0x15000, chain_rtab=FAKE + 0x16000, cap_chains=10, join_offsets=FAKE + 0x17000, join_itab=FAKE + 0x18000,
           join_rtab=FAKE + 0x19000, cap_joins=10, row_chain=FAKE + 0x1a000, row_join=FAKE + 0x1b000, row_candidates=FAKE + 0x1c000,
           cap_rows=10, event=FAKE + 0x1d000, status=FAKE + 0x1e000)
SCRATCH = FAKE + 0x40000


def _refused(lib, text, scratch=SCRATCH, sbytes=1 << 20, null=None, spatial=(7, 9, 11), out=None, **kw):
    d, o = _lib.ursn_cluster_chain_desc(), _lib.ursn_cluster_chain_out()
    for k, v in DESC.items():
        setattr(d, k, kw.pop(k, v))
    for i, s in enumerate(spatial):
        d.spatial[i] = s
    for k, v in dict(OUT, **(out or {})).items():
        setattr(o, k, v)
    assert not kw, kw
    rc = lib.ursn_cluster_chains(None if null == "desc" else ctypes.byref(d), None if null == "out" else ctypes.byref(o), _p(scratch),
                                 sbytes, None)
    msg = lib.ursn_last_error()
    assert rc != 0 and msg.startswith(b"cluster_chains:") and text in msg, (rc, msg)


def test_cluster_chains_refusals(lib):
    """Null streams and fake device pointers: a call that got past its checks would fault here, not return."""
    who = b"cluster_chains"
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
    r(b": max_gap = 0 outside [1, 31]", max_gap=0)
    r(b": max_gap = 32 outside [1, 31]", max_gap=32)
    r(b": max_gap = -2147483648 outside [1, 31]", max_gap=-2 ** 31)
    r(b": min_cos = nan outside [0, 1]", min_cos=float("nan"))
    r(b": min_cos = -0.1 outside [0, 1]", min_cos=-0.1)
    r(b": min_cos = 1.5 outside [0, 1]", min_cos=1.5)
    r(b": min_cos = inf outside [0, 1]", min_cos=float("inf"))
    r(b": min_size = 0 < 1", min_size=0)
    r(b": min_size = -5 < 1", min_size=-5)
    r(b": same_class = 2, expected 0 or 1", same_class=2)
    r(b": same_class = -1, expected 0 or 1", same_class=-1)
    r(b": feat_cap = -1 < 0", feat_cap=-1)
    ro(b": cap_rows = -1 < 0", cap_rows=-1)
    ro(b": cap_rows = -9223372036854775808 < 0", cap_rows=-2 ** 63)
    ro(b": cap_chains = -1 < 0", cap_chains=-1)
    ro(b": cap_joins = -1 < 0", cap_joins=-1)
    r(b": null offsets / table_offsets", offsets=None)
    r(b": null offsets / table_offsets", table_offsets=None)
    r(b": null index / cluster", index=None)
    r(b": null index / cluster", cluster=None)
    r(b": null itab / rtab", itab=None)
    r(b": null itab / rtab", rtab=None)
    r(b": class_mask = 0x6 needs cls", cls=None)
    r(b": same_class needs cls", cls=None, class_mask=0)
    ro(b": null out->status", status=None)
    for key in ("chain_offsets", "join_offsets", "event"):
        ro(b": null out->chain_offsets / out->join_offsets / out->event", **{key: None})
    ro(b": null out->merged", merged=None)
    for key in ("chain_itab", "chain_rtab", "first", "size", "cls"):
        ro(b": null out->chain_itab / out->chain_rtab / out->first / out->size / out->cls", **{key: None})
    for key in ("join_itab", "join_rtab"):
        ro(b": null out->join_itab / out->join_rtab", **{key: None})
    for key in ("row_chain", "row_join", "row_candidates"):
        ro(b": null out->row_chain / out->row_join / out->row_candidates", **{key: None})
    r(b": null scratch", scratch=None)
    aligned8 = b": offsets / table_offsets / itab / rtab / the out tables / scratch must be 8-byte aligned"
    for key in ("offsets", "table_offsets", "itab", "rtab"):
        r(aligned8, **{key: DESC[key] + 4})
    for key in ("chain_offsets", "chain_itab", "chain_rtab", "join_offsets", "join_itab", "join_rtab", "event"):
        ro(aligned8, **{key: OUT[key] + 4})
    r(aligned8, scratch=SCRATCH + 4)
    aligned4 = b": index / cluster / merged / first / size / the row arrays / status must be 4-byte aligned"
    for key in ("index", "cluster"):
        r(aligned4, **{key: DESC[key] + 2})
    for key in ("merged", "first", "size", "row_chain", "row_join", "row_candidates"):
        ro(aligned4, **{key: OUT[key] + 2})
    ro(aligned4, status=OUT["status"] + 1)
    need = lib.ursn_cluster_chains_scratch_bytes(2, 10)
    r(b": scratch of %d bytes is too small, %d needed" % (need - 8, need), sbytes=need - 8)
    # legal shapes of a call get as far as the scratch size: no cls; 2-D; the ends of the ranges; no rows / chains / joins / records /
    # entries
    small = b": scratch of 0 bytes is too small"
    r(small, cls=None, class_mask=0, same_class=0, sbytes=0)
    r(small, cls=FAKE + 0x7001, class_mask=0xFFFFFFFF, sbytes=0)                                       # bytes: no alignment asked
    _refused(lib, who + small, out=dict(cls=OUT["cls"] + 1), sbytes=0)
    r(small, ndim=2, spatial=(32768, 32768, -5), sbytes=0)
    r(small, max_gap=1, min_cos=0.0, min_size=1, sbytes=0)
    r(small, max_gap=31, min_cos=1.0, min_size=2 ** 31 - 1, sbytes=0)
    _refused(lib, who + small, out=dict(cap_rows=0, row_chain=None, row_join=None, row_candidates=None), sbytes=0)
    _refused(lib, who + small, out=dict(cap_chains=0, chain_itab=None, chain_rtab=None, first=None, size=None, cls=None), sbytes=0)
    _refused(lib, who + small, out=dict(cap_joins=0, join_itab=None, join_rtab=None), sbytes=0)
    r(small, feat_cap=0, itab=None, rtab=None, sbytes=0)
    _refused(lib, who + small, out=dict(merged=None), m_total=0, index=None, cluster=None, sbytes=0)


def test_cluster_chain_spec_refusals():
    s = ClusterChainSpec()
    assert (s.max_gap, s.min_cos, s.min_size, s.classes, s.same_class) == (6, 0.9, 3, None, True) and s.class_mask() == 0
    assert repr(s) == "ClusterChainSpec(max_gap=6, min_cos=0.9, min_size=3, classes=None, same_class=True)"
    s = ClusterChainSpec(31, 1, 1, {1, 4}, False)
    assert (s.max_gap, s.min_cos, type(s.min_cos), sorted(s.classes), s.class_mask(), s.same_class) == (31, 1.0, float, [1, 4], 18, False)
    assert ClusterChainSpec(1, 0.0, 2 ** 31 - 1, [0, 31]).class_mask() == 0x80000001
    for bad in (0, 32, -1, 6.0, True, "6", None):
        with pytest.raises(ValueError) as e:
            ClusterChainSpec(max_gap=bad)
        assert "max_gap" in str(e.value) and repr(bad) in str(e.value), str(e.value)
    for bad in (-0.1, 1.5, float("nan"), float("inf"), True, "0.9", None):
        with pytest.raises(ValueError) as e:
            ClusterChainSpec(min_cos=bad)
        assert "min_cos" in str(e.value) and repr(bad) in str(e.value), str(e.value)
    for bad in (0, -3, 2 ** 31, 3.0, True, "3", None):
        with pytest.raises(ValueError) as e:
            ClusterChainSpec(min_size=bad)
        assert "min_size" in str(e.value) and repr(bad) in str(e.value), str(e.value)
    for bad in ((), [32], [-1], [1, 1], [1.0], ["1"], [True], 3):
        with pytest.raises(ValueError) as e:
            ClusterChainSpec(classes=bad)
        assert "classes" in str(e.value) and repr(bad) in str(e.value), str(e.value)
    for bad in (0, 1, None, "True"):
        with pytest.raises(ValueError) as e:
            ClusterChainSpec(same_class=bad)
        assert "same_class" in str(e.value) and repr(bad) in str(e.value), str(e.value)
    with pytest.raises(ValueError):
        cluster_chains_numpy([0, 0], [], None, [], [0, 0], (4, 4), 2)
    with pytest.raises(ValueError):
        cluster_chains_numpy([0, 0], [], None, [], [0, 0], (4, 4), ClusterChainSpec(classes=(1,), same_class=False))   # classes need cls
    with pytest.raises(ValueError):
        cluster_chains_numpy([0, 0], [], None, [], [0, 0], (4, 4), ClusterChainSpec())                                 # same_class too
    assert cluster_chains_numpy([0, 0], [], None, [], [0, 0], (4, 4), ClusterChainSpec(same_class=False))["events"].tolist() == [[0, 0, 0, -1]]


# ---- config keys, driver, Python surface ---------------------------------------------------------------------------------------
def test_config_keys_default_off_and_validated(tmp_path):
    c = ssnet_config()
    assert c.ANA_CHAINS == "" and (c.CHAIN_GAP, c.CHAIN_MIN_COS, c.CHAIN_MIN_SIZE, c.CHAIN_CLASSES, c.CHAIN_SAME_CLASS) == (6, 0.9, 3, [], True)
    out = io.StringIO()
    with redirect_stdout(out):
        c.dump()
    keys = ("ANA_CHAINS", "CHAIN_GAP", "CHAIN_MIN_COS", "CHAIN_MIN_SIZE", "CHAIN_CLASSES", "CHAIN_SAME_CLASS")
    for key in keys:
        assert any(line.startswith(key + ".") or line.startswith(key + " ") for line in out.getvalue().split("\n")), key
    p = tmp_path / "a.cfg"
    p.write_text("ANA_CHAINS '/tmp/chains.csv'\nCHAIN_GAP 31\nCHAIN_MIN_COS 0.75\nCHAIN_MIN_SIZE 5\nCHAIN_CLASSES [1, 2]\n"
                 "CHAIN_SAME_CLASS False\n")
    with redirect_stdout(io.StringIO()):
        c.override(str(p))
    assert [getattr(c, k) for k in keys] == ["/tmp/chains.csv", 31, 0.75, 5, [1, 2], False]
    fresh = ssnet_config()
    assert [getattr(fresh, k) for k in keys] == ["", 6, 0.9, 3, [], True]
    for text in ("ANA_CHAINS True\n", "ANA_CHAINS 1\n", "ANA_CHAINS ['a.csv']\n", "ANA_CHAINS None\n", "CHAIN_GAP 0\n", "CHAIN_GAP 32\n",
                 "CHAIN_GAP 6.0\n", "CHAIN_GAP '6'\n", "CHAIN_MIN_COS -0.1\n", "CHAIN_MIN_COS 1.5\n", "CHAIN_MIN_COS '0.9'\n",
                 "CHAIN_MIN_COS float('nan')\n", "CHAIN_MIN_SIZE 0\n", "CHAIN_MIN_SIZE 3.0\n", "CHAIN_MIN_SIZE '3'\n", "CHAIN_CLASSES [32]\n",
                 "CHAIN_CLASSES [1, 1]\n", "CHAIN_CLASSES [1.0]\n", "CHAIN_CLASSES 1\n", "CHAIN_SAME_CLASS 1\n", "CHAIN_SAME_CLASS 'yes'\n"):
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


def test_driver_refuses_ana_chains_without_ana_cluster(tmp_path):
    """Before a stream is opened or a device is touched; the file is not created."""
    csv = tmp_path / "chains.csv"
    for text in ("TRAIN False\nANA_CHAINS '%s'\n" % csv,
                 "TRAIN False\nSPARSE_IO True\nSPARSE_SCORES True\nCHAIN_GAP 12\nANA_CHAINS '%s'\n" % csv):
        with pytest.raises(ValueError) as e:
            _driver(tmp_path, text).initialize()
        assert "ANA_CHAINS" in str(e.value) and "ANA_CLUSTER" in str(e.value), str(e.value)
    assert not csv.exists()
    head = chains_csv_header()
    assert head.endswith("\n") and head[:-1].split(",") == ["entry", "chain"] + list(CHAIN_INT) + list(CHAIN_REAL)
    cols = {name: np.array([3 + c, -(7 + c)], np.int64) for c, name in enumerate(CHAIN_INT)}
    cols.update({name: np.array([0.5, 1.0 / 3.0 + c]) for c, name in enumerate(CHAIN_REAL)})
    cells = chains_csv_row(5, 1, cols)[:-1].split(",")
    assert cells[:18] == ["5", "1"] + [str(-(7 + c)) for c in range(16)]
    assert [float(x) for x in cells[18:]] == [1.0 / 3.0 + c for c in range(5)]
    assert len(vertices_csv_header().split(",")) == 24                                # the vertices file is as it was


def test_set_cluster_chains_leaves_want_as_it_was():
    """construct(allocate=False) never touches a device."""
    net = uresnet(dims=[16, 16, 16, 1], num_class=3, base_num_outputs=4, num_strides=2)
    assert net._want_names() == ("scores", "pred", "ana")
    net.set_cluster_chains(ClusterChainSpec(12))
    assert net._want_names() == ("scores", "pred", "ana")
    net.set_clustering(ClusterSpec())
    assert net._want_names() == ("scores", "pred", "ana", "cluster")
    net.set_cluster_chains(None)
    for bad in (True, 1, 2.0, "2", ClusterSpec()):
        with pytest.raises(ValueError) as e:
            net.set_cluster_chains(bad)
        assert "set_cluster_chains" in str(e.value)
    with pytest.raises(ValueError) as e:
        net.cluster_chains(None, [np.arange(3)], None, {"cluster": [np.zeros(3)], "clusters": [{"first": np.zeros(1)}]}, 5)
    assert "cluster_chains" in str(e.value)


def test_the_lattice_case_crosses_the_one_step_thresholds():
    """The GPU test test_the_lattice_crosses_every_one_step_threshold runs 2,100 three-voxel fragments, ten to a line, followed by
    60,000 entries without a cluster, with max_gap 3 (210 chains of ten rows) and max_gap 2 (nothing in reach: 2,100 chains).  With
    the constants of the source as they are now:"""
    with open(os.path.join(ROOT, "u-resnet_amd", "csrc", "cluster_chain.hip")) as f:
        src = f.read()
    const = {name: int(value) for name, value in re.findall(r"#define (CH_[A-Z_]+) (\d+)\b", src)}
    scan, wave_cap, walk_cap, grid_cap, tile = (const[k] for k in ("CH_SCAN_THREADS", "CH_WAVE_GRID_CAP", "CH_WALK_GRID_CAP",
                                                                  "CH_GRID_CAP", "CH_TILE"))
    assert "const int64_t first = WAVE ? (int64_t)blockIdx.x * 4 : (int64_t)blockIdx.x * 256" in src          # 4 end points per workgroup
    assert "dim3(ch_grid(K, 64, CH_WALK_GRID_CAP)), dim3(64)" in src                                          # 64 chains per workgroup
    shape, index, ids, rows = cases.lattice()
    entries, keys = index.size, 2 * rows
    assert (rows, entries, (ids >= 0).sum()) == (2100, 66300, 6300)
    # the three one-workgroup scans: tiles, rows, keys -- each takes a second chunk, and the last threads take none
    tiles = -(-entries // tile)
    for items, per, busy in ((tiles, 2, 518), (rows, 3, 700), (keys, 5, 840)):
        assert items > scan and -(-items // scan) == per and -(-items // per) == busy < scan, (items, per, busy)
    assert tiles == 1036 and entries % tile == 60                                   # the last tile is ragged too
    # the search: every row is eligible, so there are `keys` end points
    sweep = 4 * wave_cap
    assert sweep < keys < 2 * sweep and (keys - sweep) % 4 == 0 and (keys - sweep) // 4 == 26 < wave_cap     # the second sweep: 26 workgroups
    assert keys > 256 and -(-keys // 256) == 17 < wave_cap                                                   # the plain form: one sweep
    # the chain walk: 64 * 32 chains a sweep
    per_sweep = 64 * walk_cap
    assert per_sweep < rows < 2 * per_sweep and rows - per_sweep == 52 < 64        # max_gap 2: a second sweep of one ragged workgroup
    assert rows // 10 == 210 and -(-210 // 64) == 4 < walk_cap and 210 % 64 == 18  # max_gap 3: four workgroups, the last ragged
    # the striding kernels run several workgroups and stay inside one sweep: crossing their cap takes a list of a million entries
    assert 1 < -(-entries // 256) == 259 < grid_cap and 1 < -(-keys // 256) < grid_cap


# ---- the statement: hand-built shapes ----------------------------------------------------------------------------------------------
ONE = ClusterSpec(26, (1, 2, 3), True)


def _run(scene_, shape, spec, with_cls=True):
    (off, index, ids, toff, tcls), at = scene_
    w = cluster_chains_numpy(off, index, None, ids, toff, shape, spec, tcls if with_cls else None)
    _invariants(w, off, ids, toff)
    return w, ids, toff, at


def _invariants(w, off, ids, toff):
    """Every row in one chain, a row in at most two joins, the joins mutual bests, first strictly increasing, sizes adding up."""
    K, coff, joff = int(toff[-1]), w["chain_offsets"], w["join_offsets"]
    ch, jn, rj, rc, f = w["chains"], w["joins"], w["row_join"], w["row_chain"], w["objects"]
    assert sorted(ch) == sorted(CHAIN_INT + CHAIN_REAL) and sorted(jn) == sorted(JOIN_INT + JOIN_REAL)
    assert all(v.shape == (coff[-1],) for v in ch.values()) and all(v.shape == (joff[-1],) for v in jn.values())
    assert rc.shape == (K,) and rj.shape == (K, 2) and w["row_candidates"].shape == (K, 2) and w["merged"].shape == ids.shape
    assert ((rj >= 0) <= (w["row_candidates"] >= 1)).all() and joff[-1] <= K
    for e in range(len(off) - 1):
        k0, k1, c0, c1 = int(toff[e]), int(toff[e + 1]), int(coff[e]), int(coff[e + 1])
        rows = np.bincount(rc[k0:k1], minlength=c1 - c0)
        assert rc[k0:k1].min(initial=0) >= 0 and np.array_equal(rows, ch["rows"][c0:c1]) and (rows >= 1).all()
        mine, them = ids[off[e]:off[e + 1]], w["merged"][off[e]:off[e + 1]]
        assert ((mine < 0) == (them < 0)).all() and np.array_equal(them[mine >= 0], rc[k0:k1][mine[mine >= 0]])
        t = w["table"]
        assert (np.diff(t["first"][c0:c1]) > 0).all() and t["size"][c0:c1].sum() == (mine >= 0).sum()
        assert np.array_equal(np.bincount(them[them >= 0], minlength=c1 - c0), t["size"][c0:c1])
        for c in range(c0, c1):
            assert t["first"][c] == np.flatnonzero(them == c - c0)[0] and ch["n"][c] == t["size"][c]
        for r in range(k0, k1):
            for side in (0, 1):
                p = rj[r, side]
                if p >= 0:                                                  # mutual, and inside one chain
                    assert rj[k0 + (p >> 1), p & 1] == 2 * (r - k0) + side and rc[k0 + (p >> 1)] == rc[r] and p >> 1 != r - k0
        lower = [(2 * (r - k0) + s, int(rj[r, s])) for r in range(k0, k1) for s in (0, 1) if 0 <= 2 * (r - k0) + s < rj[r, s]]
        assert [(int(a), int(b)) for a, b in zip(jn["key_a"][joff[e]:joff[e + 1]], jn["key_b"][joff[e]:joff[e + 1]])] == lower
        for j in range(joff[e], joff[e + 1]):
            ka, kb = int(jn["key_a"][j]), int(jn["key_b"][j])
            assert jn["pos_a"][j] == f["end_hi" if ka & 1 else "end_lo"][k0 + (ka >> 1)] and jn["chain"][j] == rc[k0 + (ka >> 1)]
            assert jn["pos_b"][j] == f["end_hi" if kb & 1 else "end_lo"][k0 + (kb >> 1)] and jn["gap"][j] == np.sqrt(float(jn["dist2"][j]))
        ev = w["events"][e]
        assert ev[0] == c1 - c0 and ev[1] == joff[e + 1] - joff[e] == ch["joins"][c0:c1].sum() and ev[2] == (ch["rows"][c0:c1] >= 2).sum()
        if c1 > c0:
            pairs = list(zip(ch["rows"][c0:c1], ch["n"][c0:c1]))
            assert pairs.index(max(pairs)) == ev[3]
        else:
            assert ev[3] == -1
    ring = (ch["mask_flags"] >> 32 & 1) == 1
    assert np.array_equal(ch["joins"], ch["rows"] - 1 + ring) and (ch["gaps"] <= ch["path"]).all() and (ch["gap2_max"] <= ch["gap2_sum"]).all()


def test_two_fragments_three_voxels_apart_are_one_chain():
    shape = (16, 16, 16)
    segs = [([(4, 4, c) for c in (1, 2, 3)], 1), ([(4, 4, c) for c in (7, 8, 9)], 1)]
    w, ids, toff, at = _run(cases.scene(shape, [segs], ONE), shape, ClusterChainSpec(6, 0.9, 3))
    ch, jn = w["chains"], w["joins"]
    assert w["chain_offsets"].tolist() == [0, 1] and w["join_offsets"].tolist() == [0, 1] and w["merged"].tolist() == [0] * 6
    assert (ch["rows"][0], ch["joins"][0], ch["n"][0], ch["first_row"][0]) == (2, 1, 6, 0)
    assert (ch["path"][0], ch["gaps"][0], ch["span"][0], ch["straightness"][0], ch["min_cos"][0]) == (8.0, 4.0, 8.0, 1.0, 1.0)   # 2 + 4 + 2
    assert (ch["end_a"][0], ch["end_b"][0], ch["gap2_sum"][0], ch["gap2_max"][0]) == (at(0, (4, 4, 1)), at(0, (4, 4, 9)), 16, 16)
    assert [ch[k][0] for k in ("lo0", "lo1", "lo2", "hi0", "hi1", "hi2")] == [4, 4, 1, 4, 4, 9] and ch["mask_flags"][0] == 2
    assert [jn[k][0] for k in JOIN_INT] == [1, 2, 16, at(0, (4, 4, 3)), at(0, (4, 4, 7)), 0]
    assert [jn[k][0] for k in JOIN_REAL] == [1.0, 1.0, 1.0, 4.0]
    assert w["row_join"].tolist() == [[-1, 2], [1, -1]] and w["row_candidates"].tolist() == [[0, 1], [1, 0]]
    assert w["events"].tolist() == [[1, 1, 1, 0]]
    assert {k: v.tolist() for k, v in w["table"].items()} == {"first": [0], "size": [6], "cls": [1]}
    # a gap beyond max_gap: two chains of one row, each walked from its lo to its hi end
    far = _run(cases.scene(shape, [segs], ONE), shape, ClusterChainSpec(3, 0.9, 3))[0]
    assert far["chain_offsets"].tolist() == [0, 2] and far["merged"].tolist() == [0, 0, 0, 1, 1, 1] and far["join_offsets"][-1] == 0
    assert far["chains"]["path"].tolist() == [2.0, 2.0] and [_bits(x) for x in far["chains"]["min_cos"]] == [0, 0]
    assert far["chains"]["end_a"].tolist() == [0, 3] and far["chains"]["end_b"].tolist() == [2, 5] and far["events"].tolist() == [[2, 0, 0, 0]]


def test_a_perpendicular_end_that_is_nearer_is_not_joined():
    shape = (16, 16, 16)
    segs = [([(4, 4, c) for c in (1, 2, 3)], 1), ([(4, 4, c) for c in (7, 8, 9)], 1), ([(4, b, 5) for b in (6, 7, 8)], 1)]
    w, ids, toff, at = _run(cases.scene(shape, [segs], ONE), shape, ClusterChainSpec(6, 0.9, 3))
    a, b, c = (int(ids[at(0, p)]) for p in ((4, 4, 1), (4, 4, 7), (4, 6, 5)))
    assert w["row_chain"][a] == w["row_chain"][b] != w["row_chain"][c] and w["join_offsets"].tolist() == [0, 1]
    assert w["row_candidates"][c].tolist() == [0, 0] and w["row_join"][c].tolist() == [-1, -1]     # (0, 2, 2) away, nearer than 4: rejected
    assert w["row_candidates"][a].tolist() == [0, 1] and w["row_candidates"][b].tolist() == [1, 0]
    d2, c_ax, c_lo, c_hi = chain_cosines([0.0, 0.0, -1.0], [0.0, 1.0, 0.0], [0, 2, 2])
    assert d2 == 8 and c_ax == 0.0 and c_lo > 0.7 and c_hi > 0.7                                     # the axes are square: c_ax alone


def test_a_best_that_is_not_mutual_is_not_a_join():
    """A's only candidate is B; B's best is C, which is nearer; only B-C join."""
    shape = (16, 16, 16)
    segs = [([(4, 4, c) for c in (0, 1, 2)], 1), ([(4, 4, c) for c in (8, 9, 10)], 1), ([(4, 6, c) for c in (3, 4, 5)], 1)]
    w, ids, toff, at = _run(cases.scene(shape, [segs], ONE), shape, ClusterChainSpec(6, 0.8, 3))
    a, b, c = (int(ids[at(0, p)]) for p in ((4, 4, 0), (4, 4, 8), (4, 6, 3)))
    assert w["row_candidates"][a].tolist() == [0, 1] and w["row_join"][a].tolist() == [-1, -1]       # it chose B; B chose C
    assert w["row_candidates"][b].tolist() == [2, 0] and w["row_join"][b].tolist() == [2 * c + 1, -1]
    assert w["row_join"][c].tolist() == [-1, 2 * b] and w["row_chain"][b] == w["row_chain"][c] != w["row_chain"][a]
    assert w["joins"]["dist2"].tolist() == [13] and w["events"].tolist() == [[2, 1, 1, int(w["row_chain"][b])]]


def test_a_ring_has_no_free_end_and_is_walked_once_round():
    shape = (16, 32, 32)
    w, ids, toff, at = _run(cases.ring(), shape, ClusterChainSpec(4, 0.7, 3, None, False))
    ch = w["chains"]
    assert toff.tolist() == [0, 8] and w["chain_offsets"].tolist() == [0, 1] and (w["row_join"] >= 0).all()
    assert (ch["rows"][0], ch["joins"][0], ch["mask_flags"][0] >> 32, ch["first_row"][0]) == (8, 8, 1, 0)
    f = w["objects"]
    assert ch["end_a"][0] == f["end_lo"][0] and ch["gap2_sum"][0] == 8 * 13 and ch["gap2_max"][0] == 13
    assert abs(ch["gaps"][0] - 8 * np.sqrt(13.0)) < 1e-9 and abs(ch["path"][0] - ch["gaps"][0] - f["length"].sum()) < 1e-9
    assert abs(ch["min_cos"][0] - np.sqrt(0.5)) < 1e-12 and ch["span"][0] == np.sqrt(13.0)   # the walk ends one gap short of its start
    assert ch["straightness"][0] == ch["span"][0] / ch["path"][0]
    # without the diagonal sides' help: at min_cos 0.75 the axes of neighbours (cos 0.707) are refused, eight chains of one
    none = _run(cases.ring(), shape, ClusterChainSpec(4, 0.75, 3, None, False))[0]
    assert none["chain_offsets"].tolist() == [0, 8] and none["join_offsets"].tolist() == [0, 0]


def test_ten_fragments_in_a_line_are_one_chain():
    shape = (8, 8, 64)
    w, ids, toff, at = _run(cases.line(), shape, ClusterChainSpec(4, 0.9, 3, None, False))
    ch = w["chains"]
    assert toff.tolist() == [0, 10, 13] and w["chain_offsets"].tolist() == [0, 1, 2] and w["join_offsets"].tolist() == [0, 9, 11]
    assert ch["rows"].tolist() == [10, 3] and ch["joins"].tolist() == [9, 2] and ch["path"].tolist() == [56.0, 14.0]
    assert ch["span"].tolist() == [56.0, 14.0] and ch["straightness"].tolist() == [1.0, 1.0] and ch["gaps"].tolist() == [36.0, 8.0]
    assert ch["end_a"].tolist() == [0, 30] and ch["end_b"].tolist() == [29, 38] and w["events"].tolist() == [[1, 9, 1, 0], [1, 2, 1, 0]]
    assert w["joins"]["key_a"][:9].tolist() == [1, 3, 5, 7, 9, 11, 13, 15, 17] and w["joins"]["key_b"][:9].tolist() == list(range(2, 20, 2))
    assert w["joins"]["key_a"][9:].tolist() == [1, 3]                                      # event-local keys
    assert w["merged"].tolist() == [0] * 39 and w["table"]["size"].tolist() == [30, 9] and w["table"]["first"].tolist() == [0, 0]


def test_each_guard_breaks_the_join():
    shape = (16, 16, 16)
    segs = [([(4, 4, c) for c in (1, 2, 3)], 1), ([(4, 4, c) for c in (7, 8, 9)], 2)]
    sc = cases.scene(shape, [segs], ONE)
    joins = lambda spec, **kw: int(_run(sc, shape, spec, **kw)[0]["join_offsets"][-1])
    assert joins(ClusterChainSpec(6, 0.9, 3, None, False)) == 1 and joins(ClusterChainSpec(6, 0.9, 3, None, False), with_cls=False) == 1
    assert joins(ClusterChainSpec(6, 0.9, 3, None, True)) == 0                             # same_class
    assert joins(ClusterChainSpec(6, 0.9, 3, (1,), False)) == 0 and joins(ClusterChainSpec(6, 0.9, 3, (1, 2), False)) == 1   # classes
    assert joins(ClusterChainSpec(6, 0.9, 4, None, False)) == 0                            # min_size
    w = _run(sc, shape, ClusterChainSpec(6, 0.9, 3, None, False))[0]
    assert w["chains"]["mask_flags"].tolist() == [6] and w["table"]["cls"].tolist() == [1]
    assert _run(sc, shape, ClusterChainSpec(6, 0.9, 3, None, False), with_cls=False)[0]["table"]["cls"].tolist() == [0]
    # a single voxel has one end position: never eligible, a chain of its own with path 0 and straightness +0.0
    lone = _run(cases.scene(shape, [[([(4, 4, 1)], 1), ([(4, 4, c) for c in (5, 6, 7)], 1)]], ONE), shape, ClusterChainSpec(6, 0.9, 1))[0]
    assert lone["chain_offsets"].tolist() == [0, 2] and lone["chains"]["path"].tolist() == [0.0, 2.0]
    assert _bits(lone["chains"]["straightness"][0]) == 0 and lone["row_candidates"].tolist() == [[0, 0], [0, 0]]


def _random(shape, seed):
    rng = np.random.default_rng(seed)
    vox, occ = int(np.prod(shape)), (0.1 if len(shape) == 3 else 0.45)
    lists = [np.flatnonzero(rng.uniform(size=vox) < occ), np.zeros(0, np.int64), np.flatnonzero(rng.uniform(size=vox) < occ)]
    cls = [rng.integers(0, 3, a.size).astype(np.uint8) for a in lists]
    off = np.concatenate([[0], np.cumsum([a.size for a in lists])])
    tabs = [cluster_numpy(a, c, shape, cases.SPEC) for a, c in zip(lists, cls)]
    ids, toff = np.concatenate([t[0] for t in tabs]), np.concatenate([[0], np.cumsum([t[1].size for t in tabs])])
    table = {k: np.concatenate([t[i] for t in tabs]) for i, k in ((1, "first"), (2, "size"), (3, "cls"))}
    return off, np.concatenate(lists), rng.uniform(0.0, 9.0, off[-1]).astype(np.float32), ids, toff, table


@pytest.mark.parametrize("shape", [(16, 16, 16), (12, 10)])
def test_nothing_merges_at_min_cos_one_on_random_lists(shape):
    """Random clusters are not collinear to the last bit: every row is its own chain and the chains ARE the clusters.  (Two-voxel
    clusters have exact axes, so a 2-D list can hold an exactly collinear pair; seed 4 is one whose lists hold none.)"""
    off, index, value, ids, toff, table = _random(shape, 4)
    w = cluster_chains_numpy(off, index, value, ids, toff, shape, ClusterChainSpec(31, 1.0, 1), table["cls"])
    _invariants(w, off, ids, toff)
    assert toff[-1] > 20 and w["join_offsets"][-1] == 0 and np.array_equal(w["chain_offsets"], toff) and np.array_equal(w["merged"], ids)
    for k in ("first", "size", "cls"):
        assert w["table"][k].dtype == table[k].dtype and np.array_equal(w["table"][k], table[k]), k
    assert np.array_equal(w["chains"]["charge"], w["objects"]["charge"]) and (w["chains"]["charge"] != 0).any()
    loose = cluster_chains_numpy(off, index, value, ids, toff, shape, ClusterChainSpec(6, 0.5, 2), table["cls"])
    _invariants(loose, off, ids, toff)
    assert loose["join_offsets"][-1] > 0


# ---- the statement on the lists of the GPU test -------------------------------------------------------------------------------------
def _single_rejections(w, off, index, toff, tcls, shape, spec):
    """Candidates refused by exactly one of the three cosines, counted per cosine, from the object records alone."""
    f, g, mc = w["objects"], spec.max_gap, np.float64(spec.min_cos)
    ends = []
    for e in range(len(toff) - 1):
        for r in range(toff[e], toff[e + 1]):
            if f["n"][r] >= spec.min_size and f["end_lo"][r] != f["end_hi"][r]:
                for side, p in ((0, f["end_lo"][r]), (1, f["end_hi"][r])):
                    x = [int(v) for v in np.unravel_index(index[p], shape)] + [0] * (3 - len(shape))
                    ends.append((e, r, x, [np.float64(v) if side == 0 else -np.float64(v) for v in f["axis"][r]]))
    alone = [0, 0, 0]
    for i, (e, r, x, u) in enumerate(ends):
        for e2, r2, x2, u2 in ends[i + 1:]:
            d = [b - a for a, b in zip(x, x2)]
            if e2 != e or r2 == r or max(abs(v) for v in d) > g or (spec.same_class and tcls[r] != tcls[r2]):
                continue
            fails = [c < mc for c in chain_cosines(u, u2, d)[1:]]
            if sum(fails) == 1:
                alone[fails.index(True)] += 1
    return alone


def test_the_fixtures_cover_every_decision():
    """The coverage condition of the GPU test's lists, on the statement: it cannot pass on empty tables.  Over the fixtures together
    (min_size 2): at least 4 joins, a chain of at least 3 rows, an end point with at least 2 accepted candidates, a best that is not
    mutual, a candidate refused by each of the three cosines alone, and same_class changing the join set."""
    joins = longest = multi = unrequited = 0
    alone, changed = [0, 0, 0], False
    for name, (shape, _, _, gap, min_cos) in cases.FIXTURES.items():
        off, index, value, cluster, toff, tcls = cases.fixture(name)[:6]
        got = {}
        for same in (True, False):
            spec = ClusterChainSpec(gap, min_cos, 2, None, same)
            w = got[same] = cluster_chains_numpy(off, index, value, cluster, toff, shape, spec, tcls)
            _invariants(w, off, cluster, toff)
            joins += int(w["join_offsets"][-1])
            longest = max(longest, int(w["chains"]["rows"].max()))
            multi += int((w["row_candidates"] >= 2).sum())
            unrequited += int(((w["row_candidates"] >= 1) & (w["row_join"] < 0)).sum())
            alone = [a + b for a, b in zip(alone, _single_rejections(w, off, index, toff, tcls, shape, spec))]
        changed |= got[True]["join_offsets"][-1] != got[False]["join_offsets"][-1]
    assert joins >= 4 and longest >= 3 and multi >= 1 and unrequited >= 1 and min(alone) >= 1 and changed, \
        (joins, longest, multi, unrequited, alone, changed)


def test_chains_are_closer_to_the_unbroken_truth_than_the_fragments():
    """Two toy events with slabs knocked out of every track, max_gap 6, min_cos 0.9, min_size 3 (the default; 1 and 2 give the same
    joins here).  Truth: the clusters of the unbroken lists restricted to the surviving voxels.  In every event the adjusted Rand
    index of the chains against the truth is strictly greater than that of the fragments, and no chain mixes two true objects."""
    shape, _, _, gap, min_cos = cases.FIXTURES["value"]
    off, index, value, cluster, toff, tcls, truth, truth_toff = cases.fixture("value")
    w = cluster_chains_numpy(off, index, value, cluster, toff, shape, ClusterChainSpec(gap, min_cos, 3), tcls)
    before = cluster_match_numpy(off, cluster, toff, truth, truth_toff)
    after = cluster_match_numpy(off, w["merged"], w["chain_offsets"], truth, truth_toff)
    for e in range(len(off) - 1):
        print("event %d: ARI %.6f -> %.6f, efficiency %.6f -> %.6f" % (e, before["event_real"][e, 0], after["event_real"][e, 0],
                                                                        before["event_real"][e, 2], after["event_real"][e, 2]))
        assert after["event_real"][e, 0] > before["event_real"][e, 0]
        rows = after["a_real"][w["chain_offsets"][e]:w["chain_offsets"][e + 1], 0]
        assert rows.size > 0 and rows.mean() == 1.0 and after["event_real"][e, 1] == 1.0
    assert w["join_offsets"][-1] >= 4 and w["chain_offsets"][-1] < toff[-1]


def test_the_statement_raises_on_inconsistent_input(monkeypatch):
    from uresnet_amd import clusters
    shape, spec = (12, 10), ClusterChainSpec(6, 0.9, 1)             # the two rows are (3, 4) apart: cos 0.8
    ok = dict(offsets=[0, 4], index=[1, 2, 35, 36], value=None, cluster=[0, 0, 1, 1], table_offsets=[0, 2], spatial=shape, spec=spec,
              cls=[1, 1])
    assert cluster_chains_numpy(**ok)["chain_offsets"].tolist() == [0, 2]
    for change in (dict(cluster=[0, 0, 2, 2]), dict(table_offsets=[0, 3], cls=[1, 2, 1]), dict(index=[1, 2, 35, 120]),
                   dict(index=[-1, 2, 35, 36]), dict(cls=[1, 32]), dict(cls=[1]), dict(spatial=(12, 10, 4, 4)), dict(offsets=[0, 2])):
        with pytest.raises(ValueError):
            cluster_chains_numpy(**dict(ok, **change))
    real = clusters.cluster_features_numpy

    def moved(*a, **kw):
        f = real(*a, **kw)
        f["end_hi"][0] = 2                                               # a member of the other row
        return f
    monkeypatch.setattr(clusters, "cluster_features_numpy", moved)
    with pytest.raises(ValueError) as e:
        cluster_chains_numpy(**ok)
    assert "not a member" in str(e.value)
