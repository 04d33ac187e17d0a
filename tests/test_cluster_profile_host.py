"""Per-cluster charge profiles, host side (no GPU): the appended symbols under an unchanged ABI 9, the scratch query, every argument
refusal of ursn_cluster_profile (include/uresnet_hip.h), ClusterProfileSpec, the ANA_PROFILES / PROFILE_* keys and the driver's
refusal, set_cluster_profiles, and the pure-Python statement (uresnet_amd.clusters.cluster_profile_numpy): invariants on random lists
and hand-checked shapes.  Every library call below is refused on its arguments before any device access, so the fake pointers are
never dereferenced."""
import ctypes
import io
import os
from contextlib import redirect_stdout

import numpy as np
import pytest

import uresnet_amd  # noqa: F401
from uresnet_amd import _lib, ssnet_config, uresnet
from uresnet_amd.clusters import (PROFILE_BIN_INT, PROFILE_BIN_REAL, PROFILE_ROW_INT, PROFILE_ROW_REAL, ClusterProfileSpec, ClusterSpec,
                                  cluster_numpy, cluster_profile_numpy, profile_bin_count)
from uresnet_amd.ssnet import objects_csv_header, profiles_csv_header, profiles_csv_row

FAKE = 0x10000
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _p(a):
    return ctypes.c_void_p(a)


def test_symbols_appended_under_abi_9(lib):
    assert _lib.ABI_VERSION == 9 and lib.ursn_abi_version() == 9
    with open(os.path.join(ROOT, "include", "uresnet_hip.h")) as f:
        hdr = f.read()
    for name in ("ursn_cluster_profile_scratch_bytes", "ursn_cluster_profile"):
        assert name in _lib.EXPORTS and hasattr(lib, name) and (name + "(") in hdr, name
    assert "#define URSN_ABI_VERSION 9" in hdr and "} ursn_cluster_prof_desc;" in hdr and "} ursn_cluster_prof_out;" in hdr
    for name in ("BI", "BR", "RI", "RR"):
        assert "#define URSN_CLPROF_%s %d " % (name, getattr(_lib, "CLPROF_" + name)) in hdr, name
    assert "#define URSN_CLPROF_BIN_OVERFLOW %d " % _lib.CLPROF_BIN_OVERFLOW in hdr
    assert (_lib.CLPROF_BI, _lib.CLPROF_BR, _lib.CLPROF_RI, _lib.CLPROF_RR) == \
        (len(PROFILE_BIN_INT), len(PROFILE_BIN_REAL), len(PROFILE_ROW_INT), len(PROFILE_ROW_REAL)) == (6, 4, 12, 6)
    assert ctypes.sizeof(_lib.ursn_cluster_prof_desc) == 112 and ctypes.sizeof(_lib.ursn_cluster_prof_out) == 64
    # the header ends with this section: nothing before it moved
    assert hdr.index("ursn_cluster_graph(") < hdr.index("ursn_cluster_profile_scratch_bytes(")
    for text in ("bin n < 2^31", "|d| < 2^46", "|charge| <= 2^62", "nb <= 65536", "nothing more"):
        assert text in hdr.split("per-cluster charge profiles")[1], text


def test_scratch_query(lib):
    """The domain only: at least 8 bytes, 8-byte granular, monotone in the list length and the row cap, 0 outside; no layout is
    pinned."""
    q = lib.ursn_cluster_profile_scratch_bytes
    ms = (0, 1, 2047, 2048, 2049, 8000, 10 ** 6, 2 ** 31 - 1)
    for n in (1, 5, 65535):
        for bins in (0, 1, 10 ** 6, 2 ** 31 - 1):
            sizes = [q(n, m, m, bins) for m in ms]
            assert all(b >= 8 and b % 8 == 0 for b in sizes) and sizes == sorted(sizes) and sizes[0] < sizes[-1], (n, bins, sizes)
            by_cap = [q(n, 8000, cap, bins) for cap in (0, 1, 100, 8000, 2 ** 40)]
            assert by_cap == sorted(by_cap) and by_cap[0] >= 8 and by_cap[-1] == by_cap[-2], (n, bins, by_cap)
    for args in ((0, 10, 1, 1), (-1, 10, 1, 1), (65536, 10, 1, 1), (1, -1, 1, 1), (1, 2 ** 31, 1, 1), (1, 2 ** 40, 1, 1), (1, 10, -1, 1),
                 (1, 10, 1, -1), (1, 10, 1, 2 ** 31), (1, 10, 1, 2 ** 62)):
        assert q(*args) == 0, args


DESC = dict(ndim=3, n=2, m_total=10, offsets=FAKE, index=FAKE + 0x1000, value=FAKE + 0x4000, cluster=FAKE + 0x2000,
            table_offsets=FAKE + 0x3000, itab=FAKE + 0x5000, rtab=FAKE + 0x6000, feat_cap=10, step=1.0, end_bins=3, max_bins=4096)
OUT = dict(bin_offsets=FAKE + 0x10000, bin_itab=FAKE + 0x11000, bin_rtab=FAKE + 0x12000, row_itab=FAKE + 0x13000,
           row_rtab=FAKE + 0x14000, cap_rows=10, bin_cap=64, status=FAKE + 0x17000)
SCRATCH = FAKE + 0x40000


def _refused(lib, text, scratch=SCRATCH, sbytes=1 << 20, null=None, spatial=(7, 9, 11), **kw):
    d, o = _lib.ursn_cluster_prof_desc(), _lib.ursn_cluster_prof_out()
    for k, v in DESC.items():
        setattr(d, k, kw.pop(k, v))
    for i, s in enumerate(spatial):
        d.spatial[i] = s
    for k, v in OUT.items():
        setattr(o, k, kw.pop(k, v))
    assert not kw, kw
    rc = lib.ursn_cluster_profile(None if null == "desc" else ctypes.byref(d), None if null == "out" else ctypes.byref(o), _p(scratch),
                                  sbytes, None)
    msg = lib.ursn_last_error()
    assert rc != 0 and msg.startswith(b"cluster_profile:") and text in msg, (rc, msg)


def test_cluster_profile_refusals(lib):
    """Null streams and fake device pointers: a call that got past its checks would fault here, not return."""
    who = b"cluster_profile"
    r = lambda text, **kw: _refused(lib, who + text, **kw)
    r(b": null desc / out", null="desc")
    r(b": null desc / out", null="out")
    r(b": n = 0 outside [1, 65535]", n=0)
    r(b": n = 65536 outside [1, 65535]", n=65536)
    r(b": m_total = -1 outside [0, 2^31)", m_total=-1)
    r(b": m_total = 2147483648 outside [0, 2^31)", m_total=2 ** 31)
    r(b": ndim = 1, must be 2 or 3", ndim=1)
    r(b": ndim = 4, must be 2 or 3", ndim=4)
    r(b": spatial[0] = 0 outside [1, 32768]", spatial=(0, 9, 11))
    r(b": spatial[1] = 32769 outside [1, 32768]", spatial=(7, 32769, 11))
    r(b": spatial[2] = -1 outside [1, 32768]", spatial=(7, 9, -1))
    r(b": prod(spatial) >= 2^31", spatial=(2048, 1024, 1024))
    for bad in (0.0, 0.49, -1.0, 4096.5, float("inf"), float("-inf"), float("nan"), 1e300):
        r(b": step = ", step=bad)
    r(b": step = 0.25 outside [0.5, 4096]", step=0.25)
    r(b": end_bins = 0 outside [1, 16]", end_bins=0)
    r(b": end_bins = 17 outside [1, 16]", end_bins=17)
    r(b": max_bins = 0 outside [1, 65536]", max_bins=0)
    r(b": max_bins = 65537 outside [1, 65536]", max_bins=65537)
    r(b": max_bins = -2147483648 outside [1, 65536]", max_bins=-2 ** 31)
    r(b": feat_cap = -1 < 0", feat_cap=-1)
    r(b": cap_rows = -1 < 0", cap_rows=-1)
    r(b": cap_rows = -9223372036854775808 < 0", cap_rows=-2 ** 63)
    r(b": bin_cap = -1 outside [0, 2^31)", bin_cap=-1)
    r(b": bin_cap = 2147483648 outside [0, 2^31)", bin_cap=2 ** 31)
    r(b": bin_cap = 9223372036854775807 outside [0, 2^31)", bin_cap=2 ** 63 - 1)
    r(b": null offsets / table_offsets", offsets=None)
    r(b": null offsets / table_offsets", table_offsets=None)
    r(b": null index / cluster", index=None)
    r(b": null index / cluster", cluster=None)
    r(b": null itab / rtab", itab=None)
    r(b": null itab / rtab", rtab=None)
    r(b": null out->status / out->bin_offsets", status=None)
    r(b": null out->status / out->bin_offsets", bin_offsets=None)
    r(b": null out->row_itab / out->row_rtab", row_itab=None)
    r(b": null out->row_itab / out->row_rtab", row_rtab=None)
    r(b": null out->bin_itab / out->bin_rtab", bin_itab=None)
    r(b": null out->bin_itab / out->bin_rtab", bin_rtab=None)
    r(b": null scratch", scratch=None)
    for key in ("offsets", "table_offsets", "itab", "rtab"):
        r(b": offsets / table_offsets / itab / rtab / the out tables / scratch must be 8-byte aligned", **{key: DESC[key] + 4})
    for key in ("bin_offsets", "bin_itab", "bin_rtab", "row_itab", "row_rtab"):
        r(b": offsets / table_offsets / itab / rtab / the out tables / scratch must be 8-byte aligned", **{key: OUT[key] + 4})
    r(b": offsets / table_offsets / itab / rtab / the out tables / scratch must be 8-byte aligned", scratch=SCRATCH + 4)
    for key in ("index", "value", "cluster"):
        r(b": index / value / cluster / status must be 4-byte aligned", **{key: DESC[key] + 2})
    r(b": index / value / cluster / status must be 4-byte aligned", status=OUT["status"] + 1)
    need = lib.ursn_cluster_profile_scratch_bytes(2, 10, 10, 64)
    r(b": scratch of %d bytes is too small, %d needed" % (need - 8, need), sbytes=need - 8)
    # legal shapes of a call get as far as the scratch size: no values; 2-D; the ends of the ranges; no rows / bins / records / entries
    r(b": scratch of 0 bytes is too small", value=None, sbytes=0)
    r(b": scratch of 0 bytes is too small", ndim=2, spatial=(32768, 32768, -5), sbytes=0)
    r(b": scratch of 0 bytes is too small", step=0.5, end_bins=1, max_bins=1, sbytes=0)
    r(b": scratch of 0 bytes is too small", step=4096.0, end_bins=16, max_bins=65536, sbytes=0)
    r(b": scratch of 0 bytes is too small", cap_rows=0, row_itab=None, row_rtab=None, sbytes=0)
    r(b": scratch of 0 bytes is too small", bin_cap=0, bin_itab=None, bin_rtab=None, sbytes=0)
    r(b": scratch of 0 bytes is too small", feat_cap=0, itab=None, rtab=None, sbytes=0)
    r(b": scratch of 0 bytes is too small", m_total=0, index=None, cluster=None, sbytes=0)


def test_cluster_profile_spec_refusals():
    s = ClusterProfileSpec()
    assert (s.step, s.end_bins, s.max_bins) == (1.0, 3, 4096) and repr(s) == "ClusterProfileSpec(step=1.0, end_bins=3, max_bins=4096)"
    s = ClusterProfileSpec(2, 16, 65536)
    assert type(s.step) is float and (s.step, s.end_bins, s.max_bins) == (2.0, 16, 65536)
    assert ClusterProfileSpec(0.5, 1, 1).step == 0.5 and ClusterProfileSpec(4096.0).step == 4096.0
    for bad in (0.0, 0.49, -1.0, 4096.5, float("inf"), float("nan"), "1", None, True, [1.0]):
        with pytest.raises(ValueError) as e:
            ClusterProfileSpec(step=bad)
        assert "step" in str(e.value) and repr(bad) in str(e.value), str(e.value)
    for bad in (0, 17, -1, 3.0, True, "3", None):
        with pytest.raises(ValueError) as e:
            ClusterProfileSpec(end_bins=bad)
        assert "end_bins" in str(e.value) and repr(bad) in str(e.value), str(e.value)
    for bad in (0, 65537, -1, 4096.0, True, "1", None):
        with pytest.raises(ValueError) as e:
            ClusterProfileSpec(max_bins=bad)
        assert "max_bins" in str(e.value) and repr(bad) in str(e.value), str(e.value)
    with pytest.raises(ValueError):
        cluster_profile_numpy([0, 0], [], None, [], [0, 0], (4, 4), 1.0)


# ---- config keys, driver, Python surface ---------------------------------------------------------------------------------------
def test_config_keys_default_off_and_validated(tmp_path):
    c = ssnet_config()
    assert c.ANA_PROFILES == "" and c.PROFILE_STEP == 1.0 and c.PROFILE_END_BINS == 3
    out = io.StringIO()
    with redirect_stdout(out):
        c.dump()
    for key in ("ANA_PROFILES", "PROFILE_STEP", "PROFILE_END_BINS"):
        assert any(line.startswith(key + ".") or line.startswith(key + " ") for line in out.getvalue().split("\n")), key
    p = tmp_path / "a.cfg"
    p.write_text("ANA_PROFILES '/tmp/profiles.csv'\nPROFILE_STEP 2.5\nPROFILE_END_BINS 5\n")
    with redirect_stdout(io.StringIO()):
        c.override(str(p))
    assert (c.ANA_PROFILES, c.PROFILE_STEP, c.PROFILE_END_BINS) == ("/tmp/profiles.csv", 2.5, 5)
    assert (ssnet_config().ANA_PROFILES, ssnet_config().PROFILE_STEP, ssnet_config().PROFILE_END_BINS) == ("", 1.0, 3)
    for text in ("ANA_PROFILES True\n", "ANA_PROFILES 1\n", "ANA_PROFILES ['a.csv']\n", "ANA_PROFILES None\n", "PROFILE_STEP 0.25\n",
                 "PROFILE_STEP 5000.0\n", "PROFILE_STEP 2\n", "PROFILE_STEP '1.0'\n", "PROFILE_STEP [1.0]\n", "PROFILE_END_BINS 0\n",
                 "PROFILE_END_BINS 17\n", "PROFILE_END_BINS 2.0\n", "PROFILE_END_BINS '3'\n"):
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


def test_driver_refuses_ana_profiles_without_ana_cluster(tmp_path):
    """Before a stream is opened or a device is touched; the file is not created."""
    csv = tmp_path / "profiles.csv"
    for text in ("TRAIN False\nANA_PROFILES '%s'\n" % csv,
                 "TRAIN False\nSPARSE_IO True\nSPARSE_SCORES True\nPROFILE_STEP 2.0\nANA_PROFILES '%s'\n" % csv):
        with pytest.raises(ValueError) as e:
            _driver(tmp_path, text).initialize()
        assert "ANA_PROFILES" in str(e.value) and "ANA_CLUSTER" in str(e.value), str(e.value)
    assert not csv.exists()
    head = profiles_csv_header()
    assert head.endswith("\n") and head[:-1].split(",") == ["entry", "cluster"] + list(PROFILE_ROW_INT) + list(PROFILE_ROW_REAL)
    rows = {name: np.array([3 + c, -(7 + c)], np.int64) for c, name in enumerate(PROFILE_ROW_INT)}
    rows.update({name: np.array([0.5, 1.0 / 3.0 + c]) for c, name in enumerate(PROFILE_ROW_REAL)})
    line = profiles_csv_row(5, 1, rows)
    cells = line[:-1].split(",")
    assert cells[:14] == ["5", "1"] + [str(-(7 + c)) for c in range(12)]
    assert [float(x) for x in cells[14:]] == [1.0 / 3.0 + c for c in range(6)]
    assert len(objects_csv_header().split(",")) == 21                                 # the objects file is as it was


def test_set_cluster_profiles_leaves_want_as_it_was():
    """construct(allocate=False) never touches a device."""
    net = uresnet(dims=[16, 16, 16, 1], num_class=3, base_num_outputs=4, num_strides=2)
    assert net._want_names() == ("scores", "pred", "ana")
    net.set_cluster_profiles(ClusterProfileSpec(2.0))
    assert net._want_names() == ("scores", "pred", "ana")
    net.set_clustering(ClusterSpec())
    assert net._want_names() == ("scores", "pred", "ana", "cluster")
    net.set_cluster_profiles(None)
    for bad in (True, 1, 1.0, "1", ClusterSpec()):
        with pytest.raises(ValueError) as e:
            net.set_cluster_profiles(bad)
        assert "set_cluster_profiles" in str(e.value)
    assert net._profile_bin_cap(1000, ClusterProfileSpec(0.5)) == 4501 and net._profile_bin_cap(0, ClusterProfileSpec()) == 1


# ---- the statement ---------------------------------------------------------------------------------------------------------------
def _lists(seed, shape, occupancy, events=2):
    """Random lists, clustered per event by cluster_numpy; a few non-finite and too-large values."""
    rng = np.random.default_rng(seed)
    conn = 26 if len(shape) == 3 else 8
    off, index, ids, value, counts = [0], [], [], [], []
    for _ in range(events):
        idx = np.flatnonzero(rng.uniform(size=int(np.prod(shape))) < occupancy)
        cls = rng.integers(0, 3, idx.size).astype(np.uint8)
        c, first, _, _ = cluster_numpy(idx, cls, shape, ClusterSpec(conn, (1, 2), False))
        index.append(idx), ids.append(c), counts.append(first.size), off.append(off[-1] + idx.size)
        value.append(rng.uniform(-3.0, 40.0, idx.size).astype(np.float32))
    value = np.concatenate(value)
    value[::17] = np.float32(np.inf)
    value[5::29] = np.float32(2.0 ** 15)
    return np.array(off), np.concatenate(index), value, np.concatenate(ids), np.concatenate([[0], np.cumsum(counts)])


@pytest.mark.parametrize("shape,step", [((16, 16, 16), 1.0), ((16, 16, 16), 0.7), ((12, 10), 0.5), ((12, 10), 3.3)])
def test_statement_invariants(shape, step):
    off, index, value, ids, toff = _lists(3, shape, 0.12 if len(shape) == 3 else 0.4)
    spec = ClusterProfileSpec(step, 2, 4096)
    p = cluster_profile_numpy(off, index, value, ids, toff, shape, spec)
    f, rows, bins, boff = p["objects"], p["rows"], p["bins"], p["bin_offsets"]
    K = int(toff[-1])
    assert K > 10 and boff.shape == (K + 1,) and boff[0] == 0 and sorted(rows) == sorted(PROFILE_ROW_INT + PROFILE_ROW_REAL)
    assert sorted(bins) == sorted(PROFILE_BIN_INT + PROFILE_BIN_REAL) and all(v.shape == (boff[-1],) for v in bins.values())
    assert np.array_equal(np.diff(boff), rows["bins"]) and (rows["flags"] & 2 == 0).all() and (rows["flags"] & 1).any()
    for r in range(K):
        lo, hi = boff[r], boff[r + 1]
        nb = hi - lo
        assert nb == profile_bin_count(f["length"][r], step, 4096)[0] == int(np.floor(f["length"][r] / step)) + 1
        assert bins["n"][lo:hi].sum() == f["n"][r] and bins["charge"][lo:hi].sum() == f["charge"][r]
        for a in range(3):
            assert bins["d%d" % a][lo:hi].sum() == f["d"][r][a]
        assert (bins["flags"][lo:hi].max() & 1) == (f["flags"][r] & 1) == (rows["flags"][r] & 1)
        filled = int((bins["n"][lo:hi] > 0).sum())
        assert rows["filled"][r] == filled and filled + int((bins["n"][lo:hi] == 0).sum()) == nb
        assert bins["n"][lo] > 0 and bins["n"][hi - 1] > 0                      # the two end members open and close the profile
        gaps, longest, between = rows["gaps"][r], rows["longest_gap"][r], nb - filled     # both ends are filled: every empty bin lies between
        assert (gaps == 0) == (longest == 0) == (between == 0) and (between == 0 or longest + gaps - 1 <= between <= longest * gaps)
        assert rows["h"][r] == min(2, nb // 2) and 0 <= rows["peak_bin"][r] < nb
        assert rows["head_n"][r] == bins["n"][lo:lo + rows["h"][r]].sum() and rows["tail_n"][r] == bins["n"][hi - rows["h"][r]:hi].sum()
        assert rows["direction"][r] == np.sign(rows["tail_charge"][r] - rows["head_charge"][r]) * (rows["h"][r] > 0)
        empty = bins["n"][lo:hi] == 0
        for name in PROFILE_BIN_REAL:
            assert (bins[name][lo:hi][empty].view(np.uint64) == 0).all()          # +0.0
        assert rows["path"][r] >= 0 and -1.0 - 1e-12 <= rows["min_cos"][r] <= 1.0 + 1e-12
        if filled < 3:
            assert rows["kink_bin"][r] == -1.0 and rows["min_cos"][r] == 1.0
        else:
            assert rows["kink_bin"][r] == -1.0 or bins["n"][lo + int(rows["kink_bin"][r])] > 0


def _one(points, values, shape, spec):
    """One event, one cluster of `points` in the given order of values (the list is sorted by index)."""
    idx = np.ravel_multi_index(np.array(points, np.int64).T, shape)
    order = np.argsort(idx)
    v = None if values is None else np.asarray(values, np.float32)[order]
    p = cluster_profile_numpy([0, idx.size], idx[order], v, np.zeros(idx.size, np.int64), [0, 1], shape, spec)
    return p, {k: x[0] for k, x in p["rows"].items()}


def test_rising_charge_gives_the_direction():
    shape = (16, 16, 16)
    pts = [(3, 4, c) for c in range(2, 14)]
    rise = [1.0 + 0.5 * i for i in range(12)]
    p, row = _one(pts, rise, shape, ClusterProfileSpec(1.0, 3))
    assert row["bins"] == 12 and row["filled"] == 12 and row["gaps"] == 0 and row["h"] == 3 and row["peak_bin"] == 11
    assert list(p["bins"]["n"]) == [1] * 12 and list(p["bins"]["charge"]) == [int(v * 65536) for v in rise]
    assert row["direction"] == 1 and row["head_charge"] == int(4.5 * 65536) and row["tail_charge"] == int(18.0 * 65536)
    assert row["head_dqdx"] == 1.5 and row["tail_dqdx"] == 6.0 and row["path"] == 11.0 and row["straightness"] == 1.0
    assert row["min_cos"] == 1.0 and row["kink_bin"] == 1.0 and row["flags"] == 0
    assert list(p["bins"]["c2"]) == [float(c) for c in range(2, 14)] and list(p["bins"]["dqdx"]) == rise
    _, back = _one(pts, rise[::-1], shape, ClusterProfileSpec(1.0, 3))
    assert back["direction"] == -1 and back["peak_bin"] == 0
    _, flat = _one(pts, [2.0] * 12, shape, ClusterProfileSpec(1.0, 3))
    assert flat["direction"] == 0 and flat["peak_bin"] == 0
    _, none = _one(pts, None, shape, ClusterProfileSpec(1.0, 3))
    assert none["direction"] == 0 and none["head_charge"] == none["tail_charge"] == 0 and none["head_n"] == none["tail_n"] == 3


def test_a_hole_is_a_gap():
    shape = (16, 16, 16)
    pts = [(5, b, 7) for b in range(1, 15) if b not in (6, 7, 8)]
    p, row = _one(pts, [1.0] * len(pts), shape, ClusterProfileSpec(1.0, 3))
    assert row["bins"] == 14 and row["filled"] == 11 and row["gaps"] == 1 and row["longest_gap"] == 3
    assert list(np.flatnonzero(p["bins"]["n"] == 0)) == [5, 6, 7] and row["path"] == 13.0 and row["straightness"] == 1.0
    two = [(5, b, 7) for b in range(1, 15) if b not in (3, 8, 9)]
    _, row = _one(two, [1.0] * len(two), shape, ClusterProfileSpec(1.0, 3))
    assert row["gaps"] == 2 and row["longest_gap"] == 2 and row["filled"] == 11


def test_an_l_shape_bends_at_its_corner():
    shape = (16, 16, 16)
    pts = [(2, 2, c) for c in range(2, 13)] + [(2, b, 12) for b in range(3, 14)]
    p, row = _one(pts, [1.0] * len(pts), shape, ClusterProfileSpec(2.0, 3))
    # a right angle spread over at most three vertices of the polyline turns by 30 degrees or more at one of them: cos <= 0.867
    assert row["min_cos"] < 0.9 and row["straightness"] < 0.95 and row["gaps"] == 0
    kink = int(row["kink_bin"])
    assert kink == row["kink_bin"] and abs(kink - (row["bins"] - 1) / 2.0) <= 1.0     # the corner is the middle of the L
    lo = int(p["bin_offsets"][0])
    corner = np.array([2.0, 2.0, 12.0])
    dist = [np.abs(np.array([p["bins"]["c%d" % a][lo + b] for a in range(3)]) - corner).sum() for b in range(int(row["bins"]))]
    assert abs(int(np.argmin(dist)) - kink) <= 1
    _, line = _one([(2, 2, c) for c in range(2, 13)], [1.0] * 11, shape, ClusterProfileSpec(2.0, 3))
    # 11 voxels in bins of 2: the polyline runs between the centroids of the two end bins, 0.5 short of the length
    assert line["min_cos"] == 1.0 and line["path"] == 9.5 and line["straightness"] == 10.0 / 9.5


def test_a_single_voxel_and_a_truncated_profile():
    shape = (12, 10)
    p, row = _one([(4, 5)], [3.0], shape, ClusterProfileSpec(1.0, 3))
    assert row["bins"] == 1 and row["h"] == 0 and row["direction"] == 0 and row["filled"] == 1 and row["path"] == 0.0
    assert row["head_dqdx"] == 0.0 and row["tail_dqdx"] == 0.0 and row["min_cos"] == 1.0 and row["kink_bin"] == -1.0
    assert row["straightness"] == 1.0 and list(p["bin_offsets"]) == [0, 1] and p["bins"]["dqdx"][0] == 3.0
    assert (p["bins"]["c0"][0], p["bins"]["c1"][0], p["bins"]["c2"][0]) == (4.0, 5.0, 0.0)
    pts = [(3, c) for c in range(10)]
    full, row = _one(pts, [1.0] * 10, shape, ClusterProfileSpec(1.0, 3, 10))
    assert row["bins"] == 10 and row["flags"] == 0
    cut, row = _one(pts, [1.0] * 10, shape, ClusterProfileSpec(1.0, 3, 4))
    assert row["bins"] == 4 and row["flags"] == 2 and list(cut["bins"]["n"]) == [1, 1, 1, 7] and row["h"] == 2
    assert row["tail_n"] == 8 and row["direction"] == 1 and list(cut["bin_offsets"]) == [0, 4]


def test_the_statement_raises_on_inconsistent_input():
    shape, spec = (12, 10), ClusterProfileSpec()
    ok = dict(offsets=[0, 3], index=[1, 2, 3], value=None, cluster=[0, 0, 1], table_offsets=[0, 2], spatial=shape, spec=spec)
    assert cluster_profile_numpy(**ok)["bin_offsets"].tolist() == [0, 2, 3]
    for change in (dict(cluster=[0, 0, 2]), dict(table_offsets=[0, 3]), dict(index=[1, 2, 120]), dict(index=[1, 2, -1])):
        with pytest.raises(ValueError):
            cluster_profile_numpy(**dict(ok, **change))
    assert cluster_profile_numpy(**dict(ok, cluster=[0, 0, -1], index=[1, 2, 500], table_offsets=[0, 1]))["rows"]["bins"].tolist() == [2]
