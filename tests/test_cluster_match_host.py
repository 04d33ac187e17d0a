"""Cluster matching, host side (no GPU): the appended symbols under an unchanged ABI 9, the scratch query, every argument refusal of
ursn_cluster_match (include/uresnet_hip.h), the ANA_MATCH key and the driver's refusal, set_cluster_matching, and the numpy statement
(uresnet_amd.clusters.cluster_match_numpy) against independent vectorised numpy.  Every library call below is refused on its
arguments before any device access, so the fake pointers are never dereferenced."""
import ctypes
import io
import os
from contextlib import redirect_stdout
from fractions import Fraction

import numpy as np
import pytest

import uresnet_amd  # noqa: F401
from uresnet_amd import _lib, ssnet_config, uresnet
from uresnet_amd.clusters import (MATCH_EVENT_INT, MATCH_EVENT_REAL, MATCH_ROW_INT, MATCH_ROW_REAL, ClusterSpec, cluster_match_numpy,
                                  cluster_numpy)
from uresnet_amd.ssnet import VoxelBatch, match_csv_header, objects_csv_header

FAKE = 0x10000
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _p(a):
    return ctypes.c_void_p(a)


def test_symbols_appended_under_abi_9(lib):
    assert _lib.ABI_VERSION == 9 and lib.ursn_abi_version() == 9
    with open(os.path.join(ROOT, "include", "uresnet_hip.h")) as f:
        hdr = f.read()
    for name in ("ursn_cluster_match_scratch_bytes", "ursn_cluster_match"):
        assert name in _lib.EXPORTS and hasattr(lib, name) and (name + "(") in hdr, name
    assert "#define URSN_ABI_VERSION 9" in hdr and "} ursn_cluster_match_desc;" in hdr and "} ursn_cluster_match_out;" in hdr
    for name in ("I", "R", "EI", "ER"):
        assert "#define URSN_CLMATCH_%s %d " % (name, getattr(_lib, "CLMATCH_" + name)) in hdr, name
    assert (_lib.CLMATCH_I, _lib.CLMATCH_R, _lib.CLMATCH_EI, _lib.CLMATCH_ER) == \
        (len(MATCH_ROW_INT), len(MATCH_ROW_REAL), len(MATCH_EVENT_INT), len(MATCH_EVENT_REAL)) == (8, 4, 12, 4)
    assert ctypes.sizeof(_lib.ursn_cluster_match_desc) == 64 and ctypes.sizeof(_lib.ursn_cluster_match_out) == 112
    # the header ends with this section: nothing before it moved
    assert hdr.index("ursn_cluster_features(") < hdr.index("ursn_cluster_match_scratch_bytes(")


def test_scratch_query(lib):
    """The domain only: at least 8 bytes, 8-byte granular, monotone in every argument inside it, 0 outside; no layout is pinned."""
    q = lib.ursn_cluster_match_scratch_bytes
    ms = (0, 1, 2047, 2048, 2049, 8000, 10 ** 6, 2 ** 31 - 1)
    caps = (0, 1, 8000, 2 ** 31)
    for n in (1, 5, 65535):
        for cap in caps:
            sizes = [q(n, m, cap, cap, cap) for m in ms]
            assert all(b >= 8 and b % 8 == 0 for b in sizes) and sizes == sorted(sizes) and sizes[0] < sizes[-1], (n, cap, sizes)
    for m in ms:
        for k in range(3):
            by_cap = [q(5, m, *[cap if i == k else 100 for i in range(3)]) for cap in caps]
            assert by_cap == sorted(by_cap) and by_cap[0] >= 8, (m, k)
        by_n = [q(n, m, 100, 100, 100) for n in (1, 2, 100, 65535)]
        assert by_n == sorted(by_n), m
    for n, m, ca, cb, pc in ((0, 10, 1, 1, 1), (-1, 10, 1, 1, 1), (65536, 10, 1, 1, 1), (1, -1, 1, 1, 1), (1, 2 ** 31, 1, 1, 1),
                             (1, 2 ** 40, 1, 1, 1), (1, 10, -1, 1, 1), (1, 10, 1, -1, 1), (1, 10, 1, 1, -1)):
        assert q(n, m, ca, cb, pc) == 0, (n, m, ca, cb, pc)


DESC = dict(n=2, m_total=10, offsets=FAKE, cluster_a=FAKE + 0x1000, table_offsets_a=FAKE + 0x2000, cluster_b=FAKE + 0x3000,
            table_offsets_b=FAKE + 0x4000, value=FAKE + 0x5000)
OUT = dict(a_int=FAKE + 0x10000, a_real=FAKE + 0x11000, cap_a=10, b_int=FAKE + 0x12000, b_real=FAKE + 0x13000, cap_b=10,
           event_int=FAKE + 0x14000, event_real=FAKE + 0x15000, pair_offsets=FAKE + 0x16000, pair_b=FAKE + 0x17000,
           pair_n=FAKE + 0x18000, pair_q=FAKE + 0x19000, pair_cap=10, status=FAKE + 0x1a000)
SCRATCH = FAKE + 0x40000


def _refused(lib, text, scratch=SCRATCH, sbytes=1 << 20, null=None, **kw):
    d, o = _lib.ursn_cluster_match_desc(), _lib.ursn_cluster_match_out()
    for k, v in DESC.items():
        setattr(d, k, kw.pop(k, v))
    for k, v in OUT.items():
        setattr(o, k, kw.pop(k, v))
    assert not kw, kw
    rc = lib.ursn_cluster_match(None if null == "desc" else ctypes.byref(d), None if null == "out" else ctypes.byref(o), _p(scratch),
                                sbytes, None)
    msg = lib.ursn_last_error()
    assert rc != 0 and text in msg, (rc, msg)


def test_cluster_match_refusals(lib):
    """Null streams and fake device pointers: a call that got past its checks would fault here, not return."""
    who = b"cluster_match"
    r = lambda text, **kw: _refused(lib, who + text, **kw)
    r(b": null desc / out", null="desc")
    r(b": null desc / out", null="out")
    r(b": n = 0 outside [1, 65535]", n=0)
    r(b": n = 65536 outside [1, 65535]", n=65536)
    r(b": m_total = -1 outside [0, 2^31)", m_total=-1)
    r(b": m_total = 2147483648 outside [0, 2^31)", m_total=2 ** 31)
    r(b": cap_a = -1 < 0", cap_a=-1)
    r(b": cap_b = -2 < 0", cap_b=-2)
    r(b": pair_cap = -1 < 0", pair_cap=-1)
    for name in ("offsets", "table_offsets_a", "table_offsets_b"):
        r(b": null offsets / table_offsets_a / table_offsets_b", **{name: None})
    r(b": null cluster_a / cluster_b", cluster_a=None)
    r(b": null cluster_a / cluster_b", cluster_b=None)
    r(b": null out->status", status=None)
    r(b": null out->event_int / out->event_real", event_int=None)
    r(b": null out->event_int / out->event_real", event_real=None)
    r(b": null out->a_int / out->a_real", a_int=None)
    r(b": null out->a_int / out->a_real", a_real=None)
    r(b": null out->b_int / out->b_real", b_int=None)
    r(b": null out->b_int / out->b_real", b_real=None)
    for name in ("pair_b", "pair_n", "pair_q"):                                    # the three cell arrays: together or not at all
        r(b": out->pair_b / pair_n / pair_q must be given together or not at all", **{name: None})
        r(b": out->pair_b / pair_n / pair_q must be given together or not at all", **{k: None for k in ("pair_b", "pair_n", "pair_q")
                                                                                      if k != name})
    r(b": the cell arrays need out->pair_offsets", pair_offsets=None)
    r(b": null scratch", scratch=None)
    for kw in (dict(offsets=FAKE + 4), dict(table_offsets_a=FAKE + 0x2004), dict(table_offsets_b=FAKE + 0x4004),
               dict(a_int=FAKE + 0x10004), dict(a_real=FAKE + 0x11004), dict(b_int=FAKE + 0x12004), dict(b_real=FAKE + 0x13004),
               dict(event_int=FAKE + 0x14004), dict(event_real=FAKE + 0x15004), dict(pair_offsets=FAKE + 0x16004),
               dict(pair_n=FAKE + 0x18004), dict(pair_q=FAKE + 0x19004), dict(scratch=SCRATCH + 4)):
        r(b": offsets / table offsets / record tables / pair_offsets / pair_n / pair_q / scratch must be 8-byte aligned", **kw)
    for kw in (dict(cluster_a=FAKE + 0x1002), dict(cluster_b=FAKE + 0x3001), dict(value=FAKE + 0x5002), dict(pair_b=FAKE + 0x17002),
               dict(status=FAKE + 0x1a002)):
        r(b": cluster_a / cluster_b / value / pair_b / status must be 4-byte aligned", **kw)
    need = lib.ursn_cluster_match_scratch_bytes(2, 10, 10, 10, 10)
    assert need >= 8
    r(b": scratch of %d bytes is too small, %d needed" % (need - 8, need), sbytes=need - 8)
    r(b": scratch of 0 bytes is too small", sbytes=0)
    big = lib.ursn_cluster_match_scratch_bytes(2, 2 ** 31 - 1, 10, 10, 10)
    r(b": scratch of %d bytes is too small, %d needed" % (big - 8, big), m_total=2 ** 31 - 1, sbytes=big - 8)
    # what is legal passes every argument check: the refusal that comes is the LAST check's, the scratch size
    r(b": scratch of 0 bytes is too small", value=None, sbytes=0)                                         # no value list
    r(b": scratch of 0 bytes is too small", pair_b=None, pair_n=None, pair_q=None, sbytes=0)              # counts only
    r(b": scratch of 0 bytes is too small", pair_b=None, pair_n=None, pair_q=None, pair_offsets=None, sbytes=0)
    r(b": scratch of 0 bytes is too small", cap_a=0, a_int=None, a_real=None, cap_b=0, b_int=None, b_real=None, sbytes=0)
    r(b": scratch of 0 bytes is too small", m_total=0, cluster_a=None, cluster_b=None, sbytes=0)


# ---- config key, driver, Python surface ----------------------------------------------------------------------------------------
def test_config_key_default_off_and_validated(tmp_path):
    c = ssnet_config()
    assert c.ANA_MATCH == ""
    out = io.StringIO()
    with redirect_stdout(out):
        c.dump()
    assert any(line.startswith("ANA_MATCH.") or line.startswith("ANA_MATCH ") for line in out.getvalue().split("\n"))
    p = tmp_path / "a.cfg"
    p.write_text("ANA_MATCH '/tmp/match.csv'\n")
    with redirect_stdout(io.StringIO()):
        c.override(str(p))
    assert c.ANA_MATCH == "/tmp/match.csv" and ssnet_config().ANA_MATCH == ""
    for text in ("ANA_MATCH True\n", "ANA_MATCH 1\n", "ANA_MATCH ['a.csv']\n", "ANA_MATCH None\n"):
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


def test_driver_refuses_ana_match_without_ana_cluster(tmp_path):
    """Before a stream is opened or a device is touched; the file is not created."""
    csv = tmp_path / "match.csv"
    for text in ("TRAIN False\nANA_MATCH '%s'\n" % csv,
                 "TRAIN False\nSPARSE_IO True\nSPARSE_SCORES True\nANA_MATCH '%s'\n" % csv):
        with pytest.raises(ValueError) as e:
            _driver(tmp_path, text).initialize()
        assert "ANA_MATCH" in str(e.value) and "ANA_CLUSTER" in str(e.value), str(e.value)
    assert not csv.exists()
    head = match_csv_header()
    assert head.endswith("\n") and head[:-1].split(",") == ["entry"] + list(MATCH_EVENT_INT) + list(MATCH_EVENT_REAL)
    assert len(head.split(",")) == 17 and len(objects_csv_header().split(",")) == 21          # the objects file is as it was


def test_set_cluster_matching_leaves_want_as_it_was():
    """construct(allocate=False) never touches a device."""
    net = uresnet(dims=[16, 16, 16, 1], num_class=3, base_num_outputs=4, num_strides=2)
    net.construct(trainable=False, use_weight=False, allocate=False)
    vb = VoxelBatch([0, 1], [5], [2.0], [1.0], None, None, 16 ** 3)
    net.set_cluster_matching(True)
    for want in (("cluster",), ("match",), ("pred", "true_cluster")):             # no spec: 'cluster' is unknown, 'match' always is
        with pytest.raises(ValueError, match=r"non-empty subset of \('scores', 'pred', 'ana'\)"):
            net.inference_voxel_scores(None, vb, want=want)
    net.set_clustering(ClusterSpec())
    for call in (lambda: net.inference_voxel_scores(None, vb, want=("softmax",)),
                 lambda: net.inference_voxel_scores(None, vb, want=("cluster", "match")),
                 lambda: net.inference_tiled_voxel_scores(None, vb, (16, 16, 16), want=("clusters",)),
                 lambda: net.inference_tiled_voxel_scores(None, vb, (16, 16, 16), want=("match",))):
        with pytest.raises(ValueError, match=r"non-empty subset of \('scores', 'pred', 'ana', 'cluster'\)"):
            call()
    # matching on, 'cluster' wanted, no labels: refused before anything is fed or launched
    nolabel = VoxelBatch([0, 1], [5], [2.0], None, None, None, 16 ** 3)
    for call in (lambda: net.inference_voxel_scores(None, vb, with_labels=False, want=("pred", "cluster")),
                 lambda: net.inference_voxel_scores(None, nolabel, want=("pred", "cluster")),
                 lambda: net.inference_tiled_voxel_scores(None, nolabel, (16, 16, 16), want=("pred", "cluster"))):
        with pytest.raises(ValueError, match="cluster matching is on and the batch has no labels"):
            call()
    for bad in (1, None, "on"):
        with pytest.raises(ValueError):
            net.set_cluster_matching(bad)
    net.set_cluster_matching(False)


# ---- the statement against independent numpy -----------------------------------------------------------------------------------
CASES = [((12, 10, 14), 6, 0.25, 1), ((12, 10, 14), 26, 0.06, 2), ((9, 16, 11), 18, 0.1, 3), ((20, 24), 4, 0.45, 4),
         ((20, 24), 8, 0.2, 5)]                                    # the shapes of test_cluster_features_host.py
_stat = {}


def _case(k):
    """One random list with random classes, clustered by cluster_numpy under two different specs, and the statement on it
    (computed once, shared, never changed)."""
    if k not in _stat:
        shape, conn, occupancy, seed = CASES[k]
        rng = np.random.default_rng(seed)
        index = np.flatnonzero(rng.uniform(size=int(np.prod(shape))) < occupancy)
        cls = rng.integers(0, 3, index.size).astype(np.uint8)
        value = rng.uniform(0.0, 50.0, index.size).astype(np.float32)
        other = {6: 26, 26: 6, 18: 6, 4: 8, 8: 4}[conn]
        a, fa, _, _ = cluster_numpy(index, cls, shape, ClusterSpec(conn, None, True, 1))
        b, fb, _, _ = cluster_numpy(index, cls, shape, ClusterSpec(other, (0, 1), False, 2))
        m = cluster_match_numpy([0, index.size], a, [0, fa.size], b, [0, fb.size], value)
        for arr in m.values():
            arr.flags.writeable = False
        _stat[k] = (a.astype(np.int64), int(fa.size), b.astype(np.int64), int(fb.size), value, m)
    return _stat[k]


def _sides(a, KA, b, KB, m):
    return (("a", a, KA, b, KB, m["a_int"], m["a_real"], m["b_int"]), ("b", b, KB, a, KA, m["b_int"], m["b_real"], m["a_int"]))


@pytest.mark.parametrize("k", range(len(CASES)))
def test_statement_against_unique_pair_keys(k):
    a, KA, b, KB, value, m = _case(k)
    assert KA > 5 and KB > 2 and (a < 0).any() and (b < 0).any() and ((a >= 0) & (b < 0)).any() and ((a < 0) & (b >= 0)).any()
    q = np.rint(value.astype(np.float64) * 65536.0).astype(np.int64)
    both = (a >= 0) & (b >= 0)
    keys, inv, counts = np.unique(a[both] * KB + b[both], return_inverse=True, return_counts=True)
    cq = np.bincount(inv, weights=q[both], minlength=keys.size).astype(np.int64)        # exact: below 2^53
    ca, cb = keys // KB, keys % KB
    # the cell list: np.unique sorts the keys, which is A row, then B id
    assert np.array_equal(m["pair_offsets"], np.concatenate([[0], np.cumsum(np.bincount(ca, minlength=KA))]))
    assert np.array_equal(m["pair_b"], cb) and np.array_equal(m["pair_n"], counts) and np.array_equal(m["pair_q"], cq)
    assert m["pair_b"].dtype == np.int32 and m["pair_n"].dtype == m["pair_q"].dtype == m["pair_offsets"].dtype == np.int64
    for side, x, KX, y, KY, it, rt, it_y in _sides(a, KA, b, KB, m):
        cx, cy = (ca, cb) if side == "a" else (cb, ca)
        assert it.dtype == np.int64 and rt.dtype == np.float64 and it.shape == (KX, 8) and rt.shape == (KX, 4)
        on = x >= 0
        assert np.array_equal(it[:, 0], np.bincount(x[on], minlength=KX))
        assert np.array_equal(it[:, 1], np.bincount(x[on], weights=q[on], minlength=KX).astype(np.int64))
        assert np.array_equal(it[:, 2], np.bincount(x[both], minlength=KX))
        assert np.array_equal(it[:, 3], np.bincount(cx, minlength=KX))
        packed = np.zeros(KX, np.int64)
        np.maximum.at(packed, cx, (counts << 32) | (0xFFFFFFFF - cy))
        has = it[:, 3] > 0
        assert has.any() and not has.all() or side == "b"
        assert np.array_equal(it[:, 4], np.where(has, 0xFFFFFFFF - (packed & 0xFFFFFFFF), -1))
        assert np.array_equal(it[:, 5], packed >> 32)
        best_q = {(int(r), int(c)): int(v) for r, c, v in zip(cx, cy, cq)}
        assert [int(v) for v in it[:, 6]] == [best_q[(r, int(it[r, 4]))] if has[r] else 0 for r in range(KX)]
        mutual = np.array([bool(has[r]) and int(it_y[it[r, 4], 4]) == r for r in range(KX)])
        assert np.array_equal(it[:, 7], 2 * mutual) and mutual.any()                    # finite values: bit 0 is clear
        n_y = np.where(has, it_y[np.maximum(it[:, 4], 0), 0], 1)
        assert np.array_equal(rt[:, 0], it[:, 5] / it[:, 0])
        assert np.array_equal(rt[:, 1], np.where(has, it[:, 5] / n_y, 0.0))
        assert np.array_equal(rt[:, 2], np.where(has, it[:, 5] / (it[:, 0] + n_y - it[:, 5]), 0.0))
        assert np.array_equal(rt[:, 3], it[:, 2] / it[:, 0])
    pairs2 = lambda v: int((v.astype(object) * (v.astype(object) - 1) // 2).sum())
    N, S, SA, SB = int(both.sum()), pairs2(counts), pairs2(m["a_int"][:, 2]), pairs2(m["b_int"][:, 2])
    ei, er = m["event_int"][0], m["event_real"][0]
    assert [int(v) for v in ei] == [N, S, SA, SB, keys.size, KA, KB, int((m["a_int"][:, 7] >> 1).sum()), int(m["a_int"][:, 5].sum()),
                                    int(m["a_int"][:, 0].sum()), int(m["b_int"][:, 5].sum()), int(m["b_int"][:, 0].sum())]
    assert int((m["b_int"][:, 7] >> 1).sum()) == ei[7]                                  # mutual pairs are pairs: as many B rows
    P = Fraction(N * (N - 1), 2)
    E = Fraction(SA * SB) / P
    ari = float((S - E) / (Fraction(SA + SB, 2) - E))                                   # exact, rounded once
    assert abs(er[0] - ari) <= 1e-12 and er[0] <= 1.0
    assert er[1] == ei[8] / ei[9] and er[2] == ei[10] / ei[11] and er[3] == 2 * ei[7] / (KA + KB)


def test_statement_edges():
    # equal counts: the lowest id wins on both sides; rows with matched = 0; an event without rows on one side; an empty event
    off = [0, 8, 8, 11, 13]
    a = np.array([0, 0, 1, 1, 2, -1, 3, 3, 0, 0, 1, -1, -1])
    b = np.array([1, 0, 0, 1, -1, 2, 1, 0, -1, -1, -1, 0, 0])
    value = np.array([1.5, 2.0 ** 15, np.nan, -2.25, np.inf, 0.5, 0.25, -(2.0 ** 15), 2.0 ** -17, 1.0, 2.0, 3.0, 4.0], np.float32)
    m = cluster_match_numpy(off, a, [0, 4, 4, 6, 6], b, [0, 3, 3, 3, 4], value)
    ai, bi = m["a_int"], m["b_int"]
    assert list(ai[:, 4]) == [0, 0, -1, 0, -1, -1] and list(ai[:, 5]) == [1, 1, 0, 1, 0, 0] and list(ai[:, 3]) == [2, 2, 0, 2, 0, 0]
    assert list(bi[:, 4]) == [0, 0, -1, -1] and list(bi[:, 3]) == [3, 3, 0, 0] and list(bi[:, 2]) == [3, 3, 0, 0]
    assert list(ai[:, 7]) == [3, 1, 1, 1, 0, 0] and list(bi[:, 7]) == [3, 0, 0, 0]     # A0 <-> B0 is the one mutual pair
    assert list(ai[:, 6]) == [0, 0, 0, 0, 0, 0]                                       # A0's best cell holds the dropped 2^15 alone
    assert list(ai[:, 1]) == [int(1.5 * 65536), int(-2.25 * 65536), 0, int(0.25 * 65536), 65536, 2 * 65536]     # 2^-17: to even, 0
    assert list(m["a_real"][2]) == [0.0, 0.0, 0.0, 0.0] and list(m["b_real"][2]) == [0.0, 0.0, 0.0, 0.0]
    assert [list(r) for r in m["event_int"]] == [[6, 0, 3, 6, 6, 4, 3, 1, 3, 7, 2, 7], [0] * 12, [0, 0, 0, 0, 0, 2, 0, 0, 0, 3, 0, 0],
                                                 [0, 0, 0, 0, 0, 0, 1, 0, 0, 0, 0, 2]]
    assert m["event_real"][0][0] == (0.0 - 18.0 / 15.0) / (4.5 - 18.0 / 15.0)
    assert [list(r) for r in m["event_real"][1:]] == [[1.0, 0.0, 0.0, 0.0]] * 3
    assert list(m["pair_offsets"]) == [0, 2, 4, 4, 6, 6, 6] and list(m["pair_b"]) == [0, 1, 0, 1, 0, 1]
    none = cluster_match_numpy(off, a, [0, 4, 4, 6, 6], b, [0, 3, 3, 3, 4])
    assert (none["a_int"][:, [1, 6, ]] == 0).all() and list(none["a_int"][:, 7]) == [2, 0, 0, 0, 0, 0] and (none["pair_q"] == 0).all()
    # identical clusterings: every row mutual, the index exactly 1; one cluster against singletons: den == 0 is not reached, P > 0
    same = cluster_match_numpy([0, 6], [0, 0, 1, 1, 1, 2], [0, 3], [0, 0, 1, 1, 1, 2], [0, 3])
    assert list(same["event_real"][0]) == [1.0, 1.0, 1.0, 1.0] and list(same["event_int"][0][:5]) == [6, 4, 4, 4, 3]
    one = cluster_match_numpy([0, 4], [0, 0, 0, 0], [0, 1], [0, 1, 2, 3], [0, 4])
    assert one["event_real"][0][0] == 0.0 and list(one["a_int"][0]) == [4, 0, 4, 4, 0, 1, 0, 2]
    single = cluster_match_numpy([0, 1], [0], [0, 1], [0], [0, 1])                  # N = 1: P == 0
    assert single["event_real"][0][0] == 1.0
    alike = cluster_match_numpy([0, 3], [0, 0, 0], [0, 1], [0, 0, 0], [0, 1])       # both one cluster: den == 0
    assert alike["event_real"][0][0] == 1.0 and list(alike["event_int"][0][:4]) == [3, 3, 3, 3]
    empty = cluster_match_numpy([0, 0, 0], np.zeros(0, np.int64), [0, 0, 0], np.zeros(0, np.int64), [0, 0, 0])
    assert empty["a_int"].shape == (0, 8) and empty["b_real"].shape == (0, 4) and list(empty["pair_offsets"]) == [0]
    assert [list(r) for r in empty["event_real"]] == [[1.0, 0.0, 0.0, 0.0]] * 2
    for bad_a, ta in (([0, 3, 0, 0], [0, 3]), ([0, -2, 1, 2], [0, 3]), ([0, 1, 1, 0], [0, 3])):   # id == K_e, id < -1, a row without members
        with pytest.raises(ValueError):
            cluster_match_numpy([0, 4], bad_a, ta, [0, 0, 0, 0], [0, 1])
    with pytest.raises(ValueError):
        cluster_match_numpy([0, 4], [0, 0, 0, 0], [0, 1], [0, 0, 0, 0], [0, 1], [1.0])
