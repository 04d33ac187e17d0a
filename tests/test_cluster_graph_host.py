"""Cluster contact graph, host side (no GPU): the appended symbols under an unchanged ABI 9, the scratch query, every argument
refusal of ursn_cluster_graph (include/uresnet_hip.h), ClusterGraphSpec, the ANA_GRAPH / GRAPH_GAP keys and the driver's refusal,
set_cluster_graph, and the pure-Python statement (uresnet_amd.clusters.cluster_graph_numpy) against an independent brute-force numpy
statement.  Every library call below is refused on its arguments before any device access, so the fake pointers are never
dereferenced."""
import ctypes
import io
import os
from contextlib import redirect_stdout

import numpy as np
import pytest

import uresnet_amd  # noqa: F401
from uresnet_amd import _lib, ssnet_config, uresnet
from uresnet_amd.clusters import (GRAPH_EDGE, GRAPH_EVENT, GRAPH_GROUP, GRAPH_ROW, ClusterGraphSpec, ClusterSpec, cluster_graph_numpy,
                                  cluster_numpy)
from uresnet_amd.ssnet import graph_csv_header, graph_csv_row, match_csv_header

FAKE = 0x10000
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _p(a):
    return ctypes.c_void_p(a)


def test_symbols_appended_under_abi_9(lib):
    assert _lib.ABI_VERSION == 9 and lib.ursn_abi_version() == 9
    with open(os.path.join(ROOT, "include", "uresnet_hip.h")) as f:
        hdr = f.read()
    for name in ("ursn_cluster_graph_scratch_bytes", "ursn_cluster_graph"):
        assert name in _lib.EXPORTS and hasattr(lib, name) and (name + "(") in hdr, name
    assert _lib.EXPORTS[-2:] == ("ursn_cluster_graph_scratch_bytes", "ursn_cluster_graph")
    assert "#define URSN_ABI_VERSION 9" in hdr and "} ursn_cluster_graph_desc;" in hdr and "} ursn_cluster_graph_out;" in hdr
    for name in ("E", "I", "G", "EV"):
        assert "#define URSN_CLGRAPH_%s %d " % (name, getattr(_lib, "CLGRAPH_" + name)) in hdr, name
    assert "#define URSN_CLGRAPH_EDGE_OVERFLOW %d " % _lib.CLGRAPH_EDGE_OVERFLOW in hdr
    assert (_lib.CLGRAPH_E, _lib.CLGRAPH_I, _lib.CLGRAPH_G, _lib.CLGRAPH_EV) == \
        (len(GRAPH_EDGE), len(GRAPH_ROW), len(GRAPH_GROUP), len(GRAPH_EVENT)) == (6, 6, 12, 4)
    assert ctypes.sizeof(_lib.ursn_cluster_graph_desc) == 88 and ctypes.sizeof(_lib.ursn_cluster_graph_out) == 88
    # the header ends with this section: nothing before it moved
    assert hdr.index("ursn_cluster_match(") < hdr.index("ursn_cluster_graph_scratch_bytes(")
    for text in ("pairs < m_total * 171 < 2^39", "dist2 <= 3 * 3^2 = 27", "below 2^15", "2^62"):
        assert text in hdr.split("cluster contact graph")[1], text


def test_scratch_query(lib):
    """The domain only: at least 8 bytes, 8-byte granular, monotone in every argument inside it, 0 outside; no layout is pinned."""
    q = lib.ursn_cluster_graph_scratch_bytes
    ms = (0, 1, 2047, 2048, 2049, 8000, 10 ** 6, 2 ** 31 - 1)
    caps = (0, 1, 8000, 2 ** 31)
    ecaps = (0, 1, 1023, 1024, 8000, 10 ** 6, 2 ** 30 - 1)
    for n in (1, 5, 65535):
        for cap in caps:
            sizes = [q(n, m, cap, cap, 100) for m in ms]
            assert all(b >= 8 and b % 8 == 0 for b in sizes) and sizes == sorted(sizes) and sizes[0] < sizes[-1], (n, cap, sizes)
    for m in ms:
        for k in range(2):
            by_cap = [q(5, m, *([cap if i == k else 100 for i in range(2)] + [100])) for cap in caps]
            assert by_cap == sorted(by_cap) and by_cap[0] >= 8, (m, k)
        by_edges = [q(5, m, 100, 100, c) for c in ecaps]
        assert all(b >= 8 and b % 8 == 0 for b in by_edges) and by_edges == sorted(by_edges) and by_edges[0] < by_edges[-1], m
        by_n = [q(n, m, 100, 100, 100) for n in (1, 2, 100, 65535)]
        assert by_n == sorted(by_n), m
    for args in ((0, 10, 1, 1, 1), (-1, 10, 1, 1, 1), (65536, 10, 1, 1, 1), (1, -1, 1, 1, 1), (1, 2 ** 31, 1, 1, 1),
                 (1, 2 ** 40, 1, 1, 1), (1, 10, -1, 1, 1), (1, 10, 1, -1, 1), (1, 10, 1, 1, -1), (1, 10, 1, 1, 2 ** 30),
                 (1, 10, 1, 1, 2 ** 62)):
        assert q(*args) == 0, args


DESC = dict(ndim=3, n=2, gap=1, m_total=10, edge_cap=16, offsets=FAKE, index=FAKE + 0x1000, cluster=FAKE + 0x2000,
            table_offsets=FAKE + 0x3000, value=FAKE + 0x4000, cls=FAKE + 0x5001)
OUT = dict(rows=FAKE + 0x10000, cap_rows=10, groups=FAKE + 0x11000, cap_groups=10, group_offsets=FAKE + 0x12000, event=FAKE + 0x13000,
           group=FAKE + 0x14000, edge_offsets=FAKE + 0x15000, edges=FAKE + 0x16000, edge_out_cap=16, status=FAKE + 0x17000)
SCRATCH = FAKE + 0x40000


def _refused(lib, text, scratch=SCRATCH, sbytes=1 << 20, null=None, spatial=(7, 9, 11), **kw):
    d, o = _lib.ursn_cluster_graph_desc(), _lib.ursn_cluster_graph_out()
    for k, v in DESC.items():
        setattr(d, k, kw.pop(k, v))
    for i, s in enumerate(spatial):
        d.spatial[i] = s
    for k, v in OUT.items():
        setattr(o, k, kw.pop(k, v))
    assert not kw, kw
    rc = lib.ursn_cluster_graph(None if null == "desc" else ctypes.byref(d), None if null == "out" else ctypes.byref(o), _p(scratch),
                                sbytes, None)
    msg = lib.ursn_last_error()
    assert rc != 0 and msg.startswith(b"cluster_graph:") and text in msg, (rc, msg)


def test_cluster_graph_refusals(lib):
    """Null streams and fake device pointers: a call that got past its checks would fault here, not return."""
    who = b"cluster_graph"
    r = lambda text, **kw: _refused(lib, who + text, **kw)
    r(b": null desc / out", null="desc")
    r(b": null desc / out", null="out")
    r(b": n = 0 outside [1, 65535]", n=0)
    r(b": n = 65536 outside [1, 65535]", n=65536)
    r(b": m_total = -1 outside [0, 2^31)", m_total=-1)
    r(b": m_total = 2147483648 outside [0, 2^31)", m_total=2 ** 31)
    r(b": ndim = 1, expected 2 or 3", ndim=1)
    r(b": ndim = 4, expected 2 or 3", ndim=4)
    r(b": spatial[0] = 0 outside [1, 32768]", spatial=(0, 9, 11))
    r(b": spatial[1] = 32769 outside [1, 32768]", spatial=(7, 32769, 11))
    r(b": spatial[2] = -1 outside [1, 32768]", spatial=(7, 9, -1))
    r(b": 2147483648 voxels, expected fewer than 2^31", spatial=(2048, 1024, 1024))
    r(b": gap = 0 outside [1, 3]", gap=0)
    r(b": gap = 4 outside [1, 3]", gap=4)
    r(b": gap = -2147483648 outside [1, 3]", gap=-2 ** 31)
    r(b": edge_cap = -1 outside [0, 2^30)", edge_cap=-1)
    r(b": edge_cap = 1073741824 outside [0, 2^30)", edge_cap=2 ** 30)
    r(b": edge_cap = 9223372036854775807 outside [0, 2^30)", edge_cap=2 ** 63 - 1)
    r(b": cap_rows = -1 < 0", cap_rows=-1)
    r(b": cap_groups = -2 < 0", cap_groups=-2)
    r(b": edge_out_cap = -9223372036854775808 < 0", edge_out_cap=-2 ** 63)
    r(b": null offsets / table_offsets", offsets=None)
    r(b": null offsets / table_offsets", table_offsets=None)
    r(b": null index / cluster", index=None)
    r(b": null index / cluster", cluster=None)
    r(b": null out->status", status=None)
    r(b": null out->group_offsets / out->event", group_offsets=None)
    r(b": null out->group_offsets / out->event", event=None)
    r(b": null out->group", group=None)
    r(b": null out->rows", rows=None)
    r(b": null out->groups", groups=None)
    r(b": out->edges needs out->edge_offsets", edge_offsets=None)
    r(b": edge_out_cap = 16 with null out->edges", edges=None)
    r(b": null scratch", scratch=None)
    for kw in (dict(offsets=FAKE + 4), dict(table_offsets=FAKE + 0x3004), dict(rows=FAKE + 0x10004), dict(groups=FAKE + 0x11004),
               dict(group_offsets=FAKE + 0x12004), dict(event=FAKE + 0x13004), dict(edge_offsets=FAKE + 0x15004),
               dict(edges=FAKE + 0x16004), dict(scratch=SCRATCH + 4)):
        r(b": offsets / table_offsets / rows / groups / group_offsets / event / edge_offsets / edges / scratch must be 8-byte", **kw)
    for kw in (dict(index=FAKE + 0x1002), dict(cluster=FAKE + 0x2001), dict(value=FAKE + 0x4002), dict(group=FAKE + 0x14002),
               dict(status=FAKE + 0x17002)):
        r(b": index / cluster / value / group / status must be 4-byte aligned", **kw)
    need = lib.ursn_cluster_graph_scratch_bytes(2, 10, 10, 10, 16)
    assert need >= 8
    r(b": scratch of %d bytes is too small, %d needed" % (need - 8, need), sbytes=need - 8)
    r(b": scratch of 0 bytes is too small", sbytes=0)
    big = lib.ursn_cluster_graph_scratch_bytes(2, 2 ** 31 - 1, 10, 10, 2 ** 30 - 1)
    r(b": scratch of %d bytes is too small, %d needed" % (big - 8, big), m_total=2 ** 31 - 1, edge_cap=2 ** 30 - 1, sbytes=big - 8)
    # what is legal passes every argument check: the refusal that comes is the LAST check's, the scratch size
    r(b": scratch of 0 bytes is too small", value=None, cls=None, sbytes=0)
    r(b": scratch of 0 bytes is too small", ndim=2, spatial=(32768, 32768, 0), gap=3, sbytes=0)
    r(b": scratch of 0 bytes is too small", edges=None, edge_out_cap=0, sbytes=0)                      # counts only
    r(b": scratch of 0 bytes is too small", edges=None, edge_offsets=None, edge_out_cap=0, sbytes=0)   # no edge list
    r(b": scratch of 0 bytes is too small", cap_rows=0, rows=None, cap_groups=0, groups=None, sbytes=0)
    r(b": scratch of 0 bytes is too small", m_total=0, index=None, cluster=None, group=None, sbytes=0)
    r(b": scratch of 0 bytes is too small", edge_cap=0, sbytes=0)


def test_cluster_graph_spec_refusals():
    assert ClusterGraphSpec().gap == 1 and ClusterGraphSpec(3).gap == 3 and repr(ClusterGraphSpec(2)) == "ClusterGraphSpec(gap=2)"
    for bad in (0, 4, -1, 1.0, True, "1", None, [1]):
        with pytest.raises(ValueError) as e:
            ClusterGraphSpec(bad)
        assert repr(bad) in str(e.value), str(e.value)
    with pytest.raises(ValueError):
        cluster_graph_numpy([0, 0], [], [], [0, 0], (4, 4), spec=1)


# ---- config keys, driver, Python surface ---------------------------------------------------------------------------------------
def test_config_keys_default_off_and_validated(tmp_path):
    c = ssnet_config()
    assert c.ANA_GRAPH == "" and c.GRAPH_GAP == 1
    out = io.StringIO()
    with redirect_stdout(out):
        c.dump()
    for key in ("ANA_GRAPH", "GRAPH_GAP"):
        assert any(line.startswith(key + ".") or line.startswith(key + " ") for line in out.getvalue().split("\n")), key
    p = tmp_path / "a.cfg"
    p.write_text("ANA_GRAPH '/tmp/graph.csv'\nGRAPH_GAP 3\n")
    with redirect_stdout(io.StringIO()):
        c.override(str(p))
    assert c.ANA_GRAPH == "/tmp/graph.csv" and c.GRAPH_GAP == 3 and ssnet_config().ANA_GRAPH == "" and ssnet_config().GRAPH_GAP == 1
    for text in ("ANA_GRAPH True\n", "ANA_GRAPH 1\n", "ANA_GRAPH ['a.csv']\n", "ANA_GRAPH None\n", "GRAPH_GAP 0\n", "GRAPH_GAP 4\n",
                 "GRAPH_GAP 2.0\n", "GRAPH_GAP [1]\n", "GRAPH_GAP '1'\n"):
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


def test_driver_refuses_ana_graph_without_ana_cluster(tmp_path):
    """Before a stream is opened or a device is touched; the file is not created."""
    csv = tmp_path / "graph.csv"
    for text in ("TRAIN False\nANA_GRAPH '%s'\n" % csv,
                 "TRAIN False\nSPARSE_IO True\nSPARSE_SCORES True\nGRAPH_GAP 2\nANA_GRAPH '%s'\n" % csv):
        with pytest.raises(ValueError) as e:
            _driver(tmp_path, text).initialize()
        assert "ANA_GRAPH" in str(e.value) and "ANA_CLUSTER" in str(e.value), str(e.value)
    assert not csv.exists()
    head = graph_csv_header()
    assert head.endswith("\n") and head[:-1].split(",") == ["entry", "group"] + list(GRAPH_GROUP)
    groups = {name: np.array([3 + c, -(7 + c)], np.int64) for c, name in enumerate(GRAPH_GROUP)}
    assert graph_csv_row(5, 1, groups) == ",".join(["5", "1"] + [str(-(7 + c)) for c in range(12)]) + "\n"
    assert len(match_csv_header().split(",")) == 17                                   # the match file is as it was


def test_set_cluster_graph_leaves_want_as_it_was():
    """construct(allocate=False) never touches a device."""
    net = uresnet(dims=[16, 16, 16, 1], num_class=3, base_num_outputs=4, num_strides=2)
    assert net._want_names() == ("scores", "pred", "ana")
    net.set_cluster_graph(ClusterGraphSpec(2))
    assert net._want_names() == ("scores", "pred", "ana")
    net.set_clustering(ClusterSpec())
    assert net._want_names() == ("scores", "pred", "ana", "cluster")
    net.set_cluster_graph(None)
    for bad in (True, 1, "1", ClusterSpec()):
        with pytest.raises(ValueError) as e:
            net.set_cluster_graph(bad)
        assert "set_cluster_graph" in str(e.value)


# ---- the statement against an independent brute-force statement ---------------------------------------------------------------
def _brute(off, index, ids, toff, spatial, gap, value, cls):
    """O(m^2) broadcasting of coordinate differences per event, np.unique on pair keys, a plain union-find.  Shares no code and no
    data structure with cluster_graph_numpy."""
    n, K = len(off) - 1, int(toff[-1])
    nd = len(spatial)
    E = {}
    for e in range(n):
        lo, hi = off[e], off[e + 1]
        idx, cid = index[lo:hi], ids[lo:hi]
        x = np.stack(np.unravel_index(idx, spatial), 1).astype(np.int64) if hi > lo else np.zeros((0, nd), np.int64)
        diff = np.abs(x[:, None, :] - x[None, :, :])
        cheb, d2 = diff.max(2) if hi > lo else np.zeros((0, 0), np.int64), (diff * diff).sum(2)
        near = (cheb <= gap) & (cid[:, None] >= 0) & (cid[None, :] >= 0) & (cid[:, None] < cid[None, :])    # i in a, j in b
        i, j = np.nonzero(near)
        if i.size == 0:
            continue
        key = (toff[e] + cid[i]) * K + (toff[e] + cid[j])
        uniq, inv = np.unique(key, return_inverse=True)
        pairs = np.bincount(inv, minlength=uniq.size)
        touch = np.bincount(inv, weights=(cheb[i, j] == 1), minlength=uniq.size).astype(np.int64)
        order = np.lexsort((j, i, d2[i, j], inv))              # by edge, then dist2, then position in a, then position in b
        firsts = order[np.concatenate([[True], inv[order][1:] != inv[order][:-1]])]
        for u in range(uniq.size):
            f = firsts[u]
            E[(int(uniq[u] // K), int(uniq[u] % K))] = (int(pairs[u]), int(touch[u]), int(d2[i[f], j[f]]), int(lo + i[f]), int(lo + j[f]))
    parent = np.arange(K)

    def find(r):
        while parent[r] != r:
            r = parent[r]
        return r

    for a, b in E:
        ra, rb = find(a), find(b)
        parent[max(ra, rb)] = min(ra, rb)
    root = np.array([find(r) for r in range(K)], np.int64)
    event_of = np.repeat(np.arange(n), np.diff(toff))
    keys = sorted(E)
    edges = np.array([[b - toff[event_of[a]]] + list(E[(a, b)]) for a, b in keys], np.int64).reshape(-1, 6)
    edge_offsets = np.concatenate([[0], np.cumsum(np.bincount([a for a, _ in keys], minlength=K))]).astype(np.int64)
    rows = np.zeros((K, 6), np.int64)
    rows[:, 2] = -1
    for r in range(K):
        mine = [(E[k][2], k[0] + k[1] - r, E[k][0], E[k][1]) for k in keys if r in k]
        if mine:
            rows[r] = [len(mine), 0, min(mine)[1] - toff[event_of[r]], min(mine)[0], sum(p[2] for p in mine), sum(p[3] > 0 for p in mine)]
    heads = np.flatnonzero(root == np.arange(K))               # ascending lowest row = the numbering
    gid = np.searchsorted(heads, root)
    group_offsets = np.searchsorted(heads, toff).astype(np.int64)
    rows[:, 1] = gid - group_offsets[event_of]
    groups = np.zeros((heads.size, 12), np.int64)
    group = np.full(index.size, -1, np.int32)
    row_of = np.where(ids >= 0, toff[np.repeat(np.arange(n), np.diff(off))] + ids, -1)
    coords = np.zeros((index.size, 3), np.int64)
    coords[:, :nd] = np.stack(np.unravel_index(np.where(ids >= 0, index, 0), spatial), 1)
    q = np.zeros(index.size, object)
    bad = np.zeros(index.size, bool)
    if value is not None:
        v = value.astype(np.float64)
        bad = ~np.isfinite(v) | (np.abs(v) >= 2.0 ** 15)
        q = np.array([0 if b else int(np.rint(s * 65536.0)) for s, b in zip(v, bad)], object)
    for g, h in enumerate(heads):
        members = np.flatnonzero(root == h)
        ent = np.flatnonzero(np.isin(row_of, members))
        group[ent] = g - group_offsets[event_of[h]]
        mask = 0 if cls is None else int(np.bitwise_or.reduce(1 << cls[members].astype(np.int64)))
        groups[g] = [members.size, sum(1 for a, _ in keys if root[a] == h), ent.size, int(sum(q[ent])), *coords[ent].min(0),
                     *coords[ent].max(0), h - toff[event_of[h]], mask | (int(bad[ent].any()) << 32)]
    events = np.zeros((n, 4), np.int64)
    for e in range(n):
        g = groups[group_offsets[e]:group_offsets[e + 1]]
        r = rows[toff[e]:toff[e + 1]]
        events[e] = [g.shape[0], g[:, 1].sum(), (r[:, 0] == 0).sum(), g[:, 2].max() if g.size else 0]
    return {"edge_offsets": edge_offsets, "edges": edges, "rows": rows, "group_offsets": group_offsets, "groups": groups,
            "events": events, "group": group}


def _random_case(rng, spatial, sizes, empty_cluster_event):
    """Random sorted lists clustered by cluster_numpy per class; event `empty_cluster_event` has entries, none in a cluster."""
    vox = int(np.prod(spatial))
    lists = [np.sort(rng.choice(vox, size=s, replace=False)) for s in sizes]
    off = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64)
    index = np.concatenate(lists).astype(np.int64)
    ids, counts, tcls = [], [], []
    for e, l in enumerate(lists):
        c = rng.integers(0, 4, l.size).astype(np.uint8)
        if e == empty_cluster_event:
            c[:] = 0
        cid, first, _, kc = cluster_numpy(l, c, spatial, ClusterSpec(None, (1, 2, 3), True, 1))
        ids.append(cid), counts.append(first.size), tcls.append(kc)
    toff = np.concatenate([[0], np.cumsum(counts)]).astype(np.int64)
    value = rng.uniform(-3.0, 40.0, index.size).astype(np.float32)
    if index.size > 5:
        value[[1, 3]] = [np.inf, 2.0 ** 15]
    return off, index, np.concatenate(ids).astype(np.int64), toff, value, np.concatenate(tcls)


@pytest.mark.parametrize("gap", [1, 2, 3])
@pytest.mark.parametrize("spatial,sizes", [((15, 16, 17), (400, 0, 350, 60, 500)), ((57, 61), (500, 0, 300, 40, 600))], ids=["3d", "2d"])
def test_statement_equals_brute_force(spatial, sizes, gap):
    rng = np.random.default_rng(gap * 10 + len(spatial))
    off, index, ids, toff, value, cls = _random_case(rng, spatial, sizes, 3)
    assert off[-1] <= 1500 and toff[4] == toff[3] and toff[-1] > 50
    for val, kc in ((value, cls), (None, None)):
        want = cluster_graph_numpy(off, index, ids, toff, spatial, ClusterGraphSpec(gap), val, kc)
        ref = _brute(off, index, ids, toff, spatial, gap, val, kc)
        assert sorted(want) == sorted(ref)
        for name in want:
            assert want[name].dtype == ref[name].dtype and np.array_equal(want[name], ref[name]), name
    assert want["edges"].shape[0] > 20 and (gap > 1 or (want["rows"][:, 0] == 0).any()) and want["events"][1].tolist() == [0, 0, 0, 0]
    assert want["events"][3].tolist() == [0, 0, 0, 0] and (want["group"][off[3]:off[4]] == -1).all()
    assert (want["groups"][:, 0] > 2).any() and want["edges"][:, 3].max() <= 3 * gap * gap


def test_statement_raises_on_what_the_device_reports():
    off, toff = [0, 4], [0, 2]
    ok = cluster_graph_numpy(off, [0, 1, 7, 30], [0, 1, 1, -1], toff, (6, 6))
    assert ok["edges"].tolist() == [[1, 2, 2, 1, 0, 1]] and ok["group"].tolist() == [0, 0, 0, -1]
    for index, ids, t, cls in (([0, 1, 7, 30], [0, 2, 1, -1], toff, None), ([0, 1, 7, 30], [0, -2, 1, -1], toff, None),
                               ([0, 1, 7, 30], [0, 0, 0, -1], toff, None), ([0, 1, 7, 36], [0, 1, 1, 1], toff, None),
                               ([0, 1, 7, 30], [0, 1, 1, -1], toff, [1, 32]), ([0, 1, 7, 30], [0, 1, 1, -1], [0, 3], None)):
        with pytest.raises(ValueError):
            cluster_graph_numpy(off, index, ids, t, (6, 6), cls=cls)
    with pytest.raises(ValueError):
        cluster_graph_numpy(off, [0, 1, 7, 30], [0, 1, 1, -1], toff, (6, 6, 6, 6))
