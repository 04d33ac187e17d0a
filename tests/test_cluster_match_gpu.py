"""Cluster matching on the device (csrc/cluster_match.hip) against the numpy statement (uresnet_amd.clusters.cluster_match_numpy).
Every comparison is np.array_equal on every table, fp64 columns by their bits.  Op level: the lists and every output sit between 0xFF
guard bands (tests/_guard.py); each case runs four times -- scratch filled 0xFF, filled 0x00, as the second call left it (the same
arguments again), and with one table insertion per entry instead of one per distinct pair of a workgroup (URSN_CLMATCH_WAVE=0) --
and all four must give the statement's bits with status 0.  Net level: set_cluster_matching with the voxel-score calls,
match_clusters, and the driver's ANA_MATCH file."""
import ctypes
import io
import os
from contextlib import redirect_stdout

import numpy as np
import pytest

from _guard import Guarded
from uresnet_amd import _lib, uresnet
from uresnet_amd import synthetic_io as sio
from uresnet_amd.clusters import (MATCH_EVENT_INT, MATCH_EVENT_REAL, MATCH_ROW_INT, MATCH_ROW_REAL, ClusterSpec, cluster_match_numpy,
                                  cluster_numpy)
from uresnet_amd.ssnet import VoxelBatch, match_csv_header

pytestmark = pytest.mark.gpu

I, R, EI, ER = _lib.CLMATCH_I, _lib.CLMATCH_R, _lib.CLMATCH_EI, _lib.CLMATCH_ER
ROUTES = ((0xFF, True), (0x00, True), (None, True), (0xFF, False))


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view({4: np.uint32, 8: np.uint64}[a.dtype.itemsize])


def _untouched(a):
    return bool((np.ascontiguousarray(a).view(np.uint8) == 0xFF).all())


def _run(lib, off, a, toff_a, b, toff_b, value, cap_a, cap_b, pair_cap, rows_a, rows_b, cells, pairs=True, routes=ROUTES):
    """Four calls of ursn_cluster_match on guarded operands.  The tables hold rows_a / rows_b / cells entries whatever the caps are,
    so what lies at or beyond a cap can be seen to be untouched.  Returns per call a dict of host arrays."""
    import torch
    n, M = off.size - 1, int(off[-1])
    g_off, g_ta, g_tb = Guarded(n + 1, torch.int64, off), Guarded(n + 1, torch.int64, toff_a), Guarded(n + 1, torch.int64, toff_b)
    g_a, g_b = Guarded(max(M, 1), torch.int32), Guarded(max(M, 1), torch.int32)
    g_val = None if value is None else Guarded(max(M, 1), torch.float32)
    if M:
        g_a.set(a.astype(np.int32)), g_b.set(b.astype(np.int32))
        if g_val is not None:
            g_val.set(value)
    need = int(lib.ursn_cluster_match_scratch_bytes(n, M, cap_a, cap_b, pair_cap))
    assert need >= 8 and need % 8 == 0
    scratch = Guarded(need, torch.uint8)
    d = _lib.ursn_cluster_match_desc()
    d.n, d.m_total, d.offsets = n, M, g_off.ptr
    d.cluster_a, d.table_offsets_a, d.cluster_b, d.table_offsets_b = g_a.ptr, g_ta.ptr, g_b.ptr, g_tb.ptr
    d.value = None if g_val is None else g_val.ptr
    inputs = [("offsets", g_off), ("table_offsets_a", g_ta), ("table_offsets_b", g_tb), ("cluster_a", g_a), ("cluster_b", g_b),
              ("scratch", scratch)] + ([] if g_val is None else [("value", g_val)])
    results = []
    for fill, wave in routes:
        if fill is not None:
            scratch.fill(fill)
        out = {"a_int": Guarded((max(rows_a, 1), I), torch.int64), "a_real": Guarded((max(rows_a, 1), R), torch.float64),
               "b_int": Guarded((max(rows_b, 1), I), torch.int64), "b_real": Guarded((max(rows_b, 1), R), torch.float64),
               "event_int": Guarded((n, EI), torch.int64), "event_real": Guarded((n, ER), torch.float64),
               "status": Guarded(1, torch.int32)}
        if pairs:
            out.update({"pair_offsets": Guarded(max(rows_a, cap_a) + 1, torch.int64), "pair_b": Guarded(max(cells, 1), torch.int32),
                        "pair_n": Guarded(max(cells, 1), torch.int64), "pair_q": Guarded(max(cells, 1), torch.int64)})
        o = _lib.ursn_cluster_match_out()
        for name, g in out.items():
            setattr(o, name, g.ptr)
        o.cap_a, o.cap_b, o.pair_cap = cap_a, cap_b, pair_cap
        if not wave:
            os.environ["URSN_CLMATCH_WAVE"] = "0"
        try:
            _lib.check(lib.ursn_cluster_match(ctypes.byref(d), ctypes.byref(o), ctypes.c_void_p(scratch.ptr), need, None))
        finally:
            os.environ.pop("URSN_CLMATCH_WAVE", None)
        torch.cuda.synchronize()
        for name, g in inputs + list(out.items()):
            g.check(name)
        results.append({name: g.numpy() for name, g in out.items()})
    return results


def _check(lib, off, a, toff_a, b, toff_b, value, cap_a=None, cap_b=None, pair_cap=None, pairs=True):
    """Runs the case and compares all four calls with the statement; returns the statement."""
    off, toff_a, toff_b = (np.asarray(x, np.int64) for x in (off, toff_a, toff_b))
    a, b = np.asarray(a, np.int64), np.asarray(b, np.int64)
    value = None if value is None else np.asarray(value, np.float32)
    want = cluster_match_numpy(off, a, toff_a, b, toff_b, value)
    KA, KB, cells = int(toff_a[-1]), int(toff_b[-1]), int(want["pair_offsets"][-1])
    cap_a, cap_b, pair_cap = (KA if cap_a is None else cap_a), (KB if cap_b is None else cap_b), (cells if pair_cap is None else pair_cap)
    ra, rb, rc = min(cap_a, KA), min(cap_b, KB), min(pair_cap, cells)
    for k, got in enumerate(_run(lib, off, a, toff_a, b, toff_b, value, cap_a, cap_b, pair_cap, KA, KB, cells, pairs)):
        what = "call %d" % k
        assert int(got["status"][0]) == 0, what
        for side, rows in (("a", ra), ("b", rb)):
            assert np.array_equal(got[side + "_int"][:rows], want[side + "_int"][:rows]), (what, side, "int")
            assert np.array_equal(_bits(got[side + "_real"][:rows]), _bits(want[side + "_real"][:rows])), (what, side, "real")
            assert _untouched(got[side + "_int"][rows:]) and _untouched(got[side + "_real"][rows:]), \
                (what, side, "rows at or beyond the count or cap were written")
        assert np.array_equal(got["event_int"], want["event_int"]), what
        assert np.array_equal(_bits(got["event_real"]), _bits(want["event_real"])), what
        if pairs:
            assert np.array_equal(got["pair_offsets"][:ra + 1], want["pair_offsets"][:ra + 1]), what     # the TRUE counts
            assert _untouched(got["pair_offsets"][ra + 1:]), what
            for name in ("pair_b", "pair_n", "pair_q"):
                assert np.array_equal(got[name][:rc], want[name][:rc]), (what, name)
                assert _untouched(got[name][rc:]), (what, name, "cells at or beyond the count or cap were written")
    return want


def _relabel(off, raw):
    """Arbitrary labels (-1 = none) -> event-local ids 0..K_e-1 in order of value, and the table offsets: every row has a member."""
    raw = np.asarray(raw, np.int64)
    ids, counts = np.full(raw.size, -1, np.int64), []
    for e in range(len(off) - 1):
        part = raw[off[e]:off[e + 1]]
        uniq, inv = np.unique(part[part >= 0], return_inverse=True)
        ids[off[e]:off[e + 1]][part >= 0] = inv
        counts.append(uniq.size)
    return ids, np.concatenate([[0], np.cumsum(counts)]).astype(np.int64)


def _clustered(off, index, cls, shape, spec):
    ids, counts = [], []
    for e in range(len(off) - 1):
        c, first, _, _ = cluster_numpy(index[off[e]:off[e + 1]], cls[off[e]:off[e + 1]], shape, spec)
        ids.append(c), counts.append(first.size)
    return np.concatenate(ids).astype(np.int64), np.concatenate([[0], np.cumsum(counts)]).astype(np.int64)


def _values(rng, m):
    return rng.uniform(-3.0, 40.0, m).astype(np.float32)


@pytest.mark.parametrize("shape,events,occupancy", [((12, 10, 14), 3, 0.9), ((20, 24), 8, 0.85)], ids=["3d", "2d"])
def test_clustered_random_classes(lib, shape, events, occupancy):
    """Long runs: at this occupancy nearly every entry lies in one giant cluster per event on side A (any class joins any) against
    the per-class clusters of side B.  One event is empty; about 3000 entries, no multiple of 64."""
    rng = np.random.default_rng(len(shape))
    lists = [np.flatnonzero(rng.uniform(size=int(np.prod(shape))) < occupancy) if e != 1 else np.zeros(0, np.int64)
             for e in range(events)]
    off = np.concatenate([[0], np.cumsum([x.size for x in lists])])
    index = np.concatenate(lists)
    cls = rng.integers(0, 3, index.size).astype(np.uint8)
    M = int(off[-1])
    assert 2500 < M < 3500 and M % 64 != 0
    a, ta = _clustered(off, index, cls, shape, ClusterSpec(None, None, False, 1))
    b, tb = _clustered(off, index, cls, shape, ClusterSpec(6 if len(shape) == 3 else 4, (1, 2), True, 2))
    want = _check(lib, off, a, ta, b, tb, _values(rng, M))
    assert want["a_int"][:, 0].max() > 200 and tb[-1] > 3 * ta[-1] and (want["a_int"][:, 3] > 10).any()


@pytest.mark.parametrize("ka,kb", [(2, 3), (3, 2), (3, 3)])
def test_alternating_giant_rows(lib, ka, kb):
    """Ids that change from lane to lane: every wave run has length 1 and the workgroup's LDS table does all the combining."""
    M = 3001
    j = np.arange(M)
    off = [0, 1700, M]
    a, ta = _relabel(off, j % ka)
    b, tb = _relabel(off, (j // 2) % kb if ka == kb else j % kb)
    want = _check(lib, off, a, ta, b, tb, _values(np.random.default_rng(ka * 8 + kb), M))
    assert list(ta) == [0, ka, 2 * ka] and want["pair_offsets"][-1] >= 2 * max(ka, kb) and want["a_int"][:, 0].min() > 400


@pytest.mark.parametrize("giant", ["a", "b"])
def test_one_giant_row_against_fragments(lib, giant):
    """701 cells in one row: the rank by B id walks a long segment, and every workgroup holds 256 distinct pairs, as many as its LDS
    table has slots.  Fragments of one entry and of four."""
    M = 2803
    j = np.arange(M)
    for frag in (j % 701, j // 4):
        one, many = _relabel([0, M], np.zeros(M, np.int64)), _relabel([0, M], frag)
        (a, ta), (b, tb) = (one, many) if giant == "a" else (many, one)
        want = _check(lib, [0, M], a, ta, b, tb, _values(np.random.default_rng(5), M))
        assert want["pair_offsets"][-1] == 701 and want["event_int"][0][4] == 701
        assert want["a_int"][0][3] == (701 if giant == "a" else 1)


def test_every_entry_its_own_rows(lib):
    """8189 cells in 16384 slots: the global table at its highest load (a half) and its longest probe walks."""
    M = 8189
    off = [0, 5003, M]
    j = np.arange(M)
    a, ta = _relabel(off, j)
    b, tb = _relabel(off, (j * 7) % M)                       # a permutation: the B rows in another order than the list
    want = _check(lib, off, a, ta, b, tb, _values(np.random.default_rng(6), M))
    assert ta[-1] == tb[-1] == M == want["event_int"][:, 7].sum() and list(want["event_real"][:, 3]) == [1.0, 1.0]


def test_missing_ids_on_either_side(lib):
    """-1 mixed in on both sides, rows with matched = 0 on both sides, entries in no row at all."""
    rng = np.random.default_rng(7)
    M = 2999
    off = [0, 1000, 1000, 2100, M]
    ra, rb = rng.integers(-1, 40, M), rng.integers(-1, 25, M)
    ra[rng.uniform(size=M) < 0.3] = -1
    rb[rng.uniform(size=M) < 0.3] = -1
    rb[(ra == 5) | (ra == 17)] = -1                          # A rows none of whose members has a B row
    ra[(rb == 3) | (rb == 11)] = -1                          # ... and the reverse
    a, ta = _relabel(off, ra)
    b, tb = _relabel(off, rb)
    want = _check(lib, off, a, ta, b, tb, _values(rng, M))
    assert ((a < 0) & (b < 0)).sum() > 100 and (want["a_int"][:, 2] == 0).sum() >= 3 and (want["b_int"][:, 2] == 0).sum() >= 3
    assert (want["a_int"][want["a_int"][:, 2] == 0][:, 4] == -1).all()


def test_equal_counts_fall_to_the_lowest_id(lib):
    """Three A rows of 6 against three B rows of 6, every cell of count 2: best = 0 for all six rows; then a list in which the ties
    sit at the HIGH ids of a row with more partners."""
    a = np.repeat([0, 1, 2], 6)
    b = np.tile(np.repeat([0, 1, 2], 2), 3)
    order = np.random.default_rng(8).permutation(18)         # arrival order must not matter
    want = _check(lib, [0, 18], a[order], [0, 3], b[order], [0, 3], None)
    assert (want["a_int"][:, 4] == 0).all() and (want["b_int"][:, 4] == 0).all() and (want["a_int"][:, 5] == 2).all()
    assert list(want["a_int"][:, 7]) == [2, 0, 0] and list(want["b_int"][:, 7]) == [2, 0, 0]
    a2 = np.array([0] * 7 + [1] * 3)
    b2 = np.array([3, 1, 1, 1, 2, 2, 2, 0, 3, 3])
    want = _check(lib, [0, 10], a2, [0, 2], b2, [0, 4], None)
    assert list(want["a_int"][:, 4]) == [1, 3] and list(want["b_int"][:, 4]) == [1, 0, 0, 1]


def test_values_out_of_range_and_no_values(lib):
    off = [0, 8, 8, 11, 13]
    a = np.array([0, 0, 1, 1, 2, -1, 3, 3, 0, 0, 1, -1, -1])
    b = np.array([1, 0, 0, 1, -1, 2, 1, 0, -1, -1, -1, 0, 0])
    value = np.array([1.5, 2.0 ** 15, np.nan, -2.25, np.inf, 0.5, 0.25, -(2.0 ** 15), 2.0 ** -17, 1.0, 2.0, -np.inf, 4.0], np.float32)
    want = _check(lib, off, a, [0, 4, 4, 6, 6], b, [0, 3, 3, 3, 4], value)
    assert list(want["a_int"][:, 7]) == [3, 1, 1, 1, 0, 0] and list(want["b_int"][:, 7]) == [3, 0, 0, 1]
    none = _check(lib, off, a, [0, 4, 4, 6, 6], b, [0, 3, 3, 3, 4], None)
    assert (none["a_int"][:, 1] == 0).all() and (none["pair_q"] == 0).all() and (none["a_int"][:, 7] & 1 == 0).all()
    big = np.full(13, np.float32(32767.998))                 # the largest charges the fixed point takes
    _check(lib, off, a, [0, 4, 4, 6, 6], b, [0, 3, 3, 3, 4], big)


def test_no_entries_and_no_rows(lib):
    z = np.zeros(0, np.int64)
    want = _check(lib, [0, 0, 0], z, [0, 0, 0], z, [0, 0, 0], z.astype(np.float32))
    assert [list(r) for r in want["event_real"]] == [[1.0, 0.0, 0.0, 0.0]] * 2
    _check(lib, [0, 0], z, [0, 0], z, [0, 0], None, cap_a=5, cap_b=3, pair_cap=4)
    _check(lib, [0, 0], z, [0, 0], z, [0, 0], None, pairs=False)
    # entries, none in a row; then rows on one side only, in one event of two
    _check(lib, [0, 4, 6], np.full(6, -1), [0, 0, 0], np.full(6, -1), [0, 0, 0], np.ones(6, np.float32), cap_a=6, cap_b=6, pair_cap=6)
    want = _check(lib, [0, 4, 9], [0, 0, 1, -1, 0, 1, 1, 0, -1], [0, 2, 4], [-1, -1, -1, -1, 0, 0, 1, 1, 1], [0, 0, 2],
                  np.arange(9, dtype=np.float32))
    assert list(want["event_int"][0]) == [0, 0, 0, 0, 0, 2, 0, 0, 0, 3, 0, 0] and want["event_int"][1][4] == 4
    _check(lib, [0, 4, 9], [-1, -1, -1, -1, 0, 0, 1, 1, 1], [0, 0, 2], [0, 0, 1, -1, 0, 1, 1, 0, -1], [0, 2, 4], None, pairs=False)


def test_short_caps_bound_what_is_written(lib):
    """cap_a, cap_b and pair_cap each one short of the need, then far short: what lies at or beyond a cap is untouched, every row and
    cell below it is complete, and pair_offsets holds the true counts."""
    rng = np.random.default_rng(9)
    M = 1501
    off = [0, 700, M]
    a, ta = _relabel(off, rng.integers(-1, 30, M))
    b, tb = _relabel(off, rng.integers(-1, 20, M))
    value = _values(rng, M)
    KA, KB = int(ta[-1]), int(tb[-1])
    cells = int(cluster_match_numpy(off, a, ta, b, tb)["pair_offsets"][-1])
    assert KA == 60 and KB == 40 and cells > 500
    for caps in ((KA - 1, None, None), (None, KB - 1, None), (None, None, cells - 1), (KA - 1, KB - 1, cells - 1), (7, 3, 11),
                 (0, 0, 0), (KA + 5, KB + 5, cells + 5)):
        _check(lib, off, a, ta, b, tb, value, *caps)


def test_an_id_outside_its_events_rows_sets_status(lib):
    """The argument check's positive control: an id equal to K_e is never used as an index; the entry is skipped, *status is non-zero
    and no border is touched (checked inside _run)."""
    off, ta, tb = np.array([0, 5, 9]), np.array([0, 2, 4]), np.array([0, 2, 3])
    a = np.array([0, 0, 1, 2, 1, 0, 1, 1, 0])                # a[3] == K_0
    b = np.array([0, 1, 1, 0, 0, 0, 0, 0, 0])
    for got in _run(lib, off, a, ta, b, tb, np.ones(9, np.float32), 4, 3, 9, 4, 3, 9):
        assert int(got["status"][0]) != 0
        assert list(got["a_int"][:, 0]) == [2, 2, 2, 2] and list(got["b_int"][:, 0]) == [2, 2, 4]      # the entry took no part
    bad_b = np.array([0, 1, 1, 0, 0, 0, 0, 1, -2])           # K_1 of side B, and an id below -1
    for got in _run(lib, off, np.minimum(a, 1), ta, bad_b, tb, None, 4, 3, 9, 4, 3, 9):
        assert int(got["status"][0]) != 0


# ---- net level -----------------------------------------------------------------------------------------------------------------
DIMS = (16, 16, 16, 1)
_cache = {}


def _net(prec):
    """16^3, two strides, 4 base filters; the bf16 plan refuses a base that is no multiple of 8, so it runs at 8, its smallest."""
    net = uresnet(dims=list(DIMS), num_class=3, base_num_outputs=4 if prec == "fp32" else 8, num_strides=2)
    net.construct(trainable=False, use_weight=False, seed=7, precision=prec)
    return net


def _events(shape=DIMS[:-1], n=2):
    if shape not in _cache:
        _cache[shape] = VoxelBatch.concat([sio.dense_to_voxels(*sio.lartpc_sparse(list(shape) + [1], 3, e)) for e in range(n)]).validate()
    return _cache[shape]


def _toff(tables):
    return np.concatenate([[0], np.cumsum([t["first"].size for t in tables])]).astype(np.int64)


def _same_match(match, want, ta, tb):
    """A match as the Python surface returns it equals the statement's tables, column by column and bit by bit."""
    assert sorted(match) == ["a", "b", "events"]
    for side, toff in (("a", ta), ("b", tb)):
        assert len(match[side]) == len(toff) - 1
        for e, got in enumerate(match[side]):
            assert sorted(got) == sorted(MATCH_ROW_INT + MATCH_ROW_REAL)
            for c, name in enumerate(MATCH_ROW_INT):
                assert got[name].dtype == np.int64 and np.array_equal(got[name], want[side + "_int"][toff[e]:toff[e + 1], c]), (side, e, name)
            for c, name in enumerate(MATCH_ROW_REAL):
                assert np.array_equal(_bits(got[name]), _bits(want[side + "_real"][toff[e]:toff[e + 1], c])), (side, e, name)
    assert sorted(match["events"]) == sorted(MATCH_EVENT_INT + MATCH_EVENT_REAL)
    for c, name in enumerate(MATCH_EVENT_INT):
        assert np.array_equal(match["events"][name], want["event_int"][:, c]), name
    for c, name in enumerate(MATCH_EVENT_REAL):
        assert np.array_equal(_bits(match["events"][name]), _bits(want["event_real"][:, c])), name


def _result_matches(net, r, vb, shape):
    """r['match'] equals the statement on the returned ids, and match_clusters on the returned ids (with the cell list)."""
    pred, true = {"cluster": r["cluster"], "clusters": r["clusters"]}, {"cluster": r["true_cluster"], "clusters": r["true_clusters"]}
    ta, tb = _toff(r["clusters"]), _toff(r["true_clusters"])
    assert ta[-1] > 0 and tb[-1] > 0
    want = cluster_match_numpy(vb.offsets, np.concatenate(r["cluster"]), ta, np.concatenate(r["true_cluster"]), tb, vb.value)
    _same_match(r["match"], want, ta, tb)
    again = net.match_clusters(None, vb, pred, true, pairs=True)
    cells = again.pop("pairs")
    _same_match(again, want, ta, tb)
    for e, (pa, pb, pn, pq) in enumerate(cells):
        lo, hi = want["pair_offsets"][ta[e]], want["pair_offsets"][ta[e + 1]]
        rows = np.repeat(np.arange(ta[e + 1] - ta[e]), np.diff(want["pair_offsets"][ta[e]:ta[e + 1] + 1]))
        assert np.array_equal(pa, rows) and np.array_equal(pb, want["pair_b"][lo:hi])
        assert np.array_equal(pn, want["pair_n"][lo:hi]) and np.array_equal(pq, want["pair_q"][lo:hi])
    # the true clusters are those of the labels under the same spec
    spec = net._cluster_spec
    for e in range(vb.n):
        lab = vb.label[vb.offsets[e]:vb.offsets[e + 1]].astype(np.uint8)
        ids, first, _, _ = cluster_numpy(r["index"][e], lab, shape, spec)
        assert np.array_equal(r["true_cluster"][e], ids) and np.array_equal(r["true_clusters"][e]["first"], first)


@pytest.mark.parametrize("prec", ["fp32", "bf16"])
def test_inference_voxel_scores_with_match(prec):
    net, vb = _net(prec), _events()
    net.set_clustering(ClusterSpec(classes=(0, 1, 2), min_size=2))
    before = net.inference_voxel_scores(None, vb, want=("pred", "cluster"))          # the setter never called: today's keys
    assert sorted(before) == ["acc_all", "acc_nonzero", "cluster", "clusters", "index", "pred"]
    net.set_cluster_matching(True)
    r = net.inference_voxel_scores(None, vb, want=("pred", "cluster"))
    assert sorted(r) == sorted(list(before) + ["match", "true_cluster", "true_clusters"])
    _result_matches(net, r, vb, DIMS[:-1])
    assert sorted(net.inference_voxel_scores(None, vb, want=("pred",))) == ["acc_all", "acc_nonzero", "index", "pred"]
    net.set_cluster_matching(False)
    off_r = net.inference_voxel_scores(None, vb, want=("pred", "cluster"))
    assert sorted(off_r) == sorted(before)
    for key in before:                                                                # ... and today's bytes
        x, y = before[key], off_r[key]
        if key == "clusters":
            assert all(np.array_equal(p[k], q[k]) and p[k].dtype == q[k].dtype for p, q in zip(x, y) for k in p)
        elif isinstance(x, list):
            assert all(np.array_equal(p, q) and p.dtype == q.dtype for p, q in zip(x, y)), key
        else:
            assert x == y, key
        if key in ("cluster", "pred"):
            assert all(np.array_equal(p, q) for p, q in zip(x, r[key])), key


@pytest.mark.parametrize("prec", ["fp32", "bf16"])
def test_tiled_match_is_in_the_large_shape(prec):
    big = (32, 32, 32)
    vb = _events(big)
    net = _net(prec)
    net.set_clustering(ClusterSpec(classes=(0, 1, 2), same_class=False))
    net.set_cluster_matching(True)
    r = net.inference_tiled_voxel_scores(None, vb, big, want=("pred", "cluster"))
    assert "match" in r and r["tiles_run"] > 1
    _result_matches(net, r, vb, big)
    net.set_cluster_matching(False)
    assert "match" not in net.inference_tiled_voxel_scores(None, vb, big, want=("pred", "cluster"))


# ---- driver --------------------------------------------------------------------------------------------------------------------
def _drive(tmp_path, tag, extra):
    from uresnet_amd.ssnet_trainval import ssnet_trainval
    inp = tmp_path / "input.cfg"
    inp.write_text("Dims [32, 32, 32, 1]\nNumClass 3\nGenerator 'lartpc_sparse'\nNumEntries 64\n"      # the driver's net has 5 strides
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
        res = t.ana_step()
        t.reset()
    with open(str(out), "rb") as f:
        return f.read(), res


def test_driver_writes_one_row_per_event(tmp_path):
    """The CSV parses back to the returned match; the driver's own records are byte for byte those of a run without the key."""
    csv = tmp_path / "match.csv"
    plain, ref = _drive(tmp_path, "plain", "")
    with_key, res = _drive(tmp_path, "match", "ANA_MATCH '%s'\n" % csv)
    assert with_key == plain and "match" not in ref and sorted(res) == sorted(list(ref) + ["match"])
    lines = csv.read_text().split("\n")
    assert lines[0] + "\n" == match_csv_header() and lines[-1] == "" and len(lines) == 2 + len(res["entries"]) == 4
    names = lines[0].split(",")
    events = res["match"]["events"]
    for e, line in enumerate(lines[1:-1]):
        row = dict(zip(names, line.split(",")))
        assert len(row) == 17 and int(row["entry"]) == int(res["entries"][e])
        for name in MATCH_EVENT_INT:
            assert int(row[name]) == int(events[name][e]), (e, name)
        for name in MATCH_EVENT_REAL:
            assert np.float64(row[name]).view(np.uint64) == events[name][e].view(np.uint64), (e, name)
    for ev, ev0 in zip(res["voxels"], ref["voxels"]):
        assert sorted(ev) == sorted(list(ev0) + ["true_cluster", "true_clusters"])
    assert events["rows_a"].sum() > 0 and events["rows_b"].sum() > 0
