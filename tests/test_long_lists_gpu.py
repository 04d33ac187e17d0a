"""The voxel-list kernels past every one-step threshold: lists of more than 2^21 entries, more than 2^22 rows, more
than 1024 boxes, thousands of events.  Op level, on the runners of the per-kernel test files: operands and outputs between guard
bands at exact scratch sizes, status 0, every comparison np.array_equal (fp64 by bits).  Each case runs twice: scratch filled 0xFF
and 0x00, and where a kernel file has a URSN_CL*_WAVE switch, one call on each route.  The expected tables come from
tests/_long_lists.py -- the statement on a base batch, tiled; or the run lattice's closed form -- or, where the list is short (the
checkerboards, the small events, the crop), from the statement itself.  tests/test_long_lists_host.py proves the constructions and
that every case here crosses the threshold it is named for; each test asserts that what it built has the numbers of that table."""
import functools

import numpy as np
import pytest

import _long_lists as L
import test_cluster_features_gpu as TF
import test_cluster_graph_gpu as TG
import test_cluster_match_gpu as TM
import test_clusters_gpu as TC
import test_tiling_gpu as TT
import test_voxel_io_gpu as TV
from uresnet_amd import tiling
from uresnet_amd.clusters import ClusterSpec

pytestmark = pytest.mark.gpu

FILLS = (0xFF, 0x00)
ROUTES = ((0xFF, True), (0x00, False))           # two scratch fills; the wave-combining route and the one-atomic-per-entry route


def _case(name, n, m_total, rows=None, boxes=None, edge_cap=None):
    c = L.BY_NAME[name]
    assert (c.n, c.m_total) == (n, m_total), (name, n, m_total)
    for have, listed in ((rows, c.rows), (boxes, c.boxes), (edge_cap, c.edge_cap)):
        assert have is None or have == listed, (name, have, listed)


def _release():
    import torch
    torch.cuda.empty_cache()


# ---- comparisons, as the _check functions of the per-kernel files make them --------------------------------------------------------
def _cluster(lib, b, spec, want, what):
    M, total = int(b.off[-1]), int(want["table_offsets"][-1])
    for k, got in enumerate(TC._run(lib, b.off, b.index, b.cls, b.shape, spec, fills=FILLS)):
        assert int(got["status"][0]) == 0, (what, k)
        assert np.array_equal(got["cluster"][:M], want["cluster"]), (what, k)
        assert np.array_equal(got["count"], want["count"]) and np.array_equal(got["table_offsets"], want["table_offsets"]), (what, k)
        for name in ("first", "size", "cls"):
            assert np.array_equal(got[name][:total], want[name]), (what, k, name)
            assert TM._untouched(got[name][total:]), (what, k, name, "rows at or beyond the count were written")
    _release()


def _features(lib, b, cl, want, what):
    wi, wr = TF._tables(want)
    wr = TF._bits(wr)
    total = int(cl["table_offsets"][-1])
    assert wi.shape[0] == total
    for k, (it, rt, status) in enumerate(TF._run(lib, b.off, b.index, b.value, cl["cluster"], cl["table_offsets"], b.shape, total,
                                                 routes=ROUTES)):
        assert status == 0, (what, k)
        for name, at, w in TF.INT_FIELDS:
            assert np.array_equal(it[:, at:at + w], wi[:, at:at + w]), (what, k, name)
        for name, at, w in TF.REAL_FIELDS:
            assert np.array_equal(rt[:, at:at + w], wr[:, at:at + w]), (what, k, name)
    _release()


def _match(lib, b, cl_a, cl_b, want, what):
    ta, tb = cl_a["table_offsets"], cl_b["table_offsets"]
    KA, KB, cells = int(ta[-1]), int(tb[-1]), int(want["pair_offsets"][-1])
    for k, got in enumerate(TM._run(lib, b.off, cl_a["cluster"], ta, cl_b["cluster"], tb, b.value, KA, KB, cells, KA, KB, cells,
                                    routes=ROUTES)):
        assert int(got["status"][0]) == 0, (what, k)
        for name in ("a_int", "b_int", "event_int", "pair_offsets", "pair_b", "pair_n", "pair_q"):
            assert np.array_equal(got[name][:want[name].shape[0]], want[name]), (what, k, name)
        for name in ("a_real", "b_real", "event_real"):
            assert np.array_equal(TM._bits(got[name][:want[name].shape[0]]), TM._bits(want[name])), (what, k, name)
    _release()


def _graph(lib, b, cl, want, what, gap=1, edge_cap=None):
    toff = cl["table_offsets"]
    K, NG, NE = int(toff[-1]), int(want["group_offsets"][-1]), int(want["edge_offsets"][-1])
    edge_cap = NE if edge_cap is None else edge_cap
    for k, got in enumerate(TG._run(lib, b.off, b.index, cl["cluster"], toff, b.shape, gap, b.value, cl["cls"], K, NG, NE, edge_cap,
                                    K, NG, NE, routes=ROUTES)):
        assert int(got["status"][0]) == 0, (what, k, int(got["status"][0]))
        for name, rows in (("rows", K), ("groups", NG), ("edges", NE)):
            assert np.array_equal(got[name][:rows], want[name]), (what, k, name)
        assert np.array_equal(got["group_offsets"], want["group_offsets"]) and np.array_equal(got["event"], want["events"]), (what, k)
        assert np.array_equal(got["edge_offsets"][:K + 1], want["edge_offsets"]), (what, k)
        assert np.array_equal(got["group"][:b.off[-1]], want["group"]) and got["group"].dtype == np.int32, (what, k)
    _release()


# ---- labels_to_voxels: one event longer than 2^21 voxels ----------------------------------------------------------------------------
@pytest.mark.parametrize("name,shape", [("labels_3d", L.LABELS_3D), ("labels_2d", L.LABELS_2D)], ids=["labels_3d", "labels_2d"])
def test_labels_to_voxels_with_two_spans_per_scan_thread(lib, name, shape):
    V = int(np.prod(shape))
    _case(name, 2, V)
    rng = np.random.default_rng(len(shape))
    labels = np.zeros((2, V), np.float32)
    for e, density in enumerate((0.03, 0.004)):                     # ~3 % non-zeros in three classes; the second event sparser
        at = np.flatnonzero(rng.uniform(size=V) < density)
        labels[e, at] = rng.integers(1, 4, at.size)
    S = L.VOX_SPAN
    for e, (empty, full) in enumerate((((3, 4, 511, 1024), (7, 512, 1023)), ((0, 1025), (1024,)))):
        for s in empty:                                             # whole spans empty and whole spans full, at the seams of the
            labels[e, s * S:(s + 1) * S] = 0                        # scan's chunks (spans 2 t, 2 t + 1 belong to thread t)
        for s in full:
            labels[e, s * S:(s + 1) * S] = 1 + s % 3
    labels[0, -1] = 2.0                                             # the ragged last span's last voxel
    nz = [np.flatnonzero(labels[e]) for e in range(2)]
    want_off = np.concatenate([[0], np.cumsum([a.size for a in nz])]).astype(np.int64)
    want_idx = np.concatenate(nz).astype(np.int32)
    want_cls = np.concatenate([labels[e][nz[e]].astype(np.uint8) for e in range(2)])
    total = int(want_off[-1])
    assert nz[1].size < nz[0].size / 2 and total > 60000
    for fill in ("nan", "zero"):
        off, idx, cls = TV._compact(lib, labels, total, fill)
        assert np.array_equal(off, want_off) and np.array_equal(idx, want_idx) and np.array_equal(cls, want_cls), fill
    off, idx, cls = TV._compact(lib, labels, total - 1, "nan")     # one entry too few: true counts, nothing behind the cap
    assert np.array_equal(off, want_off) and np.array_equal(idx, want_idx[:-1]) and np.array_equal(cls, want_cls[:-1])
    _release()


def test_labels_to_voxels_over_hundreds_of_events_with_runs_of_empty_ones(lib):
    """The event loop of voxel_scan: 700 events of two spans each, the first, the last and two runs of 100+ events all zero."""
    c = L.BY_NAME["labels_many_events"]
    n, V = c.n, c.m_total
    rng = np.random.default_rng(70)
    labels = (rng.integers(1, 4, (n, V)) * (rng.uniform(size=(n, V)) < 0.05)).astype(np.float32)
    for a, b in ((0, 1), (30, 140), (400, 530), (n - 1, n)):
        labels[a:b] = 0
    labels[200] = 2.0                                               # a full event between sparse ones
    nz = [np.flatnonzero(labels[e]) for e in range(n)]
    want_off = np.concatenate([[0], np.cumsum([a.size for a in nz])]).astype(np.int64)
    want_idx = np.concatenate(nz).astype(np.int32)
    want_cls = np.concatenate([labels[e][nz[e]].astype(np.uint8) for e in range(n)])
    assert (np.diff(want_off) == 0).sum() >= 242 and want_off[-1] > 40000
    for fill in ("nan", "zero"):
        off, idx, cls = TV._compact(lib, labels, int(want_off[-1]), fill)
        assert np.array_equal(off, want_off) and np.array_equal(idx, want_idx) and np.array_equal(cls, want_cls), fill
    _release()


# ---- list (a): a random batch of three events, replicated past 2^21 entries -----------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _random():
    base = L.random_base()
    ca, cb = L.cluster_statement(base, L.SPEC_ANY_CLASS), L.cluster_statement(base, L.SPEC_PER_CLASS)
    R, M = L.R_RANDOM, int(base.off[-1])
    b = L.repeat(base, R)
    _case("random_replicated", b.off.size - 1, int(b.off[-1]), R * int(cb["table_offsets"][-1]))
    return base, b, ca, cb, L.tile_cluster(ca, R), L.tile_cluster(cb, R), R, M


def test_cluster_voxels_on_replicated_events_past_two_spans_per_scan_thread(lib):
    _, b, _, _, _, want, _, _ = _random()
    assert (want["cluster"] == -1).any() and (np.diff(b.off) == 0).sum() == L.R_RANDOM
    _cluster(lib, b, L.SPEC_PER_CLASS, want, "replicated")


def test_cluster_voxels_on_one_run_lattice_event(lib):
    b, want = L.run_lattice(L.LATTICE, 2)
    _case("lattice", 1, int(b.off[-1]), int(want["count"][0]))
    _cluster(lib, b, ClusterSpec(26, None, True, 2), want, "lattice")


def test_cluster_features_on_the_replicated_list(lib):
    base, b, _, cb, _, cl, R, M = _random()
    _features(lib, b, cl, L.tile_features(L.features_statement(base, cb), R, M), "replicated")


def test_cluster_match_on_the_replicated_list_strides_over_its_slots(lib):
    base, b, ca, cb, cl_a, cl_b, R, _ = _random()
    want = L.tile_match(L.match_statement(base, ca, cb), R)
    assert L.match_slots(b.off[-1]) == 2 ** 23 and want["pair_offsets"][-1] >= cl_b["table_offsets"][-1] > 3 * cl_a["table_offsets"][-1]
    _match(lib, b, cl_a, cl_b, want, "replicated")


def test_cluster_graph_on_the_replicated_list(lib):
    base, b, _, cb, _, cl, R, M = _random()
    want = L.tile_graph(L.graph_statement(base, cb, 1), R, M)
    assert want["edges"].shape[0] > 50000
    _graph(lib, b, cl, want, "replicated")


# ---- rows: single-voxel and two-voxel clusters past the strides of cluster_features ---------------------------------------------------
@pytest.mark.parametrize("name,R", [("rows_40k", L.R_ROWS_40K), ("rows_262k", L.R_ROWS_262K)], ids=["rows_40k", "rows_262k"])
def test_cluster_features_with_more_rows_than_one_trip_of_its_row_kernels(lib, name, R):
    base = L.own_rows_base(pairs_join=True)
    cb = L.cluster_statement(base, L.SPEC_ROWS)
    b, cl = L.repeat(base, R), L.tile_cluster(cb, R)
    _case(name, b.off.size - 1, int(b.off[-1]), int(cl["table_offsets"][-1]))
    want = L.tile_features(L.features_statement(base, cb), R, int(base.off[-1]))
    assert sorted(set(want["n"])) == [1, 2]
    _features(lib, b, cl, want, name)


# ---- more than 2^22 rows, shared by match, graph and features -------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _rows_4m():
    base = L.own_rows_base()
    cb = L.cluster_statement(base, L.SPEC_ROWS)
    R = L.R_ROWS_4M
    b, cl = L.repeat(base, R), L.tile_cluster(cb, R)
    return base, cb, b, cl, R, int(base.off[-1])


def test_cluster_match_with_more_rows_than_one_trip(lib):
    base, cb, b, cl, R, _ = _rows_4m()
    _case("rows_4m", b.off.size - 1, int(b.off[-1]), int(cl["table_offsets"][-1]))
    rev, rev_base = L.reversed_ids(cl, b.off), L.reversed_ids(cb, base.off)
    want = L.tile_match(L.match_statement(base, cb, rev_base), R)
    assert want["pair_offsets"][-1] == b.off[-1] == want["event_int"][:, 7].sum()          # every entry a cell, every row mutual
    _match(lib, b, cl, rev, want, "rows_4m")


def test_cluster_graph_with_more_rows_and_groups_than_one_trip(lib):
    base, cb, b, cl, R, M = _rows_4m()
    want = L.tile_graph(L.graph_statement(base, cb, 1), R, M)
    _case("rows_4m", b.off.size - 1, int(b.off[-1]), int(cl["table_offsets"][-1]), edge_cap=want["edges"].shape[0])
    assert want["groups"].shape[0] == cl["table_offsets"][-1] - want["edges"].shape[0] > L.CG_STRIDE
    _graph(lib, b, cl, want, "rows_4m")


def test_cluster_features_with_more_than_four_million_rows(lib):
    base, cb, b, cl, R, M = _rows_4m()
    _features(lib, b, cl, L.tile_features(L.features_statement(base, cb), R, M), "rows_4m")


# ---- cluster_graph: more than 1024 rows for its scan; a slot table wider than one trip over a tiny list --------------------------------
def _checkerboard_12():
    shape = (12, 12, 12)
    x = np.stack(np.unravel_index(np.arange(1728), shape), 1)
    b = L.Batch(shape, np.array([0, 1728], np.int64), np.arange(1728, dtype=np.int64), (1 + x.sum(1) % 2).astype(np.uint8),
                np.random.default_rng(12).uniform(-3.0, 40.0, 1728).astype(np.float32))
    return b, L.cluster_statement(b, ClusterSpec(6, (1, 2), True, 1))


def _checkerboard_3x8():
    shape, off, index, cls, ids, toff, tcls = TG._checkerboard(n=3)
    b = L.Batch(shape, off, index, cls, np.random.default_rng(8).uniform(-3.0, 40.0, index.size).astype(np.float32))
    return b, {"cluster": ids, "table_offsets": toff, "cls": tcls}


@pytest.mark.parametrize("name,build", [("checkerboard_3x8", _checkerboard_3x8), ("checkerboard_12", _checkerboard_12)],
                         ids=["checkerboard_3x8", "checkerboard_12"])
def test_cluster_graph_scans_two_rows_per_thread(lib, name, build):
    b, cl = build()
    _case(name, b.off.size - 1, int(b.off[-1]), int(cl["table_offsets"][-1]))
    want = L.graph_statement(b, cl, 1)
    assert want["events"][:, 0].tolist() == [1] * (b.off.size - 1)
    _graph(lib, b, cl, want, name)


def test_cluster_graph_strides_over_a_slot_table_far_wider_than_the_list(lib):
    b, cl = _checkerboard_3x8()
    c = L.BY_NAME["checkerboard_wide_table"]
    _case(c.name, b.off.size - 1, int(b.off[-1]), int(cl["table_offsets"][-1]))
    assert L.graph_slots(c.edge_cap) == 2 ** 23
    _graph(lib, b, cl, L.graph_statement(b, cl, 1), c.name, edge_cap=c.edge_cap)


# ---- crop_write with more than 1024 boxes ----------------------------------------------------------------------------------------------
def test_crop_write_scans_two_boxes_per_thread(lib):
    big, tile = L.CROP_BIG, L.CROP_TILE
    boxes = tiling.grid(big, tile, L.CROP_HALO, n=3)
    _case("crop_boxes", 3, 0, boxes=len(boxes))
    vb = TT._random_batch(41, big, (150, 0, 2500))                  # a sparse event, one without entries (357 empty boxes), a dense one
    got = TT._device_crop(lib, vb, big, tile, boxes)
    _, src, owned = TT._check_crop(got, vb, big, tile, boxes, "1071 boxes")
    assert (got["count"][:357] == 0).sum() > 50 and (got["count"][357:714] == 0).all() and (got["count"][714:] > 0).sum() > 300
    assert np.array_equal(np.sort(src[owned == 1]), np.arange(2650))
    TT._check_crop(TT._device_crop(lib, vb, big, tile, boxes, scratch_fill=0x00), vb, big, tile, boxes, "scratch 0x00")
    _release()


# ---- many small events: the statements directly ------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _small(name, seed):
    c = L.BY_NAME[name]
    b = L.small_events(c.n, c.m_total, seed)
    _case(name, b.off.size - 1, int(b.off[-1]))
    return b, L.cluster_statement(b, L.SPEC_ROWS), L.cluster_statement(b, ClusterSpec(6, None, False, 1))


SMALL = [("small_events_5000", 3), ("small_events_700", 4)]


@pytest.mark.parametrize("name,seed", SMALL, ids=[s[0] for s in SMALL])
def test_cluster_voxels_on_many_small_events(lib, name, seed):
    b, cl, cl6 = _small(name, seed)
    _cluster(lib, b, L.SPEC_ROWS, cl, name)
    _cluster(lib, b, ClusterSpec(6, None, False, 1), cl6, name)


@pytest.mark.parametrize("name,seed", SMALL, ids=[s[0] for s in SMALL])
def test_cluster_features_on_many_small_events(lib, name, seed):
    b, cl, _ = _small(name, seed)
    _features(lib, b, cl, L.features_statement(b, cl), name)


@pytest.mark.parametrize("name,seed", SMALL, ids=[s[0] for s in SMALL])
def test_cluster_match_on_many_small_events(lib, name, seed):
    b, cl, cl6 = _small(name, seed)
    _match(lib, b, cl, cl6, L.match_statement(b, cl, cl6), name)


@pytest.mark.parametrize("name,seed", SMALL, ids=[s[0] for s in SMALL])
def test_cluster_graph_on_many_small_events(lib, name, seed):
    b, cl, _ = _small(name, seed)
    for gap in (1, 3):
        _graph(lib, b, cl, L.graph_statement(b, cl, gap), name, gap=gap)
