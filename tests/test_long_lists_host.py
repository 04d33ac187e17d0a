"""Host half of the long-list tests (tests/_long_lists.py), on a CPU: the tiled expectation of a replicated batch
equals the statement run directly on the repeated batch; the run lattice's closed form equals cluster_numpy; the thresholds the
helper names are the constants of the sources; and every GPU case of tests/test_long_lists_gpu.py crosses, raggedly, the threshold
it is named for -- by arithmetic on those constants, so a retuned kernel fails here instead of dropping a case back under it."""
import functools
import os
import re

import numpy as np
import pytest

import _long_lists as L
from uresnet_amd import tiling

CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "u-resnet_amd", "csrc")


def _same(got, want):
    """Every table equal, fp64 / fp32 by bits, dtypes included."""
    assert sorted(got) == sorted(want)
    for k in want:
        g, w = np.ascontiguousarray(got[k]), np.ascontiguousarray(want[k])
        assert g.dtype == w.dtype and g.shape == w.shape, (k, g.dtype, w.dtype, g.shape, w.shape)
        assert np.array_equal(g.view(np.uint8), w.view(np.uint8)), k


# ---- replicated events -----------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _base(kind):
    """A base batch small enough to run the statements on three copies of it: the builders of the GPU cases at smaller shapes."""
    if kind == "random":
        return L.random_base(seed=5, shape=(8, 7, 9), occupancy=0.5)
    if kind == "rows":
        return L.own_rows_base(seed=6, shape=(8, 8, 8), pairs=3)
    if kind == "rows_join":
        return L.own_rows_base(seed=7, pairs_join=True, shape=(8, 8, 8), pairs=3)
    return L.small_events(40, 60, 8, empty_runs=((5, 12),))


KINDS = ["random", "rows", "rows_join", "small"]


def _specs(kind):
    return (L.SPEC_ANY_CLASS, L.SPEC_PER_CLASS) if kind == "random" else (L.SPEC_ROWS, L.ClusterSpec(6, None, False, 1))


@pytest.mark.parametrize("R", [2, 3])
@pytest.mark.parametrize("kind", KINDS)
def test_the_tiled_expectation_equals_the_statement_on_the_repeated_batch(kind, R):
    b = _base(kind)
    rep = L.repeat(b, R)
    M = int(b.off[-1])
    assert rep.off.size == R * (b.off.size - 1) + 1 and int(rep.off[-1]) == R * M
    spec_a, spec_b = _specs(kind)
    ca, cb = L.cluster_statement(b, spec_a), L.cluster_statement(b, spec_b)
    ra, rb = L.cluster_statement(rep, spec_a), L.cluster_statement(rep, spec_b)
    _same(L.tile_cluster(ca, R), ra)
    _same(L.tile_cluster(cb, R), rb)
    assert ca["table_offsets"][-1] > 0 and cb["table_offsets"][-1] > 0
    _same(L.tile_features(L.features_statement(b, cb), R, M), L.features_statement(rep, rb))
    _same(L.tile_match(L.match_statement(b, ca, cb), R), L.match_statement(rep, ra, rb))
    for gap in (1, 2):
        want = L.graph_statement(rep, rb, gap)
        _same(L.tile_graph(L.graph_statement(b, cb, gap), R, M), want)
    if kind != "small":
        assert want["edges"].shape[0] > 0                    # the columns that move are there to be moved


def test_the_columns_that_move_are_the_only_ones_that_differ_between_replicas():
    """The converse of the test above: without the shift the tiled tables are wrong exactly in end_lo / end_hi and pos_a / pos_b."""
    b = _base("random")
    M = int(b.off[-1])
    cb = L.cluster_statement(b, L.SPEC_PER_CLASS)
    rep = L.repeat(b, 2)
    rb = L.cluster_statement(rep, L.SPEC_PER_CLASS)
    f, g = L.features_statement(rep, rb), L.graph_statement(rep, rb)
    f0, g0 = L.tile_features(L.features_statement(b, cb), 2, 0), L.tile_graph(L.graph_statement(b, cb), 2, 0)
    assert sorted(k for k in f if not np.array_equal(f[k], f0[k])) == ["end_hi", "end_lo"]
    assert [k for k in g if not np.array_equal(g[k], g0[k])] == ["edges"]
    assert np.array_equal(g["edges"][:, :4], g0["edges"][:, :4]) and (g["edges"][:, 4:] != g0["edges"][:, 4:]).any()


def test_the_base_batches_of_the_gpu_cases_are_ones_the_statements_accept():
    """No id outside [-1, K_e), no row without a member: the statements raise on either, so running them is the check; and the
    numbers of the case table are those of the builders."""
    b = L.random_base()
    ca, cb = L.cluster_statement(b, L.SPEC_ANY_CLASS), L.cluster_statement(b, L.SPEC_PER_CLASS)
    L.features_statement(b, cb), L.match_statement(b, ca, cb), L.graph_statement(b, cb)
    c = L.BY_NAME["random_replicated"]
    assert (c.n, c.m_total, c.rows) == (3 * L.R_RANDOM, L.R_RANDOM * int(b.off[-1]), L.R_RANDOM * int(cb["table_offsets"][-1]))
    assert b.off[1] == b.off[2] and (cb["cluster"] == -1).any()                      # an empty event; dropped entries
    for join, names, Rs in ((True, ("rows_40k", "rows_262k"), (L.R_ROWS_40K, L.R_ROWS_262K)), (False, ("rows_4m",), (L.R_ROWS_4M,))):
        o = L.own_rows_base(pairs_join=join)
        co = L.cluster_statement(o, L.SPEC_ROWS)
        L.features_statement(o, co)
        g = L.graph_statement(o, co)
        L.match_statement(o, co, L.reversed_ids(co, o.off))
        K, M, NE = int(co["table_offsets"][-1]), int(o.off[-1]), int(g["edge_offsets"][-1])
        assert sorted(set(co["size"])) == ([1, 2] if join else [1]) and (join or (K == M and 0 < NE < 20))
        assert int(g["group_offsets"][-1]) == K - NE                               # the edges join pairs (a forest): groups = rows - edges
        for name, R in zip(names, Rs):
            c = L.BY_NAME[name]
            assert (c.n, c.m_total, c.rows) == (3 * R, R * M, R * K), name
            assert join or c.edge_cap == R * NE
    for name, seed in (("small_events_5000", 3), ("small_events_700", 4)):
        c = L.BY_NAME[name]
        s = L.small_events(c.n, c.m_total, seed)
        sizes = np.diff(s.off)
        assert sizes[0] == sizes[-1] == 0 and sizes.max() <= 6 and s.off.size == c.n + 1 and s.off[-1] == c.m_total
        cs = L.cluster_statement(s, L.SPEC_ROWS)
        L.features_statement(s, cs), L.graph_statement(s, cs), L.match_statement(s, cs, L.cluster_statement(s, L.ClusterSpec(6, None, False)))
        empty = "".join("e" if x == 0 else "." for x in sizes)
        assert name != "small_events_5000" or len(re.findall("e{300,}", empty[1:-1])) >= 2      # runs of 300+ empty events
        all_dropped = [e for e in range(c.n) if sizes[e] and (cs["cluster"][s.off[e]:s.off[e + 1]] == -1).all()]
        assert len(all_dropped) >= 5


# ---- the run lattice -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("min_size", [1, 2])
@pytest.mark.parametrize("shape", L.LATTICE_SMALL, ids=lambda s: "x".join(map(str, s)))
def test_the_run_lattice_equals_cluster_numpy(shape, min_size):
    b, want = L.run_lattice(shape, min_size)
    M = int(b.off[-1])
    assert 300 < M < 6000
    _same(want, L.cluster_statement(b, L.ClusterSpec(26, None, True, min_size)))
    x = np.unravel_index(b.index, shape)[2]
    if shape[2] % 15:
        assert (x == shape[2] - 1).any() and (x == 0).any()                          # runs cut off by the row end
    sizes = np.bincount(L.run_lattice(shape, 1)[1]["cluster"])
    assert sorted(set(sizes)) == [1, 2, 3, 4]
    assert min_size == 1 or ((want["cluster"] == -1).sum() == (sizes == 1).sum() and want["size"].min() == 2)


def test_the_long_lattice_drops_runs_on_both_sides_of_every_span_boundary():
    """In every 2048-entry span of the long lattice some runs are dropped and some kept, so every count cluster_scan sums is
    non-trivial; the spans' counts differ from each other; and the numbers are those of the case table."""
    b, want = L.run_lattice(L.LATTICE, 2)
    c = L.BY_NAME["lattice"]
    M = int(b.off[-1])
    assert (c.n, c.m_total, c.rows) == (1, M, int(want["count"][0]))
    dropped = want["cluster"] == -1
    kept_rep = np.zeros(M, bool)
    kept_rep[want["first"]] = True
    span = np.arange(M) // L.CL_SPAN
    nd, nk = np.bincount(span, dropped), np.bincount(span, kept_rep)
    assert nd.size == L.cdiv(M, L.CL_SPAN) and (nd > 0).all() and (nk > 0).all() and np.unique(nk[:-1]).size > 3
    for edge in range(L.CL_SPAN, M, L.CL_SPAN):                                      # ... within 16 entries of every boundary
        assert dropped[edge - 16:edge].any() and dropped[edge:edge + 16].any(), edge


# ---- the constants ---------------------------------------------------------------------------------------------------------------
def _src(name):
    with open(os.path.join(CSRC, name)) as f:
        return f.read()


def _define(text, name):
    m = re.findall(r"^#define %s (\d+)\b" % name, text, re.M)
    assert len(m) == 1, (name, m)
    return int(m[0])


def test_the_named_thresholds_are_the_constants_of_the_sources():
    vox, cl, til = _src("voxel_io.hip"), _src("cluster.hip"), _src("tiling.hip")
    cf, cm, cg = _src("cluster_features.hip"), _src("cluster_match.hip"), _src("cluster_graph.hip")
    assert _define(vox, "VOX_ITER") == L.VOX_ITER and re.search(r"^#define VOX_SPAN \(256 \* VOX_ITER\)", vox, re.M)
    assert _define(cl, "CL_ITER") == L.CL_ITER and re.search(r"^#define CL_SPAN \(256 \* CL_ITER\)", cl, re.M)
    for text, kernel, threads in ((vox, "voxel_scan_kernel", L.VOXEL_SCAN_THREADS), (cl, "cluster_scan_kernel", L.CLUSTER_SCAN_THREADS),
                                  (til, "crop_scan_kernel", L.CROP_SCAN_THREADS)):
        launch = re.findall(r"hipLaunchKernelGGL\(%s, dim3\(1\), dim3\((\d+)\)" % kernel, text)
        assert launch == [str(threads)], (kernel, launch)
        assert len(re.findall(r"__launch_bounds__\(%d\) void %s\(" % (threads, kernel), text)) == 1, kernel
        body = text[text.index("void %s(" % kernel):]
        assert re.search(r"chunk = \(B \+ %d\) / %d;" % (threads - 1, threads), body[:1500]), kernel
    assert _define(cf, "CF_ROW_BLOCKS") == L.CF_ROW_BLOCKS and re.search(r"^#define CF_I URSN_CLFEAT_I$", cf, re.M)
    assert "rb256 > CF_ROW_BLOCKS ? CF_ROW_BLOCKS : rb256" in cf and "rb64 > 4 * CF_ROW_BLOCKS ? 4 * CF_ROW_BLOCKS : rb64" in cf
    assert "ib > 4 * CF_ROW_BLOCKS ? 4 * CF_ROW_BLOCKS : ib)), dim3(256)" in cf and "cdiv64(a.rows_max * CF_I, 256)" in cf
    assert "cdiv64(a.rows_max, 256), rb64 = cdiv64(a.rows_max, 64)" in cf
    assert "clfeat_axis_kernel, rows64, dim3(64)" in cf and "clfeat_anchor_kernel, rows256, dim3(256)" in cf
    assert "clfeat_ends_kernel, rows256, dim3(256)" in cf
    assert _define(cm, "CM_GRID_CAP") == L.CM_GRID_CAP and _define(cm, "CM_SCAN_THREADS") == L.CM_SCAN_THREADS
    assert _define(cg, "CG_GRID_CAP") == L.CG_GRID_CAP and _define(cg, "CG_SCAN_THREADS") == L.CG_SCAN_THREADS
    assert "b > CM_GRID_CAP ? CM_GRID_CAP : b" in cm and "b > CG_GRID_CAP ? CG_GRID_CAP : b" in cg
    assert "clmatch_event_kernel, dim3((unsigned)cdiv64(d->n, 256)), dim3(256)" in cm
    assert "while (t < 2 * (m_total < 1 ? 1 : m_total)) t <<= 1;" in cm and "while (t < 2 * edge_cap + 2) t <<= 1;" in cg
    assert (L.CM_STRIDE, L.CG_STRIDE, L.CF_INIT_THREADS, L.CF_ROW256_THREADS, L.CF_ROW64_THREADS) == (2 ** 22, 2 ** 22, 2 ** 20, 2 ** 18, 2 ** 18)


# ---- every case crosses its threshold, raggedly -------------------------------------------------------------------------------------
def _ragged_scan(items, threads, whole_waves=False):
    """A one-workgroup scan over `items` takes a second step in some thread, its chunk count is no multiple of 1024 or 256
    (whole_waves: of 1024 only -- the 3 x 8^3 checkerboard has 6 x 256 rows; the 12^3 one beside it is ragged), the last thread's
    chunk is short or empty and the trailing threads own nothing."""
    chunk, last_owner, last = L.scan_chunks(items, threads)
    assert chunk >= 2 and items % 1024 and (whole_waves or items % 256), (items, chunk)
    assert last == (items, items), (items, last)                                      # lo == hi == B
    assert last_owner[1] == items and 0 < last_owner[1] - last_owner[0] <= chunk


def _ragged_stride(items, stride, unit=256):
    """A striding kernel takes a second trip that is neither full nor a whole number of workgroups."""
    assert stride < items < 2 * stride and (items - stride) % unit, (items, stride)


def _voxel_scan(c):
    _ragged_scan(L.cdiv(c.m_total, L.VOX_SPAN), L.VOXEL_SCAN_THREADS)
    assert c.m_total > 2 ** 21 and c.m_total % L.VOX_SPAN and c.n >= 2


def _cluster_scan(c):
    _ragged_scan(L.cdiv(c.m_total, L.CL_SPAN), L.CLUSTER_SCAN_THREADS)
    assert c.m_total > 2 ** 21 + 2048 and c.m_total % L.CL_SPAN and c.m_total % 256


def _event_blocks(c):
    assert c.n > L.EVENT_BLOCK and c.n % L.EVENT_BLOCK and c.n % 64                   # clmatch_event, and the `j <= n` threads


CROSSES = {
    "voxel_scan": _voxel_scan,
    "cluster_scan": _cluster_scan,
    "crop_scan": lambda c: _ragged_scan(c.boxes, L.CROP_SCAN_THREADS),
    "graph_scan": lambda c: _ragged_scan(c.rows, L.CG_SCAN_THREADS, whole_waves=c.name == "checkerboard_3x8"),
    "clfeat_init": lambda c: (_ragged_stride(c.rows * L.CF_I, L.CF_INIT_THREADS), _is(c.rows < L.CF_ROW256_THREADS)),
    "clfeat_rows": lambda c: (_ragged_stride(c.rows, L.CF_ROW256_THREADS), _ragged_stride(c.rows, L.CF_ROW64_THREADS, 64)),
    "match_slots": lambda c: (_is(L.match_slots(c.m_total) == 2 * L.CM_STRIDE), _is(c.m_total > 2 ** 21)),
    "graph_slots": lambda c: (_is(L.graph_slots(c.edge_cap) == 2 * L.CG_STRIDE), _is(c.edge_cap >= 2 ** 21), _is(c.m_total < 4096)),
    "match_rows": lambda c: (_ragged_stride(c.rows, L.CM_STRIDE), _ragged_stride(c.m_total, L.CM_STRIDE)),
    "graph_rows": lambda c: (_ragged_stride(c.rows, L.CG_STRIDE), _ragged_stride(c.rows - c.edge_cap, L.CG_STRIDE), _is(0 < c.edge_cap < 2 ** 17)),
    "entry_blocks": lambda c: _is(L.cdiv(c.m_total, 256) > 8000),
    "event_blocks": _event_blocks,
    "events_over_entries": lambda c: _is(c.n + 1 > c.m_total > 0),
}


def _is(x):
    assert x


@pytest.mark.parametrize("case", L.CASES, ids=lambda c: c.name)
def test_the_case_crosses_the_threshold_it_is_named_for(case):
    assert case.crosses and 1 <= case.n <= 65535 and case.m_total < 2 ** 31
    for what in case.crosses:
        CROSSES[what](case)


def test_every_row_of_the_threshold_table_has_a_named_case():
    have = {w for c in L.CASES for w in c.crosses}
    assert have == set(CROSSES), set(CROSSES) ^ have
    names = [c.name for c in L.CASES]
    assert len(set(names)) == len(names)


def test_the_shapes_of_the_label_and_crop_cases_give_the_numbers_of_the_table():
    assert int(np.prod(L.LABELS_3D)) == L.BY_NAME["labels_3d"].m_total and L.cdiv(L.BY_NAME["labels_3d"].m_total, L.VOX_SPAN) == 1065
    assert int(np.prod(L.LABELS_2D)) == L.BY_NAME["labels_2d"].m_total == 2 ** 21 + 2048 + 256
    c = L.BY_NAME["crop_boxes"]
    assert len(tiling.grid(L.CROP_BIG, L.CROP_TILE, L.CROP_HALO, n=c.n)) == c.boxes
    assert L.BY_NAME["checkerboard_3x8"].rows == 3 * 8 ** 3 and L.BY_NAME["checkerboard_12"].rows == 12 ** 3
