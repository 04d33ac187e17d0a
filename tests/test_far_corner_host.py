"""Host half of the far-corner tests (tests/_far_corner.py), on a CPU.  The statements are translation-equivariant:
at the large shape they equal, bit for bit, what they give in the small frame in every column that is not a position, and the
positions differ by exactly the event's shift -- so the GPU tests' expected values are not "whatever the statement says" alone.
Every batch the GPU modules run reaches what it is named for: the far faces, the last plane of the volume, both sides of index
2^30, search windows and balls that a far face clips.  The arithmetic bounds the header states hold on the long track.  Every shape
is accepted by the scratch queries and the argument checks of the calls it is used with and refused one step further; the calls
below are all refused before any device access, so the fake pointers are never dereferenced."""
import functools

import numpy as np
import pytest

import _far_corner as far
import test_cluster_chain_host as chain_host
import test_cluster_cone_host as cone_host
import test_cluster_features_host as features_host
import test_cluster_graph_host as graph_host
import test_cluster_profile_host as profile_host
import test_cluster_split_host as split_host
import test_cluster_vertex_host as vertex_host
import test_clusters_host as clusters_host
import test_tiling_host as tiling_host
from uresnet_amd import clusters as C
from uresnet_amd import symmetry as S

SOURCES = {"cluster": "random", "features": "random", "graph": "random", "profile": "random", "vertex": "random", "chain": "chain",
           "cone": "cone", "split": "split"}
IDS = dict(ids=far.shape_id)
PLACED = (far.FAR, far.ORIGIN, far.MIDDLE)


def _spec(family, shape):
    if family == "cluster":
        return far.SPEC_3D if len(shape) == 3 else far.SPEC_2D
    return far.WIDEST.get(family)


@functools.lru_cache(maxsize=None)
def _small_statement(family, small_shape, key):
    """The statement in the small frame, once per distinct small batch (the roomy shapes share theirs)."""
    return far.statement(family, _small_statement.batches[key], _spec(family, small_shape))


_small_statement.batches = {}


def _statements(family, shape):
    fb = far.far_batch(SOURCES[family], shape)
    key = (family, fb.small.shape, fb.small.index.tobytes())
    _small_statement.batches[key] = fb.small
    return fb, _small_statement(family, fb.small.shape, key), far.statement(family, fb.big, _spec(family, shape))


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint8)


# ---- equivariance ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", far.SHAPES_CAPPED, **IDS)
@pytest.mark.parametrize("family", sorted(SOURCES))
def test_the_statements_are_translation_equivariant(family, shape):
    fb, small, big = _statements(family, shape)
    ws, wb = far.flatten(family, small), far.flatten(family, big)
    assert sorted(ws) == sorted(wb) and set(far.COORD_COLUMNS[family]) <= set(ws)
    shifts = np.zeros((fb.shifts.shape[0], 3), np.int64)
    shifts[:, :len(shape)] = fb.shifts
    moved = 0
    for k in sorted(ws):
        a, b = ws[k], wb[k]
        assert a.dtype == b.dtype and a.shape == b.shape, k
        if k not in far.COORD_COLUMNS[family]:
            assert np.array_equal(_bits(a), _bits(b)), (k, "differs and is not a position")
            continue
        kind, count = far.COORD_COLUMNS[family][k]
        if kind == "free":                                   # formed from bin centroids, which are anchor + sum / n: they round with them
            assert np.allclose(a, b, rtol=1e-12, atol=1e-9, equal_nan=True), k
            continue
        owner = far.event_of_rows(family, k, big, fb.big.toff)
        assert owner.size == a.shape[0], k
        move = shifts[owner] if a.ndim == 2 else shifts[owner, int(k[-1])]
        if kind == "sum":
            n = wb[k.rsplit(".", 1)[0] + "." + count if "." in k else count]
            move = move * (n[:, None] if a.ndim == 2 else n)
        if k.startswith("bins."):                            # a segment without members has no centroid: zeros, here and there
            move = np.where(wb["bins.n"] == 0, 0, move)
        if kind == "real":                                   # anchor + sum / n below 2^15 in fp64: a few ulp of 2^-38
            assert np.abs(b - (a + move)).max(initial=0.0) <= 2.0 ** -30, k
        else:
            assert np.array_equal(b.astype(np.int64) - a, move), k
        moved += int(np.any(move != 0))
    assert moved > 0 or not far.COORD_COLUMNS[family]        # the columns that move are there to be moved


def test_translate_is_what_the_batches_are_made_by():
    for family, shape in (("random", far.LARGEST_VOLUME), ("split", far.CAPPED_2D), ("cone", far.LARGEST_PLANE)):
        fb = far.far_batch(family, shape)
        assert np.array_equal(far.translate(fb.small.off, fb.small.index, fb.small.shape, shape, fb.shifts), fb.big.index)
    index, box, lo = far.crop(np.array([130, 131, 262]), (8, 8, 16))
    assert box == (2, 1, 5) and lo.tolist() == [1, 0, 2] and index.tolist() == [0, 1, 9]


# ---- every batch reaches what it is named for ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", far.SHAPES_VOLUME, **IDS)
@pytest.mark.parametrize("source", ["random", "chain", "cone", "split"])
def test_every_batch_reaches_the_faces_the_last_plane_and_both_sides_of_the_pivot(source, shape):
    fb = far.far_batch(source, shape)
    b, V = fb.big, far.volume(shape)
    assert V < far.MAX_VOLUME and (shape == far.WIDEST_2D or max(shape) <= far.MAX_EXTENT)
    x = far.coords(b.index, shape)
    assert (x.max(axis=0) == np.array(shape) - 1).all()                                         # some entry on each far face
    assert int(b.index.max()) >= V - far.volume(shape[1:])                                      # within one plane of V
    assert far.pivot(shape) == (2 ** 30 if shape != far.CAPPED_2D else 2 ** 29)
    for e, where in enumerate(fb.placement):
        ie, xe = b.index[b.off[e]:b.off[e + 1]], x[b.off[e]:b.off[e + 1]]
        assert (where is None) == (ie.size == 0) and (np.diff(ie) > 0).all()
        if where == far.FAR:
            assert (xe.max(axis=0) == np.array(shape) - 1).all()
        if where == far.ORIGIN:
            assert (xe.min(axis=0) == far.coords(fb.small.index[b.off[e]:b.off[e + 1]], fb.small.shape).min(axis=0)).all()
        if where == far.MIDDLE:
            assert ie.min() < far.pivot(shape) <= ie.max()
    used = [s for s in far.sources(source, len(shape)) if far.fits(s, shape)]
    longest = max(int((np.diff(s.off) > 1).sum()) for s in used)                                # events of one source take the placements in turn
    assert set(PLACED[:min(longest, 3)]) <= set(fb.placement), fb.placement
    assert source != "random" or longest >= 3                                                   # the lists most calls run: all three, in every shape


@pytest.mark.parametrize("shape", far.SHAPES_CAPPED, **IDS)
def test_joins_and_links_are_accepted_through_windows_a_far_face_clips(shape):
    """At max_gap 31 / reach 127 the window around the end point / apex of an accepted join / link would extend past S_a - 1."""
    top = np.array(shape) - 1
    for family, table, columns, reach in (("chain", "joins", ("pos_a", "pos_b"), 31), ("cone", "links", ("pos",), 127)):
        fb, _, want = _statements(family, shape)
        rows = want[table]
        assert rows[columns[0]].size > 0
        clipped = np.zeros(rows[columns[0]].size, bool)
        for c in columns:
            clipped |= (far.coords(fb.big.index[rows[c]], shape) + reach > top).any(axis=1)
        assert clipped.any(), family


@pytest.mark.parametrize("shape", far.SHAPES_CAPPED, **IDS)
def test_a_junction_lies_within_the_radius_of_a_far_face(shape):
    _, _, want = _statements("split", shape)
    j = want["junctions"]
    hi = np.stack([j["hi%d" % a] for a in range(len(shape))], axis=1)
    assert j["row"].size > 0 and (hi + far.WIDEST["split"].radius > np.array(shape) - 1).any()


# ---- the long track and the header's bounds ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("axis", sorted(far.LONG_TRACK))
def test_the_long_track_holds_the_bounds_the_header_states(axis):
    s = far.long_track(far.LONG_TRACK[axis])
    x = far.coords(s.index, s.shape)
    assert s.index.size == 32768 and sorted(x[:, axis].tolist()) == list(range(32768))
    assert (np.abs(np.diff(x[np.argsort(x[:, axis])], axis=0)) <= 1).all()                      # 26-connected, end to end
    f = far.statement("features", s)
    nb, nb_true, _ = C.profile_bin_count(f["length"][0], 0.5, C.PROFILE_MAX_BINS)
    print("axis %d: n %d  max|s| %d  max|dd| %d  length %.2f  nb %d of %d" % (axis, f["n"][0], np.abs(f["s"]).max(), np.abs(f["dd"]).max(),
                                                                             f["length"][0], nb, nb_true))
    assert f["n"].tolist() == [32768] and np.abs(f["s"]).max() < 2 ** 46 and np.abs(f["dd"]).max() < 2 ** 61 and nb <= 65536
    assert f["dd"][0][axis] > 2.9e12 and f["length"][0] > 32767
    if axis == 0:
        assert abs(f["length"][0] - 32768.98) < 0.01 and nb == 65536 < nb_true
        g = far.statement("features", far.long_track(far.LONG_TRACK[0], 150))
        assert C.profile_bin_count(g["length"][0], 0.5, C.PROFILE_MAX_BINS)[:2] == (65536, 65536)   # the stated maximum, not cut


# ---- the symmetry remap in closed form -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("spatial", [(5, 5, 5), (6, 6), (4, 6, 6), (3, 3, 7)], **IDS)
def test_the_closed_form_of_the_remap_is_apply_numpy(spatial):
    nd, V = len(spatial), int(np.prod(spatial))
    codes = [int(c) for c in S.group("cube", spatial)]
    assert len(codes) in (8, 16, 48)
    for c in codes:
        where = np.argsort(S.apply_numpy(np.arange(V, dtype=np.int64).reshape(spatial), spatial, c).reshape(-1))
        got = far.remap_closed_form(np.arange(-1, V + 2), spatial, S.perms(nd)[c >> nd], [(c >> k) & 1 for k in range(nd)])
        assert np.array_equal(got[1:V + 1], where) and got[0] == -1 and got[V + 1:].tolist() == [V, V + 1], (spatial, c)
    for spatial in (far.CUBE, far.WIDEST_2D):
        assert len(S.group("cube", spatial)) == S.count(len(spatial)) and 2 ** 31 - 2 ** 20 < far.volume(spatial) < 2 ** 31


# ---- accepted, and refused one step further ----------------------------------------------------------------------------------------------
PAST = b": scratch of 0 bytes is too small"          # what a call says whose other arguments were all accepted
WIDEST_ARGS = {"features": {}, "graph": dict(gap=3), "profile": dict(step=0.5, end_bins=16, max_bins=65536), "vertex": dict(radius=3),
               "chain": dict(max_gap=31), "cone": dict(reach=127), "split": dict(radius=3)}
HOSTS = {"features": features_host, "graph": graph_host, "profile": profile_host, "vertex": vertex_host, "chain": chain_host,
         "cone": cone_host, "split": split_host}


def _one_step_further(shape):
    """The shapes one step outside: the last axis one longer where that leaves the contract, else the first."""
    out = []
    for a in (len(shape) - 1, 0):
        s = list(shape)
        s[a] += 1
        if s[a] > far.MAX_EXTENT or far.volume(s) >= far.MAX_VOLUME:
            out.append(tuple(s))
    assert out, shape
    return out


@pytest.mark.parametrize("shape", far.SHAPES_CAPPED, **IDS)
def test_the_capped_calls_accept_the_shape_and_refuse_one_step_further(lib, shape):
    nd = len(shape)
    pad = lambda s: tuple(s) + (0,) * (3 - len(s))
    for family, host in sorted(HOSTS.items()):
        host._refused(lib, PAST, ndim=nd, spatial=pad(shape), sbytes=0, **WIDEST_ARGS[family])
        for worse in _one_step_further(shape):
            with pytest.raises(AssertionError):                                       # refused, and not for its scratch
                host._refused(lib, PAST, ndim=nd, spatial=pad(worse), sbytes=0, **WIDEST_ARGS[family])
            host._refused(lib, b"", ndim=nd, spatial=pad(worse), sbytes=0, **WIDEST_ARGS[family])
    for family, q in (("features", lambda n, m: lib.ursn_cluster_features_scratch_bytes(n, m, m)),
                      ("chain", lib.ursn_cluster_chains_scratch_bytes), ("cone", lib.ursn_cluster_cones_scratch_bytes),
                      ("split", lib.ursn_cluster_split_scratch_bytes)):
        b = far.far_batch(SOURCES[family], shape).big
        assert q(b.off.size - 1, int(b.off[-1])) >= 8, family


@pytest.mark.parametrize("shape", far.SHAPES_VOLUME, **IDS)
def test_the_volume_calls_accept_the_shape_and_refuse_one_step_further(lib, shape):
    nd = len(shape)
    conn = 26 if nd == 3 else 8
    clusters_host._refused(lib, PAST, ndim=nd, spatial=shape, connectivity=conn, sbytes=0)
    tile = (16,) * nd
    for refused in (tiling_host._count_refused, tiling_host._write_refused):
        refused(lib, PAST, ndim=nd, big=shape, tile=tile, sbytes=0)
    sp = (tiling_host.ctypes.c_int32 * nd)
    assert lib.ursn_crop_scratch_bytes(nd, sp(*shape), sp(*tile), 9) > 0
    b = far.far_batch("random", shape).big
    assert lib.ursn_cluster_scratch_bytes(b.off.size - 1, int(b.off[-1])) >= 8
    s = list(shape)
    while far.volume(s) < far.MAX_VOLUME:                                             # the first shape past 2^31 voxels along axis 0
        s[0] += 1
    assert far.volume(s) - far.volume(shape[1:]) < far.MAX_VOLUME
    clusters_host._refused(lib, b": prod(spatial) >= 2^31", ndim=nd, spatial=tuple(s), connectivity=conn, sbytes=0)
    for refused in (tiling_host._count_refused, tiling_host._write_refused):
        refused(lib, b": prod(big) >= 2^31", ndim=nd, big=tuple(s), tile=tile, sbytes=0)
    assert lib.ursn_crop_scratch_bytes(nd, sp(*s), sp(*tile), 9) == 0
