"""Loss weights made on the device (include/uresnet_hip.h: ursn_make_weights; make_weights.hip), from the three kernels up to the
DEVICE_WEIGHTS driver switch.

Oracle: `_oracle` below, a second statement of the definition with explicit offset loops (for every foreground voxel and every
offset of Chebyshev norm 1..3: is the position inside the volume, does it hold another foreground class), independent of the
padded-slice one in uresnet_amd.weights; every case compares the two on the host before it looks at the device.  Weights are
compared bit for bit (tests/_abi.py::same_bits), counts exactly; nothing is skipped or tolerated.  Label, output, counts and scratch
are `_Guarded` buffers with canaries; every case runs with label and output on a 256-byte boundary (the 16-byte paths) and one
float past it (the scalar paths), and the bytes next to the output must keep their fill.

Shapes are the smallest that reach every path: volumes smaller than a tile and than the radius, ragged tiles in every axis, event
starts off 16 and off 4 bytes in the byte map (voxels % 16 and voxels % 4 != 0), exactly one tile, one tile plus one voxel in
each axis (2 x 2 x 2 tiles with a one-voxel rim), several spans of the write pass."""
import ctypes
import itertools
import re

import numpy as np
import pytest

from _abi import _Guarded, same_bits
from uresnet_amd import _lib, symmetry, uresnet
from uresnet_amd import synthetic_io as sio
from uresnet_amd.ssnet import VoxelBatch
from uresnet_amd.weights import WeightSpec, make_weights_numpy

pytestmark = pytest.mark.gpu

TILE3, TILE2 = (8, 8, 64), (64, 64)      # box tiles of the categorise pass; test_tile_constants pins them
SPAN = 4096                               # voxels per workgroup of the write pass
GUARD = 4096
SHAPES = [(1, 1, 1), (1, 1, 5), (3, 5, 7), (2, 6, 22), (17, 9, 70), (16, 16, 16), TILE3, tuple(t + 1 for t in TILE3),
          (1, 1), (5, 7), (33, 65), (64, 64), tuple(t + 1 for t in TILE2)]
NAN64 = 0x7FF8000000000000


def _ids(sp):
    return "x".join(str(s) for s in sp)


# ---- the oracle ------------------------------------------------------------------------------------------------------------
def _oracle_categories(label, sp, ncls):
    """Per event: class c [V] (-1 none) and d [V], the smallest Chebyshev distance (1..3, else 99) from a foreground voxel to a voxel
    of another foreground class inside the event's volume."""
    sp = tuple(sp)
    V = int(np.prod(sp))
    coords = np.stack(np.unravel_index(np.arange(V), sp), axis=1)
    offsets = [o for o in itertools.product(range(-3, 4), repeat=len(sp)) if any(o)]
    cs, ds = [], []
    for l in label:
        c = np.full(V, -1, np.int64)
        for v in np.flatnonzero((l > -1) & (l < ncls)):      # NaN compares false
            c[v] = int(l[v])                                 # int() truncates toward zero
        d = np.full(V, 99, np.int64)
        fg = np.flatnonzero(c >= 1)
        if fg.size and np.unique(c[fg]).size > 1:
            for off in offsets:
                q = coords[fg] + np.array(off)
                inside = np.ones(fg.size, bool)
                for a in range(len(sp)):
                    inside &= (q[:, a] >= 0) & (q[:, a] < sp[a])
                v = fg[inside]
                u = np.zeros(v.size, np.int64)
                for a in range(len(sp)):
                    u = u * sp[a] + q[inside, a]
                hit = (c[u] >= 1) & (c[u] != c[v])
                d[v[hit]] = np.minimum(d[v[hit]], max(abs(o) for o in off))
        cs.append(c)
        ds.append(d)
    return np.stack(cs), np.stack(ds)


def _oracle(cat, ncls, r, mode, scale):
    c, d = cat
    n, V = c.shape
    k = np.where((d <= r) & (c >= 1), ncls, c)
    counts = np.zeros((n, ncls + 1), np.int64)
    weight = np.zeros((n, V), np.float32)
    for e in range(n):
        for j in range(ncls + 1):
            counts[e, j] = int(np.count_nonzero(k[e] == j))
            if counts[e, j]:
                s = float(np.float32(scale[j]))
                weight[e, k[e] == j] = np.float32(s / float(counts[e, j])) if mode == "invfreq" else np.float32(s)
    return weight, counts


# ---- one device call -------------------------------------------------------------------------------------------------------
def _scratch(lib, sp, n, ncls, r, fill):
    import torch
    need = int(lib.ursn_make_weights_scratch_bytes(len(sp), (ctypes.c_int32 * 3)(*(list(sp) + [1])[:3]), n, ncls, r))
    assert need > 0
    g = _Guarded(need, GUARD, 0 if fill == "nan64" else fill)
    if fill == "nan64":
        g.view[:need // 8 * 8].view(torch.int64).fill_(NAN64)
    return g, need


def _make(lib, label, sp, ncls, r, mode, scale, shift=0, fill=0xFF, with_counts=True, scratch=None):
    """One ursn_make_weights call on host labels [n, V]; label and output start `shift` floats past a 256-byte boundary."""
    import torch
    n, V = label.shape
    nb = n * V * 4

    def place():
        g = _Guarded(nb + 32, GUARD, 0xFF)
        return g, g.ptr + 4 * shift, g.view[4 * shift:4 * shift + nb]

    gl, lptr, lview = place()
    lview.copy_(torch.from_numpy(np.ascontiguousarray(label).reshape(-1).view(np.uint8)))
    go, optr, oview = place()
    gc = _Guarded(n * (ncls + 1) * 8, GUARD, 0xFF)
    sc, need = scratch if scratch is not None else _scratch(lib, sp, n, ncls, r, fill)
    d = _lib.ursn_make_weights_desc()
    d.ndim, d.n, d.voxels, d.ncls, d.radius, d.mode = len(sp), n, V, ncls, r, ("class", "invfreq").index(mode)
    for i, s in enumerate(sp):
        d.spatial[i] = s
    for i in range(9):
        d.scale[i] = float(scale[i]) if i <= ncls else float("nan")      # entries past ncls are never read
    torch.cuda.synchronize()
    _lib.check(lib.ursn_make_weights(ctypes.byref(d), ctypes.c_void_p(lptr), ctypes.c_void_p(optr),
                                     ctypes.c_void_p(gc.ptr) if with_counts else None, ctypes.c_void_p(sc.ptr), need, None))
    torch.cuda.synchronize()
    for g in (gl, go, gc, sc):
        assert g.guards_intact() == (True, True)
    raw = go.view.cpu().numpy()
    assert (raw[:4 * shift] == 0xFF).all() and (raw[4 * shift + nb:] == 0xFF).all(), "bytes next to the output were written"
    assert same_bits(lview.cpu().numpy().view(np.float32).reshape(n, V), label), "the label was written"
    counts = gc.view.cpu().numpy().view(np.int64).reshape(n, ncls + 1).copy()
    if not with_counts:
        assert (gc.view.cpu().numpy() == 0xFF).all()
    return oview.cpu().numpy().view(np.float32).reshape(n, V).copy(), counts


def _scale(seed, ncls):
    s = np.random.default_rng(seed).uniform(-2.0, 6.0, 9).astype(np.float32)
    s[ncls + 1:] = np.nan
    return s


def _check(lib, label, sp, ncls, radii=(0, 1, 2, 3), seed=0, shifts=(0, 1)):
    """Every radius, both modes, both placements against the oracle; returns the oracle's counts per radius."""
    label = np.ascontiguousarray(label, np.float32)
    cat = _oracle_categories(label, sp, ncls)
    scale = _scale(seed, ncls)
    seen = {}
    for r in radii:
        for mode in ("invfreq", "class"):
            want, want_counts = _oracle(cat, ncls, r, mode, scale)
            if mode == "invfreq" or r == radii[-1]:      # the categories do not depend on the mode: 'class' once per case
                w_np, c_np = make_weights_numpy(label, sp, ncls, WeightSpec(mode, r, [float(s) for s in scale[:ncls + 1]]))
                assert same_bits(w_np, want) and np.array_equal(c_np, want_counts), "the two host statements disagree"
            for shift in shifts:
                got, counts = _make(lib, label, sp, ncls, r, mode, scale, shift)
                assert np.array_equal(counts, want_counts), (sp, r, mode, shift, counts, want_counts)
                bad = np.flatnonzero(got.view(np.uint32).reshape(-1) != want.view(np.uint32).reshape(-1))
                assert bad.size == 0, (sp, r, mode, shift, bad.size, bad[:8], got.reshape(-1)[bad[:8]], want.reshape(-1)[bad[:8]])
        seen[r] = want_counts
    return seen


def _dense(rng, n, sp, ncls, holes=False):
    V = int(np.prod(sp))
    lab = rng.integers(0, ncls, (n, V)).astype(np.float32)
    lab += (rng.uniform(0, 0.9, (n, V)) * (lab > 0)).astype(np.float32)         # fractions truncate away
    if holes:
        u = rng.uniform(0, 1, (n, V))
        lab[u < 0.04] = np.nan
        lab[(u >= 0.04) & (u < 0.08)] = -1.0
        lab[(u >= 0.08) & (u < 0.12)] = float(ncls)
        lab[(u >= 0.12) & (u < 0.14)] = -0.5           # truncates to class 0
        lab[(u >= 0.14) & (u < 0.16)] = 1e9
        lab[(u >= 0.16) & (u < 0.17)] = -np.inf
    return lab


# ---- 1. constants ----------------------------------------------------------------------------------------------------------
def test_tile_constants(lib):
    """The scratch holds one byte per voxel (rounded up to 16), 64 bytes per tile and event, 64 bytes per event."""
    q = lib.ursn_make_weights_scratch_bytes

    def sp3(*e):
        return (ctypes.c_int32 * 3)(*(list(e) + [1])[:3])
    one = q(3, sp3(*TILE3), 1, 3, 1)
    assert one == 4096 + 64 + 64
    for ax in range(3):
        e = list(TILE3)
        e[ax] += 1
        assert q(3, sp3(*e), 1, 3, 1) == (int(np.prod(e)) + 15) // 16 * 16 + 2 * 64 + 64
    assert q(2, sp3(*TILE2), 1, 3, 1) == 4096 + 64 + 64
    for ax in range(2):
        e = list(TILE2)
        e[ax] += 1
        assert q(2, sp3(*e), 1, 3, 1) == (int(np.prod(e)) + 15) // 16 * 16 + 2 * 64 + 64
    assert int(np.prod(TILE3)) == int(np.prod(TILE2)) == SPAN


# ---- 2. labels -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [1, 3])
@pytest.mark.parametrize("sp", SHAPES, ids=_ids)
def test_dense_random_classes(lib, sp, n):
    ncls = (2, 3, 5, 8)[(SHAPES.index(sp) + n) % 4]
    seen = _check(lib, _dense(np.random.default_rng(100 + SHAPES.index(sp)), n, sp, ncls), sp, ncls, seed=n)
    if int(np.prod(sp)) >= 100 and ncls > 2:
        assert seen[1][:, ncls].min() > 0


@pytest.mark.parametrize("ncls", [2, 3, 5, 8])
def test_every_class_count_on_one_shape(lib, ncls):
    _check(lib, _dense(np.random.default_rng(ncls), 3, (5, 9, 23), ncls), (5, 9, 23), ncls, seed=ncls)


@pytest.mark.parametrize("sp", [(3, 5, 7), (17, 9, 70), (33, 65), tuple(t + 1 for t in TILE2)], ids=_ids)
def test_out_of_range_negative_and_nan_labels(lib, sp):
    """They get weight 0, are counted nowhere and make no boundary (the oracle says so; here also directly)."""
    ncls, n = 3, 3
    label = _dense(np.random.default_rng(7), n, sp, ncls, holes=True)
    seen = _check(lib, label, sp, ncls, seed=5)
    none = ~((label > -1) & (label < ncls))
    assert none.sum() > 0
    for r in range(4):
        assert np.array_equal(seen[r].sum(axis=1), (~none).sum(axis=1))
        w, _ = _make(lib, label, sp, ncls, r, "class", np.full(9, 3.0, np.float32))
        assert (w[none] == 0).all() and (w[~none] == 3.0).all()


@pytest.mark.parametrize("dims", [(16, 16, 16, 1), (64, 64, 1)], ids=["16x16x16", "64x64"])
def test_lartpc_sparse_events(lib, dims):
    sp = dims[:-1]
    ev = [sio.lartpc_sparse(dims, 3, e) for e in range(4)]
    label = np.stack([e[1] for e in ev])
    weight = np.stack([e[2] for e in ev])
    seen = _check(lib, label[:3], sp, 3, seed=1)
    seen3 = _check(lib, label[3:], sp, 3, seed=2)
    if dims[0] == 16:                                   # the issue's census of these toy events
        assert [int(seen3[r][0, 3]) for r in (1, 2, 3)] == [39, 54, 61]
        assert list(seen[1][:, 3]) == [0, 0, 0] and list(seen[2][:, 3]) == [19, 5, 29]
    else:
        assert seen3[1][0, 3] > 0 or seen[1][:, 3].max() > 0
    got, _ = _make(lib, label, sp, 3, 0, "invfreq", np.ones(9, np.float32))       # the producer thread's np.bincount weights
    assert same_bits(got, weight)


@pytest.mark.parametrize("sp", [(3, 5, 7), (16, 16, 16), (9, 9, 65), (64, 64), (5, 7)], ids=_ids)
def test_all_background_and_one_foreground_class(lib, sp):
    V = int(np.prod(sp))
    seen = _check(lib, np.zeros((3, V), np.float32), sp, 3)
    assert all(list(seen[r][e]) == [V, 0, 0, 0] for r in range(4) for e in range(3))
    lab = np.full((3, V), 2.0, np.float32)
    lab[1] = (np.random.default_rng(0).uniform(0, 1, V) < 0.5) * 2.0
    lab[2, ::3] = np.nan
    seen = _check(lib, lab, sp, 3)
    assert all(seen[r][:, 3].max() == 0 for r in range(4))          # a single foreground class meets nobody


# ---- 3. adversarial pairs --------------------------------------------------------------------------------------------------
def _pairs(sp, anchor, sign):
    """One event per (direction, distance 1..4): class 1 at `anchor`, class 2 at anchor + sign * distance * direction, where the
    directions are all non-zero 0/1 vectors (faces, edges, the corner).  Returns labels [n, V] and the distance of each event."""
    nd, V = len(sp), int(np.prod(sp))
    labels, dist = [], []
    for direction in itertools.product((0, 1), repeat=nd):
        if not any(direction):
            continue
        for k in range(1, 5):
            b = tuple(a + sign * k * s for a, s in zip(anchor, direction))
            assert all(0 <= x < e for x, e in zip(b, sp)), (sp, anchor, b)
            lab = np.zeros(sp, np.float32)
            lab[tuple(anchor)], lab[b] = 1.0, 2.0
            labels.append(lab.reshape(V))
            dist.append(k)
    return np.stack(labels), np.array(dist)


PAIR_CASES = [
    ("tile_seam_3d", (14, 14, 72), (7, 7, 63), 1),      # the anchor is the last voxel of tile (0, 0, 0): every pair crosses
    ("tile_seam_3d_back", (14, 14, 72), (8, 8, 64), -1),
    ("tile_seam_2d", (70, 70), (63, 63), 1),
    ("tile_seam_2d_back", (70, 70), (64, 64), -1),
    ("volume_corner_3d", (5, 6, 7), (0, 0, 0), 1),
    ("volume_far_corner_3d", (5, 6, 7), (4, 5, 6), -1),
    ("volume_far_corner_ragged", (9, 9, 66), (8, 8, 65), -1),
    ("volume_corner_2d", (6, 7), (0, 0), 1),
    ("volume_far_corner_2d", (66, 67), (65, 66), -1),
]


@pytest.mark.parametrize("name, sp, anchor, sign", PAIR_CASES, ids=[c[0] for c in PAIR_CASES])
def test_pairs_at_distance_r_and_r_plus_1(lib, name, sp, anchor, sign):
    label, dist = _pairs(sp, anchor, sign)
    seen = _check(lib, label, sp, 3, radii=(1, 2, 3), shifts=(0,))
    for r in (1, 2, 3):                                   # distance <= r: both voxels are boundary; r + 1 and beyond: neither
        assert np.array_equal(seen[r][:, 3], np.where(dist <= r, 2, 0)), (name, r)
        assert np.array_equal(seen[r][:, 1], np.where(dist <= r, 0, 1))


@pytest.mark.parametrize("sp", [(5, 6, 7), (3, 1, 5), (6, 7), (70, 5)], ids=_ids)
def test_flat_neighbours_that_are_not_spatial_neighbours(lib, sp):
    """Class 1 at the end of a row and class 2 at the start of the next; class 1 in the last voxel of an event and class 2 in
    the first of the next: flat-index neighbours, never a boundary once the row is longer than r + 1."""
    V, W = int(np.prod(sp)), sp[-1]
    label = np.zeros((3, V), np.float32)
    label[0, W - 1], label[0, W] = 1.0, 2.0               # row end / next row start
    label[0, V - 1], label[1, 0] = 1.0, 2.0               # event seam 0 | 1
    label[1, V - 1], label[2, 0] = 2.0, 1.0               # event seam 1 | 2
    seen = _check(lib, label, sp, 3, radii=(1, 2, 3))
    for r in (1, 2, 3):
        row_pair = 2 if (W - 1 <= r and (len(sp) == 2 or sp[-2] > 1)) else 0      # (.., y, W-1) and (.., y+1, 0) are W - 1 apart
        assert list(seen[r][:, 3]) == [row_pair, 0, 0], (sp, r, seen[r])


# ---- 4. state --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("sp", [(17, 9, 70), (65, 65)], ids=_ids)
def test_result_depends_only_on_the_arguments(lib, sp):
    ncls, n = 3, 3
    label = _dense(np.random.default_rng(11), n, sp, ncls, holes=True)
    scale = _scale(3, ncls)
    want, want_counts = make_weights_numpy(label, sp, ncls, WeightSpec("invfreq", 2, [float(s) for s in scale[:4]]))
    for fill in (0x00, 0xFF, "nan64", 0x7F):
        got, counts = _make(lib, label, sp, ncls, 2, "invfreq", scale, 1, fill=fill)
        assert same_bits(got, want) and np.array_equal(counts, want_counts), fill
    got, _ = _make(lib, label, sp, ncls, 2, "invfreq", scale, 1, with_counts=False)      # counts_out is optional
    assert same_bits(got, want)
    # one scratch buffer sized for a larger call: twice in a row, then the larger call in between
    big_sp = tuple(s + 9 for s in sp)
    big = _dense(np.random.default_rng(12), 4, big_sp, ncls)
    shared = _scratch(lib, big_sp, 4, ncls, 3, 0xFF)
    a = _make(lib, label, sp, ncls, 2, "invfreq", scale, 1, scratch=shared)
    b = _make(lib, label, sp, ncls, 2, "invfreq", scale, 1, scratch=shared)
    c = _make(lib, big, big_sp, ncls, 3, "invfreq", scale, 0, scratch=shared)
    d = _make(lib, label, sp, ncls, 2, "invfreq", scale, 1, scratch=shared)
    assert same_bits(c[0], make_weights_numpy(big, big_sp, ncls, WeightSpec("invfreq", 3, [float(s) for s in scale[:4]]))[0])
    for got, counts in (a, b, d):
        assert same_bits(got, want) and np.array_equal(counts, want_counts)


def test_many_tiles_per_event_and_many_events(lib):
    """More tiles than one pass of the reduce kernel's unrolled loop takes (8 x 64), and a batch wider than 3."""
    sp, ncls = (72, 40, 130), 5                        # 9 x 5 x 3 = 135 tiles ... and a 2-D volume of 23 x 24 = 552 tiles
    label = _dense(np.random.default_rng(21), 2, sp, ncls)
    want, want_counts = make_weights_numpy(label, sp, ncls, WeightSpec("invfreq", 1))
    got, counts = _make(lib, label, sp, ncls, 1, "invfreq", np.ones(9, np.float32))
    assert same_bits(got, want) and np.array_equal(counts, want_counts)
    sp = (1450, 1500)
    label = _dense(np.random.default_rng(22), 1, sp, 3)
    want, want_counts = make_weights_numpy(label, sp, 3, WeightSpec("invfreq", 1))
    got, counts = _make(lib, label, sp, 3, 1, "invfreq", np.ones(9, np.float32), 1)
    assert same_bits(got, want) and np.array_equal(counts, want_counts)
    sp = (3, 5, 7)
    label = _dense(np.random.default_rng(23), 37, sp, 3)
    want, want_counts = make_weights_numpy(label, sp, 3, WeightSpec("invfreq", 2))
    got, counts = _make(lib, label, sp, 3, 2, "invfreq", np.ones(9, np.float32), 1)
    assert same_bits(got, want) and np.array_equal(counts, want_counts)


# ---- 5. through the net ----------------------------------------------------------------------------------------------------
# the bf16 plan takes base filter counts that are multiples of 8 only
NET_CASES = [((16, 16, 16, 1), "fp32", 4, 2), ((32, 32, 1), "fp32", 4, 3), ((16, 16, 16, 1), "bf16", 8, 2), ((32, 32, 1), "bf16", 8, 3)]
NET_IDS = ["%s_%s" % ("x".join(str(d) for d in c[0][:-1]), c[1]) for c in NET_CASES]
SPEC = WeightSpec("invfreq", 2, [1.0, 2.0, 3.0, 5.0])
_inputs = {}


def _net_inputs(dims):
    if dims not in _inputs:
        ev = [sio.lartpc_sparse(dims, 3, e) for e in (2, 3)]
        data, label = (np.stack([e[j] for e in ev]) for j in range(2))
        w, counts = make_weights_numpy(label, dims[:-1], 3, SPEC)
        assert counts[:, 3].min() > 0                      # both events have boundary voxels at this radius
        _inputs[dims] = (data, label, w)
    return _inputs[dims]


def _build(dims, prec, base, ns):
    net = uresnet(dims=list(dims), num_class=3, base_num_outputs=base, num_strides=ns)
    net.construct(trainable=True, use_weight=True, learning_rate=1e-3, seed=7, precision=prec)
    return net


def _step(net, *args, **kw):
    net.zero_gradients(None)
    before = net.feed_stats['h2d_bytes'] if hasattr(net, 'feed_stats') else 0
    res, _ = net.accum_gradients(None, *args, **kw)
    return res, net.get_gradients(), net.feed_stats['h2d_bytes'] - before


def _same_step(a, b):
    return a[0] == b[0] and all(same_bits(a[1][k], b[1][k]) for k in b[1])


@pytest.mark.parametrize("dims, prec, base, ns", NET_CASES, ids=NET_IDS)
def test_step_with_made_weights_equals_step_on_host_weights(dims, prec, base, ns):
    data, label, w = _net_inputs(dims)
    sp = dims[:-1]
    n, V = label.shape
    ref_net, net = _build(dims, prec, base, ns), _build(dims, prec, base, ns)
    ref = _step(ref_net, data, label, w)
    assert np.isfinite(ref[0][1:]).all() and ref[0][1] > 0
    got = _step(net, data, label, make_weight=SPEC)
    assert _same_step(got, ref), (got[0], ref[0])
    assert same_bits(net.last_feed()['input_weight'].cpu().numpy(), w)
    assert ref[2] - got[2] == n * V * 4 and got[2] == 2 * n * V * 4          # the weight tensor no longer crosses PCIe
    # the symmetry runs over data and label only, the weights are made from the permuted label
    codes = symmetry.group("cube", sp)
    codes = [codes[len(codes) // 2 + 1], codes[-1]]
    got, want = _step(net, data, label, symmetry=codes, make_weight=SPEC), _step(ref_net, data, label, w, symmetry=codes)
    assert _same_step(got, want)
    assert same_bits(net.last_feed()['input_weight'].cpu().numpy(), symmetry.apply_batch(w, sp, codes))
    assert not _same_step(got, ref)
    # normalisation in place, in the made weights' own slot
    got, want = _step(net, data, label, make_weight=SPEC, normalize_weight=True), _step(ref_net, data, label, w, normalize_weight=True)
    assert _same_step(got, want)
    last = net.last_feed()['input_weight']
    assert same_bits(last.cpu().numpy(), ref_net.last_feed()['input_weight'].cpu().numpy())
    assert any(d is not None and d.data_ptr() == last.data_ptr() for d in net._feed_slots['made_weight'].dev)
    got, want = (_step(net, data, label, make_weight=SPEC, normalize_weight=True, symmetry=codes),
                 _step(ref_net, data, label, w, normalize_weight=True, symmetry=codes))
    assert _same_step(got, want)
    # run_test, and the stand-alone call
    want_test = ref_net.run_test(None, data, label, w)
    assert net.run_test(None, data, label, make_weight=SPEC) == want_test
    assert net.make_summary(None, data, label, make_weight=SPEC)['loss'] == want_test[0][0]
    assert (net.run_test(None, data, label, make_weight=SPEC, normalize_weight=True)
            == ref_net.run_test(None, data, label, w, normalize_weight=True))
    made, counts = net.make_weights(None, label, SPEC, as_numpy=True, with_counts=True)
    assert same_bits(made, w) and np.array_equal(counts, make_weights_numpy(label, sp, 3, SPEC)[1])
    assert same_bits(net.make_weights(None, label, SPEC).cpu().numpy(), w)
    # refusals leave the net usable
    with pytest.raises(ValueError):
        net.accum_gradients(None, data, label, w, make_weight=SPEC)
    assert _same_step(_step(net, data, label, make_weight=SPEC), ref)


@pytest.mark.parametrize("dims, prec, base, ns", NET_CASES, ids=NET_IDS)
def test_voxel_fed_step_with_made_weights(dims, prec, base, ns):
    data, label, w = _net_inputs(dims)
    n = data.shape[0]
    vb_w = VoxelBatch.concat([sio.dense_to_voxels(data[i], label[i], w[i]) for i in range(n)]).validate()
    vb = VoxelBatch.concat([sio.dense_to_voxels(data[i], label[i]) for i in range(n)]).validate()
    assert np.array_equal(vb.index, vb_w.index) and vb.weight is None      # a foreground voxel's weight never equals the background's
    ref_net, net = _build(dims, prec, base, ns), _build(dims, prec, base, ns)
    ref = _step(ref_net, data, label, w)

    def vstep(nn, batch, **kw):
        nn.zero_gradients(None)
        before = nn.feed_stats['h2d_bytes'] if hasattr(nn, 'feed_stats') else 0
        res, _ = nn.accum_gradients_voxels(None, batch, **kw)
        return res, nn.get_gradients(), nn.feed_stats['h2d_bytes'] - before
    with_lists = vstep(ref_net, vb_w)
    assert _same_step(with_lists, ref)
    got = vstep(net, vb, make_weight=SPEC)
    assert _same_step(got, ref)
    assert same_bits(net.last_feed()['input_weight'].cpu().numpy(), w)
    pad16 = lambda b: (b + 15) & ~15
    assert with_lists[2] - got[2] == pad16(vb_w.weight.nbytes) + pad16(vb_w.bg_weight.nbytes)      # the two lists stay at home
    codes = [5, 3]
    assert _same_step(vstep(net, vb, make_weight=SPEC, symmetry=codes, normalize_weight=True),
                      _step(ref_net, data, label, w, symmetry=codes, normalize_weight=True))
    assert net.run_test_voxels(None, vb, make_weight=SPEC) == ref_net.run_test(None, data, label, w)
    with pytest.raises(ValueError):
        net.accum_gradients_voxels(None, vb_w, make_weight=SPEC)


# ---- 6. driver -------------------------------------------------------------------------------------------------------------
def _driver_run(tmp_path, tag, extra, capsys, sparse=False):
    from uresnet_amd.ssnet_trainval import ssnet_trainval
    inp = tmp_path / "input.cfg"
    inp.write_text("Dims [32, 32, 32, 1]\nNumClass 3\nGenerator 'lartpc_sparse'\nNumEntries 64\n"
                   "Keys {'data': 'main_data', 'label': 'main_label', 'weight': 'main_weight'}\n")
    cfg = tmp_path / ("train_%s.cfg" % tag)
    cfg.write_text("NUM_CLASS 3\nBASE_NUM_FILTERS 4\nMAIN_INPUT_CONFIG '%s'\nTEST_INPUT_CONFIG '%s'\nLOGDIR '%s'\nSAVE_FILE ''\n"
                   "ITERATIONS 2\nMINIBATCH_SIZE 2\nNUM_MINIBATCHES 2\nTEST_BATCH_SIZE 2\nLEARNING_RATE 0.001\nTRAIN True\n"
                   "USE_WEIGHTS True\nREPORT_STEPS 1\nSUMMARY_STEPS 1\nCHECKPOINT_STEPS 0\nKEYWORD_DATA 'main_data'\n"
                   "KEYWORD_LABEL 'main_label'\nKEYWORD_WEIGHT 'main_weight'\nKEYWORD_TEST_DATA 'main_data'\n"
                   "KEYWORD_TEST_LABEL 'main_label'\nKEYWORD_TEST_WEIGHT 'main_weight'\nDEVICE_WEIGHT_NORM True\nSPARSE_IO %s\n%s"
                   % (inp, inp, tmp_path / ("log_" + tag), sparse, extra))
    t = ssnet_trainval()
    t.override_config(str(cfg))
    t.initialize()
    capsys.readouterr()
    rows, run = [], t._run_minibatches       # the per-minibatch metrics as the driver reads them, before '%6.6f' rounds them
    t._run_minibatches = lambda want_metrics: rows.append(run(want_metrics)) or rows[-1]
    for _ in range(2):
        t.train_step()
    printed = capsys.readouterr().out
    fed = t._net.last_feed()['input_weight'].cpu().numpy()
    h2d = t._net.feed_stats['h2d_bytes']
    log = (tmp_path / ("log_" + tag) / "train" / "scalars.jsonl").read_text() + (tmp_path / ("log_" + tag) / "test" / "scalars.jsonl").read_text()
    t.reset()
    return np.stack(rows), printed, log, fed, h2d


def test_driver_with_device_weights(tmp_path, capsys):
    """Two iterations (two minibatches each, report and summary every iteration, a test stream) of a 3-D synthetic training config
    with DEVICE_WEIGHTS 'invfreq', radius 0, against the same run on the IO's host weights.  At radius 0 the device makes the bits
    lartpc_sparse made with np.bincount; both runs normalise on the device (DEVICE_WEIGHT_NORM True, the host's float32 np.sum would
    differ from it), so every reported figure, the printed report and the summary logs are equal exactly."""
    strip = lambda s: re.sub(r"Mem \S+ @ \S+ \S+", "", s)
    host, printed_host, log_host, fed_host, h2d_host = _driver_run(tmp_path, "host", "", capsys)
    dev, printed_dev, log_dev, fed_dev, h2d_dev = _driver_run(tmp_path, "dev", "DEVICE_WEIGHTS 'invfreq'\n", capsys)
    assert host.shape == (2, 2, 3) and np.isfinite(host).all() and (host[:, :, 0] > 0).all()
    assert np.array_equal(dev, host)
    assert strip(printed_dev) == strip(printed_host) and printed_dev.count("Test set: loss=") == 2
    assert log_dev == log_host and log_dev.count("\n") == 4
    assert same_bits(fed_dev, fed_host)
    assert h2d_dev < h2d_host
    # the voxel feed: the weight lists are dropped from the batch, same figures
    vox, printed_vox, log_vox, fed_vox, _ = _driver_run(tmp_path, "vox", "DEVICE_WEIGHTS 'invfreq'\n", capsys, sparse=True)
    assert np.array_equal(vox, host) and strip(printed_vox) == strip(printed_host) and log_vox == log_host
    # a boundary category, scaled up, with augmentation: finite, and another loss
    aug, _, log_aug, fed_aug, _ = _driver_run(tmp_path, "r2", "DEVICE_WEIGHTS 'invfreq'\nWEIGHT_RADIUS 2\nWEIGHT_SCALE [1.0, 1.0, 1.0, 4.0]\n"
                                               "AUGMENT 'cube'\n", capsys)
    assert np.isfinite(aug).all() and (aug[:, :, 0] > 0).all() and not np.array_equal(aug, host)
    assert np.abs(fed_aug.sum(axis=1, dtype=np.float64) - 1.0).max() < 1e-5
    cls, _, _, fed_cls, _ = _driver_run(tmp_path, "cls", "DEVICE_WEIGHTS 'class'\nWEIGHT_SCALE [0.5, 2.0, 3.0, 1.0]\n", capsys)
    assert np.isfinite(cls).all() and (cls[:, :, 0] > 0).all()
