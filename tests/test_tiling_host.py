"""Tiled inference and crop training, host side (no GPU): the appended symbols under an unchanged ABI 9, the scratch query, every
argument refusal of ursn_crop_count / ursn_crop_write / ursn_scores_scatter (include/uresnet_hip.h), the box grid, the numpy
statement of the device passes (uresnet_amd.tiling.crop_numpy / stitch_numpy) against a brute-force dense crop, the training
crops' determinism, the config keys and the keywords' refusals.  Every library call below is refused on its arguments before any
device access, so the fake pointers are never dereferenced."""
import ctypes
import inspect
import io
import os
from contextlib import redirect_stdout

import numpy as np
import pytest

import uresnet_amd  # noqa: F401
from uresnet_amd import _lib, ssnet_config, tiling, uresnet
from uresnet_amd import synthetic_io as sio
from uresnet_amd.ssnet import VoxelBatch

FAKE = 0x10000
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
WAVES, VOX_PER_GROUP, MAX_GROUPS = 4, 4096, 32     # csrc/tiling.hip: parts per workgroup, slab voxels per workgroup, its ceiling
GRIDS = [((40, 24, 56), (16, 16, 16), 4), ((48, 80), (32, 32), 8), ((64, 32, 48), (16, 16, 16), 0)]


def _p(a):
    return ctypes.c_void_p(a)


def _sp(*ext):
    return (ctypes.c_int32 * 3)(*(list(ext) + [1] * (3 - len(ext))))


def test_symbols_appended_under_abi_9(lib):
    assert _lib.ABI_VERSION == 9 and lib.ursn_abi_version() == 9
    with open(os.path.join(ROOT, "include", "uresnet_hip.h")) as f:
        hdr = f.read()
    for name in ("ursn_crop_count", "ursn_crop_scratch_bytes", "ursn_crop_write", "ursn_scores_scatter"):
        assert name in _lib.EXPORTS and hasattr(lib, name) and (name + "(") in hdr, name
    assert "#define URSN_ABI_VERSION 9" in hdr


def _want_scratch(big, tile, boxes):
    slab = min(tile[0], big[0]) * int(np.prod(big[1:]))
    groups = min(max(-(-slab // VOX_PER_GROUP), 1), MAX_GROUPS)
    return boxes * (3 + 2 * groups * WAVES) * 4


def test_scratch_query(lib):
    q = lib.ursn_crop_scratch_bytes
    for big, tile in (((40, 24, 56), (16, 16, 16)), ((48, 80), (32, 32)), ((8, 8, 8), (4, 4, 4)), ((768, 768, 768), (192, 192, 192)),
                      ((16, 16, 16), (16, 16, 16)), ((4, 4), (32, 32)), ((1, 4096), (1, 1)), ((1, 4097), (1, 1))):
        for boxes in (1, 3, 48, 1 << 20):
            assert q(len(big), _sp(*big), _sp(*tile), boxes) == _want_scratch(big, tile, boxes) > 0, (big, tile, boxes)
    bad = [(1, (4, 4, 4), (2, 2, 2), 1), (4, (4, 4, 4), (2, 2, 2), 1), (3, (0, 4, 4), (2, 2, 2), 1), (3, (4, 4, -1), (2, 2, 2), 1),
           (3, (4, 4, 4), (2, 0, 2), 1), (2, (4, 4), (0, 2), 1), (3, (2048, 1024, 1024), (2, 2, 2), 1),
           (3, (4, 4, 4), (2048, 1024, 1024), 1), (2, (65536, 32768), (2, 2), 1), (3, (4, 4, 4), (2, 2, 2), 0),
           (3, (4, 4, 4), (2, 2, 2), -1), (3, (4, 4, 4), (2, 2, 2), (1 << 20) + 1)]
    for nd, big, tile, boxes in bad:
        assert q(nd, _sp(*big), _sp(*tile), boxes) == 0, (nd, big, tile, boxes)
    assert q(3, None, _sp(2, 2, 2), 1) == 0 and q(3, _sp(4, 4, 4), None, 1) == 0
    assert q(3, _sp(2047, 1024, 1024), _sp(2, 2, 2), 1) > 0                      # just below 2^31 voxels


# ---- refusals ------------------------------------------------------------------------------------------------------------------
def _desc(ndim=3, big=(8, 8, 8), tile=(4, 4, 4), n=2, boxes=3, m_total=10, offsets=FAKE, index=FAKE + 0x1000, value=FAKE + 0x2000,
          label=FAKE + 0x3000, weight=FAKE + 0x4000, bg_weight=FAKE + 0x5000, box_event=FAKE + 0x6000, box_origin=FAKE + 0x7000,
          core_lo=FAKE + 0x8000, core_hi=FAKE + 0x9000):
    d = _lib.ursn_crop_desc()
    d.ndim, d.n, d.boxes, d.m_total = ndim, n, boxes, m_total
    for i in range(3):
        d.big[i] = big[i] if i < len(big) else 0
        d.tile[i] = tile[i] if i < len(tile) else 0
    for name in ("offsets", "index", "value", "label", "weight", "bg_weight", "box_event", "box_origin", "core_lo", "core_hi"):
        setattr(d, name, locals()[name])
    return d


def _out(offsets=FAKE + 0x10000, index=FAKE + 0x11000, value=FAKE + 0x12000, label=FAKE + 0x13000, weight=FAKE + 0x14000,
         bg_weight=FAKE + 0x15000, src=FAKE + 0x16000, owned=FAKE + 0x17001, cap=10):
    o = _lib.ursn_crop_out()
    for name in ("offsets", "index", "value", "label", "weight", "bg_weight", "src", "owned"):
        setattr(o, name, locals()[name])
    o.cap = cap
    return o


SCRATCH = FAKE + 0x20000


def _count_refused(lib, text, desc=None, count=FAKE + 0x30000, owned=FAKE + 0x31000, scratch=SCRATCH, sbytes=1 << 20, **kw):
    d = _desc(**kw) if desc is None else desc
    rc = lib.ursn_crop_count(ctypes.byref(d) if d != "null" else None, _p(count), _p(owned), _p(scratch), sbytes, None)
    msg = lib.ursn_last_error()
    assert rc != 0 and text in msg, (rc, msg)


def _write_refused(lib, text, desc=None, out=None, scratch=SCRATCH, sbytes=1 << 20, okw=None, **kw):
    d = _desc(**kw) if desc is None else desc
    o = _out(**(okw or {})) if out is None else out
    rc = lib.ursn_crop_write(ctypes.byref(d) if d != "null" else None, ctypes.byref(o) if o != "null" else None, _p(scratch),
                             sbytes, None)
    msg = lib.ursn_last_error()
    assert rc != 0 and text in msg, (rc, msg)


def _shared_refusals(refused, who):
    """The checks both crop entry points make on the descriptor and the scratch, in the order the library makes them."""
    refused(who + b": null desc", desc="null")
    refused(who + b": ndim = 1, must be 2 or 3", ndim=1)
    refused(who + b": ndim = 4, must be 2 or 3", ndim=4)
    refused(who + b": big[0] = 0 < 1", big=(0, 8, 8))
    refused(who + b": big[2] = -3 < 1", big=(8, 8, -3))
    refused(who + b": tile[1] = 0 < 1", tile=(4, 0, 4))
    refused(who + b": tile[1] = -1 < 1", ndim=2, tile=(4, -1))
    refused(who + b": prod(big) >= 2^31", big=(2048, 1024, 1024))
    refused(who + b": prod(big) >= 2^31", ndim=2, big=(65536, 32768))
    refused(who + b": prod(tile) >= 2^31", tile=(2048, 1024, 1024))
    refused(who + b": n = 0 outside [1, 65535]", n=0)
    refused(who + b": n = -2 outside [1, 65535]", n=-2)
    refused(who + b": n = 65536 outside [1, 65535]", n=65536)
    refused(who + b": boxes = 0 outside [1, 1048576]", boxes=0)
    refused(who + b": boxes = -1 outside [1, 1048576]", boxes=-1)
    refused(who + b": boxes = 1048577 outside [1, 1048576]", boxes=(1 << 20) + 1)
    refused(who + b": m_total = -1 outside [0, 2^31)", m_total=-1)
    refused(who + b": m_total = 2147483648 outside [0, 2^31)", m_total=2 ** 31)
    refused(who + b": null offsets / index", offsets=None)
    refused(who + b": null offsets / index", index=None)
    refused(who + b": null box_event / box_origin", box_event=None)
    refused(who + b": null box_event / box_origin", box_origin=None)
    refused(who + b": core_lo and core_hi must come together", core_lo=None)
    refused(who + b": core_lo and core_hi must come together", core_hi=None)
    refused(who + b": null scratch", scratch=None)
    refused(who + b": offsets / scratch must be 8-byte aligned", offsets=FAKE + 4)
    refused(who + b": offsets / scratch must be 8-byte aligned", scratch=SCRATCH + 4)
    for name in ("index", "value", "label", "weight", "bg_weight", "box_event", "box_origin", "core_lo", "core_hi"):
        refused(who + b": index / value / label / weight / bg_weight / box arrays must be 4-byte aligned",
                **{name: FAKE + 0xA002})
    need = _want_scratch((8, 8, 8), (4, 4, 4), 3)
    refused(who + b": scratch of %d bytes is too small, %d needed" % (need - 1, need), sbytes=need - 1)
    refused(who + b": scratch of 0 bytes is too small", sbytes=0)


def test_crop_count_refusals(lib):
    _shared_refusals(lambda text, **kw: _count_refused(lib, text, **kw), b"crop_count")
    _count_refused(lib, b"crop_count: null count_out / owned_out", count=None)
    _count_refused(lib, b"crop_count: null count_out / owned_out", owned=None)
    _count_refused(lib, b"crop_count: count_out / owned_out must be 8-byte aligned", count=FAKE + 0x30004)
    _count_refused(lib, b"crop_count: count_out / owned_out must be 8-byte aligned", owned=FAKE + 0x31004)


def test_crop_write_refusals(lib):
    _shared_refusals(lambda text, **kw: _write_refused(lib, text, **kw), b"crop_write")
    _write_refused(lib, b"crop_write: null out / out->offsets / out->index", out="null")
    _write_refused(lib, b"crop_write: null out / out->offsets / out->index", okw=dict(offsets=None))
    _write_refused(lib, b"crop_write: null out / out->offsets / out->index", okw=dict(index=None))
    _write_refused(lib, b"crop_write: cap = -1 < 0", okw=dict(cap=-1))
    _write_refused(lib, b"crop_write: value output without a value list", value=None)
    _write_refused(lib, b"crop_write: label output without a label list", label=None)
    _write_refused(lib, b"crop_write: weight output without a weight list", weight=None)
    _write_refused(lib, b"crop_write: weight and bg_weight outputs must come together", okw=dict(weight=None))
    _write_refused(lib, b"crop_write: weight and bg_weight outputs must come together", okw=dict(bg_weight=None))
    _write_refused(lib, b"crop_write: bg_weight output without a bg_weight array", bg_weight=None)
    _write_refused(lib, b"crop_write: out->offsets must be 8-byte aligned", okw=dict(offsets=FAKE + 0x10004))
    for name in ("index", "value", "label", "weight", "bg_weight", "src"):
        _write_refused(lib, b"crop_write: out->index / value / label / weight / bg_weight / src must be 4-byte aligned",
                       okw={name: FAKE + 0x1A002})


def test_scores_scatter_refusals(lib):
    def refused(text, src=FAKE, owned=FAKE + 0x1001, m=5, ncls=3, scores=FAKE + 0x2000, pred=FAKE + 0x3001, ana=FAKE + 0x4001,
                scores_out=FAKE + 0x5000, pred_out=FAKE + 0x6001, ana_out=FAKE + 0x7001, rows_out=9):
        rc = lib.ursn_scores_scatter(_p(src), _p(owned), m, ncls, _p(scores), _p(pred), _p(ana), _p(scores_out), _p(pred_out),
                                     _p(ana_out), rows_out, None)
        msg = lib.ursn_last_error()
        assert rc != 0 and text in msg, (rc, msg)
    refused(b"scores_scatter: null src / owned", src=None)
    refused(b"scores_scatter: null src / owned", owned=None)
    refused(b"scores_scatter: m = -1 outside [0, 2^31)", m=-1)
    refused(b"scores_scatter: m = 2147483648 outside [0, 2^31)", m=2 ** 31)
    refused(b"scores_scatter: rows_out = -1 outside [0, 2^31)", rows_out=-1)
    refused(b"scores_scatter: rows_out = 2147483648 outside [0, 2^31)", rows_out=2 ** 31)
    refused(b"scores_scatter: num_class 0 not in [1,8]", ncls=0)
    refused(b"scores_scatter: num_class 9 not in [1,8]", ncls=9)
    refused(b"scores_scatter: all three outputs are null", scores_out=None, pred_out=None, ana_out=None)
    refused(b"scores_scatter: scores and scores_out must come together", scores=None)
    refused(b"scores_scatter: scores and scores_out must come together", scores_out=None)
    refused(b"scores_scatter: pred and pred_out must come together", pred=None)
    refused(b"scores_scatter: pred and pred_out must come together", pred_out=None)
    refused(b"scores_scatter: ana and ana_out must come together", ana=None)
    refused(b"scores_scatter: ana and ana_out must come together", ana_out=None)
    for name, at in (("src", FAKE + 2), ("scores", FAKE + 0x2002), ("scores_out", FAKE + 0x5001)):
        refused(b"scores_scatter: src / scores / scores_out must be 4-byte aligned", **{name: at})


# ---- the grid ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("big,tile,halo", GRIDS + [((16, 16, 16), (16, 16, 16), 4), ((10, 40), (32, 32), 8), ((33, 33), (32, 32), 0)],
                         ids=lambda v: "x".join(map(str, v)) if isinstance(v, tuple) else str(v))
def test_grid_cores_partition_the_volume_inside_their_boxes(big, tile, halo):
    boxes = tiling.grid(big, tile, halo)
    nd, T = len(big), np.array(tile)
    stride = T - 2 * halo
    assert boxes.ndim == nd and (boxes.event == 0).all()
    owners = np.zeros(big, np.int64)
    for b in range(len(boxes)):
        o, lo, hi = boxes.origin[b], boxes.core_lo[b], boxes.core_hi[b]
        assert (lo >= 0).all() and (hi <= T).all() and (lo < hi).all(), b            # the core lies inside the box, and is not empty
        assert (o >= 0).all() and ((o + T <= np.array(big)) | (o == 0)).all(), b      # a box overhangs only where S < T
        owners[tuple(slice(int(a), int(c)) for a, c in zip(o + lo, o + hi))] += 1
    assert (owners == 1).all()
    for ax, (S, Tt) in enumerate(zip(big, tile)):
        got = sorted(set(int(x) for x in boxes.origin[:, ax]))
        want = [0] if S <= Tt else sorted(set(list(range(0, S - Tt, int(stride[ax]))) + [S - Tt]))
        assert got == want, (ax, got, want)
    # per event the same boxes again, event-major
    three = tiling.grid(big, tile, halo, n=3)
    per = len(boxes)
    assert len(three) == 3 * per and list(three.event) == [e for e in range(3) for _ in range(per)]
    for e in range(3):
        assert np.array_equal(three.origin[e * per:(e + 1) * per], boxes.origin)
        assert np.array_equal(three.core_lo[e * per:(e + 1) * per], boxes.core_lo)


def test_grid_shapes_of_the_issue():
    assert len(tiling.grid((40, 24, 56), (16, 16, 16), 4)) == 48 and len(tiling.grid((48, 80), (32, 32), 8)) == 8
    origins, lo, hi = tiling.axis_grid(40, 16, 4)         # S - T = 24 is a multiple of the stride 8: no doubled origin
    assert origins == [0, 8, 16, 24] and lo == [0, 12, 20, 28] and hi == [12, 20, 28, 40]
    origins, lo, hi = tiling.axis_grid(56, 16, 4)         # the last origin, 40, is the stride's next step as well
    assert origins == [0, 8, 16, 24, 32, 40]
    origins, lo, hi = tiling.axis_grid(80, 32, 8)         # S - T = 48 = 3 strides
    assert origins == [0, 16, 32, 48] and lo == [0, 24, 40, 56] and hi == [24, 40, 56, 80]
    origins, lo, hi = tiling.axis_grid(50, 32, 8)         # S - T = 18 is NOT a multiple of the stride 16: 0, 16, then 18
    assert origins == [0, 16, 18] and lo == [0, 24, 33] and hi == [24, 33, 50]
    assert tiling.axis_grid(24, 32, 8) == ([0], [0], [24]) and tiling.axis_grid(32, 32, 8) == ([0], [0], [32])
    for kw in (dict(halo=-1), dict(halo=8), dict(halo=9)):
        with pytest.raises(ValueError):
            tiling.grid((40, 40), (16, 16), **kw)
    for big, tile in (((4, 4), (2, 2, 2)), ((4,), (2,)), ((0, 4), (2, 2)), ((4, 4), (2, 0)), ((65536, 32768), (2, 2))):
        with pytest.raises(ValueError):
            tiling.grid(big, tile, 0)


# ---- crop_numpy / stitch_numpy -------------------------------------------------------------------------------------------------
def _large_batch(big, entries=(0, 1, 2)):
    dims = list(big) + [1]
    return VoxelBatch.concat([sio.dense_to_voxels(*sio.lartpc_sparse(dims, 3, e)) for e in entries])


def _brute_force_crop(vb, big, tile, boxes):
    """voxels_to_dense at the large shape, a padded slice per box, dense_to_voxels: no index arithmetic shared with crop_numpy."""
    data, label, weight = sio.voxels_to_dense(vb)
    listed = np.zeros((vb.n, vb.voxels), bool)
    pos = np.full((vb.n, vb.voxels), -1, np.int64)
    for e in range(vb.n):
        a, b = int(vb.offsets[e]), int(vb.offsets[e + 1])
        listed[e, vb.index[a:b]] = True
        pos[e, vb.index[a:b]] = np.arange(a, b)
    pad = [(t, t) for t in tile]
    out = []
    for b in range(len(boxes)):
        e = int(boxes.event[b])
        sl = tuple(slice(int(o) + t, int(o) + 2 * t) for o, t in zip(boxes.origin[b], tile))
        cut = lambda a, fill: np.pad(a[e].reshape(big), pad, constant_values=fill)[sl].reshape(-1)
        keep = np.flatnonzero(cut(listed, False))
        out.append((keep, cut(data, 0)[keep], cut(label, 0)[keep], cut(weight, 0)[keep], cut(pos, -1)[keep]))
    return out


@pytest.mark.parametrize("big,tile,halo", GRIDS[:2], ids=["3d", "2d"])
def test_crop_numpy_is_the_dense_crop(big, tile, halo):
    vb = _large_batch(big)
    hand = [[-3] * len(big), [s - 5 for s in big], [0] * len(big), [0] * len(big), [s + 1 for s in big]]   # overhangs, a duplicate, an empty box
    grid = tiling.grid(big, tile, halo, n=vb.n)
    boxes = tiling.Boxes(np.concatenate([grid.event, [1, 2, 0, 0, 1]]), np.concatenate([grid.origin, hand]),
                         np.concatenate([grid.core_lo, np.zeros((5, len(big)), int)]),
                         np.concatenate([grid.core_hi, np.tile(tile, (5, 1))]))
    crop, src, owned, count, owned_count = tiling.crop_numpy(vb, big, tile, boxes)
    crop.validate()
    assert crop.n == len(boxes) and crop.voxels == int(np.prod(tile)) and np.array_equal(np.diff(crop.offsets), count)
    want = _brute_force_crop(vb, big, tile, boxes)
    assert count[-1] == 0 and count[-2] == count[-3] > 0
    for b, (index, value, label, weight, pos) in enumerate(want):
        a, z = int(crop.offsets[b]), int(crop.offsets[b + 1])
        assert np.array_equal(crop.index[a:z], index), b
        assert np.array_equal(crop.value[a:z], value) and np.array_equal(crop.label[a:z], label), b
        assert np.array_equal(crop.weight[a:z], weight) and np.array_equal(src[a:z], pos), b
        assert crop.bg_weight[b] == vb.bg_weight[boxes.event[b]]
        local = np.stack(np.unravel_index(index, tile), axis=1) if index.size else np.zeros((0, len(big)), np.int64)
        core = np.all((local >= boxes.core_lo[b]) & (local < boxes.core_hi[b]), axis=1)
        assert np.array_equal(owned[a:z], core.astype(np.uint8)) and owned_count[b] == core.sum(), b
    # the grid's cores partition the volume: every list entry is owned exactly once among the grid's boxes
    m_grid = int(crop.offsets[len(grid)])
    assert np.array_equal(np.sort(src[:m_grid][owned[:m_grid] == 1]), np.arange(int(vb.offsets[-1])))


def test_crop_numpy_optional_roles_and_foreign_events():
    big, tile = (8, 8, 8), (4, 4, 4)
    full = VoxelBatch([0, 512], np.arange(512), np.arange(512) + 1.0, voxels=512)       # every voxel listed, no label, no weight
    boxes = tiling.Boxes([0, 1, -1, 0], [[0, 0, 0], [0, 0, 0], [0, 0, 0], [4, 4, 4]])
    crop, src, owned, count, owned_count = tiling.crop_numpy(full, big, tile, boxes)
    assert list(count) == [64, 0, 0, 64] and list(owned_count) == [64, 0, 0, 64] and (owned == 1).all()
    assert crop.label is None and crop.weight is None and crop.bg_weight is None
    assert np.array_equal(crop.index[:64], np.arange(64)) and np.array_equal(crop.index[64:], np.arange(64))
    assert np.array_equal(src[64:], np.ravel_multi_index(np.meshgrid(*[np.arange(4, 8)] * 3, indexing="ij"), big).reshape(-1))


@pytest.mark.parametrize("big,tile,halo", GRIDS, ids=["3d", "2d", "halo0"])
def test_crop_then_stitch_is_the_identity(big, tile, halo):
    vb = _large_batch(big)
    M = int(vb.offsets[-1])
    tag = np.arange(M, dtype=np.float32) * 3 + 1                # a tagged list: the value names the entry
    tagged = VoxelBatch(vb.offsets, vb.index, tag, voxels=vb.voxels)
    boxes = tiling.grid(big, tile, halo, n=vb.n)
    out = {"scores": np.full((M, 2), -1, np.float32), "pred": np.full(M, 255, np.uint8)}
    written = np.zeros(M, np.int64)
    for first in range(0, len(boxes), 5):                      # batches of 5 boxes, as the tiled inference would run them
        crop, src, owned, _, _ = tiling.crop_numpy(tagged, big, tile, boxes.select(slice(first, first + 5)))
        rows = np.stack([crop.value, crop.value + 0.5], axis=1)
        tiling.stitch_numpy(out, src, owned, scores=rows, pred=(crop.value % 251).astype(np.uint8), ana=None)
        np.add.at(written, src[owned == 1], 1)
    assert (written == 1).all()
    assert np.array_equal(out["scores"], np.stack([tag, tag + 0.5], axis=1)) and np.array_equal(out["pred"], (tag % 251).astype(np.uint8))
    # rows that are not owned leave the output alone
    keep = {"scores": np.full((M, 2), -1, np.float32)}
    crop, src, owned, _, _ = tiling.crop_numpy(tagged, big, tile, boxes)
    tiling.stitch_numpy(keep, src, np.zeros_like(owned), scores=np.zeros((src.size, 2), np.float32))
    assert (keep["scores"] == -1).all()


def test_random_boxes_are_a_pure_function_of_their_arguments():
    big, tile = (40, 24, 56), (16, 16, 16)
    vb = _large_batch(big)
    empty = VoxelBatch.concat([vb, VoxelBatch([0, 0], [], [], [], [], [0.5], vb.voxels)])
    a, b = tiling.random_boxes(7, empty, big, tile), tiling.random_boxes(7, empty, big, tile)
    assert np.array_equal(a.origin, b.origin) and list(a.event) == [0, 1, 2, 3] and a.core_lo is None and a.core_hi is None
    assert (a.origin[3] == 0).all()                                                   # no voxels: origin 0
    assert (a.origin >= 0).all() and (a.origin + np.array(tile) <= np.array(big)).all()
    c = tiling.random_boxes(8, empty, big, tile)
    assert not np.array_equal(a.origin[:3], c.origin[:3])
    assert np.array_equal(tiling.random_boxes([7, 2, 0, 1], empty, big, tile).origin, tiling.random_boxes((7, 2, 0, 1), empty, big, tile).origin)
    assert not np.array_equal(tiling.random_boxes([7, 2, 0, 1], empty, big, tile).origin, tiling.random_boxes([7, 3, 0, 1], empty, big, tile).origin)
    # an event's box does not depend on its batch-mates' lists, only on its position in the batch
    alone = tiling.random_boxes(7, VoxelBatch.concat([sio.dense_to_voxels(*sio.lartpc_sparse(list(big) + [1], 3, 0))]), big, tile)
    assert np.array_equal(alone.origin[0], a.origin[0])
    # every crop holds the voxel it was centred on, so no crop of a non-empty event is empty
    _, _, _, count, _ = tiling.crop_numpy(empty, big, tile, a)
    assert (count[:3] > 0).all() and count[3] == 0
    small = tiling.random_boxes(1, _large_batch((10, 40), (0,)), (10, 40), (32, 32))   # narrower than the tile along axis 0
    assert small.origin[0, 0] == 0 and 0 <= small.origin[0, 1] <= 8


# ---- config keys, the synthetic IO and the keywords ----------------------------------------------------------------------------
def test_config_keys_default_off_and_validated(tmp_path):
    c = ssnet_config()
    assert (c.ANA_TILE, c.ANA_TILE_HALO, c.ANA_TILE_BATCH, c.TRAIN_CROP, c.CROP_SEED) == ([], 0, 4, [], 0)
    out = io.StringIO()
    with redirect_stdout(out):
        c.dump()
    for key in ("ANA_TILE", "ANA_TILE_HALO", "ANA_TILE_BATCH", "TRAIN_CROP", "CROP_SEED"):
        assert any(line.startswith(key + ".") for line in out.getvalue().split("\n")), key
    p = tmp_path / "a.cfg"
    p.write_text("ANA_TILE [40, 24, 56]\nANA_TILE_HALO 4\nANA_TILE_BATCH 3\nTRAIN_CROP [48, 80]\nCROP_SEED 11\n")
    with redirect_stdout(io.StringIO()):
        c.override(str(p))
    assert (c.ANA_TILE, c.ANA_TILE_HALO, c.ANA_TILE_BATCH, c.TRAIN_CROP, c.CROP_SEED) == ([40, 24, 56], 4, 3, [48, 80], 11)
    assert ssnet_config().ANA_TILE == [] and ssnet_config().TRAIN_CROP == []
    for text in ("ANA_TILE (40, 24, 56)\n", "ANA_TILE [40]\n", "ANA_TILE [40, 24, 56, 8]\n", "ANA_TILE [40, 0, 56]\n",
                 "ANA_TILE [40.0, 24, 56]\n", "TRAIN_CROP [48, -80]\n", "TRAIN_CROP 48\n", "TRAIN_CROP ['a', 'b']\n",
                 "ANA_TILE_HALO -1\n", "ANA_TILE_HALO 2.0\n", "ANA_TILE_BATCH 0\n", "ANA_TILE_BATCH 1.5\n", "CROP_SEED 'x'\n"):
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


def test_driver_refuses_the_keys_without_their_companions(tmp_path):
    """Every refusal comes before a stream is opened or a device is touched."""
    for text, word in (("TRAIN False\nANA_TILE [40, 24, 56]\n", "SPARSE_IO"), ("TRAIN_CROP [40, 24, 56]\n", "SPARSE_IO"),
                       ("TRAIN False\nSPARSE_IO True\nANA_TILE [40, 24, 56]\nANA_CSV '%s'\n" % (tmp_path / "a.csv"), "ANA_CSV"),
                       ("TRAIN False\nSPARSE_IO True\nANA_TILE [40, 24, 56]\nANA_TTA [0, 1]\n", "ANA_TTA")):
        with pytest.raises(ValueError, match=word):
            _driver(tmp_path, text).initialize()
    # a key of the other mode is ignored: TRAIN_CROP while analysing, ANA_TILE while training, need nothing
    assert _driver(tmp_path, "TRAIN False\nTRAIN_CROP [40, 24, 56]\n")._big_shape() == []
    assert _driver(tmp_path, "ANA_TILE [40, 24, 56]\n")._big_shape() == []
    assert _driver(tmp_path, "SPARSE_IO True\nTRAIN_CROP [40, 24, 56]\n")._big_shape() == [40, 24, 56]


def test_synthetic_io_produces_large_events():
    cfg = {"Dims": [16, 16, 16, 1], "NumClass": 3, "Generator": "lartpc_sparse", "NumEntries": 8}
    src = sio.synthetic_threadio()
    src.configure({"filler_cfg": cfg})
    src.produce_voxels()
    src.produce_large([40, 24, 56])
    src.start_manager(2)
    src.next()
    vb = src.fetch_voxels()
    assert src.fetch_data("data").dim() == [2, 16, 16, 16, 1] and src.fetch_entries() == [0, 1]
    want = _large_batch((40, 24, 56), (0, 1))
    assert vb.voxels == 40 * 24 * 56 and np.array_equal(vb.offsets, want.offsets) and np.array_equal(vb.index, want.index)
    assert np.array_equal(vb.value, want.value) and np.array_equal(vb.weight, want.weight)
    src.reset()
    for bad in ([40, 24], [40, 24, 0]):
        other = sio.synthetic_threadio()
        other.configure({"filler_cfg": cfg})
        with pytest.raises(ValueError):
            other.produce_large(bad)


def test_run_methods_take_crop():
    from uresnet_amd.ssnet import ssnet_base
    for name in ("accum_gradients_voxels", "run_test_voxels"):
        assert inspect.signature(getattr(ssnet_base, name)).parameters["crop"].default is None, name
    assert list(inspect.signature(ssnet_base.inference_tiled_voxel_scores).parameters) == ["self", "sess", "big_batch", "big", "halo",
                                                                                           "tile_batch", "want"]
    assert list(inspect.signature(ssnet_base.upload_voxels).parameters) == ["self", "vb", "big"]
    doc = ssnet_base.inference_tiled_voxel_scores.__doc__
    assert "receptive field" in doc and "set_bn_mode('moving')" in doc


def test_crop_keyword_refusals_come_before_any_device_use():
    """construct(allocate=False) never touches a device: whatever came after the refusal would raise something else."""
    net = uresnet(dims=[16, 16, 16, 1], num_class=3, base_num_outputs=4, num_strides=2)
    net.construct(trainable=True, use_weight=True, learning_rate=1e-3, allocate=False)
    vb = VoxelBatch([0, 1], [5], [2.0], [1.0], [0.5], [0.25], 16 ** 3)
    boxes = tiling.Boxes([0], [[0, 0, 0]])
    for crop in ((vb, boxes), (None, boxes), "boxes", (vb,)):
        for call in (lambda: net.accum_gradients_voxels(None, None, crop=crop), lambda: net.run_test_voxels(None, None, crop=crop)):
            with pytest.raises(ValueError, match="crop"):
                call()
    with pytest.raises(ValueError, match="voxels must be None"):
        net.accum_gradients_voxels(None, vb, crop=(vb, boxes))
    for call in (lambda: net.inference_tiled_voxel_scores(None, vb, (16, 16, 16), want=()),
                 lambda: net.inference_tiled_voxel_scores(None, vb, (16, 16, 16), want=("softmax",)),
                 lambda: net.inference_tiled_voxel_scores(None, vb, (16, 16, 16), tile_batch=0)):
        with pytest.raises(ValueError):
            call()
    two = uresnet(dims=[16, 16, 16, 2], num_class=3, base_num_outputs=4, num_strides=2)
    two.construct(trainable=False, use_weight=False, allocate=False)
    with pytest.raises(ValueError, match="one value per voxel"):
        two.inference_tiled_voxel_scores(None, vb, (16, 16, 16))
