"""Tiled inference and crop training on the device (include/uresnet_hip.h; csrc/tiling.hip): ursn_crop_count / ursn_crop_write /
ursn_scores_scatter against their numpy statement (uresnet_amd.tiling.crop_numpy / stitch_numpy), ssnet_base's
inference_tiled_voxel_scores and crop= against the same boxes cropped on the host and fed through the calls that existed before,
and one driver run each with ANA_TILE and TRAIN_CROP.

Every comparison is on bit patterns (the one exception, a batch of another size in moving mode, says so), every op-level output
holds exactly the bytes it may be written between canary guards and is filled with 0xFF before the call."""
import ctypes
import io
from contextlib import redirect_stdout

import numpy as np
import pytest

import _far_corner as far
from _abi import _Guarded, same_bits
from _net import max_rel
from uresnet_amd import _lib, tiling, uresnet
from uresnet_amd import synthetic_io as sio
from uresnet_amd.ssnet import VoxelBatch
from uresnet_amd.weights import WeightSpec

pytestmark = pytest.mark.gpu

GUARD = 1024
STEP = 256            # list entries a crop workgroup takes per iteration (4 waves of 64): 257 entries are one over it
SHAPES = [((40, 24, 56), (16, 16, 16), 4), ((48, 80), (32, 32), 8)]
SHAPE_IDS = ["3d", "2d"]


def _dev(a):
    import torch
    a = np.ascontiguousarray(a)
    if a.size == 0:
        return torch.empty(16, dtype=torch.uint8, device="cuda")
    return torch.from_numpy(a).cuda()


def _random_batch(seed, big, counts, weight=True):
    """Events with the given numbers of distinct random voxels, random values / labels / weights (bit patterns matter, not values)."""
    rng = np.random.default_rng(seed)
    V = int(np.prod(big))
    idx = [np.sort(rng.choice(V, m, replace=False)).astype(np.int32) for m in counts]
    off = np.concatenate([[0], np.cumsum(counts)]).astype(np.int64)
    M = int(off[-1])
    f = lambda: rng.standard_normal(M).astype(np.float32)
    return VoxelBatch(off, np.concatenate(idx) if M else np.zeros(0, np.int32), f(), f(), f() if weight else None,
                      rng.standard_normal(len(counts)).astype(np.float32) if weight else None, V).validate()


def _crop_desc(vb, big, tile, boxes, keep, drop=()):
    nd = len(big)
    d = _lib.ursn_crop_desc()
    d.ndim, d.n, d.boxes, d.m_total = nd, vb.n, len(boxes), int(vb.offsets[-1])
    for i in range(nd):
        d.big[i], d.tile[i] = big[i], tile[i]
    for name in ("offsets", "index", "value", "label", "weight", "bg_weight"):
        a = getattr(vb, name)
        if a is not None and name not in drop:
            keep[name] = _dev(a)
            setattr(d, name, keep[name].data_ptr())
    for name in ("event", "origin", "core_lo", "core_hi"):
        a = getattr(boxes, name)
        if a is not None:
            keep["box_" + name] = _dev(a)
            setattr(d, name if name.startswith("core") else "box_" + name, keep["box_" + name].data_ptr())
    return d


def _device_crop(lib, vb, big, tile, boxes, cap=None, absent=(), scratch_fill=0xFF):
    """ursn_crop_count, then ursn_crop_write into guarded 0xFF-filled outputs of exactly `cap` entries (default: the true total).
    Returns the raw outputs; asserts every guard, the scratch's included."""
    import torch
    keep = {}
    src_drop = tuple(n for n in absent if n in ("value", "label")) + (("weight", "bg_weight") if "weight" in absent else ())
    d = _crop_desc(vb, big, tile, boxes, keep, drop=src_drop)
    B = len(boxes)
    need = int(lib.ursn_crop_scratch_bytes(len(big), d.big, d.tile, B))
    assert need > 0
    scratch = _Guarded(need, GUARD, scratch_fill)
    cnt, own = _Guarded(8 * B, GUARD, 0xFF), _Guarded(8 * B, GUARD, 0xFF)
    torch.cuda.synchronize()
    P = lambda g: ctypes.c_void_p(g.ptr)
    _lib.check(lib.ursn_crop_count(ctypes.byref(d), P(cnt), P(own), P(scratch), need, None))
    torch.cuda.synchronize()
    res = {"count": cnt.view.cpu().numpy().view(np.int64).copy(), "owned_count": own.view.cpu().numpy().view(np.int64).copy()}
    total = int(res["count"].sum())
    cap = total if cap is None else cap
    sizes = {"offsets": 8 * (B + 1), "index": 4 * cap, "value": 4 * cap, "label": 4 * cap, "weight": 4 * cap, "bg_weight": 4 * B,
             "src": 4 * cap, "owned": cap}
    have = ["offsets", "index"] + [n for n in ("value", "label") if getattr(vb, n) is not None and n not in absent]
    if vb.weight is not None and "weight" not in absent:
        have += ["weight", "bg_weight"]
    have += [n for n in ("src", "owned") if n not in absent]
    out = {n: _Guarded(sizes[n], GUARD, 0xFF) for n in have}
    o = _lib.ursn_crop_out()
    for n, g in out.items():
        setattr(o, n, g.ptr)
    o.cap = cap
    torch.cuda.synchronize()
    _lib.check(lib.ursn_crop_write(ctypes.byref(d), ctypes.byref(o), P(scratch), need, None))
    torch.cuda.synchronize()
    assert lib.ursn_last_kernel_name() == b"crop_write"
    for n, g in list(out.items()) + [("scratch", scratch), ("count", cnt), ("owned_count", own)]:
        assert g.guards_intact() == (True, True), n
    dt = {"offsets": np.int64, "index": np.int32, "value": np.uint32, "label": np.uint32, "weight": np.uint32, "bg_weight": np.uint32,
          "src": np.int32, "owned": np.uint8}
    for n, g in out.items():
        res[n] = g.view.cpu().numpy().view(dt[n]).copy()
    res["cap"] = cap
    return res


def _u32(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _check_crop(got, vb, big, tile, boxes, what):
    """The device outputs against crop_numpy, bit for bit; past `cap` and the true total nothing but the 0xFF fill."""
    crop, src, owned, count, owned_count = tiling.crop_numpy(vb, big, tile, boxes)
    assert np.array_equal(got["count"], count) and np.array_equal(got["owned_count"], owned_count), what
    assert np.array_equal(got["offsets"], crop.offsets), what                    # the true counts, whatever cap is
    m = min(got["cap"], int(crop.offsets[-1]))
    want = {"index": crop.index, "src": src, "owned": owned}
    for n in ("value", "label", "weight"):
        if getattr(crop, n) is not None:
            want[n] = _u32(getattr(crop, n))
    for n, w in want.items():
        if n in got:
            assert np.array_equal(got[n][:m], w[:m]), (what, n)
            assert (got[n][m:].view(np.uint8) == 0xFF).all(), (what, n, "written past the entries")
    if "bg_weight" in got:
        assert np.array_equal(got["bg_weight"], _u32(crop.bg_weight)), what
    return crop, src, owned


# ---- op level: the crop -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("big,tile,halo", SHAPES, ids=SHAPE_IDS)
def test_crop_equals_crop_numpy_on_the_grid(lib, big, tile, halo):
    boxes = tiling.grid(big, tile, halo, n=3)
    V = int(np.prod(big))
    dense = V // 3                                       # long ranges: every wave of a box walks several 64-entry steps
    for j, counts in enumerate([(0, STEP + 1, 3 * STEP + 5), (STEP + 1, 0, 64), (dense, 63, 65), (0, 0, 0)]):
        vb = _random_batch(100 + j, big, counts)
        got = _device_crop(lib, vb, big, tile, boxes)
        crop, src, owned = _check_crop(got, vb, big, tile, boxes, counts)
        crop.validate()
        M = int(vb.offsets[-1])
        assert np.array_equal(np.sort(src[owned == 1]), np.arange(M))          # the cores partition the volume
        assert got["count"].sum() >= M and got["owned_count"].sum() == M


def test_crop_of_a_fully_listed_volume(lib):
    big, tile = (8, 8, 8), (4, 4, 4)
    vb = VoxelBatch([0, 512, 1024], np.tile(np.arange(512), 2), np.arange(1024) + 1.0, np.arange(1024) % 3, voxels=512).validate()
    for halo in (0, 1):
        boxes = tiling.grid(big, tile, halo, n=2)
        got = _device_crop(lib, vb, big, tile, boxes)
        _check_crop(got, vb, big, tile, boxes, halo)
        assert (got["count"] == 64).all() and got["owned_count"].sum() == 1024


def test_crop_of_hand_made_boxes(lib):
    big, tile = (40, 24, 56), (16, 16, 16)
    vb = _random_batch(7, big, (700, 0, 900))
    origin = [[-3, -5, -7], [30, 15, 50], [8, 4, 20], [8, 4, 20], [100, 100, 100], [-16, 0, 0], [0, 0, 0], [12, 4, 20]]
    event = [0, 2, 2, 2, 0, 0, 1, 5]                     # overhangs, a duplicate, boxes outside, an empty event, a foreign event
    lo = [[0, 0, 0], [2, 3, 4], [4, 4, 4], [4, 4, 4], [0, 0, 0], [0, 0, 0], [0, 0, 0], [0, 0, 0]]
    hi = [[16, 16, 16], [10, 9, 6], [12, 12, 12], [12, 12, 12], [16, 16, 16], [16, 16, 16], [16, 16, 16], [0, 0, 0]]
    boxes = tiling.Boxes(event, origin, lo, hi)
    got = _device_crop(lib, vb, big, tile, boxes)
    _check_crop(got, vb, big, tile, boxes, "hand-made")
    assert got["count"][2] == got["count"][3] > 0 and list(got["count"][4:]) == [0, 0, 0, 0] and got["count"][0] > 0
    # without cores every box owns all of itself
    plain = tiling.Boxes(event, origin)
    got = _device_crop(lib, vb, big, tile, plain)
    _check_crop(got, vb, big, tile, plain, "no cores")
    assert np.array_equal(got["count"], got["owned_count"]) and (got["owned"] == 1).all()
    for b in range(len(boxes)):                           # B = 1, every box on its own
        one = boxes.select(slice(b, b + 1))
        _check_crop(_device_crop(lib, vb, big, tile, one), vb, big, tile, one, b)
    # a box that covers the whole volume: the crop is the list itself, moved by the origin
    small, wide = (10, 6, 12), (16, 16, 16)
    vs = _random_batch(8, small, (STEP + 1, 300))
    cover = tiling.Boxes([0, 1, 1], [[-2, -3, -1], [0, 0, 0], [-6, -10, -4]])
    got = _device_crop(lib, vs, small, wide, cover)
    _check_crop(got, vs, small, wide, cover, "cover")
    assert list(got["count"]) == [STEP + 1, 300, 300] and np.array_equal(got["src"][:STEP + 1], np.arange(STEP + 1))


@pytest.mark.parametrize("big,tile,origin", [((40, 24, 56), (16, 16, 16), (8, 4, 20)), ((48, 80), (32, 32), (9, 40))], ids=SHAPE_IDS)
def test_crop_takes_the_faces_and_nothing_one_step_outside(lib, big, tile, origin):
    nd = len(big)
    mid = [o + t // 2 for o, t in zip(origin, tile)]
    inside, outside = [], []
    for ax in range(nd):
        for x, where in ((origin[ax], inside), (origin[ax] - 1, outside), (origin[ax] + tile[ax] - 1, inside),
                         (origin[ax] + tile[ax], outside)):
            p = list(mid)
            p[ax] = x
            where.append(int(np.ravel_multi_index(p, big)))
    index = np.sort(np.array(inside + outside, np.int32))
    vb = VoxelBatch([0, index.size], index, np.arange(index.size) + 1.0, voxels=int(np.prod(big))).validate()
    boxes = tiling.Boxes([0], [list(origin)], [[1] * nd], [[t - 1 for t in tile]])     # the core: the box without its faces
    got = _device_crop(lib, vb, big, tile, boxes)
    _check_crop(got, vb, big, tile, boxes, "faces")
    assert got["count"][0] == 2 * nd and got["owned_count"][0] == 0
    assert sorted(index[got["src"]]) == sorted(inside)


@pytest.mark.parametrize("big,tile,halo", SHAPES, ids=SHAPE_IDS)
def test_crop_with_a_short_cap_and_with_each_optional_array_absent(lib, big, tile, halo):
    boxes = tiling.grid(big, tile, halo, n=3)
    vb = _random_batch(11, big, (STEP + 1, 0, 3 * STEP + 5))
    total = int(tiling.crop_numpy(vb, big, tile, boxes)[3].sum())
    for cap in (total - 1, total // 2, 0):
        got = _device_crop(lib, vb, big, tile, boxes, cap=cap)                     # the outputs hold `cap` entries and not one more
        _check_crop(got, vb, big, tile, boxes, cap)
        assert int(got["offsets"][-1]) == total > cap
    full = _device_crop(lib, vb, big, tile, boxes)
    for name in ("value", "label", "weight", "src", "owned"):
        got = _device_crop(lib, vb, big, tile, boxes, absent=(name,))
        assert name not in got and ("bg_weight" in got) == (name != "weight")
        _check_crop(got, vb, big, tile, boxes, name)
        for k in got:
            assert np.array_equal(got[k], full[k]), (name, k)
    bare = _device_crop(lib, vb, big, tile, boxes, absent=("value", "label", "weight", "src", "owned"))
    assert sorted(bare) == ["cap", "count", "index", "offsets", "owned_count"] and np.array_equal(bare["index"], full["index"])
    noweight = VoxelBatch(vb.offsets, vb.index, vb.value, vb.label, voxels=vb.voxels)
    _check_crop(_device_crop(lib, noweight, big, tile, boxes), noweight, big, tile, boxes, "a batch without weights")


def test_crop_does_not_depend_on_the_scratch_or_on_earlier_calls(lib):
    big, tile, halo = SHAPES[0]
    boxes = tiling.grid(big, tile, halo, n=3)
    vb, other = _random_batch(21, big, (900, 5, 400)), _random_batch(22, big, (3000, 3000, 3000))
    first = _device_crop(lib, vb, big, tile, boxes, scratch_fill=0x00)
    _device_crop(lib, other, big, tile, boxes, scratch_fill=0x7F)
    again = _device_crop(lib, vb, big, tile, boxes, scratch_fill=0xFF)
    for k in first:
        assert np.array_equal(first[k], again[k]), k


# ---- op level: the scatter --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("ncls", [1, 3, 8])
def test_scatter_equals_stitch_numpy(lib, ncls):
    import torch
    rng = np.random.default_rng(31 + ncls)
    rows_out, m = 3 * STEP + 7, 2 * STEP + 1
    src = rng.permutation(rows_out)[:m].astype(np.int32)                           # distinct targets: every row written at most once
    scores = rng.standard_normal((m, ncls)).astype(np.float32)
    pred, ana = rng.integers(0, 200, m).astype(np.uint8), rng.integers(0, 3, m).astype(np.uint8)
    d_src, d_scores, d_pred, d_ana = _dev(src), _dev(scores), _dev(pred), _dev(ana)
    P = lambda t: ctypes.c_void_p(t.ptr if isinstance(t, _Guarded) else t.data_ptr()) if t is not None else None
    for what, owned in (("none", np.zeros(m, np.uint8)), ("all", np.ones(m, np.uint8)), ("mixed", (rng.uniform(0, 1, m) < 0.5).astype(np.uint8))):
        d_owned = _dev(owned)
        for want in (("scores", "pred", "ana"), ("scores",), ("pred",), ("ana",)):
            out = {"scores": _Guarded(rows_out * ncls * 4, GUARD, 0xFF), "pred": _Guarded(rows_out, GUARD, 0xFF),
                   "ana": _Guarded(rows_out, GUARD, 0xFF)}
            torch.cuda.synchronize()
            g = lambda n, t: t if n in want else None
            _lib.check(lib.ursn_scores_scatter(P(d_src), P(d_owned), m, ncls, P(g("scores", d_scores)), P(g("pred", d_pred)),
                                               P(g("ana", d_ana)), P(g("scores", out["scores"])), P(g("pred", out["pred"])),
                                               P(g("ana", out["ana"])), rows_out, None))
            torch.cuda.synchronize()
            ref = {"scores": np.full((rows_out, ncls), 0xFFFFFFFF, np.uint32), "pred": np.full(rows_out, 0xFF, np.uint8),
                   "ana": np.full(rows_out, 0xFF, np.uint8)}
            tiling.stitch_numpy(ref, src, owned, **{n: {"scores": scores.view(np.uint32), "pred": pred, "ana": ana}[n] for n in want})
            for n, gd in out.items():
                assert gd.guards_intact() == (True, True), (what, want, n)
                got = gd.view.cpu().numpy().view(ref[n].dtype).reshape(ref[n].shape)
                assert np.array_equal(got, ref[n]), (what, want, n)               # rows not owned keep their 0xFF fill
    # a source position outside [0, rows_out) writes nothing; m = 0 launches nothing
    wild = src.copy()
    wild[::7] = rows_out
    wild[3::7] = -1
    out = _Guarded(rows_out, GUARD, 0xFF)
    d_wild, d_one = _dev(wild), _dev(np.ones(m, np.uint8))
    torch.cuda.synchronize()
    _lib.check(lib.ursn_scores_scatter(P(d_wild), P(d_one), m, ncls, None, P(d_pred), None, None, P(out), None, rows_out, None))
    _lib.check(lib.ursn_scores_scatter(P(d_wild), P(d_one), 0, ncls, None, P(d_pred), None, None, P(out), None, rows_out, None))
    torch.cuda.synchronize()
    ok = (wild >= 0) & (wild < rows_out)
    ref = np.full(rows_out, 0xFF, np.uint8)
    ref[wild[ok]] = pred[ok]
    assert out.guards_intact() == (True, True) and np.array_equal(out.view.cpu().numpy(), ref)


# ---- op level: the largest legal extents (tests/_far_corner.py) ----------------------------------------------------
FAR_BIG = [(far.LARGEST_VOLUME, (16, 16, 16)), (far.AXIS0_CAP, (16, 16, 16)), (far.WIDEST_2D, (32, 32))]


def _far_corner_list(big, seed):
    """Three events, the middle one empty: a few hundred distinct voxels within 40 of the far corner, the far corner itself, and
    voxel 0 and its neighbours at the origin."""
    rng = np.random.default_rng(seed)
    nd, top = len(big), np.array(big, np.int64) - 1
    lists = []
    for m in (300, 0, 400):
        x = np.concatenate([top - rng.integers(0, 40, (m, nd)), rng.integers(0, 3, (m // 20, nd)), top[None, :][:m], 0 * top[None, :][:m]])
        lists.append(np.unique(far.ravel(x, big)))
    off = np.concatenate([[0], np.cumsum([a.size for a in lists])]).astype(np.int64)
    M = int(off[-1])
    f = lambda: rng.standard_normal(M).astype(np.float32)
    return VoxelBatch(off, np.concatenate(lists).astype(np.int32), f(), f(), f(), rng.standard_normal(3).astype(np.float32),
                      far.volume(big)).validate()


@pytest.mark.parametrize("big,tile", FAR_BIG, ids=[far.shape_id(b) for b, _ in FAR_BIG])
def test_crop_and_scatter_in_the_far_corner(lib, big, tile):
    """Boxes flush with the far corner, overhanging it by half a tile, entirely beyond it and at the origin, in the largest volume,
    with axis 0 at its cap and in the widest 2-D shape: the crop against crop_numpy, then the scatter of scores computed on the
    crop against stitch_numpy."""
    import torch
    nd, top = len(big), np.array(big, np.int64) - 1
    T = np.array(tile, np.int64)
    vb = _far_corner_list(big, 41 + nd)
    M = int(vb.offsets[-1])
    assert int(vb.index.max()) == far.volume(big) - 1 and int(vb.index.min()) == 0 and M > 600
    origin = [top + 1 - T, top + 1 - T, top + 1 - T // 2, top + 1, top + 1 + T, 0 * T, -(T // 2), top + 1 - 2 * T, top - 20]
    event = [0, 2, 2, 0, 2, 0, 2, 2, 1]                      # the last: an empty event's box
    lo = [0 * T] * 8 + [0 * T]
    hi = [T, T // 2, T, T, T, T, T, T - 3, T]
    boxes = tiling.Boxes(event, [[int(v) for v in o] for o in origin], [[int(v) for v in a] for a in lo], [[int(v) for v in a] for a in hi])
    for fill in (0xFF, 0x00):
        got = _device_crop(lib, vb, big, tile, boxes, scratch_fill=fill)
        crop, src, owned = _check_crop(got, vb, big, tile, boxes, (big, fill))
    count = got["count"].tolist()
    assert count[0] > 0 and count[1] > 0 and count[2] > 0 and count[3:5] == [0, 0] and count[5] > 0 and count[6] > 0 and count[8] == 0
    one = boxes.select(slice(2, 3))                          # the overhanging box on its own
    _check_crop(_device_crop(lib, vb, big, tile, one), vb, big, tile, one, (big, "overhang"))
    # the scatter back into the list: rows of boxes that own them
    m, ncls = int(crop.offsets[-1]), 3
    rng = np.random.default_rng(5)
    scores = rng.standard_normal((m, ncls)).astype(np.float32)
    pred, ana = rng.integers(0, 200, m).astype(np.uint8), rng.integers(0, 3, m).astype(np.uint8)
    first = np.zeros(m, np.uint8)                            # every list row written at most once: its first owner only
    seen = set()
    for k in np.flatnonzero(owned):
        if int(src[k]) not in seen:
            seen.add(int(src[k]))
            first[k] = 1
    out = {"scores": _Guarded(M * ncls * 4, GUARD, 0xFF), "pred": _Guarded(M, GUARD, 0xFF), "ana": _Guarded(M, GUARD, 0xFF)}
    keep = [_dev(a) for a in (src.astype(np.int32), first, scores, pred, ana)]
    P = lambda t: ctypes.c_void_p(t.ptr if isinstance(t, _Guarded) else t.data_ptr())
    torch.cuda.synchronize()
    _lib.check(lib.ursn_scores_scatter(P(keep[0]), P(keep[1]), m, ncls, P(keep[2]), P(keep[3]), P(keep[4]), P(out["scores"]),
                                       P(out["pred"]), P(out["ana"]), M, None))
    torch.cuda.synchronize()
    ref = {"scores": np.full((M, ncls), 0xFFFFFFFF, np.uint32), "pred": np.full(M, 0xFF, np.uint8), "ana": np.full(M, 0xFF, np.uint8)}
    tiling.stitch_numpy(ref, src, first, scores=scores.view(np.uint32), pred=pred, ana=ana)
    assert len(seen) > 50
    for n, g in out.items():
        assert g.guards_intact() == (True, True), n
        assert np.array_equal(g.view.cpu().numpy().view(ref[n].dtype).reshape(ref[n].shape), ref[n]), n


# ---- net level ----------------------------------------------------------------------------------------------------------------------
NETS = [
    # dims, F, num_strides, classes, precision, large shape, halo
    ((16, 16, 16, 1), 4, 2, 3, "fp32", (40, 24, 56), 4),
    ((32, 32, 1), 8, 3, 3, "bf16", (48, 80), 8),
    ((16, 16, 16, 1), 8, 2, 3, "bf16", (40, 24, 56), 4),
]
NET_IDS = ["16x16x16_f4_fp32", "32x32_f8_bf16", "16x16x16_f8_bf16"]
_cache = {}


def _large(big, entries=(0, 1, 2)):
    key = (big, entries)
    if key not in _cache:
        _cache[key] = VoxelBatch.concat([sio.dense_to_voxels(*sio.lartpc_sparse(list(big) + [1], 3, e)) for e in entries]).validate()
    return _cache[key]


def _net(case, trainable=False, bn_moving=False, use_weight=True):
    dims, F, ns, ncls, prec = case[:5]
    net = uresnet(dims=list(dims), num_class=ncls, base_num_outputs=F, num_strides=ns)
    net.construct(trainable=trainable, use_weight=use_weight, learning_rate=1e-3, seed=7, precision=prec, bn_moving=bn_moving)
    return net


def _random_stats(net, seed):
    """Plausible statistics: means ~ N(0, 0.3), variances in [0.2, 2] (as tests/test_bn_moving_gpu.py draws them)."""
    rng = np.random.default_rng(seed)
    v = {}
    for name, c, _ in net._bn_specs:
        v[name + "/moving_mean"] = rng.normal(0.0, 0.3, c).astype(np.float32)
        v[name + "/moving_variance"] = rng.uniform(0.2, 2.0, c).astype(np.float32)
    return v


def _host_tiled(net, vb, big, halo, tile_batch, want=("scores", "pred", "ana")):
    """The definition: the grid's boxes cropped by crop_numpy, those that own nothing dropped, the rest grouped in box order, each
    group through the EXISTING inference_voxel_scores, stitched by stitch_numpy."""
    tile = tuple(int(d) for d in net._dims[:-1])
    boxes = tiling.grid(big, tile, halo, n=vb.n)
    owned_count = tiling.crop_numpy(vb, big, tile, boxes)[4]
    keep = np.flatnonzero(owned_count > 0)
    run = boxes.select(keep)
    M, C = int(vb.offsets[-1]), net._num_class
    out = {"scores": np.zeros((M, C), np.float32), "pred": np.zeros(M, np.uint8), "ana": np.zeros(M, np.uint8)}
    forwards = 0
    for first in range(0, len(run), tile_batch):
        crop, src, owned, _, _ = tiling.crop_numpy(vb, big, tile, run.select(slice(first, first + tile_batch)))
        bare = VoxelBatch(crop.offsets, crop.index, crop.value, voxels=crop.voxels)
        r = net.inference_voxel_scores(None, bare, with_labels=False, want=want)
        tiling.stitch_numpy(out, src, owned, **{w: np.concatenate(r[w]) for w in want})
        forwards += 1
    off = vb.offsets
    res = {w: [out[w][off[i]:off[i + 1]] for i in range(vb.n)] for w in want}
    res["index"] = [vb.index[off[i]:off[i + 1]] for i in range(vb.n)]
    res.update(tiles_total=len(boxes), tiles_run=int(keep.size), forwards=forwards)
    return res


def _same_result(a, b):
    if set(a) != set(b):
        return False
    for k in a:
        if isinstance(a[k], int):
            if a[k] != b[k]:
                return False
        elif not all(x.dtype == y.dtype and x.shape == y.shape and np.array_equal(x.view(np.uint8), y.view(np.uint8))
                     for x, y in zip(a[k], b[k])):
            return False
    return True


@pytest.mark.parametrize("case", NETS, ids=NET_IDS)
def test_tiled_inference_equals_host_crops_through_the_existing_call(case):
    big, halo = case[5], case[6]
    vb = _large(big)
    net = _net(case)
    resident = net.upload_voxels(vb, big)
    assert net.feed_stats["h2d_calls"] == 1
    seen = set()
    for h, tb in ((halo, 3), (halo, 1), (0, 3), (0, 1)):
        h2d = net.feed_stats["h2d_calls"]
        got = net.inference_tiled_voxel_scores(None, resident, big, halo=h, tile_batch=tb)
        assert net.feed_stats["h2d_calls"] == h2d                  # the list went up once, with upload_voxels
        want = _host_tiled(net, vb, big, h, tb)
        assert _same_result(got, want), (h, tb)
        assert got["forwards"] == -(-got["tiles_run"] // tb)
        seen |= set(np.unique(np.concatenate(got["ana"]))) | set(10 + np.unique(np.concatenate(got["pred"])))
    assert seen - {0, 10}, "neither the ana rule nor the argmax ever left class 0: the comparison would be empty"
    # a subset of the outputs, and a VoxelBatch instead of a resident batch (uploaded by the call): the same rows
    sub = net.inference_tiled_voxel_scores(None, vb, big, halo=halo, tile_batch=3, want=("pred",))
    full = net.inference_tiled_voxel_scores(None, resident, big, halo=halo, tile_batch=3)
    assert set(sub) == {"index", "pred", "tiles_total", "tiles_run", "forwards"}
    assert all(np.array_equal(a, b) for a, b in zip(sub["pred"], full["pred"]))


@pytest.mark.parametrize("case", NETS, ids=NET_IDS)
def test_a_volume_of_the_networks_size_is_one_box_equal_to_inference_voxel_scores(case):
    dims = case[0]
    tile = tuple(dims[:-1])
    vb = _large(tile)
    assert (np.diff(vb.offsets) > 0).all()
    net = _net(case)
    ref = net.inference_voxel_scores(None, VoxelBatch(vb.offsets, vb.index, vb.value, voxels=vb.voxels), with_labels=False)
    for halo in (0, 4):
        got = net.inference_tiled_voxel_scores(None, vb, tile, halo=halo, tile_batch=vb.n)
        assert (got["tiles_total"], got["tiles_run"], got["forwards"]) == (vb.n, vb.n, 1)
        for k in ("index", "scores", "pred", "ana"):
            assert all(x.dtype == y.dtype and np.array_equal(x.view(np.uint8), y.view(np.uint8)) for x, y in zip(got[k], ref[k])), k


def test_tiles_that_own_no_voxel_are_not_run():
    big, halo = (40, 24, 56), 4
    net = _net(NETS[0])
    want_3d = {0: 17, 1: 25, 2: 21}                      # owning boxes of 48, from crop_numpy on the CPU
    for e, want in want_3d.items():
        vb = _large(big, (e,))
        owned = tiling.crop_numpy(vb, big, (16, 16, 16), tiling.grid(big, (16, 16, 16), halo))[4]
        assert int((owned > 0).sum()) == want and owned.size == 48          # the condition on the inputs
        got = net.inference_tiled_voxel_scores(None, vb, big, halo=halo, tile_batch=3)
        assert (got["tiles_run"], got["tiles_total"]) == (want, 48) and got["forwards"] == -(-want // 3)
    vb = _large(big)
    got = net.inference_tiled_voxel_scores(None, vb, big, halo=halo, tile_batch=3)
    assert (got["tiles_run"], got["tiles_total"]) == (17 + 25 + 21, 144)
    net2 = _net(NETS[1])
    vb = _large((48, 80), (0,))
    owned = tiling.crop_numpy(vb, (48, 80), (32, 32), tiling.grid((48, 80), (32, 32), 8))[4]
    assert int((owned > 0).sum()) == 7 and owned.size == 8
    got = net2.inference_tiled_voxel_scores(None, vb, (48, 80), halo=8, tile_batch=3)
    assert (got["tiles_run"], got["tiles_total"], got["forwards"]) == (7, 8, 3)
    # a batch without a single voxel: nothing runs, every list is empty
    none = VoxelBatch([0, 0, 0], [], [], voxels=48 * 80)
    got = net2.inference_tiled_voxel_scores(None, none, (48, 80), halo=8)
    assert (got["tiles_run"], got["tiles_total"], got["forwards"]) == (0, 16, 0) and got["scores"][1].shape == (0, 3)


@pytest.mark.parametrize("case", NETS, ids=NET_IDS)
def test_in_moving_mode_the_tile_batch_does_not_matter(case):
    """The 1e-5 max_rel that tests/test_bn_moving_gpu.py holds 'an event no longer depends on its batch' to; in batch mode the same
    comparison is far off, which shows that the bound has something to hold."""
    big, halo = case[5], case[6]
    vb = _large(big)
    net = _net(case, bn_moving=True)
    net.set_bn_moving(_random_stats(net, 19))
    res = {}
    for mode in ("batch", "moving"):
        net.set_bn_mode(mode)
        one = net.inference_tiled_voxel_scores(None, vb, big, halo=halo, tile_batch=1, want=("scores",))
        three = net.inference_tiled_voxel_scores(None, vb, big, halo=halo, tile_batch=3, want=("scores",))
        res[mode] = max_rel(np.concatenate(one["scores"]), np.concatenate(three["scores"]))
    print("%s: tile_batch 1 against 3, scores max_rel: batch mode %.2e, moving mode %.2e" % (NET_IDS[NETS.index(case)], res["batch"], res["moving"]))
    assert res["moving"] < 1e-5
    assert res["batch"] > 1e-3


def _grad_bits(net):
    g = net.get_gradients()
    return {k: np.ascontiguousarray(v, np.float32).view(np.uint32) for k, v in g.items()}


@pytest.mark.parametrize("case", NETS, ids=NET_IDS)
def test_crop_training_equals_feeding_the_host_crop(case):
    big = case[5]
    vb = _large(big)
    nd = len(big)
    net = _net(case, trainable=True)
    tile = tuple(int(d) for d in net._dims[:-1])
    resident = net.upload_voxels(vb, big)
    boxes = tiling.random_boxes(5, vb, big, tile)
    crop = tiling.crop_numpy(vb, big, tile, boxes)[0]
    assert (np.diff(crop.offsets) > 0).all()
    noweight = VoxelBatch(vb.offsets, vb.index, vb.value, vb.label, voxels=vb.voxels)
    crop_nw = VoxelBatch(crop.offsets, crop.index, crop.value, crop.label, voxels=crop.voxels)
    resident_nw = net.upload_voxels(noweight, big)
    codes = [1, 0, 3] if nd == 3 else [1, 0, 2]
    spec = WeightSpec("invfreq", 1, [1.0, 2.0, 2.0, 5.0])
    variants = [({}, resident, crop), (dict(symmetry=codes), resident, crop), (dict(normalize_weight=True), resident, crop),
                (dict(make_weight=spec), resident_nw, crop_nw),
                (dict(symmetry=codes, make_weight=spec, normalize_weight=True), resident_nw, crop_nw)]
    for kw, res_batch, host_crop in variants:
        net.zero_gradients(None)
        want_m, _ = net.accum_gradients_voxels(None, host_crop, **kw)
        want_g = _grad_bits(net)
        net.zero_gradients(None)
        got_m, _ = net.accum_gradients_voxels(None, None, crop=(res_batch, boxes), **kw)
        got_g = _grad_bits(net)
        assert same_bits(np.asarray(got_m[1:], np.float32), np.asarray(want_m[1:], np.float32)), (kw, got_m, want_m)
        assert np.isfinite(got_m[1]) and got_m[1] > 0
        for k in want_g:
            assert np.array_equal(got_g[k], want_g[k]), (sorted(kw), k)
        assert any(v.any() for v in got_g.values())
        got_t, _ = net.run_test_voxels(None, None, crop=(res_batch, boxes), **{k: v for k, v in kw.items() if k != "symmetry"})
        want_t, _ = net.run_test_voxels(None, host_crop, **{k: v for k, v in kw.items() if k != "symmetry"})
        assert same_bits(np.asarray(got_t, np.float32), np.asarray(want_t, np.float32)), kw
    # boxes that overhang, repeat and hold nothing feed like any other event
    odd = tiling.Boxes([2, 2, 0, 1], [[-5] * nd, [-5] * nd, [s + 1 for s in big], [s - 9 for s in big]])
    host = tiling.crop_numpy(vb, big, tile, odd)[0]
    net.zero_gradients(None)
    want_m, _ = net.accum_gradients_voxels(None, host)
    want_g = _grad_bits(net)
    net.zero_gradients(None)
    got_m, _ = net.accum_gradients_voxels(None, None, crop=(resident, odd))
    assert same_bits(np.asarray(got_m[1:], np.float32), np.asarray(want_m[1:], np.float32))
    assert all(np.array_equal(v, want_g[k]) for k, v in _grad_bits(net).items())


def test_results_do_not_depend_on_the_scratch_or_on_the_calls_before():
    import torch
    case = NETS[0]
    big, halo = case[5], case[6]
    vb, other = _large(big), _large(big, (5, 6))
    net = _net(case, trainable=True)
    tile = tuple(int(d) for d in net._dims[:-1])
    resident = net.upload_voxels(vb, big)
    boxes = tiling.random_boxes(9, vb, big, tile)

    def both():
        r = net.inference_tiled_voxel_scores(None, resident, big, halo=halo, tile_batch=3)
        net.zero_gradients(None)
        m, _ = net.accum_gradients_voxels(None, None, crop=(resident, boxes))
        return r, np.asarray(m[1:], np.float32), _grad_bits(net)
    first = both()
    for fill in (0.0, float("nan")):
        net._crop_scratch_buf.view(dtype=torch.float64).fill_(fill)
        # other batches, other batch sizes, other entry points in between
        net.inference_tiled_voxel_scores(None, other, big, halo=0, tile_batch=2)
        net.accum_gradients_voxels(None, None, crop=(net.upload_voxels(other, big), tiling.random_boxes(1, other, big, tile)))
        net.inference_voxel_scores(None, tiling.crop_numpy(vb, big, tile, boxes)[0], with_labels=False)
        net._crop_scratch_buf.view(dtype=torch.float64).fill_(fill)
        again = both()
        assert _same_result(first[0], again[0]), fill
        assert same_bits(first[1], again[1]) and all(np.array_equal(v, again[2][k]) for k, v in first[2].items()), fill


# ---- driver -------------------------------------------------------------------------------------------------------------------------
def _driver(tmp_path, tag, text):
    from uresnet_amd.ssnet_trainval import ssnet_trainval
    inp = tmp_path / "input.cfg"
    inp.write_text("Dims [32, 32, 32, 1]\nNumClass 3\nGenerator 'lartpc_sparse'\nNumEntries 64\n"
                   "Keys {'data': 'data', 'label': 'label', 'weight': 'weight'}\n")
    cfg = tmp_path / ("%s.cfg" % tag)
    cfg.write_text("NUM_CLASS 3\nBASE_NUM_FILTERS 4\nMAIN_INPUT_CONFIG '%s'\nLOGDIR ''\nSAVE_FILE ''\nMINIBATCH_SIZE 2\n"
                   "SUMMARY_STEPS 0\nCHECKPOINT_STEPS 0\nSPARSE_IO True\n%s" % (inp, text))
    t = ssnet_trainval()
    with redirect_stdout(io.StringIO()):
        t.override_config(str(cfg))
    return t


def _records(path):
    recs = []
    with open(str(path), "rb") as f:
        blob = f.read()
    f = io.BytesIO(blob)
    while f.tell() < len(blob):
        recs.append(np.load(f))
    return recs


def test_driver_analyses_large_events_tile_by_tile(tmp_path, capsys):
    big = (80, 48, 64)
    out = tmp_path / "tiled.npy"
    t = _driver(tmp_path, "ana", "TRAIN False\nUSE_WEIGHTS False\nITERATIONS 1\nANA_OUTPUT_CONFIG '%s'\nANA_TILE %s\nANA_TILE_HALO 4\n"
                "ANA_TILE_BATCH 3\n" % (out, list(big)))
    t.initialize()
    assert [int(d) for d in t._net._dims] == [32, 32, 32, 1]
    t.batch_process()
    t.reset()
    printed = capsys.readouterr().out
    assert "Tiles" in printed and "of 36" in printed
    # the same batch through the method, on a network built as the driver builds its own (seed TF_RANDOM_SEED)
    vb = _large(big, (0, 1))
    net = uresnet(dims=[32, 32, 32, 1], num_class=3, base_num_outputs=4)
    net.construct(trainable=False, use_weight=False, seed=1234)
    r = net.inference_tiled_voxel_scores(None, vb, big, halo=4, tile_batch=3)
    assert 0 < r["tiles_run"] < r["tiles_total"] == 36
    recs = _records(out)
    assert len(recs) == 6
    for i in range(2):
        keep = r["ana"][i] != 0
        assert keep.any()
        assert np.array_equal(recs[3 * i], r["index"][i][keep]) and np.array_equal(recs[3 * i + 1], r["ana"][i][keep])
        assert same_bits(recs[3 * i + 2], np.ascontiguousarray(r["scores"][i][keep]))
    # interactive mode returns the per-event lists with indices in the large shape
    t = _driver(tmp_path, "ana2", "TRAIN False\nUSE_WEIGHTS False\nANA_TILE %s\nANA_TILE_HALO 4\nANA_TILE_BATCH 3\n" % list(big))
    t.initialize()
    res = t.ana_step()
    t.reset()
    assert res["tiles"] == (r["tiles_run"], 36) and res["acc_all"] is None and 0.0 <= res["acc_nonzero"] <= 1.0
    for i in range(2):
        assert np.array_equal(res["voxels"][i]["index"], r["index"][i]) and same_bits(res["voxels"][i]["scores"], r["scores"][i])
        assert int(res["voxels"][i]["index"].max()) >= 32 ** 3


def test_driver_trains_on_crops(tmp_path, capsys):
    big = (80, 48, 64)
    t = _driver(tmp_path, "train", "TRAIN True\nUSE_WEIGHTS True\nITERATIONS 2\nNUM_MINIBATCHES 1\nREPORT_STEPS 1\nLEARNING_RATE 0.001\n"
                "TRAIN_CROP %s\nCROP_SEED 3\nAUGMENT 'flip'\nAUGMENT_SEED 2\n" % list(big))
    t.initialize()
    t.train_step()
    got = {k: np.ascontiguousarray(v, np.float32).view(np.uint32) for k, v in t._net.get_gradients().items()}
    printed = capsys.readouterr().out
    assert "Train set" in printed and "nan" not in printed.lower()
    # the first step again, by hand: upload, one crop per event from (CROP_SEED, iteration 0, minibatch 0, rank 0), device-side norm
    from uresnet_amd import symmetry
    vb = _large(big, (0, 1))
    net = uresnet(dims=[32, 32, 32, 1], num_class=3, base_num_outputs=4)
    net.construct(trainable=True, use_weight=True, learning_rate=0.001, seed=1234)
    boxes = tiling.random_boxes([3, 0, 1, 0], vb, big, (32, 32, 32))
    codes = symmetry.draw(2, 0, 0, 0, 2, symmetry.group("flip", [32, 32, 32]))
    net.zero_gradients(None)
    net.accum_gradients_voxels(None, None, crop=(net.upload_voxels(vb, big), boxes), normalize_weight=True, symmetry=codes)
    want = _grad_bits(net)
    assert all(np.array_equal(got[k], want[k]) for k in want) and any(v.any() for v in want.values())
    t.train_step()                                       # a second iteration draws other crops and still trains
    assert "nan" not in capsys.readouterr().out.lower()
    t.reset()
