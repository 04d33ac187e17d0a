"""Cube-symmetry augmentation and test-time averaging on the device (include/uresnet_hip.h; symmetry.hip), bit for bit against
the numpy definition uresnet_amd.symmetry.apply_numpy.  Op level: inputs are random 32-bit patterns viewed as float (NaN payloads,
-0.0, denormals), so any arithmetic on the way would show; every tensor sits between 0xFF-filled margins and canary guards.  Net
level: the pinned contract that a step depends only on its inputs makes "the device permuted the feed" and "numpy permuted the
feed" comparable bit for bit on ONE net."""
import ctypes
import types

import numpy as np
import pytest

import _far_corner as far
from _abi import _Guarded, same_bits
from uresnet_amd import _lib, uresnet
from uresnet_amd import symmetry as S
from uresnet_amd import synthetic_io as sio
from uresnet_amd.ssnet import VoxelBatch

pytestmark = pytest.mark.gpu

GUARD = 4096
T = 32                # SYM_T, the tile edge of the transposing path: sizes T - 1, T, T + 1 and 2T - 1, 2T, 2T + 1 are its edges


def _i32(*v):
    return (ctypes.c_int32 * len(v))(*v)


def _bits(shape, seed):
    return np.random.default_rng(seed).integers(0, 2 ** 32, size=shape, dtype=np.uint32).view(np.float32)


def _desc(spatial, n, channels, codes):
    d = _lib.ursn_sym_desc()
    d.ndim = len(spatial)
    for i, s in enumerate(spatial):
        d.spatial[i] = s
    d.n, d.channels = n, channels
    keep = _i32(*codes)
    d.ops = ctypes.cast(keep, ctypes.POINTER(ctypes.c_int32))
    return d, keep


class _Placed(object):
    """A tensor of `nbytes` that starts `shift` floats past a 256-byte boundary, inside a 0xFF-filled (or `fill`-filled) view with
    16 spare bytes behind it, inside canary guards."""

    def __init__(self, nbytes, shift, host=None, fill=0xFF):
        import torch
        self.g, self.nbytes, self.shift, self.fill = _Guarded(nbytes + 32, GUARD, fill), nbytes, shift, fill
        self.ptr = self.g.ptr + 4 * shift
        self.view = self.g.view[4 * shift:4 * shift + nbytes]
        if host is not None:
            self.view.copy_(torch.from_numpy(np.ascontiguousarray(host).reshape(-1).view(np.uint8)))

    def f32(self, shape):
        return self.view.cpu().numpy().view(np.float32).reshape(shape).copy()

    def check_surroundings(self):
        assert self.g.guards_intact() == (True, True)
        raw = self.g.view.cpu().numpy()
        assert (raw[:4 * self.shift] == self.fill).all() and (raw[4 * self.shift + self.nbytes:] == self.fill).all(), \
            "bytes next to the tensor were written"

    def untouched(self):
        self.check_surroundings()
        return bool((self.view == self.fill).all().item())


def _apply(lib, xs, spatial, codes, src_shifts=(0, 0, 0), dst_shifts=(0, 0, 0)):
    """One ursn_sym_apply call on 1..3 host tensors [n, *spatial, C]; returns the outputs after checking guards, margins and that
    the inputs are unchanged."""
    import torch
    n = xs[0].shape[0]
    C = xs[0].size // (n * int(np.prod(spatial)))
    d, keep = _desc(spatial, n, C, codes)
    src = [_Placed(x.nbytes, s, x) for x, s in zip(xs, src_shifts)]
    dst = [_Placed(x.nbytes, s) for x, s in zip(xs, dst_shifts)]
    ptrs = []
    for i in range(3):
        ptrs += [ctypes.c_void_p(src[i].ptr), ctypes.c_void_p(dst[i].ptr)] if i < len(xs) else [None, None]
    torch.cuda.synchronize()
    _lib.check(lib.ursn_sym_apply(ctypes.byref(d), *(ptrs + [None])))
    torch.cuda.synchronize()
    for p, x in zip(src, xs):
        p.check_surroundings()
        assert same_bits(p.f32(x.shape), x), "an input was written"
    for p in dst:
        p.check_surroundings()
    return [p.f32(x.shape) for p, x in zip(dst, xs)]


def _check_apply(lib, spatial, codes, channels=1, seed=0, pairs=1, src_shifts=(0, 0, 0), dst_shifts=(0, 0, 0)):
    n = len(codes)
    xs = [_bits((n,) + tuple(spatial) + (channels,), seed + 17 * k) for k in range(pairs)]
    got = _apply(lib, xs, spatial, codes, src_shifts, dst_shifts)
    for k in range(pairs):
        want = S.apply_batch(xs[k], spatial, codes)
        bad = [int(c) for i, c in enumerate(codes) if not same_bits(got[k][i], want[i])]
        assert not bad, "tensor %d: codes %s of shape %s x %d differ from apply_numpy" % (k, bad, spatial, channels)


# ---- ursn_sym_apply ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("spatial", [(5, 5, 5), (33, 33, 33), (7, 7), (66, 66)], ids=lambda s: "x".join(map(str, s)))
def test_every_code_in_one_call(lib, spatial):
    """One event per code: every code of the group, and a different code per event, in ONE launch."""
    _check_apply(lib, spatial, list(range(S.count(len(spatial)))))


@pytest.mark.parametrize("s", [1, 3, T - 1, T, T + 1, 2 * T - 1, 2 * T, 2 * T + 1])
def test_tile_edges_along_the_transposed_axes(lib, s):
    for k, spatial in enumerate(((s, s), (2, s, s), (s, 3, s), (s, s, 2), (s, s, s) if s <= T + 1 else (s, s))):
        _check_apply(lib, spatial, S.group("cube", spatial), seed=s + k)      # axes 0 <-> 1, 1 <-> 2, 0 <-> 2 and all of them


@pytest.mark.parametrize("spatial", [(4, 6, 6), (6, 4, 6), (5, 9)], ids=lambda s: "x".join(map(str, s)))
def test_non_cubic_shapes(lib, spatial):
    codes = S.group("cube", spatial)
    assert len(codes) == (4 if len(spatial) == 2 else 16)
    _check_apply(lib, spatial, codes)


@pytest.mark.parametrize("channels", [1, 3, 5, 8])
def test_channels(lib, channels):
    _check_apply(lib, (17, 17, 17), list(range(48)), channels=channels, seed=channels)
    _check_apply(lib, (2 * T + 2, 2 * T + 2), list(range(8)), channels=channels, seed=channels + 1)
    _check_apply(lib, (3, 2 * T + 1), [0, 1, 2, 3], channels=channels, seed=channels + 2)      # row path, rows of odd length


@pytest.mark.parametrize("shift", [0, 1, 2, 3])
def test_tensors_off_the_256_byte_boundary(lib, shift):
    """Source and destination 0..3 floats past a 256-byte boundary, in every combination: the 16-byte paths only where both
    sides allow them."""
    for other in range(4):
        _check_apply(lib, (7, 7, 7), list(range(48)), seed=4 * shift + other, src_shifts=(shift,) * 3, dst_shifts=(other,) * 3)
        _check_apply(lib, (6, 8), [0, 1, 2, 3], seed=shift, src_shifts=(shift,) * 3, dst_shifts=(other,) * 3)
    _check_apply(lib, (5, 5, 5), [3, 17, 44], seed=9, pairs=3, src_shifts=(shift, (shift + 1) % 4, (shift + 2) % 4),
                 dst_shifts=((shift + 3) % 4, shift, (shift + 1) % 4))


@pytest.mark.parametrize("pairs", [1, 2, 3])
def test_one_two_or_three_pairs_and_a_code_per_event(lib, pairs):
    _check_apply(lib, (9, 9, 9), [29, 0, 46], pairs=pairs, seed=pairs)
    _check_apply(lib, (T + 2, T + 2), [6, 3, 5], pairs=pairs, seed=pairs + 3)


def test_largest_batch(lib):
    codes = [i % 8 for i in range(1024)]
    _check_apply(lib, (3, 3), codes, pairs=2)


# ---- ursn_sym_accumulate ----------------------------------------------------------------------------------------------------
def _dyadic(shape, seed):
    return (np.random.default_rng(seed).integers(0, 4097, shape).astype(np.float64) / 1024.0).astype(np.float32)


def _accumulate(lib, views, spatial, channels, shift=0):
    """views: [(x [n, *spatial, C], codes)], accumulated in order into one NaN-filled buffer; the last call scales by 1 / K."""
    import torch
    K = len(views)
    n = views[0][0].shape[0]
    dst = _Placed(views[0][0].nbytes, shift)                     # 0xFF bytes: NaN everywhere
    for k, (x, codes) in enumerate(views):
        d, keep = _desc(spatial, n, channels, codes)
        src = _Placed(x.nbytes, (shift + k) % 4, x)
        torch.cuda.synchronize()
        _lib.check(lib.ursn_sym_accumulate(ctypes.byref(d), ctypes.c_void_p(src.ptr), ctypes.c_void_p(dst.ptr), int(k == 0),
                                           ctypes.c_float(np.float32(1.0 / K) if k == K - 1 else 1.0), None))
        torch.cuda.synchronize()
        src.check_surroundings()
        assert same_bits(src.f32(x.shape), x)
    dst.check_surroundings()
    return dst.f32(views[0][0].shape)


def _mean_formula(terms):
    """fp32 left-to-right sum in list order, then times np.float32(1 / K)."""
    acc = np.zeros_like(terms[0]) + terms[0]
    for t in terms[1:]:
        acc = (acc + t).astype(np.float32)
    return (acc * np.float32(1.0 / len(terms))).astype(np.float32)


@pytest.mark.parametrize("K", [1, 2, 3])
@pytest.mark.parametrize("spatial, channels", [((T + 1, T + 1, 5), 3), ((7, T + 3, T + 3), 3), ((2 * T + 1, 2 * T + 1), 1), ((9, 9, 9), 8)],
                         ids=["34x34x5x3", "7x35x35x3", "65x65x1", "9x9x9x8"])
def test_accumulate_matches_the_fp32_formula(lib, spatial, channels, K):
    n = 3
    pool = S.group("cube", spatial)
    rng = np.random.default_rng(K)
    views = [(_dyadic((n,) + spatial + (channels,), 10 * K + k), [int(c) for c in rng.choice(pool, n)]) for k in range(K)]
    for shift in (0, 1):
        got = _accumulate(lib, views, spatial, channels, shift)
        want = _mean_formula([S.apply_batch(x, spatial, codes) for x, codes in views])
        assert same_bits(got, want), (spatial, channels, K, shift)


# ---- ursn_voxels_to_dense_sym / ursn_voxel_index_sym ------------------------------------------------------------------------
def _events(spatial, seed):
    """An empty event, a full event and two ordinary ones, with a background weight that differs per event."""
    V = int(np.prod(spatial))
    rng = np.random.default_rng(seed)
    parts = []
    for e, m in enumerate((0, V, V // 3, 1)):
        idx = np.sort(rng.choice(V, m, replace=False)).astype(np.int32)
        parts.append(VoxelBatch([0, m], idx, _bits((m,), seed + e), _bits((m,), seed + 10 + e), _bits((m,), seed + 20 + e),
                                _bits((1,), seed + 30 + e), V))
    return VoxelBatch.concat(parts).validate()


def _upload_batch(vb, index=None):
    import torch
    keep = {k: torch.from_numpy(np.ascontiguousarray(getattr(vb, k) if k != 'index' or index is None else index)).cuda()
            for k in ('offsets', 'index', 'value', 'label', 'weight', 'bg_weight')}
    b = _lib.ursn_voxel_batch()
    b.n, b.voxels = vb.n, vb.voxels
    for k, t in keep.items():
        setattr(b, k, t.data_ptr())
    return b, keep


VOX_SHAPES = [(5, 5, 5), (6, 6), (3, T + 1, T + 1), (4, 6, 6)]


@pytest.mark.parametrize("spatial", VOX_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_voxels_to_dense_sym_is_apply_numpy_of_the_plain_expansion(lib, spatial):
    import torch
    vb = _events(spatial, 3)
    n, V, nd = vb.n, vb.voxels, len(spatial)
    assert V % 4 != 0 or spatial != (5, 5, 5)
    plain = sio.voxels_to_dense(vb)
    pool = S.group("cube", spatial)
    for trial in range(3):
        codes = [int(c) for c in np.random.default_rng(trial).choice(pool, n)] if trial else [pool[-1], pool[1], 0, pool[len(pool) // 2]]
        b, keep = _upload_batch(vb)
        for roles in ((0, 1, 2), (0,)):
            if roles == (0,):
                b.weight = b.bg_weight = None
            outs = [_Placed(n * V * 4, k + 1) if k in roles else None for k in range(3)]
            torch.cuda.synchronize()
            _lib.check(lib.ursn_voxels_to_dense_sym(ctypes.byref(b), nd, _i32(*spatial), _i32(*codes),
                                                    *([ctypes.c_void_p(o.ptr) if o else None for o in outs] + [None])))
            torch.cuda.synchronize()
            for k in roles:
                outs[k].check_surroundings()
                want = S.apply_batch(plain[k].reshape((n,) + spatial), spatial, codes).reshape(n, V)
                assert same_bits(outs[k].f32((n, V)), want), (spatial, codes, k)
        # the identity is the plain expansion
        b, keep = _upload_batch(vb)
        b.weight = b.bg_weight = None
        out = _Placed(n * V * 4, 0)
        _lib.check(lib.ursn_voxels_to_dense_sym(ctypes.byref(b), nd, _i32(*spatial), _i32(*([0] * n)), ctypes.c_void_p(out.ptr), None,
                                                None, None))
        torch.cuda.synchronize()
        assert same_bits(out.f32((n, V)), plain[0])


@pytest.mark.parametrize("spatial", VOX_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_voxel_index_sym_finds_the_list_in_the_transformed_volume(lib, spatial):
    import torch
    vb = _events(spatial, 5)
    n, V, nd = vb.n, vb.voxels, len(spatial)
    pool = S.group("cube", spatial)
    codes = [pool[-1], pool[len(pool) // 2], pool[1], pool[-2]]
    # two entries outside [0, V): skipped by the scatter, passed through by the remap
    index = vb.index.copy()
    M = index.shape[0]
    index[[1, M - 2]] = [V + 5, -1]
    b, keep = _upload_batch(vb, index)
    b.weight = b.bg_weight = None
    dense = _Placed(n * V * 4, 0)
    remapped = _Placed(M * 4, 1)
    torch.cuda.synchronize()
    _lib.check(lib.ursn_voxels_to_dense_sym(ctypes.byref(b), nd, _i32(*spatial), _i32(*codes), ctypes.c_void_p(dense.ptr), None, None,
                                            None))
    _lib.check(lib.ursn_voxel_index_sym(nd, _i32(*spatial), n, _i32(*codes), ctypes.c_void_p(keep['offsets'].data_ptr()),
                                        ctypes.c_void_p(keep['index'].data_ptr()), ctypes.c_void_p(remapped.ptr), None))
    torch.cuda.synchronize()
    dense.check_surroundings()
    remapped.check_surroundings()
    vol = dense.f32((n, V))
    out = remapped.view.cpu().numpy().view(np.int32).copy()
    assert np.array_equal(keep['index'].cpu().numpy(), index), "the input list was written"
    assert out[1] == V + 5 and out[M - 2] == -1
    ok = np.ones(M, bool)
    ok[[1, M - 2]] = False
    for e in range(n):
        a, z = int(vb.offsets[e]), int(vb.offsets[e + 1])
        sel = np.arange(a, z)[ok[a:z]]
        # where numpy's transform puts voxel i: the position of i in the transformed arange volume
        where = np.argsort(S.apply_numpy(np.arange(V, dtype=np.int64).reshape(spatial), spatial, codes[e]).reshape(-1))
        assert np.array_equal(out[sel], where[index[sel]]), (spatial, e)
        assert len(set(out[sel].tolist())) == len(sel)
        assert same_bits(vol[e][out[sel]], vb.value[sel]), "gathering the transformed volume at index_out gives the value list"


def _far_corner_lists(spatial, n, seed):
    """n events: the corners of the volume, entries on every far face and random ones; two entries of event 0 outside [0, V)."""
    rng = np.random.default_rng(seed)
    nd, top = len(spatial), np.array(spatial, np.int64) - 1
    corners = np.array([[top[a] if (k >> a) & 1 else 0 for a in range(nd)] for k in range(1 << nd)], np.int64)
    lists = []
    for e in range(n):
        x = rng.integers(0, top + 1, (40 + 8 * nd, nd))
        for a in range(nd):
            x[40 + 8 * a:48 + 8 * a, a] = top[a]                             # on the far face of axis a
        lists.append(np.unique(np.concatenate([far.ravel(corners, spatial), far.ravel(x, spatial)])))
    off = np.concatenate([[0], np.cumsum([a.size for a in lists])]).astype(np.int64)
    index = np.concatenate(lists)
    V = far.volume(spatial)
    index[[1, int(off[1]) - 2]] = [V + 5, -1]
    return off, index.astype(np.int32)


@pytest.mark.parametrize("spatial", [far.CUBE, far.WIDEST_2D], ids=far.shape_id)
def test_voxel_index_sym_at_the_largest_extents(lib, spatial):
    """Every code, one event each, in a cube of 1290^3 and in 46340^2 voxels (just under 2^31; no dense volume of that size can be
    made): the expected values are the closed form o[a] = f_a(i[P[a]]) in Python integers (tests/_far_corner.py, proved equal to
    apply_numpy on small cubes in tests/test_far_corner_host.py).  The inverse code takes the remapped list back."""
    import torch
    nd, V = len(spatial), far.volume(spatial)
    codes = [int(c) for c in S.group("cube", spatial)]
    n = len(codes)
    assert n == S.count(nd) == (48 if nd == 3 else 8) and V > 2 ** 31 - 2 ** 20
    off, index = _far_corner_lists(spatial, n, 17 + nd)
    M = index.size
    d_off, d_idx = torch.from_numpy(off).cuda(), torch.from_numpy(index).cuda()
    remapped, back = _Placed(M * 4, 1), _Placed(M * 4, 3)
    inverse = [S.inverse(nd, c) for c in codes]
    assert all(S.compose(nd, c, i) == 0 and S.compose(nd, i, c) == 0 for c, i in zip(codes, inverse))
    torch.cuda.synchronize()
    _lib.check(lib.ursn_voxel_index_sym(nd, _i32(*spatial), n, _i32(*codes), ctypes.c_void_p(d_off.data_ptr()),
                                        ctypes.c_void_p(d_idx.data_ptr()), ctypes.c_void_p(remapped.ptr), None))
    _lib.check(lib.ursn_voxel_index_sym(nd, _i32(*spatial), n, _i32(*inverse), ctypes.c_void_p(d_off.data_ptr()),
                                        ctypes.c_void_p(remapped.ptr), ctypes.c_void_p(back.ptr), None))
    torch.cuda.synchronize()
    remapped.check_surroundings(), back.check_surroundings()
    out = remapped.view.cpu().numpy().view(np.int32).copy()
    assert np.array_equal(d_idx.cpu().numpy(), index), "the input list was written"
    assert out[1] == V + 5 and out[off[1] - 2] == -1
    top = far.ravel([[s - 1 for s in spatial]], spatial)[0]
    for e, c in enumerate(codes):
        a, z = int(off[e]), int(off[e + 1])
        want = far.remap_closed_form(index[a:z], spatial, S.perms(nd)[c >> nd], [(c >> k) & 1 for k in range(nd)])
        assert np.array_equal(out[a:z], want), (spatial, c)
        assert {0, int(top)} <= set(index[a:z].tolist()) and int(want[want < V].max()) == top   # the corners map to corners
    assert np.array_equal(back.view.cpu().numpy().view(np.int32), index), "the inverse code does not take the list back"


# ---- refusals: non-zero, outputs untouched ----------------------------------------------------------------------------------
def test_refusals_leave_the_outputs_untouched(lib):
    import torch
    spatial, n = (4, 6, 6), 2
    x = _bits((n,) + spatial + (1,), 1)
    src, dst = _Placed(x.nbytes, 0, x), _Placed(x.nbytes, 0)
    P = lambda p: ctypes.c_void_p(p.ptr) if p is not None else None

    def apply(text, sp=spatial, nn=n, codes=(0, 0), s=src, d=dst, fn="apply"):
        desc, keep = _desc(sp, nn, 1, codes)
        if fn == "apply":
            rc = lib.ursn_sym_apply(ctypes.byref(desc), P(s), P(d), None, None, None, None, None)
        else:
            rc = lib.ursn_sym_accumulate(ctypes.byref(desc), P(s), P(d), 0, 1.0, None)
        torch.cuda.synchronize()
        assert rc != 0 and text in lib.ursn_last_error(), (rc, lib.ursn_last_error())
        assert dst.untouched() and same_bits(src.f32(x.shape), x)
    for fn in ("apply", "accumulate"):
        apply(b"permutes axes of unequal size", codes=(0, 16), fn=fn)         # (1,0,2) on (4,6,6)
        apply(b"ops[0] = 48 outside [0, 48)", codes=(48, 0), fn=fn)
        apply(b"n = 1025 outside [1, 1024]", sp=(1, 1, 1), nn=1025, codes=(0,) * 1025, fn=fn)
        apply(b"null first src / dst", s=None, fn=fn)
        apply(b"null first src / dst", d=None, fn=fn)
    desc, keep = _desc(spatial, n, 1, (0, 0))
    for off in (0, 4, x.nbytes - 4):
        rc = lib.ursn_sym_apply(ctypes.byref(desc), P(src), ctypes.c_void_p(src.ptr + off), None, None, None, None, None)
        assert rc != 0 and b"dst0 overlaps src0" in lib.ursn_last_error()
    rc = lib.ursn_sym_apply(ctypes.byref(desc), P(src), P(dst), P(src), None, None, None, None)
    assert rc != 0 and b"src1 and dst1 must come together" in lib.ursn_last_error()
    torch.cuda.synchronize()
    assert dst.untouched() and same_bits(src.f32(x.shape), x)

    vb = _events((5, 5, 5), 2)
    b, keep = _upload_batch(vb)
    out = _Placed(vb.n * vb.voxels * 4, 0)
    for text, kw in ((b"prod(spatial) = 150", dict(sp=(5, 5, 6))), (b"ops[2] = 48 outside", dict(codes=(0, 0, 48, 0))),
                     (b"permutes axes of unequal size", dict(sp=(5, 25), nd=2, codes=(0, 0, 4, 0))), (b"null batch or data", dict(data=None))):
        sp = kw.get("sp", (5, 5, 5))
        rc = lib.ursn_voxels_to_dense_sym(ctypes.byref(b), kw.get("nd", 3), _i32(*sp), _i32(*kw.get("codes", (0, 0, 0, 0))),
                                          P(out) if "data" not in kw else None, None, None, None)
        torch.cuda.synchronize()
        assert rc != 0 and text in lib.ursn_last_error(), (rc, lib.ursn_last_error())
        assert out.untouched()
    rc = lib.ursn_voxel_index_sym(3, _i32(5, 5, 5), vb.n, _i32(0, 0, 16, 99), ctypes.c_void_p(keep['offsets'].data_ptr()),
                                  ctypes.c_void_p(keep['index'].data_ptr()), P(out), None)
    torch.cuda.synchronize()
    assert rc != 0 and b"ops[3] = 99 outside" in lib.ursn_last_error() and out.untouched()


# ---- net level --------------------------------------------------------------------------------------------------------------
NET_CASES = [((16, 16, 16, 1), "fp32", (5, 43)), ((16, 16, 16, 1), "bf16", (5, 43)), ((32, 32, 1), "fp32", (3, 6)), ((32, 32, 1), "bf16", (3, 6))]
NET_IDS = ["%s_%s" % ("x".join(str(d) for d in c[0][:-1]), c[1]) for c in NET_CASES]
TTA_CODES = {3: [0, 13, 43], 2: [0, 5, 3]}
_nets, _inputs = {}, {}


def _net(dims, prec):
    """3 classes, base 8, num_strides 2.  One net per shape and precision serves every test: no test applies a gradient, and a
    call depends only on its inputs."""
    if (dims, prec) not in _nets:
        net = uresnet(dims=list(dims), num_class=3, base_num_outputs=8, num_strides=2)
        net.construct(trainable=True, use_weight=True, learning_rate=1e-3, seed=7, precision=prec)
        _nets[(dims, prec)] = net
    return _nets[(dims, prec)]


def _net_inputs(dims):
    """Two lartpc_sparse events with dyadic weights (their per-event sums are exact in any order), dense and as a VoxelBatch."""
    if dims not in _inputs:
        ev = [sio.lartpc_sparse(dims, 3, e) for e in range(2)]
        data, label = (np.stack([e[j] for e in ev]) for j in range(2))
        V = data.shape[1]
        w = (np.random.default_rng(21).integers(1, 4097, (2, V)).astype(np.float64) / 1024.0).astype(np.float32)
        bg = np.array([5.0 / 1024.0, 0.75], np.float32)
        w[(data == 0) & (label == 0)] = 0.0
        w += ((data == 0) & (label == 0)) * bg[:, None]
        vb = VoxelBatch.concat([sio.dense_to_voxels(data[i], label[i], w[i]) for i in range(2)]).validate()
        _inputs[dims] = (data, label, w, vb)
    return _inputs[dims]


def _flat(x, spatial, codes):
    return S.apply_batch(x.reshape((x.shape[0],) + spatial), spatial, codes).reshape(x.shape)


def _step(net, fn, *args, **kw):
    net.zero_gradients(None)
    res, _ = fn(None, *args, **kw)
    return res, net.get_gradients()


def _same_step(a, b):
    return a[0] == b[0] and all(same_bits(a[1][k], b[1][k]) for k in b[1])


@pytest.mark.parametrize("dims, prec, codes", NET_CASES, ids=NET_IDS)
def test_step_with_symmetry_equals_step_on_numpy_transformed_arrays(dims, prec, codes):
    import torch
    net, spatial = _net(dims, prec), tuple(dims[:-1])
    data, label, w, vb = _net_inputs(dims)
    tdata, tlabel, tw = (_flat(a, spatial, codes) for a in (data, label, w))
    keep = [a.copy() for a in (data, label, w)]
    for norm in (False, True):
        ref = _step(net, net.accum_gradients, tdata, tlabel, tw, normalize_weight=norm)
        assert np.isfinite(ref[0][1:]).all() and ref[0][1] > 0
        got = _step(net, net.accum_gradients, data, label, w, normalize_weight=norm, symmetry=codes)
        assert _same_step(got, ref), (norm, got[0], ref[0])
        last = net.last_feed()
        assert same_bits(last['input_data'].cpu().numpy(), tdata) and same_bits(last['input_label'].cpu().numpy(), tlabel)
        if not norm:
            assert same_bits(last['input_weight'].cpu().numpy(), tw)
        got = _step(net, net.accum_gradients_voxels, vb, normalize_weight=norm, symmetry=codes)
        assert _same_step(got, ref), ("voxels", norm, got[0], ref[0])
        # caller-owned device tensors go through _feed unchanged and are never written
        dev = [torch.from_numpy(a).cuda() for a in (data, label, w)]
        got = _step(net, net.accum_gradients, *dev, normalize_weight=norm, symmetry=codes)
        assert _same_step(got, ref)
        assert all(same_bits(t.cpu().numpy(), a) for t, a in zip(dev, keep))
    assert all(same_bits(a, b) for a, b in zip((data, label, w), keep)), "a caller's host array was written"
    # the transformed step is another step, and None / the identity are the plain call
    plain = _step(net, net.accum_gradients, data, label, w)
    assert not _same_step(plain, ref)
    assert _same_step(_step(net, net.accum_gradients, data, label, w, symmetry=None), plain)
    assert _same_step(_step(net, net.accum_gradients, data, label, w, symmetry=[0, 0]), plain)
    assert _same_step(_step(net, net.accum_gradients_voxels, vb, symmetry=None), plain)
    assert _same_step(_step(net, net.accum_gradients_voxels, vb, symmetry=[0, 0]), plain)
    with pytest.raises(ValueError):
        net.accum_gradients(None, data, label, w, symmetry=[0])
    with pytest.raises(_lib.UrsnError):
        net.accum_gradients(None, data, label, w, symmetry=[0, S.count(len(spatial))])


@pytest.mark.parametrize("dims, prec, codes", NET_CASES, ids=NET_IDS)
def test_inference_tta_is_the_mean_of_the_back_mapped_softmaxes(dims, prec, codes):
    net, spatial = _net(dims, prec), tuple(dims[:-1])
    nd = len(spatial)
    data, label, w, vb = _net_inputs(dims)
    views = TTA_CODES[nd]
    terms = []
    for c in views:
        sm = net.inference(None, _flat(data, spatial, [c] * 2))[0]
        terms.append(S.apply_batch(sm, spatial, [S.inverse(nd, c)] * 2))
    for K in (1, 2, 3):
        want = _mean_formula(terms[:K])
        got = net.inference_tta(None, data, views[:K])
        assert got.shape == (2,) + spatial + (3,) and same_bits(got, want), K
    assert same_bits(net.inference_tta(None, data, views, as_numpy=False).cpu().numpy(), want)
    assert not same_bits(want, terms[0])

    # the voxel-list form: the same scores at the listed voxels, pred / ana by the rule on them
    r = net.inference_voxel_scores_tta(None, vb, views)
    off = vb.offsets
    for i in range(2):
        idx = vb.index[off[i]:off[i + 1]]
        sc = want[i].reshape(-1, 3)[idx]
        assert np.array_equal(r['index'][i], idx) and same_bits(r['scores'][i], sc)
        assert r['pred'][i].dtype == np.uint8 and np.array_equal(r['pred'][i], sc.argmax(axis=1))
        rule = ((sc[:, 1] > sc[:, 2]) * 1 + (sc[:, 2] >= sc[:, 1]) * 2) * (vb.value[off[i]:off[i + 1]] > 1.0)
        assert r['ana'][i].dtype == np.uint8 and np.array_equal(r['ana'][i], rule)
    one = net.inference_voxel_scores_tta(None, vb, [views[1]])
    plain = net.inference_voxel_scores(None, vb, with_labels=False)
    for i in range(2):
        idx = vb.index[off[i]:off[i + 1]]
        assert same_bits(one['scores'][i], terms[1][i].reshape(-1, 3)[idx])
        assert same_bits(net.inference_voxel_scores_tta(None, vb, [0])['scores'][i], plain['scores'][i])


# ---- driver -----------------------------------------------------------------------------------------------------------------
def _parent_run_minibatches(self, want_metrics):
    """ssnet_trainval._run_minibatches as it stood before AUGMENT: the accumulate calls are made without the keyword."""
    c, net = self._cfg, self._net
    rows = []
    norm = self._norm_kw()
    net.zero_gradients(self._sess)
    for _ in range(c.NUM_MINIBATCHES):
        if c.SPARSE_IO:
            res, doc = net.accum_gradients_voxels(self._sess, self._pull_voxels(self._input_main), fetch=want_metrics, **norm)
        else:
            data, label, weight = self._pull(self._input_main, c.KEYWORD_DATA, c.KEYWORD_LABEL, c.KEYWORD_WEIGHT)
            res, doc = net.accum_gradients(sess=self._sess, input_data=data, input_label=label, input_weight=weight,
                                           fetch=want_metrics, **norm)
        self._descr_metrics = doc[1:]
        if want_metrics:
            rows.append(res[1:])
        self._advance_main()
    self._last_minibatch = net.last_feed()
    net.apply_gradients(self._sess)
    return np.asarray(rows, np.float32) if want_metrics else None


def _driver_run(tmp_path, tag, sparse, augment, parent=False):
    from uresnet_amd.ssnet_trainval import ssnet_trainval
    inp = tmp_path / "input.cfg"
    inp.write_text("Dims [32, 32, 1]\nNumClass 3\nGenerator 'lartpc_sparse'\nNumEntries 32\n"
                   "Keys {'data': 'main_data', 'label': 'main_label', 'weight': 'main_weight'}\n")
    cfg = tmp_path / ("train_%s.cfg" % tag)
    cfg.write_text("NUM_CLASS 3\nBASE_NUM_FILTERS 4\nMAIN_INPUT_CONFIG '%s'\nLOGDIR ''\nSAVE_FILE ''\nITERATIONS 2\nMINIBATCH_SIZE 2\n"
                   "NUM_MINIBATCHES 2\nLEARNING_RATE 0.001\nTRAIN True\nUSE_WEIGHTS True\nREPORT_STEPS 1\nSUMMARY_STEPS 0\n"
                   "CHECKPOINT_STEPS 0\nKEYWORD_DATA 'main_data'\nKEYWORD_LABEL 'main_label'\nKEYWORD_WEIGHT 'main_weight'\n"
                   "SPARSE_IO %s\n%s" % (inp, sparse, "AUGMENT 'cube'\nAUGMENT_SEED 5\n" if augment else ""))
    t = ssnet_trainval()
    t.override_config(str(cfg))
    t.initialize()
    drawn = []
    if parent:
        t._run_minibatches = types.MethodType(_parent_run_minibatches, t)
    else:
        kw = t._sym_kw
        t._sym_kw = lambda mb, n: drawn.append(kw(mb, n)) or drawn[-1]
    for _ in range(2):
        t.train_step()
    weights = t._net.get_variables()
    t.reset()
    return weights, drawn


@pytest.mark.parametrize("sparse", [False, True], ids=["dense", "sparse_io"])
def test_driver_augment_is_reproducible_and_off_by_default(tmp_path, capsys, sparse):
    a, drawn_a = _driver_run(tmp_path, "a", sparse, True)
    b, drawn_b = _driver_run(tmp_path, "b", sparse, True)
    assert drawn_a == drawn_b and len(drawn_a) == 4
    ops = [d['symmetry'] for d in drawn_a]
    assert all(len(o) == 2 and set(o) <= set(range(8)) for o in ops) and len({tuple(o) for o in ops}) > 1
    assert ops == [S.draw(5, it, mb, 0, 2, list(range(8))) for it in (0, 1) for mb in (0, 1)]
    assert all(same_bits(a[k], b[k]) for k in a), "two runs from scratch with the same AUGMENT_SEED differ"
    off, drawn_off = _driver_run(tmp_path, "off", sparse, False)
    assert drawn_off == [{}] * 4
    parent, _ = _driver_run(tmp_path, "parent", sparse, False, parent=True)
    assert all(same_bits(off[k], parent[k]) for k in off), "the default config no longer trains like the parent's loop"
    assert not all(same_bits(a[k], off[k]) for k in a), "AUGMENT 'cube' changed nothing"
    capsys.readouterr()


def _ana_run(tmp_path, tag, sparse, tta):
    """Two interactive ana_step calls of the driver on 2-D events; returns their results, the bytes of the ANA_OUTPUT file and
    what inference_tta gives for the first batch with the driver's own net."""
    from uresnet_amd.ssnet_trainval import ssnet_trainval
    inp = tmp_path / "ana_input.cfg"
    inp.write_text("Dims [32, 32, 1]\nNumClass 3\nGenerator 'lartpc_sparse'\nNumEntries 32\n"
                   "Keys {'data': 'data', 'label': 'label', 'weight': 'weight'}\n")
    out = tmp_path / ("ssnet_%s.npy" % tag)
    cfg = tmp_path / ("ana_%s.cfg" % tag)
    cfg.write_text("NUM_CLASS 3\nBASE_NUM_FILTERS 4\nMAIN_INPUT_CONFIG '%s'\nANA_OUTPUT_CONFIG '%s'\nLOGDIR ''\nSAVE_FILE ''\n"
                   "ITERATIONS 2\nMINIBATCH_SIZE 2\nTRAIN False\nUSE_WEIGHTS False\nSUMMARY_STEPS 0\nCHECKPOINT_STEPS 0\n"
                   "SPARSE_IO %s\nSPARSE_SCORES %s\n%s" % (inp, out, sparse, sparse, "ANA_TTA %s\n" % tta if tta else ""))
    a = ssnet_trainval()
    a.override_config(str(cfg))
    a.initialize()
    res = [a.ana_step() for _ in range(2)]
    again = None
    if tta and not sparse:
        again = a._net.inference_tta(None, res[0]['input'].reshape(2, -1), tta)
    a.reset()
    return res, out.read_bytes(), again


@pytest.mark.parametrize("sparse", [False, True], ids=["dense", "sparse_io"])
def test_driver_ana_tta(tmp_path, capsys, sparse):
    """ANA_TTA [0] is the plain ana pass (same scores, same records, the accuracies of the head up to its fp32 rounding: they are
    ratios of counts below 2^24, so 2^-23 relative covers one rounding of the quotient); a list of views goes through the TTA
    methods."""
    plain, plain_bytes, _ = _ana_run(tmp_path, "plain", sparse, None)
    one, one_bytes, _ = _ana_run(tmp_path, "one", sparse, [0])
    assert one_bytes == plain_bytes and len(one_bytes) > 0
    for p, o in zip(plain, one):
        assert np.array_equal(p['entries'], o['entries'])
        assert abs(o['acc_nonzero'] - p['acc_nonzero']) <= 2.0 ** -23 * p['acc_nonzero']
        if sparse:
            assert o['acc_all'] is None
            for ev_p, ev_o in zip(p['voxels'], o['voxels']):
                assert same_bits(ev_p['scores'], ev_o['scores']) and np.array_equal(ev_p['pred'], ev_o['pred'])
        else:
            assert abs(o['acc_all'] - p['acc_all']) <= 2.0 ** -23 * p['acc_all']
            assert same_bits(o['softmax'], p['softmax'])
    views = [0, 5, 6]
    many, many_bytes, again = _ana_run(tmp_path, "many", sparse, views)
    assert len(many_bytes) > 0
    if sparse:
        assert not all(same_bits(a['scores'], b['scores']) for a, b in zip(many[0]['voxels'], plain[0]['voxels']))
    else:
        assert same_bits(many[0]['softmax'], again) and not same_bits(many[0]['softmax'], plain[0]['softmax'])
    capsys.readouterr()
