"""Cube-symmetry codes, host side (no GPU): the numpy definition in uresnet_amd/symmetry.py against an explicit index-loop
restatement of o[a] = f_a(i[P[a]]), the group arithmetic against the C helpers of include/uresnet_hip.h, the per-minibatch draw,
the three config keys, and the argument refusals that return before any device access (the pointers are never dereferenced)."""
import ctypes
import inspect
import io
import itertools
from contextlib import redirect_stdout

import numpy as np
import pytest

import uresnet_amd  # noqa: F401
from uresnet_amd import _lib, ssnet_config
from uresnet_amd import symmetry as S

FAKE = 0x10000
PERMS = {3: [(0, 1, 2), (0, 2, 1), (1, 0, 2), (1, 2, 0), (2, 0, 1), (2, 1, 0)], 2: [(0, 1), (1, 0)]}


def _i32(*v):
    return (ctypes.c_int32 * len(v))(*v)


def index_loop(x, spatial, code):
    """The issue's second statement of an op, voxel by voxel: input voxel i lands at o with o[a] = f_a(i[P[a]])."""
    nd = len(spatial)
    P = PERMS[nd][code >> nd]
    out = np.empty_like(x)
    for i in itertools.product(*[range(s) for s in spatial]):
        o = tuple(spatial[a] - 1 - i[P[a]] if (code >> a) & 1 else i[P[a]] for a in range(nd))
        out[o] = x[i]
    return out


def test_symbols_appended_under_abi_9(lib):
    assert _lib.ABI_VERSION == 9 and lib.ursn_abi_version() == 9
    for name in ("ursn_sym_count", "ursn_sym_valid", "ursn_sym_inverse", "ursn_sym_compose", "ursn_sym_apply",
                 "ursn_sym_accumulate", "ursn_voxels_to_dense_sym", "ursn_voxel_index_sym"):
        assert name in _lib.EXPORTS and hasattr(lib, name), name


@pytest.mark.parametrize("spatial,channels", [((3, 3, 3), 2), ((3, 3), 0)])
def test_apply_numpy_is_the_index_loop(spatial, channels):
    shape = spatial + ((channels,) if channels else ())
    x = np.arange(int(np.prod(shape)), dtype=np.float32).reshape(shape) + 1.0   # distinct values
    nd = len(spatial)
    assert S.perms(nd) == PERMS[nd] and S.count(nd) == (48 if nd == 3 else 8)
    for code in range(S.count(nd)):
        got = S.apply_numpy(x, spatial, code)
        assert got.shape == x.shape and got.flags["C_CONTIGUOUS"]
        assert np.array_equal(got, index_loop(x, spatial, code)), code
    assert np.array_equal(S.apply_numpy(x, spatial, 0), x)


@pytest.mark.parametrize("nd", [2, 3])
def test_inverse_and_compose_agree_with_the_library(lib, nd):
    cnt = S.count(nd)
    assert lib.ursn_sym_count(nd) == cnt and lib.ursn_sym_count(1) == 0 and lib.ursn_sym_count(4) == 0
    spatial = (3,) * nd
    x = np.arange(3 ** nd * 2, dtype=np.float32).reshape(spatial + (2,))
    for a in range(cnt):
        inv = S.inverse(nd, a)
        assert lib.ursn_sym_inverse(nd, a) == inv
        assert S.compose(nd, a, inv) == 0 and S.compose(nd, inv, a) == 0
        assert np.array_equal(S.apply_numpy(S.apply_numpy(x, spatial, a), spatial, inv), x), a
        for b in range(cnt):
            c = S.compose(nd, a, b)
            assert lib.ursn_sym_compose(nd, a, b) == c, (a, b)
            assert np.array_equal(S.apply_numpy(S.apply_numpy(x, spatial, a), spatial, b), S.apply_numpy(x, spatial, c)), (a, b)
    for bad in (-1, cnt):
        assert lib.ursn_sym_inverse(nd, bad) == -1 and lib.ursn_sym_compose(nd, bad, 0) == -1 and lib.ursn_sym_compose(nd, 0, bad) == -1
        with pytest.raises(ValueError):
            S.inverse(nd, bad)


def test_valid_admits_exactly_the_equal_axis_permutations(lib):
    # (4,6,6): axes 1 and 2 may swap -> P in {(0,1,2), (0,2,1)}; (6,4,6): axes 0 and 2 -> {(0,1,2), (2,1,0)}; (5,9): no swap
    want = {(4, 6, 6): [k * 8 + f for k in (0, 1) for f in range(8)],
            (6, 4, 6): [k * 8 + f for k in (0, 5) for f in range(8)],
            (5, 9): [0, 1, 2, 3],
            (6, 6, 6): list(range(48)), (7, 7): list(range(8))}
    for spatial, codes in want.items():
        nd = len(spatial)
        assert [c for c in range(S.count(nd)) if S.valid(spatial, c)] == codes, spatial
        assert [c for c in range(S.count(nd)) if lib.ursn_sym_valid(nd, _i32(*spatial), c)] == codes, spatial
        assert S.group("cube", spatial) == codes and S.group("flip", spatial) == list(range(1 << nd)) and S.group("", spatial) == [0]
        for c in (-1, S.count(nd)):
            assert not S.valid(spatial, c) and not lib.ursn_sym_valid(nd, _i32(*spatial), c)
    with pytest.raises(ValueError):
        S.apply_numpy(np.zeros((4, 6, 6), np.float32), (4, 6, 6), 16)
    with pytest.raises(ValueError):
        S.group("rot", (4, 4, 4))


def test_draw_is_a_function_of_its_tuple():
    codes = S.group("cube", (6, 6, 6))
    a = S.draw(7, 3, 1, 0, 64, codes)
    before = np.random.get_state()
    np.random.random(5)                          # the global generator is neither read ...
    assert S.draw(7, 3, 1, 0, 64, codes) == a
    after = np.random.get_state()
    S.draw(7, 3, 1, 0, 64, codes)                # ... nor advanced
    assert np.array_equal(np.random.get_state()[1], after[1]) and np.random.get_state()[2] == after[2]
    np.random.set_state(before)
    assert len(a) == 64 and set(a) <= set(codes) and len(set(a)) > 8
    assert S.draw(7, 3, 1, 0, 16, codes) == a[:16]      # the batch size only cuts the stream
    others = [S.draw(8, 3, 1, 0, 64, codes), S.draw(7, 4, 1, 0, 64, codes), S.draw(7, 3, 2, 0, 64, codes), S.draw(7, 3, 1, 1, 64, codes)]
    for o in others:
        assert o != a
    assert len({tuple(o) for o in others}) == 4
    assert S.draw(7, 3, 1, 0, 5, [0]) == [0] * 5
    assert set(S.draw(1, 0, 0, 0, 200, [3, 9])) == {3, 9}


def test_config_keys_default_off_and_are_type_checked(tmp_path):
    c = ssnet_config()
    assert c.AUGMENT == "" and c.AUGMENT_SEED == 0 and c.ANA_TTA == []
    p = tmp_path / "a.cfg"
    p.write_text("AUGMENT 'cube'\nAUGMENT_SEED 11\nANA_TTA [0, 7, 47]\n")
    with redirect_stdout(io.StringIO()):
        c.override(str(p))
    assert (c.AUGMENT, c.AUGMENT_SEED, c.ANA_TTA) == ("cube", 11, [0, 7, 47])
    fresh = ssnet_config()
    assert fresh.AUGMENT == "" and fresh.AUGMENT_SEED == 0 and fresh.ANA_TTA == []
    for i, line in enumerate(("AUGMENT 'rot'", "AUGMENT 1", "AUGMENT True", "AUGMENT_SEED 'x'", "AUGMENT_SEED 1.5", "ANA_TTA 3",
                              "ANA_TTA (0, 1)", "ANA_TTA [0, 'a']", "ANA_TTA [48]", "ANA_TTA [-1]", "ANA_TTA [1.0]")):
        bad = tmp_path / ("b%d.cfg" % i)
        bad.write_text(line + "\n")
        with redirect_stdout(io.StringIO()), pytest.raises(TypeError):
            ssnet_config().override(str(bad))


def test_run_methods_take_symmetry():
    from uresnet_amd.ssnet import ssnet_base
    for name in ("accum_gradients", "accum_gradients_voxels"):
        assert inspect.signature(getattr(ssnet_base, name)).parameters["symmetry"].default is None, name
    assert list(inspect.signature(ssnet_base.inference_tta).parameters) == ["self", "sess", "input_data", "codes", "as_numpy"]
    assert list(inspect.signature(ssnet_base.inference_voxel_scores_tta).parameters) == ["self", "sess", "voxels", "codes"]


def test_ana_tta_is_refused_with_ana_csv():
    from uresnet_amd.ssnet_trainval import ssnet_trainval
    t = ssnet_trainval()
    t._cfg.TRAIN, t._cfg.ANA_TTA, t._cfg.ANA_CSV = False, [0, 1], "out.csv"
    with pytest.raises(ValueError, match="ONE forward pass"):
        t.initialize()


# ---- refusals that need no device -------------------------------------------------------------------------------------------
def _desc(spatial=(6, 6, 6), n=2, channels=1, ops=(0, 0)):
    d = _lib.ursn_sym_desc()
    d.ndim = len(spatial)
    for i, s in enumerate(spatial):
        d.spatial[i] = s
    d.n, d.channels = n, channels
    keep = _i32(*ops) if ops is not None else None
    d.ops = ctypes.cast(keep, ctypes.POINTER(ctypes.c_int32)) if keep is not None else None
    return d, keep


def _apply_refused(lib, text, d, ptrs=None):
    ptrs = [FAKE, FAKE + 0x100000, None, None, None, None] if ptrs is None else ptrs
    rc = lib.ursn_sym_apply(ctypes.byref(d) if d is not None else None, *([ctypes.c_void_p(p) for p in ptrs] + [None]))
    msg = lib.ursn_last_error()
    assert rc != 0 and text in msg, (rc, msg)


def test_sym_apply_refusals(lib):
    _apply_refused(lib, b"null desc", None)
    for kw, text in ((dict(spatial=(6,)), b"ndim = 1 not in {2, 3}"), (dict(n=0, ops=(0,)), b"n = 0 outside [1, 1024]"),
                     (dict(n=1025, ops=(0,) * 1025), b"n = 1025 outside [1, 1024]"), (dict(ops=None), b"null spatial / ops"),
                     (dict(spatial=(6, 0, 6)), b"spatial[1] = 0 < 1"), (dict(channels=0), b"channels = 0 outside [1, 8]"),
                     (dict(channels=9), b"channels = 9 outside [1, 8]"), (dict(ops=(0, 48)), b"ops[1] = 48 outside [0, 48)"),
                     (dict(ops=(-1, 0)), b"ops[0] = -1 outside [0, 48)"), (dict(spatial=(7, 7), ops=(0, 8)), b"ops[1] = 8 outside [0, 8)"),
                     (dict(spatial=(4, 6, 6), ops=(8, 16)), b"ops[1] = 16 permutes axes of unequal size"),
                     (dict(spatial=(5, 9), ops=(3, 4)), b"ops[1] = 4 permutes axes of unequal size"),
                     (dict(spatial=(2048, 2048, 512), n=1, ops=(0,)), b">= 2^31"),
                     (dict(spatial=(1024, 1024, 512), n=1, ops=(0,), channels=4), b"prod(spatial) * channels")):
        d, keep = _desc(**kw)
        _apply_refused(lib, text, d)
    d, keep = _desc()                            # 2 x 216 floats = 1728 bytes per tensor
    B = FAKE + 0x100000
    _apply_refused(lib, b"null first src / dst", d, [None, B, None, None, None, None])
    _apply_refused(lib, b"null first src / dst", d, [FAKE, None, None, None, None, None])
    _apply_refused(lib, b"src1 and dst1 must come together", d, [FAKE, B, FAKE + 0x2000, None, None, None])
    _apply_refused(lib, b"src2 and dst2 must come together", d, [FAKE, B, None, None, None, B + 0x2000])
    _apply_refused(lib, b"4-byte aligned", d, [FAKE + 2, B, None, None, None, None])
    _apply_refused(lib, b"4-byte aligned", d, [FAKE, B + 1, None, None, None, None])
    _apply_refused(lib, b"dst0 overlaps src0", d, [FAKE, FAKE, None, None, None, None])
    _apply_refused(lib, b"dst0 overlaps src0", d, [FAKE, FAKE + 1724, None, None, None, None])
    _apply_refused(lib, b"dst0 overlaps src0", d, [FAKE + 1724, FAKE, None, None, None, None])
    _apply_refused(lib, b"dst0 overlaps src1", d, [FAKE, B, B + 4, B + 0x4000, None, None])
    _apply_refused(lib, b"overlaps dst", d, [FAKE, B, FAKE + 0x2000, B + 1724, None, None])
    rc = lib.ursn_sym_accumulate(ctypes.byref(d), ctypes.c_void_p(FAKE), ctypes.c_void_p(FAKE + 8), 1, 1.0, None)
    assert rc != 0 and b"sym_accumulate: dst0 overlaps src0" in lib.ursn_last_error()
    rc = lib.ursn_sym_accumulate(ctypes.byref(d), ctypes.c_void_p(FAKE), None, 1, 1.0, None)
    assert rc != 0 and b"null first src / dst" in lib.ursn_last_error()


def test_voxel_sym_refusals(lib):
    b = _lib.ursn_voxel_batch()
    b.n, b.voxels = 2, 216
    b.offsets, b.index, b.value = FAKE, FAKE + 0x1000, FAKE + 0x2000
    out = ctypes.c_void_p(FAKE + 0x100000)

    def refused(text, batch=b, nd=3, spatial=(6, 6, 6), ops=(0, 0), data=out):
        rc = lib.ursn_voxels_to_dense_sym(ctypes.byref(batch) if batch is not None else None, nd, _i32(*spatial), _i32(*ops), data,
                                          None, None, None)
        msg = lib.ursn_last_error()
        assert rc != 0 and text in msg, (rc, msg)
    refused(b"null batch or data output", batch=None)
    refused(b"null batch or data output", data=None)
    refused(b"prod(spatial) = 252, the batch has 216 voxels", spatial=(6, 6, 7))
    refused(b"ops[1] = 48 outside", ops=(0, 48))
    refused(b"permutes axes of unequal size", spatial=(4, 6, 9), ops=(0, 8))
    refused(b"ndim = 4", nd=4)
    big = _lib.ursn_voxel_batch()
    big.n, big.voxels = 1025, 216
    big.offsets, big.index, big.value = FAKE, FAKE + 0x1000, FAKE + 0x2000
    refused(b"n = 1025 outside [1, 1024]", batch=big, ops=(0,) * 1025)
    nolist = _lib.ursn_voxel_batch()
    nolist.n, nolist.voxels = 2, 216
    refused(b"null offsets / index / value", batch=nolist)

    def irefused(text, nd=3, spatial=(6, 6, 6), n=2, ops=(0, 0), offsets=FAKE, index=FAKE + 0x1000, index_out=FAKE + 0x2000):
        rc = lib.ursn_voxel_index_sym(nd, _i32(*spatial), n, _i32(*ops), ctypes.c_void_p(offsets), ctypes.c_void_p(index),
                                      ctypes.c_void_p(index_out), None)
        msg = lib.ursn_last_error()
        assert rc != 0 and text in msg, (rc, msg)
    irefused(b"null offsets / index / index_out", offsets=None)
    irefused(b"null offsets / index / index_out", index_out=None)
    irefused(b"offsets 8-byte aligned", offsets=FAKE + 4)
    irefused(b"4-byte", index=FAKE + 0x1002)
    irefused(b"index_out must not be index", index_out=FAKE + 0x1000)
    irefused(b"n = 1025 outside", n=1025, ops=(0,) * 1025)
    irefused(b"ops[0] = 9 outside [0, 8)", nd=2, spatial=(5, 5), ops=(9, 0))
    irefused(b"permutes axes of unequal size", nd=2, spatial=(5, 9), ops=(0, 5))
