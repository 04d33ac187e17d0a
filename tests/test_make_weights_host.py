"""Loss weights made on the device, host side (no GPU): the two appended symbols under an unchanged ABI 9, the scratch query, the
argument refusals of ursn_make_weights (include/uresnet_hip.h), WeightSpec, the numpy statement of the definition
(uresnet_amd.weights.make_weights_numpy), the config keys and the make_weight keyword's refusals.  Every library call below is
refused on its arguments before any device access, so the fake pointers are never dereferenced."""
import ctypes
import inspect
import io
from contextlib import redirect_stdout

import numpy as np
import pytest

import uresnet_amd  # noqa: F401
from _abi import same_bits
from uresnet_amd import _lib, ssnet_config, symmetry, uresnet
from uresnet_amd import synthetic_io as sio
from uresnet_amd.ssnet import VoxelBatch
from uresnet_amd.weights import WeightSpec, make_weights_numpy

FAKE = 0x10000
TILE3, TILE2 = (8, 8, 64), (64, 64)      # the categorise pass's box tiles; test_make_weights_gpu.py pins them as well


def _p(a):
    return ctypes.c_void_p(a)


def _sp(*ext):
    return (ctypes.c_int32 * 3)(*(list(ext) + [1] * (3 - len(ext))))


def test_symbols_appended_under_abi_9(lib):
    assert _lib.ABI_VERSION == 9 and lib.ursn_abi_version() == 9
    for name in ("ursn_make_weights", "ursn_make_weights_scratch_bytes"):
        assert name in _lib.EXPORTS and hasattr(lib, name)


def _tiles(sp):
    tile = TILE3 if len(sp) == 3 else TILE2
    return int(np.prod([-(-s // t) for s, t in zip(sp, tile)]))


def _want_scratch(sp, n):
    return (n * int(np.prod(sp)) + 15) // 16 * 16 + n * _tiles(sp) * 64 + n * 64


def test_scratch_query(lib):
    q = lib.ursn_make_weights_scratch_bytes
    for sp in ((1, 1, 1), (8, 8, 64), (9, 8, 64), (8, 9, 64), (8, 8, 65), (192, 192, 192), (1, 1), (64, 64), (65, 64), (64, 65)):
        for n in (1, 3, 65535):
            assert q(len(sp), _sp(*sp), n, 3, 2) == _want_scratch(sp, n) > 0, (sp, n)
    # monotone in n and in every extent; independent of the radius and the class count inside the domain
    for nd, base in ((3, [5, 9, 70]), (2, [33, 65])):
        last = 0
        for n in (1, 2, 3, 100, 65535):
            got = q(nd, _sp(*base), n, 3, 1)
            assert got > last
            last = got
        for ax in range(nd):
            last = 0
            for ext in (1, 7, 8, 9, 63, 64, 65, 200):
                sp = list(base)
                sp[ax] = ext
                got = q(nd, _sp(*sp), 2, 3, 1)
                assert got > last, (sp, got, last)
                last = got
        assert len({q(nd, _sp(*base), 2, c, r) for c in range(1, 9) for r in range(4)}) == 1
    bad = [(1, (4, 4, 4), 1, 3, 0), (4, (4, 4, 4), 1, 3, 0), (3, (0, 4, 4), 1, 3, 0), (3, (4, -1, 4), 1, 3, 0), (2, (4, 0), 1, 3, 0),
           (3, (2048, 1024, 1024), 1, 3, 0), (2, (65536, 32768), 1, 3, 0), (3, (4, 4, 4), 0, 3, 0), (3, (4, 4, 4), -1, 3, 0),
           (3, (4, 4, 4), 65536, 3, 0), (3, (4, 4, 4), 1, 0, 0), (3, (4, 4, 4), 1, 9, 0), (3, (4, 4, 4), 1, 3, -1),
           (3, (4, 4, 4), 1, 3, 4)]
    for nd, sp, n, c, r in bad:
        assert q(nd, _sp(*sp), n, c, r) == 0, (nd, sp, n, c, r)
    assert q(3, None, 1, 3, 0) == 0
    assert q(3, _sp(2047, 1024, 1024), 1, 3, 0) > 0 and q(2, _sp(65535, 32768), 1, 3, 0) > 0     # just below 2^31 voxels


def _desc(ndim=3, spatial=(4, 4, 4), n=2, voxels=None, ncls=3, radius=1, mode=1, scale=None):
    d = _lib.ursn_make_weights_desc()
    d.ndim, d.n, d.ncls, d.radius, d.mode = ndim, n, ncls, radius, mode
    for i, s in enumerate(spatial):
        d.spatial[i] = s
    d.voxels = int(np.prod(spatial[:ndim])) if voxels is None else voxels
    for i in range(9):
        d.scale[i] = 1.0 if scale is None or i >= len(scale) else scale[i]
    return d


def _refused(lib, text, desc=None, label=FAKE, out=FAKE + 0x100000, counts=None, scratch=FAKE + 0x200000, sbytes=1 << 20, **kw):
    d = _desc(**kw) if desc is None else desc
    rc = lib.ursn_make_weights(ctypes.byref(d) if d != "null" else None, _p(label), _p(out), _p(counts), _p(scratch), sbytes, None)
    msg = lib.ursn_last_error()
    assert rc != 0 and text in msg, (rc, msg)


def test_make_weights_refusals(lib):
    _refused(lib, b"null desc", desc="null")
    _refused(lib, b"null desc / label", label=None)
    _refused(lib, b"null desc / label / weight_out", out=None)
    _refused(lib, b"null desc / label / weight_out / scratch", scratch=None)
    _refused(lib, b"n = 0 outside [1, 65535]", n=0)
    _refused(lib, b"n = -3 outside [1, 65535]", n=-3)
    _refused(lib, b"n = 65536 outside [1, 65535]", n=65536)
    _refused(lib, b"ndim = 1, must be 2 or 3", ndim=1, voxels=4)
    _refused(lib, b"ndim = 4, must be 2 or 3", ndim=4, voxels=64)
    _refused(lib, b"spatial[1] = 0 < 1", spatial=(4, 0, 4), voxels=16)
    _refused(lib, b"spatial[2] = -2 < 1", spatial=(4, 4, -2), voxels=16)
    _refused(lib, b"spatial[0] = 0 < 1", ndim=2, spatial=(0, 4), voxels=4)
    _refused(lib, b"prod(spatial) = 64 but voxels = 63", voxels=63)
    _refused(lib, b"prod(spatial) = 16 but voxels = 64", ndim=2, spatial=(4, 4, 4), voxels=64)     # 2-D ignores spatial[2]
    _refused(lib, b"prod(spatial) >= 2^31", spatial=(2048, 1024, 1024), voxels=2 ** 31)
    _refused(lib, b"prod(spatial) >= 2^31", ndim=2, spatial=(65536, 32768), voxels=2 ** 31)
    _refused(lib, b"ncls = 0 outside [1, 8]", ncls=0)
    _refused(lib, b"ncls = 9 outside [1, 8]", ncls=9)
    _refused(lib, b"radius = -1 outside [0, 3]", radius=-1)
    _refused(lib, b"radius = 4 outside [0, 3]", radius=4)
    _refused(lib, b"unknown mode 2", mode=2)
    _refused(lib, b"unknown mode -1", mode=-1)
    _refused(lib, b"scale[0] is not finite", scale=[float("nan")])
    _refused(lib, b"scale[3] is not finite", scale=[1, 1, 1, float("inf")])
    _refused(lib, b"scale[2] is not finite", scale=[1, 1, float("-inf")])
    d = _desc(scale=[1, 1, 1, 1, float("nan")])          # entries past ncls are not read
    _refused(lib, b"too small", desc=d, sbytes=0)
    _refused(lib, b"label / weight_out must be 4-byte aligned", label=FAKE + 2)
    _refused(lib, b"label / weight_out must be 4-byte aligned", out=FAKE + 0x100001)
    _refused(lib, b"scratch / counts_out must be 8-byte aligned", scratch=FAKE + 0x200004)
    _refused(lib, b"scratch / counts_out must be 8-byte aligned", counts=FAKE + 0x300004)
    need = _want_scratch((4, 4, 4), 2)
    _refused(lib, b"scratch of %d bytes is too small, %d needed" % (need - 1, need), sbytes=need - 1)
    _refused(lib, b"scratch of 0 bytes is too small", sbytes=0)
    # 2 x 64 floats = 512 bytes: one float apart, the last byte, and weight_out just below label all overlap, equal ones too
    _refused(lib, b"weight_out overlaps label", out=FAKE)
    _refused(lib, b"weight_out overlaps label", out=FAKE + 4)
    _refused(lib, b"weight_out overlaps label", out=FAKE + 508)
    _refused(lib, b"weight_out overlaps label", label=FAKE + 0x100, out=FAKE + 0x100 - 508)


def test_weight_spec_validation():
    s = WeightSpec()
    assert (s.mode, s.radius, s.scale) == ("invfreq", 0, None) and s.mode_code() == 1 and WeightSpec("class").mode_code() == 0
    assert same_bits(s.scales(3), np.ones(4, np.float32))
    assert same_bits(WeightSpec("class", 2, [1, 2, 3.5, 4]).scales(3), np.array([1, 2, 3.5, 4], np.float32))
    assert WeightSpec(radius=np.int64(3)).radius == 3
    for kw in (dict(mode="frequency"), dict(mode=1), dict(radius=-1), dict(radius=4), dict(radius=1.0), dict(radius=True),
               dict(radius="1"), dict(scale=[1.0]), dict(scale=[1.0] * 10), dict(scale=[1, float("nan")]),
               dict(scale=[1, float("inf"), 1]), dict(scale=3.0), dict(scale=["a", "b"])):
        with pytest.raises(ValueError):
            WeightSpec(**kw)
    with pytest.raises(ValueError):
        WeightSpec(scale=[1, 1, 1]).scales(3)            # 3 entries for 3 classes: num_class + 1 expected
    with pytest.raises(ValueError):
        WeightSpec(scale=[1, 1e39]).scales(1)            # finite as a double, infinite as the float32 the device reads
    for c in (0, 9):
        with pytest.raises(ValueError):
            WeightSpec().scales(c)


# ---- the numpy statement ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dims", [(16, 16, 16, 1), (32, 32, 1)], ids=["16x16x16", "32x32"])
def test_radius_0_invfreq_is_lartpc_sparse(dims):
    for entry in range(4):
        _, label, weight = sio.lartpc_sparse(dims, 3, entry)
        w, counts = make_weights_numpy(label[None], dims[:-1], 3, WeightSpec("invfreq", 0))
        assert same_bits(w[0], weight), entry
        assert counts[0, 3] == 0 and np.array_equal(counts[0, :3], np.bincount(label.astype(np.int64), minlength=3))


def _random_label(rng, n, sp, ncls, holes=True):
    lab = rng.integers(0, ncls, (n,) + tuple(sp)).astype(np.float32)
    lab *= rng.uniform(0, 1, lab.shape) < 0.5                       # half background
    lab += (rng.uniform(0, 0.9, lab.shape) * (lab > 0)).astype(np.float32)      # fractions truncate away
    if holes:
        bad = rng.uniform(0, 1, lab.shape)
        lab[bad < 0.03] = np.nan
        lab[(bad >= 0.03) & (bad < 0.05)] = -1.0
        lab[(bad >= 0.05) & (bad < 0.07)] = float(ncls)
    return lab.reshape(n, -1)


@pytest.mark.parametrize("sp", [(6, 6, 6), (9, 9)], ids=["cube", "square"])
def test_commutes_with_every_symmetry(sp):
    rng = np.random.default_rng(3)
    ncls = 4
    lab = _random_label(rng, 1, sp, ncls)[0]
    codes = symmetry.group("cube", sp)
    assert len(codes) == (48 if len(sp) == 3 else 8)
    scale = [0.5, 1.0, 2.0, 3.0, 7.0]
    for r in range(4):
        for mode in ("class", "invfreq"):
            spec = WeightSpec(mode, r, scale)
            w, counts = make_weights_numpy(lab[None], sp, ncls, spec)
            assert r == 0 or counts[0, ncls] > 0
            for code in codes:
                w2, c2 = make_weights_numpy(symmetry.apply_numpy(lab, sp, code)[None], sp, ncls, spec)
                assert np.array_equal(c2, counts)
                assert same_bits(w2[0], symmetry.apply_numpy(w[0], sp, code)), (r, mode, code)


@pytest.mark.parametrize("nd", [3, 2])
def test_pair_at_distance_r_is_boundary_and_at_r_plus_1_is_not(nd):
    sp = (9,) * nd
    for r in range(1, 4):
        directions = [tuple(int(a == b) for b in range(nd)) for a in range(nd)] + [(1,) * nd]
        for direction in directions:
            for dist, want in ((r, True), (r + 1, False)):
                lab = np.zeros(sp, np.float32)
                a = (1,) * nd
                b = tuple(1 + dist * s for s in direction)
                lab[a], lab[b] = 1.0, 2.0
                w, counts = make_weights_numpy(lab.reshape(1, -1), sp, 3, WeightSpec("class", r, [1, 2, 3, 9]))
                w = w.reshape(sp)
                V = 9 ** nd
                if want:
                    assert w[a] == 9 and w[b] == 9 and list(counts[0]) == [V - 2, 0, 0, 2], (r, direction, dist)
                else:
                    assert w[a] == 2 and w[b] == 3 and list(counts[0]) == [V - 2, 1, 1, 0], (r, direction, dist)
    # same class, background, none and out-of-range neighbours make no boundary; flat-index neighbours across a row end neither
    lab = np.zeros((1, 4, 5), np.float32) if nd == 3 else np.zeros((4, 5), np.float32)
    flat = lab.reshape(-1)
    flat[4], flat[5] = 1.0, 2.0                       # end of row 0, start of row 1
    _, counts = make_weights_numpy(flat[None], lab.shape, 3, WeightSpec("class", 1))
    assert counts[0, 3] == 0
    flat[:] = [1.0, np.nan, 1.0, 3.0, 1.0, -1.0, 1.0, 0.0, 1.0, 1.5] * 2
    _, counts = make_weights_numpy(flat[None], lab.shape, 3, WeightSpec("class", 3))
    assert list(counts[0]) == [2, 12, 0, 0]


def test_invfreq_rounds_one_fp64_division():
    lab = np.array([[0, 0, 0, 1, 1, 1, 1, 1, 1, 1, 2, 2, 2, 5, np.nan, 0.5]], np.float32)
    w, counts = make_weights_numpy(lab, (4, 4), 3, WeightSpec("invfreq", 0, [0.1, 0.3, 0.7, 1.0]))
    assert list(counts[0]) == [4, 7, 3, 0]
    s = np.array([0.1, 0.3, 0.7], np.float32).astype(np.float64)
    want = (s / np.array([4.0, 7.0, 3.0])).astype(np.float32)
    assert same_bits(w[0], np.array([want[0]] * 3 + [want[1]] * 7 + [want[2]] * 3 + [0, 0, want[0]], np.float32))


# ---- config keys and the keyword -------------------------------------------------------------------------------------------
def test_config_keys_default_off_and_dump(tmp_path):
    c = ssnet_config()
    assert (c.DEVICE_WEIGHTS, c.WEIGHT_RADIUS, c.WEIGHT_SCALE) == ("", 0, [])
    out = io.StringIO()
    with redirect_stdout(out):
        c.dump()
    for key in ("DEVICE_WEIGHTS", "WEIGHT_RADIUS", "WEIGHT_SCALE"):
        assert any(line.startswith(key + ".") for line in out.getvalue().split("\n")), key
    p = tmp_path / "a.cfg"
    p.write_text("DEVICE_WEIGHTS 'invfreq'\nWEIGHT_RADIUS 2\nWEIGHT_SCALE [1.0, 2.0, 2.0, 5]\n")
    with redirect_stdout(io.StringIO()):
        c.override(str(p))
    assert (c.DEVICE_WEIGHTS, c.WEIGHT_RADIUS, c.WEIGHT_SCALE) == ("invfreq", 2, [1.0, 2.0, 2.0, 5])
    assert ssnet_config().DEVICE_WEIGHTS == "" and ssnet_config().WEIGHT_SCALE == []
    for text in ("DEVICE_WEIGHTS 'balanced'\n", "DEVICE_WEIGHTS True\n", "WEIGHT_RADIUS 4\n", "WEIGHT_RADIUS -1\n",
                 "WEIGHT_RADIUS 1.0\n", "WEIGHT_SCALE 1.0\n", "WEIGHT_SCALE ['a']\n"):
        bad = tmp_path / "b.cfg"
        bad.write_text(text)
        with redirect_stdout(io.StringIO()), pytest.raises(TypeError):
            ssnet_config().override(str(bad))


def test_run_methods_take_make_weight():
    from uresnet_amd.ssnet import ssnet_base
    for name in ("accum_gradients", "run_test", "accum_gradients_voxels", "run_test_voxels"):
        assert inspect.signature(getattr(ssnet_base, name)).parameters["make_weight"].default is None, name
    assert list(inspect.signature(ssnet_base.make_weights).parameters) == ["self", "sess", "input_label", "spec", "as_numpy",
                                                                             "with_counts"]


def test_make_weight_with_a_given_weight_raises_before_any_device_use():
    """construct(allocate=False) never touches a device: whatever came after the refusal would raise something else."""
    dims = (16, 16, 16, 1)
    V = 16 ** 3
    data, label, weight = (np.zeros((1, V), np.float32) for _ in range(3))
    spec = WeightSpec()
    net = uresnet(dims=list(dims), num_class=3, base_num_outputs=4, num_strides=2)
    net.construct(trainable=True, use_weight=True, learning_rate=1e-3, allocate=False)
    vb = VoxelBatch([0, 1], [5], [2.0], [1.0], [0.5], [0.25], V)
    for call in (lambda: net.accum_gradients(None, data, label, weight, make_weight=spec),
                 lambda: net.accum_gradients(None, data, label, input_weight=weight, symmetry=[0], make_weight=spec),
                 lambda: net.run_test(None, data, label, weight, make_weight=spec),
                 lambda: net.accum_gradients_voxels(None, vb, make_weight=spec),
                 lambda: net.run_test_voxels(None, vb, make_weight=spec),
                 lambda: net.accum_gradients(None, data, label, make_weight="invfreq"),
                 lambda: net.accum_gradients(None, data, label, make_weight=WeightSpec(scale=[1, 1]))):
        with pytest.raises(ValueError):
            call()
    off = uresnet(dims=list(dims), num_class=3, base_num_outputs=4, num_strides=2)
    off.construct(trainable=True, use_weight=False, learning_rate=1e-3, allocate=False)
    for call in (lambda: off.accum_gradients(None, data, label, make_weight=spec),
                 lambda: off.run_test(None, data, label, make_weight=spec)):
        with pytest.raises(ValueError):
            call()
