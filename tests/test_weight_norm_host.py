"""Per-event weight normalisation, host side (no GPU): the two appended symbols under an unchanged ABI 9, the scratch query, the
argument refusals of ursn_normalize_weights (include/uresnet_hip.h) and the DEVICE_WEIGHT_NORM flag.  Every call below is refused
on its arguments before any device access, so the pointers are never dereferenced."""
import ctypes
import io
from contextlib import redirect_stdout

import pytest

import uresnet_amd  # noqa: F401
from uresnet_amd import _lib, ssnet_config

FAKE = 0x10000
SPAN = 16384          # voxels per workgroup (WNORM_SPAN): one fp64 partial per event and span


def _p(a):
    return ctypes.c_void_p(a)


def test_symbols_appended_under_abi_9(lib):
    assert _lib.ABI_VERSION == 9 and lib.ursn_abi_version() == 9
    for name in ("ursn_normalize_weights", "ursn_normalize_weights_scratch_bytes"):
        assert name in _lib.EXPORTS and hasattr(lib, name)


def test_scratch_query(lib):
    q = lib.ursn_normalize_weights_scratch_bytes
    assert q(1, 1) == 8 and q(1, SPAN) == 8 and q(1, SPAN + 1) == 16 and q(3, 2 * SPAN + 7) == 3 * 3 * 8
    sizes = [1, 3, SPAN - 1, SPAN, SPAN + 1, 192 ** 3, 256 ** 3, 2 ** 31 - 1]
    for n in (1, 2, 4, 65535):
        got = [q(n, v) for v in sizes]
        assert all(g > 0 for g in got) and got == sorted(got)
        assert all(q(n, v) <= q(n + 1 if n < 65535 else n, v) for v in sizes)
    assert q(4, 192 ** 3) == 4 * -(-192 ** 3 // SPAN) * 8
    for n, v in ((0, 64), (-1, 64), (65536, 64), (1, 0), (1, -5), (1, 2 ** 31), (1, 2 ** 40)):
        assert q(n, v) == 0, (n, v)


def _refused(lib, text, weight=FAKE, out=FAKE + 0x100000, n=2, voxels=64, sums=None, scratch=FAKE + 0x200000, sbytes=1 << 20):
    rc = lib.ursn_normalize_weights(_p(weight), _p(out), n, voxels, _p(sums), _p(scratch), sbytes, None)
    msg = lib.ursn_last_error()
    assert rc != 0 and text in msg, (rc, msg)


def test_normalize_weights_refusals(lib):
    _refused(lib, b"null weight", weight=None)
    _refused(lib, b"null weight / out", out=None)
    _refused(lib, b"null weight / out / scratch", scratch=None)
    _refused(lib, b"n = 0 outside [1, 65535]", n=0)
    _refused(lib, b"n = -3 outside [1, 65535]", n=-3)
    _refused(lib, b"n = 65536 outside [1, 65535]", n=65536)
    _refused(lib, b"voxels = 0 < 1", voxels=0)
    _refused(lib, b"voxels = -1 < 1", voxels=-1)
    _refused(lib, b">= 2^31", voxels=2 ** 31)
    _refused(lib, b"scratch of 8 bytes is too small, 16 needed", sbytes=8)
    _refused(lib, b"scratch of 0 bytes is too small", sbytes=0)
    _refused(lib, b"too small, 24 needed", n=1, voxels=2 * SPAN + 1, out=FAKE + 0x1000000, sbytes=23)
    _refused(lib, b"scratch must be 8-byte aligned", scratch=FAKE + 0x200004)
    _refused(lib, b"4-byte aligned", weight=FAKE + 2)
    _refused(lib, b"4-byte aligned", out=FAKE + 0x100001)
    _refused(lib, b"4-byte aligned", sums=FAKE + 0x300002)
    # 2 x 64 floats = 512 bytes: one float apart, the last byte, and out just below weight all overlap; touching ranges do not
    _refused(lib, b"out overlaps weight", out=FAKE + 4)
    _refused(lib, b"out overlaps weight", out=FAKE + 508)
    _refused(lib, b"out overlaps weight", weight=FAKE + 0x100, out=FAKE + 0x100 - 508)


def test_device_weight_norm_flag(tmp_path):
    assert ssnet_config().DEVICE_WEIGHT_NORM is False
    p = tmp_path / "a.cfg"
    p.write_text("DEVICE_WEIGHT_NORM True\n")
    c = ssnet_config()
    with redirect_stdout(io.StringIO()):
        c.override(str(p))
    assert c.DEVICE_WEIGHT_NORM is True and ssnet_config().DEVICE_WEIGHT_NORM is False
    bad = tmp_path / "b.cfg"
    bad.write_text("DEVICE_WEIGHT_NORM 1\n")
    with redirect_stdout(io.StringIO()), pytest.raises(TypeError):
        ssnet_config().override(str(bad))


def test_run_methods_take_normalize_weight():
    """The keyword exists on every method the issue names and defaults to off."""
    import inspect
    from uresnet_amd.ssnet import ssnet_base
    for name in ("accum_gradients", "run_test", "make_summary", "accum_gradients_voxels", "run_test_voxels"):
        par = inspect.signature(getattr(ssnet_base, name)).parameters
        assert par["normalize_weight"].default is False, name
