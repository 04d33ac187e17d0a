"""Voxel-list scores, host side (no GPU): ABI 9, the SPARSE_SCORES flag, and the argument refusals of ursn_scores_at_voxels /
ursn_infer_voxels (include/uresnet_hip.h).  Every call below is refused on its arguments before any device access, so the
pointers are never dereferenced."""
import ctypes
import io
from contextlib import redirect_stdout

import pytest

import uresnet_amd  # noqa: F401
from uresnet_amd import _lib, ssnet_config

FAKE = 0x1000
P = ctypes.c_void_p(FAKE)


def test_abi_is_9(lib):
    assert _lib.ABI_VERSION == 9 and lib.ursn_abi_version() == 9
    assert "ursn_scores_at_voxels" in _lib.EXPORTS and "ursn_infer_voxels" in _lib.EXPORTS


def test_sparse_scores_flag(tmp_path):
    assert ssnet_config().SPARSE_SCORES is False
    p = tmp_path / "a.cfg"
    p.write_text("SPARSE_IO True\nSPARSE_SCORES True\n")
    c = ssnet_config()
    with redirect_stdout(io.StringIO()):
        c.override(str(p))
    assert c.SPARSE_SCORES is True and c.SPARSE_IO is True and ssnet_config().SPARSE_SCORES is False
    bad = tmp_path / "b.cfg"
    bad.write_text("SPARSE_SCORES 1\n")
    with redirect_stdout(io.StringIO()), pytest.raises(TypeError):
        ssnet_config().override(str(bad))


def _desc(**kw):
    d = _lib.ursn_vscores_desc()
    d.n, d.voxels, d.ncls = 1, 64, 3
    d.z, d.z_cstride, d.dtype = FAKE, 4, 0
    d.mean = d.rstd = d.beta = d.data = d.offsets = d.index = FAKE
    for k, v in kw.items():
        setattr(d, k, v)
    return d


def _refused(lib, d, outs, text):
    rc = lib.ursn_scores_at_voxels(ctypes.byref(d) if d is not None else None, outs[0], outs[1], outs[2], None)
    msg = lib.ursn_last_error()
    assert rc != 0 and text in msg, (rc, msg)


def test_scores_at_voxels_refusals(lib):
    all3 = (P, P, P)
    _refused(lib, None, all3, b"null desc")
    _refused(lib, _desc(offsets=None), all3, b"null desc / offsets")
    _refused(lib, _desc(index=None), all3, b"null")
    _refused(lib, _desc(), (None, None, None), b"all three outputs are null")
    _refused(lib, _desc(ncls=2), all3, b"needs >= 3 classes")
    _refused(lib, _desc(data=None), all3, b"needs data")
    _refused(lib, _desc(ncls=0), (P, None, None), b"num_class 0 not in [1,8]")
    _refused(lib, _desc(ncls=9, z_cstride=16), (P, None, None), b"num_class 9 not in [1,8]")
    _refused(lib, _desc(dtype=1, z_cstride=4), all3, b"bf16 logits need channel stride 8")
    _refused(lib, _desc(dtype=1, z_cstride=16, ncls=8), all3, b"bf16 logits need channel stride 8")
    _refused(lib, _desc(dtype=2), all3, b"dtype 2")
    _refused(lib, _desc(ncls=6, z_cstride=4), all3, b"z_cstride 4 < num_class 6")
    _refused(lib, _desc(n=0), all3, b"n = 0")
    _refused(lib, _desc(voxels=2 ** 31), all3, b"2^31")
    _refused(lib, _desc(rstd=None), all3, b"mean without rstd")


def test_infer_voxels_refusals(lib):
    acc = (ctypes.c_float * 2)()

    def call(net, data, offsets, index, m, outs):
        rc = lib.ursn_infer_voxels(net, data, None, 1, offsets, index, m, outs[0], outs[1], outs[2], acc, None)
        return rc, lib.ursn_last_error()

    rc, msg = call(None, P, None, P, 4, (P, P, P))
    assert rc != 0 and b"null offsets" in msg
    rc, msg = call(None, P, P, None, 4, (P, P, P))
    assert rc != 0 and b"null offsets / index" in msg
    rc, msg = call(None, P, P, P, 4, (None, None, None))
    assert rc != 0 and b"all three outputs are null" in msg
    rc, msg = call(None, P, P, P, -1, (P, P, P))
    assert rc != 0 and b"m_total = -1" in msg
    rc, msg = call(None, P, P, P, 4, (P, P, P))
    assert rc != 0 and b"null handle" in msg
