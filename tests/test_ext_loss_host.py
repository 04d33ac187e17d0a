"""External loss boundary, host side (no GPU): the five appended symbols under an unchanged ABI 9, the argument refusals of the
three op-level calls (include/uresnet_hip.h) and the Python surface on a net without device state.  Every call below is refused
on its arguments before any device access, so the pointers are never dereferenced."""
import ctypes

import numpy as np
import pytest

import uresnet_amd  # noqa: F401
from uresnet_amd import _lib

FAKE = 0x100000   # 16-byte aligned, never dereferenced
NEW = ("ursn_logits_dense", "ursn_dlogits_pack", "ursn_conv0_input_grad", "ursn_forward_logits", "ursn_backward_logits")


def _p(a):
    return ctypes.c_void_p(a)


def test_symbols_appended_under_abi_9(lib):
    assert _lib.ABI_VERSION == 9 and lib.ursn_abi_version() == 9
    for name in NEW:
        assert name in _lib.EXPORTS and hasattr(lib, name), name


def _refused(lib, rc, text):
    msg = lib.ursn_last_error()
    assert rc != 0 and msg and text in msg, (rc, msg, text)


def _desc(**kw):
    d = _lib.ursn_vscores_desc()
    d.n, d.voxels, d.ncls, d.z, d.z_cstride, d.dtype = 2, 64, 3, FAKE, 4, 0
    d.mean, d.rstd, d.beta = FAKE + 0x100, FAKE + 0x200, FAKE + 0x300
    for k, v in kw.items():
        setattr(d, k, v)
    return d


def test_logits_dense_refusals(lib):
    call = lambda d, out=FAKE + 0x10000: lib.ursn_logits_dense(ctypes.byref(d) if d is not None else None, _p(out), None)
    _refused(lib, call(None), b"null desc")
    _refused(lib, call(_desc(z=None)), b"null desc / z")
    _refused(lib, call(_desc(), out=None), b"logits_out")
    for ncls in (0, -1, 9):
        _refused(lib, call(_desc(ncls=ncls, z_cstride=16)), b"num_class %d not in [1,8]" % ncls)
    for vox in (0, -4):
        _refused(lib, call(_desc(voxels=vox)), b"voxels = %d < 1" % vox)
    _refused(lib, call(_desc(voxels=2 ** 31)), b">= 2^31")
    for n in (0, -2):
        _refused(lib, call(_desc(n=n)), b"n = %d outside" % n)
    _refused(lib, call(_desc(dtype=2)), b"dtype 2")
    _refused(lib, call(_desc(dtype=1, z_cstride=8, z=FAKE + 8)), b"bf16 z must be 16-byte aligned")
    _refused(lib, call(_desc(dtype=1, z_cstride=4)), b"bf16 z needs channel stride 8")
    _refused(lib, call(_desc(ncls=5, z_cstride=4)), b"z_cstride 4 < num_class 5")
    _refused(lib, call(_desc(z=FAKE + 2)), b"fp32 z must be 4-byte aligned")
    _refused(lib, call(_desc(rstd=None)), b"mean without rstd / beta")
    _refused(lib, call(_desc(), out=FAKE + 0x10002), b"logits_out must be 4-byte aligned")


def test_dlogits_pack_refusals(lib):
    def call(g=FAKE, n=2, voxels=64, ncls=3, out=FAKE + 0x10000, cs=4, dtype=0):
        return lib.ursn_dlogits_pack(_p(g), n, voxels, ncls, _p(out), cs, dtype, None)
    _refused(lib, call(g=None), b"null dlogits")
    _refused(lib, call(out=None), b"null dlogits / out")
    for ncls in (0, 9):
        _refused(lib, call(ncls=ncls, cs=16), b"num_class %d not in [1,8]" % ncls)
    _refused(lib, call(voxels=0), b"voxels = 0 < 1")
    _refused(lib, call(voxels=2 ** 31), b">= 2^31")
    _refused(lib, call(n=0), b"n = 0 outside")
    _refused(lib, call(dtype=3), b"dtype 3")
    _refused(lib, call(ncls=5, cs=4), b"out_cstride 4 < num_class 5")
    _refused(lib, call(ncls=3, cs=2), b"out_cstride 2 < num_class 3")
    _refused(lib, call(dtype=1, cs=8, out=FAKE + 0x10008), b"bf16 out must be 16-byte aligned")
    _refused(lib, call(dtype=1, cs=4), b"bf16 out needs channel stride 8")
    _refused(lib, call(g=FAKE + 1), b"dlogits must be 4-byte aligned")
    _refused(lib, call(out=FAKE + 0x10002), b"fp32 out must be 4-byte aligned")


def test_conv0_input_grad_refusals(lib):
    def call(ndim=3, sp=(8, 8, 8), n=2, cin=1, F=8, dz=FAKE, cs=8, dtype=0, w=FAKE + 0x100000, out=FAKE + 0x200000):
        arr = (ctypes.c_int32 * 3)(*sp) if sp is not None else None
        return lib.ursn_conv0_input_grad(ndim, arr, n, cin, F, _p(dz), cs, dtype, _p(w), _p(out), None)
    _refused(lib, call(sp=None), b"null spatial")
    _refused(lib, call(dz=None), b"null spatial / dz")
    _refused(lib, call(w=None), b"/ w")
    _refused(lib, call(out=None), b"dinput_out")
    _refused(lib, call(ndim=1), b"ndim 1 not in {2, 3}")
    _refused(lib, call(ndim=4), b"ndim 4 not in {2, 3}")
    _refused(lib, call(sp=(8, 0, 8)), b"spatial[1] = 0 < 1")
    _refused(lib, call(sp=(2048, 2048, 512)), b">= 2^31")
    _refused(lib, call(n=0), b"n = 0 outside")
    _refused(lib, call(cin=0), b"cin = 0")
    _refused(lib, call(F=0, cs=8), b"F = 0")
    _refused(lib, call(dtype=2), b"dtype 2")
    _refused(lib, call(F=8, cs=4), b"dz_cstride 4 < F 8")
    _refused(lib, call(dtype=1, cin=3), b"one input channel")
    _refused(lib, call(dtype=1, F=4, cs=8), b"multiples of 8")
    _refused(lib, call(dtype=1, F=8, cs=12), b"multiples of 8")
    _refused(lib, call(dtype=1, dz=FAKE + 8), b"bf16 dz must be 16-byte aligned")
    _refused(lib, call(dz=FAKE + 2), b"fp32 dz must be 4-byte aligned")
    _refused(lib, call(out=FAKE + 0x200001), b"4-byte aligned")


def test_net_level_refuse_null_handle(lib):
    rc = lib.ursn_forward_logits(None, _p(FAKE), 1, _p(FAKE + 0x1000), None)
    _refused(lib, rc, b"null handle")
    rc = lib.ursn_backward_logits(None, _p(FAKE), _p(FAKE + 0x1000), 1, None, None)
    _refused(lib, rc, b"null handle")


def test_python_methods_raise_without_a_trainable_net():
    import torch
    from uresnet_amd import uresnet
    from uresnet_amd.autograd import UResNetFunction
    net = uresnet(dims=[16, 16, 16, 1], num_class=3, base_num_outputs=4, num_strides=2)
    net.construct(trainable=False, use_weight=False, allocate=False)
    data = np.zeros((1, 16 ** 3), np.float32)
    with pytest.raises(RuntimeError, match="trainable=False"):
        net.forward_logits(None, data)
    with pytest.raises(RuntimeError, match="trainable=False"):
        net.backward_logits(None, np.zeros((1, 16, 16, 16, 3), np.float32))
    with pytest.raises(RuntimeError, match="trainable=False"):
        net.accum_gradients_custom(None, data, lambda z: z.sum())
    with pytest.raises(RuntimeError, match="trainable=False"):
        UResNetFunction.apply(net, None, torch.zeros(1, 16 ** 3))
    # a trainable net that was never allocated has no device state either
    net2 = uresnet(dims=[16, 16, 16, 1], num_class=3, base_num_outputs=4, num_strides=2)
    net2.construct(trainable=True, use_weight=False, allocate=False)
    with pytest.raises(RuntimeError):
        net2.backward_logits(None, np.zeros((1, 16, 16, 16, 3), np.float32))
