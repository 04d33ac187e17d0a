"""BatchNorm moving statistics, the part that needs no GPU: exported symbols, the size query, the bare op's refusals (all before
any device access), the numpy restatement of the update that the GPU tests hold the kernel to bit for bit, the driver keys, the
refusals of set_bn_moving and the checkpoint key names against the scopes of the reference's saved graph."""
import ctypes
import json
import os

import numpy as np
import pytest

from uresnet_amd import _lib, uresnet
from uresnet_amd.config import ssnet_config

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("ursn_bn_moving_size", "ursn_bn_attach", "ursn_bn_update", "ursn_bn_moving_update", "ursn_bn_set_frozen")


def bn_update_np(moving_mean, moving_var, mean, rstd, momentum, eps):
    """slim's assign_moving_average (no zero-debias) as ursn_bn_update evaluates it: every operation in float64, one rounding to
    float32 per element.  The batch variance is recovered from the stored fp32 rstd: v = max(1 / (rstd * rstd) - eps, 0) with
    eps the fp32 value the handle holds."""
    m, v = np.asarray(moving_mean, np.float32).astype(np.float64), np.asarray(moving_var, np.float32).astype(np.float64)
    x, r = np.asarray(mean, np.float32).astype(np.float64), np.asarray(rstd, np.float32).astype(np.float64)
    mu, e = np.float64(momentum), np.float64(np.float32(eps))
    bv = np.maximum(1.0 / (r * r) - e, 0.0)
    return (m - mu * (m - x)).astype(np.float32), (v - mu * (v - bv)).astype(np.float32)


def test_symbols_exported_under_abi_9():
    lib = _lib.load()
    assert _lib.ABI_VERSION == 9 and lib.ursn_abi_version() == 9
    hdr = open(os.path.join(ROOT, "include", "uresnet_hip.h")).read()
    assert "#define URSN_ABI_VERSION 9" in hdr
    for name in NEW:
        assert name in _lib.EXPORTS and hasattr(lib, name) and (name + "(") in hdr, name


@pytest.mark.parametrize("dims,base,ncls,ns,prec", [((32, 32, 1), 4, 3, 3, "fp32"), ((16, 16, 16, 1), 4, 3, 2, "fp32"),
                                                    ((32, 32, 32, 1), 8, 3, 5, "fp32"), ((32, 32, 32, 1), 8, 3, 5, "bf16"),
                                                    ((64, 64, 1), 6, 3, 3, "fp32"), ((192, 192, 192, 1), 16, 3, 5, "fp32")])
def test_size_query_is_twice_the_sum_of_cout(dims, base, ncls, ns, prec):
    lib = _lib.load()
    net = uresnet(dims=list(dims), num_class=ncls, base_num_outputs=base, num_strides=ns)
    net.construct(allocate=False, precision=prec)
    sizes, info, total = _lib.ursn_sizes(), _lib.ursn_layer_info(), ctypes.c_int64(-1)
    assert lib.ursn_query(ctypes.byref(net._cfg), ctypes.byref(sizes)) == 0
    want = 0
    for i in range(int(sizes.n_layers)):
        assert lib.ursn_query_layer(ctypes.byref(net._cfg), i, ctypes.byref(info)) == 0
        want += 2 * int(info.cout)
    assert lib.ursn_bn_moving_size(ctypes.byref(net._cfg), ctypes.byref(total)) == 0
    assert total.value == want == net._bn_size and want > 0
    if ns == 5:
        assert int(sizes.n_layers) == 58
    # the Python table tiles the buffer in the same order
    off = 0
    for name, c, at in net._bn_specs:
        assert at == off
        off += 2 * c
    assert off == want


def test_size_query_refusals():
    lib = _lib.load()
    total = ctypes.c_int64(0)
    assert lib.ursn_bn_moving_size(None, ctypes.byref(total)) != 0 and b"null" in lib.ursn_last_error()
    net = uresnet(dims=[32, 32, 1], num_class=3, base_num_outputs=4, num_strides=3)
    net.construct(allocate=False)
    assert lib.ursn_bn_moving_size(ctypes.byref(net._cfg), None) != 0
    cfg = net._native_config(1)
    cfg.spatial[0] = 36
    assert lib.ursn_bn_moving_size(ctypes.byref(cfg), ctypes.byref(total)) != 0 and b"divisible" in lib.ursn_last_error()


def test_bare_op_refusals_come_before_any_device_access():
    """The pointers below are host addresses (or plain integers): a call that touched them on a device, or launched, would
    fault or report a HIP error instead of the refusal's own text."""
    lib = _lib.load()
    buf = (ctypes.c_float * 8)()
    p = ctypes.cast(buf, ctypes.c_void_p)
    ok = dict(mean=p, rstd=p, mm=p, mv=p, count=8, momentum=0.5, eps=1e-3)

    def call(**kw):
        a = dict(ok, **kw)
        return lib.ursn_bn_moving_update(a["mean"], a["rstd"], a["mm"], a["mv"], a["count"], a["momentum"], a["eps"], None)

    for name in ("mean", "rstd", "mm", "mv"):
        assert call(**{name: None}) != 0 and b"null" in lib.ursn_last_error(), name
    for count in (0, -1, 2 ** 31):
        assert call(count=count) != 0 and b"count" in lib.ursn_last_error(), count
    for momentum in (-1e-9, 1.0 + 1e-9, float("nan"), float("inf")):
        assert call(momentum=momentum) != 0 and b"momentum" in lib.ursn_last_error(), momentum
    assert call(eps=0.0) != 0 and b"eps" in lib.ursn_last_error()
    assert call(mean=ctypes.c_void_p(p.value + 2)) != 0 and b"aligned" in lib.ursn_last_error()
    # the handle-level calls refuse a null handle
    assert lib.ursn_bn_attach(None, None) != 0 and lib.ursn_bn_update(None, 0.5, None) != 0 and lib.ursn_bn_set_frozen(None, 1) != 0


def test_numpy_restatement_against_a_hand_computed_case():
    eps = np.float32(1e-3)
    # rstd = 2 -> 1 / 4 - eps (eps as the fp32 value, in float64); rstd = 40 -> 1 / 1600 - eps < 0 -> 0
    mean, rstd = np.array([1.5, -2.0], np.float32), np.array([2.0, 40.0], np.float32)
    mm, mv = np.array([0.0, 1.0], np.float32), np.array([1.0, 0.5], np.float32)
    got_m, got_v = bn_update_np(mm, mv, mean, rstd, 0.25, 1e-3)
    bv0 = 0.25 - float(eps)
    want_m = np.array([0.0 - 0.25 * (0.0 - 1.5), 1.0 - 0.25 * (1.0 + 2.0)], np.float64)   # 0.375, 0.25
    want_v = np.array([1.0 - 0.25 * (1.0 - bv0), 0.5 - 0.25 * (0.5 - 0.0)], np.float64)
    assert got_m.dtype == got_v.dtype == np.float32
    assert np.array_equal(got_m, want_m.astype(np.float32)) and np.array_equal(got_m, np.array([0.375, 0.25], np.float32))
    assert np.array_equal(got_v, want_v.astype(np.float32)) and got_v[1] == np.float32(0.375)
    # momentum 1 replaces, momentum 0 keeps; from the initial 0 / 1 with momentum 1 the mean is taken over exactly
    a, b = bn_update_np(mm, mv, mean, rstd, 1.0, 1e-3)
    assert np.array_equal(a, mean) and b[1] == 0.0 and abs(float(b[0]) - bv0) < 1e-7
    a, b = bn_update_np(mm, mv, mean, rstd, 0.0, 1e-3)
    assert np.array_equal(a, mm) and np.array_equal(b, mv)
    # one rounding: the float64 result of a case whose float32 evaluation differs
    m1, x1 = np.array([1.0], np.float32), np.array([1.0 + 2.0 ** -23], np.float32)
    a, _ = bn_update_np(m1, m1, x1, np.array([1.0], np.float32), 1.0 / 3.0, 1e-3)
    assert a[0] == np.float32(1.0 - (1.0 / 3.0) * (1.0 - (1.0 + 2.0 ** -23)))


def test_config_keys_parsed_and_defaulted(tmp_path):
    c = ssnet_config()
    assert c.BN_MOVING is False and c.BN_DECAY == 0.999 and c.ANA_BN == 'batch'
    f = tmp_path / "a.cfg"
    f.write_text("BN_MOVING True\nBN_DECAY 0.99\nANA_BN 'moving'\n")
    c.override(str(f))
    assert c.BN_MOVING is True and c.BN_DECAY == 0.99 and c.ANA_BN == 'moving'
    assert ssnet_config().BN_MOVING is False                       # instance attributes: the class defaults stay
    for bad in ("ANA_BN 'frozen'\n", "BN_DECAY 1.5\n", "BN_DECAY -0.1\n", "BN_MOVING 1\n", "BN_DECAY 'x'\n", "ANA_BN 1\n"):
        f.write_text(bad)
        with pytest.raises(TypeError):
            ssnet_config().override(str(f))
    # the decay the reference's graph holds as 1 - decay (never used there: UPDATE_OPS never run)
    with open(os.path.join(ROOT, "tests", "golden", "ref_graph.json")) as g:
        G = json.load(g)
    assert G["moving_average_decay_constants"] == [0.001] and abs((1.0 - ssnet_config.BN_DECAY) - 0.001) < 1e-12
    assert G["batchnorm_variable_sets"] == [['beta', 'moving_mean', 'moving_variance']]


def test_key_names_follow_the_reference_scopes():
    with open(os.path.join(ROOT, "tests", "golden", "ref_graph.json")) as f:
        G = json.load(f)
    net = uresnet(dims=[512, 512, 1], num_class=3, base_num_outputs=16)
    net.construct(allocate=False)
    names = net.bn_moving_names()
    scopes = [c["scope"] for c in G["forward_convs"]]
    assert len(names) == 2 * 58 and len(scopes) >= 40
    for i, scope in enumerate(scopes):
        assert names[2 * i] == scope + "/BatchNorm/moving_mean" and names[2 * i + 1] == scope + "/BatchNorm/moving_variance"
    assert len(set(names)) == len(names) and not set(names) & set(net.variable_names())
    # the trainable-variable surface is what it was: 116 tensors, none of them a moving statistic
    assert len(net.variable_names()) == 116 and all(n.endswith(("/weights", "/BatchNorm/beta")) for n in net.variable_names())


def _net(bn_moving=True):
    net = uresnet(dims=[32, 32, 1], num_class=3, base_num_outputs=4, num_strides=3)
    net.construct(allocate=False, bn_moving=bn_moving)
    return net


def _values(net, fill_var=1.0):
    v = {}
    for name, c, _ in net._bn_specs:
        v[name + "/moving_mean"] = np.zeros(c, np.float32)
        v[name + "/moving_variance"] = np.full(c, fill_var, np.float32)
    return v


def test_set_bn_moving_refusals():
    """Validation is host work and comes first: names, shapes and values are refused before the buffer is looked for."""
    net = _net()
    good = _values(net)
    key_m, key_v = "UResNet/conv0/BatchNorm/moving_mean", "UResNet/conv2/BatchNorm/moving_variance"
    missing = dict(good)
    del missing[key_v]
    with pytest.raises(KeyError, match="conv2/BatchNorm/moving_variance"):
        net.set_bn_moving(missing)
    for key, arr in ((key_m, np.zeros(5, np.float32)), (key_v, np.ones((3, 1), np.float32)), (key_v, np.ones(4, np.float32))):
        with pytest.raises(ValueError, match="shape"):
            net.set_bn_moving(dict(good, **{key: arr}))
    for bad in (-1e-6, float("nan"), float("inf")):
        with pytest.raises(ValueError, match="negative or non-finite"):
            net.set_bn_moving(dict(good, **{key_v: np.array([1.0, bad, 1.0], np.float32)}))
    with pytest.raises(ValueError, match="non-finite"):
        net.set_bn_moving(dict(good, **{key_m: np.array([0.0, float("nan"), 0.0, 0.0], np.float32)}))
    with pytest.raises(ValueError, match="negative"):   # strict=False skips absent names, not bad values
        net.set_bn_moving({key_v: np.array([1.0, -1.0, 1.0], np.float32)}, strict=False)
    # everything valid: the only thing missing on this box is the buffer itself (allocate=False)
    with pytest.raises(RuntimeError, match="no moving statistics"):
        net.set_bn_moving(good)
    with pytest.raises(RuntimeError, match="no moving statistics"):
        net.get_bn_moving()


def test_mode_and_construct_arguments():
    net = _net(bn_moving=False)
    assert net.bn_mode() == 'batch' and net._bn_buf is None
    net.set_bn_mode('batch')
    with pytest.raises(ValueError):
        net.set_bn_mode('frozen')
    with pytest.raises(RuntimeError, match="no moving statistics"):   # frozen without a buffer
        net.set_bn_mode('moving')
    assert net.bn_mode() == 'batch'
    for bad in (-0.1, 1.1):
        with pytest.raises(ValueError, match="bn_decay"):
            uresnet(dims=[32, 32, 1], num_class=3, base_num_outputs=4, num_strides=3).construct(allocate=False, bn_decay=bad)
