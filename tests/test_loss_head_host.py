"""Device loss head, host side (no GPU): the appended symbols under an unchanged ABI 9, every argument refusal of ursn_loss_head
and of the net-level calls (each before any device access, so the fake pointers are never dereferenced), LossSpec validation, and
the oracle of the GPU tests checked three ways: the neutral spec against oracle.loss_and_metrics, the analytic gradient against
torch autograd over loss_torch in fp64, and central finite differences."""
import ctypes
import math

import numpy as np
import pytest
import torch

import uresnet_amd  # noqa: F401
from oracle import uresnet_np as O
from uresnet_amd import _lib
from uresnet_amd.config import ssnet_config
from uresnet_amd.losses import LossSpec, loss_numpy, loss_torch
from _loss_cases import CLASSES, SPEC_IDS, SPECS, make_case, rel_err

FAKE = 0x100000   # 16-byte aligned, never dereferenced
NEW = ("ursn_loss_head_scratch_bytes", "ursn_loss_head", "ursn_accum_step_loss", "ursn_eval_loss", "ursn_read_loss_terms")


def _p(a):
    return ctypes.c_void_p(a)


def test_symbols_appended_under_abi_9(lib):
    assert _lib.ABI_VERSION == 9 and lib.ursn_abi_version() == 9
    for name in NEW:
        assert name in _lib.EXPORTS and hasattr(lib, name), name
    C = ctypes
    P = C.c_void_p
    assert lib.ursn_loss_head.argtypes == [C.POINTER(_lib.ursn_vscores_desc), P, P, C.POINTER(_lib.ursn_loss_desc), P, C.c_int32,
                                           C.c_int32, P, C.c_int32, P, P, C.c_size_t, P]
    assert lib.ursn_loss_head_scratch_bytes.argtypes == [C.c_int32, C.c_int64, C.c_int32]
    assert lib.ursn_loss_head_scratch_bytes.restype == C.c_size_t
    assert lib.ursn_accum_step_loss.argtypes == [P, P, P, P, C.c_int32, C.POINTER(_lib.ursn_loss_desc), P]
    assert lib.ursn_eval_loss.argtypes == lib.ursn_accum_step_loss.argtypes
    assert lib.ursn_read_loss_terms.argtypes == [P, C.POINTER(C.c_float), P]
    assert [f[0] for f in _lib.ursn_loss_desc._fields_] == ["gamma", "smoothing", "dice_weight", "dice_eps", "ignore_label"]
    assert ctypes.sizeof(_lib.ursn_loss_desc) == 40


def test_scratch_bytes_domain(lib):
    f = lib.ursn_loss_head_scratch_bytes
    assert f(1, 1, 1) > 0 and f(1, 1, 1) % 8 == 0
    assert f(3, 4099, 3) >= f(1, 1, 3)
    for bad in ((0, 64, 3), (65536, 64, 3), (2, 0, 3), (2, 2 ** 31, 3), (2, 64, 0), (2, 64, 9)):
        assert f(*bad) == 0, bad


def _refused(lib, rc, text):
    msg = lib.ursn_last_error()
    assert rc != 0 and msg and text in msg, (rc, msg, text)


def _desc(**kw):
    d = _lib.ursn_vscores_desc()
    d.n, d.voxels, d.ncls, d.z, d.z_cstride, d.dtype = 2, 64, 3, FAKE, 4, 0
    d.mean, d.rstd, d.beta = FAKE + 0x100, FAKE + 0x200, FAKE + 0x300
    d.data = FAKE + 0x400
    for k, v in kw.items():
        setattr(d, k, v)
    return d


def _spec(gamma=0.0, smoothing=0.0, dice_weight=0.0, dice_eps=1.0, ignore_label=-1):
    return _lib.ursn_loss_desc(gamma, smoothing, dice_weight, dice_eps, ignore_label)


def test_loss_head_refusals(lib):
    need = lib.ursn_loss_head_scratch_bytes(2, 64, 3)

    def call(d=None, label=FAKE + 0x1000, weight=FAKE + 0x2000, spec=None, out=FAKE + 0x10000, cs=4, dt=0, bs=None, blocks=0,
             out8=FAKE + 0x3000, scratch=FAKE + 0x20000, sb=need, no_desc=False, no_spec=False):
        d = _desc() if d is None else d
        spec = _spec() if spec is None else spec
        return lib.ursn_loss_head(None if no_desc else ctypes.byref(d), _p(label), _p(weight), None if no_spec else ctypes.byref(spec),
                                  _p(out), cs, dt, _p(bs), blocks, _p(out8), _p(scratch), sb, None)
    # null arguments
    _refused(lib, call(no_desc=True), b"null desc")
    _refused(lib, call(no_spec=True), b"null desc / spec")
    _refused(lib, call(d=_desc(z=None)), b"null z")
    _refused(lib, call(label=None), b"label")
    _refused(lib, call(out8=None), b"out8")
    _refused(lib, call(scratch=None), b"scratch")
    _refused(lib, call(d=_desc(rstd=None)), b"mean without rstd / beta")
    # domain
    for ncls in (0, -1, 9):
        _refused(lib, call(d=_desc(ncls=ncls, z_cstride=16), cs=16), b"num_class %d not in [1,8]" % ncls)
    for n in (0, -2, 65536):
        _refused(lib, call(d=_desc(n=n)), b"n = %d outside" % n)
    for vox in (0, -4, 2 ** 31):
        _refused(lib, call(d=_desc(voxels=vox)), b"voxels = %d outside" % vox)
    _refused(lib, call(d=_desc(dtype=2)), b"dtype 2")
    _refused(lib, call(d=_desc(dtype=1, z_cstride=4)), b"bf16 z needs channel stride 8")
    _refused(lib, call(d=_desc(ncls=5, z_cstride=4), cs=8), b"z_cstride 4 < num_class 5")
    _refused(lib, call(dt=2), b"out_dtype 2")
    _refused(lib, call(cs=2), b"out_cstride 2 < num_class 3")
    _refused(lib, call(dt=1, cs=4), b"bf16 dlog_out needs channel stride 8")
    # the spec's ranges
    for g in (0.5, 0.999, 1e-9, -1.0, float("nan"), float("inf")):
        _refused(lib, call(spec=_spec(gamma=g)), b"the focal exponent must be 0 or >= 1")
    for s in (-0.1, 1.0, 2.0, float("nan")):
        _refused(lib, call(spec=_spec(smoothing=s)), b"smoothing")
    for w in (-1.0, float("nan"), float("inf")):
        _refused(lib, call(spec=_spec(dice_weight=w)), b"dice_weight")
    for e in (0.0, -1.0, float("nan"), float("inf")):
        _refused(lib, call(spec=_spec(dice_weight=1.0, dice_eps=e)), b"dice_eps")
    # alignment
    _refused(lib, call(d=_desc(z=FAKE + 2)), b"fp32 z must be 4-byte aligned")
    _refused(lib, call(d=_desc(dtype=1, z_cstride=8, z=FAKE + 8), dt=1, cs=8), b"bf16 z must be 16-byte aligned")
    _refused(lib, call(label=FAKE + 0x1002), b"4-byte aligned")
    _refused(lib, call(weight=FAKE + 0x2001), b"4-byte aligned")
    _refused(lib, call(d=_desc(data=FAKE + 0x402)), b"4-byte aligned")
    _refused(lib, call(out8=FAKE + 0x3002), b"4-byte aligned")
    _refused(lib, call(scratch=FAKE + 0x20004), b"scratch must be 8-byte aligned")
    _refused(lib, call(out=FAKE + 0x10002), b"fp32 dlog_out must be 4-byte aligned")
    _refused(lib, call(dt=1, cs=8, out=FAKE + 0x10008), b"bf16 dlog_out must be 16-byte aligned")
    # the BatchNorm-backward partials
    bs = FAKE + 0x40000
    _refused(lib, call(bs=bs, blocks=1, out=None), b"dlog_out is null")
    _refused(lib, call(bs=bs, blocks=1, d=_desc(mean=None, rstd=None, beta=None)), b"need mean / rstd")
    _refused(lib, call(bs=bs + 4, blocks=1), b"partials must be 8-byte aligned")
    _refused(lib, call(bs=bs, blocks=1, cs=8), b"4-padded layout")
    _refused(lib, call(bs=bs, blocks=1, dt=1, cs=8), b"bf16 z and bf16 dlog_out")
    _refused(lib, call(bs=bs, blocks=1, d=_desc(z_cstride=8)), b"4-padded layout")
    _refused(lib, call(bs=bs, blocks=2), b"2 partial blocks, the head's partition has 1")
    # scratch too small
    _refused(lib, call(sb=need - 8), b"scratch too small")
    _refused(lib, call(sb=0), b"scratch too small")


def test_net_level_refuse_null_handle(lib):
    sp = _spec()
    rc = lib.ursn_accum_step_loss(None, _p(FAKE), _p(FAKE), None, 1, ctypes.byref(sp), None)
    _refused(lib, rc, b"null handle")
    rc = lib.ursn_eval_loss(None, _p(FAKE), _p(FAKE), None, 1, ctypes.byref(sp), None)
    _refused(lib, rc, b"null handle")
    out = (ctypes.c_float * 2)()
    _refused(lib, lib.ursn_read_loss_terms(None, out, None), b"null argument")


def test_loss_spec_validation():
    s = LossSpec()
    assert (s.gamma, s.smoothing, s.dice_weight, s.dice_eps, s.ignore_label) == (0.0, 0.0, 0.0, 1.0, -1) and s.neutral
    assert not LossSpec(gamma=1.0).neutral and not LossSpec(ignore_label=0).neutral and not LossSpec(dice_weight=1e-3).neutral
    assert LossSpec(dice_eps=2.0).neutral   # eps alone changes nothing without a Dice term
    for kw in (dict(gamma=0.5), dict(gamma=1e-6), dict(gamma=-1), dict(gamma=float("inf")), dict(gamma=float("nan")),
               dict(smoothing=-0.01), dict(smoothing=1.0), dict(smoothing=float("nan")),
               dict(dice_weight=-1e-9), dict(dice_weight=float("inf")), dict(dice_weight=float("nan")),
               dict(dice_eps=0.0), dict(dice_eps=-1.0), dict(dice_eps=float("nan")),
               dict(ignore_label=1.5), dict(ignore_label="1"), dict(ignore_label=True), dict(ignore_label=2 ** 31)):
        with pytest.raises(ValueError):
            LossSpec(**kw)
    with pytest.raises(AttributeError):
        s.gamma = 2.0
    assert LossSpec(gamma=1, ignore_label=np.int64(255)).ignore_label == 255
    from uresnet_amd import uresnet
    net = uresnet(dims=[16, 16, 16, 1], num_class=3, base_num_outputs=4, num_strides=2)
    net.construct(trainable=True, use_weight=False, allocate=False)
    with pytest.raises(TypeError, match="LossSpec"):
        net._loss_desc({"gamma": 2.0})
    d = net._loss_desc(LossSpec(gamma=2.0, smoothing=0.1, dice_weight=0.5, dice_eps=0.25, ignore_label=7))
    assert (d.gamma, d.smoothing, d.dice_weight, d.dice_eps, d.ignore_label) == (2.0, 0.1, 0.5, 0.25, 7)


@pytest.mark.parametrize("use_w", [False, True])
@pytest.mark.parametrize("ncls", CLASSES)
def test_neutral_spec_is_the_oracles_head(ncls, use_w):
    """Inside the bounds tests/test_ops_gpu.py::test_softmax_ce_head holds the head to."""
    z, data, label, weight = make_case(10 + ncls, 3, 500, ncls)
    w = weight if use_w else None
    m = O.loss_and_metrics(z.astype(np.float64), data.astype(np.float64), label.astype(np.float64), None if w is None else w.astype(np.float64))
    r = loss_numpy(z, data, label, w, LossSpec())
    assert abs(r["loss"] - m["loss"]) <= 1e-5 * abs(m["loss"])   # one class: both are exactly 0
    assert r["ce_term"] == r["loss"] and r["dice_term"] == 0.0
    assert abs(r["acc_all"] - m["acc_all"]) < 1e-6
    assert abs(r["acc_nonzero"] - m["acc_nonzero"]) < 1e-6
    assert ncls == 1 or rel_err(r["dlogits"], m["dlogits"]) < 1e-5


@pytest.mark.parametrize("spec", [s[1] for s in SPECS], ids=SPEC_IDS)
def test_analytic_gradient_against_autograd(spec):
    worst = 0.0
    for ncls in CLASSES:
        for use_w in (False, True):
            z, data, label, weight = make_case(20 + ncls, 2, 257, ncls)
            w = weight if use_w else None
            r = loss_numpy(z, data, label, w, spec)
            zt = torch.tensor(z.astype(np.float64), requires_grad=True)
            loss = loss_torch(spec, label, w)(zt)
            loss.backward()
            g = zt.grad.numpy()
            assert abs(r["loss"] - float(loss)) <= 1e-12 * abs(float(loss)), (ncls, use_w)
            gmax = np.abs(g).max()
            if gmax == 0.0:
                assert np.abs(r["dlogits"]).max() == 0.0
                continue
            err = np.abs(r["dlogits"] - g).max() / gmax
            worst = max(worst, err)
            assert err <= 1e-10, (ncls, use_w, err)
    print("analytic against autograd, %s: worst %.3g of max" % (spec, worst))


@pytest.mark.parametrize("spec", [s[1] for s in SPECS] + [LossSpec(gamma=1.0), LossSpec(gamma=1.5, smoothing=0.05, dice_weight=2.0, dice_eps=0.5)],
                         ids=SPEC_IDS + ["focal1", "focal1.5_smooth_dice"])
def test_finite_differences(spec):
    ncls = 4
    z, data, label, weight = make_case(31, 2, 40, ncls)
    z = z.astype(np.float64)
    r = loss_numpy(z, data, label, weight, spec)
    h = 1e-5
    rng = np.random.default_rng(3)
    for _ in range(8):   # a handful of voxels, every class lane; not the gap-30 voxel (its derivative is below the difference's noise)
        i, v = int(rng.integers(0, 2)), int(rng.integers(0, 40))
        if (i, v) == (1, 20):
            v = 21
        for k in range(ncls):
            zp, zm = z.copy(), z.copy()
            zp[i, v, k] += h
            zm[i, v, k] -= h
            fd = (loss_numpy(zp, data, label, weight, spec)["loss"] - loss_numpy(zm, data, label, weight, spec)["loss"]) / (2 * h)
            assert abs(fd - r["dlogits"][i, v, k]) <= 1e-7 * max(1.0, np.abs(r["dlogits"]).max()), (i, v, k, fd, r["dlogits"][i, v, k])


def test_ignored_and_invalid_labels():
    z, data, label, weight = make_case(41, 2, 64, 3)
    spec = LossSpec(gamma=2.0, dice_weight=0.5, ignore_label=1)
    r = loss_numpy(z, data, label, weight, spec)
    assert np.abs(r["dlogits"][label == 1]).max() == 0.0 and np.abs(r["dlogits"][label != 1]).max() > 0
    lab2 = label.copy()
    lab2[0, 0] = 7.0   # outside [0, C) and not ignored
    assert math.isnan(loss_numpy(z, data, lab2, weight, spec)["loss"])
    assert math.isfinite(loss_numpy(z, data, lab2, weight, LossSpec(ignore_label=7))["loss"])
    # an ignored voxel still counts in the accuracies, as the head counts it
    a = loss_numpy(z, data, label, weight, LossSpec())
    assert r["acc_all"] == a["acc_all"] and r["acc_nonzero"] == a["acc_nonzero"]


def test_config_keys_parse_and_default_to_off(tmp_path):
    c = ssnet_config()
    assert (c.LOSS_FOCAL_GAMMA, c.LOSS_LABEL_SMOOTHING, c.LOSS_DICE_WEIGHT, c.LOSS_DICE_EPS, c.LOSS_IGNORE_LABEL) == (0., 0., 0., 1., -1)
    assert c.loss_spec() is None
    f = tmp_path / "loss.cfg"
    f.write_text("LOSS_FOCAL_GAMMA 2.\nLOSS_LABEL_SMOOTHING 0.1\nLOSS_DICE_WEIGHT 0.5\nLOSS_DICE_EPS 0.25\nLOSS_IGNORE_LABEL 0\n")
    c.override(str(f))
    s = c.loss_spec()
    assert (s.gamma, s.smoothing, s.dice_weight, s.dice_eps, s.ignore_label) == (2.0, 0.1, 0.5, 0.25, 0)
    for line in ("LOSS_FOCAL_GAMMA 0.5", "LOSS_FOCAL_GAMMA 2", "LOSS_LABEL_SMOOTHING 1.", "LOSS_DICE_WEIGHT -1.", "LOSS_DICE_EPS 0.",
                 "LOSS_IGNORE_LABEL 1."):
        f.write_text(line + "\n")
        with pytest.raises(TypeError):
            ssnet_config().override(str(f))
    d = ssnet_config()
    f.write_text("LOSS_DICE_EPS 2.\n")   # eps alone leaves the plan's head in place
    d.override(str(f))
    assert d.loss_spec() is None
