"""The model shapes both plans accept, queried on the host (ursn_query / ursn_query_layer: the plan is built for sizes only,
nothing runs): every configuration inside a plan's documented domain is accepted with the reference's parameter count and
layer table (oracle.uresnet_np.param_specs / layer_table, lib/uresnet.py:22-123), every one outside it is refused with a
message that names the reason, and construct() raises a Python exception for it.

Domains: fp32 (net.hip plan()): any input channel count >= 1, any base_num_outputs >= 1, 1..8 classes.  bf16 (net_bf16.hip
plan()): one input channel, base_num_outputs a multiple of 8, 1..8 classes."""
import ctypes
import itertools

import pytest

from oracle import uresnet_np as O
from uresnet_amd import _lib, uresnet

NDIMS = (2, 3)
CINS = (1, 2, 3, 4, 8)
WIDTHS = (1, 2, 3, 4, 6, 8, 12, 16, 24, 32)
CLASSES = (1, 2, 3, 4, 6, 7, 8, 9)
STRIDES = (1, 3, 5)
PRECS = ("fp32", "bf16")


def _config(ndim, cin, F, ncls, ns, prec, max_batch=2):
    cfg = _lib.ursn_config()
    cfg.ndim = ndim
    for i in range(3):
        cfg.spatial[i] = 32 if i < ndim else 1
    cfg.cin, cfg.base_filters, cfg.num_class, cfg.num_strides = cin, F, ncls, ns
    cfg.max_batch, cfg.trainable, cfg.use_weight, cfg.bn_eps = max_batch, 1, 1, 1e-3
    cfg.act_dtype = 1 if prec == "bf16" else 0
    return cfg


def _refusal(cin, F, ncls, prec):
    """None inside the documented domain, else a fragment the error message must contain (the plan's first failing check)."""
    if prec == "bf16" and cin != 1:
        return b"one input channel"
    if prec == "bf16" and F % 8:
        return b"multiple of 8"
    if ncls > 8:
        return b"num_class"
    return None


def _query(cfg):
    lib = _lib.load()
    s = _lib.ursn_sizes()
    rc = lib.ursn_query(ctypes.byref(cfg), ctypes.byref(s))
    return rc, s, lib.ursn_last_error()


@pytest.mark.parametrize("prec", PRECS)
@pytest.mark.parametrize("ndim", NDIMS)
def test_query_accepts_exactly_the_documented_domain(ndim, prec):
    lib = _lib.load()
    info = _lib.ursn_layer_info()
    n_ok = 0
    for cin, F, ncls, ns in itertools.product(CINS, WIDTHS, CLASSES, STRIDES):
        cfg = _config(ndim, cin, F, ncls, ns, prec)
        rc, s, err = _query(cfg)
        why = _refusal(cin, F, ncls, prec)
        case = (ndim, cin, F, ncls, ns, prec)
        if why is not None:
            assert rc != 0, case
            assert why in err, (case, err)
            continue
        assert rc == 0, (case, err)
        n_ok += 1
        specs = O.param_specs(ndim, cin, F, ncls, ns)
        assert s.n_params == sum(int(O.np.prod(sh)) for _, sh in specs), case
        table = O.layer_table(ndim, cin, F, ncls, ns)
        assert s.n_layers == len(table), case
        # the full per-layer table on the narrow widths and class counts (the paddings under test); the count above elsewhere
        if F in (1, 3, 6, 8, 24) and ncls in (1, 4, 7, 8) and cin in (1, 3, 8):
            for i, ref in enumerate(table):
                assert lib.ursn_query_layer(ctypes.byref(cfg), i, ctypes.byref(info)) == 0, (case, i, lib.ursn_last_error())
                got = ("deconv" if info.transposed else "conv", info.k, info.stride, info.cin, info.cout, info.name.decode())
                assert got == (ref["kind"], ref["k"], ref["stride"], ref["cin"], ref["cout"], ref["name"]), (case, got, ref)
            assert lib.ursn_query_layer(ctypes.byref(cfg), len(table), ctypes.byref(info)) != 0
    assert n_ok > 0


@pytest.mark.parametrize("dims,F,ncls,prec,why", [
    ((32, 32, 1), 8, 9, "fp32", "num_class"),
    ((32, 32, 1), 8, 9, "bf16", "num_class"),
    ((32, 32, 2), 8, 3, "bf16", "one input channel"),
    ((32, 32, 1), 12, 3, "bf16", "multiple of 8"),
])
def test_construct_raises_outside_the_domain(dims, F, ncls, prec, why):
    net = uresnet(dims=list(dims), num_class=ncls, base_num_outputs=F, num_strides=3)
    with pytest.raises(Exception, match=why):
        net.construct(trainable=True, use_weight=True, allocate=False, precision=prec)


@pytest.mark.parametrize("dims,F,ncls,prec", [
    ((32, 32, 8), 6, 7, "fp32"),
    ((16, 16, 16, 3), 1, 1, "fp32"),
    ((32, 32, 1), 24, 6, "bf16"),
])
def test_construct_accepts_inside_the_domain(dims, F, ncls, prec):
    net = uresnet(dims=list(dims), num_class=ncls, base_num_outputs=F, num_strides=3)
    net.construct(trainable=True, use_weight=True, allocate=False, precision=prec)
    assert net._n_params == sum(int(O.np.prod(sh)) for _, sh in O.param_specs(len(dims) - 1, dims[-1], F, ncls, 3))
