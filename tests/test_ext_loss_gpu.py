"""External loss boundary on the GPU: the three op-level passes of ext_loss.hip against host restatements / the fp64 oracle, and
the net-level pair ursn_forward_logits / ursn_backward_logits through ssnet_base and torch.autograd on both plans.

Bounds: 2e-5 of the tensor's max is the project's in-situ fp32 bound for one kernel against fp64 on the same
operands; `replay` comparisons are on raw bits (same code, same order of every sum: no tolerance); gradients against the oracle
follow the rule of tests/test_net_gpu.py::test_accum_gradients_parity (4 x the fp32 oracle's own deviation, at least 2e-3, never
above 5e-2); two paths that share a forward are held to l2_rel <= 1e-3 (test_normalise_on_load_plan_matches_default)."""
import ctypes

import numpy as np
import pytest
import torch

from oracle import uresnet_np as O
from _abi import Handle, bits, make_cfg, same_bits, upload
from _net import as_f32_exact, l2_rel, make_inputs, max_rel, oracle_params
from uresnet_amd import _lib, uresnet
from uresnet_amd.autograd import UResNetFunction

pytestmark = pytest.mark.gpu

GUARD = 64                      # floats of guard pattern on either side of an op-level output
PATTERN = np.float32(-1.2345678e-7)
VOXELS = (1, 7, 256, 4099)      # 4099: more than one 1024-voxel span per event, odd, a tail that is no multiple of 4
BATCHES = (1, 3)


def _p(t):
    return ctypes.c_void_p(t.data_ptr()) if t is not None else None


def _bf16_bits(a):
    """fp32 array of bf16-exact values -> uint16 bit patterns."""
    return (np.ascontiguousarray(a, np.float32).view(np.uint32) >> 16).astype(np.uint16)


def _dev_u16(a):
    return torch.from_numpy(a.view(np.int16).copy()).cuda()


def _guarded(nfloat, off):
    """Device floats [GUARD | off | nfloat | GUARD] filled with the guard pattern; returns (buffer, index of the output)."""
    buf = torch.full((GUARD + off + nfloat + GUARD,), float(PATTERN), dtype=torch.float32, device="cuda")
    return buf, GUARD + off


def _check_guards(buf, start, nfloat, what):
    h = buf.cpu().numpy()
    pat = np.full(1, PATTERN, np.float32).view(np.uint32)[0]
    assert (bits(h[:start]) == pat).all(), "%s: memory in front of the output was written" % (what,)
    assert (bits(h[start + nfloat:]) == pat).all(), "%s: memory behind the output was written" % (what,)
    return h[start:start + nfloat]


# ---- 1. ursn_logits_dense -----------------------------------------------------------------------------------------------
def _layouts(ncls):
    lay = [("fp32", ncls), ("fp32", 8), ("bf16", 8)]
    if ncls <= 4:
        lay.append(("fp32", 4))
    return [l for i, l in enumerate(lay) if l not in lay[:i]]


@pytest.mark.parametrize("ncls", [1, 3, 4, 5, 8])
def test_logits_dense_op(lib, ncls):
    rng = np.random.default_rng(100 + ncls)
    worst = 0.0
    for vox in VOXELS:
        for n in BATCHES:
            P = n * vox
            for dt, cs in _layouts(ncls):
                z = rng.standard_normal((P, cs)).astype(np.float32) * 3
                if dt == "bf16":
                    z = O.bf16_round(z)
                    zd = _dev_u16(_bf16_bits(z))
                else:
                    zd = torch.from_numpy(z).cuda()
                mean = rng.standard_normal(8).astype(np.float32)
                rstd = rng.uniform(0.5, 2.0, 8).astype(np.float32)
                beta = rng.standard_normal(8).astype(np.float32)
                md, rd, bd = upload(mean, rstd, beta)
                for with_mean in (True, False):
                    ref = z[:, :ncls].astype(np.float64)
                    if with_mean:
                        ref = (ref - mean[:ncls].astype(np.float64)) * rstd[:ncls].astype(np.float64) + beta[:ncls].astype(np.float64)
                    for off in (0, 1):   # 16-byte aligned and one float off
                        buf, start = _guarded(P * ncls, off)
                        assert (buf.data_ptr() + 4 * start) % 16 == 4 * off
                        d = _lib.ursn_vscores_desc()
                        d.n, d.voxels, d.ncls, d.z, d.z_cstride, d.dtype = n, vox, ncls, zd.data_ptr(), cs, int(dt == "bf16")
                        if with_mean:
                            d.mean, d.rstd, d.beta = md.data_ptr(), rd.data_ptr(), bd.data_ptr()
                        _lib.check(lib.ursn_logits_dense(ctypes.byref(d), ctypes.c_void_p(buf.data_ptr() + 4 * start), None))
                        torch.cuda.synchronize()
                        what = "logits_dense vox %d n %d ncls %d %s stride %d mean %s off %d" % (vox, n, ncls, dt, cs, with_mean, off)
                        got = _check_guards(buf, start, P * ncls, what).reshape(P, ncls)
                        err = max_rel(got, ref)
                        worst = max(worst, err)
                        assert err <= 2e-5, (what, err)
    print("logits_dense ncls %d: worst error %.3g of max" % (ncls, worst))


# ---- 2. ursn_dlogits_pack -----------------------------------------------------------------------------------------------
# +-0; ties that round to even downwards (1 + 2^-8 -> 1, mantissa 0) and upwards (1 + 3 * 2^-8 -> 1 + 2^-6); the tie 2 - 2^-8 and
# a value just under 2, which both round up into the next binade; a large finite value
SPECIALS = np.array([0.0, -0.0, 1.00390625, 1.01171875, -1.00390625, 1.99609375, 1.9999999, 2.0 ** -126, -3.0e38], np.float32)


@pytest.mark.parametrize("ncls", [1, 3, 4, 5, 8])
def test_dlogits_pack_op(lib, ncls):
    rng = np.random.default_rng(200 + ncls)
    for vox in VOXELS:
        for n in BATCHES:
            P = n * vox
            g = (rng.standard_normal((P, ncls)) / vox).astype(np.float32)
            flat = g.reshape(-1)
            k = min(flat.size, SPECIALS.size)
            flat[:k] = SPECIALS[:k]
            gd = torch.from_numpy(g).cuda()
            for dt, cs in _layouts(ncls):
                what = "dlogits_pack vox %d n %d ncls %d %s stride %d" % (vox, n, ncls, dt, cs)
                if dt == "bf16":
                    out = torch.full((GUARD * 2 + P * 8 + GUARD * 2,), 0x5A5A, dtype=torch.int16, device="cuda")
                    start = GUARD * 2
                    assert (out.data_ptr() + 2 * start) % 16 == 0
                    _lib.check(lib.ursn_dlogits_pack(_p(gd), n, vox, ncls, ctypes.c_void_p(out.data_ptr() + 2 * start), 8, 1, None))
                    torch.cuda.synchronize()
                    h = out.cpu().numpy().view(np.uint16)
                    assert (h[:start] == 0x5A5A).all() and (h[start + P * 8:] == 0x5A5A).all(), what
                    want = np.zeros((P, 8), np.uint16)
                    want[:, :ncls] = _bf16_bits(O.bf16_round(g))   # round-to-nearest-even of each value, pad lanes zero
                    assert np.array_equal(h[start:start + P * 8].reshape(P, 8), want), what
                else:
                    buf, start = _guarded(P * cs, 0)
                    _lib.check(lib.ursn_dlogits_pack(_p(gd), n, vox, ncls, ctypes.c_void_p(buf.data_ptr() + 4 * start), cs, 0, None))
                    torch.cuda.synchronize()
                    got = _check_guards(buf, start, P * cs, what).reshape(P, cs)
                    # stride 4 with <= 4 classes: the head's 16-byte store, pad lanes zero; every other stride: its scalar branch,
                    # which leaves the pad lanes as they were
                    want = np.full((P, cs), 0.0 if (cs == 4 and ncls <= 4) else PATTERN, np.float32)
                    want[:, :ncls] = g
                    assert same_bits(got, want), what


def test_bf16_rounding_cases_are_what_they_claim():
    """The special values really are ties / next-binade cases under the host restatement."""
    r = O.bf16_round(SPECIALS)
    assert r[2] == 1.0 and r[3] == np.float32(1.015625) and r[4] == -1.0 and r[5] == 2.0 and r[6] == 2.0
    assert bits(r[:2]).tolist() == [0, 0x80000000]


# ---- 3. ursn_conv0_input_grad -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("spatial", [(5, 7), (32, 32), (3, 5, 9), (8, 16, 32), (16, 16, 16)])
def test_conv0_input_grad_op(lib, spatial):
    rng = np.random.default_rng(300 + len(spatial) + spatial[-1])
    nd, n, V = len(spatial), 2, int(np.prod(spatial))
    sp = (ctypes.c_int32 * 3)(*(list(spatial) + [1] * (3 - nd)))
    worst = 0.0
    cases = [("fp32", cin, F, cs) for cin in (1, 3) for F in (1, 4, 8, 16) for cs in sorted({F, ((F + 3) & ~3) if F % 4 else F + 4})]
    cases += [("bf16", 1, F, cs) for F in (8, 16) for cs in (F, F + 8)]
    for dt, cin, F, cs in cases:
        dz = rng.standard_normal((n,) + tuple(spatial) + (F,)).astype(np.float32)
        w = (rng.standard_normal((3,) * nd + (cin, F)) * 0.3).astype(np.float32)
        wref = w
        pad = np.full((n * V, cs), 7.0e37, np.float32)   # pad lanes hold a large finite value: they must not be read into the sum
        if dt == "bf16":
            dz = O.bf16_round(dz)
            pad = O.bf16_round(pad)
            wref = O.bf16_round(w)   # the kernel rounds the fp32 master weights to bf16 on load
        pad[:, :F] = dz.reshape(n * V, F)
        dzd = _dev_u16(_bf16_bits(pad)) if dt == "bf16" else torch.from_numpy(pad).cuda()
        wd = torch.from_numpy(w).cuda()
        buf, start = _guarded(n * V * cin, 0)
        _lib.check(lib.ursn_conv0_input_grad(nd, sp, n, cin, F, _p(dzd), cs, int(dt == "bf16"), _p(wd),
                                             ctypes.c_void_p(buf.data_ptr() + 4 * start), None))
        torch.cuda.synchronize()
        what = "conv0_input_grad %s %s cin %d F %d stride %d" % (spatial, dt, cin, F, cs)
        got = _check_guards(buf, start, n * V * cin, what).reshape((n,) + tuple(spatial) + (cin,))
        x = np.zeros((n,) + tuple(spatial) + (cin,), np.float64)
        ref = O.conv_bwd(x, wref.astype(np.float64), 1, dz.astype(np.float64))[0]
        err = max_rel(got, ref)
        worst = max(worst, err)
        assert err <= 2e-5, (what, err)
    print("conv0_input_grad %s: worst error %.3g of max" % (spatial, worst))


# ---- net-level fixtures -------------------------------------------------------------------------------------------------
# dims, F, classes, num_strides, batch, batch the handle is built for
SHAPES = [((16, 16, 16, 1), 8, 3, 2, 2, 2), ((32, 32, 1), 8, 5, 3, 2, 2), ((8, 16, 32, 1), 8, 4, 2, 1, 2)]
SHAPE_IDS = ["3d_3cls", "2d_5cls", "3d_4cls_batch1of2"]
PLANS = ["fp32", "bf16"]


def _net(shape, plan, use_weight=True, lr=None):
    dims, F, ncls, ns, N, NB = shape
    net = uresnet(dims=list(dims), num_class=ncls, base_num_outputs=F, num_strides=ns)
    net.construct(trainable=True, use_weight=use_weight, learning_rate=lr, precision=plan)
    P = as_f32_exact(oracle_params(dims, F, ncls, num_strides=ns))
    net.set_variables(P)
    if NB > N:   # a handle built for a larger batch than the one under test
        big = make_inputs(dims, ncls, NB, seed=77)
        net.run_test(None, *big)
    return net, P


def _grad_vec(net):
    torch.cuda.synchronize()
    return net._grads.detach().cpu().numpy().copy()


# ---- 4. logits in situ ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("plan", PLANS)
@pytest.mark.parametrize("shape", SHAPES, ids=SHAPE_IDS)
def test_forward_logits_in_situ(shape, plan):
    dims, F, ncls, ns, N, NB = shape
    net, P = _net(shape, plan)
    data, label, weight = make_inputs(dims, ncls, N, seed=5)
    logits = net.forward_logits(None, data, as_numpy=True)
    assert logits.shape == (N,) + tuple(dims[:-1]) + (ncls,) and logits.dtype == np.float32
    assert isinstance(net.forward_logits(None, data), torch.Tensor)
    z = net.debug_tensor("UResNet/conv2:z").astype(np.float64)
    mean = net.debug_tensor("UResNet/conv2:mean").astype(np.float64)
    rstd = net.debug_tensor("UResNet/conv2:rstd").astype(np.float64)
    beta = net.get_variables()["UResNet/conv2/BatchNorm/beta"].astype(np.float64)
    ref = (z - mean) * rstd + beta
    err = max_rel(logits, ref)
    print("forward_logits in situ %s %s: %.3g of max" % (dims, plan, err))
    assert err <= 2e-5, err
    if plan == "fp32":
        d = O.reshape_inputs(dims, data)[0].astype(np.float64)
        ref_logits, _ = O.forward(P, d, F, num_strides=ns)
        assert max_rel(logits, ref_logits) < 1e-3


# ---- 5. replay is the step, bit for bit ---------------------------------------------------------------------------------
@pytest.mark.parametrize("plan", PLANS)
@pytest.mark.parametrize("shape", SHAPES, ids=SHAPE_IDS)
def test_replay_of_the_heads_dlogits_is_the_step(shape, plan):
    dims, F, ncls, ns, N, NB = shape
    net, P = _net(shape, plan)
    data, label, weight = make_inputs(dims, ncls, N, seed=6)
    dd, ld, wd = upload(data, label, weight)
    net.zero_gradients(None)
    net.accum_gradients(None, dd, ld, wd)
    G1 = _grad_vec(net)
    D = net.debug_tensor("logits:grad")
    assert D.shape == (N,) + tuple(dims[:-1]) + (ncls,) and np.abs(D).max() > 0
    net.zero_gradients(None)
    net.forward_logits(None, dd)
    assert net.backward_logits(None, D) is None
    G2 = _grad_vec(net)
    assert np.abs(G1).max() > 0
    assert same_bits(G1, G2), "%d of %d gradient elements differ" % (int((bits(G1) != bits(G2)).sum()), G1.size)
    # accumulation is a SUM (lib/ssnet.py:77), as test_accum_gradients_parity checks it for a step
    net.forward_logits(None, dd)
    net.backward_logits(None, torch.from_numpy(D).cuda())
    g1 = {k: v for k, v in net.get_gradients().items()}
    off = 0
    for name, shp, o, cnt in net._specs:
        a = G1[o:o + cnt]
        if np.abs(a).max() > 1e-12:
            assert max_rel(g1[name].reshape(-1), 2 * a) < 1e-5, name


# ---- 6. arbitrary d-logits against the oracle -----------------------------------------------------------------------------
ORACLE_SHAPES = [((16, 16, 16, 1), 4, 3, 2, 2, 2), ((32, 32, 1), 8, 5, 3, 2, 2)]


@pytest.mark.parametrize("shape", ORACLE_SHAPES, ids=["3d_f4_3cls", "2d_f8_5cls"])
def test_arbitrary_dlogits_against_oracle(shape):
    dims, F, ncls, ns, N, NB = shape
    net, P = _net(shape, "fp32")
    data, _, _ = make_inputs(dims, ncls, N, seed=8)
    vox = int(np.prod(dims[:-1]))
    rng = np.random.default_rng(9)
    dl = (rng.standard_normal((N,) + tuple(dims[:-1]) + (ncls,)) / vox).astype(np.float32)
    d64 = O.reshape_inputs(dims, data)[0].astype(np.float64)
    _, tape = O.forward(P, d64, F, num_strides=ns)
    g_ref, din_ref = O.backward(P, tape, dl.astype(np.float64))
    P32 = type(P)((k, v.astype(np.float32)) for k, v in P.items())
    _, tape32 = O.forward(P32, d64.astype(np.float32), F, num_strides=ns)
    g_32, din_32 = O.backward(P32, tape32, dl)

    net.zero_gradients(None)
    net.forward_logits(None, data)
    din = net.backward_logits(None, dl, want_input_grad=True)
    assert tuple(din.shape) == (N,) + tuple(dims) and din.dtype == torch.float32
    din = din.cpu().numpy()
    g = net.get_gradients()
    bad = []
    for k in g_ref:
        if np.abs(g_ref[k]).max() <= 1e-12:
            continue
        e, floor = l2_rel(g[k], g_ref[k]), l2_rel(g_32[k], g_ref[k])
        if e > min(max(2e-3, 4 * floor), 5e-2):
            bad.append((k, e, floor))
    e, floor = l2_rel(din, din_ref), l2_rel(din_32, din_ref)
    print("input gradient %s: l2_rel %.3g (fp32 oracle %.3g)" % (dims, e, floor))
    if e > min(max(2e-3, 4 * floor), 5e-2):
        bad.append(("d data", e, floor))
    assert not bad, bad


@pytest.mark.parametrize("plan", PLANS)
@pytest.mark.parametrize("shape", ORACLE_SHAPES, ids=["3d_f4_3cls", "2d_f8_5cls"])
def test_input_gradient_in_situ(shape, plan):
    dims, F, ncls, ns, N, NB = shape
    if plan == "bf16":
        F = 8   # the bf16 plan needs base filters in multiples of 8
    shape = (dims, F, ncls, ns, N, NB)
    net, P = _net(shape, plan)
    data, _, _ = make_inputs(dims, ncls, N, seed=10)
    rng = np.random.default_rng(11)
    dl = (rng.standard_normal((N,) + tuple(dims[:-1]) + (ncls,)) / np.prod(dims[:-1])).astype(np.float32)
    net.forward_logits(None, data)
    din = net.backward_logits(None, dl, want_input_grad=True).cpu().numpy()
    dz = net.debug_tensor("UResNet/conv0:dz").astype(np.float64)
    w = net.get_variables()["UResNet/conv0/weights"]
    if plan == "bf16":
        w = O.bf16_round(w)
    x = O.reshape_inputs(dims, data)[0].astype(np.float64)
    ref = O.conv_bwd(x, w.astype(np.float64), 1, dz)[0]
    err = max_rel(din, ref)
    print("input gradient in situ %s %s: %.3g of max" % (dims, plan, err))
    assert np.abs(ref).max() > 0 and err <= 2e-5, err


# ---- 7. autograd ----------------------------------------------------------------------------------------------------------
def _reference_loss(logits, label, weight):
    """lib/ssnet.py:67-71 in torch: mean over events of sum over pixels of weight * cross-entropy."""
    N, C = logits.shape[0], logits.shape[-1]
    ce = torch.nn.functional.cross_entropy(logits.reshape(-1, C), label.reshape(-1).long(), reduction="none").reshape(N, -1)
    return (ce * weight.reshape(N, -1)).sum(dim=1).mean()


# bf16: the d-logits torch hands back are rounded to bf16 by dlogits_pack, the head rounds its own fp32 expression: the two can
# differ by one bf16 rounding where the fp32 values differ in their last bits.  The project has no bound for that, so it was
# measured: on an MI355X, this shape and these inputs, the worst per-tensor l2_rel against accum_gradients is 0 -- every rounded
# d-logit equals the head's and the gradient buffers are bit-equal (DESIGN.md "External loss boundary").  The bound is 4 x the
# measured figure, never above 2^-6, the project's bf16 path-consistency bar; there are no atomics on either path and every
# reduction has a fixed order, so the figure is reproducible.
BF16_AUTOGRAD_MEASURED = 0.0
BF16_AUTOGRAD_BOUND = min(4 * BF16_AUTOGRAD_MEASURED, 2.0 ** -6)


@pytest.mark.parametrize("plan", PLANS)
def test_autograd_function_matches_the_step(plan):
    shape = ((16, 16, 16, 1), 8, 3, 2, 2, 2)
    dims, F, ncls, ns, N, NB = shape
    net, P = _net(shape, plan)
    data, label, weight = make_inputs(dims, ncls, N, seed=12)
    dd, ld, wd = upload(data, label, weight)
    net.zero_gradients(None)
    res, _ = net.accum_gradients(None, dd, ld, wd)
    g_step = net.get_gradients()
    net.zero_gradients(None)
    x = dd.clone().requires_grad_(True)
    logits = UResNetFunction.apply(net, None, x)
    logits.retain_grad()
    loss = _reference_loss(logits, ld, wd)
    loss.backward()
    g_auto = net.get_gradients()
    worst = max(l2_rel(g_auto[k], g_step[k]) for k in g_step if np.abs(g_step[k]).max() > 1e-12)
    lrel = abs(float(loss.item()) - res[1]) / abs(res[1])
    print("autograd %s: loss rel %.3g, worst per-tensor l2_rel against accum_gradients %.4g" % (plan, lrel, worst))
    if plan == "fp32":
        assert lrel <= 1e-4, lrel
        assert worst <= 1e-3, worst
    else:
        assert worst <= BF16_AUTOGRAD_BOUND, worst
    # the input gradient: shape of the input, the bits backward_logits returns for the same d-logits
    assert x.grad is not None and tuple(x.grad.shape) == tuple(x.shape)
    dl = logits.grad.detach().clone()
    net.forward_logits(None, dd)
    din = net.backward_logits(None, dl, want_input_grad=True)
    assert same_bits(x.grad.cpu().numpy().reshape(-1), din.cpu().numpy().reshape(-1))
    assert float(x.grad.abs().max()) > 0
    # without requires_grad no input gradient is formed
    net.zero_gradients(None)
    y = UResNetFunction.apply(net, None, dd)
    assert not y.requires_grad


@pytest.mark.parametrize("plan", PLANS)
def test_accum_gradients_custom_focal(plan):
    shape = ((16, 16, 16, 1), 8, 3, 2, 2, 2)
    dims, F, ncls, ns, N, NB = shape
    net, P = _net(shape, plan, lr=1e-3)
    data, label, weight = make_inputs(dims, ncls, N, seed=13)
    lab = torch.from_numpy(label).cuda().long()

    def focal(logits, gamma=2.0):
        logp = torch.log_softmax(logits.reshape(N, -1, ncls), dim=-1)
        lp = torch.gather(logp, 2, lab.reshape(N, -1, 1))[..., 0]
        return (-(1.0 - lp.exp()) ** gamma * lp).mean()

    before = net.get_variables()
    net.zero_gradients(None)
    res, doc = net.accum_gradients_custom(None, data, focal)
    assert doc == ['', 'loss'] and res[0] is None and np.isfinite(res[1]) and res[1] > 0
    assert net.accum_gradients_custom(None, data, focal, fetch=False)[0] is None
    net.apply_gradients(None)
    after = net.get_variables()
    assert all(np.isfinite(v).all() for v in after.values())
    assert any(not np.array_equal(before[k], after[k]) for k in before)
    assert not np.array_equal(before["UResNet/conv0/weights"], after["UResNet/conv0/weights"])


# ---- 8. state rules -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("plan", PLANS)
def test_backward_logits_needs_its_forward(lib, plan):
    shape = ((16, 16, 16, 1), 8, 3, 2, 2, 2)
    dims, F, ncls, ns, N, NB = shape
    net, P = _net(shape, plan)
    data, label, weight = make_inputs(dims, ncls, N, seed=14)
    dd, ld, wd = upload(data, label, weight)
    dl = torch.full((N,) + tuple(dims[:-1]) + (ncls,), 1e-4, dtype=torch.float32, device="cuda")
    net.zero_gradients(None)
    net.accum_gradients(None, dd, ld, wd)
    G = _grad_vec(net)

    def refused(text, fn):
        with pytest.raises((_lib.UrsnError, ValueError, RuntimeError)) as e:
            fn()
        assert text in str(e.value), str(e.value)
        assert same_bits(G, _grad_vec(net)), "a refused call changed the gradient buffer"

    refused("no ursn_forward_logits has run", lambda: net.backward_logits(None, dl))
    net.forward_logits(None, dd)
    net.inference(None, dd)
    refused("another run call", lambda: net.backward_logits(None, dl))
    net.forward_logits(None, dd)
    net.run_test(None, dd, ld, wd)
    refused("another run call", lambda: net.backward_logits(None, dl))
    net.forward_logits(None, dd)
    refused("shape", lambda: net.backward_logits(None, dl[:1]))            # a different batch, seen by the Python layer
    rc = lib.ursn_backward_logits(net._handle, _p(dd), _p(dl), 1, None, None)   # ... and by the library
    assert rc != 0 and b"batch 1" in lib.ursn_last_error()
    rc = lib.ursn_backward_logits(net._handle, _p(ld), _p(dl), N, None, None)   # another data tensor
    assert rc != 0 and b"data is not the tensor" in lib.ursn_last_error()
    assert same_bits(G, _grad_vec(net))
    net.backward_logits(None, dl)                                           # the refusals left the forward pending
    assert not same_bits(G, _grad_vec(net))
    G = _grad_vec(net)
    refused("already consumed", lambda: net.backward_logits(None, dl))
    net.forward_logits(None, dd)
    net.apply_gradients(None)
    G = _grad_vec(net)
    refused("ursn_apply_adam changed the parameters", lambda: net.backward_logits(None, dl))


def _pair(h, dd, dl, n, want_din):
    """forward_logits + backward_logits on a bare handle: (logits, gradient buffer, input gradient) as host arrays."""
    ncls, pix = int(h.cfg.num_class), h.pix
    logits = torch.full((n, pix, ncls), float("nan"), dtype=torch.float32, device="cuda")
    din = torch.full((n, pix * int(h.cfg.cin)), float("nan"), dtype=torch.float32, device="cuda") if want_din else None
    torch.cuda.synchronize()
    h.last_n = n
    _lib.check(h.lib.ursn_forward_logits(h.handle, _p(dd), n, _p(logits), None))
    _lib.check(h.lib.ursn_backward_logits(h.handle, _p(dd), _p(dl), n, _p(din), None))
    torch.cuda.synchronize()
    return logits.cpu().numpy(), h.host("grads"), (din.cpu().numpy() if want_din else None)


@pytest.mark.parametrize("plan", PLANS)
def test_pair_depends_only_on_its_arguments(plan):
    dims, F, ncls, ns, N = (16, 16, 16, 1), 8, 3, 2, 2
    data, label, weight = make_inputs(dims, ncls, N, seed=15)
    other = make_inputs(dims, ncls, N, seed=16)
    dd, ld, wd = upload(data, label, weight)
    od, ol, ow = upload(*other)
    rng = np.random.default_rng(17)
    dl, = upload((rng.standard_normal((N, int(np.prod(dims[:-1])), ncls)) / 4096).astype(np.float32))
    results = {}
    for fill in ("zero", "nan"):
        with Handle(make_cfg(dims, F, ncls, ns, N, bf16=(plan == "bf16")), fill) as h:
            h.zero_grad(fetch=False)
            first = _pair(h, dd, dl, N, True)
            assert np.isfinite(first[0]).all() and np.isfinite(first[1]).all() and np.isfinite(first[2]).all()
            # unrelated calls of every kind, other inputs, another batch size
            h.accum_step(od, ol, ow, N, fetch=False)
            h.eval(od, ol, ow, 1)
            h.infer(od, ol, N)
            h.infer_labels(od, ol, 1)
            _pair(h, od, dl, N, False)
            h.zero_grad(fetch=False)
            again = _pair(h, dd, dl, N, True)
            for a, b, name in zip(first, again, ("logits", "gradients", "input gradient")):
                assert same_bits(a, b), "%s differ after unrelated calls (fill %s)" % (name, fill)
            results[fill] = first
    for a, b, name in zip(results["zero"], results["nan"], ("logits", "gradients", "input gradient")):
        assert same_bits(a, b), "%s depend on what the workspace held at create" % name
