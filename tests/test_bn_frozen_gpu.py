"""Frozen-BatchNorm training on the device: the op-level entries against their statement, the single-pass kernels against the
reduce / zero-mean finalise / apply route (two processes: URSN_BN_FROZEN_FUSED is read once), net-level gradients against the
oracle differentiated through fixed statistics, the mode's side effects, every training entry under it, and independence of the
workspace fill and of the handle's history.

Shapes: those of tests/test_bn_moving_gpu.py.  Moving statistics always come from bn_calibrate on ANOTHER batch, so the network is
alive (no reference gradient tensor is zero: asserted).  Reference: tests/_bn_frozen.py."""
import ctypes
import functools
import os
import subprocess
import sys

import numpy as np
import pytest

import _bn_frozen as B
from _abi import Handle, bits, compare_outputs, make_cfg, same_bits, upload
from _bn_frozen import CASES, FULL, IDS, PAD, S3D
from _net import as_f32_exact, l2_rel, make_inputs, max_rel, oracle_params
from oracle import uresnet_np as O
from uresnet_amd import _lib
from uresnet_amd.ssnet import VoxelBatch

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---- 1. op level against the statement ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("relu", B.F32_RELU)
@pytest.mark.parametrize("C", B.F32_C)
def test_op_fp32_is_rstd_times_g(C, relu):
    """dz == np.float32(rstd) * g as values (the sign of a zero is not compared); dbeta against the fp64 sum at the 2e-5 of
    tests/test_ops_gpu.py; nothing behind the operands is written.  C = 6 takes the scalar path; V = 1, 255, 256, 771 voxels."""
    for V in B.F32_V:
        c = B.f32_case(C, V, relu)
        dz, db = B.run_f32_op(C, V, relu)
        want = (c["rstd"][None, :] * c["g"]).astype(np.float32)
        assert np.array_equal(dz[:V * C].reshape(V, C), want), (C, V, relu)
        ref = c["g"].astype(np.float64).sum(axis=0)
        assert np.abs(db[:C] - ref).max() <= 2e-5 * (np.abs(ref).max() + 1e-30), (C, V, relu)
        assert np.isnan(dz[V * C:]).all() and np.isnan(db[C:]).all(), (C, V, relu)


@pytest.mark.parametrize("C,mask,form", B.bf_variants(), ids=["C%d-mask%d-%s" % v for v in B.bf_variants()])
def test_op_bf16_is_the_statement_rounded_once(C, mask, form):
    """Every mask kind (none, y > 0, bn(z) > 0, mask bytes) with the join's second BatchNorm, the residual share set and
    accumulated, and the second gradient operand: each output is its fp32 statement rounded once to bf16."""
    V, c = B.BF_V, B.bf_case(C, mask, form)
    out = B.run_bf_op(C, mask, form)
    g = c["g"]
    assert np.array_equal(out["dz"][:V * C].reshape(V, C), B.bf_round(c["rstd"][None, :] * g))
    ref = g.astype(np.float64).sum(axis=0)
    tol = 1e-5 * np.abs(g.astype(np.float64)).sum(axis=0).max()        # tests/test_bf16_ops_gpu.py's d(beta) tolerance
    assert np.abs(out["dbeta"] - ref).max() <= tol
    if form == "join2":
        assert np.array_equal(out["dz2"][:V * C].reshape(V, C), B.bf_round(c["rstd2"][None, :] * g))
        assert np.abs(out["dbeta2"] - ref).max() <= tol
    if form in ("dres_set", "dres_acc"):
        want = B.bf_round(c["base"] + g) if form == "dres_acc" else B.bf_round(g)
        assert np.array_equal(out["dres"][:V * C].reshape(V, C), want)
    for k in ("dz", "dz2", "dres"):
        if k in out:
            assert np.isnan(out[k][V * C:]).all(), k


# ---- 2. the single pass against the always-correct route -------------------------------------------------------------------------
@pytest.fixture(scope="module")
def ab(tmp_path_factory):
    """The child of tests/_bn_frozen.py once per value of the switch, one after the other."""
    d = tmp_path_factory.mktemp("bn_frozen_ab")
    outs = {}
    for v in ("0", "1"):
        f = str(d / ("fused%s.npz" % v))
        e = dict(os.environ)
        e["URSN_BN_FROZEN_FUSED"] = v
        subprocess.run([sys.executable, os.path.join(ROOT, "tests", "_bn_frozen.py"), ROOT, f], check=True, env=e, timeout=600)
        outs[v] = dict(np.load(f))
    return outs


def test_fused_against_path1_op_level(ab):
    """Every variant of 1.: outputs equal as values (guards included: both NaN), every d(beta) bitwise."""
    a, b = ab["0"], ab["1"]
    keys = [k for k in a if not k.startswith("net|")]
    assert sorted(keys) == sorted(k for k in b if not k.startswith("net|")) and len(keys) > 200
    for k in keys:
        if "dbeta" in k:
            assert same_bits(a[k], b[k]), k
        else:
            assert np.array_equal(a[k], b[k], equal_nan=True), k


@pytest.mark.parametrize("prec", ["fp32", "bf16"])
def test_fused_against_path1_net_level(ab, prec):
    """Full-depth shape: the loss identical, every gradient tensor equal as values, the d(beta) tensors bitwise -- and the two
    processes really took different routes (profiler pass 5)."""
    a, b = ab["0"], ab["1"]
    name = "bn_bwd" if prec == "fp32" else "bbn_bwd"
    assert list(a["net|%s|kernels" % prec]) == [name], a["net|%s|kernels" % prec]
    assert name + "_frozen" in list(b["net|%s|kernels" % prec])
    assert float(a["net|%s|loss" % prec]) == float(b["net|%s|loss" % prec])
    keys = [k for k in a if k.startswith("net|%s|g|" % prec)]
    assert len(keys) == 116
    for k in keys:
        assert np.array_equal(a[k], b[k]), k
        if k.endswith("beta"):
            assert same_bits(a[k], b[k]), k


# ---- 3. net-level gradients against the frozen oracle -----------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _device_step(ci):
    """One frozen step (and a second one) on the device; computed once per case, shared, never modified."""
    shape, prec = CASES[ci]
    tag, dims, base, ncls, ns, n = shape
    net, P, stats = B.calibrated_net(shape, prec)
    data, label, weight = make_inputs(dims, ncls, n, seed=B.SEED_STEP)
    net.zero_gradients(None)
    res, doc = net.accum_gradients(None, data, label, weight)
    g = net.get_gradients()
    net.accum_gradients(None, data, label, weight)
    g2 = net.get_gradients()
    return P, stats, (data, label, weight), res, g, g2


@pytest.mark.parametrize("ci", range(len(CASES)), ids=IDS)
def test_net_gradients_against_the_frozen_oracle(ci):
    shape, prec = CASES[ci]
    tag, dims, base, ncls, ns, n = shape
    P, stats, (data, label, weight), res, g, g2 = _device_step(ci)
    g_ref, m = B.oracle_frozen_step(P, shape, stats, data, label, weight)
    assert all(np.abs(v).max() > 0 for v in g_ref.values()), [k for k, v in g_ref.items() if np.abs(v).max() == 0]
    if prec == "fp32":
        g_32, _ = B.oracle_frozen_step(P, shape, stats, data, label, weight, noise_floor=True)
        print("%s: loss gpu %.7f oracle %.7f" % (tag, res[1], m["loss"]))
        assert abs(res[1] - m["loss"]) <= 1e-4 * abs(m["loss"])
        bad, worst = [], 0.0
        for k in g_ref:      # the rule of tests/test_net_gpu.py::test_accum_gradients_parity, the floor under the same swap
            e, floor = l2_rel(g[k], g_ref[k]), l2_rel(g_32[k], g_ref[k])
            worst = max(worst, e)
            if e > min(max(2e-3, 4 * floor), 5e-2):
                bad.append((k, e, floor))
        print("%s: worst gradient rel-L2 %.2e over %d tensors" % (tag, worst, len(g_ref)))
        assert not bad, bad
    else:
        g_q, m_q = B.oracle_frozen_step(P, shape, stats, data, label, weight, quant=True)
        wk = [k for k in g_q if k.endswith("/weights")]
        e_gq = [l2_rel(g[k], g_q[k]) for k in wk]
        e_qx = [l2_rel(g_q[k], g_ref[k]) for k in wk]
        cos = lambda a, b: float(np.dot(np.ravel(a).astype(np.float64), np.ravel(b)) / (np.linalg.norm(np.asarray(a, np.float64)) * np.linalg.norm(b) + 1e-300))
        c_gpu, c_emu = min(cos(g[k], g_ref[k]) for k in wk), min(cos(g_q[k], g_ref[k]) for k in wk)
        bound = 1.5 * np.median(e_qx) + 0.02      # tests/test_bf16_net_gpu.py::test_bf16_accum_gradients_against_emulating_oracle
        print("%s bf16: loss gpu %.5f emu %.5f | filter grads vs emu: median %.2e max %.2e (bound %.2e) | cosine min %.4f (emu %.4f)"
              % (tag, res[1], m_q["loss"], np.median(e_gq), max(e_gq), bound, c_gpu, c_emu))
        assert abs(res[1] - m_q["loss"]) <= 1e-2 * abs(m_q["loss"])
        assert np.median(e_gq) <= bound and max(e_gq) <= 2 * bound
        assert c_gpu >= min(0.95, c_emu - 0.05)
    assert max(max_rel(g2[k], 2 * g[k]) for k in g) < 1e-5      # a second call doubles the buffer


# ---- 4. side effects ---------------------------------------------------------------------------------------------------------------
def test_moving_buffer_is_constant_and_training_works():
    tag, dims, base, ncls, ns, n = S3D
    net, P, stats = B.calibrated_net(S3D, "fp32", lr=1e-3)
    data, label, weight = make_inputs(dims, ncls, n, seed=B.SEED_STEP)
    before_v = net.get_variables()
    losses = []
    for it in range(5):
        net.zero_gradients(None)
        losses.append(net.accum_gradients(None, data, label, weight)[0][1])
        net.apply_gradients(None)
    after = net.get_bn_moving()
    assert list(after) == list(stats) and all(same_bits(after[k], stats[k]) for k in stats)
    assert all(not np.array_equal(v, before_v[k]) for k, v in net.get_variables().items())
    last = net.run_test(None, data, label, weight)[0][0]
    print("golden3d: five Adam steps on one batch, loss %s -> %.5f" % (["%.5f" % l for l in losses], last))
    assert last < losses[0] and losses[-1] < losses[0]


def test_batch_mode_is_untouched_by_the_mode():
    tag, dims, base, ncls, ns, n = S3D
    data, label, weight = make_inputs(dims, ncls, n, seed=B.SEED_STEP)
    net = B.build_net(S3D, "fp32")
    net.set_variables(as_f32_exact(oracle_params(dims, base, ncls, num_strides=ns)))
    net.zero_gradients(None)
    first = net.accum_gradients(None, data, label, weight)[0]
    g_first = net.get_gradients()
    net.bn_calibrate(None, [make_inputs(dims, ncls, n, seed=B.SEED_CALIB)[0]])
    net.set_bn_mode('frozen')
    net.zero_gradients(None)
    frozen = net.accum_gradients(None, data, label, weight)[0]
    assert frozen[1] != first[1]
    net.set_bn_mode('batch')
    net.zero_gradients(None)
    again = net.accum_gradients(None, data, label, weight)[0]
    assert again == first and all(same_bits(v, g_first[k]) for k, v in net.get_gradients().items())


# ---- 5. entries --------------------------------------------------------------------------------------------------------------------
def test_voxel_feed_equals_the_dense_feed():
    tag, dims, base, ncls, ns, n = S3D
    V = int(np.prod(dims[:-1]))
    net, P, stats = B.calibrated_net(S3D, "fp32")
    data, label, weight = make_inputs(dims, ncls, n, seed=B.SEED_STEP)
    net.zero_gradients(None)
    dense = net.accum_gradients(None, data, label, weight)[0]
    g_dense = net.get_gradients()
    vb = VoxelBatch(np.arange(n + 1) * V, np.tile(np.arange(V, dtype=np.int32), n), data.reshape(-1), label.reshape(-1),
                    weight.reshape(-1), np.zeros(n, np.float32), V)
    net.zero_gradients(None)
    vox = net.accum_gradients_voxels(None, vb)[0]
    assert vox == dense and all(same_bits(v, g_dense[k]) for k, v in net.get_gradients().items())
    assert all(same_bits(v, stats[k]) for k, v in net.get_bn_moving().items())


@pytest.mark.parametrize("shape,prec", [(S3D, "fp32"), (FULL, "fp32"), (FULL, "bf16")], ids=["golden3d-fp32", "full-fp32", "full-bf16"])
def test_logits_pair_replays_the_step(shape, prec):
    import torch
    tag, dims, base, ncls, ns, n = shape
    net, P, stats = B.calibrated_net(shape, prec)
    dd, ld, wd = upload(*make_inputs(dims, ncls, n, seed=B.SEED_STEP))
    net.zero_gradients(None)
    net.accum_gradients(None, dd, ld, wd)
    torch.cuda.synchronize()
    G1 = net._grads.detach().cpu().numpy().copy()
    D = net.debug_tensor("logits:grad")
    net.zero_gradients(None)
    net.forward_logits(None, dd)
    net.backward_logits(None, D)
    torch.cuda.synchronize()
    G2 = net._grads.detach().cpu().numpy().copy()
    assert np.abs(G1).max() > 0 and same_bits(G1, G2), "%d of %d gradient elements differ" % (int((bits(G1) != bits(G2)).sum()), G1.size)


def test_input_gradient_against_autograd_with_fixed_statistics():
    """Arbitrary d-logits: parameter gradients and d(input) against torch autograd through the fixed-statistics network, at the
    rule tests/test_ext_loss_gpu.py::test_arbitrary_dlogits_against_oracle uses in batch mode (floor: the numpy oracle in fp32
    under the same swap)."""
    tag, dims, base, ncls, ns, n = S3D
    net, P, stats = B.calibrated_net(S3D, "fp32")
    data, _, _ = make_inputs(dims, ncls, n, seed=B.SEED_STEP)
    rng = np.random.default_rng(9)
    dl = (rng.standard_normal((n,) + tuple(dims[:-1]) + (ncls,)) / np.prod(dims[:-1])).astype(np.float32)
    g_ref, din_ref, _ = B.torch_frozen_step(P, S3D, stats, data, None, None, dlogits=dl)
    P32 = type(P)((k, v.astype(np.float32)) for k, v in P.items())
    with B.frozen_step_oracle(B.bn_scopes(len(dims) - 1, dims[-1], base, ncls, ns), stats):
        _, tape32 = O.forward(P32, O.reshape_inputs(dims, data)[0].astype(np.float32), base, num_strides=ns)
        g_32, din_32 = O.backward(P32, tape32, dl)
    net.zero_gradients(None)
    net.forward_logits(None, data)
    din = net.backward_logits(None, dl, want_input_grad=True).cpu().numpy()
    g = net.get_gradients()
    bad = []
    for k in g_ref:
        e, floor = l2_rel(g[k], g_ref[k]), l2_rel(g_32[k], g_ref[k])
        if e > min(max(2e-3, 4 * floor), 5e-2):
            bad.append((k, e, floor))
    e, floor = l2_rel(din, din_ref), l2_rel(din_32, din_ref)
    print("frozen input gradient: l2_rel %.3g (fp32 oracle %.3g)" % (e, floor))
    if e > min(max(2e-3, 4 * floor), 5e-2):
        bad.append(("d data", e, floor))
    assert not bad, bad


def test_refusals_and_the_handle_works_afterwards():
    tag, dims, base, ncls, ns, n = S3D
    lib = _lib.load()
    data, label, weight = make_inputs(dims, ncls, n, seed=B.SEED_STEP)
    net = B.build_net(S3D, "fp32")
    net._ensure_handle(n)
    with pytest.raises(_lib.UrsnError, match="not frozen"):      # needs frozen mode on
        _lib.check(lib.ursn_bn_frozen_train(net._handle, 1))
    net.set_bn_mode('moving')
    with pytest.raises(_lib.UrsnError, match="forward-only"):    # frozen alone still refuses to train
        net.accum_gradients(None, data, label, weight)
    net.set_bn_mode('frozen')
    net.zero_gradients(None)
    first = net.accum_gradients(None, data, label, weight)[0]
    g_first = net.get_gradients()
    with pytest.raises(_lib.UrsnError, match="last forward was frozen"):
        _lib.check(lib.ursn_bn_update(net._handle, 0.1, None))
    net.forward_logits(None, data)
    with pytest.raises(_lib.UrsnError, match="last forward was frozen"):
        _lib.check(lib.ursn_bn_update(net._handle, 0.1, None))
    # turning frozen off clears the training switch: 'moving' afterwards is forward-only again
    _lib.check(lib.ursn_bn_set_frozen(net._handle, 0))
    _lib.check(lib.ursn_bn_set_frozen(net._handle, 1))
    with pytest.raises(_lib.UrsnError, match="forward-only"):
        net.accum_gradients(None, data, label, weight)
    net.set_bn_mode('frozen')
    net.zero_gradients(None)
    again = net.accum_gradients(None, data, label, weight)[0]
    assert again == first and all(same_bits(v, g_first[k]) for k, v in net.get_gradients().items())


# ---- 6. state independence ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape,prec", [(FULL, "fp32"), (FULL, "bf16"), (PAD, "fp32")],
                         ids=["full3d_f8_ns5-fp32", "full3d_f8_ns5-bf16", "2d_f6_pad_lanes-fp32"])
def test_frozen_step_does_not_depend_on_workspace_fill_or_history(shape, prec):
    """The method of tests/test_bn_moving_gpu.py::test_frozen_results_do_not_depend_on_workspace_fill_or_history on a frozen
    TRAINING step: zero, NaN and huge-finite workspace, and after other calls on the handle (a batch-mode step on other data,
    an evaluation, an earlier frozen step)."""
    import torch
    tag, dims, base, ncls, ns, n = shape
    cfg = make_cfg(dims, base, ncls, ns, n, trainable=1, use_weight=1, bf16=(prec == "bf16"))
    lib = _lib.load()
    total = ctypes.c_int64(0)
    _lib.check(lib.ursn_bn_moving_size(ctypes.byref(cfg), ctypes.byref(total)))
    rng = np.random.default_rng(37)
    host, info, off, i = np.zeros(total.value, np.float32), _lib.ursn_layer_info(), 0, 0
    while lib.ursn_query_layer(ctypes.byref(cfg), i, ctypes.byref(info)) == 0:
        c = int(info.cout)
        host[off:off + c] = rng.normal(0.0, 0.3, c)
        host[off + c:off + 2 * c] = rng.uniform(0.2, 2.0, c)
        off, i = off + 2 * c, i + 1
    assert off == total.value
    (moving,) = upload(host)
    A, Bt = upload(*make_inputs(dims, ncls, n, seed=43)), upload(*make_inputs(dims, ncls, n, seed=44))
    ref = None
    for fill, history in (("zero", False), ("nan", False), ("big", False), ("nan", True)):
        with Handle(cfg, fill) as h:
            _lib.check(lib.ursn_bn_attach(h.handle, ctypes.c_void_p(moving.data_ptr())))
            if history:
                h.accum_step(Bt[0], Bt[1], Bt[2], n)                      # batch mode, other data
                _lib.check(lib.ursn_bn_set_frozen(h.handle, 1))
                h.eval(Bt[0], Bt[1], Bt[2], n)
                _lib.check(lib.ursn_bn_frozen_train(h.handle, 1))
                h.accum_step(Bt[0], Bt[1], Bt[2], n)                      # a frozen step on other data
                h.zero_grad()
            _lib.check(lib.ursn_bn_set_frozen(h.handle, 1))
            _lib.check(lib.ursn_bn_frozen_train(h.handle, 1))
            got = h.accum_step(A[0], A[1], A[2], n)
            assert np.isfinite(got["metrics"]).all() and np.isfinite(got["grads"]).all(), (fill, history)
            if ref is None:
                ref = got
            else:
                compare_outputs("%s fill=%s history=%s" % (tag, fill, history), ref, got, h, h)
    assert same_bits(moving.cpu().numpy(), host)
    torch.cuda.synchronize()
