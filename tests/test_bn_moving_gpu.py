"""BatchNorm moving statistics on the device: the update against its numpy restatement bit for bit, calibration as the
cumulative mean, tracking as a pure side effect, the frozen forward against the oracle normalising with given statistics, an
event's independence of its batch, every forward-only entry under the mode, the refusals, state independence, the checkpoint
round trip through the driver and the data-parallel average.

Shapes: the two golden shapes (2-D 32^2 F=4 3 strides, 3-D 16^3 F=4 2 strides) at batch 3, one full-depth 3-D 32^3 F=8 5 strides at
batch 2 (deep-level, pointwise, stride-2, transposed branches and the side-stream shortcuts; both precisions) and the 2-D F=6
shape of tests/test_state_independence_gpu.py whose widths are not multiples of 4 (pad lanes; fp32 -- the bf16 plan needs
F % 8 == 0, which also keeps the F=4 golden shapes on fp32)."""
import contextlib
import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest

from oracle import uresnet_np as O
from _abi import Handle, bits, compare_outputs, make_cfg, same_bits, upload
from _net import as_f32_exact, make_inputs, max_rel, oracle_params
from test_bn_moving_host import bn_update_np
from uresnet_amd import _lib, uresnet
from uresnet_amd.ssnet import VoxelBatch, class_stats_from_counts

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

S2D = ("golden2d", (32, 32, 1), 4, 3, 3, 3)        # tag, dims, F, classes, num_strides, batch
S3D = ("golden3d", (16, 16, 16, 1), 4, 3, 2, 3)
FULL = ("full3d_f8_ns5", (32, 32, 32, 1), 8, 3, 5, 2)
PAD = ("2d_f6_pad_lanes", (64, 64, 1), 6, 3, 3, 3)
CASES = [(S2D, "fp32"), (S3D, "fp32"), (FULL, "fp32"), (FULL, "bf16"), (PAD, "fp32")]
IDS = ["%s-%s" % (c[0][0], c[1]) for c in CASES]
EPS = 1e-3


def build(shape, prec, bn_moving=True, decay=0.9, trainable=True, seed=7, use_weight=True):
    tag, dims, base, ncls, ns, n = shape
    net = uresnet(dims=list(dims), num_class=ncls, base_num_outputs=base, num_strides=ns)
    net.construct(trainable=trainable, use_weight=use_weight, learning_rate=1e-2, seed=seed, precision=prec, bn_moving=bn_moving,
                  bn_decay=decay)
    return net


def scopes(net):
    return [name[:-len("/BatchNorm")] for name, _, _ in net._bn_specs]


def layer_stats(net):
    """Every layer's stored mean / rstd of the last forward, as the consumers read them."""
    return [(net.debug_tensor(s + ":mean"), net.debug_tensor(s + ":rstd")) for s in scopes(net)]


def fold(net, moving, stats, momentum):
    """The numpy restatement applied to a get_bn_moving() dict, layer by layer."""
    out = {}
    for s, (mean, rstd) in zip(scopes(net), stats):
        km, kv = s + "/BatchNorm/moving_mean", s + "/BatchNorm/moving_variance"
        out[km], out[kv] = bn_update_np(moving[km], moving[kv], mean, rstd, momentum, EPS)
    return out


def assert_same_dict(got, want, what):
    assert list(got) == list(want), what
    for k in want:
        assert same_bits(got[k], want[k]), "%s: %s differs in %d of %d elements" % (what, k, int((bits(got[k]) != bits(want[k])).sum()),
                                                                                 want[k].size)


def random_stats(net, seed):
    """Plausible statistics: means ~ N(0, 0.3), variances in [0.2, 2]."""
    rng = np.random.default_rng(seed)
    v = {}
    for name, c, _ in net._bn_specs:
        v[name + "/moving_mean"] = rng.normal(0.0, 0.3, c).astype(np.float32)
        v[name + "/moving_variance"] = rng.uniform(0.2, 2.0, c).astype(np.float32)
    return v


# ---- 1. the update is exact ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape,prec", CASES, ids=IDS)
def test_update_equals_the_numpy_restatement_bitwise(shape, prec):
    tag, dims, base, ncls, ns, n = shape
    net = build(shape, prec, decay=0.9)
    momentum = 1.0 - 0.9
    moving = net.get_bn_moving()
    assert all((v == (1.0 if k.endswith("variance") else 0.0)).all() for k, v in moving.items())
    changed = 0
    for it in range(3):
        net.zero_gradients(None)
        for j in range(2):   # gradient accumulation of 2: one update per minibatch, as UPDATE_OPS would run
            data, label, weight = make_inputs(dims, ncls, n, seed=300 + 2 * it + j)
            net.accum_gradients(None, data, label, weight)
            want = fold(net, moving, layer_stats(net), momentum)
            got = net.get_bn_moving()
            assert_same_dict(got, want, "%s iteration %d minibatch %d" % (tag, it, j))
            changed += sum(int(not same_bits(got[k], moving[k])) for k in got)
            moving = got
        net.apply_gradients(None)
    assert changed >= 6 * len(moving) - 12          # every vector moved at every update (bar a constant channel or two)


def test_update_touches_only_its_operands():
    """The statistics vectors are read only -- pad lanes included -- and a bare-op call on a slice leaves its neighbours alone."""
    import torch
    from uresnet_amd import hiprt
    net = build(PAD, "fp32")
    dims, ncls, n = PAD[1], PAD[3], PAD[5]
    lib = _lib.load()

    def raw(name):   # the whole padded vector
        ptr, vox, ch, cs = ctypes.c_void_p(), ctypes.c_int64(), ctypes.c_int32(), ctypes.c_int32()
        _lib.check(lib.ursn_tensor(net._handle, name.encode(), ctypes.byref(ptr), ctypes.byref(vox), ctypes.byref(ch), ctypes.byref(cs)))
        torch.cuda.synchronize()
        buf = (ctypes.c_float * cs.value)()
        hiprt.memcpy_d2h(buf, ptr.value, cs.value * 4)
        return np.frombuffer(buf, dtype=np.float32).copy(), ch.value

    data, label, weight = make_inputs(dims, ncls, n, seed=5)
    net.zero_gradients(None)
    net.set_bn_moving(random_stats(net, 1))
    net._bn_tracking = False
    net.accum_gradients(None, data, label, weight)
    padded = 0
    before = {s + k: raw(s + k) for s in scopes(net) for k in (":mean", ":rstd")}
    _lib.check(lib.ursn_bn_update(net._handle, 0.5, None))
    for name, (vec, ch) in before.items():
        after, _ = raw(name)
        assert same_bits(after, vec), name
        assert (vec[ch:] == 0).all(), name            # pad lanes stay 0
        padded += vec.size - ch
    assert padded > 0
    # the bare op on the middle third of a vector: the other two thirds keep their bits
    rng = np.random.default_rng(2)
    C = 1000
    mean, rstd, mm, mv = upload(rng.normal(0, 1, C), rng.uniform(0.5, 2, C), rng.normal(0, 1, 3 * C), rng.uniform(0.2, 2, 3 * C))
    mm0, mv0 = mm.cpu().numpy(), mv.cpu().numpy()
    _lib.check(lib.ursn_bn_moving_update(mean.data_ptr(), rstd.data_ptr(), mm.data_ptr() + 4 * C, mv.data_ptr() + 4 * C, C, 0.3,
                                         EPS, None))
    torch.cuda.synchronize()
    wm, wv = bn_update_np(mm0[C:2 * C], mv0[C:2 * C], mean.cpu().numpy(), rstd.cpu().numpy(), 0.3, EPS)
    want_m, want_v = mm0.copy(), mv0.copy()
    want_m[C:2 * C], want_v[C:2 * C] = wm, wv
    assert same_bits(mm.cpu().numpy(), want_m) and same_bits(mv.cpu().numpy(), want_v)


# ---- 2. calibration is the cumulative mean ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape,prec", [(S3D, "fp32"), (FULL, "bf16")], ids=["golden3d-fp32", "full3d_f8_ns5-bf16"])
def test_calibration_is_the_cumulative_mean(shape, prec):
    tag, dims, base, ncls, ns, n = shape
    net = build(shape, prec, trainable=False, use_weight=False)
    batches = [make_inputs(dims, ncls, n, seed=70 + k)[0] for k in range(3)]
    stats = []
    for b in batches:      # the same forward, batch by batch: a forward's statistics depend on its input alone
        net.inference(None, b)
        stats.append(layer_stats(net))
    net.set_bn_moving(random_stats(net, 3))          # reset=True starts from 0 / 1 whatever the buffer held
    net.set_bn_mode('moving')
    assert net.bn_calibrate(None, iter(batches)) == 3
    assert net.bn_mode() == 'moving'                 # left as it was found
    want = {k: (np.ones_like(v) if k.endswith("variance") else np.zeros_like(v)) for k, v in net.get_bn_moving().items()}
    for k, st in enumerate(stats):
        want = fold(net, want, st, 1.0 / (k + 1))
    assert_same_dict(net.get_bn_moving(), want, tag)
    # ... which is the mean of the three batch means up to the roundings of the running form
    for s, *per in zip(scopes(net), *stats):
        mean3 = np.mean([p[0].astype(np.float64) for p in per], axis=0)
        assert np.abs(want[s + "/BatchNorm/moving_mean"] - mean3).max() <= 1e-6 * (1.0 + np.abs(mean3).max())


def test_voxel_and_custom_loss_steps_update_once_each():
    """accum_gradients_voxels and accum_gradients_custom enqueue one update after their forward, like accum_gradients."""
    from uresnet_amd import synthetic_io as sio
    tag, dims, base, ncls, ns, n = S3D
    net = build(S3D, "fp32", decay=0.9)
    data, label, weight = make_inputs(dims, ncls, n, seed=81)
    vb = VoxelBatch.concat([sio.dense_to_voxels(data[i], label[i], weight[i]) for i in range(n)])
    moving = net.get_bn_moving()
    net.zero_gradients(None)
    net.accum_gradients_voxels(None, vb)
    want = fold(net, moving, layer_stats(net), 1.0 - 0.9)
    assert_same_dict(net.get_bn_moving(), want, "accum_gradients_voxels")
    assert not same_bits(want["UResNet/conv1/BatchNorm/moving_mean"], moving["UResNet/conv1/BatchNorm/moving_mean"])
    moving = want
    res, _ = net.accum_gradients_custom(None, make_inputs(dims, ncls, n, seed=82)[0], lambda logits: (logits * logits).mean())
    assert np.isfinite(res[1])
    want = fold(net, moving, layer_stats(net), 1.0 - 0.9)
    assert_same_dict(net.get_bn_moving(), want, "accum_gradients_custom")
    assert not same_bits(want["UResNet/conv1/BatchNorm/moving_mean"], moving["UResNet/conv1/BatchNorm/moving_mean"])
    # ... and never run_test / inference
    net.run_test(None, data, label, weight)
    net.inference(None, data)
    assert_same_dict(net.get_bn_moving(), want, "run_test / inference")


# ---- 3. tracking changes nothing else ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape,prec", [(S3D, "fp32"), (FULL, "bf16")], ids=["golden3d-fp32", "full3d_f8_ns5-bf16"])
def test_tracking_changes_nothing_else(shape, prec):
    tag, dims, base, ncls, ns, n = shape
    out = {}
    for on in (False, True):
        net = build(shape, prec, bn_moving=on, decay=0.999)
        metrics = []
        for it in range(2):
            net.zero_gradients(None)
            for j in range(2):
                data, label, weight = make_inputs(dims, ncls, n, seed=500 + 2 * it + j)
                res, _ = net.accum_gradients(None, data, label, weight)
                metrics.append(res[1:])
            grads = net.get_gradients()
            net.apply_gradients(None)
        out[on] = (np.asarray(metrics, np.float32), grads, net.get_variables())
        if on:
            mv = net.get_bn_moving()
            assert any((v != (1.0 if k.endswith("variance") else 0.0)).any() for k, v in mv.items())
        del net
    assert same_bits(out[False][0], out[True][0])
    for i in (1, 2):
        for k in out[False][i]:
            assert same_bits(out[False][i][k], out[True][i][k]), k


# ---- 4. frozen forward against the oracle ----------------------------------------------------------------------------------------
@contextlib.contextmanager
def frozen_oracle(net, stats):
    """oracle.uresnet_np.bn_fwd swapped for a version that normalises with the given statistics (the idiom of
    tests/_net.py::parallel_oracle).  The oracle's forward calls bn_fwd once per layer in TF variable order, the order of the
    moving-statistics table."""
    orig, order = O.bn_fwd, iter(scopes(net))

    def bn_fwd(z, beta, eps=O.BN_EPS):
        s = next(order)
        m = stats[s + "/BatchNorm/moving_mean"].astype(np.float64)
        v = stats[s + "/BatchNorm/moving_variance"].astype(np.float64)
        assert z.shape[-1] == m.size, s
        r = 1.0 / np.sqrt(v + eps)
        xhat = (z - m) * r
        return xhat + beta, (xhat, r)
    O.bn_fwd = bn_fwd
    try:
        yield
    finally:
        O.bn_fwd = orig
    assert next(order, None) is None, "the oracle did not normalise every layer"


def oracle_frozen_forward(net, P, stats, shape, data, quant):
    tag, dims, base, ncls, ns, n = shape
    O.QUANT = O.bf16_round if quant else None
    try:
        with frozen_oracle(net, stats):
            d = O.reshape_inputs(dims, data)[0].astype(np.float64)
            logits, _ = O.forward(P, O._q(d), base, num_strides=ns)
    finally:
        O.QUANT = None
    return logits, O.softmax(logits)


@pytest.mark.parametrize("shape,prec", CASES, ids=IDS)
def test_frozen_forward_against_the_oracle(shape, prec):
    tag, dims, base, ncls, ns, n = shape
    P = as_f32_exact(oracle_params(dims, base, ncls, num_strides=ns))
    data, label, _ = make_inputs(dims, ncls, n, seed=13)
    net = build(shape, prec, trainable=False, use_weight=False)
    net.set_variables(P)
    stats = random_stats(net, 17)
    net.set_bn_moving(stats)
    net.set_bn_mode('moving')
    logits, sm_ref = oracle_frozen_forward(net, P, stats, shape, data, prec == "bf16")
    sm = net.inference_labels(None, data, with_softmax=True)[-1]      # (the call that keeps the feed for debug_tensor)
    # what the consumers read is the moving mean itself, and the reciprocal root the finalise would have formed from the variance
    for s in scopes(net):
        assert same_bits(net.debug_tensor(s + ":mean"), stats[s + "/BatchNorm/moving_mean"]), s
        r = 1.0 / np.sqrt(stats[s + "/BatchNorm/moving_variance"].astype(np.float64) + np.float64(np.float32(EPS)))
        assert max_rel(net.debug_tensor(s + ":rstd"), r) <= 2.0 ** -23, s
    if prec == "bf16":
        e = float(np.abs(sm - sm_ref).max())
        print("%s bf16: softmax max-abs against the bf16-emulating frozen oracle %.2e" % (tag, e))
        assert e <= 6e-2
        return
    c2 = "UResNet/conv2"
    z = net.debug_tensor(c2 + ":z").astype(np.float64)
    got_logits = (z - net.debug_tensor(c2 + ":mean")) * net.debug_tensor(c2 + ":rstd").astype(np.float64) + P[c2 + "/BatchNorm/beta"]
    e_l, e_s = max_rel(got_logits, logits), max_rel(sm, sm_ref)
    print("%s fp32: logits max_rel %.2e, softmax max_rel %.2e" % (tag, e_l, e_s))
    assert e_l < 1e-3 and e_s < 1e-3
    srt = np.sort(logits, axis=-1)
    safe = (srt[..., -1] - srt[..., -2]) > 1e-3
    assert safe.mean() > 0.95
    assert np.array_equal(sm.argmax(-1)[safe], logits.argmax(-1)[safe])


# ---- 5. an event no longer depends on its batch ------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", [S2D, S3D, FULL], ids=[S2D[0], S3D[0], FULL[0]])
def test_an_event_no_longer_depends_on_its_batch(shape):
    """fp32, the plan of the existing batch-split test whose 1e-5 bound this is (tests/test_net_gpu.py).  The inputs (seed 41) were
    checked with the fp64 oracle before they were committed: in batch mode event A alone and inside [A, B, C] differ by 0.24
    (3-D golden shape) and 0.38 (2-D) max_rel, far from the 1e-3 the test asks for."""
    tag, dims, base, ncls, ns, n = shape
    data, _, _ = make_inputs(dims, ncls, n, seed=41)
    net = build(shape, "fp32", trainable=False, use_weight=False)
    net.set_variables(as_f32_exact(oracle_params(dims, base, ncls, num_strides=ns)))
    net.set_bn_moving(random_stats(net, 19))
    res = {}
    for mode in ('batch', 'moving'):
        net.set_bn_mode(mode)
        together = net.inference(None, data)[0][0]
        alone = net.inference(None, data[:1])[0][0]
        res[mode] = max_rel(alone, together)
    print("%s: event alone against the event in its batch, softmax max_rel: batch mode %.2e, moving mode %.2e"
          % (tag, res['batch'], res['moving']))
    assert res['moving'] < 1e-5
    assert res['batch'] > 1e-3


# ---- 6. every forward-only entry honours the mode -----------------------------------------------------------------------------------
@pytest.mark.parametrize("shape,prec", [(S3D, "fp32"), (FULL, "bf16")], ids=["golden3d-fp32", "full3d_f8_ns5-bf16"])
def test_every_forward_only_entry_honours_the_mode(shape, prec):
    tag, dims, base, ncls, ns, n = shape
    V = int(np.prod(dims[:-1]))
    data, label, weight = make_inputs(dims, ncls, n, seed=29)
    net = build(shape, prec, trainable=False, use_weight=True)
    net.set_bn_moving(random_stats(net, 23))
    net.set_bn_mode('batch')
    sm_batch = net.inference(None, data)[0]
    net.set_bn_mode('moving')
    sm, acc_all, acc_nz = net.inference(None, data, label)
    assert float(np.abs(sm - sm_batch).max()) > 1e-3            # the mode is not a no-op on these inputs
    # inference_labels: the reference's rule on this softmax; its own softmax output is the same bits
    lab, a1, a2, sm2 = net.inference_labels(None, data, label, with_softmax=True)
    assert same_bits(sm2, sm) and (a1, a2) == (acc_all, acc_nz)
    want = np.stack([O.ana_label_rule(sm[i], data[i].reshape(dims[:-1])) for i in range(n)])
    assert np.array_equal(lab, want)
    # inference_voxel_scores on the full list: the bits of the softmax at every voxel
    full = VoxelBatch(np.arange(n + 1) * V, np.tile(np.arange(V, dtype=np.int32), n), data.reshape(-1), label.reshape(-1), None, None, V)
    r = net.inference_voxel_scores(None, full, want=('scores', 'pred'))
    scores, pred = np.stack(r['scores']), np.stack(r['pred']).astype(np.int64)
    assert same_bits(scores, np.ascontiguousarray(sm.reshape(n, V, ncls)))
    # inference_stats: counts from that prediction, exactly; score means to 1e-10
    st = net.inference_stats(None, data, label, with_softmax=True)
    assert same_bits(st['softmax'], sm)
    t = label.astype(np.int64)
    conf = np.zeros((n, ncls, ncls), np.int64)
    ssum, ssq = np.zeros((n, ncls)), np.zeros((n, ncls))
    for e in range(n):
        np.add.at(conf[e], (t[e], pred[e]), 1)
        for k in range(ncls):
            s = scores[e][t[e] == k, k].astype(np.float64)
            ssum[e, k], ssq[e, k] = s.sum(), (s * s).sum()
    assert np.array_equal(st['conf'], conf)
    ref = class_stats_from_counts(conf, np.zeros((n, 2), np.int64), ssum, ssq)
    some = ref['npx'] > 0
    assert np.all(np.abs(st['score_mean'] - ref['score_mean'])[some] <= 1e-10 * np.abs(ref['score_mean'])[some])
    # run_test: the accuracies of inference, the weighted cross-entropy of this softmax
    res, _ = net.run_test(None, data, label, weight)
    assert abs(res[1] - acc_all) < 1e-6 and abs(res[2] - acc_nz) < 1e-6
    p = np.take_along_axis(sm.reshape(n, V, ncls).astype(np.float64), t[..., None], axis=-1)[..., 0]
    loss = float((-np.log(p) * weight).sum(axis=1).mean())
    assert abs(res[0] - loss) <= 1e-4 * abs(loss)
    # ... and in batch mode the same calls give the batch-mode softmax again
    net.set_bn_mode('batch')
    assert same_bits(net.inference(None, data)[0], sm_batch)


# ---- 7. refusals -----------------------------------------------------------------------------------------------------------------
def test_refusals_and_the_handle_works_afterwards():
    import torch
    tag, dims, base, ncls, ns, n = S3D
    lib = _lib.load()
    data, label, weight = make_inputs(dims, ncls, n, seed=31)
    net = build(S3D, "fp32")
    net._ensure_handle(n)
    with pytest.raises(_lib.UrsnError, match="no forward has run"):
        _lib.check(lib.ursn_bn_update(net._handle, 0.1, None))
    net.zero_gradients(None)
    first, _ = net.accum_gradients(None, data, label, weight)
    g_first, mv_first = net.get_gradients(), net.get_bn_moving()
    for bad in (-0.5, 1.5, float("nan")):
        with pytest.raises(_lib.UrsnError, match="momentum"):
            _lib.check(lib.ursn_bn_update(net._handle, bad, None))
    net.set_bn_mode('moving')
    with pytest.raises(_lib.UrsnError, match="frozen"):
        net.accum_gradients(None, data, label, weight)
    with pytest.raises(_lib.UrsnError, match="frozen"):
        net.forward_logits(None, data)
    with pytest.raises(_lib.UrsnError, match="frozen"):
        net.backward_logits(None, np.zeros((n,) + dims[:-1] + (ncls,), np.float32))
    with pytest.raises(_lib.UrsnError, match="last forward was frozen"):
        net.inference(None, data)
        _lib.check(lib.ursn_bn_update(net._handle, 0.1, None))
    with pytest.raises(_lib.UrsnError, match="cannot detach"):
        _lib.check(lib.ursn_bn_attach(net._handle, None))
    assert_same_dict(net.get_bn_moving(), mv_first, "refused calls wrote the moving buffer")
    assert all(same_bits(a, g_first[k]) for k, a in net.get_gradients().items())
    # frozen without a buffer, at both levels
    bare = build(S3D, "fp32", bn_moving=False)
    bare._ensure_handle(n)
    with pytest.raises(_lib.UrsnError, match="no moving buffer"):
        _lib.check(lib.ursn_bn_set_frozen(bare._handle, 1))
    with pytest.raises(_lib.UrsnError, match="no moving buffer"):
        _lib.check(lib.ursn_bn_update(bare._handle, 0.1, None))
    with pytest.raises(RuntimeError, match="no moving statistics"):
        bare.set_bn_mode('moving')
    # the handles work normally afterwards: the same step gives the same bits, and the tracked net updates again
    for x in (net, bare):
        x.set_bn_mode('batch')
        x.zero_gradients(None)
    net.set_bn_moving({k: (np.ones_like(v) if k.endswith("variance") else np.zeros_like(v)) for k, v in mv_first.items()})
    again, _ = net.accum_gradients(None, data, label, weight)
    assert again == first and all(same_bits(a, g_first[k]) for k, a in net.get_gradients().items())
    assert_same_dict(net.get_bn_moving(), mv_first, "the update after the refusals")
    bare.set_variables(net.get_variables())
    third, _ = bare.accum_gradients(None, data, label, weight)
    assert third == first
    torch.cuda.synchronize()


# ---- 8. state independence -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape,prec", [(FULL, "fp32"), (FULL, "bf16"), (PAD, "fp32")],
                         ids=["full3d_f8_ns5-fp32", "full3d_f8_ns5-bf16", "2d_f6_pad_lanes-fp32"])
def test_frozen_results_do_not_depend_on_workspace_fill_or_history(shape, prec):
    import torch
    tag, dims, base, ncls, ns, n = shape
    cfg = make_cfg(dims, base, ncls, ns, n, trainable=0, use_weight=1, bf16=(prec == "bf16"))
    lib = _lib.load()
    total = ctypes.c_int64(0)
    _lib.check(lib.ursn_bn_moving_size(ctypes.byref(cfg), ctypes.byref(total)))
    rng = np.random.default_rng(37)
    host, info, off = np.zeros(total.value, np.float32), _lib.ursn_layer_info(), 0
    i = 0
    while lib.ursn_query_layer(ctypes.byref(cfg), i, ctypes.byref(info)) == 0:
        c = int(info.cout)
        host[off:off + c] = rng.normal(0.0, 0.3, c)
        host[off + c:off + 2 * c] = rng.uniform(0.2, 2.0, c)
        off, i = off + 2 * c, i + 1
    assert off == total.value
    (moving,) = upload(host)
    A, B = upload(*make_inputs(dims, ncls, n, seed=43)), upload(*make_inputs(dims, ncls, n, seed=44))

    def frozen_calls(h):
        out = {"infer": h.infer(A[0], A[1], n), "eval": h.eval(A[0], A[1], A[2], n)}
        if ncls >= 3:
            out["infer_labels"] = h.infer_labels(A[0], A[1], n)
        return out

    ref = None
    for fill, interleave in (("zero", False), ("nan", False), ("nan", True)):
        with Handle(cfg, fill) as h:
            _lib.check(lib.ursn_bn_attach(h.handle, ctypes.c_void_p(moving.data_ptr())))
            _lib.check(lib.ursn_bn_set_frozen(h.handle, 1))
            if interleave:      # a batch-mode call on other data overwrites every layer's statistics in between
                frozen_calls(h)
                _lib.check(lib.ursn_bn_set_frozen(h.handle, 0))
                h.eval(B[0], B[1], B[2], n)
                _lib.check(lib.ursn_bn_set_frozen(h.handle, 1))
            got = frozen_calls(h)
            for k, o in got.items():
                assert np.isfinite(o["softmax_out"]).all() if "softmax_out" in o else True, (fill, k)
            if ref is None:
                ref = got
            else:
                for k in ref:
                    compare_outputs("%s %s fill=%s interleave=%s" % (tag, k, fill, interleave), ref[k], got[k], h, h)
    assert same_bits(moving.cpu().numpy(), host)      # frozen calls only read the buffer
    torch.cuda.synchronize()


# ---- 9. checkpoint round trip through the driver ----------------------------------------------------------------------------------
_ANA_CHILD = r"""
import sys
import numpy as np
root, cfg_moving, cfg_plain, cfg_avoid, out = sys.argv[1:6]
sys.path.insert(0, root)
from uresnet_amd.ssnet_trainval import ssnet_trainval
res = {}
for tag, cfg in (("moving", cfg_moving), ("plain", cfg_plain), ("avoid", cfg_avoid)):
    a = ssnet_trainval()
    a.override_config(cfg)
    a.initialize()
    assert a._net.bn_mode() == 'moving'
    for k, v in a._net.get_bn_moving().items():
        res[tag + "|" + k.replace("/", "|")] = v
    if tag == "moving":
        a.batch_process()
    a.reset()
np.savez(out, **res)
"""


def test_checkpoint_round_trip_through_the_driver(tmp_path, capsys):
    from uresnet_amd import synthetic_io as sio
    from uresnet_amd.ssnet_trainval import ssnet_trainval
    dims = [32, 32, 32, 1]                     # the driver builds the full-depth net: 5 strides
    inp = tmp_path / "input.cfg"
    inp.write_text("Dims %s\nNumClass 3\nGenerator 'lartpc_sparse'\nNumEntries 32\n"
                   "Keys {'data': 'data', 'label': 'label', 'weight': 'weight'}\n" % dims)
    common = "NUM_CLASS 3\nBASE_NUM_FILTERS 4\nMAIN_INPUT_CONFIG '%s'\nMINIBATCH_SIZE 2\nSUMMARY_STEPS 0\n" % inp
    cfg = tmp_path / "train.cfg"
    cfg.write_text(common + "LOGDIR ''\nSAVE_FILE '%s'\nITERATIONS 2\nNUM_MINIBATCHES 2\nLEARNING_RATE 0.001\nTRAIN True\n"
                   "USE_WEIGHTS True\nREPORT_STEPS 1\nCHECKPOINT_STEPS 2\nBN_MOVING True\nBN_DECAY 0.9\n" % (tmp_path / "ckpt" / "uresnet"))
    t = ssnet_trainval()
    t.override_config(str(cfg))
    t.initialize()
    t.batch_process()
    assert "saved @" in capsys.readouterr().out
    tnet = t._net
    names = tnet.bn_moving_names()
    with np.load(str(tmp_path / "ckpt" / "uresnet-1.npz")) as f:
        saved = {k: f[k] for k in f.files}
    assert set(saved) == set(tnet.variable_names()) | set(names)
    live = tnet.get_bn_moving()
    assert all(same_bits(saved[k], live[k]) for k in names)
    assert any((saved[k] != (1.0 if k.endswith("variance") else 0.0)).any() for k in names)      # four updates happened
    # the saving process's frozen output, on the plan the ana driver will build (not trainable, no weights)
    ref = uresnet(dims=dims, num_class=3, base_num_outputs=4)
    ref.construct(trainable=False, use_weight=False, bn_moving=True)
    ref.set_variables({k: saved[k] for k in tnet.variable_names()})
    ref.set_bn_moving({k: saved[k] for k in names})
    ref.set_bn_mode('moving')
    pair = np.stack([sio.lartpc_sparse(dims, 3, e)[0] for e in range(2)]).reshape(2, -1)
    want = ref.inference_labels(None, pair)[0]
    t.reset()
    # a snapshot without the arrays, as a run without BN_MOVING writes it
    np.savez(str(tmp_path / "ckpt" / "plain-1.npz"), **{k: saved[k] for k in tnet.variable_names()})
    out = tmp_path / "labels.npy"
    ana = "LOGDIR ''\nSAVE_FILE ''\nITERATIONS 1\nTRAIN False\nUSE_WEIGHTS False\nCHECKPOINT_STEPS 0\nANA_BN 'moving'\n"
    cfg_m, cfg_p, cfg_a = tmp_path / "ana_moving.cfg", tmp_path / "ana_plain.cfg", tmp_path / "ana_avoid.cfg"
    avoided = ["UResNet/conv0/BatchNorm/moving_mean", "UResNet/deconv0/BatchNorm/moving_variance"]
    cfg_a.write_text(common + ana + "LOAD_FILE '%s'\nAVOID_LOAD_PARAMS %r\n" % (tmp_path / "ckpt" / "uresnet-1", [avoided[0], avoided[1] + ":0"]))
    cfg_m.write_text(common + ana + "LOAD_FILE '%s'\nANA_OUTPUT_CONFIG '%s'\n" % (tmp_path / "ckpt" / "uresnet-1", out))
    cfg_p.write_text(common + ana + "LOAD_FILE '%s'\n" % (tmp_path / "ckpt" / "plain-1"))
    res = tmp_path / "child.npz"
    p = subprocess.run([sys.executable, "-c", _ANA_CHILD, ROOT, str(cfg_m), str(cfg_p), str(cfg_a), str(res)], stdout=subprocess.PIPE,
                       stderr=subprocess.PIPE, text=True, timeout=600)
    assert p.returncode == 0, p.stderr[-3000:]
    # the snapshot without the arrays restores, and says what 'moving' then normalises with
    assert p.stdout.count("no BatchNorm moving statistics loaded") == 1 and "bn_calibrate" in p.stdout
    with np.load(str(res)) as f:
        child = {k: f[k] for k in f.files}
    for k in names:
        assert same_bits(child["moving|" + k.replace("/", "|")], saved[k]), k
        plain = child["plain|" + k.replace("/", "|")]
        assert (plain == (1.0 if k.endswith("variance") else 0.0)).all(), k
        avoid = child["avoid|" + k.replace("/", "|")]      # AVOID_LOAD_PARAMS (with or without TF's ':0'): those keep 0 / 1
        if k in avoided:
            assert (avoid == (1.0 if k.endswith("variance") else 0.0)).all() and not same_bits(avoid, saved[k]), k
        else:
            assert same_bits(avoid, saved[k]), k
    with open(str(out), "rb") as f:
        for e in range(2):
            got = np.load(f)
            assert got.shape == (32, 32, 32) and same_bits(got, np.ascontiguousarray(want[e])), e


# ---- 10. data parallel -----------------------------------------------------------------------------------------------------------
_RANK = r"""
import os, sys
import numpy as np
root, out = sys.argv[1], sys.argv[2]
sys.path.insert(0, root); sys.path.insert(0, root + "/tests")
import torch
import torch.distributed as dist
from _net import make_inputs
from uresnet_amd import uresnet
rank = int(os.environ["RANK"])
dist.init_process_group("gloo", rank=rank, world_size=2)
dims, base, ncls, ns = (16, 16, 16, 1), 4, 3, 2
net = uresnet(dims=list(dims), num_class=ncls, base_num_outputs=base, num_strides=ns)
net.construct(trainable=True, use_weight=True, learning_rate=1e-2, seed=7, bn_moving=True, bn_decay=0.9)
net.zero_gradients(None)
net.accum_gradients(None, *make_inputs(dims, ncls, 2, seed=60 + rank))
own = net.get_bn_moving()
net.apply_gradients(None)
after = net.get_bn_moving()
res = {"own|" + k.replace("/", "|"): v for k, v in own.items()}
res.update({"after|" + k.replace("/", "|"): v for k, v in after.items()})
np.savez(out, **res)
dist.barrier()
dist.destroy_process_group()
"""


def test_data_parallel_ranks_average_their_moving_statistics(tmp_path):
    env = dict(os.environ, MASTER_ADDR="127.0.0.1", MASTER_PORT=str(29900 + os.getpid() % 90), WORLD_SIZE="2",
               HSA_ENABLE_IPC_MODE_LEGACY="0")
    outs = [str(tmp_path / ("rank%d.npz" % r)) for r in range(2)]
    procs = [subprocess.Popen([sys.executable, "-c", _RANK, ROOT, outs[r]], env=dict(env, RANK=str(r)), stdout=subprocess.PIPE,
                              stderr=subprocess.PIPE, text=True) for r in range(2)]
    for p in procs:
        so, se = p.communicate(timeout=600)
        assert p.returncode == 0, se[-2000:]
    a, b = np.load(outs[0]), np.load(outs[1])
    keys = [k[len("own|"):] for k in a.files if k.startswith("own|")]
    assert len(keys) == 2 * 25            # 25 conv-like layers at 2 strides
    differ = 0
    for k in keys:
        assert same_bits(a["after|" + k], b["after|" + k]), ("ranks diverged", k)
        want = (a["own|" + k] + b["own|" + k]) * np.float32(0.5)
        assert want.dtype == np.float32 and same_bits(a["after|" + k], want), k
        differ += int(not same_bits(a["own|" + k], b["own|" + k]))
    assert differ >= len(keys) - 2       # the ranks saw different minibatches
