"""Voxel-list scores on the device (include/uresnet_hip.h, ABI 9; vscores_kernel in voxel_io.hip): ursn_scores_at_voxels against
an fp64 softmax in numpy, ursn_infer_voxels / ssnet_base.inference_voxel_scores bit for bit against the dense heads of both
plans, and the SPARSE_SCORES ana driver against the dense and the SPARSE_IO drivers.

Op-level bounds: scores within 1e-6 (fp32 logits, expf) / 1e-5 (bf16 logits, __expf) absolute of the fp64 softmax, the bounds
tests/test_model_shapes_gpu.py holds the dense heads to; pred / ana exact (the inputs carry no fp64 top-2 margin and no
|logit 1 - logit 2| below 1e-5: asserted on the host for every case, smallest margin of all cases when written 2.3e-4); rows of
out-of-range indices all zero; the bytes around every output untouched.  Net level: every comparison is on bit patterns."""
import ctypes

import numpy as np
import pytest

from _abi import _Guarded, same_bits
from uresnet_amd import _lib, uresnet
from uresnet_amd import synthetic_io as sio
from uresnet_amd.ssnet import VoxelBatch

pytestmark = pytest.mark.gpu

GUARD = 4096
BLOCK = 256          # threads of a vscores workgroup: 257 entries are one over a block multiple

# (dtype, z_cstride, classes): fp32 4-padded logits (one 16-byte load), fp32 stride 8, bf16 pieces of 8
LAYOUTS = [(0, 4, c) for c in (1, 3, 4)] + [(0, 8, c) for c in (1, 3, 4, 6, 8)] + [(1, 8, c) for c in (1, 3, 4, 6, 8)]
VOXELS = (1, 63, 4097)
# entries per event: M = 0, one over a block multiple, an empty first / middle / last event, all empty
COUNTS = [(0,), (BLOCK + 1,), (0, 5, BLOCK + 1), (7, 0, 3), (BLOCK + 1, 2, 0), (0, 0, 0)]


def _bf16_round(a):
    """fp32 -> the nearest bf16 (ties to even), as fp32 values and as uint16 bit patterns."""
    u = np.ascontiguousarray(a, np.float32).view(np.uint32).astype(np.uint64)
    r = ((u + 0x7FFF + ((u >> 16) & 1)) >> 16).astype(np.uint16)
    return (r.astype(np.uint32) << 16).view(np.float32), r


def _op_case(dtype, cs, ncls, V, counts, seed, with_bn=True):
    """Inputs of one ursn_scores_at_voxels call and its fp64 expectation (host only)."""
    rng = np.random.default_rng(seed)
    n = len(counts)
    z = (2.0 * rng.standard_normal((n * V, cs))).astype(np.float32)
    zbits = None
    if dtype == 1:
        z, zbits = _bf16_round(z)
    mean = rng.uniform(-0.5, 0.5, ncls).astype(np.float32)
    rstd = rng.uniform(0.5, 1.5, ncls).astype(np.float32)
    beta = rng.uniform(-0.5, 0.5, ncls).astype(np.float32)
    data = rng.uniform(0.0, 3.0, (n, V)).astype(np.float32)
    index, off = [], [0]
    for i, m in enumerate(counts):
        idx = np.sort(rng.integers(0, V, m)).astype(np.int32)      # op level: the kernel does not need distinct indices
        if m >= 3:                                                  # two entries outside [0, V)
            idx[int(rng.integers(0, m))] = -1
            idx[int(rng.integers(0, m))] = V
        index.append(idx)
        off.append(off[-1] + m)
    index = np.concatenate(index).astype(np.int32) if off[-1] else np.zeros(0, np.int32)
    off = np.asarray(off, np.int64)
    M = int(off[-1])
    event = np.repeat(np.arange(n), np.diff(off))
    ok = (index >= 0) & (index < V)
    p = event * V + np.where(ok, index, 0)
    raw = z[p, :ncls].astype(np.float64)
    if with_bn:
        r64 = rstd.astype(np.float64)
        logit = raw * r64 + (beta.astype(np.float64) - mean.astype(np.float64) * r64)
    else:
        logit = raw
    e = np.exp(logit - logit.max(axis=1, keepdims=True)) if M else np.zeros((0, ncls))
    scores = e / e.sum(axis=1, keepdims=True) if M else e
    pred = scores.argmax(axis=1) if M else np.zeros(0, np.int64)
    margin = np.inf
    if M and ncls >= 2 and ok.any():
        srt = np.sort(logit[ok], axis=1)
        margin = float((srt[:, -1] - srt[:, -2]).min())
    ana = None
    if ncls >= 3:
        rule = (scores[:, 1] > scores[:, 2]) * 1 + (scores[:, 2] >= scores[:, 1]) * 2
        ana = rule * (data.reshape(-1)[p] > np.float32(1.0))
        if ok.any():
            margin = min(margin, float(np.abs(logit[ok, 1] - logit[ok, 2]).min()))
        ana = np.where(ok, ana, 0).astype(np.uint8)
    scores = np.where(ok[:, None], scores, 0.0)
    pred = np.where(ok, pred, 0).astype(np.uint8)
    return dict(n=n, V=V, ncls=ncls, cs=cs, dtype=dtype, z=zbits if dtype == 1 else z, mean=mean, rstd=rstd, beta=beta,
                data=data, offsets=off, index=index, M=M, ok=ok, scores=scores, pred=pred, ana=ana, margin=margin,
                with_bn=with_bn)


def _dev(a):
    import torch
    a = np.ascontiguousarray(a)
    if a.size == 0:
        return torch.empty(16, dtype=torch.uint8, device="cuda")
    if a.dtype == np.uint16:
        return torch.from_numpy(a.view(np.int16)).cuda()
    return torch.from_numpy(a).cuda()


def _run_op(lib, c, want):
    """One ursn_scores_at_voxels call into 0xFF-filled outputs that hold exactly M rows between canary guards."""
    import torch
    keep = {k: _dev(c[k]) for k in ("z", "mean", "rstd", "beta", "data", "offsets", "index")}
    d = _lib.ursn_vscores_desc()
    d.n, d.voxels, d.ncls = c["n"], c["V"], c["ncls"]
    d.z, d.z_cstride, d.dtype = keep["z"].data_ptr(), c["cs"], c["dtype"]
    if c["with_bn"]:
        d.mean, d.rstd, d.beta = (keep[k].data_ptr() for k in ("mean", "rstd", "beta"))
    d.data, d.offsets, d.index = (keep[k].data_ptr() for k in ("data", "offsets", "index"))
    M = c["M"]
    size = {"scores": M * c["ncls"] * 4, "pred": M, "ana": M}
    out = {w: _Guarded(size[w], GUARD, 0xFF) for w in want}
    torch.cuda.synchronize()
    ptr = lambda w: ctypes.c_void_p(out[w].ptr) if w in out else None
    _lib.check(lib.ursn_scores_at_voxels(ctypes.byref(d), ptr("scores"), ptr("pred"), ptr("ana"), None))
    torch.cuda.synchronize()
    assert lib.ursn_last_kernel_name() == b"vscores"
    res = {}
    for w, g in out.items():
        assert g.guards_intact() == (True, True), w
        raw = g.view.cpu().numpy().copy()
        res[w] = raw.view(np.float32).reshape(M, c["ncls"]) if w == "scores" else raw
    return res


def _check_op(c, got):
    tol = 1e-5 if c["dtype"] == 1 else 1e-6
    assert c["margin"] >= 1e-5, "test input with a near tie: margin %.3g" % c["margin"]
    if "scores" in got:
        assert got["scores"].shape == c["scores"].shape
        if c["M"]:
            err = float(np.abs(got["scores"].astype(np.float64) - c["scores"]).max())
            assert err <= tol, err
            assert not got["scores"][~c["ok"]].view(np.uint32).any(), "rows of out-of-range indices must be zero bits"
    if "pred" in got:
        assert np.array_equal(got["pred"], c["pred"])
    if "ana" in got:
        assert np.array_equal(got["ana"], c["ana"])


@pytest.mark.parametrize("dtype, cs, ncls", LAYOUTS, ids=["%s_cs%d_%dcls" % ("bf16" if d else "fp32", s, c) for d, s, c in LAYOUTS])
def test_scores_at_voxels_against_fp64(lib, dtype, cs, ncls):
    seed = 1000 * dtype + 100 * cs + 10 * ncls
    smallest = np.inf
    for V in VOXELS:
        for j, counts in enumerate(COUNTS):
            c = _op_case(dtype, cs, ncls, V, counts, seed + 7 * j + V)
            want = ("scores", "pred") + (("ana",) if ncls >= 3 else ())
            _check_op(c, _run_op(lib, c, want))
            smallest = min(smallest, c["margin"])
    # every subset of the outputs gives the same rows; logits given directly (NULL mean)
    c = _op_case(dtype, cs, ncls, 4097, (BLOCK + 1, 2, 0), seed + 5)
    full = _run_op(lib, c, ("scores", "pred") + (("ana",) if ncls >= 3 else ()))
    for w in full:
        one = _run_op(lib, c, (w,))
        assert np.array_equal(one[w].view(np.uint8), full[w].view(np.uint8)), w
    c = _op_case(dtype, cs, ncls, 63, (7, 0, 3), seed + 6, with_bn=False)
    _check_op(c, _run_op(lib, c, ("scores", "pred")))
    print("smallest fp64 margin of the inputs: %.3g" % smallest)


# ---- net level ------------------------------------------------------------------------------------------------------------
NET_CASES = [
    # dims, F, num_strides, classes, precision, events fed, plan max_batch (0: as fed)
    ((16, 16, 16, 1), 4, 2, 3, "fp32", 2, 0),
    ((32, 32, 1), 16, 3, 3, "fp32", 2, 0),
    ((32, 32, 32, 1), 8, 3, 6, "fp32", 3, 4),
    ((32, 32, 32, 1), 8, 3, 3, "bf16", 2, 0),
    ((32, 32, 1), 8, 3, 4, "bf16", 2, 0),
]
_NET_IDS = ["%s_f%d_%dcls_%s" % ("x".join(str(d) for d in c[0][:-1]), c[1], c[3], c[4]) for c in NET_CASES]
_in_cache = {}


def _inputs(dims, ncls, n, first=0):
    key = (dims, ncls, n, first)
    if key not in _in_cache:
        ev = [sio.lartpc_sparse(dims, ncls, first + e) for e in range(n)]
        data, label, weight = (np.stack([e[j] for e in ev]) for j in range(3))
        weight = weight / weight.sum(axis=1, keepdims=True)
        vb = VoxelBatch.concat([sio.dense_to_voxels(data[i], label[i], weight[i]) for i in range(n)]).validate()
        _in_cache[key] = (data, label, weight, vb)
    return _in_cache[key]


def _net(dims, F, ns, ncls, prec, max_batch=0, trainable=True):
    net = uresnet(dims=list(dims), num_class=ncls, base_num_outputs=F, num_strides=ns)
    net.construct(trainable=trainable, use_weight=True, learning_rate=1e-3, seed=7, precision=prec)
    if max_batch:
        net._ensure_handle(max_batch)
    return net


def _f32(x):
    return np.asarray([x], np.float32)


def _same_result(a, b):
    if set(a) != set(b):
        return False
    for k in a:
        if k.startswith("acc"):
            if not same_bits(_f32(a[k]), _f32(b[k])):
                return False
        elif not all(x.dtype == y.dtype and x.shape == y.shape and np.array_equal(x.view(np.uint8), y.view(np.uint8))
                     for x, y in zip(a[k], b[k])):
            return False
    return True


def _records(lib, net):
    cnt = ctypes.c_int64(0)
    _lib.check(lib.ursn_profile_read(net._handle, None, 0, ctypes.byref(cnt)))
    recs = (_lib.ursn_prof_rec * max(int(cnt.value), 1))()
    _lib.check(lib.ursn_profile_read(net._handle, recs, int(cnt.value), ctypes.byref(cnt)))
    return [(r.kernel.decode(), int(r.pass_), float(r.ms)) for r in recs[:int(cnt.value)]]


@pytest.mark.parametrize("case", NET_CASES, ids=_NET_IDS)
def test_inference_voxel_scores_equals_the_dense_heads_bit_for_bit(lib, case):
    dims, F, ns, ncls, prec, n, mb = case
    data, label, weight, vb = _inputs(dims, ncls, n)
    V = vb.voxels
    net = _net(dims, F, ns, ncls, prec, mb)
    sm, acc_all, acc_nz = net.inference(None, data, label)
    lab, acc_all_l, acc_nz_l = net.inference_labels(None, data, label)
    h2d = net.feed_stats['h2d_bytes']
    r = net.inference_voxel_scores(None, vb)
    M, pad = int(vb.offsets[-1]), lambda b: (b + 15) & ~15
    assert net.feed_stats['h2d_bytes'] - h2d == pad(8 * (n + 1)) + 3 * pad(4 * M)      # offsets, index, value, label: nothing dense
    assert set(r) == {'index', 'scores', 'pred', 'ana', 'acc_all', 'acc_nonzero'}
    assert same_bits(_f32(r['acc_all']), _f32(acc_all_l)) and same_bits(_f32(r['acc_nonzero']), _f32(acc_nz_l))
    assert same_bits(_f32(r['acc_all']), _f32(acc_all)) and same_bits(_f32(r['acc_nonzero']), _f32(acc_nz))
    seen = set()
    for i in range(n):
        index = vb.index[vb.offsets[i]:vb.offsets[i + 1]]
        assert index.size > 0 and np.array_equal(r['index'][i], index)
        assert r['scores'][i].dtype == np.float32 and r['pred'][i].dtype == np.uint8 and r['ana'][i].dtype == np.uint8
        assert same_bits(r['scores'][i], np.ascontiguousarray(sm[i].reshape(V, ncls)[index]))
        assert np.array_equal(r['ana'][i], lab[i].reshape(-1)[index].astype(np.uint8))
        assert np.array_equal(r['pred'][i], r['scores'][i].argmax(axis=1).astype(np.uint8))
        seen |= set(np.unique(r['ana'][i]))
    assert seen - {0}, "the ana rule never fired: the comparison would be empty"

    # a subset of the outputs and no labels: the same rows, no accuracies
    sub = net.inference_voxel_scores(None, vb, with_labels=False, want=('pred',))
    assert set(sub) == {'index', 'pred'} and all(np.array_equal(a, b) for a, b in zip(sub['pred'], r['pred']))

    # order independence: an accum_gradients step and a batch of another size in between change nothing
    net.zero_gradients(None)
    net.accum_gradients(None, data, label, weight)
    one = _inputs(dims, ncls, 1, first=5)[3]
    net.inference_voxel_scores(None, one)
    assert _same_result(net.inference_voxel_scores(None, vb), r)

    # no dense head without labels: one "vscores" launch recorded as pass 6, the dense head only with labels
    _lib.check(lib.ursn_profile_enable(net._handle, 1))
    net.inference_voxel_scores(None, vb, with_labels=False)
    recs = _records(lib, net)
    assert [k for k, p, _ in recs if p == 6] == ["vscores"], [k for k, p, _ in recs if p == 6]
    assert not any("head" in k for k, _, _ in recs)
    assert lib.ursn_last_kernel_name() == b"vscores"
    net.inference_voxel_scores(None, vb, with_labels=True)
    recs = _records(lib, net)
    assert sorted(k for k, p, _ in recs if p == 6) == sorted(["bhead" if prec == "bf16" else "head", "vscores"])
    _lib.check(lib.ursn_profile_enable(net._handle, 0))
    print("%s: vscores %.4f ms for %d entries" % (_NET_IDS[NET_CASES.index(case)], [ms for k, _, ms in recs if k == "vscores"][0], M))


def test_an_event_without_voxels_and_an_empty_batch():
    dims, ncls = (16, 16, 16, 1), 3
    data, label, weight, vb = _inputs(dims, ncls, 2)
    net = _net(dims, 4, 2, ncls, "fp32", trainable=False)
    full = net.inference_voxel_scores(None, vb)
    a, b = int(vb.offsets[1]), int(vb.offsets[2])
    gap = VoxelBatch([0, 0, b - a], vb.index[a:b], vb.value[a:b], vb.label[a:b], None, None, vb.voxels)
    # BatchNorm runs on batch statistics, so a batch with another first event is another network input: compare with dense
    d2, l2, _ = sio.voxels_to_dense(gap)
    sm = net.inference(None, d2, l2)[0]
    r = net.inference_voxel_scores(None, gap)
    assert r['scores'][0].shape == (0, ncls) and r['pred'][0].shape == (0,) and r['index'][0].shape == (0,)
    assert same_bits(r['scores'][1], np.ascontiguousarray(sm[1].reshape(-1, ncls)[gap.index]))
    none = VoxelBatch([0, 0], [], [], [], None, None, vb.voxels)
    r0 = net.inference_voxel_scores(None, none)
    assert r0['scores'][0].shape == (0, ncls) and r0['ana'][0].shape == (0,) and np.isfinite(r0['acc_all'])
    assert _same_result(net.inference_voxel_scores(None, vb), full)


def test_infer_voxels_refusals_that_need_a_handle(lib):
    import torch
    two = _net((32, 32, 1), 4, 2, 2, "fp32", trainable=False)
    two._ensure_handle(1)
    data = torch.zeros(1, 1024, device="cuda")
    off = torch.zeros(2, dtype=torch.int64, device="cuda")
    idx = torch.zeros(4, dtype=torch.int32, device="cuda")
    out = torch.zeros(64, device="cuda")
    P = lambda t: ctypes.c_void_p(t.data_ptr())
    rc = lib.ursn_infer_voxels(two._handle, P(data), None, 1, P(off), P(idx), 0, P(out), None, P(out), None, None)
    assert rc != 0 and b"needs >= 3 classes" in lib.ursn_last_error()
    with pytest.raises(ValueError):
        two.inference_voxel_scores(None, VoxelBatch([0, 0], [], [], [], None, None, 1024))
    assert lib.ursn_infer_voxels(two._handle, P(data), None, 1, P(off), P(idx), 0, P(out), P(out), None, None, None) == 0
    wide = uresnet(dims=[32, 32, 2], num_class=3, base_num_outputs=4, num_strides=2)
    wide.construct(trainable=False, use_weight=False, seed=7)
    wide._ensure_handle(1)
    data2 = torch.zeros(1, 2048, device="cuda")
    rc = lib.ursn_infer_voxels(wide._handle, P(data2), None, 1, P(off), P(idx), 0, P(out), None, None, None, None)
    assert rc != 0 and b"one input channel" in lib.ursn_last_error()
    with pytest.raises(ValueError) as e:
        wide.inference_voxel_scores(None, VoxelBatch([0, 0], [], [], [], None, None, 1024))
    assert "dims[-1] must be 1" in str(e.value)


# ---- driver ---------------------------------------------------------------------------------------------------------------
def _ana_cfg(tmp_path, tag, sparse, scores):
    inp = tmp_path / "input.cfg"
    inp.write_text("Dims [32, 32, 32, 1]\nNumClass 3\nGenerator 'lartpc_sparse'\nNumEntries 64\n"
                   "Keys {'data': 'data', 'label': 'label', 'weight': 'weight'}\n")
    out = tmp_path / ("ssnet_%s.npy" % tag)
    ana = tmp_path / ("ana_%s.cfg" % tag)
    ana.write_text("NUM_CLASS 3\nBASE_NUM_FILTERS 4\nMAIN_INPUT_CONFIG '%s'\nANA_OUTPUT_CONFIG '%s'\nLOGDIR ''\nSAVE_FILE ''\n"
                   "ITERATIONS 2\nMINIBATCH_SIZE 2\nTRAIN False\nUSE_WEIGHTS False\nSUMMARY_STEPS 0\nCHECKPOINT_STEPS 0\n"
                   "SPARSE_IO %s\nSPARSE_SCORES %s\n" % (inp, out, sparse, scores))
    return ana, out


def _raw_records(path):
    """The .npy records of a file as (array, raw bytes) pairs."""
    recs = []
    with open(str(path), "rb") as f:
        blob = f.read()
    import io
    f = io.BytesIO(blob)
    while f.tell() < len(blob):
        a = f.tell()
        arr = np.load(f)
        recs.append((arr, blob[a:f.tell()]))
    return recs


def test_driver_writes_score_records_and_never_goes_dense(tmp_path, capsys):
    from uresnet_amd.ssnet_trainval import ssnet_trainval
    V = 32 ** 3
    # dense driver, interactive: the softmax of iterations 1 and 2
    cfg, _ = _ana_cfg(tmp_path, "dense", False, False)
    a = ssnet_trainval()
    a.override_config(str(cfg))
    a.initialize()
    dense = [a.ana_step() for _ in range(2)]
    a.reset()
    # SPARSE_IO alone: the (index, class) records as they are today
    cfg, out_sparse = _ana_cfg(tmp_path, "sparse", True, False)
    a = ssnet_trainval()
    a.override_config(str(cfg))
    a.initialize()
    a.batch_process()
    a.reset()
    # SPARSE_IO + SPARSE_SCORES: two batch iterations, then one interactive step
    cfg, out_scores = _ana_cfg(tmp_path, "scores", True, True)
    a = ssnet_trainval()
    a.override_config(str(cfg))
    a.initialize()
    a.batch_process()
    r = a.ana_step()
    stats = dict(a._net.feed_stats)
    a.reset()
    capsys.readouterr()

    old, new = _raw_records(out_sparse), _raw_records(out_scores)
    assert len(old) == 2 * 4 and len(new) == 3 * 6
    for e in range(4):
        it, i = divmod(e, 2)
        (index, index_raw), (cls, cls_raw), (scores, _) = new[3 * e:3 * e + 3]
        assert index_raw == old[2 * e][1] and cls_raw == old[2 * e + 1][1]            # byte for byte, header included
        assert index.dtype == np.int32 and cls.dtype == np.uint8 and index.size > 0
        assert scores.dtype == np.float32 and scores.shape == (index.size, 3)
        assert list(dense[it]['entries']) == [2 * it, 2 * it + 1]
        assert same_bits(scores, np.ascontiguousarray(dense[it]['softmax'][i].reshape(V, 3)[index]))
    for e in (4, 5):                                                                  # the interactive step's records
        index, cls, scores = (x[0] for x in new[3 * e:3 * e + 3])
        assert index.shape == cls.shape and scores.shape == (index.size, 3) and set(np.unique(cls)) <= {1, 2}

    assert set(r) == {'entries', 'acc_all', 'acc_nonzero', 'voxels'}
    assert len(r['voxels']) == 2 and list(r['entries']) == [4, 5]
    for ev, entry in zip(r['voxels'], r['entries']):
        assert set(ev) == {'index', 'value', 'label', 'scores', 'pred'}
        d, l, _ = sio.lartpc_sparse([32, 32, 32, 1], 3, entry)
        index = np.flatnonzero((d != 0) | (l != 0))
        assert np.array_equal(ev['index'], index) and same_bits(ev['value'], d[index]) and same_bits(ev['label'], l[index])
        assert ev['scores'].shape == (index.size, 3) and ev['scores'].dtype == np.float32
        assert np.array_equal(ev['pred'], ev['scores'].argmax(axis=1).astype(np.uint8))
    # three batches of two events went to the device as lists: less than ONE dense event tensor in all
    assert stats['h2d_calls'] == 3 and stats['h2d_bytes'] < V * 4
