"""Per-event, per-class analysis statistics on the device (include/uresnet_hip.h; cstats_kernel in ana_stats.hip).

Op level: ursn_class_stats against ursn_scores_at_voxels on the same z with a list that names every voxel -- the kernel-independent
bits of scores and pred -- from which numpy forms conf / other / nonzero and fp64 sums.  Counts are exactly equal.  score_sum and
score_sq are within 1e-10 relative: both sides are fp64 sums of the same fp32 values, a fixed-order sum of m non-negative terms is
within m * 2^-53 relative, m <= 2e4 here, so about 2e-12.  The derived score_std is within 1e-6 absolute: the variance is a
difference of two quantities each good to about 1e-15, so good to about 1e-14 absolute, and its square root to <= 1e-7 when the
true std is 0.
Net level: ssnet_base.inference_stats against inference_voxel_scores on the full voxel list (same bounds), its dense outputs bit
for bit against inference_labels, the voxel-list feed bit for bit against the dense feed, on both plans.
Driver: ANA_CSV rows against the numpy loop of the reference's example_scripts/ana_csv.py on the returned softmax / label."""
import ctypes

import numpy as np
import pytest

from _abi import _Guarded, same_bits
from test_ana_stats_host import reference_rows
from uresnet_amd import _lib, uresnet
from uresnet_amd import synthetic_io as sio
from uresnet_amd.ssnet import VoxelBatch, class_stats_from_counts

pytestmark = pytest.mark.gpu

GUARD = 4096
SPAN = 4096          # CSTATS_SPAN: voxels of one event a cstats workgroup owns (256 threads x 16 steps)
N = 3
# 1, 5, one less / one more than a span, three spans per event with a voxel count that is no multiple of 4
VOXELS = (1, 5, SPAN - 1, SPAN + 1, 2 * SPAN + 1001)
# (name, dtype, channel stride (0: compact = ncls), byte offset of z): the 16-byte path, fp32 stride 8, compact fp32 from a base
# that is only 4-byte aligned, bf16 pieces of 8
LAYOUTS = [("fp32_cs4", 0, 4, 0), ("fp32_cs8", 0, 8, 0), ("fp32_compact_off4", 0, 0, 4), ("bf16_cs8", 1, 8, 0)]
CASES = [(l, c) for l in LAYOUTS for c in (1, 2, 3, 4, 5, 8) if not (l[0] == "fp32_cs4" and c > 4)]


def _bf16_round(a):
    u = np.ascontiguousarray(a, np.float32).view(np.uint32).astype(np.uint64)
    r = ((u + 0x7FFF + ((u >> 16) & 1)) >> 16).astype(np.uint16)
    return r


def _labels(rng, ncls, V):
    """Event 0: random classes plus labels ncls, -1 and 2.7 (class 2 after the cast, or outside with fewer than 3 classes);
    event 1: one class only (every other class is one no voxel carries); event 2: all 0."""
    lab = np.zeros((N, V), np.float32)
    lab[0] = rng.integers(0, max(ncls - 1, 1), V)
    for j, v in enumerate((float(ncls), -1.0, 2.7)):
        lab[0, (3 * j + 1) % V::13] = v           # V = 1: only 2.7 survives; V = 5: one of each
    lab[1] = float(min(1, ncls - 1))
    return lab


def _dev(a):
    import torch
    a = np.ascontiguousarray(a)
    if a.dtype == np.uint16:
        return torch.from_numpy(a.view(np.int16)).cuda()
    return torch.from_numpy(a).cuda()


class _Op(object):
    """The device inputs of one shape, shared by the oracle call and the calls under test."""

    def __init__(self, layout, ncls, V, seed):
        import torch
        _, dtype, cs, zoff = layout
        cs = cs or ncls
        rng = np.random.default_rng(seed)
        z = (2.0 * rng.standard_normal((N * V, cs))).astype(np.float32)
        self.dtype, self.cs, self.ncls, self.V = dtype, cs, ncls, V
        esz = 2 if dtype == 1 else 4
        self.zbuf = torch.zeros(N * V * cs * esz + 16, dtype=torch.uint8, device="cuda")      # torch allocations are 256-byte aligned
        src = _dev(_bf16_round(z) if dtype == 1 else z).reshape(-1).view(torch.uint8)
        self.zbuf[zoff:zoff + src.numel()].copy_(src)
        self.zptr = self.zbuf.data_ptr() + zoff
        self.bn = [_dev(rng.uniform(-0.5, 0.5, ncls).astype(np.float32)), _dev(rng.uniform(0.5, 1.5, ncls).astype(np.float32)),
                   _dev(rng.uniform(-0.5, 0.5, ncls).astype(np.float32))]
        self.data_h = rng.uniform(-1.0, 3.0, (N, V)).astype(np.float32)
        self.label_h = _labels(rng, ncls, V)
        self.data, self.label = _dev(self.data_h), _dev(self.label_h)
        self.offsets = _dev(np.arange(N + 1, dtype=np.int64) * V)
        self.index = _dev(np.tile(np.arange(V, dtype=np.int32), N))
        torch.cuda.synchronize()

    def desc(self, with_bn, with_data, listed):
        d = _lib.ursn_vscores_desc()
        d.n, d.voxels, d.ncls = N, self.V, self.ncls
        d.z, d.z_cstride, d.dtype = self.zptr, self.cs, self.dtype
        if with_bn:
            d.mean, d.rstd, d.beta = (t.data_ptr() for t in self.bn)
        if with_data:
            d.data = self.data.data_ptr()
        if listed:
            d.offsets, d.index = self.offsets.data_ptr(), self.index.data_ptr()
        return d

    def oracle(self, lib, with_bn):
        """ursn_scores_at_voxels over every voxel, then numpy."""
        import torch
        C, V = self.ncls, self.V
        scores = torch.empty((N * V, C), dtype=torch.float32, device="cuda")
        pred = torch.empty(N * V, dtype=torch.uint8, device="cuda")
        d = self.desc(with_bn, False, True)
        _lib.check(lib.ursn_scores_at_voxels(ctypes.byref(d), ctypes.c_void_p(scores.data_ptr()), ctypes.c_void_p(pred.data_ptr()),
                                             None, None))
        torch.cuda.synchronize()
        return _counts(scores.cpu().numpy().reshape(N, V, C), pred.cpu().numpy().reshape(N, V).astype(np.int64),
                       self.label_h, self.data_h)


def _counts(scores, pred, label, data):
    """conf / other / nonzero / fp64 sums of [n, V, C] scores, [n, V] pred, label and (optional) data, as the header defines them."""
    n, V, C = scores.shape
    conf, other, nonzero = np.zeros((n, C, C), np.int64), np.zeros((n, 2), np.int64), np.zeros((n, 2), np.int64)
    ssum, ssq = np.zeros((n, C)), np.zeros((n, C))
    for e in range(n):
        lab = label[e].reshape(-1)
        t = np.trunc(lab).astype(np.int64)
        ok = (t >= 0) & (t < C)
        np.add.at(conf[e], (t[ok], pred[e][ok]), 1)
        other[e] = [np.count_nonzero(~ok & (lab > 0)), np.count_nonzero(~ok & ~(lab > 0))]
        if data is not None:
            nz = data[e].reshape(-1) > 0
            nonzero[e] = [np.count_nonzero(nz), np.count_nonzero(nz & ok & (pred[e] == t))]
        for k in range(C):
            s = scores[e][ok & (t == k), k].astype(np.float64)
            ssum[e, k], ssq[e, k] = s.sum(), (s * s).sum()
    return dict(conf=conf, other=other, nonzero=nonzero if data is not None else None, score_sum=ssum, score_sq=ssq)


_SHAPES = {"conf": lambda C: (N, C, C), "other": lambda C: (N, 2), "nonzero": lambda C: (N, 2), "score_sum": lambda C: (N, C),
           "score_sq": lambda C: (N, C)}


def _run(lib, op, with_bn, with_data, fill=0xFF, expect_rc0=True, tweak=None):
    """One ursn_class_stats call into 0xFF-filled outputs and a `fill`-filled scratch between canary guards; returns the raw
    bytes of every output (rc, message and bytes when a refusal is expected)."""
    import torch
    C = op.ncls
    names = ["conf", "other", "score_sum", "score_sq"] + (["nonzero"] if with_data else [])
    out = {k: _Guarded(int(np.prod(_SHAPES[k](C))) * 8, GUARD, 0xFF) for k in names}
    sbytes = int(lib.ursn_class_stats_scratch_bytes(N, op.V, C))
    assert sbytes > 0
    scratch = _Guarded(sbytes, GUARD, fill)
    o = _lib.ursn_class_stats_out()
    for k in names:
        setattr(o, k, out[k].ptr)
    d = op.desc(with_bn, with_data, False)
    args = dict(d=d, label=op.label.data_ptr(), out=o, scratch=scratch.ptr, sbytes=sbytes)
    if tweak:
        tweak(args)
    torch.cuda.synchronize()
    P = lambda v: None if v is None else ctypes.c_void_p(v)
    rc = lib.ursn_class_stats(ctypes.byref(args["d"]) if args["d"] is not None else None, P(args["label"]),
                              ctypes.byref(args["out"]) if args["out"] is not None else None, P(args["scratch"]), args["sbytes"], None)
    msg = lib.ursn_last_error()
    torch.cuda.synchronize()
    raw = {}
    for k, g in list(out.items()) + [("scratch", scratch)]:
        assert g.guards_intact() == (True, True), k
        if k != "scratch":
            raw[k] = g.view.cpu().numpy().copy()
    if expect_rc0:
        assert rc == 0, msg
        return raw
    return rc, msg, raw


def _decode(raw, C):
    return {k: v.view(np.float64 if k.startswith("score") else np.int64).reshape(_SHAPES[k](C)) for k, v in raw.items()}


def _check(got, want, what):
    for k in ("conf", "other", "nonzero"):
        if k in got:
            assert np.array_equal(got[k], want[k]), (what, k, got[k], want[k])
    for k in ("score_sum", "score_sq"):
        assert np.all(np.abs(got[k] - want[k]) <= 1e-10 * np.abs(want[k])), (what, k, got[k], want[k])
    a = class_stats_from_counts(got["conf"], got["other"], got["score_sum"], got["score_sq"])
    b = class_stats_from_counts(want["conf"], want["other"], want["score_sum"], want["score_sq"])
    assert np.all(np.abs(a["score_std"] - b["score_std"]) <= 1e-6), (what, a["score_std"], b["score_std"])


@pytest.mark.parametrize("layout, ncls", CASES, ids=["%s_%dcls" % (l[0], c) for l, c in CASES])
def test_class_stats_against_scores_at_voxels(lib, layout, ncls):
    seed = 100 * LAYOUTS.index(layout) + ncls
    for V in VOXELS:
        op = _Op(layout, ncls, V, seed + V)
        for with_bn in (True, False):
            want = op.oracle(lib, with_bn)
            for with_data in (True, False):
                got = _decode(_run(lib, op, with_bn, with_data), ncls)
                assert ("nonzero" in got) == with_data
                _check(got, want, (V, with_bn, with_data))
        if V == VOXELS[-1]:
            # the labels really hold what the issue lists
            assert np.count_nonzero(want["conf"][1].sum(axis=1)) == 1 and want["conf"][2].sum() == want["conf"][2][0].sum() == V
            assert want["other"][0, 0] > 0 and want["other"][0, 1] > 0
            # scratch of 0xFF bytes, of zeros, and a second run: the same bits in every output
            a = _run(lib, op, True, True, fill=0xFF)
            b = _run(lib, op, True, True, fill=0x00)
            c = _run(lib, op, True, True, fill=0xFF)
            for k in a:
                assert np.array_equal(a[k], b[k]) and np.array_equal(a[k], c[k]), k
    assert lib.ursn_last_kernel_name() == b"cstats_final"


def test_class_stats_refusals_write_nothing(lib):
    op = _Op(LAYOUTS[0], 3, SPAN + 1, 5)

    def refused(text, with_data=True, **kw):
        def tweak(a):
            for k, v in kw.items():
                if k in ("n", "voxels", "ncls", "z", "z_cstride", "dtype", "rstd", "data"):
                    setattr(a["d"], k, v)
                elif k in ("conf", "nonzero", "score_sum"):
                    setattr(a["out"], k, v)
                else:
                    a[k] = v
        rc, msg, raw = _run(lib, op, True, with_data, expect_rc0=False, tweak=tweak)
        assert rc != 0 and text in msg, (rc, msg, text)
        for k, v in raw.items():
            assert (v == 0xFF).all(), (text, k)

    refused(b"n = 0 outside", n=0)
    refused(b"n = 65536 outside", n=65536)
    refused(b"voxels = 0 < 1", voxels=0)
    refused(b"voxels = 2147483648 >= 2^31", voxels=2 ** 31)
    refused(b"ncls = 0 not in", ncls=0)
    refused(b"ncls = 9 not in", ncls=9)
    refused(b"null desc", d=None)
    refused(b"null label", label=None)
    refused(b"null out", out=None)
    refused(b"null out->conf", conf=None)
    refused(b"null scratch", scratch=None)
    refused(b"null z", z=None)
    refused(b"dtype 2", dtype=2)
    refused(b"z_cstride 2 < ncls 3", z_cstride=2)
    refused(b"bf16 logits need channel stride 8", dtype=1)
    refused(b"z must be 4-byte aligned", z=op.zptr + 2)
    refused(b"mean without rstd / beta", rstd=None)
    refused(b"out->nonzero needs data", data=None)
    refused(b"label / data must be 4-byte aligned", label=op.label.data_ptr() + 1)
    refused(b"must be 8-byte aligned", score_sum=op.data.data_ptr() + 4)
    refused(b"scratch_bytes = 8 is too small", sbytes=8)
    refused(b"scratch must be 8-byte aligned", scratch=op.data.data_ptr() + 4, sbytes=1 << 30)


# ---- net level ------------------------------------------------------------------------------------------------------------
NET_CASES = [
    # dims, F, num_strides, classes, precision, events
    ((32, 32, 1), 8, 3, 3, "fp32", 3),
    ((16, 16, 16, 1), 8, 2, 3, "bf16", 2),
    ((32, 32, 2), 8, 3, 4, "fp32", 2),
]
_NET_IDS = ["%s_%dcls_%s" % ("x".join(str(d) for d in c[0]), c[3], c[4]) for c in NET_CASES]


def _inputs(dims, ncls, n, first=0):
    gen = sio.lartpc_sparse if dims[-1] == 1 else sio.dense_uniform
    ev = [gen(dims, ncls, first + e) for e in range(n)]
    data, label, weight = (np.stack([e[j] for e in ev]) for j in range(3))
    return data, label, weight / weight.sum(axis=1, keepdims=True)


def _net(dims, F, ns, ncls, prec, trainable=False):
    net = uresnet(dims=list(dims), num_class=ncls, base_num_outputs=F, num_strides=ns)
    net.construct(trainable=trainable, use_weight=True, learning_rate=1e-3, seed=7, precision=prec)
    return net


def _same_stats(a, b):
    assert set(a) == set(b)
    for k in a:
        x, y = np.asarray(a[k]), np.asarray(b[k])
        assert x.dtype == y.dtype and x.shape == y.shape and np.array_equal(x.reshape(-1).view(np.uint8), y.reshape(-1).view(np.uint8)), k


def _records(lib, net):
    cnt = ctypes.c_int64(0)
    _lib.check(lib.ursn_profile_read(net._handle, None, 0, ctypes.byref(cnt)))
    recs = (_lib.ursn_prof_rec * max(int(cnt.value), 1))()
    _lib.check(lib.ursn_profile_read(net._handle, recs, int(cnt.value), ctypes.byref(cnt)))
    return [(r.kernel.decode(), int(r.pass_), float(r.ms)) for r in recs[:int(cnt.value)]]


@pytest.mark.parametrize("case", NET_CASES, ids=_NET_IDS)
def test_inference_stats(lib, case):
    dims, F, ns, ncls, prec, n = case
    one = dims[-1] == 1
    data, label, weight = _inputs(dims, ncls, n)
    V = label.shape[1]
    net = _net(dims, F, ns, ncls, prec)
    st = net.inference_stats(None, data, label, with_labels=one, with_softmax=True)

    # the dense outputs are those of inference_labels (inference, where the label rule is refused), bit for bit
    if one:
        lab, acc_all, acc_nz, sm = net.inference_labels(None, data, label, with_softmax=True)
        assert same_bits(st['labels'], lab)
    else:
        sm, acc_all, acc_nz = net.inference(None, data, label)
        assert 'labels' not in st
        with pytest.raises(_lib.UrsnError):
            net.inference_stats(None, data, label, with_labels=True)
    assert same_bits(st['softmax'], sm)
    f32 = lambda x: np.asarray([x], np.float32)
    assert same_bits(f32(st['acc_all_batch']), f32(acc_all))
    assert same_bits(f32(st['acc_nonzero_batch']), f32(acc_nz)) or (not one and np.isnan(acc_nz) and np.isnan(st['acc_nonzero_batch']))

    # scores and pred at every voxel: the gather head on the full list; softmax argmax where a list cannot be fed (no top-2 tie)
    if one:
        full = VoxelBatch(np.arange(n + 1) * V, np.tile(np.arange(V, dtype=np.int32), n), data.reshape(-1), label.reshape(-1),
                          None, None, V)
        r = net.inference_voxel_scores(None, full, want=('scores', 'pred'))
        scores = np.stack(r['scores'])
        pred = np.stack(r['pred']).astype(np.int64)
        assert same_bits(scores, np.ascontiguousarray(sm.reshape(n, V, ncls)))
    else:
        scores = sm.reshape(n, V, ncls)
        srt = np.sort(scores, axis=-1)
        assert not (srt[..., -1] == srt[..., -2]).any(), "a top-2 tie: softmax argmax is not the logit argmax there"
        pred = scores.argmax(axis=-1)
    want = _counts(scores, pred, label, data if one else None)
    for k in ("conf", "other"):
        assert np.array_equal(st[k], want[k]), k
    ref = class_stats_from_counts(want["conf"], want["other"], want["score_sum"], want["score_sq"], want["nonzero"])
    some = ref['npx'] > 0
    assert np.all(np.abs(st['score_mean'] - ref['score_mean'])[some] <= 1e-10 * np.abs(ref['score_mean'])[some])
    assert np.all(np.abs(st['score_std'] - ref['score_std']) <= 1e-6)
    for k in ('npx', 'acc_class', 'acc_all', 'acc_nonzero_label', 'acc_nonzero_data'):
        assert np.array_equal(st[k], ref[k], equal_nan=(st[k].dtype == np.float64)), k
    assert np.isnan(st['acc_nonzero_data']).all() == (not one)
    if one:
        # the mean of the per-event data accuracies' numerators / denominators is the head's batch figure
        nzs = want["nonzero"].sum(axis=0)
        assert abs(nzs[1] / nzs[0] - acc_nz) <= 1e-6
    assert abs(st['acc_all'].mean() - acc_all) <= 1e-6

    # without dense outputs the dense head is not launched: one pass-6 record, "cstats"
    _lib.check(lib.ursn_profile_enable(net._handle, 1))
    bare = net.inference_stats(None, data, label)
    recs = _records(lib, net)
    assert [k for k, p, _ in recs if p == 6] == ["cstats"], [k for k, p, _ in recs if p == 6]
    net.inference_stats(None, data, label, with_softmax=True)
    recs = _records(lib, net)
    assert sorted(k for k, p, _ in recs if p == 6) == sorted(["bhead" if prec == "bf16" else "head", "cstats"])
    _lib.check(lib.ursn_profile_enable(net._handle, 0))
    dense_keys = {'labels', 'softmax', 'acc_all_batch', 'acc_nonzero_batch'}
    assert not (set(bare) & dense_keys)
    _same_stats(bare, {k: v for k, v in st.items() if k not in dense_keys})

    # the voxel-list feed gives the dense feed's bits
    if one:
        vb = VoxelBatch.concat([sio.dense_to_voxels(data[i], label[i]) for i in range(n)])
        h2d = net.feed_stats['h2d_bytes']
        sv = net.inference_stats_voxels(None, vb, with_labels=True, with_softmax=True)
        M, pad = int(vb.offsets[-1]), lambda b: (b + 15) & ~15
        assert net.feed_stats['h2d_bytes'] - h2d == pad(8 * (n + 1)) + 3 * pad(4 * M)      # offsets, index, value, label: nothing dense
        _same_stats(sv, st)

    # a handle that served an accum_gradients at another batch size first gives the same bits
    other = _net(dims, F, ns, ncls, prec, trainable=True)
    d1, l1, w1 = _inputs(dims, ncls, 1, first=5)
    other.zero_gradients(None)
    other.accum_gradients(None, d1, l1, w1)
    _same_stats(other.inference_stats(None, data, label, with_labels=one, with_softmax=True), st)


# ---- driver ---------------------------------------------------------------------------------------------------------------
def _ana_cfg(tmp_path, tag, csv=True, sparse=False, scores=False):
    inp = tmp_path / "input.cfg"
    inp.write_text("Dims [32, 32, 32, 1]\nNumClass 3\nGenerator 'lartpc_sparse'\nNumEntries 64\n"
                   "Keys {'data': 'data', 'label': 'label', 'weight': 'weight'}\n")
    out, csvf = tmp_path / ("ssnet_%s.npy" % tag), tmp_path / ("ana_%s.csv" % tag)
    ana = tmp_path / ("ana_%s.cfg" % tag)
    ana.write_text("NUM_CLASS 3\nBASE_NUM_FILTERS 4\nMAIN_INPUT_CONFIG '%s'\nANA_OUTPUT_CONFIG '%s'\nLOGDIR ''\nSAVE_FILE ''\n"
                   "ITERATIONS 2\nMINIBATCH_SIZE 2\nTRAIN False\nUSE_WEIGHTS False\nSUMMARY_STEPS 0\nCHECKPOINT_STEPS 0\n"
                   "SPARSE_IO %s\nSPARSE_SCORES %s\n%s" % (inp, out, sparse, scores, "ANA_CSV '%s'\n" % csvf if csv else ""))
    return ana, out, csvf


def _drive(cfg, batch=False):
    from uresnet_amd.ssnet_trainval import ssnet_trainval
    a = ssnet_trainval()
    a.override_config(str(cfg))
    a.initialize()
    if batch:
        a.batch_process()
        res = None
    else:
        res = [a.ana_step() for _ in range(2)]
    a.reset()
    return res


def test_driver_appends_the_reference_csv(tmp_path, capsys):
    plain_cfg, plain_out, _ = _ana_cfg(tmp_path, "plain", csv=False)
    plain = _drive(plain_cfg)
    cfg, out, csvf = _ana_cfg(tmp_path, "csv")
    res = _drive(cfg)
    assert out.read_bytes() == plain_out.read_bytes()                 # the ANA_OUTPUT records, byte for byte
    text = csvf.read_text()
    lines = text.splitlines(True)
    from uresnet_amd.ssnet import ana_csv_header
    assert len(lines) == 5 and lines[0] == ana_csv_header(3)

    for it in range(2):
        r = res[it]
        assert set(r) == set(plain[it]) | {'stats'}
        assert same_bits(r['softmax'], plain[it]['softmax']) and r['acc_nonzero'] == plain[it]['acc_nonzero']
        sm, lab = r['softmax'], r['label']
        rows, _ = reference_rows(list(r['entries']), sm, lab, 3)
        srt = np.sort(sm, axis=-1)
        tie = srt[..., -1] == srt[..., -2]            # np.argmax(softmax) may differ from the logit argmax only there
        assert tie.mean() <= 1e-3, tie.mean()
        pred = sm.argmax(axis=-1)
        for i in range(2):
            f = lines[1 + 2 * it + i].rstrip('\n').split(',')
            assert len(f) == 3 + 4 * 3 and int(f[0]) == r['entries'][i] == 2 * it + i
            l, p, t = np.squeeze(lab[i]), pred[i], tie[i]
            ok = p == l
            assert float((ok & ~t).mean()) - 1e-6 <= float(f[1]) <= float((ok | t).mean()) + 1e-6
            nzm = l > 0
            assert float((ok & ~t)[nzm].mean()) - 1e-6 <= float(f[2]) <= float((ok | t)[nzm].mean()) + 1e-6
            for k in range(3):
                npx, acc, mean, std = f[3 + 4 * k:7 + 4 * k]
                assert int(npx) == rows[i]['npx'][k] == r['stats']['npx'][i, k]
                m = l == k
                if not m.any():
                    assert (acc, mean, std) == ('-1', '-1', '-1')
                    continue
                assert float((ok & ~t)[m].mean()) - 1e-6 <= float(acc) <= float((ok | t)[m].mean()) + 1e-6
                assert abs(float(mean) - rows[i]['mean'][k]) <= 1e-5 * abs(rows[i]['mean'][k])
                assert abs(float(std) - rows[i]['std'][k]) <= 1e-5 * abs(rows[i]['std'][k]) + 1e-9
        assert np.isfinite(r['stats']['acc_nonzero_data']).all()

    # SPARSE_IO: the same CSV text; its records are those of SPARSE_IO without ANA_CSV, interactive and batch mode alike
    sp_plain_cfg, sp_plain_out, _ = _ana_cfg(tmp_path, "sp_plain", csv=False, sparse=True)
    _drive(sp_plain_cfg)
    sp_cfg, sp_out, sp_csv = _ana_cfg(tmp_path, "sp_csv", sparse=True)
    sp = _drive(sp_cfg)
    assert sp_csv.read_text() == text and sp_out.read_bytes() == sp_plain_out.read_bytes()
    assert same_bits(sp[1]['softmax'], res[1]['softmax'])
    b_cfg, b_out, b_csv = _ana_cfg(tmp_path, "sp_batch", sparse=True)
    _drive(b_cfg, batch=True)
    assert b_csv.read_text() == text and b_out.read_bytes() == sp_plain_out.read_bytes()
    # a second run appends rows, not a second header
    _drive(b_cfg, batch=True)
    assert b_csv.read_text() == text + "".join(lines[1:])

    bad, _, _ = _ana_cfg(tmp_path, "bad", sparse=True, scores=True)
    from uresnet_amd.ssnet_trainval import ssnet_trainval
    a = ssnet_trainval()
    a.override_config(str(bad))
    with pytest.raises(ValueError) as e:
        a.initialize()
    assert "ANA_CSV" in str(e.value) and "SPARSE_SCORES" in str(e.value)
    capsys.readouterr()
