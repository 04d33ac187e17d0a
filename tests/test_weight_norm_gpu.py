"""Per-event weight normalisation on the device (include/uresnet_hip.h: ursn_normalize_weights; weight_norm.hip), from the
kernel pair up to the DEVICE_WEIGHT_NORM driver switch.

Oracle everywhere: S = np.sum(w, axis=1, dtype=np.float64), expected w / np.float32(S)[:, None] in float32.  Weights of the
exact cases are k / 1024 with integer k in [0, 4096]: every partial sum, in any order, is an integer multiple of 2^-10 below
2^27 and therefore exact in fp64, so the expected bits do not depend on the device's summation order and the comparison is
bit for bit (tests/_abi.py::same_bits).  Outputs sit between 0xFF-filled margins and canary guards.

Shapes (n, voxels) are the smallest that reach every path of the kernels: an event shorter than one 16-byte vector, event
starts off a 16-byte boundary (voxels % 4 != 0), a scalar tail, exactly one span, several spans with a ragged last one."""
import ctypes
import re

import numpy as np
import pytest

from _abi import _Guarded, same_bits
from uresnet_amd import _lib, uresnet
from uresnet_amd import synthetic_io as sio
from uresnet_amd.ssnet import VoxelBatch

pytestmark = pytest.mark.gpu

SPAN = 16384          # voxels per workgroup (WNORM_SPAN); test_span_constant pins it
GUARD = 4096
SHAPES = [(1, 1), (1, 3), (3, 5), (2, 1023), (3, 4099), (2, 4096), (4, 32768), (2, 2 * SPAN + 7), (2, SPAN)]
NAN64 = 0x7FF8000000000000


def _ids(s):
    return "%dx%d" % s


def _dyadic(n, V, seed, lo=0):
    return (np.random.default_rng(seed).integers(lo, 4097, (n, V)).astype(np.float64) / 1024.0).astype(np.float32)


def _oracle(w):
    S = np.sum(w, axis=1, dtype=np.float64)
    with np.errstate(divide="ignore", invalid="ignore"):
        return w / np.float32(S)[:, None], np.float32(S)


def _scratch(lib, n, V, fill, at_least=0):
    """Guarded scratch of the size the query asks for (or `at_least`), pre-filled: a byte value, or 'nan64' for quiet fp64 NaNs."""
    import torch
    need = max(int(lib.ursn_normalize_weights_scratch_bytes(n, V)), at_least)
    g = _Guarded(need, GUARD, 0 if fill == "nan64" else fill)
    if fill == "nan64":
        g.view.view(torch.int64).fill_(NAN64)
    return g, need


def _normalize(lib, w, w_shift=0, out_shift=None, fill=0xFF, scratch=None, sums=True):
    """One ursn_normalize_weights call on host weights [n, V].  The weight tensor starts `w_shift` floats past a 256-byte
    boundary; out_shift None = in place, else a second buffer that far past one.  Returns (out, sums, weight afterwards)."""
    import torch
    n, V = w.shape
    nb = n * V * 4

    def place(shift):
        g = _Guarded(nb + 32, GUARD, 0xFF)
        return g, g.ptr + 4 * shift, g.view[4 * shift:4 * shift + nb]

    gw, wptr, wview = place(w_shift)
    wview.copy_(torch.from_numpy(w.reshape(-1).view(np.uint8)))
    go, optr, oview = (gw, wptr, wview) if out_shift is None else place(out_shift)
    gs = _Guarded(n * 4, GUARD, 0xFF)
    sc, need = scratch if scratch is not None else _scratch(lib, n, V, fill)
    torch.cuda.synchronize()
    _lib.check(lib.ursn_normalize_weights(ctypes.c_void_p(wptr), ctypes.c_void_p(optr), n, V,
                                          ctypes.c_void_p(gs.ptr) if sums else None, ctypes.c_void_p(sc.ptr), need, None))
    torch.cuda.synchronize()
    for g, shift in ((gw, w_shift), (go, out_shift if out_shift is not None else w_shift)):
        assert g.guards_intact() == (True, True)
        raw = g.view.cpu().numpy()
        assert (raw[:4 * shift] == 0xFF).all() and (raw[4 * shift + nb:] == 0xFF).all(), "bytes next to the tensor were written"
    assert sc.guards_intact() == (True, True) and gs.guards_intact() == (True, True)
    f32 = lambda v: v.cpu().numpy().view(np.float32).reshape(n, V).copy()
    s = gs.view.cpu().numpy().view(np.float32).copy()
    if not sums:
        assert (gs.view.cpu().numpy() == 0xFF).all()
    return f32(oview), s, f32(wview)


def test_span_constant(lib):
    q = lib.ursn_normalize_weights_scratch_bytes
    assert q(1, SPAN) == 8 and q(1, SPAN + 1) == 16 and q(3, 2 * SPAN + 7) == 72


# ---- 1. exact cases --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", SHAPES, ids=_ids)
def test_dyadic_weights_match_the_oracle_bit_for_bit(lib, shape):
    n, V = shape
    w = _dyadic(n, V, 1000 + V)
    want, want_s = _oracle(w)
    assert np.isfinite(want).all()
    for w_shift in (0, 1):                                # 16-byte aligned, and one float past it
        out, s, _ = _normalize(lib, w, w_shift)           # in place
        assert same_bits(out, want) and same_bits(s, want_s), ("in place", w_shift)
    # out of place: equally placed pairs take the 16-byte path, the unequal pairs go element by element
    for w_shift, out_shift in ((0, 0), (1, 1), (1, 0), (0, 3)):
        out, s, after = _normalize(lib, w, w_shift, out_shift)
        assert same_bits(out, want) and same_bits(s, want_s), ("out of place", w_shift, out_shift)
        assert same_bits(after, w), "out of place wrote the weight tensor"
    out, _, _ = _normalize(lib, w, 0, 0, sums=False)      # sums_out is optional
    assert same_bits(out, want)


# ---- 2. general inputs -----------------------------------------------------------------------------------------------------
def _ulps(a, b):
    """Distance in units of the last place between positive finite fp32 arrays."""
    return np.abs(a.view(np.int32).astype(np.int64) - b.view(np.int32).astype(np.int64))


@pytest.mark.parametrize("shape", [(3, 4099), (4, 32768)], ids=_ids)
def test_inverse_frequency_like_weights_within_one_ulp(lib, shape):
    """Background 1.0, half a percent of the voxels log-normal up to 1e3.  The device's fp64 sum takes another order than
    numpy's, so it may differ in its last bits and, rarely, round to the neighbouring float: 1 ulp on sums_out, and 1 ulp on
    every element (the issue's bound)."""
    n, V = shape
    rng = np.random.default_rng(77 + V)
    w = np.ones((n, V), np.float32)
    hot = rng.uniform(0, 1, (n, V)) < 0.005
    w[hot] = np.minimum(rng.lognormal(3.0, 1.5, int(hot.sum())), 1e3).astype(np.float32)
    assert w.max() > 100 and hot.sum() > 10
    want, want_s = _oracle(w)
    for w_shift, out_shift in ((0, None), (1, None), (0, 0), (1, 0)):
        out, s, _ = _normalize(lib, w, w_shift, out_shift)
        du, ds = int(_ulps(out, want).max()), int(_ulps(s, want_s).max())
        print("%s shift %s/%s: max element distance %d ulp, max sum distance %d ulp" % (_ids(shape), w_shift, out_shift, du, ds))
        assert du <= 1 and ds <= 1


# ---- 3. state --------------------------------------------------------------------------------------------------------------
def test_result_depends_only_on_the_arguments(lib):
    n, V = 3, 2 * SPAN + 7
    w = _dyadic(n, V, 5) * np.float32(1.0 / 3.0)          # not dyadic any more: the bits now depend on the summation order
    runs = [_normalize(lib, w, 1, fill=f) for f in (0x00, 0xFF, "nan64", 0x7F)]
    for out, s, _ in runs[1:]:
        assert same_bits(out, runs[0][0]) and same_bits(s, runs[0][1])
    # one scratch buffer, sized for the larger shape: twice in a row, then a larger call in between
    big = _dyadic(4, 3 * SPAN + 1, 6)
    shared = _scratch(lib, 4, 3 * SPAN + 1, 0xFF)
    a = _normalize(lib, w, 1, scratch=shared)
    b = _normalize(lib, w, 1, scratch=shared)
    c = _normalize(lib, big, 0, scratch=shared)
    d = _normalize(lib, w, 1, scratch=shared)
    assert same_bits(c[0], _oracle(big)[0])
    for out, s, _ in (a, b, d):
        assert same_bits(out, runs[0][0]) and same_bits(s, runs[0][1])


def test_call_enqueues_and_does_not_synchronise(lib):
    import torch
    n, V = 4, 32768
    w = _dyadic(n, V, 8)
    dev = torch.from_numpy(w).cuda()
    need = int(lib.ursn_normalize_weights_scratch_bytes(n, V))
    scratch = torch.empty(need // 8, dtype=torch.float64, device="cuda")
    ballast = torch.ones(1 << 27, dtype=torch.float32, device="cuda")      # 512 MB: each pass moves 1 GB
    torch.cuda.synchronize()
    for _ in range(60):
        ballast.mul_(1.0001)
    _lib.check(lib.ursn_normalize_weights(ctypes.c_void_p(dev.data_ptr()), ctypes.c_void_p(dev.data_ptr()), n, V, None,
                                          ctypes.c_void_p(scratch.data_ptr()), need,
                                          ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)))
    done = torch.cuda.Event()
    done.record()
    busy = not done.query()
    torch.cuda.synchronize()
    assert busy, "the call returned only after the stream had drained"
    assert same_bits(dev.cpu().numpy(), _oracle(w)[0])


# ---- 4. zero-sum event -----------------------------------------------------------------------------------------------------
def test_zero_sum_event_gets_numpys_nan_and_leaves_the_others_alone(lib):
    w = _dyadic(3, 4099, 9)
    w[1] = 0.0
    want, want_s = _oracle(w)
    assert np.isnan(want[1]).all() and want_s[1] == 0.0
    for out_shift in (None, 0):
        out, s, _ = _normalize(lib, w, 0, out_shift)
        assert np.isnan(out[1]).all()
        assert same_bits(out[0], want[0]) and same_bits(out[2], want[2]) and same_bits(s, want_s)


# ---- 5. net level ----------------------------------------------------------------------------------------------------------
NET_CASES = [((32, 32, 1), "fp32", 4, 3), ((16, 16, 16, 1), "fp32", 4, 2), ((32, 32, 1), "bf16", 8, 3), ((16, 16, 16, 1), "bf16", 8, 2)]
NET_IDS = ["%s_%s" % ("x".join(str(d) for d in c[0][:-1]), c[1]) for c in NET_CASES]
_inputs = {}


def _net_inputs(dims):
    """Two lartpc_sparse events with their weights replaced by dyadic ones (>= 1/1024, so no event sums to zero): dense arrays,
    the oracle's normalised weights, and the same batch as a VoxelBatch (listed weights and bg_weight dyadic too)."""
    if dims not in _inputs:
        ev = [sio.lartpc_sparse(dims, 3, e) for e in range(2)]
        data, label = (np.stack([e[j] for e in ev]) for j in range(2))
        V = data.shape[1]
        w_raw = _dyadic(2, V, 21, lo=1)
        bg = np.array([5.0 / 1024.0, 0.75], np.float32)
        w_raw[(data == 0) & (label == 0)] = 0.0
        w_raw += ((data == 0) & (label == 0)) * bg[:, None]
        vb = VoxelBatch.concat([sio.dense_to_voxels(data[i], label[i], w_raw[i]) for i in range(2)]).validate()
        assert all(same_bits(a, b) for a, b in zip(sio.voxels_to_dense(vb), (data, label, w_raw)))
        _inputs[dims] = (data, label, w_raw, _oracle(w_raw)[0], vb)
    return _inputs[dims]


def _build(dims, prec, base, ns, trainable=True):
    net = uresnet(dims=list(dims), num_class=3, base_num_outputs=base, num_strides=ns)
    net.construct(trainable=trainable, use_weight=True, learning_rate=1e-3, seed=7, precision=prec)
    return net


def _step(net, *args, **kw):
    net.zero_gradients(None)
    res, _ = net.accum_gradients(None, *args, **kw)
    return res, net.get_gradients()


def _same_step(a, b):
    return a[0] == b[0] and all(same_bits(a[1][k], b[1][k]) for k in b[1])


@pytest.mark.parametrize("dims, prec, base, ns", NET_CASES, ids=NET_IDS)
def test_step_with_device_normalisation_equals_step_on_normalised_weights(dims, prec, base, ns):
    import torch
    data, label, w_raw, w_want, vb = _net_inputs(dims)
    ref_net, net = _build(dims, prec, base, ns), _build(dims, prec, base, ns)
    ref = _step(ref_net, data, label, w_want)
    assert np.isfinite(ref[0][1:]).all() and ref[0][1] > 0
    keep = w_raw.copy()
    got = _step(net, data, label, w_raw, normalize_weight=True)
    assert _same_step(got, ref), (got[0], ref[0])
    assert same_bits(w_raw, keep), "the caller's host array was written"
    assert same_bits(net.last_feed()['input_weight'].cpu().numpy(), w_want)          # last_feed holds normalised weights
    # a caller-owned device tensor goes through _feed unchanged: normalised out of place, never written
    w_dev = torch.from_numpy(w_raw).cuda()
    got = _step(net, data, label, w_dev, normalize_weight=True)
    assert _same_step(got, ref)
    assert same_bits(w_dev.cpu().numpy(), w_raw), "the caller's device tensor was written"
    assert net.last_feed()['input_weight'].data_ptr() != w_dev.data_ptr()
    # without the keyword nothing is normalised: raw weights give another loss
    assert _step(net, data, label, w_raw)[0][1] != ref[0][1]
    want_test = ref_net.run_test(None, data, label, w_want)
    assert net.run_test(None, data, label, w_raw, normalize_weight=True) == want_test
    assert net.run_test(None, data, label, w_dev, normalize_weight=True) == want_test
    assert same_bits(w_dev.cpu().numpy(), w_raw) and same_bits(w_raw, keep)
    summ = net.make_summary(None, data, label, w_raw, normalize_weight=True)
    assert [summ['loss'], summ['accuracy_all'], summ['accuracy_nonzero']] == want_test[0]
    # re-running last_feed() (what the driver's summary step does) must not normalise again
    _step(net, data, label, w_raw, normalize_weight=True)
    last = net.last_feed()
    assert net.run_test(None, last['input_data'], last['input_label'], last['input_weight']) == want_test


# ---- 6. voxel feed ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("prec, base", [("fp32", 4), ("bf16", 8)])
def test_voxel_fed_step_normalises_the_expanded_tensor(prec, base):
    dims, ns = (16, 16, 16, 1), 2
    data, label, w_raw, w_want, vb = _net_inputs(dims)
    ref_net, net = _build(dims, prec, base, ns), _build(dims, prec, base, ns)
    ref = _step(ref_net, data, label, w_want)
    keep_w, keep_bg = vb.weight.copy(), vb.bg_weight.copy()
    net.zero_gradients(None)
    res, _ = net.accum_gradients_voxels(None, vb, normalize_weight=True)
    assert _same_step((res, net.get_gradients()), ref)
    assert same_bits(net.last_feed()['input_weight'].cpu().numpy(), w_want)
    assert net.run_test_voxels(None, vb, normalize_weight=True) == ref_net.run_test(None, data, label, w_want)
    assert same_bits(vb.weight, keep_w) and same_bits(vb.bg_weight, keep_bg)


# ---- 7. driver -------------------------------------------------------------------------------------------------------------
DRIVER_DIMS = (64, 64)


def _driver_run(tmp_path, on, capsys):
    from uresnet_amd.ssnet_trainval import ssnet_trainval
    tag = "on" if on else "off"
    inp = tmp_path / "input.cfg"
    inp.write_text("Dims [%d, %d, 1]\nNumClass 3\nGenerator 'lartpc_sparse'\nNumEntries 64\n"
                   "Keys {'data': 'main_data', 'label': 'main_label', 'weight': 'main_weight'}\n" % DRIVER_DIMS)
    cfg = tmp_path / ("train_%s.cfg" % tag)
    cfg.write_text("NUM_CLASS 3\nBASE_NUM_FILTERS 4\nMAIN_INPUT_CONFIG '%s'\nTEST_INPUT_CONFIG '%s'\nLOGDIR '%s'\nSAVE_FILE ''\n"
                   "ITERATIONS 3\nMINIBATCH_SIZE 2\nNUM_MINIBATCHES 1\nTEST_BATCH_SIZE 2\nLEARNING_RATE 0.001\nTRAIN True\n"
                   "USE_WEIGHTS True\nREPORT_STEPS 1\nSUMMARY_STEPS 2\nCHECKPOINT_STEPS 0\nKEYWORD_DATA 'main_data'\n"
                   "KEYWORD_LABEL 'main_label'\nKEYWORD_WEIGHT 'main_weight'\nKEYWORD_TEST_DATA 'main_data'\n"
                   "KEYWORD_TEST_LABEL 'main_label'\nKEYWORD_TEST_WEIGHT 'main_weight'\nDEVICE_WEIGHT_NORM %s\n"
                   % (inp, inp, tmp_path / ("log_" + tag), on))
    t = ssnet_trainval()
    t.override_config(str(cfg))
    t.initialize()
    assert t._cfg.DEVICE_WEIGHT_NORM is on and t._norm_kw() == ({'normalize_weight': True} if on else {})
    capsys.readouterr()
    rows, run = [], t._run_minibatches       # the per-minibatch metrics as the driver reads them, before '%6.6f' rounds them
    t._run_minibatches = lambda want_metrics: rows.append(run(want_metrics)) or rows[-1]
    for _ in range(3):
        t.train_step()
    first = [float(x) for x in rows[0][0]]   # NUM_MINIBATCHES 1: iteration 0 is one row
    printed = capsys.readouterr().out
    fed = t._net.last_feed()['input_weight'].cpu().numpy()      # normalised exactly once, wherever it was done
    assert np.abs(fed.sum(axis=1, dtype=np.float64) - 1.0).max() < 1e-5
    log = (tmp_path / ("log_" + tag) / "train" / "scalars.jsonl").read_text()
    t.reset()
    return first, printed, log


def test_driver_with_device_weight_norm(tmp_path, capsys):
    """Three iterations of a 2-D synthetic training config (64 x 64 lartpc_sparse events, whose inverse-frequency weights have
    non-trivial sums; USE_WEIGHTS True) with DEVICE_WEIGHT_NORM True against False, same seed.  The two differ only through the
    host's float32 pairwise np.sum against the device's fp64 sum: relative error of the host sum <= ceil(log2(voxels)) * 2^-24,
    the loss is linear in 1 / S_e, so the losses of iteration 0 agree within twice that bound plus 2^-22 for the head's own
    rounding; the accuracies do not depend on the weights' scale at all.  Later iterations: finite only (Adam amplifies last-bit
    differences)."""
    import json
    off, printed_off, log_off = _driver_run(tmp_path, False, capsys)
    on, printed_on, log_on = _driver_run(tmp_path, True, capsys)
    voxels = DRIVER_DIMS[0] * DRIVER_DIMS[1]
    bound = 2 * int(np.ceil(np.log2(voxels))) * 2.0 ** -24 + 2.0 ** -22
    print("iteration 0: loss %.9g (host normalisation) / %.9g (device), relative difference %.3g, bound %.3g"
          % (off[0], on[0], abs(on[0] - off[0]) / abs(off[0]), bound))
    assert np.isfinite(off).all() and off[0] > 0
    assert abs(on[0] - off[0]) <= bound * max(abs(on[0]), abs(off[0]))
    assert on[1:] == off[1:]
    line = re.compile(r"^Train set: loss=(\S+)   acc\. all=(\S+)   acc\. nonzero=(\S+)   $", re.M)
    test_line = re.compile(r"^Test set: loss=(\S+)   acc\. all=(\S+)   acc\. nonzero=(\S+)   $", re.M)
    head = re.compile(r"^@ iteration \d+ LR 0\.001 Mem \S+ @ \d{4}-\d\d-\d\d \d\d:\d\d:\d\d$", re.M)
    for printed in (printed_off, printed_on):
        assert len(head.findall(printed)) == 3
        rows, tests = line.findall(printed), test_line.findall(printed)
        assert len(rows) == 3 and len(tests) == 3
        assert np.isfinite(np.array(rows + tests, np.float64)).all()
    # the printed form is the same line for line once the numbers are masked
    mask = lambda s: re.sub(r"[-+]?\d[\d.e+:-]*", "#", s)
    assert mask(printed_on) == mask(printed_off)
    for log in (log_off, log_on):             # summary steps 0 and 2 re-feed last_feed()
        recs = [json.loads(x) for x in log.strip().split("\n")]
        assert [r['iteration'] for r in recs] == [0, 2]
        assert all(np.isfinite(r['loss']) and r['loss'] > 0 for r in recs)
