"""Voxel-list I/O on the device (include/uresnet_hip.h, ABI 8; voxel_io.hip): ursn_voxels_to_dense against the numpy
expansion, ursn_labels_to_voxels against np.flatnonzero, the *_voxels methods of ssnet_base against their dense namesakes and
the SPARSE_IO driver against the dense driver.  Every comparison is exact: bit patterns (tests/_abi.py::same_bits) or
np.array_equal; outputs are pre-filled with NaN bytes between canary guards.

Op-level shapes are the smallest at which tails and seams occur: 6x10x14 (840 voxels: no multiple of 4, 16 or 64), 32x32,
16^3 (exactly two compaction spans) and 33x16x16 = 8448 = four spans of 2048 + 256.  The issue's 32x16x16 = 8192 is an exact
multiple of the span (any power-of-two span divides it), so the last shape is one step off it."""
import ctypes

import numpy as np
import pytest

from _abi import FILLS, _Guarded, same_bits
from uresnet_amd import _lib, uresnet
from uresnet_amd import synthetic_io as sio
from uresnet_amd.ssnet import VoxelBatch

pytestmark = pytest.mark.gpu

SHAPES = [(6, 10, 14), (32, 32), (16, 16, 16), (33, 16, 16)]
SPAN = 2048          # voxels per compaction workgroup (VOX_SPAN), four waves of 512
GUARD = 4096


def _ids(s):
    return "x".join(str(d) for d in s)


# ---- inputs, built once ---------------------------------------------------------------------------------------------------
def _event(kind, shape, seed):
    """One event as a one-event VoxelBatch with label and weight."""
    V = int(np.prod(shape))
    rng = np.random.default_rng(100 + seed)
    if kind == "lartpc":
        return sio.dense_to_voxels(*sio.lartpc_sparse(tuple(shape) + (1,), 3, seed))
    if kind == "empty":
        return VoxelBatch([0, 0], [], [], [], [], [0.25 + seed], V)
    idx = np.arange(V) if kind == "full" else np.array([0, V - 1])
    m = idx.size
    return VoxelBatch([0, m], idx, rng.uniform(1, 50, m), rng.integers(1, 3, m), rng.uniform(0.5, 1.5, m), [0.125 * (1 + seed)], V)


_BATCHES = {1: [("lartpc",), ("full",), ("ends",), ("empty",)],
            3: [("lartpc", "empty", "lartpc"), ("full", "ends", "lartpc"), ("ends", "full", "empty")]}
_vb_cache = {}


def _batches(shape, n):
    key = (tuple(shape), n)
    if key not in _vb_cache:
        _vb_cache[key] = [VoxelBatch.concat([_event(k, shape, 3 * j + i) for i, k in enumerate(kinds)]).validate()
                          for j, kinds in enumerate(_BATCHES[n])]
    return _vb_cache[key]


def _dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).cuda() if a.size else torch.empty(4, dtype=torch.uint8, device="cuda")


def _expand(lib, vb, with_extra, shift=0):
    """ursn_voxels_to_dense into NaN-filled guarded buffers; `shift` floats of offset make the flat outputs start off a
    16-byte boundary.  Returns the outputs as [n, V] arrays (None for roles not asked for)."""
    import torch
    n, V = vb.n, vb.voxels
    keep = [_dev(a) for a in (vb.offsets, vb.index, vb.value, vb.label, vb.weight, vb.bg_weight)]
    b = _lib.ursn_voxel_batch()
    b.n, b.voxels = n, V
    b.offsets, b.index, b.value = (t.data_ptr() for t in keep[:3])
    if with_extra:
        b.label, b.weight, b.bg_weight = (t.data_ptr() for t in keep[3:])
    bufs = [_Guarded((n * V + 4) * 4, GUARD, 0xFF) for _ in range(3 if with_extra else 1)]
    torch.cuda.synchronize()
    ptrs = [ctypes.c_void_p(g.ptr + 4 * shift) for g in bufs] + [None] * (3 - len(bufs))
    _lib.check(lib.ursn_voxels_to_dense(ctypes.byref(b), ptrs[0], ptrs[1], ptrs[2], None))
    torch.cuda.synchronize()
    out = []
    for g in bufs:
        assert g.guards_intact() == (True, True)
        raw = g.view.cpu().numpy()
        lo, hi = 4 * shift, 4 * shift + 4 * n * V
        assert (raw[:lo] == 0xFF).all() and (raw[hi:] == 0xFF).all(), "bytes next to the output were written"
        out.append(raw[lo:hi].copy().view(np.float32).reshape(n, V))
    return out + [None] * (3 - len(out))


@pytest.mark.parametrize("n", [1, 3])
@pytest.mark.parametrize("shape", SHAPES, ids=_ids)
def test_voxels_to_dense_equals_the_numpy_expansion(lib, shape, n):
    for vb in _batches(shape, n):
        want = sio.voxels_to_dense(vb)
        for with_extra in (True, False):
            for shift in (0, 1, 3):
                got = _expand(lib, vb, with_extra, shift)
                assert same_bits(got[0], want[0])
                if with_extra:
                    assert same_bits(got[1], want[1]) and same_bits(got[2], want[2])


# ---- ursn_labels_to_voxels ------------------------------------------------------------------------------------------------
def _volume(kind, V, seed):
    v = np.zeros(V, np.float32)
    rng = np.random.default_rng(seed)
    if kind == "ones":
        v[:] = 1.0
    elif kind == "first":
        v[0] = 2.0
    elif kind == "last":
        v[-1] = 1.0
    elif kind == "seams":       # a run of non-zeros across every wave and workgroup seam
        for s in range(SPAN // 4, V, SPAN // 4):
            v[s - 3:s + 3] = 1.0 + (s // 512) % 2
        v[max(V - 2, 0):] = 2.0
    elif kind == "mixed":
        v[:] = rng.integers(0, 3, V)
    return v


_VOLUMES = {1: [("zero",), ("ones",), ("first",), ("last",), ("seams",), ("mixed",)],
            3: [("mixed", "zero", "seams"), ("ones", "first", "last"), ("zero", "zero", "mixed"), ("last", "ones", "first")]}


def _compact(lib, labels, cap, fill):
    import torch
    n, V = labels.shape
    dev = torch.from_numpy(labels).cuda()
    need = int(lib.ursn_labels_to_voxels_scratch_bytes(n, V))
    scratch = _Guarded(need, GUARD, FILLS[fill])
    index, cls, off = _Guarded(cap * 4, GUARD, 0xFF), _Guarded(cap, GUARD, 0xFF), _Guarded((n + 1) * 8, GUARD, 0xFF)
    torch.cuda.synchronize()
    _lib.check(lib.ursn_labels_to_voxels(ctypes.c_void_p(dev.data_ptr()), n, V, ctypes.c_void_p(index.ptr),
                                         ctypes.c_void_p(cls.ptr), cap, ctypes.c_void_p(off.ptr), ctypes.c_void_p(scratch.ptr),
                                         need, None))
    torch.cuda.synchronize()
    for g in (scratch, index, cls, off):      # index / cls hold exactly `cap` entries: the guard sits right behind entry cap
        assert g.guards_intact() == (True, True)
    return (off.view.cpu().numpy().view(np.int64).copy(), index.view.cpu().numpy().view(np.int32).copy(),
            cls.view.cpu().numpy().copy())


@pytest.mark.parametrize("n", [1, 3])
@pytest.mark.parametrize("shape", SHAPES, ids=_ids)
def test_labels_to_voxels_equals_flatnonzero(lib, shape, n):
    V = int(np.prod(shape))
    assert lib.ursn_labels_to_voxels_scratch_bytes(1, V) == 4 * -(-V // SPAN)     # pins SPAN, which places the seams above
    for j, kinds in enumerate(_VOLUMES[n]):
        labels = np.stack([_volume(k, V, 10 * j + i) for i, k in enumerate(kinds)])
        nz = [np.flatnonzero(labels[i]) for i in range(n)]
        want_off = np.concatenate([[0], np.cumsum([a.size for a in nz])]).astype(np.int64)
        want_idx = np.concatenate(nz).astype(np.int32)
        want_cls = np.concatenate([labels[i][nz[i]].astype(np.uint8) for i in range(n)])
        total = int(want_off[-1])
        runs = [_compact(lib, labels, total, fill) for fill in ("zero", "nan", "big")] + [_compact(lib, labels, total, "zero")]
        for off, idx, cls in runs:            # three scratch fills and a repeat: the same bits
            assert np.array_equal(off, want_off) and np.array_equal(idx, want_idx) and np.array_equal(cls, want_cls)
        if total >= 3:                        # three entries too few: true counts, the first `cap` entries, nothing behind them
            off, idx, cls = _compact(lib, labels, total - 3, "nan")
            assert np.array_equal(off, want_off)
            assert np.array_equal(idx, want_idx[:total - 3]) and np.array_equal(cls, want_cls[:total - 3])


# ---- net level ------------------------------------------------------------------------------------------------------------
NET_CASES = [((16, 16, 16, 1), "fp32"), ((16, 16, 16, 1), "bf16"), ((32, 32, 1), "fp32"), ((32, 32, 1), "bf16")]
_net_cache = {}


def _net_inputs(dims, n=2, first=0):
    """lartpc_sparse entries first .. first + n - 1 as dense arrays (weights normalised per event, lib/ssnet_trainval.py:173) and
    as the equivalent VoxelBatch."""
    key = (dims, n, first)
    if key not in _net_cache:
        ev = [sio.lartpc_sparse(dims, 3, first + e) for e in range(n)]
        data, label, weight = (np.stack([e[j] for e in ev]) for j in range(3))
        weight = weight / weight.sum(axis=1, keepdims=True)
        vb = VoxelBatch.concat([sio.dense_to_voxels(data[i], label[i], weight[i]) for i in range(n)]).validate()
        assert all(same_bits(a, b) for a, b in zip(sio.voxels_to_dense(vb), (data, label, weight)))
        _net_cache[key] = (data, label, weight, vb)
    return _net_cache[key]


def _build(dims, prec, trainable=True):
    net = uresnet(dims=list(dims), num_class=3, base_num_outputs=8, num_strides=3)
    net.construct(trainable=trainable, use_weight=True, learning_rate=1e-3, seed=7, precision=prec)
    return net


def _grads_equal(a, b):
    return all(same_bits(a[k], b[k]) for k in a)


@pytest.mark.parametrize("dims, prec", NET_CASES, ids=["%s_%s" % (_ids(d[:-1]), p) for d, p in NET_CASES])
def test_voxel_fed_step_eval_and_inference_equal_the_dense_ones(dims, prec):
    """The dense tensors ursn_voxels_to_dense writes carry the bits of the dense feed, and a call depends only on its
    arguments (include/uresnet_hip.h): gradients, metrics and labels are the same bits.

    h2d bytes: a listed voxel costs 16 bytes (index, value, label, weight) against 12 per voxel of the dense form, so the
    ratio is 4/3 of the occupancy plus the offsets.  The lartpc_sparse entries 0-1 used here list 77 + 86 of 2 x 4096 voxels at
    16^3 (2.0 %): 2.8 % of the dense bytes, and the issue's 5 % bound is asserted there.  At 32x32 the same generator lists
    125 + 122 of 2 x 1024 pixels (12 %): no list form of 16 bytes per entry can stay below 16 % there, so for that shape the
    test asserts the byte count itself (the packed sections), not the bound."""
    data, label, weight, vb = _net_inputs(dims)
    net = _build(dims, prec)
    net.zero_gradients(None)
    res_d, doc_d = net.accum_gradients(None, data, label, weight)
    g_d = net.get_gradients()
    dense_bytes = net.feed_stats['h2d_bytes']
    assert dense_bytes == data.nbytes + label.nbytes + weight.nbytes
    net.zero_gradients(None)
    res_v, doc_v = net.accum_gradients_voxels(None, vb)
    voxel_bytes = net.feed_stats['h2d_bytes'] - dense_bytes
    assert doc_v == doc_d and res_v == res_d and _grads_equal(net.get_gradients(), g_d)
    M, pad = int(vb.offsets[-1]), lambda b: (b + 15) & ~15
    assert voxel_bytes == pad(8 * (vb.n + 1)) + 4 * pad(4 * M) + pad(4 * vb.n)
    occupancy = M / float(vb.n * vb.voxels)
    print("%s: %d listed of %d voxels (%.1f %%), %d bytes against %d dense (%.1f %%)"
          % (_ids(dims), M, vb.n * vb.voxels, 100 * occupancy, voxel_bytes, dense_bytes, 100.0 * voxel_bytes / dense_bytes))
    if len(dims) == 4:
        assert occupancy < 0.03 and voxel_bytes < 0.05 * dense_bytes
    assert net.run_test_voxels(None, vb) == net.run_test(None, data, label, weight)
    lab_d, acc_all, acc_nz = net.inference_labels(None, data, label)
    sets, acc_all_v, acc_nz_v = net.inference_voxels(None, vb)
    assert (acc_all_v, acc_nz_v) == (acc_all, acc_nz)
    flat = lab_d.reshape(vb.n, -1)
    assert (flat != 0).any()
    for i, (index, cls) in enumerate(sets):
        assert index.dtype == np.int32 and cls.dtype == np.uint8
        assert np.array_equal(index, np.flatnonzero(flat[i])) and np.array_equal(cls, flat[i][index].astype(np.uint8))
    assert len(net.inference_voxels(None, vb, with_labels=False)) == 1
    bad = VoxelBatch(vb.offsets, vb.index.copy(), vb.value, vb.label, vb.weight, vb.bg_weight, vb.voxels)
    bad.index[1] = bad.index[0]
    calls = net.feed_stats['h2d_calls']
    with pytest.raises(ValueError):
        net.accum_gradients_voxels(None, bad)
    assert net.feed_stats['h2d_calls'] == calls          # refused before anything reached the device


@pytest.mark.parametrize("dims, prec", NET_CASES[:1] + NET_CASES[3:], ids=["16x16x16_fp32", "32x32_bf16"])
def test_three_voxel_batches_back_to_back_without_fetch(dims, prec):
    """fetch=False never waits for compute: the list and dense buffers of batch k + 2 reuse those of batch k, ordered by the
    consumed / copied events only.  Same bits as feeding with fetch=True."""
    batches = [_net_inputs(dims, 2, first)[3] for first in (0, 2, 4)]
    net = _build(dims, prec)
    net.zero_gradients(None)
    rows = [net.accum_gradients_voxels(None, vb, fetch=True)[0][1:] for vb in batches]
    g_sync = net.get_gradients()
    net.zero_gradients(None)
    for vb in batches:
        assert net.accum_gradients_voxels(None, vb, fetch=False)[0] is None
    assert net.read_metrics() == rows[-1]
    assert _grads_equal(net.get_gradients(), g_sync)


# ---- driver ---------------------------------------------------------------------------------------------------------------
def _cfgs(tmp_path, sparse, tag):
    inp = tmp_path / "input.cfg"
    inp.write_text("Dims [32, 32, 32, 1]\nNumClass 3\nGenerator 'lartpc_sparse'\nNumEntries 64\n"
                   "Keys {'data': 'data', 'label': 'label', 'weight': 'weight'}\n")
    train = tmp_path / ("train_%s.cfg" % tag)
    train.write_text("NUM_CLASS 3\nBASE_NUM_FILTERS 4\nMAIN_INPUT_CONFIG '%s'\nTEST_INPUT_CONFIG '%s'\nLOGDIR '%s'\nSAVE_FILE '%s'\n"
                     "ITERATIONS 3\nMINIBATCH_SIZE 2\nNUM_MINIBATCHES 2\nTEST_BATCH_SIZE 2\nLEARNING_RATE 0.001\nTRAIN True\n"
                     "USE_WEIGHTS True\nREPORT_STEPS 1\nSUMMARY_STEPS 2\nCHECKPOINT_STEPS 2\nSPARSE_IO %s\n"
                     % (inp, inp, tmp_path / ("log_" + tag), tmp_path / ("ckpt_" + tag) / "uresnet", sparse))
    out = tmp_path / ("ssnet_%s.npy" % tag)
    ana = tmp_path / ("ana_%s.cfg" % tag)
    ana.write_text("NUM_CLASS 3\nBASE_NUM_FILTERS 4\nMAIN_INPUT_CONFIG '%s'\nANA_OUTPUT_CONFIG '%s'\nLOGDIR ''\nSAVE_FILE ''\n"
                   "ITERATIONS 2\nMINIBATCH_SIZE 2\nTRAIN False\nUSE_WEIGHTS False\nSUMMARY_STEPS 0\nCHECKPOINT_STEPS 0\n"
                   "SPARSE_IO %s\n" % (inp, out, sparse))
    return train, ana, out


def test_driver_trains_and_writes_voxel_sets_with_sparse_io(tmp_path, capsys):
    from uresnet_amd.ssnet_trainval import ssnet_trainval
    train, ana, out_sparse = _cfgs(tmp_path, True, "sparse")
    t = ssnet_trainval()
    t.override_config(str(train))
    t.initialize()
    t.batch_process()
    printed = capsys.readouterr().out
    assert printed.count("@ iteration") == 3 and "Train set: loss=" in printed and "Test set: loss=" in printed
    assert "saved @" in printed and (tmp_path / "ckpt_sparse" / "uresnet-1.npz").is_file()
    assert t._net.feed_stats['h2d_bytes'] < 0.05 * (3 * 2 * 2 * 3 * 32 ** 3 * 4)     # six training batches, never dense
    t.reset()

    _, ana_dense, out_dense = _cfgs(tmp_path, False, "dense")
    for cfg in (ana, ana_dense):
        a = ssnet_trainval()
        a.override_config(str(cfg))
        a.initialize()
        a.batch_process()
        if cfg is ana:
            r = a.ana_step()                  # interactive mode: the reference's dense-shaped dictionary, one more record pair
            assert set(r) == {'entries', 'input', 'label', 'softmax', 'acc_all', 'acc_nonzero'}
            assert r['softmax'].shape == (2, 32, 32, 32, 3) and r['input'].shape == (2, 32, 32, 32, 1)
            want = np.stack([sio.lartpc_sparse([32, 32, 32, 1], 3, e)[0] for e in r['entries']])
            assert same_bits(r['input'].reshape(2, -1), want)
        a.reset()
    with open(str(out_sparse), "rb") as fs, open(str(out_dense), "rb") as fd:
        for e in range(4):
            index, cls, dense = np.load(fs), np.load(fs), np.load(fd).reshape(-1)
            assert index.dtype == np.int32 and cls.dtype == np.uint8 and index.size > 0
            assert np.array_equal(index, np.flatnonzero(dense)) and np.array_equal(cls, dense[index].astype(np.uint8))
        for e in range(2):                    # the interactive step's records are well formed too
            index, cls = np.load(fs), np.load(fs)
            assert index.shape == cls.shape and set(np.unique(cls)) <= {1, 2}
