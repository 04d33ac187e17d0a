"""Voxel-list I/O, host side (no GPU): the dense <-> list conversion of synthetic_io, VoxelBatch.validate(), the list-side
weight normalisation (lib/ssnet_trainval.py:173), the SPARSE_IO flag, and the argument refusals of the two C entry points
(include/uresnet_hip.h: they return before any device access, so they run without a device).  Every comparison of arrays is
exact."""
import ctypes
import io
from contextlib import redirect_stdout

import numpy as np
import pytest

import uresnet_amd  # noqa: F401
from uresnet_amd import _lib, ssnet_config
from uresnet_amd import synthetic_io as sio
from uresnet_amd.ssnet import VoxelBatch
from _abi import same_bits


def _roundtrip(data, label, weight):
    vb = sio.dense_to_voxels(data, label, weight).validate()
    d, l, w = sio.voxels_to_dense(vb)
    assert same_bits(d[0], data) and same_bits(l[0], label) and same_bits(w[0], weight)
    return vb


@pytest.mark.parametrize("dims", [(32, 32, 1), (16, 16, 16, 1)], ids=["2d32", "3d16"])
@pytest.mark.parametrize("entry", range(5))
def test_roundtrip_lartpc_sparse(dims, entry):
    data, label, weight = sio.lartpc_sparse(dims, 3, entry)
    vb = _roundtrip(data, label, weight)
    assert vb.n == 1 and vb.voxels == label.size
    assert np.array_equal(vb.index, np.flatnonzero(label))          # background voxels carry the background weight: unlisted
    assert vb.bg_weight[0] == weight[np.flatnonzero(label == 0)[0]] and vb.bg_weight[0] > 0


def test_roundtrip_dense_uniform_lists_every_voxel():
    data, label, weight = sio.dense_uniform((16, 16, 16, 1), 3, 0)
    vb = _roundtrip(data, label, weight)
    assert vb.index.size == 4096 and vb.bg_weight[0] == 0.0        # no voxel with data == 0 and label == 0


def test_roundtrip_all_zero_event_has_an_empty_list():
    z = np.zeros(4096, np.float32)
    w = np.full(4096, 1.0 / 4096, np.float32)
    vb = _roundtrip(z, z, w)
    assert vb.index.size == 0 and list(vb.offsets) == [0, 0] and vb.bg_weight[0] == w[0]


def test_concat_and_batch_roundtrip():
    ev = [sio.lartpc_sparse((16, 16, 16, 1), 3, e) for e in range(3)]
    ev.insert(1, (np.zeros(4096, np.float32), np.zeros(4096, np.float32), np.full(4096, 0.5, np.float32)))
    vb = VoxelBatch.concat([sio.dense_to_voxels(*e) for e in ev]).validate()
    assert vb.n == 4 and vb.offsets[1] == vb.offsets[2]
    for got, j in zip(sio.voxels_to_dense(vb), range(3)):
        assert same_bits(got, np.stack([e[j] for e in ev]))


def _good():
    return VoxelBatch([0, 3, 3, 5], [1, 4, 9, 0, 9], np.ones(5), np.ones(5), np.ones(5), np.ones(3), voxels=10)


def test_validate_accepts_a_good_batch():
    assert _good().validate().n == 3          # 9 then 0 across an event seam is no decrease


@pytest.mark.parametrize("what, edit, text", [
    ("index == voxels", lambda b: b.index.__setitem__(2, 10), "index[2] = 10 outside"),
    ("negative index", lambda b: b.index.__setitem__(0, -1), "index[0] = -1 outside"),
    ("repeated index", lambda b: b.index.__setitem__(1, 1), "strictly increasing"),
    ("decreasing pair", lambda b: b.index.__setitem__(slice(0, 2), [4, 1]), "strictly increasing"),
    ("offsets[0] != 0", lambda b: b.offsets.__setitem__(0, 1), "offsets[0] = 1"),
    ("decreasing offsets", lambda b: b.offsets.__setitem__(1, 4), "offsets decrease"),
    ("length mismatch (value)", lambda b: setattr(b, "value", np.ones(4, np.float32)), "value has shape"),
    ("length mismatch (offsets[-1])", lambda b: b.offsets.__setitem__(3, 6), "index has shape"),
    ("length mismatch (bg_weight)", lambda b: setattr(b, "bg_weight", np.ones(2, np.float32)), "bg_weight has shape"),
], ids=lambda x: x if isinstance(x, str) and " " in x else "")
def test_validate_refuses(what, edit, text):
    b = _good()
    edit(b)
    with pytest.raises(ValueError) as e:
        b.validate()
    assert text in str(e.value), (what, str(e.value))


@pytest.mark.parametrize("dims", [(32, 32, 1), (16, 16, 16, 1)], ids=["2d32", "3d16"])
def test_list_side_weight_normalisation_sums_to_one(dims):
    ev = [sio.lartpc_sparse(dims, 3, e) for e in range(5)]
    vb = VoxelBatch.concat([sio.dense_to_voxels(*e) for e in ev])
    raw = VoxelBatch.concat([sio.dense_to_voxels(*e) for e in ev])
    vb.normalize_weights()
    assert vb.weight.dtype == np.float32 and vb.bg_weight.dtype == np.float32
    for i in range(vb.n):
        a, b = int(vb.offsets[i]), int(vb.offsets[i + 1])
        total = np.sum(vb.weight[a:b], dtype=np.float64) + (vb.voxels - (b - a)) * np.float64(vb.bg_weight[i])
        assert abs(total - 1.0) < 1e-6, (i, total)
        # one divisor per event: ratios between weights survive (to fp32 rounding of the quotient)
        s = np.float64(raw.bg_weight[i]) / np.float64(vb.bg_weight[i])
        assert np.allclose(raw.weight[a:b] / s, vb.weight[a:b], rtol=3e-7, atol=0)


def test_threadio_fetch_voxels_matches_the_dense_batch():
    tio = sio.synthetic_threadio()
    tio.configure({'filler_cfg': {'Dims': [16, 16, 16, 1], 'NumClass': 3, 'Generator': 'lartpc_sparse', 'NumEntries': 8}})
    with pytest.raises(RuntimeError):
        tio.fetch_voxels()
    tio.produce_voxels()
    tio.start_manager(2)
    for _ in range(2):
        tio.next()
        vb = tio.fetch_voxels().validate()
        dense = [tio.fetch_data(k).data() for k in ('data', 'label', 'weight')]
        for got, want in zip(sio.voxels_to_dense(vb), dense):
            assert same_bits(got, np.ascontiguousarray(want))
    tio.reset()


def test_sparse_io_flag(tmp_path):
    assert ssnet_config().SPARSE_IO is False
    p = tmp_path / "a.cfg"
    p.write_text("SPARSE_IO True\n")
    c = ssnet_config()
    with redirect_stdout(io.StringIO()):
        c.override(str(p))
    assert c.SPARSE_IO is True and ssnet_config().SPARSE_IO is False
    bad = tmp_path / "b.cfg"
    bad.write_text("SPARSE_IO 1\n")
    with redirect_stdout(io.StringIO()), pytest.raises(TypeError):
        ssnet_config().override(str(bad))


def test_voxel_methods_need_one_channel():
    from uresnet_amd import uresnet
    net = uresnet(dims=[32, 32, 2], num_class=3, base_num_outputs=4)
    net.construct(trainable=True, use_weight=True, allocate=False)
    for call in (lambda: net.accum_gradients_voxels(None, _good()), lambda: net.run_test_voxels(None, _good()),
                 lambda: net.inference_voxels(None, _good())):
        with pytest.raises((ValueError, RuntimeError)) as e:
            call()
        assert "dims[-1] must be 1" in str(e.value)


# ---- the C entry points refuse bad arguments before any device access -------------------------------------------------
def _batch(n=1, voxels=64, fake=0x1000):
    b = _lib.ursn_voxel_batch()
    b.n, b.voxels = n, voxels
    b.offsets = b.index = b.value = b.label = b.weight = b.bg_weight = fake
    return b


def test_voxels_to_dense_refusals(lib):
    P = ctypes.c_void_p(0x1000)      # never dereferenced: every call below is refused on its arguments
    assert lib.ursn_voxels_to_dense(None, P, P, P, None) != 0 and b"null" in lib.ursn_last_error()
    assert lib.ursn_voxels_to_dense(ctypes.byref(_batch()), None, P, P, None) != 0 and b"null" in lib.ursn_last_error()
    b = _batch()
    b.index = None
    assert lib.ursn_voxels_to_dense(ctypes.byref(b), P, P, P, None) != 0 and b"null" in lib.ursn_last_error()
    assert lib.ursn_voxels_to_dense(ctypes.byref(_batch(n=0)), P, P, P, None) != 0 and b"n = 0" in lib.ursn_last_error()
    assert lib.ursn_voxels_to_dense(ctypes.byref(_batch(voxels=0)), P, P, P, None) != 0 and b"voxels = 0" in lib.ursn_last_error()
    assert lib.ursn_voxels_to_dense(ctypes.byref(_batch(voxels=2 ** 31)), P, P, P, None) != 0 and b"2^31" in lib.ursn_last_error()
    b = _batch()
    b.weight = None                  # a weight output without a weight list
    assert lib.ursn_voxels_to_dense(ctypes.byref(b), P, P, P, None) != 0 and b"weight" in lib.ursn_last_error()


def test_labels_to_voxels_refusals(lib):
    P = ctypes.c_void_p(0x1000)
    need = lib.ursn_labels_to_voxels_scratch_bytes(3, 8448)
    assert need >= 3 * 4 and lib.ursn_labels_to_voxels_scratch_bytes(0, 8448) == 0
    assert lib.ursn_labels_to_voxels(None, 1, 64, P, P, 8, P, P, need, None) != 0 and b"null" in lib.ursn_last_error()
    assert lib.ursn_labels_to_voxels(P, 1, 64, P, P, 8, P, None, need, None) != 0 and b"null" in lib.ursn_last_error()
    assert lib.ursn_labels_to_voxels(P, 0, 64, P, P, 8, P, P, need, None) != 0 and b"n = 0" in lib.ursn_last_error()
    assert lib.ursn_labels_to_voxels(P, 1, 0, P, P, 8, P, P, need, None) != 0 and b"voxels = 0" in lib.ursn_last_error()
    assert lib.ursn_labels_to_voxels(P, 1, 2 ** 31, P, P, 8, P, P, 1 << 30, None) != 0 and b"2^31" in lib.ursn_last_error()
    assert lib.ursn_labels_to_voxels(P, 3, 8448, P, P, 8, P, P, need - 1, None) != 0 and b"too small" in lib.ursn_last_error()
