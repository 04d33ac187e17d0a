#!/usr/bin/env python
"""What the voxel-list boundary costs and saves at the cfg3 shape (192^3, F = 8, batch 4, fp32, lartpc_sparse events).

    (a) dense_step   the training step fed from pinned dense host buffers every iteration (as bench.py --host-feed)
    (b) voxel_step   the same step fed from voxel lists (accum_gradients_voxels)
    (c) expand       ursn_voxels_to_dense alone, against the floor of writing 3 x n x voxels x 4 bytes at 6.3 TB/s
    (d) compact      ursn_labels_to_voxels alone on the label volume of one inference
    (e) bytes        H2D / D2H bytes per step (training feed) and per ana batch for each form

    (f) ana_scores   with --ana-scores, INSTEAD of (a)-(e): per-batch wall time and D2H bytes of inference_voxel_scores (class
                     scores, argmax class and ana label at the event's own voxels) against what the dense path must do for the
                     same information -- inference() with the dense softmax copied back plus a host gather -- on the same events in
                     the same session, alternating; plus the size of the vscores launch from ursn_profile_read

(a) and (b) are host clocks around `--steps` steps that end in a device synchronise, taken `--repeats` times in alternation
(a b a b ...) after a warm-up of both; (c) and (d) are HIP events around `--calls` back-to-back calls, `--repeats` times.
Every figure is reported as median with (min .. max).  `--lib PATH` times (c) a second time through another build of the
library (e.g. one compiled with -DURSN_VOXEL_FILL_NT=1), alternating with the default one.  Prints one JSON line.

    python tools/voxel_feed_bench.py [--steps 20] [--repeats 5] [--calls 50] [--lib other/liburesnet_hip.so]
    python tools/voxel_feed_bench.py --ana-scores [--steps 5] [--repeats 5]
"""
import argparse
import ctypes
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

HBM_WRITE_BPS = 6.3e12     # achievable HBM rate of a streaming float4 kernel on the MI355X (8 TB/s spec)


def stat(xs, digits=3):
    xs = sorted(xs)
    return {"median": round(float(np.median(xs)), digits), "min": round(xs[0], digits), "max": round(xs[-1], digits)}


def ana_scores(args):
    """Leg (f): the voxel-list output side against the dense softmax + host gather."""
    import torch
    import uresnet_amd  # noqa: F401
    from uresnet_amd import _lib, uresnet
    from uresnet_amd import synthetic_io as sio
    from uresnet_amd.ssnet import VoxelBatch
    assert torch.cuda.is_available(), "voxel_feed_bench.py needs a HIP device"
    lib = _lib.load()
    dims, ncls, n = (args.size,) * 3 + (1,), 3, args.batch
    V = args.size ** 3
    ev = [sio.lartpc_sparse(dims, ncls, e) for e in range(n)]
    data, label = (np.stack([e[j] for e in ev]) for j in range(2))
    vb = VoxelBatch.concat([sio.dense_to_voxels(e[0], e[1]) for e in ev]).validate()
    off, M = vb.offsets, int(vb.offsets[-1])
    pin = [torch.from_numpy(a).pin_memory().numpy() for a in (data, label)]
    net = uresnet(dims=list(dims), num_class=ncls, base_num_outputs=8)
    net.construct(trainable=False, use_weight=False, seed=1234)

    def dense():        # the softmax crosses PCIe whole; scores / class / ana label of the listed voxels on the host
        sm, acc_all, acc_nz = net.inference(None, pin[0], pin[1])
        out = []
        for i in range(n):
            idx = vb.index[off[i]:off[i + 1]]
            sc = sm[i].reshape(V, ncls)[idx]
            ana = ((sc[:, 1] > sc[:, 2]) * 1 + (sc[:, 2] >= sc[:, 1]) * 2) * (vb.value[off[i]:off[i + 1]] > 1.0)
            out.append((sc, sc.argmax(axis=1).astype(np.uint8), ana.astype(np.uint8)))
        return out

    def voxel():
        return net.inference_voxel_scores(None, vb)

    def timed(call):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(args.steps):
            call()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) / args.steps * 1e3

    want, got = dense(), voxel()        # warm-up of both, and the two forms agree bit for bit
    for i in range(n):
        assert np.array_equal(want[i][0].view(np.uint32), got['scores'][i].view(np.uint32))
        assert np.array_equal(want[i][1], got['pred'][i]) and np.array_equal(want[i][2], got['ana'][i])
    h0 = net.feed_stats['h2d_bytes']
    dense()
    h1 = net.feed_stats['h2d_bytes']
    voxel()
    h2 = net.feed_stats['h2d_bytes']
    ms = {"dense": [], "voxel": []}
    for _ in range(args.repeats):
        ms["dense"].append(timed(dense))
        ms["voxel"].append(timed(voxel))

    _lib.check(lib.ursn_profile_enable(net._handle, 1))
    kern = {}
    for name, call in (("voxel", voxel), ("dense", dense)):
        call()
        cnt = ctypes.c_int64(0)
        _lib.check(lib.ursn_profile_read(net._handle, None, 0, ctypes.byref(cnt)))
        recs = (_lib.ursn_prof_rec * max(int(cnt.value), 1))()
        _lib.check(lib.ursn_profile_read(net._handle, recs, int(cnt.value), ctypes.byref(cnt)))
        rows = [(r.kernel.decode(), r.pass_, r.ms, r.launches) for r in recs[:int(cnt.value)]]
        kern[name] = {"forward_ms": round(sum(r[2] for r in rows if r[1] != 6), 3),
                      "pass6": {r[0]: {"ms": round(r[2], 4), "launches": r[3]} for r in rows if r[1] == 6}}
    _lib.check(lib.ursn_profile_enable(net._handle, 0))
    print(json.dumps({
        "shape": "%d^3 F=8 batch %d fp32 inference, lartpc_sparse" % (args.size, n), "steps": args.steps, "repeats": args.repeats,
        "listed_voxels": M, "occupancy": round(M / float(n * V), 6),
        "dense_ana_ms": stat(ms["dense"]), "voxel_ana_ms": stat(ms["voxel"]),
        "bytes": {"d2h_dense": n * V * ncls * 4, "d2h_voxel": M * (4 * ncls + 2), "h2d_dense": h1 - h0, "h2d_voxel": h2 - h1},
        "kernels": kern,
    }))


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--calls", type=int, default=50)
    ap.add_argument("--size", type=int, default=192, help="edge of the cubic volume (192 = cfg3)")
    ap.add_argument("--batch", type=int, default=4)
    ap.add_argument("--lib", default=None, help="second build of liburesnet_hip.so for leg (c)")
    ap.add_argument("--ana-scores", action="store_true", help="leg (f) instead of (a)-(e)")
    args = ap.parse_args()
    if args.ana_scores:
        return ana_scores(args)

    import torch
    import uresnet_amd  # noqa: F401
    from uresnet_amd import _lib, uresnet
    from uresnet_amd import synthetic_io as sio
    from uresnet_amd.ssnet import VoxelBatch
    assert torch.cuda.is_available(), "voxel_feed_bench.py needs a HIP device"
    lib = _lib.load()
    dims, ncls, n = (args.size,) * 3 + (1,), 3, args.batch
    V = args.size ** 3
    ev = [sio.lartpc_sparse(dims, ncls, e) for e in range(n)]
    data, label, weight = (np.stack([e[j] for e in ev]) for j in range(3))
    vb = VoxelBatch.concat([sio.dense_to_voxels(*e) for e in ev]).normalize_weights().validate()
    weight /= weight.sum(axis=1, keepdims=True)           # lib/ssnet_trainval.py:173
    pin = [torch.from_numpy(a).pin_memory().numpy() for a in (data, label, weight)]
    net = uresnet(dims=list(dims), num_class=ncls, base_num_outputs=8)
    net.construct(trainable=True, use_weight=True, learning_rate=1e-4, seed=1234)

    def dense_step():
        net.zero_gradients(None)
        net.accum_gradients(None, pin[0], pin[1], pin[2], fetch=False)
        net.apply_gradients(None)

    def voxel_step():
        net.zero_gradients(None)
        net.accum_gradients_voxels(None, vb, fetch=False)
        net.apply_gradients(None)

    def timed(step):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(args.steps):
            step()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) / args.steps * 1e3

    for _ in range(3):
        dense_step()
        voxel_step()
    net._copy_stream()
    b0 = net.feed_stats['h2d_bytes']
    dense_step()
    b1 = net.feed_stats['h2d_bytes']
    voxel_step()
    b2 = net.feed_stats['h2d_bytes']
    ms = {"dense": [], "voxel": []}
    for _ in range(args.repeats):
        ms["dense"].append(timed(dense_step))
        ms["voxel"].append(timed(voxel_step))

    # ---- (c) the expansion alone ------------------------------------------------------------------------------------------
    dev = [torch.from_numpy(a).cuda() for a in (vb.offsets, vb.index, vb.value, vb.label, vb.weight, vb.bg_weight)]
    b = _lib.ursn_voxel_batch()
    b.n, b.voxels = n, V
    b.offsets, b.index, b.value, b.label, b.weight, b.bg_weight = (t.data_ptr() for t in dev)
    out = [torch.empty((n, V), dtype=torch.float32, device="cuda") for _ in range(3)]
    optr = [ctypes.c_void_p(t.data_ptr()) for t in out]
    stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)

    def events_us(call):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(args.calls):
            call()
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1) / args.calls * 1e3

    def expand_with(L):
        fn = L.ursn_voxels_to_dense
        return lambda: _lib.check(fn(ctypes.byref(b), optr[0], optr[1], optr[2], stream))
    libs = {"default": expand_with(lib)}
    if args.lib:
        other = ctypes.CDLL(os.path.abspath(args.lib))
        other.ursn_voxels_to_dense.restype = ctypes.c_int
        other.ursn_voxels_to_dense.argtypes = lib.ursn_voxels_to_dense.argtypes
        libs["other"] = expand_with(other)
    for call in libs.values():
        events_us(call)
    expand = {k: [] for k in libs}
    for _ in range(args.repeats):
        for k, call in libs.items():
            expand[k].append(events_us(call))
    want = sio.voxels_to_dense(vb)
    assert all(np.array_equal(t.cpu().numpy().view(np.uint32), w.view(np.uint32)) for t, w in zip(out, want))
    floor_us = 3.0 * n * V * 4 / HBM_WRITE_BPS * 1e6

    # ---- (d) the compaction alone, on the label volume of one inference ---------------------------------------------------
    labels = net.inference_labels(None, out[0], out[1], as_numpy=False)[0].reshape(n, V).contiguous()
    cap = int(np.count_nonzero(vb.value > 1.0))
    index = torch.empty(max(cap, 1), dtype=torch.int32, device="cuda")
    cls = torch.empty(max(cap, 1), dtype=torch.uint8, device="cuda")
    offs = torch.empty(n + 1, dtype=torch.int64, device="cuda")
    sbytes = int(lib.ursn_labels_to_voxels_scratch_bytes(n, V))
    scratch = torch.empty(sbytes, dtype=torch.uint8, device="cuda")
    P = lambda t: ctypes.c_void_p(t.data_ptr())

    def compact():
        _lib.check(lib.ursn_labels_to_voxels(P(labels), n, V, P(index), P(cls), cap, P(offs), P(scratch), sbytes, stream))
    events_us(compact)
    comp = [events_us(compact) for _ in range(args.repeats)]
    host = labels.cpu().numpy()
    total = int(offs.cpu()[-1])
    assert total == int(np.count_nonzero(host)) and total <= cap
    assert np.array_equal(index[:total].cpu().numpy(), np.concatenate([np.flatnonzero(h) for h in host]))

    res = {
        "shape": "%d^3 F=8 batch %d fp32, lartpc_sparse" % (args.size, n), "steps": args.steps, "repeats": args.repeats,
        "listed_voxels": int(vb.offsets[-1]), "occupancy": round(int(vb.offsets[-1]) / float(n * V), 6),
        "dense_step_ms": stat(ms["dense"]), "voxel_step_ms": stat(ms["voxel"]),
        "expand_us": {k: stat(v, 1) for k, v in expand.items()},
        "expand_floor_us": round(floor_us, 1),
        "expand_over_floor": round(float(np.median(expand["default"])) / floor_us, 2),
        "compact_us": stat(comp, 1), "compact_read_floor_us": round(2.0 * n * V * 4 / HBM_WRITE_BPS * 1e6, 1),
        "labelled_voxels": total,
        "bytes": {"train_h2d_dense": b1 - b0, "train_h2d_voxel": b2 - b1,
                  "ana_d2h_dense": n * V * 4, "ana_d2h_voxel": 8 * (n + 1) + 5 * total},
    }
    print(json.dumps(res))


if __name__ == "__main__":
    main()
