#!/usr/bin/env python
"""What the per-cluster object records (cluster_features.hip, ssnet_base.cluster_features / set_cluster_features) cost, against what
they replace.

Lists: those of tools/cluster_bench.py -- --batch lartpc_sparse events at --size^3 (default 4 x 192^3), the stitched list of one tiled
batch, --tiled-batch lartpc_sparse events at --tiled-size^3 (default 2 x 256^3) -- and --dense-batch dense_uniform events at
--dense-size^3 (default 4 x 96^3: every voxel listed, three random classes, the worst case).  The class of an entry is its true
label; ursn_cluster_voxels (default spec) makes the ids on the device first, and that call is timed too.

Per list, between device events: the seven launches of ursn_cluster_features with the wave combining (the default) and with one
atomic per entry (URSN_CLFEAT_WAVE=0), a device-to-device copy of the list (index, value, ids: the floor of anything that reads it
once), and ursn_cluster_voxels alone.  Host routes, once each: the D2H copy of ids and values, then clusters.cluster_features_numpy
(lists up to --numpy-max entries: it is pure Python) and a vectorised numpy version (np.add.at moments around the same anchor,
np.linalg.eigh, projections, extreme members by sorting), the fair host competitor.  Medians over --repeats windows of --inner calls,
ms per call.  Where the statement runs, the device tables are compared with it bit for bit.

Prints a table and one JSON line.

    python tools/cluster_features_bench.py [--size 192] [--batch 4] [--dense-size 96] [--dense-batch 4] [--tiled-size 256]
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


def vectorised_numpy(off, index, value, cluster, toff, shape):
    """The fair host competitor: the same quantities with numpy's own reductions (fp64 sums, eigh); not bit-compatible."""
    ev = np.searchsorted(off, np.arange(index.size), side="right") - 1
    keep = np.flatnonzero(cluster >= 0)
    row = cluster[keep] + toff[ev[keep]]
    K = int(toff[-1])
    x = np.stack(np.unravel_index(index[keep], shape), axis=1).astype(np.int64)
    n = np.bincount(row, minlength=K)
    s = np.zeros((K, 3), np.int64)
    np.add.at(s, row, x)
    charge = np.bincount(row, weights=value[keep].astype(np.float64), minlength=K)
    m = (2 * s + n[:, None]) // np.maximum(2 * n[:, None], 1)
    dx = (x - m[row]).astype(np.float64)
    d = np.zeros((K, 3))
    np.add.at(d, row, dx)
    dd = np.zeros((K, 3, 3))
    np.add.at(dd, row, dx[:, :, None] * dx[:, None, :])
    fn = np.maximum(n, 1)[:, None].astype(np.float64)
    mean = d / fn
    cov = dd / fn[:, :, None] - mean[:, :, None] * mean[:, None, :]
    w, v = np.linalg.eigh(cov)
    axis = v[:, :, 2]
    t = np.einsum("ij,ij->i", axis[row], dx).astype(np.float32)
    order = np.lexsort((keep, t, row))                      # by row, then t, then position
    start = np.concatenate([[0], np.cumsum(n)])[:-1]
    end_lo = keep[order[start]]
    order_hi = np.lexsort((-keep, t, row))
    end_hi = keep[order_hi[start + n - 1]]
    return n, charge, s / fn, w[:, ::-1], axis, end_lo, end_hi


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", type=int, default=192)
    ap.add_argument("--batch", type=int, default=4)
    ap.add_argument("--dense-size", type=int, default=96)
    ap.add_argument("--dense-batch", type=int, default=4)
    ap.add_argument("--tiled-size", type=int, default=256)
    ap.add_argument("--tiled-batch", type=int, default=2)
    ap.add_argument("--numpy-max", type=int, default=200000)
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--inner", type=int, default=5)
    args = ap.parse_args()
    import torch
    from uresnet_amd import _lib
    from uresnet_amd import synthetic_io as sio
    from uresnet_amd.clusters import ClusterSpec, cluster_features_numpy
    from uresnet_amd.ssnet import VoxelBatch
    assert torch.cuda.is_available(), "cluster_features_bench: no HIP device visible"
    lib = _lib.load()
    spec = ClusterSpec()
    I, R = _lib.CLFEAT_I, _lib.CLFEAT_R

    def timed(fn):
        ms = []
        for _ in range(args.repeats):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            for _ in range(args.inner):
                fn()
            b.record()
            b.synchronize()
            ms.append(a.elapsed_time(b) / args.inner)
        return float(np.median(ms))

    def events(gen, shape, n):
        return VoxelBatch.concat([sio.dense_to_voxels(*gen(list(shape) + [1], 3, e)) for e in range(n)])

    cases = [("lartpc_sparse", (args.size,) * 3, events(sio.lartpc_sparse, (args.size,) * 3, args.batch)),
             ("tiled lartpc_sparse", (args.tiled_size,) * 3, events(sio.lartpc_sparse, (args.tiled_size,) * 3, args.tiled_batch)),
             ("dense_uniform", (args.dense_size,) * 3, events(sio.dense_uniform, (args.dense_size,) * 3, args.dense_batch))]
    out = {}
    stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    for name, shape, vb in cases:
        off, index, cls = vb.offsets.astype(np.int64), vb.index.astype(np.int32), vb.label.astype(np.uint8)
        value = vb.value.astype(np.float32)
        n, M = vb.n, int(off[-1])
        d_off, d_index, d_cls, d_value = (torch.from_numpy(a).cuda() for a in (off, index, cls, value))
        need = int(lib.ursn_cluster_scratch_bytes(n, M))
        scratch = torch.empty(need // 8, dtype=torch.int64, device="cuda")
        ints = torch.empty(3 * M + n + 1, dtype=torch.int32, device="cuda")
        tcls, toff = torch.empty(M, dtype=torch.uint8, device="cuda"), torch.empty(n + 1, dtype=torch.int64, device="cuda")
        d = _lib.ursn_cluster_desc()
        d.ndim, d.n, d.m_total = 3, n, M
        for i, s in enumerate(shape):
            d.spatial[i] = s
        d.offsets, d.index, d.cls = d_off.data_ptr(), d_index.data_ptr(), d_cls.data_ptr()
        d.connectivity, d.class_mask, d.same_class, d.min_size = 26, spec.class_mask(), 1, 1
        o = _lib.ursn_cluster_out()
        base = ints.data_ptr()
        o.cluster, o.first, o.size, o.count, o.status = base, base + 4 * M, base + 8 * M, base + 12 * M, base + 12 * M + 4 * n
        o.cls, o.table_offsets, o.cap = tcls.data_ptr(), toff.data_ptr(), M
        clusters = lambda: _lib.check(lib.ursn_cluster_voxels(ctypes.byref(d), ctypes.byref(o), ctypes.c_void_p(scratch.data_ptr()),
                                                              need, stream))
        clusters()
        torch.cuda.synchronize()
        assert int(ints[3 * M + n].item()) == 0, "a bounded device loop ran out"
        K = int(toff[-1].item())

        fneed = int(lib.ursn_cluster_features_scratch_bytes(n, M, K))
        fscratch = torch.empty(fneed // 8, dtype=torch.int64, device="cuda")
        itab = torch.empty((max(K, 1), I), dtype=torch.int64, device="cuda")
        rtab = torch.empty((max(K, 1), R), dtype=torch.float64, device="cuda")
        status = torch.empty(1, dtype=torch.int32, device="cuda")
        fd = _lib.ursn_cluster_feat_desc()
        fd.ndim, fd.n, fd.m_total = 3, n, M
        for i, s in enumerate(shape):
            fd.spatial[i] = s
        fd.offsets, fd.index, fd.value, fd.cluster, fd.table_offsets = d_off.data_ptr(), d_index.data_ptr(), d_value.data_ptr(), base, \
            toff.data_ptr()
        fo = _lib.ursn_cluster_feat_out()
        fo.itab, fo.rtab, fo.cap, fo.status = itab.data_ptr(), rtab.data_ptr(), K, status.data_ptr()
        features = lambda: _lib.check(lib.ursn_cluster_features(ctypes.byref(fd), ctypes.byref(fo),
                                                                ctypes.c_void_p(fscratch.data_ptr()), fneed, stream))
        copies = [torch.empty_like(d_index), torch.empty_like(d_value), torch.empty(M, dtype=torch.int32, device="cuda")]

        def copy():
            copies[0].copy_(d_index)
            copies[1].copy_(d_value)
            copies[2].copy_(ints[:M])
        features(), copy()
        torch.cuda.synchronize()
        assert int(status.item()) == 0, "cluster_features: status %d" % int(status.item())
        wave_tabs = (itab.cpu().numpy().copy(), rtab.cpu().numpy().copy())
        rec = dict(shape=list(shape), events=n, list_entries=M, clusters=K, scratch_bytes=fneed, features_wave_ms=timed(features))
        os.environ["URSN_CLFEAT_WAVE"] = "0"
        try:
            features()
            torch.cuda.synchronize()
            rec["routes_same_bits"] = bool(np.array_equal(itab.cpu().numpy(), wave_tabs[0]) and
                                           np.array_equal(rtab.cpu().numpy().view(np.int64), wave_tabs[1].view(np.int64)))
            rec["features_plain_ms"] = timed(features)
        finally:
            os.environ.pop("URSN_CLFEAT_WAVE", None)
        rec["copy_ms"], rec["cluster_voxels_ms"] = timed(copy), timed(clusters)
        t0 = time.perf_counter()
        host_ids, host_value, host_toff = ints[:M].cpu().numpy(), d_value.cpu().numpy(), toff.cpu().numpy()
        rec["d2h_ms"] = (time.perf_counter() - t0) * 1e3
        t0 = time.perf_counter()
        vectorised_numpy(off, index.astype(np.int64), host_value, host_ids.astype(np.int64), host_toff, shape)
        rec["numpy_vectorised_ms"] = (time.perf_counter() - t0) * 1e3
        if M <= args.numpy_max:
            t0 = time.perf_counter()
            want = cluster_features_numpy(off, index, host_value, host_ids, host_toff, shape)
            rec["statement_ms"] = (time.perf_counter() - t0) * 1e3
            it, rt = wave_tabs
            rec["same_bits"] = bool(
                all(np.array_equal(it[:, a:a + w].reshape(want[k].shape), want[k]) for k, a, w in (
                    ("n", 0, 1), ("charge", 1, 1), ("s", 2, 3), ("lo", 5, 3), ("hi", 8, 3), ("m", 11, 3), ("d", 14, 3), ("dd", 17, 6),
                    ("flags", 23, 1), ("end_lo", 24, 1), ("end_hi", 25, 1))) and
                all(np.array_equal(rt[:, a:a + w].reshape(want[k].shape).view(np.int64), want[k].astype(np.float64).view(np.int64))
                    for k, a, w in (("centroid", 0, 3), ("cov", 3, 6), ("eval", 9, 3), ("axis", 12, 3), ("length", 15, 1),
                                    ("t_lo", 16, 1), ("t_hi", 17, 1))))
        out[name] = rec
        print("%-20s %d x %d^3, %d entries, %d clusters: features %.3f ms (one atomic per entry: %.3f ms, same bits: %s), list copy "
              "%.3f ms, cluster_voxels %.3f ms | host: D2H %.3f ms, vectorised numpy %.0f ms, statement %s%s"
              % (name, n, shape[0], M, K, rec["features_wave_ms"], rec["features_plain_ms"], rec["routes_same_bits"], rec["copy_ms"],
                 rec["cluster_voxels_ms"], rec["d2h_ms"], rec["numpy_vectorised_ms"],
                 "%.0f ms" % rec["statement_ms"] if "statement_ms" in rec else "not run (> %d entries)" % args.numpy_max,
                 "; device == statement: %s" % rec["same_bits"] if "same_bits" in rec else ""))
        del scratch, ints, tcls, toff, copies, fscratch, itab, rtab
    out["repeats"], out["inner"] = args.repeats, args.inner
    print(json.dumps(out))


if __name__ == "__main__":
    main()
