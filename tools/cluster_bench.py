#!/usr/bin/env python
"""What the voxel clusters (cluster.hip, ssnet_base.cluster_voxels / set_clustering) cost, against what they replace.

Lists: --batch lartpc_sparse events at --size^3 (default 4 x 192^3), --dense-batch dense_uniform events at --dense-size^3 (every
voxel listed, three random classes: the worst case, one entry per voxel and no structure), and the stitched list of one tiled
batch, --tiled-batch lartpc_sparse events at --tiled-size^3 (default 2 x 256^3) in the large shape.  The class of an entry is its
true label: the passes do not care where the classes come from, and no network has to run.

Per list: the seven launches of ursn_cluster_voxels timed between device events (default spec: connectivity 26, every class but 0,
same_class, min_size 1), against a device-to-device copy of the list's index and class arrays (the floor of anything that reads the
list once), and against the host route the feature replaces: the D2H copy of the class array plus clusters.cluster_numpy (lists up
to --numpy-max entries; it is pure Python), and scipy.ndimage.label per class on the dense volume where scipy imports (the volume
is built on the host first; that is part of the route).  Medians over --repeats windows of --inner calls, ms per call; the host
routes run once.  Where cluster_numpy runs, the device ids are compared with it.

Prints a table and one JSON line.

    python tools/cluster_bench.py [--size 192] [--batch 4] [--dense-size 96] [--dense-batch 4] [--tiled-size 256] [--tiled-batch 2]
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
    from uresnet_amd.clusters import ClusterSpec, cluster_numpy
    from uresnet_amd.ssnet import VoxelBatch
    assert torch.cuda.is_available(), "cluster_bench: no HIP device visible"
    lib = _lib.load()
    spec = ClusterSpec()
    try:
        from scipy import ndimage
    except ImportError:
        ndimage = None

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
             ("dense_uniform", (args.dense_size,) * 3, events(sio.dense_uniform, (args.dense_size,) * 3, args.dense_batch)),
             ("tiled lartpc_sparse", (args.tiled_size,) * 3, events(sio.lartpc_sparse, (args.tiled_size,) * 3, args.tiled_batch))]
    out = {}
    stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    for name, shape, vb in cases:
        off, index, cls = vb.offsets.astype(np.int64), vb.index.astype(np.int32), vb.label.astype(np.uint8)
        n, M = vb.n, int(off[-1])
        d_off, d_index, d_cls = (torch.from_numpy(a).cuda() for a in (off, index, cls))
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
        run = lambda: _lib.check(lib.ursn_cluster_voxels(ctypes.byref(d), ctypes.byref(o), ctypes.c_void_p(scratch.data_ptr()), need,
                                                         stream))
        copies = [torch.empty_like(d_index), torch.empty_like(d_cls)]

        def copy():
            copies[0].copy_(d_index)
            copies[1].copy_(d_cls)
        run(), copy()
        torch.cuda.synchronize()
        assert int(ints[3 * M + n].item()) == 0, "a bounded device loop ran out"
        rec = dict(shape=list(shape), events=n, list_entries=M, clusters=int(toff[-1].item()), scratch_bytes=need,
                   device_ms=timed(run), copy_ms=timed(copy))
        t0 = time.perf_counter()
        host_cls = d_cls.cpu().numpy()
        rec["d2h_ms"] = (time.perf_counter() - t0) * 1e3
        if M <= args.numpy_max:
            t0 = time.perf_counter()
            want = [cluster_numpy(index[off[e]:off[e + 1]], host_cls[off[e]:off[e + 1]], shape, spec)[0] for e in range(n)]
            rec["numpy_ms"] = (time.perf_counter() - t0) * 1e3
            rec["same_ids"] = bool(np.array_equal(ints[:M].cpu().numpy(), np.concatenate(want)))
        if ndimage is not None:
            t0 = time.perf_counter()
            found = 0
            for e in range(n):
                dense = np.zeros(int(np.prod(shape)), np.uint8)
                dense[index[off[e]:off[e + 1]]] = host_cls[off[e]:off[e + 1]]
                dense = dense.reshape(shape)
                for k in (1, 2):
                    found += ndimage.label(dense == k, structure=np.ones((3, 3, 3), bool))[1]
            rec["scipy_ms"] = (time.perf_counter() - t0) * 1e3
            rec["scipy_clusters"] = found
        out[name] = rec
        print("%-20s %d x %d^3, %d entries, %d clusters: device %.3f ms, list copy %.3f ms | host: D2H %.3f ms, cluster_numpy %s, "
              "scipy on the dense volume %s%s"
              % (name, n, shape[0], M, rec["clusters"], rec["device_ms"], rec["copy_ms"], rec["d2h_ms"],
                 "%.0f ms" % rec["numpy_ms"] if "numpy_ms" in rec else "not run (> %d entries)" % args.numpy_max,
                 "%.0f ms (%d clusters)" % (rec["scipy_ms"], rec["scipy_clusters"]) if "scipy_ms" in rec else "no scipy",
                 "; ids equal cluster_numpy: %s" % rec["same_ids"] if "same_ids" in rec else ""))
        del scratch, ints, tcls, toff, copies
    out["repeats"], out["inner"] = args.repeats, args.inner
    print(json.dumps(out))


if __name__ == "__main__":
    main()
