#!/usr/bin/env python
"""What the per-cluster charge profiles (cluster_profile.hip, ssnet_base.cluster_profiles / set_cluster_profiles) cost, against what
they replace.

Lists: those of tools/cluster_features_bench.py -- --batch lartpc_sparse events at --size^3 (default 4 x 192^3), the stitched list
of one tiled batch, --tiled-batch lartpc_sparse events at --tiled-size^3 (default 2 x 256^3) -- and --dense-batch dense_uniform
events at --dense-size^3 (default 4 x 96^3: every voxel listed, three random classes, the worst case).  The class of an entry is
its true label; ursn_cluster_voxels (default spec) and ursn_cluster_features make the ids and the object records on the device
first.  The bin table is sized exactly from the lengths, as ssnet_base.cluster_profiles does.

Per list, between device events: the six launches of ursn_cluster_profile with the combining (the default) and with one atomic set
per entry (URSN_CLPROF_WAVE=0), a device-to-device copy of the list (index, value, ids: the floor of anything that reads it once),
and ursn_cluster_features alone.  Host routes, once each: a vectorised numpy version (the bins by the same expressions on whole
arrays, np.add.at sums; the row records are left out, which favours it) and clusters.cluster_profile_numpy (lists up to --numpy-max
entries: it is pure Python, and it includes the object records).  Medians over --repeats windows of --inner calls, ms per call.
Where the statement runs, the device tables are compared with it bit for bit.

Prints a table and one JSON line.

    python tools/cluster_profile_bench.py [--size 192] [--batch 4] [--dense-size 96] [--dense-batch 4] [--tiled-size 256] [--step 1.0]
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


def vectorised_numpy(off, index, value, cluster, toff, shape, m, axis, t_lo, length, step, max_bins):
    """The fair host competitor for the bin records: the statement's expressions on whole arrays, np.add.at for the sums."""
    ev = np.searchsorted(off, np.arange(index.size), side="right") - 1
    keep = np.flatnonzero(cluster >= 0)
    row = cluster[keep] + toff[ev[keep]]
    x = np.stack(np.unravel_index(index[keep], shape), axis=1).astype(np.int64)
    dx = x - m[row]
    t = ((axis[row, 0] * dx[:, 0] + axis[row, 1] * dx[:, 1]) + axis[row, 2] * dx[:, 2]).astype(np.float32)
    nb_true = np.floor(length / step).astype(np.int64) + 1
    nb = np.minimum(nb_true, max_bins)
    pad = (nb_true.astype(np.float64) * step - length) / 2.0
    boff = np.concatenate([[0], np.cumsum(nb)])
    u = ((t.astype(np.float64) - t_lo[row].astype(np.float64)) + pad[row]) / step
    b = np.minimum(np.maximum(np.floor(u).astype(np.int64), 0), nb[row] - 1)
    g = boff[row] + b
    B = int(boff[-1])
    n = np.bincount(g, minlength=B)
    v = value[keep].astype(np.float64)
    ok = np.isfinite(v) & (np.abs(v) < 32768.0)
    q = np.zeros(B, np.int64)
    np.add.at(q, g[ok], np.rint(v[ok] * 65536.0).astype(np.int64))
    d = np.zeros((B, 3), np.int64)
    np.add.at(d, g, dx)
    return boff, n, q, d


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", type=int, default=192)
    ap.add_argument("--batch", type=int, default=4)
    ap.add_argument("--dense-size", type=int, default=96)
    ap.add_argument("--dense-batch", type=int, default=4)
    ap.add_argument("--tiled-size", type=int, default=256)
    ap.add_argument("--tiled-batch", type=int, default=2)
    ap.add_argument("--step", type=float, default=1.0)
    ap.add_argument("--numpy-max", type=int, default=200000)
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--inner", type=int, default=5)
    args = ap.parse_args()
    import torch
    from uresnet_amd import _lib
    from uresnet_amd import synthetic_io as sio
    from uresnet_amd.clusters import (PROFILE_BIN_INT, PROFILE_BIN_REAL, PROFILE_ROW_INT, PROFILE_ROW_REAL, ClusterProfileSpec,
                                      ClusterSpec, cluster_profile_numpy)
    from uresnet_amd.ssnet import VoxelBatch
    assert torch.cuda.is_available(), "cluster_profile_bench: no HIP device visible"
    lib = _lib.load()
    spec, pspec = ClusterSpec(), ClusterProfileSpec(args.step)
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
        _lib.check(lib.ursn_cluster_voxels(ctypes.byref(d), ctypes.byref(o), ctypes.c_void_p(scratch.data_ptr()), need, stream))
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
        features()
        torch.cuda.synchronize()
        assert int(status.item()) == 0, "cluster_features: status %d" % int(status.item())
        host_it, host_rt = itab.cpu().numpy(), rtab.cpu().numpy()
        length = host_rt[:K, 15]
        nb = np.minimum(np.floor(length / pspec.step).astype(np.int64) + 1, pspec.max_bins)
        B = int(nb.sum())

        pneed = int(lib.ursn_cluster_profile_scratch_bytes(n, M, K, B))
        pscratch = torch.empty(pneed // 8, dtype=torch.int64, device="cuda")
        boff = torch.empty(K + 1, dtype=torch.int64, device="cuda")
        bi = torch.empty((max(B, 1), _lib.CLPROF_BI), dtype=torch.int64, device="cuda")
        br = torch.empty((max(B, 1), _lib.CLPROF_BR), dtype=torch.float64, device="cuda")
        ri = torch.empty((max(K, 1), _lib.CLPROF_RI), dtype=torch.int64, device="cuda")
        rr = torch.empty((max(K, 1), _lib.CLPROF_RR), dtype=torch.float64, device="cuda")
        pstatus = torch.empty(1, dtype=torch.int32, device="cuda")
        pd = _lib.ursn_cluster_prof_desc()
        pd.ndim, pd.n, pd.m_total = 3, n, M
        for i, s in enumerate(shape):
            pd.spatial[i] = s
        pd.offsets, pd.index, pd.value, pd.cluster, pd.table_offsets = d_off.data_ptr(), d_index.data_ptr(), d_value.data_ptr(), base, \
            toff.data_ptr()
        pd.itab, pd.rtab, pd.feat_cap = itab.data_ptr(), rtab.data_ptr(), K
        pd.step, pd.end_bins, pd.max_bins = pspec.step, pspec.end_bins, pspec.max_bins
        po = _lib.ursn_cluster_prof_out()
        po.bin_offsets, po.bin_itab, po.bin_rtab, po.row_itab, po.row_rtab = boff.data_ptr(), bi.data_ptr(), br.data_ptr(), \
            ri.data_ptr(), rr.data_ptr()
        po.cap_rows, po.bin_cap, po.status = K, B, pstatus.data_ptr()
        profile = lambda: _lib.check(lib.ursn_cluster_profile(ctypes.byref(pd), ctypes.byref(po),
                                                              ctypes.c_void_p(pscratch.data_ptr()), pneed, stream))
        copies = [torch.empty_like(d_index), torch.empty_like(d_value), torch.empty(M, dtype=torch.int32, device="cuda")]

        def copy():
            copies[0].copy_(d_index)
            copies[1].copy_(d_value)
            copies[2].copy_(ints[:M])

        def tables():
            return [t.cpu().numpy().copy() for t in (boff, bi, br, ri, rr)]
        profile(), copy()
        torch.cuda.synchronize()
        assert int(pstatus.item()) == 0, "cluster_profile: status %d" % int(pstatus.item())
        wave = tables()
        rec = dict(shape=list(shape), events=n, list_entries=M, clusters=K, bins=B, step=pspec.step, scratch_bytes=pneed,
                   profile_wave_ms=timed(profile))
        os.environ["URSN_CLPROF_WAVE"] = "0"
        try:
            profile()
            torch.cuda.synchronize()
            rec["routes_same_bits"] = bool(all(np.array_equal(a.view(np.int64), b.view(np.int64)) for a, b in zip(tables(), wave)))
            rec["profile_plain_ms"] = timed(profile)
        finally:
            os.environ.pop("URSN_CLPROF_WAVE", None)
        rec["copy_ms"], rec["features_ms"] = timed(copy), timed(features)
        t0 = time.perf_counter()
        host_ids, host_value, host_toff = ints[:M].cpu().numpy(), d_value.cpu().numpy(), toff.cpu().numpy()
        rec["d2h_ms"] = (time.perf_counter() - t0) * 1e3
        t0 = time.perf_counter()
        vb_off, vn, vq, vd = vectorised_numpy(off, index.astype(np.int64), host_value, host_ids.astype(np.int64), host_toff, shape,
                                              host_it[:K, 11:14], host_rt[:K, 12:15], host_rt[:K, 16], length, pspec.step,
                                              pspec.max_bins)
        rec["numpy_vectorised_ms"] = (time.perf_counter() - t0) * 1e3
        rec["vectorised_same_bins"] = bool(np.array_equal(vb_off, wave[0]) and np.array_equal(vn, wave[1][:B, 0]) and
                                           np.array_equal(vq, wave[1][:B, 1]) and np.array_equal(vd, wave[1][:B, 2:5]))
        if M <= args.numpy_max:
            t0 = time.perf_counter()
            want = cluster_profile_numpy(off, index, host_value, host_ids, host_toff, shape, pspec)
            rec["statement_ms"] = (time.perf_counter() - t0) * 1e3
            same = np.array_equal(wave[0], want["bin_offsets"])
            for tab, names, src in ((wave[1], PROFILE_BIN_INT, "bins"), (wave[2], PROFILE_BIN_REAL, "bins"),
                                    (wave[3], PROFILE_ROW_INT, "rows"), (wave[4], PROFILE_ROW_REAL, "rows")):
                rows = B if src == "bins" else K
                same = same and all(np.array_equal(tab[:rows, c].view(np.int64), want[src][k].view(np.int64))
                                    for c, k in enumerate(names))
            rec["same_bits"] = bool(same)
        out[name] = rec
        print("%-20s %d x %d^3, %d entries, %d clusters, %d bins: profile %.3f ms (one atomic set per entry: %.3f ms, same bits: %s), "
              "list copy %.3f ms, cluster_features %.3f ms | host: D2H %.3f ms, vectorised numpy %.0f ms (same bins: %s), statement %s%s"
              % (name, n, shape[0], M, K, B, rec["profile_wave_ms"], rec["profile_plain_ms"], rec["routes_same_bits"], rec["copy_ms"],
                 rec["features_ms"], rec["d2h_ms"], rec["numpy_vectorised_ms"], rec["vectorised_same_bins"],
                 "%.0f ms" % rec["statement_ms"] if "statement_ms" in rec else "not run (> %d entries)" % args.numpy_max,
                 "; device == statement: %s" % rec["same_bits"] if "same_bits" in rec else ""), flush=True)
        del scratch, ints, tcls, toff, copies, fscratch, itab, rtab, pscratch, boff, bi, br, ri, rr
    out["repeats"], out["inner"] = args.repeats, args.inner
    print(json.dumps(out))


if __name__ == "__main__":
    main()
