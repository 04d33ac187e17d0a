#!/usr/bin/env python
"""What the cluster split costs on the device (cluster_split.hip, ssnet_base.cluster_split / set_cluster_split), against the passes
it follows and against doing it on the host.

Lists: --batch lartpc_sparse events at --size^3 (default 4 x 192^3), --big-batch lartpc_sparse events at --big-size^3 (default
2 x 256^3, the size of a stitched tiled event) and --dense-batch dense_uniform events at --dense-size^3 (default 4 x 96^3: every
voxel listed, the worst case), each at radius 1, 2 and 3 with kink_cos -0.7, min_size 8 and grow 2 radius.  The clusters are those
of the TRUE classes under the default spec (ursn_cluster_voxels).

Per list and radius, between device events: ursn_cluster_split in the plain form (one thread per entry of an eligible row; the
default) and in the wave form (URSN_CLSPLIT_WAVE=1: one wave64 per entry, one lane per list row of its ball), with the piece and
junction tables at their true sizes.  Per list: ursn_cluster_voxels alone, and a device-to-device copy of the lists the call reads
(index and ids: the floor of anything that reads them once).  The host alternative: the D2H copy of the index and the ids, then
clusters.cluster_split_numpy, for lists up to --numpy-max entries (it is the statement, not a tuned competitor; its time says what
a per-voxel Python loop costs) -- and the device is compared with it bit for bit.  Medians over --repeats windows of --inner calls,
ms per call.

Prints a table and one JSON line.

    python tools/cluster_split_bench.py [--size 192] [--batch 4] [--big-size 256] [--big-batch 2] [--dense-size 96] [--dense-batch 4]
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
    ap.add_argument("--big-size", type=int, default=256)
    ap.add_argument("--big-batch", type=int, default=2)
    ap.add_argument("--dense-size", type=int, default=96)
    ap.add_argument("--dense-batch", type=int, default=4)
    ap.add_argument("--numpy-max", type=int, default=60000)
    ap.add_argument("--min-size", type=int, default=8)
    ap.add_argument("--kink-cos", type=float, default=-0.7)
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--inner", type=int, default=5)
    args = ap.parse_args()
    import torch
    from uresnet_amd import _lib
    from uresnet_amd import synthetic_io as sio
    from uresnet_amd.clusters import (SPLIT_JUNCTION_INT, SPLIT_JUNCTION_REAL, SPLIT_PIECE, ClusterSpec, ClusterSplitSpec,
                                      cluster_split_numpy)
    assert torch.cuda.is_available(), "cluster_split_bench: no HIP device visible"
    lib = _lib.load()
    spec = ClusterSpec()

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
        parts = []
        for e in range(n):
            vb = sio.dense_to_voxels(*gen(list(shape) + [1], 3, e))
            parts.append((np.asarray(vb.index, np.int64), np.asarray(vb.label)))
        off = np.concatenate([[0], np.cumsum([p[0].size for p in parts])]).astype(np.int64)
        return off, np.concatenate([p[0] for p in parts]).astype(np.int32), np.concatenate([p[1] for p in parts]).astype(np.uint8)

    lists = []
    if args.batch:
        lists.append(("lartpc_sparse", (args.size,) * 3, events(sio.lartpc_sparse, (args.size,) * 3, args.batch)))
    if args.big_batch:
        lists.append(("lartpc_sparse big", (args.big_size,) * 3, events(sio.lartpc_sparse, (args.big_size,) * 3, args.big_batch)))
    if args.dense_batch:
        lists.append(("dense_uniform", (args.dense_size,) * 3, events(sio.dense_uniform, (args.dense_size,) * 3, args.dense_batch)))
    out = {}
    stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    ptr = lambda t: ctypes.c_void_p(t.data_ptr())
    new = lambda shp, dt: torch.empty(shp, dtype=dt, device="cuda")
    for name, shape, (off, index, label) in lists:
        n, M = off.size - 1, int(off[-1])
        d_off, d_index, d_cls = (torch.from_numpy(a).cuda() for a in (off, index, label))
        need = int(lib.ursn_cluster_scratch_bytes(n, M))
        scratch = new(need // 8, torch.int64)
        ints, tcls, toff = new(3 * M + n + 1, torch.int32), new(M, torch.uint8), new(n + 1, torch.int64)
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
        cluster = lambda: _lib.check(lib.ursn_cluster_voxels(ctypes.byref(d), ctypes.byref(o), ptr(scratch), need, stream))
        cluster()
        torch.cuda.synchronize()
        assert int(ints[3 * M + n].item()) == 0, "a bounded device loop ran out"
        K = int(toff[-1].item())
        cluster_ms = timed(cluster)
        copies = [torch.empty_like(d_index), new(M, torch.int32)]

        def copy():
            copies[0].copy_(d_index)
            copies[1].copy_(ints[:M])
        copy()
        copy_ms = timed(copy)
        t0 = time.perf_counter()
        host_index, host_ids = d_index.cpu().numpy().astype(np.int64), ints[:M].cpu().numpy().astype(np.int64)
        d2h_ms = (time.perf_counter() - t0) * 1e3
        host_toff, host_size, host_tcls = toff.cpu().numpy(), ints[2 * M:2 * M + K].cpu().numpy(), tcls[:max(K, 1)].cpu().numpy()
        rows_of = (host_ids + np.repeat(host_toff[:-1], np.diff(off)))[host_ids >= 0]
        evaluated = int((host_size[rows_of] >= args.min_size).sum())
        sneed = int(lib.ursn_cluster_split_scratch_bytes(n, M))
        sscratch = new(sneed // 8, torch.int64)
        fixed = {"split": new(max(M, 1), torch.int32), "mark": new(max(M, 1), torch.uint8), "piece_offsets": new(n + 1, torch.int64),
                 "junction_offsets": new(n + 1, torch.int64), "rows": new((max(K, 1), _lib.CLSPLIT_ROW), torch.int32),
                 "event": new((n, _lib.CLSPLIT_EV), torch.int64), "status": new(1, torch.int32)}
        for radius in (1, 2, 3):
            sd = _lib.ursn_cluster_split_desc()
            sd.ndim, sd.n, sd.radius, sd.m_total = 3, n, radius, M
            for i, s in enumerate(shape):
                sd.spatial[i] = s
            sd.offsets, sd.index, sd.cluster, sd.table_offsets = d_off.data_ptr(), d_index.data_ptr(), ints.data_ptr(), toff.data_ptr()
            sd.size, sd.cls = ints.data_ptr() + 8 * M, tcls.data_ptr()
            sd.kink_cos, sd.min_size, sd.class_mask, sd.grow = args.kink_cos, args.min_size, 0, 2 * radius
            so = _lib.ursn_cluster_split_out()
            for key, t in fixed.items():
                setattr(so, key, t.data_ptr())
            so.cap_rows = K
            split = lambda: _lib.check(lib.ursn_cluster_split(ctypes.byref(sd), ctypes.byref(so), ptr(sscratch), sneed, stream))
            split()                                             # no piece or junction table yet: the offsets hold the true counts
            torch.cuda.synchronize()
            code = int(fixed["status"].item())
            assert code == 0, "cluster_split: status %d" % code
            P, J = int(fixed["piece_offsets"][n].item()), int(fixed["junction_offsets"][n].item())
            tabs = dict(fixed, first=new(max(P, 1), torch.int32), size=new(max(P, 1), torch.int32), cls=new(max(P, 1), torch.uint8),
                        piece_itab=new((max(P, 1), _lib.CLSPLIT_PI), torch.int64),
                        junction_itab=new((max(J, 1), _lib.CLSPLIT_JI), torch.int64),
                        junction_rtab=new((max(J, 1), _lib.CLSPLIT_JR), torch.float64))
            for key, t in tabs.items():
                setattr(so, key, t.data_ptr())
            so.cap_pieces, so.cap_junctions = P, J
            split()
            torch.cuda.synchronize()

            def fetch():
                cut = {"first": P, "size": P, "cls": P, "piece_itab": P, "junction_itab": J, "junction_rtab": J, "rows": K, "split": M,
                       "mark": M}
                return {k: (t[:cut[k]] if k in cut else t).cpu().numpy().copy() for k, t in tabs.items()}
            wave = fetch()                                      # named for the comparisons below: the default form's tables
            mark = wave["mark"]
            rec = dict(shape=list(shape), events=n, radius=radius, kink_cos=args.kink_cos, min_size=args.min_size, list_entries=M, rows=K,
                       evaluated=evaluated,
                       pieces=P, junctions=J, cut=int((mark & 16 > 0).sum()), kinks=int((mark & 32 > 0).sum()),
                       attached=int((mark & 64 > 0).sum()), scratch_bytes=sneed, split_plain_ms=timed(split), cluster_voxels_ms=cluster_ms,
                       copy_ms=copy_ms, d2h_ms=d2h_ms)
            os.environ["URSN_CLSPLIT_WAVE"] = "1"
            try:
                split()
                torch.cuda.synchronize()
                plain = fetch()
                rec["routes_same_bits"] = bool(all(np.array_equal(plain[k].view(np.uint8), wave[k].view(np.uint8)) for k in wave))
                rec["split_wave_ms"] = timed(split)
            finally:
                os.environ.pop("URSN_CLSPLIT_WAVE", None)
            if M <= args.numpy_max:
                t0 = time.perf_counter()
                want = cluster_split_numpy(off, host_index, host_ids, host_toff, host_size, shape,
                                           ClusterSplitSpec(radius, args.kink_cos, args.min_size, None, 2 * radius), host_tcls[:K])
                rec["statement_ms"] = (time.perf_counter() - t0) * 1e3
                same = all(np.array_equal(wave[k], want[w]) for k, w in (("piece_offsets", "piece_offsets"), ("split", "split"),
                                                                           ("junction_offsets", "junction_offsets"), ("mark", "mark"),
                                                                           ("rows", "rows"), ("event", "events")))
                same = same and all(np.array_equal(wave[k], want["table"][k]) for k in ("first", "size", "cls"))
                for c, col in enumerate(SPLIT_PIECE):
                    same = same and np.array_equal(wave["piece_itab"][:, c], want["pieces"][col])
                for c, col in enumerate(SPLIT_JUNCTION_INT):
                    same = same and np.array_equal(wave["junction_itab"][:, c], want["junctions"][col])
                for c, col in enumerate(SPLIT_JUNCTION_REAL):
                    same = same and np.array_equal(wave["junction_rtab"][:, c].view(np.uint64), want["junctions"][col].view(np.uint64))
                rec["same_bits"] = bool(same)
            out["%s radius %d" % (name, radius)] = rec
            print("%-18s radius %d: %d x %d^3, %d entries (%d evaluated), %d rows, %d cut (%d kinks, %d attached), %d junctions, %d pieces: "
                  "split %.3f ms (wave form %.3f ms, same bits: %s), cluster_voxels %.3f ms, list copy %.3f ms | host: D2H %.3f ms, "
                  "statement %s%s"
                  % (name, radius, n, shape[0], M, rec["evaluated"], K, rec["cut"], rec["kinks"], rec["attached"], J, P, rec["split_plain_ms"],
                     rec["split_wave_ms"], rec["routes_same_bits"], cluster_ms, copy_ms, d2h_ms,
                     "%.0f ms" % rec["statement_ms"] if "statement_ms" in rec else "not run",
                     "; device == statement: %s" % rec["same_bits"] if "same_bits" in rec else ""), flush=True)
            del tabs
        del scratch, sscratch, copies, ints, toff, tcls, fixed
        torch.cuda.empty_cache()
    out["repeats"], out["inner"] = args.repeats, args.inner
    print(json.dumps(out))


if __name__ == "__main__":
    main()
