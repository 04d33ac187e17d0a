#!/usr/bin/env python
"""What matching predicted clusters to true clusters on the device (cluster_match.hip, ssnet_base.match_clusters /
set_cluster_matching) costs, against what it replaces.

Lists: --batch lartpc_sparse events at --size^3 (default 4 x 192^3) and --dense-batch dense_uniform events at --dense-size^3
(default 4 x 96^3: every voxel listed, the worst case).  Side A clusters the argmax class of a network with random weights
(inference_voxel_scores), side B the true labels, both with ursn_cluster_voxels under the default spec.

Per list, between device events: ursn_cluster_match with the wave and workgroup combining (the default) and with one table insertion
per entry (URSN_CLMATCH_WAVE=0), both with the cell list; a device-to-device copy of the lists it reads (two id arrays and the
values: the floor of anything that reads them once); ursn_cluster_voxels alone.  The host alternative, once: the D2H copy of the two
id arrays, then vectorised numpy (np.unique on pair keys, np.maximum.at for the best partner, bincounts, the Rand index).  Medians
over --repeats windows of --inner calls, ms per call.  Lists up to --numpy-max entries are compared with clusters.cluster_match_numpy
bit for bit.

Prints a table and one JSON line.

    python tools/cluster_match_bench.py [--size 192] [--batch 4] [--dense-size 96] [--dense-batch 4]
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


def vectorised_numpy(off, a, toff_a, b, toff_b):
    """The host competitor: contingency table by np.unique on pair keys, row maxima by np.maximum.at, purities, efficiencies and the
    adjusted Rand index per batch (integer sums in Python integers)."""
    ev = np.searchsorted(off, np.arange(a.size), side="right") - 1
    ra, rb = np.where(a >= 0, a + toff_a[ev], -1), np.where(b >= 0, b + toff_b[ev], -1)
    KA, KB = int(toff_a[-1]), int(toff_b[-1])
    both = (ra >= 0) & (rb >= 0)
    keys, counts = np.unique(ra[both] * max(KB, 1) + rb[both], return_counts=True)
    ca, cb = keys // max(KB, 1), keys % max(KB, 1)
    na, nb = np.bincount(ra[ra >= 0], minlength=KA), np.bincount(rb[rb >= 0], minlength=KB)
    best_a, best_b = np.zeros(KA, np.int64), np.zeros(KB, np.int64)
    np.maximum.at(best_a, ca, (counts << 32) | (0xFFFFFFFF - cb))
    np.maximum.at(best_b, cb, (counts << 32) | (0xFFFFFFFF - ca))
    purity = (best_a >> 32) / np.maximum(na, 1)
    efficiency = (best_b >> 32) / np.maximum(nb, 1)
    pairs2 = lambda v: int((v.astype(object) * (v.astype(object) - 1) // 2).sum())
    N = int(both.sum())
    S, SA, SB, P = pairs2(counts), pairs2(np.bincount(ca, weights=counts, minlength=KA).astype(np.int64)), \
        pairs2(np.bincount(cb, weights=counts, minlength=KB).astype(np.int64)), N * (N - 1) // 2
    E = SA * SB / P if P else 0.0
    den = (SA + SB) / 2 - E
    return purity, efficiency, (S - E) / den if P and den else 1.0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", type=int, default=192)
    ap.add_argument("--batch", type=int, default=4)
    ap.add_argument("--dense-size", type=int, default=96)
    ap.add_argument("--dense-batch", type=int, default=4)
    ap.add_argument("--numpy-max", type=int, default=200000)
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--inner", type=int, default=5)
    args = ap.parse_args()
    import torch
    from uresnet_amd import _lib, uresnet
    from uresnet_amd import synthetic_io as sio
    from uresnet_amd.clusters import ClusterSpec, cluster_match_numpy
    from uresnet_amd.ssnet import VoxelBatch
    assert torch.cuda.is_available(), "cluster_match_bench: no HIP device visible"
    lib = _lib.load()
    spec = ClusterSpec()
    I, R, EI, ER = _lib.CLMATCH_I, _lib.CLMATCH_R, _lib.CLMATCH_EI, _lib.CLMATCH_ER

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
             ("dense_uniform", (args.dense_size,) * 3, events(sio.dense_uniform, (args.dense_size,) * 3, args.dense_batch))]
    out = {}
    stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    for name, shape, vb in cases:
        net = uresnet(dims=list(shape) + [1], num_class=3, base_num_outputs=8)
        net.construct(trainable=False, use_weight=False, seed=7)
        pred = np.concatenate(net.inference_voxel_scores(None, vb, with_labels=False, want=("pred",))["pred"])
        del net
        torch.cuda.empty_cache()
        off, index, value = vb.offsets.astype(np.int64), vb.index.astype(np.int32), vb.value.astype(np.float32)
        n, M = vb.n, int(off[-1])
        d_off, d_index, d_value = (torch.from_numpy(a).cuda() for a in (off, index, value))
        need = int(lib.ursn_cluster_scratch_bytes(n, M))
        scratch = torch.empty(need // 8, dtype=torch.int64, device="cuda")

        def side(cls):
            """ursn_cluster_voxels on one class array: (the call, ids | first | size | count | status, table offsets)."""
            d_cls = torch.from_numpy(np.ascontiguousarray(cls, dtype=np.uint8)).cuda()
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
            call = lambda: _lib.check(lib.ursn_cluster_voxels(ctypes.byref(d), ctypes.byref(o), ctypes.c_void_p(scratch.data_ptr()),
                                                              need, stream))
            call()
            torch.cuda.synchronize()
            assert int(ints[3 * M + n].item()) == 0, "a bounded device loop ran out"
            return call, ints, toff, (d, o, d_cls, tcls)

        clusters, ia, ta, keep_a = side(pred)
        _, ib, tb, keep_b = side(vb.label)
        KA, KB = int(ta[-1].item()), int(tb[-1].item())
        mneed = int(lib.ursn_cluster_match_scratch_bytes(n, M, KA, KB, M))
        mscratch = torch.empty(mneed // 8, dtype=torch.int64, device="cuda")
        tabs = {"a_int": torch.empty((max(KA, 1), I), dtype=torch.int64, device="cuda"),
                "a_real": torch.empty((max(KA, 1), R), dtype=torch.float64, device="cuda"),
                "b_int": torch.empty((max(KB, 1), I), dtype=torch.int64, device="cuda"),
                "b_real": torch.empty((max(KB, 1), R), dtype=torch.float64, device="cuda"),
                "event_int": torch.empty((n, EI), dtype=torch.int64, device="cuda"),
                "event_real": torch.empty((n, ER), dtype=torch.float64, device="cuda"),
                "pair_offsets": torch.empty(KA + 1, dtype=torch.int64, device="cuda"),
                "pair_b": torch.empty(max(M, 1), dtype=torch.int32, device="cuda"),
                "pair_n": torch.empty(max(M, 1), dtype=torch.int64, device="cuda"),
                "pair_q": torch.empty(max(M, 1), dtype=torch.int64, device="cuda"),
                "status": torch.empty(1, dtype=torch.int32, device="cuda")}
        md = _lib.ursn_cluster_match_desc()
        md.n, md.m_total, md.offsets, md.value = n, M, d_off.data_ptr(), d_value.data_ptr()
        md.cluster_a, md.table_offsets_a, md.cluster_b, md.table_offsets_b = ia.data_ptr(), ta.data_ptr(), ib.data_ptr(), tb.data_ptr()
        mo = _lib.ursn_cluster_match_out()
        for key, t in tabs.items():
            setattr(mo, key, t.data_ptr())
        mo.cap_a, mo.cap_b, mo.pair_cap = KA, KB, M
        match = lambda: _lib.check(lib.ursn_cluster_match(ctypes.byref(md), ctypes.byref(mo), ctypes.c_void_p(mscratch.data_ptr()),
                                                          mneed, stream))
        copies = [torch.empty(M, dtype=torch.int32, device="cuda"), torch.empty(M, dtype=torch.int32, device="cuda"),
                  torch.empty_like(d_value)]

        def copy():
            copies[0].copy_(ia[:M])
            copies[1].copy_(ib[:M])
            copies[2].copy_(d_value)

        def fetch():
            cells = int(tabs["pair_offsets"][KA].item())
            return {k: (t[:cells] if k in ("pair_b", "pair_n", "pair_q") else t).cpu().numpy().copy() for k, t in tabs.items()}
        match(), copy()
        torch.cuda.synchronize()
        assert int(tabs["status"].item()) == 0, "cluster_match: status %d" % int(tabs["status"].item())
        wave = fetch()
        rec = dict(shape=list(shape), events=n, list_entries=M, rows_a=KA, rows_b=KB, cells=int(wave["pair_offsets"][KA]),
                   scratch_bytes=mneed, match_combined_ms=timed(match))
        os.environ["URSN_CLMATCH_WAVE"] = "0"
        try:
            match()
            torch.cuda.synchronize()
            plain = fetch()
            rec["routes_same_bits"] = bool(all(np.array_equal(plain[k].view(np.uint8), wave[k].view(np.uint8)) for k in wave))
            rec["match_plain_ms"] = timed(match)
        finally:
            os.environ.pop("URSN_CLMATCH_WAVE", None)
        rec["copy_ms"], rec["cluster_voxels_ms"] = timed(copy), timed(clusters)
        t0 = time.perf_counter()
        host_a, host_b = ia[:M].cpu().numpy().astype(np.int64), ib[:M].cpu().numpy().astype(np.int64)
        host_ta, host_tb = ta.cpu().numpy(), tb.cpu().numpy()
        rec["d2h_ms"] = (time.perf_counter() - t0) * 1e3
        t0 = time.perf_counter()
        purity, efficiency, ari = vectorised_numpy(off, host_a, host_ta, host_b, host_tb)
        rec["numpy_vectorised_ms"] = (time.perf_counter() - t0) * 1e3
        rec["ari_first_event"] = float(wave["event_real"][0][0])
        assert np.array_equal(purity, wave["a_real"][:KA, 0]) and np.array_equal(efficiency, wave["b_real"][:KB, 0])
        if M <= args.numpy_max:
            t0 = time.perf_counter()
            want = cluster_match_numpy(off, host_a, host_ta, host_b, host_tb, value)
            rec["statement_ms"] = (time.perf_counter() - t0) * 1e3
            rec["same_bits"] = bool(all(np.array_equal(np.ascontiguousarray(wave[k][:want[k].shape[0]]).view(np.uint8),
                                                       np.ascontiguousarray(want[k]).view(np.uint8)) for k in want))
        out[name] = rec
        print("%-14s %d x %d^3, %d entries, %d x %d rows, %d cells: match %.3f ms (one insertion per entry: %.3f ms, same bits: %s), "
              "list copy %.3f ms, cluster_voxels %.3f ms | host: D2H %.3f ms, vectorised numpy %.1f ms, statement %s%s"
              % (name, n, shape[0], M, KA, KB, rec["cells"], rec["match_combined_ms"], rec["match_plain_ms"], rec["routes_same_bits"],
                 rec["copy_ms"], rec["cluster_voxels_ms"], rec["d2h_ms"], rec["numpy_vectorised_ms"],
                 "%.0f ms" % rec["statement_ms"] if "statement_ms" in rec else "not run (> %d entries)" % args.numpy_max,
                 "; device == statement: %s" % rec["same_bits"] if "same_bits" in rec else ""))
        del scratch, mscratch, tabs, copies, ia, ib, ta, tb, keep_a, keep_b
        torch.cuda.empty_cache()
    out["repeats"], out["inner"] = args.repeats, args.inner
    print(json.dumps(out))


if __name__ == "__main__":
    main()
