#!/usr/bin/env python
"""What the cluster contact graph and the interaction groups cost on the device (cluster_graph.hip, ssnet_base.cluster_graph /
set_cluster_graph), against what they replace.

Lists: --batch lartpc_sparse events at --size^3 (default 4 x 192^3; at gap 1 and gap 3), --big-batch lartpc_sparse events at
--big-size^3 (default 2 x 256^3, the size of a stitched tiled event; gap 1) and --dense-batch dense_uniform events at
--dense-size^3 (default 4 x 96^3: every voxel listed, the worst case; gap 1).  The clusters are those of the TRUE classes under the
default spec (ursn_cluster_voxels): tracks and showers as a consumer sees them, whatever a network with random weights would say.

Per list, between device events: ursn_cluster_graph with the wave and workgroup combining (the default) and with one table
insertion per near pair (URSN_CLGRAPH_WAVE=0), both with the edge list; a device-to-device copy of the lists it reads (index, ids,
values: the floor of anything that reads them once); ursn_cluster_voxels alone.  The host alternative, once: the D2H copy of the ids
and the index, then vectorised numpy -- one sorted-key join (np.searchsorted on event * volume + index) per neighbour offset,
np.unique on the edge keys, components by minimum-label propagation.  (A KD-tree route needs scipy, which this tool does not
require.)  Medians over --repeats windows of --inner calls, ms per call.  Lists up to --numpy-max entries are compared with
clusters.cluster_graph_numpy bit for bit at gap 1.

Prints a table and one JSON line.

    python tools/cluster_graph_bench.py [--size 192] [--batch 4] [--big-size 256] [--big-batch 2] [--dense-size 96] [--dense-batch 4]
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


def vectorised_numpy(off, index, ids, toff, shape, gap):
    """The host competitor.  Returns (edge keys, pairs per edge, group label per row)."""
    shape = np.asarray(shape, np.int64)
    vol = int(shape.prod())
    ev = np.searchsorted(off, np.arange(index.size), side="right") - 1
    keep = np.flatnonzero(ids >= 0)
    key = ev[keep] * vol + index[keep]                      # ascending: events back to back, indices sorted inside
    row = toff[ev[keep]] + ids[keep]
    x = np.stack(np.unravel_index(index[keep], shape), 1)
    K = int(toff[-1])
    found = []
    r = np.arange(-gap, gap + 1)
    for d in np.stack(np.meshgrid(r, r, r, indexing="ij"), -1).reshape(-1, 3):
        if tuple(d) <= (0, 0, 0):                           # every unordered pair once
            continue
        y = x + d
        ok = ((y >= 0) & (y < shape)).all(1)
        want = key[ok] + int((d[0] * shape[1] + d[1]) * shape[2] + d[2])
        at = np.searchsorted(key, want)
        hit = (at < key.size) & (key[np.minimum(at, key.size - 1)] == want)
        a, b = row[ok][hit], row[at[hit]]
        diff = a != b
        found.append(np.minimum(a, b)[diff] * K + np.maximum(a, b)[diff])
    keys, pairs = np.unique(np.concatenate(found) if found else np.zeros(0, np.int64), return_counts=True)
    ea, eb = keys // max(K, 1), keys % max(K, 1)
    label = np.arange(K)
    while True:                                             # minimum-label propagation over the edges
        low = np.minimum(label[ea], label[eb])
        new = label.copy()
        np.minimum.at(new, ea, low)
        np.minimum.at(new, eb, low)
        new = new[new]
        if np.array_equal(new, label):
            return keys, pairs, label
        label = new


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", type=int, default=192)
    ap.add_argument("--batch", type=int, default=4)
    ap.add_argument("--big-size", type=int, default=256)
    ap.add_argument("--big-batch", type=int, default=2)
    ap.add_argument("--dense-size", type=int, default=96)
    ap.add_argument("--dense-batch", type=int, default=4)
    ap.add_argument("--numpy-max", type=int, default=100000)
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--inner", type=int, default=5)
    args = ap.parse_args()
    import torch
    from uresnet_amd import _lib
    from uresnet_amd import synthetic_io as sio
    from uresnet_amd.clusters import ClusterGraphSpec, ClusterSpec, cluster_graph_numpy
    from uresnet_amd.ssnet import VoxelBatch
    assert torch.cuda.is_available(), "cluster_graph_bench: no HIP device visible"
    lib = _lib.load()
    spec = ClusterSpec()
    E, I, G, EV = _lib.CLGRAPH_E, _lib.CLGRAPH_I, _lib.CLGRAPH_G, _lib.CLGRAPH_EV

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

    cases = []
    if args.batch:
        vb = events(sio.lartpc_sparse, (args.size,) * 3, args.batch)
        cases += [("lartpc_sparse gap 1", (args.size,) * 3, vb, 1), ("lartpc_sparse gap 3", (args.size,) * 3, vb, 3)]
    if args.big_batch:
        cases.append(("lartpc_sparse big gap 1", (args.big_size,) * 3, events(sio.lartpc_sparse, (args.big_size,) * 3, args.big_batch), 1))
    if args.dense_batch:
        cases.append(("dense_uniform gap 1", (args.dense_size,) * 3,
                      events(sio.dense_uniform, (args.dense_size,) * 3, args.dense_batch), 1))
    out = {}
    stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    for name, shape, vb, gap in cases:
        off, index, value = vb.offsets.astype(np.int64), vb.index.astype(np.int32), vb.value.astype(np.float32)
        n, M = vb.n, int(off[-1])
        d_off, d_index, d_value = (torch.from_numpy(a).cuda() for a in (off, index, value))
        need = int(lib.ursn_cluster_scratch_bytes(n, M))
        scratch = torch.empty(need // 8, dtype=torch.int64, device="cuda")
        d_cls = torch.from_numpy(np.ascontiguousarray(vb.label, dtype=np.uint8)).cuda()
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
        edge_cap = 4 * K + 1024
        while True:                                         # what ssnet_base.cluster_graph does: double while the table overflows
            gneed = int(lib.ursn_cluster_graph_scratch_bytes(n, M, K, K, edge_cap))
            gscratch = torch.empty(gneed // 8, dtype=torch.int64, device="cuda")
            tabs = {"rows": torch.empty((max(K, 1), I), dtype=torch.int64, device="cuda"),
                    "groups": torch.empty((max(K, 1), G), dtype=torch.int64, device="cuda"),
                    "group_offsets": torch.empty(n + 1, dtype=torch.int64, device="cuda"),
                    "event": torch.empty((n, EV), dtype=torch.int64, device="cuda"),
                    "group": torch.empty(max(M, 1), dtype=torch.int32, device="cuda"),
                    "edge_offsets": torch.empty(K + 1, dtype=torch.int64, device="cuda"),
                    "edges": torch.empty((edge_cap, E), dtype=torch.int64, device="cuda"),
                    "status": torch.empty(1, dtype=torch.int32, device="cuda")}
            gd = _lib.ursn_cluster_graph_desc()
            gd.ndim, gd.n, gd.gap, gd.m_total, gd.edge_cap = 3, n, gap, M, edge_cap
            for i, s in enumerate(shape):
                gd.spatial[i] = s
            gd.offsets, gd.index, gd.cluster, gd.table_offsets = d_off.data_ptr(), d_index.data_ptr(), ints.data_ptr(), toff.data_ptr()
            gd.value, gd.cls = d_value.data_ptr(), tcls.data_ptr()
            go = _lib.ursn_cluster_graph_out()
            for key, t in tabs.items():
                setattr(go, key, t.data_ptr())
            go.cap_rows, go.cap_groups, go.edge_out_cap = K, K, edge_cap
            graph = lambda: _lib.check(lib.ursn_cluster_graph(ctypes.byref(gd), ctypes.byref(go), ctypes.c_void_p(gscratch.data_ptr()),
                                                              gneed, stream))
            graph()
            torch.cuda.synchronize()
            code = int(tabs["status"].item())
            if code != _lib.CLGRAPH_EDGE_OVERFLOW:
                break
            edge_cap *= 2
        assert code == 0, "cluster_graph: status %d" % code
        copies = [torch.empty_like(d_index), torch.empty(M, dtype=torch.int32, device="cuda"), torch.empty_like(d_value)]

        def copy():
            copies[0].copy_(d_index)
            copies[1].copy_(ints[:M])
            copies[2].copy_(d_value)

        def fetch():
            ne, ng = int(tabs["edge_offsets"][K].item()), int(tabs["group_offsets"][n].item())
            cut = {"edges": ne, "groups": ng}
            return {k: (t[:cut[k]] if k in cut else t).cpu().numpy().copy() for k, t in tabs.items()}
        copy()
        wave = fetch()
        rec = dict(shape=list(shape), events=n, gap=gap, list_entries=M, rows=K, edges=int(wave["edges"].shape[0]),
                   groups=int(wave["groups"].shape[0]), edge_cap=edge_cap, scratch_bytes=gneed, graph_combined_ms=timed(graph))
        os.environ["URSN_CLGRAPH_WAVE"] = "0"
        try:
            graph()
            torch.cuda.synchronize()
            plain = fetch()
            rec["routes_same_bits"] = bool(all(np.array_equal(plain[k].view(np.uint8), wave[k].view(np.uint8)) for k in wave))
            rec["graph_plain_ms"] = timed(graph)
        finally:
            os.environ.pop("URSN_CLGRAPH_WAVE", None)
        rec["copy_ms"], rec["cluster_voxels_ms"] = timed(copy), timed(clusters)
        t0 = time.perf_counter()
        host_ids, host_index = ints[:M].cpu().numpy().astype(np.int64), d_index.cpu().numpy().astype(np.int64)
        host_toff = toff.cpu().numpy()
        rec["d2h_ms"] = (time.perf_counter() - t0) * 1e3
        t0 = time.perf_counter()
        keys, pairs, label = vectorised_numpy(off, host_index, host_ids, host_toff, shape, gap)
        rec["numpy_vectorised_ms"] = (time.perf_counter() - t0) * 1e3
        assert keys.size == rec["edges"] and np.array_equal(pairs, wave["edges"][:, 1]) and \
            np.unique(label).size == rec["groups"], "the host route and the device disagree"
        if M <= args.numpy_max and gap == 1:
            t0 = time.perf_counter()
            want = cluster_graph_numpy(off, host_index, host_ids, host_toff, shape, ClusterGraphSpec(gap), value,
                                       tcls[:K].cpu().numpy())
            rec["statement_ms"] = (time.perf_counter() - t0) * 1e3
            names = {"rows": "rows", "groups": "groups", "group_offsets": "group_offsets", "events": "event", "edges": "edges",
                     "edge_offsets": "edge_offsets", "group": "group"}
            rec["same_bits"] = bool(all(np.array_equal(wave[names[k]][:want[k].shape[0]], want[k]) for k in want))
        out[name] = rec
        print("%-24s %d x %d^3, %d entries, %d rows, %d edges, %d groups: graph %.3f ms (one insertion per near pair: %.3f ms, same "
              "bits: %s), list copy %.3f ms, cluster_voxels %.3f ms | host: D2H %.3f ms, vectorised numpy %.1f ms, statement %s%s"
              % (name, n, shape[0], M, K, rec["edges"], rec["groups"], rec["graph_combined_ms"], rec["graph_plain_ms"],
                 rec["routes_same_bits"], rec["copy_ms"], rec["cluster_voxels_ms"], rec["d2h_ms"], rec["numpy_vectorised_ms"],
                 "%.0f ms" % rec["statement_ms"] if "statement_ms" in rec else "not run",
                 "; device == statement: %s" % rec["same_bits"] if "same_bits" in rec else ""), flush=True)
        del scratch, gscratch, tabs, copies, ints, toff, tcls
        torch.cuda.empty_cache()
    out["repeats"], out["inner"] = args.repeats, args.inner
    print(json.dumps(out))


if __name__ == "__main__":
    main()
