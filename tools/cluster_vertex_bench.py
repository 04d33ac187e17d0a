#!/usr/bin/env python
"""What the vertex candidates cost on the device (cluster_vertex.hip, ssnet_base.cluster_vertices / set_cluster_vertices), against
what they replace and against the contact graph at the same reach.

Lists: --batch lartpc_sparse events at --size^3 (default 4 x 192^3), --big-batch lartpc_sparse events at --big-size^3 (default
2 x 256^3, the size of a stitched tiled event) and --dense-batch dense_uniform events at --dense-size^3 (default 4 x 96^3: every
voxel listed, the worst case), each at radius 1, 2 and 3 with min_size 3.  The clusters are those of the TRUE classes under the
default spec (ursn_cluster_voxels): tracks and showers as a consumer sees them, whatever a network with random weights would say.

Per list and radius, between device events: ursn_cluster_vertices in the wave form (one wave64 per end point, one lane per row of
the neighbourhood; the default) and in the plain form (URSN_CLVTX_WAVE=0: one thread per end point, one insertion per pair); a
device-to-device copy of the lists it reads (index, ids, the two object tables: the floor of anything that reads them once);
ursn_cluster_features alone; ursn_cluster_graph at gap = radius without its edge list, the yardstick: it searches from every entry
where the vertex call searches from at most 2 K end points.  The host alternative, once: the D2H copy of the ids, the index and the
two object tables, then vectorised numpy -- one sorted-key join (np.searchsorted on event * volume + index) per neighbour offset
for the links and for the incidences, components by minimum-label propagation, np.unique on the (vertex, row) keys.  Medians over
--repeats windows of --inner calls, ms per call.  Lists up to --numpy-max entries are compared with clusters.cluster_vertices_numpy
bit for bit.

Prints a table and one JSON line.

    python tools/cluster_vertex_bench.py [--size 192] [--batch 4] [--big-size 256] [--big-batch 2] [--dense-size 96] [--dense-batch 4]
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


def vectorised_numpy(off, index, ids, toff, itab, shape, radius, min_size):
    """The host competitor.  Returns (vertices, distinct incidences)."""
    shape = np.asarray(shape, np.int64)
    vol = int(shape.prod())
    ev = np.searchsorted(off, np.arange(index.size), side="right") - 1
    keep = np.flatnonzero(ids >= 0)
    key = ev[keep] * vol + index[keep]                      # ascending: events back to back, indices sorted inside
    row = toff[ev[keep]] + ids[keep]
    K = int(toff[-1])
    ok = itab[:K, 0] >= min_size
    lo, hi = itab[:K, 24][ok], itab[:K, 25][ok]
    rows = np.flatnonzero(ok)
    pos = np.concatenate([lo, hi[hi != lo]])                # the end points: position, key 2 r + side
    ekey = np.concatenate([2 * rows, 2 * rows[hi != lo] + 1])
    order = np.argsort(pos)
    pos, ekey = pos[order], ekey[order]
    x = np.stack(np.unravel_index(index[pos], shape), 1)
    pkey = ev[pos] * vol + index[pos]                       # ascending with pos
    label = np.arange(2 * K)
    r = np.arange(-radius, radius + 1)
    offsets = np.stack(np.meshgrid(r, r, r, indexing="ij"), -1).reshape(-1, 3)
    la, lb, near = [], [], []
    for d in offsets:
        y = x + d
        inside = ((y >= 0) & (y < shape)).all(1)
        want = pkey[inside] + int((d[0] * shape[1] + d[1]) * shape[2] + d[2])
        at = np.searchsorted(pkey, want)                    # end point against end point: the links
        hit = (at < pkey.size) & (pkey[np.minimum(at, pkey.size - 1)] == want)
        a, b = ekey[inside][hit], ekey[at[hit]]
        diff = (a >> 1) != (b >> 1)
        la.append(a[diff]), lb.append(b[diff])
        at = np.searchsorted(key, want)                     # end point against every entry with an id: the incidences
        hit = (at < key.size) & (key[np.minimum(at, key.size - 1)] == want)
        near.append((ekey[inside][hit], row[at[hit]]))
    ea, eb = np.concatenate(la), np.concatenate(lb)
    while True:                                             # minimum-label propagation over the links
        low = np.minimum(label[ea], label[eb])
        new = label.copy()
        np.minimum.at(new, ea, low)
        np.minimum.at(new, eb, low)
        new = new[new]
        if np.array_equal(new, label):
            break
        label = new
    vertices = np.unique(label[ekey]).size
    cells = np.unique(np.concatenate([label[k] * max(K, 1) + rw for k, rw in near]) if near else np.zeros(0, np.int64)).size
    return vertices, cells


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", type=int, default=192)
    ap.add_argument("--batch", type=int, default=4)
    ap.add_argument("--big-size", type=int, default=256)
    ap.add_argument("--big-batch", type=int, default=2)
    ap.add_argument("--dense-size", type=int, default=96)
    ap.add_argument("--dense-batch", type=int, default=4)
    ap.add_argument("--numpy-max", type=int, default=100000)
    ap.add_argument("--min-size", type=int, default=3)
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--inner", type=int, default=5)
    args = ap.parse_args()
    import torch
    from uresnet_amd import _lib
    from uresnet_amd import synthetic_io as sio
    from uresnet_amd.clusters import VERTEX_INT, VERTEX_REAL, ClusterSpec, ClusterVertexSpec, cluster_vertices_numpy
    from uresnet_amd.ssnet import VoxelBatch
    assert torch.cuda.is_available(), "cluster_vertex_bench: no HIP device visible"
    lib = _lib.load()
    spec = ClusterSpec()
    FI, FR = _lib.CLFEAT_I, _lib.CLFEAT_R
    VI, VR, IN, EV = _lib.CLVTX_VI, _lib.CLVTX_VR, _lib.CLVTX_IN, _lib.CLVTX_EV

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
    for name, shape, vb in lists:
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
        _lib.check(lib.ursn_cluster_voxels(ctypes.byref(d), ctypes.byref(o), ptr(scratch), need, stream))
        torch.cuda.synchronize()
        assert int(ints[3 * M + n].item()) == 0, "a bounded device loop ran out"
        K = int(toff[-1].item())
        # the object records
        fneed = int(lib.ursn_cluster_features_scratch_bytes(n, M, K))
        fscratch = torch.empty(fneed // 8, dtype=torch.int64, device="cuda")
        itab = torch.empty((max(K, 1), FI), dtype=torch.int64, device="cuda")
        rtab = torch.empty((max(K, 1), FR), dtype=torch.float64, device="cuda")
        fstatus = torch.empty(1, dtype=torch.int32, device="cuda")
        fd = _lib.ursn_cluster_feat_desc()
        fd.ndim, fd.n, fd.m_total = 3, n, M
        for i, s in enumerate(shape):
            fd.spatial[i] = s
        fd.offsets, fd.index, fd.value, fd.cluster, fd.table_offsets = d_off.data_ptr(), d_index.data_ptr(), d_value.data_ptr(), \
            ints.data_ptr(), toff.data_ptr()
        fo = _lib.ursn_cluster_feat_out()
        fo.itab, fo.rtab, fo.cap, fo.status = itab.data_ptr(), rtab.data_ptr(), K, fstatus.data_ptr()
        features = lambda: _lib.check(lib.ursn_cluster_features(ctypes.byref(fd), ctypes.byref(fo), ptr(fscratch), fneed, stream))
        features()
        torch.cuda.synchronize()
        assert int(fstatus.item()) == 0, "cluster_features: status %d" % int(fstatus.item())
        features_ms = timed(features)
        copies = [torch.empty_like(d_index), torch.empty(M, dtype=torch.int32, device="cuda"), torch.empty_like(itab), torch.empty_like(rtab)]

        def copy():
            copies[0].copy_(d_index)
            copies[1].copy_(ints[:M])
            copies[2].copy_(itab)
            copies[3].copy_(rtab)
        copy()
        copy_ms = timed(copy)
        t0 = time.perf_counter()
        host_ids, host_index = ints[:M].cpu().numpy().astype(np.int64), d_index.cpu().numpy().astype(np.int64)
        host_toff, host_itab, host_rtab = toff.cpu().numpy(), itab.cpu().numpy(), rtab.cpu().numpy()
        d2h_ms = (time.perf_counter() - t0) * 1e3
        for radius in (1, 2, 3):
            inc_cap = 4 * K + 1024
            while True:                                     # what ssnet_base.cluster_vertices does: double while the table overflows
                vneed = int(lib.ursn_cluster_vertices_scratch_bytes(n, M, inc_cap))
                vscratch = torch.empty(vneed // 8, dtype=torch.int64, device="cuda")
                tabs = {"vertex_offsets": torch.empty(n + 1, dtype=torch.int64, device="cuda"),
                        "vtx_itab": torch.empty((max(2 * K, 1), VI), dtype=torch.int64, device="cuda"),
                        "vtx_rtab": torch.empty((max(2 * K, 1), VR), dtype=torch.float64, device="cuda"),
                        "inc_offsets": torch.empty(2 * K + 1, dtype=torch.int64, device="cuda"),
                        "incidence": torch.empty((inc_cap, IN), dtype=torch.int64, device="cuda"),
                        "row_vertex": torch.empty((max(K, 1), 2), dtype=torch.int32, device="cuda"),
                        "event": torch.empty((n, EV), dtype=torch.int64, device="cuda"),
                        "status": torch.empty(1, dtype=torch.int32, device="cuda")}
                vd = _lib.ursn_cluster_vtx_desc()
                vd.ndim, vd.n, vd.radius, vd.m_total, vd.inc_cap = 3, n, radius, M, inc_cap
                for i, s in enumerate(shape):
                    vd.spatial[i] = s
                vd.offsets, vd.index, vd.cluster, vd.table_offsets = d_off.data_ptr(), d_index.data_ptr(), ints.data_ptr(), toff.data_ptr()
                vd.itab, vd.rtab, vd.feat_cap, vd.cls = itab.data_ptr(), rtab.data_ptr(), K, tcls.data_ptr()
                vd.min_size, vd.class_mask = args.min_size, 0
                vo = _lib.ursn_cluster_vtx_out()
                for key, t in tabs.items():
                    setattr(vo, key, t.data_ptr())
                vo.cap_vertices, vo.inc_out_cap, vo.cap_rows = 2 * K, inc_cap, K
                vertices = lambda: _lib.check(lib.ursn_cluster_vertices(ctypes.byref(vd), ctypes.byref(vo), ptr(vscratch), vneed, stream))
                vertices()
                torch.cuda.synchronize()
                code = int(tabs["status"].item())
                if code != _lib.CLVTX_INC_OVERFLOW:
                    break
                inc_cap *= 2
            assert code == 0, "cluster_vertices: status %d" % code

            def fetch():
                nv = int(tabs["vertex_offsets"][n].item())
                ni = int(tabs["inc_offsets"][nv].item())
                cut = {"vtx_itab": nv, "vtx_rtab": nv, "inc_offsets": nv + 1, "incidence": ni}
                return {k: (t[:cut[k]] if k in cut else t).cpu().numpy().copy() for k, t in tabs.items()}
            wave = fetch()
            rec = dict(shape=list(shape), events=n, radius=radius, min_size=args.min_size, list_entries=M, rows=K,
                       vertices=int(wave["vtx_itab"].shape[0]), incidences=int(wave["incidence"].shape[0]),
                       junctions=int(wave["event"][:, 1].sum()), most_ends=int(wave["vtx_itab"][:, 0].max()) if wave["vtx_itab"].size else 0,
                       inc_cap=inc_cap, scratch_bytes=vneed, vertices_wave_ms=timed(vertices), features_ms=features_ms, copy_ms=copy_ms,
                       d2h_ms=d2h_ms)
            os.environ["URSN_CLVTX_WAVE"] = "0"
            try:
                vertices()
                torch.cuda.synchronize()
                plain = fetch()
                rec["routes_same_bits"] = bool(all(np.array_equal(plain[k].view(np.uint8), wave[k].view(np.uint8)) for k in wave))
                rec["vertices_plain_ms"] = timed(vertices)
            finally:
                os.environ.pop("URSN_CLVTX_WAVE", None)
            # the yardstick: the contact graph at the same reach, without its edge list
            edge_cap = inc_cap
            while True:                                     # a graph that overflowed returns early: its time would not count
                gneed = int(lib.ursn_cluster_graph_scratch_bytes(n, M, K, K, edge_cap))
                gscratch = torch.empty(gneed // 8, dtype=torch.int64, device="cuda")
                gt = {"rows": torch.empty((max(K, 1), _lib.CLGRAPH_I), dtype=torch.int64, device="cuda"),
                      "groups": torch.empty((max(K, 1), _lib.CLGRAPH_G), dtype=torch.int64, device="cuda"),
                      "group_offsets": torch.empty(n + 1, dtype=torch.int64, device="cuda"),
                      "event": torch.empty((n, _lib.CLGRAPH_EV), dtype=torch.int64, device="cuda"),
                      "group": torch.empty(max(M, 1), dtype=torch.int32, device="cuda"),
                      "status": torch.empty(1, dtype=torch.int32, device="cuda")}
                gd = _lib.ursn_cluster_graph_desc()
                gd.ndim, gd.n, gd.gap, gd.m_total, gd.edge_cap = 3, n, radius, M, edge_cap
                for i, s in enumerate(shape):
                    gd.spatial[i] = s
                gd.offsets, gd.index, gd.cluster, gd.table_offsets = d_off.data_ptr(), d_index.data_ptr(), ints.data_ptr(), toff.data_ptr()
                gd.value, gd.cls = d_value.data_ptr(), tcls.data_ptr()
                go = _lib.ursn_cluster_graph_out()
                for key, t in gt.items():
                    setattr(go, key, t.data_ptr())
                go.cap_rows, go.cap_groups, go.edge_out_cap = K, K, 0
                graph = lambda: _lib.check(lib.ursn_cluster_graph(ctypes.byref(gd), ctypes.byref(go), ptr(gscratch), gneed, stream))
                graph()
                torch.cuda.synchronize()
                rec["graph_status"] = int(gt["status"].item())
                if rec["graph_status"] != _lib.CLGRAPH_EDGE_OVERFLOW:
                    break
                edge_cap *= 2
            assert rec["graph_status"] == 0, "cluster_graph: status %d" % rec["graph_status"]
            rec["graph_edge_cap"] = edge_cap
            rec["graph_ms"] = timed(graph)
            t0 = time.perf_counter()
            nv, ni = vectorised_numpy(off, host_index, host_ids, host_toff, host_itab, shape, radius, args.min_size)
            rec["numpy_vectorised_ms"] = (time.perf_counter() - t0) * 1e3
            assert (nv, ni) == (rec["vertices"], rec["incidences"]), "the host route and the device disagree: %r" % ((nv, ni),)
            if M <= args.numpy_max:
                t0 = time.perf_counter()
                want = cluster_vertices_numpy(off, host_index, value, host_ids, host_toff, shape, ClusterVertexSpec(radius, args.min_size),
                                              tcls[:K].cpu().numpy())
                rec["statement_ms"] = (time.perf_counter() - t0) * 1e3
                same = np.array_equal(wave["vertex_offsets"], want["vertex_offsets"]) and \
                    np.array_equal(wave["inc_offsets"], want["inc_offsets"]) and np.array_equal(wave["incidence"], want["incidence"]) and \
                    np.array_equal(wave["row_vertex"], want["row_vertex"]) and np.array_equal(wave["event"], want["events"])
                for c, col in enumerate(VERTEX_INT):
                    same = same and np.array_equal(wave["vtx_itab"][:, c], want["vertices"][col])
                for c, col in enumerate(VERTEX_REAL):
                    same = same and np.array_equal(wave["vtx_rtab"][:, c].view(np.uint64), want["vertices"][col].view(np.uint64))
                rec["same_bits"] = bool(same)
            out["%s radius %d" % (name, radius)] = rec
            print("%-20s radius %d: %d x %d^3, %d entries, %d rows, %d vertices (%d junctions, most ends %d), %d incidences: vertices "
                  "%.3f ms (plain form %.3f ms, same bits: %s), graph at this gap %.3f ms, features %.3f ms, list copy %.3f ms | host: D2H "
                  "%.3f ms, vectorised numpy %.1f ms, statement %s%s"
                  % (name, radius, n, shape[0], M, K, rec["vertices"], rec["junctions"], rec["most_ends"], rec["incidences"],
                     rec["vertices_wave_ms"], rec["vertices_plain_ms"], rec["routes_same_bits"], rec["graph_ms"], features_ms, copy_ms,
                     d2h_ms, rec["numpy_vectorised_ms"], "%.0f ms" % rec["statement_ms"] if "statement_ms" in rec else "not run",
                     "; device == statement: %s" % rec["same_bits"] if "same_bits" in rec else ""), flush=True)
            del vscratch, gscratch, tabs, gt
            torch.cuda.empty_cache()
        del scratch, fscratch, copies, ints, toff, tcls, itab, rtab
        torch.cuda.empty_cache()
    out["repeats"], out["inner"] = args.repeats, args.inner
    print(json.dumps(out))


if __name__ == "__main__":
    main()
