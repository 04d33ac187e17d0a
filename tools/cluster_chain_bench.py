#!/usr/bin/env python
"""What the cluster chains cost on the device (cluster_chain.hip, ssnet_base.cluster_chains / set_cluster_chains), against what they
replace and against the vertex candidates at their longest reach.

Lists: --batch lartpc_sparse events at --size^3 (default 4 x 192^3), the same events with slabs knocked out of every track (a voxel
survives when on axes 0 and 2 its coordinate % 12 / % 10 lies outside [5, 7) / [3, 5): joins exist), --big-batch lartpc_sparse
events at --big-size^3 (default 2 x 256^3, the size of a stitched tiled event) and --dense-batch dense_uniform events at
--dense-size^3 (default 4 x 96^3: every voxel listed, the worst case), each at max_gap 4, 8, 16 and 31 with min_cos 0.9 and
min_size 3.  The clusters are those of the TRUE classes under the default spec (ursn_cluster_voxels).

Per list and max_gap, between device events: ursn_cluster_chains in the wave form (one wave64 per end point, one lane per plane of
its slab; the default) and in the plain form (URSN_CLCHAIN_WAVE=0: one thread per end point).  Per list: ursn_cluster_vertices at
radius 3 (its own longest reach: a list walk from every end point), ursn_cluster_features alone, and a device-to-device copy of the
lists the call reads (index, ids, the two object tables: the floor of anything that reads them once).  The host alternative, once
per max_gap: the D2H copy of the index and the two object tables, then a vectorised numpy join on the end points (blocks of end
points against all of their event: the three cosines, the packed best, the mutual test).  Medians over --repeats windows of --inner
calls, ms per call.  Lists up to --numpy-max entries are compared with clusters.cluster_chains_numpy bit for bit.

Prints a table and one JSON line.

    python tools/cluster_chain_bench.py [--size 192] [--batch 4] [--big-size 256] [--big-batch 2] [--dense-size 96] [--dense-batch 4]
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


def vectorised_numpy(off, index, toff, itab, rtab, tcls, shape, max_gap, min_cos, min_size):
    """The host competitor: the joins from the object tables.  Returns their number."""
    shape = np.asarray(shape, np.int64)
    K = int(toff[-1])
    lo, hi = itab[:K, 24], itab[:K, 25]
    rows = np.flatnonzero((itab[:K, 0] >= min_size) & (lo != hi))
    key = np.concatenate([2 * rows, 2 * rows + 1])
    pos = np.concatenate([lo[rows], hi[rows]])
    u = np.concatenate([rtab[rows, 12:15], -rtab[rows, 12:15]])
    x = np.stack(np.unravel_index(index[pos], shape), 1)
    ev = np.searchsorted(toff, key >> 1, side="right") - 1
    best = np.full(2 * K, np.iinfo(np.int64).max, np.int64)
    for e in np.unique(ev):
        sel = np.flatnonzero(ev == e)
        for at in range(0, sel.size, 512):
            a = sel[at:at + 512]
            d = x[sel][None, :, :] - x[a][:, None, :]                                  # [a, b, 3] = x(b) - x(a)
            ok = (np.abs(d).max(2) <= max_gap) & ((key[a] >> 1)[:, None] != (key[sel] >> 1)[None, :]) & \
                (tcls[key[a] >> 1][:, None] == tcls[key[sel] >> 1][None, :])
            ia, ib = np.nonzero(ok)
            if not ia.size:
                continue
            ka, kb, dd = key[a][ia], key[sel][ib], d[ia, ib].astype(np.float64)
            ua, ub = u[a][ia], u[sel][ib]
            swap = ka > kb                                                             # evaluated with the lower key first
            dd = np.where(swap[:, None], -dd, dd)
            up, uq = np.where(swap[:, None], ub, ua), np.where(swap[:, None], ua, ub)
            dist2 = (dd * dd).sum(1)
            s = np.sqrt(dist2)
            c_ax = -((up[:, 0] * uq[:, 0] + up[:, 1] * uq[:, 1]) + up[:, 2] * uq[:, 2])
            c_lo = (-((up[:, 0] * dd[:, 0] + up[:, 1] * dd[:, 1]) + up[:, 2] * dd[:, 2])) / s
            c_hi = ((uq[:, 0] * dd[:, 0] + uq[:, 1] * dd[:, 1]) + uq[:, 2] * dd[:, 2]) / s
            good = (c_ax >= min_cos) & (c_lo >= min_cos) & (c_hi >= min_cos)
            np.minimum.at(best, ka[good], (dist2[good].astype(np.int64) << 32) | kb[good])
    have = np.flatnonzero(best != np.iinfo(np.int64).max)
    partner = best[have] & 0xFFFFFFFF
    mutual = (best[partner] & 0xFFFFFFFF) == have
    return int((mutual & (have < partner)).sum())


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", type=int, default=192)
    ap.add_argument("--batch", type=int, default=4)
    ap.add_argument("--big-size", type=int, default=256)
    ap.add_argument("--big-batch", type=int, default=2)
    ap.add_argument("--dense-size", type=int, default=96)
    ap.add_argument("--dense-batch", type=int, default=4)
    ap.add_argument("--numpy-max", type=int, default=100000)
    ap.add_argument("--host-max", type=int, default=40000)
    ap.add_argument("--min-size", type=int, default=3)
    ap.add_argument("--min-cos", type=float, default=0.9)
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--inner", type=int, default=5)
    args = ap.parse_args()
    import torch
    from uresnet_amd import _lib
    from uresnet_amd import synthetic_io as sio
    from uresnet_amd.clusters import CHAIN_INT, CHAIN_REAL, JOIN_INT, JOIN_REAL, ClusterChainSpec, ClusterSpec, cluster_chains_numpy
    assert torch.cuda.is_available(), "cluster_chain_bench: no HIP device visible"
    lib = _lib.load()
    spec = ClusterSpec()
    FI, FR = _lib.CLFEAT_I, _lib.CLFEAT_R

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

    def events(gen, shape, n, knock=False):
        """(offsets, index, value, label) of n events; with ``knock`` the slabs are taken out."""
        parts = []
        for e in range(n):
            vb = sio.dense_to_voxels(*gen(list(shape) + [1], 3, e))
            index, keep = np.asarray(vb.index, np.int64), np.ones(vb.index.size, bool)
            if knock:
                c = np.unravel_index(index, shape)
                keep = ~((c[0] % 12 >= 5) & (c[0] % 12 < 7)) & ~((c[2] % 10 >= 3) & (c[2] % 10 < 5))
            parts.append((index[keep], np.asarray(vb.value, np.float32)[keep], np.asarray(vb.label)[keep]))
        off = np.concatenate([[0], np.cumsum([p[0].size for p in parts])]).astype(np.int64)
        return off, np.concatenate([p[0] for p in parts]).astype(np.int32), np.concatenate([p[1] for p in parts]), \
            np.concatenate([p[2] for p in parts]).astype(np.uint8)

    lists = []
    if args.batch:
        lists.append(("lartpc_sparse", (args.size,) * 3, events(sio.lartpc_sparse, (args.size,) * 3, args.batch)))
        lists.append(("lartpc_sparse cut", (args.size,) * 3, events(sio.lartpc_sparse, (args.size,) * 3, args.batch, True)))
    if args.big_batch:
        lists.append(("lartpc_sparse big", (args.big_size,) * 3, events(sio.lartpc_sparse, (args.big_size,) * 3, args.big_batch)))
    if args.dense_batch:
        lists.append(("dense_uniform", (args.dense_size,) * 3, events(sio.dense_uniform, (args.dense_size,) * 3, args.dense_batch)))
    out = {}
    stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    ptr = lambda t: ctypes.c_void_p(t.data_ptr())
    new = lambda shp, dt: torch.empty(shp, dtype=dt, device="cuda")
    for name, shape, (off, index, value, label) in lists:
        n, M = off.size - 1, int(off[-1])
        d_off, d_index, d_value, d_cls = (torch.from_numpy(a).cuda() for a in (off, index, value, label))
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
        _lib.check(lib.ursn_cluster_voxels(ctypes.byref(d), ctypes.byref(o), ptr(scratch), need, stream))
        torch.cuda.synchronize()
        assert int(ints[3 * M + n].item()) == 0, "a bounded device loop ran out"
        K = int(toff[-1].item())
        fneed = int(lib.ursn_cluster_features_scratch_bytes(n, M, K))
        fscratch = new(fneed // 8, torch.int64)
        itab, rtab, fstatus = new((max(K, 1), FI), torch.int64), new((max(K, 1), FR), torch.float64), new(1, torch.int32)
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
        copies = [torch.empty_like(d_index), new(M, torch.int32), torch.empty_like(itab), torch.empty_like(rtab)]

        def copy():
            copies[0].copy_(d_index)
            copies[1].copy_(ints[:M])
            copies[2].copy_(itab)
            copies[3].copy_(rtab)
        copy()
        copy_ms = timed(copy)
        t0 = time.perf_counter()
        host_index = d_index.cpu().numpy().astype(np.int64)
        host_toff, host_itab, host_rtab, host_tcls = toff.cpu().numpy(), itab.cpu().numpy(), rtab.cpu().numpy(), tcls[:max(K, 1)].cpu().numpy()
        d2h_ms = (time.perf_counter() - t0) * 1e3
        host_ids = ints[:M].cpu().numpy().astype(np.int64)
        # the vertex candidates at their longest reach
        inc_cap = 4 * K + 1024
        while True:
            vneed = int(lib.ursn_cluster_vertices_scratch_bytes(n, M, inc_cap))
            vscratch = new(vneed // 8, torch.int64)
            vt = {"vertex_offsets": new(n + 1, torch.int64), "vtx_itab": new((max(2 * K, 1), _lib.CLVTX_VI), torch.int64),
                  "vtx_rtab": new((max(2 * K, 1), _lib.CLVTX_VR), torch.float64), "inc_offsets": new(2 * K + 1, torch.int64),
                  "incidence": new((inc_cap, _lib.CLVTX_IN), torch.int64), "row_vertex": new((max(K, 1), 2), torch.int32),
                  "event": new((n, _lib.CLVTX_EV), torch.int64), "status": new(1, torch.int32)}
            vd = _lib.ursn_cluster_vtx_desc()
            vd.ndim, vd.n, vd.radius, vd.m_total, vd.inc_cap = 3, n, 3, M, inc_cap
            for i, s in enumerate(shape):
                vd.spatial[i] = s
            vd.offsets, vd.index, vd.cluster, vd.table_offsets = d_off.data_ptr(), d_index.data_ptr(), ints.data_ptr(), toff.data_ptr()
            vd.itab, vd.rtab, vd.feat_cap, vd.cls = itab.data_ptr(), rtab.data_ptr(), K, tcls.data_ptr()
            vd.min_size, vd.class_mask = args.min_size, 0
            vo = _lib.ursn_cluster_vtx_out()
            for key, t in vt.items():
                setattr(vo, key, t.data_ptr())
            vo.cap_vertices, vo.inc_out_cap, vo.cap_rows = 2 * K, inc_cap, K
            vertices = lambda: _lib.check(lib.ursn_cluster_vertices(ctypes.byref(vd), ctypes.byref(vo), ptr(vscratch), vneed, stream))
            vertices()
            torch.cuda.synchronize()
            code = int(vt["status"].item())
            if code != _lib.CLVTX_INC_OVERFLOW:
                break
            inc_cap *= 2
        assert code == 0, "cluster_vertices: status %d" % code
        vertices_ms = timed(vertices)
        del vscratch, vt
        # the chains
        cneed = int(lib.ursn_cluster_chains_scratch_bytes(n, M))
        cscratch = new(cneed // 8, torch.int64)
        cap = max(K, 1)
        tabs = {"merged": new(max(M, 1), torch.int32), "chain_offsets": new(n + 1, torch.int64), "first": new(cap, torch.int32),
                "size": new(cap, torch.int32), "cls": new(cap, torch.uint8), "chain_itab": new((cap, _lib.CLCHAIN_CI), torch.int64),
                "chain_rtab": new((cap, _lib.CLCHAIN_CR), torch.float64), "join_offsets": new(n + 1, torch.int64),
                "join_itab": new((cap, _lib.CLCHAIN_JI), torch.int64), "join_rtab": new((cap, _lib.CLCHAIN_JR), torch.float64),
                "row_chain": new(cap, torch.int32), "row_join": new((cap, 2), torch.int32), "row_candidates": new((cap, 2), torch.int32),
                "event": new((n, _lib.CLCHAIN_EV), torch.int64), "status": new(1, torch.int32)}
        for max_gap in (4, 8, 16, 31):
            cd = _lib.ursn_cluster_chain_desc()
            cd.ndim, cd.n, cd.max_gap, cd.m_total = 3, n, max_gap, M
            for i, s in enumerate(shape):
                cd.spatial[i] = s
            cd.offsets, cd.index, cd.cluster, cd.table_offsets = d_off.data_ptr(), d_index.data_ptr(), ints.data_ptr(), toff.data_ptr()
            cd.itab, cd.rtab, cd.feat_cap, cd.cls = itab.data_ptr(), rtab.data_ptr(), K, tcls.data_ptr()
            cd.min_cos, cd.min_size, cd.class_mask, cd.same_class = args.min_cos, args.min_size, 0, 1
            co = _lib.ursn_cluster_chain_out()
            for key, t in tabs.items():
                setattr(co, key, t.data_ptr())
            co.cap_chains = co.cap_joins = co.cap_rows = K
            chains = lambda: _lib.check(lib.ursn_cluster_chains(ctypes.byref(cd), ctypes.byref(co), ptr(cscratch), cneed, stream))
            chains()
            torch.cuda.synchronize()
            code = int(tabs["status"].item())
            assert code == 0, "cluster_chains: status %d" % code

            def fetch():
                nc, nj = int(tabs["chain_offsets"][n].item()), int(tabs["join_offsets"][n].item())
                cut = {"first": nc, "size": nc, "cls": nc, "chain_itab": nc, "chain_rtab": nc, "join_itab": nj, "join_rtab": nj,
                       "row_chain": K, "row_join": K, "row_candidates": K, "merged": M}
                return {k: (t[:cut[k]] if k in cut else t).cpu().numpy().copy() for k, t in tabs.items()}
            wave = fetch()
            rec = dict(shape=list(shape), events=n, max_gap=max_gap, min_cos=args.min_cos, min_size=args.min_size, list_entries=M, rows=K,
                       end_points=int(2 * ((host_itab[:K, 0] >= args.min_size) & (host_itab[:K, 24] != host_itab[:K, 25])).sum()),
                       chains=int(wave["chain_itab"].shape[0]), joins=int(wave["join_itab"].shape[0]),
                       longest=int(wave["chain_itab"][:, 0].max()) if wave["chain_itab"].size else 0,
                       candidates=int(wave["row_candidates"].sum()), scratch_bytes=cneed, chains_wave_ms=timed(chains),
                       vertices_radius3_ms=vertices_ms, features_ms=features_ms, copy_ms=copy_ms, d2h_ms=d2h_ms)
            os.environ["URSN_CLCHAIN_WAVE"] = "0"
            try:
                chains()
                torch.cuda.synchronize()
                plain = fetch()
                rec["routes_same_bits"] = bool(all(np.array_equal(plain[k].view(np.uint8), wave[k].view(np.uint8)) for k in wave))
                rec["chains_plain_ms"] = timed(chains)
            finally:
                os.environ.pop("URSN_CLCHAIN_WAVE", None)
            rec["numpy_vectorised_ms"] = float("nan")
            if rec["end_points"] <= args.host_max:              # blocks of end points against all of their event: quadratic
                t0 = time.perf_counter()
                nj = vectorised_numpy(off, host_index, host_toff, host_itab, host_rtab, host_tcls, shape, max_gap, args.min_cos,
                                      args.min_size)
                rec["numpy_vectorised_ms"] = (time.perf_counter() - t0) * 1e3
                assert nj == rec["joins"], "the host route and the device disagree: %d joins, %d" % (nj, rec["joins"])
            if M <= args.numpy_max:
                t0 = time.perf_counter()
                want = cluster_chains_numpy(off, host_index, value, host_ids, host_toff, shape,
                                            ClusterChainSpec(max_gap, args.min_cos, args.min_size), host_tcls[:K])
                rec["statement_ms"] = (time.perf_counter() - t0) * 1e3
                same = all(np.array_equal(wave[k], want[w]) for k, w in (("chain_offsets", "chain_offsets"), ("join_offsets", "join_offsets"),
                                                                           ("merged", "merged"), ("row_chain", "row_chain"),
                                                                           ("row_join", "row_join"), ("row_candidates", "row_candidates"),
                                                                           ("event", "events")))
                same = same and all(np.array_equal(wave[k], want["table"][k]) for k in ("first", "size", "cls"))
                for c, col in enumerate(CHAIN_INT):
                    same = same and np.array_equal(wave["chain_itab"][:, c], want["chains"][col])
                for c, col in enumerate(CHAIN_REAL):
                    same = same and np.array_equal(wave["chain_rtab"][:, c].view(np.uint64), want["chains"][col].view(np.uint64))
                for c, col in enumerate(JOIN_INT):
                    same = same and np.array_equal(wave["join_itab"][:, c], want["joins"][col])
                for c, col in enumerate(JOIN_REAL):
                    same = same and np.array_equal(wave["join_rtab"][:, c].view(np.uint64), want["joins"][col].view(np.uint64))
                rec["same_bits"] = bool(same)
            out["%s max_gap %d" % (name, max_gap)] = rec
            print("%-18s max_gap %2d: %d x %d^3, %d entries, %d rows, %d end points, %d candidates, %d joins, %d chains (longest %d): "
                  "chains %.3f ms (plain form %.3f ms, same bits: %s), vertices at radius 3 %.3f ms, features %.3f ms, list copy %.3f ms "
                  "| host: D2H %.3f ms, vectorised numpy %.1f ms, statement %s%s"
                  % (name, max_gap, n, shape[0], M, K, rec["end_points"], rec["candidates"], rec["joins"], rec["chains"], rec["longest"],
                     rec["chains_wave_ms"], rec["chains_plain_ms"], rec["routes_same_bits"], vertices_ms, features_ms, copy_ms, d2h_ms,
                     rec["numpy_vectorised_ms"], "%.0f ms" % rec["statement_ms"] if "statement_ms" in rec else "not run",
                     "; device == statement: %s" % rec["same_bits"] if "same_bits" in rec else ""), flush=True)
        del scratch, fscratch, cscratch, copies, ints, toff, tcls, itab, rtab, tabs
        torch.cuda.empty_cache()
    out["repeats"], out["inner"] = args.repeats, args.inner
    print(json.dumps(out))


if __name__ == "__main__":
    main()
