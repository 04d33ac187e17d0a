#!/usr/bin/env python
"""What the cluster cones cost on the device (cluster_cone.hip, ssnet_base.cluster_cones / set_cluster_cones), against what they
replace and against the cluster chains at their longest gap.

Lists: the chain bench's three sparse ones -- --batch lartpc_sparse events at --size^3 (default 4 x 192^3), the same events with
slabs knocked out of every track, --big-batch lartpc_sparse events at --big-size^3 (default 2 x 256^3) -- its dense one
(--dense-batch dense_uniform events at --dense-size^3, default 4 x 96^3: every voxel listed, the worst case), and one "shower" list:
the lartpc_sparse events with every shower blob thinned (a voxel of class 1 survives when a fixed multiplicative hash of its index
is 0 modulo 4), so that fragments exist.  Each at reach 16, 48 and 127 with min_cos 0.8, seed_size 8 and min_size 1.  The clusters
are those of the TRUE classes under the default spec (ursn_cluster_voxels).

Per list and reach, between device events: ursn_cluster_cones in the wave form (one wave64 per child row, the lanes striding the
planes; the default) and in the plain form (URSN_CLCONE_WAVE=0: one thread per child row).  Per list: ursn_cluster_chains at max_gap
31, ursn_cluster_features alone, and a device-to-device copy of the lists the call reads (index, ids, the two object tables: the
floor of anything that reads them once).  The host alternative, once per reach: the D2H copy of the index and the two object tables,
then a vectorised numpy search (blocks of child rows against all apexes of their event).  Medians over --repeats windows of --inner
calls, ms per call.  Lists up to --numpy-max entries are compared with clusters.cluster_cones_numpy bit for bit.

Prints a table and one JSON line.

    python tools/cluster_cone_bench.py [--size 192] [--batch 4] [--big-size 256] [--big-batch 2] [--dense-size 96] [--dense-batch 4]
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


def vectorised_numpy(index, toff, itab, rtab, tcls, shape, reach, min_cos, seed_size, min_size):
    """The host competitor: the links from the object tables.  Returns their number."""
    shape = np.asarray(shape, np.int64)
    K = int(toff[-1])
    n, lo, hi = itab[:K, 0], itab[:K, 24], itab[:K, 25]
    parent = (n >= seed_size) & (lo != hi)
    rows = np.flatnonzero(parent)
    prow = np.concatenate([rows, rows])
    pos = np.concatenate([lo[rows], hi[rows]])
    u = np.concatenate([rtab[rows, 12:15], -rtab[rows, 12:15]])
    x = np.stack(np.unravel_index(index[pos], shape), 1)
    ev_p = np.searchsorted(toff, prow, side="right") - 1
    kids = np.flatnonzero(n >= min_size)
    ev_c = np.searchsorted(toff, kids, side="right") - 1
    links = 0
    for e in np.unique(ev_c):
        sel, cs = np.flatnonzero(ev_p == e), kids[ev_c == e]
        if not sel.size:
            continue
        for at in range(0, cs.size, 128):
            c = cs[at:at + 128]
            d = itab[c, 11:14][:, None, :] - x[sel][None, :, :]                        # [c, apex, 3] = m(c) - x(apex)
            dist2 = (d * d).sum(2)
            nc, npar = n[c][:, None], n[prow[sel]][None, :]
            ok = (np.abs(d).max(2) <= reach) & (dist2 >= 1) & (dist2 <= reach * reach) & (c[:, None] != prow[sel][None, :]) & \
                ((npar > nc) | ((npar == nc) & (prow[sel][None, :] < c[:, None]))) & (tcls[c][:, None] == tcls[prow[sel]][None, :])
            ic, ia = np.nonzero(ok)
            if not ic.size:
                continue
            dd, ua = d[ic, ia].astype(np.float64), u[sel][ia]
            t = (ua[:, 0] * dd[:, 0] + ua[:, 1] * dd[:, 1]) + ua[:, 2] * dd[:, 2]
            good = t / np.sqrt(dist2[ic, ia].astype(np.float64)) >= min_cos
            ax = rtab[c[ic], 12:15]
            c_ax = np.fabs((ua[:, 0] * ax[:, 0] + ua[:, 1] * ax[:, 1]) + ua[:, 2] * ax[:, 2])
            good &= ~parent[c[ic]] | (c_ax >= min_cos)
            links += int(np.unique(ic[good]).size)
    return links


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
    ap.add_argument("--min-cos", type=float, default=0.8)
    ap.add_argument("--seed-size", type=int, default=8)
    ap.add_argument("--min-size", type=int, default=1)
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--inner", type=int, default=5)
    args = ap.parse_args()
    import torch
    from uresnet_amd import _lib
    from uresnet_amd import synthetic_io as sio
    from uresnet_amd.clusters import CONE_INT, CONE_REAL, LINK_INT, LINK_REAL, ClusterConeSpec, ClusterSpec, cluster_cones_numpy
    assert torch.cuda.is_available(), "cluster_cone_bench: no HIP device visible"
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

    def events(gen, shape, n, knock=None):
        """(offsets, index, value, label) of n events; ``knock`` 'slabs' takes slabs out of everything, 'thin' thins the showers."""
        parts = []
        for e in range(n):
            vb = sio.dense_to_voxels(*gen(list(shape) + [1], 3, e))
            index, label, keep = np.asarray(vb.index, np.int64), np.asarray(vb.label), np.ones(vb.index.size, bool)
            if knock == "slabs":
                c = np.unravel_index(index, shape)
                keep = ~((c[0] % 12 >= 5) & (c[0] % 12 < 7)) & ~((c[2] % 10 >= 3) & (c[2] % 10 < 5))
            if knock == "thin":
                keep = (label != 1) | (((index * 2654435761) >> 7) % 4 == 0)
            parts.append((index[keep], np.asarray(vb.value, np.float32)[keep], label[keep]))
        off = np.concatenate([[0], np.cumsum([p[0].size for p in parts])]).astype(np.int64)
        return off, np.concatenate([p[0] for p in parts]).astype(np.int32), np.concatenate([p[1] for p in parts]), \
            np.concatenate([p[2] for p in parts]).astype(np.uint8)

    lists = []
    if args.batch:
        lists.append(("lartpc_sparse", (args.size,) * 3, events(sio.lartpc_sparse, (args.size,) * 3, args.batch)))
        lists.append(("lartpc_sparse cut", (args.size,) * 3, events(sio.lartpc_sparse, (args.size,) * 3, args.batch, "slabs")))
        lists.append(("lartpc_sparse thin", (args.size,) * 3, events(sio.lartpc_sparse, (args.size,) * 3, args.batch, "thin")))
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
        cap = max(K, 1)
        # the chains at their longest gap
        hneed = int(lib.ursn_cluster_chains_scratch_bytes(n, M))
        hscratch = new(hneed // 8, torch.int64)
        htabs = {"merged": new(max(M, 1), torch.int32), "chain_offsets": new(n + 1, torch.int64), "first": new(cap, torch.int32),
                 "size": new(cap, torch.int32), "cls": new(cap, torch.uint8), "chain_itab": new((cap, _lib.CLCHAIN_CI), torch.int64),
                 "chain_rtab": new((cap, _lib.CLCHAIN_CR), torch.float64), "join_offsets": new(n + 1, torch.int64),
                 "join_itab": new((cap, _lib.CLCHAIN_JI), torch.int64), "join_rtab": new((cap, _lib.CLCHAIN_JR), torch.float64),
                 "row_chain": new(cap, torch.int32), "row_join": new((cap, 2), torch.int32), "row_candidates": new((cap, 2), torch.int32),
                 "event": new((n, _lib.CLCHAIN_EV), torch.int64), "status": new(1, torch.int32)}
        hd = _lib.ursn_cluster_chain_desc()
        hd.ndim, hd.n, hd.max_gap, hd.m_total = 3, n, 31, M
        for i, s in enumerate(shape):
            hd.spatial[i] = s
        hd.offsets, hd.index, hd.cluster, hd.table_offsets = d_off.data_ptr(), d_index.data_ptr(), ints.data_ptr(), toff.data_ptr()
        hd.itab, hd.rtab, hd.feat_cap, hd.cls = itab.data_ptr(), rtab.data_ptr(), K, tcls.data_ptr()
        hd.min_cos, hd.min_size, hd.class_mask, hd.same_class = 0.9, 3, 0, 1
        ho = _lib.ursn_cluster_chain_out()
        for key, t in htabs.items():
            setattr(ho, key, t.data_ptr())
        ho.cap_chains = ho.cap_joins = ho.cap_rows = K
        chains = lambda: _lib.check(lib.ursn_cluster_chains(ctypes.byref(hd), ctypes.byref(ho), ptr(hscratch), hneed, stream))
        chains()
        torch.cuda.synchronize()
        assert int(htabs["status"].item()) == 0, "cluster_chains: status %d" % int(htabs["status"].item())
        chains_ms = timed(chains)
        del hscratch, htabs
        # the cones
        cneed = int(lib.ursn_cluster_cones_scratch_bytes(n, M))
        cscratch = new(cneed // 8, torch.int64)
        tabs = {"merged": new(max(M, 1), torch.int32), "shower_offsets": new(n + 1, torch.int64), "first": new(cap, torch.int32),
                "size": new(cap, torch.int32), "cls": new(cap, torch.uint8), "shower_itab": new((cap, _lib.CLCONE_SI), torch.int64),
                "shower_rtab": new((cap, _lib.CLCONE_SR), torch.float64), "link_offsets": new(n + 1, torch.int64),
                "link_itab": new((cap, _lib.CLCONE_LI), torch.int64), "link_rtab": new((cap, _lib.CLCONE_LR), torch.float64),
                "row_shower": new(cap, torch.int32), "row_parent": new(cap, torch.int32), "row_candidates": new(cap, torch.int32),
                "row_children": new((cap, 2), torch.int32), "row_depth": new(cap, torch.int32),
                "event": new((n, _lib.CLCONE_EV), torch.int64), "status": new(1, torch.int32)}
        for reach in (16, 48, 127):
            cd = _lib.ursn_cluster_cone_desc()
            cd.ndim, cd.n, cd.reach, cd.m_total = 3, n, reach, M
            for i, s in enumerate(shape):
                cd.spatial[i] = s
            cd.offsets, cd.index, cd.cluster, cd.table_offsets = d_off.data_ptr(), d_index.data_ptr(), ints.data_ptr(), toff.data_ptr()
            cd.itab, cd.rtab, cd.feat_cap, cd.cls = itab.data_ptr(), rtab.data_ptr(), K, tcls.data_ptr()
            cd.min_cos, cd.min_size, cd.class_mask, cd.same_class, cd.seed_size = args.min_cos, args.min_size, 0, 1, args.seed_size
            co = _lib.ursn_cluster_cone_out()
            for key, t in tabs.items():
                setattr(co, key, t.data_ptr())
            co.cap_showers = co.cap_links = co.cap_rows = K
            cones = lambda: _lib.check(lib.ursn_cluster_cones(ctypes.byref(cd), ctypes.byref(co), ptr(cscratch), cneed, stream))
            cones()
            torch.cuda.synchronize()
            code = int(tabs["status"].item())
            assert code == 0, "cluster_cones: status %d" % code

            def fetch():
                ns, nl = int(tabs["shower_offsets"][n].item()), int(tabs["link_offsets"][n].item())
                cut = {"first": ns, "size": ns, "cls": ns, "shower_itab": ns, "shower_rtab": ns, "link_itab": nl, "link_rtab": nl,
                       "row_shower": K, "row_parent": K, "row_candidates": K, "row_children": K, "row_depth": K, "merged": M}
                return {k: (t[:cut[k]] if k in cut else t).cpu().numpy().copy() for k, t in tabs.items()}
            wave = fetch()
            rec = dict(shape=list(shape), events=n, reach=reach, min_cos=args.min_cos, seed_size=args.seed_size, min_size=args.min_size,
                       list_entries=M, rows=K,
                       apexes=int(2 * ((host_itab[:K, 0] >= args.seed_size) & (host_itab[:K, 24] != host_itab[:K, 25])).sum()),
                       showers=int(wave["shower_itab"].shape[0]), links=int(wave["link_itab"].shape[0]),
                       largest=int(wave["shower_itab"][:, 0].max()) if wave["shower_itab"].size else 0,
                       depth=int(wave["row_depth"].max()) if K else 0,
                       candidates=int(wave["row_candidates"].sum()), scratch_bytes=cneed, cones_wave_ms=timed(cones),
                       chains_gap31_ms=chains_ms, features_ms=features_ms, copy_ms=copy_ms, d2h_ms=d2h_ms)
            os.environ["URSN_CLCONE_WAVE"] = "0"
            try:
                cones()
                torch.cuda.synchronize()
                plain = fetch()
                rec["routes_same_bits"] = bool(all(np.array_equal(plain[k].view(np.uint8), wave[k].view(np.uint8)) for k in wave))
                rec["cones_plain_ms"] = timed(cones)
            finally:
                os.environ.pop("URSN_CLCONE_WAVE", None)
            rec["numpy_vectorised_ms"] = float("nan")
            if K <= args.host_max:                              # blocks of child rows against all apexes of their event
                t0 = time.perf_counter()
                nl = vectorised_numpy(host_index, host_toff, host_itab, host_rtab, host_tcls, shape, reach, args.min_cos,
                                      args.seed_size, args.min_size)
                rec["numpy_vectorised_ms"] = (time.perf_counter() - t0) * 1e3
                assert nl == rec["links"], "the host route and the device disagree: %d links, %d" % (nl, rec["links"])
            if M <= args.numpy_max:
                t0 = time.perf_counter()
                want = cluster_cones_numpy(off, host_index, value, host_ids, host_toff, shape,
                                           ClusterConeSpec(reach, args.min_cos, args.seed_size, args.min_size), host_tcls[:K])
                rec["statement_ms"] = (time.perf_counter() - t0) * 1e3
                same = all(np.array_equal(wave[k], want[w]) for k, w in (
                    ("shower_offsets", "shower_offsets"), ("link_offsets", "link_offsets"), ("merged", "merged"), ("row_shower", "row_shower"),
                    ("row_parent", "row_parent"), ("row_candidates", "row_candidates"), ("row_children", "row_children"),
                    ("row_depth", "row_depth"), ("event", "events")))
                same = same and all(np.array_equal(wave[k], want["table"][k]) for k in ("first", "size", "cls"))
                for c, col in enumerate(CONE_INT):
                    same = same and np.array_equal(wave["shower_itab"][:, c], want["showers"][col])
                for c, col in enumerate(CONE_REAL):
                    same = same and np.array_equal(wave["shower_rtab"][:, c].view(np.uint64), want["showers"][col].view(np.uint64))
                for c, col in enumerate(LINK_INT):
                    same = same and np.array_equal(wave["link_itab"][:, c], want["links"][col])
                for c, col in enumerate(LINK_REAL):
                    same = same and np.array_equal(wave["link_rtab"][:, c].view(np.uint64), want["links"][col].view(np.uint64))
                rec["same_bits"] = bool(same)
            out["%s reach %d" % (name, reach)] = rec
            print("%-18s reach %3d: %d x %d^3, %d entries, %d rows, %d apexes, %d candidates, %d links, %d showers (largest %d, depth %d): "
                  "cones %.3f ms (plain form %.3f ms, same bits: %s), chains at max_gap 31 %.3f ms, features %.3f ms, list copy %.3f ms "
                  "| host: D2H %.3f ms, vectorised numpy %.1f ms, statement %s%s"
                  % (name, reach, n, shape[0], M, K, rec["apexes"], rec["candidates"], rec["links"], rec["showers"], rec["largest"],
                     rec["depth"], rec["cones_wave_ms"], rec["cones_plain_ms"], rec["routes_same_bits"], chains_ms, features_ms, copy_ms,
                     d2h_ms, rec["numpy_vectorised_ms"], "%.0f ms" % rec["statement_ms"] if "statement_ms" in rec else "not run",
                     "; device == statement: %s" % rec["same_bits"] if "same_bits" in rec else ""), flush=True)
        del scratch, fscratch, cscratch, copies, ints, toff, tcls, itab, rtab, tabs
        torch.cuda.empty_cache()
    out["repeats"], out["inner"] = args.repeats, args.inner
    print(json.dumps(out))


if __name__ == "__main__":
    main()
