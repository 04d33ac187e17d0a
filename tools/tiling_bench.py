#!/usr/bin/env python
"""What tiling (tiling.hip, ssnet_base.inference_tiled_voxel_scores) costs and what it gives, on lartpc_sparse events.

Part 1, the passes: events of 4 x the network's size per axis (--size S: network S^3, events (4 S)^3, --batch events), the grid at
--halo.  ursn_crop_count over all boxes, then for ALL kept boxes in one call ursn_crop_write and ursn_scores_scatter (rows of
random scores), timed between device events, against a device-to-device copy of the list's index and value arrays of the same
run: the floor of anything that reads the list once.  Medians over --repeats windows of --inner calls, ms per call.

Part 2, a tiled event end to end: inference_tiled_voxel_scores on the resident batch (wall clock, it synchronises) against the
same boxes cropped with tiling.crop_numpy on the host and fed one batch of --tile-batch at a time through inference_voxel_scores
and stitched with tiling.stitch_numpy -- what a user without the passes does.  Also tiles run of tiles total.

Part 3, what tiling is not: the SAME weights (get_variables / set_variables) in a network built at (2 T)^3 (--agree-tile T) and in
a network built at T^3 that analyses the same events as tiles of half the size per axis at halo 0, 8 and 16, both in moving mode
with the same (initial) moving statistics: the share of listed voxels whose `pred` agrees.

Prints a table and one JSON line.

    python tools/tiling_bench.py [--size 64] [--batch 2] [--halo 8] [--tile-batch 4] [--agree-tile 64] [--filters 16]
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
    ap.add_argument("--size", type=int, default=64)
    ap.add_argument("--batch", type=int, default=2)
    ap.add_argument("--halo", type=int, default=8)
    ap.add_argument("--tile-batch", type=int, default=4)
    ap.add_argument("--agree-tile", type=int, default=64)
    ap.add_argument("--filters", type=int, default=16)
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--inner", type=int, default=5)
    args = ap.parse_args()
    import torch
    from uresnet_amd import _lib, tiling, uresnet
    from uresnet_amd import synthetic_io as sio
    from uresnet_amd.ssnet import VoxelBatch
    assert torch.cuda.is_available(), "tiling_bench: no HIP device visible"
    lib = _lib.load()
    P = lambda t: ctypes.c_void_p(t.data_ptr()) if t is not None else None

    def events(big, n, first=0):
        return VoxelBatch.concat([sio.dense_to_voxels(*sio.lartpc_sparse(list(big) + [1], 3, first + e)) for e in range(n)])

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

    out = {}
    # ---- part 1 and 2 ----------------------------------------------------------------------------------------------------------
    T, S = args.size, 4 * args.size
    tile, big = (T, T, T), (S, S, S)
    net = uresnet(dims=list(tile) + [1], num_class=3, base_num_outputs=args.filters)
    net.construct(trainable=False, use_weight=False, seed=7)
    vb = events(big, args.batch)
    bare = VoxelBatch(vb.offsets, vb.index, vb.value, voxels=vb.voxels)
    M = int(vb.offsets[-1])
    resident = net.upload_voxels(bare, big)
    boxes = tiling.grid(big, tile, args.halo, args.batch)
    stream = net._stream(None)
    dev_boxes = net._upload_boxes(boxes, "tiling_bench")
    d = net._crop_desc(resident, boxes, dev_boxes)
    scratch = net._crop_scratch(d)
    counts = torch.empty((2, len(boxes)), dtype=torch.int64, device="cuda")
    count = lambda: _lib.check(lib.ursn_crop_count(ctypes.byref(d), P(counts[0]), P(counts[1]), P(scratch), scratch.numel() * 8, stream))
    count()
    host_counts = counts.cpu().numpy()
    keep = np.flatnonzero(host_counts[1] > 0)
    run = boxes.select(keep)
    m = int(host_counts[0][keep].sum())
    dev_run = net._upload_boxes(run, "tiling_bench")
    dr = net._crop_desc(resident, run, dev_run)
    bufs = {"offsets": torch.empty(len(run) + 1, dtype=torch.int64, device="cuda"), "index": torch.empty(m, dtype=torch.int32, device="cuda"),
            "value": torch.empty(m, device="cuda"), "src": torch.empty(m, dtype=torch.int32, device="cuda"),
            "owned": torch.empty(m, dtype=torch.uint8, device="cuda")}
    o = _lib.ursn_crop_out()
    for k, t in bufs.items():
        setattr(o, k, t.data_ptr())
    o.cap = m
    write = lambda: _lib.check(lib.ursn_crop_write(ctypes.byref(dr), ctypes.byref(o), P(scratch), scratch.numel() * 8, stream))
    rows, big_rows = torch.rand((m, 3), device="cuda"), torch.empty((M, 3), device="cuda")
    pred, big_pred = torch.zeros(m, dtype=torch.uint8, device="cuda"), torch.empty(M, dtype=torch.uint8, device="cuda")
    scatter = lambda: _lib.check(lib.ursn_scores_scatter(P(bufs["src"]), P(bufs["owned"]), m, 3, P(rows), P(pred), None, P(big_rows),
                                                         P(big_pred), None, M, stream))
    list_src = [torch.empty(M, dtype=torch.int32, device="cuda"), torch.empty(M, device="cuda")]
    list_dst = [torch.empty_like(t) for t in list_src]

    def copy():
        for a, b in zip(list_src, list_dst):
            b.copy_(a)
    for fn in (count, write, scatter, copy):
        fn()
    torch.cuda.synchronize()
    ms = {"count": timed(count), "write": timed(write), "scatter": timed(scatter), "copy": timed(copy)}
    out["passes"] = dict(ms, network=T, events=S, batch=args.batch, halo=args.halo, list_entries=M, boxes=len(boxes), boxes_kept=len(run),
                         crop_entries=m)
    print("passes at %d x %d^3 events, network %d^3, halo %d: %d list entries, %d boxes (%d own a voxel, %d crop entries)"
          % (args.batch, S, T, args.halo, M, len(boxes), len(run), m))
    print("  crop_count %.4f ms   crop_write %.4f ms   scores_scatter %.4f ms   sum %.4f ms   list copy (index + value) %.4f ms"
          % (ms["count"], ms["write"], ms["scatter"], ms["count"] + ms["write"] + ms["scatter"], ms["copy"]))

    tb = args.tile_batch
    net.inference_tiled_voxel_scores(None, resident, big, halo=args.halo, tile_batch=tb)       # warm-up: handle, buffers
    t0 = time.perf_counter()
    r = net.inference_tiled_voxel_scores(None, resident, big, halo=args.halo, tile_batch=tb)
    t_dev = time.perf_counter() - t0

    def host_path():
        res = {"scores": np.zeros((M, 3), np.float32), "pred": np.zeros(M, np.uint8), "ana": np.zeros(M, np.uint8)}
        owned_count = tiling.crop_numpy(bare, big, tile, boxes)[4]
        todo = boxes.select(np.flatnonzero(owned_count > 0))
        for first in range(0, len(todo), tb):
            crop, src, owned, _, _ = tiling.crop_numpy(bare, big, tile, todo.select(slice(first, first + tb)))
            got = net.inference_voxel_scores(None, crop, with_labels=False)
            tiling.stitch_numpy(res, src, owned, **{w: np.concatenate(got[w]) for w in ("scores", "pred", "ana")})
        return res
    host_path()
    t0 = time.perf_counter()
    h = host_path()
    t_host = time.perf_counter() - t0
    same = all(np.array_equal(np.concatenate(r[w]).view(np.uint8), h[w].view(np.uint8)) for w in ("scores", "pred", "ana"))
    out["tiled"] = dict(device_s=t_dev, host_s=t_host, tiles_run=r["tiles_run"], tiles_total=r["tiles_total"], forwards=r["forwards"],
                        tile_batch=tb, same_bits=bool(same))
    print("tiled batch, tile_batch %d: device passes %.3f s, host crops through inference_voxel_scores %.3f s (same bits: %s); "
          "%d of %d tiles run in %d forwards" % (tb, t_dev, t_host, same, r["tiles_run"], r["tiles_total"], r["forwards"]))
    del net, resident

    # ---- part 3 ----------------------------------------------------------------------------------------------------------------
    A = args.agree_tile
    small, large = (A, A, A), (2 * A, 2 * A, 2 * A)
    whole = uresnet(dims=list(large) + [1], num_class=3, base_num_outputs=args.filters)
    whole.construct(trainable=False, use_weight=False, seed=7, bn_moving=True)
    tiles = uresnet(dims=list(small) + [1], num_class=3, base_num_outputs=args.filters)
    tiles.construct(trainable=False, use_weight=False, seed=11, bn_moving=True)
    tiles.set_variables(whole.get_variables())
    tiles.set_bn_moving(whole.get_bn_moving())
    whole.set_bn_mode("moving")
    tiles.set_bn_mode("moving")
    ev = events(large, 4, first=10)
    ev = VoxelBatch(ev.offsets, ev.index, ev.value, voxels=ev.voxels)
    ref = np.concatenate(whole.inference_voxel_scores(None, ev, with_labels=False, want=("pred",))["pred"])
    out["agreement"] = {}
    for halo in (0, 8, 16):
        if A - 2 * halo < 1:
            continue
        got = tiles.inference_tiled_voxel_scores(None, ev, large, halo=halo, tile_batch=4, want=("pred",))
        share = float((np.concatenate(got["pred"]) == ref).mean())
        out["agreement"][str(halo)] = dict(share=share, tiles_run=got["tiles_run"], tiles_total=got["tiles_total"])
        print("same weights at %d^3 against tiles of %d^3, moving mode, halo %2d: pred agrees at %.4f of %d voxels (%d of %d tiles run)"
              % (2 * A, A, halo, share, ref.size, got["tiles_run"], got["tiles_total"]))
    print(json.dumps(out))


if __name__ == "__main__":
    main()
