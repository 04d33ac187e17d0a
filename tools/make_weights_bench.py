#!/usr/bin/env python
"""What making the loss weights on the device costs, at 4 x 192^3 and 4 x 256^3.

    (a) device_us      ONE ursn_make_weights call between two device events, `--calls` calls one by one: median (min .. max),
                       for labels `lartpc_sparse` (a few tracks and showers on an empty background) and `dense_uniform` (every
                       voxel a random class, two thirds of them foreground: every thread enters the neighbour scan), radius
                       0, 1, 2, 3, mode 'invfreq'
    (b) d2d_us         a device-to-device copy of one [n, voxels] fp32 tensor (reads one tensor, writes one; the call reads
                       one, writes and reads a quarter -- the byte map -- and writes one: 2.5 tensors against 2), same clock
    (c) h2d_us         the copy the call replaces: the dense weight tensor from page-locked host memory, same clock
    (d) numpy_ms       weights.make_weights_numpy on the host, radii `--numpy-radii`, once each (wall clock)
    (e) h2d_bytes      ssnet_base.feed_stats['h2d_bytes'] of one accumulate call with and without make_weight, dense feed and
                       voxel feed, at `--feed-size`^3 (the bytes scale with the volume; the network is built for this leg only)

Ratios `over_d2d` and `over_h2d` are medians over medians.  Prints one JSON line.  The bench.py headline with the feature off
is measured with bench.py itself, alternating with the parent commit on one box.

    python tools/make_weights_bench.py [--sizes 192,256] [--calls 50] [--numpy-radii 0,1] [--feed-size 64] [--no-feed]
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


def stat(xs, digits=1):
    xs = sorted(xs)
    return {"median": round(float(np.median(xs)), digits), "min": round(xs[0], digits), "max": round(xs[-1], digits)}


def timed_us(fn, calls):
    import torch
    out = []
    for _ in range(3):
        fn()
    for _ in range(calls):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        e1.synchronize()
        out.append(e0.elapsed_time(e1) * 1e3)
    return out


def one_size(args, size):
    import torch
    from uresnet_amd import _lib
    from uresnet_amd import synthetic_io as sio
    from uresnet_amd.weights import WeightSpec, make_weights_numpy
    lib = _lib.load()
    dims, ncls, n = (size,) * 3 + (1,), 3, args.batch
    V = size ** 3
    P = lambda t: ctypes.c_void_p(t.data_ptr())
    stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    res = {"shape": "%d x %d^3" % (n, size), "tensor_bytes": n * V * 4}
    out = torch.empty((n, V), dtype=torch.float32, device="cuda")
    counts = torch.empty((n, ncls + 1), dtype=torch.int64, device="cuda")
    sp = (ctypes.c_int32 * 3)(size, size, size)
    need = int(lib.ursn_make_weights_scratch_bytes(3, sp, n, ncls, 3))
    scratch = torch.empty((need + 7) // 8, dtype=torch.float64, device="cuda")

    for gen in ("lartpc_sparse", "dense_uniform"):
        label = np.stack([sio.GENERATORS[gen](dims, ncls, e)[1] for e in range(n)])
        lab = torch.from_numpy(label).cuda()
        leg = {"foreground_fraction": round(float(np.count_nonzero(label >= 1)) / label.size, 5)}
        for r in range(4):
            d = _lib.ursn_make_weights_desc()
            d.ndim, d.n, d.voxels, d.ncls, d.radius, d.mode = 3, n, V, ncls, r, 1
            for i in range(3):
                d.spatial[i] = size
            for i in range(9):
                d.scale[i] = 1.0
            call = lambda: _lib.check(lib.ursn_make_weights(ctypes.byref(d), P(lab), P(out), P(counts), P(scratch), need, stream))
            leg["r%d_us" % r] = stat(timed_us(call, args.calls))
            leg["r%d_boundary_voxels" % r] = int(counts.cpu().numpy()[:, ncls].sum())
            if r in args.numpy_radii and gen == "lartpc_sparse":
                t0 = time.perf_counter()
                want, want_counts = make_weights_numpy(label, dims[:-1], ncls, WeightSpec("invfreq", r))
                res["numpy_ms_r%d" % r] = round((time.perf_counter() - t0) * 1e3, 1)
                assert np.array_equal(out.cpu().numpy().view(np.uint32), want.view(np.uint32))
                assert np.array_equal(counts.cpu().numpy(), want_counts)
        res[gen] = leg
        del lab

    src = torch.rand((n, V), dtype=torch.float32, device="cuda")
    res["d2d_us"] = stat(timed_us(lambda: out.copy_(src), args.calls))
    host = torch.empty((n, V), dtype=torch.float32, pin_memory=True)
    host.fill_(1.0)
    res["h2d_us"] = stat(timed_us(lambda: out.copy_(host, non_blocking=True), args.calls))
    for gen in ("lartpc_sparse", "dense_uniform"):
        for r in range(4):
            m = res[gen]["r%d_us" % r]["median"]
            res[gen]["r%d_over_d2d" % r] = round(m / res["d2d_us"]["median"], 2)
            res[gen]["r%d_over_h2d" % r] = round(m / res["h2d_us"]["median"], 3)
    return res


def feed_bytes(args):
    """h2d_bytes of one accumulate call per feed, with host weights and with make_weight."""
    from uresnet_amd import uresnet
    from uresnet_amd import synthetic_io as sio
    from uresnet_amd.ssnet import VoxelBatch
    from uresnet_amd.weights import WeightSpec
    size, n, ncls = args.feed_size, args.batch, 3
    dims = (size,) * 3 + (1,)
    ev = [sio.lartpc_sparse(dims, ncls, e) for e in range(n)]
    data, label, weight = (np.stack([e[j] for e in ev]) for j in range(3))
    vb_w = VoxelBatch.concat([sio.dense_to_voxels(data[i], label[i], weight[i]) for i in range(n)])
    vb = VoxelBatch.concat([sio.dense_to_voxels(data[i], label[i]) for i in range(n)])
    net = uresnet(dims=list(dims), num_class=ncls, base_num_outputs=8)
    net.construct(trainable=True, use_weight=True, learning_rate=1e-4, seed=1234)
    spec = WeightSpec("invfreq", 0)
    legs = {"dense_host_weights": lambda: net.accum_gradients(None, data, label, weight, fetch=False),
            "dense_make_weight": lambda: net.accum_gradients(None, data, label, fetch=False, make_weight=spec),
            "voxel_host_weights": lambda: net.accum_gradients_voxels(None, vb_w, fetch=False),
            "voxel_make_weight": lambda: net.accum_gradients_voxels(None, vb, fetch=False, make_weight=spec)}
    out = {"shape": "%d x %d^3" % (n, size), "listed_voxels": int(vb.offsets[-1])}
    net.zero_gradients(None)
    for name, fn in legs.items():
        before = net.feed_stats["h2d_bytes"] if hasattr(net, "feed_stats") else 0
        fn()
        out[name] = net.feed_stats["h2d_bytes"] - before
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--sizes", default="192,256")
    ap.add_argument("--batch", type=int, default=4)
    ap.add_argument("--calls", type=int, default=50)
    ap.add_argument("--numpy-radii", default="0,1")
    ap.add_argument("--feed-size", type=int, default=64)
    ap.add_argument("--no-feed", action="store_true")
    args = ap.parse_args()
    args.numpy_radii = [int(r) for r in args.numpy_radii.split(",") if r]
    import torch
    import uresnet_amd  # noqa: F401
    assert torch.cuda.is_available(), "make_weights_bench.py needs a HIP device"
    res = {"batch": args.batch, "calls": args.calls, "sizes": [one_size(args, int(s)) for s in args.sizes.split(",")]}
    if not args.no_feed:
        res["h2d_bytes"] = feed_bytes(args)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
