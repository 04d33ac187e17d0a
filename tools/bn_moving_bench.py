#!/usr/bin/env python
"""What BatchNorm moving statistics cost, at 4 x 192^3 (cfg3, fp32) and 4 x 256^3 (cfg5, bf16), lartpc_sparse events, base
filters 8, 3 classes.

    (a) update         ursn_bn_update after a forward: device-event time per call over a queue of `--queue` calls
                       (`update_us`; the host enqueue is part of it when it is the slower side), and the "bn_moving_update"
                       record of the profile log: launches of one call and its device time (the buffer is restored afterwards)
    (b) frozen load    the "bn_frozen_load" record of the profile log of a frozen forward: launches and device time
    (c) labels_ms      ssnet_base.inference_labels (device tensors in, device tensor out: forward + head + synchronise) in
                       'batch' and in 'moving' mode, alternating, and the per-repeat difference moving - batch.  The statistics
                       reductions inside the conv kernels still run in 'moving' mode (their finalise writes to a scratch pair),
                       so 'moving' costs what 'batch' costs plus the load launch

Every figure is a median with (min .. max).  Prints one JSON line.

    python tools/bn_moving_bench.py [--shapes 192:fp32,256:bf16] [--batch 4] [--repeats 7] [--queue 200]
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


def stat(xs, digits=3):
    xs = sorted(xs)
    return {"median": round(float(np.median(xs)), digits), "min": round(xs[0], digits), "max": round(xs[-1], digits)}


def profile_records(lib, _lib, handle):
    cnt = ctypes.c_int64(0)
    _lib.check(lib.ursn_profile_read(handle, None, 0, ctypes.byref(cnt)))
    recs = (_lib.ursn_prof_rec * max(int(cnt.value), 1))()
    _lib.check(lib.ursn_profile_read(handle, recs, int(cnt.value), ctypes.byref(cnt)))
    return list(recs[:int(cnt.value)])


def one_shape(args, size, prec):
    import torch
    from uresnet_amd import _lib, uresnet
    from uresnet_amd import synthetic_io as sio
    lib = _lib.load()
    dims, ncls, n = (size,) * 3 + (1,), 3, args.batch
    data = torch.from_numpy(np.stack([sio.lartpc_sparse(dims, ncls, e)[0] for e in range(n)])).cuda()
    net = uresnet(dims=list(dims), num_class=ncls, base_num_outputs=8)
    net.construct(trainable=False, use_weight=False, seed=1234, precision=prec, bn_moving=True)
    res = {"shape": "%d x %d^3 %s" % (n, size, prec), "layers": len(net._bn_specs), "moving_floats": net._bn_size}

    labels = lambda: net.inference_labels(None, data, as_numpy=False)

    def timed(fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3

    assert net.bn_calibrate(None, [data]) == 1         # usable statistics: the batch's own
    for mode in ('batch', 'moving') * 2:               # warm both modes
        net.set_bn_mode(mode)
        labels()
    t = {'batch': [], 'moving': []}
    for _ in range(args.repeats):
        for mode in ('batch', 'moving'):
            net.set_bn_mode(mode)
            t[mode].append(timed(labels))
    res["labels_ms"] = {m: stat(v) for m, v in t.items()}
    res["labels_moving_minus_batch_ms"] = stat([b - a for a, b in zip(t['batch'], t['moving'])])

    # ---- (b) the frozen load in the profile log ------------------------------------------------------------------------------
    net.set_bn_mode('moving')
    _lib.check(lib.ursn_profile_enable(net._handle, 1))
    us, launches = [], set()
    for _ in range(args.repeats):
        labels()
        hit = [r for r in profile_records(lib, _lib, net._handle) if r.kernel == b"bn_frozen_load"]
        assert len(hit) == 1, len(hit)
        us.append(float(hit[0].ms) * 1e3)
        launches.add(int(hit[0].launches))
    _lib.check(lib.ursn_profile_enable(net._handle, 0))
    res["frozen_load_us"], res["frozen_load_launches"] = stat(us, 1), sorted(launches)
    net.set_bn_mode('batch')
    _lib.check(lib.ursn_profile_enable(net._handle, 1))
    labels()
    assert not [r for r in profile_records(lib, _lib, net._handle) if r.kernel == b"bn_frozen_load"]   # batch mode: no such launch
    _lib.check(lib.ursn_profile_enable(net._handle, 0))

    # ---- (a) the update ------------------------------------------------------------------------------------------------------
    keep = net.get_bn_moving()
    labels()                                           # a batch-mode forward whose statistics the updates fold in
    stream = net._stream(None)
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    per_call = []
    for _ in range(args.repeats):
        torch.cuda.synchronize()
        e0.record()
        for _ in range(args.queue):
            _lib.check(lib.ursn_bn_update(net._handle, 0.001, stream))
        e1.record()
        torch.cuda.synchronize()
        per_call.append(e0.elapsed_time(e1) * 1e3 / args.queue)
    res["update_us"] = stat(per_call, 2)
    # ... and as the profile log records one call: launches and device time of the kernel alone
    _lib.check(lib.ursn_profile_enable(net._handle, 1))
    us, launches = [], set()
    for _ in range(args.repeats):
        labels()
        _lib.check(lib.ursn_bn_update(net._handle, 0.001, stream))
        hit = [r for r in profile_records(lib, _lib, net._handle) if r.kernel == b"bn_moving_update"]
        assert len(hit) == 1, len(hit)
        us.append(float(hit[0].ms) * 1e3)
        launches.add(int(hit[0].launches))
    _lib.check(lib.ursn_profile_enable(net._handle, 0))
    res["update_kernel_us"], res["update_launches"] = stat(us, 1), sorted(launches)
    net.set_bn_moving(keep)
    net._destroy()
    del net
    torch.cuda.empty_cache()
    return res


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--shapes", default="192:fp32,256:bf16", help="comma list of edge:precision")
    ap.add_argument("--batch", type=int, default=4)
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--queue", type=int, default=200)
    args = ap.parse_args()
    import torch
    import uresnet_amd  # noqa: F401
    assert torch.cuda.is_available(), "bn_moving_bench.py needs a HIP device"
    out = []
    for item in args.shapes.split(","):
        size, prec = item.split(":")
        out.append(one_shape(args, int(size), prec))
    print(json.dumps({"batch": args.batch, "repeats": args.repeats, "queue": args.queue, "shapes": out}))


if __name__ == "__main__":
    main()
