#!/usr/bin/env python
"""What the reference's per-event CSV numbers (example_scripts/ana_csv.py:67-116) cost on the host and on the device, at
4 x 192^3 (cfg3, fp32) and 4 x 256^3 (cfg5, bf16), lartpc_sparse events, base filters 8, 3 classes.

    (a) host path      what a user had before inference_stats: inference() with the dense softmax copied to the host
                       (`infer_copy_ms`, forward pass + head + D2H copy) plus the numpy loop of ana_csv.py over it
                       (`numpy_loop_ms`), each part timed on its own
    (b) stats_ms       ssnet_base.inference_stats: forward pass + the class-statistics kernels, a few hundred bytes back
    (c) cstats         the "cstats" record of the profile log (pass 6; both launches of ursn_class_stats): time, algorithmic
                       bytes (logits + label + data of every voxel) and GB/s

Every figure is a median with (min .. max).  Prints one JSON line.

    python tools/ana_stats_bench.py [--shapes 192:fp32,256:bf16] [--batch 4] [--repeats 5]
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


def numpy_loop(softmax_batch, label_batch, num_class):
    """example_scripts/ana_csv.py:67-116 (the numbers only; the text formatting is not timed)."""
    rows = []
    for index in range(len(softmax_batch)):
        softmax, label = softmax_batch[index], np.squeeze(label_batch[index])
        prediction = np.argmax(softmax, axis=-1).astype(np.float32)
        acc_all = float((prediction == label).sum()) / prediction.size
        nonzero_px = np.where(label > 0)
        acc_nonzero = float((prediction[nonzero_px] == label[nonzero_px]).sum()) / max(prediction[nonzero_px].size, 1)
        row = [acc_all, acc_nonzero]
        for class_label in range(num_class):
            class_mask = np.where(label == class_label)
            npx = label[class_mask].size
            if npx:
                class_score = (softmax[..., class_label])[class_mask]
                row += [npx, float((prediction[class_mask] == class_label).sum()) / npx, class_score.mean(), class_score.std()]
            else:
                row += [0, -1., -1., -1.]
        rows.append(row)
    return rows


def one_shape(args, size, prec):
    import torch
    from uresnet_amd import _lib, uresnet
    from uresnet_amd import synthetic_io as sio
    lib = _lib.load()
    dims, ncls, n = (size,) * 3 + (1,), 3, args.batch
    ev = [sio.lartpc_sparse(dims, ncls, e) for e in range(n)]
    data, label = (torch.from_numpy(np.stack([e[j] for e in ev])).pin_memory().numpy() for j in range(2))
    net = uresnet(dims=list(dims), num_class=ncls, base_num_outputs=8)
    net.construct(trainable=False, use_weight=False, seed=1234, precision=prec)
    res = {"shape": "%d x %d^3 %s" % (n, size, prec), "softmax_bytes": n * size ** 3 * ncls * 4}

    def timed(fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = fn()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3, out

    infer = lambda: net.inference(None, data, label)
    stats = lambda: net.inference_stats(None, data, label)
    for _ in range(2):
        sm = infer()[0]
        st = stats()
    rows = numpy_loop(sm, label.reshape(sm.shape[:-1]), ncls)
    for i, row in enumerate(rows):          # the two paths agree (ties aside) before they are compared for speed
        assert [int(x) for x in row[2::4]] == [int(x) for x in st['npx'][i]], (row, st['npx'][i])
        assert abs(row[0] - st['acc_all'][i]) <= 1e-3
    t_inf, t_loop, t_st = [], [], []
    for _ in range(args.repeats):
        ms, out = timed(infer)
        t_inf.append(ms)
        t0 = time.perf_counter()
        numpy_loop(out[0], label.reshape(out[0].shape[:-1]), ncls)
        t_loop.append((time.perf_counter() - t0) * 1e3)
        t_st.append(timed(stats)[0])
    res["infer_copy_ms"], res["numpy_loop_ms"], res["stats_ms"] = stat(t_inf), stat(t_loop), stat(t_st)

    # ---- (c) the cstats record of the profile log -------------------------------------------------------------------------
    _lib.check(lib.ursn_profile_enable(net._handle, 1))
    ms, nbytes = [], 0.0
    for _ in range(args.repeats):
        stats()
        cnt = ctypes.c_int64(0)
        _lib.check(lib.ursn_profile_read(net._handle, None, 0, ctypes.byref(cnt)))
        recs = (_lib.ursn_prof_rec * max(int(cnt.value), 1))()
        _lib.check(lib.ursn_profile_read(net._handle, recs, int(cnt.value), ctypes.byref(cnt)))
        hit = [r for r in recs[:int(cnt.value)] if r.kernel == b"cstats"]
        assert len(hit) == 1, [r.kernel for r in recs[:int(cnt.value)] if r.pass_ == 6]
        ms.append(float(hit[0].ms))
        nbytes = float(hit[0].bytes)
    _lib.check(lib.ursn_profile_enable(net._handle, 0))
    res["cstats_us"] = stat([m * 1e3 for m in ms], 1)
    res["cstats_bytes"] = nbytes
    res["cstats_GBps"] = round(nbytes / (float(np.median(ms)) * 1e-3) / 1e9, 1)
    net._destroy()
    del net
    torch.cuda.empty_cache()
    return res


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--shapes", default="192:fp32,256:bf16", help="comma list of edge:precision")
    ap.add_argument("--batch", type=int, default=4)
    ap.add_argument("--repeats", type=int, default=5)
    args = ap.parse_args()
    import torch
    import uresnet_amd  # noqa: F401
    assert torch.cuda.is_available(), "ana_stats_bench.py needs a HIP device"
    out = []
    for item in args.shapes.split(","):
        size, prec = item.split(":")
        out.append(one_shape(args, int(size), prec))
    print(json.dumps({"batch": args.batch, "repeats": args.repeats, "shapes": out}))


if __name__ == "__main__":
    main()
