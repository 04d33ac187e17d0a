#!/usr/bin/env python
"""What the per-event weight normalisation costs on the host and on the device, at 4 x 192^3 (cfg3, fp32) and 4 x 256^3
(cfg5, bf16), lartpc_sparse weights.

    (a) host_norm_ms   the host pass exactly as ssnet_trainval._pull does it: weight /= np.sum(weight, axis=1).reshape(n, 1),
                       numpy, one process, on a fresh copy of the raw weights each time (the copy is outside the clock)
    (b) device_us      ursn_normalize_weights alone, HIP events around `--calls` back-to-back calls: in place (feed slot) and
                       out of place (caller's tensor), alternating, `--repeats` times
    (c) bytes / floor  bytes moved (one read for the sum, one read and one write for the divide: 3 x n x voxels x 4) and the
                       time that takes at 6.3 TB/s
    (d) step_ms        the training step fed from pinned dense host buffers every iteration with the switch off (host pass
                       inside the loop, as the driver runs it: the parent's behaviour) and on (normalize_weight=True),
                       `--steps` steps ending in a device synchronise, alternating, `--repeats` times

Every figure is a median with (min .. max).  Prints one JSON line.

    python tools/weight_norm_bench.py [--shapes 192:fp32,256:bf16] [--steps 10] [--repeats 5] [--calls 20] [--no-step]
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

HBM_BPS = 6.3e12     # achievable HBM rate of a streaming float4 kernel on the MI355X (8 TB/s spec)


def stat(xs, digits=3):
    xs = sorted(xs)
    return {"median": round(float(np.median(xs)), digits), "min": round(xs[0], digits), "max": round(xs[-1], digits)}


def one_shape(args, size, prec):
    import torch
    from uresnet_amd import _lib, uresnet
    from uresnet_amd import synthetic_io as sio
    lib = _lib.load()
    dims, ncls, n = (size,) * 3 + (1,), 3, args.batch
    V = size ** 3
    ev = [sio.lartpc_sparse(dims, ncls, e) for e in range(n)]
    data, label, raw = (np.stack([e[j] for e in ev]) for j in range(3))
    res = {"shape": "%d x %d^3 %s" % (n, size, prec), "bytes_moved": 3 * n * V * 4,
           "floor_us": round(3.0 * n * V * 4 / HBM_BPS * 1e6, 1)}

    # ---- (a) the host pass --------------------------------------------------------------------------------------------------
    host, work = [], np.empty_like(raw)
    for _ in range(args.repeats + 1):
        np.copyto(work, raw)
        t0 = time.perf_counter()
        work /= np.sum(work, axis=1).reshape([work.shape[0], 1])
        host.append((time.perf_counter() - t0) * 1e3)
    res["host_norm_ms"] = stat(host[1:])

    # ---- (b) the device call alone ------------------------------------------------------------------------------------------
    P = lambda t: ctypes.c_void_p(t.data_ptr())
    stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    w_dev, out = torch.from_numpy(raw).cuda(), torch.empty((n, V), dtype=torch.float32, device="cuda")
    need = int(lib.ursn_normalize_weights_scratch_bytes(n, V))
    scratch = torch.empty(need // 8, dtype=torch.float64, device="cuda")
    sums = torch.empty(n, dtype=torch.float32, device="cuda")

    def call(dst):
        return lambda: _lib.check(lib.ursn_normalize_weights(P(w_dev), P(dst), n, V, P(sums), P(scratch), need, stream))

    def events_us(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(args.calls):
            fn()
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1) / args.calls * 1e3

    call(out)()
    S = np.sum(raw, axis=1, dtype=np.float64)
    assert np.allclose(sums.cpu().numpy(), np.float32(S), rtol=2.0 ** -23, atol=0)      # the same float, or its neighbour
    assert np.abs(out.cpu().numpy().astype(np.float64) * S[:, None] - raw).max() <= 2e-7 * raw.max()
    legs = {"out_of_place": call(out), "in_place": call(w_dev)}     # in place renormalises its own output: same traffic
    for fn in legs.values():
        events_us(fn)
    us = {k: [] for k in legs}
    for _ in range(args.repeats):
        for k, fn in legs.items():
            us[k].append(events_us(fn))
    res["device_us"] = {k: stat(v, 1) for k, v in us.items()}
    res["device_over_floor"] = round(float(np.median(us["out_of_place"])) / res["floor_us"], 2)
    del w_dev, out
    if args.no_step:
        return res

    # ---- (d) the training step with the switch off and on ----------------------------------------------------------------------
    pin = [torch.from_numpy(a).pin_memory().numpy() for a in (data, label, raw)]
    io_buf = torch.from_numpy(raw.copy()).pin_memory().numpy()      # the IO buffer the host pass mutates
    net = uresnet(dims=list(dims), num_class=ncls, base_num_outputs=8)
    net.construct(trainable=True, use_weight=True, learning_rate=1e-4, seed=1234, precision=prec)

    def step_off():
        np.copyto(io_buf, pin[2])                                    # the IO thread's refill: outside the driver's own pass
        net.zero_gradients(None)
        io_buf[...] /= np.sum(io_buf, axis=1).reshape([n, 1])       # ssnet_trainval._pull
        net.accum_gradients(None, pin[0], pin[1], io_buf, fetch=False)
        net.apply_gradients(None)

    def step_on():
        np.copyto(io_buf, pin[2])
        net.zero_gradients(None)
        net.accum_gradients(None, pin[0], pin[1], io_buf, fetch=False, normalize_weight=True)
        net.apply_gradients(None)

    def timed(step):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(args.steps):
            step()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) / args.steps * 1e3

    for _ in range(2):
        step_off()
        step_on()
    ms = {"off": [], "on": []}
    for _ in range(args.repeats):
        ms["off"].append(timed(step_off))
        ms["on"].append(timed(step_on))
    res["step_ms_switch_off"], res["step_ms_switch_on"] = stat(ms["off"]), stat(ms["on"])
    net._destroy()
    del net
    torch.cuda.empty_cache()
    return res


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--shapes", default="192:fp32,256:bf16", help="comma list of edge:precision")
    ap.add_argument("--batch", type=int, default=4)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--no-step", action="store_true", help="legs (a)-(c) only")
    args = ap.parse_args()
    import torch
    import uresnet_amd  # noqa: F401
    assert torch.cuda.is_available(), "weight_norm_bench.py needs a HIP device"
    out = []
    for item in args.shapes.split(","):
        size, prec = item.split(":")
        out.append(one_shape(args, int(size), prec))
    print(json.dumps({"batch": args.batch, "steps": args.steps, "repeats": args.repeats, "calls": args.calls, "shapes": out}))


if __name__ == "__main__":
    main()
