#!/usr/bin/env python
"""What the device loss head costs, at 4 x 192^3 F 8 (cfg3, fp32) and 4 x 256^3 F 8 (cfg5, bf16), lartpc_sparse events fed from
device tensors (the shapes of tools/ext_loss_bench.py).

    (a) step_ms                 accum_gradients(fetch=False): the fused step, the plan's own head
    (b) custom_<spec>_ms        accum_gradients_custom with losses.loss_torch(spec): the external loss boundary
    (c) loss_<spec>_ms          accum_gradients(loss=spec, fetch=False): the device loss head
                                specs: neutral, focal + smoothing (gamma 2, 0.1), focal + Dice (gamma 2, weight 0.5)
    (d) launches                "losshead" / "losssums" / "lossfinal" from ursn_profile_read, weight gradients serialised on the
                                caller's stream while profiling, each against its counted bytes at 6.3 TB/s

(a)-(c): `--steps` calls ending in a device synchronise, the legs alternating, `--repeats` times; every figure is a median with
(min .. max).  One GPU process; reads nothing from the oracle.  Prints one JSON line.

    python tools/loss_head_bench.py [--shapes 192:fp32,256:bf16] [--steps 5] [--repeats 5]
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
NEW = ("losshead", "losssums", "lossfinal")


def stat(xs, digits=3):
    xs = sorted(xs)
    return {"median": round(float(np.median(xs)), digits), "min": round(xs[0], digits), "max": round(xs[-1], digits)}


def one_shape(args, size, prec):
    import torch
    from uresnet_amd import _lib, uresnet
    from uresnet_amd import synthetic_io as sio
    from uresnet_amd.losses import LossSpec, loss_torch
    lib = _lib.load()
    dims, ncls, n = (size,) * 3 + (1,), 3, args.batch
    ev = [sio.lartpc_sparse(dims, ncls, e) for e in range(n)]
    data, label, weight = (torch.from_numpy(np.stack([e[j] for e in ev])).cuda() for j in range(3))
    weight = weight / weight.sum(dim=1, keepdim=True)
    net = uresnet(dims=list(dims), num_class=ncls, base_num_outputs=8)
    net.construct(trainable=True, use_weight=True, learning_rate=1e-4, seed=1234, precision=prec)
    res = {"shape": "%d x %d^3 F 8 %s" % (n, size, prec)}
    specs = {"neutral": LossSpec(), "focal_smooth": LossSpec(gamma=2.0, smoothing=0.1), "focal_dice": LossSpec(gamma=2.0, dice_weight=0.5)}

    legs = {"step_ms": lambda: net.accum_gradients(None, data, label, weight, fetch=False)}
    for name, spec in specs.items():
        legs["custom_%s_ms" % name] = (lambda f: lambda: net.accum_gradients_custom(None, data, f, fetch=False))(loss_torch(spec, label, weight))
        legs["loss_%s_ms" % name] = (lambda s: lambda: net.accum_gradients(None, data, label, weight, fetch=False, loss=s))(spec)

    def timed(fn):
        net.zero_gradients(None)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(args.steps):
            fn()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) / args.steps * 1e3

    for fn in legs.values():
        for _ in range(2):
            fn()
    ms = {k: [] for k in legs}
    for _ in range(args.repeats):
        for k, fn in legs.items():
            ms[k].append(timed(fn))
    for k in legs:
        res[k] = stat(ms[k])
    for name in specs:   # how far (c) sits from (a) and from (b)
        res["loss_%s_over_step_ms" % name] = round(res["loss_%s_ms" % name]["median"] - res["step_ms"]["median"], 3)
        res["loss_%s_under_custom_ms" % name] = round(res["custom_%s_ms" % name]["median"] - res["loss_%s_ms" % name]["median"], 3)

    # ---- (d) the new launches, timed by the library's own events -------------------------------------------------------------
    _lib.check(lib.ursn_set_wgrad_overlap(net._handle, 0))      # concurrent kernels time-slice: serialise for per-kernel timing
    res["launches"] = {}
    for name, spec in specs.items():
        _lib.check(lib.ursn_profile_enable(net._handle, 1))
        per, floor = {}, {}
        for _ in range(args.repeats):
            legs["loss_%s_ms" % name]()
            torch.cuda.synchronize()
            cnt = ctypes.c_int64(0)
            _lib.check(lib.ursn_profile_read(net._handle, None, 0, ctypes.byref(cnt)))
            recs = (_lib.ursn_prof_rec * max(cnt.value, 1))()
            _lib.check(lib.ursn_profile_read(net._handle, recs, cnt.value, ctypes.byref(cnt)))
            seen = {}
            for r in recs[:cnt.value]:
                k = r.kernel.decode()
                if k in NEW:
                    seen[k] = seen.get(k, 0) + 1
                    key = k if seen[k] == 1 else "%s#%d" % (k, seen[k])
                    per.setdefault(key, []).append(r.ms * 1e3)
                    floor[key] = r.bytes / HBM_BPS * 1e6
        _lib.check(lib.ursn_profile_enable(net._handle, 0))
        out = {}
        for k in per:
            us = stat(per[k], 1)
            out[k] = {"us": us, "floor_us": round(floor[k], 1), "over_floor": round(us["median"] / max(floor[k], 1e-9), 2)}
        res["launches"][name] = out or "not measured"
    _lib.check(lib.ursn_set_wgrad_overlap(net._handle, 1))
    net._destroy()
    del net
    torch.cuda.empty_cache()
    return res


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--shapes", default="192:fp32,256:bf16", help="comma list of edge:precision")
    ap.add_argument("--batch", type=int, default=4)
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--repeats", type=int, default=5)
    args = ap.parse_args()
    import torch
    import uresnet_amd  # noqa: F401
    assert torch.cuda.is_available(), "loss_head_bench.py needs a HIP device"
    out = []
    for item in args.shapes.split(","):
        size, prec = item.split(":")
        out.append(one_shape(args, int(size), prec))
    print(json.dumps({"batch": args.batch, "steps": args.steps, "repeats": args.repeats, "shapes": out}))


if __name__ == "__main__":
    main()
