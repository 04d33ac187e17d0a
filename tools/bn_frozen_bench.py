#!/usr/bin/env python
"""What frozen-BatchNorm training costs and saves, at 4 x 192^3 (cfg3, fp32) and 4 x 256^3 (cfg5, bf16), lartpc_sparse events,
base filters 8, 3 classes.  Three legs per shape, each in a process of its own (URSN_BN_FROZEN_FUSED is read once per process),
run one after the other:

    batch    set_bn_mode('batch'): the reduce + finalise + apply passes as every step runs them
    path1    set_bn_mode('frozen') with URSN_BN_FROZEN_FUSED=0: the same passes, the finalise writing zero means
    fused    set_bn_mode('frozen'): the single-pass kernels wherever the sums are not already free

    bn_bwd_ms     the BatchNorm-backward launches of ONE step, summed: profiler records of pass id 5 (device events around every
                  record; weight gradients serialised on the caller's stream while profiling), per kernel name and in total,
                  with the bytes the records declare
    images_per_s  `--steps` accumulate steps + one synchronise between host clocks, `--repeats` times, unprofiled

Every figure is a median with (min .. max).  Prints one JSON line.

    python tools/bn_frozen_bench.py [--shapes 192:fp32,256:bf16] [--batch 4] [--steps 5] [--repeats 5]
"""
import argparse
import ctypes
import json
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
LEGS = (("batch", 'batch', "1"), ("path1", 'frozen', "0"), ("fused", 'frozen', "1"))


def stat(xs, digits=3):
    xs = sorted(xs)
    return {"median": round(float(np.median(xs)), digits), "min": round(xs[0], digits), "max": round(xs[-1], digits)}


def leg(args, size, prec, mode):
    import torch
    from uresnet_amd import _lib, uresnet
    from uresnet_amd import synthetic_io as sio
    lib = _lib.load()
    dims, ncls, n = (size,) * 3 + (1,), 3, args.batch
    ev = [sio.lartpc_sparse(dims, ncls, e) for e in range(n)]
    data, label, weight = (torch.from_numpy(np.stack([e[j] for e in ev])).cuda() for j in range(3))
    net = uresnet(dims=list(dims), num_class=ncls, base_num_outputs=8)
    net.construct(trainable=True, use_weight=True, seed=1234, precision=prec, bn_moving=True)
    assert net.bn_calibrate(None, [data]) == 1
    net.set_bn_mode(mode)
    step = lambda: net.accum_gradients(None, data, label, weight, fetch=False)
    net.zero_gradients(None)
    for _ in range(3):
        step()
    torch.cuda.synchronize()
    ips = []
    for _ in range(args.repeats):
        t0 = time.perf_counter()
        for _ in range(args.steps):
            step()
        torch.cuda.synchronize()
        ips.append(args.steps * n / (time.perf_counter() - t0))
    per, total, nbytes = {}, [], 0.0
    for _ in range(args.repeats):
        _lib.check(lib.ursn_profile_enable(net._handle, 1))
        step()
        torch.cuda.synchronize()
        cnt = ctypes.c_int64(0)
        _lib.check(lib.ursn_profile_read(net._handle, None, 0, ctypes.byref(cnt)))
        recs = (_lib.ursn_prof_rec * max(int(cnt.value), 1))()
        _lib.check(lib.ursn_profile_read(net._handle, recs, int(cnt.value), ctypes.byref(cnt)))
        _lib.check(lib.ursn_profile_enable(net._handle, 0))
        bn = [r for r in recs[:int(cnt.value)] if int(r.pass_) == 5]
        one = {}
        for r in bn:
            one[r.kernel.decode()] = one.get(r.kernel.decode(), 0.0) + float(r.ms)
        for k, v in one.items():
            per.setdefault(k, []).append(v)
        total.append(sum(one.values()))
        nbytes = sum(float(r.bytes) for r in bn)
        records = len(bn)
    return {"bn_bwd_ms": stat(total), "per_kernel_ms": {k: stat(v) for k, v in per.items()}, "records": records,
            "declared_GB": round(nbytes / 1e9, 3), "images_per_s": stat(ips, 2)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default="192:fp32,256:bf16")
    ap.add_argument("--batch", type=int, default=4)
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--leg", default="")      # internal: size:prec:mode, runs one leg in this process
    args = ap.parse_args()
    if args.leg:
        size, prec, mode = args.leg.split(":")
        print("LEG " + json.dumps(leg(args, int(size), prec, mode)))
        return
    out = []
    for spec in args.shapes.split(","):
        size, prec = spec.split(":")
        res = {"shape": "%d x %s^3 %s" % (args.batch, size, prec)}
        for name, mode, fused in LEGS:
            env = dict(os.environ)
            env["URSN_BN_FROZEN_FUSED"] = fused
            cmd = [sys.executable, os.path.abspath(__file__), "--leg", "%s:%s:%s" % (size, prec, mode), "--batch", str(args.batch),
                   "--steps", str(args.steps), "--repeats", str(args.repeats)]
            p = subprocess.run(cmd, env=env, check=True, stdout=subprocess.PIPE, universal_newlines=True)
            res[name] = json.loads([l for l in p.stdout.splitlines() if l.startswith("LEG ")][-1][4:])
        out.append(res)
    print(json.dumps({"bn_frozen_bench": out}))


if __name__ == "__main__":
    main()
