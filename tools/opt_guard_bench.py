#!/usr/bin/env python
"""What the guarded optimiser step costs, at the parameter count of the default workload (3-D 192^3, 8 base filters: ursn_query),
on a handle of batch 1 with random gradients.

    plain_adam_us        ursn_apply_adam: the one Adam launch
    guarded_neutral_us   ursn_apply_adam_guarded with clip_norm 0, weight_decay 0, skip_nonfinite 1 (finite gradients): statistics
                         (two launches), decision (one thread), Adam over the chunk table
    guarded_clip_decay_us  the same with a clip below the gradient norm and weight_decay 0.01
    stats_us             ursn_grad_stats without parameter norms: the statistics pass alone (reads the gradient buffer once)
    stats_with_params_us ursn_grad_stats with parameter norms (reads gradients and parameters)
    copy_us              a device-to-device copy of the bytes the statistics pass reads (the gradient buffer): the yardstick
    stats_over_copy      median stats_us / median copy_us

HIP events around `--calls` back-to-back calls, the legs alternating, `--repeats` times after a warm-up round; every figure is a
median with (min .. max), in microseconds per call.  Prints one JSON line.

    python tools/opt_guard_bench.py [--size 192] [--base 8] [--calls 50] [--repeats 7]
"""
import argparse
import ctypes
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def stat(xs, digits=1):
    xs = sorted(xs)
    return {"median": round(float(np.median(xs)), digits), "min": round(xs[0], digits), "max": round(xs[-1], digits)}


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--size", type=int, default=192)
    ap.add_argument("--base", type=int, default=8)
    ap.add_argument("--calls", type=int, default=50)
    ap.add_argument("--repeats", type=int, default=7)
    args = ap.parse_args()
    import torch
    from uresnet_amd import _lib, uresnet
    assert torch.cuda.is_available(), "opt_guard_bench.py needs a HIP device"
    lib = _lib.load()
    net = uresnet(dims=[args.size] * 3 + [1], num_class=3, base_num_outputs=args.base)
    net.construct(trainable=True, use_weight=True, learning_rate=1e-4, seed=1234)
    net.set_optimizer(skip_nonfinite=True)          # allocates and attaches the state
    n = net._n_params
    net._grads.copy_(torch.randn(n, device="cuda") * 1e-3)
    h, stream = net._handle, net._stream(None)
    norm = net.grad_stats(None, with_param_norms=False)['global']['grad_norm']

    def desc(clip, wd):
        d = _lib.ursn_opt_desc()
        d.lr, d.clip_norm, d.weight_decay, d.skip_nonfinite = 1e-4, clip, wd, 1
        return d

    d_neutral, d_on = desc(0.0, 0.0), desc(norm / 3.0, 0.01)
    dst = torch.empty_like(net._grads)
    legs = {
        "plain_adam_us": lambda: _lib.check(lib.ursn_apply_adam(h, 1e-4, stream)),
        "guarded_neutral_us": lambda: _lib.check(lib.ursn_apply_adam_guarded(h, ctypes.byref(d_neutral), stream)),
        "guarded_clip_decay_us": lambda: _lib.check(lib.ursn_apply_adam_guarded(h, ctypes.byref(d_on), stream)),
        "stats_us": lambda: _lib.check(lib.ursn_grad_stats(h, 0, stream)),
        "stats_with_params_us": lambda: _lib.check(lib.ursn_grad_stats(h, 1, stream)),
        "copy_us": lambda: dst.copy_(net._grads),
    }

    def events_us(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(args.calls):
            fn()
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1) / args.calls * 1e3

    for fn in legs.values():
        events_us(fn)
    us = {k: [] for k in legs}
    for _ in range(args.repeats):
        for k, fn in legs.items():
            us[k].append(events_us(fn))
    st = net.last_apply_status(None)
    assert st['skipped_total'] == 0 and torch.isfinite(net._params).all().item(), st
    res = {"n_params": n, "n_tensors": len(net._specs), "grad_bytes": 4 * n, "calls": args.calls, "repeats": args.repeats}
    res.update({k: stat(v) for k, v in us.items()})
    res["stats_over_copy"] = round(float(np.median(us["stats_us"]) / np.median(us["copy_us"])), 2)
    res["guarded_neutral_over_plain"] = round(float(np.median(us["guarded_neutral_us"]) / np.median(us["plain_adam_us"])), 2)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
