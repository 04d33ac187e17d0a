#!/usr/bin/env python
"""What the symmetry passes (symmetry.hip) cost on the device at 4 x 192^3, one input channel.

ursn_sym_apply on the (data, label, weight) triple, per op class --

    flip        identity permutation, flips only                      (row copies, reversed when the last axis flips)
    keep-last   the two outer axes swap, the last axis stays last     (row copies from permuted rows)
    move-last   the last axis moves                                   (32 x 32 tiles through LDS)
    mixed       a different random code per event

-- against two baselines timed in the same run, alternating with it:

    copy        a device-to-device copy of the same three tensors: the floor, every byte read once and written once
    torch       permute(...).flip(...).contiguous() on the same tensors: what a user without the pass would call

and ursn_voxels_to_dense_sym against the unchanged ursn_voxels_to_dense on a lartpc_sparse batch.  Times are device-event
medians over --repeats windows of --inner calls, in ms per call; `x copy` is the ratio to the copy floor of the same run.
Prints a table and one JSON line.

    python tools/symmetry_bench.py [--size 192] [--batch 4] [--repeats 7] [--inner 5]
"""
import argparse
import ctypes
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

CLASSES = [("flip", [1, 2, 4, 7]), ("keep-last", [16, 21]), ("move-last", [8, 13, 24, 32, 43])]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", type=int, default=192)
    ap.add_argument("--batch", type=int, default=4)
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--inner", type=int, default=5)
    args = ap.parse_args()
    import torch
    from uresnet_amd import _lib
    from uresnet_amd import symmetry as S
    from uresnet_amd import synthetic_io as sio
    from uresnet_amd.ssnet import VoxelBatch
    assert torch.cuda.is_available(), "symmetry_bench: no HIP device visible"
    lib = _lib.load()
    n, s = args.batch, args.size
    spatial, V = (s, s, s), s ** 3
    dev = torch.device("cuda")
    src = [torch.rand((n, V), device=dev) for _ in range(3)]
    dst = [torch.empty((n, V), device=dev) for _ in range(3)]
    stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    P = lambda t: ctypes.c_void_p(t.data_ptr()) if t is not None else None

    def desc(codes):
        d = _lib.ursn_sym_desc()
        d.ndim = 3
        for i in range(3):
            d.spatial[i] = s
        d.n, d.channels = n, 1
        keep = (ctypes.c_int32 * n)(*codes)
        d.ops = ctypes.cast(keep, ctypes.POINTER(ctypes.c_int32))
        return d, keep

    def ours(codes):
        d, keep = desc(codes)

        def run():
            _lib.check(lib.ursn_sym_apply(ctypes.byref(d), P(src[0]), P(dst[0]), P(src[1]), P(dst[1]), P(src[2]), P(dst[2]), stream))
        run.keep = keep
        return run

    def torch_pass(code):
        perm, flips = S.perms(3)[code >> 3], [a + 1 for a in range(3) if (code >> a) & 1]

        def run():
            for t in src:
                v = t.view(n, s, s, s).permute(0, *[p + 1 for p in perm])
                (v.flip(flips) if flips else v).contiguous()
        return run

    def copy():
        for a, b in zip(src, dst):
            b.copy_(a)

    def time_all(variants):
        """{name: fn} -> {name: median ms per call}; the variants alternate inside every repeat."""
        for fn in variants.values():
            fn()
            fn()
        torch.cuda.synchronize()
        ms = {k: [] for k in variants}
        for _ in range(args.repeats):
            for k, fn in variants.items():
                a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                a.record()
                for _ in range(args.inner):
                    fn()
                b.record()
                b.synchronize()
                ms[k].append(a.elapsed_time(b) / args.inner)
        return {k: float(np.median(v)) for k, v in ms.items()}

    nbytes = 3 * n * V * 4 * 2
    rows, out = [], {"shape": "%d x %d^3 x 3 tensors" % (n, s), "bytes_moved": nbytes, "classes": {}}
    for name, codes in CLASSES:
        for code in codes:
            # the kernel is checked against torch's own pass on the tensors that are timed
            ours([code] * n)()
            want = src[0].view(n, s, s, s).permute(0, *[p + 1 for p in S.perms(3)[code >> 3]])
            flips = [a + 1 for a in range(3) if (code >> a) & 1]
            want = (want.flip(flips) if flips else want).contiguous().view(n, V)
            assert torch.equal(dst[0], want), "code %d: ursn_sym_apply differs from torch" % code
            t = time_all({"copy": copy, "ours": ours([code] * n), "torch": torch_pass(code)})
            rows.append((name, code, t["copy"], t["ours"], t["torch"]))
    mixed = S.draw(0, 0, 0, 0, n, list(range(48)))
    t = time_all({"copy": copy, "ours": ours(mixed)})
    rows.append(("mixed", -1, t["copy"], t["ours"], float("nan")))

    print("| class | code | copy ms | sym_apply ms | x copy | GB/s | torch ms | x copy |")
    print("|---|---|---|---|---|---|---|---|")
    for name, code, c, o, tt in rows:
        print("| %s | %s | %.3f | %.3f | %.2f | %.0f | %.3f | %.2f |" % (name, code if code >= 0 else "per event", c, o, o / c,
                                                                      nbytes / o / 1e6, tt, tt / c))
        out["classes"].setdefault(name, []).append({"code": code, "copy_ms": round(c, 4), "sym_apply_ms": round(o, 4),
                                                    "torch_ms": None if tt != tt else round(tt, 4),
                                                    "x_copy": round(o / c, 3), "torch_x_copy": None if tt != tt else round(tt / c, 3)})
    worst = {name: max(r[3] / r[2] for r in rows if r[0] == name) for name, _ in CLASSES}
    behind = [r for r in rows if r[4] == r[4] and r[3] > r[4]]
    out["worst_x_copy"] = {k: round(v, 3) for k, v in worst.items()}
    out["slower_than_torch"] = [r[1] for r in behind]

    # voxel feed: the expansion with and without the op
    ev = [sio.lartpc_sparse((s, s, s, 1), 3, e) for e in range(n)]
    vb = VoxelBatch.concat([sio.dense_to_voxels(e[0], e[1], np.full(V, 1.0 / V, np.float32) + (e[0].reshape(-1) != 0)) for e in ev])
    keep = {k: torch.from_numpy(getattr(vb, k)).to(dev) for k in ("offsets", "index", "value", "label", "weight", "bg_weight")}
    b = _lib.ursn_voxel_batch()
    b.n, b.voxels = n, V
    for k, tns in keep.items():
        setattr(b, k, tns.data_ptr())
    sp = (ctypes.c_int32 * 3)(s, s, s)
    ops = (ctypes.c_int32 * n)(*S.draw(1, 0, 0, 0, n, list(range(48))))

    def plain():
        _lib.check(lib.ursn_voxels_to_dense(ctypes.byref(b), P(dst[0]), P(dst[1]), P(dst[2]), stream))

    def sym():
        _lib.check(lib.ursn_voxels_to_dense_sym(ctypes.byref(b), 3, sp, ops, P(dst[0]), P(dst[1]), P(dst[2]), stream))
    t = time_all({"plain": plain, "sym": sym})
    out["voxels"] = {"entries": int(vb.offsets[-1]), "voxels_to_dense_ms": round(t["plain"], 4),
                     "voxels_to_dense_sym_ms": round(t["sym"], 4), "ratio": round(t["sym"] / t["plain"], 3)}
    print("\nvoxels_to_dense %.3f ms, voxels_to_dense_sym %.3f ms (x %.3f), %d list entries"
          % (t["plain"], t["sym"], t["sym"] / t["plain"], int(vb.offsets[-1])))
    print(json.dumps(out))
    return 1 if behind else 0


if __name__ == "__main__":
    sys.exit(main())
