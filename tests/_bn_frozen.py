"""Helpers of the frozen-BatchNorm training tests (test_bn_frozen_host.py, test_bn_frozen_gpu.py).

Reference derivative: the numpy oracle with bn_fwd swapped for the given-statistics version (the idiom of
tests/test_bn_moving_gpu.py::frozen_oracle) and bn_bwd swapped for  dz = r * dy, dbeta = sum dy  -- both inside the caller, in TF
variable order.  O.step_gradients, O.QUANT and _net.fp32_noise_floor under the swap are then the frozen gradient, its bf16
emulation and its fp32 noise floor.

Run as a program (`python _bn_frozen.py ROOT OUT.npz`) this file is the child of the A/B tests: URSN_BN_FROZEN_FUSED is read once
per process, so the single-pass kernels and the reduce / zero-mean finalise / apply route are compared across two processes that
run the same op-level variants and the same full-depth steps and store every result."""
import contextlib
import ctypes
import os
import sys

import numpy as np

S2D = ("golden2d", (32, 32, 1), 4, 3, 3, 3)        # tag, dims, F, classes, num_strides, batch
S3D = ("golden3d", (16, 16, 16, 1), 4, 3, 2, 3)
FULL = ("full3d_f8_ns5", (32, 32, 32, 1), 8, 3, 5, 2)
PAD = ("2d_f6_pad_lanes", (64, 64, 1), 6, 3, 3, 3)
CASES = [(S2D, "fp32"), (S3D, "fp32"), (FULL, "fp32"), (FULL, "bf16"), (PAD, "fp32")]
IDS = ["%s-%s" % (c[0][0], c[1]) for c in CASES]
EPS = 1e-3
SEED_CALIB, SEED_STEP = 51, 52


def bn_scopes(ndim, cin, base, ncls, ns):
    from oracle import uresnet_np as O
    return [l["name"] for l in O.layer_table(ndim, cin, base, ncls, num_strides=ns)]


@contextlib.contextmanager
def frozen_step_oracle(scopes, stats):
    """oracle.uresnet_np with BatchNorm on FIXED statistics, forward and backward.  stats: get_bn_moving()'s dict."""
    from oracle import uresnet_np as O
    fwd0, bwd0, order = O.bn_fwd, O.bn_bwd, iter(scopes)

    def bn_fwd(z, beta, eps=O.BN_EPS):
        s = next(order)
        m = stats[s + "/BatchNorm/moving_mean"].astype(z.dtype)
        v = stats[s + "/BatchNorm/moving_variance"].astype(z.dtype)
        assert z.shape[-1] == m.size, s
        r = (1.0 / np.sqrt(v + z.dtype.type(eps))).astype(z.dtype)
        xhat = (z - m) * r
        return xhat + beta, (xhat, r)

    O.bn_fwd = bn_fwd
    O.bn_bwd = lambda cache, dy: (cache[1] * dy, dy.sum(axis=tuple(range(dy.ndim - 1))))
    try:
        yield
    finally:
        O.bn_fwd, O.bn_bwd = fwd0, bwd0
    assert next(order, None) is None, "the oracle did not normalise every layer"


def oracle_frozen_step(P, shape, stats, data, label, weight, quant=False, noise_floor=False):
    """(gradients, metrics) of one frozen step: fp64, its bf16 emulation (quant), or the independent fp32 evaluation."""
    from oracle import uresnet_np as O
    from _net import fp32_noise_floor
    tag, dims, base, ncls, ns, n = shape
    scopes = bn_scopes(len(dims) - 1, dims[-1], base, ncls, ns)
    O.QUANT = O.bf16_round if quant else None
    try:
        with frozen_step_oracle(scopes, stats):
            if noise_floor:
                return fp32_noise_floor(P, dims, base, data, label, weight, num_strides=ns)
            return O.step_gradients(P, dims, base, data, label, weight, num_strides=ns)
    finally:
        O.QUANT = None


def batch_statistics(P, shape, data):
    """Another batch's batch statistics in get_bn_moving()'s layout, from the fp64 oracle (host tests: no device to calibrate on)."""
    from oracle import uresnet_np as O
    tag, dims, base, ncls, ns, n = shape
    scopes, seen, orig = bn_scopes(len(dims) - 1, dims[-1], base, ncls, ns), [], O.bn_fwd

    def bn_fwd(z, beta, eps=O.BN_EPS):
        ax = tuple(range(z.ndim - 1))
        seen.append((z.mean(axis=ax), z.var(axis=ax)))
        return orig(z, beta, eps)
    O.bn_fwd = bn_fwd
    try:
        O.forward(P, O.reshape_inputs(dims, data)[0].astype(np.float64), base, num_strides=ns)
    finally:
        O.bn_fwd = orig
    assert len(seen) == len(scopes)
    out = {}
    for s, (m, v) in zip(scopes, seen):
        out[s + "/BatchNorm/moving_mean"] = m.astype(np.float32)
        out[s + "/BatchNorm/moving_variance"] = v.astype(np.float32)
    return out


@contextlib.contextmanager
def torch_fixed_bn(scopes, stats):
    """oracle.uresnet_torch.forward with `bn` swapped for the fixed-statistics layer: autograd then differentiates through
    constants, with no hand-written backward anywhere."""
    import torch
    from oracle import uresnet_torch as T
    orig, order = T.bn, iter(scopes)

    def bn(z, beta, eps=T.BN_EPS):
        s = next(order)
        shape = [1, -1] + [1] * (z.dim() - 2)
        m = torch.as_tensor(stats[s + "/BatchNorm/moving_mean"]).to(z.dtype).view(shape)
        v = torch.as_tensor(stats[s + "/BatchNorm/moving_variance"]).to(z.dtype).view(shape)
        return (z - m) * torch.rsqrt(v + eps) + beta.view(shape)
    T.bn = bn
    try:
        yield
    finally:
        T.bn = orig
    assert next(order, None) is None


def torch_frozen_step(P, shape, stats, data, label, weight, dlogits=None):
    """fp64 torch autograd: (parameter gradients, d data, loss).  dlogits given: the vector-Jacobian product with it instead of
    the head's loss."""
    import torch
    from oracle import uresnet_torch as T
    tag, dims, base, ncls, ns, n = shape
    scopes = bn_scopes(len(dims) - 1, dims[-1], base, ncls, ns)
    Pt = T.params_from_numpy(P)
    d = torch.as_tensor(np.asarray(data, np.float64).reshape((-1,) + tuple(dims))).requires_grad_(True)
    with torch_fixed_bn(scopes, stats):
        logits = T.forward(Pt, d, base, num_strides=ns)
    if dlogits is None:
        l = torch.as_tensor(label).reshape((-1,) + tuple(dims[:-1]))
        w = None if weight is None else torch.as_tensor(np.asarray(weight, np.float64)).reshape((-1,) + tuple(dims[:-1]))
        loss = T.loss_fn(logits, l, w)
    else:
        loss = (logits * torch.as_tensor(np.asarray(dlogits, np.float64))).sum()
    grads = torch.autograd.grad(loss, list(Pt.values()) + [d])
    return ({k: g.numpy() for k, g in zip(Pt.keys(), grads[:-1])}, grads[-1].numpy(), float(loss.item()))


# ---- device side ---------------------------------------------------------------------------------------------------------------
def build_net(shape, prec, lr=1e-2, bn_moving=True):
    from uresnet_amd import uresnet
    tag, dims, base, ncls, ns, n = shape
    net = uresnet(dims=list(dims), num_class=ncls, base_num_outputs=base, num_strides=ns)
    net.construct(trainable=True, use_weight=True, learning_rate=lr, seed=7, precision=prec, bn_moving=bn_moving, bn_decay=0.9)
    return net


def calibrated_net(shape, prec, lr=1e-2):
    """(net in 'frozen' mode, oracle parameters, moving statistics calibrated on ANOTHER batch -- the network is alive)."""
    from _net import as_f32_exact, make_inputs, oracle_params
    tag, dims, base, ncls, ns, n = shape
    P = as_f32_exact(oracle_params(dims, base, ncls, num_strides=ns))
    net = build_net(shape, prec, lr)
    net.set_variables(P)
    assert net.bn_calibrate(None, [make_inputs(dims, ncls, n, seed=SEED_CALIB)[0]]) == 1
    stats = net.get_bn_moving()
    net.set_bn_mode('frozen')
    return net, P, stats


def pass5_kernels(net, call):
    """Names of the BatchNorm-backward launches (profiler pass id 5) that `call` makes, with their byte counts."""
    from uresnet_amd import _lib
    lib = _lib.load()
    _lib.check(lib.ursn_profile_enable(net._handle, 1))
    call()
    cnt = ctypes.c_int64(0)
    _lib.check(lib.ursn_profile_read(net._handle, None, 0, ctypes.byref(cnt)))
    recs = (_lib.ursn_prof_rec * max(int(cnt.value), 1))()
    _lib.check(lib.ursn_profile_read(net._handle, recs, int(cnt.value), ctypes.byref(cnt)))
    _lib.check(lib.ursn_profile_enable(net._handle, 0))
    return [(r.kernel.decode(), float(r.bytes)) for r in recs[:int(cnt.value)] if int(r.pass_) == 5]


# ---- op level ------------------------------------------------------------------------------------------------------------------
F32_C, F32_V, F32_RELU = (4, 6, 8, 16, 64), (1, 255, 256, 257 * 3), ("none", "y", "z")
BF_C, BF_V = (8, 16, 64), 2 * 1024 + 257 * 3
BF_FORMS = ("plain", "join2", "dres_set", "dres_acc")      # + "dy2" at C = 8, mask bn(z) > 0
GUARD = 64


def _clear_of_zero(z, mean, rstd, beta):
    """Moves the elements whose bn(z) lies within 1e-2 of 0 away from it: the mask bn(z) > 0 then does not hang on the last bit
    of the device's fmaf."""
    t = (z - mean) * rstd + beta
    return np.where(np.abs(t) < 1e-2, z + 1.0 / rstd, z)


def f32_case(C, V, relu):
    rng = np.random.default_rng(1000 * C + V + len(relu))
    mean = rng.normal(0.0, 0.3, C).astype(np.float32)
    rstd = (1.0 / np.sqrt(rng.uniform(0.2, 2.0, C) + EPS)).astype(np.float32)
    beta = rng.normal(0.0, 0.3, C).astype(np.float32)
    z = _clear_of_zero(rng.standard_normal((V, C)) * 1.5 + 0.3, mean.astype(np.float64), rstd.astype(np.float64), beta.astype(np.float64))
    z = z.astype(np.float32)
    y = rng.standard_normal((V, C)).astype(np.float32)
    dy = rng.standard_normal((V, C)).astype(np.float32)
    if relu == "none":
        g = dy
    elif relu == "y":
        g = dy * (y > 0)
    else:
        t = (z.astype(np.float64) - mean) * rstd.astype(np.float64) + beta
        assert np.abs(t).min() > 1e-3
        g = dy * (t > 0)
    return dict(mean=mean, rstd=rstd, beta=beta, z=z, y=y, dy=dy, g=g.astype(np.float32))


def run_f32_op(C, V, relu):
    """-> dz with GUARD floats behind it, dbeta with GUARD floats behind it (both started as NaN / 0 | NaN)."""
    import torch
    from uresnet_amd import _lib
    lib, c = _lib.load(), f32_case(C, V, relu)
    dev = {k: torch.from_numpy(v).cuda() for k, v in c.items() if k != "g"}
    dz = torch.full((V * C + GUARD,), float("nan"), dtype=torch.float32, device="cuda")
    db = torch.full((C + GUARD,), float("nan"), dtype=torch.float32, device="cuda")
    db[:C] = 0.0
    nb = lib.ursn_bn_scratch_bytes(V, C)
    scratch = torch.full((nb,), 0xFF, dtype=torch.uint8, device="cuda")      # NaN-filled: nothing is read that the call did not write
    P = lambda t: ctypes.c_void_p(t.data_ptr())
    _lib.check(lib.ursn_bn_backward_frozen(P(dev["dy"]), P(dev["y"]) if relu == "y" else None, P(dev["z"]), P(dev["mean"]),
                                           P(dev["rstd"]), P(dev["beta"]), P(dz), P(db), V, C, int(relu != "none"), P(scratch), nb,
                                           None))
    torch.cuda.synchronize()
    return dz.cpu().numpy(), db.cpu().numpy()


def bf_round(a):
    """fp32 values rounded once to bf16 (round to nearest even), as fp32."""
    from oracle import uresnet_np as O
    return O.bf16_round(np.asarray(a, np.float32))


def mask_bytes(y):
    m = (y.reshape(-1, y.shape[-1] // 8, 8) > 0).astype(np.uint8)
    return (m << np.arange(8, dtype=np.uint8)).sum(axis=-1).astype(np.uint8)


def bf_case(C, mask, form):
    V = BF_V
    rng = np.random.default_rng(7000 + 100 * C + 10 * mask + len(form))
    mean = rng.normal(0.0, 0.3, C).astype(np.float32)
    rstd = (1.0 / np.sqrt(rng.uniform(0.2, 2.0, C) + EPS)).astype(np.float32)
    rstd2 = (1.0 / np.sqrt(rng.uniform(0.2, 2.0, C) + EPS)).astype(np.float32)
    beta = rng.normal(0.0, 0.3, C).astype(np.float32)
    z = bf_round(rng.standard_normal((V, C)) * 1.5 + 0.3)
    for _ in range(4):      # bf16-representable z whose bn(z) stays clear of 0
        z = bf_round(_clear_of_zero(z.astype(np.float64), mean.astype(np.float64), rstd.astype(np.float64), beta.astype(np.float64)))
    y = bf_round(rng.standard_normal((V, C)))
    dy, dy2 = bf_round(rng.standard_normal((V, C))), bf_round(rng.standard_normal((V, C)))
    base = bf_round(rng.standard_normal((V, C)))
    g = (dy + dy2).astype(np.float32) if form == "dy2" else dy
    if mask in (1, 3):
        g = g * (y > 0)
    elif mask == 2:
        t = (z.astype(np.float64) - mean) * rstd.astype(np.float64) + beta
        assert np.abs(t).min() > 1e-3
        g = g * (t > 0)
    return dict(mean=mean, rstd=rstd, rstd2=rstd2, beta=beta, z=z, y=y, dy=dy, dy2=dy2, base=base, g=g.astype(np.float32))


def run_bf_op(C, mask, form):
    """-> dict of fp32 arrays: dz, dbeta (+ dz2, dbeta2 | dres), every bf16 output with GUARD elements behind it."""
    import torch
    from uresnet_amd import _lib
    lib, c, V = _lib.load(), bf_case(C, mask, form), BF_V
    f32 = lambda a: torch.from_numpy(np.ascontiguousarray(a, np.float32)).cuda()
    b16 = lambda a: f32(a).to(torch.bfloat16)
    keep = dict(mean=f32(c["mean"]), rstd=f32(c["rstd"]), rstd2=f32(c["rstd2"]), beta=f32(c["beta"]), z=b16(c["z"]), y=b16(c["y"]),
                dy=b16(c["dy"]), dy2=b16(c["dy2"]), mk=torch.from_numpy(mask_bytes(c["y"])).cuda())
    out = lambda: torch.full((V * C + GUARD,), float("nan"), dtype=torch.bfloat16, device="cuda")
    d = _lib.ursn_bn_bf16_desc()
    d.voxels, d.channels, d.relu = V, C, int(mask != 0)
    d.z, d.mean, d.rstd, d.beta = keep["z"].data_ptr(), keep["mean"].data_ptr(), keep["rstd"].data_ptr(), keep["beta"].data_ptr()
    d.dy = keep["dy"].data_ptr()
    if mask == 1:
        d.y = keep["y"].data_ptr()
    if mask == 3:
        d.mask = keep["mk"].data_ptr()
    res = {"dz": out(), "dbeta": torch.zeros(C, device="cuda")}
    d.dz, d.dbeta = res["dz"].data_ptr(), res["dbeta"].data_ptr()
    if form == "dy2":
        d.dy2 = keep["dy2"].data_ptr()
    if form == "join2":
        res["dz2"], res["dbeta2"] = out(), torch.zeros(C, device="cuda")
        d.z2, d.mean2, d.rstd2 = keep["z"].data_ptr(), keep["mean"].data_ptr(), keep["rstd2"].data_ptr()
        d.dz2, d.dbeta2 = res["dz2"].data_ptr(), res["dbeta2"].data_ptr()
    if form in ("dres_set", "dres_acc"):
        res["dres"] = out()
        res["dres"][:V * C] = b16(c["base"]).reshape(-1)
        d.dres, d.dres_accumulate = res["dres"].data_ptr(), int(form == "dres_acc")
    nb = lib.ursn_bn_bf16_scratch_bytes(V, C)
    scratch = torch.full((nb,), 0xFF, dtype=torch.uint8, device="cuda")
    _lib.check(lib.ursn_bn_bf16_backward_frozen(ctypes.byref(d), ctypes.c_void_p(scratch.data_ptr()), nb, None))
    torch.cuda.synchronize()
    return {k: v.float().cpu().numpy() for k, v in res.items()}


def bf_variants():
    v = [(C, mask, form) for C in BF_C for mask in (0, 1, 2, 3) for form in BF_FORMS]
    return v + [(8, 2, "dy2")]


def net_step(shape, prec):
    """One frozen accum_gradients at the full-depth shape: loss, gradients, and the pass-5 launches it made."""
    from _net import make_inputs
    tag, dims, base, ncls, ns, n = shape
    net, P, stats = calibrated_net(shape, prec)
    data, label, weight = make_inputs(dims, ncls, n, seed=SEED_STEP)
    net.zero_gradients(None)
    res = []
    kern = pass5_kernels(net, lambda: res.append(net.accum_gradients(None, data, label, weight)[0]))
    return res[0][1], net.get_gradients(), kern


def _child(out_path):
    res = {}
    for C in F32_C:
        for V in F32_V:
            for relu in F32_RELU:
                dz, db = run_f32_op(C, V, relu)
                res["f32|%d|%d|%s|dz" % (C, V, relu)], res["f32|%d|%d|%s|dbeta" % (C, V, relu)] = dz, db
    for C, mask, form in bf_variants():
        for k, v in run_bf_op(C, mask, form).items():
            res["bf|%d|%d|%s|%s" % (C, mask, form, k)] = v
    for prec in ("fp32", "bf16"):
        loss, g, kern = net_step(FULL, prec)
        res["net|%s|loss" % prec] = np.float64(loss)
        res["net|%s|kernels" % prec] = np.array(sorted(set(k for k, _ in kern)))
        for k, v in g.items():
            res["net|%s|g|%s" % (prec, k.replace("/", "!"))] = v
    np.savez(out_path, **res)


if __name__ == "__main__":
    sys.path.insert(0, sys.argv[1])
    sys.path.insert(0, os.path.join(sys.argv[1], "tests"))
    _child(sys.argv[2])
