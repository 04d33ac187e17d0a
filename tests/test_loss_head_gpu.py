"""Device loss head on the GPU: ursn_loss_head between NaN guard bands against losses.loss_numpy (the fp64 oracle, itself checked
against torch autograd in tests/test_loss_head_host.py), the neutral spec against the heads bit for bit, and the net-level calls
through ssnet_base on both plans.

Bounds.  Loss and terms: relative 1e-5; accuracies 1e-6; fp32 dlogits: 1e-5 of the tensor's max -- what tests/test_ops_gpu.py holds
ursn_softmax_ce to.  bf16 dlogits: each stored value within one bf16 ulp of the bf16 rounding of the fp64 value.  Where a value
misses that (a d-logit whose terms cancel: with smoothing, q_k meets smoothing / C somewhere in every large case) the issue's
procedure applies: a float32 restatement of the kernel's statements in numpy (_restate32), and 4 x the restatement's own deviation
from fp64 allowed -- the deviation in the issue's metric, the largest over a tensor, here narrowed to the lanes of the value's own
voxel.  It is not taken at the single element: two independent fp32 evaluations of a cancelling sum err by amounts whose ratio at
one element is heavy-tailed.  The two values of the matrix's 11.9 million that need the allowance (one lane of one voxel, with and
without a weight) show it (4099 x 3 voxels, 5 classes, bf16,
BatchNorm operands, gamma 2 + smoothing 0.1; label lane -0.336, this lane f (q - s/C) + h q = -0.0050 + 0.0050): fp64 6.5571e-08, the
kernel 6.6590e-08 (2 bf16 ulps), the restatement 6.5969e-08 (1 ulp, by a hair); deviations 1.0e-09 and 4.0e-10, the restatement's
over the voxel 6.3e-08.  Every such value is printed with these figures and DESIGN.md records the count.  One exception, forced by the neutral spec having to BE the head: the head
forms the label lane as w/n * (q_l - 1) with q_l rounded to fp32, so where q_l is within an ulp of 1 (the gap-30 voxel every case
holds) no statement that is bit-equal to the head's can know that lane better than w/n * 2^-23; under the neutral spec only, a
stored value may therefore also lie within that absolute distance of the fp64 value.  Every other spec is held to the ulp bound
at that voxel too (the kernel forms 1 - q_l from the other classes' terms).
Net level: two paths that share a forward are held to l2_rel <= 1e-3 on the fp32 plan (tests/test_ext_loss_gpu.py).  On the bf16
plan that file's bound is 4 x a figure measured for two paths that round the SAME fp32 expression (0: bit-equal); the loss head and
torch evaluate different fp32 expressions of one gradient, which agree to ~1e-6 and so round to the same or to adjacent bf16
values, and one flipped rounding moves a bf16 backward on these shapes by 1-2e-2 per tensor (measured between two runs of the
custom path itself, torch's loss in fp32 against fp64).  So the head is separated from the backward's sensitivity: every stored
d-logit within one bf16 ulp of the custom path's; where none differs, bit-equal gradients; and on BOTH plans the step's own stored
d-logits, replayed through forward_logits / backward_logits, must give the step's gradient buffer bit for bit (partials included).
Gradients against the oracle follow tests/test_net_gpu.py::
test_accum_gradients_parity (4 x the fp32 oracle's own deviation, at least 2e-3, never above 5e-2)."""
import ctypes

import numpy as np
import pytest
import torch

from oracle import uresnet_np as O
import _bn_frozen as B
from _abi import Handle, bits, make_cfg, same_bits, upload
from _guard import Guarded
from _loss_cases import BATCHES, CLASSES, SPEC_IDS, SPECS, VOXELS, make_case, rel_err
from _net import as_f32_exact, l2_rel, make_inputs, oracle_params
from uresnet_amd import _lib, uresnet
from uresnet_amd.losses import LossSpec, loss_numpy, loss_torch
from uresnet_amd.ssnet import VoxelBatch

pytestmark = pytest.mark.gpu


def _layouts(ncls):
    lay = [("fp32", ncls), ("fp32", 8), ("bf16", 8)]
    if ncls <= 4:
        lay.append(("fp32", 4))
    return [l for i, l in enumerate(lay) if l not in lay[:i]]


def _head_blocks(P):
    return max(1, min(4096, (P + 1023) // 1024))


def _desc_of(spec):
    return _lib.ursn_loss_desc(spec.gamma, spec.smoothing, spec.dice_weight, spec.dice_eps, spec.ignore_label)


class OpCase(object):
    """Operands of one op-level call, every one between NaN borders.  `logits` (fp32-exact) are what the kernel is to see without
    BatchNorm operands; with them the stored z is (logits - beta) / rstd + mean and `seen` is recomputed from what was stored."""

    def __init__(self, z, data, label, weight, layout, with_bn, use_w, seed=0, out_layout=None):
        n, vox, ncls = z.shape
        P = n * vox
        dt, cs = layout
        self.n, self.vox, self.ncls, self.P, self.dt, self.cs = n, vox, ncls, P, dt, cs
        self.odt, self.ocs = out_layout if out_layout else layout
        rng = np.random.default_rng(1000 + seed)
        raw = z.reshape(P, ncls).astype(np.float64)
        self.mean = self.rstd = self.beta = None
        if with_bn:
            mean, rstd, beta = rng.standard_normal(8), rng.uniform(0.5, 2.0, 8), rng.standard_normal(8)
            mean, rstd, beta = (a.astype(np.float32) for a in (mean, rstd, beta))
            raw = (raw - beta[:ncls]) / rstd[:ncls] + mean[:ncls]
            self.mean, self.rstd, self.beta = (Guarded((8,), torch.float32, a) for a in (mean, rstd, beta))
        stored = np.full((P, cs), 7.0e37, np.float32)   # pad lanes hold a large finite value: they must not reach any sum
        stored[:, :ncls] = raw.astype(np.float32)
        if dt == "bf16":
            stored = O.bf16_round(stored)
            self.z = Guarded((P, cs), torch.bfloat16, torch.from_numpy(stored))
        else:
            self.z = Guarded((P, cs), torch.float32, stored)
        seen = stored[:, :ncls].astype(np.float64)
        if with_bn:
            # the logits the kernel sees are fp32: fma(z, rstd, beta - mean * rstd), the statement ursn_logits_dense writes out
            # (tests/test_ext_loss_gpu.py holds it to the fp64 value); an fp64 evaluation from z would differ in the last fp32 bit
            d = _lib.ursn_vscores_desc()
            d.n, d.voxels, d.ncls, d.z, d.z_cstride, d.dtype = n, vox, ncls, self.z.ptr, cs, int(dt == "bf16")
            d.mean, d.rstd, d.beta = self.mean.ptr, self.rstd.ptr, self.beta.ptr
            dense = torch.empty((P, ncls), dtype=torch.float32, device="cuda")
            _lib.check(_lib.load().ursn_logits_dense(ctypes.byref(d), ctypes.c_void_p(dense.data_ptr()), None))
            torch.cuda.synchronize()
            ref = (seen - mean[:ncls].astype(np.float64)) * rstd[:ncls].astype(np.float64) + beta[:ncls].astype(np.float64)
            seen = dense.cpu().numpy().astype(np.float64)
            assert rel_err(seen, ref) <= 2e-5
        self.seen = seen.reshape(n, vox, ncls)
        self.raw = stored[:, :ncls].astype(np.float64)
        self.data_h, self.label_h, self.weight_h = data, label, (weight if use_w else None)
        self.data = Guarded((n, vox), torch.float32, data)
        self.label = Guarded((n, vox), torch.float32, label)
        self.weight = Guarded((n, vox), torch.float32, weight) if use_w else None
        self.want_bs = with_bn and self.odt == dt and (dt == "bf16" or (cs == 4 and ncls <= 4))
        self.BC = 8 if dt == "bf16" else 4

    def run(self, lib, spec, fill=0xFF, want_out=True, scratch_short=0):
        """One call.  Returns (out8 [8] fp32, raw bytes of the dlogits payload or None, partials [blocks, 3, C] or None)."""
        out = Guarded((self.P, self.ocs), torch.bfloat16 if self.odt == "bf16" else torch.float32) if want_out else None
        out8 = Guarded((8,), torch.float32)
        need = lib.ursn_loss_head_scratch_bytes(self.n, self.vox, self.ncls)
        assert need > 0
        scratch = Guarded((need,), torch.uint8).fill(fill)
        nb = _head_blocks(self.P)
        bs = Guarded((nb, 3, self.BC), torch.float64) if (self.want_bs and want_out) else None
        d = _lib.ursn_vscores_desc()
        d.n, d.voxels, d.ncls, d.z, d.z_cstride, d.dtype = self.n, self.vox, self.ncls, self.z.ptr, self.cs, int(self.dt == "bf16")
        if self.mean is not None:
            d.mean, d.rstd, d.beta = self.mean.ptr, self.rstd.ptr, self.beta.ptr
        d.data = self.data.ptr
        sd = _desc_of(spec)
        P = ctypes.c_void_p
        rc = lib.ursn_loss_head(ctypes.byref(d), P(self.label.ptr), P(self.weight.ptr) if self.weight else None, ctypes.byref(sd),
                                P(out.ptr) if out else None, self.ocs, int(self.odt == "bf16"), P(bs.ptr) if bs else None,
                                nb if bs else 0, P(out8.ptr), P(scratch.ptr), need - scratch_short, None)
        if scratch_short:
            return rc
        _lib.check(rc)
        torch.cuda.synchronize()
        what = "loss_head n %d vox %d ncls %d %s/%d -> %s/%d" % (self.n, self.vox, self.ncls, self.dt, self.cs, self.odt, self.ocs)
        for g, name in ((self.z, "z"), (self.mean, "mean"), (self.rstd, "rstd"), (self.beta, "beta"), (self.data, "data"),
                        (self.label, "label"), (self.weight, "weight"), (out, "dlog_out"), (out8, "out8"), (scratch, "scratch"),
                        (bs, "partials")):
            if g is not None:
                g.check("%s: %s" % (what, name))
        self.last_out = out
        return (out8.numpy().copy(), out.bytes.cpu().numpy().copy() if out else None, bs.numpy().copy() if bs else None)

    def dlogits_of(self, raw_bytes):
        """Stored payload -> ([P, stride] fp32 values, bf16 widened)."""
        if self.odt == "bf16":
            u = raw_bytes.view(np.uint16).astype(np.uint32) << 16
            return u.view(np.float32).reshape(self.P, 8)
        return raw_bytes.view(np.float32).reshape(self.P, self.ocs)


def _bf16_ulp(r):
    a = np.maximum(np.abs(r), 2.0 ** -126)
    return 2.0 ** (np.floor(np.log2(a)) - 7)


def _restate32(c, spec):
    """The kernel's statements for a spec other than the neutral one, restated in numpy float32 on the logits the kernel sees (same
    forms: 1 - q_l from the other classes' terms, log1p for -log q_l, the Dice gradient as q_k sum_j q_j (r_k - r_j)); the Dice
    coefficients come from fp64 sums, as the finalise forms them.  Not a bit copy (numpy's exp / log, pairwise sums): an independent
    fp32 evaluation whose own deviation from fp64 measures what fp32 can know of a d-logit."""
    f32 = np.float32
    C, n = c.ncls, c.n
    z = c.seen.reshape(c.P, C).astype(f32)
    lab = np.trunc(c.label_h.reshape(-1)).astype(np.int64)
    w = (np.ones(c.P, f32) if c.weight_h is None else c.weight_h.reshape(-1).astype(f32))
    ign = (lab == spec.ignore_label) if spec.ignore_label != -1 else np.zeros(c.P, bool)
    onehot = (np.arange(C)[None, :] == lab[:, None])
    m = z.max(-1, keepdims=True)
    e = np.exp(z - m)
    ssum = e.sum(-1)
    inv = f32(1) / ssum
    el, eo = (e * onehot).sum(-1), (e * ~onehot).sum(-1)
    om, ql = eo * inv, el * inv
    lg = np.log(ssum)
    zl = (z * onehot).sum(-1)
    with np.errstate(divide='ignore', invalid='ignore'):
        cel = np.where(eo < f32(0.5) * el, np.log1p(eo / np.where(el > 0, el, f32(1))), lg - (zl - m[:, 0]))
    sm = f32(spec.smoothing)
    ce = cel
    if spec.smoothing > 0:
        ce = (f32(1) - sm) * cel + sm * (lg - (z - m).sum(-1) / f32(C))
    gam = f32(spec.gamma)
    if spec.gamma == 0:
        fm1, f = np.zeros(c.P, f32), np.ones(c.P, f32)
    else:
        with np.errstate(divide='ignore', invalid='ignore'):
            fm1 = np.ones(c.P, f32) if spec.gamma == 1 else om if spec.gamma == 2 else np.where(om > 0, np.exp((gam - f32(1)) * np.log(om)), f32(0))
        f = fm1 * om
    h = gam * fm1 * ql * ce
    wn = w * (f32(1) / f32(n))
    soc = sm / f32(C)
    q = e * inv[:, None]
    dce = np.where(onehot, (f * (sm - soc - om) - h * om)[:, None], f[:, None] * (q - soc) + h[:, None] * q)
    g = wn[:, None] * dce
    if spec.dice_weight > 0:
        q64 = q.astype(np.float64) * (~ign)[:, None]
        I, S, Y = (q64 * onehot).sum(0), q64.sum(0), (onehot & ~ign[:, None]).sum(0).astype(np.float64)
        U = S + Y + spec.dice_eps
        a, b = (-2.0 / (C * U)).astype(f32), ((2.0 * I + spec.dice_eps) / (C * U * U)).astype(f32)
        r = b[None, :] + np.where(onehot, a[None, :], f32(0))
        dk = (q[:, None, :] * (r[:, :, None] - r[:, None, :])).sum(-1)
        g = g + (f32(spec.dice_weight) * q) * dk
    g = np.where(ign[:, None], f32(0), g)
    assert g.dtype == np.float32
    return g


ALLOWANCE = {"values": 0, "checked": 0, "worst_ratio": 0.0}   # bf16 values that took the restatement allowance, over the whole run


def _check_against_oracle(c, spec, out8, got, bs, what):
    ref = loss_numpy(c.seen, c.data_h, c.label_h, c.weight_h, spec)
    for name, v, r in (("loss", out8[0], ref["loss"]), ("ce_term", out8[4], ref["ce_term"]), ("dice_term", out8[5], ref["dice_term"])):
        assert abs(float(v) - r) <= 1e-5 * abs(r) + 1e-30, (what, name, float(v), r)
    assert abs(float(out8[1]) - ref["acc_all"]) < 1e-6, (what, out8[1], ref["acc_all"])
    if np.isnan(ref["acc_nonzero"]):
        assert np.isnan(out8[2]), what
    else:
        assert abs(float(out8[2]) - ref["acc_nonzero"]) < 1e-6, (what, out8[2], ref["acc_nonzero"])
    assert float(out8[3]) == float((c.data_h > 0).sum()) and out8[6] == 0 and out8[7] == 0, what
    assert np.isfinite(out8[[0, 1, 3, 4, 5]]).all(), what
    g = ref["dlogits"].reshape(c.P, c.ncls)
    vals = got[:, :c.ncls]
    assert np.isfinite(vals).all(), what   # nothing left unwritten (the payload was NaN), no NaN out
    err = 0.0
    if c.odt == "bf16":
        assert (got[:, c.ncls:] == 0).all() and not np.signbit(got[:, c.ncls:]).any(), what + ": bf16 pad lanes must be +0"
        want = O.bf16_round(g.astype(np.float32)).astype(np.float64)
        dev = np.abs(vals.astype(np.float64) - want)
        ulp = _bf16_ulp(np.maximum(np.abs(g), np.abs(want)))   # a rounding up into the next binade is followed by that binade's step
        ok = dev <= ulp
        ALLOWANCE["checked"] += ok.size
        if spec.neutral:   # see the head of the file
            w = (np.ones(c.P) if c.weight_h is None else c.weight_h.reshape(-1).astype(np.float64)) / c.n
            ok |= np.abs(vals.astype(np.float64) - g) <= (w * 2.0 ** -23)[:, None]
        elif not ok.all():
            # the issue's procedure for a bound fp32 cannot meet: a float32 restatement of the same statements, 4 x ITS deviation
            # from fp64 allowed.  The deviation is the issue's metric -- the largest over a tensor -- taken over the lanes of the
            # value's own voxel only (they share one softmax, ce and focal factor): see the head of the file
            rest = _restate32(c, spec).astype(np.float64)
            rdev = np.abs(rest - g)
            vdev = rdev.max(-1, keepdims=True)
            gdev = np.abs(vals.astype(np.float64) - g)
            allowed = ~ok & (gdev <= 4.0 * vdev)
            for i, k in np.argwhere(allowed):
                ALLOWANCE["values"] += 1
                ALLOWANCE["worst_ratio"] = max(ALLOWANCE["worst_ratio"], float(gdev[i, k] / vdev[i, 0]))
                print("    restatement allowance, %s: stored %.9g, fp64 %.9g (bf16 %.9g), float32 restatement %.9g: deviation %.3g, the "
                      "restatement's %.3g here and %.3g over the voxel" % (what, vals[i, k], g[i, k], want[i, k], rest[i, k], gdev[i, k],
                                                                          rdev[i, k], vdev[i, 0]))
            ok |= allowed
        assert ok.all(), (what, "%d values beyond one bf16 ulp" % int((~ok).sum()), float((dev / ulp).max()),
                          [(float(vals[i, k]), float(want[i, k]), float(g[i, k])) for i, k in np.argwhere(~ok)[:4]])
    else:
        if c.ocs == 4 and c.ncls <= 4:
            assert (bits(got[:, c.ncls:].copy()) == 0).all(), what + ": pad lanes of the 16-byte store must be +0"
        else:
            assert (bits(got[:, c.ncls:].copy()) == 0xFFFFFFFF).all(), what + ": pad lanes of a scalar-store layout were written"
        if np.abs(g).max() > 0:
            err = rel_err(vals, g)
            assert err < 1e-5, (what, err)
        else:
            assert np.abs(vals).max() == 0, what
    if bs is not None:   # from the STORED values, in fp64; third row zero
        sv = vals.astype(np.float64)
        mean, rstd = (x.numpy()[:c.ncls].astype(np.float64) for x in (c.mean, c.rstd))
        xhat = (c.raw - mean) * rstd
        tot = bs.sum(0)
        scale = np.abs(sv).sum(0) + 1e-300
        assert (np.abs(tot[0, :c.ncls] - sv.sum(0)) <= 1e-5 * scale).all(), what
        assert (np.abs(tot[1, :c.ncls] - (sv * xhat).sum(0)) <= 1e-5 * (np.abs(sv * xhat).sum(0) + 1e-300)).all(), what
        assert (bs[:, 2, :] == 0).all() and (tot[:2, c.ncls:] == 0).all(), what
    return err


# ---- 1. op level: the shape matrix against the oracle -----------------------------------------------------------------------
@pytest.mark.parametrize("spec", [s[1] for s in SPECS], ids=SPEC_IDS)
@pytest.mark.parametrize("ncls", CLASSES)
def test_loss_head_op(lib, ncls, spec):
    worst, cases = 0.0, 0
    for vox in VOXELS:
        for n in BATCHES:
            for with_bn in (False, True):
                z, data, label, weight = make_case(7 * vox + n + ncls, n, vox, ncls, ties=not with_bn)
                for li, layout in enumerate(_layouts(ncls)):
                    for use_w in (False, True):
                        c = OpCase(z, data, label, weight, layout, with_bn, use_w, seed=li)
                        what = "vox %d n %d ncls %d %s stride %d bn %s weight %s %s" % ((vox, n, ncls) + layout + (with_bn, use_w, spec))
                        out8, raw, bs = c.run(lib, spec, fill=0xFF)
                        worst = max(worst, _check_against_oracle(c, spec, out8, c.dlogits_of(raw), bs, what))
                        # the scratch needs no initialisation and the same arguments give the same bits
                        out8b, rawb, bsb = c.run(lib, spec, fill=0x00)
                        assert same_bits(out8, out8b) and np.array_equal(raw, rawb), what + ": a second call gave other bits"
                        assert bs is None or np.array_equal(bs.view(np.uint64), bsb.view(np.uint64)), what
                        cases += 1
    print("loss_head ncls %d %s: %d cases, worst fp32 dlogits error %.3g of max; bf16 values so far: %d checked, %d on the restatement "
          "allowance (worst stored / restatement deviation %.3g)" % (ncls, spec, cases, worst, ALLOWANCE["checked"], ALLOWANCE["values"],
                                                                     ALLOWANCE["worst_ratio"]))


def test_loss_only_and_scratch_size(lib):
    """dlog_out NULL: loss and metrics only, the same bits; a scratch 8 bytes short is refused before any launch."""
    for spec in (SPECS[3][1], SPECS[5][1]):
        z, data, label, weight = make_case(5, 3, 1025, 3)
        c = OpCase(z, data, label, weight, ("fp32", 4), True, True)
        full, _, _ = c.run(lib, spec)
        only, raw, bs = c.run(lib, spec, want_out=False)
        assert raw is None and bs is None and same_bits(full, only)
        rc = c.run(lib, spec, scratch_short=8)
        assert rc != 0 and b"scratch too small" in lib.ursn_last_error()


def test_invalid_and_ignored_labels(lib):
    z, data, label, weight = make_case(6, 2, 255, 3)
    label = label.copy()
    label[1, 7] = 5.0
    c = OpCase(z, data, label, weight, ("fp32", 4), False, True)
    out8, _, _ = c.run(lib, LossSpec(gamma=2.0))
    assert np.isnan(out8[0]) and np.isnan(out8[4])            # outside [0, C) and not ignored: NaN, as the head
    out8, raw, _ = c.run(lib, LossSpec(gamma=2.0, dice_weight=0.5, ignore_label=5))
    assert np.isfinite(out8[:6]).all()
    got = c.dlogits_of(raw)
    assert (got[255 + 7] == 0).all() and np.abs(got[255 + 8]).max() > 0   # an ignored voxel stores zeros
    ref = loss_numpy(c.seen, data, label, weight, LossSpec(gamma=2.0, dice_weight=0.5, ignore_label=5))
    assert abs(out8[0] - ref["loss"]) <= 1e-5 * abs(ref["loss"]) and rel_err(got[:, :3], ref["dlogits"].reshape(-1, 3)) < 1e-5


# ---- 2. op level: the neutral spec is the head, bit for bit -------------------------------------------------------------------
def _head(lib, z, data, label, weight):
    """ursn_softmax_ce on compact fp32 logits: (out3, dlogits [P, ncls])."""
    n, vox, ncls = z.shape
    zd, dd, ld = upload(z, data, label)
    wd = upload(weight)[0] if weight is not None else None
    dl = torch.full((n * vox, ncls), float("nan"), dtype=torch.float32, device="cuda")
    scratch = torch.empty(1 << 20, dtype=torch.uint8, device="cuda")
    out = (ctypes.c_float * 3)()
    p = lambda t: ctypes.c_void_p(t.data_ptr()) if t is not None else None
    _lib.check(lib.ursn_softmax_ce(p(zd), p(dd), p(ld), p(wd), n, vox, ncls, None, p(dl), out, p(scratch), 1 << 20, None))
    return np.array(list(out), np.float32), dl


@pytest.mark.parametrize("ncls", CLASSES)
def test_neutral_spec_is_the_head_op(lib, ncls):
    """fp32 layouts: dlogits and out8[0..2] carry the bits of ursn_softmax_ce (out8[3], which that call does not return, is the exact
    count).  bf16 output: the bits of ursn_dlogits_pack fed the head's own dlogits -- with fp32 logits in, where the kernel takes
    head_kernel's expf / logf.  With bf16 z in it takes bhead_kernel's fast __expf / __logf instead (that is what makes the bf16
    PLAN's step bit-equal, checked at net level below), so against the fp32 head's packed dlogits those bits may differ by a bf16
    rounding: held to one bf16 ulp, the count printed.  The BatchNorm-backward partials have no op-level call of the heads to be
    compared with: test_neutral_step_is_the_step compares the whole gradient buffer they feed."""
    spec = LossSpec()
    flips = total = 0
    for vox in VOXELS:
        for n in BATCHES:
            for use_w in (False, True):
                z, data, label, weight = make_case(3 * vox + n + ncls, n, vox, ncls)
                w = weight if use_w else None
                out3, dl = _head(lib, z, data, label, w)
                dl_h = dl.cpu().numpy()
                for layout in [l for l in _layouts(ncls) if l[0] == "fp32"]:
                    c = OpCase(z, data, label, weight, layout, False, use_w)
                    out8, raw, _ = c.run(lib, spec)
                    what = "neutral vox %d n %d ncls %d stride %d weight %s" % (vox, n, ncls, layout[1], use_w)
                    assert same_bits(out8[:3], out3), (what, out8[:3], out3)
                    assert same_bits(out8[4:5], out3[:1]) and out8[5] == 0
                    assert same_bits(np.ascontiguousarray(c.dlogits_of(raw)[:, :ncls]), dl_h), what
                packed = torch.full((n * vox, 8), 0x5A5A, dtype=torch.int16, device="cuda")
                _lib.check(lib.ursn_dlogits_pack(ctypes.c_void_p(dl.data_ptr()), n, vox, ncls, ctypes.c_void_p(packed.data_ptr()), 8, 1, None))
                torch.cuda.synchronize()
                want = packed.cpu().numpy().view(np.uint16)
                c = OpCase(z, data, label, weight, ("fp32", ncls), False, use_w, out_layout=("bf16", 8))
                out8, raw, _ = c.run(lib, spec)
                assert np.array_equal(raw.view(np.uint16).reshape(-1, 8), want), "neutral fp32 in, bf16 out: vox %d n %d ncls %d" % (vox, n, ncls)
                assert same_bits(out8[:3], out3)
                # bf16 z in: logits that are bf16-exact, so both heads see the same values
                zb = O.bf16_round(z)
                out3b, dlb = _head(lib, zb, data, label, w)
                _lib.check(lib.ursn_dlogits_pack(ctypes.c_void_p(dlb.data_ptr()), n, vox, ncls, ctypes.c_void_p(packed.data_ptr()), 8, 1, None))
                torch.cuda.synchronize()
                want = packed.cpu().numpy().view(np.uint16).astype(np.int64)
                c = OpCase(zb, data, label, weight, ("bf16", 8), False, use_w)
                out8, raw, _ = c.run(lib, spec)
                got = raw.view(np.uint16).reshape(-1, 8).astype(np.int64)
                # same sign and adjacent patterns: one bf16 ulp (a zero against the smallest values of either sign included)
                d = np.abs(np.where(got & 0x8000, -(got & 0x7FFF), got & 0x7FFF) - np.where(want & 0x8000, -(want & 0x7FFF), want & 0x7FFF))
                tiny = ((got & 0x7FFF) < 0x0080) & ((want & 0x7FFF) < 0x0080)
                assert ((d <= 1) | tiny).all(), ("neutral bf16 in: vox %d n %d ncls %d" % (vox, n, ncls), int(d.max()))
                flips += int((d != 0).sum())
                total += d.size
                assert abs(float(out8[0]) - float(out3b[0])) <= 1e-5 * abs(float(out3b[0])) + 1e-30
                assert same_bits(out8[1:3], out3b[1:3])
    print("neutral ncls %d: %d of %d bf16 values differ from the fp32 head's packed dlogits by one ulp (fast exp / log)" % (ncls, flips, total))


# ---- net-level fixtures -------------------------------------------------------------------------------------------------------
# dims, F, classes, num_strides, batch, batch the handle is built for
SHAPES = [((16, 16, 16, 1), 8, 3, 2, 2, 2), ((16, 16, 16, 1), 8, 4, 2, 2, 2), ((16, 16, 16, 1), 8, 5, 2, 2, 2),
          ((32, 32, 1), 8, 3, 3, 2, 2), ((16, 16, 16, 1), 8, 3, 2, 1, 2)]
SHAPE_IDS = ["3d_3cls", "3d_4cls", "3d_5cls", "2d_3cls", "3d_3cls_batch1of2"]
SHAPE_8 = ((16, 16, 16, 1), 8, 8, 2, 2, 2)   # every lane of the 8-channel logits piece carries a class
PLANS = ["fp32", "bf16"]
NONNEUTRAL = SPECS[1:]


def _net(shape, plan, use_weight=True, lr=None):
    dims, F, ncls, ns, N, NB = shape
    net = uresnet(dims=list(dims), num_class=ncls, base_num_outputs=F, num_strides=ns)
    net.construct(trainable=True, use_weight=use_weight, learning_rate=lr, precision=plan)
    P = as_f32_exact(oracle_params(dims, F, ncls, num_strides=ns))
    net.set_variables(P)
    if NB > N:   # a handle built for a larger batch than the one under test
        net.run_test(None, *make_inputs(dims, ncls, NB, seed=77))
    return net, P


def _grad_vec(net):
    torch.cuda.synchronize()
    return net._grads.detach().cpu().numpy().copy()


def _inputs(dims, ncls, N, seed):
    """make_inputs with weights of order 1: the loss terms then have comparable sizes."""
    data, label, weight = make_inputs(dims, ncls, N, seed=seed)
    return data, label, (weight * weight.shape[1]).astype(np.float32)


# ---- 3. the neutral step is the step -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("plan", PLANS)
@pytest.mark.parametrize("shape", SHAPES + [SHAPE_8], ids=SHAPE_IDS + ["3d_8cls"])
def test_neutral_step_is_the_step(shape, plan):
    dims, F, ncls, ns, N, NB = shape
    net, P = _net(shape, plan)
    dd, ld, wd = upload(*make_inputs(dims, ncls, N, seed=21))
    net.zero_gradients(None)
    r1, doc1 = net.accum_gradients(None, dd, ld, wd)
    G1 = _grad_vec(net)
    D1 = net.debug_tensor("logits:grad")
    net.zero_gradients(None)
    r2, doc2 = net.accum_gradients(None, dd, ld, wd, loss=LossSpec())
    G2 = _grad_vec(net)
    assert doc1 == doc2 and np.abs(G1).max() > 0
    assert same_bits(np.float32(r1[1:]), np.float32(r2[1:])), (r1, r2)
    assert same_bits(D1, net.debug_tensor("logits:grad")), "the stored dlogits differ"
    assert same_bits(G1, G2), "%d of %d gradient elements differ" % (int((bits(G1) != bits(G2)).sum()), G1.size)
    ce, dice = net.last_loss_terms()
    assert same_bits(np.float32([ce]), np.float32([r1[1]])) and dice == 0.0
    assert net.accum_gradients(None, dd, ld, wd, fetch=False, loss=LossSpec())[0] is None


# ---- 4. every other spec against the custom path ------------------------------------------------------------------------------
def _kernels_of(net, call):
    lib = _lib.load()
    _lib.check(lib.ursn_profile_enable(net._handle, 1))
    call()
    cnt = ctypes.c_int64(0)
    _lib.check(lib.ursn_profile_read(net._handle, None, 0, ctypes.byref(cnt)))
    recs = (_lib.ursn_prof_rec * max(int(cnt.value), 1))()
    _lib.check(lib.ursn_profile_read(net._handle, recs, int(cnt.value), ctypes.byref(cnt)))
    _lib.check(lib.ursn_profile_enable(net._handle, 0))
    return [(r.kernel.decode(), int(r.pass_), int(r.launches)) for r in recs[:int(cnt.value)]]


def _against_custom(net, spec, dd, ld, wd, plan, what):
    net.zero_gradients(None)
    rc, _ = net.accum_gradients_custom(None, dd, loss_torch(spec, ld, wd))
    g_c, d_c = net.get_gradients(), net.debug_tensor("logits:grad")
    net.zero_gradients(None)
    rl, _ = net.accum_gradients(None, dd, ld, wd, loss=spec)
    g_l = net.get_gradients()
    d_l = net.debug_tensor("logits:grad")
    # the head apart from the backward's sensitivity: the step's OWN stored d-logits through forward_logits / backward_logits give
    # the step's gradient buffer bit for bit -- d-logits, BatchNorm-backward partials and handle state are what the plan's head
    # would have left for the same values (tests/test_ext_loss_gpu.py::test_replay_of_the_heads_dlogits_is_the_step)
    G_l = _grad_vec(net)
    net.zero_gradients(None)
    net.forward_logits(None, dd)
    net.backward_logits(None, d_l)
    G_r = _grad_vec(net)
    assert np.abs(G_l).max() > 0 and same_bits(G_l, G_r), "%s %s %s: %d of %d gradient elements differ from the replay of the stored d-logits" % (
        what, plan, spec, int((bits(G_l) != bits(G_r)).sum()), G_l.size)
    assert same_bits(d_l, net.debug_tensor("logits:grad"))
    lrel = abs(rl[1] - rc[1]) / abs(rc[1])
    worst = max(l2_rel(g_l[k], g_c[k]) for k in g_c if np.abs(g_c[k]).max() > 1e-12)
    ce, dice = net.last_loss_terms()
    print("%s %s %s: loss %.6f (custom %.6f, rel %.3g) = ce %.6f + %g * dice %.6f; worst per-tensor l2_rel %.4g"
          % (what, plan, spec, rl[1], rc[1], lrel, ce, spec.dice_weight, dice, worst))
    assert lrel <= 1e-5, lrel
    assert abs((ce + spec.dice_weight * dice) - rl[1]) <= 1e-5 * abs(rl[1])
    assert (dice > 0) == (spec.dice_weight > 0)
    if plan == "fp32":
        assert rel_err(d_l, d_c) < 1e-5
        assert worst <= 1e-3, worst
    else:   # see the head of the file
        ndiff = int((d_l != d_c).sum())
        print("    bf16: %d of %d stored d-logits differ from the custom path's" % (ndiff, d_l.size))
        assert (np.abs(d_l.astype(np.float64) - d_c) <= _bf16_ulp(d_c.astype(np.float64))).all()
        if ndiff == 0:
            assert worst == 0.0, worst
    return rl


@pytest.mark.parametrize("plan", PLANS)
@pytest.mark.parametrize("spec", [s[1] for s in NONNEUTRAL], ids=SPEC_IDS[1:])
def test_spec_against_custom_path(spec, plan):
    shape = SHAPES[0]
    dims, F, ncls, ns, N, NB = shape
    net, P = _net(shape, plan)
    dd, ld, wd = upload(*_inputs(dims, ncls, N, seed=22))
    _against_custom(net, spec, dd, ld, wd, plan, SHAPE_IDS[0])
    recs = _kernels_of(net, lambda: net.accum_gradients(None, dd, ld, wd, fetch=False, loss=spec))
    mine = [r for r in recs if r[0] in ("losshead", "losssums", "lossfinal")]
    want = ["losssums", "lossfinal", "losshead"] if spec.dice_weight > 0 else ["losshead", "lossfinal"]
    assert [r[0] for r in mine] == want and all(r[1] == 6 and r[2] == 1 for r in mine), mine
    assert not any(r[0] in ("head", "bhead") for r in recs), "the plan's head ran as well"


@pytest.mark.parametrize("plan", PLANS)
@pytest.mark.parametrize("shape", SHAPES[1:], ids=SHAPE_IDS[1:])
def test_shapes_against_custom_path(shape, plan):
    dims, F, ncls, ns, N, NB = shape
    net, P = _net(shape, plan)
    dd, ld, wd = upload(*_inputs(dims, ncls, N, seed=23))
    _against_custom(net, SPECS[5][1], dd, ld, wd, plan, SHAPE_IDS[SHAPES.index(shape)])
    _against_custom(net, SPECS[3][1], dd, ld, wd, plan, SHAPE_IDS[SHAPES.index(shape)])


# ---- 5. against the oracle's backward ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("spec", [SPECS[3][1], SPECS[5][1]], ids=[SPEC_IDS[3], SPEC_IDS[5]])
@pytest.mark.parametrize("shape", [((16, 16, 16, 1), 4, 3, 2, 2, 2), ((32, 32, 1), 8, 5, 3, 2, 2)], ids=["3d_f4_3cls", "2d_f8_5cls"])
def test_step_against_oracle_backward(shape, spec):
    dims, F, ncls, ns, N, NB = shape
    net, P = _net(shape, "fp32")
    data, label, weight = _inputs(dims, ncls, N, seed=24)
    d64 = O.reshape_inputs(dims, data)[0].astype(np.float64)
    logits, tape = O.forward(P, d64, F, num_strides=ns)
    ref = loss_numpy(logits, data, label, weight, spec)
    g_ref, _ = O.backward(P, tape, ref["dlogits"])
    P32 = type(P)((k, v.astype(np.float32)) for k, v in P.items())
    logits32, tape32 = O.forward(P32, d64.astype(np.float32), F, num_strides=ns)
    g_32, _ = O.backward(P32, tape32, loss_numpy(logits32, data, label, weight, spec)["dlogits"].astype(np.float32))
    net.zero_gradients(None)
    res, _ = net.accum_gradients(None, data, label, weight, loss=spec)
    assert abs(res[1] - ref["loss"]) <= 1e-4 * abs(ref["loss"]), (res[1], ref["loss"])
    g = net.get_gradients()
    bad = []
    for k in g_ref:
        if np.abs(g_ref[k]).max() <= 1e-12:
            continue
        e, floor = l2_rel(g[k], g_ref[k]), l2_rel(g_32[k], g_ref[k])
        if e > min(max(2e-3, 4 * floor), 5e-2):
            bad.append((k, e, floor))
    assert not bad, bad


# ---- 6. entries ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("plan", PLANS)
def test_voxel_feed_equals_the_dense_feed(plan):
    shape = SHAPES[0]
    dims, F, ncls, ns, N, NB = shape
    V = int(np.prod(dims[:-1]))
    net, P = _net(shape, plan)
    data, label, weight = _inputs(dims, ncls, N, seed=25)
    spec = SPECS[5][1]
    net.zero_gradients(None)
    dense = net.accum_gradients(None, data, label, weight, loss=spec)[0]
    G = _grad_vec(net)
    terms = net.last_loss_terms()
    vb = VoxelBatch(np.arange(N + 1) * V, np.tile(np.arange(V, dtype=np.int32), N), data.reshape(-1), label.reshape(-1),
                    weight.reshape(-1), np.zeros(N, np.float32), V)
    net.zero_gradients(None)
    vox = net.accum_gradients_voxels(None, vb, loss=spec)[0]
    assert vox == dense and same_bits(G, _grad_vec(net)) and net.last_loss_terms() == terms
    assert net.run_test_voxels(None, vb, loss=spec)[0] == net.run_test(None, data, label, weight, loss=spec)[0]


def test_frozen_batchnorm_training_against_custom_path():
    tag, dims, base, ncls, ns, n = B.S3D
    net, P, stats = B.calibrated_net(B.S3D, "fp32")
    dd, ld, wd = upload(*_inputs(dims, ncls, n, seed=26))
    _against_custom(net, SPECS[5][1], dd, ld, wd, "fp32", "frozen " + tag)
    assert all(same_bits(v, stats[k]) for k, v in net.get_bn_moving().items())
    # forward-only 'moving' mode: the training entry is refused, the evaluation runs
    net.set_bn_mode('moving')
    with pytest.raises(_lib.UrsnError, match="frozen"):
        net.accum_gradients(None, dd, ld, wd, loss=SPECS[5][1])
    assert np.isfinite(net.run_test(None, dd, ld, wd, loss=SPECS[5][1])[0][0])


@pytest.mark.parametrize("plan", PLANS)
def test_run_test_returns_the_steps_loss_and_leaves_the_gradients(plan):
    shape = SHAPES[0]
    dims, F, ncls, ns, N, NB = shape
    net, P = _net(shape, plan)
    dd, ld, wd = upload(*_inputs(dims, ncls, N, seed=27))
    for spec in (SPECS[2][1], SPECS[5][1]):
        net.zero_gradients(None)
        step = net.accum_gradients(None, dd, ld, wd, loss=spec)[0]
        terms = net.last_loss_terms()
        G = _grad_vec(net)
        res, doc = net.run_test(None, dd, ld, wd, loss=spec)
        assert doc == ['loss', 'acc. all', 'acc. nonzero']
        assert same_bits(np.float32(res), np.float32(step[1:])) and net.last_loss_terms() == terms
        assert same_bits(G, _grad_vec(net)), "run_test changed the gradient buffer"
    plain = net.run_test(None, dd, ld, wd)[0]
    assert same_bits(np.float32(plain), np.float32(net.run_test(None, dd, ld, wd, loss=LossSpec())[0]))


@pytest.mark.parametrize("plan", PLANS)
def test_step_ends_a_pending_forward_logits(lib, plan):
    shape = SHAPES[0]
    dims, F, ncls, ns, N, NB = shape
    net, P = _net(shape, plan)
    dd, ld, wd = upload(*_inputs(dims, ncls, N, seed=28))
    dl = torch.full((N,) + tuple(dims[:-1]) + (ncls,), 1e-4, dtype=torch.float32, device="cuda")
    for call in (lambda: net.accum_gradients(None, dd, ld, wd, loss=SPECS[1][1]), lambda: net.run_test(None, dd, ld, wd, loss=SPECS[4][1])):
        net.zero_gradients(None)
        net.forward_logits(None, dd)
        call()
        G = _grad_vec(net)
        with pytest.raises(_lib.UrsnError, match="another run call"):
            net.backward_logits(None, dl)
        assert same_bits(G, _grad_vec(net)), "a refused call changed the gradient buffer"
    # refusals of the net-level call come before any launch: the gradient buffer survives them (check_call, as in every run call,
    # has by then ended a pending forward_logits)
    net.zero_gradients(None)
    net.accum_gradients(None, dd, ld, wd, loss=SPECS[1][1])
    G = _grad_vec(net)
    bad = _lib.ursn_loss_desc(0.5, 0.0, 0.0, 1.0, -1)
    p = lambda t: ctypes.c_void_p(t.data_ptr())
    rc = lib.ursn_accum_step_loss(net._handle, p(dd), p(ld), p(wd), N, ctypes.byref(bad), None)
    assert rc != 0 and b"focal exponent" in lib.ursn_last_error()
    rc = lib.ursn_accum_step_loss(net._handle, p(dd), None, p(wd), N, ctypes.byref(_desc_of(SPECS[1][1])), None)
    assert rc != 0 and b"input_label is null" in lib.ursn_last_error()
    rc = lib.ursn_accum_step_loss(net._handle, p(dd), p(ld), p(wd), NB + 1, ctypes.byref(_desc_of(SPECS[1][1])), None)
    assert rc != 0 and b"batch" in lib.ursn_last_error()
    assert same_bits(G, _grad_vec(net))


# ---- 7. state independence -----------------------------------------------------------------------------------------------------
def _loss_step(h, dd, ld, wd, n, spec):
    sd = _desc_of(spec)
    p = lambda t: ctypes.c_void_p(t.data_ptr())
    h.last_n = n
    _lib.check(h.lib.ursn_accum_step_loss(h.handle, p(dd), p(ld), p(wd), n, ctypes.byref(sd), None))
    m = h.read_metrics()["metrics"]
    t = (ctypes.c_float * 2)()
    _lib.check(h.lib.ursn_read_loss_terms(h.handle, t, None))
    return m, np.array(list(t), np.float32), h.host("grads")


@pytest.mark.parametrize("plan", PLANS)
def test_step_depends_only_on_its_arguments(plan):
    dims, F, ncls, ns, N = (16, 16, 16, 1), 8, 3, 2, 2
    dd, ld, wd = upload(*_inputs(dims, ncls, N, seed=29))
    od, ol, ow = upload(*_inputs(dims, ncls, N, seed=30))
    spec = SPECS[5][1]
    results = {}
    for fill in ("zero", "nan"):
        with Handle(make_cfg(dims, F, ncls, ns, N, bf16=(plan == "bf16")), fill) as h:
            h.zero_grad(fetch=False)
            first = _loss_step(h, dd, ld, wd, N, spec)
            assert all(np.isfinite(a).all() for a in first)
            h.accum_step(od, ol, ow, N, fetch=False)          # unrelated calls of every kind, other inputs, another batch size
            h.eval(od, ol, ow, 1)
            h.infer(od, ol, N)
            _loss_step(h, od, ol, ow, 1, SPECS[2][1])
            h.zero_grad(fetch=False)
            again = _loss_step(h, dd, ld, wd, N, spec)
            for a, b, name in zip(first, again, ("metrics", "terms", "gradients")):
                assert same_bits(a, b), "%s differ after unrelated calls (fill %s)" % (name, fill)
            results[fill] = first
    for a, b, name in zip(results["zero"], results["nan"], ("metrics", "terms", "gradients")):
        assert same_bits(a, b), "%s depend on what the workspace held at create" % name
