"""A call's results depend only on its arguments, the parameter / gradient / Adam buffers and the Adam step: not on what the
caller-owned workspace held before ursn_create, not on the calls the handle served before, not on whether the host waited
between enqueues (include/uresnet_hip.h, at ursn_create).

Every other net-level test makes one call on a fresh handle whose workspace came straight from the allocator (usually zero
pages), so a kernel that reads a halo row, a pad lane, a statistics partial or a split-K slab nothing wrote in this call, or
host state that survives a call (ginit, the waiting BatchNorm-backward reductions, the bf16 plan's pack state), would pass
there.  Here the test owns the buffers (tests/_abi.py), fills the workspace with NaN or huge finite bytes before create, runs
scripted call histories and compares BITS: there are no atomics in csrc/ and every reduction has a fixed order, so two runs
of the same call owe each other equality and no comparison in this module has a tolerance.  Check 0 establishes that promise
on the hardware (two identical fresh handles) before checks 1-3 rely on it.

The shapes are ones the suite already holds to the fp64 oracle (tests/test_model_shapes_gpu.py, tests/test_net_gpu.py,
tests/test_bf16_net_gpu.py), so a failure here is about state and not arithmetic.  Assertions are on the calls' OUTPUTS
(metrics, gradients, softmax, labels, post-Adam buffers); first_difference() names the first stored tensor that differs for
the message only (pad lanes nobody reads may keep the fill).  One process, no environment switches; each handle is destroyed
and its canary guards checked before the next is built, apart from the pair being compared."""
import pytest

import numpy as np

from _abi import Handle, compare_outputs, make_cfg, upload
from _net import make_inputs

pytestmark = pytest.mark.gpu

# tag, dims, F, classes, num_strides, bf16, trainable, use_weight, batch of the workspace-fill check
CASES = [
    ("3d_f8_3cls_fp32", (32, 32, 64, 1), 8, 3, 3, False, 1, 1, 2),
    ("3d_f8_3cls_bf16", (32, 32, 64, 1), 8, 3, 3, True, 1, 1, 2),
    ("2d_f16_2cls_padded_logits_fp32", (64, 64, 1), 16, 2, 3, False, 1, 1, 2),
    ("6cls_padded_logits_fp32", (32, 32, 64, 1), 8, 6, 3, False, 1, 1, 2),
    ("6cls_padded_logits_bf16", (32, 32, 64, 1), 8, 6, 3, True, 1, 1, 2),
    ("2d_f6_widths_not_multiple_of_4_fp32", (64, 64, 1), 6, 3, 3, False, 1, 1, 2),   # the layers ursn_create clears
    ("cin3_fp32", (32, 32, 32, 3), 8, 3, 3, False, 1, 1, 2),
    ("npot_48x32x80_fp32", (48, 32, 80, 1), 8, 3, 4, False, 1, 1, 2),
    ("npot_48x32x80_bf16", (48, 32, 80, 1), 8, 3, 4, True, 1, 1, 2),
    ("full_depth_bottom_1x1x3_fp32", (32, 32, 96, 1), 8, 3, 5, False, 1, 1, 1),
    ("f24_bf16", (16, 32, 32, 1), 24, 3, 2, True, 1, 1, 1),
    ("no_weight_null_pointer_fp32", (32, 32, 64, 1), 8, 3, 3, False, 1, 0, 2),
    ("inference_only_fp32", (32, 32, 64, 1), 8, 3, 3, False, 0, 1, 2),   # no backward workspace: eval / infer only
    ("inference_only_bf16", (32, 32, 64, 1), 8, 3, 3, True, 0, 1, 2),
    ("64x64x128_capped_grids_fp32", (64, 64, 128, 1), 8, 3, 5, False, 1, 1, 2),    # capped grids, z-segments, split-K slabs
    ("64x64x128_capped_grids_bf16", (64, 64, 128, 1), 8, 3, 5, True, 1, 1, 2),
]
IDS = [c[0] for c in CASES]
TRAINABLE = [c for c in CASES if c[6]]


class Feed(object):
    """Device-resident minibatches of a case: name -> (data, label, weight-or-None) with `n` leading rows each."""

    def __init__(self, case, batches):
        tag, dims, base, ncls, ns, bf16, trainable, use_weight, n1 = case
        self.dev = {}
        for name, (n, seed) in batches.items():
            d, l, w = make_inputs(dims, ncls, n, seed=seed)
            self.dev[name] = upload(d, l, w if use_weight else None)   # use_weight = 0: weight = NULL

    def get(self, name, n):
        d, l, w = self.dev[name]
        assert n <= d.shape[0]
        return d, l, w   # the first n images of a contiguous [N, ...] batch are its first n rows


def _cfg(case, max_batch):
    tag, dims, base, ncls, ns, bf16, trainable, use_weight, n1 = case
    return make_cfg(dims, base, ncls, ns, max_batch, trainable=trainable, use_weight=use_weight, bf16=bf16)


def _has_labels_call(case):
    return case[3] >= 3 and case[1][-1] == 1   # ursn_infer_labels: >= 3 classes and one input channel


def _run(h, op, feed, stream=None):
    """One scripted call on a handle: (kind, batch name, n) -> dict of host outputs."""
    kind, name, n = op
    if kind == "zero_grad":
        return h.zero_grad(stream)
    if kind == "apply_adam":
        return h.apply_adam(1e-3, stream)
    d, l, w = feed.get(name, n)
    if kind == "accum":
        return h.accum_step(d, l, w, n, stream)
    if kind == "eval":
        return h.eval(d, l, w, n, stream)
    if kind == "infer":
        return h.infer(d, l, n, stream)
    if kind == "infer_labels":
        return h.infer_labels(d, l, n, stream)
    raise ValueError(kind)


def _assert_finite(what, out):
    """Loss, gradients and parameters.  (The accuracies are not held to this: accuracy_nonzero is NaN by definition when the
    input has more than one channel, tests/test_model_shapes_gpu.py; they are still compared bit for bit.)"""
    if out is None:
        return
    if out.get("metrics") is not None and out["metrics"].size == 3:
        assert np.isfinite(out["metrics"][0]), "%s: loss is %r" % (what, float(out["metrics"][0]))
    for k in ("grads", "params"):
        if out.get(k) is not None:
            assert np.isfinite(out[k]).all(), "%s: %s has %d non-finite elements" % (what, k, int((~np.isfinite(out[k])).sum()))


def _fill_script(case):
    n = case[8]
    if case[6]:
        s = [("zero_grad", None, 0), ("accum", "A", n), ("apply_adam", None, 0)]
    else:
        s = []
    s += [("eval", "A", n), ("infer", "A", n)]
    if _has_labels_call(case):
        s.append(("infer_labels", "A", n))
    return s


def _lockstep(case, fills, script, feed, max_batch):
    """The script on a handle over fills[0] and, call by call beside it, on a handle over each other fill (two handles alive at
    a time, so that first_difference can look at both after the call that differs)."""
    tag = case[0]
    for fill in fills[1:]:
        with Handle(_cfg(case, max_batch), fills[0]) as a, Handle(_cfg(case, max_batch), fill) as b:
            for i, op in enumerate(script):
                oa, ob = _run(a, op, feed), _run(b, op, feed)
                what = "%s, call %d %s%s, workspace %s against %s" % (tag, i, op[0], "" if op[1] is None else "(%s,%d)" % op[1:],
                                                                      fills[0], fill)
                _assert_finite(what, oa)
                compare_outputs(what, oa, ob, a, b)


# ---- the driver itself ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", [CASES[0], CASES[1]], ids=IDS[:2])
def test_driver_fill_reaches_the_kernels_and_guards_catch_a_write(case):
    """What checks 1-3 lean on in tests/_abi.py: the fill is still in the workspace after ursn_create (a create that cleared
    the whole workspace would make check 1 vacuous: most bytes must survive it), first_difference finds the stored tensors of
    both passes, and check_guards notices one changed canary byte on either side of a buffer."""
    from _abi import FILLS, first_difference
    feed = Feed(case, {"A": (2, 101)})
    with Handle(_cfg(case, 2), "nan") as a, Handle(_cfg(case, 2), "big") as b:
        kept = float((a.ws.view == FILLS["nan"]).float().mean().item())
        assert kept > 0.5, "ursn_create cleared %.0f %% of the workspace" % (100 * (1 - kept))
        d, l, w = feed.get("A", 2)
        compare_outputs(case[0], a.accum_step(d, l, w, 2), b.accum_step(d, l, w, 2), a, b)
        for name in ("UResNet/conv0:z", "UResNet/conv0:mean", "UResNet/conv0", "UResNet/conv2:z", "logits:grad",
                     "UResNet/conv2:dz", "UResNet/conv0:dz"):
            assert a.tensor(name) is not None, name
        z, ch = a.tensor("UResNet/conv2:z")
        assert ch == 3 and z.shape[0] == 2 * a.pix and z.shape[1] > ch, (z.shape, ch)   # the logits' pad lanes are read as well
        assert first_difference(a, b).startswith("first difference:")
        for g in (a.ws, a.grads):
            for idx in (0, g.raw.numel() - 1):
                keep = int(g.raw[idx].item())
                g.raw[idx] = keep ^ 0x01
                with pytest.raises(AssertionError, match="canary"):
                    a.check_guards()
                g.raw[idx] = keep
        a.check_guards()


# ---- 0. precondition --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_0_two_identical_fresh_handles_agree(case):
    """Same fill, same inputs, same calls: equal bits.  Asserted apart from checks 1-3 so that their failures cannot be
    confused with run-to-run noise; with no atomics in the code a failure HERE means a race or an uninitialised read."""
    feed = Feed(case, {"A": (case[8], 101)})
    _lockstep(case, ["zero", "zero"], _fill_script(case), feed, case[8])


# ---- 1. workspace fill ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_1_results_do_not_depend_on_the_workspace_fill(case):
    """Handles created over zero, NaN (0xFF..) and huge finite (0x7F..) workspaces run zero_grad, accum_step(n = max_batch),
    apply_adam, eval, infer(+label), infer_labels and agree bit for bit at every call, with finite loss and gradients."""
    feed = Feed(case, {"A": (case[8], 101)})
    _lockstep(case, ["zero", "nan", "big"], _fill_script(case), feed, case[8])


# ---- 2. history -------------------------------------------------------------------------------------------------------
def _history_script(case):
    lab = _has_labels_call(case)
    if not case[6]:
        return [("eval", "A", 3), ("infer", "C", 2), ("infer_labels" if lab else "infer", "B", 1), ("eval", "B", 1),
                ("infer", "A", 3), ("eval", "C", 2)]
    return [("accum", "A", 3), ("eval", "B", 1), ("infer", "C", 2), ("infer_labels" if lab else "infer", "B", 1),
            ("zero_grad", None, 0), ("accum", "B", 1), ("accum", "C", 2), ("apply_adam", None, 0), ("eval", "A", 3),
            ("zero_grad", None, 0), ("accum", "A", 3), ("infer", "B", 1)]


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_2_results_do_not_depend_on_the_calls_before(case):
    """One handle planned for max_batch = 3 serves a script that mixes call kinds, batch sizes (3, 1, 2: a smaller batch
    after a larger one leaves stale tail images in every tensor) and inputs.  Each call's outputs are compared with the same
    call made as the FIRST call of a fresh handle with the same max_batch, the parameters / gradient buffer / Adam slots and
    step as they stood before that call, and a differently filled workspace.  zero_grad has no input but the buffer: its
    output is held to all-zero bits directly."""
    tag = case[0]
    feed = Feed(case, {"A": (3, 201), "B": (1, 202), "C": (2, 203)})
    script = _history_script(case)
    fresh_fills = ["big", "zero", "nan"]
    with Handle(_cfg(case, 3), "nan") as h:
        for i, op in enumerate(script):
            what = "%s, call %d %s%s after %s" % (tag, i, op[0], "" if op[1] is None else "(%s,%d)" % op[1:],
                                                  " > ".join(o[0] + ("" if o[1] is None else "(%s,%d)" % o[1:])
                                                             for o in script[:i]) or "nothing")
            if op[0] == "zero_grad":
                out = _run(h, op, feed)
                assert not out["grads"].view(np.uint32).any(), what
                continue
            before = h.state() if case[6] else None
            out = _run(h, op, feed)
            _assert_finite(what, out)
            fill = fresh_fills[i % 3]
            with Handle(_cfg(case, 3), fill, state=before) as f:
                compare_outputs(what + " against a fresh handle (workspace %s)" % fill, _run(f, op, feed), out, f, h)


# ---- 3. enqueue-only against synchronised -----------------------------------------------------------------------------
def _train(h, feed, stream, sync):
    import torch
    for it in range(3):
        h.zero_grad(stream, fetch=False)
        if sync:
            torch.cuda.synchronize()
        for name in (("A", "B"), ("C", "A"), ("B", "C"))[it]:
            d, l, w = feed.get(name, 2)
            h.accum_step(d, l, w, 2, stream, fetch=False)   # out3 = NULL: enqueues only
            if sync:
                torch.cuda.synchronize()
        h.apply_adam(1e-3, stream, fetch=False)
        if sync:
            torch.cuda.synchronize()
    out = h.read_metrics(stream)   # first host synchronisation of the enqueue-only run
    torch.cuda.synchronize()
    out.update(params=h.host("params"), adam_m=h.host("adam_m"), adam_v=h.host("adam_v"), grads=h.host("grads"))
    return out


@pytest.mark.parametrize("explicit_stream", [False, True], ids=["default_stream", "own_stream"])
@pytest.mark.parametrize("case", TRAINABLE, ids=[c[0] for c in TRAINABLE])
def test_3_enqueue_only_equals_synchronised(case, explicit_stream):
    """Three training iterations of zero_grad, accum_step(out3 = NULL) x 2 on different minibatches, apply_adam enqueued with
    no host synchronisation until the end (what bench.py and real training do), against the same calls with a device
    synchronisation after each: params, adam_m, adam_v, the gradient buffer and the last metrics equal bit for bit.  The
    weight gradients and the forward shortcut convs run on the handle's second stream, ordered by events only; the run on an
    explicit torch.cuda.Stream() keeps the ordering from leaning on the legacy default stream's implicit synchronisation."""
    import torch
    tag = case[0]
    feed = Feed(case, {"A": (2, 301), "B": (2, 302), "C": (2, 303)})   # uploaded and synchronised before the first enqueue
    stream = torch.cuda.Stream() if explicit_stream else None
    with Handle(_cfg(case, 2), "nan") as a, Handle(_cfg(case, 2), "big") as b:
        out_a = _train(a, feed, stream, sync=False)
        out_b = _train(b, feed, stream, sync=True)
        _assert_finite(tag, out_a)
        compare_outputs("%s, 3 iterations enqueue-only against synchronised on %s" %
                        (tag, "an explicit stream" if explicit_stream else "the default stream"), out_a, out_b, a, b)
