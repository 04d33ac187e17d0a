"""In-situ parity across the model shapes the two plans accept (tests/test_model_shapes_host.py pins the domain): input
channel counts other than one, class counts 1..8 (every padding of the logits layer), base widths that are not 4, 8 or 16
(levels narrower than four channels, widths that are not a multiple of four), extents that are not powers of two and
bottom levels of extent 1.  Each case runs one accum_gradients step and holds every layer to the kernel-level bounds of
tests/_insitu.py (fp32: 2e-5 of max, 1e-5 for the elementwise passes; bf16: one ulp + 2e-5 of max), then checks the head
against the product's own stored logits (independent of how well the network is conditioned):

    loss                within 1e-5 relative of the fp64 loss of bn(z_conv2 stored)
    accuracy_all        exact (a voxel whose fp64 top-2 margin is below 1e-5 may go either way)
    accuracy_nonzero    likewise, or NaN when the input has more than one channel (oracle.uresnet_np.loss_and_metrics)
    inference() softmax within 1e-6 (fp32) / 1e-5 (bf16 head: __expf) absolute of an fp64 softmax of the logits it stored

Layers: lib/uresnet.py:37-121, lib/resnet_module.py:25-68, lib/ssnet.py:57-71.  PARITY UNPINNED (oracle/__init__.py)."""
import time

import numpy as np
import pytest

from oracle import uresnet_np as O
from _insitu import InSitu
from _net import as_f32_exact, make_inputs, oracle_params
from uresnet_amd import uresnet

pytestmark = pytest.mark.gpu

CASES = [
    # tag, dims, F, classes, batch, num_strides, precision, plan max_batch
    ("cin2_generic_conv0_odd_stride_fp32", (32, 32, 32, 2), 8, 3, 2, 3, "fp32", 0),
    ("cin4_tiled_conv0_4cls_fused_head_fp32", (32, 32, 32, 4), 8, 4, 2, 3, "fp32", 0),
    ("cin8_conv0_8to8_8cls_unit_fusions_fp32", (32, 32, 32, 8), 8, 8, 1, 3, "fp32", 0),
    ("6cls_padded_stride8_logits_fp32", (32, 32, 64, 1), 8, 6, 2, 3, "fp32", 0),
    ("7cls_padded_stride8_logits_fp32", (32, 32, 64, 1), 8, 7, 2, 3, "fp32", 0),
    ("1cls_degenerate_softmax_2d_fp32", (64, 64, 1), 16, 1, 2, 3, "fp32", 0),
    ("2cls_padded_stride4_logits_2d_fp32", (64, 64, 1), 16, 2, 2, 3, "fp32", 0),
    ("f6_widths_not_multiple_of_4_2d_fp32", (64, 64, 1), 6, 3, 2, 3, "fp32", 0),
    ("f2_levels_under_4_channels_2d_fp32", (32, 64, 1), 2, 3, 2, 4, "fp32", 0),
    ("f12_concat_views_stride24_fp32", (32, 32, 32, 1), 12, 3, 2, 2, "fp32", 0),
    ("f32_wide_level0_fp32", (16, 32, 32, 1), 32, 5, 1, 2, "fp32", 0),
    ("npot_48x32x80_bottom_3x2x5_fp32", (48, 32, 80, 1), 8, 3, 2, 4, "fp32", 0),
    ("bottom_1x1x3_fp32", (32, 32, 96, 1), 8, 3, 1, 5, "fp32", 0),
    ("2d_bottom_1x16_fp32", (32, 512, 1), 8, 3, 2, 5, "fp32", 0),
    ("cin3_batch3_of_plan4_fp32", (32, 32, 32, 3), 8, 3, 3, 3, "fp32", 4),
    ("1cls_bhead_bf16", (32, 32, 64, 1), 8, 1, 2, 3, "bf16", 0),
    ("4cls_bhead_bf16", (32, 32, 64, 1), 8, 4, 2, 3, "bf16", 0),
    ("6cls_bhead_bf16", (32, 32, 64, 1), 8, 6, 2, 3, "bf16", 0),
    ("8cls_bhead_bf16", (32, 32, 64, 1), 8, 8, 2, 3, "bf16", 0),
    ("f24_generic_families_concat_stride48_bf16", (16, 32, 32, 1), 24, 3, 1, 2, "bf16", 0),
    ("f32_wide_level0_bf16", (32, 32, 32, 1), 32, 5, 1, 3, "bf16", 0),
    ("npot_48x32x80_bf16", (48, 32, 80, 1), 8, 3, 2, 4, "bf16", 0),
]

_T0 = []


def _step(dims, base, ncls, N, ns, prec, max_batch=0, seed=37):
    P = as_f32_exact(oracle_params(dims, base, ncls, num_strides=ns))
    data, label, weight = make_inputs(dims, ncls, N, seed=seed)
    net = uresnet(dims=list(dims), num_class=ncls, base_num_outputs=base, num_strides=ns)
    net.construct(trainable=True, use_weight=True, learning_rate=1e-3, precision=prec)
    if max_batch:
        net._ensure_handle(max_batch)   # a plan sized for more images than are fed
    net.set_variables(P)
    net.zero_gradients(None)
    res, _ = net.accum_gradients(None, data, label, weight)
    assert np.isfinite(res[1])
    return net, P, data, label, weight, res


def _near_ties(logits, tol=1e-5):
    srt = np.sort(logits, axis=-1)
    if logits.shape[-1] < 2:
        return np.zeros(logits.shape[:-1], bool)
    return (srt[..., -1] - srt[..., -2]) < tol


@pytest.mark.parametrize("case", CASES, ids=[c[0] for c in CASES])
def test_every_layer_and_the_head_in_situ(case):
    if not _T0:
        _T0.append(time.perf_counter())
    tag, dims, base, ncls, N, ns, prec, mb = case
    bf16 = prec == "bf16"
    net, P, data, label, weight, res = _step(dims, base, ncls, N, ns, prec, mb)
    chk = InSitu(net, P, dims, base, ncls, ns, data, label, weight, bf16=bf16)
    T = chk.run(tag)
    assert set(T.worst) >= {"z", "rstd", "act", "join", "dlogits", "dz", "dw", "dx"}, sorted(T.worst)

    # the head against the logits this step stored
    logits = chk.bn_apply("UResNet/conv2")
    m = O.loss_and_metrics(logits, chk.data, chk.label, chk.weight)
    assert abs(res[1] - m["loss"]) <= 1e-5 * abs(m["loss"]), (res[1], m["loss"])
    lab = chk.label.astype(np.int64)
    tie = _near_ties(logits)
    pred = m["pred"]
    # a near-tie voxel may be counted either way: the product's accuracy lies between the oracle's with every near-tie wrong
    # and with every near-tie right; with none, both bounds are the oracle's value and the check is exact
    lo = float(((pred == lab) & ~tie).mean())
    hi = float(((pred == lab) | tie).mean())
    assert lo - 1e-7 <= res[2] <= hi + 1e-7, (res[2], m["acc_all"], int(tie.sum()))
    if data.size // N != lab[0].size:   # more than one input channel: undefined in the reference, NaN in both
        assert np.isnan(m["acc_nonzero"]) and np.isnan(res[3]), (res[3], m["acc_nonzero"])
    else:
        nz = chk.data[..., 0] > 0
        lo = float(((pred == lab) & ~tie)[nz].mean())
        hi = float(((pred == lab) | tie)[nz].mean())
        assert lo - 1e-7 <= res[3] <= hi + 1e-7, (res[3], m["acc_nonzero"], int((tie & nz).sum()))

    # inference(): softmax of the logits this forward pass stored
    sm = net.inference(None, data)[0]
    z = net.debug_tensor("UResNet/conv2:z").astype(np.float64)
    mu = net.debug_tensor("UResNet/conv2:mean").astype(np.float64)
    r = net.debug_tensor("UResNet/conv2:rstd").astype(np.float64)
    ref = O.softmax((z - mu) * r + np.asarray(P["UResNet/conv2/BatchNorm/beta"], np.float64))
    assert sm.shape == ref.shape, (sm.shape, ref.shape)
    err = float(np.abs(sm - ref).max())
    assert err <= (1e-5 if bf16 else 1e-6), err
    print("%s: head loss %.7g (fp64 of stored logits %.7g), softmax max abs err %.2e, %d near-tie voxels; %.1f s into the module"
          % (tag, res[1], m["loss"], err, int(tie.sum()), time.perf_counter() - _T0[0]))


@pytest.mark.parametrize("case", [
    ((32, 32, 32, 2), 8, 3, 2, True, 3),   # generic conv0 on an odd-stride input
    ((32, 32, 32, 4), 8, 4, 2, True, 3),   # tiled 4 -> 8 conv0, unpadded 4-class logits
], ids=["cin2_fp32", "cin4_4cls_fp32"])
def test_net_level_gradients_multi_channel_input(case):
    """test_net_gpu.py::test_accum_gradients_parity on a multi-channel input: every gradient against the fp64 oracle."""
    from test_net_gpu import test_accum_gradients_parity
    test_accum_gradients_parity(case)
