"""Frozen-BatchNorm training, host side: the reference derivative the GPU tests use (numpy oracle with bn_fwd / bn_bwd swapped
for the fixed-statistics layer) against torch autograd through oracle.uresnet_torch.forward with `bn` swapped the same way; the
driver key; the mode's refusal without moving statistics; the C-ABI surface."""
import os

import numpy as np
import pytest

from _bn_frozen import S2D, S3D, batch_statistics, oracle_frozen_step, torch_frozen_step
from _net import as_f32_exact, l2_rel, make_inputs, oracle_params
from oracle import uresnet_np as O
from uresnet_amd import _lib, uresnet
from uresnet_amd.config import ssnet_config

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize("shape", [S3D, S2D], ids=[S3D[0], S2D[0]])
def test_swapped_oracle_is_the_fixed_statistics_derivative(shape):
    """Statistics: another batch's batch statistics, so every layer is alive.  The hand-written reverse pass with
    dz = r * dy against autograd, which knows nothing of it: 1e-10 rel-L2 per tensor (measured 2.7e-15 / 4.6e-15).  And the
    frozen gradient is a different gradient (the distance to the batch-mode one is printed), no tensor of it zero."""
    tag, dims, base, ncls, ns, n = shape
    P = as_f32_exact(oracle_params(dims, base, ncls, num_strides=ns))
    stats = batch_statistics(P, shape, make_inputs(dims, ncls, n, seed=51)[0])
    data, label, weight = make_inputs(dims, ncls, n, seed=52)
    g, m = oracle_frozen_step(P, shape, stats, data, label, weight)
    gt, _, loss_t = torch_frozen_step(P, shape, stats, data, label, weight)
    assert abs(m["loss"] - loss_t) <= 1e-12 * abs(loss_t)
    worst = max(l2_rel(g[k], gt[k]) for k in g)
    print("%s: swapped oracle against torch autograd, worst rel-L2 %.1e over %d tensors" % (tag, worst, len(g)))
    assert list(g) == list(gt) and worst <= 1e-10
    assert all(np.abs(v).max() > 0 for v in g.values())
    g_batch, _ = O.step_gradients(P, dims, base, data, label, weight, num_strides=ns)
    dist = sorted(l2_rel(g_batch[k], g[k]) for k in g)
    print("%s: batch-mode gradient against the frozen one, rel-L2 per tensor: min %.2g median %.2g" % (tag, dist[0], dist[len(dist) // 2]))
    assert dist[len(dist) // 2] > 5e-2      # not the same gradient: the typical tensor lies outside the widest bound any GPU test allows
    assert O.bn_bwd.__name__ == "bn_bwd" and O.bn_fwd.__name__ == "bn_fwd"      # the swap was undone


def test_train_bn_key(tmp_path):
    c = ssnet_config()
    assert c.TRAIN_BN == 'batch'
    f = tmp_path / "a.cfg"
    f.write_text("TRAIN_BN 'frozen'\n")
    c.override(str(f))
    assert c.TRAIN_BN == 'frozen'
    for bad in ("TRAIN_BN 'moving'\n", "TRAIN_BN 1\n", "TRAIN_BN True\n", "TRAIN_BN ''\n"):
        f.write_text(bad)
        with pytest.raises(TypeError):
            ssnet_config().override(str(f))
    assert ssnet_config().TRAIN_BN == 'batch' and ssnet_config().BN_MOVING is False


def test_frozen_mode_needs_moving_statistics():
    net = uresnet(dims=[32, 32, 1], num_class=3, base_num_outputs=4, num_strides=3)
    net.construct(allocate=False, bn_moving=False)
    with pytest.raises(RuntimeError, match="no moving statistics"):
        net.set_bn_mode('frozen')
    assert net.bn_mode() == 'batch'
    with pytest.raises(ValueError, match="'batch', 'moving' or 'frozen'"):
        net.set_bn_mode('fixed')
    assert "dz = rstd * g" in net.set_bn_mode.__doc__


def test_abi_surface():
    """Appended functions only: declared in the header, exported, bound; the version stays 9."""
    lib = _lib.load()
    with open(os.path.join(ROOT, "include", "uresnet_hip.h")) as f:
        hdr = f.read()
    for name in ("ursn_bn_frozen_train", "ursn_bn_backward_frozen", "ursn_bn_bf16_backward_frozen"):
        assert name in _lib.EXPORTS and hasattr(lib, name) and (name + "(") in hdr, name
    assert "#define URSN_ABI_VERSION 9" in hdr and lib.ursn_abi_version() == 9
    # refused before any device work: null handle, null arguments
    assert lib.ursn_bn_frozen_train(None, 1) != 0 and b"null handle" in lib.ursn_last_error()
    assert lib.ursn_bn_backward_frozen(None, None, None, None, None, None, None, None, 8, 8, 0, None, 0, None) != 0
    assert lib.ursn_bn_bf16_backward_frozen(None, None, 0, None) != 0
