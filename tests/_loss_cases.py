"""Specs and operands shared by tests/test_loss_head_host.py and tests/test_loss_head_gpu.py (plain helper module, no conftest).
Importable without a GPU."""
import numpy as np

from uresnet_amd.losses import LossSpec

# the specs of the GPU tests; the host test checks loss_numpy's analytic gradient against torch autograd for every one of them
SPECS = [("neutral", LossSpec()),
         ("focal2", LossSpec(gamma=2.0)),
         ("smooth", LossSpec(smoothing=0.1)),
         ("focal2_smooth", LossSpec(gamma=2.0, smoothing=0.1)),
         ("dice", LossSpec(dice_weight=1.0)),
         ("focal2_dice_ignore0", LossSpec(gamma=2.0, dice_weight=0.5, ignore_label=0))]
SPEC_IDS = [s[0] for s in SPECS]

VOXELS = (1, 255, 1025, 4099)   # one thread; under one workgroup; one voxel into a second block (head_blocks = cdiv(P, 1024));
#                                 several blocks, odd, a tail that is no multiple of 4
BATCHES = (1, 3)
CLASSES = (1, 2, 3, 4, 5, 8)


def make_case(seed, n, vox, ncls, ties=True):
    """Logits scaled by 3 with exact ties and one voxel whose label logit leads by 30 (q_l within an ulp of 1: the focal
    factor's hard corner), data, label, weight; fp32 arrays.  ``ties=False``: for logits that a BatchNorm produces, where a
    tie of the stored values is a near-tie of the logits and the argmax of an fp32 and an fp64 evaluation may differ.  A case of ONE
    voxel keeps its random logits: the loss of a lone gap-30 voxel is 2e-14, which the head's own statement (m + log(sum)) - z_l
    rounds to 0, and the neutral spec has to be that statement."""
    rng = np.random.default_rng(seed)
    z = (rng.standard_normal((n, vox, ncls)) * 3).astype(np.float32)
    label = rng.integers(0, ncls, (n, vox)).astype(np.float32)
    if ties and vox >= 16:
        z[0, 2:9] = 1.25                      # exact ties: argmax must return the lowest index
    gap = (n - 1, vox // 2)
    if ncls > 1 and n * vox > 1:
        z[gap] = np.linspace(-1.0, 0.5, ncls).astype(np.float32)
        z[gap][int(label[gap])] = z[gap].max() + 30.0
    data = (rng.uniform(0, 1, (n, vox)) * (rng.uniform(0, 1, (n, vox)) > 0.6)).astype(np.float32)
    weight = rng.uniform(0.1, 2.0, (n, vox)).astype(np.float32)
    return z, data, label, weight


def rel_err(a, b):
    """max |a - b| / max |b| (tests/test_ops_gpu.py)."""
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return float(np.abs(a - b).max() / max(np.abs(b).max(), 1e-30))
