"""Every op-level kernel family between NaN guard bands, its scratch at exactly the stated size.

The parity tests (test_ops_gpu.py, test_bf16_ops_gpu.py) hand the kernels plain torch tensors: the caching allocator rounds every
block up and packs live tensors behind it, so a store one row / plane / channel vector past the end, or a load from there that meets
a zero weight, is invisible.  Here every operand of every call is a tests/_guard.py::Guarded -- payload exact to the byte between
two 0xFF (NaN) borders -- and after each call

  * both borders of EVERY operand (inputs too) are still 0xFF                                   (no store outside a tensor),
  * no output element is NaN                        (everything written; no NaN loaded from a border reached the arithmetic),
  * the result agrees with the fp64 oracle at the tolerances of the two parity files (imported, no new numbers),
  * scratch filled 0x00 and scratch filled 0xFF give the same output BITS                       (no read of unwritten scratch),
  * the forward-with-statistics call is accepted at exactly ursn_conv_stats_scratch_bytes(d) and refused, before any launch,
    at 8 bytes less; the weight gradient runs at exactly ursn_conv_wgrad_scratch_bytes(d).

ROWS is the one table: each row names the family ursn_conv_plan must report per pass (None: the row does not run that pass);
tests/test_op_guards_host.py proves on a CPU that every row still reaches the family it names.  Shapes are the smallest ragged
ones the existing lists already prove each family accepts."""
import collections
import ctypes
import functools
import zlib

import numpy as np
import pytest
import torch

from oracle import uresnet_np as O
from _abi import same_bits
from _guard import Guarded, all_written
from _insitu import staged_bn
from _ops import desc, rel_err, stream
from test_bf16_ops_gpu import BF_TOL
from test_ops_gpu import TOL, _join_mask_words
from uresnet_amd import _lib

pytestmark = pytest.mark.gpu
WG_TOL, BF_WG_TOL = 5e-5, 2e-5          # the weight-gradient bounds of test_ops_gpu.py / test_bf16_ops_gpu.py

Row = collections.namedtuple("Row", "tag dtype ndim N S ci co k stride tr algo ex fams")
F, B = 0, 1
ROWS = [Row(*r) for r in [
    # tag, dtype, ndim, N, S, cin, cout, k, stride, transposed, algo, extras, (forward, data gradient, weight gradient)
    # ---- fp32 -----------------------------------------------------------------------------------------------------------------
    ("pconv3d", F, 3, 2, (8, 12, 16), 16, 8, 1, 1, 0, 0, {}, ("pconv", "pconv", "pwgrad")),
    ("pconv3d_odd_split", F, 3, 2, (5, 7, 19), 16, 8, 1, 1, 0, 0, {"split": 8}, ("pconv", "pconv", "pwgrad")),
    ("pconv2d", F, 2, 2, (16, 40), 32, 16, 1, 1, 0, 0, {}, ("pconv", "pconv", "pwgrad")),
    ("pconv2d_split", F, 2, 2, (12, 40), 16, 8, 1, 1, 0, 0, {"split": 8}, ("pconv", "pconv", "pwgrad")),
    ("pconv3d_s2", F, 3, 1, (8, 8, 12), 16, 32, 1, 2, 0, 5, {"acc": (1,)}, ("pconv", "pconv", "pwgrad")),
    ("pconv3d_grid", F, 3, 2, (7, 9, 27), 16, 8, 1, 1, 0, 0, {}, ("pconv", "pconv", "pwgrad")),      # four workgroups by default (tests/_partitions.py caps them)
    ("dconv3d_odd", F, 3, 1, (5, 7, 9), 128, 64, 3, 1, 0, 0, {}, ("dconv", None, "dwgrad")),
    ("dconv3d_rag", F, 3, 1, (4, 6, 10), 192, 80, 3, 1, 0, 0, {}, ("dconv", None, "dwgrad")),
    ("dconv3d_n2", F, 3, 2, (6, 6, 6), 128, 256, 3, 1, 0, 0, {}, ("dconv", "dconv", "dwgrad")),
    ("dconv3d_dg_odd", F, 3, 1, (5, 7, 9), 128, 128, 3, 1, 0, 0, {}, ("dconv", "dconv", "dwgrad")),
    ("dconv2d_odd", F, 2, 1, (9, 21), 128, 64, 3, 1, 0, 0, {}, ("dconv", None, "dwgrad")),
    ("igemm3d_odd", F, 3, 1, (9, 11, 21), 64, 32, 3, 1, 0, 0, {}, ("igemm", "igemm", "igemm_wgrad")),
    ("igemm3d_smallbox", F, 3, 1, (5, 7, 6), 32, 16, 3, 1, 0, 0, {}, ("igemm", "igemm", "wgrad_mfma")),
    ("igemm3d_smallbox_n2_pw", F, 3, 2, (6, 6, 6), 64, 32, 3, 1, 0, 0, {"pw": 1}, ("igemm", "igemm", "wgrad_mfma")),
    ("igemm3d_n2_pw", F, 3, 2, (8, 8, 32), 64, 32, 3, 1, 0, 0, {"pw": 1}, ("igemm", "igemm", "igemm_wgrad")),
    ("igemm3d_co32", F, 3, 2, (24, 48, 48), 32, 32, 3, 1, 0, 0, {}, ("igemm", "igemm", "igemm_wgrad")),
    ("igemm2d_odd", F, 2, 1, (19, 37), 64, 128, 3, 1, 0, 4, {}, ("igemm", "igemm", "igemm_wgrad")),
    ("igemm2d_n2_pw", F, 2, 2, (32, 48), 32, 16, 3, 1, 0, 0, {"pw": 1}, ("igemm", "igemm", "igemm_wgrad")),
    ("tconv3d_odd", F, 3, 1, (19, 13, 45), 16, 8, 3, 1, 0, 0, {}, ("tconv", "tconv", "twgrad")),
    ("tconv3d_n2", F, 3, 2, (9, 11, 37), 8, 8, 3, 1, 0, 0, {}, ("tconv", "tconv", "twgrad")),
    ("tconv3d_cin1", F, 3, 2, (19, 13, 45), 1, 8, 3, 1, 0, 0, {}, ("tconv", None, "twgrad")),
    ("tconv3d_pad3", F, 3, 2, (16, 16, 32), 8, 3, 3, 1, 0, 0, {"out_cs": 4}, ("tconv", "tconv", "twgrad")),
    ("tconv3d_split", F, 3, 2, (9, 11, 37), 16, 8, 3, 1, 0, 0, {"split": 8}, ("tconv", "tconv", "twgrad")),
    ("tconv3d_norm", F, 3, 2, (9, 11, 37), 16, 16, 3, 1, 0, 0, {"norm": 1}, ("tconv", None, "twgrad")),
    ("tconv3d_norm8", F, 3, 2, (8, 16, 32), 8, 8, 3, 1, 0, 0, {"norm": 1}, ("tconv", None, "twgrad")),
    ("tconv3d_pw", F, 3, 2, (9, 11, 37), 16, 8, 3, 1, 0, 0, {"pw": 1}, (None, "tconv", None)),
    ("tconv3d_pw_split", F, 3, 2, (8, 16, 32), 16, 8, 3, 1, 0, 0, {"pw": 1, "split": 8}, (None, "tconv", None)),
    ("tconv3d_bs1", F, 3, 2, (9, 11, 37), 8, 8, 3, 1, 0, 0, {"bs": 1, "bs_relu": 1}, (None, "tconv", None)),
    ("tconv3d_bs2", F, 3, 2, (9, 11, 37), 8, 8, 3, 1, 0, 0, {"bs": 2, "bs_relu": 2}, (None, "tconv", None)),
    ("tconv3d_bs1_pad3", F, 3, 2, (8, 16, 32), 8, 3, 3, 1, 0, 0, {"bs": 1, "bs_relu": 1, "out_cs": 4}, (None, "tconv", None)),
    ("tconv3d_bs1_split", F, 3, 2, (9, 11, 37), 16, 8, 3, 1, 0, 0, {"bs": 1, "bs_relu": 1, "split": 8}, (None, "tconv", None)),
    ("tconv3d_vdz", F, 3, 2, (9, 11, 37), 8, 8, 3, 1, 0, 0, {"vdz": 1, "vdz_relu": 1}, (None, "tconv", None)),
    ("tconv3d_vdz_bs2", F, 3, 2, (21, 8, 40), 8, 8, 3, 1, 0, 0, {"vdz": 1, "vdz_relu": 0, "bs": 2, "bs_relu": 2}, (None, "tconv", None)),
    ("tconv3d_cblocks", F, 3, 2, (24, 48, 48), 32, 16, 3, 1, 0, 3, {}, ("tconv", "tconv", "twgrad")),
    # a long column, Z = 41: five z segments of 9 planes by default (twgradz: 10 after the plane-pair round-up), and long ragged ones under tests/_partitions.py
    ("tconv3d_long", F, 3, 2, (41, 9, 33), 8, 8, 3, 1, 0, 0, {}, ("tconv", "tconv", "twgrad")),
    ("tconv3d_long_split", F, 3, 2, (41, 9, 33), 16, 8, 3, 1, 0, 0, {"split": 8}, ("tconv", "tconv", "twgrad")),
    ("tconv3d_long_norm", F, 3, 2, (41, 9, 33), 16, 16, 3, 1, 0, 0, {"norm": 1}, ("tconv", None, "twgrad")),
    ("tconv3d_long_pw", F, 3, 2, (41, 9, 33), 16, 8, 3, 1, 0, 0, {"pw": 1}, (None, "tconv", None)),
    ("tconv3d_long_bs2", F, 3, 2, (41, 9, 33), 8, 8, 3, 1, 0, 0, {"bs": 2, "bs_relu": 2}, (None, "tconv", None)),
    ("tconv3d_long_vdz", F, 3, 2, (41, 9, 33), 8, 8, 3, 1, 0, 0, {"vdz": 1, "vdz_relu": 1}, (None, "tconv", None)),
    ("tconv2d_odd", F, 2, 1, (37, 300), 16, 16, 3, 1, 0, 0, {}, ("tconv", "tconv", "twgrad")),
    ("tconv2d_n2", F, 2, 2, (16, 256), 16, 16, 3, 1, 0, 0, {}, ("tconv", "tconv", "twgrad")),
    ("tconv2d_pad5", F, 2, 2, (16, 256), 16, 5, 3, 1, 0, 0, {"out_cs": 8}, ("tconv", "tconv", "twgrad")),
    ("tconv2d_split", F, 2, 2, (16, 256), 16, 8, 3, 1, 0, 0, {"split": 8}, ("tconv", "tconv", "twgrad")),
    ("tconv2d_norm", F, 2, 2, (12, 300), 8, 8, 3, 1, 0, 0, {"norm": 1}, ("tconv", None, "twgrad")),
    ("tconv2d_pw", F, 2, 2, (16, 256), 16, 16, 3, 1, 0, 0, {"pw": 1}, (None, "tconv", None)),
    ("vwgrad3d", F, 3, 2, (10, 7, 70), 8, 3, 3, 1, 0, 0, {"out_cs": 4}, (None, None, "vwgrad")),
    ("vwgrad3d_odd", F, 3, 2, (9, 7, 71), 8, 3, 3, 1, 0, 0, {"out_cs": 4}, (None, None, "vwgrad")),
    ("vwgrad3d_zseg", F, 3, 2, (19, 5, 53), 8, 3, 3, 1, 0, 0, {"out_cs": 4}, (None, None, "vwgrad")),      # two z segments: 10 planes and 9
    ("s2scatter3d_odd", F, 3, 1, (5, 7, 19), 16, 16, 3, 2, 1, 0, {}, ("s2scatter", None, None)),
    ("s2scatter3d_n2", F, 3, 2, (8, 16, 32), 32, 16, 3, 2, 1, 0, {}, ("s2scatter", None, None)),
    ("s2scatter2d_odd", F, 2, 1, (17, 35), 16, 32, 3, 2, 1, 0, {}, ("s2scatter", None, None)),
    ("s2scatter3d_dgrad", F, 3, 1, (10, 14, 38), 16, 16, 3, 2, 0, 0, {}, (None, "s2scatter", None)),
    ("s2scatter2d_dgrad_n2", F, 2, 2, (24, 96), 16, 32, 3, 2, 0, 0, {}, (None, "s2scatter", None)),
    ("s2scatter2d_dgrad_lowodd", F, 2, 1, (38, 150), 16, 32, 3, 2, 0, 0, {}, (None, "s2scatter", None)),
    ("tdeconv3d_odd", F, 3, 1, (9, 11, 37), 16, 8, 3, 2, 1, 0, {}, ("tdeconv", None, None)),
    ("tdeconv3d_n2", F, 3, 2, (8, 16, 32), 16, 8, 3, 2, 1, 0, {}, ("tdeconv", None, None)),
    ("tdeconv2d_odd", F, 2, 1, (9, 300), 16, 8, 3, 2, 1, 0, {}, ("tdeconv", None, None)),
    ("tdeconv3d_zseg", F, 3, 2, (13, 9, 19), 16, 8, 3, 2, 1, 0, {}, ("tdeconv", None, None)),      # low-resolution Z >= 12: two z segments (7 + 6 planes), a seam inside the column
    ("tdeconv2d_zseg", F, 2, 1, (13, 300), 16, 8, 3, 2, 1, 0, {}, ("tdeconv", None, None)),
    ("tdeconv3d_dgrad_rag", F, 3, 1, (18, 22, 74), 8, 16, 3, 2, 0, 0, {}, (None, "tdeconv", None)),
    ("tdeconv3d_dgrad_n2", F, 3, 2, (16, 32, 64), 8, 16, 3, 2, 0, 0, {}, (None, "tdeconv", None)),
    ("tdeconv3d_dgrad_zseg", F, 3, 1, (26, 18, 38), 8, 16, 3, 2, 0, 0, {}, (None, "tdeconv", None)),      # low-resolution (13, 9, 19): 7 + 6 planes
    ("tdeconv3d_pw", F, 3, 2, (18, 22, 74), 8, 16, 3, 2, 0, 0, {"pw": 1}, (None, "tdeconv+pw", None)),
    ("tdeconv3d_pw_cs24", F, 3, 2, (16, 16, 64), 8, 16, 3, 2, 0, 0, {"pw": 1, "pw_cs": 24}, (None, "tdeconv+pw", None)),
    ("tdeconv3d_pw_zseg", F, 3, 2, (30, 16, 34), 8, 16, 3, 2, 0, 0, {"pw": 1}, (None, "tdeconv+pw", None)),      # low-resolution (15, 8, 17): 8 + 7 planes
    ("s2conv3d_odd", F, 3, 1, (17, 21, 45), 16, 32, 3, 2, 0, 0, {}, ("s2conv", None, "s2wgrad")),
    ("s2conv3d_n2", F, 3, 2, (16, 32, 64), 8, 16, 3, 2, 0, 0, {}, ("s2conv", None, "s2wgrad")),
    ("s2conv2d_odd", F, 2, 1, (37, 75), 8, 16, 3, 2, 0, 0, {}, ("s2conv", None, "s2wgrad")),
    ("s2conv3d_tr_odd", F, 3, 1, (9, 11, 37), 32, 16, 3, 2, 1, 0, {}, (None, "s2conv", "s2wgrad")),
    ("s2conv2d_tr_odd", F, 2, 1, (19, 41), 16, 8, 3, 2, 1, 0, {}, (None, "s2conv", "s2wgrad")),
    ("s2conv2d_tr_n2", F, 2, 2, (24, 80), 32, 16, 3, 2, 1, 0, {}, (None, "s2conv", "s2wgrad")),
    ("gconv3d_odd", F, 3, 1, (4, 10, 20), 12, 20, 3, 1, 0, 0, {}, ("gconv_mfma", "gconv_mfma", "wgrad_mfma")),
    ("gconv3d_allodd", F, 3, 2, (5, 7, 9), 12, 20, 3, 1, 0, 0, {}, ("gconv_mfma", "gconv_mfma", "wgrad_mfma")),
    ("gconv3d_s2_n2", F, 3, 2, (8, 12, 16), 8, 16, 3, 2, 0, 2, {}, ("gconv_mfma", "gconv_mfma", "wgrad_mfma")),
    ("gconv2d_n2", F, 2, 2, (8, 8), 16, 5, 3, 1, 0, 0, {}, ("gconv_mfma", "gconv_mfma", "wgrad_mfma")),
    ("gconv3d_tr_n2", F, 3, 2, (4, 6, 8), 16, 8, 3, 2, 1, 2, {}, ("gconv_mfma", "gconv_mfma", "wgrad_mfma")),
    ("naive3d_odd", F, 3, 1, (4, 10, 20), 12, 20, 3, 1, 0, 1, {}, ("naive", "naive", "naive")),
    ("naive3d_allodd", F, 3, 2, (3, 5, 7), 12, 20, 3, 2, 0, 1, {}, ("naive", "naive", "naive")),
    ("naive2d_tr_n2", F, 2, 2, (8, 8), 32, 16, 3, 2, 1, 1, {}, ("naive", "naive", "naive")),
    # ---- bf16 -----------------------------------------------------------------------------------------------------------------
    ("b0conv_odd", B, 3, 2, (9, 21, 37), 1, 8, 3, 1, 0, 0, {}, ("b0conv", None, "b0wgrad")),
    ("b0conv_zseg", B, 3, 1, (40, 18, 34), 1, 8, 3, 1, 0, 0, {}, ("b0conv", None, "b0wgrad")),
    ("b0conv_zseg_odd", B, 3, 1, (41, 9, 70), 1, 8, 3, 1, 0, 0, {}, ("b0conv", None, "b0wgrad")),      # 11 + 11 + 11 + 8 planes by default; one halving gives 21 + 20
    ("bs2k8_n2", B, 3, 2, (8, 12, 36), 8, 16, 3, 2, 0, 0, {}, ("bs2k8", "bdeconv", "bs2k8w")),
    ("bs2k8_odd", B, 3, 1, (7, 11, 35), 8, 16, 3, 2, 0, 0, {}, ("bs2k8", "bconv", "bs2k8w")),
    ("bs2k8_lowodd", B, 3, 1, (14, 22, 70), 8, 16, 3, 2, 0, 0, {}, ("bs2k8", "bdeconv", "bs2k8w")),
    ("bdeconv_n2", B, 3, 2, (4, 6, 18), 16, 8, 3, 2, 1, 0, {}, ("bdeconv", "bs2k8", "bs2k8w")),
    ("bdeconv_odd", B, 3, 1, (3, 5, 17), 16, 8, 3, 2, 1, 0, {}, ("bdeconv", "bs2k8", "bs2k8w")),
    ("bconv_k3s2_odd", B, 3, 1, (7, 9, 21), 16, 32, 3, 2, 0, 0, {}, ("bconv", "bconv", "bwgrad")),
    ("bsconv_k3s2_n2_sc", B, 3, 2, (8, 12, 20), 16, 32, 3, 2, 0, 0, {}, ("bconv", "bsconv", "bwgrad")),
    ("bsconv_k3s2_lowodd", B, 3, 1, (10, 14, 22), 16, 32, 3, 2, 0, 0, {}, ("bconv", "bsconv", "bwgrad")),
    ("bsconv_deconv_n2_sc", B, 3, 2, (6, 8, 12), 32, 16, 3, 2, 1, 0, {}, ("bsconv", "bconv", "bwgrad")),
    ("bsconv_deconv_odd", B, 3, 1, (5, 7, 11), 32, 16, 3, 2, 1, 0, {}, ("bsconv", "bconv", "bwgrad")),
    ("bsconv_deconv_rag_sc", B, 3, 1, (5, 8, 8), 128, 64, 3, 2, 1, 0, {}, ("bsconv", "bconv", "bwgrad")),
    ("bpw_odd", B, 3, 2, (7, 9, 37), 16, 8, 1, 1, 0, 0, {}, ("bpw", "bpw", "bwgrad")),
    ("bconv_k1s2_n2", B, 3, 2, (8, 12, 36), 8, 16, 1, 2, 0, 0, {}, ("bconv", "bconv", "bwgrad")),
    ("b3conv_odd", B, 3, 2, (9, 21, 37), 8, 8, 3, 1, 0, 0, {}, ("b3conv", "b3conv", "b3wgrad")),
    ("b3conv_16_8_odd", B, 3, 2, (11, 19, 35), 16, 8, 3, 1, 0, 0, {}, ("b3conv", "b3conv", "b3wgrad")),
    ("b3conv_16_16_zseg", B, 3, 1, (36, 9, 40), 16, 16, 3, 1, 0, 0, {}, ("b3conv", "b3conv", "b3wgrad")),
    ("b3conv_norm_odd", B, 3, 2, (9, 21, 37), 8, 8, 3, 1, 0, 0, {"norm": 1}, ("b3conv", None, "b3wgrad")),
    ("b3conv_norm_relu_odd", B, 3, 2, (11, 19, 35), 16, 16, 3, 1, 0, 0, {"norm": 1, "in_relu": 1}, ("b3conv", None, "b3wgrad")),
    ("b3conv_norm_zseg", B, 3, 1, (37, 9, 33), 8, 8, 3, 1, 0, 0, {"norm": 1, "in_relu": 1}, ("b3conv", None, "b3wgrad")),      # Z >= 36: more than one z segment
    ("b3conv_pw_odd", B, 3, 2, (9, 21, 37), 16, 8, 3, 1, 0, 0, {"pw": 1}, (None, "b3conv", None)),
    ("b3conv_pw_split_zseg", B, 3, 1, (40, 10, 34), 16, 8, 3, 1, 0, 0, {"pw": 1, "split": 8, "acc": (0,)}, (None, "b3conv", None)),
    ("bcbconv_odd_cb", B, 3, 2, (9, 21, 37), 32, 32, 3, 1, 0, 0, {}, ("bcbconv", "bcbconv", "bwgrad")),
    ("bcbconv_16_24_cb", B, 3, 2, (7, 11, 33), 16, 24, 3, 1, 0, 0, {}, ("bcbconv", "bconv", "bwgrad")),
    ("bcbconv_pw_odd", B, 3, 2, (9, 21, 37), 32, 16, 3, 1, 0, 0, {"pw": 1}, (None, "bcbconv", None)),
    ("bdconv_rag_dp", B, 3, 1, (5, 12, 21), 128, 64, 3, 1, 0, 0, {}, ("bdconv", "bdconv", "bdwgrad")),
    ("bdconv_odd_dp", B, 3, 1, (5, 11, 21), 128, 64, 3, 1, 0, 0, {}, ("bdconv", "bdconv", "bdwgrad")),
    ("bdconv_n4_dp", B, 3, 4, (8, 8, 8), 64, 64, 3, 1, 0, 0, {}, ("bdconv", "bdconv", "bdwgrad")),
    ("bconv_24_40", B, 3, 1, (4, 6, 20), 24, 40, 3, 1, 0, 0, {}, ("bconv", "bconv", "bwgrad")),
    ("b3conv_8_16", B, 3, 1, (6, 10, 33), 8, 16, 3, 1, 0, 0, {}, ("b3conv", "b3conv", "bwgrad")),
    ("bconv2d_n2", B, 2, 2, (24, 70), 16, 16, 3, 1, 0, 0, {}, ("bconv", "bconv", "bwgrad")),
    ("bconv2d_s2_n2", B, 2, 2, (24, 70), 16, 32, 3, 2, 0, 0, {}, ("bconv", "bconv", "bwgrad")),
    ("bconv2d_deconv", B, 2, 1, (12, 20), 32, 16, 3, 2, 1, 0, {}, ("bconv", "bconv", "bwgrad")),
]]
BY_TAG = {r.tag: r for r in ROWS}
assert len(BY_TAG) == len(ROWS)
# every family ursn_conv_plan can name, per pass it serves (the host test checks the table covers them)
FAMILIES = {
    (F, 0): {"pconv", "dconv", "igemm", "tconv", "s2scatter", "tdeconv", "s2conv", "gconv_mfma", "naive"},
    (F, 1): {"pconv", "dconv", "igemm", "tconv", "s2scatter", "tdeconv", "tdeconv+pw", "s2conv", "gconv_mfma", "naive"},
    (F, 2): {"twgrad", "pwgrad", "dwgrad", "igemm_wgrad", "vwgrad", "s2wgrad", "wgrad_mfma"},
    (B, 0): {"b0conv", "bs2k8", "bdeconv", "bsconv", "bpw", "b3conv", "bcbconv", "bdconv", "bconv"},
    (B, 1): {"bs2k8", "bdeconv", "bsconv", "bpw", "b3conv", "bcbconv", "bdconv", "bconv"},
    (B, 2): {"b0wgrad", "b3wgrad", "bdwgrad", "bs2k8w", "bwgrad"},
}
# kernel names the parity files assert after a call of these families (startswith)
KERNEL_PREFIX = {"dconv": b"dconv", "dwgrad": b"dwgrad", "tdeconv+pw": b"tdeconv<16,", "b0conv": b"b0conv_bf16", "b0wgrad": b"b0wgrad_bf16",
                 "bcbconv": b"bcbconv_bf16", "bdconv": b"bdconv_bf16", "bsconv": b"bsconv_bf16", "bdwgrad": b"bdwgrad_bf16"}
# the families a forced ursn_conv_desc.algo stands for (conv_dispatch / wgrad_dispatch; 1 is the naive reference the plan never names)
FORCED = {1: {"naive"}, 2: {"gconv_mfma", "wgrad_mfma"}, 3: {"tconv", "tdeconv", "twgrad"}, 4: {"igemm", "igemm_wgrad"},
          5: {"pconv", "pwgrad"}, 6: {"s2conv", "s2wgrad"}, 7: {"s2scatter"}}
DUMMY = 0x1000      # "a pointer is set" for the host-only queries


def odd_grid(row, ps):
    """Every extent of the grid the pass's kernel walks is odd (so no multiple of any tile extent).  The scatter-type data gradient
    of a stride-2 conv walks the LOW-resolution grid and these families take even full-resolution extents only."""
    S = tuple((v + 1) // 2 for v in row.S) if ps == 1 and row.stride == 2 and not row.tr and row.fams[1] not in ("gconv_mfma", "naive", "bconv", "pconv") else row.S
    return all(v % 2 for v in S)


def rows_for(ps):
    return [r.tag for r in ROWS if r.fams[ps] is not None]


def plan_name(row, ps, d=None):
    """The family ursn_conv_plan reports (algo 1 is the naive reference: the plan does not know it, the dispatcher checks it first)."""
    lib = _lib.load()
    d = build_desc(row, ps) if d is None else d
    buf = ctypes.create_string_buffer(32)
    _lib.check(lib.ursn_conv_plan(ctypes.byref(d), ps, buf, 32))
    return buf.value.decode()


def build_desc(row, ps, ptr=lambda name: DUMMY):
    """The descriptor of pass ps (0 forward, 1 data gradient, 2 weight gradient) with the fused forms that pass takes."""
    ex, bf = row.ex, row.dtype == B
    d = desc(row.ndim, row.N, row.S, row.ci, row.co, row.k, row.stride, transposed=row.tr, out_cs=ex.get("out_cs", 0), algo=row.algo)
    d.dtype = row.dtype
    h = ex.get("split", 0)
    if h and (not bf or ps == 1):
        d.in_split = h
        if not bf:
            d.in_cstride, d.in2_cstride = h, row.ci - h
        if ps == 1:
            d.dx2 = ptr("dx2")
        else:
            d.x2 = ptr("x2")
    if ex.get("norm") and ps != 1:
        d.in_mean, d.in_rstd, d.in_beta, d.in_relu = ptr("in_mean"), ptr("in_rstd"), ptr("in_beta"), ex.get("in_relu", 0)
    if ps == 1:
        if ex.get("pw"):
            d.pw_dy, d.pw_w, d.pw_dy_cstride = ptr("pw_dy"), ptr("pw_w"), ex.get("pw_cs", 0)
        if ex.get("bs"):
            d.bs_z, d.bs_mean, d.bs_rstd, d.bs_z_cstride, d.bs_relu = ptr("bs_z"), ptr("bs_mean"), ptr("bs_rstd"), 8, ex["bs_relu"]
            if ex["bs_relu"] == 1:
                d.bs_beta = ptr("bs_beta")
            if ex["bs_relu"] == 2:
                d.bs_mask = ptr("bs_mask")
            if ex["bs"] == 2:
                d.bs_z2, d.bs_mean2, d.bs_rstd2, d.bs_z2_cstride = ptr("bs_z2"), ptr("bs_mean2"), ptr("bs_rstd2"), 8
            d.bs_partial = ptr("bs_partial")
        if ex.get("vdz"):
            d.vdz_z, d.vdz_coef, d.vdz_out, d.vdz_relu = ptr("vdz_z"), ptr("vdz_coef"), ptr("vdz_out"), ex.get("vdz_relu", 0)
    return d


# ---- operands and references: computed once per row, shared by the three passes, never modified ---------------------------------
def _f32(a):
    return np.asarray(a, np.float32).astype(np.float64)


@functools.lru_cache(maxsize=None)
def case(tag):
    row = BY_TAG[tag]
    ex, bf, nd = row.ex, row.dtype == B, row.ndim
    rng = np.random.default_rng(zlib.crc32(tag.encode()))
    q = (lambda a: O.bf16_round(np.asarray(a, np.float64))) if bf else _f32      # what the kernel reads, exactly
    c = {}
    in_shape = (row.N,) + row.S + (row.ci,)
    if ex.get("norm"):
        c["z"] = q(rng.standard_normal(in_shape) * 1.7 + 0.8)
        c["in_mean"], c["in_rstd"] = _f32(rng.standard_normal(row.ci) * 0.5 + 0.8), _f32(rng.uniform(0.4, 1.6, row.ci))
        c["in_beta"] = _f32(rng.standard_normal(row.ci) * 0.3)
        if bf:
            x = staged_bn(c["z"], c["in_mean"], c["in_rstd"], c["in_beta"], ex.get("in_relu", 0))
        else:
            x = (c["z"] - c["in_mean"]) * c["in_rstd"] + c["in_beta"]
    elif bf and row.ci == 1:      # conv0 of the bf16 plan reads the fp32 data, staged as bf16
        c["x32"] = (rng.uniform(0, 4, in_shape) * (rng.uniform(0, 1, in_shape) > 0.6)).astype(np.float32)
        x = O.bf16_round(c["x32"].astype(np.float64))
    else:
        x = q(rng.standard_normal(in_shape))
    wscale = 0.05 if row.ci >= 128 else 0.1 if row.ci >= 32 else 0.2
    w = q(rng.standard_normal((row.k,) * nd + ((row.co, row.ci) if row.tr else (row.ci, row.co))) * wscale)
    y = O.deconv_fwd(x, w) if row.tr else O.conv_fwd(x, w, row.stride)
    dy = q(rng.standard_normal(y.shape))
    if ex.get("vdz"):      # `dy` is g, the gradient at the BatchNorm's output; the kernel forms dz on load (test_ops_gpu.py)
        ax = tuple(range(nd + 1))
        z = _f32(rng.standard_normal(y.shape) * 1.7 + 0.8)
        beta = _f32(rng.standard_normal(row.co) * 0.4)
        mean, rstd = z.mean(axis=ax), 1.0 / np.sqrt(z.var(axis=ax) + 1e-3)
        f = lambda a: np.asarray(a, dtype=np.float32)   # noqa: E731
        S32, T32 = f(rstd), f(beta) - f(mean) * f(rstd)
        keep = (f(z) * S32 + T32) > 0 if ex.get("vdz_relu") else np.ones(y.shape, dtype=bool)
        gm = dy * keep
        xhat = (z - mean) * rstd
        c1, c2 = gm.mean(axis=ax), (gm * xhat).mean(axis=ax)
        c["vdz_z"], c["dz"] = z, rstd * (gm - c1 - xhat * c2)
        c["vdz_coef"] = np.stack([f(rstd), -(f(rstd) * f(rstd)) * f(c2), -f(rstd) * f(c1), f(mean), S32, T32]).astype(np.float32)
        dx, dw = (O.deconv_bwd if row.tr else lambda a, b, g: O.conv_bwd(a, b, row.stride, g))(x, w, c["dz"])
    else:
        dx, dw = O.deconv_bwd(x, w, dy) if row.tr else O.conv_bwd(x, w, row.stride, dy)
    if ex.get("pw"):
        c["pw_w"] = q(rng.standard_normal((1,) * nd + (row.ci, row.co)) * 0.3)
        c["pw_dy"] = q(rng.standard_normal(y.shape))
        c["dx_pw"] = dx + O.conv_bwd(x, c["pw_w"], row.stride, c["pw_dy"])[0]
    if ex.get("bs"):
        ax = tuple(range(nd + 1))
        zs = (row.N,) + row.S + (8,)
        c["bs_z"], c["bs_z2"] = _f32(rng.standard_normal(zs) * 1.5 + 0.3), _f32(rng.standard_normal(zs) * 0.7 - 0.2)
        for s in ("", "2"):
            z = c["bs_z" + s]
            c["bs_mean" + s], c["bs_rstd" + s] = _f32(z.mean(axis=ax)), _f32(1.0 / np.sqrt(z.var(axis=ax) + 1e-3))
        c["bs_beta"] = _f32(rng.standard_normal(8) * 0.3)
        f = lambda a: np.asarray(a, dtype=np.float32)   # noqa: E731
        if ex["bs_relu"] == 1:      # the kernel's own fp32 expression, so both sides agree on borderline elements
            c["bs_keep"] = (f(c["bs_z"]) * f(c["bs_rstd"]) + (f(c["bs_beta"]) - f(c["bs_mean"]) * f(c["bs_rstd"]))) > 0
        elif ex["bs_relu"] == 2:
            c["bs_keep"] = rng.random(zs) < 0.6
        else:
            c["bs_keep"] = np.ones(zs, dtype=bool)
        c["bs_mask"] = _join_mask_words(c["bs_keep"]).view(np.int64)
    c.update(x=x, w=w, y=y, dy=dy, dx=dx, dw=dw, base=q(rng.standard_normal(in_shape)))
    for v in c.values():
        v.setflags(write=False)
    return c


def _tdt(row):
    return torch.bfloat16 if row.dtype == B else torch.float32


def _padded(a, cs, fill=0.0):
    """[..., C] -> [..., cs] with `fill` in the pad lanes (cs = 0 / C: unchanged)."""
    if not cs or cs == a.shape[-1]:
        return a
    out = np.full(a.shape[:-1] + (cs,), fill, dtype=a.dtype)
    out[..., :a.shape[-1]] = a
    return out


def inputs(row, ps):
    """name -> Guarded for every INPUT operand of pass ps."""
    c, ex, dt, bf = case(row.tag), row.ex, _tdt(row), row.dtype == B
    ops = {}
    G = lambda a, t=dt: Guarded(a.shape, t, values=a)   # noqa: E731
    if ps in (0, 2):
        src = c["z"] if ex.get("norm") else c["x"]
        h = ex.get("split", 0)
        if bf and row.ci == 1:
            ops["x"] = G(c["x32"], torch.float32)
        elif h and not bf:
            ops["x"], ops["x2"] = G(np.ascontiguousarray(src[..., :h])), G(np.ascontiguousarray(src[..., h:]))
        else:
            ops["x"] = G(src)
        if ex.get("norm"):
            for k in ("in_mean", "in_rstd", "in_beta"):
                ops[k] = G(c[k], torch.float32)
    if ps == 0:
        ops["w"] = G(c["w"], torch.float32)
    if ps == 2:
        ops["dy"] = G(_padded(c["dy"], ex.get("out_cs", 0)))
    if ps == 1:
        ops["dy"] = G(_padded(c["dy"], ex.get("out_cs", 0)))
        ops["w"] = G(c["w"], torch.float32)
        if ex.get("pw"):
            ops["pw_dy"] = G(_padded(c["pw_dy"], ex.get("pw_cs", 0), np.nan))      # the stride's pad lanes are never read
            ops["pw_w"] = G(c["pw_w"].reshape(row.ci, row.co), torch.float32)
        if ex.get("bs"):
            for k in ("bs_z", "bs_mean", "bs_rstd") + (("bs_beta",) if ex["bs_relu"] == 1 else ()) + \
                    (("bs_z2", "bs_mean2", "bs_rstd2") if ex["bs"] == 2 else ()):
                ops[k] = G(c[k], torch.float32)
            if ex["bs_relu"] == 2:
                ops["bs_mask"] = G(c["bs_mask"], torch.int64)
        if ex.get("vdz"):
            ops["vdz_z"], ops["vdz_coef"] = G(c["vdz_z"], torch.float32), G(c["vdz_coef"], torch.float32)
    return ops


def check_all(ops, when):
    for name, g in ops.items():
        g.check("%s (%s)" % (name, when))


def _ptr(ops):
    return lambda name: ops[name].ptr if name in ops else DUMMY


def _P(g):
    return ctypes.c_void_p(g.ptr)


def check_family(row, ps, d=None):
    """ursn_conv_plan describes the automatic dispatch (algo 0) and must name the row's family; a forced algo names its family
    itself (and refuses a shape that family does not take)."""
    want = row.fams[ps]
    if row.algo == 0:
        got = plan_name(row, ps, d)
        assert got == want, (row.tag, ps, got, want)
    else:
        assert want in FORCED[row.algo], (row.tag, ps, want)


def _assert_family(lib, row, ps, d):
    check_family(row, ps, d)
    return KERNEL_PREFIX.get(row.fams[ps])


def _assert_kernel(lib, prefix, row, extra=b""):
    name = lib.ursn_last_kernel_name()
    if prefix is not None:
        assert name.startswith(prefix), (row.tag, name)
    assert name.endswith(extra), (row.tag, name)


def _close(row, got, want, what):
    if row.dtype == B:
        e = np.abs(got - want).max() / np.abs(want).max()
        assert e <= BF_TOL, (row.tag, what, e)
    else:
        e = rel_err(got, want)
        assert e < TOL, (row.tag, what, e)


# ---- forward with fused statistics ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("tag", rows_for(0))
def test_forward_with_statistics_at_the_exact_scratch_size(tag):
    row, lib = BY_TAG[tag], _lib.load()
    c, ex, co = case(tag), row.ex, row.co
    ops = inputs(row, 0)
    d = build_desc(row, 0, _ptr(ops))
    prefix = _assert_family(lib, row, 0, d)
    ocs = ex.get("out_cs", 0) or co
    yshape = c["y"].shape[:-1] + (ocs,)
    need = lib.ursn_conv_stats_scratch_bytes(ctypes.byref(d))
    if row.dtype == B and row.tr:      # bf16 transposed convs take their statistics at net level: the query says 0, the call is refused
        assert need == 0
        one = Guarded((8,), torch.uint8)
        y = Guarded(yshape, _tdt(row))
        assert lib.ursn_conv_forward_stats(ctypes.byref(d), _P(ops["x"]), _P(ops["w"]), _P(y), _P(one), _P(one), 1e-3, _P(one), 8, stream()) != 0
        _lib.check(lib.ursn_conv_forward(ctypes.byref(d), _P(ops["x"]), _P(ops["w"]), _P(y), stream()))
        check_all(dict(ops, y=y), "forward")
        _assert_kernel(lib, prefix, row)
        all_written(y, "y")
        _close(row, y.numpy(), c["y"], "y")
        return
    assert need > 0 and need % 8 == 0, need
    runs = []
    for fill in (0x00, 0xFF):
        out = {"y": Guarded(yshape, _tdt(row)), "mean": Guarded((co,), torch.float32), "rstd": Guarded((co,), torch.float32),
               "scratch": Guarded((need,), torch.uint8).fill(fill)}
        both = dict(ops, **out)
        if fill == 0x00:      # 8 bytes less: refused before any launch
            rc = lib.ursn_conv_forward_stats(ctypes.byref(d), _P(ops["x"]), _P(ops["w"]), _P(out["y"]), _P(out["mean"]), _P(out["rstd"]),
                                             1e-3, _P(out["scratch"]), need - 8, stream())
            assert rc != 0 and b"scratch too small" in lib.ursn_last_error(), (tag, rc, lib.ursn_last_error())
            torch.cuda.synchronize()
            assert bool((out["y"].bytes == 0xFF).all()) and bool((out["mean"].bytes == 0xFF).all()), "a refused call launched"
        _lib.check(lib.ursn_conv_forward_stats(ctypes.byref(d), _P(ops["x"]), _P(ops["w"]), _P(out["y"]), _P(out["mean"]), _P(out["rstd"]),
                                               1e-3, _P(out["scratch"]), need, stream()))
        check_all(both, "forward, scratch 0x%02X" % fill)
        _assert_kernel(lib, prefix, row)
        for k in ("y", "mean", "rstd"):
            all_written(out[k], k)
        runs.append({k: out[k].numpy() for k in ("y", "mean", "rstd")})
    for k in ("y", "mean", "rstd"):
        assert same_bits(runs[0][k], runs[1][k]), (tag, k, "depends on what the scratch held")
    y = runs[0]["y"]
    _close(row, y[..., :co], c["y"], "y")
    assert np.all(y[..., co:] == 0), "pad lanes of a padded output"
    ys = y[..., :co].astype(np.float64) if row.dtype == B else c["y"]      # bf16: the statistics of the STORED tensor
    ax = tuple(range(ys.ndim - 1))
    mu, var = ys.mean(axis=ax), ys.var(axis=ax)
    e_mu = np.abs(runs[0]["mean"] - mu).max()
    print("%s: mean err %.2e (std %.2e), rstd rel err %.2e, scratch %d bytes" % (
        tag, e_mu, np.sqrt(var.max()), rel_err(runs[0]["rstd"], 1 / np.sqrt(var + 1e-3)), need))
    if row.dtype == B:
        assert e_mu < 1e-5 * np.sqrt(var.max()) + 1e-6 * np.abs(mu).max()
    else:
        assert e_mu < 1e-5 * np.sqrt(var.max())
    assert rel_err(runs[0]["rstd"], 1 / np.sqrt(var + 1e-3)) < 1e-5


# ---- data gradient, overwrite and accumulate ------------------------------------------------------------------------------------
@pytest.mark.parametrize("tag", rows_for(1))
def test_data_gradient_overwrite_and_accumulate(tag):
    row, lib = BY_TAG[tag], _lib.load()
    c, ex, dt, bf = case(tag), row.ex, _tdt(row), row.dtype == B
    ops = inputs(row, 1)
    h = ex.get("split", 0)
    dx_ref = c["dx_pw"] if ex.get("pw") else c["dx"]
    in_shape = dx_ref.shape
    ax = tuple(range(row.ndim + 1))
    for acc in ex.get("acc", (0, 1)):
        base = c["base"] if acc else None
        out = {}
        if h:
            out["dx"] = Guarded(in_shape[:-1] + (h,), dt, None if base is None else np.ascontiguousarray(base[..., :h]))
            out["dx2"] = Guarded(in_shape[:-1] + (row.ci - h,), dt, None if base is None else np.ascontiguousarray(base[..., h:]))
        else:
            out["dx"] = Guarded(in_shape, dt, base)
        both = dict(ops, **out)
        d = build_desc(row, 1, _ptr(both))
        if ex.get("bs"):
            nb = lib.ursn_conv_bs_blocks(ctypes.byref(d))
            assert nb > 0
            out["bs_partial"] = both["bs_partial"] = Guarded((nb, 3, 8), torch.float64)      # blocks x 3 x (channels of dx) doubles, exactly
            d.bs_partial = out["bs_partial"].ptr
        if ex.get("vdz"):
            out["vdz_out"] = both["vdz_out"] = Guarded(c["dy"].shape, torch.float32)
            d.vdz_out = out["vdz_out"].ptr
        prefix = _assert_family(lib, row, 1, d)
        _lib.check(lib.ursn_conv_backward_data(ctypes.byref(d), _P(ops["dy"]), _P(ops["w"]), _P(out["dx"]), acc, stream()))
        check_all(both, "data gradient, accumulate %d" % acc)
        if not acc or row.fams[1] == "tdeconv+pw":
            _assert_kernel(lib, prefix, row, b"+pw" if row.fams[1] == "tdeconv+pw" else b"")
        if ex.get("vdz"):
            assert lib.ursn_last_kernel_name().startswith(b"tconv_dgrad<8,8>+dz")
        for k, g in out.items():
            all_written(g, k)
        got = np.concatenate([out["dx"].numpy(), out["dx2"].numpy()], axis=-1) if h else out["dx"].numpy()
        want = dx_ref + (base if acc else 0.0)
        _close(row, got, want, "dx, accumulate %d" % acc)
        if ex.get("vdz"):
            assert rel_err(out["vdz_out"].numpy(), c["dz"]) < 1e-5
        if ex.get("bs"):
            keep = c["bs_keep"]
            g = want[..., :8] * keep
            sums = out["bs_partial"].numpy().sum(axis=0)
            ref = np.stack([g.sum(axis=ax), (g * (c["bs_z"] - c["bs_mean"]) * c["bs_rstd"]).sum(axis=ax),
                            (g * (c["bs_z2"] - c["bs_mean2"]) * c["bs_rstd2"]).sum(axis=ax)])
            k = 3 if ex["bs"] == 2 else 2
            assert np.abs(sums[:k] - ref[:k]).max() < 1e-6 * np.abs(g).sum(axis=ax).max()


# ---- weight gradient at exactly ursn_conv_wgrad_scratch_bytes -------------------------------------------------------------------
@pytest.mark.parametrize("tag", rows_for(2))
def test_weight_gradient_at_the_exact_scratch_size(tag):
    row, lib = BY_TAG[tag], _lib.load()
    c = case(tag)
    ops = inputs(row, 2)
    d = build_desc(row, 2, _ptr(ops))
    prefix = _assert_family(lib, row, 2, d)
    need = lib.ursn_conv_wgrad_scratch_bytes(ctypes.byref(d))
    assert need > 0
    tol = BF_WG_TOL if row.dtype == B else WG_TOL
    runs = []
    for fill in (0x00, 0xFF):
        out = {"dw": Guarded(c["dw"].shape, torch.float32, np.zeros(c["dw"].shape)), "scratch": Guarded((need,), torch.uint8).fill(fill)}
        both = dict(ops, **out)
        for rep in (1, 2) if fill == 0x00 else (1,):      # dw accumulates (assign_add)
            _lib.check(lib.ursn_conv_backward_weight(ctypes.byref(d), _P(ops["x"]), _P(ops["dy"]), _P(out["dw"]), _P(out["scratch"]), need,
                                                     stream()))
            check_all(both, "weight gradient, scratch 0x%02X, call %d" % (fill, rep))
            _assert_kernel(lib, prefix, row)
            all_written(out["dw"], "dw")
            got = out["dw"].numpy().copy()
            e = rel_err(got, rep * c["dw"])
            assert e < tol, (tag, rep, e)
            if rep == 1:
                runs.append(got)
    assert same_bits(runs[0], runs[1]), (tag, "dw depends on what the scratch held")


# ---- positive control: the check sees a real kernel's store ---------------------------------------------------------------------
@pytest.mark.parametrize("tag", ["tconv3d_n2", "b3conv_odd"])
def test_a_store_behind_the_payload_is_reported(tag):
    """The output is declared with N - 1 images (its borders hold more than one whole image) and the kernel is called with N: every
    store lands inside the allocation, the last image in the back border."""
    row, lib = BY_TAG[tag], _lib.load()
    c = case(tag)
    assert row.N >= 2
    ops = inputs(row, 0)
    d = build_desc(row, 0, _ptr(ops))
    y = Guarded((row.N - 1,) + c["y"].shape[1:], _tdt(row))
    image_bytes = y.nbytes // (row.N - 1)
    assert min(b.numel() for b in y.borders()) >= image_bytes
    _lib.check(lib.ursn_conv_forward(ctypes.byref(d), _P(ops["x"]), _P(ops["w"]), _P(y), stream()))
    with pytest.raises(AssertionError, match="border"):
        y.check("y")
    check_all(ops, "positive control")      # the inputs are untouched all the same
    all_written(y, "y")


# ---- the other op-level entry points --------------------------------------------------------------------------------------------
V_BN = 4 * 6 * 10 * 3
V_BN_BLOCKS = 5 * 7 * 9 * 11      # odd, and 4 (8 channels) to 28 (64 channels) blocks of the reduce kernels where V_BN gives 1 to 6
BN_CASES = [(3, 0, False), (8, 1, False), (12, 1, False), (64, 0, True)]


@pytest.mark.parametrize("C,relu,res", BN_CASES)
def test_bn_forward_backward_and_frozen_backward(C, relu, res, V=V_BN):
    lib = _lib.load()
    rng = np.random.default_rng(C)
    z = _f32(rng.standard_normal((V, C)) * 2.0 + 0.5)
    beta = _f32(rng.standard_normal(C) * 0.3)
    r = _f32(rng.standard_normal((V, C))) if res else None
    y, cache = O.bn_fwd(z, beta)
    y = np.maximum(y + r if res else y, 0) if relu else (y + r if res else y)
    dy = _f32(rng.standard_normal((V, C)))
    nb = lib.ursn_bn_scratch_bytes(V, C)
    G = lambda a: Guarded(a.shape, torch.float32, values=a)   # noqa: E731
    ops = {"z": G(z), "beta": G(beta), "dy": G(dy)}
    if res:
        ops["res"] = G(r)
    fwd, bwd, frz = [], [], []
    for fill in (0x00, 0xFF):
        out = {"y": Guarded((V, C), torch.float32), "stats": Guarded((2 * C,), torch.float32), "scratch": Guarded((nb,), torch.uint8).fill(fill)}
        both = dict(ops, **out)
        _lib.check(lib.ursn_bn_forward(_P(ops["z"]), _P(ops["beta"]), _P(ops["res"]) if res else None, _P(out["y"]), V, C, 1e-3, relu,
                                       _P(out["stats"]), _P(out["scratch"]), nb, stream()))
        check_all(both, "bn forward")
        all_written(out["y"], "y"), all_written(out["stats"], "stats")
        fwd.append((out["y"].numpy(), out["stats"].numpy()))
        # backward (batch statistics), mask from the stored y
        out2 = {"dz": Guarded((V, C), torch.float32), "dbeta": Guarded((C,), torch.float32, np.zeros(C))}
        out["scratch"].fill(fill)
        both = dict(both, **out2)
        _lib.check(lib.ursn_bn_backward(_P(ops["dy"]), _P(out["y"]), _P(ops["z"]), _P(out2["dz"]), _P(out2["dbeta"]), V, C, 1e-3, relu,
                                        _P(out["scratch"]), nb, stream()))
        check_all(both, "bn backward")
        all_written(out2["dz"], "dz"), all_written(out2["dbeta"], "dbeta")
        bwd.append((out2["dz"].numpy(), out2["dbeta"].numpy()))
        # backward through FIXED statistics
        st = {"mean": Guarded((C,), torch.float32, out["stats"].tensor[:C].clone()), "rstd": Guarded((C,), torch.float32, out["stats"].tensor[C:].clone())}
        out3 = {"dz": Guarded((V, C), torch.float32), "dbeta": Guarded((C,), torch.float32, np.zeros(C))}
        out["scratch"].fill(fill)
        both = dict(ops, y=out["y"], scratch=out["scratch"], **st, **{"f" + k: v for k, v in out3.items()})
        _lib.check(lib.ursn_bn_backward_frozen(_P(ops["dy"]), _P(out["y"]) if relu else None, _P(ops["z"]), _P(st["mean"]), _P(st["rstd"]),
                                               _P(ops["beta"]), _P(out3["dz"]), _P(out3["dbeta"]), V, C, relu, _P(out["scratch"]), nb, stream()))
        check_all(both, "bn backward, frozen")
        all_written(out3["dz"], "dz"), all_written(out3["dbeta"], "dbeta")
        frz.append((out3["dz"].numpy(), out3["dbeta"].numpy()))
    for a, b in zip(fwd[0] + bwd[0] + frz[0], fwd[1] + bwd[1] + frz[1]):
        assert same_bits(a, b), "depends on what the scratch held"
    assert rel_err(fwd[0][0], y) < 1e-5
    assert rel_err(fwd[0][1][C:], cache[1]) < 1e-5
    g = dy * (y > 0) if relu else dy
    dz, dbeta = O.bn_bwd(cache, g)
    assert rel_err(bwd[0][0], dz) < 2e-5 and rel_err(bwd[0][1], dbeta) < 2e-5
    rstd = fwd[0][1][C:].astype(np.float64)
    assert rel_err(frz[0][0], rstd * g) < 2e-5 and rel_err(frz[0][1], g.sum(0)) < 2e-5


@pytest.mark.parametrize("C,relu,res", BN_CASES)
def test_bn_forward_backward_and_frozen_backward_on_several_blocks(C, relu, res):
    test_bn_forward_backward_and_frozen_backward(C, relu, res, V=V_BN_BLOCKS)


def _mask_bytes(y):
    m = (y.reshape(-1, y.shape[-1] // 8, 8) > 0).astype(np.uint8)
    return (m << np.arange(8, dtype=np.uint8)).sum(axis=-1).astype(np.uint8)


@pytest.mark.parametrize("C", [8, 16, 32])
@pytest.mark.parametrize("form", ["join_identity", "join_conv_shortcut"])
def test_bf16_bn_join_forward_backward_and_frozen_backward(C, form):
    """The residual join of the bf16 plan (test_bf16_ops_gpu.py): out = relu(bn(z) + x | + bn2(z2)) with its mask bytes, and the
    backward from them -- dz and the identity share dres, or dz2 / d(beta2) of the second BatchNorm -- on batch statistics and on
    fixed statistics, scratch exactly ursn_bn_bf16_scratch_bytes."""
    lib, V = _lib.load(), 3 * 7 * 9 * 41
    two = form == "join_conv_shortcut"
    rng = np.random.default_rng(C + 5 + two)
    rb = lambda a: O.bf16_round(np.asarray(a, np.float64))   # noqa: E731
    z, dy = rb(rng.standard_normal((V, C)) * 1.5 + 0.3), rb(rng.standard_normal((V, C)))
    mean, rstd = _f32(z.mean(0)), _f32(1 / np.sqrt(z.var(0) + 1e-3))
    beta = _f32(rng.standard_normal(C) * 0.3)
    Gf = lambda a: Guarded(a.shape, torch.float32, values=a)   # noqa: E731
    Gb = lambda a: Guarded(a.shape, torch.bfloat16, values=a)   # noqa: E731
    ops = {"z": Gb(z), "dy": Gb(dy), "mean": Gf(mean), "rstd": Gf(rstd), "beta": Gf(beta)}
    d = _lib.ursn_bn_bf16_desc()
    d.voxels, d.channels, d.relu = V, C, 1
    d.z, d.mean, d.rstd, d.beta = ops["z"].ptr, ops["mean"].ptr, ops["rstd"].ptr, ops["beta"].ptr
    if two:
        z2 = rb(rng.standard_normal((V, C)) * 0.7 - 0.2)
        mean2, rstd2, beta2 = _f32(z2.mean(0)), _f32(1 / np.sqrt(z2.var(0) + 1e-3)), _f32(rng.standard_normal(C) * 0.3)
        ops.update(z2=Gb(z2), mean2=Gf(mean2), rstd2=Gf(rstd2), beta2=Gf(beta2))
        d.z2, d.mean2, d.rstd2, d.beta2 = ops["z2"].ptr, ops["mean2"].ptr, ops["rstd2"].ptr, ops["beta2"].ptr
        yref = np.maximum((z - mean) * rstd + beta + (z2 - mean2) * rstd2 + beta2, 0.0)
    else:
        res = rb(rng.standard_normal((V, C)))
        ops["res"] = Gb(res)
        d.res = ops["res"].ptr
        yref = np.maximum((z - mean) * rstd + beta + res, 0.0)
    out = {"y": Guarded((V, C), torch.bfloat16), "mask": Guarded((V, C // 8), torch.uint8)}
    d.y, d.mask_out = out["y"].ptr, out["mask"].ptr
    _lib.check(lib.ursn_bn_bf16_forward(ctypes.byref(d), stream()))
    check_all(dict(ops, **out), "bf16 bn forward")
    all_written(out["y"], "y")
    ys = out["y"].numpy().astype(np.float64)
    assert np.abs(ys - yref).max() <= BF_TOL * np.abs(yref).max()
    assert np.array_equal(out["mask"].tensor.cpu().numpy(), _mask_bytes(ys))
    g = dy * (ys > 0)
    xh = (z - mean) * rstd
    want = {"batch": {"dz": rstd * (g - g.mean(0) - xh * (g * xh).mean(0))}, "frozen": {"dz": rstd * g}}
    if two:
        xh2 = (z2 - mean2) * rstd2
        want["batch"]["dz2"], want["frozen"]["dz2"] = rstd2 * (g - g.mean(0) - xh2 * (g * xh2).mean(0)), rstd2 * g
    else:
        want["batch"]["dres"] = want["frozen"]["dres"] = g
    nb = lib.ursn_bn_bf16_scratch_bytes(V, C)
    for name, fn in (("batch", lib.ursn_bn_bf16_backward), ("frozen", lib.ursn_bn_bf16_backward_frozen)):
        runs = []
        for fill in (0x00, 0xFF):
            o = {"dz": Guarded((V, C), torch.bfloat16), "dbeta": Guarded((C,), torch.float32, np.zeros(C)),
                 "scratch": Guarded((nb,), torch.uint8).fill(fill)}
            b = _lib.ursn_bn_bf16_desc()
            b.voxels, b.channels, b.relu = V, C, 1
            b.z, b.mean, b.rstd, b.beta = d.z, d.mean, d.rstd, d.beta
            b.dy, b.mask, b.dz, b.dbeta = ops["dy"].ptr, out["mask"].ptr, o["dz"].ptr, o["dbeta"].ptr
            if two:
                o["dz2"], o["dbeta2"] = Guarded((V, C), torch.bfloat16), Guarded((C,), torch.float32, np.zeros(C))
                b.z2, b.mean2, b.rstd2, b.dz2, b.dbeta2 = d.z2, d.mean2, d.rstd2, o["dz2"].ptr, o["dbeta2"].ptr
            else:
                o["dres"] = Guarded((V, C), torch.bfloat16)
                b.dres, b.dres_accumulate = o["dres"].ptr, 0
            _lib.check(fn(ctypes.byref(b), _P(o["scratch"]), nb, stream()))
            check_all(dict(ops, **out, **o), "bf16 bn backward (%s)" % name)
            keys = [k for k in sorted(o) if k != "scratch"]
            for k in keys:
                all_written(o[k], k)
            runs.append({k: o[k].numpy() for k in keys})
        for k in runs[0]:
            assert same_bits(runs[0][k], runs[1][k]), (name, k, "depends on what the scratch held")
        for k, ref in want[name].items():
            assert np.abs(runs[0][k] - ref).max() <= BF_TOL * np.abs(ref).max(), (name, k)
        for k in ("dbeta", "dbeta2") if two else ("dbeta",):
            assert np.abs(runs[0][k] - g.sum(0)).max() <= 1e-5 * np.abs(g).sum(0).max(), (name, k)


def _head_scratch_bytes(lib, n, pix, ncls):
    """ursn_softmax_ce has no size query: a call with 0 bytes is refused with "(have < need)" before anything runs."""
    one = Guarded((ncls,), torch.float32, np.zeros(ncls))
    out = (ctypes.c_float * 3)()
    assert lib.ursn_softmax_ce(_P(one), None, None, None, n, pix, ncls, None, None, out, _P(one), 0, stream()) != 0
    msg = lib.ursn_last_error().decode()
    assert "scratch too small" in msg, msg
    return int(msg.rsplit("<", 1)[1].strip(" )"))


HEAD_CASES = [(3, True), (5, False)]
PIX_HEAD_BLOCKS = 1777      # 3 x 1777 voxels: six blocks of 1024, the last ragged (500: two)


@pytest.mark.parametrize("ncls,use_w", HEAD_CASES)
def test_softmax_ce_head_outputs_guarded(ncls, use_w, pix=500):
    lib = _lib.load()
    rng = np.random.default_rng(ncls)
    n = 3
    logits = _f32(rng.standard_normal((n, pix, ncls)) * 3)
    logits[0, :7] = 1.25
    data = _f32(rng.uniform(0, 1, (n, pix)) * (rng.uniform(0, 1, (n, pix)) > 0.6))
    label = rng.integers(0, ncls, (n, pix)).astype(np.float64)
    w = _f32(rng.uniform(0.1, 2, (n, pix))) if use_w else None
    m = O.loss_and_metrics(logits, data, label, w)
    G = lambda a: Guarded(a.shape, torch.float32, values=a)   # noqa: E731
    ops = {"logits": G(logits), "data": G(data), "label": G(label)}
    if use_w:
        ops["weight"] = G(w)
    nb = _head_scratch_bytes(lib, n, pix, ncls)
    runs = []
    for fill in (0x00, 0xFF):
        out = {"softmax": Guarded((n, pix, ncls), torch.float32), "dlogits": Guarded((n, pix, ncls), torch.float32),
               "scratch": Guarded((nb,), torch.uint8).fill(fill)}
        o3 = (ctypes.c_float * 3)()
        _lib.check(lib.ursn_softmax_ce(_P(ops["logits"]), _P(ops["data"]), _P(ops["label"]), _P(ops["weight"]) if use_w else None, n, pix, ncls,
                                       _P(out["softmax"]), _P(out["dlogits"]), o3, _P(out["scratch"]), nb, stream()))
        check_all(dict(ops, **out), "softmax_ce")
        all_written(out["softmax"], "softmax"), all_written(out["dlogits"], "dlogits")
        runs.append((out["softmax"].numpy(), out["dlogits"].numpy(), np.array(list(o3), np.float32)))
    for a, b in zip(*runs):
        assert same_bits(a, b), "depends on what the scratch held"
    sm, dl, o3 = runs[0]
    assert abs(o3[0] - m["loss"]) / abs(m["loss"]) < 1e-5 and abs(o3[1] - m["acc_all"]) < 1e-6 and abs(o3[2] - m["acc_nonzero"]) < 1e-6
    assert rel_err(sm, m["softmax"]) < 1e-5 and rel_err(dl, m["dlogits"]) < 1e-5


@pytest.mark.parametrize("ncls,use_w", HEAD_CASES)
def test_softmax_ce_head_outputs_guarded_on_several_blocks(ncls, use_w):
    test_softmax_ce_head_outputs_guarded(ncls, use_w, pix=PIX_HEAD_BLOCKS)


def test_adam_buffers_guarded():
    lib, n = _lib.load(), 10007
    rng = np.random.default_rng(0)
    p = {"a": _f32(rng.standard_normal(n))}
    opt = O.Adam(p, lr=1e-3)
    ops = {"p": Guarded((n,), torch.float32, p["a"]), "m": Guarded((n,), torch.float32, np.zeros(n)), "v": Guarded((n,), torch.float32, np.zeros(n))}
    for t in range(1, 4):
        g = _f32(rng.standard_normal(n) * 10.0 ** rng.integers(-6, 2, n))
        opt.apply(p, {"a": g})
        ops["g"] = Guarded((n,), torch.float32, g)
        _lib.check(lib.ursn_adam(_P(ops["p"]), _P(ops["g"]), _P(ops["m"]), _P(ops["v"]), n, 1e-3, 0.9, 0.999, 1e-8, t, stream()))
        check_all(ops, "adam step %d" % t)
    for k in ("p", "m", "v"):
        all_written(ops[k], k)
    assert rel_err(ops["p"].numpy(), p["a"]) < 1e-6
