"""Production work partitions at test-size shapes: one table of environment sets.

The launchers pick their work split (z segments, split-K groups, boxes per workgroup, grid caps) from workgroup counts tuned for 256
CUs, so the guarded rows of tests/test_op_guards_gpu.py sit on the "too few workgroups" side of every threshold and the bench
workloads on the other.  Each SET below moves, through the library's switches (two of them test inputs: URSN_CU_COUNT, the CU count
the slot-count splits divide by, and URSN_B0_MINWG), a group of those rows onto the branch a bench layer takes by default; tests/test_partitions_host.py proves on a CPU that the branch is taken (ursn_conv_partition, the scratch
queries) and tests/test_partitions_gpu.py runs the guarded checks there.  The switches are read once per process: one child process
per set.  Plain helper module (no conftest), importable without a GPU."""
import collections
import ctypes
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FWD, DGRAD, WGRAD = 0, 1, 2

# what a (row, pass) must show under the set; d: the default environment's report, g: the set's.  part = the four words of
# ursn_conv_partition (include/uresnet_hip.h says what they mean per family), stats / wgrad = the scratch-size queries.
REQUIRE = {
    # dconv: gsplit 1, SLAB off, the conv kernel's own statistics partials = workgroups * 128 doubles
    "dconv_gsplit1": lambda d, g, ps: g["part"][2] == 0 and g["part"][3] == 0 and (ps != FWD or g["stats"] == g["part"][0] * 128 * 8),
    # bdwgrad: one slice holds every box
    "bdwgrad_one_slice": lambda d, g, ps: g["part"][2] == 1 and g["part"][1] == g["part"][3] >= 4 and d["part"][1] == 1 and g["wgrad"] < d["wgrad"],
    # bdwgrad: several boxes per workgroup, several slices (the LDS double buffer flips inside a slice)
    "bdwgrad_walk": lambda d, g, ps: g["part"][1] >= 2 and g["part"][2] >= 2 and d["part"][1] == 1,
    "bdwgrad_walk_ragged": lambda d, g, ps: g["part"][1] >= 2 and g["part"][2] >= 2 and d["part"][1] == 1 and g["part"][3] % g["part"][1] != 0,
    # b3conv: one segment of all Z >= 36 planes (default: segments of at most 16)
    "b3_whole_z": lambda d, g, ps: g["part"][3] == 1 and g["part"][1] == g["Z"] >= 36 and d["part"][1] <= 16 and d["part"][3] > 1 and
    (ps != FWD or g["stats"] == g["part"][2] * 32 * 8),
    # b3conv: two segments of more than 16 planes each (what the default split gives at 256^3: long segments, several per column)
    "b3_long_segments": lambda d, g, ps: g["part"][3] == 2 and g["part"][1] > 16 and d["part"][1] <= 16,
    # b3wgrad: one column of all Z planes per tile (default: columns of at most 8 planes), one slab each
    "b3w_one_column": lambda d, g, ps: g["part"][1] == g["Z"] and d["part"][1] <= 8 and g["part"][0] < d["part"][0] and g["wgrad"] < d["wgrad"],
    # b3wgrad: the fold stage runs (default: too few slabs) ...
    "fold": lambda d, g, ps: d["part"][3] == 0 and g["part"][3] >= 2 and g["part"][0] >= 4 * g["part"][3] and g["part"][2] < g["part"][0],
    # ... and its last group is short
    "fold_ragged": lambda d, g, ps: d["part"][3] == 0 and g["part"][3] >= 2 and g["part"][0] >= 4 * g["part"][3] and g["part"][0] % g["part"][3] != 0,
    # box kernels: a larger box, fewer workgroups
    "larger_box": lambda d, g, ps: g["part"][3] > d["part"][3] and g["part"][0] < d["part"][0],
    # bcbconv: whole-Z columns
    "bcb_whole_z": lambda d, g, ps: g["part"][3] == 1 and d["part"][3] > 1 and g["part"][1] > d["part"][1],
    # bdconv: the 256-voxel box of form <2,8>, no split-K
    "bd_box256": lambda d, g, ps: g["part"][3] == 256 and d["part"][3] == 128 and g["part"][2] == 0,
    # bdconv: form <4,8> (four chunks per round: `rounds` = chunks / 4), 128-voxel box, no split-K
    "bd_form1": lambda d, g, ps: g["part"][3] == 128 and g["part"][2] == 0 and g["part"][1] * 4 == g["chunks"],
    # bsconv: the 4 x 4 x 8 coarse box of form <mt,8> (default at small volumes: 4 x 4 x 4)
    "bs_box128": lambda d, g, ps: g["part"][3] == 128 and d["part"][3] == 64 and g["part"][0] < d["part"][0],
    # pconv: the cap holds, the first workgroup takes >= 3 steps of 256 voxels, the last step is short
    "pconv_capped": lambda d, g, ps: g["part"][0] == 2 < d["part"][0] and g["part"][1] >= 3 and 0 < g["part"][3] < 256 and
    (ps != FWD or g["stats"] < d["stats"]),
    # tconv / twgrad / tdeconv / vwgrad (resident slots = occupancy x URSN_CU_COUNT): one segment of all the planes the kernel
    # marches (Zm: the low-resolution Z for tdeconv), where the default split has two or more
    "slots_whole_z": lambda d, g, ps: nz(g) == 1 and g["part"][1] == g["Zm"] and nz(d) >= 2 and d["part"][1] < g["Zm"] and
    g["part"][0] < d["part"][0] and (ps != FWD or (g["part"][2] == g["part"][0] and g["stats"] < d["stats"])) and
    (ps != WGRAD or g["wgrad"] <= d["wgrad"]),
    # ... two or more segments, each longer than the default's, the last one short
    "long_ragged": lambda d, g, ps: nz(g) >= 2 and g["part"][1] > d["part"][1] and g["Zm"] % g["part"][1] != 0 and
    (nz(g) - 1) * g["part"][1] < g["Zm"],
    # ... whose length is odd
    "long_ragged_odd_last": lambda d, g, ps: REQUIRE["long_ragged"](d, g, ps) and (g["Zm"] % g["part"][1]) % 2 == 1,
    # twgradz: ursn_pick_zseg picked an odd segment and make_wplan rounded it up to a plane pair (bit 32 of word 3), which the
    # default split of the row may do too -- at another length; the last segment is short and odd
    "long_ragged_pair_up": lambda d, g, ps: REQUIRE["long_ragged_odd_last"](d, g, ps) and g["part"][3] >> 32 == 1 and g["part"][1] % 2 == 0 and
    g["part"][2] == 2 * g["part"][0],
    # twgradz: an even picked segment, no round-up
    "long_ragged_no_pair_up": lambda d, g, ps: REQUIRE["long_ragged"](d, g, ps) and g["part"][3] >> 32 == 0,
    # bconv / bwgrad: a persistent workgroup walks two or more boxes of the default's size (default: one box per workgroup, so its
    # word 2 is the box count) ...
    "box_walk": lambda d, g, ps: g["part"][1] >= 2 and d["part"][1] == 1 and g["part"][3] == d["part"][3] and g["part"][0] < d["part"][0] and
    g["part"][1] * (g["part"][2] - 1) < d["part"][2] <= g["part"][1] * g["part"][2],
    # ... and the last workgroup's walk is short
    "box_walk_ragged": lambda d, g, ps: REQUIRE["box_walk"](d, g, ps) and d["part"][2] % g["part"][1] != 0,
    # ... and the contraction has several chunks (weights re-staged per chunk inside the walk)
    "box_walk_chunks": lambda d, g, ps: REQUIRE["box_walk"](d, g, ps) and g["chunks"] >= 2,
    # b0conv / b0wgrad: one segment of all Z planes (default: 16 or fewer)
    "b0_whole_z": lambda d, g, ps: nz(g) == 1 and g["part"][1] == g["Z"] >= 40 and d["part"][1] <= 16 and nz(d) > 1 and g["part"][0] < d["part"][0] and
    (ps != FWD or d["stats"] >= g["stats"] >= g["part"][2] * 32 * 8) and (ps != WGRAD or g["wgrad"] <= d["wgrad"]),      # (the query is the larger of this and the 8 -> 8 kernel's)
    # b0conv / b0wgrad: two segments of 20 planes or more ...
    "b0_long_segments": lambda d, g, ps: nz(g) == 2 and g["part"][1] >= 20 and d["part"][1] <= 16,
    # ... the second one short
    "b0_long_ragged": lambda d, g, ps: REQUIRE["b0_long_segments"](d, g, ps) and g["Z"] % g["part"][1] != 0,
}


def nz(r):
    """z segments of a report (word 3 without the twgrad round-up bit)"""
    return r["part"][3] & 0xFFFFFFFF


_LONG = ("tconv3d_long", "tconv3d_long_split")
_LONG_DG = ("tconv3d_long_pw", "tconv3d_long_bs2", "tconv3d_long_vdz")

# the kernel the last launch of a forward / weight-gradient check must have noted under the requirement
KERNEL = {"dconv_gsplit1": b"dconv", "bd_box256": b"bdconv_bf16<2,8>", "bd_form1": b"bdconv_bf16<4,8>",
          "long_ragged_pair_up": b"twgradz<8,8>", "long_ragged_no_pair_up": b"twgradz<8,8>"}

Set = collections.namedtuple("Set", "name env rows extras bench")
SETS = [
    Set("dconv_gsplit1", {"URSN_DCONV_MINWG": "1"},
        [(t, ps, "dconv_gsplit1") for t, pss in (("dconv3d_odd", (FWD,)), ("dconv3d_rag", (FWD,)), ("dconv3d_n2", (FWD, DGRAD)),
                                               ("dconv3d_dg_odd", (FWD, DGRAD)), ("dconv2d_odd", (FWD,))) for ps in pss], (),
        "cfg3 (192^3 x 4, fp32) level 3, 24^3 x 4 with 64 -> 64 channels: tiles * cout blocks >= 160 at gsplit 1"),
    Set("bdwgrad_one_slice", {"URSN_BDWGRAD_WGS": "1"},
        [(t, WGRAD, "bdwgrad_one_slice") for t in ("bdconv_rag_dp", "bdconv_odd_dp", "bdconv_n4_dp")], (),
        "no bench layer has ONE slice; the walk over every box of the tensor by one workgroup is cfg5 level 3's (four boxes) at its longest"),
    Set("bdwgrad_walk", {"URSN_BDWGRAD_WGS": "5"},
        [("bdconv_rag_dp", WGRAD, "bdwgrad_walk"), ("bdconv_odd_dp", WGRAD, "bdwgrad_walk"), ("bdconv_n4_dp", WGRAD, "bdwgrad_walk_ragged")], (),
        "cfg5 (256^3 x 4, bf16) level 3, 32^3 x 4 with 64 -> 64 channels: 512 boxes over 128 slices, four boxes per workgroup; level 4: two"),
    Set("b3_whole_z", {"URSN_B3_NZSEG": "1"},
        [("b3conv_16_16_zseg", FWD, "b3_whole_z"), ("b3conv_16_16_zseg", DGRAD, "b3_whole_z"), ("b3conv_pw_split_zseg", DGRAD, "b3_whole_z"),
         ("b3conv_norm_zseg", FWD, "b3_whole_z")], (),
        "cfg5 level 0 marches 64 planes per segment (8 -> 8, 16 -> 8) and level 1 none above 16; a single segment needs 2,048 tiles, "
        "which no bench layer has: the set stands for the long march (the plane ring wraps 12 times here, twice by default)"),
    Set("b3_long_segments", {"URSN_B3_NZSEG": "2"},
        [("b3conv_16_16_zseg", FWD, "b3_long_segments"), ("b3conv_16_16_zseg", DGRAD, "b3_long_segments"),
         ("b3conv_pw_split_zseg", DGRAD, "b3_long_segments"), ("b3conv_norm_zseg", FWD, "b3_long_segments")], (),
        "cfg5 level 0: four segments of 64 planes per column (8 and 16 -> 8 channels): segments longer than 16 planes with a seam between them"),
    Set("b3w_one_column", {"URSN_B3W_MINWG": "1"},
        [(t, WGRAD, "b3w_one_column") for t in ("b3conv_odd", "b3conv_16_8_odd", "b3conv_16_16_zseg", "b3conv_norm_odd",
                                               "b3conv_norm_relu_odd", "b3conv_norm_zseg")], (),
        "cfg5 level 0 (8 -> 8 plane-pair form, 16 -> 8): 1,024 tiles, one 256-plane column each"),
    Set("slab_fold3", {"URSN_SLAB_FOLD": "3"},
        [("b3conv_odd", WGRAD, "fold"), ("b3conv_16_8_odd", WGRAD, "fold"), ("b3conv_norm_odd", WGRAD, "fold"),
         ("b3conv_norm_relu_odd", WGRAD, "fold"), ("b3conv_16_16_zseg", WGRAD, "fold_ragged")], (),
        "cfg5 levels 0 and 1: 1,024 slabs folded in groups of 16 (evenly: a short last group needs a slab count that is no multiple of 16, "
        "which the bench volumes do not give and other volumes do)"),
    Set("slab_fold5", {"URSN_SLAB_FOLD": "5"},
        [("b3conv_odd", WGRAD, "fold_ragged"), ("b3conv_16_8_odd", WGRAD, "fold_ragged"), ("b3conv_norm_odd", WGRAD, "fold_ragged"),
         ("b3conv_norm_relu_odd", WGRAD, "fold_ragged"), ("b3conv_16_16_zseg", WGRAD, "fold")], (),
        "as slab_fold3, with the short last group on the plane-pair (8 -> 8) and the 16 -> 8 forms"),
    Set("larger_boxes", {"URSN_BCONV_MINWG": "1", "URSN_BWGRAD_MINWG": "1", "URSN_BCB_MINWG": "1", "URSN_BDCONV_MINWG": "1"},
        [(t, WGRAD, "larger_box") for t in ("bconv_k3s2_odd", "bsconv_k3s2_n2_sc", "bsconv_k3s2_lowodd", "bsconv_deconv_n2_sc",
                                           "bsconv_deconv_odd", "bsconv_deconv_rag_sc", "bpw_odd", "bconv_k1s2_n2", "bcbconv_odd_cb",
                                           "bcbconv_16_24_cb", "bconv_24_40", "b3conv_8_16", "bconv2d_n2", "bconv2d_s2_n2", "bconv2d_deconv")] +
        [("bcbconv_odd_cb", FWD, "bcb_whole_z"), ("bcbconv_odd_cb", DGRAD, "bcb_whole_z"), ("bcbconv_16_24_cb", FWD, "bcb_whole_z"),
         ("bcbconv_pw_odd", DGRAD, "bcb_whole_z")] +
        [(t, ps, "bd_box256") for t in ("bdconv_rag_dp", "bdconv_odd_dp", "bdconv_n4_dp") for ps in (FWD, DGRAD)], (),
        "cfg5: bwgrad of the stride-2 / transposed / 32-channel layers of levels 0-3 (>= 256 boxes x chunks: the first, largest box); "
        "bcbconv at level 1 (128^3 x 4: 256 columns, whole-Z); bdconv at level 3 (32^3 x 4: 512 boxes of 256 voxels, form <2,8>, gsplit 1)"),
    Set("bdconv_form1", {"URSN_BDCONV_FORM": "1,1"},
        [(t, FWD, "bd_form1") for t in ("bdconv_rag_dp", "bdconv_odd_dp")], (),      # (their data gradients contract 64 channels: two chunks, no form <4,8>)
        "cfg5 level 4 (16^3 x 4, 128 -> 128): form <2,8> gives 128 workgroups < 192, form <4,8> on 128-voxel boxes 256: taken at gsplit 1"),
    Set("bsconv_box128", {"URSN_BSCONV_NT": "8"},
        [("bsconv_k3s2_n2_sc", DGRAD, "bs_box128"), ("bsconv_k3s2_lowodd", DGRAD, "bs_box128"), ("bsconv_deconv_n2_sc", FWD, "bs_box128"),
         ("bsconv_deconv_odd", FWD, "bs_box128")], (),
        "cfg5: the transposed conv 32 -> 16 from level 2 to level 1 and the data gradient of the stride-2 conv 16 -> 32 (coarse grid 64^3 x 4: "
        "8,192 boxes of 128 voxels >= 512, so <mt,8> is taken; below that the 64-voxel box)"),
    Set("grid_caps", {"URSN_EW_GRID": "2", "URSN_BEW_GRID": "2", "URSN_BEW_AGRID": "2", "URSN_HEAD_GRID": "2", "URSN_PCONV_GRID": "2"},
        [("pconv3d_grid", FWD, "pconv_capped"), ("pconv3d_grid", DGRAD, "pconv_capped")], ("bn", "bn_bf16", "head", "loss_head", "adam"),
        "every level-0 / level-1 layer of cfg1-cfg5: the caps (512 / 1,024 / 4,096 blocks, 1,024 pconv workgroups) are saturated from "
        "2^19 voxels up, every block takes hundreds of trips and the partial buffers hold exactly `cap` rows"),
    Set("slots_whole_z", {"URSN_CU_COUNT": "1"},
        [(t, ps, "slots_whole_z") for t in _LONG + ("tconv3d_cblocks", "tconv2d_odd") for ps in (FWD, DGRAD, WGRAD)] +
        [("tconv3d_long_norm", FWD, "slots_whole_z"), ("tconv3d_long_norm", WGRAD, "slots_whole_z")] +
        [(t, DGRAD, "slots_whole_z") for t in _LONG_DG + ("tdeconv3d_dgrad_zseg", "tdeconv3d_pw_zseg")] +
        [("tdeconv3d_zseg", FWD, "slots_whole_z"), ("tdeconv2d_zseg", FWD, "slots_whole_z"), ("vwgrad3d_zseg", WGRAD, "slots_whole_z")], (),
        "cfg3 (192^3 x 4, fp32) levels 0 and 1: ursn_pick_zseg takes several rounds over 256 x occupancy slots and segments of tens of planes; "
        "one segment of the whole column is the longest march (the plane ring wraps 10 to 13 times at Z = 37 / 41, twice by default) and "
        "what a volume of many tiles and few planes gets"),
    Set("slots_long_ragged", {"URSN_CU_COUNT": "4"},
        [(t, ps, "long_ragged_odd_last") for t in _LONG for ps in (FWD, DGRAD)] + [(t, DGRAD, "long_ragged_odd_last") for t in _LONG_DG] +
        [(t, WGRAD, "long_ragged_pair_up") for t in _LONG] +
        [("tconv2d_odd", FWD, "long_ragged_odd_last"), ("tconv2d_odd", DGRAD, "long_ragged_odd_last"), ("tconv2d_odd", WGRAD, "long_ragged")], (),
        "cfg3 levels 0 and 1 (192 / 96 planes): several long segments per column with seams between them; 192 and 96 split evenly, "
        "other volumes leave a short last segment, and twgradz rounds an odd pick up to a plane pair (here 21 -> 22 + 19)"),
    Set("slots_long_ragged_16", {"URSN_CU_COUNT": "5"},
        [("tconv3d_long_norm", FWD, "long_ragged_odd_last"), ("tconv3d_long_norm", WGRAD, "long_ragged_odd_last"),
         ("tconv3d_long", WGRAD, "long_ragged_no_pair_up"), ("tconv3d_long_split", WGRAD, "long_ragged_no_pair_up"),
         ("tconv2d_odd", WGRAD, "long_ragged")], (),
        "as slots_long_ragged for the 16 -> 16 kernels (occupancy 2 and 1: another count gives them 14 + 14 + 13), and twgradz on an "
        "even pick (14), which the round-up leaves alone"),
    Set("box_walks", {"URSN_CU_COUNT": "2"},
        [("bsconv_k3s2_lowodd", FWD, "box_walk_ragged")] +
        [(t, FWD, "box_walk") for t in ("bsconv_k3s2_n2_sc", "bconv_k1s2_n2", "bconv_24_40", "bconv2d_n2", "bconv2d_s2_n2")] +
        [("bsconv_deconv_odd", DGRAD, "box_walk_ragged"), ("bsconv_deconv_rag_sc", DGRAD, "box_walk_chunks")] +
        [(t, DGRAD, "box_walk") for t in ("bsconv_deconv_n2_sc", "bcbconv_16_24_cb", "bconv2d_n2", "bconv2d_s2_n2")] +
        [(t, WGRAD, "box_walk_ragged") for t in ("bconv_k3s2_odd", "bpw_odd", "bcbconv_16_24_cb")] +
        [("bsconv_deconv_rag_sc", WGRAD, "box_walk_chunks")] +
        [(t, WGRAD, "box_walk") for t in ("bsconv_deconv_odd", "bconv2d_n2", "bconv2d_deconv", "bconv_24_40")], (),
        "every bconv / bwgrad layer of cfg5 (256^3 x 4, bf16): a persistent grid of 256 x occupancy workgroups, each walking several boxes "
        "and re-staging its LDS between them (two to hundreds); the last workgroup's walk is short whenever boxes % per != 0"),
    Set("b0_whole_z", {"URSN_B0_MINWG": "1"},
        [(t, ps, "b0_whole_z") for t in ("b0conv_zseg", "b0conv_zseg_odd") for ps in (FWD, WGRAD)], (),
        "cfg5 conv0 (256^3 x 4): 4,096 tiles >= 2,048, so every workgroup marches the whole 256-plane column"),
    Set("b0_long_segments", {"URSN_B0_MINWG": "5"},
        [("b0conv_zseg", FWD, "b0_long_segments"), ("b0conv_zseg", WGRAD, "b0_long_segments"),
         ("b0conv_zseg_odd", FWD, "b0_long_ragged"), ("b0conv_zseg_odd", WGRAD, "b0_long_ragged")], (),
        "conv0 of a volume with 1,024 to 2,047 tiles (128^3 x 4 has 1,024): two long segments per column with a seam between them; "
        "20 + 20 planes, and 21 + 20"),
]
# rows a set names that the default plan already puts on the set's branch (the requirement holds; nothing moves)
AT_DEFAULT = {("dconv_gsplit1", "dconv3d_rag", FWD): "192 contraction channels are 12 chunks: no split but gsplit 1 is legal, so this row "
                                                     "runs dconv<STATS, SLAB = false> in the default suite too"}
BY_NAME = {s.name: s for s in SETS}
assert len(BY_NAME) == len(SETS)

# Numeric / partition switches of DESIGN.md's table that no set drives, each with the reason.
NOT_DRIVEN = {
    "URSN_BCONV_MINWG": "set in larger_boxes, but moves no row: below the threshold bconv_plan falls back to the FIRST fitting candidate, which "
                        "is the largest box -- the box the bench layers take; the forward / data-gradient rows are already there by default",
    "URSN_B3_MINWG": "the z split of b3conv is driven through URSN_B3_NZSEG (b3_whole_z, b3_long_segments); the threshold itself is moot at test shapes",
    "URSN_BCONV_BOX": "replaces the first box candidate with one no bench layer is planned with",
    "URSN_BCONV_LDS_KB": "first-pass LDS budget: the default (158 KB) is what every bench layer gets; a lower value is an A/B state",
    "URSN_BWGRAD_LDS_KB": "as URSN_BCONV_LDS_KB (156 KB)",
    "URSN_BCONV_NBUF": "single-buffered staging is what bconv_plan gives the 32-channel chunks on the large boxes by default, at the bench and in "
                       "the rows bconv_k3s2_odd / bsconv_k3s2_* / bsconv_deconv_* here (family word ...1); forcing it on the narrower layers, "
                       "which fit two buffers everywhere, is an A/B state",
    "URSN_GCONV_BN": "4 restores wide column blocks where voxel tiles are few; the bench's gconv_mfma layers (cfg3's 6^3 level) are such layers "
                     "and take the default 2",
    "URSN_IGEMM_MINX": "narrowest row of the fp32 implicit GEMM: moves rows between families, not a partition",
    "URSN_IGEMM_LDS_KB": "occupancy cap (A/B state)",
    "URSN_IGEMM_ALLTAPS": "kernel form, not a partition",
    "URSN_S2_MINX": "moves the 6^3 level between families (in-situ row of tests/test_insitu_gpu.py territory), not a partition",
    "URSN_B3WGRAD_PAIR": "the non-pair 8 -> 8 weight gradient is no bench layer's default",
    "URSN_B3WGRADZ_LDSPAD": "LDS padding (occupancy A/B), not a partition",
    "URSN_BDWGRAD_MAXVOX": "family limit, not a partition", "URSN_DWGRAD_MAXVOX": "family limit, not a partition",
    "URSN_DCONV_MINK": "family limit, not a partition", "URSN_DCONV_MAXVOX": "family limit, not a partition",
    "URSN_DCONV_MAXVOX2D": "family limit, not a partition",
    "URSN_WGRAD_PRIO": "stream priority", "URSN_NORM_ON_LOAD": "fusion switch (tests/test_insitu_gpu.py SWITCHES)",
    "URSN_S2CONV_V2": "kernel form (tests/test_insitu_gpu.py SWITCHES)", "URSN_GRAPH": "hipGraph replay, not a partition",
}


def driven():
    return {k for s in SETS for k in s.env}


# ---- child side -------------------------------------------------------------------------------------------------------------------
def report(name):
    """{"tag/pass": {fam, part, stats, wgrad, chunks}} for the rows of set `name` (or of every set: name None), plus the scratch
    queries of the elementwise kernels.  Host logic only."""
    import test_op_guards_gpu as G
    from uresnet_amd import _lib
    lib = _lib.load()
    rows = sorted({(t, ps) for s in SETS if name in (None, s.name) for t, ps, _ in s.rows})
    out = {}
    for tag, ps in rows:
        row = G.BY_TAG[tag]
        assert row.fams[ps] is not None and (row.algo == 0 or row.fams[ps] in G.FORCED[row.algo]), (tag, ps)
        d = G.build_desc(row, ps)
        part = (ctypes.c_int64 * 4)()
        rc = lib.ursn_conv_partition(ctypes.byref(d), ps, part)
        K = row.co if ps == DGRAD else row.ci
        out["%s/%d" % (tag, ps)] = {
            # (a forced algo names its family itself: ursn_conv_plan does not see it, ursn_conv_partition follows the dispatcher)
            "fam": G.plan_name(row, ps, d) if row.algo == 0 else row.fams[ps], "want_fam": row.fams[ps], "part": list(part) if rc == 0 else None,
            "chunks": K // 32, "Z": row.S[0], "Zm": row.S[0] // 2 if row.stride == 2 and not row.tr and ps == DGRAD else row.S[0],
            "no_stats": bool(row.dtype == G.B and row.tr),
            "stats": int(lib.ursn_conv_stats_scratch_bytes(ctypes.byref(d))) if ps == FWD else None,
            "wgrad": int(lib.ursn_conv_wgrad_scratch_bytes(ctypes.byref(d))) if ps == WGRAD else None}
    V, big = G.V_BN_BLOCKS, 1 << 24
    out["bn"] = {str(C): [int(lib.ursn_bn_scratch_bytes(v, C)) for v in (V, big)] for C, _, _ in G.BN_CASES}
    Vb = 3 * 7 * 9 * 41
    out["bn_bf16"] = {str(C): [int(lib.ursn_bn_bf16_scratch_bytes(v, C)) for v in (Vb, big)] for C in (8, 16, 32)}
    out["loss_head"] = [int(lib.ursn_loss_head_scratch_bytes(3, v, 3)) for v in (4099, big)]
    return out


def run_child(code, env, timeout):
    """One child process with `env` on top of an environment cleared of every switch a set names."""
    base = {k: v for k, v in os.environ.items() if k not in driven()}
    pre = "import sys; sys.path.insert(0, %r); sys.path.insert(0, %r)\n" % (ROOT, os.path.join(ROOT, "tests"))
    return subprocess.run([sys.executable, "-c", pre + code], env=dict(base, **env), cwd=ROOT, stdout=subprocess.PIPE, stderr=subprocess.PIPE,
                          text=True, timeout=timeout)


def host_report(name, env):
    p = run_child("import json, _partitions as P\nprint('REPORT ' + json.dumps(P.report(%r)))" % name, env, 300)
    assert p.returncode == 0, (p.stdout[-1500:], p.stderr[-2500:])
    return json.loads([l for l in p.stdout.splitlines() if l.startswith("REPORT ")][-1][7:])


def check_rows(s, dflt, got):
    """The host half: every (row, pass) of set `s` stays with its family and shows the required change.  Returns the rows that moved."""
    moved = []
    for tag, ps, req in s.rows:
        k = "%s/%d" % (tag, ps)
        d, g = dflt[k], got[k]
        assert g["fam"] == g["want_fam"] == d["fam"], (s.name, k, "the switch pushed the row onto another kernel", g["fam"])
        assert d["part"] is not None and g["part"] is not None, (s.name, k, "partition not reported")
        assert REQUIRE[req](d, g, ps), (s.name, k, req, "default", d, "set", g)
        if ps == FWD and g["no_stats"]:      # bf16 transposed convs take their statistics at net level: the query says 0
            assert g["stats"] == 0, (s.name, k, g["stats"])
        elif ps == FWD:
            assert g["stats"] > 0 and g["stats"] % 8 == 0, (s.name, k, g["stats"])
        if ps == WGRAD:
            assert g["wgrad"] > 0 and g["wgrad"] % 8 == 0, (s.name, k, g["wgrad"])
        if g["part"] != d["part"]:
            moved.append((tag, ps))
    return moved


def check_caps(dflt, got):
    """grid_caps: the scratch queries of the BatchNorm and head kernels shrink to the cap and no longer grow with the voxel count."""
    for fam in ("bn", "bn_bf16"):
        for C, (small, big) in got[fam].items():
            assert small == big and small % 8 == 0 and 0 < small < dflt[fam][C][0] < dflt[fam][C][1], (fam, C, got[fam][C], dflt[fam][C])
    small, big = got["loss_head"]
    assert small == big and small % 8 == 0 and 0 < small < dflt["loss_head"][0] < dflt["loss_head"][1], (got["loss_head"], dflt["loss_head"])


def gpu_child(name):
    """The GPU half, inside the set's environment: the guarded checks of tests/test_op_guards_gpu.py (imported, not restated) on
    every row of the set -- borders intact, no NaN, scratch-fill independence (the same call twice: the same bits), oracle
    agreement at the imported tolerances, forward statistics accepted at exactly the stated scratch size and refused 8 bytes below."""
    import time
    import test_op_guards_gpu as G
    s = BY_NAME[name]
    for k, v in s.env.items():
        assert os.environ.get(k) == v, (k, os.environ.get(k))
    t0 = time.time()
    fn = {FWD: G.test_forward_with_statistics_at_the_exact_scratch_size, DGRAD: G.test_data_gradient_overwrite_and_accumulate,
          WGRAD: G.test_weight_gradient_at_the_exact_scratch_size}
    from uresnet_amd import _lib
    for tag, ps, req in s.rows:
        fn[ps](tag)
        if ps != DGRAD and req in KERNEL:      # (the data-gradient check ends on its accumulate call)
            assert _lib.load().ursn_last_kernel_name() == KERNEL[req], (tag, ps, _lib.load().ursn_last_kernel_name())
        print("ok %s pass %d" % (tag, ps))
    if "bn" in s.extras:
        for C, relu, res in G.BN_CASES:
            G.test_bn_forward_backward_and_frozen_backward(C, relu, res, V=G.V_BN_BLOCKS)
        print("ok bn")
    if "bn_bf16" in s.extras:
        for C in (8, 16, 32):
            for form in ("join_identity", "join_conv_shortcut"):
                G.test_bf16_bn_join_forward_backward_and_frozen_backward(C, form)
        print("ok bn_bf16")
    if "head" in s.extras:
        for ncls, use_w in G.HEAD_CASES:
            G.test_softmax_ce_head_outputs_guarded(ncls, use_w, pix=G.PIX_HEAD_BLOCKS)
        print("ok head")
    if "adam" in s.extras:
        G.test_adam_buffers_guarded()
        print("ok adam")
    if "loss_head" in s.extras:
        _loss_head_cases(int(s.env["URSN_HEAD_GRID"]))
        print("ok loss_head")
    print("PARTITION_OK %s %.1f s" % (name, time.time() - t0))


def _loss_head_cases(cap):
    """tests/_loss_cases.py against the fp64 oracle of losses.py at the bounds of tests/test_loss_head_gpu.py (its own checker), under
    a block cap: 3 x 4,099 voxels are 13 blocks of 1,024 by default, `cap` blocks of 25 ragged trips here."""
    import numpy as np
    import test_loss_head_gpu as L
    from _abi import same_bits
    from _loss_cases import SPECS, make_case
    from uresnet_amd import _lib
    lib = _lib.load()
    L._head_blocks = lambda P: max(1, min(cap, (P + 1023) // 1024))      # the caller states the head's block count: the capped one
    n, vox, ncls = 3, 4099, 3
    assert L._head_blocks(n * vox) == cap
    for sid in ("neutral", "focal2_smooth", "dice"):
        spec = dict(SPECS)[sid]
        for with_bn in (False, True):
            z, data, label, weight = make_case(7 * vox + n + ncls, n, vox, ncls, ties=not with_bn)
            for li, layout in enumerate(L._layouts(ncls)):
                c = L.OpCase(z, data, label, weight, layout, with_bn, True, seed=li)
                what = "%s %s bn %s under a cap of %d blocks" % (sid, layout, with_bn, cap)
                out8, raw, bs = c.run(lib, spec, fill=0xFF)
                L._check_against_oracle(c, spec, out8, c.dlogits_of(raw), bs, what)
                out8b, rawb, bsb = c.run(lib, spec, fill=0x00)
                assert same_bits(out8, out8b) and np.array_equal(raw, rawb), what + ": a second call gave other bits"
                assert bs is None or np.array_equal(bs.view(np.uint64), bsb.view(np.uint64)), what
