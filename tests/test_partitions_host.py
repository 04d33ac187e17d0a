"""Host half of the production-partition sets (tests/_partitions.py): on a CPU, in a child process per set (the
switches are read once per process), every (row, pass) of the set still reaches the family tests/test_op_guards_gpu.ROWS names,
ursn_conv_partition reports the required change against the default environment, and the scratch-size queries stay consistent.
ursn_conv_partition reads the plan function the family's launcher calls (b3_plan, w3_plan, dc_plan, dw_plan, the box pickers, make_plan /
make_wplan / make_dplan / vw_plan of the fp32 tiled families, c0_plan)."""
import functools
import os
import re

import pytest

import _partitions as P
import test_op_guards_gpu as G


@functools.lru_cache(maxsize=None)
def default_report():
    return P.host_report(None, {})


@pytest.mark.parametrize("name", [s.name for s in P.SETS])
def test_the_set_moves_its_rows_onto_the_production_branch(name):
    s = P.BY_NAME[name]
    dflt, got = default_report(), P.host_report(name, s.env)
    moved = P.check_rows(s, dflt, got)
    for tag, ps, _ in s.rows:
        if (name, tag, ps) in P.AT_DEFAULT:
            assert (tag, ps) not in moved, (name, tag, ps, "no longer at the default: drop it from AT_DEFAULT")
        else:
            assert (tag, ps) in moved, (name, tag, ps, "the set leaves the row on its default partition")
    for ps in {ps for _, ps, _ in s.rows}:
        assert any(p == ps for _, p in moved), (name, ps, "no row of this pass moves")
    if s.extras:
        P.check_caps(dflt, got)
    print(name, "moved", moved)


def test_the_default_environment_reports_the_small_shape_partitions():
    """The premise: at the default thresholds the rows sit on the other side -- split-K slabs, one box per workgroup, short z
    segments, no fold stage -- and the elementwise scratch grows with the voxel count."""
    d = default_report()
    assert d["dconv3d_n2/0"]["part"][3] == 1 and d["dconv3d_n2/0"]["part"][2] > 1
    assert d["bdconv_rag_dp/2"]["part"][1] == 1
    assert d["b3conv_16_16_zseg/0"]["part"][1] <= 16 and d["b3conv_16_16_zseg/0"]["part"][3] > 1
    assert d["b3conv_odd/2"]["part"][3] == 0
    assert d["pconv3d_grid/0"]["part"][0] == 4
    assert d["tconv3d_long/0"]["part"][1:] == [9, 40, 5] and d["tconv3d_long/2"]["part"][1] == 10 and d["tconv3d_long/2"]["part"][3] == (1 << 32) + 5
    assert d["tdeconv3d_zseg/0"]["part"][1:] == [7, 8, 2] and d["tdeconv3d_pw_zseg/1"]["part"][1:] == [8, 0, 2] and d["vwgrad3d_zseg/2"]["part"][1:] == [10, 8, 2]
    assert d["tconv2d_odd/0"]["part"][1:] == [8, 10, 5]
    assert all(d[k]["part"][1] == 1 for k in ("bsconv_k3s2_lowodd/0", "bsconv_deconv_odd/1", "bconv_k3s2_odd/2", "bsconv_deconv_rag_sc/1"))
    assert d["b0conv_zseg/0"]["part"] == [12, 10, 12, 4] and d["b0conv_zseg_odd/2"]["part"] == [16, 11, 16, 4]
    for fam in ("bn", "bn_bf16"):
        for C, (small, big) in d[fam].items():
            assert 0 < small < big, (fam, C)


def test_every_row_of_every_set_is_a_guarded_row_and_each_family_has_a_named_case():
    need = {"dconv_gsplit1", "bdwgrad_one_slice", "bdwgrad_walk", "bdwgrad_walk_ragged", "b3_whole_z", "b3w_one_column", "fold_ragged",
            "larger_box", "bcb_whole_z", "bd_box256", "pconv_capped", "slots_whole_z", "long_ragged", "long_ragged_odd_last",
            "long_ragged_pair_up", "long_ragged_no_pair_up", "box_walk", "box_walk_ragged", "box_walk_chunks", "b0_whole_z",
            "b0_long_segments", "b0_long_ragged"}
    have = set()
    for s in P.SETS:
        assert s.rows and s.bench
        for tag, ps, req in s.rows:
            assert tag in G.BY_TAG and G.BY_TAG[tag].fams[ps] is not None and req in P.REQUIRE, (s.name, tag, ps, req)
            have.add(req)
    assert need <= have, need - have
    # b3conv's whole-Z segment: every fused form the family has at op level (normalise-on-load, fused shortcut term, split, accumulate)
    ex = [G.BY_TAG[t].ex for t, ps, _ in P.BY_NAME["b3_whole_z"].rows]
    assert any(e.get("norm") for e in ex) and any(e.get("pw") and e.get("split") for e in ex) and any(1 in e.get("acc", (0, 1)) for e in ex)
    # the slot-count sets: whole-Z on every family that takes ursn_pick_zseg, a Z >= 37 row where the family has one, the channel-
    # blocked tconv and every fused form tconv has at op level; ragged long segments on tconv (3-D and 2-D) and both twgradz outcomes
    rows = P.BY_NAME["slots_whole_z"].rows
    fams = {(G.BY_TAG[t].fams[ps], ps) for t, ps, _ in rows}
    assert {("tconv", 0), ("tconv", 1), ("twgrad", 2), ("tdeconv", 0), ("tdeconv", 1), ("tdeconv+pw", 1), ("vwgrad", 2)} <= fams, fams
    for fam in ("tconv", "twgrad"):
        assert any(G.BY_TAG[t].S[0] >= 37 and G.BY_TAG[t].ndim == nd for t, ps, _ in rows if G.BY_TAG[t].fams[ps] == fam for nd in (2,)), fam
        assert any(G.BY_TAG[t].S[0] >= 37 and G.BY_TAG[t].ndim == 3 for t, ps, _ in rows if G.BY_TAG[t].fams[ps] == fam), fam
    assert any(t == "tconv3d_cblocks" for t, _, _ in rows) and any(G.BY_TAG[t].ndim == 2 and G.BY_TAG[t].tr for t, _, _ in rows)
    for name in ("slots_whole_z", "slots_long_ragged"):
        ex = [G.BY_TAG[t].ex for t, ps, _ in P.BY_NAME[name].rows]
        assert all(any(e.get(k) for e in ex) for k in ("split", "pw", "bs", "vdz")), name
    assert any(G.BY_TAG[t].ex.get("norm") for t, _, _ in P.BY_NAME["slots_whole_z"].rows + P.BY_NAME["slots_long_ragged_16"].rows)
    assert any(G.BY_TAG[t].ex.get("split") and req == "long_ragged_pair_up" for t, _, req in P.BY_NAME["slots_long_ragged"].rows)
    # the box walks: all three passes, each with a short last walk; a stride-2, a transposed, a 2-D and the 128 -> 64 row
    bw = P.BY_NAME["box_walks"].rows
    for ps in (0, 1, 2):
        assert any(p == ps and req == "box_walk_ragged" for _, p, req in bw), ps
        assert all(G.BY_TAG[t].fams[p] == ("bwgrad" if p == 2 else "bconv") for t, p, _ in bw)
    tags = [G.BY_TAG[t] for t, _, _ in bw]
    assert any(r.stride == 2 and not r.tr for r in tags) and any(r.tr for r in tags) and any(r.ndim == 2 for r in tags)
    assert any(G.BY_TAG[t].ci == 128 and G.BY_TAG[t].co == 64 and req == "box_walk_chunks" for t, _, req in bw)


def test_every_numeric_switch_is_driven_or_listed_with_a_reason():
    """Every number-valued or structured switch of DESIGN.md's A/B table is either in a set's environment or in NOT_DRIVEN with the
    reason (extends tests/test_host.py::test_switch_table_matches_sources, which holds the table to the sources)."""
    with open(os.path.join(P.ROOT, "DESIGN.md")) as f:
        design = f.read()
    section = design.split("### A/B switches", 1)[1].split("\n## ", 1)[0]
    rows = "\n".join(l for l in section.splitlines() if l.startswith("|"))
    numeric = set(re.findall(r'(URSN_[A-Z0-9_]+)=(?:n\b|p\b|"|\d+\|)', rows))
    assert {"URSN_DCONV_MINWG", "URSN_BDWGRAD_WGS", "URSN_B3_NZSEG", "URSN_SLAB_FOLD", "URSN_EW_GRID", "URSN_BDCONV_FORM",
            "URSN_BSCONV_NT", "URSN_PCONV_GRID", "URSN_CU_COUNT", "URSN_B0_MINWG"} <= numeric, sorted(numeric)
    numeric |= {"URSN_BCONV_NBUF", "URSN_B3WGRAD_PAIR"}      # on / off in the table, partition-like in effect
    drv = P.driven()
    assert {"URSN_CU_COUNT", "URSN_B0_MINWG"} <= drv, "the two test inputs are there to be driven by a set"
    missing = sorted(n for n in numeric if n not in drv and n not in P.NOT_DRIVEN)
    assert not missing, "neither in a set nor in NOT_DRIVEN: %s" % missing
    stale = sorted(n for n in P.NOT_DRIVEN if n not in numeric)
    assert not stale, "in NOT_DRIVEN but no numeric switch of the table: %s" % stale
    both = sorted(n for n in P.NOT_DRIVEN if n in drv and n != "URSN_BCONV_MINWG")
    assert not both, both
    for n, why in P.NOT_DRIVEN.items():
        assert len(why) > 10, n


def test_families_without_a_plan_struct_are_not_reported():
    import ctypes
    from uresnet_amd import _lib
    lib = _lib.load()
    out = (ctypes.c_int64 * 4)()
    for tag, ps in (("igemm3d_odd", 0), ("igemm3d_odd", 2), ("bpw_odd", 0), ("bs2k8_n2", 0), ("bs2k8_n2", 1), ("bs2k8_n2", 2), ("gconv3d_odd", 0)):
        d = G.build_desc(G.BY_TAG[tag], ps)
        assert lib.ursn_conv_partition(ctypes.byref(d), ps, out) != 0 and b"not reported" in lib.ursn_last_error(), tag
    # reported: the families that split by ursn_pick_zseg and conv0 of the bf16 plan (one z segment each at these shapes) ...
    for tag, ps, want in (("tconv3d_n2", 0, [8, 9, 8, 1]), ("tconv3d_n2", 2, [12, 9, 24, 1]), ("b0conv_odd", 0, [6, 9, 6, 1]), ("b0conv_odd", 2, [6, 9, 6, 1]),
                          ("tdeconv3d_odd", 0, [4, 9, 4, 1]), ("tdeconv3d_pw", 1, [8, 9, 0, 1]), ("vwgrad3d_odd", 2, [8, 9, 8, 1])):
        d = G.build_desc(G.BY_TAG[tag], ps)
        assert lib.ursn_conv_partition(ctypes.byref(d), ps, out) == 0 and list(out) == want, (tag, ps, list(out))
    # ... and a forced tiled family (algo 3), which ursn_conv_plan does not see: the query follows the dispatcher
    d = G.build_desc(G.BY_TAG["tconv3d_cblocks"], 0)
    assert lib.ursn_conv_partition(ctypes.byref(d), 0, out) == 0 and list(out) == [72, 8, 72, 3], list(out)
    assert lib.ursn_conv_partition(None, 0, out) != 0


@pytest.mark.parametrize("src,query,launcher,plan", [
    ("conv_deep.hip", "deep_conv_partition", "launch_deep_conv", "dc_plan("),
    ("bf16_wgraddeep.hip", "bdwgrad_partition", "launch_bdwgrad", "dw_plan("),
    ("bf16_conv3.hip", "b3conv_partition", "launch_b3conv", "b3_plan("),
    ("bf16_wgrad3.hip", "b3wgrad_partition", "launch_b3wgrad", "w3_plan("),
    ("bf16_wgrad3.hip", "b3wgrad_partition", "slab_fold", "slab_fold_group("),
    ("bf16_convcb.hip", "bcbconv_partition", "launch_bcbconv", "cb_plan("),
    ("bf16_convdeep.hip", "bdconv_partition", "launch_bdconv", "bd_plan("),
    ("bf16_conv.hip", "bconv_partition", "launch_bconv", "bconv_plan("),
    ("bf16_conv.hip", "bwgrad_partition", "launch_bwgrad", "bwgrad_plan("),
    ("bf16_scatter.hip", "bsconv_partition", "launch_bsconv", "bs_plan("),
    ("conv_pointwise.hip", "pointwise_conv_partition", "launch_pointwise_conv", "pconv_grid("),
    ("conv_tiled.hip", "tiled_conv_partition", "launch_tiled_conv", "make_plan("),
    ("conv_tiled.hip", "tiled_conv_partition", "launch_tiled_conv_bn", "make_plan("),
    ("conv_tiled.hip", "tiled_wgrad_partition", "launch_tiled_wgrad", "make_wplan("),
    ("deconv_tiled.hip", "tiled_deconv_partition", "launch_tiled_deconv", "make_dplan("),
    ("wgrad_valu.hip", "valu_wgrad_partition", "launch_valu_wgrad", "vw_plan("),
    ("bf16_conv0.hip", "b0conv_partition", "launch_b0conv", "c0_plan("),
    ("bf16_conv0.hip", "b0wgrad_partition", "launch_b0wgrad", "c0_plan("),
])
def test_the_query_and_the_launcher_call_the_same_plan_function(src, query, launcher, plan):
    """Source text only: the body of the family's partition query and the body of its launcher both call the one plan function."""
    with open(os.path.join(P.ROOT, "u-resnet_amd", "csrc", src)) as f:
        text = f.read()

    def body(name):
        m = re.search(r"^(?:static )?(?:int|bool) %s\([^;{]*\{" % re.escape(name), text, re.M)
        assert m, (src, name)
        return text[m.end():text.index("\n}\n", m.end())]

    assert plan in body(query) and plan in body(launcher), (src, query, launcher, plan)
