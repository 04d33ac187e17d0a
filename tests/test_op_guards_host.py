"""Host side of tests/test_op_guards_gpu.py: the statistics-scratch query and the table of guarded rows, checked without a device
(ursn_conv_plan, ursn_conv_stats_scratch_bytes, ursn_conv_wgrad_scratch_bytes and ursn_conv_bs_blocks are host logic only)."""
import ctypes

import pytest

import test_op_guards_gpu as G
from uresnet_amd import _lib


@pytest.mark.parametrize("row", G.ROWS, ids=[r.tag for r in G.ROWS])
def test_every_row_reaches_the_family_it_names_and_has_a_stated_scratch_size(row):
    lib = _lib.load()
    assert any(f is not None for f in row.fams)
    for ps in range(3):
        if row.fams[ps] is None:
            continue
        d = G.build_desc(row, ps)
        G.check_family(row, ps, d)      # algo 0: ursn_conv_plan names it; forced algo: the algo stands for it
        if ps == 0:
            need = lib.ursn_conv_stats_scratch_bytes(ctypes.byref(d))
            if row.dtype == G.B and row.tr:
                assert need == 0      # refused by the call: statistics of bf16 transposed convs are taken at net level
            else:
                assert need > 0 and need % 8 == 0, (row.tag, need)   # > 0 also proves a forced algo takes the shape
        if ps == 1 and row.ex.get("bs"):
            assert lib.ursn_conv_bs_blocks(ctypes.byref(d)) > 0
        if ps == 2:
            assert lib.ursn_conv_wgrad_scratch_bytes(ctypes.byref(d)) > 0


@pytest.mark.parametrize("dtype", [G.F, G.B], ids=["fp32", "bf16"])
@pytest.mark.parametrize("ps", [0, 1, 2], ids=["forward", "dgrad", "wgrad"])
def test_the_table_covers_every_family_of_the_plan(dtype, ps):
    have = {r.fams[ps] for r in G.ROWS if r.dtype == dtype and r.fams[ps] is not None}
    assert G.FAMILIES[(dtype, ps)] <= have, G.FAMILIES[(dtype, ps)] - have
    # ... and, except the naive reference (algo 1, which the plan never names), each through ursn_conv_plan itself (an algo 0 row)
    planned = {r.fams[ps] for r in G.ROWS if r.dtype == dtype and r.fams[ps] is not None and r.algo == 0}
    assert G.FAMILIES[(dtype, ps)] - {"naive"} <= planned, G.FAMILIES[(dtype, ps)] - planned
    # per family: a row with N = 2 (an image seam inside the payload)
    for fam in G.FAMILIES[(dtype, ps)]:
        rows = [r for r in G.ROWS if r.dtype == dtype and r.fams[ps] == fam]
        assert any(r.N >= 2 for r in rows), (fam, "no row with an image seam")
        assert any(G.odd_grid(r, ps) for r in rows), (fam, "no row with every extent odd")


def test_the_query_is_zero_where_the_call_refuses():
    lib = _lib.load()
    assert lib.ursn_conv_stats_scratch_bytes(None) == 0
    for row, change in ((G.BY_TAG["tconv3d_n2"], dict(k=2)), (G.BY_TAG["tconv3d_n2"], dict(algo=5)), (G.BY_TAG["tconv3d_n2"], dict(algo=7)),
                        (G.BY_TAG["pconv3d"], dict(algo=4)), (G.BY_TAG["b3conv_odd"], dict(transposed=1, stride=2))):
        d = G.build_desc(row, 0)
        for k, v in change.items():
            setattr(d, k, v)
        assert lib.ursn_conv_stats_scratch_bytes(ctypes.byref(d)) == 0, (row.tag, change)
    d = G.build_desc(G.BY_TAG["igemm3d_odd"], 0)      # normalise-on-load has no implicit-GEMM kernel
    d.in_mean = d.in_rstd = d.in_beta = G.DUMMY
    assert lib.ursn_conv_stats_scratch_bytes(ctypes.byref(d)) == 0
    d = G.build_desc(G.BY_TAG["pconv3d"], 0)          # the pointwise kernel's partials do not depend on the voxel count ...
    a = lib.ursn_conv_stats_scratch_bytes(ctypes.byref(d))
    d.in_sp[0] *= 4
    assert lib.ursn_conv_stats_scratch_bytes(ctypes.byref(d)) == a
    # ... and exceed ursn_bn_scratch_bytes(out voxels, cout), the size the header used to state
    assert a > lib.ursn_bn_scratch_bytes(2 * 8 * 12 * 16, 8)
