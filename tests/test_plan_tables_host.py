"""The host queries against a snapshot of what they answered before the topology table (csrc/topology.h) was extracted from the
two plans: tools/plan_snapshot.py recomputes, for a matrix of configurations and under ten switch sets (one child process each:
the plans read their switches at create), the return code and error text of ursn_query, its sizes (workspace_bytes among them),
the ursn_query_layer rows, the ursn_query_concat pairs and ursn_bn_moving_size.  tests/golden/plan_tables.json holds one SHA-256
per group of those records, written by the same tool on the commit named in its "parent" field; every field must be equal.
After a mismatch, `python tools/plan_snapshot.py --dump FILE --set NAME` on both builds shows the records that differ.

Nothing here touches a device."""
import ctypes
import importlib.util
import json
import os

import pytest

from uresnet_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_spec = importlib.util.spec_from_file_location("plan_snapshot", os.path.join(ROOT, "tools", "plan_snapshot.py"))
snap = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(snap)

with open(os.path.join(ROOT, "tests", "golden", "plan_tables.json")) as _f:
    GOLDEN = json.load(_f)


@pytest.fixture(scope="module")
def current():
    return snap.run_sets()


def test_snapshot_covers_every_switch_set():
    assert sorted(GOLDEN["sets"]) == sorted(snap.SWITCH_SETS)
    assert len(GOLDEN["parent"]) == 40


@pytest.mark.parametrize("name", sorted(snap.SWITCH_SETS))
def test_plan_tables_equal_the_parents(current, name):
    want, got = GOLDEN["sets"][name], current[name]
    assert sorted(got) == sorted(want)
    for group in sorted(want):
        assert got[group] == want[group], (name, group)


def _matrix_bf16():
    for group, case in snap.cases():
        if case[5] == "bf16" and case[6] == 2 and case[7] == 1:   # layer facts depend on neither max_batch nor trainable
            yield case


def test_bf16_rows_are_the_fp32_rows_of_the_same_shape():
    lib = _lib.load()
    n_ok = 0
    for case in _matrix_bf16():
        rec = snap.record(_lib, lib, case)
        if rec["rc"] != 0:
            continue
        twin = snap.record(_lib, lib, case[:5] + ("fp32",) + case[6:])
        assert twin["rc"] == 0, case
        assert rec["layers"] == twin["layers"], case
        assert rec["concat"] == twin["concat"], case
        n_ok += 1
    assert n_ok > 0


def test_bf16_refusals_reach_query_layer():
    lib = _lib.load()
    info = _lib.ursn_layer_info()
    sizes = _lib.ursn_sizes()
    n_refused = 0
    for case in _matrix_bf16():
        cfg = snap.make_config(_lib, case)
        if lib.ursn_query(ctypes.byref(cfg), ctypes.byref(sizes)) == 0:
            continue
        why = lib.ursn_last_error()
        assert lib.ursn_query_layer(ctypes.byref(cfg), 0, ctypes.byref(info)) != 0, case
        assert lib.ursn_last_error() == why, case
        n_refused += 1
    assert n_refused > 0
