"""GPU half of the production-partition sets (tests/_partitions.py): one child process per set, in the set's
environment, runs the guarded checks of tests/test_op_guards_gpu.py (imported there, not restated) on the set's rows -- every operand
between NaN borders, scratch at exactly the stated size, forward statistics refused 8 bytes below it, no NaN out, the same bits from
the same call whatever the scratch held, and the fp64 oracle at the tolerances of the parity files (TOL, WG_TOL, BF_TOL, BF_WG_TOL,
the 1e-5 head bounds).  A forced partition changes the summation order: nothing is compared bitwise with the default partition.
The children run one after the other; the timeout is a hang guard only (the in-situ file's 900 s), nothing is rerun."""
import time

import pytest

import _partitions as P

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("name", [s.name for s in P.SETS])
def test_guarded_rows_at_the_production_partition(name):
    s = P.BY_NAME[name]
    t0 = time.time()
    p = P.run_child("import _partitions as P\nP.gpu_child(%r)" % name, s.env, 900)
    wall = time.time() - t0
    print("%s: child wall time %.1f s; %s" % (name, wall, [l for l in p.stdout.splitlines() if l.startswith("PARTITION_OK")]))
    assert p.returncode == 0 and "PARTITION_OK %s" % name in p.stdout, (name, p.returncode, p.stdout[-1500:], p.stderr[-2500:])
    done = [l for l in p.stdout.splitlines() if l.startswith("ok ")]
    assert len(done) == len(s.rows) + len(s.extras), (name, done)
