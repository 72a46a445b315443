"""The sorted route of mm_partners and the rule calls (include/mm_wait.h, mm_tuning.wait_sort_mtests) on a real MI355X: the
drivers of tests/test_partners_sorted.py on the product's library — the existing partners and rule-call drivers on an engine
class forced onto the route, table lengths on both sides of the LDS sample and of the sort's tile, the per-query self term,
the role-keyed table, an empty table, the size rule at its boundary, the two routes on one random script — grouped into seven
scenarios.  Each runs in a process of its own (tests/partners_sorted_gpu_worker.py) under its own time limit."""
import os
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu
WORKER = os.path.join(os.path.dirname(os.path.abspath(__file__)), "partners_sorted_gpu_worker.py")

# seconds: hang guards, a generous multiple of what the oracle's side of a scenario takes (every scenario takes seconds)
LIMITS = {"partners_lengths": 120, "partners_rest": 120, "move_if_lengths": 120, "move_if_rest": 120, "table_and_sample": 120,
          "new_shapes": 120, "routes_agree": 120}


# After a scenario that hung (time limit) or died of a signal (abort, segmentation fault: what a GPU fault looks like from
# here) nothing more is started on the card from this module: the remaining scenarios fail at once and say why.
STOPPED = []


@pytest.mark.parametrize("case", sorted(LIMITS))
def test_gpu_partners_sorted(case):
    assert not STOPPED, "not started: %s" % STOPPED[0]
    try:
        p = subprocess.run([sys.executable, WORKER, case], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True,
                           timeout=LIMITS[case])
    except subprocess.TimeoutExpired as ex:
        STOPPED.append("%s did not end within %d s" % (case, LIMITS[case]))
        raise AssertionError("%s; output so far: %s" % (STOPPED[0], (ex.stdout or "")[-4000:]))
    print(p.stdout)
    if p.returncode < 0 or p.returncode in (124, 134, 137, 139):
        STOPPED.append("%s ended with status %d" % (case, p.returncode))
    assert p.returncode == 0, p.stdout[-4000:]
    assert "%s ok" % case in p.stdout
