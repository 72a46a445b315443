"""mm_expire_if, mm_move_if and mm_move_out_if (include/mm_wait.h) on a real MI355X: the drivers of tests/test_move_if.py on
the product's library, against numpy over the oracle — chains of every length at which the walk's geometry changes, candidate
counts around the tile of queries, partner counts and distances exactly at the limits, the pool at entry, seats, a move only
where someone fits, MM_ERR_FULL judged on the selected, a wrapped ring, the equivalences with the plain calls, errors,
ShardedSearch and the random script — grouped into five scenarios.  Each runs in a process of its own
(tests/move_if_gpu_worker.py) under its own time limit."""
import os
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu
WORKER = os.path.join(os.path.dirname(os.path.abspath(__file__)), "move_if_gpu_worker.py")

# seconds: hang guards, a generous multiple of what the oracle's side of a scenario takes (every scenario takes seconds)
LIMITS = {"chain_lengths": 120, "candidate_counts": 120, "rules_and_seats": 120, "slots_and_calls": 120, "script": 120}


# After a scenario that hung (time limit) or died of a signal (abort, segmentation fault: what a GPU fault looks like from
# here) nothing more is started on the card from this module: the remaining scenarios fail at once and say why.
STOPPED = []


@pytest.mark.parametrize("case", sorted(LIMITS))
def test_gpu_move_if(case):
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
