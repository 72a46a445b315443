"""mm_move_out, mm_moved_rows and mm_enqueue_stamped (include/mm_wait.h) on a real MI355X: the drivers of
tests/test_carry.py at product geometry, against mm_move on a second engine and the oracle.  The pools are the smallest that
cross every chunk, wave and ring boundary the kernels have (capacity 8192, 16 384 for the twins with a restart, 2048 for the
full pool); each scenario runs in a process of its own (tests/carry_gpu_worker.py) under its own time limit, and never more
than two processes hold the GPU."""
import os
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu
WORKER = os.path.join(os.path.dirname(os.path.abspath(__file__)), "carry_gpu_worker.py")

# seconds: hang guards of the order tests/test_gpu_move.py uses, not measurements (every scenario takes seconds)
LIMITS = {"twins_seed1": 240, "twins_seed2_restart": 240, "stamped_edges_slot_list": 240, "ring_wrap": 120, "rows": 240,
          "roles_refused": 120, "full_pool": 120, "two_ranks": 240}


# After a scenario that hung (time limit) or died of a signal (abort, segmentation fault: what a GPU fault looks like from
# here) nothing more is started on the card from this module: the remaining scenarios fail at once and say why.
STOPPED = []


# two_ranks last: its GPU work runs in rank processes the worker starts, and whatever ends one of them badly comes back as
# one of the statuses below, after which nothing else would be started anyway
ORDER = sorted(c for c in LIMITS if c != "two_ranks") + ["two_ranks"]


@pytest.mark.parametrize("case", ORDER)
def test_gpu_carry(case):
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
