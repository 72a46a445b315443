"""mm_move (include/mm_wait.h) on a real MI355X: the drivers of tests/test_move.py at product geometry, against the oracle.
The pools are the smallest that cross every chunk, wave and ring boundary the kernels have; each scenario runs in a process
of its own (tests/move_gpu_worker.py) under its own time limit."""
import os
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu
WORKER = os.path.join(os.path.dirname(os.path.abspath(__file__)), "move_gpu_worker.py")

# seconds: hang guards of the order tests/test_gpu_wait.py uses, not measurements (every scenario takes seconds)
LIMITS = {"script_seed1": 240, "script_seed2_restart": 240, "selected_count_edges": 240, "tier_chain": 120,
          "roles_cleared": 120, "roles_refused": 120, "roles_refused_wrapped": 120, "full_pool": 120}


# After a scenario that hung (time limit) or died of a signal (abort, segmentation fault: what a GPU fault looks like from
# here) nothing more is started on the card from this module: the remaining scenarios fail at once and say why.
STOPPED = []


@pytest.mark.parametrize("case", sorted(LIMITS))
def test_gpu_move(case):
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
