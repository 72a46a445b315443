"""mm_rotate (include/mm_wait.h) on a real MI355X: the drivers of tests/test_rotate.py on the product's library, against the
oracle, plus the product geometry — a 1v1 chain long enough for the pair path, a 5v5 chain long enough for the team path
beside one short enough for k_walk, each ticked right after a rotation.  Each scenario runs in a process of its own
(tests/rotate_gpu_worker.py) under its own time limit."""
import os
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu
WORKER = os.path.join(os.path.dirname(os.path.abspath(__file__)), "rotate_gpu_worker.py")

# seconds: hang guards of the order tests/test_gpu_move.py uses, not measurements (every scenario takes seconds)
LIMITS = {"named_cases": 120, "slots_and_full_pool": 120, "errors": 120, "host_route": 120, "script_seed1": 240,
          "script_seed2_restart": 240, "pair_geometry": 120, "team_geometry": 120}


# After a scenario that hung (time limit) or died of a signal (abort, segmentation fault: what a GPU fault looks like from
# here) nothing more is started on the card from this module: the remaining scenarios fail at once and say why.
STOPPED = []


@pytest.mark.parametrize("case", sorted(LIMITS))
def test_gpu_rotate(case):
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
