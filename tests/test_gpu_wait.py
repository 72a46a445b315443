"""The engine clock (include/mm_wait.h) on a real MI355X: the scripts of tests/test_wait.py at product geometry, and
expiry, wait statistics and matched waits on the 1M pools of BASELINE cfg-2 and cfg-3, every tick against the oracle
with the same cancels.  Each scenario runs in a process of its own (tests/wait_gpu_worker.py) under its own time limit."""
import os
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu
WORKER = os.path.join(os.path.dirname(os.path.abspath(__file__)), "wait_gpu_worker.py")

# seconds: a generous multiple of what the oracle (the slow side) needs for the scenario
LIMITS = {"script_seed1": 240, "script_seed2": 240, "script_generic_walk": 300, "script_restart": 420,
          "cfg2_1m": 420, "cfg3_1m": 420}


# After a scenario that hung (time limit) or died of a signal (abort, segmentation fault: what a GPU fault looks like from
# here) nothing more is started on the card from this module: the remaining scenarios fail at once and say why.
STOPPED = []


@pytest.mark.parametrize("case", sorted(LIMITS))
def test_gpu_wait(case):
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
