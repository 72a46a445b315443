"""The engine clock (include/mm_wait.h) on a real MI355X: the scripts of tests/test_wait.py at product geometry, its
targeted cases at their own sizes (the selection's chunk and wave edges, every histogram bucket and bucket 32, the 64-bit
age sum carrying at each step of its reduction, mm_expire's strict threshold up to 2^32 - 1, mm_matches_wait per path),
and expiry, wait statistics and matched waits on the 1M pools of BASELINE cfg-2 and cfg-3, every tick against the oracle
with the same cancels.  Each scenario runs in a process of its own (tests/wait_gpu_worker.py) under its own time limit."""
import os
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu
WORKER = os.path.join(os.path.dirname(os.path.abspath(__file__)), "wait_gpu_worker.py")

# seconds: a generous multiple of what the oracle (the slow side) needs for the scenario
LIMITS = {"script_seed1": 240, "script_seed2": 240, "script_generic_walk": 300, "script_restart": 420, "script_tiled": 240,
          "cfg2_1m": 420, "cfg3_1m": 420}
# The targeted cases of tests/test_wait.py at its sizes (pools of 900 to 6000, chains of WT_CHUNK +- 1).  Measured once on an
# MI355X, the whole process (interpreter and imports included) / the drivers alone, in seconds:
#   calls 2.1 / 0.2   expiry_cases 2.3 / 0.2   clock_wrap_and_ring_laps 2.1 / 0.2   histogram_and_old_ages 2.0 / 0.2
#   sum_carries_and_thresholds 2.5 / 0.3   selection_edges 2.2 / 0.3   matches_wait_paths 2.1 / 0.1
# The limit is ten times that and never under 60 s: the oracle's share grows with the machine's load, and a limit that is
# too tight reads as a hang and stops the module.
LIMITS.update({"calls": 60, "expiry_cases": 60, "clock_wrap_and_ring_laps": 60, "histogram_and_old_ages": 60,
               "sum_carries_and_thresholds": 60, "selection_edges": 60, "matches_wait_paths": 60})


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
