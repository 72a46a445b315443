"""mm_partner_stats (include/mm_wait.h) on a real MI355X: the drivers of tests/test_partner_stats.py on the product's library,
against numpy over the oracle and against the product's own mm_partners over the same slots — table lengths on both sides of
the sort's tile and of the walk's boundaries, every radix pass, the ends of int32, segments of group, region and party, own and
other modes, marks and seats, errors, ShardedSearch, the random script — grouped into five scenarios.  Each runs in a process
of its own (tests/partner_stats_gpu_worker.py) under its own time limit."""
import os
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu
WORKER = os.path.join(os.path.dirname(os.path.abspath(__file__)), "partner_stats_gpu_worker.py")

# seconds: hang guards, a generous multiple of what the oracle's side of a scenario takes (every scenario takes seconds)
LIMITS = {"tile_boundaries": 120, "passes_bias_and_clamp": 120, "segments_and_modes": 120, "who_waits_and_calls": 120, "script": 120}


# After a scenario that hung (time limit) or died of a signal (abort, segmentation fault: what a GPU fault looks like from
# here) nothing more is started on the card from this module: the remaining scenarios fail at once and say why.
STOPPED = []


@pytest.mark.parametrize("case", sorted(LIMITS))
def test_gpu_partner_stats(case):
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
