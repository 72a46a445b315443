"""Moves, rotations and stamped enqueues in front of the long-chain walks on a real MI355X: the drivers of
tests/test_long_chain.py on the product's library at the product's geometry, against numpy over the oracle — a move into a 1v1
chain of PL_MAX - 1, PL_MAX and 3 x PK_T + 1 players (mm_move and mm_move_out + mm_enqueue_stamped, a range of new slots and a
wrapped list), a rotation in front of a tiled pair tick under kp_rounds and kp_round, a move of more than BK_CHUNK players into
a 5v5 chain of several chunks under the four team tunings, refused roles at that count, the low-rate regime of a standing
chain with a rotation and a move every period, run_stream over a team-path chain against the owner route, and the random script
of every wait call at long-chain sizes (two seeds, one with a restart, and one under force_generic).  Each case asserts from
mm_path_stats that the tick ran on the path it was built for and prints the counters.  Each runs in a process of its own
(tests/long_chain_gpu_worker.py) under its own time limit."""
import os
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu
WORKER = os.path.join(os.path.dirname(os.path.abspath(__file__)), "long_chain_gpu_worker.py")

# seconds: hang guards, not targets (every case takes seconds)
LIMITS = {"pair_moved_in_below": 120, "pair_moved_in_at": 120, "pair_moved_in_tiles": 120, "pair_rotated": 120,
          "team_moved_in": 120, "team_refused": 120, "team_stream_regime": 120, "stream_long": 120,
          "long_script_seed2": 120, "long_script_seed6_restart": 120, "long_script_generic_walk": 120}


# After a case that hung (time limit) or died of a signal (abort, segmentation fault: what a GPU fault looks like from
# here) nothing more is started on the card from this module: the remaining cases fail at once and say why.
STOPPED = []


@pytest.mark.parametrize("case", sorted(LIMITS))
def test_gpu_long_chain(case):
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


def test_gpu_wait_stress_with_fuzzed_knobs():
    """Ten seconds of tests/stress.py --wait --fuzz-knobs in a child process: long_script with drawn seeds, rounds and restarts
    under random combinations of mm_tuning fields; at least one scenario must have completed."""
    assert not STOPPED, "not started: %s" % STOPPED[0]
    stress = os.path.join(os.path.dirname(WORKER), "stress.py")
    try:
        p = subprocess.run([sys.executable, stress, "10", "9", "--wait", "--fuzz-knobs"], stdout=subprocess.PIPE,
                           stderr=subprocess.STDOUT, text=True, timeout=120)
    except subprocess.TimeoutExpired as ex:
        STOPPED.append("stress.py --wait did not end within 120 s")
        raise AssertionError("%s; output so far: %s" % (STOPPED[0], (ex.stdout or "")[-4000:]))
    print(p.stdout)
    if p.returncode < 0 or p.returncode in (124, 134, 137, 139):
        STOPPED.append("stress.py --wait ended with status %d" % p.returncode)
    assert p.returncode == 0, p.stdout[-4000:]
    done = [ln for ln in p.stdout.splitlines() if ln.startswith("gpu_stress --wait --fuzz-knobs:")]
    assert done and int(done[0].split(":")[1].split()[0]) >= 1, p.stdout[-2000:]
