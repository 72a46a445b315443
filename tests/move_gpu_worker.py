"""One GPU scenario of tests/test_gpu_move.py, in a process of its own:  python tests/move_gpu_worker.py <case>
(the test starts it under a time limit, so a scenario that hangs ends there and takes no other one with it).
Exit status 0: the scenario held.  The drivers are those of the CPU tier (tests/move_scenarios.py); the engine is the
product's, the witness the oracle."""
import os
import sys
import time

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, HERE)

from microservice_matchmaking_amd import Engine                          # noqa: E402
from oracle.oracle import OracleEngine, build                            # noqa: E402
from move_scenarios import (bucket_lengths, full_case, log_counts, move_script, role_cases,   # noqa: E402
                            selected_count_edges, tier_chain)


def script(seed, restart_at=()):
    """The randomised script at product geometry: capacity 8192, about 1 500 and then up to 400 players a round, eight
    rounds.  What it must have covered to count: players moved and lobbies in the strict and in the fallback mode."""
    log = move_script(Engine, OracleEngine, seed=seed, restart_at=restart_at)
    moved, lobbies = log_counts(log)
    print("moved %d players, lobbies per mode %s" % (moved, lobbies))
    assert moved > 100 and lobbies[2] > 5 and lobbies[3] > 5, (moved, lobbies)
    return log


def script_restart(seed):
    assert script(seed) == script(seed, restart_at=(2, 5))


def edges():
    """BK_PER_WAVE - 1 / BK_PER_WAVE / + 1 and BK_CHUNK - 1 / BK_CHUNK / + 1 selected players out of three rating groups of
    2 * WT_CHUNK + 1, lengths from the source; the first count also with every stored lobby's seat among the selected."""
    w, c = bucket_lengths()
    done = selected_count_edges(Engine, OracleEngine, [w - 1, w, w + 1, c - 1, c, c + 1], capacity=16384)
    print("selected counts (count, source ticked first, selected): %s" % done)
    assert len(done) == 7


CASES = {
    "script_seed1": lambda: script(1),
    "script_seed2_restart": lambda: script_restart(2),
    "selected_count_edges": edges,
    "tier_chain": lambda: print("tiers: %d -> %d" % tier_chain(Engine, OracleEngine)),
    "roles_cleared": lambda: role_cases(Engine, OracleEngine, clear=True),
    "roles_refused": lambda: print("refused %d" % role_cases(Engine, OracleEngine, clear=False)),
    "roles_refused_wrapped": lambda: print("refused %d" % role_cases(Engine, OracleEngine, clear=False, wrap=True)),
    "full_pool": lambda: full_case(Engine, OracleEngine),
}

if __name__ == "__main__":
    import torch
    assert torch.cuda.is_available(), "GPU tests need a GPU; there is no CPU fallback"
    build()
    t0 = time.perf_counter()
    CASES[sys.argv[1]]()
    print("%s ok in %.1f s" % (sys.argv[1], time.perf_counter() - t0))
