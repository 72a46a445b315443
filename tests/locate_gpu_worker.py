"""One GPU scenario of tests/test_gpu_locate.py, in a process of its own:  python tests/locate_gpu_worker.py <case>
(the test starts it under a time limit, so a scenario that hangs ends there and takes no other one with it).
Exit status 0: the scenario held.  The drivers are those of the CPU tier (tests/locate_scenarios.py); the engine is the
product's, the witness the oracle."""
import os
import sys
import time

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, HERE)

from microservice_matchmaking_amd import Engine                          # noqa: E402
from oracle.oracle import OracleEngine, build                            # noqa: E402
from locate_scenarios import (chain_length, chain_lengths, clock_off, clock_on, duplicates, errors, lobby_seats, marks,   # noqa: E402
                              marks_rotate, no_scratch_leak, none_cases, null_outputs, several_groups, sharded)


def chains():
    for n in chain_lengths():
        for tick in (True, False):
            chain_length(Engine, OracleEngine, n, tick)


def marked():
    for marker in ("cancel", "expire"):
        marks(Engine, OracleEngine, marker)
    marks_rotate(Engine, OracleEngine)


def places():
    lobby_seats(Engine, OracleEngine)
    several_groups(Engine, OracleEngine)
    none_cases(Engine, OracleEngine)
    duplicates(Engine, OracleEngine)
    no_scratch_leak(Engine, OracleEngine)


def calls():
    clock_off(Engine, OracleEngine)
    clock_on(Engine, OracleEngine)
    null_outputs(Engine, OracleEngine)
    errors(Engine)
    sharded(Engine)


CASES = {"chain_lengths": chains, "marks": marked, "lobbies_groups_none_duplicates": places, "clock_null_errors_sharded": calls}

if __name__ == "__main__":
    import torch
    assert torch.cuda.is_available(), "GPU tests need a GPU; there is no CPU fallback"
    build()
    t0 = time.perf_counter()
    CASES[sys.argv[1]]()
    print("%s ok in %.1f s" % (sys.argv[1], time.perf_counter() - t0))
