"""One GPU scenario group of tests/test_gpu_move_if.py, in a process of its own:  python tests/move_if_gpu_worker.py <case>
(the test starts it under a time limit, so a scenario that hangs ends there and takes no other one with it).
Exit status 0: the scenarios held.  The drivers are those of the CPU tier (tests/move_if_scenarios.py); the engine is the
product's, the witness numpy over the oracle."""
import os
import sys
import time

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, HERE)

from microservice_matchmaking_amd import Engine                          # noqa: E402
from oracle.oracle import OracleEngine, build                            # noqa: E402
from locate_scenarios import chain_lengths                               # noqa: E402
from move_if_scenarios import (candidate_count, chain_length, errors, full_on_the_selected, into_company, limits,   # noqa: E402
                               move_if_script, out_plus_stamped, plain_calls, pool_at_entry, seats, sharded, wrapped_ring)
from partners_scenarios import query_counts                              # noqa: E402


def chains():
    for n in chain_lengths():
        for tick in (True, False):
            chain_length(Engine, OracleEngine, n, tick)


def counts():
    for k1 in query_counts():
        for spread in (False, True):
            candidate_count(Engine, OracleEngine, k1, spread)


def rules():
    limits(Engine, OracleEngine)
    pool_at_entry(Engine, OracleEngine)
    seats(Engine, OracleEngine)
    into_company(Engine, OracleEngine)


def slots():
    full_on_the_selected(Engine, OracleEngine)
    wrapped_ring(Engine, OracleEngine)
    plain_calls(Engine)
    out_plus_stamped(Engine, OracleEngine)
    errors(Engine)
    sharded(Engine)


def script():
    for seed in (1, 2):
        move_if_script(Engine, OracleEngine, seed=seed)


CASES = {"chain_lengths": chains, "candidate_counts": counts, "rules_and_seats": rules, "slots_and_calls": slots, "script": script}

if __name__ == "__main__":
    import torch
    assert torch.cuda.is_available(), "GPU tests need a GPU; there is no CPU fallback"
    build()
    t0 = time.perf_counter()
    CASES[sys.argv[1]]()
    print("%s ok in %.1f s" % (sys.argv[1], time.perf_counter() - t0))
