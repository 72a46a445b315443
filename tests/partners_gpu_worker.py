"""One GPU scenario of tests/test_gpu_partners.py, in a process of its own:  python tests/partners_gpu_worker.py <case>
(the test starts it under a time limit, so a scenario that hangs ends there and takes no other one with it).
Exit status 0: the scenario held.  The drivers are those of the CPU tier (tests/partners_scenarios.py); the engine is the
product's, the witness numpy over the oracle."""
import os
import sys
import time

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, HERE)

from microservice_matchmaking_amd import Engine                          # noqa: E402
from oracle.oracle import OracleEngine, build                            # noqa: E402
from partners_scenarios import (chain_length, chain_lengths, errors, exact_distances, filters, group_override, marks,   # noqa: E402
                                marks_move_rotate, none_duplicates_capacity, null_outputs, partners_script, query_count,
                                query_counts, roles, seats, self_exclusion, several_groups, sharded,
                                stored_anchor_has_no_partner)


def chains():
    for n in chain_lengths():
        for tick in (True, False):
            chain_length(Engine, OracleEngine, n, tick)


def counts():
    for nq in query_counts():
        for spread in (False, True):
            query_count(Engine, OracleEngine, nq, spread)


def predicate():
    exact_distances(Engine, OracleEngine)
    filters(Engine, OracleEngine)
    self_exclusion(Engine, OracleEngine)
    for marker in ("cancel", "expire"):
        marks(Engine, OracleEngine, marker)
    marks_move_rotate(Engine, OracleEngine)


def places():
    seats(Engine, OracleEngine)
    roles(Engine, OracleEngine)
    several_groups(Engine, OracleEngine)
    group_override(Engine, OracleEngine)
    none_duplicates_capacity(Engine, OracleEngine)
    null_outputs(Engine, OracleEngine)
    errors(Engine)
    sharded(Engine)


def script():
    stored_anchor_has_no_partner(Engine, OracleEngine)
    partners_script(Engine, OracleEngine)


CASES = {"chain_lengths": chains, "query_counts": counts, "predicate_and_marks": predicate, "places_and_calls": places,
         "script": script}

if __name__ == "__main__":
    import torch
    assert torch.cuda.is_available(), "GPU tests need a GPU; there is no CPU fallback"
    build()
    t0 = time.perf_counter()
    CASES[sys.argv[1]]()
    print("%s ok in %.1f s" % (sys.argv[1], time.perf_counter() - t0))
