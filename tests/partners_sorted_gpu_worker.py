"""One GPU scenario of tests/test_gpu_partners_sorted.py, in a process of its own:  python tests/partners_sorted_gpu_worker.py <case>
(the test starts it under a time limit, so a scenario that hangs ends there and takes no other one with it).
Exit status 0: the scenario held.  The drivers are those of the CPU tier (tests/partners_sorted_scenarios.py and, on an engine
class forced onto the sorted route, tests/partners_scenarios.py and tests/move_if_scenarios.py); the engine is the product's,
the witnesses numpy over the oracle and the product's own tiles route."""
import os
import sys
import time

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, HERE)

import move_if_scenarios as mv                                           # noqa: E402
import partners_scenarios as ps                                          # noqa: E402
from locate_scenarios import chain_lengths                               # noqa: E402
from microservice_matchmaking_amd import Engine                          # noqa: E402
from oracle.oracle import OracleEngine, build                            # noqa: E402
from partners_sorted_scenarios import (empty_table, marked_twin, role_byte, route_choice, routes_agree, sorted_cls,   # noqa: E402
                                       table_and_sample, table_lengths)

SORTED = sorted_cls(Engine)


def partners_lengths():
    for n in chain_lengths():
        for tick in (True, False):
            ps.chain_length(SORTED, OracleEngine, n, tick)
    for nq in ps.query_counts():
        for spread in (False, True):
            ps.query_count(SORTED, OracleEngine, nq, spread)


def partners_rest():
    for name in ("exact_distances", "filters", "self_exclusion", "marks_move_rotate", "seats", "roles", "several_groups",
                 "group_override", "none_duplicates_capacity", "null_outputs", "stored_anchor_has_no_partner", "partners_script"):
        getattr(ps, name)(SORTED, OracleEngine)
    for marker in ("cancel", "expire"):
        ps.marks(SORTED, OracleEngine, marker)


def move_if_lengths():
    for n in chain_lengths():
        for tick in (True, False):
            mv.chain_length(SORTED, OracleEngine, n, tick)
    for k1 in ps.query_counts():
        for spread in (False, True):
            mv.candidate_count(SORTED, OracleEngine, k1, spread)


def move_if_rest():
    for name in ("limits", "pool_at_entry", "seats", "into_company", "full_on_the_selected", "wrapped_ring", "out_plus_stamped",
                 "move_if_script"):
        getattr(mv, name)(SORTED, OracleEngine)


def table():
    for n in table_lengths():
        table_and_sample(Engine, OracleEngine, n)


def new_shapes():
    marked_twin(Engine, OracleEngine)
    role_byte(Engine, OracleEngine)
    empty_table(Engine, OracleEngine)
    route_choice(Engine, OracleEngine)


def agree():
    routes_agree(Engine)


CASES = {"partners_lengths": partners_lengths, "partners_rest": partners_rest, "move_if_lengths": move_if_lengths,
         "move_if_rest": move_if_rest, "table_and_sample": table, "new_shapes": new_shapes, "routes_agree": agree}

if __name__ == "__main__":
    import torch
    assert torch.cuda.is_available(), "GPU tests need a GPU; there is no CPU fallback"
    build()
    t0 = time.perf_counter()
    CASES[sys.argv[1]]()
    print("%s ok in %.1f s" % (sys.argv[1], time.perf_counter() - t0))
