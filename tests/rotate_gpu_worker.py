"""One GPU scenario of tests/test_gpu_rotate.py, in a process of its own:  python tests/rotate_gpu_worker.py <case>
(the test starts it under a time limit, so a scenario that hangs ends there and takes no other one with it).
Exit status 0: the scenario held.  The drivers are those of the CPU tier (tests/rotate_scenarios.py); the engine is the
product's, the witness the oracle."""
import os
import sys
import time

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, HERE)

from microservice_matchmaking_amd import Engine                          # noqa: E402
from oracle.oracle import OracleEngine, build                            # noqa: E402
from rotate_scenarios import (SHAPES, assert_share, blocked_head, boundaries, dead_seat, errors, full_one_short,   # noqa: E402
                              group_counts, group_override, host_route_equivalence, lobby_shape, pair_geometry,
                              rotate_script, slots_contiguous, slots_wrapped_with_a_waiting_player_in_the_way,
                              team_geometry)


def script(seed, restart_at=()):
    log, calls, hits = rotate_script(Engine, OracleEngine, seed=seed, restart_at=restart_at)
    assert_share(calls, hits)
    return log


def script_restart(seed):
    assert script(seed, restart_at=(2, 5)) == script(seed)


def named():
    """The small closed forms, one after another (each a fraction of a second)."""
    blocked_head(Engine, OracleEngine)
    for n in (1, 7, 16):
        print("groups %d: selected %s" % (n, group_counts(Engine, OracleEngine, n)))
    for name in sorted(SHAPES):
        assert lobby_shape(Engine, OracleEngine, name) == SHAPES[name][3]
    dead_seat(Engine, OracleEngine)
    boundaries(Engine, OracleEngine)
    group_override(Engine, OracleEngine)


def slots():
    slots_contiguous(Engine, OracleEngine)
    slots_wrapped_with_a_waiting_player_in_the_way(Engine, OracleEngine)
    full_one_short(Engine, OracleEngine)


CASES = {
    "named_cases": named,
    "slots_and_full_pool": slots,
    "errors": lambda: errors(Engine),
    "host_route": lambda: print("rotated %d" % host_route_equivalence(Engine, OracleEngine)),
    "script_seed1": lambda: script(1),
    "script_seed2_restart": lambda: script_restart(2),
    "pair_geometry": lambda: print("lobbies %d then %d, paths %d" % pair_geometry(Engine, OracleEngine)),
    "team_geometry": lambda: print("lobbies %d, paths %d" % team_geometry(Engine, OracleEngine)),
}

if __name__ == "__main__":
    import torch
    assert torch.cuda.is_available(), "GPU tests need a GPU; there is no CPU fallback"
    build()
    t0 = time.perf_counter()
    CASES[sys.argv[1]]()
    print("%s ok in %.1f s" % (sys.argv[1], time.perf_counter() - t0))
