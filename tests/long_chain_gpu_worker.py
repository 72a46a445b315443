"""One GPU case of tests/test_gpu_long_chain.py, in a process of its own:  python tests/long_chain_gpu_worker.py <case>
(the test starts it under a time limit, so a case that hangs ends there and takes no other one with it).
Exit status 0: the case held.  The drivers are those of the CPU tier (tests/long_chain_scenarios.py) at the product's
geometry (tests/geometry.py); the engine is the product's, the witness numpy over the oracle.  Every driver prints one line of
mm_path_stats counters per tick it was built for."""
import os
import sys
import time

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, HERE)

import geometry as G                                                     # noqa: E402
from microservice_matchmaking_amd import Engine                          # noqa: E402
from oracle.oracle import OracleEngine, build                            # noqa: E402
import long_chain_scenarios as lc                                        # noqa: E402


def geo():
    return G.geometry(Engine, small=False)


def pair_moved_in(which):
    for route in ("move", "move_out+stamped"):
        for wrapped in (False, True):
            lc.pair_moved_in(Engine, OracleEngine, geo(), which, route, wrapped)


def pair_rotated():
    for tuning in (None, {"pair_persist": 0}):
        lc.pair_rotated(Engine, OracleEngine, geo(), tuning)


def team_moved_in():
    for tuning, path_ok in lc.TEAM_TUNINGS:
        lc.team_moved_in(Engine, OracleEngine, geo(), tuning, path_ok)


def team_refused():
    lc.team_moved_in(Engine, OracleEngine, geo(), *lc.TEAM_TUNINGS[0], clear=False)


def team_stream_regime():
    print("team_stream_regime: %d lobbies, the same with team_late0 = 0" % lc.team_stream_regime_both(Engine, OracleEngine, geo()))


def stream_long():
    print("stream_long: matched %d, moved %s, rotated %s in %s rounds" % lc.stream_long(Engine, OracleEngine, geo()))


CASES = {
    "pair_moved_in_below": lambda: pair_moved_in("PL_MAX-1"),
    "pair_moved_in_at": lambda: pair_moved_in("PL_MAX"),
    "pair_moved_in_tiles": lambda: pair_moved_in("3xPK_T+1"),
    "pair_rotated": pair_rotated,
    "team_moved_in": team_moved_in,
    "team_refused": team_refused,
    "team_stream_regime": team_stream_regime,
    "stream_long": stream_long,
    "long_script_seed2": lambda: lc.long_script(Engine, OracleEngine, geo(), seed=2),
    "long_script_seed6_restart": lambda: lc.long_script(Engine, OracleEngine, geo(), seed=6, restart_at=(1,)),
    "long_script_generic_walk": lambda: lc.long_script(Engine, OracleEngine, geo(), seed=4, tuning={"force_generic": 1}, coverage=False),
}

if __name__ == "__main__":
    import torch
    assert torch.cuda.is_available(), "GPU tests need a GPU; there is no CPU fallback"
    build()
    t0 = time.perf_counter()
    CASES[sys.argv[1]]()
    print("%s ok in %.1f s" % (sys.argv[1], time.perf_counter() - t0))
