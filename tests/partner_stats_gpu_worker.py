"""One GPU scenario of tests/test_gpu_partner_stats.py, in a process of its own:  python tests/partner_stats_gpu_worker.py <case>
(the test starts it under a time limit, so a scenario that hangs ends there and takes no other one with it).
Exit status 0: the scenario held.  The drivers are those of the CPU tier (tests/partner_stats_scenarios.py); the engine is
the product's, the witnesses numpy over the oracle and the product's own mm_partners."""
import os
import sys
import time

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, HERE)

from microservice_matchmaking_amd import Engine                          # noqa: E402
from oracle.oracle import OracleEngine, build                            # noqa: E402
from move_scenarios import four_mode_config                              # noqa: E402
from partner_stats_scenarios import (all_equal, bias_and_clamp, errors, radix_byte, seats_and_roles, segments, sharded,   # noqa: E402
                                     stats_script, tile_boundary, tile_counts, two_modes, who_waits)
from wait_scenarios import three_mode_config                             # noqa: E402


def tiles():
    for n in tile_counts():
        tile_boundary(Engine, OracleEngine, n)
    for n in (1, 2, 65):
        tile_boundary(Engine, OracleEngine, n, tick=True)


def passes():
    for byte in range(4):
        radix_byte(Engine, OracleEngine, byte)
    all_equal(Engine, OracleEngine)
    bias_and_clamp(Engine, OracleEngine)


def places():
    segments(Engine, OracleEngine)
    two_modes(Engine, OracleEngine, three_mode_config)
    two_modes(Engine, OracleEngine, four_mode_config)


def waits():
    who_waits(Engine, OracleEngine)
    seats_and_roles(Engine, OracleEngine)
    errors(Engine)
    sharded(Engine)


def script():
    stats_script(Engine, OracleEngine)


CASES = {"tile_boundaries": tiles, "passes_bias_and_clamp": passes, "segments_and_modes": places, "who_waits_and_calls": waits,
         "script": script}

if __name__ == "__main__":
    import torch
    assert torch.cuda.is_available(), "GPU tests need a GPU; there is no CPU fallback"
    build()
    t0 = time.perf_counter()
    CASES[sys.argv[1]]()
    print("%s ok in %.1f s" % (sys.argv[1], time.perf_counter() - t0))
