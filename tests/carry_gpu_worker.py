"""One GPU scenario of tests/test_gpu_carry.py, in a process of its own:  python tests/carry_gpu_worker.py <case>
(the test starts it under a time limit, so a scenario that hangs ends there and takes no other one with it).
Exit status 0: the scenario held.  The drivers are those of the CPU tier (tests/carry_scenarios.py); the engine is the
product's, the witnesses mm_move on a second engine of the product and the oracle."""
import os
import sys
import time

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, HERE)

import numpy as np                                                       # noqa: E402

from microservice_matchmaking_amd import Engine                          # noqa: E402
from oracle.oracle import OracleEngine, build                            # noqa: E402
from carry_scenarios import (RANK_WEIGHTS, RankFailure, full_pool, one_engine, rank_script, rows_cases, script_worker, spawn,   # noqa: E402
                             stamped_edges, stamped_refused, stamped_ring, twin_script)
from microservice_matchmaking_amd.sharding import ChainSharding, union_digest   # noqa: E402
from move_scenarios import four_mode_config                               # noqa: E402


def twins(seed, restart_at=(), capacity=8192):
    """The twin-engine script at product geometry: capacity 8192 or 16 384, about 1 500 and then up to 400 players a round,
    eight rounds, two HIP engines in this process (mm_move on one, the two-call route on the other) and the oracle."""
    moved, refused, lobbies = twin_script(Engine, OracleEngine, seed=seed, restart_at=restart_at, capacity=capacity)
    print("moved %d players (%d refused), lobbies per mode %s" % (moved, refused, lobbies))
    assert moved > 100 and lobbies[2] > 5 and lobbies[3] > 5, (moved, lobbies)


def ring():
    for in_the_way in (False, True):
        stamped_ring(Engine, OracleEngine, in_the_way, capacity=8192)


def two_ranks():
    """Two processes, two HIP engines, one device, over gloo: the cross-rank script against ONE HIP engine's mm_move.  The
    ranks run first and are gone before this process opens the GPU: never more than two processes hold it."""
    own = ChainSharding(4, 7, 2, RANK_WEIGHTS[2]).chain_owner
    assert (own[2] != own[3]).any() and (own[2] == own[3]).any()
    gathered, owner = spawn(script_worker, 2, ("hip",), timeout=150)
    assert owner == own.tolist()
    want = one_engine(Engine, four_mode_config(), rank_script)
    got = {}
    for res in gathered:
        assert not (set(res["digests"]) & set(got))
        got.update(res["digests"])
    assert set(got) == set(want["digests"]) and union_digest(got) == union_digest(want["digests"])
    for k in ("selected", "refused", "taken", "expired"):
        assert sum(r[k] for r in gathered) == want[k], (k, [r[k] for r in gathered], want[k])
    for md in range(4):
        assert np.array_equal(np.sort(np.concatenate([r["waits"][md] for r in gathered])), want["waits"][md]), md
    print("selected per rank %s, taken per rank %s, one engine %d" % ([r["selected"] for r in gathered],
                                                                      [r["taken"] for r in gathered], want["selected"]))
    assert want["selected"] > 100 and min(r["taken"] for r in gathered) > 0


CASES = {
    "twins_seed1": lambda: twins(1),
    "twins_seed2_restart": lambda: twins(2, restart_at=(2, 5), capacity=16384),
    "stamped_edges_slot_list": lambda: print("batch sizes %s" % stamped_edges(Engine, OracleEngine, capacity=8192)),
    "ring_wrap": ring,
    "rows": lambda: print("rows: %s" % rows_cases(Engine, OracleEngine)),
    "roles_refused": lambda: print("refused %d" % stamped_refused(Engine, OracleEngine)),
    "full_pool": lambda: full_pool(Engine, OracleEngine),
    "two_ranks": two_ranks,
}

if __name__ == "__main__":
    build()
    t0 = time.perf_counter()
    if sys.argv[1] != "two_ranks":                                       # (two_ranks: its rank processes open the GPU first)
        import torch
        assert torch.cuda.is_available(), "GPU tests need a GPU; there is no CPU fallback"
    try:
        CASES[sys.argv[1]]()
    except RankFailure as ex:
        # a rank that hung or died of a signal: this process ends with the status the test stops the module on
        print("%s: %s" % (sys.argv[1], ex))
        sys.stdout.flush()
        sys.exit(ex.status)
    print("%s ok in %.1f s" % (sys.argv[1], time.perf_counter() - t0))
