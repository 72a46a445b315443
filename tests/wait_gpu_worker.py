"""One GPU scenario of tests/test_gpu_wait.py, in a process of its own:  python tests/wait_gpu_worker.py <case>
(the test starts it under a time limit, so a scenario that hangs ends there and takes no other one with it).
Exit status 0: the scenario held.  The drivers are those of the CPU tier (tests/wait_scenarios.py); the engine is the
product's, the witness the oracle."""
import os
import sys
import time

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, HERE)

from helpers import assert_same_state                                   # noqa: E402
from microservice_matchmaking_amd import Engine, make_config, mode_1v1, mode_team   # noqa: E402
from microservice_matchmaking_amd.synth import ROLE_WEIGHTS_5V5, make_pool          # noqa: E402
from oracle.oracle import OracleEngine, build                            # noqa: E402
import wait_scenarios as ws                                              # noqa: E402
from wait_scenarios import (Tracker, assert_wait_stats, expire_both, expiry_script, three_mode_config,   # noqa: E402
                            chunk_length, tick_both)


def script(seed, restart_at=(), tuning=None):
    """Script 1 at product geometry: tens of thousands of players a mode over seven rating groups, so the LDS-resident pair
    walk (kp_late: the longest 1v1 chain stays under PL_MAX; script_tiled below reaches the tiled rounds), the team path and
    the selection kernels' many-chunk grids all see expired entries.  Every mode expires in every round, with a
    threshold drawn from the range of one round's clock step, so whoever a round leaves behind is about as likely to go
    as to stay.  What the script must have covered to count: expired lists that together are longer than one workgroup's
    chunk of the selection kernels, and lobbies between players of different stamps."""
    log = expiry_script(Engine, OracleEngine, cfg=three_mode_config(1 << 18), seed=seed, rounds=6, first=90_000,
                        batch=20_000, restart_at=restart_at, tuning=tuning, cancel_frac=0.02, expire_p=1.0, age_max=60)
    n_exp = sum(len(x[3]) for x in log if x[0] == "expired")
    n_match = sum(len(x[3]) for x in log if x[0] == "tick")
    print("expired %d players in %d calls, %d lobbies" % (n_exp, sum(1 for x in log if x[0] == "expired"), n_match))
    assert n_exp > chunk_length() and n_match > 2000, (n_exp, n_match)
    return log


def script_restart(seed):
    assert script(seed) == script(seed, restart_at=(1, 3))


TWO_GROUPS = [(0, 2499, "low"), (2500, 5000, "high")]


def script_tiled(seed, engine_cls=Engine, small=False):
    """The same script on a two-group table with batches of up to 8 x PL_MAX players over its three modes: mode 0's longest
    chain reaches PL_MAX (asserted before the first tick), in the first round and again whenever a later batch is large enough,
    so the tiled pair rounds filter expired entries.  What it must have covered: pair_tiled_passes > 0 in a tick of mode 0 of
    a round whose expiry of mode 0 selected somebody."""
    import geometry as G
    pl_max = G.geometry(engine_cls, small=small)["PL_MAX"]
    ticks = []

    class Recording(engine_cls):
        def tick(self, mode=0, *args, **kw):
            if not ticks:
                assert int(self.queue_depth(0).max()) >= pl_max, (self.queue_depth(0), pl_max)
            m = super().tick(mode, *args, **kw)
            ticks.append((mode, self.path_stats()["pair_tiled_passes"]))
            return m

    cfg = make_config([mode_1v1(window=40, region_filter=True), mode_team(2, 3, 300, (1, 1)), mode_team(5, 2, 200, (1, 1, 1, 1, 1))],
                      capacity=1 << (40 * pl_max).bit_length(), groups=TWO_GROUPS)
    log = expiry_script(Recording, OracleEngine, cfg=cfg, seed=seed, rounds=4, first=8 * pl_max, batch=8 * pl_max,
                        cancel_frac=0.02, expire_p=1.0, age_max=60)
    assert len(ticks) == 3 * 4
    tiled = [ticks[3 * rnd][1] for rnd in range(4)]                                  # mode 0's tick of every round
    expired = [sum(len(x[3]) for x in log if x[0] == "expired" and x[1] == rnd and x[2] == 0) for rnd in range(4)]
    print("script_tiled: mode 0 per round: pair_tiled_passes %s, expired just before %s" % (tiled, expired))
    assert any(t > 0 and x > 0 for t, x in zip(tiled, expired)), (tiled, expired)


def million(mode_dict, pool_kw, seed, n=1_000_000, engine_cls=Engine):
    """A seeded pool of 1M stamped in four batches; the first (about 30 %) expires; then the tick against the oracle with
    the same cancels.  wait_stats before the expiry, after it (pending) and after the tick; matches_wait for every seat."""
    cfg = make_config([mode_dict], capacity=1 << (n - 1).bit_length())
    rating, cons = make_pool(n, seed=seed, **pool_kw)
    cuts = [0, n * 300 // 1000, n * 533 // 1000, n * 766 // 1000, n]
    with engine_cls(cfg) as a, OracleEngine(cfg) as b:
        tr = Tracker(cfg)
        for k in range(4):
            a.clock_set(1000 + 250 * k)
            tr.clock_set(1000 + 250 * k)
            sa = a.enqueue(rating[cuts[k]:cuts[k + 1]], cons[cuts[k]:cuts[k + 1]])
            sb = b.enqueue(rating[cuts[k]:cuts[k + 1]], cons[cuts[k]:cuts[k + 1]])
            assert np.array_equal(sa, sb)
            tr.enqueued(sa)
        a.clock_set(2000)
        tr.clock_set(2000)
        assert_wait_stats(a, tr, 0, "1M stamped")
        assert sum(w["waiting"] for w in a.wait_stats(0)) == n
        t0 = time.perf_counter()
        s, g, age = expire_both(a, b, tr, 0, 900, "1M, the first batch")
        assert s.size == cuts[1] and (age == 1000).all()
        print("expired %d of 1M (host time of the call + the check %.1f ms)" % (s.size, (time.perf_counter() - t0) * 1e3))
        assert_wait_stats(a, tr, 0, "1M, expiry pending")
        m = tick_both(a, b, tr, 0, "1M after the expiry")
        assert len(m) > n // 100 and np.unique(a.matches_wait()).size == 3
        assert_same_state(a, b, cfg, "1M after the expiry")
        assert_wait_stats(a, tr, 0, "1M after the tick")
        s2, _, _ = expire_both(a, b, tr, 0, 700, "1M, the second batch's leftovers")
        tick_both(a, b, tr, 0, "1M second tick")
        assert_same_state(a, b, cfg, "1M second tick")
        print("lobbies %d, second expiry %d" % (len(m), s2.size))


# ---- the targeted cases of tests/test_wait.py, at its sizes: every driver prints the line of what it covered --------------

def drivers(*calls):
    for fn, *args in calls:
        if fn is ws.clock_never_set:
            print(fn(Engine, *args))
        else:
            print(fn(Engine, OracleEngine, *args))


def selection_edges():
    drivers(*[(ws.selection_edges, delta) for delta in (-1, 0, 1)])


def expiry_cases():
    drivers((ws.everything_expires,), (ws.nothing_expires,), (ws.anchor_and_head, 0, 1), (ws.anchor_and_head, 2, 5),
            (ws.expire_cancel_overlap,), (ws.before_the_clock,))


def clock_wrap_and_ring_laps():
    drivers((ws.clock_wrap,), (ws.ring_laps,))


def histogram_and_old_ages():
    drivers((ws.every_bucket,), *[(ws.old_ages, mode, seat_oldest) for mode in (0, 2) for seat_oldest in (False, True)])


def sum_carries_and_thresholds():
    drivers(*[(ws.sum_carries, p, cancels) for cancels in (False, True) for p in ws.CARRY_PATTERNS], (ws.sum_carries, "grid", False, True),
            *[(ws.threshold_edges, max_age) for max_age in ws.EDGE_AGES + (0xFFFFFFFF,)])


def matches_wait_paths():
    # (the product's geometry: the team case is the one chain of 6000 that the team path, not k_walk, takes)
    drivers(*[(ws.matches_wait_paths, kind, True) for kind in ("pair", "team", "generic")])


def calls():
    drivers((ws.reset_keeps_the_clock,), (ws.clock_never_set,))


CASES = {
    "selection_edges": selection_edges,
    "expiry_cases": expiry_cases,
    "clock_wrap_and_ring_laps": clock_wrap_and_ring_laps,
    "histogram_and_old_ages": histogram_and_old_ages,
    "sum_carries_and_thresholds": sum_carries_and_thresholds,
    "matches_wait_paths": matches_wait_paths,
    "calls": calls,
    "script_seed1": lambda: script(1),
    "script_seed2": lambda: script(2),
    "script_generic_walk": lambda: script(3, tuning={"force_generic": 1}),
    "script_restart": lambda: script_restart(4),
    "script_tiled": lambda: script_tiled(3),      # (round 1: a chain of 20 145 entries of which 1 399 have just expired)
    "cfg2_1m": lambda: million(mode_1v1(window=25, region_filter=True), {}, 1),
    "cfg3_1m": lambda: million(mode_team(5, 2, 50, (1, 1, 1, 1, 1)), {"role_weights": ROLE_WEIGHTS_5V5}, 2),
}

if __name__ == "__main__":
    import torch
    assert torch.cuda.is_available(), "GPU tests need a GPU; there is no CPU fallback"
    build()
    t0 = time.perf_counter()
    CASES[sys.argv[1]]()
    print("%s ok in %.1f s" % (sys.argv[1], time.perf_counter() - t0))
