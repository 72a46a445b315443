#!/usr/bin/env python
"""Test infrastructure (it drives the oracle, so it lives under tests/).  Randomised differential stress on a real GPU: HIP engine vs oracle over many seeded
scenarios (pool sizes that hit the LDS-resident walk, the tiled rounds and the hand-over
between them; windows from 0 to wider than the rating span; 1..64 regions; multi-tick with
arrivals and cancels).  Usage: python tests/stress.py [seconds] [seed] [team] [--fuzz-knobs] [--wide] [--edges] [--patterns] [--wait]

--fuzz-knobs (round 6): every scenario's engine is created with a random COMBINATION of the engine's tuning fields
(include/mm_engine.h mm_tuning, passed per engine through mm_engine_create_ex) off their defaults — batch sizes, the
persistent launch shapes on / off / cut short, bounded waits of zero, the test hooks that make a kp_rounds launch stop at a
random iteration and a kt_fc chunk flag never come.  Round 5's tile-length bug needed a stop of kp_rounds to show and no
default-configuration test could see it; one knob at a time found it, combinations are what this draws.  The draw is a
function of the scenario's seed alone (MM_STRESS_ONLY=<seed> replays scenario AND knobs); a failure prints both.

--wide: configurations past the reference's shape instead — 1-16 rating groups from random tables (contiguous,
overlapping, gapped; default group anywhere), 1-16 modes (1v1 and team modes, up to 256 chains), ratings spanning the
whole table and beyond it; scores checked exactly (helpers.exact_scores).  Its draws come from a stream of their own:
without the flag every seed gives the scenario it always gave.

--edges: chains of EXACT length instead — one or two rating groups, every batch sized so that a chain starts its tick at
B + d players, B from the boundary tables of tests/geometry.py (the lengths at which the kernels and the host loop switch
behaviour, read from the source and computed from the drawn tuning), d from -2 .. 2.  A stream of its own as well.

--patterns: STRUCTURED arrival orders instead of i.i.d. draws — the first batch is a family of tests/patterns.py (nested,
shifted, sorted, runs, interleaved, blocked head, dead tiles, alive share; with `team`: dense, nested, shifted members,
scarce / sorted / missing roles) with its parameter from the geometry tables of the drawn tuning; later batches are
another pattern or a random pool; cancels are a whole range, every m-th player or random.  A stream of its own.

--wait: the wait layer (include/mm_wait.h) in front of the long-chain walks instead — tests/long_chain_scenarios.py's
long_script with a drawn seed, round count and restart round: moves, rule calls, stamped enqueues, rotations, locate and
partners between ticks whose chains the tiled pair path and the team path take, against the oracle and the numpy witnesses
after every call; sizes from tests/geometry.py for the engine's build.  A stream of its own.

MM_STRESS_ENGINE=emu_small runs the same scenarios without a GPU on the fiber-shim build of the
kernel source with the tiny tile geometry (tests/emu/), pool sizes divided by 16 so that they
land on the same paths (LDS-resident walk / tiled rounds / hand-over; team path / k_walk)."""
import os
import sys
import time

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, ROOT)
sys.path.insert(0, HERE)

from helpers import assert_exact_scores, assert_exact_scores_any, assert_same_state, assert_same_tick  # noqa: E402
from microservice_matchmaking_amd import Engine, cons_make, make_config, mode_1v1, mode_team  # noqa: E402
from microservice_matchmaking_amd._abi import NO_SLOT  # noqa: E402
from oracle.oracle import OracleEngine  # noqa: E402

SCALE = 1
if os.environ.get("MM_STRESS_ENGINE", "gpu") == "emu_small":
    from emu_engine import EmuEngineSmall as Engine  # noqa: E402,F811
    SCALE = 16
elif os.environ.get("MM_STRESS_ENGINE", "gpu") == "emu":      # product geometry under the shim: slow, sizes as on the GPU
    from emu_engine import EmuEngine as Engine  # noqa: E402,F811


def scaled(n):
    return int(n) // SCALE if n >= 100 else int(n)


FUZZ = False          # set by main() from the command line

# field of mm_tuning -> the values a draw picks from (the default is always among them or is what "not drawn" leaves)
PAIR_KNOBS = {
    "pair_persist": [0, 1], "pair_ptiles": [3, 5, 6, 8, 12, 20, 32], "pair_pbatch": [1, 2, 7, 48, 96],
    "pair_batch": [1, 2, 7, 48], "pair_ptimeout_us": [0, 50, 5000], "pair_pinject": [0] + list(range(1, 41)),
    "pair_tiles_max": [10, 20, 40], "pair_tile_fixed": [0, 1], "pair_xcd": [0, 1], "pair_group_min": [0, 4, 64],
    "pair_nxseg": [0, 64, 256, 1024, 2048], "pair_nxstage": [0, 512, 2048],
}
TEAM_KNOBS = {
    "team_batch": [1, 2, 4, 16], "team_f2": [0, 1, 3, 32, 1000], "team_rebuild": [1, 3, 8, 32], "team_emit_max": [1, 2, 8, 32],
    "team_split": [0, 1], "team_fwait": [0, 16, 16384], "team_fix_max": [0, 3, 0xFFFFFFFF], "team_fix_t8": [0, 10, 64],
    "team_fix_t4": [0, 64, 1000], "team_pull_xcd": [0, 1], "team_nowait": [0, 1, 2, 3, 7], "team_late": [0, 1, 6, 80],
    "team_late0": [0, 512, 10 ** 7], "team_cap": [8, 64, 512, 4096],
}
COMMON_KNOBS = {"results_early": [0, 1], "results_tail": [0, 1], "look_poll": [0, 1]}


def draw_tuning(seed, tables):
    """None without --fuzz-knobs; else {field: value}: every field of `tables` drawn with probability 0.35."""
    if not FUZZ:
        return None
    krng = np.random.default_rng([int(seed), 0x6B6E6F62])       # its own stream: the scenario is the same with and without
    t = {}
    for table in tables + [COMMON_KNOBS]:
        for name, menu in table.items():
            if krng.random() < 0.35:
                t[name] = int(menu[krng.integers(0, len(menu))])
    if krng.integers(0, 50) == 0:
        t["force_generic"] = 1
    return t


def random_team_mode(rng):
    """A team mode the config validator accepts: teams * team_size <= 16, quotas sum to team_size."""
    teams = int(rng.choice([2, 2, 2, 3, 4]))
    team_size = int(rng.integers(1 if teams > 2 else 2, 16 // teams + 1))
    team_size = min(team_size, 8)
    n_roles = int(rng.integers(1, min(team_size, 5) + 1))
    quota = np.ones(n_roles, np.int64)
    for _ in range(team_size - n_roles):
        quota[rng.integers(0, n_roles)] += 1
    window = int(rng.choice([5, 25, 50, 150, 600, 10 ** 6]))
    return mode_team(team_size, teams, window, tuple(int(q) for q in quota),
                     region_filter=bool(rng.integers(0, 3) == 0), party_filter=bool(rng.integers(0, 5) == 0))


def random_group_table(rng):
    """1-16 groups: contiguous, overlapping (the lowest index wins) or with gaps (the default group takes them)."""
    n = int(rng.integers(1, 17))
    kind = int(rng.integers(0, 3))
    width = int(rng.choice([1, 50, 300, 1000, 5000]))
    lo = int(rng.choice([0, 0, -3000, 1500]))
    rows = []
    for i in range(n):
        a = lo + i * width
        if kind == 1:                                           # overlapping: each reaches into the next ones
            a -= int(rng.integers(0, width + 1))
            b = a + width + int(rng.integers(0, 2 * width + 1))
        elif kind == 2:                                         # gaps: a share of each step is nobody's
            b = a + max(0, width - 1 - int(rng.integers(0, width // 2 + 1)))
        else:
            b = a + width - 1
        rows.append((a, b, "g%d" % i))
    return rows, int(rng.integers(0, n))


def wide_main(budget, seed0):
    """--wide: group tables, mode counts and rating ranges past the reference's seven groups and four modes."""
    t_end = time.time() + budget
    n_done = 0
    k = 0
    only = os.environ.get("MM_STRESS_ONLY")
    while time.time() < t_end:
        seed = seed0 * 100003 + k
        k += 1
        if only:
            if k > 1:
                break
            seed = int(only)
        rng = np.random.default_rng([seed, 0x77696465])
        groups, dflt = random_group_table(rng)
        n_modes = int(rng.choice([1, 2, 4, 16]))
        modes = []
        for _ in range(n_modes):
            if rng.integers(0, 2):
                window = int(rng.choice([0, 3, 25, 200, 10 ** 6, 0x3FFFFFFF]))
                modes.append(mode_1v1(window=window, region_filter=bool(rng.integers(0, 2)),
                                      party_filter=bool(rng.integers(0, 4) == 0)))
            else:
                modes.append(random_team_mode(rng))
        chains = n_modes * len(groups)
        capacity = 1 << (18 if chains <= 16 else 16)
        cfg = make_config(modes, capacity=capacity, groups=groups, default_group=dflt, timing=False)
        lo = min(g[0] for g in groups) - 100
        hi = max(g[1] for g in groups) + 100
        regions = int(rng.choice([1, 2, 8]))
        top = 40000 if chains <= 16 else 12000
        sizes = [scaled(rng.choice([50, 3000, 20000, top]))] + \
                [scaled(rng.choice([0, 100, 3000])) for _ in range(int(rng.integers(0, 3)))]
        tag = "wide seed %d groups=%s default=%d modes=%s sizes=%s" % (seed, groups, dflt, modes, sizes)
        if os.environ.get("MM_STRESS_VERBOSE"):
            print(tag, flush=True)
        rating_of = {}
        with Engine(cfg) as a, OracleEngine(cfg) as b:
            live = np.zeros(0, np.uint32)
            for j, n in enumerate(sizes):
                rating = rng.integers(lo, hi + 1, size=n).astype(np.int32)
                mode = rng.integers(0, n_modes, size=n)
                role = np.array([rng.integers(0, modes[int(m)]["n_roles"]) for m in mode], dtype=np.int64)
                cons = cons_make(mode, rng.integers(0, regions, size=n), rng.integers(0, 3, size=n), role)
                sa, sb = a.enqueue(rating, cons), b.enqueue(rating, cons)
                assert np.array_equal(sa, sb), tag
                ok = sa != NO_SLOT
                rating_of.update(zip(sa[ok].tolist(), rating[ok].tolist()))
                live = np.concatenate([live, sa[ok]])
                if live.size > 10 and rng.integers(0, 3) == 0:
                    cs = rng.choice(live, size=max(1, live.size // 50), replace=False)
                    a.cancel(cs)
                    b.cancel(cs)
                    live = np.setdiff1d(live, cs)
                for md in range(n_modes):
                    ma, mb = a.tick(md), b.tick(md)
                    assert_same_tick(ma, mb, tag + " tick %d mode %d" % (j, md))
                    assert_exact_scores(ma, cfg.modes[md], rating_of, tag + " tick %d mode %d" % (j, md))
                    live = np.setdiff1d(live, ma.slots.ravel())
                assert_same_state(a, b, cfg, tag)
        n_done += 1
    print("gpu_stress --wide: %d scenarios ok (seeds %d..%d)" % (n_done, seed0 * 100003, seed0 * 100003 + k - 1))


def edges_main(budget, seed0, count=None):
    """--edges: chains of exact length.  One or two rating groups, every batch sized so that ONE chain starts its tick at
    B + d players — B from the boundary tables of the running engine (tests/geometry.py: read from the source, computed from
    the DRAWN tuning with --fuzz-knobs, whose pair_ptiles / pair_tiles_max / pair_group_min move boundaries), d from
    -2 .. 2 — predicates and cancels as in the default family.  Draws come from a stream of their own.  `count`: that
    many scenarios instead of a time budget."""
    import geometry
    t_end = time.time() + budget
    n_done = 0
    k = 0
    only = os.environ.get("MM_STRESS_ONLY")
    while time.time() < t_end and (count is None or k < count):
        seed = seed0 * 100003 + k
        k += 1
        if only:
            if k > 1:
                break
            seed = int(only)
        rng = np.random.default_rng([seed, 0x65646765])
        team = bool(rng.integers(0, 3) == 0)
        tuning = draw_tuning(seed, [TEAM_KNOBS if team else PAIR_KNOBS])
        geo = geometry.geometry(Engine, small=SCALE > 1, tuning=tuning)
        table = geometry.team_boundaries(geo) if team else geometry.pair_boundaries(geo)
        # what a scenario may cost: the oracle walks a chain on one thread; the shim pays for every pass of every tile
        top = (1 << 18) if SCALE == 1 else 10 * geo["PK_T"]
        table = [e for e in table if 8 <= e[0] <= top]
        if team:
            window = int(rng.choice([25, 150, 600, 10 ** 6]))
            modes = [mode_team(2, 2, window, (1, 1)) if rng.integers(0, 2) else mode_team(5, 2, window, (1, 1, 1, 1, 1))]
            regions, party = 1, False
        else:
            window = int(rng.choice([0, 1, 3, 10, 25, 60, 200, 1000, 10 ** 6]))
            regions = int(rng.choice([1, 2, 4, 8, 64]))
            party = bool(rng.integers(0, 4) == 0)
            modes = [mode_1v1(window=window, region_filter=regions > 1, party_filter=party)]
        nr = modes[0]["n_roles"]
        two = bool(rng.integers(0, 2))
        groups = [(0, 2499, "low"), (2500, 5000, "high")] if two else [(0, 5000, "all")]
        aim = int(rng.integers(0, len(groups)))                     # the group whose chain is aimed at the boundary
        targets = [int(table[rng.integers(0, len(table))][0]) + int(rng.integers(-2, 3)) for _ in range(int(rng.integers(1, 4)))]
        cfg = make_config(modes, capacity=2 * max(targets) + 4096, groups=groups, default_group=0, timing=False)
        tag = "edges seed %d team=%d w=%d regions=%d party=%d groups=%d aim=%d targets=%s tuning=%s" % (
            seed, team, window, regions, party, len(groups), aim, targets, tuning)
        if os.environ.get("MM_STRESS_VERBOSE"):
            print(tag, flush=True)
        rating_of = np.zeros(cfg.capacity, np.int64)
        with (Engine(cfg, tuning) if tuning else Engine(cfg)) as a, OracleEngine(cfg) as b:
            live = np.zeros(0, np.uint32)
            for j, target in enumerate(targets):
                # cancels first (they are purged at the head of the tick), then the batch that brings the aimed chain —
                # the ORACLE's depth minus the cancelled players still in it — to the target exactly
                if live.size > 10 and rng.integers(0, 3) == 0:
                    cs = rng.choice(live, size=max(1, live.size // 50), replace=False)
                    a.cancel(cs)
                    b.cancel(cs)
                    live = np.setdiff1d(live, cs)
                qs = np.intersect1d(b.queue_slots(0, aim), live)
                if qs.size > target:                                 # an earlier target left more: the surplus gives up as well
                    cs = rng.choice(qs, size=qs.size - target, replace=False)
                    a.cancel(cs)
                    b.cancel(cs)
                    live = np.setdiff1d(live, cs)
                n = max(0, target - qs.size)
                lo, hi = groups[aim][0], groups[aim][1]
                rating = rng.integers(lo, hi + 1, size=n).astype(np.int32)
                if two:                                              # a few players for the other chain as well
                    other = groups[1 - aim]
                    rating = np.concatenate([rating, rng.integers(other[0], other[1] + 1, size=int(rng.integers(0, 40))).astype(np.int32)])
                    rating = rating[rng.permutation(rating.size)]
                n = rating.size
                cons = cons_make(0, rng.integers(0, regions, size=n), rng.integers(0, 3 if party else 1, size=n), rng.integers(0, nr, size=n))
                sa, sb = a.enqueue(rating, cons), b.enqueue(rating, cons)
                assert np.array_equal(sa, sb), tag
                rating_of[sa] = rating
                live = np.concatenate([live, sa])
                # the family's point: the aimed chain starts this tick (behind the purge) at the target, exactly
                assert np.intersect1d(b.queue_slots(0, aim), live).size == target, (tag, j)
                ma, mb = a.tick(0), b.tick(0)
                assert_same_tick(ma, mb, tag + " tick %d" % j)
                assert_exact_scores_any(ma, cfg.modes[0], rating_of, tag + " tick %d" % j)
                live = np.setdiff1d(live, ma.slots.ravel())
                assert_same_state(a, b, cfg, tag)
        n_done += 1
    print("gpu_stress --edges%s: %d scenarios ok (seeds %d..%d)" % (" --fuzz-knobs" if FUZZ else "", n_done, seed0 * 100003, seed0 * 100003 + k - 1))


def patterns_main(budget, seed0, team=False, count=None):
    """--patterns: see the module docstring.  The first tick of the first pattern is also held against the family's
    closed form (lobbies; the pass structure and pairs where it has one) on the ORACLE's side."""
    import geometry
    import patterns
    t_end = time.time() + budget
    n_done = 0
    k = 0
    only = os.environ.get("MM_STRESS_ONLY")
    while time.time() < t_end and (count is None or k < count):
        seed = seed0 * 100003 + k
        k += 1
        if only:
            if k > 1:
                break
            seed = int(only)
        rng = np.random.default_rng([seed, 0x70617474])
        tuning = draw_tuning(seed, [TEAM_KNOBS if team else PAIR_KNOBS])
        geo = geometry.geometry(Engine, small=SCALE > 1, tuning=tuning)
        # what a scenario may cost: the oracle walks a chain on one thread, the shim pays for every pass of every tile
        max_players, max_passes = ((1 << 17), 6000) if SCALE == 1 else (5 * geo["PK_T"], 600)
        cases = [patterns.draw(rng, geo, team, max_players, max_passes)]
        later = []                                               # after the first pattern: another pattern or a random pool
        for _ in range(int(rng.integers(0, 3))):
            later.append(patterns.draw(rng, geo, team, max_players, max_passes) if rng.integers(0, 2) else int(scaled(rng.choice([100, 3000, 20000]))))
        m = cases[0].mode
        mode = mode_1v1(window=m[1], region_filter=m[2]) if m[0] == "1v1" else mode_team(m[1], m[2], m[3], m[4])
        nr = mode["n_roles"]
        two = bool(rng.integers(0, 2))
        groups = [patterns.GROUP + ("all",)] + ([(patterns.GROUP[1] + 1, patterns.GROUP[1] + 5000, "other")] if two else [])
        total = cases[0].players + sum(x if isinstance(x, int) else x.players for x in later)
        cfg = make_config([mode], capacity=total + 4096 + (scaled(30000) if two else 0), groups=groups, default_group=0, timing=False)
        tag = "patterns seed %d team=%d first=%s later=%s groups=%d tuning=%s" % (
            seed, team, cases[0], [x if isinstance(x, int) else str(x) for x in later], len(groups), tuning)
        if os.environ.get("MM_STRESS_VERBOSE"):
            print(tag, flush=True)
        rating_of = np.zeros(cfg.capacity, np.int64)
        with (Engine(cfg, tuning) if tuning else Engine(cfg)) as a, OracleEngine(cfg) as b:
            live = np.zeros(0, np.uint32)
            ticks = 0

            def enqueue(rating, cons):
                nonlocal live
                sa, sb = a.enqueue(rating, cons), b.enqueue(rating, cons)
                assert np.array_equal(sa, sb), tag
                rating_of[sa] = rating
                live = np.concatenate([live, sa])
                return sa

            def cancel(cs):
                nonlocal live
                cs = np.asarray(cs, np.uint32)
                a.cancel(cs)
                b.cancel(cs)
                live = np.setdiff1d(live, cs)

            def tick(expect=None):
                nonlocal live, ticks
                ma, mb = a.tick(0), b.tick(0)
                if expect is not None:                            # the pattern did not degenerate: the oracle's side of the closed form
                    g0 = mb.group == 0
                    assert int(g0.sum()) == expect.lobbies, (tag, "closed form: lobbies", int(g0.sum()), expect.lobbies)
                    if expect.passes is not None:
                        assert np.bincount(mb.pass_[g0].astype(np.int64), minlength=expect.n_passes).tolist() == expect.per_pass, (tag, "closed form: lobbies per pass")
                        if not two:
                            assert mb.stats["pairs"] == expect.pairs and mb.stats["passes_max"] == expect.n_passes, (tag, "closed form: pairs, passes")
                assert_same_tick(ma, mb, tag + " tick %d" % ticks)
                assert_exact_scores_any(ma, cfg.modes[0], rating_of, tag + " tick %d" % ticks)
                live = np.setdiff1d(live, ma.slots.ravel())
                assert_same_state(a, b, cfg, tag + " tick %d" % ticks)
                ticks += 1

            def play(case, closed_form):
                """The case's own script: enqueues, its structured cancels, its ticks."""
                mine = np.zeros(0, np.uint32)
                first = closed_form
                for step in case.steps:
                    if step[0] == "enqueue":
                        cs = step[2]
                        if not closed_form:                       # a later family's roles folded into the ones this mode knows
                            cs = (cs & np.uint32(0xFFF0FFFF)) | ((((cs >> np.uint32(16)) & np.uint32(0xF)) % np.uint32(nr)) << np.uint32(16))
                        mine = np.concatenate([mine, enqueue(step[1], cs)])
                        if first and two:                         # a random pool for the other chain rides along
                            n2 = int(scaled(rng.choice([50, 3000, 30000])))
                            enqueue((groups[1][0] + rng.integers(0, 300, size=n2)).astype(np.int32), cons_make(0, 0, 0, rng.integers(0, nr, size=n2)))
                        first = False
                    elif step[0] == "cancel":
                        cancel(mine[step[1]])
                    else:
                        tick(step[1] if closed_form else None)

            play(cases[0], True)
            for x in later:
                if live.size > 10:                                # structured or random cancels among those still waiting
                    kind = int(rng.integers(0, 4))
                    q = np.intersect1d(b.queue_slots(0, 0), live)
                    if kind == 0 and q.size > 4:                  # a whole range of the queue
                        lo = int(rng.integers(0, q.size - 1))
                        cancel(b.queue_slots(0, 0)[lo:lo + int(rng.integers(1, max(2, q.size // 3)))])
                    elif kind == 1 and q.size > 4:                # every m-th queued player
                        cancel(b.queue_slots(0, 0)[int(rng.integers(0, 3))::int(rng.integers(2, 9))])
                    elif kind == 2:
                        cancel(rng.choice(live, size=max(1, live.size // 50), replace=False))
                if isinstance(x, int):
                    enqueue(rng.integers(0, 5001, size=x).astype(np.int32), cons_make(0, rng.integers(0, 4, size=x), 0, rng.integers(0, nr, size=x)))
                    tick()
                else:
                    play(x, False)                                # (its players under THIS scenario's mode: parity only)
        n_done += 1
    print("gpu_stress --patterns%s%s: %d scenarios ok (seeds %d..%d)" % (" team" if team else "", " --fuzz-knobs" if FUZZ else "", n_done, seed0 * 100003, seed0 * 100003 + k - 1))


def team_main(budget, seed0):
    """Team modes only: long chains take mm_team.inc, short ones and cancel ticks k_walk."""
    t_end = time.time() + budget
    n_done = 0
    k = 0
    only = os.environ.get("MM_STRESS_ONLY")
    while time.time() < t_end:
        seed = seed0 * 100003 + k
        k += 1
        if only:
            if k > 1:
                break
            seed = int(only)
        rng = np.random.default_rng(seed)
        modes = [random_team_mode(rng)]
        nr = modes[0]["n_roles"]
        cfg = make_config(modes, capacity=1 << 18, timing=False)
        regions = int(rng.choice([1, 2, 8])) if modes[0]["region_filter"] else 1
        parties = 3 if modes[0]["party_filter"] else 1
        lo = int(rng.choice([0, 0, 1000, 2400]))
        hi = int(rng.choice([1499, 2600, 5000, 5000]))
        if hi <= lo:
            hi = lo + 600
        w = rng.random(nr) + 0.05
        w /= w.sum()
        sizes = [scaled(rng.choice([3000, 20000, 60000, 120000]))] + \
                [scaled(rng.choice([0, 100, 5000, 30000])) for _ in range(int(rng.integers(0, 4)))]
        tuning = draw_tuning(seed, [TEAM_KNOBS])
        tag = "team seed %d mode=%s ratings=[%d,%d] sizes=%s tuning=%s" % (seed, modes[0], lo, hi, sizes, tuning)
        if os.environ.get("MM_STRESS_VERBOSE"):
            print(tag, flush=True)
        with (Engine(cfg, tuning) if tuning else Engine(cfg)) as a, OracleEngine(cfg) as b:
            live = np.zeros(0, np.uint32)
            for j, n in enumerate(sizes):
                rating = rng.integers(lo, hi + 1, size=n).astype(np.int32)
                cons = cons_make(0, rng.integers(0, regions, size=n), rng.integers(0, parties, size=n),
                                 rng.choice(nr, size=n, p=w))
                sa, sb = a.enqueue(rating, cons), b.enqueue(rating, cons)
                assert np.array_equal(sa, sb), tag
                live = np.concatenate([live, sa])
                if live.size > 10 and rng.integers(0, 4) == 0:
                    cs = rng.choice(live, size=max(1, live.size // 50), replace=False)
                    a.cancel(cs)
                    b.cancel(cs)
                    live = np.setdiff1d(live, cs)
                ma, mb = a.tick(0), b.tick(0)
                assert_same_tick(ma, mb, tag + " tick %d" % j)
                live = np.setdiff1d(live, ma.slots.ravel())
                assert_same_state(a, b, cfg, tag)
        n_done += 1
    print("gpu_stress team%s: %d scenarios ok (seeds %d..%d)" % (" --fuzz-knobs" if FUZZ else "", n_done, seed0 * 100003, seed0 * 100003 + k - 1))


def wait_main(budget, seed0):
    """--wait: long_chain_scenarios.long_script, drawn."""
    import geometry as G
    from long_chain_scenarios import long_script
    geo = G.geometry(Engine, small=SCALE != 1)
    t_end = time.time() + budget
    n_done = 0
    k = 0
    only = os.environ.get("MM_STRESS_ONLY")
    while time.time() < t_end:
        seed = seed0 * 100003 + k
        k += 1
        if only:
            if k > 1:
                break
            seed = int(only)
        rng = np.random.default_rng([seed, 0x77616974])
        rounds = int(rng.integers(2, 4))
        restart_at = (int(rng.integers(0, rounds)),) if rng.integers(0, 3) == 0 else ()
        tuning = draw_tuning(seed, [PAIR_KNOBS, TEAM_KNOBS])
        tag = "wait seed %d rounds=%d restart_at=%s tuning=%s" % (seed, rounds, restart_at, tuning)
        if os.environ.get("MM_STRESS_VERBOSE"):
            print(tag, flush=True)
        try:
            long_script(Engine, OracleEngine, geo, seed=seed, rounds=rounds, restart_at=restart_at, tuning=tuning, coverage=False)
        except AssertionError as ex:
            raise AssertionError("%s: %s" % (tag, ex)) from ex
        n_done += 1
    print("gpu_stress --wait%s: %d scenarios ok (seeds %d..%d)" % (" --fuzz-knobs" if FUZZ else "", n_done, seed0 * 100003, seed0 * 100003 + k - 1))


def main(argv=None):
    global FUZZ
    argv = list(sys.argv[1:] if argv is None else argv)
    FUZZ = "--fuzz-knobs" in argv
    ARGV = [a for a in argv if not a.startswith("--")]
    budget = float(ARGV[0]) if len(ARGV) > 0 else 30.0
    seed0 = int(ARGV[1]) if len(ARGV) > 1 else 1
    if "--wide" in argv:
        return wide_main(budget, seed0)
    if "--edges" in argv:
        return edges_main(budget, seed0)
    if "--wait" in argv:
        return wait_main(budget, seed0)
    if "--patterns" in argv:
        return patterns_main(budget, seed0, team=len(ARGV) > 2 and ARGV[2] == "team")
    if len(ARGV) > 2 and ARGV[2] == "team":
        return team_main(budget, seed0)
    t_end = time.time() + budget
    n_done = 0
    k = 0
    only = os.environ.get("MM_STRESS_ONLY")              # one scenario by its seed (what a failure's message names)
    while time.time() < t_end:
        seed = seed0 * 100003 + k
        k += 1
        if only:
            if k > 1:
                break
            seed = int(only)
        rng = np.random.default_rng(seed)
        window = int(rng.choice([0, 1, 3, 10, 25, 60, 200, 1000, 10 ** 6]))
        regions = int(rng.choice([1, 2, 4, 8, 64]))
        party = bool(rng.integers(0, 4) == 0)
        modes = [mode_1v1(window=window, region_filter=regions > 1, party_filter=party)]
        if rng.integers(0, 3) == 0:
            modes.append(mode_team(2, 2, 300, (1, 1)))
        cfg = make_config(modes, capacity=1 << 19, timing=False)
        lo = int(rng.choice([0, 0, 1000, 2400]))
        hi = int(rng.choice([1499, 2600, 5000, 5000]))
        if hi <= lo:
            hi = lo + 600
        sizes = [scaled(rng.choice([50, 3000, 20000, 70000, 150000, 260000]))] + \
                [scaled(rng.choice([0, 100, 5000, 40000])) for _ in range(int(rng.integers(0, 4)))]
        tuning = draw_tuning(seed, [PAIR_KNOBS] + ([TEAM_KNOBS] if len(modes) > 1 else []))
        tag = "seed %d w=%d regions=%d party=%d modes=%d ratings=[%d,%d] sizes=%s tuning=%s" % (
            seed, window, regions, party, len(modes), lo, hi, sizes, tuning)
        if os.environ.get("MM_STRESS_VERBOSE"):
            print(tag, flush=True)                      # (a crash inside the library leaves no assertion message behind)
        with (Engine(cfg, tuning) if tuning else Engine(cfg)) as a, OracleEngine(cfg) as b:
            live = np.zeros(0, np.uint32)
            for j, n in enumerate(sizes):
                rating = rng.integers(lo, hi + 1, size=n).astype(np.int32)
                mode = rng.integers(0, len(modes), size=n) if len(modes) > 1 else np.zeros(n, np.int64)
                role = np.where(mode == 1, rng.integers(0, 2, size=n), 0)
                cons = cons_make(mode, rng.integers(0, regions, size=n), rng.integers(0, 3 if party else 1, size=n), role)
                sa, sb = a.enqueue(rating, cons), b.enqueue(rating, cons)
                assert np.array_equal(sa, sb), tag
                live = np.concatenate([live, sa])
                if live.size > 10 and rng.integers(0, 3) == 0:
                    cs = rng.choice(live, size=max(1, live.size // 50), replace=False)
                    a.cancel(cs)
                    b.cancel(cs)
                    live = np.setdiff1d(live, cs)
                for md in range(len(modes)):
                    ma, mb = a.tick(md), b.tick(md)
                    assert_same_tick(ma, mb, tag + " tick %d mode %d" % (j, md))
                    live = np.setdiff1d(live, ma.slots.ravel())
                assert_same_state(a, b, cfg, tag)
        n_done += 1
    print("gpu_stress%s: %d scenarios ok (seeds %d..%d)" % (" --fuzz-knobs" if FUZZ else "", n_done, seed0 * 100003, seed0 * 100003 + k - 1))


if __name__ == "__main__":
    main()
