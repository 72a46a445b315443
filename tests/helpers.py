"""Shared drivers: run a golden case or a random scenario against any ABI engine class."""
from __future__ import annotations

import json
import os
from fractions import Fraction

import numpy as np

from microservice_matchmaking_amd._abi import NO_SLOT, cons_make
from microservice_matchmaking_amd.config import make_config, mode_1v1

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "mode_r_cases.json")


def load_golden():
    with open(GOLDEN) as f:
        return json.load(f)


def players_to_arrays(players):
    p = np.asarray(players, dtype=np.int64).reshape(-1, 5)
    rating = p[:, 0].astype(np.int32)
    cons = cons_make(p[:, 4], p[:, 1], p[:, 2], p[:, 3])
    return rating, cons


def run_golden_case(engine_cls, case, capacity=64):
    cfg = make_config(case["modes"], capacity=capacity)
    eng = engine_cls(cfg)
    try:
        for step in case["steps"]:
            if step["op"] == "enqueue":
                r, c = players_to_arrays(step["players"])
                slots = eng.enqueue(r, c)
                if "expect_slots" in step:
                    assert slots.tolist() == step["expect_slots"], (case["name"], slots)
            elif step["op"] == "cancel":
                eng.cancel(np.asarray(step["slots"], dtype=np.uint32))
            elif step["op"] == "tick":
                m = eng.tick(step["mode"])
                ex = step["expect"]
                tag = "%s tick(mode %d)" % (case["name"], step["mode"])
                assert m.slots.tolist() == ex["matches"], (tag, m.slots.tolist())
                assert m.group.tolist() == ex["group"], tag
                assert m.pass_.tolist() == ex["pass"], tag
                assert np.allclose(m.score, np.asarray(ex["score"], np.float32), atol=1e-6), tag
                assert m.stats["pairs"] == ex["pairs"], (tag, m.stats["pairs"])
                assert m.stats["passes_max"] == ex["passes_max"], (tag, m.stats["passes_max"])
                assert m.stats["pool_after"] == ex["pool_after"], (tag, m.stats["pool_after"])
                assert m.stats["matches"] == len(ex["matches"]), tag
                assert eng.queue_depth(step["mode"]).tolist() == ex["depth"], (tag, eng.queue_depth(step["mode"]))
                for g, lb in ex["lobby"].items():
                    s, t = eng.lobby_state(step["mode"], int(g))
                    assert s.tolist() == lb["slots"], (tag, g, s)
                    assert t.tolist() == lb["teams"], (tag, g, t)
            else:
                raise ValueError(step["op"])
    finally:
        eng.close()


def assert_same_tick(a, b, tag="", score_tol=1e-6):
    """a, b: Matches.  Bit-exact assignments/order; scores within tolerance."""
    assert a.slots.shape == b.slots.shape, (tag, a.slots.shape, b.slots.shape)
    assert np.array_equal(a.slots, b.slots), (tag, "slots differ at row",
                                              int(np.argmax((a.slots != b.slots).any(axis=1))))
    assert np.array_equal(a.group, b.group), (tag, "group")
    assert np.array_equal(a.pass_, b.pass_), (tag, "pass")
    assert np.allclose(a.score, b.score, atol=score_tol, rtol=0), (tag, "score")
    for k in ("pool_before", "pool_after", "matches", "players_matched", "passes_max", "pairs", "scanned"):
        assert a.stats[k] == b.stats[k], (tag, k, a.stats[k], b.stats[k])


def f32_nearest(q: Fraction) -> np.float32:
    """The f32 nearest to the exact rational q, ties to even: a candidate and its two neighbours, judged exactly."""
    c = np.float32(float(q))
    best = None
    for x in (np.nextafter(c, np.float32(-np.inf)), c, np.nextafter(c, np.float32(np.inf))):
        d = abs(Fraction(float(x)) - q)
        if best is None or d < best[0] or (d == best[0] and int(np.float32(x).view(np.uint32)) & 1 == 0):
            best = (d, np.float32(x))
    return best[1]


def exact_scores(slots, mode, rating_of):
    """The score every emitted lobby must carry (include/mm_engine.h: |sum of team max - sum of team min| / team_size):
    team sums in emission (team) order from the enqueued ratings as Python ints, the difference exact, the quotient
    rounded once to the nearest f32.  slots: (n, teams * team_size); mode: dict or mm_mode_config; rating_of: slot -> int."""
    ts = int(mode["team_size"] if isinstance(mode, dict) else mode.team_size)
    out = np.empty(len(slots), np.float32)
    for i, row in enumerate(slots):
        sums = [sum(int(rating_of[int(s)]) for s in row[t:t + ts]) for t in range(0, len(row), ts)]
        out[i] = f32_nearest(Fraction(max(sums) - min(sums), ts))
    return out


def assert_exact_scores(m, mode, rating_of, tag=""):
    """Bit-exact scores of one tick's Matches against exact_scores (no tolerance)."""
    want = exact_scores(m.slots, mode, rating_of)
    got = np.asarray(m.score, np.float32)
    bad = np.flatnonzero(got.view(np.uint32) != want.view(np.uint32))
    assert bad.size == 0, (tag, "score", int(bad[0]), float(got[bad[0]]), float(want[bad[0]]), m.slots[bad[0]].tolist())


def assert_exact_scores_any(m, mode, rating_of, tag=""):
    """assert_exact_scores on every lobby of a tick of up to 20 000 lobbies; a longer list is checked whole by the
    same rule in numpy (team sums as int64, the quotient in double — exact or not a dyadic rational, so its rounding to
    f32 is the nearest f32 — compared to the bit) and by assert_exact_scores on 20 000 lobbies spread over it."""
    rows = np.arange(len(m))
    if len(m) > 20000:
        ts = int(mode.team_size)
        sums = np.asarray(rating_of)[m.slots].reshape(len(m), -1, ts).sum(axis=2)
        want = ((sums.max(axis=1) - sums.min(axis=1)).astype(np.float64) / ts).astype(np.float32)
        bad = np.flatnonzero(want.view(np.uint32) != np.asarray(m.score, np.float32).view(np.uint32))
        assert bad.size == 0, (tag, "score", int(bad[0]), float(m.score[bad[0]]), float(want[bad[0]]))
        rows = np.unique(np.linspace(0, len(m) - 1, 20000).astype(np.int64))
    sub = type(m)(m.slots[rows], m.score[rows], m.group[rows], m.pass_[rows], m.stats)
    assert_exact_scores(sub, mode, rating_of, tag)


def assert_same_state(ea, eb, cfg, tag=""):
    """Queue depth, queue ORDER (requeue ordering, worker.ex:239-248 -> requeue/worker.ex:51-54: the
    survivors of a tick in the order the broker would deliver them next) and the stored lobby."""
    for mode in range(cfg.n_modes):
        assert np.array_equal(ea.queue_depth(mode), eb.queue_depth(mode)), (tag, "depth", mode)
        for g in range(cfg.n_groups):
            qa, qb = ea.queue_slots(mode, g), eb.queue_slots(mode, g)
            assert np.array_equal(qa, qb), (tag, "queue order", mode, g,
                                            int(np.argmax(qa != qb)) if qa.shape == qb.shape else (qa.shape, qb.shape))
            sa, ta = ea.lobby_state(mode, g)
            sb, tb = eb.lobby_state(mode, g)
            assert np.array_equal(sa, sb) and np.array_equal(ta, tb), (tag, "lobby", mode, g, sa, sb)


def run_full_tile_one_pass(engine_cls, oracle_cls, tag):
    """More than 1024 lobbies in one tile and pass — the immediate emission of the pair walk's pass_apply
    (mm_pair.inc, `i >= PT_THREADS`: a thread defers one lobby, the tile's further ones are stored right away).
    One 1v1 mode, one region, the window as wide as the rating span: every player fits its neighbour, so the first
    pass pairs the whole queue.  One rating group of 20 000 players is the smallest chain that is tiled at all
    (kp_late takes the ones below 16 384): three tiles of 8192 positions, and a full tile emits 4096 lobbies in that
    pass.  The tile length is pinned to the largest (mm_tuning.pair_tile_fixed): left to itself the host walks a chain
    of 20 000 in ten tiles of 2048, which hold 1024 lobbies at most and never reach the branch (one of 4096 needs a
    chain of more than 40 x 2048 players).  Equality with the oracle, all 10 000 lobbies and a tick of at most two
    passes together say that one pass put more than 1024 lobbies into a tile."""
    n = 20000
    cfg = make_config([mode_1v1(window=1500, region_filter=True)], capacity=1 << 15)
    rating = np.random.default_rng(41).integers(0, 1400, size=n).astype(np.int32)      # the first rating group: 0 .. 1499
    cons = cons_make(np.zeros(n, np.int64), 0, 0, 0)
    with engine_cls(cfg, {"pair_tile_fixed": 1}) as e, oracle_cls(cfg) as o:
        assert np.array_equal(e.enqueue(rating, cons), o.enqueue(rating, cons))
        me, mo = e.tick(0), o.tick(0)
        assert_same_tick(me, mo, tag)
        assert_same_state(e, o, cfg, tag)
        assert len(me) == n // 2, (tag, len(me))
        assert me.stats["passes_max"] <= 2, (tag, me.stats["passes_max"])


def read_matches(e, first, count, mode=0):
    """mm_matches for the window [first, first + count) of the engine's last tick: (slots, score, group, pass)."""
    import ctypes as C
    L = e.lobby_size(mode)
    slots, score = np.empty((count, L), np.uint32), np.empty(count, np.float32)
    group, pass_ = np.empty(count, np.uint32), np.empty(count, np.uint32)
    e._check(e._fn("matches")(e._h, first, count, *(a.ctypes.data_as(C.c_void_p) for a in (slots, score, group, pass_))), "matches")
    return slots, score, group, pass_


def run_match_list_routes(engine_cls, oracle_cls, tag):
    """The routes a tick's match list takes to the host, end to end.
    One: run_full_tile_one_pass's pool — 20 000 all-fitting players of one rating group, 10 000 lobbies, more than either
    8192 threshold, behind a look at the chains — under the four combinations of results_early and results_tail (the
    tail kernel, or copy commands on the copy stream): every list is the oracle's, and the four are each other's to the
    bit, slots, score, pass and group.
    Two: a seven-group pool of 600 players that takes no look (no chain is long enough for the tiled rounds), so its list
    leaves packed: read whole, and again in windows of 1, 3 and 64 entries whose concatenation is the whole."""
    n = 20000
    cfg = make_config([mode_1v1(window=1500, region_filter=True)], capacity=1 << 15)
    rating = np.random.default_rng(41).integers(0, 1400, size=n).astype(np.int32)
    cons = cons_make(np.zeros(n, np.int64), 0, 0, 0)
    with oracle_cls(cfg) as o:
        o.enqueue(rating, cons)
        mo = o.tick(0)
    assert len(mo) == n // 2, (tag, len(mo))
    first = None
    for early in (1, 0):
        for tail in (1, 0):
            t = "%s early %d tail %d" % (tag, early, tail)
            with engine_cls(cfg, {"pair_tile_fixed": 1, "results_early": early, "results_tail": tail}) as e:
                e.enqueue(rating, cons)
                me = e.tick(0)
                assert e.path_stats()["host_looks"] >= 1, t
            assert_same_tick(me, mo, t)
            if first is None:
                first = me
            for a, b, what in ((me.slots, first.slots, "slots"), (me.score.view(np.uint32), first.score.view(np.uint32), "score"),
                               (me.pass_, first.pass_, "pass"), (me.group, first.group, "group")):
                assert np.array_equal(a, b), (t, what)
    cfg = make_config([mode_1v1(window=40, region_filter=True)], capacity=4096)
    rng = np.random.default_rng(43)
    rating = rng.integers(0, 5001, size=600).astype(np.int32)
    cons = cons_make(0, rng.integers(0, 2, size=600), 0, 0)
    with engine_cls(cfg) as e, oracle_cls(cfg) as o:
        assert np.array_equal(e.enqueue(rating, cons), o.enqueue(rating, cons))
        me, mo = e.tick(0), o.tick(0)
        assert_same_tick(me, mo, tag + " packed")
        assert e.path_stats()["host_looks"] == 0 and len(np.unique(me.group)) == 7 and 64 < len(me) <= 300, (tag, len(me))
        whole = read_matches(e, 0, len(me))
        for a, b in zip(whole, (me.slots, me.score, me.group, me.pass_)):
            assert np.array_equal(a.view(np.uint32), b.view(np.uint32)), (tag, "packed, whole")
        for w in (1, 3, 64):
            parts = [read_matches(e, at, min(w, len(me) - at)) for at in range(0, len(me), w)]
            for k in range(4):
                assert np.array_equal(np.concatenate([p[k] for p in parts]).view(np.uint32), whole[k].view(np.uint32)), (tag, "windows of", w, k)


def random_scenario(rng, cfg, ea, eb, n_rounds=4, batch=200, cancel_frac=0.05, n_regions=3,
                    rating_lo=0, rating_hi=5000, n_parties=2):
    """Drive two engines with the same random enqueue/cancel/tick script and compare."""
    live = []
    rating_of = {}                    # slot -> the rating it was enqueued with (slots are reused: the latest wins)
    for rnd in range(n_rounds):
        n = int(rng.integers(0, batch + 1))
        rating = rng.integers(rating_lo, rating_hi + 1, size=n).astype(np.int32)
        mode = rng.integers(0, cfg.n_modes, size=n)
        role = np.array([rng.integers(0, cfg.modes[int(m)].n_roles) for m in mode], dtype=np.uint32)
        region = rng.integers(0, n_regions, size=n)
        party = rng.integers(0, n_parties, size=n)
        cons = cons_make(mode, region, party, role)
        sa = ea.enqueue(rating, cons)
        sb = eb.enqueue(rating, cons)
        assert np.array_equal(sa, sb), "slots"
        live.extend(int(s) for s in sa if s != NO_SLOT)
        rating_of.update((int(s), int(r)) for s, r in zip(sa, rating) if s != NO_SLOT)
        if live and cancel_frac > 0:
            k = int(len(live) * cancel_frac)
            if k:
                idx = rng.choice(len(live), size=k, replace=False)
                cs = np.asarray([live[i] for i in idx], dtype=np.uint32)
                ea.cancel(cs)
                eb.cancel(cs)
                gone = set(cs.tolist())
                live = [s for s in live if s not in gone]
        for mode_i in range(cfg.n_modes):
            ma = ea.tick(mode_i)
            mb = eb.tick(mode_i)
            assert_same_tick(ma, mb, tag="round %d mode %d" % (rnd, mode_i))
            assert_exact_scores(ma, cfg.modes[mode_i], rating_of, "round %d mode %d" % (rnd, mode_i))
            assert_exact_scores(mb, cfg.modes[mode_i], rating_of, "round %d mode %d" % (rnd, mode_i))
            gone = set(ma.slots.ravel().tolist())
            live = [s for s in live if s not in gone]
        assert_same_state(ea, eb, cfg, tag="round %d" % rnd)


def run_wrapping_stream(engine_cls, oracle_cls, capacity=4096, ticks=120, per_tick=500, seed=17):
    """A stream that laps the slot ring many times while some players wait for the whole run
    (loners in thinly populated rating groups and regions): the handles of every batch, every
    tick and the final state must be those of the oracle, and no batch may be refused while
    the pool has free slots.  Returns (laps of the ring, batches that had to step over a slot)."""
    from microservice_matchmaking_amd.config import mode_1v1
    cfg = make_config([mode_1v1(window=25, region_filter=True)], capacity=capacity)
    rng = np.random.default_rng(seed)
    handed, stepped = 0, 0
    with engine_cls(cfg) as a, oracle_cls(cfg) as b:
        for t in range(ticks):
            n = int(rng.integers(per_tick // 2, per_tick + 1))
            # most of the traffic in one dense band; a few loners in the other rating groups (a loner
            # inside the band's own group would become an anchor nobody fits and hold the whole chain
            # up until a fitting player arrives: reference behaviour, MATCH_CHECK.md section 4)
            rating = np.where(rng.random(n) < 0.97, rng.integers(2000, 2100, size=n),
                              rng.choice([rng.integers(0, 2000), rng.integers(2500, 5001)], size=n)).astype(np.int32)
            cons = cons_make(0, rng.integers(0, 4, size=n), 0, 0)
            sa, sb = a.enqueue(rating, cons), b.enqueue(rating, cons)
            assert np.array_equal(sa, sb), ("handles differ at tick", t)
            handed += n
            stepped += int((np.diff(sa.astype(np.int64)) % capacity != 1).any())
            if t % 7 == 3:                                            # some of the waiting give up
                depth_before = int(a.queue_depth(0).sum())
                if depth_before:
                    cs = rng.choice(sa, size=min(5, n), replace=False)
                    a.cancel(cs)
                    b.cancel(cs)
            ma, mb = a.tick(0), b.tick(0)
            assert_same_tick(ma, mb, "wrapping stream tick %d" % t)
        assert_same_state(a, b, cfg, "wrapping stream")
    return handed / capacity, stepped


def run_starving_team_stream(engine_cls, oracle_cls, preload=200_000, ticks=40, per_tick=400, cancels=25, seed=11,
                             capacity=1 << 19):
    """cfg-5 where it ends up after a minute (reference lib/search/worker.ex:352-358 deliveries, :291-324 attempts):
    cfg-3's role weights give 10 % supports for 20 % of the seats, so half of the 5v5 arrivals can never be seated and
    the pool grows into chains of tens of thousands of players in which a tick seats a handful of lobbies — the team
    path (chains >= 4096 players) in its starving regime, every tick, with cancels trickling in.  Engine vs oracle,
    after every tick: lobbies, order, counters, queue order, stored lobby.  Returns the lobbies per tick."""
    from microservice_matchmaking_amd.config import mode_team
    from microservice_matchmaking_amd.synth import ROLE_WEIGHTS_5V5, make_pool
    cfg = make_config([mode_team(5, 2, 50, (1, 1, 1, 1, 1))], capacity=capacity)
    rng = np.random.default_rng(seed)
    per = []
    with engine_cls(cfg) as a, oracle_cls(cfg) as b:
        rating, cons = make_pool(preload, seed=seed, role_weights=ROLE_WEIGHTS_5V5)
        sa, sb = a.enqueue(rating, cons), b.enqueue(rating, cons)
        assert np.array_equal(sa, sb)
        waiting = set(sa.tolist())
        ma, mb = a.tick(0), b.tick(0)                      # the backlog a minute of the stream leaves behind
        assert_same_tick(ma, mb, "starving stream: preload")
        waiting -= set(ma.slots.ravel().tolist())
        depth = a.queue_depth(0)
        for t in range(ticks):
            rating, cons = make_pool(per_tick, seed=1000 * seed + t, role_weights=ROLE_WEIGHTS_5V5)
            sa, sb = a.enqueue(rating, cons), b.enqueue(rating, cons)
            assert np.array_equal(sa, sb), ("handles differ at tick", t)
            waiting |= set(sa.tolist())
            if cancels and t % 2 == 1:
                cs = rng.choice(np.fromiter(waiting, dtype=np.uint32), size=cancels, replace=False)
                a.cancel(cs)
                b.cancel(cs)
                waiting -= set(cs.tolist())
            ma, mb = a.tick(0), b.tick(0)
            assert_same_tick(ma, mb, "starving stream tick %d" % t)
            assert_same_state(a, b, cfg, "starving stream tick %d" % t)
            waiting -= set(ma.slots.ravel().tolist())
            per.append(len(ma))
    return per, depth


def run_anchor_moves_to_the_emptied_first_team(tuning, engine_cls, oracle_cls, bystanders=70, capacity=4096, score_tol=1e-6):
    """Hand-built, three ticks of a 2v2 mode in one rating group (engine vs oracle after every tick, and the exact layouts
    of the stored lobby).  Tick 1 leaves the stored lobby team 1: [A, C], team 2: [B]; A and C cancel.  Tick 2's head meets
    the stale lobby (anchor A: rejected, it sits out the pass), the filter leaves team 2: [B] with B the anchor.  D fits B
    and is seated in the empty team 1, which makes D the anchor mid-fill: E (fits D, not B) is taken, F (fits B, not D) is
    not, and the lobby stays open.  Tick 3: G arrives at the tail, the head of the queue fills the stored lobby, and it is
    emitted on the spot.  `bystanders` players nobody near 500 fits keep the chain long enough for the team path (the open
    lobby blocks them until tick 3).  Returns mm_path_stats after each tick and tick 3's lobbies."""
    from microservice_matchmaking_amd.config import mode_team
    cfg = make_config([mode_team(2, 2, 100, (2,))], capacity=capacity)
    others = 1000 + 5 * (np.arange(bystanders) % 70)
    stats = []
    with engine_cls(cfg, tuning) as a, oracle_cls(cfg) as b:
        def both(fn):
            return fn(a), fn(b)

        def tick(tag):
            ma, mb = both(lambda e: e.tick(0))
            assert_same_tick(ma, mb, tag, score_tol)
            assert_same_state(a, b, cfg, tag)
            stats.append(a.path_stats())
            return ma
        r1 = np.concatenate([[500, 510, 520], others]).astype(np.int32)
        sa, sb = both(lambda e: e.enqueue(r1, cons_make(np.zeros(r1.size))))
        assert np.array_equal(sa, sb)
        tick("tick 1")
        slots, teams = a.lobby_state(0, 0)
        assert slots.tolist() == [int(sa[0]), int(sa[2]), int(sa[1])] and teams.tolist() == [0, 0, 1]
        both(lambda e: e.cancel(np.asarray([sa[0], sa[2]], np.uint32)))
        r2 = np.asarray([600, 690, 450], np.int32)       # D, E, F
        s2, _ = both(lambda e: e.enqueue(r2, cons_make(np.zeros(3))))
        tick("tick 2")
        slots, teams = a.lobby_state(0, 0)
        assert slots.tolist() == [int(s2[0]), int(sa[1]), int(s2[1])] and teams.tolist() == [0, 1, 1]
        s3, _ = both(lambda e: e.enqueue(np.asarray([650], np.int32), cons_make(np.zeros(1))))
        ma = tick("tick 3")
        assert len(ma) >= 1 and ma.slots[0].tolist() == [int(s2[0]), int(s3[0]), int(sa[1]), int(s2[1])]
    return stats, ma


# run_anchor_moves_to_the_emptied_first_team at the product's geometry (4100 bystanders, capacity 8192), under the shim
# and on the device: tuning -> {tick: mm_path_stats counters}, i.e. which kernel runs which pass: tick 2 (the anchor moves)
# always in the pass kernels; tick 3's fill from the head of the queue in kt_late where it is on, and then 678 lobbies.
ANCHOR_MOVES_PRODUCT = [
    ({}, {2: {"crit_team_f_passes": 2, "crit_team_late_passes": 0},
          3: {"team_late_launches": 1, "crit_team_f_passes": 1, "crit_team_late_passes": 2, "crit_team_late_lobbies": 678}}),
    ({"team_f2": 0}, {2: {"crit_team_fc_passes": 2}, 3: {"crit_team_fc_passes": 1, "crit_team_late_passes": 2}}),
    ({"team_late": 0, "team_split": 0}, {2: {"crit_team_f_passes": 2}, 3: {"crit_team_f_passes": 3, "crit_team_f_lobbies": 678}}),
    # ticks 1 and 3 begin in kt_late with the long chain
    ({"team_late0": 10000000}, {1: {"team_late_launches": 1, "crit_team_late_passes": 2, "crit_team_f_passes": 0},
                                3: {"team_late_launches": 1, "crit_team_f_passes": 1, "crit_team_late_passes": 2,
                                    "crit_team_late_lobbies": 678}}),
]
ANCHOR_MOVES_PRODUCT_IDS = ["default", "f2=0", "late=0-split=0", "late0=1e7"]


def assert_path_counts(stats, want):
    """want: {tick: {mm_path_stats counter: value}}; stats: path_stats() after each tick, tick 1 first."""
    for tick, counts in want.items():
        got = {k: stats[tick - 1][k] for k in counts}
        assert got == counts, ("tick %d" % tick, got, counts)
