"""Shared drivers for mm_move_out / mm_moved_rows / mm_enqueue_stamped (include/mm_wait.h): tests/test_carry.py runs them
on the CPU shim, tests/test_gpu_carry.py on the GPU.

The main witness is the equivalence the header states: on one engine, mm_move_out, then mm_expired + mm_moved_rows, then
mm_enqueue_stamped of the same rows with their groups is mm_move word for word.  So two engines of one class run one
script, A through mm_move and B through the two-call route, and are compared after every step; A is additionally held
against the unchanged oracle and the test's own slot -> (rating, constraint word, stamp) table through move_scenarios.Duo,
which ties B to Mode R.  A stamped enqueue on its own is an enqueue to the oracle, and to the test's table one that brings
its own stamps."""
from __future__ import annotations

import os

import numpy as np

from helpers import assert_same_state, assert_same_tick
from microservice_matchmaking_amd._abi import NO_SLOT, MMError, cons_make
from microservice_matchmaking_amd.config import make_config, mode_1v1, mode_team
from microservice_matchmaking_amd.sharding import rating_groups
from move_scenarios import (MM_ERR_FULL, MM_ERR_RANGE, ROLE_MASK, Duo, bucket_lengths, four_mode_config, pool,
                            rewrite)
from wait_scenarios import U32, assert_wait_stats, random_batch, tick_both

ONE_GROUP = [(0, 1_000_000, "all")]
# expected load per (mode, group) chain for the rank tests: under ChainSharding's rule these put chain (2, g) and chain
# (3, g) on different ranks for some g and on the same rank for others (asserted where they are used)


def carry_route(e, from_mode, to_mode, max_age, cons_clear=0):
    """mm_move by the two-call route on ONE engine.  Returns mm_move's four columns and sets e.last_move like it."""
    old, group, age, rating, cons, stamp = e.move_out(from_mode, to_mode, max_age, cons_clear)
    new = e.enqueue_stamped(rating, cons, stamp, group.astype(np.uint8)) if old.size else np.zeros(0, np.uint32)
    e.last_move = {"selected": int(old.size), "refused": int((new == NO_SLOT).sum())}
    return old, group, age, new


def carry_engine(engine_cls):
    """engine_cls with `move` going through the two-call route: every script written for mm_move runs on it unchanged."""
    return type("Carry" + engine_cls.__name__, (engine_cls,), {"move": carry_route})


def stamps_of(e):
    """stamp[capacity] as the engine holds it: the tail of a version-2 snapshot (include/mm_engine.h)."""
    return np.frombuffer(e.snapshot()[-4 * int(e.cfg.capacity):], dtype=np.uint32).copy()


def assert_twins(a, c, cfg, tag=""):
    """Two engines of one class in the same state: queues in order, stored lobbies, wait statistics of every mode."""
    assert_same_state(a, c, cfg, tag)
    if a.clock()[1]:
        assert a.clock() == c.clock(), (tag, a.clock(), c.clock())
        for md in range(cfg.n_modes):
            for g, (x, y) in enumerate(zip(a.wait_stats(md), c.wait_stats(md))):
                assert (x["waiting"], x["oldest_age"], x["age_sum"]) == (y["waiting"], y["oldest_age"], y["age_sum"]) and \
                    np.array_equal(x["hist"], y["hist"]), (tag, "wait_stats", md, g, x, y)


def twin_script(engine_cls, oracle_cls, seed=5, rounds=8, first=1500, batch=400, clock0=1000, step_max=60, age_max=120,
                restart_at=(), cancel_frac=0.03, rule=(2, 3, ROLE_MASK), capacity=8192):
    """move_scenarios.move_script's shape on two engines of one class: A moves through mm_move (and is held against the
    oracle and the test's table, Duo), B through mm_move_out + mm_moved_rows + mm_enqueue_stamped.  After every step:
    the lists, the new-slot column against out_slot, every queue, every stored lobby, the wait statistics of every mode;
    after every tick the lobbies, the counters and every word of mm_matches_wait.  Returns (moved, refused, lobbies)."""
    cfg = four_mode_config(capacity)
    rng = np.random.default_rng(seed)
    d = Duo(engine_cls, oracle_cls, cfg)
    c = engine_cls(cfg)
    now, moved, refused, lobbies = clock0, 0, 0, [0] * cfg.n_modes
    try:
        for rnd in range(rounds):
            tag = "round %d" % rnd
            now += int(rng.integers(1, step_max + 1))
            d.clock(now)
            c.clock_set(now)
            rating, cons = random_batch(rng, cfg, first if rnd == 0 else int(rng.integers(0, batch + 1)))
            assert np.array_equal(d.enqueue(rating, cons), c.enqueue(rating, cons)), (tag, "slots")
            assert_twins(d.a, c, cfg, tag + " enqueue")
            live = d.tr.live_slots()
            k = int(live.size * cancel_frac)
            if k:
                cs = rng.choice(live, size=k, replace=False)
                mode_of = np.full(int(cfg.capacity), -1, np.int64)
                for md in range(cfg.n_modes):
                    for g in range(cfg.n_groups):
                        mode_of[d.a.lobby_state(md, g)[0]] = md
                        mode_of[d.a.queue_slots(md, g)] = md
                for e in (d.a, d.b, c):
                    e.cancel(cs)
                for md in range(cfg.n_modes):
                    d.tr.marked(md, cs[mode_of[cs] == md])
                assert_twins(d.a, c, cfg, tag + " cancel")
            max_age = int(rng.integers(0, age_max + 1))
            ga = d.move(rule[0], rule[1], max_age, rule[2], tag)
            gc = carry_route(c, rule[0], rule[1], max_age, rule[2])
            for name, x, y in zip(("slots", "group", "age", "new slot"), ga, gc):
                assert np.array_equal(x, y), (tag, "move", name, x[:8], y[:8], x.size, y.size)
            assert d.a.last_move == c.last_move, (tag, d.a.last_move, c.last_move)
            moved += int(ga[0].size)
            refused += int((ga[3] == NO_SLOT).sum())
            assert_twins(d.a, c, cfg, tag + " move")
            for md in range(cfg.n_modes):
                if rng.random() < 0.4:
                    max_age = int(rng.integers(age_max // 2, 2 * age_max))
                    ga, gc = d.expire(md, max_age, tag), c.expire(md, max_age)
                    for x, y in zip(ga, gc):
                        assert np.array_equal(x, y), (tag, "expire", md)
                    assert_twins(d.a, c, cfg, tag + " expire")
            if rnd in restart_at:
                for who in ("a", "c"):
                    e = d.a if who == "a" else c
                    blob, clk = e.snapshot(), e.clock()
                    e.close()
                    e = engine_cls(cfg)
                    e.restore(blob)
                    assert e.clock() == clk
                    if who == "a":
                        d.a = e
                    else:
                        c = e
                assert_twins(d.a, c, cfg, tag + " restart")
                assert_same_state(d.a, d.b, cfg, tag + " restart")
            for md in range(cfg.n_modes):
                ma = tick_both(d.a, d.b, d.tr, md, "%s mode %d" % (tag, md))
                mc = c.tick(md)
                assert_same_tick(ma, mc, "%s mode %d twins" % (tag, md))
                assert np.array_equal(d.a.matches_wait(), c.matches_wait()), (tag, "matches_wait", md)
                lobbies[md] += len(ma)
                assert_twins(d.a, c, cfg, "%s tick %d" % (tag, md))
            assert_same_state(d.a, d.b, cfg, tag)
            for md in range(cfg.n_modes):
                assert_wait_stats(c, d.tr, md, tag + " B against the table")
    finally:
        d.__exit__()
        c.close()
    return moved, refused, lobbies


# ---- the two halves against the oracle and the test's table ---------------------------------------------------------------

def move_out_both(d, from_mode, to_mode, max_age, cons_clear=0, tag=""):
    """A moves out; the list is what numpy says and the rows are the table's (rating, rewritten word, stamp) of the listed
    slots; B cancels them.  Returns A's six columns."""
    want = d.tr.expected_expiry(d.a, from_mode, max_age)
    got = d.a.move_out(from_mode, to_mode, max_age, cons_clear)
    for name, w, x in zip(("slots", "group", "age"), want, got):
        assert np.array_equal(w, x), (tag, "moved out", name, from_mode, to_mode, max_age, w[:8], x[:8], w.size, x.size)
    old, group, age, rating, cons, stamp = got
    assert np.array_equal(rating, d.tr.rating[old]), (tag, "rating")
    assert np.array_equal(cons, rewrite(d.tr.cons[old], to_mode, cons_clear)), (tag, "cons", cons[:8])
    assert np.array_equal(stamp, d.tr.stamp[old]), (tag, "stamp", stamp[:8], d.tr.stamp[old][:8])
    assert np.array_equal(stamp, ((d.tr.now - age.astype(np.int64)) % U32).astype(np.uint32)), (tag, "stamp = clock - age")
    assert d.a._fn("moved")(d.a._h, 0, 1, None) == MM_ERR_RANGE and d.a._fn("moved")(d.a._h, 0, 0, None) == 0
    d.b.cancel(old)
    d.tr.marked(from_mode, old)
    return got


def stamped_both(d, rating, cons, stamp, group=None, tag=""):
    """A enqueues with stamps, B enqueues the same rows: the same slots; the table takes the supplied stamps."""
    stamp = np.asarray(stamp, np.uint32)
    sa, sb = d.a.enqueue_stamped(rating, cons, stamp, group), d.b.enqueue(rating, cons, group)
    assert np.array_equal(sa, sb), (tag, "slots", sa[:8], sb[:8], int((sa != sb).sum()))
    ok = sa != NO_SLOT
    d.tr.enqueued_rows(sa, rating, cons)
    d.tr.stamp[sa[ok]] = stamp[ok]
    assert d.a.last_enqueue_stats["accepted"] == int(ok.sum()) and d.a.last_enqueue_stats["rejected"] == int((~ok).sum())
    return sa


def check_stamped(d, modes, slots, stamp, tag=""):
    """What the issue asks of every stamped enqueue: mm_wait_stats is numpy's, and an mm_expire at a threshold between two
    supplied stamps selects, of the batch, exactly the older rows."""
    for md in modes:
        d.stats(md, tag)
    ok = slots != NO_SLOT
    age = ((d.tr.now - np.asarray(stamp, np.int64)) % U32)[ok]
    assert np.unique(age).size >= 2, (tag, "the batch needs two different ages")
    thr = int(np.median(np.unique(age)[:-1]))               # >= the smallest age, < the largest: both sides are non-empty
    older = set(slots[ok][age > thr].tolist())
    got = set()
    for md in modes:
        got |= set(d.expire(md, thr, tag)[0].tolist())
    assert older and older <= got and not (set(slots[ok][age <= thr].tolist()) & got), (tag, len(older), len(got))
    return thr


def random_stamps(rng, now, n, age_max=5000):
    return ((now - rng.integers(0, age_max + 1, size=n)) % U32).astype(np.uint32)


def rows_cases(engine_cls, oracle_cls, capacity=8192):
    """mm_moved_rows against the table, case by case; every case goes on through mm_enqueue_stamped on the same engine,
    so the ticks that follow hold the carried stamps against the table as well."""
    done = []
    # a stored lobby's anchor and a queue's head, 1v1 and 5v5
    for src, dst, roles, clear in ((0, 1, 1, 0), (2, 3, 5, ROLE_MASK)):
        with Duo(engine_cls, oracle_cls, four_mode_config(capacity)) as d:
            d.clock(1000)
            d.enqueue(*pool(700, 21, src, roles))
            d.tick(src, "old wave")
            seated = np.concatenate([d.a.lobby_state(src, g)[0] for g in range(7)])
            heads = [int(q[0]) for q in (d.a.queue_slots(src, g) for g in range(7)) if q.size]
            assert seated.size > 0 and heads
            d.clock(1500)
            d.enqueue(*pool(700, 22, src, roles))
            old, group, age, rating, cons, stamp = move_out_both(d, src, dst, 499, clear, "anchor and head")
            assert set(seated.tolist()) <= set(old.tolist()) and set(heads) <= set(old.tolist()) and (age == 500).all()
            new = stamped_both(d, rating, cons, stamp, group.astype(np.uint8), "anchor and head")
            assert (new != NO_SLOT).all()
            d.tick_all("anchor and head")
            done.append(("anchor", src, int(old.size)))
    with Duo(engine_cls, oracle_cls, four_mode_config(capacity)) as d:
        # a player from before the first mm_clock_set
        d.enqueue(*pool(901, 51, 2, 5))
        d.tick(2)
        d.clock(4000)
        d.clock(4100)
        d.enqueue(*pool(300, 52, 2, 5))
        got = move_out_both(d, 2, 3, 99, ROLE_MASK, "before the clock")
        assert got[0].size > 0 and (got[2] == 100).all() and (got[5] == 4000).all()
        stamped_both(d, got[3], got[4], got[5], got[1].astype(np.uint8))
        d.tick_all("before the clock")
        done.append(("before the clock", int(got[0].size)))
    with Duo(engine_cls, oracle_cls, four_mode_config(capacity)) as d:
        # the clock crossing 2^32
        d.clock(0xFFFFFF00)
        d.enqueue(*pool(900, 41, 2, 5))
        d.tick(2)
        d.clock(0xFFFFFFF0)
        d.enqueue(*pool(400, 42, 2, 5))
        d.clock(0x00000010)
        got = move_out_both(d, 2, 3, 0x20, ROLE_MASK, "across the wrap")
        assert got[0].size > 0 and (got[2] == 0x110).all() and (got[5] == 0xFFFFFF00).all()
        stamped_both(d, got[3], got[4], got[5], got[1].astype(np.uint8))
        d.tick_all("across the wrap")
        d.clock(0x00000020)
        assert (d.expire(3, 0x11F, "the carried stamp is from before the wrap")[2] == 0x120).all()
        d.tick_all("across the wrap, end")
        done.append(("wrap", int(got[0].size)))
    with Duo(engine_cls, oracle_cls, four_mode_config(capacity)) as d:
        # to_mode a mode this engine does not have; nothing selected; everything selected; twice in a row
        d.clock(100)
        d.enqueue(*pool(900, 12, 2, 5))
        d.enqueue(*pool(400, 13, 0))
        d.tick_all("first tick")
        d.clock(101)
        depth = [d.a.queue_depth(md).tolist() for md in range(4)]
        none = move_out_both(d, 2, 3, 1, ROLE_MASK, "age == max_age is not older")
        assert all(x.size == 0 for x in none)
        assert d.a._fn("moved_rows")(d.a._h, 0, 0, None, None, None) == 0
        assert d.a._fn("moved_rows")(d.a._h, 0, 1, None, None, None) == MM_ERR_RANGE
        left = d.waiting(2)
        got = move_out_both(d, 2, 9, 0, ROLE_MASK, "to a mode of another engine")
        assert got[0].size == left > 0 and ((got[4] & 0xF) == 9).all() and (np.diff(got[1].astype(np.int64)) >= 0).all()
        assert [d.a.queue_depth(md).tolist() for md in range(4)] == depth     # marked, not dropped: no queue has changed
        assert d.waiting(2) == 0
        assert all(x.size == 0 for x in move_out_both(d, 2, 9, 0, ROLE_MASK, "twice in a row"))
        nxt = d.enqueue(*pool(3, 4, 0))                         # (Duo.enqueue: the oracle's slots) no slot was taken
        assert (nxt != NO_SLOT).all()
        d.clock(102)
        left0 = d.waiting(0)
        got0 = move_out_both(d, 0, 1, 0, 0, "another pair of modes right behind it")
        assert got0[0].size == left0 > 0
        stamped_both(d, got0[3], got0[4], got0[5], got0[1].astype(np.uint8))
        d.tick_all("after")
        done.append(("foreign mode", int(got[0].size)))
    return done


# ---- mm_enqueue_stamped on its own ------------------------------------------------------------------------------------------

def stamped_plain(engine_cls, oracle_cls, behind, n=1200, capacity=8192):
    """Stamps of mixed ages into an empty pool, or (behind) behind queues and stored lobbies."""
    cfg = four_mode_config(capacity)
    rng = np.random.default_rng(61)
    with Duo(engine_cls, oracle_cls, cfg) as d:
        d.clock(50_000)
        if behind:
            d.enqueue(*random_batch(rng, cfg, 1500))
            d.tick_all("the pool holds queues and stored lobbies")
            assert sum(d.a.lobby_state(md, g)[0].size for md in range(4) for g in range(7)) > 0
            d.clock(50_100)
        tails = {(md, g): d.a.queue_slots(md, g) for md in range(4) for g in range(7)}
        rating, cons = random_batch(rng, cfg, n)
        stamp = random_stamps(rng, d.tr.now, n)
        s = stamped_both(d, rating, cons, stamp, tag="plain")
        assert (s != NO_SLOT).all()
        grp = rating_groups(cfg, rating)
        for (md, g), t in tails.items():                       # behind whoever was queued, in batch order
            q = d.a.queue_slots(md, g)
            assert np.array_equal(q[:t.size], t) and np.array_equal(q[t.size:], s[((cons & 0xF) == md) & (grp == g)])
        assert np.array_equal(stamps_of(d.a)[s], stamp)
        check_stamped(d, range(4), s, stamp, "plain")
        d.tick_all("after")
        d.clock(d.tr.now + 7)
        d.tick_all("and the ages go on")


def stamped_ring(engine_cls, oracle_cls, in_the_way, capacity=1024):
    """move_scenarios' ring cases for a stamped batch: next_slot 124 slots before the end of the ring, 300 rows.
    in_the_way False: the plain range, wrapped (the last 124 slots, then 0..175).  True: waiting players hold the slots from
    0 on, the host hands the device a slot list (the last 124, then the 176 behind the waiting players) and every stamp
    must follow its row to the slot it got."""
    cfg = make_config([mode_1v1(window=0), mode_1v1(window=5000)], capacity=capacity)
    held = capacity - 424                                      # 600 of 1024
    assert held % 2 == 0 and held <= 250_000
    strict = (np.arange(held if in_the_way else 300) * 20 + np.arange(held if in_the_way else 300) % 7).astype(np.int32)
    assert np.unique(strict).size == strict.size              # all different: nobody matches at window 0
    loose = pool(300 if in_the_way else held, 41, 1, lo=0, hi=1499)
    rng = np.random.default_rng(62)
    with Duo(engine_cls, oracle_cls, cfg) as d:
        d.clock(10_000)
        if in_the_way:
            d.enqueue(strict, cons_make(np.zeros(strict.size)))
            d.enqueue(*loose)
        else:
            d.enqueue(*loose)
            d.enqueue(strict, cons_make(np.zeros(strict.size)))
        assert len(d.tick(1, "the loose mode empties")) == loose[0].size // 2
        d.clock(10_030)
        rating = (np.arange(300) * 20 + 11).astype(np.int32)
        stamp = random_stamps(rng, d.tr.now, 300, 9000)
        s = stamped_both(d, rating, cons_make(np.zeros(300)), stamp, tag="ring")
        want = list(range(capacity - 124, capacity)) + (list(range(held, held + 176)) if in_the_way else list(range(0, 176)))
        assert s.tolist() == want
        assert np.array_equal(stamps_of(d.a)[s], stamp)
        check_stamped(d, [0], s, stamp, "ring")
        d.enqueue(*pool(40, 42, 1))
        d.tick_all("after")


def stamped_refused(engine_cls, oracle_cls, n=1200, capacity=8192):
    """A batch with rows the mode cannot seat (roles >= 1 into the one-role 5v5): NO_SLOT, their ring positions used up, no
    stamp written for them, and the plain enqueue that follows gets the slots it gets on a twin that enqueued unstamped."""
    cfg = four_mode_config(capacity)
    rng = np.random.default_rng(63)
    with Duo(engine_cls, oracle_cls, cfg) as d, engine_cls(cfg) as twin:
        d.clock(777)
        twin.clock_set(777)
        d.clock(20_000)
        twin.clock_set(20_000)
        rating, cons = pool(n, 311, 3, 5)
        stamp = random_stamps(rng, d.tr.now, n)
        before = stamps_of(d.a)
        assert (before == 777).all()
        s = stamped_both(d, rating, cons, stamp, tag="refused")
        role = (cons >> 16) & 0xF
        assert np.array_equal(s == NO_SLOT, role >= 1) and 0 < int((s == NO_SLOT).sum()) < n
        after = stamps_of(d.a)
        ok = s != NO_SLOT
        assert np.array_equal(after[s[ok]], stamp[ok])
        rest = np.ones(capacity, bool)
        rest[s[ok]] = False
        assert (after[rest] == 777).all()                       # the ring positions of the refused rows among them
        assert np.array_equal(twin.enqueue(rating, cons), s)
        nxt = pool(300, 313, 3, 1)
        assert np.array_equal(d.enqueue(*nxt), twin.enqueue(*nxt))
        check_stamped(d, [3], s, stamp, "refused")
        d.tick_all("after")
        return int((s == NO_SLOT).sum())


def stamped_edges(engine_cls, oracle_cls, sizes=None, capacity=8192):
    """Batch sizes BK_PER_WAVE - 1 / BK_PER_WAVE / + 1 and BK_CHUNK - 1 / BK_CHUNK / + 1 (lengths from the source), every one
    through the slot list: two players who never match hold slots 0 and 1, refused rows use the ring up to 500 positions
    before its end, so the batch wraps onto the held slots and steps over them."""
    w, c = bucket_lengths()
    sizes = sizes or [w - 1, w, w + 1, c - 1, c, c + 1]
    cfg = four_mode_config(capacity)
    rng = np.random.default_rng(64)
    for n in sizes:
        assert 500 < n < capacity - 502
        with Duo(engine_cls, oracle_cls, cfg) as d:
            d.clock(30_000)
            d.enqueue(np.asarray([100, 3000], np.int32), cons_make([0, 0]))
            filler = pool(capacity - 502, 65, 3, 5)
            filler = (filler[0], filler[1] | np.uint32(1 << 16))        # role >= 1: the one-role mode refuses every row
            assert (d.enqueue(*filler) == NO_SLOT).all()
            d.clock(30_500)
            rating, cons = random_batch(rng, cfg, n)
            stamp = random_stamps(rng, d.tr.now, n)
            s = stamped_both(d, rating, cons, stamp, tag="edge %d" % n)
            assert s.tolist() == list(range(capacity - 500, capacity)) + list(range(2, 2 + n - 500))
            assert np.array_equal(stamps_of(d.a)[s], stamp)
            check_stamped(d, range(4), s, stamp, "edge %d" % n)
            d.tick_all("edge %d" % n)
    return sizes


def lobby_requeue(engine_cls, oracle_cls, capacity=8192):
    """A ready check that failed: one player of a lobby declines, the others come back with stamp = clock at the tick -
    their mm_matches_wait word, and their ages go on from where they were."""
    cfg = four_mode_config(capacity)
    with Duo(engine_cls, oracle_cls, cfg) as d:
        d.clock(1000)
        d.enqueue(*pool(300, 71, 3, 1))
        d.clock(1300)
        d.enqueue(*pool(300, 72, 3, 1))
        d.clock(1450)
        rating_of, cons_of = d.tr.rating.copy(), d.tr.cons.copy()
        m = d.tick(3, "the lobbies")
        wait = d.a.matches_wait()
        assert len(m) > 3 and set(np.unique(wait).tolist()) <= {150, 450} and np.unique(wait[1][1:]).size >= 1
        tick_clock = d.tr.now
        d.clock(1500)
        back = m.slots[1][1:].astype(np.int64)                   # lobby 1's players but the one who declined
        stamp = ((tick_clock - wait[1][1:].astype(np.int64)) % U32).astype(np.uint32)
        s = stamped_both(d, rating_of[back], cons_of[back], stamp, tag="requeue")
        assert (s != NO_SLOT).all()
        assert np.array_equal(d.tr.ages(s), wait[1][1:] + 50)
        d.stats(3, "requeue")
        assert max(x["oldest_age"] for x in d.a.wait_stats(3)) >= int(wait[1][1:].max()) + 50
        d.enqueue(*pool(40, 73, 3, 1))
        d.tick_all("the returned players are seated with their true wait")


def full_pool(engine_cls, oracle_cls, capacity=2048):
    """MM_ERR_FULL from mm_enqueue_stamped leaves everything as it was; mm_move_out needs no free slot at all."""
    cfg = four_mode_config(capacity)
    rng = np.random.default_rng(66)
    with Duo(engine_cls, oracle_cls, cfg) as d:
        d.clock(5)
        n = capacity // 2 + 100
        d.enqueue(*pool(n, 321, 2, 5, lo=0, hi=1499))
        d.clock(50)
        before = stamps_of(d.a)
        rating, cons = pool(n, 322, 3, 1)
        with_err = None
        try:
            d.a.enqueue_stamped(rating, cons, random_stamps(rng, 50, n, 40))
        except MMError as ex:
            with_err = ex.status
        assert with_err == MM_ERR_FULL, with_err
        assert_same_state(d.a, d.b, cfg, "after MM_ERR_FULL")
        assert np.array_equal(stamps_of(d.a), before)
        for md in range(4):
            d.stats(md, "after MM_ERR_FULL")
        assert d.enqueue(*pool(1, 323, 0)).tolist() == [n]        # next_slot is where it was
        got = move_out_both(d, 2, 3, 0, ROLE_MASK, "out of a pool too full for mm_move")
        assert got[0].size == n and (got[2] == 45).all()
        d.tick_all("the old slots are free again")
        s = stamped_both(d, got[3], got[4], got[5], got[1].astype(np.uint8), "and now there is room")
        assert (s != NO_SLOT).all()
        check_stamped(d, [3], np.concatenate([s, d.enqueue(*pool(10, 324, 3, 1))]),
                      np.concatenate([got[5], np.full(10, 50, np.uint32)]), "full")
        d.tick_all("end")


# ---- ranks -------------------------------------------------------------------------------------------------------------------

RANK_WEIGHTS = {2: np.array([[9, 1, 1, 1, 1, 1, 1], [1, 1, 1, 1, 1, 1, 1], [5, 3, 3, 3, 3, 3, 4], [4, 2, 2, 2, 2, 2, 3]], float),
                4: np.array([[8, 6, 5, 3, 3, 1, 1], [1, 2, 8, 6, 9, 5, 6], [9, 7, 6, 5, 6, 9, 3], [8, 7, 1, 4, 8, 5, 1]], float)}


def rank_engine(engine):
    if engine == "hip":
        from microservice_matchmaking_amd import Engine
        return Engine
    from emu_engine import EmuEngineSmall
    return EmuEngineSmall


def rank_script(sh, seed=11, rounds=6, first=1500, batch=400, rule=(2, 3, ROLE_MASK)):
    """The move script with global ids on one rank's share (or, world_size 1, on the whole pool through mm_move): every rank
    sees the same batches and the same cancels by global index.  Returns what the ranks' results are compared on."""
    import hashlib
    cfg = sh.cfg
    rng = np.random.default_rng(seed)
    hashers = {(m, g): hashlib.blake2b(digest_size=16) for m in range(cfg.n_modes) for g in range(cfg.n_groups)}
    waits = [[] for _ in range(cfg.n_modes)]
    selected = refused = taken = expired = 0
    now, first_id = 1000, 0
    for rnd in range(rounds):
        now += int(rng.integers(1, 61))
        sh.engine.clock_set(now)
        rating, cons = random_batch(rng, cfg, first if rnd == 0 else int(rng.integers(0, batch + 1)))
        idx, slots = sh.enqueue(rating, cons, first_global_index=first_id)
        gone = rng.random(rating.size) < 0.03                   # by global index: the same players on every rank
        sh.engine.cancel(slots[gone[idx] & (slots != NO_SLOT)])
        first_id += rating.size
        got = sh.move(rule[0], rule[1], int(rng.integers(0, 121)), rule[2])
        lm = sh.engine.last_move if sh.world_size == 1 else sh.last_move
        selected += int(got[0].size)
        refused += int(lm["refused"])
        taken += int(lm.get("taken", lm["selected"] - lm["refused"]))
        if rnd % 2:
            expired += int(sh.engine.expire(rule[1], int(rng.integers(100, 241)))[0].size)
        for md in range(cfg.n_modes):
            m = sh.tick(md)
            if len(m):
                ids = sh.global_ids(m)
                assert (ids >= 0).all()
                waits[md].append(sh.engine.matches_wait().ravel())
                for g in np.unique(m.group):
                    hashers[(md, int(g))].update(np.ascontiguousarray(ids[m.group == g], dtype="<i8").tobytes())
    owner = sh.sharding.chain_owner
    return {"digests": {k: h.hexdigest() for k, h in hashers.items() if owner[k] == sh.rank},
            "selected": selected, "refused": refused, "taken": taken, "expired": expired,
            "waits": [np.sort(np.concatenate(w)) if w else np.zeros(0, np.uint32) for w in waits]}


def _init(rank, world, port):
    import torch.distributed as dist
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    return dist


def script_worker(rank, world, port, engine, out_q, capacity=8192):
    from microservice_matchmaking_amd.sharding import ShardedSearch
    dist = _init(rank, world, port)
    with ShardedSearch(four_mode_config(capacity), rank_engine(engine), rank, world, RANK_WEIGHTS[world]) as sh:
        res = rank_script(sh)
        gathered = [None] * world
        dist.all_gather_object(gathered, res)
        if rank == 0:
            out_q.put((gathered, sh.sharding.chain_owner.tolist()))
    dist.barrier()
    dist.destroy_process_group()


STREAM = dict(qps=20_000, seconds=0.6, tick_ms=10.0, seed=5)
AFTER_MS = 50


def stream_cfg():
    return make_config([mode_team(5, 2, 50, (1, 1, 1, 1, 1)), mode_team(5, 2, 50, (5,))], capacity=1 << 14)


def stream_run(sh):
    from microservice_matchmaking_amd.stream import run_stream, stream_schedule
    from microservice_matchmaking_amd.synth import ROLE_WEIGHTS_5V5
    res = run_stream(sh, stream_schedule(**STREAM), role_weights=ROLE_WEIGHTS_5V5, realtime=False,
                     fallback=[(0, 1, AFTER_MS, ROLE_MASK)])
    owner = sh.sharding.chain_owner
    return {"digests": {k: v for k, v in res["digests"].items() if owner[k] == sh.rank}, "moved": res["moved"],
            "refused": res["refused"], "matched": res["matched"], "full_at_s": res["full_at_s"],
            "wait_ms": [np.sort(w) for w in res["wait_ms"]]}


def stream_worker(rank, world, port, engine, out_q):
    from microservice_matchmaking_amd.sharding import ShardedSearch
    dist = _init(rank, world, port)
    w = np.outer([1.0, 0.6], [0.30, 0.10, 0.10, 0.10, 0.10, 0.10, 0.20])
    with ShardedSearch(stream_cfg(), rank_engine(engine), rank, world, w) as sh:
        res = stream_run(sh)
        gathered = [None] * world
        dist.all_gather_object(gathered, res)
        if rank == 0:
            out_q.put((gathered, sh.sharding.chain_owner.tolist()))
    dist.barrier()
    dist.destroy_process_group()


def full_worker(rank, world, port, engine, out_q):
    """Two ranks, one rating group: rank 0 owns the strict chain, rank 1 the fallback's, whose pool is too full for the
    players rank 0 sends.  Every rank must raise MM_ERR_FULL; a rank that did not would hang in the barrier below."""
    from microservice_matchmaking_amd.sharding import ShardedSearch
    dist = _init(rank, world, port)
    cfg = make_config([mode_1v1(window=0), mode_1v1(window=0)], capacity=2048, groups=ONE_GROUP)
    with ShardedSearch(cfg, rank_engine(engine), rank, world, np.array([[2.0], [1.0]])) as sh:
        assert sh.sharding.chain_owner.tolist() == [[0], [1]]
        sh.engine.clock_set(10)
        rating = (np.arange(2500) * 13).astype(np.int32)        # all different: a window of 0 matches nobody
        sh.enqueue(rating, cons_make(np.r_[np.zeros(1500), np.ones(1000)]))
        sh.engine.clock_set(20)
        status = 0
        try:
            sh.move(0, 1, 5)
        except MMError as ex:
            status = ex.status
        depth = [int(sh.engine.queue_depth(md).sum()) for md in range(2)]
        gathered = [None] * world
        dist.all_gather_object(gathered, (status, depth, int(sh.engine.expire(0, 0)[0].size)))
        if rank == 0:
            out_q.put(gathered)
    dist.barrier()
    dist.destroy_process_group()


class RankFailure(AssertionError):
    """A rank process of spawn() did not end well.  status: what a caller that is itself a worker process should exit with —
    124 after a hang, 134 / 137 / 139 after a rank that died of a signal (the statuses tests/test_gpu_carry.py stops on),
    1 after a rank that merely failed."""

    def __init__(self, status, what):
        super().__init__(what)
        self.status = status


def _rank_status(code):
    return 1 if code >= 0 else {6: 134, 9: 137, 11: 139}.get(-code, 139)


def spawn(target, world, args, timeout=400):
    """tests/test_sharding_gloo.py's spawn: `world` processes, the result from rank 0's queue, every exit status 0.  A rank
    that dies is noticed at once (the others would wait for it in a collective until the time limit)."""
    import queue
    import socket
    import time

    import torch.multiprocessing as mp
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        port = s.getsockname()[1]
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    procs = [ctx.Process(target=target, args=(r, world, port) + args[:1] + (q,) + args[1:]) for r in range(world)]
    for p in procs:
        p.start()
    try:
        t_end, out = time.monotonic() + timeout, None
        while out is None:
            try:
                out = (q.get(timeout=0.5),)
            except queue.Empty:
                bad = [(r, p.exitcode) for r, p in enumerate(procs) if p.exitcode not in (None, 0)]
                if bad:
                    raise RankFailure(max(_rank_status(c) for _, c in bad), "ranks ended with (rank, status) %s" % bad)
                if time.monotonic() > t_end:
                    raise RankFailure(124, "no result from rank 0 within %d s" % timeout)
        out = out[0]
        for r, p in enumerate(procs):
            p.join(timeout=120)
            if p.exitcode is None:
                raise RankFailure(124, "rank %d did not end" % r)
            if p.exitcode != 0:
                raise RankFailure(_rank_status(p.exitcode), "rank %d ended with status %d" % (r, p.exitcode))
    finally:
        for p in procs:                                        # a rank that is still there after a failure must not stay behind
            if p.is_alive():
                p.terminate()
                p.join(timeout=30)
    return out


def leaving_worker(rank, world, port, code, out_q):
    """Rank 1 leaves with `code` before the rendezvous; rank 0 waits for it there (tests/test_carry.py: spawn notices)."""
    if rank == 1:
        os._exit(code)
    _init(rank, world, port)


def one_engine(engine_cls, cfg, run):
    """The same script on ONE engine through mm_move (ShardedSearch of one rank)."""
    from microservice_matchmaking_amd.sharding import ShardedSearch
    with ShardedSearch(cfg, engine_cls, 0, 1) as one:
        return run(one)
