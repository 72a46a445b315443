"""Shared drivers for mm_rotate (include/mm_wait.h): tests/test_rotate.py runs them on the CPU shim, tests/test_gpu_rotate.py
on the GPU (one scenario per process, tests/rotate_gpu_worker.py).

The witness is the unchanged oracle: a rotation is a cancel of the LIVE seats of the selected stored lobbies plus an enqueue
of the same rows — rating, constraint word, rating group — so engine A rotates, the test works out in numpy which seats that
must have been (lobby_state and queue_slots of A as they stood before the call, against the test's own live table), requires
A's list to be exactly that, cancels the old slots on oracle B and enqueues the same rows with their groups there: the slots
B hands out must be A's mm_moved column word for word.  From there on the two tick alike, and every wait figure of A is the
clock minus the stamp the player got when it FIRST arrived.

RotOwnerEngine is the restatement: the route an owner has today (move_scenarios.OwnerEngine plus the rotation), on the
oracle and numpy tables alone."""
from __future__ import annotations

import numpy as np

from helpers import assert_same_state
from microservice_matchmaking_amd._abi import NO_SLOT, MMError, cons_make
from microservice_matchmaking_amd.config import REFERENCE_RATING_GROUPS, make_config, mode_1v1, mode_team
from move_scenarios import (MM_ERR_FULL, MM_ERR_INVALID_ARG, MM_ERR_RANGE, MM_ERR_STATE, ROLE_MASK, Duo, MoveTracker,
                            OwnerEngine, four_mode_config, pool)
from wait_scenarios import assert_wait_stats, random_batch, tick_both

MM_PATH_GENERIC, MM_PATH_PAIR, MM_PATH_TEAM = 1, 2, 4


def expected_rotation(tr, eng, mode, max_seated, min_queue=1):
    """include/mm_wait.h, mm_rotate: per rating group the LIVE seats of the stored lobby in lobby_state's order, all of them
    iff there are 1..max_seated and the queue (cancelled, unpurged entries included) holds at least min_queue entries."""
    slots, group = [], []
    for g in range(tr.cfg.n_groups):
        ls = eng.lobby_state(mode, g)[0].astype(np.uint32)
        live = ls[~tr.gone[mode, ls]]
        if 1 <= live.size <= max_seated and eng.queue_slots(mode, g).size >= min_queue:
            slots.append(live)
            group.append(np.full(live.size, g, np.uint32))
    slots = np.concatenate(slots) if slots else np.zeros(0, np.uint32)
    group = np.concatenate(group) if group else np.zeros(0, np.uint32)
    return slots, group, tr.ages(slots)


def rotate_both(a, b, tr, mode, max_seated, min_queue=1, tag="", tick=True):
    """A rotates; its list is what numpy says; B cancels the old slots and enqueues the same rows with their groups; the
    slots B hands out are A's new-slot column.  Then (tick) both tick the mode alike, the states are the same and A's wait
    statistics are the tracker's.  Returns A's four columns (and the tick's matches with tick=True)."""
    cfg = tr.cfg
    want = expected_rotation(tr, a, mode, max_seated, min_queue)
    got = a.rotate(mode, max_seated, min_queue)
    for name, w, x in zip(("slots", "group", "age"), want, got):
        assert np.array_equal(w, x), (tag, "rotated", name, mode, max_seated, min_queue, w[:8], x[:8], w.size, x.size)
    old, group, _, new = got
    b.cancel(old)
    nb = b.enqueue(tr.rating[old], tr.cons[old], group.astype(np.uint8)) if old.size else np.zeros(0, np.uint32)
    assert np.array_equal(nb, new), (tag, "new slots", nb[:8], new[:8], int((nb != new).sum()))
    assert (new != NO_SLOT).all(), (tag, "nobody can be refused")
    tr.moved(mode, old, new, tr.cons[old])
    assert_same_state(a, b, cfg, tag + " after the rotation")
    assert_wait_stats(a, tr, mode, tag + " after the rotation")
    if not tick:
        return got
    m = tick_both(a, b, tr, mode, tag + " tick after the rotation")
    assert_same_state(a, b, cfg, tag + " after the tick")
    assert_wait_stats(a, tr, mode, tag + " after the tick")
    return got, m


class RotOwnerEngine(OwnerEngine):
    """OwnerEngine plus the rotation as an owner does it today: per rating group the stored lobby, a live table, rating and
    constraint word from a table of its own, cancel, enqueue with the groups, the stamps carried."""

    def rotate(self, mode, max_seated, min_queue=1):
        if self.tr.now is None:
            raise MMError(MM_ERR_STATE, "owner rotate")
        s, g, a = expected_rotation(self.tr, self.b, mode, max_seated, min_queue)
        self.b.cancel(s)
        new = self.b.enqueue(self.tr.rating[s], self.tr.cons[s], g.astype(np.uint8)) if s.size else np.zeros(0, np.uint32)
        self.tr.moved(mode, s, new, self.tr.cons[s])
        return s, g, a, new


class RDuo(Duo):
    def rotate(self, mode, max_seated, min_queue=1, tag="", tick=True):
        return rotate_both(self.a, self.b, self.tr, mode, max_seated, min_queue, tag, tick)

    def enqueue_grouped(self, rating, cons, group):
        group = np.asarray(group, np.uint8)
        sa, sb = self.a.enqueue(rating, cons, group), self.b.enqueue(rating, cons, group)
        assert np.array_equal(sa, sb), ("slots", sa[:8], sb[:8])
        self.tr.enqueued_rows(sa, rating, cons)
        return sa


def region_cfg(capacity=256, groups=REFERENCE_RATING_GROUPS):
    return make_config([mode_1v1(window=25, region_filter=True)], capacity=capacity, groups=groups)


# ---- 1. the blocked head, closed form ---------------------------------------------------------------------------------

def blocked_head(engine_cls, oracle_cls):
    """A, B, C in one rating group of a region-filtered 1v1: B and C fit each other, neither fits A, and A came first."""
    with RDuo(engine_cls, oracle_cls, region_cfg()) as d:
        d.clock(100)
        A, B, C = d.enqueue(np.asarray([1000, 1000, 1005], np.int32), cons_make(0, [0, 1, 1])).tolist()
        assert len(d.tick(0, "A anchors and blocks")) == 0
        assert d.a.lobby_state(0, 0)[0].tolist() == [A] and d.a.queue_slots(0, 0).tolist() == [B, C]
        assert len(d.tick(0, "and again: the chain stands still")) == 0
        d.clock(150)
        (s, g, age, new), m = d.rotate(0, 1, 1, "blocked head")
        assert s.tolist() == [A] and g.tolist() == [0] and age.tolist() == [50]
        assert len(m) == 1 and sorted(m.slots[0].tolist()) == sorted([B, C])
        assert d.a.matches_wait().tolist() == [[50, 50]]
        st = d.a.wait_stats(0)
        assert [w["waiting"] for w in st] == [1, 0, 0, 0, 0, 0, 0] and st[0]["oldest_age"] == 50 and st[0]["age_sum"] == 50
        assert d.a.lobby_state(0, 0)[0].tolist() == new.tolist()        # A anchors again, behind the lobby it had blocked


# ---- 2. the scan across rating groups ----------------------------------------------------------------------------------

def wide_groups(n):
    return [(1000 * g, 1000 * g + 999, "g%d" % g) for g in range(n)]


def group_counts(engine_cls, oracle_cls, n_groups):
    """n_groups rating groups in a 1v1 of window 0 with all ratings different (nobody ever matches), by g % 4: empty |
    stored lobby only | queue only | lobby and queue.  min_queue 1 takes the last kind, min_queue 0 the second too."""
    done = []
    for min_queue in (1, 0):
        cfg = make_config([mode_1v1(window=0)], capacity=256, groups=wide_groups(n_groups))
        with RDuo(engine_cls, oracle_cls, cfg) as d:
            kind = [3] if n_groups == 1 else [g % 4 for g in range(n_groups)]
            d.clock(10)
            first = [1000 * g + 7 * j for g in range(n_groups) for j in range({1: 1, 3: 3}.get(kind[g], 0))]
            d.enqueue(np.asarray(first, np.int32), cons_make(np.zeros(len(first))))
            assert len(d.tick(0, "anchors")) == 0
            late = [1000 * g + 500 + 7 * j for g in range(n_groups) if kind[g] == 2 for j in range(2)]
            d.clock(20)
            d.enqueue(np.asarray(late, np.int32), cons_make(np.zeros(len(late))))
            assert [d.a.lobby_state(0, g)[0].size for g in range(n_groups)] == [int(k in (1, 3)) for k in kind]
            assert [d.a.queue_slots(0, g).size for g in range(n_groups)] == [{2: 2, 3: 2}.get(k, 0) for k in kind]
            d.clock(30)
            (s, g, age, new), _ = d.rotate(0, 1, min_queue, "%d groups, min_queue %d" % (n_groups, min_queue))
            want = [x for x in range(n_groups) if kind[x] == 3 or (min_queue == 0 and kind[x] == 1)]
            assert g.tolist() == want and (age == 20).all()
            done.append(int(s.size))
            d.rotate(0, 1, min_queue, "and once more")
    return done


# ---- 3. lobby shapes ---------------------------------------------------------------------------------------------------

SHAPES = {                                                   # name: (team_size, teams, quota, seated)
    "1v1_lone_anchor": (1, 2, (1,), 1),
    "3_teams_of_2": (2, 3, (2,), 5),
    "5v5_9_seated": (5, 2, (5,), 9),
    "2x8_15_seated": (8, 2, (8,), 15),                       # the most seats a stored lobby can hold
}


def seated_lobby(d, mode, seated, behind=3, rating=1000, far=1300):
    """`seated` players of one rating who fit each other, then `behind` who fit nobody (window 10): one tick seats the
    first lot into the stored lobby of group 0 and leaves the others queued."""
    r = np.concatenate([np.full(seated, rating), far + 40 * np.arange(behind)]).astype(np.int32)
    s = d.enqueue(r, cons_make(mode, np.zeros(r.size)))
    assert len(d.tick(mode, "seat %d" % seated)) == 0
    ls = d.a.lobby_state(mode, 0)[0]
    assert sorted(ls.tolist()) == sorted(s[:seated].tolist()) and d.a.queue_slots(mode, 0).tolist() == s[seated:].tolist()
    return s, ls


def lobby_shape(engine_cls, oracle_cls, name):
    ts, teams, quota, seated = SHAPES[name]
    cfg = make_config([mode_team(ts, teams, 10, quota) if ts > 1 else mode_1v1(window=10)], capacity=256)
    with RDuo(engine_cls, oracle_cls, cfg) as d:
        d.clock(5)
        _, ls = seated_lobby(d, 0, seated)
        d.clock(9)
        if seated > 1:
            assert d.rotate(0, seated - 1, 1, name + ": one seat too many", tick=False)[0].size == 0
        (s, g, age, new), m = d.rotate(0, seated, 1, name)
        assert np.array_equal(s, ls) and (g == 0).all() and (age == 4).all() and len(m) == 0
        assert not set(d.a.lobby_state(0, 0)[0].tolist()) & set(ls.tolist())     # the old seats are gone from the lobby
        assert d.a.path_stats()["paths"] == (MM_PATH_GENERIC if ts > 1 else MM_PATH_PAIR)   # a chain this short is k_walk's
        d.clock(12)
        d.enqueue(np.full(2 * ts * teams, 1000, np.int32), cons_make(0, np.zeros(2 * ts * teams)))
        d.rotate(0, ts * teams, 0, name + " with fresh players")
        return int(s.size)


def dead_seat(engine_cls, oracle_cls):
    """5v5 with four seated, one of them cancelled: three LIVE seats.  max_seated 2 selects nobody, 3 selects the three, and
    the dead seat is not in the list."""
    cfg = make_config([mode_team(5, 2, 10, (5,))], capacity=256)
    with RDuo(engine_cls, oracle_cls, cfg) as d:
        d.clock(5)
        _, ls = seated_lobby(d, 0, 4)
        d.cancel(0, ls[1:2])
        assert d.a.lobby_state(0, 0)[0].size == 4            # still listed: nothing has looked at the lobby since
        assert d.rotate(0, 2, 1, "three live seats, max_seated 2", tick=False)[0].size == 0
        (s, _, _, _), _ = d.rotate(0, 3, 1, "three live seats, max_seated 3")
        assert s.tolist() == [ls[0], ls[2], ls[3]]


# ---- 4. boundaries -----------------------------------------------------------------------------------------------------

def boundaries(engine_cls, oracle_cls):
    cfg = make_config([mode_team(5, 2, 10, (5,))], capacity=256)
    with RDuo(engine_cls, oracle_cls, cfg) as d:
        d.clock(1)
        s, ls = seated_lobby(d, 0, 4, behind=3)
        assert d.rotate(0, 3, 1, "|S| == max_seated + 1", tick=False)[0].size == 0
        assert d.rotate(0, 4, 4, "len == min_queue - 1", tick=False)[0].size == 0
        assert d.rotate(0, 4, 3, "|S| == max_seated and len == min_queue", tick=False)[0].size == 4
        d.tick(0, "the four sit again")
    with RDuo(engine_cls, oracle_cls, cfg) as d:               # a queue of cancelled, unpurged entries counts
        d.clock(1)
        s, ls = seated_lobby(d, 0, 2, behind=2)
        d.cancel(0, s[2:])
        assert d.a.queue_slots(0, 0).size == 2
        (got, _, _, _), _ = d.rotate(0, 2, 2, "two cancelled entries are a queue of two")
        assert got.size == 2
    with RDuo(engine_cls, oracle_cls, cfg) as d:               # min_queue 0 with an empty queue
        d.clock(1)
        seated_lobby(d, 0, 3, behind=0)
        assert d.a.queue_slots(0, 0).size == 0
        assert d.rotate(0, 3, 1, "empty queue, min_queue 1", tick=False)[0].size == 0
        (got, _, _, _), _ = d.rotate(0, 3, 0, "empty queue, min_queue 0")
        assert got.size == 3


# ---- 5. slots ----------------------------------------------------------------------------------------------------------

def anchors(d, n_groups, mode=0, extra=1):
    """One anchor and `extra` queued players per rating group of a window-0 1v1 (wide_groups): ticked, nobody matches."""
    r = np.asarray([1000 * g + 7 * j for g in range(n_groups) for j in range(1 + extra)], np.int32)
    s = d.enqueue(r, cons_make(mode, np.zeros(r.size)))
    assert len(d.tick(mode, "anchors")) == 0
    return s


def slots_contiguous(engine_cls, oracle_cls):
    cfg = make_config([mode_1v1(window=0)], capacity=64, groups=wide_groups(7))
    with RDuo(engine_cls, oracle_cls, cfg) as d:
        d.clock(1)
        anchors(d, 7)                                          # slots 0..13
        (s, _, _, new), _ = d.rotate(0, 1, 1, "contiguous")
        assert s.tolist() == list(range(0, 14, 2)) and new.tolist() == list(range(14, 21))
        assert d.enqueue(np.asarray([3], np.int32), cons_make([0])).tolist() == [21]


def slots_wrapped_with_a_waiting_player_in_the_way(engine_cls, oracle_cls):
    """capacity 32.  Mode 1 (window 5000) churns the ring until next_slot is 28 while mode 0's anchors and queues hold
    slots 0..7 and a long-waiting loner holds 30: a rotation of 4 gets 28, 29, 31 and — wrapped, behind the held 0..7 — 8."""
    cfg = make_config([mode_1v1(window=0), mode_1v1(window=5000)], capacity=32, groups=wide_groups(4))
    with RDuo(engine_cls, oracle_cls, cfg) as d:
        d.clock(1)
        anchors(d, 4)                                          # 0..7
        pair = lambda k: (np.asarray([500, 500], np.int32) + k, cons_make([1, 1]))
        d.enqueue(*pair(0))                                    # 8, 9
        d.tick(1)
        for k in range(10):                                    # 10..29
            d.enqueue(*pair(k))
            d.tick(1)
        lone = d.enqueue(np.asarray([1500, 2600], np.int32), cons_make([1, 1]))      # 30, 31: two groups, nobody to meet
        assert lone.tolist() == [30, 31]
        d.cancel(1, lone[1:])
        d.tick(1)                                              # 31 is free again, 30 waits on; the ring is back at 0
        for k in range(10):                                    # 8, 9 | 10, 11 | ... behind the held 0..7: the ring comes to 28
            got = d.enqueue(*pair(k))
            d.tick(1)
        assert got.tolist() == [26, 27]
        d.clock(50)
        (s, _, age, new), _ = d.rotate(0, 1, 1, "wrapped, with a waiting player in the way")
        assert s.tolist() == [0, 2, 4, 6] and (age == 49).all() and new.tolist() == [28, 29, 31, 8]
        assert d.enqueue(*pair(3)).tolist() == [9, 10]


def full_one_short(engine_cls, oracle_cls):
    """Free slots one short of the selection: MM_ERR_FULL and nothing has changed — snapshot bytes, the slot the next
    enqueue gets, the lists — and the engine stays usable."""
    cfg = make_config([mode_1v1(window=0)], capacity=16, groups=wide_groups(4))
    with RDuo(engine_cls, oracle_cls, cfg) as d:
        d.clock(1)
        anchors(d, 4, extra=2)                                 # 12 of 16 slots: an anchor and two queued per group
        d.enqueue(np.asarray([50], np.int32), cons_make([0]))   # 13 held, 3 free, 4 selected
        d.clock(9)
        before = d.a.snapshot() if hasattr(d.a, "snapshot") else None
        assert d.a.expire(0, 1000)[0].size == 0                 # (an empty list from another call)
        with_err = None
        try:
            d.a.rotate(0, 1, 1)
        except MMError as ex:
            with_err = ex.status
        assert with_err == MM_ERR_FULL, with_err
        assert d.a._fn("expired")(d.a._h, 0, 1, None, None, None) == MM_ERR_RANGE
        assert d.a._fn("moved")(d.a._h, 0, 1, None) == MM_ERR_RANGE
        assert d.a._fn("moved_rows")(d.a._h, 0, 1, None, None, None) == MM_ERR_RANGE
        assert d.a.snapshot() == before
        assert_same_state(d.a, d.b, cfg, "after MM_ERR_FULL")
        d.stats(0, "after MM_ERR_FULL")
        d.cancel(0, d.a.queue_slots(0, 3)[-1:])                 # somebody gives up ...
        d.tick(0, "... and the purge frees the slot")
        assert d.enqueue(np.asarray([60], np.int32), cons_make([0])).tolist() == [13]   # next_slot was where it had been
        d.cancel(0, np.asarray([13], np.uint32))
        d.tick(0)
        (s, _, _, new), _ = d.rotate(0, 1, 1, "with exactly enough room")
        assert s.size == 4 and sorted(new.tolist()) == sorted(set(range(16)) - set(range(11)) - {12} | {11, 13})


# ---- 6. the group override ---------------------------------------------------------------------------------------------

def group_override(engine_cls, oracle_cls):
    """Players placed into rating group 5 by override, with ratings of group 0: the rotation keeps them in group 5."""
    with RDuo(engine_cls, oracle_cls, region_cfg()) as d:
        d.clock(3)
        s = d.enqueue_grouped(np.asarray([100, 100, 110], np.int32), cons_make(0, [0, 1, 1]), [5, 5, 5])
        assert len(d.tick(0)) == 0 and d.a.lobby_state(0, 5)[0].tolist() == [s[0]]
        d.clock(8)
        (old, g, _, new), m = d.rotate(0, 1, 1, "override")
        assert old.tolist() == [s[0]] and g.tolist() == [5] and len(m) == 1 and m.group.tolist() == [5]
        assert d.a.lobby_state(0, 5)[0].tolist() == new.tolist() and d.a.queue_depth(0).sum() == 0
        assert d.a.lobby_state(0, 0)[0].size == 0


# ---- 7. the host route on a second engine of the same kind -------------------------------------------------------------

def host_route(eng, tr, mode, max_seated, min_queue):
    """What mm_rotate replaces: mm_lobby_state per rating group, a table of the owner's, mm_cancel, mm_enqueue_stamped."""
    s, g, a = expected_rotation(tr, eng, mode, max_seated, min_queue)
    eng.cancel(s)
    new = eng.enqueue_stamped(tr.rating[s], tr.cons[s], tr.stamp[s], g.astype(np.uint8)) if s.size else np.zeros(0, np.uint32)
    return s, g, a, new


def host_route_equivalence(engine_cls, oracle_cls, seed=3, rounds=6):
    """Two engines of the same kind, the same script: one rotates through mm_rotate, the other through the host route.
    The same lists and new slots, queue order, stamps (wait statistics, matches_wait) and ticks."""
    cfg = four_mode_config(4096)
    rng = np.random.default_rng(seed)
    rotated = 0
    with RDuo(engine_cls, oracle_cls, cfg) as d, engine_cls(cfg) as c:
        for rnd in range(rounds):
            d.clock(100 + 17 * rnd)
            c.clock_set(100 + 17 * rnd)
            rating, cons = random_batch(rng, cfg, 300 if rnd == 0 else 60)
            assert np.array_equal(d.enqueue(rating, cons), c.enqueue(rating, cons))
            for md in range(cfg.n_modes):
                L = int(cfg.modes[md].teams * cfg.modes[md].team_size)
                args = (md, int(rng.integers(1, L)), int(rng.integers(0, 3)))
                want = host_route(c, d.tr, *args)
                got = d.rotate(*args, tag="round %d mode %d" % (rnd, md), tick=False)
                for w, x in zip(want, got):
                    assert np.array_equal(w, x), (rnd, md, w, x)
                rotated += int(got[0].size)
                assert_same_state(d.a, c, cfg, "host route, round %d mode %d" % (rnd, md))
                assert_wait_stats(c, d.tr, md, "host route")
                ma, mc = d.tick(md), c.tick(md)
                assert np.array_equal(ma.slots, mc.slots) and np.array_equal(d.a.matches_wait(), c.matches_wait())
                assert_same_state(d.a, c, cfg, "host route after the tick, round %d mode %d" % (rnd, md))
                assert_wait_stats(c, d.tr, md, "host route after the tick")
    assert rotated > 10
    return rotated


# ---- 8. errors ---------------------------------------------------------------------------------------------------------

def errors(engine_cls):
    def status(a, *args):
        try:
            a.rotate(*args)
        except MMError as ex:
            return ex.status
        return 0

    cfg = region_cfg()
    with engine_cls(cfg) as a:
        a.enqueue(np.asarray([1000, 1000], np.int32), cons_make(0, [0, 1]))
        a.tick(0)
        assert status(a, 0, 1, 1) == MM_ERR_STATE                            # the clock was never set
        a.clock_set(5)
        assert status(a, 1, 1, 1) == MM_ERR_INVALID_ARG                      # no such mode
        assert status(a, 0, 0, 1) == MM_ERR_INVALID_ARG                      # max_seated == 0
        assert a.lobby_state(0, 0)[0].tolist() == [0] and a.queue_slots(0, 0).tolist() == [1]
        got = a.rotate(0, 1, 2)                                              # nothing selected: MM_OK, empty lists, no slot taken
        assert all(x.size == 0 for x in got)
        assert a._fn("moved")(a._h, 0, 0, None) == 0 and a._fn("moved")(a._h, 0, 1, None) == MM_ERR_RANGE
        assert a.enqueue(np.asarray([4000], np.int32), cons_make([0])).tolist() == [2]
        got = a.rotate(0, 1, 1)
        assert got[0].tolist() == [0] and got[3].tolist() == [3]
        assert a._fn("moved_rows")(a._h, 0, 1, None, None, None) == MM_ERR_RANGE   # mm_moved_rows reads empty
        assert a._fn("rotate")(a._h, 0, 1, 1, None) == 0                     # n_selected may be NULL (nothing left to select)
    with engine_cls(cfg, {"fail_tick": 1}) as a:                             # a poisoned engine
        a.clock_set(1)
        a.enqueue(np.asarray([1000, 1000], np.int32), cons_make(0, [0, 1]))
        try:
            a.tick(0)
            raise AssertionError("the tick was to fail")
        except MMError:
            pass
        assert status(a, 0, 1, 1) == MM_ERR_STATE
        a.reset()
        a.clock_set(2)
        assert a.rotate(0, 1, 1)[0].size == 0


# ---- 9. random scripts -------------------------------------------------------------------------------------------------

def rotate_script(engine_cls, oracle_cls, seed=1, rounds=8, first=500, batch=90, restart_at=(), cfg=None):
    """Enqueue, cancel, expire, move, rotate, tick and snapshot / restore mixed, in a region-filtered 1v1, two role-bound
    team modes and a role-free one (move_scenarios.four_mode_config), against the oracle after every step.  The batches
    are small against 4 modes x 7 groups, so most chains end a tick with a short-handed stored lobby: the rotations have
    somebody to select.  Returns (log, rotate calls, rotate calls that selected somebody)."""
    cfg = cfg or four_mode_config(4096)
    rng = np.random.default_rng(seed)
    d = RDuo(engine_cls, oracle_cls, cfg)
    a_cls = engine_cls
    now, calls, hits, log = 1000, 0, 0, []
    try:
        for rnd in range(rounds):
            now += int(rng.integers(1, 60))
            d.clock(now)
            rating, cons = random_batch(rng, cfg, first if rnd == 0 else int(rng.integers(0, batch + 1)))
            d.enqueue(rating, cons)
            live = d.tr.live_slots()
            k = int(live.size * 0.03)
            if k:
                cs = rng.choice(live, size=k, replace=False)
                mode_of = np.full(int(cfg.capacity), -1, np.int64)
                for md in range(cfg.n_modes):
                    for g in range(cfg.n_groups):
                        mode_of[d.a.lobby_state(md, g)[0]] = md
                        mode_of[d.a.queue_slots(md, g)] = md
                d.a.cancel(cs)
                d.b.cancel(cs)
                for md in range(cfg.n_modes):
                    d.tr.marked(md, cs[mode_of[cs] == md])
            if rng.random() < 0.5:
                got = d.move(2, 3, int(rng.integers(20, 200)), ROLE_MASK, "round %d" % rnd)
                log.append(("moved", rnd, got[0].tolist(), got[3].tolist()))
            if rng.random() < 0.3:
                md = int(rng.integers(0, cfg.n_modes))
                got = d.expire(md, int(rng.integers(60, 300)), "round %d" % rnd)
                log.append(("expired", rnd, md, got[0].tolist()))
            for md in range(cfg.n_modes):
                L = int(cfg.modes[md].teams * cfg.modes[md].team_size)
                for _ in range(int(rng.integers(1, 3))):        # one or two rounds of rotate and tick, as the stream runs them
                    got, m = d.rotate(md, int(rng.integers(1, L)), int(rng.integers(0, 3)), "round %d mode %d" % (rnd, md))
                    calls += 1
                    hits += int(got[0].size > 0)
                    log.append(("rotated", rnd, md, got[0].tolist(), got[3].tolist(), m.slots.tolist()))
            if rnd in restart_at and getattr(d.a, "restartable", True):
                blob, clk = d.a.snapshot(), d.a.clock()
                d.a.close()
                d.a = a_cls(cfg)
                d.a.restore(blob)
                assert d.a.clock() == clk
                assert_same_state(d.a, d.b, cfg, "right after restore %d" % rnd)
            for md, m in enumerate(d.tick_all("round %d" % rnd)):
                log.append(("tick", rnd, md, m.slots.tolist()))
    finally:
        d.__exit__()
    return log, calls, hits


def assert_share(calls, hits):
    print("rotate calls %d, of which %d selected somebody" % (calls, hits))
    assert calls >= 32 and 4 * hits >= calls, (calls, hits)


# ---- 10. the stream ----------------------------------------------------------------------------------------------------

STREAM = dict(qps=100, seconds=3.0, tick_ms=100.0, seed=7)     # 30 periods of about 10 arrivals: the low-rate regime
LOW_RATE = dict(qps=50, seconds=6.0, tick_ms=100.0, seed=11)   # 60 periods of about 5 (the shim takes tens of ms a call)


def stream_cfg():
    return make_config([mode_1v1(window=25, region_filter=True)], capacity=1 << 12)


def stream_run(sh, rounds, sched=None):
    from microservice_matchmaking_amd.stream import run_stream, stream_schedule
    rot = None if rounds is None else {"max_seated": [1], "min_queue": 1, "rounds": rounds}
    res = run_stream(sh, stream_schedule(**(sched or STREAM)), realtime=False, rotate=rot)
    owner = sh.sharding.chain_owner
    out = {"digests": {k: v for k, v in res["digests"].items() if owner[k] == sh.rank}, "matched": res["matched"],
           "lobbies": {k: v for k, v in res["lobbies"].items() if owner[k] == sh.rank}, "full_at_s": res["full_at_s"],
           "depth": [x.tolist() for x in res["depth"]]}
    if rounds is not None:
        out.update({"rotated": res["rotated"], "rotate_rounds": res["rotate_rounds"],
                    "wait_ms": [np.sort(w) for w in res["wait_ms"]]})
    return out


def stream_one(engine_cls, rounds, sched=None):
    from microservice_matchmaking_amd.sharding import ShardedSearch
    with ShardedSearch(stream_cfg(), engine_cls, 0, 1) as sh:
        return stream_run(sh, rounds, sched)


def stream_worker(rank, world, port, engine, out_q, rounds=1):
    from carry_scenarios import _init, rank_engine
    from microservice_matchmaking_amd.sharding import ShardedSearch
    dist = _init(rank, world, port)
    with ShardedSearch(stream_cfg(), rank_engine(engine), rank, world) as sh:
        res = stream_run(sh, rounds)
        gathered = [None] * world
        dist.all_gather_object(gathered, res)
        if rank == 0:
            out_q.put(gathered)
    dist.barrier()
    dist.destroy_process_group()


def assert_ranks_are_one_engine(gathered, want):
    """Every chain has one owner: the ranks' digests together are the one engine's, the counters sum, and every rank ran the
    rounds the one engine ran (the stop decisions are maxima over the ranks)."""
    digests = {}
    for r in gathered:
        assert not set(r["digests"]) & set(digests)
        digests.update(r["digests"])
    assert digests == want["digests"]
    assert sum(r["matched"] for r in gathered) == want["matched"]
    assert [sum(r["rotated"][0] for r in gathered)] == want["rotated"]
    assert all(r["rotate_rounds"] == want["rotate_rounds"] for r in gathered), [r["rotate_rounds"] for r in gathered]
    assert np.array_equal(np.sort(np.concatenate([r["wait_ms"][0] for r in gathered])), want["wait_ms"][0])


# ---- 11. product geometry (GPU tier) -----------------------------------------------------------------------------------

def pair_geometry(engine_cls, oracle_cls, per_chain=3 * 4096):
    """A region-filtered 1v1 with a few times 4096 players in the chain of rating group 0 behind a blocked anchor: the tick
    after the rotation runs the pair path with the rotated seat among the cancelled entries it filters and the same player
    at the tail."""
    cfg = make_config([mode_1v1(window=25, region_filter=True)], capacity=1 << 16)
    with RDuo(engine_cls, oracle_cls, cfg) as d:
        d.clock(10)
        lone = d.enqueue(np.asarray([700, 1700], np.int32), cons_make(0, [9, 9]))     # a rare region: anchors of groups 0 and 1
        assert len(d.tick(0, "rare anchors")) == 0
        d.clock(500)
        rating, cons = pool(per_chain, 71, 0, hi=1499)
        d.enqueue(rating, cons)
        d.enqueue(*pool(40, 72, 0, lo=1500, hi=1999))
        (s, g, age, new), m = d.rotate(0, 1, 1, "pair geometry")
        assert s.tolist() == lone.tolist() and (age == 490).all() and len(m) > per_chain // 4
        ps = d.a.path_stats()
        assert ps["paths"] & MM_PATH_PAIR, ps
        (s2, _, _, _), m2 = d.rotate(0, 1, 1, "and the leftovers")
        return len(m), len(m2), ps["paths"]


def team_geometry(engine_cls, oracle_cls, n=6000):
    """5v5: rating group 0 holds enough players for the team path behind a stored lobby of a few seats, rating group 3 a
    chain short enough for k_walk (which takes the chains the team path leaves; mm_path_stats records it only when it
    walks alone — lobby_shape asserts that); both lobbies rotate, and the tick after it seats people in both groups."""
    cfg = make_config([mode_team(5, 2, 50, (1, 1, 1, 1, 1))], capacity=1 << 15)
    with RDuo(engine_cls, oracle_cls, cfg) as d:
        d.clock(10)
        d.enqueue(*pool(7, 81, 0, 2, hi=1499))                 # two roles only: a lobby of a few seats that cannot fill
        d.enqueue(*pool(5, 82, 0, 2, lo=2500, hi=2999))
        assert len(d.tick(0, "partial lobbies")) == 0
        seated = [d.a.lobby_state(0, g)[0].size for g in (0, 3)]
        assert min(seated) >= 1
        d.clock(300)
        d.enqueue(*pool(n, 83, 0, 5, hi=1499))
        d.enqueue(*pool(400, 84, 0, 5, lo=2500, hi=2999))
        (s, g, age, new), m = d.rotate(0, 9, 1, "team geometry")
        assert sorted(set(g.tolist())) == [0, 3] and s.size == sum(seated) and (age == 290).all() and len(m) > 0
        ps = d.a.path_stats()
        assert ps["paths"] & MM_PATH_TEAM, ps
        assert set(m.group.tolist()) == {0, 3}
        d.rotate(0, 9, 1, "and the leftovers")
        return len(m), ps["paths"]
