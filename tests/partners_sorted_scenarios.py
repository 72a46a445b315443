"""Shared drivers for the sorted route of mm_partners and the rule calls (include/mm_wait.h, mm_tuning.wait_sort_mtests):
tests/test_partners_sorted.py runs them on the CPU shim, tests/test_gpu_partners_sorted.py on the GPU (each scenario group in
a process of its own, tests/partners_sorted_gpu_worker.py).

The route changes how the partner counts are worked out, never a word of them, so the witness is what it always was:
partners_scenarios.expected_partners, numpy over the unchanged oracle.  The second witness is the tiles route.  sorted_cls and
tiles_cls wrap an engine class so that every engine of it is forced onto one route and says so after every call
(mm_wait_route_get); the drivers of partners_scenarios and move_if_scenarios take the class and run on the new route unchanged."""
from __future__ import annotations

import ctypes as C

import numpy as np

from geometry import _value, source_defines
from locate_scenarios import CAPACITY, blocked_cfg
from microservice_matchmaking_amd._abi import MM_ROUTE_NONE, MM_ROUTE_SORTED, MM_ROUTE_TILES, NO_SLOT, cons_make
from microservice_matchmaking_amd.config import make_config, mode_1v1, mode_team
from move_if_scenarios import MAX, IfDuo, rule
from move_scenarios import ROLE_MASK, four_mode_config
from partner_stats_scenarios import one_group_cfg
from partners_scenarios import PARTY, REGION, partners_both
from rotate_scenarios import RDuo
from wait_scenarios import random_batch, three_mode_config

MM_ERR_OOM = -3
CALLS = {"partners": 1, "expire_if": 2, "move_if": 3, "move_out_if": 4}
NEVER, ALWAYS = 0xFFFFFFFF, 0


def sample_size():
    """Keys of the sorted table a workgroup stages in LDS, from its #define."""
    return _value("FITQ_SAMPLE", source_defines())


def sort_tile():
    return _value("FIT_TILE", source_defines())


def table_lengths():
    s, t = sample_size(), sort_tile()
    # (s + 2: the first table whose last sample has a key behind it — the last bucket of the sample is not empty)
    return sorted({1, 2, s - 1, s, s + 1, s + 2, t - 1, t + 1, 2 * t + 1})


# ---- 1. the engine-class wrappers --------------------------------------------------------------------------------------

def _routed(engine_cls, mtests, route, name):
    def checked(call):
        def method(self, *args, **kw):
            out = getattr(engine_cls, call)(self, *args, **kw)
            r = self.wait_route()
            assert r["call"] == CALLS[call], (call, r)
            # (a call that counted nothing — no query, nobody old enough — says NONE)
            assert r["route"] in (MM_ROUTE_NONE, route), (call, "route", r)
            if call == "partners" and len(args) > 1 and np.asarray(args[1]).size:
                assert r["route"] == route and r["queries"] == np.asarray(args[1]).size, (call, r)
            assert r["threshold"] == (mtests if r["route"] != MM_ROUTE_NONE else 0), (call, r)
            if r["route"] != MM_ROUTE_SORTED:
                assert r["keys"] == 0 and r["passes"] == 0, (call, r)
            else:
                assert 4 <= r["passes"] <= 7 and r["keys"] <= r["bound"], (call, r)
            return out
        return method

    def init(self, cfg, tuning=None):
        engine_cls.__init__(self, cfg, dict(tuning or {}, wait_sort_mtests=mtests))

    body = {c: checked(c) for c in CALLS}
    body["__init__"] = init
    return type(name + engine_cls.__name__, (engine_cls,), body)


_CACHE = {}


def sorted_cls(engine_cls):
    """engine_cls with wait_sort_mtests = 0 laid over whatever tuning it is given: every count takes the sorted route."""
    return _CACHE.setdefault(("s", engine_cls), _routed(engine_cls, ALWAYS, MM_ROUTE_SORTED, "Sorted"))


def tiles_cls(engine_cls):
    """The same with 0xFFFFFFFF: every count takes the tiles route."""
    return _CACHE.setdefault(("t", engine_cls), _routed(engine_cls, NEVER, MM_ROUTE_TILES, "Tiles"))


# ---- 2. the table's length around the sample and the sort's tile -------------------------------------------------------

def table_and_sample(engine_cls, oracle_cls, n):
    """n players of n consecutive ratings in a fixed shuffled order, one rating group, window 0: everybody waits.  At window 3
    the i-th smallest has min(i, 3) + min(n - 1 - i, 3) partners and a gap of 1; a free slot and a slot past the capacity
    are NONE; the table holds exactly the n."""
    with RDuo(sorted_cls(engine_cls), oracle_cls, one_group_cfg(CAPACITY)) as d:
        i = np.random.default_rng(n).permutation(n)
        s = d.enqueue_grouped((10 + i).astype(np.int32), cons_make(np.zeros(n)), np.full(n, 3))
        q = np.concatenate([s, [CAPACITY - 1, CAPACITY + 7]]).astype(np.uint32)
        got = partners_both(d, 0, q, None, 3, 0, "a table of %d" % n)
        r = d.a.wait_route()
        assert (r["route"], r["keys"], r["queries"], r["passes"]) == (MM_ROUTE_SORTED, n, n + 2, 6), r   # the rating's four passes, the role's byte, the group's
        assert np.array_equal(got[0][:n], np.minimum(i, 3) + np.minimum(n - 1 - i, 3)), "partners"
        assert (got[2][:n] == (1 if n > 1 else NO_SLOT)).all(), "gap"
        assert got[0][n:].tolist() == [0, 0] and got[2][n:].tolist() == [NO_SLOT] * 2 and not got[1][n:].any()
        for gap in (True, False):                              # without by_role: the table without the role, then partners alone
            two = d.a.partners(0, q, window=3, flags=0, by_role=False, gap=gap)
            assert np.array_equal(two[0], got[0]) and (np.array_equal(two[2], got[2]) if gap else two[2] is None), gap
            assert d.a.wait_route()["passes"] == 5
        ends = s[np.argsort(i)[[0, n // 2, n - 1]]]             # the smallest, the middle, the largest: window 2^32 - 1
        assert (partners_both(d, 0, ends, None, 0xFFFFFFFF, 0, "everybody")[0] == n - 1).all()
        assert len(d.tick(0, "the next tick is the oracle's")) == 0


# ---- 3. self is per query ----------------------------------------------------------------------------------------------

def marked_twin(engine_cls, oracle_cls):
    """Two players of equal rating and region, one of them MARKED: the LIVE one is in the table and must not count itself,
    the MARKED one is not and must count its twin; a MARKED player alone in its region has nobody."""
    cfg = make_config([mode_1v1(window=0)], capacity=256)
    with RDuo(sorted_cls(engine_cls), oracle_cls, cfg) as d:
        s = d.enqueue(np.asarray([500, 500, 700, 500], np.int32), cons_make(0, [1, 1, 2, 3]))
        d.cancel(0, s[1:3])
        got = partners_both(d, 0, s, None, 0, REGION, "queue entries")
        assert got[0].tolist() == [0, 1, 0, 0] and got[2].tolist() == [NO_SLOT, 0, NO_SLOT, NO_SLOT], got
        got = partners_both(d, 0, s, None, 0, 0, "the same without the filter")
        assert got[0].tolist() == [1, 2, 0, 1] and got[2].tolist() == [0, 0, 200, 0], got
        d.tick(0, "the next tick")
    with RDuo(sorted_cls(engine_cls), oracle_cls, three_mode_config(CAPACITY)) as d:          # three teams of two, roles 1 + 1
        s = d.enqueue(np.asarray([1000, 1000], np.int32), cons_make(1, 0, 0, [0, 1]))
        assert len(d.tick(1, "two of six sit down")) == 0
        ls = d.b.lobby_state(1, 0)[0]
        assert sorted(ls.tolist()) == sorted(s.tolist())
        d.cancel(1, ls[1:2])
        got = partners_both(d, 1, ls, None, 0, 0, "the same pair as seats of a stored lobby")
        assert got[0].tolist() == [0, 1] and got[2].tolist() == [NO_SLOT, 0], got
        assert got[1][1].tolist()[:2] in ([1, 0], [0, 1])
        d.tick(1, "the next tick")


# ---- 4. the role byte --------------------------------------------------------------------------------------------------

def role_byte(engine_cls, oracle_cls):
    """A 5-role team mode with the party filter beside a 2-role mode: by_role from the role-keyed table.  Role 2 has no
    candidate, role 4 one member only — which is asked — and mode 0's players of roles 2 .. 4 are asked about mode 1,
    which does not seat them."""
    cfg = make_config([mode_team(5, 2, 200, (1, 1, 1, 1, 1), party_filter=True), mode_team(2, 2, 300, (1, 1))], capacity=2048)
    with RDuo(sorted_cls(engine_cls), oracle_cls, cfg) as d:
        rng = np.random.default_rng(5)
        n = 240
        role = rng.choice([0, 1, 1, 3, 3, 3], size=n)
        role[7] = 4
        party = rng.integers(0, 3, size=n)
        s = d.enqueue(rng.integers(900, 1400, size=n).astype(np.int32), cons_make(0, rng.integers(0, 2, size=n), party, role))
        m = 60
        there = d.enqueue(rng.integers(900, 1400, size=m).astype(np.int32),
                          cons_make(1, rng.integers(0, 2, size=m), rng.integers(0, 3, size=m), rng.integers(0, 2, size=m)))
        for when in ("before the ticks", "after the ticks"):
            got = partners_both(d, 0, s, tag="roles " + when)
            r = d.a.wait_route()
            assert r["route"] == MM_ROUTE_SORTED and r["passes"] == 6, r        # the rating's four, byte 40, the group's
            assert not got[1][:, [2, 5, 6, 7]].any() and got[1][:, 3].any()
            assert d.a.partners(0, s, by_role=False)[1] is None and d.a.wait_route()["passes"] == 6    # (the party filter's byte)
            got = partners_both(d, 0, s, None, 500, 0, "no filter " + when)
            assert d.a.wait_route()["passes"] == 6                              # no filter, but the role's byte
            if when == "before the ticks":
                assert got[1][7, 4] == 0 and (got[1][np.arange(n) != 7, 4] == 1).all()     # role 4's only member does not count itself
            d.a.partners(0, s, window=500, flags=0, by_role=False)
            assert d.a.wait_route()["passes"] == 5                              # neither: the extra pass is gone
            got = partners_both(d, 0, s, 1, 400, REGION | PARTY, "mode 0's players against mode 1 " + when)
            assert not got[1][:, 2:].any() and (got[0].any() or when != "before the ticks")
            partners_both(d, 1, there, 0, 400, REGION, "and mode 1's against mode 0 " + when)
            partners_both(d, 0, np.concatenate([s[::3], there[::2]]), None, 0xFFFFFFFF, PARTY, "a mixture " + when)
            if when == "before the ticks":
                d.cancel(0, s[5:9])
            partners_both(d, 0, s, tag="role 4's only member MARKED " + when)
            for md in (0, 1):
                d.tick(md, "roles")


# ---- 5. an empty table -------------------------------------------------------------------------------------------------

def empty_table(engine_cls, oracle_cls):
    """Nobody waits in in_mode; and everybody there is MARKED: zeros, MM_NO_SLOT, a table of no key."""
    with IfDuo(sorted_cls(engine_cls), oracle_cls, blocked_cfg(2)) as d:
        d.clock(100)
        here = d.enqueue(np.asarray([500, 500, 501], np.int32), cons_make([0, 0, 0]))
        for flags in (0, REGION):
            got = partners_both(d, 0, here, 1, 5, flags, "nobody waits in mode 1")
            assert not got[0].any() and not got[1].any() and (got[2] == NO_SLOT).all()
            assert d.a.wait_route()["keys"] == 0
        there = d.enqueue(np.asarray([500, 502], np.int32), cons_make([1, 1]))
        d.cancel(1, there)
        got = partners_both(d, 0, here, 1, 5, 0, "everybody in mode 1 is MARKED")
        assert not got[0].any() and (got[2] == NO_SLOT).all() and d.a.wait_route()["keys"] == 0
        got = partners_both(d, 1, there, 1, 5, 0, "and asked themselves")
        assert not got[0].any() and (got[2] == NO_SLOT).all() and d.a.wait_route()["keys"] == 0
        d.clock(200)
        assert d.expire_if(0, 50, rule(1, 5, 0, 1, MAX), "nobody has a partner there")[0].size == 0
        r = d.a.wait_route()
        assert (r["call"], r["route"], r["queries"], r["keys"]) == (2, MM_ROUTE_SORTED, 3, 0), r
        assert d.expire_if(0, 150, rule(1, 5, 0, 0, 0), "nobody is old enough")[0].size == 0
        assert d.a.wait_route()["route"] == MM_ROUTE_NONE and d.a.wait_route()["call"] == 2
        assert d.move_if(0, 1, 50, 0, rule(1, 5, 0, 0, 0), "everybody has none")[0].size == 3
        d.end("the ticks afterwards are the oracle's")


# ---- 6. the size rule --------------------------------------------------------------------------------------------------

def _pool_2048(d, old):
    """Exactly 2048 accepted players of distinct ratings in seven groups; the first `old` of them stamped 100, the rest 900."""
    n = 2048
    d.clock(1000)
    rating = (10 + np.random.default_rng(old).permutation(n)).astype(np.int32)
    cons, grp = cons_make(np.zeros(n)), (np.arange(n) % 7).astype(np.uint8)
    stamp = np.where(np.arange(n) < old, 100, 900).astype(np.uint32)
    sa, sb = d.a.enqueue_stamped(rating, cons, stamp, grp), d.b.enqueue(rating, cons, grp)
    assert np.array_equal(sa, sb) and (sa != NO_SLOT).all()
    d.tr.enqueued_rows(sa, rating, cons)
    d.tr.stamp[sa] = stamp
    return sa


def route_choice(engine_cls, oracle_cls):
    """wait_sort_mtests = 1 and a bound of 2048: 2^20 predicate tests are 512 queries — 511 go TILES, 512 go SORTED."""
    tuning = {"wait_sort_mtests": 1}
    with IfDuo(engine_cls, oracle_cls, one_group_cfg(8192), tuning) as d:
        s = _pool_2048(d, 0)
        cols = {}
        for nq, route in ((511, MM_ROUTE_TILES), (512, MM_ROUTE_SORTED)):
            cols[nq] = partners_both(d, 0, s[:nq], None, 9, 0, "%d queries" % nq)
            r = d.a.wait_route()
            assert (r["call"], r["route"], r["queries"], r["bound"], r["threshold"]) == (1, route, nq, 2048, 1), r
            assert r["keys"] == (2048 if route == MM_ROUTE_SORTED else 0) and r["passes"] == (6 if route == MM_ROUTE_SORTED else 0), r
        for c in range(3):
            assert np.array_equal(cols[511][c], cols[512][c][:511])
        d.a.partners(0, s[:0])
        assert d.a.wait_route() == dict(call=1, route=MM_ROUTE_NONE, queries=0, bound=0, threshold=0, keys=0, passes=0)
    for old, route in ((511, MM_ROUTE_TILES), (512, MM_ROUTE_SORTED)):
        with IfDuo(engine_cls, oracle_cls, one_group_cfg(8192), tuning) as d:
            _pool_2048(d, old)
            got = d.expire_if(0, 500, rule(0, 9, 0, 3, MAX), "%d old enough" % old)
            assert d.last["k1"] == old and 0 < got[0].size < old
            r = d.a.wait_route()
            assert (r["call"], r["route"], r["queries"], r["bound"], r["threshold"]) == (2, route, old, 2048, 1), r
            assert r["keys"] == (2048 if route == MM_ROUTE_SORTED else 0), r
            d.end()


# ---- 7. the two routes on one script -----------------------------------------------------------------------------------

def routes_agree(engine_cls, seed=1, rounds=6, first=500, batch=90, restart_at=(3,)):
    """A tiles engine and a sorted engine fed the same random script over four_mode_config — enqueue, cancel, move, the rule
    calls, rotate, tick, a snapshot restart — with questions in between: every column of every call is equal, and a
    question changes no byte of either snapshot."""
    cfg = four_mode_config(4096)
    rng = np.random.default_rng(seed)
    classes = (tiles_cls(engine_cls), sorted_cls(engine_cls))
    e = [c(cfg) for c in classes]
    asked = hits = 0

    def both(tag, call):
        out = [call(x) for x in e]
        flat = [[np.asarray(c) for c in (o if isinstance(o, tuple) else (o,)) if c is not None] for o in out]
        assert len(flat[0]) == len(flat[1]), tag
        for k, (x, y) in enumerate(zip(*flat)):
            assert np.array_equal(x, y), (tag, "column", k, x[:8], y[:8])
        return out[0]

    def question(tag):
        nonlocal asked, hits
        md, im = int(rng.integers(0, cfg.n_modes)), int(rng.integers(0, cfg.n_modes))
        q = rng.integers(0, cfg.capacity + 50, size=int(rng.integers(1, 700))).astype(np.uint32)
        window = [None, 0, int(rng.integers(1, 400)), 0xFFFFFFFF][int(rng.integers(0, 4))]
        flags = [None, 0, REGION, PARTY, REGION | PARTY][int(rng.integers(0, 5))]
        before = [x.snapshot() for x in e]
        assert before[0] == before[1], (tag, "the two engines' snapshots differ")
        got = both(tag, lambda x: x.partners(md, q, im, window, flags))
        assert [x.snapshot() for x in e] == before, (tag, "a question changed a snapshot")
        asked += 1
        hits += int(got[0].any())

    def drawn_rule():
        lo = int(rng.integers(0, 3))
        return rule(int(rng.integers(0, cfg.n_modes)), [None, 0, int(rng.integers(1, 400)), 0xFFFFFFFF][int(rng.integers(0, 4))],
                    [None, 0, REGION, PARTY][int(rng.integers(0, 4))], lo, [lo, lo + 5, MAX][int(rng.integers(0, 3))])

    try:
        now = 1000
        for rnd in range(rounds):
            now += int(rng.integers(1, 60))
            both("clock", lambda x: x.clock_set(now))
            rating, cons = random_batch(rng, cfg, first if rnd == 0 else int(rng.integers(0, batch + 1)))
            slots = both("enqueue", lambda x: x.enqueue(rating, cons))
            question("round %d after the enqueue" % rnd)
            cs = rng.choice(slots[slots != NO_SLOT], size=int(slots.size * 0.03), replace=False) if slots.size > 40 else slots[:0]
            both("cancel", lambda x: x.cancel(cs))
            question("round %d after the cancels" % rnd)
            r = drawn_rule()
            both("move_if", lambda x: x.move_if(2, 3, int(60 + 30 * rnd), ROLE_MASK, r))
            question("round %d after move_if" % rnd)
            r = drawn_rule()
            md = int(rng.integers(0, cfg.n_modes))
            both("expire_if", lambda x: x.expire_if(md, 150, r))
            question("round %d after expire_if" % rnd)
            r = drawn_rule()
            both("move_out_if", lambda x: x.move_out_if(0, 1, 120, 0, r))
            for md in range(cfg.n_modes):
                L = int(cfg.modes[md].teams * cfg.modes[md].team_size)
                both("rotate", lambda x: x.rotate(md, int(L - 1), 0))
                question("round %d mode %d after the rotation" % (rnd, md))
            if rnd in restart_at:
                for k, c in enumerate(classes):
                    blob = e[k].snapshot()
                    e[k].close()
                    e[k] = c(cfg)
                    e[k].restore(blob)
                question("round %d after the restore" % rnd)
            for md in range(cfg.n_modes):
                both("tick", lambda x: x.tick(md).slots)
            question("round %d after the ticks" % rnd)
    finally:
        for x in e:
            x.close()
    assert asked >= 6 * rounds and 4 * hits >= asked, (asked, hits)


# ---- 8. a failed allocation of the table -------------------------------------------------------------------------------

def release_on_failure(engine_cls, oracle_cls, shim):
    """The k-th allocation of a first call failing, for every k the call makes, on both routes of one engine
    (wait_sort_mtests = 1, a bound of 2048: 512 queries are sorted, 511 tiles): MM_ERR_OOM every time, the sorted call makes
    the table's four allocations more; the shim's live blocks are back where they were, the snapshot is the one from before,
    the record says NONE, and the next call succeeds on either route.  The same for a rule call whose table cannot be had."""
    shim.emu_live_blocks.restype = C.c_long
    shim.emu_fail_alloc_in.argtypes = [C.c_long]
    shim.emu_fail_alloc_in.restype = None
    tuning = {"wait_sort_mtests": 1}
    made = {}
    for nq in (512, 511):
        for k in range(1, 20):
            with IfDuo(engine_cls, oracle_cls, one_group_cfg(8192), tuning) as d:
                s = _pool_2048(d, 0)
                blob, base = d.a.snapshot(), shim.emu_live_blocks()
                out = np.zeros(nq, np.uint32)
                shim.emu_fail_alloc_in(k)
                try:
                    rc = d.a._fn("partners")(d.a._h, 0, 0, 9, 0, nq, s[:nq].ctypes.data_as(C.c_void_p), out.ctypes.data_as(C.c_void_p), None, None)
                finally:
                    shim.emu_fail_alloc_in(0)
                if rc == 0:
                    made[nq] = k - 1
                    break
                assert rc == MM_ERR_OOM, (nq, k, rc)
                assert shim.emu_live_blocks() == base, (nq, k, base, shim.emu_live_blocks())
                assert d.a.snapshot() == blob and d.a.wait_route()["route"] == MM_ROUTE_NONE, (nq, k)
                for n2, route in ((512, MM_ROUTE_SORTED), (511, MM_ROUTE_TILES)):
                    partners_both(d, 0, s[:n2], None, 9, 0, "after allocation %d of %d queries failed" % (k, nq))
                    assert d.a.wait_route()["route"] == route
    assert made[512] == made[511] + 4 and made[511] >= 2, made
    for k in (3, 4, 5, 6):                                          # the candidates' two buffers, then the table's four
        with IfDuo(engine_cls, oracle_cls, one_group_cfg(8192), tuning) as d:
            _pool_2048(d, 600)
            blob, base = d.a.snapshot(), shim.emu_live_blocks()
            n_sel = C.c_uint32(7)
            from microservice_matchmaking_amd._abi import MMPartnerRule
            r = MMPartnerRule(0, 9, 0, 3, MAX)
            shim.emu_fail_alloc_in(k)
            try:
                rc = d.a._fn("expire_if")(d.a._h, 0, 500, C.byref(r), C.byref(n_sel))
            finally:
                shim.emu_fail_alloc_in(0)
            assert rc == MM_ERR_OOM and n_sel.value == 0, (k, rc, n_sel.value)
            assert shim.emu_live_blocks() == base and d.a.snapshot() == blob, (k, base, shim.emu_live_blocks())
            assert d.a.wait_route()["route"] == MM_ROUTE_NONE
            got = d.expire_if(0, 500, rule(0, 9, 0, 3, MAX), "the retry")
            assert d.last["k1"] == 600 and got[0].size > 0 and d.a.wait_route()["route"] == MM_ROUTE_SORTED
            d.end()
