"""The engine clock (include/mm_wait.h) on the CPU shim: arrival stamps, mm_expire / mm_expired, mm_wait_stats,
mm_matches_wait, the version-2 snapshot and the stream's ttl_ms.  The reference has no time-out on the search path and
sees queue depth only (Search.Worker.status/0, lib/search/worker.ex:115-117, :326-334); an expiry is an mm_cancel of
slots the device selects, so the unchanged oracle is the witness for all of it (tests/wait_scenarios.py).  The same
drivers run on the GPU in tests/test_gpu_wait.py."""
import struct

import numpy as np
import pytest

from emu_engine import EmuEngine, EmuEngineSmall
from helpers import assert_same_state
from microservice_matchmaking_amd import MMError
from microservice_matchmaking_amd._abi import cons_make
from microservice_matchmaking_amd.config import make_config, mode_1v1, mode_team
from microservice_matchmaking_amd.sharding import ShardedSearch
from microservice_matchmaking_amd.stream import run_stream, stream_schedule
from microservice_matchmaking_amd.synth import ROLE_WEIGHTS_5V5, make_pool
from wait_scenarios import (Tracker, assert_wait_stats, chunk_length, expire_both, expiry_script, three_mode_config,
                            tick_both)

MM_ERR_RANGE, MM_ERR_STATE, MM_ERR_INVALID_ARG = -8, -9, -1
ENGINES = [EmuEngine, EmuEngineSmall]


class Duo:
    """Engine A and oracle B driven alike, with the test's own stamp table."""

    def __init__(self, engine_cls, oracle_cls, cfg, tuning=None):
        self.cfg = cfg
        self.a = engine_cls(cfg, tuning) if tuning else engine_cls(cfg)
        self.b = oracle_cls(cfg)
        self.tr = Tracker(cfg)

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.a.close()
        self.b.close()

    def clock(self, now):
        self.a.clock_set(now)
        self.tr.clock_set(now)

    def enqueue(self, rating, cons):
        sa, sb = self.a.enqueue(rating, cons), self.b.enqueue(rating, cons)
        assert np.array_equal(sa, sb)
        self.tr.enqueued(sa)
        return sa

    def cancel(self, mode, slots):
        self.a.cancel(slots)
        self.b.cancel(slots)
        self.tr.marked(mode, slots)

    def expire(self, mode, max_age, tag=""):
        return expire_both(self.a, self.b, self.tr, mode, max_age, tag)

    def tick(self, mode=0, tag=""):
        m = tick_both(self.a, self.b, self.tr, mode, tag)
        assert_same_state(self.a, self.b, self.cfg, tag)
        return m

    def waiting(self, mode=0):
        return sum(self.tr.waiting(self.a, mode, g).size for g in range(self.cfg.n_groups))


def pool(n, seed, mode=0, n_roles=1, **kw):
    rng = np.random.default_rng(seed)
    rating = rng.integers(kw.get("lo", 0), kw.get("hi", 5000) + 1, size=n).astype(np.int32)
    return rating, cons_make(mode, rng.integers(0, 3, size=n), 0, rng.integers(0, n_roles, size=n))


# ---- 1. expiry equals cancel ---------------------------------------------------------------------------------------

@pytest.mark.parametrize("engine_cls", ENGINES, ids=lambda c: c.__name__)
@pytest.mark.parametrize("seed", [5, 6, 7])
def test_random_script_expiry_is_a_cancel_of_the_selected_slots(oracle_cls, engine_cls, seed):
    log = expiry_script(engine_cls, oracle_cls, seed=seed)
    assert sum(len(x[3]) for x in log if x[0] == "expired") > 100 and sum(len(x[3]) for x in log if x[0] == "tick") > 50


@pytest.mark.parametrize("engine_cls", ENGINES, ids=lambda c: c.__name__)
def test_everything_expires_then_nothing_is_left_to_expire(oracle_cls, engine_cls):
    with Duo(engine_cls, oracle_cls, three_mode_config()) as d:
        d.clock(100)
        for md, roles in ((0, 1), (1, 2), (2, 5)):
            d.enqueue(*pool(900, 10 + md, md, roles))
        for md in range(3):
            d.tick(md, "first tick")
        d.clock(101)
        for md in range(3):
            left = d.waiting(md)
            s, g, a = d.expire(md, 0, "everything")
            assert s.size == left > 0 and (a == 1).all() and (np.diff(g.astype(np.int64)) >= 0).all()
            s2, _, _ = d.expire(md, 0, "twice in a row")          # the second list is empty
            assert s2.size == 0
            assert len(d.tick(md, "after everything expired")) == 0
            assert d.waiting(md) == 0 and int(d.a.queue_depth(md).sum()) == 0


@pytest.mark.parametrize("engine_cls", ENGINES, ids=lambda c: c.__name__)
def test_nothing_expires_and_nothing_changes(oracle_cls, engine_cls):
    with Duo(engine_cls, oracle_cls, three_mode_config()) as d:
        d.clock(7)
        d.enqueue(*pool(1200, 3, 0))
        d.clock(5007)
        s, _, _ = d.expire(0, 5000, "age == max_age is not older than max_age")
        assert s.size == 0
        before = d.waiting(0)
        assert len(d.tick(0)) > 0 and d.waiting(0) < before


@pytest.mark.parametrize("engine_cls", ENGINES, ids=lambda c: c.__name__)
@pytest.mark.parametrize("mode,roles", [(0, 1), (2, 5)], ids=["1v1", "5v5"])
def test_stored_lobby_anchor_and_queue_head_expire(oracle_cls, engine_cls, mode, roles):
    """After a tick every group with an odd player out holds an anchor in its stored lobby and, where nobody fitted, a
    queue behind it.  The old players expire while a younger wave stays: the stored lobbies lose their seats (the
    stale-lobby rule decides what the first live attempt sees, docs/MATCH_CHECK.md section 4) and the queues their heads."""
    with Duo(engine_cls, oracle_cls, three_mode_config()) as d:
        d.clock(1000)
        d.enqueue(*pool(700, 21, mode, roles))
        d.tick(mode, "old wave")
        seated = np.concatenate([d.a.lobby_state(mode, g)[0] for g in range(7)])
        heads = [int(q[0]) for q in (d.a.queue_slots(mode, g) for g in range(7)) if q.size]
        assert seated.size > 0 and heads
        d.clock(1500)
        d.enqueue(*pool(700, 22, mode, roles))
        s, g, a = d.expire(mode, 499, "the old wave")
        assert set(seated.tolist()) <= set(s.tolist()) and set(heads) <= set(s.tolist()) and (a == 500).all()
        for grp in range(7):                                   # within a group: the stored lobby's seats first
            mine = s[g == grp]
            ls = d.b.lobby_state(mode, grp)[0]
            assert np.array_equal(mine[:ls.size], ls)
        d.tick(mode, "the young wave alone")
        d.clock(1501)
        d.tick(mode, "and once more")


@pytest.mark.parametrize("engine_cls", ENGINES, ids=lambda c: c.__name__)
def test_expire_and_cancel_overlap(oracle_cls, engine_cls):
    with Duo(engine_cls, oracle_cls, three_mode_config()) as d:
        d.clock(50)
        old = d.enqueue(*pool(800, 31, 1, 2))
        d.tick(1)
        d.clock(90)
        young = d.enqueue(*pool(300, 32, 1, 2))
        still = np.intersect1d(old, d.tr.live_slots())
        d.cancel(1, np.concatenate([still[::3], young[::5]]))  # some of the old give up by themselves first
        s, _, _ = d.expire(1, 10, "the rest of the old")
        assert set(s.tolist()) == set(still.tolist()) - set(still[::3].tolist())
        d.a.cancel(s[:50])                                     # cancelling the expired again changes nothing
        d.b.cancel(s[:50])
        d.tick(1, "after both")
        assert_wait_stats(d.a, d.tr, 1)


@pytest.mark.parametrize("engine_cls", ENGINES, ids=lambda c: c.__name__)
def test_ring_laps_and_a_reused_slot_carries_its_new_stamp(oracle_cls, engine_cls):
    cfg = make_config([mode_1v1(window=25, region_filter=True)], capacity=1024)
    rng = np.random.default_rng(4)
    with Duo(engine_cls, oracle_cls, cfg) as d:
        handed, seen = 0, set()
        reused = 0
        for t in range(40):
            d.clock(10 * t)
            n = int(rng.integers(100, 201))
            # (loners outside the band's own rating group: inside it one would be an anchor nobody fits and hold the chain up)
            rating = np.where(rng.random(n) < 0.97, rng.integers(2000, 2100, size=n),
                              rng.choice([rng.integers(0, 2000), rng.integers(2500, 5001)], size=n)).astype(np.int32)
            s = d.enqueue(rating, cons_make(0, rng.integers(0, 3, size=n), 0, 0))
            reused += len(seen & set(s.tolist()))
            seen |= set(s.tolist())
            handed += n
            if t % 2 == 1:
                d.expire(0, 60, "lap tick %d" % t)             # loners older than six periods leave
            d.tick(0, "lap tick %d" % t)
            assert_wait_stats(d.a, d.tr, 0, "lap tick %d" % t)
        assert handed > 3 * 1024 and reused > 1024


@pytest.mark.parametrize("engine_cls", ENGINES, ids=lambda c: c.__name__)
def test_clock_crosses_two_to_the_32(oracle_cls, engine_cls):
    with Duo(engine_cls, oracle_cls, three_mode_config()) as d:
        d.clock(0xFFFFFF00)
        d.enqueue(*pool(900, 41, 0))
        d.tick(0)
        d.clock(0xFFFFFFF0)
        d.enqueue(*pool(400, 42, 0))
        d.clock(0x00000010)                                    # 0x110 after the first wave, 0x20 after the second
        assert d.a.clock() == (0x10, True)
        s, _, a = d.expire(0, 0x20, "across the wrap")
        assert s.size > 0 and (a == 0x110).all()
        m = d.tick(0, "across the wrap")
        assert len(m) > 0
    log = expiry_script(engine_cls, oracle_cls, seed=9, clock0=0xFFFFFF00, step_max=120, rounds=6)
    assert any(x[0] == "expired" and x[3] for x in log)


@pytest.mark.parametrize("engine_cls", ENGINES, ids=lambda c: c.__name__)
def test_players_enqueued_before_the_first_clock_set_wait_from_then(oracle_cls, engine_cls):
    with Duo(engine_cls, oracle_cls, three_mode_config()) as d:
        d.enqueue(*pool(901, 51, 0))
        d.tick(0)
        assert d.a.clock() == (0, False)
        d.clock(4000)
        assert_wait_stats(d.a, d.tr, 0)
        assert sum(w["age_sum"] for w in d.a.wait_stats(0)) == 0 and sum(w["waiting"] for w in d.a.wait_stats(0)) == d.waiting(0) > 0
        d.clock(4100)
        d.enqueue(*pool(300, 52, 0))
        s, _, a = d.expire(0, 99, "whoever was there before the clock")
        assert s.size > 0 and (a == 100).all()
        d.tick(0)
    expiry_script(engine_cls, oracle_cls, seed=11, clock_from=3, rounds=7)


# ---- 2. kernel boundaries -------------------------------------------------------------------------------------------

@pytest.mark.parametrize("delta", [-1, 0, 1])
def test_selection_at_the_chunk_and_wave_edges(oracle_cls, delta):
    """One chain of B - 1, B, B + 1 players (B: queue entries per workgroup of the selection kernels).  A queue nobody
    has ticked is in arrival order, so what age selects is a prefix: prefixes that end on each side of a wave's and of
    the chunk's edge.  Then a single selected player anywhere — first, last, on each side of the edge — by cancelling
    everybody else first: the kernels still walk the cancelled entries and rank the one that is left."""
    B = chunk_length()
    n = B + delta
    cfg = make_config([mode_1v1(window=0)], capacity=2 * B + 64)
    rating = (np.arange(n) % 1400).astype(np.int32)           # all bronze: one chain
    cons = cons_make(np.zeros(n))
    for p in sorted({1, 63, 64, 65, B // 4 - 1, B // 4, B // 4 + 1, B - 1, B, B + 1, n} & set(range(1, n + 1))):
        with Duo(EmuEngine, oracle_cls, cfg) as d:
            d.clock(10)
            d.enqueue(rating[:p], cons[:p])
            d.clock(20)
            if p < n:
                d.enqueue(rating[p:], cons[p:])
            assert d.a.queue_depth(0).tolist() == [n, 0, 0, 0, 0, 0, 0]
            s, g, a = d.expire(0, 5, "prefix %d of %d" % (p, n))
            assert s.size == p and (g == 0).all() and (a == 10).all()
            d.tick(0, "prefix %d of %d" % (p, n))
    for p in sorted({0, 1, B - 2, B - 1, B, n - 1} & set(range(n))):
        with Duo(EmuEngine, oracle_cls, cfg) as d:
            d.clock(10)
            sl = d.enqueue(rating, cons)
            d.clock(20)
            d.cancel(0, np.delete(sl, p))
            s, g, a = d.expire(0, 5, "only %d of %d" % (p, n))
            assert s.tolist() == [int(sl[p])] and a.tolist() == [10]
            assert_wait_stats(d.a, d.tr, 0)
            d.tick(0, "only %d of %d" % (p, n))


# ---- 3. wait_stats ----------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("engine_cls", ENGINES, ids=lambda c: c.__name__)
def test_wait_stats_over_every_histogram_bucket(oracle_cls, engine_cls):
    """Waves enqueued at halving distances from the end: ages 2^31 - 1, 2^30 - 1, ..., 1, 0 land in buckets 31..0; checked against numpy
    over the same set after the enqueues, after pending cancels and after the ticks."""
    cfg = three_mode_config(capacity=16384)
    last = 5 + (1 << 31) - 1                                   # the clock at the end; wave k is 2^(31-k) - 1 old then, wave 31 new
    with Duo(engine_cls, oracle_cls, cfg) as d:
        for k in range(32):
            d.clock(last - ((1 << (31 - k)) - 1))
            for md, roles in ((0, 1), (2, 5)):
                d.enqueue(*pool(40 + k, 100 + 2 * k + md, md, roles, lo=0, hi=1499 if k % 2 else 5000))
        assert d.a.clock() == (last, True)
        for md in (0, 2):
            assert_wait_stats(d.a, d.tr, md, "before anything")
            st = d.a.wait_stats(md)
            hist = sum(w["hist"].astype(np.int64) for w in st)
            assert (hist[0:32] > 0).all() and hist[32] == 0 and max(w["oldest_age"] for w in st) == (1 << 31) - 1
            mine = np.concatenate([d.tr.waiting(d.a, md, g) for g in range(7)])[::4]
            d.cancel(md, mine)
            assert_wait_stats(d.a, d.tr, md, "pending cancels do not wait")
            d.tick(md)
            assert_wait_stats(d.a, d.tr, md, "after the tick")
        d.enqueue(*pool(100, 999, 0))
        st = d.a.wait_stats(0)
        assert sum(int(w["hist"][0]) for w in st) >= 100       # age 0: bucket 0


# ---- 4. matches_wait -------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("engine_cls", ENGINES, ids=lambda c: c.__name__)
@pytest.mark.parametrize("kind", ["pair", "team", "generic"])
def test_matches_wait_is_the_clock_minus_the_stamp(oracle_cls, engine_cls, kind):
    mode, roles = (0, 1) if kind != "team" else (2, 5)
    paths = {"pair": 2, "team": 4, "generic": 1}[kind]
    with Duo(engine_cls, oracle_cls, three_mode_config(), {"force_generic": 1} if kind == "generic" else None) as d:
        with pytest.raises(MMError) as ei:
            d.a.matches_wait()
        assert ei.value.status == MM_ERR_STATE
        seen = set()
        # (the full geometry leaves team chains under 4096 players to k_walk: its team case is one chain of 6000)
        big = kind == "team" and engine_cls is EmuEngine
        for t, n in enumerate((6000 if big else 1500, 600, 900, 5)):
            d.clock(1000 + 37 * t * t)
            d.enqueue(*pool(n, 60 + t, mode, roles, hi=1499 if big else 5000))
            m = d.tick(mode, "%s wave %d" % (kind, t))          # (tick_both compares every word)
            if t == 0:
                assert d.a.path_stats()["paths"] & paths
            w = d.a.matches_wait()
            seen |= set(np.unique(w).tolist())
            assert w.shape == m.slots.shape
        assert len(seen) > 2                                    # players of several waves were seated together


# ---- 5. snapshot -----------------------------------------------------------------------------------------------------

def _header(blob):
    magic, version, abi, header_bytes, capacity, n_groups, n_modes, n_chains, next_slot, cancel_pending, chain_bytes = \
        struct.unpack_from("<11I", blob, 0)
    return dict(version=version, header_bytes=header_bytes, capacity=capacity, n_chains=n_chains, chain_bytes=chain_bytes)


@pytest.mark.parametrize("engine_cls", ENGINES, ids=lambda c: c.__name__)
def test_stop_and_restore_in_the_middle_changes_nothing(oracle_cls, engine_cls):
    straight = expiry_script(engine_cls, oracle_cls, seed=13, stats=False)
    stopped = expiry_script(engine_cls, oracle_cls, seed=13, stats=False, restart_at=(1, 3, 4))
    assert straight == stopped and any(x[0] == "expired" and x[3] for x in straight)


def test_snapshot_versions(oracle_cls):
    cfg = three_mode_config()
    with EmuEngineSmall(cfg) as a, EmuEngineSmall(cfg) as c:
        a.enqueue(*pool(1000, 71, 0))
        a.tick(0)
        v1 = a.snapshot()
        h = _header(v1)
        queued = sum(int(a.queue_depth(md).sum()) for md in range(3))
        size_v1 = h["header_bytes"] + h["capacity"] + h["n_chains"] * h["chain_bytes"] + 12 * queued
        assert h["version"] == 1 and len(v1) == size_v1      # an engine that never set its clock: the snapshot it always wrote
        a.clock_set(77)
        v2 = a.snapshot()
        assert _header(v2)["version"] == 2 and len(v2) == size_v1 + 4 + 4 * h["capacity"]
        assert v2[h["header_bytes"]:size_v1] == v1[h["header_bytes"]:]    # the version-1 payload first, unchanged
        c.clock_set(5)
        c.restore(v1)                                          # a version-1 blob: the clock is off afterwards
        assert c.clock()[1] is False
        with pytest.raises(MMError) as ei:
            c.expire(0, 0)
        assert ei.value.status == MM_ERR_STATE
        c.restore(v2)
        assert c.clock() == (77, True)
        c.clock_set(80)
        s, _, age = c.expire(0, 0)
        assert s.size == queued + sum(c.lobby_state(0, g)[0].size for g in range(7)) and (age == 3).all()
        bad = bytearray(v2)
        bad[-3] ^= 1                                           # the stamps are under the checksum
        with pytest.raises(MMError):
            c.restore(bytes(bad))
        with pytest.raises(MMError):
            c.restore(v2[:-4])


def test_reset_keeps_the_clock(oracle_cls):
    with Duo(EmuEngineSmall, oracle_cls, three_mode_config()) as d:
        d.clock(300)
        d.enqueue(*pool(500, 81, 0))
        d.expire(0, 0)
        d.a.reset()
        d.b.reset()
        d.tr = Tracker(d.cfg)
        d.tr.clock_set(300)
        assert d.a.clock() == (300, True)
        with pytest.raises(MMError) as ei:                     # the list of an expiry before the reset is gone
            d.a._check(d.a._fn("expired")(d.a._h, 0, 1, None, None, None), "expired")
        assert ei.value.status == MM_ERR_RANGE
        d.enqueue(*pool(500, 82, 0))
        d.clock(310)
        s, _, a = d.expire(0, 9)
        assert s.size == 500 and (a == 10).all()
        d.tick(0)


# ---- 6. off means off -------------------------------------------------------------------------------------------------

def test_without_a_clock_every_wait_call_says_so():
    cfg = three_mode_config()
    with EmuEngine(cfg) as a:
        a.enqueue(*pool(300, 91, 0))
        a.tick(0)
        assert a.clock() == (0, False)
        for call in (lambda: a.expire(0, 10), lambda: a.wait_stats(0), lambda: a.matches_wait()):
            with pytest.raises(MMError) as ei:
                call()
            assert ei.value.status == MM_ERR_STATE
        a.clock_set(1000)
        a.clock_set(1000)                                      # standing still is not going backwards
        with pytest.raises(MMError) as ei:
            a.clock_set(999)
        assert ei.value.status == MM_ERR_RANGE and a.clock() == (1000, True)
        with pytest.raises(MMError) as ei:
            a.clock_set(1000 + (1 << 31))                      # half the ring ahead reads as behind
        assert ei.value.status == MM_ERR_RANGE
        a.clock_set(1000 + (1 << 31) - 1)
        for call in (lambda: a.expire(3, 10), lambda: a.wait_stats(3)):
            with pytest.raises(MMError) as ei:
                call()
            assert ei.value.status == MM_ERR_INVALID_ARG
        s, g, age = a.expire(0, 0)
        assert s.size > 0
        for first, count in ((s.size, 1), (0, s.size + 1), (s.size + 1, 0)):
            assert a._fn("expired")(a._h, first, count, None, None, None) == MM_ERR_RANGE
        assert a._fn("expired")(a._h, s.size, 0, None, None, None) == 0
        assert a._fn("matches_wait")(a._h, 0, 1, None) == MM_ERR_RANGE    # the last tick ran before the clock was set


def test_a_poisoned_engine_answers_state(oracle_cls):
    cfg = three_mode_config()
    with EmuEngine(cfg, {"fail_tick": 1}) as a:
        a.clock_set(1)
        a.enqueue(*pool(300, 92, 0))
        with pytest.raises(MMError):
            a.tick(0)
        for call in (lambda: a.expire(0, 0), lambda: a.wait_stats(0), lambda: a.clock_set(2), lambda: a.matches_wait()):
            with pytest.raises(MMError) as ei:
                call()
            assert ei.value.status == MM_ERR_STATE
        assert a._fn("expired")(a._h, 0, 0, None, None, None) == MM_ERR_STATE
        a.reset()
        a.clock_set(2)
        assert a.expire(0, 0)[0].size == 0


# ---- 7. the stream ------------------------------------------------------------------------------------------------------

STREAM = dict(qps=20_000, seconds=0.6, tick_ms=10.0, seed=5)
TTL_MS = 50


def _starving(cls, ttl_ms):
    cfg = make_config([mode_team(5, 2, 50, (1, 1, 1, 1, 1))], capacity=1 << 14)
    sched = stream_schedule(STREAM["qps"], STREAM["seconds"], STREAM["tick_ms"], STREAM["seed"])
    with ShardedSearch(cfg, cls, 0, 1) as s:
        res = run_stream(s, sched, role_weights=ROLE_WEIGHTS_5V5, realtime=False, ttl_ms=ttl_ms)
        seated = sum(len(s.engine.lobby_state(0, g)[0]) for g in range(7))
    periods = int(TTL_MS / STREAM["tick_ms"]) + 1              # arrivals within the TTL plus one period
    n = np.array([x[2] for x in sched])
    bound = int(max(n[max(0, k - periods + 1):k + 1].sum() for k in range(len(n))))
    return res, seated, bound


def test_starving_stream_without_a_ttl_outgrows_the_bound(oracle_cls):
    """cfg-3's role weights give 10 % supports for 20 % of the seats: the 5v5 stream has no steady state.
    On the oracle alone: the backlog passes what a TTL would allow."""
    res, _, bound = _starving(oracle_cls, None)
    assert "expired" not in res and "wait_ms" not in res
    assert int(res["depth"][0].sum()) > 2 * bound


def test_starving_stream_with_a_ttl_stays_bounded(oracle_cls):
    res, seated, bound = _starving(EmuEngineSmall, TTL_MS)
    assert res["full_at_s"] is None and res["expired"][0] > 0
    assert res["depth_max"][0] <= bound                        # whoever is left arrived within the TTL plus one period
    assert int(res["depth"][0].sum()) + seated + res["matched"] + res["expired"][0] == res["ingested"]
    w = res["wait_ms"][0]
    assert w.size == res["matched"] > 0 and w.max() <= TTL_MS and (w % STREAM["tick_ms"] == 0).all()
    # the engine's figure next to the stream's own: a player stamped at the end of its period waited floor - (what was
    # left of that period when it arrived), so floor is never less and less than a period more
    fl = res["floor"][0] * 1e3
    assert (fl - w >= -1e-6).all() and (fl - w < STREAM["tick_ms"] + 1e-6).all()
