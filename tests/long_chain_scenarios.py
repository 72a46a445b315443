"""Moves, rotations and stamped enqueues in front of the LONG-chain walks: tests/test_long_chain.py runs these drivers on the
CPU shim's tiny geometry, tests/test_gpu_long_chain.py on the GPU at the product's (one case per process,
tests/long_chain_gpu_worker.py).

The other wait-layer scripts run at pool sizes where every chain is short, so the tick behind a move or a rotation is
walked by kp_late or k_walk.  Here the tick behind the call is the tiled pair path (kp_init .. kp_rounds / kp_round, then the
hand-over to kp_late), the team pass kernels on several chunks, or kt_late from the first pass — chosen through the sizes, which
all come from tests/geometry.py, and ASSERTED from mm_path_stats.  To the walk kernels a moved entry is an enqueued one and a
mark is a cancel; what these cases pin is the host's books behind the calls (live_upper, cancel_pending, the ring position,
h_state, tk_last_len) where they decide something: live_upper gates the tiled rounds (`bound >= PL_MAX`) and the team path
(`>= TT_MIN`) and sizes pair_open's buffers, tk_last_len decides whether kt_late takes a tick from its first pass.

The witness is the one of the other wait-layer files: the unchanged oracle cancels the old slots and enqueues the same rows
(move_if_scenarios.IfDuo), the lists come from numpy over the oracle's state, and after every step the states, the wait
statistics and every tick's lobbies and matched waits are compared.  Every driver prints one line of counters per tick it was
built for."""
from __future__ import annotations

import numpy as np

from helpers import assert_same_state
from microservice_matchmaking_amd._abi import NO_SLOT, cons_make
from microservice_matchmaking_amd.config import make_config, mode_1v1, mode_team
from move_if_scenarios import IfDuo, IfOwnerEngine, same_list
from move_scenarios import ROLE_MASK, bucket_lengths, pool, rewrite
from rotate_scenarios import MM_PATH_PAIR, MM_PATH_TEAM, RotOwnerEngine

ONE_GROUP = [(0, 5000, "all")]
REGION_BITS = 0xFF << 4                                     # MM_CONS_REGION's field
COUNTERS = ("pair_tiled_passes", "pair_rounds_launches", "pair_round_launches", "team_f_launches", "team_fc_launches",
            "team_late_launches")


def counters(tag, ps):
    """One line per tick a case was built for: which kernels ran it."""
    print("%s: paths %d %s" % (tag, ps["paths"], " ".join("%s=%d" % (k, ps[k]) for k in COUNTERS)))
    return ps


def block_length():
    """Rows per workgroup of the bucketing kernels a move's rows go through (BK_CHUNK; the small build does not scale it)."""
    return bucket_lengths()[1]


class LDuo(IfDuo):
    """IfDuo with the two plain routes of a move, each followed by the comparison of the whole state."""

    def move(self, from_mode, to_mode, max_age, cons_clear=0, tag=""):
        got = super().move(from_mode, to_mode, max_age, cons_clear, tag)
        assert_same_state(self.a, self.b, self.cfg, tag + " after mm_move")
        return got

    def move_out_stamped(self, from_mode, to_mode, max_age, cons_clear=0, tag=""):
        """mm_move_out, then mm_enqueue_stamped of its rows on the same engine: the move in two halves."""
        want = self.tr.expected_expiry(self.b, from_mode, max_age)
        s, g, a, rating, cons, stamp = self.a.move_out(from_mode, to_mode, max_age, cons_clear)
        same_list(tag, "move_out", want, (s, g, a))
        assert np.array_equal(rating, self.tr.rating[s]) and np.array_equal(stamp, self.tr.stamp[s]), (tag, "rows")
        assert np.array_equal(cons, rewrite(self.tr.cons[s], to_mode, cons_clear)), (tag, "constraint words")
        new = self.a.enqueue_stamped(rating, cons, stamp, g.astype(np.uint8)) if s.size else np.zeros(0, np.uint32)
        self._requeued(tag, from_mode, to_mode, cons_clear, s, g, new)
        return s, g, a, new

    def by(self, route):
        return {"move": self.move, "move_out+stamped": self.move_out_stamped}[route]


# ---- 1. a move into a 1v1 chain that the tiled pair path takes --------------------------------------------------------

PAIR_LENGTHS = {"PL_MAX-1": lambda geo: geo["PL_MAX"] - 1, "PL_MAX": lambda geo: geo["PL_MAX"],
                "3xPK_T+1": lambda geo: 3 * geo["PK_T"] + 1}
FILLER = 64


def strict_and_fallback(capacity):
    """A strict 1v1 (small window, region filter) and its fallback (wider window, no filter), one rating group."""
    return make_config([mode_1v1(window=5, region_filter=True), mode_1v1(window=25)], capacity=capacity, groups=ONE_GROUP,
                       default_group=0)


def pair_moved_in(engine_cls, oracle_cls, geo, which, route, wrapped):
    """The fallback's chain is preloaded and never ticked; the strict mode holds k old players — BK_CHUNK + 1, so the requeue
    crosses a block of the bucketing, or half the destination's length where that is shorter (the small build scales PL_MAX
    and not BK_CHUNK) — who all move, region bits cleared.  The source ticks first: its purge releases the k old slots and
    live_upper drops by them, to EXACTLY the destination's length n.  Then the destination ticks: with n = PL_MAX - 1 in
    kp_late alone, with n = PL_MAX and n = 3 x PK_T + 1 through the tiled rounds — a live_upper that missed the moved
    players would keep both on kp_late, one that kept the old slots would tile the first.  Then a second move into the
    leftovers and a second tick.
    wrapped: the pool ends k - FILLER / 2 slots behind the ring position, slot 0 holds a waiting player of the destination
    and slots 1 .. FILLER are free again (a filler that matched): the move's slots wrap and step over slot 0, so the host
    hands the device a slot LIST (d_in_sel) instead of a range."""
    n = PAIR_LENGTHS[which](geo)
    k = min(block_length() + 1, n // 2)
    k2 = 65
    pre = n - k
    tag = "pair_moved_in %s %s %s" % (which, route, "wrapped" if wrapped else "contiguous")
    capacity = 1 + FILLER + k + (pre - 1) + (k - FILLER // 2) if wrapped else n + k + 2 * k2 + 64
    with LDuo(engine_cls, oracle_cls, strict_and_fallback(capacity)) as d:
        d.clock(10)
        if wrapped:
            lone = d.enqueue(np.asarray([2500], np.int32), cons_make([1], [0]))
            assert lone.tolist() == [0]
            d.enqueue(np.full(FILLER, 100, np.int32), cons_make(np.zeros(FILLER), 7))
            assert len(d.tick(0, tag + ": the filler")) == FILLER // 2
            pre -= 1
        src = d.enqueue(*pool(k, 501, 0))
        d.enqueue(*pool(pre, 502, 1))
        first = int(src[0]) + k + pre                            # the ring position
        d.clock(100)
        s, g, a, new = d.by(route)(0, 1, 50, REGION_BITS, tag)
        assert np.array_equal(s, src) and (a == 90).all() and (new != NO_SLOT).all()
        assert (d.tr.cons[new] & REGION_BITS == 0).all()
        if wrapped:
            want = np.concatenate([np.arange(first, capacity), np.arange(1, 1 + FILLER // 2)])
            assert first + k > capacity and np.array_equal(new, want), (tag, new[:4], new[-4:], first, capacity)
        else:
            assert np.array_equal(new, np.arange(first, first + k)), (tag, new[:4], first)
        assert int(d.b.queue_depth(1)[0]) == n and np.array_equal(d.b.queue_slots(1, 0)[-k:], new)
        assert len(d.tick(0, tag + ": the source, first")) == 0
        m = d.tick(1, tag + ": the destination")
        ps = counters(tag + ", %d players" % n, d.a.path_stats())
        assert ps["paths"] == MM_PATH_PAIR and len(m) > n // 4, (tag, ps["paths"], len(m))
        if n < geo["PL_MAX"]:
            assert ps["pair_tiled_passes"] == 0, (tag, n, ps["pair_tiled_passes"])
        else:
            assert ps["pair_tiled_passes"] > 0, (tag, n, ps["pair_tiled_passes"])
        d.clock(200)
        src2 = d.enqueue(*pool(k2, 503, 0))
        d.clock(300)
        s2, _, a2, new2 = d.by(route)(0, 1, 50, REGION_BITS, tag + ", the second move")
        assert np.array_equal(s2, src2) and (a2 == 100).all() and (new2 != NO_SLOT).all()
        assert len(d.tick(0, tag + ": the source again")) == 0
        m2 = d.tick(1, tag + ": the leftovers and the second move")
        assert int(d.b.queue_depth(1)[0]) + 2 * len(m2) + d.b.lobby_state(1, 0)[0].size >= k2   # (an anchor nobody fits may hold them all up)
        d.end(tag + ": the last ticks")
        return n, k, len(m), len(m2)


# ---- 2. a rotation in front of a tiled pair tick ----------------------------------------------------------------------

def pair_rotated(engine_cls, oracle_cls, geo, tuning=None):
    """rotate_scenarios.pair_geometry with PL_MAX + PK_T / 2 players in the chain of rating group 0: the tick after the
    rotation runs the TILED rounds with the rotated seat among the marked entries they filter and the same player at the tail.
    tuning {"pair_persist": 0}: kp_round takes the batches launch by launch instead of kp_rounds."""
    per_chain = geo["PL_MAX"] + geo["PK_T"] // 2
    capacity = 1 << (per_chain + 64).bit_length()
    cfg = make_config([mode_1v1(window=25, region_filter=True)], capacity=capacity)
    tag = "pair_rotated %s" % (tuning or "default")
    with LDuo(engine_cls, oracle_cls, cfg, tuning) as d:
        d.clock(10)
        lone = d.enqueue(np.asarray([700, 1700], np.int32), cons_make(0, [9, 9]))     # a rare region: anchors of groups 0 and 1
        assert len(d.tick(0, "rare anchors")) == 0
        d.clock(500)
        d.enqueue(*pool(per_chain, 71, 0, hi=1499))
        d.enqueue(*pool(40, 72, 0, lo=1500, hi=1999))
        assert int(d.b.queue_depth(0)[0]) == per_chain
        (s, g, age, new), m = d.rotate(0, 1, 1, tag)
        ps = counters(tag + ", %d players" % per_chain, d.a.path_stats())
        # (how many lobbies is the oracle's business: an anchor nobody fits ends the chain's tick early, the reference's rule)
        assert s.tolist() == lone.tolist() and (age == 490).all() and len(m) > 0
        assert ps["paths"] == MM_PATH_PAIR and ps["pair_tiled_passes"] > 0, (tag, ps)
        if tuning and tuning.get("pair_persist") == 0:
            assert ps["pair_round_launches"] > 0 and ps["pair_rounds_launches"] == 0, (tag, ps)
        else:
            assert ps["pair_rounds_launches"] > 0, (tag, ps)
        d.rotate(0, 1, 1, tag + ", the leftovers")
        d.end(tag + ": the last ticks")
        return per_chain, len(m)


# ---- 3. a move into a 5v5 chain that the team pass kernels take on several chunks ---------------------------------------

def four_modes_one_group(capacity):
    """move_scenarios.four_mode_config's modes over ONE rating group: the players concentrate."""
    return make_config([mode_1v1(window=40, region_filter=True), mode_team(2, 3, 300, (1, 1)),
                        mode_team(5, 2, 200, (1, 1, 1, 1, 1)), mode_team(5, 2, 400, (5,))], capacity=capacity, groups=ONE_GROUP,
                       default_group=0)


# tuning -> what mm_path_stats must say of the destination's tick: the four tunings of helpers.ANCHOR_MOVES_PRODUCT
TEAM_TUNINGS = [
    ({}, lambda ps: ps["team_f_launches"] > 0 and ps["team_fc_launches"] == 0),
    ({"team_f2": 0}, lambda ps: ps["team_fc_launches"] > 0 and ps["team_f_launches"] == 0),
    ({"team_late": 0, "team_split": 0}, lambda ps: ps["team_f_launches"] > 0 and ps["team_late_launches"] == 0),
    ({"team_late0": 10**7}, lambda ps: ps["team_late_launches"] >= 1 and ps["team_build_launches"] >= 1),
]
TEAM_TUNING_IDS = ["default", "f2=0", "late=0-split=0", "late0=1e7"]


def team_moved_in(engine_cls, oracle_cls, geo, tuning, path_ok, clear=True):
    """Modes 2 -> 3 of four_mode_config (a five-role 5v5 into its role-free fallback with the wider window) in one rating
    group.  The destination is preloaded with TT_MIN + 2 x TT_CH + 1 players and never ticked; more than BK_CHUNK players
    move in; the source ticks first (its purge takes live_upper down by the old slots), then the destination: the team path
    on four chunks and more, in the kernels `tuning` stands for (never ticked, the whole chain counts as arrivals: only
    team_late0 = 10^7 lets kt_late take it from the first pass).
    clear=False: the role field stays, so the rows of roles 1 .. 4 — every row but each fifth, more than BK_CHUNK of them — are
    refused: NO_SLOT in the new column, expired only, their ring positions used up as the oracle's enqueue of the same rows
    uses them (the enqueue behind it must get the oracle's slots)."""
    pre = geo["TT_MIN"] + 2 * geo["TT_CH"] + 1
    bk = block_length()
    k = bk + 1 if clear else 5 * (bk // 4 + 1)
    tag = "team_moved_in %s %s" % (tuning or "default", "cleared" if clear else "roles kept")
    with LDuo(engine_cls, oracle_cls, four_modes_one_group(pre + 2 * k + 1024), tuning) as d:
        d.clock(10)
        d.enqueue(*pool(pre, 601, 3))
        rating, cons = pool(k, 602, 2)
        src = d.enqueue(rating, cons_make(2, (cons >> 4) & 0xFF, 0, np.arange(k) % 5))
        d.clock(100)
        s, g, a, new = d.move(2, 3, 50, ROLE_MASK if clear else 0, tag)
        assert np.array_equal(s, src) and (a == 90).all()
        refused = np.arange(k) % 5 >= 1
        if clear:
            assert (new != NO_SLOT).all() and d.a.last_move == {"selected": k, "refused": 0}
        else:
            assert np.array_equal(new == NO_SLOT, refused) and int(refused.sum()) > bk, (tag, int((new == NO_SLOT).sum()))
            assert d.a.last_move == {"selected": k, "refused": int(refused.sum())}, (tag, d.a.last_move)
        seated = int((new != NO_SLOT).sum())
        assert int(d.b.queue_depth(3)[0]) == pre + seated
        nxt = d.enqueue(*pool(37, 603, 3))                       # (LDuo.enqueue: the ring position is the oracle's)
        assert (nxt != NO_SLOT).all()
        assert len(d.tick(2, tag + ": the source, first")) == 0
        m = d.tick(3, tag + ": the destination")
        ps = counters(tag + ", %d players" % (pre + seated + 37), d.a.path_stats())
        assert ps["paths"] & MM_PATH_TEAM and len(m) > 0, (tag, ps["paths"], len(m))
        assert path_ok(ps), (tag, {c: ps[c] for c in COUNTERS + ("team_build_launches",)})
        d.end(tag + ": the last ticks")
        return pre + seated, len(m)


# ---- 4. the low-rate regime: a long standing 5v5 chain, a few arrivals, a rotation and a move every period ---------------

WIDE_GROUP = [(0, 10**6, "all")]
REGIME_PERIODS = 6


def regime_cfg(capacity):
    """A five-role 5v5 and its role-free fallback with the wider window, one rating group wide enough for lonely ratings."""
    return make_config([mode_team(5, 2, 200, (1, 1, 1, 1, 1)), mode_team(5, 2, 400, (5,))], capacity=capacity, groups=WIDE_GROUP,
                       default_group=0)


def late_only(ps):
    """kt_late took the tick from its first pass: no pass of kt_f or kt_fc on the critical chain."""
    return ps["paths"] & MM_PATH_TEAM and ps["team_late_launches"] >= 1 and ps["crit_team_f_passes"] == 0 and ps["crit_team_fc_passes"] == 0


def pass_kernels(ps):
    return ps["paths"] & MM_PATH_TEAM and ps["crit_team_f_passes"] + ps["crit_team_fc_passes"] >= 1


def team_stream_regime(engine_cls, oracle_cls, geo, tuning=None):
    """What run_stream(rotate=..., fallback=...) meets at a low rate.  Mode 0 holds TT_MIN + TT_CH players of roles 0 .. 3: no
    lobby can fill (patterns.role_missing's family), so the first tick leaves a short-handed stored lobby and tk_last_len.
    Mode 1, the fallback, holds as many players 101 rating points apart — seven within an anchor's window of 400, never ten,
    and the chain's rating span stays under the 2^19 the team path takes.  Then REGIME_PERIODS periods:
    the clock advances, 40 players arrive in mode 0 (roles 0 .. 4, so lobbies fill now and then) with three more whose ratings
    nobody is near, five players cancel, mode 0 rotates, mm_move_if moves who has waited a period and fits nobody
    ("nobody here fits me": the three) to the fallback, mm_expire_if drops the old ones without a close neighbour, both
    modes tick.  Each period's arrivals are far under team_late0, so with the default tuning kt_late takes the fallback's tick
    from its first pass in every period, behind a move-in (periods 1 .. 5: the arrivals of period p are old enough in period
    p + 1; asserted below) as without one — unless tk_last_len or live_upper lag.  Mode 0's tick behind a rotation is NOT
    kt_late's while the head of its queue is live, and cannot be: the rotation marks every seat of the stored lobby, so
    kt_init judges the live head against the stale lobby, and that head is the player the last tick — run to quiescence
    against the same seats — could not seat; it sits out, and team_walk turns late_ok off for a head that sat out
    (t.sitout).  Every period rotates (asserted), so for mode 0's ticks of the periods the pass kernels are pinned instead,
    and kt_late only where the head itself was marked by the period's cancels, move or expiry (the test's own table says
    which: at least one period of the first kind is required, the printed lines name them).
    Two more periods pin the threshold itself: exactly team_late0 arrivals (kt_late), then team_late0 + 1 (the pass kernels).
    tuning {"team_late0": 0}: the pass kernels take every tick; the caller compares the lobbies of the two runs.
    -> the lobbies of every tick."""
    n0 = geo["TT_MIN"] + geo["TT_CH"]
    tag = "team_stream_regime %s" % (tuning or "default")
    rng = np.random.default_rng(77)
    with LDuo(engine_cls, oracle_cls, regime_cfg(4 * n0 + 8192), tuning) as d:
        late0 = d.a.tuning()["team_late0"]
        now = 1000
        d.clock(now)
        d.enqueue(rng.integers(0, 5001, size=n0).astype(np.int32), cons_make(0, 0, 0, rng.integers(0, 4, size=n0)))
        d.enqueue((100_000 + 101 * np.arange(n0)).astype(np.int32), cons_make(np.ones(n0)))
        log = [d.tick(md, tag + ": the standing chains").slots.tolist() for md in (0, 1)]
        assert log == [[], []] and 1 <= d.b.lobby_state(0, 0)[0].size <= 8 and 1 <= d.b.lobby_state(1, 0)[0].size <= 9
        rotated_at, moved_at, sat_out_at = [], [], []
        for p in range(REGIME_PERIODS):
            now += 100
            d.clock(now)
            t = "%s, period %d" % (tag, p)
            rating = np.concatenate([rng.integers(0, 5001, size=40), 200_000 + 5000 * (3 * p + np.arange(3))]).astype(np.int32)
            d.enqueue(rating, cons_make(0, 0, 0, rng.integers(0, 5, size=43)))
            live0 = np.concatenate([d.tr.waiting(d.b, 0, 0)])
            d.cancel(0, rng.choice(live0, size=5, replace=False).astype(np.uint32))
            rot = d.rotate(0, 9, 1, t, tick=False)
            mv = d.move_if(0, 1, 50, ROLE_MASK, {"in_mode": 0, "window": 200, "flags": 0, "min_partners": 0, "max_partners": 0}, t)
            d.expire_if(0, 350, {"in_mode": 0, "window": 2, "flags": 0, "min_partners": 0, "max_partners": 0}, t)
            head_live = not d.tr.gone[0, d.b.queue_slots(0, 0)[0]]
            sat_out_at += [p] * bool(head_live and rot[0].size)
            for md in (0, 1):
                log.append(d.tick(md, "%s mode %d" % (t, md)).slots.tolist())
                ps = counters("%s mode %d (rotated %d, moved in %d)" % (t, md, rot[0].size, mv[0].size), d.a.path_stats())
                want = pass_kernels if not late0 or (md == 0 and rot[0].size and head_live) else late_only
                assert want(ps), (t, md, {c: ps[c] for c in COUNTERS + ("crit_team_f_passes", "crit_team_fc_passes")})
            rotated_at += [p] * (rot[0].size > 0)
            moved_at += [p] * (mv[0].size > 0)
        print("%s: rotated in periods %s, moved in %s, the head sat out in %s" % (tag, rotated_at, moved_at, sat_out_at))
        assert rotated_at == list(range(REGIME_PERIODS)) and moved_at == list(range(1, REGIME_PERIODS)), (tag, rotated_at, moved_at)
        assert sat_out_at, tag
        for extra, edge in ((0, late_only), (1, pass_kernels)):
            now += 100
            d.clock(now)
            n = engine_cls.tuning_defaults()["team_late0"] + extra
            d.enqueue(rng.integers(0, 5001, size=n).astype(np.int32), cons_make(0, 0, 0, rng.integers(0, 4, size=n)))
            log.append(d.tick(0, "%s, %d arrivals" % (tag, n)).slots.tolist())
            ps = counters("%s, %d arrivals and nothing else" % (tag, n), d.a.path_stats())
            assert (edge if late0 else pass_kernels)(ps), (tag, n, {c: ps[c] for c in COUNTERS + ("crit_team_f_passes", "crit_team_fc_passes")})
        d.end(tag + ": the last ticks")
        return log


def team_stream_regime_both(engine_cls, oracle_cls, geo):
    """The regime under the default tuning and with kt_late's first pass off: the same lobbies, tick for tick."""
    late, passes = team_stream_regime(engine_cls, oracle_cls, geo), team_stream_regime(engine_cls, oracle_cls, geo, {"team_late0": 0})
    assert late == passes and sum(len(x) for x in late) > 0
    return sum(len(x) for x in late)


# ---- 6. run_stream with a fallback rule and rotations over a chain the team path takes -----------------------------------

class LongOwnerEngine(IfOwnerEngine, RotOwnerEngine):
    """The host route an owner has today, with the rule of mm_move_if and the rotation: oracle plus numpy tables."""


STREAM_PERIODS, STREAM_TICK_MS, STREAM_LOW_RATE = 6, 100.0, 12


def stream_rule(n0):
    """At most two others within a window in which a chain of n0 / 2 players over 5000 rating points holds about six: a few
    in a hundred of the old enough move, at the shim's density as at the product's, and the chain stays the team path's."""
    return {"in_mode": 0, "window": max(1, 30000 // n0), "flags": 0, "min_partners": 0, "max_partners": 2}


def stream_long_schedule(n0, seed=9):
    """stream_schedule's tuples, built by hand: n0 arrivals in the first period, STREAM_LOW_RATE in each of the others."""
    rng = np.random.default_rng(seed)
    out = []
    for k in range(STREAM_PERIODS):
        t_open, t_close, n = k * STREAM_TICK_MS * 1e-3, (k + 1) * STREAM_TICK_MS * 1e-3, n0 if k == 0 else STREAM_LOW_RATE
        out.append((t_open, t_close, n, seed + 1 + k, np.sort(rng.uniform(t_open, t_close, size=n))))
    return out


def stream_long(engine_cls, oracle_cls, geo):
    """One run_stream on one rank: a five-role 5v5 with cfg-3's role weights (supports scarce: about half of a batch stays)
    and its role-free fallback, one rating group.  The first period brings 3 x TT_MIN + 2 x TT_CH players, so the chain the first tick
    starts with and the one it leaves are both the team path's; the other periods bring a dozen.  Every period whoever has
    waited 250 ms with at most two others within stream_rule's window moves to the fallback, and both modes run up to two rounds of
    rotate-then-tick.  The engine's run against LongOwnerEngine's — the host route on the oracle: digests, matched, moved,
    refused, rotated, rounds and the sorted waits.  The path is recorded per tick of mode 0: the first on the team path — in the
    pass kernels where the batch exceeds team_late0 (the product's geometry; the knob is not scaled, so whether the shim's
    batch exceeds it is read from the tuning) — and every tick of a later period that moved somebody out and rotated on the team path too."""
    from microservice_matchmaking_amd.sharding import ShardedSearch
    from microservice_matchmaking_amd.stream import run_stream
    from microservice_matchmaking_amd.synth import ROLE_WEIGHTS_5V5
    n0 = 3 * geo["TT_MIN"] + 2 * geo["TT_CH"]
    cfg = make_config([mode_team(5, 2, 500, (1, 1, 1, 1, 1)), mode_team(5, 2, 1000, (5,))], capacity=1 << (2 * n0 + 4096).bit_length(),
                      groups=ONE_GROUP, default_group=0)
    ticks = []

    class Recording(engine_cls):
        def tick(self, mode=0, *args, **kw):
            m = super().tick(mode, *args, **kw)
            if mode == 0:
                ticks.append(counters("stream_long tick %d of mode 0" % len(ticks), self.path_stats()))
            return m

    out = []
    for cls in (Recording, LongOwnerEngine):
        with ShardedSearch(cfg, cls, 0, 1) as s:
            out.append(run_stream(s, stream_long_schedule(n0), role_weights=ROLE_WEIGHTS_5V5, realtime=False,
                                  fallback=[(0, 1, 250, ROLE_MASK, stream_rule(n0))], rotate={"max_seated": [9, 9], "rounds": 2}))
    got, want = out
    for key in ("digests", "matched", "moved", "refused", "rotated", "rotate_rounds", "full_at_s"):
        assert got[key] == want[key], ("stream_long", key, got[key], want[key])
    assert all(np.array_equal(np.sort(x), np.sort(y)) for x, y in zip(got["wait_ms"], want["wait_ms"])), "stream_long wait_ms"
    assert got["matched"] > n0 // 4 and got["moved"][0] > 0 and got["rotated"][0] > 0 and got["full_at_s"] is None, \
        (got["matched"], got["moved"], got["rotated"])
    first_in_passes = n0 > engine_cls.tuning_defaults()["team_late0"]
    assert ticks[0]["paths"] & MM_PATH_TEAM and (ticks[0]["team_f_launches"] > 0) == first_in_passes, ticks[0]
    assert len(ticks) > STREAM_PERIODS and all(t["paths"] & MM_PATH_TEAM for t in ticks), [t["paths"] for t in ticks]
    return got["matched"], got["moved"], got["rotated"], got["rotate_rounds"]


# ---- 5. the random script at long-chain sizes --------------------------------------------------------------------------

TWO_GROUPS = [(0, 2499, "low"), (2500, 5000, "high")]
FALLBACKS = ((0, 4, REGION_BITS), (2, 3, ROLE_MASK))           # (strict mode, its fallback, what the move clears)


def five_mode_config(capacity):
    """move_scenarios.four_mode_config's modes plus mode 4, the 1v1's fallback (wider window, no filter), two rating groups."""
    return make_config([mode_1v1(window=40, region_filter=True), mode_team(2, 3, 300, (1, 1)),
                        mode_team(5, 2, 200, (1, 1, 1, 1, 1)), mode_team(5, 2, 400, (5,)), mode_1v1(window=80)],
                       capacity=capacity, groups=TWO_GROUPS)


def mode_counts(geo):
    """Players per mode of the first batch: two rating groups, so a little over twice the chain length each mode is to reach."""
    pair, team = geo["PL_MAX"] + geo["PK_T"], geo["TT_MIN"] + 2 * geo["TT_CH"]
    over = lambda n: 2 * n + n // 8 + 64
    return [over(pair), 2 * geo["TT_MIN"], over(team), over(team), over(geo["PL_MAX"])]


def players(rng, cfg, mode, n):
    roles = int(cfg.modes[mode].n_roles)
    return rng.integers(0, 5001, size=n).astype(np.int32), cons_make(mode, rng.integers(0, 3, size=n), 0, rng.integers(0, roles, size=n))


def mixed(rng, cfg, counts):
    """counts[mode] players of every mode in one shuffled batch."""
    parts = [players(rng, cfg, md, n) for md, n in enumerate(counts)]
    rating, cons = np.concatenate([p[0] for p in parts]), np.concatenate([p[1] for p in parts])
    order = rng.permutation(rating.size)
    return rating[order], cons[order]


def long_script(engine_cls, oracle_cls, geo, seed=1, rounds=3, restart_at=(), tuning=None, coverage=True):
    """move_if_scenarios.move_if_script's shape on IfDuo at long-chain sizes: five_mode_config, a first batch after which —
    before any tick, asserted — the longest chain of the strict 1v1 holds PL_MAX + PK_T entries, the longest of its fallback
    PL_MAX, and the longest of either 5v5 TT_MIN + 2 x TT_CH; later batches hold up to an eighth of it.  The first batch comes
    in two parts 30 ms apart, the older one BK_CHUNK + 200 players of the strict 1v1 and a quarter of that of the strict 5v5,
    and a round's age thresholds lie above the age of the round's own arrivals: a call selects the older part and the
    leftovers of earlier rounds, never tens of thousands at once (the numpy witness of the partner counts is quadratic).
    Round 0's moves take the whole older part (any partner count, a threshold under its age): that is when the fallbacks'
    chains are long, and BK_CHUNK + 200 rows go through the requeue at once.
    Per round: the clock, the batch, 2 % cancels, the clock again; from each strict mode to its fallback one of mm_move,
    mm_move_if and mm_move_out_if + mm_enqueue_stamped (the 5v5 every other time with the role field kept: refused rows);
    mm_expire_if with a drawn rule; mm_rotate of every mode; mm_locate and mm_partners on 64 drawn slots, the snapshot unchanged; every mode
    ticks.  restart_at: rounds before whose ticks A is dumped, created again and restored.  The decisions are drawn from a
    stream of their own, so a seed makes the same calls at the shim's sizes and at the product's.
    coverage: what the script must have covered, from the counters it summed — tiled pair passes and team pass-kernel launches
    in a fallback's tick of a round that moved somebody in, a kt_late launch, more than BK_CHUNK players moved, a refused
    row, a rotation that selected somebody.  (Off under a drawn tuning or force_generic: the paths are the tuning's.)
    -> the sums."""
    from locate_scenarios import locate_both
    from move_if_scenarios import ANYBODY, drawn_rule
    from partners_scenarios import partners_both
    counts = mode_counts(geo)
    first = sum(counts)
    cfg = five_mode_config(1 << (3 * first).bit_length())
    dec, dat = np.random.default_rng([seed, 1]), np.random.default_rng([seed, 2])
    bk = block_length()
    cov = {"tiled_after_move_in": 0, "team_passes_after_move_in": 0, "late_launches": 0, "moved": 0, "refused": 0,
           "rotations_selecting": 0, "rule_calls": 0, "lobbies": 0}
    tag0 = "long_script seed %d %s" % (seed, tuning or "")
    d = LDuo(engine_cls, oracle_cls, cfg, tuning)
    now = 1000
    try:
        for rnd in range(rounds):
            tag = "%s round %d" % (tag0, rnd)
            now += int(dec.integers(1, 60))
            d.clock(now)
            if rnd == 0:
                old = [bk + 200, 0, (bk + 200) // 4, 0, 0]
                d.enqueue(*mixed(dat, cfg, old))
                now += 30
                d.clock(now)
                d.enqueue(*mixed(dat, cfg, [c - o for c, o in zip(counts, old)]))
                depth = [int(d.b.queue_depth(md).max()) for md in range(5)]
                want = [geo["PL_MAX"] + geo["PK_T"], 0, geo["TT_MIN"] + 2 * geo["TT_CH"], geo["TT_MIN"] + 2 * geo["TT_CH"], geo["PL_MAX"]]
                assert all(x >= w for x, w in zip(depth, want)), (tag, depth, want)
            else:
                n = int(dec.integers(0, 1025)) * (first // 8) // 1024
                d.enqueue(*mixed(dat, cfg, np.bincount(dat.integers(0, 5, size=n), minlength=5).tolist()))
            live = d.tr.live_slots()
            cs = dat.choice(live, size=live.size // 50, replace=False)
            mode_of = np.full(int(cfg.capacity), -1, np.int64)
            for md in range(cfg.n_modes):
                for g in range(cfg.n_groups):
                    mode_of[d.b.lobby_state(md, g)[0]] = md
                    mode_of[d.b.queue_slots(md, g)] = md
            d.a.cancel(cs)
            d.b.cancel(cs)
            for md in range(cfg.n_modes):
                d.tr.marked(md, cs[mode_of[cs] == md])
            young = int(dec.integers(1, 20))
            now += young
            d.clock(now)
            moved_in = {}
            for src, dst, clear in FALLBACKS:
                kind, max_age, r = int(dec.integers(0, 3)), young + int(dec.integers(0, 60)), drawn_rule(dec, (src, dst))
                if rnd == 0:
                    max_age, r = young + max_age % 30, ANYBODY   # the whole older part, whichever the call: the chains are long NOW
                if src == 2 and (rnd + seed) % 2 == 0:
                    clear = 0                                    # the role field stays: roles 1 .. 4 are refused
                t = "%s %d -> %d" % (tag, src, dst)
                if kind == 0:
                    got = d.move(src, dst, max_age, clear, t)
                elif kind == 1:
                    got = d.move_if(src, dst, max_age, clear, r, t)
                else:
                    got = d.move_out_if(src, dst, max_age, clear, r if dec.integers(0, 2) else ANYBODY, t)
                cov["rule_calls"] += kind > 0
                seated = int((got[3] != NO_SLOT).sum())
                moved_in[dst] = seated
                cov["moved"] += seated
                cov["refused"] += int(got[0].size) - seated
            md = int(dec.integers(0, cfg.n_modes))
            d.expire_if(md, young + int(dec.integers(20, 200)), drawn_rule(dec, (md, (md + 1) % 5)), tag + " expire_if")
            cov["rule_calls"] += 1
            for md in range(cfg.n_modes):
                L = int(cfg.modes[md].teams * cfg.modes[md].team_size)
                got = d.rotate(md, int(dec.integers(1, L)), int(dec.integers(0, 3)), "%s mode %d" % (tag, md), tick=False)
                cov["rotations_selecting"] += int(got[0].size > 0)
            md = int(dec.integers(0, cfg.n_modes))
            q = np.concatenate([dat.choice(d.tr.live_slots(), size=48), dat.integers(0, int(cfg.capacity), size=16)]).astype(np.uint32)
            locate_both(d, md, q, tag + " locate")
            partners_both(d, md, q, tag=tag + " partners")
            if rnd in restart_at and getattr(d.a, "restartable", True):
                blob, clk = d.a.snapshot(), d.a.clock()
                d.a.close()
                d.a = engine_cls(cfg, tuning) if tuning else engine_cls(cfg)
                d.a.restore(blob)
                assert d.a.clock() == clk
                assert_same_state(d.a, d.b, cfg, "%s right after the restore" % tag)
            for md in range(cfg.n_modes):
                m = d.tick(md, "%s mode %d" % (tag, md))
                ps = d.a.path_stats()
                cov["lobbies"] += len(m)
                cov["late_launches"] += ps["team_late_launches"]
                if md == 4 and moved_in.get(4):
                    cov["tiled_after_move_in"] += counters("%s mode 4, %d moved in" % (tag, moved_in[4]), ps)["pair_tiled_passes"]
                if md == 3 and moved_in.get(3):
                    ps = counters("%s mode 3, %d moved in" % (tag, moved_in[3]), ps)
                    cov["team_passes_after_move_in"] += ps["team_f_launches"] + ps["team_fc_launches"]
            for md in range(cfg.n_modes):
                d.stats(md, tag + " after the ticks")
    finally:
        d.__exit__()
    print("%s covered %s" % (tag0, cov))
    if coverage:
        assert cov["tiled_after_move_in"] > 0 and cov["team_passes_after_move_in"] > 0 and cov["late_launches"] >= 1, cov
        assert cov["moved"] > bk and cov["refused"] >= 1 and cov["rotations_selecting"] >= 1, cov
    return cov
