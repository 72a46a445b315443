"""Configurations past the reference's seven rating groups: 9-16 groups, tables that are not contiguous and ascending,
up to 16 modes (256 (mode, group) chains), rating spans and windows at the edges of the packed key, and team sums far
enough apart that the score needs more than 32 bits.  Every engine run is compared with the oracle bit for bit
(assert_same_tick / assert_same_state) and every emitted score with the exact reference (helpers.exact_scores).

CPU tier: the oracle, the literal restatement (oracle/literal_ref.py), the fiber-shim builds of the kernel source
(EmuEngine: product geometry, EmuEngineSmall: tiny tiles) and the host-side group decision of libmm_engine.so.
GPU tier (`-m gpu`): the same scenarios on the device, at sizes that reach the tiled pair path and the team path."""
import contextlib
import ctypes as C
import math
import os
import re

import numpy as np
import pytest

from emu_engine import EmuEngine, EmuEngineSmall
from helpers import assert_exact_scores, assert_same_state, assert_same_tick, exact_scores
from microservice_matchmaking_amd import MMError
from microservice_matchmaking_amd._abi import NO_SLOT, cons_make, decode_players
from microservice_matchmaking_amd.config import make_config, mode_1v1, mode_team
from oracle.literal_ref import find_rating_group_by_rating, team_name
from test_oracle_literal import MODE_SETS, literal_stage, literal_tick, to_payload

I32_MIN, I32_MAX = -2 ** 31, 2 ** 31 - 1
KEY_SPAN = 1 << 19                                  # a fast pair chain's rating span must stay below this (packed key)


def named(rows):
    return [(int(a), int(b), "g%d" % i) for i, (a, b) in enumerate(rows)]


_GAPPED = [(0, 999), (1500, 1999), (2500, 2999), (4000, 5000)]
# name -> (rows, default_group or None for make_config's div(n, 2) + 1)
TABLES = {
    "contiguous16": ([(1000 * i, 1000 * i + 999) for i in range(16)], None),
    "nine": ([(0, 499)] + [(500 * i, 500 * i + 499) for i in range(1, 8)] + [(4000, 5000)], None),
    "overlapping": ([(0, 2000), (1500, 2500), (1000, 1200), (2400, 5000), (-100, 6000)], None),
    "gaps_default0": (_GAPPED, 0),
    "gaps_default_last": (_GAPPED, len(_GAPPED) - 1),
    "negative": ([(-5000, -2001), (-2000, -1), (0, 0), (1, 3000)], None),
    "all_int32": ([(I32_MIN, I32_MAX)], None),
    "single_points": ([(1500, 1500), (1501, 1501), (0, 1499), (1502, 5000), (2000, 2000)], None),
    "from_gt_to": ([(0, 1999), (3000, 2000), (2000, 5000)], None),
}


def table_cfg(name, modes, capacity=4096):
    rows, dflt = TABLES[name]
    groups = named(rows)
    return make_config(modes, capacity=capacity, groups=groups, default_group=dflt), groups


def literal_group(groups, cfg, r):
    """Index of the group find_rating_group_by_rating picks, with the configuration's default mapped through."""
    g = find_rating_group_by_rating(r, groups, groups[cfg.default_group])
    return groups.index(g)


def edge_ratings(groups):
    """Every from - 1, from, to, to + 1 and INT32_MIN / MAX, as Python ints (some outside int32)."""
    pts = {I32_MIN, I32_MAX}
    for lo, hi, _ in groups:
        pts |= {lo - 1, lo, hi, hi + 1}
    return sorted(pts)


def groups_pool(rng, groups, per_group, regions=4, width=None):
    """per_group players inside each group's range (a `width`-wide band at its start if given), arrival order mixed."""
    rating = np.concatenate([rng.integers(lo, (hi if width is None else min(hi, lo + width - 1)) + 1, size=per_group)
                             for lo, hi, _ in groups]).astype(np.int32)
    rating = rating[rng.permutation(rating.size)]
    return rating, cons_make(0, rng.integers(0, regions, size=rating.size), 0, 0)


def run_ticks(a, b, cfg, batches, rng, tag, cancel=0, rating_of=None, modes=None):
    """Enqueue each (rating, cons) batch on both, cancel `cancel` waiting players from the second batch on, tick every
    mode (or `modes`), compare tick by tick and the whole state.  Returns the path stats of the first tick per mode."""
    rating_of = {} if rating_of is None else rating_of
    live = np.zeros(0, np.uint32)
    first = {}
    for k, (rating, cons) in enumerate(batches):
        sa, sb = a.enqueue(rating, cons), b.enqueue(rating, cons)
        assert np.array_equal(sa, sb), (tag, "slots", k)
        ok = sa != NO_SLOT
        rating_of.update(zip(sa[ok].tolist(), rating[ok].tolist()))
        live = np.concatenate([live, sa[ok]])
        if k and cancel and live.size > cancel:
            cs = rng.choice(live, size=cancel, replace=False)
            a.cancel(cs)
            b.cancel(cs)
            live = np.setdiff1d(live, cs)
        for md in (range(cfg.n_modes) if modes is None else modes):
            ma, mb = a.tick(md), b.tick(md)
            t = "%s batch %d mode %d" % (tag, k, md)
            assert_same_tick(ma, mb, t)
            assert_exact_scores(ma, cfg.modes[md], rating_of, t)
            assert_exact_scores(mb, cfg.modes[md], rating_of, t)
            if k == 0 and hasattr(a, "path_stats"):
                first[md] = a.path_stats()
            live = np.setdiff1d(live, ma.slots.ravel())
        assert_same_state(a, b, cfg, "%s batch %d" % (tag, k))
    return first


# ---- 1. the score: team sums 2^31 and more apart ------------------------------------------------------------------

WRAP_MODE = mode_team(2, 2, 0x3FFFFFFF, (1, 1))
WRAP_GROUPS = [(I32_MIN, I32_MAX, "all")]
WRAP_RATING = np.array([0, 2 ** 30 - 1, -(2 ** 30 - 1), 2 ** 30 - 1], np.int32)
WRAP_ROLE = np.array([0, 0, 1, 1])


def check_wrap_repro(eng):
    """Lobby [0, 2 | 1, 3]: team sums -1 073 741 823 and 2 147 483 646, score 1 610 612 734.5 -> 1 610 612 736.0 in f32
    (a 32-bit difference wrapped it to -536 870 912.0)."""
    slots = eng.enqueue(WRAP_RATING, cons_make(0, 0, 0, WRAP_ROLE))
    assert slots.tolist() == [0, 1, 2, 3]
    m = eng.tick(0)
    assert m.slots.tolist() == [[0, 2, 1, 3]]
    assert m.score.view(np.uint32)[0] == np.float32(1610612736.0).view(np.uint32), float(m.score[0])
    assert_exact_scores(m, WRAP_MODE, dict(enumerate(WRAP_RATING.tolist())), "wrap repro")


def test_exact_score_reference_rounds_once_to_nearest_even():
    from fractions import Fraction
    from helpers import f32_nearest
    assert f32_nearest(Fraction(3221225469, 2)) == np.float32(1610612736.0)
    assert f32_nearest(Fraction(2 ** 24 + 1)) == np.float32(2 ** 24)            # a tie: to the even mantissa
    assert f32_nearest(Fraction(2 ** 24 + 3)) == np.float32(2 ** 24 + 4)
    assert f32_nearest(Fraction(2 ** 24 + 3, 3) * 3) == np.float32(2 ** 24 + 4)
    assert f32_nearest(Fraction(1, 3)) == np.float32(1) / np.float32(3)
    got = exact_scores(np.array([[0, 2, 1, 3]]), WRAP_MODE, dict(enumerate(WRAP_RATING.tolist())))
    assert got.view(np.uint32)[0] == np.float32(1610612736.0).view(np.uint32)


@pytest.mark.parametrize("which", ["oracle", "emu"])
def test_score_of_team_sums_2_31_apart(oracle_cls, which):
    cfg = make_config([WRAP_MODE], capacity=64, groups=WRAP_GROUPS)
    with (oracle_cls(cfg) if which == "oracle" else EmuEngine(cfg)) as eng:
        check_wrap_repro(eng)


def wide_team_scores(a, b, n, seed):
    """One 2v2 chain of n players whose ratings fill +-(2^30 - 1) under the widest window.  Engine vs oracle, scores
    exact; returns the largest difference of team sums among the lobbies (the wrap needs 2^31 or more)."""
    cfg = a.cfg
    rng = np.random.default_rng(seed)
    rating = rng.integers(-(2 ** 30 - 1), 2 ** 30, size=n).astype(np.int32)
    cons = cons_make(0, 0, 0, rng.integers(0, 2, size=n))
    sa, sb = a.enqueue(rating, cons), b.enqueue(rating, cons)
    assert np.array_equal(sa, sb)
    rating_of = dict(zip(sa.tolist(), rating.tolist()))
    ma, mb = a.tick(0), b.tick(0)
    assert_same_tick(ma, mb, "wide team scores")
    assert_exact_scores(ma, cfg.modes[0], rating_of, "wide team scores")
    assert_exact_scores(mb, cfg.modes[0], rating_of, "wide team scores")
    assert_same_state(a, b, cfg, "wide team scores")
    return max(abs(sum(rating_of[int(s)] for s in r[:2]) - sum(rating_of[int(s)] for s in r[2:])) for r in ma.slots)


def test_score_of_team_sums_2_31_apart_on_a_long_chain(oracle_cls):
    """The same on a chain long enough for the team path of the tiny-geometry shim build (TT_MIN = 64)."""
    cfg = make_config([mode_team(2, 2, 0x3FFFFFFF, (1, 1))], capacity=4096, groups=WRAP_GROUPS)
    with EmuEngineSmall(cfg) as a, oracle_cls(cfg) as b:
        assert wide_team_scores(a, b, 600, 5) >= 2 ** 31


# ---- 2. the oracle against the literal restatement on custom tables -----------------------------------------------

def literal_script(oracle_cls, tname, mset, seed, rounds=4):
    """test_oracle_matches_literal_chain_by_chain's script on a custom group table (one literal stage per mode: Mode R's
    per-chain tick), ratings near every group's edges: emissions, passes, pair counts and stored lobbies."""
    rng = np.random.default_rng(seed)
    cfg, groups = table_cfg(tname, MODE_SETS[mset])
    eng = oracle_cls(cfg)
    stages = [literal_stage(cfg, groups) for _ in range(cfg.n_modes)]
    edges = [r for r in edge_ratings(groups) if I32_MIN <= r <= I32_MAX]
    live = []
    try:
        for rnd in range(rounds):
            n = int(rng.integers(40, 200))
            centre = np.asarray(edges)[rng.integers(0, len(edges), size=n)].astype(np.int64)
            rating = np.clip(centre + rng.integers(-60, 61, size=n), I32_MIN, I32_MAX).astype(np.int32)
            mode = rng.integers(0, cfg.n_modes, size=n)
            role = np.array([rng.integers(0, cfg.modes[int(m)].n_roles) for m in mode])
            cons = cons_make(mode, rng.integers(0, 2, size=n), rng.integers(0, 2, size=n), role)
            slots = eng.enqueue(rating, cons)
            for s, r, c in zip(slots, rating, cons):
                stages[int(c) & 0xF].deliver(to_payload(s, r, c))
            live.extend(slots.tolist())
            if rnd > 0 and live:
                cs = rng.choice(np.asarray(live), size=max(1, len(live) // 10), replace=False)
                eng.cancel(cs.astype(np.uint32))
                for s in cs:
                    for st in stages:
                        st.cancel(int(s))
                live = [s for s in live if s not in set(cs.tolist())]
            for mode_i in range(cfg.n_modes):
                pairs0 = stages[mode_i].pairs
                lit = literal_tick(stages[mode_i], cfg, groups)
                m = eng.tick(mode_i)
                got = [(int(g), int(p), s.tolist()) for g, p, s in zip(m.group, m.pass_, m.slots)]
                assert got == lit[mode_i], (tname, mset, seed, rnd, mode_i)
                assert m.stats["pairs"] == stages[mode_i].pairs - pairs0, (tname, mset, seed, rnd, mode_i, "pairs")
                gone = set(m.slots.ravel().tolist())
                live = [s for s in live if s not in gone]
                for gi, g in enumerate(groups):
                    want = []
                    for rec in stages[mode_i].lobbies.tables[g[2]]:
                        if rec[2] == "mode%d" % mode_i:
                            want = [p["id"] for t in range(cfg.modes[mode_i].teams) for p in rec[1].get(team_name(t), [])]
                    s, _ = eng.lobby_state(mode_i, gi)
                    assert s.tolist() == want, (tname, mset, seed, rnd, mode_i, gi)
    finally:
        eng.close()


@pytest.mark.parametrize("tname", sorted(TABLES))
@pytest.mark.parametrize("mset", ["1v1_region", "5v5_roles", "mixed"])
def test_oracle_matches_literal_on_custom_group_tables(oracle_cls, tname, mset):
    for seed in (1, 2):
        literal_script(oracle_cls, tname, mset, seed)


# ---- 3. one group decision everywhere ------------------------------------------------------------------------------

def _find_group(lib, fn, cfg, x):
    g = C.c_uint32(0xFFFF)
    f = getattr(lib, fn)
    f.argtypes = [C.POINTER(type(cfg)), C.c_double, C.POINTER(C.c_uint32)]
    f.restype = C.c_int
    assert f(C.byref(cfg), float(x), C.byref(g)) == 0
    return int(g.value)


@pytest.mark.parametrize("tname", sorted(TABLES))
def test_find_rating_group_agrees_with_the_literal_rule(oracle_cls, tname):
    """mm_find_rating_group (libmm_engine.so, host side), mo_find_rating_group (the oracle) and the shim build, on every
    edge of the table, the edges +-0.5, INT32_MIN/MAX and beyond, -0.0 and NaN."""
    from microservice_matchmaking_amd.engine import load_library
    cfg, groups = table_cfg(tname, [mode_1v1()])
    xs = []
    for r in edge_ratings(groups):
        xs += [float(r), r - 0.5, r + 0.5]
    xs += [-0.0, 2.0 ** 31, -(2.0 ** 31) - 1, 1e300, -1e300]
    with EmuEngine(cfg) as emu:
        emu_lib = emu._lib
    libs = [(load_library(), "mm_find_rating_group"), (oracle_cls._lib, "mo_find_rating_group"),
            (emu_lib, "mm_find_rating_group")]
    for x in xs:
        want = literal_group(groups, cfg, x)
        for lib, fn in libs:
            assert _find_group(lib, fn, cfg, x) == want, (tname, fn, x, want)
    for lib, fn in libs:
        assert _find_group(lib, fn, cfg, math.nan) == cfg.default_group, (tname, fn)


def bucketing_matches_the_literal_rule(engine_cls, tname):
    """Players at every edge (int32 ones), enqueued without a group override: each (mode 0, group) queue holds
    exactly the players whose group the literal rule picks, in arrival order."""
    cfg, groups = table_cfg(tname, [mode_1v1(window=0, region_filter=True)])
    pts = [r for r in edge_ratings(groups) if I32_MIN <= r <= I32_MAX]
    rating = np.asarray(pts * 2, np.int64).astype(np.int32)
    cons = cons_make(0, np.arange(rating.size) % 256, 0, 0)
    with engine_cls(cfg) as eng:
        slots = eng.enqueue(rating, cons)
        want = [literal_group(groups, cfg, int(r)) for r in rating]
        for g in range(len(groups)):
            got = eng.queue_slots(0, g).tolist()
            assert got == [int(s) for s, w in zip(slots, want) if w == g], (tname, g)
        assert eng.queue_depth(0).tolist() == [want.count(g) for g in range(len(groups))], tname


@pytest.mark.parametrize("tname", sorted(TABLES))
def test_bucketing_matches_the_literal_rule(oracle_cls, tname):
    bucketing_matches_the_literal_rule(oracle_cls, tname)
    bucketing_matches_the_literal_rule(EmuEngine, tname)


@pytest.mark.parametrize("tname", sorted(TABLES))
def test_codec_group_column_matches_the_literal_rule(tname):
    """mm_decode_players' group column for JSON numbers written every way: integers at each edge, .5 steps, exponent
    forms, -0.0, and integers outside int32."""
    import json
    from microservice_matchmaking_amd.engine import load_library
    cfg, groups = table_cfg(tname, [mode_1v1()])
    texts = ["1499.5", "1.5e3", "1.5E+3", "-0.0", "0.0", "2147483648", "-2147483649", "2147483647.5", "-2147483648.5",
             "1e10", "-1e10", "4999.999", "-0.5"]
    for r in edge_ratings(groups):
        texts += [str(r), "%d.5" % r, "%de0" % r]
    msgs = [b'{"game-mode":"m","rating":' + t.encode() + b'}' for t in texts]
    out = decode_players(load_library(), cfg, ["m"], msgs)
    for t, g in zip(texts, out["group"]):
        assert int(g) == literal_group(groups, cfg, json.loads(t)), (tname, t, int(g))


# ---- 4. more than eight tiled chains / 5. team path on 16 groups / 7. span and key edges (shim and device) ---------

def contiguous(n, width=2000):
    return [(width * i, width * i + width - 1, "g%d" % i) for i in range(n)]


def many_chains_pair(engine_cls, oracle_cls, n_groups, per_group, extra, tuning=None, seed=1):
    """1v1 +-25 with the region filter on n_groups contiguous groups, per_group players each, then `extra` arrivals per
    group and cancels for two more ticks.  Returns the path stats of the first tick."""
    groups = contiguous(n_groups)
    cfg = make_config([mode_1v1(window=25, region_filter=True)], capacity=1 << 20, groups=groups)
    rng = np.random.default_rng(seed)
    batches = [groups_pool(rng, groups, per_group)] + [groups_pool(rng, groups, extra) for _ in range(2)]
    with (engine_cls(cfg, tuning) if tuning else engine_cls(cfg)) as a, oracle_cls(cfg) as b:
        return run_ticks(a, b, cfg, batches, rng, "%d groups x %d" % (n_groups, per_group), cancel=200).get(0)


def test_shim_nine_tiled_pair_chains(oracle_cls):
    """Nine chains, each longer than the tiny geometry's kp_late reach (PL_MAX = 1536): all tiled."""
    many_chains_pair(EmuEngineSmall, oracle_cls, 9, 1560, 60)


def many_chains_team(engine_cls, oracle_cls, n_groups, per_group, extra, tuning=None, seed=2):
    """5v5 with five roles on n_groups contiguous groups: every chain at least per_group players."""
    from microservice_matchmaking_amd.synth import ROLE_WEIGHTS_5V5
    groups = contiguous(n_groups, 500)
    cfg = make_config([mode_team(5, 2, 50, (1, 1, 1, 1, 1))], capacity=1 << 20, groups=groups)
    rng = np.random.default_rng(seed)
    w = np.asarray(ROLE_WEIGHTS_5V5, np.float64)
    batches = []
    for n in (per_group, extra, extra):
        rating, _ = groups_pool(rng, groups, n)
        batches.append((rating, cons_make(0, 0, 0, rng.choice(5, size=rating.size, p=w / w.sum()))))
    with (engine_cls(cfg, tuning) if tuning else engine_cls(cfg)) as a, oracle_cls(cfg) as b:
        return run_ticks(a, b, cfg, batches, rng, "team %d groups x %d" % (n_groups, per_group), cancel=100).get(0)


def test_shim_team_path_on_sixteen_groups(oracle_cls):
    many_chains_team(EmuEngineSmall, oracle_cls, 16, 150, 20)


SPAN_WINDOWS = [KEY_SPAN - 1, KEY_SPAN, 1 << 20, 0x3FFFFFFF]


def span_edges(engine_cls, oracle_cls, window, team, per_chain, seed=3):
    """Two groups: one chain of rating span exactly 2^19 - 1 (the fast pair path's key fully used), one of span 2^19
    (out of its reach); regions 0 / 255 and parties 0 / 15 under both filters (key bits 19-30)."""
    groups = [(0, KEY_SPAN - 1, "a"), (1 << 21, (1 << 21) + KEY_SPAN, "b")]
    mode = (mode_team(2, 2, window, (1, 1), region_filter=True, party_filter=True) if team else
            mode_1v1(window=window, region_filter=True, party_filter=True))
    cfg = make_config([mode], capacity=1 << 18, groups=groups)
    rng = np.random.default_rng(seed)
    batches = []
    for k in range(2):
        rating = np.concatenate([rng.integers(lo, hi + 1, size=per_chain if k == 0 else per_chain // 10)
                                 for lo, hi, _ in groups])
        if k == 0:
            rating[:4] = [0, KEY_SPAN - 1, 1 << 21, (1 << 21) + KEY_SPAN]       # the span's both ends in each chain
        rating = rating.astype(np.int32)
        cons = cons_make(0, rng.choice([0, 255], size=rating.size), rng.choice([0, 15], size=rating.size),
                         rng.integers(0, 2, size=rating.size) if team else 0)
        batches.append((rating, cons))
    with engine_cls(cfg) as a, oracle_cls(cfg) as b:
        run_ticks(a, b, cfg, batches, rng, "span edges w=%d team=%d" % (window, team), cancel=20)


@pytest.mark.parametrize("team", [False, True], ids=["pair", "team"])
@pytest.mark.parametrize("window", SPAN_WINDOWS)
def test_shim_span_and_key_edges(oracle_cls, window, team):
    span_edges(EmuEngineSmall, oracle_cls, window, team, 300 if team else 1600)


@pytest.mark.parametrize("which", ["oracle", "emu"])
def test_window_past_2_30_refused_at_create(oracle_cls, which):
    cls = oracle_cls if which == "oracle" else EmuEngine
    with cls(make_config([mode_1v1(window=0x3FFFFFFF)], capacity=64)):
        pass
    for m in (mode_1v1(window=0x40000000), mode_team(2, 2, 0x40000000, (1, 1))):
        with pytest.raises(MMError) as ei:
            cls(make_config([m], capacity=64))
        assert ei.value.status == -1


# ---- 6. 256 chains ---------------------------------------------------------------------------------------------------

WIDE_MODES = [
    mode_1v1(window=50),
    mode_1v1(window=25, region_filter=True, party_filter=True),
    mode_team(2, 2, 150, (1, 1)),
    mode_team(1, 3, 200, (1,)),
    mode_team(1, 4, 200, (1,)),
    mode_team(4, 2, 200, (2, 2)),
    mode_team(8, 2, 400, (1, 1, 1, 1, 1, 1, 1, 1)),
    mode_team(2, 2, 150, (1, 0, 1)),                                  # role 1: a quota of zero, never seated
    mode_1v1(window=0),
    mode_1v1(window=10 ** 6, region_filter=True),
    mode_team(3, 2, 100, (3,)),
    mode_team(2, 4, 300, (2,)),
    mode_team(5, 2, 120, (1, 1, 1, 1, 1)),
    mode_team(2, 2, 0x3FFFFFFF, (1, 1)),
    mode_team(4, 2, 100, (2, 2), party_filter=True),
    mode_1v1(window=5, region_filter=True),
]


def all_chains_batch(rng, cfg, per_chain):
    """per_chain players for every (mode, group): ratings inside the group, every role of the mode (the zero-quota
    ones too: refused at enqueue), regions 0-2, parties 0-1."""
    ratings, conss = [], []
    for md in range(cfg.n_modes):
        nr = int(cfg.modes[md].n_roles)
        for g in range(cfg.n_groups):
            lo, hi = int(cfg.groups[g].from_), int(cfg.groups[g].to)
            ratings.append(rng.integers(lo, lo + min(hi - lo, 300) + 1, size=per_chain))
            conss.append(cons_make(md, rng.integers(0, 3, size=per_chain), rng.integers(0, 2, size=per_chain),
                                   rng.integers(0, nr, size=per_chain)))
    rating, cons = np.concatenate(ratings).astype(np.int32), np.concatenate(conss)
    p = rng.permutation(rating.size)
    return rating[p], cons[p]


def chains_256(engine_cls, oracle_cls, per_chain, device_enqueue=False, capacity=1 << 14, seed=4):
    """16 modes x 16 groups, one batch that covers every chain (through enqueue and, on the device, through
    enqueue_device too), a tick of every mode; then a snapshot restored into a fresh engine, and the original, the
    restored engine and the oracle go on with arrivals and cancels."""
    groups = contiguous(16, 1000)
    cfg = make_config(WIDE_MODES, capacity=capacity, groups=groups)
    assert cfg.n_modes * cfg.n_groups == 256
    rng = np.random.default_rng(seed)
    rating, cons = all_chains_batch(rng, cfg, per_chain)
    rating_of = {}
    with engine_cls(cfg) as a, oracle_cls(cfg) as b:
        sa, sb = a.enqueue(rating, cons), b.enqueue(rating, cons)
        assert np.array_equal(sa, sb)
        ok = sa != NO_SLOT
        zero_quota = ((cons & 0xF) == 7) & (((cons >> 16) & 0xF) == 1)
        assert zero_quota.any() and np.array_equal(~ok, zero_quota)          # refused at enqueue, nothing else is
        rating_of.update(zip(sa[ok].tolist(), rating[ok].tolist()))
        assert all((a.queue_depth(m) > 0).all() for m in range(cfg.n_modes))
        with contextlib.ExitStack() as stack:
            engines = [a]
            if device_enqueue:                       # the same batch from device memory, into an engine of its own
                import torch
                d = stack.enter_context(engine_cls(cfg))
                first = d.enqueue_device(torch.from_numpy(rating).cuda(), torch.from_numpy(cons.view(np.int32)).cuda())
                assert first == 0 and d.last_enqueue_stats["accepted"] == int(ok.sum())
                assert_same_state(d, b, cfg, "256 chains, enqueue_device")
                engines.append(d)
            lobbies = 0
            for md in range(cfg.n_modes):
                mb = b.tick(md)
                assert_exact_scores(mb, cfg.modes[md], rating_of, "256 chains mode %d" % md)
                for e in engines:
                    assert_same_tick(e.tick(md), mb, "256 chains mode %d (%s)" % (md, "device" if e is not a else "host"))
                lobbies += len(mb)
            assert lobbies > 0
            for e in engines:
                assert_same_state(e, b, cfg, "256 chains")
        blob = a.snapshot()
        with engine_cls(cfg) as c:
            c.restore(blob)
            assert_same_state(c, b, cfg, "256 chains, right after restore")
            for k in range(2):
                rating, cons = all_chains_batch(rng, cfg, max(2, per_chain // 4))
                sa, sb, sc = a.enqueue(rating, cons), b.enqueue(rating, cons), c.enqueue(rating, cons)
                assert np.array_equal(sa, sb) and np.array_equal(sc, sb)
                ok = sa != NO_SLOT
                rating_of.update(zip(sa[ok].tolist(), rating[ok].tolist()))
                cs = rng.choice(sa[ok], size=50, replace=False)
                for e in (a, b, c):
                    e.cancel(cs)
                for md in range(cfg.n_modes):
                    ma, mb, mc = a.tick(md), b.tick(md), c.tick(md)
                    assert_same_tick(ma, mb, "256 chains after restore, tick %d mode %d" % (k, md))
                    assert_same_tick(mc, mb, "256 chains restored engine, tick %d mode %d" % (k, md))
                    assert_exact_scores(mc, cfg.modes[md], rating_of, "256 chains restored, mode %d" % md)
                assert_same_state(a, b, cfg, "256 chains after restore, tick %d" % k)
                assert_same_state(c, b, cfg, "256 chains restored engine, tick %d" % k)


def test_shim_256_chains_and_a_snapshot_round_trip(oracle_cls):
    chains_256(EmuEngine, oracle_cls, per_chain=20)


# ---- 8. the --wide fuzz ----------------------------------------------------------------------------------------------

def load_stress(name):
    import importlib.util
    spec = importlib.util.spec_from_file_location(name, os.path.join(os.path.dirname(os.path.abspath(__file__)),
                                                                     "stress.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_shim_wide_fuzz(monkeypatch, capsys):
    monkeypatch.setenv("MM_STRESS_ENGINE", "emu_small")
    load_stress("wide_stress_emu").main(["4", "1", "--wide"])
    out = capsys.readouterr().out
    assert "--wide" in out and "scenarios ok" in out, out


# ---- the device ------------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def gpu_cls():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a GPU; there is no CPU fallback"
    from microservice_matchmaking_amd import Engine
    return Engine


XCD_LINE = re.compile(r"physical XCD mask of each chain's workgroups in its last kp_rounds launch:((?: g\d+=0x[0-9a-f]+)+)")


def xcd_masks(err):
    """{group: mask} of the first MM_PAIR_DEBUG line naming the XCDs of each chain's last kp_rounds launch."""
    m = XCD_LINE.search(err)
    assert m, err[-2000:]
    return {int(g): int(x, 16) for g, x in re.findall(r"g(\d+)=0x([0-9a-f]+)", m.group(1))}


@pytest.mark.gpu
def test_gpu_score_of_team_sums_2_31_apart(gpu_cls, oracle_cls):
    cfg = make_config([WRAP_MODE], capacity=64, groups=WRAP_GROUPS)
    with gpu_cls(cfg) as eng:
        check_wrap_repro(eng)
    cfg = make_config([mode_team(2, 2, 0x3FFFFFFF, (1, 1))], capacity=1 << 15, groups=WRAP_GROUPS)
    with gpu_cls(cfg) as a, oracle_cls(cfg) as b:
        assert wide_team_scores(a, b, 12000, 5) >= 2 ** 31


@pytest.mark.gpu
@pytest.mark.parametrize("n_groups", [9, 12, 16])
def test_gpu_more_than_eight_tiled_pair_chains(gpu_cls, oracle_cls, n_groups, capfd):
    """kp_rounds with more chains than XCDs: pair_xcd_map's n > 8 branch puts whole chains together on an XCD.
    The tick's tile length is the shortest that holds the longest chain in 32 tiles or fewer: 30 000 players a chain
    -> 2048-position tiles, 15 tiles a chain; 16 chains over 8 XCDs -> two chains (30 workgroups, <= 32 CUs) an XCD.
    Every chain's workgroups must still run on ONE physical XCD (MM_PAIR_DEBUG's mask line), so with more than eight
    chains some share one; no stop, no fall-back."""
    ps = many_chains_pair(gpu_cls, oracle_cls, n_groups, 30000, 2000, tuning={"debug": 1})
    err = capfd.readouterr().err
    stops = ps["pair_stops_timeout"] + ps["pair_stops_xcd"] + ps["pair_stops_inject"]
    assert ps["pair_rounds_launches"] >= 1 and stops == 0 and ps["degraded"] == 0, ps
    masks = xcd_masks(err)
    tiled = {g: x for g, x in masks.items() if x}
    assert len(tiled) == n_groups, masks
    assert all(bin(x).count("1") == 1 for x in tiled.values()), masks
    assert len(set(tiled.values())) < len(tiled) and len(set(tiled.values())) <= 8, masks


@pytest.mark.gpu
def test_gpu_tiled_pair_chains_past_the_shared_xcd_map(gpu_cls, oracle_cls):
    """Nine chains of 40 000 players: 20 tiles of 2048 each, two of them on one XCD would need 40 workgroups there
    (more than its 32 CUs): pair_xcd_map gives up and the batch walks launch by launch (kp_round)."""
    ps = many_chains_pair(gpu_cls, oracle_cls, 9, 40000, 2000)
    assert ps["pair_round_launches"] >= 1, ps


@pytest.mark.gpu
@pytest.mark.parametrize("late", [False, True], ids=["default", "kt_late"])
def test_gpu_team_path_on_sixteen_groups(gpu_cls, oracle_cls, late):
    """5v5 with roles on 16 groups, every chain at least TT_MIN = 4096 players (tc_pull_xcd's G-based layout at G = 16);
    MM_TEAM_LATE=1000: every chain is handed to kt_late after its first passes."""
    ps = many_chains_team(gpu_cls, oracle_cls, 16, 5000, 300, tuning={"team_late": 1000} if late else None)
    assert ps["paths"] & 4, ps                                          # MM_PATH_TEAM
    if late:
        assert ps["team_late_launches"] >= 1, ps


@pytest.mark.gpu
@pytest.mark.parametrize("team", [False, True], ids=["pair", "team"])
@pytest.mark.parametrize("window", SPAN_WINDOWS)
def test_gpu_span_and_key_edges(gpu_cls, oracle_cls, window, team):
    span_edges(gpu_cls, oracle_cls, window, team, 6000 if team else 20000)


@pytest.mark.gpu
@pytest.mark.parametrize("tname", sorted(TABLES))
def test_gpu_bucketing_matches_the_literal_rule(gpu_cls, tname):
    bucketing_matches_the_literal_rule(gpu_cls, tname)


@pytest.mark.gpu
def test_gpu_window_past_2_30_refused_at_create(gpu_cls):
    for m in (mode_1v1(window=0x40000000), mode_team(2, 2, 0x40000000, (1, 1))):
        with pytest.raises(MMError) as ei:
            gpu_cls(make_config([m], capacity=64))
        assert ei.value.status == -1


@pytest.mark.gpu
def test_gpu_256_chains_and_a_snapshot_round_trip(gpu_cls, oracle_cls):
    chains_256(gpu_cls, oracle_cls, per_chain=40, device_enqueue=True)


@pytest.mark.gpu
def test_gpu_wide_fuzz(gpu_cls, capsys):
    load_stress("wide_stress_gpu").main(["25", "2", "--wide"])
    out = capsys.readouterr().out
    assert "--wide" in out and "scenarios ok" in out, out
