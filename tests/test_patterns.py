"""Structured arrival orders (tests/patterns.py): pools whose ORDER puts the walk into regimes an i.i.d. pool never
reaches — one lobby per pass for tens of thousands of passes, every partner at one exact distance, all N / 2 lobbies in
one pass, an anchor nobody fits — each with a closed form of what Mode R does with it.

Four tiers.  (1) the closed form against the C oracle, every family, moderate sizes and the nested chain of 132 000
players (more than 65 535 passes, more than 2^32 pairs); (2) the literal restatement (oracle/literal_ref.py) against the
C oracle on every family at up to 1 500 players; (3) the CPU shim with the tiny geometry against the oracle, every family
and parameter, sizes from tests/geometry.py; (4) the device with the product geometry (`gpu`).  In every case the
regime — passes, lobbies per pass, pairs — is asserted on the ORACLE's output before an engine is compared with it."""
import numpy as np
import pytest

import geometry as G
import patterns as P
from emu_engine import EmuEngineSmall
from helpers import assert_exact_scores_any, assert_same_state, assert_same_tick
from microservice_matchmaking_amd import Engine, cons_make, make_config, mode_1v1, mode_team
from test_oracle_literal import literal_stage, literal_tick, to_payload

MM_PATH_PAIR, MM_PATH_TEAM = 2, 4
GROUPS1 = [P.GROUP + ("all",)]
GROUPS2 = GROUPS1 + [(P.GROUP[1] + 1, P.GROUP[1] + 5000, "other")]
KINDS = {"emu_small": (EmuEngineSmall, True), "gpu": (Engine, False)}
GEO, GEO_ERRORS = {}, {}
for _kind, (_cls, _small) in KINDS.items():        # at collection: a library that is not built fails ITS cases, not the file
    try:
        GEO[_kind] = G.geometry(_cls, small=_small)
    except (OSError, ImportError, KeyError, ValueError) as _err:
        GEO_ERRORS[_kind] = _err


@pytest.fixture(scope="module")
def gpu_cls():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a GPU; there is no CPU fallback"
    return Engine


@pytest.fixture
def engine_cls(request):
    def of(kind):
        return request.getfixturevalue("gpu_cls") if kind == "gpu" else EmuEngineSmall
    return of


def mode_of(case):
    m = case.mode
    return mode_1v1(window=m[1], region_filter=m[2]) if m[0] == "1v1" else mode_team(m[1], m[2], m[3], m[4])


def check_expect(m, eng, e, tag, whole_tick=True):
    """The oracle's tick of group 0 against the closed form.  whole_tick: no other chain ran, the tick's counters are
    this chain's."""
    g0 = m.group == 0
    assert int(g0.sum()) == e.lobbies, (tag, "lobbies", int(g0.sum()), e.lobbies)
    if e.passes is not None:
        got = np.bincount(m.pass_[g0].astype(np.int64), minlength=e.n_passes).tolist()
        assert got == e.per_pass, (tag, "lobbies per pass", got[:8], e.per_pass[:8])
        assert max(got, default=0) == e.max_in_a_pass, tag
        if whole_tick:
            assert m.stats["passes_max"] == e.n_passes, (tag, "passes", m.stats["passes_max"], e.n_passes)
            assert m.stats["pairs"] == e.pairs, (tag, "pairs", m.stats["pairs"], e.pairs)
    else:
        assert int((m.pass_[g0] == 0).sum()) == e.first_pass, (tag, "lobbies of pass 0")
        if whole_tick:
            assert m.stats["passes_max"] >= e.min_passes, (tag, "regime", m.stats["passes_max"])
    assert len(eng.lobby_state(0, 0)[0]) == e.stored, (tag, "stored lobby")
    assert int(eng.queue_depth(0)[0]) == e.depth, (tag, "depth")


def other_pool(n, seed=5):
    """The random pool of the second rating group (window 3: ratings from a narrow band so that lobbies do form)."""
    rng = np.random.default_rng(seed)
    return (GROUPS2[1][0] + rng.integers(0, 200, size=n)).astype(np.int32)


def run_case(case, oracle_cls, engine=None, tuning=None, second_group=0, clock=None):
    """The case's script on the oracle (checked against the closed form) and, beside it, on `engine` (checked against the
    oracle: lobbies, order, counters, queue order, stored lobby, exact scores).  second_group: that many random players
    of another rating group ride along with the first batch.  Returns the engine's path stats per tick (or the oracle's
    Matches when there is no engine).  clock: a list that gets (oracle seconds, engine seconds) of every tick."""
    import time
    groups = GROUPS2 if second_group else GROUPS1
    mode = mode_of(case)
    cfg = make_config([mode], capacity=case.players + second_group + 8, groups=groups, default_group=0, timing=False)
    b = oracle_cls(cfg)
    a = (engine(cfg, tuning) if tuning else engine(cfg)) if engine else None
    rating_of = np.zeros(cfg.capacity, np.int64)
    slots, out, first = np.zeros(0, np.uint32), [], True
    try:
        for step in case.steps:
            if step[0] == "enqueue":
                rating, cs = step[1], step[2]
                at = None
                if first and second_group:               # spread over the arrival order; the chains do not interact
                    at = np.sort(np.random.default_rng(9).choice(rating.size + second_group, size=second_group, replace=False))
                    mine = np.setdiff1d(np.arange(rating.size + second_group), at)
                    r2, c2 = np.zeros(rating.size + second_group, np.int32), np.zeros(rating.size + second_group, np.uint32)
                    r2[mine], c2[mine], r2[at] = rating, cs, other_pool(second_group)
                    # roles of the riders: any the mode knows
                    c2[at] = cons_make(0, 0, 0, np.arange(second_group) % cfg.modes[0].n_roles)
                    rating, cs = r2, c2
                first = False
                sb = b.enqueue(rating, cs)
                if a is not None:
                    assert np.array_equal(a.enqueue(rating, cs), sb), (str(case), "slots")
                rating_of[sb] = rating
                slots = np.concatenate([slots, sb if at is None else sb[mine]])
            elif step[0] == "cancel":
                cs = slots[step[1]]
                b.cancel(cs)
                if a is not None:
                    a.cancel(cs)
            else:
                tag = "%s tick %d" % (case, len(out))
                t0 = time.perf_counter()
                mb = b.tick(0)
                t1 = time.perf_counter()
                check_expect(mb, b, step[1], tag, whole_tick=not second_group)
                if a is None:
                    out.append(mb)
                    continue
                t2 = time.perf_counter()
                ma = a.tick(0)
                if clock is not None:
                    clock.append((t1 - t0, time.perf_counter() - t2))
                assert_same_tick(ma, mb, tag)
                assert_same_state(a, b, cfg, tag)
                assert_exact_scores_any(ma, cfg.modes[0], rating_of, tag)
                out.append(a.path_stats())
    finally:
        b.close()
        if a is not None:
            a.close()
    return out


# ----------------------------------------------------------------------------------------------------------------------
# the cases of one geometry
# ----------------------------------------------------------------------------------------------------------------------
def shifted_distances(geo):
    T = geo["PK_T"]
    return sorted({63, 64, 65, T - 1, T, T + 1, 2 * T - 1, 2 * T, 2 * T + 1, geo["PL_MAX"]})


def tile_length(geo, n):
    """pair_walk: the tile length of a tick's first batch — the shortest that keeps the chain within tiles_cap tiles."""
    for t in reversed(geo["tile_lengths"][1:]):
        if -(-n // t) <= G.tiles_cap(geo):
            return t
    return geo["tile_lengths"][0]


def horizon_cases(geo, one_tile_too=True):
    """stretches and decoy aimed at the horizon — two tiles of the length the CHAIN is cut into: for each tile length a
    chain of the shortest length that is tiled with it, partners (and a repaired pointer's second fit) at t, 2t - 1 ...
    2t + 1 positions, the first of them counted from a tile's first position.  Tile lengths no tiled chain of the geometry
    can have (tiles_cap x t < PL_MAX) have no case; neither has a chain whose fillers' ratings would leave the packed key.
    one_tile_too=False leaves out the stretches of t - 1 .. t + 1 (the shim pays three seconds for every tiled tick;
    shifted(d) has those distances)."""
    out, cap = [], G.tiles_cap(geo)
    for t in sorted(geo["tile_lengths"]):
        lo = max(geo["PL_MAX"], cap * (t // 2) + 1)
        if lo > cap * t:
            continue
        for d in ((t - 1, t, t + 1) if one_tile_too else ()) + (2 * t - 1, 2 * t, 2 * t + 1):
            c = P.stretches(d, -(-lo // (d + 1)))
            assert tile_length(geo, c.players) == t, (t, d, c.players)
            out.append(c)
        n = lo + 8
        if 1000 + 4 * n < P.SPAN_MAX["1v1"]:
            assert tile_length(geo, n) == t and n > 2 * t + 8
            out += [P.decoy(p, n) for p in (2 * t - 2, 2 * t - 1, 2 * t, 2 * t + 1)]
    # the LDS-resident walk (a chain below PL_MAX): its own repair behind the cursor
    out += [P.decoy(p, geo["PL_MAX"] - 2) for p in (G.WAVE, geo["PL_MAX"] // 2, geo["PL_MAX"] - 6)]
    return out


def pair_cases(geo, k_nested, levels_long, one_tile_too=True):
    """Every pair family and parameter for one geometry.  k_nested: values of the nested chains (passes of the tick);
    levels_long: passes - 1 of the runs of about a tile."""
    T, PL = geo["PK_T"], geo["PL_MAX"]
    out = [P.nested(k_nested), P.nested_dead(k_nested // 2 + 3)]
    out += [P.shifted(d) for d in shifted_distances(geo)]
    out += [P.in_order(4 * T + 1), P.in_order(4 * T + 1, reverse=True), P.in_order(PL), P.in_order(PL - 1, reverse=True)]
    out += [P.runs(1, 6), P.runs(63, 3), P.runs(64, 3), P.runs(65, 3), P.runs(T - 1, levels_long), P.runs(T + 1, levels_long)]
    out += [P.interleaved(R, max(1, 2 * T // R)) for R in (2, 64, 255, 256)]
    out += [P.blocked_head(PL + 64, "partner"), P.blocked_head(PL + 64, "cancel"), P.blocked_head(2 * G.WAVE, "cancel")]
    out += [P.carried_head(1200)]     # 600 steps through kp_late's ring of 512; 1201 players: below PL_MAX in every geometry
    out += P.dead_variants(4 * T, T)
    # the alive share after pass 0 at, one below and one above the two compaction rules (mm_pair.inc: `qlen * 4 < m * 3`
    # on the tiled path — chains from PL_MAX on — and `m > PL_COMPACT_MIN && qlen * 2 < m` in the LDS-resident walk)
    out += [P.alive_share_at(PL, 3, 4, d, T) for d in (-1, 0, 1)]
    out += [P.alive_share_at(geo["PL_COMPACT_MIN"] + 2, 1, 2, d, G.WAVE) for d in (-1, 0, 1)]
    return out + horizon_cases(geo, one_tile_too)


def team_distances(geo):
    return sorted({geo["TF_BW"] * 32 - 1, geo["TF_BW"] * 32 + 1, geo["TT_CH"] - 1, geo["TT_CH"] + 1,
                   geo["TT_SCAN_CAP"] - 1, geo["TT_SCAN_CAP"] + 1})


def team_cases(geo, scale, far_shapes=("5v5", "2v2", "3x2")):
    """Every team family for one geometry; chains of at least TT_MIN players (the team path).  scale: the many-pass
    families' pass counts.  far_shapes: the shapes that run the distances past a chunk (the shim pays for every
    player of a team chain, tests/geometry.py team_boundaries)."""
    tt = geo["TT_MIN"]
    out = []
    for shape in P.SHAPES:
        L = P.SHAPES[shape][1] * P.SHAPES[shape][2]
        out += [P.team_dense(shape, max(tt // L + 1, 3 * scale)), P.team_nested(shape, max(tt // L + 1, scale)),
                P.team_shifted_blocks(shape, max(tt // L + 1, geo["TT_SCAN_CAP"] + 1))]
        for d in team_distances(geo):
            if d <= 2 * geo["TT_CH"] or shape in far_shapes:
                out.append(P.team_shifted(shape, d, max(2, -(-tt // (d + L - 1)))))
    q = max(scale, tt // 20 + 1)
    out += [P.scarce_role_at_the_tail(q), P.role_sorted(max(scale // 4, tt // 50 + 1)), P.role_missing(max(5, tt // 4 + 1))]
    return out


def ident(c):
    return str(c).replace(" ", "")


def small_cases():
    """<= 1 500 players each: the literal restatement's tier (pure Python, one deep copy of the lobby per attempt)."""
    geo = dict(PK_T=128, tile_lengths=(128, 64, 32), pair_ptiles=3, pair_tiles_max=3, PL_MAX=384, PL_COMPACT_MIN=64,
               TT_MIN=64, TF_BW=4, TT_CH=48, TT_SCAN_CAP=24)
    out = [c for c in pair_cases(geo, 120, 1) if c.players <= 1500]
    out += [c for c in team_cases(geo, 12) if c.players <= 1500]
    return out


def shim_cases(team):
    if "emu_small" not in GEO:
        return []
    geo = GEO["emu_small"]
    return team_cases(geo, 24, far_shapes=("2v2",)) if team else pair_cases(geo, geo["PL_MAX"] // 2 + 32, 1, one_tile_too=False)


def gpu_cases(team):
    if "gpu" not in GEO:
        return []
    geo = GEO["gpu"]
    return team_cases(geo, 400) if team else pair_cases(geo, geo["PL_MAX"] + 300, 2)


def moderate_cases():
    """The closed forms against the oracle alone, at the product's geometry where the oracle can afford it."""
    geo = GEO.get("gpu") or GEO.get("emu_small")
    if geo is None:
        return []
    return pair_cases(geo, 3000, 2) + team_cases(geo, 200)


# ----------------------------------------------------------------------------------------------------------------------
# 1. closed forms against the oracle
# ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", sorted(KINDS))
def test_the_geometry_is_read(kind):
    assert kind in GEO, GEO_ERRORS[kind]


def test_cons_packing_is_the_engine_s():
    rng = np.random.default_rng(1)
    region, role = rng.integers(0, 256, size=500), rng.integers(0, 16, size=500)
    assert np.array_equal(P.cons(500, region=region, role=role), cons_make(0, region, 0, role))


@pytest.mark.parametrize("case", moderate_cases(), ids=ident)
def test_closed_form_is_the_oracle_s(oracle_cls, case):
    run_case(case, oracle_cls)


NESTED_LONG = 66000


def test_nested_chain_past_16_bit_passes_and_32_bit_pairs(oracle_cls):
    """k = 66 000: 132 000 players, one lobby per pass.  passes = k > 65 535 and pairs = k^2 > 2^32 hold from k = 65 537
    on; the 1.4 % more that 66 000 costs keep both counters clear of the very first value past the limit.  The oracle
    walks 4.36e9 attempts on one thread (about 20 s)."""
    case = P.nested(NESTED_LONG)
    e = case.steps[-1][1]
    assert e.n_passes > 65535 and e.pairs > 1 << 32
    (m,) = run_case(case, oracle_cls)
    assert m.pass_.tolist() == list(range(NESTED_LONG))
    # the partner is always the LAST queued player: lobby j is (slot j, slot 2k - 1 - j)
    assert np.array_equal(m.slots, np.stack([np.arange(NESTED_LONG), 2 * NESTED_LONG - 1 - np.arange(NESTED_LONG)], axis=1))


# ----------------------------------------------------------------------------------------------------------------------
# 2. second witness: the literal restatement
# ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", small_cases(), ids=ident)
def test_literal_restatement_agrees_on_structured_orders(oracle_cls, case):
    """The harness of tests/test_oracle_literal.py: emissions, pass numbers, stored lobbies and pair counts."""
    assert case.players <= 1500
    cfg = make_config([mode_of(case)], capacity=case.players + 8, groups=GROUPS1, default_group=0, timing=False)
    eng, stage = oracle_cls(cfg), literal_stage(cfg, GROUPS1)
    slots = np.zeros(0, np.uint32)
    try:
        for step in case.steps:
            if step[0] == "enqueue":
                s = eng.enqueue(step[1], step[2])
                for x in zip(s, step[1], step[2]):
                    stage.deliver(to_payload(*x))
                slots = np.concatenate([slots, s])
            elif step[0] == "cancel":
                eng.cancel(slots[step[1]])
                for s in slots[step[1]]:
                    stage.cancel(int(s))
            else:
                pairs0 = stage.pairs
                lit = literal_tick(stage, cfg, GROUPS1)[0]
                m = eng.tick(0)
                check_expect(m, eng, step[1], str(case))
                got = [(int(g), int(p), s.tolist()) for g, p, s in zip(m.group, m.pass_, m.slots)]
                assert got == lit, (str(case), "emissions")
                assert m.stats["pairs"] == stage.pairs - pairs0, (str(case), "pairs")
                want = [p["id"] for rec in stage.lobbies.tables["all"] for t in range(cfg.modes[0].teams)
                        for p in rec[1].get("team %d" % (t + 1), [])]
                assert eng.lobby_state(0, 0)[0].tolist() == want, (str(case), "stored lobby")
                assert eng.queue_slots(0, 0).tolist() == [p["id"] for p in stage.queues["all"] if stage.active.in_queue(p["id"])]
    finally:
        eng.close()


# ----------------------------------------------------------------------------------------------------------------------
# 3. the CPU shim, tiny geometry
# ----------------------------------------------------------------------------------------------------------------------
def assert_path(geo, case, stats, tag):
    """The family took the path it is meant for (first tick's mm_path_stats)."""
    ps = stats[0]
    n0 = case.steps[0][1].size - sum(s[1].size for s in case.steps[1:2] if s[0] == "cancel")
    if case.mode[0] == "1v1":
        assert ps["paths"] == MM_PATH_PAIR, (tag, ps["paths"])
        if n0 < geo["PL_MAX"]:
            assert ps["pair_tiled_passes"] == 0, (tag, ps)
        else:
            assert ps["pair_tiled_passes"] >= 1, (tag, ps)
    elif geo["TT_MIN"] <= n0:
        assert ps["paths"] & MM_PATH_TEAM, (tag, ps["paths"])


@pytest.mark.parametrize("case", shim_cases(False), ids=ident)
def test_shim_pair_families(oracle_cls, case):
    assert_path(GEO["emu_small"], case, run_case(case, oracle_cls, EmuEngineSmall), str(case))


def one_of_each(cases, smallest=False):
    """The first case of every family (smallest: the one with the fewest players)."""
    out = {}
    for c in cases:
        if c.family not in out or (smallest and c.players < out[c.family].players):
            out[c.family] = c
    return list(out.values())


@pytest.mark.parametrize("case", one_of_each(shim_cases(False), smallest=True), ids=ident)
def test_shim_pair_families_beside_a_random_group(oracle_cls, case):
    """Once more beside a second rating group that holds a random pool: another chain shares the launches."""
    run_case(case, oracle_cls, EmuEngineSmall, second_group=GEO["emu_small"]["PK_T"] + 100)


@pytest.mark.parametrize("case", shim_cases(True), ids=ident)
def test_shim_team_families(oracle_cls, case):
    assert_path(GEO["emu_small"], case, run_case(case, oracle_cls, EmuEngineSmall), str(case))


# ----------------------------------------------------------------------------------------------------------------------
# 4. the device, product geometry
# ----------------------------------------------------------------------------------------------------------------------
def gpu_param(cases):
    return [pytest.param(c, id=ident(c), marks=pytest.mark.gpu) for c in cases]


@pytest.mark.parametrize("case", gpu_param(gpu_cases(False)))
def test_gpu_pair_families(gpu_cls, oracle_cls, case):
    assert_path(GEO["gpu"], case, run_case(case, oracle_cls, gpu_cls), str(case))


@pytest.mark.parametrize("case", gpu_param(one_of_each(gpu_cases(False))))
def test_gpu_pair_families_beside_a_random_group(gpu_cls, oracle_cls, case):
    run_case(case, oracle_cls, gpu_cls, second_group=3 * GEO["gpu"]["PL_MAX"])


@pytest.mark.parametrize("case", gpu_param(gpu_cases(True)))
def test_gpu_team_families(gpu_cls, oracle_cls, case):
    assert_path(GEO["gpu"], case, run_case(case, oracle_cls, gpu_cls), str(case))


@pytest.mark.gpu
def test_gpu_nested_chain_past_16_bit_passes_and_32_bit_pairs(gpu_cls, oracle_cls):
    """132 000 players, 66 000 passes of one lobby, 4.356e9 pairs: pass numbers, mm_stats.pairs, queue order and stored
    lobby are the oracle's (run_case), and the tick stayed on the headline path: inside kp_rounds for the tiled part,
    every pass of the critical chain accounted for, no fall-back on default tuning."""
    case, clock = P.nested(NESTED_LONG), []
    (ps,) = run_case(case, oracle_cls, gpu_cls, clock=clock)
    print("nested(%d): oracle %.2f s, engine %.3f s, path stats %s" % (NESTED_LONG, clock[0][0], clock[0][1], ps))
    assert ps["paths"] == MM_PATH_PAIR, ps
    assert ps["pair_rounds_passes"] > 0, ps
    assert ps["crit_passes"] == NESTED_LONG, ps
    assert ps["crit_rounds_passes"] + ps["crit_round_passes"] + ps["crit_late_passes"] == ps["crit_passes"], ps
    assert ps["pair_tiled_passes"] == ps["crit_rounds_passes"] + ps["crit_round_passes"], ps
    # the chain leaves the tiled path when fewer than PL_MAX players are queued: after k - PL_MAX / 2 passes
    assert abs(ps["pair_tiled_passes"] - (NESTED_LONG - GEO["gpu"]["PL_MAX"] // 2)) <= 1, ps
    assert not ps["degraded"], ps


@pytest.mark.gpu
@pytest.mark.parametrize("family", ["sorted", "reverse_sorted", "team_dense_5v5", "team_dense_2v2", "team_dense_3x2"])
def test_gpu_one_pass_at_a_million_players(gpu_cls, oracle_cls, family):
    """All N / L lobbies of a 1M pool in ONE pass."""
    n = 1 << 20
    if family.startswith("team_dense"):
        shape = family.rsplit("_", 1)[1]
        case = P.team_dense(shape, n // (P.SHAPES[shape][1] * P.SHAPES[shape][2]))
    else:
        case = P.in_order(n, reverse=family == "reverse_sorted")
    assert case.steps[-1][1].n_passes == 1
    (ps,) = run_case(case, oracle_cls, gpu_cls)
    assert ps["paths"] == (MM_PATH_PAIR if case.mode[0] == "1v1" else MM_PATH_TEAM), ps


# ----------------------------------------------------------------------------------------------------------------------
# tests/stress.py --patterns
# ----------------------------------------------------------------------------------------------------------------------
def stress_module(name):
    import importlib.util
    import os
    path = os.path.join(os.path.dirname(os.path.abspath(__file__)), "stress.py")
    spec = importlib.util.spec_from_file_location(name, path)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


@pytest.mark.parametrize("what", ["pair", "team"])
def test_shim_structured_order_stress_with_fuzzed_knobs(what, monkeypatch, capsys):
    """tests/stress.py --patterns --fuzz-knobs on the fiber-shim build: six seeded scenarios each — a pattern family with
    its parameter from the geometry tables of the DRAWN tuning, then another pattern or a random pool, structured
    cancels in between (the device's share: test_gpu_structured_order_stress_with_fuzzed_knobs)."""
    monkeypatch.setenv("MM_STRESS_ENGINE", "emu_small")
    mod = stress_module("shim_stress_patterns_" + what)
    monkeypatch.setattr(mod, "FUZZ", True)
    mod.patterns_main(600.0, 21 if what == "pair" else 22, team=what == "team", count=6)
    out = capsys.readouterr().out
    assert "--patterns%s --fuzz-knobs: 6 scenarios ok" % (" team" if what == "team" else "") in out, out


@pytest.mark.gpu
@pytest.mark.parametrize("what", ["pair", "team"])
def test_gpu_structured_order_stress_with_fuzzed_knobs(gpu_cls, what, capsys):
    """Twenty seconds each of tests/stress.py --patterns --fuzz-knobs on the device."""
    mod = stress_module("gpu_stress_patterns_" + what)
    mod.main(["20", "9" if what == "pair" else "10"] + (["team"] if what == "team" else []) + ["--patterns", "--fuzz-knobs"])
    out = capsys.readouterr().out
    assert "--patterns" in out and "--fuzz-knobs" in out and "scenarios ok" in out, out
