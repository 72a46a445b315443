"""Pins oracle/mode_r.c against the literal restatement of worker.ex (oracle/literal_ref.py):
same random scripts (enqueue batches, cancels between ticks, mixed modes sharing a group
queue) must give identical emissions, lobby states and pair counts."""
import numpy as np
import pytest

from microservice_matchmaking_amd._abi import cons_make
from microservice_matchmaking_amd.config import (REFERENCE_RATING_GROUPS, make_config, mode_1v1,
                                                 mode_dicts, mode_team)
from oracle.literal_ref import SearchStage, find_rating_group_by_rating, team_name

MODE_SETS = {
    "1v1": [mode_1v1(window=50)],
    "1v1_region": [mode_1v1(window=25, region_filter=True)],
    "5v5_roles": [mode_team(5, 2, 120, (1, 1, 1, 1, 1))],
    "mixed": [mode_1v1(window=40, region_filter=True), mode_team(2, 2, 150, (1, 1)),
              mode_team(3, 2, 200, (3,), party_filter=True)],
    "3teams": [mode_team(2, 3, 300, (2,))],
}


def literal_stage(cfg, groups=REFERENCE_RATING_GROUPS):
    """groups: (from, to, name) rows as make_config got them; a cfg.default_group other than
    generic/worker.ex:27's div(n, 2) + 1 is handed to the literal stage explicitly."""
    md = mode_dicts(cfg)
    dflt = None if cfg.default_group == len(groups) // 2 + 1 else groups[cfg.default_group]
    return SearchStage({"mode%d" % i: m for i, m in enumerate(md)}, groups, dflt)


def to_payload(slot, rating, cons):
    c = int(cons)
    return {"id": int(slot), "rating": int(rating), "game-mode": "mode%d" % (c & 0xF),
            "region": (c >> 4) & 0xFF, "party": (c >> 12) & 0xF, "role": (c >> 16) & 0xF}


def literal_tick(stage, cfg, groups=REFERENCE_RATING_GROUPS):
    """All groups, all modes in one mixed run; returns per-mode emission lists
    [(group_index, pass, [slots in team order])]."""
    per_mode = {m: [] for m in range(cfg.n_modes)}
    for gi, g in enumerate(groups):
        n0 = len(stage.emitted)
        plog = []
        stage.run_group_to_quiescence(g[2], pass_log=plog)
        for em, ps in zip(stage.emitted[n0:], plog):
            mode = int(em["game-mode"][4:])
            teams = cfg.modes[mode].teams
            slots = [p["id"] for t in range(teams) for p in em["teams"][team_name(t)]]
            per_mode[mode].append((gi, ps, slots))
    return per_mode


@pytest.mark.parametrize("mset", sorted(MODE_SETS))
@pytest.mark.parametrize("seed", [1, 2, 3])
def test_oracle_matches_literal(oracle_cls, mset, seed):
    rng = np.random.default_rng(1000 * seed + len(mset))
    cfg = make_config(MODE_SETS[mset], capacity=4096)
    eng = oracle_cls(cfg)
    stage = literal_stage(cfg)
    live = []
    for rnd in range(4):
        n = int(rng.integers(20, 160))
        # narrow rating band so that lobbies actually fill; a few outliers hit A1's default
        rating = rng.integers(1300, 2300, size=n).astype(np.int32)
        rating[rng.random(n) < 0.03] = 6000
        mode = rng.integers(0, cfg.n_modes, size=n)
        role = np.array([rng.integers(0, cfg.modes[int(m)].n_roles) for m in mode])
        cons = cons_make(mode, rng.integers(0, 2, size=n), rng.integers(0, 2, size=n), role)
        slots = eng.enqueue(rating, cons)
        for s, r, c in zip(slots, rating, cons):
            stage.deliver(to_payload(s, r, c))
        live.extend(slots.tolist())
        if rnd > 0 and live:
            cs = rng.choice(np.asarray(live), size=max(1, len(live) // 10), replace=False)
            eng.cancel(cs.astype(np.uint32))
            for s in cs:
                stage.cancel(int(s))
            live = [s for s in live if s not in set(cs.tolist())]
        pairs0 = stage.pairs
        lit = literal_tick(stage, cfg)
        pairs_oracle = 0
        for mode_i in range(cfg.n_modes):
            m = eng.tick(mode_i)
            got = [(int(g), int(p), s.tolist()) for g, p, s in zip(m.group, m.pass_, m.slots)]
            assert got == lit[mode_i], (mset, seed, rnd, mode_i)
            pairs_oracle += m.stats["pairs"]
            gone = set(m.slots.ravel().tolist())
            live = [s for s in live if s not in gone]
            # open lobbies agree too
            for gi, g in enumerate(REFERENCE_RATING_GROUPS):
                want = []
                for rec in stage.lobbies.tables[g[2]]:
                    if rec[2] == "mode%d" % mode_i:
                        want = [p["id"] for t in range(cfg.modes[mode_i].teams)
                                for p in rec[1].get(team_name(t), [])]
                s, _ = eng.lobby_state(mode_i, gi)
                assert s.tolist() == want, (mset, seed, rnd, mode_i, gi)
        if cfg.n_modes == 1:
            # with several modes in one group queue the literal keeps rotating a quiescent
            # mode's players while another mode still progresses, so only the single-mode
            # pair count is schedule-independent
            assert pairs_oracle == stage.pairs - pairs0, (mset, seed, rnd)


def test_oracle_matches_literal_chain_by_chain(oracle_cls):
    """Mode R ends a tick per chain (docs/MATCH_CHECK.md section 4): with one literal stage per
    mode — the same code, fed only its own mode's players — the oracle agrees on every random
    script with cancels, not only on most of them.  (In the mixed run above a quiescent mode's
    players keep rotating while another mode still progresses, so a head that a stale lobby
    rejected can meet the filtered lobby within the tick instead of at the next one: 29 of 400
    random scripts then differ in a stored lobby.  Seed 15 is one of them.)"""
    mset = "mixed"
    for seed in [15, 23, 24, 78, 88] + list(range(400, 595)):
        rng = np.random.default_rng(1000 * seed + len(mset))
        cfg = make_config(MODE_SETS[mset], capacity=4096)
        eng = oracle_cls(cfg)
        stages = [literal_stage(cfg) for _ in range(cfg.n_modes)]
        live = []
        for rnd in range(4):
            n = int(rng.integers(20, 160))
            rating = rng.integers(1300, 2300, size=n).astype(np.int32)
            rating[rng.random(n) < 0.03] = 6000
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
                lit = literal_tick(stages[mode_i], cfg)
                m = eng.tick(mode_i)
                got = [(int(g), int(p), s.tolist()) for g, p, s in zip(m.group, m.pass_, m.slots)]
                assert got == lit[mode_i], (seed, rnd, mode_i)
                assert m.stats["pairs"] == stages[mode_i].pairs - pairs0, (seed, rnd, mode_i, "pairs")
                gone = set(m.slots.ravel().tolist())
                live = [s for s in live if s not in gone]
                for gi, g in enumerate(REFERENCE_RATING_GROUPS):
                    want = []
                    for rec in stages[mode_i].lobbies.tables[g[2]]:
                        if rec[2] == "mode%d" % mode_i:
                            want = [p["id"] for t in range(cfg.modes[mode_i].teams)
                                    for p in rec[1].get(team_name(t), [])]
                    s, _ = eng.lobby_state(mode_i, gi)
                    assert s.tolist() == want, (seed, rnd, mode_i, gi)
        eng.close()


def test_literal_rating_group_matches_golden():
    from helpers import load_golden
    import math
    for rating, want in load_golden()["rating_group_cases"]["cases"]:
        r = math.nan if rating == "nan" else rating
        g = find_rating_group_by_rating(r)
        assert REFERENCE_RATING_GROUPS.index(g) == want
    assert find_rating_group_by_rating(None)[2] == "diamond"


def test_per_chain_tick_boundary_is_the_only_departure_from_the_shared_queue():
    """The golden case `tick_ends_per_chain_while_another_mode_of_the_group_progresses` on the
    literal restatement, both ways: one literal stage per mode (Mode R's per-chain tick) leaves B
    queued and the lobby empty, exactly as the golden case says; ONE literal queue for both modes
    (worker.ex:308-321 read literally: the group's rotation goes on while mode 1 seats players)
    seats B one rotation later inside the same tick.  The next tick brings both to the same state."""
    from helpers import load_golden, players_to_arrays
    case = [c for c in load_golden()["cases"] if c["name"].startswith("tick_ends_per_chain")][0]
    cfg = make_config(case["modes"], capacity=64)

    def run(shared):
        stages = [literal_stage(cfg)] if shared else [literal_stage(cfg) for _ in range(cfg.n_modes)]
        next_slot, lobbies = 0, []
        for step in case["steps"]:
            if step["op"] == "enqueue":
                r, c = players_to_arrays(step["players"])
                for rr, cc in zip(r, c):
                    stages[0 if shared else int(cc) & 0xF].deliver(to_payload(next_slot, rr, cc))
                    next_slot += 1
            elif step["op"] == "cancel":
                for s in step["slots"]:
                    for st in stages:
                        st.cancel(s)
            else:
                st = stages[0 if shared else step["mode"]]
                st.run_group_to_quiescence("bronze")
                rec = [r for r in st.lobbies.tables["bronze"] if r[2] == "mode%d" % step["mode"]]
                lobbies.append([p["id"] for r in rec for t in sorted(r[1]) for p in r[1][t]])
        return lobbies

    per_chain, shared = run(False), run(True)
    want = [s["expect"]["lobby"]["0"]["slots"] for s in case["steps"] if s["op"] == "tick"]
    assert per_chain == want == [[0], [], [], [1]]
    assert shared == [[0], [1], [], [1]]           # B meets the filtered lobby within tick 2 (3rd entry: mode 1's lobby)
    assert per_chain[-1] == shared[-1]             # deferred to the tick boundary, never lost
