"""The walk's geometry boundaries, with chains of EXACT length and partners at EXACT distances.

Every other parity test draws its chain lengths at random; the kernels switch behaviour at exact lengths (PL_MAX, the
tile lengths and their multiples, kp_rounds' reach, TT_MIN, chunks of TT_CH ...) and at exact distances (a tile, the
horizon of two tiles, kp_nx_init's segment and staged window, the 16-bit offsets of nx16 and of kt_f's records).  Here
every case uses ONE rating group, so the chain length is the number of players enqueued, and the lengths and distances
come from tests/geometry.py, which reads them from the source.  Each case: engine vs oracle, lobbies and their order,
counters, queue order, stored lobby, and scores to the bit.  The same cases run on the CPU shim with the tiny geometry
(tests/emu, `not gpu`) and on the device with the product's (`gpu`)."""
import numpy as np
import pytest

import geometry as G
from emu_engine import EmuEngineSmall
from helpers import assert_exact_scores_any, assert_same_state, assert_same_tick
from microservice_matchmaking_amd import Engine, cons_make, make_config, mode_1v1, mode_team
from microservice_matchmaking_amd._abi import MMError
from microservice_matchmaking_amd.synth import ROLE_WEIGHTS_5V5, make_pool

MM_PATH_TEAM = 4
MM_ERR_FULL = -4
ONE_GROUP = [(0, 5000, "all")]
KINDS = {"emu_small": (EmuEngineSmall, True), "gpu": (Engine, False)}
GEO, GEO_ERRORS = {}, {}
for _kind, (_cls, _small) in KINDS.items():        # at collection: a library that is not built fails ITS cases, below, not the file
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
    """kind -> engine class (the device's only when the case is one of the gpu tier)."""
    def of(kind):
        return request.getfixturevalue("gpu_cls") if kind == "gpu" else EmuEngineSmall
    return of


def case(kind, *args, id):
    return pytest.param(kind, *args, id="%s-%s" % (kind, id), marks=[pytest.mark.gpu] if kind == "gpu" else [])


def one_group(modes, capacity):
    return make_config(modes, capacity=capacity, groups=ONE_GROUP, default_group=0, timing=False)


def pair_pool(n, pred, seed=1):
    """sparse: window 25 + region filter, 4 regions, ratings over the whole group (most players stay, many passes);
    dense: window 0, ratings from 40 values (the chain shrinks through every shorter boundary within the tick)."""
    rng = np.random.default_rng([seed, n])
    if pred == "sparse":
        return (rng.integers(0, 5001, size=n).astype(np.int32), cons_make(0, rng.integers(0, 4, size=n), 0, 0),
                mode_1v1(window=25, region_filter=True))
    return (rng.integers(0, 40, size=n) * 100).astype(np.int32), cons_make(np.zeros(n, np.int64)), mode_1v1(window=0)


def team_pool(n, shape, seed=1):
    """5v5: cfg-3's role weights (supports scarce), window 100; 2v2: roles (1, 1), role 1 one player in five, window 300."""
    if shape == "5v5":
        rating, cons = make_pool(n, seed=seed, role_weights=ROLE_WEIGHTS_5V5)
        return rating, cons, mode_team(5, 2, 100, (1, 1, 1, 1, 1))
    rng = np.random.default_rng([seed, n])
    return (rng.integers(0, 5001, size=n).astype(np.int32), cons_make(0, 0, 0, (rng.random(n) < 0.2).astype(np.uint32)),
            mode_team(2, 2, 300, (1, 1)))


class Pair:
    """The engine under test and the oracle, driven by the same calls; remembers every slot's rating for the scores."""

    def __init__(self, engine, oracle, cfg, tuning=None):
        self.cfg, self.a, self.b = cfg, engine(cfg, tuning) if tuning else engine(cfg), oracle(cfg)
        self.rating_of = np.zeros(cfg.capacity, np.int64)

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.a.close()
        self.b.close()

    def enqueue(self, rating, cons):
        sa, sb = self.a.enqueue(rating, cons), self.b.enqueue(rating, cons)
        assert np.array_equal(sa, sb), "slots"
        self.rating_of[sa] = rating
        return sa

    def cancel(self, slots):
        slots = np.asarray(slots, np.uint32)
        self.a.cancel(slots)
        self.b.cancel(slots)

    def tick(self, tag, mode=0):
        ma, mb = self.a.tick(mode), self.b.tick(mode)
        assert_same_tick(ma, mb, tag)
        assert_same_state(self.a, self.b, self.cfg, tag)
        assert_exact_scores_any(ma, self.cfg.modes[mode], self.rating_of, tag)
        return ma


# ------------------------------------------------------------------------------------------------------------------
# a. pair: a tick that STARTS at an exact length
# ------------------------------------------------------------------------------------------------------------------
def pair_length_cases():
    out = []
    for kind, geo in GEO.items():
        for entry in G.pair_boundaries(geo):
            for n, preds in G.pair_plan(entry, geo, shim=kind != "gpu"):
                for pred in preds:
                    out.append(case(kind, entry[0], n, pred, id="%s-%d-%s" % (entry[1], n, pred)))
    return out


def assert_pair_path(geo, n, ps, tag, shim):
    """Where mm_path_stats can tell the two sides of a boundary apart, it must: the table sits on the real switch points.
    PL_MAX: no tiled pass below it, at least one from it on.  pair_ptiles x PK_T: up to it kp_rounds takes the chain from the
    first batch (no kp_round launch in the tick), one more player and the tick starts launch by launch.  The other
    boundaries (tile lengths, the tiles_max multiples, PL_COMPACT_MIN, kp_init's rows, kp_nx_init's segments) leave no
    counter of their own in the record: parity alone."""
    assert ps["paths"] == 2, (tag, ps["paths"])
    if n < geo["PL_MAX"]:
        assert ps["pair_tiled_passes"] == 0 and ps["pair_rounds_launches"] == 0 and ps["pair_round_launches"] == 0, (tag, ps)
    else:
        assert ps["pair_tiled_passes"] >= 1, (tag, ps)
        if n <= geo["pair_ptiles"] * geo["PK_T"]:
            # (on the device a kp_rounds launch that gave up — a bounded wait that ran out on a busy GPU — is followed by
            # kp_round batches; the shim has no such stop)
            stops = 0 if shim else ps["pair_stops_timeout"] + ps["pair_stops_xcd"]
            assert ps["pair_rounds_launches"] >= 1 and (ps["pair_round_launches"] == 0 or stops > 0), (tag, ps)
        else:
            assert ps["pair_round_launches"] >= 1, (tag, ps)


@pytest.mark.parametrize("kind,B,n,pred", pair_length_cases())
def test_pair_tick_starts_at_an_exact_length(engine_cls, oracle_cls, kind, B, n, pred):
    rating, cons, mode = pair_pool(n, pred)
    tag = "%s B=%d n=%d %s" % (kind, B, n, pred)
    with Pair(engine_cls(kind), oracle_cls, one_group([mode], n + 8)) as p:
        p.enqueue(rating, cons)
        assert int(p.b.queue_depth(0)[0]) == n                 # the construction: one chain of exactly n players
        p.tick(tag)
        assert_pair_path(GEO[kind], n, p.a.path_stats(), tag, shim=kind != "gpu")


# ------------------------------------------------------------------------------------------------------------------
# b. a later tick at an exact length: a stored anchor and a rotated queue, or cancels purged at the head of the tick
# ------------------------------------------------------------------------------------------------------------------
def second_tick_boundaries(geo):
    """[(B, name, team?, plus)]: the subset of both tables a later tick is aimed at.  plus: B + 1 is a side of its own
    (geometry.pair_boundaries); PL_MAX and TT_MIN are `<` / `>=` tests, B - 1 and B are their two sides."""
    return [(geo["PL_MAX"], "PL_MAX", False, False), (geo["PK_T"], "T", False, True),
            (geo["pair_ptiles"] * (geo["PK_T"] // 4), "ptiles_x_T/4", False, True),
            (geo["TT_MIN"], "TT_MIN", True, False), (geo["TT_CH"] * 8, "TT_CHx8", True, True)]


def later_deltas(kind, plus):
    """The device runs B - 1, B, B + 1 everywhere; the shim B + 1 only where it is a side of its own (what it costs: geometry.pair_plan)."""
    return (-1, 0, 1) if kind == "gpu" or plus else (-1, 0)


def second_tick_cases():
    return [case(kind, B, team, d, id="%s%+d" % (name, d))
            for kind, geo in GEO.items() for B, name, team, plus in second_tick_boundaries(geo) for d in later_deltas(kind, plus)]


def later_pool(n, team, seed, pred="sparse"):
    return team_pool(n, "2v2", seed) if team else pair_pool(n, pred, seed)


def later_pred(kind, B):
    """The shim pays for every pass of a tiled chain (geometry.pair_plan): from PL_MAX on its later ticks use the dense predicate."""
    return "dense" if kind != "gpu" and B >= GEO[kind]["PL_MAX"] else "sparse"


@pytest.mark.parametrize("kind,B,team,delta", second_tick_cases())
def test_second_tick_starts_at_an_exact_length(engine_cls, oracle_cls, kind, B, team, delta):
    """Tick once, read the depth d from the ORACLE, enqueue B - d + delta more, tick again: the second tick starts at
    exactly B + delta queued players behind whatever the first tick left in the lobby."""
    geo = GEO[kind]
    n0 = max(B // 2, 8)
    r0, c0, mode = later_pool(n0, team, 3, later_pred(kind, B))
    tag = "%s second tick B=%d%+d" % (kind, B, delta)
    with Pair(engine_cls(kind), oracle_cls, one_group([mode], 2 * B + 64)) as p:
        p.enqueue(r0, c0)
        p.tick(tag + " (first)")
        d = int(p.b.queue_depth(0)[0])
        assert 0 < d < B + delta, (tag, d)
        r1, c1, _ = later_pool(B + delta - d, team, 4, later_pred(kind, B))
        p.enqueue(r1, c1)
        assert int(p.b.queue_depth(0)[0]) == B + delta
        p.tick(tag)
        ps = p.a.path_stats()
        if team and B == geo["TT_MIN"]:
            assert bool(ps["paths"] & MM_PATH_TEAM) == (B + delta >= geo["TT_MIN"]), (tag, ps["paths"])
        if not team and B == geo["PL_MAX"]:
            assert (ps["pair_tiled_passes"] >= 1) == (B + delta >= geo["PL_MAX"]), (tag, ps)


def cancel_tick_cases():
    """The second-tick subset and the eight rows of kp_init's unrolled loop (what lies behind the chain's end matters to it).
    On the shim the chains past PL_MAX run the head+tail variant only (geometry.pair_plan: what a long chain costs there)."""
    out = []
    for kind, geo in GEO.items():
        rows8 = 8 * geo["KP_INIT_ROW"]                     # (the unrolled loop's bound lets a thread in too early at B - 1, if at all)
        for B, name, team, plus in second_tick_boundaries(geo) + [(rows8, "init_8rows", False, False)]:
            for delta in later_deltas(kind, plus):
                for variant in ("spread", "head+tail"):
                    if kind != "gpu" and B > geo["PL_MAX"] and not team and variant == "spread":
                        continue
                    out.append(case(kind, B, team, delta, variant, id="%s%+d-%s" % (name, delta, variant)))
    return out


@pytest.mark.parametrize("kind,B,team,delta,variant", cancel_tick_cases())
def test_cancel_tick_starts_at_an_exact_length(engine_cls, oracle_cls, kind, B, team, delta, variant):
    """Enqueue B + delta + k, cancel k spread over the queue, tick: the purge at the head of the tick leaves exactly
    B + delta.  head+tail: the head of the queue is among the cancelled, and so is the player at index B + delta — the
    first entry BEHIND the chain's new end, which the purge does not overwrite — whose rating lies far outside everybody
    else's: nobody may read it (kp_init and kt_init read the queue eight rows at a time: a row too many takes that rating
    into the span, the span no longer fits the packed key, and the chain falls back to k_walk — same lobbies, which is
    why the path is asserted)."""
    geo = GEO[kind]
    k = 5
    n = B + delta + k
    rating, cons, mode = later_pool(n, team, 5, later_pred(kind, B))
    idx = np.linspace(1, n - 2, k).astype(np.int64)
    if variant == "head+tail":
        idx = np.concatenate([[0], np.linspace(2, n - k - 2, k - 2).astype(np.int64), [n - k]])
        rating[n - k] = -(1 << 30)                              # (outside every group: the default group takes it)
    assert np.unique(idx).size == k
    tag = "%s cancel tick B=%d%+d %s" % (kind, B, delta, variant)
    with Pair(engine_cls(kind), oracle_cls, one_group([mode], n + 8)) as p:
        s = p.enqueue(rating, cons)
        p.cancel(s[idx])
        p.tick(tag)
        ps = p.a.path_stats()
        if team:
            assert bool(ps["paths"] & MM_PATH_TEAM) == (B + delta >= geo["TT_MIN"]), (tag, ps["paths"])
        else:
            assert (ps["pair_tiled_passes"] >= 1) == (B + delta >= geo["PL_MAX"]), (tag, ps)


# ------------------------------------------------------------------------------------------------------------------
# c. pair: the partner at an exact distance behind its anchor
# ------------------------------------------------------------------------------------------------------------------
FILLER = 1000


def distance_chain(pre, dists, tail=6):
    """`pre` fillers, then for every D of `dists`: an anchor A (rating 100 j), D - 1 fillers (rating 1000+: they fit one
    another, never an A), the partner P (rating 100 j + 5) — P sits exactly D positions behind A; D = 0 leaves P out
    (2^16 fillers behind an anchor nobody fits).  Returns rating, [(index of A, index of P or None)]."""
    rating, marks = [np.full(pre, FILLER, np.int32)], []
    at = pre
    for j, D in enumerate(dists):
        if D > 0:
            rating += [np.asarray([100 * j], np.int32), np.full(D - 1, FILLER, np.int32), np.asarray([100 * j + 5], np.int32)]
            marks.append((at, at + D))
            at += D + 1
        else:
            rating += [np.asarray([100 * j], np.int32), np.full(-D, FILLER, np.int32)]
            marks.append((at, None))
            at += 1 - D
    rating.append(np.full(tail, FILLER, np.int32))
    return np.concatenate(rating), marks


def pair_distance_cases():
    out = []
    for kind, geo in GEO.items():
        mid = geo["PK_T"] // 2                                   # an even number of fillers: they leave in pairs in front of A
        for X, name, gpu_only in G.pair_distances(geo):
            if kind != "gpu" and (gpu_only or X > G.shim_distance_max(geo)):
                continue
            for d in (-1, 0, 1):
                out.append(case(kind, 0, (X + d,), id="%s%+d-head" % (name, d)))
            out.append(case(kind, mid, (X,), id="%s-mid_tile" % name))
            out.append(case(kind, mid, (X - 1, X + 1, X), id="%s-three_pairs" % name))
        if kind == "gpu":
            for nobody in (geo["NX_FAR"], geo["NX_NONE"], geo["NX_NONE"] + 1, geo["NX_NONE"] + 2):
                out.append(case(kind, 0, (-nobody,), id="nobody_within_%d" % nobody))
                out.append(case(kind, mid, (geo["PK_T"], -nobody), id="pair_then_nobody_within_%d" % nobody))
    return out


@pytest.mark.parametrize("kind,pre,dists", pair_distance_cases())
def test_pair_partner_at_an_exact_distance(engine_cls, oracle_cls, kind, pre, dists):
    """Window 10, no filter.  Besides parity: the lobby (A, P) is in the tick's list — the distance was exercised —
    and an anchor without a partner is what the tick leaves in the stored lobby."""
    rating, marks = distance_chain(pre, dists)
    tag = "%s pre=%d distances=%s" % (kind, pre, dists)
    with Pair(engine_cls(kind), oracle_cls, one_group([mode_1v1(window=10)], rating.size + 8)) as p:
        s = p.enqueue(rating, cons_make(np.zeros(rating.size, np.int64)))
        m = p.tick(tag)
        first = {int(a): int(b) for a, b in m.slots}
        for ia, ip in marks:
            if ip is not None:
                assert first.get(int(s[ia])) == int(s[ip]), (tag, "lobby (A, P) missing", ia, ip)
            else:
                held, _ = p.a.lobby_state(0, 0)
                assert held.tolist() == [int(s[ia])], (tag, "the lone anchor is not in the stored lobby", held)


# ------------------------------------------------------------------------------------------------------------------
# d. team: chains of exact length; the only fitting players of a role at an exact distance
# ------------------------------------------------------------------------------------------------------------------
def team_length_cases():
    out = []
    for kind, geo in GEO.items():
        for entry in G.team_boundaries(geo):
            for n, shapes in G.team_plan(entry, geo, shim=kind != "gpu"):
                for shape in shapes:
                    out.append(case(kind, entry[0], n, shape, id="%s-%d-%s" % (entry[1], n, shape)))
    return out


@pytest.mark.parametrize("kind,B,n,shape", team_length_cases())
def test_team_tick_starts_at_an_exact_length(engine_cls, oracle_cls, kind, B, n, shape):
    geo = GEO[kind]
    rating, cons, mode = team_pool(n, shape)
    tag = "%s B=%d n=%d %s" % (kind, B, n, shape)
    with Pair(engine_cls(kind), oracle_cls, one_group([mode], n + 8)) as p:
        p.enqueue(rating, cons)
        assert int(p.b.queue_depth(0)[0]) == n
        p.tick(tag)
        # TT_MIN is the one team boundary mm_path_stats tells apart (chunks, staged words and kt_late's reach leave no
        # counter of their own): shorter chains stay with k_walk
        paths = p.a.path_stats()["paths"]
        assert bool(paths & MM_PATH_TEAM) == (geo["TT_MIN"] <= n <= geo["TT_MAX"]), (tag, paths)


def team_distance_chain(geo, sub, pos, total):
    """2v2, roles (1, 1), window 10.  The anchor A and its team-mate-to-be A2 (role 0, rating 0), then `sub` role-1
    players that do NOT fit A (rating 1000) and then the only two that do (rating 5): they sit `sub` entries down the
    role-1 sub-queue behind A.  Role-0 fillers of rating 3000 (no role 1 ever fits them) put the first of the two `pos`
    positions behind A (pos = 0: directly behind the `sub`) and bring the chain to `total` players."""
    R, C = [0, 0], [0, 0]
    gap = max(0, pos - 2 - sub) if pos else 0
    step = gap // (sub + 1) if sub else gap
    for i in range(sub):
        R += [3000] * step + [1000]
        C += [0] * step + [1]
    R += [3000] * (gap - step * sub)
    C += [0] * (gap - step * sub)
    ip = len(R)
    R += [5, 5]
    C += [1, 1]
    pad = max(0, total - len(R))
    R += [3000] * pad
    C += [0] * pad
    return np.asarray(R, np.int32), cons_make(0, 0, 0, np.asarray(C, np.uint32)), ip


def team_distance_cases():
    out = []
    for kind, geo in GEO.items():
        total = max(geo["TT_MIN"], 2 * geo["TT_CH"]) + 7
        for X, name, tuning in ((geo["TF_PAD"], "TF_PAD", None), (geo["team_cap"], "team_cap", None), (8, "team_cap=8", {"team_cap": 8})):
            for d in (-1, 0, 1):
                out.append(case(kind, X + d, 0, total, tuning, id="sub-%s%+d" % (name, d)))
        for X, name in ((1 << geo["TF_FAR_BITS"], "2^TF_FAR_BITS"), (geo["TF_BW"] * 32, "TF_BWx32")):
            for d in (-1, 0, 1):
                out.append(case(kind, 3, X + d, max(total, X + geo["TT_CH"] + 9), None, id="pos-%s%+d" % (name, d)))
    return out


@pytest.mark.parametrize("kind,sub,pos,total,tuning", team_distance_cases())
def test_team_member_at_an_exact_distance(engine_cls, oracle_cls, kind, sub, pos, total, tuning):
    """The staged sub-queue window (TF_PAD), the entries a thread of kt_f looks at (TT_SCAN_CAP / team_cap, also set to 8),
    the 16-bit record of a member's position (2^TF_FAR_BITS: TT_FAR) and the staged bitmap words (TF_BW x 32 positions)."""
    geo = GEO[kind]
    rating, cons, ip = team_distance_chain(geo, sub, pos, total)
    if pos:
        assert ip == pos, (ip, pos)
    tag = "%s sub=%d pos=%d n=%d tuning=%s" % (kind, sub, pos, rating.size, tuning)
    with Pair(engine_cls(kind), oracle_cls, one_group([mode_team(2, 2, 10, (1, 1))], rating.size + 8), tuning) as p:
        s = p.enqueue(rating, cons)
        m = p.tick(tag)
        assert p.a.path_stats()["paths"] & MM_PATH_TEAM, tag
        assert sorted(m.slots[0].tolist()) == sorted(int(x) for x in s[[0, 1, ip, ip + 1]]), (tag, m.slots[0], ip)


# ------------------------------------------------------------------------------------------------------------------
# e. a pool that is full to the last slot at a boundary
# ------------------------------------------------------------------------------------------------------------------
def full_pool_cases():
    out = []
    for kind, geo in GEO.items():
        out += [case(kind, geo["PL_MAX"], False, id="PL_MAX"), case(kind, geo["TT_MIN"], True, id="TT_MIN"),
                case(kind, geo["PL_MAX"] + 37, False, id="PL_MAX+37"), case(kind, geo["TT_MIN"] + 37, True, id="TT_MIN+37")]
    return out


@pytest.mark.parametrize("kind,n,team", full_pool_cases())
def test_full_pool_at_a_boundary(engine_cls, oracle_cls, kind, n, team):
    """capacity == n exactly (also a capacity that is no power of two): the enqueue succeeds, one more player is refused
    with MM_ERR_FULL by both and changes nothing, the tick is the oracle's."""
    rating, cons, mode = later_pool(n, team, 6)
    tag = "%s full pool n=%d" % (kind, n)
    with Pair(engine_cls(kind), oracle_cls, one_group([mode], n)) as p:
        p.enqueue(rating, cons)
        for eng in (p.a, p.b):
            with pytest.raises(MMError) as err:
                eng.enqueue(rating[:1], cons[:1])
            assert err.value.status == MM_ERR_FULL, (tag, err.value)
        assert int(p.a.queue_depth(0)[0]) == int(p.b.queue_depth(0)[0]) == n
        m = p.tick(tag)
        if m.slots.size:                                         # the slots the tick released are handed out again, all of them
            p.enqueue(rating[:m.slots.size], cons[:m.slots.size])
            assert int(p.b.queue_depth(0)[0]) + len(p.b.lobby_state(0, 0)[0]) == n
            p.tick(tag + " (refill)")


# ------------------------------------------------------------------------------------------------------------------
# the tables themselves
# ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", sorted(KINDS))
def test_the_tables_name_every_boundary(kind):
    """What the tables must hold (the constants by name, the lengths derived from them), that a missing constant is an
    error, and that every entry is aimed at by a case of this engine's tier at B - 1 and at B."""
    assert kind in GEO, GEO_ERRORS[kind]
    geo = GEO[kind]
    T, cap, pt = geo["PK_T"], G.tiles_cap(geo), geo["pair_ptiles"]
    pair = {b for b, _, _, _ in G.pair_boundaries(geo)}
    want = {64, 1024, 8 * 1024, geo["PL_COMPACT_MIN"], geo["PL_MAX"], (pt + 1) * T, geo["PK_TILES_MAX"] * T, geo["PK_GROUP_MIN"] * T,
            geo["NXI_STAGE"], geo["NXI_SEG"], geo["NX_SEG_MIN"], geo["NX_FAR"], geo["NX_NONE"], 1 << 16}
    # the codes of nx16: 16 bits, and no offset a walk stores (inside two tiles, or a chain below PL_MAX) can look like one
    assert geo["NX_FAR"] < geo["NX_NONE"] == 0xFFFF and max(2 * T, geo["PL_MAX"]) < geo["NX_FAR"]
    for t in (T, T // 2, T // 4):
        want |= {t, 2 * t, cap * t, pt * t}
    assert want <= pair, sorted(want - pair)
    team = {b for b, _, _, _ in G.team_boundaries(geo)}
    want = {geo["TT_MIN"], geo["TF_BW"] * 32, 1 << geo["TF_FAR_BITS"], geo["TL_BITS_MAX"]} | {geo["TT_CH"] * k for k in (1, 2, 8, 9, 32, 33)}
    assert want <= team, sorted(want - team)
    texts = G.source_defines()
    del texts["PL_MAX"]
    with pytest.raises(KeyError):
        G._value("PL_MAX", texts)
    with pytest.raises(KeyError):
        G._value("PL_WORDS", texts)                              # (a constant defined through a missing one)
    aimed = {(c.values[1], c.values[2]) for c in pair_length_cases() if c.values[0] == kind}
    for b, name, _, gpu_only in G.pair_boundaries(geo):
        if kind == "gpu" or not gpu_only:
            assert (b, b - 1) in aimed and (b, b) in aimed, (kind, name)
    aimed = {(c.values[1], c.values[2]) for c in team_length_cases() if c.values[0] == kind}
    for b, name, _, gpu_only in G.team_boundaries(geo):
        if kind == "gpu" or not gpu_only:
            assert (b, b - 1) in aimed and (b, b) in aimed, (kind, name)
