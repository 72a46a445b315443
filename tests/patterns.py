"""Deterministic pools in STRUCTURED arrival orders, each with what Mode R must do with it in closed form.

Pure numpy; imports no engine.  Every other differential test draws ratings, regions and roles i.i.d.; for a FIFO
first-fit search the ORDER decides how far an anchor's partner lies, how many lobbies a pass seats and how many passes a
tick has.  A family here returns a Case: the mode, and a script of steps

    ("enqueue", rating:int32[n], cons:uint32[n])      in arrival order
    ("cancel", idx)                                   positions in the concatenation of everything enqueued so far
    ("tick", Expect)                                  what docs/MATCH_CHECK.md says this tick does

All families live in ONE rating group, GROUP = (0, 10**7): the chain is everybody enqueued.

How the closed forms are derived (docs/MATCH_CHECK.md sections 2-5, nothing read off an engine).  A pass pops every
queued player once, in order (section 4).  A popped player meets the open lobby (section 3): an EMPTY lobby takes him as
its anchor — no predicate is evaluated, so no pair is counted (section 5) — otherwise one pair is counted and he is
seated if he fits the anchor and a team has room for his role (section 2), else he goes back to the tail.  A filled
lobby is emitted and the next popped player opens a new one; an unfilled lobby is carried into the next pass.  The tick
ends after the first pass that seats nobody, or when the queue is empty.  So a tick is described pass by pass by three
numbers: `qlen` (players queued at the start of the pass), `opened` (lobbies opened by an anchor in it) and `lobbies`
(lobbies emitted in it), and

    pairs = sum over the passes of (qlen - opened)         every pop that did not open a lobby met an anchor
    qlen of the next pass = qlen - players seated in this one

Each family's docstring walks its own order through these rules and states (qlen, opened, lobbies) per pass; Expect
derives lobbies, passes, the lobbies-per-pass list and pairs from that.

Lengths and distances are arguments: tests take them from tests/geometry.py (wave 64, the tile lengths T, the 2T
horizon, PL_MAX, PL_COMPACT_MIN, TT_MIN, TT_CH, TF_BW, TT_SCAN_CAP, 2^TF_FAR_BITS), so the same family lands on the same
branch of the tiny shim geometry and of the product's."""
from dataclasses import dataclass, field

import numpy as np

GROUP = (0, 10 ** 7)
STEP = 4                # rating step between values that must NOT fit one another (66 000 of them span 264 000 ratings)
WINDOW = 3              # < STEP
FAR = 400_000           # a rating nobody of a pool comes near
# The packed keys of the pair and team paths hold a chain's rating SPAN in 19 bits (mm_pair.inc / mm_team.inc
# PK_SPAN_BITS: a wider chain is walked by k_walk): every family stays inside, or it would test the generic walk only.
SPAN_MAX = {"1v1": (1 << 19) - 1, "team": (1 << 19) - 1}


def cons(n, region=0, role=0, mode=0):
    """include/mm_engine.h MM_CONS_*: mode (4 bits) | region (8) << 4 | party (4) << 12 | role (4) << 16."""
    z = np.zeros(n, np.uint32)
    return (z + np.uint32(mode)) | (np.asarray(region, np.uint32) + z) << np.uint32(4) | (np.asarray(role, np.uint32) + z) << np.uint32(16)


@dataclass
class Expect:
    """passes: [(qlen, opened, lobbies)] or None (no closed form for the pass structure: `lobbies` and `first_pass` then).
    stored / depth: players in the stored lobby / queued after the tick."""
    passes: list = None
    stored: int = 0
    depth: int = 0
    lobbies: int = None
    first_pass: int = None        # lobbies of pass 0 where `passes` is None
    min_passes: int = 1           # the regime where `passes` is None

    def __post_init__(self):
        if self.passes is not None:
            self.lobbies = sum(p[2] for p in self.passes)

    @property
    def n_passes(self):
        return len(self.passes)

    @property
    def per_pass(self):
        return [p[2] for p in self.passes]

    @property
    def pairs(self):
        return sum(q - o for q, o, _ in self.passes)

    @property
    def max_in_a_pass(self):
        return max(self.per_pass, default=0)


@dataclass
class Case:
    family: str
    params: dict
    mode: tuple                    # ("1v1", window, region_filter) | ("team", team_size, teams, window, quota)
    steps: list = field(default_factory=list)

    def __post_init__(self):
        r = np.concatenate([s[1] for s in self.steps if s[0] == "enqueue"]).astype(np.int64)
        assert GROUP[0] <= r.min() and r.max() - r.min() <= SPAN_MAX[self.mode[0]], (str(self), r.min(), r.max())

    @property
    def lobby_size(self):
        return 2 if self.mode[0] == "1v1" else self.mode[1] * self.mode[2]

    @property
    def players(self):
        return sum(s[1].size for s in self.steps if s[0] == "enqueue")

    def __str__(self):
        return "%s(%s)" % (self.family, ", ".join("%s=%s" % kv for kv in self.params.items()))


PAIR = ("1v1", WINDOW, False)


def _one_tick(family, params, mode, rating, cs, expect, cancel=None):
    steps = [("enqueue", np.asarray(rating, np.int32), np.asarray(cs, np.uint32))]
    if cancel is not None and len(cancel):
        steps.append(("cancel", np.asarray(cancel, np.int64)))
    steps.append(("tick", expect))
    return Case(family, params, mode, steps)


# ----------------------------------------------------------------------------------------------------------------------
# pair (1v1) families
# ----------------------------------------------------------------------------------------------------------------------
def _nested_passes(k, L=2, extra=0):
    # pass j: L (k - j) players of the family (+ `extra` that fit nobody) queued, the head opens the only lobby
    return [(L * (k - j) + extra, 1, 1) for j in range(k)]


def nested(k):
    """up ++ reversed(up), up = k ratings STEP apart, window < STEP: only equal ratings fit.
    Pass j (k - j values left, queue u_j .. u_k-1, u_k-1' .. u_j'): u_j opens the lobby, 2 (k - j) - 2 players are
    rejected, the LAST queued player u_j' is its partner.  One lobby per pass, k passes, then the queue is empty;
    pairs = sum (2 (k - j) - 1) = k^2."""
    up = np.arange(k, dtype=np.int64) * STEP
    e = Expect(_nested_passes(k))
    assert e.pairs == k * k
    return _one_tick("nested", {"k": k}, PAIR, np.concatenate([up, up[::-1]]), cons(2 * k), e)


def _shifted_passes(k, L=2):
    """up ++ up' generalised to lobbies of L: k anchors a_0 .. a_k-1, then k member blocks M_0 .. M_k-1 of L - 1 players
    (M_i fits a_i only).  State at the start of a pass: `a` values are used up, and either nothing is carried or the
    lobby holds M_a whole (L - 1 players, opened by M_a's first).  qlen = L (k - a) - (L - 1 if carried).
    In the pass: carried -> the head a_a completes it (lobby 1), a += 1.  Then, a < k: a_a opens, M_a completes (lobby),
    a += 1; then, a < k: the first of M_a opens and the rest of M_a is seated behind it — carried into the next pass."""
    out, a, carried = [], 0, False
    while a < k:
        q = L * (k - a) - ((L - 1) if carried else 0)
        opened = lob = 0
        if carried:
            lob, a, carried = lob + 1, a + 1, False
        if a < k:
            opened, lob, a = opened + 1, lob + 1, a + 1
            if a < k:
                opened, carried = opened + 1, True
        out.append((q, opened, lob))
    return out


def shifted(d):
    """up ++ up with k = d values: in pass 0 the anchor u_0 has its partner u_0' EXACTLY d positions behind it.  Then
    u_1' opens a lobby nobody behind it fits and is carried; pass 1: the head u_1 fits it at once, u_2 opens and finds
    u_2' d - 2 positions behind, u_3' is carried ... two lobbies a pass, the distance shrinking by 2: d // 2 + 1 passes,
    d lobbies (see _shifted_passes for qlen and opened)."""
    up = np.arange(d, dtype=np.int64) * STEP
    e = Expect(_shifted_passes(d))
    assert e.n_passes == d // 2 + 1 and e.lobbies == d
    return _one_tick("shifted", {"d": d}, PAIR, np.concatenate([up, up]), cons(2 * d), e)


def stretches(d, count, tail=2):
    """EVERY anchor of pass 0 has its partner exactly d positions behind it, inside a chain of any length: `count` times an
    anchor, d - 1 fillers (one rating of their own, FAR from every anchor's) and the partner, then `tail` (even) fillers.
    Pass 0: each anchor opens, its fillers are rejected, its partner fits; the tail pairs up in order: count + tail / 2
    lobbies.  Pass 1: the F = count (d - 1) fillers pair up in order, an odd one is left in the stored lobby.
    shifted(d) cannot put a partner on the horizon's end of a TILED chain — its chain of 2d players is cut into tiles of
    at most d / 2 — this family can: the first anchor sits on a tile's first position, the others anywhere in theirs."""
    assert tail % 2 == 0
    F = count * (d - 1)
    r = np.concatenate([np.concatenate([[(s + 1) * STEP], np.full(d - 1, FAR), [(s + 1) * STEP]]) for s in range(count)] + [np.full(tail, FAR)])
    ps = [(r.size, count + tail // 2, count + tail // 2)] + ([(F, (F + 1) // 2, F // 2)] if F else [])
    return _one_tick("stretches", {"d": d, "count": count}, PAIR, r, cons(r.size), Expect(ps, stored=F % 2))


def decoy(p, n):
    """A REPAIRED pointer with the second fit at an exact position.  Ratings W = 0, X = 6, Y1 = 3 (window 3: W and X both
    fit Y1, W does not fit X), O = 900, then fillers that fit nobody (four apart from 1000 up), Y2 = 6 at position p, more
    fillers, and O' = 900 last.  Pass 0: W opens, X is rejected, Y1 fits W; O opens, everybody is rejected, O' fits: two
    lobbies, and X's first fit (Y1, what next[X] says) has left the queue.  Pass 1: X, at position 1 of the same
    layout, opens; its next fit is Y2, p - 1 positions on — found by the repair, or by the walk's scan when p lies past
    the horizon; the filler behind Y2 opens a lobby nobody fits.  Pass 2 seats nobody: X and Y2 are the tick's third
    lobby, that filler is stored, n - 7 fillers stay queued."""
    assert 4 < p < n - 3
    F = n - 6
    r = np.concatenate([[0, 6, 3, 900], 1000 + 4 * np.arange(F), [900]])
    r = np.insert(r, p, 6)
    assert r.size == n and r[p] == 6 and r[-1] == 900
    return _one_tick("decoy", {"p": p, "n": n}, PAIR, r, cons(n), Expect([(n, 2, 2), (n - 4, 2, 1), (n - 7, 0, 0)], stored=1, depth=n - 7))


def in_order(n, reverse=False):
    """Arrival order = rating order: ratings 0 0 1 1 2 2 ... (reverse: descending in the same pairs), window 0.  Player 2j opens, 2j + 1 is the first to be
    asked and fits.  One pass, n // 2 lobbies, as many pairs; an odd n leaves the last player in the stored lobby and
    the queue empty.  (A million players span 2^19 ratings: inside the packed key.)"""
    r = np.arange(n, dtype=np.int64) // 2
    e = Expect([(n, (n + 1) // 2, n // 2)], stored=n % 2)
    return _one_tick("reverse_sorted" if reverse else "sorted", {"n": n}, ("1v1", 0, False), r.max() - r if reverse else r, cons(n), e)


def runs(B, levels):
    """3^levels blocks of B equal ratings, alternating between two values more than a window apart (X Y X Y ...).
    B even: every block pairs up inside itself, one pass.  B odd: block 0 (X) pairs up and its last player opens a lobby;
    block 1 (Y) is rejected whole — the carried anchor reaches over a whole foreign run; the head of block 2 (X) fits,
    the other B - 1 pair up; block 3 starts as block 0 did.  Per triple of blocks: 3B queued, B lobbies, B opened
    ((B + 1) / 2 in its first block, (B - 1) / 2 in its third).  What is rejected — every third block — alternates
    between the two values again: the next pass sees the same family with a third of the blocks.  After `levels` passes
    one block is left: (B - 1) / 2 lobbies, (B + 1) / 2 opened, its last player stays in the stored lobby, queue empty."""
    nb = 3 ** levels
    r = np.repeat(np.where(np.arange(nb) % 2 == 0, 1000, 2000), B)
    if B % 2 == 0:
        e = Expect([(nb * B, nb * B // 2, nb * B // 2)])
    else:
        ps = [((nb // 3 ** p) * B, (nb // 3 ** (p + 1)) * B, (nb // 3 ** (p + 1)) * B) for p in range(levels)]
        e = Expect(ps + [(B, (B + 1) // 2, (B - 1) // 2)], stored=1)
    return _one_tick("runs", {"B": B, "levels": levels}, PAIR, r, cons(r.size), e)


def interleaved(R, c):
    """One rating, region i % R with the region filter on, 2 R c players: R interleaved sub-chains, the partner of
    player i is i + R.  Pass 0: the head of every stretch of R + 1 players opens, the next R - 1 are of other regions
    (rejected), the last fits: n // (R + 1) lobbies in pass 0.  Every region holds an even number of players and a
    carried anchor's region always has an odd number left in the queue, so no anchor starves: n / 2 lobbies in all and an
    empty queue.  The pass structure after pass 0 has no closed form we trust: the regime (more than one pass) is read
    off the oracle."""
    n = 2 * R * c
    e = Expect(None, lobbies=n // 2, first_pass=n // (R + 1), min_passes=2)
    return _one_tick("interleaved", {"R": R, "c": c}, ("1v1", WINDOW, True), np.full(n, 1000), cons(n, region=np.arange(n) % R), e)


def blocked_head(n, then):
    """One head player (rating FAR) nobody fits, in front of n (even) players in rating order.
    Tick 1: the head opens the lobby, n rejections; the second pass seats nobody either (n more pairs) and ends the
    tick: zero lobbies, the queue unchanged, the head stored.
    then = "partner": the head's only partner arrives at the tail.  Pass 0: n rejections, the partner fits (1 lobby);
        pass 1: the pool in rating order, n / 2 lobbies; the queue is empty.
    then = "cancel": the head is cancelled instead.  The first attempt of the next tick judges player 0 against the
        STALE lobby (one pair, rejected), then the lobby is filtered (MATCH_CHECK section 4): players 1 .. n-1 pair up in
        order, (n - 2) / 2 lobbies, player n-1 opens a lobby and is carried; pass 1: player 0 meets it, n - 1 steps of
        WINDOW away: rejected, the tick ends with player 0 queued and player n-1 stored."""
    assert n % 2 == 0 and n >= 4
    r = np.concatenate([[FAR], np.arange(n, dtype=np.int64) * WINDOW])
    steps = [("enqueue", r.astype(np.int32), cons(n + 1)),
             ("tick", Expect([(n + 1, 1, 0), (n, 0, 0)], stored=1, depth=n))]
    if then == "partner":
        steps += [("enqueue", np.asarray([FAR + 1], np.int32), cons(1)), ("tick", Expect([(n + 1, 0, 1), (n, n // 2, n // 2)]))]
    else:
        steps += [("cancel", np.asarray([0])), ("tick", Expect([(n, n // 2, (n - 2) // 2), (1, 0, 0)], stored=1, depth=1))]
    return Case("blocked_head", {"n": n, "then": then}, PAIR, steps)


def carried_head(n):
    """One player alone, then n (even) more of his rating.
    Tick 1: he opens the lobby and the queue is empty: one pass, no lobby, he is stored.
    Tick 2: player 0 meets the stored lobby and fits (one pair, one lobby, nobody opened it in this pass); players
        1 .. n-1 pair up in order, (n - 2) / 2 lobbies, and player n-1 opens a lobby and stays in it: one pass, n / 2
        lobbies, n / 2 opened, the queue empty.
    What it is for: the LDS-resident walk hands its steps to the consumer through a ring of 512 (mm_pair.inc PL_RING, the
    same in every geometry).  The carried anchor's step is the ring's first, so the blocks of 64 steps that follow lie at
    1 + 64 j: n / 2 > 512 makes one of them wrap around the ring's end and the producer wait for room."""
    assert n % 2 == 0 and n >= 2
    steps = [("enqueue", np.full(1, 1000, np.int32), cons(1)), ("tick", Expect([(1, 1, 0)], stored=1)),
             ("enqueue", np.full(n, 1000, np.int32), cons(n)), ("tick", Expect([(n, n // 2, n // 2)], stored=1))]
    return Case("carried_head", {"n": n}, PAIR, steps)


DENSE = ("1v1", 10 ** 6, False)     # everybody fits everybody: the survivors of the cancels pair up in order


def dead(n, dead_idx, name):
    """n players in rating order who ALL fit one another (window past the span), `dead_idx` cancelled before the tick.
    A cancelled entry vanishes when popped and counts no pair (MATCH_CHECK section 4): the S survivors pair up in order,
    one pass, S // 2 lobbies; an odd S leaves the last survivor stored.  S = 0: no pass at all."""
    dead_idx = np.unique(np.asarray(dead_idx, np.int64))
    S = n - dead_idx.size
    e = Expect([(S, (S + 1) // 2, S // 2)] if S else [], stored=S % 2)
    return _one_tick("dead", {"n": n, "variant": name, "cancelled": int(dead_idx.size)}, DENSE, np.arange(n), cons(n), e, dead_idx)


def dead_variants(n, T):
    """The structured cancels of the issue over a pool of n >= 3 T players: a whole middle tile, the first tile, every
    second player, everyone but the first and the last."""
    mid = (n // T // 2) * T
    return [dead(n, np.arange(mid, mid + T), "middle_tile"), dead(n, np.arange(T), "first_tile"),
            dead(n, np.arange(1, n, 2), "every_second"), dead(n, np.arange(1, n - 1), "all_but_first_and_last")]


def nested_dead(k):
    """nested(k) with the middle third of the values cancelled on both sides: nested over the k' values left."""
    up = np.arange(k, dtype=np.int64) * STEP
    gone = np.arange(k // 3, 2 * k // 3)
    kk = k - gone.size
    return _one_tick("nested_dead", {"k": k}, PAIR, np.concatenate([up, up[::-1]]), cons(2 * k),
                     Expect(_nested_passes(kk)), np.concatenate([gone, 2 * k - 1 - gone]))


def alive_share(c, prefix, k, loner):
    """The alive share after pass 0, set by the cancel count.  Enqueued: c + prefix players of one rating (prefix even),
    nested(k) behind them with `loner` (0 / 1) players nobody fits in its middle (popped while a lobby is open in every
    pass, so rejected, never an anchor before he is alone); the first c are cancelled.  The tick
    starts with m = prefix + 2k + loner players.  Pass 0: the prefix pairs up (prefix / 2 lobbies), u_0 opens and its
    partner is the last of the nested part: 2k - 2 + loner are alive after it — the number the kernels compare with m
    (tiled path: compaction when alive * 4 < m * 3; LDS-resident path: m > PL_COMPACT_MIN and alive * 2 < m).  Then
    nested's passes with the loner rejected in every one, and a last pass in which the loner opens a lobby alone."""
    assert prefix % 2 == 0 and loner in (0, 1) and k >= 2
    up = 1000 + np.arange(k, dtype=np.int64) * STEP
    r = np.concatenate([np.full(c + prefix, 500), up, np.full(loner, FAR), up[::-1]])
    ps = [(prefix + 2 * k + loner, prefix // 2 + 1, prefix // 2 + 1)] + _nested_passes(k, extra=loner)[1:]
    if loner:
        ps.append((1, 1, 0))
    m, alive = prefix + 2 * k + loner, 2 * k - 2 + loner
    return _one_tick("alive_share", {"cancelled": c, "m": m, "alive": alive, "k": k}, PAIR, r, cons(r.size),
                     Expect(ps, stored=loner), np.arange(c))


def alive_share_at(m_min, num, den, delta, c):
    """alive_share with  den * alive - num * m == delta  (delta < 0: below the share num / den) and the smallest
    m >= m_min that allows it: den * alive - num * m = (den - num) 2k - 2 den + (den - num) loner - num * prefix."""
    for m in range(m_min, m_min + 64):
        for loner in (0, 1):
            # alive = (delta + num * m) / den, = 2k - 2 + loner
            if (delta + num * m) % den:
                continue
            alive = (delta + num * m) // den
            k2 = alive + 2 - loner
            prefix = m - k2 - loner
            if k2 % 2 == 0 and k2 >= 4 and prefix >= 0 and prefix % 2 == 0:
                return alive_share(c, prefix, k2 // 2, loner)
    raise ValueError((m_min, num, den, delta))


# ----------------------------------------------------------------------------------------------------------------------
# team families: "5v5" = team_size 5, 2 teams, quota (1, 1, 1, 1, 1); "2v2" = quota (2,); "3x2" = three teams of two
# ----------------------------------------------------------------------------------------------------------------------
SHAPES = {"5v5": ("team", 5, 2, WINDOW, (1, 1, 1, 1, 1)), "2v2": ("team", 2, 2, WINDOW, (2,)), "3x2": ("team", 2, 3, WINDOW, (2,))}


def _lobby_roles(shape):
    """Roles of L consecutive players that fill one lobby in ANY seating order: every role `teams` x quota times.
    (Section 2, step 3: a player is refused only when every team is full for his role.)"""
    _, ts, teams, _, quota = SHAPES[shape]
    return np.tile(np.repeat(np.arange(len(quota)), quota), teams)[:ts * teams]


def team_dense(shape, lobbies):
    """One rating, roles so that every L = team_size x teams consecutive players fill a lobby: the head of each stretch
    opens, the L - 1 behind it are seated one after another.  One pass, n / L lobbies, L - 1 pairs each."""
    roles = _lobby_roles(shape)
    n = lobbies * roles.size
    return _one_tick("team_dense", {"shape": shape, "lobbies": lobbies}, SHAPES[shape], np.full(n, 1000),
                     cons(n, role=np.tile(roles, lobbies)), Expect([(n, lobbies, lobbies)]))


def _anchors_and_members(shape, k, members_reversed):
    roles = _lobby_roles(shape)
    val = (1 + np.arange(k, dtype=np.int64)) * STEP
    order = val[::-1] if members_reversed else val
    rating = np.concatenate([val, np.repeat(order, roles.size - 1)])
    role = np.concatenate([np.full(k, roles[0]), np.tile(roles[1:], k)])
    return rating, cons(rating.size, role=role)


def team_nested(shape, k):
    """k anchors in ascending rating, then — in REVERSE order — for each anchor the L - 1 players of its rating that fill
    its lobby.  As nested: the head opens, everybody but the last L - 1 queued is rejected, one lobby per pass, k passes,
    pairs = sum (L (k - j) - 1)."""
    L = _lobby_roles(shape).size
    rating, cs = _anchors_and_members(shape, k, True)
    return _one_tick("team_nested", {"shape": shape, "k": k}, SHAPES[shape], rating, cs, Expect(_nested_passes(k, L)))


def team_shifted_blocks(shape, d):
    """d anchors, then their member blocks in the SAME order: the first fitting member of the pass-0 anchor sits exactly d
    positions behind it, and every later anchor's members lie a whole shrinking stretch away (_shifted_passes)."""
    L = _lobby_roles(shape).size
    rating, cs = _anchors_and_members(shape, d, False)
    e = Expect(_shifted_passes(d, L))
    assert e.lobbies == d and e.n_passes == d // 2 + 1
    return _one_tick("team_shifted_blocks", {"shape": shape, "d": d}, SHAPES[shape], rating, cs, e)


def team_shifted(shape, d, stretches):
    """EVERY anchor of pass 0 has its first fitting member exactly d positions behind it: `stretches` times an anchor,
    d - 1 fillers (one rating of their own, far from every anchor's), the L - 1 members of the anchor.  Pass 0: each
    anchor opens, its fillers are rejected, its members fill the lobby: `stretches` lobbies.  The fillers' roles run
    through a lobby's roles over and over, so in pass 1 every L of them in a row fill a lobby; F mod L of them are
    left in the stored lobby, and the queue is empty."""
    roles = _lobby_roles(shape)
    L, F = roles.size, stretches * (d - 1)
    frole = roles[np.arange(F) % L].reshape(stretches, d - 1)
    rating, role = [], []
    for s in range(stretches):
        rating += [[(s + 1) * STEP], np.full(d - 1, FAR), np.full(L - 1, (s + 1) * STEP)]
        role += [[roles[0]], frole[s], roles[1:]]
    rating, role = np.concatenate(rating), np.concatenate(role)
    ps = [(rating.size, stretches, stretches)] + ([(F, -(-F // L), F // L)] if F else [])
    return _one_tick("team_shifted", {"shape": shape, "d": d, "stretches": stretches}, SHAPES[shape], rating,
                     cons(rating.size, role=role), Expect(ps, stored=F % L))


def scarce_role_at_the_tail(q):
    """5v5, one rating.  Roles 0-3 round-robin, 4q players each, and the 4q players of role 4 only at the tail (20q in
    all, 2q lobbies).  Pass 0: the first 8 are seated (two per role), everybody up to the tail is rejected, two of role 4
    fill the lobby; the third opens a new one, the fourth joins it, the rest is rejected: 1 lobby, 2 opened, 12 seated.
    Passes 1 .. q-1 start with two of role 4 in the lobby: the first 8 fill it, the next 8 open and half fill another,
    the tail completes it and leaves two more seated: 2 lobbies, 2 opened, 20 seated.  That uses up the tail; the last
    pass finds 8 players queued, who fill the carried lobby: 1 lobby, nothing opened.  q + 1 passes."""
    m = 4 * q
    role = np.concatenate([np.arange(4 * m) % 4, np.full(m, 4)])
    ps = [(20 * q, 2, 1)] + [(20 * q - 12 - 20 * (p - 1), 2, 2) for p in range(1, q)] + [(8, 0, 1)]
    e = Expect(ps)
    assert e.lobbies == 2 * q
    return _one_tick("scarce_role_at_the_tail", {"q": q}, SHAPES["5v5"], np.full(5 * m, 1000), cons(5 * m, role=role), e)


def role_sorted(t):
    """5v5, one rating, m = 10t + 2 players of role 0 first, then m of role 1, ... m of role 4 (m / 2 = 5t + 1 lobbies).
    A lobby takes two players of each role.  Pass 0: two of every block are seated, the second of role 4 fills the lobby;
    the third of role 4 opens the next, the fourth joins: 12 seated, 2 opened, 1 lobby, {4} carried.  From then on a
    period of four passes: with roles {4} carried the blocks 0-3 fill the lobby (8 seated), the third of role 3 opens and
    roles 3, 4 give two each (12 seated, 1 opened, 1 lobby, {3, 4} carried); likewise with {3, 4} and {2, 3, 4} carried;
    with {1, 2, 3, 4} carried role 0 fills it, its next two open a lobby that ALL other blocks complete in the same pass,
    and role 4 starts another: 14 seated, 2 opened, 2 lobbies — in the last period role 4 is used up by then: 12 seated,
    1 opened, and the queue is empty.  1 + 4t passes."""
    m = 10 * t + 2
    ps, q = [], 5 * m
    ps.append((q, 2, 1))
    q -= 12
    for period in range(t):
        for _ in range(3):
            ps.append((q, 1, 1))
            q -= 12
        last = period == t - 1
        ps.append((q, 1 if last else 2, 2))
        q -= 12 if last else 14
    assert q == 0
    e = Expect(ps)
    assert e.lobbies == m // 2 and e.n_passes == 1 + 4 * t
    return _one_tick("role_sorted", {"t": t}, SHAPES["5v5"], np.full(5 * m, 1000), cons(5 * m, role=np.repeat(np.arange(5), m)), e)


def role_missing(m):
    """5v5, one rating, roles 0-3 round-robin (m each, m >= 5) and ONE player of role 4 in the middle.  Tick 1: two of
    each role 0-3 and the one of role 4 are seated, a second pass seats nobody: zero lobbies, 9 of 10 stored.
    Tick 2, after one more player of role 4 arrived at the tail: pass 0 rejects everybody and seats him (1 lobby); pass 1
    opens a lobby with the next 8; pass 2 seats nobody."""
    assert m >= 5
    role = np.arange(4 * m) % 4
    role = np.concatenate([role[:2 * m], [4], role[2 * m:]])
    n = role.size
    steps = [("enqueue", np.full(n, 1000, np.int32), cons(n, role=role)),
             ("tick", Expect([(n, 1, 0), (n - 9, 0, 0)], stored=9, depth=n - 9)),
             ("enqueue", np.full(1, 1000, np.int32), cons(1, role=4)),
             ("tick", Expect([(n - 8, 0, 1), (n - 9, 1, 0), (n - 17, 0, 0)], stored=8, depth=n - 17))]
    return Case("role_missing", {"m": m}, SHAPES["5v5"], steps)


# ----------------------------------------------------------------------------------------------------------------------
# a random family with a parameter from the geometry tables (tests/stress.py --patterns)
# ----------------------------------------------------------------------------------------------------------------------
def draw(rng, geo, team, max_players, max_passes):
    """One Case: the family and its parameter drawn from `geo` (tests/geometry.py's dict, computed from the drawn tuning),
    lengths and distances jittered by -2 .. 2 around the boundaries.  A draw that is too large for the tier (players,
    passes of its first tick) is drawn again."""
    T, PL, PC = geo["PK_T"], geo["PL_MAX"], geo["PL_COMPACT_MIN"]
    cap = min(geo["pair_ptiles"], geo["pair_tiles_max"])

    def j(x, lo=2):
        return max(lo, int(x) + int(rng.integers(-2, 3)))

    def pick(*xs):
        return xs[int(rng.integers(0, len(xs)))]

    pair = [
        lambda: nested(j(pick(32, T // 4, T // 2, PL // 2, PL // 2 + T // 2, T))),
        lambda: nested_dead(j(pick(48, T // 2, PL // 2 + T // 4), 6)),
        lambda: shifted(j(pick(63, 64, 65, T // 4, T // 2, T, 2 * T, PL, cap * T // 4))),
        lambda: in_order(j(pick(64, T, PL, 4 * T, (geo["pair_ptiles"] + 1) * T, cap * T)), reverse=bool(rng.integers(0, 2))),
        lambda: runs(pick(1, 63, 64, 65, T - 1, T + 1, T // 4 + 1), int(rng.integers(1, 4))),
        lambda: interleaved(pick(2, 64, 255, 256), int(rng.integers(1, max(2, 4 * T // 256)))),
        lambda: blocked_head(2 * (j(pick(64, T, PL, 2 * PL), 4) // 2), pick("partner", "cancel")),
        lambda: pick(*dead_variants(pick(3, 4, 6) * T + int(rng.integers(0, 3)), T)),
        lambda: alive_share_at(pick(PL, PL + T // 2, 2 * PL), 3, 4, int(rng.integers(-2, 3)), pick(1, 64, T)),
        lambda: alive_share_at(pick(PC + 2, (PC + PL) // 2), 1, 2, int(rng.integers(-2, 3)), pick(1, 64, T)),
    ]
    tt, ch, sc, bw = geo["TT_MIN"], geo["TT_CH"], geo["team_cap"], geo["TF_BW"] * 32

    def shape():
        return pick(*SHAPES)

    def L(s):
        return SHAPES[s][1] * SHAPES[s][2]

    def shifted_team():
        s, d = shape(), j(pick(sc, geo["TT_SCAN_CAP"], ch, 2 * ch, 1 << min(geo["TF_FAR_BITS"], 14), bw), 3)
        return team_shifted(s, d, int(rng.integers(1, 4)) + tt // (d + L(s)))

    teams = [
        lambda: (lambda s: team_dense(s, j(pick(tt, 2 * ch, 9 * ch) // L(s) + 1)))(shape()),
        lambda: (lambda s: team_nested(s, j(pick(tt // L(s) + 1, 2 * ch // L(s), 48))))(shape()),
        lambda: (lambda s: team_shifted_blocks(s, j(pick(tt // L(s) + 1, sc, ch // 2))))(shape()),
        shifted_team,
        lambda: scarce_role_at_the_tail(j(pick(tt // 20 + 1, 32, 2 * ch // 20))),
        lambda: role_sorted(j(pick(tt // 50 + 1, 8, ch // 25))),
        lambda: role_missing(j(pick(tt // 4 + 1, ch, 8), 5)),
    ]
    for _ in range(200):
        c = pick(*(teams if team else pair))()
        e = next(s[1] for s in c.steps if s[0] == "tick")
        if c.players <= max_players and (e.passes is None or e.n_passes <= max_passes):
            return c
    raise RuntimeError("no pattern fits %d players / %d passes" % (max_players, max_passes))
