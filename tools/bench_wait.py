#!/usr/bin/env python
"""What the engine clock (include/mm_wait.h) costs on BASELINE cfg-2's pool (1M players, 1v1, +-25 rating, region
filter): mm_expire at 0 %, 1 % and 50 % expired, mm_wait_stats, the tick with the clock on beside the same tick with it
off, the enqueue with stamps beside the enqueue without.  Medians over --steps steps (at least 20); both variants of a
pair run in the same process, step by step in turns.  The yardstick for mm_expire and mm_wait_stats is `bucket_ms`, the
HIP-event time of bucketing the same 1M players, measured here: both move about the same bytes per player.

mm_expire and mm_wait_stats are timed on the host around the call (what the owner waits for: launches, the
synchronisation, and for mm_expire the copy of the list and the host mirror's update); the kernels' own durations come
from a kernel trace of this script (rocprofv3 --kernel-trace --stats -- python tools/bench_wait.py --steps 20).

--move adds mm_move at 0 %, 1 % and 50 % selected (cfg-2's pool as mode 0, the same game with a window of +-100 and no
region filter as mode 1, its fallback; twice the capacity, since the old slots are held until the next tick) beside the
route an owner had before it, timed in the same process in turns: mm_expire, mm_expired, a numpy gather of rating and
constraint word from a host table, mm_enqueue of the same rows.  The enqueue and tick figures above are restated in the
same output (they must not have moved: k_bucket_scatter is untouched).

--carry adds, on the same two-mode engine and pool, the two-call route that carries players between engines, run on one
engine — mm_move_out, mm_expired, mm_moved_rows, mm_enqueue_stamped of the same rows — in turns with mm_move and with the
host route, at the same three shares.  What to expect at 1 %: between the two (it spares the host gather of the host route
and adds one 4-byte column each way to mm_move).  All three must leave the same queue depths.

--rotate adds mm_rotate on cfg-2's pool with a stored anchor in every rating group (an anchor of a region nobody else is
from, ticked into the stored lobby before the pool arrives) beside the host route it replaces — mm_lobby_state per rating
group, the owner's table, mm_cancel, mm_enqueue_stamped — in turns on the same engine; both must hand out the same slots and
leave the same queues.

--locate adds mm_locate on cfg-2's pool, all of it waiting in its queues with one player in a thousand cancelled, for 1,
1 000 and 100 000 queried slots drawn from the waiting players: the call, the same call with ahead == NULL (no counting pass)
and the host route it replaces — mm_queue_slots and mm_lobby_state per rating group, then the numpy search over them against
the owner's table of cancelled slots — in turns on the same engine; the call and the host route must give the same answer.

--partners adds mm_partners on the same waiting pool (all of it queued, one player in a thousand cancelled), at the mode's own
window and flags, for 1, 1 000 and 100 000 queried slots: the call with all three outputs, the call with `partners` only, and
the host route it replaces — mm_queue_slots and mm_lobby_state per rating group, then numpy over the owner's table of ratings
and constraint words: the LIVE candidates sorted by (region, rating) once per role and once together, two binary searches per
query and role for the counts, the sorted neighbours for the gap — in turns on the same engine; the call and the host route
must give the same three columns.  A one-slot mm_locate follows every host route, timed on its own (after_host_drain_ms):
in some processes the first GPU call after the route stalls for tens of milliseconds, and that
belongs to no call of the rotation.

--move-if adds mm_move_if and mm_expire_if (the selection by age kept where the partner count lies in a range) on cfg-2's pool
with a wider 1v1 mode as the fallback, all of the pool waiting and 1 000 entries cancelled, at 0 %, 1 % and 10 % old enough,
beside plain mm_move at the same share and the host route — the owner's stamp table, mm_partners on the old slots, a numpy
filter, mm_cancel, mm_enqueue_stamped — in turns on the same engine; the host route must hand out the same new slots.

--partner-stats adds mm_partner_stats on the same waiting pool (all of it queued, 1 000 entries cancelled), at the mode's own
window and flags, beside the two routes to the same records that exist without it, in turns on the same engine: mm_partners
over every waiting slot (partners and gap) plus the numpy bucketing per rating group, and the host route of --partners
extended to every waiting player plus the same bucketing.  All three must produce the same records, every step.  The
kernel-by-kernel split (key build, each radix pass, the search) comes from a kernel trace of --partner-stats-trace-run,
handed in with --partner-stats-trace.

--partners-sorted and --move-if-sorted add mm_partners and the rule calls by their two routes (include/mm_wait.h: tiles,
sorted) and by the default size rule, on three engines of one process in turns over the pools of --partners and --move-if, with
the product queries x bound >> 20 at which the forced routes cross — the measured value of mm_tuning.wait_sort_mtests; the
kernels' own durations come from a kernel trace of --partners-sorted-trace-run.  --legs-only skips the clock's own legs.

Usage (GPU box, repo root):  python tools/bench_wait.py [--steps 30] [--players 1000000] > profiles/wait_1m.json
                             python tools/bench_wait.py --move > profiles/wait_move_1m.json
                             python tools/bench_wait.py --carry > profiles/wait_carry_1m.json
                             python tools/bench_wait.py --rotate > profiles/wait_rotate_1m.json
                             python tools/bench_wait.py --locate > profiles/wait_locate_1m.json
                             python tools/bench_wait.py --partners > profiles/wait_partners_1m.json
                             python tools/bench_wait.py --move-if > profiles/wait_move_if_1m.json
                             python tools/bench_wait.py --partner-stats > profiles/wait_partner_stats_1m.json
                             python tools/bench_wait.py --legs-only --partners-sorted > profiles/wait_partners_sorted_1m.json
                             python tools/bench_wait.py --legs-only --move-if-sorted > profiles/wait_move_if_sorted_1m.json"""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def med(xs):
    return float(np.median(np.asarray(xs, dtype=np.float64)))


def spread(xs):
    a = np.asarray(xs, dtype=np.float64)
    return {"median": float(np.median(a)), "p10": float(np.percentile(a, 10)), "p90": float(np.percentile(a, 90)), "n": int(a.size)}


def measure_move(args, rating, cons, d_rating, d_cons, now):
    """mm_move and the host route, in turns on one engine: the same pool, the same split into an old and a young batch, the
    same players selected; both leave the same queues behind (checked once per share)."""
    from microservice_matchmaking_amd import Engine, make_config, mode_1v1
    n = args.players
    cap = 2 << (n - 1).bit_length()
    cfg = make_config([mode_1v1(window=25, region_filter=True), mode_1v1(window=100)], capacity=cap, timing=True)
    out = {}
    with Engine(cfg) as eng:
        eng.clock_set(now)
        for label, frac in (("0pct", 0.0), ("1pct", 0.01), ("50pct", 0.5)):
            old = int(n * frac)
            t_move, t_host, parts, depth = [], [], {"expire_ms": [], "gather_ms": [], "enqueue_ms": []}, {}
            for k in range(args.warmup + args.steps):
                for route in ("move", "host") if k % 2 == 0 else ("host", "move"):
                    eng.reset()
                    now += 10
                    eng.clock_set(now)
                    if old:
                        eng.enqueue_device(d_rating[:old], d_cons[:old])
                    now += 100
                    eng.clock_set(now)
                    eng.enqueue_device(d_rating[old:], d_cons[old:])        # slot i holds player i: the owner's table is (rating, cons)
                    t0 = time.perf_counter()
                    if route == "move":
                        got = eng.move(0, 1, 50)
                        t1 = time.perf_counter()
                        assert got[0].size == old and (got[3] != 0xFFFFFFFF).all()
                        if k >= args.warmup:
                            t_move.append((t1 - t0) * 1e3)
                    else:
                        slots, group, _ = eng.expire(0, 50)
                        ta = time.perf_counter()
                        r2 = rating[slots]
                        c2 = (cons[slots] & np.uint32(0x000FFFF0)) | np.uint32(1)
                        g2 = group.astype(np.uint8)
                        tb = time.perf_counter()
                        new = eng.enqueue(r2, c2, g2) if old else np.zeros(0, np.uint32)
                        t1 = time.perf_counter()
                        assert slots.size == old and new.size == old
                        if k >= args.warmup:
                            t_host.append((t1 - t0) * 1e3)
                            parts["expire_ms"].append((ta - t0) * 1e3)
                            parts["gather_ms"].append((tb - ta) * 1e3)
                            parts["enqueue_ms"].append((t1 - tb) * 1e3)
                    depth[route] = (eng.queue_depth(0).tolist(), eng.queue_depth(1).tolist())
            assert depth["move"] == depth["host"], depth
            out[label] = {"selected": old, "move_call_ms": spread(t_move), "host_route_ms": spread(t_host),
                          "host_route_parts_ms": {k: med(v) for k, v in parts.items()},
                          "move_over_host": med(t_move) / med(t_host)}
    out["note"] = ("host time around the calls; the host route's stamp is the time of the re-enqueue, mm_move's the original one. "
                   "capacity %d: a moved player's old slot is held until from_mode's next tick on either route" % cap)
    return out


def measure_carry(args, rating, cons, d_rating, d_cons, now):
    """mm_move, the two-call route (mm_move_out + mm_expired + mm_moved_rows + mm_enqueue_stamped) and the host route, in turns
    on one engine: the same pool, the same old and young batch, the same players selected, the same queue depths behind."""
    from microservice_matchmaking_amd import Engine, make_config, mode_1v1
    n = args.players
    cap = 2 << (n - 1).bit_length()
    cfg = make_config([mode_1v1(window=25, region_filter=True), mode_1v1(window=100)], capacity=cap, timing=True)
    out = {}
    routes = ("move", "carry", "host")
    with Engine(cfg) as eng:
        eng.clock_set(now)
        for label, frac in (("0pct", 0.0), ("1pct", 0.01), ("50pct", 0.5)):
            old = int(n * frac)
            t = {r: [] for r in routes}
            parts = {"move_out_ms": [], "enqueue_stamped_ms": []}
            depth = {}
            for k in range(args.warmup + args.steps):
                for route in routes[k % 3:] + routes[:k % 3]:
                    eng.reset()
                    now += 10
                    eng.clock_set(now)
                    if old:
                        eng.enqueue_device(d_rating[:old], d_cons[:old])
                    now += 100
                    eng.clock_set(now)
                    eng.enqueue_device(d_rating[old:], d_cons[old:])        # slot i holds player i: the owner's table is (rating, cons)
                    t0 = time.perf_counter()
                    if route == "move":
                        got = eng.move(0, 1, 50)
                        t1 = time.perf_counter()
                        assert got[0].size == old and (got[3] != 0xFFFFFFFF).all()
                    elif route == "carry":
                        slots, group, _, r2, c2, s2 = eng.move_out(0, 1, 50)
                        ta = time.perf_counter()
                        new = eng.enqueue_stamped(r2, c2, s2, group.astype(np.uint8)) if old else np.zeros(0, np.uint32)
                        t1 = time.perf_counter()
                        assert slots.size == old and new.size == old and (s2 == now - 100).all()
                        if k >= args.warmup:
                            parts["move_out_ms"].append((ta - t0) * 1e3)
                            parts["enqueue_stamped_ms"].append((t1 - ta) * 1e3)
                    else:
                        slots, group, _ = eng.expire(0, 50)
                        r2 = rating[slots]
                        c2 = (cons[slots] & np.uint32(0x000FFFF0)) | np.uint32(1)
                        new = eng.enqueue(r2, c2, group.astype(np.uint8)) if old else np.zeros(0, np.uint32)
                        t1 = time.perf_counter()
                        assert slots.size == old and new.size == old
                    if k >= args.warmup:
                        t[route].append((t1 - t0) * 1e3)
                    depth[route] = (eng.queue_depth(0).tolist(), eng.queue_depth(1).tolist())
            assert depth["move"] == depth["host"] == depth["carry"], depth
            m = {r: med(t[r]) for r in routes}
            out[label] = {"selected": old, "move_call_ms": spread(t["move"]), "carry_route_ms": spread(t["carry"]),
                          "host_route_ms": spread(t["host"]), "carry_route_parts_ms": {k: med(v) for k, v in parts.items()},
                          "carry_over_move": m["carry"] / m["move"], "carry_over_host": m["carry"] / m["host"],
                          "carry_between_move_and_host": bool(m["move"] <= m["carry"] <= m["host"])}
    out["note"] = ("host time around the calls, the wrapper's numpy buffers included; the carry route and mm_move keep the original "
                   "stamp, the host route's stamp is the time of the re-enqueue.  capacity %d" % cap)
    return out


def measure_rotate(args, d_rating, d_cons, now):
    """mm_rotate and the host route, in turns on one engine: the same pool behind the same stored anchors, the same seats
    selected, the same new slots and queues behind."""
    from microservice_matchmaking_amd import Engine, make_config, mode_1v1
    from microservice_matchmaking_amd._abi import cons_make
    n = args.players
    cap = 1 << (n - 1).bit_length()
    if cap - n < 64:
        cap *= 2
    cfg = make_config([mode_1v1(window=25, region_filter=True)], capacity=cap, timing=True)
    G = int(cfg.n_groups)
    a_rating = np.asarray([(cfg.groups[g].from_ + cfg.groups[g].to) // 2 for g in range(G)], np.int32)
    a_cons = cons_make(0, np.full(G, 200))                       # a region of their own: nobody in the pool fits them
    t = {"rotate": [], "host": []}
    parts = {"lobby_state_ms": [], "cancel_ms": [], "enqueue_stamped_ms": []}
    seen = {}
    with Engine(cfg) as eng:
        eng.clock_set(now)
        for k in range(args.warmup + args.steps):
            for route in ("rotate", "host") if k % 2 == 0 else ("host", "rotate"):
                eng.reset()
                now += 10
                eng.clock_set(now)
                stamp0 = now
                anchors = eng.enqueue(a_rating, a_cons)            # slots 0 .. G-1: the owner's table is (a_rating, a_cons, stamp0)
                assert len(eng.tick(0)) == 0
                now += 100
                eng.clock_set(now)
                eng.enqueue_device(d_rating, d_cons)
                t0 = time.perf_counter()
                if route == "rotate":
                    old, group, age, new = eng.rotate(0, 1, 1)
                    t1 = time.perf_counter()
                else:
                    seats = [eng.lobby_state(0, g)[0] for g in range(G)]
                    ta = time.perf_counter()
                    old = np.concatenate(seats).astype(np.uint32)
                    group = np.repeat(np.arange(G, dtype=np.uint32), [s.size for s in seats])
                    eng.cancel(old)
                    tb = time.perf_counter()
                    new = eng.enqueue_stamped(a_rating[old], a_cons[old], np.full(old.size, stamp0, np.uint32), group.astype(np.uint8))
                    t1 = time.perf_counter()
                    if k >= args.warmup:
                        parts["lobby_state_ms"].append((ta - t0) * 1e3)
                        parts["cancel_ms"].append((tb - ta) * 1e3)
                        parts["enqueue_stamped_ms"].append((t1 - tb) * 1e3)
                assert old.tolist() == anchors.tolist() and new.size == G
                if k >= args.warmup:
                    t[route].append((t1 - t0) * 1e3)
                seen[route] = (new.tolist(), eng.queue_depth(0).tolist(), [int(eng.queue_slots(0, g)[-1]) for g in range(G)],
                               [w["oldest_age"] for w in eng.wait_stats(0)])
    assert seen["rotate"] == seen["host"], seen
    return {"selected": G, "groups": G, "rotate_call_ms": spread(t["rotate"]), "host_route_ms": spread(t["host"]),
            "host_route_parts_ms": {k: med(v) for k, v in parts.items()},
            "rotate_over_host": med(t["rotate"]) / med(t["host"]),
            "note": "host time around the calls, the wrapper's numpy buffers included; %d players queued behind %d stored anchors, "
                    "capacity %d; both routes hand out the same slots and keep the anchors' stamps" % (n, G, cap)}


def host_locate(eng, mode, gone, q):
    """What mm_locate replaces: every rating group's queue and stored lobby copied to the host, then the search in numpy —
    position and LIVE entries ahead from the lists and the owner's table of cancelled slots (`gone`), gathered per query."""
    cap, G = int(eng.cfg.capacity), int(eng.cfg.n_groups)
    where = np.zeros(cap, np.uint32)
    group = np.full(cap, 0xFFFFFFFF, np.uint32)
    position = np.full(cap, 0xFFFFFFFF, np.uint32)
    ahead = np.zeros(cap, np.uint32)
    for g in range(G):
        qs = eng.queue_slots(mode, g)
        ls = eng.lobby_state(mode, g)[0]
        live = ~gone[qs]
        where[qs] = 1 + 4 * gone[qs]
        group[qs] = g
        position[qs] = np.arange(qs.size, dtype=np.uint32)
        ahead[qs] = np.cumsum(live, dtype=np.uint32) - live
        where[ls] = 2 + 4 * gone[ls]
        group[ls] = g
        position[ls] = np.arange(ls.size, dtype=np.uint32)
    return where[q], group[q], position[q], ahead[q]


def measure_locate(args, d_rating, d_cons, now):
    """mm_locate, mm_locate with ahead == NULL and the host route, in turns on one engine over the same waiting pool."""
    from microservice_matchmaking_amd import Engine, make_config, mode_1v1
    n = args.players
    cap = 1 << (n - 1).bit_length()
    cfg = make_config([mode_1v1(window=25, region_filter=True)], capacity=cap, timing=True)
    rng = np.random.default_rng(3)
    routes = ("locate", "no_ahead", "host")
    out = {}
    with Engine(cfg) as eng:
        eng.clock_set(now)
        eng.enqueue_device(d_rating, d_cons)                       # slot i holds player i; nobody ticks: all of them wait
        gone = np.zeros(cap, bool)
        gone[rng.choice(n, size=max(n // 1000, 1), replace=False)] = True
        eng.cancel(np.flatnonzero(gone).astype(np.uint32))
        eng.clock_set(now + 100)
        waiting = np.flatnonzero(~gone[:n]).astype(np.uint32)
        for nq in (1, 1000, 100000):
            q = rng.choice(waiting, size=min(nq, waiting.size), replace=False).astype(np.uint32)
            t = {r: [] for r in routes}
            got = {}
            for k in range(args.warmup + args.steps):
                for route in routes[k % 3:] + routes[:k % 3]:
                    t0 = time.perf_counter()
                    if route == "locate":
                        got[route] = eng.locate(0, q)
                    elif route == "no_ahead":
                        got[route] = eng.locate(0, q, ahead=False)
                    else:
                        got[route] = host_locate(eng, 0, gone, q)
                    t1 = time.perf_counter()
                    if k >= args.warmup:
                        t[route].append((t1 - t0) * 1e3)
            for c in range(4):
                assert np.array_equal(got["locate"][c], got["host"][c]), ("locate and the host route differ", nq, c)
                assert c == 3 or np.array_equal(got["locate"][c], got["no_ahead"][c]), ("ahead == NULL changes a column", nq, c)
            assert (got["locate"][0] == 1).all() and (got["locate"][4] == 100).all()
            m = {r: med(t[r]) for r in routes}
            out["%d_queries" % q.size] = {"queries": int(q.size), "locate_call_ms": spread(t["locate"]),
                                          "locate_no_ahead_call_ms": spread(t["no_ahead"]), "host_route_ms": spread(t["host"]),
                                          "locate_over_host": m["locate"] / m["host"], "no_ahead_over_locate": m["no_ahead"] / m["locate"]}
    out["note"] = ("host time around the calls, the wrapper's numpy buffers included; %d players waiting in %d queues, %d of them "
                   "cancelled and not yet purged, capacity %d; the host route copies every queue of the mode (4 bytes a player) and "
                   "builds position and ahead for the whole pool whatever the number of queries" % (n, int(cfg.n_groups), int(gone.sum()), cap))
    return out


def host_partners(eng, mode, gone, rating, cons, q, window):
    """What mm_partners replaces, for a region-filtered mode asked about itself: every rating group's queue and stored lobby
    copied to the host, the LIVE players keyed by (region, rating) from the owner's table and sorted — once per role for the
    counts, once together for the gap — then two binary searches per query and list.  A query that waits is in its own
    lists: one is taken off its role's count, and its gap looks past itself."""
    cap, G = int(eng.cfg.capacity), int(eng.cfg.n_groups)
    group = np.full(cap, -1, np.int64)
    lists = []
    for g in range(G):
        both = np.concatenate([eng.lobby_state(mode, g)[0], eng.queue_slots(mode, g)]).astype(np.int64)
        group[both] = g
        lists.append(both[~gone[both]])
    key_of = (((cons.astype(np.int64) >> 4) & 0xFF) << 33) + (rating.astype(np.int64) + (1 << 31))   # region | rating, one order
    role_of = (cons >> 16) & 0xF
    partners = np.zeros(q.size, np.uint32)
    by_role = np.zeros((q.size, 8), np.uint32)
    gap = np.full(q.size, 0xFFFFFFFF, np.uint32)
    qg = group[q]
    for g in range(G):
        i = np.flatnonzero(qg == g)
        w = lists[g]
        if i.size == 0 or w.size == 0:
            continue
        p = q[i].astype(np.int64)
        k, base = key_of[p], key_of[p] >> 33 << 33
        lo, hi = np.maximum(k - window, base), np.minimum(k + window, base + (1 << 32) - 1)
        alive = ~gone[p]
        for r in np.unique(role_of[w]):
            ks = np.sort(key_of[w[role_of[w] == r]])
            c = np.searchsorted(ks, hi, "right") - np.searchsorted(ks, lo, "left")
            by_role[i, r] = c - (alive & (role_of[p] == r))
        ks = np.sort(key_of[w])
        left, right = np.searchsorted(ks, k, "left"), np.searchsorted(ks, k, "right")
        twin = right - left - alive >= 1                       # somebody else of the same region and rating
        below = np.where(left > 0, ks[np.maximum(left - 1, 0)], -1)
        above = np.where(right < ks.size, ks[np.minimum(right, ks.size - 1)], -1)
        d = np.full(i.size, 1 << 40, np.int64)
        d = np.where((below >= base), np.minimum(d, k - below), d)
        d = np.where((above >= 0) & (above < base + (1 << 32)), np.minimum(d, above - k), d)
        d = np.where(twin, 0, d)
        gap[i] = np.where(d < (1 << 40), np.minimum(d, 0xFFFFFFFE), 0xFFFFFFFF)
    partners[:] = by_role.sum(1)
    return partners, by_role, gap


def measure_partners(args, rating, cons, d_rating, d_cons, now):
    """mm_partners with all three outputs, with `partners` only, and the host route, in turns on one engine over the same
    waiting pool, at the mode's own window and flags."""
    from microservice_matchmaking_amd import Engine, make_config, mode_1v1
    n = args.players
    cap = 1 << (n - 1).bit_length()
    cfg = make_config([mode_1v1(window=25, region_filter=True)], capacity=cap, timing=True)
    rng = np.random.default_rng(3)
    routes = ("all", "count", "host")
    table_r, table_c = np.zeros(cap, np.int32), np.zeros(cap, np.uint32)
    table_r[:n], table_c[:n] = rating, cons                        # slot i holds player i: the owner's table
    out = {}
    with Engine(cfg) as eng:
        eng.clock_set(now)
        eng.enqueue_device(d_rating, d_cons)                       # nobody ticks: all of them wait
        gone = np.zeros(cap, bool)
        gone[rng.choice(n, size=max(n // 1000, 1), replace=False)] = True
        eng.cancel(np.flatnonzero(gone).astype(np.uint32))
        waiting = np.flatnonzero(~gone[:n]).astype(np.uint32)
        for nq in (1, 1000, 100000):
            q = rng.choice(waiting, size=min(nq, waiting.size), replace=False).astype(np.uint32)
            t = {r: [] for r in routes}
            t["drain"] = []
            got = {}
            for k in range(args.warmup + args.steps):
                for route in routes[k % 3:] + routes[:k % 3]:
                    t0 = time.perf_counter()
                    if route == "all":
                        got[route] = eng.partners(0, q)
                    elif route == "count":
                        got[route] = eng.partners(0, q, by_role=False, gap=False)
                    else:
                        got[route] = host_partners(eng, 0, gone, table_r, table_c, q, 25)
                    t1 = time.perf_counter()
                    if route == "host":
                        # In some processes the first GPU call after the host route stalls, by 9 to 29 ms where the same
                        # call takes 0.1 ms alone (profiles/wait_partners_1m_no_drain.json: the one-query leg without this
                        # call).  The cause is not known.  A one-slot mm_locate comes first here, timed
                        # on its own and reported as after_host_drain_ms, so no call of the rotation inherits it.
                        eng.locate(0, q[:1])
                        t2 = time.perf_counter()
                        if k >= args.warmup:
                            t["drain"].append((t2 - t1) * 1e3)
                    if k >= args.warmup:
                        t[route].append((t1 - t0) * 1e3)
            for c in range(3):
                assert np.array_equal(got["all"][c], got["host"][c]), ("mm_partners and the host route differ", nq, c)
            assert np.array_equal(got["all"][0], got["count"][0]), ("NULL outputs change the count", nq)
            m = {r: med(t[r]) for r in routes}
            out["%d_queries" % q.size] = {"queries": int(q.size), "partners_mean": float(got["all"][0].mean()),
                                          "partners_call_ms": spread(t["all"]), "partners_count_only_call_ms": spread(t["count"]),
                                          "host_route_ms": spread(t["host"]), "after_host_drain_ms": spread(t["drain"]),
                                          "partners_over_host": m["all"] / m["host"],
                                          "count_only_over_all": m["count"] / m["all"]}
    out["note"] = ("host time around the calls, the wrapper's numpy buffers included; %d players waiting in %d queues, %d of them "
                   "cancelled and not yet purged, capacity %d, window 25 and the region filter; the host route copies every queue "
                   "of the mode (4 bytes a player) and sorts the pool per rating group whatever the number of queries, the call "
                   "tests every query against every entry of its rating group" % (n, int(cfg.n_groups), int(gone.sum()), cap))
    return out


def measure_move_if(args, rating, cons, d_rating, d_cons, now):
    """mm_move_if, mm_expire_if, plain mm_move and the host route, in turns on one engine: cfg-2's pool as mode 0 with a second,
    wider 1v1 mode, all of the pool waiting, 1 000 entries cancelled, the oldest 0 %, 1 % and 10 % old enough.  Two rules at the
    mode's own window and filter, in_mode = from_mode: [0, 0] ("nobody here fits me") and [0, M], M the median partner count of
    the pool, which keeps about half of the candidates.  The host route: the owner's stamp table says who is old, mm_partners
    counts on those slots, numpy filters, mm_cancel and mm_enqueue_stamped re-queue with rows from the owner's tables; it must
    hand out mm_move_if's new-slot column."""
    from microservice_matchmaking_amd import Engine, make_config, mode_1v1
    from microservice_matchmaking_amd.sharding import rating_groups
    n = args.players
    cap = 2 << (n - 1).bit_length()
    cfg = make_config([mode_1v1(window=25, region_filter=True), mode_1v1(window=100)], capacity=cap, timing=True)
    rng = np.random.default_rng(3)
    gone_slots = np.sort(rng.choice(n, size=min(1000, n), replace=False)).astype(np.uint32)
    gone = np.zeros(n, bool)
    gone[gone_slots] = True
    group_of = rating_groups(cfg, rating).astype(np.uint8)     # the owner's tables: slot i holds player i
    cons_to = (cons & np.uint32(0x000FFFF0)) | np.uint32(1)
    routes = ("move_if", "expire_if", "move", "host")
    out = {}
    with Engine(cfg) as eng:
        eng.clock_set(now)
        eng.enqueue_device(d_rating, d_cons)
        eng.cancel(gone_slots)
        median = int(np.median(eng.partners(0, np.arange(0, n, max(n // 4096, 1), dtype=np.uint32), by_role=False, gap=False)[0]))
        for label, frac in (("0pct", 0.0), ("1pct", 0.01), ("10pct", 0.1)):
            old = int(n * frac)
            out[label] = {"old_enough": int(old - gone[:old].sum())}
            for rname, hi in (("nobody_fits", 0), ("at_most_median", median)):
                rule = {"in_mode": 0, "min_partners": 0, "max_partners": hi}
                t = {r: [] for r in routes}
                parts = {"table_ms": [], "partners_ms": [], "filter_ms": [], "cancel_ms": [], "enqueue_stamped_ms": []}
                seen = {}
                for k in range(args.warmup + args.steps):
                    for route in routes[k % 4:] + routes[:k % 4]:
                        eng.reset()
                        now += 10
                        eng.clock_set(now)
                        if old:
                            eng.enqueue_device(d_rating[:old], d_cons[:old])
                        now += 100
                        eng.clock_set(now)
                        eng.enqueue_device(d_rating[old:], d_cons[old:])
                        eng.cancel(gone_slots)
                        stamp = np.full(n, now, np.uint32)         # the owner's stamp table
                        stamp[:old] = now - 100
                        t0 = time.perf_counter()
                        if route == "move_if":
                            got = eng.move_if(0, 1, 50, 0, rule)
                            t1 = time.perf_counter()
                            seen[route] = (got[0], got[3])
                        elif route == "expire_if":
                            got = eng.expire_if(0, 50, rule)
                            t1 = time.perf_counter()
                            seen[route] = (got[0],)
                        elif route == "move":
                            got = eng.move(0, 1, 50)
                            t1 = time.perf_counter()
                            assert got[0].size == out[label]["old_enough"]
                        else:
                            is_old = np.flatnonzero(((np.uint32(now) - stamp) > 50) & ~gone).astype(np.uint32)
                            is_old = is_old[np.argsort(group_of[is_old], kind="stable")]      # mm_expire's order: group, then arrival
                            ta = time.perf_counter()
                            cnt = eng.partners(0, is_old, by_role=False, gap=False)[0] if is_old.size else np.zeros(0, np.uint32)
                            tb = time.perf_counter()
                            sel = is_old[cnt <= hi]
                            tc = time.perf_counter()
                            if sel.size:
                                eng.cancel(sel)
                            td = time.perf_counter()
                            new = eng.enqueue_stamped(rating[sel], cons_to[sel], stamp[sel], group_of[sel]) if sel.size else np.zeros(0, np.uint32)
                            t1 = time.perf_counter()
                            seen[route] = (sel, new)
                            if k >= args.warmup:
                                for name, v in zip(parts, (ta - t0, tb - ta, tc - tb, td - tc, t1 - td)):
                                    parts[name].append(v * 1e3)
                        if k >= args.warmup:
                            t[route].append((t1 - t0) * 1e3)
                assert np.array_equal(seen["move_if"][0], seen["host"][0]), ("mm_move_if and the host route select differently", label, rname)
                assert np.array_equal(seen["move_if"][1], seen["host"][1]), ("the host route hands out other slots", label, rname)
                assert np.array_equal(seen["move_if"][0], seen["expire_if"][0]), ("mm_expire_if selects differently", label, rname)
                m = {r: med(t[r]) for r in routes}
                print("move_if %s %s: %s" % (label, rname, {r: round(v, 3) for r, v in m.items()}), file=sys.stderr, flush=True)
                out[label][rname] = {"max_partners": hi, "selected": int(seen["move_if"][0].size),
                                     "move_if_call_ms": spread(t["move_if"]), "expire_if_call_ms": spread(t["expire_if"]),
                                     "move_call_ms": spread(t["move"]), "host_route_ms": spread(t["host"]),
                                     "host_route_parts_ms": {k: med(v) for k, v in parts.items()},
                                     "move_if_over_host": m["move_if"] / m["host"], "move_if_over_move": m["move_if"] / m["move"],
                                     "expire_if_over_host": m["expire_if"] / m["host"]}
    out["note"] = ("host time around the calls, the wrapper's numpy buffers included; %d players waiting in mode 0, %d of them "
                   "cancelled, capacity %d, window 25 and the region filter, median partner count %d; plain mm_move moves everybody "
                   "old enough, the rule calls and the host route the selected only" % (n, int(gone.sum()), cap, median))
    return out


ROUTES = (("tiles", {"wait_sort_mtests": 0xFFFFFFFF}), ("sorted", {"wait_sort_mtests": 0}), ("default", None))
ROUTE_NAMES = {0: "none", 1: "tiles", 2: "sorted"}


def crossing(points, bound):
    """Where the medians of the two forced routes cross, as queries x bound >> 20: linear interpolation between the two
    measured points that bracket it.  points: [(queries, tiles_ms, sorted_ms)], queries ascending.  None: they do not cross."""
    for (q0, t0, s0), (q1, t1, s1) in zip(points, points[1:]):
        d0, d1 = t0 - s0, t1 - s1
        if d0 < 0 <= d1:
            q = q0 + (q1 - q0) * (-d0) / (d1 - d0)
            return {"between_queries": [q0, q1], "queries": q, "mtests": int(q * bound) >> 20}
    return None


def measure_partners_sorted(args, rating, cons, d_rating, d_cons, now):
    """mm_partners by its two routes and by the default rule, in turns on three engines over the same waiting pool (--partners'
    pool: all of it queued, one player in a thousand cancelled), at the mode's own window and flags: `partners` only and all
    three outputs, for 100 .. 100 000 queried slots and for every waiting slot.  The columns must be equal every step."""
    from microservice_matchmaking_amd import Engine, make_config, mode_1v1
    n = args.players
    cap = 1 << (n - 1).bit_length()
    cfg = make_config([mode_1v1(window=25, region_filter=True)], capacity=cap, timing=True)
    rng = np.random.default_rng(3)
    gone = np.zeros(cap, bool)
    gone[rng.choice(n, size=max(n // 1000, 1), replace=False)] = True
    waiting = np.flatnonzero(~gone[:n]).astype(np.uint32)
    engines = {}
    for name, tuning in ROUTES:
        eng = engines[name] = Engine(cfg, tuning)
        eng.clock_set(now)
        eng.enqueue_device(d_rating, d_cons)                       # nobody ticks: all of them wait
        eng.cancel(np.flatnonzero(gone).astype(np.uint32))
    names = tuple(engines)
    out = {"threshold_default": engines["default"].tuning()["wait_sort_mtests"]}
    curve = {"count": [], "all": []}
    for nq in sorted({min(x, waiting.size) for x in (100, 1000, 10000, 100000, waiting.size)}):
        q = waiting if nq == waiting.size else rng.choice(waiting, size=nq, replace=False).astype(np.uint32)
        point = {"queries": int(q.size)}
        for question, kw in (("count", {"by_role": False, "gap": False}), ("all", {})):
            t = {r: [] for r in names}
            got, route = {}, {}
            for k in range(args.warmup + args.steps):
                for r in names[k % 3:] + names[:k % 3]:
                    t0 = time.perf_counter()
                    got[r] = engines[r].partners(0, q, **kw)
                    t1 = time.perf_counter()
                    if k >= args.warmup:
                        t[r].append((t1 - t0) * 1e3)
                for r in names[1:]:
                    for c in range(3):
                        assert (got[r][c] is None and got["tiles"][c] is None) or np.array_equal(got[r][c], got["tiles"][c]), \
                            ("the routes differ", nq, question, r, c)
            for r in names:
                route[r] = engines[r].wait_route()
            assert route["tiles"]["route"] == 1 and route["sorted"]["route"] == 2
            best = min(med(t["tiles"]), med(t["sorted"]))
            point[question] = {"tiles_ms": spread(t["tiles"]), "sorted_ms": spread(t["sorted"]), "default_ms": spread(t["default"]),
                               "default_route": ROUTE_NAMES[route["default"]["route"]], "keys": route["sorted"]["keys"],
                               "passes": route["sorted"]["passes"], "bound": route["sorted"]["bound"],
                               "sorted_over_tiles": med(t["sorted"]) / med(t["tiles"]), "default_over_better": med(t["default"]) / best}
            curve[question].append((int(q.size), med(t["tiles"]), med(t["sorted"])))
            print("partners_sorted %d %s: %s" % (q.size, question, {r: round(med(t[r]), 3) for r in names}), file=sys.stderr, flush=True)
        out["%d_queries" % q.size] = point
    bound = min(n, cap)
    out["crossing"] = {question: crossing(pts, bound) for question, pts in curve.items()}
    out["note"] = ("host time around the calls, the wrapper's numpy buffers included; %d players waiting in %d queues, %d of them "
                   "cancelled and not yet purged, capacity %d, window 25 and the region filter; three engines with the same pool, "
                   "wait_sort_mtests 0xFFFFFFFF (tiles), 0 (sorted) and the built-in default, called in turns; crossing: the "
                   "product queries x bound >> 20 at which the forced routes' medians cross" % (n, int(cfg.n_groups), int(gone.sum()), cap))
    for eng in engines.values():
        eng.close()
    return out


def measure_move_if_sorted(args, rating, cons, d_rating, d_cons, now):
    """mm_move_if and mm_expire_if by the two routes and by the default rule, in turns on three engines: --move-if's pool (cfg-2
    as mode 0 with a wider 1v1 as the fallback, all of it waiting, 1 000 entries cancelled), the oldest 0 %, 1 %, 10 % and
    100 % old enough, the rule "nobody here fits me" at the mode's own window and filter.  The lists must be equal every step."""
    from microservice_matchmaking_amd import Engine, make_config, mode_1v1
    n = args.players
    cap = 2 << (n - 1).bit_length()
    cfg = make_config([mode_1v1(window=25, region_filter=True), mode_1v1(window=100)], capacity=cap, timing=True)
    rng = np.random.default_rng(3)
    gone_slots = np.sort(rng.choice(n, size=min(1000, n), replace=False)).astype(np.uint32)
    gone = np.zeros(n, bool)
    gone[gone_slots] = True
    engines = {name: Engine(cfg, tuning) for name, tuning in ROUTES}
    names = tuple(engines)
    rule = {"in_mode": 0, "min_partners": 0, "max_partners": 0}
    out = {"threshold_default": engines["default"].tuning()["wait_sort_mtests"]}
    for label, frac in (("0pct", 0.0), ("1pct", 0.01), ("10pct", 0.1), ("100pct", 1.0)):
        old = int(n * frac)
        point = {"old_enough": int(old - gone[:old].sum())}
        for call in ("move_if", "expire_if"):
            t = {r: [] for r in names}
            seen, route = {}, {}
            for k in range(args.warmup + args.steps):
                for r in names[k % 3:] + names[:k % 3]:
                    eng = engines[r]
                    eng.reset()
                    now += 10
                    eng.clock_set(now)
                    if old:
                        eng.enqueue_device(d_rating[:old], d_cons[:old])
                    now += 100
                    eng.clock_set(now)
                    if old < n:
                        eng.enqueue_device(d_rating[old:], d_cons[old:])
                    eng.cancel(gone_slots)
                    t0 = time.perf_counter()
                    got = eng.move_if(0, 1, 50, 0, rule) if call == "move_if" else eng.expire_if(0, 50, rule)
                    t1 = time.perf_counter()
                    seen[r] = got
                    route[r] = eng.wait_route()
                    if k >= args.warmup:
                        t[r].append((t1 - t0) * 1e3)
                for r in names[1:]:
                    for c in range(len(seen["tiles"])):
                        assert np.array_equal(seen[r][c], seen["tiles"][c]), ("the routes differ", label, call, r, c)
            best = min(med(t["tiles"]), med(t["sorted"]))
            point[call] = {"selected": int(seen["tiles"][0].size), "tiles_ms": spread(t["tiles"]), "sorted_ms": spread(t["sorted"]),
                           "default_ms": spread(t["default"]), "default_route": ROUTE_NAMES[route["default"]["route"]],
                           "sorted_route": ROUTE_NAMES[route["sorted"]["route"]], "keys": route["sorted"]["keys"],
                           "sorted_over_tiles": med(t["sorted"]) / med(t["tiles"]), "default_over_better": med(t["default"]) / best}
            print("move_if_sorted %s %s: %s" % (label, call, {r: round(med(t[r]), 3) for r in names}), file=sys.stderr, flush=True)
        out[label] = point
    out["note"] = ("host time around the calls, the wrapper's numpy buffers included; %d players waiting in mode 0, %d of them "
                   "cancelled, capacity %d, window 25 and the region filter, the rule [0, 0] in from_mode; three engines, "
                   "wait_sort_mtests 0xFFFFFFFF (tiles), 0 (sorted) and the built-in default, in turns; nobody old enough: no "
                   "count runs on either route" % (n, int(gone.sum()), cap))
    for eng in engines.values():
        eng.close()
    return out


def partners_sorted_trace_run(args):
    """Only mm_partners on the sorted route, --steps times at 100 000 queries with all three outputs and with the count alone,
    on --partners-sorted's pool: the run to trace."""
    import torch
    from microservice_matchmaking_amd import Engine, make_config, mode_1v1
    from microservice_matchmaking_amd.synth import make_pool
    n = args.players
    cap = 1 << (n - 1).bit_length()
    cfg = make_config([mode_1v1(window=25, region_filter=True)], capacity=cap, timing=True)
    rating, cons = make_pool(n, seed=1)
    rng = np.random.default_rng(3)
    with Engine(cfg, {"wait_sort_mtests": 0}) as eng:
        eng.clock_set(1)
        eng.enqueue_device(torch.from_numpy(rating).cuda(), torch.from_numpy(cons.view(np.int32)).cuda())
        q = rng.choice(n, size=min(100000, n), replace=False).astype(np.uint32)
        for _ in range(args.steps):
            eng.partners(0, q)
            got = eng.partners(0, q, by_role=False, gap=False)
    print(json.dumps({"calls": 2 * args.steps, "queries": int(q.size), "partners_mean": float(got[0].mean())}))


def bucket_records(partners, gap, group, candidates):
    """mm_partner_group (include/mm_wait.h) per rating group, in numpy, from mm_partners' two columns over the waiting players
    and each player's rating group."""
    pow2 = 1 << np.arange(33, dtype=np.uint64)
    bits = lambda v: np.bincount(np.searchsorted(pow2, v, side="right").astype(np.int64), minlength=33)[:33].tolist()
    out = []
    for g, cand in enumerate(candidates):
        p, d = partners[group == g].astype(np.uint64), gap[group == g].astype(np.uint64)
        has = d != 0xFFFFFFFF
        out.append({"waiting": int(p.size), "candidates": int(cand), "alone": int((p == 0).sum()), "unreachable": int((~has).sum()),
                    "partners_sum": int(p.sum()), "gap_sum": int(d[has].sum()), "partners_max": int(p.max()) if p.size else 0,
                    "gap_max": int(d[has].max()) if has.any() else 0, "partners_hist": bits(p), "gap_hist": bits(d[has])})
    return out


def plain_records(recs):
    return [{k: (v.tolist() if hasattr(v, "tolist") else v) for k, v in r.items()} for r in recs]


FIT_SEQUENCE = ("k_fit_count", "k_wait_scan", "k_fit_keys")


def trace_split(path):
    """The kernels of mm_partner_stats out of a kernel trace (rocprofv3 --kernel-trace, its *_kernel_trace.csv) of
    `--partner-stats-trace-run`: a call is k_fit_count, k_wait_scan, k_fit_keys, then k_fit_hist / k_fit_scan / k_fit_scatter
    once per radix pass, then k_fit_search.  Medians over the calls, in microseconds."""
    import csv
    rows = []
    with open(path, newline="") as f:
        for r in csv.DictReader(f):
            name = r.get("Kernel_Name", "")
            short = next((k for k in FIT_SEQUENCE + ("k_fit_hist", "k_fit_scan", "k_fit_scatter", "k_fit_search") if name.startswith(k)), None)
            if short:
                rows.append((int(r["Start_Timestamp"]), int(r["End_Timestamp"]), short))
    rows.sort()
    calls, cur = [], None
    for t0, t1, k in rows:
        if k == "k_fit_count":
            cur = {"key_build": 0.0, "passes": [], "search": 0.0, "first": t0}
            calls.append(cur)
        if cur is None:
            continue
        us = (t1 - t0) / 1e3
        if k in FIT_SEQUENCE:
            cur["key_build"] += us
        elif k == "k_fit_hist":
            cur["passes"].append({"hist": us, "scan": 0.0, "scatter": 0.0})
        elif k in ("k_fit_scan", "k_fit_scatter") and cur["passes"]:
            cur["passes"][-1][k[6:]] += us
        elif k == "k_fit_search":
            cur["search"] = us
            cur["span"] = (t1 - cur["first"]) / 1e3
    calls = [c for c in calls if "span" in c]
    if not calls:
        return None
    n_pass = max(len(c["passes"]) for c in calls)
    calls = [c for c in calls if len(c["passes"]) == n_pass]
    return {"calls": len(calls), "unit": "us, medians over the calls of the trace",
            "key_build_count_scan_keys": med([c["key_build"] for c in calls]),
            "radix_passes": [{k: med([c["passes"][p][k] for c in calls]) for k in ("hist", "scan", "scatter")} for p in range(n_pass)],
            "search": med([c["search"] for c in calls]),
            "first_start_to_last_end": med([c["span"] for c in calls])}


def partner_stats_pool(args, d_rating, d_cons, now):
    """cfg-2's pool as --partners sets it up: all of it waiting, 1 000 entries cancelled."""
    from microservice_matchmaking_amd import Engine, make_config, mode_1v1
    n = args.players
    cap = 1 << (n - 1).bit_length()
    cfg = make_config([mode_1v1(window=25, region_filter=True)], capacity=cap, timing=True)
    eng = Engine(cfg)
    eng.clock_set(now)
    eng.enqueue_device(d_rating, d_cons)                           # nobody ticks: all of them wait
    gone = np.zeros(cap, bool)
    gone[np.random.default_rng(3).choice(n, size=min(1000, n), replace=False)] = True
    eng.cancel(np.flatnonzero(gone).astype(np.uint32))
    return eng, cfg, gone


def measure_partner_stats(args, rating, cons, d_rating, d_cons, now):
    """mm_partner_stats, mm_partners over every waiting slot plus the numpy bucketing, and the host's sorted tables plus the
    same bucketing, in turns on one engine over the same waiting pool, at the mode's own window and flags: the same records."""
    from microservice_matchmaking_amd.sharding import rating_groups
    n = args.players
    eng, cfg, gone = partner_stats_pool(args, d_rating, d_cons, now)
    cap, G = int(cfg.capacity), int(cfg.n_groups)
    table_r, table_c = np.zeros(cap, np.int32), np.zeros(cap, np.uint32)
    table_r[:n], table_c[:n] = rating, cons                        # slot i holds player i: the owner's tables
    waiting = np.flatnonzero(~gone[:n]).astype(np.uint32)
    group = rating_groups(cfg, rating)[waiting]
    candidates = np.bincount(group, minlength=G)
    routes = ("stats", "device", "host")
    t = {r: [] for r in routes}
    t["drain"], t["device_call"], t["host_tables"] = [], [], []
    got = {}
    with eng:
        for k in range(args.warmup + args.steps):
            for route in routes[k % 3:] + routes[:k % 3]:
                t0 = time.perf_counter()
                if route == "stats":
                    got[route] = plain_records(eng.partner_stats(0))
                elif route == "device":
                    p, _, d = eng.partners(0, waiting, by_role=False)
                    ta = time.perf_counter()
                    got[route] = bucket_records(p, d, group, candidates)
                else:
                    p, _, d = host_partners(eng, 0, gone, table_r, table_c, waiting, 25)
                    ta = time.perf_counter()
                    got[route] = bucket_records(p, d, group, candidates)
                t1 = time.perf_counter()
                if route == "host":                                # (as --partners: the first GPU call after the host route, on its own)
                    eng.locate(0, waiting[:1])
                    t2 = time.perf_counter()
                    if k >= args.warmup:
                        t["drain"].append((t2 - t1) * 1e3)
                if k >= args.warmup:
                    t[route].append((t1 - t0) * 1e3)
                    if route != "stats":
                        t["device_call" if route == "device" else "host_tables"].append((ta - t0) * 1e3)
            assert got["stats"] == got["device"], "mm_partner_stats and mm_partners over every slot differ"
            assert got["stats"] == got["host"], "mm_partner_stats and the host route differ"
    m = {r: med(t[r]) for r in routes}
    print("partner_stats: %s" % {r: round(v, 3) for r, v in m.items()}, file=sys.stderr, flush=True)
    out = {"waiting": int(waiting.size), "groups": G, "window": 25, "flags": "region filter",
           "partner_stats_call_ms": spread(t["stats"]), "partners_every_slot_route_ms": spread(t["device"]),
           "partners_every_slot_call_ms": spread(t["device_call"]), "host_route_ms": spread(t["host"]),
           "host_route_tables_ms": spread(t["host_tables"]), "after_host_drain_ms": spread(t["drain"]),
           "partner_stats_over_partners_route": m["stats"] / m["device"], "partner_stats_over_host_route": m["stats"] / m["host"],
           "partner_stats_beats_both": bool(m["stats"] < m["device"] and m["stats"] < m["host"]),
           "records": got["stats"],
           "note": "host time around the calls, the wrapper's numpy buffers included; %d players waiting in %d queues, %d cancelled "
                   "and not yet purged, capacity %d; all three routes produce the same records (checked every step); both other "
                   "routes include the numpy bucketing of a million (partners, gap) pairs" % (int(waiting.size), G, int(gone.sum()), cap)}
    if args.partner_stats_trace:
        out["kernels"] = trace_split(args.partner_stats_trace)
    return out


def partner_stats_trace_run(args):
    """Nothing but --steps calls of mm_partner_stats on the pool of --partner-stats: what a kernel trace is taken of."""
    import torch
    from microservice_matchmaking_amd.synth import make_pool
    rating, cons = make_pool(args.players, seed=1)
    eng, _, _ = partner_stats_pool(args, torch.from_numpy(rating).cuda(), torch.from_numpy(cons.view(np.int32)).cuda(), 1)
    with eng:
        for _ in range(args.steps):
            recs = eng.partner_stats(0)
    print(json.dumps({"calls": args.steps, "waiting": sum(r["waiting"] for r in recs)}))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--players", type=int, default=1_000_000)
    ap.add_argument("--clock-first", action="store_true",
                    help="create the engine with the clock before the one without (two engines are two sets of allocations: "
                         "does a difference between their ticks follow the clock or the engine's place in memory?)")
    ap.add_argument("--move", action="store_true", help="also measure mm_move beside the host route it replaces")
    ap.add_argument("--carry", action="store_true",
                    help="also measure mm_move_out + mm_enqueue_stamped on one engine beside mm_move and the host route")
    ap.add_argument("--rotate", action="store_true",
                    help="also measure mm_rotate beside the host route it replaces (mm_lobby_state per group, mm_cancel, mm_enqueue_stamped)")
    ap.add_argument("--locate", action="store_true",
                    help="also measure mm_locate, with and without the ahead column, beside the host route it replaces "
                         "(mm_queue_slots and mm_lobby_state per group, the numpy search)")
    ap.add_argument("--partners", action="store_true",
                    help="also measure mm_partners, with all three outputs and with the count alone, beside the host route it "
                         "replaces (mm_queue_slots and mm_lobby_state per group, sorted numpy tables)")
    ap.add_argument("--move-if", action="store_true",
                    help="also measure mm_move_if and mm_expire_if beside plain mm_move and the host route they replace (the owner's "
                         "stamp table, mm_partners, a numpy filter, mm_cancel, mm_enqueue_stamped)")
    ap.add_argument("--partner-stats", action="store_true",
                    help="also measure mm_partner_stats beside mm_partners over every waiting slot and the host's sorted tables, "
                         "each with the numpy bucketing it needs")
    ap.add_argument("--partner-stats-trace", metavar="CSV", default=None,
                    help="with --partner-stats: the kernel trace (rocprofv3 --kernel-trace, *_kernel_trace.csv) of a "
                         "--partner-stats-trace-run, for the kernel-by-kernel split of the call")
    ap.add_argument("--partner-stats-trace-run", action="store_true",
                    help="only call mm_partner_stats --steps times on the pool of --partner-stats and exit: the run to trace")
    ap.add_argument("--partners-sorted", action="store_true",
                    help="also measure mm_partners by the tiles route, the sorted route and the default rule (wait_sort_mtests), "
                         "100 queries to every waiting slot, and where the two routes cross")
    ap.add_argument("--move-if-sorted", action="store_true",
                    help="also measure mm_move_if and mm_expire_if by the two routes and the default rule at 0 %, 1 %, 10 % and 100 % old enough")
    ap.add_argument("--partners-sorted-trace-run", action="store_true",
                    help="only call mm_partners on the sorted route --steps times on the pool of --partners-sorted and exit: the run to trace")
    ap.add_argument("--legs-only", action="store_true",
                    help="skip the clock's own enqueue / tick / expire legs: only the legs asked for are measured and printed")
    args = ap.parse_args()
    assert args.steps >= 20, "medians of at least 20 steps"
    import torch
    assert torch.cuda.is_available(), "needs a GPU; there is no CPU path"
    if args.partner_stats_trace_run:
        return partner_stats_trace_run(args)
    if args.partners_sorted_trace_run:
        return partners_sorted_trace_run(args)
    from bench import kernel_source_hash
    from microservice_matchmaking_amd import Engine, make_config, mode_1v1
    from microservice_matchmaking_amd.synth import make_pool

    n = args.players
    cap = 1 << (n - 1).bit_length()
    cfg = make_config([mode_1v1(window=25, region_filter=True)], capacity=cap, timing=True)
    rating, cons = make_pool(n, seed=1)
    d_rating = torch.from_numpy(rating).cuda()
    d_cons = torch.from_numpy(cons.view(np.int32)).cuda()
    if args.legs_only:
        out = {"workload": "cfg-2: %d players, 1v1, +-25 rating + region filter, uniform ratings, capacity %d" % (n, cap),
               "source_hash": kernel_source_hash(), "steps": args.steps, "warmup": args.warmup, "device": torch.cuda.get_device_name(0)}
        if args.partners_sorted:
            out["partners_sorted"] = measure_partners_sorted(args, rating, cons, d_rating, d_cons, 1)
        if args.move_if_sorted:
            out["move_if_sorted"] = measure_move_if_sorted(args, rating, cons, d_rating, d_cons, 1)
        print(json.dumps(out, indent=1))
        return
    if args.clock_first:
        on, off = Engine(cfg), Engine(cfg)
    else:
        off, on = Engine(cfg), Engine(cfg)
    on.clock_set(1)

    # ---- enqueue and tick, clock off / on, in turns -------------------------------------------------------------------
    rows = {"off": {"bucket_ms": [], "enqueue_total_ms": [], "tick_total_ms": [], "walk_ms": [], "step_ms": []},
            "on": {"bucket_ms": [], "enqueue_total_ms": [], "tick_total_ms": [], "walk_ms": [], "step_ms": []}}
    lobbies = {}
    now = 1
    for k in range(args.warmup + args.steps):
        for name, eng in (("off", off), ("on", on)) if k % 2 == 0 else (("on", on), ("off", off)):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            eng.reset()
            if name == "on":
                now += 10
                eng.clock_set(now)
            eng.enqueue_device(d_rating, d_cons)
            m = eng.tick(0, reuse=True)
            t1 = time.perf_counter()
            if k >= args.warmup:
                r = rows[name]
                r["bucket_ms"].append(eng.last_enqueue_stats["bucket_ms"])
                r["enqueue_total_ms"].append(eng.last_enqueue_stats["total_ms"])
                r["tick_total_ms"].append(m.stats["total_ms"])
                r["walk_ms"].append(m.stats["walk_ms"])
                r["step_ms"].append((t1 - t0) * 1e3)
            lobbies[name] = len(m)
    assert lobbies["on"] == lobbies["off"]
    w = on.matches_wait()
    assert w.shape == (lobbies["on"], 2) and not w.any()      # stamped and matched under the same clock

    # ---- mm_expire at 0 %, 1 %, 50 % and mm_wait_stats over the whole pool ---------------------------------------------
    expire = {}
    stats_ms = []
    for label, frac in (("0pct", 0.0), ("1pct", 0.01), ("50pct", 0.5)):
        old = int(n * frac)
        d_r0, d_c0, d_r1, d_c1 = d_rating[:old], d_cons[:old], d_rating[old:], d_cons[old:]
        call, got = [], None
        for k in range(args.warmup + args.steps):
            on.reset()
            now += 10
            on.clock_set(now)
            if old:
                on.enqueue_device(d_r0, d_c0)
            now += 100
            on.clock_set(now)
            on.enqueue_device(d_r1, d_c1)
            if label == "0pct":
                t0 = time.perf_counter()
                st = on.wait_stats(0)
                t1 = time.perf_counter()
                assert sum(g["waiting"] for g in st) == n
                if k >= args.warmup:
                    stats_ms.append((t1 - t0) * 1e3)
            t0 = time.perf_counter()
            got = on.expire(0, 50)
            t1 = time.perf_counter()
            assert got[0].size == old
            if k >= args.warmup:
                call.append((t1 - t0) * 1e3)
        expire[label] = {"expired": old, "call_ms": spread(call)}

    move = measure_move(args, rating, cons, d_rating, d_cons, now) if args.move else None
    carry = measure_carry(args, rating, cons, d_rating, d_cons, now) if args.carry else None
    rotate = measure_rotate(args, d_rating, d_cons, now) if args.rotate else None
    locate = measure_locate(args, d_rating, d_cons, now) if args.locate else None
    partners = measure_partners(args, rating, cons, d_rating, d_cons, now) if args.partners else None
    move_if = measure_move_if(args, rating, cons, d_rating, d_cons, now) if args.move_if else None
    partner_stats = measure_partner_stats(args, rating, cons, d_rating, d_cons, now) if args.partner_stats else None
    partners_sorted = measure_partners_sorted(args, rating, cons, d_rating, d_cons, now) if args.partners_sorted else None
    move_if_sorted = measure_move_if_sorted(args, rating, cons, d_rating, d_cons, now) if args.move_if_sorted else None

    bucket = med(rows["off"]["bucket_ms"])
    out = {
        "workload": "cfg-2: %d players, 1v1, +-25 rating + region filter, uniform ratings, capacity %d" % (n, cap),
        "source_hash": kernel_source_hash(), "steps": args.steps, "warmup": args.warmup,
        "device": torch.cuda.get_device_name(0), "created_first": "clock on" if args.clock_first else "clock off",
        "enqueue": {"bucket_ms_clock_off": spread(rows["off"]["bucket_ms"]), "bucket_ms_clock_on": spread(rows["on"]["bucket_ms"]),
                    "total_ms_clock_off": spread(rows["off"]["enqueue_total_ms"]), "total_ms_clock_on": spread(rows["on"]["enqueue_total_ms"])},
        "tick": {"total_ms_clock_off": spread(rows["off"]["tick_total_ms"]), "total_ms_clock_on": spread(rows["on"]["tick_total_ms"]),
                 "walk_ms_clock_off": spread(rows["off"]["walk_ms"]), "walk_ms_clock_on": spread(rows["on"]["walk_ms"]),
                 "step_ms_clock_off": spread(rows["off"]["step_ms"]), "step_ms_clock_on": spread(rows["on"]["step_ms"]),
                 "lobbies": lobbies["on"],
                 "note": "clock on: the tick also gathers the matched players' waits (k_wait_matched) and copies them to the host"},
        "expire": expire,
        "wait_stats": {"call_ms": spread(stats_ms)},
        "yardstick": {"bucket_ms": bucket,
                      "expire_call_over_bucket": {k: v["call_ms"]["median"] / bucket for k, v in expire.items()},
                      "wait_stats_call_over_bucket": med(stats_ms) / bucket,
                      "note": "call_ms is host time around the call (launches + synchronisation + copies), bucket_ms the HIP-event "
                              "time of three kernels: the kernels' own durations are in the kernel trace of this script"},
    }
    if move is not None:
        out["move"] = move
    if carry is not None:
        out["carry"] = carry
    if rotate is not None:
        out["rotate"] = rotate
    if locate is not None:
        out["locate"] = locate
    if partners is not None:
        out["partners"] = partners
    if move_if is not None:
        out["move_if"] = move_if
    if partner_stats is not None:
        out["partner_stats"] = partner_stats
    if partners_sorted is not None:
        out["partners_sorted"] = partners_sorted
    if move_if_sorted is not None:
        out["move_if_sorted"] = move_if_sorted
    print(json.dumps(out, indent=1))
    off.close()
    on.close()


if __name__ == "__main__":
    main()
