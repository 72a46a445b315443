"""The streaming leg of the path (BASELINE cfg-5): a Poisson arrival stream, one enqueue and one
tick per mode every tick period, on one engine or on one rank's share of the chains.

What replaces what: the arrivals of a period are the deliveries `Search.Worker` would receive
(reference lib/search/worker.ex:352-358), a tick is `consume/5` run to quiescence for one mode
(worker.ex:291-324).  The stream is driven by TICK COUNT, not by wall time, so what is matched
in which tick is deterministic (and is compared with the oracle in tests/); wall time only
enters the reported latency.

Two latencies per matched player:
  real   wall time at which its lobby came back from mm_tick, minus its arrival time;
  floor  end of the tick period in which it was matched, minus its arrival time — what an
         engine with a free tick would give.  It is the time the player waited for fitting
         partners to ARRIVE (reference behaviour: a lobby waits until a fitting player is
         delivered, docs/MATCH_CHECK.md §4); real - floor is what the engine adds.
"""
from __future__ import annotations

import hashlib
import time

import numpy as np

from ._abi import MMError
from .synth import make_pool


def stream_batch(n, seed, mode_weights=None, role_weights=None):
    """One period's arrivals.  Players of mode 0 (1v1) carry no role."""
    rating, cons = make_pool(n, seed=seed, mode_weights=mode_weights, role_weights=role_weights)
    if mode_weights:
        cons = np.where((cons & 0xF) == 0, cons & ~np.uint32(0xF << 16), cons).astype(np.uint32)
    return rating, cons


def stream_schedule(qps, seconds, tick_ms, seed):
    """[(t_open, t_close, n, batch seed, sorted arrival times)] — the same on every rank."""
    rng = np.random.default_rng(seed)
    n_ticks = int(seconds * 1000.0 / tick_ms)
    out = []
    for k in range(n_ticks):
        t_open, t_close = k * tick_ms * 1e-3, (k + 1) * tick_ms * 1e-3
        n = int(rng.poisson(qps * tick_ms * 1e-3))
        out.append((t_open, t_close, n, seed + 1 + k, np.sort(rng.uniform(t_open, t_close, size=n))))
    return out


def run_stream(search, schedule, mode_weights=None, role_weights=None, realtime=True, batches=None, ttl_ms=None,
               fallback=None, rotate=None):
    """Drive `search` (a sharding.ShardedSearch: one engine + the chains this rank owns) through
    the schedule.  Returns a dict with per-mode latency arrays (real, floor), matched players,
    per-tick cost and a digest per chain of everything it emitted, in order.
    `batches`: the arrivals of every tick of the schedule, made by the caller before the clock starts
    (stream_batch(n, seed, ...) per entry — at 200 000 players a tick numpy needs longer than the 10 ms period to
    draw them, and a leg would fall behind because of the host, not the engine).
    `ttl_ms`: a search time-out (include/mm_wait.h; the reference has none).  Every period the engine's clock is set to the
    period's end in milliseconds, every mode expires whoever has waited longer than ttl_ms, then the modes tick.  The result
    then also holds `expired` (players per mode), `wait_ms` (per mode, the engine's own figure for every matched player:
    clock at its tick minus clock at its enqueue — whole periods, beside `real` and `floor`) and `depth_max` (per mode,
    the deepest the queues were after a tick).  None: no clock, nothing of this runs.
    `fallback`: rules [(from_mode, to_mode, after_ms, cons_clear)] of mm_move (include/mm_wait.h): every period, after the
    clock is set and the arrivals are in and before the expiry, whoever has waited in from_mode for longer than after_ms
    moves to to_mode with its stamp, the rules in list order (so tiers chain within a period).  A rule may carry a fifth
    element, a partner rule (_abi.PartnerRule or a dict of its fields): the move is then mm_move_if — of the players old
    enough only those whose partner count lies in the rule's range (ShardedSearch.move_if).  The clock runs as for
    ttl_ms; the result also holds `moved` and `refused` (players per rule: the ones THIS rank selected, and the ones it
    refused — on several ranks every rank calls the move collectively, sharding.ShardedSearch.move, and the sums over the
    ranks are the one-engine figures), `wait_ms` and `depth_max`.  A move that finds a destination without room
    (MM_ERR_FULL, on every rank) ends the stream like a refused batch: `full_at_s`.  With a fallback on several ranks a batch
    refused on ONE rank ends the stream on all of them (one all-reduced flag a period): the moves are collectives.
    `rotate`: {"max_seated": [per mode], "min_queue": 1, "rounds": R} of mm_rotate (include/mm_wait.h): every period, after a
    mode's tick, up to R rounds of rotate-then-tick un-block the chains whose open lobby nobody in the queue fits (a mode
    whose max_seated is 0 is left alone).  The rounds of a mode end when a rotate selected nobody or a round's tick emitted
    nothing; on several ranks each of the two is the maximum over the ranks (one all-reduce each), so every chain goes through
    the rounds it would go through on one engine.  Every round's lobbies go into the same latency arrays, wait figures and
    digests.  The clock runs as for ttl_ms; the result also holds `rotated` (players per mode, this rank's) and
    `rotate_rounds` (rounds run per mode).  A rotation without room (MM_ERR_FULL) ends the stream: `full_at_s`."""
    assert batches is None or len(batches) == len(schedule)
    fallback = list(fallback or ())
    clocked = ttl_ms is not None or bool(fallback) or rotate is not None
    cfg = search.cfg
    n_modes, n_groups = int(cfg.n_modes), int(cfg.n_groups)
    total = sum(s[2] for s in schedule)
    arrival = np.zeros(total, dtype=np.float64)                 # by global arrival index
    real = [[] for _ in range(n_modes)]
    floor = [[] for _ in range(n_modes)]
    hashers = {(m, g): hashlib.blake2b(digest_size=16) for m in range(n_modes) for g in range(n_groups)}
    emitted = {key: 0 for key in hashers}
    tick_cost = []
    matched = 0
    first = 0
    full_at_s = None
    expired = [0] * n_modes
    wait_ms = [[] for _ in range(n_modes)]
    depth_max = [0] * n_modes
    moved, refused = [0] * len(fallback), [0] * len(fallback)
    rotated, rotate_rounds = [0] * n_modes, [0] * n_modes
    if rotate is not None:
        rot_seated = [int(x) for x in rotate["max_seated"]]
        rot_queue, rot_rounds = int(rotate.get("min_queue", 1)), int(rotate.get("rounds", 1))
        assert len(rot_seated) == n_modes

    def over_ranks(*flags):
        """Each flag: true on any rank (one all-reduce for all of them; on one rank the flags themselves)."""
        if search.world_size == 1:
            return flags
        return tuple(v > 0 for v in search.max_over_ranks([1.0 if f else 0.0 for f in flags]))

    def tick_mode(md, t_close):
        """One tick of mode md into the latency arrays, wait figures and digests -> lobbies emitted."""
        nonlocal matched
        m = search.tick(md)
        t1 = time.perf_counter()
        if clocked:
            if len(m):
                wait_ms[md].append(search.engine.matches_wait().ravel().astype(np.float64))
            depth_max[md] = max(depth_max[md], int(search.engine.queue_depth(md).sum()))
        if len(m):
            ids = search.global_ids(m)
            flat = ids.ravel()
            real[md].append((t1 - t_start) - arrival[flat])
            floor[md].append(t_close - arrival[flat])
            matched += flat.size
            for g in np.unique(m.group):
                sel = np.ascontiguousarray(ids[m.group == g], dtype="<i8")
                hashers[(md, int(g))].update(sel.tobytes())
                emitted[(md, int(g))] += int(sel.shape[0])
        return len(m)

    # (a generation-2 collection of the interpreter's heap is a pause of tens of milliseconds in one tick of a real-time
    # run: nothing here makes reference cycles, so the collector rests until the stream is over)
    import gc
    gc_was = gc.isenabled()
    if realtime:
        gc.disable()
    t_start = time.perf_counter()
    try:
        for k, (t_open, t_close, n, sd, ts) in enumerate(schedule):
            rating, cons = batches[k] if batches is not None else stream_batch(n, sd, mode_weights, role_weights)
            arrival[first:first + n] = ts
            if realtime:
                # the period has to be over: sleep through most of it and spin only for the last stretch (a thread that spins
                # all the time is the first one a CPU quota throttles, for tens of milliseconds at a time)
                while True:
                    left = t_close - (time.perf_counter() - t_start)
                    if left <= 0:
                        break
                    if left > 0.0006:
                        time.sleep(left - 0.0004)
            t0 = time.perf_counter()
            if clocked:
                search.engine.clock_set(int(round(t_close * 1e3)))  # this period's arrivals are stamped with its end
            refused_here = False
            try:
                search.enqueue(rating, cons, first_global_index=first)
            except MMError as ex:
                if ex.status != -4:                                 # MM_ERR_FULL: fewer than n free slots in the pool
                    raise
                refused_here = True
            if fallback and search.world_size != 1:
                # the moves below are collectives: a rank that left the loop alone would leave the others waiting in them,
                # so with a fallback on several ranks a batch refused on ONE rank ends the stream on all
                refused_here = max(search.max_over_ranks([1.0 if refused_here else 0.0])) > 0
            if refused_here:
                # The batch is refused as a whole and nothing of it was queued (include/mm_engine.h): for the
                # service these deliveries stay unacked in the broker (prefetch back-pressure,
                # lib/search/worker.ex:29) until lobbies free slots.  The stream ends here and says so.
                full_at_s = t_open
                break
            first += n
            try:
                for i, (src, dst, after_ms, cons_clear, *rule) in enumerate(fallback):
                    if rule:
                        got = search.move_if(src, dst, int(after_ms), int(cons_clear), rule[0])
                    else:
                        got = search.move(src, dst, int(after_ms), int(cons_clear))
                    moved[i] += int(got[0].size)
                    refused[i] += int((search.engine if search.world_size == 1 else search).last_move["refused"])
            except MMError as ex:
                if ex.status != -4:                                 # MM_ERR_FULL: no room for the moved players where they go
                    raise
                full_at_s = t_open
                break
            if ttl_ms is not None:
                for md in range(n_modes):
                    expired[md] += int(search.engine.expire(md, int(ttl_ms))[0].size)
            for md in range(n_modes):
                tick_mode(md, t_close)
                if rotate is None or rot_seated[md] == 0:
                    continue
                for _ in range(rot_rounds):
                    k_sel, full = 0, False
                    try:
                        k_sel = int(search.rotate(md, rot_seated[md], rot_queue)[0].size)
                    except MMError as ex:
                        if ex.status != -4:                         # MM_ERR_FULL: no free slots beside the rotated players
                            raise
                        full = True
                    rotated[md] += k_sel
                    some, full = over_ranks(k_sel > 0, full)        # one decision for all ranks: they tick the same rounds
                    if full:
                        full_at_s = t_open
                    if full or not some:
                        break
                    rotate_rounds[md] += 1
                    if not over_ranks(tick_mode(md, t_close) > 0)[0]:
                        break
                if full_at_s is not None:
                    break
            if full_at_s is not None:
                break
            tick_cost.append(time.perf_counter() - t0)
    finally:
        # whatever ends the loop (a refused batch is handled above; a failed tick, Ctrl-C): the interpreter gets its collector back
        if realtime and gc_was:
            gc.enable()
    elapsed = time.perf_counter() - t_start
    depth = [search.engine.queue_depth(md).astype(np.int64) for md in range(n_modes)]
    cat = lambda parts: np.concatenate(parts) if parts else np.zeros(0)
    out = {
        "real": [cat(x) for x in real], "floor": [cat(x) for x in floor],
        "matched": matched, "elapsed": elapsed, "tick_cost": np.asarray(tick_cost),
        "depth": depth, "digests": {k: h.hexdigest() for k, h in hashers.items()}, "lobbies": emitted,
        "arrivals": total, "ingested": first, "full_at_s": full_at_s,
    }
    if clocked:
        out.update({"wait_ms": [cat(x) for x in wait_ms], "depth_max": depth_max})
    if ttl_ms is not None:
        out["expired"] = expired
    if fallback:
        out.update({"moved": moved, "refused": refused})
    if rotate is not None:
        out.update({"rotated": rotated, "rotate_rounds": rotate_rounds})
    return out


def latency_summary(real, floor):
    """p50 / p99 / max of the real latency and of the arrival-limited floor, in ms."""
    if real.size == 0:
        return {"p50_ms": None, "p99_ms": None, "max_ms": None, "floor_p50_ms": None, "floor_p99_ms": None,
                "matched_players": 0}
    return {"p50_ms": float(np.percentile(real, 50) * 1e3), "p99_ms": float(np.percentile(real, 99) * 1e3),
            "max_ms": float(real.max() * 1e3),
            "floor_p50_ms": float(np.percentile(floor, 50) * 1e3), "floor_p99_ms": float(np.percentile(floor, 99) * 1e3),
            "engine_added_p99_ms": float(np.percentile(real - floor, 99) * 1e3),
            "matched_players": int(real.size)}
