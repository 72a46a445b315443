// TEST INFRASTRUCTURE ONLY: pair_plan, the batch logic of the pair walk (DESIGN.md §4.3 "The batch logic on the host"),
// driven look by look on made-up PairChain rows: no engine, no kernel.  Seeded and deterministic.  What it asserts is what
// DESIGN.md promises (tile length, tile count, persistent batches, cool-down, stops, watchdog), knob by knob at the extremes
// of tests/stress.py's menus.  Built by `make plan_check` with the tiny geometry; exit status 0 and "plan_check ok" = pass.
#include "../../microservice_matchmaking_amd/csrc/mm_engine.hip"

static unsigned long long rng_s;
static uint32_t rnd(uint32_t n)                    // [0, n)
{
    rng_s = rng_s * 6364136223846793005ull + 1442695040888963407ull;
    return (uint32_t)((rng_s >> 33) % n);
}
#define CHECK(c, ...) do { if (!(c)) { fprintf(stderr, "plan_check: %s failed (line %d): ", #c, __LINE__); fprintf(stderr, __VA_ARGS__); fprintf(stderr, "\n"); exit(1); } } while (0)

static bool is_tiled(const PairChain& c) { return c.fast && c.stage == PS_TILED; }
static void settle(PairChain& c) { c.want_compact = 0; c.stage = c.m < PL_MAX ? PS_LATE : PS_TILED; }

struct Life {                                      // one engine's life: its knobs, its kp_rounds state, what the test expects of it
    mm_tuning tn;
    KpRoundsState K;
    mm_path_stats ps;
    PairParams P;
    PairChain rows[MM_MAX_GROUPS];
    uint32_t G, cool, stops, yields;               // expected: cool-down left, stops and yields counted so far
    bool off;                                      // expected: a PF_XCD stop was seen
};
static unsigned long long n_looks, n_next[4];      // looks taken, plans by kind

// one tick: looks until the tiled stage is over; the "device" between two looks is the few lines at the end of the loop
static void tick(Life& E, uint32_t seed)
{
    const mm_tuning& tn = E.tn;
    const uint32_t cap_on = tn.pair_ptiles < tn.pair_tiles_max ? tn.pair_ptiles : tn.pair_tiles_max;
    E.G = 1u + rnd(seed % 7u == 0u ? MM_MAX_GROUPS : 8u);
    memset(E.rows, 0, sizeof(E.rows));              // (kp_init: pfail = 0)
    for (uint32_t g = 0; g < E.G; ++g) {
        PairChain& c = E.rows[g];
        c.fast = rnd(8u) != 0u;
        c.m = rnd(3u) ? PL_MAX / 2u + rnd(tn.pair_ptiles * PK_TMAX) : PL_MAX + rnd(45u * PK_TMAX);
        c.qlen = c.m - rnd(c.m / 2u);
        settle(c);
    }
    PairLoop L;
    PairPlan pl;
    uint32_t prev_tp = 0;                          // tile length of the tick's last batch
    bool all_compacted = false;                    // a compact-everything request since that batch
    for (uint32_t look = 0;; ++look) {
        CHECK(look < 4000u, "seed %u: the tick does not end", seed);
        bool want = false, reach = true;
        uint32_t longest = 0, new_stops = 0, new_yields = 0;
        for (uint32_t g = 0; g < E.G; ++g) {
            const PairChain& c = E.rows[g];
            if (!is_tiled(c)) continue;
            want |= c.want_compact != 0;
            longest = c.m > longest ? c.m : longest;
            reach &= (c.m + PK_TMAX - 1u) / PK_TMAX <= tn.pair_ptiles;
            if (L.after_persist && c.pfail) ((c.pfail & 0xFFu) == PF_YIELD ? new_yields : new_stops) += 1u;
            if (L.after_persist && c.pfail && (c.pfail & 0xFFu) == PF_XCD) E.off = true;
        }
        if (new_stops) E.cool = 16u;
        E.stops += new_stops;
        E.yields += new_yields;
        E.ps.degraded = 0;
        const int rc = pair_plan(E.rows, E.G, tn, L, E.K, E.ps, E.P, pl);
        ++n_looks;
        CHECK(rc == MM_OK, "seed %u look %u: status %d", seed, look, rc);
        // stops: counted once, by kind, a yield costs nothing
        const uint32_t by_kind = E.ps.pair_stops_xcd + E.ps.pair_stops_inject + E.ps.pair_stops_timeout;
        CHECK(E.K.pair_pstops == E.stops && by_kind == E.stops && E.ps.pair_yields == E.yields, "seed %u look %u: %u stops (%u by kind), %u yields counted; %u and %u happened",
              seed, look, E.K.pair_pstops, by_kind, E.ps.pair_yields, E.stops, E.yields);
        CHECK(!new_stops || E.ps.degraded, "seed %u look %u: a stop without `degraded`", seed, look);
        {   // the same rows at the next look, no launch between: no counter moves
            Life S = E;
            PairLoop L2 = L;
            PairPlan p2;
            L2.after_persist = false;
            pair_plan(S.rows, S.G, tn, L2, S.K, S.ps, S.P, p2);
            CHECK(S.K.pair_pstops == E.stops && S.ps.pair_yields == E.yields && S.ps.pair_stops_xcd == E.ps.pair_stops_xcd && S.ps.pair_stops_inject == E.ps.pair_stops_inject &&
                  S.ps.pair_stops_timeout == E.ps.pair_stops_timeout, "seed %u look %u: a stop counted twice", seed, look);
        }
        ++n_next[pl.next];
        if (pl.next == PN_DONE) { CHECK(!longest, "seed %u look %u: over with a tiled chain of %u", seed, look, longest); return; }
        CHECK(longest, "seed %u look %u: no tiled chain, and not over", seed, look);
        const bool on = tn.pair_persist && !E.off, would = on && !want && reach;   // `would`: kp_rounds' kind of batch
        if (pl.next == PN_COMPACT) {
            if (pl.ask == 0xFFFFFFFFu) all_compacted = true;
            for (uint32_t g = 0; g < E.G; ++g) {
                PairChain& c = E.rows[g];
                if (is_tiled(c) && (c.want_compact || ((pl.ask >> g) & 1u))) { c.m = c.qlen; settle(c); }
            }
            continue;
        }
        // tile length: never longer than the batch before, unless everything was compacted between the two
        CHECK(!prev_tp || pl.tp <= prev_tp || all_compacted, "seed %u look %u: tile length %u after %u", seed, look, pl.tp, prev_tp);
        CHECK(pl.tp == PK_TMAX || (!tn.pair_tile_fixed && (pl.tp == PK_TMAX / 2u || pl.tp == PK_TMAX / 4u)), "seed %u look %u: tile length %u", seed, look, pl.tp);
        prev_tp = pl.tp;
        all_compacted = false;
        // tile count: covers the longest chain; within the ONE cap when a shorter tile length was chosen
        CHECK((unsigned long long)pl.tiles * pl.tp >= longest, "seed %u look %u: %u tiles of %u for a chain of %u", seed, look, pl.tiles, pl.tp, longest);
        CHECK(pl.tp == PK_TMAX || pl.tiles <= (on ? cap_on : tn.pair_tiles_max), "seed %u look %u: %u tiles of %u, kp_rounds %s", seed, look, pl.tiles, pl.tp, on ? "on" : "off");
        // persistent batches, and the cool-down: 16 batches of kp_rounds' kind go launch by launch; no other batch counts
        if (pl.next == PN_ROUNDS)
            CHECK(would && !E.cool, "seed %u look %u: a persistent batch (persist %u, off %d, cool-down %u, compaction wanted %d, within reach %d)",
                  seed, look, tn.pair_persist, (int)E.off, E.cool, (int)want, (int)reach);
        if (would && E.cool) { CHECK(E.ps.degraded, "seed %u look %u: a cool-down batch without `degraded`", seed, look); --E.cool; }
        else if (would && E.G <= 8u) CHECK(pl.next == PN_ROUNDS, "seed %u look %u: kp_round where kp_rounds was due", seed, look);   // (up to 8 chains: an XCD each, the map cannot fail)
        if (!on && !want && reach) CHECK(E.ps.degraded, "seed %u look %u: a fall-back batch without `degraded`", seed, look);
        CHECK(E.K.pair_pcool == E.cool, "seed %u look %u: cool-down %u, expected %u", seed, look, E.K.pair_pcool, E.cool);
        // the device: a stop of some kind behind a persistent batch now and then; chains shrink and are compacted
        const uint32_t inject = pl.next == PN_ROUNDS && rnd(3u) == 0u ? 1u + rnd(4u) : 0u;   // PF_TIMEOUT, PF_XCD, PF_INJECT, PF_YIELD
        const uint32_t victim = rnd(E.G);
        for (uint32_t g = 0; g < E.G; ++g) {
            PairChain& c = E.rows[g];
            if (!is_tiled(c)) continue;
            if (pl.next == PN_ROUNDS) c.pfail = inject && (g == victim || rnd(4u) == 0u) ? inject | (rnd(3u) << 8) : 0u;   // (it stays in the record)
            if (pl.next == PN_ROUNDS && inject && inject != PF_YIELD && rnd(2u)) continue;                                  // (stopped at the first barrier)
            const uint32_t n = pl.next == PN_ROUNDS ? 1u + rnd(tn.pair_pbatch) : pl.passes;
            c.passes += n; c.rounds += n; c.ppass += pl.next == PN_ROUNDS ? n : 0u;
            const uint32_t gone = rnd(c.qlen / 2u + 1u);
            c.qlen -= gone; c.n_out += gone / 2u;
            // (no kernel does this: the guard's case.  Not during a cool-down: the guard's compaction comes behind its decrement)
            if (!inject && !E.cool && rnd(100u) == 0u) c.m += rnd(4u * PK_TMAX);
            if (rnd(10u) == 0u) c.want_compact = 1u;                           // (left for the host to see)
            else if (4u * c.qlen < 3u * c.m || (E.P.pyq[g] && c.qlen <= E.P.pyq[g])) { c.m = c.qlen; settle(c); }
        }
    }
}

// the same rows again and again: MM_ERR_INTERNAL at the 65th idle look; rows that move start the count anew
static void watchdog(Life& E, uint32_t move_at)
{
    memset(E.rows, 0, sizeof(E.rows));
    E.G = 3u;
    for (uint32_t g = 0; g < E.G; ++g) { E.rows[g].fast = 1u; E.rows[g].m = E.rows[g].qlen = PL_MAX + g * PK_TMAX; settle(E.rows[g]); }
    PairLoop L;
    PairPlan pl;
    for (uint32_t look = 0, idle = 0;; ++look, ++idle) {
        if (look == move_at) { ++E.rows[1].passes; idle = 0; }
        const int rc = pair_plan(E.rows, E.G, E.tn, L, E.K, E.ps, E.P, pl);
        if (idle < 65u) CHECK(rc == MM_OK, "watchdog: status %d at idle look %u", rc, idle);
        else { CHECK(rc == MM_ERR_INTERNAL, "watchdog: status %d at idle look %u", rc, idle); return; }
    }
}

int main()
{
    static const uint32_t ptiles[2] = {3u, 32u}, tiles_max[2] = {10u, 40u}, batch[2] = {1u, 48u}, group_min[2] = {0u, 64u};
    static Life E;
    unsigned long long lives = 0;
    for (uint32_t k = 0; k < 64u; ++k)
        for (uint32_t seed = 0; seed < 48u; ++seed, ++lives) {
            memset(&E, 0, sizeof(E));
            tune_defaults(&E.tn);
            E.tn.pair_persist = k & 1u; E.tn.pair_ptiles = ptiles[(k >> 1) & 1u]; E.tn.pair_tiles_max = tiles_max[(k >> 2) & 1u];
            E.tn.pair_tile_fixed = (k >> 3) & 1u; E.tn.pair_batch = batch[(k >> 4) & 1u]; E.tn.pair_group_min = group_min[(k >> 5) & 1u];
            E.tn.debug = 0;
            rng_s = 0x9E3779B97F4A7C15ull * (k * 48u + seed + 1u);
            for (uint32_t t = 0; t < 4u; ++t) tick(E, k * 48u + seed);     // (the kp_rounds state lives on from tick to tick)
            if (seed < 2u) watchdog(E, seed ? 40u : 0xFFFFFFFFu);
        }
    CHECK(n_next[PN_ROUNDS] > 1000u && n_next[PN_ROUND] > 1000u && n_next[PN_COMPACT] > 1000u, "too few plans of a kind: %llu %llu %llu",
          n_next[PN_COMPACT], n_next[PN_ROUNDS], n_next[PN_ROUND]);
    printf("plan_check ok: %llu lives of 4 ticks, %llu looks; %llu compactions, %llu kp_rounds batches, %llu kp_round batches\n", lives, n_looks,
           n_next[PN_COMPACT], n_next[PN_ROUNDS], n_next[PN_ROUND]);
    return 0;
}
