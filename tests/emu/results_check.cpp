// TEST INFRASTRUCTURE ONLY: the match list (struct MatchList of mm_engine.hip) driven directly on the
// fiber shim, a program of its own (`make results_check`; `make results_check_san`: address + undefined).  Its rule builds
// the three thresholds of matches_finish small (MM_PACK_MAX=8, MM_TAIL_MAX=64, MM_MAIN_COPY_MAX=16) so that made-up emission
// logs of a few hundred lobbies take all four routes.  For seeded lives over 1..MM_MAX_GROUPS groups, L in {2, 4, 10},
// uneven looks and both knobs on and off it asserts: the route is the one the documented rule predicts; r_marked <=
// r_sent <= n_out after every step, and the marks never run ahead of the wait that covers them; after the close the list
// reads back as the logs, whole and in every window on, and one off, a group boundary; exactly the emitted slots became
// FREE; counts that cannot be answer MM_ERR_INTERNAL; a dropped list answers MM_ERR_RANGE.  It says which one broke, with
// the life's number.  Exit status 0 and "results_check ok" = pass.
#include "../../microservice_matchmaking_amd/csrc/mm_engine.hip"

static unsigned g_life = 0;
#define CHECK(c, ...) do { if (!(c)) { fprintf(stderr, "results_check: life %u: %s failed (line %d): ", g_life, #c, __LINE__); fprintf(stderr, __VA_ARGS__); fprintf(stderr, "\n"); exit(1); } } while (0)
#define OK(call) do { const int rc_ = (call); CHECK(rc_ == MM_OK, "%s -> %d", #call, rc_); } while (0)

static unsigned long long rng_s = 2026;
static uint32_t rnd(uint32_t n)                    // [0, n)
{
    rng_s = rng_s * 6364136223846793005ull + 1442695040888963407ull;
    return (uint32_t)((rng_s >> 33) % n);
}

static const uint32_t CAP = 4096;
static unsigned g_routes[5];

static mm_engine* engine(uint32_t G, uint32_t L)
{
    mm_config cfg;
    OK(mm_config_default(&cfg));
    cfg.capacity = CAP;
    cfg.flags = 0;
    cfg.n_groups = G;
    cfg.default_group = 0;
    mm_mode_config& m = cfg.modes[0];
    m.team_size = L / 2u; m.teams = 2; m.n_roles = 1; m.role_quota[0] = (uint8_t)(L / 2u);
    for (uint32_t r = 1; r < MM_MAX_ROLES; ++r) m.role_quota[r] = 0;
    mm_engine* e = nullptr;
    OK(mm_engine_create(&cfg, &e));
    return e;
}

// One tick's made-up emission logs: group g emits fin[g] lobbies of L distinct LIVE slots each.
struct Life {
    uint32_t G, L, total;
    uint32_t fin[MM_MAX_GROUPS], before[MM_MAX_GROUPS], pre[MM_MAX_GROUPS + 1];
    std::vector<uint32_t> slots;                   // group-major emission order, L words a lobby
    std::vector<float> score;
    std::vector<uint32_t> pass, group;
    std::vector<uint8_t> state0;                   // h_state as the tick begins
};

static void life_make(mm_engine* e, Life& F, uint32_t scale)
{
    const uint32_t G = F.G = e->cfg.n_groups, L = F.L = e->cfg.modes[0].teams * e->cfg.modes[0].team_size;
    static const uint32_t most[4] = {8, 16, 64, 300};   // lobbies of the tick at most: around the three thresholds
    uint32_t left = 1u + rnd(most[scale]);
    if (left * L > 3000u) left = 3000u / L;
    F.total = 0;
    for (uint32_t g = 0; g < G; ++g) {
        uint32_t n = g + 1u == G ? left : rnd(left + 1u);
        if (G > 2u && rnd(4u) == 0u) n = 0;        // groups that stay at zero
        F.fin[g] = n; left -= n; F.total += n;
        F.before[g] = n * L + rnd(2u * L);
    }
    F.pre[0] = 0;
    for (uint32_t g = 0; g < G; ++g) F.pre[g + 1u] = F.pre[g] + F.fin[g];
    std::vector<uint32_t> perm(CAP);
    for (uint32_t i = 0; i < CAP; ++i) perm[i] = i;
    for (uint32_t i = CAP - 1u; i > 0; --i) std::swap(perm[i], perm[rnd(i + 1u)]);
    F.slots.assign(perm.begin(), perm.begin() + (size_t)F.total * L);
    F.score.resize(F.total); F.pass.resize(F.total); F.group.resize(F.total);
    std::fill(e->h_state.begin(), e->h_state.end(), (uint8_t)MM_ST_FREE);
    for (uint32_t s : F.slots) e->h_state[s] = MM_ST_LIVE;
    for (uint32_t i = 0; i < 40u; ++i) {           // bystanders nobody emits: they stay as they are
        const uint32_t s = perm[(size_t)F.total * L + i];
        e->h_state[s] = i % 2u ? MM_ST_LIVE : MM_ST_CANCELLED;
    }
    F.state0 = e->h_state;
    for (uint32_t g = 0; g < G; ++g)
        for (uint32_t j = 0; j < F.fin[g]; ++j) {
            const uint32_t i = F.pre[g] + j;
            F.score[i] = (float)(g * 4096u + j) * 0.25f; F.pass[i] = 7u * j + g; F.group[i] = g;
            memcpy(e->d_out_slots + (size_t)g * e->out_slot_stride + (size_t)j * L, &F.slots[(size_t)i * L], L * sizeof(uint32_t));
            e->d_out_score[(size_t)g * e->out_rec_stride + j] = F.score[i];
            e->d_out_pass[(size_t)g * e->out_rec_stride + j] = F.pass[i];
        }
}

static void invariants(const mm_engine* e, const Life& F, const char* step)
{
    for (uint32_t g = 0; g < F.G; ++g)
        CHECK(e->ml.r_marked[g] <= e->ml.r_sent[g] && e->ml.r_sent[g] <= F.fin[g], "%s: group %u marked %u sent %u n_out %u", step, g,
              e->ml.r_marked[g], e->ml.r_sent[g], F.fin[g]);
}

// ... the slots of the lobbies below r_marked are FREE, every other slot is as the tick found it
static void states(const mm_engine* e, const Life& F, const char* step)
{
    std::vector<uint8_t> want = F.state0;
    for (uint32_t g = 0; g < F.G; ++g)
        for (size_t k = (size_t)F.pre[g] * F.L; k < (size_t)(F.pre[g] + e->ml.r_marked[g]) * F.L; ++k) want[F.slots[k]] = MM_ST_FREE;
    for (uint32_t s = 0; s < CAP; ++s) CHECK(e->h_state[s] == want[s], "%s: slot %u is %u, not %u", step, s, e->h_state[s], want[s]);
}

static TickTotals totals(const Life& F, const uint32_t* n_out)
{
    TickTotals T;
    memset(&T, 0, sizeof(T));
    for (uint32_t g = 0; g < F.G; ++g) { T.n_out[g] = n_out[g]; T.had[g] = F.before[g]; T.total += n_out[g]; }
    return T;
}

// the looks of a life: n_out[] grows unevenly, some groups stop growing; returns whether a look was taken
static bool looks(mm_engine* e, const Life& F)
{
    const uint32_t n_looks = rnd(5u);
    uint32_t cur[MM_MAX_GROUPS] = {0};
    bool have = false;
    for (uint32_t k = 0; k < n_looks; ++k) {
        matches_place(e, F.before);
        CHECK(e->ml.r_based, "no bases after a look");
        for (uint32_t g = 0, run = 0; g < F.G; ++g) {      // documented: a region of before / L + 1 lobbies a group
            CHECK(e->ml.r_base[g] == run, "look %u: base of group %u is %u, not %u", k, g, e->ml.r_base[g], run);
            run += F.before[g] / F.L + 1u;
        }
        uint32_t sent0[MM_MAX_GROUPS], marked0[MM_MAX_GROUPS], fresh = 0;
        const bool pending0 = e->ml.ev_copy_pending;
        for (uint32_t g = 0; g < F.G; ++g) {
            sent0[g] = e->ml.r_sent[g]; marked0[g] = e->ml.r_marked[g];
            if (have && cur[g] > sent0[g]) fresh += cur[g] - sent0[g];
        }
        const uint32_t min_new = rnd(3u) == 0u ? 32u : 8u;
        OK(matches_ship(e, have ? cur : nullptr, min_new));
        const bool ships = have && e->tn.results_early && fresh >= min_new;
        for (uint32_t g = 0; g < F.G; ++g) {
            // the marks follow the wait: what was on its way BEFORE this call is marked, what this call sent is not
            CHECK(e->ml.r_marked[g] == (pending0 ? sent0[g] : marked0[g]), "look %u: group %u marked %u", k, g, e->ml.r_marked[g]);
            CHECK(e->ml.r_sent[g] == (ships && cur[g] > sent0[g] ? cur[g] : sent0[g]), "look %u: group %u sent %u", k, g, e->ml.r_sent[g]);
        }
        CHECK(e->ml.ev_copy_pending == ships, "look %u: copies pending %d, expected %d", k, (int)e->ml.ev_copy_pending, (int)ships);
        invariants(e, F, "look");
        states(e, F, "look");
        for (uint32_t g = 0; g < F.G; ++g)
            if (rnd(3u)) { const uint32_t slow = 1u + rnd(3u); cur[g] += rnd(F.fin[g] - cur[g] + 1u) / slow; }
        have = true;
    }
    return n_looks > 0;
}

static MatchRoute predicted(bool based, uint32_t total, uint32_t fresh, const mm_tuning& tn)
{
    if (!based && total > 0u && total <= 8u) return MR_PACKED;
    if (fresh == 0u) return MR_NONE;
    if (tn.results_tail && fresh <= 64u) return MR_TAIL;
    return fresh <= 16u ? MR_COPY_MAIN : MR_COPY_STREAM;
}

static void reads(mm_engine* e, const Life& F)
{
    const uint32_t L = F.L, n = F.total;
    std::vector<uint32_t> sl((size_t)n * L + 1u), pa(n + 1u), gr(n + 1u);
    std::vector<float> sc(n + 1u);
    std::vector<uint32_t> edges;
    for (uint32_t g = 0; g <= F.G; ++g)
        for (int d = -1; d <= 1; ++d)
            if ((int)F.pre[g] + d >= 0 && F.pre[g] + d <= n) edges.push_back(F.pre[g] + d);
    for (uint32_t a : edges)
        for (uint32_t b : edges) {
            if (b < a) continue;
            OK(matches_read(e, a, b - a, sl.data(), sc.data(), gr.data(), pa.data()));
            if (b == a) continue;                  // (an empty window anywhere in the list is no error)
            CHECK(memcmp(sl.data(), F.slots.data() + (size_t)a * L, (size_t)(b - a) * L * sizeof(uint32_t)) == 0, "slots of [%u, %u)", a, b);
            CHECK(memcmp(sc.data(), F.score.data() + a, (b - a) * sizeof(float)) == 0, "scores of [%u, %u)", a, b);
            CHECK(memcmp(pa.data(), F.pass.data() + a, (b - a) * sizeof(uint32_t)) == 0, "passes of [%u, %u)", a, b);
            CHECK(memcmp(gr.data(), F.group.data() + a, (b - a) * sizeof(uint32_t)) == 0, "groups of [%u, %u)", a, b);
        }
    CHECK(matches_read(e, n, 1, sl.data(), nullptr, nullptr, nullptr) == MM_ERR_RANGE, "a window past the end");
    CHECK(matches_read(e, 1, n, sl.data(), nullptr, nullptr, nullptr) == MM_ERR_RANGE, "a window over the end");
}

static void life(mm_engine* e, uint32_t scale)
{
    Life F;
    life_make(e, F, scale);
    e->tn.results_early = rnd(4u) ? 1u : 0u;
    e->tn.results_tail = rnd(2u);
    e->h_counters[0] = 0;                          // the liveness filter released nobody
    matches_open(e, F.L);
    invariants(e, F, "open");
    looks(e, F);
    const bool based = e->ml.r_based, pending0 = e->ml.ev_copy_pending;
    uint32_t sent0[MM_MAX_GROUPS], marked0[MM_MAX_GROUPS], fresh = 0, nrel = 77;
    for (uint32_t g = 0; g < F.G; ++g) { sent0[g] = e->ml.r_sent[g]; marked0[g] = e->ml.r_marked[g]; fresh += F.fin[g] - sent0[g]; }
    const TickTotals T = totals(F, F.fin);
    OK(matches_finish(e, T));
    const MatchRoute want = predicted(based, F.total, fresh, e->tn), got = e->ml.route;
    CHECK(got == want, "route %d, predicted %d (bases %d, total %u, fresh %u, early %u, tail %u)", (int)got, (int)want, (int)based,
          F.total, fresh, e->tn.results_early, e->tn.results_tail);
    ++g_routes[got];
    const bool waited = pending0 && got != MR_NONE;          // one batch of copies in flight at a time
    for (uint32_t g = 0; g < F.G; ++g) {
        CHECK(e->ml.r_sent[g] == F.fin[g], "finish: group %u sent %u of %u", g, e->ml.r_sent[g], F.fin[g]);
        CHECK(e->ml.r_marked[g] == (waited ? sent0[g] : marked0[g]), "finish: group %u marked %u before the tick's synchronisation", g, e->ml.r_marked[g]);
    }
    CHECK(e->ml.ev_copy_pending == (got == MR_COPY_STREAM || (pending0 && !waited)), "finish: copies pending %d", (int)e->ml.ev_copy_pending);
    if (got == MR_PACKED)
        for (uint32_t g = 0; g < F.G; ++g) CHECK(e->ml.r_base[g] == F.pre[g], "packed: base of group %u", g);
    invariants(e, F, "finish");
    states(e, F, "finish");
    const bool pending1 = e->ml.ev_copy_pending;
    for (uint32_t g = 0; g < F.G; ++g) marked0[g] = e->ml.r_marked[g];
    OK(matches_extras(e, T, &nrel));
    CHECK(nrel == 0u && !e->ml.ev_copy_pending, "extras: %u released, copies pending %d", nrel, (int)e->ml.ev_copy_pending);
    for (uint32_t g = 0; g < F.G; ++g)             // (what the copy stream brought is marked; the engine's stream is not synchronised yet)
        CHECK(e->ml.r_marked[g] == (pending1 ? F.fin[g] : marked0[g]), "extras: group %u marked %u before the tick's synchronisation", g, e->ml.r_marked[g]);
    invariants(e, F, "extras");
    matches_close(e, T);
    for (uint32_t g = 0; g < F.G; ++g)
        CHECK(e->ml.r_marked[g] == F.fin[g] && e->ml.r_sent[g] == F.fin[g], "close: group %u marked %u sent %u n_out %u", g, e->ml.r_marked[g],
              e->ml.r_sent[g], F.fin[g]);
    states(e, F, "close");                         // every emitted slot FREE, no other slot changed
    reads(e, F);
    e->ml.drop();
    uint32_t one[MM_MAX_LOBBY];
    CHECK(matches_read(e, 0, 1, one, nullptr, nullptr, nullptr) == MM_ERR_RANGE, "a read of one entry after the drop");
    OK(matches_read(e, 0, 0, one, nullptr, nullptr, nullptr));
}

// counts that cannot be: fewer lobbies than were sent, more than the group's region holds
static void impossible_counts(mm_engine* e)
{
    Life F;
    do life_make(e, F, 3); while (F.fin[0] < 20u);
    e->tn.results_early = 1; e->tn.results_tail = 1;
    e->h_counters[0] = 0;
    for (int which = 0; which < 2; ++which) {
        matches_open(e, F.L);
        matches_place(e, F.before);
        OK(matches_ship(e, F.fin, 8u));
        CHECK(e->ml.r_sent[0] == F.fin[0], "nothing was sent");
        uint32_t no[MM_MAX_GROUPS];
        memcpy(no, F.fin, sizeof(no));
        no[0] = which ? F.before[0] / F.L + 2u : F.fin[0] - 1u;
        const TickTotals T = totals(F, no);
        CHECK(matches_finish(e, T) == MM_ERR_INTERNAL, "%s", which ? "more lobbies than before / L + 1" : "a final count below what was sent");
        no[0] = F.before[0] / F.L + 1u;            // ... and the region's last place is one
        if (which) CHECK(matches_finish(e, totals(F, no)) != MM_ERR_INTERNAL, "before / L + 1 lobbies");
        e->ml.drop();
    }
}

int main()
{
    static const uint32_t Ls[3] = {2, 4, 10};
    for (uint32_t G = 1; G <= MM_MAX_GROUPS; ++G)
        for (uint32_t l = 0; l < 3; ++l) {
            mm_engine* e = engine(G, Ls[l]);
            for (uint32_t k = 0; k < 24; ++k) { ++g_life; life(e, k % 4u); }
            if (G == 3u || G == MM_MAX_GROUPS) impossible_counts(e);
            mm_engine_destroy(e);
        }
    printf("routes: none %u, packed %u, tail %u, copies on the engine's stream %u, on the copy stream %u\n", g_routes[MR_NONE],
           g_routes[MR_PACKED], g_routes[MR_TAIL], g_routes[MR_COPY_MAIN], g_routes[MR_COPY_STREAM]);
    for (int r = MR_PACKED; r <= MR_COPY_STREAM; ++r) CHECK(g_routes[r] > 0, "route %d was never taken", r);
    printf("results_check ok: %u lives\n", g_life);
    return 0;
}
