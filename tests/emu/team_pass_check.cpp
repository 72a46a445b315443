// TEST INFRASTRUCTURE ONLY: the team walk's pass (mm_team.inc: head_fill, open_lobby_close, pass_close, the kills) through the
// C ABI on the fiber shim, as a program of its own so that it can be built under sanitizers (`make team_pass_check_san`:
// address + undefined, tiny geometry; device memory is malloc'ed under the shim, so a kernel reading or writing past a buffer
// is reported).  Two parts: the hand-built scenario of helpers.run_anchor_moves_to_the_emptied_first_team (a stale lobby, a
// head that sits out, an anchor that moves to the emptied team mid-fill, a lobby left open, then a stored lobby that the
// head of the queue fills), with its lobbies checked; and one random 3v3 pool with cancels over four ticks, whose checksum
// is printed (the same under every launch shape: run it with MM_TEAM_F2=0, MM_TEAM_LATE=0, MM_TEAM_LATE0=10000000).
// And two scenarios of tests/stale_lobby_scenarios.py with team_late0 set high, so that the cancel tick runs in kt_late:
// head_fill's restart behind an anchor that moved, and the lobby it fills emitted on the spot (head_cancelled_move_fills,
// head_taken_late_move_fills; the derivations stand there).
// Exit status 0 and "team_pass_check ok" = pass.
#include "../../microservice_matchmaking_amd/csrc/mm_engine.hip"

#define CHECK(c, ...) do { if (!(c)) { fprintf(stderr, "team_pass_check: %s failed (line %d): ", #c, __LINE__); fprintf(stderr, __VA_ARGS__); fprintf(stderr, "\n"); exit(1); } } while (0)
#define OK(call) do { const int rc_ = (call); CHECK(rc_ == MM_OK, "%s -> %d", #call, rc_); } while (0)

static unsigned long long rng_s = 12345;
static uint32_t rnd(uint32_t n)                    // [0, n)
{
    rng_s = rng_s * 6364136223846793005ull + 1442695040888963407ull;
    return (uint32_t)((rng_s >> 33) % n);
}

static mm_engine* engine(uint32_t team_size, uint32_t teams, uint32_t window, uint32_t n_roles, const uint8_t* quota, uint32_t capacity)
{
    mm_config cfg;
    OK(mm_config_default(&cfg));
    cfg.capacity = capacity;
    cfg.flags = 0;
    mm_mode_config& m = cfg.modes[0];
    m.team_size = team_size; m.teams = teams; m.window = window; m.flags = 0; m.n_roles = n_roles;
    for (uint32_t r = 0; r < MM_MAX_ROLES; ++r) m.role_quota[r] = r < n_roles ? quota[r] : 0;
    mm_engine* e = nullptr;
    OK(mm_engine_create(&cfg, &e));
    return e;
}

static void anchor_moves()
{
    const uint8_t quota[1] = {2};
    mm_engine* e = engine(2, 2, 100, 1, quota, 4096);
    int32_t r1[73] = {500, 510, 520};              // A, B, C and seventy bystanders nobody near 500 fits
    uint32_t c1[73] = {0}, s1[73], n = 0, nm = 0, ls[MM_MAX_LOBBY];
    uint8_t lt[MM_MAX_LOBBY];
    for (int i = 0; i < 70; ++i) r1[3 + i] = 1000 + 5 * i;
    OK(mm_enqueue(e, 73, r1, c1, nullptr, s1, nullptr));
    OK(mm_tick(e, 0, &nm, nullptr));
    OK(mm_lobby_state(e, 0, 0, &n, ls, lt));
    CHECK(nm == 0 && n == 3 && ls[0] == s1[0] && ls[1] == s1[2] && ls[2] == s1[1], "tick 1: %u lobbies, %u stored", nm, n);
    const uint32_t gone[2] = {s1[0], s1[2]};       // A and C cancel: team 2: [B] is left
    OK(mm_cancel(e, 2, gone));
    const int32_t r2[3] = {600, 690, 450};         // D, E, F
    const uint32_t c2[3] = {0, 0, 0};
    uint32_t s2[3];
    OK(mm_enqueue(e, 3, r2, c2, nullptr, s2, nullptr));
    OK(mm_tick(e, 0, &nm, nullptr));
    OK(mm_lobby_state(e, 0, 0, &n, ls, lt));
    CHECK(nm == 0 && n == 3 && ls[0] == s2[0] && ls[1] == s1[1] && ls[2] == s2[1] && lt[0] == 0 && lt[1] == 1 && lt[2] == 1,
          "tick 2: %u lobbies, %u stored", nm, n);
    const int32_t r3 = 650;                        // G
    const uint32_t c3 = 0;
    uint32_t s3, first[4];
    OK(mm_enqueue(e, 1, &r3, &c3, nullptr, &s3, nullptr));
    OK(mm_tick(e, 0, &nm, nullptr));
    CHECK(nm >= 1, "tick 3: no lobby");
    OK(mm_matches(e, 0, 1, first, nullptr, nullptr, nullptr));
    CHECK(first[0] == s2[0] && first[1] == s3 && first[2] == s1[1] && first[3] == s2[1], "tick 3: the first lobby");
    printf("anchor_moves: tick 3 emits %u lobbies\n", nm);
    mm_engine_destroy(e);
}

static void random_pool()
{
    const uint8_t quota[2] = {2, 1};
    mm_engine* e = engine(3, 2, 400, 2, quota, 1u << 13);
    static int32_t rating[4000];
    static uint32_t cons[4000], slot[4000], live[8000], out[4000 * 6];
    uint32_t n_live = 0;
    unsigned long long sum = 0;
    for (int t = 0; t < 4; ++t) {
        const uint32_t n = t == 0 ? 3000u : 400u;
        for (uint32_t i = 0; i < n; ++i) {
            rating[i] = (int32_t)rnd(1400u);       // one rating group: one chain on the team path
            cons[i] = MM_CONS_MAKE(0u, 0u, 0u, rnd(3u) == 0u ? 1u : 0u);
        }
        OK(mm_enqueue(e, n, rating, cons, nullptr, slot, nullptr));
        for (uint32_t i = 0; i < n; ++i) live[n_live++] = slot[i];
        if (t >= 1) {                              // cancels: waiting players and members of the stored lobby alike
            uint32_t cs[40];
            for (uint32_t i = 0; i < 40u; ++i) cs[i] = live[rnd(n_live)];
            OK(mm_cancel(e, 40, cs));
        }
        uint32_t nm = 0;
        mm_stats st;
        OK(mm_tick(e, 0, &nm, &st));
        CHECK(nm * 6u <= sizeof(out) / sizeof(out[0]), "%u lobbies", nm);
        OK(mm_matches(e, 0, nm, out, nullptr, nullptr, nullptr));
        for (uint32_t i = 0; i < nm * 6u; ++i) sum = sum * 1000003ull + out[i];
        sum = sum * 1000003ull + st.pairs + st.passes_max;
        printf("random_pool: tick %d: %u lobbies, %u passes\n", t, nm, st.passes_max);
    }
    printf("random_pool: checksum %016llx\n", sum);
    mm_engine_destroy(e);
}

// One rating group that holds every rating below; kt_late walks every tick from its first pass (unless MM_TEAM_LATE=0 turns it off).
static mm_engine* engine_late(uint32_t team_size, uint32_t teams)
{
    mm_config cfg;
    OK(mm_config_default(&cfg));
    cfg.capacity = 4096;
    cfg.flags = 0;
    cfg.n_groups = 1; cfg.groups[0].from = -100000; cfg.groups[0].to = 10000000; cfg.default_group = 0;
    mm_mode_config& m = cfg.modes[0];
    m.team_size = team_size; m.teams = teams; m.window = 100; m.flags = 0; m.n_roles = 1;
    for (uint32_t r = 0; r < MM_MAX_ROLES; ++r) m.role_quota[r] = r == 0 ? team_size : 0;
    mm_tuning t;
    t.size = sizeof(t);
    OK(mm_tuning_default(&t));
    OK(mm_tuning_set(&t, "team_late0", 10000000u));
    mm_engine* e = nullptr;
    OK(mm_engine_create_ex(&cfg, &t, &e));
    return e;
}

// the cancel tick ran in kt_late from its first pass to its last (where kt_late is on)
static void check_late(mm_engine* e, const char* what)
{
    mm_tuning t;
    t.size = sizeof(t);
    OK(mm_tuning_get(e, &t));
    mm_path_stats ps;
    ps.size = sizeof(ps);
    OK(mm_path_stats_get(e, &ps));
    if (t.team_late != 0u)
        CHECK(ps.team_late_launches >= 1u && ps.crit_team_late_passes == ps.crit_team_passes && ps.crit_team_passes >= 1u &&
              ps.crit_team_f_passes == 0u && ps.crit_team_fc_passes == 0u, "%s: %u launches of kt_late, %u of %u passes", what,
              ps.team_late_launches, ps.crit_team_late_passes, ps.crit_team_passes);
}

enum { NBY = 70 };                                 // bystanders: 5000 + 101 i, nobody fits them and they fit nobody
static uint32_t bystanders(int32_t* r, uint32_t at)
{
    for (int i = 0; i < NBY; ++i) r[at + i] = 5000 + 101 * i;
    return at + NBY;
}

static void expect_rows(mm_engine* e, uint32_t nm, const uint32_t* want, uint32_t rows, uint32_t L, const char* what)
{
    uint32_t got[3 * MM_MAX_LOBBY];
    CHECK(nm == rows && rows <= 3u, "%s: %u lobbies, not %u", what, nm, rows);
    OK(mm_matches(e, 0, nm, got, nullptr, nullptr, nullptr));
    for (uint32_t i = 0; i < rows * L; ++i) CHECK(got[i] == want[i], "%s: lobby %u seat %u is slot %u, not %u", what, i / L, i % L, got[i], want[i]);
}

// stale_lobby_scenarios.py head_cancelled_move_fills (A1 x B1 x C2), 2v2
static void head_cancelled_move_fills()
{
    mm_engine* e = engine_late(2, 2);
    int32_t r1[3 + NBY] = {500, 510, 520};         // A, B, C
    uint32_t c1[3 + NBY] = {0}, s1[3 + NBY], n = 0, nm = 0, ls[MM_MAX_LOBBY];
    uint8_t lt[MM_MAX_LOBBY];
    const uint32_t n1 = bystanders(r1, 3);
    OK(mm_enqueue(e, n1, r1, c1, nullptr, s1, nullptr));
    OK(mm_tick(e, 0, &nm, nullptr));
    OK(mm_lobby_state(e, 0, 0, &n, ls, lt));
    CHECK(nm == 0 && n == 3 && ls[0] == s1[0] && ls[1] == s1[2] && ls[2] == s1[1], "tick 1: %u lobbies, %u stored", nm, n);
    const int32_t r2[13] = {680, 600, 690, 450, 650, 3000, 3001, 3002, 3003, 3004, 3005, 3006, 3007};   // P, D, E, F, G, h0..h7
    const uint32_t c2[13] = {0};
    uint32_t s2[13];
    OK(mm_enqueue(e, 13, r2, c2, nullptr, s2, nullptr));
    const uint32_t gone[3] = {s1[0], s1[2], s1[3]};   // A, C and the head of the queue
    OK(mm_cancel(e, 3, gone));
    OK(mm_tick(e, 0, &nm, nullptr));
    const uint32_t want[12] = {s2[1], s2[4], s1[1], s2[2],  s2[5], s2[7], s2[6], s2[8],  s2[9], s2[11], s2[10], s2[12]};
    expect_rows(e, nm, want, 3, 4, "head_cancelled_move_fills");
    OK(mm_lobby_state(e, 0, 0, &n, ls, lt));
    CHECK(n == 1 && ls[0] == s1[4] && lt[0] == 0, "tick 2: %u stored", n);
    check_late(e, "head_cancelled_move_fills");
    printf("head_cancelled_move_fills: tick 2 emits %u lobbies\n", nm);
    mm_engine_destroy(e);
}

// stale_lobby_scenarios.py head_taken_late_move_fills (A3 x B5 x C2), 3v3 with negative ratings
static void head_taken_late_move_fills()
{
    mm_engine* e = engine_late(3, 2);
    const int32_t r1[4] = {-500, -510, -520, -530};   // A, B, C, D
    const uint32_t c1[4] = {0};
    uint32_t s1[4], n = 0, nm = 0, ls[MM_MAX_LOBBY];
    uint8_t lt[MM_MAX_LOBBY];
    OK(mm_enqueue(e, 4, r1, c1, nullptr, s1, nullptr));
    OK(mm_tick(e, 0, &nm, nullptr));
    OK(mm_lobby_state(e, 0, 0, &n, ls, lt));
    CHECK(nm == 0 && n == 4 && ls[0] == s1[0] && ls[1] == s1[1] && ls[2] == s1[2] && ls[3] == s1[3] && lt[2] == 0 && lt[3] == 1,
          "tick 1: %u lobbies, %u stored", nm, n);
    int32_t r2[19 + NBY] = {-505, -370, -540, -450, -360, -620, -400};   // H, P, K1, M, E, F, G, then h0..h11
    uint32_t c2[19 + NBY] = {0}, s2[19 + NBY];
    for (int i = 0; i < 12; ++i) r2[7 + i] = 3000 + i;
    const uint32_t n2 = bystanders(r2, 19);
    OK(mm_enqueue(e, n2, r2, c2, nullptr, s2, nullptr));
    OK(mm_cancel(e, 3, s1));                       // A, B, C
    OK(mm_tick(e, 0, &nm, nullptr));
    const uint32_t* const h = s2 + 7;
    const uint32_t want[18] = {s2[3], s2[4], s2[6], s1[3], s2[0], s2[2],  h[0], h[2], h[4], h[1], h[3], h[5],  h[6], h[8], h[10], h[7], h[9], h[11]};
    expect_rows(e, nm, want, 3, 6, "head_taken_late_move_fills");
    OK(mm_lobby_state(e, 0, 0, &n, ls, lt));
    CHECK(n == 1 && ls[0] == s2[19] && lt[0] == 0, "tick 2: %u stored", n);
    check_late(e, "head_taken_late_move_fills");
    printf("head_taken_late_move_fills: tick 2 emits %u lobbies\n", nm);
    mm_engine_destroy(e);
}

int main()
{
    anchor_moves();
    random_pool();
    head_cancelled_move_fills();
    head_taken_late_move_fills();
    printf("team_pass_check ok\n");
    return 0;
}
