// mm_team.inc — the team-mode walk (anything that is not 1v1: team_size > 1 or more than two
// teams), included by mm_engine.hip after mm_pair.inc (it shares the packed key, pk_*).
//
// What it computes: Search.Worker.consume/5 (reference lib/search/worker.ex:291-324) under the
// canonical schedule (docs/MATCH_CHECK.md §4) for one mode, every rating group, cancel ticks
// included (k_purge first; kt_init then applies the stale-lobby rule).  Chains it does not take
// (short ones, a rating span over 2^19) are walked by k_walk in the same tick.
//
// The observation that makes a pass parallel (docs/MATCH_CHECK.md §2.3-2.4): whether a popped
// player is SEATED depends only on the anchor (window + filters) and on how many players of
// its role the lobby holds over all teams — a team with a free seat of the role exists exactly
// when that count is below teams * quota[role].  Which team it lands in (the rating-sum rule)
// never changes who is seated.  So the lobby an anchor `a` opens consists of, per role r, the
// first  teams*quota[r] - [role(a) = r]  queued players after `a` that fit `a`, and it is filled
// by the last of them in queue order.  Nobody before the cursor is looked at again within a
// pass, so
//     F[a] = the player the cursor picks after a's lobby is emitted
// is a function of the queue as it stands when the pass begins, for EVERY queued a at once,
// and the pass itself is the pointer chase  a -> F[a] -> F[F[a]] ...  from the head.
//
// The work of a pass (all chains and all 512-position chunks of the queue):
//   kt_build  (first two passes of a tick, then every eighth) stable partition of the queued players by
//             role into sub-queues (key, position), per 64-block role ranks (ballot + popcount); between
//             two rebuilds a player that leaves the queue is a tombstone in its sub-queue
//   kt_f      F for every queued player, incrementally: the lobby an anchor opens is on record; members
//             that left the queue are REPLACED (the first entries that fit behind the role's last member
//             in its sub-queue: round 4), only an anchor without a record is looked up from scratch (scan
//             of the role sub-queues from its rank); also the pass's snapshot of the bitmap
//   kt_f2     (first 32 passes) F o F, so that the chase takes two lobbies per trip to memory
//   chase     one workgroup per chain; wave 0: the stored lobby's fill from the head of the queue (emitted
//             on the spot if it fills), the chase over F, the lobby left open at the end of the pass; its
//             look-ups role by role on the workgroup's other waves (LookCtl)
//   emit      one wave per emitted lobby: the members (from kt_f's record), the seats replayed in queue
//             order (the team choice needs the order), the lobby written, the players taken out
// and its launches:
//   passes with kt_f2 (lobby-rich: hundreds per pass)   kt_f (+ a column of workgroups that fill the stored
//             lobbies from the heads of the queues meanwhile) | kt_f2 | kt_chase — the chasers, their
//             other waves pulling F and F o F through the XCD's L2, and the EMITTER workgroups, which
//             take the lobbies off vis[] while the chase is still running
//   the passes after them                               kt_fc — chasers, emitters and kt_f's chunks in
//             ONE launch: a chaser takes F[a] as soon as the flag of a's chunk is up, so the chase runs
//             beside kt_f instead of behind it
//   the last passes (a handful of lobbies each)         kt_late, once: one persistent workgroup per chain
// Written once for the pass kernels' chaser (tc_chaser) and kt_late's: the close of a pass (pass_close), a player's leaving the
// queue (tq_leave), the tail of an emission (emit_members), lobby_clear, lobby_needs.  The stored lobby's fill from the head of
// the queue and the lobby left open stand twice, in tc_chaser and in kt_late's head_fill / open_lobby_close (see there).
//   (Rounds 2-5 could also run kt_f | kt_chase | kt_emit one behind the other — MM_TEAM_LIVE=0 / MM_TEAM_FUSED=0; taken out in round 6.)
// What workgroups of one launch tell each other goes through agent-scope atomics (pub_st / pub_ld);
// the one that waits always has the lower index, i.e. is dispatched first.
// Chunk populations per role are kept current by the kills (atomicSub), so there is no count
// kernel after the first pass.
//
// Arrays are the pair path's (never used in the same tick): DESIGN.md §4.4.

#define TT_NONE 0xFFFFFFFFu          // F: the lobby fills and nobody is queued behind it
#define TT_PART 0xFFFFFFFEu          // F: the lobby cannot fill in this pass
#define TT_UNK 0xFFFFFFFDu           // F: scan cap reached, kt_chase looks itself
#define TT_FAR 0xFFFFFFFAu            // kt_f's fix-up, inside tf_chunk only: a replacement member 2^16 positions away
#define TT_WAIT 0xFFFFFFFBu          // tcf_load: the chunk's flag did not come in time — the chaser looks itself AND says so in vis[]
#define TV_AHEAD 512u                // vis[]: entries behind the published ones an emitter's dispatcher may look at (>= TC_EMIT_MAX * TC_WAVES)
#define TV_LOOKED 0x40000000u        // vis[]: "the chaser looked this lobby up itself, kt_f's record of the anchor may be in the making"
#ifndef TT_CH
#define TT_CH 512u                   // positions per workgroup of the chunk kernels (a multiple of 64)
#endif
#define TT_WAVES (TT_CH / 64u)
#define TT_WORDS (TT_CH / 32u)
#ifndef TT_MIN
#define TT_MIN 4096u                 // shorter chains stay with k_walk (launch bound)
#endif
#define TT_MAX (1u << 22)            // longer chains stay with k_walk (kt_build sums the chunk counters per workgroup)
#ifndef TT_SCAN_CAP
#define TT_SCAN_CAP 512u            // sub-queue entries one thread of kt_f looks at per role
#endif
#ifndef TF_PAD
#define TF_PAD 240u                  // kt_f stages a chunk's own players of a role + this many in LDS
#endif

struct TeamChain {
    uint32_t fast, done, m, qlen;
    int32_t rmin;
    uint32_t passes, n_out, before, err;
    unsigned long long pairs, scanned;
    uint32_t len[MM_MAX_ROLES], off[MM_MAX_ROLES];   // sub-queues of the current pass
    uint32_t n_vis, head, out_base, cur_pass;        // kt_chase -> kt_emit
    uint32_t sitout, extra0, changed0, head_role;    // cancel tick: what the head's attempt against the stale lobby did
    uint32_t dbg[8];
    uint32_t tmk[8];                                 // MM_PAIR_DEBUG: phase timers of kt_f's workgroup of chunk 1 (cycles, summed over the passes)
    uint32_t lt[16];                                 // MM_PAIR_DEBUG: kt_late — passes, lobbies by record / by look-up, open look-ups, fills,
                                                     //   sub-queue entries scanned per role [5..9], cycles: records, look-ups, fills, all, ring waits
    // kt_chase -> the emitter workgroups of the SAME launch (agent-scope atomics; P.seq names the launch)
    unsigned long long pub_go;                       // P.seq << 32 | the out index of vis[0]'s lobby: the emitters may start
    unsigned long long pub_end;                      // P.seq << 32 | anchors in vis[]: the pass is over
    uint32_t pub_pass, flags_late;                   // the pass number (stored before pub_go); kt_fc: anchors whose chunk flag did not come in time this
                                                     //   tick — the chaser looked the lobby up itself (mm_path_stats: a slower pass, never a wrong one)
    // the stored lobby's fill from the head of the queue, done in kt_f's launch (tc_chaser<.., 1>) -> the chase in kt_chase's (<.., 2>)
    uint32_t h_a, h_flags, h_gone, h_err, h_fill, h_pad;   // where the chase begins; head | changed << 1 | over << 2; players it took; errors; debug count
    // what the chaser did this tick, by launch shape (mm_path_stats crit_team_*): passes as kt_f | kt_f2 | kt_chase, as kt_fc, inside
    // kt_late [0..2]; lobbies it reached in them [3..5]; look-ups it did itself in the pass kernels [6], inside kt_late [7]
    uint32_t cp[8];
};

struct TeamParams {
    uint32_t mode, n_groups, capacity, window, eqmask;
    uint32_t out_cap, out_slot_stride, out_rec_stride;
    uint32_t bits_stride, pstride, chunk_stride, blk_stride;
    uint32_t purge;      // a cancel is pending: k_purge ran, ChainDev.head_state is valid
    uint8_t* state;      // ActiveUser mirror
    uint32_t* released;  // slots the liveness filter released
    uint32_t* n_released;
    uint32_t scan_cap;   // sub-queue entries one thread of kt_f looks at per role before it gives up (TT_UNK)
    uint32_t late_bail;  // kt_late hands a chain back after a pass that seated more lobbies than this
    uint32_t debug;      // MM_PAIR_DEBUG: phase timers of one kt_f workgroup in TeamChain.dbg
    uint32_t fwait;      // kt_fc: polls a chaser waits for the flag of a kt_f chunk before it looks the lobby up itself (MM_TEAM_FWAIT)
    uint32_t nowait;     // test hook (MM_TEAM_NOWAIT=n): the flag of every n-th chunk never comes
    uint32_t fix_max;    // kt_f: a chunk with more (anchor, role) replacements than this looks its lobbies up from scratch (MM_TEAM_FIXMAX)
    uint32_t fix_t8, fix_t4;   // kt_f: a wave with more replacements than this gives each eight / four lanes instead of sixteen (MM_TEAM_FIXT8 / _FIXT4)
    uint32_t hf_x;       // kt_f: the workgroups with this blockIdx.x fill the stored lobbies from the heads of the queues while the chunks work (0xFFFFFFFF: kt_chase does, MM_TEAM_SPLIT=0)
    uint32_t pull_xcd;   // kt_chase: the chain's emitter workgroups on the chaser's XCD pull F and F o F through its L2 first (MM_TEAM_PULLX=0: off)
    uint32_t act;        // bit g: chain g was still walked when the host last looked (kt_f's workgroups of the others leave without a load)
    // kt_fc: kt_f's workgroups in the order the chasers need them — the chains aligned at their ENDS, by falling
    // distance to the end: a chaser finishes when the last chunk of its chain is done, plus the hops that are left
    // from there, so the chunks with the longest way to go come first.  Segment s: the s + 1 longest chains, distances
    // fo_dhi[s] down to fo_dhi[s + 1] + 1, from workgroup fo_start[s]; fo_chain / fo_nch: the chains by falling length.
    uint32_t fo_n, fo_start[MM_MAX_GROUPS + 1], fo_dhi[MM_MAX_GROUPS + 1], fo_chain[MM_MAX_GROUPS], fo_nch[MM_MAX_GROUPS];
    uint32_t seq;        // kt_chase launches of this tick so far, this one included (never 0)
    uint32_t n_emit;     // emitter workgroups per rating group behind the launch's chasers (>= 1)
    ModeDev M;
    ChainDev* chains;
    TeamChain* tchains;
    int32_t* q_rating;
    uint32_t* q_cons;
    uint32_t* q_slot;
    uint32_t* tkey;      // [group][pstride] packed key by queue position
    uint32_t* bits[2];   // [group][bits_stride] queued bitmap: [0] as the pass began, [1] current
    uint32_t* bitsB;     // [group][bits_stride] ... as it was when kt_build last split the queue by role: what the ranks count
    uint32_t* sqk;       // [group][pstride] sub-queues: keys, role segments back to back
    uint32_t* sqp;       //                  ... positions
    uint32_t* fv;        // [group][pstride] F
    uint32_t* fpos;      // [group][pstride] kt_f's record: the last member of the lobby the position opens (TT_NONE: none)
    uint16_t* memb;      // [group][pstride][L - 1] ... and every member, as its distance from the position
    uint32_t* fv2;       // [group][pstride] F o F (kt_f2; only in the lobby-rich passes at the start of a tick)
    uint32_t use_f2;     // this pass has fv2
    uint32_t* vis;       // [group][pstride] anchors of the lobbies the pass emits, in order
    uint32_t* blkbase;   // [group][role][blk_stride] players of the role queued before the 64-block
    uint32_t* chunk;     // [group][role][chunk_stride] players of the role queued in the chunk
    uint32_t* chunkB;    // [group][role][chunk_stride] ... when kt_build last ran: the chunk's entries in the sub-queues
    uint32_t* sqi;       // [group][pstride] where kt_build put the position in the sub-queues (for the tombstone)
    uint32_t* fdone;     // [group][chunk_stride] kt_fc: P.seq of the launch whose kt_f chunk has stored its F
    uint32_t* out_slots;
    float* out_score;
    uint32_t* out_pass;
};

struct TwScratch {       // one wave's lobby under construction (LDS)
    uint32_t pos[MM_MAX_LOBBY], spos[MM_MAX_LOBBY];
    int32_t rat[MM_MAX_LOBBY];
    uint32_t con[MM_MAX_LOBBY], slo[MM_MAX_LOBBY];
    uint32_t sqx[MM_MAX_LOBBY];                              // where the player stands in its role's sub-queue (tw_sort_load -> tq_kill)
};

// What workgroups of ONE launch tell each other (kt_chase's chaser -> its emitter workgroups; kt_fc's kt_f chunks
// -> its chasers): agent scope, through to memory.  Workgroups are dispatched in index order, and the one that
// is waited for always has the lower index.
static __device__ __forceinline__ void pub_st(uint32_t* p, uint32_t v) { __hip_atomic_store(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
static __device__ __forceinline__ uint32_t pub_ld(const uint32_t* p) { return uni(__hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)); }
static __device__ __forceinline__ unsigned long long pub_ld64(const unsigned long long* p)
{
    const unsigned long long v = __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    return ((unsigned long long)uni((uint32_t)(v >> 32)) << 32) | uni((uint32_t)v);
}
static __device__ __forceinline__ void pub_st64(unsigned long long* p, unsigned long long v) { __hip_atomic_store(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
#define TC_SPIN_MAX (1u << 21)       // polls before a waiting wave gives the tick up (seconds: the other side died)

static __device__ __forceinline__ uint32_t wave_sum(uint32_t v, int lane)
{
    for (int d = 1; d < 64; d <<= 1) v += (uint32_t)__shfl((int)v, lane ^ d);
    return v;
}
// ------------------------------------------------------------------------------------
// kt_init: one workgroup per rating group — rating span, eligibility, the tick's counters.
// ------------------------------------------------------------------------------------
__global__ __launch_bounds__(1024) void kt_init(TeamParams P)
{
    __shared__ int32_t s_lo[16], s_hi[16];
    __shared__ LobbyDev s_lb;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const uint32_t g = blockIdx.x;
    const uint32_t c = P.mode * P.n_groups + g;
    ChainDev* const ch = P.chains + c;
    TeamChain* const tc = P.tchains + g;
    const size_t qo = (size_t)c * P.capacity;
    const int32_t* const qr = P.q_rating + qo;
    const ModeDev& M = P.M;
    const uint32_t m = ch->len;
    int32_t lo = 0x7FFFFFFF, hi = (int32_t)0x80000000;
    uint32_t i0 = tid;                                    // (eight loads in flight per thread, as in kp_init)
    for (; i0 + 7u * 1024u < m; i0 += 8u * 1024u) {
        int32_t r[8];
#pragma unroll
        for (uint32_t u = 0; u < 8u; ++u) r[u] = qr[i0 + u * 1024u];
#pragma unroll
        for (uint32_t u = 0; u < 8u; ++u) {
            lo = r[u] < lo ? r[u] : lo;
            hi = r[u] > hi ? r[u] : hi;
        }
    }
    for (uint32_t i = i0; i < m; i += 1024) {
        const int32_t r = qr[i];
        lo = r < lo ? r : lo;
        hi = r > hi ? r : hi;
    }
    for (int d = 1; d < 64; d <<= 1) {
        const int32_t ol = __shfl(lo, lane ^ d), oh = __shfl(hi, lane ^ d);
        lo = ol < lo ? ol : lo;
        hi = oh > hi ? oh : hi;
    }
    if (lane == 0) { s_lo[wave] = lo; s_hi[wave] = hi; }
    __syncthreads();
    if (wave != 0) return;
    for (uint32_t i = (uint32_t)lane; i < (uint32_t)(sizeof(LobbyDev) / 4); i += 64u) ((uint32_t*)&s_lb)[i] = ((const uint32_t*)&ch->lobby)[i];
    wave_sync();
    for (int w = 0; w < 16; ++w) {
        lo = s_lo[w] < lo ? s_lo[w] : lo;
        hi = s_hi[w] > hi ? s_hi[w] : hi;
    }
    // every seated player can become the anchor after a cancel: all of them go through the packed key
    for (uint32_t t = 0; t < M.teams; ++t)
        for (uint32_t k = 0; k < s_lb.cnt[t]; ++k) {
            const int32_t r = s_lb.rating[t][k];
            lo = r < lo ? r : lo;
            hi = r > hi ? r : hi;
        }
    bool fast = m >= TT_MIN && m <= TT_MAX && s_lb.n < M.L;
    if (m > 0 && ((long long)hi - (long long)lo) >= (1ll << PK_SPAN_BITS)) fast = false;
    for (uint32_t r = 0; r < M.n_roles; ++r)
        if (M.teams * M.quota[r] > 15u) fast = false;              // seats per role live in nibbles
    const uint32_t before = m + s_lb.n + (P.purge ? ch->purged : 0u);
    // Deferred effect of mm_cancel on the stored lobby (docs/MATCH_CHECK.md section 4, the order
    // of operations inside one attempt, search/worker.ex:295-321): an empty queue means no
    // attempt; a cancelled head filters the lobby before anybody is judged; a live head is judged
    // against the STALE lobby first, then remove_inactive_players filters it (that attempt never
    // emits).  The head then sits out the rest of the first pass: it was popped already.
    uint32_t sitout = 0, extra0 = 0, changed0 = 0, head_role = 0;
    if (fast && P.purge && ch->head_state != 0u) {
        if (ch->head_state == 1u && lobby_has_cancelled(s_lb, M, P.state)) {
            const uint32_t hc = P.q_cons[qo];
            head_role = (hc >> 16) & 7u;
            const int t = lobby_try_seat(s_lb, M, qr[0], hc, P.q_slot[qo], lane);
            lobby_filter(s_lb, M, P.state, P.released, P.n_released, lane);
            if (t >= 0) { extra0 = 1; changed0 = 1; }
            else sitout = 1;
        } else lobby_filter(s_lb, M, P.state, P.released, P.n_released, lane);
        wave_sync();
        for (uint32_t i = (uint32_t)lane; i < (uint32_t)(sizeof(LobbyDev) / 4); i += 64u) ((uint32_t*)&ch->lobby)[i] = ((const uint32_t*)&s_lb)[i];
    }
    if (lane == 0) {
        tc->fast = fast ? 1u : 0u;
        tc->done = 0;
        tc->m = m;
        tc->qlen = m - extra0;
        tc->rmin = m ? lo : 0;
        tc->passes = 0;
        tc->n_out = 0;
        tc->before = before;
        tc->err = 0;
        tc->pairs = 0;
        tc->scanned = 0;
        tc->n_vis = 0;
        tc->head = 0;
        tc->out_base = 0;
        tc->cur_pass = 0;
        tc->sitout = sitout;
        tc->extra0 = extra0;
        tc->changed0 = changed0;
        tc->head_role = head_role;
        tc->pub_go = 0; tc->pub_end = 0; tc->pub_pass = 0; tc->flags_late = 0;
        for (int k = 0; k < 8; ++k) tc->cp[k] = 0;
        for (int k = 0; k < 8; ++k) { tc->dbg[k] = 0; tc->tmk[k] = 0; }
        for (int k = 0; k < 16; ++k) tc->lt[k] = 0;
        tc->dbg[6] = sitout | (extra0 << 1) | ((fast && P.purge && ch->head_state != 0u) ? 4u : 0u);
    }
}

// kt_pack: grid (chunks, rating groups).  Packed keys, the bitmap, the chunk populations.
__global__ __launch_bounds__(TT_CH) void kt_pack(TeamParams P)
{
    __shared__ uint32_t s_c[MM_MAX_ROLES];
    const int tid = threadIdx.x, lane = tid & 63;
    const uint32_t g = blockIdx.y, cb = blockIdx.x;
    const TeamChain* const tc = P.tchains + g;
    if (!tc->fast) return;
    const uint32_t m = tc->m, nch = (m + TT_CH - 1u) / TT_CH;
    if (cb >= nch) return;
    const uint32_t nr = P.M.n_roles;
    const size_t qo = ((size_t)P.mode * P.n_groups + g) * P.capacity, po = (size_t)g * P.pstride;
    if (tid < (int)MM_MAX_ROLES) s_c[tid] = 0;
    __syncthreads();
    const uint32_t pos = cb * TT_CH + (uint32_t)tid;
    const bool inq = pos < m;
    const bool in = inq && !(pos == 0u && (tc->sitout | tc->extra0));   // the head after a cancel: kt_init
    uint32_t role = 0;
    if (inq) {
        const uint32_t cn = P.q_cons[qo + pos];
        role = (cn >> 16) & 7u;
        P.tkey[po + pos] = pk_pack(P.q_rating[qo + pos], cn, tc->rmin, P.eqmask);
        P.fv[po + pos] = 0u;                  // anything but TT_PART (kt_f keeps that one)
        P.fpos[po + pos] = TT_NONE;           // no lobby on record: the queue is new
        P.vis[po + pos] = TT_NONE;            // nothing published (the pair path's ticks use the array for something else)
    }
    // An emitter's dispatcher looks at vis[i] BEFORE it knows how many anchors the pass has published, for i up to a chain's
    // worker count beyond them (tc_emitter) — with a chain of a few hundred players (the test geometry: TT_MIN = 64) that is
    // beyond m, where a pair tick of another mode has left its REC words: found by tests/stress.py on the shim in round 5
    // (a wild anchor, a read far outside fv[]).  The product geometry (TT_MIN = 4096 > 32 x 15 workers) never gets there;
    // the words behind the queue are reset all the same.
    if (cb + 1u == nch)
        for (uint32_t q = m + (uint32_t)tid; q < m + TV_AHEAD && q < P.pstride; q += TT_CH) P.vis[po + q] = TT_NONE;
    if (tid < (int)TT_WORDS) {
        const uint32_t wi = cb * TT_WORDS + (uint32_t)tid, nwords = (m + 31u) >> 5;
        if (wi < nwords) {
            const uint32_t left = m - wi * 32u;
            uint32_t wbits = left >= 32u ? 0xFFFFFFFFu : ((1u << left) - 1u);
            if (wi == 0u && (tc->sitout | tc->extra0)) wbits &= ~1u;
            P.bits[1][(size_t)g * P.bits_stride + wi] = wbits;
        }
    }
    for (uint32_t r = 0; r < nr; ++r) {
        const unsigned long long mk = __ballot(in && role == r);
        if (lane == 0 && mk) atomicAdd(&s_c[r], (uint32_t)__popcll(mk));
    }
    __syncthreads();
    if (tid < (int)nr) P.chunk[((size_t)g * MM_MAX_ROLES + tid) * P.chunk_stride + cb] = s_c[tid];
}

// ------------------------------------------------------------------------------------
// kt_build: grid (chunks, rating groups).  The queue as the pass finds it, split by role.
// ------------------------------------------------------------------------------------
__global__ __launch_bounds__(TT_CH) void kt_build(TeamParams P)
{
    __shared__ uint32_t s_base[MM_MAX_ROLES], s_tot[MM_MAX_ROLES], s_wc[TT_WAVES][MM_MAX_ROLES];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const uint32_t g = blockIdx.y, cb = blockIdx.x;
    TeamChain* const tc = P.tchains + g;
    if (!tc->fast || tc->done) return;
    const uint32_t m = tc->m, nch = (m + TT_CH - 1u) / TT_CH;
    if (cb >= nch) return;
    const uint32_t nr = P.M.n_roles;
    const size_t qo = ((size_t)P.mode * P.n_groups + g) * P.capacity, po = (size_t)g * P.pstride;
    if (tid < (int)MM_MAX_ROLES) { s_base[tid] = 0; s_tot[tid] = 0; }
    __syncthreads();
    // players of every role queued before this chunk / in the whole chain
    const uint32_t* const chunk = P.chunk + (size_t)g * MM_MAX_ROLES * P.chunk_stride;
    {
        uint32_t pb[MM_MAX_ROLES], pt[MM_MAX_ROLES];
#pragma unroll
        for (uint32_t r = 0; r < MM_MAX_ROLES; ++r) pb[r] = pt[r] = 0;
        for (uint32_t k = tid; k < nch; k += TT_CH) {
            uint32_t v[MM_MAX_ROLES];
#pragma unroll
            for (uint32_t r = 0; r < MM_MAX_ROLES; ++r) v[r] = r < nr ? chunk[(size_t)r * P.chunk_stride + k] : 0u;   // all roles in flight
#pragma unroll
            for (uint32_t r = 0; r < MM_MAX_ROLES; ++r) {
                pt[r] += v[r];
                if (k < cb) pb[r] += v[r];
            }
        }
#pragma unroll
        for (uint32_t r = 0; r < MM_MAX_ROLES; ++r) {
            if (r < nr) {
                const uint32_t b = wave_sum(pb[r], lane), t = wave_sum(pt[r], lane);
                if (lane == 0 && t) { atomicAdd(&s_base[r], b); atomicAdd(&s_tot[r], t); }
            }
        }
    }
    __syncthreads();
    const uint32_t pos = cb * TT_CH + (uint32_t)tid;
    const uint32_t* const b1 = P.bits[1] + (size_t)g * P.bits_stride;
    uint32_t* const bB = P.bitsB + (size_t)g * P.bits_stride;
    if (tid < (int)TT_WORDS) {                        // who the sub-queues hold: the ranks of the passes to come count these
        const uint32_t wi = cb * TT_WORDS + (uint32_t)tid;
        if (wi < ((m + 31u) >> 5)) bB[wi] = b1[wi];
    }
    if ((uint32_t)tid < nr) {
        const size_t ci = ((size_t)g * MM_MAX_ROLES + (uint32_t)tid) * P.chunk_stride + cb;
        P.chunkB[ci] = P.chunk[ci];
    }
    const bool alive = pos < m && ((b1[pos >> 5] >> (pos & 31u)) & 1u);
    const uint32_t role = pos < m ? (P.q_cons[qo + pos] >> 16) & 7u : 0u;
    unsigned long long mymask = 0;
    uint32_t myc = 0;
    for (uint32_t r = 0; r < nr; ++r) {
        const unsigned long long mk = __ballot(alive && role == r);
        if (role == r) mymask = mk;                      // (of a player that has left as well: where its entry would stand)
        if ((uint32_t)lane == r) myc = (uint32_t)__popcll(mk);
    }
    if ((uint32_t)lane < nr) s_wc[wave][lane] = myc;
    __syncthreads();
    uint32_t bb = 0, off = 0;
    if ((uint32_t)lane < nr) {
        bb = s_base[lane];
        for (int w = 0; w < wave; ++w) bb += s_wc[w][lane];
        for (int r2 = 0; r2 < lane; ++r2) off += s_tot[r2];
        // (a role's row holds blk_stride = pstride / 64 blocks.  The last chunk's waves behind the stride — a pool whose
        // capacity is no multiple of TT_CH, nearly full with one chain — used to write their base into the NEXT role's first
        // blocks, racing with the chunk those belong to: tests/test_boundaries.py, chains of k x TT_CH + 1 players)
        if ((pos >> 6) < P.blk_stride) P.blkbase[po + (size_t)lane * P.blk_stride + (pos >> 6)] = bb;
    }
    const uint32_t mybb = (uint32_t)__shfl((int)bb, (int)role), myoff = (uint32_t)__shfl((int)off, (int)role);
    if (pos < m) {
        const uint32_t idx = myoff + mybb + (uint32_t)__popcll(mymask & ((1ull << lane) - 1ull));
        if (alive) {
            P.sqk[po + idx] = P.tkey[po + pos];
            P.sqp[po + idx] = pos;
        }
        // a player that has left the queue: the entry in front of where its own would stand (may wrap to -1: kt_f's
        // fix-up goes on at sqi + 1, behind the role's last member, whether that one is still queued or not)
        P.sqi[po + pos] = alive ? idx : idx - 1u;
    }
    if (cb == 0u && (uint32_t)tid < nr) { tc->len[tid] = s_tot[tid]; tc->off[tid] = off; }
}

// ------------------------------------------------------------------------------------
// kt_f: grid (chunks, rating groups), one thread per queue position.
//
// F[a] is decided by a's lobby: per role the first `need` queued players behind a that fit a.  Nobody
// joins a queue during a tick, so as long as every one of those players is still queued they stay the
// first ones that fit, whoever else left: the lobby — and with it the position of its last member — is
// the same as in the pass before, and only "who is queued behind the last member" has to be looked up
// again.  kt_f therefore keeps, per anchor, the lobby it found (memb: the members' positions as 16-bit
// distances from the anchor; fpos: the last one) and works in three steps:
//   A  every queued position: ranks in the role sub-queues (ballots), the supply test, and — if the
//      anchor has a lobby on record — one bitmap probe per member.  Anchors whose lobby lost a member
//      (or that have none on record: first pass, scan cap, 16-bit overflow) go on the chunk's work list;
//   B  the work list: the scans of the role sub-queues (windows staged in LDS), one lane per anchor AND
//      role; then one lane per anchor turns what they found into positions and writes the record;
//   C  every queued position: F = the first queued position behind the lobby's last member.
// After the first pass of a tick step B sees about one anchor in seven (profiles/README.md, round 2).
// Round 4: that is step B for anchors WITHOUT a record only.  An anchor whose recorded lobby lost members keeps
// the others and gets replacements (tf_chunk's head comment: where, why that is exact, and the measurements
// that led there — kt_f is bound by the instructions it issues, not by its trips to memory).
// ------------------------------------------------------------------------------------
#ifndef TF_SHORT
#define TF_SHORT 128u                 // kt_f, step B: keys a lane looks at alone before the scan goes to a whole wave
#endif
#ifndef TF_FAR_BITS
#define TF_FAR_BITS 16u               // kt_f: a member this many bits of positions away does not fit the record (the logic tests build with fewer)
#endif
#ifndef TF_BW
#define TF_BW TT_CH                   // kt_f: bitmap words staged in LDS from the chunk's first word on (a multiple of TT_CH: 16 384 positions ahead)
#endif
#ifndef TF_KW
#define TF_KW (TT_CH + 5u * TF_PAD)   // kt_f: words of LDS for the staged windows (TF_PAD a role with up to five roles, less with more)
#endif
#ifndef TF_TB
#define TF_TB 4u                      // kt_f: replacements of members that left — tasks a wave has in flight together
#endif
#define TF_REL_BITS 13u              // kt_f, step B: a member's sub-queue index relative to the staged window | role << 13
// LIVE: kt_chase's chasers run in the same launch (kt_fc): F goes through to memory and the chunk's flag
// (P.fdone = P.seq) follows it, so that a chaser on another XCD can take F as soon as the chunk is done
template <int LIVE>
static __device__ __forceinline__ void tf_chunk(const TeamParams& P, const uint32_t g, const uint32_t cb,
                                                uint16_t (&s_tmp)[MM_MAX_LOBBY - 1u][TT_CH])     // the members of the anchors at work, by the anchor's place
{
    // Round 4.  Measured first (MM_PAIR_DEBUG phase timers, profiles/r04_team_kt_f_*): with the dependent trips of a chunk cut
    // from seven to three the chunk took exactly as long as before — 31k cycles — because kt_f is bound by instruction issue,
    // not by latency: ~1 800 wave instructions per 64 positions and pass (windows of five sub-queues staged, five rank ballots,
    // the scans of the ~28 anchors per chunk that lost a member) on six waves a SIMD.  So the work is cut instead:
    // * an anchor whose lobby LOST members keeps the others and only replaces the lost ones (`fix`): the members of a role
    //   are the first that fit behind the anchor in the role's sub-queue, and everything up to the role's last member that is
    //   not a member was looked at and does not fit, or has left — so the replacements are the first entries that fit BEHIND
    //   that last member (lost or not).  Where that is in the sub-queue is sqi[its position] + 1 (kt_build leaves, for a
    //   position that has left the queue, the entry in front of which it would stand), a few keys from there are read, and the
    //   positions of the entries that fit.  One lane per anchor, wave 0 of the workgroup; no windows, no ranks.
    // * only an anchor WITHOUT a lobby on record (the first pass of a tick, a member 2^16 positions away) is looked up from
    //   scratch — the round-2 code below, which a workgroup enters only if it has such an anchor.
    // * the bitmap from the chunk's first position on is staged in LDS (TF_BW words, one per thread) with the first loads;
    //   member probes and step C read it there.
    __shared__ uint32_t s_k[TF_KW];                           // (full look-ups) the sub-queue windows of this chunk, role after role
    __shared__ uint32_t s_b[TF_BW];                           // the queue bitmap from the chunk's first word on
    __shared__ uint32_t s_j0[MM_MAX_ROLES], s_o[MM_MAX_ROLES + 1], s_len[MM_MAX_ROLES], s_off[MM_MAX_ROLES], s_seats[MM_MAX_ROLES];
    // (40 KB in all, so that four workgroups fit a CU: the arrays of the replacements share their place with arrays the
    // look-ups from scratch use — which a workgroup only starts when its replacements are done)
    __shared__ uint16_t s_jr[MM_MAX_ROLES][TT_CH];            // (full look-ups) rank of every position in every role's sub-queue, less s_j0
    uint16_t* const s_task = &s_jr[0][0];                     // the replacements, per role that lost somebody: place in the chunk | role << 9 | the anchor's role << 12
    __shared__ uint16_t s_item[TT_CH];                        // the anchors to look up from scratch: place in the chunk | role << 9
    __shared__ uint32_t s_long[TT_CH];                        // (full look-ups) the long scans: task | seats found << 12 | (where it stands - s_j0) << 16
    uint16_t* const s_fix = reinterpret_cast<uint16_t*>(s_long);            // the anchors that lost members: place in the chunk
    uint16_t* const s_lost = reinterpret_cast<uint16_t*>(s_long) + TT_CH;   // ... and which of the record's slots
    __shared__ uint32_t s_key[TT_CH];                         // packed keys of the chunk
    __shared__ uint32_t s_res[TT_CH];                         // step B: flags of the scans, then -> C: last member's position, TT_PART, TT_UNK
    __shared__ uint16_t s_rm[MM_MAX_ROLES][MM_MAX_ROLES];     // [the anchor's role][role]: the role's slots in the anchor's record
    __shared__ uint32_t s_n, s_nl, s_nfix, s_ntask;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    if (!((P.act >> g) & 1u)) return;                         // the chain was done at the host's last look: not a single load
    TeamChain* const tc = P.tchains + g;
    const uint32_t nr = P.M.n_roles, LM = P.M.L - 1u;
    const size_t qo = ((size_t)P.mode * P.n_groups + g) * P.capacity, po = (size_t)g * P.pstride;
    const uint32_t pos = cb * TT_CH + (uint32_t)tid;
    const uint32_t pc = pos < P.capacity ? pos : P.capacity - 1u;      // (the loads go out before the chain's length is known)
    // the queue as this pass finds it: nobody leaves it while kt_f runs, so kt_f reads the current bitmap — and
    // copies its chunk's words into the snapshot kt_f2 / kt_chase / kt_emit read while they take players out
    const uint32_t* const b0 = P.bits[1] + (size_t)g * P.bits_stride;
    const uint32_t wb0 = cb * TT_WORDS;                       // the chunk's first bitmap word
    // ---- everything whose address depends on no other load goes out together: the chain's record, the position's own
    //      words, its lobby on record, the bitmap ahead ----
    const uint32_t c_fast = tc->fast, c_done = tc->done, m = tc->m;
    const uint32_t bwB_raw = P.bitsB[(size_t)g * P.bits_stride + (pc >> 5)];
    const uint32_t cn_raw = P.q_cons[qo + pc];
    const uint32_t prevF_raw = P.fv[po + pc];
    const uint32_t fp_raw = P.fpos[po + pc];
    const uint32_t mykey_raw = P.tkey[po + pc];
    uint32_t d[MM_MAX_LOBBY - 1u];
    {
        const uint16_t* const mb = P.memb + (po + pc) * LM;
#pragma unroll
        for (uint32_t k = 0; k < MM_MAX_LOBBY - 1u; ++k) d[k] = k < LM ? mb[k] : 0u;
    }
    uint32_t bv[TF_BW / TT_CH];
#pragma unroll
    for (uint32_t u = 0; u < TF_BW / TT_CH; ++u) {
        const uint32_t wi = wb0 + u * TT_CH + (uint32_t)tid;
        bv[u] = b0[wi < P.bits_stride ? wi : 0u];
    }
    uint32_t rlen = 0, roff = 0;
    if ((uint32_t)tid < nr) { rlen = tc->len[tid]; roff = tc->off[tid]; }
    const uint32_t nch = (m + TT_CH - 1u) / TT_CH, nwords = (m + 31u) >> 5;
    if (LIVE) {
        // the chain's chaser runs beside this workgroup and sets `done` when its pass ends the chain (a last pass that
        // seats nobody is over in a few microseconds — while kt_f's workgroups are still being dispatched): ONE thread
        // looks, so that the workgroup stays or leaves as a whole (a wave that left would take the set-up of the
        // others' LDS tables with it)
        __shared__ uint32_t s_stay;
        if (tid == 0) s_stay = (c_fast && !c_done && cb < nch) ? 1u : 0u;
        __syncthreads();
        if (!s_stay) return;
    } else if (!c_fast || c_done || cb >= nch) return;
#pragma unroll
    for (uint32_t u = 0; u < TF_BW / TT_CH; ++u) {
        const uint32_t wi = wb0 + u * TT_CH + (uint32_t)tid;
        if (wi >= nwords) bv[u] = 0u;                         // (beyond the chain the words are somebody else's)
        s_b[u * TT_CH + (uint32_t)tid] = bv[u];
    }
    if (tid < (int)TT_WORDS && wb0 + (uint32_t)tid < nwords) P.bits[0][(size_t)g * P.bits_stride + wb0 + (uint32_t)tid] = bv[0];
    const bool inq = pos < m;
    const uint32_t bwB = inq ? bwB_raw : 0u, cn = inq ? cn_raw : 0u, prevF = inq ? prevF_raw : 0u;
    const uint32_t fp = inq ? fp_raw : TT_NONE, mykey = inq ? mykey_raw : 0u;
    const unsigned long long le = (2ull << lane) - 1ull;
    const bool tmr = P.debug && g == 0u && cb == (nch >> 1) && tid == 0;   // a workgroup in the middle of the longest chain
    long long tq = tmr ? clock64() : 0;
#define TFMARK(K) do { if (tmr) { const long long now = clock64(); atomicAdd(&tc->tmk[K], (uint32_t)(now - tq)); tq = now; } } while (0)
    if ((uint32_t)tid < nr) {
        s_len[tid] = rlen;
        s_off[tid] = roff;
        s_seats[tid] = P.M.teams * P.M.quota[tid];
    }
    if (tid == 0) { s_n = 0; s_nl = 0; s_nfix = 0; s_ntask = 0; }
    if ((uint32_t)tid < nr * nr) {                            // (the record keeps the members role after role)
        const uint32_t ar = (uint32_t)tid / nr, r = (uint32_t)tid % nr;
        uint32_t ns = 0;
        for (uint32_t q = 0; q < r; ++q) ns += P.M.teams * P.M.quota[q] - (ar == q ? 1u : 0u);
        s_rm[ar][r] = (uint16_t)(((1u << (P.M.teams * P.M.quota[r] - (ar == r ? 1u : 0u))) - 1u) << ns);
    }
    s_res[tid] = 0;
    s_key[tid] = mykey;
    __syncthreads();
    TFMARK(0);
    // ---- step A: who is queued, whose lobby still stands ----
    const bool alive = inq && ((s_b[(uint32_t)tid >> 5] >> (pos & 31u)) & 1u);
    const bool inB = inq && ((bwB >> (pos & 31u)) & 1u);     // has an entry in the sub-queues (it may have left the queue since)
    const uint32_t role = inB ? (cn >> 16) & 7u : 0u;
    // a lobby that could not fill in an earlier pass of this tick cannot fill now: nobody joins
    // the queue during a tick, so the supply behind an anchor only shrinks.  One that ran into the
    // scan cap is not looked up again either: to kt_chase both say "look yourself", which is always
    // right, and the long scans that end at the cap are the most expensive ones
    const bool stuck = alive && (prevF == TT_PART || prevF == TT_UNK);
    bool part = stuck;
    uint32_t fpos = TT_NONE;                                  // the lobby's last member, once known
    bool todo = alive && !stuck, fix = false;
    if (todo && fp != TT_NONE) {                              // a lobby on record: are all its members still queued?
        uint32_t lost = 0;
        if (fp - cb * TT_CH < 32u * TF_BW) {                  // its last member — so all of them — within the staged bitmap
#pragma unroll
            for (uint32_t k = 0; k < MM_MAX_LOBBY - 1u; ++k) {
                if (k < LM) {
                    const uint32_t rel = (uint32_t)tid + d[k];
                    lost |= ((~s_b[rel >> 5] >> (rel & 31u)) & 1u) << k;
                }
            }
        } else {
#pragma unroll
            for (uint32_t k = 0; k < MM_MAX_LOBBY - 1u; ++k) {
                if (k < LM) {
                    const uint32_t mp = pos + d[k];
                    lost |= ((~b0[mp >> 5] >> (mp & 31u)) & 1u) << k;
                }
            }
        }
        todo = false;
        if (!lost) fpos = fp;
        else {
            fix = true;
            s_lost[tid] = (uint16_t)lost;
#pragma unroll
            for (uint32_t k = 0; k < MM_MAX_LOBBY - 1u; ++k) if (k < LM) s_tmp[k][tid] = (uint16_t)d[k];
            for (uint32_t r = 0; r < nr; ++r)                 // a task per role that lost somebody
                if (lost & s_rm[role][r]) s_task[atomicAdd(&s_ntask, 1u)] = (uint16_t)((uint32_t)tid | (r << 9) | (role << 12));
        }
    }
    {   // the two work lists
        const unsigned long long tm = __ballot(todo), fm = __ballot(fix);
        uint32_t wb = 0, fb = 0;
        if (lane == 0 && tm) wb = atomicAdd(&s_n, (uint32_t)__popcll(tm));
        if (lane == 0 && fm) fb = atomicAdd(&s_nfix, (uint32_t)__popcll(fm));
        wb = (uint32_t)__shfl((int)wb, 0);
        fb = (uint32_t)__shfl((int)fb, 0);
        if (todo) s_item[wb + (uint32_t)__popcll(tm & (le >> 1))] = (uint16_t)((uint32_t)tid | (role << 9));
        if (fix) s_fix[fb + (uint32_t)__popcll(fm & (le >> 1))] = (uint16_t)((uint32_t)tid | (role << 9));
    }
    __syncthreads();
    // A chunk with MANY lobbies to mend (the first passes of a tick: one anchor in eight) is better off with the windows of
    // its sub-queues staged once for all of them: they go on the from-scratch list
    const bool mend = s_ntask <= P.fix_max;
    if (!mend) {
        for (uint32_t i = (uint32_t)tid, nf = s_nfix, n0 = s_n; i < nf; i += TT_CH) s_item[n0 + i] = s_fix[i];
        __syncthreads();
        if (tid == 0) { s_n += s_nfix; s_nfix = 0; s_ntask = 0; }
        __syncthreads();
        if (fix) { todo = true; fix = false; }
    }
    TFMARK(1);
    const uint32_t n_items = s_n, n_fix = s_nfix;
    if (tmr) atomicAdd(&tc->dbg[2], n_items + n_fix);
    // ---- the lobbies that lost members.  A task = (anchor, role that lost somebody).  The waves share the tasks; a wave
    //      sets up to TF_TB of them up lane by lane (where the role's last member stands in the sub-queue: one trip for all
    //      of them), then reads 64 entries — keys and positions — behind each of those places (a second trip for all of
    //      them) and the first that fit take the slots of those who left.  (One lane per task, sixteen entries a trip, was
    //      measured first: with one entry in fifteen fitting, the slowest of a chunk's ~35 tasks needed five trips.) ----
    {
        const uint32_t n_task = s_ntask, per = (n_task + TT_WAVES - 1u) / TT_WAVES;
        const uint32_t t_lo = (uint32_t)wave * per, t_hi = t_lo + per < n_task ? t_lo + per : n_task;
        const uint32_t* const sk = P.sqk + po;
        const uint32_t* const sp = P.sqp + po;
        for (uint32_t ts = t_lo; ts < t_hi; ts += 64u) {
            // set-up, a lane per task: one trip for all of the wave's tasks
            uint32_t v_at = 0, v_lr = 0, v_j = 0, v_end = 0, v_lo = 0, v_rng = 0;
            if (ts + (uint32_t)lane < t_hi) {
                const uint32_t tk = s_task[ts + (uint32_t)lane], at = tk & (TT_CH - 1u), r = (tk >> 9) & 7u, arole = tk >> 12;
                const uint32_t lw = s_lost[at];
                pk_bounds(s_key[at], P.window, v_lo, v_rng);
                const uint32_t rm = s_rm[arole][r];
                v_lr = lw & rm;                               // the role's slots that are empty now
                uint32_t lastd = 0;                           // the role's last member so far, lost or not
                for (uint32_t mk = rm; mk; mk &= mk - 1u) { const uint32_t dk = s_tmp[(uint32_t)__ffs((int)mk) - 1u][at]; lastd = dk > lastd ? dk : lastd; }
                v_end = s_off[r] + s_len[r];
                v_at = at;
                v_j = P.sqi[po + cb * TT_CH + at + lastd] + 1u;
            }
            // Several tasks a step, four entries a lane (one aligned 16-byte piece of the keys, one of the positions).  How many
            // lanes a task gets depends on how many tasks the wave has: sixteen (64 entries behind the role's last member: a
            // replacement is nearly always among them, and a chunk with a few tasks is waited for) down to four (sixteen
            // entries, sixteen tasks a step: the first passes of a tick, when a wave has a dozen tasks and the launch is bound
            // by the instructions it issues and the lines it reads, not by a trip more for the task that finds nothing)
            const uint32_t t_end = t_hi - ts < 64u ? t_hi - ts : 64u;
            const uint32_t gl = t_end <= P.fix_t8 ? 16u : t_end <= P.fix_t4 ? 8u : 4u, per_step = 64u / gl;
            const uint32_t q = (uint32_t)lane / gl, sl = (uint32_t)lane % gl, gsh = q * gl, gmask = gl == 16u ? 0xFFFFu : (1u << gl) - 1u;
            for (uint32_t tb = 0; tb < t_end; tb += per_step) {
                const int src = (int)((tb + q) & 63u);
                const bool have = tb + q < t_end;
                const uint32_t at = (uint32_t)__shfl((int)v_at, src), e2 = (uint32_t)__shfl((int)v_end, src);
                const uint32_t lo = (uint32_t)__shfl((int)v_lo, src), rng = (uint32_t)__shfl((int)v_rng, src);
                uint32_t lr = (uint32_t)__shfl((int)v_lr, src), j = (uint32_t)__shfl((int)v_j, src);
                if (!have) lr = 0;
                const uint32_t apos = cb * TT_CH + at;
                uint16_t* const mb = P.memb + (po + apos) * LM;
                uint32_t budget = P.scan_cap, fl = 0;
                bool on = lr != 0u;                           // (the same in the sixteen lanes of a task)
                if (on && j >= e2) { fl = 1u; on = false; }
                while (__ballot(on)) {
                    const uint32_t js = (j & ~3u) + 4u * sl;
                    uint4 k4 = make_uint4(0xFFFFFFFFu, 0xFFFFFFFFu, 0xFFFFFFFFu, 0xFFFFFFFFu), p4 = make_uint4(0u, 0u, 0u, 0u);
                    if (on && js < e2) {
                        k4 = *reinterpret_cast<const uint4*>(sk + js);
                        p4 = *reinterpret_cast<const uint4*>(sp + js);
                    }
                    uint32_t h = 0;                           // which of my four entries fit (a key of a player that left fits no interval)
                    h |= (js >= j && js < e2 && pk_in(k4.x, lo, rng)) ? 1u : 0u;
                    h |= (js + 1u >= j && js + 1u < e2 && pk_in(k4.y, lo, rng)) ? 2u : 0u;
                    h |= (js + 2u >= j && js + 2u < e2 && pk_in(k4.z, lo, rng)) ? 4u : 0u;
                    h |= (js + 3u >= j && js + 3u < e2 && pk_in(k4.w, lo, rng)) ? 8u : 0u;
                    if (!on) h = 0;
                    uint32_t rank = 0, total = 0;             // entries of the task that fit: in front of mine, in all
#pragma unroll
                    for (uint32_t e = 0; e < 4u; ++e) {
                        const unsigned long long be = __ballot((h >> e) & 1u);
                        const uint32_t gm = (uint32_t)(be >> gsh) & gmask;
                        rank += (uint32_t)__popc(gm & ((1u << sl) - 1u));
                        total += (uint32_t)__popc(gm);
                    }
                    for (uint32_t hh = h; hh; hh &= hh - 1u, ++rank) {
                        uint32_t mine = lr;                   // the rank-th of the empty slots
                        for (uint32_t x = 0; x < rank && mine; ++x) mine &= mine - 1u;
                        if (!mine) break;
                        const uint32_t e = (uint32_t)__ffs((int)hh) - 1u, k = (uint32_t)__ffs((int)mine) - 1u;
                        const uint32_t pv = e == 0u ? p4.x : e == 1u ? p4.y : e == 2u ? p4.z : p4.w, dk = pv - apos;
                        s_tmp[k][at] = (uint16_t)dk;
                        if (dk >> TF_FAR_BITS) atomicOr(&s_res[at], 2u);   // does not fit the record: "look yourself", and from scratch in the next pass
                        if (LIVE) __hip_atomic_store(&mb[k], (uint16_t)dk, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);   // (an emitter of this launch may read it)
                        else mb[k] = (uint16_t)dk;
                    }
                    for (uint32_t x = total; x && lr; --x) lr &= lr - 1u;
                    if (on) {
                        if (!lr) on = false;
                        else {
                            j = (j & ~3u) + 4u * gl;
                            budget = budget > 4u * gl ? budget - 4u * gl : 0u;
                            if (j >= e2) { fl = 1u; on = false; }          // the role cannot fill any more
                            else if (!budget) { fl = 2u; on = false; }    // the scan cap
                        }
                    }
                }
                if (fl && sl == 0u) atomicOr(&s_res[at], fl);
            }
        }
    }
    __syncthreads();
    if ((uint32_t)tid < n_fix) {                              // the anchor's record: its last member
        const uint32_t at = s_fix[tid] & (TT_CH - 1u), apos = cb * TT_CH + at, fl = s_res[at];
        uint32_t res = (fl & 1u) ? TT_PART : TT_UNK, rec = TT_NONE;
        if (!fl) {
            uint32_t lastd = 0;
            for (uint32_t k = 0; k < LM; ++k) { const uint32_t dk = s_tmp[k][at]; lastd = dk > lastd ? dk : lastd; }
            res = rec = apos + lastd;
        }
        if (LIVE) pub_st(&P.fpos[po + apos], rec);
        else P.fpos[po + apos] = rec;
        s_res[at] = res;
    }
    TFMARK(2);
    if (n_items) {
    // ---- the anchors without a lobby on record, from scratch (a uniform branch: the whole workgroup or nobody).
    //      What the scans read: per role, the sub-queue from the first entry behind the chunk's first position, as
    //      long as the chunk's own players of the role plus TF_PAD (where a scan that succeeds normally ends);
    //      longer scans go on in HBM ----
    // (the last chunk's waves behind the stride — pos >> 6 >= blk_stride, so pos >= pstride >= capacity >= m — read a word of
    // the next role's row here: inside the group's pstride words, and unused, these positions hold nobody; kt_build writes none)
    const uint32_t bbv = (uint32_t)lane < nr ? P.blkbase[po + (size_t)lane * P.blk_stride + (pos >> 6)] : 0u;
    if (tid < 64) {                                           // one lane per role: every load of the set-up in flight at once
        const bool on = (uint32_t)lane < nr;
        const uint32_t rj0 = on ? P.blkbase[po + (size_t)lane * P.blk_stride + cb * (TT_CH / 64u)] : 0u;
        const uint32_t pad = (TF_KW - TT_CH) / nr < TF_PAD ? (TF_KW - TT_CH) / nr : TF_PAD;
        const uint32_t rw = on ? P.chunkB[((size_t)g * MM_MAX_ROLES + (uint32_t)lane) * P.chunk_stride + cb] + pad : 0u;
        uint32_t o = rw;                                      // inclusive prefix of the window lengths over the roles
        for (int dd = 1; dd < (int)MM_MAX_ROLES; dd <<= 1) {
            const uint32_t t = (uint32_t)__shfl((int)o, lane >= dd ? lane - dd : 0);
            if (lane >= dd) o += t;
        }
        if (on) {
            s_j0[lane] = rj0;
            s_o[lane] = o - rw;
            if ((uint32_t)lane == nr - 1u) s_o[nr] = o;
        }
    }
    __syncthreads();
    {   // every role's window: all loads first, then the stores (a window is rarely longer than the workgroup)
        uint32_t sv[MM_MAX_ROLES];
#pragma unroll
        for (uint32_t r = 0; r < MM_MAX_ROLES; ++r) {
            sv[r] = 0;
            if (r < nr) {
                const uint32_t j0 = s_j0[r], w = s_o[r + 1u] - s_o[r];
                if ((uint32_t)tid < w && j0 + (uint32_t)tid < s_len[r]) sv[r] = P.sqk[po + s_off[r] + j0 + (uint32_t)tid];
            }
        }
#pragma unroll
        for (uint32_t r = 0; r < MM_MAX_ROLES; ++r) {
            if (r < nr) {
                const uint32_t j0 = s_j0[r], o = s_o[r], w = s_o[r + 1u] - o;
                if ((uint32_t)tid < w && j0 + (uint32_t)tid < s_len[r]) s_k[o + (uint32_t)tid] = sv[r];
            }
        }
        for (uint32_t r = 0; r < nr; ++r) {
            const uint32_t j0 = s_j0[r], o = s_o[r], w = s_o[r + 1u] - o, end = s_len[r];
            const uint32_t* const sk = P.sqk + po + s_off[r];
            for (uint32_t i = (uint32_t)tid + TT_CH; i < w && j0 + i < end; i += TT_CH) s_k[o + i] = sk[j0 + i];
        }
    }
    // the ballots need every lane; the cheapest test of all: a role whose sub-queue has fewer
    // entries behind me than I need seats ends the question
#pragma unroll
    for (uint32_t r = 0; r < MM_MAX_ROLES; ++r) {
        if (r < nr) {
            const unsigned long long mk = __ballot(inB && role == r);
            const uint32_t base = (uint32_t)__shfl((int)bbv, (int)r);
            const uint32_t jr = base + (uint32_t)__popcll(mk & le);       // sub-queue entries of the role up to and including mine
            s_jr[r][tid] = (uint16_t)(jr - s_j0[r]);
            const uint32_t need = s_seats[r] - (role == r ? 1u : 0u);
            if (todo && s_len[r] - jr < need) part = true;
        }
    }
    if (part && todo) s_res[tid] = 1u;                        // (its scans find the same; kept out of the lobbies below)
    __syncthreads();
    // ---- the scans: one lane per (anchor of the work list, role) — the roles of a lobby are
    //      independent of each other, and a wave runs as long as its slowest lane.  A lane looks at the
    //      first TF_SHORT keys of its stretch; the few scans that need more go on a second list ----
    const uint32_t n_tasks = n_items * nr;
    for (uint32_t t = (uint32_t)tid; t < n_tasks; t += TT_CH) {
        const uint32_t it = s_item[t / nr], r = t % nr, at = it & (TT_CH - 1u), arole = it >> 9;
        const uint32_t need = s_seats[r] - (arole == r ? 1u : 0u);
        if (!need || (s_res[at] & 1u)) continue;
        uint32_t ns = 0;                                      // the role's first slot in the lobby
        for (uint32_t q = 0; q < r; ++q) ns += s_seats[q] - (arole == q ? 1u : 0u);
        uint32_t lo, rng;
        pk_bounds(s_key[at], P.window, lo, rng);
        const uint32_t end = s_len[r];
        const uint32_t j0 = s_j0[r], tag = (r << TF_REL_BITS) - j0;          // s_tmp entry of sub-queue index j: j + tag
        uint32_t j = j0 + s_jr[r][at];
        const uint32_t cap_end = end - j > P.scan_cap ? j + P.scan_cap : end;
        uint32_t cnt = 0;
        {   // the staged window: eight keys a step, the (few) that fit are noted as they come
            const uint32_t w = s_o[r + 1u] - s_o[r];
            uint32_t lim = j0 + w < cap_end ? j0 + w : cap_end;
            lim = lim - j > TF_SHORT ? j + TF_SHORT : lim;
            const uint32_t* const lk = s_k + s_o[r] - j0;                 // lk[j] for j0 <= j < j0 + w
            while (cnt < need && j + 8u <= lim) {
                uint32_t m8 = 0;
#pragma unroll
                for (uint32_t u = 0; u < 8u; ++u) m8 |= pk_in(lk[j + u], lo, rng) ? (1u << u) : 0u;
                while (m8 && cnt < need) {
                    s_tmp[ns + cnt][at] = (uint16_t)(j + (uint32_t)__ffs((int)m8) - 1u + tag);
                    m8 &= m8 - 1u;
                    ++cnt;
                }
                j += 8u;
            }
            while (cnt < need && j < lim) {
                if (pk_in(lk[j], lo, rng)) { s_tmp[ns + cnt][at] = (uint16_t)(j + tag); ++cnt; }
                ++j;
            }
        }
        if (cnt < need && j < cap_end) {                      // not there yet: the waves finish it together
            const uint32_t li = atomicAdd(&s_nl, 1u);
            if (li < TT_CH) { s_long[li] = t | (cnt << 12) | ((j - j0) << 16); continue; }
            // the list is full (a first pass with many long scans): on alone, window first, then HBM
            const uint32_t* const sk = P.sqk + po + s_off[r];
            const uint32_t w = s_o[r + 1u] - s_o[r], lds_end = j0 + w < cap_end ? j0 + w : cap_end;
            const uint32_t* const lk = s_k + s_o[r] - j0;
            while (cnt < need && j < lds_end) {
                if (pk_in(lk[j], lo, rng)) { s_tmp[ns + cnt][at] = (uint16_t)(j + tag); ++cnt; }
                ++j;
            }
            while (cnt < need && j < cap_end) {
                if (pk_in(sk[j], lo, rng)) { s_tmp[ns + cnt][at] = (uint16_t)(j + tag); ++cnt; }
                ++j;
            }
        }
        if (cnt < need) atomicOr(&s_res[at], j < end ? 2u : 1u);          // scan cap reached / the role cannot fill
    }
    __syncthreads();
    // the long scans: a wave each, 64 keys a step and four steps in flight — out of the staged window as far as it goes
    for (uint32_t li = (uint32_t)wave, nl = s_nl < TT_CH ? s_nl : TT_CH; li < nl; li += TT_WAVES) {
        const uint32_t lw = s_long[li], t = lw & 0xFFFu;
        const uint32_t it = s_item[t / nr], r = t % nr, at = it & (TT_CH - 1u), arole = it >> 9;
        const uint32_t need = s_seats[r] - (arole == r ? 1u : 0u);
        uint32_t ns = 0;
        for (uint32_t q = 0; q < r; ++q) ns += s_seats[q] - (arole == q ? 1u : 0u);
        uint32_t lo, rng;
        pk_bounds(s_key[at], P.window, lo, rng);
        const uint32_t end = s_len[r];
        const uint32_t* const sk = P.sqk + po + s_off[r];
        const uint32_t j0 = s_j0[r], tag = (r << TF_REL_BITS) - j0, js = j0 + s_jr[r][at];
        const uint32_t cap_end = end - js > P.scan_cap ? js + P.scan_cap : end;
        const uint32_t wend = j0 + (s_o[r + 1u] - s_o[r]) < end ? j0 + (s_o[r + 1u] - s_o[r]) : end;    // the staged window ends here
        const uint32_t* const lk = s_k + s_o[r] - j0;
        uint32_t j = j0 + (lw >> 16), cnt = (lw >> 12) & 15u;
        while (cnt < need && j < cap_end) {
            uint32_t k[4];
#pragma unroll
            for (uint32_t u = 0; u < 4u; ++u) {
                const uint32_t c = j + u * 64u + (uint32_t)lane;
                k[u] = c < cap_end ? (c < wend ? lk[c] : sk[c]) : 0u;
            }
#pragma unroll
            for (uint32_t u = 0; u < 4u; ++u) {
                const uint32_t c = j + u * 64u + (uint32_t)lane;
                const bool ok = c < cap_end && pk_in(k[u], lo, rng);
                const unsigned long long bal = __ballot(ok);
                const uint32_t rank = cnt + (uint32_t)__popcll(bal & (le >> 1));
                if (ok && rank < need) s_tmp[ns + rank][at] = (uint16_t)(c + tag);
                cnt += (uint32_t)__popcll(bal);
            }
            j += 256u;
        }
        if (cnt < need && lane == 0) atomicOr(&s_res[at], cap_end < end ? 2u : 1u);
    }
    __syncthreads();
    // ---- the lobbies: sub-queue indices -> queue positions, all loads in flight together;
    //      the record for the passes to come ----
    if ((uint32_t)tid < n_items) {
        const uint32_t at = s_item[tid] & (TT_CH - 1u), apos = cb * TT_CH + at, fl = s_res[at];
        uint32_t res = (fl & 1u) ? TT_PART : TT_UNK, rec = TT_NONE;
        if (!fl) {
            uint32_t mp[MM_MAX_LOBBY - 1u];
#pragma unroll
            for (uint32_t k = 0; k < MM_MAX_LOBBY - 1u; ++k) {
                mp[k] = apos;
                if (k < LM) {
                    const uint32_t t = s_tmp[k][at], r = t >> TF_REL_BITS;
                    mp[k] = P.sqp[po + s_off[r] + s_j0[r] + (t & ((1u << TF_REL_BITS) - 1u))];
                }
            }
            uint16_t* const mb = P.memb + (po + apos) * LM;
            uint32_t last = apos, far = 0;
#pragma unroll
            for (uint32_t k = 0; k < MM_MAX_LOBBY - 1u; ++k) {
                if (k < LM) {
                    const uint32_t dk = mp[k] - apos;
                    if (LIVE) __hip_atomic_store(&mb[k], (uint16_t)dk, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);   // (an emitter of this launch may read it)
                    else mb[k] = (uint16_t)dk;
                    far |= dk >> TF_FAR_BITS;
                    last = mp[k] > last ? mp[k] : last;
                }
            }
            res = last;
            if (!far) rec = last;                             // a member 2^16 positions away: no record, looked up again every pass
        }
        if (LIVE) pub_st(&P.fpos[po + apos], rec);
        else P.fpos[po + apos] = rec;
        s_res[at] = res;
    }
    TFMARK(3);
    }
    __syncthreads();
    TFMARK(4);
    // ---- step C ----
    if (alive) {
        uint32_t F = TT_NONE;
        if (stuck) F = prevF;
        else {
            if (todo || fix) fpos = s_res[tid];
            if (fpos >= TT_UNK) F = fpos;                          // TT_PART / TT_UNK from step B
            else {
                const uint32_t q = fpos + 1u;
                uint32_t wi = q >> 5;
                if (wi < nwords) {
                    uint32_t v = (wi - wb0 < TF_BW ? s_b[wi - wb0] : b0[wi]) & (0xFFFFFFFFu << (q & 31u));
                    while (v == 0u && ++wi < nwords) v = wi - wb0 < TF_BW ? s_b[wi - wb0] : b0[wi];
                    if (v) F = (wi << 5) + (uint32_t)__ffs((int)v) - 1u;
                }
            }
        }
        if (LIVE) pub_st(&P.fv[po + pos], F);
        else P.fv[po + pos] = F;
        if (P.debug & 2u) {   // MM_PAIR_DEBUG with MM_TEAM_BATCH=1: how many F values a pass really changes
            atomicAdd(&tc->dbg[5], 1u);
            if (tc->passes != 0u && prevF != F) atomicAdd(&tc->dbg[4], 1u);
        }
    }
    TFMARK(5);
    if (LIVE) {
        // every F of the chunk has arrived in memory: the chunk's flag
        tw_store_wait();
        __syncthreads();
        if (tid == 0) pub_st(&P.fdone[(size_t)g * P.chunk_stride + cb], P.seq);
    }
#undef TFMARK
}

// ------------------------------------------------------------------------------------
// kt_f2: F composed with itself, one thread per queue position.  The chase of kt_chase is a chain of
// dependent loads, one per emitted lobby (~0.18 us each); with F2 = F o F next to F it takes two lobbies
// per round trip (both words of an anchor are loaded together).  Worth its launch only while a pass emits
// hundreds of lobbies: the host runs it in the first passes of a tick only.
// F2[a] = F[F[a]] when a's lobby fills and hands over to a queued player; TT_UNK otherwise ("step singly").
// ------------------------------------------------------------------------------------
__global__ __launch_bounds__(TT_CH) void kt_f2(TeamParams P)
{
    const uint32_t g = blockIdx.y, cb = blockIdx.x;
    const TeamChain* const tc = P.tchains + g;
    if (!tc->fast || tc->done) return;
    const uint32_t m = tc->m;
    const uint32_t pos = cb * TT_CH + threadIdx.x;
    if (pos >= m) return;
    const size_t po = (size_t)g * P.pstride;
    const uint32_t* const b0 = P.bits[0] + (size_t)g * P.bits_stride;
    if (!((b0[pos >> 5] >> (pos & 31u)) & 1u)) return;
    const uint32_t f = P.fv[po + pos];
    P.fv2[po + pos] = f < TT_UNK ? P.fv[po + f] : TT_UNK;
}

// ------------------------------------------------------------------------------------
// wave-wide helpers of kt_chase / kt_emit
// ------------------------------------------------------------------------------------

// first queued position >= from (bitmap of the start of the pass), or TT_NONE
static __device__ __forceinline__ uint32_t tw_succ(const uint32_t* b0, uint32_t from, uint32_t m, int lane)
{
    if (from >= m) return TT_NONE;
    const uint32_t nwords = (m + 31u) >> 5, w0 = from >> 5;
    for (uint32_t wb = w0; wb < nwords; wb += 64u) {
        const uint32_t wi = wb + (uint32_t)lane;
        uint32_t v = wi < nwords ? b0[wi] : 0u;
        if (wi == w0) v &= 0xFFFFFFFFu << (from & 31u);
        const unsigned long long b = __ballot(v != 0u);
        if (b) {
            const int l = __ffsll(b) - 1;
            const uint32_t vv = (uint32_t)__shfl((int)v, l);
            return ((wb + (uint32_t)l) << 5) + (uint32_t)__ffs((int)vv) - 1u;
        }
    }
    return TT_NONE;
}

// the first `need` entries of the sub-queue [j0, len) that fit (lo, rng): their positions are
// appended to out[nout..]; returns how many there were (<= need).
static __device__ __forceinline__ uint32_t tw_collect(const uint32_t* sk, const uint32_t* sp, uint32_t j0, uint32_t len, uint32_t need,
                                      uint32_t lo, uint32_t rng, uint32_t* out, uint32_t nout, int lane, uint32_t* trips = nullptr)
{
    uint32_t got = 0;
    for (uint32_t p = j0; p < len && got < need; p += 64u) {
        if (trips) *trips += 1u;
        const uint32_t j = p + (uint32_t)lane;
        const bool ok = j < len && pk_in(sk[j], lo, rng);
        const unsigned long long b = __ballot(ok);
        const uint32_t nb = (uint32_t)__popcll(b), room = need - got;
        const uint32_t rk = (uint32_t)__popcll(b & ((1ull << lane) - 1ull));
        if (ok && rk < room) out[nout + got + rk] = sp[j];
        got += nb < room ? nb : room;
    }
    return got;
}

// per role (returned in lane r): sub-queue entries of the role at positions <= a
static __device__ __forceinline__ uint32_t tw_starts(const TeamParams& P, uint32_t g, uint32_t a, uint32_t m, int lane)
{
    const size_t qo = ((size_t)P.mode * P.n_groups + g) * P.capacity, po = (size_t)g * P.pstride;
    const uint32_t* const b0 = P.bitsB + (size_t)g * P.bits_stride;       // the sub-queues' entries, not the queue's players
    const uint32_t b = a >> 6, pos = (b << 6) + (uint32_t)lane, pc = pos < m ? pos : m - 1u;
    // (three loads that do not wait for each other: a look-up begins with ONE trip to memory)
    const uint32_t bw = b0[pc >> 5];
    const uint32_t cn = P.q_cons[qo + pc];
    const uint32_t bb = (uint32_t)lane < P.M.n_roles ? P.blkbase[po + (size_t)lane * P.blk_stride + b] : 0u;
    const bool alive = pos < m && ((bw >> (pos & 31u)) & 1u);
    const uint32_t role = (cn >> 16) & 7u;
    const unsigned long long le = (2ull << (a & 63u)) - 1ull;
    uint32_t st = 0;
    for (uint32_t r = 0; r < P.M.n_roles; ++r) {
        const unsigned long long mk = __ballot(alive && role == r);
        if ((uint32_t)lane == r) st = bb + (uint32_t)__popcll(mk & le);
    }
    return st;
}

// S.pos[0..n) -> S.spos ascending (queue order = seat order), with the players' records
static __device__ __forceinline__ void tw_sort_load(TwScratch& S, uint32_t n, const TeamParams& P, uint32_t g, int lane)
{
    const size_t qo = ((size_t)P.mode * P.n_groups + g) * P.capacity;
    wave_sync();
    uint32_t mine = 0, rk = 0;
    if ((uint32_t)lane < n) {
        mine = S.pos[lane];
        for (uint32_t k = 0; k < n; ++k) rk += S.pos[k] < mine ? 1u : 0u;
    }
    wave_sync();
    if ((uint32_t)lane < n) {
        S.spos[rk] = mine;
        S.rat[rk] = P.q_rating[qo + mine];
        S.con[rk] = P.q_cons[qo + mine];
        S.slo[rk] = P.q_slot[qo + mine];
        S.sqx[rk] = P.sqi[(size_t)g * P.pstride + mine];
    }
    wave_sync();
}

// docs/MATCH_CHECK.md §2.3-2.4 for S's players in queue order; they are known to be seatable
static __device__ __forceinline__ uint32_t tw_replay(LobbyDev& lb, const TwScratch& S, uint32_t n, const ModeDev& M, int lane)
{
    LobbySum L;
    wave_sync();
    lsum_load(L, lb, M);
    uint32_t err = 0;
    for (uint32_t k = 0; k < n; ++k)
        if (lsum_seat(L, lb, M, S.rat[k], S.con[k], S.slo[k], lane) < 0) err = MM_ERRF_SEAT_INVARIANT;
    wave_sync();
    return err;
}

// A player leaves the queue.  WHAT: the records of the queue that the caller keeps current with this call —
//   TQ_BITS   its bit in `bits`, the chaser's bitmap: bits[1] in memory (the pass kernels) or kt_late's copy in LDS
//   TQ_CHUNK  its role's population of its chunk
//   TQ_TOMB   its entry `sqx` of the role sub-queue (tw_sort_load's S.sqx; TQ_SQI: looked up here, a trip more) becomes a tombstone, a key no
//             interval holds, and stays where it is until kt_build runs again.  kt_late writes none: its bitmap skips the entries, the next tick rebuilds.
enum { TQ_BITS = 1, TQ_CHUNK = 2, TQ_TOMB = 4, TQ_ALL = 7, TQ_SQI = 8 };
static __device__ __forceinline__ uint32_t* tq_chunk(const TeamParams& P, uint32_t g, uint32_t role, uint32_t pos)
{
    return &P.chunk[((size_t)g * MM_MAX_ROLES + role) * P.chunk_stride + pos / TT_CH];
}
template <int WHAT>
static __device__ __forceinline__ void tq_leave(const TeamParams& P, uint32_t g, uint32_t* bits, uint32_t pos, uint32_t cons, uint32_t sqx)
{
    if (WHAT & TQ_BITS) atomicAnd(&bits[pos >> 5], ~(1u << (pos & 31u)));
    if (WHAT & TQ_CHUNK) atomicSub(tq_chunk(P, g, (cons >> 16) & 7u, pos), 1u);
    if (WHAT & TQ_TOMB) P.sqk[(size_t)g * P.pstride + ((WHAT & TQ_SQI) ? P.sqi[(size_t)g * P.pstride + pos] : sqx)] = 0xFFFFFFFFu;
}
// ... S's players, a lane each
template <int WHAT>
static __device__ __forceinline__ void tq_kill(const TeamParams& P, uint32_t g, uint32_t* bits, const TwScratch& S, uint32_t n, int lane)
{
    if ((uint32_t)lane < n) tq_leave<WHAT>(P, g, bits, S.spos[lane], S.con[lane], (WHAT & TQ_SQI) ? 0u : S.sqx[lane]);
}

// the lobby record is empty again
static __device__ __forceinline__ void lobby_clear(LobbyDev& lb, int lane)
{
    if (lane == 0) {
        lb.n = 0;
        for (uint32_t t = 0; t < MM_MAX_TEAMS; ++t) lb.cnt[t] = 0;
    }
}

// seats per role of the lobby an anchor of role `arole` opens, a nibble each: teams * quota[r], less the anchor's own
static __device__ __forceinline__ uint32_t lobby_needs(const ModeDev& M, uint32_t arole)
{
    uint32_t needs = 0;
    for (uint32_t r = 0; r < M.n_roles; ++r) needs |= (M.teams * M.quota[r] - (r == arole ? 1u : 0u)) << (4u * r);
    return needs;
}

static __device__ __forceinline__ void tw_lobby_copy(uint32_t* dst, const uint32_t* src, int lane)
{
    wave_sync();
    for (uint32_t i = (uint32_t)lane; i < (uint32_t)(sizeof(LobbyDev) / 4); i += 64u) dst[i] = src[i];
    wave_sync();
}

// tw_collect, eight 64-entry steps per trip to memory.  BITS: only entries whose player is still queued by the LDS
// bitmap `bits` (kt_late, which writes no tombstones); without it the keys decide alone (a tombstone fits no interval).
template <int BITS, int S2>          // S2: 64-entry steps a trip (registers: two a step)
static __device__ __forceinline__ uint32_t tl_collect(const uint32_t* sk, const uint32_t* sp, const uint32_t* bits, uint32_t j0, uint32_t len,
                                      uint32_t need, uint32_t lo, uint32_t rng, uint32_t* out, uint32_t nout, int lane,
                                      uint32_t& scanned)
{
    uint32_t got = 0;
    for (uint32_t p = j0; p < len && got < need; p += 64u * S2) {
        scanned += 64u * S2;
        uint32_t k[S2], q[S2];
        // (scalar bases, one shared lane offset per step: the loads need no address registers of their own)
        const uint32_t* const bk = sk + p;
        const uint32_t* const bp = sp + p;
        const uint32_t rem = len - p;
#pragma unroll
        for (uint32_t u = 0; u < (uint32_t)S2; ++u) {
            const uint32_t i = u * 64u + (uint32_t)lane;
            k[u] = i < rem ? bk[i] : 0xFFFFFFFFu;
            q[u] = i < rem ? bp[i] : 0u;
        }
#pragma unroll
        for (uint32_t u = 0; u < (uint32_t)S2; ++u) {
            const bool ok = pk_in(k[u], lo, rng) && (!BITS || l_alive(bits, q[u]));      // a key of padding lies above every interval
            const unsigned long long b = __ballot(ok);
            const uint32_t nb = (uint32_t)__popcll(b), room = need - got;
            const uint32_t rk = (uint32_t)__popcll(b & ((1ull << lane) - 1ull));
            if (ok && rk < room) out[nout + got + rk] = q[u];
            got += nb < room ? nb : room;
        }
    }
    return got;
}

// The look-up of a lobby, all roles at once: the first TLA_STEPS x 64 entries of EVERY role's stretch are asked for
// together (one trip to memory instead of one per role — the stretches come from HBM, 0.7 us a trip); a role that
// needs more goes on alone, eight steps a trip.  `needs`: seats per role, a nibble each; `st`: lane r holds the
// role's first entry.  Appends the positions to out[nout..]; returns the number found, *short_mask: roles that ran dry.
template <int BITS, int S1, int S2>  // S1: 64-entry steps of every role in the first trip; S2: of one role in the trips after it
static __device__ __forceinline__ uint32_t tl_collect_all(const TeamParams& P, const uint32_t (&rlen)[MM_MAX_ROLES], const uint32_t (&roff)[MM_MAX_ROLES],
                                          size_t po, const uint32_t* bits, uint32_t st,
                                          uint32_t needs, uint32_t lo, uint32_t rng, uint32_t* out, uint32_t nout, int lane,
                                          uint32_t* short_mask, uint32_t (&scanned)[MM_MAX_ROLES])   // (MM_PAIR_DEBUG's counters: registers)
{
    const uint32_t nr = P.M.n_roles;
    uint32_t k[MM_MAX_ROLES][S1], q[MM_MAX_ROLES][S1], j0[MM_MAX_ROLES], len[MM_MAX_ROLES];
#pragma unroll
    for (uint32_t r = 0; r < MM_MAX_ROLES; ++r) {
        j0[r] = lane_get(st, (int)r);                          // (a scalar)
        len[r] = r < nr ? rlen[r] : 0u;                        // the chain's sub-queues do not move while kt_late runs: the caller holds them
        const bool on = r < nr && ((needs >> (4u * r)) & 15u) != 0u;
        // (scalar bases, one shared lane offset per step: the loads need no address registers of their own)
        const uint32_t* const bk = P.sqk + po + (r < nr ? roff[r] : 0u) + j0[r];
        const uint32_t* const bp = P.sqp + po + (r < nr ? roff[r] : 0u) + j0[r];
        const uint32_t rem = on && len[r] > j0[r] ? len[r] - j0[r] : 0u;
#pragma unroll
        for (uint32_t u = 0; u < (uint32_t)S1; ++u) {
            const uint32_t i = u * 64u + (uint32_t)lane;
            k[r][u] = i < rem ? bk[i] : 0xFFFFFFFFu;
            q[r][u] = i < rem ? bp[i] : 0u;
        }
    }
    uint32_t got_all = 0, dry = 0;
#pragma unroll
    for (uint32_t r = 0; r < MM_MAX_ROLES; ++r) {
        const uint32_t need = r < nr ? (needs >> (4u * r)) & 15u : 0u;
        if (!need) continue;
        uint32_t got = 0;
        scanned[r] += S1 * 64u;
#pragma unroll
        for (uint32_t u = 0; u < (uint32_t)S1; ++u) {
            const bool ok = pk_in(k[r][u], lo, rng) && (!BITS || l_alive(bits, q[r][u]));
            const unsigned long long b = __ballot(ok);
            const uint32_t nb = (uint32_t)__popcll(b), room = need - got;
            const uint32_t rk = (uint32_t)__popcll(b & ((1ull << lane) - 1ull));
            if (ok && rk < room) out[nout + got_all + got + rk] = q[r][u];
            got += nb < room ? nb : room;
        }
        if (got < need && j0[r] + S1 * 64u < len[r])
            got += tl_collect<BITS, S2>(P.sqk + po + roff[r], P.sqp + po + roff[r], bits, j0[r] + S1 * 64u, len[r], need - got,
                              lo, rng, out, nout + got_all + got, lane, scanned[r]);
        if (got < need) dry |= 1u << r;
        got_all += got;
    }
    *short_mask = dry;
    return got_all;
}

// the filled lobby `lb`, in team order (search/worker.ex:313-319)
static __device__ __forceinline__ void tl_write_lobby(const TeamParams& P, uint32_t g, const LobbyDev& lb, uint32_t idx, uint32_t pass)
{
    const ModeDev& M = P.M;
    long long smin = 0, smax = 0;
    uint32_t k = 0;
    uint32_t* os = P.out_slots + (size_t)g * P.out_slot_stride + (size_t)idx * M.L;
    for (uint32_t t = 0; t < M.teams; ++t) {
        long long sm = 0;
        for (uint32_t j = 0; j < lb.cnt[t]; ++j) {
            os[k++] = lb.slot[t][j];
            sm += lb.rating[t][j];
        }
        if (t == 0 || sm < smin) smin = sm;
        if (t == 0 || sm > smax) smax = sm;
    }
    // |team sums| differ by up to 2^35 (a window of 2^30 - 1 around the anchor, 8 a team): the difference is exact in
    // double, the quotient is rounded to f32 once (see k_walk's emission)
    P.out_score[(size_t)g * P.out_rec_stride + idx] = (float)((double)(smax - smin) / (double)M.team_size);
    P.out_pass[(size_t)g * P.out_rec_stride + idx] = pass;
}

// The tail of an emission, for the members in S.pos[0..nf) and an empty `lb`: their records in queue order, the seats replayed
// (the team choice needs the order), the lobby written at out index `idx`, the players taken out of the queue (WHAT, bits: tq_leave).
template <int WHAT>
static __device__ __forceinline__ uint32_t emit_members(const TeamParams& P, uint32_t g, LobbyDev& lb, TwScratch& S, uint32_t nf,
                                                        uint32_t idx, uint32_t pass, uint32_t err, uint32_t* bits, int lane)
{
    tw_sort_load(S, nf, P, g, lane);
    err |= tw_replay(lb, S, nf, P.M, lane);
    if (lb.n != P.M.L) err |= MM_ERRF_SEAT_INVARIANT;
    // is_filled: emit in team order (search/worker.ex:313-319)
    if (lane == 0 && !err) tl_write_lobby(P, g, lb, idx, pass);
    tq_kill<WHAT>(P, g, bits, S, nf, lane);
    return err;
}

// One lobby a pass emits (kt_emit's unit of work, and the emitter waves' behind kt_chase): the anchor `a`, its members
// from kt_f's record (or looked up when kt_chase went by its own look-up), the seats replayed in queue order (the team
// choice needs the order), the lobby written at out index `idx`, the players taken out of the queue.
// LIVE: kt_f's workgroups run in the same launch (kt_fc) — the anchor's record was stored through to memory before its
// chunk's flag went up, and is read from there.
template <int LIVE>
static __device__ __forceinline__ uint32_t te_emit_one(const TeamParams& P, uint32_t g, const TeamChain* tc, LobbyDev& lb, TwScratch& S,
                                                       uint32_t a, uint32_t idx, uint32_t pass, uint32_t err, int lane)
{
    const ModeDev& M = P.M;
    const size_t qo = ((size_t)P.mode * P.n_groups + g) * P.capacity, po = (size_t)g * P.pstride;
    const uint32_t m = tc->m, nr = M.n_roles;
    const bool looked = (a & TV_LOOKED) != 0u;                // the chaser did not have kt_f's F for this anchor: neither do we
    a &= ~TV_LOOKED;
    wave_sync();
    lobby_clear(lb, lane);
    if (lane == 0) S.pos[0] = a;
    const uint32_t LM = M.L - 1u;
    const bool mine = (uint32_t)lane >= 1u && (uint32_t)lane <= LM;
    uint32_t Fa, fpa, dm = 0;                                 // all of the record in one trip
    if (LIVE) {
        Fa = pub_ld(&P.fv[po + a]);
        fpa = pub_ld(&P.fpos[po + a]);
        if (mine) dm = __hip_atomic_load(&P.memb[(po + a) * LM + (uint32_t)lane - 1u], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    } else {
        Fa = P.fv[po + a];
        fpa = P.fpos[po + a];
        if (mine) dm = P.memb[(po + a) * LM + (uint32_t)lane - 1u];
    }
    const bool rec = !looked && Fa != TT_PART && Fa != TT_UNK && fpa != TT_NONE;   // kt_chase went by kt_f's F, and kt_f left the lobby on record
    uint32_t nf = 1;
    if (rec) {
        if (mine) S.pos[lane] = a + dm;
        nf = M.L;
    }
    uint32_t lo = 0, rng = 0, needs = 0, st = 0;
    if (!rec) {
        pk_bounds(P.tkey[po + a], P.window, lo, rng);
        needs = lobby_needs(M, (P.q_cons[qo + a] >> 16) & 7u);
        st = tw_starts(P, g, a, m, lane);
    }
    for (uint32_t r = 0; r < nr && !rec; ++r) {
        const uint32_t need = (needs >> (4u * r)) & 15u;
        const uint32_t j0 = lane_get(st, (int)r);
        if (!need) continue;
        const uint32_t got = tw_collect(P.sqk + po + tc->off[r], P.sqp + po + tc->off[r], j0, tc->len[r], need,
                                        lo, rng, S.pos, nf, lane);
        nf += got;
        if (got < need) err |= MM_ERRF_SEAT_INVARIANT;
    }
    return emit_members<TQ_ALL>(P, g, lb, S, nf, idx, pass, err, P.bits[1] + (size_t)g * P.bits_stride, lane);
}


// ------------------------------------------------------------------------------------
// kt_chase: one pass of every chain.  Workgroup g < n_groups is chain g's CHASER (wave 0 chases, the other
// waves pull F through the XCD's L2).  With P.n_emit > 0 the launch carries n_emit EMITTER workgroups per chain
// behind the chasers (workgroups are dispatched in index order, so a chaser is on the chip before the emitters
// that wait for it): every wave of them takes the lobbies  w, w + W, w + 2W ...  of the pass (W waves per chain)
// off vis[] as the chaser publishes them — kt_emit's work, begun while the chase is still running instead of
// in a launch of its own behind it.  What crosses between the workgroups goes through agent-scope atomics:
// vis[i] (TT_NONE: not published yet; the emitter puts TT_NONE back), TeamChain.pub_*.
// Exactness: an emitter takes players out behind the cursor only (a lobby's members all lie before the
// next anchor), and the chaser reads the bitmap of the start of the pass (bits[0]) and sub-queue entries of
// positions beyond the cursor — nothing an emitter writes.
// ------------------------------------------------------------------------------------
#define TC_THREADS 1024
#define TC_WAVES (TC_THREADS / 64)
#define TC_EMIT_MAX 32u              // emitter workgroups per chain at most
static_assert(TC_EMIT_MAX * TC_WAVES <= TV_AHEAD, "kt_pack resets TV_AHEAD words of vis[] behind the queue");
// TW_SINK / tw_sload (the dependent load of the chase through the scalar cache): <mm_gfx950.h>

// An emitter workgroup (index eb among the launch's emitters) of `n_waves` waves: chain eb % n_groups.  Wave 0 is the
// workgroup's DISPATCHER — the only wave that looks at memory while there is nothing to do: lane j keeps worker wave
// j's next index into vis[], one vector load looks at all of them, and an anchor that has arrived goes into the
// worker's slot in LDS (and TT_NONE back into vis[]).  The workers wait on their slots.  (Every wave polling vis[]
// for itself — the first version — put 2 500 waves on 14 cache lines in the lobby-rich passes.)
#define TT_END 0xFFFFFFFCu           // a worker's slot: the pass is over for you
struct EmitCtl { uint32_t slot[TC_WAVES], idx[TC_WAVES], go, base, pass; };
template <int LIVE>
static __device__ __forceinline__ void tc_emitter(const TeamParams& P, uint32_t eb, uint32_t n_waves, int wave, int lane,
                                                  LobbyDev& lb, TwScratch& S, EmitCtl& C)
{
    const uint32_t g = eb % P.n_groups;
    TeamChain* const tc = P.tchains + g;
    if (!tc->fast) return;
    if (threadIdx.x < TC_WAVES) C.slot[threadIdx.x] = TT_NONE;
    if (threadIdx.x == 0) C.go = 0;
    __syncthreads();
    const uint32_t nw = n_waves - 1u, W = P.n_emit * nw;
    if (wave == 0) {
        uint32_t* const vis = P.vis + (size_t)g * P.pstride;
        uint32_t spins = 0;
        bool dead = false;
        // the chaser's go (the stored lobby has met the queue: the index of vis[0]'s lobby is known), or the end of
        // a pass that has nothing for anybody
        for (;;) {
            const unsigned long long go = pub_ld64(&tc->pub_go), en = pub_ld64(&tc->pub_end);
            if ((uint32_t)(go >> 32) == P.seq) { if (lane == 0) C.base = (uint32_t)go; break; }
            if ((uint32_t)(en >> 32) == P.seq && (uint32_t)en == 0u) { dead = true; break; }
            __builtin_amdgcn_s_sleep(8);
            if (++spins > TC_SPIN_MAX) { if (lane == 0) atomicOr(&tc->err, MM_ERRF_SYNC_TIMEOUT); dead = true; break; }
        }
        if (!dead && lane == 0) C.pass = pub_ld(&tc->pub_pass);          // (stored and acknowledged before the go)
        wave_sync();
        if (lane == 0) lds_st(&C.go, dead ? 2u : 1u);
        if (dead) return;
        const bool mine = (uint32_t)lane >= 1u && (uint32_t)lane <= nw;
        uint32_t my_i = (eb / P.n_groups) * nw + (uint32_t)lane - 1u;
        bool fin = !mine;
        for (;;) {
            const bool free = !fin && lds_ld(&C.slot[lane]) == TT_NONE;
            // every worker's next entry and the end word in one trip; the end word is stored after every entry has arrived
            uint32_t v = TT_NONE;
            // (my_i < pstride: kt_pack resets vis[] behind the queue up to the group's stride and no further — ADVICE r05: with
            // a chain within TV_AHEAD of its stride the look-ahead ran into the next group's anchors, past the allocation for the last)
            if (free && my_i < P.pstride) v = __hip_atomic_load(&vis[my_i], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            const unsigned long long en = pub_ld64(&tc->pub_end);
            if (free && v != TT_NONE) {
                C.idx[lane] = my_i;
                __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
                lds_st(&C.slot[lane], v);
                pub_st(&vis[my_i], TT_NONE);
                my_i += W;
            } else if (free && (uint32_t)(en >> 32) == P.seq && my_i >= (uint32_t)en) {
                lds_st(&C.slot[lane], TT_END);
                fin = true;
            }
            if (!__ballot(!fin)) break;
            __builtin_amdgcn_s_sleep(4);
            if (++spins > TC_SPIN_MAX) {
                if (lane == 0) atomicOr(&tc->err, MM_ERRF_SYNC_TIMEOUT);
                if (mine) lds_st(&C.slot[lane], TT_END);
                break;
            }
        }
        return;
    }
    // ---------------- a worker ----------------
    uint32_t err = 0, spins = 0;
    uint32_t go;
    while ((go = uni(lds_ld(&C.go))) == 0u) {
        __builtin_amdgcn_s_sleep(4);
        if (++spins > 8u * TC_SPIN_MAX) return;
    }
    if (go != 1u) return;
    const uint32_t base = uni(lds_ld(&C.base)), pass = uni(lds_ld(&C.pass));
    for (;;) {
        uint32_t a;
        while ((a = uni(lds_ld(&C.slot[wave]))) == TT_NONE) {
            __builtin_amdgcn_s_sleep(2);
            if (++spins > 8u * TC_SPIN_MAX) { a = TT_END; err |= MM_ERRF_SYNC_TIMEOUT; break; }
        }
        if (a == TT_END) break;
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
        const uint32_t i = uni(lds_ld(&C.idx[wave]));
        wave_sync();                                         // (every lane has seen them)
        if (lane == 0) lds_st(&C.slot[wave], TT_NONE);       // the dispatcher may bring the next one
        if (base + i >= P.out_cap) continue;                 // the chaser reports the overflow
        err = te_emit_one<LIVE>(P, g, tc, lb, S, a, base + i, pass, err, lane);
    }
    if (err && lane == 0) atomicOr(&tc->err, err);
}

// ------------------------------------------------------------------------------------
// The chaser's own look-ups (the lobby that stays open at the end of a pass, an anchor beyond kt_f's horizon, the stored
// lobby's fill from the head of the queue), role by role on HELPER waves of its workgroup.  A look-up was one wave going
// through the roles one after the other — a trip to memory per role and 256 entries, and the role that runs dry (every pass
// ends on one) is read to its end: ~13 dependent trips, 11 us, twice a pass, a quarter of a cfg-3 tick.  Now wave 0 posts
// the look-up in LDS (where every role's stretch begins, how many it needs, the anchor's interval) and takes role 0 itself;
// wave r takes role r, 512 entries a trip; wave 0 collects what they found.  A look-up costs what its longest role costs.
// ------------------------------------------------------------------------------------
#define TLK_EXIT 0xFFFFFFFFu
struct LookCtl {
    uint32_t seq;                        // the look-up's number (wave 0 counts them; TLK_EXIT: the chaser is through)
    uint32_t lo, rng;                    // the anchor's interval
    uint32_t j0[MM_MAX_ROLES], need[MM_MAX_ROLES];
    uint32_t ack[MM_MAX_ROLES];          // role r's helper: = seq once got / pos / scanned stand
    uint32_t got[MM_MAX_ROLES], scanned[MM_MAX_ROLES];
    uint32_t off[MM_MAX_ROLES], len[MM_MAX_ROLES];   // the chain's sub-queues in this pass (wave 0 has them: no trip for the helpers)
    uint32_t pos[MM_MAX_ROLES][MM_MAX_LOBBY];
};

// wave `r` (1 <= r < roles) of the chaser's workgroup
static __device__ __forceinline__ void tlk_helper(const TeamParams& P, uint32_t g, LookCtl& K, uint32_t r, int lane)
{
    const size_t po = (size_t)g * P.pstride;
    uint32_t seen = 0;
    for (;;) {
        // (no time-out of its own: the chaser is a wave of this workgroup, says good-bye on every way out, and may be kept
        // waiting for a long time itself — by chunks that find no CU — before its next look-up)
        const uint32_t sq = uni(lds_ld(&K.seq));
        if (sq == TLK_EXIT) break;
        if (sq == seen) { __builtin_amdgcn_s_sleep(1); continue; }
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
        seen = sq;
        const uint32_t need = uni(lds_ld(&K.need[r]));
        uint32_t got = 0, scanned = 0;
        if (need) {
            const uint32_t off = uni(lds_ld(&K.off[r])), len = uni(lds_ld(&K.len[r]));
            got = tl_collect<0, 8>(P.sqk + po + off, P.sqp + po + off, nullptr, uni(lds_ld(&K.j0[r])), len, need,
                                   uni(lds_ld(&K.lo)), uni(lds_ld(&K.rng)), K.pos[r], 0u, lane, scanned);
        }
        wave_sync();
        if (lane == 0) { K.got[r] = got; K.scanned[r] = scanned; }
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
        if (lane == 0) lds_st(&K.ack[r], sq);
    }
}

// wave 0: one look-up.  st: lane r holds where role r's stretch begins (v_off, v_len: the role's sub-queue); needs: seats per role, a nibble each.  The
// positions found are appended to out[nout..] (role after role); returns their number, *dry: the roles that ran dry.
static __device__ __forceinline__ uint32_t tlk_lookup(const TeamParams& P, uint32_t g, uint32_t v_off, uint32_t v_len, LookCtl& K, uint32_t& kseq,
                                                      uint32_t st, uint32_t needs, uint32_t lo, uint32_t rng,
                                                      uint32_t* out, uint32_t nout, int lane, uint32_t* dry, uint32_t& scanned)
{
    const uint32_t nr = P.M.n_roles, nw = blockDim.x >> 6;    // (roles beyond the workgroup's waves stay with wave 0)
    const size_t po = (size_t)g * P.pstride;
    wave_sync();
    if ((uint32_t)lane < nr) {
        K.j0[lane] = st;
        K.need[lane] = (needs >> (4u * (uint32_t)lane)) & 15u;
        K.off[lane] = v_off;                                  // (the chaser loaded them when it began: they do not move within a pass)
        K.len[lane] = v_len;
    }
    if (lane == 0) { K.lo = lo; K.rng = rng; }
    kseq = kseq + 1u == TLK_EXIT ? 1u : kseq + 1u;
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
    if (lane == 0) lds_st(&K.seq, kseq);
    // role 0 is wave 0's own (and the roles beyond the workgroup's waves)
    uint32_t got_all = 0, dm = 0;
    for (uint32_t r = 0; r < nr; r = r ? r + 1u : (nw < nr ? nw : nr)) {
        const uint32_t need = (needs >> (4u * r)) & 15u;
        if (!need) continue;
        const uint32_t off = lane_get(v_off, (int)r);
        const uint32_t got = tl_collect<0, 8>(P.sqk + po + off, P.sqp + po + off, nullptr, lane_get(st, (int)r), lane_get(v_len, (int)r), need,
                                              lo, rng, out, nout + got_all, lane, scanned);
        if (got < need) dm |= 1u << r;
        got_all += got;
    }
    uint32_t err = 0;
    for (uint32_t r = 1; r < nr && r < nw; ++r) {
        const uint32_t need = (needs >> (4u * r)) & 15u;
        uint32_t spins = 0;
        while (uni(lds_ld(&K.ack[r])) != kseq) {
            __builtin_amdgcn_s_sleep(1);
            if (++spins > 8u * TC_SPIN_MAX) { err = 1u; break; }
        }
        if (err) break;
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
        if (!need) continue;
        const uint32_t got = uni(lds_ld(&K.got[r]));
        if ((uint32_t)lane < got) out[nout + got_all + (uint32_t)lane] = K.pos[r][lane];
        scanned += uni(lds_ld(&K.scanned[r]));
        if (got < need) dm |= 1u << r;
        got_all += got;
    }
    wave_sync();
    *dry = err ? 0x80000000u | dm : dm;                       // (bit 31: a helper did not answer — MM_ERRF_SYNC_TIMEOUT for the caller)
    return got_all;
}

// kt_fc: F of the anchor `a`, as soon as kt_f's workgroup of its chunk — same launch — has stored it.  The flags of
// 64 chunks from `fbase` on are kept in `fready` (a look at them is one trip for 32 768 positions).
static __device__ __forceinline__ uint32_t tcf_load(const TeamParams& P, uint32_t g, uint32_t a, uint32_t& fbase,
                                                    unsigned long long& fready, uint32_t& err, long long& waited, int lane,
                                                    uint32_t& fwait)
{
    const uint32_t ck = a / TT_CH;
    uint32_t spins = 0;
    const long long w0 = P.debug ? clock64() : 0;
    if (P.nowait && ck % P.nowait == 0u) return TT_WAIT;       // test hook: this chunk's flag "never comes"
    for (;;) {
        if (ck - fbase < 64u && ((fready >> (ck - fbase)) & 1ull)) break;
        if (ck - fbase >= 64u) fbase = ck;                    // (the cursor only moves forward)
        uint32_t fi = fbase + (uint32_t)lane;
        fi = fi < P.chunk_stride ? fi : P.chunk_stride - 1u;
        const uint32_t v = __hip_atomic_load(&P.fdone[(size_t)g * P.chunk_stride + fi], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        fready = __ballot(v == P.seq);
        if ((fready >> (ck - fbase)) & 1ull) {
            // (nothing this CU's scalar cache holds of the chunks whose flags have just been seen may be older than the flags:
            // nobody has read those lines in this launch, by the reasoning below — the invalidate makes it hold by construction)
            tw_sinv();
            break;
        }
        // A chunk that is late — its workgroup found no CU yet: somebody else's kernels hold them — is no reason to fail the
        // tick: F is a short cut, the chaser can always look the lobby up itself (what it does for TT_UNK).  Nothing in this
        // launch waits for a workgroup that may not be on the chip.
        __builtin_amdgcn_s_sleep(4);
        // (after the first flag that did not come the chaser does not wait long for the others of the pass: the chunks are
        // late because something else holds the CUs, and 586 chunks x MM_TEAM_FWAIT would be seconds)
        if (++spins > fwait) { fwait = fwait > 64u ? fwait >> 8 : fwait; return TT_WAIT; }
    }
    if (P.debug) waited += clock64() - w0;                    // MM_PAIR_DEBUG: cycles spent on the flags
    // The chunk is final and was stored through to memory.  A plain load through the scalar cache is safe: nothing on
    // this XCD has looked at the chunk's F since the launch began, except its own kt_f workgroup (whose stores its L2
    // has seen).  (Measured and dropped: the workgroup's other waves pulling every finished chunk through the XCD's
    // L2 ahead of the chaser, as kt_chase's do — a hop costs 505 cycles with and 490 without.)
    return tw_sload(P.fv + (size_t)g * P.pstride + a);
}

// ------------------------------------------------------------------------------------
// A pass of a chain around its chase.  pass_close — the pass's counters, the first-pass rules of a cancel tick, `done` — is
// one body for tc_chaser (kt_chase, kt_fc, kt_f's head-fill column) and kt_late's wave 0.  head_fill (the stored lobby meets
// the queue from its head) and open_lobby_close (the lobby that stays open) are kt_late's; tc_chaser keeps its own text of
// both: built on head_fill alone kt_fc's pass was 1.9 us slower, with the view in its chase loop more; and kt_late with its own
// text inline again runs 1 % slower than with these two functions (profiles/team_pass_refactor_check.txt, 4a, 4c).  A rule changed in one
// is changed in the other; what they share beneath — lobby_clear, lobby_needs, tq_kill, lsum_seat — is written once.
// ------------------------------------------------------------------------------------
struct PassTally { uint32_t nvis, head, n_open, gone, err; bool changed, over; };       // what one pass did; over: the chase has nothing left to do
struct PassCounts { uint32_t qlen, passes, n_out; unsigned long long pairs, scanned; };  // the chain's running counts (TeamChain's)

// How kt_late's chaser sees the queue: the bitmap in LDS, current (a pass only takes players out behind the cursor); look-ups by
// the chaser alone, all roles abreast, the entries of players that left skipped by the bitmap; no tombstones.
struct QvLate {
    enum { KILL = TQ_BITS | TQ_CHUNK };
    const TeamParams& P;
    const uint32_t g;
    uint32_t* const bits;
    const uint32_t (&rlen)[MM_MAX_ROLES];                     // the sub-queues of the last kt_build: fixed for the launch
    const uint32_t (&roff)[MM_MAX_ROLES];
    uint32_t (&d_sc)[MM_MAX_ROLES];                           // MM_PAIR_DEBUG: sub-queue entries scanned per role
    __device__ __forceinline__ uint32_t succ(uint32_t from, uint32_t m, int lane) const { return uni(l_succ(bits, from, m, lane)); }
    __device__ __forceinline__ uint32_t lookup(uint32_t st, uint32_t needs, uint32_t lo, uint32_t rng, uint32_t* out, uint32_t nout, int lane,
                                               uint32_t* dry)
    {
        return tl_collect_all<1, 2, 8>(P, rlen, roff, (size_t)g * P.pstride, bits, st, needs, lo, rng, out, nout, lane, dry, d_sc);
    }
};
static_assert(PK_NO == TT_NONE, "l_succ's and tw_succ's `nobody` are one value");

// The stored lobby meets the queue from its head (LobbyState.get_state, lobby_state.ex:61-104).
// Normally one window: the anchor in the first team.  After a cancel emptied the lower
// teams, the first player seated there becomes the anchor (MATCH_CHECK.md section 2.1) and
// the players behind it are judged by ITS window: collect with the current anchor, seat
// in queue order until the anchor moves, collect again from there.
// If the lobby fills it is emitted right here (out index *n_out, pass *pass: read only then) and `lb` is empty from then on.
// Returns where the chase begins (TT_NONE: nobody is queued behind); T.over: everybody was popped against the lobby and it
// is still open — the pass is over.
// A seated player leaves the queue at once, on lane 0 (tc_chaser's own fill: together when the fill is over, for the tombstones' trip).
static __device__ __forceinline__ uint32_t head_fill(QvLate& V, TeamChain* tc, LobbySum& L, LobbyDev& lb, TwScratch& S, uint32_t m,
                                                     const uint32_t* n_out, const uint32_t* pass, PassTally& T, int lane)
{
    const TeamParams& P = V.P;
    const ModeDev& M = P.M;
    const uint32_t g = V.g;
    uint32_t nseat = 0, from = 0;
    bool moved = true;
    for (uint32_t stage = 0; stage < MM_MAX_TEAMS && moved && L.n < M.L; ++stage) {
        moved = false;
        uint32_t lo, rng;
        pk_bounds(pk_pack(L.ar, L.ac, tc->rmin, P.eqmask), P.window, lo, rng);
        const uint32_t st = from ? tw_starts(P, g, from - 1u, m, lane) : 0u;
        wave_sync();
        uint32_t dry = 0;
        const uint32_t nf = V.lookup(st, L.free, lo, rng, S.pos, 0u, lane, &dry);
        tw_sort_load(S, nf, P, g, lane);
        const uint32_t at0 = L.at;
        uint32_t k = 0;
        while (k < nf && !moved) {
            if (lsum_seat(L, lb, M, S.rat[k], S.con[k], S.slo[k], lane) < 0) T.err |= MM_ERRF_SEAT_INVARIANT;
            if (lane == 0) tq_leave<QvLate::KILL>(P, g, V.bits, S.spos[k], S.con[k], 0u);   // the open lobby holds the player from here on
            ++nseat;
            ++k;
            if (L.at != at0) moved = true;
        }
        wave_sync();
        if (k) from = S.spos[k - 1u] + 1u;
        if (moved && lane == 0) tc->dbg[7] += 1u;
    }
    wave_sync();
    T.gone += nseat;
    T.changed = nseat > 0u;
    T.over = L.n != M.L;
    if (T.over) return TT_NONE;
    // filled by the player at from - 1 (lb holds it, seated in queue order)
    if (*n_out >= P.out_cap) T.err |= MM_ERRF_OUT_OVERFLOW;
    else if (lane == 0) tl_write_lobby(P, g, lb, *n_out, *pass);
    wave_sync();
    lobby_clear(lb, lane);
    wave_sync();
    lsum_load(L, lb, M);
    T.head = 1;
    T.changed = true;
    return V.succ(from, m, lane);
}

// The lobby the anchor S.pos[0] opens stays open: it and everybody it takes (S, in queue order) are seated, nobody else
// is queued behind — the pass is over.
static __device__ __forceinline__ void open_lobby_close(const QvLate& V, LobbyDev& lb, const TwScratch& S, uint32_t nf, PassTally& T, int lane)
{
    T.err |= tw_replay(lb, S, nf, V.P.M, lane);
    tq_kill<QvLate::KILL>(V.P, V.g, V.bits, S, nf, lane);
    T.n_open = 1;
    T.changed = true;
    T.gone += nf;
    T.over = true;
}

// The end of a pass: the chain's counts move on by what the pass did.  On the first pass of a cancel tick the head was
// popped against the stale lobby in kt_init; if that rejected it, it sat the pass out and is back in the queue for the next
// (lane 0 puts it back into `bits`, the chaser's current bitmap; team_walk keeps such a tick from kt_late to this day — a
// head that sat out is not in the first pass's sub-queues — but the rule is the same one).  Returns `done`.
static __device__ __forceinline__ bool pass_close(const TeamParams& P, uint32_t g, const TeamChain* tc, uint32_t* bits, PassTally& T,
                                                  PassCounts& C, int lane)
{
    const uint32_t left = C.qlen - T.gone - T.nvis * P.M.L;
    const bool first = C.passes == 0u;
    const uint32_t popped = C.qlen + (first ? tc->extra0 : 0u);
    if (first && tc->changed0) T.changed = true;
    if (first && tc->sitout && lane == 0) {
        atomicOr(&bits[0], 1u);
        atomicAdd(tq_chunk(P, g, tc->head_role, 0u), 1u);
    }
    C.n_out += T.head + T.nvis;
    C.pairs += (unsigned long long)(popped - (T.nvis + T.n_open));
    C.scanned += (unsigned long long)popped;
    C.qlen = left;
    C.passes += 1u;
    return !(T.changed || T.nvis) || left == 0u || T.err;
}

// The chaser of chain g (one wave).  USE_F2: the passes that have F o F (kt_f2) — its own instantiation, so that the
// plain chase stays as tight as it was.  LIVE: kt_f's chunks run in the same launch (kt_fc).
// PHASE 0: a whole pass.  1: only the stored lobby's fill from the head of the queue (in kt_f's launch, beside its chunks: it needs
// nothing of F — what it takes out lies in front of where the chase begins, which is what kt_fc's argument needs of it); the state goes
// into TeamChain.h_*.  2: the pass from there on (kt_chase, behind kt_f2).
template <int USE_F2, int LIVE, int PHASE = 0>
static __device__ __forceinline__ void tc_chaser(const TeamParams& P, const uint32_t g, const int lane, LobbyDev& s_lb, TwScratch& S,
                                                 uint32_t* const s_hf, uint32_t* const s_hfc, LookCtl& K)
{
    uint32_t kseq = 0;                                        // look-ups posted to the helper waves so far
    const uint32_t v_off = (uint32_t)lane < P.M.n_roles ? P.tchains[g].off[lane] : 0u;   // lane r: role r's sub-queue in this pass
    const uint32_t v_len = (uint32_t)lane < P.M.n_roles ? P.tchains[g].len[lane] : 0u;
    TeamChain* const tc = P.tchains + g;
    if (tc->done || tc->qlen == 0u) {
        if (PHASE == 1) return;
        if (lane == 0) { tc->done = 1; tc->n_vis = 0; tc->head = 0; }
        if (lane == 0) pub_st64(&tc->pub_end, (unsigned long long)P.seq << 32);
        return;
    }
    const ModeDev& M = P.M;
    const uint32_t c = P.mode * P.n_groups + g;
    ChainDev* const ch = P.chains + c;
    const size_t qo = (size_t)c * P.capacity, po = (size_t)g * P.pstride;
    const uint32_t m = tc->m, qlen = tc->qlen;
    uint32_t* const bits1 = P.bits[1] + (size_t)g * P.bits_stride;   // the current bitmap
    // the bitmap of the start of the pass: kt_f's copy — or, LIVE, the current one: what this pass takes out lies
    // behind the cursor, and the chaser only ever asks for positions from the cursor on
    const uint32_t* const b0 = P.bits[(LIVE || PHASE == 1) ? 1 : 0] + (size_t)g * P.bits_stride;
    const uint32_t* const fv = P.fv + po;
    uint32_t* const vis = P.vis + po;
    uint32_t fbase = 0, fwait = P.fwait;
    unsigned long long fready = 0;
    const long long t_all0 = (LIVE && P.debug) ? clock64() : 0;
    long long t_chase0 = 0, t_wait = 0, t_hop = 0, t_lk[4] = {0, 0, 0, 0};   // (MM_PAIR_DEBUG: the look-ups — starts, the roles' stretches, the members' records, seats + kills)
    if (PHASE != 1 && lane == 0) pub_st(&tc->pub_pass, tc->passes);

    tw_lobby_copy((uint32_t*)&s_lb, (const uint32_t*)&ch->lobby, lane);
    LobbySum L;
    lsum_load(L, s_lb, M);

    uint32_t nvis = 0, head = 0, n_open = 0, gone = 0, err = 0;
    uint32_t d_late = 0;                              // anchors whose chunk flag did not come (TeamChain.flags_late)
    uint32_t d_fill = 0, d_look = 0, d_nlook = 0;     // MM_PAIR_DEBUG: entries looked at by the stored lobby's fill / by the look-ups, look-ups
    bool changed = false, over = false;
    uint32_t a = TT_NONE;
    if (PHASE == 2) {                                         // the head of the queue has met the stored lobby (kt_f's launch)
        const uint32_t hfl = tc->h_flags;
        a = tc->h_a;
        head = hfl & 1u;
        changed = (hfl & 2u) != 0u;
        over = (hfl & 4u) != 0u;
        gone = tc->h_gone;
        err = tc->h_err;
        d_fill = tc->h_fill;
    } else if (L.n > 0u) {
        if (lane == 0) tc->cp[6] += 1u;
        // The stored lobby meets the queue from its head (LobbyState.get_state, lobby_state.ex:61-104).
        // Normally one window: the anchor in the first team.  After a cancel emptied the lower
        // teams, the first player seated there becomes the anchor (MATCH_CHECK.md section 2.1) and
        // the players behind it are judged by ITS window: collect with the current anchor, seat
        // in queue order until the anchor moves, collect again from there.
        uint32_t nseat = 0, from = 0;
        bool moved = true;
        for (uint32_t stage = 0; stage < MM_MAX_TEAMS && moved && L.n < M.L; ++stage) {
            moved = false;
            uint32_t lo, rng;
            pk_bounds(pk_pack(L.ar, L.ac, tc->rmin, P.eqmask), P.window, lo, rng);
            const uint32_t st = from ? tw_starts(P, g, from - 1u, m, lane) : 0u;
            wave_sync();
            uint32_t dry = 0;
            const uint32_t nf = tlk_lookup(P, g, v_off, v_len, K, kseq, st, L.free, lo, rng, S.pos, 0u, lane, &dry, d_fill);
            if (dry >> 31) err |= MM_ERRF_SYNC_TIMEOUT;
            tw_sort_load(S, nf, P, g, lane);
            const uint32_t at0 = L.at;
            uint32_t k = 0;
            while (k < nf && !moved) {
                if (lsum_seat(L, s_lb, M, S.rat[k], S.con[k], S.slo[k], lane) < 0) err |= MM_ERRF_SEAT_INVARIANT;
                if (lane == 0) { s_hf[nseat] = S.spos[k]; s_hfc[nseat] = S.con[k]; }
                ++nseat;
                ++k;
                if (L.at != at0) moved = true;
            }
            wave_sync();
            if (k) from = S.spos[k - 1u] + 1u;
            if (moved && lane == 0) tc->dbg[7] += 1u;
        }
        wave_sync();
        gone += nseat;
        // the players it took leave the queue, whether it filled or not
        if ((uint32_t)lane < nseat) { S.spos[lane] = s_hf[lane]; S.con[lane] = s_hfc[lane]; }
        wave_sync();
        tq_kill<TQ_ALL | TQ_SQI>(P, g, bits1, S, nseat, lane);
        if (L.n == M.L) {
            // filled by the player at from - 1: emitted right here (s_lb holds it, seated in queue order); the
            // lobby is empty from here on
            if (tc->n_out >= P.out_cap) err |= MM_ERRF_OUT_OVERFLOW;
            else if (lane == 0) tl_write_lobby(P, g, s_lb, tc->n_out, tc->passes);
            wave_sync();
            lobby_clear(s_lb, lane);
            wave_sync();
            lsum_load(L, s_lb, M);
            head = 1;
            changed = true;
            a = tw_succ(b0, from, m, lane);
        } else {
            // everybody was popped against it and it is still open: the pass is over
            changed = nseat > 0u;
            over = true;
        }
    } else a = tw_succ(b0, 0u, m, lane);
    if (PHASE == 1) {
        tw_lobby_copy((uint32_t*)&ch->lobby, (const uint32_t*)&s_lb, lane);
        if (lane == 0) {
            tc->h_a = a;
            tc->h_flags = head | (changed ? 2u : 0u) | (over ? 4u : 0u);
            tc->h_gone = gone;
            tc->h_err = err;
            tc->h_fill = d_fill;
        }
        return;
    }
    {
        // the emitters may start: vis[i]'s lobby is the (n_out + head + i)-th of the chain's tick
        tw_store_wait();                                      // (pub_pass has arrived)
        if (lane == 0) pub_st64(&tc->pub_go, ((unsigned long long)P.seq << 32) | (unsigned long long)(tc->n_out + head));
    }

    if (LIVE && P.debug) t_chase0 = clock64();
    while (!over && a != TT_NONE) {
        if (USE_F2) {
            // two lobbies per round trip while it lasts: a's lobby fills and hands over to F, F's lobby fills and
            // hands over to F2 (kt_f2).  Anything else — a lobby that does not fill, the scan horizon — is left
            // to the single step below, which looks at `a` again.
            for (;;) {
                uint32_t F1, F2;
                tw_sload2(fv + uni(a), P.fv2 + po + uni(a), F1, F2);
                if (!(F1 < TT_UNK && (F2 < TT_UNK || F2 == TT_NONE))) break;
                if (lane == 0) { pub_st(&vis[nvis], a); pub_st(&vis[nvis + 1u], F1); }
                nvis += 2u;
                a = F2;
                if (a == TT_NONE) break;
            }
            if (a == TT_NONE) break;
        }
        // wave-uniform address: the scalar path is the shorter one (LIVE: once the chunk's flag is up)
        const long long h0 = (LIVE && P.debug) ? clock64() : 0;
        uint32_t F = LIVE ? tcf_load(P, g, uni(a), fbase, fready, err, t_wait, lane, fwait) : tw_sload(fv + uni(a));
        const bool flagless = LIVE && F == TT_WAIT;          // no F for this anchor: the look-up below, and the emitter is told
        if (flagless) { F = TT_UNK; ++d_late; }
        if (F < TT_UNK || F == TT_NONE) {
            if (lane == 0) pub_st(&vis[nvis], a);
            ++nvis;
            a = F;
            if (LIVE && P.debug) t_hop += clock64() - h0;
            continue;
        }
        // the lobby `a` opens does not fill within kt_f's horizon: look with the whole wave
        ++d_nlook;
        long long tl0 = (LIVE && P.debug) ? clock64() : 0;
#define TLMARK(K) do { if (LIVE && P.debug) { const long long now = clock64(); t_lk[K] += now - tl0; tl0 = now; } } while (0)
        uint32_t lo, rng;
        pk_bounds(P.tkey[po + a], P.window, lo, rng);
        const uint32_t needs = lobby_needs(M, (P.q_cons[qo + a] >> 16) & 7u);
        const uint32_t st = tw_starts(P, g, a, m, lane);
        wave_sync();
        if (lane == 0) S.pos[0] = a;
        TLMARK(0);
        uint32_t dry = 0;
        // (eight 64-entry steps a trip: the role that runs dry — every pass ends on one — is read to its end)
        const uint32_t nf = 1u + tlk_lookup(P, g, v_off, v_len, K, kseq, st, needs, lo, rng, S.pos, 1u, lane, &dry, d_look);
        if (dry >> 31) err |= MM_ERRF_SYNC_TIMEOUT;
        const bool ok = dry == 0u;
        TLMARK(1);
        tw_sort_load(S, nf, P, g, lane);
        TLMARK(2);
        if (ok) {
            if (lane == 0) pub_st(&vis[nvis], flagless ? (a | TV_LOOKED) : a);
            ++nvis;
            a = tw_succ(b0, S.spos[nf - 1u] + 1u, m, lane);
            continue;
        }
        // it stays open: `a` and everybody it takes are seated, nobody else is queued behind
        err |= tw_replay(s_lb, S, nf, M, lane);
        tq_kill<TQ_ALL>(P, g, bits1, S, nf, lane);
        TLMARK(3);
#undef TLMARK
        n_open = 1;
        changed = true;
        gone += nf;
        over = true;
    }

    tw_lobby_copy((uint32_t*)&ch->lobby, (const uint32_t*)&s_lb, lane);
    if (lane == 0) {
        const uint32_t base = tc->n_out, n_new = head + nvis;
        if (base + n_new > P.out_cap) err |= MM_ERRF_OUT_OVERFLOW;
        PassTally T = {nvis, head, n_open, gone, err, changed, over};
        PassCounts C = {qlen, tc->passes, base, tc->pairs, tc->scanned};
        const uint32_t pass = C.passes;
        const bool done = pass_close(P, g, tc, bits1, T, C, lane);
        tc->out_base = base;
        tc->n_out = C.n_out;
        tc->n_vis = (err & MM_ERRF_OUT_OVERFLOW) ? 0u : nvis;
        tc->head = (err & MM_ERRF_OUT_OVERFLOW) ? 0u : head;
        tc->cur_pass = pass;
        tc->pairs = C.pairs;
        tc->scanned = C.scanned;
        tc->qlen = C.qlen;
        tc->passes = C.passes;
        if (done) tc->done = 1;
        if (err) atomicOr(&tc->err, err);          // (the emitters of this launch report theirs the same way)
        if (d_late) tc->flags_late += d_late;
        tc->cp[LIVE ? 1 : 0] += 1u;
        tc->cp[LIVE ? 4 : 3] += n_new;
        tc->cp[6] += d_nlook;
        if (P.debug) { tc->dbg[0] += d_fill; tc->dbg[1] += d_look; tc->dbg[3] += d_nlook; }
        if (LIVE && P.debug) {   // cycles/16: the whole pass of the chaser, the chase loop alone; passes and lobbies of the live kind
            const long long now = clock64();
            tc->lt[8] += (uint32_t)(t_wait >> 4);
            tc->lt[13] += (uint32_t)(t_hop >> 4);
            tc->lt[9] += (uint32_t)((now - t_all0) >> 4);
            tc->lt[10] += (uint32_t)((now - t_chase0) >> 4);
            tc->lt[11] += 1u;
            tc->lt[12] += nvis;
            for (int q = 0; q < 4; ++q) tc->lt[4 + q] += (uint32_t)(t_lk[q] >> 4);
            tc->lt[3] += d_nlook;
        }
    }
    {
        // the pass is over: how many anchors vis[] holds (the emitters leave when they are past them)
        tw_store_wait();                                      // (every vis[] entry has arrived)
        if (lane == 0) pub_st64(&tc->pub_end, ((unsigned long long)P.seq << 32) | (unsigned long long)((err & MM_ERRF_OUT_OVERFLOW) ? 0u : nvis));
    }
}

// The chase of a lobby-rich pass is a chain of dependent loads of (F, F o F), two lobbies a trip: 480 cycles when the line
// comes from memory (kt_f / kt_f2 wrote it from every XCD), 170 when it is in the chaser's L2.  The chaser's own fifteen waves
// pulling the arrays through that L2 do not get ahead of it: ONE CU brings in ~15 KB a trip, which is as fast as the chaser
// consumes them (measured, rounds 3 and 4).  Other CUs of the chaser's XCD do: the emitter workgroups of the chain that run on it
// — workgroup b runs on XCD (b + c) % 8 (observed, not promised: a wrong guess costs what it costs today, misses) — each pull a
// slice of the chain's F and F o F before they start waiting for lobbies (the chaser spends ~8 us on the stored lobby first).
static __device__ __forceinline__ void tc_pull_xcd(const TeamParams& P, uint32_t eb)
{
    const uint32_t G = P.n_groups, g = eb % G, e = eb / G;
    if ((G * (e + 1u)) & 7u) return;                          // blockIdx.x - g = G (e + 1): not the chaser's XCD
    const TeamChain* const tc = P.tchains + g;
    if (!tc->fast || tc->done || tc->qlen == 0u) return;
    if (tc->passes != 0u && tc->n_vis < 64u) return;          // (a short chase: not worth it)
    uint32_t rank = 0, nsame = 0;
    for (uint32_t x = 0; x < P.n_emit; ++x)
        if (!((G * (x + 1u)) & 7u)) { rank += x < e ? 1u : 0u; ++nsame; }
    const uint4* const f4 = (const uint4*)(P.fv + (size_t)g * P.pstride);
    const uint4* const g4 = (const uint4*)(P.fv2 + (size_t)g * P.pstride);
    const uint32_t n4 = (tc->m + 3u) >> 2, stride = nsame * TC_THREADS;
    uint32_t acc = 0;
    for (uint32_t i = rank * TC_THREADS + threadIdx.x; i < n4; i += 4u * stride) {
        uint4 v[4], w[4];
#pragma unroll
        for (uint32_t u = 0; u < 4u; ++u) {
            const uint32_t k = i + u * stride < n4 ? i + u * stride : i;
            v[u] = f4[k];
            w[u] = g4[k];
        }
#pragma unroll
        for (uint32_t u = 0; u < 4u; ++u) acc ^= v[u].x ^ v[u].y ^ v[u].z ^ v[u].w ^ w[u].x ^ w[u].y ^ w[u].z ^ w[u].w;
    }
    TW_SINK(acc);
}

// what a chaser / emitter workgroup of kt_fc (and the head-fill workgroup of kt_f) keeps where a chunk keeps its member lists
struct TcRoles { LobbyDev lbw[TT_WAVES]; TwScratch Sw[TT_WAVES]; uint32_t hf[MM_MAX_LOBBY], hfc[MM_MAX_LOBBY]; EmitCtl ctl; LookCtl look; };

__global__ __launch_bounds__(TC_THREADS) void kt_chase(TeamParams P)
{
    constexpr int USE_F2 = 1;                     // (kt_chase<0> — a pass without F o F as kt_f | kt_chase — was rounds 2-5's MM_TEAM_LIVE=0; kt_fc is that pass now)
    __shared__ LobbyDev s_lbw[TC_WAVES];          // [0]: the chaser's
    __shared__ TwScratch s_Sw[TC_WAVES];
    __shared__ uint32_t s_hf[MM_MAX_LOBBY], s_hfc[MM_MAX_LOBBY];
    __shared__ EmitCtl s_ctl;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    if (blockIdx.x >= P.n_groups) {
        if (USE_F2 && P.pull_xcd) tc_pull_xcd(P, blockIdx.x - P.n_groups);
        tc_emitter<0>(P, blockIdx.x - P.n_groups, TC_WAVES, wave, lane, s_lbw[wave], s_Sw[wave], s_ctl);
        return;
    }
    const uint32_t g = blockIdx.x;
    const TeamChain* const tc = P.tchains + g;
    if (!tc->fast) return;
    __shared__ LookCtl s_look;
    if (threadIdx.x == 0) s_look.seq = 0;
    if (threadIdx.x < MM_MAX_ROLES) s_look.ack[threadIdx.x] = 0;
    __syncthreads();
    if (wave >= 1 && (uint32_t)wave < P.M.n_roles) {          // the helper waves of the chaser's look-ups, a role each
        tlk_helper(P, g, s_look, (uint32_t)wave, lane);
        return;
    }
    if (threadIdx.x >= 64) {
        // the other waves only pull F through this XCD's L2 (kt_f wrote it from every XCD, so the
        // chase's dependent loads would each go out to HBM): sequential 16-byte reads, discarded
        if (tc->done || tc->qlen == 0u) return;
        // ... when the chase is long enough to pay for it: the last pass's lobby count predicts this one's
        if (tc->passes != 0u && tc->n_vis < 64u) return;
        const uint4* const f4 = (const uint4*)(P.fv + (size_t)g * P.pstride);
        const uint4* const g4 = (const uint4*)(P.fv2 + (size_t)g * P.pstride);
        const uint32_t n4 = (tc->m + 3u) >> 2, w0 = P.M.n_roles, np = (TC_WAVES - w0) * 64u;
        uint32_t acc = 0;
        for (uint32_t i = threadIdx.x - 64u * w0; i < n4; i += np) {
            const uint4 v = f4[i];
            acc ^= v.x ^ v.y ^ v.z ^ v.w;
            if (USE_F2) { const uint4 v2 = g4[i]; acc ^= v2.x ^ v2.y ^ v2.z ^ v2.w; }
        }
        TW_SINK(acc);
        return;
    }
    if (USE_F2 && P.hf_x != 0xFFFFFFFFu) tc_chaser<USE_F2, 0, 2>(P, g, lane, s_lbw[0], s_Sw[0], s_hf, s_hfc, s_look);
    else tc_chaser<USE_F2, 0>(P, g, lane, s_lbw[0], s_Sw[0], s_hf, s_hfc, s_look);
    if (lane == 0) lds_st(&s_look.seq, TLK_EXIT);             // the helper waves may go
}

// ------------------------------------------------------------------------------------
// kt_f: grid (chunks [+ 1], rating groups).  The extra column (TeamParams.hf_x, the lobby-rich passes) fills the chains' stored
// lobbies from the heads of their queues while the chunks work — the first 8 us of a chase that needs nothing of F.
// ------------------------------------------------------------------------------------
__global__ __launch_bounds__(TT_CH) MM_WAVES_PER_SIMD(8) void kt_f(TeamParams P)
{
    __shared__ uint16_t s_tmp[MM_MAX_LOBBY - 1u][TT_CH];
    static_assert(sizeof(TcRoles) <= sizeof(s_tmp), "the head-fill workgroup's lobby lives in kt_f's member lists");
    if (blockIdx.x == P.hf_x) {
        TcRoles& R = *reinterpret_cast<TcRoles*>(&s_tmp[0][0]);
        const uint32_t g = blockIdx.y;
        const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
        if (!((P.act >> g) & 1u) || !P.tchains[g].fast) return;
        if (threadIdx.x == 0) R.look.seq = 0;
        if (threadIdx.x < MM_MAX_ROLES) R.look.ack[threadIdx.x] = 0;
        __syncthreads();
        if (wave == 0) {
            tc_chaser<0, 0, 1>(P, g, lane, R.lbw[0], R.Sw[0], R.hf, R.hfc, R.look);
            if (lane == 0) lds_st(&R.look.seq, TLK_EXIT);      // the helper waves may go
        } else if ((uint32_t)wave < P.M.n_roles) tlk_helper(P, g, R.look, (uint32_t)wave, lane);
        return;
    }
    tf_chunk<0>(P, blockIdx.y, blockIdx.x, s_tmp);
}

// ------------------------------------------------------------------------------------
// kt_fc: kt_f and the chase of a pass in ONE launch (the passes without kt_f2).  Workgroups [0, n_groups): the chasers;
// then kt_f's chunks (TeamParams.fo_*: by falling distance to the end of their chain); then n_emit emitter
// workgroups per chain (if any).  A chaser takes F[a] once the flag of a's chunk is up (tcf_load), so the chase of
// a pass runs beside kt_f instead of behind it: a pass costs about max(kt_f, chase) instead of their sum plus a
// launch boundary.  Exactness: the chaser reads what it always reads; what it writes while kt_f is still at work —
// the players the stored lobby and the lobby left open at the end take out of the queue (and, with emitters, the
// members of emitted lobbies) — lies behind the cursor or is met by no anchor this pass still visits, and
// kt_f's record of an anchor stays valid under any bitmap between the start and the end of the pass: its members
// are the first ones that fit among players it SAW queued, and whoever it saw gone stays gone.
// ------------------------------------------------------------------------------------
#ifndef KT_FC_WPS
#define KT_FC_WPS 6
#endif
__global__ __launch_bounds__(TT_CH) MM_WAVES_PER_SIMD(KT_FC_WPS) void kt_fc(TeamParams P)
{
    // a workgroup is a chaser, an emitter or a kt_f chunk: the first two keep their lobbies where the third keeps its
    // member lists.  (Measured: capping the kernel at 64 registers so that four workgroups fit a CU instead of three
    // changes nothing — 10.24 against 10.22 ms per cfg-3 tick.)
    typedef TcRoles Roles;
    __shared__ uint16_t s_tmp[MM_MAX_LOBBY - 1u][TT_CH];
    static_assert(sizeof(Roles) <= sizeof(s_tmp), "the chaser's / emitters' lobbies live in kt_f's member lists");
    Roles& R = *reinterpret_cast<Roles*>(&s_tmp[0][0]);
    LobbyDev* const s_lbw = R.lbw;
    TwScratch* const s_Sw = R.Sw;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    // Order of the workgroups: the chasers, kt_f's chunks, the emitters.  The chasers wait for chunks and the emitters
    // for the chasers; nobody who waits may keep the one he waits for off the chip, so only the chasers — one workgroup
    // per chain — stand in front of the chunks (the emitters did at first: with enough of them, or a few engines on one
    // device, they fill the CUs while kt_f's chunks queue behind them, and the launch ends in its time-outs).
    // The shim of the tests runs workgroups one after another: chunks, chasers, emitters there.
    const uint32_t G = P.n_groups, C = P.fo_start[P.fo_n];
    uint32_t role, k;                                          // 0 chaser, 1 chunk, 2 emitter; index within the role
    if (MM_WAITERS_FIRST) {
        if (blockIdx.x < G) { role = 0; k = blockIdx.x; }
        else if (blockIdx.x < G + C) { role = 1; k = blockIdx.x - G; }
        else { role = 2; k = blockIdx.x - G - C; }
    } else {
        if (blockIdx.x < C) { role = 1; k = blockIdx.x; }
        else if (blockIdx.x < C + G) { role = 0; k = blockIdx.x - C; }
        else { role = 2; k = blockIdx.x - C - G; }
    }
    if (role == 0) {
        if (!P.tchains[k].fast) return;
        if (threadIdx.x == 0) R.look.seq = 0;
        if (threadIdx.x < MM_MAX_ROLES) R.look.ack[threadIdx.x] = 0;
        __syncthreads();
        if (wave == 0) {
            tc_chaser<0, 1>(P, k, lane, s_lbw[0], s_Sw[0], R.hf, R.hfc, R.look);
            if (lane == 0) lds_st(&R.look.seq, TLK_EXIT);      // the helper waves may go
        } else if ((uint32_t)wave < P.M.n_roles) tlk_helper(P, k, R.look, (uint32_t)wave, lane);   // the chaser's look-ups, a role each
        return;
    }
    if (role == 2) {
        tc_emitter<1>(P, k, TT_WAVES, wave, lane, s_lbw[wave], s_Sw[wave], R.ctl);
        return;
    }
    uint32_t sg = 0;
    while (sg + 1u < P.fo_n && k >= P.fo_start[sg + 1u]) ++sg;
    const uint32_t kk = k - P.fo_start[sg], dist = P.fo_dhi[sg] - kk / (sg + 1u), j = kk % (sg + 1u);
    tf_chunk<1>(P, P.fo_chain[j], P.fo_nch[j] - dist, s_tmp);
}

// ------------------------------------------------------------------------------------
// kt_late: the passes of a chain that emit only a handful of lobbies each, back to back in ONE launch,
// one workgroup per rating group.
//
// Late in a tick (and in every tick of a stream whose pool starves: BASELINE cfg-5 after a minute) a pass of
// a 150 000-player chain visits ten anchors, and a pass kernel (kt_f over every position, the chase beside it)
// costs ~50 us for them.  With kt_f's lobby records the whole of F is not needed there: the chaser
// (wave 0) looks at the anchors the cursor really visits —
//     record of the anchor (fv / fpos / memb: one trip to memory) -> are all members still queued?  (bitmap
//     in LDS) -> the lobby is the recorded one: hand it to an emitter wave, take its players out of the LDS
//     bitmap, cursor = first queued position behind the last member (LDS scan)
// and only when a member has left (or no record exists) looks the lobby up itself, role by role, in the
// sub-queues of the last kt_build (entries of players that left since are skipped by the LDS bitmap; nobody
// writes tombstones here: the chain is walked to its end in this launch and the next tick rebuilds).
// Waves 1.. take the lobbies from an LDS ring: the players' records, the seats replayed in queue order
// (the team choice needs the order: lsum_seat, as kt_emit), the lobby written, the chunk populations.
// What a pass does around the chase: head_fill and open_lobby_close (tc_chaser's rules over the LDS bitmap, QvLate) and
// pass_close, the one tc_chaser calls.  The bitmap goes back to HBM once, at the end.
// Exactness: a pass only takes players out BEHIND the cursor (a lobby's members all lie before the next
// anchor), so the current bitmap is, for everything the pass still looks at, the bitmap of its start.
// ------------------------------------------------------------------------------------
#define TL_THREADS 512
#define TL_WAVES (TL_THREADS / 64)
#define TL_RING 32u
#ifndef TL_BITS_MAX
#define TL_BITS_MAX (1u << 20)       // positions of a chain whose bitmap fits the workgroup's LDS (128 KB)
#endif
struct TlJob { uint32_t seq, n, idx, pass, pos[MM_MAX_LOBBY]; };

__global__ __launch_bounds__(TL_THREADS) void kt_late(TeamParams P)
{
    __shared__ uint32_t s_bits[TL_BITS_MAX / 32u + 64u];     // zero padded: l_succ reads 64 words a step
    __shared__ TlJob s_ring[TL_RING];
    __shared__ LobbyDev s_lbw[TL_WAVES];                     // [0]: the chain's open lobby (the chaser's)
    __shared__ TwScratch s_Sw[TL_WAVES];
    __shared__ uint32_t s_ticket, s_produced, s_fin, s_err;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const uint32_t g = blockIdx.x;
    TeamChain* const tc = P.tchains + g;
    if (!tc->fast || tc->done || tc->m > TL_BITS_MAX) return;
    const ModeDev& M = P.M;
    const uint32_t c = P.mode * P.n_groups + g;
    ChainDev* const ch = P.chains + c;
    const size_t qo = (size_t)c * P.capacity, po = (size_t)g * P.pstride;
    const uint32_t m = tc->m, nr = M.n_roles, LM = M.L - 1u;
    uint32_t* const gbits = P.bits[1] + (size_t)g * P.bits_stride;
    {
        const uint32_t nwords = (m + 31u) >> 5;
        for (uint32_t i = tid; i < TL_BITS_MAX / 32u + 64u; i += TL_THREADS) s_bits[i] = i < nwords ? gbits[i] : 0u;
        if ((uint32_t)tid < TL_RING) s_ring[tid].seq = (uint32_t)tid;
        if (tid == 0) { s_ticket = 0; s_produced = 0; s_fin = 0; s_err = 0; }
    }
    __syncthreads();
    LobbyDev& s_lb = s_lbw[wave];
    TwScratch& S = s_Sw[wave];

    if (wave == 0) {
        // ---------------- the chaser: pass after pass (head_fill, the chase below, open_lobby_close, pass_close) ----------------
        tw_lobby_copy((uint32_t*)&s_lb, (const uint32_t*)&ch->lobby, lane);
        LobbySum L;
        lsum_load(L, s_lb, M);
        PassCounts C = {tc->qlen, tc->passes, tc->n_out, tc->pairs, tc->scanned};   // in registers across the passes, stored once
        const uint32_t passes0 = C.passes, n_out0 = C.n_out;
        uint32_t err = 0, rk = 0;
        uint32_t rlen[MM_MAX_ROLES], roff[MM_MAX_ROLES];       // the sub-queues of the last kt_build: fixed for this launch
#pragma unroll
        for (uint32_t r = 0; r < MM_MAX_ROLES; ++r) { rlen[r] = r < nr ? tc->len[r] : 0u; roff[r] = r < nr ? tc->off[r] : 0u; }
        bool done = C.qlen == 0u, bailed = false;
        // MM_PAIR_DEBUG: what the chaser did and where its time went (TeamChain.lt)
        uint32_t d_rec = 0, d_look = 0, d_open = 0, d_fill = 0, d_sc[MM_MAX_ROLES] = {0, 0, 0, 0, 0, 0, 0, 0};
        long long c_rec = 0, c_look = 0, c_fill = 0, c_ring = 0;
        const long long c_all0 = clock64();
        if (P.debug && lane == 0) tc->lt[15] = C.passes;
        QvLate V = {P, g, s_bits, rlen, roff, d_sc};
        while (!done) {
            PassTally T = {0u, 0u, 0u, 0u, err, false, false};
            uint32_t a = TT_NONE;
            if (L.n > 0u) {
                const long long c0 = clock64();                 // (MM_PAIR_DEBUG, lt[12]: the fill with its emission on the spot)
                ++d_fill;
                a = head_fill(V, tc, L, s_lb, S, m, &C.n_out, &C.passes, T, lane);
                c_fill += clock64() - c0;
            } else a = V.succ(0u, m, lane);

            while (!T.over && a != TT_NONE) {
                // Everything that depends on `a` alone is asked for in ONE trip: its record (lane 0 F, lane 1 the last
                // member, lanes 2.. the members' distances) and — wanted only when the record turns out stale — its key
                // and what places it in the role sub-queues (tw_starts: the 64-block's entries and roles, the ranks
                // in front of the block).
                const long long c1 = clock64();
                uint32_t v = 0;
                if (lane == 0) v = P.fv[po + a];
                else if (lane == 1) v = P.fpos[po + a];
                else if ((uint32_t)lane < LM + 2u) v = P.memb[(po + a) * LM + (uint32_t)lane - 2u];
                const uint32_t blk = a >> 6, bpos = (blk << 6) + (uint32_t)lane;
                const uint32_t bwB = P.bitsB[(size_t)g * P.bits_stride + (bpos >> 5)];
                const uint32_t bcn = P.q_cons[qo + (bpos < m ? bpos : a)];
                const uint32_t bbs = (uint32_t)lane < nr ? P.blkbase[po + (size_t)lane * P.blk_stride + blk] : 0u;
                const uint32_t akey = P.tkey[po + a];
                const uint32_t F = lane_get(v, 0), fp = lane_get(v, 1);
                bool have = false;
                uint32_t nf = 1, last = a;
                if (F != TT_PART && F != TT_UNK && fp != TT_NONE) {
                    const bool mine = lane >= 2 && (uint32_t)lane < LM + 2u;
                    const uint32_t mp = a + v;
                    const bool dead = mine && (mp >= m || !l_alive(s_bits, mp));
                    if (!__ballot(dead)) {
                        if (lane == 0) S.pos[0] = a;
                        if (mine) S.pos[lane - 1] = mp;
                        nf = M.L;
                        last = fp;
                        have = true;
                    }
                }
                c_rec += clock64() - c1;
                if (have) ++d_rec;
                if (!have) {
                    // no record, or a member has left: look with the whole wave (kt_chase's own look-up), all roles abreast
                    const long long c2 = clock64();
                    ++d_look;
                    uint32_t lo, rng;
                    pk_bounds(akey, P.window, lo, rng);
                    const bool inB = bpos < m && ((bwB >> (bpos & 31u)) & 1u);       // tw_starts on what trip one brought
                    const uint32_t brole = inB ? (bcn >> 16) & 7u : 0u;
                    const uint32_t arole = (lane_get(bcn, (int)(a & 63u)) >> 16) & 7u;
                    const unsigned long long le = (2ull << (a & 63u)) - 1ull;
                    uint32_t st = 0;
                    for (uint32_t r = 0; r < nr; ++r) {
                        const unsigned long long mk = __ballot(inB && brole == r);
                        const uint32_t base = lane_get(bbs, (int)r);
                        if ((uint32_t)lane == r) st = base + (uint32_t)__popcll(mk & le);
                    }
                    wave_sync();
                    if (lane == 0) S.pos[0] = a;
                    uint32_t dry = 0;
                    nf += V.lookup(st, lobby_needs(M, arole), lo, rng, S.pos, 1u, lane, &dry);
                    const bool ok = dry == 0u;
                    wave_sync();
                    c_look += clock64() - c2;
                    if (!ok) {
                        ++d_open;
                        tw_sort_load(S, nf, P, g, lane);
                        open_lobby_close(V, s_lb, S, nf, T, lane);
                        wave_sync();
                        lsum_load(L, s_lb, M);                   // (the next pass begins with it)
                        break;
                    }
                    uint32_t mx = (uint32_t)lane < nf ? S.pos[lane] : 0u;
                    for (int dd = 1; dd < 64; dd <<= 1) { const uint32_t o2 = (uint32_t)__shfl((int)mx, lane ^ dd); mx = o2 > mx ? o2 : mx; }
                    last = mx;
                }
                // the lobby fills: an emitter wave seats and writes it; its players are behind the cursor from here on
                if (C.n_out + T.head + T.nvis >= P.out_cap) { T.err |= MM_ERRF_OUT_OVERFLOW; T.over = true; break; }
                wave_sync();
                {
                    TlJob& J = s_ring[rk % TL_RING];
                    const long long c3 = clock64();
                    while (uni(lds_ld(&J.seq)) != rk) __builtin_amdgcn_s_sleep(1);
                    c_ring += clock64() - c3;
                    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
                    if ((uint32_t)lane < nf) {
                        const uint32_t pos = S.pos[lane];
                        J.pos[lane] = pos;
                        tq_leave<TQ_BITS>(P, g, s_bits, pos, 0u, 0u);      // (the chunk populations: the emitter, which has the roles)
                    }
                    if (lane == 0) { J.n = nf; J.idx = C.n_out + T.head + T.nvis; J.pass = C.passes; }
                    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
                    wave_lockstep();
                    if (lane == 0) lds_st(&J.seq, rk + 1u);
                    ++rk;
                }
                ++T.nvis;
                a = V.succ(last + 1u, m, lane);
            }

            const uint32_t n_new = T.head + T.nvis;
            done = pass_close(P, g, tc, s_bits, T, C, lane);
            wave_sync();                                      // (the head's bit, if pass_close put it back)
            err = T.err;
            // a pass that seats many lobbies after all (a newcomer unblocked a cascade): back to the pass kernels,
            // which look lobbies up for everybody at once — the host rebuilds the sub-queues first (no tombstones here)
            if (!done && n_new > P.late_bail) { bailed = true; break; }
        }
        if (lane == 0) { lds_st(&s_produced, rk); lds_st(&s_fin, 1u); }
        tw_lobby_copy((uint32_t*)&ch->lobby, (const uint32_t*)&s_lb, lane);
        if (lane == 0) {
            tc->n_out = C.n_out;
            tc->n_vis = 0;
            tc->head = 0;
            tc->out_base = C.n_out;
            tc->cur_pass = C.passes;
            tc->pairs = C.pairs;
            tc->scanned = C.scanned;
            tc->qlen = C.qlen;
            tc->passes = C.passes;
            tc->done = bailed ? 0u : 1u;
            tc->cp[2] += C.passes - passes0;
            tc->cp[5] += C.n_out - n_out0;
            tc->cp[7] += d_look + d_fill;
            if (err) atomicOr(&s_err, err);
            if (P.debug) {
                tc->lt[0] = C.passes - tc->lt[15]; tc->lt[1] = d_rec; tc->lt[2] = d_look; tc->lt[3] = d_open; tc->lt[4] = d_fill;
#pragma unroll
                for (uint32_t r = 0; r < 5u; ++r) tc->lt[5u + r] = d_sc[r];      // (unrolled: the counters stay in registers)
                tc->lt[10] = (uint32_t)(c_rec >> 4); tc->lt[11] = (uint32_t)(c_look >> 4); tc->lt[12] = (uint32_t)(c_fill >> 4);
                tc->lt[13] = (uint32_t)((clock64() - c_all0) >> 4); tc->lt[14] = (uint32_t)(c_ring >> 4);
            }
        }
    } else {
        // ---------------- emitters: one lobby per ticket (emit_members, as te_emit_one for a lobby on record) ----------------
        uint32_t err = 0;
        for (;;) {
            uint32_t t = 0;
            if (lane == 0) t = atomicAdd(&s_ticket, 1u);
            t = lane_get(t, 0);
            TlJob& J = s_ring[t % TL_RING];
            bool stop = false;
            while (uni(lds_ld(&J.seq)) != t + 1u) {
                if (uni(lds_ld(&s_fin)) && t >= uni(lds_ld(&s_produced))) { stop = true; break; }
                __builtin_amdgcn_s_sleep(2);
            }
            if (stop) break;
            __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
            const uint32_t nf = J.n, idx = J.idx, pass = J.pass;
            if ((uint32_t)lane < nf) S.pos[lane] = J.pos[lane];
            __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
            wave_lockstep();
            if (lane == 0) lds_st(&J.seq, t + TL_RING);          // the slot is free again
            lobby_clear(s_lb, lane);
            err = emit_members<TQ_CHUNK>(P, g, s_lb, S, nf, idx, pass, err, nullptr, lane);   // (the chaser took them out of the bitmap)
            wave_sync();
        }
        if (err && lane == 0) atomicOr(&s_err, err);
    }
    __syncthreads();
    {   // the bitmap goes back once (kt_fin_scatter reads it)
        const uint32_t nwords = (m + 31u) >> 5;
        for (uint32_t i = tid; i < nwords; i += TL_THREADS) gbits[i] = s_bits[i];
        if (tid == 0 && s_err) atomicOr(&tc->err, s_err);
    }
}

// ------------------------------------------------------------------------------------
// kt_fin_scatter / kt_fin_copy: survivors back into the chain's q_* arrays, queue order
// preserved (= requeue order, worker.ex:239-248), and the tick counters.
// ------------------------------------------------------------------------------------
__global__ __launch_bounds__(TT_CH) void kt_fin_scatter(TeamParams P)
{
    __shared__ uint32_t s_base, s_wc[TT_WAVES];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const uint32_t g = blockIdx.y, cb = blockIdx.x;
    TeamChain* const tc = P.tchains + g;
    if (!tc->fast) return;
    const uint32_t m = tc->m, nch = (m + TT_CH - 1u) / TT_CH;
    if (cb >= nch) return;
    const size_t qo = ((size_t)P.mode * P.n_groups + g) * P.capacity, po = (size_t)g * P.pstride;
    if (tid == 0) s_base = 0;
    __syncthreads();
    const uint32_t* const chunk = P.chunk + (size_t)g * MM_MAX_ROLES * P.chunk_stride;
    uint32_t pb = 0;
    for (uint32_t r = 0; r < P.M.n_roles; ++r)
        for (uint32_t k = tid; k < cb; k += TT_CH) pb += chunk[(size_t)r * P.chunk_stride + k];
    pb = wave_sum(pb, lane);
    if (lane == 0 && pb) atomicAdd(&s_base, pb);
    const uint32_t pos = cb * TT_CH + (uint32_t)tid;
    const uint32_t* const b1 = P.bits[1] + (size_t)g * P.bits_stride;
    const bool alive = pos < m && ((b1[pos >> 5] >> (pos & 31u)) & 1u);
    const unsigned long long mk = __ballot(alive);
    if (lane == 0) s_wc[wave] = (uint32_t)__popcll(mk);
    __syncthreads();
    uint32_t off = s_base, tot = 0;
    for (int w = 0; w < (int)TT_WAVES; ++w) {
        if (w < wave) off += s_wc[w];
        tot += s_wc[w];
    }
    if (alive) {
        const uint32_t d = off + (uint32_t)__popcll(mk & ((1ull << lane) - 1ull));
        P.sqk[po + d] = (uint32_t)P.q_rating[qo + pos];
        P.sqp[po + d] = P.q_cons[qo + pos];
        P.fv[po + d] = P.q_slot[qo + pos];
    }
    if (cb == nch - 1u && tid == 0 && s_base + tot != tc->qlen) atomicOr(&tc->err, (uint32_t)MM_ERRF_SEAT_INVARIANT);
}

__global__ __launch_bounds__(TT_CH) void kt_fin_copy(TeamParams P)
{
    const int tid = threadIdx.x;
    const uint32_t g = blockIdx.y, cb = blockIdx.x;
    const TeamChain* const tc = P.tchains + g;
    if (!tc->fast) return;
    const uint32_t c = P.mode * P.n_groups + g;
    const size_t qo = (size_t)c * P.capacity, po = (size_t)g * P.pstride;
    const uint32_t i = cb * TT_CH + (uint32_t)tid;
    if (i < tc->qlen) {
        P.q_rating[qo + i] = (int32_t)P.sqk[po + i];
        P.q_cons[qo + i] = P.sqp[po + i];
        P.q_slot[qo + i] = P.fv[po + i];
    }
    if (cb == 0u && tid == 0) {
        ChainDev* const ch = P.chains + c;
        ch->len = tc->qlen;
        ch->head_state = 0;
        ch->purged = 0;
        ch->before = tc->before;
        ch->n_out = tc->n_out;
        ch->passes = tc->passes;
        ch->pairs = tc->pairs;
        ch->scanned = tc->scanned;
        ch->err |= tc->err | (tc->done ? 0u : MM_ERRF_PASS_LIMIT);
    }
}
