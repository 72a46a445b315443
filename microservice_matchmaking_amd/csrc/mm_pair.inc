// mm_pair.inc — the pair (1v1) fast path of the search walk.  Included by mm_engine.hip.
//
// Same semantics as k_walk (Search.Worker.consume/5 to quiescence under the schedule of
// docs/MATCH_CHECK.md §4), restricted to modes with team_size 1 / teams 2 (cancel ticks
// included: k_purge + the stale-lobby rule in kp_init).  For such a mode the open lobby holds
// at most ONE player (the anchor) and
// match_check (MATCH_CHECK.md §2) is a symmetric predicate fit(anchor, candidate), so the
// walk is a cursor over the FIFO queue:
//
//     anchor a = first queued player at/after the cursor      (seated: worker.ex:320 save)
//     partner j = first queued player after a that fits a      (worker.ex:296-306, :313-319)
//     emit (a, j); cursor = j + 1; a pass ends when the cursor runs off the queue
//
// The chain of (a, j) steps is sequential, but "first queued player after i that fits i" —
// next[i] — is a masked arg-min over queue position that is data parallel over i, and it
// only ever becomes stale when next[i] itself leaves the queue (everything between i and
// next[i] was rejected by i once and stays rejected).  So the pair path keeps next[] for
// every queued player (computed by all CUs, repaired incrementally) and the cursor walk
// degenerates to pointer chasing:  a -> next[a] -> first alive after it -> ...
//
// Data (per rating group, HBM resident, index space = queue order at the start of the tick):
//   key[i]   u32  filter bits << 19 | (rating - rmin): "fits the anchor" is one interval test
//                 on the whole word (pk_bounds / pk_in); bit 31 = left the queue (LDS copies)
//   oidx[i]  u32  index of the player in the chain's q_* arrays (for slot / rating / cons)
//   nx16[i]  u16  forward offset of next[i]; 0 = not computed, 0xFFFF = none to the end of
//                 the queue, 0xFFFE = none inside the scan horizon
//   bits     1 bit per index: still queued
//
// Kernels:  kp_init (rating span, eligibility, anchor), kp_pack (key/oidx/bits),
//           kp_nx_init (next[] for everybody, all CUs),
//           kp_round (long chains: one launch per pass; every tile's workgroup walks the route,
//           applies the pass to its tile and prepares it for the next one),
//           kc_* (compaction of long chains), kp_late (one workgroup per chain, the whole
//           chain LDS resident: one wave chases pointers 64 steps blind, one takes the players out of the
//           bitmap, one emits the lobbies, thirteen repair next[]),
//           kp_finish (survivors back to the q_* arrays, ChainDev counters).

#define PK_NO 0xFFFFFFFFu
#define PK_ABORT 0xFFFFFFFEu

#define NX_INV 0u
#define NX_NONE 0xFFFFu
#define NX_FAR 0xFFFEu

// Geometry.  The test build under tests/emu also compiles a second library with tiny values so
// that small pools exercise tiles, routing and compaction on the CPU shim.
#ifndef PK_T
#define PK_T 8192u                   // the LARGEST tile of the tiled path (index positions)
#endif
// The fused tiled path (kp_round and what it calls, the compaction kernels) is compiled for three tile
// lengths, PK_TMAX, PK_TMAX / 2 and PK_TMAX / 4: the host picks, batch by batch, the smallest one that keeps
// the longest chain within PK_TILES_MAX tiles — a pass costs one dependent load per tile in the walk plus
// work proportional to the tile in every workgroup, and the chains shrink by an order of magnitude during
// a tick.  Inside those templates PK_T is the tile length of the instantiation; everywhere else it is PK_TMAX.
enum : uint32_t { PK_TMAX = PK_T };
#undef PK_T
static constexpr uint32_t PK_T = PK_TMAX;
#ifndef PK_TILES_MAX
#define PK_TILES_MAX 40u
#endif
#define PK_XSEG 4u                   // chains that can share one XCD in kp_round's workgroup map
#ifndef PK_GS
#define PK_GS 8u                     // tiles per group of the route's second level (kp_group)
#endif
#ifndef PK_GROUP_MIN
#define PK_GROUP_MIN 64u             // tiles of the longest chain from which a batch runs with the second level
#endif
#ifndef PL_MAX
#define PL_MAX 16384u                // kp_late takes chains SHORTER than this (LDS resident; one index is a sentinel)
#endif
#define PL_THREADS 1024
#define PL_WORDS (PL_MAX / 32u)
#ifndef PL_COMPACT_MIN
#define PL_COMPACT_MIN 2048u
#endif
#define LNX_NONE 0xFFFFu
#define LNX_INV 0xFFFEu
#define PS_TILED 0u
#define PS_LATE 1u
#define PS_DONE 2u
#define TC_ENT 0u                    // tilectl rows: entry position of the round (PK_NO: not on the path)
#define TC_OFF 1u                    // emission offset of the tile's first match
#define TC_DISP 2u                   // what happens to the tile's exit anchor
#define TC_ALIVE 3u                  // queued players in the tile
#define TC_BASE 4u                   // compaction: new index of the tile's first survivor
#define TC_N 5u
#define DISP_NONE 0xFFFFFFFFu        // the path leaves the tile with an empty lobby
#define DISP_SEATED 0xFFFFFFFEu      // the exit anchor stays in the lobby (no partner until the end)
#define REC_CLEAN 0u
#define REC_PARTNER 1u
#define REC_FAR 2u
#define REC_NONE 3u
#define EV_NONE 0u
#define EV_DONE 1u
#define EV_COMPACT 2u

// What a pass of the fused tiled path (kp_round) hands to the next one.  Two copies per chain,
// indexed by launch parity: every workgroup reads one and (only tile 0) writes the other.
struct RoundState {
    uint32_t live;         // still walked by tiled rounds in this batch
    uint32_t done;         // quiescent or empty: the tick is over for this chain
    uint32_t want_compact, rounds;
    uint32_t qlen, passes, n_out, has_anchor;
    uint32_t a_key, a_slot, a_cons, a_team;
    int32_t  a_rating;
    uint32_t pos0;         // first pass of a cancel tick: the head was already judged (MATCH_CHECK.md §4)
    uint32_t changed0, extra0;
    uint32_t a_oi;         // kp_rounds: the anchor's index in the chain's q_* arrays while a_slot / a_rating / a_cons have
                           //   not been fetched (PK_NO: they are valid)
    unsigned long long pairs, scanned;
};

// PairChain.dbg[]: what kp_late counted in the tick (late_store writes them; report_pair and path_stats_pair read them)
enum : uint32_t {
    PD_STALE = 0,          // careful steps whose next[] pointed at a player who had left
    PD_INV = 1,            // ... whose next[] was unknown
    PD_SLOWSUCC = 2,       // careful steps
    PD_COMPACT = 3,        // compactions inside the kernel
    PD_FIXED = 4,          // repairs done by wave 3
    PD_CLK = 5,            // the chaser: shader-clock cycles
    PD_WALL = 6,           // ... and 100 MHz ticks
    PD_WRAPC = 7           // ... of the cycles, the carried anchor's scans from the head of the queue
};

struct PairChain {
    uint32_t fast;         // 1 = this chain is walked by the pair path this tick
    uint32_t m;            // index-space length
    uint32_t qlen;         // queued players (set bits)
    uint32_t buf;          // current key/oidx buffer
    int32_t  rmin;
    uint32_t has_anchor;   // the open lobby holds a player
    uint32_t a_key, a_slot, a_cons, a_team;
    int32_t  a_rating;
    uint32_t passes, n_out, before, err;
    uint32_t pos0;         // cancel tick: the first pass starts here (1: the head met the stale lobby already)
    uint32_t changed0;     // ... and that attempt already changed the lobby
    uint32_t extra0;       // ... and took the head out of the queue (it is the anchor now)
    unsigned long long pairs, scanned;
    unsigned long long tested;   // diagnostics (MM_PAIR_TUNE bit 13): predicate tests the kernels physically performed
    unsigned long long tested_nx;   // ... of them in kp_nx_init
    uint32_t dbg[8];       // diagnostics (MM_PAIR_DEBUG): PD_* above
    // tiled path
    uint32_t stage;        // PS_TILED: walked by the tile kernels; PS_LATE: fits kp_late; PS_DONE
    uint32_t ntiles;
    uint32_t want_compact; // route asks the host for a compaction before the next batch
    uint32_t cur_pass;     // pass number of the round being applied
    uint32_t new_m;        // compaction: index-space length after it
    uint32_t rounds;       // tiled rounds walked (diagnostics)
    uint32_t ghops;        // hops of tile 0's walks that took a whole group of tiles (diagnostics, kp_group)
    uint32_t gtry, gstale; // ... entries it looked at / that were not of the round
    uint32_t tm[16];       // diagnostics: cycles per kernel phase, accumulated over the rounds (tile 1)
    uint32_t pfail;        // kp_rounds: 0, or why the persistent launch gave up (PF_* | iteration << 8); the host then walks
                           //   on with one launch per pass (kp_round) — the chain's state is committed either way
    uint32_t ppass;        // kp_rounds: passes walked inside persistent launches (diagnostics)
    uint32_t pxm;          // kp_rounds: the XCDs (HW_REG_XCC_ID bits) the chain's workgroups of the last launch ran on (diagnostics)
    uint32_t pslow[4];     // kp_rounds, tile 1's walker: hops that left the fast path because the exit anchor's partner had left
                           //   (rescans over the chain's keys in memory), their cycles / 16, hops on REC_FAR, their cycles / 16
    uint32_t ptm[16];      // kp_rounds: cycles per phase (tile 1): 0 barrier, 3 lookahead refresh, 6 walk beside the first sweep, 9 apply,
                           //   1 / 12 / 2 repair (detect, items, far items), 7 / 8 / 10 tables, 4 head scan + arrival, 5 passes, 13 / 15 walk loop
    RoundState rs[2];
};

struct PairParams {
    uint32_t mode, n_groups, capacity, window, eqmask;
    uint32_t out_slot_stride, out_rec_stride, bits_stride;
    uint32_t pstride;                   // elements per group in the pair arrays (capacity rounded up to 64)
    uint32_t tune;                      // MM_PAIR_TUNE: bits 0-3 repair waves off (15 = none), 4-11 sleep
    uint32_t purge;                     // a cancel is pending: k_purge ran, ChainDev.head_state is valid
    uint8_t* state;                     // ActiveUser mirror
    uint32_t* released;                 // slots the liveness filter released
    uint32_t* n_released;
    ChainDev* chains;
    PairChain* pchains;                 // [n_groups]
    int32_t* q_rating;                  // [chain][capacity]
    uint32_t* q_cons;
    uint32_t* q_slot;
    uint32_t* key[2];                   // [group][capacity]
    uint32_t* oidx[2];
    uint16_t* nx16[2];
    uint32_t* bits[2];                  // [group][bits_stride]
    uint32_t* scratch;                  // [group][capacity]: REC of the tiled path, staging of kp_finish
    uint16_t* g16;                      // [group][capacity]: tiled path, next anchor inside the tile
    // fused tiled path (kp_round): what workgroups read from each other, double buffered by parity
    uint32_t* rec2[2];                  // [group][pstride]  REC
    uint16_t* exa[2];                   // [group][pstride]  exit anchor of every entry
    uint32_t* bitsp[2];                 // [group][bits_stride]  queue bitmap at the start of the pass
    uint32_t* headp[2];                 // [group][max_tiles]  first fit of the carried anchor per tile
    uint4* grec;                        // [group][pstride / PK_GS ...]  second level of the route (kp_group): per group of PK_GS tiles,
                                        //   for every entry into its first two tiles: where the cursor leaves the group, the lobbies on the way
    uint32_t grp;                       // tiles per group of the batch's second route level (0: one level)
    // kp_round's workgroup -> (rating group, tile) map of the batch.  Dispatch is round robin over the XCDs (block b runs
    // on XCD b % 8: observed, not promised — a wrong guess only costs cache misses), and every XCD has an L2 of its own:
    // with the tiles of ONE chain on one XCD (two for the longest) that L2 holds one chain's route tables instead of
    // every chain's, and the walk's dependent loads hit it.  xseg[x][k] = g | phase << 8 | stride << 16, xcnt[x][k] tiles:
    // slot s of XCD x walks tile phase + (s - slots before) * stride of rating group g.  xslots = 0: the plain (tile, group) grid.
    uint32_t xslots;
    uint32_t xseg[8][PK_XSEG];
    uint16_t xcnt[8][PK_XSEG];
    uint32_t gstride;                   // grec entries per rating group
    // kp_rounds (several passes per launch): per rating group one 64-bit word — arrivals of the chain's workgroups
    // (low half) | the iteration nobody may start any more (high half, 0: none) — and the XCDs its workgroups run on
    unsigned long long* pbar;
    uint32_t* pxmask;
    uint32_t ptimeout0, ptimeout1;      // wall-clock ticks (100 MHz) a workgroup waits at the first / at a later barrier
    uint32_t pinject;                   // test hook: tile 1 of every chain declares "stop" when it arrives after this iteration (0: never)
    uint32_t* pyield;                   // one word per launch: a chain has ended its batch early and asks the others to stop too
    uint32_t pyq[MM_MAX_GROUPS];        // a chain whose queue has shrunk to this many players ends the batch (0: never): compacted, the
                                        //   longest chain gets by with shorter tiles (a pass costs in proportion to the tile length), or fits kp_late
    uint16_t* wpre;                     // [group][bits_stride]: compaction word prefixes
    uint32_t* tilectl;                  // [TC_N][group][max_tiles]
    uint32_t max_tiles;
    uint32_t* out_slots;
    float* out_score;                   // |ra - rb| / 1: within the window (<= 2^30 - 1), so (float)(int32_t) never wraps
    uint32_t* out_pass;
    // What the host saw when it last looked at the chains — constant for the whole batch of kp_round launches
    // (a chain's length and buffer only change in the compaction between batches): kernel arguments, so that a
    // workgroup's first loads do not wait for a load of the chain's record.  bm = 0: not walked by kp_round.
    uint32_t bm[MM_MAX_GROUPS];
    uint8_t bbuf[MM_MAX_GROUPS];
};

// key = dead << 31 | filter bits << 19 | (rating - rmin).  `dead` is only ever set in LDS copies
// (a player that left the queue).  With the filter bits above the rating, "fits the anchor"
// (docs/MATCH_CHECK.md §2.2: same filter bits, |rating delta| <= window) is ONE interval test
// on the whole word:  key - lo <= range  (unsigned), lo = anchor's filter bits | max(r - w, 0).
// A dead key lies above every interval, so a scan needs neither a bitmap read nor a mask.
#define PK_DEAD 0x80000000u
#define PK_SPAN_BITS 19
#define PK_RMASK 0x7FFFFu
static __device__ __forceinline__ uint32_t pk_pack(int32_t r, uint32_t cons, int32_t rmin, uint32_t eqmask)
{
    return ((uint32_t)r - (uint32_t)rmin) | (((cons & eqmask) >> 4) << PK_SPAN_BITS);
}
static __device__ __forceinline__ uint32_t pk_rating(uint32_t k) { return k & PK_RMASK; }
// interval of the keys that fit the queued anchor ka (bit 31 clear)
static __device__ __forceinline__ void pk_bounds(uint32_t ka, uint32_t w, uint32_t& lo, uint32_t& rng)
{
    const uint32_t ra = ka & PK_RMASK, top = ka & ~PK_RMASK;
    const uint32_t rl = ra > w ? ra - w : 0u;
    const uint32_t rh = ra + w < PK_RMASK ? ra + w : PK_RMASK;
    lo = top | rl;
    rng = rh - rl;
}
static __device__ __forceinline__ bool pk_in(uint32_t kc, uint32_t lo, uint32_t rng) { return kc - lo <= rng; }
static __device__ __forceinline__ bool pk_fit(uint32_t ka, uint32_t kc, uint32_t w)
{
    uint32_t lo, rng;
    pk_bounds(ka, w, lo, rng);
    return pk_in(kc, lo, rng);
}

// ------------------------------------------------------------------------------------
// kp_init: one workgroup per rating group.  Rating span of the chain (queue + anchor),
// eligibility for the packed-key path, the tick's starting counters.
// ------------------------------------------------------------------------------------
__global__ __launch_bounds__(1024) void kp_init(PairParams P, uint32_t max_len)
{
    __shared__ int32_t s_lo[16], s_hi[16];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const uint32_t g = blockIdx.x;
    const uint32_t c = P.mode * P.n_groups + g;
    ChainDev* const ch = P.chains + c;
    PairChain* const pc = P.pchains + g;
    const int32_t* const qr = P.q_rating + (size_t)c * P.capacity;
    const uint32_t m = ch->len;
    int32_t lo = 0x7FFFFFFF, hi = (int32_t)0x80000000;
    // (eight loads in flight per thread: one workgroup reads a 300 000-player queue, and one load per trip to memory was
    // 47 us at the head of every tick of cfg-2 — round 5)
    uint32_t i0 = tid;
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
    if (tid == 0) {
        for (int w = 1; w < 16; ++w) {
            lo = s_lo[w] < lo ? s_lo[w] : lo;
            hi = s_hi[w] > hi ? s_hi[w] : hi;
        }
        const LobbyDev& lb = ch->lobby;
        uint32_t has = 0, team = 0, a_slot = 0, a_cons = 0;
        int32_t a_rating = 0;
        if (lb.n) {
            has = 1;
            team = lb.cnt[0] ? 0u : 1u;
            a_slot = lb.slot[team][0];
            a_rating = lb.rating[team][0];
            a_cons = lb.cons[team][0];
            lo = a_rating < lo ? a_rating : lo;
            hi = a_rating > hi ? a_rating : hi;
        }
        bool fast = lb.n <= 1u && m <= max_len;
        if (m + has > 0 && ((long long)hi - (long long)lo) >= (1ll << PK_SPAN_BITS)) fast = false;
        if (m + has == 0) lo = 0;
        // Deferred effect of mm_cancel on the stored lobby (docs/MATCH_CHECK.md §4, the order of
        // operations inside one attempt, search/worker.ex:295-321): an empty queue means no attempt,
        // the lobby stays as stored; a cancelled head filters it before anybody is judged; a live
        // head is judged against the STALE lobby first, then remove_inactive_players filters it
        // (and that attempt never emits).
        uint32_t pos0 = 0, changed0 = 0, extra0 = 0;
        if (fast && P.purge && has) {
            const uint32_t hs = ch->head_state;
            const uint32_t stale_slot = a_slot;
            if (hs != 0u && P.state[stale_slot] != MM_ST_LIVE) {
                if (hs == 1u) {
                    const size_t qo = (size_t)c * P.capacity;
                    const int32_t hr = qr[0];
                    const uint32_t hc = P.q_cons[qo];
                    const uint32_t d = hr >= a_rating ? (uint32_t)hr - (uint32_t)a_rating : (uint32_t)a_rating - (uint32_t)hr;
                    pos0 = 1;
                    if (d <= P.window && (((hc ^ a_cons) & P.eqmask) == 0u)) {
                        // added to the other team; the filter then leaves it alone in the lobby
                        extra0 = 1; changed0 = 1;
                        a_slot = P.q_slot[qo]; a_rating = hr; a_cons = hc; team = 1u - team;
                    } else has = 0;
                } else has = 0;
                P.state[stale_slot] = MM_ST_FREE;
                P.released[atomicAdd(P.n_released, 1u)] = stale_slot;
            }
        }
        pc->fast = fast ? 1u : 0u;
        pc->m = m;
        pc->qlen = m - extra0;
        pc->pos0 = pos0;
        pc->changed0 = changed0;
        pc->extra0 = extra0;
        pc->buf = 0;
        pc->rmin = lo;
        pc->has_anchor = has;
        pc->a_key = has ? pk_pack(a_rating, a_cons, lo, P.eqmask) : 0u;
        pc->a_slot = a_slot;
        pc->a_cons = a_cons;
        pc->a_team = team;
        pc->a_rating = a_rating;
        pc->passes = 0;
        pc->n_out = 0;
        pc->before = m + lb.n + (P.purge ? ch->purged : 0u);
        pc->err = 0;
        pc->pairs = 0;
        pc->scanned = 0;
        pc->tested = 0;
        pc->tested_nx = 0;
        for (int k = 0; k < 8; ++k) pc->dbg[k] = 0;
        pc->stage = m < PL_MAX ? PS_LATE : PS_TILED;
        pc->ntiles = (m + PK_T - 1u) / PK_T;
        pc->want_compact = 0;
        pc->cur_pass = 0;
        pc->new_m = m;
        pc->rounds = 0;
        pc->ghops = 0; pc->gtry = 0; pc->gstale = 0;
        for (int k = 0; k < 16; ++k) { pc->tm[k] = 0; pc->ptm[k] = 0; }
        pc->pfail = 0; pc->ppass = 0;
        for (int k = 0; k < 4; ++k) pc->pslow[k] = 0;
        pc->pxm = 0;
        P.pbar[g] = 0ull; P.pxmask[g] = 0u;          // (kp_rounds' words start from zero: here and behind every batch, kc_commit)
        if (g == 0u) *P.pyield = 0u;
    }
    // tile populations (every tile full but the last)
    if (m <= max_len) {
        const uint32_t nt = (m + PK_T - 1u) / PK_T;
        for (uint32_t t = tid; t < P.max_tiles; t += 1024) {
            P.tilectl[((size_t)TC_ENT * P.n_groups + g) * P.max_tiles + t] = PK_NO;
            P.tilectl[((size_t)TC_ALIVE * P.n_groups + g) * P.max_tiles + t] =
                t < nt ? dev_min_u32(PK_T, m - t * PK_T) : 0u;
        }
    }
}

// kp_pack: grid (blocks over index space, rating groups).
__global__ __launch_bounds__(1024) void kp_pack(PairParams P)
{
    const uint32_t g = blockIdx.y;
    const PairChain* const pc = P.pchains + g;
    if (!pc->fast) return;
    const uint32_t m = pc->m;
    const uint32_t i = blockIdx.x * 1024u + threadIdx.x;
    const uint32_t c = P.mode * P.n_groups + g;
    const size_t qo = (size_t)c * P.capacity, po = (size_t)g * P.pstride;
    if (i < m) {
        P.key[0][po + i] = pk_pack(P.q_rating[qo + i], P.q_cons[qo + i], pc->rmin, P.eqmask);
        P.oidx[0][po + i] = i;
        P.nx16[0][po + i] = (uint16_t)NX_INV;
    }
    if ((i & 31u) == 0u && i < m + 32u) {          // bitmap word of [i, i+32): ones below m
        const uint32_t left = i < m ? m - i : 0u;
        uint32_t wbits = left >= 32u ? 0xFFFFFFFFu : ((1u << left) - 1u);
        if (i == 0u && pc->extra0) wbits &= ~1u;               // the head sits in the lobby already
        P.bits[0][(size_t)g * P.bits_stride + (i >> 5)] = wbits;
    }
}

// kp_nx_init: next[] for every queued player.  A workgroup stages its 2048 anchors and the
// 6144 candidates after them in LDS; one wave per anchor, 64 candidates per step (ballot +
// ffs = arg-min over queue position).  Everybody is queued at this point, so there is no
// liveness test.  A fit beyond the staged window is looked up in HBM (rare unless the pool is
// sparse).  The horizon of a chain that will be walked by the tiled path is the end of the
// tile after the anchor's own.
#define NXI_THREADS 512
#define NXI_SEG 2048u
#define NXI_STAGE 8192u
__global__ __launch_bounds__(NXI_THREADS) void kp_nx_init(PairParams P, uint32_t seg, uint32_t stage)
{
    __shared__ uint32_t s_k[NXI_STAGE];
    const uint32_t g = blockIdx.y;
    const PairChain* const pc = P.pchains + g;
    if (!pc->fast) return;
    const uint32_t m = pc->m;
    const uint32_t s0 = blockIdx.x * seg;              // seg anchors per workgroup (NXI_SEG, or fewer for a small pool: host)
    if (s0 >= m) return;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const size_t po = (size_t)g * P.pstride;
    const uint32_t* const key = P.key[0] + po;
    const uint32_t w = P.window;
    const uint32_t stage_end = dev_min_u32(m, s0 + stage);       // stage <= NXI_STAGE entries: the anchors and the candidates behind them
    for (uint32_t i = tid; i < stage_end - s0; i += NXI_THREADS) s_k[i] = key[s0 + i];
    __syncthreads();
    const uint32_t a_end = dev_min_u32(m, s0 + seg);
    unsigned long long tst = 0;
    for (uint32_t a = s0 + (uint32_t)wave; a < a_end; a += NXI_THREADS / 64) {
        const uint32_t akey = s_k[a - s0];
        uint32_t klo, krng;
        pk_bounds(akey, w, klo, krng);
        const uint32_t hend = m < PL_MAX ? m : dev_min_u32(m, (a / PK_T + 2u) * PK_T);
        const uint32_t lend = dev_min_u32(hend, stage_end);
        uint32_t j = PK_NO;
        // (round 5, measured and taken out again: four 64-candidate steps per round trip to LDS instead of one — the kernel
        // took 285 us either way; it is not the dependent reads of a wave's 256 anchors that bound it)
        for (uint32_t p = a + 1u; p < lend; p += 64u) {
            const uint32_t cidx = p + (uint32_t)lane;
            const bool ok = cidx < lend && pk_in(s_k[cidx - s0], klo, krng);
            const unsigned long long b = __ballot(ok);
            if (b) { j = p + (uint32_t)__ffsll(b) - 1u; break; }
        }
        if (j == PK_NO) {
            for (uint32_t p = lend > a + 1u ? lend : a + 1u; p < hend; p += 64u) {
                const uint32_t cidx = p + (uint32_t)lane;
                const bool ok = cidx < hend && pk_in(key[cidx], klo, krng);
                const unsigned long long b = __ballot(ok);
                if (b) { j = p + (uint32_t)__ffsll(b) - 1u; break; }
            }
        }
        if (lane == 0)
            P.nx16[0][po + a] = (uint16_t)(j != PK_NO ? j - a : (hend == m ? NX_NONE : NX_FAR));
        tst += (j != PK_NO ? j : hend) - a;               // candidates this anchor was tested against
    }
    if ((P.tune & 0x2000u) && lane == 0 && tst) { atomicAdd(&(P.pchains + g)->tested, tst); atomicAdd(&(P.pchains + g)->tested_nx, tst); }
}

// ------------------------------------------------------------------------------------
// kp_late: the whole chain in LDS, one workgroup per rating group.
// ------------------------------------------------------------------------------------

// Lanes of one wave run in lockstep on the GPU (this is only a scheduling barrier there);
// the CPU shim runs them one after another between collectives, so a "every lane reads, then
// lane 0 writes" sequence needs a rendezvous in between to mean the same thing in both.
static __device__ __forceinline__ void wave_lockstep() { __builtin_amdgcn_wave_barrier(); }

// wave-uniform values: pin them to scalar registers
static __device__ __forceinline__ uint32_t uni(uint32_t v) { return (uint32_t)__builtin_amdgcn_readfirstlane((int)v); }
static __device__ __forceinline__ uint32_t lane_get(uint32_t v, int l) { return (uint32_t)__builtin_amdgcn_readlane((int)v, l); }

// LDS words other waves of the workgroup update while we run: relaxed workgroup-scope
// atomics (a real ds_read / ds_write every time, never a register copy, never a flat op).
static __device__ __forceinline__ uint32_t lds_ld(const uint32_t* p)
{
    return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
}
static __device__ __forceinline__ uint32_t lds_ld16(const uint16_t* p)
{
    return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
}
static __device__ __forceinline__ void lds_st(uint32_t* p, uint32_t v)
{
    __hip_atomic_store(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
}
static __device__ __forceinline__ void lds_st16(uint16_t* p, uint16_t v)
{
    __hip_atomic_store(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
}

static __device__ __forceinline__ uint32_t l_alive(const uint32_t* bits, uint32_t i)
{
    return (lds_ld(bits + (i >> 5)) >> (i & 31u)) & 1u;
}

// One round trip to LDS of a scan for the first queued key (no dead flag) inside [klo, klo + krng]: N 64-candidate
// steps from p, all N * 64 of them inside the chain — N keys per lane loaded, then balloted in order.  The first
// fit's index, or PK_NO.  ABORTABLE: `ev` is read along with the keys, and a trip without a fit that saw an event
// posted says PK_ABORT.  Wave-wide.
template <uint32_t N, bool ABORTABLE>
static __device__ __forceinline__ uint32_t l_scan_trip(const uint32_t* key, uint32_t klo, uint32_t krng, uint32_t p, int lane,
                                                       const uint32_t* ev = nullptr)
{
    uint32_t kv[N];
#pragma unroll
    for (uint32_t u = 0; u < N; ++u) kv[u] = lds_ld(key + p + 64u * u + (uint32_t)lane);
    uint32_t e = EV_NONE;
    if (ABORTABLE) e = lds_ld(ev);
#pragma unroll
    for (uint32_t u = 0; u < N; ++u) {
        const unsigned long long b = __ballot(pk_in(kv[u], klo, krng));
        if (b) return p + 64u * u + (uint32_t)__ffsll(b) - 1u;
    }
    return ABORTABLE && uni(e) != EV_NONE ? PK_ABORT : PK_NO;
}
// ... and one bounded step of it: the chain may end inside the 64 candidates from p
static __device__ __forceinline__ uint32_t l_scan_step(const uint32_t* key, uint32_t klo, uint32_t krng, uint32_t p, uint32_t end, int lane)
{
    const uint32_t c = p + (uint32_t)lane;
    const bool ok = c < end && pk_in(lds_ld(key + c), klo, krng);
    const unsigned long long b = __ballot(ok);
    return b ? p + (uint32_t)__ffsll(b) - 1u : PK_NO;
}

// first index in [from, end) whose key is queued (no dead flag) and fits akey, or PK_NO.  Wave-wide.
// The chaser's own scans (nobody aborts them): four 64-candidate steps per round trip to LDS — late in a tick the
// carried anchor's first fit from the head of the queue lies thousands of positions away, one dependent read per step
// (round 5: one trip of four steps for the fit that lies near, then SIXTEEN steps a trip — the carried anchor's scan of
// a late pass runs over thousands of positions, 2.1k cycles a pass of the longest chain at four steps a trip)
static __device__ __forceinline__ uint32_t l_scan_fit(const uint32_t* key, uint32_t akey, uint32_t from, uint32_t end, uint32_t w, int lane)
{
    uint32_t klo, krng, j;
    pk_bounds(akey, w, klo, krng);
    uint32_t p = from;
    if (p + 256u <= end) {
        if ((j = l_scan_trip<4, false>(key, klo, krng, p, lane)) != PK_NO) return j;
        p += 256u;
    }
    for (; p + 1024u <= end; p += 1024u)
        if ((j = l_scan_trip<16, false>(key, klo, krng, p, lane)) != PK_NO) return j;
    for (; p + 256u <= end; p += 256u)
        if ((j = l_scan_trip<4, false>(key, klo, krng, p, lane)) != PK_NO) return j;
    for (; p < end; p += 64u)
        if ((j = l_scan_step(key, klo, krng, p, end, lane)) != PK_NO) return j;
    return PK_NO;
}
// The same for the repair waves, which give up (PK_ABORT) once an event is posted at `ev`.
// (round 5): four steps a trip as well, the event looked at once per trip — late in a tick a
// repair scans thousands of positions, the thirteen waves were as busy as the pass is long (one 64-candidate step
// per dependent read) and the chaser met what they had not reached yet: ~330 careful steps a tick on stale entries
// (sixteen steps a trip, as the chaser's own scan has them, bring the repairs nothing more: 87 stale hits against 96)
static __device__ __forceinline__ uint32_t l_scan_fit_ev(const uint32_t* key, uint32_t akey, uint32_t from, uint32_t end, uint32_t w, int lane,
                                                         const uint32_t* ev)
{
    uint32_t klo, krng, j;
    pk_bounds(akey, w, klo, krng);
    uint32_t p = from;
    for (; p + 256u <= end; p += 256u)
        if ((j = l_scan_trip<4, true>(key, klo, krng, p, lane, ev)) != PK_NO) return j;
    for (; p < end; p += 64u) {
        if ((j = l_scan_step(key, klo, krng, p, end, lane)) != PK_NO) return j;
        if (lds_ld(ev) != EV_NONE) return PK_ABORT;
    }
    return PK_NO;
}

// first queued index >= pos, or PK_NO.  Wave-wide: 64 bitmap words per step.
static __device__ __forceinline__ uint32_t l_succ(const uint32_t* bits, uint32_t pos, uint32_t m, int lane)
{
    if (pos >= m) return PK_NO;
    const uint32_t nwords = (m + 31u) >> 5, w0 = pos >> 5;
    for (uint32_t wb = w0; wb < nwords; wb += 64u) {
        const uint32_t wi = wb + (uint32_t)lane;
        uint32_t v = wi < nwords ? lds_ld(bits + wi) : 0u;
        if (wi == w0) v &= 0xFFFFFFFFu << (pos & 31u);
        const unsigned long long b = __ballot(v != 0u);
        if (b) {
            const int l = __ffsll(b) - 1;
            const uint32_t vv = lane_get(v, l);
            return ((wb + (uint32_t)l) << 5) + (uint32_t)__ffs((int)vv) - 1u;
        }
    }
    return PK_NO;
}

#define PL_RING 512u                 // (anchor, partner) steps in flight between chaser and consumer
#define PL_EXT 0xFFFEu               // ring: the anchor is held by value (s_ext), not an index
#define PL_NOPART 0xFFFFu            // ring: anchor seated, no partner (it stays in the lobby)
#define PL_S (PL_MAX - 1u)           // sentinel index: nxg[PL_S] points at itself, nobody lives there
#define PL_SPEC 64u                  // steps chased speculatively before they are checked

// kp_late keeps, per index i of the chain, one LDS word  nxg[i] = next[i] | (4 * g[i]) << 16:
//   next[i]  first queued player after i that fits i           (LNX_NONE / LNX_INV codes)
//   g[i]     first queued player after next[i]  = the anchor the cursor picks after the lobby
//            (i, next[i]) is emitted;  PL_S when unknown or when the queue ends first
// Both only go stale by their target leaving the queue, which the bitmap shows.  The walk
// a -> g[a] -> g[g[a]] ... is then a bare chain of dependent LDS reads (three instructions a
// step; late_blind_chase); 64 steps are chased blind, checked against the bitmap by 64 lanes at once
// (late_blind_check), and the confirmed prefix is handed through the ring (LateRing::push_block) to the
// consumer waves (wave 1, late_kill: bitmap; wave 2, late_emit: emission).  An anchor the blind chase cannot
// take — carried in, stale or unknown next[] — gets one careful step (late_careful_step).  Thirteen waves
// keep nxg repaired (late_repair).  The chaser's own state is a LateCursor, what it counts a LateDiag.
static __device__ __forceinline__ uint32_t nxg_make(uint32_t t, uint32_t gi) { return t | ((gi << 2) << 16); }

// first queued index >= from (one lane's own loop), or PL_S
static __device__ __forceinline__ uint32_t lane_succ(const uint32_t* bits, uint32_t from, uint32_t nwords)
{
    uint32_t wi = from >> 5;
    if (wi >= nwords) return PL_S;
    uint32_t v = lds_ld(bits + wi) & (0xFFFFFFFFu << (from & 31u));
    while (v == 0u) {
        if (++wi >= nwords) return PL_S;
        v = lds_ld(bits + wi);
    }
    return (wi << 5) + (uint32_t)__ffs((int)v) - 1u;
}

// kp_late's LDS, one object.
struct LateLds {
    uint32_t path[PL_SPEC];         // first in LDS: the chase addresses it with immediates
    uint32_t nxg[PL_MAX];
    uint32_t key[PL_MAX];
    uint32_t bits[PL_WORDS + 64];   // zero padded: 64 words can be read past the end
    uint16_t wpre[PL_WORDS];        // compaction: queued players before the word
    uint32_t ring[PL_RING];         // anchor | partner << 16
    uint16_t ringp[PL_RING];        // pass of the step, relative to the kernel's first
    uint32_t wtot[16];
    uint32_t event, m, head, tail, killed, aidx, buf, nout;
    uint32_t ext[5];                // anchor by value: slot, rating, cons, key, team
};

// The ring of steps of the walk between the chaser and the consumer: head (pushed by wave 0) >= killed (both players
// out of the bitmap, wave 1) >= tail (lobby emitted, wave 2: the slot is free again).  rk / rtail are the chaser's
// registers: steps pushed, the consumer's tail as last seen.
struct LateRing {
    LateLds& S;
    const int lane;
    uint32_t rk = 0, rtail = 0;
    __device__ __forceinline__ LateRing(LateLds& S_, int lane_) : S(S_), lane(lane_) {}
    // the consumers' side: step i's (anchor | partner << 16), its pass
    __device__ __forceinline__ uint32_t step(uint32_t i) const { return S.ring[i % PL_RING]; }
    __device__ __forceinline__ uint32_t pass_of(uint32_t i) const { return S.ringp[i % PL_RING]; }
    // the chaser's side: wait until n more steps fit
    __device__ __forceinline__ void room(uint32_t n)
    {
        if (rk - rtail + n > PL_RING) {
            rtail = uni(lds_ld(&S.tail));
            while (rk - rtail + n > PL_RING) { __builtin_amdgcn_s_sleep(2); rtail = uni(lds_ld(&S.tail)); }
        }
    }
    // ns steps handed to the consumer, lane l's the (ia, it) of lane l: it drops both players from the queue
    // bitmap and, when there is a partner, emits the lobby
    __device__ __forceinline__ void push_block(uint32_t ns, uint32_t ia, uint32_t it, uint32_t pass)
    {
        room(ns);
        if ((uint32_t)lane < ns) {
            S.ring[(rk + (uint32_t)lane) % PL_RING] = ia | (it << 16);
            S.ringp[(rk + (uint32_t)lane) % PL_RING] = (uint16_t)pass;
        }
        rk += ns;
        if (lane == 0) lds_st(&S.head, rk);
    }
    // one step (a, t), wave uniform
    __device__ __forceinline__ void push(uint32_t a, uint32_t t, uint32_t pass) { push_block(1u, a, t, pass); }
    // until every pushed step is in the bitmap (emission may still be under way)
    __device__ __forceinline__ void drain()
    {
        uint32_t kd = uni(lds_ld(&S.killed));
        while (kd != rk) { __builtin_amdgcn_s_sleep(1); kd = uni(lds_ld(&S.killed)); }
    }
};

// The chaser's state (wave 0; uniform across its lanes).  a_idx: index of the anchor, or PL_EXT when it is
// held by value (carried in from an earlier tick / over a compaction).
struct LateCursor {
    uint32_t has_anchor, a_idx, a_pushed;
    uint32_t qlen, pos, passes, in_pass, changed, n_out;
    unsigned long long pairs, scanned;
    // the pass is over; false: it changed nothing, and the walk is over with it
    __device__ __forceinline__ bool end_pass() { ++passes; in_pass = 0; return changed != 0u; }
    // empty lobby: the popped player opens it (no pair evaluation)
    __device__ __forceinline__ void open_lobby(uint32_t a)
    {
        --qlen; --pairs; changed = 1; has_anchor = 1; a_idx = a; a_pushed = 0;
        pos = a + 1u;
    }
};
static __device__ __forceinline__ LateCursor late_cursor_open(const PairChain* pc)
{
    LateCursor C;
    C.has_anchor = pc->has_anchor; C.a_idx = PL_EXT; C.a_pushed = 1;
    C.qlen = pc->qlen; C.pos = pc->pos0; C.passes = pc->passes; C.in_pass = pc->pos0 ? 1u : 0u; C.changed = pc->changed0;
    C.n_out = pc->n_out;
    C.pairs = pc->pairs; C.scanned = pc->scanned;
    if (pc->pos0) { C.scanned += C.qlen + pc->extra0; C.pairs += C.qlen + pc->extra0; }    // the pass is already under way
    return C;
}
static __device__ __forceinline__ void late_cursor_commit(PairChain* pc, const LateCursor& C)
{
    pc->pos0 = 0; pc->changed0 = 0; pc->extra0 = 0;
    pc->qlen = C.qlen; pc->has_anchor = C.has_anchor; pc->passes = C.passes; pc->n_out = C.n_out;
    pc->pairs = C.pairs; pc->scanned = C.scanned;
}

// What the waves count (PairChain.dbg[PD_*], PairChain.tested).
struct LateDiag {
    uint32_t stale = 0, inv = 0, slowsucc = 0, compact = 0, fixed = 0, clk = 0, wall = 0, wrapc = 0;
    unsigned long long tst = 0;      // candidates this wave's scans were tested against
};

static __device__ __forceinline__ uint32_t late_anchor_key(const LateLds& S, uint32_t a_idx)
{
    return a_idx == PL_EXT ? S.ext[3] : (S.key[a_idx] & ~PK_DEAD);
}

// ---- load the chain: bitmap, keys with dead flags, nxg from nx16 ----
static __device__ __forceinline__ void late_load(const PairParams& P, const PairChain* pc, LateLds& S, uint32_t m, uint32_t g, size_t po, int tid)
{
    const uint32_t nwords = (m + 31u) >> 5;
    for (uint32_t i = tid; i < PL_WORDS + 64u; i += PL_THREADS)
        S.bits[i] = i < nwords ? P.bits[pc->buf][(size_t)g * P.bits_stride + i] : 0u;
    const uint32_t* const key = P.key[pc->buf] + po;
    __syncthreads();
    for (uint32_t i = tid; i < m; i += PL_THREADS) S.key[i] = key[i] | (l_alive(S.bits, i) ? 0u : PK_DEAD);
    if (tid == 0) {
        S.event = EV_NONE; S.m = m; S.head = 0; S.tail = 0; S.killed = 0; S.aidx = PK_NO; S.buf = pc->buf;
        S.ext[0] = pc->a_slot; S.ext[1] = (uint32_t)pc->a_rating; S.ext[2] = pc->a_cons;
        S.ext[3] = pc->a_key; S.ext[4] = pc->a_team;
    }
    __syncthreads();
    for (uint32_t i = tid; i < PL_MAX; i += PL_THREADS) {
        uint32_t t = LNX_NONE, gi = PL_S;
        if (i < m) {
            const uint32_t o = P.nx16[pc->buf][po + i];
            t = o == NX_NONE ? LNX_NONE : (o == NX_INV || o == NX_FAR) ? LNX_INV : i + o;
            if (t < LNX_INV) gi = lane_succ(S.bits, t + 1u, nwords);
        }
        S.nxg[i] = nxg_make(t, gi);
    }
    __syncthreads();
}

// ---- blind chase: x -> g[x], PL_SPEC times from the anchor, every word met into S.path ----
static __device__ __forceinline__ void late_blind_chase(LateLds& S, uint32_t a_idx, int lane)
{
    uint32_t x4 = a_idx << 2;
    for (uint32_t k0 = 0; k0 < PL_SPEC; k0 += 8u) {
#pragma unroll
        for (uint32_t k = 0; k < 8u; ++k) {
            const uint32_t r = lds_ld((const uint32_t*)((const char*)S.nxg + x4));
            S.path[k0 + k] = r;
            x4 = r >> 16;
        }
        if (uni(x4) == (PL_S << 2)) {          // parked: the rest of the block is the sentinel
            for (uint32_t k = k0 + 8u + (uint32_t)lane; k < PL_SPEC; k += 64u) S.path[k] = nxg_make(LNX_NONE, PL_S);
            break;
        }
    }
}

// ---- check the 64 steps at once; the confirmed prefix goes to the consumer.  Confirmed steps. ----
static __device__ __forceinline__ uint32_t late_blind_check(LateLds& S, LateCursor& C, LateRing& R, uint32_t pass, int lane)
{
    const uint32_t r = S.path[lane];
    const uint32_t rp = lane ? S.path[lane - 1] : 0u;
    const uint32_t ia = lane ? (rp >> 18) : C.a_idx;      // anchor of step `lane`
    const uint32_t it = r & 0xFFFFu, ig = r >> 18;
    bool ok = ia != PL_S && it < LNX_INV && ig != PL_S;
    if (ok) ok = l_alive(S.bits, it) && l_alive(S.bits, ig);
    const unsigned long long good = __ballot(ok);
    const uint32_t ns = good == ~0ull ? 64u : (uint32_t)__ffsll(~good) - 1u;
    if (ns) {
        R.push_block(ns, ia, it, pass);
        // every step: partner leaves the queue, the next player opens a lobby
        C.qlen -= 2u * ns; C.pairs -= ns; C.n_out += ns; C.changed = 1;
        C.a_idx = lane_get(ig, (int)ns - 1);
        C.a_pushed = 0;
    }
    return ns;
}

// ---- one careful step for the anchor C.a_idx; t: its partner when the caller knows it, or PK_NO.
// false: the pass ends here (nobody fits the anchor until the end, or the pass ran off the queue) ----
static __device__ __forceinline__ bool late_careful_step(LateLds& S, LateCursor& C, LateRing& R, LateDiag& D, uint32_t t, uint32_t m, uint32_t w,
                                                         uint32_t pass, int lane)
{
    const uint32_t a_key = late_anchor_key(S, C.a_idx);
    if (t == PK_NO) {
        const uint32_t cnx = uni(lds_ld(S.nxg + C.a_idx)) & 0xFFFFu;
        if (cnx == LNX_NONE) return false;                  // nobody fits until the end
        if (cnx < LNX_INV && l_alive(S.bits, cnx)) t = cnx;
        else {
            if (cnx == LNX_INV) ++D.inv; else ++D.stale;
            const uint32_t from = cnx == LNX_INV ? C.a_idx + 1u : cnx + 1u;
            t = uni(l_scan_fit(S.key, a_key, from, m, w, lane));
            D.tst += (t == PK_NO ? m : t) - from;
            if (t == PK_NO) return false;
        }
    }
    // is_filled (search/worker.ex:313-319): hand the step to the consumer
    R.push(C.a_idx, t, pass);
    --C.qlen; C.changed = 1; C.has_anchor = 0; C.pos = t + 1u; ++C.n_out;
    ++D.slowsucc;
    const uint32_t a2 = uni(l_succ(S.bits, t + 1u, m, lane));
    if (a2 == PK_NO) return false;                          // pass ran off the queue
    C.open_lobby(a2);
    return true;
}

// ---- wave 0: the cursor walk (MATCH_CHECK.md §3, §4), until the queue is quiescent or wants a compaction ----
static __device__ __forceinline__ void late_chase(LateLds& S, LateCursor& C, LateRing& R, LateDiag& D, uint32_t m, uint32_t w, uint32_t pass0,
                                                  int lane)
{
    __builtin_amdgcn_s_setprio(3);
    uint32_t ev = EV_NONE;
    const long long tc0 = clock64(), tw0 = wall_clock64();
    for (;;) {
        if (!C.in_pass) {
            R.drain();                              // a new pass reads the bitmap from the head
            if (C.qlen == 0u) { ev = EV_DONE; break; }                 // while (len > 0)
            if (m > PL_COMPACT_MIN && C.qlen * 2u < m) { ev = EV_COMPACT; break; }
            C.in_pass = 1; C.pos = 0; C.changed = 0;
            C.scanned += C.qlen;
            C.pairs += C.qlen;
        }
        uint32_t t = PK_NO;
        if (!C.has_anchor) {
            const uint32_t a = uni(l_succ(S.bits, C.pos, m, lane));
            if (a == PK_NO) {                                       // pass ran off the queue
                if (C.end_pass()) continue;
                ev = EV_DONE; break;
            }
            C.open_lobby(a);
        } else {
            // anchor carried into this pass: first fit from the head of the queue
            const long long ts = clock64();
            t = uni(l_scan_fit(S.key, late_anchor_key(S, C.a_idx), C.pos, m, w, lane));
            D.tst += (t == PK_NO ? m : t) - C.pos;
            D.wrapc += (uint32_t)(clock64() - ts);
            if (t == PK_NO) {                                       // nobody fits: pass without change?
                if (C.end_pass()) continue;
                ev = EV_DONE; break;
            }
        }
        // Inside one pass.  Nothing here writes the bitmap: the consumer wave does,
        // and the cursor never looks back.
        const uint32_t pass = C.passes - pass0;
        for (;;) {
            // (round 5: a look at the anchor's own word first — every pass ENDS on an anchor without a partner, and the blind
            // chase used to find that out with a block of eight dependent reads and a 64-lane check that confirmed nothing,
            // ~1.4k cycles where one read says it; likewise after every careful step that lands on such an anchor)
            bool blind = t == PK_NO && C.a_idx != PL_EXT;
            if (blind) {
                const uint32_t r0 = uni(lds_ld(S.nxg + C.a_idx));
                blind = (r0 & 0xFFFFu) < LNX_INV && (r0 >> 18) != PL_S;
            }
            if (blind) {
                late_blind_chase(S, C.a_idx, lane);
                if (late_blind_check(S, C, R, pass, lane) == PL_SPEC) continue;
            }
            if (!late_careful_step(S, C, R, D, t, m, w, pass, lane)) break;
            t = PK_NO;
        }
        if (C.has_anchor && !C.a_pushed) { R.push(C.a_idx, PL_NOPART, pass); C.a_pushed = 1; }   // seated, stays
        if (!C.end_pass()) { ev = EV_DONE; break; }
    }
    D.clk += (uint32_t)(clock64() - tc0);
    D.wall += (uint32_t)(wall_clock64() - tw0);
    if (lane == 0) { S.aidx = C.has_anchor ? C.a_idx : PK_NO; S.nout = C.n_out; lds_st(&S.event, ev); }
    __builtin_amdgcn_s_setprio(0);
}

// ---- wave 1: consumer, first half: the steps' players leave the queue (LDS only) ----
// Kept apart from the emission (wave 2) since round 3: the chaser opens every pass by waiting until all
// pushed steps are in the bitmap, and with one consumer wave the kills of the last steps of a pass sat behind
// the emission loads of the steps before them (two dependent loads from HBM: 0.48M of the 2.94M cycles of the
// longest chain's walking wave were spent in that wait).
static __device__ __forceinline__ void late_kill(LateLds& S, const LateRing& R, int lane)
{
    uint32_t ktail = uni(lds_ld(&S.killed));
    for (;;) {
        uint32_t head = uni(lds_ld(&S.head));
        if (head == ktail) {
            if (lds_ld(&S.event) != EV_NONE) {
                head = uni(lds_ld(&S.head));
                if (head == ktail) break;
            } else { __builtin_amdgcn_s_sleep(1); continue; }
        }
        const uint32_t nb = dev_min_u32(64u, head - ktail);
        if ((uint32_t)lane < nb) {
            const uint32_t e = R.step(ktail + (uint32_t)lane);
            const uint32_t a = e & 0xFFFFu, t = e >> 16;
            if (a != PL_EXT) { atomicAnd(&S.bits[a >> 5], ~(1u << (a & 31u))); atomicOr(&S.key[a], PK_DEAD); }
            if (t != PL_NOPART) { atomicAnd(&S.bits[t >> 5], ~(1u << (t & 31u))); atomicOr(&S.key[t], PK_DEAD); }
        }
        wave_lockstep();
        ktail += nb;
        if (lane == 0) lds_st(&S.killed, ktail);            // the chaser only waits for this
    }
}

// ---- wave 2: consumer, second half: the lobbies of the steps that are in the bitmap, 64 at a time ----
static __device__ __forceinline__ void late_emit(const PairParams& P, LateLds& S, const LateRing& R, uint32_t& emit_idx, uint32_t g, size_t qo,
                                                 size_t po, uint32_t pass0, int lane)
{
    uint32_t* const os = P.out_slots + (size_t)g * P.out_slot_stride;
    float* const osc = P.out_score + (size_t)g * P.out_rec_stride;
    uint32_t* const opass = P.out_pass + (size_t)g * P.out_rec_stride;
    uint32_t tail = uni(lds_ld(&S.tail));
    const uint32_t* const oidx = P.oidx[uni(lds_ld(&S.buf))] + po;
    for (;;) {
        const uint32_t killed = uni(lds_ld(&S.killed));
        if (killed == tail) {
            if (lds_ld(&S.event) != EV_NONE && uni(lds_ld(&S.head)) == tail && uni(lds_ld(&S.killed)) == tail) break;
            __builtin_amdgcn_s_sleep(2);
            continue;
        }
        const uint32_t nb = dev_min_u32(64u, killed - tail);
        const bool mine = (uint32_t)lane < nb;
        const uint32_t e = mine ? R.step(tail + (uint32_t)lane) : 0xFFFFFFFFu;
        const uint32_t a = e & 0xFFFFu, t = e >> 16;
        const bool is_match = mine && t != PL_NOPART;
        const unsigned long long mm = __ballot(is_match);
        if (is_match) {
            const uint32_t k = emit_idx + (uint32_t)__popcll(mm & ((1ull << lane) - 1ull));
            const uint32_t ka = a == PL_EXT ? S.ext[3] : S.key[a];
            const uint32_t kt = S.key[t];
            const uint32_t ra = pk_rating(ka), rt = pk_rating(kt);
            const uint32_t team = a == PL_EXT ? S.ext[4] : 0u;
            os[2u * k + team] = a == PL_EXT ? S.ext[0] : P.q_slot[qo + oidx[a]];
            os[2u * k + (1u - team)] = P.q_slot[qo + oidx[t]];
            osc[k] = (float)(int32_t)(ra > rt ? ra - rt : rt - ra);
            opass[k] = pass0 + R.pass_of(tail + (uint32_t)lane);
        }
        emit_idx += (uint32_t)__popcll(mm);
        tail += nb;
        wave_lockstep();
        if (lane == 0) lds_st(&S.tail, tail);               // the ring slots are free again
    }
}

// ---- waves 3..15: repair nxg behind the cursor ----
static __device__ __forceinline__ void late_repair(LateLds& S, LateDiag& D, uint32_t m, uint32_t w, uint32_t fix_waves, uint32_t fix_sleep,
                                                   int wave, int lane)
{
    const uint32_t nwords = (m + 31u) >> 5;
    const uint32_t fw = (uint32_t)wave - 3u;
    const uint32_t nchunks = fw < fix_waves ? (m + 63u) >> 6 : 0u;
    uint32_t chunk = fw;
    uint32_t idle = 0;
    // (Round 5, measured and taken out: the sweeps starting over at the head of the queue whenever the cursor begins a
    // pass — "what the cursor meets was made stale by the pass before, so a sweep that stays ahead of it hands it fresh
    // entries".  They never finish the chain's tail then: 254 stale hits a tick against 100, kp_late 1.60 against 1.20 ms.)
    while (lds_ld(&S.event) == EV_NONE) {
        if (chunk >= nchunks) {
            chunk = fw;
            if (idle) __builtin_amdgcn_s_sleep(32);
            idle = 1;
            if (chunk >= nchunks) { __builtin_amdgcn_s_sleep(64); continue; }
        }
        if (fix_sleep & 1u) __builtin_amdgcn_s_sleep(1);
        if (fix_sleep & 2u) __builtin_amdgcn_s_sleep(2);
        if (fix_sleep & 4u) __builtin_amdgcn_s_sleep(4);
        if (fix_sleep & 8u) __builtin_amdgcn_s_sleep(8);
        if (fix_sleep & 16u) __builtin_amdgcn_s_sleep(16);
        if (fix_sleep & 32u) __builtin_amdgcn_s_sleep(32);
        const uint32_t i = (chunk << 6) + (uint32_t)lane;
        bool need = false, need_g = false;
        uint32_t from = 0, t = LNX_NONE;
        if (i < m && l_alive(S.bits, i)) {
            const uint32_t r = lds_ld(S.nxg + i);
            t = r & 0xFFFFu;
            const uint32_t gi = r >> 18;
            if (t == LNX_INV) { need = true; from = i + 1u; }
            else if (t != LNX_NONE) {
                // (both probes in one trip to LDS)
                const uint32_t at = l_alive(S.bits, t), ag = l_alive(S.bits, gi == PL_S ? t : gi);
                if (!at) { need = true; from = t + 1u; }
                else if (gi == PL_S || !ag) need_g = true;
            }
        }
        unsigned long long todo = __ballot(need);
        while (todo) {
            const int l = __ffsll(todo) - 1;
            todo &= todo - 1ull;
            const uint32_t ai = (uint32_t)__shfl((int)i, l), af = (uint32_t)__shfl((int)from, l);
            const uint32_t j = l_scan_fit_ev(S.key, S.key[ai] & ~PK_DEAD, af, m, w, lane, &S.event);
            if (j == PK_ABORT) { todo = 0; need = false; need_g = false; break; }
            D.tst += (j == PK_NO ? m : j) - af;
            if (lane == l) { t = j == PK_NO ? LNX_NONE : j; need_g = true; }
            idle = 0;
            ++D.fixed;
        }
        if (need_g) {                       // one 32-bit store: next[] and g[] stay a consistent pair
            const uint32_t gi = t < LNX_INV ? lane_succ(S.bits, t + 1u, nwords) : PL_S;
            lds_st(S.nxg + i, nxg_make(t, gi));
        }
        chunk += fix_waves;
    }
}

// ---- an anchor that is still an index leaves the index space by value (the walk is over, or a compaction renumbers) ----
static __device__ __forceinline__ void late_anchor_by_value(const PairParams& P, LateLds& S, LateCursor& C, size_t qo, size_t po, int tid)
{
    if (tid == 0 && S.aidx != PK_NO && S.aidx != PL_EXT) {
        const uint32_t oi = P.oidx[S.buf][po + S.aidx];
        S.ext[0] = P.q_slot[qo + oi];
        S.ext[1] = (uint32_t)P.q_rating[qo + oi];
        S.ext[2] = P.q_cons[qo + oi];
        S.ext[3] = S.key[S.aidx] & ~PK_DEAD;
        S.ext[4] = 0;
    }
    __syncthreads();
    if (S.aidx != PK_NO) { C.a_idx = PL_EXT; C.a_pushed = 1; }
}

// compaction: the new index of the queued player i = queued players before it
static __device__ __forceinline__ uint32_t late_rank(const LateLds& S, uint32_t i)
{
    return S.wpre[i >> 5] + (uint32_t)__popc(S.bits[i >> 5] & ((1u << (i & 31u)) - 1u));
}

// ---- compaction: drop everybody who left the queue.  The new index-space length. ----
static __device__ __forceinline__ uint32_t late_compact(const PairParams& P, LateLds& S, uint32_t m, size_t po, int tid, int lane, int wave)
{
    const uint32_t nwords = (m + 31u) >> 5;
    const uint32_t cur = S.buf;
    // exclusive prefix of the per-word populations
    const uint32_t pcw = (uint32_t)tid < nwords ? (uint32_t)__popc(S.bits[tid]) : 0u;
    const uint32_t incl = wave_incl_scan(pcw, lane);
    if (lane == 63) S.wtot[wave] = incl;
    __syncthreads();
    if ((uint32_t)tid < PL_WORDS) {
        uint32_t off = 0;
        for (int x = 0; x < wave; ++x) off += S.wtot[x];
        S.wpre[tid] = (uint16_t)(off + incl - pcw);
    }
    __syncthreads();
    const uint32_t* const oidx = P.oidx[cur] + po;
    uint32_t* const oidx_new = P.oidx[cur ^ 1u] + po;
    // chunks in ascending order: a chunk's survivors land at or below their source
    for (uint32_t base = 0; base < m; base += PL_THREADS) {
        const uint32_t i = base + (uint32_t)tid;
        uint32_t r = PK_NO, nk = 0, nv = 0, no = 0;
        if (i < m && l_alive(S.bits, i)) {
            r = late_rank(S, i);
            nk = S.key[i];
            const uint32_t v = S.nxg[i];
            uint32_t t = v & 0xFFFFu, gi = v >> 18;
            if (t < LNX_INV) {
                if (l_alive(S.bits, t)) {
                    t = late_rank(S, t);
                    if (gi != PL_S && l_alive(S.bits, gi)) gi = late_rank(S, gi);
                    else gi = PL_S;
                } else { t = LNX_INV; gi = PL_S; }
            } else gi = PL_S;
            nv = nxg_make(t, gi);
            no = oidx[i];
        }
        __syncthreads();
        if (r != PK_NO) { S.key[r] = nk; S.nxg[r] = nv; oidx_new[r] = no; }
        __syncthreads();
    }
    const uint32_t nm = (uint32_t)S.wpre[nwords - 1u] + (uint32_t)__popc(S.bits[nwords - 1u]);
    __syncthreads();
    for (uint32_t i = tid; i < PL_WORDS; i += PL_THREADS) {
        const uint32_t lo = i << 5;
        S.bits[i] = lo + 32u <= nm ? 0xFFFFFFFFu : (lo < nm ? (1u << (nm - lo)) - 1u : 0u);
    }
    for (uint32_t i = nm + (uint32_t)tid; i < m; i += PL_THREADS) S.nxg[i] = nxg_make(LNX_NONE, PL_S);
    if (tid == 0) { S.m = nm; S.buf = cur ^ 1u; S.event = EV_NONE; S.aidx = PK_NO; }
    __syncthreads();
    return S.m;
}

// ---- store the chain back ----
static __device__ __forceinline__ void late_store(const PairParams& P, PairChain* pc, const LateLds& S, const LateCursor& C, const LateDiag& D,
                                                  uint32_t emit_idx, uint32_t m, uint32_t g, int tid, int lane)
{
    const uint32_t nwords = (m + 31u) >> 5;
    for (uint32_t i = tid; i < nwords; i += PL_THREADS) P.bits[S.buf][(size_t)g * P.bits_stride + i] = S.bits[i];
    if (tid == 0) {
        pc->stage = PS_DONE;
        pc->m = m;
        pc->buf = S.buf;
        late_cursor_commit(pc, C);
        if (C.has_anchor) {
            pc->a_key = S.ext[3];
            pc->a_slot = S.ext[0];
            pc->a_cons = S.ext[2];
            pc->a_team = S.ext[4];
            pc->a_rating = (int32_t)S.ext[1];
        }
        pc->dbg[PD_STALE] = D.stale;
        pc->dbg[PD_INV] = D.inv;
        pc->dbg[PD_SLOWSUCC] = D.slowsucc;
        pc->dbg[PD_COMPACT] = D.compact;
        pc->dbg[PD_CLK] = D.clk;
        pc->dbg[PD_WALL] = D.wall;
        pc->dbg[PD_WRAPC] = D.wrapc;
    }
    if (tid == 128 && emit_idx != S.nout) atomicOr(&pc->err, MM_ERRF_SEAT_INVARIANT);
    if (tid == 192) pc->dbg[PD_FIXED] = D.fixed;     // repairs done by wave 3
    if ((P.tune & 0x2000u) && lane == 0 && D.tst) atomicAdd(&pc->tested, D.tst);
}

__global__ __launch_bounds__(PL_THREADS) void kp_late(PairParams P)
{
    __shared__ LateLds S;

    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const uint32_t g = blockIdx.x;
    PairChain* const pc = P.pchains + g;
    if (!pc->fast || pc->stage != PS_LATE) return;
    const uint32_t c = P.mode * P.n_groups + g;
    const size_t qo = (size_t)c * P.capacity, po = (size_t)g * P.pstride;
    const uint32_t w = P.window;

    uint32_t m = pc->m;
    const uint32_t pass0 = pc->passes;
    late_load(P, pc, S, m, g, po, tid);

    LateCursor C = late_cursor_open(pc);                          // wave 0
    LateRing R(S, lane);
    uint32_t emit_idx = pc->n_out;                                // consumer (wave 2)
    LateDiag D;
    const uint32_t fix_waves = 13u - dev_min_u32(P.tune & 15u, 13u);   // repair waves actually working (waves 3..15)
    const uint32_t fix_sleep = (P.tune >> 4) & 0xFFu;

    for (;;) {
        if (wave == 0) late_chase(S, C, R, D, m, w, pass0, lane);
        else if (wave == 1) late_kill(S, R, lane);
        else if (wave == 2) late_emit(P, S, R, emit_idx, g, qo, po, pass0, lane);
        else late_repair(S, D, m, w, fix_waves, fix_sleep, wave, lane);
        __syncthreads();
        const uint32_t ev = S.event;
        late_anchor_by_value(P, S, C, qo, po, tid);
        if (ev == EV_DONE) break;
        m = late_compact(P, S, m, po, tid, lane, wave);
        ++D.compact;
    }
    late_store(P, pc, S, C, D, emit_idx, m, g, tid, lane);
}

// ------------------------------------------------------------------------------------
// The tiled path: chains too long for one workgroup's LDS.  One ROUND = one pass of the
// cursor over the queue (MATCH_CHECK.md §4).  Its three steps — until round 5 also available as
// three launches (kp_tile_prep / kp_route / kp_tile_apply, MM_PAIR_FUSED=0: rounds 1-2's form,
// taken out in round 6) — are, per tile (PK_T index positions) of every chain:
//
//   prepare        repair next[] of the tile's players, then pointer-double the tile's step graph
//                  (anchor -> index after its partner; dead index -> next index) so that for
//                  EVERY entry position x the tile knows where a cursor entering at x leaves
//                  it: REC[x] = (kind, matches made inside the tile, landing position).
//   route          follow REC from tile to tile (one dependent load per tile instead of one per
//                  match), resolve what crosses tiles (partner in a later tile, anchor carried to
//                  the next pass, head match of the anchor carried in): per tile the entry, the
//                  emission offset, what becomes of the exit anchor; the pass counters.
//   apply          tiles on the path: walk the in-tile chain from the entry, drop the
//                  matched players from the queue bitmap, emit.
// kp_round does all three for one pass in one launch, kp_rounds for a batch of passes.
//
// Nothing inside a pass invalidates the tables made before it: a pass only removes
// players BEHIND the cursor, and next[] / the step graph only look ahead.
// ------------------------------------------------------------------------------------
#define PT_THREADS 1024
#define PF_N 6u                      // 16-byte loads per thread with which kp_round pulls REC / bitmap through its XCD's L2

static __device__ __forceinline__ uint32_t* tc_row(const PairParams& P, uint32_t row, uint32_t g)
{
    return P.tilectl + ((size_t)row * P.n_groups + g) * P.max_tiles;
}

static __device__ __forceinline__ uint32_t rec_make(uint32_t kind, uint32_t cnt, uint32_t land)
{
    return (kind << 30) | (cnt << 17) | land;
}

// 16-byte copies HBM -> LDS of `n` 32-bit words (both sides 16-byte aligned, n rounded up by the
// caller's padding).  One load instruction moves four words.
static __device__ __forceinline__ void copy_words_x4(uint32_t* dst, const uint32_t* src, uint32_t n, int tid, int nthreads)
{
    const uint4* const s4 = (const uint4*)src;
    uint4* const d4 = (uint4*)dst;
    for (uint32_t i = tid; i < (n + 3u) >> 2; i += nthreads) d4[i] = s4[i];
}

// ---- the phases of a tile's preparation, shared by kp_round and kp_rounds.  All take the
//      tile's LDS arrays; every thread of the (1024-thread) workgroup calls them. ----

// keys of the own tile and the next one into LDS, dead flag folded in from s_bits (tile-local
// bitmap of both tiles), 64 dead keys of padding after the horizon
template <uint32_t TP>
static __device__ __forceinline__ void prep_stage_keys(uint32_t* s_key, const uint32_t* s_bits, const uint32_t* gkey,
                                                       uint32_t hl, int tid, int nthreads = PT_THREADS)
{
    constexpr uint32_t PK_T = TP;                 // the tile length of this instantiation
    (void)PK_T;
    // (2 * PK_T + 64) / 4 groups of four keys over at least STG_T threads: at most STG per thread.  All
    // loads of a thread are issued before the first one is used (one memory latency, not STG of them).
    constexpr uint32_t STG_T = PT_THREADS - 64u;      // the fewest threads it is called with (kp_round: all waves but the walker)
    constexpr uint32_t STG = ((2u * PK_T + 64u) / 4u + STG_T - 1u) / STG_T;
    const uint32_t ngroups = (hl + 64u + 3u) >> 2;
    uint4 k[STG];
#pragma unroll
    for (uint32_t j = 0; j < STG; ++j) {
        const uint32_t i4 = (uint32_t)tid + j * (uint32_t)nthreads;
        if (i4 < ngroups && (i4 << 2) < hl) k[j] = ((const uint4*)gkey)[i4];
        else k[j] = uint4{0xFFFFFFFFu, 0xFFFFFFFFu, 0xFFFFFFFFu, 0xFFFFFFFFu};
    }
#pragma unroll
    for (uint32_t j = 0; j < STG; ++j) {
        const uint32_t i4 = (uint32_t)tid + j * (uint32_t)nthreads;
        if (i4 >= ngroups) continue;
        const uint32_t i = i4 << 2;
        const uint32_t nib = (s_bits[i >> 5] >> (i & 31u)) & 0xFu;        // i is a multiple of 4
        uint4 q = k[j];
        q.x = i + 0u < hl ? (q.x | ((nib & 1u) ? 0u : PK_DEAD)) : 0xFFFFFFFFu;
        q.y = i + 1u < hl ? (q.y | ((nib & 2u) ? 0u : PK_DEAD)) : 0xFFFFFFFFu;
        q.z = i + 2u < hl ? (q.z | ((nib & 4u) ? 0u : PK_DEAD)) : 0xFFFFFFFFu;
        q.w = i + 3u < hl ? (q.w | ((nib & 8u) ? 0u : PK_DEAD)) : 0xFFFFFFFFu;
        ((uint4*)s_key)[i4] = q;
    }
}

// repair next[]: players whose partner left the queue, or never computed.
//   repair_sweep   barrier-free; a wave looks at its own 64-player chunks (c = wv, wv + nwv, ...) and
//                  repairs what it finds itself, scanning up to RP_SHORT x 64 candidates per item.  An item
//                  whose first fit lies further away goes to the workgroup's long list (its next[] says
//                  NX_PEND meanwhile) — late in a tick a fit is thousands of positions away, and one
//                  wave walking there alone would keep the other fifteen waiting.
//   repair_long    the whole workgroup scans for every listed item, sixteen chunks abreast.
// The sweep runs twice per round in kp_round: by the waves that would otherwise idle during the
// walk (targets that had left the queue when the pass began: the lookahead tile's departures of the
// pass before), and again after the pass has been applied to the own tile (its own departures).
// gbits: the tile-local bitmap in HBM, for targets beyond the staged horizon (after a compaction).
#define NX_PEND 0xFFFDu              // on the long list (LDS copy only; never read by a walk or published)
#ifndef RP_SHORT
#define RP_SHORT 16u                 // 64-candidate steps a wave scans alone before an item goes to the long list
#endif
#define RP_GROUP 4u                  // waves that scan one long item abreast (16 / RP_GROUP items at a time)
#define RP_MAXLONG (PK_T / 32u < 256u ? PK_T / 32u : 256u)    // long list and its result slots: the first 2 x this of s_pc
// first index in [from, end) whose staged key fits (klo, krng), or PK_NO; gives up (returns PK_NO, *stop = where)
// once `limit` is reached.  Four 64-candidate steps per round trip to LDS.  Positions from `end` on are never
// matched (the staged keys are dead-padded for 64 entries behind the horizon only, so every step is bounded).
static __device__ __forceinline__ uint32_t scan4(const uint32_t* s_key, uint32_t klo, uint32_t krng, uint32_t from, uint32_t end,
                                                 uint32_t limit, uint32_t stride, int lane, uint32_t* stop, uint32_t& tst)
{
    uint32_t p = from;
    for (; p < limit; p += 4u * stride) {
        tst += 256u;                                      // (diagnostics: candidates tested, an upper bound of four steps)
        uint32_t kv[4];
#pragma unroll
        for (uint32_t u = 0; u < 4u; ++u) kv[u] = p + u * stride < end ? s_key[p + u * stride + (uint32_t)lane] : 0xFFFFFFFFu;
#pragma unroll
        for (uint32_t u = 0; u < 4u; ++u) {
            const unsigned long long b = __ballot(pk_in(kv[u], klo, krng));
            if (b) return p + u * stride + (uint32_t)__ffsll(b) - 1u;
        }
    }
    *stop = p;
    return PK_NO;
}

// s_todo: RP_TODO words of LDS of this wave's own (the items of its chunks, i | from << 16).
#define RP_TODO ((PK_T - 2u * RP_MAXLONG) / (PT_THREADS / 64u))      // per wave; all of it inside s_pc[PK_T + 64]
// what becomes of the item `ai` once its short scan has ended: the fit `j`, or — nobody within RP_SHORT steps, the scan
// stopped at `p` — the end of the horizon, or a place on the workgroup's long list
template <uint32_t TP>
static __device__ __forceinline__ void repair_finish(const uint32_t* s_key, uint16_t* s_nx, uint32_t* s_long, uint32_t* s_nlong,
                                                     uint32_t ai, uint32_t klo, uint32_t krng, uint32_t j, uint32_t p, uint32_t hl,
                                                     bool to_end, int lane, uint32_t& tst)
{
    constexpr uint32_t PK_T = TP;                 // the tile length of this instantiation
    (void)PK_T;
    uint32_t val;
    if (j != PK_NO) val = j - ai;
    else if (p >= hl) val = to_end ? NX_NONE : NX_FAR;
    else {
        uint32_t kx = 0;
        if (lane == 0) kx = atomicAdd(s_nlong, 1u);
        kx = lane_get(kx, 0);                             // lane 0's ticket for everybody
        if (kx < RP_MAXLONG) {
            if (lane == 0) s_long[kx] = ai | (p << 16);
            val = NX_PEND;
        } else {                                          // list full: this wave goes all the way
            j = scan4(s_key, klo, krng, p, hl, hl, 64u, lane, &p, tst);
            val = j != PK_NO ? j - ai : (to_end ? NX_NONE : NX_FAR);
        }
    }
    if (lane == 0) lds_st16(s_nx + ai, (uint16_t)val);
}

template <uint32_t TP>
static __device__ __forceinline__ void repair_item(const uint32_t* s_key, uint16_t* s_nx, uint32_t* s_long, uint32_t* s_nlong,
                                                   uint32_t ai, uint32_t af, uint32_t hl, bool to_end, uint32_t w, int lane, uint32_t& tst)
{
    constexpr uint32_t PK_T = TP;                 // the tile length of this instantiation
    (void)PK_T;
    uint32_t klo, krng;
    pk_bounds(s_key[ai] & ~PK_DEAD, w, klo, krng);
    uint32_t p = af;
    const uint32_t j = scan4(s_key, klo, krng, af, hl, dev_min_u32(hl, af + RP_SHORT * 64u), 64u, lane, &p, tst);
    repair_finish<PK_T>(s_key, s_nx, s_long, s_nlong, ai, klo, krng, j, p, hl, to_end, lane, tst);
}

// (Round 5, built, measured and taken out: repair_item2 — two items of a wave scanned side by side, their round trips to
// LDS overlapping.  Same values; cfg-2 9.77-9.96 ms a step without it against 10.03-10.31 with it on one box
// (profiles/r05_ab_pair_micro.txt): the tile work is bound by instruction ISSUE on the tile's one CU, and the masked
// second stream of reads is more instructions per trip, whatever latency it hides.)

// Detection of one wave's chunks (c = wv, wv + nwv, ...), straight-line code: the LDS reads of all its
// chunks are in flight together.  The players that need a repair are packed (i | from << 16) into
// `list` — the wave's own when `shared_cnt` is null (*n_own = how many), else the workgroup's list, whose
// length is kept in *shared_cnt.  What does not fit the list is repaired on the spot.
template <uint32_t TP, uint32_t MAXC>
static __device__ __forceinline__ void repair_detect(const uint32_t* s_key, uint16_t* s_nx, uint32_t* s_long, uint32_t* s_nlong,
                                                     uint32_t* list, uint32_t cap, uint32_t* shared_cnt, uint32_t* n_own,
                                                     const uint32_t* gbits, uint32_t tl, uint32_t hl, bool to_end,
                                                     uint32_t w, int lane, uint32_t wv, uint32_t nwv, uint32_t& tst)
{
    constexpr uint32_t PK_T = TP;                 // the tile length of this instantiation
    (void)PK_T;
    constexpr uint32_t NCH = PK_T / 64u;                  // chunks of the tile
    uint32_t ki[MAXC], oo[MAXC], kq[MAXC], from[MAXC];
#pragma unroll
    for (uint32_t k = 0; k < MAXC; ++k) {
        const uint32_t i = dev_min_u32(((wv + k * nwv) << 6) + (uint32_t)lane, PK_T - 1u);
        ki[k] = s_key[i];
        oo[k] = lds_ld16(s_nx + i);
    }
#pragma unroll
    for (uint32_t k = 0; k < MAXC; ++k) {
        const uint32_t i = ((wv + k * nwv) << 6) + (uint32_t)lane;
        kq[k] = s_key[dev_min_u32(i + oo[k], hl)];                  // s_key[hl]: dead padding
    }
    uint32_t tot = 0;
#pragma unroll
    for (uint32_t k = 0; k < MAXC; ++k) {
        const uint32_t c8 = wv + k * nwv;
        const uint32_t i = (c8 << 6) + (uint32_t)lane;
        const uint32_t o = oo[k], q = i + o;
        const bool mine = c8 < NCH && i < tl && !(ki[k] & PK_DEAD);
        const bool ptr = o != NX_INV && o != NX_NONE && o != NX_FAR && o != NX_PEND;
        bool tdead = (kq[k] & PK_DEAD) != 0u;
        if (__ballot(mine && ptr && q >= hl)) {                     // behind the staged horizon (after a compaction): ask HBM
            if (mine && ptr && q >= hl) tdead = !((xld(gbits + (q >> 5)) >> (q & 31u)) & 1u);   // (another workgroup's words: past the L1)
        }
        from[k] = !mine ? 0u : (o == NX_INV ? i + 1u : ((ptr && tdead) ? q + 1u : 0u));
        tot += (uint32_t)__popcll(__ballot(from[k] != 0u));
    }
    uint32_t cnt = 0;
    if (shared_cnt) {
        if (tot) {
            if (lane == 0) cnt = atomicAdd(shared_cnt, tot);
            cnt = lane_get(cnt, 0);
        }
    }
    const unsigned long long below = (1ull << lane) - 1ull;
#pragma unroll
    for (uint32_t k = 0; k < MAXC; ++k) {
        const uint32_t c8 = wv + k * nwv;
        const uint32_t i = (c8 << 6) + (uint32_t)lane;
        const unsigned long long nb = __ballot(from[k] != 0u);
        const uint32_t slot = cnt + (uint32_t)__popcll(nb & below);
        if (from[k] != 0u && slot < cap) list[slot] = i | (from[k] << 16);
        const uint32_t nxt = cnt + (uint32_t)__popcll(nb);
        if (nxt > cap) {                                            // the list is full: these go right away
            unsigned long long rest = nb;
            while (rest) {
                const int l = __ffsll(rest) - 1;
                rest &= rest - 1ull;
                if (cnt + (uint32_t)__popcll(nb & ((1ull << l) - 1ull)) >= cap)
                    repair_item<PK_T>(s_key, s_nx, s_long, s_nlong, (c8 << 6) + (uint32_t)l, lane_get(from[k], l), hl, to_end, w, lane, tst);
            }
        }
        cnt = nxt;
    }
    if (n_own) *n_own = dev_min_u32(cnt, cap);
}

// One wave sweeps its chunks and repairs what it finds (barrier-free: kp_round's sweep during the walk).
template <uint32_t TP>
static __device__ __forceinline__ void repair_sweep(const uint32_t* s_key, uint16_t* s_nx, uint32_t* s_long, uint32_t* s_nlong,
                                                    uint32_t* s_todo, const uint32_t* gbits, uint32_t tl, uint32_t hl, bool to_end,
                                                    uint32_t w, int lane, uint32_t wv, uint32_t nwv, uint32_t& tst)
{
    constexpr uint32_t PK_T = TP;                 // the tile length of this instantiation
    (void)PK_T;
    uint32_t cnt = 0;
    repair_detect<PK_T, (PK_T / 64u + 12u) / 13u>(s_key, s_nx, s_long, s_nlong, s_todo, RP_TODO, nullptr, &cnt, gbits, tl, hl, to_end,
                                            w, lane, wv, nwv, tst);      // thirteen or more waves sweep
    wave_lockstep();
    for (uint32_t it = 0; it < cnt; ++it) {
        const uint32_t item = uni(s_todo[it]);
        repair_item<PK_T>(s_key, s_nx, s_long, s_nlong, item & 0xFFFFu, item >> 16, hl, to_end, w, lane, tst);
    }
}

// Every thread of the workgroup calls it, after a barrier behind the last sweep.  s_found[0 .. RP_MAXLONG)
// must hold PK_NO.  Ends with the long list empty again (counter and s_found reset) behind a barrier.
template <uint32_t TP>
static __device__ __forceinline__ void repair_long(const uint32_t* s_key, uint16_t* s_nx, const uint32_t* s_long,
                                                   uint32_t* s_found, uint32_t* s_nlong, uint32_t hl, bool to_end,
                                                   uint32_t w, int tid, uint32_t& tst)
{
    constexpr uint32_t PK_T = TP;                 // the tile length of this instantiation
    (void)PK_T;
    const int lane = tid & 63;
    const uint32_t wave = (uint32_t)tid >> 6;
    const uint32_t nlong = dev_min_u32(*s_nlong, RP_MAXLONG);
    const uint32_t ngroups = (PT_THREADS / 64u) / RP_GROUP, grp = wave / RP_GROUP, gw = wave % RP_GROUP;
    for (uint32_t it = grp; it < nlong; it += ngroups) {
        const uint32_t item = s_long[it];
        const uint32_t ai = item & 0xFFFFu, p0 = item >> 16;
        uint32_t klo, krng;
        pk_bounds(s_key[ai] & ~PK_DEAD, w, klo, krng);
        for (uint32_t p = p0 + gw * 64u; p < hl;) {
            if (uni(lds_ld(s_found + it)) < p) break;             // somebody found a fit in front of here
            uint32_t stop = p;
            const uint32_t j = scan4(s_key, klo, krng, p, hl, dev_min_u32(hl, p + 1u), RP_GROUP * 64u, lane, &stop, tst);   // four stripes
            if (j != PK_NO) {
                if (lane == 0) atomicMin(s_found + it, j);
                break;
            }
            p = stop;
        }
    }
    __syncthreads();
    for (uint32_t it = tid; it < nlong; it += PT_THREADS) {
        const uint32_t ai = s_long[it] & 0xFFFFu, f = s_found[it];
        s_nx[ai] = (uint16_t)(f != PK_NO ? f - ai : (to_end ? NX_NONE : NX_FAR));
        s_found[it] = PK_NO;
    }
    __syncthreads();
    if (tid == 0) *s_nlong = 0;
}

// the whole repair of a tile by the whole workgroup (kp_round's second sweep): all sixteen
// waves detect into ONE list, then pull items from it one by one (a wave whose chunks hold many
// items would otherwise keep the other fifteen waiting), then scan for the far ones together.
// ctl[0] = long list length, ctl[1] = list length, ctl[2] = pull cursor (all zero on entry, behind a barrier).
// s_long = scratch: [0, RP_MAXLONG) long list, [RP_MAXLONG, 2 RP_MAXLONG) its result slots (PK_NO), then the list.
template <uint32_t TP>
static __device__ __forceinline__ void prep_repair(const uint32_t* s_key, uint16_t* s_nx, uint32_t* s_long, uint32_t* ctl,
                                                   const uint32_t* gbits, uint32_t tl, uint32_t hl, bool to_end, uint32_t w,
                                                   int tid, uint32_t& tst, uint32_t* tmv = nullptr)
{
    constexpr uint32_t PK_T = TP;                 // the tile length of this instantiation
    (void)PK_T;
    const int lane = tid & 63;
    uint32_t* const list = s_long + 2u * RP_MAXLONG;
    constexpr uint32_t CAP = PK_T - 2u * RP_MAXLONG;
    long long tq = tmv ? clock64() : 0;
    repair_detect<PK_T, (PK_T / 64u + PT_THREADS / 64u - 1u) / (PT_THREADS / 64u)>(s_key, s_nx, s_long, &ctl[0], list, CAP, &ctl[1], nullptr,
                                                                           gbits, tl, hl, to_end, w, lane, (uint32_t)tid >> 6,
                                                                           PT_THREADS / 64u, tst);
    __syncthreads();
    if (tmv) { const long long now = clock64(); tmv[1] += (uint32_t)(now - tq); tq = now; }
    const uint32_t n = dev_min_u32(ctl[1], CAP);
    // round robin over the one list: neighbours in the list (players of one chunk, often pointing at the same
    // departed partner) go to different waves.  (A ticket counter pulled by lane 0 inside this loop was
    // miscompiled into a loop that never takes a new ticket on gfx950 / ROCm 7.2: keep the loop counted.)
    for (uint32_t it = (uint32_t)tid >> 6; it < n; it += PT_THREADS / 64u) {
        const uint32_t i0 = uni(list[it]);
        repair_item<PK_T>(s_key, s_nx, s_long, &ctl[0], i0 & 0xFFFFu, i0 >> 16, hl, to_end, w, lane, tst);
    }

    __syncthreads();
    if (tmv) { const long long now = clock64(); tmv[12] += (uint32_t)(now - tq); tmv[11] += ctl[0]; tmv[14] += n; tq = now; }
    repair_long<PK_T>(s_key, s_nx, s_long, s_long + RP_MAXLONG, &ctl[0], hl, to_end, w, tid, tst);
    if (tid == 0) { ctl[1] = 0; ctl[2] = 0; }
    __syncthreads();
    if (tmv) { const long long now = clock64(); tmv[2] += (uint32_t)(now - tq); }
}

// step graph of the tile: node x in [0, PK_T]; PK_T = "left the tile, lobby empty".
//   queued x with its partner inside the tile -> first queued player after the partner (one
//   match); queued x otherwise -> itself (exit anchor); x not queued -> next queued.
// s_nw[w] = first queued index at or after word w (PK_T if none) makes "first queued at or
// after p" two loads and no loop.  Also writes g16 (the single step, for the in-tile chain).
static __device__ __forceinline__ void prep_build(const uint32_t* s_key, const uint16_t* s_nx, const uint32_t* s_bits,
                                                  uint16_t* s_nw, uint32_t* s_pc, uint16_t* gg, uint32_t tl, int tid)
{
    const uint32_t nwords_own = (tl + 31u) >> 5;
    for (uint32_t wv = tid; wv <= PK_T / 32u; wv += PT_THREADS) {
        uint32_t ww = wv, r = PK_T;
        while (ww < nwords_own) {
            const uint32_t bw = s_bits[ww];
            if (bw) { r = (ww << 5) + (uint32_t)__ffs((int)bw) - 1u; break; }
            ++ww;
        }
        s_nw[wv] = (uint16_t)(r < tl ? r : PK_T);
    }
    __syncthreads();
    for (uint32_t x0 = 2u * tid; x0 <= PK_T; x0 += 2u * PT_THREADS) {
        uint32_t gpair = 0;
#pragma unroll
        for (uint32_t h = 0; h < 2u; ++h) {
            const uint32_t x = x0 + h;
            uint32_t v = PK_T, gx = PK_T;                           // beyond the queue
            if (x < tl) {
                const bool alive = !(s_key[x] & PK_DEAD);
                const uint32_t o = alive ? (uint32_t)s_nx[x] : 0u;
                const bool internal = alive && o != NX_NONE && o != NX_FAR && x + o < tl;
                if (alive && !internal) v = x;                      // exit anchor: terminal
                else {
                    const uint32_t from = internal ? x + o + 1u : x + 1u;
                    const uint32_t wi = from >> 5;                  // <= PK_T / 32
                    const uint32_t bw = wi < nwords_own ? s_bits[wi] & (0xFFFFFFFFu << (from & 31u)) : 0u;
                    uint32_t nxt = bw ? (wi << 5) + (uint32_t)__ffs((int)bw) - 1u : (uint32_t)s_nw[wi < PK_T / 32u ? wi + 1u : PK_T / 32u];
                    if (nxt >= tl) nxt = PK_T;
                    v = nxt | (internal ? 1u << 16 : 0u);
                    if (internal) gx = nxt;
                }
            }
            if (x <= PK_T) s_pc[x] = v;
            gpair |= gx << (16u * h);
        }
        if (x0 < tl) *(uint32_t*)(gg + x0) = gpair;
    }
}

// resolve every node to the terminal its path ends at (exit anchor, or PK_T) and the matches
// on the way: asynchronous pointer jumping, no barrier inside.
//   A node word is  ptr (bits 0-14) | final (15) | matches on the way (16-31).  Steps only go
//   forward (ptr > x), terminals point at themselves.  Every thread owns the nodes x = tid + k *
//   PT_THREADS and is the only writer of their words; it replaces (ptr, cnt) by (ptr of ptr,
//   cnt + cnt of ptr) — with whatever the target's word holds at that moment: any word ever
//   stored for a node is a valid jump from it, so a stale read only costs a step — until the
//   target is final.  A jump strictly increases ptr (a node that is not final never points at
//   itself: the terminals are marked before the barrier), so every node ends, in about
//   log2(matches per tile) sweeps instead of one dependent step per span.
static __device__ __forceinline__ void prep_resolve(uint32_t* s_pc, int tid)
{
    constexpr uint32_t NPT = (PK_T + PT_THREADS - 1u) / PT_THREADS;     // nodes per thread (8 at the product geometry)
    uint32_t v[NPT];
    uint32_t open = 0;                                    // bit k: node k of this thread is not final yet
#pragma unroll
    for (uint32_t k = 0; k < NPT; ++k) {
        const uint32_t x = (uint32_t)tid + k * PT_THREADS;
        if (x < PK_T) {
            v[k] = s_pc[x];
            const uint32_t px = v[k] & 0x7FFFu;
            if (px == x || px == PK_T) { v[k] |= 0x8000u; s_pc[x] = v[k]; }   // exit anchor / leaves the tile: terminal
            else open |= 1u << k;
        } else v[k] = 0x8000u;
    }
    if (tid == 0) s_pc[PK_T] = PK_T | 0x8000u;
    __syncthreads();
    while (__ballot(open != 0u)) {
#pragma unroll
        for (uint32_t kk = 0; kk < NPT; ++kk) {
            const uint32_t k = NPT - 1u - kk;             // back to front: the high nodes finish first
            if (open & (1u << k)) {
                const uint32_t v2 = lds_ld(s_pc + (v[k] & 0x7FFFu));
                uint32_t nv = (v2 & 0x7FFFu) | ((v[k] & 0xFFFF0000u) + (v2 & 0xFFFF0000u));
                if (v2 & 0x8000u) { nv |= 0x8000u; open &= ~(1u << k); }
                v[k] = nv;
                lds_st(s_pc + (uint32_t)tid + k * PT_THREADS, nv);
            }
        }
    }
}

// publish: REC for every entry position (and, when asked, the exit anchor itself), next[] back
static __device__ __forceinline__ void prep_publish(const uint32_t* s_pc, const uint16_t* s_nx, uint32_t* rec, uint16_t* exa,
                                                    uint16_t* gnx, uint32_t tl, int tid)
{
    for (uint32_t x = tid; x < tl; x += PT_THREADS) {
        const uint32_t v = s_pc[x];
        const uint32_t e = v & 0x7FFFu, cnt = v >> 16;
        uint32_t r;
        if (e >= tl) r = rec_make(REC_CLEAN, cnt, PK_T);
        else {
            const uint32_t o = s_nx[e];
            if (o == NX_NONE) r = rec_make(REC_NONE, cnt, e);
            else if (o == NX_FAR) r = rec_make(REC_FAR, cnt, e);
            else r = rec_make(REC_PARTNER, cnt, e + o + 1u);
        }
        rec[x] = r;
        if (exa) exa[x] = (uint16_t)e;
    }
    uint4* const nx4 = (uint4*)gnx;
    for (uint32_t i = tid; i < (tl + 7u) >> 3; i += PT_THREADS) nx4[i] = ((const uint4*)s_nx)[i];
}

// prep_build + prep_resolve + prep_publish for kp_round in one piece: every thread keeps its nodes
// x = tid + k * PT_THREADS in registers from the step graph to the published REC, and all the LDS
// reads of a thread's nodes are issued together (the three separate functions walk the tile three
// times, one dependent LDS read after another).  Same tables, same values.
template <uint32_t TP>
static __device__ __forceinline__ void prep_tables(const uint32_t* s_key, const uint16_t* s_nx, const uint32_t* s_bits,
                                                   uint16_t* s_nw, uint32_t* s_pc, uint16_t* gg, uint32_t* rec, uint16_t* exa,
                                                   uint16_t* gnx, uint32_t tl, int tid, uint32_t* tmv = nullptr)
{
    constexpr uint32_t PK_T = TP;                 // the tile length of this instantiation
    (void)PK_T;
    long long tq = tmv ? clock64() : 0;
#define PT_MARK(K) do { if (tmv) { const long long now = clock64(); tmv[K] += (uint32_t)(now - tq); tq = now; } } while (0)
    constexpr uint32_t NPT = (PK_T + PT_THREADS - 1u) / PT_THREADS;     // nodes per thread (8 at the product geometry)
    const int lane = tid & 63;
    (void)lane;
    // ---- first queued index at or after every bitmap word (prep_build, first half) ----
    const uint32_t nwords_own = (tl + 31u) >> 5;
    for (uint32_t wv = tid; wv <= PK_T / 32u; wv += PT_THREADS) {
        uint32_t ww = wv, r = PK_T;
        while (ww < nwords_own) {
            const uint32_t bw = s_bits[ww];
            if (bw) { r = (ww << 5) + (uint32_t)__ffs((int)bw) - 1u; break; }
            ++ww;
        }
        s_nw[wv] = (uint16_t)(r < tl ? r : PK_T);
    }
    // ---- step graph: the reads that do not need s_nw first, branch free (all in flight together) ----
    uint32_t v[NPT], from[NPT], bw[NPT], kx[NPT], ox[NPT];
    bool internal[NPT];
#pragma unroll
    for (uint32_t k = 0; k < NPT; ++k) {
        const uint32_t x = dev_min_u32((uint32_t)tid + k * PT_THREADS, PK_T - 1u);
        kx[k] = s_key[x];
        ox[k] = s_nx[x];
    }
#pragma unroll
    for (uint32_t k = 0; k < NPT; ++k) {
        const uint32_t x = (uint32_t)tid + k * PT_THREADS;
        const bool in = x < tl;
        const bool alive = in && !(kx[k] & PK_DEAD);
        const uint32_t o = ox[k];
        internal[k] = alive && o != NX_NONE && o != NX_FAR && o != NX_INV && x + o < tl;
        const bool term = alive && !internal[k];
        from[k] = (!in || term) ? PK_NO : (internal[k] ? x + o + 1u : x + 1u);
        v[k] = term ? (x | 0x8000u) : (PK_T | 0x8000u);         // exit anchor: terminal; beyond the queue: leaves the tile
        const uint32_t wi = dev_min_u32(from[k] >> 5, PK_T / 32u);  // from <= PK_T when it is a position
        const uint32_t word = s_bits[wi];
        bw[k] = (from[k] != PK_NO && wi < nwords_own) ? word & (0xFFFFFFFFu << (from[k] & 31u)) : 0u;
    }
    __syncthreads();                                            // s_nw
    uint32_t open = 0;                                          // bit k: node k of this thread is not final yet
#pragma unroll
    for (uint32_t k = 0; k < NPT; ++k) {
        const uint32_t x = (uint32_t)tid + k * PT_THREADS;
        uint32_t gx = PK_T;
        if (from[k] != PK_NO) {
            const uint32_t wi = from[k] >> 5;
            uint32_t nxt = bw[k] ? (wi << 5) + (uint32_t)__ffs((int)bw[k]) - 1u
                                 : (uint32_t)s_nw[wi < PK_T / 32u ? wi + 1u : PK_T / 32u];
            if (nxt >= tl) nxt = PK_T;
            v[k] = nxt | (internal[k] ? 1u << 16 : 0u);
            if (nxt == PK_T) v[k] |= 0x8000u;                   // leaves the tile: final
            else open |= 1u << k;
            if (internal[k]) gx = nxt;
        }
        if (x < PK_T) s_pc[x] = v[k];
        if (x < tl) gg[x] = (uint16_t)gx;                       // g16: the single step, for the in-tile chain
    }
    if (tid == 0) s_pc[PK_T] = PK_T | 0x8000u;
    __syncthreads();
    PT_MARK(7);
    // ---- resolve (prep_resolve): asynchronous pointer jumping on the nodes still open ----
    while (__ballot(open != 0u)) {
#pragma unroll
        for (uint32_t kk = 0; kk < NPT; ++kk) {
            const uint32_t k = NPT - 1u - kk;                   // back to front: the high nodes finish first
            if (open & (1u << k)) {
                const uint32_t v2 = lds_ld(s_pc + (v[k] & 0x7FFFu));
                uint32_t nv = (v2 & 0x7FFFu) | ((v[k] & 0xFFFF0000u) + (v2 & 0xFFFF0000u));
                if (v2 & 0x8000u) { nv |= 0x8000u; open &= ~(1u << k); }
                v[k] = nv;
                lds_st(s_pc + (uint32_t)tid + k * PT_THREADS, nv);
            }
        }
    }
    PT_MARK(8);
    // ---- publish (prep_publish) from the registers ----
    uint32_t ex[NPT], on[NPT];
#pragma unroll
    for (uint32_t k = 0; k < NPT; ++k) {
        ex[k] = v[k] & 0x7FFFu;
        on[k] = ex[k] < tl ? (uint32_t)s_nx[ex[k]] : NX_NONE;
    }
#pragma unroll
    for (uint32_t k = 0; k < NPT; ++k) {
        const uint32_t x = (uint32_t)tid + k * PT_THREADS;
        if (x >= tl) continue;
        const uint32_t e = ex[k], cnt = v[k] >> 16, o = on[k];
        uint32_t r;
        if (e >= tl) r = rec_make(REC_CLEAN, cnt, PK_T);
        else if (o == NX_NONE) r = rec_make(REC_NONE, cnt, e);
        else if (o == NX_FAR) r = rec_make(REC_FAR, cnt, e);
        else r = rec_make(REC_PARTNER, cnt, e + o + 1u);
        rec[x] = r;
        exa[x] = (uint16_t)e;
    }
    if (gnx) {                                                  // (kp_rounds keeps next[] in LDS from pass to pass)
        uint4* const nx4 = (uint4*)gnx;
        for (uint32_t i = tid; i < (tl + 7u) >> 3; i += PT_THREADS) nx4[i] = ((const uint4*)s_nx)[i];
    }
    PT_MARK(10);
#undef PT_MARK
}


// ------------------------------------------------------------------------------------
// The pass that kp_round and kp_rounds share.  Both kernels do the same round by design — walk the route
// of the pass, apply it to the own tile, prepare the tile for the next one — once per launch (kp_round) or for a
// batch of passes with the tile resident in LDS (kp_rounds), and kp_round is where every stop of kp_rounds goes
// on: the two must never differ in what a pass is.  So everything of the pass that does not depend on how a
// workgroup gets at its data is written once, here:
//
//   pair_wg_map, PairTile                   which (chain, tile) a workgroup is, and the tile's geometry
//   round_state_open / round_state_commit   RoundState <-> the chain's committed record (also kp_round_commit)
//   PassEmit                                a thread's deferred lobby: loads early, stores late
//   PairWalk, walk_head, walk_general_hop,  the walk's running state, the carried anchor's head match, a hop
//   walk_close                              that is not of the fast kind, the state behind the pass
//   pass_apply                              section 2: the pass on the own tile
//   head_first_fit                          the carried anchor's first fit in the tile, for the next pass
//
// The one systematic difference is how the walk reads what OTHER workgroups wrote: the previous launch did
// (kp_round: plain loads) or this one (kp_rounds: past the vector L1) — a policy type, LdLaunch / LdPeer.
// What a kernel owns: its staging and L2 pull (kp_round) or lookahead refresh and flag barrier (kp_rounds), its
// fast path (kp_round's knows the second route level, kp_rounds's is tw_hops), what follows the publication,
// the order of the sections and every barrier between them.
// Nothing here reads threadIdx: kp_rounds hands in the index it launders once per iteration (TW_LAUNDER), and
// what is derived from it must not be hoisted out of that loop.
// ------------------------------------------------------------------------------------

// Wave-wide: first queued index in [from, m) whose key fits akey (HBM keys + bitmap), or PK_NO.
static __device__ __forceinline__ uint32_t w_scan_fit(const uint32_t* key, const uint32_t* bits, uint32_t akey, uint32_t from, uint32_t m,
                                      uint32_t w, int lane)
{
    uint32_t klo, krng;
    pk_bounds(akey, w, klo, krng);
    for (uint32_t p = from; p < m; p += 64u) {
        const uint32_t c = p + (uint32_t)lane;
        bool ok = false;
        if (c < m && ((bits[c >> 5] >> (c & 31u)) & 1u)) ok = pk_in(key[c], klo, krng);
        const unsigned long long b = __ballot(ok);
        if (b) return p + (uint32_t)__ffsll(b) - 1u;
    }
    return PK_NO;
}

// Wave-wide, like w_scan_fit, on a bitmap other workgroups of this launch have written.
static __device__ __forceinline__ uint32_t w_scan_fit_x(const uint32_t* key, const uint32_t* bits, uint32_t akey, uint32_t from, uint32_t m,
                                                        uint32_t w, int lane)
{
    uint32_t klo, krng;
    pk_bounds(akey, w, klo, krng);
    // four 64-candidate steps per trip to memory, bitmap words and keys side by side (round 5: one step a trip, the key
    // behind its bitmap word — 5.4k cycles for each of the ~50 hops a tick whose partner has just left, on every tile's walker)
    for (uint32_t p = from; p < m; p += 256u) {
        uint32_t bw[4], kv[4];
#pragma unroll
        for (uint32_t u = 0; u < 4u; ++u) {
            const uint32_t c = p + 64u * u + (uint32_t)lane;
            bw[u] = c < m ? xld(bits + (c >> 5)) : 0u;
            kv[u] = c < m ? key[c] : 0xFFFFFFFFu;
        }
#pragma unroll
        for (uint32_t u = 0; u < 4u; ++u) {
            const uint32_t c = p + 64u * u + (uint32_t)lane;
            const unsigned long long b = __ballot(((bw[u] >> (c & 31u)) & 1u) != 0u && pk_in(kv[u], klo, krng));
            if (b) return p + 64u * u + (uint32_t)__ffsll(b) - 1u;
        }
    }
    return PK_NO;
}

// How the walk reads REC, exit anchors, head partners and the pass-start bitmap of other tiles.
struct LdLaunch {                    // the previous launch wrote them (kp_round)
    static __device__ __forceinline__ uint32_t ld(const uint32_t* p) { return *p; }
    static __device__ __forceinline__ uint32_t ld16(const uint16_t* p) { return *p; }
    static __device__ __forceinline__ uint32_t scan_fit(const uint32_t* key, const uint32_t* bits, uint32_t akey, uint32_t from, uint32_t m,
                                                        uint32_t w, int lane) { return w_scan_fit(key, bits, akey, from, m, w, lane); }
};
struct LdPeer {                      // workgroups of this launch did, in front of a flag barrier (kp_rounds)
    static __device__ __forceinline__ uint32_t ld(const uint32_t* p) { return xld(p); }
    static __device__ __forceinline__ uint32_t ld16(const uint16_t* p) { return xld16(p); }
    static __device__ __forceinline__ uint32_t scan_fit(const uint32_t* key, const uint32_t* bits, uint32_t akey, uint32_t from, uint32_t m,
                                                        uint32_t w, int lane) { return w_scan_fit_x(key, bits, akey, from, m, w, lane); }
};

// The workgroup's (rating group, tile) under the batch's map (PairParams.xseg), and its place among the chain's
// workgroups of its XCD (xj of xn; PK_NO / 0 on the plain grid).  false: a slot nobody walks.
static __device__ __forceinline__ bool pair_wg_map(const PairParams& P, uint32_t& g, uint32_t& t, uint32_t& xj, uint32_t& xn)
{
    g = blockIdx.y; t = blockIdx.x;
    xj = PK_NO; xn = 0;
    if (!P.xslots) return true;
    const uint32_t x = blockIdx.x & 7u;
    uint32_t sl = blockIdx.x >> 3;
    bool found = false;
#pragma unroll
    for (uint32_t k = 0; k < PK_XSEG; ++k) {
        const uint32_t c = P.xcnt[x][k];
        if (!found && sl < c) {
            const uint32_t sg = P.xseg[x][k];
            g = sg & 0xFFu;
            t = ((sg >> 8) & 0xFFu) + sl * (sg >> 16);
            xj = sl; xn = c;
            found = true;
        }
        if (!found) sl -= c;
    }
    return found;
}

// Tile t of rating group g in a chain of m index positions (m, buf: what the host saw, from the kernel arguments).
template <uint32_t TP>
struct PairTile {
    uint32_t m, buf, ntiles;
    uint32_t base, tl, hl;           // first index; length of the tile; of the tile and its lookahead tile
    uint32_t own_words, hwords;      // bitmap words of tl / of hl
    size_t qo, po;                   // the chain's offset in the q_* arrays / the group's in the pair arrays
    const uint32_t* key;
    const uint32_t* oidx;
    uint16_t* gnx;                   // next[] of the tile
    __device__ __forceinline__ PairTile(const PairParams& P, uint32_t g, uint32_t t, uint32_t m_, uint32_t buf_)
    {
        m = m_; buf = buf_;
        ntiles = (m + TP - 1u) / TP;
        qo = (size_t)(P.mode * P.n_groups + g) * P.capacity;
        po = (size_t)g * P.pstride;
        base = t * TP;
        tl = dev_min_u32(TP, m - base);
        hl = dev_min_u32(2u * TP, m - base);
        own_words = (tl + 31u) >> 5;
        hwords = (hl + 31u) >> 5;
        key = P.key[buf] + po;
        oidx = P.oidx[buf] + po;
        gnx = P.nx16[buf] + po + base;
    }
};

// The chain's committed record as the state a batch starts from / a batch's last state back into the record.
static __device__ __forceinline__ RoundState round_state_open(const PairChain* pc)
{
    RoundState S;
    S.live = 1; S.done = 0; S.want_compact = 0; S.rounds = pc->rounds; S.a_oi = PK_NO;
    S.qlen = pc->qlen; S.passes = pc->passes; S.n_out = pc->n_out; S.has_anchor = pc->has_anchor;
    S.a_key = pc->a_key; S.a_slot = pc->a_slot; S.a_cons = pc->a_cons; S.a_team = pc->a_team;
    S.a_rating = pc->a_rating; S.pairs = pc->pairs; S.scanned = pc->scanned;
    S.pos0 = pc->pos0; S.changed0 = pc->changed0; S.extra0 = pc->extra0;
    return S;
}
static __device__ __forceinline__ void round_state_commit(PairChain* pc, const RoundState& S)
{
    pc->qlen = S.qlen; pc->passes = S.passes; pc->n_out = S.n_out; pc->has_anchor = S.has_anchor;
    pc->a_key = S.a_key; pc->a_slot = S.a_slot; pc->a_cons = S.a_cons; pc->a_team = S.a_team;
    pc->a_rating = S.a_rating; pc->pairs = S.pairs; pc->scanned = S.scanned; pc->rounds = S.rounds;
    pc->want_compact = S.want_compact;
    pc->pos0 = S.pos0; pc->changed0 = S.changed0; pc->extra0 = S.extra0;
}

// The deferred lobby of a thread (section 2): two dependent loads per player (oidx -> q_slot) and four stores,
// none of which anything in the launch waits for.  pass_apply issues the first loads, load() the second ones
// (behind the repair), store() the stores (at the end) — the workgroup does not stand at a barrier for them.
struct PassEmit {
    uint32_t em_off = PK_NO, em_ia = 0, em_iq = 0, em_score = 0, em_sa = 0, em_sq = 0;     // a step of the in-tile path
    uint32_t hd_off = PK_NO, hd_iq = 0, hd_score = 0, hd_sq = 0, hd_sa = 0, hd_team = 0;   // the head match (thread 0)
    uint32_t pass = 0;
    bool loaded = false;
    __device__ __forceinline__ void load(const PairParams& P, size_t qo)
    {
        if (loaded) return;
        loaded = true;
        if (em_off != PK_NO) { em_sa = P.q_slot[qo + em_ia]; em_sq = P.q_slot[qo + em_iq]; }
        if (hd_off != PK_NO) hd_sq = P.q_slot[qo + hd_iq];
    }
    __device__ __forceinline__ void store(const PairParams& P, uint32_t g, size_t qo)
    {
        load(P, qo);
        uint32_t* const eos = P.out_slots + (size_t)g * P.out_slot_stride;
        if (em_off != PK_NO) {
            eos[2u * em_off] = em_sa; eos[2u * em_off + 1u] = em_sq;
            P.out_score[(size_t)g * P.out_rec_stride + em_off] = (float)(int32_t)em_score;
            P.out_pass[(size_t)g * P.out_rec_stride + em_off] = pass;
        }
        if (hd_off != PK_NO) {
            eos[2u * hd_off + hd_team] = hd_sa; eos[2u * hd_off + (1u - hd_team)] = hd_sq;
            P.out_score[(size_t)g * P.out_rec_stride + hd_off] = (float)(int32_t)hd_score;
            P.out_pass[(size_t)g * P.out_rec_stride + hd_off] = pass;
        }
        em_off = PK_NO; hd_off = PK_NO;
    }
};

// The walk's running state (wave 0, everything wave uniform).
struct PairWalk {
    uint32_t tt, x;                  // the cursor: tile, position in it
    uint32_t k;                      // lobbies of the pass so far
    bool have_r;                     // rpre is the REC at the cursor
    uint32_t rpre;
    uint32_t my_entry, my_off, my_disp, my_kill, my_head, my_hoff;   // the own tile's share of the route (s_my[0..5])
    uint32_t has_anchor, a_key, a_team;                              // the open lobby behind the cursor
    uint32_t a_oi;                   // the seated anchor's index in the q_* arrays (slot, rating, cons are fetched off the walk)
    bool quiescent;
    __device__ __forceinline__ PairWalk(const RoundState& S, uint32_t a_oi_)
        : tt(0), x(S.pos0), k(0), have_r(false), rpre(0), my_entry(PK_NO), my_off(0), my_disp(DISP_NONE), my_kill(PK_NO),
          my_head(0), my_hoff(0), has_anchor(S.has_anchor), a_key(S.a_key), a_team(S.a_team), a_oi(a_oi_), quiescent(false) {}
    __device__ __forceinline__ void publish(uint32_t* s_my) const
    {
        s_my[0] = my_entry; s_my[1] = my_off; s_my[2] = my_disp; s_my[3] = my_kill; s_my[4] = my_head; s_my[5] = my_hoff;
        s_my[6] = 0; s_my[7] = 0;
    }
};

// Head match: the carried anchor's partner is the first tile's prepared first fit that exists (hp: one word per
// tile).  `early`: hp0 is the word of this lane's tile among the first 64, loaded ahead.
template <uint32_t TP, class Ld>
static __device__ __forceinline__ void walk_head(PairWalk& W, const PairTile<TP>& G, uint32_t t, const uint32_t* hp, uint32_t n_out, int lane,
                                                 bool early = false, uint32_t hp0 = PK_NO)
{
    if (!W.has_anchor) return;
    uint32_t j = PK_NO;
    for (uint32_t tb = 0; tb < G.ntiles && j == PK_NO; tb += 64u) {
        const uint32_t v = early && tb == 0u ? hp0 : (tb + (uint32_t)lane < G.ntiles ? Ld::ld(hp + tb + lane) : PK_NO);
        const unsigned long long b = __ballot(v != PK_NO);
        if (b) j = lane_get(v, __ffsll(b) - 1);
    }
    if (j == PK_NO) W.quiescent = true;              // a pass without a change
    else {
        if (j / TP == t) { W.my_kill = j - G.base; W.my_head = 1; W.my_hoff = n_out; }
        W.k = 1; W.has_anchor = 0;
        W.tt = (j + 1u) / TP; W.x = (j + 1u) % TP;
    }
}

// One hop of the walk from (W.tt < ntiles, W.x) that the fast paths did not take: a clean exit, an exit anchor
// without a partner inside the horizon, with a partner that left in the pass before (rescan), or without any
// until the end of the queue (it stays seated).  tmr: kp_rounds' timers of the slow kinds (PairChain.pslow).
template <uint32_t TP, class Ld>
static __device__ __forceinline__ void walk_general_hop(PairWalk& W, const PairParams& P, const PairTile<TP>& G, uint32_t t,
                                                        const uint32_t* rec, const uint16_t* exa, const uint32_t* bits_src,
                                                        uint32_t n_out, int lane, bool tmr, PairChain* pc)
{
    const uint32_t m = G.m, ntiles = G.ntiles, w = P.window;
    const uint32_t tlt = dev_min_u32(TP, m - W.tt * TP);
    if (W.x >= tlt) { ++W.tt; W.x = 0; W.have_r = false; return; }
    const uint32_t rr = W.have_r ? W.rpre : uni(Ld::ld(rec + (size_t)W.tt * TP + W.x));
    W.have_r = false;
    const uint32_t kind = rr >> 30, cnt = (rr >> 17) & 0x1FFFu, land = rr & 0x1FFFFu;
    const uint32_t t0 = W.tt, x0 = W.x;
    if (t0 == t) { W.my_entry = x0; W.my_off = n_out + W.k; }
    uint32_t d = DISP_NONE;
    W.k += cnt;
    if (kind == REC_CLEAN) { ++W.tt; W.x = 0; }
    else {
        uint32_t q = PK_NO, a = t0 * TP + land;              // exit anchor (FAR / NONE kinds)
        if (kind == REC_PARTNER) {
            q = t0 * TP + land - 1u;
            // partner still queued at the start of this pass?  (and, meanwhile, the next REC)
            const uint32_t t2 = (q + 1u) / TP, x2 = (q + 1u) % TP;
            const uint32_t bw = Ld::ld(bits_src + (q >> 5));
            const bool in2 = t2 < ntiles && x2 < dev_min_u32(TP, m - t2 * TP);
            if (in2) W.rpre = Ld::ld(rec + (size_t)t2 * TP + x2);
            if ((uni(bw) >> (q & 31u)) & 1u) { W.have_r = in2; W.rpre = uni(W.rpre); }
            else {
                const long long ts0 = tmr ? clock64() : 0;
                a = t0 * TP + Ld::ld16(exa + (size_t)t0 * TP + x0);
                q = uni(Ld::scan_fit(G.key, bits_src, G.key[a], q + 1u, m, w, lane));
                if (tmr) { atomicAdd(&pc->pslow[0], 1u); atomicAdd(&pc->pslow[1], (uint32_t)((clock64() - ts0) >> 4)); }
            }
        } else if (kind == REC_FAR) {
            const long long ts0 = tmr ? clock64() : 0;
            q = uni(Ld::scan_fit(G.key, bits_src, G.key[a], (t0 + 2u) * TP, m, w, lane));
            if (tmr) { atomicAdd(&pc->pslow[2], 1u); atomicAdd(&pc->pslow[3], (uint32_t)((clock64() - ts0) >> 4)); }
        }
        if (q != PK_NO) {
            d = q;
            W.k += 1u;
            if (q / TP == t) W.my_kill = q - G.base;
            W.tt = (q + 1u) / TP; W.x = (q + 1u) % TP;
        } else {
            // nobody fits until the end of the queue: the anchor stays in the lobby.  Its key is what every tile
            // needs before the pass ends (the next pass's head partner); slot, rating and role / region are fetched
            // off the critical path through a_oi (kp_round: tile 0 patches the record when the kernel ends;
            // kp_rounds: whoever emits the anchor, or the epilogue)
            d = DISP_SEATED;
            W.has_anchor = 1;
            tw_sload2_v(G.key + a, G.oidx + a, W.a_key, W.a_oi);
            W.a_team = 0;
            W.tt = ntiles;
        }
    }
    if (t0 == t) W.my_disp = d;
}

// The chain's state behind the pass the walk W has just finished from state S (one lane).  a_oi: what becomes of
// RoundState.a_oi when the pass changed the lobby.
static __device__ __forceinline__ RoundState walk_close(const RoundState& S, const PairWalk& W, uint32_t m, uint32_t a_oi)
{
    RoundState N = S;
    N.rounds = S.rounds + 1u;
    N.passes = S.passes + 1u;
    N.pos0 = 0; N.changed0 = 0; N.extra0 = 0;
    N.pairs = S.pairs + S.qlen + S.extra0; N.scanned = S.scanned + S.qlen + S.extra0;
    if (W.quiescent) {
        // nobody fits the carried anchor: a pass without a change ends the tick — unless the
        // change of this pass was its very first attempt (cancel tick, the head joined the
        // stale lobby): then the next pass is the one without a change
        if (!S.changed0) { N.done = 1; N.live = 0; }
    } else {
        const uint32_t seats = W.k - S.has_anchor + W.has_anchor;        // players that opened a lobby
        N.pairs -= seats;
        N.qlen = S.qlen - (W.k + seats);
        N.n_out = S.n_out + W.k;
        N.has_anchor = W.has_anchor; N.a_key = W.a_key; N.a_team = W.a_team; N.a_oi = a_oi;
        if ((W.k + seats == 0u && !S.changed0) || N.qlen == 0u) { N.done = 1; N.live = 0; }
        else if (N.qlen < PL_MAX || N.qlen * 4u < m * 3u) N.want_compact = 1;
    }
    return N;
}

// Section 2, the pass on the own tile (every thread; s_my[0..5] hold the walk's verdict on it): wave 0 collects
// the in-tile path, then everybody takes its players out of the bitmap and the keys and notes its lobby in E.
// S: the chain's state the pass started from; a_oi: S's anchor's q_* index where its slot has not been fetched
// (PK_NO: S.a_slot is valid).  The caller's barrier ends the section.
template <uint32_t TP>
static __device__ __forceinline__ void pass_apply(const PairParams& P, const PairTile<TP>& G, uint32_t g, PairChain* pc,
                                                  const RoundState& S, uint32_t a_oi, uint32_t* s_key, const uint16_t* s_nx,
                                                  const uint16_t* s_g, uint32_t* s_bits, uint16_t* s_path, uint32_t* s_my,
                                                  PassEmit& E, int tid, int lane, int wave)
{
    const uint32_t base = G.base, tl = G.tl;
    const uint32_t my_entry = s_my[0], my_off = s_my[1], d = s_my[2], my_kill = s_my[3];
    uint32_t* const os = P.out_slots + (size_t)g * P.out_slot_stride;
    E.pass = S.passes;
    if (wave == 0) {
        uint32_t n = 0;
        if (my_entry != PK_NO) {
            const uint32_t a = uni(l_succ(s_bits, my_entry, tl, lane));
            if (a != PK_NO) {
                uint32_t x = a;
                for (;;) {
#pragma unroll
                    for (uint32_t k = 0; k < 8u; ++k) {
                        s_path[n + k] = (uint16_t)x;
                        x = lds_ld16(s_g + x);
                    }
                    n += 8u;
                    if (uni(x) == TP) break;
                }
                const uint32_t pv = (uint32_t)lane < 8u ? (uint32_t)s_path[n - 8u + (uint32_t)lane] : TP;
                const unsigned long long parked = __ballot(pv == TP);
                n = n - 8u + (parked ? (uint32_t)__ffsll(parked) - 1u : 8u);
            }
        }
        if (lane == 0) s_my[6] = n;
    }
    __syncthreads();
    const uint32_t n = s_my[6];
    if (tid == 0 && my_kill != PK_NO) {                    // a partner that an earlier tile's anchor (or the
        const uint32_t kj = s_key[my_kill] & ~PK_DEAD;     // carried anchor) found in this tile
        atomicAnd(&s_bits[my_kill >> 5], ~(1u << (my_kill & 31u)));
        atomicOr(&s_key[my_kill], PK_DEAD);
        if (s_my[4]) {                                     // the head match is emitted here
            const uint32_t ra = pk_rating(S.a_key), rj = pk_rating(kj);
            E.hd_off = s_my[5];
            E.hd_iq = G.oidx[base + my_kill];
            E.hd_score = ra > rj ? ra - rj : rj - ra;
            E.hd_team = S.a_team;
            E.hd_sa = a_oi != PK_NO ? P.q_slot[G.qo + a_oi] : S.a_slot;
        }
    }
    for (uint32_t i = tid; i < n; i += PT_THREADS) {
        const uint32_t a = s_path[i];
        const uint32_t o = s_nx[a];
        const bool internal = o != NX_NONE && o != NX_FAR && a + o < tl;
        const uint32_t ka = s_key[a] & ~PK_DEAD;
        atomicAnd(&s_bits[a >> 5], ~(1u << (a & 31u)));
        atomicOr(&s_key[a], PK_DEAD);
        uint32_t qabs = PK_NO, kq = 0;
        if (internal) {
            const uint32_t j = a + o;
            kq = s_key[j] & ~PK_DEAD;
            atomicAnd(&s_bits[j >> 5], ~(1u << (j & 31u)));
            atomicOr(&s_key[j], PK_DEAD);
            qabs = base + j;
        } else {
            if (i + 1u != n || d == DISP_NONE) atomicOr(&pc->err, MM_ERRF_SEAT_INVARIANT);
            if (d != DISP_SEATED && d != DISP_NONE) { qabs = d; kq = G.key[qabs]; }
        }
        if (qabs != PK_NO) {
            const uint32_t ra = pk_rating(ka), rq = pk_rating(kq);
            const uint32_t sc = ra > rq ? ra - rq : rq - ra;
            if (i < PT_THREADS) {                          // the lobby of this step: the first loads now (PassEmit)
                E.em_off = my_off + i;
                E.em_ia = G.oidx[base + a];
                E.em_iq = G.oidx[qabs];
                E.em_score = sc;
            } else {                                       // more than 1024 lobbies in one tile and pass: right away
                os[2u * (my_off + i)] = P.q_slot[G.qo + G.oidx[base + a]];
                os[2u * (my_off + i) + 1u] = P.q_slot[G.qo + G.oidx[qabs]];
                P.out_score[(size_t)g * P.out_rec_stride + my_off + i] = (float)(int32_t)sc;
                P.out_pass[(size_t)g * P.out_rec_stride + my_off + i] = S.passes;
            }
        }
    }
    if (tid == 0) {
        if (n) {
            const uint32_t a = s_path[n - 1u], o = s_nx[a];
            const bool internal = o != NX_NONE && o != NX_FAR && a + o < tl;
            if (internal && d != DISP_NONE) atomicOr(&pc->err, MM_ERRF_SEAT_INVARIANT);
        } else if (d != DISP_NONE) atomicOr(&pc->err, MM_ERRF_SEAT_INVARIANT);
    }
}

// The carried anchor's first fit inside the tile (the next pass starts from the head): its minimum into *best_min,
// which holds PK_NO beforehand and is complete behind the workgroup's next barrier.
static __device__ __forceinline__ void head_first_fit(const uint32_t* s_key, uint32_t a_key, uint32_t w, uint32_t tl, int tid, int lane,
                                                      uint32_t* best_min)
{
    uint32_t klo, krng;
    pk_bounds(a_key, w, klo, krng);
    uint32_t best = PK_NO;
    for (uint32_t i = tid; i < tl; i += PT_THREADS)
        if (best == PK_NO && pk_in(s_key[i], klo, krng)) best = i;
    const unsigned long long b = __ballot(best != PK_NO);
    if (b) {
        // lanes hold increasing i within a stride, the first lane with a hit holds the wave's minimum
        // only within its own stride: take the true minimum
        uint32_t v = best;
        for (int dd = 1; dd < 64; dd <<= 1) { const uint32_t o2 = (uint32_t)__shfl((int)v, lane ^ dd); v = o2 < v ? o2 : v; }
        if (lane == 0) atomicMin(best_min, v);
    }
}

// ------------------------------------------------------------------------------------
// kp_round: the three launches of a round fused into ONE.  Every tile's workgroup
//   1. walks the route of pass p itself (wave 0; the same deterministic walk in every
//      workgroup, so nobody waits for anybody),
//   2. applies pass p to its own tile (in-tile chain, bitmap, emission),
//   3. prepares its tile for pass p+1.
// Everything a workgroup reads from another one (REC, exit anchors, the bitmap at the start
// of the pass, head partners, the chain's round state) was written by the PREVIOUS launch
// into the buffers of the other parity, so there is no intra-launch communication at all.
// The price: a tile sees its lookahead tile as it was one pass ago.  That only ever shows
// too many queued players (a superset), so an exit anchor may point at a partner that has
// just left the queue; the walk checks the partner against the pass-start bitmap and rescans
// if so (rare: the partner must have been matched in exactly the previous pass).
// `first`: the launch that opens a batch only prepares (there is no route yet).
// ------------------------------------------------------------------------------------
template <uint32_t TP>
__global__ __launch_bounds__(PT_THREADS) void kp_round(PairParams P, uint32_t r, uint32_t first)
{
    constexpr uint32_t PK_T = TP;                 // the tile length of this instantiation
    (void)PK_T;
    __shared__ __attribute__((aligned(16))) uint32_t s_key[2 * PK_T + 64];
    __shared__ __attribute__((aligned(16))) uint16_t s_nx[PK_T];
    __shared__ __attribute__((aligned(16))) uint16_t s_g[PK_T + 8];
    __shared__ uint32_t s_pc[PK_T + 64];
    __shared__ __attribute__((aligned(16))) uint32_t s_bits[2 * PK_T / 32 + 4];
    __shared__ uint32_t s_cnt[16];
    __shared__ uint16_t s_nw[PK_T / 32 + 2];
    __shared__ uint16_t s_path[PK_T / 2 + 72];
    __shared__ RoundState s_N;
    __shared__ uint32_t s_my[8];                 // entry, offset, disposition, incoming kill, head flag, head offset, n, -

    uint32_t g, t, xj, xn;                       // xj of xn: my place among the chain's workgroups of this XCD
    if (!pair_wg_map(P, g, t, xj, xn)) return;
    PairChain* const pc = P.pchains + g;
    const uint32_t bm = P.bm[g];                 // from the kernel arguments: no load in front of the tile's loads
    if (bm == 0u || t >= (bm + PK_T - 1u) / PK_T) return;
    const PairTile<TP> G(P, g, t, bm, P.bbuf[g]);
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const uint32_t cpar = r & 1u, npar = cpar ^ 1u;
    const uint32_t w = P.window;
    const uint32_t* const bits_src = (first ? P.bits[G.buf] : P.bitsp[cpar]) + (size_t)g * P.bits_stride;
    uint32_t* const bits_dst = P.bitsp[npar] + (size_t)g * P.bits_stride;

    const RoundState S = first ? round_state_open(pc) : pc->rs[cpar];
    // The tile's own state is asked for before anything of the round state is looked at (the two come from
    // HBM side by side instead of one after the other).
    long long tq = clock64();
    // the walk's first load (where the carried anchor finds its partner, one word per tile) is in flight while the
    // tile's own state comes in
    uint32_t hp0 = PK_NO;
    if (!first && wave == 0 && (uint32_t)lane < G.ntiles) hp0 = P.headp[cpar][(size_t)g * P.max_tiles + (uint32_t)lane];
    for (uint32_t i = tid; i < 2u * PK_T / 32u + 4u; i += PT_THREADS) s_bits[i] = i < G.hwords ? bits_src[(G.base >> 5) + i] : 0u;
    copy_words_x4((uint32_t*)s_nx, (const uint32_t*)G.gnx, (G.tl + 1u) >> 1, tid, PT_THREADS);
    if (!first) copy_words_x4((uint32_t*)s_g, (const uint32_t*)(P.g16 + G.po + G.base), (G.tl + 1u) >> 1, tid, PT_THREADS);
    if (tid == 0) { s_cnt[1] = 0; s_cnt[2] = 0; s_cnt[3] = 0; s_cnt[4] = 0; }   // long list, list, cursor; staging waves done
    if ((uint32_t)tid < RP_MAXLONG) s_pc[RP_MAXLONG + tid] = PK_NO;      // repair_long's result slots
    __syncthreads();
    if (!S.live) {                               // ended earlier in this batch: keep both parities equal
        for (uint32_t i = tid; i < G.own_words; i += PT_THREADS) bits_dst[(G.base >> 5) + i] = s_bits[i];
        if (t == 0 && tid == 0) pc->rs[npar] = S;
        return;
    }
    // diagnostics (MM_PAIR_DEBUG): cycles per phase of tile 1; MM_PAIR_TUNE bit 15: only rounds from the 200th on
    const bool tmr = t == 1u && tid == 0 && !first && (!(P.tune & 0x8000u) || S.rounds >= 200u);
#define TMARK(K) do { if (tmr) { const long long now = clock64(); pc->tm[K] += (uint32_t)(now - tq); tq = now; } } while (0)
    if (tmr) pc->tm[5] += 1u;
    if ((P.tune & 0x2000u) && tid == 0) tc_row(P, TC_DISP, g)[t] = mm_xcc_id() | (S.rounds << 8);   // diagnostics: placement
    if (tid < 8) s_g[PK_T + tid] = (uint16_t)PK_T;
    if (tid == 0) s_N = S;
    TMARK(0);

    PassEmit E;                                  // this thread's lobby of section 2
    uint32_t tst = 0;                            // diagnostics: candidates this wave tested (MM_PAIR_TUNE bit 13)
    uint32_t seat_oi = PK_NO, seat_slot = 0, seat_cons = 0;   // the anchor this pass leaves seated: its q_* index and values
    int32_t seat_rating = 0;
    if (!first) {
        // ================= 1. the route of pass p (MATCH_CHECK.md §4), wave 0 =================
        // meanwhile the other fifteen waves stage the keys (dead flags as of the start of the pass;
        // step 2 adds the flags of the players this pass removes from the own tile)
        // The walk is a chain of dependent loads of REC / bitmap words that OTHER workgroups wrote in the previous
        // launch — on other XCDs as a rule, so every hop would miss this XCD's L2 and go out to the fabric (~1200
        // cycles a hop measured, against ~250 for an L2 hit).  The workgroups of a chain that share an XCD
        // (dispatch is round robin over the XCDs: linear id % 8; a guess that only costs misses when wrong) pull the
        // chain's tables through their L2 together, each a share of the tiles, before anything else; the walk
        // then mostly hits (issued behind the first barrier: in front of it they only delay the tile's own loads).  The first PF_ENT entries of a tile only when the tile is longer (a cursor enters a
        // tile a short way in, behind the partner of the previous tile's exit anchor).
        uint4 pf[PF_N];
#pragma unroll
        for (uint32_t u = 0; u < PF_N; ++u) pf[u] = uint4{0u, 0u, 0u, 0u};
        if (wave != 0 && !(P.tune & 0x1000u)) {
            // (the whole tile instead of its first 2816 entries when the chain's workgroups share one XCD: measured, no gain —
            // profiles/r03_ab_pair_xcd.txt)
            constexpr uint32_t PF_ENT = PK_T < 2816u ? PK_T : 2816u;                 // REC entries per tile
            constexpr uint32_t PF_Q = PF_ENT / 4u + PK_T / 128u;                     // 16-byte pieces per tile: REC + bitmap words
            // this workgroup's share: one of the chain's workgroups on this XCD
            const uint32_t R = xn ? xn : (G.ntiles >> 3 ? G.ntiles >> 3 : 1u), myr = xn ? xj : (t >> 3) % R;
            const uint4* const rec4 = (const uint4*)(P.rec2[cpar] + G.po);
            const uint4* const bit4 = (const uint4*)bits_src;
#pragma unroll
            for (uint32_t u = 0; u < PF_N; ++u) {
                const uint32_t wk = (uint32_t)tid - 64u + u * (PT_THREADS - 64u);
                const uint32_t tj = myr + (wk / PF_Q) * R, c = wk % PF_Q;
                // (no more than this workgroup's fair share of the chain's tiles: with the chain on one XCD that is two or
                // three tiles, not the seven the loads could cover — what another workgroup of the XCD pulls is in the L2 too)
                if (tj < G.ntiles && wk / PF_Q < (G.ntiles + R - 1u) / R) {
                    if (c < PF_ENT / 4u) {
                        if (tj * PK_T + c * 4u < G.m) pf[u] = rec4[(tj * PK_T) / 4u + c];
                    } else if ((tj * PK_T) / 32u + (c - PF_ENT / 4u) * 4u < (G.m + 31u) / 32u) pf[u] = bit4[(tj * PK_T) / 128u + (c - PF_ENT / 4u)];
                }
            }
        }
        if (wave != 0) {
            prep_stage_keys<PK_T>(s_key, s_bits, G.key + G.base, G.hl, tid - 64, PT_THREADS - 64);
#pragma unroll
            for (uint32_t u = 0; u < PF_N; ++u) TW_SINK(pf[u].x);                    // the loads above are wanted in the cache only
            __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");        // this wave's keys are in LDS ...
            wave_lockstep();
            if (lane == 0) atomicAdd(&s_cnt[4], 1u);                      // ... before it says so
        }
        if (wave != 0 && !(P.tune & 0x4000u)) {
            // While wave 0 walks: the first repair sweep.  The keys are staged by waves 1 .. 15;
            // everybody here waits for them (wave 0 cannot join a barrier now), then repairs the players whose
            // partner had left the queue when this pass began.  What the sweep writes stays valid through the
            // pass: it only replaces a departed partner by the next fit that is still queued NOW — if the pass
            // takes that one too, the second sweep sees it.  Anchors on this pass's path keep their next[]: an
            // in-tile partner is queued by construction, an exit anchor's is looked up by the walk itself.
            while (lds_ld(&s_cnt[4]) < (uint32_t)(PT_THREADS / 64 - 1)) __builtin_amdgcn_s_sleep(1);
            __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
            repair_sweep<PK_T>(s_key, s_nx, s_pc, &s_cnt[1], s_pc + 2u * RP_MAXLONG + (uint32_t)wave * RP_TODO, bits_src + (G.base >> 5),
                         G.tl, G.hl, G.base + G.hl == G.m, w, lane, (uint32_t)wave - 1u, PT_THREADS / 64u - 1u, tst);
        }
        if (wave == 0) {
            // the walk is the one serial piece of the round: it must not queue for issue slots behind the three
            // waves that share its SIMD and are staging / sweeping meanwhile
            __builtin_amdgcn_s_setprio(3);
            const uint32_t* const rec = P.rec2[cpar] + G.po;
            const uint16_t* const exa = P.exa[cpar] + G.po;
            const uint32_t m = G.m, base = G.base, n_out = S.n_out;
            PairWalk W(S, PK_NO);
            walk_head<TP, LdLaunch>(W, G, t, P.headp[cpar] + (size_t)g * P.max_tiles, n_out, lane, true, hp0);
            const long long tw0 = (P.tune & 0x2000u) ? clock64() : 0;
            uint32_t dbg_hops = 0, dbg_ghops = 0, dbg_gtry = 0, dbg_gstale = 0, gskip = PK_NO;
            bool to_group = false;
            // (the second route level only exists at the longest tile length: a chain of PK_GROUP_MIN tiles is never walked
            // with a shorter one — the other instantiations carry none of it in their hop loop)
            const bool grp_on = TP == PK_TMAX && P.grp != 0u;
            long long th0 = tw0;
            uint32_t dbg_early = 0, dbg_late = 0;
            while (!W.quiescent && W.tt < G.ntiles) {
                if (P.tune & 0x2000u) {
                    const long long now = clock64();
                    if (dbg_hops) { if (dbg_hops <= 4u) dbg_early += (uint32_t)(now - th0); else dbg_late += (uint32_t)(now - th0); }
                    th0 = now;
                }
                ++dbg_hops;
                // Second level (long chains, kp_group): the cursor stands in the first tile of a group this tile
                // does not belong to — one hop to where the walk goes on behind the group (or where, inside it, the
                // general code has to look: then the entry says "here", and the hop below is the ordinary one).
                if (grp_on && W.tt * PK_T + W.x != gskip) {
                    const uint32_t gr = W.tt / PK_GS;
                    if (gr != t / PK_GS && W.tt == gr * PK_GS) {
                        const uint4* const ge = P.grec + (size_t)g * P.gstride + (size_t)gr * PK_T + W.x;
                        uint32_t gp, gc, gq, gs;
                        tw_sload4_v((const uint32_t*)ge, gp, gc, gq, gs);
                        ++dbg_gtry;
                        if (gs != r) ++dbg_gstale;
                        if (gs == r && gp != W.tt * PK_T + W.x) {
                            ++dbg_ghops;
                            W.k += gc;
                            if (gq != PK_NO && gq / PK_T == t) W.my_kill = gq - base;
                            W.tt = gp / PK_T;
                            W.x = gp % PK_T;
                            W.have_r = false;
                            continue;
                        }
                        gskip = W.tt * PK_T + W.x;   // not an entry of this round (or it says "here"): tile by tile from here
                    }
                }
                // Fast path — almost every hop: the tile's REC says "exit anchor with a partner" and the partner
                // is still queued.  Everything is wave uniform and kept scalar; one round trip to memory per
                // hop (the partner's bitmap word and the next REC together).  Anything else (a clean exit, no
                // partner inside the horizon, a partner that left in the pass before) falls through to the
                // general hop below, which redoes the hop from the same state.
                if (W.have_r) {
                    // the loop carries the cursor's absolute position and the REC there in scalar registers, nothing else
                    uint32_t p = W.tt * PK_T + W.x, rr = W.rpre;
                    while ((rr >> 30) == REC_PARTNER) {
                        const uint32_t tb = p & ~(PK_T - 1u);
                        // (the first tile of somebody else's group: back to the top, there is a hop over the whole group)
                        if (grp_on && (tb / PK_T) % PK_GS == 0u && tb / (PK_T * PK_GS) != t / PK_GS && p != gskip) { to_group = true; break; }
                        const uint32_t q = tb + (rr & 0x1FFFFu) - 1u, nxt = q + 1u;
                        if (nxt >= m) break;                                          // the end of the queue: the general hop
                        uint32_t bw, r2;
                        tw_sload2(bits_src + (q >> 5), rec + nxt, bw, r2);             // through the scalar cache: the shorter path
                        if (!((bw >> (q & 31u)) & 1u)) break;
                        if (tb == base) { W.my_entry = p - base; W.my_off = n_out + W.k; W.my_disp = q; }
                        W.k += ((rr >> 17) & 0x1FFFu) + 1u;
                        if ((q & ~(PK_T - 1u)) == base) W.my_kill = q - base;
                        p = nxt;
                        rr = r2;
                    }
                    W.tt = p / PK_T;
                    W.x = p % PK_T;
                    W.rpre = rr;
                }
                if (W.tt >= G.ntiles) break;
                if (to_group) { to_group = false; continue; }
                walk_general_hop<TP, LdLaunch>(W, P, G, t, rec, exa, bits_src, n_out, lane, false, pc);
            }
            __builtin_amdgcn_s_setprio(0);
            if ((P.tune & 0x2000u) && tmr) {
                atomicAdd(&pc->tm[13], (uint32_t)((clock64() - tw0) >> 4));          // the walk loop alone: cycles / 16 ...
                atomicAdd(&pc->tm[15], dbg_hops);                                    // ... and its iterations
                atomicAdd(&pc->tm[12], dbg_early >> 4);                              // iterations 1-4 / the later ones, cycles / 16
                atomicAdd(&pc->tm[14], dbg_late >> 4);
            }
            if (lane == 0 && t == 0u && dbg_gtry) { atomicAdd(&pc->ghops, dbg_ghops); atomicAdd(&pc->gtry, dbg_gtry); atomicAdd(&pc->gstale, dbg_gstale); }
            seat_oi = W.a_oi;
            if (lane == 0) {
                s_N = walk_close(S, W, m, S.a_oi);
                W.publish(s_my);
            }
        }
        __syncthreads();
        TMARK(6);
        // ================= 2. pass p on the own tile =================
        pass_apply<TP>(P, G, g, pc, S, PK_NO, s_key, s_nx, s_g, s_bits, s_path, s_my, E, tid, lane, wave);
        __syncthreads();
        TMARK(9);
    } else __syncthreads();

    // what everybody needs of the next round's state (the whole record goes to HBM from one thread)
    struct { uint32_t live, has_anchor, a_key; } N;
    N.live = s_N.live; N.has_anchor = s_N.has_anchor; N.a_key = s_N.a_key;
    if (t == 0 && tid == 0) {
        pc->rs[npar] = s_N;
        if (seat_oi != PK_NO) {                  // loads now, the three stores at the end (SEAT_PATCH)
            seat_slot = P.q_slot[G.qo + seat_oi];
            seat_rating = P.q_rating[G.qo + seat_oi];
            seat_cons = P.q_cons[G.qo + seat_oi];
        }
    }
#define SEAT_PATCH() do { if (t == 0 && tid == 0 && seat_oi != PK_NO) {                                          \
        pc->rs[npar].a_slot = seat_slot; pc->rs[npar].a_rating = seat_rating; pc->rs[npar].a_cons = seat_cons; } } while (0)
    for (uint32_t i = tid; i < G.own_words; i += PT_THREADS) bits_dst[(G.base >> 5) + i] = s_bits[i];
    if (!N.live) { E.store(P, g, G.qo); SEAT_PATCH(); return; }

    // ================= 3. the own tile for pass p + 1 =================
    if (first) {
        prep_stage_keys<PK_T>(s_key, s_bits, G.key + G.base, G.hl, tid);
        __syncthreads();
    }
    prep_repair<PK_T>(s_key, s_nx, s_pc, &s_cnt[1], bits_src + (G.base >> 5), G.tl, G.hl, G.base + G.hl == G.m, w, tid, tst,
                      tmr && !(P.tune & 0x2000u) ? pc->tm : nullptr);
    E.load(P, G.qo);                             // the oidx loads of section 2 have long arrived
    prep_tables<PK_T>(s_key, s_nx, s_bits, s_nw, s_pc, P.g16 + G.po + G.base, P.rec2[npar] + G.po + G.base, P.exa[npar] + G.po + G.base,
                G.gnx, G.tl, tid, tmr ? pc->tm : nullptr);
    TMARK(3);
    __syncthreads();                             // every node of s_pc is final: the samples below read other threads' nodes
    if (tid == 0) s_cnt[0] = PK_NO;
    __syncthreads();
    if (N.has_anchor) head_first_fit(s_key, N.a_key, w, G.tl, tid, lane, &s_cnt[0]);
    __syncthreads();
    if (tid == 0) P.headp[npar][(size_t)g * P.max_tiles + t] = s_cnt[0] == PK_NO ? PK_NO : G.base + s_cnt[0];
    E.store(P, g, G.qo);
    SEAT_PATCH();
    if ((P.tune & 0x2000u) && lane == 0) {          // + the carried anchor's scan of the tile (one test per position)
        const unsigned long long all = (unsigned long long)tst + (wave == 0 && N.has_anchor ? G.tl : 0u);
        if (all) atomicAdd(&pc->tested, all);
    }
    TMARK(4);
#undef TMARK
#undef SEAT_PATCH
}

// ------------------------------------------------------------------------------------
// kp_rounds: SEVERAL passes per launch, the tiles resident.  The same round as kp_round — walk, apply, prepare —
// but a workgroup keeps its tile (keys of the own and the lookahead tile, next[], the in-tile chain, the bitmap) in
// LDS from pass to pass and the chain's round state in registers / LDS (every workgroup's walk computes the same
// one), so that a pass starts without the two rounds of loads that open a kp_round launch, without staging 2 x PK_T
// keys, and reads the tables the other tiles published through an L2 that still holds them.  What a pass hands to
// the next one across workgroups — REC, exit anchors, the bitmap at the start of the pass, the carried anchor's first
// fit per tile — goes through the same double-buffered arrays as in kp_round, and the launch boundary that ordered
// them there is a flag barrier among the chain's workgroups here:
//
//   publish (plain stores) -> every wave waits for its stores' acknowledgements -> __syncthreads -> ONE arrival
//   (64-bit atomic add on the chain's word) ... poll that word -> __syncthreads -> scalar cache invalidated ->
//   loads that go past the vector L1 (xld) or through the scalar cache.
//
// That is an exchange through ONE XCD's L2 (the L2s of different XCDs are not coherent with each other): the host
// maps every chain's workgroups onto one XCD (PairParams.xseg; dispatch is round robin over the XCDs — observed, not
// promised), every workgroup says at the first barrier where it runs (HW_REG_XCC_ID), and a chain that finds itself
// on two XCDs stops there (PF_XCD): nothing has been walked yet, the host goes on with kp_round.
// Waiting is bounded: whoever has waited for PairParams.ptimeout0 / 1 ticks declares "nobody starts iteration i"
// with a compare-and-swap on the arrival word that only succeeds while the arrivals are still incomplete — so either
// every workgroup of the chain runs iteration i or none does, whatever the timing — and everybody leaves through the
// epilogue, which commits the chain exactly like kp_round_commit: a stop costs the passes that were not walked,
// never the tick (the host continues with one launch per pass).  Workgroups that have not been dispatched when that
// happens (another engine's launch holds the CUs) find the word and leave at once.
// Iteration 0 only prepares (kp_round's `first`), iterations 1 .. K walk pass after pass, the last one does not
// prepare again.  [it_begin, it_end): the GPU runs all of it in one launch; the CPU shim of the tests, which runs
// workgroups one after another, one iteration per launch with the resident state kept per workgroup (MM_RESIDENT).
// ------------------------------------------------------------------------------------
#define PF_TIMEOUT 1u                // somebody waited too long at a barrier
#define PF_XCD 2u                    // the chain's workgroups are not on one XCD
#define PF_INJECT 3u                 // PairParams.pinject (tests)
#define PF_YIELD 4u                  // no failure: another chain has asked for the batch to end (PairParams.pyield)

template <uint32_t TP>
struct RoundsRes {
    alignas(16) uint32_t key[2 * TP + 64];
    alignas(16) uint16_t nx[TP];
    alignas(16) uint16_t g[TP + 8];
    alignas(16) uint32_t pc[TP + 64];
    alignas(16) uint32_t bits[2 * TP / 32 + 4];
    uint32_t cnt[16];
    uint16_t nw[TP / 32 + 2];
    uint16_t path[TP / 2 + 72];
    RoundState S, N;                 // the chain's state before / after the pass being walked
    uint32_t my[8];
    uint32_t ctl[4];                 // [0] this workgroup has left (shim launches), [1] barrier verdict, [2] passes walked
    uint32_t tm[16];                 // diagnostics (tile 1)
};

template <uint32_t TP>
__global__ __launch_bounds__(PT_THREADS) void kp_rounds(PairParams P, uint32_t it_begin, uint32_t it_end, uint32_t K)
{
    constexpr uint32_t PK_T = TP;                 // the tile length of this instantiation
    (void)PK_T;
    MM_RESIDENT(RoundsRes<TP>, L);
    uint32_t* const s_key = L.key;
    uint16_t* const s_nx = L.nx;
    uint16_t* const s_g = L.g;
    uint32_t* const s_pc = L.pc;
    uint32_t* const s_bits = L.bits;
    uint32_t* const s_cnt = L.cnt;
    uint16_t* const s_nw = L.nw;
    uint16_t* const s_path = L.path;
    uint32_t* const s_my = L.my;

    uint32_t g, t, xj, xn;
    if (!pair_wg_map(P, g, t, xj, xn)) return;
    PairChain* const pc = P.pchains + g;
    const uint32_t bm = P.bm[g];
    if (bm == 0u || t >= (bm + PK_T - 1u) / PK_T) return;
    const PairTile<TP> G(P, g, t, bm, P.bbuf[g]);
    const int tid_o = threadIdx.x;
    const uint32_t w = P.window;
    uint32_t* const bits_com = P.bits[G.buf] + (size_t)g * P.bits_stride;      // the committed bitmap
    unsigned long long* const bar = P.pbar + g;
    long long tq = clock64();
#define TMARK(K_) do { if (tmr) { const long long now = clock64(); L.tm[K_] += (uint32_t)(now - tq); tq = now; } } while (0)

    if (it_begin == 0u) {
        // ---- prologue: the committed state of the chain and of the own tile ----
        const int tid = tid_o;
        MM_RESIDENT_FRESH(L);
        if (tid == 0) {
            const RoundState S = round_state_open(pc);
            L.S = S;
            L.N = S;
            L.ctl[0] = 0; L.ctl[1] = 0; L.ctl[2] = 0;
            for (int k = 0; k < 16; ++k) L.tm[k] = 0;
        }
        for (uint32_t i = tid; i < 2u * PK_T / 32u + 4u; i += PT_THREADS) s_bits[i] = i < G.hwords ? bits_com[(G.base >> 5) + i] : 0u;
        copy_words_x4((uint32_t*)s_nx, (const uint32_t*)G.gnx, (G.tl + 1u) >> 1, tid, PT_THREADS);
        if (tid < 8) s_g[PK_T + tid] = (uint16_t)PK_T;
        if (tid == 0) { s_cnt[1] = 0; s_cnt[2] = 0; s_cnt[3] = 0; s_cnt[4] = 0; }   // long list, list, cursor (prep_repair)
        if ((uint32_t)tid < RP_MAXLONG) s_pc[RP_MAXLONG + tid] = PK_NO;              // repair_long's result slots
        __syncthreads();
        prep_stage_keys<PK_T>(s_key, s_bits, G.key + G.base, G.hl, tid);
        __syncthreads();
    } else if (L.ctl[0]) return;                 // (shim launches: this chain has been committed already)

    uint32_t stop = 0;                           // PF_* | iteration << 8 when the launch gives up
    bool ended = false;
    uint32_t tst = 0;
    long long dw0 = 0;                           // MM_PAIR_TUNE bit 16: every tile's cycles from barrier to arrival (thread 0), into grec
    uint32_t dwork = 0, dn = 0;
    for (uint32_t it = it_begin; it < it_end; ++it) {
        // (the thread's index as the compiler cannot see through, once per iteration: what is derived from it — the LDS
        // addresses of a thread's eight nodes, its chunks, its words — is computed where it is used, not kept across the loop)
        int tid_l = tid_o;
        TW_LAUNDER(tid_l);
        const int tid = tid_l, lane = tid & 63, wave = tid >> 6;
        const bool tmr = t == 1u && tid == 0;
        const uint32_t cpar = it & 1u, npar = cpar ^ 1u;
        const uint32_t* const bits_src = P.bitsp[cpar] + (size_t)g * P.bits_stride;
        uint32_t* const bits_dst = P.bitsp[npar] + (size_t)g * P.bits_stride;
        PassEmit E;                              // this thread's lobby of section 2

        if (it > 0u) {
            // ================= 0. everybody's tables of iteration it - 1 are out =================
            if (tid == 0) {
                uint32_t verdict = 0;
                const unsigned long long need = (unsigned long long)G.ntiles * it;
                const long long t0 = wall_clock64();
                const long long limit = it == 1u ? (long long)P.ptimeout0 : (long long)P.ptimeout1;
                for (;;) {
                    const unsigned long long wv = xld64(bar);
                    const uint32_t f = (uint32_t)(wv >> 32);
                    if (f != 0u && (f >> 8) <= it) { verdict = f; break; }          // nobody starts this iteration
                    if ((wv & 0xFFFFFFFFull) >= need) break;
                    if (f == 0u && xld(P.pyield) != 0u) {
                        // the batch is to end (the longest chain wants its compaction): the same declaration as a time-out's,
                        // and like it only while nobody can have gone past this barrier
                        const unsigned long long nv = wv | ((unsigned long long)(PF_YIELD | (it << 8)) << 32);
                        if (atomicCAS(bar, wv, nv) == wv) { verdict = PF_YIELD | (it << 8); break; }
                        continue;
                    }
                    if (f == 0u && wall_clock64() - t0 > limit) {
                        // only while the arrivals are still incomplete: then nobody has gone past this barrier
                        const unsigned long long nv = wv | ((unsigned long long)(PF_TIMEOUT | (it << 8)) << 32);
                        if (atomicCAS(bar, wv, nv) == wv) { verdict = PF_TIMEOUT | (it << 8); break; }
                        continue;
                    }
                    __builtin_amdgcn_s_sleep(1);
                }
                if (!verdict && it == 1u) {
                    const uint32_t xm = xld(P.pxmask + g);
                    if (xm & (xm - 1u)) verdict = PF_XCD | (1u << 8);               // the same for every workgroup of the chain
                }
                L.ctl[1] = verdict;
            }
            __syncthreads();
            tw_sinv();
            if (L.ctl[1]) { stop = L.ctl[1]; break; }
            TMARK(0);
            if (tid == 0 && (P.tune & 0x10000u)) dw0 = clock64();             // (diagnostics: this tile's pass begins)
            const RoundState S = L.S;
            // ================= 1. the route of the pass (wave 0) beside the first repair sweep =================
            if (wave != 0) {
                // The lookahead tile as its workgroup left it: who is gone there since the last look gets the dead flag.  Only
                // the sweep needs that, not the walk: the fifteen waves do it among themselves (a counter in LDS is their
                // rendezvous; wave 0 is on its way already).
                for (uint32_t i = PK_T / 32u + (uint32_t)tid - 64u; i < G.hwords; i += PT_THREADS - 64u) {
                    const uint32_t nw_ = xld(bits_src + (G.base >> 5) + i);
                    uint32_t gone = s_bits[i] & ~nw_;
                    s_bits[i] = nw_;
                    while (gone) {
                        const uint32_t b = (uint32_t)__ffs((int)gone) - 1u;
                        gone &= gone - 1u;
                        s_key[(i << 5) + b] |= PK_DEAD;
                    }
                }
                if ((uint32_t)tid - 64u < RP_MAXLONG) s_pc[RP_MAXLONG + tid - 64] = PK_NO;      // repair_long's result slots
                __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
                wave_lockstep();
                if (lane == 0) atomicAdd(&s_cnt[4], 1u);
                while (lds_ld(&s_cnt[4]) < (uint32_t)(PT_THREADS / 64 - 1)) __builtin_amdgcn_s_sleep(1);
                __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
                // (no sweep in the batch's last iteration: what it puts on the long list is only finished by the prepare step,
                // and there is none behind the last pass — the next batch's first prepare finds the same departures)
                if (it != K && !(P.tune & 0x4000u))
                    repair_sweep<PK_T>(s_key, s_nx, s_pc, &s_cnt[1], s_pc + 2u * RP_MAXLONG + (uint32_t)wave * RP_TODO, bits_src + (G.base >> 5),
                                       G.tl, G.hl, G.base + G.hl == G.m, w, lane, (uint32_t)wave - 1u, PT_THREADS / 64u - 1u, tst);
            }
            if (wave == 0) {
                __builtin_amdgcn_s_setprio(3);
                const uint32_t* const rec = P.rec2[cpar] + G.po;
                const uint16_t* const exa = P.exa[cpar] + G.po;
                const uint32_t m = G.m, base = G.base, n_out = S.n_out;
                PairWalk W(S, S.a_oi);
                walk_head<TP, LdPeer>(W, G, t, P.headp[cpar] + (size_t)g * P.max_tiles, n_out, lane);
                uint32_t dbg_hops = 0;
                const long long tw0 = tmr ? clock64() : 0;
                while (!W.quiescent && W.tt < G.ntiles) {
                    ++dbg_hops;
                    // Fast path (kp_round's, minus the second route level): exit anchor with a partner that is still
                    // queued — one round trip through the scalar cache per hop
                    if (W.have_r) {
                        uint32_t p = W.tt * PK_T + W.x, rr = W.rpre;
                        // a hop whose partner lies in front of the own tile, or whose anchor lies behind it, concerns nobody here:
                        // the tight loop (mm_gfx950.h); the hops in between keep the own tile's books
                        const uint32_t p_in = p;
                        const long long th0 = tmr ? clock64() : 0;
                        tw_hops(tw_sptr(bits_src), tw_sptr(rec), m, ~(PK_T - 1u), base, p, rr, W.k);
                        while ((rr >> 30) == REC_PARTNER) {
                            const uint32_t tb = p & ~(PK_T - 1u);
                            if (tb > base) break;
                            const uint32_t q = tb + (rr & 0x1FFFFu) - 1u, nxt = q + 1u;
                            if (nxt >= m) break;                                          // the end of the queue: the general hop
                            uint32_t bw, r2;
                            tw_sload2(bits_src + (q >> 5), rec + nxt, bw, r2);
                            if (!((bw >> (q & 31u)) & 1u)) break;
                            if (tb == base) { W.my_entry = p - base; W.my_off = n_out + W.k; W.my_disp = q; }
                            W.k += ((rr >> 17) & 0x1FFFu) + 1u;
                            if ((q & ~(PK_T - 1u)) == base) W.my_kill = q - base;
                            p = nxt;
                            rr = r2;
                        }
                        tw_hops(tw_sptr(bits_src), tw_sptr(rec), m, ~(PK_T - 1u), 0xFFFFFFFFu, p, rr, W.k);
                        dbg_hops += p / PK_T - p_in / PK_T;                            // (diagnostics: a fast hop advances a tile)
                        if (tmr) L.tm[3] += (uint32_t)(clock64() - th0);               // ... and the fast hops' cycles
                        W.tt = p / PK_T;
                        W.x = p % PK_T;
                        W.rpre = rr;
                    }
                    if (W.tt >= G.ntiles) break;
                    walk_general_hop<TP, LdPeer>(W, P, G, t, rec, exa, bits_src, n_out, lane, tmr, pc);
                }
                __builtin_amdgcn_s_setprio(0);
                if (tmr) { L.tm[13] += (uint32_t)((clock64() - tw0) >> 4); L.tm[15] += dbg_hops; }
                if (lane == 0) {
                    L.N = walk_close(S, W, m, W.has_anchor ? W.a_oi : PK_NO);
                    W.publish(s_my);
                }
            }
            __syncthreads();
            TMARK(6);
            // ================= 2. the pass on the own tile =================
            pass_apply<TP>(P, G, g, pc, S, S.a_oi, s_key, s_nx, s_g, s_bits, s_path, s_my, E, tid, lane, wave);
            if (tid == 0) {
                L.S = L.N;                       // the pass is in the tile: from here on the chain's state is the new one
                L.ctl[2] += 1u;
            }
            __syncthreads();
            TMARK(9);
        }
        // what everybody needs of the state behind the pass
        struct { uint32_t live, has_anchor, a_key; } N;
        N.live = L.S.live; N.has_anchor = L.S.has_anchor; N.a_key = L.S.a_key;
        if (!N.live || it == K) { E.store(P, g, G.qo); ended = true; break; }       // the chain's tick is over / the batch is: no tables for nobody
        if (it > 0u && L.S.qlen <= P.pyq[g]) {
            // every workgroup of the chain sees the same queue length behind the same pass: they all leave here, and the
            // other chains are asked to (they find the word at their next barrier)
            if (t == 0u && tid == 0) __hip_atomic_store(P.pyield, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            E.store(P, g, G.qo); ended = true; break;
        }

        // ================= 3. the own tile for the next pass =================
        for (uint32_t i = tid; i < G.own_words; i += PT_THREADS) bits_dst[(G.base >> 5) + i] = s_bits[i];
        if (tid == 0) { s_cnt[0] = PK_NO; s_cnt[4] = 0; }                    // (the head scan's minimum; the next pass's rendezvous)
        prep_repair<PK_T>(s_key, s_nx, s_pc, &s_cnt[1], bits_src + (G.base >> 5), G.tl, G.hl, G.base + G.hl == G.m, w, tid, tst,
                          tmr ? L.tm : nullptr);
        E.load(P, G.qo);
        // (the head scan's minimum is complete behind the barriers inside prep_tables)
        if (N.has_anchor) head_first_fit(s_key, N.a_key, w, G.tl, tid, lane, &s_cnt[0]);
        prep_tables<PK_T>(s_key, s_nx, s_bits, s_nw, s_pc, s_g, P.rec2[npar] + G.po + G.base, P.exa[npar] + G.po + G.base,
                          nullptr, G.tl, tid, tmr ? L.tm : nullptr);
        if (tmr) tq = clock64();
        if (tid == 0) P.headp[npar][(size_t)g * P.max_tiles + t] = s_cnt[0] == PK_NO ? PK_NO : G.base + s_cnt[0];
        {
            // Read back what the tile has just published, a word per 64 bytes of REC and of the bitmap: a STORE does not leave
            // its line in the L2 (whoever loads it next goes to memory: 460-480 cycles a dependent load, whichever XCD he is on),
            // a load does — and the chain's workgroups share this XCD's L2, so the walks of the next pass take their hops at
            // 160-170 cycles (tools/ubench/xwg_hop.hip, profiles/r04_ubench_xwg_hop.txt).  Only a launch that goes on can use
            // that: a new launch starts by invalidating the L2.  (Stores and loads may pass each other on the way: the line
            // ends up resident and current either way, the L2 is where this XCD's stores are performed.)
            uint32_t acc = 0;
            const uint32_t* const rb = P.rec2[npar] + G.po + G.base;
            for (uint32_t i = (uint32_t)tid * 16u; i < G.tl; i += PT_THREADS * 16u) acc ^= xld(rb + i);
            for (uint32_t i = (uint32_t)tid * 16u; i < G.own_words; i += PT_THREADS * 16u) acc ^= xld(bits_dst + (G.base >> 5) + i);
            TW_SINK(acc);
        }
        // ---- the tables are out: arrive ----
        tw_store_wait();
        __syncthreads();
        if (tid == 0) {
            unsigned long long add = 1ull;
            if (it == 0u) {
                const uint32_t o = atomicOr(P.pxmask + g, 1u << mm_xcc_id());
                TW_KEEP(o);
                tw_store_wait();
            }
            if (it > 0u && (P.tune & 0x10000u)) { dwork += (uint32_t)(clock64() - dw0); ++dn; }   // (diagnostics: ... and ends)
            if (P.pinject && P.pinject == it && t == 1u) {
                // The test hook's stop, declared like everybody else's: only into an EMPTY high half.  (Until round 5 it was
                // ADDED with the arrival; when the chain's yield had been declared in the same iteration the two declarations
                // summed to an iteration nobody ever reaches, and the chain's workgroups waited for each other for good — a
                // dense 260 000-player pool under tests/stress.py with MM_PAIR_PINJECT=2 hung the device until the process
                // was killed.  No production path adds to the high half.)
                for (;;) {
                    const unsigned long long o = xld64(bar);
                    if (o >> 32) { atomicAdd(bar, 1ull); break; }
                    if (atomicCAS(bar, o, (o + 1ull) | ((unsigned long long)(PF_INJECT | ((it + 1u) << 8)) << 32)) == o) break;
                }
            } else atomicAdd(bar, add);
        }
        E.store(P, g, G.qo);                     // nobody in this launch waits for the lobbies: behind the arrival
        TMARK(4);
    }
    if (!ended && !stop) return;                 // (shim launches: the resident state goes on in the next launch)

    // ---- epilogue: the chain's state back into its committed form (what kp_round_commit / kp_round_stage do) ----
    const int tid = tid_o, lane = tid & 63;
    const bool tmr = t == 1u && tid == 0;
    __syncthreads();
    for (uint32_t i = tid; i < G.own_words; i += PT_THREADS) bits_com[(G.base >> 5) + i] = s_bits[i];
    for (uint32_t i = tid; i < G.tl; i += PT_THREADS)           // (a chain that ended in mid-sweep: "on the long list" is no value to keep)
        if (s_nx[i] == NX_PEND) s_nx[i] = (uint16_t)NX_INV;
    __syncthreads();
    {
        uint4* const nx4 = (uint4*)G.gnx;
        for (uint32_t i = tid; i < (G.tl + 7u) >> 3; i += PT_THREADS) nx4[i] = ((const uint4*)s_nx)[i];
    }
    if (tid == 0) L.ctl[0] = 1;
    if (t == 0 && tid == 0) {
        RoundState S = L.S;
        if (S.has_anchor && S.a_oi != PK_NO) {   // the seated anchor's values, not fetched on the way
            S.a_slot = P.q_slot[G.qo + S.a_oi]; S.a_rating = P.q_rating[G.qo + S.a_oi]; S.a_cons = P.q_cons[G.qo + S.a_oi];
        }
        if (!S.done && P.pyq[g] && S.qlen <= P.pyq[g]) S.want_compact = 1u;      // (the yield is for a compaction)
        round_state_commit(pc, S);
        if (S.done) pc->stage = PS_DONE;
        pc->pfail = stop;
        pc->ppass += L.ctl[2];
        pc->pxm = xld(P.pxmask + g);
    }
    if (tmr) {
        for (int k = 0; k < 16; ++k) if (L.tm[k]) atomicAdd(&pc->ptm[k], L.tm[k]);
        atomicAdd(&pc->ptm[5], L.ctl[2]);
    }
    if ((P.tune & 0x2000u) && lane == 0 && tst) atomicAdd(&pc->tested, (unsigned long long)tst);
    if ((P.tune & 0x10000u) && tid == 0 && dn) {              // which tile the chain's barrier waits for (grec is idle in kp_rounds batches)
        uint32_t* const dg = (uint32_t*)(P.grec + (size_t)g * P.gstride + t);
        atomicAdd(dg + 0, dwork);
        atomicAdd(dg + 1, dn);
    }
#undef TMARK
}

// ------------------------------------------------------------------------------------
// kp_group: the second level of the route, for chains of many tiles (a 3M-player chain of a 10M pool is 366
// tiles of 8192: one dependent hop per tile and pass was 35 us of a 61 us pass).  One launch behind every
// kp_round, grid (groups of PK_GS tiles, rating groups): for EVERY entry position x of the group's first
// tile — where a cursor that comes from the group before lands: partners lie inside the tile after the
// anchor's — the hops of the walk's fast path (kp_round section 1: exit anchor with a partner that is still
// queued, or a clean run through a tile) are followed to the end of the group, on the tables kp_round has just
// published and the bitmap of the pass to come, i.e. exactly what the next walk would read hop by hop:
//     grec[x] = (position where the walk goes on, lobbies on the way, the last partner taken, -)
// Anything else on the way (no partner inside the horizon, none at all, a partner that has left) ends the
// composition there: the walk's general code takes over at that position, as it always did.  The next walk then
// takes one hop per group it only passes through, and walks tile by tile inside its own group alone:
// tiles / PK_GS + PK_GS hops instead of tiles.
// ------------------------------------------------------------------------------------
template <uint32_t TP>
__global__ __launch_bounds__(1024) void kp_group(PairParams P, uint32_t r_next)
{
    constexpr uint32_t PK_T = TP;                 // the tile length of this instantiation
    (void)PK_T;
    const uint32_t g = blockIdx.y, gr = blockIdx.x;
    const uint32_t m = P.bm[g];
    if (m == 0u) return;
    const uint32_t ntiles = (m + PK_T - 1u) / PK_T;
    if (gr * P.grp >= ntiles) return;
    const uint32_t cpar = r_next & 1u;            // what the round before wrote = what the next walk reads
    if (!(P.pchains + g)->rs[cpar].live) return;
    const size_t po = (size_t)g * P.pstride;
    const uint32_t* const rec = P.rec2[cpar] + po;
    const uint32_t* const bits = P.bitsp[cpar] + (size_t)g * P.bits_stride;
    uint4* const out = P.grec + (size_t)g * P.gstride + (size_t)gr * PK_T;           // one tile's worth of entries per group
    const uint32_t t0 = gr * P.grp, gend = t0 + P.grp;
    // Which entries can the next walk use at all?  A cursor that comes from the group before leaves it through an exit
    // anchor of ITS last tile (a partner lies inside the tile after its anchor's) or runs off that tile clean: the
    // landing positions of that tile's REC, a few dozen of the tile's thousands.  Only those are composed (and stamped
    // with the round: the walk takes an entry of this round only, anything else it walks tile by tile as before —
    // the first group, a partner found beyond the horizon).
    __shared__ uint32_t s_mark[PK_T / 32u];
    __shared__ uint32_t s_list[PK_T];
    __shared__ uint32_t s_n;
    for (uint32_t i = threadIdx.x; i < PK_T / 32u; i += 1024u) s_mark[i] = 0;
    if (threadIdx.x == 0) s_n = 0;
    __syncthreads();
    for (uint32_t back = 1; back <= 2u && back <= t0; ++back) {      // (two tiles back: next[] made under a longer tile reaches further)
        const uint32_t tp = t0 - back, tlp = dev_min_u32(PK_T, m - tp * PK_T);
        constexpr uint32_t GE = PK_T / 1024u ? PK_T / 1024u : 1u;
        uint32_t rv[GE];
#pragma unroll
        for (uint32_t i = 0; i < GE; ++i) {
            const uint32_t xp = threadIdx.x + i * 1024u;
            rv[i] = xp < tlp ? rec[(size_t)tp * PK_T + xp] : (REC_NONE << 30);
        }
#pragma unroll
        for (uint32_t i = 0; i < GE; ++i) {
            const uint32_t kind = rv[i] >> 30, land = rv[i] & 0x1FFFFu;
            uint32_t nxt = PK_NO;
            if (kind == REC_PARTNER) nxt = tp * PK_T + land;                  // the position behind the partner
            else if (kind == REC_CLEAN) nxt = (tp + 1u) * PK_T;
            if (nxt != PK_NO && nxt / PK_T == t0) atomicOr(&s_mark[(nxt % PK_T) >> 5], 1u << (nxt & 31u));
        }
    }
    __syncthreads();
    for (uint32_t i = threadIdx.x; i < PK_T / 32u; i += 1024u) {
        uint32_t w = s_mark[i];
        if (!w) continue;
        const uint32_t at = atomicAdd(&s_n, (uint32_t)__popc(w));
        uint32_t k = 0;
        while (w) { s_list[at + k++] = (i << 5) + (uint32_t)__ffs((int)w) - 1u; w &= w - 1u; }
    }
    __syncthreads();
    const uint32_t n = s_n;
    for (uint32_t li = threadIdx.x; li < n; li += 1024u) {
        const uint32_t e = s_list[li];
        uint32_t tt = t0, x = e, cnt = 0, qlast = PK_NO;
        const uint32_t tl0 = dev_min_u32(PK_T, m - t0 * PK_T);
        if (x >= tl0) { tt = t0 + 1u; x = 0; }                                 // behind the end of the queue: the walk moves on itself
        else {
            uint32_t rr = rec[(size_t)t0 * PK_T + x];
            for (uint32_t hop = 0; hop < 4u * PK_GS + 8u; ++hop) {
                const uint32_t kind = rr >> 30, c = (rr >> 17) & 0x1FFFu, land = rr & 0x1FFFFu;
                uint32_t nt, nx, r2 = 0;
                if (kind == REC_PARTNER) {
                    // one trip: the partner's bitmap word and the REC behind the partner, as in the walk's fast path
                    const uint32_t q = tt * PK_T + land - 1u, nxt = q + 1u;
                    const uint32_t bw = bits[q >> 5];
                    if (nxt < m && nxt / PK_T < gend) r2 = rec[nxt];
                    if (!((bw >> (q & 31u)) & 1u)) break;                      // the partner has left: the walk's general code
                    cnt += c + 1u;
                    qlast = q;
                    nt = nxt / PK_T;
                    nx = nxt % PK_T;
                } else if (kind == REC_CLEAN) {
                    nt = tt + 1u;
                    nx = 0;
                    if (nt < gend && nt < ntiles) r2 = rec[(size_t)nt * PK_T];
                    cnt += c;
                } else break;                                                  // no partner inside the horizon / none at all
                tt = nt;
                x = nx;
                rr = r2;
                // behind the group, behind the queue, or behind the end of the last tile: the walk goes on from here
                if (nt >= gend || nt >= ntiles || nx >= dev_min_u32(PK_T, m - nt * PK_T)) break;
            }
        }
        // (an entry still on its way at the bound of the loop stands where it got to: every prefix of the path is valid)
        out[e] = uint4{tt * PK_T + x, cnt, qlast, r_next};
    }
}

// kp_round_commit: after a batch, the latest parity back into the chain's committed state (what
// the host, the compaction kernels, kp_late and kp_finish read).  Grid (tiles, groups).
template <uint32_t TP>
__global__ __launch_bounds__(256) void kp_round_commit(PairParams P, uint32_t r_next)
{
    constexpr uint32_t PK_T = TP;                 // the tile length of this instantiation
    (void)PK_T;
    const uint32_t g = blockIdx.y, t = blockIdx.x;
    PairChain* const pc = P.pchains + g;
    if (!pc->fast || pc->stage != PS_TILED || t >= (pc->m + PK_T - 1u) / PK_T) return;
    const uint32_t cpar = r_next & 1u;
    const int tid = threadIdx.x;
    const uint32_t m = pc->m;
    const uint32_t w0 = t * (PK_T / 32u);
    const uint32_t nw = (dev_min_u32(PK_T, m - t * PK_T) + 31u) >> 5;
    const uint32_t* const src = P.bitsp[cpar] + (size_t)g * P.bits_stride + w0;
    uint32_t* const dst = P.bits[pc->buf] + (size_t)g * P.bits_stride + w0;
    for (uint32_t i = tid; i < nw; i += 256) dst[i] = src[i];
    __syncthreads();
    if (t == 0 && tid == 0) {
        const RoundState S = pc->rs[cpar];
        round_state_commit(pc, S);
    }
}

// the host asks for a compaction the walk has not asked for: a chain whose QUEUED players would fit the tiles of a kp_rounds
// launch while its index space does not yet (a bit per rating group)
__global__ __launch_bounds__(64) void kp_ask_compact(PairParams P, uint32_t mask)
{
    const uint32_t g = blockIdx.x;
    PairChain* const pc = P.pchains + g;
    if (threadIdx.x == 0 && ((mask >> g) & 1u) && pc->fast && pc->stage == PS_TILED) pc->want_compact = 1u;
}

// the stage flips after every workgroup of kp_round_commit has read it
__global__ __launch_bounds__(64) void kp_round_stage(PairParams P, uint32_t r_next)
{
    const uint32_t g = blockIdx.x;
    PairChain* const pc = P.pchains + g;
    if (!pc->fast || pc->stage != PS_TILED) return;
    if (threadIdx.x == 0) {
        if (pc->rs[r_next & 1u].done) pc->stage = PS_DONE;
        // the host's wish for this batch (PairParams.pyq): compact as soon as the queued players fit — the compaction kernels are
        // enqueued behind every batch and look at want_compact themselves, no look of the host in between
        else if (P.pyq[g] && pc->qlen <= P.pyq[g]) pc->want_compact = 1u;
    }
}

// ------------------------------------------------------------------------------------
// Compaction of a tiled chain (asked for by the walk): survivors move to the front of the
// other buffer, next[] offsets are re-expressed in the new index space.
//   kc_words   per tile: queued players before each bitmap word (tile-local)
//   kc_plan    per chain: new first index of every tile, the new length, the new bitmap
//   kc_scatter per tile: move key / oidx / next[]
//   kc_commit  per chain: switch buffers
// ------------------------------------------------------------------------------------
template <uint32_t TP>
__global__ __launch_bounds__(256) void kc_words(PairParams P)
{
    constexpr uint32_t PK_T = TP;                 // the tile length of this instantiation
    (void)PK_T;
    __shared__ uint32_t s_wtot[4];
    const uint32_t g = blockIdx.y, t = blockIdx.x;
    const PairChain* const pc = P.pchains + g;
    if (!pc->fast || pc->stage != PS_TILED || !pc->want_compact || t >= (pc->m + PK_T - 1u) / PK_T) return;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const uint32_t m = pc->m;
    const uint32_t w0 = t * (PK_T / 32u);
    const uint32_t nw = (dev_min_u32(PK_T, m - t * PK_T) + 31u) >> 5;
    const uint32_t* const bits = P.bits[pc->buf] + (size_t)g * P.bits_stride + w0;
    const uint32_t pcw = (uint32_t)tid < nw ? (uint32_t)__popc(bits[tid]) : 0u;    // PK_T/32 = 256 words
    const uint32_t incl = wave_incl_scan(pcw, lane);
    if (lane == 63) s_wtot[wave] = incl;
    __syncthreads();
    uint32_t offw = 0;
    for (int x = 0; x < wave; ++x) offw += s_wtot[x];
    if ((uint32_t)tid < nw) P.wpre[(size_t)g * P.bits_stride + w0 + tid] = (uint16_t)(offw + incl - pcw);
    if (tid == 255) tc_row(P, TC_ALIVE, g)[t] = offw + incl;          // recount (also checks the bookkeeping)
}

template <uint32_t TP>
__global__ __launch_bounds__(1024) void kc_plan(PairParams P)
{
    constexpr uint32_t PK_T = TP;                 // the tile length of this instantiation
    (void)PK_T;
    const uint32_t g = blockIdx.x;
    PairChain* const pc = P.pchains + g;
    if (!pc->fast || pc->stage != PS_TILED || !pc->want_compact) return;
    __shared__ uint32_t s_total;
    const int tid = threadIdx.x;
    uint32_t* const talive = tc_row(P, TC_ALIVE, g);
    uint32_t* const tbase = tc_row(P, TC_BASE, g);
    if (tid == 0) {
        uint32_t run = 0;
        for (uint32_t t = 0; t < (pc->m + PK_T - 1u) / PK_T; ++t) { tbase[t] = run; run += talive[t]; }
        s_total = run;
        pc->new_m = run;
        if (run != pc->qlen) pc->err |= MM_ERRF_SEAT_INVARIANT;
    }
    __syncthreads();
    const uint32_t nm = s_total;
    uint32_t* const nbits = P.bits[pc->buf ^ 1u] + (size_t)g * P.bits_stride;
    for (uint32_t i = tid; i < (nm >> 5) + 2u; i += 1024) {
        const uint32_t lo = i << 5;
        nbits[i] = lo + 32u <= nm ? 0xFFFFFFFFu : (lo < nm ? (1u << (nm - lo)) - 1u : 0u);
    }
}

template <uint32_t TP>
__global__ __launch_bounds__(1024) void kc_scatter(PairParams P)
{
    constexpr uint32_t PK_T = TP;                 // the tile length of this instantiation
    (void)PK_T;
    const uint32_t g = blockIdx.y, t = blockIdx.x;
    const PairChain* const pc = P.pchains + g;
    if (!pc->fast || pc->stage != PS_TILED || !pc->want_compact || t >= (pc->m + PK_T - 1u) / PK_T) return;
    const int tid = threadIdx.x;
    const uint32_t m = pc->m, buf = pc->buf;
    const size_t po = (size_t)g * P.pstride;
    const uint32_t* const bits = P.bits[buf] + (size_t)g * P.bits_stride;
    const uint16_t* const wpre = P.wpre + (size_t)g * P.bits_stride;
    const uint32_t* const tbase = tc_row(P, TC_BASE, g);
    const uint32_t base = t * PK_T;
    const uint32_t tl = dev_min_u32(PK_T, m - base);
    for (uint32_t x = tid; x < tl; x += 1024) {
        const uint32_t i = base + x;
        const uint32_t bw = bits[i >> 5];
        if (!((bw >> (i & 31u)) & 1u)) continue;
        const uint32_t r = tbase[t] + wpre[i >> 5] + (uint32_t)__popc(bw & ((1u << (i & 31u)) - 1u));
        P.key[buf ^ 1u][po + r] = P.key[buf][po + i];
        P.oidx[buf ^ 1u][po + r] = P.oidx[buf][po + i];
        const uint32_t o = P.nx16[buf][po + i];
        uint32_t no = NX_INV;
        if (o == NX_NONE) no = NX_NONE;
        else if (o != NX_INV && o != NX_FAR) {
            const uint32_t q = i + o;
            const uint32_t qw = q < m ? bits[q >> 5] : 0u;
            if ((qw >> (q & 31u)) & 1u) {
                const uint32_t rq = tbase[q / PK_T] + wpre[q >> 5] + (uint32_t)__popc(qw & ((1u << (q & 31u)) - 1u));
                no = rq - r;
            }
        }
        P.nx16[buf ^ 1u][po + r] = (uint16_t)no;
    }
}

template <uint32_t TP>
__global__ __launch_bounds__(1024) void kc_commit(PairParams P)
{
    constexpr uint32_t PK_T = TP;                 // the tile length of this instantiation
    (void)PK_T;
    const uint32_t g = blockIdx.x;
    PairChain* const pc = P.pchains + g;
    // the last kernel behind every batch: the arrival word, the XCD mask and the yield word of the next kp_rounds launch start
    // from zero (round 5: a memset command of its own in front of every launch was 6 us of launch gap, eight times a tick)
    if (threadIdx.x == 0) { P.pbar[g] = 0ull; P.pxmask[g] = 0u; if (g == 0u) *P.pyield = 0u; }
    if (!pc->fast || pc->stage != PS_TILED || !pc->want_compact) return;
    const int tid = threadIdx.x;
    const uint32_t nm = pc->new_m;
    const uint32_t nt = (nm + PK_T - 1u) / PK_T;
    uint32_t* const talive = tc_row(P, TC_ALIVE, g);
    for (uint32_t t = tid; t < P.max_tiles; t += 1024) talive[t] = t < nt ? dev_min_u32(PK_T, nm - t * PK_T) : 0u;
    __syncthreads();
    if (tid == 0) {
        pc->m = nm;
        pc->ntiles = nt;
        pc->buf ^= 1u;
        pc->want_compact = 0;
        if (nm < PL_MAX) pc->stage = PS_LATE;
    }
}

// ------------------------------------------------------------------------------------
// kp_finish: survivors back into the chain's q_* arrays (queue order preserved = requeue
// order, worker.ex:239-248), the anchor back into the LobbyState record, tick counters.
// One workgroup per rating group.
// ------------------------------------------------------------------------------------
__global__ __launch_bounds__(1024) void kp_finish(PairParams P)
{
    __shared__ uint32_t wtot[16];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const uint32_t g = blockIdx.x;
    PairChain* const pc = P.pchains + g;
    if (!pc->fast) return;
    const uint32_t c = P.mode * P.n_groups + g;
    ChainDev* const ch = P.chains + c;
    const size_t qo = (size_t)c * P.capacity, po = (size_t)g * P.pstride;
    const uint32_t m = pc->m;
    const uint32_t* const oidx = P.oidx[pc->buf] + po;
    const uint32_t* const bits = P.bits[pc->buf] + (size_t)g * P.bits_stride;
    uint32_t* const t_rating = P.key[pc->buf ^ 1u] + po;        // free buffers as staging
    uint32_t* const t_cons = P.oidx[pc->buf ^ 1u] + po;
    uint32_t* const t_slot = P.scratch + po;
    uint32_t wr = 0;
    for (uint32_t base = 0; base < m; base += 1024u) {
        const uint32_t i = base + (uint32_t)tid;
        const bool live = i < m && ((bits[i >> 5] >> (i & 31u)) & 1u);
        const unsigned long long bm = __ballot(live);
        if (lane == 0) wtot[wave] = (uint32_t)__popcll(bm);
        __syncthreads();
        uint32_t off = wr, tot = 0;
        for (int x = 0; x < 16; ++x) {
            if (x < wave) off += wtot[x];
            tot += wtot[x];
        }
        if (live) {
            const uint32_t d = off + (uint32_t)__popcll(bm & ((1ull << lane) - 1ull));
            const uint32_t oi = oidx[i];
            t_rating[d] = (uint32_t)P.q_rating[qo + oi];
            t_cons[d] = P.q_cons[qo + oi];
            t_slot[d] = P.q_slot[qo + oi];
        }
        wr += tot;
        __syncthreads();
    }
    for (uint32_t i = tid; i < wr; i += 1024u) {
        P.q_rating[qo + i] = (int32_t)t_rating[i];
        P.q_cons[qo + i] = t_cons[i];
        P.q_slot[qo + i] = t_slot[i];
    }
    if (tid == 0) {
        LobbyDev& lb = ch->lobby;
        lb.n = pc->has_anchor;
        lb.cnt[0] = lb.cnt[1] = 0;
        if (pc->has_anchor) {
            const uint32_t t = pc->a_team;
            lb.cnt[t] = 1;
            lb.slot[t][0] = pc->a_slot;
            lb.rating[t][0] = pc->a_rating;
            lb.cons[t][0] = pc->a_cons;
        }
        ch->len = wr;
        ch->head_state = 0;
        ch->purged = 0;
        ch->before = pc->before;
        ch->n_out = pc->n_out;
        ch->passes = pc->passes;
        ch->pairs = pc->pairs;
        ch->scanned = pc->scanned;
        ch->err |= pc->err | (wr != pc->qlen ? MM_ERRF_SEAT_INVARIANT : 0u);
    }
}
