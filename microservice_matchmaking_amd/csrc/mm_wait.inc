// mm_wait.inc — the clock of include/mm_wait.h on the device: expiry selection as a stable stream compaction over a
// mode's queues, the same selection gathering the rows of a move into another mode (mm_move), the rotation of blocked
// lobbies' seats to their queues' tails (mm_rotate), wait statistics, a slot's place in its queue (mm_locate), the partner
// counts of mm_partners and mm_partner_stats.  Included by mm_engine.hip (ChainDev, LobbyDev, dev_min_u32, wave_incl_scan,
// the WT_* chunk geometry); the host functions that launch these kernels (wait_alloc .. mm_wait_stats) are there, like the
// pair and team host loops.  k_wait_matched sits beside k_pack_results in mm_engine.hip, whose PackArgs it shares.  DESIGN.md §4.6.
//
// The waiting players of a mode are walked in ONE order by every kernel here — rating group ascending; within a group
// the stored lobby's seats as mm_lobby_state lists them, then the queue from head to tail — cut into chunks of WT_CHUNK
// queue entries, one workgroup per chunk (a chain of 300 000 players is 147 workgroups, not k_purge's one).  A group
// has at least one chunk: an empty queue may still have a stored lobby, and the group's first chunk carries its seats.
// The walk is written once, in the first part of this file, and every kernel that walks is made of its pieces:
//   WaitChunk / wait_chunk   where a workgroup's chunk lies: group, queue, the chunk's rows;
//   wait_load<COLS>          a wave's WT_PER_WAVE queue entries into registers: the streamed columns, then the gathers;
//   wait_seat, wait_live     the lane's seat of the stored lobby (wave 0 of a group's first chunk), and "does it wait?";
//   wait_count_body          per-wave counts into the chunk's rows (k_wait_count, k_loc_count, k_fit_count);
//   wait_rank                a selected lane's place behind the wave's base — the stable compactions;
//   wait_wave_sum / wait_wave_max / wait_wave_sum64, wait_bucket   what the two statistics kernels reduce with.
// mm_expire is count / scan / scatter over that order, the shape of k_bucket_*: per-wave counts, one exclusive scan
// down the (chunk, wave) rows, then every wave writes its selected entries at base + wave-ballot rank — a stable
// compaction, so the list is in queue order.  Per entry: q_slot streamed, stamp[slot] and state[slot] gathered.
// This file is not self-contained: it needs six macros defined BEFORE its #include, which mm_engine.hip does right in front
// of it — WT_THREADS, WT_WAVES, WT_PER_WAVE, WT_CHUNK, WT_ROWS, WT_SEATS, the chunk geometry of every kernel below.  They
// live there because the host code sizes its buffers and grids by them (wait_alloc, wait_grid) and because the tests read
// WT_CHUNK out of mm_engine.hip (tests/geometry.py's SOURCES, tests/wait_scenarios.py: chains of WT_CHUNK - 1 / + 1
// players); a test suite that predates this file must find it where it always was.
#if !defined(WT_THREADS) || !defined(WT_WAVES) || !defined(WT_PER_WAVE) || !defined(WT_CHUNK) || !defined(WT_ROWS) || !defined(WT_SEATS)
#error "mm_wait.inc: define the WT_* chunk geometry before including this file (mm_engine.hip does)"
#endif

struct WaitGroupDev {                         // mm_wait_group (include/mm_wait.h) with a type atomicAdd takes
    uint32_t waiting, oldest_age;
    unsigned long long age_sum;
    uint32_t hist[33];
    uint32_t pad;
};

struct WaitParams {
    uint32_t mode, n_groups, capacity, teams;
    uint32_t now, max_age;
    uint32_t max_chunks;                      // chunks `rows` has room for
    const ChainDev* chains;
    const uint32_t* q_slot;
    const uint32_t* stamp;
    uint8_t* state;
    uint32_t* rows;                           // [chunk][WT_ROWS]; behind them the total ([max_chunks * WT_ROWS])
    uint32_t* out_slot;                       // the expired, in order: slot | rating group | age
    uint32_t* out_group;
    uint32_t* out_age;
    WaitGroupDev* stats;                      // [n_groups], zeroed by the host
};

static __device__ __forceinline__ uint32_t wait_chunks_of(uint32_t len) { return len ? (len + WT_CHUNK - 1u) / WT_CHUNK : 1u; }

// ---- the walk's pieces ----

// Where chunk b of the mode lies: four words, the same for all threads of the workgroup (scalar registers).  The addresses
// are derived from them where they are used and not kept: held across a kernel's inner loops they cost k_par_count_all
// two spilled SGPRs and k_fit_search its eighth wave.
struct WaitChunk {
    uint32_t b, g, k, len;                    // the chunk; its rating group, its number inside the group, the queue's length
    // the queue's first entry in q_slot / q_rating / q_cons
    __device__ __forceinline__ size_t qo(const WaitParams& P) const { return (size_t)(P.mode * P.n_groups + g) * P.capacity; }
    // the chunk's counters: [0] the seats', [1 + wave] a wave's; and those of the group's first chunk
    __device__ __forceinline__ uint32_t* row(const WaitParams& P) const { return P.rows + (size_t)b * WT_ROWS; }
    __device__ __forceinline__ const uint32_t* group_row(const WaitParams& P) const { return P.rows + (size_t)(b - k) * WT_ROWS; }
    // the group's stored lobby
    __device__ __forceinline__ const LobbyDev& lobby(const WaitParams& P) const { return P.chains[P.mode * P.n_groups + g].lobby; }
    // the wave's first entry; does the wave carry the seats' row?
    __device__ __forceinline__ uint32_t first(int wave) const { return k * WT_CHUNK + (uint32_t)wave * WT_PER_WAVE; }
    __device__ __forceinline__ bool seats(int wave) const { return wave == 0 && k == 0u; }
};

// The wave's number as a scalar: its first entry, its row and whether it carries the seats then cost no vector register
// and no lane mask.
static __device__ __forceinline__ int wait_wave() { return __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6)); }

// false: b is past the mode's last chunk.
static __device__ __forceinline__ bool wait_chunk(const WaitParams& P, uint32_t b, WaitChunk& c)
{
    if (b >= P.max_chunks) return false;
    uint32_t base = 0;
    c.b = b;
    for (c.g = 0; c.g < P.n_groups; ++c.g) {
        c.len = dev_min_u32(P.chains[P.mode * P.n_groups + c.g].len, P.capacity);
        const uint32_t nb = wait_chunks_of(c.len);
        if (b < base + nb) { c.k = b - base; return true; }
        base += nb;
    }
    return false;
}

// The (team, seat) of the idx-th seated player of a stored lobby in mm_lobby_state's order (team by team); false past the last.
static __device__ __forceinline__ bool wait_seat_at(const LobbyDev& lb, uint32_t teams, uint32_t idx, uint32_t& t, uint32_t& i)
{
    for (t = 0; t < teams && t < MM_MAX_TEAMS; ++t) {
        const uint32_t c = dev_min_u32(lb.cnt[t], 8u);
        if (idx < c) { i = idx; return true; }
        idx -= c;
    }
    return false;
}

// Lane `lane`'s seat of the chunk's stored lobby as the LobbyDev record holds it: slot, rating, constraint word.  MM_NO_SLOT
// in a chunk that is not its group's first and past the last seat (a lobby seats at most WT_SEATS).  What a caller does
// not read is not loaded.
struct WaitSeat {
    uint32_t sl, cn;
    int32_t rt;
};

static __device__ __forceinline__ WaitSeat wait_seat(const WaitParams& P, const WaitChunk& c, int lane)
{
    WaitSeat s;
    s.sl = MM_NO_SLOT; s.cn = 0u; s.rt = 0;
    uint32_t t = 0, i = 0;
    if (c.k == 0u && (uint32_t)lane < WT_SEATS && wait_seat_at(c.lobby(P), P.teams, (uint32_t)lane, t, i)) {
        s.sl = c.lobby(P).slot[t][i];
        s.rt = c.lobby(P).rating[t][i];
        s.cn = c.lobby(P).cons[t][i];
    }
    return s;
}

// Is the player in `sl` waiting (LIVE: not cancelled, not expired before) ...
static __device__ __forceinline__ bool wait_live(const WaitParams& P, uint32_t sl) { return sl < P.capacity && P.state[sl] == MM_ST_LIVE; }

// ... and for how long?
static __device__ __forceinline__ bool wait_age(const WaitParams& P, uint32_t sl, uint32_t& age)
{
    if (!wait_live(P, sl)) return false;
    age = P.now - P.stamp[sl];
    return true;
}

// The selection by age, of the count and of every scatter: strictly older than the threshold.
static __device__ __forceinline__ bool wait_older(const WaitParams& P, uint32_t age) { return age > P.max_age; }

// A wave's WT_PER_WAVE queue entries from w0 on, in registers.  COLS says what is read beside the slots: WL_ROW streams the
// entry's rating and constraint word with them (q_rating, q_cons), WL_AGE gathers stamp[slot] (age = now - stamp; it means
// something for a LIVE entry only), WL_TAG gathers tag[slot]; a column left out reads 0.  state[slot] is always gathered.
// Two levels — the streamed columns, then the gathers — and every load of a level is issued before the first one is used
// (the gathers are latency, not bandwidth).  Bit r of the result: this lane's entry r is LIVE.  Row WT_ITERS of the
// streamed columns is nobody's entry: k_fit_search keeps the seat there.
#define WT_ITERS (WT_PER_WAVE / 64)
#define WL_ROW 1u
#define WL_AGE 2u
#define WL_TAG 4u
struct WaitRows {
    uint32_t sl[WT_ITERS + 1], cn[WT_ITERS + 1];
    int32_t rt[WT_ITERS + 1];
    uint32_t age[WT_ITERS], tg[WT_ITERS];
};

template <uint32_t COLS>
static __device__ __forceinline__ uint32_t wait_load(const WaitParams& P, const WaitChunk& c, uint32_t w0, int lane, WaitRows& R,
                                                     const int32_t* __restrict__ q_rating = nullptr,
                                                     const uint32_t* __restrict__ q_cons = nullptr,
                                                     const uint32_t* __restrict__ tag = nullptr)
{
    const size_t qo = c.qo(P);
#pragma unroll
    for (uint32_t r = 0; r < WT_ITERS; ++r) {
        const uint32_t i = w0 + r * 64 + lane;
        const bool in = i < c.len;
        R.sl[r] = in ? P.q_slot[qo + i] : MM_NO_SLOT;
        R.rt[r] = (COLS & WL_ROW) && in ? q_rating[qo + i] : 0;
        R.cn[r] = (COLS & WL_ROW) && in ? q_cons[qo + i] : 0u;
    }
    uint8_t st[WT_ITERS];
#pragma unroll
    for (uint32_t r = 0; r < WT_ITERS; ++r) {
        const bool in = R.sl[r] < P.capacity;
        st[r] = in ? P.state[R.sl[r]] : (uint8_t)MM_ST_FREE;
        R.age[r] = (COLS & WL_AGE) && in ? P.stamp[R.sl[r]] : P.now;
        R.tg[r] = (COLS & WL_TAG) && in ? tag[R.sl[r]] : 0u;
    }
    uint32_t live = 0;
#pragma unroll
    for (uint32_t r = 0; r < WT_ITERS; ++r) {
        if (st[r] == MM_ST_LIVE) live |= 1u << r;
        R.age[r] = P.now - R.age[r];
    }
    return live;
}

// Where a selected lane writes in a stable compaction: `base` plus the selected lanes below it (lt: the lanes below this
// one); base moves on behind the wave's selected.  Every lane of the wave must call it (ballot).
static __device__ __forceinline__ uint32_t wait_rank(bool sel, unsigned long long lt, uint32_t& base)
{
    const unsigned long long m = __ballot(sel);
    const uint32_t at = base + (uint32_t)__popcll(m & lt);
    base += (uint32_t)__popcll(m);
    return at;
}

// A value over the wave, in every lane: a butterfly of shuffles.
static __device__ __forceinline__ uint32_t wait_wave_sum(uint32_t v, int lane)
{
    for (int d = 32; d >= 1; d >>= 1) v += (uint32_t)__shfl((int)v, lane ^ d);
    return v;
}

static __device__ __forceinline__ uint32_t wait_wave_max(uint32_t v, int lane)
{
    for (int d = 32; d >= 1; d >>= 1) {
        const uint32_t o = (uint32_t)__shfl((int)v, lane ^ d);
        v = o > v ? o : v;
    }
    return v;
}

static __device__ __forceinline__ unsigned long long wait_wave_sum64(unsigned long long v, int lane)
{
    for (int d = 32; d >= 1; d >>= 1) {
        const uint32_t lo = (uint32_t)__shfl((int)(uint32_t)v, lane ^ d), hi = (uint32_t)__shfl((int)(uint32_t)(v >> 32), lane ^ d);
        v += ((unsigned long long)hi << 32) | lo;
    }
    return v;
}

// The bucket of MM_WAIT_HIST and MM_PARTNER_HIST: 0 for 0, else the value's bit length.
static __device__ __forceinline__ uint32_t wait_bucket(uint32_t v) { return v ? 32u - (uint32_t)__builtin_clz(v) : 0u; }

// The count of a count / scan / scatter: how many of a wave's entries are selected into row[1 + wave], how many of the
// seats into row[0].  Selected: LIVE, and (OLDER) older than P.max_age.  SEATS false: the seats' row counts 0.
template <bool OLDER, bool SEATS>
static __device__ __forceinline__ void wait_count_body(const WaitParams& P)
{
    const int tid = threadIdx.x, lane = tid & 63, wave = wait_wave();
    for (uint32_t b = blockIdx.x;; b += gridDim.x) {
        WaitChunk c;
        if (!wait_chunk(P, b, c)) return;
        const uint32_t w0 = c.first(wave);
        uint32_t cnt = 0;
        if (w0 < c.len) {
            WaitRows R;
            const uint32_t live = wait_load<OLDER ? WL_AGE : 0u>(P, c, w0, lane, R);
#pragma unroll
            for (uint32_t r = 0; r < WT_ITERS; ++r)
                cnt += (uint32_t)__popcll(__ballot(((live >> r) & 1u) && (!OLDER || wait_older(P, R.age[r]))));
        }
        if (lane == 0) c.row(P)[1 + wave] = cnt;
        if (wave == 0) {
            uint32_t age = 0;
            const uint32_t sl = SEATS ? wait_seat(P, c, lane).sl : MM_NO_SLOT;
            const bool sel = OLDER ? wait_age(P, sl, age) && wait_older(P, age) : wait_live(P, sl);
            const unsigned long long m = __ballot(sel);
            if (lane == 0) c.row(P)[0] = (uint32_t)__popcll(m);
        }
    }
}

__global__ __launch_bounds__(WT_THREADS) void k_wait_fill(uint32_t n, uint32_t* __restrict__ stamp, uint32_t now)
{
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) stamp[i] = now;
}

__global__ __launch_bounds__(WT_THREADS) void k_wait_count(WaitParams P) { wait_count_body<true, true>(P); }

// Exclusive scan down n_rows counters, in place; the total goes to *total.  One workgroup; every thread must call it.
static __device__ __forceinline__ void rows_scan_body(uint32_t* __restrict__ rows, uint32_t n_rows, uint32_t* __restrict__ total_out)
{
    __shared__ uint32_t wtot[WT_WAVES];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const uint32_t per = (n_rows + WT_THREADS - 1) / WT_THREADS;
    const uint32_t r0 = dev_min_u32(tid * per, n_rows), r1 = dev_min_u32(r0 + per, n_rows);
    uint32_t s = 0;
    for (uint32_t r = r0; r < r1; ++r) s += rows[r];
    const uint32_t incl = wave_incl_scan(s, lane);
    if (lane == 63) wtot[wave] = incl;
    __syncthreads();
    uint32_t run = incl - s;
    for (int w = 0; w < wave; ++w) run += wtot[w];
    for (uint32_t r = r0; r < r1; ++r) {
        const uint32_t h = rows[r];
        rows[r] = run;
        run += h;
    }
    if (tid == 0) {
        uint32_t total = 0;
        for (int w = 0; w < WT_WAVES; ++w) total += wtot[w];
        *total_out = total;
    }
}

// Exclusive scan down the rows of k_wait_count, in place; the total behind them.  One workgroup.
__global__ __launch_bounds__(WT_THREADS) void k_wait_scan(WaitParams P)
{
    uint32_t chunks = 0;
    for (uint32_t g = 0; g < P.n_groups; ++g) chunks += wait_chunks_of(dev_min_u32(P.chains[P.mode * P.n_groups + g].len, P.capacity));
    chunks = dev_min_u32(chunks, P.max_chunks);
    rows_scan_body(P.rows, chunks * WT_ROWS, P.rows + (size_t)P.max_chunks * WT_ROWS);
}

// What mm_move's scatter gathers beside the list (include/mm_wait.h): the rows of an enqueue into the other mode, on the
// device, at the ranks of the list — rating, rewritten constraint word, rating group as a byte (k_bucket_* take that
// column), and the stamp the player keeps.  cons' = (cons & keep) | to_mode, keep = ~cons_clear & MM_CONS_USER_MASK & ~0xF.
struct MoveCols {
    const int32_t* q_rating;
    const uint32_t* q_cons;
    int32_t* rating;
    uint32_t* cons;
    uint32_t* stamp;
    uint8_t* group;
    uint32_t keep, to_mode;
};

// What the non-marking scatter of the mm_*_if calls writes at a candidate's rank instead of the list: the query record
// par_count_body stages (x rating | y constraint word, un-rewritten | z rating group | w slot), the age the selection
// computed, and the partner count preset to 0.  n: the candidates the columns have room for.
struct CandCols {
    uint4* rec;
    uint32_t* age;
    uint32_t* cnt;
    uint32_t n;
};

// Every selected player at its rank, and marked as k_cancel marks a slot.  A slot is in one queue or one lobby, once:
// the mark a thread sets is read by nobody else, so the selection is the one k_wait_count counted.
// GATHER (mm_move): the selected player's row goes along — a queue entry's rating and constraint word from the position
// the wave streams anyway (wait_load's WL_ROW), a lobby seat's from the LobbyDev record; the stamp is the clock minus the
// age the selection computed.
// CAND (mm_expire_if, mm_move_if, mm_move_out_if): the same selection at the same ranks, but NOTHING is marked and no
// list is written — the row goes into C as a query record for the partner count; state[] is only read.
// wait_scatter_put: one selected player of rating group g, from a queue or from a seat, to rank `at`.
template <bool GATHER, bool CAND>
static __device__ __forceinline__ void wait_scatter_put(const WaitParams& P, const MoveCols& M, const CandCols& C, uint32_t at, uint32_t g,
                                                        uint32_t sl, int32_t rt, uint32_t cn, uint32_t age)
{
    if (CAND) {
        if (at >= C.n) return;
        C.rec[at] = make_uint4((uint32_t)rt, cn, g, sl);
        C.age[at] = age;
        C.cnt[at] = 0u;
        return;
    }
    if (at >= P.capacity) return;
    P.out_slot[at] = sl;
    P.out_group[at] = g;
    P.out_age[at] = age;
    if (GATHER) {
        M.rating[at] = rt;
        M.cons[at] = (cn & M.keep) | M.to_mode;
        M.group[at] = (uint8_t)g;
        M.stamp[at] = P.now - age;
    }
    P.state[sl] = MM_ST_CANCELLED;
}

template <bool GATHER, bool CAND>
static __device__ __forceinline__ void wait_scatter_body(const WaitParams& P, const MoveCols& M, const CandCols& C)
{
    constexpr uint32_t COLS = GATHER || CAND ? WL_AGE | WL_ROW : WL_AGE;
    const int tid = threadIdx.x, lane = tid & 63, wave = wait_wave();
    const unsigned long long lt = (1ull << lane) - 1ull;
    for (uint32_t b = blockIdx.x;; b += gridDim.x) {
        WaitChunk c;
        if (!wait_chunk(P, b, c)) return;
        const uint32_t w0 = c.first(wave);
        uint32_t base = c.row(P)[1 + wave];
        if (w0 < c.len) {
            WaitRows R;
            const uint32_t live = wait_load<COLS>(P, c, w0, lane, R, M.q_rating, M.q_cons);
#pragma unroll
            for (uint32_t r = 0; r < WT_ITERS; ++r) {
                const bool sel = ((live >> r) & 1u) && wait_older(P, R.age[r]);
                const uint32_t at = wait_rank(sel, lt, base);
                if (sel) wait_scatter_put<GATHER, CAND>(P, M, C, at, c.g, R.sl[r], R.rt[r], R.cn[r], R.age[r]);
            }
        }
        if (wave == 0) {
            const WaitSeat s = wait_seat(P, c, lane);
            uint32_t age = 0, seat_base = c.row(P)[0];
            const bool sel = wait_age(P, s.sl, age) && wait_older(P, age);
            const uint32_t at = wait_rank(sel, lt, seat_base);
            if (sel) wait_scatter_put<GATHER, CAND>(P, M, C, at, c.g, s.sl, s.rt, s.cn, age);
        }
    }
}

static __device__ __forceinline__ MoveCols move_cols_none()
{
    MoveCols none;
    none.q_rating = nullptr; none.q_cons = nullptr; none.rating = nullptr; none.cons = nullptr;
    none.stamp = nullptr; none.group = nullptr; none.keep = 0u; none.to_mode = 0u;
    return none;
}

static __device__ __forceinline__ CandCols cand_cols_none()
{
    CandCols none;
    none.rec = nullptr; none.age = nullptr; none.cnt = nullptr; none.n = 0u;
    return none;
}

__global__ __launch_bounds__(WT_THREADS) void k_wait_scatter(WaitParams P) { wait_scatter_body<false, false>(P, move_cols_none(), cand_cols_none()); }

// mm_move's and mm_move_out's scatter: the list as k_wait_scatter writes it, plus the rows — for k_bucket_* on this engine
// (mm_move), or for the host to hand to another engine's mm_enqueue_stamped (mm_move_out reads rating, word and stamp back).
__global__ __launch_bounds__(WT_THREADS) void k_move_scatter(WaitParams P, MoveCols M) { wait_scatter_body<true, false>(P, M, cand_cols_none()); }

// The candidates of an mm_*_if call: who k_wait_count counted, as query records at their ranks.  M: q_rating and q_cons only.
__global__ __launch_bounds__(WT_THREADS) void k_cand_scatter(WaitParams P, MoveCols M, CandCols C) { wait_scatter_body<false, true>(P, M, C); }

// The second selection of the mm_*_if calls (include/mm_wait.h): candidate i of n stays iff lo <= cnt[i] <= hi, cnt the
// partner count par_count_body left beside its record.  Count / scan / scatter again, over a LIST this time — a thread per
// candidate, a row per wave (k_sel_count), rows_scan_body down the rows with the total behind them (k_sel_scan), then every
// kept candidate goes to its rank in the call's final columns and is marked as k_cancel marks a slot (k_sel_scatter): a
// stable compaction, so the list is mm_expire's order restricted to the kept.  The candidates and the final columns are
// different buffers: a compaction in place would race across workgroups.
struct SelParams {
    uint32_t n, capacity;                     // candidates; slots of the pool
    uint32_t lo, hi;                          // min_partners, max_partners
    uint32_t now;
    const uint4* rec;                         // [n] as CandCols
    const uint32_t* age;
    const uint32_t* cnt;
    uint32_t* rows;                           // [ceil(n / 64)]; behind them the total
    uint8_t* state;
    uint32_t* out_slot;                       // the list, as WaitParams
    uint32_t* out_group;
    uint32_t* out_age;
};

static __device__ __forceinline__ uint32_t sel_rows_of(uint32_t n) { return (n + 63u) / 64u; }

__global__ __launch_bounds__(SEL_TILE) void k_sel_count(SelParams S)
{
    const uint32_t i = blockIdx.x * SEL_TILE + threadIdx.x;
    const uint32_t c = i < S.n ? S.cnt[i] : 0u;
    const unsigned long long m = __ballot(i < S.n && c >= S.lo && c <= S.hi);
    if ((threadIdx.x & 63) == 0 && i < S.n) S.rows[i >> 6] = (uint32_t)__popcll(m);
}

__global__ __launch_bounds__(WT_THREADS) void k_sel_scan(SelParams S) { rows_scan_body(S.rows, sel_rows_of(S.n), S.rows + sel_rows_of(S.n)); }

// ROWS (mm_move_if, mm_move_out_if): the rows of the enqueue go along, the constraint word rewritten here.
template <bool ROWS>
static __device__ __forceinline__ void sel_scatter_body(const SelParams& S, const MoveCols& M)
{
    const uint32_t i = blockIdx.x * SEL_TILE + threadIdx.x;
    const int lane = threadIdx.x & 63;
    const uint32_t c = i < S.n ? S.cnt[i] : 0u;
    const bool sel = i < S.n && c >= S.lo && c <= S.hi;
    const unsigned long long m = __ballot(sel);
    if (!sel) return;
    const uint32_t at = S.rows[i >> 6] + (uint32_t)__popcll(m & ((1ull << lane) - 1ull));
    const uint4 q = S.rec[i];
    if (at >= S.capacity || q.w >= S.capacity) return;
    const uint32_t age = S.age[i];
    S.out_slot[at] = q.w;
    S.out_group[at] = q.z;
    S.out_age[at] = age;
    if (ROWS) {
        M.rating[at] = (int32_t)q.x;
        M.cons[at] = (q.y & M.keep) | M.to_mode;
        M.group[at] = (uint8_t)q.z;
        M.stamp[at] = S.now - age;
    }
    S.state[q.w] = MM_ST_CANCELLED;
}

__global__ __launch_bounds__(SEL_TILE) void k_sel_scatter(SelParams S) { sel_scatter_body<false>(S, move_cols_none()); }
__global__ __launch_bounds__(SEL_TILE) void k_sel_scatter_rows(SelParams S, MoveCols M) { sel_scatter_body<true>(S, M); }

// mm_rotate (include/mm_wait.h): the LIVE seats of the stored lobbies of one mode leave and rejoin their own queue's
// tail.  No queue is streamed: a chain is selected by its LobbyDev record, state[] of its seats and ChainDev.len alone, so
// both kernels are ONE workgroup — a wave per rating group (groups wave, wave + WT_WAVES, ...), a lane per seat in
// wait_seat_at's order, at most MM_MAX_GROUPS x WT_SEATS gathers in all.
struct RotateParams {
    uint32_t mode, n_groups, capacity, teams;
    uint32_t max_seated, min_queue;
    const ChainDev* chains;
    const uint32_t* stamp;
    uint8_t* state;
    uint32_t* base;                           // [n_groups] rank of the group's first seat in the list (k_rotate_count)
    uint32_t* total;                          // the players selected
};

// Lane `lane`'s seat of chain (mode, g): is it LIVE, and is the chain selected — 1 <= LIVE seats <= max_seated and a queue
// of at least min_queue entries (ChainDev.len: entries cancelled and not yet purged count)?  `m`: the LIVE lanes.
// The same for every lane of a wave; every lane of the wave must call it (ballot).
static __device__ __forceinline__ bool rotate_chain(const RotateParams& P, uint32_t g, int lane, uint32_t& sl, uint32_t& t,
                                                    uint32_t& i, unsigned long long& m)
{
    const ChainDev& ch = P.chains[P.mode * P.n_groups + g];
    sl = MM_NO_SLOT; t = 0; i = 0;
    if ((uint32_t)lane < WT_SEATS && wait_seat_at(ch.lobby, P.teams, (uint32_t)lane, t, i)) sl = ch.lobby.slot[t][i];
    m = __ballot(sl < P.capacity && P.state[sl] == MM_ST_LIVE);
    const uint32_t c = (uint32_t)__popcll(m);
    return c >= 1u && c <= P.max_seated && ch.len >= P.min_queue;
}

__global__ __launch_bounds__(WT_THREADS) void k_rotate_count(RotateParams P)
{
    __shared__ uint32_t s_cnt[MM_MAX_GROUPS];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    for (uint32_t g = (uint32_t)wave; g < P.n_groups && g < MM_MAX_GROUPS; g += WT_WAVES) {
        uint32_t sl, t, i;
        unsigned long long m;
        const bool sel = rotate_chain(P, g, lane, sl, t, i, m);
        if (lane == 0) s_cnt[g] = sel ? (uint32_t)__popcll(m) : 0u;
    }
    __syncthreads();
    if (tid == 0) {                           // an exclusive scan over at most MM_MAX_GROUPS counts
        uint32_t run = 0;
        for (uint32_t g = 0; g < P.n_groups && g < MM_MAX_GROUPS; ++g) {
            P.base[g] = run;
            run += s_cnt[g];
        }
        *P.total = run;
    }
}

// The list columns (WaitParams' out_*: slot | rating group | age), the rows of the enqueue that follows (MoveCols: rating
// and constraint word as the LobbyDev record holds them, the group byte, stamp[slot] itself) and the marks of k_cancel.
// A slot sits in one lobby, once: the marks of one wave are read by no other, so every wave selects what k_rotate_count
// counted — and within a wave the ballot of rotate_chain has read state[] before the first mark is written.
__global__ __launch_bounds__(WT_THREADS) void k_rotate_scatter(RotateParams P, uint32_t now, uint32_t* __restrict__ out_slot,
                                                               uint32_t* __restrict__ out_group, uint32_t* __restrict__ out_age,
                                                               MoveCols M)
{
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const unsigned long long lt = (1ull << lane) - 1ull;
    for (uint32_t g = (uint32_t)wave; g < P.n_groups && g < MM_MAX_GROUPS; g += WT_WAVES) {
        uint32_t sl, t, i;
        unsigned long long m;
        if (!rotate_chain(P, g, lane, sl, t, i, m)) continue;
        const uint32_t at = P.base[g] + (uint32_t)__popcll(m & lt);
        if (((m >> lane) & 1ull) && at < P.capacity) {
            const LobbyDev& lb = P.chains[P.mode * P.n_groups + g].lobby;
            const uint32_t st = P.stamp[sl];
            out_slot[at] = sl;
            out_group[at] = g;
            out_age[at] = now - st;
            M.rating[at] = lb.rating[t][i];
            M.cons[at] = lb.cons[t][i];
            M.group[at] = (uint8_t)g;
            M.stamp[at] = st;
            P.state[sl] = MM_ST_CANCELLED;
        }
    }
}

// mm_wait_stats: one streaming pass over the same chunks.  Counts, sums and maxima in registers, reduced per wave; the
// histogram in LDS; a workgroup merges its chunk into the group's record with one atomic per non-empty field.
__global__ __launch_bounds__(WT_THREADS) void k_wait_stats(WaitParams P)
{
    __shared__ uint32_t s_hist[33];
    __shared__ uint32_t s_cnt, s_max;
    __shared__ unsigned long long s_sum;
    const int tid = threadIdx.x, lane = tid & 63, wave = wait_wave();
    for (uint32_t b = blockIdx.x;; b += gridDim.x) {
        WaitChunk c;
        if (!wait_chunk(P, b, c)) return;
        if (tid < 33) s_hist[tid] = 0;
        if (tid == 0) { s_cnt = 0; s_max = 0; s_sum = 0; }
        __syncthreads();
        const uint32_t w0 = c.first(wave);
        uint32_t cnt = 0, mx = 0;
        unsigned long long sum = 0;
        if (c.seats(wave)) {
            uint32_t age = 0;
            if (wait_age(P, wait_seat(P, c, lane).sl, age)) {
                cnt = 1; mx = age; sum = age;
                atomicAdd(&s_hist[wait_bucket(age)], 1u);
            }
        }
        if (w0 < c.len) {
            WaitRows R;
            const uint32_t live = wait_load<WL_AGE>(P, c, w0, lane, R);
#pragma unroll
            for (uint32_t r = 0; r < WT_ITERS; ++r)
                if ((live >> r) & 1u) {
                    ++cnt;
                    mx = R.age[r] > mx ? R.age[r] : mx;
                    sum += R.age[r];
                    atomicAdd(&s_hist[wait_bucket(R.age[r])], 1u);
                }
        }
        cnt = wait_wave_sum(cnt, lane);
        mx = wait_wave_max(mx, lane);
        sum = wait_wave_sum64(sum, lane);
        if (lane == 0 && cnt) {
            atomicAdd(&s_cnt, cnt);
            atomicMax(&s_max, mx);
            atomicAdd(&s_sum, sum);
        }
        __syncthreads();
        WaitGroupDev* const out = P.stats + c.g;
        if (tid < 33 && s_hist[tid]) atomicAdd(&out->hist[tid], s_hist[tid]);
        if (tid == 64 && s_cnt) {
            atomicAdd(&out->waiting, s_cnt);
            atomicMax(&out->oldest_age, s_max);
            atomicAdd(&out->age_sum, s_sum);
        }
        __syncthreads();
    }
}

// mm_locate (include/mm_wait.h): where a queried slot stands in `mode` — one more pass of the walk above, and read-only:
// nothing of the pool is written, only the call's own scratch.  k_loc_mark tags the queried slots (tag[slot] = query + 1;
// tag[capacity] is all zero between calls) and presets every query's row to MM_AT_NONE; k_loc_count counts the LIVE
// entries per wave into rows of k_wait_count's layout, which the unchanged k_wait_scan turns into ranks; k_loc_scatter
// streams the queues again, gathers state[slot] and tag[slot] per entry, and a tagged entry writes its query's row;
// k_loc_collect gives a duplicated slot's other queries the winner's row; k_loc_clear takes the tags off again.
// A slot sits in one queue or one lobby, once: every row has one writer.
struct LocParams {
    uint32_t n, stride;                       // queries; words between the columns of `out`
    uint32_t want_ahead;                      // 0: k_loc_count and k_wait_scan did not run, `ahead` is not asked for
    const uint32_t* q;                        // [n] the queried slots
    uint32_t* tag;                            // [capacity]
    uint32_t* out;                            // [5][stride]: where | group | position | ahead | age
};

#define LOC_NONE 0u                           // MM_AT_* of include/mm_wait.h
#define LOC_QUEUE 1u
#define LOC_LOBBY 2u
#define LOC_MARKED 4u

static __device__ __forceinline__ void loc_write(const LocParams& L, uint32_t i, uint32_t where, uint32_t group, uint32_t position,
                                                 uint32_t ahead, uint32_t age)
{
    if (i >= L.n) return;
    L.out[i] = where;
    L.out[(size_t)L.stride + i] = group;
    L.out[2u * (size_t)L.stride + i] = position;
    L.out[3u * (size_t)L.stride + i] = ahead;
    L.out[4u * (size_t)L.stride + i] = age;
}

__global__ __launch_bounds__(WT_THREADS) void k_loc_mark(LocParams L, uint32_t capacity)
{
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= L.n) return;
    loc_write(L, i, LOC_NONE, MM_NO_SLOT, MM_NO_SLOT, 0u, 0u);
    const uint32_t s = L.q[i];
    if (s < capacity) L.tag[s] = i + 1u;      // among duplicates any one winner will do (k_loc_collect)
}

// k_wait_count's body with the predicate "LIVE" and no age; the seats' row counts 0 (a seat has nobody ahead).
__global__ __launch_bounds__(WT_THREADS) void k_loc_count(WaitParams P) { wait_count_body<false, false>(P); }

__global__ __launch_bounds__(WT_THREADS) void k_loc_scatter(WaitParams P, LocParams L)
{
    const int tid = threadIdx.x, lane = tid & 63, wave = wait_wave();
    const unsigned long long lt = (1ull << lane) - 1ull;
    for (uint32_t b = blockIdx.x;; b += gridDim.x) {
        WaitChunk c;
        if (!wait_chunk(P, b, c)) return;
        const uint32_t w0 = c.first(wave);
        if (w0 < c.len) {
            // LIVE entries of this queue in front of the wave: its scanned rank less the rank of the group's first queue row
            uint32_t base = L.want_ahead ? c.row(P)[1 + wave] - c.group_row(P)[1] : 0u;
            WaitRows R;
            const uint32_t live = wait_load<WL_TAG>(P, c, w0, lane, R, nullptr, nullptr, L.tag);
#pragma unroll
            for (uint32_t r = 0; r < WT_ITERS; ++r) {
                const bool lv = (live >> r) & 1u;
                const uint32_t ahead = wait_rank(lv, lt, base);
                if (R.tg[r])
                    loc_write(L, R.tg[r] - 1u, LOC_QUEUE | (lv ? 0u : LOC_MARKED), c.g, w0 + r * 64 + (uint32_t)lane, ahead,
                              P.stamp ? P.now - P.stamp[R.sl[r]] : 0u);
            }
        }
        if (c.seats(wave)) {
            const uint32_t sl = wait_seat(P, c, lane).sl;
            const uint32_t tg = sl < P.capacity ? L.tag[sl] : 0u;
            if (tg)
                loc_write(L, tg - 1u, LOC_LOBBY | (P.state[sl] == MM_ST_LIVE ? 0u : LOC_MARKED), c.g, (uint32_t)lane, 0u,
                          P.stamp ? P.now - P.stamp[sl] : 0u);
        }
    }
}

// A query whose slot's tag names another query (the same slot, queried more than once) takes that query's row.  The winner's
// row was written by the launches before this one and nobody reads a loser's row: no race.
__global__ __launch_bounds__(WT_THREADS) void k_loc_collect(LocParams L, uint32_t capacity)
{
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= L.n) return;
    const uint32_t s = L.q[i];
    if (s >= capacity) return;
    const uint32_t t = L.tag[s];
    if (t == 0u || t - 1u == i || t - 1u >= L.n) return;
#pragma unroll
    for (uint32_t c = 0; c < 5u; ++c) L.out[c * (size_t)L.stride + i] = L.out[c * (size_t)L.stride + (t - 1u)];
}

// A launch of its own behind the collect (which reads the tags): tag[] is all zero again, found or not.
__global__ __launch_bounds__(WT_THREADS) void k_loc_clear(LocParams L, uint32_t capacity)
{
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= L.n) return;
    const uint32_t s = L.q[i];
    if (s < capacity) L.tag[s] = 0u;
}

// mm_partners (include/mm_wait.h): how many waiting players of chain (in_mode, g) fit a queried player at a window and a
// set of filters the caller names — step 2 of match_check (docs/MATCH_CHECK.md) with the queried player in the anchor's
// place — and how far away the nearest one is.  Read-only, like mm_locate, whose passes (k_loc_mark / k_loc_scatter /
// k_loc_collect / k_loc_clear, launched as they are, `ahead` off) find every query's chain and position first.
// k_par_gather, one thread per query, then builds the query's record — rating | constraint word | rating group | slot, from
// q_rating / q_cons at the position or from the LobbyDev seat; group MM_NO_SLOT for a slot that is not in the mode — and
// presets its result words.  k_par_count* stream in_mode's queues in the walk's chunks: a wave keeps its WT_PER_WAVE entries
// (slot, rating, constraint word, LIVE mask) in registers, the workgroup stages the queries of its chunk's rating group out
// of a tile of PAR_QTILE records into LDS and every wave loops over them — the query is wave-uniform, its fields are
// broadcast LDS reads — counting with ballot + popcount into the query's LDS words; a tile's non-zero words are merged
// into the global result with one atomic each.  Integer adds and minima commute: the result is exact in any order.
// The queried player itself is excluded by SLOT, inside the test (a slot sits in one queue or one lobby, once): with
// in_mode == mode it would fit itself at distance 0, and a minimum cannot be corrected afterwards.
#if !defined(PAR_QTILE)
#error "mm_wait.inc: define PAR_QTILE beside the WT_* chunk geometry before including this file (mm_engine.hip does)"
#endif

struct ParParams {
    uint32_t n, stride;                       // queries; queries `rec` and the columns of `out` have room for
    uint32_t gx;                              // workgroups striding over the chunks; gridDim.x / gx of them over the query tiles
    uint32_t window, eqmask;                  // the predicate: |rating difference| <= window, (cons ^ cons) & eqmask == 0
    uint32_t loc_stride;
    const uint32_t* q;                        // [n] the queried slots (mm_locate's scratch)
    const uint32_t* loc;                      // [5][loc_stride] mm_locate's rows: where | group | position | .. | ..
    const int32_t* q_rating;
    const uint32_t* q_cons;
    uint4* rec;                               // [n] x rating | y constraint word | z rating group (MM_NO_SLOT: none) | w slot
    uint32_t* out;                            // partners[stride] | gap[stride] | by_role[stride][MM_MAX_ROLES]
};

// P: the walk's parameters for the mode the queries are looked up in.
__global__ __launch_bounds__(WT_THREADS) void k_par_gather(WaitParams P, ParParams Q)
{
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= Q.n) return;
    const uint32_t where = Q.loc[i] & (LOC_QUEUE | LOC_LOBBY);
    const uint32_t g = Q.loc[(size_t)Q.loc_stride + i], pos = Q.loc[2u * (size_t)Q.loc_stride + i];
    uint4 r;
    r.x = 0u; r.y = 0u; r.z = MM_NO_SLOT; r.w = Q.q[i];
    if (g < P.n_groups) {
        if (where == LOC_QUEUE && pos < P.capacity) {
            const size_t at = (size_t)(P.mode * P.n_groups + g) * P.capacity + pos;
            r.x = (uint32_t)Q.q_rating[at];
            r.y = Q.q_cons[at];
            r.z = g;
        } else if (where == LOC_LOBBY) {
            const LobbyDev& lb = P.chains[P.mode * P.n_groups + g].lobby;
            uint32_t t = 0, s = 0;
            if (wait_seat_at(lb, P.teams, pos, t, s)) {
                r.x = (uint32_t)lb.rating[t][s];
                r.y = lb.cons[t][s];
                r.z = g;
            }
        }
    }
    Q.rec[i] = r;
    Q.out[i] = 0u;
    Q.out[(size_t)Q.stride + i] = MM_NO_SLOT;
#pragma unroll
    for (uint32_t k = 0; k < MM_MAX_ROLES; ++k) Q.out[2u * (size_t)Q.stride + (size_t)i * MM_MAX_ROLES + k] = 0u;
}

// One register row of candidates against one query: sl, rt, cn this lane's candidate's slot, rating and constraint word.
// A candidate that does not wait (not LIVE, or past the queue's end) carries PAR_DEAD in its constraint word, a bit no
// constraint word has (MM_CONS_USER_MASK) and no staged query carries: the filter test of the predicate rejects it, so
// liveness costs no instruction and no lane mask per row.  The difference of two int32 ratings as an ordered unsigned
// subtraction: exact up to 2^32 - 1.  Every lane of the wave must call it (ballot).
#define PAR_DEAD 0x80000000u
template <bool ROLES, bool GAP>
static __device__ __forceinline__ void par_row(const ParParams& Q, const uint4& q, uint32_t sl, int32_t rt, uint32_t cn,
                                               uint32_t& cnt, uint32_t& dmin, uint32_t* __restrict__ role_row)
{
    const bool ok = sl != q.w && ((cn ^ q.y) & (Q.eqmask | PAR_DEAD)) == 0u;
    const int32_t qr = (int32_t)q.x;
    const uint32_t d = rt >= qr ? (uint32_t)rt - (uint32_t)qr : (uint32_t)qr - (uint32_t)rt;
    const bool fit = ok && d <= Q.window;
    cnt += (uint32_t)__popcll(__ballot(fit));
    if (ROLES && fit) {
        atomicAdd(&role_row[(cn >> 16) & (MM_MAX_ROLES - 1u)], 1u);   // MM_CONS_ROLE: below n_roles <= MM_MAX_ROLES by mm_enqueue's rule
    }
    if (GAP && ok) dmin = dev_min_u32(dmin, dev_min_u32(d, 0xFFFFFFFEu));
}

// P: the walk's parameters for in_mode.  Workgroup blockIdx.x % gx strides over the chunks, blockIdx.x / gx over the tiles.
template <bool ROLES, bool GAP>
static __device__ __forceinline__ void par_count_body(const WaitParams& P, const ParParams& Q)
{
    __shared__ uint4 s_rec[PAR_QTILE];                    // the kept queries: x rating | y constraint word | z query | w slot
    __shared__ uint32_t s_cnt[PAR_QTILE];
    __shared__ uint32_t s_gap[GAP ? PAR_QTILE : 1];
    __shared__ uint32_t s_role[ROLES ? PAR_QTILE * MM_MAX_ROLES : 1];
    __shared__ uint32_t s_nk;
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = wait_wave();
    const uint32_t gx = Q.gx ? Q.gx : 1u, bx = blockIdx.x % gx, by = blockIdx.x / gx, gy = gridDim.x / gx;
    const uint32_t n_tiles = (Q.n + PAR_QTILE - 1u) / PAR_QTILE;
    if (by >= gy) return;
    for (uint32_t b = bx;; b += gx) {
        WaitChunk c;
        if (!wait_chunk(P, b, c)) return;
        const uint32_t w0 = c.first(wave), g = c.g;
        const bool rows = w0 < c.len, seats = c.seats(wave);
        // The load and the seats in lines of this body's own, not wait_load<WL_ROW> and wait_seat: through them k_par_count_gap
        // measured 0.2 to 0.3 % above the parent in every set, at a spread of 0.04 % (profiles/wait_walk_refactor_check.txt).
        const size_t qo = c.qo(P);
        uint32_t sl[WT_ITERS], cn[WT_ITERS];
        int32_t rt[WT_ITERS];
        uint32_t s_sl = MM_NO_SLOT, s_cn = PAR_DEAD;
        int32_t s_rt = 0;
        if (rows) {                                       // the three streamed columns, then the gather of state[]
#pragma unroll
            for (uint32_t r = 0; r < WT_ITERS; ++r) {
                const uint32_t i = w0 + r * 64 + lane;
                const bool in = i < c.len;
                sl[r] = in ? P.q_slot[qo + i] : MM_NO_SLOT;
                rt[r] = in ? Q.q_rating[qo + i] : 0;
                cn[r] = in ? Q.q_cons[qo + i] : 0u;
            }
            uint8_t st[WT_ITERS];
#pragma unroll
            for (uint32_t r = 0; r < WT_ITERS; ++r) st[r] = sl[r] < P.capacity ? P.state[sl[r]] : (uint8_t)MM_ST_FREE;
#pragma unroll
            for (uint32_t r = 0; r < WT_ITERS; ++r) cn[r] = st[r] == MM_ST_LIVE ? cn[r] & ~PAR_DEAD : PAR_DEAD;
        }
        if (seats) {                                      // the stored lobby's seats (at most WT_SEATS: a lane past the last finds none)
            const LobbyDev& lb = c.lobby(P);
            uint32_t t = 0, i = 0;
            if (wait_seat_at(lb, P.teams, (uint32_t)lane, t, i)) {
                s_sl = lb.slot[t][i];
                s_rt = lb.rating[t][i];
                s_cn = wait_live(P, s_sl) ? lb.cons[t][i] & ~PAR_DEAD : PAR_DEAD;
            }
        }
        for (uint32_t tile = by; tile < n_tiles; tile += gy) {
            if (tid == 0) s_nk = 0u;
            __syncthreads();
            for (uint32_t x = (uint32_t)tid; x < PAR_QTILE; x += WT_THREADS) {
                const uint32_t qi = tile * PAR_QTILE + x;
                if (qi >= Q.n) continue;
                uint4 q = Q.rec[qi];
                if (q.z != g) continue;
                const uint32_t j = atomicAdd(&s_nk, 1u);  // (j < PAR_QTILE: at most one per record of the tile)
                q.y &= ~PAR_DEAD;
                q.z = qi;
                s_rec[j] = q;
                s_cnt[j] = 0u;
                if (GAP) s_gap[j] = MM_NO_SLOT;
                if (ROLES) {
#pragma unroll
                    for (uint32_t r = 0; r < MM_MAX_ROLES; ++r) s_role[j * MM_MAX_ROLES + r] = 0u;
                }
            }
            __syncthreads();
            const uint32_t nk = dev_min_u32(s_nk, PAR_QTILE);
            if (rows) {
#pragma unroll 1
                for (uint32_t j = 0; j < nk; ++j) {
                    const uint4 q = s_rec[j];
                    uint32_t* const role_row = ROLES ? &s_role[j * MM_MAX_ROLES] : s_role;
                    uint32_t cnt = 0u, dmin = MM_NO_SLOT;
#pragma unroll
                    for (uint32_t r = 0; r < WT_ITERS; ++r) par_row<ROLES, GAP>(Q, q, sl[r], rt[r], cn[r], cnt, dmin, role_row);
                    if (lane == 0 && cnt) atomicAdd(&s_cnt[j], cnt);
                    if (GAP && dmin != MM_NO_SLOT && dmin < s_gap[j]) atomicMin(&s_gap[j], dmin);
                }
            }
            if (seats) {                                  // one more row, of wave 0 of the group's first chunk alone
#pragma unroll 1
                for (uint32_t j = 0; j < nk; ++j) {
                    const uint4 q = s_rec[j];
                    uint32_t cnt = 0u, dmin = MM_NO_SLOT;
                    par_row<ROLES, GAP>(Q, q, s_sl, s_rt, s_cn, cnt, dmin, ROLES ? &s_role[j * MM_MAX_ROLES] : s_role);
                    if (lane == 0 && cnt) atomicAdd(&s_cnt[j], cnt);
                    if (GAP && dmin != MM_NO_SLOT && dmin < s_gap[j]) atomicMin(&s_gap[j], dmin);
                }
            }
            __syncthreads();
            for (uint32_t j = (uint32_t)tid; j < nk; j += WT_THREADS) {
                const uint32_t qi = s_rec[j].z;
                if (s_cnt[j]) atomicAdd(&Q.out[qi], s_cnt[j]);
                if (GAP && s_gap[j] != MM_NO_SLOT) atomicMin(&Q.out[(size_t)Q.stride + qi], s_gap[j]);
            }
            if (ROLES) {
                for (uint32_t x = (uint32_t)tid; x < nk * MM_MAX_ROLES; x += WT_THREADS) {
                    const uint32_t v = s_role[x];
                    if (v) atomicAdd(&Q.out[2u * (size_t)Q.stride + (size_t)s_rec[x / MM_MAX_ROLES].z * MM_MAX_ROLES + x % MM_MAX_ROLES], v);
                }
            }
            // (the next tile's first barrier stands between these reads and its staging writes)
        }
        __syncthreads();                                  // ... and this one before the next chunk's
    }
}

// partners only | + by_role | + gap | all three: a column nobody asked for costs nothing
__global__ __launch_bounds__(WT_THREADS) void k_par_count(WaitParams P, ParParams Q) { par_count_body<false, false>(P, Q); }
__global__ __launch_bounds__(WT_THREADS) void k_par_count_role(WaitParams P, ParParams Q) { par_count_body<true, false>(P, Q); }
__global__ __launch_bounds__(WT_THREADS) void k_par_count_gap(WaitParams P, ParParams Q) { par_count_body<false, true>(P, Q); }
__global__ __launch_bounds__(WT_THREADS) void k_par_count_all(WaitParams P, ParParams Q) { par_count_body<true, true>(P, Q); }

// mm_partner_stats (include/mm_wait.h): mm_partners' two words for EVERY waiting player of a mode, aggregated per rating
// group — from a sorted table of in_mode's waiting players instead of queries x group length predicate tests.  Read-only.
//   k_fit_count    in_mode's walk, wait_count_body: the LIVE entries per wave, and the LIVE seats in the seats' row; the
//                  unchanged k_wait_scan turns the rows into ranks with the total — the table's length — behind them;
//   k_fit_keys     the same walk: one 64-bit key per waiting candidate at its rank (a stable compaction: the table's first
//                  order is the walk's) — rating group << 48 | the constraint-word fields the filters compare << 32 (region
//                  in bits 32..39, party in 40..43, zero where a filter is off) | rating ^ 2^31, unsigned order;
//   k_fit_hist / k_fit_scan / k_fit_scatter   one LSD radix pass over one byte of the key, FIT_TILE keys a workgroup: the
//                  tile's digit histogram into hist[digit][tile], an exclusive scan along every digit's row (a wave a
//                  digit) with the 256 totals behind the table, then every key to the start of its digit (the scan of the
//                  totals, done by every scatter workgroup for itself) + hist[digit][tile] + its rank among the tile's
//                  keys of that digit.  The rank is stable: a tile is cut
//                  into waves and rows in index order, a key's rank is the count of its digit in the rows before it (an
//                  LDS counter per wave and digit, the waves before it added afterwards) plus the lanes below it in its own
//                  row (eight ballots give the lanes of the same digit).  Three launches a pass, no workgroup waits for
//                  another; the host leaves out the passes whose byte is zero in every key;
//   k_fit_search   mode's walk: per waiting player two binary searches for rating -+ window (in 64 bits, clamped to int32)
//                  with the player's own group and filter fields in front — keys of another segment compare below or
//                  above the pair, so the searches need no segment bounds — and two more inside that range for the run
//                  of equal ratings; the run, or else the table's neighbours of the same segment, give the gap.  With
//                  in_mode == mode the player itself is in the table exactly once: 1 comes off both counts.  Then
//                  k_wait_stats' aggregation: registers, wave, LDS, one global atomic per touched word of the record.
#if !defined(FIT_TILE)
#error "mm_wait.inc: define FIT_TILE beside the WT_* chunk geometry before including this file (mm_engine.hip does)"
#endif
#define FIT_PER_WAVE (FIT_TILE / WT_WAVES)
#define FIT_ITERS (FIT_PER_WAVE / 64)
#define FIT_DIGITS 256u

struct FitGroupDev {                          // mm_partner_group (include/mm_wait.h) with types atomicAdd takes
    uint32_t waiting, candidates, alone, unreachable;
    unsigned long long partners_sum, gap_sum;
    uint32_t partners_max, gap_max;
    uint32_t partners_hist[33];
    uint32_t gap_hist[33];
};

struct FitParams {
    uint32_t window, eqmask;                  // mm_partners' predicate
    uint32_t self;                            // 1: in_mode == mode, every query is in the table once
    uint32_t key_cap;                         // keys each half of `keys` has room for
    uint32_t shift;                           // the pass's byte of the key
    const int32_t* q_rating;
    const uint32_t* q_cons;
    const uint32_t* n_keys;                   // the table's length: the total behind the rows of k_fit_count
    const unsigned long long* keys;           // what a pass reads; the sorted table for k_fit_search
    unsigned long long* keys_out;             // what k_fit_keys and a pass write
    uint32_t* hist;                           // [FIT_DIGITS][tiles]; the digits' totals from [FIT_DIGITS * tiles of key_cap] on
    FitGroupDev* stats;                       // [n_groups], zeroed by the host
};

static __device__ __forceinline__ uint32_t fit_tiles(uint32_t n) { return (n + FIT_TILE - 1u) / FIT_TILE; }

static __device__ __forceinline__ unsigned long long fit_prefix(uint32_t g, uint32_t cons, uint32_t eqmask)
{
    return ((unsigned long long)g << 48) | ((unsigned long long)((cons & eqmask) >> 4) << 32);
}

static __device__ __forceinline__ uint32_t fit_bias(int32_t rating) { return (uint32_t)rating ^ 0x80000000u; }

__global__ __launch_bounds__(WT_THREADS) void k_fit_count(WaitParams P) { wait_count_body<false, true>(P); }

// P: the walk's parameters for in_mode, the rows scanned.
__global__ __launch_bounds__(WT_THREADS) void k_fit_keys(WaitParams P, FitParams F)
{
    const int tid = threadIdx.x, lane = tid & 63, wave = wait_wave();
    const unsigned long long lt = (1ull << lane) - 1ull;
    for (uint32_t b = blockIdx.x;; b += gridDim.x) {
        WaitChunk c;
        if (!wait_chunk(P, b, c)) return;
        const uint32_t w0 = c.first(wave), base0 = c.row(P)[1 + wave];
        uint32_t base = base0, mine = 0u;
        if (w0 < c.len) {
            // (the load in its own lines, not wait_load<WL_ROW>: through the loader's LIVE mask this kernel measured 11 to 13 % slower,
            // 42 VGPRs for 34 — profiles/wait_walk_refactor_check.txt)
            const size_t qo = c.qo(P);
            uint32_t sl[WT_ITERS], cn[WT_ITERS];
            int32_t rt[WT_ITERS];
#pragma unroll
            for (uint32_t r = 0; r < WT_ITERS; ++r) {
                const uint32_t i = w0 + r * 64 + lane;
                const bool in = i < c.len;
                sl[r] = in ? P.q_slot[qo + i] : MM_NO_SLOT;
                rt[r] = in ? F.q_rating[qo + i] : 0;
                cn[r] = in ? F.q_cons[qo + i] : 0u;
            }
            uint8_t st[WT_ITERS];
#pragma unroll
            for (uint32_t r = 0; r < WT_ITERS; ++r) st[r] = sl[r] < P.capacity ? P.state[sl[r]] : (uint8_t)MM_ST_FREE;
#pragma unroll
            for (uint32_t r = 0; r < WT_ITERS; ++r) {
                const bool lv = st[r] == MM_ST_LIVE;
                const uint32_t at = wait_rank(lv, lt, base);
                if (lv && at < F.key_cap) F.keys_out[at] = fit_prefix(c.g, cn[r], F.eqmask) | fit_bias(rt[r]);
            }
            mine = base - base0;
        }
        if (wave == 0) {
            const WaitSeat s = wait_seat(P, c, lane);
            const uint32_t seat0 = c.row(P)[0];
            uint32_t seat_base = seat0;
            const bool lv = wait_live(P, s.sl);
            const uint32_t at = wait_rank(lv, lt, seat_base);
            if (lv && at < F.key_cap) F.keys_out[at] = fit_prefix(c.g, s.cn, F.eqmask) | fit_bias(s.rt);
            mine += seat_base - seat0;
        }
        if (lane == 0 && mine) atomicAdd(&F.stats[c.g].candidates, mine);
    }
}

__global__ __launch_bounds__(WT_THREADS) void k_fit_hist(FitParams F)
{
    __shared__ uint32_t s_h[FIT_DIGITS];
    const uint32_t tid = threadIdx.x;
    const uint32_t n = dev_min_u32(*F.n_keys, F.key_cap), tiles = fit_tiles(n);
    for (uint32_t t = blockIdx.x; t < tiles; t += gridDim.x) {
        for (uint32_t d = tid; d < FIT_DIGITS; d += WT_THREADS) s_h[d] = 0u;
        __syncthreads();
#pragma unroll
        for (uint32_t r = 0; r < FIT_TILE / WT_THREADS; ++r) {
            const uint32_t i = t * FIT_TILE + r * WT_THREADS + tid;
            if (i < n) atomicAdd(&s_h[(uint32_t)(F.keys[i] >> F.shift) & (FIT_DIGITS - 1u)], 1u);
        }
        __syncthreads();
        for (uint32_t d = tid; d < FIT_DIGITS; d += WT_THREADS) F.hist[(size_t)d * tiles + t] = s_h[d];
        __syncthreads();
    }
}

// A wave per digit: the exclusive scan along hist[digit][0 .. tiles) in place — the keys of the digit in the tiles in front —
// 64 tiles a step, and the digit's total behind the table.  FIT_DIGITS / WT_WAVES workgroups, no wave looks at another's
// row and there is no barrier; the scan ACROSS the digits, 256 totals, is done by every workgroup of k_fit_scatter for itself.
__global__ __launch_bounds__(WT_THREADS) void k_fit_scan(FitParams F)
{
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const uint32_t tiles = fit_tiles(dev_min_u32(*F.n_keys, F.key_cap)), d = blockIdx.x * WT_WAVES + (uint32_t)wave;
    if (d >= FIT_DIGITS) return;
    uint32_t* const row = F.hist + (size_t)d * tiles;
    uint32_t run = 0u;
    for (uint32_t base = 0; base < tiles; base += 64u) {
        const uint32_t i = base + (uint32_t)lane, v = i < tiles ? row[i] : 0u, incl = wave_incl_scan(v, lane);
        if (i < tiles) row[i] = run + incl - v;
        run += (uint32_t)__shfl((int)incl, 63);
    }
    if (lane == 0) F.hist[(size_t)FIT_DIGITS * fit_tiles(F.key_cap) + d] = run;
}

__global__ __launch_bounds__(WT_THREADS) void k_fit_scatter(FitParams F)
{
    __shared__ uint32_t s_cnt[WT_WAVES][FIT_DIGITS];      // keys of a digit per wave; then where the wave's first one goes
    __shared__ uint32_t s_dig[FIT_DIGITS], s_wtot[WT_WAVES];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const unsigned long long lt = (1ull << lane) - 1ull;
    const uint32_t n = dev_min_u32(*F.n_keys, F.key_cap), tiles = fit_tiles(n);
    {   // where a digit's keys start in the output: the exclusive scan of k_fit_scan's 256 totals, a thread per digit
        static_assert(WT_THREADS == FIT_DIGITS, "a thread per digit");
        const uint32_t v = F.hist[(size_t)FIT_DIGITS * fit_tiles(F.key_cap) + (uint32_t)tid], incl = wave_incl_scan(v, lane);
        if (lane == 63) s_wtot[wave] = incl;
        __syncthreads();
        uint32_t run = incl - v;
        for (int w = 0; w < wave; ++w) run += s_wtot[w];
        s_dig[tid] = run;
        __syncthreads();
    }
    for (uint32_t t = blockIdx.x; t < tiles; t += gridDim.x) {
        for (uint32_t d = (uint32_t)tid; d < WT_WAVES * FIT_DIGITS; d += WT_THREADS) s_cnt[d / FIT_DIGITS][d % FIT_DIGITS] = 0u;
        __syncthreads();
        const uint32_t w0 = t * FIT_TILE + (uint32_t)wave * FIT_PER_WAVE;
        unsigned long long key[FIT_ITERS];
        uint32_t rank[FIT_ITERS];
#pragma unroll
        for (uint32_t r = 0; r < FIT_ITERS; ++r) {
            const uint32_t i = w0 + r * 64 + lane;
            key[r] = i < n ? F.keys[i] : ~0ull;
        }
#pragma unroll
        for (uint32_t r = 0; r < FIT_ITERS; ++r) {
            const bool in = w0 + r * 64 + lane < n;
            const uint32_t d = (uint32_t)(key[r] >> F.shift) & (FIT_DIGITS - 1u);
            unsigned long long same = __ballot(in);       // the lanes of this row that hold my digit
#pragma unroll
            for (uint32_t bit = 0; bit < 8u; ++bit) {
                const bool one = (d >> bit) & 1u;
                const unsigned long long m = __ballot(one);
                same &= one ? m : ~m;
            }
            // the lowest lane of a digit counts for all of them; what the counter held before is the rows in front
            const int lead = in ? __popcll((same & (0ull - same)) - 1ull) : lane;
            uint32_t before = 0u;
            if (in && lane == lead) {                     // (no atomic: the counter is this wave's alone, and one lane per digit of the row is here)
                before = s_cnt[wave][d];
                s_cnt[wave][d] = before + (uint32_t)__popcll(same);
            }
            before = (uint32_t)__shfl((int)before, lead);
            rank[r] = before + (uint32_t)__popcll(same & lt);
        }
        __syncthreads();
        for (uint32_t d = (uint32_t)tid; d < FIT_DIGITS; d += WT_THREADS) {
            uint32_t run = s_dig[d] + F.hist[(size_t)d * tiles + t];
            for (uint32_t w = 0; w < WT_WAVES; ++w) {
                const uint32_t c = s_cnt[w][d];
                s_cnt[w][d] = run;
                run += c;
            }
        }
        __syncthreads();
#pragma unroll
        for (uint32_t r = 0; r < FIT_ITERS; ++r) {
            if (w0 + r * 64 + lane >= n) continue;
            const uint32_t at = s_cnt[wave][(uint32_t)(key[r] >> F.shift) & (FIT_DIGITS - 1u)] + rank[r];
            if (at < F.key_cap) F.keys_out[at] = key[r];
        }
        __syncthreads();
    }
}

// The first index in [lo, hi) whose key is not below k (OVER: is above k); hi when there is none.
template <bool OVER>
static __device__ __forceinline__ uint32_t fit_bound(const unsigned long long* __restrict__ keys, uint32_t lo, uint32_t hi, unsigned long long k)
{
    while (lo < hi) {
        const uint32_t mid = lo + (hi - lo) / 2u;
        const unsigned long long v = keys[mid];
        if (OVER ? v <= k : v < k) lo = mid + 1u;
        else hi = mid;
    }
    return lo;
}

// mm_partners' `partners` and `gap` of one waiting player of rating group g, from the sorted table of n keys.
static __device__ __forceinline__ void fit_one(const FitParams& F, uint32_t n, uint32_t g, int32_t rating, uint32_t cons,
                                               uint32_t& partners, uint32_t& gap)
{
    const unsigned long long pre = fit_prefix(g, cons, F.eqmask);
    long long lo = (long long)rating - (long long)F.window, hi = (long long)rating + (long long)F.window;
    if (lo < -2147483648ll) lo = -2147483648ll;
    if (hi > 2147483647ll) hi = 2147483647ll;
    const uint32_t mine = fit_bias(rating);
    const uint32_t a = fit_bound<false>(F.keys, 0u, n, pre | fit_bias((int32_t)lo));
    const uint32_t b = fit_bound<true>(F.keys, a, n, pre | fit_bias((int32_t)hi));
    partners = b - a - F.self;
    const uint32_t e = fit_bound<false>(F.keys, a, b, pre | mine);
    const uint32_t f = fit_bound<true>(F.keys, e, b, pre | mine);
    gap = MM_NO_SLOT;
    if (f - e > F.self) { gap = 0u; return; }
    if (e > 0u) {
        const unsigned long long v = F.keys[e - 1u];
        if ((v >> 32) == (pre >> 32)) gap = dev_min_u32(mine - (uint32_t)v, 0xFFFFFFFEu);
    }
    if (f < n) {
        const unsigned long long v = F.keys[f];
        if ((v >> 32) == (pre >> 32)) gap = dev_min_u32(gap, dev_min_u32((uint32_t)v - mine, 0xFFFFFFFEu));
    }
}

// P: the walk's parameters for `mode`; F.keys the sorted table.
__global__ __launch_bounds__(WT_THREADS) void k_fit_search(WaitParams P, FitParams F)
{
    __shared__ uint32_t s_ph[33], s_gh[33];
    __shared__ uint32_t s_cnt, s_alone, s_unr, s_pmax, s_gmax;
    __shared__ unsigned long long s_psum, s_gsum;
    const int tid = threadIdx.x, lane = tid & 63, wave = wait_wave();
    const uint32_t n = dev_min_u32(*F.n_keys, F.key_cap);
    for (uint32_t b = blockIdx.x;; b += gridDim.x) {
        WaitChunk c;
        if (!wait_chunk(P, b, c)) return;
        if (tid < 33) { s_ph[tid] = 0; s_gh[tid] = 0; }
        if (tid == 0) { s_cnt = 0; s_alone = 0; s_unr = 0; s_pmax = 0; s_gmax = 0; s_psum = 0; s_gsum = 0; }
        __syncthreads();
        const uint32_t w0 = c.first(wave);
        uint32_t cnt = 0, alone = 0, unr = 0, pmax = 0, gmax = 0;
        unsigned long long psum = 0, gsum = 0;
        WaitRows R;                                       // the wave's queue rows; in row WT_ITERS the seat (wave 0 of the group's first chunk)
        uint32_t live = 0;
        if (w0 < c.len) live = wait_load<WL_ROW>(P, c, w0, lane, R, F.q_rating, F.q_cons);
        if (c.seats(wave)) {
            const WaitSeat s = wait_seat(P, c, lane);
            R.sl[WT_ITERS] = s.sl; R.rt[WT_ITERS] = s.rt; R.cn[WT_ITERS] = s.cn;
            if (wait_live(P, s.sl)) live |= 1u << WT_ITERS;
        }
#pragma unroll
        for (uint32_t r = 0; r <= WT_ITERS; ++r)
            if ((live >> r) & 1u) {
                uint32_t partners, gap;
                fit_one(F, n, c.g, R.rt[r], R.cn[r], partners, gap);
                ++cnt;
                psum += partners;
                pmax = partners > pmax ? partners : pmax;
                alone += partners == 0u;
                atomicAdd(&s_ph[wait_bucket(partners)], 1u);
                if (gap == MM_NO_SLOT) ++unr;
                else {
                    gsum += gap;
                    gmax = gap > gmax ? gap : gmax;
                    atomicAdd(&s_gh[wait_bucket(gap)], 1u);
                }
            }
        cnt = wait_wave_sum(cnt, lane);
        alone = wait_wave_sum(alone, lane);
        unr = wait_wave_sum(unr, lane);
        pmax = wait_wave_max(pmax, lane);
        gmax = wait_wave_max(gmax, lane);
        psum = wait_wave_sum64(psum, lane);
        gsum = wait_wave_sum64(gsum, lane);
        if (lane == 0 && cnt) {
            atomicAdd(&s_cnt, cnt);
            atomicAdd(&s_alone, alone);
            atomicAdd(&s_unr, unr);
            atomicMax(&s_pmax, pmax);
            atomicMax(&s_gmax, gmax);
            atomicAdd(&s_psum, psum);
            atomicAdd(&s_gsum, gsum);
        }
        __syncthreads();
        FitGroupDev* const out = F.stats + c.g;
        if (tid < 33 && s_ph[tid]) atomicAdd(&out->partners_hist[tid], s_ph[tid]);
        if (tid >= 64 && tid < 64 + 33 && s_gh[tid - 64]) atomicAdd(&out->gap_hist[tid - 64], s_gh[tid - 64]);
        if (tid == 128 && s_cnt) {
            atomicAdd(&out->waiting, s_cnt);
            if (s_alone) atomicAdd(&out->alone, s_alone);
            if (s_unr) atomicAdd(&out->unreachable, s_unr);
            if (s_psum) atomicAdd(&out->partners_sum, s_psum);
            if (s_gsum) atomicAdd(&out->gap_sum, s_gsum);
            if (s_pmax) atomicMax(&out->partners_max, s_pmax);
            if (s_gmax) atomicMax(&out->gap_max, s_gmax);
        }
        __syncthreads();
    }
}

// The sorted route of mm_partners and the rule calls (include/mm_wait.h, mm_tuning.wait_sort_mtests): the two words of
// fit_one PER QUERY RECORD — the n records k_par_gather / k_cand_scatter write — from the same sorted table of in_mode's
// waiting players, in place of queries x group length predicate tests.  Two things differ from k_fit_search.
//   self is per query, not per call: a query sits in the table exactly once iff in_mode == mode, the lookup found it
//   (rec.z != MM_NO_SLOT) and it is LIVE — mm_partners answers MARKED queries too, and those are no candidates.  The LIVE
//   bit is the lookup's `where` word (LOC_MARKED); the candidates of a rule call are all LIVE and pass no such column.
//   The search is not 4 x log2(n) dependent global loads: a workgroup stages up to FITQ_SAMPLE evenly spaced keys of the
//   table in LDS (fitq_stage), every bound is narrowed there to the stretch between two neighbouring samples and finished
//   with the log2(n / FITQ_SAMPLE) global steps that remain; a table no longer than the sample is searched in LDS alone.
//   The four bounds of a query are searched independently of each other (lo <= mine <= hi orders them anyway): four chains
//   of loads in flight, not one.
// A record with rec.z == MM_NO_SLOT keeps the preset of k_par_gather (0, the zero row, MM_NO_SLOT).
#if !defined(FITQ_SAMPLE)
#error "mm_wait.inc: define FITQ_SAMPLE beside FIT_TILE before including this file (mm_engine.hip does)"
#endif

struct FitQParams {
    uint32_t n, stride;                       // query records; queries the columns of `out` have room for
    uint32_t same_mode;                       // 1: in_mode == mode, a LIVE query that was found is in the table once
    uint32_t want_gap;                        // 0: the gap column is not written (a rule call keeps the ages there)
    uint32_t n_roles;                         // k_fit_query_role: the roles in_mode seats
    const uint32_t* where;                    // [n] the lookup's `where` words; NULL: every query is LIVE (the rule calls)
    const uint4* rec;                         // [n] as ParParams
    uint32_t* out;                            // partners[stride] | gap[stride] | by_role[stride][MM_MAX_ROLES]
};

// The staged sample: key j * step of the n keys for j < m; step 1 and m == n while the table fits the sample.
struct FitSample {
    uint32_t n, step, m;
};

// Every thread of the workgroup must call it (barrier).
static __device__ __forceinline__ FitSample fitq_stage(const FitParams& F, unsigned long long* __restrict__ s_key)
{
    FitSample S;
    S.n = dev_min_u32(*F.n_keys, F.key_cap);
    S.step = S.n > FITQ_SAMPLE ? (S.n + FITQ_SAMPLE - 1u) / FITQ_SAMPLE : 1u;
    S.m = (S.n + S.step - 1u) / S.step;                   // <= FITQ_SAMPLE, and (m - 1) * step < n
    for (uint32_t j = threadIdx.x; j < S.m; j += WT_THREADS) s_key[j] = F.keys[(size_t)j * S.step];
    __syncthreads();
    return S;
}

// fit_bound over the whole table: the first sample not below k (OVER: above k) is sample j — the bound lies behind
// sample j - 1 and not behind sample j (behind the last sample: not behind the table's end).
template <bool OVER>
static __device__ __forceinline__ uint32_t fitq_bound(const FitParams& F, const FitSample& S, const unsigned long long* __restrict__ s_key,
                                                      unsigned long long k)
{
    uint32_t lo = 0u, hi = S.m;
    while (lo < hi) {
        const uint32_t mid = lo + (hi - lo) / 2u;
        const unsigned long long v = s_key[mid];
        if (OVER ? v <= k : v < k) lo = mid + 1u;
        else hi = mid;
    }
    const uint32_t a = lo ? (lo - 1u) * S.step + 1u : 0u, b = lo < S.m ? lo * S.step : S.n;
    return fit_bound<OVER>(F.keys, a, b, k);
}

// fit_one for the segment `pre` (group, filter fields and, in the role-keyed table, the role): self 1 takes the query itself off.
static __device__ __forceinline__ void fitq_one(const FitParams& F, const FitSample& S, const unsigned long long* __restrict__ s_key,
                                                unsigned long long pre, int32_t rating, uint32_t self, bool want_gap,
                                                uint32_t& partners, uint32_t& gap)
{
    long long lo = (long long)rating - (long long)F.window, hi = (long long)rating + (long long)F.window;
    if (lo < -2147483648ll) lo = -2147483648ll;
    if (hi > 2147483647ll) hi = 2147483647ll;
    const uint32_t mine = fit_bias(rating);
    const uint32_t a = fitq_bound<false>(F, S, s_key, pre | fit_bias((int32_t)lo));
    const uint32_t b = fitq_bound<true>(F, S, s_key, pre | fit_bias((int32_t)hi));
    partners = b - a - self;
    gap = MM_NO_SLOT;
    if (!want_gap) return;
    const uint32_t e = fitq_bound<false>(F, S, s_key, pre | mine);
    const uint32_t f = fitq_bound<true>(F, S, s_key, pre | mine);
    if (f - e > self) { gap = 0u; return; }
    if (e > 0u) {
        const unsigned long long v = F.keys[e - 1u];
        if ((v >> 32) == (pre >> 32)) gap = dev_min_u32(mine - (uint32_t)v, 0xFFFFFFFEu);
    }
    if (f < S.n) {
        const unsigned long long v = F.keys[f];
        if ((v >> 32) == (pre >> 32)) gap = dev_min_u32(gap, dev_min_u32((uint32_t)v - mine, 0xFFFFFFFEu));
    }
}

// Is query i in the table itself?
static __device__ __forceinline__ uint32_t fitq_self(const FitQParams& Q, uint32_t i)
{
    return Q.same_mode && !(Q.where && (Q.where[i] & LOC_MARKED)) ? 1u : 0u;
}

// F.keys: the sorted table of in_mode, keyed as mm_partner_stats keys it.  A thread per query record, the workgroups
// stride over the records.
__global__ __launch_bounds__(WT_THREADS) void k_fit_query(FitQParams Q, FitParams F)
{
    __shared__ unsigned long long s_key[FITQ_SAMPLE];
    const FitSample S = fitq_stage(F, s_key);
    for (uint32_t i = blockIdx.x * WT_THREADS + threadIdx.x; i < Q.n; i += gridDim.x * WT_THREADS) {
        const uint4 q = Q.rec[i];
        if (q.z == MM_NO_SLOT) continue;
        uint32_t partners, gap;
        fitq_one(F, S, s_key, fit_prefix(q.z, q.y, F.eqmask), (int32_t)q.x, fitq_self(Q, i), Q.want_gap != 0u, partners, gap);
        Q.out[i] = partners;
        if (Q.want_gap) Q.out[(size_t)Q.stride + i] = gap;
    }
}

// by_role: the table is keyed with the role nibble in front of the filter fields (F.eqmask holds the role's bits, fit_prefix
// puts them at 44..47), so every role of in_mode is a segment of its own — by_role[r] is the count of the query's segment
// with role r in the role's place, partners the row's sum, gap the minimum over the roles; the query itself comes off its
// own role's segment only.
__global__ __launch_bounds__(WT_THREADS) void k_fit_query_role(FitQParams Q, FitParams F)
{
    __shared__ unsigned long long s_key[FITQ_SAMPLE];
    const FitSample S = fitq_stage(F, s_key);
    for (uint32_t i = blockIdx.x * WT_THREADS + threadIdx.x; i < Q.n; i += gridDim.x * WT_THREADS) {
        const uint4 q = Q.rec[i];
        if (q.z == MM_NO_SLOT) continue;
        const unsigned long long pre = fit_prefix(q.z, q.y, F.eqmask) & ~(0xFull << 44);
        const uint32_t self = fitq_self(Q, i), own = (q.y >> 16) & 0xFu;
        uint32_t sum = 0u, near = MM_NO_SLOT;
        for (uint32_t r = 0; r < Q.n_roles && r < MM_MAX_ROLES; ++r) {
            uint32_t partners, gap;
            fitq_one(F, S, s_key, pre | ((unsigned long long)r << 44), (int32_t)q.x, r == own ? self : 0u, Q.want_gap != 0u, partners, gap);
            Q.out[2u * (size_t)Q.stride + (size_t)i * MM_MAX_ROLES + r] = partners;
            sum += partners;
            near = dev_min_u32(near, gap);
        }
        Q.out[i] = sum;
        if (Q.want_gap) Q.out[(size_t)Q.stride + i] = near;
    }
}
