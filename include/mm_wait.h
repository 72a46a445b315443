/*
 * mm_wait.h — the engine's clock: arrival stamps, expiry of long-waiting players, their move to a
 * fallback mode — inside one engine or carried to another one with their rows and stamps — the
 * rotation of a blocked lobby's players to their queue's tail, wait times, a player's place in
 * its queue, how many waiting players fit a player and how far away the nearest one is, and expiry and moves that
 * select by that number.
 *
 * An extension of include/mm_engine.h (same rules: plain C types, status codes and never an
 * abort, every entry point selects the engine's HIP device itself, MM_ERR_STATE on an engine
 * whose tick failed half way).  It lives in a header of its own because the functions of
 * mm_engine.h are the ones the CPU oracle mirrors call for call (mo_*); nothing here needs a
 * mirror: an expiry is, by definition, an mm_cancel of a set of slots the device selects, so
 * the oracle checks it through mo_cancel.
 *
 * What this stands in for in the reference (paths relative to the reference's matchmaking/):
 * nothing it has.  The search path of OpenMatchmaking/microservice-matchmaking has no time-out —
 * a player nobody fits is requeued for ever (requeue_player/5, lib/search/worker.ex:239-248 ->
 * lib/requeue/worker.ex:51-54) — and the only view of a queue is its depth
 * (Search.Worker.status/0, lib/search/worker.ex:115-117, :326-334 -> AMQP.Queue.status).  A service
 * that wants "search timed out after 30 s" or "how long do people wait in diamond" keeps a table
 * of its own beside the broker; with the engine in between that table is already on the device
 * (the queues in order, the ActiveUser mirror, the stored lobbies), plus one stamp per slot.
 *
 * Everything is OFF until the owner sets the clock for the first time.  An engine that never
 * calls mm_clock_set allocates nothing for this, launches nothing for this and writes the same
 * snapshot as before.
 *
 * Widening a search is mm_move: after some seconds the owner gives up on the strict queue and the
 * device puts the player into a looser mode (a wider window, no region filter, "any role"), with
 * the stamp it had — so ages go on, tiers chain and the wait statistics tell the true wait.
 *
 * Carrying a player between engines is mm_move cut in two: mm_move_out selects and marks as mm_move
 * does and hands the rows out (mm_expired: slot, group, age; mm_moved_rows: rating, rewritten
 * constraint word, stamp), mm_enqueue_stamped takes rows in WITH their stamps.  The same two calls
 * re-queue the rest of a lobby whose ready check failed (stamp = clock at the tick - its
 * mm_matches_wait word) and refill an engine from redelivered messages that carry their own times.
 * On ONE engine mm_move_out + mm_enqueue_stamped of the same rows with their groups is mm_move word
 * for word — the same new slots (out_slot == mm_moved's column), the same queue order, the same
 * stamps: slot allocation steps over LIVE and CANCELLED slots alike, so marking the old slots before
 * or after the new ones are picked makes no difference.
 *
 * Un-blocking a chain is mm_rotate.  A chain has one open lobby and a tick ends with the first pass
 * that seats nobody (docs/MATCH_CHECK.md section 4), so an anchor nobody in the queue fits stalls
 * everybody behind it.  mm_rotate is mm_move onto the players' OWN chains, selected by the stored
 * lobbies instead of by age: the seats of every short-handed lobby with a queue behind it are marked
 * as mm_cancel marks them and the same players join the tail of their queue with the stamps they had.
 * The next tick drops the emptied lobby (the stale-lobby rule) and the queue's head anchors a new one.
 * No new matching rule: to the oracle it is mo_cancel plus mo_enqueue of the same rows.
 *
 * Answering a status request is mm_locate: where a slot stands in a mode right now — in which
 * rating group's queue and at which position, how many waiting players are ahead of it, for how
 * long it has waited, or that it sits in the stored lobby, or that a cancel or an expiry has marked
 * it already.  It reads what mm_queue_slots, mm_lobby_state and the stamps hold, on the device, in
 * one pass of mm_expire's walk, and changes nothing: it works with the clock off as well.
 *
 * Whether a player's wait can end at all is mm_partners.  A queue position does not predict a wait: a
 * chain is a first fit against one anchor (docs/MATCH_CHECK.md sections 2-4), so a player with 17 others
 * in front and nobody within its window waits for ever, and the player at the tail with a partner two
 * entries in front leaves in the next tick.  mm_partners counts, per queried slot, the waiting players of
 * its rating group — in its own mode or in another one, the fallback an mm_move rule would send it to —
 * that pass step 2 of match_check against it at a window and a set of filters the caller names, splits
 * the count by role and reports the distance to the nearest candidate, which is the window at which the
 * player would first have a partner.  It applies the existing predicate to a question, matches nobody
 * and changes nothing; the witness is numpy over the oracle's lists.
 *
 * What a chain looks like as a whole is mm_partner_stats: mm_partners' count and gap for EVERY waiting player of a mode,
 * aggregated per rating group — how many have nobody inside the window, how many have nobody of their region at all, the
 * histogram of gaps a window is chosen from.  Asking mm_partners about everybody costs pool x group length; this call
 * sorts in_mode's waiting players on the device once (a radix sort of one 64-bit key each) and answers every player
 * with binary searches.  Same predicate, same witness, nothing changes.
 *
 * Acting on that answer is mm_expire_if, mm_move_if and mm_move_out_if: the plain call's selection by age, kept only
 * where the player's partner count lies in a range the owner names (mm_partner_rule).  Age alone is the wrong rule for
 * a first-fit chain: an old player with forty partners inside its window leaves a queue that would have seated it in
 * the next tick, and a player with nobody in range sits out the full max_age for nothing.  No new matching rule: the
 * selection is mm_expire's list filtered by mm_partners' number, and everything after it is the plain call's.
 *
 * Not here: the NIF binding (native/mm_nif.c; INTEGRATION.md section 7 names the calls to add);
 * an ALL-OR-NOTHING move across engines (chain (A, g) and chain (B, g) of a ShardedSearch may have
 * different owners: mm_move_out has expired the players on their source before the destination's
 * mm_enqueue_stamped can answer MM_ERR_FULL, so a full destination loses them — sharding.py raises
 * on every rank); a device-pointer variant of mm_enqueue_stamped (mm_move and mm_rotate hand their
 * gathered stamps to the stamped scatter inside the engine); matching a waiting player against a wider window
 * INSIDE its own queue (a new matching rule, with no witness in the reference or the oracle — mm_partners
 * is the measurement such a decision would rest on: how many partners at window W, and nothing more);
 * mm_partners and the rule calls across two engines (chain (mode, g) and chain (in_mode, g) of a ShardedSearch
 * may have different owners: sharding.py raises for in_mode != mode).
 */
#ifndef MM_WAIT_H
#define MM_WAIT_H

#include "mm_engine.h"

#ifdef __cplusplus
extern "C" {
#endif

#define MM_WAIT_HIST 33u /* bucket 0: age 0; bucket 1 + floor(log2(age)) otherwise */

/* The waiting players of one (mode, rating group): the LIVE entries of the queue plus the LIVE
 * seats of the stored lobby (a cancelled or expired player that the next tick will drop is not
 * waiting).  Ages are (uint32_t)(clock - stamp).
 * Reference: Search.Worker.status/0 (lib/search/worker.ex:115-117, :326-334) sees the depth only. */
typedef struct mm_wait_group {
    uint32_t waiting;            /* players                                               */
    uint32_t oldest_age;         /* largest age among them (0 when nobody waits)          */
    uint64_t age_sum;            /* sum of their ages                                     */
    uint32_t hist[MM_WAIT_HIST]; /* players per age bucket                                */
    uint32_t pad;
} mm_wait_group;

/* Sets the engine's clock.  The unit is the owner's (milliseconds of a monotonic clock is the
 * intended one); ages are (uint32_t)(clock - stamp), exact for every wait below 2^32 units: an age
 * of 2^32 - 2 lands in histogram bucket 32 and is older than max_age = 2^32 - 3.  Only a single step
 * is limited: the clock does not go backwards, MM_ERR_RANGE (and nothing changes) when
 * (int32_t)(now - current) < 0, so one call advances it by 2^31 - 1 at the most (and a stamp handed
 * to mm_enqueue_stamped is at most 2^31 - 1 behind the clock).  The FIRST call switches the feature on: stamp[capacity] is
 * allocated, every player already waiting is stamped `now`, and from then on mm_enqueue and
 * mm_enqueue_device stamp every accepted player with the clock's value at the call.
 * Reference: none (the deliveries of lib/search/worker.ex:352-358 carry no arrival time). */
int mm_clock_set(mm_engine* e, uint32_t now);

/* *now = the clock, *enabled = 1 once mm_clock_set has been called (either may be NULL).
 * Host state only.  Reference: none. */
int mm_clock_get(const mm_engine* e, uint32_t* now, uint32_t* enabled);

/* Expires every waiting player of `mode` (see mm_wait_group) whose age is greater than max_age:
 * each is marked exactly as mm_cancel marks a slot, and with the same effect at the same time —
 * the start of the mode's next tick drops them from their queue, filters them out of the stored
 * lobby (remove_inactive_players/1, lib/search/worker.ex:267-280) and, where the head of a queue
 * was among them, applies the stale-lobby rule (docs/MATCH_CHECK.md section 4).
 * *n_expired (may be NULL) = how many; the list stays readable through mm_expired.
 * MM_ERR_STATE: the clock was never set.  MM_ERR_INVALID_ARG: no such mode.
 * Reference: none — the search path has no time-out; ActiveUser.remove_user/1
 * (lib/models/active_user.ex:57-66) is what each expiry amounts to. */
int mm_expire(mm_engine* e, uint32_t mode, uint32_t max_age, uint32_t* n_expired);

/* Entries [first, first + count) of the last mm_expire's, mm_move's, mm_move_out's or mm_rotate's list: the slot, its rating
 * group and the age it had reached.  Order: rating group ascending; within a group the stored lobby's
 * seats in the order mm_lobby_state lists them, then the queue from head to tail — the same on
 * every run, so an owner can publish its "no match found" replies from it.  Readable until the
 * next mm_expire, mm_move, mm_move_out, mm_rotate, mm_reset or mm_restore.  Any output pointer may be NULL.
 * MM_ERR_RANGE: the range is not inside the list.  Reference: none. */
int mm_expired(mm_engine* e, uint32_t first, uint32_t count, uint32_t* slots, uint32_t* group,
               uint32_t* age);

/* Moves every waiting player of `from_mode` whose age is greater than max_age into `to_mode`:
 * exactly the players mm_expire(from_mode, max_age) selects, in exactly its order (mm_expired
 * reads the list's slot, group and age columns afterwards, as after mm_expire).
 *   the old slot   is marked as mm_expire marks it: from_mode's next tick drops it, and until then
 *                  it is held — a move of k players needs k FREE slots beside them;
 *   the new entry  goes to the tail of chain (to_mode, the same rating group), in list order,
 *                  behind whoever is queued there, with the old rating and the constraint word
 *                  ((cons & ~cons_clear) & MM_CONS_USER_MASK & ~0xF) | to_mode, in a new slot taken
 *                  from the ring exactly as mm_enqueue takes them for a batch of *n_selected;
 *   the stamp      of the new slot is the old slot's: the player's age goes on.
 * A player to_mode cannot seat (role >= n_roles or a quota of 0 after cons_clear: mm_enqueue's
 * rule) is expired only: its new slot is MM_NO_SLOT, it uses up its ring position as a refused row
 * of mm_enqueue does, and it is counted in *n_refused.  *n_selected, *n_refused may be NULL.
 * MM_ERR_INVALID_ARG: no such mode, from_mode == to_mode, cons_clear with a bit outside
 * MM_CONS_USER_MASK or inside the mode nibble.  MM_ERR_STATE: the clock was never set.
 * MM_ERR_FULL: fewer FREE slots than selected players — all or nothing: nothing is marked, queues,
 * stamps, the ring position and the list of mm_expired (empty) are as if nobody had been selected.
 * Any other failure once the first mark may be on the device leaves the engine MM_ERR_STATE until
 * mm_reset / mm_restore, as for mm_expire.  Nothing of a move is in a snapshot that a pool of
 * queues, states and stamps does not already hold (versions 1 and 2 are unchanged).
 * Reference: none (a requeued player goes back to the queue it came from, requeue_player/5,
 * lib/search/worker.ex:239-248); to the oracle a move is mo_cancel of the old slots plus
 * mo_enqueue of the same rows. */
int mm_move(mm_engine* e, uint32_t from_mode, uint32_t to_mode, uint32_t max_age,
            uint32_t cons_clear, uint32_t* n_selected, uint32_t* n_refused);

/* Entries [first, first + count) of the last mm_move's or mm_rotate's list, fourth column: the new slot, or
 * MM_NO_SLOT for a refused player.  Range rule and lifetime as mm_expired (after an mm_expire the
 * column is empty).  Reference: none. */
int mm_moved(mm_engine* e, uint32_t first, uint32_t count, uint32_t* new_slot);

/* The first half of mm_move: selects exactly the players mm_expire(from_mode, max_age) selects, in
 * exactly its order, and marks them exactly as mm_expire does (from_mode's next tick drops them);
 * the list stays readable through mm_expired, and mm_moved_rows reads what an enqueue elsewhere
 * needs.  It takes no new slot and touches no other queue: never MM_ERR_FULL.  to_mode only goes
 * into the rewritten constraint word and may be a mode THIS engine does not have (the destination
 * may be another engine); mm_moved reads an empty column afterwards, as after mm_expire.
 * MM_ERR_INVALID_ARG: no such from_mode, to_mode >= MM_MAX_MODES, from_mode == to_mode, cons_clear
 * with a bit outside MM_CONS_USER_MASK or inside the mode nibble.  MM_ERR_STATE: the clock was never
 * set.  A failure once the first mark may be on the device leaves the engine MM_ERR_STATE until
 * mm_reset / mm_restore, as for mm_expire.  *n_selected may be NULL.
 * Reference: none (as mm_move); to the oracle it is mo_cancel of the listed slots. */
int mm_move_out(mm_engine* e, uint32_t from_mode, uint32_t to_mode, uint32_t max_age,
                uint32_t cons_clear, uint32_t* n_selected);

/* Entries [first, first + count) of the last mm_move_out's list, the rows: the rating, the
 * constraint word already rewritten to ((cons & ~cons_clear) & MM_CONS_USER_MASK & ~0xF) | to_mode,
 * and the stamp (the clock at the call minus the age mm_expired reports).  Range rule and lifetime
 * as mm_expired; the columns are empty after mm_expire, mm_move, mm_rotate, mm_reset and mm_restore.  Any
 * output pointer may be NULL.  Reference: none. */
int mm_moved_rows(mm_engine* e, uint32_t first, uint32_t count, int32_t* rating, uint32_t* cons,
                  uint32_t* stamp);

/* Rotates the blocked lobbies of `mode`.  For every rating group g, ascending: S = the LIVE seats of
 * the stored lobby of chain (mode, g) in mm_lobby_state's order, len = the queue length mm_queue_slots
 * reports at this moment (entries cancelled and not yet purged count).  The chain is selected iff
 * 1 <= |S| <= max_seated and len >= min_queue, and then ALL of S is: all seats of a chain or none.
 * The list is in mm_expire's order restricted to seats (group ascending, then S's order), and the
 * effect is exactly mm_move's with to_mode == from_mode and cons_clear == 0 over that selection:
 *   the old slot   is marked as mm_cancel marks it and held until the mode's next purge — a rotation
 *                  of k players needs k FREE slots beside them;
 *   the new entry  goes to the tail of the player's own chain, in list order, with its rating and
 *                  its constraint word unchanged and rating group g as the group override (a player
 *                  placed by override stays in its group), in a new slot taken from the ring exactly
 *                  as mm_enqueue takes them for a batch of *n_selected;
 *   the stamp      of the new slot is the old slot's: the player's age goes on.
 * Nobody can be refused (the mode seats them already).  mm_expired reads old slot, group and age,
 * mm_moved the new slots, mm_moved_rows reads empty; lifetime of the lists as after mm_move.  The
 * host mirrors end up as after mm_cancel plus mm_enqueue.  Nothing selected: MM_OK, *n_selected = 0,
 * no slot is taken, the lists are empty.  *n_selected may be NULL.
 * MM_ERR_INVALID_ARG: no such mode, max_seated == 0.  MM_ERR_STATE: the clock was never set.
 * MM_ERR_FULL: fewer FREE slots than selected players — all or nothing: nothing is marked, queues,
 * stamps, the ring position and the lists (empty) are as if nobody had been selected.  Any other
 * failure once the first mark may be on the device leaves the engine MM_ERR_STATE until mm_reset /
 * mm_restore, as for mm_move.  Nothing new goes into a snapshot; results never depend on mm_tuning.
 * Cost: no queue is streamed — at most n_groups x 32 seats are looked at, two waits on the stream
 * (one when nothing is selected).
 * Reference: none (requeue_player/5, lib/search/worker.ex:239-248, requeues the player that did NOT
 * fit, never the lobby it did not fit into); to the oracle a rotation is mo_cancel of the listed
 * slots plus mo_enqueue of the same rows with their groups. */
int mm_rotate(mm_engine* e, uint32_t mode, uint32_t max_seated, uint32_t min_queue,
              uint32_t* n_selected);

/* mm_enqueue (include/mm_engine.h) in every respect — slot choice, MM_ERR_FULL, the `group`
 * override, refused rows, out_slot, st — except that accepted player i is stamped stamp[i] instead
 * of the clock: its age is clock - stamp[i] from the start.  Nothing is written for a refused row.
 * MM_ERR_STATE: the clock was never set.  MM_ERR_INVALID_ARG: stamp == NULL with n > 0 (and
 * mm_enqueue's).  MM_ERR_RANGE, and nothing has changed: some (int32_t)(clock - stamp[i]) < 0 — a
 * stamp ahead of the clock would read as an age near 2^32 and expire at once.
 * Reference: none (the deliveries of lib/search/worker.ex:352-358 carry no arrival time). */
int mm_enqueue_stamped(mm_engine* e, uint32_t n, const int32_t* rating, const uint32_t* cons,
                       const uint8_t* group, const uint32_t* stamp, uint32_t* out_slot,
                       mm_enqueue_stats* st);

/* per_group[cfg.n_groups]: who waits in `mode`, per rating group, and for how long.
 * MM_ERR_STATE: the clock was never set.
 * Reference: Search.Worker.status/0 (lib/search/worker.ex:115-117, :326-334), depth only. */
int mm_wait_stats(mm_engine* e, uint32_t mode, mm_wait_group* per_group);

#define MM_AT_NONE   0u /* not in this mode: free, matched, never handed out, >= capacity, or waiting in another mode */
#define MM_AT_QUEUE  1u /* an entry of the queue of (mode, group)                                                      */
#define MM_AT_LOBBY  2u /* a seat of the stored lobby of (mode, group)                                                 */
#define MM_AT_MARKED 4u /* or-ed in: cancelled / expired / moved / rotated, still listed until the mode's next tick drops it */

/* mm_wait_route.route: how the last mm_partners / rule call counted its partners (mm_wait_route_get, below) */
#define MM_ROUTE_NONE   0u /* the last such call counted nothing (n == 0, no output asked for, nobody old enough, refused) */
#define MM_ROUTE_TILES  1u /* every query against every entry of its rating group                                          */
#define MM_ROUTE_SORTED 2u /* binary searches in a sorted table of in_mode's waiting players (mm_partner_stats' table)     */

/* Where slots[i] stands in `mode` at this moment, for i < n; each output column has n words and any
 * of them may be NULL.
 *   where     MM_AT_QUEUE or MM_AT_LOBBY, with MM_AT_MARKED or-ed in when the slot is no longer LIVE
 *             (marked by mm_cancel, mm_expire, mm_move, mm_move_out or mm_rotate and not yet dropped);
 *             MM_AT_NONE when the slot is in no queue and no stored lobby of this mode.
 *   group     the rating group of the chain; MM_NO_SLOT for NONE.
 *   position  QUEUE: the index in the list mm_queue_slots(mode, group) returns, head = 0 (entries
 *             cancelled and not yet purged count, as they do there); LOBBY: the index in
 *             mm_lobby_state's list; MM_NO_SLOT for NONE.
 *   ahead     QUEUE: the LIVE entries at smaller positions of the same queue — what a client shows
 *             (the same definition for a MARKED entry); LOBBY and NONE: 0.
 *   age       clock - stamp[slot] for every slot found, MARKED ones included; 0 for NONE, and 0
 *             everywhere while the clock was never set (the call does not switch it on).
 * A slot may be queried more than once: each occurrence gets the same answer.  A slot >= capacity
 * is NONE.  n == 0: MM_OK, nothing is launched.
 * Read-only: no queue, lobby, state, stamp, host mirror or ring position changes, the lists of
 * mm_expired / mm_moved / mm_moved_rows stay as they are, a snapshot taken after the call is byte
 * for byte the one taken before it; results never depend on mm_tuning.  An engine that never calls
 * it allocates and launches nothing for it.
 * MM_ERR_INVALID_ARG: e == NULL, no such mode, slots == NULL with n > 0, n > capacity.
 * MM_ERR_STATE: the engine is poisoned by a failed tick.  MM_ERR_HIP / MM_ERR_OOM do NOT poison
 * the engine (nothing was marked); the call's scratch is released and the next call starts afresh.
 * Cost: two streams of the mode's queues (one when ahead == NULL) with two gathers per entry, one
 * wait on the stream; nothing proportional to the capacity after the first call.
 * Reference: Search.Worker.status/0 (lib/search/worker.ex:115-117, :326-334), depth only. */
int mm_locate(mm_engine* e, uint32_t mode, uint32_t n, const uint32_t* slots, uint32_t* where,
              uint32_t* group, uint32_t* position, uint32_t* ahead, uint32_t* age);

/* How many waiting players fit slots[i], for i < n, and how far away the nearest one is.  Any of the three outputs
 * may be NULL, and a column that is not asked for costs nothing on the device.
 *   the query player p   the player in slots[i], where mm_locate(mode) would find it: an entry of a queue or a seat of a
 *                        stored lobby of `mode`, a MARKED one included.  g is the rating group of that chain (for a player
 *                        placed by the `group` override too: mm_move's rule); p's rating and constraint word are the ones
 *                        the engine holds — the queue entry's, or the seat's in the stored lobby.
 *   the candidates W     the waiting players of chain (in_mode, g) in mm_wait_group's sense: the LIVE entries of the queue
 *                        plus the LIVE seats of the stored lobby.  p's own slot is never a candidate.  in_mode may be mode.
 *   the predicate        step 2 of match_check (docs/MATCH_CHECK.md) with p in the anchor's place, at the `window` and
 *                        `flags` passed: W fits iff |W.rating - p.rating| <= window, and MM_MODE_REGION_FILTER => equal
 *                        regions, and MM_MODE_PARTY_FILTER => equal parties.  The difference is exact for any two int32
 *                        ratings, `window` is a full uint32_t, the predicate is symmetric.  cfg.modes[in_mode].window and
 *                        .flags ask about in_mode as it matches; any other value asks "what if".
 *   partners[i]          the candidates that fit.
 *   by_role[i * MM_MAX_ROLES + r]   the same count split by MM_CONS_ROLE(W.cons); the row sums to partners[i].
 *   gap[i]               the smallest |W.rating - p.rating| over the candidates that pass the two FLAG filters, the window
 *                        ignored: the window at which p would first have a partner.  Saturates at 0xFFFFFFFE;
 *                        MM_NO_SLOT: there is none.
 * A slot mm_locate would answer with MM_AT_NONE in `mode` (a slot >= capacity is one) gets partners 0, a zero by_role
 * row and gap MM_NO_SLOT.  A slot queried more than once gets the same answer each time.  n == 0, or all
 * three outputs NULL: MM_OK, nothing is launched.
 * Read-only, exactly as mm_locate: no queue, lobby, state, stamp, host mirror or ring position changes, the lists of
 * mm_expired / mm_moved / mm_moved_rows stay as they are, a snapshot taken after the call is byte for byte the one taken
 * before it; results never depend on mm_tuning; it works with the clock off.  An engine that never calls it allocates
 * and launches nothing for it.
 * MM_ERR_INVALID_ARG: e == NULL, no such mode or in_mode, a `flags` bit outside the two MM_MODE_* filters, slots == NULL
 * with n > 0, n > capacity.  MM_ERR_STATE: the engine is poisoned by a failed tick.  MM_ERR_HIP / MM_ERR_OOM do NOT
 * poison the engine; the call's scratch (and mm_locate's) is released and the next call starts afresh.
 * Cost: mm_locate's with ahead == NULL (one stream of mode's queues, four small launches), one thread per query to
 * build its record, then the count by one of two routes (mm_wait_route_get says which; the columns are the same words):
 *   tiles    one stream of in_mode's queues (slot, rating, constraint word, one gather of state[]) per tile of 512
 *            queries, each query tested against the entries of its own rating group only: queries x group length
 *            predicate tests in all;
 *   sorted   mm_partner_stats' table of in_mode — two streams of its queues and the radix passes, one more pass and
 *            the role in the key when by_role is asked for — then four binary searches per query (per query and role
 *            for by_role), each narrowed in a sample of the table held in LDS; 16 bytes of scratch per key.  Its cost
 *            is the table's, nearly whatever n is.
 * The sorted route is taken iff mm_tuning.wait_sort_mtests != 0xFFFFFFFF and n x bound >= wait_sort_mtests << 20,
 * bound = min(players queued in ALL modes, entries not yet purged included; capacity) — a crude upper bound of in_mode's
 * waiting players, the one the host knows without asking the device.  One wait on the stream either way; nothing
 * proportional to the capacity after the first call.
 * Reference: none.  Search.Worker.status/0 (lib/search/worker.ex:115-117, :326-334) sees the depth only. */
int mm_partners(mm_engine* e, uint32_t mode, uint32_t in_mode, uint32_t window, uint32_t flags, uint32_t n,
                const uint32_t* slots, uint32_t* partners, uint32_t* by_role, uint32_t* gap);

#define MM_PARTNER_HIST 33u /* bucket 0: value 0; bucket 1 + floor(log2(value)) otherwise, as MM_WAIT_HIST */

/* mm_partners' two words over every waiting player of one chain (mode, rating group), aggregated. */
typedef struct mm_partner_group {      /* 304 bytes */
    uint32_t waiting;                  /* the queries: waiting players of chain (mode, g)                       */
    uint32_t candidates;               /* waiting players of chain (in_mode, g)                                 */
    uint32_t alone;                    /* queries with partners == 0                                            */
    uint32_t unreachable;              /* queries with gap == MM_NO_SLOT: no candidate passes the flag filters  */
    uint64_t partners_sum;             /* sum of partners over the queries                                      */
    uint64_t gap_sum;                  /* sum of gap over the queries that have one                             */
    uint32_t partners_max;
    uint32_t gap_max;                  /* 0 when no query has a gap                                             */
    uint32_t partners_hist[MM_PARTNER_HIST];  /* every query, by its partners                                   */
    uint32_t gap_hist[MM_PARTNER_HIST];       /* the queries that have a gap, by it; sums to waiting - unreachable */
} mm_partner_group;

/* per_group[cfg.n_groups]: what a chain looks like as a whole.  For every rating group g the queries are the waiting
 * players of chain (mode, g) in mm_wait_group's sense — the LIVE queue entries plus the LIVE seats of the stored lobby; a
 * MARKED player is neither a query nor a candidate — and for each query p, partners(p) and gap(p) are exactly the two
 * words mm_partners(e, mode, in_mode, window, flags, 1, &p.slot, &partners, NULL, &gap) returns on the same pool: p is
 * never its own partner, differences are exact for any two int32 ratings, `window` is a full uint32_t, gap saturates at
 * 0xFFFFFFFE, rating and constraint word are the ones the engine holds, a player placed by the `group` override belongs
 * to the chain it sits in.  The record of g is the aggregate of those words over the queries of g.
 * Read-only, exactly as mm_locate and mm_partners: nothing of the pool, the host mirrors or the lists of mm_expired /
 * mm_moved / mm_moved_rows changes, a snapshot taken after the call is byte for byte the one taken before it; it works
 * with the clock off; results never depend on mm_tuning.  An engine that never calls it allocates and launches nothing
 * for it.  Nobody waiting: MM_OK and zeroed records.
 * MM_ERR_INVALID_ARG: e == NULL, per_group == NULL, no such mode or in_mode, a `flags` bit outside the two MM_MODE_*
 * filters.  MM_ERR_STATE: the engine is poisoned by a failed tick.  MM_ERR_HIP / MM_ERR_OOM do NOT poison the engine;
 * the call's scratch is released and the next call starts afresh.
 * Cost: no step is queries x group length.  Two streams of in_mode's queues write one 64-bit key per waiting candidate
 * (rating group | the fields the filters compare | rating in unsigned order), an LSD radix sort of the keys on the
 * device — four passes for the rating, one more for each filter set and one when there is more than one rating group,
 * three launches a pass — then one stream of mode's queues with four binary searches per waiting player; 16 bytes of
 * scratch per key, grown to the longest call so far; one wait on the stream.
 * Reference: none.  Search.Worker.status/0 (lib/search/worker.ex:115-117, :326-334) sees the depth only. */
int mm_partner_stats(mm_engine* e, uint32_t mode, uint32_t in_mode, uint32_t window, uint32_t flags,
                     mm_partner_group* per_group);

/* Which of the players old enough a rule call selects: those whose partner count lies in a range. */
typedef struct mm_partner_rule {
    uint32_t in_mode;       /* whose chains are searched: chain (in_mode, g), g the player's rating group        */
    uint32_t window, flags; /* mm_partners' predicate: |rating difference| <= window, MM_MODE_* filters          */
    uint32_t min_partners;  /* selected iff min_partners <= partners <= max_partners                             */
    uint32_t max_partners;
} mm_partner_rule;

/* mm_expire, mm_move and mm_move_out with a second condition.  Player p is selected iff
 *   mm_expire(mode, max_age) — from_mode for the moves — would select p, AND
 *   the `partners` word mm_partners(mode, rule->in_mode, rule->window, rule->flags, 1, &p.slot, ..) would return lies
 *   in [rule->min_partners, rule->max_partners],
 * both on the pool as it stands when the call enters: a candidate this same call goes on to select still counts (two old
 * players in range of each other are each other's partners, and with max_partners == 0 both stay), so the selection
 * does not depend on any order.  mm_partners' rules hold unchanged: p is never its own partner, MARKED candidates do
 * not count, p's rating and constraint word are the ones the engine holds — the un-rewritten word, whatever cons_clear
 * says — and the seats of stored lobbies are queries and candidates alike.
 * The list is mm_expire's order restricted to the selected players, and everything from there on is the plain call's,
 * word for word: the marks, the host mirrors, mm_expired / mm_moved / mm_moved_rows and their lifetimes, the new slots
 * "as mm_enqueue takes them for a batch of *n_selected", the stamps carried over, the refused rows, and MM_ERR_FULL all
 * or nothing — judged on the number finally selected, not on the number old enough.
 * With [0, 0xFFFFFFFF] each call is its plain call.  The two intended uses:
 *   in_mode == from_mode, [0, 0], the mode's own window and flags            "nobody here fits me";
 *   in_mode == to_mode, [1, 0xFFFFFFFF], the destination's window and flags  "move only where someone fits".
 * MM_ERR_INVALID_ARG: the plain call's cases, rule == NULL, rule->in_mode >= n_modes, a flags bit outside the two
 * MM_MODE_* filters, min_partners > max_partners.  MM_ERR_STATE: as the plain call.  A failure before the first mark
 * leaves the engine usable and, MM_ERR_FULL apart, releases the call's scratch as mm_partners does; from the first mark
 * on it leaves the engine MM_ERR_STATE until mm_reset / mm_restore, as for the plain call.  An engine that never calls
 * them allocates and launches nothing for them; results never depend on mm_tuning; nothing new goes into a snapshot.
 * Cost: the plain call's age count, then — only when somebody is old enough — one more stream of from_mode's queues that
 * writes a record per candidate and marks nothing, the partner count by one of mm_partners' two routes — tiles: one
 * stream of in_mode's queues per tile of 512 candidates (candidates x group length predicate tests); sorted: the table
 * of in_mode and four binary searches per candidate; chosen by mm_partners' rule with the number old enough for n —
 * then a count, a scan and a scatter over the candidates.
 * Scratch is mm_partners', sized by the candidates (and the table's on the sorted route).  Waits on the stream: mm_move_if three at the most (the candidates,
 * the selected — before anything is marked, for MM_ERR_FULL — and the lists); mm_expire_if and mm_move_out_if two
 * (nobody can be refused, so the selected count comes back with the lists); one when nobody is old enough.
 * Reference: none (as mm_expire, mm_move, mm_move_out); to the oracle the effect is mo_cancel plus mo_enqueue. */
int mm_expire_if(mm_engine* e, uint32_t mode, uint32_t max_age, const mm_partner_rule* rule, uint32_t* n_expired);
int mm_move_if(mm_engine* e, uint32_t from_mode, uint32_t to_mode, uint32_t max_age, uint32_t cons_clear,
               const mm_partner_rule* rule, uint32_t* n_selected, uint32_t* n_refused);
int mm_move_out_if(mm_engine* e, uint32_t from_mode, uint32_t to_mode, uint32_t max_age, uint32_t cons_clear,
                   const mm_partner_rule* rule, uint32_t* n_selected);

/* Which route the engine's last mm_partners / mm_expire_if / mm_move_if / mm_move_out_if took to its partner counts, and
 * what the choice was made on.  Size-versioned like mm_path_stats; host state only — no device call — and diagnostics
 * only: the route never changes a result.  MM_ERR_INVALID_ARG: e or out NULL, out->size < 8. */
typedef struct mm_wait_route {
    uint32_t size;       /* in: caller's sizeof; out: bytes filled */
    uint32_t call;       /* 1 mm_partners, 2 mm_expire_if, 3 mm_move_if, 4 mm_move_out_if; 0: none yet */
    uint32_t route;      /* MM_ROUTE_* */
    uint32_t queries, bound, threshold;   /* what the choice was made on: n or the number old enough, the bound above, wait_sort_mtests */
    uint32_t keys;       /* SORTED: the table's length; else 0 */
    uint32_t passes;     /* SORTED: radix passes run; else 0 */
} mm_wait_route;
int mm_wait_route_get(mm_engine* e, mm_wait_route* out);

/* How long the players of the last tick's lobbies had waited: L = teams * team_size words per
 * match, laid out like mm_matches' `slots`; each word is the clock at that tick minus the seated
 * player's stamp.  Computed at the end of mm_tick (a matched slot is free afterwards and a later
 * enqueue stamps it again), only while the clock is on; readable until the next mm_tick / mm_reset.
 * MM_ERR_STATE: the clock was never set.  MM_ERR_RANGE: the range is outside the last tick's list
 * (also when that tick ran before the clock was set).
 * Reference: none (the published lobby of lib/search/worker.ex:313-319 carries no times). */
int mm_matches_wait(mm_engine* e, uint32_t first, uint32_t count, uint32_t* wait);

#ifdef __cplusplus
}
#endif
#endif /* MM_WAIT_H */
