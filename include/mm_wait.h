/*
 * mm_wait.h — the engine's clock: arrival stamps, expiry of long-waiting players, wait times.
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
 * Not here: the NIF binding (native/mm_nif.c; INTEGRATION.md names the calls to add), widening
 * of a waiting player's window, moving an expired player to another mode.
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
 * intended one); ages are computed modulo 2^32, which is exact while nobody waits 2^31 units.
 * The clock does not go backwards: MM_ERR_RANGE (and nothing changes) when
 * (int32_t)(now - current) < 0.  The FIRST call switches the feature on: stamp[capacity] is
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

/* Entries [first, first + count) of the last mm_expire's list: the slot, its rating group and
 * the age it had reached.  Order: rating group ascending; within a group the stored lobby's
 * seats in the order mm_lobby_state lists them, then the queue from head to tail — the same on
 * every run, so an owner can publish its "no match found" replies from it.  Readable until the
 * next mm_expire, mm_reset or mm_restore.  Any output pointer may be NULL.
 * MM_ERR_RANGE: the range is not inside the list.  Reference: none. */
int mm_expired(mm_engine* e, uint32_t first, uint32_t count, uint32_t* slots, uint32_t* group,
               uint32_t* age);

/* per_group[cfg.n_groups]: who waits in `mode`, per rating group, and for how long.
 * MM_ERR_STATE: the clock was never set.
 * Reference: Search.Worker.status/0 (lib/search/worker.ex:115-117, :326-334), depth only. */
int mm_wait_stats(mm_engine* e, uint32_t mode, mm_wait_group* per_group);

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
