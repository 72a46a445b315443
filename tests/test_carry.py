"""mm_move_out, mm_moved_rows and mm_enqueue_stamped (include/mm_wait.h) on the CPU shim: a waiting player leaves one
engine with its row and its arrival stamp and joins another one with them.  The reference has nothing of the kind (a
requeued player goes back to the queue it came from, requeue_player/5, lib/search/worker.ex:239-248, and no delivery
carries an arrival time, :352-358); the witness is the header's equivalence — on one engine the two calls ARE mm_move —
with mm_move itself held against the unchanged oracle (tests/carry_scenarios.py).  The same drivers run on the GPU in
tests/test_gpu_carry.py."""
import numpy as np
import pytest

from carry_scenarios import (ONE_GROUP, RANK_WEIGHTS, RankFailure, _rank_status, carry_engine, carry_route, full_pool, full_worker, leaving_worker, lobby_requeue,
                             one_engine, rank_script, rows_cases, script_worker, spawn, stamped_edges, stamped_plain,
                             stamped_refused, stamped_ring, stamps_of, stream_cfg, stream_run, stream_worker, twin_script)
from emu_engine import EmuEngine, EmuEngineSmall
from microservice_matchmaking_amd import MMError
from microservice_matchmaking_amd._abi import NO_SLOT
from microservice_matchmaking_amd.config import make_config, mode_1v1
from microservice_matchmaking_amd.sharding import ChainSharding, ShardedSearch, union_digest
from move_scenarios import (MM_ERR_FULL, MM_ERR_INVALID_ARG, MM_ERR_RANGE, MM_ERR_STATE, ROLE_MASK, bucket_lengths,
                            four_mode_config, move_script, pool)

ENGINES = [EmuEngine, EmuEngineSmall]
ids = dict(ids=lambda c: c.__name__)


# ---- 1. twin engines: mm_move on A, mm_move_out + mm_moved_rows + mm_enqueue_stamped on B -------------------------------

@pytest.mark.parametrize("engine_cls", ENGINES, **ids)
@pytest.mark.parametrize("seed", [5, 6])
def test_twin_engines_the_two_call_route_is_mm_move(oracle_cls, engine_cls, seed):
    moved, refused, lobbies = twin_script(engine_cls, oracle_cls, seed=seed, restart_at=(3,))
    assert moved > 100 and lobbies[2] > 5 and lobbies[3] > 5


def test_the_move_script_itself_runs_on_the_two_call_route(oracle_cls):
    """tests/move_scenarios.py's own script, every check of it, with `move` replaced by the route: the same log."""
    assert move_script(carry_engine(EmuEngineSmall), oracle_cls, seed=7, restart_at=(2,)) == \
        move_script(EmuEngineSmall, oracle_cls, seed=7, restart_at=(2,))


# ---- 2. the rows ---------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("engine_cls", ENGINES, **ids)
def test_moved_rows_are_the_owners_table(oracle_cls, engine_cls):
    done = rows_cases(engine_cls, oracle_cls)
    assert [x[0] for x in done] == ["anchor", "anchor", "before the clock", "wrap", "foreign mode"]


# ---- 3. the stamped enqueue on its own -----------------------------------------------------------------------------------

@pytest.mark.parametrize("engine_cls", ENGINES, **ids)
@pytest.mark.parametrize("behind", [False, True], ids=["empty", "behind"])
def test_stamps_of_mixed_ages(oracle_cls, engine_cls, behind):
    stamped_plain(engine_cls, oracle_cls, behind)


@pytest.mark.parametrize("engine_cls", ENGINES, **ids)
def test_a_waiting_player_inside_the_ring_range_the_stamp_follows_the_slot(oracle_cls, engine_cls):
    stamped_ring(engine_cls, oracle_cls, True)


@pytest.mark.parametrize("engine_cls", ENGINES, **ids)
def test_the_ring_wraps_inside_the_batch(oracle_cls, engine_cls):
    stamped_ring(engine_cls, oracle_cls, False)


@pytest.mark.parametrize("engine_cls", ENGINES, **ids)
def test_refused_rows_get_no_stamp(oracle_cls, engine_cls):
    assert stamped_refused(engine_cls, oracle_cls) > 0


@pytest.mark.parametrize("engine_cls", ENGINES, **ids)
@pytest.mark.parametrize("which", range(6))
def test_batch_sizes_at_the_bucketing_edges(oracle_cls, engine_cls, which):
    w, c = bucket_lengths()
    sizes = [w - 1, w, w + 1, c - 1, c, c + 1]
    assert sizes[3] > sizes[2]
    assert stamped_edges(engine_cls, oracle_cls, [sizes[which]]) == [sizes[which]]


@pytest.mark.parametrize("engine_cls", ENGINES, **ids)
def test_the_rest_of_a_lobby_comes_back_with_its_wait(oracle_cls, engine_cls):
    lobby_requeue(engine_cls, oracle_cls)


# ---- 4. errors -----------------------------------------------------------------------------------------------------------

def _status(fn, *args, **kw):
    with pytest.raises(MMError) as ei:
        fn(*args, **kw)
    return ei.value.status


@pytest.mark.parametrize("engine_cls", ENGINES, **ids)
def test_clock_off_and_argument_errors(engine_cls):
    with engine_cls(four_mode_config()) as a:
        rating, cons = pool(300, 91, 2, 5)
        a.enqueue(rating, cons)
        stamp = np.zeros(300, np.uint32)
        assert _status(a.enqueue_stamped, rating, cons, stamp) == MM_ERR_STATE        # the clock was never set
        assert _status(a.move_out, 2, 3, 0, ROLE_MASK) == MM_ERR_STATE
        a.clock_set(1000)
        assert _status(a.move_out, 4, 3, 0, 0) == MM_ERR_INVALID_ARG                  # no such from_mode
        assert _status(a.move_out, 2, 16, 0, 0) == MM_ERR_INVALID_ARG                 # to_mode >= MM_MAX_MODES
        assert _status(a.move_out, 2, 2, 0, 0) == MM_ERR_INVALID_ARG                  # from_mode == to_mode
        for bad in (1 << 20, 0x80000000, 0x1, ROLE_MASK | 0x8):                       # outside the user mask, inside the mode nibble
            assert _status(a.move_out, 2, 3, 0, bad) == MM_ERR_INVALID_ARG
        assert int(a.queue_depth(2).sum()) == 300 and all(w["waiting"] == 0 for w in a.wait_stats(3))
        # NULL stamp, bad group
        f = a._fn("enqueue_stamped")
        from microservice_matchmaking_amd._abi import _ptr
        assert f(a._h, 300, _ptr(rating), _ptr(cons), None, None, None, None) == MM_ERR_INVALID_ARG
        assert f(a._h, 0, None, None, None, None, None, None) == 0
        assert _status(a.enqueue_stamped, rating, cons, stamp, np.full(300, 7, np.uint8)) == MM_ERR_INVALID_ARG
        assert a.enqueue(*pool(1, 92, 0)).tolist() == [300]                           # nothing took a slot
        a.clock_set(1001)
        got = a.move_out(2, 15, 0, ROLE_MASK | (0xFF << 4))                           # region and role cleared, a foreign mode: legal
        assert got[0].size == 300 and ((got[4] & 0xF) == 15).all() and (got[4] >> 4 == 0).all() and (got[5] == 1000).all()
        for first, count in ((300, 1), (0, 301), (301, 0)):
            assert a._fn("moved_rows")(a._h, first, count, None, None, None) == MM_ERR_RANGE
        assert a._fn("moved_rows")(a._h, 0, 300, None, None, None) == 0
        assert a.expire(0, 5)[0].size == 0
        assert a._fn("moved_rows")(a._h, 0, 1, None, None, None) == MM_ERR_RANGE      # empty after mm_expire
        a.enqueue(*pool(50, 93, 0))
        a.clock_set(1002)
        assert a.move_out(0, 1, 0)[0].size == 51
        assert a._fn("moved_rows")(a._h, 0, 51, None, None, None) == 0
        assert a.move(2, 3, 0, ROLE_MASK)[0].size == 0
        assert a._fn("moved_rows")(a._h, 0, 1, None, None, None) == MM_ERR_RANGE      # ... and after mm_move
        assert a.move_out(1, 0, 0)[0].size == 0
        a.reset()
        assert a._fn("moved_rows")(a._h, 0, 1, None, None, None) == MM_ERR_RANGE


@pytest.mark.parametrize("engine_cls", ENGINES, **ids)
def test_a_stamp_ahead_of_the_clock_is_refused_and_nothing_has_changed(engine_cls):
    cfg = four_mode_config()
    with engine_cls(cfg) as a, engine_cls(cfg) as twin:
        for e in (a, twin):
            e.clock_set(5000)
            e.enqueue(*pool(700, 94, 2, 5))
        rating, cons = pool(200, 95, 3, 1)
        stamp = np.full(200, 4000, np.uint32)
        stamp[137] = 5001
        depth, before = [a.queue_depth(md).tolist() for md in range(4)], stamps_of(a)
        assert _status(a.enqueue_stamped, rating, cons, stamp) == MM_ERR_RANGE
        stamp[137] = 5000 + (1 << 31)                                                 # half the ring away still counts as ahead
        assert _status(a.enqueue_stamped, rating, cons, stamp) == MM_ERR_RANGE
        assert [a.queue_depth(md).tolist() for md in range(4)] == depth and np.array_equal(stamps_of(a), before)
        nxt = pool(30, 96, 0)
        assert np.array_equal(a.enqueue(*nxt), twin.enqueue(*nxt))                    # the ring is where it was
        stamp[137] = 5000                                                             # the clock itself is not ahead
        s = a.enqueue_stamped(rating, cons, stamp)
        assert np.array_equal(s, twin.enqueue(rating, cons)) and np.array_equal(stamps_of(a)[s], stamp)
    with engine_cls(cfg) as a:
        a.clock_set(0xFFFFFFF0)
        a.clock_set(0x10)                                                             # across 2^32: a stamp from before the wrap is behind
        s = a.enqueue_stamped(rating[:2], cons[:2], np.asarray([0xFFFFFF00, 0x10], np.uint32))
        assert a.expire(3, 0x10)[2].tolist() == [0x110]
        assert _status(a.enqueue_stamped, rating[:1], cons[:1], np.asarray([0x11], np.uint32)) == MM_ERR_RANGE


@pytest.mark.parametrize("engine_cls", ENGINES, **ids)
def test_a_full_pool_refuses_the_stamped_batch_and_nothing_has_changed(oracle_cls, engine_cls):
    full_pool(engine_cls, oracle_cls)


@pytest.mark.parametrize("engine_cls", ENGINES, **ids)
def test_a_poisoned_engine_answers_state(engine_cls):
    with engine_cls(four_mode_config(), {"fail_tick": 1}) as a:
        a.clock_set(1)
        rating, cons = pool(300, 92, 2, 5)
        a.enqueue(rating, cons)
        with pytest.raises(MMError):
            a.tick(2)
        assert _status(a.move_out, 2, 3, 0, ROLE_MASK) == MM_ERR_STATE
        assert _status(a.enqueue_stamped, rating, cons, np.ones(300, np.uint32)) == MM_ERR_STATE
        assert a._fn("moved_rows")(a._h, 0, 0, None, None, None) == MM_ERR_STATE
        a.reset()
        a.clock_set(2)
        assert a.move_out(2, 3, 0, ROLE_MASK)[0].size == 0
        assert (a.enqueue_stamped(rating, cons, np.ones(300, np.uint32)) != NO_SLOT).all()


# ---- 5. ranks over gloo --------------------------------------------------------------------------------------------------

def _merge(gathered):
    got = {}
    for res in gathered:
        assert not (set(res["digests"]) & set(got))              # every chain has exactly one owner
        got.update(res["digests"])
    return got


@pytest.mark.timeout(600)
@pytest.mark.parametrize("world", [2, 4])
def test_ranks_move_across_engines_like_one_engine(world):
    own = ChainSharding(4, 7, world, RANK_WEIGHTS[world]).chain_owner
    assert (own[2] != own[3]).any() and (own[2] == own[3]).any()     # both kinds of move: to another rank, and at home
    gathered, owner = spawn(script_worker, world, ("emu",))
    assert owner == own.tolist()
    want = one_engine(EmuEngineSmall, four_mode_config(), rank_script)
    got = _merge(gathered)
    assert set(got) == set(want["digests"]) and union_digest(got) == union_digest(want["digests"])
    for k in ("selected", "refused", "taken", "expired"):
        assert sum(r[k] for r in gathered) == want[k], (k, [r[k] for r in gathered], want[k])
    assert want["selected"] > 100 and want["taken"] > 100
    for md in range(4):
        assert np.array_equal(np.sort(np.concatenate([r["waits"][md] for r in gathered])), want["waits"][md]), md
    assert want["waits"][3].size > 0 and want["waits"][2].size > 0


@pytest.mark.timeout(600)
def test_the_five_role_stream_widens_on_two_ranks():
    gathered, owner = spawn(stream_worker, 2, ("emu",))
    own = np.asarray(owner)
    assert (own[0] != own[1]).any() and (own[0] == own[1]).any()
    want = one_engine(EmuEngineSmall, stream_cfg(), stream_run)
    got = _merge(gathered)
    assert union_digest(got) == union_digest(want["digests"])
    assert [sum(r["moved"][0] for r in gathered)] == want["moved"] and want["moved"][0] > 0
    assert [sum(r["refused"][0] for r in gathered)] == want["refused"]
    assert sum(r["matched"] for r in gathered) == want["matched"] > 0
    assert all(r["full_at_s"] is None for r in gathered) and want["full_at_s"] is None
    for md in range(2):
        assert np.array_equal(np.sort(np.concatenate([r["wait_ms"][md] for r in gathered])), want["wait_ms"][md]), md
    assert want["wait_ms"][1].size > 0 and want["wait_ms"][1].max() > 50      # seated in the fallback after waiting in the strict mode


@pytest.mark.timeout(300)
def test_a_destination_rank_without_room_raises_on_every_rank():
    """(the spawn's join is the guard: a rank that did not raise would wait for the others in its next collective)"""
    gathered = spawn(full_worker, 2, ("emu",), timeout=200)
    assert [g[0] for g in gathered] == [MM_ERR_FULL, MM_ERR_FULL]
    assert gathered[0][1] == [1500, 0] and gathered[1][1] == [0, 1000]       # the destination took nothing
    assert gathered[0][2] == 0                                               # ... and the source had expired its players: not all-or-nothing


def test_a_rank_that_leaves_early_is_noticed_and_reported_with_a_status():
    """What tests/carry_gpu_worker.py exits with when a rank of its two-rank scenario ends badly: spawn does not wait for the
    time limit while the other rank sits in a collective, and a signal becomes one of the statuses the GPU test stops on."""
    with pytest.raises(RankFailure) as ei:
        spawn(leaving_worker, 2, (3,), timeout=120)
    assert ei.value.status == 1 and "(1, 3)" in str(ei.value)
    assert [_rank_status(c) for c in (3, -6, -9, -11, -7)] == [1, 134, 137, 139, 139]


def test_one_rank_still_moves_through_mm_move(oracle_cls):
    with ShardedSearch(four_mode_config(), EmuEngineSmall, 0, 1) as one:
        one.engine.clock_set(5)
        one.enqueue(*pool(500, 97, 2, 5))
        one.engine.clock_set(9)
        got = one.move(2, 3, 0, ROLE_MASK)
        assert got[0].size == 500 and (got[3] != NO_SLOT).all() and not hasattr(one, "last_move")
        assert np.array_equal(one.local_to_global[got[3].astype(np.int64)], one.local_to_global[got[0].astype(np.int64)])
